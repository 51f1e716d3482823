"""Rules N1-N9 of DESIGN.md 8r in Python integers and Python floats, written independently of the device code: the stand-in the
device's top-down raster is compared with, bit for bit.

N3: a face takes part iff its indices lie in [0, V), its three z are finite and the exact doubled area of its snapped triangle is
not 0; the others are counted under their first cause in that order.  N4: the centre (65536 col + 32768, 65536 row + 32768) belongs
to a face under Z3 (`zonal_standin.centre_in_rings`, pinned by hand-worked cases) on the triangle as a ring of three vertices.
N5: the height is a chain of Python float operations -- IEEE float64, each rounded on its own --, in the stated order.  N6: the
greatest key of the height's bit pattern wins, equal keys go to the lowest face: a plain double loop in ascending face order that
replaces the winner on a strictly greater key."""
import math
import struct
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))

from crs_standin import CrsStandinBackend  # noqa: E402
from zonal_standin import HALF, ONE, centre_in_rings  # noqa: E402

FACES, BAD_INDEX, ZERO_AREA, NONFINITE_Z, EMPTY_BOX, ITEMS, TESTS, INSIDE, SKIPPED, COVERED, STAT_WORDS = range(11)
SMALL_CELLS_DEFAULT, ITEM_ROWS_DEFAULT, ITEM_COLS = 256, 16, 64
NAN_BITS = 0x7FF8000000000000


def bits_of(z: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", z))[0]


def key_of(z: float) -> int:
    """N6: the order-preserving 64-bit key of a float64: greater key <=> greater value, -0.0 below +0.0."""
    u = bits_of(z)
    return (~u) & 0xFFFFFFFFFFFFFFFF if u >> 63 else u | (1 << 63)


def height_at(a, b, c, za, zb, zc, px, py):
    """N5: the face's height at (px, py), or None where the pair is skipped (D == 0 or a height that is not finite).  The int
    differences are exact in float64 (below 2^53)."""
    ex1, ey1, ex2, ey2 = float(b[0] - a[0]), float(b[1] - a[1]), float(c[0] - a[0]), float(c[1] - a[1])
    dx, dy = float(px - a[0]), float(py - a[1])
    D = ex1 * ey2 - ey1 * ex2
    Nb = dx * ey2 - dy * ex2
    Nc = ex1 * dy - ey1 * dx
    if D == 0.0:
        return None
    z = (za + (zb - za) * (Nb / D)) + (zc - za) * (Nc / D)
    return z if math.isfinite(z) else None


def nadir_raster(verts_q, z, faces, window, small_cells=0, item_rows=0):
    """verts_q (V, 2) integers in cell units, z (V,) floats, faces (F, 3) integers, window = (col_off, row_off, width, height)
    -> (face (height, width) int32, -1 for none; z (height, width) float64, NaN for none; stats (10,) int64 as GR_NADIR_STAT_*).
    small_cells and item_rows (0: the defaults) enter the item word alone."""
    col_off, row_off, width, height = (int(v) for v in window)
    small = int(small_cells) or SMALL_CELLS_DEFAULT
    rows_per_item = int(item_rows) or ITEM_ROWS_DEFAULT
    vq = [(int(x), int(y)) for x, y in np.asarray(verts_q).reshape(-1, 2)]
    zz = [float(v) for v in np.asarray(z, dtype=np.float64).reshape(-1)]
    V = len(vq)
    face_out = np.full((height, width), -1, dtype=np.int32)
    best_key = [[0] * width for _ in range(height)]          # 0: no face yet (no finite height has key 0)
    best_z = np.full((height, width), np.nan, dtype=np.float64)
    stats = np.zeros(STAT_WORDS, dtype=np.int64)
    for f, (i, j, k) in enumerate(np.asarray(faces).reshape(-1, 3).tolist()):
        if not (0 <= i < V and 0 <= j < V and 0 <= k < V):
            stats[BAD_INDEX] += 1
            continue
        za, zb, zc = zz[i], zz[j], zz[k]
        if not (math.isfinite(za) and math.isfinite(zb) and math.isfinite(zc)):
            stats[NONFINITE_Z] += 1
            continue
        a, b, c = vq[i], vq[j], vq[k]
        if (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]) == 0:
            stats[ZERO_AREA] += 1
            continue
        stats[FACES] += 1
        xs, ys = (a[0], b[0], c[0]), (a[1], b[1], c[1])
        c0, c1 = max(-((HALF - min(xs)) // ONE), col_off), min((max(xs) - HALF) // ONE, col_off + width - 1)
        r0, r1 = max(-((HALF - min(ys)) // ONE), row_off), min((max(ys) - HALF) // ONE, row_off + height - 1)
        if c0 > c1 or r0 > r1:
            stats[EMPTY_BOX] += 1
            continue
        w, h = c1 - c0 + 1, r1 - r0 + 1
        stats[TESTS] += w * h
        if w * h > small:
            stats[ITEMS] += -(-w // ITEM_COLS) * -(-h // rows_per_item)
        ring = [[a, b, c]]
        for row in range(r0, r1 + 1):
            for col in range(c0, c1 + 1):
                px, py = ONE * col + HALF, ONE * row + HALF
                if not centre_in_rings(px, py, ring):
                    continue
                stats[INSIDE] += 1
                zf = height_at(a, b, c, za, zb, zc, px, py)
                if zf is None:
                    stats[SKIPPED] += 1
                    continue
                key = key_of(zf)
                y, x = row - row_off, col - col_off
                if key > best_key[y][x]:          # strictly: an equal key keeps the lower face
                    best_key[y][x] = key
                    best_z[y, x] = zf
                    face_out[y, x] = f
    stats[COVERED] = int((face_out >= 0).sum())
    return face_out, best_z, stats[:10].copy()


class StandInRasterizer:
    """`NadirRasterizer` on the host: the same checks, then `nadir_raster`."""

    def __init__(self, verts_q, z, faces):
        from geograypher_amd import _hip

        self.V, self.F = _hip.check_nadir_tables(np.asarray(verts_q), np.asarray(z), np.asarray(faces))
        self.verts_q, self.z, self.faces = np.asarray(verts_q), np.asarray(z, dtype=np.float64), np.asarray(faces)
        self.windows = []          # every window asked for, in order

    def window(self, col_off, row_off, width, height, small_cells=0, item_rows=0):
        from geograypher_amd import _hip

        _hip.check_nadir_window(int(col_off), int(row_off), int(width), int(height), int(small_cells), int(item_rows))
        self.windows.append((int(col_off), int(row_off), int(width), int(height)))
        face, z, stats = nadir_raster(self.verts_q, self.z, self.faces, (col_off, row_off, width, height), small_cells, item_rows)
        if stats[BAD_INDEX]:
            raise ValueError(f"gr_nadir_raster: {int(stats[BAD_INDEX])} faces name a vertex outside [0, {self.V})")
        return face, z, stats


class StandInBackend(CrsStandinBackend):
    """`HipRaster.nadir_rasterizer` (and, from tests/crs_standin.py, `reproject_points`) on the host: for the host tests of the
    layers above the call (`top_down_raster`, the mesh methods, `aggregate_images`)."""

    def nadir_rasterizer(self, verts_q, z, faces):
        if not hasattr(self, "rasterizers"):
            self.rasterizers = []
        self.rasterizers.append(StandInRasterizer(verts_q, z, faces))
        return self.rasterizers[-1]
