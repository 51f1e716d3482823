"""Rules B1-B4 of DESIGN.md 8m in Python integers, written independently of the device code: the stand-in the device's polygon
burn is compared with.  Exact: membership is `zonal_standin.centre_in_rings` (Z3, pinned by hand-worked cases), everything else
is a loop over rows in painter's order.

B1: the window is (col_off, row_off, width, height) in cells of the parent grid; cell (y, x) of the window is cell
(row_off + y, col_off + x) of the grid, whose centre is (65536 col + 32768, 65536 row + 32768) in ring units.  B3: the rows are
painted in ascending index, so the highest row that holds a centre stays.  B4: out = values[rows], `fill` where rows is -1."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))

from crs_standin import CrsStandinBackend  # noqa: E402
from zonal_standin import HALF, ONE, centre_in_rings, to_cell_units  # noqa: E402,F401


def burn(rings_q, ring_polygon, n_polygons, window, values=None, fill=255):
    """rings_q: a list of rings of (qx, qy) integer vertices in cell units, ring_polygon their rows, window = (col_off, row_off,
    width, height) -> (rows (height, width) int32, out (height, width) uint8 or None without `values`, stats (8,) int64 as
    GR_BURN_STAT_*; word 0, the cells tested, is left 0: it depends on the work decomposition; word 2, the burned cells, is
    counted by the pass that writes `out` and stays 0 without `values`)."""
    col_off, row_off, width, height = (int(v) for v in window)
    rows = np.full((height, width), -1, dtype=np.int32)
    stats = np.zeros(8, dtype=np.int64)
    stats[3] = max([len(r) for r in rings_q], default=0)
    stats[4] = sum(1 for r in rings_q if len(r) < 3)
    for p in range(n_polygons):
        mine = [r for r, row in zip(rings_q, ring_polygon) if row == p and len(r) >= 3]
        if not mine:
            continue
        xs = [v[0] for r in mine for v in r]
        ys = [v[1] for r in mine for v in r]
        # the cells whose centre the box of the rings can hold, cut to the window
        c0, c1 = max(-((HALF - min(xs)) // ONE), col_off), min((max(xs) - HALF) // ONE, col_off + width - 1)
        r0, r1 = max(-((HALF - min(ys)) // ONE), row_off), min((max(ys) - HALF) // ONE, row_off + height - 1)
        for row in range(r0, r1 + 1):
            for col in range(c0, c1 + 1):
                if centre_in_rings(ONE * col + HALF, ONE * row + HALF, mine):
                    stats[1] += 1
                    rows[row - row_off, col - col_off] = p
    out = None
    if values is not None:
        values = np.asarray(values)
        out = np.where(rows >= 0, values[np.maximum(rows, 0)] if len(values) else fill, fill).astype(np.uint8)
        stats[2] = int((rows >= 0).sum())
    return rows, out, stats


def rings_of_table(ring_vertices, ring_offsets):
    rv, off = np.asarray(ring_vertices), np.asarray(ring_offsets)
    return [[(int(x), int(y)) for x, y in rv[off[r]:off[r + 1]]] for r in range(len(off) - 1)]


class StandInBurner:
    """`PolygonBurner` on the host: the same checks, then `burn`."""

    def __init__(self, ring_vertices, ring_offsets, ring_polygon, n_polygons, values=None):
        from geograypher_amd import _hip

        self.n_rings = _hip.check_burn_tables(ring_vertices, ring_offsets, ring_polygon, n_polygons, values)
        self.rings = rings_of_table(ring_vertices, ring_offsets)
        self.ring_polygon = [int(p) for p in ring_polygon]
        self.n_polygons = int(n_polygons)
        self.values = None if values is None else np.asarray(values, dtype=np.uint8)
        self.windows = []          # every window asked for, in order

    def window(self, col_off, row_off, width, height, items, fill=255, want_values=True):
        from geograypher_amd import _hip

        _hip.check_burn_window(int(col_off), int(row_off), int(width), int(height), np.asarray(items), self.n_polygons, self.n_rings, int(fill))
        if want_values and self.values is None:
            raise ValueError("gr_burn_polygons: this burner was made without values")
        self.windows.append((int(col_off), int(row_off), int(width), int(height)))
        rows, out, stats = burn(self.rings, self.ring_polygon, self.n_polygons, (col_off, row_off, width, height),
                                self.values if want_values else None, fill)
        items = np.asarray(items, dtype=np.int64).reshape(-1, 7)
        stats[0] = int((items[:, 3] * items[:, 4]).sum())
        return rows, out, stats


class StandInBackend(CrsStandinBackend):
    """`HipRaster.polygon_burner` (and, from tests/crs_standin.py, `reproject_points`) on the host: for the host tests of the layers
    above the burn (`burn_polygons`, `write_chips`)."""

    def __init__(self):
        self.burners = []

    def polygon_burner(self, ring_vertices, ring_offsets, ring_polygon, n_polygons, values=None):
        self.burners.append(StandInBurner(ring_vertices, ring_offsets, ring_polygon, n_polygons, values))
        return self.burners[-1]
