"""Checker of gr_sample_raster / raster samples (DESIGN.md "Raster samples", T2-T7) on the host: a numpy restatement of the rules,
operation for operation -- every operation a float64 operation rounded on its own, as the device performs them --, so that the
device's results are compared with `np.array_equal(..., equal_nan=True)` and nothing wider.

`sample_raster_np` is the restatement; `sample_by_loop` a second, independent way to the same samples (a Python loop per point
with `math.floor` and Python comparisons, the shape of the reference's per-point `rasterio.sample`), used on the hand-worked scene
and as the host baseline of tools/height_above_ground_rate.py.  `StandInBackend` is `HipRaster.sample_raster` on the CPU, for
host-logic tests."""
import math

import numpy as np

STAT_WORDS = 4   # inside, nodata, ground, bad faces (the device's block)


def invert_affine_np(transform):
    """T2, restated (Python floats, the order of the `affine` package)."""
    a, b, c, d, e, f = (float(v) for v in transform)
    det = a * e - b * d
    idet = 1.0 / det
    ia, ib, id_, ie = e * idet, -b * idet, -d * idet, a * idet
    return (ia, ib, -c * ia - f * ib, id_, ie, -c * id_ - f * ie)


def query_points_np(points, faces):
    """T3: the vertices themselves (faces None), or ((p0 + p1) + p2) / 3.0 per component; (queries (N, 3), bad (N,) bool).  A
    face with a vertex outside [0, V) has no query point (zeros here, never used)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if faces is None:
        return points, np.zeros(len(points), dtype=bool)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    bad = np.any((faces < 0) | (faces >= len(points)), axis=1) if len(faces) else np.zeros(0, dtype=bool)
    safe = np.where(bad[:, None], 0, faces)
    if len(points) == 0:
        return np.zeros((len(faces), 3)), bad
    corners = points[safe]
    with np.errstate(all="ignore"):
        q = ((corners[:, 0] + corners[:, 1]) + corners[:, 2]) / 3.0
    q[bad] = 0.0
    return q, bad


def sample_raster_np(points, faces, data, inverse6, nodata, fill, labels=None, threshold=None, ground_id=None,
                     only_existing=False):
    """-> dict(values (N, B), height (N,), labels (a relabelled COPY, or None), stats (4,) int64, inside, nodata_hit, bad, cf, rf,
    queries)."""
    data = np.asarray(data)
    if data.ndim == 2:
        data = data[None]
    B, H, W = data.shape
    ia, ib, ic, id_, ie, jf = (np.float64(v) for v in inverse6)
    q, bad = query_points_np(points, faces)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(all="ignore"):
        cf = np.floor((x * ia + y * ib) + ic)   # T4
        rf = np.floor((x * id_ + y * ie) + jf)
        inside = ~bad & (cf >= 0) & (cf < W) & (rf >= 0) & (rf < H)
    col = np.where(inside, cf, 0).astype(np.int64)
    row = np.where(inside, rf, 0).astype(np.int64)
    outside_value = 0.0 if nodata is None else np.float64(nodata)
    values = np.where(inside[:, None], data[:, row, col].T.astype(np.float64), outside_value)   # T5
    hit = np.zeros(len(q), dtype=bool)
    if nodata is not None:
        equal = values == np.float64(nodata)
        values = np.where(equal, np.float64(fill), values)
        hit = equal.any(axis=1) & ~bad
    with np.errstate(all="ignore"):
        height = np.where(bad, np.nan, z - values[:, 0])   # T6
    out_labels, n_ground = None, 0
    if labels is not None:
        out_labels = np.array(labels, dtype=np.float64)   # a copy
        flat = out_labels.reshape(-1)
        with np.errstate(all="ignore"):
            mask = height < np.float64(threshold)
        if only_existing:
            mask = mask & np.isfinite(flat)
        flat[mask] = ground_id
        n_ground = int(mask.sum())
    stats = np.array([int(inside.sum()), int(hit.sum()), n_ground, int(bad.sum())], dtype=np.int64)
    return dict(values=values, height=height, labels=out_labels, stats=stats, inside=inside, nodata_hit=hit, bad=bad, cf=cf, rf=rf,
                queries=q)


def sample_by_loop(xy, data, transform, nodata, fill):
    """The samples of (x, y) points one at a time, from the FORWARD transform: (N, B) float64.  Own inverse, `math.floor`, Python
    comparisons; a point is outside when floor raises (NaN, infinities)."""
    data = np.asarray(data)
    if data.ndim == 2:
        data = data[None]
    B, H, W = data.shape
    ia, ib, ic, id_, ie, jf = invert_affine_np(transform)
    out = np.empty((len(xy), B), dtype=np.float64)
    for n, (x, y) in enumerate(xy):
        x, y = float(x), float(y)
        try:
            col, row = math.floor((x * ia + y * ib) + ic), math.floor((x * id_ + y * ie) + jf)
        except (ValueError, OverflowError):
            col = row = -1
        for b in range(B):
            v = float(data[b, row, col]) if 0 <= col < W and 0 <= row < H else (0.0 if nodata is None else float(nodata))
            if nodata is not None and v == float(nodata):
                v = float(fill)
            out[n, b] = v
    return out


def on_cell_edge(points, faces, inverse6):
    """(N,) bool: queries whose column or row coordinate is a whole number (exactly on a cell edge)."""
    ia, ib, ic, id_, ie, jf = (np.float64(v) for v in inverse6)
    q, _ = query_points_np(points, faces)
    cx, ry = (q[:, 0] * ia + q[:, 1] * ib) + ic, (q[:, 0] * id_ + q[:, 1] * ie) + jf
    return (cx == np.floor(cx)) | (ry == np.floor(ry))


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


class StandInBackend:
    """`HipRaster.sample_raster` on the CPU; numpy arrays out.  `labels` of dtype float64 are rewritten in place, as the device
    rewrites a device tensor; the arguments of the last call are kept in `last`."""

    def sample_raster(self, points, faces, raster_data, inverse6, nodata, fill, *, want_values=True, want_height=False, labels=None,
                      threshold=None, ground_id=None, only_existing=False, check=True):
        points, data = _np(points), _np(raster_data)
        faces = None if faces is None else _np(faces)
        if data.dtype not in (np.float32, np.float64):
            data = data.astype(np.float64)
        self.last = dict(points=points, faces=faces, data=data, inverse6=tuple(inverse6), nodata=nodata, fill=fill,
                         threshold=threshold, ground_id=ground_id, only_existing=only_existing)
        if labels is not None and (threshold is None or ground_id is None):
            raise ValueError("labels need threshold and ground_id")
        r = sample_raster_np(points, faces, data, inverse6, nodata, fill, labels=labels, threshold=threshold, ground_id=ground_id,
                             only_existing=only_existing)
        if check and r["bad"].any():
            raise ValueError(f"gr_sample_raster: {int(r['bad'].sum())} faces name a vertex outside [0, {len(points)})")
        out_labels = None
        if labels is not None:
            if isinstance(labels, np.ndarray) and labels.dtype == np.float64:
                np.copyto(labels, r["labels"].reshape(labels.shape))
                out_labels = labels
            else:
                out_labels = r["labels"]
        return (r["values"] if want_values else None, r["height"] if want_height else None, out_labels, r["stats"])


# -- the hand-worked scene ---------------------------------------------------------------------------------------------------------
HAND_TRANSFORM = (0.5, 0.0, 10.0, 0.0, -0.5, 20.0)   # 3 rows x 5 columns of 0.5 m cells: x in [10, 12.5), y in (18.5, 20]
HAND_DATA = np.array([[101.0, 102.0, 103.0, 104.0, 105.0],
                      [201.0, 202.0, 203.0, 204.0, 205.0],
                      [301.0, 302.0, 303.0, 304.0, 305.0]])
HAND_NODATA = -9999.0


def hand_cases():
    """[((x, y), expected sample or None for "outside", what it is)] on HAND_DATA / HAND_TRANSFORM."""
    cases = []
    for r in range(3):
        for c in range(5):
            cases.append(((10.25 + 0.5 * c, 19.75 - 0.5 * r), HAND_DATA[r, c], f"the middle of cell ({r}, {c})"))
    cases += [
        ((10.0, 20.0), 101.0, "the top-left corner of the raster: inside"),
        ((10.5, 19.75), 102.0, "on the edge between columns 0 and 1: the cell to the right"),
        ((12.0, 19.25), 205.0, "on the edge between columns 3 and 4, row 1"),
        ((10.25, 19.5), 201.0, "on the edge between rows 0 and 1: the cell below"),
        ((11.25, 19.0), 303.0, "on the edge between rows 1 and 2"),
        ((11.0, 19.5), 203.0, "on an inner corner: the cell right of and below it"),
        ((10.0, 19.25), 201.0, "on the left outer edge: inside"),
        ((11.75, 20.0), 104.0, "on the top outer edge: inside"),
        ((12.5, 19.75), None, "on the right outer edge: outside"),
        ((10.25, 18.5), None, "on the bottom outer edge: outside"),
        ((12.5, 18.5), None, "the bottom-right corner: outside"),
        ((9.75, 19.75), None, "left of the raster"),
        ((12.75, 19.75), None, "right of the raster"),
        ((11.25, 20.25), None, "above the raster"),
        ((11.25, 18.25), None, "below the raster"),
    ]
    return cases


def centred_faces(centres, z=0.0):
    """(points (3 n, 3) float64, faces (n, 3) int32): one triangle per centre c with corners c + (-1, -0.5), c + (1, -0.5),
    c + (0, 1) and heights z - 1.5, z, z + 1.5: for coordinates on a 0.25 lattice of moderate size the centre
    ((p0 + p1) + p2) / 3.0 is exactly (c, z)."""
    centres = np.asarray(centres, dtype=np.float64).reshape(-1, 2)
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), (len(centres),))
    corners = np.array([[-1.0, -0.5, -1.5], [1.0, -0.5, 0.0], [0.0, 1.0, 1.5]])
    points = (np.column_stack([centres, z])[:, None, :] + corners[None]).reshape(-1, 3)
    return points, np.arange(3 * len(centres), dtype=np.int32).reshape(-1, 3)


# -- the random scene --------------------------------------------------------------------------------------------------------------
RANDOM_TRANSFORM = (0.5, 0.0, 100.0, 0.0, -0.5, 215.0)   # 30 rows x 40 columns of 0.5 m cells: x in [100, 120), y in (200, 215]
RANDOM_NODATA = -32768.0


def random_scene(seed=5, n_faces=4000):
    """(points (V, 3), faces (F, 3) int32, data (30, 40) float32, transform, nodata): every vertex on a 0.25 m lattice (corners
    c + d1, c + d2, c - d1 - d2 around a lattice centre c, so that half the centres lie exactly on cell edges), centres from 3 m
    outside the raster on every side, every 16th cell nodata.  The corners of a face are scattered through the vertex array."""
    rng = np.random.default_rng(seed)
    data = np.round(rng.uniform(50.0, 60.0, (30, 40)) * 8.0) / 8.0
    data[rng.uniform(size=data.shape) < 1.0 / 16.0] = RANDOM_NODATA
    c = np.round(rng.uniform([97.0, 197.0], [123.0, 218.0], (n_faces, 2)) * 4.0) / 4.0
    d1, d2 = (np.round(rng.uniform(-1.5, 1.5, (n_faces, 2)) * 4.0) / 4.0 for _ in range(2))
    cz = np.round(rng.uniform(48.0, 66.0, n_faces) * 4.0) / 4.0
    dz1, dz2 = (np.round(rng.uniform(-1.0, 1.0, n_faces) * 4.0) / 4.0 for _ in range(2))
    corners = np.stack([np.column_stack([c + d1, cz + dz1]), np.column_stack([c + d2, cz + dz2]),
                        np.column_stack([c - d1 - d2, cz - dz1 - dz2])], axis=1).reshape(-1, 3)
    order = rng.permutation(len(corners))
    place = np.empty_like(order)
    place[order] = np.arange(len(corners))
    faces = place[np.arange(len(corners)).reshape(-1, 3)].astype(np.int32)
    return corners[order], faces, data.astype(np.float32), RANDOM_TRANSFORM, RANDOM_NODATA
