"""Checkers of the polygon-on-polygon overlap areas (gr_polygon_box_pairs_count / _fill, gr_polygon_overlap_areas; rules A1-A9 of
DESIGN.md 8o), all on the host, and the scenes both test files share:

 - `exact_pair`: the rules in exact rational arithmetic (fractions.Fraction over Python integers) for one pair of rows;
 - `exact_areas`: the same rules for many pairs.  Every TERM is formed exactly, as an integer numerator over an integer denominator;
   the terms of a pair are then summed in fixed point with FIXED_BITS = 256 fractional bits, each rounded down, because a sum of
   thousands of Fractions of unrelated denominators takes seconds a pair.  A pair of n terms is off by less than n 2^-256 square
   grid steps -- 10^-60 of anything it is compared with -- and "exactly 0" reads |area| < 2^-200 (`is_zero`).  `exact_pair` pins it;
 - `restated_areas`: the same rules in numpy float64 in the operation order of A5, the terms of a pair summed sequentially;
 - `StandInBackend`: the binding's `polygon_overlap` over `restated_areas`, for the host layers;
 - `clip_area`: an INDEPENDENT exact check, Sutherland-Hodgman in Fractions of a simple polygon against a convex clipper.

A table is the five arrays of `PlanarPolygons.snapped`: ring vertices (N, 2), ring offsets (R + 1,), ring polygon (R,), ring is hole
(R,), polygon boxes (P, 4), every ring counter-clockwise."""
from fractions import Fraction

import numpy as np

from geograypher_amd.utils.geometric import PlanarPolygons, overlap_work_items, snap_polygon_pair

# A6.  K = 4 x the largest r = |restated - exact| / (2^-53 area_abs) over every pair of every scene below, rounded up to a power of
# two.  Measured by tests/test_polygon_overlap_host.py::test_the_bound_is_measured: r_max = 4.27, on the scene "edges" at the local origin, pair (3, 3)
# (the row of 513 vertices against the row of 4097: a sequential sum of 13 186 terms), so 4 r_max = 17.1 and K = 32.  The largest
# ratio the DEVICE reached on an MI355X over the same scenes (tests/test_polygon_overlap_gpu.py::test_scenes_within_the_bound prints
# it per scene): 1.012, on the scene "tiling"; "stars" 0.950, "edges" 0.310 -- its tree-shaped sum is kinder than the sequential one.
OVERLAP_BOUND_K = 32.0
BOUND_SCENE = "edges"
DEVICE_LARGEST_RATIO = 1.012   # recorded, not asserted: the device is held to OVERLAP_BOUND_K
FIXED_BITS = 256
STAT_WORDS = 8
SHIFT = (600000.0, 4200000.0)   # UTM-sized coordinates: every scene is checked at its local origin and shifted here


def is_zero(area_fixed) -> bool:
    return abs(area_fixed) < (1 << (FIXED_BITS - 200))


def fixed_to_float(v) -> float:
    return float(Fraction(v, 1 << FIXED_BITS))


# -- the rows of a table as edge lists -------------------------------------------------------------------------------------------------
def row_edges(table, row):
    """(xl, yl, xr, yr (E,) int64, sign (E,) int64, slots (E,) int64) of the non-vertical edges of the rings of 3 or more vertices of
    `row`, ordered by slot: A4."""
    rv, off, rp, rh, _ = table
    out = [[] for _ in range(6)]
    for r in np.nonzero(np.asarray(rp) == row)[0]:
        ring = np.asarray(rv[off[r]:off[r + 1]], dtype=np.int64)
        if len(ring) < 3:
            continue
        nxt = np.roll(ring, -1, axis=0)
        live = ring[:, 0] != nxt[:, 0]
        rising = nxt[:, 0] > ring[:, 0]
        sigma = -1 if rh[r] else 1
        for k, v in enumerate((np.where(rising, ring[:, 0], nxt[:, 0]), np.where(rising, ring[:, 1], nxt[:, 1]),
                               np.where(rising, nxt[:, 0], ring[:, 0]), np.where(rising, nxt[:, 1], ring[:, 1]),
                               -sigma * np.where(rising, 1, -1), off[r] + np.arange(len(ring)))):
            out[k].append(v[live])
    return tuple(np.concatenate(v) if v else np.zeros(0, dtype=np.int64) for v in out)


def pair_frame(table_a, table_b, a, b):
    """A3: (X0, X1, Y) of a pair, integers."""
    ba, bb = table_a[4][a], table_b[4][b]
    return int(max(ba[0], bb[0])), int(min(ba[2], bb[2])), int(min(ba[1], bb[1]))


def taking_part(ea, eb, X0, X1):
    """A3 in int64: (index into ea, index into eb, lo, hi) of the edge pairs with hi > lo, a-major."""
    lo = np.maximum(np.maximum(ea[0][:, None], eb[0][None, :]), X0)
    hi = np.minimum(np.minimum(ea[2][:, None], eb[2][None, :]), X1)
    i, j = np.nonzero(hi > lo)
    return i, j, lo[i, j], hi[i, j]


# -- exact ----------------------------------------------------------------------------------------------------------------------------
def exact_terms(ea, eb, X0, X1, Y):
    """The terms I(e, f) of a pair as exact quotients: (numerators, denominators, signs) object arrays of Python integers."""
    i, j, lo, hi = taking_part(ea, eb, X0, X1)
    obj = lambda v: np.asarray(v, dtype=np.int64).astype(object)   # noqa: E731
    lo, hi = obj(lo), obj(hi)
    w = hi - lo
    xe, ye, dxe, dye = obj(ea[0][i]), obj(ea[1][i]) - Y, obj(ea[2][i] - ea[0][i]), obj(ea[3][i] - ea[1][i])
    xf, yf, dxf, dyf = obj(eb[0][j]), obj(eb[1][j]) - Y, obj(eb[2][j] - eb[0][j]), obj(eb[3][j] - eb[1][j])
    ne0, ne1 = ye * dxe + dye * (lo - xe), ye * dxe + dye * (hi - xe)      # heights of e times dxe
    nf0, nf1 = yf * dxf + dyf * (lo - xf), yf * dxf + dyf * (hi - xf)
    q = dxe * dxf
    d0, d1 = ne0 * dxf - nf0 * dxe, ne1 * dxf - nf1 * dxe                  # (he - hf) q at lo and at hi
    m0 = np.where(d0 <= 0, ne0 * dxf, nf0 * dxe)                           # the lower height times q
    m1 = np.where(d1 <= 0, ne1 * dxf, nf1 * dxe)
    cross = ((d0 < 0) & (d1 > 0)) | ((d0 > 0) & (d1 < 0))
    num, den = (m0 + m1) * w, 2 * q
    if np.any(cross):
        c = np.nonzero(cross)[0]
        S = d0[c] - d1[c]
        H = ne0[c] * S + dye[c] * d0[c] * w[c]                             # the crossing height times dxe S
        num[c] = w[c] * ((m0[c] * S + H * dxf[c]) * d0[c] - (H * dxf[c] + m1[c] * S) * d1[c])
        den[c] = 2 * q[c] * S * S
    return num, den, obj(ea[4][i] * eb[4][j])


def exact_pair(table_a, table_b, a, b):
    """(area, area_abs) of one pair as Fractions, in square grid steps."""
    X0, X1, Y = pair_frame(table_a, table_b, a, b)
    num, den, sign = exact_terms(row_edges(table_a, a), row_edges(table_b, b), X0, X1, Y)
    terms = [Fraction(int(n), int(d)) for n, d in zip(num, den)]
    return sum((int(s) * t for s, t in zip(sign, terms)), Fraction(0)), sum((abs(t) for t in terms), Fraction(0))


def box_pairs(table_a, table_b):
    """A2: (n, 2) int64, ascending by (a, b)."""
    ba, bb = np.asarray(table_a[4], dtype=np.int64).reshape(-1, 4), np.asarray(table_b[4], dtype=np.int64).reshape(-1, 4)
    hit = ((np.maximum(ba[:, None, 0], bb[None, :, 0]) < np.minimum(ba[:, None, 2], bb[None, :, 2]))
           & (np.maximum(ba[:, None, 1], bb[None, :, 1]) < np.minimum(ba[:, None, 3], bb[None, :, 3])))
    return np.argwhere(hit).astype(np.int64).reshape(-1, 2)


def table_stats(table_a, table_b, n_pairs, n_items):
    """A9 without the edge-pair word."""
    stats = np.zeros(STAT_WORDS, dtype=np.int64)
    stats[0], stats[1] = n_pairs, n_items
    for rv, off, rp, rh, _ in (table_a, table_b):
        for r in range(len(rp)):
            ring = np.asarray(rv[off[r]:off[r + 1]], dtype=np.int64)
            stats[5] = max(stats[5], len(ring))
            if len(ring) < 3:
                stats[4] += 1
            else:
                stats[3] += int(np.sum(ring[:, 0] == np.roll(ring[:, 0], -1)))
    return stats


def exact_areas(table_a, table_b, pairs, n_items=0):
    """(area, area_abs: lists of fixed-point integers with FIXED_BITS fractional bits, square grid steps; stats (8,) int64)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    stats = table_stats(table_a, table_b, len(pairs), n_items)
    edges_a, edges_b = {}, {}
    area, area_abs = [], []
    for a, b in pairs.tolist():
        ea = edges_a.setdefault(a, row_edges(table_a, a))
        eb = edges_b.setdefault(b, row_edges(table_b, b))
        num, den, sign = exact_terms(ea, eb, *pair_frame(table_a, table_b, a, b))
        stats[2] += len(num)
        terms = (num << FIXED_BITS) // den if len(num) else num
        area.append(int(np.sum(terms * sign)) if len(num) else 0)
        area_abs.append(int(np.sum(np.abs(terms))) if len(num) else 0)
    return area, area_abs, stats


# -- the numpy restatement of A5 ---------------------------------------------------------------------------------------------------------------
def restated_terms(ea, eb, X0, X1, Y):
    """(terms I(e, f) float64 in A5's order of operations, signs float64)."""
    i, j, lo, hi = taking_part(ea, eb, X0, X1)
    f64 = lambda v: np.asarray(v, dtype=np.int64).astype(np.float64)   # noqa: E731  (|values| < 2^41: exact)
    lo, hi = f64(lo - X0), f64(hi - X0)
    rec = []
    for e, k in ((ea, i), (eb, j)):
        xl, xr, yl, yr = f64(e[0][k] - X0), f64(e[2][k] - X0), f64(e[1][k] - Y), f64(e[3][k] - Y)
        rec.append((xl, yl, (yr - yl) / (xr - xl)))
    (xe, ye, me), (xf, yf, mf) = rec
    he0, he1 = ye + me * (lo - xe), ye + me * (hi - xe)
    hf0, hf1 = yf + mf * (lo - xf), yf + mf * (hi - xf)
    d_lo, d_hi, w = he0 - hf0, he1 - hf1, hi - lo
    h0, h1 = np.minimum(he0, hf0), np.minimum(he1, hf1)
    cross = ((d_lo < 0) & (d_hi > 0)) | ((d_lo > 0) & (d_hi < 0))
    with np.errstate(divide="ignore", invalid="ignore"):   # (the branch is formed for every pair and taken where they cross)
        t = d_lo / (d_lo - d_hi)
        w0 = t * w
        hc = ye + me * ((lo + w0) - xe)
        crossing = (0.5 * (h0 + hc)) * w0 + (0.5 * (hc + h1)) * (w - w0)
    return np.where(cross, crossing, (0.5 * (h0 + h1)) * w), f64(ea[4][i] * eb[4][j])


def sequential_sum(values) -> float:
    return float(np.cumsum(values)[-1]) if len(values) else 0.0


def restated_areas(table_a, table_b, pairs, n_items=0):
    """(area (n,), area_abs (n,) float64 in square grid steps, stats (8,) int64)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    stats = table_stats(table_a, table_b, len(pairs), n_items)
    edges_a, edges_b = {}, {}
    area, area_abs = np.zeros(len(pairs)), np.zeros(len(pairs))
    for k, (a, b) in enumerate(pairs.tolist()):
        ea = edges_a.setdefault(a, row_edges(table_a, a))
        eb = edges_b.setdefault(b, row_edges(table_b, b))
        terms, sign = restated_terms(ea, eb, *pair_frame(table_a, table_b, a, b))
        stats[2] += len(terms)
        area[k], area_abs[k] = sequential_sum(sign * terms), sequential_sum(np.abs(terms))
    return area, area_abs, stats


class StandInOverlap:
    def __init__(self, table_a, table_b):
        self.table_a, self.table_b = ([np.asarray(x) for x in t] for t in (table_a, table_b))
        self.calls = []

    def pairs(self):
        return box_pairs(self.table_a, self.table_b).astype(np.int32)

    def areas(self, pairs, items):
        from geograypher_amd import _hip

        _hip.check_overlap_items(pairs, items, self.table_a[1], self.table_a[2], len(self.table_a[4]), self.table_b[1], self.table_b[2],
                                 len(self.table_b[4]))
        self.calls.append((len(pairs), len(items)))
        return restated_areas(self.table_a, self.table_b, pairs, len(items))


class StandInBackend:
    """The binding's `polygon_overlap` on the host: the same checks, `restated_areas` in place of the device."""

    def __init__(self):
        self.overlaps = []

    def polygon_overlap(self, table_a, table_b):
        from geograypher_amd import _hip

        _hip.check_overlap_tables(table_a, table_b)
        self.overlaps.append(StandInOverlap(table_a, table_b))
        return self.overlaps[-1]


# -- the independent check --------------------------------------------------------------------------------------------------------------------
def clip_area(subject, clipper) -> Fraction:
    """area(subject n clipper) in Fractions: Sutherland-Hodgman of the simple polygon `subject` against the CONVEX, counter-clockwise
    `clipper`, then the shoelace sum (the degenerate bridges the clip leaves along the clipper's edges have no area)."""
    poly = [(Fraction(x), Fraction(y)) for x, y in subject]
    clip = [(Fraction(x), Fraction(y)) for x, y in clipper]
    for k in range(len(clip)):
        (ax, ay), (bx, by) = clip[k], clip[(k + 1) % len(clip)]
        side = lambda p: (bx - ax) * (p[1] - ay) - (by - ay) * (p[0] - ax)   # noqa: E731  (> 0: left of a b, inside)
        out = []
        for n in range(len(poly)):
            p, q = poly[n], poly[(n + 1) % len(poly)]
            sp, sq = side(p), side(q)
            if sp >= 0:
                out.append(p)
            if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        poly = out
        if not poly:
            return Fraction(0)
    return abs(sum(poly[n - 1][0] * poly[n][1] - poly[n][0] * poly[n - 1][1] for n in range(len(poly)))) / 2


# -- scenes ------------------------------------------------------------------------------------------------------------------------------
def square(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


HOLED = [square(0, 0, 4, 4), square(1, 1, 3, 3)]
# (name, rows of A, rows of B, area(A row 0 n B row 0) in m^2 or None: left to the independent check, candidate pairs)
HAND_CASES = [
    ("holed square against a square", [HOLED], [[square(2, 2, 6, 6)]], 3, 1),
    ("holed square against itself", [HOLED], [HOLED], 12, 1),
    ("L-shape against a square in its notch", [[[(0, 0), (4, 0), (4, 2), (2, 2), (2, 4), (0, 4)]]], [[square(2.5, 2.5, 3.5, 3.5)]], 0, 1),
    ("a square inside the other's hole", [HOLED], [[square(1.5, 1.5, 2.5, 2.5)]], 0, 1),
    ("a hole partly covered", [HOLED], [[square(0, 0, 2, 2)]], 3, 1),
    ("two triangles", [[[(0, 0), (4, 0), (0, 4)]]], [[[(0, 0), (4, 4), (0, 4)]]], 4, 1),
    ("the crossing triangles", [[[(0, 0), (4, 0), (2, 4)]]], [[[(0, 3), (2, -1), (4, 3)]]], None, 1),
    ("squares that share an edge", [[square(0, 0, 2, 2)]], [[square(2, 0, 4, 2)]], 0, 0),
    ("squares that touch at a vertex", [[square(0, 0, 2, 2)]], [[square(2, 2, 4, 4)]], 0, 0),
]


def polygons_of(rows, shift=(0.0, 0.0)):
    """rows: [[exterior, hole, ...] or [[exterior, hole, ...], [exterior, ...]] (a multi-part row: a list of parts)] -> PlanarPolygons."""
    rings, owner, holes = [], [], []
    for p, row in enumerate(rows):
        parts = row if np.ndim(row[0][0]) == 2 else [row]   # a part is a list of rings, a ring a list of points
        for part in parts:
            for k, ring in enumerate(part):
                rings.append(np.asarray(ring, dtype=np.float64) + np.asarray(shift))
                owner.append(p)
                holes.append(k > 0)
    return PlanarPolygons(rings, owner, holes, n_polygons=len(rows))


def wavy_ring(n, centre, radius, lobes=7, phase=0.0):
    angle = np.linspace(0, 2 * np.pi, n, endpoint=False) + phase
    r = radius * (0.65 + 0.35 * np.cos(lobes * angle) ** 2)
    return np.stack([centre[0] + r * np.cos(angle), centre[1] + r * np.sin(angle)], axis=1)


def star_rows(seed, n_rows, extent=(130.0, 100.0)):
    """Seeded star-shaped polygons of 3-40 vertices, one ring a row.  The angles about the centre are jittered steps of a full turn,
    so that no gap reaches a half turn from 4 vertices on: the ring is star-shaped about its centre and therefore simple (sorted
    uniform angles, as tests/test_polygon_burn_gpu.py draws them, give self-intersecting rings, which are undefined here)."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n_rows):
        n = int(rng.integers(3, 41))
        angle = 2 * np.pi * (np.arange(n) + rng.uniform(0.0, 0.8, n)) / n + rng.uniform(0, 2 * np.pi)
        radius = rng.uniform(2.0, 11.0) * rng.uniform(0.4, 1.0, n)
        centre = rng.uniform((0, 0), extent)
        rows.append([centre + np.stack([radius * np.cos(angle), radius * np.sin(angle)], axis=1)])
    return rows


def scene_edges():
    """Rows of 255, 256, 257 and 513 edges (the LDS side) against rows of 255, 256, 257 and 4097 edges (the lane side: 4097 is one more
    than a b-tile, so its last tile has 1 slot)."""
    A = [[wavy_ring(n, (10.0 + k, 10.0), 9.0, lobes=5, phase=0.1 * k)] for k, n in enumerate((255, 256, 257, 513))]
    B = [[wavy_ring(n, (12.0, 9.0 + k), 8.0, lobes=6, phase=0.3 + 0.2 * k)] for k, n in enumerate((255, 256, 257, 4097))]
    return A, B


def scene_rings():
    """Two-part rows of 300 + 777 and 777 + 300 vertices: tiles of 256 slots start and end inside rings and span two of them."""
    A = [[[wavy_ring(300, (20.0, 20.0), 12.0)], [wavy_ring(777, (52.0, 22.0), 18.0, lobes=9)]]]
    B = [[[wavy_ring(777, (30.0, 24.0), 17.0, lobes=4, phase=0.2)], [wavy_ring(300, (58.0, 18.0), 11.0, phase=0.5)]]]
    return A, B


def scene_parts():
    """A multi-part row with two holes against a row across both parts; with small tiles the ring ends fall inside tiles."""
    part_1 = [wavy_ring(30, (10.0, 10.0), 9.0, lobes=3), square(6.5, 8.0, 8.5, 10.0)[::-1], [(11.0, 9.0), (13.5, 9.5), (13.0, 12.0), (11.5, 12.5), (10.5, 11.0)]]
    part_2 = [wavy_ring(12, (27.0, 11.0), 5.0, lobes=2)]
    A = [[part_1, part_2], [square(40, 40, 41, 41)]]
    B = [[wavy_ring(23, (17.0, 10.5), 12.5, lobes=4, phase=0.4)], [square(7.0, 8.5, 8.0, 9.5)]]
    return A, B


def scene_stars():
    return star_rows(21, 200), star_rows(22, 200)


def tiling_quads(seed, extent=(130.0, 100.0), step=10.0):
    """Jittered quadrilaterals that tile a rectangle beyond `extent` on every side (the construction of tests/test_zonal_counts_gpu.py):
    interior grid vertices move, the outline does not."""
    rng = np.random.default_rng(seed)
    xs, ys = np.arange(-2 * step, extent[0] + 3 * step, step), np.arange(-2 * step, extent[1] + 3 * step, step)
    gx, gy = np.meshgrid(xs, ys)
    jitter = rng.uniform(-0.4 * step, 0.4 * step, gx.shape + (2,))
    jitter[[0, -1], :, :] = 0
    jitter[:, [0, -1], :] = 0
    vx, vy = gx + jitter[..., 0], gy + jitter[..., 1]
    return [[np.array([(vx[j, i], vy[j, i]), (vx[j, i + 1], vy[j, i + 1]), (vx[j + 1, i + 1], vy[j + 1, i + 1]), (vx[j + 1, i], vy[j + 1, i])])]
            for j in range(len(ys) - 1) for i in range(len(xs) - 1)]


def scene_tiling():
    return star_rows(23, 50), tiling_quads(24)


SCENES = {"edges": scene_edges, "rings": scene_rings, "parts": scene_parts, "stars": scene_stars, "tiling": scene_tiling}
for _k, (_name, _a, _b, _area, _n) in enumerate(HAND_CASES):
    SCENES[f"hand {_k}"] = (lambda a=_a, b=_b: (a, b))

_CACHE = {}


def scene_tables(name, shifted=False):
    """(table_a, table_b, pairs (n, 2) int64) of a scene, cached: the snapped tables behind one origin and the candidate pairs."""
    key = (name, bool(shifted))
    if key not in _CACHE:
        rows_a, rows_b = SCENES[name]()
        shift = SHIFT if shifted else (0.0, 0.0)
        table_a, table_b, _ = snap_polygon_pair(polygons_of(rows_a, shift), polygons_of(rows_b, shift))
        _CACHE[key] = (table_a, table_b, box_pairs(table_a, table_b))
    return _CACHE[key]


_EXACT = {}


def scene_exact(name, shifted=False):
    """`exact_areas` of a scene over its candidate pairs, computed once and shared."""
    key = (name, bool(shifted))
    if key not in _EXACT:
        table_a, table_b, pairs = scene_tables(name, shifted)
        _EXACT[key] = exact_areas(table_a, table_b, pairs)
    return _EXACT[key]


def scene_items(name, shifted=False, tile=None):
    table_a, table_b, pairs = scene_tables(name, shifted)
    return overlap_work_items(table_a[1], table_a[2], table_b[1], table_b[2], pairs, *(() if tile is None else (tile,)))


MIN_AREA = 10 ** 6   # square grid steps: 1e-6 m^2


def far_from_every_bound(name, shifted=False) -> bool:
    """The condition on the scenes: every candidate pair has an exact area of 0 or of at least 1e-6 m^2."""
    area, _, _ = scene_exact(name, shifted)
    return all(is_zero(v) or v >= (MIN_AREA << FIXED_BITS) for v in area)
