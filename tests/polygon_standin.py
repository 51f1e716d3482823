"""Checkers of gr_polygon_class_weights / label_polygons (DESIGN.md "Polygon labels"), all on the host:

(a) an EXACT oracle in Python integers and `fractions.Fraction`: the intersection of a snapped triangle with a polygon is clipped
    in rational arithmetic (list-based Sutherland-Hodgman of every ring against the triangle), so areas are exact, and the
    containment decision is `area(T n P) == area(T)` -- deliberately not the device's method (sign tests of ring edges against
    the open triangle plus an even-odd test of the centroid);
(b) a float64 stand-in that follows the device's operation order for the overlay area (Python floats: every operation rounded
    on its own, like the library built with -ffp-contract=off) and restates its sign predicates in Python integers;
(c) `StandInBackend`, the `HipRaster.polygon_class_weights` interface over (b), for host-logic tests without a GPU;
(d) seeded scene generators on an integer lattice (`lattice_scene`, `wave_scene`) with their answers computed once per process
    (`lattice_case`, `wave_case`), and a canary, `within_wrapped64`: (b)'s containment with 64-bit determinants.

(a)-(c) take the snapped table of `PlanarPolygons.snapped`, or a raw one of `make_table`, and (F, 6) integer triangles.
"""
import functools
from fractions import Fraction
from pathlib import Path

import numpy as np

GRID2_PER_M2 = 10 ** 12   # grid cells (1e-6 m squared) per square metre
GOLDEN = Path(__file__).resolve().parent / "golden" / "label_polygons.npz"   # tests/golden/make_golden_label_polygons.py
SCENES = ("tin", "folded", "integer")


def load_scene(name):
    """Scene `name` of the committed fixture as a dict of its arrays, plus "polygons" (a PlanarPolygons), "weighting" (None
    where the scene has none) and "e_ref"."""
    from geograypher_amd.utils.geometric import PlanarPolygons

    with np.load(GOLDEN) as z:
        d = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}
        d["e_ref"] = float(z["e_ref"])
    off = d["ring_offsets"]
    rings = [d["rings"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    d["polygons"] = PlanarPolygons(rings, d["ring_polygon"], d["ring_is_hole"], n_polygons=int(d["n_polygons"]))
    d["weighting"] = d["face_weighting"] if d["face_weighting"].size else None
    return d


def overlay_tolerance(e_ref, pairs_per_polygon, want):
    """The overlay bound per (polygon, class): 4 e_ref n_pairs + 1e-12 |sum|."""
    return 4.0 * e_ref * np.asarray(pairs_per_polygon, dtype=np.float64)[:, None] + 1e-12 * np.abs(want)


# -- shared integer helpers ----------------------------------------------------------------------------------------------------
def _orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def ccw_triangle(t6):
    """((x0, y0), (x1, y1), (x2, y2)) counter-clockwise as Python ints, and twice the area (0: collapsed)."""
    x0, y0, x1, y1, x2, y2 = (int(v) for v in t6)
    o = _orient(x0, y0, x1, y1, x2, y2)
    if o < 0:
        return ((x0, y0), (x2, y2), (x1, y1)), -o
    return ((x0, y0), (x1, y1), (x2, y2)), o


def polygon_rings(table, p):
    """[(vertices as a list of int pairs, is_hole)] of polygon p."""
    rv, roff, rpoly, rhole, _ = table
    out = []
    for r in np.nonzero(np.asarray(rpoly) == p)[0]:
        pts = [(int(x), int(y)) for x, y in rv[int(roff[r]):int(roff[r + 1])]]
        if len(pts) >= 3:
            out.append((pts, bool(rhole[r])))
    return out


def polygon_has_rows(table, p):
    """Does any row of the ring table name polygon p?  The device meets a polygon through its ring rows -- of any length -- and a
    polygon without rows has no box (the table's empty box 1 1 0 0 is a placeholder, not a region)."""
    return bool(np.any(np.asarray(table[2]) == p))


def candidate_faces(tri, box):
    """Faces whose box overlaps the polygon's (closed boxes), as the device pairs them."""
    tri = np.asarray(tri)
    xs, ys = tri[:, 0::2], tri[:, 1::2]
    return np.nonzero((xs.min(1) <= box[2]) & (xs.max(1) >= box[0]) & (ys.min(1) <= box[3]) & (ys.max(1) >= box[1]))[0]


# -- (a) the exact oracle -------------------------------------------------------------------------------------------------------
def _clip_ring_exact(ring, a, b):
    """Sutherland-Hodgman of a ring (Fractions) against the half-plane left of a -> b."""
    out = []
    n = len(ring)
    for i in range(n):
        s, e = ring[i - 1], ring[i]
        ds = _orient(a[0], a[1], b[0], b[1], s[0], s[1])
        de = _orient(a[0], a[1], b[0], b[1], e[0], e[1])
        if (de >= 0) != (ds >= 0):
            t = Fraction(ds) / Fraction(ds - de)
            out.append((s[0] + t * (e[0] - s[0]), s[1] + t * (e[1] - s[1])))
        if de >= 0:
            out.append(e)
    return out


def _area2_exact(ring):
    return sum(ring[i - 1][0] * ring[i][1] - ring[i][0] * ring[i - 1][1] for i in range(len(ring)))


def exact_intersection_area2(t, rings):
    """Twice area(triangle n polygon) in grid cells, a Fraction: exterior rings minus holes (rings counter-clockwise)."""
    total = Fraction(0)
    for pts, hole in rings:
        ring = [(Fraction(x), Fraction(y)) for x, y in pts]
        for k in range(3):
            if not ring:
                break
            ring = _clip_ring_exact(ring, t[k], t[(k + 1) % 3])
        a2 = _area2_exact(ring) if ring else Fraction(0)
        total += -a2 if hole else a2
    return total


def exact_pairs(tri, face_class, table):
    """{(face, polygon): (contained, twice the intersection area in grid cells as a Fraction, twice the triangle's area)} for
    every pair of a labelled, uncollapsed face and a polygon whose boxes overlap (GR_POLY_STAT_TESTED of the header: whether or not
    the polygon has a ring of 3 or more vertices)."""
    boxes = table[4]
    pairs = {}
    for p in range(len(boxes)):
        if not polygon_has_rows(table, p):
            continue
        rings = polygon_rings(table, p)   # none usable (all shorter than 3 vertices): the pair is tested and adds nothing
        for f in candidate_faces(tri, boxes[p]):
            if face_class[f] < 0:
                continue
            t, o = ccw_triangle(tri[f])
            if o == 0:
                continue
            a2 = exact_intersection_area2(t, rings)
            pairs[(int(f), p)] = (a2 == o, a2, o)
    return pairs


def exact_class_weights(tri, face_class, face_weight, table, n_classes, within, pairs=None):
    """(P, C) float64: the exact rational sums (areas in square metres times the float weights taken as exact), rounded once."""
    pairs = exact_pairs(tri, face_class, table) if pairs is None else pairs
    sums = [[Fraction(0)] * n_classes for _ in range(len(table[4]))]
    for (f, p), (contained, a2, o) in pairs.items():
        if within and not contained:
            continue
        area = Fraction(o if within else a2, 2 * GRID2_PER_M2)
        sums[p][int(face_class[f])] += area * Fraction(float(face_weight[f]))
    return np.array([[float(v) for v in row] for row in sums], dtype=np.float64).reshape(len(table[4]), n_classes)


# -- (b) the float64 stand-in ---------------------------------------------------------------------------------------------------
def _sgn(v):
    return (v > 0) - (v < 0)


def edge_meets_interior(t, a, b, orient=_orient):
    """The device's predicate: does the closed segment a b meet the open interior of the counter-clockwise triangle t?"""
    s = [_sgn(orient(a[0], a[1], b[0], b[1], v[0], v[1])) for v in t]
    npos, nneg = sum(x > 0 for x in s), sum(x < 0 for x in s)
    if npos == 0 or nneg == 0:
        return False
    k = s.index(1 if npos == 1 else -1)
    p0, p1, p2 = t[k], t[(k + 1) % 3], t[(k + 2) % 3]
    f1a, f2a = _sgn(orient(*p0, *p1, *a)), _sgn(orient(*p2, *p0, *a))
    f1b, f2b = _sgn(orient(*p0, *p1, *b)), _sgn(orient(*p2, *p0, *b))
    return (f1a > 0 and f2a > 0) or (f1b > 0 and f2b > 0) or (f1a <= 0 and f2b <= 0) or (f1b <= 0 and f2a <= 0)


def within_standin(t, rings, orient=_orient):
    """No ring edge meets the open interior, and 3 x centroid is inside by the even-odd rule over all rings."""
    c3x, c3y = t[0][0] + t[1][0] + t[2][0], t[0][1] + t[1][1] + t[2][1]
    parity = 0
    for pts, _hole in rings:
        for i in range(len(pts)):
            a, b = pts[i - 1], pts[i]
            if (3 * a[1] > c3y) != (3 * b[1] > c3y):
                o = orient(3 * a[0], 3 * a[1], 3 * b[0], 3 * b[1], c3x, c3y)
                parity ^= int((o > 0) == (b[1] > a[1]))
            if edge_meets_interior(t, a, b, orient):
                return False
    return parity == 1


def wrapped_int64_orient(ax, ay, bx, by, cx, cy):
    """The orientation determinant as 64-bit two's-complement arithmetic would have it (every difference, every product and their
    difference wrap)."""
    def wrap(v):
        return (v + (1 << 63)) % (1 << 64) - (1 << 63)

    return wrap(wrap(wrap(bx - ax) * wrap(cy - ay)) - wrap(wrap(by - ay) * wrap(cx - ax)))


def within_wrapped64(t, rings):
    """A canary, not a checker: `within_standin` as a kernel that forgot the 128-bit type would decide.  The tests show with it
    that the large lattice scene tells such a kernel from the exact oracle."""
    return within_standin(t, rings, wrapped_int64_orient)


class _Stream:
    """The streamed clip of one ring: three half-plane stages with first / previous point each, then the shoelace sum."""

    def __init__(self, e1, e2):
        self.planes = [((0.0, 0.0), e1), (e1, (e2[0] - e1[0], e2[1] - e1[1])), (e2, (0.0 - e2[0], 0.0 - e2[1]))]
        self.first = [None, None, None]
        self.prev = [None, None, None]
        self.out_first = self.out_prev = None
        self.sum = 0.0

    def put(self, k, x, y):
        if k == 3:
            if self.out_first is None:
                self.out_first = (x, y)
            else:
                self.sum += self.out_prev[0] * y - x * self.out_prev[1]
            self.out_prev = (x, y)
            return
        (ax, ay), (ex, ey) = self.planes[k]
        d = ex * (y - ay) - ey * (x - ax)
        if self.first[k] is None:
            self.first[k] = (x, y, d)
        else:
            self.edge(k, self.prev[k], (x, y, d))
        self.prev[k] = (x, y, d)

    def edge(self, k, s, p):
        sx, sy, sd = s
        x, y, d = p
        if (d >= 0.0) != (sd >= 0.0):
            t = sd / (sd - d)
            self.put(k + 1, sx + t * (x - sx), sy + t * (y - sy))
        if d >= 0.0:
            self.put(k + 1, x, y)

    def close(self):
        for k in range(3):
            if self.first[k] is not None:
                self.edge(k, self.prev[k], self.first[k])
        if self.out_first is not None:
            self.sum += self.out_prev[0] * self.out_first[1] - self.out_first[0] * self.out_prev[1]
        return self.sum


def overlay_area_standin(t, rings):
    """area(triangle n polygon) in square metres in the device's operation order: metres relative to vertex 0, rings in table
    order, holes subtracted, 0.5 * sum."""
    x0, y0 = t[0]
    e1 = (float(t[1][0] - x0) * 1e-6, float(t[1][1] - y0) * 1e-6)
    e2 = (float(t[2][0] - x0) * 1e-6, float(t[2][1] - y0) * 1e-6)
    acc = 0.0
    for pts, hole in rings:
        st = _Stream(e1, e2)
        for x, y in pts:
            st.put(0, float(x - x0) * 1e-6, float(y - y0) * 1e-6)
        s = st.close()
        acc = acc - s if hole else acc + s
    return 0.5 * acc


def standin_pairs(tri, face_class, table, within):
    """{(face, polygon): contained (within) or the float area (overlay)} over the same pairs as `exact_pairs`."""
    boxes = table[4]
    pairs = {}
    for p in range(len(boxes)):
        if not polygon_has_rows(table, p):
            continue
        rings = polygon_rings(table, p)   # none usable (all shorter than 3 vertices): the pair is tested and adds nothing
        for f in candidate_faces(tri, boxes[p]):
            if face_class[f] < 0:
                continue
            t, o = ccw_triangle(tri[f])
            if o == 0:
                continue
            pairs[(int(f), p)] = within_standin(t, rings) if within else overlay_area_standin(t, rings)
    return pairs


def polygon_class_weights_np(tri, face_class, face_weight, table, n_classes, within, pairs=None):
    """((P, C) float64 weights summed in face order, stats (4,) int64) -- what gr_polygon_class_weights computes.  `pairs`: the
    `standin_pairs` of this mode where they are at hand, over at least the faces that take part."""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 6)
    face_class = np.asarray(face_class).astype(np.int64)
    face_class = np.where((face_class >= 0) & (face_class < n_classes), face_class, -1)
    face_weight = np.asarray(face_weight, dtype=np.float64)
    boxes = table[4]
    weights = np.zeros((len(boxes), n_classes), dtype=np.float64)
    pairs = standin_pairs(tri, face_class, table, within) if pairs is None else select_pairs(pairs, face_class, n_classes)
    contributing = 0
    for (f, p), got in sorted(pairs.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        if within:
            if not got:
                continue
            area = float(ccw_triangle(tri[f])[1]) / 2e12
        else:
            area = got
            if not area > 0.0:
                continue
        weights[p, face_class[f]] += area * float(face_weight[f])
        contributing += 1
    sizes = np.diff(np.asarray(table[1])) if len(table[1]) > 1 else np.zeros(0, dtype=np.int64)
    stats = np.array([len(pairs), contributing, int(sizes.max()) if sizes.size else 0, 0], dtype=np.int64)
    return weights, stats


# -- (c) the backend for host-logic tests -------------------------------------------------------------------------------------
def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


class StandInBackend:
    """`HipRaster.polygon_class_weights` on the CPU; records the arguments of the last call in `last`."""

    def polygon_class_weights(self, tri, face_class, face_weight, ring_vertices, ring_offsets, ring_polygon, ring_is_hole,
                              polygon_boxes, n_classes, within=True):
        table = tuple(_np(x) for x in (ring_vertices, ring_offsets, ring_polygon, ring_is_hole, polygon_boxes))
        self.last = dict(tri=_np(tri), face_class=_np(face_class), face_weight=_np(face_weight), table=table,
                         n_classes=n_classes, within=within)
        return polygon_class_weights_np(_np(tri), _np(face_class), _np(face_weight), table, int(n_classes), bool(within))


# -- (d) generated scenes shared by the host and the device tests ------------------------------------------------------------------
# Raw snapped tables for `HipRaster.polygon_class_weights`, so that coordinates near 2^40 and odd tables reach the kernel without
# the metre snap.  Everything is drawn on a lattice of LATTICE_NODES x LATTICE_NODES nodes, LATTICE_SUB sub-steps to the step, in
# Python integers; validity is CHECKED with integer tests (the exact oracle is an oracle for valid input only).
LATTICE_NODES = 7
LATTICE_SUB = 4
EMPTY_BOX = (1, 1, 0, 0)
SMALL = dict(scale=10 ** 6, offset=0)                       # steps of one metre
LARGE = dict(scale=15 * 10 ** 10, offset=10 ** 11)          # |q| <= 6 * 1.5e11 + 1e11 = 1e12 < 2^40; every lattice area >= 2^64
LATTICE_SEED = {"small": 7, "large": 7}   # chosen on the CPU: the category counts test_label_polygons_host.py asserts hold


def _on_segment(a, b, p):
    """p on the closed segment a b."""
    return _orient(*a, *b, *p) == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


def segments_meet(a, b, c, d):
    """Do the closed segments a b and c d share a point?"""
    o1, o2 = _sgn(_orient(*a, *b, *c)), _sgn(_orient(*a, *b, *d))
    o3, o4 = _sgn(_orient(*c, *d, *a)), _sgn(_orient(*c, *d, *b))
    if o1 * o2 < 0 and o3 * o4 < 0:
        return True
    return _on_segment(a, b, c) or _on_segment(a, b, d) or _on_segment(c, d, a) or _on_segment(c, d, b)


def ring_is_simple(pts):
    """Distinct vertices, consecutive edges share their vertex only, other edges share nothing, non-zero area."""
    n = len(pts)
    if n < 3 or len(set(pts)) != n or _area2_exact(pts) == 0:
        return False
    for i in range(n):
        a, b, c = pts[i - 1], pts[i], pts[(i + 1) % n]
        if _orient(*a, *b, *c) == 0 and (b[0] - a[0]) * (c[0] - b[0]) + (b[1] - a[1]) * (c[1] - b[1]) <= 0:
            return False   # the ring turns back on itself
        for j in range(i + 2, n):
            if (j + 1) % n == i:
                continue
            if segments_meet(pts[i], pts[(i + 1) % n], pts[j], pts[(j + 1) % n]):
                return False
    return True


def point_in_ring(pts, p):
    """1: strictly inside, 0: on the ring, -1: outside (even-odd, integers)."""
    parity = 0
    for i in range(len(pts)):
        a, b = pts[i - 1], pts[i]
        if _on_segment(a, b, p):
            return 0
        if (a[1] > p[1]) != (b[1] > p[1]) and (_orient(*a, *b, *p) > 0) == (b[1] > a[1]):
            parity ^= 1
    return 1 if parity else -1


def _edges_meet(r1, r2):
    return any(segments_meet(r1[i - 1], r1[i], r2[j - 1], r2[j]) for i in range(len(r1)) for j in range(len(r2)))


def ring_strictly_inside(inner, outer):
    """Every point of `inner` is strictly inside `outer`: no edges meet and the vertices are inside."""
    return not _edges_meet(inner, outer) and all(point_in_ring(outer, p) == 1 for p in inner)


def rings_apart(r1, r2):
    """The closed regions of two simple rings share no point: no edges meet and neither holds a vertex of the other."""
    return not _edges_meet(r1, r2) and point_in_ring(r1, r2[0]) == -1 and point_in_ring(r2, r1[0]) == -1


def has_contact(t, rings):
    """A ring vertex on the triangle's boundary or a triangle vertex on a ring edge (collinear overlapping edges have one of the
    two)."""
    for pts, _hole in rings:
        for i in range(len(pts)):
            if any(_on_segment(t[k], t[(k + 1) % 3], pts[i]) for k in range(3)):
                return True
            if any(_on_segment(pts[i - 1], pts[i], v) for v in t):
                return True
    return False


def _draw_ring(rng, x0, y0, w, h, step, min_area2=0):
    """A simple counter-clockwise ring of 3 to 8 vertices on multiples of `step` inside the window, as a list of int pairs: points
    drawn freely, ordered by angle about their mean, kept only if the integer tests call the result simple."""
    for _ in range(1000):
        k = int(rng.integers(3, 9))
        pts = {(x0 + step * int(rng.integers(0, w // step + 1)), y0 + step * int(rng.integers(0, h // step + 1))) for _ in range(k)}
        if len(pts) < 3:
            continue
        pts = sorted(pts)
        cx, cy = sum(p[0] for p in pts) / len(pts), sum(p[1] for p in pts) / len(pts)
        pts.sort(key=lambda p: np.arctan2(p[1] - cy, p[0] - cx))
        if ring_is_simple(pts) and _area2_exact(pts) > min_area2:
            return pts
    raise RuntimeError("no simple ring found")


def _draw_faces(rng, n, collapsed=0.0):
    """n triangles on the lattice nodes (sub-step units), half of them short (legs of 1-2 steps), either winding; a share
    `collapsed` has zero area (a repeated corner or three corners in line)."""
    s, top = LATTICE_SUB, LATTICE_SUB * (LATTICE_NODES - 1)
    out = []
    while len(out) < n:
        flat = rng.random() < collapsed
        if len(out) % 2 == 0:
            a = (s * int(rng.integers(0, LATTICE_NODES)), s * int(rng.integers(0, LATTICE_NODES)))
            b, c = ((a[0] + s * int(rng.integers(-2, 3)), a[1] + s * int(rng.integers(-2, 3))) for _ in range(2))
        else:
            a, b, c = ((s * int(rng.integers(0, LATTICE_NODES)), s * int(rng.integers(0, LATTICE_NODES))) for _ in range(3))
        if flat:
            c = a if rng.random() < 0.5 else (2 * b[0] - a[0], 2 * b[1] - a[1])
        if min(b + c) < 0 or max(b + c) > top or (_orient(*a, *b, *c) == 0) != flat:
            continue
        out.append(a + b + c)
    return out


def make_table(rows, n_polygons, unit=1, offset=0):
    """The raw table (ring_vertices (N, 2) int64, ring_offsets (R + 1,) int64, ring_polygon (R,) int32, ring_is_hole (R,) int32,
    polygon_boxes (P, 4) int64) of rows [(polygon, vertices in lattice units, is_hole)] in the given order; x -> x unit + offset,
    y -> y unit - offset.  A polygon's box is over the vertices of all its rows, however short; EMPTY_BOX without any."""
    verts, off, poly, hole = [], [0], [], []
    boxes = [None] * n_polygons
    for p, pts, is_hole in rows:
        pts = [(x * unit + offset, y * unit - offset) for x, y in pts]
        verts += pts
        off.append(len(verts))
        poly.append(p)
        hole.append(int(is_hole))
        if 0 <= p < n_polygons and pts:
            xs, ys = [q[0] for q in pts], [q[1] for q in pts]
            b = boxes[p]
            boxes[p] = (min(xs), min(ys), max(xs), max(ys)) if b is None else \
                (min(b[0], *xs), min(b[1], *ys), max(b[2], *xs), max(b[3], *ys))
    boxes = [EMPTY_BOX if b is None else b for b in boxes]
    return (np.array(verts, dtype=np.int64).reshape(-1, 2), np.array(off, dtype=np.int64), np.array(poly, dtype=np.int32),
            np.array(hole, dtype=np.int32), np.array(boxes, dtype=np.int64).reshape(n_polygons, 4))


def _draw_polygon(rng, kind):
    """[(ring, is_hole)] in lattice sub-steps: kind "plain", "holed" (a hole strictly inside the exterior, on the finest lattice) or
    "two_part" (a second exterior on the half-step lattice, apart from the first: neither overlapping nor touching)."""
    s, top = LATTICE_SUB, LATTICE_SUB * (LATTICE_NODES - 1)
    for _ in range(200):
        w, h = s * int(rng.integers(3, 7)), s * int(rng.integers(3, 7))
        x0, y0 = s * int(rng.integers(0, (top - w) // s + 1)), s * int(rng.integers(0, (top - h) // s + 1))
        ext = _draw_ring(rng, x0, y0, w, h, s, min_area2=8 * s * s)
        if kind == "plain":
            return [(ext, False)]
        xs, ys = [p[0] for p in ext], [p[1] for p in ext]
        for _ in range(200):
            if kind == "holed":
                side = int(rng.integers(2, 7))
                hx, hy = int(rng.integers(min(xs), max(xs) - side + 1)), int(rng.integers(min(ys), max(ys) - side + 1))
                other = _draw_ring(rng, hx, hy, side, side, 1)
                ok = ring_strictly_inside(other, ext)
            else:
                pw, ph = s * int(rng.integers(2, 4)), s * int(rng.integers(2, 4))
                px, py = (s // 2) * int(rng.integers(0, 2 * (top - pw) // s + 1)), (s // 2) * int(rng.integers(0, 2 * (top - ph) // s + 1))
                other = _draw_ring(rng, px, py, pw, ph, s // 2, min_area2=3 * s * s)
                ok = rings_apart(other, ext)
            if ok:
                return [(ext, False), (other, kind == "holed")]
    raise RuntimeError("no valid polygon found")


def lattice_scene(scale, offset, seed, n_faces=257, n_polygons=12):
    """(tri (F, 6) int64, table, info): triangles (half of them short, none collapsed, either winding) and polygons -- in turn
    plain, holed, two-part, plain -- on the lattice; every lattice coordinate times `scale`, then + offset in x and - offset in
    y.  Rings are simple and counter-clockwise with 3 to 8 vertices; holes lie strictly inside; the parts of a polygon are apart:
    all checked here with integer tests.  info: {"holed": rows, "two_part": rows}."""
    assert scale % LATTICE_SUB == 0
    rng = np.random.default_rng(seed)
    kinds = [("plain", "holed", "two_part", "plain")[p % 4] for p in range(n_polygons)]
    rows = []
    for p, kind in enumerate(kinds):
        rings = _draw_polygon(rng, kind)
        assert all(ring_is_simple(r) and _area2_exact(r) > 0 and 3 <= len(r) <= 8 for r, _ in rings)
        assert kind != "holed" or ring_strictly_inside(rings[1][0], rings[0][0])
        assert kind != "two_part" or rings_apart(rings[1][0], rings[0][0])
        rows += [(p, r, hole) for r, hole in rings]
    unit = scale // LATTICE_SUB
    tri = np.array(_draw_faces(rng, n_faces), dtype=np.int64).reshape(n_faces, 6) * unit
    tri[:, 0::2] += offset
    tri[:, 1::2] -= offset
    info = {"holed": [p for p, k in enumerate(kinds) if k == "holed"], "two_part": [p for p, k in enumerate(kinds) if k == "two_part"]}
    return tri, make_table(rows, n_polygons, unit, offset), info


WAVE_POLYGONS = 6
WAVE_FAR = 8   # lattice steps in x between the main lattice and the far polygon


WAVE_SEED = 12   # chosen on the CPU: the far polygon meets a face at every face count above 1, and the single face meets polygons


def wave_scene(n_faces, n_classes, seed=WAVE_SEED):
    """(tri, face_class (F,) int32, face_weight (F,) float64, table, info) on the small lattice, for the wave and workgroup structure
    and the raw-table contract.  The geometry depends on (n_faces, seed) only, the classes on n_classes too.
    Faces, in caller order: either winding; about one in eight collapsed; classes -1 and n_classes (both skipped) among the valid
    ones; weights in [0, 1] that include 0 (an area error is not scaled up).  With n_classes > 1 the last class is carried by
    collapsed faces only (info["idle_class"]).
    The first face and about a quarter of the rest of ONE run of 64 faces (info["far_run"]) lie WAVE_FAR steps to the right of the lattice.
    Table, WAVE_POLYGONS rows: 0 holed; 1 without rings; 2 plain; 3 whose only rings have 0, 1 and 2 vertices; 4 two-part; 5 small and
    far to the right, meeting only faces of the far run.  A ring row with ring_polygon = -1 lies between the runs of rows 0 and 2, one
    with ring_polygon = P between those of rows 3 and 4; both cover the whole lattice, so they would show if they were not ignored."""
    s, top, P = LATTICE_SUB, LATTICE_SUB * (LATTICE_NODES - 1), WAVE_POLYGONS
    rng = np.random.default_rng([seed, n_faces])
    holed, plain, two = _draw_polygon(rng, "holed"), _draw_polygon(rng, "plain"), _draw_polygon(rng, "two_part")
    far = _draw_ring(rng, s * WAVE_FAR, 0, 3 * s, 3 * s, s, min_area2=4 * s * s)
    whole = [(0, 0), (top, 0), (top, top), (0, top)]
    mid = s * (LATTICE_NODES // 2)
    rows = [(0, holed[0][0], False), (0, holed[1][0], True), (-1, whole, False), (2, plain[0][0], False),
            (3, [], False), (3, [(mid, mid)], False), (3, [(mid - s, mid), (mid + s, mid + s)], False), (P, whole, False),
            (4, two[0][0], False), (4, two[1][0], False), (5, far, False)]
    faces = _draw_faces(rng, n_faces, collapsed=0.125)
    far_run = min(1, (n_faces - 1) // 64)
    for f in range(64 * far_run, min(64 * far_run + 64, n_faces)):
        if rng.random() < 0.25 or (f == 64 * far_run and n_faces > 1):
            faces[f] = tuple(v + (s * WAVE_FAR if k % 2 == 0 else 0) for k, v in enumerate(faces[f]))
    unit = SMALL["scale"] // s
    tri = np.array(faces, dtype=np.int64).reshape(n_faces, 6) * unit
    weight = np.where(rng.random(n_faces) < 0.15, 0.0, np.where(rng.random(n_faces) < 0.3, 1.0, rng.uniform(0.1, 1.0, n_faces)))
    rng = np.random.default_rng([seed, n_faces, n_classes])
    idle = n_classes - 1 if n_classes > 1 else None
    n_used = n_classes - 1 if n_classes > 1 else 1
    u = rng.random(n_faces)
    cls = np.where(u < 0.1, -1, np.where(u < 0.2, n_classes, rng.integers(0, n_used, n_faces)))
    flat = np.array([_orient(*f) == 0 for f in faces])
    if idle is not None:
        cls[flat] = idle
    solid = np.nonzero(~flat)[0]
    if len(solid) >= 8:   # every kind is there, whatever was drawn
        cls[solid[1]], cls[solid[2]], weight[solid[3]] = -1, n_classes, 0.0
    info = {"idle_class": idle, "far_run": far_run, "far_polygon": 5, "no_usable_rings": [1, 3], "collapsed": flat}
    return tri, cls.astype(np.int32), weight, make_table(rows, P, unit), info


@functools.lru_cache(maxsize=None)
def lattice_case(name):
    """The lattice scene "small" or "large" with its answers, computed once per process: dict of tri, table, info, exact
    (`exact_pairs`), within and overlay (`standin_pairs`) over all faces labelled, and e_scene = the largest |stand-in - exact|
    overlay area of a pair in square metres -- what the device's overlay tolerance on this scene is built from."""
    tri, table, info = lattice_scene(seed=LATTICE_SEED[name], **{"small": SMALL, "large": LARGE}[name])
    return _case(tri, table, info)


@functools.lru_cache(maxsize=None)
def wave_case(n_faces, seed=WAVE_SEED):
    """The geometry of `wave_scene(n_faces, *, seed)` with its answers as in `lattice_case` (every face taken as labelled: the pairs
    do not depend on the classes)."""
    tri, _cls, _w, table, info = wave_scene(n_faces, 1, seed)
    return _case(tri, table, info)


def _case(tri, table, info):
    labelled = np.zeros(len(tri), dtype=np.int64)
    exact = exact_pairs(tri, labelled, table)
    overlay = standin_pairs(tri, labelled, table, False)
    e_scene = max([Fraction(0)] + [abs(Fraction(overlay[k]) - exact[k][1] / (2 * GRID2_PER_M2)) for k in exact])
    return dict(tri=tri, table=table, info=info, exact=exact, within=standin_pairs(tri, labelled, table, True), overlay=overlay,
                e_scene=float(e_scene))


def select_pairs(pairs, face_class, n_classes):
    """The pairs of the faces whose class is in [0, n_classes)."""
    return {k: v for k, v in pairs.items() if 0 <= face_class[k[0]] < n_classes}
