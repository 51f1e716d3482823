"""Checkers of gr_polygon_class_weights / label_polygons (DESIGN.md "Polygon labels"), all on the host:

(a) an EXACT oracle in Python integers and `fractions.Fraction`: the intersection of a snapped triangle with a polygon is clipped
    in rational arithmetic (list-based Sutherland-Hodgman of every ring against the triangle), so areas are exact, and the
    containment decision is `area(T n P) == area(T)` -- deliberately not the device's method (sign tests of ring edges against
    the open triangle plus an even-odd test of the centroid);
(b) a float64 stand-in that follows the device's operation order for the overlay area (Python floats: every operation rounded
    on its own, like the library built with -ffp-contract=off) and restates its sign predicates in Python integers;
(c) `StandInBackend`, the `HipRaster.polygon_class_weights` interface over (b), for host-logic tests without a GPU.

All three take the snapped table of `PlanarPolygons.snapped` and (F, 6) integer triangles.
"""
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
    every pair of a labelled, uncollapsed face and a polygon whose boxes overlap."""
    boxes = table[4]
    pairs = {}
    for p in range(len(boxes)):
        rings = polygon_rings(table, p)
        if not rings:
            continue
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


def edge_meets_interior(t, a, b):
    """The device's predicate: does the closed segment a b meet the open interior of the counter-clockwise triangle t?"""
    s = [_sgn(_orient(a[0], a[1], b[0], b[1], v[0], v[1])) for v in t]
    npos, nneg = sum(x > 0 for x in s), sum(x < 0 for x in s)
    if npos == 0 or nneg == 0:
        return False
    k = s.index(1 if npos == 1 else -1)
    p0, p1, p2 = t[k], t[(k + 1) % 3], t[(k + 2) % 3]
    f1a, f2a = _sgn(_orient(*p0, *p1, *a)), _sgn(_orient(*p2, *p0, *a))
    f1b, f2b = _sgn(_orient(*p0, *p1, *b)), _sgn(_orient(*p2, *p0, *b))
    return (f1a > 0 and f2a > 0) or (f1b > 0 and f2b > 0) or (f1a <= 0 and f2b <= 0) or (f1b <= 0 and f2a <= 0)


def within_standin(t, rings):
    """No ring edge meets the open interior, and 3 x centroid is inside by the even-odd rule over all rings."""
    c3x, c3y = t[0][0] + t[1][0] + t[2][0], t[0][1] + t[1][1] + t[2][1]
    parity = 0
    for pts, _hole in rings:
        for i in range(len(pts)):
            a, b = pts[i - 1], pts[i]
            if (3 * a[1] > c3y) != (3 * b[1] > c3y):
                o = _orient(3 * a[0], 3 * a[1], 3 * b[0], 3 * b[1], c3x, c3y)
                parity ^= int((o > 0) == (b[1] > a[1]))
            if edge_meets_interior(t, a, b):
                return False
    return parity == 1


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
        rings = polygon_rings(table, p)
        if not rings:
            continue
        for f in candidate_faces(tri, boxes[p]):
            if face_class[f] < 0:
                continue
            t, o = ccw_triangle(tri[f])
            if o == 0:
                continue
            pairs[(int(f), p)] = within_standin(t, rings) if within else overlay_area_standin(t, rings)
    return pairs


def polygon_class_weights_np(tri, face_class, face_weight, table, n_classes, within):
    """((P, C) float64 weights summed in face order, stats (4,) int64) -- what gr_polygon_class_weights computes."""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 6)
    face_class = np.asarray(face_class).astype(np.int64)
    face_class = np.where((face_class >= 0) & (face_class < n_classes), face_class, -1)
    face_weight = np.asarray(face_weight, dtype=np.float64)
    boxes = table[4]
    weights = np.zeros((len(boxes), n_classes), dtype=np.float64)
    pairs = standin_pairs(tri, face_class, table, within)
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
