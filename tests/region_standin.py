"""Checker of gr_points_in_region / gr_submesh_extract (DESIGN.md "Region of interest", Q3-Q6), on the host and by another method
than the device's:

* containment through `vector_standin.row_contains` (Python integers, the ray along +y, the boundary by dot products), every row
  tried for every point;
* the buffer by the clamped parameter t = clamp(u.e / L2, 0, 1) and the exact squared distance to a + t e as a
  `fractions.Fraction`, compared with D^2 -- the device never divides: it compares cross^2 with D^2 L2 in 256 bits;
* the sub-mesh by plain Python loops.

Only the count of wide comparisons follows the device's order of visits (the rule of Q4: edges in table order, while the point is
neither contained nor within D of an earlier edge); the decisions do not depend on it.

`points_in_region_np` also reports each point's case, so tests can require the hard ones.  `StandInBackend` has the two `HipRaster`
methods on the CPU, for host-logic tests.
"""
from fractions import Fraction

import numpy as np

import vector_standin as vs

STAT_WORDS = 4   # inside, inside by the buffer only, wide comparisons (the device's block)
CASES = ("on_ring", "two_rows", "in_hole_outside", "in_hole_within_D", "at_D_edge", "at_D_vertex", "one_step_beyond")


def _edges(table):
    """(E, 4) int64 ax ay bx by of every edge of every ring with at least 3 vertices, in table order, and per row its rings as
    vector_standin wants them (coordinates times 3)."""
    rv, roff, rpoly = table[0], table[1], table[2]
    out = []
    for r in range(len(rpoly)):
        pts = [(int(x), int(y)) for x, y in rv[int(roff[r]):int(roff[r + 1])]]
        if len(pts) >= 3:
            out += [(*pts[i - 1], *pts[i]) for i in range(len(pts))]
    return np.array(out, dtype=np.int64).reshape(-1, 4), vs._rings_of_rows(table)


def distance2(px, py, ax, ay, bx, by):
    """(exact squared distance from the point to the closed edge as a Fraction, t): the clamped parameter of the nearest point."""
    ux, uy, ex, ey = px - ax, py - ay, bx - ax, by - ay
    L2 = ex * ex + ey * ey
    t = Fraction(0) if L2 == 0 else min(max(Fraction(ux * ex + uy * ey, L2), Fraction(0)), Fraction(1))
    dx, dy = ux - t * ex, uy - t * ey
    return dx * dx + dy * dy, t


def _wide_count(px, py, table, D, rows3):
    """256-bit comparisons the device forms for this point (Q4's order of visits)."""
    rv, roff, rpoly, _, boxes = table
    wide, near, r, R = 0, False, 0, len(rpoly)
    while r < R:
        row = int(rpoly[r])
        r1 = r
        while r1 < R and int(rpoly[r1]) == row:
            r1 += 1
        b = [int(v) for v in boxes[row]]
        if b[0] <= b[2] and b[1] <= b[3] and b[0] - D <= px <= b[2] + D and b[1] - D <= py <= b[3] + D:
            for q in range(r, r1):
                pts = [(int(x), int(y)) for x, y in rv[int(roff[q]):int(roff[q + 1])]]
                if len(pts) < 3:
                    continue
                for i in range(len(pts)):
                    (ax, ay), (bx, by) = pts[i - 1], pts[i]
                    if vs.on_ring([(ax, ay), (bx, by)], px, py):
                        return wide
                    if D > 0 and not near and min(ax, bx) - D <= px <= max(ax, bx) + D and min(ay, by) - D <= py <= max(ay, by) + D:
                        d2, t = distance2(px, py, ax, ay, bx, by)
                        wide += 1 if 0 < t < 1 else 0
                        near = d2 <= D * D
            if row in rows3 and vs.row_contains(rows3[row], 3 * px, 3 * py)[0]:
                return wide
        r = r1
    return wide


def points_in_region_np(points_q, table, D):
    """(mask (N,) bool, info): Q3 or Q4.  info: the (N,) bool arrays of CASES, "contained", "near", "wide" (N,) int64 (the wide comparisons per point) and "stats" (STAT_WORDS,) int64.
    `table` is the snapped ring table of `PlanarPolygons.snapped`, D the buffer in grid steps."""
    points_q = np.asarray(points_q, dtype=np.int64).reshape(-1, 2)
    D = int(D)
    boxes = np.asarray(table[4], dtype=np.int64).reshape(-1, 4)
    edges, rows3 = _edges(table)
    N = len(points_q)
    info = {k: np.zeros(N, dtype=bool) for k in CASES + ("contained", "near")}
    info["wide"] = np.zeros(N, dtype=np.int64)
    for i in range(N):
        px, py = int(points_q[i, 0]), int(points_q[i, 1])
        n_rows, in_hole = 0, False
        for p in np.nonzero((boxes[:, 0] <= px) & (px <= boxes[:, 2]) & (boxes[:, 1] <= py) & (py <= boxes[:, 3]))[0]:
            rings = rows3.get(int(p))
            if not rings:
                continue
            inside, edge = vs.row_contains(rings, 3 * px, 3 * py)
            n_rows += inside
            info["on_ring"][i] |= edge
            if not inside:
                in_hole |= any(hole and vs.crossings_above(pts, 3 * px, 3 * py) % 2 == 1 for pts, hole in rings)
        # the edges that can be within D + 1 of the point: everything the classification needs; the rest is farther
        best, best_t = None, []
        if len(edges):
            lo, hi = np.minimum(edges[:, :2], edges[:, 2:]), np.maximum(edges[:, :2], edges[:, 2:])
            m = D + 1
            cand = np.nonzero((lo[:, 0] - m <= px) & (px <= hi[:, 0] + m) & (lo[:, 1] - m <= py) & (py <= hi[:, 1] + m))[0]
            for e in cand:
                ax, ay, bx, by = (int(v) for v in edges[e])
                d2, t = distance2(px, py, ax, ay, bx, by)
                degenerate = (ax, ay) == (bx, by)
                if best is None or d2 < best:
                    best, best_t = d2, [(t, degenerate)]
                elif d2 == best:
                    best_t.append((t, degenerate))
        near = D > 0 and best is not None and best <= D * D
        contained = n_rows > 0
        info["contained"][i], info["near"][i] = contained, near
        info["two_rows"][i] = n_rows >= 2
        info["in_hole_outside"][i] = in_hole and not contained and not near
        info["in_hole_within_D"][i] = in_hole and not contained and near
        if D > 0 and not contained and best is not None:
            if best == D * D:
                interior = any(0 < t < 1 for t, deg in best_t)
                info["at_D_edge"][i] = interior
                info["at_D_vertex"][i] = not interior
            info["one_step_beyond"][i] = D * D < best <= (D + 1) * (D + 1)
        info["wide"][i] = _wide_count(px, py, table, D, rows3)
    mask = info["contained"] | info["near"]
    info["stats"] = np.array([int(mask.sum()), int((info["near"] & ~info["contained"]).sum()), int(info["wide"].sum()), 0], dtype=np.int64)
    return mask, info


def submesh_np(mask, faces):
    """(face_ids int64, point_ids int64, new_faces (n, 3) int32, bad faces): Q5 and Q6 by loops."""
    mask = np.asarray(mask).reshape(-1)
    V = len(mask)
    face_ids, used, bad = [], set(), 0
    for f, tri in enumerate(np.asarray(faces).reshape(-1, 3).tolist()):
        if any(v < 0 or v >= V for v in tri):
            bad += 1
        elif any(mask[v] for v in tri):
            face_ids.append(f)
            used.update(tri)
    point_ids = sorted(used)
    place = {v: k for k, v in enumerate(point_ids)}
    new_faces = [[place[v] for v in np.asarray(faces).reshape(-1, 3)[f].tolist()] for f in face_ids]
    return (np.array(face_ids, dtype=np.int64), np.array(point_ids, dtype=np.int64),
            np.array(new_faces, dtype=np.int32).reshape(-1, 3), bad)


class StandInBackend:
    """`HipRaster.points_in_region` and `HipRaster.submesh_extract` on the CPU; records the arguments of the last calls."""

    def points_in_region(self, points_q, ring_vertices, ring_offsets, ring_polygon, ring_is_hole, polygon_boxes, buffer_steps=0):
        table = tuple(vs._np(x) for x in (ring_vertices, ring_offsets, ring_polygon, ring_is_hole, polygon_boxes))
        D = int(buffer_steps)
        if not 0 <= D < 2 ** 40:
            raise ValueError(f"gr_points_in_region: buffer D={D} outside [0, 2^40) grid steps")
        self.last_region = dict(points_q=vs._np(points_q), table=table, D=D)
        mask, info = points_in_region_np(vs._np(points_q), table, D)
        return mask, info["stats"]

    def submesh_extract(self, mask, faces, check=True):
        mask, faces = vs._np(mask), vs._np(faces)
        self.last_submesh = dict(mask=mask, faces=faces)
        face_ids, point_ids, new_faces, bad = submesh_np(mask, faces)
        if check and bad:
            raise ValueError(f"gr_submesh_extract: {bad} faces name a vertex outside [0, {len(mask)})")
        return face_ids, point_ids, new_faces, np.array([len(face_ids), len(point_ids), bad], dtype=np.int64)


# -- scenes shared by the host and the device tests ----------------------------------------------------------------------------
STEP = 1e-6      # one grid step, in metres
HAND_D = 2.5     # metres


def hand_scene():
    """The hand-worked scene: (PlanarPolygons, [((x, y), in the region with D = 2.5 m, in the region with D = 0, what it is)]).
    row 0: the square (0, 0)-(20, 20) with the square hole (5, 5)-(15, 15); row 1: the square (18, 18)-(26, 26) over row 0's corner;
    row 2: the triangle (40, 0) (46, 0) (46, 8), whose edge (46, 8)-(40, 0) runs along (3, 4): its outward unit normal is
    (-4, 3) / 5, so 0.5 (-4, 3) = (-2, 1.5) is exactly 2.5 m long; (1.5, 2.0) is too."""
    from geograypher_amd.utils.geometric import PlanarPolygons

    polygons = PlanarPolygons(
        [vs.square(0, 0, 20, 20), vs.square(5, 5, 15, 15), vs.square(18, 18, 26, 26), np.array([[40.0, 0.0], [46.0, 0.0], [46.0, 8.0]])],
        [0, 0, 1, 2], [False, True, False, False])
    s = STEP
    cases = [
        ((2.0, 2.0), True, True, "strictly inside row 0"),
        ((0.0, 10.0), True, True, "on row 0's exterior ring"),
        ((5.0, 10.0), True, True, "on the hole's ring"),
        ((15.0, 15.0), True, True, "on the hole's vertex"),
        ((10.0, 10.0), False, False, "in the hole, 5 m from its ring"),
        ((7.0, 10.0), True, False, "in the hole, 2 m from its ring: the buffer grows into holes"),
        ((7.5, 10.0), True, False, "in the hole, exactly 2.5 m from its ring"),
        ((7.5 + s, 10.0), False, False, "... one grid step farther"),
        ((19.0, 19.0), True, True, "in rows 0 and 1: a union, not an xor"),
        ((24.0, 24.0), True, True, "in row 1 only"),
        ((10.0, -2.5), True, False, "exactly 2.5 m below row 0's bottom edge"),
        ((10.0, -2.5 - s), False, False, "... one grid step farther"),
        ((10.0, -2.5 + s), True, False, "... one grid step nearer"),
        ((41.0, 5.5), True, False, "exactly 2.5 m from the slanted edge: its point (43, 4) + 0.5 (-4, 3)"),
        ((41.0 - s, 5.5), False, False, "... one grid step farther in x"),
        ((41.0, 5.5 + s), False, False, "... one grid step farther in y"),
        ((41.0 + s, 5.5), True, False, "... one grid step nearer"),
        ((47.5, 10.0), True, False, "exactly 2.5 m from the corner (46, 8): offset (1.5, 2.0)"),
        ((47.5 + s, 10.0), False, False, "... one grid step farther in x"),
        ((47.5, 10.0 + s), False, False, "... one grid step farther in y"),
        ((47.5 - s, 10.0), True, False, "... one grid step nearer"),
        ((48.5, 4.0), True, False, "outside the joint box by exactly 2.5 m"),
        ((48.5 + s, 4.0), False, False, "outside the joint box by one grid step more than 2.5 m"),
        ((44.0, 2.0), True, True, "inside the triangle"),
        ((43.0, 4.0), True, True, "on the slanted edge"),
        ((33.0, 4.0), False, False, "between the rows, far from all"),
        ((100.0, 100.0), False, False, "outside everything"),
    ]
    return polygons, cases


def strip_mesh(n=6):
    """A strip of 2 n triangles over the vertices (i, 0) and (i, 1), i = 0..n, plus one vertex (0.5, 0.5) that no face uses:
    (points (2 n + 3, 3) float64, faces (2 n, 3) int64).  Vertex 2 i is (i, 0), vertex 2 i + 1 is (i, 1), the last is the loose one."""
    pts = [(float(i), float(j), 0.0) for i in range(n + 1) for j in (0, 1)] + [(0.5, 0.5, 0.0)]
    faces = []
    for i in range(n):
        faces += [(2 * i, 2 * i + 2, 2 * i + 1), (2 * i + 1, 2 * i + 2, 2 * i + 3)]
    return np.array(pts, dtype=np.float64), np.array(faces, dtype=np.int64)


RANDOM_SEED = 5   # chosen on the CPU: the stand-in alone meets the case counts the device test asserts
RANDOM_D = 2500000   # 2.5 m


def random_scene(seed=RANDOM_SEED, n_points=4000, n_faces=8000, n_rows=40, extent=160.0):
    """(points_q (4000, 2) int64, faces (8000, 3) int32, ring table): 40 rows on a 0.5 m lattice -- every fourth a rectangle with a
    large hole, every fourth a rectangle with sides along (3, 4) and (-4, 3), the others plain rectangles, overlapping where
    they happen to --, and points of four kinds: lattice points anywhere, lattice points on the rings, lattice points at offsets
    of length exactly 2.5 m from ring vertices ((+-2.5, 0), (0, +-2.5), (+-1.5, +-2), (+-2, +-1.5)), and copies of those one grid
    step away, and lattice points deep inside the holes.  Faces join points that are near one another in the array; some points are used by no face."""
    from geograypher_amd.utils.geometric import PlanarPolygons, snap_to_grid

    rng = np.random.default_rng(seed)
    rings, rows, holes = [], [], []
    for p in range(n_rows):
        c = np.round(rng.uniform(12.0, extent - 12.0, 2) * 2.0) / 2.0
        if p % 4 == 1:
            m, n = (0.5 * rng.integers(2, 6, 2)).tolist()
            a = np.array([3.0, 4.0]) * m
            b = np.array([-4.0, 3.0]) * n
            ring = np.array([c, c + a, c + a + b, c + b])
        else:
            half = np.round(rng.uniform(6.0 if p % 4 == 0 else 2.0, 9.0, 2) * 2.0) / 2.0
            ring = vs.square(c[0] - half[0], c[1] - half[1], c[0] + half[0], c[1] + half[1])
            if p % 4 == 0:
                inner = np.round(half * 0.7 * 2.0) / 2.0
                rings.append(ring); rows.append(p); holes.append(False)
                ring = vs.square(c[0] - inner[0], c[1] - inner[1], c[0] + inner[0], c[1] + inner[1])
                rings.append(ring); rows.append(p); holes.append(True)
                continue
        rings.append(ring); rows.append(p); holes.append(False)
    polygons = PlanarPolygons(rings, rows, holes, n_polygons=n_rows)

    offsets = np.array([(2.5, 0), (-2.5, 0), (0, 2.5), (0, -2.5)] + [(sx * a, sy * b) for a, b in ((1.5, 2.0), (2.0, 1.5))
                                                                      for sx in (1, -1) for sy in (1, -1)])
    on_ring, at_D, cores = [], [], []
    for ring, hole in zip(polygons.rings, polygons.ring_is_hole):
        at_D.append((ring[:, None, :] + offsets[None]).reshape(-1, 2))            # around every ring vertex
        for i in range(len(ring)):
            a, b = ring[i - 1], ring[i]
            k = int(round(np.abs(b - a).max() / (1.5 if (a[0] != b[0] and a[1] != b[1]) else 0.5)))
            along = a + (b - a) * (np.arange(k + 1) / max(k, 1))[:, None]     # lattice points of the edge
            on_ring.append(along)
            pick = along[rng.permutation(len(along))[:4]]
            at_D.append((pick[:, None, :] + offsets[None]).reshape(-1, 2))
        if hole:   # lattice points of the hole's core, farther than 2.5 m from its ring
            lo, hi = ring.min(axis=0) + 3.0, ring.max(axis=0) - 3.0
            if np.all(hi >= lo):
                cores.append(np.round(rng.uniform(lo, hi, (24, 2)) * 2.0) / 2.0)
    on_ring, at_D, cores = np.concatenate(on_ring), np.concatenate(at_D), np.concatenate(cores)
    on_ring = on_ring[rng.permutation(len(on_ring))[:300]]
    at_D = at_D[rng.permutation(len(at_D))[:1200]]
    n_free = n_points - len(on_ring) - 2 * len(at_D) - len(cores)
    free = np.round(rng.uniform(0.0, extent, (n_free, 2)) * 2.0) / 2.0
    q = snap_to_grid(np.concatenate([free, cores, on_ring, at_D]))
    steps = np.array([(1, 0), (-1, 0), (0, 1), (0, -1)], dtype=np.int64)[rng.integers(0, 4, len(at_D))]
    q = np.concatenate([q, snap_to_grid(at_D) + steps])
    # order by a coarse cell, so that the faces below join neighbours and the kept part of the mesh is a patchwork
    cell = (q // 8000000)
    order = np.lexsort((rng.random(len(q)), cell[:, 0], cell[:, 1]))
    q = q[order]
    first = rng.integers(0, n_points, n_faces)
    faces = np.stack([first, (first + rng.integers(1, 9, n_faces)) % n_points, (first + rng.integers(9, 17, n_faces)) % n_points],
                     axis=1).astype(np.int32)
    bounds = polygons.bounds_snapped()
    lo, hi = np.minimum(q.min(axis=0), bounds[0]), np.maximum(q.max(axis=0), bounds[1])
    origin = lo + (hi - lo) // 2
    return np.ascontiguousarray(q - origin), faces, polygons.snapped(origin)


# -- the wide-product trap ------------------------------------------------------------------------------------------------------
def truncated_128_decision(px, py, ax, ay, bx, by, D):
    """Q4's perpendicular case with both products cut to their low 128 bits."""
    ux, uy, ex, ey = px - ax, py - ay, bx - ax, by - ay
    c = ex * uy - ey * ux
    m = (1 << 128) - 1
    return ((c * c) & m) <= ((D * D * (ex * ex + ey * ey)) & m)


def float64_decision(px, py, ax, ay, bx, by, D):
    """Q4's perpendicular case in float64."""
    ux, uy, ex, ey = (np.float64(v) for v in (px - ax, py - ay, bx - ax, by - ay))
    c = ex * uy - ey * ux
    return bool(c * c <= np.float64(D) * np.float64(D) * (ex * ex + ey * ey))


def wide_trap():
    """(ring table, D, points_q (2, 2) int64 -- the outer point first --, the long edge): one triangle with an edge 2^41 grid steps
    long that rises 3 steps over its length, D = 2^39, and two points one grid step apart in x on either side of the line at
    distance D from that edge, a third of the way along it.  D^2 L2 = 2^160 + 9 2^78 and D |e| = 2^80 + 1.125: the inner point's
    cross product is 2^80 - 1, the outer point's 2^80 + 2.  Cut to 128 bits, the inner point's square (just below 2^160) looks
    huge and the point falls out; in float64 both cross products round to 2^80 and the outer point falls in."""
    from geograypher_amd.utils.geometric import PlanarPolygons  # noqa: F401  (the table is built by hand: the ring is too large for metres)

    ax, ay, bx, by = -(1 << 40), 0, 1 << 40, 3
    D = 1 << 39
    ring = np.array([[ax, ay], [bx, by], [0, -(1 << 20)]], dtype=np.int64)   # counter-clockwise? the area's sign is checked below
    x, y = ring[:, 0].astype(object), ring[:, 1].astype(object)
    area2 = sum(x[i - 1] * y[i] - x[i] * y[i - 1] for i in range(3))
    if area2 < 0:
        ring = ring[::-1].copy()
    table = (ring, np.array([0, 3], dtype=np.int64), np.array([0], dtype=np.int32), np.array([0], dtype=np.int32),
             np.array([[ring[:, 0].min(), ring[:, 1].min(), ring[:, 0].max(), ring[:, 1].max()]], dtype=np.int64))
    ex, ey = bx - ax, by - ay
    py = ay + D + 1
    # the x at which the point crosses the offset line: the largest ux with cross^2 > D^2 L2 is outside, ux + 1 inside
    lo, hi = 0, ex
    L2 = ex * ex + ey * ey

    def outside(ux):
        c = ex * (py - ay) - ey * ux
        return c * c > D * D * L2

    assert outside(lo) and not outside(hi // 2 + hi // 4)
    hi = hi // 2 + hi // 4
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if outside(mid) else (lo, mid)
    points = np.array([[ax + lo, py], [ax + hi, py]], dtype=np.int64)
    return table, D, points, (ax, ay, bx, by)
