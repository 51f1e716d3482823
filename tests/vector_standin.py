"""Checker of gr_face_polygon_index / vector textures (DESIGN.md "Vector textures", V3-V5), on the host and by another method than
the device's:

* every row is tried for every face -- no cell grid; a vectorised box test only spares the ring walk of rows whose box cannot hold
  the centre --, in Python integers (no overflow, no 128-bit emulation);
* even-odd with the ray along +y and the half-open rule in x (the device shoots along +x, half-open in y): off the boundary the
  parity does not depend on the ray, so the device's handling of ring vertices and horizontal edges is checked, not copied;
* its own boundary test (collinear and between the end points, by dot product -- the device compares against the edge's box).

`face_polygon_index_np` also reports what kind of case each face is (on a boundary, in several rows, in a hole), so that tests can
require the hard cases to be present.  `StandInBackend` is `HipRaster.face_polygon_index` on the CPU, for host-logic tests.
"""
import numpy as np

STAT_WORDS = 4   # tested, labelled, longest list, bad faces (the device's block)


def _orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def _rings_of_rows(table):
    """{row: [(vertices as int pairs times 3, is_hole)]} for rows with rings."""
    rv, roff, rpoly, rhole = table[:4]
    out = {}
    for r in range(len(rpoly)):
        pts = [(3 * int(x), 3 * int(y)) for x, y in rv[int(roff[r]):int(roff[r + 1])]]
        if len(pts) >= 3:
            out.setdefault(int(rpoly[r]), []).append((pts, bool(rhole[r])))
    return out


def on_ring(pts, px, py, orient=_orient):
    """Is the point on an edge or vertex of the ring?  Collinear with the edge and between its ends (dot products); an edge of
    no length (a repeated vertex) is its one point."""
    for i in range(len(pts)):
        (ax, ay), (bx, by) = pts[i - 1], pts[i]
        if (ax, ay) == (bx, by):
            if (px, py) == (ax, ay):
                return True
        elif orient(ax, ay, bx, by, px, py) == 0:
            d = (px - ax) * (bx - ax) + (py - ay) * (by - ay)
            if 0 <= d <= (bx - ax) ** 2 + (by - ay) ** 2:
                return True
    return False


def crossings_above(pts, px, py, orient=_orient):
    """Edges the ray from the point along +y crosses, half-open in x: an edge counts when exactly one end has x > px and the
    point is strictly below it."""
    n = 0
    for i in range(len(pts)):
        (ax, ay), (bx, by) = pts[i - 1], pts[i]
        if (ax > px) != (bx > px):
            if ax > bx:
                ax, ay, bx, by = bx, by, ax, ay
            if orient(ax, ay, bx, by, px, py) < 0:   # right of the edge taken in the direction of rising x: below it
                n += 1
    return n


def row_contains(rings, px, py, orient=_orient):
    """(inside the closed region, on a ring) of one row: V4."""
    if any(on_ring(pts, px, py, orient) for pts, _ in rings):
        return True, True
    return sum(crossings_above(pts, px, py, orient) for pts, _ in rings) % 2 == 1, False


def face_polygon_index_np(verts_q, faces, table, orient=_orient):
    """(face_polygon (F,) int32, info): the highest row whose closed region holds 3 x centre = the sum of the face's three snapped
    vertices, -1 for none; info = {"on_boundary", "multi", "in_hole": (F,) bool arrays, "tested": box hits}.  `table` is the
    snapped ring table of `PlanarPolygons.snapped`; `orient` can be replaced to ask what another arithmetic would have decided."""
    verts_q = np.asarray(verts_q, dtype=np.int64).reshape(-1, 2)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    boxes = 3 * np.asarray(table[4], dtype=np.int64).reshape(-1, 4)
    rows = _rings_of_rows(table)
    c3 = verts_q[faces].sum(axis=1)
    F = len(faces)
    out = np.full(F, -1, dtype=np.int32)
    info = {k: np.zeros(F, dtype=bool) for k in ("on_boundary", "multi", "in_hole")}
    tested = 0
    for f in range(F):
        px, py = int(c3[f, 0]), int(c3[f, 1])
        hits = 0
        cand = np.nonzero((boxes[:, 0] <= px) & (px <= boxes[:, 2]) & (boxes[:, 1] <= py) & (py <= boxes[:, 3]))[0]
        for p in cand:
            rings = rows.get(int(p))
            if not rings:
                continue
            tested += 1
            inside, edge = row_contains(rings, px, py, orient)
            if edge:
                info["on_boundary"][f] = True
            if inside:
                hits += 1
                out[f] = p   # candidates rise: the last one that holds the centre is the highest
            else:
                info["in_hole"][f] |= any(hole and not on_ring(pts, px, py, orient) and crossings_above(pts, px, py, orient) % 2 == 1
                                          for pts, hole in rings)
        info["multi"][f] = hits >= 2
    info["tested"] = tested
    return out, info


def wrapped_int64_orient(ax, ay, bx, by, cx, cy):
    """The orientation determinant as 64-bit two's-complement arithmetic would have it (every product and the difference wrap)."""
    def wrap(v):
        return (v + (1 << 63)) % (1 << 64) - (1 << 63)

    return wrap(wrap(wrap(bx - ax) * wrap(cy - ay)) - wrap(wrap(by - ay) * wrap(cx - ax)))


def device_rule_contains(rings, px, py, orient=_orient):
    """V4 as the DEVICE evaluates it (ray along +x, half-open in y, boundary by the edge's box).  Not used to check the device --
    that is `row_contains`, by the other ray --, only with `wrapped_int64_orient`, to show that the determinants the device forms
    would decide wrongly in 64 bits."""
    parity = 0
    for pts, _ in rings:
        for i in range(len(pts)):
            (ax, ay), (bx, by) = pts[i - 1], pts[i]
            cross = (ay <= py) != (by <= py)
            in_box = min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by)
            if cross or in_box:
                o = orient(ax, ay, bx, by, px, py)
                if o == 0 and in_box:
                    return True
                if cross and (o > 0) == (by > ay):
                    parity ^= 1
    return parity == 1


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


class StandInBackend:
    """`HipRaster.face_polygon_index` on the CPU (the cell table is accepted and ignored: the answer must not depend on it);
    records the arguments of the last call in `last`."""

    def face_polygon_index(self, verts_q, faces, ring_vertices, ring_offsets, ring_polygon, ring_is_hole, polygon_boxes,
                           cell_table, check=True):
        table = tuple(_np(x) for x in (ring_vertices, ring_offsets, ring_polygon, ring_is_hole, polygon_boxes))
        verts_q, faces = _np(verts_q), _np(faces)
        self.last = dict(verts_q=verts_q, faces=faces, table=table, cell_table=cell_table)
        bad = np.any((faces < 0) | (faces >= len(verts_q)), axis=1) if len(faces) else np.zeros(0, dtype=bool)
        if check and bad.any():
            raise ValueError(f"gr_face_polygon_index: {int(bad.sum())} faces name a vertex outside [0, {len(verts_q)})")
        out = np.full(len(faces), -1, dtype=np.int32)
        got, info = face_polygon_index_np(verts_q, faces[~bad], table)
        out[~bad] = got
        lists = np.diff(_np(cell_table[1]))
        stats = np.array([info["tested"], int((out >= 0).sum()), int(lists.max()) if lists.size else 0, int(bad.sum())],
                         dtype=np.int64)
        return out, stats


# -- scenes shared by the host and the device tests ----------------------------------------------------------------------------
def centred_faces(centres):
    """(vertices (3 n, 2) float, faces (n, 3) int32): one triangle per centre c, corners c + (-1, -0.5), c + (1, -0.5), c + (0, 1),
    whose sum is exactly 3 c for coordinates on a 0.5 m lattice."""
    centres = np.asarray(centres, dtype=np.float64).reshape(-1, 2)
    corners = np.array([[-1.0, -0.5], [1.0, -0.5], [0.0, 1.0]])
    verts = (centres[:, None, :] + corners[None]).reshape(-1, 2)
    return verts, np.arange(3 * len(centres), dtype=np.int32).reshape(-1, 3)


def square(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)


def hand_scene():
    """The hand-worked scene: (PlanarPolygons, [(centre, expected row, what it is)]).
    row 0: the square (0, 0)-(10, 10) with the square hole (3, 3)-(7, 7); row 1: the square (8, 8)-(14, 14) over row 0's corner;
    row 2: two parts, (20, 0)-(24, 4) and (26, 0)-(30, 4); row 3: the diamond (40, 0) (44, 4) (40, 8) (36, 4)."""
    from geograypher_amd.utils.geometric import PlanarPolygons

    diamond = np.array([[40.0, 0.0], [44.0, 4.0], [40.0, 8.0], [36.0, 4.0]])
    polygons = PlanarPolygons(
        [square(0, 0, 10, 10), square(3, 3, 7, 7), square(8, 8, 14, 14), square(20, 0, 24, 4), square(26, 0, 30, 4), diamond],
        [0, 0, 1, 2, 2, 3], [False, True, False, False, False, False])
    cases = [
        ((1.5, 1.5), 0, "strictly inside row 0"),
        ((5.0, 5.0), -1, "in the hole of row 0"),
        ((0.0, 5.0), 0, "on an exterior edge"),
        ((0.0, 0.0), 0, "on an exterior vertex"),
        ((3.0, 5.0), 0, "on the hole's edge"),
        ((7.0, 7.0), 0, "on the hole's vertex"),
        ((9.0, 9.0), 1, "in rows 0 and 1: the higher row wins"),
        ((8.0, 8.0), 1, "on row 1's vertex, inside row 0"),
        ((10.0, 10.0), 1, "on row 0's vertex, inside row 1"),
        ((12.0, 12.0), 1, "in row 1 only"),
        ((-2.0, 10.0), -1, "level with row 0's top edge and its vertices, to their left"),
        ((34.0, 4.0), -1, "level with the diamond's left and right vertex, to their left"),
        ((38.0, 4.0), 3, "inside the diamond, level with its right vertex"),
        ((40.0, 4.0), 3, "the diamond's centre"),
        ((44.0, 4.0), 3, "on the diamond's right vertex"),
        ((46.0, 4.0), -1, "level with the diamond's vertices, to their right"),
        ((-3.0, 0.0), -1, "level with row 0's bottom edge, outside"),
        ((25.0, 4.0), -1, "between the parts of row 2, level with their top edges"),
        ((25.0, 2.0), -1, "between the parts of row 2"),
        ((22.0, 2.0), 2, "in the first part of row 2"),
        ((28.0, 2.0), 2, "in the second part of row 2"),
        ((26.0, 2.0), 2, "on the second part's left edge"),
        ((100.0, 100.0), -1, "outside everything"),
    ]
    return polygons, cases


def lattice_scene():
    """The hand scene's polygons under the 0.5 m lattice over x in [-1, 46), y in [-1, 15.5): (points_q (3102, 2) int64, faces
    (3102, 3) int32, ring table).  Face i is [i, i, i], so 3 x its centre is 3 x point i: `face_polygon_index` and `points_in_region`
    are asked about the same points -- on vertices, on horizontal and slanted edges, on the hole's boundary, in overlapping rows."""
    x, y = np.meshgrid(np.arange(-1.0, 46.0, 0.5), np.arange(-1.0, 15.5, 0.5))
    points_q, table = snapped_scene(np.stack([x.ravel(), y.ravel()], axis=1), hand_scene()[0])
    return points_q, np.repeat(np.arange(len(points_q), dtype=np.int32)[:, None], 3, axis=1), table


RANDOM_SEED = 3   # chosen on the CPU: the stand-in counts at least 50 boundary, 50 multi-row and 50 in-hole centres (asserted)


def random_scene(seed=RANDOM_SEED, n_faces=4000, n_polygons=300, extent=40.0):
    """(vertices (V, 2) float64, faces (F, 3) int32, PlanarPolygons): every coordinate on a 0.5 m lattice inside an `extent`
    square, so that centres on ring edges and vertices, overlapping rows and holes are all common.  Polygons: every third an
    axis-aligned rectangle, the others star-shaped with 3 to 40 vertices; every fourth row has a hole.  Faces: half with their
    centre exactly on a lattice point (corners c + d1, c + d2, c - d1 - d2, flat ones among them), half with three lattice
    corners drawn freely near a point."""
    from geograypher_amd.utils.geometric import PlanarPolygons

    rng = np.random.default_rng(seed)

    def lattice(a):
        return np.clip(np.round(np.asarray(a, dtype=np.float64) * 2.0) / 2.0, 0.0, extent)

    def valid(ring):
        x, y = ring[:, 0], ring[:, 1]
        return len(np.unique(ring, axis=0)) >= 3 and np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y) != 0

    rings, rows, holes = [], [], []
    for p in range(n_polygons):
        c = rng.uniform(2.0, extent - 2.0, 2)
        r0 = rng.uniform(1.0, 3.5)
        if p % 3 == 0:
            half = rng.uniform(0.5, r0, 2)
            ring = lattice(square(c[0] - half[0], c[1] - half[1], c[0] + half[0], c[1] + half[1]))
        else:
            k = int(rng.integers(3, 41))
            a = np.sort(rng.uniform(0.0, 2 * np.pi, k))
            r = r0 * rng.uniform(0.6, 1.0, k)
            ring = lattice(c + np.stack([r * np.cos(a), r * np.sin(a)], axis=1))
        if not valid(ring):
            ring = lattice(square(c[0] - 1.5, c[1] - 1.5, c[0] + 1.5, c[1] + 1.5))
        rings.append(ring)
        rows.append(p)
        holes.append(False)
        if p % 4 == 1:
            hole = lattice(c + 0.4 * (ring - c))
            if valid(hole):
                rings.append(hole)
                rows.append(p)
                holes.append(True)
    half_n = n_faces // 2
    c = lattice(rng.uniform(0.0, extent, (half_n, 2)))
    d1, d2 = (np.round(rng.uniform(-2.0, 2.0, (half_n, 2)) * 2.0) / 2.0 for _ in range(2))
    on_lattice = np.stack([c + d1, c + d2, c - d1 - d2], axis=1)
    c = rng.uniform(0.0, extent, (n_faces - half_n, 1, 2))
    free = np.round((c + rng.uniform(-2.0, 2.0, (n_faces - half_n, 3, 2))) * 2.0) / 2.0
    verts = np.concatenate([on_lattice, free]).reshape(-1, 2)
    order = rng.permutation(len(verts))            # face f's corners are scattered through the vertex array
    place = np.empty_like(order)
    place[order] = np.arange(len(verts))
    faces = place[np.arange(len(verts)).reshape(-1, 3)].astype(np.int32)
    return verts[order], faces, PlanarPolygons(rings, rows, holes, n_polygons=n_polygons)


def snapped_scene(verts, polygons):
    """(verts_q (V, 2) int64, ring table) as the mesh class hands them to the backend (rule V2)."""
    from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh

    return TexturedPhotogrammetryMesh._snap_with_polygons(np.asarray(verts, dtype=np.float64), polygons)
