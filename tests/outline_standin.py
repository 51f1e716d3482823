"""Exact stand-in of gr_class_outlines and of the host's nesting, written independently of the device
code and by other means: Python integers, dictionaries of edge counts and a plain walk from ring to ring -- no sort of packed keys,
no binary search, no pointer doubling.  `StandInBackend` is `HipRaster.class_outlines` on the CPU, for host-logic tests; the scenes at
the end are shared by the host and the device tests.
"""
import numpy as np

STAT_WORDS = 8   # faces without a class, zero-area, turned, cancelled pairs, multi edges, bad faces (the device's block)
SNAP_LIMIT = 1 << 40


def _area2(p, q, r):
    return (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0])


def outlines_np(verts_q, faces, face_class, n_classes):
    """{"canon", "ring_vertices", "ring_offsets", "ring_class", "stats", "n_edges", "n_rings", "slots"}: X2-X6."""
    xy = [(int(x), int(y)) for x, y in np.asarray(verts_q, dtype=np.int64).reshape(-1, 2)]
    tris = np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist()
    classes = [int(c) for c in np.asarray(face_class).reshape(-1)]
    V = len(xy)
    # X2: equal snapped (x, y) are one vertex, the smallest index of the group
    first, canon = {}, []
    for i, p in enumerate(xy):
        canon.append(first.setdefault(p, i))
    # X3: the directed edges of the faces that take part
    stats = [0] * STAT_WORDS
    count = {}
    for tri, c in zip(tris, classes):
        if any(v < 0 or v >= V for v in tri):
            stats[5] += 1
            continue
        if not 0 <= c < n_classes:
            stats[0] += 1
            continue
        a, b, d = (canon[v] for v in tri)
        area = _area2(xy[a], xy[b], xy[d])
        if area == 0:
            stats[1] += 1
            continue
        if area < 0:
            stats[2] += 1
            b, d = d, b
        for e in ((a, b), (b, d), (d, a)):
            count[(c, *e)] = count.get((c, *e), 0) + 1
    # X4: opposite edges of one class cancel; the slots are the copies that are left, sorted by (class, from, to)
    slots = []
    for (c, a, b), n in count.items():
        back = count.get((c, b, a), 0)
        if a < b:
            stats[3] += min(n, back)
        if n - back > 1:
            stats[4] += 1
        slots += [(c, a, b, copy) for copy in range(n - back)]
    slots.sort()
    # X5: at every (class, vertex) the k-th incoming copy (by from, copy) is followed by the k-th outgoing one (by to, copy)
    coming, going = {}, {}
    for s, (c, a, b, copy) in enumerate(slots):
        coming.setdefault((c, b), []).append((a, copy, s))
        going.setdefault((c, a), []).append((b, copy, s))
    follower = [None] * len(slots)
    for where, inc in coming.items():
        out = going.get(where, [])
        assert len(inc) == len(out), "X5: a (class, vertex) with unequal incoming and outgoing copies"
        for (_, _, s), (_, _, t) in zip(sorted(inc), sorted(out)):
            follower[s] = t
    # X6: a ring is walked from its smallest slot; rings ordered by (class, leader)
    seen = [False] * len(slots)
    rings = []
    for s in range(len(slots)):
        if seen[s]:
            continue
        ring, t = [], s
        while not seen[t]:
            seen[t] = True
            ring.append(t)
            t = follower[t]
        assert t == s, "X5 is a bijection: the walk comes back to its start"
        rings.append(ring)
    rings.sort(key=lambda ring: (slots[ring[0]][0], ring[0]))
    offsets = [0]
    for ring in rings:
        offsets.append(offsets[-1] + len(ring))
    return {
        "canon": np.array(canon, dtype=np.int32).reshape(-1),
        "ring_vertices": np.array([slots[s][1] for ring in rings for s in ring], dtype=np.int32).reshape(-1),
        "ring_offsets": np.array(offsets, dtype=np.int64),
        "ring_class": np.array([slots[ring[0]][0] for ring in rings], dtype=np.int32).reshape(-1),
        "stats": np.array(stats, dtype=np.int64),
        "n_edges": len(slots), "n_rings": len(rings), "slots": slots,
    }


class StandInBackend:
    """`HipRaster.class_outlines` on the CPU; records the arguments of the last call."""

    def class_outlines(self, verts_q, faces, face_class, n_classes, capacity=None, check=True):
        host = lambda a: np.asarray(a.cpu() if hasattr(a, "detach") else a)
        verts_q, faces, face_class = host(verts_q), host(faces), host(face_class)
        if not 0 <= int(n_classes) <= 65535:
            raise ValueError(f"gr_class_outlines: n_classes={int(n_classes)} outside [0, 65535]")
        self.last_outline = dict(verts_q=verts_q, faces=faces, face_class=face_class, n_classes=int(n_classes))
        self.outline_calls = getattr(self, "outline_calls", 0) + 1
        got = outlines_np(verts_q, faces, face_class, int(n_classes))
        if check and got["stats"][5]:
            raise ValueError(f"gr_class_outlines: {int(got['stats'][5])} faces name a vertex outside [0, {len(verts_q)})")
        return got["canon"], got["ring_vertices"], got["ring_offsets"], got["ring_class"], got["stats"]


# -- X7: winding numbers against face counts, by brute force --------------------------------------------------------------------------
def winding_number(ring, px, py):
    """Winding number of the integer ring [(x, y)] around a point that is on none of its edges."""
    wn = 0
    for i in range(len(ring)):
        (ax, ay), (bx, by) = ring[i - 1], ring[i]
        if (ay <= py) != (by <= py):
            side = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
            assert side != 0, "the point lies on an edge"
            if by > ay and side > 0:
                wn += 1
            if by < ay and side < 0:
                wn -= 1
    return wn


def point_in_triangle(p, a, b, c):
    """1 strictly inside, 0 outside, None on the boundary (either winding)."""
    s = [_area2(a, b, p), _area2(b, c, p), _area2(c, a, p)]
    if _area2(a, b, c) < 0:
        s = [-v for v in s]
    if min(s) > 0:
        return 1
    return 0 if min(s) < 0 else None


def x7_mismatches(verts_q, faces, face_class, n_classes, got=None):
    """At 3 x centre of every face (all coordinates times 3): for every class, the winding number of its rings against the number of
    its taking-part faces that hold the point.  Returns (points checked, mismatches); a point on some face's boundary is an
    AssertionError -- the scenes keep clear of that."""
    got = got or outlines_np(verts_q, faces, face_class, n_classes)
    xy = [(3 * int(x), 3 * int(y)) for x, y in np.asarray(verts_q).reshape(-1, 2)]
    tris = np.asarray(faces).reshape(-1, 3).tolist()
    classes = [int(c) for c in np.asarray(face_class).reshape(-1)]
    rings = {}
    off = got["ring_offsets"]
    for r, c in enumerate(got["ring_class"].tolist()):
        rings.setdefault(c, []).append([xy[v] for v in got["ring_vertices"][off[r]:off[r + 1]].tolist()])
    live = [(tri, c) for tri, c in zip(tris, classes) if 0 <= c < n_classes and _area2(*(xy[v] for v in tri)) != 0]
    checked = wrong = 0
    for tri, _ in live:
        p = tuple(sum(xy[v][k] for v in tri) // 3 for k in (0, 1))
        cover = {}
        for other, c in live:
            inside = point_in_triangle(p, *(xy[v] for v in other))
            assert inside is not None, "a face centre on another face's boundary"
            cover[c] = cover.get(c, 0) + inside
        for c in range(n_classes):
            checked += 1
            wrong += sum(winding_number(ring, *p) for ring in rings.get(c, [])) != cover.get(c, 0)
    return checked, wrong


# -- X8: nesting, in Python integers ---------------------------------------------------------------------------------------------------
def ring_area2(ring):
    return sum(ring[i - 1][0] * ring[i][1] - ring[i][0] * ring[i - 1][1] for i in range(len(ring)))


def in_closed_region(ring, px, py):
    """On the ring, or a non-zero winding number."""
    for i in range(len(ring)):
        (ax, ay), (bx, by) = ring[i - 1], ring[i]
        if (bx - ax) * (py - ay) - (by - ay) * (px - ax) == 0 and (px - ax) * (px - bx) <= 0 and (py - ay) * (py - by) <= 0:
            return True
    return winding_number(ring, px, py) != 0


def nest_np(verts_q, got):
    """(areas2, home): home[r] of a hole = the exterior of its class with the smallest area (then the smallest ring number) whose
    closed region holds all of the hole's vertices, -1 for none and for exteriors."""
    xy = [(int(x), int(y)) for x, y in np.asarray(verts_q).reshape(-1, 2)]
    off = got["ring_offsets"]
    rings = [[xy[v] for v in got["ring_vertices"][off[r]:off[r + 1]].tolist()] for r in range(len(off) - 1)]
    areas2 = [ring_area2(ring) for ring in rings]
    home = [-1] * len(rings)
    for r, ring in enumerate(rings):
        if areas2[r] >= 0:
            continue
        fits = [(areas2[e], e) for e in range(len(rings))
                if areas2[e] > 0 and got["ring_class"][e] == got["ring_class"][r] and all(in_closed_region(rings[e], *p) for p in ring)]
        if fits:
            home[r] = min(fits)[1]
    return areas2, home


# -- scenes shared by the host and the device tests -------------------------------------------------------------------------------------
def grid_mesh(nx, ny, step=1_000_000, jitter=0, seed=0):
    """(verts_q ((nx + 1)(ny + 1), 2) int64, faces (2 nx ny, 3) int32, quad_of_face): a grid of nx x ny quads, each cut into two
    counter-clockwise faces along its (0,0)-(1,1) diagonal; vertex (i, j) has index j (nx + 1) + i.  jitter: every vertex is moved by
    up to that many grid steps each way (up to 0.15 step keeps every face counter-clockwise, so no two overlap)."""
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
    verts = np.stack([ii.ravel(), jj.ravel()], axis=1).astype(np.int64) * step
    if jitter:
        verts = verts + rng.integers(-jitter, jitter + 1, verts.shape)
    faces, quad = [], []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i
            faces += [[a, b, c], [a, c, d]]
            quad += [j * nx + i] * 2
    return verts, np.array(faces, dtype=np.int32), np.array(quad)


def quad_classes(quad_of_face, classes_of_quads):
    return np.asarray(classes_of_quads, dtype=np.int32).reshape(-1)[quad_of_face]


def height_field(n=12, seed=3):
    """A jittered n x n height field with three classes in blobs, a class-free border strip and some NaN faces: (points (V, 3) float64
    metres around a far-away origin, faces (F, 3) int64, labels (F,) float64 with NaN).  No two faces overlap in plan view."""
    rng = np.random.default_rng(seed)
    verts, faces, quad = grid_mesh(n, n, step=1_000_000, jitter=150_000, seed=seed)
    xy = verts.astype(np.float64) * 1e-6
    points = np.column_stack([xy[:, 0] + 512_000.0, xy[:, 1] + 4_100_000.0, rng.random(len(xy)) * 3.0])
    centres = xy[faces].mean(axis=1)
    labels = np.full(len(faces), np.nan)
    for cls, (cx, cy, r) in enumerate(((3.5, 3.5, 2.6), (8.5, 4.0, 2.2), (6.0, 8.5, 2.8))):
        labels[np.hypot(centres[:, 0] - cx, centres[:, 1] - cy) < r] = float(cls)
    labels[np.hypot(centres[:, 0] - 6.0, centres[:, 1] - 8.5) < 0.9] = 0.0     # an island of class 0 in a hole of class 2
    labels[rng.random(len(faces)) < 0.04] = np.nan
    return points, faces.astype(np.int64), labels


def reversed_faces(faces):
    return np.ascontiguousarray(np.asarray(faces)[:, ::-1])


def fold_scene():
    """A strip folded over itself: both faces lie on the same side of their shared edge b-a, which is left in two copies."""
    verts = np.array([[0, 0], [0, 2_000_000], [2_000_000, 1_000_000], [1_100_000, 900_000]], dtype=np.int64)
    return verts, np.array([[0, 2, 1], [1, 0, 3]], dtype=np.int32)


def seam_scene():
    """Two quads side by side whose shared edge exists twice, under different vertex indices (a split seam)."""
    s = 1_000_000
    verts = np.array([[0, 0], [s, 0], [s, s], [0, s], [s, 0], [2 * s, 0], [2 * s, s], [s, s]], dtype=np.int64)
    return verts, np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], dtype=np.int32)


def wall_scene():
    """Two quads joined by a vertical wall: the wall's faces have no area in plan view and its two rims coincide."""
    s = 1_000_000
    verts = np.array([[0, 0], [s, 0], [s, s], [0, s],          # the lower quad
                      [s, 0], [2 * s, 0], [2 * s, s], [s, s]], dtype=np.int64)   # the upper quad; 4 and 7 stand above 1 and 2
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7], [1, 4, 7], [1, 7, 2]], dtype=np.int32)
    return verts, faces


def unit_area_scene():
    """Snapped doubled areas of exactly +1, -1 and 0, and four faces whose area products need more than 64 bits, all within
    |value| <= 2^40 - 1: 4 L^2 at the corners of the range; a doubled area of exactly +1 between products of about 2^82; a doubled
    area of exactly 2^64, which 64-bit arithmetic wraps to 0 (the face would be dropped); and one of exactly 2^63, which it wraps to
    -2^63 (the face would be turned over)."""
    L = SNAP_LIMIT - 1
    m = 2 * L - 5
    a = (-L + 3, -L)
    verts = np.array([[0, 0], [1, 0], [0, 1],                     # +1
                      [10, 10], [10, 11], [11, 10],               # -1
                      [20, 20], [21, 21], [22, 22],               # 0
                      [-L, -L], [L, -L], [L, L],                  # 4 L^2
                      a, [a[0] + m - 1, a[1] + m], [a[0] + m - 2, a[1] + m - 1],   # (m - 1)(m - 1) - m (m - 2) = 1
                      [100, 100], [100 + 2 ** 32, 100], [100, 100 + 2 ** 32],      # 2^64
                      [-200, -200], [-200 + 2 ** 32, -200], [-200, -200 + 2 ** 31]], dtype=np.int64)   # 2^63
    assert np.abs(verts).max() <= L
    return verts, np.arange(21, dtype=np.int32).reshape(7, 3)


def delaunay_scene(n_faces, seed=0):
    """The first n_faces triangles of the Delaunay triangulation of random snapped points (scipy): (verts_q, faces)."""
    from scipy.spatial import Delaunay

    rng = np.random.default_rng(seed)
    n_points = max(8, int(n_faces * 0.6) + 8)
    verts = rng.integers(-50_000_000, 50_000_000, (n_points, 2)).astype(np.int64)
    simplices = Delaunay(verts.astype(np.float64)).simplices
    assert len(simplices) >= n_faces
    return verts, np.ascontiguousarray(simplices[:n_faces], dtype=np.int32)


def disk_classes(verts_q, faces, n_disks=4, seed=0):
    """Coherent classes: the class of the first of a few random disks that holds the face centre, else none."""
    rng = np.random.default_rng(seed + 100)
    centres = np.asarray(verts_q, dtype=np.float64)[faces].mean(axis=1)
    cls = np.full(len(faces), -1, dtype=np.int32)
    for k in reversed(range(n_disks)):
        c, r = rng.uniform(-40e6, 40e6, 2), rng.uniform(15e6, 35e6)
        cls[np.hypot(*(centres - c).T) < r] = k % 3
    return cls
