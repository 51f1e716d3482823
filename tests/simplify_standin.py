"""Ring simplification on the CPU: rules S1-S9 of DESIGN.md section 8q in Python integers, chain by chain with an explicit stack
-- the exact stand-in of gr_simplify_rings (`HipRaster.ring_simplifier`), a `StandInBackend` for the host tests, and the scenes
the host and the device tests share.  Written independently of the package: it imports nothing of `geograypher_amd`, and this
module must not be "simplified" to call `utils.geometric` -- the tests would then compare the package with itself.  (The S9 flags
are computed here by dictionaries, not by the package's sort.)"""
import numpy as np

GRID = 1e-6
STAT_WORDS = 8
KEPT, COLLAPSED, PASSES, WIDE, SHORT = 0, 1, 2, 3, 4   # the words of the statistics block


def chord_w(a, b, p):
    """S3: (w, L2, case) of vertex p against the chord a -> b; w = d^2 L2, or d^2 on a chord of no length."""
    ex, ey, ux, uy = b[0] - a[0], b[1] - a[1], p[0] - a[0], p[1] - a[1]
    L2, t = ex * ex + ey * ey, ux * ex + uy * ey
    if L2 == 0:
        return ux * ux + uy * uy, 0, "point"
    if t <= 0:
        return (ux * ux + uy * uy) * L2, L2, "start"
    if t >= L2:
        vx, vy = p[0] - b[0], p[1] - b[1]
        return (vx * vx + vy * vy) * L2, L2, "end"
    c = ex * uy - ey * ux
    return c * c, L2, "inside"


def area2(pts):
    return sum(pts[i - 1][0] * pts[i][1] - pts[i][0] * pts[i - 1][1] for i in range(len(pts)))


def simplify_ring(pts, fixed, T, first_index, tally):
    """S2-S6 for one ring: pts a list of (x, y) Python integers, fixed a list of flags or None, T in grid steps, first_index the
    ring's first vertex in the table (the tie-break of S4 is by table index).  -> the sorted kept positions in the ring ([] when it
    collapses).  tally gathers: passes (the deepest level at which a chain had an interior vertex, counted from 1), wide (interior
    vertices measured against the inside of their chord, over all chains), and what the scene assertions of the tests ask for:
    ties (chains whose largest w is shared), at_tolerance (chains whose largest w equals the bound), endpoint (vertices measured
    against a chord end), collapsed, short."""
    n = len(pts)
    if n < 3:
        tally["short"] += 1
        return []
    anchors = [i for i in range(n) if fixed is not None and fixed[i]]
    if not anchors:
        anchors = [min(range(n), key=lambda i: (pts[i][0], pts[i][1], i))]
    kept = set(anchors)
    stack = [(a, anchors[(k + 1) % len(anchors)], 1) for k, a in enumerate(anchors)]
    while stack:
        a, b, level = stack.pop()
        interior, i = [], (a + 1) % n
        while i != b:
            interior.append(i)
            i = (i + 1) % n
        if not interior:
            continue
        tally["passes"] = max(tally["passes"], level)
        best, best_key, shared, L2 = None, None, 0, 0
        for i in interior:
            w, L2, case = chord_w(pts[a], pts[b], pts[i])
            tally["wide"] += case == "inside"
            tally["endpoint"] += case in ("start", "end")
            key = (-w, pts[i][0], pts[i][1], first_index + i)
            if best_key is None or key < best_key:
                shared = shared + 1 if (best_key is not None and key[0] == best_key[0]) else 1
                best, best_key = i, key
            elif key[0] == best_key[0]:
                shared += 1
        w = -best_key[0]
        bound = T * T * L2 if L2 else T * T
        tally["ties"] += shared > 1
        tally["at_tolerance"] += w == bound
        if w > bound:
            kept.add(best)
            stack.append((a, best, level + 1))
            stack.append((best, b, level + 1))
    out = sorted(kept)
    if len(out) < 3 or area2([pts[i] for i in out]) == 0:
        tally["collapsed"] += 1
        return []
    return out


def simplify_np(ring_vertices, ring_offsets, T, fixed=None):
    """The whole table: (keep (N,) uint8, kept_index (M,) int32, out_offsets (R + 1,) int64, stats (STAT_WORDS,) int64, tally)."""
    rv = np.asarray(ring_vertices, dtype=np.int64).reshape(-1, 2)
    off = np.asarray(ring_offsets, dtype=np.int64).reshape(-1)
    fx = None if fixed is None else np.asarray(fixed).reshape(-1).astype(bool).tolist()
    pts_all = [(int(x), int(y)) for x, y in rv.tolist()]
    tally = dict(passes=0, wide=0, ties=0, at_tolerance=0, endpoint=0, collapsed=0, short=0)
    keep = np.zeros(len(rv), dtype=np.uint8)
    kept_index, out_offsets = [], [0]
    for r in range(len(off) - 1):
        s, e = int(off[r]), int(off[r + 1])
        for i in simplify_ring(pts_all[s:e], None if fx is None else fx[s:e], int(T), s, tally):
            keep[s + i] = 1
            kept_index.append(s + i)
        out_offsets.append(len(kept_index))
    stats = np.zeros(STAT_WORDS, dtype=np.int64)
    stats[KEPT], stats[COLLAPSED], stats[PASSES] = len(kept_index), tally["collapsed"], tally["passes"]
    stats[WIDE], stats[SHORT] = tally["wide"], tally["short"]
    return keep, np.array(kept_index, dtype=np.int32), np.array(out_offsets, dtype=np.int64), stats, tally


def shared_border_fixed_np(ring_vertices, ring_offsets):
    """S9 by dictionaries: 1 where the vertex's position has more than one distinct unordered pair of neighbour positions."""
    rv = [(int(x), int(y)) for x, y in np.asarray(ring_vertices, dtype=np.int64).reshape(-1, 2).tolist()]
    off = [int(v) for v in np.asarray(ring_offsets).reshape(-1).tolist()]
    pairs = {}
    for r in range(len(off) - 1):
        ring = rv[off[r]:off[r + 1]]
        for i, p in enumerate(ring):
            pairs.setdefault(p, set()).add(tuple(sorted((ring[i - 1], ring[(i + 1) % len(ring)]))))
    return np.array([len(pairs[p]) > 1 for p in rv], dtype=np.uint8)


def tol_steps(tol_meters):
    return int(np.rint(float(tol_meters) / GRID))


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


class StandInSimplifier:
    def __init__(self, owner):
        self.owner = owner

    def simplify(self, ring_vertices, ring_offsets, tol_meters, fixed=None):
        rv, off = _np(ring_vertices), _np(ring_offsets)
        fx = None if fixed is None else _np(fixed)
        self.owner.last_simplify = dict(ring_vertices=rv, ring_offsets=off, tol_meters=tol_meters, fixed=fx)
        keep, kept_index, out_offsets, stats, _ = simplify_np(rv, off, tol_steps(tol_meters), fx)
        return keep, kept_index, out_offsets, stats


class StandInBackend:
    """`HipRaster.ring_simplifier` on the CPU; records the arguments of the last call."""

    def ring_simplifier(self):
        return StandInSimplifier(self)


# -- scenes shared by the host and the device tests ----------------------------------------------------------------------------
def table(rings):
    """(ring_vertices (N, 2) int64, ring_offsets (R + 1,) int64) of a list of rings."""
    rings = [np.asarray(r, dtype=np.int64).reshape(-1, 2) for r in rings]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
    return (np.concatenate(rings) if rings else np.zeros((0, 2), dtype=np.int64)), off


K, M = 1000, 10   # the 3-4-5 scene: a chord along (4 K, 3 K), a vertex offset by (-3 M, 4 M) from its middle: distance 5 M exactly


def hand_scenes():
    """name -> (ring, fixed or None, T, the kept indices worked out by hand; [] = the ring collapses).  Without fixed vertices a
    ring is anchored at its smallest (x, y), vertex 0 in every scene here (S2); its first chain runs from the anchor back to
    itself, a chord of no length, so the first split is the vertex farthest from the anchor."""
    scenes = {}
    # Collinear vertices on every side of a square.  Far corner (10, 10) first; every other vertex is a corner (kept: 10 / sqrt 2
    # off the diagonal) or lies ON its chord (w = 0, never above the bound).
    square = [(0, 0), (5, 0), (10, 0), (10, 4), (10, 10), (3, 10), (0, 10), (0, 6), (0, 2)]
    scenes["collinear vertices, T = 0"] = (square, None, 0, [0, 2, 4, 6])
    scenes["collinear vertices, T = 3"] = (square, None, 3, [0, 2, 4, 6])
    # T = 0 drops only what lies on the chord: (5, 1) is one step off (0, 0) -> (10, 0) and stays, (5, 10) is on (10, 10) -> (0, 10)
    scenes["T = 0 keeps one step off the chord"] = ([(0, 0), (5, 1), (10, 0), (10, 10), (5, 10), (0, 10)], None, 0, [0, 1, 2, 3, 5])
    # Exactly at the tolerance.  (4 K, 3 K) is farthest from the anchor (25 K^2 against 18 K^2); (3 K, -3 K) is far off the chord
    # back; vertex 1 = the middle of (0, 0) -> (4 K, 3 K) plus (-3 M, 4 M), perpendicular to it: 5 M off, foot inside.
    ring345 = [(0, 0), (2 * K - 3 * M, 3 * K // 2 + 4 * M), (4 * K, 3 * K), (3 * K, -3 * K)]
    scenes["a vertex exactly at the tolerance is dropped"] = (ring345, None, 5 * M, [0, 2, 3])
    scenes["one step under it, the vertex is kept"] = (ring345, None, 5 * M - 1, [0, 1, 2, 3])
    # Projections beyond the chord's ends.  F = (100, 0) is farthest from the anchor.  Chain A -> F: p = (0, 6) has t = 0 (d^2 = 36),
    # G = (50, -40) is 40 off (foot inside), q = (97, 4) is 4 off: G splits.  Chain A -> G, chord (50, -40): p has t = -240 <= 0, so
    # d^2 = |p - A|^2 = 36.  Chain G -> F, chord (50, 40), L2 = 4100: q - G = (47, 44) has t = 4110 >= L2, so d^2 = |q - F|^2 = 9 + 16
    # = 25.  Chain F -> A: (50, 60) is 60 off.  So T = 4 keeps all, T = 5 drops q (25 > 25 fails), T = 6 drops p too (36 > 36 fails).
    ends = [(0, 0), (0, 6), (50, -40), (97, 4), (100, 0), (50, 60)]
    scenes["beyond the chord's ends, T = 4"] = (ends, None, 4, [0, 1, 2, 3, 4, 5])
    scenes["beyond the chord's ends, T = 5"] = (ends, None, 5, [0, 1, 2, 4, 5])
    scenes["beyond the chord's ends, T = 6"] = (ends, None, 6, [0, 2, 4, 5])
    # The degenerate chord of a one-anchor ring: d^2 = |p - A|^2 against T^2.  (3, 4) is 5 from the anchor, (4, 1) sqrt 17.  T = 5:
    # 25 > 25 fails, only the anchor is left: the ring collapses.  T = 2: (3, 4) stays; (4, 1) against (3, 4) -> (0, 0): cross =
    # (-3)(-3) - (-4)(1) = 13, 169 > 4 * 25: stays.
    tri = [(0, 0), (3, 4), (4, 1)]
    scenes["the degenerate chord, T = 2"] = (tri, None, 2, [0, 1, 2])
    scenes["the degenerate chord, T = the reach: the ring collapses"] = (tri, None, 5, [])
    # Three vertices tie on the degenerate chord (all 10 from the anchor): (6, -8), the smallest (x, y), wins.  Then (6, 8) against
    # (0, 0) -> (6, -8): t = -28 <= 0, d^2 = 100; (10, 0): 8 off.  (6, 8) splits; (10, 0) against (6, 8) -> (6, -8): 4 off.  T = 1: all.
    scenes["a three-way tie on the degenerate chord"] = ([(0, 0), (6, 8), (10, 0), (6, -8)], None, 1, [0, 1, 2, 3])
    # A square between two tips on the x axis: its four corners are all 10 off the axis, two in either chain.  B = (30, 0) is
    # farthest from A = (-30, 0).  Chain A -> B: (-10, -10) and (10, -10) tie, the smaller x wins; chain B -> A: (-10, 10) wins
    # over (10, 10).  The losers, against (-10, -10) -> (30, 0) and (30, 0) -> (-10, 10): cross^2 / L2 = 40000 / 1700 = 23.5.
    tips = [(-30, 0), (-10, -10), (10, -10), (30, 0), (10, 10), (-10, 10)]
    scenes["a square whose corners tie, T = 3"] = (tips, None, 3, [0, 1, 2, 3, 4, 5])
    scenes["a square whose corners tie, T = 5"] = (tips, None, 5, [0, 1, 3, 5])
    # A sliver: (100, 0) is kept, both middle vertices are 1 off its chord: two vertices are left, the ring collapses (S6)
    scenes["a sliver collapses: two vertices left"] = ([(0, 0), (50, 1), (100, 0), (50, -1)], None, 2, [])
    # Three fixed vertices on one line; (10, 1) is 1 off the chord (20, 0) -> (0, 0) and goes at T = 1: what is left has no area
    flat = [(0, 0), (10, 0), (20, 0), (10, 1)]
    scenes["fixed vertices on a line: no area left"] = (flat, [1, 1, 1, 0], 1, [])
    scenes["fixed vertices on a line, T = 0"] = (flat, [1, 1, 1, 0], 0, [0, 1, 2, 3])
    return scenes


def s9_scene():
    """Three classes: A (left) and B (right) share a wiggly vertical border between the junctions J0 (bottom, where C joins from
    below) and J1 (top, on the outer boundary -- a junction of A and B only, fixed all the same: three neighbour pairs), C lies
    under both; A has a hole that is an island of B.  -> (rings, names, the interior vertices of the shared border).  The
    rings: 0 = A's exterior, 1 = A's hole, 2 = B's exterior, 3 = B's island (the hole's positions, the other way round), 4 = C."""
    wiggle = [(1000, 100 + 50 * k + (7 * k * k) % 23) for k in range(1, 17)]          # y rises unevenly; x jitters below by < 13
    wiggle = [(1000 + ((-1) ** k) * ((5 * k) % 13), y) for k, (x, y) in enumerate(wiggle)]
    J0, J1 = (1000, 100), (1000, 1000)
    A = [(0, 100), J0] + wiggle + [J1, (0, 1000)]
    B = [J0, (2000, 100), (2000, 1000), J1] + wiggle[::-1]
    C = [(0, 0), (2000, 0), (2000, 100), J0, (0, 100)]
    island = [(300, 400), (500, 380), (620, 520), (560, 700), (380, 690), (310, 560), (305, 480)]
    return [A, island[::-1], B, island, C], ("A", "A hole", "B", "B island", "C"), wiggle


def sawtooth(n=300):
    """One ring of n vertices that splits off ONE vertex per pass: teeth that alternate above and below the x axis and grow
    linearly, p_k = (10 k, +-7 k).  Vertex 0 is the anchor; the last vertex is farthest from it.  In every chain p_0 -> p_m the teeth
    on p_m's side lie ON the chord and those on the other side are 14 (m - 1 - 2 j) 10 / |chord| off: p_(m-1) is farthest, alone.
    So the passes keep p_(n-1), p_(n-2), ..., p_1: n - 1 of them, one per interior vertex."""
    return [(10 * k, 7 * k * (-1) ** k) for k in range(n)]


def random_scene(seed=5, rings=40, total=4000):
    """About `rings` rings and `total` vertices: closed random walks on a coarse grid (steps of -1, 0 or 1 times 5 on either axis),
    like traced outlines: short chains whose farthest vertex is exactly one grid step off, ties between such vertices and
    projections beyond a chord's end are all common.  Rings may cross themselves and repeat positions: S1 does not forbid it."""
    rng = np.random.default_rng(seed)
    out = []
    for n in rng.integers(total // rings - 40, total // rings + 40, rings):
        steps = rng.integers(-1, 2, (int(n), 2))
        steps[np.all(steps == 0, axis=1)] = (1, 0)
        out.append((rng.integers(0, 400, 2) + np.cumsum(steps, axis=0)) * 5)
    return out


RANDOM_T = 5   # grid steps: with coordinates on multiples of 5, distances of exactly 5 abound
