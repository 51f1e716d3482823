"""Exact scenes and rational references for the three device calls of the multiview-detection workflow (gr_ray_pairs,
gr_community_points, gr_rays_clip); no test in here (tests/test_ray_edges_host.py, tests/test_ray_edges_gpu.py).

The references restate the rule text of DESIGN.md (section 8, "Multiview detections", and L14 of section 8p) and of the
docstrings in csrc/ray_dev.hpp and csrc/rays.hip over the rationals (`fractions.Fraction`; an integer is the Fraction with
denominator 1 and is kept as a Python int, which is only faster).  They import neither the package's host form
(utils/numeric.py) nor the numpy stand-ins (tests/ray_standin.py, tests/community_standin.py): the host test compares all of
those with what is written here.

Every scene is built so that each intermediate of the float64 computation is exact (segments along the coordinate axes with
dyadic end points: the length is one component's absolute value, the unit vector a signed basis vector; right triangles with
legs 2 under vertical rays: det = +-4).  The device, the stand-ins and the rational reference then agree bit for bit and no
tolerance is needed."""
import math
from fractions import Fraction

import numpy as np

NAN = "NaN"   # what closest_points_exact returns for a pair with a zero-length segment
INT32_MIN = -(2**31)


# -- rationals --------------------------------------------------------------------------------------------------------------------
def _q(x):
    f = Fraction(float(x))   # a finite float is a rational
    return f.numerator if f.denominator == 1 else f


def _vec(p):
    return tuple(_q(c) for c in p)


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _along(p, t, u):
    return (p[0] + t * u[0], p[1] + t * u[1], p[2] + t * u[2])


def _clip0(x, hi):
    return min(max(x, 0), hi)


def _div(x, d):
    return x if d == 1 else Fraction(x) / d


def round_once(x):
    """The float64 nearest to the rational x (int / int is correctly rounded)."""
    f = Fraction(x)
    return f.numerator / f.denominator


def _axis_unit(p0, p1):
    """(unit vector, length) of a segment along a coordinate axis; (None, 0) for a zero-length one, whose unit is 0 / 0."""
    d = _sub(p1, p0)
    nz = [k for k in range(3) if d[k] != 0]
    if not nz:
        return None, 0
    assert len(nz) == 1, "closest_points_exact is defined for segments along a coordinate axis"
    u = [0, 0, 0]
    u[nz[0]] = 1 if d[nz[0]] > 0 else -1
    return tuple(u), abs(d[nz[0]])


# -- segment_closest_points -------------------------------------------------------------------------------------------------------
def _closest(a0, a1, b0, b1):
    """(pA, pB, kind) or (NAN, NAN, "zero"); kind is "before", "after" or "middle" for a parallel pair, else the pair
    (oob_a, oob_b)."""
    return _closest_q(_vec(a0), _vec(a1), _vec(b0), _vec(b1))


def _closest_q(a0, a1, b0, b1):
    """... on triples of rationals."""
    uA, mA = _axis_unit(a0, a1)
    uB, mB = _axis_unit(b0, b1)
    if uA is None or uB is None:
        return NAN, NAN, "zero"
    n = _cross(uA, uB)
    denom = _dot(n, n)   # |n|^2: 0 or 1 for two signed basis vectors, so sqrt and square give it back exactly
    assert denom in (0, 1)
    if denom == 0:
        # parallel: B's ends on A's axis, measured from a0
        base = _dot(uA, a0)
        d0, d1 = _dot(uA, b0) - base, _dot(uA, b1) - base
        before = d0 <= 0 and d1 <= 0
        after = d0 >= mA and d1 >= mA
        if before or after:
            return (a1 if after else a0), (b0 if abs(d0) < abs(d1) else b1), ("after" if after else "before")
        pA = _along(a0, _clip0(d0, mA), uA)
        g = _sub(b0, pA)
        al = _dot(g, uA)
        return pA, (pA[0] + (g[0] - al * uA[0]), pA[1] + (g[1] - al * uA[1]), pA[2] + (g[2] - al * uA[2])), "middle"
    t = _sub(b0, a0)
    t0 = _div(_dot(_cross(t, uB), n), denom)
    t1 = _div(_dot(_cross(t, uA), n), denom)
    pA = _along(a0, _clip0(t0, mA), uA)
    pB = _along(b0, _clip0(t1, mB), uB)
    oob_a, oob_b = t0 < 0 or t0 > mA, t1 < 0 or t1 > mB
    if oob_a:   # first B from the clamped A ...
        pB = _along(b0, _clip0(_dot(_sub(pA, b0), uB), mB), uB)
    if oob_b:   # ... then A from the updated B
        pA = _along(a0, _clip0(_dot(_sub(pB, a0), uA), mA), uA)
    return pA, pB, (oob_a, oob_b)


def closest_points_exact(a0, a1, b0, b1):
    """The closest points (pA, pB) of segment A = a0 -> a1 and segment B = b0 -> b1, both clamped to their segments, as triples
    of rationals; NAN when either segment has no length.  Segments along a coordinate axis with dyadic end points only."""
    pA, pB, kind = _closest(a0, a1, b0, b1)
    return NAN if kind == "zero" else (pA, pB)


def pair_kind_exact(a0, a1, b0, b1):
    """"zero", "before", "after", "middle", or (oob_a, oob_b) for a non-parallel pair."""
    return _closest(a0, a1, b0, b1)[2]


def distance_exact(a0, a1, b0, b1):
    """|pA - pB|: the square root of a rational, rounded once (the rational is a float64 on these scenes); NaN for NAN."""
    pp = closest_points_exact(a0, a1, b0, b1)
    if pp == NAN:
        return float("nan")
    e = _sub(*pp)
    d2 = Fraction(_dot(e, e))
    assert Fraction(float(d2)) == d2
    return math.sqrt(float(d2))


def ray_pair_edges_exact(starts, ends, threshold):
    """(i, j, d) sorted by (i, j) of every pair i < j (A is ray i) with d <= threshold; all images taken as distinct."""
    n = len(starts)
    out = [(i, j, distance_exact(starts[i], ends[i], starts[j], ends[j])) for i in range(n) for j in range(i + 1, n)]
    out = [e for e in out if e[2] <= threshold]   # NaN never is
    return (np.array([e[0] for e in out], np.int32), np.array([e[1] for e in out], np.int32), np.array([e[2] for e in out], np.float64))


def community_sum_exact(starts, ends, members):
    """(sum of pA and pB over all ordered pairs of distinct members as three rationals, the number of points summed); (NAN, 0)
    when a member has no length."""
    total, count = [0, 0, 0], 0
    s, e = {i: _vec(starts[i]) for i in members}, {i: _vec(ends[i]) for i in members}
    for i in members:
        for j in members:
            if i == j:
                continue
            pA, pB, kind = _closest_q(s[i], e[i], s[j], e[j])
            if kind == "zero":
                return NAN, 0
            total = [total[k] + pA[k] + pB[k] for k in range(3)]
            count += 2
    return tuple(total), count


def community_points_exact(starts, ends, community, M):
    """L14: per community the mean of pA and pB over all ordered pairs of distinct members, taken as a rational and rounded once:
    (M, 3) float64.  NaN for fewer than two members, and for a zero-length member together with any other member."""
    community = np.asarray(community)
    out = np.full((int(M), 3), np.nan)
    for c in range(int(M)):
        members = [int(i) for i in np.nonzero(community == c)[0]]
        if len(members) < 2:
            continue
        total, count = community_sum_exact(starts, ends, members)
        if total == NAN:
            continue
        assert max(abs(Fraction(x).numerator) for x in total) < 2**53 and max(Fraction(x).denominator for x in total) <= 2
        out[c] = [round_once(Fraction(x) / count) for x in total]
    return out


# -- Moller-Trumbore --------------------------------------------------------------------------------------------------------------
def clip_hits_exact(origins, directions, points, faces):
    """Per ray the list of (face, t, u, v) of every triangle it hits, t, u, v rationals: double-sided, the edges and vertices
    inclusive (u >= 0, v >= 0, u + v <= 1), t >= 0, det == 0 never a hit; a face with an index outside [0, V) is never hit, nor
    is anything with a coordinate that is not finite (ray or triangle)."""
    origins, directions, points = (np.asarray(x, np.float64).reshape(-1, 3) for x in (origins, directions, points))
    faces = np.asarray(faces).reshape(-1, 3)
    V = len(points)
    fin_p = np.isfinite(points).all(axis=1)
    good = [k for k in range(len(faces)) if all(0 <= int(v) < V and fin_p[int(v)] for v in faces[k])]
    used = sorted({int(v) for k in good for v in faces[k]})

    def denominator(rows):
        return math.lcm(*[Fraction(float(c)).denominator for row in rows for c in row]) if len(rows) else 1

    den_p = denominator(points[used])
    scaled = {}   # scale -> the triangles (v0, e1, e2) as integers

    def triangles(L):
        if L not in scaled:
            P = {v: tuple(int(Fraction(float(c)) * L) for c in points[v]) for v in used}
            scaled[L] = [(k, P[int(faces[k][0])], _sub(P[int(faces[k][1])], P[int(faces[k][0])]),
                          _sub(P[int(faces[k][2])], P[int(faces[k][0])])) for k in good]
        return scaled[L]

    hits = []
    for o, d in zip(origins, directions):
        mine = []
        hits.append(mine)
        if not (np.isfinite(o).all() and np.isfinite(d).all()):
            continue
        # everything times L: integers; t, u and v do not change when the origin, the direction and the triangle are all scaled
        L = math.lcm(den_p, denominator([o, d]))
        oi = tuple(int(Fraction(float(c)) * L) for c in o)
        di = tuple(int(Fraction(float(c)) * L) for c in d)
        for k, v0, e1, e2 in triangles(L):
            p = _cross(di, e2)
            det = _dot(e1, p)
            if det == 0:
                continue
            sg = 1 if det > 0 else -1
            s = _sub(oi, v0)
            un = _dot(s, p) * sg          # u = un / |det|
            if un < 0:
                continue
            q = _cross(s, e1)
            vn = _dot(di, q) * sg
            if vn < 0 or un + vn > abs(det):
                continue
            tn = _dot(e2, q) * sg
            if tn < 0:
                continue
            mine.append((k, Fraction(tn, abs(det)), Fraction(un, abs(det)), Fraction(vn, abs(det))))
    return hits


def nearest_hits(hits, n_faces=None, without=()):
    """Per ray the winning (face, t, u, v) among the faces below `n_faces` and not in `without`, None for a miss: the nearest t,
    of equal t the first face."""
    out = []
    for mine in hits:
        mine = [h for h in mine if (n_faces is None or h[0] < n_faces) and h[0] not in without]
        out.append(min(mine, key=lambda h: (h[1], h[0])) if mine else None)
    return out


def clip_outputs(origins, directions, winners):
    """hit (N,) bool, t (N,), p (N, 3) from the winners: t and p = o + t d rounded once, NaN on a miss."""
    n = len(winners)
    hit = np.array([w is not None for w in winners], dtype=bool).reshape(n)
    t, p = np.full(n, np.nan), np.full((n, 3), np.nan)
    for r, w in enumerate(winners):
        if w is None:
            continue
        t[r] = round_once(w[1])
        p[r] = [round_once(Fraction(float(origins[r][k])) + w[1] * Fraction(float(directions[r][k]))) for k in range(3)]
    return hit, t, p


def clip_exact(origins, directions, points, faces):
    """Moller-Trumbore over the rationals (the rules of `clip_hits_exact`): hit, t, p."""
    origins, directions = np.asarray(origins, np.float64).reshape(-1, 3), np.asarray(directions, np.float64).reshape(-1, 3)
    return clip_outputs(origins, directions, nearest_hits(clip_hits_exact(origins, directions, points, faces)))


# -- comparing bits ---------------------------------------------------------------------------------------------------------------
def same_bits(got, want):
    """NaN in the same places (whatever its sign and payload) and every other float64 equal bit for bit.  The rationals have one
    zero: a float zero of either sign is that zero (a ray that starts on a triangle whose det is negative has t = -0.0, which
    is >= 0 and a hit), so -0.0 is read as 0.0 on both sides; nothing else is."""
    got, want = np.ascontiguousarray(got, np.float64) + 0.0, np.ascontiguousarray(want, np.float64) + 0.0
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]))


# -- scenes -----------------------------------------------------------------------------------------------------------------------
ZERO_LENGTH = 30   # the one zero-length segment of axis_segments()

_AXIS_SEGMENTS = [
    # along x, on the line y = 10, z = 10: A = [10, 20] and every parallel case against it
    ((10, 10, 10), (20, 10, 10)),        # 0: A
    ((2, 10, 10), (6, 10, 10)),          # 1: wholly before
    ((6, 10, 10), (2, 10, 10)),          # 2: ... travelling the other way
    ((24, 10, 10), (30, 10, 10)),        # 3: wholly after
    ((30, 10, 10), (24, 10, 10)),        # 4
    ((20, 10, 10), (26, 10, 10)),        # 5: touching A's end
    ((4, 10, 10), (10, 10, 10)),         # 6: touching A's start
    ((16, 10, 10), (28, 10, 10)),        # 7: overlapping
    ((28, 10, 10), (16, 10, 10)),        # 8
    ((12.5, 10, 10), (17.5, 10, 10)),    # 9: inside
    ((17.5, 10, 10), (12.5, 10, 10)),    # 10
    ((10, 10, 10), (20, 10, 10)),        # 11: duplicate of 0
    ((20, 10, 10), (10, 10, 10)),        # 12: ... reversed
    # the same, offset sideways
    ((2, 13.5, 10), (6, 13.5, 10)),      # 13: before
    ((24, 10, 12), (30, 10, 12)),        # 14: after
    ((16, 13.5, 12), (28, 13.5, 12)),    # 15: overlapping
    ((17.5, 12, 10), (12.5, 12, 10)),    # 16: inside, reversed
    ((20, 11.5, 10), (26, 11.5, 10)),    # 17: touching
    # along y, on x = 40, z = 20
    ((40, 10, 20), (40, 20, 20)),        # 18
    ((40, 2, 20), (40, 6, 20)),          # 19
    ((40, 30, 20), (40, 24, 20)),        # 20
    ((40, 14, 20), (40, 26, 20)),        # 21
    ((42.5, 12, 20), (42.5, 18, 20)),    # 22
    ((40, 20, 20), (40, 10, 20)),        # 23
    # along z, on x = 50, y = 50
    ((50, 50, 10), (50, 50, 20)),        # 24
    ((50, 50, 2), (50, 50, 6)),          # 25
    ((50, 50, 30), (50, 50, 24.5)),      # 26
    ((50, 50, 14), (50, 50, 26)),        # 27
    ((51.5, 50, 12), (51.5, 50, 18)),    # 28
    ((50, 50, 20), (50, 50, 10)),        # 29
    ((30, 30, 30), (30, 30, 30)),        # 30: zero length
    # perpendicular pairs
    ((15, 5, 10), (15, 15, 10)),         # 31: crosses 0 at (15, 10, 10)
    ((15, 10, 10), (15, 18, 10)),        # 32: touches 0 with its start
    ((15, 12, 14), (15, 12, 22)),        # 33: against 0 the parameter along A is inside, the one along B outside
    ((25, 40, 10), (25, 45, 10)),        # 34: against 0 both outside
    ((3, 10, 5), (3, 10, 8)),            # 35: against 0 both outside, on the other side
    ((33, 2, 10), (33, 8, 10)),          # 36
    ((40, 15, 15), (40, 15, 25)),        # 37: crosses 18 at (40, 15, 20)
    ((45, 50, 15), (55, 50, 15)),        # 38: crosses 24 at (50, 50, 15)
    ((50, 45, 20), (50, 55, 20)),        # 39: touches 24's end with its middle
]


def pair_kinds(starts, ends):
    """The count of every kind over all ordered pairs of distinct segments: {"zero", "before", "after", "middle", "skew",
    "oob_a", "oob_b", "oob_both"} ("skew": not parallel; the oob counts are among those)."""
    count = dict.fromkeys(("zero", "before", "after", "middle", "skew", "oob_a", "oob_b", "oob_both"), 0)
    n = len(starts)
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            kind = pair_kind_exact(starts[i], ends[i], starts[j], ends[j])
            if isinstance(kind, str):
                count[kind] += 1
            else:
                count["skew"] += 1
                count["oob_a"] += kind[0]
                count["oob_b"] += kind[1]
                count["oob_both"] += kind[0] and kind[1]
    return count


def axis_segments():
    """(starts, ends), each (40, 3) float64: the table above."""
    starts = np.array([s for s, _ in _AXIS_SEGMENTS], dtype=np.float64)
    ends = np.array([e for _, e in _AXIS_SEGMENTS], dtype=np.float64)
    both = np.concatenate([starts, ends])
    assert np.array_equal(both * 2, np.rint(both * 2)) and both.min() > 0 and both.max() < 64
    seg = ends - starts
    along = (seg != 0).sum(axis=1)
    assert np.array_equal(np.nonzero(along == 0)[0], [ZERO_LENGTH]) and along.max() == 1
    with np.errstate(invalid="ignore"):
        mag = np.sqrt((seg[:, 0] * seg[:, 0] + seg[:, 1] * seg[:, 1]) + seg[:, 2] * seg[:, 2])
        unit = seg / mag[:, None]
    keep = along == 1
    assert np.array_equal(mag, np.abs(seg).max(axis=1)) and np.isin(unit[keep], (-1.0, 0.0, 1.0)).all()
    assert np.array_equal(np.abs(unit[keep]).sum(axis=1), np.ones(keep.sum()))
    kinds = pair_kinds(starts, ends)
    assert all(kinds[k] > 0 for k in kinds), kinds
    assert len({(tuple(s), tuple(e)) for s, e in zip(starts, ends)}) < len(starts), "no duplicate"
    return starts, ends


def axis_community(m, seed):
    """(starts, ends), each (m, 3) float64: m segments along the axes with integer end points in [1, 32] and lengths 1 .. 8.
    The first rows of a longer draw with the same seed are the shorter draw."""
    raw = np.random.default_rng(seed).integers(0, 1 << 16, size=(m, 6))
    starts = 9.0 + (raw[:, :3] % 16)
    axis, sign, length = raw[:, 3] % 3, 1.0 - 2.0 * (raw[:, 4] % 2), 1.0 + (raw[:, 5] % 8)
    ends = starts.copy()
    ends[np.arange(m), axis] += sign * length
    both = np.concatenate([starts, ends])
    assert np.array_equal(both, np.rint(both)) and both.min() >= 1 and both.max() <= 32
    assert ((ends - starts != 0).sum(axis=1) == 1).all()
    # 2 m (m - 1) points of at most 32 each: every partial sum is an integer far below 2^53, in any order
    assert 2 * m * (m - 1) * 32 < 2**53
    return starts, ends


def parallel_pairs(starts, ends):
    """Ordered pairs of distinct segments along one axis (no zero-length segment in the scene)."""
    axis = np.argmax(ends - starts != 0, axis=1)
    same = axis[:, None] == axis[None, :]
    return int(same.sum()) - len(axis)


FIELD_TOP, FIELD_BOTTOM = 10.0, 1.0   # where the vertical rays of stacked_field start: above and below every height
FIELD_OFFSET = 2.0                    # x and y of the first lattice vertex: one step outside the border is then a normal number


def stacked_field(g, seed):
    """A g x g height field on a pitch of 2 (x, y from FIELD_OFFSET) with heights 4 + k / 8, k in [0, 16]; every cell is cut along one of its diagonals
    (which one alternates), the triangles' vertex order rotates and the faces are shuffled by `seed`; vertical rays.
    -> dict: points (g g, 3), faces (2 (g - 1)^2, 3) int32, origins, directions (N, 3), kind (N,) of str: what each ray is
    aimed at -- "interior", "diagonal", "edge", "vertex", "border", "outside", "surface" (starts on it: t == 0), "past" (starts
    one step past it and points away), "away" (points away from it).  The rays are shuffled by `seed` as well."""
    rng = np.random.default_rng(seed)
    height = 4.0 + rng.integers(0, 17, size=(g, g)) / 8.0
    ii, jj = np.meshgrid(np.arange(g), np.arange(g), indexing="ij")
    points = np.stack([FIELD_OFFSET + 2.0 * ii, FIELD_OFFSET + 2.0 * jj, height], axis=-1).reshape(-1, 3)
    vid = lambda i, j: i * g + j
    faces = []
    for i in range(g - 1):
        for j in range(g - 1):
            a, b, c, d = vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)
            pair = [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
            for tri in pair:
                rot = len(faces) % 3
                faces.append(tri[rot:] + tri[:rot])
    faces = np.array(faces, dtype=np.int32)[rng.permutation(len(faces))]
    e1, e2 = points[faces[:, 1]] - points[faces[:, 0]], points[faces[:, 2]] - points[faces[:, 0]]
    assert np.array_equal(np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]), np.full(len(faces), 4.0))   # det = +-4
    assert np.array_equal(height * 8, np.rint(height * 8))

    side = 2.0 * (g - 1)
    xy, kind = [], []

    def add(x, y, what, shift=FIELD_OFFSET):
        xy.append((x + shift, y + shift)); kind.append(what)

    for i in range(g - 1):
        for j in range(g - 1):
            # one ray inside each of the cell's two triangles, whichever diagonal cuts it
            if (i + j) % 2 == 0:
                add(2 * i + 1.25, 2 * j + 0.5, "interior"); add(2 * i + 0.5, 2 * j + 1.25, "interior")
            else:
                add(2 * i + 0.5, 2 * j + 0.25, "interior"); add(2 * i + 1.5, 2 * j + 1.75, "interior")
            if (3 * i + j) % 8 == 0:
                add(2 * i + 1.0, 2 * j + 1.0, "diagonal")
                add(2 * i + 0.5, 2 * j + (0.5 if (i + j) % 2 == 0 else 1.5), "diagonal")
    for i in range(0, g - 1, 8):
        for j in range(1, g - 1):
            add(2 * i + 1.0, 2.0 * j, "edge"); add(2.0 * j, 2 * i + 0.5, "edge")
    for i in range(1, g - 1, 3):
        for j in range(1, g - 1, 3):
            add(2.0 * i, 2.0 * j, "vertex")
    for k in range(0, g - 1, 3):
        add(0.0, 2 * k + 1.0, "border"); add(side, 2 * k + 0.5, "border"); add(2 * k + 1.5, 0.0, "border"); add(2 * k + 1.0, side, "border")
    for x, y in ((0.0, 0.0), (side, 0.0), (0.0, side), (side, side), (0.0, 4.0), (side, 6.0)):
        add(x, y, "border")
    up, down = np.nextafter(FIELD_OFFSET + side, np.inf), np.nextafter(FIELD_OFFSET, -np.inf)
    for k in (1, g - 2):
        y0, y1 = FIELD_OFFSET + 2 * k + 1.0, FIELD_OFFSET + 2.0 * k
        add(down, y0, "outside", 0.0); add(up, y1, "outside", 0.0); add(y0 - 0.5, down, "outside", 0.0); add(y1, up, "outside", 0.0)
    # the faces of a ragged last chunk of 128 get a second ray each: with 8 faces it would otherwise win 8 rays or fewer
    for k in range(len(faces) // 128 * 128, len(faces)):
        c = points[faces[k, 0]] + 0.25 * e1[k] + 0.25 * e2[k]
        add(c[0], c[1], "interior", 0.0)
    n_plain = len(xy)
    origins = np.array([(x, y, FIELD_TOP if k % 2 == 0 else FIELD_BOTTOM) for k, (x, y) in enumerate(xy)])
    directions = np.array([(0.0, 0.0, -1.0 if k % 2 == 0 else 1.0) for k in range(n_plain)])
    # rays that point away from the surface, from above and from below
    extra_o, extra_d = [], []
    for k, (x, y) in enumerate(((3.25, 4.5), (6.0, 8.0), (11.0, 12.0), (20.5, 2.25))):
        extra_o.append((x + FIELD_OFFSET, y + FIELD_OFFSET, FIELD_TOP if k % 2 == 0 else FIELD_BOTTOM)); extra_d.append((0.0, 0.0, 1.0 if k % 2 == 0 else -1.0))
        kind.append("away")
    # rays that start on the surface and one step past it: at a lattice vertex and at the middle of a cell's lower edge, where the
    # surface's height is a float64
    for (x, y, z) in ((8.0, 10.0, height[4, 5]), (13.0, 6.0, (height[6, 3] + height[7, 3]) / 2)):
        assert Fraction(float(z)) * 16 == int(Fraction(float(z)) * 16)
        x, y = x + FIELD_OFFSET, y + FIELD_OFFSET
        extra_o.append((x, y, z)); extra_d.append((0.0, 0.0, -1.0)); kind.append("surface")
        extra_o.append((x, y, z)); extra_d.append((0.0, 0.0, 1.0)); kind.append("surface")
        extra_o.append((x, y, np.nextafter(z, np.inf))); extra_d.append((0.0, 0.0, 1.0)); kind.append("past")
        extra_o.append((x, y, np.nextafter(z, -np.inf))); extra_d.append((0.0, 0.0, -1.0)); kind.append("past")
    origins = np.concatenate([origins, np.array(extra_o)])
    directions = np.concatenate([directions, np.array(extra_d)])
    order = rng.permutation(len(origins))
    return {"points": points, "faces": faces, "origins": origins[order], "directions": directions[order],
            "kind": np.array(kind)[order], "g": g}


def field_census(scene, winners):
    """What the winners of a stacked field's rays show: the counts of hits, of winners with u == 0, v == 0, u + v == 1 and
    t == 0, and of winners per chunk of 128 faces."""
    won = [w for w in winners if w is not None]
    chunks = np.bincount([w[0] // 128 for w in won], minlength=-(-len(scene["faces"]) // 128))
    return {"hits": len(won), "u0": sum(w[2] == 0 for w in won), "v0": sum(w[3] == 0 for w in won),
            "uv1": sum(w[2] + w[3] == 1 for w in won), "t0": sum(w[1] == 0 for w in won), "chunks": chunks.tolist()}


# -- what the host test and the device test both run --------------------------------------------------------------------------------
RAY_TILE = 256             # GR_RAY_TILE of csrc/rays.hip
EMBED_THRESHOLD = 200.0    # above the diameter of axis_segments() (coordinates below 64: under 111), below the filler's spacing


def embedded_segments(seed=0):
    """axis_segments() at shuffled positions among n = 2 RAY_TILE + 40 rays, the others non-parallel filler farther than
    EMBED_THRESHOLD from everything -> dict: starts, ends (n, 3), ids (n,) all distinct, pos (40,) the position of every scene
    segment, want = (i, j, d): the exact edges at EMBED_THRESHOLD, in positions, sorted."""
    seg_s, seg_e = axis_segments()
    m, n = len(seg_s), 2 * RAY_TILE + 40
    rng = np.random.default_rng(seed)
    fixed = list(range(RAY_TILE - 5, RAY_TILE + 5)) + list(range(2 * RAY_TILE - 6, 2 * RAY_TILE + 6)) + list(range(n - 8, n))
    rest = np.setdiff1d(np.arange(n), fixed)
    pos = rng.permutation(np.concatenate([fixed, rng.choice(rest, m - len(fixed), replace=False)]))
    assert len(set(pos.tolist())) == m
    for edge in (RAY_TILE, 2 * RAY_TILE):
        assert edge - 1 in pos and edge in pos            # the scene straddles both tile borders ...
    assert (pos >= 2 * RAY_TILE).sum() >= 8 and (pos < RAY_TILE - 5).any()   # ... and reaches into the ragged last tile
    # the filler: 1000 apart along x, at most 10 long, directions drawn at random
    k = np.arange(n, dtype=np.float64)
    starts = np.stack([1000.0 * (k + 2), rng.uniform(-5, 5, n), rng.uniform(-5, 5, n)], axis=1)
    ends = starts + rng.uniform(1, 5, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    starts[pos], ends[pos] = seg_s, seg_e
    filler = np.setdiff1d(np.arange(n), pos)
    unit = (ends - starts)[filler]
    unit /= np.sqrt((unit * unit).sum(axis=1))[:, None]
    cr = np.cross(unit[:, None, :], unit[None, :, :])
    assert ((cr * cr).sum(axis=2) + np.eye(len(filler)) > 0).all(), "two filler rays are parallel"
    assert np.abs(unit).max(axis=1).max() < 1, "a filler ray lies along an axis"
    assert 1000.0 - 20.0 > EMBED_THRESHOLD and 2000.0 - 64.0 - 10.0 > EMBED_THRESHOLD
    seg_at = {int(p): s for s, p in enumerate(pos)}
    places = sorted(seg_at)
    want = [(p, q, distance_exact(seg_s[seg_at[p]], seg_e[seg_at[p]], seg_s[seg_at[q]], seg_e[seg_at[q]]))
            for a, p in enumerate(places) for q in places[a + 1:]]
    want = [w for w in want if w[2] <= EMBED_THRESHOLD]
    return {"starts": starts, "ends": ends, "ids": rng.permutation(n).astype(np.int32), "pos": pos, "n": n,
            "want": (np.array([w[0] for w in want], np.int32), np.array([w[1] for w in want], np.int32),
                     np.array([w[2] for w in want], np.float64))}


def segment_communities():
    """Community layouts on axis_segments(): a list of (name, community (40,) int32, M)."""
    n = len(_AXIS_SEGMENTS)
    idx = np.arange(n)
    finite = idx != ZERO_LENGTH
    out = []
    out.append(("all finite members in one", np.where(finite, 0, -1).astype(np.int32), 1))
    three = np.where(finite, idx % 3, -1)
    three[[4, 17, 33]] = (-1, 3, 2**31 - 1)   # no community, M, far beyond M: ignored
    out.append(("three interleaved, some rays ignored", three.astype(np.int32), 3))
    with_zero = np.where(idx % 2 == 0, 2, 3)
    with_zero[[ZERO_LENGTH, 0, 7, 31]] = 0    # the zero-length segment among others: NaN; community 1 is empty: NaN
    out.append(("a zero-length member, an empty community", with_zero.astype(np.int32), 4))
    alone = np.where(idx % 2 == 0, 0, 2)
    alone[ZERO_LENGTH] = 1
    out.append(("the zero-length segment alone", alone.astype(np.int32), 3))
    out.append(("all singletons", idx.astype(np.int32), n))
    return out


COMMUNITY_SIZES = (2, 3, 63, 64, 65, 255, 256, 257)   # around a wave, and around GR_COMM_POINTS_LDS = 256


def community_seed(m):
    return 11 if m >= 256 else m   # 256 and 257 share a seed: the first 256 members of the one are the other


def joined_communities(seed=3):
    """Every axis_community of COMMUNITY_SIZES in one call, their rays interleaved: starts, ends (965, 3), community (965,)
    int32, label: {m: its community}."""
    rng = np.random.default_rng(seed)
    label = dict(zip(COMMUNITY_SIZES, rng.permutation(len(COMMUNITY_SIZES)).tolist()))
    parts = [axis_community(m, community_seed(m)) for m in COMMUNITY_SIZES]
    starts, ends = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    community = np.concatenate([np.full(m, label[m], dtype=np.int32) for m in COMMUNITY_SIZES])
    order = rng.permutation(len(community))
    return starts[order], ends[order], community[order], label


def field_specials(scene):
    """The field with three triangles and some rays appended that the rules single out -> dict: points, faces, origins,
    directions, base (the field's own rays come first), model (the field ray that the last seven copy), and the indices
    in_plane, control, zero_direction, scaled, first_nonfinite of the appended rays."""
    points, faces = scene["points"], scene["faces"]
    V, g = len(points), scene["g"]
    more_p = [(100, 100, 5), (102, 100, 5), (100, 102, 5),     # a level triangle far from the field
              (100, 110, 5), (101, 110, 5), (102, 110, 5)]     # three collinear points
    more_f = [(V, V + 1, V + 2), (V + 3, V + 4, V + 5), (g + 1, g + 1, 2 * g + 2)]   # ... and a repeated vertex
    model = int(np.nonzero((scene["kind"] == "interior") & (scene["directions"][:, 2] < 0))[0][0])
    o = scene["origins"][model]
    nan, inf = float("nan"), float("inf")
    more_o = [(99, 100.5, 5), (100.5, 100.5, 9), (5, 5, 10), tuple(o),
              (nan, o[1], o[2]), (o[0], inf, o[2]), (o[0], o[1], -inf), tuple(o), tuple(o), tuple(o)]
    more_d = [(1, 0, 0), (0, 0, -1), (0, 0, 0), (0, 0, -4),
              (0, 0, -1), (0, 0, -1), (0, 0, -1), (0, 0, nan), (inf, 0, -1), (0, 0, -inf)]
    base = len(scene["origins"])
    return {"points": np.concatenate([points, np.array(more_p, dtype=np.float64)]),
            "faces": np.concatenate([faces, np.array(more_f, dtype=np.int32)]),
            "origins": np.concatenate([scene["origins"], np.array(more_o, dtype=np.float64)]),
            "directions": np.concatenate([scene["directions"], np.array(more_d, dtype=np.float64)]),
            "base": base, "model": model, "in_plane": base, "control": base + 1, "zero_direction": base + 2, "scaled": base + 3,
            "first_nonfinite": base + 4}


def nonfinite_vertices(scene):
    """The field's points with a NaN, a +inf and a -inf in three interior vertices (one coordinate each)."""
    g, points = scene["g"], scene["points"].copy()
    points[3 * g + 3, 0] = float("nan")
    points[7 * g + 9, 1] = float("inf")
    points[11 * g + 5, 2] = -float("inf")
    return points


def bad_index_cases(scene):
    """(face, value, faces with that one index replaced) for the faces 0, 127, 128, F - 1 and the values V, -1, INT32_MIN."""
    V, F = len(scene["points"]), len(scene["faces"])
    out = []
    for face in (0, 127, 128, F - 1):
        for col, value in enumerate((V, -1, INT32_MIN)):
            faces = scene["faces"].copy()
            faces[face, (face + col) % 3] = value
            out.append((face, value, faces))
    return out


FACE_PREFIXES = (1, 127, 128, 129, 255, 256, 257)   # around the chunk of GR_CLIP_CHUNK = 128 triangles
RAY_PREFIXES = (1, 63, 64, 65, 255, 256, 257, 513)  # around a wave and a workgroup of 256 rays
