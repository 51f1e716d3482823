"""The rational references of tests/ray_edge_scenes.py against the numpy stand-ins and the package's host form, bit for bit, on
every scene that tests/test_ray_edges_gpu.py then puts to the device: this is what licenses "bit for bit" there.  It is also
the first pin of the parallel branches of the stand-ins on POINTS (the goldens of scene b hold distances), and it asserts that
the scenes contain what they claim, count by count."""
from fractions import Fraction

import numpy as np
import pytest

from geograypher_amd.utils import numeric
from tests import community_standin as cs
from tests import ray_edge_scenes as sc
from tests.ray_standin import clip_rays_np, pair_distance, ray_pair_edges_np


@pytest.fixture(scope="module")
def segments():
    return sc.axis_segments()


@pytest.fixture(scope="module")
def fields():
    out = {}
    for seed in (1, 2):
        f = sc.stacked_field(15, seed)
        f["hits"] = sc.clip_hits_exact(f["origins"], f["directions"], f["points"], f["faces"])
        out[seed] = f
    return out


def _pairs(n):
    i, j = np.divmod(np.arange(n * n), n)
    return i[i != j], j[i != j]


def test_axis_segments_holds_every_case(segments):
    starts, ends = segments
    assert len(starts) == 40
    assert sc.pair_kinds(starts, ends) == {"zero": 78, "before": 156, "after": 160, "middle": 208, "skew": 958, "oob_a": 738,
                                           "oob_b": 738, "oob_both": 572}
    # against segment 0 = [10, 20] on the x axis, as A and as B: the cases the table names
    kind = lambda a, b: sc.pair_kind_exact(starts[a], ends[a], starts[b], ends[b])
    assert [kind(0, b) for b in range(1, 18)] == ["before", "before", "after", "after", "after", "before", "middle", "middle",
                                                  "middle", "middle", "middle", "middle", "before", "after", "middle", "middle", "after"]
    assert [kind(b, 0) for b in (1, 2, 3, 4, 9, 7)] == ["after", "before", "before", "after", "middle", "middle"]
    assert kind(0, 31) == (False, False) and kind(0, 33) == (False, True) and kind(0, 34) == (True, True) and kind(33, 0) == (True, False)
    assert sc.closest_points_exact(starts[0], ends[0], starts[31], ends[31]) == ((15, 10, 10), (15, 10, 10))
    assert sc.closest_points_exact(starts[0], ends[0], starts[30], ends[30]) == sc.NAN
    # a wrong point that a distance cannot see: overlapping, B = [16, 28] travelling down from 28
    assert sc.closest_points_exact(starts[0], ends[0], starts[8], ends[8]) == ((20, 10, 10), (20, 10, 10))
    assert sc.closest_points_exact(starts[0], ends[0], starts[15], ends[15]) == ((16, 10, 10), (16, Fraction(27, 2), 12))


def test_points_of_the_host_form_equal_the_rational_reference(segments):
    starts, ends = segments
    pA, pB, dist = numeric.segment_closest_points(starts, ends, starts, ends)
    for i, j in zip(*_pairs(len(starts))):
        want = sc.closest_points_exact(starts[i], ends[i], starts[j], ends[j])
        if want == sc.NAN:
            assert np.isnan(pA[i, j]).all() and np.isnan(pB[i, j]).all() and np.isnan(dist[i, j])
            continue
        assert sc.same_bits(pA[i, j], [float(x) for x in want[0]]) and sc.same_bits(pB[i, j], [float(x) for x in want[1]]), (i, j)
        assert sc.same_bits(dist[i, j], sc.distance_exact(starts[i], ends[i], starts[j], ends[j]))


def test_pair_distance_equals_the_exact_distance(segments):
    starts, ends = segments
    i, j = _pairs(len(starts))
    want = np.array([sc.distance_exact(starts[a], ends[a], starts[b], ends[b]) for a, b in zip(i, j)])
    assert np.isnan(want).sum() == 78 and (want[~np.isnan(want)] == 0).sum() > 20
    assert sc.same_bits(pair_distance(starts, ends, i, j), want)


def test_points_of_the_stand_ins_pair_by_pair(segments):
    """Every unordered pair as a community of its own: the mean of pA(i, j), pB(i, j), pA(j, i), pB(j, i) is as close to the
    points of one pair as a community gets."""
    starts, ends = segments
    n = len(starts)
    iu, ju = np.triu_indices(n, 1)
    for lo in range(0, len(iu), n // 2):   # n / 2 disjoint-in-label communities per call of the stand-in
        rows = np.arange(lo, min(lo + n // 2, len(iu)))
        s = np.concatenate([starts[iu[rows]], starts[ju[rows]]])
        e = np.concatenate([ends[iu[rows]], ends[ju[rows]]])
        community = np.concatenate([np.arange(len(rows)), np.arange(len(rows))])
        want = sc.community_points_exact(s, e, community, len(rows))
        assert sc.same_bits(cs.community_points(s, e, community, len(rows)), want)
        for c in (0, len(rows) - 1):
            assert sc.same_bits(numeric.intersection_average(s[community == c], e[community == c]), want[c])


def test_community_layouts_on_axis_segments(segments):
    starts, ends = segments
    for name, community, M in sc.segment_communities():
        want = sc.community_points_exact(starts, ends, community, M)
        assert sc.same_bits(cs.community_points(starts, ends, community, M), want), name
        sizes = np.bincount(community[(community >= 0) & (community < M)], minlength=M)
        for c in range(M):
            if sizes[c] >= 2:
                assert sc.same_bits(numeric.intersection_average(starts[community == c], ends[community == c]), want[c]), (name, c)
            else:
                assert np.isnan(want[c]).all()
    layouts = {name: (community, M) for name, community, M in sc.segment_communities()}
    community, M = layouts["a zero-length member, an empty community"]
    want = sc.community_points_exact(starts, ends, community, M)
    assert np.isnan(want[:2]).all() and np.isfinite(want[2:]).all()
    community, M = layouts["three interleaved, some rays ignored"]
    assert np.isfinite(sc.community_points_exact(starts, ends, community, M)).all() and (community == 3).sum() == 1
    assert np.isnan(sc.community_points_exact(starts, ends, *layouts["all singletons"])).all()


@pytest.fixture(scope="module")
def communities():
    out = {}
    for m in sc.COMMUNITY_SIZES:
        starts, ends = sc.axis_community(m, sc.community_seed(m))
        out[m] = (starts, ends, sc.community_points_exact(starts, ends, np.zeros(m, dtype=np.int32), 1))
    return out


# ordered pairs of axis_community(m, community_seed(m)): before, after, middle, not parallel, of those oob_a, oob_b, both
KINDS = {
    2: (1, 1, 0, 0, 0, 0, 0),
    3: (1, 1, 0, 4, 3, 3, 2),
    63: (643, 191, 530, 2542, 1793, 1793, 1266),
    64: (426, 330, 564, 2712, 1933, 1933, 1388),
    65: (598, 282, 504, 2776, 1968, 1968, 1418),
    255: (8265, 4663, 8614, 43228, 30771, 30771, 21834),
    256: (8807, 4283, 8904, 43286, 30346, 30346, 21316),
    257: (8837, 4329, 8966, 43660, 30600, 30600, 21494),
}


@pytest.mark.parametrize("m", sc.COMMUNITY_SIZES)
def test_axis_community(communities, m):
    starts, ends, want = communities[m]
    parallel = sc.parallel_pairs(starts, ends)
    print(f"m = {m}: {parallel} of {m * (m - 1)} ordered pairs are parallel")
    assert m == 2 or 4 * parallel >= m * (m - 1)
    kinds = sc.pair_kinds(starts, ends)
    assert kinds["zero"] == 0 and kinds["before"] + kinds["after"] + kinds["middle"] == parallel
    assert tuple(kinds[k] for k in ("before", "after", "middle", "skew", "oob_a", "oob_b", "oob_both")) == KINDS[m]
    zeros = np.zeros(m, dtype=np.int32)
    assert sc.same_bits(cs.community_points(starts, ends, zeros, 1), want)
    assert sc.same_bits(numeric.intersection_average(starts, ends), want[0])


def test_256_and_257_members_share_their_first_256(communities):
    """The two sides of GR_COMM_POINTS_LDS on the same rays: the sum over 257 members less every pair with the last member is
    the sum over 256 (all sums are integers: exact in any order)."""
    s256, e256, _ = communities[256]
    s257, e257, _ = communities[257]
    assert np.array_equal(s257[:256], s256) and np.array_equal(e257[:256], e256)
    big, n_big = sc.community_sum_exact(s257, e257, list(range(257)))
    small, n_small = sc.community_sum_exact(s256, e256, list(range(256)))
    last = [0, 0, 0]
    for other in range(256):
        for a, b in ((256, other), (other, 256)):
            pA, pB = sc.closest_points_exact(s257[a], e257[a], s257[b], e257[b])
            last = [last[k] + pA[k] + pB[k] for k in range(3)]
    assert tuple(b - l for b, l in zip(big, last)) == small and n_big - 4 * 256 == n_small == 2 * 256 * 255


def test_joined_communities_are_the_single_ones(communities):
    starts, ends, community, label = sc.joined_communities()
    assert len(community) == sum(sc.COMMUNITY_SIZES) and sorted(label.values()) == list(range(len(label)))
    for m in (2, 3, 63, 257):
        mine = np.nonzero(community == label[m])[0]
        assert len(mine) == m and np.ptp(mine) > m   # interleaved with the others
        assert sc.same_bits(sc.community_points_exact(starts, ends, np.where(community == label[m], 0, -1), 1), communities[m][2])


def test_embedded_segments_on_the_stand_in():
    e = sc.embedded_segments()
    assert e["n"] == 2 * sc.RAY_TILE + 40 and len(np.unique(e["ids"])) == e["n"]
    i, j, d = ray_pair_edges_np(e["starts"], e["ends"], e["ids"], sc.EMBED_THRESHOLD)
    assert len(i) == 39 * 38 // 2 and np.isin(i, e["pos"]).all() and np.isin(j, e["pos"]).all()   # the filler meets nothing
    assert np.array_equal(i, e["want"][0]) and np.array_equal(j, e["want"][1]) and sc.same_bits(d, e["want"][2])
    # pairs that sit in different tiles, both ways round a tile border, are parallel: their j is not their place in the tile
    seg = {int(p): s for s, p in enumerate(e["pos"])}
    far = [(a, b) for a, b in zip(i.tolist(), j.tolist()) if b >= sc.RAY_TILE and isinstance(
        sc.pair_kind_exact(e["starts"][a], e["ends"][a], e["starts"][b], e["ends"][b]), str)]
    assert len(far) > 100 and any(a < sc.RAY_TILE for a, _ in far) and any(a >= 2 * sc.RAY_TILE for a, _ in far) and seg
    # ... and ends[3 i] is read in the "after" case alone: some of those have their A beyond the first tile
    after = [a for a, b in far if sc.pair_kind_exact(e["starts"][a], e["ends"][a], e["starts"][b], e["ends"][b]) == "after"]
    assert sum(a >= sc.RAY_TILE for a in after) >= 10


@pytest.mark.parametrize("seed", (1, 2))
def test_stacked_field(fields, seed):
    f = fields[seed]
    n, F = len(f["origins"]), len(f["faces"])
    assert F == 392 and F % 128 == 8 and 513 <= n <= 600
    winners = sc.nearest_hits(f["hits"])
    census = sc.field_census(f, winners)
    print(f"seed {seed}: {n} rays, {census}")
    assert census == {1: {"hits": 557, "u0": 66, "v0": 63, "uv1": 61, "t0": 4, "chunks": [213, 168, 160, 16]},
                      2: {"hits": 557, "u0": 65, "v0": 72, "uv1": 53, "t0": 4, "chunks": [214, 182, 145, 16]}}[seed]
    assert min(census["chunks"]) >= 10
    hit = np.array([w is not None for w in winners])
    for kind, count, hits in (("interior", 400, True), ("diagonal", 50, True), ("edge", 52, True), ("vertex", 25, True),
                              ("border", 26, True), ("outside", 8, False), ("surface", 4, True), ("past", 4, False), ("away", 4, False)):
        assert (f["kind"] == kind).sum() == count and (hit[f["kind"] == kind] == hits).all(), kind
    # both diagonals carry rays with u + v == 1, u == 0 or v == 0, and every face wins a ray
    assert set(w[0] for w in winners if w is not None) == set(range(F))
    ties = sum(len({h[1] for h in mine}) == 1 and len(mine) >= 2 for mine in f["hits"])
    assert ties >= 100   # rays on shared edges and vertices hit several triangles at one t
    # vertex V - 1 is valid and wins
    assert any(w is not None and len(f["points"]) - 1 in f["faces"][w[0]] for w in winners)
    got = clip_rays_np(f["origins"], f["directions"], f["points"], f["faces"])
    want = sc.clip_outputs(f["origins"], f["directions"], winners)
    assert np.array_equal(got[0], want[0]) and sc.same_bits(got[1], want[1]) and sc.same_bits(got[2], want[2])
    again = sc.clip_exact(f["origins"], f["directions"], f["points"], f["faces"])
    assert np.array_equal(again[0], want[0]) and sc.same_bits(again[1], want[1]) and sc.same_bits(again[2], want[2])
    for prefix in sc.FACE_PREFIXES:
        got = clip_rays_np(f["origins"], f["directions"], f["points"], f["faces"][:prefix])
        want = sc.clip_outputs(f["origins"], f["directions"], sc.nearest_hits(f["hits"], prefix))
        assert np.array_equal(got[0], want[0]) and sc.same_bits(got[1], want[1]) and sc.same_bits(got[2], want[2]), prefix
        assert want[0].sum() >= min(prefix, 128)


def test_rays_and_triangles_the_rules_single_out(fields):
    f = fields[1]
    sp = sc.field_specials(f)
    want = sc.clip_exact(sp["origins"], sp["directions"], sp["points"], sp["faces"])
    got = clip_rays_np(sp["origins"], sp["directions"], sp["points"], sp["faces"])
    assert np.array_equal(got[0], want[0]) and sc.same_bits(got[1], want[1]) and sc.same_bits(got[2], want[2])
    base, full = sp["base"], sc.clip_outputs(f["origins"], f["directions"], sc.nearest_hits(f["hits"]))
    assert np.array_equal(want[0][:base], full[0]) and sc.same_bits(want[1][:base], full[1])   # nothing else is disturbed
    hit = want[0]
    assert not hit[sp["in_plane"]] and hit[sp["control"]] and want[1][sp["control"]] == 4.0 and not hit[sp["zero_direction"]]
    assert hit[sp["scaled"]] and want[1][sp["scaled"]] == full[1][sp["model"]] / 4 and sc.same_bits(want[2][sp["scaled"]], full[2][sp["model"]])
    assert not hit[sp["first_nonfinite"]:].any() and len(hit) - sp["first_nonfinite"] == 6
    points = sc.nonfinite_vertices(f)
    want = sc.clip_exact(f["origins"], f["directions"], points, f["faces"])
    got = clip_rays_np(f["origins"], f["directions"], points, f["faces"])
    assert np.array_equal(got[0], want[0]) and sc.same_bits(got[1], want[1]) and sc.same_bits(got[2], want[2])
    assert 10 <= (want[0] != full[0]).sum() <= 30   # the interiors of the faces around the three vertices, and the vertices


def test_bad_index_cases_take_one_face_out(fields):
    f = fields[1]
    full = sc.nearest_hits(f["hits"])
    for face, value, faces in sc.bad_index_cases(f):
        assert (faces != f["faces"]).sum() == 1 and not 0 <= faces[face].min() < faces[face].max() < len(f["points"])
        want = sc.clip_exact(f["origins"], f["directions"], f["points"], faces)
        less_winners = sc.nearest_hits(f["hits"], without={face})
        less = sc.clip_outputs(f["origins"], f["directions"], less_winners)
        assert np.array_equal(want[0], less[0]) and sc.same_bits(want[1], less[1]) and sc.same_bits(want[2], less[2])
        lost = [r for r, w in enumerate(full) if w is not None and w[0] == face]
        assert lost and not want[0][[r for r in lost if f["kind"][r] == "interior"]].any()
        neighbours = {face - 1, face + 1} & set(range(len(faces)))
        assert all(any(w is not None and w[0] == k for w in less_winners) for k in neighbours)
