"""gr_ray_pairs, gr_community_points and gr_rays_clip on the exact scenes of tests/ray_edge_scenes.py, bit for bit against the
rational references there (tests/test_ray_edges_host.py holds the numpy stand-ins to the same references, which is what makes
"bit for bit" the right demand: every intermediate of the float64 computation is exact on these scenes).  No tolerance in this
file.  What each test would catch is listed in DESIGN.md (section 8, "Multiview detections", and section 8p)."""
import numpy as np
import pytest

from geograypher_amd import _hip
from tests import ray_edge_scenes as sc

pytestmark = pytest.mark.gpu


def _np(x):
    return x.cpu().numpy()


class debug:
    """GR_OPT_DEBUG set for a block."""

    def __init__(self, hip, flags):
        self.hip, self.flags = hip, flags

    def __enter__(self):
        self.hip.set_option(_hip.GR_OPT_DEBUG, self.flags)

    def __exit__(self, *exc):
        self.hip.set_option(_hip.GR_OPT_DEBUG, 0)


# -- gr_ray_pairs -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def embedded():
    return sc.embedded_segments()


@pytest.mark.parametrize("flags", (0, _hip.GR_DBG_RAY_GRID_7, _hip.GR_DBG_POISON_RAYS, _hip.GR_DBG_RAY_GRID_7 | _hip.GR_DBG_POISON_RAYS))
def test_ray_pairs_parallel_branch_reads_global_indices(hip, embedded, flags):
    """Parallel, collinear, touching and duplicate segments in all three tiles of 552 rays and across the tile borders: the
    parallel branch reads ends[3 j] and ends[3 ia] by the rays' places in the whole call."""
    e = embedded
    with debug(hip, flags):
        i, j, d = (_np(x) for x in hip.ray_pair_edges(e["starts"], e["ends"], e["ids"], sc.EMBED_THRESHOLD))
        count = hip.ray_pair_count(e["starts"], e["ends"], e["ids"], sc.EMBED_THRESHOLD)
    scene = np.isin(i, e["pos"]) & np.isin(j, e["pos"])
    assert scene.all(), "an edge with a filler ray"
    want = e["want"]
    assert count == len(want[0]) == len(i)
    assert np.array_equal(i, want[0]) and np.array_equal(j, want[1])
    wrong = np.nonzero(d.view(np.uint64) != want[2].view(np.uint64))[0]
    assert wrong.size == 0, [(int(i[k]), int(j[k]), float(d[k]), float(want[2][k])) for k in wrong[:5]]


# -- gr_community_points ------------------------------------------------------------------------------------------------------------
def test_community_points_layouts_on_axis_segments(hip):
    starts, ends = sc.axis_segments()
    for name, community, M in sc.segment_communities():
        got = _np(hip.community_points(starts, ends, community, M))
        assert got.shape == (M, 3) and sc.same_bits(got, sc.community_points_exact(starts, ends, community, M)), name


@pytest.fixture(scope="module")
def communities():
    out = {}
    for m in sc.COMMUNITY_SIZES:
        starts, ends = sc.axis_community(m, sc.community_seed(m))
        out[m] = (starts, ends, sc.community_points_exact(starts, ends, np.zeros(m, dtype=np.int32), 1))
    return out


@pytest.mark.parametrize("m", sc.COMMUNITY_SIZES)
def test_community_points_one_community_of(hip, communities, m):
    """n = m rays: 2, 255, 256 and 257 are also the edges of the preparation kernels' workgroup."""
    starts, ends, want = communities[m]
    got = _np(hip.community_points(starts, ends, np.zeros(m, dtype=np.int32), 1))
    assert sc.same_bits(got, want), (got, want)


def test_community_points_both_sides_of_the_lds_limit_on_the_same_rays(hip, communities):
    """257 rays of which the first 256 form the community (members in LDS), then all 257 (records from global memory): each is
    its own exact mean, and tests/test_ray_edges_host.py shows that the two exact sums differ by the last member's pairs."""
    starts, ends, want257 = communities[257]
    first = np.where(np.arange(257) < 256, 0, -1).astype(np.int32)
    assert sc.same_bits(_np(hip.community_points(starts, ends, first, 1)), communities[256][2])
    assert sc.same_bits(_np(hip.community_points(starts, ends, np.zeros(257, dtype=np.int32), 1)), want257)
    # ... and both in one call: a ray has one label, so the smaller community is a copy of the first 256 rays appended
    s2, e2 = np.concatenate([starts, starts[:256]]), np.concatenate([ends, ends[:256]])
    both = np.concatenate([np.zeros(257, dtype=np.int32), np.ones(256, dtype=np.int32)])
    got = _np(hip.community_points(s2, e2, both, 2))
    assert sc.same_bits(got[0], want257[0]) and sc.same_bits(got[1], communities[256][2][0])


def test_community_points_joined_and_a_second_call_on_the_grown_scratch(hip, communities):
    starts, ends, community, label = sc.joined_communities()
    M = len(label)
    want = np.stack([communities[m][2][0] for m in sorted(label, key=label.get)])
    seg_s, seg_e = sc.axis_segments()
    _, other, other_M = sc.segment_communities()[1]
    other_want = sc.community_points_exact(seg_s, seg_e, other, other_M)
    swapped = (M - 1 - community).astype(np.int32)   # other labels on the same rays
    for flags in (0, _hip.GR_DBG_POISON_STAGE):
        with debug(hip, flags):
            got = _np(hip.community_points(starts, ends, community, M))
            small = _np(hip.community_points(seg_s, seg_e, other, other_M))   # the scratch stays at the larger call's size
            back = _np(hip.community_points(starts, ends, swapped, M))
        assert sc.same_bits(got, want), flags
        assert sc.same_bits(small, other_want), flags
        assert sc.same_bits(back, want[::-1]), flags


# -- gr_rays_clip -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fields():
    out = {}
    for seed in (1, 2):
        f = sc.stacked_field(15, seed)
        f["hits"] = sc.clip_hits_exact(f["origins"], f["directions"], f["points"], f["faces"])
        f["want"] = sc.clip_outputs(f["origins"], f["directions"], sc.nearest_hits(f["hits"]))
        out[seed] = f
    return out


def _clip(hip, origins, directions, points, faces):
    hit, t, p = (_np(x) for x in hip.clip_rays(origins, directions, points, faces))
    assert hit.dtype == bool and np.array_equal(np.isnan(t), ~hit) and np.array_equal(np.isnan(p), np.repeat(~hit[:, None], 3, axis=1))
    return hit, t, p


def _same(got, want):
    return np.array_equal(got[0], want[0]) and sc.same_bits(got[1], want[1]) and sc.same_bits(got[2], want[2])


def _explain(got, want, f):
    rows = np.nonzero((got[0] != want[0]) | ~((got[1] == want[1]) | (np.isnan(got[1]) & np.isnan(want[1]))))[0]
    return [(int(r), str(f["kind"][r]) if r < len(f["kind"]) else "appended", bool(got[0][r]), float(got[1][r]), float(want[1][r])) for r in rows[:8]]


@pytest.mark.parametrize("seed", (1, 2))
def test_rays_clip_stacked_field(hip, fields, seed):
    """392 shuffled triangles: three whole chunks of 128 and one of 8, every chunk the winner of some rays; rays on shared
    edges, lattice vertices and the outer border hit, one step outside misses, t == 0 hits."""
    f = fields[seed]
    got = _clip(hip, f["origins"], f["directions"], f["points"], f["faces"])
    assert _same(got, f["want"]), _explain(got, f["want"], f)


@pytest.mark.parametrize("prefix", sc.FACE_PREFIXES)
def test_rays_clip_face_prefixes(hip, fields, prefix):
    f = fields[1]
    want = sc.clip_outputs(f["origins"], f["directions"], sc.nearest_hits(f["hits"], prefix))
    got = _clip(hip, f["origins"], f["directions"], f["points"], f["faces"][:prefix])
    assert _same(got, want), _explain(got, want, f)


def test_rays_clip_ray_prefixes(hip, fields):
    f = fields[2]
    full = _clip(hip, f["origins"], f["directions"], f["points"], f["faces"])
    assert len(f["origins"]) >= max(sc.RAY_PREFIXES)
    for n in sc.RAY_PREFIXES:
        got = _clip(hip, f["origins"][:n], f["directions"][:n], f["points"], f["faces"])
        assert got[0].shape == (n,) and np.array_equal(got[0], full[0][:n])
        assert np.array_equal(got[1].view(np.uint64), full[1][:n].view(np.uint64)), n
        assert np.array_equal(got[2].view(np.uint64), full[2][:n].view(np.uint64)), n


def test_rays_clip_never_a_hit(hip, fields):
    """A ray in a triangle's plane, a zero direction, a triangle with a repeated vertex or three collinear ones, NaN and
    infinities in an origin, a direction or a vertex: never a hit, NaN outputs, and every other ray as in the plain run.  A
    direction of length 4 gives t / 4 and the same point."""
    f = fields[1]
    sp = sc.field_specials(f)
    want = sc.clip_exact(sp["origins"], sp["directions"], sp["points"], sp["faces"])
    got = _clip(hip, sp["origins"], sp["directions"], sp["points"], sp["faces"])
    assert _same(got, want), _explain(got, want, f)
    base = sp["base"]
    assert _same(tuple(x[:base] for x in got), f["want"])
    assert not got[0][sp["in_plane"]] and got[0][sp["control"]] and not got[0][sp["zero_direction"]] and not got[0][sp["first_nonfinite"]:].any()
    assert got[1][sp["scaled"]] == f["want"][1][sp["model"]] / 4 and sc.same_bits(got[2][sp["scaled"]], f["want"][2][sp["model"]])
    points = sc.nonfinite_vertices(f)
    want = sc.clip_exact(f["origins"], f["directions"], points, f["faces"])
    got = _clip(hip, f["origins"], f["directions"], points, f["faces"])
    assert _same(got, want), _explain(got, want, f)


def test_rays_clip_bad_indices_one_face_at_a_time(hip, fields):
    """Index V, -1 and INT32_MIN in one face of the first chunk's first and last slot, the second chunk's first slot and the
    last face: that face is never hit, its neighbours in the list still win their rays.  Index V - 1 is valid and wins."""
    f = fields[1]
    V = len(f["points"])
    full = sc.nearest_hits(f["hits"])
    corner = [r for r, w in enumerate(full) if w is not None and V - 1 in f["faces"][w[0]] and f["kind"][r] == "interior"]
    assert corner
    for face, value, faces in sc.bad_index_cases(f):
        want = sc.clip_outputs(f["origins"], f["directions"], sc.nearest_hits(f["hits"], without={face}))
        got = _clip(hip, f["origins"], f["directions"], f["points"], faces)
        assert _same(got, want), (face, value, _explain(got, want, f))
        assert got[0][corner].all()


def test_rays_clip_without_triangles(hip, fields):
    f = fields[1]
    got = _clip(hip, f["origins"], f["directions"], np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32))
    assert not got[0].any() and got[0].shape == (len(f["origins"]),)
