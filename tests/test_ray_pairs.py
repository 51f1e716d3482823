"""gr_ray_pairs / gr_rays_clip on the device against the reference goldens (tests/golden/reference_triangulation.npz, made by
the real reference functions) and, where no golden can exist, against the numpy stand-in of tests/ray_standin.py.

Tolerances are not chosen here: `e_ref` is the reference's own float64 error against its long-double run, measured by the
fixture maker and stored; tol = 4 e_ref (2: another valid operation order may err to the other side; 2: slack).  The edge-set
tests demand EXACT equality, which is fair because no reference distance lies within tol of a tested threshold (re-asserted
here from the stored long-double distances; the share of pairs left out of the comparison is zero)."""
import ctypes

import numpy as np
import pytest

from geograypher_amd import _hip
from geograypher_amd.utils import numeric, synthetic
from tests.conftest import GOLDEN
from tests.ray_standin import StandInBackend, clip_rays_np, ray_pair_edges_np, rows_distance

pytestmark = pytest.mark.gpu
TILE = 256


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN / "reference_triangulation.npz", allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


def _np(t):
    return t.cpu().numpy()


def _ld(gold, key):
    return gold[key + "_hi"].astype(np.longdouble) + gold[key + "_lo"].astype(np.longdouble)


def _standin_tol(gold):
    """Device against the numpy stand-in on survey scenes (coordinates up to about 300, as in golden scene a): both are
    held to 4 e_ref against the reference's long-double run (the stand-in by tests/test_triangulation_host.py, the device by the
    golden tests here), so they are at most 8 e_ref apart."""
    return 8 * float(gold["a__e_ref"])


def _candidates(ids):
    n = len(ids)
    return np.triu(np.ones((n, n), dtype=bool), 1) & (ids[:, None] != ids[None, :])


@pytest.mark.parametrize("scene", ["a", "c"])
def test_edge_set_exact_and_distances_within_the_references_own_error(hip, gold, scene):
    starts, ends, ids = gold[f"{scene}__starts"], gold[f"{scene}__ends"], gold[f"{scene}__ids"]
    d64, dld = gold[f"{scene}__dist64"], _ld(gold, f"{scene}__distld")
    tol = 4 * float(gold[f"{scene}__e_ref"])
    cand = _candidates(ids)
    for t in gold[f"{scene}__thresholds"]:
        with np.errstate(invalid="ignore"):
            assert np.min(np.abs(dld[cand & np.isfinite(dld)] - t)) > tol, "a fixture pair sits on the threshold"
            want_i, want_j = np.nonzero(cand & (d64 <= t))
        i, j, d = (_np(x) for x in hip.ray_pair_edges(starts, ends, ids, float(t)))
        assert np.array_equal(i, want_i) and np.array_equal(j, want_j)
        err = np.abs(d.astype(np.longdouble) - dld[i, j])
        bit_equal = int((d == d64[i, j]).sum())
        print(f"scene {scene} threshold {t}: {len(i)} edges, max |d - d_longdouble| {float(err.max()):.3g} (tol {tol:.3g}), "
              f"{bit_equal} of {len(i)} bit-equal to the reference's float64")
        assert err.max() <= tol
        # the edge list of calc_graph_weights: content AND order, for both steps
        for step in gold[f"{scene}__steps"]:
            k = list(gold[f"{scene}__thresholds"]).index(t)
            ref = gold[f"{scene}__edges__t{k}__s{step}__none"]
            gi, gj, gw = numeric.ray_pair_edges(starts, ends, ids, float(t), step=int(step), backend=hip)
            assert np.array_equal(gi, ref[:, 0].astype(np.int64)) and np.array_equal(gj, ref[:, 1].astype(np.int64))
            # w = 1 / d: relative error of d carries over
            assert np.all(np.abs(gw - ref[:, 2]) <= tol * ref[:, 2] ** 2 + 4 * np.finfo(np.float64).eps * ref[:, 2])


def test_integer_scene_is_bit_equal_to_the_reference(hip, gold):
    """Parallel, collinear (overlapping, disjoint before / after), touching, duplicate and zero-length segments on integer
    coordinates: every intermediate is exact, so the distances equal the reference's float64 bit for bit."""
    starts, ends, ids, d64 = gold["b__starts"], gold["b__ends"], gold["b__ids"], gold["b__dist64"]
    cand = _candidates(ids)
    assert np.isnan(d64[7]).all(), "the zero-length segment has no distance in the reference"
    for t in gold["b__thresholds"]:
        with np.errstate(invalid="ignore"):
            want_i, want_j = np.nonzero(cand & (d64 <= t))
        i, j, d = (_np(x) for x in hip.ray_pair_edges(starts, ends, ids, float(t)))
        assert np.array_equal(i, want_i) and np.array_equal(j, want_j)
        assert np.array_equal(d, d64[i, j])
        assert 7 not in set(i) | set(j)
    # everything finite, through a huge threshold: before / after / middle all compared
    i, j, d = (_np(x) for x in hip.ray_pair_edges(starts, ends, ids, 1e9))
    want_i, want_j = np.nonzero(cand & np.isfinite(d64))
    assert np.array_equal(i, want_i) and np.array_equal(j, want_j) and np.array_equal(d, d64[i, j])
    # duplicates in different images: d = 0, weight 1 / min_dist after the host step
    gi, gj, gw = numeric.ray_pair_edges(starts, ends, ids, 0.0, backend=hip)
    pairs = list(zip(gi.tolist(), gj.tolist()))
    assert (0, 6) in pairs and (0, 15) not in pairs      # 15 duplicates 0 in the SAME image
    assert gw[pairs.index((0, 6))] == 1 / 1e-6


@pytest.fixture(scope="module")
def survey():
    return synthetic.detection_survey()


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_launch_edges(hip, gold, survey, n):
    starts, ends, ids = survey["ray_starts"][:n], survey["ray_ends"][:n], survey["ray_IDs"][:n]
    if n > 2:   # the first cameras' rays only would share few images: interleave the images
        pick = np.arange(n) * (len(survey["ray_IDs"]) // n)
        starts, ends, ids = survey["ray_starts"][pick], survey["ray_ends"][pick], survey["ray_IDs"][pick]
    want = ray_pair_edges_np(starts, ends, ids, 4.0)
    got = [_np(x) for x in hip.ray_pair_edges(starts, ends, ids, 4.0)]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert n < 2 or len(want[0]) == 0 or np.abs(got[2] - want[2]).max() <= _standin_tol(gold)
    assert hip.ray_pair_count(starts, ends, ids, 4.0) == len(want[0])
    if n >= 64:
        assert len(want[0]) > 0


def test_capacity_protocol(hip, survey):
    import torch

    starts, ends, ids = survey["ray_starts"], survey["ray_ends"], survey["ray_IDs"]
    want = ray_pair_edges_np(starts, ends, ids, 0.5)
    total = len(want[0])
    assert total > 1000
    for cap, calls in ((0, 2), (total - 1, 2), (total, 1), (None, 1)):
        got = [_np(x) for x in hip.ray_pair_edges(starts, ends, ids, 0.5, capacity=cap)]
        assert hip.last_ray_pair_calls == calls
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # the raw call: an overflow reports the total and leaves the buffers alone
    s_t, e_t, id_t = hip._ray_inputs(starts, ends, ids)
    ei = torch.full((total,), -7, dtype=torch.int32, device=hip.device)
    ej = torch.full((total,), -7, dtype=torch.int32, device=hip.device)
    ed = torch.full((total,), -7.0, dtype=torch.float64, device=hip.device)
    n_total = ctypes.c_int64(0)
    rc = hip.lib.gr_ray_pairs(hip._ctx, s_t.data_ptr(), e_t.data_ptr(), id_t.data_ptr(), len(ids), 0.5, ei.data_ptr(),
                              ej.data_ptr(), ed.data_ptr(), total - 1, ctypes.byref(n_total), hip._stream())
    assert rc == -6 and n_total.value == total
    assert bool((ei == -7).all()) and bool((ej == -7).all()) and bool((ed == -7.0).all())
    assert b"call again" in hip.lib.gr_last_error(hip._ctx)


def test_images_and_non_finite_coordinates(hip, survey):
    starts, ends, ids = survey["ray_starts"][:300].copy(), survey["ray_ends"][:300].copy(), survey["ray_IDs"][:300]
    assert len(hip.ray_pair_edges(starts, ends, np.zeros(300, dtype=np.int64), 1e9)[0]) == 0   # one image: no edge
    two = np.arange(300) % 2
    want = ray_pair_edges_np(starts, ends, two, 1.0)
    got = [_np(x) for x in hip.ray_pair_edges(starts, ends, two, 1.0)]
    assert len(want[0]) > 0 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    bad = {5: np.nan, 17: np.inf, 40: -np.inf}
    for k, v in bad.items():
        starts[k, k % 3] = v
    ends[77] = np.nan
    ends[90, 2] = np.inf
    ids2 = np.arange(300) % 7
    got = [_np(x) for x in hip.ray_pair_edges(starts, ends, ids2, 1e9)]
    touched = set(bad) | {77, 90}
    assert not (set(got[0]) | set(got[1])) & touched
    ok = np.array([k for k in range(300) if k not in touched])
    want = ray_pair_edges_np(starts[ok], ends[ok], ids2[ok], 1e9)
    assert np.array_equal(got[0], ok[want[0]]) and np.array_equal(got[1], ok[want[1]])
    assert np.isfinite(got[2]).all()


@pytest.fixture(scope="module")
def big(hip):
    """About 50 000 rays, on the device, with their edges at 0.5 from one call on the current stream."""
    b = synthetic.detection_survey(n_objects=2500, n_cameras=40, seed=4)
    b["dev"] = hip._ray_inputs(b["ray_starts"], b["ray_ends"], b["ray_IDs"])
    b["edges_dev"] = hip.ray_pair_edges(*b["dev"], 0.5)
    b["calls"] = hip.last_ray_pair_calls
    b["edges"] = [_np(x) for x in b["edges_dev"]]
    return b


def test_two_streams_share_the_scratch_in_turn(hip, big):
    """Two calls of one context on two streams, back to back: inputs already on the device, the capacity exact, nothing on the
    host between them but the second call itself.  Each sorts about two million edges through the context's scratch
    (milliseconds of device work), and the second call poisons that scratch first (GR_OPT_DEBUG 1024): were the first call's
    sort still running when gr_ray_pairs returned, its edges would come back torn.  Also the strided grid (2048)."""
    import torch

    s_t, e_t, id_t = big["dev"]
    want = big["edges"]
    total = len(want[0])
    assert total > 1_000_000
    streams = [torch.cuda.Stream(device=hip.device) for _ in range(2)]
    outs = []
    hip.set_option(_hip.GR_OPT_DEBUG, _hip.GR_DBG_POISON_RAYS)
    try:
        for k, st in enumerate(streams):
            with torch.cuda.stream(st):
                outs.append(hip.ray_pair_edges(s_t[k:], e_t[k:], id_t[k:], 0.5, capacity=total))
                assert hip.last_ray_pair_calls == 1
        for st in streams:
            st.synchronize()
        hip.set_option(_hip.GR_OPT_DEBUG, _hip.GR_DBG_POISON_RAYS | _hip.GR_DBG_RAY_GRID_7)
        strided = [_np(x) for x in hip.ray_pair_edges(s_t, e_t, id_t, 0.5, capacity=total)]
        strided_count = hip.ray_pair_count(s_t, e_t, id_t, 0.5)
    finally:
        hip.set_option(_hip.GR_OPT_DEBUG, 0)
    got0 = [_np(x) for x in outs[0]]
    assert all(np.array_equal(a, b) for a, b in zip(got0, want))
    keep = want[0] >= 1   # the second call dropped ray 0: the same edges, indices one lower
    got1 = [_np(x) for x in outs[1]]
    assert np.array_equal(got1[0], want[0][keep] - 1) and np.array_equal(got1[1], want[1][keep] - 1)
    assert np.array_equal(got1[2], want[2][keep])
    assert all(np.array_equal(a, b) for a, b in zip(strided, want)) and strided_count == total


def test_poisoned_scratch_strided_grid_and_permutation(hip, gold, survey):
    starts, ends, ids = survey["ray_starts"], survey["ray_ends"], survey["ray_IDs"]
    want = ray_pair_edges_np(starts, ends, ids, 0.5)
    poison, grid7 = _hip.GR_DBG_POISON_RAYS, _hip.GR_DBG_RAY_GRID_7
    for dbg in (poison, grid7, poison | grid7):   # poisoned scratch; 7 workgroups striding over the 15 tiles; both
        hip.set_option(_hip.GR_OPT_DEBUG, dbg)
        try:
            got = [_np(x) for x in hip.ray_pair_edges(starts, ends, ids, 0.5)]
            count = hip.ray_pair_count(starts, ends, ids, 0.5)
        finally:
            hip.set_option(_hip.GR_OPT_DEBUG, 0)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and count == len(want[0])
        assert np.abs(got[2] - want[2]).max() <= _standin_tol(gold)
    perm = np.random.default_rng(1).permutation(len(ids))
    pi, pj, pd = (_np(x) for x in hip.ray_pair_edges(starts[perm], ends[perm], ids[perm], 0.5))
    a, b = perm[pi], perm[pj]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    order = np.lexsort((hi, lo))
    assert np.array_equal(lo[order], want[0]) and np.array_equal(hi[order], want[1])
    # the distance of (j, i) is not bitwise that of (i, j) (A and B are not treated alike), but both are the reference's
    # float64 up to its own error on coordinates of this size
    assert np.abs(pd[order] - want[2]).max() <= _standin_tol(gold)


def test_scale_fifty_thousand_rays(hip, gold, big):
    """No all-pairs oracle at this size: 200 sampled rows against the stand-in over all columns, and the total against two
    decompositions.  Row ranges: the edges whose row i lies in [r0, r1) number count(rays[r0:]) - count(rays[r1:]) -- two
    count-only calls on suffixes, with other N and other tiles than the full call -- and the edge list must hold exactly that
    many rows in every range (summed over the ranges this is the total; range by range it also catches a miscount that
    depends on the tile row).  Image groups, beyond what the issue names: edges inside group 0, inside group 1 and across."""
    starts, ends, ids = big["ray_starts"], big["ray_ends"], big["ray_IDs"]
    n = len(ids)
    assert 45_000 < n < 55_000
    i, j, d = big["edges"]
    total = len(i)
    print(f"{n} rays, {total} edges at 0.5, {big['calls']} call(s)")
    assert np.all(i < j) and np.all(ids[i] != ids[j]) and np.all(d <= 0.5)
    key = i.astype(np.int64) * n + j
    assert np.all(np.diff(key) > 0), "sorted by (i, j), no duplicates"
    # 200 sampled rows against the stand-in over all columns (1e7 pairs)
    rows = np.sort(np.random.default_rng(0).choice(n, 200, replace=False))
    for r0 in range(0, 200, 20):
        rr = rows[r0:r0 + 20]
        ds = rows_distance(starts, ends, rr)
        with np.errstate(invalid="ignore"):
            keep = (rr[:, None] < np.arange(n)[None, :]) & (ids[rr][:, None] != ids[None, :]) & (ds <= 0.5)
        near = np.abs(ds - 0.5) <= _standin_tol(gold)   # a pair this close to the threshold may fall either way: left out, and counted
        assert not near.any()
        wi, wj = np.nonzero(keep)
        sel = np.isin(i, rr)
        assert np.array_equal(i[sel], rr[wi]) and np.array_equal(j[sel], wj)
        assert np.abs(d[sel] - ds[wi, wj]).max() <= _standin_tol(gold)
    # row ranges (the docstring above)
    s_t, e_t, id_t = big["dev"]
    bounds = [0, 255, 256, 10_000, 25_001, 49_000, n]
    suffix = [hip.ray_pair_count(s_t[r:], e_t[r:], id_t[r:], 0.5) for r in bounds]
    assert suffix[0] == total and suffix[-1] == 0
    for r0, r1, c0, c1 in zip(bounds[:-1], bounds[1:], suffix[:-1], suffix[1:]):
        assert int(((i >= r0) & (i < r1)).sum()) == c0 - c1, (r0, r1)
    # images split in two groups -> edges inside group 0, inside group 1 (two calls on subsets: other N, other tiles) and
    # across (all rays, images relabelled to their group)
    group = ids % 2
    inside = [hip.ray_pair_count(starts[group == g], ends[group == g], ids[group == g], 0.5) for g in (0, 1)]
    across = hip.ray_pair_count(starts, ends, group, 0.5)
    assert sum(inside) + across == total
    assert hip.ray_pair_count(starts, ends, ids, 0.5) == total


@pytest.mark.parametrize("tag", ["ceil", "floor"])
def test_rays_clip_against_long_double(hip, gold, tag):
    origins, directions = gold["clip__origins"], gold["clip__directions"]
    points, faces = gold[f"clip__{tag}__points"], gold[f"clip__{tag}__faces"]
    _, _, _, margin = clip_rays_np(origins, directions, points, faces)
    excluded = margin <= 1e-6   # rays aimed at a shared edge or vertex could take either triangle: none in the fixture
    assert excluded.sum() == 0
    hit, t, pts = (_np(x) for x in hip.clip_rays(origins, directions, points, faces))
    assert hit.all()
    e_t = np.abs(t.astype(np.longdouble) - _ld(gold, f"clip__{tag}__t")).max()
    e_p = np.abs(pts.astype(np.longdouble) - _ld(gold, f"clip__{tag}__p")).max()
    print(f"clip {tag}: |t - t_ld| {float(e_t):.3g} (tol {4 * float(gold[f'clip__{tag}__e_t']):.3g}), "
          f"|p - p_ld| {float(e_p):.3g} (tol {4 * float(gold[f'clip__{tag}__e_p']):.3g})")
    assert e_t <= 4 * float(gold[f"clip__{tag}__e_t"]) and e_p <= 4 * float(gold[f"clip__{tag}__e_p"])


def test_rays_clip_misses_limits_and_bad_faces(hip, gold):
    points, faces = gold["clip__floor__points"], gold["clip__floor__faces"]
    origins = np.array([[0.0, 0.0, 50.0], [0.0, 0.0, 50.0], [1e4, 0.0, 50.0], [10.0, 10.0, -50.0]])
    directions = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 1.0]])
    hit, t, pts = (_np(x) for x in hip.clip_rays(origins, directions, points, faces))
    assert hit.tolist() == [True, False, False, True]      # away from it; beside it; from below (double-sided)
    assert np.isnan(t[1]) and np.isnan(pts[2]).all()
    bad = faces.copy()
    bad[:, 0] = 10_000   # indices beyond the points: such faces are never hit (and never read)
    assert not _np(hip.clip_rays(origins, directions, points, bad)[0]).any()
    assert _np(hip.clip_rays(origins[:0], directions[:0], points, faces)[0]).shape == (0,)
    with pytest.raises(ValueError, match="at most 65536"):
        hip.clip_rays(origins, directions, points, np.zeros((65537, 3), dtype=np.int32))


def test_triangulate_detections_device_equals_stand_in(hip, tmp_path):
    s = synthetic.detection_survey(n_objects=30, n_cameras=30, seed=2)
    cams, det = synthetic.detection_survey_cameras(s)
    bounds = (synthetic.boundary_grid(9, lambda x, y: 30.0 + 0.01 * x), synthetic.boundary_grid(9, lambda x, y: -2.0 + 0 * x))
    kw = dict(boundaries=bounds, similarity_threshold_meters=0.5, louvain_resolution=2.0, seed=3)
    (tmp_path / "dev").mkdir()
    (tmp_path / "host").mkdir()
    got = cams.triangulate_detections(det, out_dir=tmp_path / "dev", backend=hip, **kw)
    want = cams.triangulate_detections(det, out_dir=tmp_path / "host", backend=StandInBackend(), **kw)
    import json

    e_dev = json.load(open(tmp_path / "dev" / "edge_weights.json"))
    e_host = json.load(open(tmp_path / "host" / "edge_weights.json"))
    assert [(a, b) for a, b, _ in e_dev] == [(a, b) for a, b, _ in e_host] and len(e_dev) > 100
    with np.load(tmp_path / "dev" / "communities.npz") as a, np.load(tmp_path / "host" / "communities.npz") as b:
        assert np.array_equal(a["ray_IDs"], b["ray_IDs"], equal_nan=True)
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-9
    # default backend: the shared HipRaster of the device
    assert np.array_equal(cams.triangulate_detections(det, **kw), got)
