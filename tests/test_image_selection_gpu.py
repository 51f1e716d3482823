"""gr_set_cover on the device against the stand-in of the rule-set (tests/setcover_standin.py): every
array of the record and its counts are EQUAL -- integers, no tolerance -- on the hand-worked cases, at the edges of the pick
reduction, of the apply kernel and of the batch loop, on prune chains, on random and survey-like incidences on both sides of the
LDS-histogram limit, and behind the projection path."""
import functools

import numpy as np
import pytest
from scipy import sparse

from geograypher_amd import _hip
from tests import setcover_standin as standin
from tests.test_image_selection_host import hand_cases, prune_chain_cases

pytestmark = pytest.mark.gpu

LDS_VIEWS = _hip.GR_SETCOVER_LDS_VIEWS
BATCH = _hip.GR_SETCOVER_BATCH


def _device(hip, A, min_obs=1, prune=True, **kwargs):
    csr = standin.incidence(A)
    return hip.set_cover(csr.indptr.astype(np.int64), csr.indices.astype(np.int32), csr.shape[0], csr.shape[1],
                         min_observations=min_obs, prune=prune, **kwargs)


def _assert_same(got, want):
    for name, dtype in (("selected", np.bool_), ("order", np.int32), ("gains", np.int64), ("pruned", np.int32)):
        assert got[name].dtype == dtype, name
        assert np.array_equal(got[name], want[name]), (name, got[name][:20], want[name][:20])
    counts = lambda r: (r["n_required"], r["n_covered"], len(r["order"]), len(r["pruned"]))   # n_required, n_covered, k, p
    assert counts(got) == counts(want)
    assert got["n_required"] == got["n_covered"]


def _check(hip, A, min_obs=1, prune=True, want=None, both_paths=True):
    """the device record equals the stand-in's, through the LDS histograms (where n_views allows them) and through global atomics"""
    want = standin.set_cover(A, min_obs, prune) if want is None else want
    got = _device(hip, A, min_obs, prune)
    _assert_same(got, want)
    assert got["lds_histogram"] == (sparse.csr_matrix(A).shape[1] <= LDS_VIEWS)
    if both_paths and got["lds_histogram"]:
        other = _device(hip, A, min_obs, prune, global_atomics=True)
        assert not other["lds_histogram"]
        _assert_same(other, want)
    return got


def _from_lists(n_faces, view_faces):
    ii = np.concatenate([np.asarray(f, dtype=np.int64) for f in view_faces]) if view_faces else np.zeros(0, dtype=np.int64)
    jj = np.concatenate([np.full(len(f), v, dtype=np.int64) for v, f in enumerate(view_faces)]) if view_faces else ii
    return sparse.csr_matrix((np.ones(len(ii), dtype=bool), (ii, jj)), shape=(n_faces, len(view_faces)))


def _disjoint(counts):
    """view v sees counts[v] faces of its own"""
    starts = np.concatenate([[0], np.cumsum(counts)])
    return _from_lists(int(starts[-1]), [np.arange(starts[v], starts[v + 1]) for v in range(len(counts))])


# -- the hand-worked cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_worked(hip, name):
    A, min_obs, prune, want = hand_cases()[name]
    got = _check(hip, A, min_obs, prune)
    assert got["selected"].tolist() == want["selected"] and got["order"].tolist() == want["order"]
    assert got["gains"].tolist() == want["gains"] and got["pruned"].tolist() == want["pruned"]
    assert got["n_required"] == got["n_covered"] == want["n_required"]


@pytest.mark.parametrize("name", sorted(prune_chain_cases()))
def test_prune_chain(hip, name):
    """removing one view makes the next examined view needed: m is lowered before the next test (M6)"""
    A, min_obs, prune, want = prune_chain_cases()[name]
    got = _check(hip, A, min_obs, prune)
    assert got["selected"].tolist() == want["selected"] and got["pruned"].tolist() == want["pruned"]
    assert standin.covers(A, standin.required_faces(A, min_obs), got["selected"])


def test_values_and_explicit_zeros_play_no_part(hip):
    from geograypher_amd.utils.numeric import select_covering_views

    A = sparse.csr_matrix((np.array([5.0, 0.0, -2.0, 1.0]), np.array([0, 1, 1, 0]), np.array([0, 2, 3, 4])), shape=(3, 2))
    want = standin.set_cover(A)
    for form in (A, A.tocoo(), A.tocsc(), A.toarray()):
        _assert_same(select_covering_views(form, backend=hip), want)


# -- the pick reduction ---------------------------------------------------------------------------------------------------------
PICK_SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, LDS_VIEWS - 1, LDS_VIEWS, LDS_VIEWS + 1]


@pytest.mark.parametrize("n_views", PICK_SIZES)
def test_pick_sizes_with_ties(hip, n_views):
    """disjoint views of 1-3 faces: every pick is a tie among many views spread over all lanes and waves of the reduction"""
    counts = np.random.default_rng(n_views).integers(1, 4, n_views)
    got = _check(hip, _disjoint(counts), both_paths=n_views <= 1025)
    assert len(got["order"]) == n_views


@pytest.mark.parametrize("winners", [(0,), (63,), (0, 63), (63, 64), (64, 127), (127, 128), (1023, 1024), (0, 1299), (1299,), (5, 70, 700)],
                         ids=lambda w: "-".join(map(str, w)))
def test_pick_tie_positions(hip, winners):
    """the tied maxima sit in the first lane, the last lane, on both sides of a wave boundary, of the workgroup's stride, at the end"""
    counts = np.full(1300, 2)
    counts[list(winners)] = 7
    got = _check(hip, _disjoint(counts), both_paths=False)
    assert got["order"][:len(winners)].tolist() == sorted(winners)
    assert got["order"][len(winners):len(winners) + 3].tolist() == [v for v in range(8) if v not in winners][:3]


# -- the apply kernel -----------------------------------------------------------------------------------------------------------
def test_one_face(hip):
    got = _check(hip, np.ones((1, 3), dtype=bool))
    assert got["order"].tolist() == [0] and got["gains"].tolist() == [1]


@pytest.mark.parametrize("n_views", [2, 64, 65, 300])
def test_a_face_seen_by_all_views(hip, n_views):
    A = sparse.vstack([_disjoint(np.full(n_views, 3)), sparse.csr_matrix(np.ones((1, n_views), dtype=bool))]).tocsr()
    _check(hip, A)
    _check(hip, A, min_obs=2)   # the shared face alone is required: view 0 and nothing else


def test_rows_of_length_1_64_65(hip):
    rng = np.random.default_rng(5)
    n_views, rows = 70, []
    for length in [1, 64, 65, 1, 65, 64, 2, 63, 70] * 40:
        row = np.zeros(n_views, dtype=bool)
        row[rng.choice(n_views, length, replace=False)] = True
        rows.append(row)
    A = np.array(rows)
    for min_obs in (1, 2, 64, 65, 66):
        _check(hip, A, min_obs)


def test_a_view_that_sees_every_face(hip):
    A = standin.random_incidence(3000, 90, 0.1, 3).tolil()
    A[:, 41] = True
    got = _check(hip, A.tocsr())
    assert got["order"].tolist() == [41] and got["gains"].tolist() == [3000] and len(got["pruned"]) == 0


def test_empty_rows_between_full_ones(hip):
    A = standin.random_incidence(4000, 50, 0.2, 4).tolil()
    A[::2] = False       # every other row empty
    A[1::6] = True       # ... and full ones among the rest
    got = _check(hip, A.tocsr())
    assert got["n_required"] == 2000
    _check(hip, A.tocsr(), min_obs=50)


# -- the batch loop -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_views", [BATCH - 1, BATCH, BATCH + 1, 3 * BATCH])
def test_batch_boundary(hip, n_views):
    """N disjoint views of equal size: N picks in index order, then the pick that finds nothing; what is enqueued behind it does nothing"""
    for prune in (True, False):
        got = _check(hip, _disjoint(np.full(n_views, 2)), prune=prune, both_paths=False)
        assert got["order"].tolist() == list(range(n_views)) and got["gains"].tolist() == [2] * n_views
        assert got["selected"].all() and len(got["pruned"]) == 0
        assert got["batches"] == n_views // BATCH + 1   # the picks 0 .. N - 1 select, pick N sets `done`


# -- random and survey-like incidences ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_case(density, seed):
    return standin.random_incidence(5000, 300, density, seed)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("density", [0.005, 0.05, 0.4])
def test_random_incidences(hip, density, seed):
    A = _random_case(density, seed)
    for min_obs in (1, 2, 3):
        for prune in (True, False):
            _check(hip, A, min_obs, prune)


@functools.lru_cache(maxsize=None)
def _footprints():
    return standin.footprint_incidence(200_000, 500, 7)


@pytest.mark.parametrize("min_obs", [1, 2, 3])
def test_footprints(hip, min_obs):
    A = _footprints()
    assert A.shape[0] > 199_000 and A.nnz > 1_000_000
    pruned = _check(hip, A, min_obs, True)
    _check(hip, A, min_obs, False)
    required = standin.required_faces(A, min_obs)
    assert standin.covers(A, required, pruned["selected"])


@pytest.mark.parametrize("n_views", [LDS_VIEWS, LDS_VIEWS + 1])
def test_random_on_both_sides_of_the_lds_limit(hip, n_views):
    A = standin.random_incidence(5000, n_views, 0.005, n_views)
    for min_obs in (1, 3):
        _check(hip, A, min_obs, True)


# -- input errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["index_equals_n_views", "negative_index", "pointer_beyond_nnz", "pointer_decreases"])
def test_bad_input_is_a_value_error_and_the_context_survives(hip, bad):
    ptr = np.array([0, 2, 3, 5], dtype=np.int64)
    views = np.array([0, 1, 2, 0, 3], dtype=np.int32)
    if bad == "index_equals_n_views":
        views[3] = 4
    elif bad == "negative_index":
        views[1] = -1
    elif bad == "pointer_beyond_nnz":
        ptr[2] = 9
    else:
        ptr[1], ptr[2] = 3, 2
    with pytest.raises(ValueError):
        hip.set_cover(ptr, views, 3, 4)
    A, min_obs, prune, _ = hand_cases()["prune"]
    _check(hip, A, min_obs, prune)


def test_limits_are_value_errors(hip):
    ptr = np.zeros(2, dtype=np.int64)
    with pytest.raises(ValueError):
        hip.set_cover(ptr, np.zeros(0, dtype=np.int32), 1, _hip.GR_SETCOVER_MAX_VIEWS + 1)
    with pytest.raises(ValueError):
        hip.set_cover(ptr, np.zeros(0, dtype=np.int32), 1, 2, min_observations=float("nan"))
    with pytest.raises(ValueError):
        hip.set_cover(ptr, np.zeros(0, dtype=np.int32), 2, 2)   # face_ptr does not hold n_faces + 1 offsets


# -- behind the projection path -------------------------------------------------------------------------------------------------
def test_hand_off_from_the_projection_path(hip, tmp_path):
    from PIL import Image
    from scipy.sparse import load_npz

    from geograypher_amd.entrypoints import determine_minimum_overlapping_images
    from geograypher_amd.meshes import TexturedPhotogrammetryMeshIndexPredictions
    from geograypher_amd.utils import synthetic

    (points, faces), cams = synthetic.config1_scene()
    H, W = cams[0].get_image_size(1.0)
    for v, cam in enumerate(cams.cameras):
        cam.image_filename = tmp_path / f"view_{v:03d}.png"
        Image.fromarray(np.zeros((H, W), dtype=np.uint8)).save(cam.image_filename)
    mesh = TexturedPhotogrammetryMeshIndexPredictions((points, faces), log_level="ERROR", backend=hip)
    mask, record, summed = mesh.select_covering_cameras(cams)
    assert summed.shape == (faces.shape[0], len(cams)) and mask.shape == (len(cams),) and mask.dtype == np.bool_
    seen = np.diff(sparse.csr_matrix(summed).indptr) > 0
    assert seen.sum() > 5000
    assert standin.covers(summed, seen, mask) and standin.irreducible(summed, seen, mask)
    _assert_same(record, standin.set_cover(summed))
    assert np.array_equal(mask, record["selected"])

    np.savez(tmp_path / "mesh.npz", points=points, faces=faces)
    result = determine_minimum_overlapping_images(
        tmp_path / "mesh.npz", None, "EPSG:4978", compute_projection=True, compute_minimal_set=True,
        projections_filename=tmp_path / "out" / "projections.npz", selected_images_mask_filename=tmp_path / "out" / "mask.npy",
        camera_set=cams, backend=hip)
    saved = load_npz(tmp_path / "out" / "projections.npz")
    assert (saved != sparse.csr_matrix(summed)).nnz == 0
    assert np.array_equal(np.load(tmp_path / "out" / "mask.npy"), mask)
    assert np.array_equal(result["selected_images"], mask)
