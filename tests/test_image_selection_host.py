"""Image selection without a device: the stand-in of the rule-set on hand-worked cases and on the
properties every selection must have; `save_images`; the entrypoint's argument handling and its file-only stage; the input
checks of `select_covering_views`."""
import logging
import math

import numpy as np
import pytest
from scipy import sparse

from geograypher_amd.cameras.cameras import PhotogrammetryCamera, PhotogrammetryCameraSet
from geograypher_amd.entrypoints import annotation_image_selection as entry
from geograypher_amd.utils import numeric
from tests import setcover_standin as standin


def _from_sets(n_faces, sets):
    A = np.zeros((n_faces, len(sets)), dtype=bool)
    for v, faces in enumerate(sets):
        A[list(faces), v] = True
    return A


def _check(record, selected, order, gains, pruned, n_required):
    assert record["selected"].tolist() == selected
    assert record["order"].tolist() == order and record["order"].dtype == np.int32
    assert record["gains"].tolist() == gains and record["gains"].dtype == np.int64
    assert record["pruned"].tolist() == pruned and record["pruned"].dtype == np.int32
    assert record["n_required"] == record["n_covered"] == n_required


# the hand-worked instances, shared with tests/test_image_selection_gpu.py: name -> (A, min_observations, prune, expected record)
def hand_cases():
    prune = _from_sets(7, [{1, 2, 3, 4}, {1, 2, 5}, {3, 4, 6}])   # faces 1..6; face 0 is seen by nobody
    twins = _from_sets(4, [{0, 1}, {2, 3}, {2, 3}, {0, 1}])
    ties = np.eye(5, dtype=bool)
    # obs = 3, 2, 1, 2, 0: at a threshold of 2 faces 0, 1 and 3 are required
    thresh = _from_sets(5, [{0, 1}, {0, 3}, {0, 1, 2, 3}])
    return {
        "prune": (prune, 1, True, dict(selected=[False, True, True], order=[0, 1, 2], gains=[4, 1, 1], pruned=[0], n_required=6)),
        "prune_off": (prune, 1, False, dict(selected=[True, True, True], order=[0, 1, 2], gains=[4, 1, 1], pruned=[], n_required=6)),
        "identical_columns": (twins, 1, True, dict(selected=[True, True, False, False], order=[0, 1], gains=[2, 2], pruned=[],
                                                   n_required=4)),
        "all_tie": (ties, 1, True, dict(selected=[True] * 5, order=[0, 1, 2, 3, 4], gains=[1] * 5, pruned=[], n_required=5)),
        "min_observations_2": (thresh, 2, True, dict(selected=[False, False, True], order=[2], gains=[3], pruned=[], n_required=3)),
        "min_observations_1.5": (thresh, 1.5, True, dict(selected=[False, False, True], order=[2], gains=[3], pruned=[],
                                                         n_required=3)),
        "min_observations_1": (thresh, 1, True, dict(selected=[False, False, True], order=[2], gains=[4], pruned=[], n_required=4)),
        "threshold_above_all": (thresh, 4, True, dict(selected=[False] * 3, order=[], gains=[], pruned=[], n_required=0)),
        "unseen_faces": (_from_sets(6, [{1}, {4}]), 1, True, dict(selected=[True, True], order=[0, 1], gains=[1, 1], pruned=[],
                                                                 n_required=2)),
        "empty": (np.zeros((0, 0), dtype=bool), 1, True, dict(selected=[], order=[], gains=[], pruned=[], n_required=0)),
        "no_faces": (np.zeros((0, 3), dtype=bool), 1, True, dict(selected=[False] * 3, order=[], gains=[], pruned=[], n_required=0)),
        "no_views": (np.zeros((4, 0), dtype=bool), 1, True, dict(selected=[], order=[], gains=[], pruned=[], n_required=0)),
    }


# an instance that pins "decrement before the next test" (M6): greedy takes 0 (5 faces), then 1, 2, 3 (one face each, in index order).
# Examined 3, 2, 1, 0: view 3 = {4, 5} is needed for face 5; view 2 = {2, 3, 6}: needed for 6; view 1 = {0, 1, 7}: needed for 7;
# view 0 = {0, 1, 2, 3, 4} is redundant.  The second instance: view 0 is redundant only as long as view 1 is still selected.
def prune_chain_cases():
    first = _from_sets(8, [{0, 1, 2, 3, 4}, {0, 1, 7}, {2, 3, 6}, {4, 5}])
    # greedy: view 0 = {0..5} (6); then views 1, 2, 3 each see 2 new faces -> view 1 (6, 7); then 2 (face 8) and 3 (face 9).
    # Examined 3 (needed: face 9), 2 (needed: face 8), then 1: face 6 is seen by 2, face 7 by 3, faces 0, 1, 2 by 0 -> redundant,
    # removed, m drops to 1 on 0, 1, 2; then 0: kept for them.  With m left stale, faces 0, 1, 2 (views 0, 1) and 3, 4, 5 (views 0, 2)
    # would all read 2, view 0 would go too and faces 0, 1, 2 be uncovered.
    second = _from_sets(10, [{0, 1, 2, 3, 4, 5}, {6, 7, 0, 1, 2}, {6, 8, 3, 4, 5}, {7, 9}])
    return {
        "first_pick_redundant": (first, 1, True, dict(selected=[False, True, True, True], order=[0, 1, 2, 3], gains=[5, 1, 1, 1],
                                                     pruned=[0], n_required=8)),
        "removal_makes_next_needed": (second, 1, True, dict(selected=[True, False, True, True], order=[0, 1, 2, 3],
                                                           gains=[6, 2, 1, 1], pruned=[1], n_required=10)),
    }


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_standin_hand_worked(name):
    A, min_obs, prune, want = hand_cases()[name]
    _check(standin.set_cover(A, min_obs, prune), **want)


@pytest.mark.parametrize("name", sorted(prune_chain_cases()))
def test_standin_prune_chain(name):
    A, min_obs, prune, want = prune_chain_cases()[name]
    record = standin.set_cover(A, min_obs, prune)
    _check(record, **want)
    assert standin.covers(A, standin.required_faces(A, min_obs), record["selected"])


def test_standin_ignores_values_and_explicit_zeros():
    A = sparse.csr_matrix((np.array([5.0, 0.0, -2.0, 1.0]), np.array([0, 1, 1, 0]), np.array([0, 2, 3, 4])), shape=(3, 2))
    record = standin.set_cover(A)   # row 0 holds an explicit zero for view 1: view 1 sees face 1 only
    _check(record, selected=[True, True], order=[0, 1], gains=[2, 1], pruned=[], n_required=3)


def _random_small(seed):
    rng = np.random.default_rng(seed)
    F, N = int(rng.integers(1, 41)), int(rng.integers(1, 13))
    A = rng.random((F, N)) < rng.choice([0.08, 0.2, 0.5])
    return A, int(rng.integers(1, 4))


@pytest.mark.parametrize("block", range(8))
def test_standin_properties_on_200_random_instances(block):
    for seed in range(25 * block, 25 * (block + 1)):
        A, min_obs = _random_small(seed)
        required = standin.required_faces(A, min_obs)
        pruned = standin.set_cover(A, min_obs, prune=True)
        plain = standin.set_cover(A, min_obs, prune=False)
        for record in (pruned, plain):
            assert standin.covers(A, required, record["selected"]), seed
            assert record["n_required"] == record["n_covered"] == int(required.sum()), seed
            assert len(set(record["order"].tolist())) == len(record["order"]), seed
        assert standin.irreducible(A, required, pruned["selected"]), seed
        assert np.array_equal(np.flatnonzero(plain["selected"]), np.sort(plain["order"])), seed
        assert len(plain["pruned"]) == 0 and np.array_equal(plain["order"], pruned["order"]), seed
        assert np.array_equal(np.flatnonzero(pruned["selected"]), np.sort(np.setdiff1d(pruned["order"], pruned["pruned"]))), seed
        optimum = standin.brute_force_optimum(A, required)
        bound = standin.greedy_bound(optimum, A, required)
        for record in (pruned, plain):
            size = int(record["selected"].sum())
            assert optimum <= size <= bound, (seed, optimum, size, bound)


def test_standin_generators():
    A = standin.random_incidence(500, 40, 0.05, 1)
    assert A.shape == (500, 40) and 0.03 < A.nnz / (500 * 40) < 0.07
    B = standin.footprint_incidence(10_000, 50, 2)
    assert B.shape == (10_000, 50) and np.diff(B.indptr).mean() > 4
    assert np.array_equal(B.toarray(), standin.footprint_incidence(10_000, 50, 2).toarray())


# -- save_images ---------------------------------------------------------------------------------------------------------------
def _camera_set(folder, names):
    cams = [PhotogrammetryCamera(folder / name, np.eye(4), f=100.0, cx=0.0, cy=0.0, image_width=8, image_height=6,
                                 local_to_epsg_4978_transform=np.eye(4)) for name in names]
    return PhotogrammetryCameraSet(cams, image_folder=folder, local_to_epsg_4978_transform=np.eye(4))


def _images(tmp_path, names=("a/one.png", "a/two.png", "b/deep/three.png"), missing=()):
    folder = tmp_path / "images"
    for name in names:
        if name not in missing:
            (folder / name).parent.mkdir(parents=True, exist_ok=True)
            (folder / name).write_bytes(name.encode())
    return folder, _camera_set(folder, names)


def test_save_images_links_and_keeps_the_folder_structure(tmp_path):
    folder, cams = _images(tmp_path)
    out = tmp_path / "out"
    cams.save_images(out)
    for name in ("a/one.png", "a/two.png", "b/deep/three.png"):
        assert (out / name).is_symlink() and (out / name).resolve() == (folder / name).resolve()
        assert (out / name).read_bytes() == name.encode()


def test_save_images_copies_and_skips_a_missing_source(tmp_path, caplog):
    folder, cams = _images(tmp_path, missing=("a/two.png",))
    out = tmp_path / "out"
    with caplog.at_level(logging.WARNING):
        cams.save_images(out, copy=True)
    assert (out / "a/one.png").read_bytes() == b"a/one.png" and not (out / "a/one.png").is_symlink()
    assert (out / "b/deep/three.png").is_file() and not (out / "a/two.png").exists()
    assert any("Could not find" in r.getMessage() and "two.png" in r.getMessage() for r in caplog.records)


def test_save_images_remove_folder(tmp_path):
    _, cams = _images(tmp_path)
    out = tmp_path / "out"
    (out / "old").mkdir(parents=True)
    (out / "old" / "stale.txt").write_text("x")
    cams.save_images(out, copy=True, remove_folder=False)
    assert (out / "old" / "stale.txt").is_file() and (out / "a/one.png").is_file()
    cams.save_images(out, copy=True, remove_folder=True)
    assert not (out / "old").exists() and (out / "a/one.png").is_file()
    with pytest.raises(FileExistsError):   # links do not overwrite: the reference's os.symlink
        cams.save_images(out, remove_folder=False)


# -- the entrypoint --------------------------------------------------------------------------------------------------------------
def test_parse_args_accepts_the_reference_flags():
    args = entry.parse_args([
        "--mesh-file", "m.npz", "--cameras-file", "c.xml", "--mesh-CRS", "4978", "--image-folder", "imgs", "--ROI", "roi.geojson",
        "--ROI-buffer-meters", "12.5", "--compute-projection", "--compute-minimal-set", "--save-selected-images",
        "--projections-filename", "p.npz", "--selected-images-mask-filename", "s.npy", "--selected-images-save-folder", "sel",
        "--downsample-target", "1.0", "--min-observations-to-be-included", "2.5", "--vis"])
    assert args.compute_projection and args.compute_minimal_set and args.save_selected_images and args.vis
    assert args.ROI_buffer_meters == 12.5 and args.min_observations_to_be_included == 2.5 and args.downsample_target == 1.0
    assert (args.projections_filename, args.selected_images_mask_filename, args.selected_images_save_folder) == ("p.npz", "s.npy", "sel")
    minimal = entry.parse_args(["--mesh-file", "m.npz", "--cameras-file", "c.xml", "--mesh-CRS", "EPSG:4978", "--image-folder", "i"])
    assert not (minimal.compute_projection or minimal.compute_minimal_set or minimal.save_selected_images or minimal.vis)
    assert minimal.min_observations_to_be_included == 1 and minimal.ROI is None and minimal.ROI_points_file is None
    import inspect

    assert set(vars(minimal)) <= set(inspect.signature(entry.determine_minimum_overlapping_images).parameters)


@pytest.mark.parametrize("kwargs,match", [
    (dict(vis=True), "vis: visualisations need pyvista, which is outside the projection path"),
    (dict(downsample_target=0.5), "mesh decimation is outside the projection path"),
    (dict(ROI="roi.geojson"), r"ROI: the vertices in the ROI's CRS are needed \(ROI_points_file\)"),
])
def test_entrypoint_not_implemented(kwargs, match):
    with pytest.raises(NotImplementedError, match=match):
        entry.determine_minimum_overlapping_images("m.npz", "c.xml", "EPSG:4978", compute_projection=True, **kwargs)


def test_entrypoint_is_exported():
    from geograypher_amd import entrypoints

    assert entrypoints.determine_minimum_overlapping_images is entry.determine_minimum_overlapping_images


def test_save_selected_images_stage_alone(tmp_path):
    folder, cams = _images(tmp_path)
    np.save(tmp_path / "mask.npy", np.array([True, False, True]))
    result = entry.determine_minimum_overlapping_images(
        None, None, "EPSG:4978", image_folder=folder, save_selected_images=True,
        selected_images_mask_filename=tmp_path / "mask.npy", selected_images_save_folder=tmp_path / "chosen", camera_set=cams)
    chosen = sorted(str(p.relative_to(tmp_path / "chosen")) for p in (tmp_path / "chosen").rglob("*.png"))
    assert chosen == ["a/one.png", "b/deep/three.png"]
    assert len(result["subset_camera_set"]) == 2


# -- select_covering_views: what it refuses before a device is touched -----------------------------------------------------------
class _NoDevice:
    def set_cover(self, *args, **kwargs):
        raise AssertionError("the device must not be reached")


@pytest.mark.parametrize("visibility", [
    np.zeros(5, dtype=bool), np.zeros((2, 3, 4), dtype=bool), np.float64(1.0),
    sparse.coo_matrix((1, numeric.SET_COVER_MAX_VIEWS + 1)), sparse.coo_matrix((numeric.SET_COVER_MAX_FACES + 1, 2)),
], ids=["rank1", "rank3", "rank0", "too_many_views", "too_many_faces"])
def test_select_covering_views_refuses_bad_input(visibility):
    with pytest.raises(ValueError):
        numeric.select_covering_views(visibility, backend=_NoDevice())


def test_select_covering_views_canonicalises(tmp_path):
    """duplicates are summed, explicit zeros dropped, indices sorted, pointers int64 and indices int32 -- what the device is given"""
    seen = {}

    class Recorder:
        def set_cover(self, face_ptr, face_views, n_faces, n_views, min_observations=1, prune=True):
            seen.update(ptr=face_ptr, views=face_views, shape=(n_faces, n_views), min_obs=min_observations, prune=prune)
            return {"selected": np.zeros(n_views, dtype=bool)}

    coo = sparse.coo_matrix((np.array([1, 1, 0, 2, 1, -1]), (np.array([0, 0, 1, 2, 2, 2]), np.array([3, 3, 0, 2, 0, 1]))), shape=(4, 5))
    numeric.select_covering_views(coo, min_observations_to_be_included=1.5, prune=False, backend=Recorder())
    assert seen["ptr"].dtype == np.int64 and seen["views"].dtype == np.int32
    assert seen["ptr"].tolist() == [0, 1, 1, 4, 4] and seen["views"].tolist() == [3, 0, 1, 2]
    assert seen["shape"] == (4, 5) and seen["min_obs"] == 1.5 and seen["prune"] is False
    dense = np.array([[0, 2.0], [0, 0], [-1, 0]])
    numeric.select_covering_views(dense, backend=Recorder())
    assert seen["ptr"].tolist() == [0, 1, 1, 2] and seen["views"].tolist() == [1, 0] and seen["prune"] is True
    assert math.isclose(seen["min_obs"], 1.0)
