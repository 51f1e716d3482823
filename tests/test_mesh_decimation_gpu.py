"""gr_cluster_count / gr_cluster_decimate on the device against the stand-in of tests/decimate_standin.py (Python integers and loops):
every comparison is exact equality on EVERY vertex and face, the statistics words included.

The kernels work one vertex or face per lane between device-wide radix sorts and scans, so the sizes that matter are the 64 lanes of a
wave, the 256 threads of a workgroup and more than one workgroup; the cell sides that matter are the smallest (every vertex a cell of
its own unless it coincides with another), one that puts lattice planes on cell faces, and the largest (one cell)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import decimate_standin as ds  # noqa: E402
from geograypher_amd import _hip  # noqa: E402
from geograypher_amd.cameras import SegmentorPhotogrammetryCameraSet  # noqa: E402
from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.predictors import ArrayLabelSegmentor  # noqa: E402
from geograypher_amd.utils import geometric, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

C1_SEARCH = {0.5: (2_012_791, 2520, 28), 0.25: (2_873_361, 1260, 28), 0.05: (6_698_783, 252, 28)}


def device_decimate(hip, verts_q, faces, s, **kw):
    return tuple(a.cpu().numpy() for a in hip.cluster_decimate(verts_q, faces, s, **kw))


def same_decimation(got, verts_q, faces, s):
    rep, face_ids, point_ids, new_faces, stats = ds.cluster_decimate_py(verts_q, faces, s)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64 and got[2].dtype == np.int64 and got[3].dtype == np.int32
    assert np.array_equal(got[0], rep), "rep"
    assert np.array_equal(got[1], face_ids) and np.array_equal(got[2], point_ids), "ids"
    assert got[3].shape == (len(face_ids), 3) and np.array_equal(got[3], new_faces), "new_faces"
    assert got[4].tolist() == stats.tolist(), "stats"
    return stats


@pytest.fixture(scope="module")
def scene():
    """The random scene: computed once, shared, not modified."""
    verts_q, faces = ds.random_scene()
    for a in (verts_q, faces):
        a.setflags(write=False)
    return verts_q, faces


def test_hand_worked_scene(hip):
    verts_q, faces, s, _, _ = ds.hand_scene()
    with pytest.raises(ValueError, match=r"gr_cluster_decimate: 1 faces name a vertex outside \[0, 10\)"):
        hip.cluster_decimate(verts_q, faces, s)
    got = device_decimate(hip, verts_q, faces, s, check=False)
    want = ds.HAND_EXPECTED
    assert got[0].tolist() == want["rep"] and got[1].tolist() == want["face_ids"] and got[2].tolist() == want["point_ids"]
    assert got[3].tolist() == want["new_faces"] and got[4].tolist() == want["stats"]
    same_decimation(got, verts_q, faces, s)
    assert hip.cluster_count(verts_q, s) == 4 and hip.cluster_count(verts_q, 2 * s) == 1


@pytest.mark.parametrize("s", [ds.RANDOM_S, 1, 250_000, 2 ** 30])
def test_random_scene_matches_on_every_vertex_and_face(hip, scene, s):
    verts_q, faces = scene
    # (check=False: at s = 1 most of the scene lies beyond cell 2^21 - 1, outside the key range, and the faces there count as bad)
    stats = same_decimation(device_decimate(hip, verts_q, faces, s, check=False), verts_q, faces, s)
    print(f"[decimation] random scene, s = {s}: stats {stats.tolist()}")
    assert (stats[_hip.GR_DECIM_STAT_OUTSIDE] > 0) == (s == 1) and (stats[_hip.GR_DECIM_STAT_BAD_FACES] > 0) == (s == 1)
    if s == ds.RANDOM_S:
        assert stats[_hip.GR_DECIM_STAT_COLLAPSED] >= 1000 and stats[_hip.GR_DECIM_STAT_DUPLICATES] >= 1000
        assert stats[_hip.GR_DECIM_STAT_CELLS] > stats[_hip.GR_DECIM_STAT_KEPT_VERTICES] > 0     # representatives no kept face uses
    if s == 2 ** 30:
        assert stats.tolist() == [0, 0, 0, 1, 8000, 0, 0, 0]                                       # one cell: every face collapses


def test_cluster_count_matches_for_eight_cell_sides(hip, scene):
    verts_q, _ = scene
    on_device = hip.to_device(verts_q, "int64")
    for s in (1, 3, 250_000, 999_999, ds.RANDOM_S, 1_000_001, 6_000_000, 2 ** 30):
        assert hip.cluster_count(on_device, s) == ds.cluster_count_py(verts_q, s), s


def test_vertex_and_face_counts_around_a_wave_and_a_workgroup(hip, scene):
    verts_q, faces = scene
    rng = np.random.default_rng(5)
    for V in (1, 63, 64, 65, 257):
        for F in (0, 1, 63, 64, 65, 257, 1025):
            prefix = np.array(faces[:F])
            beyond = prefix >= V
            prefix[beyond] = rng.integers(0, V, int(beyond.sum()))          # re-drawn inside the prefix
            same_decimation(device_decimate(hip, verts_q[:V], prefix, ds.RANDOM_S), verts_q[:V], prefix, ds.RANDOM_S)


def test_no_vertices_and_no_faces(hip, scene):
    verts_q, faces = scene
    none = device_decimate(hip, np.zeros((0, 3), dtype=np.int64), np.zeros((0, 3), dtype=np.int32), 7)
    assert [a.shape for a in none[:4]] == [(0,), (0,), (0,), (0, 3)] and none[4].tolist() == [0] * 8
    only_vertices = device_decimate(hip, verts_q[:300], np.zeros((0, 3), dtype=np.int32), ds.RANDOM_S)
    same_decimation(only_vertices, verts_q[:300], np.zeros((0, 3), dtype=np.int32), ds.RANDOM_S)
    assert only_vertices[4][_hip.GR_DECIM_STAT_CELLS] > 0 and only_vertices[4][_hip.GR_DECIM_STAT_KEPT_VERTICES] == 0
    only_faces = device_decimate(hip, np.zeros((0, 3), dtype=np.int64), faces[:65], 7, check=False)    # every face names a missing vertex
    assert only_faces[1].shape == (0,) and only_faces[4].tolist() == [0, 0, 65, 0, 0, 0, 0, 0]
    assert hip.cluster_count(np.zeros((0, 3), dtype=np.int64), 7) == 0


def test_a_bad_face_index_and_a_vertex_outside_the_key_range(hip, scene):
    verts_q, faces = scene
    broken = np.array(faces)
    broken[[5, 4000, 7999], [0, 1, 2]] = [-1, len(verts_q), 2 ** 31 - 1]
    with pytest.raises(ValueError, match=r"gr_cluster_decimate: 3 faces name a vertex outside \[0, 4000\)"):
        hip.cluster_decimate(verts_q, broken, ds.RANDOM_S)
    got = device_decimate(hip, verts_q, broken, ds.RANDOM_S, check=False)     # the faces read nothing and are not kept
    same_decimation(got, verts_q, broken, ds.RANDOM_S)
    assert got[4][_hip.GR_DECIM_STAT_BAD_FACES] == 3 and not np.isin([5, 4000, 7999], got[1]).any()
    outside = np.array(verts_q)
    outside[[0, 70, 3999]] = [[-1, 0, 0], [0, (1 << 21) * 3, 0], [5, 5, (1 << 62)]]      # q < 0, and a cell component >= 2^21 at s = 3
    got = device_decimate(hip, outside, faces, 3, check=False)
    stats = same_decimation(got, outside, faces, 3)
    beyond = ((outside < 0) | (outside // 3 >= 1 << 21)).any(axis=1)       # the three, and the scene's own highest vertices at s = 3
    assert stats[_hip.GR_DECIM_STAT_OUTSIDE] == beyond.sum() >= 3 and np.array_equal(got[0] == -1, beyond)
    assert got[0][[0, 70, 3999]].tolist() == [-1, -1, -1]
    assert hip.cluster_count(outside, 3) == ds.cluster_count_py(outside, 3)


@pytest.mark.parametrize("target", sorted(C1_SEARCH))
def test_cell_size_search_on_C1_through_the_device(hip, target):
    (points, _), _ = synthetic.config1_scene()
    assert geometric.cluster_cell_size(hip, geometric.snap_points_3d(points), target) == C1_SEARCH[target]


def test_c1_end_to_end_equals_the_oracle_on_the_standins_mesh(hip, oracle_backend_cls):
    from oracle import oracle_c

    (points, faces), cams = synthetic.config1_scene()
    mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=hip, downsample_target=0.25, downsample_method="cluster")
    _, face_ids, point_ids, new_faces, _ = ds.cluster_decimate_py(geometric.snap_points_3d(points), faces, C1_SEARCH[0.25][0])
    assert np.array_equal(mesh.decimated_point_IDs, point_ids) and np.array_equal(mesh.decimated_face_IDs, face_ids)
    assert np.array_equal(mesh.points, points[point_ids]) and np.array_equal(mesh.faces, new_faces)
    assert mesh.last_decimation_stats["probes"] == 28 and mesh.last_decimation_stats["faces_kept"] == 2426
    want_mesh = TexturedPhotogrammetryMesh((points[point_ids], new_faces.astype(np.int64)), log_level="ERROR", backend=oracle_backend_cls())
    views = cams[0:2]
    got = mesh.pix2face(views, render_img_scale=0.5, apply_distortion=False, near=0.05)
    want = want_mesh.pix2face(views, render_img_scale=0.5, apply_distortion=False, near=0.05)
    assert np.array_equal(np.asarray(got), np.asarray(want)) and (np.asarray(got) >= 0).sum() > 10000
    C = 4
    h, w = views[0].get_image_size(1.0)
    recs = views.get_raster_records(1.0, near=0.05)
    labels = [synthetic.synthetic_labels(oracle_c.raster(points[point_ids], new_faces, recs[v], h, w), v, C) for v in range(2)]
    seg = SegmentorPhotogrammetryCameraSet(views, ArrayLabelSegmentor(labels, C, filenames=[c.image_filename for c in views.cameras]))
    got_avg, got_info = mesh.aggregate_projected_images(seg, aggregate_img_scale=0.5)
    want_avg, want_info = want_mesh.aggregate_projected_images(seg, aggregate_img_scale=0.5)
    assert np.array_equal(got_avg, want_avg, equal_nan=True) and got_avg.shape == (2426, C)
    assert np.array_equal(got_info["summed_projections"], want_info["summed_projections"], equal_nan=True)
    assert np.array_equal(got_info["projection_counts"], want_info["projection_counts"]) and want_info["projection_counts"].sum() > 0
    full = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=hip)
    full.pix2face(cams[0:1], render_img_scale=0.5, apply_distortion=False, near=0.05)   # the full mesh is uploaded again for later users


def test_shapes_are_checked_before_the_library_is_called(hip):
    with pytest.raises(ValueError, match=r"vertices must be \(V, 3\), got \(4, 2\)"):
        hip.cluster_count(np.zeros((4, 2), dtype=np.int64), 5)
    with pytest.raises(ValueError, match=r"vertices must be \(V, 3\), got \(12,\)"):
        hip.cluster_decimate(np.zeros(12, dtype=np.int64), np.zeros((2, 3), dtype=np.int32), 5)
    with pytest.raises(ValueError, match=r"faces must be \(F, 3\), got \(2, 4\)"):
        hip.cluster_decimate(np.zeros((4, 3), dtype=np.int64), np.zeros((2, 4), dtype=np.int32), 5)


@pytest.mark.parametrize("name,call", [
    ("gr_cluster_count", lambda b, vq, f: b.cluster_count(vq, 0)),
    ("gr_cluster_count", lambda b, vq, f: b.cluster_count(vq, 2 ** 30 + 1)),
    ("gr_cluster_decimate", lambda b, vq, f: b.cluster_decimate(vq, f, 0)),
    ("gr_cluster_decimate", lambda b, vq, f: b.cluster_decimate(vq, f, 2 ** 30 + 1)),
    ("gr_cluster_count", lambda b, vq, f: b._call("gr_cluster_count", 0, 4, 5, b._stats(1).data_ptr(), b._stream())),
    ("gr_cluster_decimate", lambda b, vq, f: b._call("gr_cluster_decimate", b.to_device(vq, "int64").data_ptr(), 4, 0, 2, 5,
                                                      b._stats(4).data_ptr(), 0, b._stats(4).data_ptr(), 0, b._stats(8).data_ptr(),
                                                      b._stream())),
], ids=["count-s0", "count-s_above", "decimate-s0", "decimate-s_above", "count-null", "decimate-null"])
def test_bad_arguments_are_GR_EINVAL_naming_the_call(hip, name, call):
    verts_q = np.arange(12, dtype=np.int64).reshape(4, 3)
    faces = np.array([[0, 1, 2], [1, 2, 3]], dtype=np.int32)
    with pytest.raises(ValueError, match=rf"{name}: {name}: (cell side s=|null arrays)"):
        call(hip, verts_q, faces)
    assert hip.cluster_count(verts_q, 1) == 4        # the context is usable afterwards
