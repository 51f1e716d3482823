"""gr_points_in_region / gr_submesh_extract on the device against the stand-in of tests/region_standin.py (Fractions, Python integers
and loops): every comparison is exact equality on EVERY point and face, the statistics words included.

The point kernel stages nothing in chunks (one point per lane, the ring table read wave-uniformly), so the sizes that matter are the
64 lanes of a wave and the 256 threads of a workgroup; the sub-mesh adds two device-wide scans."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import region_standin as rs  # noqa: E402
import vector_standin as vs  # noqa: E402
from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import geometric, synthetic  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)


def device_region(hip, points_q, table, D):
    mask, stats = hip.points_in_region(points_q, *table, D)
    return mask.cpu().numpy(), stats.cpu().numpy()


def device_submesh(hip, mask, faces, **kw):
    face_ids, point_ids, new_faces, counts = hip.submesh_extract(mask, faces, **kw)
    return face_ids.cpu().numpy(), point_ids.cpu().numpy(), new_faces.cpu().numpy(), counts.cpu().numpy()


def same_submesh(got, mask, faces):
    face_ids, point_ids, new_faces, bad = rs.submesh_np(mask, faces)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int64 and got[2].dtype == np.int32
    assert np.array_equal(got[0], face_ids) and np.array_equal(got[1], point_ids) and np.array_equal(got[2], new_faces)
    assert got[2].shape == (len(face_ids), 3) and got[3].tolist() == [len(face_ids), len(point_ids), bad]


@pytest.fixture(scope="module")
def scene():
    """The random scene with the stand-in's answer: computed once, shared, not modified."""
    points_q, faces, table = rs.random_scene()
    mask, info = rs.points_in_region_np(points_q, table, rs.RANDOM_D)
    for a in (points_q, faces, mask):
        a.setflags(write=False)
    return points_q, faces, table, mask, info


def test_hand_worked_scene(hip):
    polygons, cases = rs.hand_scene()
    points = np.array([c for c, _, _, _ in cases])
    standin = rs.StandInBackend()
    for D_meters, column in ((rs.HAND_D, 1), (0, 2)):
        mask, stats = geometric.points_in_region(hip, polygons, points, D_meters)
        mask, stats = mask.cpu().numpy(), stats.cpu().numpy()
        for case, got in zip(cases, mask):
            assert bool(got) == case[column], (case[0], case[3], D_meters)
        want, want_stats = geometric.points_in_region(standin, polygons, points, D_meters)
        assert mask.dtype == bool and np.array_equal(mask, want) and np.array_equal(stats, want_stats)
    # outside the joint box by exactly D, and by one grid step more
    by_name = {what: (point, inside) for point, inside, _, what in cases}
    assert by_name["outside the joint box by exactly 2.5 m"][1] and not by_name["outside the joint box by one grid step more than 2.5 m"][1]


def test_random_scene_has_the_hard_cases_and_matches_on_every_point_and_face(hip, scene):
    points_q, faces, table, want, info = scene
    counts = {k: int(info[k].sum()) for k in rs.CASES}
    print(f"[roi_crop] random scene: {len(points_q)} points, {len(faces)} faces, {len(table[4])} rows, {counts}, inside {int(want.sum())}, "
          f"stats {info['stats'].tolist()}")
    assert len(points_q) == 4000 and len(faces) == 8000 and len(table[4]) == 40 and table[3].sum() >= 5
    for k in ("on_ring", "two_rows", "in_hole_outside", "in_hole_within_D", "at_D_edge", "one_step_beyond"):
        assert counts[k] >= 50, k
    assert counts["at_D_vertex"] >= 20
    got, stats = device_region(hip, points_q, table, rs.RANDOM_D)
    assert np.array_equal(got, want)
    assert np.array_equal(stats, info["stats"])
    sub = device_submesh(hip, got, faces)
    same_submesh(sub, want, faces)
    assert 0 < len(sub[0]) < len(faces) and 0 < len(sub[1]) < int(np.isin(np.arange(len(points_q)), faces).sum()) + 1
    assert (want & ~np.isin(np.arange(len(points_q)), faces)).any()    # a point of the region that no face uses


@pytest.mark.parametrize("n", SIZES)
def test_point_counts_around_a_wave_and_a_workgroup(hip, scene, n):
    points_q, _, table, want, info = scene
    # the LAST points of the scene: the shifted copies, where the decisions are closest
    got, stats = device_region(hip, points_q[-n:], table, rs.RANDOM_D)
    assert np.array_equal(got, want[-n:])
    near_only = info["near"][-n:] & ~info["contained"][-n:]
    assert stats.tolist() == [int(want[-n:].sum()), int(near_only.sum()), int(info["wide"][-n:].sum()), 0]


def test_vertex_and_face_counts_around_a_wave_and_a_workgroup(hip, scene):
    _, _, _, want, _ = scene
    rng = np.random.default_rng(11)
    for V in SIZES:
        mask = want[1000:1000 + V] if V > 1 else np.array([True])
        for F in SIZES:
            faces = rng.integers(0, V, (F, 3)).astype(np.int32)
            same_submesh(device_submesh(hip, mask, faces), mask, faces)
    same_submesh(device_submesh(hip, np.zeros(65, dtype=bool), np.zeros((0, 3), dtype=np.int32)), np.zeros(65, dtype=bool), np.zeros((0, 3)))
    none = device_submesh(hip, np.zeros(257, dtype=bool), rng.integers(0, 257, (65, 3)))
    assert none[0].shape == (0,) and none[1].shape == (0,) and none[2].shape == (0, 3) and none[3].tolist() == [0, 0, 0]
    everything = rng.permutation(np.arange(300 * 3) % 257).reshape(-1, 3).astype(np.int32)
    all_kept = device_submesh(hip, np.ones(257, dtype=bool), everything)
    assert np.array_equal(all_kept[0], np.arange(300)) and np.array_equal(all_kept[1], np.arange(257)) and np.array_equal(all_kept[2], everything)


def test_no_buffer_empty_ROI_and_rings_the_snap_dropped(hip, scene):
    points_q, _, table, _, _ = scene
    want0, info0 = rs.points_in_region_np(points_q[-1500:], table, 0)
    got0, stats0 = device_region(hip, points_q[-1500:], table, 0)
    assert np.array_equal(got0, want0) and np.array_equal(stats0, info0["stats"]) and stats0[1] == 0 and stats0[2] == 0 and want0.any()
    # an ROI without rings keeps nothing
    empty = PlanarPolygons([], [], [], n_polygons=3).snapped()
    got, stats = device_region(hip, points_q[:257], empty, rs.RANDOM_D)
    assert not got.any() and stats.tolist() == [0, 0, 0, 0]
    none = PlanarPolygons([], [], [], n_polygons=0).snapped()
    assert not device_region(hip, points_q[:65], none, 0)[0].any()
    # row 0's ring collapses on the grid and is dropped (an empty box); row 1 has no ring at all; row 2 is a square
    polygons = PlanarPolygons([np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 2e-7]]), vs.square(10, 10, 12, 12)], [0, 2], [False, False], n_polygons=3)
    pts = np.array([[0.5, 0.0], [0.5, 1e-6], [11.0, 11.0], [11.0, 13.0], [11.0, 13.0 + 2e-6], [0.0, 0.0]])
    for D_meters in (0, 1.0):
        vq, tab = geometric.snap_with_polygons(pts, polygons)
        assert len(tab[2]) == 1 and tab[4][0].tolist() == [1, 1, 0, 0]
        D = geometric.region_buffer_steps(D_meters)
        want, info = rs.points_in_region_np(vq, tab, D)
        got, stats = device_region(hip, vq, tab, D)
        assert np.array_equal(got, want) and np.array_equal(stats, info["stats"])
        assert want.tolist() == [False, False, True, D > 0, False, False]


def test_the_last_vertex_and_the_last_face(hip):
    polygons = PlanarPolygons([vs.square(0, 0, 1, 1)], [0], [False])
    for n in (257, 300):
        pts = np.column_stack([np.full(n, 50.0), np.arange(n, dtype=np.float64)])
        pts[-1] = [0.5, 0.5]
        mask, stats = geometric.points_in_region(hip, polygons, pts, 0.25)
        mask = mask.cpu().numpy()
        assert mask.tolist() == [False] * (n - 1) + [True] and stats.cpu().numpy().tolist() == [1, 0, 0, 0]
        faces = np.stack([np.arange(n), (np.arange(n) + 1) % (n - 1), (np.arange(n) + 2) % (n - 1)], axis=1).astype(np.int32)
        faces[-1] = [3, n - 1, 7]
        got = device_submesh(hip, mask, faces)
        assert got[0].tolist() == [n - 1] and got[1].tolist() == [3, 7, n - 1] and got[2].tolist() == [[0, 2, 1]]
        same_submesh(got, mask, faces)


def test_a_bad_face_index_is_a_ValueError(hip, scene):
    _, faces, _, want, _ = scene
    broken = np.array(faces)
    broken[[5, 4000, 7999], [0, 1, 2]] = [-1, len(want), 2 ** 31 - 1]
    with pytest.raises(ValueError, match=r"gr_submesh_extract: 3 faces name a vertex outside \[0, 4000\)"):
        hip.submesh_extract(want, broken)
    got = device_submesh(hip, want, broken, check=False)    # the faces read nothing and are not kept
    same_submesh(got, want, broken)
    assert got[3][2] == 3 and not np.isin([5, 4000, 7999], got[0]).any()
    with pytest.raises(ValueError, match="buffer D="):
        hip.points_in_region(np.zeros((1, 2), dtype=np.int64), *scene[2], 2 ** 40)
    with pytest.raises(ValueError, match="buffer D="):
        hip.points_in_region(np.zeros((1, 2), dtype=np.int64), *scene[2], -1)


def test_the_wide_product_trap(hip):
    table, D, points_q, edge = rs.wide_trap()
    assert np.abs(table[0]).max() == 2 ** 40 and abs(edge[2] - edge[0]) == 2 ** 41 and np.abs(points_q).max() <= 2 ** 40
    assert (points_q[1] - points_q[0]).tolist() == [1, 0]
    want, info = rs.points_in_region_np(points_q, table, D)
    assert want.tolist() == [False, True] and info["wide"].tolist() == [1, 1]
    exact = want.tolist()
    cut = [rs.truncated_128_decision(int(x), int(y), *edge, D) for x, y in points_q]
    floats = [rs.float64_decision(int(x), int(y), *edge, D) for x, y in points_q]
    assert cut != exact and cut[1] is False          # cut to 128 bits the inner point falls out
    assert floats != exact and floats[0] is True     # in float64 the outer point falls in
    got, stats = device_region(hip, points_q, table, D)
    assert got.tolist() == exact and np.array_equal(stats, info["stats"])


def test_chain_crop_then_pix2face_equals_the_full_mesh_through_face_IDs(hip):
    (points, faces), cams = synthetic.config1_scene()
    lo, hi = points[:, :2].min(axis=0), points[:, :2].max(axis=0)
    roi = [vs.square(*(lo + (hi - lo) * 0.2), *(lo + (hi - lo) * 0.6))]
    full = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=hip)
    (sub_points, sub_faces), point_IDs, face_IDs = full.select_mesh_ROI(roi, buffer_meters=0.02 * float((hi - lo).max()),
                                                                        return_original_IDs=True, points_in_ROI_CRS=points)
    assert 0 < len(face_IDs) < len(faces) and np.array_equal(sub_points[sub_faces], points[faces[face_IDs]])
    same_submesh((face_IDs, point_IDs, sub_faces.astype(np.int32), np.array([len(face_IDs), len(point_IDs), 0])),
                 geometric.points_in_region(rs.StandInBackend(), roi, points, 0.02 * float((hi - lo).max()))[0], faces)
    view = cams[0:1]
    want = full.pix2face(view, render_img_scale=0.5, apply_distortion=False, near=0.05)[0]
    cropped = TexturedPhotogrammetryMesh((sub_points, sub_faces), log_level="ERROR", backend=hip)
    got = cropped.pix2face(view, render_img_scale=0.5, apply_distortion=False, near=0.05)[0]
    new_id = np.full(len(faces) + 1, -2, dtype=np.int64)    # the last entry takes the background's -1
    new_id[face_IDs] = np.arange(len(face_IDs))
    kept = new_id[want] >= 0
    assert kept.sum() > 1000 and (~kept).sum() > 1000
    assert np.array_equal(got[kept], new_id[want][kept])
    full.pix2face(view, render_img_scale=0.5, apply_distortion=False, near=0.05)   # the full mesh is uploaded again for later users
