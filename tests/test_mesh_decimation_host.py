"""Mesh decimation by vertex clustering without a GPU: rules D1-D9 on a hand-worked scene with every fate
written out, the cell-size search on C1 against the table of the design, `decimate()` and the constructor against the stand-in, what
is refused, the three entry points end to end on the CPU stand-ins, and the C ABI of the two new calls.  The backend is
tests/decimate_standin.py (Python integers and loops)."""
import inspect
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import decimate_standin as ds  # noqa: E402
import region_standin as rs  # noqa: E402
import vector_standin as vs  # noqa: E402
from geograypher_amd import _hip, build  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import geometric, synthetic  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]

# target -> (cells, s, kept vertices, kept faces, collapsed, duplicates) on C1 (V = 5041, F = 9800, s_min = 49)
C1_TABLE = {0.5: (2520, 2_012_791, 2520, 4873, 4861, 66), 0.25: (1260, 2_873_361, 1260, 2426, 7268, 106),
            0.05: (252, 6_698_783, 245, 415, 9379, 6)}
C1_PROBES = 28


@pytest.fixture(scope="module")
def c1():
    """C1 with the stand-in's decimation at 0.25: computed once, shared, not modified."""
    (points, faces), cams = synthetic.config1_scene()
    verts_q = geometric.snap_points_3d(points)
    s = C1_TABLE[0.25][1]
    rep, face_ids, point_ids, new_faces, stats = ds.cluster_decimate_py(verts_q, faces, s)
    for a in (points, faces, verts_q, face_ids, point_ids, new_faces):
        a.setflags(write=False)
    return dict(points=points, faces=faces, cams=cams, verts_q=verts_q, s=s, face_ids=face_ids, point_ids=point_ids,
                dec_points=points[point_ids], dec_faces=new_faces.astype(np.int64), stats=stats)


def mesh_of(c1, backend=None, **kw):
    return TexturedPhotogrammetryMesh((c1["points"], c1["faces"]), log_level="ERROR", backend=backend or ds.StandInBackend(), **kw)


# -- D1-D8 ---------------------------------------------------------------------------------------------------------------------------
def test_hand_worked_scene_every_fate():
    verts_q, faces, s, vertex_fates, face_fates = ds.hand_scene()
    corner = {"A": (0, 0, 0), "B": (1, 0, 0), "C": (0, 1, 0), "D": (1, 1, 0)}
    rep, face_ids, point_ids, new_faces, stats = ds.StandInBackend().cluster_decimate(verts_q, faces, s, check=False)
    for i, (q, cell, want_rep, why) in enumerate(vertex_fates):
        assert ds.cell_of(q, s) == corner[cell], (i, why)
        assert rep[i] == want_rep, (i, why)
    kept = set(face_ids.tolist())
    for f, (corners, fate, why) in enumerate(face_fates):
        assert (f in kept) == (fate == "kept"), (f, why)
    fates = [fate for _, fate, _ in face_fates]
    assert rep.tolist() == ds.HAND_EXPECTED["rep"] and face_ids.tolist() == ds.HAND_EXPECTED["face_ids"]
    assert point_ids.tolist() == ds.HAND_EXPECTED["point_ids"] and new_faces.tolist() == ds.HAND_EXPECTED["new_faces"]
    assert stats.tolist() == ds.HAND_EXPECTED["stats"]
    assert stats.tolist()[:7] == [fates.count("kept"), 3, fates.count("bad"), 4, fates.count("collapsed"), fates.count("duplicate"), 0]
    # the kept face has ITS winding: the representatives of face 1 in face 1's order
    assert point_ids[new_faces[0]].tolist() == [rep[v] for v in faces[1]] == [6, 4, 0]
    assert 8 in rep and 8 not in point_ids                      # D's representative: no kept face uses it
    assert ds.cluster_count_py(verts_q, s) == 4 and ds.cluster_count_py(verts_q, 2 * s) == 1
    with pytest.raises(ValueError, match=r"gr_cluster_decimate: 1 faces name a vertex outside \[0, 10\)"):
        ds.StandInBackend().cluster_decimate(verts_q, faces, s)
    # a vertex outside the key range takes no cell, and a face that names it is bad
    far = np.array(verts_q)
    far[9] = [(1 << 21) * s, 0, 0]
    far[8] = [-1, 5, 5]
    out = ds.cluster_decimate_py(far, faces, s)
    assert out[0][8] == -1 and out[0][9] == -1 and out[4].tolist() == [1, 3, 2, 3, 2, 2, 2, 0]


def test_random_scene_holds_the_hard_cases():
    verts_q, faces = ds.random_scene()
    cases = ds.hard_cases(verts_q, faces, ds.RANDOM_S)
    print(f"[decimation] random scene: {cases}")
    assert verts_q.shape == (4000, 3) and faces.shape == (8000, 3) and verts_q.min() == 0
    assert np.array_equal(faces[:300], faces[300:600, ::-1])
    assert cases["boundary"] >= 1000 and cases["tie_cells"] >= 50 and cases["coincident"] >= 300
    assert cases["collapsed"] >= 1000 and cases["duplicates"] >= 1000 and cases["unused_representatives"] >= 1
    assert cases["unnamed_vertices"] >= 50 and cases["tie_cells_apart"] >= 10


# -- D1, D2, D4 ----------------------------------------------------------------------------------------------------------------------
def test_snap_and_cell_range():
    q = geometric.snap_points_3d(np.array([[10.0, -2.0, 5.0], [10.0000014, -1.0, 5.5], [12.5, -2.0, 5.0]]))
    assert q.dtype == np.int64 and q.tolist() == [[0, 0, 0], [1, 1_000_000, 500_000], [2_500_000, 0, 0]]
    assert geometric.cluster_cell_range(q) == (2, 2_500_001)          # ceil(2 500 001 / 2^21) = 2
    assert geometric.cluster_cell_range(np.zeros((3, 3), dtype=np.int64)) == (1, 1)
    assert geometric.cluster_cell_range(np.array([[(1 << 41) - 1, 0, 0]])) == (1 << 20, 1 << 30)
    with pytest.raises(ValueError, match="2\\^41"):
        geometric.snap_points_3d(np.array([[0.0, 0.0, 0.0], [(1 << 41) * 1e-6, 0.0, 0.0]]))
    with pytest.raises(ValueError, match=r"\(V, 3\)"):
        geometric.snap_points_3d(np.zeros((4, 2)))
    assert geometric.snap_points_3d(np.zeros((0, 3))).shape == (0, 3)


@pytest.mark.parametrize("target", sorted(C1_TABLE))
def test_cell_size_search_reproduces_the_table_on_C1(c1, target):
    cells, s, kept_points, kept_faces, collapsed, duplicates = C1_TABLE[target]
    backend = ds.StandInBackend()
    assert geometric.cluster_cell_range(c1["verts_q"])[0] == 49
    assert geometric.cluster_cell_size(backend, c1["verts_q"], target) == (s, cells, C1_PROBES) and backend.probes == C1_PROBES
    assert cells <= max(1, int(target * 5041))
    stats = ds.cluster_decimate_py(c1["verts_q"], c1["faces"], s)[4]
    assert stats.tolist() == [kept_faces, kept_points, 0, cells, collapsed, duplicates, 0, 0]
    assert kept_faces + collapsed + duplicates == 9800


def test_target_one_returns_the_mesh_unchanged_and_a_tiny_target_leaves_no_face(c1):
    mesh = mesh_of(c1)
    (points, faces), point_IDs, face_IDs = mesh.decimate(1.0, return_original_IDs=True)
    assert mesh.last_decimation_stats["cell_size_steps"] == 49 and mesh.last_decimation_stats["probes"] == 1
    assert np.array_equal(points, c1["points"]) and np.array_equal(faces, c1["faces"])
    assert np.array_equal(point_IDs, np.arange(5041)) and np.array_equal(face_IDs, np.arange(9800))
    with pytest.raises(ValueError, match="left no face"):
        mesh.decimate(1e-4)
    assert mesh.last_decimation_stats["faces_kept"] == 0 and mesh.last_decimation_stats["cells"] == 1


# -- decimate() and the constructor (D9) ---------------------------------------------------------------------------------------------
def test_decimate_equals_the_standin_and_keeps_input_rows(c1):
    mesh = mesh_of(c1)
    (points, faces), point_IDs, face_IDs = mesh.decimate(0.25, return_original_IDs=True)
    assert np.array_equal(point_IDs, c1["point_ids"]) and np.array_equal(face_IDs, c1["face_ids"])
    assert np.array_equal(points, c1["dec_points"]) and np.array_equal(faces, c1["dec_faces"]) and faces.dtype == np.int64
    assert point_IDs.dtype == np.int64 and face_IDs.dtype == np.int64 and np.all(np.diff(point_IDs) > 0) and np.all(np.diff(face_IDs) > 0)
    assert np.array_equal(points, c1["points"][point_IDs])            # rows of the input, bit for bit: no vertex was moved
    assert mesh.points.shape[0] == 5041 and mesh.faces.shape[0] == 9800   # the mesh itself is not changed
    st = mesh.last_decimation_stats
    assert (st["requested_vertex_fraction"], st["cell_size_steps"], st["probes"], st["cells"]) == (0.25, c1["s"], C1_PROBES, 1260)
    assert st["achieved_vertex_fraction"] == 1260 / 5041 and st["achieved_face_fraction"] == 2426 / 9800
    assert st["cell_size_meters"] == c1["s"] * 1e-6 and (st["faces_collapsed"], st["faces_duplicate"], st["bad_faces"]) == (7268, 106, 0)
    # the cell side itself: no search
    plain = mesh.decimate(cell_size_meters=c1["s"] * 1e-6)
    assert np.array_equal(plain[0], points) and np.array_equal(plain[1], faces) and mesh.last_decimation_stats["probes"] == 0
    assert mesh.last_decimation_stats["requested_vertex_fraction"] is None


def test_constructor_decimates_and_carries_textures_over(c1):
    V, F = 5041, 9800
    vertex_texture, face_texture = np.arange(V, dtype=np.float64) * 0.5, np.arange(F, dtype=np.float64) % 7
    mesh = mesh_of(c1, downsample_target=0.25, downsample_method="cluster", texture=vertex_texture)
    assert np.array_equal(mesh.decimated_point_IDs, c1["point_ids"]) and np.array_equal(mesh.decimated_face_IDs, c1["face_ids"])
    assert np.array_equal(mesh.points, c1["dec_points"]) and np.array_equal(mesh.faces, c1["dec_faces"])
    assert mesh.downsample_target == 0.25 and mesh.downsample_method == "cluster" and mesh.ROI_point_IDs is None
    assert np.array_equal(mesh.vertex_texture[:, 0], vertex_texture[c1["point_ids"]]) and mesh.face_texture is None
    mesh = mesh_of(c1, downsample_target=0.25, downsample_method="cluster", texture=face_texture)
    assert np.array_equal(mesh.face_texture[:, 0], face_texture[c1["face_ids"]]) and mesh.vertex_texture is None
    assert np.array_equal(mesh.original_point_IDs(), c1["point_ids"])
    # an array of a current count is taken as it is; any other count too (set_texture then refuses it)
    assert np.array_equal(mesh.to_current_mesh(np.arange(1260)), np.arange(1260)) and len(mesh.to_current_mesh(np.arange(7))) == 7
    two_columns = np.column_stack([face_texture, -face_texture])
    assert np.array_equal(mesh.to_current_mesh(two_columns), two_columns[c1["face_ids"]])
    plain = mesh_of(c1)
    assert plain.decimated_point_IDs is None and plain.original_point_IDs() is None and plain.to_current_mesh(face_texture) is face_texture


def test_constructor_composes_the_ROI_crop_with_the_decimation(c1):
    points, faces = c1["points"], c1["faces"]
    lo, hi = points[:, :2].min(axis=0), points[:, :2].max(axis=0)
    roi = [vs.square(*(lo + (hi - lo) * 0.2), *(lo + (hi - lo) * 0.7))]

    class Backend(ds.StandInBackend, rs.StandInBackend):
        pass

    face_texture = np.arange(len(faces), dtype=np.float64)
    mesh = mesh_of(c1, backend=Backend(), ROI=roi, ROI_buffer_meters=1.0, points_in_ROI_CRS=points, downsample_target=0.5,
                   downsample_method="cluster", texture=face_texture)
    cropped = mesh_of(c1, backend=Backend(), ROI=roi, ROI_buffer_meters=1.0, points_in_ROI_CRS=points)
    assert 0 < len(cropped.ROI_face_IDs) < len(faces) and np.array_equal(mesh.ROI_face_IDs, cropped.ROI_face_IDs)
    (want_points, want_faces), point_IDs, face_IDs = cropped.decimate(0.5, return_original_IDs=True)
    assert np.array_equal(mesh.decimated_point_IDs, point_IDs) and np.array_equal(mesh.decimated_face_IDs, face_IDs)   # index the CROPPED mesh
    assert np.array_equal(mesh.points, want_points) and np.array_equal(mesh.faces, want_faces)
    assert 0 < len(face_IDs) < len(cropped.ROI_face_IDs) and len(point_IDs) <= len(cropped.ROI_point_IDs) // 2
    assert np.array_equal(mesh.face_texture[:, 0], face_texture[cropped.ROI_face_IDs][face_IDs])
    assert np.array_equal(mesh.original_point_IDs(), cropped.ROI_point_IDs[point_IDs])
    assert np.array_equal(mesh.points, points[mesh.original_point_IDs()])
    by_cropped_count = np.arange(len(cropped.ROI_point_IDs)) * 2.0     # an array of the cropped count passes the crop and is gathered
    assert np.array_equal(mesh.to_current_mesh(by_cropped_count), by_cropped_count[point_IDs])


def test_the_ambiguity_of_equal_counts_is_a_ValueError():
    # 6 vertices and 6 faces before the decimation: an array of 6 rows fits both
    points = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [10.0, 0.0, 0.0], [0.0, 10.0, 0.0], [10.0, 10.0, 0.0], [10.0, 10.1, 0.0]])
    faces = np.array([[0, 2, 3], [1, 3, 2], [2, 4, 3], [2, 5, 3], [0, 1, 2], [4, 5, 3]])
    mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=ds.StandInBackend(), downsample_method="cluster",
                                      downsample_target=0.7)
    assert mesh.points.shape[0] == 4 and mesh.faces.shape[0] == 2 and mesh.decimated_face_IDs.tolist() == [0, 2]
    with pytest.raises(ValueError, match="Cannot infer whether the array belongs to vertices or faces"):
        mesh.to_current_mesh(np.arange(6))
    with pytest.raises(ValueError, match="Cannot infer whether the array belongs to vertices or faces"):
        TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=ds.StandInBackend(), downsample_method="cluster",
                                   downsample_target=0.7, texture=np.arange(6.0))


# -- what is refused -----------------------------------------------------------------------------------------------------------------
def test_refusals(c1):
    with pytest.raises(NotImplementedError, match=re.escape("mesh decimation is outside the projection path (meshes.py:215-226)")):
        mesh_of(c1, downsample_target=0.25)
    with pytest.raises(ValueError, match="downsample_method must be None or 'cluster', got 'quadric'"):
        mesh_of(c1, downsample_target=0.25, downsample_method="quadric")
    for bad in (0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"downsample_target must lie in \(0, 1\]"):
            mesh_of(c1, downsample_target=bad, downsample_method="cluster")
        with pytest.raises(ValueError, match=r"downsample_target must lie in \(0, 1\]"):
            mesh_of(c1).decimate(bad)
    mesh = mesh_of(c1)
    with pytest.raises(ValueError, match="exactly one of downsample_target and cell_size_meters"):
        mesh.decimate()
    with pytest.raises(ValueError, match="exactly one of downsample_target and cell_size_meters"):
        mesh.decimate(0.5, cell_size_meters=1.0)
    for bad in (48e-6, 0.0, -1.0, 100.841903):      # s_min = 49 steps, s_max = 100 841 902
        with pytest.raises(ValueError, match="cell_size_meters=.* is outside"):
            mesh.decimate(cell_size_meters=bad)
    assert len(mesh.decimate(cell_size_meters=49e-6)[1]) == 9800 and mesh.last_decimation_stats["cell_size_steps"] == 49


# -- the entry points ----------------------------------------------------------------------------------------------------------------
def _files(tmp_path, c1):
    from PIL import Image

    sub = c1["cams"][0:2]
    h, w = sub.cameras[0].get_image_size()
    rng = np.random.default_rng(1)
    for i, c in enumerate(sub.cameras):
        c.image_filename = Path(tmp_path, "images", "flight", f"img_{i}.png")
        for folder in ("images", "labels"):
            (tmp_path / folder / "flight").mkdir(parents=True, exist_ok=True)
        blocks = rng.integers(0, 4, (h // 16 + 1, w // 16 + 1)).astype(np.uint8)
        Image.fromarray(np.kron(blocks, np.ones((16, 16), dtype=np.uint8))[:h, :w]).save(tmp_path / "labels" / "flight" / f"img_{i}.png")
        Image.fromarray(np.zeros((h, w), dtype=np.uint8)).save(c.image_filename)
    sub.image_folder = Path(tmp_path, "images")
    np.savez(tmp_path / "mesh.npz", points=c1["points"], faces=c1["faces"])
    np.savez(tmp_path / "decimated.npz", points=c1["dec_points"], faces=c1["dec_faces"])
    return sub


def test_render_labels_with_cluster_equals_the_mesh_decimated_beforehand(tmp_path, oracle_backend_cls, c1):
    from PIL import Image

    from geograypher_amd.entrypoints.render_labels import parse_args, render_labels

    class Backend(ds.StandInBackend, oracle_backend_cls):
        pass

    sub = _files(tmp_path, c1)
    texture = (np.arange(9800) % 3).astype(np.float64)
    kw = dict(render_image_scale=0.25, apply_distortion=False, camera_set=sub)
    mesh = render_labels(tmp_path / "mesh.npz", None, tmp_path / "images", texture, tmp_path / "renders", "EPSG:4978", mesh_downsample=0.25,
                         mesh_downsample_method="cluster", backend=Backend(), **kw)
    assert np.array_equal(mesh.decimated_face_IDs, c1["face_ids"]) and np.array_equal(mesh.faces, c1["dec_faces"])
    assert np.array_equal(mesh.face_texture[:, 0], texture[c1["face_ids"]])
    render_labels(tmp_path / "decimated.npz", None, tmp_path / "images", texture[c1["face_ids"]], tmp_path / "want", "EPSG:4978",
                  backend=Backend(), **kw)
    seen = 0
    for i in range(2):
        got = np.asarray(Image.open(tmp_path / "renders" / "flight" / f"img_{i}.tif"))
        assert np.array_equal(got, np.asarray(Image.open(tmp_path / "want" / "flight" / f"img_{i}.tif")))
        seen += int((got != got.max()).sum())
    assert seen > 0
    with pytest.raises(NotImplementedError, match=re.escape("mesh_downsample: mesh decimation is outside the projection path (meshes.py:215-226)")):
        render_labels(tmp_path / "mesh.npz", None, tmp_path / "images", texture, tmp_path / "x", "EPSG:4978", mesh_downsample=0.25,
                      backend=Backend(), **kw)
    with pytest.raises(ValueError, match="downsample_method must be None or 'cluster'"):
        render_labels(tmp_path / "mesh.npz", None, tmp_path / "images", texture, tmp_path / "x", "EPSG:4978", mesh_downsample=0.25,
                      mesh_downsample_method="quadric", backend=Backend(), **kw)
    args = parse_args(["--mesh-file", "m.npz", "--mesh-CRS", "EPSG:4978", "--cameras-file", "c.xml", "--image-folder", "i", "--texture",
                       "t.npy", "--render-savefolder", "o", "--mesh-downsample", "0.25", "--mesh-downsample-method", "cluster"])
    assert args.mesh_downsample == 0.25 and args.mesh_downsample_method == "cluster"
    assert set(vars(args)) <= set(inspect.signature(render_labels).parameters)
    with pytest.raises(SystemExit):
        parse_args(["--mesh-file", "m.npz", "--mesh-CRS", "EPSG:4978", "--cameras-file", "c.xml", "--image-folder", "i", "--texture",
                    "t.npy", "--render-savefolder", "o", "--mesh-downsample-method", "quadric"])


def test_aggregate_images_with_cluster_equals_the_mesh_decimated_beforehand(tmp_path, oracle_backend_cls, c1):
    from geograypher_amd.entrypoints.aggregate_images import aggregate_images, parse_args

    class Backend(ds.StandInBackend, oracle_backend_cls):
        pass

    sub = _files(tmp_path, c1)
    ids = {0: "a", 1: "b", 2: "c", 3: "d"}
    (tmp_path / "ids.json").write_text(json.dumps(ids))
    kw = dict(take_every_nth_camera=1, aggregate_image_scale=0.25, camera_set=sub, IDs_to_labels=ids)
    mesh, values, classes = aggregate_images(tmp_path / "mesh.npz", None, tmp_path / "images", tmp_path / "labels", "EPSG:4978",
                                             mesh_downsample=0.25, mesh_downsample_method="cluster", backend=Backend(), **kw)
    assert np.array_equal(mesh.decimated_face_IDs, c1["face_ids"]) and np.array_equal(mesh.points, c1["dec_points"])
    _, want_values, want_classes = aggregate_images(tmp_path / "decimated.npz", None, tmp_path / "images", tmp_path / "labels", "EPSG:4978",
                                                    backend=Backend(), **kw)
    assert values.shape == (2426, 4) and np.array_equal(values, want_values, equal_nan=True)
    assert classes.shape == (2426, 1) and np.array_equal(classes, want_classes, equal_nan=True) and np.isfinite(classes).sum() > 100
    with pytest.raises(NotImplementedError, match=re.escape("mesh_downsample: mesh decimation is outside the projection path (meshes.py:215-226)")):
        aggregate_images(tmp_path / "mesh.npz", None, tmp_path / "images", tmp_path / "labels", "EPSG:4978", mesh_downsample=0.25,
                         backend=Backend(), **kw)
    args = parse_args(["--mesh-file", "m.npz", "--mesh-CRS", "EPSG:4978", "--cameras-file", "c.xml", "--image-folder", "i",
                       "--label-folder", "l", "--IDs-to-labels", "ids.json", "--mesh-downsample", "0.25", "--mesh-downsample-method",
                       "cluster"])
    assert args.mesh_downsample == 0.25 and args.mesh_downsample_method == "cluster"
    assert set(vars(args)) <= set(inspect.signature(aggregate_images).parameters)


def test_image_selection_with_cluster_equals_the_mesh_decimated_beforehand(tmp_path, oracle_backend_cls, c1):
    from geograypher_amd.entrypoints.annotation_image_selection import determine_minimum_overlapping_images, parse_args

    class Backend(ds.StandInBackend, oracle_backend_cls):
        pass

    sub = _files(tmp_path, c1)
    kw = dict(compute_projection=True, camera_set=sub)
    got = determine_minimum_overlapping_images(tmp_path / "mesh.npz", None, "EPSG:4978", projections_filename=tmp_path / "got.npz",
                                               downsample_target=0.25, downsample_method="cluster", backend=Backend(), **kw)
    want = determine_minimum_overlapping_images(tmp_path / "decimated.npz", None, "EPSG:4978", projections_filename=tmp_path / "want.npz",
                                                backend=Backend(), **kw)
    got, want = (m.toarray() if hasattr(m, "toarray") else np.asarray(m) for m in (got["summed_projections"], want["summed_projections"]))
    assert got.shape == (2426, 2) and np.array_equal(got, want) and (got > 0).any(axis=1).sum() > 100
    with pytest.raises(NotImplementedError, match=re.escape("downsample_target: mesh decimation is outside the projection path (meshes.py:215-226)")):
        determine_minimum_overlapping_images(tmp_path / "mesh.npz", None, "EPSG:4978", downsample_target=0.25, backend=Backend(), **kw)
    args = parse_args(["--mesh-file", "m.npz", "--cameras-file", "c.xml", "--mesh-CRS", "4978", "--image-folder", "i",
                       "--downsample-target", "0.25", "--downsample-method", "cluster"])
    assert args.downsample_target == 0.25 and args.downsample_method == "cluster"
    assert set(vars(args)) <= set(inspect.signature(determine_minimum_overlapping_images).parameters)


# -- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_source_name_the_new_calls():
    header = (ROOT / "include" / "geograster.h").read_text()
    companion = (ROOT / "include" / "geograster_decimate.h").read_text()
    source = (ROOT / "geograypher_amd" / "csrc" / "decimate.hip").read_text()
    internal = (ROOT / "geograypher_amd" / "csrc" / "gr_internal.hpp").read_text()
    kinds = {"int64_t": ctypes_kind("int64"), "int": ctypes_kind("int"), "int32_t": ctypes_kind("int")}
    for name, n_args in (("gr_cluster_count", 6), ("gr_cluster_decimate", 12)):
        decl = re.search(rf"\bint {name}\((.*?)\);", companion, re.S).group(1)
        arguments = [" ".join(a.split()) for a in decl.split(",")]
        assert len(arguments) == n_args == len(_hip._DECIMATE_SIGNATURES[name])
        for argument, ctype in zip(arguments, _hip._DECIMATE_SIGNATURES[name]):      # a pointer, a 64-bit integer or an int, as declared
            want = ctypes_kind("pointer") if "*" in argument else kinds[[w for w in re.findall(r"\w+", argument) if w != "const"][0]]
            assert ctype in want, (name, argument)
        assert name in _hip.DECIMATE_SYMBOLS and re.search(rf"\bint {name}\(gr_ctx \*c,", source)
        definition = re.search(rf"\bint {name}\((gr_ctx \*c,.*?)\) \{{", source, re.S).group(1)
        assert len(definition.split(",")) == n_args
        assert f'"{name}' in source                                               # the call's name in its messages
    kernels = ("k_decim_keys", "k_decim_heads", "k_decim_scatter_rep", "k_decim_faces", "k_decim_face_flags", "k_submesh_write")
    assert all(k in source and k in internal for k in kernels)
    assert '#include "geograster_decimate.h"' in header and "#define GR_VERSION 126" in header
    assert "meshes/meshes.py:215-226" in companion and "without a GR_VERSION bump" in companion
    assert (_hip.GR_DECIM_STAT_KEPT_FACES, _hip.GR_DECIM_STAT_KEPT_VERTICES, _hip.GR_DECIM_STAT_BAD_FACES, _hip.GR_DECIM_STAT_CELLS,
            _hip.GR_DECIM_STAT_COLLAPSED, _hip.GR_DECIM_STAT_DUPLICATES, _hip.GR_DECIM_STAT_OUTSIDE, _hip.GR_DECIM_STAT_WORDS) == (0, 1, 2, 3, 4, 5, 6, 8)
    steps = (ROOT / "geograypher_amd" / "csrc" / "cub_steps.hpp").read_text()      # the sorts and scans: steps of cub_steps.hpp
    assert "SortPairs<u64, int32_t> sort_d2(c, p, V, dbits), sort_key(c, p, V, 64);" in source and "compact_write(" in source and "stage_acquire" in source
    assert "hipcub::DeviceRadixSort::SortPairs(" in steps and "hipcub::DeviceScan::ExclusiveSum(" in steps
    assert "asm" not in re.sub(r"//[^\n]*", "", source)
    assert any(p.name == "decimate.hip" for p in build.SOURCES) and any(p.name == "compact_dev.hpp" for p in build.HEADERS)
    assert callable(_hip.HipRaster.cluster_count) and callable(_hip.HipRaster.cluster_decimate)
    # the write kernel is shared with the sub-mesh extraction, not copied
    polygons = (ROOT / "geograypher_amd" / "csrc" / "polygons.hip").read_text()
    shared = (ROOT / "geograypher_amd" / "csrc" / "compact_dev.hpp").read_text()
    assert "void k_submesh_write(" in shared and "void k_submesh_write(" not in polygons + source
    assert '#include "compact_dev.hpp"' in polygons and '#include "compact_dev.hpp"' in source


def ctypes_kind(kind):
    import ctypes

    return {"pointer": (ctypes.c_void_p,), "int64": (ctypes.c_int64,), "int": (ctypes.c_int, ctypes.c_int32)}[kind]


def test_library_exports_the_new_calls():
    import ctypes

    lib = ctypes.CDLL(str(_hip.library_path()))
    assert all(hasattr(lib, name) for name in _hip.DECIMATE_SYMBOLS)
    lib.gr_version.restype = ctypes.c_int
    assert lib.gr_version() == 126
