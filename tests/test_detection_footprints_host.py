"""Detection footprints without a GPU: the exact stand-in of tests/member_outline_standin.py against rule Y5
(the per-column results of the class-outline stand-in, concatenated) and against X7 per class by brute force, the sparse input of
`face_label_outlines` and `export_face_labels_vector`, `project_detections` end to end on the CPU stand-ins, and the C ABI of the
new call."""
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, str(Path(__file__).resolve().parent))

import member_outline_standin as msn  # noqa: E402
import outline_standin as osn  # noqa: E402
from geograypher_amd import _hip, build  # noqa: E402
from geograypher_amd.constants import CLASS_ID_KEY  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import synthetic  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"


def mesh_of(points, faces, backend):
    return TexturedPhotogrammetryMesh((np.asarray(points, dtype=np.float64), np.asarray(faces, dtype=np.int64)), log_level="ERROR",
                                      backend=backend)


# -- the stand-in: Y5 and X7 -------------------------------------------------------------------------------------------------------------
def scenes():
    verts, faces, quad = osn.grid_mesh(5, 5, jitter=120_000, seed=1)
    yield "overlapping memberships on a grid", verts, faces, msn.random_rows(len(faces), 4, seed=2), 4
    yield "a face in every class", verts, faces, [list(range(6)) if f == 7 else ([f % 6] if f % 3 else []) for f in range(len(faces))], 6
    yield "empty rows first, inside and last", verts, faces, [[] if f in (0, 20, len(faces) - 1) else [0, 2] for f in range(len(faces))], 3
    yield "all faces clockwise", verts, osn.reversed_faces(faces), msn.random_rows(len(faces), 3, seed=3), 3
    yield "classes outside the range", verts, faces, [[-2, 1, 3, 9]] * len(faces), 3
    verts, faces = osn.fold_scene()
    yield "a fold", verts, faces, [[0, 1], [0]], 2
    shift = np.array([[0, 0], [0, 7], [0, 0], [3, 0], [0, 7], [0, 0], [5, 1], [0, 0]])   # no face centre on another face's edge
    verts, faces = osn.seam_scene()
    yield "a duplicated seam", verts + shift, faces, [[0, 1], [0, 1], [0], [0, 1]], 2
    verts, faces = osn.wall_scene()
    yield "a vertical wall", verts + shift, faces, [[0, 1]] * 6, 2


@pytest.mark.parametrize("scene", list(scenes()), ids=lambda s: s[0])
def test_stand_in_is_the_per_class_trace_concatenated(scene):
    """Y5: class after class, what the class-outline stand-in gives for the class alone."""
    _, verts, faces, rows, n_classes = scene
    face_ptr, face_members = msn.csr_of_rows(rows)
    got = msn.members_np(verts, faces, face_ptr, face_members, n_classes)
    vertices, offsets, classes, stats = [], [0], [], np.zeros(osn.STAT_WORDS, dtype=np.int64)
    for column in range(n_classes):
        alone = osn.outlines_np(verts, faces, msn.column_classes(face_ptr, face_members, column, len(faces)), 1)
        assert np.array_equal(alone["canon"], got["canon"])
        vertices += alone["ring_vertices"].tolist()
        offsets += (alone["ring_offsets"][1:] + offsets[-1]).tolist()
        classes += [column] * alone["n_rings"]
        stats[1:5] += alone["stats"][1:5]   # zero-area, turned, cancelled, multi: per member, so they add up over the columns
    assert got["ring_vertices"].tolist() == vertices and got["ring_offsets"].tolist() == offsets and got["ring_class"].tolist() == classes
    assert got["stats"][1:5].tolist() == stats[1:5].tolist() and got["stats"][msn.BAD_ROWS] == 0
    assert got["stats"][0] == sum(not 0 <= c < n_classes for r in rows for c in set(r))


@pytest.mark.parametrize("scene", list(scenes()), ids=lambda s: s[0])
def test_stand_in_obeys_the_winding_rule_per_class(scene):
    """X7 by brute force: at every face centre the winding number of class c's rings is the number of member faces of c there."""
    _, verts, faces, rows, n_classes = scene
    face_ptr, face_members = msn.csr_of_rows(rows)
    got = msn.members_np(verts, faces, face_ptr, face_members, n_classes)
    checked = 0
    for column in range(n_classes):
        alone = msn.column_classes(face_ptr, face_members, column, len(faces))
        keep = got["ring_class"] == column
        lengths = np.diff(got["ring_offsets"])[keep]
        rings = dict(ring_vertices=np.concatenate([got["ring_vertices"][got["ring_offsets"][r]:got["ring_offsets"][r + 1]]
                                                   for r in np.nonzero(keep)[0]] + [np.zeros(0, dtype=np.int32)]).astype(np.int32),
                     ring_offsets=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), ring_class=np.zeros(int(keep.sum()), dtype=np.int32))
        n, wrong = osn.x7_mismatches(verts, faces, alone, 1, got=rings)
        assert wrong == 0
        checked += n
    assert checked or not any(0 <= c < n_classes for r in rows for c in r)


def test_malformed_tables_are_counted():
    verts, faces, _ = osn.grid_mesh(2, 2)
    ptr, members = msn.csr_of_rows([[0, 1], [1], [], [0, 2], [2], [1, 2], [0], [0, 1, 2]])
    assert msn.bad_rows(ptr, members, 8) == 0
    for edit_ptr, edit_members, want in ((None, {0: 1, 1: 0}, 1), (None, {1: 0}, 1), ({0: 1}, None, 1), ({8: 11}, None, 1), ({4: 2}, None, 1)):
        p, m = ptr.copy(), members.copy()
        for k, v in (edit_ptr or {}).items():
            p[k] = v
        for k, v in (edit_members or {}).items():
            m[k] = v
        assert msn.bad_rows(p, m, 8) >= want and msn.bad_ptr(p, len(m), 8) == (want if edit_ptr else 0)
        got = msn.members_np(verts, faces, p, m, 3)
        assert got["n_edges"] == 0 and got["stats"][msn.BAD_ROWS] > 0
        with pytest.raises(ValueError, match="gr_member_outlines: .* violations"):
            msn.StandInBackend().member_outlines(verts, faces, p, m, 3)


# -- face_label_outlines and export_face_labels_vector on sparse input -------------------------------------------------------------------
def many_hot(n_faces, n_classes, seed):
    rng = np.random.default_rng(seed)
    dense = np.zeros((n_faces, n_classes))
    for f, row in enumerate(msn.random_rows(n_faces, n_classes, seed)):
        dense[f, row] = rng.integers(1, 5, len(row))
    dense[:, 3] = 0.0   # an empty column
    return dense


FIELDS = ("ring_offsets", "ring_class", "ring_vertex_ids", "ring_xy", "ring_is_hole")


def test_sparse_labels_are_traced_in_one_call():
    """Fails before sparse input existed: `face_labels[:, column] > 0` followed by `.astype(np.int32) - 1` does not work on a
    scipy.sparse matrix."""
    points, faces, _ = osn.height_field()
    dense = many_hot(len(faces), 7, seed=4)
    want = mesh_of(points, faces, msn.StandInBackend()).face_label_outlines(dense, points_in_export_CRS=points)
    assert want.stats["calls"] == 6 and len(want) > 6
    rows, cols = np.nonzero(dense)
    split = np.concatenate([dense[rows, cols] - 1, np.ones(len(rows))])          # every entry twice in COO: v - 1 and 1, summed to v
    for name, matrix in (("csr_matrix", sp.csr_matrix(dense)), ("csc_array", sp.csc_array(dense)),
                         ("coo_matrix", sp.coo_matrix((split, (np.tile(rows, 2), np.tile(cols, 2))), shape=dense.shape))):
        backend = msn.StandInBackend()
        got = mesh_of(points, faces, backend).face_label_outlines(matrix, points_in_export_CRS=points)
        assert backend.member_calls == 1 and getattr(backend, "outline_calls", 0) == 0 and got.stats["calls"] == 1, name
        assert backend.last_members["n_classes"] == 7 and backend.last_members["face_members"].dtype == np.int32
        for field in FIELDS:
            assert np.array_equal(getattr(got, field), getattr(want, field)), (name, field)
        differ = ("calls", "faces_without_class")      # the dense path counts, per column, the faces that are not in it; Y3 counts members
        assert {k: v for k, v in got.stats.items() if k not in differ} == {k: v for k, v in want.stats.items() if k not in differ}
        assert got.stats["faces_without_class"] == 0


def test_entries_that_are_not_positive_take_no_part():
    from geograypher_amd.utils.geometric import csr_members

    points, faces, _ = osn.height_field()
    dense = many_hot(len(faces), 5, seed=8)
    noisy = dense.copy()
    noisy[dense == 0] = np.where(np.random.default_rng(1).random(int((dense == 0).sum())) < 0.3, -2.0, 0.0)
    matrix = sp.csr_matrix(noisy)
    rows, cols = np.nonzero(noisy == 0)
    explicit = sp.csr_matrix((np.concatenate([matrix.data, np.zeros(20)]), (np.concatenate([matrix.nonzero()[0], rows[:20]]),
                                                                           np.concatenate([matrix.nonzero()[1], cols[:20]]))), shape=dense.shape)
    assert explicit.nnz == matrix.nnz + 20 and (matrix.data < 0).any()
    cancel = sp.coo_matrix((np.array([3.0, -3.0, 2.0]), (np.array([5, 5, 6]), np.array([1, 1, 2]))), shape=dense.shape)   # sums to 0
    ptr, members = csr_members(cancel)
    assert members.tolist() == [2] and ptr[6] == 0 and ptr[7] == 1
    want = mesh_of(points, faces, msn.StandInBackend()).face_label_outlines(dense, points_in_export_CRS=points)
    for m in (matrix, explicit):
        got = mesh_of(points, faces, msn.StandInBackend()).face_label_outlines(m, points_in_export_CRS=points)
        assert all(np.array_equal(getattr(got, f), getattr(want, f)) for f in FIELDS)
    ptr, members = csr_members(explicit)
    assert len(members) == int((dense > 0).sum()) and ptr[-1] == len(members) and msn.bad_rows(ptr, members, len(faces)) == 0


def test_a_backend_without_member_outlines_gets_a_call_per_column():
    points, faces, _ = osn.height_field()
    dense = many_hot(len(faces), 6, seed=12)
    old = osn.StandInBackend()
    assert not hasattr(old, "member_outlines")
    got = mesh_of(points, faces, old).face_label_outlines(sp.csr_array(dense), points_in_export_CRS=points)
    want = mesh_of(points, faces, msn.StandInBackend()).face_label_outlines(sp.csr_array(dense), points_in_export_CRS=points)
    assert old.outline_calls == 5 == got.stats["calls"] and want.stats["calls"] == 1
    assert all(np.array_equal(getattr(got, f), getattr(want, f)) for f in FIELDS)
    with pytest.raises(ValueError, match="face labels for a mesh"):
        mesh_of(points, faces, old).face_label_outlines(sp.csr_array(dense[:-1]), points_in_export_CRS=points)
    wide = sp.csr_array((np.ones(1), (np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64))), shape=(len(faces), 2 ** 31 - 1))
    with pytest.raises(ValueError, match="at most 2147483646"):
        mesh_of(points, faces, msn.StandInBackend()).face_label_outlines(wide, points_in_export_CRS=points)
    empty = mesh_of(points, faces, msn.StandInBackend()).face_label_outlines(sp.csr_array(dense.shape), points_in_export_CRS=points)
    assert len(empty) == 0 and empty.stats["calls"] == 1


def test_export_of_a_sparse_matrix_has_a_row_per_present_column(tmp_path):
    points, faces, _ = osn.height_field()
    dense = many_hot(len(faces), 7, seed=4)
    mesh = mesh_of(points, faces, msn.StandInBackend())
    polygons, columns = mesh.export_face_labels_vector(sp.csr_array(dense), tmp_path / "sparse.geojson", points_in_export_CRS=points)
    want, want_columns = mesh_of(points, faces, msn.StandInBackend()).export_face_labels_vector(dense, tmp_path / "dense.geojson",
                                                                                                points_in_export_CRS=points)
    present = [float(c) for c in range(7) if (dense[:, c] > 0).any()]
    assert columns[CLASS_ID_KEY][:len(present)].tolist() == present == want_columns[CLASS_ID_KEY][:len(present)].tolist()
    assert mesh.last_outline_stats["calls"] == 1 and mesh.last_outline_stats["rows"] == len(columns[CLASS_ID_KEY])
    assert (tmp_path / "sparse.geojson").read_text() == (tmp_path / "dense.geojson").read_text()
    assert len(polygons.rings) == len(want.rings) and len(PlanarPolygons.from_geojson(tmp_path / "sparse.geojson")[0]) == len(polygons)


# -- the entry point -------------------------------------------------------------------------------------------------------------------
def test_project_detections_end_to_end(tmp_path, oracle_backend_cls, monkeypatch):
    from PIL import Image

    import geograypher_amd.entrypoints.project_detections as module
    from geograypher_amd.constants import INSTANCE_ID_KEY
    from geograypher_amd.entrypoints import project_detections

    class Full(msn.StandInBackend, oracle_backend_cls):
        pass

    (points, faces), cams = synthetic.config1_scene()
    sub = cams[0:2]
    (tmp_path / "images").mkdir()
    for i, c in enumerate(sub.cameras):
        c.image_filename = Path(tmp_path, "images", f"img{i}.png")
        Image.fromarray(np.zeros((480, 640), dtype=np.uint8)).save(c.image_filename)
    sub.image_folder = Path(tmp_path, "images")
    seen = {}

    def camera_set(cameras_filename, image_folder, default_sensor_params):
        seen.update(cameras_filename=cameras_filename, image_folder=image_folder, default_sensor_params=default_sensor_params)
        return sub

    monkeypatch.setattr(module, "MetashapeCameraSet", camera_set)
    np.savez(tmp_path / "mesh.npz", points=points, faces=faces)
    export_points = points + np.array([500_000.0, 4_000_000.0, 0.0])
    np.save(tmp_path / "export_points.npy", export_points)
    args = (tmp_path / "mesh.npz", "EPSG:4978", "cameras.xml")
    common = dict(projections_to_mesh_filename=tmp_path / "out" / "projections.npz", backend=Full())
    polygons, joined = project_detections(
        *args, project_to_mesh=True, convert_to_geospatial=True, image_folder=tmp_path / "images",
        detections_folder=GOLDEN / "tabular" / "cols", projections_to_geospatial_savefilename=tmp_path / "out" / "first.geojson",
        default_focal_length=500.0, segmentor_kwargs={"split_bbox": False}, export_points_file=tmp_path / "export_points.npy", **common)
    assert seen == dict(cameras_filename="cameras.xml", image_folder=tmp_path / "images", default_sensor_params={"f": 500.0, "cx": 0, "cy": 0})
    assert (tmp_path / "out" / "projections.npz").is_file() and (tmp_path / "out" / "projections_detection_info.csv").is_file()
    matrix = sp.load_npz(tmp_path / "out" / "projections.npz")
    assert matrix.shape == (len(faces), 10) and matrix.nnz > 50          # the shape came from the first image: 480 x 640
    present = sorted(set(matrix.nonzero()[1].tolist()))
    assert joined[INSTANCE_ID_KEY].tolist() == present and len(present) >= 3 and len(polygons) == len(present)
    assert CLASS_ID_KEY not in joined and "Unnamed: 0" not in joined
    assert {"image_path", "xmin", "species", "label_int", "score", INSTANCE_ID_KEY} <= set(joined)
    species = ["pine", "oak", "fir", "pine", "oak", "fir, grand", "pine", "fir", "oak", "oak"]    # a.csv then b.csv, instance_ID = row
    assert joined["species"].tolist() == [species[i] for i in present]
    features = json.loads((tmp_path / "out" / "first.geojson").read_text())["features"]
    assert [f["properties"][INSTANCE_ID_KEY] for f in features] == present and all(CLASS_ID_KEY not in f["properties"] for f in features)
    assert all(f["geometry"]["coordinates"] for f in features)
    # the same polygons as the mesh method gives for the matrix
    want, want_columns = mesh_of(points, faces, msn.StandInBackend()).export_face_labels_vector(matrix, points_in_export_CRS=export_points)
    assert want_columns[CLASS_ID_KEY].tolist() == [float(i) for i in present]
    assert len(want.rings) == len(polygons.rings) and all(np.array_equal(a, b) for a, b in zip(want.rings, polygons.rings))
    # the second step alone, from the two files
    again, joined_again = project_detections(*args, convert_to_geospatial=True, export_points_file=export_points,
                                             projections_to_geospatial_savefilename=tmp_path / "out" / "second.geojson", **common)
    assert (tmp_path / "out" / "second.geojson").read_text() == (tmp_path / "out" / "first.geojson").read_text()
    assert list(joined_again) == list(joined) and all(joined_again[k].tolist() == joined[k].tolist() for k in joined if k != "score")
    assert str(joined_again["score"].tolist()) == str(joined["score"].tolist())      # NaN for the empty cell, both times
    # the first step alone returns the matrix
    only = project_detections(*args, project_to_mesh=True, image_folder=tmp_path / "images", detections_folder=GOLDEN / "tabular" / "cols",
                              image_shape=(480, 640), segmentor_kwargs={"split_bbox": False}, backend=Full())
    assert (only != matrix).nnz == 0
    # a column of the table named like a projected one, and rows without a match
    rows, merged = module.join_detection_info({CLASS_ID_KEY: np.array([0.0, 2.0, 7.0]), "area": np.array([1.0, 2.0, 3.0])},
                                              {"Unnamed: 0": [0, 1, 2], INSTANCE_ID_KEY: [2, 0, 5], "area": [9, 8, 7]})
    assert rows.tolist() == [0, 1] and merged["area"].tolist() == [1.0, 2.0] and merged["area_right"].tolist() == [8, 9]
    assert merged[INSTANCE_ID_KEY].tolist() == [0, 2] and set(merged) == {"area", "area_right", INSTANCE_ID_KEY}


def test_project_detections_refusals(tmp_path):
    from geograypher_amd.entrypoints.project_detections import parse_args, project_detections

    (points, faces), _ = synthetic.config1_scene()
    np.savez(tmp_path / "mesh.npz", points=points, faces=faces)
    args = (tmp_path / "mesh.npz", "EPSG:4978", "cameras.xml")
    with pytest.raises(NotImplementedError, match="^convert_to_geospatial: .*export_points_file or export_CRS"):
        project_detections(*args, convert_to_geospatial=True, projections_to_mesh_filename=tmp_path / "p.npz")
    with pytest.raises(ValueError, match="export_points_file and export_CRS are both given"):
        project_detections(*args, convert_to_geospatial=True, export_points_file=points, export_CRS="EPSG:32610")
    with pytest.raises(ValueError, match="^No projections_to_mesh_savefilename provided$"):
        project_detections(*args, convert_to_geospatial=True, export_points_file=points)
    with pytest.raises(FileNotFoundError, match="projections_to_mesh_filename .*missing.npz not found"):
        project_detections(*args, convert_to_geospatial=True, export_points_file=points, projections_to_mesh_filename=tmp_path / "missing.npz")
    with pytest.raises(NotImplementedError, match="^vis_mesh"):
        project_detections(*args, project_to_mesh=True, vis_mesh=True)
    with pytest.raises(NotImplementedError, match="^vis_geodata"):
        project_detections(*args, convert_to_geospatial=True, vis_geodata=True, export_points_file=points)
    sp.save_npz(tmp_path / "p.npz", sp.csr_array((len(faces), 2), dtype=int))
    (tmp_path / "p_detection_info.csv").write_text(",instance_ID\n0,0\n1,1\n")
    with pytest.raises(NotImplementedError, match="geojson"):
        project_detections(*args, convert_to_geospatial=True, export_points_file=points, projections_to_mesh_filename=tmp_path / "p.npz",
                           projections_to_geospatial_savefilename=tmp_path / "x.gpkg", backend=msn.StandInBackend())
    (tmp_path / "none").mkdir()
    with pytest.raises(ValueError, match="No image_shape provided and folder of images"):
        project_detections(*args[:2], ROOT / "tests" / "golden" / "metashape_camera.xml", project_to_mesh=True, image_folder=tmp_path / "none",
                           detections_folder=GOLDEN / "tabular" / "cols", default_focal_length=500.0, backend=msn.StandInBackend())
    base = ["--mesh-filename", "m.npz", "--mesh-CRS", "EPSG:4978", "--cameras-filename", "c.xml"]
    parsed = parse_args(base)
    assert parsed.project_to_mesh is False and parsed.convert_to_geospatial is False and parsed.image_shape is None
    assert parsed.mesh_filename == Path("m.npz") and parsed.export_CRS is None and parsed.vis_mesh is False
    parsed = parse_args(base + ["--project-to-mesh", "--convert-to-geospatial", "--image-shape", "3000", "4000", "--default-focal-length",
                                "3000.5", "--export-CRS", "EPSG:32610", "--projections-to-geospatial-savefilename", "out.geojson"])
    assert parsed.project_to_mesh is True and parsed.convert_to_geospatial is True and parsed.image_shape == (3000, 4000)
    assert parsed.default_focal_length == 3000.5 and parsed.export_CRS == "EPSG:32610"
    assert parsed.projections_to_geospatial_savefilename == Path("out.geojson")
    import inspect

    assert set(vars(parsed)) == set(inspect.signature(project_detections).parameters) - {"segmentor_kwargs", "backend"}


# -- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_companion_header_and_binding_agree():
    """The contract tests/test_cabi.py keeps for include/geograster.h, for the companion header that geograster.h includes: every
    function it declares is in the binding's companion table with as many arguments, each of the declared kind (a pointer, a
    64-bit integer, an int), and the library exports it."""
    import ctypes

    main = (ROOT / "include" / "geograster.h").read_text()
    assert re.search(r'^#include "geograster_outlines.h"$', main, re.M) and main.index("geograster_outlines.h") < main.rindex("#ifdef __cplusplus")
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", (ROOT / "include" / "geograster_outlines.h").read_text(), flags=re.S)
    declared = {name: [a.strip() for a in " ".join(args.split()).split(",")]
                for name, args in re.findall(r"\b(gr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}
    assert sorted(declared) == sorted(_hip._COMPANION_SIGNATURES) == sorted(_hip.COMPANION_SYMBOLS) == ["gr_member_outlines"]
    assert not set(declared) & set(_hip._SIGNATURES)
    kinds = {ctypes.c_int64: "int64", ctypes.c_int: "int", ctypes.c_int32: "int"}
    lib = ctypes.CDLL(str(build.build()))
    for name, arguments in declared.items():
        argtypes = _hip._COMPANION_SIGNATURES[name]
        assert len(arguments) == len(argtypes) and hasattr(lib, name), name
        for argument, ctype in zip(arguments, argtypes):
            want = "pointer" if "*" in argument else {"int64_t": "int64", "int32_t": "int", "int": "int"}[argument.split()[0]]
            got = "pointer" if ctype is ctypes.c_void_p or issubclass(ctype, ctypes._Pointer) else kinds[ctype]
            assert want == got, f"{name}: {argument!r} is bound as {ctype.__name__}"


def test_header_binding_and_source_name_the_new_call():
    header = (ROOT / "include" / "geograster.h").read_text()
    companion = (ROOT / "include" / "geograster_outlines.h").read_text()
    source = (ROOT / "geograypher_amd" / "csrc" / "polygons.hip").read_text()
    internal = (ROOT / "geograypher_amd" / "csrc" / "gr_internal.hpp").read_text()
    name, n_args = "gr_member_outlines", 18
    decl = re.search(rf"\bint {name}\((.*?)\);", companion, re.S).group(1)
    assert len(decl.split(",")) == n_args == len(_hip._COMPANION_SIGNATURES[name])
    definition = re.search(rf"\bint {name}\((gr_ctx \*c,.*?)\) \{{", source, re.S).group(1)
    assert len(definition.split(",")) == n_args
    assert "k_outline_member_edges" in source and "k_outline_member_edges" in internal and "outline_trace" in internal
    assert (_hip.GR_OUTL_STAT_BAD_ROWS, _hip.GR_OUTL_STAT_WORDS, _hip.GR_MEMBER_MAX_CLASSES, _hip.GR_OUTL_MAX_CLASSES) == (6, 8, 2 ** 31 - 2, 65535)
    assert re.search(r"GR_OUTL_STAT_BAD_ROWS = 6\b", header) and re.search(r"GR_MEMBER_MAX_CLASSES = 2147483646\b", header)
    # both entry points hand their edge kernel to the one trace, which alone sorts, scans and acquires scratch
    for entry, kernel in (("gr_class_outlines", "k_outline_face_edges"), (name, "k_outline_member_edges")):
        start = source.index(f"int {entry}(gr_ctx *c,")
        body = source[start:source.index("\n}\n", start)]
        assert "outline_trace(c, " in body and kernel in body and "hipcub::" not in body and "stage_acquire" not in body
    assert source.count("static int outline_trace(") == 2     # the declaration and the definition
    # every argument check returns GR_EINVAL, naming the call, before the first device call
    body = source[source.index(f"int {name}(gr_ctx *c,"):]
    checks = body[:body.index("hipSetDevice")]
    assert checks.count("return fail(c, GR_EINVAL, \"gr_member_outlines:") == 3 and "if (!c) return GR_EINVAL;" in checks
    for condition in ("V < 0", "F < 0", "nnz < 0", "ring_vertex_cap < 0", "nnz > 0x7FFFFFFFll / 3", "n_classes < 0",
                      "n_classes > GR_MEMBER_MAX_CLASSES", "!stats", "!face_ptr", "nnz > 0 && !face_members", "F > 0 && !faces"):
        assert condition in checks, condition
    assert "hipLaunchKernelGGL" not in checks and "hipMemsetAsync" not in checks
    kernel = source[source.index("void k_outline_member_edges("):source.index("// pair, cl [n] sorted")]
    assert "atomic" not in kernel and kernel.count("stat_add_u32(") + kernel.count("stat_count(") == 5      # no atomics but the counters
    assert not re.search(r"\b(double|float)\b", kernel)
    assert any(p.name == "polygons.hip" for p in build.SOURCES) and callable(_hip.HipRaster.member_outlines)


def test_a_call_without_a_context_is_refused_by_the_library():
    import ctypes

    lib = ctypes.CDLL(str(build.build()))
    lib.gr_member_outlines.restype = ctypes.c_int
    lib.gr_member_outlines.argtypes = _hip._COMPANION_SIGNATURES["gr_member_outlines"]
    n = ctypes.c_int64(0)
    assert lib.gr_member_outlines(None, None, 0, None, 0, None, None, 0, 1, None, None, None, None, 0, ctypes.byref(n), ctypes.byref(n),
                                  None, None) == _hip.GR_EINVAL
