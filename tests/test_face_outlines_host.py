"""Class outlines without a GPU: the exact stand-in of tests/outline_standin.py against rule X7 by brute force,
the round trip mesh -> `.geojson` -> `face_polygon_index`, the nesting of rule X8, files and arguments, `aggregate_images` end to end
on the CPU stand-ins, and the C ABI of the new call."""
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import outline_standin as osn  # noqa: E402
import region_standin as rs  # noqa: E402
import vector_standin as vs  # noqa: E402
from geograypher_amd import _hip, build  # noqa: E402
from geograypher_amd.constants import CLASS_ID_KEY, CLASS_NAMES_KEY  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import geometric, synthetic  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]


class Backend(osn.StandInBackend, vs.StandInBackend):
    pass


def mesh_of(points, faces, **kw):
    return TexturedPhotogrammetryMesh((np.asarray(points, dtype=np.float64), np.asarray(faces, dtype=np.int64)), log_level="ERROR",
                                      backend=kw.pop("backend", None) or Backend(), **kw)


def metres(verts_q):
    return np.column_stack([np.asarray(verts_q, dtype=np.float64) * 1e-6, np.zeros(len(verts_q))])


# -- X7 --------------------------------------------------------------------------------------------------------------------------------
def x7_scenes():
    rng = np.random.default_rng(11)
    verts, faces, quad = osn.grid_mesh(5, 5, jitter=120_000, seed=1)
    yield "random classes on a grid: pinch vertices", verts, faces, rng.integers(-1, 3, len(faces)).astype(np.int32), 3
    yield "a checkerboard", verts, faces, osn.quad_classes(quad, [(i + j) % 2 for j in range(5) for i in range(5)]), 2
    yield "all faces clockwise", verts, osn.reversed_faces(faces), osn.quad_classes(quad, rng.integers(0, 2, 25)), 2
    # a crown layer above the ground, partly of the ground's class: the class overlaps itself in plan view
    crown, crown_faces, crown_quad = osn.grid_mesh(3, 3, step=1_100_000, jitter=90_000, seed=2)
    both = np.vstack([verts, crown + np.array([733_331, 871_717])])
    both_faces = np.vstack([faces, crown_faces + len(verts)])
    both_classes = np.concatenate([np.zeros(len(faces), dtype=np.int32), osn.quad_classes(crown_quad, [0, 1, 0, 1, 0, -1, 0, 0, 1])])
    yield "a crown above ground of its own class", both, both_faces, both_classes, 2
    verts, faces = osn.fold_scene()
    yield "a fold, one class", verts, faces, [0, 0], 1
    yield "a fold, two classes", verts, faces, [0, 1], 2
    verts, faces = osn.seam_scene()
    yield "a duplicated seam", verts + np.array([[0, 0], [0, 7], [0, 0], [3, 0], [0, 7], [0, 0], [5, 1], [0, 0]]), faces, [0, 0, 0, 0], 1
    verts, faces = osn.wall_scene()
    yield "a vertical wall", verts + np.array([[0, 0], [0, 7], [0, 0], [3, 0], [0, 7], [0, 0], [5, 1], [0, 0]]), faces, [0] * 6, 1


@pytest.mark.parametrize("scene", list(x7_scenes()), ids=lambda s: s[0])
def test_standin_obeys_X7(scene):
    _, verts, faces, classes, n_classes = scene
    got = osn.outlines_np(verts, faces, classes, n_classes)
    checked, wrong = osn.x7_mismatches(verts, faces, classes, n_classes, got)
    assert checked >= 2 and wrong == 0
    # every ring closes over edges that exist, and no edge of a class is left twice in opposite directions
    slots = set()
    off = got["ring_offsets"]
    for r, c in enumerate(got["ring_class"].tolist()):
        ring = got["ring_vertices"][off[r]:off[r + 1]].tolist()
        assert len(ring) >= 3
        slots.update((c, a, b) for a, b in zip(ring, ring[1:] + ring[:1]))
    assert not any((c, b, a) in slots for c, a, b in slots)


def test_overlapping_class_has_overlapping_rings():
    """What X7 documents: a crown above ground of the same class gives rings that overlap; the winding number there is 2."""
    _, verts, faces, classes, n_classes = list(x7_scenes())[3]
    got = osn.outlines_np(verts, faces, classes, n_classes)
    xy = [(3 * int(x), 3 * int(y)) for x, y in verts]
    rings0 = [[xy[v] for v in got["ring_vertices"][got["ring_offsets"][r]:got["ring_offsets"][r + 1]].tolist()]
              for r in np.nonzero(got["ring_class"] == 0)[0]]
    crown_face = faces[50]   # crown quad 0, class 0, above ground of class 0
    p = tuple(sum(xy[v][k] for v in crown_face) // 3 for k in (0, 1))
    assert sum(osn.winding_number(ring, *p) for ring in rings0) == 2


# -- the round trip ------------------------------------------------------------------------------------------------------------------
def test_round_trip_through_geojson_and_face_polygon_index(tmp_path):
    points, faces, labels = osn.height_field()
    backend = Backend()
    mesh = mesh_of(points, faces, backend=backend)
    polygons, columns = mesh.export_face_labels_vector(labels, tmp_path / "map.geojson", label_names=["oak", "fir", "ash"],
                                                       points_in_export_CRS=points)
    assert columns[CLASS_ID_KEY].tolist() == [0.0, 1.0, 2.0] and columns[CLASS_NAMES_KEY].tolist() == ["oak", "fir", "ash"]
    assert mesh.last_outline_stats["orphan_holes"] == 0 and mesh.last_outline_stats["rows"] == 3
    assert polygons.ring_is_hole.sum() >= 2 and (polygons.ring_polygon == 0).sum() >= 3   # class 0: two parts, one of them an island
    back, properties = PlanarPolygons.from_geojson(tmp_path / "map.geojson")
    assert len(back) == 3 and properties[CLASS_ID_KEY].tolist() == [0.0, 1.0, 2.0] and list(properties[CLASS_NAMES_KEY]) == ["oak", "fir", "ash"]
    assert len(back.rings) == len(polygons.rings) and all(np.array_equal(a, b) for a, b in zip(back.rings, polygons.rings))
    data = json.loads((tmp_path / "map.geojson").read_text())
    assert all(f["geometry"]["type"] == "MultiPolygon" and all(ring[0] == ring[-1] for part in f["geometry"]["coordinates"] for ring in part)
               for f in data["features"])
    index = mesh.face_polygon_index(back, points_in_polygon_CRS=points)
    _, info = vs.face_polygon_index_np(backend.last["verts_q"], backend.last["faces"], backend.last["table"])
    assert info["on_boundary"].sum() == 0          # the condition: no face centre lies on an outline
    want = np.where(np.isnan(labels), -1, np.nan_to_num(labels)).astype(np.int32)
    assert np.array_equal(index, want) and (want >= 0).sum() > 100 and (want < 0).sum() > 100


# -- X8 --------------------------------------------------------------------------------------------------------------------------------
def nested(verts, faces, classes, n_classes):
    got = osn.outlines_np(verts, faces, classes, n_classes)
    areas2, home = geometric.nest_outline_rings(verts[got["ring_vertices"]], got["ring_offsets"], got["ring_class"])
    want_areas2, want_home = osn.nest_np(verts, got)
    assert areas2 == want_areas2 and home.tolist() == want_home
    return got, areas2, home.tolist()


def test_X8_holes_islands_and_a_touching_hole(tmp_path):
    s2 = 2 * 10 ** 12   # twice the area of a quad, in grid steps squared
    verts3, faces3, quad3 = osn.grid_mesh(3, 3)
    got, areas2, home = nested(verts3, faces3, osn.quad_classes(quad3, [0, 0, 0, 0, 1, 0, 0, 0, 0]), 2)
    assert got["ring_class"].tolist() == [0, 0, 1] and sorted(areas2[:2]) == [-s2, 9 * s2] and areas2[2] == s2
    hole = areas2.index(-s2)
    assert home[hole] == 1 - hole and home[1 - hole] == -1 and home[2] == -1
    # an island of class 0 inside the hole of a ring of class 0: a part of its own, the hole stays with the outer ring
    verts5, faces5, quad5 = osn.grid_mesh(5, 5)
    rings5 = np.zeros((5, 5), dtype=np.int32)
    rings5[1:4, 1:4] = 1
    rings5[2, 2] = 0
    got, areas2, home = nested(verts5, faces5, osn.quad_classes(quad5, rings5), 2)
    of_class0 = [r for r in range(got["n_rings"]) if got["ring_class"][r] == 0]
    assert sorted(areas2[r] for r in of_class0) == [-9 * s2, s2, 25 * s2]
    outer, island, hole = (next(r for r in of_class0 if areas2[r] == a) for a in (25 * s2, s2, -9 * s2))
    assert home[hole] == outer and home[island] == -1
    mesh = mesh_of(metres(verts5), faces5)
    polygons, columns = mesh.export_face_labels_vector(osn.quad_classes(quad5, rings5).astype(np.float64), points_in_export_CRS=metres(verts5))
    row0 = [(bool(h), len(r)) for r, p, h in zip(polygons.rings, polygons.ring_polygon, polygons.ring_is_hole) if p == 0]
    assert sorted(row0) == [(False, 4), (False, 20), (True, 12)] and row0.index((True, 12)) == row0.index((False, 20)) + 1
    # the island lies inside the outer ring too: the smaller exterior is only a candidate for what it holds
    got1, areas2_1, home1 = nested(verts5, faces5, osn.quad_classes(quad5, 1 - rings5), 2)
    assert sum(a < 0 for a in areas2_1) == 2 and all(h >= 0 for a, h in zip(areas2_1, home1) if a < 0)
    # a hole that touches the outer ring in one vertex
    verts4, faces4, quad4 = osn.grid_mesh(4, 4)
    touching = np.zeros(16, dtype=np.int32)
    touching[5], touching[0] = 1, -1
    got, areas2, home = nested(verts4, faces4, osn.quad_classes(quad4, touching), 2)
    assert sorted(areas2) == [-s2, s2, 15 * s2] and home[areas2.index(-s2)] == areas2.index(15 * s2)
    assert osn.x7_mismatches(verts4 * 3 + np.arange(50).reshape(25, 2) % 7, faces4, osn.quad_classes(quad4, touching), 2)[1] == 0
    # a hole no exterior of its class holds becomes a row of its own, flagged
    verts = np.array([[0, 0], [4, 0], [4, 4], [0, 4]], dtype=np.int64) * 1_000_000
    _, home_orphan = geometric.nest_outline_rings(verts[[0, 3, 2, 1]], [0, 4], [0])
    assert home_orphan.tolist() == [-1]


def test_orphan_hole_gets_a_row_of_its_own():
    class Orphan(Backend):
        def class_outlines(self, verts_q, faces, face_class, n_classes, **kw):
            canon = np.arange(len(verts_q), dtype=np.int32)
            return (canon, np.array([0, 3, 2, 1, 0, 1, 2], dtype=np.int32), np.array([0, 4, 7]), np.array([0, 0], dtype=np.int32),
                    np.zeros(8, dtype=np.int64))

    points = np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 4.0], [0.0, 4.0]])
    mesh = mesh_of(np.column_stack([points, np.zeros(4)]), [[0, 1, 2], [0, 2, 3]], backend=Orphan())
    polygons, columns = mesh.export_face_labels_vector(np.zeros(2), points_in_export_CRS=points)
    assert len(polygons) == 2 and columns[CLASS_ID_KEY].tolist() == [0.0, 0.0] and mesh.last_outline_stats["orphan_holes"] == 1
    assert polygons.ring_polygon.tolist() == [0, 1] and not polygons.ring_is_hole.any()


# -- files and arguments ---------------------------------------------------------------------------------------------------------------
def test_arguments_files_and_label_forms(tmp_path):
    points, faces, labels = osn.height_field()
    mesh = mesh_of(points, faces)
    kw = dict(points_in_export_CRS=points)
    for bad, match in ((dict(export_file=tmp_path / "map.gpkg"), "geojson"), (dict(ensure_non_overlapping=True), "ensure_non_overlapping"),
                       (dict(simplify_tol=0.05), "simplify_tol"), (dict(vis=True), "vis"), (dict(export_crs="EPSG:4326"), "export_crs")):
        with pytest.raises(NotImplementedError, match=match):
            mesh.export_face_labels_vector(labels, **bad, **kw)
    with pytest.raises(ValueError, match="face labels for a mesh"):
        mesh.export_face_labels_vector(labels[:-1], **kw)
    with pytest.raises(ValueError, match="points_in_export_CRS must be"):
        mesh.face_label_outlines(labels, points_in_export_CRS=points[:-1])
    with pytest.raises(ValueError, match="whole numbers"):
        mesh.face_label_outlines(np.where(np.isnan(labels), np.nan, labels + 0.5), **kw)
    far = points.copy()
    far[0, 0] += 3.0e6
    with pytest.raises(ValueError, match="2\\^40"):
        mesh.face_label_outlines(labels, points_in_export_CRS=far)
    with pytest.raises(TypeError):
        mesh.face_label_outlines(labels)   # the points are required
    # label forms: (F,), (F, 1), integers, the mesh's own texture; 2-D points
    base = mesh.face_label_outlines(labels, **kw)
    assert base.ring_class.dtype == np.float64 and base.ring_vertex_ids.dtype == np.int32 and base.ring_offsets.dtype == np.int64
    assert base.ring_xy.shape == (base.ring_offsets[-1], 2) and np.array_equal(base.ring_xy, points[base.ring_vertex_ids, :2])
    assert base.ring_is_hole.dtype == bool and base.stats["rings"] == len(base) == len(base.ring_class)
    assert base.stats["faces_without_class"] == int(np.isnan(labels).sum()) and mesh.last_outline_stats == base.stats
    as_int = np.where(np.isnan(labels), 7, labels).astype(np.int64)
    textured = mesh_of(points, faces, texture=labels.reshape(-1, 1))
    for other in (mesh.face_label_outlines(labels.reshape(-1, 1), **kw), textured.face_label_outlines(**kw),
                  mesh.face_label_outlines(labels, points_in_export_CRS=points[:, :2])):
        for field in ("ring_offsets", "ring_class", "ring_vertex_ids", "ring_xy", "ring_is_hole"):
            assert np.array_equal(getattr(other, field), getattr(base, field)), field
    ints = mesh.face_label_outlines(as_int, **kw)
    assert sorted(set(ints.ring_class.tolist())) == [0.0, 1.0, 2.0, 7.0]
    # drop_nan=False: the unlabelled faces are one more class, reported as NaN, behind the others
    with_nan = mesh.face_label_outlines(labels, drop_nan=False, **kw)
    n = len(base)
    assert np.array_equal(with_nan.ring_class[:n], base.ring_class) and np.isnan(with_nan.ring_class[n:]).all() and len(with_nan) > n
    assert np.array_equal(with_nan.ring_vertex_ids[:base.ring_offsets[-1]], base.ring_vertex_ids)
    assert np.array_equal(with_nan.ring_vertex_ids[base.ring_offsets[-1]:], ints.ring_vertex_ids[ints.ring_offsets[np.argmax(ints.ring_class == 7)]:])
    polygons, columns = mesh.export_face_labels_vector(labels, tmp_path / "nan.geojson", label_names=["a", "b", "c"], drop_nan=False, **kw)
    assert np.isnan(columns[CLASS_ID_KEY][3]) and columns[CLASS_NAMES_KEY].tolist() == ["a", "b", "c", "nan"]
    assert json.loads((tmp_path / "nan.geojson").read_text())["features"][3]["properties"] == {CLASS_ID_KEY: None, CLASS_NAMES_KEY: "nan"}
    # many-hot: one call per non-empty column, a face takes part where its value is > 0
    many = np.zeros((len(faces), 5))
    many[labels == 0, 1] = 0.5
    many[labels == 2, 1] = 2.0
    many[labels == 1, 4] = 1.0
    many[labels == 2, 3] = -1.0    # not > 0: no part, and no call for the column
    backend = Backend()
    hot = mesh_of(points, faces, backend=backend).face_label_outlines(many, **kw)
    assert backend.outline_calls == 2 and hot.stats["calls"] == 2 and sorted(set(hot.ring_class.tolist())) == [1.0, 4.0]
    merged = mesh.face_label_outlines(np.where((labels == 0) | (labels == 2), 0.0, np.nan), **kw)
    k = int((hot.ring_class == 1).sum())
    assert np.array_equal(hot.ring_vertex_ids[:hot.ring_offsets[k]], merged.ring_vertex_ids) and k == len(merged)
    only_1 = mesh.face_label_outlines(np.where(labels == 1, 0.0, np.nan), **kw)
    assert np.array_equal(hot.ring_vertex_ids[hot.ring_offsets[k]:], only_1.ring_vertex_ids)
    assert np.array_equal(hot.ring_offsets[k:] - hot.ring_offsets[k], only_1.ring_offsets)
    polygons, columns = mesh.export_face_labels_vector(many, **kw)
    assert columns[CLASS_ID_KEY].tolist() == [1.0, 4.0] and len(polygons) == 2
    # more distinct classes than one call takes
    with pytest.raises(ValueError, match="65535"):
        big = mesh_of(np.zeros((3, 3)), np.zeros((70000, 3), dtype=np.int64))
        big.face_label_outlines(np.arange(70000, dtype=np.float64), points_in_export_CRS=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="n_classes=65536"):
        Backend().class_outlines(np.zeros((3, 2), dtype=np.int64), np.zeros((0, 3), dtype=np.int32), [], 65536)


# -- the entry point -------------------------------------------------------------------------------------------------------------------
def test_aggregate_images_writes_the_top_down_map(tmp_path, oracle_backend_cls):
    from PIL import Image

    from geograypher_amd.entrypoints.aggregate_images import aggregate_images, parse_args

    class Full(osn.StandInBackend, rs.StandInBackend, vs.StandInBackend, oracle_backend_cls):
        pass

    (points, faces), cams = synthetic.config1_scene()
    sub = cams[0:2]
    for i, c in enumerate(sub.cameras):
        c.image_filename = Path(tmp_path, "images", "flight", f"img_{i}.JPG")
    sub.image_folder = Path(tmp_path, "images")
    lo, hi = points[:, :2].min(axis=0), points[:, :2].max(axis=0)
    roi = [vs.square(*(lo + (hi - lo) * 0.2), *(lo + (hi - lo) * 0.7))]
    h, w = sub.cameras[0].get_image_size()
    rng = np.random.default_rng(1)
    for i in range(2):
        (tmp_path / "labels" / "flight").mkdir(parents=True, exist_ok=True)
        blocks = rng.integers(0, 4, (h // 32 + 1, w // 32 + 1)).astype(np.uint8)
        Image.fromarray(np.kron(blocks, np.ones((32, 32), dtype=np.uint8))[:h, :w]).save(tmp_path / "labels" / "flight" / f"img_{i}.png")
    np.savez(tmp_path / "mesh.npz", points=points, faces=faces)
    export_points = points + np.array([500_000.0, 4_000_000.0, 0.0])     # the vertices in the CRS of the map
    np.save(tmp_path / "export_points.npy", export_points)
    ids = {0: "a", 1: "b", 2: "c", 3: "d"}
    kw = dict(take_every_nth_camera=1, aggregate_image_scale=0.25, camera_set=sub, IDs_to_labels=ids)
    args = (tmp_path / "mesh.npz", None, tmp_path / "images", tmp_path / "labels", "EPSG:4978")
    mesh, _, classes = aggregate_images(*args, ROI=roi, ROI_buffer_radius_meters=0.0, ROI_points_file=points,
                                        top_down_vector_projection_savefile=tmp_path / "out" / "map.geojson",
                                        top_down_points_file=tmp_path / "export_points.npy", backend=Full(), **kw)
    assert mesh.ROI_point_IDs is not None and 0 < len(mesh.ROI_point_IDs) < len(points)
    got, properties = PlanarPolygons.from_geojson(tmp_path / "out" / "map.geojson")
    present = sorted(set(classes[np.isfinite(classes)].tolist()))
    assert len(present) == 4 and properties[CLASS_ID_KEY].tolist() == present and list(properties[CLASS_NAMES_KEY]) == ["a", "b", "c", "d"]
    want, _ = mesh.export_face_labels_vector(classes[:, 0], label_names=["a", "b", "c", "d"],
                                             points_in_export_CRS=export_points[mesh.ROI_point_IDs])   # the CROPPED vertices
    assert len(got.rings) == len(want.rings) > 4 and all(np.array_equal(a, b) for a, b in zip(got.rings, want.rings))
    assert np.array_equal(got.ring_polygon, want.ring_polygon) and np.array_equal(got.ring_is_hole, want.ring_is_hole)
    # the array form, no ROI
    aggregate_images(*args, top_down_vector_projection_savefile=tmp_path / "out" / "full.geojson", top_down_points_file=export_points,
                     backend=Full(), **kw)
    assert len(PlanarPolygons.from_geojson(tmp_path / "out" / "full.geojson")[0]) == 4
    # without the points: the error as it was, word for word
    with pytest.raises(NotImplementedError, match="^top_down_vector_projection_savefile: the vector export needs geopandas, which is "
                                                  "outside the projection path$"):
        aggregate_images(*args, top_down_vector_projection_savefile="map.geojson", backend=Full(), **kw)
    # bad inputs fail before the aggregation: points without a map, points of the wrong length, another file format
    with pytest.raises(ValueError, match="top_down_points_file is given but"):
        aggregate_images(*args, top_down_points_file=export_points, backend=Full(), **kw)
    with pytest.raises(ValueError, match="top_down_points_file must hold"):
        aggregate_images(*args, top_down_vector_projection_savefile=tmp_path / "x.geojson", top_down_points_file=export_points[:-1],
                         backend=None, **kw)
    with pytest.raises(NotImplementedError, match="geojson"):
        aggregate_images(*args, top_down_vector_projection_savefile=tmp_path / "x.gpkg", top_down_points_file=export_points,
                         backend=None, **kw)
    parsed = parse_args(["--mesh-file", "m.npz", "--mesh-CRS", "EPSG:4978", "--cameras-file", "c.xml", "--image-folder", "i",
                         "--label-folder", "l", "--IDs-to-labels", "ids.json", "--top-down-vector-projection-savefile", "map.geojson",
                         "--top-down-points-file", "p.npy"])
    assert parsed.top_down_points_file == Path("p.npy") and parsed.top_down_vector_projection_savefile == "map.geojson"
    assert parse_args(["--mesh-file", "m.npz", "--mesh-CRS", "EPSG:4978", "--cameras-file", "c.xml", "--image-folder", "i",
                       "--label-folder", "l", "--IDs-to-labels", "ids.json"]).top_down_points_file is None


# -- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_source_name_the_new_call():
    header = (ROOT / "include" / "geograster.h").read_text()
    source = (ROOT / "geograypher_amd" / "csrc" / "polygons.hip").read_text()
    internal = (ROOT / "geograypher_amd" / "csrc" / "gr_internal.hpp").read_text()
    name, n_args = "gr_class_outlines", 16
    decl = re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == n_args == len(_hip._SIGNATURES[name])
    assert name in _hip.EXPORTED_SYMBOLS and re.search(rf"\bint {name}\(gr_ctx \*c,", source)
    definition = re.search(rf"\bint {name}\((gr_ctx \*c,.*?)\) \{{", source, re.S).group(1)
    assert len(definition.split(",")) == n_args
    kernels = ("k_outline_canon", "k_outline_face_edges", "k_outline_cancel", "k_outline_successor", "k_outline_round", "k_outline_emit_rings")
    assert all(k in source and k in internal for k in kernels)
    assert "Scratch stage;" in internal and "Scratch stage_b;" in internal and "meshes/meshes.py:1308-1445" in header
    call = source[source.index(f"int {name}(gr_ctx *c,"):]       # the call has two blocks: one in each arena member
    assert "stage_acquire(c, c->stage, " in call and "stage_acquire(c, c->stage_b, " in call
    assert (_hip.GR_OUTL_STAT_NO_CLASS, _hip.GR_OUTL_STAT_ZERO_AREA, _hip.GR_OUTL_STAT_TURNED, _hip.GR_OUTL_STAT_CANCELLED,
            _hip.GR_OUTL_STAT_MULTI, _hip.GR_OUTL_STAT_BAD_FACES, _hip.GR_OUTL_STAT_WORDS, _hip.GR_OUTL_MAX_CLASSES) == (0, 1, 2, 3, 4, 5, 8, 65535)
    steps = (ROOT / "geograypher_amd" / "csrc" / "cub_steps.hpp").read_text()      # the sorts and scans: steps of cub_steps.hpp
    assert "SortPairs<int64_t, int32_t> sort_vertex(c, pa, V, 64);" in call and "ExclusiveSum<int32_t> scan_flag(c, pa, N3)" in call
    assert "hipcub::DeviceRadixSort::SortPairs(" in steps and "hipcub::DeviceScan::ExclusiveSum(" in steps
    outline_start = source.index("gr_class_outlines: the outline rings")
    outline_part = source[outline_start:source.index('extern "C" {', outline_start)]       # every outline kernel and device helper
    assert all(outline_part.count(k + "(") >= 1 for k in kernels) and "k_outline_ring_words(" in outline_part
    assert not re.search(r"\b(double|float)\b", outline_part)      # no floating point anywhere in the call
    shared = (ROOT / "geograypher_amd" / "csrc" / "geom_dev.hpp").read_text()      # ... nor in the helpers it counts and loads faces with
    assert "stat_count(" in outline_part and "load_face(" in outline_part and '#include "geom_dev.hpp"' in source
    assert "stat_count(" in shared and not re.search(r"\b(double|float)\b", shared)
    assert any(p.name == "polygons.hip" for p in build.SOURCES) and callable(_hip.HipRaster.class_outlines)
    assert callable(TexturedPhotogrammetryMesh.face_label_outlines) and callable(TexturedPhotogrammetryMesh.export_face_labels_vector)


# -- X8 at scale: the candidate search must not be quadratic ---------------------------------------------------------------------------
def noise_rings(side, cell=10_000_000, origin=(0, 0)):
    """One big exterior with side x side cells; every cell holds a small hole, every second hole an island, every fourth island a hole
    of its own: (ring_q, ring_offsets, class index, expected home).  Rings are squares; exteriors counter-clockwise, holes clockwise."""
    def square(x0, y0, x1, y1, hole):
        ring = [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]
        return ring[::-1] if hole else ring

    ox, oy = origin
    rings, home = [square(ox - cell, oy - cell, ox + (side + 1) * cell, oy + (side + 1) * cell, False)], [-1]
    for j in range(side):
        for i in range(side):
            x, y, k = ox + i * cell, oy + j * cell, j * side + i
            rings.append(square(x + 1_000_000, y + 1_000_000, x + 9_000_000, y + 9_000_000, True))
            home.append(0)
            if k % 2 == 0:
                rings.append(square(x + 2_000_000, y + 2_000_000, x + 8_000_000, y + 8_000_000, False))
                home.append(-1)
                if k % 4 == 0:
                    rings.append(square(x + 3_000_000, y + 3_000_000, x + 7_000_000, y + 7_000_000, True))
                    home.append(len(rings) - 2)
    ring_q = np.array([p for ring in rings for p in ring], dtype=np.int64)
    return ring_q, np.arange(len(rings) + 1, dtype=np.int64) * 4, np.zeros(len(rings), dtype=np.int64), home


def test_X8_search_is_not_quadratic(monkeypatch):
    # the same answer as the brute-force stand-in on a small field, also far from the origin (Python-integer products)
    for origin in ((0, 0), (2 ** 40 - 10 ** 9, -(2 ** 40) + 10 ** 7)):
        ring_q, off, cls, home = noise_rings(6, origin=origin)
        got = {"ring_vertices": np.arange(len(ring_q)), "ring_offsets": off, "ring_class": cls}
        want_areas2, want_home = osn.nest_np(ring_q, got)
        areas2, found = geometric.nest_outline_rings(ring_q, off, cls)
        assert areas2 == want_areas2 and found.tolist() == want_home == home
    # 60 x 60 cells: 3600 + 900 holes against 1801 exteriors; exact tests stay near one per hole, far from holes x exteriors
    ring_q, off, cls, home = noise_rings(60)
    calls = []
    real = geometric._RingLocator.contains
    monkeypatch.setattr(geometric._RingLocator, "contains", lambda self, px, py: calls.append(1) or real(self, px, py))
    areas2, found = geometric.nest_outline_rings(ring_q, off, cls)
    n_holes = sum(a < 0 for a in areas2)
    assert found.tolist() == home and n_holes == 4500 and len(calls) <= 8 * n_holes
    # a class of its own is searched on its own: the same rings under another class index find no home there
    other = cls.copy()
    other[1::7] = 1
    _, split = geometric.nest_outline_rings(ring_q, off, other, areas2=areas2)
    assert all(h < 0 or other[h] == other[r] for r, h in enumerate(split.tolist()))
