"""Vector textures without a GPU (DESIGN.md "Vector textures"): the rules on a hand-worked scene, the cell-table builder against
brute force, the per-column values (V6), the GeoJSON reader, `determine_IDs_to_labels` / `remap_texture` / `load_texture` against
the reference's own answers (tests/golden/reference_vector_texture.npz, made by tests/golden/make_golden_vector_texture.py), the
`render_labels` entry point end to end on the CPU stand-ins, and the C ABI of the new call."""
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import vector_standin as vs  # noqa: E402
from geograypher_amd import _hip, build  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMesh, TexturedPhotogrammetryMeshChunked  # noqa: E402
from geograypher_amd.utils import geometric, synthetic  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons, polygon_cell_table  # noqa: E402
from geograypher_amd.utils.indexing import determine_IDs_to_labels  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "reference_vector_texture.npz"


def hand_mesh(backend=None):
    polygons, cases = vs.hand_scene()
    verts, faces = vs.centred_faces([c for c, _, _ in cases])
    points = np.column_stack([verts, np.linspace(0.0, 5.0, len(verts))])
    mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=backend or vs.StandInBackend())
    return mesh, points, polygons, np.array([row for _, row, _ in cases], dtype=np.int32)


# -- the rules on the hand-worked scene ------------------------------------------------------------------------------------------
def test_hand_worked_scene_every_value_written_out():
    mesh, points, polygons, want = hand_mesh()
    got = mesh.face_polygon_index(polygons, points_in_polygon_CRS=points)
    assert got.dtype == np.int32 and got.tolist() == want.tolist()
    assert want.tolist() == [0, -1, 0, 0, 0, 0, 1, 1, 1, 1, -1, -1, 3, 3, 3, -1, -1, -1, -1, 2, 2, 2, -1]
    assert mesh.last_vector_stats["faces_labelled"] == 15 and mesh.last_vector_stats["pairs_tested"] >= 15
    # what the backend was handed: snapped vertices behind one origin, int32 faces, the ring table, a cell table that fits it
    last = mesh.backend.last
    assert last["verts_q"].dtype == np.int64 and last["verts_q"].shape == (len(points), 2) and last["faces"].dtype == np.int32
    grid, offsets, rows = last["cell_table"]
    assert len(offsets) == grid[4] * grid[5] + 1 and offsets[-1] == len(rows)
    # a zero-area face still has a centre
    flat = TexturedPhotogrammetryMesh((np.array([[1.0, 1, 0], [2, 2, 0], [3, 3, 0], [50, 50, 0.0]]), np.array([[0, 1, 2]])),
                                      log_level="ERROR", backend=vs.StandInBackend())
    assert flat.face_polygon_index(polygons, points_in_polygon_CRS=flat.points).tolist() == [0]


def test_inputs_that_raise():
    mesh, points, polygons, _ = hand_mesh()
    with pytest.raises(NotImplementedError, match="points_in_polygon_CRS"):
        mesh.face_polygon_index(polygons)
    with pytest.raises(NotImplementedError, match="geopandas"):
        mesh.face_polygon_index("crowns.gpkg", points_in_polygon_CRS=points)
    with pytest.raises(ValueError, match="points_in_polygon_CRS must be"):
        mesh.face_polygon_index(polygons, points_in_polygon_CRS=points[:-1])
    far = points.copy()
    far[0, 0] = 3.0e6
    with pytest.raises(ValueError, match="2\\^40"):
        mesh.face_polygon_index(polygons, points_in_polygon_CRS=far)
    with pytest.raises(NotImplementedError, match="geojson"):
        mesh.get_values_for_faces_from_vector("crowns.shp", "species", points_in_polygon_CRS=points)


# -- the cell table --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [None, "one", "fine"])
def test_cell_table_against_brute_force(grid):
    verts, _, polygons = vs.random_scene(n_faces=30, n_polygons=120)
    boxes = vs.snapped_scene(verts, polygons)[1][4]
    boxes[7] = [1, 1, 0, 0]   # a row without rings
    if grid == "one":
        grid = [-(1 << 43), -(1 << 43), 1 << 44, 1 << 44, 1, 1]
    elif grid == "fine":
        grid = [int(3 * boxes[:, 0].min()) + 1000, int(3 * boxes[:, 1].min()), 3_000_001, 1_700_000, 23, 40]   # cuts some boxes off
    g, offsets, rows = polygon_cell_table(boxes, grid=grid)
    x0, y0, cw, ch, nx, ny = (int(v) for v in g)
    assert offsets.dtype == np.int64 and rows.dtype == np.int32 and offsets[0] == 0 and offsets[-1] == len(rows)
    for iy in range(ny):
        for ix in range(nx):
            lo_x, lo_y = x0 + ix * cw, y0 + iy * ch
            meets = [p for p, b in enumerate(3 * boxes) if b[0] <= b[2] and b[0] <= lo_x + cw - 1 and b[2] >= lo_x
                     and b[1] <= lo_y + ch - 1 and b[3] >= lo_y]
            cell = iy * nx + ix
            assert rows[offsets[cell]:offsets[cell + 1]].tolist() == sorted(meets, reverse=True), (ix, iy)
    if grid is None:   # the chosen grid covers the closed bounds and spends a bounded number of entries
        live = 3 * boxes[boxes[:, 0] <= boxes[:, 2]]
        assert x0 == live[:, 0].min() and x0 + nx * cw > live[:, 2].max() and y0 + ny * ch > live[:, 3].max()
        assert nx * ny > 1 and len(rows) <= max(geometric.CELL_LIST_BUDGET * len(live), 4096)


def test_chosen_grid_stays_small_under_polygons_that_span_everything():
    small = [[i, j, i + 1, j + 1] for i in range(0, 400, 2) for j in range(0, 40, 2)]
    boxes = np.array(small + [[0, 0, 400, 40]] * 40, dtype=np.int64) * 1_000_000
    grid, offsets, rows = polygon_cell_table(boxes)
    assert len(rows) <= max(geometric.CELL_LIST_BUDGET * len(boxes), 4096)
    assert polygon_cell_table(np.zeros((0, 4), dtype=np.int64))[0].tolist() == [0, 0, 1, 1, 1, 1]
    with pytest.raises(ValueError, match="cell grid"):
        polygon_cell_table(boxes, grid=[0, 0, 0, 1, 1, 1])


# -- V6: values per column -------------------------------------------------------------------------------------------------------
def test_values_nulls_and_dtypes_one_column_and_several():
    mesh, points, polygons, want = hand_mesh()
    columns = {"species": np.array(["oak", "fir", "ash", "elm"], dtype=object), "crown": np.array([11, 12, 13, 14], dtype=np.int64),
               "height": np.array([1.5, 2.5, 3.5, 4.5])}
    inside = want >= 0
    species, all_species = mesh.get_values_for_faces_from_vector((polygons, columns), "species", points_in_polygon_CRS=points)
    assert species.dtype == object and all_species is not None and all_species.tolist() == ["oak", "fir", "ash", "elm"]
    assert species[inside].tolist() == columns["species"][want[inside]].tolist() and set(species[~inside]) == {"null"}
    assert species[:7].tolist() == ["oak", "null", "oak", "oak", "oak", "oak", "fir"]
    crown, _ = mesh.get_values_for_faces_from_vector((polygons, columns), ["crown"], points_in_polygon_CRS=points)
    assert crown.dtype == np.int64 and crown[inside].tolist() == (want[inside] + 11).tolist() and set(crown[~inside]) == {0}
    height, _ = mesh.get_values_for_faces_from_vector((polygons, columns), "height", points_in_polygon_CRS=points)
    assert height.dtype == np.float64 and np.all(np.isnan(height[~inside])) and height[inside].tolist() == (want[inside] + 1.5).tolist()
    faces_d, all_d = mesh.get_values_for_faces_from_vector((polygons, columns), ["crown", "species"], points_in_polygon_CRS=points)
    assert list(faces_d) == ["crown", "species"] == list(all_d)
    assert np.array_equal(faces_d["crown"], crown) and faces_d["species"].tolist() == species.tolist()
    # fixed-width strings come back as objects: "null" is not cut to the column's width
    short, _ = mesh.get_values_for_faces_from_vector((polygons, {"s": np.array(["a", "b", "c", "d"])}), None, points_in_polygon_CRS=points)
    assert short.dtype == object and short[1] == "null" and short[0] == "a"
    with pytest.raises(ValueError, match="No column name provided and ambigious which column to use"):
        mesh.get_values_for_faces_from_vector((polygons, columns), None, points_in_polygon_CRS=points)
    with pytest.raises(ValueError, match="4 polygons"):
        mesh.get_values_for_faces_from_vector((polygons, {"s": np.arange(3)}), "s", points_in_polygon_CRS=points)


# -- GeoJSON -----------------------------------------------------------------------------------------------------------------------
def _ring(a):
    return [list(map(float, p)) for p in a] + [list(map(float, a[0]))]


def write_hand_geojson(path):
    sq = vs.square
    features = [
        {"type": "Feature", "properties": {"species": "oak", "crown": 11, "height": 1.5, "mixed": 1},
         "geometry": {"type": "Polygon", "coordinates": [_ring(sq(0, 0, 10, 10)), _ring(sq(3, 3, 7, 7))]}},
        {"type": "Feature", "properties": {"species": "fir", "crown": 12, "height": 2, "mixed": "x"},
         "geometry": {"type": "Polygon", "coordinates": [_ring(sq(8, 8, 14, 14))]}},
        {"type": "Feature", "properties": {"species": "rock", "crown": 99, "height": 0.5, "mixed": None},
         "geometry": {"type": "Point", "coordinates": [1.5, 1.5]}},
        {"type": "Feature", "properties": {"species": "ash", "crown": 13, "height": 3.5, "mixed": 2.5},
         "geometry": {"type": "MultiPolygon", "coordinates": [[_ring(sq(20, 0, 24, 4))], [_ring(sq(26, 0, 30, 4))]]}},
    ]
    Path(path).write_text(json.dumps({"type": "FeatureCollection", "features": features}))


def test_from_geojson_rows_are_feature_numbers(tmp_path):
    write_hand_geojson(tmp_path / "crowns.geojson")
    polygons, props = PlanarPolygons.from_geojson(tmp_path / "crowns.geojson")
    assert len(polygons) == 4 and polygons.ring_polygon.tolist() == [0, 0, 1, 3, 3]
    assert polygons.ring_is_hole.tolist() == [False, True, False, False, False]
    assert all(len(r) == 4 for r in polygons.rings)   # the closing vertex is dropped
    assert props["species"].dtype == object and props["crown"].dtype == np.int64 and props["height"].dtype == np.float64
    assert props["mixed"].dtype == object and props["mixed"].tolist() == [1, "x", None, 2.5]
    assert props["height"].tolist() == [1.5, 2.0, 0.5, 3.5]
    # the Point feature keeps row 2 and holds nothing: (1.5, 1.5) is row 0's, the two-part feature is row 3
    verts, faces = vs.centred_faces([(1.5, 1.5), (5, 5), (9, 9), (22, 2), (28, 2), (25, 2)])
    points = np.column_stack([verts, np.zeros(len(verts))])
    mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=vs.StandInBackend())
    crown, all_values = mesh.get_values_for_faces_from_vector(tmp_path / "crowns.geojson", "crown", points_in_polygon_CRS=points)
    assert crown.tolist() == [11, 0, 12, 13, 13, 0] and all_values.tolist() == [11, 12, 99, 13]
    (tmp_path / "not.geojson").write_text(json.dumps({"type": "Feature"}))
    with pytest.raises(ValueError, match="FeatureCollection"):
        PlanarPolygons.from_geojson(tmp_path / "not.geojson")


# -- IDs_to_labels, remap_texture, load_texture against the reference ----------------------------------------------------------------
def _golden_case(z, case):
    texture = z[f"{case}/texture"]
    if texture.dtype.kind == "U":
        texture = texture.astype(object)
    all_values = z[f"{case}/all_values"].astype(object) if f"{case}/all_values" in z.files else None
    background_ID = int(z[f"{case}/background_ID"]) if f"{case}/background_ID" in z.files else None
    given = None
    if f"{case}/given_ids" in z.files:
        given = {int(k): str(v) for k, v in zip(z[f"{case}/given_ids"], z[f"{case}/given_labels"])}
    table = None if bool(z[f"{case}/is_none"]) else dict(zip(z[f"{case}/ids"].tolist(), z[f"{case}/labels"].tolist()))
    return texture, all_values, background_ID, given, table


def _golden_cases(prefix):
    with np.load(GOLDEN) as z:
        return sorted({k.split("/")[0] for k in z.files if k.startswith(prefix)})


@pytest.mark.parametrize("case", _golden_cases("det_"))
def test_determine_IDs_to_labels_like_the_reference(case):
    with np.load(GOLDEN) as z:
        texture, all_values, background_ID, _, want = _golden_case(z, case)
    got = determine_IDs_to_labels(texture, all_discrete_texture_values=all_values, background_ID=background_ID)
    if want is None:
        assert got is None
    else:
        assert list(got) == list(want)
        got_labels, want_labels = np.array(list(got.values())), np.array(list(want.values()))
        if want_labels.dtype.kind == "f":   # (a NaN among the values is a label of its own, as in the reference)
            assert np.array_equal(got_labels.astype(np.float64), want_labels, equal_nan=True)
        else:
            assert got_labels.tolist() == want_labels.tolist()


@pytest.mark.parametrize("case", _golden_cases("remap_"))
def test_remap_texture_and_load_texture_like_the_reference(case):
    with np.load(GOLDEN) as z:
        texture, all_values, background_ID, given, want = _golden_case(z, case)
        remapped = z[f"{case}/remapped"]
    n = len(texture)
    mesh = TexturedPhotogrammetryMesh((np.zeros((n + 2, 3)), np.zeros((n, 3), dtype=np.int64)), log_level="ERROR",
                                      backend=vs.StandInBackend())
    mesh.IDs_to_labels = "untouched"
    got = mesh.remap_texture(texture, IDs_to_labels=given, all_discrete_texture_values=all_values, background_ID=background_ID)
    assert got.shape == remapped.shape and np.array_equal(np.asarray(got, dtype=np.float64), remapped, equal_nan=True)
    assert mesh.IDs_to_labels == want and (want is None or list(mesh.IDs_to_labels) == list(want))
    if all_values is None:   # load_texture is remap_texture + set_texture for an array
        mesh.IDs_to_labels = "untouched"
        mesh.load_texture(texture, IDs_to_labels=given, background_ID=background_ID)
        assert mesh.IDs_to_labels == want and mesh.vertex_texture is None
        assert np.array_equal(np.asarray(mesh.face_texture, dtype=np.float64), remapped, equal_nan=True)


def test_remap_texture_errors_and_load_texture_sources(tmp_path):
    mesh, points, polygons, want = hand_mesh()
    with pytest.raises(ValueError, match="one-to-one"):
        mesh.remap_texture(np.array(["a", "b"], dtype=object), IDs_to_labels={0: "a", 1: "a"})
    with pytest.raises(ValueError, match="only ints"):
        mesh.remap_texture(np.array(["a", "b"], dtype=object), IDs_to_labels={0.5: "a", 1: "b"})
    mesh.remap_texture(np.array([1, 2]), update_IDs_to_labels=False)
    assert mesh.IDs_to_labels is None
    # None only sets the table; .npy; .geojson (species strings -> IDs over ALL the file's values); anything else is a raster
    mesh.load_texture(None, IDs_to_labels={0: "a"})
    assert mesh.IDs_to_labels == {0: "a"} and mesh.face_texture is None
    np.save(tmp_path / "tex.npy", (want + 1).astype(np.int64))
    mesh.load_texture(tmp_path / "tex.npy")
    assert mesh.face_texture[:, 0].tolist() == (want + 1).tolist() and mesh.IDs_to_labels == {i: i for i in range(5)}
    write_hand_geojson(tmp_path / "crowns.geojson")
    verts, faces = vs.centred_faces([(1.5, 1.5), (5, 5), (9, 9), (22, 2)])
    pts = np.column_stack([verts, np.zeros(len(verts))])
    m2 = TexturedPhotogrammetryMesh((pts, faces), log_level="ERROR", backend=vs.StandInBackend())
    m2.load_texture(tmp_path / "crowns.geojson", texture_column_name="species", points_in_polygon_CRS=pts)
    assert m2.IDs_to_labels == {0: "ash", 1: "fir", 2: "oak", 3: "rock"}
    assert np.array_equal(m2.face_texture[:, 0], [2.0, np.nan, 1.0, 0.0], equal_nan=True)   # "null" has no ID: NaN
    with pytest.raises(NotImplementedError, match="points_in_polygon_CRS"):
        m2.load_texture(tmp_path / "crowns.geojson", texture_column_name="species")
    with pytest.raises(NotImplementedError, match="raster"):
        m2.load_texture(tmp_path / "dtm.tif")
    # the constructor keeps its behaviour: same exception for a vector file
    with pytest.raises(NotImplementedError, match="only .npy texture files"):
        TexturedPhotogrammetryMesh((pts, faces), texture=tmp_path / "crowns.geojson", log_level="ERROR", backend=vs.StandInBackend())


# -- the entry point ---------------------------------------------------------------------------------------------------------------
def test_render_labels_end_to_end_on_the_stand_ins(tmp_path, oracle_backend_cls):
    from PIL import Image

    from geograypher_amd.entrypoints.render_labels import render_labels

    class Backend(vs.StandInBackend, oracle_backend_cls):
        pass

    (points, faces), cams = synthetic.config1_scene()
    sub = cams[0:2]
    for i, c in enumerate(sub.cameras):
        c.image_filename = Path(tmp_path, "images", "flight", f"img_{i}.JPG")
    sub.image_folder = Path(tmp_path, "images")
    np.savez(tmp_path / "mesh.npz", points=points, faces=faces)
    np.save(tmp_path / "points_utm.npy", points)
    lo, hi = points[:, :2].min(axis=0), points[:, :2].max(axis=0)
    mid = (lo + hi) / 2
    features = [{"type": "Feature", "properties": {"species": name},
                 "geometry": {"type": "Polygon", "coordinates": [_ring(vs.square(*a, *b))]}}
                for name, a, b in (("oak", lo, mid), ("fir", mid, hi), ("ash", lo + (hi - lo) * [0.4, 0.4], lo + (hi - lo) * [0.6, 0.6]))]
    (tmp_path / "crowns.geojson").write_text(json.dumps({"type": "FeatureCollection", "features": features}))
    out = tmp_path / "renders"
    mesh = render_labels(tmp_path / "mesh.npz", None, tmp_path / "images", tmp_path / "crowns.geojson", out, "EPSG:4978",
                         texture_column_name="species", render_image_scale=0.25, n_cameras_per_chunk=1,
                         texture_points_file=tmp_path / "points_utm.npy", apply_distortion=False, camera_set=sub, backend=Backend())
    assert isinstance(mesh, TexturedPhotogrammetryMeshChunked)
    assert json.loads((out / "IDs_to_labels.json").read_text()) == {"0": "ash", "1": "fir", "2": "oak"}
    h, w = sub.cameras[0].get_image_size()
    for i in range(2):
        img = np.asarray(Image.open(out / "flight" / f"img_{i}.tif"))
        assert img.dtype == np.uint8 and img.shape == (h, w) and set(np.unique(img)) <= {0, 1, 2}
    # the texture the renders were made from: the highest feature wins in the overlap, faces outside every feature have no ID
    index = mesh.face_polygon_index(PlanarPolygons.from_geojson(tmp_path / "crowns.geojson")[0], points_in_polygon_CRS=points)
    want = np.where(index >= 0, np.array([2.0, 1.0, 0.0])[np.maximum(index, 0)], np.nan)
    assert np.array_equal(mesh.face_texture[:, 0], want, equal_nan=True) and {0, 1, 2} <= set(index.tolist())
    for kw in ({"DTM_file": "dtm.tif"}, {"ROI": "roi.geojson"}, {"mesh_downsample": 0.5}, {"vis": True},
               {"mesh_vis_file": "m.png"}, {"labels_vis_folder": "v"}):
        with pytest.raises(NotImplementedError):
            render_labels(tmp_path / "mesh.npz", None, tmp_path / "images", np.zeros(len(faces)), out, "EPSG:4978", camera_set=sub,
                          backend=Backend(), **kw)


# -- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_source_name_the_new_call():
    header = (ROOT / "include" / "geograster.h").read_text()
    decl = re.search(r"\bint gr_face_polygon_index\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == 24 == len(_hip._SIGNATURES["gr_face_polygon_index"])
    assert "gr_face_polygon_index" in _hip.EXPORTED_SYMBOLS and "#define GR_VERSION 126" in header
    assert "meshes/meshes.py:990-1079" in header and "GR_FPI_STAT_BAD_FACES" in header
    assert (_hip.GR_FPI_STAT_TESTED, _hip.GR_FPI_STAT_LABELLED, _hip.GR_FPI_STAT_LONGEST_LIST, _hip.GR_FPI_STAT_BAD_FACES,
            _hip.GR_FPI_STAT_WORDS) == (0, 1, 2, 3, 4)
    source = (ROOT / "geograypher_amd" / "csrc" / "polygons.hip").read_text()
    assert re.search(r"\bint gr_face_polygon_index\(gr_ctx \*c,", source) and "k_face_polygon_index" in source
    assert any(p.name == "polygons.hip" for p in build.SOURCES)
    assert "k_face_polygon_index" in (ROOT / "geograypher_amd" / "csrc" / "gr_internal.hpp").read_text()
    assert callable(_hip.HipRaster.face_polygon_index)
