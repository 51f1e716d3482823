"""CRS reprojection on the host (DESIGN.md "CRS reprojection"): the numpy stand-in of tests/crs_standin.py against the mpmath oracle
of tests/golden/crs_wgs84.npz, and the Python surface -- designators, axis order, the mesh and camera methods, the
`points_in_*_CRS` keywords, the entry points' flags -- driven through the stand-in backend."""
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))

import crs_standin as cs  # noqa: E402
import outline_standin  # noqa: E402
import polygon_standin  # noqa: E402
import raster_standin  # noqa: E402
import region_standin  # noqa: E402
import vector_standin  # noqa: E402
from geograypher_amd.cameras.cameras import PhotogrammetryCamera, PhotogrammetryCameraSet  # noqa: E402
from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import geospatial  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons  # noqa: E402
from geograypher_amd.utils.geospatial import WGS84CRS  # noqa: E402
from geograypher_amd.utils.raster import PlanarRaster  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
UTM10 = "EPSG:32610"


class Backend(cs.CrsStandinBackend, region_standin.StandInBackend, vector_standin.StandInBackend, raster_standin.StandInBackend,
              polygon_standin.StandInBackend, outline_standin.StandInBackend):
    pass


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.fixture(scope="module")
def golden():
    return cs.load_golden()


@pytest.fixture(scope="module")
def scene():
    """The UTM grid lifted onto the ellipsoid by the stand-in: (mesh in ECEF, its vertices back in UTM: the stand-in's array)."""
    utm, faces = cs.utm_grid_scene()
    ecef, status = cs.reproject(utm, (cs.TM, -123.0, 0.9996, 500000.0, 0.0), (cs.ECEF, 0, 1, 0, 0))
    assert not status.any()
    mesh = TexturedPhotogrammetryMesh((ecef, faces), backend=Backend(), log_level="ERROR")
    array, _ = cs.reproject(ecef, (cs.ECEF, 0, 1, 0, 0), (cs.TM, -123.0, 0.9996, 500000.0, 0.0))
    assert np.abs(array - utm).max() < 1e-7
    array.setflags(write=False)
    return mesh, array, utm


# -- the stand-in against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", cs.PAIRS)
def test_standin_within_twice_its_recorded_error(golden, src, dst):
    bound = cs.bounds(golden, 2.0)
    assert (golden["standin_err_m"] > 0).all() and (golden["standin_err_m"] < 1e-8).all()   # a few 1e-9 m: what float64 gives
    for g in range(len(golden["tm_params"])):
        rows = np.nonzero(golden["group"] == g)[0]
        got, status = cs.reproject(golden[f"in_{src}"][rows], cs.golden_crs(golden, src, g), cs.golden_crs(golden, dst, g))
        flag = golden[f"flag_{src}_{dst}"][rows]
        assert same(status, flag) and same(np.isnan(got).all(axis=1), flag != 0) and same(np.isnan(got).any(axis=1), flag != 0)
        assert (cs.worst_errors(got, golden[f"exp_{src}_{dst}"][rows], dst, from_ecef=src == "ecef") <= bound).all()


def test_golden_covers_the_edges(golden):
    geo, group, prm = golden["in_geo"], golden["group"], golden["tm_params"]
    dlon = (geo[:, 0] - prm[group, 0] + 180.0) % 360.0 - 180.0
    assert 200 <= len(geo) <= 400
    assert (geo[:, 1] == 0).any() and (dlon == 0).sum() > 10 and {80.0, -80.0, 84.0, -84.0, 90.0, -90.0} <= set(geo[:, 1])
    assert {3.0, 6.0, 20.0} <= set(np.abs(dlon).round(9)) and (geo[:, 2] < 0).any()
    assert (prm[:, 3] == 10000000.0).any() and {-177.0, 177.0} <= set(prm[:, 0])   # a southern zone, zones 1 and 60
    for g, lon0 in ((2, -177.0), (3, 177.0)):   # both sides of the antimeridian in one zone
        lons = geo[(group == g) & (golden["flag_geo_tm"] == 0), 0]
        assert (lons > 0).any() and (lons < 0).any()
    assert (golden["flag_geo_tm"] == 2).sum() >= 6 and (golden["flag_ecef_tm"] == 1).sum() >= 2
    assert (np.abs(golden["in_ecef"]).sum(axis=1) == 0).sum() == 1   # the origin
    assert ((golden["in_ecef"][:, :2] == 0).all(axis=1) & (golden["in_ecef"][:, 2] != 0)).sum() >= 4   # the axis
    # the published position the oracle was checked against
    i = int(np.nanargmin(np.abs(geo[:, 1] - (43 + 38 / 60 + 33.24 / 3600)) + np.abs(geo[:, 0] + (79 + 23 / 60 + 13.7 / 3600))))
    assert abs(golden["exp_geo_tm"][i, 0] - 630084.31) < 0.25 and abs(golden["exp_geo_tm"][i, 1] - 4833438.55) < 0.25


def test_header_constants_are_the_goldens_to_the_last_bit(golden):
    import make_crs_constants as consts

    header = consts.read_header()
    assert len(header) == 13 and [float(v).hex() for v in header] == [float(v).hex() for v in golden["constants"]]
    assert header == [cs.RECT_RADIUS] + cs.ALPHA + cs.BETA
    # the issue's 30-digit figures, as a cross-check of the tool (not its source)
    quoted = [6367449.1458234153093, 8.3773182062446983e-4, 7.6085277735724892e-7, 1.1976455032424921e-9, 2.4291706803973132e-12,
              5.7118183691541053e-15, 1.4799980270526193e-17, 8.3773216405794868e-4, 5.9058701522203652e-8, 1.6734826653438249e-10,
              2.1647981104903862e-13, 3.7879309688396013e-16, 7.2367692879656038e-19]
    assert np.allclose(header, quoted, rtol=1e-12, atol=1e-30)
    mp = pytest.importorskip("mpmath")
    with mp.workdps(30):
        A = consts.rectifying_radius(mp)
        assert float(A) == header[0] and float(consts.alpha(mp, 1, A)) == header[1] and float(consts.beta(mp, 1, A)) == header[7]


# -- designators -----------------------------------------------------------------------------------------------------------------------
def test_designators_and_refusals():
    assert WGS84CRS.parse("EPSG:4978") == WGS84CRS.parse(4978) == WGS84CRS.parse(" epsg:4978 ") and WGS84CRS.parse(4978).kind == 0
    for code in (4326, 4979):
        c = WGS84CRS.parse(f"EPSG:{code}")
        assert c.kind == 1 and c.lat_first and c.epsg == code
    north, south = WGS84CRS.parse("EPSG:32610"), WGS84CRS.parse(np.int64(32733))
    assert (north.kind, north.lon0, north.k0, north.false_easting, north.false_northing, north.lat_first) == \
        (2, -123.0, 0.9996, 500000.0, 0.0, False)
    assert (south.lon0, south.false_northing, south.epsg) == (15.0, 10000000.0, 32733) and str(south) == "EPSG:32733"
    assert WGS84CRS.parse(32601).lon0 == -177.0 and WGS84CRS.parse(32660).lon0 == 177.0 and WGS84CRS.parse(32760).lon0 == 177.0
    assert WGS84CRS.parse(north) is north and WGS84CRS.utm(10) == north
    tm = WGS84CRS.transverse_mercator(12.5, 1.0, 0.0, -5000000.0)
    assert geospatial.crs_tuple(tm) == (2, 12.5, 1.0, 0.0, -5000000.0) and tm.epsg is None
    for bad in ("EPSG:26910", 26910, "EPSG:3857", "EPSG:32661", "EPSG:32600", 32761, "EPSG:32700", "WGS 84", None, 4978.0, True):
        with pytest.raises(NotImplementedError, match="pyproj"):
            WGS84CRS.parse(bad)
    with pytest.raises(ValueError, match="k0 > 0"):
        WGS84CRS.transverse_mercator(0.0, 0.0)
    with pytest.raises(ValueError, match="1 ... 60"):
        WGS84CRS.utm(61)
    assert geospatial.is_CRS_designator("EPSG:32610") and geospatial.is_CRS_designator(32610) and geospatial.is_CRS_designator(tm)
    assert not geospatial.is_CRS_designator(np.zeros((3, 3))) and not geospatial.is_CRS_designator(None)


def test_get_projected_CRS():
    assert geospatial.get_projected_CRS(37.8, -122.3) == 32610          # San Francisco: (183 - 122.3) / 6 = 10.1
    assert geospatial.get_projected_CRS(-33.9, 18.4, assume_western_hem=False) == 32734   # Cape Town: 201.4 / 6 = 33.6
    assert geospatial.get_projected_CRS(-33.9, 18.4) == 32727           # flipped to 18.4 W: 164.6 / 6 = 27.4
    assert geospatial.get_projected_CRS(43.64, -79.39) == 32617         # the landmark of the golden file
    assert geospatial.get_projected_CRS(46.0, 9.0, assume_western_hem=False) == 32632 and isinstance(geospatial.get_projected_CRS(1, 1), int)


def test_axis_order_and_convert_CRS_3D_points(scene):
    mesh, array, utm = scene
    backend = mesh.backend
    lon_lat = mesh.get_mesh_points_in_CRS("EPSG:4326", use_vertices=True)
    lat_lon = mesh.get_mesh_points_in_CRS("EPSG:4326", use_vertices=True, force_easting_northing=False)
    assert same(lat_lon, lon_lat[:, [1, 0, 2]]) and (np.abs(lon_lat[:, 0] + 122.41) < 0.01).all() and (np.abs(lon_lat[:, 1] - 37.78) < 0.01).all()
    assert same(mesh.reproject_CRS(4979), lat_lon) and same(mesh.reproject_CRS(UTM10), array)
    for force in (True, False):   # a projected CRS is easting first either way
        assert same(mesh.get_mesh_points_in_CRS(UTM10, use_vertices=True, force_easting_northing=force), array)
    with pytest.raises(NotImplementedError, match="EPSG:4978"):
        mesh.reproject_CRS(UTM10, inplace=True)
    # pyproj's contract: both sides in the authority's order
    assert same(geospatial.convert_CRS_3D_points(mesh.points, "EPSG:4978", "EPSG:4326", backend=backend), lat_lon)
    back = geospatial.convert_CRS_3D_points(lat_lon, "EPSG:4326", UTM10, backend=backend)
    assert np.abs(back - utm).max() < 1e-7
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        geospatial.convert_CRS_3D_points(np.zeros((4, 2)), 4978, 4326, backend=backend)
    assert mesh.last_reproject_stats == {"nonfinite": 0, "beyond_central_meridian": 0, "bad_faces": 0}


def test_face_centres_are_the_mean_of_the_reprojected_vertices(scene):
    mesh, array, _ = scene
    corners = array[mesh.faces]
    want = ((corners[:, 0] + corners[:, 1]) + corners[:, 2]) / 3.0
    assert same(mesh.get_mesh_points_in_CRS(UTM10), want) and want.shape == (len(mesh.faces), 3)
    out, status = cs.reproject_faces(mesh.points, [[0, 1, len(mesh.points)], [0, 1, 2]], (0, 0, 1, 0, 0), (2, -123.0, 0.9996, 5e5, 0.0))
    assert status.tolist() == [cs.BAD_FACE, cs.OK] and np.isnan(out[0]).all() and same(out[1], ((array[0] + array[1]) + array[2]) / 3.0)
    no_crs = TexturedPhotogrammetryMesh((array, mesh.faces), input_CRS=None, backend=Backend(), log_level="ERROR")
    assert same(no_crs.get_mesh_points_in_CRS(UTM10), want) and same(no_crs.get_mesh_points_in_CRS(UTM10, use_vertices=True), array)


# -- the points_in_*_CRS keywords ------------------------------------------------------------------------------------------------------
SQUARES = [np.array([[x, y], [x + 25, y], [x + 25, y + 25], [x, y + 25]], dtype=np.float64) + (552000.0, 4182000.0)
           for x, y in ((2.0, 3.0), (30.0, 31.0), (20.0, 20.0))]
DTM = PlanarRaster(np.full((8, 8), 12.0, dtype=np.float32), (10.0, 0.0, 551990.0, 0.0, -10.0, 4182070.0), nodata=-9999.0)


def _keyword_calls(mesh):
    polygons = PlanarPolygons.from_sequence(SQUARES)
    labels = (np.arange(len(mesh.faces)) % 3).astype(np.float64)
    return {
        "select_mesh_ROI": ("points_in_ROI_CRS", lambda p: mesh.select_mesh_ROI([SQUARES[0]], buffer_meters=1.5, return_original_IDs=True,
                                                                                points_in_ROI_CRS=p)),
        "label_polygon_weights": ("points_in_polygon_CRS", lambda p: mesh.label_polygon_weights(labels, polygons, points_in_polygon_CRS=p)),
        "label_polygons": ("points_in_polygon_CRS", lambda p: mesh.label_polygons(labels, polygons, points_in_polygon_CRS=p)),
        "face_polygon_index": ("points_in_polygon_CRS", lambda p: mesh.face_polygon_index(polygons, points_in_polygon_CRS=p)),
        "get_values_for_faces_from_vector": ("points_in_polygon_CRS", lambda p: mesh.get_values_for_faces_from_vector(
            (polygons, {"k": np.array([5, 6, 7])}), "k", points_in_polygon_CRS=p)),
        "face_label_outlines": ("points_in_export_CRS", lambda p: mesh.face_label_outlines(labels, points_in_export_CRS=p).ring_xy),
        "get_values_from_raster_file": ("points_in_raster_CRS", lambda p: mesh.get_values_from_raster_file(
            DTM, return_mesh_points=True, points_in_raster_CRS=p)),
        "get_height_above_ground": ("points_in_raster_CRS", lambda p: mesh.get_height_above_ground(DTM, points_in_raster_CRS=p)),
        "label_ground_class": ("points_in_raster_CRS", lambda p: mesh.label_ground_class(
            DTM, height_above_ground_threshold=9.0, labels=labels.copy(), ground_ID=np.nan, points_in_raster_CRS=p)),
    }


def _flat(result):
    if isinstance(result, (tuple, list)):
        return [x for r in result for x in _flat(r)]
    if isinstance(result, dict):
        return [x for k in sorted(result) for x in _flat(result[k])]
    return [np.asarray(result)]


@pytest.mark.parametrize("name", ["select_mesh_ROI", "label_polygon_weights", "label_polygons", "face_polygon_index",
                                  "get_values_for_faces_from_vector", "face_label_outlines", "get_values_from_raster_file",
                                  "get_height_above_ground", "label_ground_class"])
def test_every_points_keyword_takes_a_designator(scene, name):
    mesh, array, _ = scene
    keyword, call = _keyword_calls(mesh)[name]
    want = _flat(call(array))
    assert any(w.size for w in want)
    for designator in (UTM10, 32610, WGS84CRS.utm(10)):
        got = _flat(call(designator))
        assert len(got) == len(want) and all(same(a, b) for a, b in zip(got, want)), designator
    with pytest.raises(NotImplementedError, match=keyword):   # None: as before
        call(None)
    with pytest.raises(ValueError, match=f"{keyword} must be"):   # arrays keep their checks
        call(array[:-1])
    with pytest.raises(NotImplementedError, match="pyproj"):
        call("EPSG:26910")


def test_the_constructors_ROI_takes_a_designator(scene):
    mesh, array, _ = scene
    by_array = TexturedPhotogrammetryMesh((mesh.points, mesh.faces), backend=Backend(), log_level="ERROR", ROI=[SQUARES[0]],
                                          ROI_buffer_meters=1.5, points_in_ROI_CRS=array)
    by_name = TexturedPhotogrammetryMesh((mesh.points, mesh.faces), backend=Backend(), log_level="ERROR", ROI=[SQUARES[0]],
                                         ROI_buffer_meters=1.5, points_in_ROI_CRS=UTM10)
    assert 0 < len(by_array.ROI_face_IDs) < len(mesh.faces)
    assert same(by_name.ROI_face_IDs, by_array.ROI_face_IDs) and same(by_name.points, by_array.points) and same(by_name.faces, by_array.faces)
    # a designator names the CROPPED mesh's points afterwards
    assert same(by_name.face_polygon_index(SQUARES, points_in_polygon_CRS=UTM10),
                by_array.face_polygon_index(SQUARES, points_in_polygon_CRS=array[by_array.ROI_point_IDs]))


def test_a_mesh_given_in_UTM_or_lat_lon_equals_the_mesh_given_in_ECEF(scene):
    mesh, array, utm = scene
    from_utm = TexturedPhotogrammetryMesh((utm, mesh.faces), input_CRS=UTM10, backend=Backend(), log_level="ERROR")
    assert from_utm.CRS == "EPSG:4978" and same(from_utm.points, mesh.points)   # the scene was lifted by the same stand-in
    lat_lon = mesh.reproject_CRS("EPSG:4326")
    from_geo = TexturedPhotogrammetryMesh((lat_lon, mesh.faces), input_CRS="EPSG:4326", backend=Backend(), log_level="ERROR")
    assert np.abs(from_geo.points - mesh.points).max() < 2 * cs.load_golden()["standin_err_m"][0] * 2
    assert from_utm.last_reproject_stats["nonfinite"] == 0
    with pytest.raises(NotImplementedError, match="pyproj"):
        TexturedPhotogrammetryMesh((utm, mesh.faces), input_CRS="EPSG:26910", backend=Backend(), log_level="ERROR")


# -- cameras -------------------------------------------------------------------------------------------------------------------------
def _camera_set(scene):
    mesh, array, _ = scene
    angle, scale = 0.4, 2.5
    m = np.eye(4)
    m[:3, :3] = scale * np.array([[np.cos(angle), -np.sin(angle), 0], [np.sin(angle), np.cos(angle), 0], [0, 0, 1]])
    m[:3, 3] = mesh.points.mean(axis=0)
    ecef = mesh.points[[0, 17, 40]] + np.array([[0, 0, 30.0], [5, 5, 40.0], [-3, 2, 50.0]])
    local = (np.linalg.inv(m) @ np.c_[ecef, np.ones(3)].T).T[:, :3]
    transforms = []
    for p in local:
        t = np.eye(4)
        t[:3, 3] = p
        transforms.append(t)
    cams = PhotogrammetryCameraSet(cam_to_world_transforms=transforms, intrinsic_params_per_sensor_type={
        0: {"f": 100.0, "cx": 0.0, "cy": 0.0, "image_width": 8, "image_height": 6}}, image_filenames=[f"a/{i}.jpg" for i in range(3)],
        image_folder="a", sensor_IDs=[0, 0, 0], local_to_epsg_4978_transform=m, validate_images=False)
    return cams, m, local


def test_camera_locations_in_a_CRS(scene):
    cams, m, local = _camera_set(scene)
    backend = Backend()
    moved = np.stack([((m[k, 0] * local[:, 0] + m[k, 1] * local[:, 1]) + m[k, 2] * local[:, 2]) + m[k, 3] for k in range(3)], axis=1)
    want, _ = cs.reproject(moved, (0, 0, 1, 0, 0), (2, -123.0, 0.9996, 500000.0, 0.0))
    hashes = [c.get_camera_hash() for c in cams.cameras]
    assert same(cams.get_camera_locations(), local)   # the default is unchanged
    assert same(cams.get_camera_locations(as_CRS=UTM10, backend=backend), want)
    assert np.abs(want[:, :2] - [552030.0, 4182030.0]).max() < 100
    cam = cams.cameras[1]
    assert cam.get_camera_location() == tuple(local[1, :2]) and cam.get_camera_location(get_z_coordinate=True) == tuple(local[1])
    assert cam.get_camera_location(as_CRS=UTM10, backend=backend) == tuple(want[1, :2])
    assert cam.get_camera_location(get_z_coordinate=True, as_CRS=32610, backend=backend) == tuple(want[1])
    lat, lon, h = cam.get_camera_location(get_z_coordinate=True, as_CRS="EPSG:4326", backend=backend)   # pyproj's order
    lon_lats = cams.get_lon_lat_coords(backend=backend)
    assert lon_lats[1] == (lon, lat) and abs(lon + 122.41) < 0.01 and abs(lat - 37.78) < 0.01 and len(lon_lats) == 3
    assert cams.lon_lats == [None] * 3 and [c.get_camera_hash() for c in cams.cameras] == hashes   # nothing was filled in
    # the ROI subset: a designator equals the array
    region = [SQUARES[0]]
    by_array = cams.get_subset_ROI(region, buffer_radius=8.0, is_geospatial=True, points_in_ROI_CRS=want, backend=backend)
    by_name = cams.get_subset_ROI(region, buffer_radius=8.0, is_geospatial=True, points_in_ROI_CRS=UTM10, backend=backend)
    assert 0 < len(by_array) < 3 and [c.get_camera_hash() for c in by_name.cameras] == [c.get_camera_hash() for c in by_array.cameras]
    with pytest.raises(NotImplementedError, match="points_in_ROI_CRS"):
        cams.get_subset_ROI(region, is_geospatial=True, backend=backend)


# -- entry points ----------------------------------------------------------------------------------------------------------------------
def test_entry_point_flag_pairs():
    from geograypher_amd.entrypoints import aggregate_images, annotation_image_selection, render_height_masks, render_labels

    args = render_height_masks.parse_args(["--image-folder", "i", "--camera-file", "c.xml", "--mesh-file", "m.npz", "--dtm-file", "d.tif",
                                           "--mesh-crs", "EPSG:4978", "--output-folder", "o", "--points-CRS", "EPSG:32610"])
    assert args.points_CRS == "EPSG:32610" and args.points_file is None
    base = ["--mesh-file", "m.npz", "--mesh-CRS", "EPSG:4978", "--cameras-file", "c.xml", "--image-folder", "i"]
    args = render_labels.parse_args(base + ["--texture", "t.geojson", "--render-savefolder", "o", "--texture-CRS", "EPSG:32610", "--DTM-CRS",
                                            "32610", "--ROI-CRS", "EPSG:32611", "--ROI-camera-CRS", "EPSG:32611"])
    assert (args.texture_CRS, args.DTM_CRS, args.ROI_CRS, args.ROI_camera_CRS) == ("EPSG:32610", "32610", "EPSG:32611", "EPSG:32611")
    assert args.texture_points_file is None and args.DTM_points_file is None and args.ROI_points_file is None
    args = aggregate_images.parse_args(base + ["--label-folder", "l", "--IDs-to-labels", "ids.json", "--DTM-CRS", "EPSG:32610", "--ROI-CRS",
                                               "EPSG:32610", "--ROI-camera-CRS", "EPSG:32610", "--top-down-CRS", "EPSG:32610"])
    assert (args.DTM_CRS, args.ROI_CRS, args.ROI_camera_CRS, args.top_down_CRS) == ("EPSG:32610",) * 4
    args = annotation_image_selection.parse_args(base + ["--ROI-CRS", "EPSG:32610", "--ROI-camera-CRS", "EPSG:32610"])
    assert (args.ROI_CRS, args.ROI_camera_CRS) == ("EPSG:32610", "EPSG:32610") and args.ROI_points_file is None
    # every parameter with a points file has the sibling, and giving both is refused before anything is read
    points = np.zeros((3, 3))
    with pytest.raises(ValueError, match="points_file and points_CRS are both given"):
        render_height_masks.render_height_masks("i", "c.xml", "m.npz", "d.tif", "EPSG:4978", None, "o", "raw", 1.0, points_file=points,
                                                points_CRS=UTM10)
    for pair in (("texture_points_file", "texture_CRS"), ("DTM_points_file", "DTM_CRS"), ("ROI_points_file", "ROI_CRS"),
                 ("ROI_camera_points_file", "ROI_camera_CRS")):
        with pytest.raises(ValueError, match=f"{pair[0]} and {pair[1]} are both given"):
            render_labels.render_labels("m.npz", "c.xml", "i", "t.npy", "o", "EPSG:4978", **{pair[0]: points, pair[1]: UTM10})
    for pair in (("DTM_points_file", "DTM_CRS"), ("ROI_points_file", "ROI_CRS"), ("ROI_camera_points_file", "ROI_camera_CRS"),
                 ("top_down_points_file", "top_down_CRS")):
        with pytest.raises(ValueError, match=f"{pair[0]} and {pair[1]} are both given"):
            aggregate_images.aggregate_images("m.npz", "c.xml", "i", "l", "EPSG:4978", **{pair[0]: points, pair[1]: UTM10})
    for pair in (("ROI_points_file", "ROI_CRS"), ("ROI_camera_points_file", "ROI_camera_CRS")):
        with pytest.raises(ValueError, match=f"{pair[0]} and {pair[1]} are both given"):
            annotation_image_selection.determine_minimum_overlapping_images("m.npz", "c.xml", "EPSG:4978", "i", **{pair[0]: points, pair[1]: UTM10})
    with pytest.raises(NotImplementedError, match="pyproj"):   # a CRS that cannot be reprojected fails before any work
        render_labels.render_labels("m.npz", "c.xml", "i", "t.npy", "o", "EPSG:4978", DTM_CRS="EPSG:26910")
    assert geospatial.points_or_CRS("f", None, "c", "32610") == WGS84CRS.utm(10) and geospatial.points_or_CRS("f", None, "c", None) is None
    assert geospatial.points_or_CRS("f", points, "c", None) is points


def test_render_height_masks_takes_the_DTMs_CRS(scene, tmp_path, monkeypatch):
    """The function form end to end, up to the renders: the heights textured onto the mesh are those of the array form."""
    from geograypher_amd.entrypoints import render_height_masks as rhm

    mesh, array, _ = scene
    np.savez(tmp_path / "mesh.npz", points=mesh.points, faces=mesh.faces)
    monkeypatch.setattr(TexturedPhotogrammetryMesh, "save_renders", lambda self, *a, **k: None)
    by_name = rhm.render_height_masks("i", None, tmp_path / "mesh.npz", DTM, "EPSG:4978", None, tmp_path / "o", "raw", 1.0,
                                      points_CRS=UTM10, camera_set=object(), backend=Backend())
    by_array = rhm.render_height_masks("i", None, tmp_path / "mesh.npz", DTM, "EPSG:4978", None, tmp_path / "o", "raw", 1.0,
                                       points_file=array, camera_set=object(), backend=Backend())
    assert same(by_name.face_texture, by_array.face_texture) and np.isfinite(by_name.face_texture).all()


# -- .epsg ---------------------------------------------------------------------------------------------------------------------------
def test_epsg_of_a_geotiff_and_a_geojson(tmp_path, scene):
    from test_height_above_ground_host import DOUBLE, SHORT, write_tiff

    data = np.full((8, 8), 12.0, dtype=np.float32)
    georef = {33550: (DOUBLE, (10.0, 10.0, 0.0)), 33922: (DOUBLE, (0.0, 0.0, 0.0, 551990.0, 4182070.0, 0.0))}
    projected = {34735: (SHORT, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32610))}
    geographic = {34735: (SHORT, (1, 1, 0, 2, 1024, 0, 1, 2, 2048, 0, 1, 4326))}
    user = {34735: (SHORT, (1, 1, 0, 2, 1024, 0, 1, 1, 3072, 0, 1, 32767))}
    for name, keys, want in (("p", projected, 32610), ("g", geographic, 4326), ("u", user, None), ("n", {}, None)):
        write_tiff(tmp_path / f"{name}.tif", data, {**georef, **keys})
        assert PlanarRaster.from_geotiff(tmp_path / f"{name}.tif").epsg == want
    assert PlanarRaster(data, DTM.transform).epsg is None and PlanarRaster(data, DTM.transform, epsg=32610).epsg == 32610
    mesh, array, _ = scene
    dtm = PlanarRaster.from_geotiff(tmp_path / "p.tif")
    assert same(mesh.get_height_above_ground(dtm, points_in_raster_CRS=dtm.epsg), mesh.get_height_above_ground(dtm, points_in_raster_CRS=array))

    ring = SQUARES[0]
    feature = {"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": [ring.tolist() + ring[:1].tolist()]}}
    for name, crs, want in (("urn", {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::32610"}}, 32610),
                            ("short", {"type": "name", "properties": {"name": "EPSG:32733"}}, 32733),
                            ("crs84", {"type": "name", "properties": {"name": "urn:ogc:def:crs:OGC:1.3:CRS84"}}, None), ("none", None, None)):
        doc = {"type": "FeatureCollection", "features": [feature]}
        if crs is not None:
            doc["crs"] = crs
        (tmp_path / f"{name}.geojson").write_text(json.dumps(doc))
        assert PlanarPolygons.from_geojson(tmp_path / f"{name}.geojson")[0].epsg == want
    assert PlanarPolygons.from_sequence(SQUARES).epsg is None
    polygons = PlanarPolygons.from_geojson(tmp_path / "urn.geojson")[0]
    assert same(mesh.face_polygon_index(polygons, points_in_polygon_CRS=polygons.epsg), mesh.face_polygon_index(polygons, points_in_polygon_CRS=array))


def test_the_binding_is_declared():
    """header <-> binding: the call, its structure and its enumerators (tests/test_cabi.py compares the full lists)."""
    import ctypes

    from geograypher_amd import _hip

    text = (ROOT / "include" / "geograster.h").read_text()
    assert re.search(r"\bint gr_reproject_points\(gr_ctx \*ctx, const double \*points, int64_t V, const int32_t \*faces, int64_t F,", text)
    assert "gr_reproject_points" in _hip.EXPORTED_SYMBOLS and len(_hip._SIGNATURES["gr_reproject_points"]) == 11
    body = re.search(r"typedef struct gr_crs \{(.*?)\} gr_crs;", text, re.S).group(1)
    fields = re.findall(r"\b(int32_t|double)\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    types = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(n, types[t]) for t, n in fields] == list(_hip.Crs._fields_)
    assert (_hip.GR_CRS_ECEF, _hip.GR_CRS_GEOGRAPHIC, _hip.GR_CRS_TM) == (cs.ECEF, cs.GEOGRAPHIC, cs.TM) == \
        (geospatial.KIND_ECEF, geospatial.KIND_GEOGRAPHIC, geospatial.KIND_TM)
