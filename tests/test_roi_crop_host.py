"""Region of interest without a GPU (DESIGN.md "Region of interest"): rules Q1-Q6 on a hand-worked scene with every answer written
out, the sub-mesh on a small strip, the constructor's crop, the camera subset, `render_labels` and `aggregate_images` end to end on
the CPU stand-ins, and the C ABI of the two new calls.  The backend is tests/region_standin.py (Fractions and Python loops)."""
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import region_standin as rs  # noqa: E402
import vector_standin as vs  # noqa: E402
from geograypher_amd import _hip, build  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import geometric, synthetic  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]


# -- Q1-Q4 ---------------------------------------------------------------------------------------------------------------------------
def test_hand_worked_scene_every_answer():
    polygons, cases = rs.hand_scene()
    points = np.array([c for c, _, _, _ in cases])
    backend = rs.StandInBackend()
    mask, stats = geometric.points_in_region(backend, polygons, points, rs.HAND_D)
    assert backend.last_region["D"] == 2500000
    for (point, want, _, what), got in zip(cases, mask):
        assert bool(got) == want, (point, what)
    mask0, stats0 = geometric.points_in_region(backend, polygons, np.column_stack([points, np.ones(len(points))]), 0)   # (N, 3) too
    for (point, _, want, what), got in zip(cases, mask0):
        assert bool(got) == want, (point, what, "D = 0")
    n_in, n_contained = sum(w for _, w, _, _ in cases), sum(w for _, _, w, _ in cases)
    assert stats[0] == n_in and stats[1] == n_in - n_contained and stats[2] > 0
    assert stats0[0] == n_contained and stats0[1] == 0 and stats0[2] == 0
    # the stand-in names the hard cases of the scene
    _, info = rs.points_in_region_np(backend.last_region["points_q"], backend.last_region["table"], 2500000)
    assert info["on_ring"].sum() >= 4 and info["two_rows"].sum() == 1 and info["in_hole_outside"].sum() >= 2
    assert info["in_hole_within_D"].sum() == 2 and info["at_D_edge"].sum() >= 3 and info["at_D_vertex"].sum() == 1
    assert info["one_step_beyond"].sum() >= 6


def test_inputs_and_bad_inputs(tmp_path):
    polygons, cases = rs.hand_scene()
    points = np.array([c for c, _, _, _ in cases])
    want = np.array([w for _, w, _, _ in cases])
    backend = rs.StandInBackend()
    # Q1: ring arrays, and a .geojson whose features are dissolved into one region
    rings = [[vs.square(0, 0, 20, 20), vs.square(5, 5, 15, 15)], vs.square(18, 18, 26, 26), np.array([[40.0, 0.0], [46.0, 0.0], [46.0, 8.0]])]
    assert np.array_equal(geometric.points_in_region(backend, rings, points, 2.5)[0], want)
    features = [{"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": [
        [[float(x), float(y)] for x, y in np.vstack([r, r[:1]])] for r in (item if isinstance(item, list) else [item])]}} for item in rings]
    (tmp_path / "roi.geojson").write_text(json.dumps({"type": "FeatureCollection", "features": features}))
    assert np.array_equal(geometric.points_in_region(backend, tmp_path / "roi.geojson", points, 2.5)[0], want)
    with pytest.raises(NotImplementedError, match="geojson"):
        geometric.points_in_region(backend, tmp_path / "roi.gpkg", points, 2.5)
    # Q2: the buffer's range
    assert geometric.region_buffer_steps(2.5) == 2500000 and geometric.region_buffer_steps(0) == 0
    for bad in (-1e-6, -3.0, 2.0 ** 40 * 1e-6, float("nan")):
        with pytest.raises(ValueError, match="buffer"):
            geometric.points_in_region(backend, polygons, points, bad)
    with pytest.raises(ValueError, match=r"\(N, 2\) or \(N, 3\)"):
        geometric.points_in_region(backend, polygons, np.zeros((4, 4)), 0)
    with pytest.raises(ValueError, match="2\\^40"):
        geometric.points_in_region(backend, polygons, np.array([[3.0e6, 0.0]]), 0)
    # Q6: a row without rings holds nothing, an ROI without rings keeps nothing
    lonely = PlanarPolygons([vs.square(0, 0, 1, 1)], [2], [False], n_polygons=4)
    assert geometric.points_in_region(backend, lonely, np.array([[0.5, 0.5], [5.0, 5.0]]), 0)[0].tolist() == [True, False]
    nothing = PlanarPolygons([], [], [], n_polygons=3)
    assert not geometric.points_in_region(backend, nothing, points, 2.5)[0].any()


# -- Q5 ------------------------------------------------------------------------------------------------------------------------------
def strip(backend=None, **kw):
    points, faces = rs.strip_mesh()
    return TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=backend or rs.StandInBackend(), **kw), points, faces


def around(x, y, r=0.1):
    return [vs.square(x - r, y - r, x + r, y + r)]


def test_submesh_on_the_strip():
    mesh, points, faces = strip()
    # vertex 6 = (3, 0) alone is in the region: the three faces that use it are kept, each by that one vertex
    (sub_points, sub_faces), point_IDs, face_IDs = mesh.select_mesh_ROI(around(3, 0), return_original_IDs=True, points_in_ROI_CRS=points)
    assert face_IDs.tolist() == [4, 5, 6] and point_IDs.tolist() == [4, 5, 6, 7, 8]
    assert face_IDs.dtype == np.int64 and point_IDs.dtype == np.int64 and sub_faces.dtype == np.int64
    assert sub_faces.tolist() == [[0, 2, 1], [1, 2, 3], [2, 4, 3]] and np.array_equal(sub_points, points[4:9])
    assert np.array_equal(sub_points[sub_faces], points[faces[face_IDs]])
    assert mesh.last_ROI_stats["points_inside"] == 1 and mesh.last_ROI_stats["faces_kept"] == 3
    # the same through the buffer: an ROI 0.5 m away, grown by 0.5 m, touches the vertex exactly
    got = mesh.select_mesh_ROI([vs.square(2.9, -1.0, 3.1, -0.5)], buffer_meters=0.5, points_in_ROI_CRS=points[:, :2])
    assert np.array_equal(got[0], sub_points) and np.array_equal(got[1], sub_faces)
    # a vertex in the region that no face uses is dropped; with nothing else in the region nothing is kept
    (p0, f0), pid, fid = mesh.select_mesh_ROI(around(0.5, 0.5), return_original_IDs=True, points_in_ROI_CRS=points)
    assert p0.shape == (0, 3) and f0.shape == (0, 3) and pid.shape == (0,) and fid.shape == (0,) and pid.dtype == np.int64
    (p1, f1), pid, fid = mesh.select_mesh_ROI([vs.square(-0.1, -0.1, 0.6, 0.6)], return_original_IDs=True, points_in_ROI_CRS=points)
    assert pid.tolist() == [0, 1, 2] and fid.tolist() == [0] and f1.tolist() == [[0, 2, 1]]
    # everything kept: the identity (the loose vertex is the last one, so the faces stay as they are)
    (p2, f2), pid, fid = mesh.select_mesh_ROI([vs.square(-1, -1, 9, 9)], return_original_IDs=True, points_in_ROI_CRS=points)
    assert np.array_equal(fid, np.arange(len(faces))) and np.array_equal(pid, np.arange(len(points) - 1))
    assert np.array_equal(f2, faces) and np.array_equal(p2, points[:-1])
    # None: the mesh unchanged
    assert mesh.select_mesh_ROI(None)[0] is mesh.points and mesh.select_mesh_ROI(None)[1] is mesh.faces
    # bad input
    with pytest.raises(NotImplementedError, match="simplify_tol_meters"):
        mesh.select_mesh_ROI(around(3, 0), simplify_tol_meters=1, points_in_ROI_CRS=points)
    with pytest.raises(NotImplementedError, match="points_in_ROI_CRS"):
        mesh.select_mesh_ROI(around(3, 0))
    with pytest.raises(ValueError, match="points_in_ROI_CRS must be"):
        mesh.select_mesh_ROI(around(3, 0), points_in_ROI_CRS=points[:-1])
    broken = faces.copy()
    broken[3, 1] = 99
    bad_mesh = TexturedPhotogrammetryMesh((points, broken), log_level="ERROR", backend=rs.StandInBackend())
    with pytest.raises(ValueError, match="gr_submesh_extract: 1 faces"):
        bad_mesh.select_mesh_ROI(around(3, 0), points_in_ROI_CRS=points)


def test_constructor_crops_before_the_texture():
    points, faces = rs.strip_mesh()
    face_tex = np.arange(len(faces), dtype=np.float64) * 10
    vert_tex = np.arange(len(points), dtype=np.float64) + 100
    mesh, _, _ = strip(ROI=around(3, 0), points_in_ROI_CRS=points, texture=face_tex)
    assert mesh.ROI_face_IDs.tolist() == [4, 5, 6] and mesh.ROI_point_IDs.tolist() == [4, 5, 6, 7, 8]
    assert mesh.faces.tolist() == [[0, 2, 1], [1, 2, 3], [2, 4, 3]] and np.array_equal(mesh.points, points[4:9])
    assert mesh.face_texture[:, 0].tolist() == [40.0, 50.0, 60.0] and mesh.vertex_texture is None     # the ORIGINAL face count
    mesh, _, _ = strip(ROI=around(3, 0), points_in_ROI_CRS=points, texture=vert_tex)
    assert mesh.vertex_texture[:, 0].tolist() == [104.0, 105.0, 106.0, 107.0, 108.0]                    # the ORIGINAL vertex count
    mesh, _, _ = strip(ROI=around(3, 0), points_in_ROI_CRS=points, texture=np.array([7.0, 8.0, 9.0]))
    assert mesh.face_texture[:, 0].tolist() == [7.0, 8.0, 9.0]                                          # the cropped count: as it is
    mesh, _, _ = strip(ROI=[vs.square(2.9, -1.0, 3.1, -0.5)], ROI_buffer_meters=0.5, points_in_ROI_CRS=points)
    assert mesh.ROI_face_IDs.tolist() == [4, 5, 6]
    with pytest.raises(ValueError, match="did not match"):
        strip(ROI=around(3, 0), points_in_ROI_CRS=points, texture=np.zeros(4))
    with pytest.raises(NotImplementedError, match="ROI cropping"):
        strip(ROI=around(3, 0))
    plain, _, _ = strip()
    assert plain.ROI_point_IDs is None and plain.ROI_face_IDs is None and plain.faces.shape == faces.shape


# -- cameras -------------------------------------------------------------------------------------------------------------------------
def test_camera_locations_and_subset_ROI(tmp_path):
    _, cams = synthetic.config1_scene()
    locations = cams.get_camera_locations()
    assert locations.shape == (len(cams), 3) and locations.dtype == np.float64
    for cam, loc in zip(cams.cameras, locations):
        assert np.array_equal(loc, np.asarray(cam.cam_to_world_transform)[:3, 3])
    backend = rs.StandInBackend()
    x, y = locations[1, :2]
    # local: ring arrays are compared with the local camera locations; the camera ON the grown region's boundary is kept
    near_1 = [vs.square(x + 1.0, y - 0.5, x + 2.0, y + 0.5)]
    dist = np.array([rs.distance2(*[int(round(v * 1e6)) for v in loc[:2]], *[int(round(v * 1e6)) for v in (x + 1.0, y - 0.5, x + 1.0, y + 0.5)])[0]
                     for loc in locations], dtype=np.float64) ** 0.5 / 1e6
    sub = cams.get_subset_ROI(near_1, buffer_radius=1.0, backend=backend)
    want = np.nonzero(dist <= 1.0)[0].tolist()
    assert 1 in want and len(want) < len(cams)
    assert [c.get_camera_hash() for c in sub.cameras] == [cams.cameras[i].get_camera_hash() for i in want]
    assert len(cams.get_subset_ROI(near_1, buffer_radius=0.5, backend=backend)) == len(np.nonzero(dist <= 0.5)[0])
    # geospatial: positions in the ROI's CRS are passed in; a .geojson is geospatial by default
    ring = vs.square(500000.0, 4000000.0, 500010.0, 4000010.0)
    (tmp_path / "roi.geojson").write_text(json.dumps({"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": [ring.tolist() + ring[:1].tolist()]}}]}))
    utm = np.tile([[400000.0, 4000005.0]], (len(cams), 1))
    utm[[0, 2]] = [[500005.0, 4000005.0], [500012.0, 4000005.0]]
    with pytest.raises(NotImplementedError, match="points_in_ROI_CRS"):
        cams.get_subset_ROI(tmp_path / "roi.geojson", backend=backend)
    with pytest.raises(NotImplementedError, match="points_in_ROI_CRS"):
        cams.get_subset_ROI([ring], is_geospatial=True, backend=backend)
    with pytest.raises(ValueError, match="points_in_ROI_CRS must be"):
        cams.get_subset_ROI(tmp_path / "roi.geojson", points_in_ROI_CRS=utm[:-1], backend=backend)
    assert len(cams.get_subset_ROI(tmp_path / "roi.geojson", points_in_ROI_CRS=utm, backend=backend)) == 1
    both = cams.get_subset_ROI(tmp_path / "roi.geojson", buffer_radius=2.0, points_in_ROI_CRS=utm, backend=backend)
    assert [c.get_camera_hash() for c in both.cameras] == [cams.cameras[i].get_camera_hash() for i in (0, 2)]
    # the two filename filters
    for i, c in enumerate(cams.cameras):
        c.image_filename = Path("/data", "flight_a" if i % 2 else "flight_b", f"img_{i}.JPG")
    assert len(cams.get_cameras_in_folder("/data/flight_a")) == len(cams) // 2
    assert len(cams.get_cameras_matching_filename_regex(r"img_[01]\.JPG$")) == 2


# -- the entry points ----------------------------------------------------------------------------------------------------------------
def _c1_with_files(tmp_path):
    (points, faces), cams = synthetic.config1_scene()
    sub = cams[0:2]
    for i, c in enumerate(sub.cameras):
        c.image_filename = Path(tmp_path, "images", "flight", f"img_{i}.JPG")
    sub.image_folder = Path(tmp_path, "images")
    lo, hi = points[:, :2].min(axis=0), points[:, :2].max(axis=0)
    roi = [vs.square(*(lo + (hi - lo) * 0.3), *(lo + (hi - lo) * 0.55))]
    return points, faces, sub, roi, lo, hi


def _manual_crop(points, faces, roi, buffer_meters):
    backend = rs.StandInBackend()
    mask, _ = geometric.points_in_region(backend, roi, points, buffer_meters)
    face_ids, point_ids, new_faces, bad = rs.submesh_np(mask, faces)
    assert bad == 0 and 0 < len(face_ids) < len(faces)
    return points[point_ids], new_faces.astype(np.int64), point_ids, face_ids


def test_render_labels_with_an_ROI_equals_the_manually_cropped_mesh(tmp_path, oracle_backend_cls):
    from PIL import Image

    from geograypher_amd.entrypoints.render_labels import parse_args, render_labels

    class Backend(rs.StandInBackend, vs.StandInBackend, oracle_backend_cls):
        pass

    points, faces, sub, roi, lo, hi = _c1_with_files(tmp_path)
    extent = float((hi - lo).max())
    buffer_meters = round(0.05 * extent, 3)
    np.savez(tmp_path / "mesh.npz", points=points, faces=faces)
    np.save(tmp_path / "points_utm.npy", points)
    ring = roi[0]
    (tmp_path / "roi.geojson").write_text(json.dumps({"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": [ring.tolist() + ring[:1].tolist()]}}]}))
    texture = (np.arange(len(faces)) % 3).astype(np.float64)
    kw = dict(render_image_scale=0.25, apply_distortion=False)
    mesh = render_labels(tmp_path / "mesh.npz", None, tmp_path / "images", texture, tmp_path / "roi_renders", "EPSG:4978",
                         ROI=tmp_path / "roi.geojson", mesh_ROI_buffer_radius_meters=buffer_meters,
                         ROI_points_file=tmp_path / "points_utm.npy", camera_set=sub, backend=Backend(), **kw)
    crop_points, crop_faces, point_ids, face_ids = _manual_crop(points, faces, roi, buffer_meters)
    assert np.array_equal(mesh.ROI_point_IDs, point_ids) and np.array_equal(mesh.ROI_face_IDs, face_ids)
    assert np.array_equal(mesh.points, crop_points) and np.array_equal(mesh.faces, crop_faces)
    assert np.array_equal(mesh.face_texture[:, 0], texture[face_ids])
    np.savez(tmp_path / "crop.npz", points=crop_points, faces=crop_faces)
    render_labels(tmp_path / "crop.npz", None, tmp_path / "images", texture[face_ids], tmp_path / "crop_renders", "EPSG:4978",
                  camera_set=sub, backend=Backend(), **kw)
    seen = 0
    for i in range(2):
        got = np.asarray(Image.open(tmp_path / "roi_renders" / "flight" / f"img_{i}.tif"))
        want = np.asarray(Image.open(tmp_path / "crop_renders" / "flight" / f"img_{i}.tif"))
        assert np.array_equal(got, want)
        seen += int((got != got.max()).sum())
    assert seen > 0
    # a vector texture and the camera cut: the points files are those of the ORIGINAL mesh; camera 1 lies outside
    features = [{"type": "Feature", "properties": {"species": name},
                 "geometry": {"type": "Polygon", "coordinates": [vs.square(*a, *b).tolist() + vs.square(*a, *b)[:1].tolist()]}}
                for name, a, b in (("oak", lo, (lo + hi) / 2), ("fir", (lo + hi) / 2, hi))]
    (tmp_path / "crowns.geojson").write_text(json.dumps({"type": "FeatureCollection", "features": features}))
    camera_points = np.array([ring.mean(axis=0), hi + 10 * extent])
    mesh2 = render_labels(tmp_path / "mesh.npz", None, tmp_path / "images", tmp_path / "crowns.geojson", tmp_path / "cut", "EPSG:4978",
                          texture_column_name="species", ROI=roi, mesh_ROI_buffer_radius_meters=buffer_meters, ROI_points_file=points,
                          ROI_camera_points_file=camera_points, cameras_ROI_buffer_radius_meters=1.0,
                          texture_points_file=tmp_path / "points_utm.npy", camera_set=sub, backend=Backend(),
                          render_image_scale=0.25, apply_distortion=False)
    assert (tmp_path / "cut" / "flight" / "img_0.tif").is_file() and not (tmp_path / "cut" / "flight" / "img_1.tif").exists()
    plain = TexturedPhotogrammetryMesh((crop_points, crop_faces), log_level="ERROR", backend=Backend())
    plain.load_texture(tmp_path / "crowns.geojson", texture_column_name="species", points_in_polygon_CRS=crop_points)
    assert np.array_equal(mesh2.face_texture, plain.face_texture, equal_nan=True) and np.isfinite(plain.face_texture).any()
    # ROI without its points still raises, exactly as before; the CLI has the two new flags
    with pytest.raises(NotImplementedError, match="ROI"):
        render_labels(tmp_path / "mesh.npz", None, tmp_path / "images", texture, tmp_path / "x", "EPSG:4978", ROI=roi, camera_set=sub,
                      backend=Backend())
    args = parse_args(["--mesh-file", "m.npz", "--mesh-CRS", "EPSG:4978", "--cameras-file", "c.xml", "--image-folder", "i", "--texture",
                       "t.npy", "--render-savefolder", "o", "--ROI", "roi.geojson", "--ROI-points-file", "p.npy",
                       "--ROI-camera-points-file", "c.npy"])
    assert args.ROI == "roi.geojson" and args.ROI_points_file == Path("p.npy") and args.ROI_camera_points_file == Path("c.npy")


def test_aggregate_images_with_an_ROI_equals_the_manually_cropped_mesh(tmp_path, oracle_backend_cls):
    from PIL import Image

    from geograypher_amd.entrypoints.aggregate_images import aggregate_images, parse_args

    class Backend(rs.StandInBackend, vs.StandInBackend, oracle_backend_cls):
        pass

    points, faces, sub, roi, lo, hi = _c1_with_files(tmp_path)
    buffer_meters = round(0.05 * float((hi - lo).max()), 3)
    h, w = sub.cameras[0].get_image_size()
    rng = np.random.default_rng(1)
    for i in range(2):
        (tmp_path / "labels" / "flight").mkdir(parents=True, exist_ok=True)
        blocks = rng.integers(0, 4, (h // 16 + 1, w // 16 + 1)).astype(np.uint8)
        Image.fromarray(np.kron(blocks, np.ones((16, 16), dtype=np.uint8))[:h, :w]).save(tmp_path / "labels" / "flight" / f"img_{i}.png")
    np.savez(tmp_path / "mesh.npz", points=points, faces=faces)
    ids = {0: "a", 1: "b", 2: "c", 3: "d"}
    (tmp_path / "ids.json").write_text(json.dumps(ids))
    kw = dict(take_every_nth_camera=1, aggregate_image_scale=0.25, camera_set=sub)
    mesh, values, classes = aggregate_images(
        tmp_path / "mesh.npz", None, tmp_path / "images", tmp_path / "labels", "EPSG:4978", ROI=roi,
        ROI_buffer_radius_meters=buffer_meters, ROI_points_file=points, IDs_to_labels=str(tmp_path / "ids.json"),
        aggregated_face_values_savefile=tmp_path / "out" / "roi_values.npy",
        predicted_face_classes_savefile=tmp_path / "out" / "roi_classes.npy", backend=Backend(), **kw)
    crop_points, crop_faces, point_ids, face_ids = _manual_crop(points, faces, roi, buffer_meters)
    assert np.array_equal(mesh.ROI_face_IDs, face_ids) and np.array_equal(mesh.faces, crop_faces)
    np.savez(tmp_path / "crop.npz", points=crop_points, faces=crop_faces)
    aggregate_images(tmp_path / "crop.npz", None, tmp_path / "images", tmp_path / "labels", "EPSG:4978", IDs_to_labels=ids,
                     aggregated_face_values_savefile=tmp_path / "out" / "crop_values.npy",
                     predicted_face_classes_savefile=tmp_path / "out" / "crop_classes.npy", backend=Backend(), **kw)
    got_v, want_v = np.load(tmp_path / "out" / "roi_values.npy"), np.load(tmp_path / "out" / "crop_values.npy")
    got_c, want_c = np.load(tmp_path / "out" / "roi_classes.npy"), np.load(tmp_path / "out" / "crop_classes.npy")
    assert got_v.shape == (len(face_ids), 4) and np.array_equal(got_v, want_v, equal_nan=True)
    assert got_c.shape == (len(face_ids), 1) and np.array_equal(got_c, want_c, equal_nan=True)
    assert np.array_equal(got_c, classes, equal_nan=True) and np.isfinite(got_c).sum() > 100 and len(np.unique(got_c[np.isfinite(got_c)])) == 4
    # the camera filters and the camera cut: only camera 0 survives the regex, and its position is outside the ROI
    cut = aggregate_images(tmp_path / "crop.npz", None, tmp_path / "images", tmp_path / "labels", "EPSG:4978", IDs_to_labels=ids,
                           filename_regex=r"img_0", subset_images_folder=tmp_path / "images" / "flight", backend=Backend(), **kw)
    assert np.isfinite(cut[2]).sum() > 0 and not np.array_equal(cut[1], want_v, equal_nan=True)
    camera_points = np.array([roi[0].mean(axis=0), hi + 1000.0])   # of the FULL set: they follow the cameras through the filters
    one = aggregate_images(tmp_path / "mesh.npz", None, tmp_path / "images", tmp_path / "labels", "EPSG:4978", IDs_to_labels=ids,
                           ROI=roi, ROI_buffer_radius_meters=buffer_meters, ROI_points_file=points,
                           ROI_camera_points_file=camera_points, backend=Backend(), **kw)
    assert np.array_equal(one[1], cut[1], equal_nan=True)            # camera 1 was cut by the ROI: the same as the regex's choice
    with pytest.raises(IndexError):   # camera 1 alone is left by the regex and lies outside: no camera, the reference's IndexError
        aggregate_images(tmp_path / "mesh.npz", None, tmp_path / "images", tmp_path / "labels", "EPSG:4978", IDs_to_labels=ids,
                         ROI=roi, ROI_buffer_radius_meters=buffer_meters, ROI_points_file=points, filename_regex=r"img_1",
                         ROI_camera_points_file=camera_points, backend=Backend(), **kw)
    for bad in ({"mesh_downsample": 0.5}, {"top_down_vector_projection_savefile": "map.geojson"}, {"vis": True}, {"ROI": roi},
                {"DTM_file": "dtm.tif"}):
        with pytest.raises(NotImplementedError):
            aggregate_images(tmp_path / "mesh.npz", None, tmp_path / "images", tmp_path / "labels", "EPSG:4978", IDs_to_labels=ids,
                             backend=Backend(), **kw, **bad)
    args = parse_args(["--mesh-file", "m.npz", "--mesh-CRS", "EPSG:4978", "--cameras-file", "c.xml", "--image-folder", "i",
                       "--label-folder", "l", "--IDs-to-labels", "ids.json", "--ROI", "roi.geojson", "--ROI-points-file", "p.npy"])
    assert args.ROI == "roi.geojson" and args.ROI_points_file == Path("p.npy") and args.take_every_nth_camera is None


# -- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_source_name_the_new_calls():
    header = (ROOT / "include" / "geograster.h").read_text()
    source = (ROOT / "geograypher_amd" / "csrc" / "polygons.hip").read_text()
    internal = (ROOT / "geograypher_amd" / "csrc" / "gr_internal.hpp").read_text()
    for name, n_args, kernels in (("gr_points_in_region", 14, ("k_points_in_region",)),
                                  ("gr_submesh_extract", 10, ("k_submesh_flags", "k_submesh_write"))):
        decl = re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1)
        assert len(decl.split(",")) == n_args == len(_hip._SIGNATURES[name])
        assert name in _hip.EXPORTED_SYMBOLS and re.search(rf"\bint {name}\(gr_ctx \*c,", source)
        assert all(k in source and k in internal for k in kernels)
    assert "#define GR_VERSION 126" in header and "meshes/meshes.py:646-731" in header and "cameras/cameras.py:1207-1273" in header
    assert (_hip.GR_PIR_STAT_INSIDE, _hip.GR_PIR_STAT_BUFFER_ONLY, _hip.GR_PIR_STAT_WIDE, _hip.GR_PIR_STAT_WORDS) == (0, 1, 2, 4)
    csrc = ROOT / "geograypher_amd" / "csrc"      # the scans: a step of cub_steps.hpp, declared and run by the shared compaction
    assert "__umul64hi" in source and "const FlagScan fs(c, p, F), vs(c, p, V);" in source and "compact_write(" in source
    assert "ExclusiveSum<int32_t> scan;" in (csrc / "compact_dev.hpp").read_text()
    assert "hipcub::DeviceScan::ExclusiveSum(" in (csrc / "cub_steps.hpp").read_text()
    assert any(p.name == "polygons.hip" for p in build.SOURCES)
    assert callable(_hip.HipRaster.points_in_region) and callable(_hip.HipRaster.submesh_extract)
