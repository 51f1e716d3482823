"""`TexturedPhotogrammetryMesh.vis`, the camera frusta and `save_renders(make_composites=True)` without a GPU: the Python paths on
the CPU oracle's ids and depth with the numpy stand-in (tests/vis_standin.py) in place of the kernels, and the argument rules."""
import json
import logging
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

from geograypher_amd.cameras import PhotogrammetryCamera, PhotogrammetryCameraSet  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.meshes import vis as mesh_vis  # noqa: E402
from geograypher_amd.utils import colormaps, synthetic  # noqa: E402
from oracle import oracle_c  # noqa: E402
from tests.oracle_backend import OracleBackend  # noqa: E402
from tests.test_vis_host import StandinBackend, standin_composite  # noqa: E402


class OraclePictureBackend(StandinBackend, OracleBackend):
    """The CPU oracle with a depth plane, and the picture calls by the stand-in."""

    def raster_face_ids(self, cams, h, w, out=None, want_depth=False, check=True):
        if not want_depth:
            return OracleBackend.raster_face_ids(self, cams, h, w)
        cams = np.asarray(cams, dtype=np.float32).reshape(-1, 16)
        planes = [oracle_c.raster(self.verts, self.faces, cam, h, w, want_depth=True) for cam in cams]
        return torch.from_numpy(np.stack([p[0] for p in planes])), torch.from_numpy(np.stack([p[1] for p in planes]))


@pytest.fixture(scope="module")
def c1():
    (points, faces), cams = synthetic.config1_scene()
    return points, faces, cams


def c1_mesh(c1, backend, **kwargs):
    points, faces, _ = c1
    classes = (np.arange(len(faces)) // 700 % 5).astype(np.float64)
    classes[::97] = np.nan
    return TexturedPhotogrammetryMesh((points, faces), texture=classes, IDs_to_labels={k: f"class {k}" for k in range(5)},
                                      backend=backend, log_level="ERROR", **kwargs)


# -- frusta ------------------------------------------------------------------------------------------------------------------------
def test_frustum_geometry_hand_worked():
    T = np.eye(4)
    T[:3, 3] = (10.0, 20.0, 30.0)
    camera = PhotogrammetryCamera(None, T, f=100.0, cx=10.0, cy=-20.0, image_width=400, image_height=200)
    points, faces, rgb = camera.get_vis_mesh(frustum_scale=2.0)
    # half width 2, half height 1, principal point (0.1, -0.2): right 2.1, left -1.9, top 0.8, bottom -1.2, all times 2
    want = np.array([[0, 0, 0], [4.2, 1.6, 2], [4.2, -2.4, 2], [-3.8, -2.4, 2], [-3.8, 1.6, 2]]) + T[:3, 3]
    assert np.allclose(points, want, rtol=0, atol=1e-12)
    assert faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1], [1, 2, 3], [3, 4, 1]]
    assert rgb.dtype == np.uint8 and rgb.tolist() == [[0, 0, 255], [255, 0, 0], [0, 0, 255], [0, 0, 255], [0, 0, 255], [0, 0, 255]]
    assert (points[faces[1]][:, 1] <= 20.0).all() and (points[faces[1]][1:, 1] == 20.0 - 2.4).all(), "the red side is the -Y side"
    # a homogeneous scale in the transform is divided out
    scaled = PhotogrammetryCamera(None, T * 2.0, f=100.0, cx=10.0, cy=-20.0, image_width=400, image_height=200)
    assert np.allclose(scaled.get_vis_mesh(2.0)[0], want, rtol=0, atol=1e-12)


def test_the_sets_frusta_are_scaled_by_the_cube_root_of_the_determinant():
    poses = [synthetic.nadir_pose(0.0, 0.0, 40.0), synthetic.nadir_pose(5.0, 0.0, 40.0)]
    cams = synthetic.camera_set_from_poses(poses, f=500.0, width=640, height=480)
    points, faces, rgb = cams.get_vis_mesh(frustum_scale=2)
    assert points.shape == (10, 3) and faces.shape == (12, 3) and rgb.shape == (12, 3) and faces[6:].min() == 5
    one = cams.cameras[1].get_vis_mesh(2)[0]
    assert np.array_equal(points[5:], one)
    local_to_world = np.diag([4.0, 4.0, 4.0, 1.0])
    cams._local_to_epsg_4978_transform = local_to_world
    assert np.allclose(cams.get_vis_mesh(frustum_scale=2)[0][5:], cams.cameras[1].get_vis_mesh(0.5)[0], rtol=0, atol=1e-12)
    assert np.array_equal(cams.get_vis_mesh(2, correct_for_scale=False)[0], points)
    assert np.array_equal(cams.get_vis_mesh(None)[0][5:], cams.cameras[1].get_vis_mesh(0.1)[0])


# -- the frame, the view and the colours -------------------------------------------------------------------------------------------
def test_picture_frame_is_east_north_up_on_the_earth_and_a_shift_elsewhere():
    lon, lat, a = np.deg2rad(-120.0), np.deg2rad(39.0), 6378137.0
    e2 = mesh_vis.WGS84_E2
    N = a / np.sqrt(1 - e2 * np.sin(lat) ** 2)
    centre = np.array([(N + 1500.0) * np.cos(lat) * np.cos(lon), (N + 1500.0) * np.cos(lat) * np.sin(lon), (N * (1 - e2) + 1500.0) * np.sin(lat)])
    M = mesh_vis.picture_frame(centre)
    up = np.array([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])
    assert np.allclose(M[:3, :3] @ M[:3, :3].T, np.eye(3), atol=1e-12) and np.allclose(M[:3, :3] @ up, (0, 0, 1), atol=1e-9)
    assert np.allclose(M[:3, :3] @ np.array([0.0, 0.0, 1.0]), (0, np.cos(lat), np.sin(lat)), atol=1e-9), "north has no east part"
    assert np.allclose(M @ np.append(centre, 1.0), (0, 0, 0, 1), atol=1e-6)
    local = mesh_vis.picture_frame(np.array([3.0, 4.0, 5.0]))
    assert np.array_equal(local[:3, :3], np.eye(3)) and local[:3, 3].tolist() == [-3.0, -4.0, -5.0]


def test_the_default_view_looks_from_the_south_west_and_holds_the_sphere():
    points = np.array([[10.0, 0, 0], [-10.0, 0, 0], [0, 10.0, 0], [0, 0, -10.0]])
    camera = mesh_vis.view_camera(None, points, (300, 400), np.eye(4), None)
    T = np.asarray(camera.cam_to_world_transform)
    position = T[:3, 3]
    assert position[0] < 0 and position[1] < 0 and position[2] > 0 and np.isclose(position[0], position[1])
    assert np.isclose(np.rad2deg(np.arcsin(position[2] / np.linalg.norm(position))), 35.264)
    assert np.allclose(T[:3, 2], -position / np.linalg.norm(position)) and np.isclose(T[2, 0], 0.0) and T[2, 1] < 0, "+Y is down"
    assert np.isclose(np.linalg.det(T[:3, :3]), 1.0)
    assert np.isclose(np.linalg.norm(position), 10.0 / np.sin(np.deg2rad(15.0)))      # the vertical angle is the narrow one
    assert np.isclose(camera.f, 150.0 / np.tan(np.deg2rad(15.0))) and (camera.image_height, camera.image_width) == (300, 400)
    tall = mesh_vis.view_camera(dict(view_angle_deg=60.0, azimuth_deg=0.0, elevation_deg=90.0), points, (400, 200), np.eye(4), None)
    assert np.isclose(np.linalg.norm(np.asarray(tall.cam_to_world_transform)[:3, 3]), 10.0 / np.sin(np.arctan(np.tan(np.deg2rad(30.0)) / 2)))
    with pytest.raises(ValueError, match="view takes"):
        mesh_vis.view_camera(dict(roll=3), points, (3, 4), np.eye(4), None)
    # a camera: its pose through local_to_epsg_4978 (a scale of 2) and the frame, its view angle in the window
    pose = synthetic.nadir_pose(1.0, 2.0, 40.0)
    given = PhotogrammetryCamera(None, pose, f=500.0, cx=3.0, cy=4.0, image_width=640, image_height=480)
    seen = mesh_vis.view_camera(given, points, (240, 320), np.eye(4), np.diag([2.0, 2.0, 2.0, 1.0]))
    assert np.allclose(np.asarray(seen.cam_to_world_transform)[:3, :3], pose[:3, :3]) and np.allclose(seen.cam_to_world_transform[:3, 3], (2, 4, 80))
    assert seen.f == 250.0 and (seen.cx, seen.cy) == (0.0, 0.0)


def test_face_colours():
    tab10 = np.floor(colormaps.table("tab10") * 255 + 0.5).astype(np.uint8)
    rgb, legend = mesh_vis.face_colours(np.array([0, 3, np.nan, 7, 1.5]), {0: "a", 3: "b"}, 5)
    assert rgb[:2].tolist() == [tab10[0].tolist(), tab10[3].tolist()] and rgb[2:].tolist() == [list(mesh_vis.NAN_RGB)] * 3
    assert legend == {"a": tab10[0].tolist(), "b": tab10[3].tolist()}
    tab20 = np.floor(colormaps.table("tab20") * 255 + 0.5).astype(np.uint8)
    assert mesh_vis.face_colours(np.array([12.0]), {12: "x"}, 1)[0].tolist() == [tab20[12].tolist()]
    viridis = np.floor(colormaps.table("viridis") * 255 + 0.5).astype(np.uint8)
    rgb, legend = mesh_vis.face_colours(np.array([[2.0], [4.0], [3.0], [np.nan]]), None, 4)
    assert rgb.tolist() == [viridis[0].tolist(), viridis[255].tolist(), viridis[128].tolist(), list(mesh_vis.NAN_RGB)]
    assert legend == {"2.0": viridis[0].tolist(), "4.0": viridis[255].tolist()}
    assert mesh_vis.face_colours(np.array([25.0, 0.0]), {25: "many"}, 2)[0].tolist() == [viridis[255].tolist(), viridis[0].tolist()]
    rgb, _ = mesh_vis.face_colours(np.array([[300.0, 20.0, -5.0], [np.nan, 1, 1]]), None, 2)
    assert rgb.tolist() == [[255, 20, 0], list(mesh_vis.NAN_RGB)]
    assert mesh_vis.face_colours(np.array([[1.0, 0.5, 0.0]]), None, 1)[0].tolist() == [[255, 127, 0]]
    assert mesh_vis.face_colours(None, None, 2)[0].tolist() == [list(mesh_vis.PLAIN_RGB)] * 2
    with pytest.raises(ValueError, match="one row per face"):
        mesh_vis.face_colours(np.zeros(3), None, 2)


# -- vis ---------------------------------------------------------------------------------------------------------------------------
def test_vis_argument_rules(c1, tmp_path, caplog):
    mesh = c1_mesh(c1, OraclePictureBackend())
    with pytest.raises(NotImplementedError, match="no window"):
        mesh.vis()
    with pytest.raises(TypeError, match="unexpected keyword"):
        mesh.vis(return_image=True, colour="red")
    with pytest.raises(ValueError, match="supersample"):
        mesh.vis(return_image=True, supersample=5)
    mesh.logger.setLevel(logging.INFO)
    mesh.logger.propagate = True
    with caplog.at_level(logging.INFO):
        image = mesh.vis(return_image=True, window_size=(40, 30), supersample=1, plotter=None, interactive=False, force_xvfb=True,
                         interactive_jupyter=False, plotter_kwargs={})
    said = [r.getMessage() for r in caplog.records if "are ignored" in r.getMessage()]
    assert len(said) == 1 and all(k in said[0] for k in ("plotter", "interactive", "force_xvfb", "plotter_kwargs", "interactive_jupyter"))
    assert image.shape == (30, 40, 3) and image.dtype == np.uint8


def test_vis_on_the_oracle_writes_the_picture_the_legend_and_restores_the_mesh(c1, tmp_path):
    points, faces, cams = c1
    backend = OraclePictureBackend()
    mesh = c1_mesh(c1, backend)
    before = mesh.pix2face(cams[0], render_img_scale=0.1, apply_distortion=False)
    held, uploads = mesh._uploaded[id(backend)], backend.uploads
    target = tmp_path / "pictures" / "mesh_and_cameras.png"
    image = mesh.vis(cams, target, return_image=True, window_size=(160, 120), supersample=2)
    from PIL import Image

    assert image.shape == (120, 160, 3) and np.array_equal(np.asarray(Image.open(target)), image)
    legend = json.loads(target.with_suffix(".legend.json").read_text())
    assert list(legend) == [f"class {k}" for k in range(5)] and legend["class 1"] == [255, 127, 14]
    colours = {tuple(c) for c in image.reshape(-1, 3).tolist()}
    assert (255, 255, 255) in colours, "white background"
    assert any(r > 150 and g < 60 and b < 60 for r, g, b in colours) and any(b > 150 and r < 60 and g < 60 for r, g, b in colours), "frusta"
    # the device holds the caller's mesh again: the same arrays, uploaded once more, and the next call uploads nothing
    assert mesh._uploaded[id(backend)][0] is held[0] and mesh._uploaded[id(backend)][1] is held[1] and backend.uploads == uploads + 2
    assert backend.n_faces == len(faces)
    assert np.array_equal(mesh.pix2face(cams[0], render_img_scale=0.1, apply_distortion=False), before) and backend.uploads == uploads + 2
    # occlusion off is another picture; a camera's view is that camera's picture; the file alone returns None
    flat = mesh.vis(cams, return_image=True, window_size=(160, 120), supersample=2, enable_ssao=False)
    assert flat.shape == image.shape and (flat != image).any() and (flat.astype(int) >= image.astype(int)).all()
    through = mesh.vis(None, return_image=True, window_size=(64, 48), supersample=1, view=cams.cameras[0])
    assert through.shape == (48, 64, 3) and not ((through == 255).all(axis=2)).any(), "the nadir camera sees the plane everywhere"
    assert mesh.vis(None, tmp_path / "only.png", window_size=(32, 24), supersample=1) is None and (tmp_path / "only.png").is_file()
    # per-vertex scalars go through vert_to_face_texture; no texture at all is one plain colour under the light
    heights = mesh.vis(None, return_image=True, window_size=(32, 24), supersample=1, vis_scalars=points[:, 2])
    assert heights.shape == (24, 32, 3)


# -- save_renders(make_composites=True) ----------------------------------------------------------------------------------------------
def test_save_renders_composites_on_the_oracle(c1, tmp_path):
    from PIL import Image

    points, faces, cams = c1
    rng = np.random.default_rng(0)
    folder = tmp_path / "images"
    folder.mkdir()
    poses = [np.asarray(c.cam_to_world_transform) for c in cams.cameras[:2]]
    files = []
    for k in range(2):
        files.append(folder / f"view{k}.png")
        Image.fromarray(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)).save(files[-1])
    cameras = [PhotogrammetryCamera(f, pose, 50.0, 0.0, 0.0, 64, 48) for f, pose in zip(files, poses)]
    camera_set = PhotogrammetryCameraSet(cameras=cameras, image_folder=folder)
    mesh = c1_mesh(c1, OraclePictureBackend())
    mesh.save_renders(camera_set, output_folder=tmp_path / "plain", apply_distortion=False, writer_threads=1)
    mesh.save_renders(camera_set, output_folder=tmp_path / "composites", make_composites=True, apply_distortion=False, writer_threads=1)
    for k in range(2):
        label = np.asarray(Image.open(tmp_path / "plain" / f"view{k}.tif"))
        got = np.asarray(Image.open(tmp_path / "composites" / f"view{k}.tif"))
        photo = np.asarray(Image.open(files[k]))
        assert label.shape == (48, 64) and got.shape == (48, 192, 3) and got.dtype == np.uint8
        assert np.array_equal(got, standin_composite(photo / 255.0, label, 0.5, True, mesh.get_IDs_to_labels()))


# -- the entrypoints ---------------------------------------------------------------------------------------------------------------
def aggregate_scene(tmp_path):
    """The mesh file, two C1 cameras with label images, and the arguments of `aggregate_images` (as tests/test_top_down_raster_host.py
    sets them up)."""
    from PIL import Image

    (points, faces), cams = synthetic.config1_scene()
    sub = cams[0:2]
    for i, c in enumerate(sub.cameras):
        c.image_filename = Path(tmp_path, "images", "flight", f"img_{i}.JPG")
    sub.image_folder = Path(tmp_path, "images")
    h, w = sub.cameras[0].get_image_size()
    rng = np.random.default_rng(1)
    (tmp_path / "labels" / "flight").mkdir(parents=True, exist_ok=True)
    for i in range(2):
        blocks = rng.integers(0, 4, (h // 32 + 1, w // 32 + 1)).astype(np.uint8)
        Image.fromarray(np.kron(blocks, np.ones((32, 32), dtype=np.uint8))[:h, :w]).save(tmp_path / "labels" / "flight" / f"img_{i}.png")
    np.savez(tmp_path / "mesh.npz", points=points, faces=faces)
    kw = dict(take_every_nth_camera=1, aggregate_image_scale=0.25, camera_set=sub, IDs_to_labels={0: "a", 1: "b", 2: "c", 3: "d"})
    return (tmp_path / "mesh.npz", None, tmp_path / "images", tmp_path / "labels", "EPSG:4978"), kw, sub


def check_pictures(folder, names, size=(1024, 768)):
    from PIL import Image

    for name in names:
        with Image.open(Path(folder, name)) as image:
            assert image.size == size and image.mode == "RGB", name
            assert len(image.getcolors(maxcolors=1 << 24)) > 8, name
        assert isinstance(json.loads(Path(folder, name).with_suffix(".legend.json").read_text()), dict)


def test_aggregate_images_writes_the_two_pictures(tmp_path):
    from geograypher_amd.entrypoints.aggregate_images import aggregate_images, parse_args

    args, kw, _ = aggregate_scene(tmp_path)
    aggregate_images(*args, vis_folder=tmp_path / "vis", backend=OraclePictureBackend(), **kw)
    check_pictures(tmp_path / "vis", ("mesh_and_cameras.png", "predicted_classes.png"))
    assert set(json.loads((tmp_path / "vis" / "predicted_classes.legend.json").read_text())) == {"a", "b", "c", "d"}
    parsed = parse_args(["--mesh-file", "m.npz", "--mesh-CRS", "EPSG:4978", "--cameras-file", "c.xml", "--image-folder", "i", "--label-folder",
                         "l", "--IDs-to-labels", "ids.json", "--vis-folder", "pictures"])
    assert parsed.vis_folder == Path("pictures")
    with pytest.raises(NotImplementedError, match="vis"):
        aggregate_images(*args, vis=True, backend=None, **kw)


def test_visualize_entrypoint(tmp_path):
    from geograypher_amd.entrypoints import visualize as entry

    (points, faces), cams = synthetic.config1_scene()
    np.savez(tmp_path / "mesh.npz", points=points, faces=faces)
    weights = np.zeros((len(faces), 3))
    weights[np.arange(len(faces)), np.arange(len(faces)) % 3] = 1.0
    weights[:50] = 0.0
    np.save(tmp_path / "weights.npy", weights)
    (tmp_path / "ids.json").write_text('{"0": "fir", "1": "oak", "2": "ash"}')
    parsed = entry.parse_args(["--mesh-file", str(tmp_path / "mesh.npz"), "--mesh-CRS", "EPSG:4978", "--screenshot-filename",
                               str(tmp_path / "out" / "view.png"), "--texture", str(tmp_path / "weights.npy"), "--IDs-to-labels",
                               str(tmp_path / "ids.json"), "--convert-texture-to-max-class", "--window-size", "200", "150", "--supersample",
                               "3", "--azimuth-deg", "90", "--elevation-deg", "60"])
    assert parsed.window_size == [200, 150] and parsed.enable_ssao is True and parsed.camera_file is None
    mesh = entry.visualize(**vars(parsed), camera_set=cams, backend=OraclePictureBackend())
    check_pictures(tmp_path / "out", ("view.png",), size=(200, 150))
    assert json.loads((tmp_path / "out" / "view.legend.json").read_text()).keys() == {"fir", "oak", "ash"}
    assert np.isnan(mesh.face_texture[:50]).all() and set(np.unique(mesh.face_texture[50:]).tolist()) == {0.0, 1.0, 2.0}
    with pytest.raises(SystemExit):
        entry.parse_args(["--mesh-file", "m.npz", "--mesh-CRS", "EPSG:4978"])     # --screenshot-filename is required
