"""`TexturedPhotogrammetryMesh.vis`, `save_renders(make_composites=True)` and the two entrypoints on the device, end to end.  The
picture of the device must equal, byte for byte, the picture the same Python path makes from the CPU oracle's ids and depth with
the numpy stand-in (tests/vis_standin.py) in place of the kernels: that holds only because the id and depth planes of the raster
path are exact against the oracle, so a difference here is a finding about those planes, not a reason for a tolerance."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

from geograypher_amd.cameras import PhotogrammetryCamera, PhotogrammetryCameraSet  # noqa: E402
from tests.fenced_backend import FencedHipRaster, fenced  # noqa: E402
from tests.test_mesh_vis_host import OraclePictureBackend, aggregate_scene, c1, c1_mesh, check_pictures  # noqa: E402,F401
from tests.test_vis_host import standin_composite  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    b = FencedHipRaster(0)
    yield b
    b.close()


def test_the_c1_picture_equals_the_oracle_and_the_standin(backend, c1):  # noqa: F811
    """C1 (9 800 faces, 8 cameras drawn as frusta), 160 x 120 at two samples a side, the default view and one camera's."""
    _, _, cams = c1
    on_device, on_host = c1_mesh(c1, backend), c1_mesh(c1, OraclePictureBackend())
    for shown, kwargs in ((cams, dict()), (cams, dict(enable_ssao=False)), (None, dict(view=cams.cameras[3], supersample=1)),
                          (cams, dict(view=dict(azimuth_deg=10.0, elevation_deg=80.0, view_angle_deg=45.0), supersample=3))):
        kwargs = {"window_size": (160, 120), "supersample": 2, "return_image": True, **kwargs}
        with fenced(backend):
            got = on_device.vis(shown, **kwargs)
        want = on_host.vis(shown, **kwargs)
        assert got.shape == (120, 160, 3) and got.dtype == np.uint8
        assert np.array_equal(got, want), (kwargs, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
        assert len({tuple(c) for c in got.reshape(-1, 3).tolist()}) > 5, kwargs


def test_save_renders_composites_equal_the_standin(backend, c1, tmp_path):  # noqa: F811
    from PIL import Image

    _, _, cams = c1
    rng = np.random.default_rng(0)
    folder = tmp_path / "images"
    folder.mkdir()
    cameras = []
    for k in range(2):
        Image.fromarray(rng.integers(0, 256, (48, 67, 3), dtype=np.uint8)).save(folder / f"view{k}.png")
        cameras.append(PhotogrammetryCamera(folder / f"view{k}.png", np.asarray(cams.cameras[k].cam_to_world_transform), 50.0, 0.0, 0.0, 67, 48))
    camera_set = PhotogrammetryCameraSet(cameras=cameras, image_folder=folder)
    mesh = c1_mesh(c1, backend)
    with fenced(backend):
        mesh.save_renders(camera_set, output_folder=tmp_path / "plain", apply_distortion=False, writer_threads=2)
        mesh.save_renders(camera_set, output_folder=tmp_path / "composites", make_composites=True, apply_distortion=False, writer_threads=2)
    for k in range(2):
        label = np.asarray(Image.open(tmp_path / "plain" / f"view{k}.tif"))
        got = np.asarray(Image.open(tmp_path / "composites" / f"view{k}.tif"))
        photo = np.asarray(Image.open(folder / f"view{k}.png"))
        assert label.shape == (48, 67) and got.shape == (48, 201, 3) and len(np.unique(label)) > 2
        assert np.array_equal(got, standin_composite(photo / 255.0, label, 0.5, True, mesh.get_IDs_to_labels()))


def test_the_entrypoints_write_their_pictures(backend, tmp_path):
    from geograypher_amd.entrypoints import visualize as entry
    from geograypher_amd.entrypoints.aggregate_images import aggregate_images

    args, kw, sub = aggregate_scene(tmp_path)
    aggregate_images(*args, vis_folder=tmp_path / "vis", backend=backend, **kw)
    check_pictures(tmp_path / "vis", ("mesh_and_cameras.png", "predicted_classes.png"))
    entry.visualize(tmp_path / "mesh.npz", "EPSG:4978", None, tmp_path / "out" / "view.png", camera_set=sub, backend=backend,
                    window_size=(320, 200), supersample=2)
    check_pictures(tmp_path / "out", ("view.png",), size=(320, 200))
