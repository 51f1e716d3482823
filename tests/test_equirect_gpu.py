"""360-degree photos on the device: gr_equirect_view (csrc/equirect.hip) behind geograypher_amd.utils.image against the numpy
stand-in (tests/equirect_standin.py, itself pinned to the reference and to live scipy by tests/test_equirect_host.py) and against
the reference's own output (tests/golden/reference_equirect.npz).

What may differ between the device and numpy is the last bits of atan2 / asin / sqrt / divide, i.e. the sampling coordinates by a
few ulp (bounded here at 1e-9 px); everything behind the coordinates is the same IEEE arithmetic in the same order.  So:
  * order 1, uint8: a sample can only change where its value before truncation lies within 1e-6 of an integer (1e-9 px times a
    texel step of at most 255 levels is 3e-7 levels) -- by one level.  Pixels with such a sample are left out of the equality
    check (never of the |diff| <= 1 check), and their share is asserted to stay under 2 %.
  * order 0: the value does not depend on the coordinate except through the choice of the tap, floor(x + 0.5); a sample can
    only change where i + 0.5 or j + 0.5 lies within 1e-9 of an integer.  Those are left out (same 2 % cap); every other pixel is
    equal.  (The value-near-an-integer rule cannot be applied to order 0: every order-0 sample of a uint8 image IS an integer.)
  * masks: a source pixel may only differ where every sample that could set it lies within 1e-9 of a rounding tie (cap 0.1 %)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import equirect_standin as standin  # noqa: E402

from geograypher_amd.utils.image import (  # noqa: E402
    perspective_from_equirectangular,
    perspectives_from_equirectangular,
)

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
VIEWS = ("down", "right", "back", "rolled", "os1", "nearest")
COORD_ATOL = 1e-9   # px: device vs numpy transcendental functions, three orders above the ~1e-12 px they differ by at W <= 8192


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN / "reference_equirect.npz") as d:
        return {k: d[k] for k in d.files}


def _view(gold, name):
    fov, yaw, pitch, roll, h, w, os_, order = gold["view_" + name]
    return dict(fov_deg=fov, output_size=(int(h), int(w)), yaw_deg=yaw, pitch_deg=pitch, roll_deg=roll, warp_order=int(order),
                oversample_factor=int(os_))


def _device_view(hip, src, view, return_mask=False, return_debug=False):
    """The backend call behind perspective_from_equirectangular, with the debug output the public function does not expose."""
    x, y = standin.view_axes(view["fov_deg"], view["output_size"], view["oversample_factor"])
    rot = standin.rotation_matrix(view["roll_deg"], view["pitch_deg"], view["yaw_deg"])
    source = hip.equirect_upload(src)
    return hip.equirect_view(source, x, y, rot, view["output_size"], view["oversample_factor"], view["warp_order"],
                             return_mask=return_mask, return_debug=return_debug)


def _near_tie(v):
    return np.abs((v + 0.5) - np.rint(v + 0.5)) < COORD_ATOL


def _doubtful_pixels(dbg, os_, order):
    """(out_h, out_w) bool: output pixels with a sample the device may legitimately resolve differently (module docstring)."""
    if order == 0:
        i, j = dbg["ij"]
        bad = _near_tie(i) | _near_tie(j)
    else:
        pre = dbg["pre"]
        bad = (np.abs(pre - np.rint(pre)) < 1e-6).any(axis=-1)
    ny, nx = bad.shape
    return bad.reshape(ny // os_, os_, nx // os_, os_).any(axis=(1, 3))


def _check_u8(label, dev, want, doubtful, order, cap=0.02):
    """`want`: the stand-in's output or the golden.  Prints the figures, then asserts."""
    assert dev.shape == want.shape and dev.dtype == want.dtype, (dev.shape, want.shape, dev.dtype, want.dtype)
    diff = np.abs(dev.astype(float) - want.astype(float))
    differs = diff.reshape(diff.shape[0], diff.shape[1], -1).max(axis=-1) > 0
    share = doubtful.mean()
    print(f"{label}: max |diff| {diff.max():.4g}, pixels differing {int(differs.sum())}, left out {int(doubtful.sum())} "
          f"({100 * share:.3f} %)")
    assert share <= cap, f"{label}: {100 * share:.3f} % of the pixels left out of the equality check (cap {100 * cap} %)"
    assert not (differs & ~doubtful).any(), f"{label}: {int((differs & ~doubtful).sum())} pixels differ outside the left-out set"
    if order == 1:
        assert diff.max() <= 1, f"{label}: max |diff| {diff.max()}"


def _check_mask(label, dev_mask, ij, H, W, want=None):
    """`want`: the reference's mask; default: the stand-in's."""
    i, j = ij
    if want is None:
        want = standin.sampling_mask(i, j, H, W)
    assert dev_mask.shape == want.shape == (H, W) and dev_mask.dtype == bool
    tie = (np.abs(np.abs(i - np.floor(i)) - 0.5) < COORD_ATOL) | (np.abs(np.abs(j - np.floor(j)) - 0.5) < COORD_ATOL)
    sure = standin.sampling_mask(i[~tie], j[~tie], H, W) if (~tie).any() else np.zeros((H, W), bool)
    maybe = np.zeros((H, W + 1), bool)
    for fi in (np.floor, np.ceil):
        for fj in (np.floor, np.ceil):
            maybe[fi(i[tie]).astype(int), fj(j[tie]).astype(int)] = True
    maybe[:, 0] |= maybe[:, -1]
    doubtful = maybe[:, :-1] & ~sure
    wrong = dev_mask != want
    print(f"{label}: mask pixels set {int(want.sum())}, differing {int(wrong.sum())}, left out {int(doubtful.sum())}")
    assert doubtful.mean() <= 0.001
    assert not (wrong & ~doubtful).any(), f"{label}: {int((wrong & ~doubtful).sum())} mask pixels differ"


@pytest.mark.parametrize("source", ["u8", "f64"])
@pytest.mark.parametrize("name", VIEWS)
def test_debug_coordinates_match_the_standin(hip, gold, name, source):
    view = _view(gold, name)
    src = gold["src_" + source]
    _, _, dbg = _device_view(hip, src, view, return_mask=True, return_debug=True)
    _, want = standin.perspective_from_equirectangular_np(src, **view, return_debug=True)
    assert dbg["ij"].shape == want["ij"].shape and dbg["ij"].dtype == np.float64
    err = np.abs(dbg["ij"] - want["ij"]).max()
    print(f"{name}/{source}: max coordinate difference {err:.3e} px")
    assert err <= COORD_ATOL


@pytest.mark.parametrize("name", VIEWS)
def test_float64_source_matches_standin_and_reference(hip, gold, name):
    view = _view(gold, name)
    src = gold["src_f64"]
    dev, mask = perspective_from_equirectangular(src, **view, return_mask=True, backend=hip)
    want, dbg = standin.perspective_from_equirectangular_np(src, **view, return_debug=True)
    _, vrange = standin.value_range(src)
    assert dev.shape == want.shape and dev.dtype == np.float64
    keep = np.ones(dev.shape[:2], bool)
    if view["warp_order"] == 0:
        keep = ~_doubtful_pixels(dbg, view["oversample_factor"], 0)
        assert (~keep).mean() <= 0.02
    e_standin = np.abs(dev - want)[keep].max()
    e_golden = np.abs(dev - gold[f"out_f64_{name}"])[keep].max()
    print(f"{name}: max |device - stand-in| {e_standin:.3e}, max |device - reference| {e_golden:.3e}, bound {1e-8 * vrange:.3e}")
    assert e_standin <= 1e-8 * vrange
    assert e_golden <= 1e-8 * vrange
    _check_mask(name + " vs stand-in", mask, dbg["ij"], *src.shape[:2])
    _check_mask(name + " vs reference", mask, dbg["ij"], *src.shape[:2], want=gold[f"mask_f64_{name}"])


@pytest.mark.parametrize("name", VIEWS)
def test_uint8_noise_matches_standin_and_reference(hip, gold, name):
    view = _view(gold, name)
    src = gold["src_u8"]
    dev, mask = perspective_from_equirectangular(src, **view, return_mask=True, backend=hip)
    want, dbg = standin.perspective_from_equirectangular_np(src, **view, return_debug=True)
    doubtful = _doubtful_pixels(dbg, view["oversample_factor"], view["warp_order"])
    _check_u8(f"{name} vs stand-in", dev, want, doubtful, view["warp_order"])
    _check_u8(f"{name} vs reference", dev, gold[f"out_u8_{name}"], doubtful, view["warp_order"])
    _check_mask(name + " vs stand-in", mask, dbg["ij"], *src.shape[:2])
    _check_mask(name + " vs reference", mask, dbg["ij"], *src.shape[:2], want=gold[f"mask_u8_{name}"])


@pytest.mark.parametrize("name", VIEWS)
def test_saturated_source_within_one_level(hip, gold, name):
    view = _view(gold, name)
    src = gold["src_sat"]
    dev = perspective_from_equirectangular(src, **view, backend=hip)
    want = standin.perspective_from_equirectangular_np(src, **view)
    for label, ref in (("stand-in", want), ("reference", gold[f"out_sat_{name}"])):
        assert dev.shape == ref.shape and dev.dtype == ref.dtype
        diff = np.abs(dev.astype(float) - ref.astype(float))
        print(f"{name} vs {label}: max |diff| {diff.max():.4g}, differing {int((diff > 0).sum())}")
        assert diff.max() <= 1


def test_realistic_size_six_views_one_upload(hip):
    """A 2048 x 4096 x 3 uint8 photo, the six views of the entrypoint's rig at 480 x 480 and 4x oversampling."""
    from geograypher_amd.entrypoints.equirectangular_to_cube_mapped import FYPS

    rng = np.random.default_rng(2048)
    src = rng.integers(0, 256, size=(2048, 4096, 3), dtype=np.uint8)
    before = hip.equirect_uploads
    views = list(perspectives_from_equirectangular(src, FYPS, output_size=(480, 480), oversample_factor=4, backend=hip))
    assert hip.equirect_uploads - before == 1
    assert len(views) == 6
    for (fov, yaw, pitch), dev in zip(FYPS, views):
        want, dbg = standin.perspective_from_equirectangular_np(src, fov, (480, 480), yaw, pitch, 0, 1, 4, return_debug=True)
        assert dev.shape == (480, 480, 3) and dev.dtype == np.float64
        _check_u8(f"yaw {yaw} pitch {pitch}", dev, want, _doubtful_pixels(dbg, 4, 1), 1)


def test_validation(hip, gold):
    src = gold["src_u8"]
    out = perspective_from_equirectangular(src, 60.0, output_size=(9, 11), backend=hip)
    assert out.dtype == np.uint8 and out.shape == (9, 11, 3)
    out = perspective_from_equirectangular(gold["src_f64"], 60.0, output_size=(9, 11), backend=hip)
    assert out.dtype == np.float64 and out.shape == (9, 11, 2)
    out = perspective_from_equirectangular(src[..., 0], 60.0, output_size=(9, 11), oversample_factor=2, backend=hip)
    assert out.dtype == np.float64 and out.shape == (9, 11)
    with pytest.raises(NotImplementedError):
        perspective_from_equirectangular(src, 60.0, output_size=(9, 11), warp_order=2, backend=hip)
    with pytest.raises(NotImplementedError):
        perspective_from_equirectangular(src.astype(np.float32), 60.0, output_size=(9, 11), backend=hip)
    zeros = perspective_from_equirectangular(np.zeros((16, 32, 3), np.uint8), 60.0, output_size=(5, 7), oversample_factor=2,
                                             backend=hip)
    assert zeros.shape == (5, 7, 3) and zeros.dtype == np.float64 and not zeros.any()
    # the C entry point refuses what the binding never sends it
    import ctypes

    source = hip.equirect_upload(src)
    R = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    p = source.tensor.data_ptr()
    args = lambda dtype, order: (hip._ctx, p, dtype, 96, 192, 3, p, p, R, 4, 4, 1, order, 0.0, 255.0, p, p, None, None, None)  # noqa: E731
    assert hip.lib.gr_equirect_view(*args(1, 1)) == -1    # GR_DTYPE_F32 is not built
    assert hip.lib.gr_equirect_view(*args(0, 2)) == -1    # order 2
    # five channels: more than one launch keeps in registers
    rng = np.random.default_rng(5)
    src5 = rng.random((32, 64, 5))
    dev = perspective_from_equirectangular(src5, 70.0, output_size=(10, 12), yaw_deg=40, pitch_deg=10, oversample_factor=2,
                                           backend=hip)
    want = standin.perspective_from_equirectangular_np(src5, 70.0, (10, 12), 40, 10, 0, 1, 2)
    assert np.abs(dev - want).max() <= 1e-8


CHAIN_XML = """<?xml version="1.0" encoding="UTF-8"?>
<document version="2.0.0">
  <chunk label="Chunk 1" enabled="true">
    <sensors next_id="1">
      <sensor id="0" label="spherical" type="spherical">
        <resolution width="128" height="64"/>
      </sensor>
    </sensors>
    <components next_id="1" active_id="0">
      <component id="0" label="Component 1">
        <transform>
          <rotation locked="true">1 0 0 0 1 0 0 0 1</rotation>
          <translation locked="true">0 0 0</translation>
          <scale locked="true">1</scale>
        </transform>
      </component>
    </components>
    <cameras next_id="2" next_group_id="1">
      <camera id="0" sensor_id="0" component_id="0" label="{root}/photo_00.png">
        <transform>1 0 0 -0.3 0 -1 0 0.1 0 0 -1 3 0 0 0 1</transform>
      </camera>
      <camera id="1" sensor_id="0" component_id="0" label="{root}/photo_01.png">
        <transform>1 0 0 0.4 0 -1 0 -0.2 0 0 -1 3 0 0 0 1</transform>
      </camera>
    </cameras>
  </chunk>
</document>
"""


def test_whole_chain_chip_rig_pix2face(hip, tmp_path):
    """Chip a two-photo folder, build the rig camera set for the views that were written, rasterize a plane below the cameras."""
    from PIL import Image

    from geograypher_amd.cameras import create_rig_cameras_from_equirectangular
    from geograypher_amd.entrypoints.equirectangular_to_cube_mapped import chip_equirectangular_folder
    from geograypher_amd.meshes import TexturedPhotogrammetryMesh
    from geograypher_amd.utils import synthetic

    photos, chips = tmp_path / "photos", tmp_path / "chips"
    photos.mkdir()
    rng = np.random.default_rng(3)
    for k in range(2):
        Image.fromarray(rng.integers(0, 256, size=(64, 128, 3), dtype=np.uint8)).save(photos / f"photo_{k:02d}.png")
    size, f = 64, 100.0
    fov = float(np.rad2deg(2 * np.arctan(size / 2 / f)))
    orientations = [{"roll_deg": 0, "pitch_deg": 0, "yaw_deg": 0}, {"roll_deg": 0, "pitch_deg": 0, "yaw_deg": 8}]
    fyps = [(fov, o["yaw_deg"], o["pitch_deg"]) for o in orientations]
    chip_equirectangular_folder(photos, chips, fyps, None, (size, size), 2, 1, backend=hip)
    xml = tmp_path / "cameras.xml"
    xml.write_text(CHAIN_XML.format(root=photos))
    rig = create_rig_cameras_from_equirectangular(
        camera_file=xml, original_images=photos, perspective_images=chips,
        rig_camera={"f": f, "cx": 0.0, "cy": 0.0, "image_width": size, "image_height": size}, rig_orientations=orientations,
        perspective_filename_format_str="_fov%d_yaw{yaw_deg:.0f}_pitch{pitch_deg:.0f}" % int(round(fov)))
    assert len(rig.cameras) == 4
    for cam in rig.cameras:
        chip = np.asarray(Image.open(cam.image_filename))
        assert chip.shape == (size, size, 3) and chip.dtype == np.uint8
    (mesh, _colors) = synthetic.make_simple_mesh([], None)
    tm = TexturedPhotogrammetryMesh(mesh, log_level="ERROR")
    ids = tm.pix2face(rig, apply_distortion=False)
    assert ids.shape == (4, size, size) and ids.dtype == np.int64
    n_faces = len(mesh[1])
    assert (ids >= 0).all() and (ids < n_faces).all()   # the plane of side 4 fills every view from 3 above it
    assert len(np.unique(ids[0])) > 100 and not np.array_equal(ids[0], ids[1])
