"""360-degree photos without a GPU: the numpy stand-in of the device resampling (tests/equirect_standin.py) against live scipy and
against the reference's own output (tests/golden/reference_equirect.npz, made by tests/golden/make_golden_equirect.py with the real
perspective_from_equirectangular under scikit-image 0.18.3), the host pieces of the package (rotation matrix, rig camera set,
folder entrypoint on the stand-in backend), and the reference's own known-answer test restated."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import equirect_standin as standin  # noqa: E402

from geograypher_amd.cameras import create_rig_cameras_from_equirectangular  # noqa: E402
from geograypher_amd.entrypoints import equirectangular_to_cube_mapped as entry  # noqa: E402
from geograypher_amd.utils.image import (  # noqa: E402
    perspective_from_equirectangular,
    perspectives_from_equirectangular,
    rotate_by_roll_pitch_yaw,
)

GOLDEN = Path(__file__).resolve().parent / "golden"
VIEWS = ("down", "right", "back", "rolled", "os1", "nearest")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN / "reference_equirect.npz") as d:
        return {k: d[k] for k in d.files}


def _view(gold, name):
    fov, yaw, pitch, roll, h, w, os_, order = gold["view_" + name]
    return dict(fov_deg=fov, output_size=(int(h), int(w)), yaw_deg=yaw, pitch_deg=pitch, roll_deg=roll, warp_order=int(order),
                oversample_factor=int(os_))


def _standin(gold, source, name, **kw):
    return standin.perspective_from_equirectangular_np(gold["src_" + source], **_view(gold, name), **kw)


def test_golden_holds_the_cases_it_should(gold):
    assert gold["src_u8"].dtype == np.uint8 and gold["src_u8"].shape[2] == 3
    assert gold["src_f64"].dtype == np.float64 and gold["src_f64"].shape[2] == 2
    assert (gold["src_sat"][:40] == 255).all() and (gold["src_sat"][40:] == gold["src_u8"][40:]).all()
    for s in ("u8", "sat", "f64"):
        assert gold["src_" + s].shape[0] <= 128 and gold["src_" + s].shape[1] <= 256
    faces = {tuple(gold["view_" + n][:3]) for n in ("down", "right", "back")}
    assert faces == {(89.999, 0, -90), (89.999, 90, 0), (89.999, 180, 0)}
    assert all(gold["view_" + n][6] == 4 for n in ("down", "right", "back"))
    assert gold["view_rolled"][3] != 0 and gold["view_rolled"][2] != 0 and gold["view_rolled"][6] == 2
    assert gold["view_rolled"][4] != gold["view_rolled"][5]
    assert gold["view_os1"][6] == 1 and gold["view_nearest"][7] == 0


@pytest.mark.parametrize("source", ["u8", "sat", "f64"])
@pytest.mark.parametrize("name", [v for v in VIEWS if v != "nearest"])
def test_standin_order1_is_bit_equal_to_live_scipy(gold, source, name):
    """The stand-in's four-tap sum, in its order, is scipy.ndimage.map_coordinates(order=1, prefilter=False) on the image with
    the wrap-around column appended -- on every sample, bit for bit."""
    from scipy import ndimage as ndi

    src = gold["src_" + source]
    _, dbg = _standin(gold, source, name, return_debug=True)
    i, j = dbg["ij"]
    vmin, vrange = standin.value_range(src)
    norm = (src.astype(float) - vmin) / vrange
    nfill = (0.0 - vmin) / vrange
    mine = standin.interpolate(norm, i, j, 1, nfill)
    ext = np.concatenate([norm, norm[:, 0:1]], axis=1)
    for ch in range(src.shape[2]):
        ref = ndi.map_coordinates(ext[..., ch], np.stack([i, j]), order=1, prefilter=False, mode="grid-constant", cval=nfill)
        assert np.array_equal(ref, mine[..., ch]), f"{int((ref != mine[..., ch]).sum())} of {ref.size} samples differ"


@pytest.mark.parametrize("name", VIEWS)
def test_standin_equals_the_reference_on_uint8_noise(gold, name):
    out, mask = _standin(gold, "u8", name, return_mask=True)
    want = gold[f"out_u8_{name}"]
    assert out.shape == want.shape and out.dtype == want.dtype
    assert np.array_equal(out, want), f"{int((out != want).sum())} values differ"
    assert np.array_equal(mask, gold[f"mask_u8_{name}"])


@pytest.mark.parametrize("name", VIEWS)
def test_standin_matches_the_reference_on_float64(gold, name):
    out, mask = _standin(gold, "f64", name, return_mask=True)
    want = gold[f"out_f64_{name}"]
    assert out.shape == want.shape and out.dtype == want.dtype == np.float64
    print(name, "max |stand-in - reference| =", np.abs(out - want).max())
    np.testing.assert_allclose(out, want, rtol=0, atol=1e-12)
    assert np.array_equal(mask, gold[f"mask_f64_{name}"])


@pytest.mark.parametrize("name", VIEWS)
def test_standin_within_one_level_of_the_reference_on_the_saturated_image(gold, name):
    """|diff| <= 1 and no tighter: where the image is flat at its maximum the reference's own [0, 1] round trip lands on either
    side of an integer depending on the last bit of scipy's interpolation (DESIGN.md "Equirectangular resampling")."""
    out, mask = _standin(gold, "sat", name, return_mask=True)
    want = gold[f"out_sat_{name}"]
    assert out.shape == want.shape and out.dtype == want.dtype
    diff = np.abs(out.astype(float) - want.astype(float))
    print(name, "max", diff.max(), "differing", int((diff > 0).sum()))
    assert diff.max() <= 1
    assert np.array_equal(mask, gold[f"mask_sat_{name}"])


def test_rotation_matrices_match_the_reference(gold):
    for (roll, pitch, yaw), r3, r4 in zip(gold["rpy"], gold["rot3"], gold["rot4"]):
        np.testing.assert_allclose(rotate_by_roll_pitch_yaw(roll, pitch, yaw), r3, rtol=0, atol=1e-15)
        np.testing.assert_allclose(rotate_by_roll_pitch_yaw(roll, pitch, yaw, return_4x4=True), r4, rtol=0, atol=1e-15)
        np.testing.assert_allclose(standin.rotation_matrix(roll, pitch, yaw), r3, rtol=0, atol=1e-15)
    assert rotate_by_roll_pitch_yaw(1, 2, 3, return_4x4=True).shape == (4, 4)


def test_rig_camera_set_matches_the_reference(gold, tmp_path):
    sys.path.insert(0, str(GOLDEN))
    import make_golden_equirect as recipe

    xml = tmp_path / "camera.xml"
    xml.write_text((GOLDEN / "metashape_camera.xml").read_text())
    rig = create_rig_cameras_from_equirectangular(
        camera_file=xml, original_images="/home/user/image_sets", perspective_images="/data/perspective",
        rig_camera=recipe.RIG_CAMERA, rig_orientations=recipe.RIG_ORIENTATIONS,
        perspective_filename_format_str=recipe.RIG_FORMAT)
    from geograypher_amd.cameras import MetashapeCameraSet

    n_source = len(MetashapeCameraSet(xml, "/data/perspective", original_image_folder="/home/user/image_sets").cameras)
    assert len(rig.cameras) == n_source * len(recipe.RIG_ORIENTATIONS) == len(gold["rig_transforms"])
    got = np.stack([c.cam_to_world_transform for c in rig.cameras])
    assert np.array_equal(got, gold["rig_transforms"])
    assert [str(c.image_filename) for c in rig.cameras] == [str(s) for s in gold["rig_filenames"]]
    assert str(rig.cameras[0].image_filename).endswith("_yaw0_pitch-90_roll0.png")
    assert np.array_equal(np.asarray(rig.get_local_to_epsg_4978_transform(), dtype=float), gold["rig_local_to_epsg_4978"])
    cam = rig.cameras[0]
    assert (cam.f, cam.image_width, cam.image_height) == (960.0, 1920, 1920)


# ---- the reference's own known-answer test (tests/test_images.py:8-86 of the reference), against the stand-in -------------------
def _py_to_xyz(pitch_yaw_deg):
    pitch, yaw = np.deg2rad(pitch_yaw_deg[0]), np.deg2rad(pitch_yaw_deg[1])
    return np.array([np.cos(pitch) * np.cos(yaw), np.cos(pitch) * np.sin(yaw), np.sin(pitch)])


@pytest.mark.parametrize("yaw_deg", [0, 45, 180, 270])
@pytest.mark.parametrize("pitch_deg", [0, 45, 90, -90])
@pytest.mark.parametrize("roll_deg", [0, 30, 45, 180])
def test_equi_to_perspective_known_answer(yaw_deg, pitch_deg, roll_deg):
    """An image whose pixel values are their own (pitch, yaw) in degrees: the centre of a view reads the view's direction."""
    output_size = (101, 151)
    i_samples = np.arange(90 - 0.5, -90, -1)
    j_samples = np.arange(-180 + 0.5, 180, 1)
    img = np.stack(np.meshgrid(i_samples, j_samples, indexing="ij"), axis=-1)
    sample, mask = standin.perspective_from_equirectangular_np(
        img, fov_deg=60, yaw_deg=yaw_deg, pitch_deg=pitch_deg, roll_deg=roll_deg, output_size=output_size, warp_order=0,
        oversample_factor=2, return_mask=True)
    assert sample.shape[:2] == output_size
    assert sample.shape[2] == 2
    assert sample.dtype == float
    assert mask.shape == img.shape[:2]
    assert mask.dtype == bool
    assert np.allclose(_py_to_xyz(sample[50, 75, :]), _py_to_xyz([pitch_deg, yaw_deg]), atol=0.01)


# ---- the Python surface on the stand-in backend ---------------------------------------------------------------------------
def test_surface_on_the_standin_backend_returns_the_reference_shapes_and_dtypes(gold):
    be = standin.StandInBackend()
    for name in VIEWS:
        for s in ("u8", "f64"):
            got = perspective_from_equirectangular(gold["src_" + s], **_view(gold, name), backend=be)
            want = gold[f"out_{s}_{name}"]
            assert got.shape == want.shape and got.dtype == want.dtype
    got, mask = perspective_from_equirectangular(gold["src_u8"], **_view(gold, "rolled"), return_mask=True, backend=be)
    assert np.array_equal(got, gold["out_u8_rolled"]) and np.array_equal(mask, gold["mask_u8_rolled"])


def test_many_views_upload_the_photo_once(gold):
    be = standin.StandInBackend()
    views = [(89.999, 0, -90), (89.999, 90, 0), (70.0, 33.0, 21.0, 17.0)]
    outs = list(perspectives_from_equirectangular(gold["src_u8"], views, output_size=(24, 24), oversample_factor=4, backend=be))
    assert be.equirect_uploads == 1 and len(outs) == 3
    assert np.array_equal(outs[0], gold["out_u8_down"]) and np.array_equal(outs[1], gold["out_u8_right"])


def test_unsupported_orders_and_views_are_refused(gold):
    be = standin.StandInBackend()
    with pytest.raises(NotImplementedError):
        perspective_from_equirectangular(gold["src_u8"], 60.0, output_size=(8, 8), warp_order=2, backend=be)
    with pytest.raises(NotImplementedError):
        perspective_from_equirectangular(gold["src_u8"], 60.0, output_size=(8, 8), warp_order=3, backend=be)
    with pytest.raises(ValueError):
        perspectives_from_equirectangular(gold["src_u8"], [(60.0, 0)], backend=be)
    assert be.equirect_uploads == 0


def test_a_source_without_variation_is_zeros():
    be = standin.StandInBackend()
    out = perspective_from_equirectangular(np.zeros((16, 32, 3), np.uint8), 60.0, output_size=(5, 7), oversample_factor=2,
                                           backend=be)
    assert out.shape == (5, 7, 3) and out.dtype == np.float64 and not out.any()


def test_binding_declares_the_entry_point():
    from geograypher_amd import _hip

    assert "gr_equirect_view" in _hip.EXPORTED_SYMBOLS
    header = (Path(__file__).resolve().parents[1] / "include" / "geograster.h").read_text()
    assert "int gr_equirect_view(gr_ctx *ctx, const void *src, int dtype" in header
    assert "#define GR_VERSION 126" in header


# ---- the folder entrypoint --------------------------------------------------------------------------------------------------
def _photo_folder(root, n, shape=(32, 64, 3)):
    from PIL import Image

    rng = np.random.default_rng(11)
    photos = {}
    for k in range(n):
        sub = root / ("a" if k % 2 == 0 else "b")
        sub.mkdir(parents=True, exist_ok=True)
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        path = sub / f"photo_{k:02d}.png"
        Image.fromarray(img).save(path)
        photos[path] = img
    (root / "notes.txt").write_text("not an image")
    return photos


def test_entrypoint_chips_a_two_photo_folder(tmp_path):
    from PIL import Image

    src, dst = tmp_path / "in", tmp_path / "out"
    photos = _photo_folder(src, 2)
    be = standin.StandInBackend()
    fyps = entry.FYPS[:3]
    last = entry.chip_equirectangular_folder(src, dst, fyps, None, (12, 10), 2, 1, backend=be)
    assert be.equirect_uploads == 2
    written = sorted(p.relative_to(dst).as_posix() for p in dst.rglob("*.png"))
    want_names = sorted(f"{p.parent.name}/{p.stem}_fov90_yaw0_pitch{pitch}.png" for p in photos for pitch in (-90, 90, 0))
    assert written == want_names
    assert np.array_equal(last, photos[sorted(photos)[-1]])
    for path, img in photos.items():
        for fov, yaw, pitch in fyps:
            want = standin.perspective_from_equirectangular_np(img, fov, (12, 10), yaw, pitch, 0, 1, 2).astype(np.uint8)
            got = np.asarray(Image.open(dst / path.parent.name / f"{path.stem}_fov90_yaw{yaw}_pitch{pitch}.png"))
            assert got.dtype == np.uint8 and np.array_equal(got, want)


def test_entrypoint_defaults_are_the_reference_ones():
    assert entry.FYPS == [(90 - 0.001, 0, -90), (90 - 0.001, 0, 90), (90 - 0.001, 0, 0), (90 - 0.001, 90, 0),
                          (90 - 0.001, 180, 0), (90 - 0.001, 270, 0)]
    assert (entry.OVERSAMPLE_FACTOR, entry.WARP_ORDER, entry.OUTPUT_SIZE) == (4, 1, (1920, 1920))
    args = entry.parse_args(["in", "out", "--n-images-to-save", "3", "--seed", "5"])
    assert (args.n_images_to_save, args.seed, args.oversample_factor, args.output_size) == (3, 5, 4, [1920, 1920])


def test_entrypoint_refuses_what_is_out_of_scope(tmp_path):
    src = tmp_path / "in"
    _photo_folder(src, 1)
    be = standin.StandInBackend()
    with pytest.raises(NotImplementedError, match="photogrammetry_cameras_path"):
        entry.chip_equirectangular_folder(src, tmp_path / "out", entry.FYPS, None, (8, 8), 1, 1,
                                          photogrammetry_cameras_path=tmp_path / "cameras.xml", backend=be)
    with pytest.raises(NotImplementedError, match="visualize_mask_sum"):
        entry.visualize_mask_sum(None, entry.FYPS, (8, 8), 1, 1, tmp_path / "sum.png")
    with pytest.raises(NotImplementedError):
        entry.chip_equirectangular_folder(src, tmp_path / "out", entry.FYPS, None, (8, 8), 1, 2, backend=be)
    assert be.equirect_uploads == 0 and not (tmp_path / "out").exists()


def test_entrypoint_seed_makes_the_subset_reproducible(tmp_path):
    src = tmp_path / "in"
    _photo_folder(src, 9, shape=(8, 16, 3))
    a = entry.select_files(src, 3, seed=7)
    b = entry.select_files(src, 3, seed=7)
    assert a == b and len(set(a)) == 3
    every_third = sorted(p for p in src.rglob("*.png"))[::3]
    assert set(a) <= set(every_third)
    draws = {tuple(entry.select_files(src, 3, seed=s)) for s in range(12)}
    assert len(draws) > 1   # the seed matters: the order of the draw changes with it
    be = standin.StandInBackend()
    entry.chip_equirectangular_folder(src, tmp_path / "o1", entry.FYPS[:1], 2, (4, 4), 1, 1, seed=3, backend=be)
    entry.chip_equirectangular_folder(src, tmp_path / "o2", entry.FYPS[:1], 2, (4, 4), 1, 1, seed=3, backend=be)
    names = [sorted(p.relative_to(tmp_path / o).as_posix() for p in (tmp_path / o).rglob("*.png")) for o in ("o1", "o2")]
    assert names[0] == names[1] and len(names[0]) == 2
