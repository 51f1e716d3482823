"""The picture kernels on the device (csrc/vis.hip) behind fenced and poisoned outputs: the composite against
the reference's own bytes (tests/golden/composites.npz) and, on random images of odd widths, against the numpy stand-in; the shaded
view and the face lights against the stand-in on planes made by numpy.  Every comparison is byte for byte."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import vis_standin as vs  # noqa: E402
from geograypher_amd.utils import colormaps, visualization  # noqa: E402
from tests.fenced_backend import FencedHipRaster, fenced  # noqa: E402
from tests.test_vis_host import golden, golden_case  # noqa: E402,F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    b = FencedHipRaster(0)
    yield b
    b.close()


def _np(t):
    return t.cpu().numpy()


# -- the composite ----------------------------------------------------------------------------------------------------------------
def test_every_golden_case_equals_the_references_bytes(backend, golden):  # noqa: F811
    for name in (str(n) for n in golden["cases"]):
        photo, label, weight, grey, table, want = golden_case(golden, name)
        with fenced(backend):
            got = visualization.create_composite(photo, label, weight, table, grey, backend=backend)
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


def random_composite_case(rng, h, w, kind):
    """-> the arguments of `backend.composite_labels` behind photo and label, numpy."""
    photo = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if kind % 2 == 0 else rng.random((h, w, 3))
    weight, grey = float(rng.choice([0.0, 0.25, 0.5, 1.0])), bool(kind % 3)
    if kind == 0:
        label, table, discrete = rng.integers(0, 14, (h, w), dtype=np.uint8), colormaps.table("tab10"), True
    elif kind == 1:
        label, table, discrete = rng.integers(0, 256, (h, w), dtype=np.uint8), colormaps.table("viridis"), False
    elif kind == 2:
        label, table, discrete = rng.normal(size=(h, w)) * 5.0, colormaps.table("viridis"), False
        label.flat[::7] = 0.0
        label.flat[3::11] = np.nan
    elif kind == 3:
        label, table, discrete = rng.random((h, w, 3)), None, False
    elif kind == 4:
        label, table, discrete = rng.integers(0, 256, (h, w, 3), dtype=np.uint8), None, False
    else:
        label, table, discrete = np.round(rng.random((h, w)) * 24.0) / 20.0, colormaps.table("tab20"), True   # a float plane, discrete
    shift, scale = vs.composite_scalars(label, discrete)
    return photo, label, table, discrete, shift, scale, weight, grey


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (17, 33), (64, 67), (2, 1100)])
def test_random_images_equal_the_standin(backend, h, w):
    """Odd widths: a row of 9 w bytes starts at every alignment, so the bytewise head and tail of every strip are crossed; 1100
    pixels a row are two strips."""
    rng = np.random.default_rng(1000 * h + w)
    for kind in range(6):
        photo, label, table, discrete, shift, scale, weight, grey = random_composite_case(rng, h, w, kind)
        want = vs.composite(photo, label, table, discrete, shift, scale, weight, grey)
        with fenced(backend):
            got = _np(backend.composite_labels(photo, label, table, discrete, shift, scale, weight, grey))
            product_shift, product_scale = visualization.composite_scalars(backend._dev(label, torch.uint8 if label.dtype == np.uint8
                                                                                         else torch.float64), discrete)
        assert (product_shift, product_scale) == (shift, scale) or (np.isnan(shift) and np.isnan(product_shift))
        assert np.array_equal(got, want), (kind, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


def test_inputs_at_every_byte_offset_equal_the_standin(backend):
    """The photo and the label strips come in by 16-byte words: views that start 1 .. 17 bytes into a buffer."""
    rng = np.random.default_rng(77)
    h, w = 5, 37
    photo, label = rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 12, (h, w), dtype=np.uint8)
    table = colormaps.table("tab10")
    want = vs.composite(photo, label, table, True, 0.0, 1.0, 0.5, True)
    for offset in (1, 2, 3, 5, 8, 15, 16, 17):
        buf_p = torch.zeros(photo.size + 64, dtype=torch.uint8, device=backend.device)
        buf_l = torch.zeros(label.size + 64, dtype=torch.uint8, device=backend.device)
        p = buf_p[offset:offset + photo.size].view(h, w, 3)
        lab = buf_l[17 - offset:17 - offset + label.size].view(h, w)
        p.copy_(torch.from_numpy(photo))
        lab.copy_(torch.from_numpy(label))
        with fenced(backend):
            got = _np(backend.composite_labels(p, lab, table, True, 0.0, 1.0, 0.5, True))
        assert np.array_equal(got, want), offset


def test_composite_refusals(backend):
    photo, label = np.zeros((2, 3, 3), dtype=np.uint8), np.zeros((2, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="uint8 colour label with discrete"):
        backend.composite_labels(photo, photo, None, discrete=True)
    with pytest.raises(ValueError, match="label"):
        backend.composite_labels(photo, np.zeros((2, 4), dtype=np.uint8), colormaps.table("tab10"))
    with pytest.raises(ValueError, match="gr_composite_labels"):
        backend.composite_labels(photo, label, np.zeros((0, 3)))


# -- the shaded view --------------------------------------------------------------------------------------------------------------
def shade_planes(rng, H, W, s, n_mesh=40, n_frusta=12):
    """ids and depth of H s x W s samples made by numpy: background (-1, +inf), mesh faces, the faces of appended frusta (the ids
    behind the mesh's), an id beyond the table, equal depths, depths of 1e-3 and 1e6, +inf under a face id."""
    F = n_mesh + n_frusta
    Hs, Ws = H * s, W * s
    ids = rng.integers(-1, F, (Hs, Ws)).astype(np.int32)
    ids[rng.random((Hs, Ws)) < 0.15] = -1
    depth = (np.round(rng.random((Hs, Ws)) * 8.0) / 4.0 + 1.0).astype(np.float32)   # steps of 0.25: many equal neighbours
    flat_i, flat_d = ids.reshape(-1), depth.reshape(-1)
    flat_d[::13] = np.float32(1e-3)
    flat_d[5::17] = np.float32(1e6)
    flat_i[7::29] = F + 3            # beyond the table: background
    flat_i[2::31] = F - 1            # the last face of the frusta
    depth[ids < 0] = np.inf
    flat_d[11::37] = np.inf          # (a face id over an infinite depth: the formula decides)
    rgb = rng.integers(0, 256, (F, 3), dtype=np.uint8)
    rgb[n_mesh:] = (255, 0, 0)
    light = rng.integers(0, 256, (F,), dtype=np.uint8)
    light[:2], light[n_mesh:] = (0, 255), 255
    return ids, depth, rgb, light


@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (33, 9), (65, 17)])
def test_shaded_views_equal_the_standin(backend, W, H):
    """Every tile border (16 output pixels) and every halo is crossed: s in 1 .. 4, r in {1, s, 2 s}."""
    rng = np.random.default_rng(100 * W + H)
    for s in (1, 2, 3, 4):
        ids, depth, rgb, light = shade_planes(rng, H, W, s)
        for r in sorted({1, s, 2 * s}):
            for k in (0.0, 0.75):
                want = vs.shade_view(ids, depth, rgb, light, s, r, k, (250, 251, 252))
                with fenced(backend):
                    got = _np(backend.shade_view(ids, depth, rgb, light, s, r, k, (250, 251, 252)))
                assert got.shape == (H, W, 3) and np.array_equal(got, want), (s, r, k, int((got != want).sum()),
                                                                             np.argwhere(got != want)[:4].tolist())
    if W > 1:   # (the neighbours of a single pixel at r = 2 s all lie outside the planes)
        assert (want != vs.shade_view(ids, depth, rgb, light, s, r, 0.0, (250, 251, 252))).any(), "the occlusion changes the picture"


def test_a_view_without_faces_is_background(backend):
    ids, depth = np.full((4, 6), -1, dtype=np.int32), np.full((4, 6), np.inf, dtype=np.float32)
    with fenced(backend):
        got = _np(backend.shade_view(ids, depth, np.zeros((0, 3), np.uint8), np.zeros((0,), np.uint8), 2, 2, 1.0, (9, 8, 7)))
    assert got.shape == (2, 3, 3) and (got == np.array([9, 8, 7], dtype=np.uint8)).all()


def test_shade_refusals(backend):
    ids, depth = np.zeros((4, 4), np.int32), np.ones((4, 4), np.float32)
    rgb, light = np.zeros((1, 3), np.uint8), np.zeros((1,), np.uint8)
    for kwargs, match in ((dict(supersample=5), "supersample"), (dict(supersample=3), "no picture"), (dict(radius=0), "radius"),
                          (dict(radius=17), "radius"), (dict(strength=-1.0), "strength"), (dict(strength=float("nan")), "strength"),
                          (dict(background=(0, 0, 256)), "background")):
        with pytest.raises(ValueError, match=match):
            backend.shade_view(ids, depth, rgb, light, **{"supersample": 1, **kwargs})
    with pytest.raises(ValueError, match="depth"):
        backend.shade_view(ids, depth[:2], rgb, light)


def test_face_lights_hand_worked_and_random(backend):
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0], [0, 3, 4]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 1], [0, 1, 3], [0, 1, 4], [0, 1, 5], [0, 1, 9]], dtype=np.int32)
    with fenced(backend):
        got = _np(backend.face_light(verts, faces, (0.0, 0.0, -1.0), 0.25))
    assert got.tolist() == [255, 255, 64, 255, 179, 255] == vs.face_light(verts, faces, (0.0, 0.0, -1.0), 0.25).tolist()
    rng = np.random.default_rng(9)
    verts = (rng.normal(size=(300, 3)) * 20.0).astype(np.float32)
    faces = rng.integers(0, 300, (1027, 3)).astype(np.int32)   # more than one workgroup; some faces repeat a vertex
    d = np.array([0.48, -0.6, 0.64])
    for ambient in (0.0, 0.3, 1.0):
        with fenced(backend):
            got = _np(backend.face_light(verts, faces, d, ambient))
        assert np.array_equal(got, vs.face_light(verts, faces, d, ambient)), ambient
    with fenced(backend):
        assert backend.face_light(verts, np.zeros((0, 3), np.int32), d).shape == (0,)
    with pytest.raises(ValueError, match="ambient"):
        backend.face_light(verts, faces, d, 1.5)
