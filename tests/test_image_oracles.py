"""The yardsticks of tests/test_image_stage_edges.py, pinned where there is no GPU: the host restatements the image-side kernels
(warp.hip, resize.hip) are compared with, against live scipy at every shape and coordinate of tests/image_edge_cases.py.

  * oracle_warp.sample_grid_constant == scipy.ndimage.map_coordinates(mode="grid-constant", prefilter=False) on finite
    coordinates: order 0 bit for bit, order 1 within 1e-12 * max(1, max |value|); the same NaN pattern for NaN / inf pixels and
    a NaN fill; `fill` on the coordinates scipy leaves undefined (NaN, +-inf)
  * oracle_resize.resize_antialias == the scikit-image >= 0.19 formulation through scipy (gaussian_filter, then zoom with
    grid_mode) within 1e-12 on [0, 1] images
  * the lenses of the inverse-map tests are one-to-one over their images (positive Jacobian determinant)
  * the oracle-backed stand-in refuses reference_float_roundtrip=True where the device path does
"""
import numpy as np
import pytest

from oracle import oracle_resize, oracle_warp
from tests import image_edge_cases as cases

ndi = pytest.importorskip("scipy.ndimage")

FILLS = [0.0, -1.0, 7.0, 7.5, np.nan]


def _scipy_sample(img, m, order, fill):
    return ndi.map_coordinates(img, m, order=order, mode="grid-constant", cval=fill, prefilter=False)


def _images(rng, shape):
    normal = rng.normal(0, 10, shape)
    small = rng.integers(-5, 200, shape).astype(np.float64)
    holes = normal.copy()
    flat = holes.reshape(-1)
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        flat[(rng.permutation(flat.size)[: max(1, flat.size // 7)] + k) % flat.size] = v
    return {"normal": normal, "small": small, "holes": holes}


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("shape", cases.WARP_IN_SHAPES, ids=[f"{h}x{w}" for h, w in cases.WARP_IN_SHAPES])
def test_sample_grid_constant_is_scipy_on_finite_coordinates(shape, order):
    rng = np.random.default_rng(shape[0] * 1009 + shape[1] * 7 + order)
    maps = [cases.edge_map(*shape, finite_only=True), cases.random_map(rng, *shape, 40, 50, non_finite=False)]
    for kind, img in _images(rng, shape).items():
        for m in maps:
            for fill in FILLS:
                with np.errstate(invalid="ignore"):
                    want = _scipy_sample(img, m, order, fill)
                got = oracle_warp.sample_grid_constant(img, m[0], m[1], order, fill)
                assert got.shape == want.shape and got.dtype == np.float64
                np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{kind} fill {fill}")
                keep = ~np.isnan(want)
                if order == 0:
                    assert np.array_equal(got[keep].view(np.uint64), want[keep].view(np.uint64)), (kind, fill)
                else:
                    inf = np.isinf(want)
                    np.testing.assert_array_equal(got[inf], want[inf])
                    fin = keep & ~inf
                    scale = max(1.0, float(np.abs(want[fin]).max())) if fin.any() else 1.0
                    assert np.abs(got[fin] - want[fin]).max(initial=0.0) <= 1e-12 * scale, (kind, fill)


def test_sample_grid_constant_is_total():
    """Where scipy is undefined (NaN, +-inf coordinates) the restatement reads `fill`, in both orders; finite coordinates of the
    same map are unaffected."""
    rng = np.random.default_rng(5)
    img = rng.normal(0, 1, (6, 9))
    m = cases.edge_map(6, 9)
    bad = ~(np.isfinite(m[0]) & np.isfinite(m[1]))
    assert bad.any() and not bad.all()
    m_finite = np.where(np.isfinite(m), m, 0.0)
    for order in (0, 1):
        for fill in FILLS:
            got = oracle_warp.sample_grid_constant(img, m[0], m[1], order, fill)
            ref = oracle_warp.sample_grid_constant(img, m_finite[0], m_finite[1], order, fill)
            assert np.array_equal(got[bad], np.full(int(bad.sum()), fill), equal_nan=True)
            assert np.array_equal(got[~bad], ref[~bad], equal_nan=True)


@pytest.mark.parametrize("dtype", ["uint8", "int16", "int64", "float32", "float64"])
def test_warp_total_is_warp_exact_on_finite_maps(dtype):
    rng = np.random.default_rng(11)
    for shape in ((6, 9), (6, 9, 1), (5, 4, 3), (1, 7, 2)):
        img = rng.integers(0, 200, shape).astype(dtype)
        m = cases.random_map(rng, shape[0], shape[1], 23, 31, non_finite=False, quarters_only=True)
        for order in (0, 1):
            for fill in (0, 7):
                want = oracle_warp.warp_exact(img, m, order, fill)
                got = oracle_warp.warp_total(img, m, order, fill)
                assert got.dtype == want.dtype and got.shape == want.shape
                np.testing.assert_array_equal(got, want)
    const = np.full((4, 5, 3), 7, dtype=dtype)
    got = oracle_warp.warp_total(const, cases.edge_map(4, 5), 1, 7)
    assert got.shape == (4, 5, 3) and got.dtype == const.dtype and (got == 7).all()


# ---- resize -----------------------------------------------------------------------------------------------------------------
def _zoom_like_skimage_019(image, out_hw):
    """skimage >= 0.19 `resize` of a float image: anti-aliasing filter, then ndi.zoom with grid_mode (the oracle's docstring)."""
    factors = [image.shape[0] / out_hw[0], image.shape[1] / out_hw[1]] + [1.0] * (image.ndim - 2)
    sigma = [max(0.0, (f - 1) / 2) for f in factors]
    filtered = ndi.gaussian_filter(image, sigma, mode="mirror")
    return ndi.zoom(filtered, [1 / f for f in factors], order=1, mode="mirror", grid_mode=True, prefilter=False)


def _resize_cases():
    out = [(i, o, C) for i, o in cases.RESIZE_SHAPES for C in cases.RESIZE_CHANNELS]
    out += cases.resize_block_shapes()
    out += [(i, o, C) for i, o in cases.RESIZE_LARGEST_RADIUS for C in (None, 3)]
    return out


@pytest.mark.parametrize("hw_in,hw_out,C", _resize_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_resize_oracle_is_scipy_at_the_edge_shapes(hw_in, hw_out, C):
    rng = np.random.default_rng(hw_in[0] * 7919 + hw_in[1] * 31 + hw_out[0] * 3 + hw_out[1] + (C or 0))
    shape = cases.with_channels(hw_in, C)
    for img in (rng.random(shape), rng.integers(0, 256, shape).astype(np.uint8) / 255.0):
        want = _zoom_like_skimage_019(img, hw_out)
        got = oracle_resize.resize_antialias(img, hw_out)
        assert got.shape == want.shape == cases.with_channels(hw_out, C)
        assert np.abs(got - want).max() <= 1e-12


# ---- lens table -------------------------------------------------------------------------------------------------------------
def test_lens_table_is_one_to_one():
    """The condition of the inverse-map tests, checked here too: every lens they use has a positive Jacobian determinant on
    every pixel at every scale (a fold-over has several inverses, and two Newton variants may pick different ones)."""
    for name, coeffs in cases.one_coefficient_lenses().items():
        for W, H in ((53, 37), (37, 53)):
            for scale in (1.0, 0.5, 0.37, 2.0):
                params = cases.lens(64, W, H, cx=0.3, cy=-0.7, **coeffs)
                h, w = int(H * scale), int(W * scale)
                assert oracle_warp.forward_jacobian_det(params, h, w, scale).min() > 0.2, (name, W, H, scale)


# ---- the stand-in backend refuses what the device path refuses ------------------------------------------------------------
def test_oracle_backend_refuses_unreproduced_float_roundtrip(oracle_backend_cls):
    be = oracle_backend_cls()
    m = be.upload_map(cases.edge_map(4, 5, finite_only=True))
    ids = np.arange(20, dtype=np.int64).reshape(4, 5) - 3
    assert be.warp_image(ids, m, order=0, fill_value=-1, reference_float_roundtrip=True).dtype == np.int64
    for img, order, fill in ((ids, 1, -1), (ids + 2**40, 0, -1), (ids, 0, 0.5), (ids.astype(np.float64), 0, -1)):
        with pytest.raises(NotImplementedError, match="reference_float_roundtrip"):
            be.warp_image(img, m, order=order, fill_value=fill, reference_float_roundtrip=True)
        assert be.warp_image(img, m, order=order, fill_value=fill).shape == (m.shape[1], m.shape[2])
    const = np.full((4, 5), -1, dtype=np.int64)   # the constant-image shortcut comes first, as in the reference
    assert (be.warp_image(const, m, order=1, fill_value=-1, reference_float_roundtrip=True) == -1).all()
