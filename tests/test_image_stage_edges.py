"""The image-side kernels (warp.hip: k_warp_nearest_i32, k_warp_f64, k_invert_distortion; resize.hip: k_resize_rows, k_resize_cols,
k_convert_f64) at the edges where kernels go wrong, each against a plain float64 restatement on the host that
tests/test_image_oracles.py pins to live scipy at the same shapes and coordinates (tests/image_edge_cases.py):

  warp      oracle_warp.sample_grid_constant: images of 1 x 1, one row, one column; outputs around one and 256 workgroups; C up
            to 7; every pair of tie / border / huge / non-finite coordinates; every dtype the wrapper takes, both of its paths;
            order 0 bit for bit, order 1 bit-equal values where float64 is exact and 1e-12 * max(1, max |value|) elsewhere
  inverse   oracle_warp.newton_inverse_map (same valid mask, 1e-8 px) and the defining property forward(inverse(p)) = p
            (1e-9 * max(h, w), the kernel's own acceptance bound) over a table of one-to-one lenses, sizes and scales
  resize    oracle_resize.resize_antialias within 1e-12 * max(1, max |value|): filters wider than the image, mixed and
            near-identity scales, block boundaries, the largest radius, the identity path bit for bit, NaN pixels

and the arguments each C entry point must refuse, without a launch."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle_resize, oracle_warp
from tests import image_edge_cases as cases

pytestmark = pytest.mark.gpu


# ---- helpers ------------------------------------------------------------------------------------------------------------
def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _same_bits(got, want):
    """The same NaN positions and the same bits everywhere else (-0.0 is not 0.0)."""
    got, want = _np(got), _np(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    if got.dtype.kind != "f":
        np.testing.assert_array_equal(got, want)
        return
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    keep = ~np.isnan(want)
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.nonzero(got[keep].view(bits) != want[keep].view(bits))[0]
    assert bad.size == 0, f"{bad.size} values differ, first: got {got[keep][bad[0]]!r}, want {want[keep][bad[0]]!r}"


def _same_values(got, want):
    """The same NaN positions and equal values everywhere else (the sign of a zero sum depends on the order of its terms)."""
    got, want = _np(got), _np(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    np.testing.assert_array_equal(got, want)  # NaN == NaN here, position by position


def _close(got, want, rel=1e-12):
    """The same NaN positions and infinities; finite values within rel * max(1, max |finite value|)."""
    got, want = _np(got), _np(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, (got.shape, got.dtype, want.shape, want.dtype)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    inf = np.isinf(want)
    np.testing.assert_array_equal(np.isinf(got), inf)
    np.testing.assert_array_equal(got[inf], want[inf])
    fin = np.isfinite(want)
    if fin.any():
        bound = rel * max(1.0, float(np.abs(want[fin]).max()))
        err = float(np.abs(got[fin] - want[fin]).max())
        assert err <= bound, f"max |diff| {err:.3e} > {bound:.3e}"


def _error(hip, rc, what="call"):
    """The Python exception the binding makes of a return code (ValueError with the library's message for GR_EINVAL)."""
    hip._check(rc, what)


SENTINEL = -12345.0


def _warp_f64_raw(hip, img, m, order, fill, h_in=None, w_in=None, C=None, h_out=None, w_out=None):
    """gr_warp_f64 itself on a float64 (H, W, C) image: (return code, float64 result before any cast).  The output starts as
    SENTINEL everywhere, so a call that must not launch leaves it so."""
    src = torch.as_tensor(np.ascontiguousarray(img, dtype=np.float64)).to(hip.device)
    mt = hip.upload_map(m)
    dims = [int(src.shape[0]), int(src.shape[1]), int(src.shape[2]), int(mt.shape[1]), int(mt.shape[2])]
    for k, v in enumerate((h_in, w_in, C, h_out, w_out)):
        if v is not None:
            dims[k] = v
    out = torch.full((int(mt.shape[1]), int(mt.shape[2]), int(src.shape[2])), SENTINEL, dtype=torch.float64, device=hip.device)
    with torch.cuda.device(hip.device):
        rc = hip.lib.gr_warp_f64(hip._ctx, src.data_ptr(), dims[0], dims[1], dims[2], mt[0].data_ptr(), mt[1].data_ptr(),
                                 dims[3], dims[4], int(order), float(fill), out.data_ptr(), hip._stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _want_f64(img3, m, order, fill):
    return np.stack([oracle_warp.sample_grid_constant(img3[:, :, ch], m[0], m[1], order, fill) for ch in range(img3.shape[2])],
                    axis=-1)


WARP_DTYPES = ["bool", "uint8", "int16", "int32", "int64", "int64_wide", "float32", "float64"]


def _small_integer_image(rng, shape, dtype):
    """Small integers in `dtype` (int64_wide: beyond the int32 range, so that the float path is taken), never constant."""
    if dtype == "bool":
        img = rng.random(shape) < 0.5
        img.reshape(-1)[0] = True
        return img
    lo = 0 if dtype == "uint8" else -5
    img = rng.integers(lo, 200, shape).astype("int64" if dtype == "int64_wide" else dtype)
    if dtype == "int64_wide":
        img = img + np.where(rng.random(shape) < 0.5, 2**40, -(2**40))
        img.reshape(-1)[0] = 2**40 + 3
    else:
        img.reshape(-1)[0] = 3
    return img


def _fills(dtype):
    if dtype in ("bool", "uint8"):
        return [0, 7, 7.5]
    if dtype.startswith("int"):
        return [0, -1, 7, 7.5]
    return [0, -1, 7, 7.5, np.nan]


# ---- warp: every pair of edge coordinates, every dtype ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WARP_DTYPES)
@pytest.mark.parametrize("shape", cases.WARP_IN_SHAPES, ids=[f"{h}x{w}" for h, w in cases.WARP_IN_SHAPES])
def test_warp_every_edge_coordinate_pair(hip, shape, dtype):
    """Order 0 bit for bit.  Order 1 on small integers at multiples of 1/4 (and at huge / non-finite coordinates, which read the
    fill value): every product and sum is exact in float64, so the values equal the restatement's whatever the order of the
    operations, integer dtypes included (a 7.5 fill takes integer images through the float path)."""
    rng = np.random.default_rng(shape[0] * 1009 + shape[1] * 7 + len(dtype))
    img = _small_integer_image(rng, shape, dtype)
    for order in (0, 1):
        m = cases.edge_map(*shape, quarters_only=order == 1)
        assert m.shape[1] * m.shape[2] % 256 != 0 and np.isinf(m).any() and np.isnan(m).any()
        mt = hip.upload_map(m)
        for fill in _fills(dtype):
            got = hip.warp_image(img, mt, order=order, fill_value=fill)
            want = oracle_warp.warp_total(img, m, order, fill)
            assert isinstance(got, np.ndarray)
            if order == 0:
                _same_bits(got, want)
            else:
                _same_values(got, want)
    # tensor in -> tensor out, cast on the device
    t = torch.as_tensor(img).to(hip.device)
    got = hip.warp_image(t, mt, order=1, fill_value=7)
    assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == t.dtype
    _same_values(got, oracle_warp.warp_total(img, m, 1, 7).reshape(got.shape))


# ---- warp: bilinear on general values, NaN / inf pixels ---------------------------------------------------------------------
@pytest.mark.parametrize("pixels", ["normal", "non_finite"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 1), (6, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_warp_general_values(hip, shape, dtype, pixels):
    """gr_warp_f64's float64 result (for float32 images: before the wrapper's cast) against the restatement: the same NaN
    pattern and infinities, finite values within 1e-12 * max(1, max |finite value|); order 0 bit for bit."""
    rng = np.random.default_rng(shape[0] * 31 + shape[1] + (dtype == "float32") * 1000 + (pixels == "normal") * 7)
    for C in cases.WARP_CHANNELS:
        img = (rng.normal(0, 10, shape + (C,)) * np.exp(rng.uniform(-2, 4))).astype(dtype)
        if pixels == "non_finite":
            flat = img.reshape(-1)
            for k, v in enumerate((np.nan, np.inf, -np.inf)):
                flat[(rng.permutation(flat.size)[: max(1, flat.size // 7)] + k) % flat.size] = v
        img64 = img.astype(np.float64)
        for m in (cases.edge_map(*shape), cases.random_map(rng, *shape, 7, 13)):
            for fill in (0.0, -1.0, 7.5, np.nan):
                for order in (0, 1):
                    rc, got = _warp_f64_raw(hip, img64, m, order, fill)
                    assert rc == 0
                    want = _want_f64(img64, m, order, fill)
                    _same_bits(got, want) if order == 0 else _close(got, want)
        # the wrapper returns that result in the image's dtype
        mt = hip.upload_map(m)
        got = hip.warp_image(img, mt, order=1, fill_value=7.5)
        _, raw = _warp_f64_raw(hip, img64, m, 1, 7.5)
        _same_bits(got, np.squeeze(raw.astype(dtype)))


# ---- warp: output shapes and channel counts --------------------------------------------------------------------------------
@pytest.mark.parametrize("out_shape", cases.WARP_OUT_SHAPES, ids=[f"{h}x{w}" for h, w in cases.WARP_OUT_SHAPES])
def test_warp_output_shapes_and_channels(hip, out_shape):
    """Outputs that differ from the input in shape, around one and 256 workgroups, for every channel count: k_warp_f64 splits
    its flat index by C, the int32 path gathers plane by plane."""
    rng = np.random.default_rng(out_shape[0] * 65537 + out_shape[1])
    for C in cases.WARP_CHANNELS:
        in_shape = (3, 257) if C % 2 else (6, 9)
        m = cases.random_map(rng, *in_shape, *out_shape, quarters_only=True)
        mt = hip.upload_map(m)
        ids = rng.integers(-5, 200, in_shape + (C,)).astype(np.int32)
        _same_bits(hip.warp_image(ids, mt, order=0, fill_value=-1), oracle_warp.warp_total(ids, m, 0, -1))
        img = ids.astype(np.float64)
        for order in (0, 1):
            rc, got = _warp_f64_raw(hip, img, m, order, -1.0)
            assert rc == 0 and got.shape == out_shape + (C,)
            want = _want_f64(img, m, order, -1.0)
            _same_bits(got, want) if order == 0 else _same_values(got, want)
        if C in (1, 3):  # (H, W, 1) is squeezed like the reference's np.squeeze, (H, W) stays
            _same_values(hip.warp_image(img, mt, order=1, fill_value=-1), np.squeeze(want))


# ---- warp: the reference's float round trip ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("shape", [(1, 7), (5, 1), (6, 9), (6, 9, 3)], ids=lambda s: "x".join(map(str, s)))
def test_reference_float_roundtrip_at_ties_and_borders(hip, shape, dtype):
    """reference_float_roundtrip=True on id images with negative ids and fill -1 is flexible_inputs_warp_reference bit for bit
    wherever the sample position lies inside the input (oracle_warp.inside_mask), at every tie and border coordinate."""
    rng = np.random.default_rng(len(shape) * 100 + shape[0] + (dtype == "int64"))
    img = rng.integers(-7, 3000, shape).astype(dtype)
    img.reshape(-1)[:2] = (-7, 2999)
    for m in (cases.edge_map(shape[0], shape[1], finite_only=True),
              cases.random_map(rng, shape[0], shape[1], 19, 23, non_finite=False)):
        got = hip.warp_image(img, hip.upload_map(m), order=0, fill_value=-1, reference_float_roundtrip=True)
        with np.errstate(invalid="ignore"):
            ref = oracle_warp.flexible_inputs_warp_reference(img, m, 0, -1)
        inside = oracle_warp.inside_mask(m, shape)
        assert got.dtype == ref.dtype == np.dtype(dtype) and got.shape == ref.shape and inside.any()
        np.testing.assert_array_equal(got[inside], ref[inside])


def test_reference_float_roundtrip_is_refused_where_it_is_not_reproduced(hip):
    """Only the int32 kernel implements the round trip: order 1, an integer image beyond the int32 range, a non-integer fill and
    a float image raise NotImplementedError instead of silently returning the exact gather (the oracle-backed stand-in of
    the CPU suite refuses the same combinations, tests/test_image_oracles.py)."""
    m = cases.edge_map(4, 5, finite_only=True)
    mt = hip.upload_map(m)
    ids = np.arange(20, dtype=np.int64).reshape(4, 5) - 3
    for img, order, fill in ((ids, 1, -1), (ids + 2**40, 0, -1), (ids, 0, 0.5), (ids.astype(np.float64), 0, -1),
                             (torch.as_tensor(ids).to(hip.device), 1, -1)):
        with pytest.raises(NotImplementedError, match="reference_float_roundtrip"):
            hip.warp_image(img, mt, order=order, fill_value=fill, reference_float_roundtrip=True)
        exact = hip.warp_image(img, mt, order=order, fill_value=fill)  # without the flag the same call is served
        _same_values(_np(exact), oracle_warp.warp_total(_np(img), m, order, fill))
    const = np.full((4, 5), -1, dtype=np.int64)  # the constant-image shortcut comes first, as in the reference
    assert (hip.warp_image(const, mt, order=1, fill_value=-1, reference_float_roundtrip=True) == -1).all()


# ---- warp: constant images, refusals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["uint8", "int64", "float32"])
@pytest.mark.parametrize("shape", [(4, 5), (4, 5, 1), (4, 5, 3)], ids=lambda s: "x".join(map(str, s)))
def test_constant_image_shortcut_shape_and_dtype(hip, shape, dtype):
    """utils/image.py:86-96: an image without variation (fill included) comes back as a constant of the squeezed INPUT shape
    and the input dtype, whatever the map's shape; numpy in -> numpy out, tensor in -> tensor out."""
    mt = hip.upload_map(cases.edge_map(9, 11))
    img = np.full(shape, 7, dtype=dtype)
    for order in (0, 1):
        got = hip.warp_image(img, mt, order=order, fill_value=7)
        assert isinstance(got, np.ndarray) and got.dtype == img.dtype and got.shape == np.squeeze(img).shape and (got == 7).all()
        t = torch.as_tensor(img).to(hip.device)
        got = hip.warp_image(t, mt, order=order, fill_value=7)
        assert isinstance(got, torch.Tensor) and got.dtype == t.dtype and got.device == t.device
        assert tuple(got.shape) == tuple(t.squeeze().shape) and bool((got == 7).all())
    # one pixel of variation, or a different fill, and the map's shape is back
    assert hip.warp_image(img, mt, order=0, fill_value=0).shape[:2] == tuple(mt.shape[1:])


def test_warp_refusals(hip):
    """Each is a Python exception with the library's message, and none is a launch (the output keeps its sentinel)."""
    m = cases.edge_map(4, 5)
    img = np.arange(20, dtype=np.float64).reshape(4, 5, 1)
    for order in (2, -1, 3):
        rc, out = _warp_f64_raw(hip, img, m, order, 0.0)
        assert rc == -1 and (out == SENTINEL).all()
        with pytest.raises(ValueError, match=f"interpolation order {order} not supported"):
            _error(hip, rc)
        for wimg in (img, img.astype(np.int32), img.astype(np.uint8)[..., 0]):  # no integer kernel takes it either
            with pytest.raises(ValueError, match=f"interpolation order {order} not supported"):
                hip.warp_image(wimg, hip.upload_map(m), order=order, fill_value=0)
    for kw in ({"h_in": 0}, {"w_in": 0}, {"C": 0}, {"h_out": 0}, {"w_out": 0}, {"h_in": -4}):
        rc, out = _warp_f64_raw(hip, img, m, 1, 0.0, **kw)
        assert rc == -1 and (out == SENTINEL).all(), kw
        with pytest.raises(ValueError, match="bad warp args"):
            _error(hip, rc)
    # gr_warp_nearest_i32: zero sizes, and a non-positive value range with the round trip (the wrapper never passes one)
    mt = hip.upload_map(m)
    src = torch.arange(20, dtype=torch.int32, device=hip.device).reshape(4, 5)
    out = torch.full(tuple(mt.shape[1:]), int(SENTINEL), dtype=torch.int32, device=hip.device)

    def nearest(h_in=4, w_in=5, h_out=int(mt.shape[1]), w_out=int(mt.shape[2]), roundtrip=0, value_range=19.0):
        with torch.cuda.device(hip.device):
            return hip.lib.gr_warp_nearest_i32(hip._ctx, src.data_ptr(), h_in, w_in, mt[0].data_ptr(), mt[1].data_ptr(), h_out,
                                               w_out, -1, roundtrip, 0.0, value_range, out.data_ptr(), hip._stream())

    for kw in ({"h_in": 0}, {"w_in": 0}, {"h_out": 0}, {"w_out": 0}):
        with pytest.raises(ValueError, match="bad warp args"):
            _error(hip, nearest(**kw))
    for bad_range in (0.0, -3.0, float("nan")):
        with pytest.raises(ValueError, match="value_range must be positive"):
            _error(hip, nearest(roundtrip=1, value_range=bad_range))
    assert nearest(roundtrip=0, value_range=0.0) == 0  # without the round trip the range is not read
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), oracle_warp.warp_total(src.cpu().numpy(), m, 0, -1))
    out.fill_(int(SENTINEL))
    for kw in ({"h_in": 0}, {"roundtrip": 1, "value_range": 0.0}):
        assert nearest(**kw) == -1
    torch.cuda.synchronize()
    assert bool((out == int(SENTINEL)).all())
    # a sampling map that is not (2, H, W)
    for bad in (np.zeros((3, 4, 5)), np.zeros((4, 5)), np.zeros((2, 4, 5, 1))):
        with pytest.raises(ValueError, match=r"sampling map must be \(2, H, W\)"):
            hip.upload_map(bad)
    with pytest.raises(ValueError, match=r"image must be \(I,J\) or \(I,J,C\)"):
        hip.warp_image(np.zeros((2, 2, 2, 2)), mt)


# ---- lens inverse --------------------------------------------------------------------------------------------------------------
def _grid(h, w):
    return np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")


def _check_inverse(hip, params, h, w, scale, max_iters=12, fill=-1.0, compare_newton=True):
    """The one-to-one condition, then the kernel against the numpy Newton solver (identical valid masks, 1e-8 px) and against
    the defining property in float64 (1e-9 * max(h, w) on every valid pixel).  Returns (map, valid)."""
    assert oracle_warp.forward_jacobian_det(params, h, w, scale).min() > 0, "lens folds over: replace it"
    got = hip.invert_distortion(params, h, w, scale, max_iters=max_iters, fill=fill).cpu().numpy()
    assert got.shape == (2, h, w) and got.dtype == np.float64
    if compare_newton:
        want = oracle_warp.newton_inverse_map(dict(params), h, w, scale, iters=max_iters, fill=-1.0)
        valid = want[0] != -1.0
        # identical masks: `fill` (NaN equal to NaN) on every pixel the solver rejects, its solution on every other
        np.testing.assert_array_equal(got[:, ~valid], np.full((2, int((~valid).sum())), fill))
        np.testing.assert_allclose(got[:, valid], want[:, valid], rtol=0, atol=1e-8)
    else:
        valid = ~np.isnan(got[0]) if np.isnan(fill) else got[0] != fill
    ti, tj = _grid(h, w)
    fr, fc = oracle_warp.forward_map_position(params, got[0], got[1], scale)
    bound = 1e-9 * max(h, w)
    assert np.abs(fr - ti)[valid].max(initial=0.0) < bound and np.abs(fc - tj)[valid].max(initial=0.0) < bound
    r, c = got[0][valid], got[1][valid]
    assert r.size == 0 or (r.min() >= 0 and r.max() <= h - 1 and c.min() >= 0 and c.max() <= w - 1)
    return got, valid


LENS_SIZES = [(1, 1), (1, 9), (9, 1), (15, 17), (16, 16), (1, 257), (257, 1), (65537, 1), (37, 53), (53, 37)]
SCALES = [1.0, 1.0 + 1e-6, 1.0 + 2e-5, 0.5, 0.37, 2.0]


@pytest.mark.parametrize("hw", LENS_SIZES, ids=[f"{h}x{w}" for h, w in LENS_SIZES])
def test_pinhole_inverse_is_the_identity_bit_for_bit(hip, hw):
    """All coefficients 0, cx = cy = 0, unit scale (1 + 1e-6 is still numpy.isclose to 1): the identity bit for bit, every pixel
    valid, row h - 1 and column w - 1 included.  (f is a power of two, so the forward model itself is exact.)"""
    h, w = hw
    ti, tj = _grid(h, w)
    for f in (64.0, 1024.0):
        for scale in (1.0, 1.0 + 1e-6):
            for iters in (1, 12, 64):
                got = hip.invert_distortion(cases.lens(f, w, h), h, w, scale, max_iters=iters).cpu().numpy()
                _same_bits(got, np.stack([ti, tj]))
    got, valid = _check_inverse(hip, cases.lens(64.0, w, h), h, w, 1.0)
    assert valid.all()


@pytest.mark.parametrize("shift", [(1, 0), (-1, 0), (0, 3), (0, -3), (3, -1), (-3, 1), (0.5, 0), (0, -0.5), (2.5, 1.5), (-1.5, -2.5)],
                         ids=lambda s: f"cx{s[0]}_cy{s[1]}")
def test_principal_point_shift_is_the_shifted_identity(hip, shift):
    """cx, cy alone: inverse(i, j) = (i - cy, j - cx) exactly, and exactly the rows and columns shifted out of the image hold
    `fill`; at half-integer shifts the last valid row / column is the one `r <= h - 1` admits."""
    cx, cy = shift
    for h, w in ((8, 11), (16, 16), (1, 9), (9, 1), (37, 53)):
        ti, tj = _grid(h, w)
        r, c = ti - cy, tj - cx
        ok = (r >= 0) & (r <= h - 1) & (c >= 0) & (c <= w - 1)
        for fill in (-1.0, 0.0, np.nan):
            got = hip.invert_distortion(cases.lens(128.0, w, h, cx=cx, cy=cy), h, w, 1.0, fill=fill).cpu().numpy()
            _same_bits(got, np.stack([np.where(ok, r, fill), np.where(ok, c, fill)]))
        # (the finite-difference solver is no yardstick on r = 0 exactly: the closed form above is; the property still holds)
        _check_inverse(hip, cases.lens(128.0, w, h, cx=cx, cy=cy), h, w, 1.0, compare_newton=False)
    # dyadic scales keep the arithmetic exact: the half-pixel convention of cameras.py:1012-1043 shifts the identity by 0.5
    for scale in (0.5, 2.0):
        H, W = 16, 24
        h, w = int(H * scale), int(W * scale)
        ti, tj = _grid(h, w)
        r, c = ti - 0.5 - cy * scale, tj - 0.5 - cx * scale
        ok = (r >= 0) & (r <= h - 1) & (c >= 0) & (c <= w - 1)
        got = hip.invert_distortion(cases.lens(128.0, W, H, cx=cx, cy=cy), h, w, scale).cpu().numpy()
        _same_bits(got, np.stack([np.where(ok, r, -1.0), np.where(ok, c, -1.0)]))


LENSES = cases.one_coefficient_lenses()


@pytest.mark.parametrize("scale", SCALES, ids=lambda s: f"s{s!r}")
@pytest.mark.parametrize("name", list(LENSES))
def test_lens_table_against_newton_and_round_trip(hip, name, scale):
    """Each coefficient alone with both signs, then all eight, at non-square sizes both ways and every scale: the unit-scale
    test (numpy.isclose) switches the pixel-centre convention exactly where forward_map_position does."""
    for W, H in ((53, 37), (37, 53)):
        params = cases.lens(64, W, H, cx=0.3, cy=-0.7, **LENSES[name])
        h, w = int(H * scale), int(W * scale)
        got, valid = _check_inverse(hip, params, h, w, scale)
        assert valid.mean() > 0.5
        if scale == 1.0 + 1e-6:  # still the unit-scale convention: the same bits as scale 1
            _same_bits(got, hip.invert_distortion(params, h, w, 1.0).cpu().numpy())
        if scale == 1.0 + 2e-5:  # no longer: the half-pixel convention moves the map by about half a pixel
            unit = hip.invert_distortion(params, h, w, 1.0).cpu().numpy()
            both = valid & (unit[0] != -1)
            assert 0.4 < np.abs(got - unit)[:, both].mean() < 0.6


def test_unit_scale_switch_is_numpy_isclose(hip):
    """|scale - 1| <= 1e-8 + 1e-5 on both sides of the bound, above and below 1."""
    params = cases.lens(64, 53, 37, cx=0.3, cy=-0.7, **cases.FULL_LENS)
    unit = hip.invert_distortion(params, 37, 53, 1.0).cpu().numpy()
    for scale in (1 + 1.0009e-5, 1 - 1.0009e-5, 1 + 1.0011e-5, 1 - 1.0011e-5):
        h, w = 37, 53  # the caller's int(37 * scale) is 36 below 1: the kernel takes h and w as given
        got, valid = _check_inverse(hip, params, h, w, scale)
        assert bool(np.isclose(scale, 1.0)) == (abs(scale - 1) < 1.001e-5)
        if np.isclose(scale, 1.0):
            _same_bits(got, unit)
        else:
            assert 0.4 < np.abs(got - unit)[:, valid & (unit[0] != -1)].mean() < 0.6


@pytest.mark.parametrize("hw", LENS_SIZES, ids=[f"{h}x{w}" for h, w in LENS_SIZES])
def test_lens_inverse_sizes(hip, hw):
    """One pixel, one row, one column, h * w around one workgroup and past 65536, with the full lens (its principal point off the
    pixel grid, so that no solution sits on the border of a one-pixel-wide image by construction)."""
    h, w = hw
    for scale in (1.0, 0.5, 0.37):
        H, W = (h, w) if scale == 1.0 else (int(np.ceil(h / scale)), int(np.ceil(w / scale)))
        assert (int(H * scale), int(W * scale)) == (h, w)
        f = float(max(64, H, W))
        for coeffs in ({}, cases.FULL_LENS):
            _check_inverse(hip, cases.lens(f, W, H, cx=0.3, cy=-0.7, **coeffs), h, w, scale)


@pytest.mark.parametrize("fill", [-1.0, 0.0, float("nan")], ids=["fill-1", "fill0", "fillnan"])
def test_lens_inverse_fill_and_iteration_limits(hip, fill):
    params = cases.lens(64, 53, 37, cx=0.3, cy=-0.7, **cases.FULL_LENS)
    ref, valid = _check_inverse(hip, params, 37, 53, 1.0)
    assert 0.5 < valid.mean() < 1.0  # both kinds of pixel are present
    got, _ = _check_inverse(hip, params, 37, 53, 1.0, fill=fill)
    _same_bits(got, np.where(valid, ref, fill))
    # 64 iterations: converged long before, the same solution
    got64, valid64 = _check_inverse(hip, params, 37, 53, 1.0, max_iters=64, fill=fill)
    np.testing.assert_array_equal(valid64, valid)
    np.testing.assert_allclose(got64[:, valid], ref[:, valid], rtol=0, atol=1e-8)
    # 1 iteration: whatever the kernel accepts meets the property, is accepted at 12 too and lies within the first step's
    # quadratic error of it; an affine lens (b1, b2, cx, cy) is solved by that one step
    got1, valid1 = _check_inverse(hip, params, 37, 53, 1.0, max_iters=1, compare_newton=False)
    assert not (valid1 & ~valid).any()
    np.testing.assert_allclose(got1[:, valid1], ref[:, valid1], rtol=0, atol=1e-6)
    affine = cases.lens(64, 53, 37, cx=0.3, cy=-0.7, b1=0.5, b2=-0.3)
    a12, v12 = _check_inverse(hip, affine, 37, 53, 1.0)
    a1, v1 = _check_inverse(hip, affine, 37, 53, 1.0, max_iters=1, compare_newton=False)
    np.testing.assert_array_equal(v1, v12)
    np.testing.assert_allclose(a1[:, v12], a12[:, v12], rtol=0, atol=1e-8)


def test_lens_inverse_refusals(hip):
    good = cases.lens(64, 53, 37, k1=0.05)
    hip.invert_distortion(good, 37, 53, 1.0, max_iters=1)
    hip.invert_distortion(good, 37, 53, 1.0, max_iters=64)
    for kw in ({"max_iters": 0}, {"max_iters": 65}, {"max_iters": -1}, {"image_scale": 0.0}, {"image_scale": -1.0},
               {"image_scale": float("nan")}, {"h": 0}, {"w": 0}):
        args = {"h": 37, "w": 53, "image_scale": 1.0, "max_iters": 12, **kw}
        with pytest.raises(ValueError, match="bad lens-inversion args"):
            hip.invert_distortion(good, **args)
    for key in ("f", "image_width", "image_height"):
        for bad in (0.0, -64.0, float("nan")):
            with pytest.raises(ValueError, match="focal length and image size must be positive"):
                hip.invert_distortion({**good, key: bad}, 37, 53, 1.0)
    with pytest.raises(ValueError, match=r"Unexpected distortion params found: \['k5'\]"):
        hip.invert_distortion({**good, "k5": 0.1}, 37, 53, 1.0)
    # no launch: the C entry point leaves the caller's buffers alone
    out = torch.full((2, 37, 53), SENTINEL, dtype=torch.float64, device=hip.device)
    par = (ctypes.c_double * 13)(*[float(good.get(k, 0.0)) for k in hip.LENS_PARAMS])
    for iters, scale in ((0, 1.0), (65, 1.0), (12, 0.0)):
        with torch.cuda.device(hip.device):
            rc = hip.lib.gr_invert_distortion_f64(hip._ctx, par, 37, 53, scale, iters, -1.0, out[0].data_ptr(), out[1].data_ptr(),
                                                  hip._stream())
        assert rc == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- resize -----------------------------------------------------------------------------------------------------------------
def _resize_want(raw, hw_out, divide_by_255):
    src = raw.astype(np.float64) / 255.0 if divide_by_255 else raw.astype(np.float64)
    return oracle_resize.resize_antialias(src, hw_out) if tuple(hw_out) != raw.shape[:2] else src


def _check_resize(hip, hw_in, hw_out, C, rng, dtypes=("uint8", "float32", "float64"), divs=(None, True, False)):
    shape = cases.with_channels(hw_in, C)
    for dtype in dtypes:
        raw = cases.resize_image_values(rng, shape, dtype)
        for div in (divs if dtype == "uint8" else (None,)):
            got = hip.resize_image(raw, hw_out, divide_by_255=div).cpu().numpy()
            want = _resize_want(raw, hw_out, dtype == "uint8" and div is not False)
            assert got.shape == cases.with_channels(hw_out, C)
            _close(got, want)


@pytest.mark.parametrize("C", cases.RESIZE_CHANNELS, ids=lambda c: f"C{c}")
@pytest.mark.parametrize("hw_in,hw_out", cases.RESIZE_SHAPES, ids=[f"{a}x{b}-{c}x{d}" for (a, b), (c, d) in cases.RESIZE_SHAPES])
def test_resize_edge_shapes(hip, hw_in, hw_out, C):
    """Filters wider than the image (the mirror index wraps several periods), one axis shrinking while the other grows or
    stays, near-identity scales, single rows and columns: every channel count and file dtype, /255 both ways."""
    rng = np.random.default_rng(hw_in[0] * 7919 + hw_in[1] * 31 + hw_out[0] * 3 + hw_out[1] + (C or 0))
    if hw_in[0] * hw_in[1] > 50000:  # (the host restatement takes seconds here: one file dtype per channel count, in turn)
        _check_resize(hip, hw_in, hw_out, C, rng, dtypes=(("float64", "uint8", "float32")[(C or 0) % 3],), divs=(None,))
    else:
        _check_resize(hip, hw_in, hw_out, C, rng)
    if C == 3:  # tensor input, on the device already
        raw = cases.resize_image_values(rng, cases.with_channels(hw_in, C), "float32")
        _close(hip.resize_image(torch.as_tensor(raw).to(hip.device), hw_out).cpu().numpy(), _resize_want(raw, hw_out, False))


BLOCK_SHAPES = cases.resize_block_shapes()


@pytest.mark.parametrize("hw_in,hw_out,C", BLOCK_SHAPES,
                         ids=[f"{a}x{b}-{c}x{d}-C{C}" for (a, b), (c, d), C in BLOCK_SHAPES])
def test_resize_block_boundaries(hip, hw_in, hw_out, C):
    """w_in * C and w_out * C at 255 / 256 / 257: the last lane of a 256-wide block, a full block, one lane of the next."""
    ch = C or 1
    assert any(abs(n * ch - 256) <= 1 for n in (hw_in[1], hw_out[1]))
    _check_resize(hip, hw_in, hw_out, C, np.random.default_rng(hw_in[1] * 1000 + hw_out[1] + ch))


@pytest.mark.parametrize("hw_in,hw_out", cases.RESIZE_LARGEST_RADIUS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resize_largest_filter_radius(hip, hw_in, hw_out):
    """Radius 1023 and 1024 (the library's limit), on rows and on columns."""
    rng = np.random.default_rng(hw_in[0] + hw_in[1])
    for C in (None, 3):
        _check_resize(hip, hw_in, hw_out, C, rng, dtypes=("uint8", "float64") if C else ("float32",), divs=(None,))


def test_resize_refusals(hip):
    out = torch.full((12, 4), SENTINEL, dtype=torch.float64, device=hip.device)
    for hw_in, hw_out in cases.RESIZE_RADIUS_TOO_LARGE:
        with pytest.raises(ValueError, match="anti-aliasing kernel radius 1025 exceeds 1024"):
            hip.resize_image(np.zeros(hw_in), hw_out)
    with pytest.raises(ValueError, match="resize to 32768 rows: at most 32767"):
        hip.resize_image(np.zeros((4, 2)), (32768, 2))
    assert hip.resize_image(np.ones((4, 2)), (32767, 2)).shape == (32767, 2)
    for hw_out in ((0, 3), (3, 0), (-1, 3)):
        src = torch.zeros((4, 2), dtype=torch.float64, device=hip.device)
        with torch.cuda.device(hip.device):
            rc = hip.lib.gr_resize_image_f64(hip._ctx, src.data_ptr(), 2, 4, 2, 1, 0, hw_out[0], hw_out[1], out.data_ptr(),
                                             hip._stream())
        with pytest.raises(ValueError, match="bad resize args"):
            _error(hip, rc)
    src = torch.zeros((6160, 4), dtype=torch.float64, device=hip.device)
    with torch.cuda.device(hip.device):
        for args in ((2, 6160, 4, 1, 0, 12, 4), (3, 6160, 4, 1, 0, 12, 4), (2, 6160, 4, 0, 0, 12, 4), (2, 0, 4, 1, 0, 12, 4)):
            assert hip.lib.gr_resize_image_f64(hip._ctx, src.data_ptr(), *args, out.data_ptr(), hip._stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())  # none was a launch
    with pytest.raises(ValueError, match=r"image must be \(H,W\) or \(H,W,C\)"):
        hip.resize_image(np.zeros((4,)))


@pytest.mark.parametrize("shape", [(1, 1), (1, 255), (256, 1), (1, 257), (16, 16, 1), (5, 17, 3), (3, 51, 5), (4, 32, 2)],
                         ids=lambda s: "x".join(map(str, s)))
def test_resize_identity_path_is_bit_exact(hip, shape):
    """Equal sizes are the conversion alone: uint8 / 255.0 is numpy's division for all 256 values (not a multiplication by the
    reciprocal), float32 is widened exactly, float64 is copied bit for bit, NaN payloads included."""
    rng = np.random.default_rng(sum(shape))
    n = int(np.prod(shape))
    u8 = np.resize(np.arange(256, dtype=np.uint8), n).reshape(shape)
    if n < 256:
        u8 = rng.integers(0, 256, shape).astype(np.uint8)
    for out_hw in (None, shape[:2]):
        _same_bits(hip.resize_image(u8, out_hw), u8 / 255.0)
        _same_bits(hip.resize_image(u8, out_hw, divide_by_255=False), u8.astype(np.float64))
        _same_bits(hip.resize_image(u8.astype(bool), out_hw, divide_by_255=False), u8.astype(bool).astype(np.float64))
    f32 = rng.normal(0, 1, shape).astype(np.float32) * np.float32(1e3)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-45, 3.4028235e38, -1e-38], dtype=np.float32)
    f32.reshape(-1)[: min(n, special.size)] = special[: min(n, special.size)]
    _same_bits(hip.resize_image(f32), f32.astype(np.float64))
    f64 = rng.normal(0, 1, shape)
    payloads = np.array([0x7FF8000000000123, 0xFFF8000000000000, 0x7FF0000000000001, 0x7FF0000000000000, 0x8000000000000000,
                         0x0000000000000001], dtype=np.uint64).view(np.float64)
    f64.reshape(-1)[: min(n, payloads.size)] = payloads[: min(n, payloads.size)]
    got = hip.resize_image(f64).cpu().numpy()
    assert got.shape == f64.shape and np.array_equal(got.view(np.uint64), f64.view(np.uint64))
    i16 = rng.integers(-300, 300, shape).astype(np.int16)  # every other dtype is widened, values kept
    _same_bits(hip.resize_image(i16), i16.astype(np.float64))


def test_resize_identity_uint8_all_values(hip):
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 256)
    got = hip.resize_image(u8).cpu().numpy()
    _same_bits(got, u8 / 255.0)
    assert (got != u8 * (1.0 / 255.0)).any()  # the two roundings differ for some value: the division is what is pinned


@pytest.mark.parametrize("hw_in,hw_out", [((40, 50), (13, 17)), ((7, 9), (15, 20)), ((5, 70), (9, 11)), ((30, 4), (7, 4)),
                                          ((1, 300), (1, 7)), ((9, 9), (2, 2))], ids=lambda s: f"{s[0]}x{s[1]}")
def test_resize_non_finite_pixels(hip, hw_in, hw_out):
    """A NaN pixel poisons exactly the outputs whose taps reach it (a tap of weight 0 included: 0 * NaN), +-inf pixels give inf
    or, where both signs meet, NaN: the pattern is the oracle's and the finite outputs stay within tolerance."""
    rng = np.random.default_rng(hw_in[0] * 100 + hw_in[1])
    for C in (None, 3):
        shape = cases.with_channels(hw_in, C)
        for dtype in ("float32", "float64"):
            for kind in ("nan", "inf", "mixed"):
                raw = cases.resize_image_values(rng, shape, dtype)
                flat = raw.reshape(-1)
                vals = {"nan": [np.nan], "inf": [np.inf], "mixed": [np.nan, np.inf, -np.inf]}[kind]
                for v in vals:
                    flat[rng.integers(0, flat.size, 2)] = v
                with np.errstate(invalid="ignore"):
                    want = _resize_want(raw, hw_out, False)
                got = hip.resize_image(raw, hw_out).cpu().numpy()
                _close(got, want)
                if kind == "nan" and max(hw_in) >= 30 and hw_out != (1, 7):
                    assert np.isnan(want).any() and not np.isnan(want).all()


def test_resize_scratch_reuse(hip):
    """A large scratch, then a small one, on one context: the second result does not depend on what the first left in the rows
    buffer."""
    rng = np.random.default_rng(77)
    small = rng.normal(0, 1, (9, 9, 2))
    big = rng.normal(0, 1, (200, 260, 3)) * 1e6
    big.reshape(-1)[::97] = np.nan
    before = hip.resize_image(small, (2, 2)).cpu().numpy()
    with np.errstate(invalid="ignore"):
        _close(hip.resize_image(big, (150, 65)).cpu().numpy(), oracle_resize.resize_antialias(big, (150, 65)))
    after = hip.resize_image(small, (2, 2)).cpu().numpy()
    _same_bits(after, before)
    _close(after, oracle_resize.resize_antialias(small, (2, 2)))
    for hw_in, hw_out in (((1, 300), (1, 7)), ((40, 3), (3, 9))):
        img = rng.normal(0, 1, hw_in)
        _close(hip.resize_image(img, hw_out).cpu().numpy(), oracle_resize.resize_antialias(img, hw_out))
