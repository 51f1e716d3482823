"""numpy stand-in of the raster -> raster call (include/geograster_warp.h): the same operations in the same
order, float64 with every operation rounded on its own, and `tests/crs_standin.reproject` for the CRS step W3.  Same-CRS results
equal the device's byte for byte (only +, x, /, floor take part); cross-CRS results agree where the conversion's error cannot flip
a floor: `warp` also returns the mask of the cells where it could ("undetermined").

`WarpStandinBackend` has the `warp_raster` and `reproject_points` of `HipRaster` on the host, so the Python layers above the
binding run without a GPU."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))

import crs_standin as cs  # noqa: E402

NEAREST, BILINEAR = 0, 1
STAT_NAMES = ("cells", "outside", "nonfinite", "beyond", "nodata", "den_zero")
STAT_WORDS = 8
DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.float32): 1, np.dtype(np.float64): 2}
# what a conversion error can move a source coordinate by: twice the 5e-7 m ceiling of DESIGN 8k on the device's error
DELTA_M = 1e-6
DELTA_DEG = 1e-6 / cs.A_WGS84 * 180.0 / np.pi


def to_dtype(value, dtype):
    """W7: float64 values -> the destination's type."""
    dtype = np.dtype(dtype)
    value = np.asarray(value, dtype=np.float64)
    if dtype == np.uint8:
        with np.errstate(invalid="ignore"):
            q = np.floor(value + 0.5)
            q = np.where(q >= 0.0, np.minimum(q, 255.0), 0.0)   # NaN: 0
        return q.astype(np.uint8)
    with np.errstate(over="ignore"):
        return value.astype(dtype)


def centres(dst_transform, window):
    """W2 -> (x, y), each (height, width)."""
    a, b, c0, d, e, f0 = (np.float64(t) for t in dst_transform)
    col_off, row_off, width, height = (int(k) for k in window)
    col = (col_off + np.arange(width, dtype=np.int64)).astype(np.float64)[None, :] + 0.5
    row = (row_off + np.arange(height, dtype=np.int64)).astype(np.float64)[:, None] + 0.5
    return (a * col + b * row) + c0, (d * col + e * row) + f0


def source_units(x, y, src_inverse):
    """W4"""
    ia, ib, ic, id_, ie, if_ = (np.float64(t) for t in src_inverse)
    return (ia * x + ib * y) + ic, (id_ * x + ie * y) + if_


def warp(data, src_inverse, src_nodata, dst_transform, window, src_crs=None, dst_crs=None, resampling=NEAREST, dst_nodata=0.0,
         dst_dtype=None):
    """data (B, H, W) uint8 / float32 / float64; src_crs, dst_crs: gr_crs tuples (kind, lon0, k0, FE, FN) or both None (same CRS)
    -> (out (B, height, width) of dst_dtype, stats (8,) int64, undetermined (height, width) bool, per-cell masks dict)."""
    data = np.asarray(data)
    assert data.ndim == 3 and data.dtype in DTYPES
    B, H, W = data.shape
    dst_dtype = np.dtype(data.dtype if dst_dtype is None else dst_dtype)
    col_off, row_off, width, height = (int(k) for k in window)
    x, y = centres(dst_transform, window)
    status = np.zeros((height, width), dtype=np.int64)
    cross = src_crs is not None or dst_crs is not None
    if cross:
        pts = np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], axis=1)
        conv, st = cs.reproject(pts, tuple(dst_crs), tuple(src_crs))
        x, y, status = conv[:, 0].reshape(x.shape), conv[:, 1].reshape(x.shape), np.asarray(st).reshape(x.shape)
    ok = status == cs.OK
    with np.errstate(all="ignore"):
        u, v = source_units(x, y, src_inverse)
    ia, ib, _, id_, ie, _ = (abs(float(t)) for t in src_inverse)
    delta = 0.0 if not cross else (DELTA_DEG if src_crs[0] == cs.KIND_NAMES.index("geo") else DELTA_M)
    nd = np.float64(dst_nodata)
    src = data.astype(np.float64)
    is_nd = np.isnan(src) if src_nodata is None else (np.isnan(src) | (src == np.float64(src_nodata)))
    value = np.full((B, height, width), nd, dtype=np.float64)
    with np.errstate(all="ignore"):
        if resampling == NEAREST:
            uu, vv = u, v
            cf, rf = np.floor(u), np.floor(v)
            inside = ok & (cf >= 0) & (cf < W) & (rf >= 0) & (rf < H)
            outside = ok & ~inside
            ci, ri = np.where(inside, cf, 0).astype(np.int64), np.where(inside, rf, 0).astype(np.int64)
            s, bad = src[:, ri, ci], is_nd[:, ri, ci]
            value = np.where(inside[None] & ~bad, s, nd)
            met_nodata = inside & bad.any(axis=0)
            den_zero = np.zeros_like(inside)
        else:
            uu, vv = u - 0.5, v - 0.5
            c0, r0 = np.floor(uu), np.floor(vv)
            fx, fy = uu - c0, vv - r0
            cin = (ok & (c0 >= 0) & (c0 < W), ok & (c0 >= -1) & (c0 < W - 1.0))
            rin = ((r0 >= 0) & (r0 < H), (r0 >= -1) & (r0 < H - 1.0))
            cidx = (np.where(cin[0], c0, 0).astype(np.int64), np.where(cin[1], c0 + 1, 0).astype(np.int64))
            ridx = (np.where(rin[0], r0, 0).astype(np.int64), np.where(rin[1], r0 + 1, 0).astype(np.int64))
            gx, gy = 1.0 - fx, 1.0 - fy
            weights = (gx * gy, fx * gy, gx * fy, fx * fy)
            num, den = np.zeros((B, height, width)), np.zeros((B, height, width))
            taking = np.zeros((B, height, width), dtype=np.int64)
            any_in = np.zeros((height, width), dtype=bool)
            met_nodata = np.zeros((height, width), dtype=bool)
            for k, (rk, ck) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                tap_in = rin[rk] & cin[ck]
                any_in |= tap_in
                s, bad = src[:, ridx[rk], cidx[ck]], is_nd[:, ridx[rk], cidx[ck]]
                part = tap_in[None] & ~bad
                met_nodata |= (tap_in[None] & bad).any(axis=0)
                num = np.where(part, num + weights[k][None] * np.where(part, s, 0.0), num)
                den = np.where(part, den + weights[k][None], den)
                taking += part
            outside = ok & ~any_in
            zero = any_in[None] & (den == 0.0)
            den_zero = zero.any(axis=0)
            value = np.where(any_in[None] & ~zero, np.where(taking == 4, num, num / den), nd)
        # the cells whose floor (and with it the cell, or the taps) an error of `delta` in the source coordinates could flip
        undetermined = ok & ((np.abs(uu - np.rint(uu)) < delta * (ia + ib)) | (np.abs(vv - np.rint(vv)) < delta * (id_ + ie)))
    stats = np.zeros(STAT_WORDS, dtype=np.int64)
    masks = dict(outside=outside, nonfinite=status == cs.NONFINITE, beyond=status == cs.BEYOND, nodata=met_nodata, den_zero=den_zero)
    stats[0] = width * height
    for k, name in enumerate(STAT_NAMES[1:], start=1):
        stats[k] = int(masks[name].sum())
    masks["u"], masks["v"] = u, v
    return to_dtype(value, dst_dtype), stats, undetermined, masks


def bilinear_tap_range(data, src_inverse, u, v):
    """(max tap - min tap) of band values over the four taps of every cell that lie in the raster, (B, h, w); 0 where none does."""
    src = np.asarray(data, dtype=np.float64)
    B, H, W = src.shape
    with np.errstate(all="ignore"):
        c0, r0 = np.floor(u - 0.5), np.floor(v - 0.5)
    lo, hi = np.full((B,) + u.shape, np.inf), np.full((B,) + u.shape, -np.inf)
    for dr in (0, 1):
        for dc in (0, 1):
            with np.errstate(all="ignore"):
                r, c = r0 + dr, c0 + dc
                inside = (r >= 0) & (r < H) & (c >= 0) & (c < W)
            s = src[:, np.where(inside, r, 0).astype(np.int64), np.where(inside, c, 0).astype(np.int64)]
            s = np.where(inside[None] & np.isfinite(s), s, np.nan)
            lo, hi = np.fmin(lo, s), np.fmax(hi, s)
    return np.where(np.isfinite(hi - lo), hi - lo, 0.0)


class WarpStandinBackend(cs.CrsStandinBackend):
    """`HipRaster.warp_raster` (and, inherited, `reproject_points`) on the host, with the binding's argument rules."""

    def warp_raster(self, data, src_inverse, src_nodata, dst_transform, window, *, src_crs=None, dst_crs=None, resampling="nearest",
                    dst_nodata=None, dst_dtype=None, out=None):
        from geograypher_amd import _hip
        from geograypher_amd.utils.geospatial import crs_tuple

        data = np.asarray(data.cpu() if hasattr(data, "cpu") else data)
        if data.ndim == 2:
            data = data[None]
        if data.dtype not in DTYPES:
            data = data.astype(np.float64)
        kind = {"nearest": NEAREST, "bilinear": BILINEAR}.get(resampling)
        if kind is None:
            raise ValueError(f"gr_warp_raster: resampling={resampling!r} is neither 'nearest' nor 'bilinear'")
        dst_dtype = np.dtype(data.dtype if dst_dtype is None else _hip.warp_numpy_dtype(dst_dtype))
        _hip.check_warp_window(data.shape, *window, dst_dtype=dst_dtype)
        nd = _hip.warp_dst_nodata(dst_nodata, src_nodata, dst_dtype)
        same = src_crs is None and dst_crs is None
        if (src_crs is None) != (dst_crs is None):
            raise ValueError("gr_warp_raster: src_crs and dst_crs are given together or not at all")
        got, stats, _und, _masks = warp(data, src_inverse, src_nodata, dst_transform, window, None if same else crs_tuple(src_crs),
                                        None if same else crs_tuple(dst_crs), kind, nd, dst_dtype)
        if out is not None:
            out[...] = got
            got = out
        return got, stats


# -- the three cross-CRS scenes of the tests ----------------------------------------------------------------------------------------
UTM10, UTM11, GEO = 32610, 32611, 4326
SCENE_SRC_TRANSFORM = (0.5, 0.0, 552000.3, 0.0, -0.5, 4182014.7)


def scene_source(dtype=np.float32, bands=1, seed=5):
    """29 x 37 cells of 0.5 m in UTM zone 10 north: a smooth field plus noise, so that neighbours differ."""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(29.0), np.arange(37.0), indexing="ij")
    data = np.stack([100.0 + 3.0 * np.sin(c / 5.0 + b) + 2.0 * np.cos(r / 4.0) + rng.normal(size=(29, 37)) for b in range(bands)])
    if np.dtype(dtype) == np.uint8:
        data = np.clip(np.rint((data - 90.0) * 12.0), 0, 255)
    return data.astype(dtype)


def cross_scenes(default_grid):
    """[(name, data, src_inverse, src epsg, dst transform, (height, width), dst epsg, cells inside the source)]; `default_grid`:
    (data, transform, src epsg, dst epsg) -> ((H, W), transform), the default grid of scene 1 (`default_warp_grid` on a backend)."""
    from geograypher_amd.utils.raster import invert_affine

    data = scene_source()
    inv = invert_affine(SCENE_SRC_TRANSFORM)
    (h1, w1), t1 = default_grid(data, SCENE_SRC_TRANSFORM, UTM10, GEO)
    geo, _, _, _ = warp(data, inv, None, t1, (0, 0, w1, h1), _crs(UTM10), _crs(GEO), NEAREST, np.nan)
    return [
        ("utm10_to_geographic_default_grid", data, inv, UTM10, t1, (h1, w1), GEO, 1000),
        ("utm10_to_utm11_at_0.7m", data, inv, UTM10, (0.7, 0.0, 23490.2, 0.0, -0.7, 4195661.6), (40, 45), UTM11, 550),
        ("geographic_to_utm10_at_0.5m", geo, invert_affine(t1), GEO, (0.5, 0.0, 551997.2, 0.0, -0.5, 4182017.6), (40, 50), UTM10, 1073),
    ]


def _crs(epsg):
    from geograypher_amd.utils.geospatial import crs_tuple

    return crs_tuple(epsg)
