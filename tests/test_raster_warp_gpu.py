"""The raster -> raster warp on the device (csrc/raster_warp.hip) behind fenced and poisoned outputs.  Same-CRS
calls equal the numpy stand-in of tests/warp_raster_standin.py byte for byte, in every cell, with no tolerance: only +, x, /, floor
take part.  Cross-CRS calls go through the device library's transcendentals: under nearest every cell the stand-in can determine
equals it exactly, under bilinear a cell agrees within what a conversion error of delta can move its weights by; the three scenes are
the ones tests/test_raster_warp_host.py counts.  Refusals run on valid device memory and leave the output untouched."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import warp_raster_standin as ws  # noqa: E402
from geograypher_amd import _hip  # noqa: E402
from geograypher_amd.utils.geospatial import default_warp_grid, warp_raster  # noqa: E402
from geograypher_amd.utils.raster import PlanarRaster, invert_affine  # noqa: E402
from tests.fenced_backend import FencedHipRaster, fenced  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = (np.uint8, np.float32, np.float64)
RESAMPLINGS = (("nearest", ws.NEAREST), ("bilinear", ws.BILINEAR))
S = _hip
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


@pytest.fixture(scope="module")
def backend():
    b = FencedHipRaster(0)
    yield b
    b.close()


def dst_nodata_of(dtype):
    return 255.0 if np.dtype(dtype) == np.uint8 else -9999.0


def source(rng, B, H, W, dtype, nodata=None, nans=False):
    """Random bands; `nodata` on about a sixth of the cells, NaN (float sources) on about a tenth."""
    if np.dtype(dtype) == np.uint8:
        data = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
    else:
        data = (rng.normal(size=(B, H, W)) * 40.0 + 100.0).astype(dtype)
    if nodata is not None:
        data[rng.random((B, H, W)) < 1 / 6] = nodata
    if nans and np.dtype(dtype) != np.uint8:
        data[rng.random((B, H, W)) < 0.1] = np.nan
    return data


def same(backend, data, src_t, src_nodata, dst_t, window, resampling, dst_dtype=None, dst_nodata=None):
    """One same-CRS call behind fences against the stand-in: every byte of the planes, every statistics word."""
    name, kind = resampling
    dst_dtype = data.dtype if dst_dtype is None else np.dtype(dst_dtype)
    nd = dst_nodata_of(dst_dtype) if dst_nodata is None else dst_nodata
    inv = invert_affine(src_t)
    want, want_stats, und, _ = ws.warp(data, inv, src_nodata, dst_t, window, resampling=kind, dst_nodata=nd, dst_dtype=dst_dtype)
    assert not und.any()
    with fenced(backend):
        out, stats = backend.warp_raster(data, inv, src_nodata, dst_t, window, resampling=name, dst_nodata=nd, dst_dtype=dst_dtype)
        got, got_stats = out.cpu().numpy(), stats.cpu().numpy()
    what = (data.shape, str(data.dtype), str(dst_dtype), name, window)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), (what, np.argwhere(got.view(np.uint8) != want.view(np.uint8))[:4].tolist())
    assert got_stats.tolist() == want_stats.tolist(), what
    return got, got_stats


def covering_transform(H, W, width, height):
    """A destination grid over the source (identity transform) with an overhang on every side and a slight rotation: no dyadic
    coefficient, so centres fall anywhere in the source's cells."""
    sx, sy = 1.3 * W / width, 1.3 * H / height
    return (sx, 0.031 * sy, -0.15 * W - 0.01, -0.027 * sx, sy, -0.15 * H + 0.02)


# -- same CRS: byte for byte -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B", [(1, 1, 1), (2, 2, 3), (3, 5, 4), (29, 37, 3)])
def test_every_width_dtype_pair_and_resampling_equals_the_standin(backend, H, W, B):
    """Widths 1, 63, 64, 65 and 257: below, at and above a wave's 64 columns, and two workgroups of 256; heights 1 and 5; all nine
    source -> destination dtype pairs; source nodata present (and, in float sources, NaN beside it)."""
    rng = np.random.default_rng(100 * H + W)
    for src_dtype in DTYPES:
        data = source(rng, B, H, W, src_dtype, nodata=7, nans=True)
        for width in (1, 63, 64, 65, 257):
            for height in (1, 5):
                t = covering_transform(H, W, width, height)
                for dst_dtype in DTYPES:
                    for resampling in RESAMPLINGS:
                        same(backend, data, IDENTITY, 7.0, t, (0, 0, width, height), resampling, dst_dtype)


def test_windows_that_leave_the_grid_on_each_side_and_one_wholly_outside(backend):
    rng = np.random.default_rng(3)
    data = source(rng, 2, 29, 37, np.float32)
    src_t = (0.5, 0.0, 100.0, 0.0, -0.5, 50.0)
    for window in [(-3, -2, 10, 6), (30, -2, 12, 6), (-3, 25, 10, 8), (30, 25, 12, 8), (-4, -4, 45, 37)]:
        for resampling in RESAMPLINGS:
            got, stats = same(backend, data, src_t, None, src_t, window, resampling)
            assert 0 < stats[S.GR_WARP_STAT_OUTSIDE] < stats[S.GR_WARP_STAT_CELLS]
    for resampling in RESAMPLINGS:
        got, stats = same(backend, data, src_t, None, src_t, (100, 100, 65, 3), resampling)
        assert np.all(got == -9999.0) and stats[S.GR_WARP_STAT_OUTSIDE] == stats[S.GR_WARP_STAT_CELLS] == 195


def test_south_up_source_rotated_transform_and_centres_on_cell_edges(backend):
    rng = np.random.default_rng(4)
    data = source(rng, 1, 29, 37, np.float64, nodata=-1.0)
    south_up = (0.5, 0.0, 10.0, 0.0, 0.5, 20.0)                       # e > 0: row 0 is the southern edge
    north_up = (0.37, 0.0, 9.0, 0.0, -0.37, 36.0)
    rotated = (0.21, 0.34, 9.5, 0.34, -0.21, 21.0)                    # b, d != 0
    for resampling in RESAMPLINGS:
        got, stats = same(backend, data, south_up, -1.0, north_up, (0, 0, 65, 45), resampling)
        assert stats[S.GR_WARP_STAT_OUTSIDE] > 0 and stats[S.GR_WARP_STAT_NODATA] > 0
        same(backend, data, south_up, -1.0, rotated, (0, 0, 65, 45), resampling)
        same(backend, data, rotated, -1.0, north_up, (0, 0, 65, 45), resampling)
        # centres exactly ON the source's cell edges (u, v integers): the half-open rule decides, nothing is undetermined
        edges = (1.0, 0.0, -0.5 - 2.0, 0.0, 1.0, -0.5 - 2.0)
        got, stats = same(backend, data, IDENTITY, -1.0, edges, (0, 0, 42, 34), resampling)
        # ... and on its cell centres' lines shifted by a half: u' = u - 0.5 is an integer for bilinear
        same(backend, data, IDENTITY, -1.0, (1.0, 0.0, -2.0, 0.0, 1.0, -2.0), (0, 0, 42, 34), resampling)


def test_nodata_absent_present_and_nan_in_a_float32_source(backend):
    rng = np.random.default_rng(5)
    t = covering_transform(13, 17, 65, 9)
    plain = source(rng, 2, 13, 17, np.float32)
    for resampling in RESAMPLINGS:
        _, stats = same(backend, plain, IDENTITY, None, t, (0, 0, 65, 9), resampling)
        assert stats[S.GR_WARP_STAT_NODATA] == 0
        marked = plain.copy()
        marked[:, 3:6, 4:9] = -5.0
        _, stats = same(backend, marked, IDENTITY, -5.0, t, (0, 0, 65, 9), resampling)
        assert stats[S.GR_WARP_STAT_NODATA] > 0
        _, unmarked = same(backend, marked, IDENTITY, None, t, (0, 0, 65, 9), resampling)          # the same cells, no nodata named
        assert unmarked[S.GR_WARP_STAT_NODATA] == 0
        holes = plain.copy()
        holes[0, 3:6, 4:9] = np.nan                                                              # one band only: counted per cell
        got, stats = same(backend, holes, IDENTITY, None, t, (0, 0, 65, 9), resampling, dst_nodata=float("nan"))
        assert stats[S.GR_WARP_STAT_NODATA] > 0 and np.isnan(got[0]).any()


def test_bilinear_with_one_two_and_four_taps_lost(backend):
    """Centres on the source's cell corners: four taps of weight 1/4.  A nodata cell takes a tap from each of its four corners; two
    nodata neighbours take two from the corner between them; a 2 x 2 block takes all four from its middle (den = 0)."""
    data = (np.arange(48, dtype=np.float64).reshape(1, 6, 8) + 1.0) * 1.5
    data[0, 1, 1] = -1.0                       # one lost at (1, 1) .. (2, 2)
    data[0, 1, 4] = data[0, 1, 5] = -1.0       # two lost at the corners between them
    data[0, 3:5, 2:4] = -1.0                   # four lost at the block's middle corner (4, 3)
    corners = (1.0, 0.0, 0.5, 0.0, 1.0, 0.5)
    got, stats = same(backend, data, IDENTITY, -1.0, corners, (0, 0, 7, 5), ("bilinear", ws.BILINEAR))
    g = data[0]
    assert got[0, 0, 0] == (0.25 * g[0, 0] + 0.25 * g[0, 1] + 0.25 * g[1, 0]) / 0.75
    assert got[0, 0, 4] == (0.25 * g[0, 4] + 0.25 * g[0, 5]) / 0.5
    assert got[0, 3, 2] == -9999.0 and stats[S.GR_WARP_STAT_DEN_ZERO] == 1
    assert got[0, 4, 5] == ((0.25 * g[4, 5] + 0.25 * g[4, 6]) + 0.25 * g[5, 5]) + 0.25 * g[5, 6]      # none lost: num, no division
    # off the corners, so that the lost weights differ
    same(backend, data, IDENTITY, -1.0, (0.7, 0.0, 0.3, 0.0, 0.9, 0.2), (0, 0, 11, 6), ("bilinear", ws.BILINEAR))
    # fx = 0 with only the (c0 + 1) taps valid: a tap takes part with weight 0, den = 0
    two = np.full((1, 2, 2), -1.0)
    two[0, :, 1] = 5.0
    got, stats = same(backend, two, IDENTITY, -1.0, IDENTITY, (0, 0, 1, 1), ("bilinear", ws.BILINEAR))
    assert got[0, 0, 0] == -9999.0 and stats[S.GR_WARP_STAT_DEN_ZERO] == 1


def test_uint8_rounding_at_exactly_one_half(backend):
    data = np.array([[[1, 2, 3], [4, 7, 250], [255, 255, 254]]], dtype=np.uint8)
    corners = (1.0, 0.0, 0.5, 0.0, 1.0, 0.5)
    got, _ = same(backend, data, IDENTITY, None, corners, (0, 0, 2, 2), ("bilinear", ws.BILINEAR), dst_nodata=0.0)
    assert got[0].tolist() == [[4, 66], [130, 192]]                   # 3.5 -> 4, 65.5 -> 66, 130.25 -> 130, 191.5 -> 192
    halves = np.array([[[0.5, 1.5, 2.5, -0.5, 254.5, 255.5, 1e9, -1e9, 2.4999999999999996]]])
    for dtype in (np.float64, np.float32):
        got, _ = same(backend, halves.astype(dtype), IDENTITY, None, IDENTITY, (0, 0, 9, 1), ("nearest", ws.NEAREST), np.uint8, 0.0)
        assert got[0, 0].tolist() == [1, 2, 3, 0, 255, 255, 255, 0, 2 if dtype == np.float64 else 3]


def test_bands_of_rows_equal_one_window_and_two_runs_are_equal(backend):
    rng = np.random.default_rng(6)
    data = source(rng, 4, 29, 37, np.uint8, nodata=0)
    t = covering_transform(29, 37, 257, 23)
    inv = invert_affine(IDENTITY)
    for name, kind in RESAMPLINGS:
        whole, stats = same(backend, data, IDENTITY, 0.0, t, (0, 0, 257, 23), (name, kind))
        parts, totals = [], np.zeros(8, dtype=np.int64)
        for row0, n in ((0, 1), (1, 7), (8, 15)):
            out, st = backend.warp_raster(data, inv, 0.0, t, (0, row0, 257, n), resampling=name, dst_nodata=255.0)
            parts.append(out.cpu().numpy())
            totals += st.cpu().numpy()
        assert np.array_equal(np.concatenate(parts, axis=1), whole) and totals.tolist() == stats.tolist()
        cols = [backend.warp_raster(data, inv, 0.0, t, (c0, 0, n, 23), resampling=name, dst_nodata=255.0)[0].cpu().numpy()
                for c0, n in ((0, 100), (100, 157))]
        assert np.array_equal(np.concatenate(cols, axis=2), whole)
        one_band = backend.warp_raster(data[2:3], inv, 0.0, t, (0, 0, 257, 23), resampling=name, dst_nodata=255.0)[0].cpu().numpy()
        assert np.array_equal(one_band[0], whole[2])                                               # W9: B does not matter
        again, _ = same(backend, data, IDENTITY, 0.0, t, (0, 0, 257, 23), (name, kind))
        assert again.tobytes() == whole.tobytes()
    # an `out` of the caller's is written in place
    mine = torch.full((4, 23, 257), 9, dtype=torch.uint8, device=backend.device)
    out, _ = backend.warp_raster(data, inv, 0.0, t, (0, 0, 257, 23), resampling="bilinear", dst_nodata=255.0, out=mine)
    assert out.data_ptr() == mine.data_ptr() and np.array_equal(mine.cpu().numpy(), whole)


# -- cross CRS ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    standin = ws.WarpStandinBackend()
    return ws.cross_scenes(lambda data, t, s, d: default_warp_grid(((data.shape[1], data.shape[2]), t), s, d, standin))


@pytest.mark.parametrize("k", [0, 1, 2])
def test_cross_crs_scenes(backend, scenes, k):
    name, data, inv, src, t, (h, w), dst, inside = scenes[k]
    data = data.astype(np.float64)
    data[0, 10:13, 20:24] = -9999.0
    window = (0, 0, w, h)
    for rname, kind in RESAMPLINGS:
        want, want_stats, und, masks = ws.warp(data, inv, -9999.0, t, window, ws._crs(src), ws._crs(dst), kind, np.nan)
        with fenced(backend):
            out, stats = backend.warp_raster(data, inv, -9999.0, t, window, src_crs=src, dst_crs=dst, resampling=rname,
                                             dst_nodata=float("nan"))
            got, got_stats = out.cpu().numpy(), stats.cpu().numpy()
        share = und.mean()
        print(f"\nwarp | {name} | {rname} | undetermined {int(und.sum())} of {und.size} | outside {got_stats[1]} (stand-in {want_stats[1]}) "
              f"| nodata {got_stats[4]} (stand-in {want_stats[4]})")
        assert share <= 0.005, (name, rname, share)                       # the cap, before anything is compared
        keep = ~und
        assert got.shape == want.shape == (1, h, w) and got_stats[0] == h * w
        if kind == ws.NEAREST:
            assert h * w - want_stats[S.GR_WARP_STAT_OUTSIDE] == inside
            assert np.array_equal(got[0][keep], want[0][keep], equal_nan=True), (name, int((got[0] != want[0]).sum()))
        else:
            assert np.array_equal(np.isnan(got[0][keep]), np.isnan(want[0][keep]))
            delta = ws.DELTA_DEG if ws._crs(src)[0] == 1 else ws.DELTA_M
            delta_cells = max(delta * (abs(inv[0]) + abs(inv[1])), delta * (abs(inv[3]) + abs(inv[4])))
            spread = ws.bilinear_tap_range(np.where(data == -9999.0, np.nan, data), inv, masks["u"], masks["v"])[0]
            bound = 2.0 * delta_cells * spread + 4.0 * np.spacing(np.abs(want[0]))
            ok = keep & ~np.isnan(want[0])
            err = np.abs(got[0] - want[0])
            print(f"warp | {name} | bilinear | worst error {np.nanmax(err[ok]):.3e}, worst error / bound {np.nanmax(err[ok] / bound[ok]):.3f}")
            assert np.all(err[ok] <= bound[ok]), (name, float(np.nanmax(err[ok] / bound[ok])))
        if not und.any():
            assert got_stats[S.GR_WARP_STAT_OUTSIDE] == want_stats[S.GR_WARP_STAT_OUTSIDE]
            assert got_stats[S.GR_WARP_STAT_NODATA] == want_stats[S.GR_WARP_STAT_NODATA] > 0
        assert got_stats[S.GR_WARP_STAT_NONFINITE] == got_stats[S.GR_WARP_STAT_BEYOND] == 0


def test_a_row_beyond_ninety_degrees_of_the_central_meridian_is_nodata(backend, scenes):
    """A geographic destination round longitude -20: 103 degrees from the central meridian of UTM zone 10, the source's CRS."""
    _, data, inv, src, _, _, _, _ = scenes[0]
    t = (0.001, 0.0, -20.0, 0.0, -0.001, 38.0)
    for rname, _kind in RESAMPLINGS:
        with fenced(backend):
            out, stats = backend.warp_raster(data, inv, None, t, (0, 0, 65, 2), src_crs=src, dst_crs=4326, resampling=rname, dst_nodata=-1.0)
            got, got_stats = out.cpu().numpy(), stats.cpu().numpy()
        assert np.all(got == -1.0) and got_stats.tolist() == [130, 0, 0, 130, 0, 0, 0, 0]
    # a latitude beyond the pole is refused as not finite
    with fenced(backend):
        out, stats = backend.warp_raster(data, inv, None, (0.001, 0.0, -123.0, 0.0, -0.001, 95.0), (0, 0, 3, 1), src_crs=src, dst_crs=4326,
                                         dst_nodata=-1.0)
        assert np.all(out.cpu().numpy() == -1.0) and stats.cpu().numpy().tolist() == [3, 0, 3, 0, 0, 0, 0, 0]


def test_the_python_layers_on_the_device(backend, scenes):
    """`default_warp_grid` and `warp_raster` through the device: the grid of scene 1, and bands that change no byte."""
    name, data, inv, src, t, (h, w), dst, inside = scenes[0]
    raster = PlanarRaster(data, ws.SCENE_SRC_TRANSFORM, None, src)
    (H, W), t_dev = default_warp_grid(raster, src, dst, backend)
    assert (H, W) == (h, w) and np.allclose(t_dev, t, rtol=1e-12, atol=0)
    whole = warp_raster(raster, ((h, w), t), dst_crs=dst, resampling="bilinear", backend=backend)
    banded = warp_raster(raster, ((h, w), t), dst_crs=dst, resampling="bilinear", backend=backend, max_device_bytes=4 * w * 7)
    assert whole.data.dtype == np.float32 and whole.data.tobytes() == banded.data.tobytes()
    assert whole.last_warp_stats == banded.last_warp_stats and whole.last_warp_stats["cells"] == h * w


def test_canopy_height_on_the_device(backend, tmp_path):
    """The roof of tests/test_raster_warp_host.py over its tilted DTM: top-down raster and bilinear warp on the device, as arrays
    and as tensors."""
    from geograypher_amd.meshes import TexturedPhotogrammetryMesh
    from tests.test_raster_warp_host import roof_scene

    points, faces, dtm, grid, want = roof_scene()
    mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=backend)
    chm = mesh.export_canopy_height_raster(dtm, tmp_path / "chm.tif", like=grid, points_in_raster_CRS=points)
    assert np.array_equal(chm.data[0], want) and mesh.last_warp_stats["den_zero"] == 1
    assert np.array_equal(PlanarRaster.from_geotiff(tmp_path / "chm.tif").data[0], want.astype(np.float32))
    tensor = mesh.export_canopy_height_raster(dtm, like=grid, points_in_raster_CRS=points, return_tensor=True)
    assert tensor.device.type == "cuda" and np.array_equal(tensor.cpu().numpy(), np.where(want == -9999.0, np.nan, want), equal_nan=True)


# -- refusals -------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_einval_names_the_call_and_leaves_the_output_untouched(backend):
    dev = backend.device
    data = torch.arange(2 * 6 * 8, dtype=torch.float64, device=dev).reshape(2, 6, 8).contiguous()
    out = torch.full((2 * 4 * 5 + 1,), 77.0, dtype=torch.float64, device=dev)
    stats = torch.full((8,), 55, dtype=torch.int64, device=dev)
    inv, t = (ctypes.c_double * 6)(*IDENTITY), (ctypes.c_double * 6)(*IDENTITY)
    bad_t = (ctypes.c_double * 6)(1.0, 0.0, float("inf"), 0.0, 1.0, 0.0)
    utm, geo, ecef = _hip.Crs(2, -123.0, 0.9996, 500000.0, 0.0), _hip.Crs(1, 0.0, 1.0, 0.0, 0.0), _hip.Crs(0, 0.0, 1.0, 0.0, 0.0)
    k0, lon0, kind = _hip.Crs(2, -123.0, 0.0, 500000.0, 0.0), _hip.Crs(2, float("nan"), 0.9996, 500000.0, 0.0), _hip.Crs(7, 0.0, 1.0, 0.0, 0.0)
    adr = ctypes.addressof

    def args(**kw):
        base = dict(data=data.data_ptr(), out=out.data_ptr(), stats=stats.data_ptr(), stream=backend._stream().value,
                    src_inverse6_h=adr(inv), dst_transform6_h=adr(t), src_crs_h=None, dst_crs_h=None, src_nodata=0.0, dst_nodata=-1.0,
                    B=2, H=6, W=8, src_dtype=2, dst_dtype=2, has_src_nodata=0, col_off=0, row_off=0, width=5, height=4, resampling=0,
                    same_crs=1)
        base.update(kw)
        return _hip.WarpRasterArgs(**base)

    lim = 1 << 23
    cases = {
        "null data": args(data=None), "null out": args(out=None), "null stats": args(stats=None),
        "null inverse": args(src_inverse6_h=None), "null transform": args(dst_transform6_h=None),
        "B = 0": args(B=0), "B = 17": args(B=17), "H = 0": args(H=0), "W = 2^23": args(W=lim), "H < 0": args(H=-1),
        "unknown source dtype": args(src_dtype=3), "unknown destination dtype": args(dst_dtype=-1), "unknown resampling": args(resampling=2),
        "empty window": args(width=0), "window offset at 2^23": args(col_off=lim), "window edge beyond 2^23": args(row_off=lim - 3),
        "window offset at -2^23": args(row_off=-lim),
        "transform not finite": args(dst_transform6_h=adr(bad_t)),
        "null CRS": args(same_crs=0, src_crs_h=adr(utm)), "ECEF source": args(same_crs=0, src_crs_h=adr(ecef), dst_crs_h=adr(geo)),
        "ECEF destination": args(same_crs=0, src_crs_h=adr(utm), dst_crs_h=adr(ecef)),
        "k0 = 0": args(same_crs=0, src_crs_h=adr(k0), dst_crs_h=adr(geo)), "lon0 NaN": args(same_crs=0, src_crs_h=adr(utm), dst_crs_h=adr(lon0)),
        "unknown kind": args(same_crs=0, src_crs_h=adr(kind), dst_crs_h=adr(geo)),
        "float64 data off by 4 bytes": args(data=data.data_ptr() + 4), "float64 out off by 4 bytes": args(out=out.data_ptr() + 4),
        "out is data": args(out=data.data_ptr()), "out inside data": args(out=data.data_ptr() + 8 * 8, B=1),
    }
    assert backend._rc("gr_warp_raster", None) == _hip.GR_EINVAL
    for what, a in cases.items():
        assert backend._rc("gr_warp_raster", ctypes.byref(a)) == _hip.GR_EINVAL, what
        message = backend.lib.gr_last_error(backend._ctx).decode()
        assert "gr_warp_raster" in message, (what, message)
    torch.cuda.synchronize(dev)
    assert bool((out == 77.0).all()) and bool((stats == 55).all()) and bool((data.reshape(-1) == torch.arange(96, device=dev)).all())
    # the same descriptor without a fault is taken: the refusals were about the one field each
    assert backend._rc("gr_warp_raster", ctypes.byref(args())) == _hip.GR_OK
    torch.cuda.synchronize(dev)
    assert np.array_equal(out[:40].reshape(2, 4, 5).cpu().numpy(), data[:, :4, :5].cpu().numpy()) and float(out[40]) == 77.0
    assert stats.cpu().tolist() == [20, 0, 0, 0, 0, 0, 0, 0]
    # ... and the binding's own checks raise before the library is called
    with pytest.raises(ValueError, match="gr_warp_raster"):
        backend.warp_raster(np.zeros((17, 2, 2)), IDENTITY, None, IDENTITY, (0, 0, 2, 2))
    with pytest.raises(ValueError, match="ECEF"):
        backend.warp_raster(np.zeros((1, 2, 2)), IDENTITY, None, IDENTITY, (0, 0, 2, 2), src_crs=4978, dst_crs=4326)
    with pytest.raises(ValueError, match="out must be"):
        backend.warp_raster(np.zeros((1, 2, 2)), IDENTITY, None, IDENTITY, (0, 0, 2, 2), out=torch.zeros((1, 2, 3), dtype=torch.float64, device=dev))
