"""The raster -> raster warp without a GPU (include/geograster_warp.h): the numpy stand-in on hand-computed
cells and against exact rationals, `default_warp_grid`, the CRS-known/unknown matrix of `warp_raster`, the file-to-file functions
and the canopy-height method through the stand-in backend, and the C ABI: header <-> `_WARP_SIGNATURES` <-> `WarpRasterArgs` <->
exported symbol."""
import ctypes
import re
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import nadir_standin as ns  # noqa: E402
import outline_standin as osn  # noqa: E402
import vector_standin as vs  # noqa: E402
import warp_raster_standin as ws  # noqa: E402
from geograypher_amd import _hip, build  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import geospatial  # noqa: E402
from geograypher_amd.utils.geospatial import WGS84CRS, default_warp_grid, warp_raster  # noqa: E402
from geograypher_amd.utils.raster import PlanarRaster, invert_affine  # noqa: E402
from geograypher_amd.utils.tiff import write_tiff_deflate  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
GRID4 = np.arange(16, dtype=np.float64).reshape(1, 4, 4)
ND = -1.0
HAND = {
    "identity": (IDENTITY, (0, 0, 4, 4)),
    "half_cell_shift": ((1.0, 0.0, 0.5, 0.0, 1.0, 0.0), (0, 0, 4, 4)),
    "twice_up": ((0.5, 0.0, 0.0, 0.0, 0.5, 0.0), (0, 0, 8, 8)),
    "twice_down": ((2.0, 0.0, 0.0, 0.0, 2.0, 0.0), (0, 0, 2, 2)),
    "rotated": ((0.0, 1.0, 0.0, 1.0, 0.0, 0.0), (0, 0, 4, 4)),
}


def hand(name, resampling, data=GRID4, **kw):
    transform, window = HAND[name]
    return ws.warp(data, invert_affine(IDENTITY), None, transform, window, resampling=resampling, dst_nodata=ND, **kw)


# -- hand-computed cells -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resampling", [ws.NEAREST, ws.BILINEAR])
def test_identity_returns_the_source(resampling):
    """Centres on centres: nearest takes the cell; bilinear has fx = fy = 0, all the weight on tap (r0, c0)."""
    out, stats, und, _ = hand("identity", resampling)
    assert np.array_equal(out, GRID4) and stats.tolist() == [16, 0, 0, 0, 0, 0, 0, 0] and not und.any()


def test_half_cell_shift():
    g = GRID4[0]
    out, stats, _, _ = hand("half_cell_shift", ws.NEAREST)
    assert np.array_equal(out[0], np.column_stack([g[:, 1:], np.full(4, ND)]))   # the centre x = c + 1 falls into column c + 1
    assert stats[_hip.GR_WARP_STAT_OUTSIDE] == 4
    out, stats, _, _ = hand("half_cell_shift", ws.BILINEAR)
    # u' = c + 0.5: the mean of columns c and c + 1; in the last column only tap c0 = 3 lies in the raster: num / den = its value
    assert np.array_equal(out[0], np.column_stack([(g[:, :-1] + g[:, 1:]) / 2.0, g[:, 3]]))
    assert stats[_hip.GR_WARP_STAT_OUTSIDE] == 0


def test_twice_up_and_twice_down():
    g = GRID4[0]
    out, _, _, _ = hand("twice_up", ws.NEAREST)
    assert np.array_equal(out[0], np.repeat(np.repeat(g, 2, axis=0), 2, axis=1))
    out, _, _, _ = hand("twice_up", ws.BILINEAR)
    # the centre (0.75, 0.75) in source cells: u' = 0.25, taps columns 0 and 1 with 3/4 and 1/4; rows likewise
    assert out[0, 1, 1] == 0.75 * (0.75 * g[0, 0] + 0.25 * g[0, 1]) + 0.25 * (0.75 * g[1, 0] + 0.25 * g[1, 1])
    assert out[0, 0, 0] == g[0, 0] and out[0, 7, 7] == g[3, 3]          # corners: one tap in the raster
    out, _, _, _ = hand("twice_down", ws.NEAREST)
    assert np.array_equal(out[0], g[1::2, 1::2])                           # the centre 2 c + 1 falls into column 2 c + 1
    out, _, _, _ = hand("twice_down", ws.BILINEAR)
    assert np.array_equal(out[0], (g[0::2, 0::2] + g[0::2, 1::2] + g[1::2, 0::2] + g[1::2, 1::2]) / 4.0)


@pytest.mark.parametrize("resampling", [ws.NEAREST, ws.BILINEAR])
def test_rotated_transform_transposes(resampling):
    out, stats, _, _ = hand("rotated", resampling)
    assert np.array_equal(out[0], GRID4[0].T) and stats[_hip.GR_WARP_STAT_OUTSIDE] == 0


def test_nodata_taps_are_left_out_and_the_rest_renormalised():
    data = GRID4.copy()
    data[0, 1, 1] = 99.0
    t = (1.0, 0.0, 0.5, 0.0, 1.0, 0.5)                                   # centres on the cell corners: four equal taps
    out, stats, _, masks = ws.warp(data, invert_affine(IDENTITY), 99.0, t, (0, 0, 3, 3), resampling=ws.BILINEAR, dst_nodata=ND)
    g = data[0]
    assert out[0, 0, 0] == (0.25 * g[0, 0] + 0.25 * g[0, 1] + 0.25 * g[1, 0]) / 0.75          # one tap lost
    assert out[0, 1, 1] == (0.25 * g[1, 2] + 0.25 * g[2, 1] + 0.25 * g[2, 2]) / 0.75
    assert out[0, 2, 2] == (g[2, 2] + g[2, 3] + g[3, 2] + g[3, 3]) / 4.0                        # none lost: no division
    assert stats[_hip.GR_WARP_STAT_NODATA] == 4 and masks["nodata"][:2, :2].all()
    near, stats, _, _ = ws.warp(data, invert_affine(IDENTITY), 99.0, IDENTITY, (0, 0, 4, 4), resampling=ws.NEAREST, dst_nodata=ND)
    assert near[0, 1, 1] == ND and stats[_hip.GR_WARP_STAT_NODATA] == 1
    # fx = 0 with only the (c0 + 1) taps valid: the participating weights sum to 0
    data = np.full((1, 2, 2), 99.0)
    data[0, :, 1] = 5.0
    out, stats, _, _ = ws.warp(data, invert_affine(IDENTITY), 99.0, IDENTITY, (0, 0, 1, 1), resampling=ws.BILINEAR, dst_nodata=ND)
    assert out[0, 0, 0] == ND and stats[_hip.GR_WARP_STAT_DEN_ZERO] == 1


def test_uint8_rounds_halves_up_and_stays_in_range():
    assert ws.to_dtype([0.5, 1.5, 2.4999, -0.5, -3.0, 254.5, 300.0, np.nan], np.uint8).tolist() == [1, 2, 2, 0, 0, 255, 255, 0]
    data = np.array([[[1, 2], [4, 7]]], dtype=np.uint8)
    out, _, _, _ = ws.warp(data, invert_affine(IDENTITY), None, (1.0, 0.0, 0.5, 0.0, 1.0, 0.5), (0, 0, 1, 1), resampling=ws.BILINEAR,
                           dst_nodata=0.0)
    assert out.dtype == np.uint8 and out[0, 0, 0] == 4                    # 3.5 -> 4


# -- against exact rationals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HAND))
def test_source_coordinates_equal_the_exact_ones(name):
    """The transforms of the hand-computed cases are dyadic: W2 and W4 are exact, and the stand-in's u, v must EQUAL the rationals."""
    transform, window = HAND[name]
    src_t = (0.5, 0.0, -1.25, 0.0, -0.25, 3.5)                            # another dyadic source grid, south edge up
    inv = invert_affine(src_t)
    x, y = ws.centres(transform, window)
    u, v = ws.source_units(x, y, inv)
    a, b, c0, d, e, f0 = (Fraction(k) for k in transform)
    ia, ib, ic, id_, ie, if_ = (Fraction(k) for k in inv)
    for r in range(window[3]):
        for c in range(window[2]):
            col, row = Fraction(2 * (window[0] + c) + 1, 2), Fraction(2 * (window[1] + r) + 1, 2)
            xe, ye = a * col + b * row + c0, d * col + e * row + f0
            assert Fraction(float(u[r, c])) == ia * xe + ib * ye + ic and Fraction(float(v[r, c])) == id_ * xe + ie * ye + if_
            # and the exact inverse: the source cell coordinates of the point
            assert Fraction(float(u[r, c])) == (xe - Fraction(src_t[2])) / Fraction(src_t[0])
            assert Fraction(float(v[r, c])) == (ye - Fraction(src_t[5])) / Fraction(src_t[4])


# -- default_warp_grid, warp_raster ----------------------------------------------------------------------------------------------------
def scene_raster(**kw):
    return PlanarRaster(ws.scene_source(**kw), ws.SCENE_SRC_TRANSFORM, None, ws.UTM10)


def test_default_warp_grid_on_a_known_outline():
    backend = ws.WarpStandinBackend()
    src = scene_raster()
    (H, W), t = default_warp_grid(src, ws.UTM10, ws.GEO, backend)
    assert (H, W) == (25, 40) and t[1] == t[3] == 0.0 and t[0] == -t[4] > 0
    # the rule, from the reprojected corners (at this size the edges' bulge is far below a cell)
    corners = np.array([[552000.3, 4182014.7, 0], [552018.8, 4182014.7, 0], [552018.8, 4182000.2, 0], [552000.3, 4182000.2, 0]])
    ll, _ = backend.reproject_points(corners, WGS84CRS.parse(ws.UTM10), WGS84CRS.parse(ws.GEO))
    xmin, xmax, ymin, ymax = ll[:, 0].min(), ll[:, 0].max(), ll[:, 1].min(), ll[:, 1].max()
    res = np.hypot(xmax - xmin, ymax - ymin) / np.hypot(37.0, 29.0)
    assert abs(t[0] - res) < 1e-9 * res and abs(t[2] - xmin) < 1e-9 and abs(t[5] - ymax) < 1e-9
    assert W == int(np.floor((xmax - xmin) / res + 0.5)) and H == int(np.floor((ymax - ymin) / res + 0.5))
    # a grid given as ((H, W), transform) is the same thing
    assert default_warp_grid(((29, 37), ws.SCENE_SRC_TRANSFORM), ws.UTM10, ws.GEO, backend) == ((H, W), t)


def test_the_three_cross_crs_scenes_are_the_ones_counted():
    backend = ws.WarpStandinBackend()
    scenes = ws.cross_scenes(lambda data, t, s, d: default_warp_grid(((data.shape[1], data.shape[2]), t), s, d, backend))
    assert [(s[5], s[7]) for s in scenes] == [((25, 40), 1000), ((40, 45), 550), ((40, 50), 1073)]
    for name, data, inv, src, t, (h, w), dst, inside in scenes:
        for resampling in (ws.NEAREST, ws.BILINEAR):
            _, stats, und, masks = ws.warp(data, inv, None, t, (0, 0, w, h), ws._crs(src), ws._crs(dst), resampling, np.nan)
            assert und.sum() == 0, name
            if resampling == ws.NEAREST:
                assert h * w - stats[_hip.GR_WARP_STAT_OUTSIDE] == inside, name
            edge = np.minimum(np.abs(masks["u"] - np.rint(masks["u"])), np.abs(masks["v"] - np.rint(masks["v"])))
            assert edge.min() > 2e-6


def test_crs_known_unknown_matrix():
    backend = ws.WarpStandinBackend()
    src = scene_raster()
    like = ((29, 37), ws.SCENE_SRC_TRANSFORM)
    same = warp_raster(src, PlanarRaster(np.zeros((29, 37)), ws.SCENE_SRC_TRANSFORM, None, ws.UTM10), backend=backend)   # both known, equal
    assert np.array_equal(same.data, src.data) and same.epsg == ws.UTM10 and same.data.dtype == np.float32
    unknown = PlanarRaster(src.data, src.transform)
    assert np.array_equal(warp_raster(unknown, like, backend=backend).data, src.data)                                     # both unknown
    with pytest.raises(ValueError, match="dst_crs="):
        warp_raster(src, like, backend=backend)                                                                           # source only
    with pytest.raises(ValueError, match="src_crs="):
        warp_raster(unknown, like, dst_crs=ws.UTM10, backend=backend)                                                     # destination only
    assert np.array_equal(warp_raster(unknown, like, src_crs=ws.UTM10, dst_crs="EPSG:32610", backend=backend).data, src.data)
    cross = warp_raster(src, dst_crs="EPSG:4326", backend=backend)                                                        # both known, differ
    assert cross.shape == (1, 25, 40) and cross.epsg == 4326 and cross.last_warp_stats["outside"] == 0
    assert np.isnan(cross.nodata) if cross.nodata is not None else True
    with pytest.raises(NotImplementedError, match="26910"):
        warp_raster(src, like, dst_crs="EPSG:26910", backend=backend)
    with pytest.raises(ValueError, match="ECEF"):
        warp_raster(src, like, dst_crs=4978, backend=backend)
    with pytest.raises(ValueError, match="no destination"):
        warp_raster(unknown, backend=backend)
    with pytest.raises(ValueError, match="resampling"):
        warp_raster(src, like, dst_crs=ws.UTM10, resampling="cubic", backend=backend)
    # the method is the function
    assert np.array_equal(src.warped(dst_crs=4326, backend=backend).data, cross.data, equal_nan=True)


def test_bands_of_rows_change_no_byte_and_resolution_builds_a_grid():
    backend = ws.WarpStandinBackend()
    src = scene_raster(bands=3)
    whole = warp_raster(src, dst_crs=ws.UTM11, resolution=0.7, resampling="bilinear", backend=backend)
    banded = warp_raster(src, dst_crs=ws.UTM11, resolution=0.7, resampling="bilinear", backend=backend, max_device_bytes=3 * 4 * whole.shape[2] * 5)
    assert whole.shape[0] == 3 and whole.transform[0] == 0.7 and np.array_equal(whole.data, banded.data, equal_nan=True)
    assert whole.last_warp_stats == banded.last_warp_stats and whole.last_warp_stats["cells"] == whole.shape[1] * whole.shape[2]
    finer = warp_raster(src, resolution=0.25, dst_crs=ws.UTM10, backend=backend)                                          # same CRS, a built grid
    assert finer.transform[0] == 0.25 and finer.shape[1] >= 58 and finer.last_warp_stats["outside"] < finer.shape[1] * finer.shape[2]


def test_host_checks_name_the_call():
    for bad in [((0, 4, 4), (0, 0, 4, 4)), ((17, 4, 4), (0, 0, 4, 4)), ((1, 1 << 23, 4), (0, 0, 4, 4)), ((1, 4, 4), (0, 0, 0, 4)),
                ((1, 4, 4), (1 << 23, 0, 4, 4)), ((1, 4, 4), (0, -(1 << 23), 4, 4)), ((4, 4), (0, 0, 4, 4))]:
        with pytest.raises(ValueError, match="gr_warp_raster"):
            _hip.check_warp_window(bad[0], *bad[1])
    _hip.check_warp_window((16, (1 << 23) - 1, 1), -5, -5, 4, 4, np.uint8)
    with pytest.raises(ValueError, match="gr_warp_raster"):
        _hip.check_warp_window((1, 4, 4), 0, 0, 4, 4, np.int16)
    with pytest.raises(ValueError, match="uint8 destination"):
        _hip.warp_dst_nodata(-9999.0, None, np.uint8)
    assert _hip.warp_dst_nodata(None, 7.0, np.uint8) == 7.0 and np.isnan(_hip.warp_dst_nodata(None, None, np.float32))


# -- file to file ----------------------------------------------------------------------------------------------------------------------
def test_reproject_raster_file_to_file(tmp_path):
    backend = ws.WarpStandinBackend()
    data = ws.scene_source(np.float32)
    data[0, 3:6, 4:7] = -9999.0
    write_tiff_deflate(tmp_path / "dtm.tif", data[0], transform=ws.SCENE_SRC_TRANSFORM, nodata=-9999.0, epsg=ws.UTM10)
    written = geospatial.reproject_raster(tmp_path / "dtm.tif", tmp_path / "dtm_4326.tif", backend=backend)
    back = PlanarRaster.from_geotiff(tmp_path / "dtm_4326.tif")
    assert back.epsg == 4326 and back.nodata == -9999.0 and back.shape == (1, 25, 40) and back.data.dtype == np.float32
    assert np.allclose(back.transform, written.transform, rtol=0, atol=0) and np.array_equal(back.data, written.data)
    (H, W), t = default_warp_grid(((29, 37), ws.SCENE_SRC_TRANSFORM), ws.UTM10, 4326, backend)
    want, stats, _, _ = ws.warp(data, invert_affine(ws.SCENE_SRC_TRANSFORM), -9999.0, t, (0, 0, W, H), ws._crs(ws.UTM10), ws._crs(4326),
                                ws.NEAREST, -9999.0)
    assert np.array_equal(back.data, want) and stats[_hip.GR_WARP_STAT_NODATA] >= 1 and (back.data == -9999.0).sum() == stats[_hip.GR_WARP_STAT_NODATA]
    # three uint8 bands stay uint8 on the way
    rgb = ws.scene_source(np.uint8, bands=3)
    write_tiff_deflate(tmp_path / "ortho.tif", np.moveaxis(rgb, 0, 2), transform=ws.SCENE_SRC_TRANSFORM, epsg=ws.UTM10)
    out = geospatial.reproject_raster(tmp_path / "ortho.tif", tmp_path / "ortho_11.tif", "EPSG:32611", resolution=0.7, backend=backend)
    assert out.data.dtype == np.uint8 and out.shape[0] == 3 and out.epsg == ws.UTM11
    again, file_dtype = geospatial.read_raster_bands(tmp_path / "ortho_11.tif")
    assert file_dtype == np.uint8 and again.epsg == ws.UTM11 and np.array_equal(again.data, out.data) and again.transform == out.transform
    # what the writer cannot hold is refused by name
    write_tiff_deflate(tmp_path / "u16.tif", np.zeros((4, 4), np.uint16), transform=ws.SCENE_SRC_TRANSFORM, epsg=ws.UTM10)
    with pytest.raises(NotImplementedError, match="uint16"):
        geospatial.reproject_raster(tmp_path / "u16.tif", tmp_path / "x.tif", backend=backend)
    write_tiff_deflate(tmp_path / "nocrs.tif", np.zeros((4, 4), np.float32), transform=ws.SCENE_SRC_TRANSFORM)
    with pytest.raises(NotImplementedError, match="no EPSG"):
        geospatial.reproject_raster(tmp_path / "nocrs.tif", tmp_path / "x.tif", backend=backend)


def test_load_downsampled_raster_data(tmp_path):
    backend = ws.WarpStandinBackend()
    data = ws.scene_source(np.float32)
    write_tiff_deflate(tmp_path / "dtm.tif", data[0], transform=ws.SCENE_SRC_TRANSFORM, epsg=ws.UTM10)
    small, source, updated = geospatial.load_downsampled_raster_data(tmp_path / "dtm.tif", 2.0, backend=backend)
    assert small.shape == (1, 14, 18) and source.shape == (1, 29, 37) and source.epsg == ws.UTM10
    a, b, c, d, e, f = ws.SCENE_SRC_TRANSFORM
    assert updated == (a * (37 / 18), 0.0, c, 0.0, e * (29 / 14), f)
    want, _, _, _ = ws.warp(data, invert_affine(ws.SCENE_SRC_TRANSFORM), None, updated, (0, 0, 18, 14), resampling=ws.BILINEAR, dst_nodata=np.nan)
    assert np.array_equal(small, want) and np.isfinite(small).all()
    # factor 1: centres on centres, the file itself
    same, _, t1 = geospatial.load_downsampled_raster_data(tmp_path / "dtm.tif", 1.0, backend=backend)
    assert np.array_equal(same, data) and t1 == ws.SCENE_SRC_TRANSFORM
    with pytest.raises(ValueError, match="downsample_factor"):
        geospatial.load_downsampled_raster_data(tmp_path / "dtm.tif", 0.0, backend=backend)
    with pytest.raises(ValueError, match="no cell left"):
        geospatial.load_downsampled_raster_data(tmp_path / "dtm.tif", 100.0, backend=backend)


# -- canopy height -----------------------------------------------------------------------------------------------------------------------
class Backend(ns.StandInBackend, ws.WarpStandinBackend, osn.StandInBackend, vs.StandInBackend):
    pass


def roof_scene():
    """(points, faces, the DTM, the grid ((6, 6), transform): one ring of cells round the roof, the canopy heights wanted on it)."""
    points = np.array([[0, 0, 10], [4, 0, 10], [4, 4, 10], [0, 4, 10]], dtype=np.float64)
    faces = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64)
    cx, cy = np.meshgrid(-2.0 + np.arange(8) + 0.5, 6.0 - np.arange(8) - 0.5)
    ground = (cx / 2.0 + cy / 4.0).astype(np.float32)
    ground[2, 5] = -9999.0                                                   # the DTM cell with centre (3.5, 3.5)
    dtm = PlanarRaster(ground, (1.0, 0.0, -2.0, 0.0, -1.0, 6.0), -9999.0)
    grid = ((6, 6), (1.0, 0.0, -1.0, 0.0, -1.0, 5.0))
    gx, gy = np.meshgrid(-1.0 + np.arange(6) + 0.5, 5.0 - np.arange(6) - 0.5)
    want = np.where((gx > 0) & (gx < 4) & (gy > 0) & (gy < 4), 10.0 - gx / 2.0 - gy / 4.0, -9999.0)
    want[1, 4] = -9999.0                                                     # the centre (3.5, 3.5): its DTM cell is nodata
    return points, faces, dtm, grid, want


def test_canopy_height_of_a_two_face_roof_over_a_tilted_dtm(tmp_path):
    """A flat roof at z = 10 over [0, 4]^2, two faces; the DTM z = x / 2 + y / 4 on 1 m cells over [-2, 6]^2, north up.  Bilinear
    sampling of a plane is the plane (dyadic weights and values: exact), so the canopy height at a centre is 10 - x / 2 - y / 4."""
    points, faces, dtm, grid, want = roof_scene()
    mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=Backend())
    chm = mesh.export_canopy_height_raster(dtm, tmp_path / "chm.tif", like=grid, points_in_raster_CRS=points)
    assert chm.nodata == -9999.0 and chm.shape == (1, 6, 6)
    # centres ON the DTM's centres: the nodata cell takes all the weight there, the neighbours of that cell give it none
    assert np.array_equal(chm.data[0], want)
    back = PlanarRaster.from_geotiff(tmp_path / "chm.tif")
    assert back.nodata == -9999.0 and np.array_equal(back.data[0], want.astype(np.float32)) and back.transform == grid[1]
    assert mesh.last_warp_stats["cells"] == 36 and mesh.last_warp_stats["den_zero"] == 1
    # off the DTM's centres: every centre has four taps, the lost one is renormalised away
    grid2 = ((4, 4), (1.0, 0.0, 0.25, 0.0, -1.0, 3.75))
    chm2 = mesh.export_canopy_height_raster(dtm, like=grid2, points_in_raster_CRS=points)
    assert (chm2.data != -9999.0).sum() == 16 and mesh.last_warp_stats["nodata"] == 2 and mesh.last_warp_stats["den_zero"] == 0
    gx, gy = np.meshgrid(0.25 + np.arange(4) + 0.5, 3.75 - np.arange(4) - 0.5)
    plane = 10.0 - gx / 2.0 - gy / 4.0
    lost = (gx > 2.5) & (gy > 2.5)                                          # the two centres with the nodata cell among their taps
    assert lost.sum() == 2 and np.array_equal(chm2.data[0][~lost], plane[~lost]) and np.all(chm2.data[0][lost] != plane[lost])
    with pytest.raises(ValueError, match="dst_crs=|src_crs="):
        mesh.export_canopy_height_raster(dtm, like=grid, points_in_raster_CRS=points, dtm_CRS=32610)
    with pytest.raises(NotImplementedError, match="tif"):
        mesh.export_canopy_height_raster(dtm, tmp_path / "x.png", like=grid, points_in_raster_CRS=points)


# -- the C ABI ---------------------------------------------------------------------------------------------------------------------------
C_TYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "double": ctypes.c_double}


def header_struct(name):
    """[(field, ctypes type)] of `typedef struct <name> { ... } <name>;` in include/geograster_warp.h: a field with a `*` is a
    pointer, every other one of the four scalar types."""
    text = (ROOT / "include" / "geograster_warp.h").read_text()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for statement in filter(None, (s.strip() for s in body.split(";"))):
        pointer = re.fullmatch(r"(?:const\s+)?\w+\s*\*\s*(\w+)", statement)
        scalar = re.fullmatch(r"(int64_t|int32_t|float|double)\s+(\w+)", statement)
        assert pointer or scalar, statement
        fields.append((pointer.group(1), ctypes.c_void_p) if pointer else (scalar.group(2), C_TYPES[scalar.group(1)]))
    return fields


def test_descriptor_mirror_equals_the_header_field_by_field():
    want = header_struct("gr_warp_raster_args")
    assert len(want) == 22
    assert [(n, t) for n, t in _hip.WarpRasterArgs._fields_] == want
    assert ctypes.sizeof(_hip.WarpRasterArgs) == 128
    assert ("stream", ctypes.c_void_p) in want


def test_header_binding_and_source_name_the_call():
    main = (ROOT / "include" / "geograster.h").read_text()
    header = (ROOT / "include" / "geograster_warp.h").read_text()
    source = (ROOT / "geograypher_amd" / "csrc" / "raster_warp.hip").read_text()
    internal = (ROOT / "geograypher_amd" / "csrc" / "gr_internal.hpp").read_text()
    stripped = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = dict(re.findall(r"\bint (gr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", stripped))
    assert declared == {"gr_warp_raster": "gr_ctx *ctx, const gr_warp_raster_args *args_h"}
    assert _hip.WARP_SYMBOLS == tuple(declared)
    assert _hip._WARP_SIGNATURES == {"gr_warp_raster": [ctypes.c_void_p, ctypes.POINTER(_hip.WarpRasterArgs)]}
    assert not re.search(r"gr_warp_raster\b", main) and main.count('#include "geograster_warp.h"') == 1
    assert main.index('#include "geograster_warp.h"') > main.index('#include "geograster_vis.h"')
    flat = " ".join(header.replace(" * ", " ").split())
    assert "#define GR_VERSION 126" in main and "without a GR_VERSION bump" in flat
    assert "NOT exempt from the stream contract" in flat and "tests/test_stream_contract_warp_gpu.py" in flat
    text = Path(build.__file__).read_text()
    assert any(p.name == "raster_warp.hip" for p in build.SOURCES) and "geograster_warp.h" in text
    assert any(p.name == "crs_dev.hpp" for p in build.HEADERS)
    assert set(re.findall(r"void (k_\w+)\(", source)) == {"k_warp_raster"} and "k_warp_raster" in internal
    # the conversion lives in ONE place: both units include the header, neither defines it
    crs = (ROOT / "geograypher_amd" / "csrc" / "crs.hip").read_text()
    dev = (ROOT / "geograypher_amd" / "csrc" / "crs_dev.hpp").read_text()
    for unit in (crs, source):
        assert '#include "crs_dev.hpp"' in unit and not re.search(r"\bint convert\(", unit)
    assert len(re.findall(r"\bint convert\(", dev)) == 1 and "bool crs_side(" in dev
    assert _hip.WARP_SIDE_LIMIT == 1 << 23 and re.search(r"WARP_MAX_SIDE = 1 << 23\b", source)
    assert list(_hip.WARP_DTYPES.values()) == [_hip.GR_DTYPE_U8, _hip.GR_DTYPE_F32, _hip.GR_DTYPE_F64]


def test_the_library_exports_the_call_and_refuses_without_a_device():
    lib = ctypes.CDLL(str(_hip.library_path()))
    fn = lib.gr_warp_raster
    fn.restype, fn.argtypes = ctypes.c_int, _hip._WARP_SIGNATURES["gr_warp_raster"]
    assert fn(None, None) == _hip.GR_EINVAL
    assert fn(None, ctypes.byref(_hip.WarpRasterArgs())) == _hip.GR_EINVAL
