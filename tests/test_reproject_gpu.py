"""gr_reproject_points on the device against the mpmath oracle of tests/golden/crs_wgs84.npz (DESIGN.md "CRS reprojection", G9).

The device library's sin, atan2, atanh ... are not correctly rounded, so the comparison with the oracle is a tolerance: 4 x the
error the golden script measured of the numpy stand-in, never above 5e-7 m.  Everything that does not depend on those functions
IS exact: the statistics, the NaN rows, the independence of a row's bits from V and from its position, in place against out of
place, one run against the next, the face mean of the reprojected vertices.

The kernel stages nothing, so the sizes that matter are the 64 lanes of a wave, the 256 lanes of a workgroup and the capacity of
the capped grid, 256 x GR_CRS_MAX_GROUPS rows, beyond which the stride loop takes a second pass."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import crs_standin as cs  # noqa: E402
from geograypher_amd import _hip  # noqa: E402
from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons  # noqa: E402
from geograypher_amd.utils.geospatial import WGS84CRS  # noqa: E402
from geograypher_amd.utils.raster import PlanarRaster  # noqa: E402

pytestmark = pytest.mark.gpu


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def host(t):
    return t.cpu().numpy()


def crs_of(t):
    kind, lon0, k0, fe, fn = t
    return WGS84CRS(kind, lon0, k0, fe, fn)


@pytest.fixture(scope="module")
def golden():
    return cs.load_golden()


def run(hip, points, src, dst, **kw):
    out, stats = hip.reproject_points(points, crs_of(src), crs_of(dst), **kw)
    return host(out), host(stats)


@pytest.mark.parametrize("src,dst", cs.PAIRS)
def test_golden_within_four_times_the_standin_error(hip, golden, src, dst):
    """1, 2: every direction pair, every system of the golden file: values within the bound, NaN exactly on the flagged rows, the
    statistics words equal to the golden's counts."""
    bound = cs.bounds(golden, 4.0)
    worst = np.zeros(3)
    for g in range(len(golden["tm_params"])):
        rows = np.nonzero(golden["group"] == g)[0]
        got, stats = run(hip, golden[f"in_{src}"][rows], cs.golden_crs(golden, src, g), cs.golden_crs(golden, dst, g))
        want, flag = golden[f"exp_{src}_{dst}"][rows], golden[f"flag_{src}_{dst}"][rows]
        assert same(np.isnan(got), np.repeat(flag != 0, 3).reshape(-1, 3)), (src, dst, g)
        assert stats.tolist() == [int((flag == 1).sum()), int((flag == 2).sum()), 0, 0]
        worst = np.maximum(worst, cs.worst_errors(got, want, dst, from_ecef=src == "ecef"))
    print(f"{src}->{dst}: device worst [planar/ECEF, h, lon/lat x a] = {worst} m, bound {bound}")
    assert (worst <= bound).all(), (worst, bound)


@pytest.fixture(scope="module")
def tiled(hip, golden):
    """Zone 10's golden ECEF rows -> UTM, alone: the bits every position of every V must reproduce."""
    rows = np.nonzero(golden["group"] == 0)[0]
    base = np.ascontiguousarray(golden["in_ecef"][rows])
    src, dst = cs.golden_crs(golden, "ecef", 0), cs.golden_crs(golden, "tm", 0)
    want, stats = run(hip, base, src, dst)
    want.setflags(write=False)
    return base, src, dst, want, stats


@pytest.mark.parametrize("V", [1, 63, 64, 65, 257, 256 * _hip.GR_CRS_MAX_GROUPS + 65])
def test_same_row_same_bits_at_every_position_and_size(hip, tiled, V):
    """3: the golden points tiled to V rows: row i equals the lone run's row i mod P, bit for bit, the statistics scale."""
    base, src, dst, want, stats1 = tiled
    P = len(base)
    idx = np.arange(V) % P
    got, stats = run(hip, base[idx], src, dst)
    assert got.shape == (V, 3) and same(got, want[idx])
    flagged = np.isnan(want[idx]).any(axis=1)
    assert int(stats[:2].sum()) == int(flagged.sum()) and stats[2] == 0


def test_in_place_and_repeat_runs_are_bit_equal(hip, tiled):
    """4"""
    import torch

    base, src, dst, want, _ = tiled
    again, _ = run(hip, base, src, dst)
    assert same(again, want)
    buf = torch.as_tensor(base).to(hip.device)
    out, stats = hip.reproject_points(buf, crs_of(src), crs_of(dst), out=buf)
    assert out.data_ptr() == buf.data_ptr() and same(host(buf), want)


@pytest.mark.parametrize("F", [1, 65])
def test_face_rows_are_the_mean_of_the_reprojected_vertices(hip, tiled, F):
    """5: ((p0 + p1) + p2) / 3 of the device's own vertex rows, bit for bit (the mean is plain float64 arithmetic); a face with a
    flagged vertex is NaN and counted once; a face naming a missing vertex is NaN and counted as bad, nothing else."""
    base, src, dst, want, _ = tiled
    V = len(base)
    rng = np.random.default_rng(F)
    faces = rng.integers(0, V, size=(F, 3)).astype(np.int32)
    if F > 1:
        faces[7] = (0, V, 1)      # one past the end
        faces[9] = (-1, 2, 3)
    got, stats = run(hip, base, src, dst, faces=faces, check=False)
    bad = ((faces < 0) | (faces >= V)).any(axis=1)
    f = np.where(bad[:, None], 0, faces)
    with np.errstate(invalid="ignore"):
        mean = ((want[f[:, 0]] + want[f[:, 1]]) + want[f[:, 2]]) / 3.0
    mean[bad] = np.nan
    assert same(got, mean)
    assert int(stats[2]) == int(bad.sum()) and int(stats[:2].sum()) == int((np.isnan(mean).any(axis=1) & ~bad).sum())
    if bad.any():
        with pytest.raises(ValueError, match="gr_reproject_points: 2 faces name a vertex outside"):
            hip.reproject_points(base, crs_of(src), crs_of(dst), faces=faces)


def test_a_mesh_of_three_vertices(hip, golden):
    """5: V = 3, one face"""
    rows = np.nonzero((golden["group"] == 0) & (golden["flag_ecef_tm"] == 0))[0][:3]
    src, dst = cs.golden_crs(golden, "ecef", 0), cs.golden_crs(golden, "tm", 0)
    verts, _ = run(hip, golden["in_ecef"][rows], src, dst)
    got, stats = run(hip, golden["in_ecef"][rows], src, dst, faces=np.array([[2, 0, 1]], dtype=np.int32))
    assert same(got, (((verts[2] + verts[0]) + verts[1]) / 3.0)[None]) and stats.tolist() == [0, 0, 0, 0]


def test_bad_arguments_name_the_call(hip):
    """6"""
    import ctypes

    import torch

    pts = torch.zeros((4, 3), dtype=torch.float64, device=hip.device)
    out = torch.zeros((4, 3), dtype=torch.float64, device=hip.device)
    faces = torch.zeros((2, 3), dtype=torch.int32, device=hip.device)
    stats = torch.zeros((4,), dtype=torch.int64, device=hip.device)
    ecef, utm = _hip.Crs(_hip.GR_CRS_ECEF, 0, 1, 0, 0), _hip.Crs(_hip.GR_CRS_TM, -123.0, 0.9996, 500000.0, 0.0)
    geo = _hip.Crs(_hip.GR_CRS_GEOGRAPHIC, 0, 1, 0, 0)
    eye = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))
    r, s = ctypes.byref, hip._stream()

    def call(points=pts.data_ptr(), V=4, f=None, F=0, pre=None, a=ecef, b=utm, o=out.data_ptr(), st=stats.data_ptr()):
        hip._call("gr_reproject_points", points, V, f, F, pre, r(a), r(b), o, st, s)

    call()
    call(pre=ctypes.addressof(eye))
    for kw, message in (
        (dict(points=None), "gr_reproject_points: null arrays"),
        (dict(o=None), "gr_reproject_points: null arrays"),
        (dict(st=None), "gr_reproject_points: null arrays"),
        (dict(V=-1), "gr_reproject_points: bad shape V=-1"),
        (dict(F=2), "gr_reproject_points: null faces with F=2"),
        (dict(a=_hip.Crs(3, 0, 1, 0, 0)), "gr_reproject_points: bad source CRS \\(kind 3"),
        (dict(b=_hip.Crs(-1, 0, 1, 0, 0)), "gr_reproject_points: bad target CRS \\(kind -1"),
        (dict(b=_hip.Crs(_hip.GR_CRS_TM, 0.0, 0.0, 0.0, 0.0)), "gr_reproject_points: bad target CRS \\(kind 2, k0 0"),
        (dict(a=_hip.Crs(_hip.GR_CRS_TM, 0.0, -1.0, 0.0, 0.0)), "gr_reproject_points: bad source CRS \\(kind 2, k0 -1"),
        (dict(a=geo, pre=ctypes.addressof(eye)), "gr_reproject_points: a pre-transform needs an ECEF source"),
        (dict(f=faces.data_ptr(), F=2, o=pts.data_ptr()), "gr_reproject_points: in place only without faces"),
    ):
        with pytest.raises(ValueError, match=message):
            call(**kw)
    with pytest.raises(ValueError, match="pre_transform must be \\(4, 4\\)"):
        hip.reproject_points(np.zeros((2, 3)), "EPSG:4978", "EPSG:32610", pre_transform=np.eye(3))
    with pytest.raises(NotImplementedError, match="pyproj"):
        hip.reproject_points(np.zeros((2, 3)), "EPSG:4978", "EPSG:26910")
    empty, stats0 = hip.reproject_points(np.zeros((0, 3)), "EPSG:4978", "EPSG:32610")
    assert tuple(empty.shape) == (0, 3) and host(stats0).tolist() == [0, 0, 0, 0]


def test_round_trip_on_the_device(hip, golden):
    """7: ECEF -> UTM -> ECEF, both legs on the device, within the bound of one."""
    rows = np.nonzero((golden["group"] == 0) & (golden["flag_ecef_tm"] == 0))[0]
    ecef = golden["in_ecef"][rows]
    src, dst = cs.golden_crs(golden, "ecef", 0), cs.golden_crs(golden, "tm", 0)
    there, _ = hip.reproject_points(ecef, crs_of(src), crs_of(dst))
    back, stats = run(hip, there, dst, src)
    err = np.abs(back - ecef).max()
    print(f"round trip ECEF -> UTM -> ECEF: {err} m")
    assert stats.tolist() == [0, 0, 0, 0] and err <= cs.bounds(golden, 4.0)[0]


def test_pre_transform_is_applied_first(hip, golden):
    """the cameras' local_to_epsg_4978: the device applies the 3 x 4 rows, then converts -- the same bits as converting the
    host's ((m0 x + m1 y) + m2 z) + m3."""
    rows = np.nonzero((golden["group"] == 1) & (golden["flag_ecef_tm"] == 0))[0][:70]
    ecef = golden["in_ecef"][rows]
    angle = 0.3
    m = np.eye(4)
    m[:3, :3] = 1.7 * np.array([[np.cos(angle), -np.sin(angle), 0], [np.sin(angle), np.cos(angle), 0], [0, 0, 1]])
    m[:3, 3] = (1000.0, -2000.0, 300.0)
    local = (np.linalg.inv(m) @ np.c_[ecef, np.ones(len(ecef))].T).T[:, :3]
    moved = np.stack([((m[k, 0] * local[:, 0] + m[k, 1] * local[:, 1]) + m[k, 2] * local[:, 2]) + m[k, 3] for k in range(3)], axis=1)
    src, dst = cs.golden_crs(golden, "ecef", 1), cs.golden_crs(golden, "tm", 1)
    assert same(run(hip, local, src, dst, pre_transform=m)[0], run(hip, moved, src, dst)[0])


@pytest.fixture(scope="module")
def utm_scene(hip):
    """A 7 x 8 grid of vertices (84 faces) over a 60 m square of UTM zone 10, lifted onto the ellipsoid by the device."""
    n, m = 7, 8
    e, nn = np.meshgrid(552000.0 + np.linspace(0, 60, m), 4182000.0 + np.linspace(0, 60, n))
    h = 20.0 + 3.0 * np.sin(e / 9.0) + 2.0 * np.cos(nn / 7.0)
    utm = np.stack([e.ravel(), nn.ravel(), h.ravel()], axis=1)
    idx = np.arange(n * m).reshape(n, m)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], axis=1), np.stack([b, d, c], axis=1)])
    ecef = host(hip.reproject_points(utm, "EPSG:32610", "EPSG:4978")[0])
    mesh = TexturedPhotogrammetryMesh((ecef, faces), backend=hip, log_level="ERROR")
    array = host(hip.reproject_points(ecef, "EPSG:4978", "EPSG:32610")[0])   # the device's own reprojection
    assert np.abs(array - utm).max() < 1e-6
    return mesh, array


def test_designator_equals_array_end_to_end(hip, utm_scene):
    """8: a CRS name in place of the points gives what the device's own reprojection, passed as an array, gives."""
    mesh, array = utm_scene
    assert same(mesh.get_mesh_points_in_CRS("EPSG:32610", use_vertices=True), array)
    squares = [np.array([[x, y], [x + 25, y], [x + 25, y + 25], [x, y + 25]], dtype=np.float64) + (552000.0, 4182000.0)
               for x, y in ((2.0, 3.0), (30.0, 31.0), (20.0, 20.0))]
    polygons = PlanarPolygons.from_sequence(squares)
    want = mesh.face_polygon_index(polygons, points_in_polygon_CRS=array)
    assert set(want.tolist()) == {-1, 0, 1, 2}
    assert same(mesh.face_polygon_index(polygons, points_in_polygon_CRS="EPSG:32610"), want)
    assert same(mesh.face_polygon_index(polygons, points_in_polygon_CRS=32610), want)

    dtm = PlanarRaster(np.full((8, 8), 12.0, dtype=np.float32), (10.0, 0.0, 551990.0, 0.0, -10.0, 4182070.0), nodata=-9999.0)
    want = mesh.get_height_above_ground(dtm, points_in_raster_CRS=array)
    assert np.isfinite(want).all() and 0 < want.min() and want.max() < 14
    assert same(mesh.get_height_above_ground(dtm, points_in_raster_CRS="EPSG:32610"), want)

    (p_want, f_want), pid_want, fid_want = mesh.select_mesh_ROI([squares[0]], buffer_meters=1.5, return_original_IDs=True,
                                                                 points_in_ROI_CRS=array)
    (p_got, f_got), pid_got, fid_got = mesh.select_mesh_ROI([squares[0]], buffer_meters=1.5, return_original_IDs=True,
                                                             points_in_ROI_CRS=WGS84CRS.utm(10))
    assert 0 < len(fid_want) < len(mesh.faces)
    assert same(p_got, p_want) and same(f_got, f_want) and same(pid_got, pid_want) and same(fid_got, fid_want)
