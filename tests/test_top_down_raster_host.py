"""The top-down raster of the mesh without a GPU (rules N1-N9): the stand-in of tests/nadir_standin.py on
hand-worked cases, against the polygon burn's stand-in on single-sheet meshes and against exact rationals; the layers above the call
(`top_down_raster`, the mesh methods, the GeoTIFF exports, `aggregate_images`) through the stand-in backend; arguments, refusals and
the C ABI of the new call."""
import re
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import burn_standin as bs  # noqa: E402
import nadir_standin as ns  # noqa: E402
import outline_standin as osn  # noqa: E402
import region_standin as rs  # noqa: E402
import vector_standin as vs  # noqa: E402
from geograypher_amd import _hip, build  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import geospatial, synthetic  # noqa: E402
from geograypher_amd.utils.geospatial import grid_from_bounds, points_to_cell_units, rings_to_cell_units, top_down_raster  # noqa: E402
from geograypher_amd.utils.raster import PlanarRaster, invert_affine  # noqa: E402
from geograypher_amd.utils.tiff import write_tiff_deflate  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
ONE = 65536
W44 = (0, 0, 4, 4)


def q(points):
    """Cell coordinates -> cell units (exact for the halves and quarters of the hand-worked cases)."""
    return [(int(round(x * ONE)), int(round(y * ONE))) for x, y in points]


def run(points, z, faces, window=W44, **kw):
    return ns.nadir_raster(q(points), z, faces, window, **kw)


# -- hand-worked 4 x 4 cases ------------------------------------------------------------------------------------------------------------
def test_one_face_left_and_top_edges_in_right_and_bottom_out():
    """The triangle (0,0) (4,0) (0,4) with z = x + 10 y: the centres (c + .5, r + .5) with c + r <= 2 lie strictly inside; those
    with c + r = 3 lie ON the hypotenuse, a right-hand boundary, which Z3 leaves out."""
    face, z, stats = run([(0, 0), (4, 0), (0, 4)], [0.0, 4.0, 40.0], [[0, 1, 2]])
    want = np.array([[0, 0, 0, -1], [0, 0, -1, -1], [0, -1, -1, -1], [-1, -1, -1, -1]])
    assert np.array_equal(face, want)
    for r in range(4):
        for c in range(4):
            assert (z[r, c] == (c + 0.5) + 10.0 * (r + 0.5)) if want[r, c] == 0 else np.isnan(z[r, c])
    assert stats.tolist() == [1, 0, 0, 0, 0, 0, 16, 6, 0, 6]       # 16 tests: the box is the window; 16 cells are "small"
    assert ns.bits_of(float(z[3, 3])) == ns.NAN_BITS
    # the mirrored triangle (4,4) (0,4) (4,0) owns the hypotenuse: its left-hand boundary
    face2, _, _ = run([(4, 4), (0, 4), (4, 0)], [0.0, 0.0, 0.0], [[0, 1, 2]])
    assert np.array_equal(face2 == 0, want == -1)


def test_a_centre_on_a_shared_edge_and_on_a_shared_vertex_has_exactly_one_owner():
    """Four faces round P = (1.5, 1.5), a cell centre, inside the square (0,0)-(3,3): both diagonals run through centres.  Every
    one of the 9 cells has exactly one owner, whichever way the faces are wound."""
    points = [(0, 0), (3, 0), (3, 3), (0, 3), (1.5, 1.5)]
    for faces in ([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], [[1, 0, 4], [1, 2, 4], [3, 2, 4], [3, 0, 4]]):
        face, _, stats = run(points, [0.0] * 5, faces)
        assert stats[ns.INSIDE] == stats[ns.COVERED] == 9 and np.all(face[:3, :3] >= 0) and np.all(face[3] == -1) and np.all(face[:, 3] == -1)
        rows, _, _ = bs.burn([[q(points)[i] for i in f] for f in faces], [0, 1, 2, 3], 4, W44)
        assert np.array_equal(face, rows)
        # the top edge's face owns the top row's interior, the left edge's face the left column's
        assert face[0, 1] == 0 and face[1, 0] == 3 and face[2, 1] == 2 and face[1, 2] == 1


def test_two_sheets_the_upper_wins_and_equal_heights_go_to_the_lower_face():
    square = [(0, 0), (4, 0), (4, 4), (0, 4)]
    points = square + square                                  # ground at z = 1, a crown at z = 5 over the same square
    ground, crown = [[0, 1, 2], [0, 2, 3]], [[4, 5, 6], [4, 6, 7]]
    z = [1.0] * 4 + [5.0] * 4
    for faces, upper in ((ground + crown, (2, 3)), (crown + ground, (0, 1))):
        face, zz, stats = run(points, z, faces)
        assert set(np.unique(face).tolist()) == set(upper) and np.all(zz == 5.0)
        assert stats[ns.INSIDE] == 32 and stats[ns.COVERED] == 16
    face, zz, _ = run(points, [2.0] * 8, crown + ground)     # the same height everywhere: faces 0 and 1, never 2 and 3
    assert set(np.unique(face).tolist()) == {0, 1} and np.all(zz == 2.0)
    face_r, _, _ = run(points, [2.0] * 8, ground + crown)
    assert np.array_equal(face_r, face)                       # the same cells go to the same POSITIONS in the face list


def test_minus_zero_sorts_below_plus_zero():
    """N6 compares keys of bit patterns.  Face 0 has z = (-0.0, -5e-324, -5e-324): at the centre (1.5, 0.5), where both weights are
    1/8 ... 3/8, each term (z_k - z_a) * weight underflows to -0.0 and -0.0 + -0.0 + -0.0 is -0.0.  Face 1, the same triangle at
    +0.0, is HIGHER by one key although it compares equal as a float, so it wins in spite of its index."""
    assert ns.key_of(-0.0) + 1 == ns.key_of(0.0) and ns.key_of(-5e-324) < ns.key_of(-0.0) and ns.key_of(1.0) > ns.key_of(0.0)
    assert ns.key_of(-np.inf) > 0 and ns.key_of(-1.7976931348623157e308) > 0
    tri = [(0, 0), (4, 0), (0, 4)]
    face, zz, _ = run(tri + tri, [-0.0, -5e-324, -5e-324, 0.0, 0.0, 0.0], [[0, 1, 2], [3, 4, 5]])
    alone, z_alone, _ = run(tri, [-0.0, -5e-324, -5e-324], [[0, 1, 2]])
    assert alone[0, 1] == 0 and ns.bits_of(float(z_alone[0, 1])) == 1 << 63          # -0.0 indeed
    assert face[0, 1] == 1 and ns.bits_of(float(zz[0, 1])) == 0
    assert np.array_equal(face >= 0, alone >= 0) and np.all(face[face >= 0] == 1)


def test_vertical_faces_nan_heights_and_bad_indices_are_counted_under_their_first_cause():
    points = [(0, 0), (4, 0), (0, 4), (2, 2), (4, 4)]
    z = [0.0, 1.0, 2.0, np.nan, 3.0]
    faces = [[0, 1, 2],      # takes part
             [0, 4, 0],      # a needle: zero area
             [0, 3, 4],      # collinear in plan view AND a NaN z: the NaN is the first cause
             [1, 3, 2],      # a NaN z
             [0, 1, 5],      # a bad index
             [-1, 3, 2],     # a bad index before the NaN
             [1, 4, 2]]      # takes part: the other half of the square
    face, _, stats = run(points, z, faces)
    assert stats[:5].tolist() == [2, 2, 1, 2, 0]
    assert set(np.unique(face).tolist()) == {0, 6} and stats[ns.COVERED] == 16
    # a face outside the window takes part with an empty box
    _, _, far = run(points, z, [[0, 1, 2]], window=(10, 10, 4, 4))
    assert far[:5].tolist() == [1, 0, 0, 0, 1] and far[ns.TESTS] == 0
    # the stand-in of the binding refuses bad indices as the binding does
    with pytest.raises(ValueError, match=r"gr_nadir_raster: 2 faces name a vertex outside \[0, 5\)"):
        ns.StandInRasterizer(np.array(q(points)), np.array(z), np.array(faces)).window(*W44)


def test_the_item_word_follows_small_cells_and_item_rows_and_nothing_else_does():
    points, z, faces = [(0, 0), (4, 0), (0, 4)], [0.0, 4.0, 40.0], [[0, 1, 2]]
    base = run(points, z, faces)
    for kw, items in ((dict(small_cells=15), 1), (dict(small_cells=15, item_rows=1), 4), (dict(small_cells=1, item_rows=3), 2),
                      (dict(small_cells=16, item_rows=1), 0)):
        face, zz, stats = run(points, z, faces, **kw)
        assert stats[ns.ITEMS] == items and np.array_equal(face, base[0]) and np.array_equal(zz, base[1], equal_nan=True)
        assert np.array_equal(np.delete(stats, ns.ITEMS), np.delete(base[2], ns.ITEMS))


# -- single-sheet meshes: the id plane is the burn's row plane ----------------------------------------------------------------------------
def height_field(n=6, seed=0, jitter=0.3, scale=1.0, origin=(0.0, 0.0)):
    """An n x n vertex grid with jittered x, y (no fold) and random z, two faces per cell of the grid, wound at random."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64))
    xy = np.stack([gx.ravel(), gy.ravel()], axis=1) + rng.uniform(-jitter, jitter, (n * n, 2))
    points = np.column_stack([xy * scale + np.asarray(origin), rng.uniform(-5, 5, n * n)])
    faces = []
    for r in range(n - 1):
        for c in range(n - 1):
            a, b, d, e = r * n + c, r * n + c + 1, (r + 1) * n + c, (r + 1) * n + c + 1
            for tri in ((a, b, e), (a, e, d)):
                faces.append(tri if rng.random() < 0.5 else tri[::-1])
    return points, np.asarray(faces, dtype=np.int32)


@pytest.mark.parametrize("transform", [(0.5, 0.0, -0.3, 0.0, -0.5, 5.4), (0.4, 0.3, -1.0, 0.3, -0.4, 3.0)], ids=["north-up", "rotated"])
def test_ids_of_a_single_sheet_equal_the_burn_of_one_row_per_face(transform):
    points, faces = height_field()
    inverse = invert_affine(transform)
    vq = points_to_cell_units(points[:, :2], inverse)
    rv, off = rings_to_cell_units([points[f, :2] for f in faces], inverse)
    assert np.array_equal(rv, vq[faces.ravel()])                      # N2: the one arithmetic of Z1
    window = (-2, -3, 16, 18)
    face, z, stats = ns.nadir_raster(vq, points[:, 2], faces, window)
    rows, _, burn_stats = bs.burn(bs.rings_of_table(rv, off), list(range(len(faces))), len(faces), window)
    assert np.array_equal(face, rows) and stats[ns.INSIDE] == burn_stats[1] == stats[ns.COVERED] > 20
    assert stats[ns.FACES] == len(faces) and np.all(np.isnan(z) == (face < 0))
    inside = z[face >= 0]
    assert inside.min() >= -5 and inside.max() <= 5


# -- N5 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_height_stays_within_its_bound_of_the_exact_rational():
    rng = np.random.default_rng(5)
    checked, worst = 0, 0.0
    for _ in range(300):
        span = int(rng.choice([1 << 18, 1 << 22, (1 << 26) - 1]))
        base = rng.integers(-(1 << 39), (1 << 39) - span, 2)
        a, b, c = ([int(base[0] + rng.integers(0, span + 1)), int(base[1] + rng.integers(0, span + 1))] for _ in range(3))
        D = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        if D == 0:
            continue
        za, zb, zc = (float(v) for v in rng.normal(0, 10.0 ** rng.integers(-3, 6), 3))
        for _ in range(4):     # a point of the triangle on the grid of centres' parity: any integer point inside will do
            u, v = sorted(rng.random(2))
            px = int(round(a[0] * u + b[0] * (v - u) + c[0] * (1 - v)))
            py = int(round(a[1] * u + b[1] * (v - u) + c[1] * (1 - v)))
            Nb = (px - a[0]) * (c[1] - a[1]) - (py - a[1]) * (c[0] - a[0])
            Nc = (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])
            wb, wc = Fraction(Nb, D), Fraction(Nc, D)
            if not (0 <= wb and 0 <= wc and wb + wc <= 1):
                continue       # rounding put the point outside: N5's bound is for members
            exact = Fraction(za) + (Fraction(zb) - Fraction(za)) * wb + (Fraction(zc) - Fraction(za)) * wc
            got = ns.height_at(a, b, c, za, zb, zc, px, py)
            bound = Fraction(16, 2 ** 53) * (abs(Fraction(za)) + abs(Fraction(zb)) + abs(Fraction(zc)))
            err = abs(Fraction(got) - exact)
            assert err <= bound, (a, b, c, za, zb, zc, px, py)
            worst = max(worst, float(err / bound)) if bound else worst
            checked += 1
    assert checked > 600 and 0.0 < worst <= 1.0


# -- windows and bands ------------------------------------------------------------------------------------------------------------------
def test_windows_with_negative_offsets_are_cuts_of_one_plane():
    points, faces = height_field(5, seed=2, origin=(-2.5, -2.0))
    vq = points_to_cell_units(points[:, :2], IDENTITY)
    whole = ns.nadir_raster(vq, points[:, 2], faces, (-4, -4, 10, 10))
    assert whole[2][ns.COVERED] > 10 and np.any(whole[0][:4, :4] >= 0)          # faces at negative rows and columns
    for window in ((-4, -4, 3, 5), (-1, -2, 4, 4), (2, 1, 4, 5), (-3, 0, 9, 1)):
        c, r, w, h = window
        face, z, stats = ns.nadir_raster(vq, points[:, 2], faces, window)
        assert np.array_equal(face, whole[0][r + 4:r + 4 + h, c + 4:c + 4 + w])
        assert np.array_equal(z, whole[1][r + 4:r + 4 + h, c + 4:c + 4 + w], equal_nan=True)
        assert stats[ns.COVERED] == int((face >= 0).sum())


def test_bands_change_no_byte_and_add_their_statistics_up():
    points, faces = height_field(6, seed=3)
    like = ((11, 9), (0.5, 0.0, 0.0, 0.0, -0.5, 5.5))
    one = ns.StandInBackend()
    whole = top_down_raster(points, faces, like, backend=one)
    assert one.rasterizers[0].windows == [(0, 0, 9, 11)]
    banded = ns.StandInBackend()
    parts = top_down_raster(points, faces, like, backend=banded, max_device_bytes=12 * 9 * 4)      # 4 rows a band
    assert banded.rasterizers[0].windows == [(0, 0, 9, 4), (0, 4, 9, 4), (0, 8, 9, 3)] and len(banded.rasterizers) == 1
    assert np.array_equal(parts[0], whole[0]) and np.array_equal(parts[1], whole[1], equal_nan=True)
    assert parts[0].dtype == np.int32 and parts[1].dtype == np.float64 and parts[0].shape == (11, 9)
    for word in ("faces", "bad_index", "zero_area", "nonfinite_z", "inside", "skipped", "covered"):
        assert parts[2][word] == whole[2][word], word
    assert tuple(whole[2]) == geospatial.TOP_DOWN_STAT_NAMES and whole[2]["covered"] == int((whole[0] >= 0).sum()) > 30
    # a GeoTIFF header and a PlanarRaster name the same grid
    raster = PlanarRaster(np.zeros(like[0]), like[1])
    assert np.array_equal(top_down_raster(points, faces, raster, backend=ns.StandInBackend())[0], whole[0])


def test_top_down_raster_refusals():
    points, faces = height_field(3)
    like = ((4, 4), IDENTITY)
    backend = ns.StandInBackend()
    with pytest.raises(ValueError, match=r"points must be \(V, 3\)"):
        top_down_raster(points[:, :2], faces, like, backend=backend)
    with pytest.raises(ValueError, match=r"faces must be an \(F, 3\) integer array"):
        top_down_raster(points, faces.astype(np.float64), like, backend=backend)
    with pytest.raises(ValueError, match="a mesh vertex is not finite or lies 2\\^40 / 65536 cells or more"):
        top_down_raster(points * 1e8, faces, like, backend=backend)
    bad = points.copy()
    bad[0, 0] = np.nan
    with pytest.raises(ValueError, match="a mesh vertex is not finite"):
        top_down_raster(bad, faces, like, backend=backend)
    with pytest.raises(ValueError, match="not inside \\[1, 2\\^23\\)"):
        top_down_raster(points, faces, ((1 << 23, 4), IDENTITY), backend=backend)
    with pytest.raises(ValueError, match="1 faces name a vertex outside \\[0, 9\\)"):
        top_down_raster(points, np.vstack([faces, [[0, 1, 9]]]), like, backend=backend)
    for args, match in (((0, 0, 0, 4), "empty or leaves"), ((1 << 23, 0, 1, 1), "empty or leaves"), ((0, -(1 << 23), 1, 1), "empty or leaves"),
                        (((1 << 23) - 1, 0, 2, 1), "empty or leaves"), ((0, 0, 1, 1, -1), "small_cells=-1"), ((0, 0, 1, 1, 65537), "small_cells"),
                        ((0, 0, 1, 1, 0, 1025), "item_rows=1025")):
        with pytest.raises(ValueError, match="gr_nadir_raster: .*" + match):
            _hip.check_nadir_window(*args)
    _hip.check_nadir_window(-(1 << 23) + 1, 0, 1, 1, 65536, 1024)
    vq = np.zeros((3, 2), dtype=np.int64)
    for args, match in (((vq.astype(np.float64), np.zeros(3), faces), "vertices must be"), ((vq, np.zeros(2), faces), "z must be"),
                        ((vq, np.zeros(3, dtype=np.int64), faces), "z must be"), ((vq, np.zeros(3), faces[:, :2]), "faces must be"),
                        ((vq + (1 << 40), np.zeros(3), faces), "2\\^40 / 65536 cells")):
        with pytest.raises(ValueError, match="gr_nadir_raster: .*" + match):
            _hip.check_nadir_tables(*args)


# -- grid_from_bounds -------------------------------------------------------------------------------------------------------------------
def test_grid_from_bounds():
    xy = np.array([[10.2, 100.1], [13.9, 97.3], [11.0, 99.0]])
    (H, W), transform = grid_from_bounds(xy, 0.5)
    assert (H, W) == (7, 8) and transform == (0.5, 0.0, 10.0, 0.0, -0.5, 100.5)
    (H, W), transform = grid_from_bounds(np.column_stack([xy, np.zeros(3)]), 2.0)       # (n, 3): z plays no part
    assert (H, W) == (3, 2) and transform == (2.0, 0.0, 10.0, 0.0, -2.0, 102.0)
    assert grid_from_bounds(np.array([[4.0, 6.0]]), 1.0) == ((1, 1), (1.0, 0.0, 4.0, 0.0, -1.0, 6.0))      # at least one cell
    assert grid_from_bounds(np.array([[-0.25, -0.25], [0.25, 0.25]]), 0.5) == ((2, 2), (0.5, 0.0, -0.5, 0.0, -0.5, 0.5))
    for res in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="resolution"):
            grid_from_bounds(xy, res)
    with pytest.raises(ValueError, match="not below 2\\^23"):
        grid_from_bounds(np.array([[0.0, 0.0], [1e7, 1.0]]), 1.0)
    with pytest.raises(ValueError, match="at least one point"):
        grid_from_bounds(np.zeros((0, 2)), 1.0)
    with pytest.raises(ValueError, match="all finite"):
        grid_from_bounds(np.array([[0.0, np.inf]]), 1.0)
    # every vertex lies in a cell of the grid
    points, _ = height_field(7, seed=9, scale=3.7, origin=(431_000.3, 4_290_000.7))
    (H, W), t = grid_from_bounds(points, 0.7)
    col, row = (points[:, 0] - t[2]) / t[0], (points[:, 1] - t[5]) / t[4]
    assert col.min() >= 0 and col.max() <= W and row.min() >= 0 and row.max() <= H and W - col.max() < 1 + 1e-9 and H - row.max() < 1 + 1e-9


# -- the TIFF writer --------------------------------------------------------------------------------------------------------------------
def test_float32_geotiff_round_trip_and_unsigned_files_as_before(tmp_path):
    from PIL import Image

    rng = np.random.default_rng(0)
    dsm = rng.normal(100.0, 30.0, (7, 5)).astype(np.float32)
    dsm[2, 3] = -9999.0
    transform = (0.25, 0.0, 431_000.0, 0.0, -0.25, 4_290_000.0)
    write_tiff_deflate(tmp_path / "dsm.tif", dsm, transform=transform, nodata=-9999.0, epsg=32610)
    back = PlanarRaster.from_geotiff(tmp_path / "dsm.tif")
    assert back.data.dtype == np.float32 and np.array_equal(back.data[0], dsm) and back.transform == transform
    assert back.nodata == -9999.0 and back.epsg == 32610
    with Image.open(tmp_path / "dsm.tif") as image:
        assert image.mode == "F" and image.tag_v2[339] == (3,) and image.tag_v2[258] == (32,)
    with pytest.raises(ValueError, match="unsupported image"):
        write_tiff_deflate(tmp_path / "f64.tif", dsm.astype(np.float64))
    # unsigned files: SampleFormat 1 and the same bytes as a file assembled here the way the writer always did
    for dtype, mode in ((np.uint8, "L"), (np.uint16, "I;16")):
        cells = rng.integers(0, 200, (6, 4)).astype(dtype)
        write_tiff_deflate(tmp_path / "u.tif", cells, transform=transform, nodata=255, epsg=32610)
        with Image.open(tmp_path / "u.tif") as image:
            assert image.mode == mode and image.tag_v2[339] == (1,) and np.array_equal(np.array(image), cells)
        # the same array as float32 differs in exactly the sample format (and, for uint8 / uint16, the bits per sample)
        tags = {}
        for name, array in (("u", cells), ("f", cells.astype(np.float32))):
            write_tiff_deflate(tmp_path / f"{name}.tif", array, transform=transform, nodata=255, epsg=32610)
            with Image.open(tmp_path / f"{name}.tif") as image:
                tags[name] = {k: v for k, v in image.tag_v2.items() if k not in (273, 279)}     # not the strips' offsets and sizes
        assert {k for k in tags["u"] if tags["u"][k] != tags["f"][k]} == {258, 339}
    rgb = rng.integers(0, 255, (5, 4, 3)).astype(np.uint8)
    write_tiff_deflate(tmp_path / "rgb.tif", rgb)
    with Image.open(tmp_path / "rgb.tif") as image:
        assert image.mode == "RGB" and image.tag_v2[339] == (1, 1, 1) and np.array_equal(np.array(image), rgb)


# -- the mesh methods -------------------------------------------------------------------------------------------------------------------
class Backend(ns.StandInBackend, osn.StandInBackend, vs.StandInBackend):
    pass


def mesh_of(points, faces, **kw):
    return TexturedPhotogrammetryMesh((np.asarray(points, dtype=np.float64), np.asarray(faces, dtype=np.int64)), log_level="ERROR",
                                      backend=kw.pop("backend", None) or Backend(), **kw)


def forest():
    """Ground: a height field of class 0 / 1 by column; over its middle a flat crown of class 2, two faces at z = 20."""
    points, faces = height_field(6, seed=4)
    crown = np.array([[1.2, 1.2, 20.0], [3.8, 1.2, 20.0], [3.8, 3.8, 20.0], [1.2, 3.8, 20.0]])
    n = len(points)
    labels = np.concatenate([np.repeat((np.arange(5) % 2)[None], 5, axis=0).repeat(2), [2.0, 2.0]]).astype(np.float64)
    return np.vstack([points, crown]), np.vstack([faces, [[n, n + 1, n + 2], [n, n + 2, n + 3]]]).astype(np.int32), labels


def test_mesh_methods_and_geotiff_exports(tmp_path):
    points, faces, labels = forest()
    mesh = mesh_of(points, faces)
    planar = points + np.array([431_000.0, 4_290_000.0, 0.0])
    face_ids, heights, transform = mesh.top_down_face_raster(resolution=0.5, points_in_raster_CRS=planar)
    (H, W), want_transform = grid_from_bounds(planar, 0.5)
    assert face_ids.shape == heights.shape == (H, W) and transform == want_transform
    direct = top_down_raster(planar, faces, ((H, W), transform), backend=ns.StandInBackend())
    assert np.array_equal(face_ids, direct[0]) and np.array_equal(heights, direct[1], equal_nan=True)
    assert mesh.last_top_down_stats == direct[2] and mesh.last_top_down_stats["faces"] == len(faces)
    under_crown = face_ids >= len(faces) - 2
    assert under_crown.sum() >= 20 and np.all(heights[under_crown] == 20.0) and np.nanmax(heights[~under_crown]) <= 5.0
    # like= : the same grid as a raster object
    again = mesh.top_down_face_raster(PlanarRaster(np.zeros((H, W)), transform), points_in_raster_CRS=planar)
    assert np.array_equal(again[0], face_ids)

    dsm = mesh.export_surface_height_raster(tmp_path / "dsm.tif", resolution=0.5, points_in_raster_CRS=planar)
    assert isinstance(dsm, PlanarRaster) and dsm.data.dtype == np.float64 and dsm.nodata == -9999.0 and dsm.transform == transform
    assert np.array_equal(dsm.data[0], np.where(face_ids >= 0, heights, -9999.0))
    file = PlanarRaster.from_geotiff(tmp_path / "dsm.tif")
    assert file.data.dtype == np.float32 and np.array_equal(file.data[0], dsm.data[0].astype(np.float32))
    assert file.transform == transform and file.nodata == -9999.0 and file.epsg is None

    classes = mesh.export_face_labels_raster(labels, tmp_path / "classes.tiff", like=tmp_path / "dsm.tif", points_in_raster_CRS=planar)
    want = np.where(face_ids >= 0, labels[np.maximum(face_ids, 0)], 255)
    assert np.array_equal(classes.data[0], want) and classes.nodata == 255.0 and set(np.unique(want).tolist()) == {0.0, 1.0, 2.0, 255.0}
    assert np.all(classes.data[0][under_crown] == 2)             # the crown hides the ground under it
    file = PlanarRaster.from_geotiff(tmp_path / "classes.tiff")
    assert np.array_equal(file.data[0], want) and file.transform == transform and file.nodata == 255.0
    # the class raster feeds the raster branch of the metrics: it is a label raster like a burned one
    cells, nodata = geospatial.raster_to_uint8(file.data[0], file.nodata)
    assert cells.dtype == np.uint8 and nodata == 255

    # faces without a label: nodata with drop_nan, refused without
    holes = labels.copy()
    holes[-2:] = np.nan
    dropped = mesh.export_face_labels_raster(holes, resolution=0.5, points_in_raster_CRS=planar)
    assert np.all(dropped.data[0][under_crown] == 255) and np.array_equal(dropped.data[0][~under_crown], want[~under_crown])
    with pytest.raises(ValueError, match="cells are won by a face without a label"):
        mesh.export_face_labels_raster(holes, resolution=0.5, points_in_raster_CRS=planar, drop_nan=False)
    # the mesh's own face texture
    textured = mesh_of(points, faces, texture=labels.reshape(-1, 1), IDs_to_labels={0: "a", 1: "b", 2: "c"})
    assert np.array_equal(textured.export_face_labels_raster(resolution=0.5, points_in_raster_CRS=planar).data[0], want)


def test_mesh_method_refusals(tmp_path):
    points, faces, labels = forest()
    mesh = mesh_of(points, faces)
    kw = dict(resolution=0.5, points_in_raster_CRS=points)
    with pytest.raises(ValueError, match="exactly one of the two"):
        mesh.top_down_face_raster(points_in_raster_CRS=points)
    with pytest.raises(ValueError, match="exactly one of the two"):
        mesh.top_down_face_raster(((4, 4), IDENTITY), resolution=1.0, points_in_raster_CRS=points)
    with pytest.raises(TypeError):
        mesh.top_down_face_raster(resolution=1.0)
    with pytest.raises(NotImplementedError, match="needs points_in_raster_CRS"):
        mesh.top_down_face_raster(resolution=1.0, points_in_raster_CRS=None)
    with pytest.raises(ValueError, match=r"points_in_raster_CRS must be \(40, 3\)"):
        mesh.top_down_face_raster(resolution=1.0, points_in_raster_CRS=points[:, :2])
    with pytest.raises(ValueError, match="resolution"):
        mesh.export_surface_height_raster(resolution=0.0, points_in_raster_CRS=points)
    for name in ("x.geojson", "x.png", "x"):
        with pytest.raises(NotImplementedError, match="tif"):
            mesh.export_surface_height_raster(tmp_path / name, **kw)
        with pytest.raises(NotImplementedError, match="tif"):
            mesh.export_face_labels_raster(labels, tmp_path / name, **kw)
    with pytest.raises(ValueError, match="float32"):
        mesh.export_surface_height_raster(nodata=np.nan, **kw)
    with pytest.raises(ValueError, match="float32"):
        mesh.export_surface_height_raster(nodata=0.1, **kw)
    big = labels.copy()
    big[0] = 255
    with pytest.raises(ValueError, match="class id 255 does not fit"):
        mesh.export_face_labels_raster(big, nodata=7, **kw)
    with pytest.raises(ValueError, match="class id 2 is the raster's nodata"):
        mesh.export_face_labels_raster(labels, nodata=2, **kw)
    for nodata in (-1, 256, 1.5):
        with pytest.raises(ValueError, match="nodata="):
            mesh.export_face_labels_raster(labels, nodata=nodata, **kw)
    with pytest.raises(ValueError, match="face labels for a mesh of"):
        mesh.export_face_labels_raster(labels[:-1], **kw)
    with pytest.raises(ValueError, match="whole numbers"):
        mesh.export_face_labels_raster(labels + 0.5, **kw)
    with pytest.raises(ValueError, match="no face labels given"):
        mesh.export_face_labels_raster(**kw)
    assert mesh.export_face_labels_raster(labels, nodata=254, **kw).nodata == 254.0
    # the vector export still refuses ensure_non_overlapping, and now says where the answer is
    with pytest.raises(NotImplementedError, match="ensure_non_overlapping.*export_face_labels_raster"):
        mesh.export_face_labels_vector(labels, ensure_non_overlapping=True, points_in_export_CRS=points)


def test_a_CRS_designator_names_the_points_and_the_files_code(tmp_path):
    """points_in_raster_CRS="EPSG:32610": the vertices are reprojected (the stand-in of the CRS stage) and the file carries the code."""
    (points, faces), _cams = synthetic.config1_scene()
    from geograypher_amd.utils.geospatial import WGS84CRS, reproject_points

    backend = Backend()
    planar = np.column_stack([points[::50, :2] + [500_000.0, 4_100_000.0], points[::50, 2] + 300.0])
    ecef, _ = reproject_points(backend, planar, 32610, 4978)
    tri = np.array([[0, 1, 2], [1, 2, 3]], dtype=np.int32)
    mesh = mesh_of(ecef, tri, backend=backend)
    want_points = np.asarray(mesh._points_in_CRS(32610))
    dsm = mesh.export_surface_height_raster(tmp_path / "dsm.tif", resolution=5.0, points_in_raster_CRS="EPSG:32610")
    assert dsm.epsg == 32610 == PlanarRaster.from_geotiff(tmp_path / "dsm.tif").epsg
    direct = top_down_raster(want_points, tri, grid_from_bounds(want_points, 5.0), backend=ns.StandInBackend())
    assert np.array_equal(dsm.data[0], np.where(direct[0] >= 0, direct[1], -9999.0)) and WGS84CRS.parse("EPSG:32610").epsg == 32610


# -- the entry point --------------------------------------------------------------------------------------------------------------------
def test_aggregate_images_writes_the_top_down_raster(tmp_path, oracle_backend_cls):
    from PIL import Image

    from geograypher_amd.entrypoints.aggregate_images import aggregate_images, parse_args

    class Full(ns.StandInBackend, osn.StandInBackend, rs.StandInBackend, vs.StandInBackend, oracle_backend_cls):
        pass

    (points, faces), cams = synthetic.config1_scene()
    sub = cams[0:2]
    for i, c in enumerate(sub.cameras):
        c.image_filename = Path(tmp_path, "images", "flight", f"img_{i}.JPG")
    sub.image_folder = Path(tmp_path, "images")
    h, w = sub.cameras[0].get_image_size()
    rng = np.random.default_rng(1)
    for i in range(2):
        (tmp_path / "labels" / "flight").mkdir(parents=True, exist_ok=True)
        blocks = rng.integers(0, 4, (h // 32 + 1, w // 32 + 1)).astype(np.uint8)
        Image.fromarray(np.kron(blocks, np.ones((32, 32), dtype=np.uint8))[:h, :w]).save(tmp_path / "labels" / "flight" / f"img_{i}.png")
    np.savez(tmp_path / "mesh.npz", points=points, faces=faces)
    export_points = points + np.array([500_000.0, 4_000_000.0, 0.0])     # the vertices in the CRS of the map
    np.save(tmp_path / "export_points.npy", export_points)
    ids = {0: "a", 1: "b", 2: "c", 3: "d"}
    kw = dict(take_every_nth_camera=1, aggregate_image_scale=0.25, camera_set=sub, IDs_to_labels=ids)
    args = (tmp_path / "mesh.npz", None, tmp_path / "images", tmp_path / "labels", "EPSG:4978")
    mesh, _, classes = aggregate_images(*args, top_down_raster_projection_savefile=tmp_path / "out" / "classes.tif",
                                        top_down_raster_resolution=4.0, top_down_points_file=tmp_path / "export_points.npy",
                                        top_down_vector_projection_savefile=tmp_path / "out" / "map.geojson", backend=Full(), **kw)
    got = PlanarRaster.from_geotiff(tmp_path / "out" / "classes.tif")
    want = mesh.export_face_labels_raster(classes[:, 0], resolution=4.0, points_in_raster_CRS=export_points)
    assert np.array_equal(got.data[0], want.data[0]) and got.transform == want.transform and got.nodata == 255.0
    present = set(np.unique(got.data[0]).tolist())
    assert got.data.shape[1:] == (26, 26) and present - {255.0} == set(classes[np.isfinite(classes)].tolist()) and len(present) >= 4
    assert (tmp_path / "out" / "map.geojson").is_file()                     # beside the vector map
    assert mesh.last_top_down_stats["covered"] == int((got.data[0] != 255).sum()) or np.isnan(classes).any()

    # refusals, all before the aggregation (backend=None would fail at the first device call)
    raster_kw = dict(top_down_raster_projection_savefile=tmp_path / "x.tif", top_down_raster_resolution=4.0)
    with pytest.raises(NotImplementedError, match="^top_down_raster_projection_savefile: the vertices in the map's CRS are needed"):
        aggregate_images(*args, backend=None, **raster_kw, **kw)
    with pytest.raises(ValueError, match="needs top_down_raster_resolution"):
        aggregate_images(*args, top_down_raster_projection_savefile=tmp_path / "x.tif", top_down_points_file=export_points, backend=None, **kw)
    for res in (0.0, -2.0, np.nan):
        with pytest.raises(ValueError, match="needs top_down_raster_resolution"):
            aggregate_images(*args, top_down_raster_projection_savefile=tmp_path / "x.tif", top_down_raster_resolution=res,
                             top_down_points_file=export_points, backend=None, **kw)
    with pytest.raises(ValueError, match="top_down_raster_resolution is given but"):
        aggregate_images(*args, top_down_raster_resolution=1.0, top_down_points_file=export_points, backend=None, **kw)
    with pytest.raises(NotImplementedError, match="written as .tif / .tiff only"):
        aggregate_images(*args, top_down_raster_projection_savefile=tmp_path / "x.png", top_down_raster_resolution=1.0,
                         top_down_points_file=export_points, backend=None, **kw)
    with pytest.raises(ValueError, match=r"needs the \(V, 3\) ORIGINAL vertices"):
        aggregate_images(*args, top_down_points_file=export_points[:, :2], backend=None, **raster_kw, **kw)
    with pytest.raises(ValueError, match="top_down_points_file must hold"):
        aggregate_images(*args, top_down_points_file=export_points[:-1], backend=None, **raster_kw, **kw)
    with pytest.raises(ValueError, match="top_down_points_file is given but"):
        aggregate_images(*args, top_down_points_file=export_points, backend=None, **kw)
    with pytest.raises(ValueError, match="both given"):
        aggregate_images(*args, top_down_points_file=export_points, top_down_CRS="EPSG:32610", backend=None, **raster_kw, **kw)

    base = ["--mesh-file", "m.npz", "--mesh-CRS", "EPSG:4978", "--cameras-file", "c.xml", "--image-folder", "i", "--label-folder", "l",
            "--IDs-to-labels", "ids.json"]
    parsed = parse_args(base + ["--top-down-raster-projection-savefile", "classes.tif", "--top-down-raster-resolution", "0.25",
                                "--top-down-CRS", "EPSG:32610"])
    assert parsed.top_down_raster_projection_savefile == Path("classes.tif") and parsed.top_down_raster_resolution == 0.25
    assert parsed.top_down_CRS == "EPSG:32610" and parsed.top_down_vector_projection_savefile is None
    none = parse_args(base)
    assert none.top_down_raster_projection_savefile is None and none.top_down_raster_resolution is None
    import inspect

    assert set(vars(none)) <= set(inspect.signature(aggregate_images).parameters)      # main() hands every flag over by name


# -- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_source_name_the_new_call():
    main = (ROOT / "include" / "geograster.h").read_text()
    header = (ROOT / "include" / "geograster_nadir.h").read_text()
    source = (ROOT / "geograypher_amd" / "csrc" / "nadir.hip").read_text()
    internal = (ROOT / "geograypher_amd" / "csrc" / "gr_internal.hpp").read_text()
    decl = re.search(r"\bint gr_nadir_raster\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == 16 == len(_hip._NADIR_SIGNATURES["gr_nadir_raster"])
    kinds = ["pointer" if "*" in a else {"int64_t": "int64", "int32_t": "int"}[a.split()[0]] for a in (x.strip() for x in decl.split(","))]
    import ctypes

    bound = ["pointer" if t is ctypes.c_void_p else {ctypes.c_int64: "int64", ctypes.c_int32: "int", ctypes.c_int: "int"}[t]
             for t in _hip._NADIR_SIGNATURES["gr_nadir_raster"]]
    assert kinds == bound
    assert _hip.NADIR_SYMBOLS == ("gr_nadir_raster",) and re.search(r"\bint gr_nadir_raster\(gr_ctx \*c,", source)
    assert "gr_nadir_raster" not in main and main.count('#include "geograster_nadir.h"') == 1
    assert main.index('#include "geograster_nadir.h"') > main.index('#include "geograster_simplify.h"')
    assert "#define GR_VERSION 126" in main and "without a GR_VERSION bump" in " ".join(header.replace(" * ", " ").split())
    words = ("FACES", "BAD_INDEX", "ZERO_AREA", "NONFINITE_Z", "EMPTY_BOX", "ITEMS", "TESTS", "INSIDE", "SKIPPED", "COVERED", "WORDS")
    for value, word in enumerate(words):
        assert re.search(rf"GR_NADIR_STAT_{word} = {value}\b", main) and getattr(_hip, f"GR_NADIR_STAT_{word}") == value
        assert getattr(ns, word if word != "WORDS" else "STAT_WORDS") == value
    assert len(geospatial.TOP_DOWN_STAT_NAMES) == _hip.GR_NADIR_STAT_WORDS == 10
    assert any(p.name == "nadir.hip" for p in build.SOURCES) and "geograster_nadir.h" in Path(build.__file__).read_text()
    kernels = set(re.findall(r"void (k_nadir_\w+)\(", source))
    assert kernels == {"k_nadir_faces", "k_nadir_items", "k_nadir_finish"} and all(k in internal for k in kernels)
    assert 'stage_acquire(c, c->stage, p.finish(), s, "nadir-raster")' in source and "ExclusiveSum<int64_t> scan(c, p, F + 1);" in source
    # the defaults and limits of the decomposition: source, binding and stand-in agree
    for name, value in (("NADIR_SMALL_DEFAULT", ns.SMALL_CELLS_DEFAULT), ("NADIR_SMALL_MAX", _hip.NADIR_SMALL_CELLS_MAX),
                        ("NADIR_ITEM_ROWS_DEFAULT", ns.ITEM_ROWS_DEFAULT), ("NADIR_ITEM_ROWS_MAX", _hip.NADIR_ITEM_ROWS_MAX),
                        ("NADIR_ITEM_COLS", ns.ITEM_COLS)):
        assert re.search(rf"\b{name} = {value}\b", source), name


def test_the_library_exports_the_call_and_refuses_a_null_context():
    import ctypes

    lib = ctypes.CDLL(str(_hip.library_path()))
    fn = lib.gr_nadir_raster
    fn.restype, fn.argtypes = ctypes.c_int, _hip._NADIR_SIGNATURES["gr_nadir_raster"]
    assert fn(None, None, None, 0, None, 0, 0, 0, 1, 1, 0, 0, None, None, None, None) == _hip.GR_EINVAL
