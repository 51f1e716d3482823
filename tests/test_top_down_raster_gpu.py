"""gr_nadir_raster on the device against tests/nadir_standin.py (rules N1-N9 of DESIGN.md 8r; the stand-in works in Python integers
and Python floats and is pinned to hand-worked cases by tests/test_top_down_raster_host.py).  Every comparison is bit for bit: the
face plane, the bit patterns of the height plane and all ten statistics words."""
import sys
from contextlib import contextmanager
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import nadir_standin as ns  # noqa: E402
from geograypher_amd import _hip  # noqa: E402
from geograypher_amd.utils.geometric import burn_work_items, row_centre_boxes, row_ring_ranges  # noqa: E402
from geograypher_amd.utils.geospatial import points_to_cell_units, rings_to_cell_units, top_down_raster  # noqa: E402
from geograypher_amd.utils.raster import invert_affine  # noqa: E402
from tests.fenced_backend import POISON, FencedHipRaster, fenced  # noqa: E402
from tests.test_top_down_raster_host import IDENTITY, height_field  # noqa: E402

pytestmark = pytest.mark.gpu
ONE = 65536


def cells(points):
    """Cell coordinates (multiples of 1 / 65536, as the scenes below use) -> (V, 2) int64 cell units."""
    return np.rint(np.asarray(points, dtype=np.float64).reshape(-1, 2) * ONE).astype(np.int64)


def device(hip, vq, z, faces, window, **kw):
    face, zz, stats = hip.nadir_rasterizer(vq, np.asarray(z, dtype=np.float64), np.asarray(faces, dtype=np.int32).reshape(-1, 3)).window(*window, **kw)
    return face.cpu().numpy(), zz.cpu().numpy(), stats.cpu().numpy()


def same(got, want):
    face, zz, stats = got
    assert face.dtype == np.int32 and zz.dtype == np.float64 and face.shape == zz.shape == want[0].shape
    assert np.array_equal(face, want[0])
    assert np.array_equal(zz.view(np.uint64), np.ascontiguousarray(want[1]).view(np.uint64))
    assert np.array_equal(stats, want[2]), (stats, want[2])


def check(hip, vq, z, faces, window, **kw):
    got = device(hip, vq, z, faces, window, **kw)
    same(got, ns.nadir_raster(vq, z, np.asarray(faces).reshape(-1, 3), window, **kw))
    return got


def soup(F, seed, side=24):
    """F random triangles of a few cells each over a side x side grid, in several sheets, on the 1/16-cell lattice: edges and
    vertices meet cell centres now and then."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0, side, (F, 1, 2))
    points = np.rint((centre + rng.uniform(-2.5, 2.5, (F, 3, 2))) * 16) / 16
    return cells(points), rng.normal(0, 3, 3 * F).round(2), np.arange(3 * F, dtype=np.int32).reshape(F, 3)


# -- the scenes of the issue ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 63, 64, 65, 257])
def test_face_counts_round_the_wave_and_the_workgroup(hip, F):
    vq, z, faces = soup(F, seed=F)
    _, _, stats = check(hip, vq, z, faces, (0, 0, 24, 24))
    assert stats[ns.FACES] + stats[ns.ZERO_AREA] == F and stats[ns.INSIDE] >= stats[ns.COVERED] > 0


def boundary_scene():
    """Faces whose clipped boxes hold 0, 1, 16 and 17 centres: with small_cells = 16, 16 is the largest a lane walks and 17 the
    smallest that becomes items."""
    points = [(0.6, 0.6), (0.9, 0.6), (0.7, 0.9),             # between centres: an empty box
              (2.2, 0.2), (2.9, 0.3), (2.4, 0.9),             # round the centre (2.5, 0.5): 1
              (0.375, 2.375), (3.625, 2.375), (0.375, 5.625),    # 4 x 4; its hypotenuse runs through four centres
              (0.4, 7.3), (16.6, 7.3), (8.0, 7.7)]            # 17 x 1
    return cells(points), np.arange(12, dtype=np.float64), np.arange(12, dtype=np.int32).reshape(4, 3)


def test_boxes_of_0_1_16_and_17_centres(hip):
    vq, z, faces = boundary_scene()
    face, _, stats = check(hip, vq, z, faces, (0, 0, 24, 12), small_cells=16)
    assert stats[ns.EMPTY_BOX] == 1 and stats[ns.TESTS] == 1 + 16 + 17 and stats[ns.ITEMS] == 1
    assert face[0, 2] == 1 and (face == 3).sum() == 8 and (face == 2).sum() == 6 and (face == 0).sum() == 0
    assert check(hip, vq, z, faces, (0, 0, 24, 12), small_cells=17)[2][ns.ITEMS] == 0
    assert check(hip, vq, z, faces, (0, 0, 24, 12), small_cells=15)[2][ns.ITEMS] == 2
    assert check(hip, vq, z, faces, (0, 0, 24, 12))[2][ns.ITEMS] == 0                 # the default, 256, walks all four in a lane
    # the same boundary at the default: boxes of 16 x 16 and 17 x 16 - 15 = 257 centres
    points = [(0.4, 0.4), (15.6, 0.4), (0.4, 15.6), (20.4, 0.4), (36.6, 0.4), (20.4, 15.6), (36.6, 15.6)]
    vq2, z2, faces2 = cells(points), np.arange(7, dtype=np.float64), [[0, 1, 2], [3, 4, 5], [4, 6, 5]]
    _, _, stats = check(hip, vq2, z2, faces2, (0, 0, 40, 17))
    assert stats[ns.TESTS] == 256 + 2 * 17 * 16 and stats[ns.ITEMS] == 2
    _, _, stats = check(hip, vq2, z2, faces2, (0, 0, 36, 17))                           # the window cuts the two to 16 x 16: no items
    assert stats[ns.TESTS] == 3 * 256 and stats[ns.ITEMS] == 0


def wide_scene():
    """One face of 1100 x 3 centres in a 1200 x 8 grid -- a span above 2^26 units, so the 128-bit determinant, and 18 items of 64
    columns --, under it a small face that it hides and beside it one that stays visible."""
    points = [(10.3, 1.4), (1110.3, 2.5), (500.7, 4.4),
              (300.2, 2.1), (303.9, 2.2), (301.0, 2.9),
              (1150.2, 5.1), (1153.9, 5.2), (1151.0, 7.9)]
    return cells(points), np.array([5.0, 7.0, 9.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0]), np.arange(9, dtype=np.int32).reshape(3, 3)


def test_one_wide_face_of_many_items(hip):
    vq, z, faces = wide_scene()
    window = (0, 0, 1200, 8)
    face, zz, stats = check(hip, vq, z, faces, window)
    assert int(vq[:3, 0].max() - vq[:3, 0].min()) > 1 << 26
    assert stats[ns.TESTS] == 1100 * 3 + 4 * 1 + 4 * 3 and stats[ns.ITEMS] == 18 and (face == 0).sum() > 1000
    assert (face == 1).sum() == 0 and (face == 2).sum() > 0 and stats[ns.INSIDE] > stats[ns.COVERED]
    assert check(hip, vq, z, faces, window, item_rows=1)[2][ns.ITEMS] == 54
    # a window inside the wide face: its clipped box is narrow, its span is not
    check(hip, vq, z, faces, (290, 1, 40, 4))


def test_two_sheets_ties_and_signed_zeros(hip):
    square = [(0, 0), (4, 0), (4, 4), (0, 4)]
    vq = cells(square + square)
    ground, crown = [[0, 1, 2], [0, 2, 3]], [[4, 5, 6], [4, 6, 7]]
    window = (0, 0, 4, 4)
    for faces, upper in ((ground + crown, {2, 3}), (crown + ground, {0, 1})):
        face, zz, _ = check(hip, vq, [1.0] * 4 + [5.0] * 4, faces, window)
        assert set(np.unique(face).tolist()) == upper and np.all(zz == 5.0)
    face, _, _ = check(hip, vq, [2.0] * 8, crown + ground, window)
    assert set(np.unique(face).tolist()) == {0, 1}                       # equal heights: the lower face
    tri = [(0, 0), (4, 0), (0, 4)]
    face, zz, _ = check(hip, cells(tri + tri), [-0.0, -5e-324, -5e-324, 0.0, 0.0, 0.0], [[0, 1, 2], [3, 4, 5]], window)
    assert face[0, 1] == 1 and zz.view(np.uint64)[0, 1] == 0             # +0.0 beats -0.0, whatever the index
    alone = check(hip, cells(tri), [-0.0, -5e-324, -5e-324], [[0, 1, 2]], window)
    assert alone[1].view(np.uint64)[0, 1] == 1 << 63
    # four faces round a cell centre, both diagonals through centres: one owner each
    points = [(0, 0), (3, 0), (3, 3), (0, 3), (1.5, 1.5)]
    _, _, stats = check(hip, cells(points), [0.0] * 5, [[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], window)
    assert stats[ns.INSIDE] == stats[ns.COVERED] == 9


def single_sheet(transform=(0.4, 0.3, -1.0, 0.3, -0.4, 3.0)):
    points, faces = height_field(9, seed=7)
    return points, faces, points_to_cell_units(points[:, :2], invert_affine(transform)), invert_affine(transform)


def test_a_window_that_cuts_faces_on_all_four_sides(hip):
    points, faces, vq, _ = single_sheet(IDENTITY)
    whole = check(hip, vq, points[:, 2], faces, (-1, -1, 11, 11))
    for window in ((2, 3, 5, 4), (-1, 4, 11, 1), (4, -1, 1, 11)):
        c, r, w, h = window
        face, zz, _ = check(hip, vq, points[:, 2], faces, window)
        assert np.array_equal(face, whole[0][r + 1:r + 1 + h, c + 1:c + 1 + w])
        assert np.array_equal(zz.view(np.uint64), np.ascontiguousarray(whole[1][r + 1:r + 1 + h, c + 1:c + 1 + w]).view(np.uint64))
    assert np.all(check(hip, vq, points[:, 2], faces, (2, 3, 5, 4))[0] >= 0)        # inside the sheet: every face there is cut


def test_uncounted_faces_and_an_empty_mesh(hip):
    points = cells([(0, 0), (4, 0), (0, 4), (2, 2), (4, 4)])
    z = [0.0, 1.0, 2.0, np.nan, 3.0]
    faces = [[0, 1, 2], [0, 4, 0], [0, 3, 4], [1, 3, 2], [1, 4, 2]]
    _, _, stats = check(hip, points, z, faces, (0, 0, 4, 4))
    assert stats[:5].tolist() == [2, 0, 1, 2, 0]
    with pytest.raises(ValueError, match=r"gr_nadir_raster: 2 faces name a vertex outside \[0, 5\)"):
        device(hip, points, z, faces + [[0, 1, 5], [-1, 3, 2]], (0, 0, 4, 4))
    face, zz, stats = check(hip, points, z, np.zeros((0, 3), dtype=np.int32), (0, 0, 3, 2))
    assert np.all(face == -1) and np.all(zz.view(np.uint64) == ns.NAN_BITS) and not stats.any()
    check(hip, np.zeros((0, 2), dtype=np.int64), np.zeros(0), np.zeros((0, 3), dtype=np.int32), (-2, -2, 3, 3))
    check(hip, points, z, [[0, 1, 2]], (10, 10, 4, 4))                   # takes part, empty box


# -- further checks ---------------------------------------------------------------------------------------------------------------------
def test_ids_equal_the_devices_own_burn_on_a_single_sheet(hip):
    """The burn walks its rows through the 128-bit Z3, the top-down raster through the int64 Z3 or the 128-bit one per face -- ONE
    function (edge_crossing_strict of geom_dev.hpp), so both give the same membership.  On the single sheet the planes are equal;
    in the wide scene (a span above 2^26 units: the 128-bit determinant on both sides) the burn's highest row is the small face 1
    where the top-down raster shows face 0, which hides it."""
    points, faces, vq, inverse = single_sheet()
    rv, _ = rings_to_cell_units([points[f, :2] for f in faces], inverse)
    wide_vq, wide_z, wide_faces = wide_scene()
    for vq, z, faces, rv, window, hidden in ((vq, points[:, 2], faces, rv, (-3, -4, 20, 18), {}),
                                             (wide_vq, wide_z, wide_faces, wide_vq[wide_faces].reshape(-1, 2), (5, 0, 1190, 7), {1: 0})):
        face, _, stats = check(hip, vq, z, faces, window)
        off, rp = 3 * np.arange(len(faces) + 1, dtype=np.int64), np.arange(len(faces), dtype=np.int32)
        burner = hip.polygon_burner(rv, off, rp, len(faces))
        items = burn_work_items(row_centre_boxes(rv, off, rp, len(faces)), row_ring_ranges(rp, len(faces)), window)
        rows, _, burn_stats = burner.window(*window, items, want_values=False)
        rows = rows.cpu().numpy()
        assert np.array_equal(rows >= 0, face >= 0) and int(burn_stats[_hip.GR_BURN_STAT_INSIDE]) == stats[ns.INSIDE] >= stats[ns.COVERED] > 50
        for under, over in hidden.items():
            assert (rows == under).sum() > 0
            rows = np.where(rows == under, over, rows)
        assert np.array_equal(rows, face) and (hidden or stats[ns.INSIDE] == stats[ns.COVERED])


def test_the_decomposition_changes_no_byte_and_two_runs_are_equal(hip):
    vq, z, faces = soup(200, seed=11, side=40)
    vq = np.vstack([vq, cells([(0.3, 10.4), (70.3, 10.6), (30.7, 12.4)])])     # a face of 70 x 2 centres among them: two items
    z = np.concatenate([z, [4.0, 2.0, 6.0]])
    faces = np.vstack([faces, [[600, 601, 602]]]).astype(np.int32)
    window = (0, 0, 80, 40)
    base = check(hip, vq, z, faces, window)
    rasterizer = hip.nadir_rasterizer(vq, z, faces)
    seen = set()
    for small_cells in (1, 16, 4096):
        for item_rows in (1, 8):
            face, zz, stats = (t.cpu().numpy() for t in rasterizer.window(*window, small_cells=small_cells, item_rows=item_rows))
            assert np.array_equal(face, base[0]) and np.array_equal(zz.view(np.uint64), base[1].view(np.uint64))
            assert np.array_equal(np.delete(stats, ns.ITEMS), np.delete(base[2], ns.ITEMS))
            seen.add(int(stats[ns.ITEMS]))
    assert len(seen) >= 4 and 0 in seen
    again = device(hip, vq, z, faces, window)
    assert all(np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)
               for a, b in zip(again, base))


def test_bands_of_top_down_raster_equal_one_window(hip):
    points, faces = height_field(9, seed=13)
    like = ((19, 17), (0.5, 0.0, -0.2, 0.0, -0.5, 8.9))
    whole = top_down_raster(points, faces, like, backend=hip)
    parts = top_down_raster(points, faces, like, backend=hip, max_device_bytes=12 * 17 * 5)
    assert np.array_equal(parts[0], whole[0]) and np.array_equal(parts[1].view(np.uint64), whole[1].view(np.uint64))
    assert parts[2]["covered"] == whole[2]["covered"] == int((whole[0] >= 0).sum()) > 100 and parts[2]["inside"] == whole[2]["inside"]
    want = ns.nadir_raster(points_to_cell_units(points[:, :2], invert_affine(like[1])), points[:, 2], faces, (0, 0, 17, 19))
    assert np.array_equal(whole[0], want[0]) and np.array_equal(whole[1].view(np.uint64), want[1].view(np.uint64))
    tensors = top_down_raster(points, faces, like, backend=hip, max_device_bytes=12 * 17 * 5, return_tensor=True)
    assert tensors[0].device.type == "cuda" and np.array_equal(tensors[0].cpu().numpy(), whole[0])


def test_refusals_happen_without_a_launch(hip):
    vq, z, faces = boundary_scene()
    rasterizer = hip.nadir_rasterizer(vq, z, faces)
    for args, match in (((0, 0, 0, 4), "empty or leaves"), ((1 << 23, 0, 1, 1), "empty or leaves"), ((0, 0, 4, 4, -1), "small_cells"),
                        ((0, 0, 4, 4, 0, 2000), "item_rows")):
        with pytest.raises(ValueError, match="gr_nadir_raster: .*" + match):
            rasterizer.window(*args)
    with pytest.raises(ValueError, match="gr_nadir_raster: .*2\\^40"):
        hip.nadir_rasterizer(vq + (1 << 40), z, faces)
    # the library's own answers: GR_EINVAL and planes that were never touched
    face = torch.full((4, 4), 77, dtype=torch.int32, device=hip.device)
    zz = torch.full((4, 4), 7.5, dtype=torch.float64, device=hip.device)
    stats = torch.full((_hip.GR_NADIR_STAT_WORDS,), 5, dtype=torch.int64, device=hip.device)
    t = {k: torch.as_tensor(v).to(hip.device) for k, v in (("vq", vq), ("z", z), ("faces", faces))}
    good = dict(vq=t["vq"].data_ptr(), z=t["z"].data_ptr(), V=12, faces=t["faces"].data_ptr(), F=4, col_off=0, row_off=0, width=4, height=4,
                small_cells=0, item_rows=0, face=face.data_ptr(), zz=zz.data_ptr(), stats=stats.data_ptr())
    for change in (dict(width=0), dict(height=-1), dict(col_off=1 << 23), dict(row_off=-(1 << 23)), dict(col_off=(1 << 23) - 2),
                   dict(V=-1), dict(F=-1), dict(F=2 ** 31 - 1), dict(small_cells=-1), dict(small_cells=65537), dict(item_rows=1025),
                   dict(vq=None), dict(z=None), dict(faces=None), dict(face=None), dict(zz=None), dict(stats=None),
                   dict(zz=zz.data_ptr() + 4)):
        rc = hip._rc("gr_nadir_raster", *{**good, **change}.values(), hip._stream())
        assert rc == _hip.GR_EINVAL, change
        with pytest.raises(ValueError, match="gr_nadir_raster"):
            hip._check(rc, "gr_nadir_raster")
    torch.cuda.synchronize()
    assert bool((face == 77).all()) and bool((zz == 7.5).all()) and bool((stats == 5).all())
    assert hip._rc("gr_nadir_raster", *good.values(), hip._stream()) == _hip.GR_OK
    torch.cuda.synchronize()
    same((face.cpu().numpy(), zz.cpu().numpy(), stats.cpu().numpy()), ns.nadir_raster(vq, z, faces, (0, 0, 4, 4)))


# -- fenced outputs, poisoned scratch ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    backend = FencedHipRaster(0)
    yield backend
    backend.close()


@contextmanager
def poison(ctx, bits):
    ctx.set_option(_hip.GR_OPT_DEBUG, bits)
    try:
        yield
    finally:
        ctx.set_option(_hip.GR_OPT_DEBUG, 0)


@pytest.mark.parametrize("bits", [0, _hip.GR_DBG_POISON_STAGE, _hip.GR_DBG_POISON_STAGE_7F], ids=["off", "ff", "7f"])
def test_between_fences_on_a_poisoned_arena(ctx, bits):
    """Every byte of both planes and of the statistics is written (the poison of the fenced allocator would show: 0x7F7F7F7F is
    no face, 1.38e306 no height of these scenes), nothing beside them is, and the list, the counts and their scan are initialised
    by the call (the arena starts as 0xFF or 0x7F)."""
    assert POISON == 0x7F
    scenes = [(*boundary_scene(), (0, 0, 24, 12), dict(small_cells=16)), (*wide_scene(), (5, 0, 1190, 7), dict(item_rows=2)),
              (*soup(130, seed=3), (-3, -3, 31, 29), dict(small_cells=4))]
    for vq, z, faces, window, kw in scenes:
        want = ns.nadir_raster(vq, z, faces, window, **kw)
        assert want[2][ns.ITEMS] > 0 and (want[0] == -1).any() and (want[0] >= 0).any()
        with poison(ctx, bits), fenced(ctx):
            inputs = [torch.as_tensor(a).to(ctx.device) for a in (vq, np.asarray(z, dtype=np.float64), faces)]
            clones = [t.clone() for t in inputs]
            face, zz, stats = ctx.nadir_rasterizer(*inputs).window(*window, **kw)
            same((face.cpu().numpy(), zz.cpu().numpy(), stats.cpu().numpy()), want)
            for t, clone in zip(inputs, clones):
                assert torch.equal(t.view(torch.int64) if t.dtype == torch.float64 else t, clone.view(torch.int64) if t.dtype == torch.float64 else clone)
