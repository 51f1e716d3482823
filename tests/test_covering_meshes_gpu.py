"""gr_points_bounds / gr_cover_grid on the device against the numpy stand-in of tests/covering_standin.py (pinned by hand in
tests/test_covering_meshes_host.py).  Nothing here has a tolerance: minima, maxima and counts are exact in any order, so `count`
and the six bounds must EQUAL the stand-in's and z_max / z_min must be np.array_equal(..., equal_nan=True) to it -- bit-equal up
to the sign of a zero, which numpy's own max leaves to the order of its operands."""
import numpy as np
import pytest

from geograypher_amd import _hip
from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh
from geograypher_amd.utils import geometric, synthetic
from tests.covering_standin import CoverStandIn, bound_tables, cover_grid_np, points_bounds_np

pytestmark = pytest.mark.gpu

BLOCK, ROWS_PER_LANE = 512, 8   # k_cover_grid's launch (csrc/cover.hip): a second workgroup beyond BLOCK * ROWS_PER_LANE rows


def _np(t):
    return t.cpu().numpy()


def _check(hip, pts, N, stride=1, tables=None):
    """bounds, nonfinite and the grid of `pts` on the device against the stand-in; returns the device's (z_max, z_min, count)."""
    want_b, want_bad = points_bounds_np(pts, stride)
    bounds, bad = (_np(x) for x in hip.points_bounds(pts, stride))
    assert int(bad[0]) == want_bad
    assert np.array_equal(bounds, want_b)
    tabs = bound_tables(want_b, N) if tables is None else tables
    want = cover_grid_np(pts, *tabs, stride=stride)
    got = tuple(_np(x) for x in hip.cover_grid(pts, *tabs, stride=stride))
    assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2])
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1], equal_nan=True)
    assert np.array_equal(np.isnan(got[0]), want[2] == 0) and np.array_equal(np.isnan(got[1]), want[2] == 0)
    return got


def _edge_points(lo_, hi_, N, rng):
    """hi[i], lo[i + 1] and their neighbours in both directions for every i, on x with y fixed and on y with x fixed, and the
    two corners of the extent."""
    lo, hi = bound_tables([lo_, hi_, lo_, hi_], N)[:2]
    vals = np.concatenate([[hi[i], lo[i + 1], np.nextafter(hi[i], -np.inf), np.nextafter(hi[i], np.inf),
                            np.nextafter(lo[i + 1], -np.inf), np.nextafter(lo[i + 1], np.inf)] for i in range(N - 1)])
    vals = vals[(vals >= lo_) & (vals <= hi_)]          # the extent stays (lo_, hi_): the tables are the fixture's
    mid = lo_ + 0.37 * (hi_ - lo_)
    xy = np.concatenate([np.column_stack([vals, np.full(len(vals), mid)]), np.column_stack([np.full(len(vals), mid), vals]),
                         np.column_stack([vals, vals]), [[lo_, lo_], [hi_, hi_]]])
    return np.column_stack([xy, rng.uniform(-10.0, 10.0, len(xy))]), lo, hi


def _relations(lo, hi):
    return (int((hi[:-1] < lo[1:]).sum()), int((hi[:-1] > lo[1:]).sum()), int((hi[:-1] == lo[1:]).sum()))


def test_rounding_edges_unit_extent(hip):
    """Extent [0, 1], N = 11: neighbouring cells miss each other by an ulp once, overlap four times and share a bound five
    times.  Points on both bounds and one ulp to either side of each."""
    pts, lo, hi = _edge_points(0.0, 1.0, 11, np.random.default_rng(1))
    assert _relations(lo, hi) == (1, 4, 5), "the fixture no longer holds all three relations between neighbouring cells"
    _, _, count = _check(hip, pts, 11)
    assert count.sum() > len(pts)   # some points in two or four cells


def test_rounding_edges_non_representable_extent(hip):
    pts, lo, hi = _edge_points(-3.7, 12.9, 50, np.random.default_rng(2))
    miss, overlap, share = _relations(lo, hi)
    assert miss + overlap + share == 49 and min(miss, overlap) > 0, "the fixture holds no cells that miss or overlap by an ulp"
    _check(hip, pts, 50)


def test_smallest_grid_midpoint_in_all_four_cells(hip):
    pts = np.array([[0.0, 0.0, 1.0], [2.0, 2.0, 5.0], [1.0, 1.0, -3.0], [1.0, 0.25, 9.0], [0.5, 1.0, -8.0]])
    z_max, z_min, count = _check(hip, pts, 2)       # cells [-1, 1] and [1, 3] per axis
    # (1, 1, -3) is in all four, (1, 0.25, 9) in both columns of row 0, (0.5, 1, -8) in both rows of column 0
    assert count.tolist() == [[4, 2], [2, 2]]
    assert z_max.tolist() == [[9.0, -3.0], [9.0, 5.0]] and z_min.tolist() == [[-8.0, -8.0], [-3.0, -3.0]]


def test_zero_extent(hip):
    one = np.array([[2.5, -1.25, 7.0]])
    z_max, z_min, count = _check(hip, one, 4)
    assert np.all(count == 1) and np.all(z_max == 7.0) and np.all(z_min == 7.0)
    rng = np.random.default_rng(3)
    vertical = np.column_stack([np.full(300, 4.2), rng.uniform(-1, 1, 300), rng.normal(size=300)])
    z_max, _, count = _check(hip, vertical, 7)
    assert np.all(count == count[0]) and np.array_equal(z_max, np.tile(z_max[0], (7, 1))) and count[0].sum() >= 300
    horizontal = vertical[:, [1, 0, 2]]
    z_max, _, count = _check(hip, horizontal, 7)
    assert np.all(count == count[:, :1]) and count[:, 0].sum() >= 300
    _check(hip, vertical, 2)
    _check(hip, vertical, 70)     # the accumulators in global memory


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 256, 257, 511, 512, 513, BLOCK * ROWS_PER_LANE, BLOCK * ROWS_PER_LANE + 1,
                               2 * BLOCK * ROWS_PER_LANE + 7])
def test_sizes_around_the_launch_shape(hip, V):
    rng = np.random.default_rng(V)
    pts = np.column_stack([rng.uniform(-50, 50, V), rng.uniform(0, 30, V), rng.normal(0, 5, V)])
    _check(hip, pts, 9)
    _check(hip, pts, 60)


def test_stride(hip):
    rng = np.random.default_rng(5)
    pts = rng.uniform(-1, 1, (1000, 3))
    for stride in (3, 7, 1000, 5000):
        _, _, count = _check(hip, pts, 6, stride=stride)
        assert count.sum() >= len(pts[::stride])
    assert _np(hip.points_bounds(pts, 5000)[0]).tolist() == np.repeat(pts[0], 2).tolist()      # subsample > V: row 0 alone
    wide = rng.uniform(-1, 1, (400, 7))
    view = wide[:, 2:5][::-1]                                                                   # neither contiguous nor forward
    assert not view.flags.c_contiguous
    _check(hip, view, 6, stride=3)
    import torch

    dev_view = torch.as_tensor(wide, device=hip.device)[:, 2:5]
    assert not dev_view.is_contiguous()
    got = tuple(_np(x) for x in hip.cover_grid(dev_view, *bound_tables(points_bounds_np(wide[:, 2:5])[0], 6)))
    want = cover_grid_np(wide[:, 2:5], *bound_tables(points_bounds_np(wide[:, 2:5])[0], 6))
    assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))


def test_both_accumulator_paths(hip):
    """N = 56 is the last grid whose accumulators live in LDS, N = 57 the first in global memory."""
    assert _hip.HipRaster.COVER_LDS_N == 56 and _hip.HipRaster.COVER_MAX_N == 1024
    rng = np.random.default_rng(6)
    pts = np.column_stack([rng.uniform(0, 400, 20000), rng.uniform(0, 300, 20000), rng.normal(50, 20, 20000)])
    for N in (50, 56, 57, 64):
        _check(hip, pts, N)
    # the same tables through both paths: a 57-cell table whose last cell holds nothing is the 56-cell table's grid plus an empty
    # row and column
    tabs = bound_tables(points_bounds_np(pts)[0], 56)
    far = [np.append(t, 1e9) for t in tabs]
    lds = tuple(_np(x) for x in hip.cover_grid(pts, *tabs))
    glob = tuple(_np(x) for x in hip.cover_grid(pts, *far))
    for a, b in zip(lds, glob):
        assert np.array_equal(a, b[:56, :56], equal_nan=True)
    assert np.all(glob[2][56] == 0) and np.all(glob[2][:, 56] == 0) and np.isnan(glob[0][56]).all()
    _check(hip, pts[:5000], 1024)


def test_contention_in_one_cell(hip):
    rng = np.random.default_rng(7)
    n = 100_000
    pts = np.column_stack([rng.uniform(0.9, 1.1, n), rng.uniform(0.9, 1.1, n), rng.normal(0, 100, n)])
    pts[:2, :2] = [[0.0, 0.0], [2.0, 2.0]]     # the extent: cells [-0.5, 0.5] [0.5, 1.5] [1.5, 2.5]
    z_max, z_min, count = _check(hip, pts, 3)
    assert count[1, 1] == n - 2 and z_max[1, 1] == pts[2:, 2].max() and z_min[1, 1] == pts[2:, 2].min()


def test_tables_that_do_not_separate_their_cells(hip):
    """Tables the host never forms -- overlapping by half a cell, unsorted, one NaN bound -- still mean what the two comparisons
    say: the kernel may not assume the regular grid it usually gets."""
    rng = np.random.default_rng(8)
    pts = np.column_stack([rng.uniform(0, 10, 3000), rng.uniform(0, 10, 3000), rng.normal(size=3000)])
    centres = np.linspace(0, 10, 8)
    wide = (centres - 2.5, centres + 2.5, centres - 0.7, centres + 0.7)
    z_max, _, count = _check(hip, pts, 8, tables=wide)
    assert count.sum() > 3 * len(pts)
    perm = rng.permutation(8)
    _check(hip, pts, 8, tables=(wide[0][perm], wide[1][perm], wide[2], wide[3]))
    holed = [t.copy() for t in bound_tables([0, 10, 0, 10], 8)]
    holed[1][3] = np.nan
    _, _, count = _check(hip, pts, 8, tables=holed)
    assert np.all(count[3] == 0)


def test_non_finite_rows(hip):
    rng = np.random.default_rng(9)
    pts = rng.uniform(-1, 1, (200, 3))
    pts[10, 0] = np.nan
    pts[20, 2] = np.inf
    pts[30, 1] = -np.inf
    pts[31, 0] = np.nan            # skipped by stride 2
    for stride, want in ((1, 4), (2, 3)):
        bounds, bad = (_np(x) for x in hip.points_bounds(pts, stride))
        assert int(bad[0]) == want == points_bounds_np(pts, stride)[1]
        assert np.array_equal(bounds, points_bounds_np(pts, stride)[0]) and np.isfinite(bounds).all()
        with pytest.raises(ValueError, match=f"{want} of the visited points"):
            geometric.covering_meshes(pts, 5, subsample=stride, backend=hip)
    _check(hip, pts, 5, stride=2)   # the grid leaves such rows out as well
    only_bad = np.full((3, 3), np.nan)
    bounds, bad = (_np(x) for x in hip.points_bounds(only_bad))
    assert int(bad[0]) == 3 and bounds.tolist() == [np.inf, -np.inf] * 3


def test_errors(hip):
    pts = np.random.default_rng(10).uniform(0, 1, (50, 3))
    for N in (1, 1025):
        with pytest.raises(ValueError, match="gr_cover_grid"):
            hip.cover_grid(pts, *([np.linspace(0.0, 1.0, N)] * 4))
    with pytest.raises(ValueError, match="gr_cover_grid"):
        hip.cover_grid(pts, *bound_tables([0, 1, 0, 1], 4), stride=0)
    with pytest.raises(ValueError, match="gr_cover_grid"):
        hip.cover_grid(pts[:0], *bound_tables([0, 1, 0, 1], 4))
    with pytest.raises(ValueError, match="gr_points_bounds"):
        hip.points_bounds(pts, 0)
    with pytest.raises(ValueError, match="gr_points_bounds"):
        hip.points_bounds(pts[:0])
    with pytest.raises(ValueError, match=r"\(V, 3\)"):
        hip.points_bounds(pts[:, :2])
    with pytest.raises(ValueError, match="one length"):
        hip.cover_grid(pts, np.zeros(4), np.zeros(4), np.zeros(5), np.zeros(5))
    _check(hip, pts, 4)             # the context still works


@pytest.mark.parametrize("slope", [0.0, 2.0])
def test_end_to_end_on_the_simple_mesh(hip, slope):
    """export_covering_meshes(N=8, z_buffer=(0, 0.5), subsample=2) on the synthetic simple mesh equals the host route over the
    stand-in, vertices bit for bit; the pair then clips vertical rays over the interior, all of which are kept.

    The simple mesh is the plane z = 0: its ceiling is z = 0 and its floor, lifted by the 0.5 buffer, z = 0.5 -- ABOVE the
    ceiling, so there a ray starts (on the ceiling) below where it ends, at exactly those two heights.  `start z >= end z` can
    hold only where a cell's relief exceeds the buffer: slope 2 is the same mesh tilted to z = 2 x (cells 4 / 7 wide: the
    ceiling clears the floor by 4 h - 0.5 = 0.64 inside and 2 h - 0.5 = 0.07 at the rim, h = 2 / 7), where it must."""
    (points, faces), _ = synthetic.make_simple_mesh([], None)
    points = points + np.array([0.0, 0.0, slope]) * points[:, :1]
    mesh = TexturedPhotogrammetryMesh((points, faces), backend=hip, log_level="ERROR")
    (up, up_f), (low, low_f) = mesh.export_covering_meshes(N=8, z_buffer=(0, 0.5), subsample=2)
    (w_up, w_up_f), (w_low, w_low_f) = geometric.covering_meshes(points, 8, z_buffer=(0, 0.5), subsample=2, backend=CoverStandIn())
    assert up.tobytes() == w_up.tobytes() and low.tobytes() == w_low.tobytes() and up.shape == (64, 3)
    assert np.array_equal(up_f, w_up_f) and np.array_equal(low_f, w_low_f) and len(up_f) == 2 * 7 * 7
    rng = np.random.default_rng(11)
    origins = np.column_stack([rng.uniform(-1.9, 1.9, 200), rng.uniform(-1.9, 1.9, 200), np.full(200, 10.0)])
    directions = np.tile([0.0, 0.0, -1.0], (200, 1))
    starts, ends, dirs, ids = geometric.clip_line_segments(((up, up_f), (low, low_f)), origins, directions, np.arange(200),
                                                           backend=hip)
    assert np.array_equal(ids, np.arange(200))
    assert np.array_equal(starts[:, :2], origins[:, :2]) and np.array_equal(ends[:, :2], origins[:, :2])
    if slope == 0.0:
        # t is about 10, formed by a handful of float64 operations: a few ulps of 10
        assert np.abs(starts[:, 2]).max() <= 1e-13 and np.abs(ends[:, 2] - 0.5).max() <= 1e-13
    else:
        assert np.all(starts[:, 2] >= ends[:, 2]) and np.allclose(dirs, directions)
