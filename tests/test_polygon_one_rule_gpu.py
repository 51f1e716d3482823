"""The device's twin of tests/test_polygon_one_rule_host.py: gr_face_polygon_index and gr_points_in_region (D = 0) walk the ring
table with ONE crossing rule and one ring span (csrc/geom_dev.hpp), so on the lattice scene each equals its stand-in on every
point, statistics words included, and the two agree with each other.  All comparisons are exact equality."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import region_standin as rs  # noqa: E402
import vector_standin as vs  # noqa: E402
from geograypher_amd.utils.geometric import polygon_cell_table  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene():
    """The lattice scene with the stand-ins' answers: computed once, shared, not modified."""
    points_q, faces, table = vs.lattice_scene()
    cells = polygon_cell_table(table[4])
    row, _ = vs.StandInBackend().face_polygon_index(points_q, faces, *table, cells)
    mask, info = rs.points_in_region_np(points_q, table, 0)
    for a in (row, mask, info["wide"]):
        a.setflags(write=False)
    return points_q, faces, table, cells, row, mask, info["wide"]


def index_words(points_q, faces, table, cells, row):
    """The statistics block of gr_face_polygon_index as V5 defines it: a face walks the list of ITS cell, highest row first, starts
    a ring walk for every row whose box holds 3 x centre and stops at the row it finds (`vector_standin` tries every row and
    takes the longest list of the whole grid: upper bounds of the first and third word)."""
    (x0, y0, cw, ch, nx, ny), offsets = (int(v) for v in cells[0]), np.asarray(cells[1])
    c3, b3 = points_q[faces].sum(axis=1), 3 * table[4]
    hit = (b3[:, 0] <= c3[:, :1]) & (c3[:, :1] <= b3[:, 2]) & (b3[:, 1] <= c3[:, 1:]) & (c3[:, 1:] <= b3[:, 3])
    tested = int((hit & (np.arange(len(b3)) >= np.maximum(row, 0)[:, None])).sum())
    ix, iy = (c3[:, 0] - x0) // cw, (c3[:, 1] - y0) // ch
    ok = (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny)
    longest = int(np.diff(offsets)[(iy * nx + ix)[ok]].max()) if ok.any() else 0
    return [tested, int((row >= 0).sum()), longest, 0]


def device_answers(hip, points_q, faces, table, cells):
    row, row_stats = hip.face_polygon_index(points_q, faces, *table, cells)
    mask, mask_stats = hip.points_in_region(points_q, *table, 0)
    return row.cpu().numpy(), row_stats.cpu().numpy().tolist(), mask.cpu().numpy(), mask_stats.cpu().numpy().tolist()


def check(hip, scene, n, table=None):
    points_q, faces, scene_table, cells, want_row, want_mask, wide = scene
    table = scene_table if table is None else table
    row, row_stats, mask, mask_stats = device_answers(hip, points_q[:n], faces[:n], table, cells)
    print(f"[one_rule] n={n}: inside {int(mask.sum())}, index words {row_stats}, region words {mask_stats}")
    assert row.dtype == np.int32 and np.array_equal(row, want_row[:n])
    assert mask.dtype == np.bool_ and np.array_equal(mask, want_mask[:n])
    assert np.array_equal(row >= 0, mask)
    assert row_stats == index_words(points_q[:n], faces[:n], scene_table, cells, want_row[:n])
    assert mask_stats == [int(want_mask[:n].sum()), 0, int(wide[:n].sum()), 0]


def test_both_kernels_equal_their_stand_ins_and_each_other(hip, scene):
    assert len(scene[0]) == 3102 and int(scene[5].sum()) == 843
    check(hip, scene, 3102)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_point_counts_around_a_wave_and_a_workgroup(hip, scene, n):
    check(hip, scene, n)


def test_short_ring_and_offset_beyond_the_vertices_are_clamped_in_both_kernels(hip, scene):
    """Two rings appended to the last row: one of two vertices, one whose end offset lies far beyond the vertex count (the span is
    clamped to nothing).  Both stand-ins skip such rings; the answers are those of the table without them."""
    rv, roff, rpoly, rhole, boxes = scene[2]
    n_rv, last = len(rv), int(rpoly[-1])
    table = (np.concatenate([rv, rv[:2]]), np.concatenate([roff, [n_rv + 2, n_rv + (1 << 40)]]).astype(np.int64),
             np.concatenate([rpoly, [last, last]]).astype(np.int32), np.concatenate([rhole, [0, 0]]).astype(np.int32), boxes)
    points_q, faces = scene[0], scene[1]
    assert np.array_equal(vs.face_polygon_index_np(points_q, faces, table)[0], scene[4])       # the stand-ins skip them
    assert np.array_equal(rs.points_in_region_np(points_q[:257], table, 0)[0], scene[5][:257])
    check(hip, scene, 3102, table)


def test_an_end_offset_beyond_the_vertices_is_cut_at_the_last_vertex(hip, scene):
    """The last ring (the diamond, four vertices) with its end offset far beyond the vertex count: clamped, its span is still the
    diamond, so every answer stays.  This pins WHERE the span is cut, not only that nothing outside is read: cut any shorter,
    the ring has fewer than three vertices and the row is empty.  (The stand-ins slice the vertex array, which cuts there too.)"""
    points_q, faces, (rv, roff, rpoly, rhole, boxes) = scene[:3]
    assert int(roff[-1]) == len(rv) and int(roff[-1] - roff[-2]) == 4 and int((scene[4] == int(rpoly[-1])).sum()) > 0
    table = (rv, np.concatenate([roff[:-1], [len(rv) + (1 << 40)]]).astype(np.int64), rpoly, rhole, boxes)
    assert np.array_equal(vs.face_polygon_index_np(points_q, faces, table)[0], scene[4])
    check(hip, scene, 3102, table)
