"""gr_burn_polygons on the device against tests/burn_standin.py (rules B1-B7 of DESIGN.md 8m; the stand-in works in Python integers
and is pinned to hand-worked cases by tests/test_polygon_burn_host.py).  All integer: every comparison is np.array_equal -- both
planes and the statistics words.  Word 0, the cells tested, is the cells of the work items."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import burn_standin as bs  # noqa: E402
from geograypher_amd import _hip  # noqa: E402
from geograypher_amd.utils.geometric import burn_work_items, row_centre_boxes, row_ring_ranges, zonal_work_items  # noqa: E402
from geograypher_amd.utils.geospatial import rings_to_cell_units  # noqa: E402
from geograypher_amd.utils.raster import invert_affine  # noqa: E402

pytestmark = pytest.mark.gpu
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


class Scene:
    """A ring table, its burner on the device and the tables of its work items: many windows, one upload."""

    def __init__(self, hip, rings, rows, P, values=None, transform=IDENTITY):
        self.rings, self.ring_rows, self.P, self.values, self.inverse = rings, [int(r) for r in rows], P, values, invert_affine(transform)
        self.rv, self.off = rings_to_cell_units(rings, self.inverse)
        self.rp = np.asarray(rows, dtype=np.int32)
        self.burner = hip.polygon_burner(self.rv, self.off, self.rp, P, values)
        self.boxes, self.ranges = row_centre_boxes(self.rv, self.off, self.rp, P), row_ring_ranges(self.rp, P)
        self.rings_q = bs.to_cell_units(rings, self.inverse)

    def device(self, window, fill=255, block=(64, 16), want_values=True):
        items = burn_work_items(self.boxes, self.ranges, window, block)
        rows, out, stats = self.burner.window(*window, items, fill=fill, want_values=want_values)
        return rows.cpu().numpy(), None if out is None else out.cpu().numpy(), stats.cpu().numpy(), items

    def check(self, window, fill=255, block=(64, 16), want_values=True):
        rows, out, stats, items = self.device(window, fill, block, want_values)
        want_rows, want_out, want_stats = bs.burn(self.rings_q, self.ring_rows, self.P, window, self.values if want_values else None, fill)
        want_stats[0] = int((items[:, 3].astype(np.int64) * items[:, 4]).sum())
        assert rows.dtype == np.int32 and rows.shape == (window[3], window[2]) and np.array_equal(rows, want_rows)
        if want_values:
            assert out.dtype == np.uint8 and np.array_equal(out, want_out)
        else:
            assert out is None
        assert np.array_equal(stats, want_stats), (stats, want_stats)
        return rows, out, stats


def square(x0, y0, x1, y1):
    return np.array([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], dtype=np.float64)


def test_hand_worked_cases(hip):
    window = (0, 0, 4, 4)
    rows, out, stats = Scene(hip, [square(1, 1, 3, 3)], [0], 1, [7]).check(window)
    assert out.tolist() == [[255, 255, 255, 255], [255, 7, 7, 255], [255, 7, 7, 255], [255, 255, 255, 255]] and stats[:5].tolist() == [4, 4, 4, 4, 0]
    rows, out, stats = Scene(hip, [square(0, 0, 3, 3), square(1, 1, 4, 4)], [0, 1], 2, [7, 9]).check(window, fill=0)
    assert rows.tolist() == [[0, 0, 0, -1], [0, 1, 1, 1], [0, 1, 1, 1], [-1, 1, 1, 1]] and stats[1] == 18 and stats[2] == 14
    for ring in (square(0.5, 0.5, 2.5, 2.5), square(0.5, 0.5, 2.5, 2.5)[::-1]):      # edges through centres: left and top in, right and bottom out
        rows, _, _ = Scene(hip, [ring], [0], 1, [1]).check(window)
        assert rows.tolist() == [[0, 0, -1, -1], [0, 0, -1, -1], [-1, -1, -1, -1], [-1, -1, -1, -1]]
    rows, _, _ = Scene(hip, [square(0, 0, 4, 4), square(1, 1, 3, 3)], [0, 0], 1, [1]).check(window)
    assert rows.tolist() == [[0, 0, 0, 0], [0, -1, -1, 0], [0, -1, -1, 0], [0, 0, 0, 0]]
    rows, out, stats = Scene(hip, [square(0, 0, 1, 1), square(3, 3, 4, 4), np.array([(0.0, 0.0), (4.0, 4.0)])], [1, 1, 1], 2, [3, 5]).check(window)
    assert rows[0, 0] == rows[3, 3] == 1 and (rows >= 0).sum() == 2 and stats[3] == 4 and stats[4] == 1
    empty = Scene(hip, [], [], 3, [1, 2, 3])                                         # rows without a ring: everything is fill
    rows, out, _ = empty.check(window, fill=9)
    assert (rows == -1).all() and (out == 9).all()
    assert (Scene(hip, [], [], 0, np.zeros(0, np.uint8)).check(window, fill=9)[1] == 9).all()


def shapes_scene(hip, H, W):
    rings = [square(-1, -1, W + 1, H + 1), square(0.2 * W, 0.2 * H, 0.75 * W + 0.4, 0.75 * H + 0.4), np.array([(0.0, 0.0), (W, 0.3 * H), (0.4 * W, H)])]
    return Scene(hip, rings, [0, 1, 2], 3, [10, 20, 30])


@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (70, 1), (65, 257)])
def test_window_shapes(hip, shape):
    H, W = shape
    shapes_scene(hip, H, W).check((0, 0, W, H))


def test_windows_with_negative_offsets_and_past_every_polygon(hip):
    scene = Scene(hip, [square(-20.3, -11.2, 9.6, 14.1), square(-3.5, -30, 2.5, 40), square(5, 5, 30, 30)], [0, 1, 2], 3, [1, 2, 3])
    rows, _, stats = scene.check((-25, -35, 40, 50))
    assert rows[0, 0] == -1 and (rows == 1).any() and (rows == 0).any() and stats[2] > 0
    rows, out, stats = scene.check((100, 200, 33, 9), fill=77)                       # hangs past every polygon: no work item at all
    assert (rows == -1).all() and (out == 77).all() and stats[:3].tolist() == [0, 0, 0]
    scene.check((-(1 << 23) + 1, -5, 3, 20))                                         # the far corner of the legal offsets
    big = Scene(hip, [square((1 << 23) - 40.5, (1 << 23) - 9.5, (1 << 23) + 5, (1 << 23) + 5)], [0], 1, [4])
    rows, _, _ = big.check(((1 << 23) - 70, (1 << 23) - 12, 70, 12))                 # ... and of the legal far edges
    assert rows[-1, -1] == 0 and rows[0, 0] == -1 and (rows >= 0).sum() == 41 * 10      # the centres ON its left and top edge are in


def test_rotated_and_sheared_transform(hip):
    transform = (0.5, 0.12, 1000.0, -0.08, -0.45, 2000.0)
    to_world = lambda cr: np.stack([transform[0] * cr[:, 0] + transform[1] * cr[:, 1] + transform[2],  # noqa: E731
                                    transform[3] * cr[:, 0] + transform[4] * cr[:, 1] + transform[5]], axis=1)
    rings = [to_world(square(-5, -5, 60, 40)), to_world(np.array([(10.0, 1.0), (45.0, 16.0), (20.0, 31.0), (2.0, 12.0)])),
             to_world(square(3.3, 4.1, 30.2, 25.7))]
    rows, _, stats = Scene(hip, rings, [0, 1, 2], 3, [5, 6, 7], transform=transform).check((0, 0, 47, 33))
    assert (rows >= 0).all() and stats[2] == 47 * 33 and (rows == 2).sum() > 0


def test_rings_at_the_chunk_edges(hip):
    """256, 257, 300 and 777 vertices: one LDS chunk exactly, one more, and more than three chunks."""
    rings = []
    for n, r0 in ((300, 12.0), (777, 18.0), (256, 6.0), (257, 9.0)):
        angle = np.linspace(0, 2 * np.pi, n, endpoint=False)
        radius = r0 * (0.6 + 0.4 * np.cos(7 * angle) ** 2)
        rings.append(np.stack([20.2 + radius * np.cos(angle), 19.7 + radius * np.sin(angle)], axis=1))
    _, _, stats = Scene(hip, rings, [0, 1, 2, 3], 4, [1, 2, 3, 4]).check((0, 0, 40, 40))
    assert stats[3] == 777


def test_star_polygons_overlap_heavily(hip):
    """200 seeded star-shaped polygons of 3-40 vertices over 97 x 131: many cells lie in several rows, the highest stays (B3)."""
    rng = np.random.default_rng(10)
    rings = []
    for _ in range(200):
        n = int(rng.integers(3, 41))
        angle = np.sort(rng.uniform(0, 2 * np.pi, n))
        radius = rng.uniform(2.0, 11.0) * rng.uniform(0.4, 1.0, n)
        centre = rng.uniform((-3, -3), (134, 100))
        rings.append(centre + np.stack([radius * np.cos(angle), radius * np.sin(angle)], axis=1))
    scene = Scene(hip, rings, list(range(200)), 200, np.arange(200) % 251)
    rows, out, stats = scene.check((0, 0, 131, 97))
    assert stats[1] > stats[2] > 0, "more than one row meets in some cell"
    assert np.array_equal(out[rows >= 0], rows[rows >= 0] % 251)
    # launch order: the same items reversed and shuffled
    items = burn_work_items(scene.boxes, scene.ranges, (0, 0, 131, 97))
    for order in (np.arange(len(items))[::-1], rng.permutation(len(items))):
        again = scene.burner.window(0, 0, 131, 97, np.ascontiguousarray(items[order]))
        assert np.array_equal(again[0].cpu().numpy(), rows) and np.array_equal(again[1].cpu().numpy(), out)


def test_block_shapes_change_neither_plane(hip):
    angle = np.linspace(0, 2 * np.pi, 90, endpoint=False)
    rings = [np.stack([35 + 33 * np.cos(angle) * (0.7 + 0.3 * np.sin(5 * angle)), 75 + 72 * np.sin(angle)], axis=1), square(10.5, 3, 69, 149.5)]
    scene = Scene(hip, rings, [0, 1], 2, [3, 4])
    base = scene.device((0, 0, 70, 150))
    for block in ((64, 128), (7, 3), (1, 1), (64, 1)):
        other = scene.device((0, 0, 70, 150), block=block)
        assert np.array_equal(other[0], base[0]) and np.array_equal(other[1], base[1]) and np.array_equal(other[2][1:], base[2][1:])
    scene.check((0, 0, 70, 150), block=(33, 128))


def test_rows_alone(hip):
    scene = shapes_scene(hip, 65, 257)
    rows, out, stats = scene.check((0, 0, 257, 65), want_values=False)
    assert out is None and stats[2] == 0 and stats[1] > 0
    without = Scene(hip, scene.rings, [0, 1, 2], 3, None)                              # a burner made without values
    assert np.array_equal(without.check((0, 0, 257, 65), want_values=False)[0], rows)
    with pytest.raises(ValueError, match="gr_burn_polygons: this burner was made without values"):
        without.device((0, 0, 257, 65))


def test_one_burner_many_windows(hip):
    """The tiles of a 2 x 3 split of a window, burned one by one through ONE burner, reassemble to the single-window result."""
    scene = shapes_scene(hip, 65, 257)
    whole = scene.check((-3, -2, 263, 70))
    cols, rows = [-3, 85, 171, 260], [-2, 30, 68]
    planes = [np.full((70, 263), 99, np.int32), np.full((70, 263), 99, np.uint8)]
    burned = 0
    for r0, r1 in zip(rows[:-1], rows[1:]):
        for c0, c1 in zip(cols[:-1], cols[1:]):
            tile = scene.device((c0, r0, c1 - c0, r1 - r0))
            planes[0][r0 + 2:r1 + 2, c0 + 3:c1 + 3], planes[1][r0 + 2:r1 + 2, c0 + 3:c1 + 3] = tile[0], tile[1]
            burned += tile[2][2]
    assert np.array_equal(planes[0], whole[0]) and np.array_equal(planes[1], whole[1]) and burned == whole[2][2]


def test_burn_and_count_agree(hip):
    """The jittered quadrilaterals that tile a raster (tests/test_zonal_counts_gpu.py), with a shared vertex on a cell centre and a
    shared edge through centres: burned with values p % 7 and counted with the zonal call, every row's count lies in the column of
    its own value, and every cell is burned.  Needs no stand-in: the two calls share Z3."""
    rng = np.random.default_rng(12)
    H, W, step = 53, 71, 6
    xs, ys = np.arange(-step, W + 2 * step, step), np.arange(-step, H + 2 * step, step)
    gx, gy = np.meshgrid(xs.astype(np.float64), ys.astype(np.float64))
    jitter = rng.uniform(-2.4, 2.4, gx.shape + (2,))
    jitter[[0, -1], :, :] = 0
    jitter[:, [0, -1], :] = 0
    vx, vy = np.rint((gx + jitter[..., 0]) * 65536) / 65536, np.rint((gy + jitter[..., 1]) * 65536) / 65536   # exact in float64
    vx[3, 3], vy[3, 3] = 12.5, 12.5                   # a shared vertex exactly on a cell centre
    vx[5, 4:6], vy[5, 4], vy[5, 5] = (18.0, 24.0), 24.5, 24.5      # a horizontal shared edge through cell centres
    rings = [np.array([(vx[j, i], vy[j, i]), (vx[j, i + 1], vy[j, i + 1]), (vx[j + 1, i + 1], vy[j + 1, i + 1]), (vx[j + 1, i], vy[j + 1, i])])
             for j in range(len(ys) - 1) for i in range(len(xs) - 1)]
    P = len(rings)
    values = (np.arange(P) % 7).astype(np.uint8)
    scene = Scene(hip, rings, list(range(P)), P, values)
    rows, burned, stats, _ = scene.device((0, 0, W, H))
    assert stats[_hip.GR_BURN_STAT_BURNED] == H * W == stats[_hip.GR_BURN_STAT_INSIDE] and (rows >= 0).all()
    items = zonal_work_items(scene.rv, scene.off, scene.rp, P, H, W)
    counts, zonal_stats = hip.zonal_class_counts(burned, None, scene.rv, scene.off, scene.rp, P, items, 7)
    counts = counts.cpu().numpy()
    assert counts.sum() == H * W and zonal_stats.cpu().numpy()[1] == H * W
    own = np.zeros_like(counts)
    own[np.arange(P), values] = counts[np.arange(P), values]
    assert np.array_equal(counts, own), "a row counted a cell that was burned with another row's value"
    assert np.array_equal(counts[np.arange(P), values], np.bincount(rows.reshape(-1), minlength=P))
    scene.check((0, 0, W, H))


@pytest.fixture(scope="module")
def ctx():
    from fenced_backend import FencedHipRaster

    backend = FencedHipRaster(0)
    yield backend
    backend.close()


@pytest.mark.parametrize("size", [1, 65, 257])
def test_fenced_outputs(ctx, size):
    """Both planes and the statistics block behind fences, poisoned: every byte written, none beside them, the inputs untouched."""
    import torch
    from fenced_backend import POISON, fenced

    scene = shapes_scene(ctx, size, size)
    assert max(scene.values) < POISON
    inputs = [scene.burner._rv, scene.burner._off, scene.burner._rp, scene.burner._values]
    clones = [t.clone() for t in inputs]
    items = torch.as_tensor(burn_work_items(scene.boxes, scene.ranges, (0, 0, size, size))).to(ctx.device)
    items_clone = items.clone()
    want_rows, want_out, want_stats = bs.burn(scene.rings_q, scene.ring_rows, 3, (0, 0, size, size), scene.values, 255)
    with fenced(ctx):
        rows, out, stats = scene.burner.window(0, 0, size, size, items, fill=255)
        only_rows = scene.burner.window(0, 0, size, size, items, fill=255, want_values=False)
    assert len(ctx.fences.live) == 0
    rows, out, stats = rows.cpu().numpy(), out.cpu().numpy(), stats.cpu().numpy()
    assert not (out == POISON).any() and not (rows == 0x7F7F7F7F).any() and not (stats == 0x7F7F7F7F7F7F7F7F).any()
    want_stats[0] = int((items_clone.cpu().numpy()[:, 3].astype(np.int64) * items_clone.cpu().numpy()[:, 4]).sum())
    assert np.array_equal(rows, want_rows) and np.array_equal(out, want_out) and np.array_equal(stats, want_stats)
    assert only_rows[1] is None and np.array_equal(only_rows[0].cpu().numpy(), want_rows)
    for t, clone in zip(inputs + [items], clones + [items_clone]):
        assert torch.equal(t, clone), "a device input was written"


def test_malformed_tables_are_refused_before_the_device(hip):
    rv, off = rings_to_cell_units([square(1, 1, 8, 8)], IDENTITY)
    burner = hip.polygon_burner(rv, off, [0], 1, [5])
    good = np.array([[0, 1, 1, 7, 7, 0, 1]], dtype=np.int32)
    assert burner.window(0, 0, 10, 10, good)[1].cpu().numpy()[1:8, 1:8].tolist() == [[5] * 7] * 7
    for bad in ([[0, 0, 0, 65, 1, 0, 1]], [[0, 8, 0, 3, 1, 0, 1]], [[1, 0, 0, 1, 1, 0, 1]], [[0, 0, 0, 1, 1, 0, 2]], [[0, 0, 9, 1, 2, 0, 1]], [[0, -1, 0, 1, 1, 0, 1]]):
        with pytest.raises(ValueError, match="gr_burn_polygons: work item 0"):
            burner.window(0, 0, 10, 10, np.array(bad, dtype=np.int32))
    for window in ((0, 0, 0, 10), (0, 0, 10, 0), (1 << 23, 0, 1, 1), ((1 << 23) - 5, 0, 6, 1), (0, -(1 << 23), 1, 1)):
        with pytest.raises(ValueError, match="gr_burn_polygons: a window"):
            burner.window(*window, good[:0])
    with pytest.raises(ValueError, match="gr_burn_polygons: fill=300"):
        burner.window(0, 0, 10, 10, good, fill=300)
    with pytest.raises(ValueError, match="gr_burn_polygons"):
        hip.polygon_burner(rv * (1 << 30), off, [0], 1, [5])
    with pytest.raises(ValueError, match="gr_burn_polygons"):
        hip.polygon_burner(rv, off, [0], 1, [256])
    with pytest.raises(ValueError, match="gr_burn_polygons"):
        hip.polygon_burner(rv, off, [1], 1, [5])
    with pytest.raises(ValueError, match="gr_burn_polygons"):
        hip.polygon_burner(rv.astype(np.float64), off, [0], 1, [5])


def test_the_kernel_skips_an_item_that_leaves_the_window(ctx):
    """B7 behind the host's back (`_call`): an item outside the window, one too large and one of an unknown row write nothing --
    the planes are those of the good items alone, and the fences around them hold."""
    import torch
    from fenced_backend import fenced

    rv, off = rings_to_cell_units([square(-50, -50, 50, 50)], IDENTITY)
    burner = ctx.polygon_burner(rv, off, [0], 1, [5])
    items = np.array([[0, 2, 2, 3, 3, 0, 1], [0, 8, 0, 3, 1, 0, 1], [0, -1, 4, 2, 1, 0, 1], [0, 0, 9, 1, 2, 0, 1], [0, 0, -1, 1, 1, 0, 1],
                      [0, 0, 0, 65, 1, 0, 1], [0, 0, 0, 1, 129, 0, 1], [1, 0, 0, 1, 1, 0, 1], [-1, 0, 0, 1, 1, 0, 1], [0, 0, 0, 0, 1, 0, 1],
                      [0, 9, 9, 1, 1, -7, 99]], dtype=np.int32)
    it_t = ctx._dev(items, torch.int32)
    with fenced(ctx):
        rows, out, stats = ctx._empty((10, 10), torch.int32), ctx._empty((10, 10), torch.uint8), ctx._stats(_hip.GR_BURN_STAT_WORDS)
        ctx._call("gr_burn_polygons", burner._rv.data_ptr(), 4, burner._off.data_ptr(), burner._rp.data_ptr(), 1, 1, burner._values.data_ptr(),
                  it_t.data_ptr(), len(items), 0, 0, 10, 10, 255, rows.data_ptr(), out.data_ptr(), stats.data_ptr(), ctx._stream())
    want = np.full((10, 10), -1, np.int32)
    want[2:5, 2:5] = 0
    want[9, 9] = 0                                   # its ring range is clamped to the rings there are
    assert np.array_equal(rows.cpu().numpy(), want) and np.array_equal(out.cpu().numpy(), np.where(want == 0, 5, 255))
    assert stats.cpu().numpy()[:5].tolist() == [10, 10, 10, 4, 0]


def test_the_library_refuses_bad_arguments_before_any_device_work(hip):
    """GR_EINVAL from the library itself, with a context: the binding's host checks are bypassed (`_rc`)."""
    import torch

    stats = hip._stats(_hip.GR_BURN_STAT_WORDS, zeroed=True)
    buf = hip._zeros((64,), torch.int64)
    p, s = buf.data_ptr(), stats.data_ptr()

    def call(**kw):
        a = dict(rv=p, n_rv=0, roff=p, rpoly=p, R=0, P=1, values=p, items=p, n_items=0, col_off=0, row_off=0, width=2, height=2, fill=255,
                 rows=p, out=p + 256, stats=s)
        a.update(kw)
        return hip._rc("gr_burn_polygons", *a.values(), hip._stream())

    assert call() == _hip.GR_OK and stats.cpu().tolist() == [0] * 8
    assert buf.cpu().view(torch.int32)[:4].tolist() == [-1] * 4 and buf.cpu().view(torch.uint8)[256:260].tolist() == [255] * 4
    assert call(out=None, values=None) == _hip.GR_OK and call(P=0, values=None) == _hip.GR_OK
    for kw in (dict(width=0), dict(height=0), dict(width=-1), dict(col_off=1 << 23), dict(col_off=-(1 << 23)), dict(row_off=1 << 23),
               dict(row_off=-(1 << 23)), dict(col_off=(1 << 23) - 1, width=2), dict(row_off=(1 << 23) - 1, height=2), dict(fill=-1), dict(fill=256),
               dict(R=-1), dict(P=-1), dict(n_items=-1), dict(n_rv=-1), dict(P=1 << 31), dict(rows=None), dict(stats=None), dict(roff=None),
               dict(R=1, rpoly=None), dict(n_rv=3, rv=None), dict(n_items=1, items=None), dict(values=None)):
        assert call(**kw) == _hip.GR_EINVAL, kw
    with pytest.raises(ValueError, match="gr_burn_polygons: fill=256 outside"):
        hip._check(call(fill=256), "gr_burn_polygons")
