"""gr_zonal_class_counts on the device against tests/zonal_standin.py (rules Z1-Z7 of DESIGN.md 8m; the stand-in works in Python
integers and is pinned to hand-worked cases by tests/test_ortho_baseline_host.py).  All integer: every comparison is
np.array_equal -- counts and the statistics words.  Word 0, the cells tested, is the cells of the work items."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import zonal_standin as zs  # noqa: E402
from geograypher_amd.utils.geometric import zonal_work_items  # noqa: E402
from geograypher_amd.utils.geospatial import rings_to_cell_units  # noqa: E402
from geograypher_amd.utils.raster import invert_affine  # noqa: E402

pytestmark = pytest.mark.gpu
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def device(hip, raster, nodata, rings, rows, P, C, transform=IDENTITY, block=(64, 16)):
    rv, off = rings_to_cell_units(rings, invert_affine(transform))
    H, W = raster.shape
    items = zonal_work_items(rv, off, rows, P, H, W, block)
    counts, stats = hip.zonal_class_counts(raster, nodata, rv, off, np.asarray(rows, dtype=np.int32), P, items, C)
    return counts.cpu().numpy(), stats.cpu().numpy(), items


def check(hip, raster, nodata, rings, rows, P, C, transform=IDENTITY, block=(64, 16)):
    counts, stats, items = device(hip, raster, nodata, rings, rows, P, C, transform, block)
    want_counts, want_stats = zs.zonal_counts(raster, nodata, zs.to_cell_units(rings, invert_affine(transform)), rows, P, C)
    want_stats[0] = int((items[:, 3].astype(np.int64) * items[:, 4]).sum())
    assert counts.dtype == np.int64 and np.array_equal(counts, want_counts)
    assert np.array_equal(stats, want_stats), (stats, want_stats)
    return counts, stats


def square(x0, y0, x1, y1):
    return np.array([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], dtype=np.float64)


def raster_of(seed, H, W, top=5):
    return np.random.default_rng(seed).integers(0, top, (H, W)).astype(np.uint8)


def test_hand_worked_cases(hip):
    raster = np.arange(16, dtype=np.uint8).reshape(4, 4) % 4      # the value of a cell is its column
    counts, _ = check(hip, raster, None, [square(1, 1, 3, 3)], [0], 1, 4)
    assert counts.tolist() == [[0, 2, 2, 0]]
    # edges through cell centres, and a second square sharing the edge x = 2.5: every centre on it is counted exactly once
    counts, stats = check(hip, raster, None, [square(0.5, 0.5, 2.5, 2.5), square(2.5, 0.5, 3.5, 2.5)], [0, 1], 2, 4)
    assert counts.sum() == 6 and counts[:, 2].sum() == 2 and stats[1] == 6
    # a hole, a two-part row, a ring of two vertices (ignored and counted)
    counts, stats = check(hip, raster, None, [square(0, 0, 4, 4), square(1, 1, 3, 3), square(0, 0, 1, 1), square(3, 3, 4, 4),
                                              np.array([(0.0, 0.0), (4.0, 4.0)])], [0, 0, 1, 1, 1], 2, 4)
    assert counts.tolist() == [[4, 2, 2, 4], [1, 0, 0, 1]] and stats[6] == 1 and stats[5] == 4


@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (70, 1), (65, 257)])
def test_raster_shapes(hip, shape):
    H, W = shape
    raster = raster_of(H * W, H, W)
    rings = [square(-1, -1, W + 1, H + 1), square(0.2 * W, 0.2 * H, 0.75 * W + 0.4, 0.75 * H + 0.4),
             np.array([(0.0, 0.0), (W, 0.3 * H), (0.4 * W, H)])]
    check(hip, raster, None, rings, [0, 1, 2], 3, 5)


def test_rotated_and_sheared_transform(hip):
    raster = raster_of(4, 33, 47)
    transform = (0.5, 0.12, 1000.0, -0.08, -0.45, 2000.0)
    to_world = lambda cr: np.stack([transform[0] * cr[:, 0] + transform[1] * cr[:, 1] + transform[2],  # noqa: E731
                                    transform[3] * cr[:, 0] + transform[4] * cr[:, 1] + transform[5]], axis=1)
    rings = [to_world(square(3.3, 4.1, 30.2, 25.7)), to_world(np.array([(10.0, 1.0), (45.0, 16.0), (20.0, 31.0), (2.0, 12.0)])),
             to_world(square(-5, -5, 60, 40))]
    counts, _ = check(hip, raster, None, rings, [0, 1, 2], 3, 5, transform=transform)
    assert counts[2].sum() == raster.size and counts[0].sum() > 0


def test_rows_outside_partly_outside_and_over_everything(hip):
    raster = raster_of(6, 20, 30)
    rings = [square(100, 100, 120, 130), square(-10, -10, -1, -1), square(-4.5, 5.2, 9.7, 30.0), square(-100, -100, 100, 100)]
    counts, stats = check(hip, raster, None, rings, [0, 1, 2, 3], 5, 5)       # row 4 has no ring at all
    assert counts[0].sum() == 0 and counts[1].sum() == 0 and counts[4].sum() == 0 and 0 < counts[2].sum() < 600
    assert np.array_equal(counts[3], np.bincount(raster.reshape(-1), minlength=5))


def test_nodata_cells_and_values_beyond_the_classes(hip):
    raster = raster_of(8, 25, 25, top=9)
    raster[3:6, 3:9] = 255
    counts, stats = check(hip, raster, 255, [square(0, 0, 25, 25), square(2.5, 2.5, 12.5, 7.5)], [0, 1], 2, 6)
    assert stats[2] == 18 + 18 and stats[3] > 0 and stats[4] == 9 and counts[0].sum() == 625 - 18 - (raster[raster < 255] >= 6).sum()
    check(hip, raster, None, [square(0, 0, 25, 25)], [0], 1, 256)             # 255 is a value like any other
    check(hip, raster, 3, [square(0, 0, 25, 25)], [0], 1, 1)


def test_a_ring_longer_than_one_chunk(hip):
    """300 and 777 vertices: more than the 256 vertices of one LDS chunk, and more than three chunks."""
    raster = raster_of(9, 40, 40)
    rings = []
    for n, r0 in ((300, 12.0), (777, 18.0), (256, 6.0), (257, 9.0)):
        angle = np.linspace(0, 2 * np.pi, n, endpoint=False)
        radius = r0 * (0.6 + 0.4 * np.cos(7 * angle) ** 2)
        rings.append(np.stack([20.2 + radius * np.cos(angle), 19.7 + radius * np.sin(angle)], axis=1))
    _, stats = check(hip, raster, None, rings, [0, 1, 2, 3], 4, 5)
    assert stats[5] == 777


def test_star_polygons(hip):
    """200 seeded star-shaped polygons of 3-40 vertices over a 97 x 131 raster with 5 classes."""
    rng = np.random.default_rng(10)
    raster = raster_of(11, 97, 131)
    rings = []
    for _ in range(200):
        n = int(rng.integers(3, 41))
        angle = np.sort(rng.uniform(0, 2 * np.pi, n))
        radius = rng.uniform(1.0, 9.0) * rng.uniform(0.4, 1.0, n)
        centre = rng.uniform((-3, -3), (134, 100))
        rings.append(centre + np.stack([radius * np.cos(angle), radius * np.sin(angle)], axis=1))
    counts, _ = check(hip, raster, None, rings, list(range(200)), 200, 5)
    assert (counts.sum(axis=1) > 0).sum() > 150


def test_rows_that_tile_the_raster_partition_its_cells(hip):
    """A grid of quadrilaterals with jittered shared vertices, snapped first so that neighbours share exactly equal vertices,
    covering the raster: the summed counts are np.bincount of the raster.  Needs no stand-in."""
    rng = np.random.default_rng(12)
    H, W, step = 53, 71, 6
    raster = raster_of(13, H, W)
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
    counts, stats, _ = device(hip, raster, None, rings, list(range(P)), P, 5)
    assert np.array_equal(counts.sum(axis=0), np.bincount(raster.reshape(-1), minlength=5)) and stats[1] == raster.size
    check(hip, raster, None, rings, list(range(P)), P, 5)


def test_block_shapes_change_nothing(hip):
    raster = raster_of(14, 150, 70)
    angle = np.linspace(0, 2 * np.pi, 90, endpoint=False)
    rings = [np.stack([35 + 33 * np.cos(angle) * (0.7 + 0.3 * np.sin(5 * angle)), 75 + 72 * np.sin(angle)], axis=1), square(10.5, 3, 69, 149.5)]
    base = device(hip, raster, 2, rings, [0, 1], 2, 5)
    for block in ((64, 128), (7, 3), (1, 1), (64, 1)):
        other = device(hip, raster, 2, rings, [0, 1], 2, 5, block=block)
        assert np.array_equal(other[0], base[0]) and np.array_equal(other[1][1:], base[1][1:])
    check(hip, raster, 2, rings, [0, 1], 2, 5, block=(33, 128))


def test_malformed_tables_are_refused_before_the_device(hip):
    raster = raster_of(15, 10, 10)
    rv, off = rings_to_cell_units([square(1, 1, 8, 8)], IDENTITY)
    items = zonal_work_items(rv, off, [0], 1, 10, 10)
    hip.zonal_class_counts(raster, None, rv, off, [0], 1, items, 5)
    for bad in ([[0, 0, 0, 65, 1, 0, 1]], [[0, 8, 0, 3, 1, 0, 1]], [[1, 0, 0, 1, 1, 0, 1]], [[0, 0, 0, 1, 1, 0, 2]], [[0, 0, 9, 1, 2, 0, 1]]):
        with pytest.raises(ValueError, match="gr_zonal_class_counts"):
            hip.zonal_class_counts(raster, None, rv, off, [0], 1, np.array(bad, dtype=np.int32), 5)
    with pytest.raises(ValueError, match="gr_zonal_class_counts"):
        hip.zonal_class_counts(raster, None, rv * (1 << 30), off, [0], 1, items, 5)
    with pytest.raises(ValueError, match="gr_zonal_class_counts"):
        hip.zonal_class_counts(raster.astype(np.float64), None, rv, off, [0], 1, items, 5)
    with pytest.raises(ValueError, match="gr_zonal_class_counts"):
        hip.zonal_class_counts(raster, None, rv, off, [0], 1, items, 257)


def test_the_library_refuses_bad_arguments_before_any_device_work(hip):
    """GR_EINVAL from the library itself, with a context: the binding's host checks are bypassed (`_rc`)."""
    import torch

    from geograypher_amd import _hip

    stats = hip._stats(_hip.GR_ZONAL_STAT_WORDS, zeroed=True)
    buf = hip._zeros((64,), torch.int64)
    p, s = buf.data_ptr(), stats.data_ptr()

    def call(**kw):
        a = dict(raster=p, H=2, W=2, nodata=-1, rv=p, n_rv=0, roff=p, rpoly=p, R=0, P=1, items=p, n_items=0, C=3, counts=p, stats=s)
        a.update(kw)
        return hip._rc("gr_zonal_class_counts", *a.values(), hip._stream())

    assert call() == _hip.GR_OK and stats.cpu().tolist() == [0] * 8
    for kw in (dict(C=0), dict(C=257), dict(H=0), dict(W=1 << 23), dict(R=-1), dict(P=-1), dict(n_items=-1), dict(n_rv=-1), dict(raster=None),
               dict(stats=None), dict(roff=None), dict(counts=None), dict(R=1, rpoly=None), dict(n_rv=3, rv=None), dict(n_items=1, items=None),
               dict(P=1 << 31)):
        assert call(**kw) == _hip.GR_EINVAL, kw
    with pytest.raises(ValueError, match="gr_zonal_class_counts: C=257 outside"):
        hip._check(call(C=257), "gr_zonal_class_counts")
