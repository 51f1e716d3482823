"""gr_polygon_box_pairs_count / _fill and gr_polygon_overlap_areas on the device against tests/overlap_standin.py (rules A1-A9 of
DESIGN.md 8o; the stand-ins are pinned to hand-worked cases and to an independent exact clip by tests/test_polygon_overlap_host.py).
Every candidate pair of every scene is compared with the exact stand-in and held to the bound of A6, K 2^-53 area_abs with the K
that the host test measures; the pair list and every statistics word are compared with np.array_equal.  The scenes satisfy the
condition that every candidate pair has an exact area of 0 or of at least 1e-6 m^2 (asserted), so no dropped-or-kept decision of
the host layers sits near a bound."""
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import overlap_standin as ov  # noqa: E402
from geograypher_amd import _hip  # noqa: E402
from geograypher_amd.utils import geospatial as gs  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons, overlap_work_items, snap_polygon_pair  # noqa: E402

pytestmark = pytest.mark.gpu
POISON_F64 = np.frombuffer(b"\x7f" * 8, dtype=np.float64)[0]


def run(hip, table_a, table_b, pairs=None, tile=None):
    """(the device's pair list, area, area_abs, stats, items) -- over the device's own pairs unless others are given."""
    overlap = hip.polygon_overlap(table_a, table_b)
    listed = overlap.pairs().cpu().numpy()
    use = listed if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32)
    items = overlap_work_items(table_a[1], table_a[2], table_b[1], table_b[2], use, *(() if tile is None else (tile,)))
    area, area_abs, stats = overlap.areas(use, items)
    return listed, area.cpu().numpy(), area_abs.cpu().numpy(), stats.cpu().numpy(), items


def ratios(area, area_abs, exact):
    """|device - exact| / (2^-53 area_abs) per pair, in exact arithmetic; 0 where everything is 0."""
    out = np.zeros(len(area))
    for k in range(len(area)):
        error = abs(Fraction(float(area[k])) - Fraction(exact[k], 1 << ov.FIXED_BITS))
        if area_abs[k] == 0:
            assert error == 0
            continue
        out[k] = float(error / (Fraction(float(area_abs[k])) / (1 << 53)))
    return out


def check_scene(hip, name, shifted, tile=None):
    table_a, table_b, pairs = ov.scene_tables(name, shifted)
    assert ov.far_from_every_bound(name, shifted)
    exact, exact_abs, want_stats = ov.scene_exact(name, shifted)
    listed, area, area_abs, stats, items = run(hip, table_a, table_b, tile=tile)
    assert listed.dtype == np.int32 and np.array_equal(listed, pairs)
    r = ratios(area, area_abs, exact)
    assert np.all(r <= ov.OVERLAP_BOUND_K), (name, shifted, float(r.max()), pairs[int(r.argmax())])
    for k in range(len(pairs)):      # area_abs itself: a sum of non-negative terms, each a few ulp off
        assert abs(Fraction(float(area_abs[k])) - Fraction(exact_abs[k], 1 << ov.FIXED_BITS)) <= Fraction(float(gs.overlap_bound(area_abs[k])))
    want_stats = want_stats.copy()
    want_stats[_hip.GR_OVERLAP_STAT_ITEMS] = len(items)
    assert np.array_equal(stats, want_stats), (stats, want_stats)
    return float(r.max()) if len(r) else 0.0, area, area_abs


@pytest.mark.parametrize("shifted", [False, True])
def test_hand_worked_cases(hip, shifted):
    for k, (name, _a, _b, want, n_pairs) in enumerate(ov.HAND_CASES):
        _, area, area_abs = check_scene(hip, f"hand {k}", shifted)
        assert len(area) == n_pairs, name
        if n_pairs and want is not None:
            assert abs(area[0] * gs.GRID_STEP_AREA - want) <= gs.overlap_bound(area_abs[0]) * gs.GRID_STEP_AREA, name
            assert (area[0] > gs.overlap_bound(area_abs[0])) == (want > 0), name


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("name", ["edges", "rings", "parts", "stars", "tiling"])
def test_scenes_within_the_bound(hip, name, shifted):
    """edges: rows of 255, 256, 257, 513 edges on the LDS side against 255, 256, 257 and 4097 on the lane side; rings: rings of 300 and
    777 vertices in two-part rows; parts: a multi-part row with two holes; stars: 200 seeded stars against 200 others; tiling: 50
    stars against the quadrilaterals that tile the plane."""
    r, _, _ = check_scene(hip, name, shifted)
    print(f"[polygon_overlap] scene {name} shifted={shifted}: largest device ratio {r:.3f} of K = {ov.OVERLAP_BOUND_K}")


def test_transposed_tables_give_the_transposed_answer(hip):
    table_a, table_b, pairs = ov.scene_tables("stars")
    exact, _, _ = ov.scene_exact("stars")
    listed, area, area_abs, _, _ = run(hip, table_b, table_a)
    order = np.lexsort((listed[:, 0], listed[:, 1]))
    assert np.array_equal(listed[order][:, ::-1], pairs)
    assert np.all(ratios(area[order], area_abs[order], exact) <= ov.OVERLAP_BOUND_K)
    # rows of 513 and 4097 edges change sides: 4097 slots on the LDS side are 17 a-tiles
    table_a, table_b, pairs = ov.scene_tables("edges")
    listed, area, area_abs, _, items = run(hip, table_b, table_a)
    order = np.lexsort((listed[:, 0], listed[:, 1]))
    assert np.array_equal(listed[order][:, ::-1], pairs) and len(items) > len(pairs)
    assert np.all(ratios(area[order], area_abs[order], ov.scene_exact("edges")[0]) <= ov.OVERLAP_BOUND_K)


@pytest.mark.parametrize("name,tile", [("parts", (8, 16)), ("parts", (1, 1)), ("parts", (256, 1)), ("parts", (3, 4096)), ("rings", (100, 333)),
                                       ("rings", (256, 64)), ("edges", (255, 4095))])
def test_other_tile_shapes_change_nothing_beyond_the_bounds(hip, name, tile):
    check_scene(hip, name, False, tile=tile)


def test_pair_order_and_repeats_are_bit_equal(hip):
    """A7: reversed and shuffled pair lists give the same bits per pair, and so do two runs."""
    table_a, table_b, pairs = ov.scene_tables("stars")
    _, area, area_abs, stats, _ = run(hip, table_a, table_b)
    again = run(hip, table_a, table_b)
    assert np.array_equal(again[1], area) and np.array_equal(again[2], area_abs) and np.array_equal(again[3], stats)
    rng = np.random.default_rng(7)
    for order in (np.arange(len(pairs))[::-1], rng.permutation(len(pairs))):
        _, a2, abs2, stats2, _ = run(hip, table_a, table_b, pairs=pairs[order])
        assert np.array_equal(a2, area[order]) and np.array_equal(abs2, area_abs[order]) and np.array_equal(stats2, stats)
    # a pair whose items stand elsewhere in the launch, among other tiles: the "rings" pair alone and behind the "parts" rows
    ta, tb, pr = ov.scene_tables("rings")
    alone = run(hip, ta, tb, tile=(100, 333))
    doubled = run(hip, ta, tb, pairs=np.concatenate([pr, pr]), tile=(100, 333))
    assert np.array_equal(doubled[1], np.concatenate([alone[1], alone[1]])) and np.array_equal(doubled[2], np.concatenate([alone[2], alone[2]]))


def test_quadrilaterals_that_tile_the_plane_partition_every_star(hip):
    """Needs no stand-in: the row sum of a star over the tiling equals the star's own area, within the summed bounds."""
    table_a, table_b, pairs = ov.scene_tables("tiling", shifted=True)
    listed, area, area_abs, _, _ = run(hip, table_a, table_b)
    rv, off, rp, _, _ = table_a
    for row in range(len(table_a[4])):
        ring = [(int(x), int(y)) for x, y in rv[off[row]:off[row + 1]]]
        own = Fraction(sum(ring[k - 1][0] * ring[k][1] - ring[k][0] * ring[k - 1][1] for k in range(len(ring))), 2)
        mine = listed[:, 0] == row
        total = sum((Fraction(float(v)) for v in area[mine]), Fraction(0))
        bound = sum((Fraction(float(v)) for v in gs.overlap_bound(area_abs[mine])), Fraction(0))
        assert own > 0 and abs(total - own) <= bound, row


def test_triangles_against_the_clipped_overlay_of_label_polygons(hip):
    """Two independent device kernels: triangles as one-ring rows against crown polygons here, and the same triangles as the faces of
    a flat mesh through `label_polygon_weights(sjoin_overlay=False)` (gr_polygon_class_weights, GR_POLY_OVERLAY: Sutherland-Hodgman
    in float64; a flat face weighs 1) against the same crowns, within that kernel's tolerance (1e-12 of the value,
    tests/test_label_polygons_gpu.py) and this one's bound."""
    from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh

    rng = np.random.default_rng(9)
    crowns = ov.polygons_of(ov.star_rows(41, 40, extent=(60.0, 60.0)))
    gx, gy = np.meshgrid(np.arange(-12.0, 75.0, 6.0), np.arange(-12.0, 75.0, 6.0))
    n = gx.shape[1]
    points = np.stack([gx + rng.uniform(-2, 2, gx.shape), gy + rng.uniform(-2, 2, gy.shape), np.zeros(gx.shape)], axis=-1).reshape(-1, 3)
    corner = np.array([j * n + i for j in range(gx.shape[0] - 1) for i in range(n - 1)])
    mesh_faces = np.concatenate([np.stack([corner, corner + 1, corner + n + 1], axis=1), np.stack([corner, corner + n + 1, corner + n], axis=1)])
    faces = PlanarPolygons([points[f, :2] for f in mesh_faces], list(range(len(mesh_faces))), [False] * len(mesh_faces))
    table_f, table_c, _ = snap_polygon_pair(faces, crowns)
    listed, area, area_abs, _, _ = run(hip, table_f, table_c)
    mine = np.zeros(len(crowns))
    np.add.at(mine, listed[:, 1], area * gs.GRID_STEP_AREA)                    # that kernel answers in m^2
    bound = np.zeros(len(crowns))
    np.add.at(bound, listed[:, 1], gs.overlap_bound(area_abs) * gs.GRID_STEP_AREA)
    mesh = TexturedPhotogrammetryMesh((points, mesh_faces.astype(np.int32)), log_level="ERROR")
    theirs = mesh.label_polygon_weights(np.zeros(len(mesh_faces)), crowns, sjoin_overlay=False, points_in_polygon_CRS=points)[:, 0]
    assert np.all(theirs > 0) and np.all(np.abs(mine - theirs) <= 1e-12 * theirs + bound), np.abs(mine - theirs).max()


def test_empty_tables_and_rows_without_rings(hip):
    none = PlanarPolygons([], [], [], n_polygons=0)
    bare = PlanarPolygons([], [], [], n_polygons=3)                                   # rows without rings: the empty box
    some = ov.polygons_of([[ov.square(0, 0, 2, 2)], [ov.square(5, 5, 6, 6)]])
    mixed = PlanarPolygons([np.array(ov.square(1, 1, 3, 3), dtype=float)], [2], [False], n_polygons=4)
    for A, B, n_pairs in ((none, none, 0), (none, some, 0), (some, none, 0), (bare, some, 0), (some, bare, 0), (some, some, 2), (some, mixed, 1)):
        table_a, table_b, _ = snap_polygon_pair(A, B)
        listed, area, area_abs, stats, items = run(hip, table_a, table_b)
        assert listed.shape == (n_pairs, 2) and area.shape == (n_pairs,) and stats[0] == n_pairs and stats[6] == 0
    assert listed.tolist() == [[0, 2]] and area[0] == 1e12
    # pairs without an item: zeros, every word written
    table_a, table_b, _ = snap_polygon_pair(some, some)
    overlap = hip.polygon_overlap(table_a, table_b)
    area, area_abs, stats = overlap.areas(np.array([[0, 0], [1, 1], [0, 1]], dtype=np.int32), np.zeros((0, 5), dtype=np.int32))
    assert area.cpu().tolist() == [0, 0, 0] and area_abs.cpu().tolist() == [0, 0, 0] and stats.cpu().tolist() == [3, 0, 0, 8, 0, 4, 0, 0]


@pytest.fixture(scope="module")
def ctx():
    from fenced_backend import FencedHipRaster

    backend = FencedHipRaster(0)
    yield backend
    backend.close()


@pytest.mark.parametrize("size", [1, 65, 257])
def test_fenced_outputs(ctx, size):
    """The offsets, the pair list, both areas and the statistics block behind fences, poisoned: every byte written, none beside them,
    the inputs untouched."""
    import torch
    from fenced_backend import fenced

    side = 6.0 * size ** 0.5
    table_a, table_b, _ = snap_polygon_pair(ov.polygons_of(ov.star_rows(50 + size, size, extent=(side, side))),
                                            ov.polygons_of(ov.star_rows(60 + size, size, extent=(side, side))))
    pairs = ov.box_pairs(table_a, table_b)
    assert len(pairs) >= size
    overlap = ctx.polygon_overlap(table_a, table_b)
    inputs = [t for t in overlap._a[:5] + overlap._b[:5]]
    clones = [t.clone() for t in inputs]
    items = torch.as_tensor(overlap_work_items(table_a[1], table_a[2], table_b[1], table_b[2], pairs)).to(ctx.device)
    items_clone = items.clone()
    with fenced(ctx):
        listed = overlap.pairs()
        area, area_abs, stats = overlap.areas(listed, items)
    assert len(ctx.fences.live) == 0
    listed, area, area_abs, stats = listed.cpu().numpy(), area.cpu().numpy(), area_abs.cpu().numpy(), stats.cpu().numpy()
    assert np.array_equal(listed, pairs) and not (area == POISON_F64).any() and not (area_abs == POISON_F64).any()
    assert not (stats == 0x7F7F7F7F7F7F7F7F).any()
    want, want_abs, want_stats = ov.restated_areas(table_a, table_b, pairs, len(items))
    assert np.array_equal(stats, want_stats)
    assert np.all(np.abs(area - want) <= 2 * gs.overlap_bound(want_abs)) and np.all(np.abs(area_abs - want_abs) <= gs.overlap_bound(want_abs))
    for t, clone in zip(inputs + [items], clones + [items_clone]):
        assert torch.equal(t, clone), "a device input was written"


def test_the_kernel_skips_bad_items_whole(ctx):
    """A8 behind the host's back (`_call`): an item that is malformed, names no pair, a pair below one in front of it or a slot outside
    its rows writes nothing and is counted -- the areas are those of the good items alone, bit for bit, and the fences hold."""
    import torch
    from fenced_backend import fenced

    table_a, table_b, pairs = ov.scene_tables("parts")
    assert pairs.tolist() == [[0, 0], [0, 1]]
    overlap = ctx.polygon_overlap(table_a, table_b)
    good = overlap_work_items(table_a[1], table_a[2], table_b[1], table_b[2], pairs, (8, 16))
    n_a, n_b, n_rv_a, n_rv_b = int(table_a[1][np.searchsorted(table_a[2], 0, "right")]), int(table_b[1][np.searchsorted(table_b[2], 0, "right")]), len(table_a[0]), len(table_b[0])
    assert n_a < n_rv_a and n_b < n_rv_b
    first = good[good[:, 0] == 0]
    bad_0 = [[0, 0, 0, 0, 1], [0, 0, 257, 0, 1], [0, 0, 1, 0, 4097], [0, -1, 2, 0, 1], [0, 0, 1, -3, 4], [0, n_rv_a - 1, 2, 0, 1], [0, 0, 1, n_rv_b, 1],
             [0, n_a - 1, 2, 0, 1],        # the second slot belongs to row 1 of a
             [0, 0, 1, n_b - 1, 2],        # ... to row 1 of b
             [-1, 0, 1, 0, 1], [2, 0, 1, 0, 1], [2 ** 31 - 1, 0, 1, 0, 1]]
    late = [[0, 0, 1, 0, 1]]                # a pair below one in front of it
    items = np.concatenate([first, np.array(bad_0, dtype=np.int32), good[good[:, 0] == 1], np.array(late, dtype=np.int32)])
    want = overlap.areas(pairs, good)
    it_t = ctx._dev(items, torch.int32)
    pr_t = ctx._dev(pairs, torch.int32)
    with fenced(ctx):
        area, area_abs, stats = ctx._empty((2,), torch.float64), ctx._empty((2,), torch.float64), ctx._stats(_hip.GR_OVERLAP_STAT_WORDS)
        ctx._call("gr_polygon_overlap_areas", *overlap._table_args(overlap._a), *overlap._table_args(overlap._b), pr_t.data_ptr(), 2, it_t.data_ptr(),
                  len(items), area.data_ptr(), area_abs.data_ptr(), stats.data_ptr(), ctx._stream())
    assert torch.equal(area, want[0]) and torch.equal(area_abs, want[1])
    want_stats = want[2].cpu().numpy().copy()
    want_stats[_hip.GR_OVERLAP_STAT_BAD_ITEMS] = len(bad_0) + len(late)
    assert np.array_equal(stats.cpu().numpy(), want_stats) and want_stats[_hip.GR_OVERLAP_STAT_ITEMS] == len(good)
    with pytest.raises(ValueError, match="gr_polygon_overlap_areas: work item"):
        overlap.areas(pairs, items)


def test_the_library_refuses_bad_arguments_before_any_device_work(hip):
    """GR_EINVAL from the library itself, with a context: the binding's host checks are bypassed (`_rc`)."""
    import torch

    stats = hip._stats(_hip.GR_OVERLAP_STAT_WORDS, zeroed=True)
    buf = hip._zeros((64,), torch.int64)
    p, s = buf.data_ptr(), stats.data_ptr()

    def table(side, **kw):
        t = dict(rv=p, n_rv=0, roff=p, rpoly=p, rhole=p, R=0, pbox=p, P=0)
        t.update({k[:-2]: v for k, v in kw.items() if k.endswith("_" + side)})
        return list(t.values())

    def areas(**kw):
        a = dict(pairs=p, n_pairs=0, items=p, n_items=0, area=p, area_abs=p, stats=s)
        a.update({k: v for k, v in kw.items() if k in a})
        return hip._rc("gr_polygon_overlap_areas", *table("a", **kw), *table("b", **kw), *a.values(), hip._stream())

    assert areas() == _hip.GR_OK and stats.cpu().tolist() == [0] * 8
    assert areas(pairs=None, items=None, area=None, area_abs=None, rv_a=None, rpoly_b=None, rhole_b=None, pbox_a=None) == _hip.GR_OK
    for kw in (dict(n_rv_a=-1), dict(R_a=-1), dict(P_b=-1), dict(n_rv_b=1 << 31), dict(R_b=1 << 31), dict(P_a=1 << 31), dict(roff_a=None), dict(roff_b=None),
               dict(n_rv_a=3, rv_a=None), dict(R_b=1, rpoly_b=None), dict(R_a=1, rhole_a=None), dict(P_b=1, pbox_b=None), dict(n_pairs=-1),
               dict(n_items=-1), dict(n_pairs=1 << 31), dict(n_items=1 << 31), dict(stats=None), dict(n_pairs=1, pairs=None), dict(n_pairs=1, area=None),
               dict(n_pairs=1, area_abs=None), dict(n_items=1, items=None)):
        assert areas(**kw) == _hip.GR_EINVAL, kw

    def count(**kw):
        a = dict(boxes_a=p, Pa=0, boxes_b=p, Pb=0, offsets=p)
        a.update(kw)
        return hip._rc("gr_polygon_box_pairs_count", *a.values(), hip._stream())

    def fill(**kw):
        a = dict(boxes_a=p, Pa=0, boxes_b=p, Pb=0, offsets=p, pairs=p, n_pairs=0)
        a.update(kw)
        return hip._rc("gr_polygon_box_pairs_fill", *a.values(), hip._stream())

    assert count() == _hip.GR_OK and fill() == _hip.GR_OK and fill(pairs=None) == _hip.GR_OK and count(boxes_a=None, boxes_b=None) == _hip.GR_OK
    for kw in (dict(Pa=-1), dict(Pb=-1), dict(Pa=(1 << 31) - 1), dict(Pb=1 << 31), dict(Pa=1, boxes_a=None), dict(Pb=1, boxes_b=None), dict(offsets=None)):
        assert count(**kw) == _hip.GR_EINVAL and fill(**kw) == _hip.GR_EINVAL, kw
    for kw in (dict(n_pairs=-1), dict(n_pairs=1 << 31), dict(n_pairs=1, pairs=None)):
        assert fill(**kw) == _hip.GR_EINVAL, kw
    with pytest.raises(ValueError, match="gr_polygon_overlap_areas: n_pairs=-1"):
        hip._check(areas(n_pairs=-1), "gr_polygon_overlap_areas")
