"""Every stage call on POISONED stage scratch (GR_DBG_POISON_STAGE: 0xFF, GR_DBG_POISON_STAGE_7F: 0x7F; csrc/gr_internal.hpp:
stage_acquire fills the whole block on the call's stream before the stage carves it).  The arena is grow-only and never cleared, so
a stage is right only if it writes every scratch word before it reads it ("Who initialises what"); a fresh block reads
as zeros and the leftovers of the same stage are often the right values, so neither shows a missing initialisation.  Two patterns,
because each is the intended initial value of some array (0xFF: `cl` of the member outlines; 0x7F: `fmin` of the communities) and
hides a missing memset of exactly that array.

One context of its own: the arena stays small and the fills cheap.  Every stage is compared with its own stand-in or oracle as its
own GPU test compares it (the helpers are imported from those tests), under no poison, 0xFF and 0x7F, and the device's answers of the
three runs are bit-equal, floats included.  The hook itself is proven by reading the scratch back (gr_debug_read_stage): a hook that
did nothing would pass everything else here."""
import ctypes
import sys
from contextlib import contextmanager
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))   # the stand-ins import one another by their plain names

import decimate_standin as ds  # noqa: E402
import member_outline_standin as msn  # noqa: E402
import outline_standin as osn  # noqa: E402
import overlap_standin as ov  # noqa: E402
import vector_standin as vs  # noqa: E402
from region_standin import points_in_region_np  # noqa: E402

from geograypher_amd import _hip
from geograypher_amd.utils import numeric, synthetic
from geograypher_amd.utils.geometric import PlanarPolygons, overlap_work_items
from oracle import oracle_resize
from tests import community_standin as cs
from tests import setcover_standin
from tests import upload_standin as su
from tests.covering_standin import points_bounds_np
from tests.image_edge_cases import resize_image_values
from tests.test_communities_gpu import PATHS, points_close, same as same_communities
from tests.test_communities_host import points_bound
from tests.test_detection_footprints_gpu import same as same_members
from tests.test_face_outlines_gpu import same as same_outlines
from tests.test_image_selection_gpu import _assert_same as same_cover, _device as device_cover
from tests.test_image_stage_edges import _close
from tests.test_mesh_decimation_gpu import device_decimate, same_decimation
from tests.test_mesh_upload_gpu import _assert_same_products as same_upload, _read as read_upload
from tests.test_polygon_overlap_gpu import check_scene as check_overlap_scene
from tests.test_roi_crop_gpu import device_region, device_submesh, same_submesh
from tests.test_stage_edges import _index_oracle
from tests.test_stage_scratch_gpu import REGION_D, _check_rays, mesh, rays  # noqa: F401  (mesh, rays: module fixtures, used here too)

pytestmark = pytest.mark.gpu

MODES = {"off": 0, "ff": _hip.GR_DBG_POISON_STAGE, "7f": _hip.GR_DBG_POISON_STAGE_7F}
BYTE = {"ff": 0xFF, "7f": 0x7F}
TAIL = 4096                  # bytes read back from the end of a block
BOUNDS_PLAN = 1024 * 64      # gr_points_bounds carves GR_BOUNDS_MAX_GRID partial records of 64 bytes, nothing else


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


@contextmanager
def poison(ctx, bits):
    ctx.set_option(_hip.GR_OPT_DEBUG, bits)
    try:
        yield
    finally:
        ctx.set_option(_hip.GR_OPT_DEBUG, 0)


@pytest.fixture(scope="module")
def ctx():
    """A context of its own: its arena holds what these tests put there, and is a few megabytes at the most."""
    backend = _hip.HipRaster(0)
    yield backend
    backend.close()


def _upload(ctx, mesh):
    ctx.upload_mesh(mesh["points"].astype(np.float32), mesh["faces"])


# ---- the hook itself ----------------------------------------------------------------------------------------------------------------

def test_the_hook_fills_the_whole_arena_and_only_when_asked(ctx, mesh):
    """Block 0.  A mid-sized call grows the arena (the row pass of a 256 x 256 x 3 resize: 786 432 bytes); gr_points_bounds on 256
    points then plans 65 536 bytes of it.  The last 4096 bytes are far behind that plan: under a poison bit every one of them is the
    pattern (0xFF when both bits are set), with the bits off they stay what they were."""
    image = np.random.default_rng(3).random((256, 256, 3))
    assert ctx.resize_image(image, (64, 64)).shape == (64, 64, 3)
    _, size = ctx.debug_stage(0)
    assert size >= 2 * 64 * 256 * 3 * 8 > 4 * BOUNDS_PLAN
    want_bounds = points_bounds_np(mesh["points"], 1)[0]
    for bits, byte in ((MODES["ff"], 0xFF), (MODES["7f"], 0x7F), (MODES["ff"] | MODES["7f"], 0xFF), (MODES["7f"], 0x7F)):
        with poison(ctx, bits):
            bounds, _ = ctx.points_bounds(mesh["points"])
        tail, size_now = ctx.debug_stage(0, -TAIL, TAIL)
        assert size_now == size and tail.dtype == torch.uint8 and tail.shape == (TAIL,)
        assert bool((tail == byte).all()), (hex(bits), hex(byte), tail.unique().tolist())
        assert np.array_equal(_np(bounds), want_bounds)   # (every fill differs from the one before: none of these bytes is left over)
    bounds, _ = ctx.points_bounds(mesh["points"])   # the bits are off
    tail, _ = ctx.debug_stage(0, -TAIL, TAIL)
    assert bool((tail == 0x7F).all()) and np.array_equal(_np(bounds), want_bounds)
    # the read-back refuses what is not there
    for block, offset, n in ((2, 0, 0), (-1, 0, 0), (0, size, 1), (0, -1 - size, 1), (0, size - 1, 2)):
        with pytest.raises(ValueError, match="gr_debug_read_stage"):
            ctx._call("gr_debug_read_stage", block, offset, n, tail.data_ptr(), ctypes.byref(ctypes.c_int64(0)), ctx._stream())


def test_the_hook_reaches_the_second_block(ctx):
    """Block 1 (stage_b) is acquired through the same function.  An outline call with 10 113 ring vertices (5003 faces, a random class
    each) grows it to 52 bytes a vertex and more; a call with two rings of four vertices then plans eleven arrays of 256 bytes and
    the temporaries of an 8-element sort in it."""
    verts, faces = osn.delaunay_scene(5003, seed=5003)
    grown = ctx.class_outlines(verts, faces, np.random.default_rng(1).integers(0, 3, len(faces)).astype(np.int32), 3)
    assert grown[1].numel() == 10113
    _, size = ctx.debug_stage(1)
    assert size >= 52 * 10113
    small_v, small_f, quad = osn.grid_mesh(2, 1)
    small_c = osn.quad_classes(quad, [0, 1])
    for mode in ("ff", "7f", "ff"):
        with poison(ctx, MODES[mode]):
            want = same_outlines(ctx, small_v, small_f, small_c, 2)
        assert want["n_rings"] == 2
        for block in (0, 1):
            tail, _ = ctx.debug_stage(block, -TAIL, TAIL)
            assert bool((tail == BYTE[mode]).all()), (mode, block, tail.unique().tolist())
    same_outlines(ctx, small_v, small_f, small_c, 2)   # the bits are off
    tail, size_now = ctx.debug_stage(1, -TAIL, TAIL)
    assert size_now == size and bool((tail == 0xFF).all())


# ---- every stage, three ways --------------------------------------------------------------------------------------------------------
# A stage function runs its export on the smallest case that takes every branch that carves scratch, holds the answer against the
# stand-in, and returns the DEVICE's arrays: those of the three modes are compared bit for bit.

def stage_mesh_upload(ctx, d):
    m = d["mesh"]
    verts = m["points"].astype(np.float32)
    ctx.upload_mesh(verts, m["faces"])
    got = read_upload(ctx)
    same_upload(got, d["upload"], d["upload"]["counts"])
    ids = _np(ctx.raster_face_ids(m["recs"], 32, 32))
    assert np.array_equal(ids, m["ids"])
    return [got["orig"], got["blk"], got["bidx"], ids]


def stage_resize_image(ctx, d):
    out = _np(ctx.resize_image(d["image"], (12, 16)))
    _close(out, d["resized"])
    return [out]


def stage_points_bounds(ctx, d):
    bounds, bad = (_np(x) for x in ctx.points_bounds(d["mesh"]["points"]))
    want, want_bad = d["bounds"]
    assert np.array_equal(bounds, want) and int(bad[0]) == want_bad == 0
    return [bounds, bad]


def stage_set_cover(ctx, d):
    A, want = d["cover"]
    got = device_cover(ctx, A, 1, True)
    same_cover(got, want)
    return [got[k] for k in ("selected", "order", "gains", "pruned")]


def stage_count_pairs(ctx, d):
    m = d["mesh"]
    _upload(ctx, m)
    cls, (want_pc, want_keys, want_mult) = d["pairs"]
    pc = torch.zeros((450,), dtype=torch.int32, device=ctx.device)
    keys, mult = ctx.project_index_pairs(m["ids"], cls, 5, pc)
    assert np.array_equal(keys, want_keys) and np.array_equal(mult, want_mult) and np.array_equal(_np(pc), want_pc)
    return [keys, mult, _np(pc)]


def stage_points_in_region(ctx, d):
    table, want_mask, info = d["region"]
    mask, stats = device_region(ctx, d["mesh"]["verts_q"], table, REGION_D)
    assert np.array_equal(mask, want_mask) and np.array_equal(stats, info["stats"])
    return [mask, stats]


def stage_submesh_extract(ctx, d):
    _, want_mask, _ = d["region"]
    got = device_submesh(ctx, want_mask, d["mesh"]["faces"])
    same_submesh(got, want_mask, d["mesh"]["faces"])
    return list(got)


def stage_class_outlines(ctx, d):
    m = d["mesh"]
    want = same_outlines(ctx, m["verts_q"], m["faces"], m["classes"], 3)
    assert want["n_rings"] >= 3
    return [_np(t) for t in ctx.class_outlines(m["verts_q"], m["faces"], m["classes"], 3, check=False)]


def stage_member_outlines(ctx, d):
    """Six faces, three classes each but one face with an empty row: gaps between the rows of the table, three rings.  Then the same
    table with one row descending (Y2): the call ends at the bad-rows word, behind the edge kernel alone."""
    verts, faces, rows = d["members"]
    want = same_members(ctx, verts, faces, rows, 3)
    assert want["n_rings"] == 3 and want["n_edges"] == 27
    out = [_np(t) for t in ctx.member_outlines(verts, faces, *msn.csr_of_rows(rows), 3, check=False)]
    face_ptr, members = msn.csr_of_rows(rows)
    members = members.copy()
    members[face_ptr[1]:face_ptr[1] + 3] = [2, 1, 0]
    assert msn.bad_ptr(face_ptr, len(members), 6) == 0 and msn.bad_rows(face_ptr, members, 6) == 2
    canon, rv, ro, rc, st = ctx.member_outlines(verts, faces, face_ptr, members, 3, check=False)
    assert rv.numel() == 0 and rc.numel() == 0 and _np(ro).tolist() == [0] and int(st[_hip.GR_OUTL_STAT_BAD_ROWS]) == 2
    return out + [_np(st)]


def stage_cluster_count(ctx, d):
    verts_q, _, s = d["decimate"]
    counts = [ctx.cluster_count(verts_q, s), ctx.cluster_count(verts_q, 2 * s), ctx.cluster_count(verts_q, 1)]
    assert counts == [ds.cluster_count_py(verts_q, s), ds.cluster_count_py(verts_q, 2 * s), ds.cluster_count_py(verts_q, 1)]
    assert counts[:2] == [4, 1]
    return [np.array(counts)]


def stage_cluster_decimate(ctx, d):
    """The hand-worked scene: ten vertices in four cells, of its faces three collapse, two are duplicates and one names a missing vertex,
    so both compactions drop something; then the same vertices without a face (the call returns behind the vertex phase)."""
    verts_q, faces, s = d["decimate"]
    got = device_decimate(ctx, verts_q, faces, s, check=False)
    stats = same_decimation(got, verts_q, faces, s)
    assert stats[_hip.GR_DECIM_STAT_COLLAPSED] > 0 and stats[_hip.GR_DECIM_STAT_DUPLICATES] > 0
    assert 0 < stats[_hip.GR_DECIM_STAT_KEPT_VERTICES] < len(verts_q)
    none = np.zeros((0, 3), dtype=np.int32)
    bare = device_decimate(ctx, verts_q, none, s)
    same_decimation(bare, verts_q, none, s)
    return list(got) + list(bare)


def stage_polygon_box_pairs_count(ctx, d):
    table_a, table_b, pairs = d["overlap"]
    listed = _np(ctx.polygon_overlap(table_a, table_b).pairs())
    assert listed.dtype == np.int32 and np.array_equal(listed, pairs) and np.array_equal(listed, ov.box_pairs(table_a, table_b))
    return [listed]


def stage_polygon_overlap_areas(ctx, d):
    """The "parts" scene in tiles of 8 x 16 slots: each of its two pairs is split over several items.  Then the same items with a
    malformed one between them and a third pair that no item names: the areas of the first two are the same bits, the third is zero,
    the bad item is counted."""
    table_a, table_b, pairs = d["overlap"]
    _, area, area_abs = check_overlap_scene(ctx, "parts", False, tile=(8, 16))
    good = overlap_work_items(table_a[1], table_a[2], table_b[1], table_b[2], pairs, (8, 16))
    assert len(good) > 2 * len(pairs) and pairs.tolist() == [[0, 0], [0, 1]]
    overlap = ctx.polygon_overlap(table_a, table_b)
    want_stats = _np(overlap.areas(pairs, good)[2]).copy()
    items = np.concatenate([good[good[:, 0] == 0], np.array([[0, 0, 257, 0, 1]], dtype=np.int32), good[good[:, 0] == 1]])
    more = np.concatenate([pairs, pairs[:1]])
    it_t, pr_t = ctx._dev(items, torch.int32), ctx._dev(more, torch.int32)
    out, out_abs, stats = ctx._empty((3,), torch.float64), ctx._empty((3,), torch.float64), ctx._stats(_hip.GR_OVERLAP_STAT_WORDS)
    ctx._call("gr_polygon_overlap_areas", *overlap._table_args(overlap._a), *overlap._table_args(overlap._b), pr_t.data_ptr(), 3,
              it_t.data_ptr(), len(items), out.data_ptr(), out_abs.data_ptr(), stats.data_ptr(), ctx._stream())
    out, out_abs, stats = _np(out), _np(out_abs), _np(stats)
    assert np.array_equal(out[:2], area) and np.array_equal(out_abs[:2], area_abs) and out[2] == 0 and out_abs[2] == 0
    want_stats[_hip.GR_OVERLAP_STAT_PAIRS] = 3
    want_stats[_hip.GR_OVERLAP_STAT_BAD_ITEMS] = 1
    assert np.array_equal(stats, want_stats) and want_stats[_hip.GR_OVERLAP_STAT_ITEMS] == len(good)
    return [area, area_abs, out, out_abs, stats]


def stage_ray_pairs(ctx, d):
    r = d["rays"]
    edges = ctx.ray_pair_edges(*r["args"])
    _check_rays(edges, r)
    assert ctx.last_ray_pair_calls == 1
    again = ctx.ray_pair_edges(*r["args"], capacity=8)   # the count overflows the buffers: the call is repeated at the total
    _check_rays(again, r)
    assert ctx.last_ray_pair_calls == 2
    return [_np(x) for x in edges + again]


def stage_louvain_communities(ctx, d):
    """hub_star(65): the wave and workgroup paths; hub_star(GR_COMM_LDS_ROW + 1): the key path on the default choice; the ring of
    cliques: several levels, so rows, tot, size and the key buffers are rebuilt over those of the level before; a call with a bad
    edge, which ends behind the first sum, then the good one again.  Each under every force_path."""
    out = []
    for name, (graph, want) in d["graphs"].items():
        for path in PATHS:
            got = ctx.louvain_communities(*graph, force_path=path)
            same_communities(got, want, rows=path is None)
            if path is None:
                paths = got["rows_per_path"]
                assert (paths[1] > 0) == (name != "ring") and (paths[2] > 0) == (name == "hub1025"), (name, paths)
            if path == "key":
                assert got["rows_per_path"][1] == 0 and got["rows_per_path"][2] > 0
            out += [got[k] for k in ("community", "size", "in", "tot")] + [np.array(got["rows_per_path"] + got["sweeps"] + got["moves"])]
    assert d["graphs"]["ring"][1]["levels"] >= 2
    (i, j, q, n), want = d["graphs"]["ring"]
    bad_q = q.copy()
    bad_q[3] = 0
    for path in PATHS:
        with pytest.raises(ValueError, match="1 bad edges"):
            ctx.louvain_communities(i, j, bad_q, n, force_path=path)
        assert ctx.last_bad_edges == 1
        same_communities(ctx.louvain_communities(i, j, q, n, force_path=path), want, rows=path is None)
    return out


def stage_community_points(ctx, d):
    s = d["survey60"]
    got = _np(ctx.community_points(s["starts"], s["ends"], s["community"], s["m"]))
    assert got.shape == (s["m"], 3) and np.isnan(got[s["m"] - 1]).all() and np.isfinite(got[s["m"] - 2]).all()
    assert points_close(got, s["want_points"], s["bound"])
    return [got]


STAGES = {
    "gr_mesh_upload": stage_mesh_upload, "gr_resize_image_f64": stage_resize_image, "gr_points_bounds": stage_points_bounds,
    "gr_set_cover": stage_set_cover, "gr_count_pairs": stage_count_pairs, "gr_points_in_region": stage_points_in_region,
    "gr_submesh_extract": stage_submesh_extract, "gr_class_outlines": stage_class_outlines, "gr_member_outlines": stage_member_outlines,
    "gr_cluster_count": stage_cluster_count, "gr_cluster_decimate": stage_cluster_decimate,
    "gr_polygon_box_pairs_count": stage_polygon_box_pairs_count, "gr_polygon_overlap_areas": stage_polygon_overlap_areas,
    "gr_ray_pairs": stage_ray_pairs, "gr_louvain_communities": stage_louvain_communities, "gr_community_points": stage_community_points,
}
assert len(STAGES) == 16


@pytest.fixture(scope="module")
def data(ctx, mesh, rays):
    """The inputs of every stage and the answers of the stand-ins: computed once, shared by the three modes, not modified."""
    d = dict(mesh=mesh, rays=rays)
    d["upload"] = su.upload_np(mesh["points"].astype(np.float32), mesh["faces"])
    d["image"] = resize_image_values(np.random.default_rng(5), (48, 64, 3), "float64")
    d["resized"] = oracle_resize.resize_antialias(d["image"], (12, 16))
    d["bounds"] = points_bounds_np(mesh["points"], 1)
    A = setcover_standin.random_incidence(200, 12, 0.5, 2)
    d["cover"] = (A, setcover_standin.set_cover(A, 1, True))
    assert len(d["cover"][1]["pruned"]) == 1
    cls = np.random.default_rng(9).integers(0, 5, mesh["ids"].shape).astype(np.float64)
    cls[np.random.default_rng(10).random(cls.shape) < 0.2] = np.nan
    d["pairs"] = (cls, _index_oracle(mesh["ids"], cls, 450, 5, True))
    table = PlanarPolygons([vs.square(3.25, 2.5, 9.75, 11.0)], [0], [False]).snapped()
    want_mask, info = points_in_region_np(mesh["verts_q"], table, REGION_D)
    assert 0 < want_mask.sum() < len(want_mask)
    d["region"] = (table, want_mask, info)
    verts, faces, _ = osn.grid_mesh(3, 1)
    d["members"] = (verts, faces, [[0, 1, 2] if f != 3 else [] for f in range(6)])
    verts_q, faces, s, _, _ = ds.hand_scene()
    d["decimate"] = (verts_q, faces, s)
    d["overlap"] = ov.scene_tables("parts", False)
    graphs = {"hub65": cs.hub_star(65), "hub1025": cs.hub_star(_hip.GR_COMM_LDS_ROW + 1), "ring": cs.clique_ring(30, 5)}
    d["graphs"] = {name: (g, cs.louvain(*g)) for name, g in graphs.items()}
    # survey60 of tests/test_communities_gpu.py: its rays, its edges from the device (no poison), the stand-in's communities
    sv = synthetic.detection_survey(n_objects=60, n_cameras=40, seed=0, sigma=0.15)
    i, j, w = numeric.ray_pair_edges(sv["ray_starts"], sv["ray_ends"], sv["ray_IDs"], 0.1, backend=ctx)
    n = len(sv["ray_IDs"])
    found = cs.louvain(i, j, numeric.quantise_weights(w), n)
    community, m = found["community"].copy(), found["n_communities"]
    assert n > 400 and m > 10
    community[:300] = m          # more members than k_community_points stages in LDS
    community[300] = m + 1       # a single member: NaN
    community[301:305] = -1      # rays of no community
    m += 2
    d["survey60"] = dict(starts=sv["ray_starts"], ends=sv["ray_ends"], community=community, m=m,
                         want_points=cs.community_points(sv["ray_starts"], sv["ray_ends"], community, m),
                         bound=points_bound(community, m, np.concatenate([sv["ray_starts"], sv["ray_ends"]])))
    return d


_UNPOISONED = {}   # stage -> the device's arrays with the bits off, computed once and never changed


def _same_bits(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, k)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("stage", list(STAGES))
def test_stage_equals_its_stand_in_on_poisoned_scratch(ctx, data, stage, mode):
    if stage not in _UNPOISONED:
        _UNPOISONED[stage] = STAGES[stage](ctx, data)
    if mode == "off":
        return   # (the run above, or the one an earlier mode made: held against the stand-in inside the stage function)
    with poison(ctx, MODES[mode]):
        got = STAGES[stage](ctx, data)
    _same_bits(got, _UNPOISONED[stage], (stage, mode))


# ---- stages in turn under poison: the production orders -----------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["ff", "7f"])
def test_triangulation_order_under_poison(ctx, data, mode):
    """`triangulate_detections`: ray pairs (65 536 edge slots: the largest plan), then the communities of that graph, then their
    points, each on the poisoned tail of the call before."""
    r = data["rays"]
    starts, ends, ids, _ = r["args"]
    with poison(ctx, MODES[mode]):
        ei, ej, ed = ctx.ray_pair_edges(*r["args"])
        _check_rays((ei, ej, ed), r)
        q = numeric.quantise_weights(1 / np.maximum(_np(ed), 1e-6))
        got = ctx.louvain_communities(ei, ej, q, len(ids))
        pts = _np(ctx.community_points(starts, ends, got["community"], got["n_communities"]))
    want = cs.louvain(_np(ei), _np(ej), q, len(ids))
    same_communities(got, want)
    assert want["n_communities"] >= 3
    assert points_close(pts, cs.community_points(starts, ends, want["community"], want["n_communities"]),
                        points_bound(want["community"], want["n_communities"], np.concatenate([starts, ends])))
    if "triangulation" in _UNPOISONED:
        _same_bits([_np(ei), _np(ej), _np(ed), got["community"], pts], _UNPOISONED["triangulation"], mode)
    _UNPOISONED["triangulation"] = [_np(ei), _np(ej), _np(ed), got["community"], pts]


@pytest.mark.parametrize("mode", ["ff", "7f"])
def test_aggregation_order_under_poison(ctx, data, mode):
    """`aggregate_images` and what follows it: upload, the pair sort, the class outlines, the region and the sub-mesh, the set cover.  A
    large call first (the row pass of a 256 x 256 x 3 resize), so that every stage sees a poisoned tail."""
    with poison(ctx, MODES[mode]):
        ctx.resize_image(np.random.default_rng(3).random((256, 256, 3)), (64, 64))
        for stage in ("gr_mesh_upload", "gr_count_pairs", "gr_class_outlines", "gr_points_in_region", "gr_submesh_extract", "gr_set_cover",
                      "gr_points_bounds", "gr_resize_image_f64"):
            got = STAGES[stage](ctx, data)
            if stage in _UNPOISONED:
                _same_bits(got, _UNPOISONED[stage], (stage, mode))
