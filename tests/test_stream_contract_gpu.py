"""Every stream-taking call of the library on a side stream, with the default stream held and the producer delayed
(tests/stream_probe.py): "all work is enqueued on `stream`" and "no hidden synchronisation" of include/geograster.h, made visible.

One `StreamProbeHipRaster` and one side stream for the module.  A row is a scene and the comparison with the stand-in or oracle that
the stage's own GPU test uses: most rows ARE the fenced case of that stage (tests/test_output_fences_gpu.py, the `test_fenced_outputs`
cases of the later stages), called with the probe as their context and at one size, the "+ 1" size of that module.  Every row runs
(a) alone on the side stream, (b) with the default stream held, (c) with its inputs zeroed until a delay on its own stream has
passed, (d) both; the fences are checked after each.

`COVERED` names, per function of the headers under include/ whose last parameter is `void *stream`, the rows that call it;
tests/test_stream_probe_host.py fails for a function in neither `COVERED` nor `EXEMPT`.  `SYNCHRONISES` names the functions whose
header comment says "Synchronises": leg A records for every library call whether it waited for its stream, and the last test holds
the two against each other.

Lengths are printed per row (`-s`): the measured wall time of (a), the hold, the delay, and which library calls leg A counted for."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))   # the stand-ins import one another by their plain names

from geograypher_amd import _hip  # noqa: E402
from geograypher_amd.utils import synthetic  # noqa: E402
from oracle import oracle_c, oracle_np  # noqa: E402
from tests import community_standin as cs  # noqa: E402
from tests import stream_probe as sp  # noqa: E402
from tests import test_communities_gpu as t_comm  # noqa: E402
from tests import test_height_above_ground_gpu as t_terrain  # noqa: E402
from tests import test_output_fences_gpu as t_fences  # noqa: E402
from tests import test_polygon_burn_gpu as t_burn  # noqa: E402
from tests import test_polygon_overlap_gpu as t_overlap  # noqa: E402
from tests import test_ring_simplify_gpu as t_simplify  # noqa: E402
from tests import test_stage_edges as t_stage  # noqa: E402
from tests import test_top_down_raster_gpu as t_nadir  # noqa: E402
from tests.test_communities_gpu import survey60  # noqa: E402,F401  (fixtures of the scenes the rows reuse)
from tests.test_communities_host import points_bound  # noqa: E402
from tests.test_face_outlines_gpu import same as same_outlines  # noqa: E402
from tests.test_output_fences_gpu import (crs_golden, decimation_scene, equirect_source, grid, grid_polygons,  # noqa: E402,F401
                                          region_table, survey, terrain, triangulation_gold)
from tests.ray_standin import ray_pair_edges_np  # noqa: E402
from tests.test_ray_pairs import _standin_tol  # noqa: E402

pytestmark = pytest.mark.gpu

_np = t_fences._np


# ---- the rows -----------------------------------------------------------------------------------------------------------------
def row_sample_raster(p, s):
    """`test_sample_raster` of tests/test_output_fences_gpu.py at N = 257, faces, three bands, without its last part: a label
    tensor rewritten in place is an output, and the probe hands the library a private copy of whatever goes through `_dev`."""
    points, faces, _, raster = s["terrain"]
    faces = faces[-257:]
    want = t_terrain.check_against_standin(p, points, faces, raster)
    assert want["values"].shape == (257, 3)
    values, height, lab, stats = p.sample_raster(points, faces, raster.data, raster.inverse, raster.nodata, np.nan, want_height=False)
    assert height is None and lab is None and t_terrain.same(_np(values), want["values"])
    assert _np(stats).tolist() == want["stats"].tolist()


def row_communities(p, s):
    """`test_one_case_behind_fenced_and_poisoned_outputs` of tests/test_communities_gpu.py on the probe, default path."""
    s, want = s["survey60"], s["louvain60"]
    got = p.louvain_communities(s["i"], s["j"], s["q"], s["n"])
    pts = _np(p.community_points(s["starts"], s["ends"], got["community"], got["n_communities"]))
    t_comm.same(got, want)
    assert t_comm.points_close(pts, cs.community_points(s["starts"], s["ends"], want["community"], want["n_communities"]),
                               points_bound(want["community"], want["n_communities"], np.concatenate([s["starts"], s["ends"]])))


def _burn_scene(size=257):
    """The scene of `test_fenced_outputs` (tests/test_polygon_burn_gpu.py) at 257 x 257 cells, without a device: the tables, the work
    items and the stand-in's answer (Python integers: computed once, outside every hold)."""
    rings = [t_burn.square(-1, -1, size + 1, size + 1), t_burn.square(0.2 * size, 0.2 * size, 0.75 * size + 0.4, 0.75 * size + 0.4),
             np.array([(0.0, 0.0), (size, 0.3 * size), (0.4 * size, size)])]
    inverse = t_burn.invert_affine(t_burn.IDENTITY)
    rv, off = t_burn.rings_to_cell_units(rings, inverse)
    rp, values, window = np.array([0, 1, 2], dtype=np.int32), [10, 20, 30], (0, 0, size, size)
    items = t_burn.burn_work_items(t_burn.row_centre_boxes(rv, off, rp, 3), t_burn.row_ring_ranges(rp, 3), window)
    want_rows, want_out, want_stats = t_burn.bs.burn(t_burn.bs.to_cell_units(rings, inverse), [0, 1, 2], 3, window, values, 255)
    want_stats[0] = int((items[:, 3].astype(np.int64) * items[:, 4]).sum())
    assert max(values) < t_fences.POISON and (want_rows == -1).sum() == 0 and len(np.unique(want_rows)) == 3
    return dict(rv=rv, off=off, rp=rp, values=values, window=window, items=items, want=(want_rows, want_out, want_stats))


def row_burn(p, s):
    b = s["burn"]
    burner = p.polygon_burner(b["rv"], b["off"], b["rp"], 3, b["values"])
    rows, out, stats = burner.window(*b["window"], b["items"], fill=255)
    only_rows = burner.window(*b["window"], b["items"], fill=255, want_values=False)
    for got, want in zip((rows, out, stats, only_rows[0]), b["want"] + (b["want"][0],)):
        assert np.array_equal(_np(got), want)
    assert only_rows[1] is None


def _overlap_scene(size=257):
    """The scene of `test_fenced_outputs` (tests/test_polygon_overlap_gpu.py) at 257 rows a table, without a device."""
    ov = t_overlap.ov
    side = 6.0 * size ** 0.5
    table_a, table_b, _ = t_overlap.snap_polygon_pair(ov.polygons_of(ov.star_rows(50 + size, size, extent=(side, side))),
                                                      ov.polygons_of(ov.star_rows(60 + size, size, extent=(side, side))))
    pairs = ov.box_pairs(table_a, table_b)
    assert len(pairs) >= size
    items = t_overlap.overlap_work_items(table_a[1], table_a[2], table_b[1], table_b[2], pairs)
    return dict(a=table_a, b=table_b, pairs=pairs, items=items, want=ov.restated_areas(table_a, table_b, pairs, len(items)))


def row_overlap(p, s):
    o = s["overlap"]
    overlap = p.polygon_overlap(o["a"], o["b"])
    listed = overlap.pairs()
    area, area_abs, stats = (_np(t) for t in overlap.areas(listed, o["items"]))
    want, want_abs, want_stats = o["want"]
    bound = t_overlap.gs.overlap_bound(want_abs)
    assert np.array_equal(_np(listed), o["pairs"]) and np.array_equal(stats, want_stats)
    assert np.all(np.abs(area - want) <= 2 * bound) and np.all(np.abs(area_abs - want_abs) <= bound)


def row_argmax_f64(p, s):
    """gr_argmax_nonzero_f64, which the binding's `argmax_nonzero` does not use: the float64 rows of `test_projection_stages`
    through both entry points; `_argmax_check` holds the first against numpy, the second must equal it bit for bit."""
    rows = t_stage._argmax_rows(np.random.default_rng(257), 3, 257)
    want = t_stage._argmax_check(p, rows)
    arr = p._dev(rows, torch.float64)
    out = p._empty((257,), torch.float64)
    p._call("gr_argmax_nonzero_f64", arr.data_ptr(), 257, 3, out.data_ptr(), p._stream())
    t_stage._same(_np(out), want)


def row_ray_pairs_short_room(p, s):
    """Count-then-fill with too little room: half the total is offered, the binding calls the library twice."""
    sv = s["survey"]
    pick = np.arange(257) * (len(sv["ray_IDs"]) // 257)
    starts, ends, ids = sv["ray_starts"][pick], sv["ray_ends"][pick], sv["ray_IDs"][pick]
    want = s["ray_edges_257"]
    total = len(want[0])
    assert total >= 2
    got = [_np(x) for x in p.ray_pair_edges(starts, ends, ids, 4.0, capacity=total // 2)]
    assert p.last_ray_pair_calls == 2
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.abs(got[2] - want[2]).max() <= _standin_tol(s["triangulation_gold"])


def row_class_outlines_short_room(p, s):
    verts_q, faces, classes = t_fences._cut(s["grid"], 257)
    E = s["outline_edges_257"]
    want = same_outlines(p, verts_q, faces, classes, 3, capacity=E // 2)
    assert want["n_edges"] == E > 1 and p.last_outline_calls == 2


def _fused_scene(grid, n=9, C=3):
    points, faces = np.array(grid["points"]), np.array(grid["faces"])
    recs = t_fences._records(32, 32, n)
    ids = np.stack([oracle_c.raster(points, faces, recs[v], 32, 32) for v in range(n)])
    labels = np.stack([synthetic.synthetic_labels(ids[v], v, C) for v in range(n)])
    F = len(faces)
    projs = [oracle_np.project_image(ids[v].astype(np.int64), t_stage._one_hot(labels[v], C), F) for v in range(n)]
    return dict(points=points, faces=faces, recs=recs, ids=ids, labels=labels, C=C, want=t_stage._want_sums(projs, F))


def _row_fused(variant):
    def body(p, s):
        """Nine views of the 450-face, 32 x 32 scene in launch groups of two: five groups."""
        f = s["fused"]
        p.set_option(_hip.GR_OPT_BATCH, 2)
        p.set_option(_hip.GR_OPT_VARIANT, variant)
        try:
            p.upload_mesh(f["points"].astype(np.float32), f["faces"])
            votes, counts = p.new_vote_buffers(f["C"])
            ids_out = p._empty(f["ids"].shape, torch.int32)
            p.raster_project_labels(f["recs"], f["labels"], f["C"], votes, counts, ids_out=ids_out)
            avg, summed, cnt = (_np(t) for t in p.finalize_votes(votes, counts))
            np.testing.assert_array_equal(_np(ids_out), f["ids"])
            want_avg, want_sum, want_cnt = f["want"]
            t_stage._same(summed, want_sum)
            t_stage._same(cnt, want_cnt)
            t_stage._same(avg, want_avg)
        finally:
            p.set_option(_hip.GR_OPT_BATCH, 64)
            p.set_option(_hip.GR_OPT_VARIANT, 0)
    return body


def row_raster_then_status(p, s):
    """One launch group without a look (the row's warm-up has looked): the view totals are added up by `raster_status`, which
    works on the stream of the last raster call, not on an argument of its own."""
    f = s["fused"]
    p.upload_mesh(f["points"].astype(np.float32), f["faces"])
    ids = p.raster_face_ids(f["recs"][:3], 32, 32, check=False)
    status = p.raster_status()
    np.testing.assert_array_equal(_np(ids), f["ids"][:3])
    assert status["overflow"] == 0 and status["views_done"] == 3 and status["records"] == s["status_records"] > 0


def _fenced_case(test, *args):
    return lambda p, s: test(p, *(s[a] if isinstance(a, str) and a in s else a for a in args))


ROWS = {
    # row: (the functions it must call, the body)
    "raster_face_ids": (["gr_mesh_upload", "gr_raster_face_ids"], _fenced_case(t_fences.test_raster_face_ids, "grid", (33, 65), 3, True)),
    "raster_project_labels": (["gr_raster_project_labels_u8"], _fenced_case(t_fences.test_raster_project_labels, "grid", (33, 65), 3)),
    "fused_side_stream": (["gr_raster_project_labels_u8", "gr_finalize_votes"], _row_fused(0)),
    "fused_votes_inline": (["gr_raster_project_labels_u8", "gr_finalize_votes"], _row_fused(_hip.GR_VAR_VOTES_INLINE)),
    "raster_then_status": (["gr_raster_face_ids"], row_raster_then_status),
    "debug_upload": (["gr_debug_read_upload"], _fenced_case(t_fences.test_debug_upload, "grid_F257")),
    "debug_stage": (["gr_debug_read_stage", "gr_points_bounds"], _fenced_case(t_fences.test_debug_stage, "grid", 257)),
    "projection_stages": (["gr_gather_texture_f64", "gr_gather_texture_u8", "gr_project_view_f64", "gr_project_values_f64",
                           "gr_finalize_sums_f64", "gr_project_labels_u8", "gr_finalize_votes", "gr_project_index_pairs",
                           "gr_count_pairs", "gr_argmax_nonzero"], _fenced_case(t_fences.test_projection_stages, 257, 3, (7, 37))),
    "argmax_f64": (["gr_argmax_nonzero", "gr_argmax_nonzero_f64"], row_argmax_f64),
    "pair_paths": (["gr_project_index_pairs", "gr_project_rect_pairs", "gr_project_polygon_pairs", "gr_count_pairs"],
                   _fenced_case(t_fences.test_pair_paths, 5)),
    "resize_image": (["gr_resize_image_f64"], _fenced_case(t_fences.test_resize_image, (37, 53), 3)),
    "warp_image": (["gr_warp_nearest_i32", "gr_warp_f64"], _fenced_case(t_fences.test_warp_image, (37, 53), 3)),
    "invert_distortion": (["gr_invert_distortion_f64"], _fenced_case(t_fences.test_invert_distortion, (37, 53))),
    "equirect_view": (["gr_equirect_view"], _fenced_case(t_fences.test_equirect_view, "equirect_source", (37, 53), 3, 2)),
    "ray_pairs": (["gr_ray_pairs"], _fenced_case(t_fences.test_ray_pairs, "triangulation_gold", "survey", 257)),
    "ray_pairs_short_room": (["gr_ray_pairs"], row_ray_pairs_short_room),
    "clip_rays": (["gr_rays_clip"], _fenced_case(t_fences.test_clip_rays, "triangulation_gold", 257, 129)),
    "cover_bounds_and_grid": (["gr_points_bounds", "gr_cover_grid"], _fenced_case(t_fences.test_cover_bounds_and_grid, 4097, 57, 3)),
    "set_cover": (["gr_set_cover"], _fenced_case(t_fences.test_set_cover, 257, True)),
    "polygon_class_weights": (["gr_polygon_class_weights"], _fenced_case(t_fences.test_polygon_class_weights, 257, 3, True)),
    "face_polygon_index": (["gr_face_polygon_index"], _fenced_case(t_fences.test_face_polygon_index, "grid", "region_table", 257)),
    "region_and_submesh": (["gr_points_in_region", "gr_submesh_extract"],
                           _fenced_case(t_fences.test_region_and_submesh, "grid", "region_table", 257)),
    "class_outlines": (["gr_class_outlines"], _fenced_case(t_fences.test_class_outlines, "grid", 257, "none")),
    "class_outlines_short_room": (["gr_class_outlines"], row_class_outlines_short_room),
    "member_outlines": (["gr_member_outlines"], _fenced_case(t_fences.test_member_outlines, "grid", 257, "none")),
    "cluster_count_and_decimate": (["gr_cluster_count", "gr_cluster_decimate"],
                                   _fenced_case(t_fences.test_cluster_count_and_decimate, "decimation_scene", 257, 257, t_fences.ds.RANDOM_S)),
    "sample_raster": (["gr_sample_raster"], row_sample_raster),
    "reproject_points": (["gr_reproject_points"], _fenced_case(t_fences.test_reproject_points, "crs_golden", 257)),
    "assemble_tiles": (["gr_assemble_tiles"], _fenced_case(t_fences.test_assemble_tiles, "65x3", "uint8", True)),
    "zonal_class_counts": (["gr_zonal_class_counts"], _fenced_case(t_fences.test_zonal_class_counts, 3, 256)),
    "burn_polygons": (["gr_burn_polygons"], row_burn),
    "polygon_overlap": (["gr_polygon_box_pairs_count", "gr_polygon_box_pairs_fill", "gr_polygon_overlap_areas"], row_overlap),
    "communities": (["gr_louvain_communities", "gr_community_points"], row_communities),
    "simplify_rings": (["gr_simplify_rings"], _fenced_case(t_simplify.test_outputs_between_fences, 257)),
    "nadir_raster": (["gr_nadir_raster"], _fenced_case(t_nadir.test_between_fences_on_a_poisoned_arena, 0)),
}

COVERED = {}
for _row, (_functions, _) in ROWS.items():
    for _f in _functions:
        COVERED.setdefault(_f, []).append(_row)

# a stream-taking function without a row: name -> the one-line reason (empty: every one has its row above)
EXEMPT = {}

# The functions whose comment in the header says that the call synchronises its stream, restated; tests/test_stream_probe_host.py
# holds the table against the headers, the last test here against what leg A recorded.
SYNCHRONISES = {
    "gr_mesh_upload", "gr_debug_read_upload", "gr_debug_read_stage", "gr_project_index_pairs", "gr_count_pairs", "gr_ray_pairs",
    "gr_class_outlines", "gr_member_outlines", "gr_set_cover", "gr_louvain_communities", "gr_community_points", "gr_simplify_rings",
    "gr_nadir_raster",
}

# Waits that are neither the library's nor the binding's: row or test -> the note, with the line of evidence.  Measured on the MI355X
# with 4 hardware queues a process (`pool_placement` of tests/stream_probe.py prints it): a stream keeps the queue the runtime gives
# it at its first use, and every fourth stream in that order shares the queue of the null stream -- its work waits behind a held
# default stream although nothing was handed to that stream.
NOTES = {
    "fused_side_stream": "csrc/geograster.hip raster_views creates gr_ctx::side with hipStreamCreateWithFlags(hipStreamNonBlocking); where "
                         "the runtime queues it with the null stream the votes wait behind the hold: recorded, leg A and the inline row must pass",
    "test_two_contexts_on_one_device_through_the_mesh_class_with_the_default_stream_held":
        "meshes.py _driving takes torch.cuda.Stream(device) per device thread; the test advances torch's pool to two streams that do "
        "not share the null stream's queue, so that a wait seen there is one of the project's code",
}
OWN_STREAM_ROWS = ("fused_side_stream",)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    backend = sp.StreamProbeHipRaster(0)
    yield backend
    backend.close()


@pytest.fixture(scope="module")
def side(probe):
    sp.cycles_per_second(probe.device)
    return sp.pick_side_stream(probe.device)


@pytest.fixture(scope="module")
def scenes(grid, equirect_source, triangulation_gold, survey, region_table, grid_polygons, decimation_scene, terrain,  # noqa: F811
           crs_golden, survey60):  # noqa: F811
    """The scenes of the fenced cases, and the references of the rows of this module: computed once, shared, never written to."""
    s = dict(grid=grid, equirect_source=equirect_source, triangulation_gold=triangulation_gold, survey=survey,
             region_table=region_table, grid_polygons=grid_polygons, decimation_scene=decimation_scene, terrain=terrain,
             crs_golden=crs_golden, survey60=survey60)
    s["louvain60"] = cs.louvain(survey60["i"], survey60["j"], survey60["q"], survey60["n"])
    s["fused"] = _fused_scene(grid)
    s["burn"], s["overlap"] = _burn_scene(), _overlap_scene()
    pick = np.arange(257) * (len(survey["ray_IDs"]) // 257)
    s["ray_edges_257"] = ray_pair_edges_np(survey["ray_starts"][pick], survey["ray_ends"][pick], survey["ray_IDs"][pick], 4.0)
    verts_q, faces, classes = t_fences._cut(grid, 257)
    s["outline_edges_257"] = t_fences.osn.outlines_np(verts_q, faces, classes, 3)["n_edges"]
    return s


@pytest.fixture(scope="module")
def status_records(probe, side, scenes):
    """What `raster_status` reports for the three views of `raster_then_status`, read from a checked call on the side stream."""
    f = scenes["fused"]
    with torch.cuda.stream(side):
        probe.upload_mesh(f["points"].astype(np.float32), f["faces"])
        probe.raster_face_ids(f["recs"][:3], 32, 32)
        side.synchronize()
    scenes["status_records"] = int(probe.last_stats["records"])
    return scenes["status_records"]


# ---- the probe itself: three planted mistakes, torch only ---------------------------------------------------------------------
def _planted(probe, side, call, hold=None, delay=0.0):
    """A "call" that should copy a private input to a poisoned output on the current stream, run as a row's body is."""
    want = torch.arange(1, 4097, dtype=torch.int32)

    def body(p):
        inp = p._dev(want.numpy(), torch.int32)
        out = p._empty((4096,), torch.int32)
        p.around_call("planted", lambda: call(out, inp))
        got = out.cpu()
        assert torch.equal(got, want), "the output differs from the input"

    if hold is None:
        return sp.run_body(probe, side, body, delay)
    with sp.held_default_stream(probe.device, hold):
        return sp.run_body(probe, side, body, delay)


def test_a_copy_on_the_current_stream_passes_both_legs(probe, side):
    _planted(probe, side, lambda out, inp: out.copy_(inp))
    _planted(probe, side, lambda out, inp: out.copy_(inp), hold=sp.MIN_HOLD_S)
    _, calls = _planted(probe, side, lambda out, inp: out.copy_(inp), hold=sp.MIN_HOLD_S + 4 * sp.MIN_DELAY_S, delay=sp.MIN_DELAY_S)
    assert [c.waited for c in calls] == [False], "leg A counts for a call that only enqueues"


def test_a_copy_on_the_default_stream_fails_leg_b(probe, side):
    def on_default(out, inp):
        with torch.cuda.stream(torch.cuda.default_stream(probe.device)):
            out.copy_(inp)

    with pytest.raises(AssertionError, match="the output differs from the input"):
        _planted(probe, side, on_default, hold=sp.MIN_HOLD_S)


def test_a_copy_on_a_third_stream_fails_leg_a(probe, side):
    third = sp.pick_side_stream(probe.device, beside=(side,))   # one that does not queue behind the delay on `side`

    def on_third(out, inp):
        with torch.cuda.stream(third):
            out.copy_(inp)
        torch.cuda.current_stream(probe.device).wait_stream(third)   # even ordered BEHIND it: it has read too early

    with pytest.raises(AssertionError, match="the output differs from the input"):
        _planted(probe, side, on_third, delay=sp.MIN_DELAY_S)
    third.synchronize()


def test_a_device_wide_wait_is_reported_as_the_end_of_the_hold(probe, side):
    def waits(out, inp):
        out.copy_(inp)
        torch.cuda.synchronize(probe.device)

    with pytest.raises(AssertionError, match="the hold ended before the results were read"):
        _planted(probe, side, waits, hold=sp.MIN_HOLD_S)


# ---- one row per call ---------------------------------------------------------------------------------------------------------
WAITED = {}      # function -> the set of what leg A saw of it: True (it waited for its stream), False (it only enqueued)


@pytest.mark.parametrize("name", list(ROWS))
def test_row(probe, side, scenes, status_records, name):
    functions, body = ROWS[name]
    record = sp.run_row(probe, side, name, lambda p: body(p, scenes), own_stream_may_queue=name in OWN_STREAM_ROWS)
    if name in OWN_STREAM_ROWS and record["held"] is False:
        print(f"stream probe | {name}: a hold ended before the results were read -- {NOTES[name]}")
    else:
        assert record["held"] is True
    missing = sorted(set(functions) - set(record["calls"]))
    assert not missing, f"row {name} no longer calls {missing}"
    assert len(record["leg_a"]) == 2 * len(record["calls"])
    for call in record["leg_a"]:
        WAITED.setdefault(call.name, set()).add(call.waited)


# ---- devices=[0, 0] through the mesh class ------------------------------------------------------------------------------------
def test_two_contexts_on_one_device_through_the_mesh_class_with_the_default_stream_held(side, grid):  # noqa: F811
    """The route `_driving(own_stream=True)` serves, under leg B, with the comparison of tests/test_devices_kwarg.py: a mesh over
    `devices=[0, 0]` gives the votes of a single-device mesh bit for bit.  The caller's thread works on the side stream; each device
    thread takes a stream of its own from torch."""
    from geograypher_amd.meshes import TexturedPhotogrammetryMesh
    from tests.test_devices_kwarg import _label_set, _same

    points, faces = np.array(grid["points"]), np.array(grid["faces"])
    poses = [synthetic.nadir_pose(7.5, 7.5, 20.0), synthetic.nadir_pose(6.0, 8.0, 16.0, yaw_deg=30.0)]
    cams = synthetic.camera_set_from_poses([poses[k % 2] for k in range(4)], 30.0, 32, 32)
    seg = _label_set(points, faces, cams, 3)
    one = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR")
    many = TexturedPhotogrammetryMesh((points, faces), devices=[0, 0], log_level="ERROR")
    want_avg, want = one.aggregate_projected_images(seg)
    assert want["projection_counts"].sum() > 0

    def run():
        t0 = sp.time.perf_counter()
        with torch.cuda.stream(side):
            got_avg, got = many.aggregate_projected_images(seg)
            side.synchronize()
        _same(got_avg, want_avg)
        _same(got["summed_projections"], want["summed_projections"])
        np.testing.assert_array_equal(got["projection_counts"], want["projection_counts"])
        return sp.time.perf_counter() - t0

    wall = run()     # measured, and the warm-up: the contexts, the uploads and the arenas synchronise as they are made, as documented
    hold = max(sp.MIN_HOLD_S, sp.HOLD_FACTOR * wall)
    coming = sp.advance_pool(many.backends[0].device, 2)   # the streams the two device threads take next (NOTES)
    assert len(coming) == 2
    with sp.held_default_stream(many.backends[0].device, hold):
        run()
    print(f"\nstream probe | devices=[0, 0] | wall {wall * 1e3:.1f} ms | hold {hold:.2f} s | default stream still held when the "
          f"results were read: True")


# ---- the header's notes against what leg A recorded ---------------------------------------------------------------------------
def test_synchronises_notes_agree_with_what_leg_a_recorded():
    """A call that waited for its stream under leg A is marked "Synchronises" in its header, a marked call waited at least once.
    Runs behind the rows (file order)."""
    if not set(COVERED) <= set(WAITED):
        pytest.fail(f"the rows have not all run: nothing recorded for {sorted(set(COVERED) - set(WAITED))}")
    print("\n| row | wall (a), ms | hold, s | delay, ms | default stream held at the read | leg A |\n|---|---|---|---|---|---|")
    for r in sp.REPORT:
        print(f"| {r['row']} | {r['wall'] * 1e3:.1f} | {r['hold']:.2f} | {r['delay'] * 1e3:.0f} | {'yes' if r['held'] else 'NO'} | "
              f"{sp._summary(r['leg_a'])} |")
    print("\nstream probe | waited for its stream under leg A: " + " ".join(sorted(f for f, seen in WAITED.items() if True in seen)))
    print("stream probe | only enqueued: " + " ".join(sorted(f for f, seen in WAITED.items() if seen == {False})))
    unmarked = sorted(f for f in COVERED if True in WAITED[f] and f not in SYNCHRONISES)
    never = sorted(f for f in COVERED if True not in WAITED[f] and f in SYNCHRONISES)
    assert not unmarked, f"waited for their stream but are not marked in the header: {unmarked}"
    assert not never, f"marked in the header but never waited: {never}"
