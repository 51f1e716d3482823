"""-m gpu: a raster context held to "any history, same answer" (tests/context_steps.py: the catalogue, the oracles' expectations,
the runner).  Every test has contexts of its own, closed in a `finally`; the session's context is not touched.  Nothing here
provokes a device fault: a refusal is a return code, GR_EOVERFLOW a protocol.

What is written down here and in context_steps.py: the step list (context_steps.CATALOGUE), the seeds (SEEDS: 11 .. 18, 60 steps
each), the image sizes (32 x 32, 96 x 64, 130 x 70)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))   # the stand-ins import one another by their plain names

import context_steps as steps  # noqa: E402

from geograypher_amd import _hip
from geograypher_amd._hip import HipRaster

pytestmark = pytest.mark.gpu

REFUSED = (ValueError, IndexError, RuntimeError)   # a return code of the library, or the binding's own check in front of it


@pytest.fixture(scope="module")
def expected():
    """The oracles' outputs per step, and for the history-free status words what a FRESH context reports (one context per step)."""
    exp = steps.expected()
    for name in steps.NAMES:
        if steps.STEPS[name].status:
            ctx = HipRaster(0)
            try:
                steps.run(ctx, [name], exp)
                exp[name]["status"] = {k: ctx.last_stats.get(k) for k in steps.STEPS[name].status}
            finally:
                ctx.close()
    # the steps take the paths they are named for
    assert exp["dense B cap 64"]["status"]["max_entries"] > 64 and exp["dense B cap 64 no look"]["status"]["overflow_causes"] != 0
    return exp


def _on_a_context(names, expected, before=None):
    ctx = HipRaster(0)
    try:
        if before is not None:
            before(ctx)
        steps.run(ctx, names, expected)
    finally:
        ctx.close()


@pytest.mark.parametrize("first", steps.NAMES)
def test_every_ordered_pair(expected, first):
    _on_a_context(steps.pair_sequence(first), expected)


@pytest.mark.parametrize("seed", steps.SEEDS)
def test_seeded_sequence(expected, seed):
    _on_a_context(steps.seeded_sequence(seed), expected)


# ---- a refusal in the middle -----------------------------------------------------------------------------------------------------
def _upload_a(ctx):
    s = steps.scene("A32")
    steps.set_options(ctx)
    ctx.upload_mesh(s["points"], s["faces"])
    return s


def _refuse_h_16385(ctx):
    s = _upload_a(ctx)
    ctx.raster_face_ids(s["recs"][:1], 16385, 32)


def _refuse_null_cameras(ctx):
    _upload_a(ctx)
    out = ctx._empty((1, 32, 32), _hip._torch().int32)
    ctx._call("gr_raster_face_ids", None, 1, 32, 32, out.data_ptr(), None, ctx._stream())


def _refuse_no_classes(ctx):
    s = _upload_a(ctx)
    votes, counts = ctx.new_vote_buffers(3)
    ctx.raster_project_labels(s["recs"][:1], steps._labels(s, 3, [0]), 0, votes, counts)


def _refuse_label_plane_shape(ctx):
    s = _upload_a(ctx)
    votes, counts = ctx.new_vote_buffers(3)
    ctx.raster_project_labels(s["recs"][:1], steps._labels(s, 3, [0])[0], 3, votes, counts)   # (h, w) where (1, h, w) is due


def _refuse_missing_vertex(ctx):
    s = steps.scene("A32")
    bad = s["faces"].copy()
    bad[77, 1] = s["points"].shape[0]
    ctx.upload_mesh(s["points"], bad)


def _refuse_no_mesh(ctx):
    ctx.raster_face_ids(steps.scene("A32")["recs"][:1], 32, 32)    # GR_ENOMESH


REFUSALS = [_refuse_h_16385, _refuse_null_cameras, _refuse_no_classes, _refuse_label_plane_shape, _refuse_missing_vertex, _refuse_no_mesh]
REFUSAL_CASES = [(r, warm) for r in REFUSALS for warm in (False, True) if not (warm and r is _refuse_no_mesh)]


@pytest.mark.parametrize("refusal,warm", REFUSAL_CASES, ids=[f"{r.__name__[8:]}-{'after_fused' if w else 'fresh'}" for r, w in REFUSAL_CASES])
def test_a_refusal_in_the_middle(expected, refusal, warm):
    """The refusal on a new context, and behind a fused call of three launch groups (winner, the side stream and its events in
    use); then the whole catalogue once.  (The mesh-less context has no call in front of its refusal.)"""

    def before(ctx):
        if warm:
            steps.run(ctx, ["fused A 5 views batch 2 C=17"], expected)
        with pytest.raises(REFUSED):
            refusal(ctx)

    _on_a_context(steps.NAMES, expected, before)


# ---- options persist, and return -------------------------------------------------------------------------------------------------
def test_options_persist_and_return(expected):
    """Tile height 6, ONE_TILE + ENT48 + GENERAL_IDS and 64 slots per tile, set ONCE: two different calls that set nothing run in
    that configuration -- the ids are the oracle's (no option changes them), the status words are those of a fresh context that
    was configured the same way, and 64 slots are too few for the dense view, which the library can only know if the option held.
    With the defaults back, the default steps give what they always give."""
    var = _hip.GR_VAR_ONE_TILE | _hip.GR_VAR_ENT48 | _hip.GR_VAR_GENERAL_IDS

    def configure(ctx):
        steps.set_options(ctx, thl=6, cap=64, var=var)

    def two_calls(ctx):
        out = []
        for name, views in (("A96", [0, 1]), ("Bfar", [0])):
            s = steps.scene(name)
            ctx.upload_mesh(s["points"], s["faces"])
            ids = ctx.raster_face_ids(s["recs"][views], s["h"], s["w"]).cpu().numpy()
            assert np.array_equal(ids, s["ids"][views]), name
            out.append({k: ctx.last_stats[k] for k in steps.STATUS_WORDS})
        return out

    fresh = HipRaster(0)
    try:
        configure(fresh)
        want = two_calls(fresh)
    finally:
        fresh.close()
    assert want[1]["max_entries"] > 64 and want[1]["overflow_causes"] == _hip.GR_CAUSE_LIST_OUTGREW
    ctx = HipRaster(0)
    try:
        steps.run(ctx, ["ids B 130x70 batch 2", "fused A 1 view C=3"], expected)
        configure(ctx)
        assert two_calls(ctx) == want
        default = HipRaster(0)   # the same two calls under the defaults report other words: the comparison above can tell
        try:
            steps.set_options(default)
            assert two_calls(default) != want
        finally:
            default.close()
        steps.run(ctx, ["ids A 32x32", "ids+depth A 96x64", "dense B cap 64", "fused A 1 view C=3"], expected)
    finally:
        ctx.close()


# ---- caller-owned vote buffers across uploads ------------------------------------------------------------------------------------
def test_vote_buffers_of_the_caller_across_uploads(expected):
    a, b, C = steps.scene("A32"), steps.scene("B96"), 3
    views = [0, 1, 2]
    ctx = HipRaster(0)
    try:
        steps.set_options(ctx)
        ctx.upload_mesh(a["points"], a["faces"])
        votes_a, counts_a = ctx.new_vote_buffers(C)
        ctx.raster_project_labels(a["recs"][views], steps._labels(a, C, views), C, votes_a, counts_a)
        ctx.upload_mesh(b["points"], b["faces"])
        votes_b, counts_b = ctx.new_vote_buffers(C)
        ctx.raster_project_labels(b["recs"][:2], steps._labels(b, C, [0, 1]), C, votes_b, counts_b)
        ctx.upload_mesh(a["points"], a["faces"])
        ctx.raster_project_labels(a["recs"][views], steps._labels(a, C, views), C, votes_a, counts_a)
        want_v, want_c = steps._votes(a, C, views)
        assert want_c.max() >= 1
        assert np.array_equal(votes_a.cpu().numpy().view(np.uint32), 2 * want_v)
        assert np.array_equal(counts_a.cpu().numpy().view(np.uint32), 2 * want_c)
        want_v, want_c = steps._votes(b, C, [0, 1])
        assert np.array_equal(votes_b.cpu().numpy().view(np.uint32), want_v)
        assert np.array_equal(counts_b.cpu().numpy().view(np.uint32), want_c)
    finally:
        ctx.close()
