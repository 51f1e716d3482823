"""-m gpu: the overflow protocol with micro lists.  With micro lists a tile's segment holds two lists, compiled entries in whole
64-entry chunks from the front and 32-byte micro records from the back; each is bounded only on its own where it is stored and
walked, so a tile can hold both within their bounds and still have them overwrite each other.  k_bin_stats reports that case
("the lists met", overflow cause 4): the view is repeated like any overflow, and the fused tile kernel must not walk it -- a
record read as an entry, or an entry read as a record, gives an arbitrary face id to the winner atomics.  Every case asserts
that it reached the cause it is about (gr_raster_overflow_causes) and compares with the C oracle bit for bit."""
import numpy as np
import pytest
import torch

from geograypher_amd import _hip
from geograypher_amd.utils import synthetic
from oracle import oracle_c

pytestmark = pytest.mark.gpu

# variant bits: micro lists always; no look at the first launch group (status-call protocol)
MICRO, NO_LOOK = _hip.GR_VAR_MICRO_ALWAYS, _hip.GR_VAR_NO_LOOK
# variant bits: one tile per workgroup; chains of tiles even in small launches
SINGLE, CHAIN = _hip.GR_VAR_ONE_TILE, _hip.GR_VAR_CHAINS
LIST_OUTGREW, LISTS_MET = _hip.GR_CAUSE_LIST_OUTGREW, _hip.GR_CAUSE_LISTS_MET   # gr_raster_overflow_causes
H, W, C = 240, 320, 4


def _lessons(h):
    return h.last_retries + h.last_stats["rebinned_groups"]


def _merge(parts):
    pts, fcs, off = [], [], 0
    for p, f in parts:
        pts.append(p)
        fcs.append(f + off)
        off += p.shape[0]
    return np.concatenate(pts), np.concatenate(fcs)


def _terrain():
    """The terrain of tests/test_micro_lists.py: faces of 2-5 px at 320 x 240 from 40 m, nearly all micro pairs."""
    return synthetic.heightfield_mesh(142, 100.0, lambda x, y: 0.5 * np.sin(x / 7.0) + 0.5 * np.cos(y / 5.0), jitter=0.3, seed=1)


def _layers():
    """Three coarse wavy surfaces through the terrain's height range, faces of about 14 px from 40 m: compiled entries (50-130
    per 64 x 32 tile), partly hidden by the terrain and partly hiding it."""
    return [synthetic.heightfield_mesh(45, 100.0 + 3 * k,
                                       lambda x, y, k=k: 0.4 * k - 0.4 + 0.5 * np.sin(y / 9.0 + k) * np.cos(x / 11.0),
                                       jitter=0.25, seed=2 + k) for k in range(3)]


def _recs(height, n=4):
    poses = [synthetic.nadir_pose(2.0 * k - 3.0, 1.5 * k - 2.0, height, yaw_deg=25.0 * k) for k in range(n)]
    return synthetic.camera_set_from_poses(poses, f=250.0, width=W, height=H).get_raster_records(1.0, near=0.05)


class _Scene:
    def __init__(self, points, faces, recs):
        self.points, self.faces, self.recs = points, faces, recs
        self.F = faces.shape[0]
        self.ids, self.depth = [], []
        for v in range(recs.shape[0]):
            ids, dep = oracle_c.raster(points, faces, recs[v], H, W, want_depth=True)
            self.ids.append(ids)
            self.depth.append(dep)
        self.labels = np.stack([synthetic.synthetic_labels(self.ids[v], v, C) for v in range(recs.shape[0])])

    def votes(self, views):
        want_v = np.zeros((self.F, C), dtype=np.uint32)
        want_c = np.zeros(self.F, dtype=np.uint32)
        for v in views:
            oracle_c.project_labels(self.ids[v], self.labels[v], self.F, C, want_v, want_c)
        return want_v, want_c


@pytest.fixture(scope="module")
def both_lists():
    """Terrain + coarse layers: every tile gets compiled entries as well as micro records.  Views 0-3 from 28 m (sparser),
    4-7 from 40 m (dense)."""
    points, faces = _merge([_terrain()] + _layers())
    return _Scene(points, faces, np.concatenate([_recs(28.0), _recs(40.0)]))


def _defaults(hip):
    hip.set_option(_hip.GR_OPT_DEBUG, 0)
    hip.set_option(_hip.GR_OPT_TILE_H_LOG2, 5)
    hip.set_option(_hip.GR_OPT_BATCH, 64)
    hip.set_option(_hip.GR_OPT_VARIANT, 0)
    hip.set_option(_hip.GR_OPT_DIRECT_CAP, 512)


@pytest.fixture(autouse=True)
def _default_options(hip):
    _defaults(hip)
    yield
    _defaults(hip)


def _causes_of_unchecked_ids(hip, recs):
    hip.raster_face_ids(recs, H, W, check=False)
    try:
        hip.raster_status()
    except RuntimeError as e:
        assert "overflow" in str(e)
    return hip.overflow_causes()


_CAPS = {}


def _meeting_cap(hip, scene, thl):
    """The slots per tile at which the dense views' lists meet and neither list outgrows its own bound: scanned with ids-only
    calls, multiples of 64 upwards.  A scene that has drifted so that no such size exists fails here instead of testing nothing.
    (Uploads the scene's mesh.)"""
    hip.upload_mesh(scene.points.astype(np.float32), scene.faces.astype(np.int32))
    if thl in _CAPS:
        return _CAPS[thl]
    hip.set_option(_hip.GR_OPT_TILE_H_LOG2, thl)
    hip.set_option(_hip.GR_OPT_VARIANT, MICRO | NO_LOOK)
    seen = {}
    for cap in range(64, 8193, 64):
        hip.set_option(_hip.GR_OPT_DIRECT_CAP, cap)
        seen[cap] = _causes_of_unchecked_ids(hip, scene.recs[4:])
        if seen[cap] in (LISTS_MET, 0):
            break
    assert seen[cap] == LISTS_MET, f"no slots per tile at which only the lists meet: {seen}"
    # ... and at that size the sparse views fit
    assert _causes_of_unchecked_ids(hip, scene.recs[:4]) == 0
    _CAPS[thl] = cap
    return cap


def _assert_votes(votes, counts, want):
    np.testing.assert_array_equal(votes.cpu().numpy().view(np.uint32), want[0])
    np.testing.assert_array_equal(counts.cpu().numpy().view(np.uint32), want[1])


PATHS = {"default": (5, 0, False), "single_tile": (5, SINGLE, False), "chain": (5, CHAIN, False),
         "tile64": (6, 0, False), "ids_out": (5, 0, True)}


@pytest.mark.parametrize("path", list(PATHS))
def test_fused_first_call_whose_lists_meet(hip, both_lists, path):
    """A fused call at a size nothing taught the context (no ids call first, no look): the dense views' lists meet.  The
    fused tile kernel must leave those views alone, the call must report GR_EOVERFLOW once for cause 4 only, and the retry
    must give the oracle's votes (and ids with ids_out=).  The same call again, with nothing left to learn, gives the same votes:
    no stale winner is left behind."""
    thl, extra, with_ids = PATHS[path]
    s = both_lists
    cap = _meeting_cap(hip, s, thl)
    views = slice(4, 8)
    want = s.votes(range(4, 8))
    hip.set_option(_hip.GR_OPT_TILE_H_LOG2, thl)
    hip.set_option(_hip.GR_OPT_VARIANT, MICRO | NO_LOOK | extra)
    hip.set_option(_hip.GR_OPT_DIRECT_CAP, cap)
    for attempt in range(2):
        votes, counts = hip.new_vote_buffers(C)
        ids_out = torch.full((4, H, W), -7, dtype=torch.int32, device=hip.device) if with_ids else None
        hip.raster_project_labels(s.recs[views], s.labels[views], C, votes, counts, ids_out=ids_out)
        st = hip.last_stats
        assert st["views_done"] == 4 and st["overflow"] == 0 and st["rebinned_groups"] == 0
        if attempt == 0:
            assert hip.last_retries == 1 and st["overflow_causes"] == LISTS_MET, st
        else:
            assert hip.last_retries == 0 and st["overflow_causes"] == 0, st
        _assert_votes(votes, counts, want)
        if with_ids:
            for v in range(4):
                np.testing.assert_array_equal(ids_out[v].cpu().numpy(), s.ids[4 + v])


def test_lists_meet_in_a_later_launch_group(hip, both_lists):
    """Launch groups of four views: the sparse views (first group) fit, the dense ones (second group) meet.  The device folds
    in the first group exactly once, `views_done` says so, and the resumed call adds the rest.  Unchecked, the first group's
    votes are all there is and the status call tells why."""
    s = both_lists
    cap = _meeting_cap(hip, s, 5)
    want = s.votes(range(8))
    hip.set_option(_hip.GR_OPT_BATCH, 4)
    hip.set_option(_hip.GR_OPT_VARIANT, MICRO | NO_LOOK)
    hip.set_option(_hip.GR_OPT_DIRECT_CAP, cap)
    votes, counts = hip.new_vote_buffers(C)
    hip.raster_project_labels(s.recs, s.labels, C, votes, counts)
    st = hip.last_stats
    assert hip.last_retries == 1 and st["views_done"] == 8 and st["overflow"] == 0 and st["overflow_causes"] == LISTS_MET, st
    _assert_votes(votes, counts, want)
    hip.set_option(_hip.GR_OPT_DIRECT_CAP, cap)
    votes, counts = hip.new_vote_buffers(C)
    hip.raster_project_labels(s.recs, s.labels, C, votes, counts, check=False)
    with pytest.raises(RuntimeError, match="overflow"):
        hip.raster_status()
    assert hip.overflow_causes() == LISTS_MET
    _assert_votes(votes, counts, s.votes(range(4)))


def test_look_at_the_first_group_learns_a_segment_for_both_lists(hip, both_lists):
    """The default protocol at that size: the library looks at the first launch group's counts, sees the lists meet, bins
    the group again with a segment that holds both -- no status retry -- and the next call has nothing to learn."""
    s = both_lists
    cap = _meeting_cap(hip, s, 5)
    want = s.votes(range(4, 8))
    hip.set_option(_hip.GR_OPT_VARIANT, MICRO)
    hip.set_option(_hip.GR_OPT_DIRECT_CAP, cap)
    votes, counts = hip.new_vote_buffers(C)
    hip.raster_project_labels(s.recs[4:], s.labels[4:], C, votes, counts)
    st = hip.last_stats
    assert (hip.last_retries, st["rebinned_groups"], st["overflow_causes"], st["views_done"]) == (0, 1, LISTS_MET, 4), st
    _assert_votes(votes, counts, want)
    votes, counts = hip.new_vote_buffers(C)
    hip.raster_project_labels(s.recs[4:], s.labels[4:], C, votes, counts)
    assert _lessons(hip) == 0 and hip.last_stats["overflow_causes"] == 0
    _assert_votes(votes, counts, want)


def test_ids_only_call_whose_lists_meet(hip, both_lists):
    """ids and depth bits at that size: checked, the retry gives the oracle's; unchecked, the status call raises and
    reports cause 4."""
    s = both_lists
    cap = _meeting_cap(hip, s, 5)
    hip.set_option(_hip.GR_OPT_VARIANT, MICRO | NO_LOOK)
    hip.set_option(_hip.GR_OPT_DIRECT_CAP, cap)
    ids, depth = hip.raster_face_ids(s.recs[4:], H, W, want_depth=True)
    assert hip.last_retries == 1 and hip.last_stats["overflow_causes"] == LISTS_MET, hip.last_stats
    for v in range(4):
        np.testing.assert_array_equal(ids[v].cpu().numpy(), s.ids[4 + v])
        np.testing.assert_array_equal(depth[v].cpu().numpy().view(np.int32), s.depth[4 + v].view(np.int32))
    hip.set_option(_hip.GR_OPT_DIRECT_CAP, cap)
    hip.raster_face_ids(s.recs[4:], H, W, check=False)
    with pytest.raises(RuntimeError, match="overflow"):
        hip.raster_status()
    assert hip.overflow_causes() == LISTS_MET


@pytest.mark.parametrize("which", ["micro_records", "compiled_entries"])
def test_single_list_overflow_with_micro_lists(hip, which):
    """One list alone outgrows its bound, with micro lists on: records beyond 1.25 x the slots per tile (the terrain alone:
    hundreds of records per tile, hardly an entry), or entries beyond the slots per tile (the coarse layers alone: about a
    hundred entries per tile, few records).  Cause 1 is reported -- not only 4 -- and the retry gives the oracle's ids,
    depth bits and votes, fused as well."""
    points, faces = _terrain() if which == "micro_records" else _merge(_layers())
    s = _Scene(points, faces, _recs(40.0, n=2))
    hip.upload_mesh(points.astype(np.float32), faces.astype(np.int32))
    hip.set_option(_hip.GR_OPT_VARIANT, MICRO | NO_LOOK)
    hip.set_option(_hip.GR_OPT_DIRECT_CAP, 64)
    ids, depth = hip.raster_face_ids(s.recs, H, W, want_depth=True)
    assert hip.last_retries == 1 and hip.last_stats["overflow_causes"] & LIST_OUTGREW, hip.last_stats
    for v in range(2):
        np.testing.assert_array_equal(ids[v].cpu().numpy(), s.ids[v])
        np.testing.assert_array_equal(depth[v].cpu().numpy().view(np.int32), s.depth[v].view(np.int32))
    hip.set_option(_hip.GR_OPT_DIRECT_CAP, 64)
    votes, counts = hip.new_vote_buffers(C)
    hip.raster_project_labels(s.recs, s.labels, C, votes, counts)
    assert hip.last_retries == 1 and hip.last_stats["overflow_causes"] & LIST_OUTGREW, hip.last_stats
    _assert_votes(votes, counts, s.votes(range(2)))


def test_poisoned_scratch_fused_call_whose_lists_meet(hip, both_lists):
    """Every entry slot and row count starts as 0xFF (debug bit 512: scratch an earlier call left behind), micro lists, a fused
    first call whose lists meet: the oracle's votes all the same; then the same call clean, with nothing left to learn."""
    s = both_lists
    cap = _meeting_cap(hip, s, 5)
    want = s.votes(range(4, 8))
    hip.set_option(_hip.GR_OPT_VARIANT, MICRO | NO_LOOK)
    hip.set_option(_hip.GR_OPT_DIRECT_CAP, cap)
    hip.set_option(_hip.GR_OPT_DEBUG, _hip.GR_DBG_POISON_SLOTS)
    votes, counts = hip.new_vote_buffers(C)
    hip.raster_project_labels(s.recs[4:], s.labels[4:], C, votes, counts)
    assert hip.last_retries == 1 and hip.last_stats["overflow_causes"] == LISTS_MET and hip.last_stats["views_done"] == 4
    _assert_votes(votes, counts, want)
    hip.set_option(_hip.GR_OPT_DEBUG, 0)
    votes, counts = hip.new_vote_buffers(C)
    hip.raster_project_labels(s.recs[4:], s.labels[4:], C, votes, counts)
    assert _lessons(hip) == 0 and hip.last_stats["overflow_causes"] == 0
    _assert_votes(votes, counts, want)
