"""-m gpu: the host's choice of tile kernel (raster_tile.hip tile_kernel / tile_batch), swept over its axes at the smallest
shapes that reach every branch.  Every case is bit-exact against the C oracle: ids, depth bits, and the votes of the fused path.

Images (three views of the lattice terrain of raster_scenes.random_stress_scene(6); two views put faces into every tile, one
looks over the rim of the mesh and leaves its right tile column empty):
  68 x 33  width a multiple of 4 -- the PLAIN ids kernel runs; two tile columns with a ragged right edge; two tile rows of
           64 x 32 tiles with a one-row bottom tile, one row of 64 x 64 tiles;
  65 x 33  width no multiple of 4 -- the general ids kernel and the one-pixel-per-lane branch of store_ids run.
Axes: tile height, entry form, micro lists, one tile per workgroup / chains, single-pass / exact binning; per setting the outputs
ids, ids + depth, fused votes, fused votes + ids (with chains at tile height 32 the fused kernel is the rolling chain, with fewer
tiles than GR_ROLL_KT) and, at 68 x 33, the general ids kernel where the plain one would run."""
import itertools

import numpy as np
import pytest
import torch

from geograypher_amd import _hip
from geograypher_amd.utils import synthetic
from oracle import oracle_c
from tests import raster_scenes

pytestmark = pytest.mark.gpu

SIZES = [(33, 68), (33, 65)]
C = 3


def _folded(cap, ent48, micro):
    """A setting the library folds onto another one, by the rules tile_kernel states (resolve_binning decides them): 40-byte
    entries need single-pass binning with segments of whole 64-entry chunks and no GR_VAR_ENT48; micro lists need 40-byte
    entries.  So GR_VAR_MICRO_ALWAYS without 40-byte entries runs the kernels of GR_VAR_MICRO_NEVER, and under exact binning
    GR_VAR_ENT48 changes nothing."""
    ent40 = cap > 0 and cap % 64 == 0 and not ent48
    return (micro and not ent40) or (ent48 and cap == 0)


# (tile height log2, slots per tile, 48-byte entries, micro lists, chains)
SETTINGS = [s for s in itertools.product((5, 6), (512, 0), (False, True), (False, True), (False, True)) if not _folded(*s[1:4])]
assert len(SETTINGS) == 16   # per tile height and chain form: 40-byte, 40-byte + micro, 48-byte, exact


def _setting_id(s):
    thl, cap, ent48, micro, chains = s
    return "tile%d_%s_%s%s_%s" % (1 << thl, "direct" if cap else "exact", "ent48" if ent48 or not cap else "ent40",
                                  "_micro" if micro else "", "chains" if chains else "one_tile")


@pytest.fixture(scope="module")
def scene():
    """The mesh, and per image size the camera records and what the oracle makes of them: ids, depth, labels and the votes with
    and without the background-is-last-face flag.  Computed once; read only."""
    points, faces, _, _, _ = raster_scenes.random_stress_scene(6)
    F = faces.shape[0]
    poses = [synthetic.nadir_pose(0.1, -0.2, 0.6, yaw_deg=17.0), synthetic.nadir_pose(2.2, 0.3, 1.2),
             synthetic.nadir_pose(-0.5, 0.4, 0.9, yaw_deg=-40.0, tilt_x_deg=25.0, tilt_y_deg=-10.0)]
    ref = {}
    for h, w in SIZES:
        recs = synthetic.camera_set_from_poses(poses, f=40.0, width=w, height=h).get_raster_records(1.0, near=0.05)
        both = [oracle_c.raster(points, faces, recs[v], h, w, want_depth=True) for v in range(len(poses))]
        ids, depth = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
        labels = np.stack([synthetic.synthetic_labels(ids[v], v, C) for v in range(len(poses))])
        votes = {}
        for compat in (True, False):
            want_v, want_c = np.zeros((F, C), dtype=np.uint32), np.zeros(F, dtype=np.uint32)
            for v in range(len(poses)):
                oracle_c.project_labels(ids[v], labels[v], F, C, want_v, want_c, neg1_is_last_face=compat)
            votes[compat] = (want_v, want_c)
        # what the shapes are chosen for: faces in every tile of views 0 and 2, an empty tile column in view 1 -- at either tile height
        tiles = lambda v: [(ids[v, y:y + 32, x:x + 64] >= 0).any() for y in range(0, h, 32) for x in range(0, w, 64)]
        assert all(tiles(0)) and all(tiles(2)) and not tiles(1)[1] and not tiles(1)[3] and tiles(1)[0]
        ref[(h, w)] = dict(recs=recs, ids=ids, depth=depth, labels=labels, votes=votes)
    return dict(points=points.astype(np.float32), faces=faces.astype(np.int32), ref=ref)


def _same_ids(got, want, what):
    bad = np.argwhere(got.cpu().numpy() != want)
    assert bad.size == 0, f"{what}: {bad.shape[0]} pixels differ, first {bad[:5].tolist()}"


def _same_votes(votes, counts, want, what):
    np.testing.assert_array_equal(votes.cpu().numpy().view(np.uint32), want[0], err_msg=what)
    np.testing.assert_array_equal(counts.cpu().numpy().view(np.uint32), want[1], err_msg=what)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % (s[1], s[0]))
@pytest.mark.parametrize("setting", SETTINGS, ids=_setting_id)
def test_every_tile_kernel_choice_is_bit_exact(hip, scene, setting, size):
    thl, cap, ent48, micro, chains = setting
    h, w = size
    r = scene["ref"][size]
    var = (_hip.GR_VAR_VOTES_INLINE | (_hip.GR_VAR_ENT48 if ent48 else 0) |
           (_hip.GR_VAR_MICRO_ALWAYS if micro else _hip.GR_VAR_MICRO_NEVER) | (_hip.GR_VAR_CHAINS if chains else _hip.GR_VAR_ONE_TILE))
    hip.set_option(_hip.GR_OPT_TILE_H_LOG2, thl)
    hip.set_option(_hip.GR_OPT_DIRECT_CAP, cap)
    hip.set_option(_hip.GR_OPT_VARIANT, var)
    try:
        hip.upload_mesh(scene["points"], scene["faces"])
        _same_ids(hip.raster_face_ids(r["recs"], h, w), r["ids"], "ids")                 # 68: the plain kernel; 65: the general one
        if w % 4 == 0:
            hip.set_option(_hip.GR_OPT_VARIANT, var | _hip.GR_VAR_GENERAL_IDS)
            _same_ids(hip.raster_face_ids(r["recs"], h, w), r["ids"], "general ids")
            hip.set_option(_hip.GR_OPT_VARIANT, var)
        ids, depth = hip.raster_face_ids(r["recs"], h, w, want_depth=True)
        _same_ids(ids, r["ids"], "ids beside depth")
        np.testing.assert_array_equal(depth.cpu().numpy().view(np.int32), r["depth"].view(np.int32), err_msg="depth bits")
        votes, counts = hip.new_vote_buffers(C)
        hip.raster_project_labels(r["recs"], r["labels"], C, votes, counts)
        _same_votes(votes, counts, r["votes"][True], "fused votes")
        votes, counts = hip.new_vote_buffers(C)
        ids_out = torch.full((r["recs"].shape[0], h, w), -7, dtype=torch.int32, device=hip.device)
        hip.raster_project_labels(r["recs"], r["labels"], C, votes, counts, ids_out=ids_out, neg1_is_last_face=False)
        _same_votes(votes, counts, r["votes"][False], "fused votes beside ids")
        _same_ids(ids_out, r["ids"], "ids of the fused kernel")
    finally:
        hip.set_option(_hip.GR_OPT_TILE_H_LOG2, 5)
        hip.set_option(_hip.GR_OPT_DIRECT_CAP, 512)
        hip.set_option(_hip.GR_OPT_VARIANT, 0)
