"""The device buffers of a context (csrc/device_buffer.hpp: Buf, reserve, reserve_group, release_all) under calls that move them:
one context of its own, the smallest shapes at which each buffer grows, every result compared exactly with oracle.oracle_c.  A
larger mesh moves the upload's group (blk, soup, orig, bvert, bidx) and a smaller one behind it leaves the group alone; a larger
image moves `ctrl`; more views in a fused call move `winner` and `touched` -- and a fresh `winner` must arrive zeroed --; contexts
are created and destroyed in turn.  (A failed allocation is not provoked on a GPU: tests/test_device_buffer_host.py covers it.)"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))   # the stand-ins import one another by their plain names

import outline_standin as osn  # noqa: E402

from geograypher_amd import _hip
from geograypher_amd.utils import synthetic
from oracle import oracle_c

pytestmark = pytest.mark.gpu

C = 3


def _np(t):
    return t.cpu().numpy()


def _scene(n, poses, h, w):
    """An n x n quad grid at z = 0, its camera records and the oracle's ids for them."""
    verts_q, faces, _ = osn.grid_mesh(n, n)
    points = np.column_stack([verts_q / 1e6, np.zeros(len(verts_q))])
    faces = faces.astype(np.int32)
    recs = synthetic.camera_set_from_poses(poses, 30.0 * w / 32, w, h).get_raster_records(1.0, near=0.05)
    ids = np.stack([oracle_c.raster(points, faces, recs[v], h, w) for v in range(len(poses))])
    assert (ids >= 0).mean() > 0.5
    return dict(points=points.astype(np.float32), faces=faces, recs=recs, ids=ids, h=h, w=w)


POSES_A = [synthetic.nadir_pose(7.5, 7.5, 20.0), synthetic.nadir_pose(6.0, 8.0, 16.0, yaw_deg=30.0),
           synthetic.nadir_pose(8.5, 6.5, 18.0, yaw_deg=-50.0)]


@pytest.fixture(scope="module")
def ctx():
    """A context of its own: its buffers start empty and hold what these tests made them hold."""
    return _hip.HipRaster(0)


@pytest.fixture(scope="module")
def mesh_a():
    s = _scene(15, POSES_A, 32, 32)
    assert s["faces"].shape == (450, 3)   # 8 blocks of 64 faces
    return s


def _raster(ctx, scene, views=slice(None)):
    ids = _np(ctx.raster_face_ids(scene["recs"][views], scene["h"], scene["w"]))
    assert np.array_equal(ids, scene["ids"][views])
    return ids


def test_mesh_group_grows_and_is_then_left_alone(ctx, mesh_a):
    mesh_b = _scene(31, [synthetic.nadir_pose(15.5, 15.5, 40.0), synthetic.nadir_pose(12.0, 17.0, 33.0, yaw_deg=30.0)], 32, 32)
    assert mesh_b["faces"].shape == (1922, 3)   # 31 blocks
    for scene in (mesh_a, mesh_b, mesh_a):
        ctx.upload_mesh(scene["points"], scene["faces"])
        _raster(ctx, scene, slice(0, 2))


def test_image_size_grows_the_tile_counters(ctx, mesh_a):
    large = _scene(15, POSES_A[:2], 64, 96)   # 2 x 2 tiles of 64 x 32 where 32 x 32 has one: `ctrl` grows
    ctx.upload_mesh(mesh_a["points"], mesh_a["faces"])
    first = _raster(ctx, mesh_a, slice(0, 2))
    _raster(ctx, large)
    assert np.array_equal(_raster(ctx, mesh_a, slice(0, 2)), first)


def test_fused_views_grow_the_winners(ctx, mesh_a):
    F = 450
    labels = np.stack([synthetic.synthetic_labels(mesh_a["ids"][v], v, C) for v in range(3)])
    ctx.upload_mesh(mesh_a["points"], mesh_a["faces"])

    def fused(n):
        votes, counts = ctx.new_vote_buffers(C)
        ctx.raster_project_labels(mesh_a["recs"][:n], labels[:n], C, votes, counts)
        want_v, want_c = np.zeros((F, C), dtype=np.uint32), np.zeros(F, dtype=np.uint32)
        for v in range(n):
            oracle_c.project_labels(mesh_a["ids"][v], labels[v], F, C, want_v, want_c, neg1_is_last_face=True)
        got = _np(votes).view(np.uint32), _np(counts).view(np.uint32)
        assert np.array_equal(got[0], want_v) and np.array_equal(got[1], want_c) and want_c.max() >= 1
        return got

    one = fused(1)
    fused(3)          # `winner` and `touched` grow: a fresh `winner` block that was not zeroed would give stale winners
    again = fused(1)
    assert np.array_equal(again[0], one[0]) and np.array_equal(again[1], one[1])


def test_contexts_in_turn(mesh_a):
    for _ in range(4):
        own = _hip.HipRaster(0)
        try:
            own.upload_mesh(mesh_a["points"], mesh_a["faces"])
            _raster(own, mesh_a, slice(0, 1))
        finally:
            own.close()
