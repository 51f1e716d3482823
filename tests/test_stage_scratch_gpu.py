"""The stage arena (gr_ctx::stage, csrc/gr_internal.hpp: stage_acquire) under the stage calls that share it: one context of its
own, one small mesh (a 16 x 16 vertex grid, 450 faces).  Every stage is compared with its own stand-in or oracle exactly as its
own GPU test compares it -- the helpers are imported from those tests --; what is new here is the ORDER of the calls: stages in
turn on one stream, a small call after a large one, and two streams back to back."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))   # the stand-ins import one another by their plain names

import outline_standin as osn  # noqa: E402
import vector_standin as vs  # noqa: E402
from region_standin import points_in_region_np  # noqa: E402

from geograypher_amd import _hip
from geograypher_amd.utils import synthetic
from geograypher_amd.utils.geometric import PlanarPolygons
from oracle import oracle_c, oracle_resize
from tests import setcover_standin
from tests.conftest import GOLDEN
from tests.covering_standin import points_bounds_np
from tests.image_edge_cases import resize_image_values
from tests.ray_standin import ray_pair_edges_np
from tests.test_face_outlines_gpu import same as same_outlines
from tests.test_image_selection_gpu import _assert_same as same_cover, _device as device_cover
from tests.test_image_stage_edges import _close, _same_bits
from tests.test_roi_crop_gpu import device_region, device_submesh, same_submesh
from tests.test_stage_edges import _index_oracle

pytestmark = pytest.mark.gpu

REGION_D = 250_000   # a quarter of a grid cell, in grid steps


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def ctx():
    """A context of its own: its arena starts empty and holds what these tests put there."""
    return _hip.HipRaster(0)


@pytest.fixture(scope="module")
def mesh():
    verts_q, faces, quad = osn.grid_mesh(15, 15)
    assert verts_q.shape == (256, 2) and faces.shape == (450, 3)
    points = np.column_stack([verts_q / 1e6, np.zeros(len(verts_q))])
    classes = osn.quad_classes(quad, [(i // 4 + 2 * (j // 4)) % 3 for j in range(15) for i in range(15)])
    cams = synthetic.camera_set_from_poses([synthetic.nadir_pose(7.5, 7.5, 20.0), synthetic.nadir_pose(6.0, 8.0, 16.0, yaw_deg=30.0)],
                                           30.0, 32, 32)
    recs = cams.get_raster_records(1.0, near=0.05)
    ids = np.stack([oracle_c.raster(points, faces.astype(np.int32), recs[v], 32, 32) for v in range(2)])
    assert (ids >= 0).sum() > 1000
    return dict(verts_q=verts_q, faces=faces.astype(np.int32), classes=classes, points=points, recs=recs, ids=ids)


@pytest.fixture(scope="module")
def rays():
    """96 rays from 4 images, their edges at 4.0 by the stand-in, and the tolerance of tests/test_ray_pairs.py for distances."""
    s = synthetic.detection_survey(n_objects=48, n_cameras=4, seed=1)
    starts, ends, ids = s["ray_starts"][:96], s["ray_ends"][:96], s["ray_IDs"][:96]
    assert len(ids) == 96 and len(np.unique(ids)) == 4
    want = ray_pair_edges_np(starts, ends, ids, 4.0)
    assert len(want[0]) > 50
    with np.load(GOLDEN / "reference_triangulation.npz", allow_pickle=False) as d:
        tol = 8 * float(d["a__e_ref"])
    return dict(args=(starts, ends, ids, 4.0), want=want, tol=tol)


def _check_rays(got, rays):
    got, want = [_np(x) for x in got], rays["want"]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.abs(got[2] - want[2]).max() <= rays["tol"]


@pytest.fixture(scope="module")
def tiny(ctx, mesh):
    """The small resize and the point bounds, first on the fresh context: what every later repeat must reproduce bit for bit."""
    image = resize_image_values(np.random.default_rng(5), (48, 64, 3), "float64")
    resized = _np(ctx.resize_image(image, (12, 16)))
    _close(resized, oracle_resize.resize_antialias(image, (12, 16)))
    bounds, bad = (_np(x) for x in ctx.points_bounds(mesh["points"]))
    want_b, want_bad = points_bounds_np(mesh["points"], 1)
    assert np.array_equal(bounds, want_b) and int(bad[0]) == want_bad == 0
    return dict(image=image, resized=resized, bounds=bounds)


def _tiny_again(ctx, mesh, tiny):
    _same_bits(ctx.resize_image(tiny["image"], (12, 16)), tiny["resized"])
    bounds, bad = (_np(x) for x in ctx.points_bounds(mesh["points"]))
    assert np.array_equal(bounds, tiny["bounds"]) and int(bad[0]) == 0


def _raster_equals_oracle(ctx, mesh):
    ctx.upload_mesh(mesh["points"].astype(np.float32), mesh["faces"])
    assert np.array_equal(_np(ctx.raster_face_ids(mesh["recs"], 32, 32)), mesh["ids"])


def test_stages_share_the_arena_in_turn(ctx, mesh, rays, tiny):
    _raster_equals_oracle(ctx, mesh)
    _tiny_again(ctx, mesh, tiny)                                                                     # resize_image (and points_bounds)
    A = setcover_standin.random_incidence(200, 12, 0.5, 2)
    want_cover = setcover_standin.set_cover(A, 1, True)
    assert len(want_cover["pruned"]) == 1
    same_cover(device_cover(ctx, A, 1, True), want_cover)                                            # set_cover
    outlines = same_outlines(ctx, mesh["verts_q"], mesh["faces"], mesh["classes"], 3)                # class_outlines
    assert outlines["n_rings"] >= 3
    ctx.set_option(_hip.GR_OPT_DEBUG, _hip.GR_DBG_POISON_RAYS)
    try:
        # ray_pair_edges: the whole arena is 0xFF now
        _check_rays(ctx.ray_pair_edges(*rays["args"]), rays)
    finally:
        ctx.set_option(_hip.GR_OPT_DEBUG, 0)
    cls = np.random.default_rng(9).integers(0, 5, mesh["ids"].shape).astype(np.float64)              # project_index_pairs (gr_count_pairs)
    cls[np.random.default_rng(10).random(cls.shape) < 0.2] = np.nan
    want_pc, want_keys, want_mult = _index_oracle(mesh["ids"], cls, 450, 5, True)
    pc = torch.zeros((450,), dtype=torch.int32, device=ctx.device)
    keys, mult = ctx.project_index_pairs(mesh["ids"], cls, 5, pc)
    assert np.array_equal(keys, want_keys) and np.array_equal(mult, want_mult) and np.array_equal(_np(pc), want_pc)
    table = PlanarPolygons([vs.square(3.25, 2.5, 9.75, 11.0)], [0], [False]).snapped()               # points_in_region + submesh_extract
    want_mask, info = points_in_region_np(mesh["verts_q"], table, REGION_D)
    assert 0 < want_mask.sum() < len(want_mask)
    mask, stats = device_region(ctx, mesh["verts_q"], table, REGION_D)
    assert np.array_equal(mask, want_mask) and np.array_equal(stats, info["stats"])
    same_submesh(device_submesh(ctx, mask, mesh["faces"]), want_mask, mesh["faces"])
    bounds, bad = (_np(x) for x in ctx.points_bounds(mesh["points"]))                                # points_bounds
    assert np.array_equal(bounds, tiny["bounds"]) and int(bad[0]) == 0
    _raster_equals_oracle(ctx, mesh)                                                                 # upload_mesh again
    _tiny_again(ctx, mesh, tiny)                                                                     # the same resize_image again


def test_large_then_small(ctx, mesh, tiny):
    A = setcover_standin.random_incidence(65536, 64, 0.25, 5)
    assert A.nnz == 1 << 20
    same_cover(device_cover(ctx, A, 1, True), setcover_standin.set_cover(A, 1, True))
    _tiny_again(ctx, mesh, tiny)


def test_two_streams(ctx, rays):
    """Stream A resizes a 2048 x 2048 x 3 image: its row pass leaves 50 MB of doubles in the arena for the column pass, and the
    call returns without waiting.  Stream B then poisons the whole arena (gr_ray_pairs under GR_DBG_POISON_RAYS).  The arena
    holds only doubles for the resize: a wrong order of the two would show as NaN pixels, never as an index out of range."""
    image = torch.from_numpy(np.random.default_rng(21).normal(0.0, 1.0, (2048, 2048, 3))).to(ctx.device)
    alone = _np(ctx.resize_image(image, (512, 512)))
    assert np.isfinite(alone).all()
    torch.cuda.synchronize()
    # nothing on the host between the two calls but the second call itself
    on_device = ctx._ray_inputs(*rays["args"][:3])
    a, b = (torch.cuda.Stream(device=ctx.device) for _ in range(2))
    ctx.set_option(_hip.GR_OPT_DEBUG, _hip.GR_DBG_POISON_RAYS)
    try:
        with torch.cuda.stream(a):
            resized = ctx.resize_image(image, (512, 512))
        with torch.cuda.stream(b):
            edges = ctx.ray_pair_edges(*on_device, rays["args"][3])
        a.synchronize()
        b.synchronize()
    finally:
        ctx.set_option(_hip.GR_OPT_DEBUG, 0)
    _same_bits(resized, alone)
    _check_rays(edges, rays)
