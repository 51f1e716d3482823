"""-m gpu: GR_OPT_VERTEX_ORDER = 1 (vertex_order="gl") through the scenes that pin rule R1 at the raster path's
edges (tests/raster_scenes.py, shared with tests/test_hip_parity.py) and through the rounding-tie, fused-multiply-add and
guard-band scenes of tests/test_oracle_raster.py, whose expected pictures the Python restatement there confirms.  Everything is
bit-exact against `oracle_c.raster(..., vertex_order="gl")`: ids, and depth bits where the R1 test checks depth.  Every test
that switches the order restores "r1" in a `finally`: a leaked "gl" would corrupt every later raster test of the session."""
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from geograypher_amd import _hip
from geograypher_amd.utils import synthetic
from oracle import oracle_c, oracle_np
from tests import raster_scenes

pytestmark = pytest.mark.gpu

# the settings that consume snapped vertices differently (tests/test_hip_parity.py VARIANTS explains the words): (tile height
# log2, slots per tile, GR_OPT_VARIANT)
VARIANTS = {"default": (5, 512, 0),
            "exact_binning": (5, 0, _hip.GR_VAR_ONE_TILE + _hip.GR_VAR_VOTES_INLINE),
            "tile64_ent48_general_ids": (6, 512, _hip.GR_VAR_ONE_TILE + _hip.GR_VAR_ENT48 + _hip.GR_VAR_GENERAL_IDS),
            "micro_always": (5, 512, _hip.GR_VAR_CHAINS + _hip.GR_VAR_MICRO_ALWAYS),
            "no_look_packed_counters": (5, 512, _hip.GR_VAR_CHAINS + _hip.GR_VAR_NO_LOOK + _hip.GR_VAR_PACKED_COUNTERS)}


@pytest.fixture(params=list(VARIANTS), autouse=True)
def raster_variant(request, hip):
    thl, cap, var = VARIANTS[request.param]
    hip.set_option(_hip.GR_OPT_TILE_H_LOG2, thl)
    hip.set_option(_hip.GR_OPT_DIRECT_CAP, cap)
    hip.set_option(_hip.GR_OPT_VARIANT, var)
    yield request.param
    hip.set_option(_hip.GR_OPT_TILE_H_LOG2, 5)
    hip.set_option(_hip.GR_OPT_DIRECT_CAP, 512)
    hip.set_option(_hip.GR_OPT_VARIANT, 0)


@contextmanager
def gl_order(hip):
    hip.set_vertex_order("gl")
    try:
        yield
    finally:
        hip.set_vertex_order("r1")


_ORACLE = {}   # scene key -> the oracle's GL pictures, computed once for all variants and never changed


def _oracle_gl(key, points, faces, recs, h, w, depth):
    if key not in _ORACLE:
        out = [oracle_c.raster(points, faces, recs[v], h, w, want_depth=True, vertex_order="gl") if depth
               else (oracle_c.raster(points, faces, recs[v], h, w, vertex_order="gl"), None) for v in range(recs.shape[0])]
        for ids, dep in out:
            ids.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def _check_views_gl(hip, key, points, faces, recs, h, w, depth=False):
    """The device in GL order against the oracle in GL order; returns the device's ids."""
    want = _oracle_gl(key, points, faces, recs, h, w, depth)
    hip.upload_mesh(np.asarray(points, dtype=np.float32), np.asarray(faces, dtype=np.int32))
    with gl_order(hip):
        if depth:
            ids, dep = hip.raster_face_ids(recs, h, w, want_depth=True)
            dep = dep.cpu().numpy()
        else:
            ids = hip.raster_face_ids(recs, h, w)
    ids = ids.cpu().numpy()
    for v in range(recs.shape[0]):
        bad = np.argwhere(ids[v] != want[v][0])
        assert bad.size == 0, f"view {v}: {bad.shape[0]} pixels differ, first {bad[:5].tolist()}"
        if depth:
            np.testing.assert_array_equal(dep[v].view(np.int32), want[v][1].view(np.int32), err_msg=f"depth view {v}")
    return ids


SIZES_2T = [(64, 64), (64, 128), (128, 64)]   # one tile; two tiles in a row (P_x != -P_y); two in a column


@pytest.mark.parametrize("size", SIZES_2T, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rounding_ties_snap_half_to_even(hip, size):
    """raster_scenes.tie_scene (tests/test_oracle_raster.py proves that floor(x + 0.5) draws another picture of it)."""
    h, w = size
    points, faces, recs = raster_scenes.tie_scene(h, w)
    ids = _check_views_gl(hip, ("tie", size), points, faces, recs, h, w, depth=True)
    assert len(np.unique(ids)) == faces.shape[0] + 1


def test_viewport_multiply_add_is_fused(hip):
    """raster_scenes.fma_scene: the one fused operation of snap_vertex, on a coordinate where unfusing it moves the vertex."""
    points, faces, recs = raster_scenes.fma_scene()
    _check_views_gl(hip, "fma", points, faces, recs, 6, 6, depth=True)


@pytest.mark.parametrize("size", SIZES_2T, ids=lambda s: f"{s[0]}x{s[1]}")
def test_guard_band_on_the_window_coordinate(hip, size):
    """raster_scenes.guard_scene: valid within |win| < 16384, clipped (k_clip_faces, planes in window terms) from there on."""
    h, w = size
    points, faces, recs = raster_scenes.guard_scene(h, w)
    ids = _check_views_gl(hip, ("guard", size), points, faces, recs, h, w, depth=True)
    assert len(np.unique(ids)) == faces.shape[0]


@pytest.mark.parametrize("variant", [0, 128, 8192], ids=["entries40", "entries48", "micro_lists"])
def test_93_pixel_boundary(hip, variant):
    points, faces, rec, h, w = raster_scenes.boundary_93_scene()
    hip.set_option(_hip.GR_OPT_VARIANT, variant)
    try:
        _check_views_gl(hip, "93", points, faces, rec, h, w, depth=True)
    finally:
        hip.set_option(_hip.GR_OPT_VARIANT, 0)
        hip.set_option(_hip.GR_OPT_DIRECT_CAP, 512)


# (h, w) -> seed of the random-stress generator: odd sizes, no multiples of the tile, one pixel; the largest row flip and the
# largest X (a million pixels each).  Rendered at image_scale 0.37 of the photos, principal point at the window centre.
ODD_SIZES = {(1, 1): 1, (3, 70): 2, (65, 33): 2, (97, 131): 3, (251, 333): 6, (457, 613): 9, (8, 16384): 1, (16384, 8): 9}


@pytest.mark.parametrize("size", list(ODD_SIZES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_odd_and_extreme_sizes(hip, size):
    points, faces, recs, h, w = raster_scenes.random_stress_scene(ODD_SIZES[size], size=size, principal_point="center",
                                                                  image_scale=0.37)
    assert (h, w) == size and recs[0, 13] == w / 2 and recs[0, 14] == h / 2
    ids = _check_views_gl(hip, ("odd", size), points, faces, recs, h, w, depth=True)
    assert (ids >= 0).any()


def test_degenerate_soup_and_non_finite_vertices(hip):
    """Faces behind and across the camera plane, zero-area and coincident faces, NaN and +-inf vertices, with depth."""
    points, faces, cams = raster_scenes.degenerate_soup_scene(0)
    points, faces = raster_scenes.broken_vertices_scene(points, faces)
    recs = cams.get_raster_records(1.0, near=0.5)
    ids = _check_views_gl(hip, "soup", points, faces, recs, 251, 333, depth=True)
    assert len(np.unique(ids)) >= 3


def test_near_plane_and_guard_band(hip):
    """R7 behind the GL snap: the 1 km ground plane at the horizon, cameras inside the terrain, an oblique near plane."""
    pts, quad, cams = raster_scenes.ground_plane_scene()
    ids = _check_views_gl(hip, "ground", pts, quad, cams.get_raster_records(1.0, near=0.1), 240, 320, depth=True)
    assert (ids[0, 121:] >= 0).all() and (ids[0, :120] == -1).all()
    points, faces, cams = raster_scenes.cameras_inside_terrain()
    for near in (0.05, 0.7):
        ids = _check_views_gl(hip, ("terrain", near), points, faces, cams.get_raster_records(1.0, near=near), 251, 333, depth=True)
        assert (ids >= 0).mean() > 0.3


def test_tile_sized_faces(hip):
    points, faces, cams = raster_scenes.tile_sized_faces_scene(1.5)
    _check_views_gl(hip, "tile_sized", points, faces, cams.get_raster_records(1.0, near=0.05), 900, 1600)


@pytest.mark.parametrize("batch", [5, 64])
def test_more_views_than_a_launch_group(hip, batch):
    points, faces, cams = raster_scenes.many_views_scene()
    hip.set_option(_hip.GR_OPT_BATCH, batch)
    try:
        _check_views_gl(hip, "many_views", points, faces, cams.get_raster_records(1.0, near=0.05), 200, 320)
    finally:
        hip.set_option(_hip.GR_OPT_BATCH, 64)


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("C", [1, 7])
def test_fused_votes_in_gl_order(hip, compat, C):
    """gr_raster_project_labels_u8 with the ids returned: the ids are the oracle's GL ids, votes and counts are what oracle_np's
    project_image + aggregate make of them."""
    points, faces, cams = raster_scenes.many_views_scene(9)
    F, h, w = faces.shape[0], 200, 320
    recs = cams.get_raster_records(1.0, near=0.05)
    want = _oracle_gl("fused", points, faces, recs, h, w, False)
    labels = np.stack([synthetic.synthetic_labels(want[v][0], v, C) for v in range(len(want))])
    projections = [oracle_np.project_image(want[v][0].astype(np.int64), oracle_np.inds_to_one_hot(labels[v], C).astype(float), F,
                                           neg1_is_last_face=compat) for v in range(len(want))]
    _, info = oracle_np.aggregate(projections, F)
    hip.upload_mesh(points.astype(np.float32), faces.astype(np.int32))
    hip.set_option(_hip.GR_OPT_BATCH, 4)      # three launch groups
    votes, counts = hip.new_vote_buffers(C)
    ids = torch.empty((len(want), h, w), dtype=torch.int32, device=hip.device)
    try:
        with gl_order(hip):
            hip.raster_project_labels(recs, labels, C, votes, counts, ids_out=ids, neg1_is_last_face=compat)
    finally:
        hip.set_option(_hip.GR_OPT_BATCH, 64)
    np.testing.assert_array_equal(ids.cpu().numpy(), np.stack([x[0] for x in want]))
    np.testing.assert_array_equal(counts.cpu().numpy().view(np.uint32), info["projection_counts"].astype(np.uint32))
    np.testing.assert_array_equal(votes.cpu().numpy().view(np.uint32), np.nan_to_num(info["summed_projections"]).astype(np.uint32))
    assert info["projection_counts"].max() > 1


@pytest.mark.parametrize("look", [True, False])
def test_overflow_and_retry(hip, look, raster_variant):
    """80 slots per tile are too few for the C1 views (tests/test_overflow_protocol.py): with the look at the first launch group
    the library bins it again itself, with GR_VAR_NO_LOOK the status call reports the overflow and the caller retries.  The
    picture after the retry is the oracle's in GL order."""
    (points, faces), cams = synthetic.config1_scene()
    recs = cams.get_raster_records(1.0, near=0.05)
    var = VARIANTS[raster_variant][2] & ~_hip.GR_VAR_NO_LOOK
    hip.set_option(_hip.GR_OPT_VARIANT, var if look else var | _hip.GR_VAR_NO_LOOK)
    hip.set_option(_hip.GR_OPT_DIRECT_CAP, 80)       # forgets what the context learned
    try:
        _check_views_gl(hip, "c1", points, faces, recs, 480, 640, depth=True)
        retries, rebinned = hip.last_retries, hip.last_stats["rebinned_groups"]
        assert hip.last_stats["overflow"] == 0 and retries + rebinned >= 1      # the call was taught something, and finished
    finally:
        hip.set_option(_hip.GR_OPT_DIRECT_CAP, 512)


def test_the_switch_reaches_the_device(hip):
    """C1: GL and R1 ids differ somewhere, on the device as in the oracle."""
    (points, faces), cams = synthetic.config1_scene()
    recs = cams.get_raster_records(1.0, near=0.05)
    gl = _check_views_gl(hip, "c1", points, faces, recs, 480, 640, depth=True)
    r1 = hip.raster_face_ids(recs, 480, 640).cpu().numpy()
    np.testing.assert_array_equal(r1[0], oracle_c.raster(points, faces, recs[0], 480, 640))
    assert (gl != r1).sum() > 0
