"""Every output the binding allocates, fenced and poisoned (tests/fenced_backend.py), at the smallest shapes where a tail can go
wrong: one element, one wave +- 1, one workgroup + 1, each stage's own staging unit + 1.

One `FencedHipRaster` for the module.  Every call runs inside `fenced(ctx)`; every returned array is compared with the stand-in
or oracle the stage's own GPU test uses, through that test's helper and with its exactness or tolerance -- the helpers are
imported from those modules, as tests/test_stage_scratch_gpu.py does.  Nothing is measured here.  What is new is the memory the
outputs live in:

  * the payload holds 0x7F bytes before the call, whatever an earlier call of the same shape left in the allocator's block: a
    store that is MISSING shows as a mismatch with the stand-in;
  * 4096 bytes of 0x7F lie on either side of the payload, the tail fence from the payload's last byte on: a store that lands
    OUTSIDE shows in `check_fences()` when the block ends.

uint8 outputs cannot tell 0x7F from a legal value: their inputs have fewer than 127 classes and nodata 255, asserted on the
stand-in's answer; the 0 / 1 flags the binding turns into bool are read as bytes (`payloads`) before they are.

`COVERED` names, per entry point of the binding that allocates an output (and those that write into buffers made by
`new_vote_buffers`), the tests here that run it; tests/test_fenced_backend_host.py fails for an entry point in neither `COVERED`
nor `EXEMPT`.  The last two tests make the capped grids of `gr_sample_raster` and `gr_set_cover` take a second pass of their
grid-stride loops."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))   # the stand-ins import one another by their plain names

import decimate_standin as ds  # noqa: E402
import equirect_standin  # noqa: E402
import member_outline_standin as msn  # noqa: E402
import outline_standin as osn  # noqa: E402
import polygon_standin as ps  # noqa: E402
import raster_standin as rs  # noqa: E402
import vector_standin as vs  # noqa: E402
from region_standin import points_in_region_np  # noqa: E402

from geograypher_amd import _hip  # noqa: E402
from geograypher_amd.utils import synthetic  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons  # noqa: E402
from geograypher_amd.utils.raster import PlanarRaster  # noqa: E402
from oracle import oracle_c, oracle_np, oracle_warp  # noqa: E402
from tests import image_edge_cases as cases  # noqa: E402
from tests import setcover_standin  # noqa: E402
from tests import test_covering_meshes_gpu as t_cover  # noqa: E402
from tests import test_equirect_gpu as t_equi  # noqa: E402
from tests import test_height_above_ground_gpu as t_terrain  # noqa: E402
from tests import test_image_selection_gpu as t_select  # noqa: E402
from tests import test_image_stage_edges as t_image  # noqa: E402
from tests import test_mesh_decimation_gpu as t_decim  # noqa: E402
from tests import test_mesh_upload_gpu as t_upload  # noqa: E402
from tests import test_ortho_assemble_gpu as t_ortho  # noqa: E402
from tests import test_polygon_weights_edges as t_poly  # noqa: E402
from tests import test_region_pairs as t_region  # noqa: E402
from tests import test_reproject_gpu as t_crs  # noqa: E402
from tests import test_stage_edges as t_stage  # noqa: E402
from tests import test_zonal_counts_gpu as t_zonal  # noqa: E402
from tests.conftest import GOLDEN  # noqa: E402
from tests.fenced_backend import POISON, FencedHipRaster, fenced  # noqa: E402
from tests.ray_standin import clip_rays_np, ray_pair_edges_np  # noqa: E402
from tests.test_detection_footprints_gpu import same as same_members  # noqa: E402
from tests.test_face_outlines_gpu import same as same_outlines  # noqa: E402
from tests.test_hip_parity import _check_views  # noqa: E402
from tests.test_ray_pairs import _standin_tol  # noqa: E402
from tests.test_roi_crop_gpu import device_region, device_submesh, same_submesh  # noqa: E402
from tests.test_vector_texture_gpu import device_index  # noqa: E402

pytestmark = pytest.mark.gpu

COVERED = {
    "raster_face_ids": ["test_raster_face_ids"],
    "raster_project_labels": ["test_raster_project_labels"],
    "new_vote_buffers": ["test_raster_project_labels", "test_projection_stages"],
    "debug_upload": ["test_debug_upload"],
    "debug_stage": ["test_debug_stage"],
    "gather_texture": ["test_projection_stages"],
    "gather_texture_u8": ["test_projection_stages"],
    "project_view": ["test_projection_stages"],
    "project_labels": ["test_projection_stages"],
    "project_values": ["test_projection_stages"],
    "finalize_votes": ["test_projection_stages"],
    "finalize_sums": ["test_projection_stages"],
    "argmax_nonzero": ["test_projection_stages"],
    "project_index_pairs": ["test_projection_stages", "test_pair_paths"],
    "PairAccumulator.add": ["test_pair_paths"],
    "PairAccumulator.add_rects": ["test_pair_paths"],
    "PairAccumulator.add_polygons": ["test_pair_paths"],
    "PairAccumulator.finish": ["test_pair_paths"],
    "resize_image": ["test_resize_image"],
    "warp_image": ["test_warp_image"],
    "invert_distortion": ["test_invert_distortion"],
    "equirect_view": ["test_equirect_view"],
    "ray_pair_edges": ["test_ray_pairs"],
    "ray_pair_count": ["test_ray_pairs"],
    "clip_rays": ["test_clip_rays"],
    "points_bounds": ["test_cover_bounds_and_grid"],
    "cover_grid": ["test_cover_bounds_and_grid"],
    "set_cover": ["test_set_cover", "test_set_cover_second_pass_of_the_capped_grids"],
    "polygon_class_weights": ["test_polygon_class_weights_on_the_grid", "test_polygon_class_weights"],
    "face_polygon_index": ["test_face_polygon_index"],
    "points_in_region": ["test_region_and_submesh"],
    "submesh_extract": ["test_region_and_submesh"],
    "class_outlines": ["test_class_outlines"],
    "member_outlines": ["test_member_outlines"],
    "cluster_count": ["test_cluster_count_and_decimate"],
    "cluster_decimate": ["test_cluster_count_and_decimate"],
    "sample_raster": ["test_sample_raster", "test_sample_raster_second_pass_of_the_capped_grid"],
    "reproject_points": ["test_reproject_points"],
    "assemble_tiles": ["test_assemble_tiles"],
    "zonal_class_counts": ["test_zonal_class_counts"],
}

# an entry point the walk of the host test picks up although none of its outputs is written by a kernel into memory the binding
# allocated: name -> the one-line reason (empty: every allocating entry point has its case above)
EXEMPT = {}

SIZES = (1, 65, 257)


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def ctx():
    backend = FencedHipRaster(0)
    yield backend
    backend.close()


def _on_device(ctx, array):
    """(device tensor, its clone): an input handed over on the device must come back bit for bit."""
    t = torch.as_tensor(np.ascontiguousarray(array)).to(ctx.device)
    return t, t.clone()


def _untouched(t, clone):
    assert torch.equal(t.reshape(-1).view(torch.uint8), clone.reshape(-1).view(torch.uint8)), "a device input was written"


def _flags_are_bytes_0_1(ctx):
    """The uint8 outputs of the calls of this block hold 0 or 1 (`selected`, the region mask): no byte kept the poison."""
    flags = ctx.fences.payloads(torch.uint8)
    assert flags
    for p in flags:
        assert int(p.max()) <= 1, f"a flag byte of the {tuple(p.shape)} output is {int(p.max())}"


# ---- the raster path ----------------------------------------------------------------------------------------------------------
RASTER_HW = [(1, 1), (31, 63), (32, 64), (33, 65), (65, 129)]


@pytest.fixture(scope="module")
def grid():
    """The 450-face grid mesh of tests/test_stage_scratch_gpu.py with its face classes, never written to."""
    verts_q, faces, quad = osn.grid_mesh(15, 15)
    assert verts_q.shape == (256, 2) and faces.shape == (450, 3)
    points = np.column_stack([verts_q / 1e6, np.zeros(len(verts_q))])
    classes = osn.quad_classes(quad, [(i // 4 + 2 * (j // 4)) % 3 for j in range(15) for i in range(15)])
    faces = faces.astype(np.int32)
    for a in (verts_q, faces, points):
        a.setflags(write=False)
    return dict(verts_q=verts_q, faces=faces, classes=np.asarray(classes, dtype=np.int32), points=points)


def _records(h, w, n):
    """n views of (h, w) from the two nadir poses of tests/test_stage_scratch_gpu.py in turn, the focal length scaled with the
    image so that every size sees the mesh and some background."""
    poses = [synthetic.nadir_pose(7.5, 7.5, 20.0), synthetic.nadir_pose(6.0, 8.0, 16.0, yaw_deg=30.0)]
    cams = synthetic.camera_set_from_poses([poses[k % 2] for k in range(n)], 30.0 * min(h, w) / 32.0, w, h)
    return cams.get_raster_records(1.0, near=0.05)


@pytest.mark.parametrize("depth", [False, True], ids=["ids", "ids_depth"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", RASTER_HW, ids=lambda s: f"{s[0]}x{s[1]}")
def test_raster_face_ids(ctx, grid, hw, n, depth):
    h, w = hw
    with fenced(ctx):
        ids = _check_views(ctx, np.array(grid["points"]), np.array(grid["faces"]), _records(h, w, n), h, w, depth=depth)
    assert (ids >= 0).any() and (h * w == 1 or (ids == -1).any())


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", RASTER_HW, ids=lambda s: f"{s[0]}x{s[1]}")
def test_raster_project_labels(ctx, grid, hw, n):
    h, w = hw
    points, faces = np.array(grid["points"]), np.array(grid["faces"])
    F, C = len(faces), 3
    recs = _records(h, w, n)
    want_ids = np.stack([oracle_c.raster(points, faces, recs[v], h, w) for v in range(n)])
    labels = np.stack([synthetic.synthetic_labels(want_ids[v], v, C) for v in range(n)])
    want_v, want_c = np.zeros((F, C), dtype=np.uint32), np.zeros(F, dtype=np.uint32)
    for v in range(n):
        oracle_c.project_labels(want_ids[v], labels[v], F, C, want_v, want_c)
    ctx.upload_mesh(points.astype(np.float32), faces)
    with fenced(ctx):
        votes, counts = ctx.new_vote_buffers(C)
        ids_out = ctx._empty((n, h, w), torch.int32)
        lab_t, lab_clone = _on_device(ctx, labels)
        ctx.raster_project_labels(recs, lab_t, C, votes, counts, ids_out=ids_out)
        np.testing.assert_array_equal(_np(ids_out), want_ids)
        np.testing.assert_array_equal(_np(votes).view(np.uint32), want_v)
        np.testing.assert_array_equal(_np(counts).view(np.uint32), want_c)
        _untouched(lab_t, lab_clone)
        # without the ids: the winners stay in the rasterizer's tiles
        v2, c2 = ctx.new_vote_buffers(C)
        ctx.raster_project_labels(recs, labels, C, v2, c2)
        np.testing.assert_array_equal(_np(v2).view(np.uint32), want_v)
        np.testing.assert_array_equal(_np(c2).view(np.uint32), want_c)


@pytest.mark.parametrize("name", ["soup_F2", "grid_F257"])
def test_debug_upload(ctx, name):
    verts, faces = t_upload.CASES[name]
    want = t_upload._standin(name)
    ctx.upload_mesh(verts, faces)
    with fenced(ctx):
        got = t_upload._read(ctx)
        t_upload._assert_properties(got, verts, faces)
        t_upload._assert_same_products(got, want, want["counts"])


@pytest.mark.parametrize("n", SIZES)
def test_debug_stage(ctx, grid, n):
    """gr_debug_read_stage copies exactly n bytes.  The stage scratch is filled with 0xFF first (GR_DBG_POISON_STAGE, under
    gr_points_bounds, which plans 65 536 bytes and writes one record at their front), so every byte of the copy differs from the
    poison of the output buffer."""
    ctx.set_option(_hip.GR_OPT_DEBUG, _hip.GR_DBG_POISON_STAGE)
    try:
        ctx.points_bounds(np.array(grid["points"]))
    finally:
        ctx.set_option(_hip.GR_OPT_DEBUG, 0)
    with fenced(ctx):
        tail, size = ctx.debug_stage(0, -n, n)
        assert size >= 65536 and tail.shape == (n,) and bool((tail == 0xFF).all())
        front, _ = ctx.debug_stage(0, 4096, n)   # behind the one record, inside the plan
        assert bool((front == 0xFF).all())


# ---- the kernels behind the rasterizer ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (7, 37)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("F", [1, 255, 257])
def test_projection_stages(ctx, F, C, hw):
    h, w = hw
    rng = np.random.default_rng(F * 1009 + C * 31 + h)
    n = 2
    ids = t_stage._ids(rng, n, h, w, F)
    ids[:, -1, -1] = F - 1                       # the last face wins the last pixel of every view
    img = rng.normal(0, 1, (n, h, w, C))
    img[rng.random(img.shape) < 0.05] = np.nan
    tex = rng.uniform(0.0, 100.0, (F, C))        # uint8 gather: every value below the poison's 127, the null value 255
    tex[rng.random(tex.shape) < 0.1] = np.nan
    labels = rng.integers(0, C + 2, (n, h, w)).astype(np.uint8)
    labels[rng.random(labels.shape) < 0.05] = 255
    cls = rng.integers(0, 5, (n, h, w)).astype(np.float64)
    cls[rng.random(cls.shape) < 0.2] = np.nan
    projs = [oracle_np.project_image(ids[v].astype(np.int64), img[v], F) for v in range(n)]
    want_avg, want_sum, want_cnt = t_stage._want_sums(projs, F)
    lab_projs = [oracle_np.project_image(ids[v].astype(np.int64), t_stage._one_hot(labels[v], C), F) for v in range(n)]
    want_lavg, want_lsum, want_lcnt = t_stage._want_sums(lab_projs, F)
    want_pc, want_keys, want_mult = t_stage._index_oracle(ids, cls, F, 5, True)
    want_tex = oracle_np.render_flat_gather(ids[0].astype(np.int64), tex)
    want_u8 = oracle_np.render_postprocess_uint8(want_tex, null_value=255)
    assert POISON not in want_u8 and (h * w == 1 or (want_u8 == 255).any())
    t_stage._mesh(ctx, F)
    with fenced(ctx):
        ids_t, ids_clone = _on_device(ctx, ids)
        t_stage._same(_np(ctx.gather_texture(ids_t[0], tex)), want_tex)
        got_u8 = _np(ctx.gather_texture_u8(ids_t[0], tex, null_value=255))
        assert got_u8.dtype == np.uint8
        np.testing.assert_array_equal(got_u8, want_u8.reshape(got_u8.shape))
        for v in range(n):
            t_stage._same(_np(ctx.project_view(ids_t[v], img[v])), projs[v])
        sums, cnt = ctx._zeros((F, C), torch.float64), ctx._zeros((F,), torch.int32)
        ctx.project_values(ids_t, img, sums, cnt)
        avg, summed, counts = (_np(t) for t in ctx.finalize_sums(sums, cnt))
        t_stage._same(summed, want_sum)
        t_stage._same(avg, want_avg)
        t_stage._same(counts, want_cnt)
        votes, vc = ctx.new_vote_buffers(C)
        ctx.project_labels(ids_t, labels, C, votes, vc)
        lavg, lsum, lcnt = (_np(t) for t in ctx.finalize_votes(votes, vc))
        t_stage._same(lsum, want_lsum)
        t_stage._same(lavg, want_lavg)
        t_stage._same(lcnt, want_lcnt)
        pc = ctx._zeros((F,), torch.int32)
        keys, mult = ctx.project_index_pairs(ids_t, cls, 5, pc)
        assert np.array_equal(keys, want_keys) and np.array_equal(mult, want_mult) and np.array_equal(_np(pc), want_pc)
        rows = t_stage._argmax_rows(rng, C, F) if F >= 32 else rng.integers(-3, 4, (F, C)) * 0.1
        rows_t, rows_clone = _on_device(ctx, rows)
        t_stage._argmax_check(ctx, rows_t)
        t_stage._argmax_check(ctx, rows.astype(np.float32))
        _untouched(ids_t, ids_clone)
        _untouched(rows_t, rows_clone)


@pytest.mark.parametrize("nc", [1, 5])
def test_pair_paths(ctx, nc):
    """One view of 7 x 37 over 257 degenerate faces: the class-index image, the same classes as rectangles in paint order, and
    polygon rings, through `project_index_pairs` and the accumulator's `add`, `add_rects`, `add_polygons` and `finish`."""
    rng = np.random.default_rng(40 + nc)
    F, h, w = 257, 7, 37
    ids = t_stage._ids(rng, 1, h, w, F)
    ids[0, -1, -1] = F - 1
    cls = rng.integers(0, nc, (1, h, w)).astype(np.float64)
    cls[rng.random(cls.shape) < 0.2] = np.nan
    want_pc, want_keys, want_mult = t_stage._index_oracle(ids, cls, F, nc, True)
    rects, painted = [], np.full((1, h, w), np.nan)
    for _ in range(9):
        i0, j0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        i1, j1 = min(h, i0 + int(rng.integers(1, 5))), min(w, j0 + int(rng.integers(1, 12)))
        rects.append((i0, j0, i1, j1, int(rng.integers(0, nc))))
        painted[0, i0:i1, j0:j1] = rects[-1][4]      # in paint order: a later rectangle overwrites an earlier one
    rects = np.array(rects, dtype=np.int32)
    rect_pc, rect_keys, rect_mult = t_stage._index_oracle(ids, painted, F, nc, True)
    rings = [(k % nc, np.array(v, dtype=np.float64)) for k, v in enumerate((
        [(0.2, 1.3), (6.4, 2.1), (5.7, 14.6), (0.9, 11.2)], [(1.5, 8.5), (6.5, 20.5), (2.5, 30.5)],
        [(0.0, 25.0), (7.0, 25.0), (7.0, 37.0), (0.0, 37.0)], [(3.1, 0.2), (6.9, 0.4), (6.2, 36.3), (3.6, 35.1)],
        [(2.2, 16.8), (4.8, 17.1), (3.4, 22.9)]))]
    table = t_region._table(rings, h, w)
    (boxes, vert_offsets, verts), _ = table
    assert len(boxes) == 5
    ring_sum, ring_cnt = t_region._expected(ids.astype(np.int64), [t_region._mask(table, nc)], F, nc, True)
    assert ring_cnt.sum() > 20 and (nc == 1 or (ring_sum > 0).sum(axis=1).max() > 1)

    def dense(keys, mult):
        out = np.zeros(F * nc, dtype=np.int64)
        out[keys] = mult
        return out.reshape(F, nc)

    t_stage._mesh(ctx, F)
    with fenced(ctx):
        ids_t, ids_clone = _on_device(ctx, ids)
        cls_t, cls_clone = _on_device(ctx, cls)
        pc = ctx._zeros((F,), torch.int32)
        keys, mult = ctx.project_index_pairs(ids_t, cls_t, nc, pc)
        assert np.array_equal(keys, want_keys) and np.array_equal(mult, want_mult) and np.array_equal(_np(pc), want_pc)
        pc = ctx._zeros((F,), torch.int32)
        acc = ctx.new_pair_accumulator(nc, pc)
        acc.add(ids_t, cls_t)
        keys, mult = acc.finish()
        assert keys.dtype == np.int64 and mult.dtype == np.int64
        assert np.array_equal(keys, want_keys) and np.array_equal(mult, want_mult) and np.array_equal(_np(pc), want_pc)
        pc = ctx._zeros((F,), torch.int32)
        acc = ctx.new_pair_accumulator(nc, pc, cap=F)      # the smallest buffer that holds one view
        acc.add_rects(ids_t, rects, np.array([0, len(rects)]))
        keys, mult = acc.finish()
        assert np.array_equal(keys, rect_keys) and np.array_equal(mult, rect_mult) and np.array_equal(_np(pc), rect_pc)
        pc = ctx._zeros((F,), torch.int32)
        acc = ctx.new_pair_accumulator(nc, pc)
        acc.add_polygons(ids_t, boxes, vert_offsets, verts, np.array([0, len(boxes)]))
        keys, mult = acc.finish()
        np.testing.assert_array_equal(dense(keys, mult), ring_sum)
        np.testing.assert_array_equal(_np(pc), ring_cnt)
        _untouched(ids_t, ids_clone)
        _untouched(cls_t, cls_clone)


# ---- the image stages ---------------------------------------------------------------------------------------------------------
IMAGE_OUT = [(1, 1), (3, 2), (37, 53)]


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("hw_out", IMAGE_OUT, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resize_image(ctx, hw_out, C):
    rng = np.random.default_rng(hw_out[0] * 100 + hw_out[1] + C)
    with fenced(ctx):
        t_image._check_resize(ctx, (48, 64), hw_out, C, rng)
        raw = cases.resize_image_values(rng, (48, 64, C), "float32")
        raw_t, raw_clone = _on_device(ctx, raw)
        t_image._close(_np(ctx.resize_image(raw_t, hw_out)), t_image._resize_want(raw, hw_out, False))
        _untouched(raw_t, raw_clone)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("hw_out", IMAGE_OUT, ids=lambda s: f"{s[0]}x{s[1]}")
def test_warp_image(ctx, hw_out, C):
    rng = np.random.default_rng(hw_out[0] * 977 + hw_out[1] + C)
    in_shape = (6, 9)
    m = cases.random_map(rng, *in_shape, *hw_out, quarters_only=True)
    ids = rng.integers(-5, 200, in_shape + (C,)).astype(np.int32)
    img = ids.astype(np.float64)
    with fenced(ctx):
        mt = ctx.upload_map(m)
        mt_clone = mt.clone()
        t_image._same_bits(ctx.warp_image(ids, mt, order=0, fill_value=-1), oracle_warp.warp_total(ids, m, 0, -1))
        t_image._same_bits(ctx.warp_image(img, mt, order=0, fill_value=-1), np.squeeze(t_image._want_f64(img, m, 0, -1.0)))
        t_image._same_values(ctx.warp_image(img, mt, order=1, fill_value=-1), np.squeeze(t_image._want_f64(img, m, 1, -1.0)))
        _untouched(mt, mt_clone)


@pytest.mark.parametrize("hw", IMAGE_OUT, ids=lambda s: f"{s[0]}x{s[1]}")
def test_invert_distortion(ctx, hw):
    h, w = hw
    with fenced(ctx):
        for coeffs in ({}, cases.FULL_LENS):
            t_image._check_inverse(ctx, cases.lens(float(max(64, h, w)), w, h, cx=0.3, cy=-0.7, **coeffs), h, w, 1.0)


@pytest.fixture(scope="module")
def equirect_source():
    with np.load(GOLDEN / "reference_equirect.npz") as d:
        src = np.array(d["src_f64"])
    assert src.shape == (64, 128, 2) and src.dtype == np.float64
    return src


@pytest.mark.parametrize("oversample", [1, 2])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("hw_out", IMAGE_OUT, ids=lambda s: f"{s[0]}x{s[1]}")
def test_equirect_view(ctx, equirect_source, hw_out, C, oversample):
    """A float64 source (the output is float64 at either oversampling: no uint8 output here), the view, the sampling mask and
    the debug coordinates against the stand-in, by the rules of tests/test_equirect_gpu.py."""
    src = equirect_source[..., 0] if C == 1 else equirect_source[..., [0, 1, 0]]
    view = dict(fov_deg=80.0, output_size=hw_out, yaw_deg=200.0, pitch_deg=-35.0, roll_deg=20.0, warp_order=1,
                oversample_factor=oversample)
    want, wdbg = equirect_standin.perspective_from_equirectangular_np(src, **view, return_debug=True)
    _, vrange = equirect_standin.value_range(src)
    with fenced(ctx):
        dev, mask, dbg = t_equi._device_view(ctx, src, view, return_mask=True, return_debug=True)
        assert dev.shape == (hw_out if C == 1 else hw_out + (C,)) and dev.dtype == np.float64
        dev = np.squeeze(dev)      # the stand-in ends, like the reference, in np.squeeze: a 1 x 1 view loses its axes there
        assert dev.shape == want.shape
        assert dbg["ij"].shape == wdbg["ij"].shape and np.abs(dbg["ij"] - wdbg["ij"]).max() <= t_equi.COORD_ATOL
        assert np.abs(dev - want).max() <= 1e-8 * vrange
        t_equi._check_mask(f"{hw_out} C{C} os{oversample}", mask, wdbg["ij"], *src.shape[:2])


# ---- multiview detections -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def triangulation_gold():
    with np.load(GOLDEN / "reference_triangulation.npz", allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def survey():
    return synthetic.detection_survey()


@pytest.mark.parametrize("n", [2, 65, 257])
def test_ray_pairs(ctx, triangulation_gold, survey, n):
    """The rays of `test_launch_edges` (tests/test_ray_pairs.py), with no room offered, the exact room and the default."""
    starts, ends, ids = survey["ray_starts"][:n], survey["ray_ends"][:n], survey["ray_IDs"][:n]
    if n > 2:
        pick = np.arange(n) * (len(survey["ray_IDs"]) // n)
        starts, ends, ids = survey["ray_starts"][pick], survey["ray_ends"][pick], survey["ray_IDs"][pick]
    want = ray_pair_edges_np(starts, ends, ids, 4.0)
    total = len(want[0])
    assert n < 64 or total > 0
    with fenced(ctx):
        dev, clones = zip(*(_on_device(ctx, a) for a in (starts, ends, ids.astype(np.int32))))
        for cap, calls in ((None, 1), (0, 2 if total else 1), (total, 1)):
            got = [_np(x) for x in ctx.ray_pair_edges(*dev, 4.0, capacity=cap)]
            assert ctx.last_ray_pair_calls == calls
            assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float64
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            assert total == 0 or np.abs(got[2] - want[2]).max() <= _standin_tol(triangulation_gold)
        assert ctx.ray_pair_count(*dev, 4.0) == total
        for t, c in zip(dev, clones):
            _untouched(t, c)


@pytest.mark.parametrize("n_tri", [1, 129])
@pytest.mark.parametrize("n", [1, 257])
def test_clip_rays(ctx, triangulation_gold, n, n_tri):
    """The rays and the "floor" surface of the golden clip scene (tests/test_ray_pairs.py): the rays repeated with a lateral
    jitter to n, the surface cut to one triangle or grown to 129 by a copy half a unit below.  The reference is the stand-in
    in long double, as for the golden file, held to the golden test's bound: 4 times the error the float64 stand-in has
    against long double on this scene.  Rays within 1e-6 (barycentric) of an edge could take either triangle and are left
    out, as there; a ray that hits nothing keeps NaN."""
    gold = triangulation_gold
    rng = np.random.default_rng(n + n_tri)
    pick = np.arange(n) % len(gold["clip__origins"])
    origins, directions = gold["clip__origins"][pick].copy(), gold["clip__directions"][pick]
    origins[len(gold["clip__origins"]):, :2] += rng.uniform(-0.3, 0.3, (max(n - len(gold["clip__origins"]), 0), 2))
    points, faces = gold["clip__floor__points"], gold["clip__floor__faces"]
    if n_tri == 1:   # the first triangle that ray 0 hits: some rays hit it, most hit nothing
        faces = next(faces[k:k + 1] for k in range(len(faces)) if clip_rays_np(origins[:1], directions[:1], points, faces[k:k + 1])[0][0])
    else:
        below = points - np.array([0.0, 0.0, 0.5])
        faces = np.concatenate([faces, faces[:n_tri - len(faces)] + len(points)]).astype(np.int32)
        points = np.concatenate([points, below])
    assert len(faces) == n_tri
    hit_ld, t_ld, p_ld, margin = clip_rays_np(origins, directions, points, faces, dtype=np.longdouble)
    sure = ~hit_ld | (margin > 1e-6)
    assert sure.mean() > 0.9 and (n == 1 or (hit_ld.any() and (n_tri > 1 or not hit_ld.all())))
    with fenced(ctx):
        hit, t, pts = (_np(x) for x in ctx.clip_rays(origins, directions, points, faces))
    assert hit.dtype == bool and np.array_equal(hit[sure], hit_ld[sure])
    miss = sure & ~hit_ld
    assert np.isnan(t[miss]).all() and np.isnan(pts[miss]).all()
    ok = sure & hit_ld
    if ok.any():
        assert np.abs(t[ok].astype(np.longdouble) - t_ld[ok]).max() <= 4 * float(gold["clip__floor__e_t"])
        assert np.abs(pts[ok].astype(np.longdouble) - p_ld[ok]).max() <= 4 * float(gold["clip__floor__e_p"])


# ---- covering meshes, image selection -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("N", [2, 56, 57])
@pytest.mark.parametrize("V", [1, 4097])
def test_cover_bounds_and_grid(ctx, V, N, stride):
    rng = np.random.default_rng(V + N)
    pts = np.column_stack([rng.uniform(-50, 50, V), rng.uniform(0, 30, V), rng.normal(0, 5, V)])
    with fenced(ctx):
        t_cover._check(ctx, pts, N, stride=stride)
        pts_t, pts_clone = _on_device(ctx, pts)
        bounds, bad = (_np(x) for x in ctx.points_bounds(pts_t, stride))
        want_b, want_bad = t_cover.points_bounds_np(pts, stride)
        assert np.array_equal(bounds, want_b) and int(bad[0]) == want_bad
        _untouched(pts_t, pts_clone)


@pytest.mark.parametrize("prune", [True, False], ids=["prune", "no_prune"])
@pytest.mark.parametrize("n_views", [1, 65, 257])
def test_set_cover(ctx, n_views, prune):
    A = setcover_standin.random_incidence(300, n_views, 0.05, n_views)
    with fenced(ctx):
        t_select._check(ctx, A, 1, prune)      # through the LDS histograms and through global atomics
        _flags_are_bytes_0_1(ctx)


# the launch caps of csrc/select.hip, restated: `#define GR_SC_MAX_GRID 1024` (line 28: workgroups of the set-up kernels) and
# `#define GR_SC_MAX_WALK_GRID 512` (line 29: workgroups that walk one view's list), each of 256 lanes
SC_MAX_GRID, SC_MAX_WALK_GRID, SC_LANES = 1024, 512, 256


@pytest.fixture(scope="module")
def capped_cover():
    F = SC_MAX_GRID * SC_LANES + 257
    i = np.arange(F)
    lists = [i[(i >= F // 5) & (i < F - F // 5)], i[i < F // 2 + 1000], i[i >= F // 2 - 1000], i[::1000]]
    assert F == 262_401 and [len(x) for x in lists[:3]] == [157_441, 132_200, 132_201]
    assert all(len(x) > SC_MAX_WALK_GRID * SC_LANES for x in lists[:3]) and F > SC_MAX_GRID * SC_LANES
    return t_select._from_lists(F, lists)


@pytest.mark.parametrize("prune", [True, False], ids=["prune", "no_prune"])
@pytest.mark.parametrize("min_obs", [1, 2])
def test_set_cover_second_pass_of_the_capped_grids(ctx, capped_cover, min_obs, prune):
    """262 401 faces and three view lists beyond 512 x 256: the set-up kernels, the apply, prune-test and prune-apply walks and
    the covered count all go round their grid-stride loops a second time."""
    want = setcover_standin.set_cover(capped_cover, min_obs, prune)
    if min_obs == 1:
        assert want["order"].tolist() == [0, 1, 2] and want["gains"].tolist() == [157_441, 52_480, 52_480]
        assert want["pruned"].tolist() == ([0] if prune else [])
    else:
        assert want["order"].tolist() == [0, 3] and want["gains"].tolist() == [157_441, 106] and len(want["pruned"]) == 0
    with fenced(ctx):
        t_select._check(ctx, capped_cover, min_obs, prune, want=want)
        _flags_are_bytes_0_1(ctx)


# ---- polygons, regions, outlines ----------------------------------------------------------------------------------------------
REGION_D = 250_000   # a quarter of a grid cell, in grid steps (tests/test_stage_scratch_gpu.py)


@pytest.fixture(scope="module")
def region_table():
    return PlanarPolygons([vs.square(3.25, 2.5, 9.75, 11.0)], [0], [False]).snapped()


@pytest.mark.parametrize("within", [True, False], ids=["within", "overlay"])
@pytest.mark.parametrize("n_classes", [1, 3])
@pytest.mark.parametrize("n_faces", SIZES)
def test_polygon_class_weights(ctx, n_faces, n_classes, within):
    """The wave scene of tests/test_polygon_weights_edges.py (a face count of its own, rows without usable rings) against the
    exact oracle with that test's tolerance."""
    tri, cls, weight, table, info = ps.wave_scene(n_faces, n_classes)
    want, tol, _standin, stats = t_poly.answers(ps.wave_case(n_faces), cls, weight, n_classes, within)
    with fenced(ctx):
        tri_t, tri_clone = _on_device(ctx, tri)
        got, got_stats = t_poly.device(ctx, tri_t, cls, weight, table, n_classes, within)
        _untouched(tri_t, tri_clone)
    assert got.shape == (ps.WAVE_POLYGONS, n_classes)
    t_poly.check(f"fenced wave F={n_faces} C={n_classes}", "within" if within else "overlay", got, got_stats, want, tol, stats)
    assert np.all(got[info["no_usable_rings"]] == 0.0)


@pytest.fixture(scope="module")
def grid_polygons(grid):
    """Two polygon rows over the grid, the second with a hole, and per face count the exact case of tests/polygon_standin.py."""
    table = PlanarPolygons([vs.square(3.25, 2.5, 9.75, 11.0), vs.square(0.5, 0.5, 14.5, 6.2), vs.square(5.0, 1.0, 8.0, 4.0)],
                           [0, 1, 1], [False, False, True]).snapped()
    tri = grid["verts_q"][grid["faces"]].reshape(-1, 6).astype(np.int64)
    return {n: ps._case(tri[:n], table, {}) for n in SIZES + (450,)}


@pytest.mark.parametrize("within", [True, False], ids=["within", "overlay"])
@pytest.mark.parametrize("n_faces", SIZES + (450,))
def test_polygon_class_weights_on_the_grid(ctx, grid, grid_polygons, n_faces, within):
    case = grid_polygons[n_faces]
    cls = grid["classes"][:n_faces]
    weight = np.random.default_rng(n_faces).uniform(0.5, 2.0, n_faces)
    want, tol, _standin, stats = t_poly.answers(case, cls, weight, 3, within)
    assert n_faces < 450 or (want > 0).all()
    with fenced(ctx):
        got, got_stats = t_poly.device(ctx, case["tri"], cls, weight, case["table"], 3, within)
    assert got.shape == (2, 3)
    t_poly.check(f"fenced grid F={n_faces}", "within" if within else "overlay", got, got_stats, want, tol, stats)


@pytest.mark.parametrize("n_faces", SIZES + (450,))
def test_face_polygon_index(ctx, grid, region_table, n_faces):
    vq, faces = grid["verts_q"], grid["faces"][:n_faces]
    want, _ = vs.face_polygon_index_np(vq, faces, region_table)
    assert n_faces < 450 or 0 < (want >= 0).sum() < n_faces
    with fenced(ctx):
        got, stats = device_index(ctx, vq, faces, region_table)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert stats[1] == np.sum(want >= 0) and stats[3] == 0


@pytest.mark.parametrize("n", SIZES + (256,))
def test_region_and_submesh(ctx, grid, region_table, n):
    """n points of the grid (257: all of them and the first again) in the buffered square; then the sub-mesh that the mask of all
    256 vertices selects from the first n faces."""
    points_q = np.concatenate([grid["verts_q"], grid["verts_q"][:1]])[:n]
    want_mask, info = points_in_region_np(points_q, region_table, REGION_D)
    full_mask, _ = points_in_region_np(grid["verts_q"], region_table, REGION_D)
    assert 0 < full_mask.sum() < 256
    faces = grid["faces"][:n]
    with fenced(ctx):
        mask, stats = device_region(ctx, points_q, region_table, REGION_D)
        _flags_are_bytes_0_1(ctx)
        assert mask.dtype == bool and np.array_equal(mask, want_mask) and np.array_equal(stats, info["stats"])
        same_submesh(device_submesh(ctx, full_mask, faces), full_mask, faces)


def _cut(grid, n_faces):
    faces = grid["faces"][:n_faces]
    return grid["verts_q"], faces, grid["classes"][:n_faces]


@pytest.mark.parametrize("capacity", ["default", "none", "exact"])
@pytest.mark.parametrize("n_faces", SIZES + (450,))
def test_class_outlines(ctx, grid, n_faces, capacity):
    verts_q, faces, classes = _cut(grid, n_faces)
    E = osn.outlines_np(verts_q, faces, classes, 3)["n_edges"]
    kw = {"default": {}, "none": {"capacity": 0}, "exact": {"capacity": E}}[capacity]
    with fenced(ctx):
        want = same_outlines(ctx, verts_q, faces, classes, 3, **kw)
    assert want["n_edges"] == E > 0 and ctx.last_outline_calls == (2 if capacity == "none" else 1)


@pytest.mark.parametrize("capacity", ["default", "none", "exact"])
@pytest.mark.parametrize("n_faces", SIZES + (450,))
def test_member_outlines(ctx, grid, n_faces, capacity):
    verts_q, faces, classes = _cut(grid, n_faces)
    rows = [sorted({int(c), (int(c) + f % 2) % 3}) if f % 7 else [] for f, c in enumerate(classes)]
    rows[-1] = [0, 1, 2]
    face_ptr, face_members = msn.csr_of_rows(rows)
    E = msn.members_np(verts_q, faces, face_ptr, face_members, 3)["n_edges"]
    kw = {"default": {}, "none": {"capacity": 0}, "exact": {"capacity": E}}[capacity]
    with fenced(ctx):
        want = same_members(ctx, verts_q, faces, rows, 3, **kw)
    assert want["n_edges"] == E > 0 and ctx.last_outline_calls == (2 if capacity == "none" else 1)


# ---- decimation, raster samples, reprojection ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decimation_scene():
    verts_q, faces = ds.random_scene()
    for a in (verts_q, faces):
        a.setflags(write=False)
    return verts_q, faces


@pytest.mark.parametrize("s", [ds.RANDOM_S, 2 ** 30], ids=["random_s", "one_cell"])
@pytest.mark.parametrize("F", [0, 1, 257])
@pytest.mark.parametrize("V", SIZES)
def test_cluster_count_and_decimate(ctx, decimation_scene, V, F, s):
    verts_q, faces = decimation_scene
    rng = np.random.default_rng(V + F)
    prefix = np.array(faces[:F])
    beyond = prefix >= V
    prefix[beyond] = rng.integers(0, V, int(beyond.sum()))          # re-drawn inside the prefix
    with fenced(ctx):
        vq_t, vq_clone = _on_device(ctx, verts_q[:V])
        assert ctx.cluster_count(vq_t, s) == ds.cluster_count_py(verts_q[:V], s)
        t_decim.same_decimation(tuple(_np(a) for a in ctx.cluster_decimate(vq_t, prefix, s)), verts_q[:V], prefix, s)
        _untouched(vq_t, vq_clone)


@pytest.fixture(scope="module")
def terrain():
    points, faces, data, transform, nodata = rs.random_scene()
    for a in (points, faces):
        a.setflags(write=False)
    three = np.concatenate([data.reshape((1,) + data.shape[-2:]) * k for k in (1.0, 0.5, -2.0)]).astype(data.dtype)
    return points, faces, PlanarRaster(data, transform, nodata), PlanarRaster(three, transform, nodata)


@pytest.mark.parametrize("bands", [1, 3])
@pytest.mark.parametrize("vertex_mode", [False, True], ids=["faces", "vertices"])
@pytest.mark.parametrize("N", SIZES)
def test_sample_raster(ctx, terrain, N, vertex_mode, bands):
    points, faces, one, three = terrain
    raster = one if bands == 1 else three
    assert raster.data.shape[0] == bands
    points, faces = (points[-N:], None) if vertex_mode else (points, faces[-N:])
    NAN = np.nan
    with fenced(ctx):
        want = t_terrain.check_against_standin(ctx, points, faces, raster)
        assert want["values"].shape == (N, bands)
        call = lambda **kw: ctx.sample_raster(points, faces, raster.data, raster.inverse, raster.nodata, NAN, **kw)  # noqa: E731
        values, height, lab, stats = call(want_values=True, want_height=False)
        assert height is None and lab is None and t_terrain.same(_np(values), want["values"])
        assert _np(stats).tolist() == want["stats"].tolist()
        values, height, lab, stats = call(want_values=False, want_height=True)
        assert values is None and lab is None and t_terrain.same(_np(height), want["height"])
        assert _np(stats).tolist() == want["stats"].tolist()
        # relabel on a device tensor, in place
        start = np.where(np.arange(N) % 5 == 0, NAN, np.arange(N) % 4).astype(np.float64)
        relabel = rs.sample_raster_np(points, faces, raster.data, raster.inverse, raster.nodata, NAN, labels=start, threshold=2.0,
                                      ground_id=11.0)
        tensor = torch.as_tensor(start.reshape(-1, 1).copy()).to(ctx.device)
        pts_t, pts_clone = _on_device(ctx, points)
        _, _, got, stats = ctx.sample_raster(pts_t, faces, raster.data, raster.inverse, raster.nodata, NAN, want_values=False,
                                             labels=tensor, threshold=2.0, ground_id=11.0)
        assert got.data_ptr() == tensor.data_ptr() and t_terrain.same(_np(tensor)[:, 0], relabel["labels"])
        assert _np(stats).tolist() == relabel["stats"].tolist()
        _untouched(pts_t, pts_clone)


RS_MAX_GRID, RS_LANES = 8192, 256   # gr_sample_raster (csrc/terrain.hip) launches min(ceil(N / 256), 8192) workgroups of 256


@pytest.mark.parametrize("vertex_mode", [False, True], ids=["faces", "vertices"])
def test_sample_raster_second_pass_of_the_capped_grid(ctx, terrain, vertex_mode):
    """8192 x 256 + 257 queries drawn with replacement from the random scene: the last 257 are reached only by the second pass of
    the grid-stride loop, and hold every kind of query."""
    points, faces, raster, _ = terrain
    N = RS_MAX_GRID * RS_LANES + 257
    assert N == 2_097_409
    rng = np.random.default_rng(8192)
    if vertex_mode:
        points, faces = points[rng.integers(0, len(points), N)], None
    else:
        faces = faces[rng.integers(0, len(faces), N)]
    want = rs.sample_raster_np(points, faces, raster.data, raster.inverse, raster.nodata, np.nan)
    tail_in, tail_nodata = want["inside"][-257:], want["nodata_hit"][-257:]
    assert tail_in.any() and (~tail_in).any() and (tail_nodata & tail_in).any()
    with fenced(ctx):
        values, height, _, stats = t_terrain.device_sample(ctx, points, faces, raster, check=False)
    assert values.shape == (N, 1) and t_terrain.same(values, want["values"]) and t_terrain.same(height, want["height"])
    assert stats.tolist() == want["stats"].tolist() and len(stats) == 4


@pytest.fixture(scope="module")
def crs_golden():
    return t_crs.cs.load_golden()


@pytest.mark.parametrize("N", [1, 257])
def test_reproject_points(ctx, crs_golden, N):
    """Zone 10's golden ECEF rows -> UTM, tiled to N rows (`out=None`): point mode within the golden test's bound of the golden
    file, NaN exactly on its flagged rows; face mode the mean of the device's own vertex rows, bit for bit, as
    tests/test_reproject_gpu.py holds it."""
    cs, golden = t_crs.cs, crs_golden
    rows = np.nonzero(golden["group"] == 0)[0]
    idx = np.arange(N) % len(rows)
    base = np.ascontiguousarray(golden["in_ecef"][rows][idx])
    src, dst = cs.golden_crs(golden, "ecef", 0), cs.golden_crs(golden, "tm", 0)
    want, flag = golden["exp_ecef_tm"][rows][idx], golden["flag_ecef_tm"][rows][idx]
    faces = np.random.default_rng(N).integers(0, N, size=(N, 3)).astype(np.int32)
    with fenced(ctx):
        base_t, base_clone = _on_device(ctx, base)
        got, stats = t_crs.run(ctx, base_t, src, dst)
        assert got.shape == (N, 3) and t_crs.same(np.isnan(got), np.repeat(flag != 0, 3).reshape(-1, 3))
        assert stats.tolist() == [int((flag == 1).sum()), int((flag == 2).sum()), 0, 0]
        assert (cs.worst_errors(got, want, "tm", from_ecef=True) <= cs.bounds(golden, 4.0)).all()
        by_face, face_stats = t_crs.run(ctx, base_t, src, dst, faces=faces)
        with np.errstate(invalid="ignore"):
            mean = ((got[faces[:, 0]] + got[faces[:, 1]]) + got[faces[:, 2]]) / 3.0
        assert by_face.shape == (N, 3) and t_crs.same(by_face, mean)
        assert int(face_stats[2]) == 0 and int(face_stats[:2].sum()) == int(np.isnan(mean).any(axis=1).sum())
        _untouched(base_t, base_clone)


# ---- the orthomosaic baseline -------------------------------------------------------------------------------------------------
ORTHO_SHAPES = {"65x3": (65, 3), "1x1": (1, 1)}


@pytest.mark.parametrize("want_counts", [True, False], ids=["counts", "no_counts"])
@pytest.mark.parametrize("count_type", sorted(t_ortho.COUNT_TYPES))
@pytest.mark.parametrize("shape", sorted(ORTHO_SHAPES))
def test_assemble_tiles(ctx, shape, count_type, want_counts):
    """Tiles as `test_extent_widths` lays them (tests/test_ortho_assemble_gpu.py) over an extent of 65 x 3 and of 1 x 1; five
    classes, nodata 255: neither the class raster nor (asserted below) a uint8 count can be the poison's 127."""
    width, height = ORTHO_SHAPES[shape]
    rng = np.random.default_rng(width)
    windows = [(c, 0, min(40, width - c), height) for c in range(0, width, 25)]
    preds = [np.where(rng.random((h, w)) < 0.1, 255, rng.integers(0, 5, (h, w))).astype(np.uint8) for _, _, w, h in windows]
    dtype = t_ortho.COUNT_TYPES[count_type]
    want = t_ortho.osn.assemble(preds, windows, width, height, 5, 255, 0.3, dtype, 4)
    assert POISON not in want[0] and (count_type != "uint8" or POISON not in want[1])
    with fenced(ctx):
        if want_counts:
            t_ortho.check(ctx, preds, windows, width, height, 5, nodataval=255, frac=0.3, count_dtype=dtype)
        else:
            classes, counts, stats = t_ortho.run(ctx, preds, windows, width, height, 5, nodataval=255, frac=0.3, count_dtype=dtype,
                                                 want_counts=False)
            assert counts is None and classes.dtype == np.uint8 and np.array_equal(classes, want[0])
            assert np.array_equal(stats, want[2])


@pytest.mark.parametrize("C", [1, 256])
@pytest.mark.parametrize("P", [1, 3])
def test_zonal_class_counts(ctx, P, C):
    H, W = 65, 257
    raster = t_zonal.raster_of(P * 1000 + C, H, W, top=9)
    raster[3:6, 3:9] = 255
    rings = [t_zonal.square(-1, -1, W + 1, H + 1), t_zonal.square(0.2 * W, 0.2 * H, 0.75 * W + 0.4, 0.75 * H + 0.4),
             np.array([(0.0, 0.0), (W, 0.3 * H), (0.4 * W, H)])][:P]
    with fenced(ctx):
        counts, _ = t_zonal.check(ctx, raster, None if C == 256 else 255, rings, list(range(P)), P, C)
    assert counts.shape == (P, C) and counts.sum() > 0
