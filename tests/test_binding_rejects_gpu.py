"""What the binding rejects on the host: every `HipRaster` method that checks a shape, one wrong input each.

One backend, one tiny mesh (4 vertices, 2 faces), 4 x 4 images.  Every case is refused before a launch: the test pins the
exception type, and the message where another test or a caller matches it (for the rest: that the message says which shape it
got).  Nothing here reaches a kernel."""
import re

import numpy as np
import pytest

from geograypher_amd import _hip

pytestmark = pytest.mark.gpu

VERTS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.float64)
FACES = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32)
FACES4 = np.zeros((2, 4), dtype=np.int32)
VQ = VERTS[:, :2].astype(np.int64)
IDS = np.zeros((4, 4), dtype=np.int32)
IMG = np.zeros((4, 4), dtype=np.float64)
CAM = np.zeros((1, _hip.GR_CAM_FLOATS), dtype=np.float32)
# one triangle ring of one polygon row, and the 1 x 1 cell table over it
RING = dict(ring_vertices=np.array([[0, 0], [4, 0], [0, 4]], dtype=np.int64), ring_offsets=np.array([0, 3], dtype=np.int64),
            ring_polygon=np.array([0], dtype=np.int32), ring_is_hole=np.array([0], dtype=np.int32),
            polygon_boxes=np.array([[0, 0, 4, 4]], dtype=np.int64))
CELLS = (np.array([0, 0, 4, 4, 1, 1]), np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32))
TRI = np.zeros((2, 6), dtype=np.int64)
RASTER = np.zeros((4, 4), dtype=np.float32)
INV6 = [0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
ECEF, UTM = "EPSG:4978", "EPSG:32610"


def ring(**changed):
    return {**RING, **changed}


def weights(b, tri=TRI, cls=np.zeros(2, dtype=np.int32), w=np.ones(2), **changed):
    return b.polygon_class_weights(tri, cls, w, n_classes=2, **ring(**changed))


def fpi(b, verts_q=VQ, faces=FACES, cells=CELLS, **changed):
    return b.face_polygon_index(verts_q, faces, cell_table=cells, **ring(**changed))


def sample(b, points=VERTS, faces=FACES, raster=RASTER, inv=INV6, **kw):
    return b.sample_raster(points, faces, raster, inv, None, 0.0, **kw)


def device_tensor(b, shape, dtype):
    import torch

    return torch.zeros(shape, dtype=getattr(torch, dtype), device=b.device)


def equirect_view_of_a_short_ray_grid(b):
    source = b.equirect_upload(np.arange(16, dtype=np.uint8).reshape(4, 4))
    return b.equirect_view(source, np.zeros(3), np.zeros(4), np.eye(3), (4, 4))


SHAPE = object()   # "the message names the shape it got": the case's last element is that shape

# (id, call, exception, what the message must match: a pattern, or SHAPE and the wrong shape)
CASES = [
    ("upload_mesh-verts_V2", lambda b: b.upload_mesh(VERTS[:, :2], FACES), ValueError, SHAPE, (4, 2)),
    ("upload_mesh-faces_F4", lambda b: b.upload_mesh(VERTS, FACES4), ValueError, SHAPE, (2, 4)),
    ("raster_face_ids-cams_15", lambda b: b.raster_face_ids(CAM[:, :15], 4, 4), ValueError, SHAPE, (1, 15)),
    ("raster_face_ids-out_dtype", lambda b: b.raster_face_ids(CAM, 4, 4, out=device_tensor(b, (1, 4, 4), "float32")),
     ValueError, "out must be a contiguous int32 tensor"),
    ("raster_face_ids-out_shape", lambda b: b.raster_face_ids(CAM, 4, 4, out=device_tensor(b, (1, 4, 5), "int32")),
     ValueError, "out must be a contiguous int32 tensor"),
    ("project_index_pairs-img_shape", lambda b: b.project_index_pairs(IDS, np.zeros((4, 5)), 2, None), ValueError, SHAPE, (1, 4, 5)),
    ("pair_accumulator_add-img_shape", lambda b: b.new_pair_accumulator(2, None, cap=16).add(IDS, np.zeros((4, 5))),
     ValueError, SHAPE, (1, 4, 5)),
    ("ray_pair_count-starts_N2", lambda b: b.ray_pair_count(VERTS[:, :2], VERTS, np.zeros(4), 1.0), ValueError, SHAPE, (4, 2)),
    ("ray_pair_edges-ends_rows", lambda b: b.ray_pair_edges(VERTS, VERTS[:3], np.zeros(4), 1.0), ValueError, SHAPE, (3, 3)),
    ("ray_pair_edges-ids_length", lambda b: b.ray_pair_edges(VERTS, VERTS, np.zeros(3), 1.0), ValueError, SHAPE, (3,)),
    ("clip_rays-origins_N2", lambda b: b.clip_rays(VERTS[:, :2], VERTS, VERTS, FACES), ValueError, SHAPE, (4, 2)),
    ("clip_rays-points_V2", lambda b: b.clip_rays(VERTS, VERTS, VERTS[:, :2], FACES), ValueError, SHAPE, (4, 2)),
    ("clip_rays-faces_F4", lambda b: b.clip_rays(VERTS, VERTS, VERTS, FACES4), ValueError, SHAPE, (2, 4)),
    ("points_bounds-points_V2", lambda b: b.points_bounds(VERTS[:, :2]), ValueError, r"points must be \(V, 3\), got \(4, 2\)"),
    ("cover_grid-points_V2", lambda b: b.cover_grid(VERTS[:, :2], *[np.zeros(2)] * 4), ValueError,
     r"points must be \(V, 3\), got \(4, 2\)"),
    ("cover_grid-tables_unequal", lambda b: b.cover_grid(VERTS, np.zeros(2), np.zeros(2), np.zeros(3), np.zeros(2)),
     ValueError, r"one length, got \[2, 2, 3, 2\]"),
    ("set_cover-face_ptr_length", lambda b: b.set_cover(np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int32), 2, 1),
     ValueError, "face_ptr must hold n_faces \\+ 1 = 3 offsets, got 2"),
    ("polygon_class_weights-tri_F5", lambda b: weights(b, tri=TRI[:, :5]), ValueError, SHAPE, (2, 5)),
    ("polygon_class_weights-weights_length", lambda b: weights(b, w=np.ones(3)), ValueError, SHAPE, (3,)),
    ("polygon_class_weights-ring_vertices_N3", lambda b: weights(b, ring_vertices=np.zeros((3, 3), dtype=np.int64)),
     ValueError, SHAPE, (3, 3)),
    ("polygon_class_weights-ring_offsets_length", lambda b: weights(b, ring_offsets=np.array([0, 1, 3])), ValueError, SHAPE, (3,)),
    ("polygon_class_weights-hole_flags_length", lambda b: weights(b, ring_is_hole=np.zeros(2, dtype=np.int32)),
     ValueError, SHAPE, (2,)),
    ("polygon_class_weights-boxes_P5", lambda b: weights(b, polygon_boxes=np.zeros((1, 5), dtype=np.int64)),
     ValueError, SHAPE, (1, 5)),
    ("face_polygon_index-verts_V3", lambda b: fpi(b, verts_q=VERTS.astype(np.int64)), ValueError, SHAPE, (4, 3)),
    ("face_polygon_index-faces_F4", lambda b: fpi(b, faces=FACES4), ValueError, SHAPE, (2, 4)),
    ("face_polygon_index-boxes_P5", lambda b: fpi(b, polygon_boxes=np.zeros((1, 5), dtype=np.int64)), ValueError, SHAPE, (1, 5)),
    ("face_polygon_index-grid_5_values", lambda b: fpi(b, cells=(CELLS[0][:5],) + CELLS[1:]), ValueError,
     "cell grid is .*got 5 values"),
    ("face_polygon_index-cell_offsets_length", lambda b: fpi(b, cells=(CELLS[0], np.array([0, 1, 1]), CELLS[2])), ValueError,
     r"gr_face_polygon_index: a 1 x 1 cell grid needs 2 cell offsets, got \(3,\)"),
    ("face_polygon_index-grid_beyond_int32", lambda b: fpi(b, cells=(np.array([0, 0, 4, 4, 2 ** 31, 1]),) + CELLS[1:]),
     ValueError, "gr_face_polygon_index: bad cell grid nx=2147483648 ny=1"),
    ("points_in_region-points_N3", lambda b: b.points_in_region(VERTS.astype(np.int64), **RING), ValueError,
     r"points must be \(N, 2\), got \(4, 3\)"),
    ("points_in_region-ring_vertices_N3", lambda b: b.points_in_region(VQ, **ring(ring_vertices=np.zeros((3, 3), dtype=np.int64))),
     ValueError, SHAPE, (3, 3)),
    ("points_in_region-buffer_negative", lambda b: b.points_in_region(VQ, buffer_steps=-1, **RING), ValueError, "buffer D=-1"),
    ("submesh_extract-faces_F4", lambda b: b.submesh_extract(np.ones(4, dtype=bool), FACES4), ValueError, SHAPE, (2, 4)),
    ("class_outlines-verts_V3", lambda b: b.class_outlines(VERTS.astype(np.int64), FACES, np.zeros(2), 2), ValueError, SHAPE, (4, 3)),
    ("class_outlines-faces_F4", lambda b: b.class_outlines(VQ, FACES4, np.zeros(2), 2), ValueError, SHAPE, (2, 4)),
    ("class_outlines-classes_length", lambda b: b.class_outlines(VQ, FACES, np.zeros(3), 2), ValueError,
     "2 faces need 2 classes, got 3"),
    ("class_outlines-too_many_classes", lambda b: b.class_outlines(VQ, FACES, np.zeros(2), 65536), ValueError,
     "gr_class_outlines: n_classes=65536"),
    ("sample_raster-points_V2", lambda b: sample(b, points=VERTS[:, :2]), ValueError, r"points must be \(V, 3\), got \(4, 2\)"),
    ("sample_raster-faces_F4", lambda b: sample(b, faces=FACES4), ValueError, SHAPE, (2, 4)),
    ("sample_raster-raster_4d", lambda b: sample(b, raster=np.zeros((1, 1, 4, 4))), ValueError,
     r"raster data must be \(B, H, W\) or \(H, W\) with no empty axis, got \(1, 1, 4, 4\)"),
    ("sample_raster-raster_empty_axis", lambda b: sample(b, raster=np.zeros((4, 0))), ValueError, "raster data must be"),
    ("sample_raster-inverse_5", lambda b: sample(b, inv=INV6[:5]), ValueError, "six coefficients, got 5"),
    ("sample_raster-labels_without_threshold", lambda b: sample(b, labels=np.zeros(2)), ValueError,
     "labels need threshold and ground_id"),
    ("sample_raster-labels_length", lambda b: sample(b, labels=np.zeros(3), threshold=1.0, ground_id=0.0), ValueError, SHAPE, (3,)),
    ("reproject_points-points_V2", lambda b: b.reproject_points(VERTS[:, :2], ECEF, UTM), ValueError,
     r"points must be \(V, 3\), got \(4, 2\)"),
    ("reproject_points-faces_F4", lambda b: b.reproject_points(VERTS, ECEF, UTM, faces=FACES4), ValueError, SHAPE, (2, 4)),
    ("reproject_points-pre_transform_3x3", lambda b: b.reproject_points(VERTS, ECEF, UTM, pre_transform=np.eye(3)), ValueError,
     r"pre_transform must be \(4, 4\), got \(3, 3\)"),
    ("reproject_points-out_dtype", lambda b: b.reproject_points(VERTS, ECEF, UTM, out=device_tensor(b, (4, 3), "float32")),
     ValueError, r"out must be a contiguous float64 \(4, 3\) tensor"),
    ("reproject_points-out_shape", lambda b: b.reproject_points(VERTS, ECEF, UTM, faces=FACES, out=device_tensor(b, (4, 3), "float64")),
     ValueError, r"out must be a contiguous float64 \(2, 3\) tensor"),
    ("project_labels-labels_shape", lambda b: b.project_labels(IDS, np.zeros((4, 5), dtype=np.uint8), 2, None, None),
     ValueError, SHAPE, (1, 4, 5)),
    ("project_values-img_shape", lambda b: b.project_values(IDS, np.zeros((4, 5, 2)), None, None), ValueError, SHAPE, (1, 4, 5, 2)),
    ("project_view-img_shape", lambda b: b.project_view(IDS, np.zeros((4, 5, 2))), ValueError, SHAPE, (4, 5, 2)),
    ("raster_project_labels-cams_count", lambda b: b.raster_project_labels(np.repeat(CAM, 2, 0), np.zeros((1, 4, 4), dtype=np.uint8),
                                                                         2, None, None),
     ValueError, "2 camera records for 1 label images"),
    ("resize_image-1d", lambda b: b.resize_image(np.zeros(4)), ValueError, r"image must be \(H,W\) or \(H,W,C\), got shape \(4,\)"),
    ("equirect_upload-1d", lambda b: b.equirect_upload(np.zeros(4)), ValueError, SHAPE, (4,)),
    ("equirect_view-ray_grid", equirect_view_of_a_short_ray_grid, ValueError, "ray grid of 4 x 3 samples"),
    ("upload_map-3HW", lambda b: b.upload_map(np.zeros((3, 4, 4))), ValueError, r"sampling map must be \(2, H, W\), got \(3, 4, 4\)"),
    ("warp_image-1d", lambda b: b.warp_image(np.arange(4.0), device_tensor(b, (2, 4, 4), "float64")), ValueError,
     r"image must be \(I,J\) or \(I,J,C\), got shape \(4,\)"),
]


@pytest.fixture(scope="module")
def backend():
    b = _hip.HipRaster(0)
    fresh = (b.last_ray_pair_calls, b.last_outline_calls)
    b.upload_mesh(VERTS, FACES)
    yield b, fresh
    b.close()


def test_count_then_fill_counters_read_zero_on_a_fresh_backend(backend):
    assert backend[1] == (0, 0)


@pytest.mark.parametrize("call,exception,match,shape", [pytest.param(*c[1:4], c[4] if len(c) > 4 else None, id=c[0]) for c in CASES])
def test_wrong_input_is_rejected_on_the_host(backend, call, exception, match, shape):
    b = backend[0]
    with pytest.raises(exception, match=re.escape(str(shape)) if match is SHAPE else match):
        call(b)
    # ... and the backend is what it was: the mesh, and no count-then-fill call was made
    assert (b.n_verts, b.n_faces, b.last_ray_pair_calls, b.last_outline_calls) == (4, 2, 0, 0)
