"""The polygon path of the sparse index aggregation (`gr_project_polygon_pairs`, `PairAccumulator.add_polygons`): region
detections tested on the device at each face's winning pixel, with real rasterization of C1 (9 800 faces: the last block
holds one full wave and 8 lanes; 640 x 480).  Two independent expectations, both compared exactly:
(a) numpy: oracle ids -> the last pixel of each face wins -> the host mask of the same rings at that pixel;
(b) the base class's dense `summed_projections` of the same segmentor through its materialised (h, w, C) image."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

from geograypher_amd import _hip
from geograypher_amd.cameras import SegmentorPhotogrammetryCameraSet
from geograypher_amd.cameras.cameras import vtk_like_near_planes
from geograypher_amd.meshes import TexturedPhotogrammetryMesh, TexturedPhotogrammetryMeshIndexPredictions
from geograypher_amd.predictors import Segmentor
from geograypher_amd.predictors.derived_segmentors import _ring_box, _ring_contains
from geograypher_amd.utils import synthetic
from oracle import oracle_c

pytestmark = pytest.mark.gpu

CHUNK = _hip.POLYGON_RING_CHUNK
H, W = 480, 640


def _table(rings, h=H, w=W):
    """[(class, (n, 2) (row, col) vertices)] -> ((boxes, vert_offsets, verts), (h, w)) as `label_regions` builds it."""
    kept = []
    for cls, v in rings:
        v = np.asarray(v, dtype=np.float64).reshape(-1, 2)
        box = _ring_box(v[:, 0], v[:, 1], h, w)
        if box is not None:
            kept.append((int(cls), box, v))
    kept.sort(key=lambda t: t[0])
    boxes = np.array([(*box, cls) for cls, box, _ in kept], dtype=np.int32).reshape(-1, 5)
    vert_offsets = np.zeros(len(kept) + 1, dtype=np.int32)
    vert_offsets[1:] = np.cumsum([v.shape[0] for _, _, v in kept])
    verts = np.concatenate([v for _, _, v in kept]) if kept else np.zeros((0, 2))
    return (boxes, vert_offsets, verts), (h, w)


def _mask(table, n_classes):
    (boxes, vert_offsets, verts), (h, w) = table
    out = np.zeros((h, w, n_classes), dtype=bool)
    for r, (i0, j0, i1, j1, cls) in enumerate(boxes.tolist()):
        ring = verts[vert_offsets[r]:vert_offsets[r + 1]]
        out[i0:i1, j0:j1, cls] |= _ring_contains(ring[:, 0], ring[:, 1], (i0, j0, i1, j1))
    return out


class _Rings(Segmentor):
    """Ring tables per view (keyed by file name): a region-detection segmentor without the files."""

    def __init__(self, tables, num_classes):
        self.tables, self.num_classes = tables, num_classes

    def label_regions(self, filename, image_scale=1):
        return self.tables[Path(filename).name] if image_scale == 1 else None

    def segment_image(self, image, filename, image_scale):
        return _mask(self.tables[Path(filename).name], self.num_classes)


class _PerPixel(Segmentor):
    """The same segmentor without its ring tables: the aggregation takes the materialised image."""

    def __init__(self, seg):
        self.seg, self.num_classes = seg, seg.num_classes

    def segment_image(self, image, filename, image_scale):
        return self.seg.segment_image(image, filename=filename, image_scale=image_scale)


@functools.lru_cache(maxsize=None)
def _scene():
    (points, faces), cams = synthetic.config1_scene()
    return points, faces, cams[0:3]


@functools.lru_cache(maxsize=None)
def _oracle_ids():
    """Oracle ids of the three views, computed once for the module and never written to."""
    points, faces, cams = _scene()
    lo, hi = points.min(axis=0), points.max(axis=0)
    nears = vtk_like_near_planes(np.stack([np.asarray(c.cam_to_world_transform, dtype=np.float64) for c in cams.cameras]),
                                 np.array([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]]))
    recs = cams.get_raster_records(1.0, near=list(nears))
    ids = np.stack([oracle_c.raster(points, faces, recs[v], H, W).astype(np.int64) for v in range(len(cams))])
    ids.setflags(write=False)
    return ids


def _expected(ids, masks, n_faces, n_classes, neg1):
    """(a): per view the last pixel (row-major) showing a face wins; the face is one observation of every class whose mask
    holds that pixel, and counts once if any does.  -> (summed (F, C) int64, counts (F,) int64)."""
    summed = np.zeros((n_faces, n_classes), dtype=np.int64)
    counts = np.zeros(n_faces, dtype=np.int64)
    for view_ids, mask in zip(ids, masks):
        flat = np.array(view_ids, dtype=np.int64).reshape(-1)
        if neg1:
            flat[flat == -1] = n_faces - 1
        ok = np.nonzero((flat >= 0) & (flat < n_faces))[0]
        last = np.full(n_faces, -1, dtype=np.int64)
        np.maximum.at(last, flat[ok], ok)
        seen = np.nonzero(last >= 0)[0]
        rows = mask.reshape(-1, n_classes)[last[seen]]
        summed[seen] += rows
        counts[seen] += rows.any(axis=1)
    return summed, counts


def _names(cams):
    return [cams.get_image_filename(v).name for v in range(len(cams))]


def _run(hip, tables, n_classes, neg1=True, batch_size=1, dense=True):
    """Aggregates through the region tables and checks (a) and, with `dense`, (b).  -> (summed, counts) of (a)."""
    points, faces, cams = _scene()
    seg = _Rings(dict(zip(_names(cams), tables)), n_classes)
    mesh = TexturedPhotogrammetryMeshIndexPredictions((points, faces), log_level="ERROR", backend=hip, neg1_is_last_face=neg1)
    avg, info = mesh.aggregate_projected_images(SegmentorPhotogrammetryCameraSet(cams, seg), n_classes=n_classes,
                                                batch_size=batch_size)
    n_used = (len(cams) // batch_size) * batch_size
    want_summed, want_counts = _expected(_oracle_ids()[:n_used], [_mask(t, n_classes) for t in tables[:n_used]],
                                         faces.shape[0], n_classes, neg1)
    got_summed = info["summed_projections"].toarray()
    got_counts = info["projection_counts"].toarray()[:, 0]
    np.testing.assert_array_equal(got_summed, want_summed)
    np.testing.assert_array_equal(got_counts, want_counts)
    with np.errstate(divide="ignore", invalid="ignore"):   # the class's own quotient: summed * (1 / counts)
        want_avg = np.where(want_counts[:, None] > 0, want_summed * np.reciprocal(want_counts.astype(float))[:, None], 0.0)
    np.testing.assert_array_equal(avg.toarray(), want_avg)
    if dense:
        base = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=hip, neg1_is_last_face=neg1)
        _, dense_info = base.aggregate_projected_images(SegmentorPhotogrammetryCameraSet(cams, _PerPixel(seg)),
                                                        batch_size=batch_size)
        dense_summed = np.asarray(dense_info["summed_projections"])
        assert dense_summed.shape == got_summed.shape
        unseen = np.isnan(dense_summed).all(axis=1)
        assert not got_summed[unseen].any()                       # NaN = no view shows the face
        np.testing.assert_array_equal(got_summed, np.nan_to_num(dense_summed, nan=0.0).astype(np.int64))
    return want_summed, want_counts


def _blobs(rng, n, n_classes, lo=3, hi=9):
    """n small star-shaped rings well inside the image (none is dropped), classes drawn at random."""
    out = []
    for _ in range(n):
        nv = int(rng.integers(lo, hi))
        t = np.sort(rng.uniform(0, 2 * np.pi, nv))
        rad = rng.uniform(4, 30, nv)
        ci, cj = rng.uniform(40, H - 40), rng.uniform(40, W - 40)
        out.append((int(rng.integers(0, n_classes)), np.stack([ci + rad * np.sin(t), cj + rad * np.cos(t)], axis=1)))
    return out


@pytest.mark.parametrize("sizes,neg1", [((0, 1, CHUNK - 1), True), ((CHUNK, CHUNK + 1, 2 * CHUNK + 1), False)])
def test_rings_per_view_around_the_chunk(hip, sizes, neg1):
    rng = np.random.default_rng(sum(sizes))
    nc = 5
    tables = [_table(_blobs(rng, n, nc)) for n in sizes]
    assert [t[0][0].shape[0] for t in tables] == list(sizes)
    summed, counts = _run(hip, tables, nc, neg1=neg1)
    assert counts.max() > 0 and (summed > 0).sum(axis=1).max() > 1   # some face lies in rings of several classes


def test_all_views_empty(hip):
    summed, counts = _run(hip, [_table([])] * 3, 4)
    assert not summed.any() and not counts.any()


def _big(ci, cj, r, n=12, phase=0.0):
    t = np.linspace(0, 2 * np.pi, n, endpoint=False) + phase
    return np.stack([ci + r * np.sin(t), cj + r * np.cos(t)], axis=1)


def test_overlaps_within_and_across_classes(hip):
    """Two overlapping rings of ONE class are one pair per face and view; overlapping rings of TWO classes are two."""
    same = _table([(2, _big(240, 300, 90)), (2, _big(240, 360, 90, phase=0.3))])
    two = _table([(0, _big(240, 300, 90)), (3, _big(240, 360, 90, phase=0.3))])
    summed, counts = _run(hip, [same, two, same], 4)
    assert summed[:, 2].max() == 2 and summed.max() == 2         # never more than one pair per view
    both = (summed[:, 0] > 0) & (summed[:, 3] > 0)
    assert both.any() and np.all(counts[both] <= 3)
    assert np.all(counts <= 3) and counts.max() == 3


def test_integer_vertex_rings_from_the_goldens(hip):
    """Pixel centres on vertices and on horizontal, vertical and diagonal edges, moved to where faces are seen."""
    golden = Path(__file__).resolve().parent / "golden" / "reference_draw_polygon.npz"
    with np.load(golden, allow_pickle=False) as g:
        names, offsets, verts = g["names"], g["offsets"], g["verts"]
    rings = [verts[offsets[k]:offsets[k + 1]] for k, name in enumerate(names) if str(name).startswith("int_")]
    assert len(rings) >= 10
    tables = []
    for v in range(3):
        placed = [(k % 3, ring * (2 + v) + np.array([60 + 37 * (k % 6), 90 + 83 * (k % 5)])) for k, ring in enumerate(rings)]
        assert all(np.array_equal(p, np.round(p)) for _, p in placed)
        tables.append(_table(placed))
    _, counts = _run(hip, tables, 3)
    assert counts.max() > 0


def test_rings_of_3_and_200_vertices(hip):
    rng = np.random.default_rng(200)
    t = np.linspace(0, 2 * np.pi, 200, endpoint=False)
    wobbly = np.stack([240 + (120 + 40 * np.sin(9 * t)) * np.sin(t), 320 + (150 + 50 * np.cos(7 * t)) * np.cos(t)], axis=1)
    tri = np.array([(100.5, 80.25), (400.0, 200.0), (150.75, 600.5)])
    tables = [_table([(1, wobbly), (0, tri)]), _table([(0, tri)]), _table([(1, wobbly)] + _blobs(rng, 20, 2, lo=3, hi=4))]
    assert tables[0][0][1].tolist() == [0, 3, 203]
    _, counts = _run(hip, tables, 2)
    assert counts.max() == 3


def test_class_outside_range_raises(hip):
    points, faces, cams = _scene()
    tables = [_table([(1, _big(240, 320, 100)), (7, _big(200, 300, 60))])] * 3
    mesh = TexturedPhotogrammetryMeshIndexPredictions((points, faces), log_level="ERROR", backend=hip)
    with pytest.raises(IndexError):
        mesh.aggregate_projected_images(SegmentorPhotogrammetryCameraSet(cams, _Rings(dict(zip(_names(cams), tables)), 5)),
                                        n_classes=5)
    _run(hip, tables, 8, dense=False)   # the same rings with enough classes; the backend is usable again


@pytest.mark.parametrize("cap,batch_size", [("tiny", 1), ("tiny", 3), ("one_view", 3)])
def test_small_key_buffer_gives_the_same_result(hip, monkeypatch, cap, batch_size):
    """A forced small buffer: the call is split by views, the buffer compacted between them, and grown for a view that
    alone exceeds it ("tiny": 64 keys) -- the pairs and counts must be those of (a), nothing dropped."""
    rng = np.random.default_rng(64)
    nc = 6
    tables = [_table(_blobs(rng, 150, nc) + [(v, _big(240, 320, 150))]) for v in range(3)]
    bounds = [int(_hip.polygon_pair_bounds(t[0][0], [0, t[0][0].shape[0]], 9800)[0]) for t in tables]
    assert min(bounds) > 64
    cap = 64 if cap == "tiny" else max(bounds)   # "one_view": every view fits, no two do
    made = []
    plain = hip.new_pair_accumulator

    def small(*args, **kwargs):
        made.append(plain(*args, cap=cap, **kwargs))
        return made[-1]

    monkeypatch.setattr(hip, "new_pair_accumulator", small)
    _run(hip, tables, nc, batch_size=batch_size, dense=False)
    acc, = made
    if cap == 64:
        assert acc.grown >= 1 and min(bounds) <= acc.cap <= max(bounds)
    else:
        assert acc.grown == 0 and acc.cap == cap and acc.compactions >= 2


def test_batch_sizes_agree(hip):
    rng = np.random.default_rng(31)
    nc = 4
    tables = [_table(_blobs(rng, 40, nc)) for _ in range(3)]
    one = _run(hip, tables, nc, batch_size=1)
    three = _run(hip, tables, nc, batch_size=3)
    np.testing.assert_array_equal(one[0], three[0])
    np.testing.assert_array_equal(one[1], three[1])


@pytest.mark.parametrize("neg1", [True, False])
def test_view_without_a_visible_face_on_drawn_ids(hip, neg1):
    """`add_polygons` on drawn ids over 300 degenerate faces: the middle view shows no face (all ids -1: with
    neg1_is_last_face every pixel then shows the LAST face), ring tables of 2, 3 and 0 rings."""
    rng = np.random.default_rng(5)
    F, h, w, nc = 300, 24, 31, 3
    hip.upload_mesh(np.zeros((3, 3), dtype=np.float32), np.zeros((F, 3), dtype=np.int32))
    ids = rng.integers(-1, F, (3, h, w)).astype(np.int32)
    ids[1] = -1
    tables = [_table([(0, [(2, 2), (2, 20), (15, 20), (15, 2)]), (2, [(10.5, 5.5), (23, 12), (8, 30)])], h, w),
              _table([(1, [(0, 0), (0, 30), (23, 30), (23, 0)]), (1, [(5, 5), (5, 9), (9, 9)]), (2, [(1, 1), (1, 8), (8, 1)])], h, w),
              _table([], h, w)]
    boxes = np.concatenate([t[0][0] for t in tables])
    poly_offsets = np.cumsum([0] + [t[0][0].shape[0] for t in tables])
    verts = np.concatenate([t[0][2] for t in tables])
    vert_offsets = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(t[0][1]) for t in tables]))])
    counts = torch.zeros((F,), dtype=torch.int32, device=hip.device)
    acc = hip.new_pair_accumulator(nc, counts, neg1_is_last_face=neg1)
    acc.add_polygons(ids, boxes, vert_offsets, verts, poly_offsets)
    keys, mult = acc.finish()
    want_summed, want_counts = _expected(ids, [_mask(t, nc) for t in tables], F, nc, neg1)
    got = np.zeros((F, nc), dtype=np.int64)
    got[keys // nc, keys % nc] = mult
    np.testing.assert_array_equal(got, want_summed)
    np.testing.assert_array_equal(counts.cpu().numpy(), want_counts)
    assert want_counts.sum() > 0 and (want_summed[F - 1, 1] == 1) == neg1
