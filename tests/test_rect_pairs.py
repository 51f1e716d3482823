"""The rectangle path of the sparse index aggregation (`gr_project_rect_pairs`, `PairAccumulator.add_rects`): detections
and image IDs looked up on the device at each face's winning pixel, with real rasterization.  Results must equal the
materialised path (the same segmentor's per-pixel image through `gr_project_index_pairs`) and the numpy restatement of
derived_meshes.py:470-550 on oracle ids."""
import numpy as np
import pytest
import torch

from geograypher_amd.cameras import SegmentorPhotogrammetryCameraSet
from geograypher_amd.cameras.cameras import vtk_like_near_planes
from geograypher_amd.meshes import TexturedPhotogrammetryMeshIndexPredictions
from geograypher_amd.predictors import ImageIDSegmentor, Segmentor, TabularRectangleSegmentor
from geograypher_amd.utils import synthetic
from oracle import oracle_c, oracle_np

pytestmark = pytest.mark.gpu


class _Boxes(Segmentor):
    """Rectangles per view (keyed by file name), painted in order -- a detection table without the CSV."""

    def __init__(self, boxes, num_classes):
        self.boxes, self.num_classes = boxes, num_classes

    def label_rectangles(self, filename, image_scale=1):
        return self.boxes[filename.name]

    def segment_image(self, image, filename, image_scale):
        rects, hw = self.boxes[filename.name]
        img = np.full(hw, np.nan)
        for imin, jmin, imax, jmax, cls in rects.tolist():
            img[imin:imax, jmin:jmax] = cls
        return img


class _PerPixel(Segmentor):
    """The same segmentor without its rectangles: the aggregation takes the materialised path."""

    def __init__(self, seg):
        self.seg, self.num_classes = seg, getattr(seg, "num_classes", None)

    def segment_image(self, image, filename, image_scale):
        return self.seg.segment_image(image, filename=filename, image_scale=image_scale)


def _random_boxes(rng, n, h, w, n_classes):
    """n boxes, a share of them reaching over the image's edges or with negative (wrapping) corners, normalised like
    `label_rectangles` does."""
    out = []
    for _ in range(n):
        i0, j0 = int(rng.integers(-h // 8, h)), int(rng.integers(-w // 8, w))
        i1, j1 = i0 + int(rng.integers(1, h // 3)), j0 + int(rng.integers(1, w // 3))
        a, b, _ = slice(i0, i1).indices(h)
        c, d, _ = slice(j0, j1).indices(w)
        if b > a and d > c:
            out.append((a, c, b, d, int(rng.integers(0, n_classes))))
    return np.array(out, dtype=np.int32).reshape(-1, 5)


def _aggregate(mesh, cams, seg, n_classes, scale):
    avg, info = mesh.aggregate_projected_images(SegmentorPhotogrammetryCameraSet(cams, seg), n_classes=n_classes,
                                                aggregate_img_scale=scale)
    return avg, info


def _assert_same(a, b):
    avg_a, info_a = a
    avg_b, info_b = b
    for k in ("summed_projections", "projection_counts"):
        assert info_a[k].shape == info_b[k].shape
        assert (info_a[k] != info_b[k]).nnz == 0, k
    assert avg_a.shape == avg_b.shape and (avg_a != avg_b).nnz == 0


def _oracle(points, faces, cams, seg, n_classes, scale, neg1):
    """derived_meshes.py:470-550 on oracle ids and the segmentor's per-pixel images, as sparse (face, class) counts."""
    lo, hi = points.min(axis=0), points.max(axis=0)
    nears = vtk_like_near_planes(np.stack([np.asarray(c.cam_to_world_transform, dtype=np.float64) for c in cams.cameras]),
                                 np.array([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]]))
    recs = cams.get_raster_records(scale, near=list(nears))
    h, w = cams[0].get_image_size(scale)
    F = faces.shape[0]
    projs = []
    for v in range(len(cams)):
        ids = oracle_c.raster(points, faces, recs[v], h, w).astype(np.int64)
        img = np.asarray(seg.segment_image(None, filename=cams.get_image_filename(v), image_scale=scale), dtype=np.float64)
        projs.append(oracle_np.project_image(ids, img.reshape(h, w, 1), F, check_null_image=True, neg1_is_last_face=neg1))
    if n_classes * F <= 50_000_000:
        _, counts, summed = oracle_np.aggregate_index_sparse(projs, F, n_classes)
        return np.asarray(counts).reshape(-1), summed
    counts = np.zeros(F, dtype=np.int64)   # too many classes for a dense (F, n_classes) array: the same sums, sparse
    keys = []
    for p in projs:
        inds = np.nonzero(np.isfinite(p[:, 0]))[0]
        counts[inds] += 1
        keys.append(inds * n_classes + p[inds, 0].astype(np.int64))
    return counts, np.unique(np.concatenate(keys), return_counts=True)


def _check_oracle(info, want, n_classes):
    counts, summed = want
    np.testing.assert_array_equal(info["projection_counts"].toarray()[:, 0], counts)
    if isinstance(summed, tuple):
        coo = info["summed_projections"].tocoo()
        keys = coo.row.astype(np.int64) * n_classes + coo.col
        order = np.argsort(keys)
        np.testing.assert_array_equal(keys[order], summed[0])
        np.testing.assert_array_equal(coo.data[order], summed[1])
    else:
        np.testing.assert_array_equal(info["summed_projections"].toarray(), summed)
    assert counts.sum() > 0


def _c1():
    (points, faces), cams = synthetic.config1_scene()
    return points, faces, cams


@pytest.mark.parametrize("neg1", [True, False])
def test_c1_boxes_fast_equals_materialised_and_oracle(hip, neg1):
    """C1 at full size: views with 0, 1, a few hundred and 5 000 boxes (several LDS chunks) and 40 classes."""
    points, faces, cams = _c1()
    h, w = cams[0].get_image_size(1.0)
    rng = np.random.default_rng(3)
    nc = 40
    sizes = [0, 1, 300, 5000, 57, 2, 180, 1000]
    boxes = {cams.get_image_filename(v).name: (_random_boxes(rng, n, h, w, nc), (h, w)) for v, n in enumerate(sizes)}
    assert boxes[cams.get_image_filename(3).name][0].shape[0] > 4000
    seg = _Boxes(boxes, nc)
    mesh = TexturedPhotogrammetryMeshIndexPredictions((points, faces), log_level="ERROR", backend=hip,
                                                      neg1_is_last_face=neg1)
    fast = _aggregate(mesh, cams, seg, nc, 1.0)
    slow = _aggregate(mesh, cams, _PerPixel(seg), nc, 1.0)
    _assert_same(fast, slow)
    _check_oracle(fast[1], _oracle(points, faces, cams, seg, nc, 1.0, neg1), nc)


def test_c1_instance_ids_1e5_classes(hip):
    """10^5 classes (one per detection, as with the default label_key instance_ID) and several views per batch."""
    points, faces, cams = _c1()
    h, w = cams[0].get_image_size(0.5)
    rng = np.random.default_rng(4)
    nc = 100_000
    boxes = {cams.get_image_filename(v).name: (_random_boxes(rng, 250, h, w, nc), (h, w)) for v in range(len(cams))}
    seg = _Boxes(boxes, nc)
    mesh = TexturedPhotogrammetryMeshIndexPredictions((points, faces), log_level="ERROR", backend=hip)
    fast = mesh.aggregate_projected_images(SegmentorPhotogrammetryCameraSet(cams, seg), n_classes=nc,
                                           aggregate_img_scale=0.5, batch_size=4)
    slow = mesh.aggregate_projected_images(SegmentorPhotogrammetryCameraSet(cams, _PerPixel(seg)), n_classes=nc,
                                           aggregate_img_scale=0.5, batch_size=4)
    _assert_same(fast, slow)
    _check_oracle(fast[1], _oracle(points, faces, cams, seg, nc, 0.5, True), nc)


def test_class_outside_range_raises_like_materialised(hip):
    points, faces, cams = _c1()
    cams = cams[0:2]
    h, w = cams[0].get_image_size(0.25)
    boxes = {cams.get_image_filename(v).name: (np.array([[0, 0, h, w, 1], [2, 3, 30, 40, 7]], dtype=np.int32), (h, w))
             for v in range(2)}
    mesh = TexturedPhotogrammetryMeshIndexPredictions((points, faces), log_level="ERROR", backend=hip)
    for seg in (_Boxes(boxes, 5), _PerPixel(_Boxes(boxes, 5))):
        with pytest.raises(IndexError):
            _aggregate(mesh, cams, seg, 5, 0.25)
    fine = _aggregate(mesh, cams, _Boxes(boxes, 8), 8, 0.25)  # the accumulator is usable again
    assert fine[1]["projection_counts"].sum() > 0


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_c1_image_ids(hip, tmp_path, scale):
    """annotation_image_selection's visibility matrix: ImageIDSegmentor, n_classes = number of views."""
    from PIL import Image

    points, faces, cams = _c1()
    H, W = cams[0].get_image_size(1.0)
    for v, cam in enumerate(cams.cameras):
        cam.image_filename = tmp_path / f"view_{v:03d}.png"
        Image.fromarray(np.zeros((H, W), dtype=np.uint8)).save(cam.image_filename)
    seg = ImageIDSegmentor(cams.get_image_filename(None, absolute=True))
    nc = len(cams)
    mesh = TexturedPhotogrammetryMeshIndexPredictions((points, faces), log_level="ERROR", backend=hip)
    fast = _aggregate(mesh, cams, seg, nc, scale)
    slow = _aggregate(mesh, cams, _PerPixel(seg), nc, scale)
    _assert_same(fast, slow)
    _check_oracle(fast[1], _oracle(points, faces, cams, seg, nc, scale, True), nc)


def _detections_csv(path, cams, h, w, rng, n_lo=50, n_hi=300):
    """A detection table in the layout project_detections reads (xmin/ymin/xmax/ymax, no instance_ID column)."""
    lines = ["image_path,xmin,ymin,xmax,ymax,score"]
    for v in range(len(cams)):
        name = cams.get_image_filename(v).name
        for _ in range(int(rng.integers(n_lo, n_hi + 1))):
            x0, y0 = rng.uniform(-40, w), rng.uniform(-40, h)
            lines.append(f"{name},{x0:.2f},{y0:.2f},{x0 + rng.uniform(5, 200):.2f},{y0 + rng.uniform(5, 200):.2f},0.5")
    path.write_text("\n".join(lines) + "\n")


def test_c2_subset_detections_table(hip, tmp_path):
    """C2 terrain (1.2 M faces), four views at 1000 x 750 with 50-300 boxes each from a real detection CSV."""
    points, faces = synthetic.terrain_mesh()
    # the segmentor's image is (h, w) at scale 1 (the only scale it reproduces): C2's poses with 1000 x 750 sensors
    small = synthetic.config2_cameras(50, f=750.0, width=1000, height=750).get_subset_cameras([11, 12, 23, 24])
    h, w = small[0].get_image_size(1.0)
    assert (h, w) == (750, 1000)
    _detections_csv(tmp_path / "det.csv", small, h, w, np.random.default_rng(9))
    seg = TabularRectangleSegmentor(tmp_path / "det.csv", (h, w), split_bbox=False)
    nc = seg.num_classes
    mesh = TexturedPhotogrammetryMeshIndexPredictions((points, faces), log_level="ERROR", backend=hip)
    fast = _aggregate(mesh, small, seg, nc, 1.0)
    slow = _aggregate(mesh, small, _PerPixel(seg), nc, 1.0)
    _assert_same(fast, slow)
    _check_oracle(fast[1], _oracle(points, faces, small, seg, nc, 1.0, True), nc)


def test_tin_detections(hip, tmp_path):
    """The irregular TIN (1.2 M faces, incoherent face order) under two C2 cameras at quarter scale."""
    points, faces = synthetic.tin_mesh()
    cams = synthetic.config2_cameras(50).get_subset_cameras([23, 24])
    h, w = cams[0].get_image_size(0.25)
    rng = np.random.default_rng(12)
    nc = 500
    boxes = {cams.get_image_filename(v).name: (_random_boxes(rng, 300, h, w, nc), (h, w)) for v in range(2)}
    seg = _Boxes(boxes, nc)
    mesh = TexturedPhotogrammetryMeshIndexPredictions((points, faces), log_level="ERROR", backend=hip)
    fast = _aggregate(mesh, cams, seg, nc, 0.25)
    slow = _aggregate(mesh, cams, _PerPixel(seg), nc, 0.25)
    _assert_same(fast, slow)
    _check_oracle(fast[1], _oracle(points, faces, cams, seg, nc, 0.25, True), nc)


@pytest.mark.parametrize("n", [65, 130])
def test_views_beyond_one_launch_group(hip, n):
    """More views than a launch group holds (64): from the second group on the kernel reads its views' rectangles at
    rect_offsets + 64 k.  Drawn ids over 300 degenerate faces, 0-3 small rectangles per view; keys, multiplicities and counts
    must equal `project_index_pairs` on the painted label images."""
    rng = np.random.default_rng(7000 + n)
    F, h, w, nc = 300, 9, 13, 6
    hip.upload_mesh(np.zeros((3, 3), dtype=np.float32), np.zeros((F, 3), dtype=np.int32))
    ids = rng.integers(-1, F, (n, h, w)).astype(np.int32)
    rects, offsets, area = [], [0], 0
    painted = np.full((n, h, w), np.nan)
    for v in range(n):
        for _ in range(int(rng.integers(0, 4))):
            i0, j0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            i1, j1 = min(h, i0 + int(rng.integers(1, 6))), min(w, j0 + int(rng.integers(1, 6)))
            cls = int(rng.integers(0, nc))
            rects.append((i0, j0, i1, j1, cls))
            painted[v, i0:i1, j0:j1] = cls  # in paint order: a later rectangle overwrites an earlier one
            area += (i1 - i0) * (j1 - j0)
        offsets.append(len(rects))
    per_view = np.diff(offsets)
    assert per_view.min() == 0 and per_view.max() == 3 and per_view[64:].sum() > 0
    assert np.isfinite(painted).sum() < area  # some rectangles overlap
    rects = np.array(rects, dtype=np.int32).reshape(-1, 5)
    got_counts = torch.zeros((F,), dtype=torch.int32, device=hip.device)
    acc = hip.new_pair_accumulator(nc, got_counts)
    acc.add_rects(ids, rects, np.array(offsets))
    got_keys, got_mult = acc.finish()
    want_counts = torch.zeros((F,), dtype=torch.int32, device=hip.device)
    want_keys, want_mult = hip.project_index_pairs(ids, painted, nc, want_counts)
    assert want_keys.size > 0 and want_mult.max() > 1
    assert np.array_equal(got_keys, want_keys) and np.array_equal(got_mult, want_mult)
    assert np.array_equal(got_counts.cpu().numpy(), want_counts.cpu().numpy())


@pytest.mark.parametrize("neg1", [True, False])
@pytest.mark.parametrize("F", [1, 255, 256, 257, 513])
def test_rects_per_view_around_the_chunk(hip, F, neg1):
    """K10r at the edges of its 512-row LDS chunk and of its 256-face block: drawn ids on a 17 x 33 image (ids[p] = p % F, three
    background pixels per view), six views with 0, 1, 511, 512, 513 and 1025 rectangles.  The 1025 of the last view are
    walked from the end in chunks of 512, 512 and 1: its last row covers the left half (those faces stop in the first chunk
    visited), its first row the whole image (a face no later row covers must reach the third chunk), the rows between are
    boxes of 1-2 pixels a side left of column 29.  Pairs and counts must equal numpy (rectangles painted in order,
    `oracle_np.project_image`, `aggregate_index_sparse`) on every face, and `project_index_pairs` on the painted images."""
    rng = np.random.default_rng(8000 + F)
    h, w, nc = 17, 33, 9
    sizes = [0, 1, 511, 512, 513, 1025]
    n = len(sizes)
    ids = np.tile((np.arange(h * w) % F).astype(np.int32), (n, 1))
    for v in range(n):
        ids[v, [7 * v + 3, 280 + v, h * w - 1 - v]] = -1   # view 0: the last pixel, which the last face wins with neg1
    ids = ids.reshape(n, h, w)
    rects = []
    for v, size in enumerate(sizes):
        for k in range(size):
            if size == 1025 and k == 0:
                rects.append((0, 0, h, w, 0))
            elif size == 1025 and k == size - 1:
                rects.append((0, 0, h, w // 2, 1))
            else:
                side = 2 if size == 1025 else 6
                i0, j0 = int(rng.integers(0, h)), int(rng.integers(0, w - 5 if size == 1025 else w))
                rects.append((i0, j0, min(h, i0 + int(rng.integers(1, side + 1))), min(w, j0 + int(rng.integers(1, side + 1))),
                              int(rng.integers(2, nc))))
    rects = np.array(rects, dtype=np.int32).reshape(-1, 5)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    painted = np.full((n, h, w), np.nan)
    last_row = np.full((h, w), -1)   # of the 1025-rectangle view: the row that painted each pixel last
    for v in range(n):
        for k in range(offsets[v], offsets[v + 1]):
            i0, j0, i1, j1, cls = rects[k].tolist()
            painted[v, i0:i1, j0:j1] = cls
            if v == n - 1:
                last_row[i0:i1, j0:j1] = k - offsets[v]
    # the pixels of that view end their walk in each of its three chunks, the single-row one included
    assert (last_row == 1024).any() and ((last_row >= 513) & (last_row < 1024)).any()
    assert ((last_row >= 1) & (last_row < 513)).any() and (last_row == 0).any()
    projs = [oracle_np.project_image(ids[v].astype(np.int64), painted[v].reshape(h, w, 1), F, check_null_image=True,
                                     neg1_is_last_face=neg1) for v in range(n)]
    want_counts = np.zeros(F, dtype=np.int64)
    want_summed = np.zeros((F, nc), dtype=np.int64)
    if F > 1:
        _, counts, want_summed = oracle_np.aggregate_index_sparse(projs, F, nc)
        want_counts = np.asarray(counts).reshape(-1)
    else:   # (aggregate_index_sparse squeezes a (1, 1) projection to a scalar: the same sums by hand)
        for p in projs:
            if np.isfinite(p[0, 0]):
                want_counts[0] += 1
                want_summed[0, int(p[0, 0])] += 1
    assert want_counts.sum() > 0

    hip.upload_mesh(np.zeros((3, 3), dtype=np.float32), np.zeros((F, 3), dtype=np.int32))

    def dense(keys, mult):
        out = np.zeros(F * nc, dtype=np.int64)
        out[keys] = mult
        return out.reshape(F, nc)

    got_counts = torch.zeros((F,), dtype=torch.int32, device=hip.device)
    acc = hip.new_pair_accumulator(nc, got_counts, neg1_is_last_face=neg1)
    acc.add_rects(ids, rects, offsets)
    got_keys, got_mult = acc.finish()
    np.testing.assert_array_equal(dense(got_keys, got_mult), want_summed)
    np.testing.assert_array_equal(got_counts.cpu().numpy(), want_counts)
    img_counts = torch.zeros((F,), dtype=torch.int32, device=hip.device)
    img_keys, img_mult = hip.project_index_pairs(ids, painted, nc, img_counts, neg1_is_last_face=neg1)
    np.testing.assert_array_equal(dense(img_keys, img_mult), want_summed)
    np.testing.assert_array_equal(img_counts.cpu().numpy(), want_counts)
    assert np.array_equal(got_keys, img_keys) and np.array_equal(got_mult, img_mult)
