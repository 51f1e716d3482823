#!/usr/bin/env python3
"""tools/region_detections_rate.py -- views/s of aggregating polygon (region) detections onto the mesh:

  region tables   TexturedPhotogrammetryMeshIndexPredictions with a segmentor that offers `label_regions`: the rings go
                  to the device, each face's winning pixel is tested there (gr_project_polygon_pairs); one class per
                  detection, as project_detections runs
  materialised    the base class with the same rings painted into the (h, w, C) bool mask on the host and uploaded --
                  only feasible at a REDUCED class count (`--classes-slow`, detection index modulo it; 12 MB per class and
                  4000 x 3000 view), over the first `--views-slow` views

Workload: C2 (terrain mesh, 50 views 4000 x 3000), 300 crown polygons of 16-64 vertices per view.  Times are HIP events
around the whole aggregation call, median of `--repeats` (5).  The region-table path is also run at the reduced class count
over the same views and compared with the materialised result.  Prints one JSON line and writes it to
profiles/region_detections_rate.json.

    python tools/region_detections_rate.py [--views 50] [--views-slow 2] [--classes-slow 8] [--repeats 5]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from geograypher_amd.cameras import SegmentorPhotogrammetryCameraSet  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMesh, TexturedPhotogrammetryMeshIndexPredictions  # noqa: E402
from geograypher_amd.predictors import Segmentor  # noqa: E402
from geograypher_amd.predictors.derived_segmentors import _ring_box, _ring_contains  # noqa: E402
from geograypher_amd.utils import synthetic  # noqa: E402

H, W = 3000, 4000


class Crowns(Segmentor):
    """Ring tables per view, keyed by file name; the class of detection k is k % num_classes."""

    def __init__(self, rings, num_classes, with_tables=True):
        self.rings, self.num_classes = rings, num_classes
        if with_tables:
            self.label_regions = self._label_regions

    def _kept(self, filename):
        out = []
        for k, v in self.rings[Path(filename).name]:
            box = _ring_box(v[:, 0], v[:, 1], H, W)
            if box is not None:
                out.append((k % self.num_classes, box, v))
        return sorted(out, key=lambda t: t[0])

    def _label_regions(self, filename, image_scale=1):
        if image_scale != 1:
            return None
        kept = self._kept(filename)
        boxes = np.array([(*box, cls) for cls, box, _ in kept], dtype=np.int32).reshape(-1, 5)
        vert_offsets = np.zeros(len(kept) + 1, dtype=np.int32)
        vert_offsets[1:] = np.cumsum([v.shape[0] for _, _, v in kept])
        return (boxes, vert_offsets, np.concatenate([v for _, _, v in kept])), (H, W)

    def segment_image(self, image, filename, image_scale):
        mask = np.zeros((H, W, self.num_classes), dtype=bool)
        for cls, box, v in self._kept(filename):
            mask[box[0]:box[2], box[1]:box[3], cls] |= _ring_contains(v[:, 0], v[:, 1], box)
        return mask


def crowns(rng, cams, per_view):
    rings, k = {}, 0
    for v in range(len(cams)):
        view = []
        for _ in range(per_view):
            nv = int(rng.integers(16, 65))
            t = np.sort(rng.uniform(0, 2 * np.pi, nv))
            rad = rng.uniform(40, 160) * rng.uniform(0.8, 1.2, nv)
            ci, cj = rng.uniform(0, H), rng.uniform(0, W)
            view.append((k, np.stack([ci + rad * np.sin(t), cj + rad * np.cos(t)], axis=1)))
            k += 1
        rings[cams.get_image_filename(v).name] = view
    return rings, k


def event_ms(fn, repeats):
    import torch

    times, out = [], None
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return out, statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--views-slow", type=int, default=2)
    ap.add_argument("--classes-slow", type=int, default=8)
    ap.add_argument("--per-view", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    points, faces = synthetic.terrain_mesh()
    cams = synthetic.config2_cameras(args.views)
    rings, n_det = crowns(np.random.default_rng(0), cams, args.per_view)
    sparse = TexturedPhotogrammetryMeshIndexPredictions((points, faces), log_level="ERROR")
    dense = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=sparse.backend)

    def fast(sub, nc):
        return sparse.aggregate_projected_images(SegmentorPhotogrammetryCameraSet(sub, Crowns(rings, nc)), n_classes=nc,
                                                 apply_distortion=False)

    def slow(sub, nc):
        return dense.aggregate_projected_images(SegmentorPhotogrammetryCameraSet(sub, Crowns(rings, nc, with_tables=False)),
                                                apply_distortion=False)

    fast(cams[0:2], n_det)  # warm-up: mesh upload, scratch, kernels
    full, ms_full = event_ms(lambda: fast(cams, n_det), args.repeats)
    sub = cams.get_subset_cameras(list(range(min(args.views_slow, len(cams)))))
    nc = args.classes_slow
    fast_k, ms_fast_k = event_ms(lambda: fast(sub, nc), args.repeats)
    slow_k, ms_slow_k = event_ms(lambda: slow(sub, nc), args.repeats)
    equal = bool(np.array_equal(fast_k[1]["summed_projections"].toarray(),
                                np.nan_to_num(np.asarray(slow_k[1]["summed_projections"])).astype(np.int64)))
    out = {
        "mesh_faces": int(faces.shape[0]), "image": f"{W}x{H}", "polygons_per_view": args.per_view, "vertices": "16-64",
        "timing": f"HIP events around the aggregation call, median of {args.repeats}",
        "region_views": len(cams), "region_classes": n_det, "region_views_per_s": round(1000.0 * len(cams) / ms_full, 2),
        "region_pairs": int(full[1]["summed_projections"].nnz),
        "materialised_views": len(sub), "materialised_classes": nc,
        "materialised_views_per_s": round(1000.0 * len(sub) / ms_slow_k, 3),
        "region_views_per_s_same_subset_and_classes": round(1000.0 * len(sub) / ms_fast_k, 2),
        "speedup_same_subset_and_classes": round(ms_slow_k / ms_fast_k, 1), "summed_equal": equal,
    }
    line = json.dumps(out)
    print(line)
    (ROOT / "profiles" / "region_detections_rate.json").write_text(line + "\n")


if __name__ == "__main__":
    main()
