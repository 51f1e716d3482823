#!/usr/bin/env python3
"""tools/detections_rate.py -- views/s of the two reference workflows that aggregate rectangle labels through
TexturedPhotogrammetryMeshIndexPredictions, each on the rectangle path (tables looked up on the device,
gr_project_rect_pairs) and on the materialised path (the per-pixel label image built on the host, uploaded and read by
gr_project_index_pairs):

  detections   project_detections: C2 (terrain mesh, 50 views 4000 x 3000), 50-300 random boxes per view from a CSV
               (TabularRectangleSegmentor, one class per detection)
  image IDs    annotation_image_selection: C3 poses (500 views 4000 x 3000), ImageIDSegmentor, n_classes = 500; the
               materialised path runs over the first 50 views only (a 96 MB int64 image per view)

Both at scale 1, as the entrypoints run.  Every result pair is checked for equality.  Prints one JSON line.

    python tools/detections_rate.py [--views-c2 50] [--views-ids 500] [--views-ids-slow 50]
"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from geograypher_amd.cameras import SegmentorPhotogrammetryCameraSet  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMeshIndexPredictions  # noqa: E402
from geograypher_amd.predictors import ImageIDSegmentor, Segmentor, TabularRectangleSegmentor  # noqa: E402
from geograypher_amd.utils import synthetic  # noqa: E402


class PerPixel(Segmentor):
    """The segmentor without `label_rectangles`: the aggregation builds and uploads its per-pixel image."""

    def __init__(self, seg):
        self.seg, self.num_classes = seg, getattr(seg, "num_classes", None)

    def segment_image(self, image, filename, image_scale):
        return self.seg.segment_image(image, filename=filename, image_scale=image_scale)


def timed(mesh, cams, seg, n_classes):
    import torch

    wrapped = SegmentorPhotogrammetryCameraSet(cams, seg)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = mesh.aggregate_projected_images(wrapped, n_classes=n_classes, apply_distortion=False)
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def same(a, b):
    return all((a[1][k] != b[1][k]).nnz == 0 for k in ("summed_projections", "projection_counts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views-c2", type=int, default=50)
    ap.add_argument("--views-ids", type=int, default=500)
    ap.add_argument("--views-ids-slow", type=int, default=50)
    args = ap.parse_args()
    from PIL import Image

    points, faces = synthetic.terrain_mesh()
    mesh = TexturedPhotogrammetryMeshIndexPredictions((points, faces), log_level="ERROR")
    out = {"mesh_faces": int(faces.shape[0]), "image": "4000x3000"}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        # detections: one CSV of 50-300 boxes per view
        cams = synthetic.config2_cameras(args.views_c2)
        rng = np.random.default_rng(0)
        lines, n_boxes = ["image_path,xmin,ymin,xmax,ymax,score"], 0
        for v in range(len(cams)):
            n = int(rng.integers(50, 301))
            n_boxes += n
            for _ in range(n):
                x0, y0 = rng.uniform(0, 4000), rng.uniform(0, 3000)
                lines.append(f"{cams.get_image_filename(v).name},{x0:.1f},{y0:.1f},{x0 + rng.uniform(20, 400):.1f},"
                             f"{y0 + rng.uniform(20, 400):.1f},0.9")
        (tmp / "det.csv").write_text("\n".join(lines) + "\n")
        seg = TabularRectangleSegmentor(tmp / "det.csv", (3000, 4000), split_bbox=False)
        timed(mesh, cams[0:2], seg, seg.num_classes)  # warm-up: mesh upload, scratch, kernels
        fast, t_fast = timed(mesh, cams, seg, seg.num_classes)
        slow, t_slow = timed(mesh, cams, PerPixel(seg), seg.num_classes)
        out.update(detections_views=len(cams), detections_boxes=n_boxes, detections_classes=seg.num_classes,
                   detections_rect_views_per_s=round(len(cams) / t_fast, 2),
                   detections_image_views_per_s=round(len(cams) / t_slow, 2),
                   detections_speedup=round(t_slow / t_fast, 1), detections_equal=same(fast, slow))

        # image IDs: every view's file is a link to one 4000 x 3000 PNG (the segmentor reads the header only)
        cams = synthetic.config3_cameras(args.views_ids)
        Image.fromarray(np.zeros((3000, 4000), dtype=np.uint8)).save(tmp / "blank.png")
        for v, cam in enumerate(cams.cameras):
            cam.image_filename = tmp / f"view_{v:04d}.png"
            cam.image_filename.symlink_to(tmp / "blank.png")
        ids_seg = ImageIDSegmentor(cams.get_image_filename(None, absolute=True))
        nc = len(cams)
        fast, t_fast = timed(mesh, cams, ids_seg, nc)
        k = min(args.views_ids_slow, len(cams))
        sub = cams.get_subset_cameras(list(range(k)))
        fast_k, t_fast_k = timed(mesh, sub, ids_seg, nc)
        slow_k, t_slow_k = timed(mesh, sub, PerPixel(ids_seg), nc)
        out.update(image_id_views=len(cams), image_id_rect_views_per_s=round(len(cams) / t_fast, 2),
                   image_id_image_views=k, image_id_image_views_per_s=round(k / t_slow_k, 2),
                   image_id_rect_views_per_s_same_subset=round(k / t_fast_k, 2),
                   image_id_speedup_same_subset=round(t_slow_k / t_fast_k, 1), image_id_equal=same(fast_k, slow_k),
                   image_id_observations=int(fast[1]["projection_counts"].sum()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
