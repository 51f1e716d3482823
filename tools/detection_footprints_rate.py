#!/usr/bin/env python3
"""tools/detection_footprints_rate.py -- rate of the member-outline trace (gr_member_outlines) on two sparse
face x class matrices, each produced by the projection path itself (`aggregate_projected_images` on the device):

  a  detection footprints: the C2 mesh (1 201 250 faces), 50 views of 4000 x 3000 with 300 rectangle detections each, every
     detection a class of its own (15 000 columns)
  b  image footprints: the C3 visibility matrix, the same mesh under 500 views, every view a class (what
     `annotation_image_selection` builds): the ground every photo sees

  device      HIP events around the binding's call (HipRaster.member_outlines: the call and its two synchronisations) with every input
              already on the device, median and best of --repeats after a warm-up
  end to end  TexturedPhotogrammetryMesh.export_face_labels_vector(sparse matrix) to a .geojson with a host clock (CSR conversion, snap,
              upload, trace, read-back, exact areas, the nesting of X8, file); `outlines_s` is the part up to and including the exact
              areas (face_label_outlines), the rest is X8, the polygons and json
  per column  what the code before this call had to do: HipRaster.class_outlines with n_classes = 1 on 64 evenly spaced non-empty
              columns (HIP events, each once after a warm-up; the face_class arrays are built and uploaded outside the clock).  The
              median TIMES the number of non-empty columns is reported as `per_column_extrapolated_s` -- an EXTRAPOLATION from 64
              columns, not a measurement of the whole
  host        a vectorised numpy restatement of Y1-Y4 and X4-X6 on this host's CPUs (tools/face_outlines_rate.numpy_outlines on the
              members' faces)

The tool ASSERTS that every array of the device equals the numpy restatement's.  Writes profiles/detection_footprints_rate.json (a
run replaces the entry of its matrix and keeps the others) and prints it as one JSON line.  No pass / fail bar on the rates.

    python tools/detection_footprints_rate.py [--repeats 5] [--matrices a b] [--views-b 500]
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from face_outlines_rate import numpy_outlines, timed  # noqa: E402


class RandomRectangles:
    """300 crown-sized boxes per view (100 to 300 pixels a side at 4 cm per pixel), every box a class of its own."""

    def __init__(self, filenames, shape, per_view=300, seed=0):
        rng = np.random.default_rng(seed)
        self.shape, self.rects = shape, {}
        for k, name in enumerate(filenames):
            h, w = rng.integers(100, 301, per_view), rng.integers(100, 301, per_view)
            i0, j0 = rng.integers(0, shape[0] - h), rng.integers(0, shape[1] - w)
            self.rects[str(name)] = np.column_stack([i0, j0, i0 + h, j0 + w, k * per_view + np.arange(per_view)]).astype(np.int32)
        self.num_classes = len(filenames) * per_view

    def label_rectangles(self, filename, image_scale=1):
        return (self.rects[str(filename)], self.shape) if image_scale == 1 else None


class WholeImage:
    """Every pixel of view k holds k: the visibility matrix of `annotation_image_selection`."""

    def __init__(self, filenames, shape):
        self.shape, self.index = shape, {str(name): k for k, name in enumerate(filenames)}
        self.num_classes = len(filenames)

    def label_rectangles(self, filename, image_scale=1):
        h, w = self.shape
        return (np.array([[0, 0, h, w, self.index[str(filename)]]], dtype=np.int32), self.shape) if image_scale == 1 else None


def numpy_members(vq, faces, face_ptr, face_members, C):
    """Y1-Y4 and X4-X6 in vectorised int64 numpy: a member is a face with the member's class."""
    face_of = np.repeat(np.arange(len(faces)), np.diff(face_ptr))
    got = list(numpy_outlines(vq, faces[face_of], face_members, C))
    got[4][5] = int((~((faces >= 0) & (faces < len(vq))).all(axis=1)).sum())   # bad faces count faces, not members
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--matrices", nargs="+", choices=("a", "b"), default=["a", "b"])
    ap.add_argument("--views-a", type=int, default=50)
    ap.add_argument("--views-b", type=int, default=500)
    ap.add_argument("--columns", type=int, default=64, help="columns the per-column path is timed on")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "detection_footprints_rate.json")
    args = ap.parse_args()
    import tempfile

    import torch

    from geograypher_amd.cameras.segmentor import SegmentorPhotogrammetryCameraSet
    from geograypher_amd.meshes.derived_meshes import TexturedPhotogrammetryMeshIndexPredictions
    from geograypher_amd.utils import synthetic
    from geograypher_amd.utils.geometric import csr_members, snap_points

    if not torch.cuda.is_available():
        raise SystemExit("detection_footprints_rate: no GPU; a rate is measured on the device or not at all")
    res = json.loads(args.out.read_text()) if args.out.is_file() else {}
    res.setdefault("runs", {})
    res["repeats"] = args.repeats
    points, faces = synthetic.terrain_mesh()
    mesh = TexturedPhotogrammetryMeshIndexPredictions((points, faces), log_level="ERROR")
    hip = mesh.backend
    vq = snap_points(points)
    faces32 = np.ascontiguousarray(faces, dtype=np.int32)
    vq_d, faces_d = hip._dev(vq, torch.int64), hip._dev(faces32, torch.int32)
    for name in args.matrices:
        cams = synthetic.config2_cameras(args.views_a) if name == "a" else synthetic.config3_cameras(args.views_b)
        filenames = [cams.get_image_filename(i, absolute=True) for i in range(len(cams))]
        segmentor = (RandomRectangles if name == "a" else WholeImage)(filenames, (3000, 4000))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, info = mesh.aggregate_projected_images(SegmentorPhotogrammetryCameraSet(cams, segmentor=segmentor), n_classes=segmentor.num_classes)
        matrix = info["summed_projections"]
        run = {"matrix": name, "faces": int(len(faces)), "views": len(cams), "columns": int(matrix.shape[1]),
               "projection_s": round(time.perf_counter() - t0, 3)}
        face_ptr, face_members = csr_members(matrix)
        nnz, C = int(len(face_members)), int(matrix.shape[1])
        ptr_d, mem_d = hip._dev(face_ptr, torch.int64), hip._dev(face_members, torch.int32)
        got = hip.member_outlines(vq_d, faces_d, ptr_d, mem_d, C)
        E, R = int(got[1].shape[0]), int(got[3].shape[0])
        run.update(nnz=nnz, ring_vertices=E, rings=R, stats=got[4].cpu().numpy().tolist(), calls_at_default_capacity=hip.last_outline_calls)
        med, best = timed(lambda: hip.member_outlines(vq_d, faces_d, ptr_d, mem_d, C, capacity=E), args.repeats)
        run["device_ms_median"], run["device_ms_best"] = med, best
        run["device_mmembers_per_s"] = round(nnz / (med * 1e-3) / 1e6, 1)
        print(json.dumps(run), flush=True)
        # the per-column path of the code before this call, on a sample of the non-empty columns
        present = np.unique(face_members)
        sample = present[np.linspace(0, len(present) - 1, min(args.columns, len(present))).astype(np.int64)]
        face_of = np.repeat(np.arange(len(faces)), np.diff(face_ptr))
        per_column = []
        for k, column in enumerate(sample.tolist()):
            alone = np.full(len(faces), -1, dtype=np.int32)
            alone[face_of[face_members == column]] = 0
            alone_d = hip._dev(alone, torch.int32)
            if k == 0:
                hip.class_outlines(vq_d, faces_d, alone_d, 1)   # warm-up
                torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            hip.class_outlines(vq_d, faces_d, alone_d, 1)
            b.record()
            b.synchronize()
            per_column.append(a.elapsed_time(b))
        run["non_empty_columns"] = int(len(present))
        run["per_column_sampled"] = len(per_column)
        run["per_column_ms_median"] = round(float(np.median(per_column)), 3)
        run["per_column_extrapolated_s"] = round(float(np.median(per_column)) * 1e-3 * len(present), 3)
        run["per_column_note"] = f"EXTRAPOLATED: the median of {len(per_column)} sampled columns times {len(present)} non-empty columns"
        print(json.dumps(run), flush=True)
        with tempfile.TemporaryDirectory() as tmp:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mesh.face_label_outlines(matrix, points_in_export_CRS=points)
            run["outlines_s"] = round(time.perf_counter() - t0, 3)
            t0 = time.perf_counter()
            mesh.export_face_labels_vector(matrix, Path(tmp, "footprints.geojson"), points_in_export_CRS=points)
            run["end_to_end_s"] = round(time.perf_counter() - t0, 3)
            run["geojson_bytes"] = Path(tmp, "footprints.geojson").stat().st_size
        run["nesting_polygons_json_share"] = round(max(run["end_to_end_s"] - run["outlines_s"], 0.0) / run["end_to_end_s"], 3)
        print(json.dumps(run), flush=True)
        t0 = time.perf_counter()
        want = numpy_members(vq, faces32, face_ptr, face_members, C)
        run["host_numpy_s"] = round(time.perf_counter() - t0, 3)
        for g, w, what in zip(got, want, ("canon", "ring_vertices", "ring_offsets", "ring_class", "stats")):
            assert np.array_equal(g.cpu().numpy(), w), f"the device's {what} differs from the numpy restatement"
        run["device_equals_numpy_on_every_array"] = True
        res["runs"][name] = run
        print(json.dumps(run), flush=True)
        res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
        res["device"] = torch.cuda.get_device_name(0)
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
