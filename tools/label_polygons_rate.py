#!/usr/bin/env python3
"""tools/label_polygons_rate.py -- rate of label_polygons (gr_polygon_class_weights) on the C2 mesh (utils/synthetic.terrain_mesh:
1 201 250 faces) against a few thousand synthetic crown polygons of 16 to 64 vertices, in both modes.

  device      HIP events around the enqueued call with every input already on the device, best and median of --repeats after a
              warm-up; and end to end through TexturedPhotogrammetryMesh.label_polygons with a host clock (snap, area ratios,
              table, upload, kernel, read-back, labels)
  stand-in    the float64 restatement (tests/polygon_standin.py, per-pair Python on one core) on the first --standin-polygons
              polygons against the whole mesh, on this host's CPUs

A pair is a (face, polygon) whose boxes overlap: the unit both sides work in.  Writes profiles/label_polygons_rate.json (and prints
it as one JSON line).  No pass / fail bar: the reference publishes no figure for this stage and does not run at the pinned snapshot.

    python tools/label_polygons_rate.py [--polygons 3000] [--repeats 5] [--standin-polygons 4]
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
sys.path.insert(0, str(ROOT / "tests"))


def crowns(n, extent, seed=0):
    """n star-shaped (hence simple) crown outlines of 16 to 64 vertices, radius 2 to 6 m, scattered over the footprint."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        k = int(rng.integers(16, 65))
        cx, cy = rng.uniform(-extent / 2, extent / 2, 2)
        r = rng.uniform(2.0, 6.0) * (1.0 + 0.25 * rng.uniform(-1, 1, k))
        a = 2 * np.pi * (np.arange(k) + rng.uniform(-0.3, 0.3, k)) / k
        out.append(np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--polygons", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--standin-polygons", type=int, default=4)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "label_polygons_rate.json")
    args = ap.parse_args()
    import torch

    import polygon_standin as standin
    from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh
    from geograypher_amd.utils import synthetic
    from geograypher_amd.utils.geometric import PlanarPolygons

    if not torch.cuda.is_available():
        raise SystemExit("label_polygons_rate: no GPU; a rate is measured on the device or not at all")
    points, faces = synthetic.terrain_mesh()
    rng = np.random.default_rng(1)
    labels = rng.integers(0, 6, len(faces)).astype(np.float64)
    weighting = rng.uniform(0.1, 1.0, len(faces))
    polys = PlanarPolygons.from_sequence(crowns(args.polygons, 400.0))
    mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR")
    hip = mesh.backend

    res = {"mesh": "C2 terrain", "faces": int(len(faces)), "polygons": args.polygons, "ring_vertices": "16-64",
           "classes": 6, "repeats": args.repeats}

    # what the mesh class hands to the backend, captured once
    captured = {}
    real = hip.polygon_class_weights

    def capture(*a, **kw):
        captured["args"], captured["kw"] = a, kw
        return real(*a, **kw)

    hip.polygon_class_weights = capture
    mesh.label_polygon_weights(labels, polys, face_weighting=weighting, points_in_polygon_CRS=points)
    hip.polygon_class_weights = real
    host_args = captured["args"]
    dtypes = (torch.int64, torch.int32, torch.float64, torch.int64, torch.int64, torch.int32, torch.int32, torch.int64)
    dev_args = [hip._dev(a, dt) for a, dt in zip(host_args[:8], dtypes)]
    n_classes = host_args[8]

    for mode, within in (("sjoin", True), ("overlay", False)):
        weights, stats = real(*dev_args, n_classes, within=within)   # warm-up: code object load
        torch.cuda.synchronize()
        pairs = int(stats.cpu()[0])
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            real(*dev_args, n_classes, within=within)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        e2e = []
        for _ in range(max(2, args.repeats // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = mesh.label_polygons(labels, polys, face_weighting=weighting, sjoin_overlay=within, points_in_polygon_CRS=points)
            e2e.append(time.perf_counter() - t0)
        assert len(out) == args.polygons
        med = float(np.median(ms))
        res[mode] = {
            "pairs_tested": pairs, "pairs_contributing": int(stats.cpu()[1]),
            "device_ms_best": round(min(ms), 3), "device_ms_median": round(med, 3),
            "device_mpairs_per_s": round(pairs / (med * 1e-3) / 1e6, 2),
            "device_mfaces_per_s": round(len(faces) / (med * 1e-3) / 1e6, 1),
            "end_to_end_s_best": round(min(e2e), 3),
            "labelled_polygons": int(np.sum(np.isfinite(np.asarray(out, dtype=np.float64)))),
        }

    # the stand-in on this host, a few polygons against the whole mesh (the arguments captured from the mesh class, computed once)
    class Capture:
        def polygon_class_weights(self, *a, **kw):
            self.args = a
            return np.zeros((len(a[7]), a[8])), np.zeros(4, dtype=np.int64)

    k = args.standin_polygons
    sub = PlanarPolygons.from_sequence([polys.rings[i] for i in range(k)])   # (one ring per row here)
    sub_mesh = TexturedPhotogrammetryMesh((points, faces), backend=Capture(), log_level="ERROR")
    sub_mesh.label_polygon_weights(labels, sub, face_weighting=weighting, points_in_polygon_CRS=points)
    tri, cls, wgt, *table, n_cls = sub_mesh.backend.args
    for mode, within in (("sjoin", True), ("overlay", False)):
        t0 = time.perf_counter()
        w_np, st_np = standin.polygon_class_weights_np(tri, cls, wgt, tuple(table), n_cls, within)
        dt = time.perf_counter() - t0
        w_dev = mesh.label_polygon_weights(labels, sub, face_weighting=weighting, sjoin_overlay=within, points_in_polygon_CRS=points)
        res[mode].update({
            "standin_polygons": k, "standin_pairs": int(st_np[0]), "standin_s": round(dt, 3),
            "standin_mpairs_per_s": round(int(st_np[0]) / dt / 1e6, 5),
            "device_over_standin_pairs_rate": round(res[mode]["device_mpairs_per_s"] / (int(st_np[0]) / dt / 1e6), 1),
            "standin_max_rel_diff_to_device": float(np.max(np.abs(w_np - w_dev) / np.maximum(np.abs(w_np), 1e-300))),
        })
    res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    res["device"] = torch.cuda.get_device_name(0)
    res["reference_note"] = "the reference's label_polygons publishes no rate and does not run at the pinned snapshot"
    line = json.dumps(res)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
