#!/usr/bin/env python3
"""tools/ring_simplify_rate.py -- rate of the exact Douglas-Peucker on the device (gr_simplify_rings) on the
outlines of the three-class "clean" C2 labelling that tools/face_outlines_rate.py builds (crown-like disks on 1 201 250 faces),
traced by gr_class_outlines, simplified at 0.05 m, 0.5 m and 2 m with the junctions of the class map fixed (S9).

  device  HIP events around the binding's call (RingSimplifier.simplify: the host check of the tables, the call with its one word
          read back per pass, the read-back of M) with every input already on the device, median and best of --repeats after a warm-up
  host    an iterative float64 numpy Douglas-Peucker on the same rings, written here, on this host's CPUs in the same run: the
          distance to the closed chord, anchors as S2.  It is NOT exact (no tie-break, float rounding): its kept count is recorded
          for context and is not compared for equality.

Then ONE ring of --big-ring vertices (a noisy circle; its first pass is one chain over the whole device), the same two ways.

Records vertices in, vertices out, rings collapsed, passes and ms per call.  Writes profiles/ring_simplify_rate.json (and prints it
as one JSON line).  No pass / fail bar: nobody has measured this stage before, and shapely runs neither here nor where this project
is built.

    python tools/ring_simplify_rate.py [--repeats 5] [--tolerances 0.05 0.5 2]
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


def numpy_douglas_peucker(q, off, fixed, tol_steps):
    """Kept vertices of every ring by an explicit stack over chains, distances in float64: the number kept (rings that end with
    fewer than 3 vertices count as empty)."""
    kept_total = 0
    xy = q.astype(np.float64)
    t2 = float(tol_steps) ** 2
    for r in range(len(off) - 1):
        s, e = int(off[r]), int(off[r + 1])
        n = e - s
        if n < 3:
            continue
        p = xy[s:e]
        anchors = np.nonzero(fixed[s:e])[0]
        if len(anchors) == 0:
            anchors = np.array([np.lexsort((p[:, 1], p[:, 0]))[0]])
        p = np.roll(p, -int(anchors[0]), axis=0)
        p = np.vstack([p, p[:1]])                                  # the ring's end stands for the first anchor again
        ends = np.r_[(anchors - anchors[0]) % n, n]
        keep = np.zeros(n + 1, dtype=bool)
        keep[ends] = True
        stack = [(int(a), int(b)) for a, b in zip(ends[:-1], ends[1:])]
        while stack:
            a, b = stack.pop()
            if b - a < 2:
                continue
            ab, ap = p[b] - p[a], p[a + 1:b] - p[a]
            L2 = ab @ ab
            t = np.clip(ap @ ab / L2, 0.0, 1.0) if L2 > 0 else np.zeros(len(ap))
            d = ap - t[:, None] * ab
            d2 = np.einsum("ij,ij->i", d, d)
            k = int(np.argmax(d2))
            if d2[k] > t2:
                keep[a + 1 + k] = True
                stack += [(a, a + 1 + k), (a + 1 + k, b)]
        m = int(keep[:n].sum())
        kept_total += m if m >= 3 else 0
    return kept_total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tolerances", type=float, nargs="+", default=[0.05, 0.5, 2.0])
    ap.add_argument("--big-ring", type=int, default=1_000_000, help="vertices of the one-ring run (0: leave it out)")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "ring_simplify_rate.json")
    args = ap.parse_args()
    import torch

    from face_outlines_rate import MESHES, crown_classes, timed
    from geograypher_amd import _hip
    from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh
    from geograypher_amd.utils import synthetic
    from geograypher_amd.utils.geometric import shared_border_fixed, snap_points

    if not torch.cuda.is_available():
        raise SystemExit("ring_simplify_rate: no GPU; a rate is measured on the device or not at all")
    n_side, extent = MESHES["c2"]
    points, faces = synthetic.terrain_mesh(n_side, extent)
    hip = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR").backend
    vq = snap_points(points)
    classes = crown_classes(points, faces, extent)[0]
    traced = hip.class_outlines(hip._dev(vq, torch.int64), hip._dev(faces, torch.int32), hip._dev(classes, torch.int32), 3)
    ring_ids, off = traced[1].cpu().numpy().astype(np.int64), traced[2].cpu().numpy().astype(np.int64)
    q = np.ascontiguousarray(vq[ring_ids])
    t0 = time.perf_counter()
    fixed = shared_border_fixed(q, off)
    fixed_s = round(time.perf_counter() - t0, 3)
    q_d, off_d, fixed_d = hip._dev(q, torch.int64), hip._dev(off, torch.int64), hip._dev(fixed, torch.uint8)
    simplifier = hip.ring_simplifier()
    res = {"mesh": "c2", "faces": int(len(faces)), "classes": 3, "rings": int(len(off) - 1), "vertices_in": int(len(q)),
           "largest_ring": int(np.diff(off).max()), "fixed_vertices": int(fixed.sum()), "shared_border_fixed_host_s": fixed_s,
           "repeats": args.repeats, "runs": []}
    for tol in args.tolerances:
        keep, kept_index, out_off, stats = simplifier.simplify(q_d, off_d, tol, fixed_d)
        st = stats.cpu().numpy().tolist()
        run = {"tol_m": tol, "vertices_out": int(kept_index.shape[0]), "collapsed_rings": st[_hip.GR_SIMPLIFY_STAT_COLLAPSED],
               "passes": st[_hip.GR_SIMPLIFY_STAT_PASSES], "wide_comparisons": st[_hip.GR_SIMPLIFY_STAT_WIDE]}
        run["device_ms_median"], run["device_ms_best"] = timed(lambda: simplifier.simplify(q_d, off_d, tol, fixed_d), args.repeats)
        run["device_mvertices_per_s"] = round(len(q) / (run["device_ms_median"] * 1e-3) / 1e6, 1)
        t0 = time.perf_counter()
        run["host_numpy_kept"] = numpy_douglas_peucker(q, off, fixed, round(tol / 1e-6))
        run["host_numpy_s"] = round(time.perf_counter() - t0, 3)
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    # ONE ring of --big-ring vertices, one chain in its first pass: a circle of 200 m radius with 0.3 m of radial noise
    if args.big_ring >= 3:
        rng = np.random.default_rng(1)
        angle = np.arange(args.big_ring) * (2 * np.pi / args.big_ring)
        radius = 200.0 + rng.uniform(-0.3, 0.3, args.big_ring)
        big = np.rint(np.column_stack([radius * np.cos(angle), radius * np.sin(angle)]) / 1e-6).astype(np.int64)
        big_off, no_fixed = np.array([0, len(big)], dtype=np.int64), np.zeros(len(big), dtype=np.uint8)
        big_d, big_off_d = hip._dev(big, torch.int64), hip._dev(big_off, torch.int64)
        res["big_ring"] = {"vertices_in": int(len(big)), "runs": []}
        for tol in args.tolerances:
            keep, kept_index, out_off, stats = simplifier.simplify(big_d, big_off_d, tol)
            st = stats.cpu().numpy().tolist()
            run = {"tol_m": tol, "vertices_out": int(kept_index.shape[0]), "passes": st[_hip.GR_SIMPLIFY_STAT_PASSES]}
            run["device_ms_median"], run["device_ms_best"] = timed(lambda: simplifier.simplify(big_d, big_off_d, tol), args.repeats)
            run["device_mvertices_per_s"] = round(len(big) / (run["device_ms_median"] * 1e-3) / 1e6, 1)
            t0 = time.perf_counter()
            run["host_numpy_kept"] = numpy_douglas_peucker(big, big_off, no_fixed, round(tol / 1e-6))
            run["host_numpy_s"] = round(time.perf_counter() - t0, 3)
            res["big_ring"]["runs"].append(run)
            print(json.dumps(run), flush=True)
    res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    res["device"] = torch.cuda.get_device_name(0)
    res["reference_note"] = "shapely's simplify publishes no rate and cannot run here; the float64 baseline is not exact and is not compared"
    line = json.dumps(res)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
