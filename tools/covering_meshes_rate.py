#!/usr/bin/env python3
"""tools/covering_meshes_rate.py -- rate of the covering meshes (gr_points_bounds, gr_cover_grid, export_covering_meshes) on the
C5 mesh's vertices (utils/synthetic.terrain_mesh(1582, 800): 2 502 724 points) at the entry point's N = 50, with subsample 2 (the
entry point's) and None.

  device      HIP events around each of the two enqueued calls with the points already on the device, best and median of
              --repeats after a warm-up; the grid kernel's bytes/s (24 bytes per visited row) as a share of the 8 TB/s peak; and
              end to end through utils.geometric.covering_meshes from host points with a host clock (upload, both kernels, tables,
              read-back, Delaunay)
  stand-in    the per-cell numpy form of the rule (tests/covering_standin.py) on the first --standin-points points, on this host's
              CPUs, and that time scaled linearly to the full vertex count -- an EXTRAPOLATION, marked as one

Writes profiles/covering_meshes_rate.json (and prints it as one JSON line).  No pass / fail bar.

    python tools/covering_meshes_rate.py [--repeats 9] [--standin-points 200000]
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

PEAK_BYTES_PER_S = 8e12   # MI355X HBM3E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--standin-points", type=int, default=200_000)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "covering_meshes_rate.json")
    args = ap.parse_args()
    import torch

    import covering_standin as standin
    from geograypher_amd._hip import default_backend
    from geograypher_amd.utils import synthetic
    from geograypher_amd.utils.geometric import covering_meshes

    if not torch.cuda.is_available():
        raise SystemExit("covering_meshes_rate: no GPU; a rate is measured on the device or not at all")
    points, _ = synthetic.terrain_mesh(1582, 800.0)
    points = np.ascontiguousarray(points, dtype=np.float64)
    hip = default_backend()
    dev = hip._dev(points, torch.float64)
    res = {"mesh": "C5 terrain vertices", "points": int(len(points)), "N": args.n, "repeats": args.repeats}

    def timed(fn):
        fn()   # warm-up: code object load, scratch
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return round(min(ms), 4), round(float(np.median(ms)), 4)

    for subsample in (2, None):
        stride = 1 if subsample is None else subsample
        rows = len(points[::stride])
        bounds = hip.points_bounds(dev, stride)[0].cpu().numpy()
        tabs = [hip._dev(t, torch.float64) for t in standin.bound_tables(bounds, args.n)]
        b_best, b_med = timed(lambda: hip.points_bounds(dev, stride))
        g_best, g_med = timed(lambda: hip.cover_grid(dev, *tabs, stride=stride))
        e2e = []
        for _ in range(max(3, args.repeats // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            (up, faces), _ = covering_meshes(points, args.n, z_buffer=(0, 1.0), subsample=subsample, backend=hip)
            e2e.append(time.perf_counter() - t0)
        k = min(args.standin_points, len(points))
        t0 = time.perf_counter()
        sb, _ = standin.points_bounds_np(points[:k], stride)
        standin.cover_grid_np(points[:k], *standin.bound_tables(sb, args.n), stride=stride)
        dt = time.perf_counter() - t0
        gbs = 24.0 * rows / (g_med * 1e-3)
        res["subsample_%s" % subsample] = {
            "visited_rows": rows, "vertices_per_surface": int(len(up)), "faces_per_surface": int(len(faces)),
            "bounds_ms_best": b_best, "bounds_ms_median": b_med, "grid_ms_best": g_best, "grid_ms_median": g_med,
            "grid_bytes_per_s": round(gbs, 0), "grid_share_of_8TBps_peak": round(gbs / PEAK_BYTES_PER_S, 4),
            "end_to_end_s_best": round(min(e2e), 4), "end_to_end_s_median": round(float(np.median(e2e)), 4),
            "standin_points": k, "standin_s": round(dt, 3),
            "standin_s_extrapolated_linearly_to_all_points": round(dt * len(points) / k, 3),
            "standin_note": "numpy stand-in on the host at standin_points, scaled linearly in V: an extrapolation, not a measurement",
        }
    res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    res["device"] = torch.cuda.get_device_name(0)
    res["reference_note"] = "the reference's export_covering_meshes publishes no rate and is not run here"
    line = json.dumps(res)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
