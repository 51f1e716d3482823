#!/usr/bin/env python3
"""tools/nearest_points_rate.py -- what the nearest-point call (gr_nearest_points) costs on the transfers it
was built for: the C2 mesh (1 201 250 faces over 400 m) and the C5 mesh (4 999 122 faces over 800 m) against the same mesh
decimated to a quarter of its vertices (`TexturedPhotogrammetryMesh.decimate(0.25)`), face centres and vertices, in both
directions (decimated -> full: what `values_from_mesh` does behind a decimated aggregation; full -> decimated: the reference's
`transfer_texture`).

  device      HIP events round the binding's call (HipRaster.nearest_points, dist2 included) with both point sets already on the
              device, median and best of --repeats after a warm-up; the call's read-backs (the bounds, one word per level) are
              inside.  `stats`: levels, carried queries, and probes (runs of cells looked up) and candidates (distances evaluated)
              per query.
  sweep       (--sweep-meshes) the constant c of the cell rule cell = c sqrt(e1 e2 / R), given to the call as `cell`, times
              max_rings in {1, 2, 3}: the median of each, and which pair was fastest.  The defaults (c = 1.5, max_rings = 2) are
              compared with it.
  host        scipy's cKDTree on this host's CPUs, build and query timed separately, query with workers=16, for context; the tool
              ASSERTS that the device names the tree's row on every query whose nearest ref is unique (the tree's distance to its
              second neighbour is greater than to its first).

Writes profiles/nearest_points_rate.json (and prints it as one JSON line).  No pass / fail bar on the rates: nobody has measured
this stage before.

    python tools/nearest_points_rate.py [--repeats 5] [--meshes c2 c5] [--sweep-meshes c2] [--kdtree-meshes c2 c5]
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

from face_outlines_rate import MESHES, timed  # noqa: E402

SWEEP_CONSTANTS = (0.75, 1.0, 1.5, 2.0, 3.0)
SWEEP_RINGS = (1, 2, 3)
WORKERS = 16


def centres(points, faces):
    p = np.asarray(points, dtype=np.float64)
    return ((p[faces[:, 0]] + p[faces[:, 1]]) + p[faces[:, 2]]) / 3.0


def rule_cell(ref, c):
    e = np.sort(ref.max(axis=0) - ref.min(axis=0))
    return float(c * np.sqrt(e[2] * e[1] / len(ref)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--meshes", nargs="+", choices=sorted(MESHES), default=sorted(MESHES))
    ap.add_argument("--sweep-meshes", nargs="*", choices=sorted(MESHES), default=["c2"])
    ap.add_argument("--kdtree-meshes", nargs="*", choices=sorted(MESHES), default=sorted(MESHES))
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "nearest_points_rate.json")
    args = ap.parse_args()
    import torch

    from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh
    from geograypher_amd.utils import synthetic
    from geograypher_amd.utils.geometric import named_nearest_stats

    if not torch.cuda.is_available():
        raise SystemExit("nearest_points_rate: no GPU; a rate is measured on the device or not at all")
    res = {"repeats": args.repeats, "kdtree_workers": WORKERS, "runs": [], "sweeps": []}
    for name in args.meshes:
        n_side, extent = MESHES[name]
        points, faces = synthetic.terrain_mesh(n_side, extent)
        faces = np.ascontiguousarray(faces, dtype=np.int64)
        mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR")
        hip = mesh.backend
        t0 = time.perf_counter()
        small_points, small_faces = mesh.decimate(0.25)
        decimate_s = round(time.perf_counter() - t0, 3)
        sets = {"face_centres": (centres(small_points, small_faces), centres(points, faces)),
                "vertices": (np.asarray(small_points, dtype=np.float64), np.asarray(points, dtype=np.float64))}
        for what, (small, full) in sets.items():
            for direction, ref, query in (("decimated_to_full", small, full), ("full_to_decimated", full, small)):
                ref_d, query_d = hip._dev(ref, torch.float64), hip._dev(query, torch.float64)
                call = lambda **kw: hip.nearest_points(ref_d, query_d, return_dist2=True, **kw)   # noqa: E731
                index, dist2, stats = call()
                st = named_nearest_stats(stats)
                med, best = timed(call, args.repeats)
                Q = len(query)
                run = {"mesh": name, "points": what, "direction": direction, "R": int(len(ref)), "Q": int(Q), "decimate_s": decimate_s,
                       "ms_median": med, "ms_best": best, "mqueries_per_s": round(Q / (med * 1e-3) / 1e6, 1),
                       "levels": st["levels"], "carried": st["carried"], "cell": st["cell"],
                       "probes_per_query": round(st["cells_probed"] / Q, 2), "candidates_per_query": round(st["candidates"] / Q, 2)}
                if name in args.kdtree_meshes:
                    from scipy.spatial import cKDTree

                    t0 = time.perf_counter()
                    tree = cKDTree(ref)
                    run["kdtree_build_s"] = round(time.perf_counter() - t0, 3)
                    t0 = time.perf_counter()
                    d, rows = tree.query(query, k=2, workers=WORKERS)
                    run["kdtree_query_k2_s"] = round(time.perf_counter() - t0, 3)
                    t0 = time.perf_counter()
                    tree.query(query, workers=WORKERS)
                    run["kdtree_query_s"] = round(time.perf_counter() - t0, 3)
                    unique = d[:, 1] > d[:, 0]
                    got = index.cpu().numpy()
                    assert np.array_equal(got[unique], rows[unique, 0]), "the device differs from the KD-tree where the nearest ref is unique"
                    run["kdtree_unique_share"] = round(float(unique.mean()), 6)
                    run["device_equals_kdtree_on_every_unique_query"] = True
                res["runs"].append(run)
                print(json.dumps(run), flush=True)
                if name in args.sweep_meshes and what == "face_centres":
                    table = {}
                    for c in SWEEP_CONSTANTS:
                        for rings in SWEEP_RINGS:
                            cell = rule_cell(ref, c)
                            table[f"c={c},rings={rings}"] = timed(lambda: call(cell=cell, max_rings=rings), 3)[0]
                    fastest = min(table, key=table.get)
                    sweep = {"mesh": name, "points": what, "direction": direction, "ms_median": table, "fastest": fastest,
                             "defaults_ms": table["c=1.5,rings=2"]}
                    res["sweeps"].append(sweep)
                    print(json.dumps(sweep), flush=True)
                del ref_d, query_d
    res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
