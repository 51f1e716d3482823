#!/usr/bin/env python3
"""tools/face_sieve_rate.py -- what the face sieve (gr_face_sieve) costs and what it buys on the noisy
three-class labellings of tools/face_outlines_rate.py: the C2 mesh (1 201 250 faces over 400 m) and the C5 mesh (4 999 122 faces
over 800 m), crown-like disks of three species with 10 % of the faces given a class (or none) at random -- what a per-face argmax
looks like.  Thresholds: min_area_m2 1 and 10, each with and without filling unseen faces.

  device      HIP events round the binding's call (HipRaster.face_sieve) with every input already on the device, median and best
              of --repeats after a warm-up: `total_ms` the sieve; `labelling_ms` the same call with min_measure = 0, i.e. the
              adjacency (keys and one sort) and ONE component pass -- the events go round the call, so the adjacency is not
              separated from that first pass; `per_round_ms` = (total - labelling) / (rounds run), a round being the targets, the
              relabelling, the read-back and the next component pass; rounds run = changing rounds + 1, the last finding nothing
  what for    rounds, components before and after, and the rings and ring vertices of export_face_labels_vector before and after
  host        the numpy / scipy stand-in of tests/face_sieve_standin.py on this host's CPUs (--standin-meshes), for context; the
              tool ASSERTS that the device's three outputs equal it

Writes profiles/face_sieve_rate.json (and prints it as one JSON line).  No pass / fail bar on the rates: nobody has measured this
stage before.

    python tools/face_sieve_rate.py [--repeats 5] [--meshes c2 c5] [--standin-meshes c2 c5]
"""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

from face_outlines_rate import MESHES, crown_classes, timed  # noqa: E402

THRESHOLDS_M2 = (1.0, 10.0)


def exported(mesh, classes, points):
    """(rings, ring vertices, seconds) of export_face_labels_vector for int classes (-1: none)."""
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        mesh.export_face_labels_vector(np.where(classes < 0, np.nan, classes), Path(tmp, "map.geojson"), points_in_export_CRS=points)
        seconds = time.perf_counter() - t0
    stats = mesh.last_outline_stats
    return int(stats["rings"]), int(stats["edges"]), round(seconds, 3)    # a ring has as many vertices as edges


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--meshes", nargs="+", choices=sorted(MESHES), default=sorted(MESHES))
    ap.add_argument("--standin-meshes", nargs="*", choices=sorted(MESHES), default=sorted(MESHES))
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "face_sieve_rate.json")
    args = ap.parse_args()
    import torch

    import face_sieve_standin as fs
    from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh
    from geograypher_amd.utils import synthetic
    from geograypher_amd.utils.geometric import face_area_weights

    if not torch.cuda.is_available():
        raise SystemExit("face_sieve_rate: no GPU; a rate is measured on the device or not at all")
    res = {"classes": 3, "repeats": args.repeats, "runs": []}
    for name in args.meshes:
        n_side, extent = MESHES[name]
        points, faces = synthetic.terrain_mesh(n_side, extent)
        faces = np.ascontiguousarray(faces, dtype=np.int32)
        mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR")
        hip = mesh.backend
        _, noisy = crown_classes(points, faces, extent)
        weights = face_area_weights(points, faces)
        V = len(points)
        faces_d, cls_d, w_d = hip._dev(faces, torch.int32), hip._dev(noisy, torch.int32), hip._dev(weights, torch.int64)
        rings0, ring_vertices0, export0_s = exported(mesh, noisy, points)
        lab_med, lab_best = timed(lambda: hip.face_sieve(faces_d, cls_d, None, 0, n_vertices=V), args.repeats)
        for area in THRESHOLDS_M2:
            for fill in (False, True):
                mm = int(np.ceil(area * 1e6))
                call = lambda: hip.face_sieve(faces_d, cls_d, w_d, mm, fill, n_vertices=V)   # noqa: E731  (the weights were checked once)
                class_out, comp, stats = call()
                st = stats.cpu().numpy()
                med, best = timed(call, args.repeats)
                rounds_run = int(st[fs.ROUNDS]) + (0 if st[fs.ROUND_CAP] else 1)
                sieved = class_out.cpu().numpy()
                rings1, ring_vertices1, export1_s = exported(mesh, sieved, points)
                run = {"mesh": name, "faces": int(len(faces)), "vertices": V, "min_area_m2": area, "fill_unseen": fill,
                       "stats": dict(zip(("rounds", "components_before", "components_after", "faces_changed", "small_left", "degenerate",
                                          "fan_edges", "round_cap", "bad_faces"), (int(x) for x in st))),
                       "total_ms_median": med, "total_ms_best": best, "labelling_ms_median": lab_med, "labelling_ms_best": lab_best,
                       "per_round_ms": round((med - lab_med) / max(rounds_run, 1), 3), "rounds_run": rounds_run,
                       "mfaces_per_s": round(len(faces) / (med * 1e-3) / 1e6, 1),
                       "rings_before": rings0, "ring_vertices_before": ring_vertices0, "export_before_s": export0_s,
                       "rings_after": rings1, "ring_vertices_after": ring_vertices1, "export_after_s": export1_s}
                if name in args.standin_meshes:
                    t0 = time.perf_counter()
                    want = fs.sieve(faces, noisy, weights, mm, fill, n_vertices=V)
                    run["host_standin_s"] = round(time.perf_counter() - t0, 3)
                    for g, w, what in zip((sieved, comp.cpu().numpy(), st), want[:3], ("class_out", "comp", "stats")):
                        assert np.array_equal(g, w), f"the device's {what} differs from the stand-in"
                    run["device_equals_standin_on_every_array"] = True
                res["runs"].append(run)
                print(json.dumps(run), flush=True)
    res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
