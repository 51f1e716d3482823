#!/usr/bin/env python3
"""tools/vector_texture_rate.py -- rate of the vector-texture point query (gr_face_polygon_index, DESIGN.md "Vector textures") on
the C2 mesh (utils/synthetic.terrain_mesh: 1 201 250 faces over 400 m) and the C5 mesh (terrain_mesh(1582, 800): 4 999 122 faces
over 800 m), each against 3 000 and 30 000 synthetic crown polygons of 16 to 64 vertices.

  device      HIP events around the enqueued call (check=False: no read-back) with every input already on the device, median and
              best of --repeats after a warm-up -- with the chosen cell grid, and with the 1 x 1 grid (one list of all rows,
              walked by every face): what the index buys
  end to end  TexturedPhotogrammetryMesh.get_values_for_faces_from_vector with a host clock (snap, ring table, cell table,
              upload, kernel, read-back, column look-up)
  stand-in    the brute-force checker (tests/vector_standin.py, Python integers on one core) on the first --standin-faces
              faces, on this host's CPUs, and its agreement with the device on them

Writes profiles/vector_texture_rate.json (and prints it as one JSON line).  No pass / fail bar: the reference publishes no figure
for this stage, and geopandas runs neither here nor where this project is built.

    python tools/vector_texture_rate.py [--repeats 5] [--standin-faces 2000] [--meshes c2 c5]
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

MESHES = {"c2": (776, 400.0), "c5": (1582, 800.0)}


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


def timed(fn, repeats):
    import torch

    fn()   # warm-up: code object load
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(float(np.median(ms)), 3), round(min(ms), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--standin-faces", type=int, default=2000)
    ap.add_argument("--meshes", nargs="+", choices=sorted(MESHES), default=sorted(MESHES))
    ap.add_argument("--polygons", nargs="+", type=int, default=[3000, 30000])
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "vector_texture_rate.json")
    args = ap.parse_args()
    import torch

    import vector_standin as standin
    from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh
    from geograypher_amd.utils import synthetic
    from geograypher_amd.utils.geometric import PlanarPolygons, polygon_cell_table

    if not torch.cuda.is_available():
        raise SystemExit("vector_texture_rate: no GPU; a rate is measured on the device or not at all")
    res = {"ring_vertices": "16-64", "repeats": args.repeats, "runs": []}
    for name in args.meshes:
        n_side, extent = MESHES[name]
        points, faces = synthetic.terrain_mesh(n_side, extent)
        mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR")
        hip = mesh.backend
        for n_polygons in args.polygons:
            polys = PlanarPolygons.from_sequence(crowns(n_polygons, extent))
            column = {"crown": np.arange(1, n_polygons + 1, dtype=np.int64)}
            vq, table = mesh._snap_with_polygons(points, polys)
            chosen = polygon_cell_table(table[4])
            side = 3 * (1 << 42)
            one = polygon_cell_table(table[4], grid=[-side, -side, 2 * side + 1, 2 * side + 1, 1, 1])
            dev = [hip._dev(vq, torch.int64), hip._dev(faces, torch.int32)] + \
                  [hip._dev(t, dt) for t, dt in zip(table, (torch.int64, torch.int64, torch.int32, torch.int32, torch.int64))]
            run = {"mesh": name, "faces": int(len(faces)), "polygons": n_polygons}
            answers = {}
            for tag, cells in (("grid", chosen), ("one_cell", one)):
                cells_dev = (cells[0], hip._dev(cells[1], torch.int64), hip._dev(cells[2], torch.int32))
                out, stats = hip.face_polygon_index(*dev, cells_dev)
                answers[tag] = out.cpu().numpy()
                st = stats.cpu().numpy()
                med, best = timed(lambda: hip.face_polygon_index(*dev, cells_dev, check=False), args.repeats)
                run[tag] = {"cells": [int(cells[0][4]), int(cells[0][5])], "list_entries": int(len(cells[2])),
                            "longest_list": int(st[2]), "ring_walks": int(st[0]), "faces_labelled": int(st[1]),
                            "device_ms_median": med, "device_ms_best": best,
                            "device_mfaces_per_s": round(len(faces) / (med * 1e-3) / 1e6, 1)}
            run["grid_equals_one_cell"] = bool(np.array_equal(answers["grid"], answers["one_cell"]))
            run["one_cell_over_grid"] = round(run["one_cell"]["device_ms_median"] / run["grid"]["device_ms_median"], 1)
            e2e = []
            for _ in range(max(2, args.repeats // 2)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                labeled, _ = mesh.get_values_for_faces_from_vector((polys, column), "crown", points_in_polygon_CRS=points)
                e2e.append(time.perf_counter() - t0)
            run["end_to_end_s_best"] = round(min(e2e), 3)
            run["end_to_end_equals_device"] = bool(np.array_equal(labeled, np.where(answers["grid"] >= 0, answers["grid"] + 1, 0)))
            k = min(args.standin_faces, len(faces))
            t0 = time.perf_counter()
            want, _ = standin.face_polygon_index_np(vq, faces[:k], table)
            dt = time.perf_counter() - t0
            run["standin"] = {"faces": k, "s": round(dt, 3), "faces_per_s": round(k / dt, 1),
                              "equals_device": bool(np.array_equal(want, answers["grid"][:k]))}
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
    res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    res["device"] = torch.cuda.get_device_name(0)
    res["reference_note"] = "the reference's gpd.overlay of face centres publishes no rate and cannot run without geopandas"
    line = json.dumps(res)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
