#!/usr/bin/env python3
"""tools/top_down_raster_rate.py -- rate of the top-down raster of a mesh (gr_nadir_raster) on the C2 terrain
mesh (utils/synthetic.terrain_mesh: 1 201 250 faces over 400 m, one sheet) and the forest scene (utils/synthetic.forest_scene: the
same terrain under 20 000 trees, 2 361 250 faces, overlap in plan view), on north-up grids of 1 m, 0.2 m and 0.05 m cells.

  device      HIP events around the binding's call (NadirRasterizer.window over the whole grid: the two planes' allocation, the
              call with its one read-back, the bad-face word's read-back) with the mesh already on the device, median and best of
              --repeats after a warm-up; cells per second of the median; the statistics words; the same at small_cells = 16,
              item_rows = 8; and with --sweep a table of (small_cells, item_rows) pairs, median of 3: what the defaults rest on
  route       for the class raster, the route the tree offered before this call: export_face_labels_vector (trace on the device,
              nesting on the host) and burn_polygons of its rows on the same grid, each with a host clock, on the C2 mesh with
              crown classes (tools/face_outlines_rate.crown_classes, "clean"), beside export_face_labels_raster on the same labelling
  host        tests/nadir_standin.py, Python integers and floats, on a 256 x 256 window of the 1 m grid -- and the tool ASSERTS that
              the device's planes and statistics on that window equal it bit for bit

Writes profiles/top_down_raster_rate.json (and prints it as one JSON line).  No pass / fail bar on the rates.

    python tools/top_down_raster_rate.py [--repeats 5] [--scenes c2 forest] [--cells 1 0.2 0.05] [--sweep]
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
sys.path.insert(0, str(ROOT / "tests"))

SWEEP = ((16, 8), (64, 8), (128, 8), (256, 8), (512, 8), (1024, 8), (128, 4), (128, 16), (256, 16), (256, 32), (512, 16))   # (small_cells, item_rows)
STAT_NAMES = ("faces", "bad_index", "zero_area", "nonfinite_z", "empty_box", "items", "tests", "inside", "skipped", "covered")


def timed(fn, repeats):
    import torch

    fn()   # warm-up: code object load, scratch growth
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
    ap.add_argument("--scenes", nargs="+", choices=["c2", "forest"], default=["c2", "forest"])
    ap.add_argument("--cells", nargs="+", type=float, default=[1.0, 0.2, 0.05])
    ap.add_argument("--sweep", action="store_true", help="also time the (small_cells, item_rows) pairs of SWEEP")
    ap.add_argument("--no-route", action="store_true", help="skip the vector route and the stand-in")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "top_down_raster_rate.json")
    args = ap.parse_args()
    import torch

    from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh
    from geograypher_amd.utils import synthetic
    from geograypher_amd.utils.geospatial import burn_polygons, grid_from_bounds, points_to_cell_units
    from geograypher_amd.utils.raster import invert_affine

    if not torch.cuda.is_available():
        raise SystemExit("top_down_raster_rate: no GPU; a rate is measured on the device or not at all")
    res = {"repeats": args.repeats, "runs": []}
    terrain = synthetic.terrain_mesh(776, 400.0)
    for scene in args.scenes:
        points, faces = terrain if scene == "c2" else synthetic.forest_scene()
        faces = np.ascontiguousarray(faces, dtype=np.int32)
        mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR")
        hip = mesh.backend
        for cell in args.cells:
            (H, W), transform = grid_from_bounds(points, cell)
            vq = points_to_cell_units(points[:, :2], invert_affine(transform))
            rasterizer = hip.nadir_rasterizer(vq, np.ascontiguousarray(points[:, 2]), faces)
            run = {"scene": scene, "faces": int(len(faces)), "cell_m": cell, "height": H, "width": W, "cells": H * W}
            for label, kw in (("default", {}), ("small_cells_16_item_rows_8", dict(small_cells=16, item_rows=8))):
                stats = rasterizer.window(0, 0, W, H, **kw)[2].cpu().numpy()
                med, best = timed(lambda: rasterizer.window(0, 0, W, H, **kw), args.repeats)
                run[label] = {"device_ms_median": med, "device_ms_best": best, "mcells_per_s": round(H * W / (med * 1e-3) / 1e6, 1),
                              "mfaces_per_s": round(len(faces) / (med * 1e-3) / 1e6, 1), "stats": dict(zip(STAT_NAMES, stats.tolist()))}
            if args.sweep:
                run["sweep_ms_median_of_3"] = [[s, r, timed(lambda: rasterizer.window(0, 0, W, H, small_cells=s, item_rows=r), 3)[0]] for s, r in SWEEP]
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
            del rasterizer
            torch.cuda.empty_cache()
        if scene == "c2" and not args.no_route:
            from face_outlines_rate import crown_classes

            import nadir_standin as ns

            clean, _noisy = crown_classes(points, faces, 400.0)
            labels = np.where(clean < 0, np.nan, clean).astype(np.float64)
            route = {"scene": "c2", "classes": "clean crowns, 3 classes", "grids": []}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mesh.face_label_outlines(labels, points_in_export_CRS=points)
            torch.cuda.synchronize()
            route["face_label_outlines_s"] = round(time.perf_counter() - t0, 3)
            t0 = time.perf_counter()
            polygons, columns = mesh.export_face_labels_vector(labels, points_in_export_CRS=points)
            torch.cuda.synchronize()
            route["export_face_labels_vector_s"] = round(time.perf_counter() - t0, 3)     # the trace again, and the nesting on the host
            values = [int(v) for v in next(iter(columns.values())).tolist()]
            for cell in [c for c in args.cells if c >= 0.2]:
                like = grid_from_bounds(points, cell)
                grid = {"cell_m": cell}
                burn_polygons(polygons, values, like, backend=hip)      # warm-up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                burned = burn_polygons(polygons, values, like, backend=hip)
                grid["burn_polygons_s"] = round(time.perf_counter() - t0, 3)
                mesh.export_face_labels_raster(labels, like=like, points_in_raster_CRS=points)     # warm-up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                raster = mesh.export_face_labels_raster(labels, like=like, points_in_raster_CRS=points)
                grid["export_face_labels_raster_s"] = round(time.perf_counter() - t0, 3)
                grid["vector_route_s"] = round(route["export_face_labels_vector_s"] + grid["burn_polygons_s"], 3)
                # one sheet, so the two routes paint the same map but for the 1e-6 m snap of the outlines against the 1 / 65536 cell
                # snap of the raster: cells whose centre lies within a grid step of a class border may differ
                grid["cells_that_differ"] = int((burned != raster.data[0]).sum())
                grid["cells"] = int(burned.size)
                route["grids"].append(grid)
            res["class_raster_route"] = route
            print(json.dumps(route), flush=True)
            # the stand-in on a 256 x 256 window of the 1 m grid
            (H, W), transform = grid_from_bounds(points, 1.0)
            vq = points_to_cell_units(points[:, :2], invert_affine(transform))
            window = (72, 72, 256, 256)
            t0 = time.perf_counter()
            want = ns.nadir_raster(vq, points[:, 2], faces, window)
            host = {"window": window, "cell_m": 1.0, "standin_s": round(time.perf_counter() - t0, 3)}
            rasterizer = hip.nadir_rasterizer(vq, np.ascontiguousarray(points[:, 2]), faces)
            got = [t.cpu().numpy() for t in rasterizer.window(*window)]
            assert np.array_equal(got[0], want[0]), "the device's face plane differs from the stand-in's"
            assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), "the device's height plane differs from the stand-in's"
            assert np.array_equal(got[2], want[2]), "the device's statistics differ from the stand-in's"
            host["device_ms_median"], host["device_ms_best"] = timed(lambda: rasterizer.window(*window), args.repeats)
            host["device_equals_standin_bit_for_bit"] = True
            res["host_standin"] = host
            print(json.dumps(host), flush=True)
    res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
