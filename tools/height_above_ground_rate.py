#!/usr/bin/env python3
"""tools/height_above_ground_rate.py -- rate of the raster-sample call (gr_sample_raster, DESIGN.md "Raster samples") on the C2
mesh (utils/synthetic.terrain_mesh: 1 201 250 faces over 400 m) and the C5 mesh (terrain_mesh(1582, 800): 4 999 122 faces over
800 m), each against a float32 DTM of its extent with cells of 1 m and of 0.25 m.

  device      HIP events around the enqueued call (check=False: no read-back) with every input already on the device, median and
              best of --repeats after a warm-up: height only (what get_height_above_ground asks for), and values + height +
              relabel together.  Beside the time, the bytes the call cannot avoid -- the faces, every vertex once, one sample per
              face, the outputs -- and the rate they amount to
  end to end  TexturedPhotogrammetryMesh.get_height_above_ground and .label_ground_class with a host clock (upload of vertices,
              faces and raster, kernel, read-back)
  host        the numpy restatement (tests/raster_standin.py) on all faces, and the per-point Python loop -- the shape of the
              reference's rasterio.sample over a list of points -- on the first --loop-faces faces, on this host's CPUs; both are
              compared with the device

Writes profiles/height_above_ground_rate.json (and prints it as one JSON line).  No pass / fail bar: the reference publishes no
figure for this stage, and rasterio runs neither here nor where this project is built.

    python tools/height_above_ground_rate.py [--repeats 5] [--loop-faces 2000] [--meshes c2 c5] [--cells 1.0 0.25]
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


def terrain_raster(points, cell, seed=0):
    """A float32 DTM over the footprint of `points`: a smooth surface a few metres under the mesh, 1 % nodata."""
    from geograypher_amd.utils.raster import PlanarRaster

    lo, hi = points[:, :2].min(axis=0), points[:, :2].max(axis=0)
    nx, ny = int(np.ceil((hi[0] - lo[0]) / cell)) + 1, int(np.ceil((hi[1] - lo[1]) / cell)) + 1
    x = lo[0] + (np.arange(nx) + 0.5) * cell
    y = hi[1] - (np.arange(ny) + 0.5) * cell
    data = (points[:, 2].min() - 3.0 + 2.0 * np.sin(x[None, :] / 37.0) * np.cos(y[:, None] / 23.0)).astype(np.float32)
    data[np.random.default_rng(seed).uniform(size=data.shape) < 0.01] = -9999.0
    return PlanarRaster(data, (cell, 0.0, float(lo[0]), 0.0, -cell, float(lo[1]) + ny * cell), nodata=-9999.0)


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
    return round(float(np.median(ms)), 4), round(min(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-faces", type=int, default=2000)
    ap.add_argument("--meshes", nargs="+", choices=sorted(MESHES), default=sorted(MESHES))
    ap.add_argument("--cells", nargs="+", type=float, default=[1.0, 0.25])
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "height_above_ground_rate.json")
    args = ap.parse_args()
    import torch

    import raster_standin as standin
    from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh
    from geograypher_amd.utils import synthetic

    if not torch.cuda.is_available():
        raise SystemExit("height_above_ground_rate: no GPU; a rate is measured on the device or not at all")
    res = {"raster_dtype": "float32", "repeats": args.repeats, "runs": []}
    for name in args.meshes:
        n_side, extent = MESHES[name]
        points, faces = synthetic.terrain_mesh(n_side, extent)
        points = np.ascontiguousarray(points, dtype=np.float64)
        faces = np.ascontiguousarray(faces, dtype=np.int32)
        F, V = len(faces), len(points)
        mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR")
        hip = mesh.backend
        p_dev, f_dev = hip._dev(points, torch.float64), hip._dev(faces, torch.int32)
        labels = (np.arange(F) % 5).astype(np.float64)
        labels[::11] = np.nan
        for cell in args.cells:
            raster = terrain_raster(points, cell)
            r_dev = hip._dev(raster.data, torch.float32)
            run = {"mesh": name, "faces": F, "vertices": V, "cell_m": cell, "raster": list(raster.shape[1:])}
            common = (p_dev, f_dev, r_dev, raster.inverse, raster.nodata, float("nan"))
            _, height, _, stats = hip.sample_raster(*common, want_values=False, want_height=True)
            height, st = height.cpu().numpy(), stats.cpu().numpy()
            run.update(inside=int(st[0]), nodata=int(st[1]))
            lab_dev = hip._dev(labels, torch.float64)
            variants = {
                "height": (lambda: hip.sample_raster(*common, want_values=False, want_height=True, check=False), 8),
                "values_height_relabel": (lambda: hip.sample_raster(*common, want_values=True, want_height=True, labels=lab_dev,
                                                                    threshold=3.0, ground_id=5.0, only_existing=True, check=False),
                                          8 + 8 + 16),
            }
            for tag, (fn, out_bytes) in variants.items():
                med, best = timed(fn, args.repeats)
                floor_bytes = F * 12 + V * 24 + F * 4 + F * out_bytes   # faces, every vertex once, a sample per face, the outputs
                run[tag] = {"device_ms_median": med, "device_ms_best": best, "device_mfaces_per_s": round(F / (med * 1e-3) / 1e6, 1),
                            "unavoidable_bytes": floor_bytes, "achieved_gb_per_s": round(floor_bytes / (med * 1e-3) / 1e9, 1)}
            e2e = {}
            for tag, fn in (("get_height_above_ground", lambda: mesh.get_height_above_ground(raster, points_in_raster_CRS=points)),
                            ("label_ground_class", lambda: mesh.label_ground_class(raster, 3.0, labels=labels.copy(), ground_ID=5,
                                                                                   points_in_raster_CRS=points))):
                times = []
                for _ in range(max(2, args.repeats // 2)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = fn()
                    times.append(time.perf_counter() - t0)
                e2e[tag] = (round(min(times), 4), out)
            run["end_to_end_s_best"] = {k: v[0] for k, v in e2e.items()}
            t0 = time.perf_counter()
            want = standin.sample_raster_np(points, faces, raster.data, raster.inverse, raster.nodata, np.nan, labels=labels,
                                            threshold=3.0, ground_id=5.0, only_existing=True)
            dt = time.perf_counter() - t0
            run["numpy"] = {"faces": F, "s": round(dt, 3), "mfaces_per_s": round(F / dt / 1e6, 2),
                            "height_equals_device": bool(np.array_equal(want["height"], height, equal_nan=True)),
                            "end_to_end_equals": bool(np.array_equal(want["height"], e2e["get_height_above_ground"][1], equal_nan=True)
                                                      and np.array_equal(want["labels"], e2e["label_ground_class"][1], equal_nan=True))}
            k = min(args.loop_faces, F)
            t0 = time.perf_counter()
            loop = standin.sample_by_loop(want["queries"][:k, :2], raster.data, raster.transform, raster.nodata, np.nan)
            dt = time.perf_counter() - t0
            run["python_loop"] = {"faces": k, "s": round(dt, 4), "faces_per_s": round(k / dt, 1),
                                  "equals_device": bool(np.array_equal(want["queries"][:k, 2] - loop[:, 0], height[:k], equal_nan=True))}
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
            del r_dev, lab_dev
    res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    res["device"] = torch.cuda.get_device_name(0)
    res["reference_note"] = ("the reference samples with rasterio.sample over a Python list of points, one at a time; it publishes "
                             "no rate and cannot run without rasterio: the per-point Python loop stands in for it")
    line = json.dumps(res)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
