#!/usr/bin/env python3
"""tools/reproject_rate.py -- rate of the CRS reprojection call (gr_reproject_points, DESIGN.md "CRS reprojection") on the vertices
of the C2 mesh (utils/synthetic.terrain_mesh: 602 176 vertices over 400 m) and of the C5 mesh (terrain_mesh(1582, 800): 2 502 724
vertices over 800 m), placed in UTM zone 10 and brought to EPSG:4978 first: the direction that is timed is ECEF -> UTM, what every
`points_in_*_CRS` designator asks for.

  device   HIP events around the enqueued call (check=False: no read-back) with the vertices already on the device, median and
           best of --repeats after a warm-up; per vertex and per face centre (three conversions a face).  Beside the time, the 48
           bytes a vertex cannot avoid (24 in, 24 out) and the rate they amount to: the call is bound by about 15 float64 library
           functions per point, not by those bytes
  host     the numpy restatement (tests/crs_standin.py) on the same vertices, on this host's CPUs, and the largest difference
           between the two in metres
  golden   the device's largest error against the mpmath oracle of tests/golden/crs_wgs84.npz over all six directions, in the
           three classes of G9 (planar and ECEF components, heights, lon / lat as radians x a)

Writes profiles/reproject_rate.json (and prints it as one JSON line).  No pass / fail bar: the reference publishes no figure for
pyproj's transform of a mesh, and pyproj runs neither here nor where this project is built.

    python tools/reproject_rate.py [--repeats 5] [--meshes c2 c5]
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
UTM10 = (2, -123.0, 0.9996, 500000.0, 0.0)
ECEF = (0, 0.0, 1.0, 0.0, 0.0)


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


def golden_errors(hip):
    import crs_standin as cs
    from geograypher_amd.utils.geospatial import WGS84CRS

    g = cs.load_golden()
    worst = np.zeros(3)
    for src, dst in cs.PAIRS:
        for group in range(len(g["tm_params"])):
            rows = np.nonzero(g["group"] == group)[0]
            out, _ = hip.reproject_points(g[f"in_{src}"][rows], WGS84CRS(*cs.golden_crs(g, src, group)),
                                          WGS84CRS(*cs.golden_crs(g, dst, group)))
            worst = np.maximum(worst, cs.worst_errors(out.cpu().numpy(), g[f"exp_{src}_{dst}"][rows], dst, from_ecef=src == "ecef"))
    return {"device_max_error_m": {"planar_and_ecef": float(worst[0]), "height": float(worst[1]), "lon_lat_times_a": float(worst[2])},
            "standin_max_error_m": [float(v) for v in g["standin_err_m"]], "points": int(len(g["group"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--meshes", nargs="+", choices=sorted(MESHES), default=sorted(MESHES))
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "reproject_rate.json")
    args = ap.parse_args()
    import torch

    import crs_standin as cs
    from geograypher_amd._hip import HipRaster
    from geograypher_amd.utils import synthetic
    from geograypher_amd.utils.geospatial import WGS84CRS

    if not torch.cuda.is_available():
        raise SystemExit("reproject_rate: no GPU; a rate is measured on the device or not at all")
    hip = HipRaster(0)
    src, dst = WGS84CRS(*ECEF), WGS84CRS(*UTM10)
    res = {"direction": "EPSG:4978 -> EPSG:32610", "repeats": args.repeats, "golden": golden_errors(hip), "runs": []}
    for name in args.meshes:
        n_side, extent = MESHES[name]
        points, faces = synthetic.terrain_mesh(n_side, extent)
        utm = np.ascontiguousarray(points, dtype=np.float64) + (552000.0, 4182000.0, 0.0)
        faces = np.ascontiguousarray(faces, dtype=np.int32)
        V, F = len(utm), len(faces)
        ecef = hip.reproject_points(utm, dst, src)[0]
        f_dev = hip._dev(faces, torch.int32)
        out_v = torch.empty((V, 3), dtype=torch.float64, device=hip.device)
        out_f = torch.empty((F, 3), dtype=torch.float64, device=hip.device)
        run = {"mesh": name, "vertices": V, "faces": F}
        med, best = timed(lambda: hip.reproject_points(ecef, src, dst, out=out_v, check=False), args.repeats)
        run["vertices_ecef_to_utm"] = {"device_ms_median": med, "device_ms_best": best,
                                       "device_mpoints_per_s": round(V / (med * 1e-3) / 1e6, 1), "unavoidable_bytes": V * 48,
                                       "achieved_gb_per_s": round(V * 48 / (med * 1e-3) / 1e9, 1)}
        med, best = timed(lambda: hip.reproject_points(ecef, src, dst, faces=f_dev, out=out_f, check=False), args.repeats)
        run["face_centres_ecef_to_utm"] = {"device_ms_median": med, "device_ms_best": best,
                                           "device_mfaces_per_s": round(F / (med * 1e-3) / 1e6, 1)}
        ecef_h = ecef.cpu().numpy()
        t0 = time.perf_counter()
        want, status = cs.reproject(ecef_h, ECEF, UTM10)
        dt = time.perf_counter() - t0
        got = out_v.cpu().numpy()
        run["numpy"] = {"points": V, "s": round(dt, 3), "mpoints_per_s": round(V / dt / 1e6, 2),
                        "max_difference_from_device_m": float(np.abs(want - got).max()),
                        "max_round_trip_error_m": float(np.abs(got - utm).max()), "flagged": int((status != 0).sum())}
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    res["device"] = torch.cuda.get_device_name(0)
    res["reference_note"] = ("the reference transforms the vertices with pyproj.Transformer (PROJ); it publishes no rate and pyproj is "
                             "installed neither here nor where this project is built, so parity with PROJ itself is unmeasured: the "
                             "numpy restatement stands in for the host, the mpmath oracle for the truth")
    line = json.dumps(res)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
