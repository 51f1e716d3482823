#!/usr/bin/env python3
"""tools/roi_crop_rate.py -- rate of the region-of-interest crop (gr_points_in_region + gr_submesh_extract, DESIGN.md "Region of
interest") on the C2 mesh (utils/synthetic.terrain_mesh: 1 201 250 faces over 400 m) and the C5 mesh (terrain_mesh(1582, 800):
4 999 122 faces over 800 m), each against an ROI of 1, 10 and 100 polygons of 16 to 64 vertices that together cover roughly a quarter
of the extent, with a buffer of 50 m.

  device      HIP events around each of the two enqueued calls with every input already on the device, median and best of --repeats
              after a warm-up (the sub-mesh call reads its three counts back: that is part of it)
  end to end  TexturedPhotogrammetryMesh.select_mesh_ROI with a host clock (snap, ring table, upload, kernels, read-back, gather)
  host        a vectorised numpy restatement of rules Q3-Q5 on this host's CPUs: per row the points in its grown box, per edge the
              crossing rule and the distance test in int64 (exact at these extents: coordinates below 2^29 grid steps, so dot and
              cross products stay below 2^61, and cross^2 <= D^2 L2 is |cross| <= isqrt(D^2 L2), the root taken per edge in Python
              integers); the sub-mesh with np.cumsum

The tool ASSERTS that the device mask equals the numpy mask on every vertex, and the ids and faces of the sub-mesh likewise.
Writes profiles/roi_crop_rate.json (and prints it as one JSON line).  No pass / fail bar on the rates: nobody has measured this
stage before, and geopandas runs neither here nor where this project is built.

    python tools/roi_crop_rate.py [--repeats 5] [--meshes c2 c5] [--polygons 1 10 100] [--buffer 50]
"""
import argparse
import json
import math
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

MESHES = {"c2": (776, 400.0), "c5": (1582, 800.0)}


def roi_polygons(n, extent, seed=0):
    """n star-shaped (hence simple) outlines of 16 to 64 vertices inside the central half-by-half square of the footprint -- a
    quarter of the extent: one polygon fills it, n polygons sit on a grid of ceil(sqrt(n)) cells a side and fill their cells."""
    rng = np.random.default_rng(seed)
    side = int(math.ceil(math.sqrt(n)))
    cell = extent / 2 / side
    out = []
    for i in range(n):
        cx = -extent / 4 + (i % side + 0.5) * cell
        cy = -extent / 4 + (i // side + 0.5) * cell
        k = int(rng.integers(16, 65))
        r = cell / 2 * (0.85 + 0.15 * rng.uniform(-1, 1, k))
        a = 2 * np.pi * (np.arange(k) + rng.uniform(-0.3, 0.3, k)) / k
        out.append(np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1))
    return out


def numpy_mask(vq, table, D):
    """Rules Q3 and Q4 in vectorised int64 numpy (see the module docstring for why that is exact here)."""
    rv, roff, rpoly, _, boxes = table
    assert max(int(np.abs(vq).max()), int(np.abs(rv).max())) + D < 2 ** 29, "the int64 restatement needs coordinates below 2^29"
    inside = np.zeros(len(vq), dtype=bool)
    for p in range(len(boxes)):
        b = boxes[p]
        rings = [r for r in range(len(rpoly)) if rpoly[r] == p and roff[r + 1] - roff[r] >= 3]
        if b[0] > b[2] or not rings:
            continue
        sel = np.nonzero(~inside & (vq[:, 0] >= b[0] - D) & (vq[:, 0] <= b[2] + D) & (vq[:, 1] >= b[1] - D) & (vq[:, 1] <= b[3] + D))[0]
        px, py = vq[sel, 0], vq[sel, 1]
        parity = np.zeros(len(sel), dtype=bool)
        hit = np.zeros(len(sel), dtype=bool)
        for r in rings:
            ring = rv[roff[r]:roff[r + 1]]
            for i in range(len(ring)):
                (ax, ay), (bx, by) = ring[i - 1], ring[i]
                ex, ey = int(bx - ax), int(by - ay)
                ux, uy = px - ax, py - ay
                cross = ex * uy - ey * ux
                crosses = (ay <= py) != (by <= py)
                parity ^= crosses & ((cross > 0) == (by > ay))
                hit |= (cross == 0) & (px >= min(ax, bx)) & (px <= max(ax, bx)) & (py >= min(ay, by)) & (py <= max(ay, by))
                if D > 0:
                    t = ux * ex + uy * ey
                    L2 = ex * ex + ey * ey
                    wx, wy = px - bx, py - by
                    hit |= np.where(t <= 0, ux * ux + uy * uy <= D * D,
                                    np.where(t >= L2, wx * wx + wy * wy <= D * D, np.abs(cross) <= math.isqrt(D * D * L2)))
        inside[sel[parity | hit]] = True
    return inside


def numpy_submesh(mask, faces):
    """Rule Q5 with np.cumsum."""
    keep = mask[faces].any(axis=1)
    face_ids = np.nonzero(keep)[0]
    used = np.zeros(len(mask), dtype=bool)
    used[faces[face_ids].reshape(-1)] = True
    point_ids = np.nonzero(used)[0]
    place = np.cumsum(used) - 1
    return face_ids, point_ids, place[faces[face_ids]]


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
    ap.add_argument("--meshes", nargs="+", choices=sorted(MESHES), default=sorted(MESHES))
    ap.add_argument("--polygons", nargs="+", type=int, default=[1, 10, 100])
    ap.add_argument("--buffer", type=float, default=50.0)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "roi_crop_rate.json")
    args = ap.parse_args()
    import torch

    from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh
    from geograypher_amd.utils import synthetic
    from geograypher_amd.utils.geometric import PlanarPolygons, region_buffer_steps, snap_with_polygons

    if not torch.cuda.is_available():
        raise SystemExit("roi_crop_rate: no GPU; a rate is measured on the device or not at all")
    res = {"ring_vertices": "16-64", "buffer_m": args.buffer, "repeats": args.repeats, "runs": []}
    D = region_buffer_steps(args.buffer)
    for name in args.meshes:
        n_side, extent = MESHES[name]
        points, faces = synthetic.terrain_mesh(n_side, extent)
        mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR")
        hip = mesh.backend
        faces32 = hip._dev(faces, torch.int32)
        for n_polygons in args.polygons:
            polys = PlanarPolygons.from_sequence(roi_polygons(n_polygons, extent))
            vq, table = snap_with_polygons(points, polys)
            dev = [hip._dev(vq, torch.int64)] + \
                  [hip._dev(t, dt) for t, dt in zip(table, (torch.int64, torch.int64, torch.int32, torch.int32, torch.int64))]
            mask, stats = hip.points_in_region(*dev, D)
            st = stats.cpu().numpy()
            run = {"mesh": name, "vertices": int(len(points)), "faces": int(len(faces)), "polygons": n_polygons,
                   "ring_vertices_total": int(len(table[0])), "points_inside": int(st[0]), "inside_by_buffer_only": int(st[1]),
                   "wide_comparisons": int(st[2])}
            med, best = timed(lambda: hip.points_in_region(*dev, D), args.repeats)
            run["points_in_region"] = {"device_ms_median": med, "device_ms_best": best,
                                       "device_mpoints_per_s": round(len(points) / (med * 1e-3) / 1e6, 1)}
            face_ids, point_ids, new_faces, _ = hip.submesh_extract(mask, faces32)
            med, best = timed(lambda: hip.submesh_extract(mask, faces32), args.repeats)
            run["submesh_extract"] = {"device_ms_median": med, "device_ms_best": best, "faces_kept": int(len(face_ids)),
                                      "points_kept": int(len(point_ids)),
                                      "device_mfaces_per_s": round(len(faces) / (med * 1e-3) / 1e6, 1)}
            e2e = []
            for _ in range(max(2, args.repeats // 2)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                (sub_points, sub_faces), pid, fid = mesh.select_mesh_ROI(polys, buffer_meters=args.buffer, return_original_IDs=True,
                                                                         points_in_ROI_CRS=points)
                e2e.append(time.perf_counter() - t0)
            run["end_to_end_s_best"] = round(min(e2e), 3)
            t0 = time.perf_counter()
            want = numpy_mask(vq, table, D)
            t1 = time.perf_counter()
            want_f, want_p, want_new = numpy_submesh(want, faces)
            t2 = time.perf_counter()
            run["host_numpy"] = {"points_in_region_s": round(t1 - t0, 3), "submesh_s": round(t2 - t1, 3)}
            assert np.array_equal(mask.cpu().numpy(), want), "the device mask differs from the numpy restatement"
            assert np.array_equal(face_ids.cpu().numpy(), want_f) and np.array_equal(point_ids.cpu().numpy(), want_p)
            assert np.array_equal(new_faces.cpu().numpy(), want_new)
            assert np.array_equal(fid, want_f) and np.array_equal(pid, want_p) and np.array_equal(sub_faces, want_new)
            run["device_equals_numpy_on_every_vertex_and_face"] = True
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
    res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    res["device"] = torch.cuda.get_device_name(0)
    res["reference_note"] = "the reference's gpd.overlay of every vertex publishes no rate and cannot run without geopandas"
    line = json.dumps(res)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
