#!/usr/bin/env python3
"""tools/mesh_decimation_rate.py -- rate of the mesh decimation by vertex clustering (gr_cluster_count + gr_cluster_decimate, DESIGN.md
section 8n) on the C2 mesh (utils/synthetic.terrain_mesh: 1 201 250 faces over 400 m) and the C5 mesh (terrain_mesh(1582, 800):
4 999 122 faces over 800 m) at the targets 0.5, 0.25 and 0.05 -- and what the decimated C2 mesh does to the raster rate at
render_img_scale = 0.25, the operating point at which a C2 face is about 3 pixels wide.

  device      HIP events around the binding's calls with the snapped vertices and the faces already on the device, median and best of
              --repeats after a warm-up: one probe (`cluster_count`, its 8-byte read-back included), the whole search
              (`cluster_cell_size`: its probes and read-backs), and `cluster_decimate` (its one read-back included)
  end to end  TexturedPhotogrammetryMesh.decimate with a host clock (snap, upload, search, decimation, read-back, gather)
  host        a vectorised numpy restatement of rules D2-D8 on this host's CPUs (np.lexsort where the device sorts by radix): the
              same search, then the decimation
  raster      on C2 at target 0.25: the ids-only rate (`raster_face_ids`, the 50-view survey of the benchmark's quarter-scale leg) and
              the fused aggregation rate (`raster_project_labels`, 4 classes, labels made from the ids on the device) of the FULL mesh
              and of the DECIMATED mesh, alternating, two rounds in this run; views per second over windows of --raster-reps calls
              (about 0.1 s of the full mesh each; the median of three windows) after two sizing calls

The tool ASSERTS that the device's search and decimation equal the numpy restatement on every vertex and face.  Writes
profiles/mesh_decimation_rate.json (and prints it as one JSON line).  No pass / fail bar on the rates: nobody has measured this stage
before, and VTK's quadric decimation runs neither here nor where this project is built.

    python tools/mesh_decimation_rate.py [--repeats 5] [--meshes c2 c5] [--targets 0.5 0.25 0.05] [--raster-reps 400]
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

MESHES = {"c2": (776, 400.0), "c5": (1582, 800.0)}


class NumpyBackend:
    """Rules D2-D8 in vectorised int64 numpy (exact: d2 < 2^62), behind the two calls of the binding."""

    @staticmethod
    def _keys(q, s):
        c = q // s
        t = 2 * (q - c * s) - s
        return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2], (t * t).sum(axis=1)

    def cluster_count(self, q, s):
        return len(np.unique(self._keys(q, s)[0]))

    def cluster_decimate(self, q, faces, s, check=True):
        V = len(q)
        key, d2 = self._keys(q, s)
        order = np.lexsort((np.arange(V), d2, key))
        head = np.ones(V, dtype=bool)
        head[1:] = key[order][1:] != key[order][:-1]
        rep = np.empty(V, dtype=np.int64)
        rep[order] = order[head][np.cumsum(head) - 1]
        rf = rep[faces]
        survives = (rf[:, 0] != rf[:, 1]) & (rf[:, 1] != rf[:, 2]) & (rf[:, 0] != rf[:, 2])
        idx = np.nonzero(survives)[0]
        triple = np.sort(rf[idx], axis=1)
        by_triple = np.lexsort((idx, triple[:, 2], triple[:, 1], triple[:, 0]))
        first = np.ones(len(idx), dtype=bool)
        first[1:] = (triple[by_triple][1:] != triple[by_triple][:-1]).any(axis=1)
        face_ids = np.sort(idx[by_triple[first]])
        used = np.zeros(V, dtype=bool)
        used[rf[face_ids].reshape(-1)] = True
        point_ids = np.nonzero(used)[0]
        place = np.cumsum(used) - 1
        stats = np.array([len(face_ids), len(point_ids), 0, int(head.sum()), int((~survives).sum()), len(idx) - len(face_ids), 0, 0])
        return rep.astype(np.int32), face_ids, point_ids, place[rf[face_ids]].astype(np.int32), stats


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


def raster_rates(points, faces, reps):
    """Views per second of the ids-only and of the fused call at render_img_scale = 0.25 on one mesh, in a context of its own."""
    import torch

    from bench import device_labels
    from geograypher_amd._hip import HipRaster
    from geograypher_amd.utils import synthetic

    cams = synthetic.survey_cameras(10, 5, 40.0, 60.0, seed=3, f=3000.0, width=4000, height=3000)
    h, w = cams[0].get_image_size(0.25)
    hip = HipRaster(0)
    recs = torch.from_numpy(cams.get_raster_records(0.25, near=1.0)).to(hip.device)
    n, C = int(recs.shape[0]), 4
    hip.upload_mesh(points.astype(np.float32), faces.astype(np.int32))
    ids = torch.empty((n, h, w), dtype=torch.int32, device=hip.device)
    hip.raster_face_ids(recs, h, w, out=ids, check=True)    # sizes the segments; counts the micro faces
    hip.raster_face_ids(recs, h, w, out=ids, check=True)    # micro lists, where learned, from here on

    def window(step):
        step()
        torch.cuda.synchronize()
        rates = []
        for _ in range(3):   # the median of three windows
            t0 = time.perf_counter()
            for _ in range(reps):
                step()
            torch.cuda.synchronize()
            rates.append(reps * n / (time.perf_counter() - t0))
        return round(sorted(rates)[1], 1)

    out = {"views": n, "image": [h, w], "faces": int(len(faces)),
           "ids_only_views_per_s": window(lambda: hip.raster_face_ids(recs, h, w, out=ids, check=False))}
    out["covered_pixel_share"] = round(float((ids >= 0).float().mean().item()), 4)
    labels = torch.stack([device_labels(ids[v], v, C) for v in range(n)])
    votes, counts = hip.new_vote_buffers(C)
    hip.raster_project_labels(recs, labels, C, votes, counts, check=True)
    hip.raster_project_labels(recs, labels, C, votes, counts, check=True)
    out["fused_views_per_s"] = window(lambda: hip.raster_project_labels(recs, labels, C, votes, counts, check=False))
    del hip, ids, labels, votes, counts
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--meshes", nargs="+", choices=sorted(MESHES), default=sorted(MESHES))
    ap.add_argument("--targets", nargs="+", type=float, default=[0.5, 0.25, 0.05])
    ap.add_argument("--raster-reps", type=int, default=400)
    ap.add_argument("--raster-target", type=float, default=0.25)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "mesh_decimation_rate.json")
    args = ap.parse_args()
    import torch

    from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh
    from geograypher_amd.utils import synthetic
    from geograypher_amd.utils.geometric import cluster_cell_range, cluster_cell_size, snap_points_3d

    if not torch.cuda.is_available():
        raise SystemExit("mesh_decimation_rate: no GPU; a rate is measured on the device or not at all")
    res = {"repeats": args.repeats, "runs": []}
    host = NumpyBackend()
    for name in args.meshes:
        n_side, extent = MESHES[name]
        points, faces = synthetic.terrain_mesh(n_side, extent)
        mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR")
        hip = mesh.backend
        verts_q = snap_points_3d(points)
        vq_dev, faces_dev = hip.to_device(verts_q, "int64"), hip.to_device(faces, "int32")
        s_min, s_max = cluster_cell_range(verts_q)
        for target in args.targets:
            s, cells, probes = cluster_cell_size(hip, verts_q, target, held=vq_dev)
            run = {"mesh": name, "vertices": int(len(points)), "faces": int(len(faces)), "target": target, "s_min": s_min, "s_max": s_max,
                   "cell_size_steps": s, "cell_size_m": round(s * 1e-6, 6), "cells": cells, "probes": probes}
            med, best = timed(lambda: hip.cluster_count(vq_dev, s), args.repeats)
            run["one_probe"] = {"device_ms_median": med, "device_ms_best": best, "device_mvertices_per_s": round(len(points) / (med * 1e-3) / 1e6, 1)}
            med, best = timed(lambda: cluster_cell_size(hip, verts_q, target, held=vq_dev), args.repeats)
            run["search"] = {"device_ms_median": med, "device_ms_best": best}
            rep, face_ids, point_ids, new_faces, stats = hip.cluster_decimate(vq_dev, faces_dev, s)
            med, best = timed(lambda: hip.cluster_decimate(vq_dev, faces_dev, s), args.repeats)
            run["cluster_decimate"] = {"device_ms_median": med, "device_ms_best": best, "faces_kept": int(len(face_ids)),
                                       "points_kept": int(len(point_ids)), "faces_collapsed": int(stats[4]), "faces_duplicate": int(stats[5]),
                                       "device_mfaces_per_s": round(len(faces) / (med * 1e-3) / 1e6, 1)}
            run["search_share_of_search_plus_decimate"] = round(run["search"]["device_ms_median"] /
                                                                (run["search"]["device_ms_median"] + med), 3)
            e2e = []
            for _ in range(max(2, args.repeats // 2)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                (dec_points, dec_faces), pid, fid = mesh.decimate(target, return_original_IDs=True)
                e2e.append(time.perf_counter() - t0)
            run["end_to_end_s_best"] = round(min(e2e), 3)
            run["achieved_vertex_fraction"] = round(mesh.last_decimation_stats["achieved_vertex_fraction"], 4)
            run["achieved_face_fraction"] = round(mesh.last_decimation_stats["achieved_face_fraction"], 4)
            t0 = time.perf_counter()
            want_search = cluster_cell_size(host, verts_q, target)
            t1 = time.perf_counter()
            want = host.cluster_decimate(verts_q, faces, s)
            t2 = time.perf_counter()
            run["host_numpy"] = {"search_s": round(t1 - t0, 3), "decimate_s": round(t2 - t1, 3)}
            assert want_search == (s, cells, probes), "the device's search differs from the numpy restatement"
            for got, expected, what in zip((rep, face_ids, point_ids, new_faces, stats), want, ("rep", "face_ids", "point_ids", "new_faces", "stats")):
                assert np.array_equal(got.cpu().numpy(), expected), f"the device's {what} differs from the numpy restatement"
            assert np.array_equal(fid, want[1]) and np.array_equal(pid, want[2]) and np.array_equal(dec_faces, want[3])
            run["device_equals_numpy_on_every_vertex_and_face"] = True
            if name == "c2" and target == args.raster_target:
                del rep, face_ids, point_ids, new_faces
                rounds = []
                for _ in range(2):   # full, decimated, full, decimated: the second round shows the spread of the first
                    full = raster_rates(points, faces, args.raster_reps)
                    decimated = raster_rates(dec_points, dec_faces, args.raster_reps)
                    rounds.append({"full": full, "decimated": decimated,
                                   "ids_only_speedup": round(decimated["ids_only_views_per_s"] / full["ids_only_views_per_s"], 3),
                                   "fused_speedup": round(decimated["fused_views_per_s"] / full["fused_views_per_s"], 3)})
                run["raster_at_scale_0.25"] = {"calls_per_window": args.raster_reps, "rounds": rounds}
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
        del vq_dev, faces_dev, mesh, hip
    res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    res["device"] = torch.cuda.get_device_name(0)
    res["reference_note"] = "the reference's VTK quadric decimation publishes no rate and cannot run where this project is built"
    line = json.dumps(res)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
