#!/usr/bin/env python3
"""tools/face_outlines_rate.py -- rate of the class-outline trace (gr_class_outlines) on the C2 mesh
(utils/synthetic.terrain_mesh: 1 201 250 faces over 400 m) and the C5 mesh (terrain_mesh(1582, 800): 4 999 122 faces over 800 m).
Classes: crown-like disks of 2 to 6 m radius over about a third of the footprint, three species, the rest without a class ("clean"),
and the same with 10 % of the faces given a class at random ("noisy": what a per-face argmax looks like).

  device      HIP events around the binding's call (HipRaster.class_outlines: the call, its two synchronisations and, when the first
              capacity was too small, its repeat) with every input already on the device, median and best of --repeats after a warm-up
  end to end  TexturedPhotogrammetryMesh.export_face_labels_vector to a .geojson with a host clock (snap, upload, trace, read-back,
              exact areas, nesting, file)
  host        a vectorised numpy restatement of rules X1-X6 on this host's CPUs (np.lexsort, np.add.reduceat, pointer doubling with
              fancy indexing), exact in int64 at these extents

The tool ASSERTS that every array of the device equals the numpy restatement's.  Writes profiles/face_outlines_rate.json (and prints it
as one JSON line).  No pass / fail bar on the rates: nobody has measured this stage before, and shapely runs neither here nor where
this project is built.

    python tools/face_outlines_rate.py [--repeats 5] [--meshes c2 c5]
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


def crown_classes(points, faces, extent, seed=0):
    """(clean, noisy) int32 classes per face: disks of 2-6 m radius, species = disk number mod 3; noisy: 10 % of the faces at random
    get one of the three classes or none."""
    rng = np.random.default_rng(seed)
    centres = points[faces].mean(axis=1)[:, :2]
    n_crowns = int(extent * extent / 3 / (np.pi * 16))
    cxy = rng.uniform(points[:, :2].min(axis=0), points[:, :2].max(axis=0), (n_crowns, 2))
    radius = rng.uniform(2.0, 6.0, n_crowns)
    clean = np.full(len(faces), -1, dtype=np.int32)
    cell = 12.0
    keys = np.floor(centres / cell).astype(np.int64)
    order = np.lexsort((keys[:, 1], keys[:, 0]))
    sorted_keys = keys[order]
    for k in range(n_crowns):   # faces within the 3 x 3 cells around the crown
        lo, hi = np.floor((cxy[k] - radius[k]) / cell).astype(np.int64), np.floor((cxy[k] + radius[k]) / cell).astype(np.int64)
        for gx in range(lo[0], hi[0] + 1):
            a = np.searchsorted(sorted_keys[:, 0], gx, "left")
            b = np.searchsorted(sorted_keys[:, 0], gx, "right")
            a2 = a + np.searchsorted(sorted_keys[a:b, 1], lo[1], "left")
            b2 = a + np.searchsorted(sorted_keys[a:b, 1], hi[1], "right")
            sel = order[a2:b2]
            clean[sel[np.hypot(*(centres[sel] - cxy[k]).T) < radius[k]]] = k % 3
    noisy = clean.copy()
    flip = rng.random(len(faces)) < 0.10
    noisy[flip] = rng.integers(-1, 3, int(flip.sum()))
    return clean, noisy


def numpy_outlines(vq, faces, cls, C):
    """X2-X6 in vectorised int64 numpy: (canon, ring_vertices, ring_offsets, ring_class, stats (8,))."""
    V = len(vq)
    assert np.abs(vq).max() < 2 ** 30, "the int64 restatement needs coordinates below 2^30"
    stats = np.zeros(8, dtype=np.int64)
    order = np.lexsort((np.arange(V), vq[:, 1], vq[:, 0]))
    sv = vq[order]
    head = np.r_[True, (sv[1:] != sv[:-1]).any(axis=1)]
    canon = np.empty(V, dtype=np.int32)
    canon[order] = order[np.maximum.accumulate(np.where(head, np.arange(V), 0))]
    ok = ((faces >= 0) & (faces < V)).all(axis=1)
    stats[5] = int((~ok).sum())
    take = ok & (cls >= 0) & (cls < C)
    stats[0] = int((ok & ~take).sum())
    tri, c = canon[faces[take]].astype(np.int64), cls[take].astype(np.int64)
    p = vq[tri]
    area = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])
    stats[1], stats[2] = int((area == 0).sum()), int((area < 0).sum())
    tri[area < 0] = tri[area < 0][:, [0, 2, 1]]
    tri, c = tri[area != 0], c[area != 0]
    frm, to, cc = tri.reshape(-1), tri[:, [1, 2, 0]].reshape(-1), np.repeat(c, 3)
    # X4: the signed count of every (class, unordered pair)
    lo, hi, sign = np.minimum(frm, to), np.maximum(frm, to), np.where(frm < to, 1, -1)
    pair = lo << 31 | hi
    order = np.lexsort((pair, cc))
    pair, cc, sign = pair[order], cc[order], sign[order]
    head = np.r_[True, (pair[1:] != pair[:-1]) | (cc[1:] != cc[:-1])] if len(pair) else np.zeros(0, dtype=bool)
    starts = np.nonzero(head)[0]
    if len(starts):
        n = np.add.reduceat(sign, starts)
        count = np.add.reduceat(np.ones_like(sign), starts)
        stats[3] = int(((count - np.abs(n)) // 2).sum())
        stats[4] = int((np.abs(n) > 1).sum())
        keep = n != 0
        gp, gc, gn = pair[starts][keep], cc[starts][keep], n[keep]
        a, b = gp >> 31, gp & 0x7FFFFFFF
        e_from = np.repeat(np.where(gn > 0, a, b), np.abs(gn))
        e_to = np.repeat(np.where(gn > 0, b, a), np.abs(gn))
        e_cls = np.repeat(gc, np.abs(gn))
        order = np.lexsort((e_to, e_from, e_cls))
        e_from, e_to, e_cls = e_from[order], e_to[order], e_cls[order]
    else:
        e_from = e_to = e_cls = np.zeros(0, dtype=np.int64)
    E = len(e_from)
    if E == 0:
        return canon, np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32), stats
    # X5: the slots by (class, to), stably, line up with the slots by (class, from)
    succ = np.empty(E, dtype=np.int64)
    succ[np.lexsort((np.arange(E), e_to, e_cls))] = np.arange(E)
    # X6: pointer doubling
    nxt, mn, off, step = succ.copy(), np.arange(E), np.zeros(E, dtype=np.int64), 1
    while step < E:
        far = mn[nxt] < mn
        off = np.where(far, step + off[nxt], off)
        mn = np.where(far, mn[nxt], mn)
        nxt = nxt[nxt]
        step *= 2
    leaders = np.nonzero(mn == np.arange(E))[0]
    length = off[succ[leaders]] + 1
    ring_offsets = np.r_[0, np.cumsum(length)]
    ring_of = np.empty(E, dtype=np.int64)
    ring_of[leaders] = np.arange(len(leaders))
    rank = np.where(mn == np.arange(E), 0, length[ring_of[mn]] - off)
    ring_vertices = np.empty(E, dtype=np.int32)
    ring_vertices[ring_offsets[ring_of[mn]] + rank] = e_from
    return canon, ring_vertices, ring_offsets.astype(np.int64), e_cls[leaders].astype(np.int32), stats


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
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "face_outlines_rate.json")
    args = ap.parse_args()
    import tempfile

    import torch

    from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh
    from geograypher_amd.utils import synthetic
    from geograypher_amd.utils.geometric import snap_points

    if not torch.cuda.is_available():
        raise SystemExit("face_outlines_rate: no GPU; a rate is measured on the device or not at all")
    res = {"classes": 3, "repeats": args.repeats, "runs": []}
    for name in args.meshes:
        n_side, extent = MESHES[name]
        points, faces = synthetic.terrain_mesh(n_side, extent)
        mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR")
        hip = mesh.backend
        vq = snap_points(points)
        vq_d, faces_d = hip._dev(vq, torch.int64), hip._dev(faces, torch.int32)
        for kind, classes in zip(("clean", "noisy"), crown_classes(points, faces, extent)):
            cls_d = hip._dev(classes, torch.int32)
            got = hip.class_outlines(vq_d, faces_d, cls_d, 3)
            E, R = int(got[1].shape[0]), int(got[3].shape[0])
            run = {"mesh": name, "classes": kind, "vertices": int(len(points)), "faces": int(len(faces)), "ring_vertices": E, "rings": R,
                   "stats": got[4].cpu().numpy().tolist(), "calls_at_default_capacity": hip.last_outline_calls}
            med, best = timed(lambda: hip.class_outlines(vq_d, faces_d, cls_d, 3, capacity=E), args.repeats)
            run["device_ms_median"], run["device_ms_best"] = med, best
            run["device_mfaces_per_s"] = round(len(faces) / (med * 1e-3) / 1e6, 1)
            with tempfile.TemporaryDirectory() as tmp:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mesh.export_face_labels_vector(np.where(classes < 0, np.nan, classes), Path(tmp, "map.geojson"), points_in_export_CRS=points)
                run["end_to_end_s"] = round(time.perf_counter() - t0, 3)
            t0 = time.perf_counter()
            want = numpy_outlines(vq, faces, classes, 3)
            run["host_numpy_s"] = round(time.perf_counter() - t0, 3)
            for g, w, what in zip(got, want, ("canon", "ring_vertices", "ring_offsets", "ring_class", "stats")):
                assert np.array_equal(g.cpu().numpy(), w), f"the device's {what} differs from the numpy restatement"
            run["device_equals_numpy_on_every_array"] = True
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
    res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    res["device"] = torch.cuda.get_device_name(0)
    res["reference_note"] = "the reference's batched unary_union publishes no rate and cannot run without shapely and geopandas"
    line = json.dumps(res)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
