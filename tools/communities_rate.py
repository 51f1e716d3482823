"""tools/communities_rate.py -- gr_louvain_communities and gr_community_points against the networkx path of calc_communities, on
one MI355X and its host.

    python tools/communities_rate.py [--objects 2500] [--reps 5] [--no-networkx] [--out profiles/communities_rate.json]

Input: `synthetic.detection_survey(n_objects=2500, n_cameras=40, seed=4)`, about 50 000 rays (the `big` survey of
tests/test_ray_pairs.py), its edges at 0.5 m from `HipRaster.ray_pair_edges`, weights 1 / max(d, 1e-6).  Timed with HIP events
around the whole call through the binding, after two warm-up calls, median of --reps: `louvain_communities` on device tensors (the
default path choice, and each forced path once) and `community_points`.  Beside them, once, on this host and the same edges: the
networkx path of `calc_communities`, tuple list included -- the reference's own method and the baseline -- in a child process
under --limit seconds; and the cost of one read of a control block behind an empty stream (what the host loop pays per sweep).
Recorded: the times, levels, sweeps per level, caps hit, the share of rows per path, both modularities."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def survey_edges(n_objects):
    from geograypher_amd._hip import HipRaster
    from geograypher_amd.utils import synthetic

    s = synthetic.detection_survey(n_objects=n_objects, n_cameras=40, seed=4)
    hip = HipRaster(0)
    dev = hip._ray_inputs(s["ray_starts"], s["ray_ends"], s["ray_IDs"])
    ei, ej, ed = hip.ray_pair_edges(*dev, 0.5)
    w = 1 / np.maximum(ed.cpu().numpy(), 1e-6)
    return s, hip, dev, ei, ej, w


def timed(fn, reps):
    import torch

    for _ in range(2):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [float(x) for x in ms], out


def device_side(n_objects, reps):
    import torch

    from geograypher_amd.utils import numeric

    s, hip, dev, ei, ej, w = survey_edges(n_objects)
    n, q = len(s["ray_IDs"]), numeric.quantise_weights(w)
    q_t = torch.as_tensor(q, device=ei.device)
    ms, ms_all, record = timed(lambda: hip.louvain_communities(ei, ej, q_t, n), reps)
    forced = {path: timed(lambda: hip.louvain_communities(ei, ej, q_t, n, force_path=path), 1)[0] for path in ("group", "key")}
    p_ms, p_all, _ = timed(lambda: hip.community_points(dev[0], dev[1], record["community"], record["n_communities"]), reps)
    word = torch.zeros(16, dtype=torch.int64, device=ei.device)
    torch.cuda.synchronize()
    reads = []
    for _ in range(300):
        t0 = time.perf_counter()
        word.cpu()
        reads.append((time.perf_counter() - t0) * 1e6)
    rows = record["rows_per_path"]
    return {"rays": n, "edges": int(ei.shape[0]), "louvain_ms": ms, "louvain_ms_all": ms_all, "louvain_forced_ms": forced,
            "community_points_ms": p_ms, "community_points_ms_all": p_all, "levels": record["levels"], "sweeps": record["sweeps"],
            "moves": record["moves"], "caps_hit": record["caps_hit"], "n_communities": record["n_communities"],
            "rows_per_path": rows, "rows_share": [r / max(sum(rows), 1) for r in rows],
            "modularity_device": numeric.community_modularity(record), "control_read_us_median": float(np.median(reads)),
            "control_reads_per_call": int(sum(record["sweeps"]) + 3 * len(record["sweeps"]) + 3)}


def networkx_side(n_objects):
    import networkx

    from geograypher_amd.utils import numeric

    s, _, _, ei, ej, w = survey_edges(n_objects)
    i, j = ei.cpu().numpy().astype(np.int64), ej.cpu().numpy().astype(np.int64)
    t0 = time.perf_counter()
    edges = [(a, b, {"weight": c}) for a, b, c in zip(i.tolist(), j.tolist(), w.tolist())]
    t1 = time.perf_counter()
    result = numeric.calc_communities(s["ray_starts"], s["ray_ends"], edges, seed=0)
    t2 = time.perf_counter()
    ids = result["ray_IDs"]
    parts = [set(np.nonzero(ids == c)[0].tolist()) for c in range(int(np.nanmax(ids)) + 1)]
    g = networkx.Graph()
    g.add_weighted_edges_from(zip(i.tolist(), j.tolist(), numeric.quantise_weights(w).tolist()))
    return {"tuple_list_s": t1 - t0, "calc_communities_s": t2 - t1, "total_s": t2 - t0, "n_communities": len(parts),
            "modularity_networkx": float(networkx.community.modularity(g, parts, weight="weight"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=2500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-networkx", action="store_true")
    ap.add_argument("--limit", type=int, default=420, help="seconds for the networkx baseline")
    ap.add_argument("--child", choices=["device", "networkx"])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "communities_rate.json"))
    args = ap.parse_args()
    if args.child:
        res = device_side(args.objects, args.reps) if args.child == "device" else networkx_side(args.objects)
        print("RESULT " + json.dumps(res))
        return
    result = {"scene": f"synthetic.detection_survey(n_objects={args.objects}, n_cameras=40, seed=4), threshold 0.5"}
    for side in ("device",) + (() if args.no_networkx else ("networkx",)):
        try:
            res = subprocess.run([sys.executable, __file__, "--child", side, "--objects", str(args.objects), "--reps", str(args.reps)],
                                 capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            result[side] = f"not measured: no result within {args.limit} s"
            print(side, result[side])
            continue
        if res.returncode != 0:
            print(res.stdout[-2000:], res.stderr[-2000:])
            raise SystemExit(f"the {side} side failed with exit status {res.returncode}: stopping")
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        result[side] = json.loads(line[7:])
        print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
