"""tools/ray_pairs_rate.py -- rate of gr_ray_pairs (the ray-pair graph of triangulate_detections) on one MI355X.

    python tools/ray_pairs_rate.py [--sizes 10000 100000] [--reps 5] [--out profiles/ray_pairs_rate.json]

Per size N (a `synthetic.detection_survey` of about N rays at its default density; threshold 0.5 m): the count-only call and
the count-then-fill protocol (`HipRaster.ray_pair_edges`: a first call that overflows the default capacity plus the repeat, or
one call when the edges fit), each timed with HIP events around the whole call after two warm-up calls, median of --reps;
pairs / s = N (N - 1) / 2 over the count-only time.  Beside it: the numpy stand-in (tests/ray_standin.py) on one
5000 x 5000 block on this host, and the float64 VALU instructions the compiler emitted for k_ray_pairs (static count from
the gfx950 assembly: the rare parallel branch included, so an upper bound per pair).  Each size is one child process under its
own time limit; a failure ends the run."""
import argparse
import json
import re
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def static_f64_ops():
    from geograypher_amd import build as gbuild

    flags = [f for f in gbuild.HIPCC_FLAGS if f != "-shared"]
    with tempfile.TemporaryDirectory() as tmp:
        asm = Path(tmp) / "rays.s"
        cmd = [gbuild.hipcc_path(), *flags, "-S", "--cuda-device-only", f"-I{gbuild.INCLUDE}", f"-I{gbuild.CSRC}", "-o", str(asm),
               str(gbuild.CSRC / "rays.hip")]
        subprocess.run(cmd, check=True, capture_output=True)
        text = asm.read_text()
    out = {}
    for name, body in re.findall(r"^(_Z\S*k_ray_pairs\S*):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M):
        ops = re.findall(r"^\s+(v_\w+_f64)(?:_e32|_e64)?\b", body, re.M)
        kinds = {}
        for op in ops:
            kinds[op] = kinds.get(op, 0) + 1
        out["fill" if "Lb1" in name else "count"] = {"f64_valu_instructions": len(ops), "by_opcode": kinds}
    return out


def one_size(n_rays: int, reps: int):
    import torch

    from geograypher_amd._hip import HipRaster
    from geograypher_amd.utils import synthetic

    survey = synthetic.detection_survey(n_objects=max(n_rays // 20, 1), n_cameras=40, seed=1)
    hip = HipRaster(0)
    s_t, e_t, id_t = hip._ray_inputs(survey["ray_starts"], survey["ray_ends"], survey["ray_IDs"])
    n = int(s_t.shape[0])

    def timed(fn):
        for _ in range(2):
            fn()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), [float(x) for x in ms]

    count_ms, count_all = timed(lambda: hip.ray_pair_count(s_t, e_t, id_t, 0.5))
    edges = hip.ray_pair_count(s_t, e_t, id_t, 0.5)
    fill_ms, fill_all = timed(lambda: hip.ray_pair_edges(s_t, e_t, id_t, 0.5))
    calls = hip.last_ray_pair_calls
    exact_ms, _ = timed(lambda: hip.ray_pair_edges(s_t, e_t, id_t, 0.5, capacity=edges))
    pairs = n * (n - 1) // 2
    return {"rays": n, "pairs": pairs, "edges": edges, "count_only_ms": count_ms, "count_only_ms_all": count_all,
            "count_then_fill_ms": fill_ms, "count_then_fill_ms_all": fill_all, "count_then_fill_calls": calls,
            "fill_at_exact_capacity_ms": exact_ms, "pairs_per_s_count_only": pairs / (count_ms * 1e-3),
            "pairs_per_s_count_then_fill": pairs / (fill_ms * 1e-3)}


def host_block():
    from geograypher_amd.utils import synthetic
    from tests.ray_standin import pair_distance

    s = synthetic.detection_survey(n_objects=500, n_cameras=40, seed=1)
    starts, ends = s["ray_starts"][:5000], s["ray_ends"][:5000]
    rows = 250   # twenty slices of the 5000 x 5000 block: the stand-in's temporaries for all of it at once would not fit
    t0 = time.perf_counter()
    for r0 in range(0, 5000, rows):
        i = np.repeat(np.arange(r0, r0 + rows), 5000)
        j = np.tile(np.arange(5000), rows)
        pair_distance(starts, ends, i, j)
    dt = time.perf_counter() - t0
    return {"block": [5000, 5000], "seconds": dt, "pairs_per_s": 25e6 / dt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ray_pairs_rate.json"))
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--limit", type=int, default=240, help="seconds per size")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(one_size(args.child, args.reps)))
        return
    result = {"threshold": 0.5, "scene": "synthetic.detection_survey(n_objects=N/20, n_cameras=40, seed=1)", "sizes": [],
              "isa": static_f64_ops(), "host_numpy_stand_in": host_block()}
    for n in args.sizes:
        res = subprocess.run([sys.executable, __file__, "--child", str(n), "--reps", str(args.reps)], capture_output=True,
                             text=True, timeout=args.limit)
        if res.returncode != 0:
            print(res.stdout[-2000:], res.stderr[-2000:])
            raise SystemExit(f"size {n} failed with exit status {res.returncode}: stopping")
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        result["sizes"].append(json.loads(line[7:]))
        print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
