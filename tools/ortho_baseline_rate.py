#!/usr/bin/env python3
"""tools/ortho_baseline_rate.py -- rates of the two device stages of the orthomosaic baseline at a size a
user would run: an extent of --side x --side pixels (default 8192) covered by chips of 1024 every 512 (up to four tiles over a
pixel), 5 classes, 10 % of the predictions unlabeled.

  assembly    HIP events around HipRaster.assemble_tiles with every table already on the device (the host checks of the tables
              are inside the events), median and best of --repeats after a warm-up, for uint8 counts with and without the counts
              plane stored, and for float64 counts; the classes are ASSERTED equal to the numpy stand-in of O1-O5
              (tests/ortho_standin.py) on the same inputs
  zonal       the class raster that came out, counted under a grid of jittered quadrilaterals of about 96 cells a side that tile
              it (a crown-sized polygon layer), the same way; the summed counts are ASSERTED equal to np.bincount of the raster
              (the partition property), which needs no stand-in

Writes profiles/ortho_baseline_rate.json (and prints it as one JSON line).  No pass / fail bar on the rates.

    python tools/ortho_baseline_rate.py [--repeats 5] [--side 8192] [--out profiles/ortho_baseline_rate.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def timed(torch, repeats, call):
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = call()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    return out, float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--side", type=int, default=8192)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "ortho_baseline_rate.json")
    args = ap.parse_args()
    import torch

    import ortho_standin as osn
    from geograypher_amd._hip import HipRaster
    from geograypher_amd.predictors import ortho_segmentor as og
    from geograypher_amd.utils.geometric import tile_bin_table, zonal_work_items
    from geograypher_amd.utils.geospatial import rings_to_cell_units

    side, chip, stride, C = args.side, 1024, 512, 5
    rng = np.random.default_rng(0)
    windows = [w for w in og.create_windows((side, side), chip, stride) if w.col_off + chip <= side and w.row_off + chip <= side]
    preds = [np.where(rng.random((chip, chip)) < 0.1, 255, rng.integers(0, C, (chip, chip))).astype(np.uint8) for _ in windows]
    hip = HipRaster(0)
    result = {"extent": [side, side], "tiles": len(windows), "chip": chip, "stride": stride, "classes": C, "repeats": args.repeats}
    want = {dtype: osn.assemble(preds, [tuple(w) for w in windows], side, side, C, 255, count_dtype=dtype)[0] for dtype in (np.uint8, float)}
    classes = None
    for name, dtype, want_counts in (("float64_counts", float, True), ("uint8", np.uint8, False), ("uint8_counts", np.uint8, True)):
        t = og.tile_tables(preds, windows, C, 0.25, dtype, 4)
        bins = tile_bin_table(t[2], side, side)
        dev = [hip._dev(t[0], torch.uint8), t[1], t[2], t[3], hip._dev(t[4], torch.float64 if dtype is float else torch.uint8), t[5]]
        out, median, best = timed(torch, args.repeats, lambda: hip.assemble_tiles(*dev, dtype, bins, side, side, C, 255, want_counts=want_counts))
        classes = out[0].cpu().numpy()
        assert np.array_equal(classes, want[dtype]), name
        stats = out[2].cpu().tolist()
        result[f"assemble_{name}"] = {"median_ms": round(median, 3), "best_ms": round(best, 3), "Gpix_per_s": round(side * side / median / 1e6, 2),
                                      "pairs": stats[3], "longest_list": stats[2]}
    # zonal counts under quadrilaterals that tile the raster
    step = 96
    xs = np.arange(-step, side + 2 * step, step, dtype=np.float64)
    gx, gy = np.meshgrid(xs, xs)
    jitter = rng.uniform(-0.4 * step, 0.4 * step, gx.shape + (2,))
    jitter[[0, -1]] = 0
    jitter[:, [0, -1]] = 0
    vx, vy = np.rint((gx + jitter[..., 0]) * 65536) / 65536, np.rint((gy + jitter[..., 1]) * 65536) / 65536
    n = len(xs) - 1
    rings = [np.array([(vx[j, i], vy[j, i]), (vx[j, i + 1], vy[j, i + 1]), (vx[j + 1, i + 1], vy[j + 1, i + 1]), (vx[j + 1, i], vy[j + 1, i])])
             for j in range(n) for i in range(n)]
    P = len(rings)
    rv, off = rings_to_cell_units(rings, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0))
    rp = np.arange(P, dtype=np.int32)
    items = zonal_work_items(rv, off, rp, P, side, side)
    dev = [hip._dev(classes, torch.uint8), 255, hip._dev(rv, torch.int64), off, rp, P, hip._dev(items, torch.int32), C]
    out, median, best = timed(torch, args.repeats, lambda: hip.zonal_class_counts(*dev))
    counts, stats = out[0].cpu().numpy(), out[1].cpu().tolist()
    assert np.array_equal(counts.sum(axis=0), np.bincount(classes[classes != 255], minlength=C)) and stats[1] == side * side
    result["zonal"] = {"polygons": P, "work_items": int(len(items)), "cells_tested": stats[0], "median_ms": round(median, 3), "best_ms": round(best, 3),
                       "Gcells_inside_per_s": round(side * side / median / 1e6, 2)}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
