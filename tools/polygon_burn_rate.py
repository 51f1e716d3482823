#!/usr/bin/env python3
"""tools/polygon_burn_rate.py -- rate of the polygon burn at a size a user would run: a grid of
--side x --side cells (default 8192) burned in one window under two polygon layers,

  tiling      the jittered quadrilaterals of about 96 cells a side of tools/ortho_baseline_rate.py's zonal leg, which tile the grid
              (7 744 at the default side): every cell lies in exactly one row, nothing contends
  crowns      3 000 seeded star-shaped polygons of 16-64 vertices and 30-90 cells radius, which overlap: the atomic maximum decides

  device      HIP events around PolygonBurner.window with the ring table and the work items already on the device (the host check
              of the items is inside the events), median and best of --repeats after a warm-up, with and without the value plane
  numpy       the same rule restated with numpy on this host (even-odd per row over the row's box of centres, int64: exact at
              this size, where every product stays below 2^63), painted in ascending row order; timed once; the row planes are
              ASSERTED equal
  write_chips the grid as an RGB GeoTIFF cut into chips of 2048 every 2048, end to end, with and without the crowns as labels

Writes profiles/polygon_burn_rate.json (and prints it as one JSON line).  No pass / fail bar on the rates.

    python tools/polygon_burn_rate.py [--repeats 5] [--side 8192] [--out profiles/polygon_burn_rate.json]
"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


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


def burn_numpy(rv, off, rp, boxes, side):
    """B2 / B3 with numpy: rows (side, side) int32.  A row's cells are those of its box whose centre an odd number of the edges of
    its rings count (half-open in y, strictly left of the upward edge); rows are painted in ascending index."""
    rows = np.full((side, side), -1, dtype=np.int32)
    first = np.searchsorted(rp, np.arange(len(boxes)), "left")
    last = np.searchsorted(rp, np.arange(len(boxes)), "right")
    for p, (c0, r0, c1, r1) in enumerate(boxes):
        c0, r0, c1, r1 = max(c0, 0), max(r0, 0), min(c1, side - 1), min(r1, side - 1)
        if c0 > c1 or r0 > r1:
            continue
        px = (65536 * np.arange(c0, c1 + 1, dtype=np.int64) + 32768)[None, :, None]
        py = (65536 * np.arange(r0, r1 + 1, dtype=np.int64) + 32768)[:, None, None]
        inside = np.zeros((r1 - r0 + 1, c1 - c0 + 1), dtype=bool)
        for r in range(first[p], last[p]):
            ring = rv[off[r]:off[r + 1]]
            if len(ring) < 3:
                continue
            a, b = ring[None, None], np.roll(ring, -1, axis=0)[None, None]
            ax, ay, bx, by = a[..., 0], a[..., 1], b[..., 0], b[..., 1]
            candidate = (ay > py) != (by > py)
            o = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
            counts = candidate & np.where(by > ay, o > 0, o < 0)
            inside ^= (counts.sum(axis=2) & 1).astype(bool)
        block = rows[r0:r1 + 1, c0:c1 + 1]
        block[inside] = p
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--side", type=int, default=8192)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "polygon_burn_rate.json")
    args = ap.parse_args()
    import torch

    from geograypher_amd._hip import HipRaster
    from geograypher_amd.predictors import ortho_segmentor as og
    from geograypher_amd.utils.geometric import burn_work_items, row_centre_boxes, row_ring_ranges
    from geograypher_amd.utils.geospatial import rings_to_cell_units
    from geograypher_amd.utils.tiff import write_tiff_deflate

    side = args.side
    rng = np.random.default_rng(0)
    step = 96
    xs = np.arange(-step, side + 2 * step, step, dtype=np.float64)
    gx, gy = np.meshgrid(xs, xs)
    jitter = rng.uniform(-0.4 * step, 0.4 * step, gx.shape + (2,))
    jitter[[0, -1]] = 0
    jitter[:, [0, -1]] = 0
    vx, vy = np.rint((gx + jitter[..., 0]) * 65536) / 65536, np.rint((gy + jitter[..., 1]) * 65536) / 65536
    n = len(xs) - 1
    tiling = [np.array([(vx[j, i], vy[j, i]), (vx[j, i + 1], vy[j, i + 1]), (vx[j + 1, i + 1], vy[j + 1, i + 1]), (vx[j + 1, i], vy[j + 1, i])])
              for j in range(n) for i in range(n)]
    crowns = []
    for _ in range(3000):
        k = int(rng.integers(16, 65))
        angle = np.sort(rng.uniform(0, 2 * np.pi, k))
        radius = rng.uniform(30.0, 90.0) * rng.uniform(0.6, 1.0, k)
        centre = rng.uniform(0, side, 2)
        crowns.append(centre + np.stack([radius * np.cos(angle), radius * np.sin(angle)], axis=1))

    hip = HipRaster(0)
    result = {"grid": [side, side], "repeats": args.repeats, "zonal_Gcells_inside_per_s_of_8m": 4.0}
    window = (0, 0, side, side)
    for name, rings in (("tiling", tiling), ("crowns", crowns)):
        P = len(rings)
        rv, off = rings_to_cell_units(rings, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0))
        rp = np.arange(P, dtype=np.int32)
        values = (np.arange(P) % 251).astype(np.uint8)
        t0 = time.perf_counter()
        boxes, ranges = row_centre_boxes(rv, off, rp, P), row_ring_ranges(rp, P)
        t1 = time.perf_counter()
        items = burn_work_items(boxes, ranges, window)
        t2 = time.perf_counter()
        burner = hip.polygon_burner(rv, off, rp, P, values)
        items_t = hip._dev(items, torch.int32)
        out, median, best = timed(torch, args.repeats, lambda: burner.window(*window, items_t))
        _, median_rows, _ = timed(torch, args.repeats, lambda: burner.window(*window, items_t, want_values=False))
        rows, stats = out[0].cpu().numpy(), out[2].cpu().tolist()
        t3 = time.perf_counter()
        want = burn_numpy(rv, off, rp, boxes.tolist(), side)
        t4 = time.perf_counter()
        assert np.array_equal(rows, want), name
        assert np.array_equal(out[1].cpu().numpy(), np.where(want >= 0, values[np.maximum(want, 0)], 255)), name
        assert stats[2] == int((want >= 0).sum())
        if name == "tiling":
            assert stats[1] == stats[2] == side * side
        result[name] = {"polygons": P, "ring_vertices": int(len(rv)), "work_items": int(len(items)), "cells_tested": stats[0],
                        "memberships": stats[1], "cells_burned": stats[2], "median_ms": round(median, 3), "best_ms": round(best, 3),
                        "rows_only_median_ms": round(median_rows, 3), "Gcells_per_s": round(side * side / median / 1e6, 2),
                        "Gcells_tested_per_s": round(stats[0] / median / 1e6, 2), "host_boxes_ms": round(1e3 * (t1 - t0), 1),
                        "host_items_ms": round(1e3 * (t2 - t1), 1), "numpy_s": round(t4 - t3, 2)}
    # write_chips end to end, with and without labels
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        transform = (0.05, 0.0, 600000.0, 0.0, -0.05, 4200000.0)
        ramp = (np.add.outer(np.arange(side), np.arange(side)) % 251).astype(np.uint8)
        rgb = np.stack([ramp, ramp[::-1], ramp[:, ::-1]], axis=2)
        write_tiff_deflate(tmp / "ortho.tif", rgb, level=1, transform=transform, epsg=32610)
        features = [{"type": "Feature", "properties": {"code": int(1 + p % 250)},
                     "geometry": {"type": "Polygon", "coordinates": [[[600000.0 + 0.05 * x, 4200000.0 - 0.05 * y] for x, y in np.vstack([ring, ring[:1]])]]}}
                    for p, ring in enumerate(crowns)]
        (tmp / "crowns.geojson").write_text(json.dumps({"type": "FeatureCollection", "features": features,
                                                        "crs": {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::32610"}}}))
        chips = {}
        for name, kw in (("imagery_only", {}), ("with_labels", dict(label_vector_file=tmp / "crowns.geojson", label_column="code",
                                                                    write_empty_tiles=True, backend=hip))):
            t0 = time.perf_counter()
            written = og.write_chips(tmp / "ortho.tif", tmp / name, 2048, 2048, **kw)
            chips[name] = {"chips": len(written), "seconds": round(time.perf_counter() - t0, 2)}
        result["write_chips"] = dict(chip=2048, stride=2048, **chips)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
