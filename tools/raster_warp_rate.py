#!/usr/bin/env python3
"""tools/raster_warp_rate.py -- rate of the raster -> raster call (gr_warp_raster) on two rasters a user would warp: a
1-band float32 DTM and a 4-band uint8 orthomosaic (RGBA), generated from a seed in UTM zone 10, data resident on the device.

  same CRS   nearest and bilinear onto a grid of the same extent at 0.8 of the cell size (1.5625 x the cells).  Beside the time,
             the bytes the call cannot avoid -- every source byte read once, every destination byte written once -- the rate they
             amount to, and its share of the 6.29 TB/s a float4 copy reaches on this chip (the streaming roof; 8 TB/s is the
             spec).  The bilinear call reads every source cell through up to four taps; the caches serve the repeats, so the same
             bytes are counted
  cross CRS  nearest and bilinear onto the default grid in EPSG:4326 (`default_warp_grid`): destination cells per second, beside the
             points per second of gr_reproject_points for the same conversion (EPSG:4326 -> EPSG:32610) on as many points
  host       the numpy stand-in (tests/warp_raster_standin.py) on a 1/16 crop of the DTM, on this host's CPUs, and whether the
             device's planes equal it (same CRS: byte for byte)

HIP events around the enqueued call, the output preallocated; median and best of --repeats after a warm-up of the same shape.
Writes profiles/raster_warp_rate.json (and prints it as one JSON line).  No pass / fail bar: the call is new, and rasterio runs
neither here nor where this project is built.

    python tools/raster_warp_rate.py [--repeats 5] [--dtm-side 8192] [--ortho-side 8192]
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

STREAM_ROOF_TB_S = 6.29
UTM10, GEO = 32610, 4326


def timed(fn, repeats):
    import torch

    fn()   # warm-up: code object load, this shape
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
    ap.add_argument("--dtm-side", type=int, default=8192)
    ap.add_argument("--ortho-side", type=int, default=8192)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "raster_warp_rate.json")
    args = ap.parse_args()
    import torch

    import warp_raster_standin as ws
    from geograypher_amd._hip import HipRaster
    from geograypher_amd.utils.geospatial import WGS84CRS, default_warp_grid
    from geograypher_amd.utils.raster import invert_affine

    if not torch.cuda.is_available():
        raise SystemExit("raster_warp_rate: no GPU; a rate is measured on the device or not at all")
    hip = HipRaster(0)
    gen = torch.Generator(device=hip.device).manual_seed(7)
    res = {"repeats": args.repeats, "stream_roof_tb_per_s": STREAM_ROOF_TB_S, "runs": []}
    rasters = {
        "dtm_float32_1_band": (torch.rand((1, args.dtm_side, args.dtm_side), generator=gen, device=hip.device, dtype=torch.float32) * 50.0 + 100.0,
                               0.5, -9999.0),
        "ortho_uint8_4_bands": (torch.randint(1, 256, (4, args.ortho_side, args.ortho_side), generator=gen, device=hip.device, dtype=torch.uint8),
                                0.05, 0.0),
    }
    for name, (data, cell, nodata) in rasters.items():
        B, H, W = (int(k) for k in data.shape)
        item = data.element_size()
        src_t = (cell, 0.0, 552000.3, 0.0, -cell, 4182014.7 + H * cell)
        inv = invert_affine(src_t)
        run = {"raster": name, "shape": [B, H, W], "cell_m": cell}
        # same CRS: the same extent at 0.8 of the cell size
        w2, h2 = int(W / 0.8), int(H / 0.8)
        dst_t = (cell * 0.8, 0.0, src_t[2], 0.0, -cell * 0.8, src_t[5])
        out = torch.empty((B, h2, w2), dtype=data.dtype, device=hip.device)
        moved = (B * H * W + B * h2 * w2) * item
        for resampling in ("nearest", "bilinear"):
            med, best = timed(lambda: hip.warp_raster(data, inv, nodata, dst_t, (0, 0, w2, h2), resampling=resampling, out=out), args.repeats)
            rate = moved / (med * 1e-3) / 1e12
            run[f"same_crs_{resampling}"] = {"destination": [h2, w2], "device_ms_median": med, "device_ms_best": best, "bytes_moved": moved,
                                             "achieved_tb_per_s": round(rate, 3), "share_of_stream_roof": round(rate / STREAM_ROOF_TB_S, 3),
                                             "gcells_per_s": round(h2 * w2 / (med * 1e-3) / 1e9, 2)}
        # cross CRS: the default grid in EPSG:4326
        (h3, w3), geo_t = default_warp_grid(((H, W), src_t), UTM10, GEO, hip)
        out = torch.empty((B, h3, w3), dtype=data.dtype, device=hip.device)
        for resampling in ("nearest", "bilinear"):
            med, best = timed(lambda: hip.warp_raster(data, inv, nodata, geo_t, (0, 0, w3, h3), src_crs=UTM10, dst_crs=GEO,
                                                      resampling=resampling, out=out), args.repeats)
            run[f"cross_crs_{resampling}"] = {"destination": [h3, w3], "device_ms_median": med, "device_ms_best": best,
                                              "mcells_per_s": round(h3 * w3 / (med * 1e-3) / 1e6, 1)}
        stats = hip.warp_raster(data, inv, nodata, geo_t, (0, 0, w3, h3), src_crs=UTM10, dst_crs=GEO, out=out)[1].cpu().numpy()
        run["cross_crs_stats"] = {k: int(v) for k, v in zip(ws.STAT_NAMES, stats)}
        # the same conversion on as many points through gr_reproject_points
        n = h3 * w3
        pts = torch.zeros((n, 3), dtype=torch.float64, device=hip.device)
        pts[:, 0] = geo_t[2] + torch.rand(n, generator=gen, device=hip.device, dtype=torch.float64) * (w3 * geo_t[0])
        pts[:, 1] = geo_t[5] + torch.rand(n, generator=gen, device=hip.device, dtype=torch.float64) * (h3 * geo_t[4])
        out_p = torch.empty_like(pts)
        med, best = timed(lambda: hip.reproject_points(pts, WGS84CRS.parse(GEO), WGS84CRS.parse(UTM10), out=out_p, check=False), args.repeats)
        run["reproject_points_same_conversion"] = {"points": n, "device_ms_median": med, "device_ms_best": best,
                                                   "mpoints_per_s": round(n / (med * 1e-3) / 1e6, 1)}
        del pts, out_p, out
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    # the numpy stand-in on a crop of the DTM, and the device against it
    data, cell, nodata = rasters["dtm_float32_1_band"]
    side = max(64, args.dtm_side // 4)
    crop = data[:, :side, :side].contiguous()
    crop_h = crop.cpu().numpy()
    src_t = (cell, 0.0, 552000.3, 0.0, -cell, 4182014.7 + side * cell)
    inv = invert_affine(src_t)
    w2 = h2 = int(side / 0.8)
    dst_t = (cell * 0.8, 0.0, src_t[2], 0.0, -cell * 0.8, src_t[5])
    host = {"source": [1, side, side], "destination": [h2, w2]}
    for resampling, kind in (("nearest", ws.NEAREST), ("bilinear", ws.BILINEAR)):
        t0 = time.perf_counter()
        want, _, _, _ = ws.warp(crop_h, inv, nodata, dst_t, (0, 0, w2, h2), resampling=kind, dst_nodata=nodata)
        dt = time.perf_counter() - t0
        got = hip.warp_raster(crop, inv, nodata, dst_t, (0, 0, w2, h2), resampling=resampling)[0].cpu().numpy()
        host[f"same_crs_{resampling}"] = {"numpy_s": round(dt, 3), "numpy_mcells_per_s": round(h2 * w2 / dt / 1e6, 2),
                                          "device_equals_numpy_bytes": bool(got.tobytes() == want.tobytes())}
    (h3, w3), geo_t = default_warp_grid(((side, side), src_t), UTM10, GEO, hip)
    t0 = time.perf_counter()
    want, _, und, _ = ws.warp(crop_h, inv, nodata, geo_t, (0, 0, w3, h3), ws._crs(UTM10), ws._crs(GEO), ws.NEAREST, nodata)
    dt = time.perf_counter() - t0
    got = hip.warp_raster(crop, inv, nodata, geo_t, (0, 0, w3, h3), src_crs=UTM10, dst_crs=GEO)[0].cpu().numpy()
    host["cross_crs_nearest"] = {"destination": [h3, w3], "numpy_s": round(dt, 3), "numpy_mcells_per_s": round(h3 * w3 / dt / 1e6, 3),
                                 "undetermined_cells": int(und.sum()), "cells_that_differ_outside_them": int(((got != want)[0] & ~und).sum())}
    res["numpy_standin"] = host
    res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    res["device"] = torch.cuda.get_device_name(0)
    res["reference_note"] = ("the reference warps with rasterio.warp.reproject (GDAL); it publishes no rate and rasterio is installed "
                             "neither here nor where this project is built, so parity with GDAL is unmeasured: the numpy restatement "
                             "stands in for the host")
    line = json.dumps(res)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
