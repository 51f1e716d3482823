#!/usr/bin/env python3
"""tools/equirect_rate.py -- sample rate of the equirectangular-to-perspective resampling (gr_equirect_view) at the entrypoint's
default sizes: one 4096 x 8192 x 3 uint8 photo, the six views of FYPS at 1920 x 1920 and 4x oversampling (354 M samples).

  device      HIP events around the six enqueued views of one photo (the photo already on the device, outputs left there), best
              and median of --repeats after a warm-up; and end to end through perspectives_from_equirectangular with a host clock
              (upload of the photo, six views, every view copied back to numpy)
  stand-in    the numpy restatement (tests/equirect_standin.py) on this host's CPUs, one view at --standin-size (the full-size
              view would need tens of GB of temporaries); numpy, like the reference's skimage path, runs it on one core

Writes profiles/equirect_rate.json (and prints it as one JSON line).  A sample is one bilinear look-up of all three channels.

    python tools/equirect_rate.py [--repeats 5] [--standin-size 480]
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

# the real reference function on one 480 x 480 view at 4x oversampling took 1.6 s where the goldens were made (scikit-image
# 0.18.3): a constant from ANOTHER machine, quoted for scale only
REFERENCE_MSAMPLES_PER_S_OTHER_MACHINE = 480 * 480 * 16 / 1.6 / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--standin-size", type=int, default=480)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "equirect_rate.json")
    args = ap.parse_args()
    import torch

    import equirect_standin as standin
    from geograypher_amd._hip import HipRaster
    from geograypher_amd.entrypoints.equirectangular_to_cube_mapped import FYPS, OUTPUT_SIZE, OVERSAMPLE_FACTOR
    from geograypher_amd.utils.image import _view_axes, perspectives_from_equirectangular, rotate_by_roll_pitch_yaw

    if not torch.cuda.is_available():
        raise SystemExit("equirect_rate: no GPU; a rate is measured on the device or not at all")
    hip = HipRaster(0)
    rng = np.random.default_rng(0)
    photo = rng.integers(0, 256, size=(4096, 8192, 3), dtype=np.uint8)
    os_ = OVERSAMPLE_FACTOR
    samples_per_photo = len(FYPS) * OUTPUT_SIZE[0] * OUTPUT_SIZE[1] * os_ * os_

    # -- device time of the six views: the binding's own call, outputs kept on the device -------------------------------------
    import ctypes

    source = hip.equirect_upload(photo)
    H, W, C = source.shape
    prepared = []
    for fov, yaw, pitch in FYPS:
        x, y = _view_axes(fov, OUTPUT_SIZE, os_)
        xy = torch.as_tensor(np.concatenate([x, y])).to(hip.device)
        R = (ctypes.c_double * 9)(*rotate_by_roll_pitch_yaw(0, pitch, yaw).reshape(9))
        out = torch.empty(OUTPUT_SIZE + (C,), dtype=torch.float64, device=hip.device)
        prepared.append((xy, len(x), R, out))

    def six_views():
        for xy, nx, R, out in prepared:
            rc = hip.lib.gr_equirect_view(hip._ctx, source.tensor.data_ptr(), 0, H, W, C, xy.data_ptr(), xy.data_ptr() + 8 * nx, R,
                                          OUTPUT_SIZE[0], OUTPUT_SIZE[1], os_, 1, source.vmin, source.vrange,
                                          source.bounds.data_ptr(), out.data_ptr(), None, None, hip._stream())
            hip._check(rc, "gr_equirect_view")

    six_views()   # warm-up: code object load
    torch.cuda.synchronize()
    device_ms = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        six_views()
        b.record()
        b.synchronize()
        device_ms.append(a.elapsed_time(b))

    # -- end to end: upload, six views, each copied back ----------------------------------------------------------------------
    list(perspectives_from_equirectangular(photo, FYPS[:1], output_size=OUTPUT_SIZE, oversample_factor=os_, backend=hip))
    e2e_s = []
    for _ in range(max(2, args.repeats // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        views = list(perspectives_from_equirectangular(photo, FYPS, output_size=OUTPUT_SIZE, oversample_factor=os_, backend=hip))
        e2e_s.append(time.perf_counter() - t0)
    assert len(views) == 6 and views[0].shape == OUTPUT_SIZE + (3,)

    # -- the stand-in on this host's CPUs ---------------------------------------------------------------------------------------
    n = args.standin_size
    fov, yaw, pitch = FYPS[3]
    t0 = time.perf_counter()
    want = standin.perspective_from_equirectangular_np(photo, fov, (n, n), yaw, pitch, 0, 1, os_)
    standin_s = time.perf_counter() - t0
    got = next(iter(perspectives_from_equirectangular(photo, [FYPS[3]], output_size=(n, n), oversample_factor=os_, backend=hip)))
    standin_samples = n * n * os_ * os_

    best, med = min(device_ms), float(np.median(device_ms))
    res = {
        "photo": "4096x8192x3 uint8", "views": len(FYPS), "output_size": list(OUTPUT_SIZE), "oversample_factor": os_,
        "samples_per_photo": samples_per_photo,
        "device_ms_per_photo_best": round(best, 3), "device_ms_per_photo_median": round(med, 3), "repeats": args.repeats,
        "device_msamples_per_s": round(samples_per_photo / (med * 1e-3) / 1e6, 1),
        "device_photos_per_s": round(1e3 / med, 3),
        "end_to_end_s_per_photo_best": round(min(e2e_s), 4),
        "end_to_end_photos_per_s": round(1.0 / min(e2e_s), 3),
        "end_to_end_msamples_per_s": round(samples_per_photo / min(e2e_s) / 1e6, 1),
        "standin_view": f"{n}x{n} at {os_}x, same photo", "standin_s": round(standin_s, 3),
        "standin_msamples_per_s": round(standin_samples / standin_s / 1e6, 3),
        "standin_photos_per_s": round(standin_samples / standin_s / samples_per_photo, 6),
        "device_over_standin": round((samples_per_photo / (med * 1e-3)) / (standin_samples / standin_s), 1),
        "standin_view_max_abs_diff_to_device": float(np.abs(got - want).max()),
        "host_cpus": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count(),
        "reference_msamples_per_s_other_machine": round(REFERENCE_MSAMPLES_PER_S_OTHER_MACHINE, 2),
        "reference_note": "constant from another machine (where the goldens were made), not measured here",
    }
    line = json.dumps(res)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
