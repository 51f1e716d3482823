#!/usr/bin/env python3
"""tools/image_selection_rate.py -- rate of the image selection (gr_set_cover) on the visibility matrices of
C3 (utils/synthetic.terrain_mesh: 1 201 250 faces, config3_cameras: 500 views) and of one GPU's share of C5 (config5_scene:
4 999 122 faces, every 8th of its 2000 views: 250), each taken from the projection path itself: every view labelled with its own
index, `TexturedPhotogrammetryMeshIndexPredictions.aggregate_projected_images` at --scale of the image size.

  device      HIP events around HipRaster.set_cover with the CSR already on the device, its read-backs (the control words once
              per batch, the record at the end) included; median and best of --repeats after a warm-up; greedy alone and
              greedy + prune; through the LDS histograms and -- where the view count allows both -- through global atomics
  end to end  utils.numeric.select_covering_views with a host clock: canonical CSR, upload, the device call, the record
  host        the numpy / scipy stand-in of the rule-set (tests/setcover_standin.py) on this host's CPUs, same matrix

The tool ASSERTS that every array of the device record equals the stand-in's.  Writes profiles/image_selection_rate.json (and
prints it as one JSON line).  No pass / fail bar on the rates: nobody has measured this stage before, and SetCoverPy runs
neither here nor where this project is built.

    python tools/image_selection_rate.py [--repeats 5] [--scenes c3 c5] [--scale 0.25]
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


def scene(name):
    from geograypher_amd.utils import synthetic

    if name == "c3":
        return synthetic.terrain_mesh(), synthetic.config3_cameras(500)
    (points, faces), cams = synthetic.config5_scene(2000)
    return (points, faces), cams.get_subset_cameras(list(range(0, 2000, 8)))


def visibility(mesh, cams, scale):
    """The (faces, views) matrix of the workflow, without image files: the segmentor answers from the cameras' own sizes."""
    from geograypher_amd.cameras.segmentor import SegmentorPhotogrammetryCameraSet
    from geograypher_amd.predictors.derived_segmentors import ImageIDSegmentor

    sizes = {cams.get_image_filename(i, absolute=True): cams[i].get_image_size(1.0) for i in range(len(cams))}

    class SizedImageIDs(ImageIDSegmentor):
        def _shape_and_index(self, filename, image_scale):
            h, w = sizes[filename]
            return (int(h * image_scale), int(w * image_scale)), self.image_filenames.index(filename)

    segmentor = SizedImageIDs(cams.get_image_filename(index=None, absolute=True))
    _, info = mesh.aggregate_projected_images(SegmentorPhotogrammetryCameraSet(cams, segmentor), n_classes=len(cams),
                                              aggregate_img_scale=scale)
    return info["summed_projections"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scenes", nargs="+", choices=["c3", "c5"], default=["c3", "c5"])
    ap.add_argument("--scale", type=float, default=0.25)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "image_selection_rate.json")
    args = ap.parse_args()
    import torch
    from scipy import sparse

    from geograypher_amd import _hip
    from geograypher_amd.meshes import TexturedPhotogrammetryMeshIndexPredictions
    from geograypher_amd.utils.numeric import select_covering_views
    from tests import setcover_standin as standin

    if not torch.cuda.is_available():
        raise SystemExit("image_selection_rate: no GPU; a rate is measured on the device or not at all")
    res = {"aggregate_img_scale": args.scale, "repeats": args.repeats, "batch": _hip.GR_SETCOVER_BATCH,
           "lds_views": _hip.GR_SETCOVER_LDS_VIEWS, "runs": []}
    arrays = ("selected", "order", "gains", "pruned")
    for name in args.scenes:
        (points, faces), cams = scene(name)
        mesh = TexturedPhotogrammetryMeshIndexPredictions((points, faces), log_level="ERROR")
        hip = mesh.backend
        t0 = time.perf_counter()
        summed = visibility(mesh, cams, args.scale)
        t_projection = time.perf_counter() - t0
        csr = sparse.csr_matrix(summed, copy=True)
        csr.sum_duplicates(); csr.eliminate_zeros(); csr.sort_indices()
        F, N = csr.shape
        ptr, views = hip._dev(csr.indptr.astype(np.int64), torch.int64), hip._dev(csr.indices.astype(np.int32), torch.int32)
        run = {"scene": name, "faces": int(F), "views": int(N), "nnz": int(csr.nnz), "projection_s": round(t_projection, 2),
               "faces_seen": int((np.diff(csr.indptr) > 0).sum()), "device": {}}
        want = {}
        for prune in (False, True):
            t0 = time.perf_counter()
            want[prune] = standin.set_cover(csr, 1, prune)
            run["host_standin_s_" + ("greedy_prune" if prune else "greedy")] = round(time.perf_counter() - t0, 3)
        for path, global_atomics in (("lds_histogram", False), ("global_atomics", True)):
            for prune in (False, True):
                got = hip.set_cover(ptr, views, F, N, prune=prune, global_atomics=global_atomics)
                assert got["lds_histogram"] == (not global_atomics)
                for key in arrays:
                    assert np.array_equal(got[key], want[prune][key]), f"{name} {path} prune={prune}: {key} differs from the stand-in"
                assert (got["n_required"], got["n_covered"]) == (want[prune]["n_required"], want[prune]["n_covered"])
                med, best = timed(lambda: hip.set_cover(ptr, views, F, N, prune=prune, global_atomics=global_atomics), args.repeats)
                run["device"][path + ("_greedy_prune" if prune else "_greedy")] = {"ms_median": med, "ms_best": best}
                run.update(k=int(len(got["order"])), p=int(len(got["pruned"])) if prune else run.get("p", 0),
                           batches=int(got["batches"]), n_required=int(got["n_required"]))
        run["selected"] = int(want[True]["selected"].sum())
        e2e = []
        for _ in range(max(2, args.repeats // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            record = select_covering_views(summed, backend=hip)
            e2e.append(time.perf_counter() - t0)
        assert np.array_equal(record["selected"], want[True]["selected"])
        run["end_to_end_s_best"] = round(min(e2e), 3)
        run["device_equals_standin_on_every_array"] = True
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
        del mesh, hip, ptr, views
    res["host_cpus"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    res["device"] = torch.cuda.get_device_name(0)
    res["reference_note"] = "the reference's SetCoverPy stage on the dense matrix publishes no rate and cannot run without SetCoverPy"
    line = json.dumps(res)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
