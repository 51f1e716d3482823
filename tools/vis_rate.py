#!/usr/bin/env python3
"""Rates of the picture calls on one MI355X -> profiles/vis_rate.json (recorded, not asserted; DESIGN.md 8s "Measured").

HIP events around the binding's call (output allocation included), the median of 5 after a warm-up.
  gr_composite_labels  4000 x 3000, uint8 photo and uint8 discrete label: the time and the share of an 8 TB/s HBM peak, counting the
                       photo and the label read once and 9 bytes a pixel written.
  gr_shade_view        1920 x 1080 and 3840 x 2160 pictures at 1 / 2 / 4 samples a side, on the C2 terrain and on the forest scene
                       from the default view of `TexturedPhotogrammetryMesh.vis`; the raster call that makes the planes is timed
                       beside it for context.
  the numpy stand-in   (tests/vis_standin.py) on this host at the smallest of those sizes, for context.
A size that fails (memory, a limit of the raster path) is recorded as "not measured" with the reason.

    python tools/vis_rate.py [--quick]
    python tools/vis_rate.py --forest-pictures FOLDER     the pictures the default occlusion strength was chosen on
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from geograypher_amd._hip import HipRaster  # noqa: E402
from geograypher_amd.cameras import vtk_like_near_plane  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.meshes import vis as mesh_vis  # noqa: E402
from geograypher_amd.meshes.meshes import LocalMesh  # noqa: E402
from geograypher_amd.utils import colormaps, synthetic  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, repeats=5):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def composite_rate(backend, h=3000, w=4000):
    rng = np.random.default_rng(0)
    photo = backend._dev(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), torch.uint8)
    label = backend._dev(rng.integers(0, 10, (h, w), dtype=np.uint8), torch.uint8)
    table = backend._dev(colormaps.table("tab10"), torch.float64)
    ms = timed(lambda: backend.composite_labels(photo, label, table, True, 0.0, 1.0, 0.5, True))
    moved = h * w * (3 + 1 + 9)
    return {"size": [w, h], "ms": ms, "bytes": moved, "share_of_8TBs_peak": moved / (ms * 1e-3) / HBM_PEAK}


def shade_rates(backend, name, points, faces, sizes, samples):
    mesh = TexturedPhotogrammetryMesh((points, faces), backend=backend, log_level="ERROR")
    pts = np.asarray(points, dtype=np.float64)
    to_picture = mesh_vis.picture_frame((pts.min(axis=0) + pts.max(axis=0)) / 2.0)
    scene = LocalMesh(np.ascontiguousarray(pts @ to_picture[:3, :3].T + to_picture[:3, 3]), np.asarray(faces, dtype=np.int64))
    rgb = backend._dev(np.random.default_rng(1).integers(0, 256, (len(faces), 3), dtype=np.uint8), torch.uint8)
    out = []
    for (W, H) in sizes:
        for s in samples:
            row = {"scene": name, "picture": [W, H], "supersample": s}
            try:
                camera = mesh_vis.view_camera(None, scene.points, (H * s, W * s), to_picture, None)
                near = vtk_like_near_plane(np.asarray(camera.cam_to_world_transform), scene.bounds())
                records, (h, w) = mesh._raster_records(camera, scene, 1.0, near=near)
                ids, depth = backend.raster_face_ids(records, h, w, want_depth=True)
                light = backend.face_light(scene.points.astype(np.float32), scene.faces.astype(np.int32),
                                           np.asarray(camera.cam_to_world_transform)[:3, 2], mesh_vis.AMBIENT)
                row["raster_ms"] = timed(lambda: backend.raster_face_ids(records, h, w, want_depth=True, check=False), 3)
                row["shade_ms"] = timed(lambda: backend.shade_view(ids[0], depth[0], rgb, light, s, s, mesh_vis.SSAO_STRENGTH))
                row["shade_flat_ms"] = timed(lambda: backend.shade_view(ids[0], depth[0], rgb, light, s, s, 0.0))
                row["covered"] = float((ids[0] >= 0).float().mean().item())
                del ids, depth
            except Exception as error:   # a size the device or the raster path does not take: recorded, not hidden
                row["not_measured"] = f"{type(error).__name__}: {error}"[:300]
            torch.cuda.empty_cache()
            out.append(row)
            print(row, flush=True)
    return out


def standin_context():
    import vis_standin as vs

    rng = np.random.default_rng(2)
    h, w = 1080, 1920
    photo, label = rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 10, (h, w), dtype=np.uint8)
    t0 = time.perf_counter()
    vs.composite(photo, label, colormaps.table("tab10"), True, 0.0, 1.0, 0.5, True)
    composite_s = time.perf_counter() - t0
    ids = rng.integers(-1, 1000, (h, w)).astype(np.int32)
    depth = (rng.random((h, w)) + 1.0).astype(np.float32)
    rgb, light = rng.integers(0, 256, (1000, 3), dtype=np.uint8), rng.integers(0, 256, (1000,), dtype=np.uint8)
    t0 = time.perf_counter()
    vs.shade_view(ids, depth, rgb, light, 1, 1, 0.75)
    return {"size": [w, h], "composite_s": composite_s, "shade_s": time.perf_counter() - t0}


def forest_pictures(backend, folder, strengths=(0.0, 0.75, 8.0, 16.0, 32.0)):
    """The pictures the default occlusion strength of `vis` was chosen on: 3 000 trees on a 200 m terrain, coloured by
    height, 480 x 360 at two samples a side from the default view, one PNG per strength: <folder>/forest_k<strength>.png."""
    points, faces = synthetic.forest_scene(n_trees=3000, n_side=200, extent=200.0)
    mesh = TexturedPhotogrammetryMesh((points, faces), backend=backend, log_level="ERROR")
    heights = points[:, 2][faces].mean(axis=1)
    for k in strengths:
        target = Path(folder, f"forest_k{k:g}.png")
        mesh_vis.render(mesh, screenshot_filename=target, vis_scalars=heights, window_size=(480, 360), supersample=2,
                        enable_ssao=k > 0, ssao_strength=k)
        print(f"wrote {target}", flush=True)


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--quick", action="store_true", help="C1 in place of C2 and the forest, 1920 x 1080 only")
    parser.add_argument("--forest-pictures", type=Path, metavar="FOLDER",
                        help="Only write the forest scene at occlusion strengths 0 / 0.75 / 8 / 16 / 32 into FOLDER (not kept in the tree)")
    args = parser.parse_args()
    backend = HipRaster(0)
    if args.forest_pictures is not None:
        forest_pictures(backend, args.forest_pictures)
        return
    result = {"device": torch.cuda.get_device_name(0), "composite": composite_rate(backend)}
    print(result["composite"], flush=True)
    sizes = [(1920, 1080)] if args.quick else [(1920, 1080), (3840, 2160)]
    scenes = {"c1": synthetic.config1_scene()[0]} if args.quick else {"c2": synthetic.terrain_mesh(), "forest": synthetic.forest_scene()[:2]}
    result["shade"] = []
    for name, (points, faces) in scenes.items():
        result["shade"] += shade_rates(backend, name, points, faces, sizes, (1, 2, 4))
    result["standin_on_this_host"] = standin_context()
    result["save_renders_with_and_without_composites"] = "not measured"
    out = ROOT / "profiles" / "vis_rate.json"
    out.parent.mkdir(exist_ok=True)
    out.write_text(json.dumps(result, indent=1))
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
