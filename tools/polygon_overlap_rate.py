#!/usr/bin/env python3
"""tools/polygon_overlap_rate.py -- rate of the polygon-on-polygon overlap areas at the size a user would
run: --crowns (default 30 000) seeded star-shaped crowns of 16-64 vertices and 2-6 m radius over the 400 m footprint of the C2 mesh,

  class_map   against the class map of the C2 labelling as tools/face_outlines_rate.py builds it and
              TexturedPhotogrammetryMesh.export_face_labels_vector traces it -- one multi-part row per class --, "clean" and with 10 %
              of the faces flipped ("noisy").  The WORST case of the method: the box of every class row covers the footprint, so every
              crown pairs with every class row and every work item scans its whole b-tile for the x-cull
  copies      against as many jittered copies of themselves: many short rows on both sides, one work item a pair

  device      HIP events around PolygonOverlap.pairs (count, read-back, fill) and around PolygonOverlap.areas (the host check of the
              items included) with both tables, the pairs and the items already on the device; median and best of --repeats after a
              warm-up
  end to end  utils.geospatial.get_overlap_vector from the two (PlanarPolygons, columns) sources, with a host clock: snap, upload,
              pair join, item builder, areas, read-back, the matrix
  numpy       the restatement of rule A5 in float64 (tests/overlap_standin.py, restated_areas) on this host over a SAMPLE of --sample
              pairs, spread evenly over the pair list; the device's areas of the sample are ASSERTED within the bound of A6 of it; the
              time is extrapolated to all pairs by the pair count and marked as extrapolated

shapely and geopandas are installed neither here nor where this project is built: the reference's own time (gpd.overlay) is NOT
measured.  Writes profiles/polygon_overlap_rate.json (and prints it as one JSON line).  No pass / fail bar on the rates.

    python tools/polygon_overlap_rate.py [--repeats 5] [--crowns 30000] [--sample 24] [--out profiles/polygon_overlap_rate.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))


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
    return out, round(float(np.median(times)), 3), round(float(np.min(times)), 3)


def star_crowns(rng, n, lo, hi):
    """n star-shaped rings of 16-64 vertices, 2-6 m radius (star-shaped about the centre: simple)."""
    rings = []
    for _ in range(n):
        k = int(rng.integers(16, 65))
        angle = 2 * np.pi * (np.arange(k) + rng.uniform(0.0, 0.8, k)) / k + rng.uniform(0, 2 * np.pi)
        radius = rng.uniform(2.0, 6.0) * rng.uniform(0.6, 1.0, k)
        rings.append(rng.uniform(lo, hi) + np.stack([radius * np.cos(angle), radius * np.sin(angle)], axis=1))
    return rings


def measure(torch, hip, name, A, B, class_values, args):
    import overlap_standin as ov
    from geograypher_amd.utils import geospatial as gs
    from geograypher_amd.utils.geometric import overlap_work_items, snap_polygon_pair

    t0 = time.perf_counter()
    table_a, table_b, _ = snap_polygon_pair(A, B)
    t1 = time.perf_counter()
    overlap = hip.polygon_overlap(table_a, table_b)
    pairs_t, pairs_ms, pairs_best = timed(torch, args.repeats, overlap.pairs)
    pairs = pairs_t.cpu().numpy()
    t2 = time.perf_counter()
    items = overlap_work_items(table_a[1], table_a[2], table_b[1], table_b[2], pairs)
    t3 = time.perf_counter()
    items_t = hip._dev(items, torch.int32)
    (area, area_abs, stats), areas_ms, areas_best = timed(torch, args.repeats, lambda: overlap.areas(pairs_t, items_t))
    area, area_abs, stats = area.cpu().numpy(), area_abs.cpu().numpy(), stats.cpu().tolist()
    run = {"scene": name, "rows_a": len(A), "rows_b": len(B), "ring_vertices_a": int(len(table_a[0])), "ring_vertices_b": int(len(table_b[0])),
           "rings_b": int(len(table_b[2])), "pairs": int(len(pairs)), "work_items": int(len(items)), "edge_pairs_taking_part": stats[2],
           "edge_pairs_scanned": int((items[:, 2].astype(np.int64) * items[:, 4]).sum()), "pairs_above_bound": int((area > gs.overlap_bound(area_abs)).sum()),
           "device_pairs_ms_median": pairs_ms, "device_pairs_ms_best": pairs_best, "device_areas_ms_median": areas_ms, "device_areas_ms_best": areas_best,
           "host_snap_s": round(t1 - t0, 2), "host_items_s": round(t3 - t2, 2)}
    run["G_edge_pairs_scanned_per_s"] = round(run["edge_pairs_scanned"] / areas_ms / 1e6, 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    counts, ids, names = gs.get_overlap_vector((A, {}), (B, {"cls": class_values}), "cls", backend=hip)
    run["end_to_end_get_overlap_vector_s"] = round(time.perf_counter() - t0, 2)
    run["rows_intersecting"], run["classes"] = int(len(ids)), len(names)
    sample = np.unique(np.linspace(0, len(pairs) - 1, min(args.sample, len(pairs))).astype(np.int64))
    t0 = time.perf_counter()
    want, want_abs, _ = ov.restated_areas(table_a, table_b, pairs[sample])
    seconds = time.perf_counter() - t0
    assert np.all(np.abs(area[sample] - want) <= 2 * gs.overlap_bound(want_abs)), name
    run["numpy_sample_pairs"], run["numpy_sample_s"] = int(len(sample)), round(seconds, 2)
    run["numpy_all_pairs_s_EXTRAPOLATED"] = round(seconds * len(pairs) / max(len(sample), 1), 1)
    print(json.dumps(run), flush=True)
    return run


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--crowns", type=int, default=30000)
    ap.add_argument("--sample", type=int, default=24)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "polygon_overlap_rate.json")
    args = ap.parse_args()
    import torch

    from face_outlines_rate import crown_classes
    from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh
    from geograypher_amd.utils import synthetic
    from geograypher_amd.utils.geometric import PlanarPolygons

    if not torch.cuda.is_available():
        raise SystemExit("polygon_overlap_rate: no GPU; a rate is measured on the device or not at all")
    points, faces = synthetic.terrain_mesh()
    mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR")
    hip = mesh.backend
    rng = np.random.default_rng(0)
    lo, hi = points[:, :2].min(axis=0), points[:, :2].max(axis=0)
    rings = star_crowns(rng, args.crowns, lo, hi)
    crowns = PlanarPolygons(rings, np.arange(len(rings)), np.zeros(len(rings), dtype=bool))
    result = {"crowns": args.crowns, "crown_vertices": [16, 64], "repeats": args.repeats, "tiles": [256, 4096], "runs": []}
    for kind, classes in zip(("clean", "noisy"), crown_classes(points, faces, 400.0)):
        class_map, columns = mesh.export_face_labels_vector(np.where(classes < 0, np.nan, classes), None, points_in_export_CRS=points)
        values = [str(v) for v in columns["class_ID"]]
        result["runs"].append(measure(torch, hip, f"class_map_{kind}", crowns, class_map, values, args))
    copies = PlanarPolygons([r + rng.uniform(-1.0, 1.0, 2) + rng.uniform(-0.1, 0.1, r.shape) for r in rings], np.arange(len(rings)),
                            np.zeros(len(rings), dtype=bool))
    args.sample = max(args.sample, 2000)
    result["runs"].append(measure(torch, hip, "copies", crowns, copies, [str(k % 3) for k in range(len(rings))], args))
    result["device"] = torch.cuda.get_device_name(0)
    result["reference_note"] = "gpd.overlay / shapely.intersection are not installed on either machine: the reference's time is not measured"
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
