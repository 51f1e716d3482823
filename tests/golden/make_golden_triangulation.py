"""tests/golden/make_golden_triangulation.py -- goldens of the multiview-detection workflow, made by the REAL reference
functions (geograypher/utils/numeric.py, cameras/cameras.py) with numpy and networkx; the modules the reference imports but
these functions never call are stubbed as in SURVEY.md Appendix B:

    PYTHONPATH=<reference checkout> python tests/golden/make_golden_triangulation.py

Output: tests/golden/reference_triangulation.npz -- data only.  Per scene <s> in a (synthetic survey, ~200 rays), b (integer
coordinates, pair by pair, no edge lists -- see ref_dist: parallel, collinear overlapping / disjoint, touching, duplicate, zero-length segments), c (rays sharing origins):
  <s>__starts, __ends, __ids        the inputs
  <s>__dist64                       compute_approximate_ray_intersections(clamp=True)[2], float64 inputs
  <s>__distld_hi, __distld_lo       the same with np.longdouble inputs, as a pair hi (float64) + lo (float32)
  <s>__e_ref                        max |dist64 - distld| over the finite pairs: the reference's own float64 error
  <s>__thresholds                   the thresholds tested; the maker asserts that no candidate pair lies within 4 e_ref of one
  <s>__edges__t<k>__s<step>__<tr>   calc_graph_weights(...): rows (i, j, weight), in the reference's order (tr: none / sq)
  a__avg_inds / a__avg, b__avg      intersection_average of a few rays
  a__graph_nodes                    the nodes of networkx.Graph(edges) at thresholds[1] (what calc_communities must label)
Cameras: cast__* (the golden Metashape camera and a copy with a homogeneous scale), seg__* (calc_line_segments without
boundaries over three cameras and the committed tabular detections, with and without limit_angle_from_vert).
Clip: clip__* -- a ray set against two small meshes, the float64 error of the test stand-in measured against long double.
"""
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(HERE))
OUT = HERE / "reference_triangulation.npz"

from make_golden_tabular import DATA, IMAGE_SHAPE, stub_missing_modules  # noqa: E402


def scene_b():
    seg = [
        ((0, 0, 0), (4, 0, 0)),     # 0 base, along x
        ((1, 2, 0), (3, 2, 0)),     # 1 parallel, overlapping, 2 away
        ((2, 0, 0), (6, 0, 0)),     # 2 collinear, overlapping
        ((6, 0, 0), (9, 0, 0)),     # 3 collinear, disjoint (after), touching 2's end
        ((-5, 0, 0), (-2, 0, 0)),   # 4 collinear, disjoint (before)
        ((4, 0, 0), (4, 3, 0)),     # 5 touching 0's end, perpendicular
        ((0, 0, 0), (4, 0, 0)),     # 6 duplicate of 0 (another image)
        ((2, 2, 2), (2, 2, 2)),     # 7 zero length
        ((4, 0, 0), (0, 0, 0)),     # 8 0 reversed (anti-parallel)
        ((7, 1, 0), (5, 1, 0)),     # 9 anti-parallel, after
        ((2, -1, 1), (2, 1, 1)),    # 10 skew, crossing above 0 at height 1
        ((0, 0, 3), (0, 0, 5)),     # 11 along z above the origin
        ((1, 1, 1), (5, 1, 1)),     # 12 parallel to 0, offset
        ((-3, 2, 0), (-1, 2, 0)),   # 13 parallel, before, offset
        ((0, 0, 0), (0, 8, 0)),     # 14 along y from the origin
        ((0, 0, 0), (4, 0, 0)),     # 15 duplicate of 0 in the SAME image as 0
    ]
    starts = np.array([s for s, _ in seg], dtype=np.float64)
    ends = np.array([e for _, e in seg], dtype=np.float64)
    ids = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 1, 2, 3, 4, 5, 0])
    return starts, ends, ids


def scene_c():
    rng = np.random.default_rng(3)
    origins = np.array([[0.0, 0.0, 50.0], [30.0, 5.0, 60.0], [-10.0, 20.0, 55.0]])
    starts, ends, ids = [], [], []
    for k, o in enumerate(origins):
        for r in range(8):
            target = np.array([rng.uniform(-20, 40), rng.uniform(-20, 40), 0.0])
            starts.append(o)
            ends.append(o + 1.2 * (target - o))
            ids.append(3 * r + k if r % 2 else k)   # rays of one origin in the same and in different images
    return np.array(starts), np.array(ends), np.array(ids)


def hi_lo(x):
    hi = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        lo = np.asarray(x - hi.astype(np.longdouble), dtype=np.float64)
    return hi, np.where(np.isfinite(hi), lo, 0.0).astype(np.float32)   # (lo < 2^-53 |hi|: float32 keeps it to 2^-77 |hi|)


def main():
    stub_missing_modules()
    from geograypher.cameras.cameras import PhotogrammetryCamera, PhotogrammetryCameraSet
    from geograypher.predictors.derived_segmentors import TabularRectangleSegmentor
    from geograypher.utils import numeric as ref
    import networkx

    from geograypher_amd.utils import synthetic
    from tests import ray_standin

    out = {}
    survey = synthetic.detection_survey(n_objects=10, n_cameras=40, seed=0)
    scenes = {
        "a": (survey["ray_starts"], survey["ray_ends"], survey["ray_IDs"], (0.1, 0.5, 4.0)),
        "b": scene_b() + ((0.0, 1.0, 2.5),),
        "c": scene_c() + ((0.05, 1.0),),
    }
    for name, (starts, ends, ids, thresholds) in scenes.items():
        n = len(starts)
        def ref_dist(s, e):
            if name != "b":
                return ref.compute_approximate_ray_intersections(s, e, s, e, clamp=True)[2]
            # The reference's `before` / `after` branches index (N, 1, 3) arrays with an (N, N) mask (numeric.py:180-196) and
            # raise IndexError for N > 1, so the pairs of this scene go through the real function one at a time (N = 1).
            d = np.empty((n, n), dtype=s.dtype)
            for i in range(n):
                for j in range(n):
                    d[i, j] = ref.compute_approximate_ray_intersections(s[i:i + 1], e[i:i + 1], s[j:j + 1], e[j:j + 1],
                                                                        clamp=True)[2][0, 0]
            return d

        with np.errstate(all="ignore"):
            d64 = ref_dist(starts, ends)
            dld = ref_dist(starts.astype(np.longdouble), ends.astype(np.longdouble))
        assert dld.dtype == np.longdouble
        fin = np.isfinite(d64) & np.isfinite(dld)
        assert np.array_equal(np.isfinite(d64), np.isfinite(dld))
        e_ref = float(np.max(np.abs(d64.astype(np.longdouble) - dld)[fin]))
        cand = np.triu(np.ones((n, n), dtype=bool), 1) & (ids[:, None] != ids[None, :]) & fin
        if name != "b":   # b is compared bit for bit with dist64 (every intermediate is exact): ties at a threshold are the point
            for t in thresholds:
                gap = float(np.min(np.abs(dld[cand] - t)))
                assert gap > 4 * e_ref, (name, t, gap, e_ref)
                print(f"scene {name}: nearest pair to threshold {t}: {gap:.3g} (tol {4 * e_ref:.3g})")
        hi, lo = hi_lo(dld)
        out.update({f"{name}__starts": starts, f"{name}__ends": ends, f"{name}__ids": ids, f"{name}__dist64": d64,
                    f"{name}__distld_hi": hi, f"{name}__distld_lo": lo, f"{name}__e_ref": np.float64(e_ref),
                    f"{name}__thresholds": np.array(thresholds)})
        print(f"scene {name}: {n} rays, e_ref {e_ref:.3g}")
        if name == "b":   # ... and calc_graph_weights cannot run on it at all: the GPU test derives b's edge sets from dist64
            continue
        steps = (max(n // 3, 2), n + 7)
        for k, t in enumerate(thresholds):
            for step in steps:
                for tag, tr in (("none", None), ("sq", lambda x: x ** 2)):
                    if tag == "sq" and k != 1:
                        continue
                    with np.errstate(all="ignore"):
                        edges = ref.calc_graph_weights(starts, ends, ids, t, step=step, transform=tr)
                    rows = np.array([(i, j, w["weight"]) for i, j, w in edges], dtype=np.float64).reshape(-1, 3)
                    out[f"{name}__edges__t{k}__s{step}__{tag}"] = rows
        out[f"{name}__steps"] = np.array(steps)
    # intersection_average
    inds = np.nonzero(survey["ray_objects"] == 0)[0]
    out["a__avg_inds"] = inds
    out["a__avg"] = ref.intersection_average(survey["ray_starts"][inds], survey["ray_ends"][inds])
    sb, eb, _ = scene_b()
    pick = np.array([0, 5, 10, 14])   # (no before / after pair among them)
    out["b__avg_inds"] = pick
    out["b__avg"] = ref.intersection_average(sb[pick], eb[pick])
    with np.errstate(all="ignore"):
        edges = ref.calc_graph_weights(survey["ray_starts"], survey["ray_ends"], survey["ray_IDs"], 0.5)
    out["a__graph_nodes"] = np.array(sorted(networkx.Graph(edges).nodes))

    # cameras: the golden Metashape camera (reference_cameras.npz holds what the reference parsed from the XML)
    with np.load(HERE / "reference_cameras.npz") as g:
        f, cx, cy = float(g["f"]), float(g["cx"]), float(g["cy"])
        w, h = int(g["image_width"]), int(g["image_height"])
        T0 = g["cam_to_world"].astype(np.float64)
    pix = np.array([[0.0, 0.0], [h / 2.0, w / 2.0], [h - 1.0, w - 1.0], [123.5, 2001.25], [2500.0, 17.0]])
    cam = PhotogrammetryCamera("img0.png", T0, f, cx, cy, w, h)
    out["cast__pixels"] = pix
    out["cast__len10"] = cam.cast_rays(pix)
    out["cast__len1000"] = cam.cast_rays(pix, line_length=1e3)
    Ts = T0.copy()
    Ts[3, 3] = 2.0
    out["cast__scaled_transform"] = Ts
    out["cast__scaled"] = PhotogrammetryCamera("img0.png", Ts, f, cx, cy, w, h).cast_rays(pix, line_length=7.0)
    assert cam.cast_rays(np.zeros((0, 2))) is None
    # calc_line_segments: three cameras named like the committed tabular detections (img2 has none)
    transforms = []
    for k in range(3):
        T = T0.copy()
        T[:3, 3] += np.array([0.7 * k, -0.4 * k, 0.1 * k])
        transforms.append(T)
    names = ["img0.png", "img1.png", "img2.png"]
    cams = PhotogrammetryCameraSet(cameras=[PhotogrammetryCamera(nm, T, f, cx, cy, w, h) for nm, T in zip(names, transforms)])
    detector = TabularRectangleSegmentor(DATA / "cols", IMAGE_SHAPE, split_bbox=False)
    out["seg__transforms"] = np.array(transforms)
    seg = cams.calc_line_segments(detector, ray_length_local=25.0)
    out.update({f"seg__{k}": np.asarray(v) for k, v in seg.items()})
    dirs = seg["ray_ends"] - seg["ray_starts"]
    ang = np.arccos(np.abs(dirs[:, 2] / np.linalg.norm(dirs, axis=1)))
    limit = float(np.sort(ang)[len(ang) // 2]) + 1e-9   # keeps about half of the rays
    out["seg__angle_limit"] = np.float64(limit)
    seg2 = cams.calc_line_segments(detector, ray_length_local=25.0, limit_angle_from_vert=limit)
    out.update({f"seg__lim__{k}": np.asarray(v) for k, v in seg2.items()})
    with tempfile.TemporaryDirectory() as tmp:
        p = cams.calc_line_segments(detector, ray_length_local=25.0, out_dir=tmp)
        assert Path(p).name == "line_segments.npz"

    # clip: survey rays (from the cameras, unit directions) against a tilted ceiling and a bumpy floor of a few triangles each
    full = synthetic.detection_survey(n_objects=12, n_cameras=10, seed=5)
    origins = full["cameras"][full["ray_IDs"]]
    directions = full["ray_ends"] - origins
    directions = directions / np.linalg.norm(directions, axis=1, keepdims=True)
    for tag, fn in (("ceil", lambda x, y: 30.0 + 0.02 * x - 0.01 * y), ("floor", lambda x, y: 2.0 * np.sin(x / 40.0) - 1.0)):
        pts, faces = synthetic.boundary_grid(7, fn)
        hit64, t64, p64, margin = ray_standin.clip_rays_np(origins, directions, pts, faces)
        hitld, tld, pld, _ = ray_standin.clip_rays_np(origins, directions, pts, faces, dtype=np.longdouble)
        assert np.array_equal(hit64, hitld) and hit64.all()
        assert float(np.min(margin)) > 1e-6, "a fixture ray is aimed at a shared edge or vertex"
        out.update({f"clip__{tag}__points": pts, f"clip__{tag}__faces": faces,
                    f"clip__{tag}__e_t": np.float64(np.max(np.abs(t64.astype(np.longdouble) - tld))),
                    f"clip__{tag}__e_p": np.float64(np.max(np.abs(p64.astype(np.longdouble) - pld)))})
        out[f"clip__{tag}__t_hi"], out[f"clip__{tag}__t_lo"] = hi_lo(tld)
        out[f"clip__{tag}__p_hi"], out[f"clip__{tag}__p_lo"] = hi_lo(pld)
        print(f"clip {tag}: {len(faces)} triangles, e_t {out[f'clip__{tag}__e_t']:.3g}, e_p {out[f'clip__{tag}__e_p']:.3g}, "
              f"min margin {float(np.min(margin)):.3g}")
    out["clip__origins"], out["clip__directions"] = origins, directions
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({len(out)} arrays, {OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
