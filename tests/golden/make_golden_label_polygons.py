#!/usr/bin/env python3
"""Writes tests/golden/label_polygons.npz: small label_polygons scenes with the answers of THIS repository's exact oracle
(tests/polygon_standin.py: Python integers and fractions.Fraction on the snapped coordinates).  They do NOT come from the
reference: shapely and geopandas are not available where this project is built, and the reference method does not run at the
pinned snapshot (get_faces_2d_gdf calls an undefined get_vertices_in_CRS, meshes.py:873).

Scenes (every array of scene S is stored as "S/<name>"):
  tin      a jittered heightfield TIN, random classes with unlabelled faces, random face weights: a convex, a non-convex, a
           holed and a two-part polygon, two polygons that overlap each other, one no face touches, one whose faces all have
           weight 0
  folded   two sheets over the same ground (faces overlap in 2D)
  integer  whole-metre right triangles, flat, unit weights, in contact with the rings: a ring edge along face edges, a polygon
           equal to one face, a ring edge from a face vertex through its interior, a hole wholly inside a face, ring vertices
           on face edges

Stored per scene: the inputs (points, faces, face_labels, face_weighting or an empty array, rings as one (N, 2) array with
ring_offsets / ring_polygon / ring_is_hole, n_polygons), the exact (P, C) weights of both modes, the exact labels of both
modes, and pairs_per_polygon (the (face, polygon) pairs whose boxes overlap).  Global: e_ref, the largest |area| error in square
metres of the float64 stand-in against the exact intersection area over all pairs of all scenes (MEASURED here, with the
stand-in on the CPU).  The maker asserts what the GPU test relies on: the stand-in decides containment like the oracle on every
pair, every polygon's label is decided by a margin beyond the comparison tolerance (none is left out), and on the integer scene
the stand-in is bit-equal to the oracle wherever the exact sum is a double.

    python tests/golden/make_golden_label_polygons.py
"""
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import polygon_standin as ps  # noqa: E402
from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import synthetic  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons  # noqa: E402

OUT = Path(__file__).resolve().parent / "label_polygons.npz"


def labels_of(weights):
    out = np.full(weights.shape[0], np.nan)
    if weights.shape[1]:
        best = np.argmax(weights, axis=1)
        has = weights[np.arange(len(best)), best] != 0
        out[has] = best[has]
    return out


def undecided(want, tol):
    """Polygons whose label the tolerance could flip: a positive top whose lead over the runner-up is within 2 tol."""
    left_out = []
    for p in range(want.shape[0]):
        order = np.argsort(-want[p], kind="stable")
        top = want[p, order[0]]
        if top == 0:
            continue
        second = want[p, order[1]] if want.shape[1] > 1 else 0.0
        if not top - second > 2 * max(tol[p, order[0]], tol[p, order[1]] if want.shape[1] > 1 else 0.0):
            left_out.append(p)
    return left_out


def circle(cx, cy, r, n, phase=0.0):
    a = phase + 2 * np.pi * np.arange(n) / n
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1)


def scene_tin():
    rng = np.random.default_rng(5)
    points, faces = synthetic.heightfield_mesh(13, 12.0, lambda x, y: 0.6 * np.sin(0.7 * x) + 0.4 * np.cos(0.9 * y), jitter=0.3,
                                               seed=3)
    labels = rng.integers(0, 4, len(faces)).astype(np.float64)
    labels[rng.random(len(faces)) < 0.1] = np.nan
    weighting = rng.uniform(0.05, 1.0, len(faces))
    u_shape = np.array([[-5.5, -5.5], [-1.5, -5.5], [-1.5, -1.0], [-2.8, -1.0], [-2.8, -4.2], [-4.1, -4.2], [-4.1, -1.0],
                        [-5.5, -1.0]])
    polys = [
        circle(3.0, 3.0, 2.2, 7),                                                   # convex
        u_shape,                                                                    # non-convex
        [circle(-3.0, 3.0, 2.5, 16), circle(-3.2, 3.1, 1.0, 9)[::-1]],              # a hole
        circle(2.5, -3.0, 2.0, 12), circle(3.6, -2.4, 1.7, 10),                     # overlap each other
        circle(40.0, 40.0, 2.0, 8),                                                 # no face touches it
        np.array([[4.6, 4.6], [5.9, 4.6], [5.9, 5.9], [4.6, 5.9]]),                 # faces of weight 0 only
    ]
    rings, rows, holes = [], [], []
    for p, item in enumerate(polys):
        for k, ring in enumerate(item if isinstance(item, list) else [item]):
            rings.append(ring); rows.append(p); holes.append(k > 0)
    # a two-part polygon: row 7
    for ring in (circle(-0.3, 0.2, 1.1, 6), circle(0.5, 4.9, 0.9, 5)):
        rings.append(ring); rows.append(7); holes.append(False)
    # the faces that can reach the weight-0 square get weight 0
    xy = points[faces][:, :, :2]
    near = (xy[:, :, 0].max(1) >= 4.6) & (xy[:, :, 1].max(1) >= 4.6)
    weighting[near] = 0.0
    return points, faces, labels, weighting, PlanarPolygons(rings, rows, holes)


def scene_folded():
    rng = np.random.default_rng(9)
    pa, fa = synthetic.heightfield_mesh(7, 6.0, lambda x, y: 0.2 * x, jitter=0.25, seed=1)
    pb, fb = synthetic.heightfield_mesh(6, 6.0, lambda x, y: 2.0 + 0.5 * y, jitter=0.2, seed=2)
    points = np.concatenate([pa, pb + np.array([0.37, -0.21, 0.0])])
    faces = np.concatenate([fa, fb + len(pa)])
    labels = rng.integers(0, 3, len(faces)).astype(np.float64)
    polys = PlanarPolygons.from_sequence([circle(0.0, 0.0, 2.4, 20, 0.1),
                                          np.array([[-2.9, -2.9], [0.4, -2.6], [-0.8, -0.5], [0.9, 1.9], [-2.7, 1.2]])])
    return points, faces, labels, None, polys


def scene_integer():
    lin = np.arange(7, dtype=np.float64)
    xx, yy = np.meshgrid(lin, lin)
    points = np.stack([xx.ravel(), yy.ravel(), np.zeros(49)], axis=1)
    faces = synthetic.grid_faces(7, 7)
    cell = np.arange(len(faces)) // 2                     # both faces of a grid cell share a class: (row + 2 column) mod 3
    labels = ((cell // 6 + 2 * (cell % 6)) % 3).astype(np.float64)
    polys = PlanarPolygons.from_sequence([
        np.array([[1.0, 1.0], [3.0, 1.0], [3.0, 3.0], [1.0, 3.0]]),                 # ring edges along face edges
        np.array([[4.0, 0.0], [5.0, 0.0], [5.0, 1.0]]),                             # equal to one face
        np.array([[4.0, 4.0], [6.0, 5.0], [6.0, 6.0], [4.0, 6.0]]),                 # an edge from a face vertex through its interior
        [np.array([[0.0, 3.0], [2.0, 3.0], [2.0, 5.0], [0.0, 5.0]]),               # a hole wholly inside the face (0,3) (1,3) (1,4)
         np.array([[0.5, 3.125], [0.75, 3.125], [0.75, 3.25], [0.5, 3.25]])],
        np.array([[3.0, 1.5], [3.5, 1.0], [4.0, 1.5], [3.5, 2.0]]),                 # ring vertices on face edges
    ])
    return points, faces, labels, None, polys


def main():
    out = {}
    area_errors = []
    per_scene = {}
    for name, make in (("tin", scene_tin), ("folded", scene_folded), ("integer", scene_integer)):
        points, faces, labels, weighting, polys = make()
        backend = ps.StandInBackend()
        mesh = TexturedPhotogrammetryMesh((points, faces), backend=backend, log_level="ERROR")
        got = {}
        for within in (True, False):
            got[within] = mesh.label_polygon_weights(labels, polys, face_weighting=weighting, sjoin_overlay=within,
                                                     points_in_polygon_CRS=points)
        call = backend.last
        tri, cls, wgt, table, C = call["tri"], call["face_class"], call["face_weight"], call["table"], call["n_classes"]
        pairs = ps.exact_pairs(tri, cls, table)
        s_within = ps.standin_pairs(tri, cls, table, True)
        s_overlay = ps.standin_pairs(tri, cls, table, False)
        assert pairs.keys() == s_within.keys() == s_overlay.keys()
        assert all(pairs[k][0] == s_within[k] for k in pairs), f"{name}: the stand-in's containment differs from the oracle"
        area_errors += [abs(Fraction(s_overlay[k]) - pairs[k][1] / (2 * ps.GRID2_PER_M2)) for k in pairs]
        want = {w: ps.exact_class_weights(tri, cls, wgt, table, C, w, pairs) for w in (True, False)}
        n_pairs = np.bincount([p for _f, p in pairs], minlength=len(polys)).astype(np.int64)
        per_scene[name] = (got, want, n_pairs, pairs, cls, wgt, C)
        ring_xy = np.concatenate(polys.rings)
        out.update({
            f"{name}/points": points, f"{name}/faces": faces, f"{name}/face_labels": labels,
            f"{name}/face_weighting": np.zeros(0) if weighting is None else weighting,
            f"{name}/rings": ring_xy, f"{name}/ring_offsets": np.cumsum([0] + [len(r) for r in polys.rings]),
            f"{name}/ring_polygon": polys.ring_polygon, f"{name}/ring_is_hole": polys.ring_is_hole,
            f"{name}/n_polygons": np.int64(len(polys)),
            f"{name}/weights_within": want[True], f"{name}/weights_overlay": want[False],
            f"{name}/labels_within": labels_of(want[True]), f"{name}/labels_overlay": labels_of(want[False]),
            f"{name}/pairs_per_polygon": n_pairs,
        })
    e_ref = float(max(area_errors))
    out["e_ref"] = np.float64(e_ref)
    for name, (got, want, n_pairs, pairs, cls, wgt, C) in per_scene.items():
        # within: only the order of the sum differs from the oracle
        np.testing.assert_allclose(got[True], want[True], rtol=1e-12, atol=0)
        tol = ps.overlay_tolerance(e_ref, n_pairs, want[False])
        assert np.all(np.abs(got[False] - want[False]) <= tol), f"{name}: the stand-in misses the overlay bound"
        assert undecided(want[False], tol) == [], f"{name}: overlay labels within the tolerance: {undecided(want[False], tol)}"
        assert undecided(want[True], 1e-12 * np.abs(want[True])) == [], f"{name}: within labels within the tolerance"
        for w in (True, False):
            assert np.array_equal(labels_of(got[w]), labels_of(want[w]), equal_nan=True)
        assert np.all(got[True] <= got[False] + tol)
    # the integer scene: bit-equal wherever the exact sum is a double
    got, want, n_pairs, pairs, cls, wgt, C = per_scene["integer"]
    assert np.array_equal(got[True], want[True])
    exact_sums = [[Fraction(0)] * C for _ in range(len(n_pairs))]
    for (f, p), (_c, a2, _o) in pairs.items():
        exact_sums[p][int(cls[f])] += a2 / (2 * ps.GRID2_PER_M2) * Fraction(float(wgt[f]))
    representable = np.array([[Fraction(float(v)) == v for v in row] for row in exact_sums])
    assert representable.any()
    assert np.array_equal(got[False][representable], want[False][representable])
    out["integer/overlay_representable"] = representable
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: e_ref = {e_ref:.3e} m^2; pairs " + ", ".join(f"{k} {len(v[3])}" for k, v in per_scene.items()) +
          f"; integer scene: {int(representable.sum())} of {representable.size} overlay sums are doubles")


if __name__ == "__main__":
    main()
