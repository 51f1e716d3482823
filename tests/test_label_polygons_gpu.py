"""gr_polygon_class_weights / label_polygons on the device against the exact oracle's committed answers
(tests/golden/label_polygons.npz, made by tests/golden/make_golden_label_polygons.py) and against oracle-free invariants at the
size of the C2 mesh.

Bounds: within (sjoin) mode decides with integers, so unit weights on the integer scene are BIT-equal to the oracle and every
other scene is within rtol 1e-12 (the order of the f64 sum is all that differs: the project's standing bound for f64 atomics);
overlay mode is within 4 e_ref n_pairs + 1e-12 sum per (polygon, class), e_ref being the stand-in's measured area error against
the exact areas (stored in the npz), and bit-equal on the integer scene wherever the exact sum is a double."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import synthetic  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons  # noqa: E402

pytestmark = pytest.mark.gpu

import polygon_standin as ps  # noqa: E402
from polygon_standin import SCENES, load_scene  # noqa: E402


def device_weights(d, within, mesh=None):
    mesh = mesh or TexturedPhotogrammetryMesh((d["points"], d["faces"]), log_level="ERROR")
    w = mesh.label_polygon_weights(d["face_labels"], d["polygons"], face_weighting=d["weighting"], sjoin_overlay=within,
                                   points_in_polygon_CRS=d["points"])
    return w, mesh


def overlay_tolerance(d):
    return ps.overlay_tolerance(d["e_ref"], d["pairs_per_polygon"], d["weights_overlay"])


def report(name, what, got, want, tol=None):
    err = np.abs(got - want)
    line = f"[label_polygons] {name} {what}: max |diff| {err.max():.3e}"
    if tol is not None:
        line += f", max diff / tolerance {np.max(err / np.maximum(tol, 1e-300)):.3e}"
    print(line)


def test_within_decisions_on_the_integer_scene_are_bit_equal():
    d = load_scene("integer")
    got, mesh = device_weights(d, True)
    report("integer", "within", got, d["weights_within"])
    assert np.array_equal(got, d["weights_within"])
    assert mesh.last_polygon_stats["pairs_tested"] == int(d["pairs_per_polygon"].sum())
    assert mesh.last_polygon_stats["largest_ring"] == 4


@pytest.mark.parametrize("name", SCENES)
def test_within_weights_match_the_exact_oracle(name):
    d = load_scene(name)
    got, mesh = device_weights(d, True)
    report(name, "within", got, d["weights_within"])
    np.testing.assert_allclose(got, d["weights_within"], rtol=1e-12, atol=0)
    assert mesh.last_polygon_stats["pairs_tested"] == int(d["pairs_per_polygon"].sum())


@pytest.mark.parametrize("name", SCENES)
def test_overlay_sums_match_the_exact_oracle(name):
    d = load_scene(name)
    got, _ = device_weights(d, False)
    tol = overlay_tolerance(d)
    report(name, "overlay", got, d["weights_overlay"], tol)
    assert np.all(np.abs(got - d["weights_overlay"]) <= tol)
    if name == "integer":
        rep = d["overlay_representable"]
        assert rep.any() and np.array_equal(got[rep], d["weights_overlay"][rep])


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("within", [True, False])
def test_labels_match_the_exact_oracle(name, within):
    d = load_scene(name)
    mesh = TexturedPhotogrammetryMesh((d["points"], d["faces"]), log_level="ERROR")
    got = np.array(mesh.label_polygons(d["face_labels"], d["polygons"], face_weighting=d["weighting"], sjoin_overlay=within,
                                       return_class_labels=False, points_in_polygon_CRS=d["points"]), dtype=np.float64)
    want_w = d["weights_within" if within else "weights_overlay"]
    want = d["labels_within" if within else "labels_overlay"]
    tol = 1e-12 * np.abs(want_w) if within else overlay_tolerance(d)
    compared = 0
    for p in range(len(want)):
        order = np.argsort(-want_w[p], kind="stable")
        top, second = want_w[p, order[0]], want_w[p, order[1]]
        if top != 0 and not top - second > 2 * max(tol[p, order[0]], tol[p, order[1]]):
            continue   # the tolerance could flip this label
        compared += 1
        assert (np.isnan(want[p]) and np.isnan(got[p])) or got[p] == want[p], (p, got[p], want[p])
    assert compared == len(want)   # no polygon of a committed scene is left out


def test_device_tensor_inputs_give_the_same_result():
    import torch

    d = load_scene("tin")
    want, mesh = device_weights(d, True)
    labels_t = torch.as_tensor(d["face_labels"]).to(mesh.backend.device)
    weighting_t = torch.as_tensor(d["weighting"]).to(mesh.backend.device)
    for within, ref in ((True, want), (False, device_weights(d, False, mesh)[0])):
        got = mesh.label_polygon_weights(labels_t, d["polygons"], face_weighting=weighting_t, sjoin_overlay=within,
                                         points_in_polygon_CRS=d["points"])
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
    # exactly summable inputs: bit-equal
    d = load_scene("integer")
    want, mesh = device_weights(d, True)
    got = mesh.label_polygon_weights(torch.as_tensor(d["face_labels"]).to(mesh.backend.device), d["polygons"],
                                     points_in_polygon_CRS=d["points"])
    assert np.array_equal(got, want)


# -- oracle-free invariants at scale ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2():
    points, faces = synthetic.terrain_mesh()
    mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR")
    rng = np.random.default_rng(21)
    labels = rng.integers(0, 4, len(faces)).astype(np.float64)
    labels[rng.random(len(faces)) < 0.05] = np.nan
    weighting = rng.uniform(0.1, 1.0, len(faces))
    lo, hi = points[:, :2].min() - 1.0, points[:, :2].max() + 1.0
    edges = np.linspace(lo, hi, 25)
    tiles = [np.array([[edges[i], edges[j]], [edges[i + 1], edges[j]], [edges[i + 1], edges[j + 1]], [edges[i], edges[j + 1]]])
             for j in range(24) for i in range(24)]
    return mesh, points, faces, labels, weighting, PlanarPolygons.from_sequence(tiles)


def test_tiling_squares_partition_the_weighted_area(c2):
    """Squares that tile the footprint cut every face into pieces that add up to the face: per class, the overlay weights
    summed over the polygons equal the sum of area x weight over the faces (the snapped area, the weight of rule 4)."""
    from geograypher_amd.utils.geometric import snap_to_grid

    mesh, points, faces, labels, weighting, tiles = c2
    overlay = mesh.label_polygon_weights(labels, tiles, face_weighting=weighting, sjoin_overlay=False, points_in_polygon_CRS=points)
    stats = dict(mesh.last_polygon_stats)
    q = snap_to_grid(points[:, :2])[faces].astype(np.float64)   # exact: |q| < 2^53
    area = np.abs((q[:, 1, 0] - q[:, 0, 0]) * (q[:, 2, 1] - q[:, 0, 1]) - (q[:, 1, 1] - q[:, 0, 1]) * (q[:, 2, 0] - q[:, 0, 0])) / 2e12
    A, B, C = (points[faces[:, k]] for k in range(3))
    n = np.cross(B - A, C - A)
    ratio = np.linalg.norm(n, axis=1) / np.abs(n[:, 2])
    for c in range(4):
        want = float(np.sum((area * ratio * weighting)[labels == c]))
        got = float(overlay[:, c].sum())
        print(f"[label_polygons] C2 tiling class {c}: got {got:.15e} want {want:.15e} rel {abs(got - want) / want:.3e}")
        assert abs(got - want) <= 1e-12 * want
    assert stats["pairs_tested"] >= int(np.isfinite(labels).sum()) and stats["largest_ring"] == 4
    # within never counts more than overlay
    within = mesh.label_polygon_weights(labels, tiles, face_weighting=weighting, sjoin_overlay=True, points_in_polygon_CRS=points)
    assert np.all(within <= overlay * (1 + 1e-12))
    assert np.all(within > 0) and np.any(within < overlay * (1 - 1e-6))   # faces on tile borders count for overlay only


def test_within_decisions_are_the_same_across_runs(c2):
    mesh, points, faces, labels, _weighting, tiles = c2
    runs = []
    for _ in range(2):
        w = mesh.label_polygon_weights(labels, tiles, sjoin_overlay=True, points_in_polygon_CRS=points)
        runs.append((w, mesh.last_polygon_stats["pairs_contributing"], mesh.last_polygon_stats["pairs_tested"]))
    assert runs[0][1:] == runs[1][1:]                        # the same pairs decided the same way
    np.testing.assert_allclose(runs[0][0], runs[1][0], rtol=1e-12, atol=0)
    # and exactly summable inputs repeat bit for bit
    d = load_scene("integer")
    a, m = device_weights(d, True)
    b, _ = device_weights(d, True, m)
    assert np.array_equal(a, b)
