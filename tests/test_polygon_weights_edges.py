"""gr_polygon_class_weights at its edges, on raw snapped tables through `HipRaster.polygon_class_weights`, against the exact oracle
of tests/polygon_standin.py (rational clipping; containment as area(T n P) == area(T), not the device's method) on scenes generated
there and checked on the host by tests/test_label_polygons_host.py.

What each scene can tell apart:
* lattice "small" (metres, determinants below 2^53) and "large" (|q| up to 1e12 < 2^40, every triangle's twice-area >= 2^64), one
  class per face (C = F = 257, unit weights): weights[p, f] is the single contribution of pair (f, p), so the device is compared
  pair by pair -- hundreds of contained, cut and touching pairs, holed and two-part polygons -- and every wave runs its leader
  loop over 64 classes.  The large scale fails a kernel whose determinants wrap to 64 bits (shown on the host with
  `within_wrapped64`), whose 128-bit-to-double conversion is wrong above 2^64, or whose 3 x coordinate products overflow.
* wave scenes: face counts around the wave and the workgroup, dead lanes, 1 / 3 / 70 classes, both windings, collapsed faces,
  classes outside [0, C), zero weights, a polygon without rings, one whose rings are all shorter than 3 vertices, ring rows whose
  polygon is outside [0, P), and a polygon only one wave's faces meet.

Bounds.  Within mode decides with integers: the set of contributing pairs equals the oracle's, values within rtol 1e-12 of the
exact ones (the project's standing bound for sums whose order varies), bit-equal where one pair fills a cell and the determinant is
below 2^53.  Overlay: 4 x e_scene per pair + 1e-12 |exact|, e_scene being the stand-in's own largest area error on that scene,
measured on the host against the exact areas; weights are at most 1, so a pair's weighted error is no larger than its area error."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import polygon_standin as ps  # noqa: E402

pytestmark = pytest.mark.gpu

WAVE_FACES = (1, 63, 64, 65, 255, 256, 257, 513)
WAVE_CLASSES = (1, 3, 70)


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def device(hip, tri, cls, weight, table, n_classes, within):
    weights, stats = hip.polygon_class_weights(tri, cls, weight, *table, n_classes=n_classes, within=within)
    return _np(weights), _np(stats)


def report(name, what, got, want, tol):
    err = np.abs(got - want)
    print(f"[polygon_weights] {name} {what}: max |diff| {err.max():.3e}, max diff / tolerance "
          f"{np.max(err / np.maximum(tol, 1e-300)):.3e}")


def answers(case, cls, weight, n_classes, within):
    """(exact weights, tolerance, stand-in weights, stand-in stats) of a cached case under a class and weight assignment."""
    tri, table = case["tri"], case["table"]
    exact = ps.select_pairs(case["exact"], cls, n_classes)
    want = ps.exact_class_weights(tri, cls, weight, table, n_classes, within, exact)
    if within:
        tol = 1e-12 * np.abs(want)
    else:
        per_polygon = np.bincount([p for _, p in exact], minlength=len(table[4]))
        tol = ps.overlay_tolerance(case["e_scene"], per_polygon, want)
    standin, stats = ps.polygon_class_weights_np(tri, cls, weight, table, n_classes, within, case["within" if within else "overlay"])
    return want, tol, standin, stats


def check(name, what, got, got_stats, want, tol, stats):
    report(name, what, got, want, tol)
    assert np.all(np.abs(got - want) <= tol)
    assert got_stats[:3].tolist() == stats[:3].tolist()    # pairs tested, pairs contributing, largest ring


# -- per-pair exposure -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["small", "large"])
def exposed(request):
    """A lattice scene with one class per face and unit weights, and its answers in both modes."""
    case = ps.lattice_case(request.param)
    n = len(case["tri"])
    cls, weight = np.arange(n, dtype=np.int32), np.ones(n)
    return request.param, case, cls, weight, {w: answers(case, cls, weight, n, w) for w in (True, False)}


def test_within_decides_every_pair_like_the_exact_oracle(hip, exposed):
    name, case, cls, weight, ans = exposed
    want, tol, _standin, stats = ans[True]
    got, got_stats = device(hip, case["tri"], cls, weight, case["table"], len(cls), True)
    contained = np.zeros(want.shape, dtype=bool)
    for (f, p), (inside, _a2, _o) in case["exact"].items():
        contained[p, f] = inside
    wrong = np.argwhere((got != 0.0) != contained)
    print(f"[polygon_weights] lattice {name} within: {int(contained.sum())} of {len(case['exact'])} pairs contained, "
          f"{len(wrong)} decided differently")
    assert wrong.tolist() == []
    check(f"lattice {name}", "within", got, got_stats, want, tol, stats)
    if name == "small":                                    # determinants below 2^53: one conversion, one division, one term
        assert np.array_equal(got, want)


def test_overlay_clips_every_pair_like_the_exact_oracle(hip, exposed):
    name, case, cls, weight, ans = exposed
    want, _tol, standin, stats = ans[False]
    tol = 4.0 * case["e_scene"] + 1e-12 * np.abs(want)    # per pair: every cell holds at most one
    got, got_stats = device(hip, case["tri"], cls, weight, case["table"], len(cls), False)
    pairs = np.zeros(want.shape, dtype=bool)
    for f, p in case["exact"]:
        pairs[p, f] = True
    print(f"[polygon_weights] lattice {name} overlay: e_scene {case['e_scene']:.3e} m^2, "
          f"{int(np.sum(got[pairs] == standin[pairs]))} of {int(pairs.sum())} pairs bit-equal to the stand-in")
    assert np.all(got[~pairs] == 0.0)
    check(f"lattice {name}", "overlay", got, got_stats, want, tol, stats)


# -- the wave and workgroup structure, the raw-table contract ---------------------------------------------------------------------
@pytest.mark.parametrize("within", [True, False], ids=["within", "overlay"])
@pytest.mark.parametrize("n_classes", WAVE_CLASSES)
@pytest.mark.parametrize("n_faces", WAVE_FACES)
def test_face_counts_classes_and_odd_tables(hip, n_faces, n_classes, within):
    tri, cls, weight, table, info = ps.wave_scene(n_faces, n_classes)
    want, tol, _standin, stats = answers(ps.wave_case(n_faces), cls, weight, n_classes, within)
    got, got_stats = device(hip, tri, cls, weight, table, n_classes, within)
    assert got.shape == (ps.WAVE_POLYGONS, n_classes)
    check(f"wave F={n_faces} C={n_classes}", "within" if within else "overlay", got, got_stats, want, tol, stats)
    assert np.all(got[info["no_usable_rings"]] == 0.0)     # the row without rings, the row of rings shorter than 3 vertices
    if info["idle_class"] is not None:
        assert np.all(got[:, info["idle_class"]] == 0.0)   # carried by collapsed faces only
    if within:
        assert np.array_equal(got != 0.0, want != 0.0)


# -- order independence ---------------------------------------------------------------------------------------------------------
def reversed_polygons(table):
    """The table with the polygons in reverse order (row p -> P - 1 - p): the runs of equal ring_polygon are taken in reverse, each
    with its rings in their order, so every polygon's rings stay consecutive and the rows outside [0, P) stay between valid runs."""
    rv, off, poly, hole, boxes = table
    P = len(boxes)
    runs, start = [], 0
    for r in range(1, len(poly) + 1):
        if r == len(poly) or poly[r] != poly[start]:
            runs.append(range(start, r))
            start = r
    rows = [(int(P - 1 - poly[r]) if 0 <= poly[r] < P else int(poly[r]), [tuple(v) for v in rv[off[r]:off[r + 1]].tolist()], hole[r])
            for run in reversed(runs) for r in run]
    out = ps.make_table(rows, P)
    assert np.array_equal(out[4], boxes[::-1])
    return out


@pytest.fixture(scope="module", params=["lattice", "wave"])
def ordered(request):
    """(name, case, classes, weights, n_classes): the small lattice scene in 3 classes, and the 257-face wave scene in 70."""
    if request.param == "lattice":
        case = ps.lattice_case("small")
        n = len(case["tri"])
        return request.param, case, (np.arange(n) % 3).astype(np.int32), np.linspace(0.25, 1.0, n), 3
    _tri, cls, weight, _table, _info = ps.wave_scene(257, 70)
    return request.param, ps.wave_case(257), cls, weight, 70


@pytest.mark.parametrize("within", [True, False], ids=["within", "overlay"])
def test_face_and_polygon_order_do_not_matter(hip, ordered, within):
    name, case, cls, weight, n_classes = ordered
    tri, table = case["tri"], case["table"]
    want, tol, _standin, stats = answers(case, cls, weight, n_classes, within)
    what = "within" if within else "overlay"
    base, base_stats = device(hip, tri, cls, weight, table, n_classes, within)
    check(f"order {name}", what, base, base_stats, want, tol, stats)
    order = np.random.default_rng(5).permutation(len(tri))
    shuffled, shuffled_stats = device(hip, tri[order], cls[order], weight[order], table, n_classes, within)
    check(f"order {name}, faces permuted", what, shuffled, shuffled_stats, want, tol, stats)
    flipped, flipped_stats = device(hip, tri, cls, weight, reversed_polygons(table), n_classes, within)
    check(f"order {name}, polygons reversed", what, flipped[::-1], flipped_stats, want, tol, stats)
    if within:                                             # the same pairs decided the same way
        assert np.array_equal(shuffled != 0.0, base != 0.0) and np.array_equal(flipped[::-1] != 0.0, base != 0.0)


def test_one_class_per_face_survives_a_face_permutation_bit_for_bit(hip):
    """With one class per face every cell is one pair's own value: a permutation of the faces moves pairs to other lanes, waves and
    workgroups and must change nothing at all."""
    case = ps.lattice_case("large")
    n = len(case["tri"])
    cls, weight = np.arange(n, dtype=np.int32), np.ones(n)
    order = np.random.default_rng(6).permutation(n)
    for within in (True, False):
        base, base_stats = device(hip, case["tri"], cls, weight, case["table"], n, within)
        got, got_stats = device(hip, case["tri"][order], cls[order], weight[order], case["table"], n, within)
        assert np.array_equal(got, base) and np.array_equal(got_stats, base_stats)


# -- written by the call ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("empty", ["F", "R", "P", "C"])
def test_outputs_are_written_when_a_size_is_zero(hip, empty):
    """`weights` and `stats` are written by the call also when it has nothing to do: caller-made buffers full of NaN and -1 come
    back as zeros, and nothing behind weights' P x C elements is touched."""
    import torch

    from geograypher_amd import _hip

    tri, cls, weight, table, _info = ps.wave_scene(63, 3)
    dev = hip.device
    t = [torch.as_tensor(np.ascontiguousarray(a)).to(dev) for a in (tri, cls, weight, table[0], table[1], table[2], table[3], table[4])]
    assert [a.dtype for a in t] == [torch.int64, torch.int32, torch.float64, torch.int64, torch.int64, torch.int32, torch.int32,
                                    torch.int64]
    F, R, P, C = (0 if empty == k else v for k, v in zip("FRPC", (len(tri), len(table[2]), len(table[4]), 3)))
    guard = 8
    weights = torch.full((P * C + guard,), float("nan"), dtype=torch.float64, device=dev)
    stats = torch.full((_hip.GR_POLY_STAT_WORDS,), -1, dtype=torch.int64, device=dev)
    hip._call("gr_polygon_class_weights", t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), F, t[3].data_ptr(), int(t[3].shape[0]),
              t[4].data_ptr(), t[5].data_ptr(), t[6].data_ptr(), R, t[7].data_ptr(), P, _hip.GR_POLY_WITHIN, C, weights.data_ptr(),
              stats.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    weights, stats = weights.cpu().numpy(), stats.cpu().numpy()
    assert np.all(weights[:P * C] == 0.0) and np.all(np.isnan(weights[P * C:]))
    assert stats.tolist() == [0] * _hip.GR_POLY_STAT_WORDS
