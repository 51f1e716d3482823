"""label_polygons on the host (no GPU): argument errors, label masking, weighting, ties, empty polygons, label strings, the
chunked class, `PlanarPolygons`, the C ABI tables -- driven through `polygon_standin.StandInBackend` -- and the stand-in itself
against the exact oracle on the committed scenes (tests/golden/label_polygons.npz) and on the generated lattice and wave scenes
that tests/test_polygon_weights_edges.py runs on the device."""
import re
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))

import polygon_standin as ps  # noqa: E402
from geograypher_amd import _hip  # noqa: E402
from geograypher_amd.meshes.derived_meshes import TexturedPhotogrammetryMeshChunked  # noqa: E402
from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import synthetic  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons  # noqa: E402

from polygon_standin import GOLDEN, SCENES, load_scene  # noqa: E402


def flat_grid(n=5):
    """(n - 1)^2 unit cells on whole metres, z = 0: every face has area 1/2 and a 3D / 2D ratio of exactly 1."""
    lin = np.arange(n, dtype=np.float64)
    xx, yy = np.meshgrid(lin, lin)
    return np.stack([xx.ravel(), yy.ravel(), np.zeros(n * n)], axis=1), synthetic.grid_faces(n, n)


def make_mesh(points, faces, cls=TexturedPhotogrammetryMesh, **kw):
    return cls((points, faces), backend=ps.StandInBackend(), log_level="ERROR", **kw)


def square(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)


# -- arguments ---------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    points, faces = flat_grid()
    mesh = make_mesh(points, faces)
    labels = np.zeros(len(faces))
    polys = [square(0, 0, 2, 2)]
    with pytest.raises(ValueError, match="one-dimensional"):
        mesh.label_polygons(np.zeros((len(faces), 2)), polys, points_in_polygon_CRS=points)
    with pytest.raises(ValueError, match="one-dimensional"):
        mesh.label_polygons(labels, polys, face_weighting=np.ones((len(faces), 2)), points_in_polygon_CRS=points)
    with pytest.raises(NotImplementedError, match="points_in_polygon_CRS"):
        mesh.label_polygons(labels, polys)
    with pytest.raises(NotImplementedError, match="geopandas"):
        mesh.label_polygons(labels, "crowns.gpkg", points_in_polygon_CRS=points)
    with pytest.raises(ValueError, match="whole numbers"):
        mesh.label_polygons(labels + 0.5, polys, points_in_polygon_CRS=points)
    with pytest.raises(ValueError, match="whole numbers"):
        mesh.label_polygons(labels - 1, polys, points_in_polygon_CRS=points)
    with pytest.raises(ValueError, match="face labels"):
        mesh.label_polygons(labels[:-1], polys, points_in_polygon_CRS=points)
    with pytest.raises(ValueError, match="points_in_polygon_CRS must be"):
        mesh.label_polygons(labels, polys, points_in_polygon_CRS=points[:-1])
    far = points.copy()
    far[0, 0] = 3e6   # 3000 km from the rest: beyond 2^40 grid steps behind any common origin
    with pytest.raises(ValueError, match="2\\^40"):
        mesh.label_polygons(labels, polys, points_in_polygon_CRS=far)
    # a column vector is squeezed, as the reference does
    assert mesh.label_polygons(labels[:, None], polys, points_in_polygon_CRS=points) == [0.0]


def test_planar_polygons_validation():
    closed = np.array([[0, 0], [2, 0], [2, 2], [0, 2], [0, 0]], dtype=np.float64)
    pp = PlanarPolygons.from_sequence([closed, [square(5, 5, 9, 9), square(6, 6, 7, 7)[::-1]]])
    assert len(pp) == 2 and [len(r) for r in pp.rings] == [4, 4, 4]          # the closing vertex is dropped
    assert list(pp.ring_polygon) == [0, 1, 1] and list(pp.ring_is_hole) == [False, False, True]
    for ring in pp.rings:   # every ring counter-clockwise, whatever it came as
        assert np.sum(ring[:, 0] * np.roll(ring[:, 1], -1) - np.roll(ring[:, 0], -1) * ring[:, 1]) > 0
    clockwise = PlanarPolygons.from_sequence([square(0, 0, 2, 2)[::-1]])
    assert np.array_equal(clockwise.rings[0], square(0, 0, 2, 2)[::-1][::-1])
    with pytest.raises(ValueError, match="fewer than 3"):
        PlanarPolygons.from_sequence([np.array([[0, 0], [1, 1], [0, 0.0]])])
    with pytest.raises(ValueError, match="non-finite"):
        PlanarPolygons.from_sequence([np.array([[0, 0], [1, np.nan], [0, 1.0]])])
    with pytest.raises(NotImplementedError):
        PlanarPolygons.from_sequence("crowns.geojson")
    with pytest.raises(NotImplementedError):
        PlanarPolygons.from_sequence(Path("crowns.geojson"))
    # rings given out of row order are grouped by row; the table names boxes per row and an empty box for a row without rings
    pp = PlanarPolygons([square(4, 4, 5, 5), square(0, 0, 1, 1), square(7, 7, 8, 9)], [2, 0, 2], [False, False, False], n_polygons=4)
    rv, off, row, hole, boxes = pp.snapped()
    assert list(row) == [0, 2, 2] and list(off) == [0, 4, 8, 12] and rv.dtype == np.int64 and row.dtype == np.int32
    assert boxes.tolist() == [[0, 0, 1000000, 1000000], [1, 1, 0, 0], [4000000, 4000000, 8000000, 9000000], [1, 1, 0, 0]]
    # a ring the grid collapses is dropped
    sliver = PlanarPolygons.from_sequence([np.array([[0, 0], [1, 0], [0.5, 1e-8]])])
    assert sliver.snapped()[2].size == 0


# -- semantics ---------------------------------------------------------------------------------------------------------------
def test_nan_labels_are_masked_and_weights_scale():
    points, faces = flat_grid()
    mesh = make_mesh(points, faces)
    polys = [square(0, 0, 2, 2)]          # the four cells (0..1, 0..1): faces 0, 1, 2, 3 and 8, 9, 10, 11
    labels = np.full(len(faces), np.nan)
    labels[[0, 1, 2]] = 1                 # 1.5 m^2 of class 1
    labels[[3, 8]] = 0                    # 1.0 m^2 of class 0
    w = mesh.label_polygon_weights(labels, polys, points_in_polygon_CRS=points)
    assert w.tolist() == [[1.0, 1.5]]
    assert mesh.label_polygons(labels, polys, points_in_polygon_CRS=points) == [1.0]
    assert mesh.last_polygon_stats["pairs_contributing"] == 5 and mesh.last_polygon_stats["largest_ring"] == 4
    weighting = np.ones(len(faces))
    weighting[[3, 8]] = 4.0
    w = mesh.label_polygon_weights(labels, polys, face_weighting=weighting, points_in_polygon_CRS=points)
    assert w.tolist() == [[4.0, 1.5]]
    assert mesh.label_polygons(labels, polys, face_weighting=weighting, points_in_polygon_CRS=points) == [0.0]


def test_face_weight_is_area_ratio_times_weighting():
    """A 3-4-5 slope: every face is 5/4 of its footprint, so a unit footprint weighs 1.25 -- in the reference's order of
    operations (utils/numeric.py:305-327)."""
    points, faces = flat_grid()
    sloped = points.copy()
    sloped[:, 2] = 0.75 * sloped[:, 0]
    mesh = make_mesh(sloped, faces)
    labels = np.zeros(len(faces))
    w = mesh.label_polygon_weights(labels, [square(0, 0, 2, 2)], points_in_polygon_CRS=sloped)
    assert w.tolist() == [[5.0]]
    call = mesh.backend.last
    assert np.all(call["face_weight"] == 1.25) and call["tri"].dtype == np.int64 and call["tri"].shape == (len(faces), 6)
    w = mesh.label_polygon_weights(labels, [square(0, 0, 2, 2)], face_weighting=np.full(len(faces), 2.0),
                                   points_in_polygon_CRS=sloped)
    assert w.tolist() == [[10.0]]


def test_sjoin_counts_whole_faces_overlay_counts_intersections():
    points, faces = flat_grid()
    mesh = make_mesh(points, faces)
    labels = np.zeros(len(faces))
    polys = [square(0, 0, 1.5, 1)]       # the cell (0, 0) and the left half of the cell (1, 0)
    within = mesh.label_polygon_weights(labels, polys, sjoin_overlay=True, points_in_polygon_CRS=points)
    overlay = mesh.label_polygon_weights(labels, polys, sjoin_overlay=False, points_in_polygon_CRS=points)
    assert within.tolist() == [[1.0]] and overlay.tolist() == [[1.5]]


def test_ties_go_to_the_lowest_class_and_empty_polygons_are_nan():
    points, faces = flat_grid()
    labels = np.zeros(len(faces))
    labels[0::2] = 2                      # the first face of every cell is class 2, the second class 0: equal areas everywhere
    weighting = np.ones(len(faces))
    weighting[2:4] = 0.0                  # the cell (1, 0) weighs nothing
    polys = [square(0, 0, 1, 1), square(20, 20, 21, 21), square(1, 0, 2, 1)]
    mesh = make_mesh(points, faces, IDs_to_labels={0: "oak", 1: "pine", 2: "fir"})
    assert mesh.label_polygon_weights(labels, polys, face_weighting=weighting, points_in_polygon_CRS=points).tolist() == \
        [[0.5, 0.0, 0.5], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    ids = mesh.label_polygons(labels, polys, face_weighting=weighting, return_class_labels=False, points_in_polygon_CRS=points)
    assert ids[0] == 0.0 and np.isnan(ids[1]) and np.isnan(ids[2]) and all(isinstance(v, float) for v in ids)
    assert mesh.label_polygons(labels, polys, face_weighting=weighting, points_in_polygon_CRS=points) == \
        ["oak", "unknown", "unknown"]
    assert mesh.label_polygons(labels, polys, face_weighting=weighting, unknown_class_label="?",
                               points_in_polygon_CRS=points)[1] == "?"
    # without IDs_to_labels the ids come back whatever return_class_labels says
    plain = make_mesh(points, faces)
    assert plain.label_polygons(labels, polys[:1], points_in_polygon_CRS=points) == [0.0]
    # no labelled face at all: no classes, every polygon NaN
    none = plain.label_polygons(np.full(len(faces), np.nan), polys, points_in_polygon_CRS=points)
    assert len(none) == 3 and all(np.isnan(v) for v in none)


def test_chunked_class_delegates():
    points, faces = flat_grid()
    labels = (np.arange(len(faces)) % 2).astype(np.float64)
    polys = [square(0, 0, 3, 2), square(1, 1, 4, 4)]
    base = make_mesh(points, faces).label_polygons(labels, polys, sjoin_overlay=False, points_in_polygon_CRS=points)
    chunked = make_mesh(points, faces, cls=TexturedPhotogrammetryMeshChunked)
    assert chunked.label_polygons(labels, polys, sjoin_overlay=False, n_polygons_per_cluster=7,
                                  points_in_polygon_CRS=points) == base


def test_device_tensor_inputs_take_the_same_host_path():
    torch = pytest.importorskip("torch")
    points, faces = flat_grid()
    mesh = make_mesh(points, faces)
    labels = (np.arange(len(faces)) % 3).astype(np.float64)
    labels[5] = np.nan
    weighting = np.linspace(0.5, 2.0, len(faces))
    polys = [square(0.2, 0.1, 3.3, 2.7)]
    want = mesh.label_polygon_weights(labels, polys, face_weighting=weighting, sjoin_overlay=False, points_in_polygon_CRS=points)
    got = mesh.label_polygon_weights(torch.as_tensor(labels), polys, face_weighting=torch.as_tensor(weighting)[:, None],
                                     sjoin_overlay=False, points_in_polygon_CRS=points)
    assert np.array_equal(got, want)


# -- the C ABI tables ----------------------------------------------------------------------------------------------------------
def test_symbol_header_and_signature_table_agree():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "geograster.h").read_text(), flags=re.S)
    decl = re.search(r"\bint gr_polygon_class_weights\((.*?)\);", header, re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    assert "gr_polygon_class_weights" in _hip.EXPORTED_SYMBOLS
    sig = _hip._SIGNATURES["gr_polygon_class_weights"]
    assert len(params) == len(sig) == 18
    for text, ctype in zip(params, sig):
        want = _hip._vp if "*" in text else (_hip._i64 if text.startswith("int64_t") else _hip._i32)
        assert ctype is want, text
    assert (_hip.GR_POLY_OVERLAY, _hip.GR_POLY_WITHIN, _hip.GR_POLY_STAT_WORDS) == (0, 1, 4)
    source = (ROOT / "geograypher_amd" / "csrc" / "polygons.hip").read_text()
    assert re.search(r"\bint gr_polygon_class_weights\(gr_ctx \*c,", source)
    from geograypher_amd import build

    assert any(p.name == "polygons.hip" for p in build.SOURCES)
    assert hasattr(_hip.HipRaster, "polygon_class_weights")


# -- the stand-in against the exact oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_standin_decides_like_the_exact_oracle_and_e_ref_is_the_measured_error(name):
    d = load_scene(name)
    mesh = make_mesh(d["points"], d["faces"])
    got = {w: mesh.label_polygon_weights(d["face_labels"], d["polygons"], face_weighting=d["weighting"], sjoin_overlay=w,
                                         points_in_polygon_CRS=d["points"]) for w in (True, False)}
    call = mesh.backend.last
    tri, cls, table = call["tri"], call["face_class"], call["table"]
    exact = ps.exact_pairs(tri, cls, table)
    within = ps.standin_pairs(tri, cls, table, True)
    overlay = ps.standin_pairs(tri, cls, table, False)
    assert exact.keys() == within.keys() == overlay.keys() and len(exact) == int(d["pairs_per_polygon"].sum())
    assert [k for k in exact if exact[k][0] != within[k]] == []          # containment: equal on every pair
    worst = max(abs(Fraction(overlay[k]) - exact[k][1] / (2 * ps.GRID2_PER_M2)) for k in exact)
    assert float(worst) <= d["e_ref"]                                     # e_ref is the largest of these over all scenes
    # the committed answers are the oracle's
    for w, key in ((True, "weights_within"), (False, "weights_overlay")):
        want = ps.exact_class_weights(tri, cls, call["face_weight"], table, call["n_classes"], w, exact)
        assert np.array_equal(want, d[key])
    np.testing.assert_allclose(got[True], d["weights_within"], rtol=1e-12, atol=0)
    tol = ps.overlay_tolerance(d["e_ref"], d["pairs_per_polygon"], d["weights_overlay"])
    assert np.all(np.abs(got[False] - d["weights_overlay"]) <= tol)


def test_e_ref_is_attained_on_a_committed_scene():
    worst = Fraction(0)
    for name in SCENES:
        d = load_scene(name)
        mesh = make_mesh(d["points"], d["faces"])
        mesh.label_polygon_weights(d["face_labels"], d["polygons"], face_weighting=d["weighting"], sjoin_overlay=False,
                                   points_in_polygon_CRS=d["points"])
        call = mesh.backend.last
        exact = ps.exact_pairs(call["tri"], call["face_class"], call["table"])
        overlay = ps.standin_pairs(call["tri"], call["face_class"], call["table"], False)
        worst = max([worst] + [abs(Fraction(overlay[k]) - exact[k][1] / (2 * ps.GRID2_PER_M2)) for k in exact])
    assert float(worst) == float(np.load(GOLDEN)["e_ref"])


def test_contact_cases_of_the_integer_scene():
    """What each contact configuration must decide, spelled out: touching is inside, crossing the open interior is not."""
    d = load_scene("integer")
    mesh = make_mesh(d["points"], d["faces"])
    mesh.label_polygon_weights(d["face_labels"], d["polygons"], points_in_polygon_CRS=d["points"])
    call = mesh.backend.last
    within = ps.standin_pairs(call["tri"], call["face_class"], call["table"], True)
    inside = {p: sorted(f for (f, q), v in within.items() if q == p and v) for p in range(5)}
    cell = lambda row, col: 2 * (row * 6 + col)   # first face of the grid cell; + 1: the second
    assert inside[0] == sorted([cell(r, c) + k for r in (1, 2) for c in (1, 2) for k in (0, 1)])   # edges along face edges
    assert inside[1] == [cell(0, 4)]                                                                # the face equal to the polygon
    assert inside[2] == [cell(4, 4) + 1, cell(5, 4), cell(5, 4) + 1, cell(5, 5), cell(5, 5) + 1]   # cut faces are out
    assert cell(3, 0) not in inside[3] and len(inside[3]) == 7                                      # the face around the hole is out
    assert inside[4] == []                                                                          # ring vertices on its edges


# -- the generated scenes: the rule's fuzz, and what the device tests rely on ----------------------------------------------------
WAVE_FACES = (1, 63, 64, 65, 255, 256, 257, 513)


def _rings(case):
    return {p: ps.polygon_rings(case["table"], p) for p in range(len(case["table"][4]))}


@pytest.mark.parametrize("name", ["small", "large"])
def test_lattice_scene_standin_equals_oracle_and_has_every_category(name):
    case = ps.lattice_case(name)
    tri, table, info, exact = case["tri"], case["table"], case["info"], case["exact"]
    assert len(tri) == 257 and np.abs(tri).max() < 2 ** 40 and np.abs(table[0]).max() < 2 ** 40
    assert exact.keys() == case["within"].keys() == case["overlay"].keys()
    assert [k for k in exact if exact[k][0] != case["within"][k]] == []          # containment: equal on every pair
    worst = max(abs(Fraction(case["overlay"][k]) - exact[k][1] / (2 * ps.GRID2_PER_M2)) for k in exact)
    assert case["e_scene"] == float(worst) > 0.0
    print(f"[label_polygons] lattice {name}: {len(exact)} pairs, e_scene {case['e_scene']:.3e} m^2")
    # valid input, checked again on the scaled table: simple counter-clockwise rings of 3 to 8 vertices, holes inside, parts apart
    rings = _rings(case)
    for p, rs in rings.items():
        assert all(ps.ring_is_simple(r) and ps._area2_exact(r) > 0 and 3 <= len(r) <= 8 for r, _ in rs)
        assert [h for _, h in rs] == ([False, True] if p in info["holed"] else [False] * len(rs))
        if p in info["holed"]:
            assert ps.ring_strictly_inside(rs[1][0], rs[0][0])
        if p in info["two_part"]:
            assert len(rs) == 2 and ps.rings_apart(rs[0][0], rs[1][0])
    assert len(info["holed"]) >= 2 and len(info["two_part"]) >= 2
    # the categories
    contained = [k for k in exact if exact[k][0]]
    partial = [k for k in exact if not exact[k][0] and exact[k][1] > 0]
    contact = [k for k in exact if ps.has_contact(ps.ccw_triangle(tri[k[0]])[0], rings[k[1]])]
    contact_in = sum(exact[k][0] for k in contact)
    assert len(contained) >= 100 and len(partial) >= 100
    assert len(contact) >= 100 and contact_in >= 30 and len(contact) - contact_in >= 30
    for kind in ("holed", "two_part"):
        assert any(k[1] in info[kind] for k in contained) and any(k[1] in info[kind] for k in partial)
    short = sum(max(abs(t[0] - t[2]), abs(t[1] - t[3]), abs(t[0] - t[4]), abs(t[1] - t[5])) <= 2 * (ps.SMALL if name == "small"
                else ps.LARGE)["scale"] for t in tri.tolist())
    assert short >= 100                                                           # legs of 1-2 lattice steps


def test_large_lattice_scene_needs_128_bits():
    """Every triangle's twice-area is at least 2^64, and a `within` whose determinants wrap to 64 bits decides differently from
    the exact oracle on at least 20 pairs: the scene tells a kernel without the 128-bit type from a right one.  The small scene
    cannot (its determinants stay below 2^53)."""
    case = ps.lattice_case("large")
    assert all(ps.ccw_triangle(t)[1] >= 2 ** 64 for t in case["tri"])
    rings = _rings(case)
    wrong = [k for k, v in case["exact"].items() if ps.within_wrapped64(ps.ccw_triangle(case["tri"][k[0]])[0], rings[k[1]]) != v[0]]
    print(f"[label_polygons] lattice large: 64-bit determinants decide {len(wrong)} of {len(case['exact'])} pairs wrongly")
    assert len(wrong) >= 20
    small = ps.lattice_case("small")
    rings = _rings(small)
    assert all(ps.ccw_triangle(t)[1] < 2 ** 53 for t in small["tri"])
    assert all(ps.within_wrapped64(ps.ccw_triangle(small["tri"][k[0]])[0], rings[k[1]]) == v[0] for k, v in small["exact"].items())


@pytest.mark.parametrize("n_faces", WAVE_FACES)
def test_wave_scene_is_what_its_docstring_says(n_faces):
    case = ps.wave_case(n_faces)
    table, info, exact = case["table"], case["info"], case["exact"]
    P = ps.WAVE_POLYGONS
    assert exact.keys() == case["within"].keys() and [k for k in exact if exact[k][0] != case["within"][k]] == []
    assert table[2].tolist() == [0, 0, -1, 2, 3, 3, 3, P, 4, 4, 5] and np.diff(table[1]).tolist()[4:7] == [0, 1, 2]
    assert table[4][1].tolist() == list(ps.EMPTY_BOX) and table[4][3].tolist() != list(ps.EMPTY_BOX)
    for p in (0, 2, 4, 5):
        rs = ps.polygon_rings(table, p)
        assert rs and all(ps.ring_is_simple(r) and ps._area2_exact(r) > 0 for r, _ in rs)
    assert ps.polygon_rings(table, 1) == [] == ps.polygon_rings(table, 3)
    far = {k[0] // 64 for k in exact if k[1] == info["far_polygon"]}
    assert far == ({info["far_run"]} if n_faces > 1 else set())                   # the other waves skip it on the ballot
    assert not any(k[1] == 1 for k in exact)
    for n_classes in (1, 3, 70):
        tri, cls, weight, table2, info2 = ps.wave_scene(n_faces, n_classes)
        assert np.array_equal(tri, case["tri"]) and all(np.array_equal(a, b) for a, b in zip(table, table2))
        assert cls.min() >= -1 and cls.max() <= n_classes and weight.min() >= 0.0
        flat = np.array([ps.ccw_triangle(t)[1] == 0 for t in tri])
        assert np.array_equal(flat, info2["collapsed"])
        if n_classes > 1:
            assert not np.any(cls[~flat] == info2["idle_class"])
    if n_faces >= 63:
        tri, cls, weight, _, info2 = ps.wave_scene(n_faces, 70)
        o = [ps._orient(*t) for t in tri.tolist()]
        assert min(o) < 0 < max(o) and info2["collapsed"].any() and (cls == -1).any() and (cls == 70).any() and (weight == 0).any()
        assert len(set(cls[:64].tolist())) > 30 and any(exact[k][0] for k in exact)
        assert any(k[1] == 3 for k in exact)                                      # faces meet the box of the row of short rings


def test_pairs_tested_counts_box_overlap_whether_or_not_a_ring_is_usable():
    """GR_POLY_STAT_TESTED is "(face, polygon) pairs whose boxes overlap": a polygon all of whose rings are shorter than 3 vertices
    is tested against every face that meets its box and adds nothing; a polygon without any ring row has no box."""
    unit = 10 ** 6
    tri = np.array([[0, 0, 4, 0, 0, 4], [1, 1, 2, 1, 1, 2], [10, 10, 12, 10, 10, 12], [-1, -1, 3, -1, -1, 3]], dtype=np.int64) * unit
    rows = [(0, [(0, 0), (6, 0), (6, 6), (0, 6)], False), (1, [(1, 1), (2, 2)], False), (1, [(1, 2)], False), (1, [], False)]
    table = ps.make_table(rows, 3, unit)
    assert table[4].tolist() == [[0, 0, 6 * unit, 6 * unit], [unit, unit, 2 * unit, 2 * unit], list(ps.EMPTY_BOX)]
    cls, w = np.zeros(4, dtype=np.int32), np.ones(4)
    for within in (True, False):
        weights, stats = ps.polygon_class_weights_np(tri, cls, w, table, 1, within)
        pairs = ps.standin_pairs(tri, cls, table, within)
        # polygon 0 meets faces 0, 1, 3; polygon 1 (no usable ring) meets 0, 1, 3 as well; polygon 2 (no rows) none, though face 3's
        # box holds the placeholder box
        assert sorted(pairs) == [(0, 0), (0, 1), (1, 0), (1, 1), (3, 0), (3, 1)] == sorted(ps.exact_pairs(tri, cls, table))
        assert stats.tolist() == [6, 2 if within else 3, 4, 0]
        assert weights[1:].tolist() == [[0.0], [0.0]] and weights[0, 0] == (8.5 if within else 8.5 + 2.0)   # face 3 keeps x, y >= 0, x + y <= 2


def test_committed_scenes_have_no_polygon_without_a_usable_ring():
    """... so the change above leaves their `pairs_per_polygon` as committed."""
    for name in SCENES:
        d = load_scene(name)
        table = d["polygons"].snapped()
        for p in range(len(table[4])):
            assert ps.polygon_has_rows(table, p) == bool(ps.polygon_rings(table, p))
