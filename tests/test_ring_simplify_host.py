"""Ring simplification without a GPU: the exact stand-in of tests/simplify_standin.py against answers worked
out by hand, its independence of a ring's start and direction (S5), shared borders (S9), rows and holes (S8), the superset property
of a region of interest simplified and buffered, the keywords of the mesh methods and of `aggregate_images`, and the C ABI of the
new call."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import outline_standin as osn  # noqa: E402
import region_standin as rs  # noqa: E402
import simplify_standin as ss  # noqa: E402
import vector_standin as vs  # noqa: E402
from geograypher_amd import _hip, build  # noqa: E402
from geograypher_amd.entrypoints.aggregate_images import aggregate_images, parse_args  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import geometric  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
METHOD = "douglas-peucker"


class Backend(ss.StandInBackend, osn.StandInBackend, rs.StandInBackend, vs.StandInBackend):
    pass


def positions(ring, kept):
    return sorted(tuple(int(v) for v in ring[i]) for i in kept)


# -- S2-S6 by hand ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ss.hand_scenes()))
def test_hand_worked_answers(name):
    ring, fixed, T, want = ss.hand_scenes()[name]
    rv, off = ss.table([ring])
    keep, kept_index, out_offsets, stats, _ = ss.simplify_np(rv, off, T, fixed)
    assert kept_index.tolist() == want and out_offsets.tolist() == [0, len(want)]
    assert keep.tolist() == [int(i in want) for i in range(len(ring))]
    assert stats[ss.KEPT] == len(want) and stats[ss.COLLAPSED] == (0 if want else 1) and stats[ss.SHORT] == 0
    # ... and through the package's host layer, tolerance in metres
    got = geometric.simplify_rings(Backend(), rv, off, T * 1e-6, fixed)
    assert got[1].tolist() == want and got[2].tolist() == [0, len(want)] and got[3]["kept_vertices"] == len(want)
    assert got[0].dtype == np.uint8 and got[1].dtype == np.int32 and got[2].dtype == np.int64
    assert got[3]["collapsed_rings"] == (0 if want else 1) and got[3]["passes"] == stats[ss.PASSES]


def test_the_scenes_meet_the_cases_they_are_named_for():
    def tally(name):
        ring, fixed, T, _ = ss.hand_scenes()[name]
        return ss.simplify_np(*ss.table([ring]), T, fixed)[4]

    assert tally("a vertex exactly at the tolerance is dropped")["at_tolerance"] == 1
    assert tally("one step under it, the vertex is kept")["at_tolerance"] == 0
    assert tally("beyond the chord's ends, T = 5")["endpoint"] == 3 and tally("beyond the chord's ends, T = 6")["at_tolerance"] == 1
    assert tally("a three-way tie on the degenerate chord")["ties"] == 1 and tally("a square whose corners tie, T = 3")["ties"] == 2
    assert tally("the degenerate chord, T = the reach: the ring collapses")["collapsed"] == 1
    # short rings come out empty and are counted apart; an empty table is nothing
    keep, kept_index, out_offsets, stats, _ = ss.simplify_np(*ss.table([[(0, 0), (5, 5)], [(0, 0), (9, 0), (0, 9)], []]), 1)
    assert out_offsets.tolist() == [0, 0, 3, 3] and kept_index.tolist() == [2, 3, 4] and stats[ss.SHORT] == 2 and stats[ss.COLLAPSED] == 0
    assert ss.simplify_np(np.zeros((0, 2), np.int64), [0], 5)[2].tolist() == [0]
    # the sawtooth splits off one vertex a pass
    stats = ss.simplify_np(*ss.table([ss.sawtooth()]), 3)[3]
    assert stats[ss.PASSES] == 299 and stats[ss.KEPT] == 300


# -- S5 ----------------------------------------------------------------------------------------------------------------------------------
def test_kept_positions_do_not_depend_on_start_or_direction():
    rings = [(name, ring, T) for name, (ring, fixed, T, _) in ss.hand_scenes().items() if fixed is None]
    rings += [(name, ring, 12) for name, ring in zip(ss.s9_scene()[1], ss.s9_scene()[0])] + [("sawtooth", ss.sawtooth(40), 3)]
    for name, ring, T in rings:
        ring = np.asarray(ring, dtype=np.int64)
        assert len(np.unique(ring, axis=0)) == len(ring), name   # S5 speaks of rings without repeated positions
        want = positions(ring, ss.simplify_np(*ss.table([ring]), T)[1])
        for turned in (ring, ring[::-1]):
            for k in range(len(ring)):
                moved = np.roll(turned, k, axis=0)
                assert positions(moved, ss.simplify_np(*ss.table([moved]), T)[1]) == want, (name, k)


# -- S9 ----------------------------------------------------------------------------------------------------------------------------------
def test_shared_borders_keep_the_same_vertices_in_both_rings():
    rings, names, wiggle = ss.s9_scene()
    rv, off = ss.table(rings)
    fixed = geometric.shared_border_fixed(rv, off)
    assert fixed.dtype == np.uint8 and np.array_equal(fixed, ss.shared_border_fixed_np(rv, off))
    fixed_positions = {tuple(int(v) for v in rv[i]) for i in np.nonzero(fixed)[0]}
    assert fixed_positions == {(1000, 100), (1000, 1000), (0, 100), (2000, 100)}   # the junctions; no vertex of the island
    for T in (0, 3, 6, 40):
        keep, kept_index, out_offsets, stats, _ = ss.simplify_np(rv, off, T, fixed)
        kept = [{tuple(int(v) for v in rv[i]) for i in kept_index[out_offsets[r]:out_offsets[r + 1]]} for r in range(len(rings))]
        border = set(wiggle)
        assert kept[0] & border == kept[2] & border                       # A and B along their border
        assert kept[1] == kept[3]                                          # A's hole and B's island
        assert fixed_positions <= kept[0] | kept[2] | kept[4]
        if T == 6:
            assert 0 < len(kept[0] & border) < len(border) and 3 <= len(kept[1]) < len(rings[1])
    # the package's sort agrees with the dictionaries on a table full of repeated positions
    rv, off = ss.table(ss.random_scene(seed=4))
    assert np.array_equal(geometric.shared_border_fixed(rv, off), ss.shared_border_fixed_np(rv, off))
    assert geometric.shared_border_fixed(np.zeros((0, 2), np.int64), [0]).shape == (0,)


def test_outlines_carry_ids_and_holes_through_the_kept_indices():
    rings, names, _ = ss.s9_scene()
    rv, off = ss.table(rings)
    areas2 = geometric.ring_areas2_exact(rv, off)
    outlines = geometric.FaceLabelOutlines(off, np.array([0.0, 0.0, 1.0, 1.0, 2.0]), np.arange(len(rv), dtype=np.int32) + 7,
                                           rv.astype(np.float64) * 1e-6, np.array([a < 0 for a in areas2]), {"rings": 5}, (rv, areas2))
    simple = outlines.simplified(12e-6, Backend(), shared_borders=True)
    fixed = ss.shared_border_fixed_np(rv, off)
    keep, kept_index, out_offsets, stats, _ = ss.simplify_np(rv, off, 12, fixed)
    assert np.array_equal(simple.ring_offsets, out_offsets) and np.array_equal(simple.ring_vertex_ids, kept_index + 7)
    assert np.array_equal(simple.ring_xy, rv[kept_index] * 1e-6) and np.array_equal(simple.ring_is_hole, outlines.ring_is_hole)
    assert np.array_equal(simple.snapped[0], rv[kept_index]) and len(simple) == 5
    assert simple.snapped[1] == geometric.ring_areas2_exact(rv[kept_index], out_offsets)
    assert simple.stats["rings"] == 5 and simple.stats["simplify_kept_vertices"] == len(kept_index) == stats[ss.KEPT]
    assert simple.stats["simplify_passes"] == stats[ss.PASSES] and simple.stats["simplify_collapsed_rings"] == 0
    free = outlines.simplified(12e-6, Backend(), shared_borders=False)
    assert np.array_equal(free.ring_vertex_ids, ss.simplify_np(rv, off, 12)[1] + 7)
    # a tolerance that collapses the island: the ring stays in the table, without vertices
    gone = outlines.simplified(400e-6, Backend())
    assert len(gone) == 5 and gone.ring_offsets[2] == gone.ring_offsets[1] and gone.snapped[1][1] == 0
    assert gone.stats["simplify_collapsed_rings"] >= 1


# -- S8 and the region of interest -----------------------------------------------------------------------------------------------------
def wiggly_square(x0, y0, side, n=24, amp=0.04, seed=3):
    """A square of `side` metres whose sides carry n jittered vertices each (a few centimetres off the line)."""
    rng = np.random.default_rng(seed)
    t = (np.arange(n) + rng.uniform(0.2, 0.8, n)) / n * side
    j = rng.uniform(-amp, amp, (4, n))
    return np.concatenate([np.column_stack([x0 + t, y0 + j[0]]), np.column_stack([x0 + side + j[1], y0 + t]),
                           np.column_stack([x0 + side - t, y0 + side + j[2]]), np.column_stack([x0 + j[3], y0 + side - t])])


def test_rows_and_holes_of_simplified_polygons():
    outer, hole, sliver = wiggly_square(0, 0, 10), wiggly_square(4, 4, 2, n=6, seed=4)[::-1], np.array([[20, 0], [25, 0.01], [30, 0], [25, -0.01]])
    lone_hole = wiggly_square(21, -1, 0.5, n=3, amp=0.001, seed=5)[::-1]
    polygons = PlanarPolygons([outer, hole, sliver, lone_hole, wiggly_square(40, 0, 5, seed=6)], [0, 0, 1, 1, 3], [False, True, False, True, False],
                              n_polygons=4)
    polygons.epsg = 32610
    simple = polygons.simplified(0.1, Backend())
    assert simple.n_polygons == 4 and simple.epsg == 32610
    assert simple.ring_polygon.tolist() == [0, 0, 3] and simple.ring_is_hole.tolist() == [False, True, False]   # S8: row 1 lost its hole too
    assert all(4 <= len(r) <= 8 for r in simple.rings)                       # about the corners stay, 0.04 m of jitter goes at 0.1 m
    kept_lone_hole = simple.last_simplify_stats["kept_vertices"] - sum(len(r) for r in simple.rings)   # kept itself, dropped with its row
    assert simple.last_simplify_stats["collapsed_rings"] == 1 and 3 <= kept_lone_hole <= 12
    for ring, source in zip(simple.rings, (outer, hole, polygons.rings[4])):   # kept vertices ARE input vertices (to the grid)
        assert all(np.abs(source - v).max(axis=1).min() < 1e-6 for v in ring)
    # a hole collapses alone and the row keeps its exterior
    tiny = PlanarPolygons([outer, wiggly_square(4, 4, 0.05, n=2, amp=0.001)[::-1]], [0, 0], [False, True]).simplified(0.1, Backend())
    assert tiny.ring_is_hole.tolist() == [False] and tiny.last_simplify_stats["collapsed_rings"] == 1
    # tolerance 0 drops nothing that is off its chord
    assert [len(r) for r in polygons.simplified(0, Backend()).rings] == [len(r) for r in polygons.rings]
    assert len(PlanarPolygons([], [], [], n_polygons=2).simplified(1.0, Backend()).rings) == 0


def test_simplified_and_buffered_region_holds_the_buffered_region():
    """The consequence of S3-S4 that makes the ROI use sound: within b of the region -> within b + s of the region simplified at s."""
    roi = PlanarPolygons([wiggly_square(0, 0, 6, n=16, amp=0.3, seed=8), wiggly_square(2, 2, 2, n=8, amp=0.2, seed=9)[::-1]], [0, 0],
                         [False, True])
    xs = np.arange(-1.5, 7.6, 0.25)
    points = np.array([(x, y) for x in xs for y in xs])
    backend = Backend()
    for b, s in ((0.0, 0.5), (0.4, 0.25), (0.25, 1.0)):
        simple = roi.simplified(s, backend)
        assert sum(len(r) for r in simple.rings) < sum(len(r) for r in roi.rings)
        inside = np.asarray(geometric.points_in_region(backend, roi, points, b)[0], dtype=bool)
        wider = np.asarray(geometric.points_in_region(backend, simple, points, b + s)[0], dtype=bool)
        assert inside.sum() > 50 and (~wider).sum() > 50 and not np.any(inside & ~wider), (b, s)


def grid_mesh(n=6):
    verts_q, faces, quad = osn.grid_mesh(n, n)
    points = np.column_stack([verts_q.astype(np.float64) * 1e-6, np.zeros(len(verts_q))])
    return points, faces, quad


def test_select_mesh_ROI_simplifies_and_widens_the_buffer():
    points, faces, _ = grid_mesh()
    mesh = TexturedPhotogrammetryMesh((points, faces.astype(np.int64)), log_level="ERROR", backend=Backend())
    lo, hi = points[:, :2].min(axis=0), points[:, :2].max(axis=0)
    side = float((hi - lo).min()) * 0.5
    roi = [wiggly_square(lo[0] + side * 0.4, lo[1] + side * 0.4, side, n=10, amp=side * 0.02, seed=2)]
    s = side * 0.05
    plain = mesh.select_mesh_ROI(roi, buffer_meters=s, return_original_IDs=True, points_in_ROI_CRS=points)
    got = mesh.select_mesh_ROI(roi, buffer_meters=s, simplify_tol_meters=s, simplify_method=METHOD, return_original_IDs=True,
                               points_in_ROI_CRS=points)
    assert mesh.backend.last_simplify["tol_meters"] == s and mesh.backend.last_region["D"] == int(np.rint(2 * s / 1e-6))
    assert 4 <= len(mesh.backend.last_region["table"][0]) < 20                 # the region test saw the simplified ring, not all 40 vertices
    assert set(plain[1].tolist()) <= set(got[1].tolist()) and set(plain[2].tolist()) <= set(got[2].tolist()) and len(got[2]) > 0
    # the constructor hands both keywords on
    cropped = TexturedPhotogrammetryMesh((points, faces.astype(np.int64)), log_level="ERROR", backend=Backend(), ROI=roi, ROI_buffer_meters=s,
                                         points_in_ROI_CRS=points, ROI_simplify_tol_meters=s, ROI_simplify_method=METHOD)
    assert np.array_equal(cropped.ROI_face_IDs, got[2])
    # not asked for by name: as before; a wrong name: ValueError
    with pytest.raises(NotImplementedError, match="simplify_tol_meters"):
        mesh.select_mesh_ROI(roi, simplify_tol_meters=s, points_in_ROI_CRS=points)
    with pytest.raises(ValueError, match="simplify_method"):
        mesh.select_mesh_ROI(roi, simplify_tol_meters=s, simplify_method="visvalingam", points_in_ROI_CRS=points)
    with pytest.raises(NotImplementedError, match="simplify_tol_meters"):
        TexturedPhotogrammetryMesh((points, faces.astype(np.int64)), log_level="ERROR", backend=Backend(), ROI=roi,
                                   points_in_ROI_CRS=points, ROI_simplify_tol_meters=s)


# -- the class map -------------------------------------------------------------------------------------------------------------------------
def three_classes(quad, n):
    """Left half class 0, right half class 1, the bottom row class 2, one quad of class 1 inside class 0."""
    cls = [(2 if j == 0 else (0 if i < n // 2 else 1)) for j in range(n) for i in range(n)]
    cls[2 * n + 1] = 1
    return osn.quad_classes(quad, cls).astype(np.float64)


def test_export_simplifies_the_class_map(tmp_path):
    n = 6
    points, faces, quad = grid_mesh(n)
    labels = three_classes(quad, n)
    mesh = TexturedPhotogrammetryMesh((points, faces.astype(np.int64)), log_level="ERROR", backend=Backend())
    plain, plain_columns = mesh.export_face_labels_vector(labels, points_in_export_CRS=points)
    step = float(np.diff(np.unique(np.round(points[:, 0], 3)))[0])
    tol = step * 0.3
    simple, columns = mesh.export_face_labels_vector(labels, export_file=tmp_path / "map.geojson", points_in_export_CRS=points,
                                                     simplify_tol=tol, simplify_method=METHOD)
    stats = mesh.last_outline_stats
    assert np.array_equal(columns["class_ID"] if "class_ID" in columns else list(columns.values())[0], [0.0, 1.0, 2.0])
    assert simple.n_polygons == plain.n_polygons == 3 and simple.ring_is_hole.sum() == plain.ring_is_hole.sum() == 1
    n_plain, n_simple = sum(len(r) for r in plain.rings), sum(len(r) for r in simple.rings)
    assert stats["simplify_kept_vertices"] == n_simple < n_plain and stats["simplify_passes"] >= 2 and stats["simplify_collapsed_rings"] == 0
    # S9: wherever two rings of the simplified map share a vertex of the plain map's border, both kept it -- the vertex sets of
    # the simplified rings, cut to the positions two plain rings share, agree ring pair by ring pair
    def grid(ring):
        return {tuple(v) for v in np.rint(ring / 1e-6).astype(np.int64).tolist()}

    plain_sets, simple_sets = [grid(r) for r in plain.rings], [grid(r) for r in simple.rings]
    shared_pairs = 0
    for a in range(len(plain_sets)):
        for b in range(a + 1, len(plain_sets)):
            both = plain_sets[a] & plain_sets[b]
            if both:
                shared_pairs += 1
                assert simple_sets[a] & both == simple_sets[b] & both
    assert shared_pairs >= 3
    back, _ = PlanarPolygons.from_geojson(tmp_path / "map.geojson")
    assert [len(r) for r in back.rings] == [len(r) for r in simple.rings]
    # a tolerance of most of a quad: the island of class 1 and class 0's hole collapse together.  A huge one leaves the fixed
    # junctions alone (S9): those of classes 0 and 1 span an area, those of the bottom row lie on one line -- class 2 loses its row
    big, big_columns = mesh.export_face_labels_vector(labels, points_in_export_CRS=points, simplify_tol=step * 0.8, simplify_method=METHOD)
    assert big.ring_is_hole.sum() == 0 and mesh.last_outline_stats["simplify_collapsed_rings"] == 2 and big.n_polygons == 3
    none, none_columns = mesh.export_face_labels_vector(labels, points_in_export_CRS=points, simplify_tol=step * 100, simplify_method=METHOD)
    assert none.n_polygons == 2 and len(none.rings) == 2 and list(none_columns.values())[0].tolist() == [0.0, 1.0]
    assert mesh.last_outline_stats["rows"] == 2 and mesh.last_outline_stats["simplify_collapsed_rings"] == 3
    # not asked for by name: as before
    with pytest.raises(NotImplementedError, match="simplify_tol"):
        mesh.export_face_labels_vector(labels, points_in_export_CRS=points, simplify_tol=tol)
    with pytest.raises(ValueError, match="simplify_method"):
        mesh.export_face_labels_vector(labels, points_in_export_CRS=points, simplify_tol=tol, simplify_method="dp")
    assert mesh.export_face_labels_vector(labels, points_in_export_CRS=points)[0].rings[0].shape == plain.rings[0].shape


def test_aggregate_images_keywords_and_flags():
    base = ["--mesh-file", "m.npz", "--mesh-CRS", "EPSG:4978", "--cameras-file", "c.xml", "--image-folder", "i", "--label-folder", "l",
            "--IDs-to-labels", "ids.json"]
    args = parse_args(base)
    assert args.top_down_simplify_tol == 0.0 and args.top_down_simplify_method is None
    args = parse_args(base + ["--top-down-simplify-tol", "0.5", "--top-down-simplify-method", METHOD])
    assert args.top_down_simplify_tol == 0.5 and args.top_down_simplify_method == METHOD
    with pytest.raises(SystemExit):
        parse_args(base + ["--top-down-simplify-method", "visvalingam"])
    # both refusals come before any file is opened
    with pytest.raises(NotImplementedError, match="top_down_simplify_tol"):
        aggregate_images("m.npz", None, "i", "l", "EPSG:4978", IDs_to_labels={0: "a"}, top_down_simplify_tol=0.5)
    with pytest.raises(ValueError, match="top_down_simplify_method"):
        aggregate_images("m.npz", None, "i", "l", "EPSG:4978", IDs_to_labels={0: "a"}, top_down_simplify_tol=0.5,
                         top_down_simplify_method="visvalingam")


# -- S1 and the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_every_S1_violation_is_a_ValueError_naming_the_call():
    rv, off = ss.table([[(0, 0), (9, 0), (0, 9)]])
    ok = _hip.check_simplify_tables(rv, off, 2e-6, np.array([1, 0, 0], dtype=np.uint8))
    assert ok == (3, 1, 2) and _hip.check_simplify_tables(np.zeros((0, 2), np.int64), np.zeros(1, np.int64), 0) == (0, 0, 0)
    assert _hip.simplify_tol_steps(0.05) == 50000 and _hip.simplify_tol_steps(2 ** 40 * 1e-6 - 1e-6) == 2 ** 40 - 1
    edge = rv.copy()
    edge[1, 0] = 2 ** 40                                          # |coordinate| = 2^40 is allowed, one more is not
    assert _hip.check_simplify_tables(edge, off, 1e-6)[0] == 3
    bad = [
        (rv.reshape(-1), off, 1e-6, None), (rv.astype(np.float64), off, 1e-6, None), (rv[:, :1], off, 1e-6, None),
        (edge + np.array([[0, 0], [1, 0], [0, 0]]), off, 1e-6, None), (-edge - np.array([[0, 0], [1, 0], [0, 0]]), off, 1e-6, None),
        (rv, [0, 2], 1e-6, None), (rv, [1, 3], 1e-6, None), (rv, [0, 2, 1, 3], 1e-6, None), (rv, np.zeros(0, np.int64), 1e-6, None),
        (rv, np.array([0.0, 3.0]), 1e-6, None), (rv, [[0, 3]], 1e-6, None),
        (rv, off, -1e-6, None), (rv, off, float("nan"), None), (rv, off, float("inf"), None), (rv, off, 2 ** 40 * 1e-6, None),
        (rv, off, "wide", None),
        (rv, off, 1e-6, np.zeros(2, np.uint8)), (rv, off, 1e-6, np.zeros((3, 1), np.uint8)), (rv, off, 1e-6, np.zeros(3, np.float64)),
    ]
    for ring_vertices, ring_offsets, tol, fixed in bad:
        with pytest.raises(ValueError, match="gr_simplify_rings"):
            _hip.check_simplify_tables(np.asarray(ring_vertices), np.asarray(ring_offsets), tol, fixed)


def test_header_binding_and_source_name_the_new_call():
    main = (ROOT / "include" / "geograster.h").read_text()
    header = (ROOT / "include" / "geograster_simplify.h").read_text()
    source = (ROOT / "geograypher_amd" / "csrc" / "simplify.hip").read_text()
    internal = (ROOT / "geograypher_amd" / "csrc" / "gr_internal.hpp").read_text()
    decl = re.search(r"\bint gr_simplify_rings\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == 12 == len(_hip._SIMPLIFY_SIGNATURES["gr_simplify_rings"])
    assert _hip.SIMPLIFY_SYMBOLS == ("gr_simplify_rings",) and re.search(r"\bint gr_simplify_rings\(gr_ctx \*c,", source)
    assert "gr_simplify_rings" not in main and main.count('#include "geograster_simplify.h"') == 1
    assert main.index('#include "geograster_simplify.h"') > main.index('#include "geograster_communities.h"')
    assert "#define GR_VERSION 126" in main and "without\n * a GR_VERSION bump" in header
    for line in ("meshes.py:695", "1241", "1417", "utils/geometric.py:70-77", "DESIGN.md section 8q"):
        assert line in header, line
    for word, value in (("KEPT", 0), ("COLLAPSED", 1), ("PASSES", 2), ("WIDE", 3), ("SHORT_RINGS", 4), ("WORDS", 8)):
        assert re.search(rf"GR_SIMPLIFY_STAT_{word} = {value}\b", main) and getattr(_hip, f"GR_SIMPLIFY_STAT_{word}") == value
    assert tuple(geometric.SIMPLIFY_STAT_NAMES) == ("kept_vertices", "collapsed_rings", "passes", "wide_comparisons", "short_rings")
    assert (ss.KEPT, ss.COLLAPSED, ss.PASSES, ss.WIDE, ss.SHORT, ss.STAT_WORDS) == (0, 1, 2, 3, 4, 8)
    assert any(p.name == "simplify.hip" for p in build.SOURCES)
    kernels = re.findall(r"__global__ __launch_bounds__\(256\) void (k_simp_\w+)\(", source)
    assert len(kernels) >= 10 and all(k in internal for k in kernels)
    assert "stage_acquire(c, c->stage, p.finish(), s, \"simplify-rings\")" in source and "const FlagScan fs(c, p, N);" in source
    assert "__umul64hi" in source and "__umul64hi" in (ROOT / "geograypher_amd" / "csrc" / "polygons.hip").read_text()
    assert callable(_hip.HipRaster.ring_simplifier) and callable(_hip.RingSimplifier.simplify)
