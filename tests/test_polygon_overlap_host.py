"""The polygon-on-polygon overlap areas without a GPU: the stand-ins of tests/overlap_standin.py on hand-worked
cases and against an independent exact clip; the item builder and the table checks; the companion header against the binding and
the library; `polygon_overlap_areas`, `get_overlap_vector` and `cf_from_vector_vector` through the stand-in backend on `.geojson`
files; and the measurement of the bound K of rule A6."""
import ctypes
import json
import math
import re
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import overlap_standin as ov  # noqa: E402
from geograypher_amd import _hip, build  # noqa: E402
from geograypher_amd.utils import geospatial as gs  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons, overlap_work_items, snap_polygon_pair  # noqa: E402
from geograypher_amd.utils.prediction_metrics import cf_from_vector_vector  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
GRID2 = 10 ** 12    # square grid steps in a square metre


# -- hand-worked cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("case", range(len(ov.HAND_CASES)))
def test_hand_worked_cases(case, shifted):
    name, rows_a, rows_b, want, n_pairs = ov.HAND_CASES[case]
    table_a, table_b, pairs = ov.scene_tables(f"hand {case}", shifted)
    assert len(pairs) == n_pairs, name
    if not n_pairs:
        return
    area, area_abs = ov.exact_pair(table_a, table_b, 0, 0)
    if want is None:   # the crossing triangles: the second one is convex
        want = ov.clip_area(rows_a[0][0], rows_b[0][0] if _is_ccw(rows_b[0][0]) else rows_b[0][0][::-1])
        assert want > 0
    assert area == Fraction(want) * GRID2 and area_abs >= area, name
    fixed, fixed_abs, stats = ov.exact_areas(table_a, table_b, pairs)
    assert abs(Fraction(fixed[0], 1 << ov.FIXED_BITS) - area) < Fraction(1, 1 << 200) and ov.is_zero(fixed[0]) == (area == 0)
    restated, restated_abs, stats_2 = ov.restated_areas(table_a, table_b, pairs)
    assert abs(restated[0] - float(area)) <= gs.overlap_bound(restated_abs[0]) and np.array_equal(stats, stats_2)
    assert restated_abs[0] == pytest.approx(float(area_abs), rel=1e-12)


def _is_ccw(ring):
    return sum(ring[k - 1][0] * ring[k][1] - ring[k][0] * ring[k - 1][1] for k in range(len(ring))) > 0


def test_statistics_by_hand():
    # a holed square (two rings of 4, each with 2 vertical edges) against a square and a ring of 2 vertices on the same row
    A = PlanarPolygons([np.array(r, dtype=float) for r in ov.HOLED], [0, 0], [False, True])
    B = PlanarPolygons([np.array(ov.square(2, 2, 6, 6), dtype=float)], [0], [False])
    table_a, table_b, _ = snap_polygon_pair(A, B)
    rv, off, rp, rh, box = table_b
    table_b = (np.concatenate([rv, rv[:2]]), np.append(off, off[-1] + 2), np.append(rp, 0).astype(np.int32), np.append(rh, 0).astype(np.int32), box)
    area, area_abs, stats = ov.exact_areas(table_a, table_b, [[0, 0]], n_items=1)
    # horizontal edges: 4 of a, 2 of b; x-ranges [0,4] and [1,3] of a against [2,6] of b cut to X = [2,4]: every one of the 8 pairs takes part
    assert stats.tolist() == [1, 1, 8, 6, 1, 4, 0, 0] and area[0] == (3 * GRID2) << ov.FIXED_BITS


def test_exact_rules_equal_the_independent_clip_on_stars():
    rng = np.random.default_rng(5)
    stars = ov.star_rows(31, 12, extent=(20.0, 20.0))
    seen_partial = 0
    for k, (ring,) in enumerate(stars):
        n = int(rng.integers(3, 9))
        angle = np.sort(rng.uniform(0, 2 * np.pi, n))
        convex = np.rint((np.array([10.0, 10.0]) + rng.uniform(3, 12) * np.stack([np.cos(angle), np.sin(angle)], axis=1)) * 1e6) / 1e6
        A, B = PlanarPolygons([ring], [0], [False]), PlanarPolygons([convex], [0], [False])
        table_a, table_b, origin = snap_polygon_pair(A, B)
        if not len(ov.box_pairs(table_a, table_b)):
            continue
        area, _ = ov.exact_pair(table_a, table_b, 0, 0)
        want = ov.clip_area([tuple(int(v) for v in p) for p in table_a[0]], [tuple(int(v) for v in p) for p in table_b[0]])
        assert area == want, k
        own = ov.clip_area([tuple(int(v) for v in p) for p in table_b[0]], [tuple(int(v) for v in p) for p in table_b[0]])
        seen_partial += 0 < area < own
    assert seen_partial >= 3


@pytest.mark.parametrize("name", ["rings", "parts", "edges"])
def test_a_row_against_itself_is_its_own_area(name):
    table_a, _, _ = ov.scene_tables(name)
    rv, off, rp, rh, _ = table_a
    for row in range(min(len(table_a[4]), 2)):
        twice = 0
        for r in np.nonzero(rp == row)[0]:
            ring = [(int(x), int(y)) for x, y in rv[off[r]:off[r + 1]]]
            a2 = sum(ring[k - 1][0] * ring[k][1] - ring[k][0] * ring[k - 1][1] for k in range(len(ring)))
            twice += -a2 if rh[r] else a2
        if off[np.searchsorted(rp, row, "right")] - off[np.searchsorted(rp, row, "left")] > 600:
            area = Fraction(ov.exact_areas(table_a, table_a, [[row, row]])[0][0], 1 << ov.FIXED_BITS)
            assert abs(area - Fraction(twice, 2)) < Fraction(1, 1 << 200)
        else:
            assert ov.exact_pair(table_a, table_a, row, row)[0] == Fraction(twice, 2)


# -- the item builder --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [(256, 4096), (8, 16), (1, 1), (256, 1), (3, 4096)])
def test_work_items_cover_every_edge_pair_once(tile):
    table_a, table_b, pairs = ov.scene_tables("parts")
    pairs = pairs[::-1].copy()          # the pairs keep their own order
    items = overlap_work_items(table_a[1], table_a[2], table_b[1], table_b[2], pairs, tile)
    assert items.dtype == np.int32 and items.shape[1] == _hip.GR_OVERLAP_ITEM_INTS and np.all(np.diff(items[:, 0]) >= 0)
    _hip.check_overlap_items(pairs, items, table_a[1], table_a[2], len(table_a[4]), table_b[1], table_b[2], len(table_b[4]))
    for k, (a, b) in enumerate(pairs.tolist()):
        seen = set()
        for _, a0, na, b0, nb in items[items[:, 0] == k].tolist():
            assert 1 <= na <= tile[0] and 1 <= nb <= tile[1]
            block = {(i, j) for i in range(a0, a0 + na) for j in range(b0, b0 + nb)}
            assert not seen & block
            seen |= block
        slots = lambda t, row: range(int(t[1][np.searchsorted(t[2], row, "left")]), int(t[1][np.searchsorted(t[2], row, "right")]))  # noqa: E731
        assert seen == {(i, j) for i in slots(table_a, a) for j in slots(table_b, b)}
    with pytest.raises(ValueError, match="at most 256 x 4096"):
        overlap_work_items(table_a[1], table_a[2], table_b[1], table_b[2], pairs, (257, 1))
    # a row without rings: its pairs have no item
    assert len(overlap_work_items([0], [], table_b[1], table_b[2], np.zeros((0, 2)))) == 0


def test_malformed_tables_and_items_are_refused():
    table_a, table_b, pairs = ov.scene_tables("parts")
    assert _hip.check_overlap_tables(table_a, table_b) == (len(table_a[2]), len(table_b[2]))
    rv, off, rp, rh, box = table_a
    for bad in (dict(rv=rv.astype(np.float64)), dict(rv=rv.reshape(-1)), dict(rv=rv * (1 << 30)), dict(off=off[:-1]), dict(off=off[::-1].copy()),
                dict(rp=rp[::-1].copy()), dict(rp=rp + 2), dict(rh=rh[:-1]), dict(rh=rh.astype(np.float64)), dict(box=box[:, :3]), dict(box=box * (1 << 30)),
                dict(box=box + np.array([1, 0, 0, 0])), dict(box=box - np.array([0, 0, 0, 1]))):
        t = dict(rv=rv, off=off, rp=rp, rh=rh, box=box)
        t.update(bad)
        with pytest.raises(ValueError, match="gr_polygon_overlap_areas"):
            _hip.check_overlap_tables(tuple(t.values()), table_b)
        with pytest.raises(ValueError, match="gr_polygon_overlap_areas.*table b"):
            _hip.check_overlap_tables(table_a, tuple(t.values()))
    args = (table_a[1], table_a[2], len(table_a[4]), table_b[1], table_b[2], len(table_b[4]))
    n_a = int(table_a[1][np.searchsorted(table_a[2], 0, "right")])
    n_b = int(table_b[1][np.searchsorted(table_b[2], 0, "right")])
    assert pairs[0].tolist() == [0, 0]
    _hip.check_overlap_items(pairs, np.array([[0, 0, n_a, 0, n_b]], dtype=np.int32), *args)
    for item in ([-1, 0, 1, 0, 1], [len(pairs), 0, 1, 0, 1], [0, 0, 0, 0, 1], [0, 0, 1, 0, 0], [0, 0, 257, 0, 1], [0, 0, 1, 0, 4097], [0, -1, 1, 0, 1],
                 [0, 0, 1, -1, 1], [0, n_a, 1, 0, 1], [0, 0, 1, n_b, 1], [0, n_a - 1, 2, 0, 1], [0, 0, 1, n_b - 1, 2]):
        with pytest.raises(ValueError, match="gr_polygon_overlap_areas: work item 0"):
            _hip.check_overlap_items(pairs, np.array([item], dtype=np.int32), *args)
    with pytest.raises(ValueError, match="gr_polygon_overlap_areas: work item 1"):        # a pair below one in front of it
        _hip.check_overlap_items(pairs, np.array([[1, 0, 1, n_b, 1], [0, 0, 1, 0, 1]], dtype=np.int32), *args)
    with pytest.raises(ValueError, match="gr_polygon_overlap_areas: work items"):
        _hip.check_overlap_items(pairs, np.zeros((1, 4), dtype=np.int32), *args)
    with pytest.raises(ValueError, match="gr_polygon_overlap_areas: pair 0"):
        _hip.check_overlap_items(np.array([[0, 2]]), np.zeros((0, 5), dtype=np.int32), *args)
    with pytest.raises(ValueError, match="gr_polygon_overlap_areas: pairs"):
        _hip.check_overlap_items(np.zeros((1, 3), dtype=np.int32), np.zeros((0, 5), dtype=np.int32), *args)


# -- the companion header -----------------------------------------------------------------------------------------------------------------
def test_companion_header_binding_and_library_agree():
    main = (ROOT / "include" / "geograster.h").read_text()
    assert re.search(r'^#include "geograster_overlap.h"$', main, re.M) and main.index("geograster_overlap.h") < main.rindex("#ifdef __cplusplus")
    assert main.index('#include "geograster_burn.h"') < main.index('#include "geograster_overlap.h"') and "#define GR_VERSION 126" in main
    assert not re.search(r"gr_polygon_overlap_areas\s*\(|gr_polygon_box_pairs", main)
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", (ROOT / "include" / "geograster_overlap.h").read_text(), flags=re.S)
    declared = {name: [a.strip() for a in " ".join(args.split()).split(",")]
                for name, args in re.findall(r"\b(gr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}
    assert sorted(declared) == sorted(_hip._OVERLAP_SIGNATURES) == sorted(_hip.OVERLAP_SYMBOLS) == [
        "gr_polygon_box_pairs_count", "gr_polygon_box_pairs_fill", "gr_polygon_overlap_areas"]
    others = (set(_hip._SIGNATURES) | set(_hip._COMPANION_SIGNATURES) | set(_hip._ORTHO_SIGNATURES) | set(_hip._DECIMATE_SIGNATURES)
              | set(_hip._BURN_SIGNATURES))
    assert not set(declared) & others
    kinds = {ctypes.c_int64: "int64", ctypes.c_int: "int", ctypes.c_int32: "int", ctypes.c_double: "double"}
    lib = ctypes.CDLL(str(build.build()))
    for name, arguments in declared.items():
        argtypes = _hip._OVERLAP_SIGNATURES[name]
        assert len(arguments) == len(argtypes) and hasattr(lib, name), name
        for argument, ctype in zip(arguments, argtypes):
            want = "pointer" if "*" in argument else {"int64_t": "int64", "int32_t": "int", "int": "int", "double": "double"}[argument.split()[0]]
            got = "pointer" if ctype is ctypes.c_void_p or issubclass(ctype, ctypes._Pointer) else kinds[ctype]
            assert want == got, f"{name}: {argument!r} is bound as {ctype.__name__}"
    assert len(declared["gr_polygon_overlap_areas"]) == 25
    assert (_hip.GR_OVERLAP_STAT_PAIRS, _hip.GR_OVERLAP_STAT_ITEMS, _hip.GR_OVERLAP_STAT_EDGE_PAIRS, _hip.GR_OVERLAP_STAT_VERTICAL,
            _hip.GR_OVERLAP_STAT_RINGS_IGNORED, _hip.GR_OVERLAP_STAT_LARGEST_RING, _hip.GR_OVERLAP_STAT_BAD_ITEMS, _hip.GR_OVERLAP_STAT_WORDS,
            _hip.GR_OVERLAP_ITEM_INTS, _hip.GR_OVERLAP_TILE_A, _hip.GR_OVERLAP_TILE_B) == (0, 1, 2, 3, 4, 5, 6, 8, 5, 256, 4096)
    assert ov.STAT_WORDS == _hip.GR_OVERLAP_STAT_WORDS and ov.OVERLAP_BOUND_K == gs.OVERLAP_BOUND_K
    assert callable(_hip.HipRaster.polygon_overlap) and callable(_hip.PolygonOverlap.pairs) and callable(_hip.PolygonOverlap.areas)
    import inspect

    assert '"geograster_overlap.h"' in inspect.getsource(build._newest_header)
    # a unit of its own; the A2 predicate stands once and both phases of the join call it; no floating-point atomic
    assert any(p.name == "overlap.hip" for p in build.SOURCES)
    source = (ROOT / "geograypher_amd" / "csrc" / "overlap.hip").read_text()
    code = "\n".join(line.split("//")[0] for line in source.splitlines())
    assert code.count("bool boxes_pair(") == 1 and code.count("boxes_pair(box,") == 2
    for name in declared:
        assert re.search(rf"\bint {name}\(gr_ctx \*c,", source)
    assert not re.search(r"atomic\w*\(\s*&?(area|partial|wsum)", code) and "unsafeAtomicAdd" not in code
    assert "-ffp-contract=off" in build.HIPCC_FLAGS
    for name in declared:   # no context: GR_EINVAL before anything else
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_int, _hip._OVERLAP_SIGNATURES[name]
        assert fn(*[None if t is ctypes.c_void_p else 0 for t in fn.argtypes]) == _hip.GR_EINVAL


# -- the host layers through the stand-in backend ----------------------------------------------------------------------------------------------
def write_geojson(path, features, epsg=None):
    """features: (properties, [ring, ...]) -- a Polygon with holes."""
    out = []
    for properties, rings in features:
        coords = [[[float(x), float(y)] for x, y in list(ring) + [ring[0]]] for ring in rings]
        out.append({"type": "Feature", "properties": properties, "geometry": {"type": "Polygon", "coordinates": coords}})
    data = {"type": "FeatureCollection", "features": out}
    if epsg is not None:
        data["crs"] = {"type": "name", "properties": {"name": f"urn:ogc:def:crs:EPSG::{epsg}"}}
    path.write_text(json.dumps(data))
    return path


def utm(ring):
    return [(x + ov.SHIFT[0], y + ov.SHIFT[1]) for x, y in ring]


def test_polygon_overlap_areas_matrix():
    A = ov.polygons_of([ov.HOLED, [ov.square(10, 10, 12, 12)], [ov.square(4, 0, 6, 4)]], ov.SHIFT)
    B = ov.polygons_of([[ov.square(2, 2, 6, 6)], [ov.square(1.5, 1.5, 2.5, 2.5)], [ov.wavy_ring(90, (2.0, 2.0), 0.9)]], ov.SHIFT)
    backend = ov.StandInBackend()
    matrix = gs.polygon_overlap_areas(A, B, backend=backend)
    assert matrix.shape == (3, 3) and matrix.dtype == np.float64
    dense = matrix.toarray()
    # row 1 of B lies in the hole, the wavy ring of radius <= 0.9 about (2, 2) too: no entry, not a zero entry; row 2 of A shares an edge with row 0
    # of B over x in [4, 6]: area 4
    assert sorted(zip(*matrix.nonzero())) == [(0, 0), (2, 0)] and dense[0, 0] == pytest.approx(3.0, abs=1e-9) and dense[2, 0] == pytest.approx(4.0, abs=1e-9)
    # the table with the longer rows goes to the lane side: B here (its rows are longer), so no swap; swapped the other way round
    assert [len(t.table_b[0]) > len(t.table_a[0]) for t in backend.overlaps] == [True]
    transposed = gs.polygon_overlap_areas(B, A, backend=backend)
    assert len(backend.overlaps[-1].table_b[0]) > len(backend.overlaps[-1].table_a[0])
    assert np.array_equal(transposed.toarray(), dense.T)
    A.epsg, B.epsg = 32610, 32611
    with pytest.raises(ValueError, match="EPSG:32610 and EPSG:32611"):
        gs.polygon_overlap_areas(A, B, backend=backend)
    empty = PlanarPolygons([], [], [], n_polygons=2)
    assert gs.polygon_overlap_areas(empty, PlanarPolygons([], [], []), backend=backend).shape == (2, 0)


def test_get_overlap_vector(tmp_path):
    crowns = write_geojson(tmp_path / "crowns.geojson", [({"id": 0}, [utm(ov.square(0, 0, 2, 2))]), ({"id": 1}, [utm(ov.square(20, 20, 21, 21))]),
                                                          ({"id": 2}, [utm(ov.square(3, 0, 5, 2))]), ({"id": 3}, [utm(ov.square(6, 0, 7, 1))])], epsg=32610)
    classes = write_geojson(tmp_path / "classes.geojson", [({"names": "pine"}, [utm(ov.square(1, 0, 4, 2))]), ({"names": "fir"}, [utm(ov.square(4, 0, 6, 2))]),
                                                           ({"names": "pine"}, [utm(ov.square(0, 1, 1, 3))]), ({"names": "oak"}, [utm(ov.square(30, 30, 31, 31))])],
                            epsg=32610)
    backend = ov.StandInBackend()
    counts, ids, names = gs.get_overlap_vector(crowns, classes, "names", backend=backend)
    assert names == ["fir", "oak", "pine"] and ids.tolist() == [0, 2]          # crown 1 meets nothing, crown 3 only touches fir
    assert counts.shape == (2, 3) and np.allclose(counts, [[0, 0, 2 + 1], [2, 0, 2]], atol=1e-9, rtol=0)
    normalised, ids_2, _ = gs.get_overlap_vector(crowns, classes, "names", normalize=True, backend=backend)
    assert np.allclose(normalised, [[0, 0, 1], [0.5, 0, 0.5]], atol=1e-12) and ids_2.tolist() == [0, 2]
    # the (PlanarPolygons, {column: values}) form of both sources
    A, _ = PlanarPolygons.from_geojson(crowns)
    B, props = PlanarPolygons.from_geojson(classes)
    again, ids_3, names_3 = gs.get_overlap_vector((A, {}), (B, {"names": list(props["names"])}), "names", backend=backend)
    assert np.array_equal(again, counts) and ids_3.tolist() == [0, 2] and names_3 == names
    with pytest.raises(ValueError, match="Class column `species` not in"):
        gs.get_overlap_vector(crowns, classes, "species", backend=backend)
    other = write_geojson(tmp_path / "other.geojson", [({"names": "pine"}, [utm(ov.square(1, 0, 4, 2))])], epsg=32611)
    with pytest.raises(ValueError, match="get_overlap_vector: the two sources are in EPSG:32610 and EPSG:32611"):
        gs.get_overlap_vector(crowns, other, "names", backend=backend)
    with pytest.raises(NotImplementedError, match="geojson only"):
        gs.get_overlap_vector(tmp_path / "crowns.shp", classes, "names", backend=backend)


def test_cf_from_vector_vector(tmp_path):
    true = write_geojson(tmp_path / "true.geojson", [({"cls": "a"}, [utm(ov.square(0, 0, 4, 4))]), ({"cls": "b"}, [utm(ov.square(4, 0, 8, 4)), utm(ov.square(5, 1, 6, 2))]),
                                                      ({"cls": "a"}, [utm(ov.square(0, 4, 4, 6))]), ({"cls": "c"}, [utm(ov.square(20, 0, 22, 2))])], epsg=32610)
    pred = write_geojson(tmp_path / "pred.geojson", [({"cls": "a"}, [utm(ov.square(0, 0, 5, 5))]), ({"cls": "b"}, [utm(ov.square(5, 0, 9, 3))]),
                                                      ({"cls": "d"}, [utm(ov.square(20, 0, 21, 1))])], epsg=32610)
    backend = ov.StandInBackend()
    cf, values = cf_from_vector_vector(pred, true, "cls", backend=backend)
    assert values == ["a", "b", "c"] and cf.shape == (4, 4)
    # true a = 16 + 8: pred a covers 16 + 4; true b = 16 - 1 (a hole): pred a covers x in [4, 5], y in [0, 4] = 4; pred b covers
    # [5, 8] x [0, 3] = 9 minus the hole = 8; true c is absent from the prediction (its only cover, d, is no column): all unlabeled
    want = np.array([[20, 0, 0, 4], [4, 8, 0, 3], [0, 0, 0, 4], [0, 0, 0, 0]], dtype=np.float64)
    assert np.allclose(cf, want, atol=1e-9, rtol=0)
    plain, _ = cf_from_vector_vector(pred, true, "cls", include_unlabeled_class=False, backend=backend)
    assert np.allclose(plain, want[:3, :3], atol=1e-9, rtol=0)
    chosen, values = cf_from_vector_vector(pred, true, "cls", column_values=["b", "d"], backend=backend)
    assert values == ["b", "d"] and np.allclose(chosen, [[8, 0, 7], [0, 0, 0], [0, 0, 0]], atol=1e-9, rtol=0)
    # rows of one class that overlap each other: summing them is no dissolve
    twice = write_geojson(tmp_path / "twice.geojson", [({"cls": "a"}, [utm(ov.square(0, 0, 4, 4))]), ({"cls": "b"}, [utm(ov.square(1, 1, 3, 3))]),
                                                        ({"cls": "a"}, [utm(ov.square(3, 3, 5, 5))])], epsg=32610)
    with pytest.raises(ValueError, match=r"rows 0 and 2 of the predicted map are both 'a' and overlap by 1 m\^2: dissolve"):
        cf_from_vector_vector(twice, true, "cls", backend=backend)
    with pytest.raises(ValueError, match="rows 0 and 2 of the true map"):
        cf_from_vector_vector(pred, twice, "cls", backend=backend)
    # rows of one class that share an edge (true a above) are fine; another CRS is refused; a missing column too
    other = write_geojson(tmp_path / "other.geojson", [({"cls": "a"}, [utm(ov.square(0, 0, 5, 5))])], epsg=32611)
    with pytest.raises(ValueError, match="cf_from_vector_vector: the two sources are in EPSG:32611 and EPSG:32610"):
        cf_from_vector_vector(other, true, "cls", backend=backend)
    with pytest.raises(ValueError, match="the predicted map has no property 'kind'"):
        cf_from_vector_vector(pred, true, "kind", backend=backend)
    from geograypher_amd.utils.prediction_metrics import compute_confusion_matrix_from_geospatial

    with pytest.raises(NotImplementedError, match="vector prediction.*cf_from_vector_vector"):
        compute_confusion_matrix_from_geospatial(pred, true, ["a", "b"], backend=backend)


# -- the bound (A6) ------------------------------------------------------------------------------------------------------------------------------
def test_the_bound_is_measured(capsys):
    """r = |numpy restatement - exact| / (2^-53 area_abs) over every candidate pair of every scene the GPU tests use, at the local
    origin and shifted to UTM-sized coordinates.  K is 4 x the largest r rounded up to a power of two: the device differs from the
    restatement only in the order of its sum."""
    worst = (0.0, None)
    for name in ov.SCENES:
        for shifted in (False, True):
            table_a, table_b, pairs = ov.scene_tables(name, shifted)
            if not len(pairs):
                continue
            assert ov.far_from_every_bound(name, shifted), (name, shifted)
            exact, exact_abs, stats = ov.scene_exact(name, shifted)
            restated, restated_abs, stats_2 = ov.restated_areas(table_a, table_b, pairs)
            assert np.array_equal(stats, stats_2)
            for k in range(len(pairs)):
                if restated_abs[k] == 0:
                    assert exact[k] == 0 and restated[k] == 0
                    continue
                error = abs(Fraction(float(restated[k])) - Fraction(exact[k], 1 << ov.FIXED_BITS))
                r = float(error / (Fraction(float(restated_abs[k])) / (1 << 53)))
                if r > worst[0]:
                    worst = (r, (name, shifted, tuple(pairs[k]), int(stats[2])))
    with capsys.disabled():
        print(f"\nlargest r = {worst[0]:.3f} at {worst[1]}")
    assert worst[0] > 0
    assert 2.0 ** math.ceil(math.log2(4 * worst[0])) == ov.OVERLAP_BOUND_K, worst
    assert worst[1][0] == ov.BOUND_SCENE
