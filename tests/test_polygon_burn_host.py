"""The polygon burn without a GPU: the stand-in the GPU tests compare the device with on hand-worked 4 x 4
cases; the work items of a window against a brute-force listing; the refusals of the table checks; the companion header against
the binding and the library; `burn_polygons`, the labelled chips of `write_chips` and its ROI filter through the stand-in backend."""
import ctypes
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import burn_standin as bs  # noqa: E402
import crs_standin as cs  # noqa: E402
from geograypher_amd import _hip, build  # noqa: E402
from geograypher_amd.constants import NULL_TEXTURE_INT_VALUE  # noqa: E402
from geograypher_amd.predictors import ortho_segmentor as og  # noqa: E402
from geograypher_amd.utils.geometric import (PlanarPolygons, burn_work_items, rectangle_meets_rows, ring_edges, row_centre_boxes,  # noqa: E402
                                             row_ring_ranges)
from geograypher_amd.utils.geospatial import burn_polygons, burn_values, rings_to_cell_units  # noqa: E402
from geograypher_amd.utils.raster import PlanarRaster, invert_affine  # noqa: E402
from geograypher_amd.utils.tiff import write_tiff_deflate  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def square(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def q(ring):
    return [(int(round(x * 65536)), int(round(y * 65536))) for x, y in ring]


# -- the stand-in by hand: unit cells, the centre of cell (row, col) is (col + 0.5, row + 0.5) ----------------------------------------
def test_stand_in_by_hand():
    window = (0, 0, 4, 4)
    # a plain square over the centres 1.5 and 2.5 on both axes
    rows, out, stats = bs.burn([q(square(1, 1, 3, 3))], [0], 1, window, values=[7], fill=255)
    assert rows.tolist() == [[-1, -1, -1, -1], [-1, 0, 0, -1], [-1, 0, 0, -1], [-1, -1, -1, -1]]
    assert out.tolist() == [[255, 255, 255, 255], [255, 7, 7, 255], [255, 7, 7, 255], [255, 255, 255, 255]]
    assert stats.tolist() == [0, 4, 4, 4, 0, 0, 0, 0]
    # two overlapping squares: row 0 holds the centres 0.5 .. 2.5, row 1 the centres 1.5 .. 3.5; where both do, row 1 stays
    both = [q(square(0, 0, 3, 3)), q(square(1, 1, 4, 4))]
    rows, out, stats = bs.burn(both, [0, 1], 2, window, values=[7, 9], fill=0)
    assert rows.tolist() == [[0, 0, 0, -1], [0, 1, 1, 1], [0, 1, 1, 1], [-1, 1, 1, 1]]
    assert out.tolist() == [[7, 7, 7, 0], [7, 9, 9, 9], [7, 9, 9, 9], [0, 9, 9, 9]]
    assert stats[1] == 18 and stats[2] == 14          # 9 + 9 memberships, 4 cells twice
    # a square through cell centres: the centres on its left and top edge are in, on its right and bottom edge out
    for ring in (square(0.5, 0.5, 2.5, 2.5), square(0.5, 0.5, 2.5, 2.5)[::-1]):
        rows, _, _ = bs.burn([q(ring)], [0], 1, window)
        assert rows.tolist() == [[0, 0, -1, -1], [0, 0, -1, -1], [-1, -1, -1, -1], [-1, -1, -1, -1]]
    # a hole: even-odd over all rings of the row
    rows, _, stats = bs.burn([q(square(0, 0, 4, 4)), q(square(1, 1, 3, 3))], [0, 0], 1, window)
    assert rows.tolist() == [[0, 0, 0, 0], [0, -1, -1, 0], [0, -1, -1, 0], [0, 0, 0, 0]] and stats[1] == 12
    # a two-part row behind a row without rings, and a ring of two vertices (ignored and counted)
    rows, out, stats = bs.burn([q(square(0, 0, 1, 1)), q(square(3, 3, 4, 4)), q([(0.0, 0.0), (4.0, 4.0)])], [1, 1, 1], 2, window, values=[3, 5])
    assert rows.tolist() == [[1, -1, -1, -1], [-1, -1, -1, -1], [-1, -1, -1, -1], [-1, -1, -1, 1]]
    assert out[0, 0] == 5 and out[1, 1] == 255 and stats.tolist() == [0, 2, 2, 4, 1, 0, 0, 0]
    # B1: a window is a part of the parent grid, and may leave it on any side
    rows, _, _ = bs.burn(both, [0, 1], 2, (-1, 2, 3, 4))
    assert rows.tolist() == [[-1, 0, 1], [-1, -1, 1], [-1, -1, -1], [-1, -1, -1]]
    # without values there is no value pass: the burned-cells word stays 0
    assert bs.burn(both, [0, 1], 2, window)[1] is None and bs.burn(both, [0, 1], 2, window)[2][2] == 0


# -- work items ---------------------------------------------------------------------------------------------------------------------
def table(rings, rows, transform=IDENTITY):
    rv, off = rings_to_cell_units([np.asarray(r, dtype=np.float64) for r in rings], invert_affine(transform))
    return rv, off, np.asarray(rows, dtype=np.int32)


def test_centre_boxes_by_hand():
    rv, off, rp = table([square(1, 1, 3, 3), square(0.5, 0.5, 2.5, 2.5), square(-3.2, -7.5, -1.6, -6.4), square(0.6, 0.6, 0.9, 0.9),
                         [(0.0, 0.0), (9.0, 9.0)]], [0, 1, 2, 3, 5])
    boxes = row_centre_boxes(rv, off, rp, 6)
    # centres c + 0.5 inside [lo, hi]: [1, 3] -> 1, 2; [0.5, 2.5] -> 0 .. 2 (the box is closed: Z3 decides the far edge);
    # [-3.2, -1.6] -> -3 alone (-1.5 lies outside) and [-7.5, -6.4] -> -8, -7; [0.6, 0.9] holds none; row 4 has no ring, row 5 only a 2-vertex ring
    assert boxes.tolist() == [[1, 1, 2, 2], [0, 0, 2, 2], [-3, -8, -3, -7], [1, 1, 0, 0], [1, 1, 0, 0], [1, 1, 0, 0]]
    assert row_ring_ranges(rp, 6).tolist() == [[0, 1], [1, 2], [2, 3], [3, 4], [4, 4], [4, 5]]


@pytest.mark.parametrize("block", [(64, 128), (7, 3), (1, 1)])
def test_work_items_against_a_brute_force_listing(block):
    rng = np.random.default_rng(3)
    lo = rng.integers(-40, 200, (30, 2))
    size = rng.integers(0, 150, (30, 2))
    boxes = np.concatenate([lo, lo + size], axis=1).astype(np.int64)
    boxes[5] = boxes[17] = (1, 1, 0, 0)                       # rows that hold no centre
    ranges = np.stack([np.arange(30) * 2, np.arange(30) * 2 + 2], axis=1)
    seen_inside = seen_straddling = seen_outside = 0
    for window in ((0, 0, 97, 131), (-50, -50, 400, 500), (30, 40, 1, 1), (150, -20, 64, 40), (1000, 1000, 5, 5), (-9, 100, 20, 3)):
        col_off, row_off, width, height = window
        items = burn_work_items(boxes, ranges, window, block)
        assert items.dtype == np.int32 and items.shape[1] == 7
        _hip.check_burn_window(col_off, row_off, width, height, items, 30, 60)
        covered = {}
        for p, c0, r0, w, h, first, last in items.tolist():
            assert 1 <= w <= block[0] and 1 <= h <= block[1] and (first, last) == (2 * p, 2 * p + 2)
            cells = covered.setdefault(p, set())
            block_cells = {(r, c) for r in range(r0, r0 + h) for c in range(c0, c0 + w)}
            assert not cells & block_cells, "the blocks of a row overlap"
            cells |= block_cells
        for p, (c0, r0, c1, r1) in enumerate(boxes.tolist()):
            want = {(r, c) for r in range(max(r0, row_off), min(r1, row_off + height - 1) + 1)
                    for c in range(max(c0, col_off), min(c1, col_off + width - 1) + 1)}
            assert covered.get(p, set()) == want, (window, p)
            box = (c1 - c0 + 1) * (r1 - r0 + 1) if c0 <= c1 else 0
            seen_inside += bool(want) and len(want) == box
            seen_straddling += 0 < len(want) < box
            seen_outside += box > 0 and not want
    assert seen_inside and seen_straddling and seen_outside
    with pytest.raises(ValueError, match="at most 64 x 128"):
        burn_work_items(boxes, ranges, (0, 0, 4, 4), (65, 1))


# -- refusals of the table checks -------------------------------------------------------------------------------------------------------
def test_malformed_tables_are_refused():
    rv, off, rp = table([square(1, 1, 8, 8), square(2, 2, 3, 3)], [0, 1])
    assert _hip.check_burn_tables(rv, off, rp, 2, np.array([1, 2])) == 2
    for bad in (dict(rv=rv.astype(np.float64)), dict(rv=rv.reshape(-1)), dict(rv=rv * (1 << 30)), dict(off=off[:-1]), dict(off=off[::-1].copy()),
                dict(off=np.array([0, 4, 7])), dict(rp=np.array([1, 0])), dict(rp=np.array([0, 2])), dict(rp=np.array([-1, 0])), dict(P=-1),
                dict(values=np.array([1])), dict(values=np.array([1, 256])), dict(values=np.array([-1, 0])), dict(values=np.array([0.5, 1.0]))):
        a = dict(rv=rv, off=off, rp=rp, P=2, values=np.array([1, 2]))
        a.update(bad)
        with pytest.raises(ValueError, match="gr_burn_polygons"):
            _hip.check_burn_tables(a["rv"], a["off"], a["rp"], a["P"], a["values"])
    good = np.array([[0, 2, 3, 4, 5, 0, 1]], dtype=np.int32)
    _hip.check_burn_window(2, 3, 4, 5, good, 2, 2)
    _hip.check_burn_window(-(1 << 23) + 1, 0, 1, (1 << 23), good[:0], 2, 2)
    for window in ((2, 3, 0, 5), (2, 3, 4, 0), (1 << 23, 0, 1, 1), (-(1 << 23), 0, 1, 1), (0, 1, 1, 1 << 23), ((1 << 23) - 1, 0, 2, 1)):
        with pytest.raises(ValueError, match="gr_burn_polygons: a window"):
            _hip.check_burn_window(*window, good[:0], 2, 2)
    for item in ([0, 1, 3, 4, 5, 0, 1], [0, 2, 2, 4, 5, 0, 1], [0, 2, 3, 5, 5, 0, 1], [0, 2, 3, 4, 6, 0, 1], [2, 2, 3, 4, 5, 0, 1], [-1, 2, 3, 4, 5, 0, 1],
                 [0, 2, 3, 0, 5, 0, 1], [0, 2, 3, 4, 5, 0, 3], [0, 2, 3, 4, 5, 1, 0], [0, 2, 3, 4, 5, -1, 1]):
        with pytest.raises(ValueError, match="gr_burn_polygons: work item 0"):
            _hip.check_burn_window(2, 3, 4, 5, np.array([item], dtype=np.int32), 2, 2)
    with pytest.raises(ValueError, match="gr_burn_polygons: work item 0"):
        _hip.check_burn_window(0, 0, 100, 200, np.array([[0, 0, 0, 65, 1, 0, 1]], dtype=np.int32), 2, 2)
    with pytest.raises(ValueError, match="gr_burn_polygons: work items"):
        _hip.check_burn_window(2, 3, 4, 5, np.zeros((1, 6), dtype=np.int32), 2, 2)
    with pytest.raises(ValueError, match="fill=256"):
        _hip.check_burn_window(2, 3, 4, 5, good, 2, 2, fill=256)
    with pytest.raises(ValueError, match="not an integer in"):
        burn_values([1, 2.5], 2)
    with pytest.raises(ValueError, match="not an integer in"):
        burn_values([1, "a"], 2)
    with pytest.raises(ValueError, match="as many values"):
        burn_values([1], 2)
    assert burn_values([0, 255.0, np.int64(7)], 3).tolist() == [0, 255, 7]


# -- one ring-table check, one cell-item check behind the four table checks ------------------------------------------------------------
LIMIT = 1 << 40
RING_TABLE = dict(rv=np.array(q(square(1, 1, 8, 8)) + q(square(2, 2, 3, 3)), dtype=np.int64), off=np.array([0, 4, 8]), rp=np.array([0, 1]), P=2)
WIDE_BOXES = np.array([[-LIMIT, -LIMIT, LIMIT, LIMIT]] * 2, dtype=np.int64)      # they hold every vertex a table may have


def at(value):
    rv = RING_TABLE["rv"].copy()
    rv[5, 1] = value
    return rv


RING_TABLE_CHECKS = {
    "gr_zonal_class_counts": lambda rv, off, rp, P: _hip.check_zonal_tables(9, 9, None, rv, off, rp, P, np.zeros((0, 7), dtype=np.int32), 3),
    "gr_burn_polygons": lambda rv, off, rp, P: _hip.check_burn_tables(rv, off, rp, P),
    "gr_polygon_overlap_areas": lambda rv, off, rp, P: _hip.check_overlap_tables((rv, off, rp, np.zeros(len(rp), dtype=np.int32), WIDE_BOXES[:P]),
                                                                                   (RING_TABLE["rv"], RING_TABLE["off"], RING_TABLE["rp"],
                                                                                    np.zeros(2, dtype=np.int32), WIDE_BOXES)),
    "gr_simplify_rings": lambda rv, off, rp, P: _hip.check_simplify_tables(rv, off, 0.5),
}
# (what is wrong, the change, refused by the checks that take no ring_polygon too, accepted by those whose limit is inclusive)
BAD_RING_TABLES = [
    ("offsets do not start at 0", dict(off=np.array([1, 4, 8])), True, False),
    ("offsets fall", dict(off=np.array([0, 9, 8])), True, False),
    ("offsets do not end at N", dict(off=np.array([0, 4, 7])), True, False),
    ("ring_polygon falls", dict(rp=np.array([1, 0])), False, False),
    ("ring_polygon names row P", dict(rp=np.array([0, 2])), False, False),
    ("ring_polygon names row -1", dict(rp=np.array([-1, 0])), False, False),
    ("vertices are flat", dict(rv=RING_TABLE["rv"].reshape(-1)), True, False),
    ("vertices are (N, 3)", dict(rv=np.zeros((8, 3), dtype=np.int64)), True, False),
    ("vertices are floats", dict(rv=RING_TABLE["rv"].astype(np.float64)), True, False),
    ("a coordinate at the limit", dict(rv=at(LIMIT)), True, True),
    ("a coordinate at minus the limit", dict(rv=at(-LIMIT)), True, True),
    ("a coordinate past the limit", dict(rv=at(LIMIT + 1)), True, False),
    ("a coordinate past minus the limit", dict(rv=at(-LIMIT - 1)), True, False),
]


@pytest.mark.parametrize("name", list(RING_TABLE_CHECKS))
@pytest.mark.parametrize("what, change, without_rows, at_the_limit", BAD_RING_TABLES, ids=[b[0] for b in BAD_RING_TABLES])
def test_one_list_of_malformed_ring_tables_for_the_four_checks(name, what, change, without_rows, at_the_limit):
    """Every check refuses the same tables under its own name; the ONE intended difference: at exactly 2^40 the tables in cell
    units (zonal counts, burn) are refused, the snapped tables of the 1e-6 m grid (overlap, simplify) are accepted."""
    check = RING_TABLE_CHECKS[name]
    check(**RING_TABLE)                                                             # the table itself is fine
    assert _hip.SIMPLIFY_COORD_LIMIT == _hip.OVERLAP_COORD_LIMIT == LIMIT
    inclusive = name in ("gr_polygon_overlap_areas", "gr_simplify_rings")
    if (name == "gr_simplify_rings" and not without_rows) or (at_the_limit and inclusive):
        check(**{**RING_TABLE, **change})
        return
    with pytest.raises(ValueError, match=f"^{name}: "):
        check(**{**RING_TABLE, **change})


BAD_CELL_ITEMS = {"p = P": [2, 0, 0, 1, 1, 0, 1], "p = -1": [-1, 0, 0, 1, 1, 0, 1], "no column": [0, 0, 0, 0, 1, 0, 1], "no row": [0, 0, 0, 1, 0, 0, 1],
                  "a negative side": [0, 5, 5, -1, 1, 0, 1], "65 columns": [0, 0, 0, 65, 1, 0, 1], "129 rows": [0, 0, 0, 1, 129, 0, 1],
                  "a cell left of the window": [0, -1, 0, 2, 1, 0, 1], "a cell above it": [0, 0, -1, 1, 2, 0, 1],
                  "a cell right of it": [0, 98, 0, 3, 1, 0, 1], "a cell below it": [0, 0, 197, 1, 4, 0, 1], "hi < lo": [0, 0, 0, 1, 1, 1, 0],
                  "hi > R": [0, 0, 0, 1, 1, 0, 3], "lo < 0": [0, 0, 0, 1, 1, -1, 1]}


@pytest.mark.parametrize("bad", list(BAD_CELL_ITEMS.values()), ids=list(BAD_CELL_ITEMS))
def test_one_list_of_malformed_cell_items_for_the_zonal_counts_and_the_burn(bad):
    """The zonal counts check their items against the window (0, 0, W, H); the burn, given that window, refuses the same items
    and both name the first bad one."""
    W, H = 100, 200
    good = [[1, 36, 72, 64, 128, 0, 2], [0, 99, 199, 1, 1, 2, 2]]
    rv, off, rp = RING_TABLE["rv"], RING_TABLE["off"], RING_TABLE["rp"]
    said = []
    for items in (good, good + [bad, bad]):
        items = np.array(items, dtype=np.int32)
        for name, check in (("gr_zonal_class_counts", lambda: _hip.check_zonal_tables(H, W, None, rv, off, rp, 2, items, 3)),
                            ("gr_burn_polygons", lambda: _hip.check_burn_window(0, 0, W, H, items, 2, 2))):
            if len(items) == 2:
                check()
                continue
            with pytest.raises(ValueError, match=f"^{name}: work item 2 ") as refusal:
                check()
            said.append(re.search(r"work item 2 (\(.*?\)) names no polygon row, no block of at most 64 x 128 cells", str(refusal.value)).group(1))
    assert said == [str(tuple(bad))] * 2


# -- the companion header -----------------------------------------------------------------------------------------------------------------
def test_companion_header_binding_and_library_agree():
    main = (ROOT / "include" / "geograster.h").read_text()
    assert re.search(r'^#include "geograster_burn.h"$', main, re.M) and main.index("geograster_burn.h") < main.rindex("#ifdef __cplusplus")
    assert main.index('#include "geograster_decimate.h"') < main.index('#include "geograster_burn.h"') and "#define GR_VERSION 126" in main
    assert not re.search(r"gr_burn_polygons\s*\(", main)
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", (ROOT / "include" / "geograster_burn.h").read_text(), flags=re.S)
    declared = {name: [a.strip() for a in " ".join(args.split()).split(",")]
                for name, args in re.findall(r"\b(gr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}
    assert sorted(declared) == sorted(_hip._BURN_SIGNATURES) == sorted(_hip.BURN_SYMBOLS) == ["gr_burn_polygons"]
    others = set(_hip._SIGNATURES) | set(_hip._COMPANION_SIGNATURES) | set(_hip._ORTHO_SIGNATURES) | set(_hip._DECIMATE_SIGNATURES)
    assert not set(declared) & others
    kinds = {ctypes.c_int64: "int64", ctypes.c_int: "int", ctypes.c_int32: "int", ctypes.c_double: "double"}
    lib = ctypes.CDLL(str(build.build()))
    for name, arguments in declared.items():
        argtypes = _hip._BURN_SIGNATURES[name]
        assert len(arguments) == len(argtypes) == 19 and hasattr(lib, name), name
        for argument, ctype in zip(arguments, argtypes):
            want = "pointer" if "*" in argument else {"int64_t": "int64", "int32_t": "int", "int": "int", "double": "double"}[argument.split()[0]]
            got = "pointer" if ctype is ctypes.c_void_p or issubclass(ctype, ctypes._Pointer) else kinds[ctype]
            assert want == got, f"{name}: {argument!r} is bound as {ctype.__name__}"
    assert (_hip.GR_BURN_STAT_TESTED, _hip.GR_BURN_STAT_INSIDE, _hip.GR_BURN_STAT_BURNED, _hip.GR_BURN_STAT_LARGEST_RING,
            _hip.GR_BURN_STAT_RINGS_IGNORED, _hip.GR_BURN_STAT_WORDS) == (0, 1, 2, 3, 4, 8)
    assert callable(_hip.HipRaster.polygon_burner) and callable(_hip.PolygonBurner.window)
    # the header is a build input: touching it makes the library stale
    import inspect

    assert '"geograster_burn.h"' in inspect.getsource(build._newest_header)
    # one ring walk: both kernels call it, and the nest stands once in the unit; the burn kernels are integer only
    source = (ROOT / "geograypher_amd" / "csrc" / "ortho.hip").read_text()
    assert source.count("zonal_parity_walk(") == 3 and source.count("edge_crossing_strict(vx[j]") == 1
    # ... and Z3, the slot search and the device ring table are DEFINED once, in the shared header; the units only call them
    units = {p.name: p.read_text() for p in build.SOURCES + build.HEADERS}
    for pattern in (r"\bvoid edge_crossing_strict\(", r"\bint64_t ring_of_slot\(", r"\bstruct RingTable\b(?! \*)"):
        assert [name for name, text in units.items() if re.search(pattern, text)] == ["geom_dev.hpp"], pattern
        assert len(re.findall(pattern, units["geom_dev.hpp"])) == 1, pattern
    for unit, calls in (("ortho.hip", ("edge_crossing_strict(",)), ("nadir.hip", ("edge_crossing_strict<NARROW>(",)),
                        ("overlap.hip", ("ring_of_slot(", "RingTable")), ("simplify.hip", ("ring_of_slot(",))):
        assert all(call in units[unit] for call in calls) and "dev_ceil_div" not in units[unit], unit
    burn = source[source.index("void k_burn_rows("):source.index("}  // namespace")]
    assert not re.search(r"\b(double|float)\b", burn) and burn.count("atomicMax(") == 1
    fn = lib.gr_burn_polygons
    fn.restype, fn.argtypes = ctypes.c_int, _hip._BURN_SIGNATURES["gr_burn_polygons"]
    assert fn(None, None, 0, None, None, 0, 0, None, None, 0, 0, 0, 1, 1, 255, None, None, None, None) == _hip.GR_EINVAL   # no context


# -- burn_polygons through the stand-in backend -----------------------------------------------------------------------------------------------
TRANSFORM = (0.5, 0.0, 600000.0, 0.0, -0.5, 4200000.0)      # half-metre cells, north up, UTM 10 N


def world(c0, r0, c1, r1):
    return [(600000.0 + 0.5 * c, 4200000.0 - 0.5 * r) for c, r in ((c0, r0), (c1, r0), (c1, r1), (c0, r1))]


def expected_label(rings, ring_rows, P, values, window, fill, transform=TRANSFORM):
    rings_q = bs.to_cell_units([np.asarray(r) for r in rings], invert_affine(transform))
    return bs.burn(rings_q, ring_rows, P, window, values, fill)


def test_burn_polygons_banded_equals_one_band(tmp_path):
    rings = [world(1.2, 0.7, 9.4, 8.8), world(5.1, 3.3, 20.0, 6.6), world(3.0, 2.0, 7.0, 5.0), world(-4, 7.6, 30, 9.2)]
    polygons = PlanarPolygons(rings, [0, 1, 1, 2], [False, False, False, False], n_polygons=4)      # row 3 has no ring
    like = PlanarRaster(np.zeros((10, 14)), TRANSFORM, epsg=32610)
    backend = bs.StandInBackend()
    whole = burn_polygons(polygons, [10, 20, 30, 40], like, fill=255, backend=backend)
    assert whole.dtype == np.uint8 and whole.shape == (10, 14) and backend.burners[-1].windows == [(0, 0, 14, 10)]
    want_rows, want, _ = expected_label(polygons.rings, polygons.ring_polygon.tolist(), 4, [10, 20, 30, 40], (0, 0, 14, 10), 255)
    assert np.array_equal(whole, want) and {10, 20, 30, 255} == set(np.unique(whole).tolist())
    banded = burn_polygons(polygons, [10, 20, 30, 40], like, fill=255, backend=backend, max_device_bytes=3 * 5 * 14)   # 3 rows a band
    assert backend.burners[-1].windows == [(0, 0, 14, 3), (0, 3, 14, 3), (0, 6, 14, 3), (0, 9, 14, 1)] and np.array_equal(banded, whole)
    rows = burn_polygons(polygons, None, like, backend=backend, rows=True, max_device_bytes=1)                     # one row a band
    assert rows.dtype == np.int32 and np.array_equal(rows, want_rows) and len(backend.burners[-1].windows) == 10
    # the other forms of the arguments: ring arrays and ((H, W), transform); a GeoTIFF path, of which only the header is read
    again = burn_polygons([np.array(rings[0]), [np.array(rings[1]), np.array(rings[2])], np.array(rings[3])], [10, 20, 30],
                          ((10, 14), TRANSFORM), backend=backend, rows=True)
    assert np.array_equal(again, want_rows)
    write_tiff_deflate(tmp_path / "rgb.tif", np.zeros((10, 14, 3), np.uint8), transform=TRANSFORM, epsg=32610)
    assert np.array_equal(burn_polygons(polygons, [10, 20, 30, 40], tmp_path / "rgb.tif", backend=backend), whole)
    with pytest.raises(ValueError, match="not an integer in"):
        burn_polygons(polygons, [10, 20, 300, 40], like, backend=backend)
    with pytest.raises(ValueError, match="fill=256"):
        burn_polygons(polygons, [10, 20, 30, 40], like, fill=256, backend=backend)
    polygons.epsg = 26910                                     # NAD83: another datum
    with pytest.raises(NotImplementedError, match="26910"):
        burn_polygons(polygons, [10, 20, 30, 40], like, backend=backend)


# -- write_chips: labelled chips ------------------------------------------------------------------------------------------------------------------
def write_geojson(path, features, epsg=None, to_lon_lat=False):
    """features: (properties, [ring, ...]) -- a Polygon with holes; `to_lon_lat`: the UTM 10 N vertices are written as EPSG:4326."""
    out = []
    for properties, rings in features:
        coords = []
        for ring in rings:
            ring = np.asarray(list(ring) + [ring[0]], dtype=np.float64)
            if to_lon_lat:
                points = np.column_stack([ring, np.zeros(len(ring))])
                ring = cs.CrsStandinBackend().reproject_points(points, 32610, 4326)[0][:, :2]
            coords.append([[float(x), float(y)] for x, y in ring])
        out.append({"type": "Feature", "properties": properties, "geometry": {"type": "Polygon", "coordinates": coords}})
    data = {"type": "FeatureCollection", "features": out}
    if epsg is not None:
        data["crs"] = {"type": "name", "properties": {"name": f"urn:ogc:def:crs:EPSG::{epsg}"}}
    path.write_text(json.dumps(data))


LABEL_RINGS = [[world(1.2, 0.7, 9.4, 8.8), world(3.1, 2.2, 5.2, 4.3)], [world(5.1, 3.3, 13.7, 6.6)], [world(11.3, 8.2, 16.9, 13.4)]]
LABEL_ROWS = [0, 0, 1, 2]
H, W, CHIP, STRIDE = 10, 14, 4, 3


@pytest.fixture()
def site(tmp_path):
    """A 10 x 14 RGB GeoTIFF and three label features: a square with a hole, a bar over it, a square over the bottom right corner
    that reaches past the raster.  20 windows of 4 every 3."""
    rgb = (np.arange(H * W * 3) % 251).astype(np.uint8).reshape(H, W, 3)
    write_tiff_deflate(tmp_path / "site.tif", rgb, transform=TRANSFORM, epsg=32610)
    features = [({"kind": "oak", "code": 3}, LABEL_RINGS[0]), ({"kind": "fir", "code": 4}, LABEL_RINGS[1]), ({"kind": "oak", "code": 3}, LABEL_RINGS[2])]
    write_geojson(tmp_path / "labels.geojson", features, epsg=32610)
    return tmp_path, rgb, features


def chip_labels(values, fill):
    rings = [ring for feature in LABEL_RINGS for ring in feature]
    return {og.get_str_from_window(w, "site.tif", ".png"): expected_label(rings, LABEL_ROWS, 3, values, tuple(w), fill)[1]
            for w in og.create_windows((H, W), CHIP, STRIDE)}


def read_png(path):
    from PIL import Image

    return np.array(Image.open(path))


def test_write_chips_with_labels(site):
    tmp_path, rgb, features = site
    backend = bs.StandInBackend()
    (tmp_path / "chips").mkdir()
    (tmp_path / "chips" / "old.txt").write_text("x")
    # label_column + label_remap, background 0: chips whose label is all 0 are skipped
    written = og.write_chips(tmp_path / "site.tif", tmp_path / "chips", CHIP, STRIDE, label_vector_file=tmp_path / "labels.geojson",
                             label_column="kind", label_remap={"oak": 1, "fir": 2}, output_suffix=".png", backend=backend)
    want = chip_labels([1, 2, 1], 0)
    assert len(want) == 20 and len(backend.burners) == 1 and len(backend.burners[0].windows) == 20      # one burner, one call per window
    kept = sorted(name for name, label in want.items() if label.any())
    assert 0 < len(kept) < 20
    assert sorted(p.name for p in (tmp_path / "chips").iterdir()) == ["anns", "imgs"]
    assert sorted(p.name for p in (tmp_path / "chips" / "anns").iterdir()) == kept == sorted(p.name for p in written)
    assert sorted(p.name for p in (tmp_path / "chips" / "imgs").iterdir()) == kept and all(p.parent.name == "imgs" for p in written)
    for name in kept:
        label = read_png(tmp_path / "chips" / "anns" / name)
        assert label.dtype == np.uint8 and label.shape == (CHIP, CHIP) and np.array_equal(label, want[name]), name
    corner = read_png(tmp_path / "chips" / "anns" / "site:12:9:4:4.png")                # past the raster on two sides: burned there too
    assert corner.tolist() == [[1, 1, 1, 1]] * 4
    image = read_png(tmp_path / "chips" / "imgs" / "site:12:9:4:4.png")
    assert image.shape == (4, 4, 3) and np.array_equal(image[:1, :2], rgb[9:, 12:]) and image[1:].sum() == 0 and image[:, 2:].sum() == 0
    assert read_png(tmp_path / "chips" / "anns" / "site:3:3:4:4.png").tolist() == want["site:3:3:4:4.png"].tolist()
    # write_empty_tiles: all 20, the empty ones all background
    written = og.write_chips(tmp_path / "site.tif", tmp_path / "chips", CHIP, STRIDE, label_vector_file=tmp_path / "labels.geojson",
                             label_column="code", write_empty_tiles=True, output_suffix=".png", backend=backend)
    want = chip_labels([3, 4, 3], 0)
    assert len(written) == 20 and all(np.array_equal(read_png(tmp_path / "chips" / "anns" / n), label) for n, label in want.items())
    # the feature number by default: feature 0 burns the value 0 = NULL_TEXTURE_INT_VALUE
    assert NULL_TEXTURE_INT_VALUE == 0
    written = og.write_chips(tmp_path / "site.tif", tmp_path / "chips", CHIP, STRIDE, label_vector_file=tmp_path / "labels.geojson",
                             output_suffix=".png", backend=backend)
    want = chip_labels([0, 1, 2], 0)
    kept = sorted(name for name, label in want.items() if label.any())
    assert sorted(p.name for p in written) == kept and all(np.array_equal(read_png(tmp_path / "chips" / "anns" / n), want[n]) for n in kept)
    # background_ind 255: the reference's test is against the constant, so only a chip that is all 0 would be skipped -- none is
    written = og.write_chips(tmp_path / "site.tif", tmp_path / "chips", CHIP, STRIDE, label_vector_file=tmp_path / "labels.geojson",
                             label_column="code", background_ind=255, output_suffix=".png", backend=backend)
    want = chip_labels([3, 4, 3], 255)
    assert len(written) == 20 and all(np.array_equal(read_png(tmp_path / "chips" / "anns" / n), label) for n, label in want.items())
    assert read_png(tmp_path / "chips" / "anns" / "site:0:0:4:4.png")[0, 0] == 255


def test_write_chips_refusals_and_values(site):
    tmp_path, _, features = site
    backend = bs.StandInBackend()
    kw = dict(label_vector_file=tmp_path / "labels.geojson", output_suffix=".png", backend=backend)
    with pytest.raises(ValueError, match="300.*not an integer in"):
        og.write_chips(tmp_path / "site.tif", tmp_path / "chips", CHIP, STRIDE, label_column="kind", label_remap={"oak": 300, "fir": 2}, **kw)
    with pytest.raises(ValueError, match="not an integer in"):
        og.write_chips(tmp_path / "site.tif", tmp_path / "chips", CHIP, STRIDE, label_column="kind", **kw)
    with pytest.raises(ValueError, match="no entry for 'fir'"):
        og.write_chips(tmp_path / "site.tif", tmp_path / "chips", CHIP, STRIDE, label_column="kind", label_remap={"oak": 1}, **kw)
    with pytest.raises(ValueError, match="no column 'genus'"):
        og.write_chips(tmp_path / "site.tif", tmp_path / "chips", CHIP, STRIDE, label_column="genus", **kw)
    with pytest.raises(ValueError, match="background_ind"):
        og.write_chips(tmp_path / "site.tif", tmp_path / "chips", CHIP, STRIDE, background_ind=256, **kw)
    # refusals that stay, before anything is removed or read
    from PIL import Image

    Image.fromarray(np.zeros((5, 7, 3), np.uint8)).save(tmp_path / "site.png")
    Image.fromarray(np.zeros((5, 7, 3), np.uint8)).save(tmp_path / "plain.tif")
    keep = tmp_path / "keep"
    keep.mkdir()
    (keep / "old.txt").write_text("x")
    for raster, which in (("site.png", dict(label_vector_file="labels.geojson")), ("site.png", dict(ROI_file="roi.geojson")),
                          ("plain.tif", dict(label_vector_file=tmp_path / "labels.geojson")), ("site.tif", dict(label_vector_file="labels.shp")),
                          ("site.tif", dict(ROI_file="roi.gpkg"))):
        with pytest.raises(NotImplementedError, match=list(which)[0]):
            og.write_chips(tmp_path / raster, keep, CHIP, STRIDE, backend=backend, **which)
    assert (keep / "old.txt").is_file() and not backend.burners


def test_labels_in_another_crs_are_reprojected(site):
    """The label file in EPSG:4326 against the UTM raster: vertex-wise reprojection, as geopandas' to_crs.  The vertices come back
    within nanometres of where they were and none lies that close to a cell centre's row or column, so the chips are the same."""
    tmp_path, _, features = site
    backend = bs.StandInBackend()
    write_geojson(tmp_path / "lonlat.geojson", features, epsg=4326, to_lon_lat=True)
    lon = json.loads((tmp_path / "lonlat.geojson").read_text())["features"][0]["geometry"]["coordinates"][0][0]
    assert -124 < lon[0] < -121 and 37 < lon[1] < 39
    og.write_chips(tmp_path / "site.tif", tmp_path / "a", CHIP, STRIDE, label_vector_file=tmp_path / "lonlat.geojson", label_column="code",
                   write_empty_tiles=True, output_suffix=".png", backend=backend)
    want = chip_labels([3, 4, 3], 0)
    assert all(np.array_equal(read_png(tmp_path / "a" / "anns" / n), label) for n, label in want.items())
    like = PlanarRaster(np.zeros((H, W)), TRANSFORM, epsg=32610)
    polygons = PlanarPolygons.from_geojson(tmp_path / "lonlat.geojson")[0]
    assert polygons.epsg == 4326
    rings = [ring for feature in LABEL_RINGS for ring in feature]
    assert np.array_equal(burn_polygons(polygons, [3, 4, 3], like, fill=0, backend=backend), expected_label(rings, LABEL_ROWS, 3, [3, 4, 3], (0, 0, W, H), 0)[1])
    write_geojson(tmp_path / "nad83.geojson", features, epsg=26910)
    with pytest.raises(NotImplementedError, match="26910"):
        og.write_chips(tmp_path / "site.tif", tmp_path / "b", CHIP, STRIDE, label_vector_file=tmp_path / "nad83.geojson", backend=backend)


# -- the ROI filter ----------------------------------------------------------------------------------------------------------------------------------
def roi_edges(rings, rows):
    rv, off, rp = table(rings, rows)
    return ring_edges(rv, off, rp)


def rect(c0, r0, c1, r1):
    return (65536 * c0, 65536 * r0, 65536 * c1, 65536 * r1)


SLIVER_WINDOWS = {(0, 0), (3, 0), (3, 3), (6, 3), (6, 6), (9, 3), (9, 6)}


def test_rectangle_meets_rows_by_hand():
    # a thin diagonal sliver from (0.12, 0.2) to (11.92, 8.1), 0.02 cells wide: it holds no cell centre of the grid
    sliver = [(0.12, 0.2), (0.14, 0.2), (11.92, 8.1), (11.9, 8.1)]
    edges, row = roi_edges([sliver], [0])
    rings_q = bs.to_cell_units([np.asarray(sliver)], IDENTITY)
    assert not any(bs.centre_in_rings(65536 * c + 32768, 65536 * r + 32768, rings_q) for r in range(12) for c in range(14))
    got = {(c, r) for c in range(0, 14, 3) for r in range(0, 10, 3) if rectangle_meets_rows(edges, row, rect(c, r, c + 4, r + 4))}
    # its long sides run along y = 0.2 + 0.671 (x - 0.12): y = 2.13 at x = 3, 2.80 at 4, 4.14 at 6, 4.82 at 7, 6.16 at 9, 6.83 at 10 and
    # 8.1 at its end x = 11.92.  Over the columns [c, c + 4] of a window it covers y in [0.2, 2.80] (c = 0), [2.13, 4.82] (c = 3),
    # [4.14, 6.83] (c = 6), [6.16, 8.1] (c = 9) and nothing (c = 12), which meets the rows [r, r + 4] of:
    assert got == SLIVER_WINDOWS
    # a square with a hole: a rectangle inside the hole meets no edge and its corner is outside the row; one inside the ring's
    # body is inside whole; one across the hole's edge meets it
    edges, row = roi_edges([square(0, 0, 20, 20), square(5, 5, 15, 15)], [0, 0])
    assert not rectangle_meets_rows(edges, row, rect(7, 7, 11, 11))
    assert rectangle_meets_rows(edges, row, rect(1, 1, 4, 4)) and rectangle_meets_rows(edges, row, rect(3, 7, 7, 11))
    assert not rectangle_meets_rows(edges, row, rect(21, 0, 25, 4)) and not rectangle_meets_rows(edges, row, rect(-9, -9, -1, -1))
    assert rectangle_meets_rows(edges, row, rect(-5, -5, 30, 30))                       # the region inside the rectangle
    # touching counts: a corner on a corner, a side on a side, a corner on the hole's corner from inside the hole
    assert rectangle_meets_rows(edges, row, rect(20, 20, 24, 24)) and rectangle_meets_rows(edges, row, rect(20, 3, 24, 7))
    assert rectangle_meets_rows(edges, row, rect(11, 11, 15, 15)) and not rectangle_meets_rows(edges, row, rect(10, 10, 14, 14))
    assert not rectangle_meets_rows(edges, row, (65536 * 20 + 1, 0, 65536 * 24, 65536 * 4))   # one unit off the side
    # two rows: the union
    edges, row = roi_edges([square(0, 0, 2, 2), square(10, 10, 12, 12)], [0, 1])
    assert rectangle_meets_rows(edges, row, rect(11, 11, 30, 30)) and rectangle_meets_rows(edges, row, rect(-1, -1, 1, 1))
    assert not rectangle_meets_rows(edges, row, rect(3, 3, 9, 9))
    assert not rectangle_meets_rows(*roi_edges([], []), rect(0, 0, 4, 4))


def test_write_chips_with_a_region(site):
    tmp_path, _, features = site
    backend = bs.StandInBackend()
    # the sliver, in world coordinates: exactly the windows it crosses, although it holds no pixel centre
    sliver = [(600000.0 + 0.5 * x, 4200000.0 - 0.5 * y) for x, y in ((0.12, 0.2), (0.14, 0.2), (11.92, 8.1), (11.9, 8.1))]
    write_geojson(tmp_path / "roi.geojson", [({}, [sliver])], epsg=32610)
    written = og.write_chips(tmp_path / "site.tif", tmp_path / "chips", CHIP, STRIDE, ROI_file=tmp_path / "roi.geojson", output_suffix=".png")
    want = sorted(f"site:{c}:{r}:4:4.png" for c, r in SLIVER_WINDOWS)
    assert sorted(p.name for p in written) == want == sorted(p.name for p in (tmp_path / "chips").iterdir())
    # with labels: the ROI selects windows, the labels are not clipped to it
    roi = world(9.5, 0, 14, 5)
    write_geojson(tmp_path / "roi.geojson", [({}, [roi])], epsg=32610)
    written = og.write_chips(tmp_path / "site.tif", tmp_path / "chips", CHIP, STRIDE, label_vector_file=tmp_path / "labels.geojson",
                             label_column="code", write_empty_tiles=True, ROI_file=tmp_path / "roi.geojson", output_suffix=".png", backend=backend)
    names = sorted(p.name for p in written)
    assert names == sorted(f"site:{c}:{r}:4:4.png" for c in (6, 9, 12) for r in (0, 3)) and len(backend.burners[0].windows) == 6
    label = read_png(tmp_path / "chips" / "anns" / "site:6:3:4:4.png")
    assert np.array_equal(label, chip_labels([3, 4, 3], 0)["site:6:3:4:4.png"]) and label[:, 0].any()      # column 6 lies outside the ROI
    # the ROI in another CRS than the raster's
    write_geojson(tmp_path / "roi4326.geojson", [({}, [roi])], epsg=4326, to_lon_lat=True)
    again = og.write_chips(tmp_path / "site.tif", tmp_path / "chips2", CHIP, STRIDE, ROI_file=tmp_path / "roi4326.geojson", output_suffix=".png",
                           backend=backend)
    assert sorted(p.name for p in again) == names


def test_chip_ortho_takes_the_new_arguments():
    import inspect

    from geograypher_amd.entrypoints import chip_ortho

    args = chip_ortho.parse_args(["o.tif", "chips", "512", "256", "--label-vector-file", "l.geojson", "--ROI-file", "r.geojson", "--background-ind", "255"])
    assert args.ROI_file == Path("r.geojson") and args.background_ind == 255 and args.label_vector_file == Path("l.geojson")
    assert chip_ortho.parse_args(["o.tif", "chips", "512", "256"]).background_ind == NULL_TEXTURE_INT_VALUE
    assert set(vars(args)) <= set(inspect.signature(og.write_chips).parameters)
