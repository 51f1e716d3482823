"""The orthomosaic baseline without a GPU: the host functions against outputs of the REAL reference
(tests/golden/ortho_baseline.npz, made by tests/golden/make_golden_ortho.py), bit for bit; the stand-ins the GPU tests compare
the device with against those goldens and against hand-worked cases; window names, the GeoTIFF round trip, the C ABI of the new
companion header, and every refusal."""
import ctypes
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import ortho_standin as osn  # noqa: E402
import zonal_standin as zs  # noqa: E402
from geograypher_amd import _hip, build  # noqa: E402
from geograypher_amd.predictors import ortho_segmentor as og  # noqa: E402
from geograypher_amd.utils import prediction_metrics as pm  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons, tile_bin_table, zonal_work_items  # noqa: E402
from geograypher_amd.utils.geospatial import get_overlap_raster, raster_to_uint8, rings_to_cell_units, zonal_class_counts  # noqa: E402
from geograypher_amd.utils.numeric import create_ramped_weighting  # noqa: E402
from geograypher_amd.utils.raster import PlanarRaster, read_geotiff_header  # noqa: E402
from geograypher_amd.utils.tiff import write_tiff_deflate  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
COUNT_TYPES = {"uint8": np.uint8, "uint16": np.uint16, "float": float}


@pytest.fixture(scope="module")
def g():
    with np.load(ROOT / "tests" / "golden" / "ortho_baseline.npz", allow_pickle=False) as d:
        out = {k: d[k] for k in d.files}
    for a in out.values():
        a.setflags(write=False)
    return out


# -- goldens of the reference ------------------------------------------------------------------------------------------------------
def test_ramped_weighting_equals_the_reference(g):
    keys = [k for k in g if k.startswith("ramp__")]
    assert len(keys) == 5 * 4 + 2 * 4
    for key in keys:
        _, shape, frac = key.split("__")[:3]
        ramp = create_ramped_weighting(tuple(int(v) for v in shape.split("x")), float(frac))
        part = {"tl": ramp[:16, :16], "br": ramp[-16:, -16:]}[key.split("__")[3]] if key.count("__") == 3 else ramp
        assert part.dtype == np.float64 and np.array_equal(part, g[key]), key
    assert np.array_equal((create_ramped_weighting((4, 4), 0.5) * (255 / 4)).astype(np.uint8),
                          [[0, 0, 0, 0], [0, 42, 42, 0], [0, 42, 42, 0], [0, 0, 0, 0]])


def test_comprehensive_metrics_equal_the_reference(g):
    for k in range(4):
        names = [str(n) for n in g[f"metrics__{k}__names"]]
        m = pm.compute_comprehensive_metrics(g[f"metrics__{k}__cf"], names)
        summary = np.array([m["accuracy"], m["class_averaged_recall"], m["class_averaged_precision"]], dtype=np.float64)
        per_class = np.array([[m["per_class"][n][f] for f in ("acc", "recall", "precision", "num_true", "num_pred")] for n in names], dtype=np.float64)
        assert np.array_equal(summary, g[f"metrics__{k}__summary"], equal_nan=True)
        assert np.array_equal(per_class, g[f"metrics__{k}__per_class"], equal_nan=True)
    assert np.isnan(g["metrics__0__per_class"][2, 1]) and np.isnan(g["metrics__0__per_class"][2, 2])   # no true, no predicted sample


def test_confusion_matrix_of_label_lists_equals_the_reference(g, tmp_path):
    cases = sorted({k.rsplit("__", 1)[0] for k in g if k.startswith("cf__")})
    assert len(cases) == 4
    for case in cases:
        labels_in = g[case + "__labels_in"]
        matrix, labels, accuracy = pm.compute_and_show_cf(g[case + "__pred"].tolist(), g[case + "__gt"].tolist(),
                                                          labels=None if labels_in.size == 0 else labels_in.tolist(),
                                                          use_labels_from=case.split("__")[2], cf_np_savefile=tmp_path / "a" / "cf.npy")
        assert np.array_equal(matrix, g[case + "__matrix"]) and np.array_equal(np.asarray(labels), g[case + "__labels"])
        assert np.array_equal(np.float64(accuracy), g[case + "__accuracy"], equal_nan=True)
        assert np.array_equal(np.load(tmp_path / "a" / "cf.npy"), matrix)


@pytest.mark.parametrize("name", sorted(COUNT_TYPES))
def test_assembly_stand_in_reproduces_the_reference(g, name):
    """Golden cases 1-3: tests/ortho_standin.py -- what the GPU tests compare the device with -- equals what the reference's real
    assemble_tiled_predictions wrote, classes and counts."""
    windows = [tuple(int(v) for v in w) for w in g["tiles__windows"]]
    classes, counts, stats = osn.assemble(list(g["tiles__preds"]), windows, 12, 12, 3, count_dtype=COUNT_TYPES[name])
    assert np.array_equal(classes, g[f"asm__{name}__classes"])
    assert counts.dtype == g[f"asm__{name}__counts"].dtype and np.array_equal(counts, g[f"asm__{name}__counts"])
    assert stats.tolist() == [int((g[f"asm__{name}__counts"].sum(axis=0) != 0).sum()), int((g[f"asm__{name}__counts"].sum(axis=0) == 0).sum()), 5, 320]


@pytest.mark.parametrize("name", sorted(COUNT_TYPES))
def test_the_driver_reproduces_the_reference_through_files(g, name, tmp_path):
    """assemble_tiled_predictions over the golden tiles as files, with the stand-in backend in place of the device: tables, bands,
    the GeoTIFF and the counts file."""
    folder = tmp_path / "pred"
    folder.mkdir()
    for pred, (c, r, w, h) in zip(g["tiles__preds"], g["tiles__windows"]):
        np.save(folder / f"ortho:{c + 30}:{r + 20}:{w}:{h}.npy", pred)
    source = PlanarRaster(np.zeros((64, 64)), (0.5, 0.0, 1000.0, 0.0, -0.5, 2000.0), epsg=32610)
    backend = osn.StandInBackend()
    classes, extent = og.assemble_tiled_predictions(source, folder, tmp_path / "out" / "cls.tif", 3, counts_savefile=tmp_path / "out" / "cnt.npy",
                                                    count_dtype=COUNT_TYPES[name], max_device_bytes=200, backend=backend)
    assert tuple(extent) == (30, 20, 12, 12) and len(backend.calls) > 1 and sum(c[1] for c in backend.calls) == 12
    assert np.array_equal(classes, g[f"asm__{name}__classes"])
    saved = np.load(tmp_path / "out" / "cnt.npy")
    assert saved.dtype == g[f"asm__{name}__counts"].dtype and np.array_equal(saved, g[f"asm__{name}__counts"])
    back = PlanarRaster.from_geotiff(tmp_path / "out" / "cls.tif")
    assert np.array_equal(back.data[0], classes) and back.nodata == 0.0 and back.epsg == 32610
    assert back.transform == (0.5, 0.0, 1015.0, 0.0, -0.5, 1990.0)


# -- windows -------------------------------------------------------------------------------------------------------------------------
def test_windows_by_hand():
    windows = og.create_windows((5, 7), 4, 3)
    assert [tuple(w) for w in windows] == [(0, 0, 4, 4), (0, 3, 4, 4), (3, 0, 4, 4), (3, 3, 4, 4), (6, 0, 4, 4), (6, 3, 4, 4)]
    assert og.get_str_from_window(og.Window(6, 3, 4, 4), "/data/site one.ortho.tif", "png") == "site one.ortho:6:3:4:4.png"
    assert og.get_str_from_window(og.Window(0, 0, 2, 9), "o.tif", ".JPG") == "o:0:0:2:9.JPG"
    files = [Path("/p") / og.get_str_from_window(w, "o.tif", ".npy") for w in windows[2:]]
    parsed, extent = og.parse_windows_from_files(files)
    assert tuple(extent) == (3, 0, 7, 7) and [tuple(w) for w in parsed] == [(0, 0, 4, 4), (0, 3, 4, 4), (3, 0, 4, 4), (3, 3, 4, 4)]
    parsed, extent = og.parse_windows_from_files(files, return_in_extent_coords=False)
    assert tuple(extent) == (3, 0, 7, 7) and tuple(parsed[0]) == (3, 0, 4, 4)
    parsed, _ = og.parse_windows_from_files([Path("a_5_6_2_3.png")], sep="_")
    assert tuple(parsed[0]) == (0, 0, 2, 3)
    for bad in ("o:1:2:3.npy", "o:1:2:3:x.npy", "plain.npy"):
        with pytest.raises(ValueError, match="col_off"):
            og.parse_windows_from_files([Path(bad)])
    with pytest.raises(ValueError, match="no prediction files"):
        og.parse_windows_from_files([])
    assert og.pad_to_full_size(np.ones((2, 3, 3)), (4, 4)).shape == (4, 4, 3) and og.pad_to_full_size(np.ones((2, 3)), (2, 3)).shape == (2, 3)
    assert og.pad_to_full_size(np.ones((2, 3)), (4, 4))[2:].sum() == 0


def test_tile_tables_and_bins():
    preds = [np.array([[0, 1, 2], [3, 255, 7]]), np.array([[0.0, 1.5, np.nan], [-1.0, 2.0, 1.0]]), np.zeros((3, 2), np.int64)]
    t = og.tile_tables(preds, [og.Window(0, 0, 3, 2), og.Window(1, 1, 3, 2), og.Window(0, 0, 2, 3)], 3)
    assert t[0].tolist() == [0, 1, 2, 255, 255, 255, 0, 255, 255, 255, 2, 1, 0, 0, 0, 0, 0, 0] and t[1].tolist() == [0, 6, 12, 18]
    assert t[3].tolist() == [0, 0, 1] and t[5].tolist() == [0, 6, 12] and t[4].dtype == np.uint8
    assert og.tile_tables(preds[:1], [og.Window(0, 0, 3, 2)], 3, count_dtype=float)[4].dtype == np.float64
    with pytest.raises(ValueError, match="Size of pred does not match window"):
        og.tile_tables(preds, [og.Window(0, 0, 3, 2), og.Window(1, 1, 2, 3), og.Window(0, 0, 2, 3)], 3)
    with pytest.raises(ValueError, match="num_classes"):
        og.tile_tables(preds, [og.Window(0, 0, 3, 2)] * 3, 256)
    ptr, tiles, side, bx, by = tile_bin_table([(0, 0, 5, 5), (4, 4, 5, 5), (8, 0, 1, 1), (0, 0, 0, 3)], 9, 9, 4)
    assert (side, bx, by) == (4, 3, 3) and ptr.tolist() == [0, 1, 2, 3, 4, 6, 7, 7, 8, 9] and tiles.tolist() == [0, 0, 2, 0, 0, 1, 1, 1, 1]
    assert og.band_rows(100, 50, 3, 1, True, 4, 1600) == 2 and og.band_rows(100, 50, 3, 1, False, 4, 10) == 1
    assert og.band_rows(10, 50, 3, 8, True, 4, 1 << 30) == 50


def test_table_checks_refuse_what_the_kernel_would_clamp():
    t = og.tile_tables([np.zeros((4, 4), np.uint8)] * 2, [og.Window(0, 0, 4, 4), og.Window(2, 1, 4, 4)], 2)
    bins = tile_bin_table(t[2], 6, 5, 4)

    def run(**kw):
        a = dict(pred_offsets=t[1], windows=t[2], tile_table=t[3], weight_offsets=t[5], n_pred_bytes=32, n_weights=16, bin_ptr=bins[0],
                 bin_tiles=bins[1], bin_side=4, bins_x=2, bins_y=2, width=6, height=5, row0=0, n_rows=5, num_classes=2, nodataval=0)
        a.update(kw)
        _hip.check_assemble_tables(**a)

    run()
    moved = t[2].copy()
    moved[1, 0] = 3
    for kw in (dict(windows=moved), dict(windows=t[2][:1]), dict(pred_offsets=np.array([0, 15, 32])), dict(tile_table=np.array([0, 1])),
               dict(weight_offsets=np.array([0, 15])), dict(n_weights=15), dict(n_pred_bytes=31), dict(bin_tiles=bins[1][::-1].copy()),
               dict(bin_tiles=np.where(bins[1] == 1, 2, bins[1])), dict(bin_ptr=bins[0][:-1]), dict(bins_x=1), dict(bin_side=0),
               dict(row0=1), dict(n_rows=-1), dict(num_classes=0), dict(num_classes=256), dict(nodataval=-1)):
        with pytest.raises(ValueError, match="gr_assemble_tiles"):
            run(**kw)
    rv, off = rings_to_cell_units([np.array([(1.0, 1.0), (8.0, 1.0), (8.0, 8.0)])], (1, 0, 0, 0, 1, 0))
    items = zonal_work_items(rv, off, [0], 1, 10, 10)
    _hip.check_zonal_tables(10, 10, None, rv, off, [0], 1, items, 5)
    for args in ((0, 10, None, rv, off, [0], 1, items, 5), (10, 1 << 23, None, rv, off, [0], 1, items, 5), (10, 10, None, rv, off, [0], 1, items, 0),
                 (10, 10, None, rv, off, [0], 1, items, 257), (10, 10, None, rv.astype(np.float64), off, [0], 1, items, 5),
                 (10, 10, None, rv + (1 << 40), off, [0], 1, items, 5), (10, 10, None, rv, off[:1], [0], 1, items, 5),
                 (10, 10, None, rv, off, [1], 1, items, 5), (10, 10, None, rv, [0, 3, 3], [1, 0], 2, items, 5),
                 (10, 10, None, rv, off, [0], 1, items[:, :6], 5), (10, 10, None, rv, off, [0], 1, items + [0, 0, 0, 64, 0, 0, 0], 5),
                 (9, 7, None, rv, off, [0], 1, items, 5)):
        with pytest.raises(ValueError, match="gr_zonal_class_counts"):
            _hip.check_zonal_tables(*args)
    assert [_hip.zonal_nodata(v) for v in (None, 0, 255.0, 256, -1, 2.5, float("nan"))] == [-1, 0, 255, -1, -1, -1, -1]
    for block in ((65, 1), (1, 129), (0, 4)):
        with pytest.raises(ValueError, match="block"):
            zonal_work_items(rv, off, [0], 1, 10, 10, block)


# -- the GeoTIFF round trip --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transform", [(0.25, 0.0, 500000.5, 0.0, -0.25, 4100000.25), (0.2, 0.05, -30.0, -0.04, -0.21, 77.5)])
@pytest.mark.parametrize("nodata,epsg", [(0, 32610), (255, 4326), (3, None)])
def test_geotiff_round_trip(tmp_path, transform, nodata, epsg):
    data = np.random.default_rng(0).integers(0, 6, (37, 53)).astype(np.uint8)
    write_tiff_deflate(tmp_path / "c.tif", data, transform=transform, nodata=nodata, epsg=epsg)
    back = PlanarRaster.from_geotiff(tmp_path / "c.tif")
    assert np.array_equal(back.data[0], data) and back.transform == transform and back.nodata == float(nodata) and back.epsg == epsg
    assert read_geotiff_header(tmp_path / "c.tif") == (transform, float(nodata), epsg, 37, 53)
    write_tiff_deflate(tmp_path / "rgba.tif", np.zeros((5, 6, 3), np.uint8), transform=transform, epsg=epsg)
    with pytest.raises(ValueError, match="image mode"):
        PlanarRaster.from_geotiff(tmp_path / "rgba.tif")
    assert read_geotiff_header(tmp_path / "rgba.tif") == (transform, None, epsg, 5, 6)
    write_tiff_deflate(tmp_path / "plain.tif", data)
    with pytest.raises(ValueError, match="no georeferencing"):
        read_geotiff_header(tmp_path / "plain.tif")


# -- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_ortho_header_and_binding_agree():
    """The contract tests/test_cabi.py keeps for include/geograster.h, for the companion header of the orthomosaic baseline: every
    function it declares is in the binding's table with as many arguments, each of the declared kind, and the library exports it."""
    main = (ROOT / "include" / "geograster.h").read_text()
    assert re.search(r'^#include "geograster_ortho.h"$', main, re.M) and main.index("geograster_ortho.h") < main.rindex("#ifdef __cplusplus")
    assert main.index('#include "geograster_outlines.h"') < main.index('#include "geograster_ortho.h"')
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", (ROOT / "include" / "geograster_ortho.h").read_text(), flags=re.S)
    declared = {name: [a.strip() for a in " ".join(args.split()).split(",")]
                for name, args in re.findall(r"\b(gr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}
    assert sorted(declared) == sorted(_hip._ORTHO_SIGNATURES) == sorted(_hip.ORTHO_SYMBOLS) == ["gr_assemble_tiles", "gr_zonal_class_counts"]
    assert not set(declared) & (set(_hip._SIGNATURES) | set(_hip._COMPANION_SIGNATURES))
    kinds = {ctypes.c_int64: "int64", ctypes.c_int: "int", ctypes.c_int32: "int", ctypes.c_double: "double"}
    lib = ctypes.CDLL(str(build.build()))
    for name, arguments in declared.items():
        argtypes = _hip._ORTHO_SIGNATURES[name]
        assert len(arguments) == len(argtypes) and hasattr(lib, name), name
        for argument, ctype in zip(arguments, argtypes):
            want = "pointer" if "*" in argument else {"int64_t": "int64", "int32_t": "int", "int": "int", "double": "double"}[argument.split()[0]]
            got = "pointer" if ctype is ctypes.c_void_p or issubclass(ctype, ctypes._Pointer) else kinds[ctype]
            assert want == got, f"{name}: {argument!r} is bound as {ctype.__name__}"
    assert any(p.name == "ortho.hip" for p in build.SOURCES)
    assert callable(_hip.HipRaster.assemble_tiles) and callable(_hip.HipRaster.zonal_class_counts)
    source = (ROOT / "geograypher_amd" / "csrc" / "ortho.hip").read_text()
    kernel = source[source.index("void k_assemble_tiles("):source.index("// The ring statistics")]
    assert "atomic" not in kernel and kernel.count("stat_") == 4          # O6: no count is formed by atomics, four statistics words
    zonal = source[source.index("void k_zonal_class_counts("):source.index("}  // namespace")]
    assert not re.search(r"\b(double|float)\b", zonal)


def test_calls_without_a_context_are_refused_by_the_library():
    lib = ctypes.CDLL(str(build.build()))
    for name in _hip.ORTHO_SYMBOLS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_int, _hip._ORTHO_SIGNATURES[name]
    assert lib.gr_assemble_tiles(None, None, 0, None, None, None, 0, None, 0, None, 0, 0, None, None, 0, 1, 1, 1, 0, 0, 0, 1, 0, None, None,
                                 None, None) == _hip.GR_EINVAL
    assert lib.gr_zonal_class_counts(None, None, 1, 1, -1, None, 0, None, None, 0, 0, None, 0, 1, None, None, None) == _hip.GR_EINVAL


# -- the zonal stand-in by hand ------------------------------------------------------------------------------------------------------
def square(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def q(ring):
    return [(int(round(x * 65536)), int(round(y * 65536))) for x, y in ring]


def test_zonal_stand_in_by_hand():
    raster = np.arange(16, dtype=np.uint8).reshape(4, 4) % 4          # the value of a cell is its column; unit cells
    counts, stats = zs.zonal_counts(raster, None, [q(square(1, 1, 3, 3))], [0], 1, 4)
    assert counts.tolist() == [[0, 2, 2, 0]] and stats.tolist() == [0, 4, 0, 0, 3, 4, 0]  + [0]
    # a square whose edges pass through cell centres: the centres on its left and top edge are in, on its right and bottom edge out
    for ring in (square(0.5, 0.5, 2.5, 2.5), square(0.5, 0.5, 2.5, 2.5)[::-1]):        # whichever way the ring runs
        counts, _ = zs.zonal_counts(raster, None, [q(ring)], [0], 1, 4)
        assert counts.tolist() == [[2, 2, 0, 0]]
    # two squares sharing such an edge: every centre on it is counted exactly once
    counts, stats = zs.zonal_counts(raster, None, [q(square(0.5, 0.5, 2.5, 2.5)), q(square(2.5, 0.5, 3.5, 2.5))], [0, 1], 2, 4)
    assert counts.tolist() == [[2, 2, 0, 0], [0, 0, 2, 0]]
    counts, _ = zs.zonal_counts(raster, None, [q(square(0.5, 0.5, 2.5, 1.5)), q(square(0.5, 1.5, 2.5, 3.5))], [0, 1], 2, 4)
    assert counts.tolist() == [[1, 1, 0, 0], [2, 2, 0, 0]]                               # ... and on a horizontal one
    # a polygon with a hole (all rings of a row, even-odd), a two-part row, a 2-vertex ring
    counts, stats = zs.zonal_counts(raster, None, [q(square(0, 0, 4, 4)), q(square(1, 1, 3, 3)), q(square(0, 0, 1, 1)), q(square(3, 3, 4, 4)),
                                                   q([(0, 0), (4, 4)])], [0, 0, 1, 1, 1], 2, 4)
    assert counts.tolist() == [[4, 2, 2, 4], [1, 0, 0, 1]] and stats[5] == 4 and stats[6] == 1 and stats[1] == 14
    # nodata and values beyond the classes
    counts, stats = zs.zonal_counts(raster, 1, [q(square(0, 0, 4, 4))], [0], 1, 3)
    assert counts.tolist() == [[4, 0, 4]] and stats.tolist() == [0, 16, 4, 4, 4, 4, 0, 0]
    # Z1: a north-up transform with half-metre cells
    inverse = PlanarRaster(raster, (0.5, 0.0, 100.0, 0.0, -0.5, 50.0)).inverse
    rings = zs.to_cell_units([[(100.5, 49.5), (101.5, 49.5), (101.5, 48.5), (100.5, 48.5)]], inverse)
    assert rings == [q(square(1, 1, 3, 3))]
    rv, off = rings_to_cell_units([[(100.5, 49.5), (101.5, 49.5), (101.5, 48.5), (100.5, 48.5)]], inverse)
    assert rv.tolist() == [list(v) for v in rings[0]] and off.tolist() == [0, 4]
    with pytest.raises(ValueError, match="2\\^40"):
        rings_to_cell_units([[(1e9, 0.0), (0.0, 0.0), (1.0, 1.0)]], inverse)
    items = zonal_work_items(rv, off, [0], 1, 4, 4, (1, 2))
    assert items.tolist() == [[0, 1, 1, 1, 2, 0, 1], [0, 2, 1, 1, 2, 0, 1]]


# -- the layers above the zonal counts, with the stand-in backend ----------------------------------------------------------------------
def write_geojson(path, rows):
    features = [{"type": "Feature", "properties": {"class_names": name}, "geometry": {"type": "Polygon", "coordinates": [[list(p) for p in ring + ring[:1]]]}}
                for name, ring in rows]
    path.write_text(json.dumps({"type": "FeatureCollection", "features": features}))


def test_overlap_raster_and_confusion_matrix(tmp_path):
    cells = np.array([[0, 0, 1, 1], [0, 2, 1, 1], [2, 2, 2, 7], [7, 7, 7, 7]], dtype=np.uint8)
    raster = PlanarRaster(cells, (1.0, 0.0, 10.0, 0.0, -1.0, 24.0), nodata=7)
    world = lambda x0, y0, x1, y1: [(10.0 + x0, 24.0 - y0), (10.0 + x1, 24.0 - y0), (10.0 + x1, 24.0 - y1), (10.0 + x0, 24.0 - y1)]  # noqa: E731
    polygons = [np.array(world(0, 0, 2, 2)), np.array(world(50, 50, 60, 60)), np.array(world(0, 3, 4, 4)), np.array(world(2, 0, 4, 3))]
    backend = zs.StandInBackend()
    matrix, valid = get_overlap_raster(polygons, raster, backend=backend)
    assert valid.tolist() == [0, 3] and valid.dtype == np.int64 and matrix.dtype == np.float64
    assert matrix.tolist() == [[3.0, 0.0, 1.0], [0.0, 4.0, 1.0]]       # row k is valid polygon k: the reference would write row 3 of 2
    matrix, _ = get_overlap_raster(PlanarPolygons.from_sequence(polygons), raster, num_classes=4, normalize=True, backend=backend)
    assert matrix.tolist() == [[0.75, 0.0, 0.25, 0.0], [0.0, 0.8, 0.2, 0.0]]
    with pytest.raises(ValueError, match="2 counted cells hold a value >= num_classes=2"):
        get_overlap_raster(polygons, raster, num_classes=2, backend=backend)
    counts, stats = zonal_class_counts(polygons, raster, backend=backend, block=(2, 1))
    assert counts.shape == (4, 3) and stats["nodata"] == 5 and stats["inside"] == 14 and stats["largest_plus_1"] == 3
    with pytest.raises(ValueError, match="not an integer in"):
        raster_to_uint8(np.array([[0.5, 1.0]]), None)
    assert raster_to_uint8(np.array([[-9999.0, 1.0]]), -9999.0)[1] == 255 and raster_to_uint8(np.array([[3.0, 1.0]]), 300.0)[1] is None
    # the confusion matrix against one feature per class name
    truth = tmp_path / "truth.geojson"
    write_geojson(truth, [("oak", world(0, 0, 2, 2)), ("fir", world(2, 0, 4, 3))])
    write_tiff_deflate(tmp_path / "pred.tif", cells, transform=raster.transform, nodata=7, epsg=32610)
    names = ["fir", "oak", "ash"]
    cf, out_names, accuracy = pm.compute_confusion_matrix_from_geospatial(tmp_path / "pred.tif", truth, names, normalize=False, backend=backend)
    assert names == ["fir", "oak", "ash"] and out_names == ["fir", "oak", "ash", "unlabeled"]
    assert cf.tolist() == [[0, 4, 1, 0], [3, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]] and accuracy == 0.0
    cf, _, accuracy = pm.compute_confusion_matrix_from_geospatial(raster, truth, names, remap_raster_inds=[1, 0, 2], backend=backend)
    assert np.array_equal(cf * 9, [[4, 0, 1, 0], [0, 3, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]]) and abs(accuracy - 7 / 9) < 1e-15
    write_geojson(truth, [("oak", world(0, 0, 2, 2)), ("oak", world(2, 0, 4, 3))])
    with pytest.raises(ValueError, match="dissolve"):
        pm.compute_confusion_matrix_from_geospatial(raster, truth, names, backend=backend)
    for kw in (dict(vis=True), dict(vis_savefile="x.png")):
        with pytest.raises(NotImplementedError, match="vis"):
            pm.compute_confusion_matrix_from_geospatial(raster, truth, names, **kw)
    with pytest.raises(NotImplementedError, match="vector prediction"):
        pm.compute_confusion_matrix_from_geospatial(tmp_path / "pred.geojson", truth, names)
    with pytest.raises(ValueError, match="Unknown extension"):
        pm.compute_confusion_matrix_from_geospatial(tmp_path / "pred.xyz", truth, names)
    with pytest.raises(NotImplementedError, match="vis"):
        pm.compute_and_show_cf([0], [0], vis=True)
    with pytest.raises(ValueError, match="Must use labels from"):
        pm.compute_and_show_cf([0], [0], use_labels_from="neither")


# -- refusals of the assembly driver, chips, entry points ---------------------------------------------------------------------------
def test_refusals_and_chips(tmp_path):
    folder = tmp_path / "pred"
    folder.mkdir()
    np.save(folder / "o:0:0:4:4.npy", np.zeros((4, 5), np.uint8))
    source = PlanarRaster(np.zeros((8, 8)), (1.0, 0.0, 0.0, 0.0, -1.0, 8.0))
    with pytest.raises(NotImplementedError, match="counts are saved as .npy"):
        og.assemble_tiled_predictions(source, folder, tmp_path / "c.tif", 2, counts_savefile=tmp_path / "counts.tif", backend=osn.StandInBackend())
    with pytest.raises(ValueError, match="Size of pred does not match window"):
        og.assemble_tiled_predictions(source, folder, tmp_path / "c.tif", 2, backend=osn.StandInBackend())
    np.save(folder / "o:0:0:4:4.npy", np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError, match="nodataval"):
        og.assemble_tiled_predictions(source, folder, tmp_path / "c.tif", 2, nodataval=256, backend=osn.StandInBackend())
    with pytest.raises(ValueError, match="count_dtype"):
        _hip._count_kind(np.int32)
    classes, extent = og.assemble_tiled_predictions(source, folder, tmp_path / "c.tif", 2, nodataval=None, backend=osn.StandInBackend())
    assert classes.tolist() == [[2, 2, 2, 2], [2, 0, 0, 2], [2, 0, 0, 2], [2, 2, 2, 2]] and PlanarRaster.from_geotiff(tmp_path / "c.tif").nodata == 2.0
    # predictions as images
    from PIL import Image

    Image.fromarray(np.ones((4, 4), np.uint8)).save(folder / "o:2:0:4:4.png")
    classes, extent = og.assemble_tiled_predictions(source, folder, tmp_path / "c.tif", 2, nodataval=None, backend=osn.StandInBackend())
    assert tuple(extent) == (0, 0, 6, 4) and classes[1].tolist() == [2, 0, 0, 1, 1, 2]
    # chips: an RGBA image, 5 x 7, chips of 4 every 3
    rgba = np.zeros((5, 7, 4), np.uint8)
    rgba[..., :3] = np.arange(35, dtype=np.uint8).reshape(5, 7, 1) + 100
    rgba[:, :6, 3] = 255                 # the last column is transparent: the chip at column 6 is all transparent
    rgba[0, 0, 3] = 0
    Image.fromarray(rgba).save(tmp_path / "site.png")
    (tmp_path / "chips").mkdir()
    (tmp_path / "chips" / "old.txt").write_text("x")
    written = og.write_chips(tmp_path / "site.png", tmp_path / "chips", 4, 3, output_suffix=".png")
    assert sorted(p.name for p in (tmp_path / "chips").iterdir()) == sorted(p.name for p in written) == [
        "site:0:0:4:4.png", "site:0:3:4:4.png", "site:3:0:4:4.png", "site:3:3:4:4.png"]
    chip = np.array(Image.open(tmp_path / "chips" / "site:3:3:4:4.png"))
    assert chip.shape == (4, 4, 3) and chip[0, 0].tolist() == [100 + 3 * 7 + 3] * 3 and chip[2:].sum() == 0 and chip[0, 3].sum() == 0
    assert np.array(Image.open(tmp_path / "chips" / "site:0:0:4:4.png"))[0, 0].tolist() == [0, 0, 0]
    assert len(og.write_chips(tmp_path / "site.png", tmp_path / "chips", 4, 3, output_suffix="png", drop_transparency=False)) == 6
    assert len(og.write_chips(tmp_path / "site.png", tmp_path / "jpg", 4, 3)) == 4 and (tmp_path / "jpg" / "site:0:0:4:4.JPG").is_file()
    with pytest.raises(NotImplementedError, match="label_vector_file"):
        og.write_chips(tmp_path / "site.png", tmp_path / "chips", 4, 3, label_vector_file="labels.geojson")
    with pytest.raises(NotImplementedError, match="ROI_file"):
        og.write_chips(tmp_path / "site.png", tmp_path / "chips", 4, 3, ROI_file="roi.geojson")


def test_entry_points_parse_the_references_arguments():
    import inspect

    from geograypher_amd.entrypoints import assemble_ortho_predictions, chip_ortho

    args = assemble_ortho_predictions.parse_args(["o.tif", "preds", "out/cls.tif", "5"])
    assert vars(args) == dict(raster_file=Path("o.tif"), pred_folder=Path("preds"), class_savefile=Path("out/cls.tif"), num_classes=5,
                              counts_savefile=None, downweight_edge_frac=0.25, nodataval=0, max_overlapping_tiles=4, count_dtype=np.uint8)
    args = assemble_ortho_predictions.parse_args(["o.tif", "preds", "cls.tif", "5", "--count-dtype", "float", "--nodataval", "255",
                                                  "--counts-savefile", "c.npy", "--downweight-edge-frac", "0.1", "--max-overlapping-tiles", "9"])
    assert args.count_dtype is float and args.nodataval == 255 and args.counts_savefile == Path("c.npy") and args.max_overlapping_tiles == 9
    assert set(vars(args)) <= set(inspect.signature(og.assemble_tiled_predictions).parameters)
    with pytest.raises(SystemExit):
        assemble_ortho_predictions.parse_args(["o.tif", "preds", "cls.tif", "5", "--count-dtype", "int32"])
    args = chip_ortho.parse_args(["o.tif", "chips", "512", "256", "--label-remap", '{"a": 1}', "--write-empty-tiles"])
    assert (args.raster_file, args.output_folder, args.chip_size, args.chip_stride) == (Path("o.tif"), Path("chips"), 512, 256)
    assert args.label_remap == {"a": 1} and args.write_empty_tiles is True and args.label_vector_file is None
    assert chip_ortho.parse_args(["o.tif", "chips", "512", "256"]).label_remap is None
    assert set(vars(args)) <= set(inspect.signature(og.write_chips).parameters)
