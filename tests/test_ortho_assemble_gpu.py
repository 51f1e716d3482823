"""gr_assemble_tiles on the device against tests/ortho_standin.py (rules O1-O8 of DESIGN.md 8m), which
tests/test_ortho_baseline_host.py pins to the outputs of the real reference.  Every rule is integer or fixed-order float64
arithmetic: all comparisons are np.array_equal -- classes, counts and the statistics words."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import ortho_standin as osn  # noqa: E402
from geograypher_amd.predictors import ortho_segmentor as og  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "ortho_baseline.npz"
COUNT_TYPES = {"uint8": np.uint8, "uint16": np.uint16, "float": float}


def run(hip, preds, windows, width, height, C, nodataval=0, frac=0.25, count_dtype=np.uint8, max_tiles=4, want_counts=True,
        rows_per_band=None, bin_side=None):
    """-> (classes, counts, stats (4,) int64) of the device through the product's driver."""
    tables = og.tile_tables(preds, [og.Window(*w) for w in windows], C, frac, count_dtype, max_tiles)
    classes, counts, stats = og.assemble_on_device(hip, tables, width, height, C, C if nodataval is None else nodataval, count_dtype,
                                                   want_counts=want_counts, rows_per_band=rows_per_band, bin_side=bin_side)
    return classes, counts, np.array([stats["with_class"], stats["without"], stats["longest_list"], stats["pairs"]], dtype=np.int64)


def check(hip, preds, windows, width, height, C, nodataval=0, frac=0.25, count_dtype=np.uint8, max_tiles=4, **kw):
    want = osn.assemble(preds, windows, width, height, C, nodataval, frac, count_dtype, max_tiles)
    got = run(hip, preds, windows, width, height, C, nodataval, frac, count_dtype, max_tiles, **kw)
    assert got[0].dtype == np.uint8 and np.array_equal(got[0], want[0])
    assert got[1].dtype == want[1].dtype and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    return got, want


def chip_scene(seed, height, width, chip, stride, C, top=None):
    """Chips of `chip` every `stride` over a height x width raster, windows reaching past its far edges (the extent is their box),
    predictions in [0, top) with some 255."""
    rng = np.random.default_rng(seed)
    windows = [tuple(w) for w in og.create_windows((height, width), chip, stride)]
    top = C + 2 if top is None else top
    preds = [np.where(rng.random((chip, chip)) < 0.1, 255, rng.integers(0, top, (chip, chip))).astype(np.uint8) for _ in windows]
    _, extent = og.parse_windows_from_files([Path(og.get_str_from_window(og.Window(*w), "o.tif", ".npy")) for w in windows])
    return preds, windows, extent.width, extent.height


@pytest.mark.parametrize("name", sorted(COUNT_TYPES))
def test_golden_cases_of_the_reference(hip, name):
    """Golden cases 1-3 themselves: the device against what the reference's assemble_tiled_predictions wrote."""
    with np.load(GOLDEN) as g:
        preds, windows = list(g["tiles__preds"]), [tuple(int(v) for v in w) for w in g["tiles__windows"]]
        classes, counts = g[f"asm__{name}__classes"], g[f"asm__{name}__counts"]
    got, _ = check(hip, preds, windows, 12, 12, 3, count_dtype=COUNT_TYPES[name])
    assert np.array_equal(got[0], classes) and np.array_equal(got[1], counts) and got[1].dtype == counts.dtype


def test_a_tie_goes_to_the_lower_class(hip):
    """4 x 4 tiles at frac 0.5: the inner 2 x 2 weighs 42, the ring 0.  Tiles of classes 2 and 1 overlapping by two columns meet
    only inner-on-ring; overlapping by three columns, and lying on each other, their inner pixels tie at 42 : 42 and the lower
    class, 1, wins although class 2 is the tile with the lower index."""
    preds = [np.full((4, 4), 2, np.uint8), np.full((4, 4), 1, np.uint8)]
    got, _ = check(hip, preds, [(0, 0, 4, 4), (2, 0, 4, 4)], 6, 4, 3, frac=0.5)
    assert got[1][2, 1, 2] == 42 and got[1][1, 1, 2] == 0 and got[0][1].tolist() == [0, 2, 2, 1, 1, 0]
    got, _ = check(hip, preds, [(0, 0, 4, 4), (1, 0, 4, 4)], 5, 4, 3, frac=0.5)
    assert got[1][2, 1, 2] == 42 and got[1][1, 1, 2] == 42 and got[0][1].tolist() == [0, 2, 1, 1, 0]
    got, _ = check(hip, preds, [(0, 0, 4, 4), (0, 0, 4, 4)], 4, 4, 3, frac=0.5)
    assert got[0][1].tolist() == [0, 1, 1, 0] and got[2].tolist() == [4, 12, 2, 32]


def test_padded_windows_and_ignored_predictions(hip):
    preds, windows, width, height = chip_scene(1, 13, 19, 8, 4, 3)
    assert (width, height) == (24, 20) and any(p.max() == 255 for p in preds) and any(((p >= 3) & (p < 255)).any() for p in preds)
    check(hip, preds, windows, width, height, 3)


def test_nine_tiles_over_a_pixel(hip):
    preds, windows, width, height = chip_scene(2, 12, 12, 9, 3, 4)
    _, want = check(hip, preds, windows, width, height, 4, max_tiles=9)
    assert want[2][2] == 9


def test_128_tiles_wrap_to_nodata(hip):
    """128 identical 4 x 4 tiles of class 1 at frac 0.5: 128 x 42 = 0 mod 256, every pixel comes out nodata (one full LDS chunk of
    tile records); with three tiles of class 0 behind them (a second chunk) class 0 has 126 and wins."""
    preds = [np.full((4, 4), 1, np.uint8)] * 128
    got, _ = check(hip, preds, [(0, 0, 4, 4)] * 128, 4, 4, 2, nodataval=7, frac=0.5)
    assert np.all(got[0] == 7) and np.all(got[1] == 0) and got[2][2] == 128
    got, _ = check(hip, preds + [np.full((4, 4), 0, np.uint8)] * 3, [(0, 0, 4, 4)] * 131, 4, 4, 2, nodataval=7, frac=0.5)
    assert got[0][1, 1] == 0 and got[1][0, 1, 1] == 126 and got[1][1, 1, 1] == 0 and got[2][2] == 131


def test_two_tile_shapes_in_one_call(hip):
    rng = np.random.default_rng(3)
    windows = [(0, 0, 8, 8), (6, 0, 5, 8), (3, 2, 8, 8), (0, 1, 5, 8)]
    preds = [rng.integers(0, 3, (h, w)).astype(np.uint8) for _, _, w, h in windows]
    tables = og.tile_tables(preds, [og.Window(*w) for w in windows], 3)
    assert len(tables[5]) == 3 and tables[3].tolist() == [0, 1, 0, 1]
    check(hip, preds, windows, 11, 10, 3)


@pytest.mark.parametrize("width", [1, 63, 64, 65, 257])
def test_extent_widths(hip, width):
    rng = np.random.default_rng(width)
    windows = [(c, r, min(40, width - c), 5) for r in (0, 3) for c in range(0, width, 25)]
    preds = [rng.integers(0, 5, (h, w)).astype(np.uint8) for _, _, w, h in windows]
    check(hip, preds, windows, width, 8, 5, frac=0.3)


def test_a_non_zero_extent_corner_and_nodataval_none(hip, tmp_path):
    rng = np.random.default_rng(5)
    files = [tmp_path / f"o:{c}:{r}:6:6.npy" for c, r in ((100, 40), (103, 40), (100, 44))]
    windows, extent = og.parse_windows_from_files(files)
    assert tuple(extent) == (100, 40, 9, 10) and tuple(windows[1]) == (3, 0, 6, 6)
    preds = [rng.integers(0, 3, (6, 6)).astype(np.uint8) for _ in files]
    got, _ = check(hip, preds, [tuple(w) for w in windows], 9, 10, 2, nodataval=None)
    assert got[0][0, 0] == 2      # the outermost ring weighs 0: no class, nodataval = num_classes


@pytest.mark.parametrize("name", sorted(COUNT_TYPES))
def test_each_count_type_on_a_crowded_scene(hip, name):
    """uint8 wraps here (frac 0.1: up to nine full weights of 63 on a pixel, two classes); float64 is bit-equal to the stand-in's
    sums in ascending tile index."""
    preds, windows, width, height = chip_scene(7, 20, 17, 9, 3, 2, top=2)
    got, _ = check(hip, preds, windows, width, height, 2, frac=0.1, count_dtype=COUNT_TYPES[name])
    if name == "uint8":
        wide = osn.assemble(preds, windows, width, height, 2, 0, 0.1, np.uint16, 4 * 257)[1]   # the same weights, no wrap
        assert np.any(wide > 255) and np.array_equal(got[1], wide.astype(np.uint8))


def test_counts_bands_and_bin_sides_change_nothing(hip):
    preds, windows, width, height = chip_scene(9, 21, 30, 8, 4, 4)
    base = run(hip, preds, windows, width, height, 4)
    want = osn.assemble(preds, windows, width, height, 4)
    assert all(np.array_equal(a, b) for a, b in zip(base, want))
    without = run(hip, preds, windows, width, height, 4, want_counts=False)
    assert without[1] is None and np.array_equal(without[0], base[0]) and np.array_equal(without[2], base[2])
    for rows_per_band in (1, 5):
        band = run(hip, preds, windows, width, height, 4, rows_per_band=rows_per_band)
        assert band[0].tobytes() == base[0].tobytes() and band[1].tobytes() == base[1].tobytes()
        assert np.array_equal(band[2][[0, 1, 3]], base[2][[0, 1, 3]]) and band[2][2] == base[2][2]
    for bin_side in (3, 16):
        other = run(hip, preds, windows, width, height, 4, bin_side=bin_side)
        assert other[0].tobytes() == base[0].tobytes() and other[1].tobytes() == base[1].tobytes() and np.array_equal(other[2], base[2])


def test_malformed_tables_are_refused_before_the_device(hip):
    preds, windows, width, height = chip_scene(11, 8, 8, 4, 4, 2)
    t = og.tile_tables(preds, [og.Window(*w) for w in windows], 2)
    from geograypher_amd.utils.geometric import tile_bin_table

    bins = tile_bin_table(t[2], width, height, 4)
    args = lambda **kw: {**dict(preds=t[0], pred_offsets=t[1], windows=t[2], tile_table=t[3], weights=t[4], weight_offsets=t[5],  # noqa: E731
                                count_dtype=np.uint8, bin_table=bins, width=width, height=height, num_classes=2, nodataval=0), **kw}
    hip.assemble_tiles(**args())
    bad_window = t[2].copy()
    bad_window[1, 0] = width
    bad_bins = (bins[0], np.where(np.arange(len(bins[1])) == 0, len(windows), bins[1]).astype(np.int32)) + bins[2:]
    for kw in (dict(windows=bad_window), dict(bin_table=bad_bins), dict(tile_table=t[3] + 1), dict(pred_offsets=t[1] + 1),
               dict(num_classes=0), dict(num_classes=256), dict(nodataval=256), dict(count_dtype=np.int32), dict(row0=5, n_rows=height)):
        with pytest.raises(ValueError, match="gr_assemble_tiles"):
            hip.assemble_tiles(**args(**kw))


def test_the_library_refuses_bad_arguments_before_any_device_work(hip):
    """GR_EINVAL from the library itself, with a context: the binding's host checks are bypassed (`_rc`).  Every refusal comes
    before the first device call, so null and dangling arguments are never touched."""
    from geograypher_amd import _hip

    stats = hip._stats(_hip.GR_ORTHO_STAT_WORDS, zeroed=True)
    one = hip._zeros((16,), __import__("torch").int64)
    p, s = one.data_ptr(), stats.data_ptr()

    def call(**kw):
        a = dict(preds=p, n_pred=0, pred_offsets=p, windows=p, tile_table=p, T=0, weights=p, n_weights=0, weight_offsets=p, n_tables=0,
                 kind=_hip.GR_COUNT_U8, bin_ptr=p, bin_tiles=p, n_entries=0, side=4, bins_x=1, bins_y=1, width=4, row0=0, n_rows=4, C=2,
                 nodataval=0, classes=p, counts=None, stats=s)
        a.update(kw)
        return hip._rc("gr_assemble_tiles", *a.values(), hip._stream())

    assert call() == _hip.GR_OK and stats.cpu().tolist() == [0, 16, 0, 0]      # no tile: sixteen pixels without a class
    for kw in (dict(C=0), dict(C=256), dict(kind=3), dict(nodataval=256), dict(stats=None), dict(bin_ptr=None), dict(classes=None),
               dict(T=-1), dict(n_rows=-1), dict(side=0), dict(bins_x=0), dict(width=5), dict(row0=1), dict(T=1, windows=None),
               dict(n_pred=1, preds=None), dict(n_entries=1, bin_tiles=None), dict(side=1, bins_x=4, bins_y=1 << 20, n_rows=1 << 19, width=1)):
        assert call(**kw) == _hip.GR_EINVAL, kw
    with pytest.raises(ValueError, match="gr_assemble_tiles: C=0 outside"):
        hip._check(call(C=0), "gr_assemble_tiles")
