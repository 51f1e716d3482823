"""tests/golden/make_golden_ortho.py -- goldens of the orthomosaic baseline, made by the REAL reference functions
(geograypher/utils/numeric.py, utils/prediction_metrics.py, predictors/ortho_segmentor.py); the modules the reference imports but
cannot find here are stubbed as in SURVEY.md Appendix B:

    PYTHONPATH=<reference checkout> python tests/golden/make_golden_ortho.py

Output: tests/golden/ortho_baseline.npz -- data only.
  ramp__<rows>x<cols>__<frac>            create_ramped_weighting; the 512 x 512 ones as their 16 x 16 corners __tl and __br
  metrics__<k>__cf / __names / __summary / __per_class
                                         compute_comprehensive_metrics: (accuracy, class_averaged_recall, class_averaged_precision)
                                         and per class (acc, recall, precision, num_true, num_pred)
  cf__<k>__pred / __gt / __labels_in / __matrix / __labels / __accuracy
                                         compute_and_show_cf(vis=False); __labels_in is empty for labels=None (use_labels_from in
                                         the case's name)
  tiles__preds / __windows               five 8 x 8 predictions in 0..3 and their windows (col_off, row_off, width, height)
  asm__<uint8|float|uint16>__classes / __counts
                                         the reference's assemble_tiled_predictions over them, 3 classes, default nodataval
rasterio is not installed: `rasterio.open` and `Window` are replaced by the in-memory stand-in below (arrays in a dict, blocks of
three rows, so that every block holds a pixel with data and the reference's skipping of all-nodata blocks plays no part), and
imageio.imread fails, so that the reference reads the `.npy` tiles with np.load."""
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(HERE))
OUT = HERE / "ortho_baseline.npz"

from make_golden_tabular import stub_missing_modules  # noqa: E402

RAMP_SHAPES = ((8, 6), (4, 4), (1, 3), (2, 2), (9, 9), (512, 512))
RAMP_FRACS = (0.25, 0.5, 0.1, 1.0)
TILE_CORNERS = ((0, 0), (4, 0), (0, 4), (4, 4), (2, 2))
STORE = {}


class Window:
    def __init__(self, col_off, row_off, width, height):
        self.col_off, self.row_off, self.width, self.height = int(col_off), int(row_off), int(width), int(height)


class Dataset:
    """What the reference's assemble_tiled_predictions uses of a rasterio dataset, over arrays kept in STORE."""

    def __init__(self, name, mode="r", height=None, width=None, count=None, dtype=None, nodata=None, **_):
        self.name = str(name)
        if mode.startswith("w"):
            STORE[self.name] = dict(data=np.zeros((count, height, width), dtype=dtype), nodata=nodata)
        self.rec = STORE.get(self.name, dict(data=np.zeros((1, 1, 1)), nodata=None))
        self.crs, self.transform = "crs", "transform"

    shape = property(lambda self: self.rec["data"].shape[1:])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def window_transform(self, window):
        return ("transform", window.col_off, window.row_off)

    @staticmethod
    def _slices(window):
        return slice(window.row_off, window.row_off + window.height), slice(window.col_off, window.col_off + window.width)

    def read(self, band=None, window=None):
        data = self.rec["data"] if band is None else self.rec["data"][band - 1]
        return data[(Ellipsis,) + self._slices(window)].copy()

    def write(self, array, band, window=None):
        self.rec["data"][band - 1][self._slices(window)] = array

    def block_windows(self):
        h, w = self.shape
        return [((0, i), Window(0, r, w, min(3, h - r))) for i, r in enumerate(range(0, h, 3))]


def main():
    stub_missing_modules()
    import imageio
    import rasterio
    import rasterio.windows

    rasterio.open = lambda name, mode="r", **kw: Dataset(name, mode, **kw)
    rasterio.windows.Window = Window
    imageio.imread.side_effect = OSError("not an image")
    import geograypher.predictors.ortho_segmentor as ref_ortho
    from geograypher.utils.numeric import create_ramped_weighting
    from geograypher.utils.prediction_metrics import compute_and_show_cf, compute_comprehensive_metrics

    ref_ortho.Window = Window
    out = {}
    for shape in RAMP_SHAPES:
        for frac in RAMP_FRACS:
            ramp = create_ramped_weighting(shape, frac)
            key = f"ramp__{shape[0]}x{shape[1]}__{frac}"
            if shape[0] > 16:
                out[key + "__tl"], out[key + "__br"] = ramp[:16, :16].copy(), ramp[-16:, -16:].copy()
            else:
                out[key] = ramp

    matrices = [
        (np.array([[3.0, 1, 0], [2, 4, 0], [0, 0, 0]]), ["a", "b", "c"]),          # class c: no true and no predicted sample
        (np.array([[5.0, 0], [0, 7]]), ["x", "y"]),
        (np.array([[0.2, 0.1, 0.0, 0.0], [0.05, 0.3, 0.05, 0.0], [0.0, 0.1, 0.2, 0.0], [0.0, 0.0, 0.0, 0.0]]), ["p", "q", "r", "unlabeled"]),
        (np.array([[2, 0, 1], [0, 0, 3], [4, 0, 6]]), ["u", "v", "w"]),             # class v: true samples, never predicted
    ]
    for k, (cf, names) in enumerate(matrices):
        with np.errstate(invalid="ignore", divide="ignore"):
            m = compute_comprehensive_metrics(cf, names)
        out[f"metrics__{k}__cf"], out[f"metrics__{k}__names"] = cf, np.array(names)
        out[f"metrics__{k}__summary"] = np.array([m["accuracy"], m["class_averaged_recall"], m["class_averaged_precision"]], dtype=np.float64)
        out[f"metrics__{k}__per_class"] = np.array([[m["per_class"][n][f] for f in ("acc", "recall", "precision", "num_true", "num_pred")]
                                                    for n in names], dtype=np.float64)

    label_cases = [
        ("both", ["a", "b", "a", "c", "b", "a"], ["a", "a", "a", "c", "b", "b"], None),
        ("gt", ["a", "b", "d", "c", "b", "a"], ["a", "a", "a", "c", "b", "b"], None),
        ("pred", [2, 0, 1, 1, 2, 2, 0], [2, 1, 1, 0, 2, 3, 0], None),
        ("both", ["a", "b", "a"], ["a", "b", "b"], ["b", "a", "z"]),
    ]
    try:
        for k, (source, pred, gt, labels) in enumerate(label_cases):
            matrix, labels_out, accuracy = compute_and_show_cf(pred, gt, labels=labels, use_labels_from=source, vis=False)
            out[f"cf__{k}__{source}__pred"], out[f"cf__{k}__{source}__gt"] = np.array(pred), np.array(gt)
            out[f"cf__{k}__{source}__labels_in"] = np.array([] if labels is None else labels)
            out[f"cf__{k}__{source}__matrix"], out[f"cf__{k}__{source}__labels"] = np.asarray(matrix), np.asarray(labels_out)
            out[f"cf__{k}__{source}__accuracy"] = np.float64(accuracy)
    except Exception as exc:   # scikit-learn missing: its confusion_matrix is a stub then
        raise SystemExit(f"compute_and_show_cf did not run against a real scikit-learn: {exc!r}")

    rng = np.random.default_rng(0)
    preds = np.stack([rng.integers(0, 4, (8, 8)).astype(np.uint8) for _ in TILE_CORNERS])
    out["tiles__preds"] = preds
    out["tiles__windows"] = np.array([(c, r, 8, 8) for c, r in TILE_CORNERS], dtype=np.int64)
    for name, dtype in (("uint8", np.uint8), ("float", float), ("uint16", np.uint16)):
        STORE.clear()
        tmp = Path(tempfile.mkdtemp())
        folder = tmp / "pred"
        folder.mkdir()
        for (c, r), pred in zip(TILE_CORNERS, preds):
            np.save(folder / f"ortho:{c}:{r}:8:8.npy", pred)
        ref_ortho.assemble_tiled_predictions(tmp / "ortho.tif", folder, tmp / "cls.tif", num_classes=3, counts_savefile=tmp / "cnt.tif",
                                             count_dtype=dtype)
        counts = STORE[str(tmp / "cnt.tif")]["data"]
        classes = STORE[str(tmp / "cls.tif")]
        assert classes["nodata"] == 0 and counts.shape == (3, 12, 12)
        for _, block in Dataset(tmp / "cnt.tif").block_windows():   # no block is all nodata: nothing was skipped
            assert np.any(counts[:, block.row_off:block.row_off + block.height].sum(axis=0) != 0)
        out[f"asm__{name}__classes"], out[f"asm__{name}__counts"] = classes["data"][0].astype(np.uint8), counts
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
