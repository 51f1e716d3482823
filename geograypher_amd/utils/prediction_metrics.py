"""Scores of the orthomosaic baseline: the confusion matrix of a class raster against ground-truth polygons, and the metrics of a
confusion matrix (reference: geograypher/utils/prediction_metrics.py).  The cells under every truth polygon are counted on the
device (`utils.geospatial.zonal_class_counts`, gr_zonal_class_counts) in place of rasterstats.zonal_stats;
the confusion matrix of two label lists is plain numpy in place of scikit-learn.  Not carried over: the plots."""
import typing
from pathlib import Path

import numpy as np

from geograypher_amd.constants import CLASS_NAMES_KEY, PATH_TYPE


def check_if_raster(filename) -> bool:
    extension = Path(filename).suffix.lower()
    if extension in (".tif", ".tiff"):
        return True
    if extension in (".geojson", ".shp"):
        return False
    raise ValueError("Unknown extension")


def compute_confusion_matrix_from_geospatial(
    prediction_file,
    groundtruth_file: PATH_TYPE,
    class_names: typing.List[str],
    vis_raster_file: typing.Union[PATH_TYPE, None] = None,
    vis_savefile: typing.Optional[str] = None,
    vis: bool = False,
    normalize: bool = True,
    remap_raster_inds=None,
    column_name: str = CLASS_NAMES_KEY,
    backend=None,
):
    """The confusion matrix of a predicted class raster against ground-truth polygons -> (cf_matrix (n + 1, n + 1) float64,
    the class names with "unlabeled" appended -- a NEW list, the caller's is left alone --, accuracy = trace / sum).

    prediction_file: a class raster, a GeoTIFF path (`.tif`) or a `PlanarRaster`; a vector prediction is a NotImplementedError.
    groundtruth_file: a `.geojson` with ONE feature per class name in the property `column_name`, in the raster's CRS; a name
    that occurs twice is a ValueError (dissolve the file by that column first), a name that is absent gives a row of zeros.
    cf[i][j] = the cells of truth class i whose raster value is j, j < len(class_names); then the columns are permuted by
    `remap_raster_inds`, a zero "unlabeled" row and column are appended, and `normalize` divides by the sum.  vis=True is a
    NotImplementedError."""
    from geograypher_amd.utils.geometric import PlanarPolygons
    from geograypher_amd.utils.geospatial import zonal_class_counts
    from geograypher_amd.utils.raster import PlanarRaster

    if vis or vis_raster_file is not None or vis_savefile is not None:
        raise NotImplementedError("vis: the plots need matplotlib, which is outside the device path")
    if not isinstance(prediction_file, PlanarRaster) and not check_if_raster(prediction_file):
        raise NotImplementedError("a vector prediction needs polygon intersections, which are not available: predict a class raster")
    if check_if_raster(groundtruth_file):
        raise NotImplementedError("a raster ground truth is not supported (nor is it by the reference)")
    if Path(groundtruth_file).suffix.lower() != ".geojson":
        raise NotImplementedError(f"{groundtruth_file}: ground truth is read as .geojson only")
    polygons, properties = PlanarPolygons.from_geojson(groundtruth_file)
    if column_name not in properties:
        raise ValueError(f"{groundtruth_file} has no property {column_name!r}")
    names = list(properties[column_name])
    n = len(class_names)
    counts, _ = zonal_class_counts(polygons, prediction_file, num_classes=None, backend=backend)
    cf_matrix = np.zeros((n, n), dtype=np.float64)
    for i, name in enumerate(class_names):
        rows = [k for k, v in enumerate(names) if v == name]
        if len(rows) > 1:
            raise ValueError(f"class {name!r} has {len(rows)} features in {groundtruth_file}: dissolve the file by {column_name!r} "
                             "so that every class is one (multi)polygon")
        if rows:
            row = counts[rows[0], :n]
            cf_matrix[i, :len(row)] = row
    if remap_raster_inds is not None:
        cf_matrix = cf_matrix[:, tuple(remap_raster_inds)]
    cf_matrix = np.pad(cf_matrix, pad_width=((0, 1), (0, 1)))
    if normalize:
        cf_matrix = cf_matrix / cf_matrix.sum()
    accuracy = np.sum(cf_matrix * np.eye(cf_matrix.shape[0])) / np.sum(cf_matrix)
    return cf_matrix, list(class_names) + ["unlabeled"], accuracy


def compute_and_show_cf(
    pred_labels: list,
    gt_labels: list,
    labels: typing.Union[None, typing.List[str]] = None,
    use_labels_from: str = "both",
    vis: bool = False,
    cf_plot_savefile: typing.Union[None, PATH_TYPE] = None,
    cf_np_savefile: typing.Union[None, PATH_TYPE] = None,
):
    """The confusion matrix of two label lists -> (cf_matrix (n, n) int64 with cf[i][j] = samples of true label labels[i]
    predicted as labels[j], labels, accuracy).  labels=None: the sorted distinct labels of `gt`, `pred` or `both`.  Samples
    whose true or predicted label is not among `labels` are left out, as scikit-learn's confusion_matrix does.  vis=True and
    cf_plot_savefile are a NotImplementedError; cf_np_savefile saves the matrix as `.npy`."""
    if vis or cf_plot_savefile is not None:
        raise NotImplementedError("vis: the plot needs matplotlib, which is outside the device path")
    if labels is None:
        if use_labels_from == "gt":
            labels = np.unique(list(gt_labels))
        elif use_labels_from == "pred":
            labels = np.unique(list(pred_labels))
        elif use_labels_from == "both":
            labels = np.unique(list(pred_labels) + list(gt_labels))
        else:
            raise ValueError(f"Must use labels from gt, pred, or both but instead was {use_labels_from}")
    if len(pred_labels) != len(gt_labels):
        raise ValueError(f"{len(pred_labels)} predicted labels and {len(gt_labels)} true labels")
    index = {label: k for k, label in enumerate(np.asarray(labels).tolist())}
    cf_matrix = np.zeros((len(index), len(index)), dtype=np.int64)
    for true, pred in zip(np.asarray(list(gt_labels)).tolist(), np.asarray(list(pred_labels)).tolist()):
        if true in index and pred in index:
            cf_matrix[index[true], index[pred]] += 1
    if cf_np_savefile:
        Path(cf_np_savefile).parent.mkdir(parents=True, exist_ok=True)
        np.save(cf_np_savefile, cf_matrix)
    accuracy = np.sum(cf_matrix * np.eye(cf_matrix.shape[0])) / np.sum(cf_matrix)
    return cf_matrix, labels, accuracy


def compute_comprehensive_metrics(cf_matrix: np.ndarray, class_names: typing.List[str]) -> dict:
    """Accuracy, class-averaged recall and precision (over the classes with a true sample; a precision of 0 / 0 counts as 0),
    and per class: acc = (TP + TN) / total, recall = TP / num_true, precision = TP / num_pred, num_true, num_pred.  A class
    without a true (predicted) sample has a NaN recall (precision)."""
    cf_matrix = np.asarray(cf_matrix)
    total = np.sum(cf_matrix)
    accuracy = np.sum(cf_matrix * np.eye(cf_matrix.shape[0])) / total
    per_class = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, class_name in zip(range(cf_matrix.shape[0]), class_names):
            true_positives = cf_matrix[i, i]
            num_true = np.sum(cf_matrix[i, :])
            num_pred = np.sum(cf_matrix[:, i])
            true_negatives = total + true_positives - num_true - num_pred
            per_class[class_name] = {
                "acc": (true_positives + true_negatives) / total,
                "recall": true_positives / num_true,
                "precision": true_positives / num_pred,
                "num_true": num_true,
                "num_pred": num_pred,
            }
    precisions = np.nan_to_num(np.array([v["precision"] for v in per_class.values()]))
    recalls = np.array([v["recall"] for v in per_class.values()])
    any_trues = np.array([v["num_true"] for v in per_class.values()]) > 0
    return {
        "accuracy": accuracy,
        "class_averaged_recall": np.mean(recalls[any_trues]),
        "class_averaged_precision": np.mean(precisions[any_trues]),
        "per_class": per_class,
    }
