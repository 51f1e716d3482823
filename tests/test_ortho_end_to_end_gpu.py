"""The orthomosaic baseline end to end on the device: an orthomosaic GeoTIFF is cut into chips, a stand-in model predicts a class
per chip pixel, `assemble_tiled_predictions` merges the predictions in several bands on the device and writes the class GeoTIFF,
and the confusion matrix against ground-truth polygons is counted on the device from that file.  Every step is compared with the
stand-ins (exact equality)."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import ortho_standin as osn  # noqa: E402
import zonal_standin as zs  # noqa: E402
from geograypher_amd.predictors import ortho_segmentor as og  # noqa: E402
from geograypher_amd.utils import prediction_metrics as pm  # noqa: E402
from geograypher_amd.utils.geospatial import get_overlap_raster  # noqa: E402
from geograypher_amd.utils.raster import PlanarRaster  # noqa: E402
from geograypher_amd.utils.tiff import write_tiff_deflate  # noqa: E402

pytestmark = pytest.mark.gpu
TRANSFORM = (0.5, 0.0, 600000.0, 0.0, -0.5, 4200000.0)


def test_chips_to_confusion_matrix(hip, tmp_path):
    rng = np.random.default_rng(0)
    H, W, C = 40, 52, 3
    truth_classes = np.zeros((H, W), np.uint8)
    truth_classes[:, 20:] = 1
    truth_classes[25:, 10:40] = 2
    image = np.stack([truth_classes * 80 + 20, np.full((H, W), 90, np.uint8), np.full((H, W), 30, np.uint8)], axis=2).astype(np.uint8)
    write_tiff_deflate(tmp_path / "site.tif", image, transform=TRANSFORM, epsg=32610)
    chips = og.write_chips(tmp_path / "site.tif", tmp_path / "chips", 16, 8, output_suffix=".png")
    assert len(chips) == 7 * 5
    from PIL import Image

    preds_folder = tmp_path / "preds"
    preds_folder.mkdir()
    for chip in chips:   # the "model": the class from the red band, a few pixels wrong, the padding unlabeled
        red = np.array(Image.open(chip))[..., 0].astype(np.int64)
        pred = np.where(rng.random(red.shape) < 0.1, rng.integers(0, C, red.shape), (red - 20) // 80)
        pred = np.where(red == 0, 255, pred)
        np.save(preds_folder / (chip.stem + ".npy"), pred.astype(np.uint8))
    classes, extent = og.assemble_tiled_predictions(tmp_path / "site.tif", preds_folder, tmp_path / "out" / "classes.tif", C,
                                                    counts_savefile=tmp_path / "out" / "counts.npy", nodataval=255,
                                                    max_device_bytes=4000, backend=hip)
    assert tuple(extent) == (0, 0, 64, 48)
    files = sorted(preds_folder.glob("*"))
    windows, _ = og.parse_windows_from_files(files)
    want_classes, want_counts, _ = osn.assemble([np.load(f) for f in files], [tuple(w) for w in windows], 64, 48, C, 255)
    assert np.array_equal(classes, want_classes) and np.array_equal(np.load(tmp_path / "out" / "counts.npy"), want_counts)
    merged = PlanarRaster.from_geotiff(tmp_path / "out" / "classes.tif")
    assert np.array_equal(merged.data[0], classes) and merged.transform == TRANSFORM and merged.nodata == 255.0 and merged.epsg == 32610
    assert (classes[2:38, 2:50] == truth_classes[2:38, 2:50]).mean() > 0.95 and np.all(classes[40:] == 255)

    # ground truth: one (multi)polygon per class, in the raster's CRS
    def world(c0, r0, c1, r1):
        return [[600000.0 + 0.5 * c, 4200000.0 - 0.5 * r] for c, r in ((c0, r0), (c1, r0), (c1, r1), (c0, r1), (c0, r0))]

    features = [("zero", [[world(0, 0, 20, 25)], [world(0, 25, 10, 40)]]), ("one", [[world(20, 0, 52, 25)], [world(40, 25, 52, 40)]]),
                ("two", [[world(10, 25, 40, 40)]])]
    truth = tmp_path / "truth.geojson"
    truth.write_text(json.dumps({"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {"class_names": n}, "geometry": {"type": "MultiPolygon", "coordinates": parts}} for n, parts in features]}))
    names = ["zero", "one", "two"]
    cf, out_names, accuracy = pm.compute_confusion_matrix_from_geospatial(tmp_path / "out" / "classes.tif", truth, names, normalize=False, backend=hip)
    want = pm.compute_confusion_matrix_from_geospatial(tmp_path / "out" / "classes.tif", truth, names, normalize=False, backend=zs.StandInBackend())
    assert out_names == names + ["unlabeled"] and np.array_equal(cf, want[0]) and accuracy == want[2] and accuracy > 0.9
    by_hand = np.zeros((4, 4))
    for t in range(3):
        by_hand[t, :3] = np.bincount(classes[:40, :52][(truth_classes == t) & (classes[:40, :52] != 255)], minlength=3)
    assert np.array_equal(cf, by_hand)
    matrix, valid = get_overlap_raster(truth, tmp_path / "out" / "classes.tif", backend=hip)
    assert valid.tolist() == [0, 1, 2] and np.array_equal(matrix, by_hand[:3, :3])
