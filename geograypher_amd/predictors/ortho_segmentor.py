"""The orthomosaic baseline: cut an orthomosaic into chips, and merge the per-chip class predictions back into one class raster
(reference: geograypher/predictors/ortho_segmentor.py; the rule-set is DESIGN.md section 8m, O1-O8).

The merge runs on the device (`HipRaster.assemble_tiles`, gr_assemble_tiles): every pixel of the extent gathers the (class,
weight) of the tiles that cover it, sums the weights per class in the count type's own arithmetic and takes the lowest class of
the largest sum.  The reference does the same through one file round trip per tile, class and window (rasterio), which is not
installed here.  The host parses the file names, reads the predictions, builds one weight table per tile shape and walks the
extent in bands that fit the device.  There is no CPU fallback: `backend` is a `HipRaster` (default: one on the current device)
or an object with the same `assemble_tiles` method.

Stated divergences: the counts are saved as `.npy` (C, H, W), not as a C-band GeoTIFF; every pixel of the extent is written
(the reference skips blocks that are all nodata, so what such a block reads back as is GDAL's choice); prediction files are
taken in sorted order (the reference's glob order is arbitrary, which matters to the float sums only); a label value of
`write_chips` outside [0, 255] is an error (the reference wraps it), and what GDAL burns for a pixel centre exactly ON a polygon
boundary is not measured."""
import os
import shutil
from collections import namedtuple
from pathlib import Path
from typing import Optional, Union

import numpy as np

from geograypher_amd.constants import NULL_TEXTURE_INT_VALUE, PATH_TYPE
from geograypher_amd.utils.numeric import create_ramped_weighting

Window = namedtuple("Window", ["col_off", "row_off", "width", "height"])
IGNORED_PREDICTION = 255                 # O4: what every prediction value that is no class becomes on the host
DEFAULT_MAX_DEVICE_BYTES = 1 << 30       # device memory a band of the assembly may take
MAX_BAND_ROWS = 65536                    # rows of one launch (the library's grid limit is higher)


def create_windows(dataset_h_w, window_size: int, window_stride: int):
    """Square windows of `window_size` every `window_stride` pixels over a (height, width) raster, columns outermost; windows at
    the far edges reach past the raster."""
    return [Window(col_off, row_off, window_size, window_size)
            for col_off in range(0, dataset_h_w[1], window_stride) for row_off in range(0, dataset_h_w[0], window_stride)]


def get_str_from_window(window, raster_file, suffix: str) -> str:
    """<stem of raster_file>:<col_off>:<row_off>:<width>:<height><suffix> (a dot is put before a suffix without one)."""
    if suffix[0] != ".":
        suffix = "." + suffix
    return f"{Path(raster_file).stem}:{window.col_off}:{window.row_off}:{window.width}:{window.height}{suffix}"


def parse_windows_from_files(files, sep: str = ":", return_in_extent_coords: bool = True):
    """(windows, extent) from file names `<stem><sep><col_off><sep><row_off><sep><width><sep><height><suffix>` (rule O1): the
    extent is the box of all windows; with `return_in_extent_coords` the windows are relative to its corner."""
    if len(files) == 0:
        raise ValueError("no prediction files to parse windows from")
    coords = []
    for file in files:
        parts = Path(file).stem.split(sep)[1:]
        try:
            coords.append([int(v) for v in parts])
        except ValueError:
            parts = None
        if parts is None or len(parts) != 4:
            raise ValueError(f"{Path(file).name} is not <stem>{sep}<col_off>{sep}<row_off>{sep}<width>{sep}<height><suffix>")
    coords = np.asarray(coords, dtype=np.int64)
    xmin, ymin = int(coords[:, 0].min()), int(coords[:, 1].min())
    xmax, ymax = int((coords[:, 0] + coords[:, 2]).max()), int((coords[:, 1] + coords[:, 3]).max())
    extent = Window(col_off=xmin, row_off=ymin, width=xmax - xmin, height=ymax - ymin)
    if return_in_extent_coords:
        coords[:, 0] -= xmin
        coords[:, 1] -= ymin
    return [Window(*(int(v) for v in c)) for c in coords], extent


def pad_to_full_size(img, desired_size):
    """Zero-pad the trailing edge of the leading axes of `img` up to `desired_size`."""
    img = np.asarray(img)
    padding = np.asarray(desired_size) - np.asarray(img.shape[:len(desired_size)])
    if np.sum(padding) > 0:
        img = np.pad(img, [(0, int(p)) for p in padding] + [(0, 0)] * (img.ndim - len(desired_size)))
    return img


def _read_prediction(path) -> np.ndarray:
    if Path(path).suffix.lower() == ".npy":
        return np.load(path)
    from PIL import Image

    with Image.open(path) as image:
        return np.array(image)


def weight_table(shape, downweight_edge_frac: float, count_dtype, max_overlapping_tiles: int) -> np.ndarray:
    """Rule O2: the weights of a tile of `shape` in the count type -- the ramp times iinfo(count_dtype).max /
    max_overlapping_tiles, truncated, for the integer types; the unscaled float64 ramp for float."""
    ramp = create_ramped_weighting(shape, downweight_edge_frac)
    if count_dtype is float or np.dtype(count_dtype) == np.float64:
        return ramp.astype(np.float64)
    return (ramp * (np.iinfo(count_dtype).max / max_overlapping_tiles)).astype(count_dtype)


def tile_tables(preds, windows, num_classes: int, downweight_edge_frac: float = 0.25, count_dtype=np.uint8,
                max_overlapping_tiles: int = 4):
    """The host tables `HipRaster.assemble_tiles` takes, from the tiles' predictions (arrays of any numeric dtype) and their
    windows: (preds uint8 concatenated, pred_offsets (T + 1,) int64, windows (T, 4) int32, tile_table (T,) int32, weights
    concatenated in the count type, weight_offsets (n_tables + 1,) int64).  A prediction whose shape is not (height, width) of its
    window is a ValueError (O1); a value that is not an integer in [0, num_classes) becomes 255 (O4); one weight table per
    distinct shape (O2)."""
    if not 1 <= int(num_classes) <= 255:
        raise ValueError(f"num_classes={num_classes} outside [1, 255]")
    flat, offsets, tables, table_of, tile_table = [], [0], [], {}, []
    for k, (pred, window) in enumerate(zip(preds, windows)):
        pred = np.asarray(pred)
        if pred.shape != (window.height, window.width):
            raise ValueError(f"Size of pred does not match window: tile {k} is {pred.shape}, its window {window.height} x {window.width}")
        if pred.dtype.kind in "ui":
            ok = (pred >= 0) & (pred < num_classes)
        else:
            with np.errstate(invalid="ignore"):
                ok = (pred >= 0) & (pred < num_classes) & (pred == np.floor(pred))
        flat.append(np.where(ok, pred, IGNORED_PREDICTION).astype(np.uint8).reshape(-1))
        offsets.append(offsets[-1] + pred.size)
        if pred.shape not in table_of:
            table_of[pred.shape] = len(tables)
            tables.append(weight_table(pred.shape, downweight_edge_frac, count_dtype, max_overlapping_tiles).reshape(-1))
        tile_table.append(table_of[pred.shape])
    dtype = np.float64 if count_dtype is float else np.dtype(count_dtype)
    return (np.concatenate(flat) if flat else np.zeros(0, np.uint8), np.asarray(offsets, dtype=np.int64),
            np.asarray([tuple(w) for w in windows], dtype=np.int32).reshape(-1, 4), np.asarray(tile_table, dtype=np.int32),
            np.concatenate(tables) if tables else np.zeros(0, dtype), np.cumsum([0] + [len(t) for t in tables]).astype(np.int64))


def band_rows(width: int, height: int, num_classes: int, count_itemsize: int, want_counts: bool, max_overlapping_tiles: int,
              max_device_bytes: int) -> int:
    """Rows of a band (O7): a row of the band costs its class bytes, its counts when asked for, and about
    max_overlapping_tiles x (a prediction byte and its share of nothing else: the weight tables are per shape)."""
    per_row = max(int(width), 1) * (1 + (num_classes * count_itemsize if want_counts else 0) + max(int(max_overlapping_tiles), 1))
    return int(max(1, min(height, MAX_BAND_ROWS, int(max_device_bytes) // per_row)))


def assemble_on_device(backend, tables, width: int, height: int, num_classes: int, nodataval: int, count_dtype=np.uint8,
                       want_counts: bool = False, rows_per_band: Optional[int] = None, bin_side: Optional[int] = None):
    """Walk the extent in bands of `rows_per_band` rows (default: one band) and assemble each from the tiles that meet it:
    -> (classes (height, width) uint8, counts (C, height, width) or None, stats dict summed over the bands -- `longest_list` their
    maximum).  The result does not depend on the band split or the bin side (O6, O7)."""
    from geograypher_amd.utils.geometric import ORTHO_BIN_SIDE, tile_bin_table

    preds, pred_offsets, windows, tile_table, weights, weight_offsets = tables
    rows_per_band = height if rows_per_band is None else max(1, int(rows_per_band))
    side = ORTHO_BIN_SIDE if bin_side is None else int(bin_side)
    classes = np.empty((height, width), dtype=np.uint8)
    counts = np.empty((num_classes, height, width), dtype=weights.dtype) if want_counts else None
    totals = np.zeros(4, dtype=np.int64)
    for row0 in range(0, height, rows_per_band):
        n_rows = min(rows_per_band, height - row0)
        meets = np.nonzero((windows[:, 1] < row0 + n_rows) & (windows[:, 1] + windows[:, 3] > row0))[0]
        if len(meets) == len(windows):
            sub = (preds, pred_offsets, windows, tile_table)
        else:   # only the tiles of this band travel to the device, in their order
            sizes = np.diff(pred_offsets)[meets]
            sub_preds = np.concatenate([preds[pred_offsets[t]:pred_offsets[t + 1]] for t in meets]) if len(meets) else preds[:0]
            sub = (sub_preds, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), windows[meets], tile_table[meets])
        bins = tile_bin_table(sub[2], width, height, side)
        cls_t, cnt_t, stats = backend.assemble_tiles(sub[0], sub[1], sub[2], sub[3], weights, weight_offsets, count_dtype, bins, width,
                                                     height, num_classes, nodataval, row0=row0, n_rows=n_rows, want_counts=want_counts)
        classes[row0:row0 + n_rows] = np.asarray(cls_t.cpu() if hasattr(cls_t, "cpu") else cls_t)
        if want_counts:
            counts[:, row0:row0 + n_rows] = np.asarray(cnt_t.cpu() if hasattr(cnt_t, "cpu") else cnt_t)
        s = np.asarray(stats.cpu() if hasattr(stats, "cpu") else stats, dtype=np.int64)
        totals[[0, 1, 3]] += s[[0, 1, 3]]
        totals[2] = max(totals[2], s[2])
    return classes, counts, dict(with_class=int(totals[0]), without=int(totals[1]), longest_list=int(totals[2]), pairs=int(totals[3]))


def _raster_georeference(raster_file):
    """(transform, epsg) of a GeoTIFF path or a `PlanarRaster`: nothing else of it is read."""
    from geograypher_amd.utils.raster import PlanarRaster, read_geotiff_header

    if isinstance(raster_file, PlanarRaster):
        return raster_file.transform, raster_file.epsg
    transform, _nodata, epsg, _h, _w = read_geotiff_header(raster_file)
    return transform, epsg


def assemble_tiled_predictions(
    raster_file,
    pred_folder: PATH_TYPE,
    class_savefile: PATH_TYPE,
    num_classes: int,
    counts_savefile: Union[PATH_TYPE, None] = None,
    downweight_edge_frac: float = 0.25,
    nodataval: Union[int, None] = NULL_TEXTURE_INT_VALUE,
    count_dtype: type = np.uint8,
    max_overlapping_tiles: int = 4,
    max_device_bytes: int = DEFAULT_MAX_DEVICE_BYTES,
    backend=None,
):
    """Merge the tile predictions of `pred_folder` into one class raster (rules O1-O8 of DESIGN.md 8m).

    raster_file: the GeoTIFF the chips were cut from, or a `PlanarRaster`; only its transform and EPSG code are read.
    pred_folder: every file is the prediction of one tile, `.npy` or an image, named as `get_str_from_window` names chips.
    class_savefile: the merged classes, a deflate GeoTIFF (uint8, GDAL_NODATA = nodataval) with the transform of the extent.
    counts_savefile: the per-class sums as `.npy` (C, H, W) in `count_dtype`; any other suffix is a NotImplementedError.
    downweight_edge_frac: the outer fraction of every tile is down-weighted along a linear ramp (the outermost ring weighs 0).
    nodataval: the value of pixels without a prediction; None: num_classes.  The default 0 cannot be told from class 0.
    count_dtype: np.uint8, np.uint16 (sums wrap modulo 2^8 / 2^16) or float.
    max_overlapping_tiles: scales the integer weights so that this many full-weight tiles do not wrap.
    max_device_bytes: the extent is assembled in bands of rows sized to this much device memory.
    Returns (classes (H, W) uint8, extent Window in the coordinates of `raster_file`)."""
    from geograypher_amd.utils.tiff import write_tiff_deflate

    pred_files = sorted(f for f in Path(pred_folder).glob("*") if f.is_file())
    if counts_savefile is not None and Path(counts_savefile).suffix.lower() != ".npy":
        raise NotImplementedError(f"counts_savefile {counts_savefile}: the counts are saved as .npy (C, H, W); a C-band GeoTIFF is not written")
    if nodataval is None:
        nodataval = num_classes
    if not 0 <= int(nodataval) <= 255:
        raise ValueError(f"nodataval={nodataval} does not fit the uint8 class raster")
    windows, extent = parse_windows_from_files(pred_files, return_in_extent_coords=True)
    tables = tile_tables([_read_prediction(f) for f in pred_files], windows, num_classes, downweight_edge_frac, count_dtype,
                         max_overlapping_tiles)
    (a, b, c, d, e, f), epsg = _raster_georeference(raster_file)
    if backend is None:
        from geograypher_amd._hip import HipRaster

        backend = HipRaster()
    want_counts = counts_savefile is not None
    rows = band_rows(extent.width, extent.height, num_classes, tables[4].dtype.itemsize, want_counts, max_overlapping_tiles, max_device_bytes)
    classes, counts, _stats = assemble_on_device(backend, tables, extent.width, extent.height, num_classes, int(nodataval), count_dtype,
                                                 want_counts=want_counts, rows_per_band=rows)
    extent_transform = (a, b, a * extent.col_off + b * extent.row_off + c, d, e, d * extent.col_off + e * extent.row_off + f)
    Path(class_savefile).parent.mkdir(parents=True, exist_ok=True)
    write_tiff_deflate(class_savefile, classes, transform=extent_transform, nodata=int(nodataval), epsg=epsg)
    if want_counts:
        Path(counts_savefile).parent.mkdir(parents=True, exist_ok=True)
        np.save(counts_savefile, counts)
    return classes, extent


class _ChipLabels:
    """The label polygons of `write_chips` on the device: one ring table in the cell units of the raster's grid, one `PolygonBurner`."""

    def __init__(self, label_vector_file, label_column, label_remap, transform, epsg, backend):
        from geograypher_amd.utils.geometric import PlanarPolygons, row_centre_boxes, row_ring_ranges
        from geograypher_amd.utils.geospatial import burn_values, rings_in_raster_CRS, rings_to_cell_units
        from geograypher_amd.utils.raster import invert_affine

        polygons, properties = PlanarPolygons.from_geojson(label_vector_file)
        P = len(polygons)
        if label_column is None:
            values = list(range(P))            # the reference's index: the feature number
        elif label_column in properties:
            values = properties[label_column].tolist()
        else:
            raise ValueError(f"label_vector_file {label_vector_file} has no column {label_column!r} (it has {sorted(properties)})")
        if label_remap is not None:
            missing = [v for v in values if v not in label_remap]
            if missing:
                raise ValueError(f"label_remap has no entry for {missing[0]!r}")
            values = [label_remap[v] for v in values]
        values = burn_values(values, P)
        if backend is None:
            from geograypher_amd._hip import HipRaster

            backend = HipRaster()
        rv, off = rings_to_cell_units(rings_in_raster_CRS(polygons, epsg, backend), invert_affine(transform))
        rp = np.asarray(polygons.ring_polygon, dtype=np.int32)
        self.burner = backend.polygon_burner(rv, off, rp, P, values)
        self.boxes, self.ranges = row_centre_boxes(rv, off, rp, P), row_ring_ranges(rp, P)

    def label(self, window, background_ind: int, keep_empty: bool):
        """The (height, width) uint8 label of a window, or None for one that is all NULL_TEXTURE_INT_VALUE unless `keep_empty`.
        Where the background is that constant, a window without a burned cell is known empty from the statistics word alone and
        its plane is not copied back."""
        from geograypher_amd._hip import GR_BURN_STAT_BURNED
        from geograypher_amd.utils.geometric import burn_work_items
        from geograypher_amd.utils.geospatial import _to_host

        items = burn_work_items(self.boxes, self.ranges, tuple(window))
        _rows, out, stats = self.burner.window(*window, items, fill=background_ind, want_values=True)
        if not keep_empty and background_ind == NULL_TEXTURE_INT_VALUE and int(_to_host(stats)[GR_BURN_STAT_BURNED]) == 0:
            return None
        label = _to_host(out).astype(np.uint8, copy=False)
        if not keep_empty and np.all(label == NULL_TEXTURE_INT_VALUE):
            return None
        return label


class _ChipRegion:
    """The region of interest of `write_chips`: the edges of its polygons in the cell units of the raster's grid (Z1)."""

    def __init__(self, ROI_file, transform, epsg, backend):
        from geograypher_amd.utils.geometric import PlanarPolygons, ring_edges
        from geograypher_amd.utils.geospatial import rings_in_raster_CRS, rings_to_cell_units
        from geograypher_amd.utils.raster import invert_affine

        polygons, _ = PlanarPolygons.from_geojson(ROI_file)
        rv, off = rings_to_cell_units(rings_in_raster_CRS(polygons, epsg, backend), invert_affine(transform))
        self.edges, self.edge_row = ring_edges(rv, off, polygons.ring_polygon)

    def meets(self, window) -> bool:
        from geograypher_amd.utils.geometric import rectangle_meets_rows

        return rectangle_meets_rows(self.edges, self.edge_row, (65536 * window.col_off, 65536 * window.row_off,
                                                                65536 * (window.col_off + window.width),
                                                                65536 * (window.row_off + window.height)))


def write_chips(
    raster_file: PATH_TYPE,
    output_folder: PATH_TYPE,
    chip_size: int,
    chip_stride: int,
    label_vector_file: Optional[PATH_TYPE] = None,
    label_column: Optional[str] = None,
    label_remap: Optional[dict] = None,
    write_empty_tiles: bool = False,
    drop_transparency: bool = True,
    remove_old: bool = True,
    output_suffix: str = ".JPG",
    ROI_file: Optional[PATH_TYPE] = None,
    background_ind: int = NULL_TEXTURE_INT_VALUE,
    backend=None,
):
    """Cut the image `raster_file` into square chips of `chip_size` every `chip_stride` pixels and write them to `output_folder`,
    named by their window (`get_str_from_window`).  Chips at the far edges are zero-padded to full size.  With
    `drop_transparency` a fourth band is dropped, its transparent pixels turned black, and a chip that is all transparent is
    not written.  `remove_old` removes `output_folder` first.  Returns the image files written.

    label_vector_file (a `.geojson`; the raster must then be a georeferenced GeoTIFF): training data as the reference writes it --
    the imagery goes to `output_folder/imgs`, and beside it `output_folder/anns/<window name>.png` holds the polygons burned into
    the chip's window on the device (one `PolygonBurner` for the file, one window call per chip; rules B1-B7 of DESIGN.md 8m in
    place of rasterio.features.rasterize): the value of the last feature that holds a pixel's centre, `background_ind` elsewhere,
    past the raster's edge too.  The values are `label_column` of the features, else the feature number, mapped through
    `label_remap` when given; every value must be an integer in [0, 255] (ValueError: the reference's astype(np.uint8) wraps).
    Labels in another CRS than the raster's are reprojected vertex by vertex.  Without `write_empty_tiles` a chip whose label is
    all NULL_TEXTURE_INT_VALUE is skipped (the reference compares with the constant, not with `background_ind`).
    ROI_file (a `.geojson`): a chip is written iff its window rectangle intersects the union of the ROI's polygons, touching
    included (`rectangle_meets_rows`: exact, on the host).  As in the reference the labels are NOT clipped to the ROI: it builds
    its label shapes before its clip takes effect.
    A vector file that is no `.geojson`, or a raster that is no georeferenced GeoTIFF beside one, is a NotImplementedError before
    anything is removed or read.  `backend`: a `HipRaster` (default: one on the current device) or an object with its
    `polygon_burner` (and `reproject_points`) method; without labels there is no device work."""
    from PIL import Image

    vector_files = [(name, file) for name, file in (("label_vector_file", label_vector_file), ("ROI_file", ROI_file)) if file is not None]
    burner = roi = None
    if vector_files:
        names = " / ".join(name for name, _ in vector_files)
        for name, file in vector_files:
            if Path(file).suffix.lower() != ".geojson":
                raise NotImplementedError(f"{name} {file}: vector files are read as .geojson only")
        if Path(raster_file).suffix.lower() not in (".tif", ".tiff"):
            raise NotImplementedError(f"{names}: {raster_file} is not a GeoTIFF; labels and regions need a georeferenced raster")
        from geograypher_amd.utils.raster import read_geotiff_header

        try:
            transform, _nodata, epsg, _height, _width = read_geotiff_header(raster_file)
        except ValueError as error:
            raise NotImplementedError(f"{names}: labels and regions need a georeferenced raster ({error})") from error
        if not 0 <= int(background_ind) <= 255:
            raise ValueError(f"background_ind={background_ind} does not fit the uint8 label raster")
        if label_vector_file is not None:
            burner = _ChipLabels(label_vector_file, label_column, label_remap, transform, epsg, backend)
        if ROI_file is not None:
            roi = _ChipRegion(ROI_file, transform, epsg, backend)
    if remove_old and os.path.isdir(output_folder):
        shutil.rmtree(output_folder)
    labels_folder = None
    if burner is not None:
        labels_folder, output_folder = Path(output_folder, "anns"), Path(output_folder, "imgs")
        labels_folder.mkdir(parents=True, exist_ok=True)
    Path(output_folder).mkdir(parents=True, exist_ok=True)
    limit, Image.MAX_IMAGE_PIXELS = Image.MAX_IMAGE_PIXELS, None
    try:
        with Image.open(raster_file) as image:
            img = np.array(image)
    finally:
        Image.MAX_IMAGE_PIXELS = limit
    if img.ndim == 2:
        img = img[:, :, None]
    written = []
    for window in create_windows(img.shape[:2], chip_size, chip_stride):
        if roi is not None and not roi.meets(window):
            continue
        if burner is not None:
            label = burner.label(window, int(background_ind), keep_empty=write_empty_tiles)
            if label is None:
                continue
            Image.fromarray(label).save(Path(labels_folder, get_str_from_window(window, raster_file, ".png")), format="PNG")
        chip = img[window.row_off:window.row_off + window.height, window.col_off:window.col_off + window.width].copy()
        if drop_transparency and chip.shape[2] == 4:
            transparent = chip[..., 3] == 0
            chip = chip[..., :3]
            if np.all(transparent):
                continue
            chip[transparent, :] = 0
        chip = pad_to_full_size(chip, (chip_size, chip_size))
        name = Path(output_folder, get_str_from_window(window, raster_file, output_suffix))
        fmt = {".jpg": "JPEG", ".jpeg": "JPEG", ".png": "PNG", ".tif": "TIFF", ".tiff": "TIFF"}.get(name.suffix.lower())
        Image.fromarray(chip[:, :, 0] if chip.shape[2] == 1 else chip).save(name, format=fmt)
        written.append(name)
    return written
