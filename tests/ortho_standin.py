"""Rules O1-O5 of DESIGN.md 8m in plain numpy, written as the reference's loop over tiles and classes
(predictors/ortho_segmentor.py:346-431): the stand-in the device's tile assembly is compared with.  tests/test_ortho_baseline_host.py
pins it to the outputs of the real reference (tests/golden/ortho_baseline.npz), which ties the GPU tests to the reference."""
import numpy as np

from geograypher_amd.utils.numeric import create_ramped_weighting


def weights_for(shape, downweight_edge_frac, count_dtype, max_overlapping_tiles):
    """O2, restated: the ramp, scaled and truncated for the integer count types."""
    ramp = create_ramped_weighting(shape, downweight_edge_frac)
    if count_dtype is not float:
        ramp = ramp * (np.iinfo(count_dtype).max / max_overlapping_tiles)
    return ramp.astype(count_dtype)


def assemble(preds, windows, width, height, num_classes, nodataval=0, downweight_edge_frac=0.25, count_dtype=np.uint8,
             max_overlapping_tiles=4, rows=None, tables=None):
    """preds: the tiles' predictions as read from disk, in ascending tile index; windows: (col_off, row_off, width, height) in
    extent coordinates -> (classes (H, W) uint8, counts (C, H, W) count_dtype, stats (4,) int64: pixels with a class, without,
    most tiles over a pixel, (tile, pixel) pairs -- over the rows [rows[0], rows[0] + rows[1]) when given, else all).  tables:
    ready-made weight tables per tile, in place of O2."""
    if nodataval is None:
        nodataval = num_classes
    counts = np.zeros((num_classes, height, width), dtype=count_dtype)
    cover = np.zeros((height, width), dtype=np.int64)
    table = {}
    for t, (pred, (col, row, w, h)) in enumerate(zip(preds, windows)):
        pred = np.asarray(pred)
        if pred.shape != (h, w):
            raise ValueError("Size of pred does not match window")
        if pred.shape not in table:
            table[pred.shape] = weights_for(pred.shape, downweight_edge_frac, count_dtype, max_overlapping_tiles)
        weighting = table[pred.shape] if tables is None else tables[t]
        cover[row:row + h, col:col + w] += 1
        for c in range(num_classes):
            mask = pred == c
            if not np.any(mask):
                continue
            counts[c, row:row + h, col:col + w] += (mask * weighting).astype(count_dtype)   # wraps for the unsigned types
    nodata = np.sum(counts, axis=0) == 0
    classes = np.argmax(counts, axis=0)
    classes[nodata] = nodataval
    band = slice(None) if rows is None else slice(rows[0], rows[0] + rows[1])
    stats = np.array([np.sum(~nodata[band]), np.sum(nodata[band]), cover[band].max() if cover[band].size else 0, cover[band].sum()],
                     dtype=np.int64)
    return classes.astype(np.uint8), counts, stats


class StandInBackend:
    """`HipRaster.assemble_tiles` on the host, from the same tables, through `assemble`: for the host tests of the driver
    (`assemble_on_device`, `assemble_tiled_predictions`)."""

    def __init__(self):
        self.calls = []

    def assemble_tiles(self, preds, pred_offsets, windows, tile_table, weights, weight_offsets, count_dtype, bin_table, width, height,
                       num_classes, nodataval, row0=0, n_rows=None, want_counts=False):
        from geograypher_amd import _hip

        n_rows = height - row0 if n_rows is None else n_rows
        bin_ptr, bin_tiles, side, bins_x, bins_y = bin_table
        _hip.check_assemble_tables(pred_offsets, windows, tile_table, weight_offsets, len(preds), len(weights), bin_ptr, bin_tiles, side,
                                   bins_x, bins_y, width, height, row0, n_rows, num_classes, nodataval)
        self.calls.append((row0, n_rows, len(tile_table)))
        tiles = [preds[pred_offsets[t]:pred_offsets[t + 1]].reshape(windows[t][3], windows[t][2]) for t in range(len(tile_table))]
        given = [np.asarray(weights[weight_offsets[k]:weight_offsets[k + 1]]).reshape(tiles[t].shape) for t, k in enumerate(tile_table)]
        classes, counts, stats = assemble(tiles, [tuple(int(v) for v in w) for w in windows], width, height, num_classes, nodataval,
                                          count_dtype=count_dtype, rows=(row0, n_rows), tables=given)
        band = slice(row0, row0 + n_rows)
        return classes[band], counts[:, band] if want_counts else None, stats
