/* geograster_ortho.h -- companion of geograster.h, which includes it inside its extern "C" block; do not include it on its own:
 * gr_ctx, the GR_* codes and the GR_COUNT_*, GR_ORTHO_* and GR_ZONAL_* enumerators are geograster.h's.  It holds the two calls of the
 * orthomosaic baseline (csrc/ortho.hip; the rule-sets O1-O8 and Z1-Z7 are DESIGN.md section 8m).  The binding keeps their signatures
 * in a table of its own (`_ORTHO_SIGNATURES`), which tests/test_ortho_baseline_host.py compares with this file.  Both calls only
 * enqueue work on `stream`, need no uploaded mesh and no context scratch, and were added without a GR_VERSION bump. */
#ifndef GEOGRASTER_ORTHO_H
#define GEOGRASTER_ORTHO_H

/* Tile assembly -- replaces the accumulation and the argmax of assemble_tiled_predictions (predictors/ortho_segmentor.py:346-431):
 * the rows [row0, row0 + n_rows) of the class raster of an extent `width` pixels wide, from the tile predictions that meet them.
 * All arrays are DEVICE pointers.
 * preds: the uint8 predictions of the T tiles, concatenated, n_pred_bytes in all; tile t is rows x columns from pred_offsets[t]
 * (T + 1 int64).  A value >= C takes no part (the host maps everything that is not a class to 255, O4).
 * windows: T x 4 int32 col_off, row_off, width, height in extent coordinates (O1).  tile_table[t]: the weight table of tile t;
 * table k is weight_offsets[k + 1] - weight_offsets[k] = width x height values of the count type from weight_offsets[k]
 * (n_tables + 1 int64) in `weights` (n_weights values): uint8 (GR_COUNT_U8), uint16 (GR_COUNT_U16) or float64 (GR_COUNT_F64), O2.
 * Bin table: bins_x x bins_y square bins of bin_side pixels from the extent's corner, bin (bx, by) at by bins_x + bx; bin_ptr
 * (bins_x bins_y + 1 int64) delimits in bin_tiles (n_bin_entries int32) the tiles whose window meets the bin, in strictly ASCENDING
 * tile index (the order of the float64 sums, O3).  The bins cover the width and the rows asked for.
 * classes: n_rows x width uint8, every byte written once: nodataval (0..255) where all C counts are 0 -- counts that wrapped to 0
 * included --, else the lowest class of the largest count (O5).  counts: C x n_rows x width of the count type, or NULL (not
 * stored).  A count is the sum of the weights of the covering tiles that predict the class, taken in the count type: modulo 2^8 or
 * 2^16, or float64 adds in ascending tile index, each rounded on its own.  No count is formed by atomics (O6).
 * stats: GR_ORTHO_STAT_WORDS uint64, written by the call.
 * Nothing is read through an index that was not checked: a bin entry outside [0, T), a table index outside [0, n_tables), a
 * window with a non-positive side, offsets that leave the arrays -- such a tile takes no part (O8; the binding refuses them with
 * ValueError first).  GR_EINVAL (the message names the call), before any device work: null arrays, negative sizes, T >= 2^31, C
 * outside [1, GR_ORTHO_MAX_CLASSES], nodataval outside [0, 255], an unknown count type, a bin table that does not cover the rows,
 * a band too tall for one launch (more than 65535 workgroup rows of 4 pixel rows). */
int gr_assemble_tiles(gr_ctx *ctx, const uint8_t *preds, int64_t n_pred_bytes, const int64_t *pred_offsets, const int32_t *windows,
                      const int32_t *tile_table, int64_t T, const void *weights, int64_t n_weights, const int64_t *weight_offsets,
                      int32_t n_tables, int32_t count_dtype, const int64_t *bin_ptr, const int32_t *bin_tiles, int64_t n_bin_entries,
                      int32_t bin_side, int32_t bins_x, int32_t bins_y, int32_t width, int64_t row0, int32_t n_rows, int32_t C,
                      int32_t nodataval, uint8_t *classes, void *counts, uint64_t *stats, void *stream);

/* Zonal class counts -- replaces rasterstats.zonal_stats(categorical=True) of get_overlap_raster (utils/geospatial.py:150-211) and
 * compute_confusion_matrix_from_geospatial (utils/prediction_metrics.py:194): counts[p][v] = the cells of value v whose centre lies
 * in polygon row p.  All arrays are DEVICE pointers.
 * raster: H x W uint8, 1 <= H, W < 2^23; nodata: the value that is not counted, or -1 for none (Z5).
 * Ring table as gr_polygon_class_weights takes it -- ring_vertices (n_ring_vertices x 2 int64), ring_offsets (R + 1 int64),
 * ring_polygon (R int32, non-decreasing) -- in PIXEL coordinates times 65536 (Z1), |value| < 2^40.  The centre of cell (row, col)
 * is (65536 col + 32768, 65536 row + 32768) (Z2) and belongs to row p iff an odd number of the edges of ALL rings of p count
 * (Z3): an edge is a candidate when exactly one of its ends has y > the centre's, and counts when the centre is STRICTLY left of
 * it taken upwards -- a centre on an edge shared by two rows belongs to exactly one of them.  Rings of fewer than 3 vertices are
 * ignored and counted.
 * items: n_items x GR_ZONAL_ITEM_INTS int32 work items -- polygon row, col0, row0, width (1..GR_ZONAL_BLOCK_W), height
 * (1..GR_ZONAL_BLOCK_H) of a block of cells inside the raster, the first ring of the row, one past its last ring (Z6).  The
 * blocks of a row must not overlap; the result does not depend on their shape.  A malformed item is skipped.
 * counts: P x C uint64, zeroed by the call; a value >= C adds nothing (Z4).  stats: GR_ZONAL_STAT_WORDS uint64, written by the
 * call (Z7).  GR_EINVAL (the message names the call), before any device work: null arrays, negative sizes, R, P or n_items >= 2^31,
 * H or W outside [1, 2^23), C outside [1, GR_ZONAL_MAX_CLASSES]. */
int gr_zonal_class_counts(gr_ctx *ctx, const uint8_t *raster, int32_t H, int32_t W, int32_t nodata, const int64_t *ring_vertices,
                          int64_t n_ring_vertices, const int64_t *ring_offsets, const int32_t *ring_polygon, int64_t R, int64_t P,
                          const int32_t *items, int64_t n_items, int32_t C, uint64_t *counts, uint64_t *stats, void *stream);

#endif /* GEOGRASTER_ORTHO_H */
