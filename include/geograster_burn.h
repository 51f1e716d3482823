/* geograster_burn.h -- companion of geograster.h, which includes it inside its extern "C" block; do not include it on its own:
 * gr_ctx, the GR_* codes and the GR_BURN_* and GR_ZONAL_* enumerators are geograster.h's.  It holds the polygon burn of the
 * orthomosaic baseline (csrc/ortho.hip; the rule-set B1-B7 is DESIGN.md section 8m), which stands where the reference's write_chips
 * calls rasterio.features.rasterize(shapes, out_shape, transform=window_transform, fill=...) per chip window
 * (predictors/ortho_segmentor.py:217-226).  The binding keeps the signature in a table of its own (`_BURN_SIGNATURES`), which
 * tests/test_polygon_burn_host.py compares with this file.  The call only enqueues work on `stream`, needs no uploaded mesh and no
 * context scratch, and was added without a GR_VERSION bump.  All arrays are DEVICE pointers. */
#ifndef GEOGRASTER_BURN_H
#define GEOGRASTER_BURN_H

/* One window of a parent raster grid: the cells [col_off, col_off + width) x [row_off, row_off + height), width, height >= 1,
 * |col_off|, |row_off| < 2^23, col_off + width <= 2^23, row_off + height <= 2^23.  The window may leave the parent raster on any
 * side: the grid has no extent here (B1).
 * Ring table as gr_zonal_class_counts takes it -- ring_vertices (n_ring_vertices x 2 int64), ring_offsets (R + 1 int64),
 * ring_polygon (R int32, non-decreasing) -- in cell coordinates of the PARENT grid times 65536 (Z1), |value| < 2^40.  The centre of
 * cell (row, col) belongs to row p under Z2 and Z3 exactly as there (B2): even-odd over all rings of p, half-open in y, strictly
 * left of the upward edge; rings of fewer than 3 vertices are ignored and counted.
 * items: n_items x GR_ZONAL_ITEM_INTS int32 work items -- polygon row, col0, row0, width (1..GR_ZONAL_BLOCK_W), height
 * (1..GR_ZONAL_BLOCK_H) of a block of cells in PARENT coordinates that lies inside the window, the first ring of the row, one past
 * its last ring (B5).  The blocks of a row must not overlap; the result does not depend on their shape.  An item that is malformed
 * or leaves the window is skipped whole (B7).
 * rows: height x width int32, every word written by the call: the HIGHEST row index among the rows that hold the cell's centre,
 * -1 where none does (B3: later rows overwrite earlier ones, whatever the order of arrival -- an integer maximum).
 * out: height x width uint8 or NULL; every byte written: values[rows], `fill` (0..255) where rows < 0 (B4).  values: P uint8,
 * needed with `out` when P > 0, not read without it.
 * stats: GR_BURN_STAT_WORDS uint64, written by the call (B6); GR_BURN_STAT_BURNED is counted by the pass that writes `out` and is 0
 * without it.  GR_EINVAL (the message names the call), before any device work: null arrays, negative sizes, R, P or n_items >=
 * 2^31, a window outside the bounds above, fill outside [0, 255], null values with an output plane. */
int gr_burn_polygons(gr_ctx *ctx, const int64_t *ring_vertices, int64_t n_ring_vertices, const int64_t *ring_offsets,
                     const int32_t *ring_polygon, int64_t R, int64_t P, const uint8_t *values, const int32_t *items, int64_t n_items,
                     int32_t col_off, int32_t row_off, int32_t width, int32_t height, int32_t fill, int32_t *rows, uint8_t *out,
                     uint64_t *stats, void *stream);

#endif /* GEOGRASTER_BURN_H */
