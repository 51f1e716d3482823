/* geograster_nadir.h -- companion of geograster.h, which includes it inside its extern "C" block; do not include it on its own:
 * gr_ctx, the GR_* codes and the GR_NADIR_STAT_* enumerators are geograster.h's.  It holds the top-down (nadir, orthographic) raster
 * of a mesh on a georeferenced grid (csrc/nadir.hip; the rule-set N1-N9 is DESIGN.md section 8r): per cell the face whose surface
 * is highest at the cell's centre and that height.  The reference has no counterpart.  The binding keeps the signature in a table
 * of its own (`_NADIR_SIGNATURES`), which tests/test_top_down_raster_host.py compares with this file.  The call needs no uploaded
 * mesh, uses the context's stage scratch (one call of a context at a time), reads two words back between its passes and was added
 * without a GR_VERSION bump.  All arrays are DEVICE pointers. */
#ifndef GEOGRASTER_NADIR_H
#define GEOGRASTER_NADIR_H

/* One window of a parent raster grid, as gr_burn_polygons takes it (B1): the cells [col_off, col_off + width) x [row_off, row_off +
 * height), width, height >= 1, |col_off|, |row_off| < 2^23, col_off + width <= 2^23, row_off + height <= 2^23.  The window may
 * leave the parent raster on any side.
 * verts_q: V x 2 int64, the vertices' x, y in cell coordinates of the PARENT grid times 65536 (Z1), |value| < 2^40 -- the CALLER
 * guarantees it; a table that breaks it reads and writes nothing outside the arrays, and its results mean nothing.  z: V float64.
 * faces: F x 3 int32.  V, F < 2^31 - 1.
 * A face takes part (N3) when its three indices lie in [0, V), its three z are finite and the exact doubled area of its snapped
 * triangle is not 0; the other faces are counted, each under its first cause in that order, and never dereferenced past the
 * indices.  The centre (65536 col + 32768, 65536 row + 32768) of a cell belongs to a face under Z3 applied to the triangle as a
 * ring of three vertices (N4): half-open in y, strictly left of the upward edge, by the sign of an exact determinant.  The height
 * of the face at the centre is N5's float64 expression, every operation rounded on its own; a (face, cell) whose denominator is 0
 * or whose height is not finite is skipped and counted.  The greatest height wins, compared through the order-preserving 64-bit
 * key of its bit pattern (-0.0 below +0.0); equal keys go to the lowest face index (N6).  The planes do not depend on small_cells,
 * item_rows, the launch or the order of arrival.
 * small_cells: a face whose box of centres, cut to the window, holds at most this many is walked by one lane; 0: the default, 256;
 * at most 65536.  item_rows: the faces above it are cut into items of 64 columns x item_rows rows, a wave each; 0: the default, 16;
 * at most 1024 (N8).
 * face_out: height x width int32, every word written: the winning face, -1 where no face holds the centre.  z_out: height x width
 * float64, every word written: the winning height, NaN (0x7FF8000000000000) where face_out is -1; 8-byte aligned -- the call keeps
 * the keys in it between its passes.  stats: GR_NADIR_STAT_WORDS uint64, written by the call (N9).
 * Synchronises `stream` once, between its passes, to read two words back, and returns with its last kernels enqueued on it.
 * GR_EINVAL (the message names gr_nadir_raster), before any device work: null arrays, negative sizes, V or F >= 2^31 - 1, a window
 * outside the bounds above, small_cells or item_rows outside their ranges. */
int gr_nadir_raster(gr_ctx *ctx, const int64_t *verts_q, const double *z, int64_t V, const int32_t *faces, int64_t F, int32_t col_off,
                    int32_t row_off, int32_t width, int32_t height, int32_t small_cells, int32_t item_rows, int32_t *face_out,
                    double *z_out, uint64_t *stats, void *stream);

#endif /* GEOGRASTER_NADIR_H */
