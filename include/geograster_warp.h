/* geograster_warp.h -- companion of geograster.h, which includes it inside its extern "C" block; do not include it on its own:
 * gr_ctx, gr_crs, the GR_* codes, GR_DTYPE_* and the GR_WARP_* enumerators are geograster.h's.  It holds the raster -> raster call
 * (csrc/raster_warp.hip; the rule-set W1-W9 is DESIGN.md section 8t): a window of a destination grid, every cell centre taken to a
 * source raster -- through the closed-form WGS84 conversion of gr_reproject_points where the two grids differ in CRS -- and
 * resampled there, nearest or bilinear.  The binding keeps the signature in a table of its own (`_WARP_SIGNATURES`) and mirrors the
 * structure (`WarpRasterArgs`); tests/test_raster_warp_host.py compares both with this file.  Added without a GR_VERSION bump.
 *
 * The call takes its arguments in ONE descriptor in HOST memory, read once before the call returns, and the stream is a field of
 * it.  It is therefore not among the functions of these headers whose last parameter is `void *stream`, and the table of
 * tests/test_stream_contract_gpu.py does not list it.  It is NOT exempt from the stream contract of geograster.h: all work is
 * enqueued on `stream`, nothing waits, nothing is read back; tests/test_stream_contract_warp_gpu.py holds it to that with the same
 * legs as that table's rows, until a change that may edit the table folds it in.  The call needs no uploaded mesh and no scratch. */
#ifndef GEOGRASTER_WARP_H
#define GEOGRASTER_WARP_H

/* data: the source, B x H x W of src_dtype (GR_DTYPE_U8, GR_DTYPE_F32 or GR_DTYPE_F64; uint8 is read as bytes, never widened in
 * memory), a DEVICE pointer, C-contiguous; 1 <= B <= GR_WARP_MAX_BANDS, 1 <= H, W < 2^23.  src_inverse6_h (a HOST pointer): the
 * inverse affine transform of the source, (ia, ib, ic, id, ie, if) as gr_sample_raster takes it.  dst_transform6_h (a HOST pointer):
 * the transform (a, b, c0, d, e, f0) of the destination's parent grid; (col_off, row_off, width, height) is the window of it that
 * is written (B1's limits: not empty, offsets inside (-2^23, 2^23), far edges at or below 2^23; it may leave the grid on any side).
 * out: B x height x width of dst_dtype, a DEVICE pointer, every byte written; it must not overlap data.  src_crs_h, dst_crs_h (HOST
 * pointers, read only where same_crs == 0): the two systems, GR_CRS_GEOGRAPHIC (lon, lat in degrees: longitude FIRST) or GR_CRS_TM.
 * Per window cell (r, c), in float64 with every operation rounded on its own (W2-W4):
 *   col = col_off + c + 0.5, row = row_off + r + 0.5;  x = (a col + b row) + c0, y = (d col + e row) + f0;
 *   same_crs != 0: (xs, ys) = (x, y); else (x, y, 0) converted dst_crs -> src_crs as gr_reproject_points converts a row -- a centre
 *   that cannot be converted is dst_nodata in every band and counted once under its cause;
 *   u = (ia xs + ib ys) + ic, v = (id xs + ie ys) + if.
 * GR_WARP_NEAREST (W5): the cell (floor(v), floor(u)); outside [0, H) x [0, W): dst_nodata, counted GR_WARP_STAT_OUTSIDE; a sample
 * equal to src_nodata (where has_src_nodata != 0) or a NaN becomes dst_nodata, the cell is counted GR_WARP_STAT_NODATA.
 * GR_WARP_BILINEAR (W6): u' = u - 0.5, v' = v - 0.5, c0 = floor(u'), fx = u' - c0, r0 = floor(v'), fy = v' - r0; the taps (r0, c0),
 * (r0, c0 + 1), (r0 + 1, c0), (r0 + 1, c0 + 1) with the weights (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy; a tap takes part iff
 * it lies in the raster and, per band, is neither src_nodata nor NaN; num = sum w v and den = sum w over the participating taps in
 * that order; den == 0: dst_nodata (GR_WARP_STAT_DEN_ZERO); all four take part: num; else num / den.  No tap in the raster:
 * GR_WARP_STAT_OUTSIDE.  A cell with a tap in the raster that, in some band, is src_nodata or NaN counts GR_WARP_STAT_NODATA.
 * Output (W7): GR_DTYPE_F64 as it is, GR_DTYPE_F32 one rounding, GR_DTYPE_U8 floor(value + 0.5) kept inside [0, 255] (NaN: 0);
 * dst_nodata is converted the same way.
 * stats: GR_WARP_STAT_WORDS uint64 on the device, zeroed and written by the call.
 * GR_EINVAL (the message names gr_warp_raster), before any device work: a null descriptor, null arrays; B, H, W out of range; an
 * unknown dtype or resampling; a window outside B1 or of more than 2^31 - 1 (row, 256 column) strips; a transform that is not
 * finite; with same_crs == 0 a null, unknown or ECEF side, k0 not > 0 or parameters that are not finite; a float64 array that is
 * not 8-byte aligned (float32: 4-byte); out overlapping data. */
typedef struct gr_warp_raster_args {
  const void *data;
  void *out;
  uint64_t *stats;
  void *stream;
  const double *src_inverse6_h;
  const double *dst_transform6_h;
  const gr_crs *src_crs_h;
  const gr_crs *dst_crs_h;
  double src_nodata;
  double dst_nodata;
  int32_t B;
  int32_t H;
  int32_t W;
  int32_t src_dtype;
  int32_t dst_dtype;
  int32_t has_src_nodata;
  int32_t col_off;
  int32_t row_off;
  int32_t width;
  int32_t height;
  int32_t resampling;
  int32_t same_crs;
} gr_warp_raster_args;

int gr_warp_raster(gr_ctx *ctx, const gr_warp_raster_args *args_h);

#endif /* GEOGRASTER_WARP_H */
