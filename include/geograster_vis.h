/* geograster_vis.h -- companion of geograster.h, which includes it inside its extern "C" block; do not include it on its own:
 * gr_ctx, the GR_* codes and GR_DTYPE_* are geograster.h's.  It holds the two picture calls (csrc/vis.hip; the rule-set V1-V12 is
 * DESIGN.md section 8s): one shaded, anti-aliased picture from the id and depth planes of the raster path, and the reference's
 * three-panel composite of a photo and a label image (utils/visualization.py:113-193).  The binding keeps the signatures in a
 * table of its own (`_VIS_SIGNATURES`) and mirrors the two structures (`ShadeArgs`, `CompositeArgs`); tests/test_vis_host.py
 * compares both with this file.  Added without a GR_VERSION bump.
 *
 * Both calls take their arguments in ONE descriptor in HOST memory, read once before the call returns, and the stream is a field
 * of it.  They are therefore not among the functions of these headers whose last parameter is `void *stream`, and the table of
 * tests/test_stream_contract_gpu.py does not list them.  They are NOT exempt from the stream contract of geograster.h: all work is
 * enqueued on `stream`, nothing waits, nothing is read back; tests/test_stream_contract_vis_gpu.py holds both to it with the same
 * legs as that table's rows, until a change that may edit the table folds them in.  Neither call needs an uploaded mesh or
 * scratch.  All arrays are DEVICE pointers, C-contiguous. */
#ifndef GEOGRASTER_VIS_H
#define GEOGRASTER_VIS_H

/* The picture (width, height >= 1, at most 32768 a side): ids and depth are height * supersample rows of width * supersample
 * samples, as gr_raster_face_ids writes them (-1 and +inf for background), supersample in [1, 4].  A sample whose id is outside
 * [0, F) takes the background colour (bg_r, bg_g, bg_b, each in [0, 255]).  Every other sample takes, per channel, in float32 with
 * every operation rounded on its own (V4-V6),
 *   (face_rgb[id][ch] * (face_light[id] / 255)) * occl,   occl = 1 / (1 + strength * sum), occl = 1 where strength == 0,
 * sum = the terms t > 0 of t = (z - z_q) / z, added in the order (-r, -r), (-r, 0), (-r, r), (0, -r), (0, r), (r, -r), (r, 0), (r, r)
 * of (row, column) offsets, z the sample's depth, z_q the neighbour's, r = radius in [1, 16]; a neighbour outside the planes counts
 * as +inf and adds nothing.  strength is finite and >= 0.  An output byte is floor(sum of the pixel's supersample^2 samples in
 * row-major order / supersample^2 + 0.5), kept inside [0, 255] (V7).  out: height x width x 3 uint8, every byte written.
 * The lights (V3): where verts or faces is not null, the call FIRST writes face_light[f] for every f < F from verts (V x 3 float32)
 * and faces (F x 3 int32), in float64: shade = |n . d| / |n|, n = (b - a) x (c - a), d = (dir_x, dir_y, dir_z) (the caller passes a
 * unit vector; finite), shade = 1 where |n| is 0 or the face names a vertex outside [0, V); face_light = floor((ambient + (1 -
 * ambient) * shade) * 255 + 0.5) kept inside [0, 255], ambient in [0, 1].  width = height = 0 with verts and faces: the lights alone.
 * V, F < 2^31 - 1.
 * GR_EINVAL (the message names gr_shade_view), before any device work: a null descriptor, null arrays, sizes or scalars outside
 * the ranges above. */
typedef struct gr_shade_args {
  const int32_t *ids;
  const float *depth;
  const uint8_t *face_rgb;   /* F x 3 */
  uint8_t *face_light;       /* F: read by the picture; written first where verts and faces are given */
  const float *verts;        /* V x 3, or null */
  const int32_t *faces;      /* F x 3, or null */
  uint8_t *out;
  void *stream;
  int64_t F;
  int64_t V;
  double dir_x;
  double dir_y;
  double dir_z;
  double ambient;
  float strength;
  int32_t width;
  int32_t height;
  int32_t supersample;
  int32_t radius;
  int32_t bg_r;
  int32_t bg_g;
  int32_t bg_b;
} gr_shade_args;

int gr_shade_view(gr_ctx *ctx, const gr_shade_args *args_h);

/* photo: height x width x 3 of photo_dtype; label: height x width (label_channels 1) or height x width x 3 (label_channels 3)
 * of label_dtype; each dtype GR_DTYPE_U8 or GR_DTYPE_F64 (float64 arrays 8-byte aligned).  table: table_rows x 3 float64, 1 to
 * 2^24 rows, read with label_channels 1.  out: height x 3 width x 3 uint8, every byte written: [label colours | photo | overlay].
 * Per pixel in float64, every operation rounded on its own (V8-V12).  A uint8 photo is divided by 255.  Label colours:
 * label_channels 3: the values, a uint8 label divided by 255 (with discrete != 0 that is GR_EINVAL: the reference wraps around
 * there).  A uint8 plane with discrete != 0: row min(label, table_rows - 1) of the table, black for label 0.  Every other plane:
 * x = the value, a uint8 label divided by 255; black where x == 0 or x is not finite (taken before the shift); with discrete == 0
 * x = (x - shift) / scale; t = x * table_rows, t == table_rows -> table_rows - 1; NaN: black; t < 0: row 0; t >= table_rows: the
 * last row; else row trunc(t).  overlay = (1 - weight) * base + weight * label colour, base the photo's channel, or (r + g) + b
 * over 3 where grey_overlay != 0.  An output byte is value * 255 truncated to int32, its low byte (0 where that is no int32).
 * GR_EINVAL (the message names gr_composite_labels), before any device work: a null descriptor, null arrays, sizes, dtypes or
 * channels outside the above, more than 2^31 - 1 (row, 1024 pixel) strips. */
typedef struct gr_composite_args {
  const void *photo;
  const void *label;
  const double *table;
  uint8_t *out;
  void *stream;
  double shift;
  double scale;
  double weight;
  int32_t width;
  int32_t height;
  int32_t table_rows;
  int32_t photo_dtype;
  int32_t label_dtype;
  int32_t label_channels;
  int32_t discrete;
  int32_t grey_overlay;
} gr_composite_args;

int gr_composite_labels(gr_ctx *ctx, const gr_composite_args *args_h);

#endif /* GEOGRASTER_VIS_H */
