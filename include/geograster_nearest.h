/* geograster_nearest.h -- companion of geograster.h, which includes it inside its extern "C" block; do not include it on its own:
 * gr_ctx, the GR_* codes and the GR_NN_STAT_* enumerators are geograster.h's.  It holds the nearest-point call
 * (csrc/nearest.hip; the rule-set K1-K9 is DESIGN.md section 8v): for every query point the row of the nearest reference point,
 * exact -- the brute-force argmin of one float64 expression, bit for bit -- found over a uniform grid of sorted cell keys.  The
 * binding keeps the signature in a table of its own (`_NEAREST_SIGNATURES`) and mirrors the structure (`NearestArgs`);
 * tests/test_nearest_points_host.py compares both with this file.  Added without a GR_VERSION bump.
 *
 * The call takes its arguments in ONE descriptor in HOST memory, read once before the call returns, and the stream is a field of
 * it.  It is therefore not among the functions of these headers whose last parameter is `void *stream`, and the table of
 * tests/test_stream_contract_gpu.py does not list it.  It is NOT exempt from the stream contract of geograster.h: all work is
 * enqueued on `stream` and the call never touches another stream.  With R > 0 and Q > 0 it synchronises `stream` once to read the
 * bounds of the reference points back and once per level to read one word back (the queries the level left unsettled); with
 * R == 0 or Q == 0 it does not wait at all.  tests/test_stream_contract_nearest_gpu.py holds it to that.  The call needs no
 * uploaded mesh; its scratch is the context's stage arena (44 R + 8 Q bytes and the sort's temporaries). */
#ifndef GEOGRASTER_NEAREST_H
#define GEOGRASTER_NEAREST_H

/* All arrays are DEVICE pointers, C-contiguous.  Limits: R and Q < 2^31 - 1.
 * K1  ref: R x 3 float64, query: Q x 3 float64.  A ref row with a NaN or infinite coordinate takes no part and is counted
 *     (GR_NN_STAT_REF_NONFINITE).  A query row with one gets index -1 and dist2 NaN and is counted (GR_NN_STAT_QUERY_NONFINITE).
 * K2  d2(q, r) = ((qx - rx) * (qx - rx) + (qy - ry) * (qy - ry)) + (qz - rz) * (qz - rz) in float64, every operation rounded on
 *     its own.
 * K3  The answer for q is the participating ref row with the smallest d2, the lowest row among equal d2: the brute-force argmin
 *     of K2 over all participating rows, bit for bit in dist2_out.  It depends on no implementation parameter (cell, max_rings),
 *     no launch order and no arrival order.
 * K4  md2 = max_distance * max_distance.  The answer is kept iff d2 <= md2 (a ref exactly at the distance is kept); otherwise
 *     index -1 and dist2 NaN.  max_distance = +inf: every answer is kept.
 * K5  R == 0, or no participating ref row: every query gets -1 / NaN.  Q == 0: only the statistics are written.
 * K6  index_out: Q int32; dist2_out: Q float64 or null; stats: GR_NN_STAT_WORDS uint64.  Every word of the three is written.
 * K7  The statistics are those of geograster.h's GR_NN_STAT_*.  REF_NONFINITE, QUERY_NONFINITE and NO_ANSWER depend on the
 *     inputs alone; LEVELS, CARRIED, CELLS_PROBED, CANDIDATES, CELL_BITS and RING_CAP describe the search and depend on cell and
 *     max_rings too.  NO_ANSWER counts every query whose index is -1, the non-finite ones included.
 * K8  cell: the side of a grid cell in the units of the coordinates; 0: the call chooses (1.5 sqrt(e1 e2 / R'), e1 >= e2 the two
 *     largest extents of the participating refs and R' their number; never below e1 / 2^20).  A given cell is raised to e1 / 2^21:
 *     an axis has at most 2^21 cells.  max_rings >= 1: a query looks at its own cell and max_rings rings of cells around it; one
 *     that is not settled then is carried to the next level, whose cells are four times as wide.  The last level has one cell.
 * K9  The stream rule above.
 * GR_EINVAL (the message names gr_nearest_points), before any device work: a null descriptor, null arrays (ref with R > 0, query or
 * index_out with Q > 0, stats always); R or Q negative or >= 2^31 - 1; cell negative, NaN or infinite; max_distance NaN or
 * negative; max_rings < 1; index_out, dist2_out or stats overlapping an input or each other. */
typedef struct gr_nearest_args {
  const double *ref;
  const double *query;
  int32_t *index_out;
  double *dist2_out;
  uint64_t *stats;
  void *stream;
  int64_t R;
  int64_t Q;
  double cell;
  double max_distance;
  int32_t max_rings;
  int32_t reserved;
} gr_nearest_args;

int gr_nearest_points(gr_ctx *ctx, const gr_nearest_args *args_h);

#endif /* GEOGRASTER_NEAREST_H */
