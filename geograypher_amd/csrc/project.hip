// geograypher_amd/csrc/project.hip -- everything behind the rasterizer: last-writer-wins winners from id images, per-face
// votes / nansums, per-view textures, texture gathers, sparse (face, class) pairs (from label images, rectangles, polygon rings), finalize, argmax -- kernels and entry points.
#include "cub_steps.hpp"
#include "gr_internal.hpp"
#include "dev_common.hpp"

using namespace grimpl;

namespace {

// last-writer-wins candidate of the unfused pass (K5): issue the global atomicMax only when neither the right nor the
// lower neighbour shows the same face.  key = pixel + 1 (the label is looked up by the vote kernel).
__device__ __forceinline__ void winner_pixel(uint32_t *__restrict__ winner, int f, int fr, int fb, int64_t p, int64_t F,
                                              int compat) {
  if (compat) {  // meshes.py:1998-2001: index -1 aliases the last face
    const int last = (int)F - 1;
    if (f == -1) f = last;
    if (fr == -1) fr = last;
    if (fb == -1) fb = last;
  }
  if (f < 0 || f >= F) return;
  if (fr == f || fb == f) return;  // a later pixel of the same face exists
  atomicMax(&winner[f], (uint32_t)(p + 1));
}

// ------------------------------------------------------------------------------------------------------------------
// K5  last-writer-wins winners from id images already in memory (the unfused path).  Four pixels per thread.  A pixel
//     can only be its face's LAST pixel in row-major order if neither its right nor its lower neighbour shows the same
//     face, so only those candidates issue the global atomicMax (~1-3 per visible face instead of ~80).  key = pixel + 1.
// ------------------------------------------------------------------------------------------------------------------
// grid (ceil(w/1024), ceil(h/WIN_ROWS), views): a thread owns 4 consecutive columns and walks WIN_ROWS rows downwards;
// the row below is loaded once and becomes the current row of the next step (16-byte id loads).
#define WIN_ROWS 16
__global__ __launch_bounds__(256) void k_winner(const int32_t *__restrict__ ids, uint32_t *__restrict__ winner, int64_t F,
                                                int h, int w, int compat) {
  const int slot = blockIdx.z;
  const int y0 = blockIdx.y * WIN_ROWS;
  const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (x0 >= w) return;
  const int64_t P = (int64_t)h * w;
  const int32_t *img = ids + slot * P;
  uint32_t *win = winner + slot * F;
  const bool vec = ((w & 3) == 0) && ((reinterpret_cast<uintptr_t>(img) & 15) == 0);
  auto load_row = [&](int y, int (&f)[5]) {
    const int32_t *row = img + (int64_t)y * w;
    if (vec) {
      const int4 c = *reinterpret_cast<const int4 *>(row + x0);
      f[0] = c.x; f[1] = c.y; f[2] = c.z; f[3] = c.w;
      f[4] = (x0 + 4 < w) ? row[x0 + 4] : -2;
    } else {
#pragma unroll
      for (int k = 0; k < 5; ++k) f[k] = (x0 + k < w) ? row[x0 + k] : -2;
    }
  };
  int cur[5], nxt[5];
  load_row(y0, cur);
  const int y1 = min(y0 + WIN_ROWS, h);
  for (int y = y0; y < y1; ++y) {
    const bool has_below = (y + 1 < h);
    if (has_below) load_row(y + 1, nxt);
    else { nxt[0] = nxt[1] = nxt[2] = nxt[3] = nxt[4] = -2; }
    const int64_t p0 = (int64_t)y * w + x0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x0 + k < w) winner_pixel(win, cur[k], cur[k + 1], nxt[k], p0 + k, F, compat);
#pragma unroll
    for (int k = 0; k < 5; ++k) cur[k] = nxt[k];
  }
}

// K6  per-face vote: one thread per face walks the views of the launch group IN ORDER (deterministic, no atomics needed:
//     a face belongs to exactly one thread).  The label of the winning pixel is looked up here (one byte per visible
//     face and view; neighbouring faces win neighbouring pixels): votes[f][label] += 1, counts[f] += 1; a label >= C
//     (255 = ignore) is an all-zero one-hot row that still counts (predictors/segmentor.py:37-69).  Winners are
//     cleared for reuse (only the faces a view shows were written: a tenth of the array).
//     Fused aggregation: a wave reads the winners of its 64 faces only for the views in which the tile kernel marked the group
//     (round 5: a bit per 256-face chunk from the cull pass's block lists -- half of the winners it made the pass read were empty).
__global__ __launch_bounds__(256) void k_vote_labels(uint32_t *__restrict__ winner, const uint8_t *__restrict__ labels,
                                                     int n_views, int64_t F, int64_t P, int C,
                                                     uint32_t *__restrict__ votes, uint32_t *__restrict__ counts,
                                                     const unsigned long long *__restrict__ stats, int group,
                                                     const uint32_t *__restrict__ touched, int tw, uint32_t *__restrict__ visits) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  // which views of the group hold a winner for this WAVE's 64 faces: the byte the tile kernel's epilogue set for the group
  // beside its winner atomic (exact: a group no pixel of the view voted into is not read at all; background pixels that alias
  // the last face mark its group like any other winner); without the map (ids given by the caller) every view can.  Lane v
  // looks at view v.
  unsigned long long dirty = ~0ull;
  if (touched) {
    const int v = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    bool d = false;
    if (v < n_views && g * 64 < F) d = reinterpret_cast<const uint8_t *>(touched + (int64_t)v * tw)[g] != 0;
    dirty = __ballot(d);
    // (view, group) pairs visited, for gr_raster_stats.chunk_visits: a slot per group, no contention
    if (visits && v == 0 && dirty) visits[g] += (uint32_t)__popcll(dirty);
  }
  if (f >= F) return;
  // a launch group whose binning overflowed (and every group after it) must not vote: its winners are incomplete.  The
  // caller learns how many views were folded in (gr_raster_status: views_done) and repeats the call for the rest.
  const bool skip = stats != nullptr && stats[GR_ST_FIRST_GROUP] <= (unsigned long long)group;
  uint32_t c = 0;
  // up to sixteen classes: the face's votes of the whole launch group are collected in TWO registers, a byte per class (a group has
  // at most 64 views), and folded into votes[] once at the end -- loads first, then stores.  (`votes[f][label] += 1` view by view
  // is a chain of dependent read-modify-writes on one array: the compiler must finish each before the next may start, eight
  // memory round trips per batch of eight views, and the kernel is nothing but latency: round 5, 1.9 us per C2 view.)
  const bool packed = C <= 16;
  unsigned long long acc0 = 0ull, acc1 = 0ull;
  // eight views' winners are requested together (the kernel is a stream over winner[views][F]: memory-level
  // parallelism, not arithmetic, sets its speed), then their labels, then the votes in view order
  for (int v0 = 0; v0 < n_views; v0 += 8) {
    const uint32_t d8 = (uint32_t)(dirty >> v0) & 0xFFu;
    if (d8 == 0u) continue;
    uint32_t key[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) key[k] = (v0 + k < n_views && ((d8 >> k) & 1u)) ? winner[(int64_t)(v0 + k) * F + f] : 0u;
    uint32_t lab[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) lab[k] = (key[k] && !skip) ? (uint32_t)labels[(int64_t)(v0 + k) * P + (key[k] - 1)] : 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (key[k] == 0) continue;
      winner[(int64_t)(v0 + k) * F + f] = 0;
      if (skip) continue;
      if ((int)lab[k] < C) {
        if (!packed) votes[f * C + lab[k]] += 1u;
        else if (lab[k] < 8u) acc0 += 1ull << (8u * lab[k]);
        else acc1 += 1ull << (8u * (lab[k] - 8u));
      }
      ++c;
    }
  }
  if (acc0 | acc1) {
    uint32_t cur[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) cur[k] = k < C ? votes[f * C + k] : 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t add = (uint32_t)((k < 8 ? acc0 : acc1) >> (8 * (k & 7))) & 0xFFu;
      if (k < C && add) votes[f * C + k] = cur[k] + add;
    }
  }
  if (c) counts[f] += c;
}

__global__ __launch_bounds__(256) void k_vote_values(uint32_t *__restrict__ winner, const double *__restrict__ img,
                                                     int n_views, int64_t F, int64_t P, int C,
                                                     double *__restrict__ sums, uint32_t *__restrict__ counts) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  // meshes.py:2060-2062 to the letter: summed = np.nansum([summed, projection], axis=0) drops a NaN of the RUNNING sum as
  // well as one of the projection -- a sum that went NaN (+inf of one view met -inf of another) starts again from zero at the
  // next view, whether that view shows the face or not.  (Found by tools/fuzz_stages.py; rounds 1-3 kept the NaN.)
  double *const acc = sums + f * C;
  for (int ch = 0; ch < C; ++ch)
    if (isnan(acc[ch])) acc[ch] = 0.0;  // left by an earlier launch: this launch holds a next view
  uint32_t c = 0;
  int last_seen = -1;
  for (int v0 = 0; v0 < n_views; v0 += 8) {  // eight views' winners are requested together, then consumed in view order
    uint32_t keyv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) keyv[k] = (v0 + k < n_views) ? winner[(int64_t)(v0 + k) * F + f] : 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t key = keyv[k];
      if (key == 0) continue;
      const int v = v0 + k;
      winner[(int64_t)v * F + f] = 0;
      const double *row = img + ((int64_t)v * P + (key - 1)) * C;
      bool any_finite = false;
      for (int ch = 0; ch < C; ++ch) {
        const double x = row[ch];
        if (isfinite(x)) any_finite = true;
        double a = acc[ch];
        if (isnan(a)) a = 0.0;          // the running sum's NaN counts as 0 ...
        if (!isnan(x)) a += x;          // ... like the projection's
        acc[ch] = a;
      }
      if (any_finite) ++c;
      last_seen = v;
    }
  }
  if (last_seen >= 0 && last_seen < n_views - 1)  // a NaN made at the face's last view here is dropped by the view behind it
    for (int ch = 0; ch < C; ++ch)
      if (isnan(acc[ch])) acc[ch] = 0.0;
  if (c) counts[f] += c;
}

__global__ __launch_bounds__(256) void k_project_view(uint32_t *__restrict__ winner, const double *__restrict__ img,
                                                      int64_t F, int C, double *__restrict__ tex) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= F * C) return;
  const int64_t f = i / C;
  const int ch = (int)(i - f * C);
  const uint32_t key = winner[f];
  tex[i] = key ? img[(int64_t)(key - 1) * C + ch] : __longlong_as_double(0x7FF8000000000000ll);
}

__global__ __launch_bounds__(256) void k_clear_u32(uint32_t *p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0;
}

// K7  render_flat gather: out[p][c] = tex[ids[p]][c] or NaN
__global__ __launch_bounds__(256) void k_gather_texture(const int32_t *__restrict__ ids, int64_t n_pix,
                                                        const double *__restrict__ tex, int64_t F, int C,
                                                        double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pix * C) return;
  const int64_t p = i / C;
  const int ch = (int)(i - p * C);
  const int f = ids[p];
  out[i] = (f >= 0 && f < F) ? tex[(int64_t)f * C + ch] : __longlong_as_double(0x7FF8000000000000ll);
}

// K9  save_renders epilogue (row f2): gather the face texture and cast it the way meshes.py:2325-2337 does --
//     values < 0, > 255 or non-finite (and pixels without a face) become `null_value`, the rest is truncated to uint8.
__global__ __launch_bounds__(256) void k_gather_texture_u8(const int32_t *__restrict__ ids, int64_t n_pix,
                                                           const double *__restrict__ tex, int64_t F, int C,
                                                           uint8_t null_value, uint8_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pix * C) return;
  const int64_t p = i / C;
  const int ch = (int)(i - p * C);
  const int f = ids[p];
  uint8_t v = null_value;
  if (f >= 0 && f < F) {
    const double x = tex[(int64_t)f * C + ch];
    if (x >= 0.0 && x <= 255.0) v = (uint8_t)x;  // false for NaN; truncation like numpy's astype(uint8)
  }
  out[i] = v;
}

// A face's winner of view v, taken: the key (pixel + 1; 0 = the view does not show the face) with its slot cleared for reuse
// (only the faces a view shows were written).  (The vote kernels load eight views' winners at once instead: measured.)
__device__ __forceinline__ uint32_t take_winner(uint32_t *__restrict__ winner, int v, int64_t F, int64_t f) {
  const uint32_t key = winner[v * F + f];
  if (key != 0) winner[v * F + f] = 0;
  return key;
}

// ... and the pixel (row pi, column pj) a non-zero key stands for in an image of width w
__device__ __forceinline__ void winner_row_col(uint32_t key, int w, int &pi, int &pj) {
  pi = (int)((key - 1) / (uint32_t)w);
  pj = (int)((key - 1) % (uint32_t)w);
}

// The tail of the emit kernels (K10, K10r, K10p).  EVERY lane of the wave must reach it (it ballots), with or without a pair.
// A lane that `has` an observation of class `cls` flags a class outside [0, n_classes) in `bad`; the others' pair keys
// f * n_classes + cls are appended behind *key_count with one atomic per wave; a key beyond key_cap is counted and dropped.
// (The ballot and the test of the same value stay together here, and this stays inlined: dev_common.hpp says why.)
__device__ __forceinline__ void emit_class(bool has, long long cls, int64_t f, long long n_classes,
                                           unsigned long long *__restrict__ keys, long long key_cap,
                                           unsigned long long *__restrict__ key_count, int *__restrict__ bad) {
  const bool emit = has && cls >= 0 && cls < n_classes;
  if (has && !emit) atomicOr(bad, 1);
  const unsigned long long key = (unsigned long long)f * (unsigned long long)n_classes + (unsigned long long)cls;
  const unsigned long long takers = __ballot(emit);
  if (takers) {
    const int lane = threadIdx.x & 63;
    const unsigned long long base = wave_append(takers, key_count, lane);
    if (emit) {
      const unsigned long long idx = base + wave_rank(takers, lane);
      if ((long long)idx < key_cap) keys[idx] = key;
    }
  }
}

// K10r and K10p keep a view's table rows {imin, jmin, imax, jmax, class} in LDS, PAIR_CHUNK rows at a time: rows
// [beg, beg + n) of `rows` go to box[0 .. n) / box_cls[0 .. n), a row per thread and step (the caller's barriers around it).
#define PAIR_CHUNK 512
__device__ __forceinline__ void stage_boxes(const int32_t *__restrict__ rows, int beg, int n, int4 *box, int *box_cls) {
  for (int k = threadIdx.x; k < n; k += 256) {
    const int32_t *r = rows + (int64_t)(beg + k) * 5;
    box[k] = make_int4(r[0], r[1], r[2], r[3]);
    box_cls[k] = r[4];
  }
}

// K10 sparse index aggregation (row f3, derived_meshes.py:470-520): one thread per face walks the views of the batch;
//     a finite winner value v is one observation of class int(v): counts[f] += 1 and the pair key f * n_classes + class
//     is appended to `keys` (wave ballot + one atomic per wave).  The pairs are counted later by sort + run-length.
__global__ __launch_bounds__(256) void k_emit_index_pairs(uint32_t *__restrict__ winner, const double *__restrict__ img,
                                                          int n_views, int64_t F, int64_t P, long long n_classes,
                                                          uint32_t *__restrict__ counts,
                                                          unsigned long long *__restrict__ keys, long long key_cap,
                                                          unsigned long long *__restrict__ key_count,
                                                          int *__restrict__ bad) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t c = 0;
  for (int v = 0; v < n_views; ++v) {
    bool has = false;
    long long cls = -1;
    const uint32_t key = f < F ? take_winner(winner, v, F, f) : 0u;
    if (key != 0) {
      const double x = img[(int64_t)v * P + (key - 1)];
      has = isfinite(x);
      // astype(int) truncates toward zero: the class lies in [0, n_classes) exactly when -1 < x < n_classes (exact in
      // double: n_classes <= 2^53).  Decided before the conversion, which is undefined for |x| >= 2^63: a value that
      // fails is never converted and goes on as class -1.
      if (x > -1.0 && x < (double)n_classes) cls = (long long)x;
    }
    if (has) ++c;
    emit_class(has, cls, f, n_classes, keys, key_cap, key_count, bad);
  }
  if (f < F && c) counts[f] += c;
}

// K10r sparse index aggregation of rectangle labels (detections / image IDs): K10 with the label image replaced by a
//     lookup.  The winner pixel p = (p / w, p % w) takes the class of the LAST rectangle of its view's list that contains it
//     (the list is in paint order: a later rectangle overwrites an earlier one); no rectangle = no observation.  The view's
//     rectangles are staged in LDS in chunks of PAIR_CHUNK, walked from the end; a block stops at the first chunk in which
//     none of its faces is still searching.  rects: int32 rows {imin, jmin, imax, jmax, class}, half-open, already clipped
//     to the image; offs: per view [offs[v], offs[v + 1]) into rects.
__global__ __launch_bounds__(256) void k_emit_rect_pairs(uint32_t *__restrict__ winner, const int32_t *__restrict__ rects,
                                                         const int32_t *__restrict__ offs, int n_views, int64_t F, int w,
                                                         long long n_classes, uint32_t *__restrict__ counts,
                                                         unsigned long long *__restrict__ keys, long long key_cap,
                                                         unsigned long long *__restrict__ key_count,
                                                         int *__restrict__ bad) {
  __shared__ int4 box[PAIR_CHUNK];
  __shared__ int box_cls[PAIR_CHUNK];
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t c = 0;
  for (int v = 0; v < n_views; ++v) {
    int pi = 0, pj = 0;
    const uint32_t key = f < F ? take_winner(winner, v, F, f) : 0u;
    bool searching = key != 0;
    if (searching) winner_row_col(key, w, pi, pj);
    bool found = false;
    int cls = 0;
    const int r0 = offs[v], r1 = offs[v + 1];
    for (int end = r1; end > r0; end -= PAIR_CHUNK) {
      // also the barrier that lets the chunk before this one (or the previous view's last one) be overwritten
      if (!__syncthreads_or(searching)) break;
      const int beg = end - PAIR_CHUNK > r0 ? end - PAIR_CHUNK : r0;
      const int n = end - beg;
      stage_boxes(rects, beg, n, box, box_cls);
      __syncthreads();
      if (searching) {
        for (int k = n - 1; k >= 0; --k) {
          const int4 b = box[k];
          if (pi >= b.x && pj >= b.y && pi < b.z && pj < b.w) {
            cls = box_cls[k];
            found = true;
            searching = false;
            break;
          }
        }
      }
    }
    if (found) ++c;
    emit_class(found, cls, f, n_classes, keys, key_cap, key_count, bad);
  }
  if (f < F && c) counts[f] += c;
}

// The fill rule of skimage.draw.polygon for one pixel (x = column, y = row) and one ring of nv >= 1 vertices (row, col), in
// double and in the host restatement's operation order (predictors/derived_segmentors.py, _ring_contains; every operation is
// rounded on its own: -ffp-contract=off): edges in vertex order starting from the last vertex; a pixel within 1e-12 of a
// vertex, or with differing parities of its right and left crossings (on an edge), is inside; otherwise inside iff the right
// crossings are odd.  The quotient -- the only fp64 division -- is formed for the edges that straddle the pixel's row alone.
__device__ __forceinline__ bool ring_contains(const double *__restrict__ vp, int nv, double x, double y) {
  const double eps = 1e-12;
  uint32_t right = 0, left = 0;
  double y0 = vp[2 * (int64_t)(nv - 1)] - y, x0 = vp[2 * (int64_t)(nv - 1) + 1] - x;
  for (int i = 0; i < nv; ++i) {
    const double y1 = vp[2 * (int64_t)i] - y, x1 = vp[2 * (int64_t)i + 1] - x;
    if (-eps < x0 && x0 < eps && -eps < y0 && y0 < eps) return true;
    const bool up = (y0 > 0.0) != (y1 > 0.0), down = (y0 < 0.0) != (y1 < 0.0);
    if (up || down) {
      const double q = (x0 * y1 - x1 * y0) / (y1 - y0);
      if (up && q > 0.0) ++right;
      if (down && q < 0.0) ++left;
    }
    x0 = x1;
    y0 = y1;
  }
  return ((right ^ left) & 1u) != 0u || (right & 1u) != 0u;
}

// K10p sparse index aggregation of polygon labels (region detections): K10r with rings in place of rectangles and a multi-hot
//     answer.  The winner pixel of a face belongs to every class that has at least one ring of the view containing it: ONE
//     pair (face, class) per class and view, however many rings of the class contain the pixel, and counts[f] += 1 when any
//     ring does.  boxes: int32 rows {imin, jmin, imax, jmax, class}, a ring's clipped candidate box, half-open, SORTED BY CLASS
//     within a view; voffs: ring r's vertices are verts[voffs[r] .. voffs[r + 1]) (double (row, col) pairs); offs: view v's
//     rings are [offs[v], offs[v + 1]).  The ring records are staged in LDS in chunks of PAIR_CHUNK and walked in order;
//     the vertices of a ring are read from global memory on a box hit only, and not at all once the face's pixel has been
//     found in the ring's class.  Because the table is class-sorted, the end of a class run is a point the whole block
//     reaches together (the records are the same LDS words for every lane): one ballot there, one append if a lane hit.
__global__ __launch_bounds__(256) void k_emit_polygon_pairs(uint32_t *__restrict__ winner, const int32_t *__restrict__ boxes,
                                                            const int32_t *__restrict__ voffs, const double *__restrict__ verts,
                                                            const int32_t *__restrict__ offs, int n_views, int64_t F, int w,
                                                            long long n_classes, uint32_t *__restrict__ counts,
                                                            unsigned long long *__restrict__ keys, long long key_cap,
                                                            unsigned long long *__restrict__ key_count,
                                                            int *__restrict__ bad) {
  __shared__ int4 box[PAIR_CHUNK];
  __shared__ int box_cls[PAIR_CHUNK];
  __shared__ int vert_beg[PAIR_CHUNK + 1];
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t c = 0;
  for (int v = 0; v < n_views; ++v) {
    int pi = 0, pj = 0;
    const uint32_t key = f < F ? take_winner(winner, v, F, f) : 0u;
    const bool live = key != 0;
    if (live) winner_row_col(key, w, pi, pj);
    const double px = (double)pj, py = (double)pi;
    bool hit = false, any = false;  // in a ring of the run's class; in any ring of the view
    int run_cls = 0;
    const int r0 = offs[v], r1 = offs[v + 1];
    for (int beg = r0; beg < r1; beg += PAIR_CHUNK) {
      // also the barrier that lets the chunk before this one (or the previous view's last one) be overwritten; a block that
      // shows no face of the view has nothing to look up
      if (!__syncthreads_or(live)) break;
      const int n = r1 - beg < PAIR_CHUNK ? r1 - beg : PAIR_CHUNK;
      stage_boxes(boxes, beg, n, box, box_cls);
      for (int k = threadIdx.x; k <= n; k += 256) vert_beg[k] = voffs[beg + k];
      __syncthreads();
      for (int k = 0; k < n; ++k) {
        const int cls = box_cls[k];
        if (cls != run_cls) {  // the same LDS word in every lane: the block takes this branch together
          emit_class(hit, run_cls, f, n_classes, keys, key_cap, key_count, bad);  // the end of a class run
          hit = false;
          run_cls = cls;
        }
        if (live && !hit) {
          const int4 b = box[k];
          if (pi >= b.x && pj >= b.y && pi < b.z && pj < b.w) {
            const int vb = vert_beg[k], nv = vert_beg[k + 1] - vb;
            if (nv > 0 && ring_contains(verts + 2 * (int64_t)vb, nv, px, py)) hit = any = true;
          }
        }
      }
    }
    emit_class(hit, run_cls, f, n_classes, keys, key_cap, key_count, bad);
    if (any) ++c;
  }
  if (f < F && c) counts[f] += c;
}

__global__ __launch_bounds__(256) void k_finalize_votes(const uint32_t *__restrict__ votes,
                                                        const uint32_t *__restrict__ counts, int64_t F, int C,
                                                        double *__restrict__ average, double *__restrict__ summed,
                                                        double *__restrict__ counts_f64) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= F * C) return;
  const int64_t f = i / C;
  const uint32_t c = counts[f];
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  const double s = c ? (double)votes[i] : nan;
  summed[i] = s;
  average[i] = c ? s / (double)c : nan;  // numpy: nan / 0 = nan
  if (i == f * C) counts_f64[f] = (double)c;
}

__global__ __launch_bounds__(256) void k_finalize_sums(double *__restrict__ sums, const uint32_t *__restrict__ counts,
                                                       int64_t F, int C, double *__restrict__ average,
                                                       double *__restrict__ counts_f64) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= F * C) return;
  const int64_t f = i / C;
  const uint32_t c = counts[f];
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  const double s = c ? sums[i] : nan;
  sums[i] = s;
  average[i] = c ? s / (double)c : nan;
  if (i == f * C) counts_f64[f] = (double)c;
}

// numpy's pairwise sum of n contiguous values (the order np.sum(a, axis=1) takes on a C-contiguous row): fewer than 8 values
// are added one by one from zero; up to 128 go to eight accumulators r[k] += a[8i + k], combined as
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), and the n % 8 tail is added one by one; more are split at
// n2 = n / 2 - (n / 2) % 8 and both halves summed the same way.
template <typename T>
__device__ T leaf_sum(const T *a, int n) {
  if (n < 8) {
    T res = (T)0;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  T r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = a[k];
  int i = 8;
  for (; i <= n - 8; i += 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] += a[i + k];
  }
  T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

// The recursion is walked leaf by leaf, left to right, without a call stack: `path` holds the turns from the root to the
// current node (bit k set: the right half at depth k), a node's (offset, length) is found again by walking down from the
// root, and the sums of left halves whose right half is still open wait in `left` -- a last-in first-out stack kept in
// registers (shifted, never indexed by a run-time value: no scratch memory).  Any int n splits at most PW_DEPTH times.
#define PW_DEPTH 25
template <typename T>
__device__ T numpy_pairwise_sum(const T *a, int n) {
  T left[PW_DEPTH];
  uint32_t path = 0;
  int depth = 0, off = 0, len = n;
  T v;
  for (;;) {
    while (len > 128) {  // down the left halves
      int n2 = len / 2;
      n2 -= n2 % 8;
      len = n2;
      ++depth;
    }
    v = leaf_sum(a + off, len);
    while (depth > 0 && ((path >> (depth - 1)) & 1u)) {  // a right half done: add it to its left half, go up
      v = left[0] + v;
#pragma unroll
      for (int k = 0; k < PW_DEPTH - 1; ++k) left[k] = left[k + 1];
      path &= ~(1u << (depth - 1));
      --depth;
    }
    if (depth == 0) break;
#pragma unroll
    for (int k = PW_DEPTH - 1; k > 0; --k) left[k] = left[k - 1];
    left[0] = v;  // a left half done: keep its sum, go to its right half
    path |= 1u << (depth - 1);
    off = 0;
    len = n;
    for (int k = 0; k < depth; ++k) {
      int n2 = len / 2;
      n2 -= n2 % 8;
      if ((path >> k) & 1u) { off += n2; len -= n2; }
      else len = n2;
    }
  }
  return v;
}

// utils/indexing.py:9-32 on float32 or float64 rows: the row sum in numpy's order and precision (a row whose sum is zero
// in that order is NaN), np.argmax's first maximum with the first NaN winning.
template <typename T>
__global__ __launch_bounds__(256) void k_argmax_nonzero(const T *__restrict__ arr, int64_t F, int C,
                                                        double *__restrict__ out) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const T *row = arr + f * C;
  T best = row[0];
  int arg = 0;
  bool bad = false;
  // np.argmax: first maximum; a NaN is "maximal" and the first NaN wins
  bool best_nan = isnan(best);
  for (int c = 0; c < C; ++c) {
    const T x = row[c];
    if (!isfinite(x)) bad = true;
    if (c > 0 && !best_nan) {
      if (isnan(x)) { best_nan = true; arg = c; }
      else if (x > best) { best = x; arg = c; }
    }
  }
  out[f] = (bad || numpy_pairwise_sum(row, C) == (T)0) ? __longlong_as_double(0x7FF8000000000000ll) : (double)arg;
}

}  // namespace

namespace grimpl {

// the fused aggregation's vote pass of one launch group (raster_views, geograster.hip)
void launch_vote_labels(gr_ctx *c, hipStream_t vs, uint32_t *win, const uint8_t *labels, int nb, int64_t F, int64_t P, int C,
                        uint32_t *votes, uint32_t *counts, int group, const uint32_t *touched, int tw) {
  Timed t(c, vs, ST_VOTE);
  hipLaunchKernelGGL(k_vote_labels, dim3((unsigned)ceil_div(F, 256)), dim3(256), 0, vs, win, labels, nb, F, P, C, votes, counts,
                     (const unsigned long long *)c->stats, group, touched, tw, touched ? c->visits : (uint32_t *)nullptr);
}

}  // namespace grimpl

namespace {

// What every projection entry point checks before its own arguments: the shape, then the mesh.
int check_projection(gr_ctx *c, int n_views, int h, int w) {
  int rc = check_common(c, n_views, h, w);
  if (rc) return rc;
  if (c->F <= 0) return fail(c, GR_ENOMESH, "gr_mesh_upload has not been called");
  return GR_OK;
}

// The "a value is no class index" check of the three pair entry points.  The consumer kernel ORs into `flag`: the context's flag
// word, zeroed ahead of the first launch group and read back behind the last (project_groups) -- or, with GR_FLAG_DEFER_CHECK,
// the caller's SECOND 64-bit word behind the pair counter (a word of its own: the counter takes 64-bit atomics, the flag a
// 32-bit one), which nobody reads here.
struct ClassCheck {
  bool defer;
  int *flag;
  const char *message;  // of GR_EINDEX; takes n_classes
  long long n_classes;
  ClassCheck(gr_ctx *c, uint64_t *key_count, int flags, const char *msg, int64_t nc)
      : defer((flags & GR_FLAG_DEFER_CHECK) != 0), flag(defer ? reinterpret_cast<int *>(key_count + 1) : c->flag), message(msg),
        n_classes((long long)nc) {}
};

// The launch-group protocol behind every projection entry point, once the arguments are checked: winner scratch for
// min(n_views, GR_MAX_BATCH) views, then per group of that many views the winners of its id images (ST_PROJECT) and the caller's
// consumer launch(es) `consume(win, v0, nb)` over views [v0, v0 + nb) (ST_VOTE), which leave the winners cleared.
template <typename Consumer>
int project_groups(gr_ctx *c, const int32_t *ids, int n_views, int h, int w, int flags, void *stream, Consumer consume,
                   const ClassCheck *check = nullptr) {
  if (n_views == 0) return GR_OK;
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  const int64_t P = (int64_t)h * w, F = c->F;
  const int B = n_views < GR_MAX_BATCH ? n_views : GR_MAX_BATCH;
  int rc = reserve_winner(c, F * B, s);
  if (rc) return rc;
  note_stream(c, s);
  uint32_t *win = c->winner;
  const int compat = (flags & GR_FLAG_NEG1_IS_LAST_FACE) ? 1 : 0;
  if (check && !check->defer) GR_HIP(c, hipMemsetAsync(c->flag, 0, sizeof(int), s));
  for (int v0 = 0; v0 < n_views; v0 += B) {
    const int nb = (n_views - v0) < B ? (n_views - v0) : B;
    {
      Timed t(c, s, ST_PROJECT);
      hipLaunchKernelGGL(k_winner, dim3((unsigned)ceil_div(ceil_div(w, 4), 256), (unsigned)ceil_div(h, WIN_ROWS), nb), dim3(256), 0,
                         s, ids + v0 * P, win, F, h, w, compat);
    }
    {
      Timed t(c, s, ST_VOTE);
      consume(win, v0, nb);
    }
  }
  GR_HIP(c, hipGetLastError());
  if (!check || check->defer) return GR_OK;
  int bad = 0;
  GR_HIP(c, hipMemcpyAsync(&bad, c->flag, sizeof(int), hipMemcpyDeviceToHost, s));
  GR_HIP(c, hipStreamSynchronize(s));
  if (bad) return fail(c, GR_EINDEX, check->message, check->n_classes);
  return GR_OK;
}

// What the three pair entry points share.  The constructor checks the shape, the mesh and the arguments all three take
// (`own_ptrs`: the entry point's own pointers are there) and leaves the code in `rc`; run() then makes the ClassCheck with the
// entry point's GR_EINDEX text and drives `launch(win, v0, nb, bad)` through the launch groups.  The members are the arguments
// every emit kernel takes, in the kernels' types (the pointers stay separate kernel parameters: polygons.hip).
struct PairCall {
  gr_ctx *c;
  const int32_t *ids;
  int n_views, h, w, flags;
  void *stream;
  hipStream_t s;
  long long n_classes, key_cap;
  unsigned long long *keys, *key_count;
  int rc;
  int64_t F = 0;
  dim3 grid;  // a thread per face
  PairCall(gr_ctx *c, const int32_t *ids, bool own_ptrs, int n_views, int h, int w, int64_t n_classes, const uint32_t *counts,
           uint64_t *keys, int64_t key_cap, uint64_t *key_count, int flags, void *stream)
      : c(c), ids(ids), n_views(n_views), h(h), w(w), flags(flags), stream(stream), s((hipStream_t)stream),
        n_classes((long long)n_classes), key_cap((long long)key_cap), keys((unsigned long long *)keys),
        key_count((unsigned long long *)key_count), rc(check_projection(c, n_views, h, w)) {
    if (rc) return;
    if (!ids || !own_ptrs || !counts || !keys || !key_count || n_classes <= 0 || key_cap < 0)
      rc = fail(c, GR_EINVAL, "bad sparse projection args");
    F = c->F;
    grid = dim3((unsigned)ceil_div(F, 256));
  }
  template <typename Launch>
  int run(const char *message, Launch launch) {
    const ClassCheck check(c, (uint64_t *)key_count, flags, message, n_classes);
    return project_groups(c, ids, n_views, h, w, flags, stream,
                          [&](uint32_t *win, int v0, int nb) { launch(win, v0, nb, check.flag); }, &check);
  }
};

}  // namespace

extern "C" {

int gr_gather_texture_f64(gr_ctx *c, const int32_t *ids, int64_t n_pix, const double *face_tex, int64_t F, int C,
                          double *out, void *stream) {
  if (!c || !ids || !face_tex || !out || n_pix < 0 || F <= 0 || C <= 0) return fail(c, GR_EINVAL, "bad gather args");
  if (n_pix == 0) return GR_OK;
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  Timed t(c, s, ST_GATHER);
  hipLaunchKernelGGL(k_gather_texture, dim3((unsigned)ceil_div(n_pix * C, 256)), dim3(256), 0, s, ids, n_pix, face_tex,
                     F, C, out);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

int gr_project_labels_u8(gr_ctx *c, const int32_t *ids, const uint8_t *labels, int n_views, int h, int w, int C,
                         uint32_t *votes, uint32_t *counts, int flags, void *stream) {
  int rc = check_projection(c, n_views, h, w);
  if (rc) return rc;
  if (!ids || !labels || !votes || !counts || C <= 0 || C > 255) return fail(c, GR_EINVAL, "bad project args C=%d", C);
  const int64_t P = (int64_t)h * w, F = c->F;
  hipStream_t s = (hipStream_t)stream;
  return project_groups(c, ids, n_views, h, w, flags, stream, [&](uint32_t *win, int v0, int nb) {
    hipLaunchKernelGGL(k_vote_labels, dim3((unsigned)ceil_div(F, 256)), dim3(256), 0, s, win, labels + v0 * P, nb, F, P, C,
                       votes, counts, (const unsigned long long *)nullptr, 0, (const uint32_t *)nullptr, 0, (uint32_t *)nullptr);
  });
}

int gr_project_values_f64(gr_ctx *c, const int32_t *ids, const double *img, int n_views, int h, int w, int C,
                          double *sums, uint32_t *counts, int flags, void *stream) {
  int rc = check_projection(c, n_views, h, w);
  if (rc) return rc;
  if (!ids || !img || !sums || !counts || C <= 0) return fail(c, GR_EINVAL, "bad project args");
  const int64_t P = (int64_t)h * w, F = c->F;
  hipStream_t s = (hipStream_t)stream;
  return project_groups(c, ids, n_views, h, w, flags, stream, [&](uint32_t *win, int v0, int nb) {
    hipLaunchKernelGGL(k_vote_values, dim3((unsigned)ceil_div(F, 256)), dim3(256), 0, s, win, img + v0 * P * C, nb, F, P, C,
                       sums, counts);
  });
}

int gr_project_view_f64(gr_ctx *c, const int32_t *ids, const double *img, int h, int w, int C, double *tex, int flags,
                        void *stream) {
  int rc = check_projection(c, 1, h, w);
  if (rc) return rc;
  if (!ids || !img || !tex || C <= 0) return fail(c, GR_EINVAL, "bad project args");
  const int64_t F = c->F;
  hipStream_t s = (hipStream_t)stream;
  return project_groups(c, ids, 1, h, w, flags, stream, [&](uint32_t *win, int, int) {  // one view: one group
    hipLaunchKernelGGL(k_project_view, dim3((unsigned)ceil_div(F * C, 256)), dim3(256), 0, s, win, img, F, C, tex);
    hipLaunchKernelGGL(k_clear_u32, dim3((unsigned)ceil_div(F, 256)), dim3(256), 0, s, win, F);
  });
}

int gr_gather_texture_u8(gr_ctx *c, const int32_t *ids, int64_t n_pix, const double *face_tex, int64_t F, int C,
                         int null_value, uint8_t *out, void *stream) {
  if (!c) return GR_EINVAL;
  if (!ids || !face_tex || !out || n_pix < 0 || F <= 0 || C <= 0 || null_value < 0 || null_value > 255)
    return fail(c, GR_EINVAL, "bad gather args");
  if (n_pix == 0) return GR_OK;
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  Timed t(c, s, ST_GATHER);
  hipLaunchKernelGGL(k_gather_texture_u8, dim3((unsigned)ceil_div(n_pix * C, 256)), dim3(256), 0, s, ids, n_pix, face_tex,
                     F, C, (uint8_t)null_value, out);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

int gr_project_index_pairs(gr_ctx *c, const int32_t *ids, const double *img, int n_views, int h, int w, int64_t n_classes,
                           uint32_t *counts, uint64_t *keys, int64_t key_cap, uint64_t *key_count, int flags,
                           void *stream) {
  PairCall p(c, ids, img != nullptr, n_views, h, w, n_classes, counts, keys, key_cap, key_count, flags, stream);
  if (p.rc) return p.rc;
  if (n_classes > (1ll << 53)) return fail(c, GR_EINVAL, "n_classes %lld exceeds 2^53", (long long)n_classes);
  const int64_t P = (int64_t)h * w;
  return p.run("an image value is not a class index in [0, %lld)", [&](uint32_t *win, int v0, int nb, int *bad) {
    hipLaunchKernelGGL(k_emit_index_pairs, p.grid, dim3(256), 0, p.s, win, img + v0 * P, nb, p.F, P, p.n_classes, counts, p.keys,
                       p.key_cap, p.key_count, bad);
  });
}

int gr_project_rect_pairs(gr_ctx *c, const int32_t *ids, const int32_t *rects, const int32_t *rect_offsets, int n_views,
                          int h, int w, int64_t n_classes, uint32_t *counts, uint64_t *keys, int64_t key_cap,
                          uint64_t *key_count, int flags, void *stream) {
  PairCall p(c, ids, rect_offsets != nullptr, n_views, h, w, n_classes, counts, keys, key_cap, key_count, flags, stream);
  if (p.rc) return p.rc;
  return p.run("a rectangle's class is not a class index in [0, %lld)", [&](uint32_t *win, int v0, int nb, int *bad) {
    hipLaunchKernelGGL(k_emit_rect_pairs, p.grid, dim3(256), 0, p.s, win, rects, rect_offsets + v0, nb, p.F, w, p.n_classes,
                       counts, p.keys, p.key_cap, p.key_count, bad);
  });
}

int gr_project_polygon_pairs(gr_ctx *c, const int32_t *ids, const int32_t *boxes, const int32_t *vert_offsets,
                             const double *verts, const int32_t *poly_offsets, int n_views, int h, int w, int64_t n_classes,
                             uint32_t *counts, uint64_t *keys, int64_t key_cap, uint64_t *key_count, int flags, void *stream) {
  PairCall p(c, ids, vert_offsets && poly_offsets, n_views, h, w, n_classes, counts, keys, key_cap, key_count, flags, stream);
  if (p.rc) return p.rc;
  return p.run("a polygon's class is not a class index in [0, %lld)", [&](uint32_t *win, int v0, int nb, int *bad) {
    hipLaunchKernelGGL(k_emit_polygon_pairs, p.grid, dim3(256), 0, p.s, win, boxes, vert_offsets, verts, poly_offsets + v0, nb,
                       p.F, w, p.n_classes, counts, p.keys, p.key_cap, p.key_count, bad);
  });
}

int gr_count_pairs(gr_ctx *c, uint64_t *keys, int64_t n, uint64_t *unique_keys, uint32_t *pair_counts, int64_t *n_unique_h,
                   void *stream) {
  if (!c) return GR_EINVAL;
  if (!keys || !unique_keys || !pair_counts || !n_unique_h || n < 0 || n > 0x7FFFFFFFll)
    return fail(c, GR_EINVAL, "bad pair-count args");
  *n_unique_h = 0;
  if (n == 0) return GR_OK;
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  // radix sort (keys -> sorted copy in context scratch) + run-length encode, both rocPRIM through hipcub
  unsigned long long *kin = (unsigned long long *)keys, *uo = (unsigned long long *)unique_keys;
  // scratch: sorted [n] | rocPRIM
  Plan p;
  const auto sorted = p.array<unsigned long long>(n);
  const SortKeys<unsigned long long> sort(c, p, n, 64);
  const RunLengthEncode<unsigned long long, uint32_t> encode(c, p, n);
  int rc = stage_acquire(c, c->stage, p.finish(), s, "sort");
  if (rc != GR_OK) return rc;
  p.base = c->stage.ptr;
  GR_TRY(sort.run(kin, sorted(), s));
  GR_TRY(encode.run(sorted(), uo, pair_counts, (int *)c->flag, s));
  int runs = 0;
  GR_HIP(c, hipMemcpyAsync(&runs, c->flag, sizeof(int), hipMemcpyDeviceToHost, s));
  GR_HIP(c, hipStreamSynchronize(s));
  *n_unique_h = runs;
  return GR_OK;
}

int gr_finalize_votes(gr_ctx *c, const uint32_t *votes, const uint32_t *counts, int64_t F, int C, double *average,
                      double *summed, double *counts_f64, void *stream) {
  if (!c || !votes || !counts || !average || !summed || !counts_f64 || F <= 0 || C <= 0)
    return fail(c, GR_EINVAL, "bad finalize args");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(k_finalize_votes, dim3((unsigned)ceil_div(F * C, 256)), dim3(256), 0, s, votes, counts, F, C,
                     average, summed, counts_f64);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

int gr_finalize_sums_f64(gr_ctx *c, double *sums, const uint32_t *counts, int64_t F, int C, double *average,
                         double *counts_f64, void *stream) {
  if (!c || !sums || !counts || !average || !counts_f64 || F <= 0 || C <= 0)
    return fail(c, GR_EINVAL, "bad finalize args");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(k_finalize_sums, dim3((unsigned)ceil_div(F * C, 256)), dim3(256), 0, s, sums, counts, F, C,
                     average, counts_f64);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

int gr_argmax_nonzero(gr_ctx *c, const void *array, int dtype, int64_t F, int C, double *out, void *stream) {
  if (!c) return GR_EINVAL;
  if (F < 0 || C <= 0) return fail(c, GR_EINVAL, "bad argmax args");
  if (dtype != GR_DTYPE_F32 && dtype != GR_DTYPE_F64) return fail(c, GR_EINVAL, "argmax dtype %d is not f32 / f64", dtype);
  if (F == 0) return GR_OK;  // (an empty tensor's data pointer may be null)
  if (!array || !out) return fail(c, GR_EINVAL, "bad argmax args");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  if (dtype == GR_DTYPE_F32)
    hipLaunchKernelGGL(k_argmax_nonzero<float>, dim3((unsigned)ceil_div(F, 256)), dim3(256), 0, s, (const float *)array, F,
                       C, out);
  else
    hipLaunchKernelGGL(k_argmax_nonzero<double>, dim3((unsigned)ceil_div(F, 256)), dim3(256), 0, s, (const double *)array,
                       F, C, out);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

int gr_argmax_nonzero_f64(gr_ctx *c, const double *array, int64_t F, int C, double *out, void *stream) {
  return gr_argmax_nonzero(c, array, GR_DTYPE_F64, F, C, out, stream);
}

}  // extern "C"
