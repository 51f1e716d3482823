// geograypher_amd/csrc/overlap.hip -- polygon-on-polygon overlap areas (gr_polygon_box_pairs_count, gr_polygon_box_pairs_fill,
// gr_polygon_overlap_areas; the rule-set A1-A9 is DESIGN.md section 8o).  Two ring tables on the 1e-6 m grid behind one origin; no
// clipping, no sorting of intersections, no topological decision: the area of a n b is the signed sum, over the non-vertical edges
// e of a and f of b, of the area under the LOWER of the two segments over their common x-range (A5).  Needs no uploaded mesh.
//
// Pair join (A2), count then fill.  One row of A per lane; the boxes of B are walked wave-uniformly (every lane reads box b at the
// same address).  boxes_pair is THE predicate of both phases; an exclusive scan (cub_steps.hpp) of the counts lies between them; a
// lane fills its own slice in ascending b, so the list is ascending by (a, b).
//
// Areas.  A workgroup takes one work item (A8): a pair, at most GR_OVERLAP_TILE_A consecutive edge slots of row a and at most
// GR_OVERLAP_TILE_B of row b.  The a-tile is staged in LDS as prepared edge records (EdgeRec: the ordered end points relative to
// (X0, Y) -- integers below 2^41, exact in a double, so the x-cull of A3 in doubles IS the integer decision --, slope, sign); every
// lane strides over the b-tile, prepares its b-edge once and walks the a-tile from LDS, every read a broadcast.  A lane keeps one
// edge record, two sums and one count: no scratch memory.  Determinism (A7): a lane sums in a fixed order, the 64 lanes of a wave
// meet in a butterfly (both partners form the same commutative sum), the four waves are added in wave order, an item's partial
// goes to scratch and k_overlap_reduce adds the partials of a pair in item order.  No floating-point atomic anywhere.
//
// Items must name their pairs in non-decreasing order.  k_overlap_item_keys writes the pair of every item (-1: none), an inclusive
// running maximum follows (cub_steps.hpp), and an item is ORDERED iff its key is >= 0 and not below the maximum before it; the
// ordered items are then non-decreasing whatever the others hold, the first ordered item of a pair is the pair's head, and the
// head's lane adds the partials up to the next larger key.  An item that is not ordered, or names a slot outside its rows, is
// skipped whole, leaves a zero partial and is counted (A8).
#include "cub_steps.hpp"
#include "geom_dev.hpp"
#include "gr_internal.hpp"

namespace {
using namespace grimpl;

typedef unsigned long long u64;

// A2, stated once: the boxes (xmin ymin xmax ymax) overlap with positive width AND positive height.  The empty box (1, 1, 0, 0)
// pairs with nothing: against any box the smaller xmax is <= 0 < 1 <= the larger xmin.
__device__ __forceinline__ bool boxes_pair(const int64_t *__restrict__ a, const int64_t *__restrict__ b) {
  return max(a[0], b[0]) < min(a[2], b[2]) && max(a[1], b[1]) < min(a[3], b[3]);
}

// counts [Pa + 1]: the rows of B that pair with row a; counts [Pa] = 0, so that the exclusive scan ends in the total.
__global__ __launch_bounds__(256) void k_overlap_pairs_count(const int64_t *__restrict__ boxes_a, int64_t Pa, const int64_t *__restrict__ boxes_b,
                                                             int64_t Pb, u64 *__restrict__ counts) {
  const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (a > Pa) return;
  u64 n = 0;
  if (a < Pa) {
    int64_t box[4] = {boxes_a[a * 4], boxes_a[a * 4 + 1], boxes_a[a * 4 + 2], boxes_a[a * 4 + 3]};
    for (int64_t b = 0; b < Pb; ++b) n += boxes_pair(box, boxes_b + b * 4) ? 1u : 0u;
  }
  counts[a] = n;
}

// pairs [n_pairs][2]: row a writes its slice [offsets[a], offsets[a + 1]) in ascending b; nothing outside the slice or the list.
__global__ __launch_bounds__(256) void k_overlap_pairs_fill(const int64_t *__restrict__ boxes_a, int64_t Pa, const int64_t *__restrict__ boxes_b,
                                                            int64_t Pb, const int64_t *__restrict__ offsets, int32_t *__restrict__ pairs,
                                                            int64_t n_pairs) {
  const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (a >= Pa) return;
  int64_t box[4] = {boxes_a[a * 4], boxes_a[a * 4 + 1], boxes_a[a * 4 + 2], boxes_a[a * 4 + 3]};
  int64_t pos = offsets[a];
  const int64_t end = min(offsets[a + 1], n_pairs);
  if (pos < 0) return;
  for (int64_t b = 0; b < Pb; ++b) {
    if (!boxes_pair(box, boxes_b + b * 4)) continue;
    if (pos < end) { pairs[pos * 2] = (int32_t)a; pairs[pos * 2 + 1] = (int32_t)b; }
    ++pos;
  }
}

// The statistics of a ring table (RingTable, ring_of_slot: geom_dev.hpp): one lane per ring (ring_stats: the largest ring, rings
// ignored) and per vertex slot (vertical edges of the rings that take part).
__global__ __launch_bounds__(256) void k_overlap_table_stats(RingTable t, u64 *__restrict__ stats) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  ring_stats<GR_OVERLAP_STAT_LARGEST_RING, GR_OVERLAP_STAT_RINGS_IGNORED>(t.roff, t.R, t.n_rv, i, stats, lane);
  bool vertical = false;
  if (i < t.n_rv && t.R > 0) {
    int64_t i0;
    const int64_t r = ring_of_slot(t.roff, 0, t.R, i);
    const int64_t m = ring_span(t.roff, (int)r, t.n_rv, i0);
    if (m >= 3 && i >= i0 && i < i0 + m) {
      const int64_t j = i + 1 == i0 + m ? i0 : i + 1;
      vertical = t.rv[i * 2] == t.rv[j * 2];
    }
  }
  stat_count(stats, GR_OVERLAP_STAT_VERTICAL, vertical, lane);
}

__global__ void k_overlap_stat_pairs(u64 *__restrict__ stats, u64 n_pairs) {
  if (threadIdx.x == 0) stats[GR_OVERLAP_STAT_PAIRS] = n_pairs;
}

// key [n_items]: the pair an item names, -1 when it names none.
__global__ __launch_bounds__(256) void k_overlap_item_keys(const int32_t *__restrict__ items, int64_t n_items, int64_t n_pairs,
                                                           int32_t *__restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_items) return;
  const int32_t p = items[i * GR_OVERLAP_ITEM_INTS];
  key[i] = p >= 0 && p < n_pairs ? p : -1;
}

// ordered: the item's key is a pair and not below any key in front of it (runmax: the inclusive running maximum of the keys)
__device__ __forceinline__ bool item_ordered(const int32_t *__restrict__ key, const int32_t *__restrict__ runmax, int64_t i) {
  return key[i] >= 0 && (i == 0 || key[i] >= runmax[i - 1]);
}

// A prepared edge (A3-A5): the end points ordered by x, relative to (X0, Y) -- integers, exact --, the slope, rounded once, and the
// sign s = -sigma sgn(x1 - x0), sigma = -1 for a hole.  xl = 1, xr = 0, s = 0: the slot takes no part (a vertical edge, a ring of
// fewer than 3 vertices): no x-range meets it.
struct EdgeRec { double xl, xr, yl, m, s, pad; };

__device__ __forceinline__ EdgeRec no_edge() { EdgeRec e; e.xl = 1.0; e.xr = 0.0; e.yl = 0.0; e.m = 0.0; e.s = 0.0; e.pad = 0.0; return e; }

// The ring of row `row` that holds vertex slot i, among the rings [r_lo, r_hi): its index, first vertex and length; -1 when the
// slot lies in no ring of that row.  Nothing is read outside the tables.
__device__ __forceinline__ int64_t locate_slot(const RingTable &t, int64_t row, int64_t r_lo, int64_t r_hi, int64_t i, int64_t &i0, int64_t &n) {
  const int64_t r = ring_of_slot(t.roff, r_lo, r_hi, i);
  n = ring_span(t.roff, (int)r, t.n_rv, i0);
  return (int64_t)t.rpoly[r] == row && i >= i0 && i < i0 + n ? r : -1;
}

// The record of vertex slot i (a slot that locate_slot has found in its row).
__device__ __forceinline__ EdgeRec prepare_edge(const RingTable &t, int64_t row, int64_t r_lo, int64_t r_hi, int64_t i, int64_t X0, int64_t Y) {
  EdgeRec e = no_edge();
  int64_t i0, n;
  const int64_t r = locate_slot(t, row, r_lo, r_hi, i, i0, n);
  if (r < 0 || n < 3) return e;
  const int64_t j = i + 1 == i0 + n ? i0 : i + 1;
  const int64_t x0 = t.rv[i * 2], y0 = t.rv[i * 2 + 1], x1 = t.rv[j * 2], y1 = t.rv[j * 2 + 1];
  if (x0 == x1) return e;   // A4
  const bool rising = x1 > x0;
  e.xl = (double)((rising ? x0 : x1) - X0);
  e.xr = (double)((rising ? x1 : x0) - X0);
  e.yl = (double)((rising ? y0 : y1) - Y);
  const double yr = (double)((rising ? y1 : y0) - Y);
  e.m = (yr - e.yl) / (e.xr - e.xl);
  e.s = (t.rhole[r] != 0) == rising ? 1.0 : -1.0;   // -sigma sgn(x1 - x0)
  return e;
}

// A5: the area under the lower of the segments e and f over [lo, hi], in this order of operations.
__device__ __forceinline__ double edge_pair_integral(const EdgeRec &e, const EdgeRec &f, double lo, double hi) {
  const double he0 = e.yl + e.m * (lo - e.xl), he1 = e.yl + e.m * (hi - e.xl);
  const double hf0 = f.yl + f.m * (lo - f.xl), hf1 = f.yl + f.m * (hi - f.xl);
  const double d_lo = he0 - hf0, d_hi = he1 - hf1, w = hi - lo;
  const double h0 = fmin(he0, hf0), h1 = fmin(he1, hf1);
  if ((d_lo < 0.0 && d_hi > 0.0) || (d_lo > 0.0 && d_hi < 0.0)) {
    const double t = d_lo / (d_lo - d_hi);
    const double w0 = t * w;
    const double hc = e.yl + e.m * ((lo + w0) - e.xl);
    return (0.5 * (h0 + hc)) * w0 + (0.5 * (hc + h1)) * (w - w0);
  }
  return (0.5 * (h0 + h1)) * w;
}

__device__ __forceinline__ double wave_sum_f64(double v) {   // the butterfly: both partners form the same sum, every lane ends with it
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

struct OverlapArgs {
  RingTable a, b;
  int64_t n_pairs, n_items;
};

// items [n_items][GR_OVERLAP_ITEM_INTS]: pair, first slot and slots of row a, first slot and slots of row b; partial [n_items][2]:
// area, area_abs of the item, every word written.
__global__ __launch_bounds__(256) void k_overlap_areas(OverlapArgs g, const int32_t *__restrict__ pairs, const int32_t *__restrict__ items,
                                                       const int32_t *__restrict__ key, const int32_t *__restrict__ runmax,
                                                       double *__restrict__ partial, u64 *__restrict__ stats) {
  __shared__ EdgeRec recs[GR_OVERLAP_TILE_A];
  __shared__ int64_t rr[4];        // the ring ranges of the two tiles
  __shared__ double wsum[4][2];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t item = blockIdx.x;
  const int32_t *it = items + item * GR_OVERLAP_ITEM_INTS;
  const int64_t a0 = it[1], na = it[2], b0 = it[3], nb = it[4];
  // everything up to the barrier below is workgroup-uniform
  bool ok = item_ordered(key, runmax, item) && na >= 1 && na <= GR_OVERLAP_TILE_A && nb >= 1 && nb <= GR_OVERLAP_TILE_B && a0 >= 0 && b0 >= 0 &&
            a0 + na <= g.a.n_rv && b0 + nb <= g.b.n_rv && g.a.R > 0 && g.b.R > 0;
  int64_t row_a = 0, row_b = 0;
  if (ok) {
    row_a = pairs[(int64_t)it[0] * 2]; row_b = pairs[(int64_t)it[0] * 2 + 1];
    ok = row_a >= 0 && row_a < g.a.P && row_b >= 0 && row_b < g.b.P;
  }
  if (!ok) {
    if (tid == 0) { partial[item * 2] = 0.0; partial[item * 2 + 1] = 0.0; atomicAdd(&stats[GR_OVERLAP_STAT_BAD_ITEMS], 1ull); }
    return;
  }
  if (tid < 4) {
    const RingTable &t = tid < 2 ? g.a : g.b;
    const int64_t slot = tid == 0 ? a0 : tid == 1 ? a0 + na - 1 : tid == 2 ? b0 : b0 + nb - 1;
    rr[tid] = ring_of_slot(t.roff, 0, t.R, slot);
  }
  // A3: the x-overlap of the two boxes and the baseline, integers
  const int64_t *ba = g.a.pbox + row_a * 4, *bb = g.b.pbox + row_b * 4;
  const int64_t X0 = max(ba[0], bb[0]), X1 = min(ba[2], bb[2]), Y = min(ba[1], bb[1]);
  const double W = (double)(X1 - X0);
  __syncthreads();
  const int64_t ra_lo = rr[0], ra_hi = rr[1] + 1, rb_lo = rr[2], rb_hi = rr[3] + 1;
  // a slot outside its row is found before anything is summed
  bool bad = false;
  int64_t i0, n;
  if (tid < na) bad = locate_slot(g.a, row_a, ra_lo, ra_hi, a0 + tid, i0, n) < 0;
  for (int64_t k = tid; k < nb; k += 256) bad |= locate_slot(g.b, row_b, rb_lo, rb_hi, b0 + k, i0, n) < 0;
  if (tid < na) recs[tid] = prepare_edge(g.a, row_a, ra_lo, ra_hi, a0 + tid, X0, Y);
  if (__syncthreads_or(bad)) {   // (the barrier also publishes the records)
    if (tid == 0) { partial[item * 2] = 0.0; partial[item * 2 + 1] = 0.0; atomicAdd(&stats[GR_OVERLAP_STAT_BAD_ITEMS], 1ull); }
    return;
  }
  double area = 0.0, area_abs = 0.0;
  uint32_t took_part = 0;   // at most 16 x 256 per lane
  for (int64_t k = tid; k < nb; k += 256) {
    const EdgeRec f = prepare_edge(g.b, row_b, rb_lo, rb_hi, b0 + k, X0, Y);
    if (f.s == 0.0) continue;
    const double f_lo = fmax(f.xl, 0.0), f_hi = fmin(f.xr, W);
    for (int j = 0; j < (int)na; ++j) {
      const EdgeRec e = recs[j];
      const double lo = fmax(e.xl, f_lo), hi = fmin(e.xr, f_hi);
      if (hi > lo) {   // A3: exact -- every operand is an integer below 2^41
        const double v = edge_pair_integral(e, f, lo, hi);
        area += (e.s * f.s) * v;
        area_abs += fabs(v);
        ++took_part;
      }
    }
  }
  area = wave_sum_f64(area);
  area_abs = wave_sum_f64(area_abs);
  if (lane == 0) { wsum[wave][0] = area; wsum[wave][1] = area_abs; }
  stat_add_u32(stats, GR_OVERLAP_STAT_EDGE_PAIRS, took_part, lane);
  __syncthreads();
  if (tid == 0) {
    partial[item * 2] = ((wsum[0][0] + wsum[1][0]) + wsum[2][0]) + wsum[3][0];
    partial[item * 2 + 1] = ((wsum[0][1] + wsum[1][1]) + wsum[2][1]) + wsum[3][1];
    atomicAdd(&stats[GR_OVERLAP_STAT_ITEMS], 1ull);
  }
}

// The partials of a pair, added in item order by the lane of the pair's head: the first ordered item that names it.  area and
// area_abs [n_pairs] are zero on entry; a pair without an item keeps the zeros.
__global__ __launch_bounds__(256) void k_overlap_reduce(const int32_t *__restrict__ key, const int32_t *__restrict__ runmax, int64_t n_items,
                                                        const double *__restrict__ partial, double *__restrict__ area,
                                                        double *__restrict__ area_abs) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_items || !item_ordered(key, runmax, i)) return;
  const int32_t p = key[i];
  if (i > 0 && runmax[i - 1] >= p) return;   // not the head
  double s = 0.0, s_abs = 0.0;
  for (int64_t j = i; j < n_items && runmax[j] == p; ++j) {   // items that are not ordered, or were skipped, left zeros
    s += partial[j * 2];
    s_abs += partial[j * 2 + 1];
  }
  area[p] = s;
  area_abs[p] = s_abs;
}

int check_boxes(gr_ctx *c, const char *name, const int64_t *boxes_a, int64_t Pa, const int64_t *boxes_b, int64_t Pb) {
  if (Pa < 0 || Pb < 0 || Pa >= 0x7FFFFFFFll || Pb >= 0x7FFFFFFFll)
    return fail(c, GR_EINVAL, "%s: a row count is negative or not below 2^31 - 1 (Pa=%lld Pb=%lld)", name, (long long)Pa, (long long)Pb);
  if ((Pa > 0 && !boxes_a) || (Pb > 0 && !boxes_b)) return fail(c, GR_EINVAL, "%s: null arrays", name);
  return GR_OK;
}

}  // namespace

extern "C" {

int gr_polygon_box_pairs_count(gr_ctx *c, const int64_t *boxes_a, int64_t Pa, const int64_t *boxes_b, int64_t Pb, int64_t *offsets,
                               void *stream) {
  if (!c) return GR_EINVAL;
  int rc = check_boxes(c, "gr_polygon_box_pairs_count", boxes_a, Pa, boxes_b, Pb);
  if (rc != GR_OK) return rc;
  if (!offsets) return fail(c, GR_EINVAL, "gr_polygon_box_pairs_count: null arrays");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  // scratch: counts [Pa + 1] | the scan's temporaries
  Plan p;
  const auto counts = p.array<u64>(Pa + 1);
  const ExclusiveSum<u64> scan(c, p, Pa + 1);
  rc = stage_acquire(c, c->stage, p.finish(), s, "polygon-box-pairs");
  if (rc != GR_OK) return rc;
  p.base = c->stage.ptr;
  hipLaunchKernelGGL(k_overlap_pairs_count, dim3((unsigned)ceil_div(Pa + 1, 256)), dim3(256), 0, s, boxes_a, Pa, boxes_b, Pb, counts());
  GR_HIP(c, hipGetLastError());
  GR_TRY(scan.run(counts(), (u64 *)offsets, s));
  return GR_OK;
}

int gr_polygon_box_pairs_fill(gr_ctx *c, const int64_t *boxes_a, int64_t Pa, const int64_t *boxes_b, int64_t Pb, const int64_t *offsets,
                              int32_t *pairs, int64_t n_pairs, void *stream) {
  if (!c) return GR_EINVAL;
  int rc = check_boxes(c, "gr_polygon_box_pairs_fill", boxes_a, Pa, boxes_b, Pb);
  if (rc != GR_OK) return rc;
  if (n_pairs < 0 || n_pairs > 0x7FFFFFFFll) return fail(c, GR_EINVAL, "gr_polygon_box_pairs_fill: n_pairs=%lld is negative or not below 2^31", (long long)n_pairs);
  if (!offsets || (n_pairs > 0 && !pairs)) return fail(c, GR_EINVAL, "gr_polygon_box_pairs_fill: null arrays");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  if (Pa == 0 || n_pairs == 0) return GR_OK;
  hipLaunchKernelGGL(k_overlap_pairs_fill, dim3((unsigned)ceil_div(Pa, 256)), dim3(256), 0, s, boxes_a, Pa, boxes_b, Pb, offsets, pairs, n_pairs);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

int gr_polygon_overlap_areas(gr_ctx *c, const int64_t *ring_vertices_a, int64_t n_ring_vertices_a, const int64_t *ring_offsets_a,
                             const int32_t *ring_polygon_a, const int32_t *ring_is_hole_a, int64_t R_a, const int64_t *polygon_boxes_a,
                             int64_t P_a, const int64_t *ring_vertices_b, int64_t n_ring_vertices_b, const int64_t *ring_offsets_b,
                             const int32_t *ring_polygon_b, const int32_t *ring_is_hole_b, int64_t R_b, const int64_t *polygon_boxes_b,
                             int64_t P_b, const int32_t *pairs, int64_t n_pairs, const int32_t *items, int64_t n_items, double *area,
                             double *area_abs, uint64_t *stats, void *stream) {
  if (!c) return GR_EINVAL;
  GR_TRY(check_ring_table(c, "gr_polygon_overlap_areas", "a", ring_vertices_a, n_ring_vertices_a, ring_offsets_a, ring_polygon_a, ring_is_hole_a,
                          R_a, polygon_boxes_a, P_a, true));
  GR_TRY(check_ring_table(c, "gr_polygon_overlap_areas", "b", ring_vertices_b, n_ring_vertices_b, ring_offsets_b, ring_polygon_b, ring_is_hole_b,
                          R_b, polygon_boxes_b, P_b, true));
  if (n_pairs < 0 || n_items < 0 || n_pairs > 0x7FFFFFFFll || n_items > 0x7FFFFFFFll)
    return fail(c, GR_EINVAL, "gr_polygon_overlap_areas: n_pairs=%lld or n_items=%lld is negative or not below 2^31", (long long)n_pairs,
                (long long)n_items);
  if (!stats || (n_pairs > 0 && (!pairs || !area || !area_abs)) || (n_items > 0 && !items))
    return fail(c, GR_EINVAL, "gr_polygon_overlap_areas: null arrays");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  u64 *st = (u64 *)stats;
  GR_HIP(c, hipMemsetAsync(st, 0, sizeof(uint64_t) * GR_OVERLAP_STAT_WORDS, s));
  if (n_pairs > 0) {
    GR_HIP(c, hipMemsetAsync(area, 0, sizeof(double) * (size_t)n_pairs, s));
    GR_HIP(c, hipMemsetAsync(area_abs, 0, sizeof(double) * (size_t)n_pairs, s));
  }
  OverlapArgs g;
  g.a = RingTable{ring_vertices_a, ring_offsets_a, polygon_boxes_a, ring_polygon_a, ring_is_hole_a, n_ring_vertices_a, R_a, P_a};
  g.b = RingTable{ring_vertices_b, ring_offsets_b, polygon_boxes_b, ring_polygon_b, ring_is_hole_b, n_ring_vertices_b, R_b, P_b};
  g.n_pairs = n_pairs; g.n_items = n_items;
  hipLaunchKernelGGL(k_overlap_stat_pairs, dim3(1), dim3(64), 0, s, st, (u64)n_pairs);
  for (const RingTable *t : {&g.a, &g.b}) {
    const int64_t n = std::max(t->R, t->n_rv);
    if (n > 0) hipLaunchKernelGGL(k_overlap_table_stats, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, *t, st);
  }
  GR_HIP(c, hipGetLastError());
  if (n_items == 0) return GR_OK;
  // scratch: key [n_items] | runmax [n_items] | partial [n_items][2] | the scan's temporaries
  Plan p;
  const auto key = p.array<int32_t>(n_items), runmax = p.array<int32_t>(n_items);
  const auto partial = p.array<double>(2 * n_items);
  const InclusiveMax<int32_t> scan(c, p, n_items);
  GR_TRY(stage_acquire(c, c->stage, p.finish(), s, "polygon-overlap"));
  p.base = c->stage.ptr;
  const dim3 per_item((unsigned)ceil_div(n_items, 256));
  hipLaunchKernelGGL(k_overlap_item_keys, per_item, dim3(256), 0, s, items, n_items, n_pairs, key());
  GR_TRY(scan.run(key(), runmax(), s));
  hipLaunchKernelGGL(k_overlap_areas, dim3((unsigned)n_items), dim3(256), 0, s, g, pairs, items, (const int32_t *)key(),
                     (const int32_t *)runmax(), partial(), st);
  hipLaunchKernelGGL(k_overlap_reduce, per_item, dim3(256), 0, s, (const int32_t *)key(), (const int32_t *)runmax(), n_items,
                     (const double *)partial(), area, area_abs);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

}  // extern "C"
