// geograypher_amd/csrc/nearest.hip -- for every query point the row of the nearest reference point (gr_nearest_points; the rule-set
// is DESIGN.md section 8v, K1-K9).  Exact: the answer is the brute-force argmin of K2's float64 expression, the lowest row among
// equal distances, whatever the grid.  Needs no uploaded mesh; its scratch is the stage arena.
//
// Shape.  BOUNDS, once: k_nn_bounds folds the participating refs into six ordered keys (atomicMin / atomicMax of integers) and counts
// the others; the host reads them back and lays the grid: cells of side `cell`, at most 2^21 per axis, indices clipped into range.
// A LEVEL: k_nn_keys gives every participating ref the key cz << 42 | cy << 21 | cx of its cell and every other row a key behind
// all of them; one stable radix sort of (key, row) (cub_steps.hpp) keeps the rows of a cell ascending; k_nn_gather writes the
// coordinates and the row of every sorted entry side by side, 32 bytes, so the members of a cell are contiguous loads.  There is
// no cell table: the cells [x0, x1] of one (cy, cz) row are one contiguous key range, found by a lower-bound search in the sorted
// keys and walked until a key leaves it.  k_nn_query, a lane per query: it walks the shells k = 0, 1, ... max_rings of its clamped
// cell and compares (d2, row) lexicographically.  After shell k every ref it has not seen lies in a cell whose index differs by
// more than k on some axis, so on that axis -- and so in all -- it is at least k cell away, less the rounding of the cell
// assignment (an index is floor of TWO rounded operations on a value below 2^21: the point may be 2^-30 cell on the wrong side of a
// cell wall, on either end) and of K2 (a few 2^-53, relative): d2 >= (k cell)^2 (1 - 2^-28).  The query is SETTLED iff the shells
// covered the whole grid, or min(best d2, md2) < (k cell)^2 (1 - 2^-20): no unseen row can win, tie, or lie within md2.  A query
// that is not settled goes onto a list (one atomic per wave; the list's order cannot reach the results, every query is answered
// by one lane from the sorted arrays alone); the host reads the count and, while it is not zero, runs the list against a grid of
// four times the cell.  The extent is at most 2^21 cells, so level 11 at the latest has one cell, which shell 0 covers: at most 12
// levels, and no other fallback.  Every word of the arena that is read was written by the call first.  No index is used that
// was not checked against its array.
#include <cmath>

#include "cub_steps.hpp"
#include "geom_dev.hpp"
#include "gr_internal.hpp"

namespace {
using namespace grimpl;

typedef unsigned long long u64;

constexpr int NN_BLOCK = 256;
constexpr int NN_COUNT_GROUPS = 1024;        // workgroups of the kernels that count: one atomic per wave of the launch and word
constexpr int64_t NN_MAX = 0x7FFFFFFFll;     // R, Q < NN_MAX
constexpr int NN_AXIS_BITS = 21;
constexpr int32_t NN_AXIS_CELLS = 1 << NN_AXIS_BITS;
constexpr int NN_MAX_LEVELS = 12;            // cells grow fourfold: 2^21 cells are one cell at level 11
constexpr u64 NN_PARKED = 1ull << 63;        // behind every key of three 21-bit indices
constexpr int32_t NN_NO_ROW = 0x7FFFFFFF;    // above every row
constexpr double NN_MARGIN = 1.0 - 0x1p-20;  // K3: the shrink of the settle bound (the rounding it covers is below 2^-28)

enum {  // the call's control words in the arena
  CT_LO = 0,           // three ordered keys: the least coordinates of the participating refs
  CT_HI = 3,           // ... the greatest
  CT_REF_BAD = 6,
  CT_QUERY_BAD = 7,
  CT_NO_ANSWER = 8,
  CT_CARRIED = 9,      // queries the running level left unsettled
  CT_PROBES = 10,
  CT_CANDS = 11,
  CT_WORDS = 16
};

struct NnGrid {   // one level's grid
  double lo[3];
  double cell;
  int32_t n[3];
  int32_t pad;
};

struct NnPoint { double x, y, z; long long row; };   // a sorted entry: 32 bytes, one cell's members side by side

struct NnHost {   // what the host knows when the statistics are written
  u64 levels, carried, cell_bits;
};

// double -> key with key(a) < key(b) iff a < b for every pair of non-NaN doubles, and back (host)
__device__ __forceinline__ u64 key_of(double v) {
  const u64 b = (u64)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
inline double value_of(u64 k) {
  const u64 b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  double v;
  memcpy(&v, &b, sizeof(v));
  return v;
}

__device__ __forceinline__ bool finite3(double x, double y, double z) {   // x - x is 0 for a finite x, NaN otherwise
  return ((x - x) == 0.0) & ((y - y) == 0.0) & ((z - z) == 0.0);
}

// the cell of a coordinate on one axis, clipped into [0, n); a NaN quotient (an infinite extent) is cell 0
__device__ __forceinline__ int32_t cell_of(double v, double lo, double cell, int32_t n) {
  const double t = (v - lo) / cell;
  return t >= 0.0 ? (t < (double)n ? (int32_t)t : n - 1) : 0;
}

// K1: the bounds of the participating refs, the number of the others
__global__ __launch_bounds__(NN_BLOCK) void k_nn_bounds(const double *__restrict__ ref, int64_t R, u64 *ctl) {
  const int lane = (int)(threadIdx.x & 63);
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  uint32_t n_bad = 0;
  for (int64_t r = (int64_t)blockIdx.x * NN_BLOCK + threadIdx.x; r < R; r += (int64_t)gridDim.x * NN_BLOCK) {
    const double v[3] = {ref[3 * r], ref[3 * r + 1], ref[3 * r + 2]};
    if (!finite3(v[0], v[1], v[2])) { n_bad += 1u; continue; }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = v[a] < lo[a] ? v[a] : lo[a];
      hi[a] = v[a] > hi[a] ? v[a] : hi[a];
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double l = __shfl_xor(lo[a], off), h = __shfl_xor(hi[a], off);
      lo[a] = l < lo[a] ? l : lo[a];
      hi[a] = h > hi[a] ? h : hi[a];
    }
  }
  if (lane == 0 && lo[0] <= hi[0]) {   // the wave saw a participating row
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(ctl + CT_LO + a, key_of(lo[a]));
      atomicMax(ctl + CT_HI + a, key_of(hi[a]));
    }
  }
  stat_add_u32(ctl, CT_REF_BAD, n_bad, lane);
}

__global__ __launch_bounds__(NN_BLOCK) void k_nn_keys(const double *__restrict__ ref, int64_t R, NnGrid g, u64 *__restrict__ keys,
                                                     int32_t *__restrict__ vals) {
  const int64_t r = (int64_t)blockIdx.x * NN_BLOCK + threadIdx.x;
  if (r >= R) return;
  const double x = ref[3 * r], y = ref[3 * r + 1], z = ref[3 * r + 2];
  u64 key = NN_PARKED;
  if (finite3(x, y, z))
    key = ((u64)cell_of(z, g.lo[2], g.cell, g.n[2]) << (2 * NN_AXIS_BITS)) | ((u64)cell_of(y, g.lo[1], g.cell, g.n[1]) << NN_AXIS_BITS) |
          (u64)cell_of(x, g.lo[0], g.cell, g.n[0]);
  keys[r] = key;
  vals[r] = (int32_t)r;
}

// the first M sorted entries are the participating refs: srow[i] is a row in [0, R), it came from k_nn_keys
__global__ __launch_bounds__(NN_BLOCK) void k_nn_gather(const double *__restrict__ ref, const int32_t *__restrict__ srow, int64_t M,
                                                       NnPoint *__restrict__ pts) {
  const int64_t i = (int64_t)blockIdx.x * NN_BLOCK + threadIdx.x;
  if (i >= M) return;
  const int32_t r = srow[i];
  NnPoint p;
  p.x = ref[3 * (int64_t)r];
  p.y = ref[3 * (int64_t)r + 1];
  p.z = ref[3 * (int64_t)r + 2];
  p.row = r;
  pts[i] = p;
}

struct NnBest { double d2; int32_t row; };

// the refs of the cells [key_lo, key_hi] of one grid row: a lower bound, then the entries until a key leaves the range
__device__ __forceinline__ void scan_run(const u64 *__restrict__ skeys, const NnPoint *__restrict__ pts, int64_t M, u64 key_lo, u64 key_hi,
                                         double qx, double qy, double qz, NnBest &best, u64 &cands) {
  int64_t a = 0, b = M;
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    if (skeys[mid] < key_lo) a = mid + 1;
    else b = mid;
  }
  for (; a < M && skeys[a] <= key_hi; ++a) {
    const NnPoint p = pts[a];
    const double dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
    const double d2 = (dx * dx + dy * dy) + dz * dz;   // K2
    const int32_t row = (int32_t)p.row;
    if (d2 < best.d2 || (d2 == best.d2 && row < best.row)) { best.d2 = d2; best.row = row; }
    cands += 1;
  }
}

// K3.  n queries: those of `list`, or all of them (list null: the first level, which also answers the non-finite ones).
// A wave walks its queries 64 at a time, so that the ballot of the unsettled is over whole waves.
__global__ __launch_bounds__(NN_BLOCK) void k_nn_query(const double *__restrict__ query, const int32_t *__restrict__ list, int64_t n,
                                                      const u64 *__restrict__ skeys, const NnPoint *__restrict__ pts, int64_t M, NnGrid g,
                                                      double md2, int max_rings, int32_t *__restrict__ index_out,
                                                      double *__restrict__ dist2_out, int32_t *__restrict__ next_list, u64 *ctl) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t wave = (int64_t)blockIdx.x * (NN_BLOCK / 64) + (int64_t)(threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * (NN_BLOCK / 64);
  u64 probes = 0, cands = 0;
  uint32_t n_bad = 0, n_none = 0;
  for (int64_t base = wave * 64; base < n; base += n_waves * 64) {   // uniform over the wave
    const int64_t t = base + lane;
    bool carried = false;
    int32_t q = -1;
    if (t < n) {
      q = list ? list[t] : (int32_t)t;
      const double qx = query[3 * (int64_t)q], qy = query[3 * (int64_t)q + 1], qz = query[3 * (int64_t)q + 2];
      NnBest best = {INFINITY, NN_NO_ROW};
      bool settled = false, finite = finite3(qx, qy, qz);
      if (finite) {
        const int32_t cx = cell_of(qx, g.lo[0], g.cell, g.n[0]), cy = cell_of(qy, g.lo[1], g.cell, g.n[1]),
                      cz = cell_of(qz, g.lo[2], g.cell, g.n[2]);
        for (int k = 0; k <= max_rings && !settled; ++k) {
          for (int dz = -k; dz <= k; ++dz) {
            const int32_t z = cz + dz;
            if (z < 0 || z >= g.n[2]) continue;
            for (int dy = -k; dy <= k; ++dy) {
              const int32_t y = cy + dy;
              if (y < 0 || y >= g.n[1]) continue;
              const u64 row_key = ((u64)z << (2 * NN_AXIS_BITS)) | ((u64)y << NN_AXIS_BITS);
              const bool whole = dz == -k || dz == k || dy == -k || dy == k;   // a row of the shell's faces: all its x; else its two ends
              if (whole) {
                const int32_t x0 = cx - k < 0 ? 0 : cx - k, x1 = cx + k > g.n[0] - 1 ? g.n[0] - 1 : cx + k;
                scan_run(skeys, pts, M, row_key | (u64)x0, row_key | (u64)x1, qx, qy, qz, best, cands);
                probes += 1;
              } else {
                if (cx - k >= 0) {
                  scan_run(skeys, pts, M, row_key | (u64)(cx - k), row_key | (u64)(cx - k), qx, qy, qz, best, cands);
                  probes += 1;
                }
                if (cx + k <= g.n[0] - 1) {
                  scan_run(skeys, pts, M, row_key | (u64)(cx + k), row_key | (u64)(cx + k), qx, qy, qz, best, cands);
                  probes += 1;
                }
              }
            }
          }
          const bool covered = cx - k <= 0 && cx + k >= g.n[0] - 1 && cy - k <= 0 && cy + k >= g.n[1] - 1 && cz - k <= 0 && cz + k >= g.n[2] - 1;
          if (covered) settled = true;
          else if (k >= 1) {
            const double reach = (double)k * g.cell;
            const double bound = (reach * reach) * NN_MARGIN;
            settled = (best.d2 < md2 ? best.d2 : md2) < bound;
          }
        }
      }
      if (!finite || settled) {
        const bool keep = finite && best.row != NN_NO_ROW && best.d2 <= md2;   // K4
        index_out[q] = keep ? best.row : -1;
        if (dist2_out) dist2_out[q] = keep ? best.d2 : NAN;
        n_bad += finite ? 0u : 1u;
        n_none += keep ? 0u : 1u;
      } else carried = true;
    }
    const u64 who = __ballot(carried);
    if (who) {
      u64 at = 0;
      if (lane == 0) at = atomicAdd(ctl + CT_CARRIED, (u64)__popcll(who));
      at = (u64)__shfl((long long)at, 0);
      // (at most n <= Q entries in all: every query is carried at most once per level)
      if (carried) next_list[at + (u64)__popcll(who & ((1ull << lane) - 1ull))] = q;
    }
  }
  stat_add(ctl, CT_PROBES, probes, lane);
  stat_add(ctl, CT_CANDS, cands, lane);
  stat_add_u32(ctl, CT_QUERY_BAD, n_bad, lane);
  stat_add_u32(ctl, CT_NO_ANSWER, n_none, lane);
}

// K5: no participating ref
__global__ __launch_bounds__(NN_BLOCK) void k_nn_none(const double *__restrict__ query, int64_t Q, int32_t *__restrict__ index_out,
                                                     double *__restrict__ dist2_out, u64 *ctl) {
  uint32_t n_bad = 0, n_none = 0;
  for (int64_t q = (int64_t)blockIdx.x * NN_BLOCK + threadIdx.x; q < Q; q += (int64_t)gridDim.x * NN_BLOCK) {
    n_bad += finite3(query[3 * q], query[3 * q + 1], query[3 * q + 2]) ? 0u : 1u;
    n_none += 1u;
    index_out[q] = -1;
    if (dist2_out) dist2_out[q] = NAN;
  }
  stat_add_u32(ctl, CT_QUERY_BAD, n_bad, (int)(threadIdx.x & 63));
  stat_add_u32(ctl, CT_NO_ANSWER, n_none, (int)(threadIdx.x & 63));
}

// K6, K7: every word of the statistics block
__global__ void k_nn_stats(const u64 *__restrict__ ctl, NnHost h, u64 *__restrict__ stats) {
  const int w = (int)threadIdx.x;
  if (w >= GR_NN_STAT_WORDS) return;
  u64 v = 0;
  switch (w) {
    case GR_NN_STAT_REF_NONFINITE: v = ctl[CT_REF_BAD]; break;
    case GR_NN_STAT_QUERY_NONFINITE: v = ctl[CT_QUERY_BAD]; break;
    case GR_NN_STAT_NO_ANSWER: v = ctl[CT_NO_ANSWER]; break;
    case GR_NN_STAT_LEVELS: v = h.levels; break;
    case GR_NN_STAT_CARRIED: v = h.carried; break;
    case GR_NN_STAT_CELLS_PROBED: v = ctl[CT_PROBES]; break;
    case GR_NN_STAT_CANDIDATES: v = ctl[CT_CANDS]; break;
    case GR_NN_STAT_CELL_BITS: v = h.cell_bits; break;
    case GR_NN_STAT_RING_CAP: v = h.carried ? 1 : 0; break;
    default: break;
  }
  stats[w] = v;
}

inline unsigned grid_of(int64_t n) { return (unsigned)ceil_div(n > 0 ? n : 1, NN_BLOCK); }
inline unsigned count_grid_of(int64_t n) { return std::min(grid_of(n), (unsigned)NN_COUNT_GROUPS); }

inline bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && na && nb && a0 < b0 + nb && b0 < a0 + na;
}

// K8: the cell of the first level.  e: the extents of the participating refs, M > 0 their number.
double first_cell(const double e[3], int64_t M, double given) {
  double s[3] = {e[0], e[1], e[2]};
  std::sort(s, s + 3);
  const double e1 = s[2], e2 = s[1];
  double cell;
  if (given > 0) cell = std::max(given, e1 / (double)NN_AXIS_CELLS);
  else {
    if (e1 == 0) cell = 1.0;
    else if (e2 == 0) cell = e1 / (double)M;
    else cell = 1.5 * std::sqrt(e1 * e2 / (double)M);
    cell = std::max(cell, e1 / (double)(NN_AXIS_CELLS / 2));
  }
  if (!(cell > 0)) cell = e1 > 0 ? e1 : 1.0;   // (an extent so small that its 2^-21 is 0)
  return cell;
}

void level_grid(const double lo[3], const double e[3], double cell, bool one_cell, NnGrid &g) {
  g.cell = cell;
  g.pad = 0;
  for (int a = 0; a < 3; ++a) {
    g.lo[a] = lo[a];
    const double t = e[a] / cell;   // the index of the greatest coordinate, as cell_of computes it
    int32_t n = 1;
    if (t >= (double)NN_AXIS_CELLS) n = NN_AXIS_CELLS;
    else if (t >= 0) n = std::min((int32_t)t + 1, NN_AXIS_CELLS);
    g.n[a] = one_cell ? 1 : n;
  }
}

}  // namespace

extern "C" {

int gr_nearest_points(gr_ctx *c, const gr_nearest_args *args_h) {
  if (!c) return GR_EINVAL;
  if (!args_h) return fail(c, GR_EINVAL, "gr_nearest_points: null descriptor");
  const gr_nearest_args g = *args_h;   // read once, here
  const int64_t R = g.R, Q = g.Q;
  if (R < 0 || Q < 0 || R >= NN_MAX || Q >= NN_MAX)
    return fail(c, GR_EINVAL, "gr_nearest_points: R=%lld, Q=%lld: each in [0, 2^31 - 1)", (long long)R, (long long)Q);
  if (!(g.cell >= 0) || std::isinf(g.cell)) return fail(c, GR_EINVAL, "gr_nearest_points: cell=%g: a finite size >= 0 (0: chosen by the call)", g.cell);
  if (!(g.max_distance >= 0)) return fail(c, GR_EINVAL, "gr_nearest_points: max_distance=%g: >= 0, +inf for none", g.max_distance);
  if (g.max_rings < 1) return fail(c, GR_EINVAL, "gr_nearest_points: max_rings=%d: >= 1", (int)g.max_rings);
  if (!g.stats || (R > 0 && !g.ref) || (Q > 0 && (!g.query || !g.index_out))) return fail(c, GR_EINVAL, "gr_nearest_points: null arrays");
  const struct { const void *p; size_t n; const char *name; } ins[] = {{g.ref, 24 * (size_t)R, "ref"}, {g.query, 24 * (size_t)Q, "query"}};
  const struct { const void *p; size_t n; const char *name; } outs[] = {{g.index_out, sizeof(int32_t) * (size_t)Q, "index_out"},
                                                                        {g.dist2_out, sizeof(double) * (size_t)Q, "dist2_out"},
                                                                        {g.stats, sizeof(uint64_t) * GR_NN_STAT_WORDS, "stats"}};
  for (const auto &o : outs) {
    for (const auto &i : ins)
      if (overlaps(o.p, o.n, i.p, i.n)) return fail(c, GR_EINVAL, "gr_nearest_points: %s overlaps %s", o.name, i.name);
    for (const auto &q : outs)
      if (&q != &o && overlaps(o.p, o.n, q.p, q.n)) return fail(c, GR_EINVAL, "gr_nearest_points: %s overlaps %s", o.name, q.name);
  }
  hipStream_t s = (hipStream_t)g.stream;
  GR_HIP(c, hipSetDevice(c->device));

  const bool search = R > 0 && Q > 0;
  const int64_t Rs = search ? R : 0, Qs = search ? Q : 0;   // nothing but the control words without a search
  Plan p;
  const auto o_ctl = p.array<u64>(CT_WORDS);
  const auto o_list_a = p.array<int32_t>(Qs), o_list_b = p.array<int32_t>(Qs);
  const auto o_skeys = p.array<u64>(Rs);
  const auto o_srow = p.array<int32_t>(Rs);
  const size_t mark = p.mark();   // the unsorted keys are dead once sorted: the sorted entries lie over them
  const auto o_keys = p.array<u64>(Rs);
  const auto o_vals = p.array<int32_t>(Rs);
  p.rewind(mark);
  const auto o_pts = p.array<NnPoint>(Rs);
  const SortPairs<u64, int32_t> sort(c, p, Rs, 64);
  GR_TRY(stage_acquire(c, c->stage, p.finish(), s, "nearest-points"));
  p.base = c->stage.ptr;
  u64 *ctl = o_ctl();
  const dim3 block(NN_BLOCK);
  const double md2 = g.max_distance * g.max_distance;   // K4
  const int max_rings = g.max_rings > NN_AXIS_CELLS ? NN_AXIS_CELLS : g.max_rings;   // more rings than cells cover every grid

  GR_HIP(c, hipMemsetAsync(ctl, 0, sizeof(u64) * CT_WORDS, s));
  GR_HIP(c, hipMemsetAsync(ctl + CT_LO, 0xFF, sizeof(u64) * 3, s));
  NnHost h = {0, 0, 0};
  if (R > 0) {
    hipLaunchKernelGGL(k_nn_bounds, dim3(count_grid_of(R)), block, 0, s, g.ref, R, ctl);
    GR_HIP(c, hipGetLastError());
  }
  int64_t M = 0;
  u64 head[CT_REF_BAD + 1] = {0};
  if (search) {
    GR_HIP(c, hipMemcpyAsync(head, ctl, sizeof(head), hipMemcpyDeviceToHost, s));
    GR_HIP(c, hipStreamSynchronize(s));   // the wait for the bounds
    M = R - (int64_t)head[CT_REF_BAD];
  }
  if (M <= 0) {
    if (Q > 0) {
      hipLaunchKernelGGL(k_nn_none, dim3(count_grid_of(Q)), block, 0, s, g.query, Q, g.index_out, g.dist2_out, ctl);
      GR_HIP(c, hipGetLastError());
    }
  } else {
    double lo[3], e[3];
    for (int a = 0; a < 3; ++a) {
      lo[a] = value_of(head[CT_LO + a]);
      e[a] = value_of(head[CT_HI + a]) - lo[a];
    }
    double cell = first_cell(e, M, g.cell);
    memcpy(&h.cell_bits, &cell, sizeof(cell));
    int32_t *list = nullptr, *next = o_list_a();
    int64_t n = Q;
    for (int level = 0;; ++level) {
      NnGrid grid;
      level_grid(lo, e, cell, level + 1 >= NN_MAX_LEVELS, grid);
      hipLaunchKernelGGL(k_nn_keys, dim3(grid_of(R)), block, 0, s, g.ref, R, grid, o_keys(), o_vals());
      GR_HIP(c, hipGetLastError());
      GR_TRY(sort.run(o_keys(), o_skeys(), o_vals(), o_srow(), s));
      hipLaunchKernelGGL(k_nn_gather, dim3(grid_of(M)), block, 0, s, g.ref, (const int32_t *)o_srow(), M, o_pts());
      GR_HIP(c, hipMemsetAsync(ctl + CT_CARRIED, 0, sizeof(u64), s));
      hipLaunchKernelGGL(k_nn_query, dim3(grid_of(n)), block, 0, s, g.query, (const int32_t *)list, n, (const u64 *)o_skeys(),
                         (const NnPoint *)o_pts(), M, grid, md2, max_rings, g.index_out, g.dist2_out, next, ctl);
      GR_HIP(c, hipGetLastError());
      u64 carried = 0;
      GR_HIP(c, hipMemcpyAsync(&carried, ctl + CT_CARRIED, sizeof(carried), hipMemcpyDeviceToHost, s));
      GR_HIP(c, hipStreamSynchronize(s));   // the one wait of a level
      h.levels += 1;
      if (carried == 0) break;
      if (level + 1 >= NN_MAX_LEVELS || (int64_t)carried > n)
        return fail(c, GR_EHIP, "gr_nearest_points: %llu of %lld queries unsettled at level %d", carried, (long long)n, level);
      h.carried += carried;
      n = (int64_t)carried;
      list = next;
      next = list == o_list_a() ? o_list_b() : o_list_a();
      cell *= 4.0;
    }
  }
  hipLaunchKernelGGL(k_nn_stats, dim3(1), dim3(64), 0, s, (const u64 *)ctl, h, (u64 *)g.stats);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

}  // extern "C"
