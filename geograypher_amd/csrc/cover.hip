// geograypher_amd/csrc/cover.hip -- the covering meshes of the multiview-detection workflow (export_covering_meshes): the bounds
// of a point set (gr_points_bounds) and, per cell of an N x N grid over them, the highest and the lowest member and the number
// of members (gr_cover_grid; the rule is DESIGN.md "Covering meshes").  Needs no uploaded mesh.  Everything is float64; nothing
// here rounds: minima, maxima and counts are exact in any order.
//
// Membership is decided by the caller's four bound tables alone (cell i of an axis holds x iff lo[i] <= x <= hi[i]), staged in
// LDS.  A workgroup first looks at the tables: when both are non-decreasing and cells two apart are disjoint (lo[i + 2] > hi[i]
// for every i) a coordinate belongs to at most two cells, neighbours, and a lane finds them from an arithmetic estimate that it
// then corrects by walking the table -- to f, the first cell with hi[f] >= x -- and confirms cell f and cell f + 1 by the two
// comparisons.  The estimate only decides how far the walk goes, never the result.  Any other table (an axis of zero extent:
// all cells equal; an extent of a few ulps; a NaN) takes the all-columns path: every cell is compared.
//
// Accumulators: order-preserving 64-bit keys of the doubles, so that unsigned integer max / min atomics do the work.
//   N <= GR_COVER_LDS_N (56)  per workgroup in LDS, 20 bytes a cell; with the tables 4 * 8 * 56 + 20 * 56^2 = 64 512 bytes of dynamic
//                              LDS beside 256 static ones: the largest N under the 64 KiB a workgroup gets without asking for
//                              more (N = 57 needs 66 804).  N = 50, the entry point's: 51 600 bytes, three workgroups of 512
//                              lanes on the 160 KiB of a gfx950 CU, 24 waves.  Flushed once per workgroup, the cells that
//                              have members only, with global atomics.
//   N above                    global atomics directly; LDS holds the tables alone (32 KiB at N = 1024).
// The global accumulators ARE the outputs: z_max / z_min hold keys between k_cover_init and k_cover_finish, which decodes them
// in place (NaN where count is 0).
#include "gr_internal.hpp"

using namespace grimpl;

#define GR_COVER_MAX_N 1024
#define GR_COVER_LDS_N 56          // largest N whose accumulators live in LDS (header comment)
#define GR_COVER_BLOCK 512         // lanes of a k_cover_grid workgroup
#define GR_COVER_ROWS_PER_LANE 8   // rows a lane takes at least before another workgroup is launched: a workgroup's flush (up to
                                   // 3 N^2 global atomics) is shared by at least 4096 rows
#define GR_COVER_MAX_GRID 1024
#define GR_BOUNDS_BLOCK 256
#define GR_BOUNDS_ROWS_PER_LANE 4
#define GR_BOUNDS_MAX_GRID 1024    // partial records of k_points_bounds (context scratch, 64 bytes each)

namespace {

typedef unsigned long long u64;

// double -> key with key(a) < key(b) iff a < b for every pair of non-NaN doubles (-0.0 below +0.0), and back
__device__ __forceinline__ u64 key_of(double v) {
  const u64 b = (u64)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(u64 k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}
#define GR_KEY_MAX_INIT 0ull    // below the key of every double that is not a NaN
#define GR_KEY_MIN_INIT (~0ull) // above ...

__device__ __forceinline__ bool finite3(double x, double y, double z) {
  // x - x is 0 for a finite x and NaN for an infinite or NaN one
  return ((x - x) == 0.0) & ((y - y) == 0.0) & ((z - z) == 0.0);
}

struct BoundsPart { double lo[3], hi[3]; u64 bad; u64 pad; };   // 64 bytes

__device__ __forceinline__ void wave_reduce_bounds(double (&lo)[3], double (&hi)[3], u64 &bad) {
  for (int off = 32; off > 0; off >>= 1) {
    for (int a = 0; a < 3; ++a) {
      const double l = __shfl_xor(lo[a], off), h = __shfl_xor(hi[a], off);
      lo[a] = l < lo[a] ? l : lo[a];
      hi[a] = h > hi[a] ? h : hi[a];
    }
    bad += (u64)__shfl_xor((long long)bad, off);
  }
}

// rows 0, stride, 2 stride, ... (n of them): per lane, per wave (shuffles), per workgroup (LDS) -> one BoundsPart per workgroup.
// A row with a NaN or infinite coordinate is counted and takes no part in the bounds.
__global__ void __launch_bounds__(GR_BOUNDS_BLOCK) k_points_bounds(const double *__restrict__ points, int64_t n, int64_t stride,
                                                                   BoundsPart *__restrict__ part) {
  __shared__ BoundsPart wave_part[GR_BOUNDS_BLOCK / 64];
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  u64 bad = 0;
  for (int64_t r = (int64_t)blockIdx.x * GR_BOUNDS_BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * GR_BOUNDS_BLOCK) {
    const double *p = points + 3 * (r * stride);
    const double v[3] = {p[0], p[1], p[2]};
    if (!finite3(v[0], v[1], v[2])) { ++bad; continue; }
    for (int a = 0; a < 3; ++a) {
      lo[a] = v[a] < lo[a] ? v[a] : lo[a];
      hi[a] = v[a] > hi[a] ? v[a] : hi[a];
    }
  }
  wave_reduce_bounds(lo, hi, bad);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    for (int a = 0; a < 3; ++a) { wave_part[wave].lo[a] = lo[a]; wave_part[wave].hi[a] = hi[a]; }
    wave_part[wave].bad = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    BoundsPart out = wave_part[0];
    for (int w = 1; w < GR_BOUNDS_BLOCK / 64; ++w) {
      for (int a = 0; a < 3; ++a) {
        out.lo[a] = wave_part[w].lo[a] < out.lo[a] ? wave_part[w].lo[a] : out.lo[a];
        out.hi[a] = wave_part[w].hi[a] > out.hi[a] ? wave_part[w].hi[a] : out.hi[a];
      }
      out.bad += wave_part[w].bad;
    }
    out.pad = 0;
    part[blockIdx.x] = out;
  }
}

// the combine: one wave over the n_part partial records
__global__ void __launch_bounds__(64) k_points_bounds_combine(const BoundsPart *__restrict__ part, int n_part,
                                                              double *__restrict__ bounds6, u64 *__restrict__ nonfinite) {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  u64 bad = 0;
  for (int k = threadIdx.x; k < n_part; k += 64) {
    const BoundsPart p = part[k];
    for (int a = 0; a < 3; ++a) {
      lo[a] = p.lo[a] < lo[a] ? p.lo[a] : lo[a];
      hi[a] = p.hi[a] > hi[a] ? p.hi[a] : hi[a];
    }
    bad += p.bad;
  }
  wave_reduce_bounds(lo, hi, bad);
  if (threadIdx.x == 0) {
    for (int a = 0; a < 3; ++a) { bounds6[2 * a] = lo[a]; bounds6[2 * a + 1] = hi[a]; }
    *nonfinite = bad;
  }
}

__global__ void __launch_bounds__(256) k_cover_init(u64 *__restrict__ kmax, u64 *__restrict__ kmin, uint32_t *__restrict__ count,
                                                    int cells) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  kmax[c] = GR_KEY_MAX_INIT; kmin[c] = GR_KEY_MIN_INIT; count[c] = 0;
}

__global__ void __launch_bounds__(256) k_cover_finish(u64 *__restrict__ kmax, u64 *__restrict__ kmin,
                                                      const uint32_t *__restrict__ count, int cells) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  const bool any = count[c] != 0;
  const double hi = any ? value_of(kmax[c]) : NAN, lo = any ? value_of(kmin[c]) : NAN;
  kmax[c] = (u64)__double_as_longlong(hi);   // the caller reads these words as doubles
  kmin[c] = (u64)__double_as_longlong(lo);
}

// The cells of one axis that hold v: up to two on a table that separates its cells (`walk`), found from the estimate `est` by
// walking to f = the first cell with hi[f] >= v and comparing cells f and f + 1; returns how many (0, 1 or 2), the first in
// `first`.  (lo and hi non-decreasing and lo[i + 2] > hi[i]: no cell below f holds v, since hi is below it, and none above
// f + 1, since lo[f + 2] > hi[f] >= v.)
__device__ __forceinline__ int axis_cells(const double *lo, const double *hi, int N, double v, int est, int &first) {
  int f = est < 0 ? 0 : (est > N - 1 ? N - 1 : est);
  while (f > 0 && hi[f - 1] >= v) --f;
  while (f < N && !(hi[f] >= v)) ++f;
  if (f >= N) return 0;
  const bool in0 = lo[f] <= v;                                  // hi[f] >= v holds
  const bool in1 = f + 1 < N && lo[f + 1] <= v && v <= hi[f + 1];
  first = in0 ? f : f + 1;
  return (int)in0 + (int)in1;
}

// One lane per visited row, a grid-stride loop.  LDS: lo_x | hi_x | lo_y | hi_y (N doubles each), then for LDS_ACC the key of the
// maximum, the key of the minimum (N^2 u64 each) and the member count (N^2 u32).
template <bool LDS_ACC>
__global__ void __launch_bounds__(GR_COVER_BLOCK) k_cover_grid(const double *__restrict__ points, int64_t n, int64_t stride, int N,
                                                              const double *__restrict__ x_lo, const double *__restrict__ x_hi,
                                                              const double *__restrict__ y_lo, const double *__restrict__ y_hi,
                                                              u64 *__restrict__ gmax, u64 *__restrict__ gmin,
                                                              uint32_t *__restrict__ gcount) {
  extern __shared__ double lds[];
  double *lo_x = lds, *hi_x = lds + N, *lo_y = lds + 2 * N, *hi_y = lds + 3 * N;
  u64 *amax = (u64 *)(lds + 4 * N), *amin = amax + N * N;
  uint32_t *acnt = (uint32_t *)(amin + N * N);
  const int tid = threadIdx.x, cells = N * N;
  for (int i = tid; i < N; i += GR_COVER_BLOCK) { lo_x[i] = x_lo[i]; hi_x[i] = x_hi[i]; lo_y[i] = y_lo[i]; hi_y[i] = y_hi[i]; }
  if (LDS_ACC)
    for (int c = tid; c < cells; c += GR_COVER_BLOCK) { amax[c] = GR_KEY_MAX_INIT; amin[c] = GR_KEY_MIN_INIT; acnt[c] = 0; }
  __syncthreads();
  // does the table of an axis separate its cells?  (every comparison is false for a NaN: such a table does not)
  int bad_x = 0, bad_y = 0;
  for (int i = tid; i < N; i += GR_COVER_BLOCK) {
    if (i + 1 < N) {
      bad_x |= !(lo_x[i] <= lo_x[i + 1]) | !(hi_x[i] <= hi_x[i + 1]);
      bad_y |= !(lo_y[i] <= lo_y[i + 1]) | !(hi_y[i] <= hi_y[i + 1]);
    }
    if (i + 2 < N) { bad_x |= !(lo_x[i + 2] > hi_x[i]); bad_y |= !(lo_y[i + 2] > hi_y[i]); }
    bad_x |= !(lo_x[i] <= hi_x[i]); bad_y |= !(lo_y[i] <= hi_y[i]);
  }
  const bool walk_x = __syncthreads_or(bad_x) == 0, walk_y = __syncthreads_or(bad_y) == 0;
  // estimate: cell = (v - lo[0]) / (lo[N - 1] - lo[0]) * (N - 1), the spacing of the cells' lower bounds
  const double x0 = lo_x[0], y0 = lo_y[0];
  const double sx = (double)(N - 1) / (lo_x[N - 1] - x0), sy = (double)(N - 1) / (lo_y[N - 1] - y0);

  for (int64_t r = (int64_t)blockIdx.x * GR_COVER_BLOCK + tid; r < n; r += (int64_t)gridDim.x * GR_COVER_BLOCK) {
    const double *p = points + 3 * (r * stride);
    const double x = p[0], y = p[1], z = p[2];
    if (!finite3(x, y, z)) continue;
    const u64 kz = key_of(z);
    int fx = 0, nx = N, fy = 0, ny = N;   // all-columns path: every cell is a candidate
    if (walk_x) {
      const double e = (x - x0) * sx;
      nx = axis_cells(lo_x, hi_x, N, x, (e >= 0.0 && e < (double)N) ? (int)e : (e >= 0.0 ? N - 1 : 0), fx);
    }
    if (walk_y) {
      const double e = (y - y0) * sy;
      ny = axis_cells(lo_y, hi_y, N, y, (e >= 0.0 && e < (double)N) ? (int)e : (e >= 0.0 ? N - 1 : 0), fy);
    }
    for (int i = fx; i < fx + nx; ++i) {
      if (!(lo_x[i] <= x && x <= hi_x[i])) continue;
      for (int j = fy; j < fy + ny; ++j) {
        if (!(lo_y[j] <= y && y <= hi_y[j])) continue;
        const int c = i * N + j;
        if (LDS_ACC) { atomicMax(&amax[c], kz); atomicMin(&amin[c], kz); atomicAdd(&acnt[c], 1u); }
        else { atomicMax(&gmax[c], kz); atomicMin(&gmin[c], kz); atomicAdd(&gcount[c], 1u); }
      }
    }
  }
  if (!LDS_ACC) return;
  __syncthreads();
  for (int c = tid; c < cells; c += GR_COVER_BLOCK) {
    const uint32_t m = acnt[c];
    if (m == 0) continue;
    atomicMax(&gmax[c], amax[c]); atomicMin(&gmin[c], amin[c]); atomicAdd(&gcount[c], m);
  }
}

}  // namespace

extern "C" {

int gr_points_bounds(gr_ctx *c, const double *points, int64_t V, int64_t stride, double *bounds6, uint64_t *nonfinite,
                     void *stream) {
  if (!c) return GR_EINVAL;
  if (V <= 0 || stride < 1 || !points || !bounds6 || !nonfinite)
    return fail(c, GR_EINVAL, "bad point-bounds args (V=%lld, stride=%lld)", (long long)V, (long long)stride);
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  const int64_t n = ceil_div(V, stride);
  const int grid = (int)std::min<int64_t>(ceil_div(n, GR_BOUNDS_BLOCK * GR_BOUNDS_ROWS_PER_LANE), GR_BOUNDS_MAX_GRID);
  // scratch: part [GR_BOUNDS_MAX_GRID]
  Carve cv;
  const auto o_part = cv.array<BoundsPart>(GR_BOUNDS_MAX_GRID);
  int rc = stage_acquire(c, c->stage, cv.total(), s, "point-bounds");
  if (rc != GR_OK) return rc;
  cv.base = c->stage.ptr;
  BoundsPart *part = o_part();
  hipLaunchKernelGGL(k_points_bounds, dim3((unsigned)grid), dim3(GR_BOUNDS_BLOCK), 0, s, points, n, stride, part);
  hipLaunchKernelGGL(k_points_bounds_combine, dim3(1), dim3(64), 0, s, (const BoundsPart *)part, grid, bounds6,
                     (u64 *)nonfinite);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

int gr_cover_grid(gr_ctx *c, const double *points, int64_t V, int64_t stride, int N, const double *x_lo, const double *x_hi,
                  const double *y_lo, const double *y_hi, double *z_max, double *z_min, uint32_t *count, void *stream) {
  if (!c) return GR_EINVAL;
  if (N < 2 || N > GR_COVER_MAX_N) return fail(c, GR_EINVAL, "N=%d: gr_cover_grid takes 2 <= N <= %d", N, GR_COVER_MAX_N);
  if (V <= 0 || stride < 1) return fail(c, GR_EINVAL, "bad cover-grid args (V=%lld, stride=%lld)", (long long)V, (long long)stride);
  if (!points || !x_lo || !x_hi || !y_lo || !y_hi || !z_max || !z_min || !count) return fail(c, GR_EINVAL, "null cover-grid arrays");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  const int64_t n = ceil_div(V, stride);
  const int cells = N * N;
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n, GR_COVER_BLOCK * GR_COVER_ROWS_PER_LANE), GR_COVER_MAX_GRID);
  u64 *kmax = (u64 *)z_max, *kmin = (u64 *)z_min;
  hipLaunchKernelGGL(k_cover_init, dim3((unsigned)ceil_div(cells, 256)), dim3(256), 0, s, kmax, kmin, count, cells);
  if (N <= GR_COVER_LDS_N)
    hipLaunchKernelGGL(k_cover_grid<true>, dim3(grid), dim3(GR_COVER_BLOCK), (size_t)(32 * N + 20 * cells), s, points, n, stride, N,
                       x_lo, x_hi, y_lo, y_hi, kmax, kmin, count);
  else
    hipLaunchKernelGGL(k_cover_grid<false>, dim3(grid), dim3(GR_COVER_BLOCK), (size_t)(32 * N), s, points, n, stride, N, x_lo, x_hi,
                       y_lo, y_hi, kmax, kmin, count);
  hipLaunchKernelGGL(k_cover_finish, dim3((unsigned)ceil_div(cells, 256)), dim3(256), 0, s, kmax, kmin,
                     (const uint32_t *)count, cells);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

}  // extern "C"
