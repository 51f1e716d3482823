// geograypher_amd/csrc/rays.hip -- the multiview-detection workflow's device side: the ray-pair graph (clamped segment-to-segment
// distance of every pair of rays from different images, kept when within a threshold) and the clip of rays against a small
// boundary mesh.  Needs no uploaded mesh.  Everything is float64 and, like the rest of the library, compiled without
// contraction: the exact `denom == 0` test for parallel rays relies on a1 * b2 - a2 * b1 of two identical directions being
// exactly zero, which a fused multiply-add would break.
#include "cub_steps.hpp"
#include "gr_internal.hpp"
#include "dev_common.hpp"
#include "ray_dev.hpp"

using namespace grimpl;

#define GR_RAY_TILE 256            // rays per side of a tile = threads of a workgroup (4 waves)
#define GR_RAY_MAX_N (1 << 23)     // rays per call: 32768 tiles a side, 536 887 296 tiles of the upper triangle
#define GR_RAY_MAX_GRID (1 << 20)  // workgroups of k_ray_pairs: beyond that many tiles a workgroup strides over several (2^28 threads a launch)
#define GR_CLIP_CHUNK 128          // triangles staged in LDS at a time by k_rays_clip
#define GR_CLIP_MAX_TRIANGLES 65536

namespace {

// Tile (row, col), row <= col, of linear index k in the row-major upper triangle of a T x T grid of tiles.  Row r starts at
// off(r) = r T - r (r - 1) / 2.  The double-precision estimate is corrected with 64-bit integers, so the decode is exact for every T
// the ray limit allows ((2 T + 1)^2 < 2^53, off < 2^63).
__host__ __device__ inline int64_t tri_off(int64_t r, int64_t T) { return r * T - r * (r - 1) / 2; }
__host__ __device__ inline void tri_decode(int64_t k, int64_t T, int64_t &row, int64_t &col) {
  const double b = 2.0 * (double)T + 1.0;
  int64_t r = (int64_t)((b - sqrt(b * b - 8.0 * (double)k)) * 0.5);
  if (r < 0) r = 0;
  if (r > T - 1) r = T - 1;
  while (r + 1 < T && tri_off(r + 1, T) <= k) ++r;
  while (r > 0 && tri_off(r, T) > k) --r;
  row = r;
  col = r + (k - tri_off(r, T));
}

__global__ void __launch_bounds__(256) k_ray_prep(const double *__restrict__ starts, const double *__restrict__ ends,
                                                  const int32_t *__restrict__ ids, int64_t n, RayRec *__restrict__ rec) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const RayRec r = ray_record(starts, ends, i, ids[i]);
  rec[i] = r;
}

// One workgroup per tile of the upper triangle (1-D grid, tri_decode; a grid-stride loop over the tiles once there are more than
// GR_RAY_MAX_GRID of them).  The B side of the tile is staged in LDS; every lane
// keeps one A ray in registers and walks the B rays -- all lanes read the same LDS address, a broadcast.  Hits (i < j, different
// image, d <= threshold; a NaN d never is) are compacted per wave: one ballot, one atomic of the wave's leader on the edge
// counter, one 64-bit key (i << 32 | j) and one distance per hit lane.  FILL false: the count alone (one atomic per wave).
template <bool FILL>
__global__ void __launch_bounds__(GR_RAY_TILE) k_ray_pairs(const RayRec *__restrict__ rec, const double *__restrict__ ends,
                                                           int64_t n, int64_t T, int64_t tiles, double threshold,
                                                           unsigned long long *__restrict__ counter,
                                                           unsigned long long *__restrict__ keys, double *__restrict__ dist,
                                                           int64_t cap) {
  __shared__ RayRec tile[GR_RAY_TILE];
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned long long found = 0;
  for (int64_t k = blockIdx.x; k < tiles; k += gridDim.x) {
    int64_t row, col;
    tri_decode(k, T, row, col);
    const int64_t j0 = col * GR_RAY_TILE;
    const int nb = (int)((n - j0) < GR_RAY_TILE ? (n - j0) : GR_RAY_TILE);
    __syncthreads();   // the tile before this one has been walked by every wave
    if (tid < nb) tile[tid] = rec[j0 + tid];
    const int64_t i = row * GR_RAY_TILE + tid;
    const bool have_a = i < n;
    const int64_t ia = have_a ? i : n - 1;   // a padded lane is ray n - 1 throughout: segment_closest_points loads ends[3 * ia]
    const RayRec a = rec[ia];
    __syncthreads();
    // a tile on the diagonal: the wave's first ray is row * TILE + (tid - lane); nothing at or before it can be a j > i
    const int jj0 = row == col ? (tid - lane) + 1 : 0;
    for (int jj = jj0; jj < nb; ++jj) {
      const RayRec b = tile[jj];
      const int64_t j = j0 + jj;
      const double d = segment_distance(a, b, ends, ia, j);
      const bool hit = have_a & (i < j) & (a.id != b.id) & (d <= threshold);
      const unsigned long long mask = __ballot(hit);
      if (mask == 0) continue;
      if (FILL) {
        const unsigned long long base = wave_append(mask, counter, lane);
        if (hit) {
          const unsigned long long pos = base + (unsigned long long)wave_rank(mask, lane);
          if (pos < (unsigned long long)cap) {
            keys[pos] = ((unsigned long long)i << 32) | (unsigned long long)j;
            dist[pos] = d;
          }
        }
      } else {
        found += (unsigned long long)__popcll(mask);
      }
    }
  }
  if (!FILL && lane == 0 && found) atomicAdd(counter, found);
}

__global__ void __launch_bounds__(256) k_ray_split_keys(const unsigned long long *__restrict__ keys, int64_t m,
                                                        int32_t *__restrict__ ei, int32_t *__restrict__ ej) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= m) return;
  const unsigned long long key = keys[k];
  ei[k] = (int32_t)(key >> 32);
  ej[k] = (int32_t)(key & 0xFFFFFFFFull);
}

// One lane per ray, the triangles staged through LDS GR_CLIP_CHUNK at a time (nine doubles each; a face with an index outside
// [0, V) is staged as NaN and can never be hit).  Double-sided Moller-Trumbore: the nearest hit with t >= 0 along the
// infinite ray; of two triangles hit at the same t the first in `faces` wins.
__global__ void __launch_bounds__(256) k_rays_clip(const double *__restrict__ origins, const double *__restrict__ dirs, int64_t n,
                                                   const double *__restrict__ points, int64_t V,
                                                   const int32_t *__restrict__ faces, int F, int32_t *__restrict__ hit,
                                                   double *__restrict__ t_out, double *__restrict__ p_out) {
  __shared__ double tri[GR_CLIP_CHUNK][9];
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool have = r < n;
  const int64_t rr = have ? r : 0;
  double ox = 0, oy = 0, oz = 0, dx = 0, dy = 0, dz = 0;
  if (n > 0) {
    ox = origins[3 * rr]; oy = origins[3 * rr + 1]; oz = origins[3 * rr + 2];
    dx = dirs[3 * rr]; dy = dirs[3 * rr + 1]; dz = dirs[3 * rr + 2];
  }
  double best = INFINITY;
  bool any = false;
  for (int f0 = 0; f0 < F; f0 += GR_CLIP_CHUNK) {
    const int nf = (F - f0) < GR_CLIP_CHUNK ? (F - f0) : GR_CLIP_CHUNK;
    __syncthreads();
    for (int e = threadIdx.x; e < nf * 3; e += 256) {   // element e: vertex e % 3 of triangle e / 3
      const int32_t v = faces[3 * (int64_t)f0 + e];
      const bool ok = v >= 0 && v < V;
      const int64_t vv = ok ? v : 0;
      double *dst = &tri[e / 3][3 * (e % 3)];
      dst[0] = ok ? points[3 * vv] : NAN;
      dst[1] = ok ? points[3 * vv + 1] : NAN;
      dst[2] = ok ? points[3 * vv + 2] : NAN;
    }
    __syncthreads();
    for (int k = 0; k < nf; ++k) {
      const double *q = tri[k];
      const double e1x = q[3] - q[0], e1y = q[4] - q[1], e1z = q[5] - q[2];
      const double e2x = q[6] - q[0], e2y = q[7] - q[1], e2z = q[8] - q[2];
      const double px = dy * e2z - dz * e2y, py = dz * e2x - dx * e2z, pz = dx * e2y - dy * e2x;
      const double det = dot3(e1x, e1y, e1z, px, py, pz);
      const double inv = 1.0 / det;
      const double sx = ox - q[0], sy = oy - q[1], sz = oz - q[2];
      const double u = dot3(sx, sy, sz, px, py, pz) * inv;
      const double qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
      const double v = dot3(dx, dy, dz, qx, qy, qz) * inv;
      const double t = dot3(e2x, e2y, e2z, qx, qy, qz) * inv;
      // every comparison is false for NaN: a degenerate triangle or a parallel ray (det == 0: inv infinite, u, v or t NaN or
      // infinite) is never a hit
      const bool ok = (det != 0.0) & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0) & (t >= 0.0) & (t < best);
      best = ok ? t : best;
      any |= ok;
    }
  }
  if (!have) return;
  hit[r] = any ? 1 : 0;
  t_out[r] = any ? best : NAN;
  p_out[3 * r] = any ? ox + best * dx : NAN;
  p_out[3 * r + 1] = any ? oy + best * dy : NAN;
  p_out[3 * r + 2] = any ? oz + best * dz : NAN;
}

}  // namespace

extern "C" {

int gr_ray_pairs_tile(int64_t tile, int64_t tiles_per_side, int64_t *row_h, int64_t *col_h) {
  if (!row_h || !col_h || tiles_per_side <= 0 || tiles_per_side > GR_RAY_MAX_N / GR_RAY_TILE || tile < 0 ||
      tile >= tri_off(tiles_per_side, tiles_per_side))
    return GR_EINVAL;
  tri_decode(tile, tiles_per_side, *row_h, *col_h);
  return GR_OK;
}

int gr_ray_pairs(gr_ctx *c, const double *starts, const double *ends, const int32_t *ray_ids, int64_t n, double threshold,
                 int32_t *edge_i, int32_t *edge_j, double *edge_d, int64_t edge_cap, int64_t *total_h, void *stream) {
  if (!c) return GR_EINVAL;
  if (!total_h || n < 0 || edge_cap < 0 || edge_cap > 0x7FFFFFFFll)
    return fail(c, GR_EINVAL, "bad ray-pair args (n=%lld, edge_cap=%lld)", (long long)n, (long long)edge_cap);
  if (n > GR_RAY_MAX_N) return fail(c, GR_EINVAL, "%lld rays: gr_ray_pairs takes at most %d per call", (long long)n, GR_RAY_MAX_N);
  const bool fill = edge_cap > 0 && edge_i && edge_j && edge_d;
  if (edge_cap > 0 && !fill) return fail(c, GR_EINVAL, "edge_cap %lld without edge buffers", (long long)edge_cap);
  *total_h = 0;
  if (n > 0 && (!starts || !ends || !ray_ids)) return fail(c, GR_EINVAL, "null ray arrays");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  const int64_t T = ceil_div(n, GR_RAY_TILE), tiles = tri_off(T, T);
  const int64_t cap = fill ? edge_cap : 0;
  int nbits = 1;
  while (((int64_t)1 << nbits) < n) ++nbits;
  // scratch: edge counter | rec [n] | keys [cap] | dist [cap] | sorted [cap] | rocPRIM
  Plan p;
  const auto o_counter = p.array<unsigned long long>(1);
  const auto o_rec = p.array<RayRec>(n);
  const auto o_keys = p.array<unsigned long long>(cap);
  const auto o_dist = p.array<double>(cap);
  const auto o_sorted = p.array<unsigned long long>(cap);
  const SortPairs<unsigned long long, double> sort(c, p, cap, 32 + nbits);   // i < n sits above bit 32; cap is 0 without edge buffers
  int rc = stage_acquire(c, c->stage, p.finish(), s, "ray-pair");
  if (rc != GR_OK) return rc;
  p.base = c->stage.ptr;
  if (c->opt_dbg & GR_DBG_POISON_RAYS) GR_HIP(c, hipMemsetAsync(p.base, 0xFF, (size_t)c->stage.have, s));   // test hook: nothing survives between calls
  unsigned long long *counter = o_counter(), *keys = o_keys(), *sorted = o_sorted();
  RayRec *rec = o_rec();
  double *dist = o_dist();
  GR_HIP(c, hipMemsetAsync(counter, 0, sizeof(unsigned long long), s));
  if (tiles > 0) {
    hipLaunchKernelGGL(k_ray_prep, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, starts, ends, ray_ids, n, rec);
    const int64_t max_grid = (c->opt_dbg & GR_DBG_RAY_GRID_7) ? 7 : GR_RAY_MAX_GRID;   // test hook: a few workgroups stride over all tiles
    const unsigned grid = (unsigned)(tiles < max_grid ? tiles : max_grid);
    if (fill)
      hipLaunchKernelGGL(k_ray_pairs<true>, dim3(grid), dim3(GR_RAY_TILE), 0, s, rec, ends, n, T, tiles, threshold, counter,
                         keys, dist, cap);
    else
      hipLaunchKernelGGL(k_ray_pairs<false>, dim3(grid), dim3(GR_RAY_TILE), 0, s, rec, ends, n, T, tiles, threshold, counter,
                         (unsigned long long *)nullptr, (double *)nullptr, (int64_t)0);
    GR_HIP(c, hipGetLastError());
  }
  unsigned long long total = 0;
  GR_HIP(c, hipMemcpyAsync(&total, counter, sizeof(total), hipMemcpyDeviceToHost, s));
  GR_HIP(c, hipStreamSynchronize(s));
  *total_h = (int64_t)total;
  if (!fill || total == 0) return GR_OK;
  if ((int64_t)total > cap)
    return fail(c, GR_EOVERFLOW, "%llu ray pairs within the threshold, the edge buffers hold %lld: call again with that capacity",
                total, (long long)cap);
  GR_TRY(sort.run(keys, sorted, dist, edge_d, s, (int64_t)total));   // total <= cap of the declared elements
  hipLaunchKernelGGL(k_ray_split_keys, dim3((unsigned)ceil_div((int64_t)total, 256)), dim3(256), 0, s, sorted, (int64_t)total,
                     edge_i, edge_j);
  GR_HIP(c, hipGetLastError());
  // the sort and the split still read the context's scratch: the call ends only when they are through, so that the next call
  // on ANY stream of this context (and every other user of the sort scratch) finds it free
  GR_HIP(c, hipStreamSynchronize(s));
  return GR_OK;
}

int gr_rays_clip(gr_ctx *c, const double *origins, const double *directions, int64_t n, const double *points, int64_t V,
                 const int32_t *faces, int64_t F, int32_t *hit, double *t, double *hit_points, void *stream) {
  if (!c) return GR_EINVAL;
  if (n < 0 || V < 0 || F < 0 || n > 0x7FFFFFFFll * 256) return fail(c, GR_EINVAL, "bad ray-clip args");
  if (F > GR_CLIP_MAX_TRIANGLES)
    return fail(c, GR_EINVAL, "%lld triangles: gr_rays_clip tests every ray against every triangle and takes at most %d (a coarse "
                "boundary surface, not the photogrammetry mesh)", (long long)F, GR_CLIP_MAX_TRIANGLES);
  if (n == 0) return GR_OK;
  if (!origins || !directions || !hit || !t || !hit_points || (F > 0 && (!points || !faces || V <= 0)))
    return fail(c, GR_EINVAL, "null ray-clip arrays");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(k_rays_clip, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, origins, directions, n, points, V, faces,
                     (int)F, hit, t, hit_points);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

}  // extern "C"
