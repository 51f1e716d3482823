// geograypher_amd/csrc/select.hip -- annotation_image_selection: a small set of views that together see every required face of
// a face x view incidence (gr_set_cover; the rule-set is DESIGN.md section 8j, M1-M8).  Needs no uploaded mesh.  Integers only:
// every count is a sum of ones, so nothing depends on scheduling.
//
// The incidence arrives face-major (CSR).  Set-up: k_sc_rows (required flags, per-view entry counts, initial gains),
// k_sc_scan (one workgroup: view pointers), k_sc_scatter (the view-major transpose).  The order of the faces WITHIN a view's
// list depends on scheduling and affects no result: every use of a list is a walk over all of it whose effects commute
// (flag stores to distinct faces, integer adds).
// Greedy: k_sc_pick (ONE workgroup: the maximum of gain << 32 | ~view, so ties go to the lowest view) and k_sc_apply (walks the
// chosen view's list; a required, uncovered face is marked and every other view of its row loses one gain) alternate, enqueued
// GR_SETCOVER_BATCH pairs at a time; the host reads the control words once per batch.  Pick is a launch of its own because apply
// changes the gains.  After `done` both kernels return at once.  Total work over the run: every row is walked once, when its
// face is covered -- O(nnz) -- plus the walk of each selected view's list.
// The decrements of one apply hit the few views that overlap the chosen one: up to GR_SETCOVER_LDS_VIEWS views a workgroup
// collects them in an LDS histogram (4 bytes a view: 16 KiB at the limit) and flushes its non-zero counters with one global
// atomic each; above, or with GR_SETCOVER_GLOBAL_ATOMICS, every decrement is a global atomic.  The chosen view's own gain,
// which every covered face would decrement, is not counted down but stored as 0 (M3: all its required faces are covered).
// Prune: k_sc_fill_m, then per examined view k_sc_prune_test (clears red[i] when a required face of the view has m < 2) and
// k_sc_prune_apply (conditional on red[i]), one word per examined view so that no launch resets what another reads.
// No cooperative launch, no waiting between workgroups; every loop is bounded by F, n_views, nnz or a clamped row.
#include "geom_dev.hpp"
#include "gr_internal.hpp"

using namespace grimpl;

#define GR_SC_BLOCK 256
#define GR_SC_PICK_BLOCK 1024
#define GR_SC_MAX_GRID 1024       // workgroups of the set-up kernels (each flushes up to 2 n_views counters)
#define GR_SC_MAX_WALK_GRID 512   // workgroups that walk one view's list (those beyond its end return at once)

namespace {

typedef unsigned long long u64;

enum {  // 32-bit control words at the front of the scratch; the host reads all GR_SC_CTL_WORDS once per batch
  SC_FLAG = 0,     // != 0: a view index outside [0, n_views) or a row pointer outside [0, nnz] / decreasing
  SC_DONE = 1,     // != 0: every gain is 0 (or the input is bad): pick and apply return at once
  SC_CUR = 2,      // the view the last pick chose
  SC_K = 3,        // views selected
  SC_P = 4,        // views pruned
  SC_NREQ = 8,     // u64 (words 8, 9): required faces
  SC_NCOV = 10,    // u64: covered faces
  GR_SC_CTL_WORDS = 16
};

// entries [b, e) of row f, clamped into [0, nnz] whatever the pointers hold; false when they had to be clamped
__device__ __forceinline__ bool row_range(const int64_t *__restrict__ face_ptr, int64_t f, int64_t nnz, int64_t &b, int64_t &e) {
  const int64_t b0 = face_ptr[f], e0 = face_ptr[f + 1];
  b = b0 < 0 ? 0 : (b0 > nnz ? nnz : b0);
  e = e0 < b ? b : (e0 > nnz ? nnz : e0);
  return b == b0 && e == e0;
}

__global__ void __launch_bounds__(GR_SC_BLOCK) k_sc_init(int n_views, uint32_t *__restrict__ ctl, int32_t *__restrict__ gain,
                                                        uint32_t *__restrict__ vcount, int32_t *__restrict__ red,
                                                        uint8_t *__restrict__ selected, int32_t *__restrict__ order,
                                                        int64_t *__restrict__ gains, int32_t *__restrict__ pruned) {
  const int v = blockIdx.x * GR_SC_BLOCK + threadIdx.x;
  if (ctl && v < GR_SC_CTL_WORDS) ctl[v] = 0;
  if (v >= n_views) return;
  if (ctl) { gain[v] = 0; vcount[v] = 0; red[v] = 1; }   // (no scratch: an empty problem, the outputs alone)
  selected[v] = 0; order[v] = -1; gains[v] = 0; pruned[v] = -1;
}

// M1, M2 and the initial M3: one lane per face, a grid-stride loop.  obs is the row length (the entries of a row are unique);
// an entry outside [0, n_views) sets the flag and is skipped here and everywhere else.  LDS (HIST): entry count | gain per view.
template <bool HIST>
__global__ void __launch_bounds__(GR_SC_BLOCK) k_sc_rows(const int64_t *__restrict__ face_ptr, const int32_t *__restrict__ face_views,
                                                        int64_t F, int n_views, int64_t nnz, double threshold,
                                                        uint8_t *__restrict__ req, uint32_t *__restrict__ vcount,
                                                        int32_t *__restrict__ gain, uint32_t *__restrict__ ctl) {
  extern __shared__ uint32_t sc_lds[];
  uint32_t *hc = sc_lds, *hg = sc_lds + n_views;
  const int tid = threadIdx.x;
  if (HIST) {
    for (int v = tid; v < 2 * n_views; v += GR_SC_BLOCK) sc_lds[v] = 0;
    __syncthreads();
  }
  u64 n_req = 0;
  int bad = 0;
  for (int64_t f = (int64_t)blockIdx.x * GR_SC_BLOCK + tid; f < F; f += (int64_t)gridDim.x * GR_SC_BLOCK) {
    int64_t b, e;
    bad |= !row_range(face_ptr, f, nnz, b, e);
    const bool required = (double)(e - b) >= threshold;
    req[f] = required ? 1 : 0;
    n_req += required ? 1 : 0;
    for (int64_t i = b; i < e; ++i) {
      const int32_t u = face_views[i];
      if ((uint32_t)u >= (uint32_t)n_views) { bad = 1; continue; }
      if (HIST) { atomicAdd(&hc[u], 1u); if (required) atomicAdd(&hg[u], 1u); }
      else { atomicAdd(&vcount[u], 1u); if (required) atomicAdd(&gain[u], 1); }
    }
  }
  n_req = wave_sum_u64(n_req);
  if ((tid & 63) == 0 && n_req) atomicAdd((u64 *)(ctl + SC_NREQ), n_req);
  if (bad) atomicOr(&ctl[SC_FLAG], 1u);
  if (!HIST) return;
  __syncthreads();
  for (int v = tid; v < n_views; v += GR_SC_BLOCK) {
    const uint32_t c = hc[v], g = hg[v];
    if (c) atomicAdd(&vcount[v], c);
    if (g) atomicAdd(&gain[v], (int32_t)g);
  }
}

// vptr = exclusive scan of vcount (n_views + 1 values), cursor = vptr: one workgroup, each lane a contiguous run of views
__global__ void __launch_bounds__(GR_SC_BLOCK) k_sc_scan(const uint32_t *__restrict__ vcount, int n_views, int64_t *__restrict__ vptr,
                                                        u64 *__restrict__ cursor) {
  __shared__ int64_t part[GR_SC_BLOCK];
  const int tid = threadIdx.x;
  const int per = (n_views + GR_SC_BLOCK - 1) / GR_SC_BLOCK;
  const int v0 = tid * per < n_views ? tid * per : n_views, v1 = v0 + per < n_views ? v0 + per : n_views;
  int64_t sum = 0;
  for (int v = v0; v < v1; ++v) sum += vcount[v];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int64_t run = 0;
    for (int t = 0; t < GR_SC_BLOCK; ++t) { const int64_t p = part[t]; part[t] = run; run += p; }
    vptr[n_views] = run;
  }
  __syncthreads();
  int64_t run = part[tid];
  for (int v = v0; v < v1; ++v) { vptr[v] = run; cursor[v] = (u64)run; run += vcount[v]; }
}

// The transpose: workgroup b owns the faces [b chunk, (b + 1) chunk).  HIST: it counts its entries per view in LDS, reserves a
// run of every view's list with ONE returning global atomic per view present, and places its faces through LDS cursors.
// LDS (HIST): base [n_views] u64 | count, then cursor [n_views] u32.
template <bool HIST>
__global__ void __launch_bounds__(GR_SC_BLOCK) k_sc_scatter(const int64_t *__restrict__ face_ptr, const int32_t *__restrict__ face_views,
                                                           int64_t F, int64_t chunk, int n_views, int64_t nnz,
                                                           u64 *__restrict__ cursor, int32_t *__restrict__ vfaces) {
  extern __shared__ u64 sc_lds64[];
  u64 *base = sc_lds64;
  uint32_t *cnt = (uint32_t *)(sc_lds64 + n_views);
  const int tid = threadIdx.x;
  const int64_t f0 = (int64_t)blockIdx.x * chunk, f1 = f0 + chunk < F ? f0 + chunk : F;
  if (HIST) {
    for (int v = tid; v < n_views; v += GR_SC_BLOCK) cnt[v] = 0;
    __syncthreads();
    for (int64_t f = f0 + tid; f < f1; f += GR_SC_BLOCK) {
      int64_t b, e;
      row_range(face_ptr, f, nnz, b, e);
      for (int64_t i = b; i < e; ++i) {
        const int32_t u = face_views[i];
        if ((uint32_t)u < (uint32_t)n_views) atomicAdd(&cnt[u], 1u);
      }
    }
    __syncthreads();
    for (int v = tid; v < n_views; v += GR_SC_BLOCK) {
      const uint32_t c = cnt[v];
      if (c) base[v] = atomicAdd(&cursor[v], (u64)c);
      cnt[v] = 0;
    }
    __syncthreads();
  }
  for (int64_t f = f0 + tid; f < f1; f += GR_SC_BLOCK) {
    int64_t b, e;
    row_range(face_ptr, f, nnz, b, e);
    for (int64_t i = b; i < e; ++i) {
      const int32_t u = face_views[i];
      if ((uint32_t)u >= (uint32_t)n_views) continue;
      const u64 pos = HIST ? base[u] + atomicAdd(&cnt[u], 1u) : atomicAdd(&cursor[u], 1ull);
      if (pos < (u64)nnz) vfaces[pos] = (int32_t)f;   // (always: the lists hold the entries k_sc_rows counted)
    }
  }
}

// M4, first half: ONE workgroup.  The winner's key is the largest gain << 32 | (0xFFFFFFFF - view).
__global__ void __launch_bounds__(GR_SC_PICK_BLOCK) k_sc_pick(const int32_t *__restrict__ gain, int n_views, uint32_t *__restrict__ ctl,
                                                             uint8_t *__restrict__ selected, int32_t *__restrict__ order,
                                                             int64_t *__restrict__ gains) {
  __shared__ u64 wave_best[GR_SC_PICK_BLOCK / 64];
  if (ctl[SC_DONE]) return;
  const int tid = threadIdx.x;
  u64 best = 0;
  for (int v = tid; v < n_views; v += GR_SC_PICK_BLOCK) {
    const int32_t g = gain[v];
    const u64 key = ((u64)(uint32_t)(g > 0 ? g : 0) << 32) | (u64)(0xFFFFFFFFu - (uint32_t)v);
    best = key > best ? key : best;
  }
  best = wave_max_u64(best);
  if ((tid & 63) == 0) wave_best[tid >> 6] = best;
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < GR_SC_PICK_BLOCK / 64; ++w) best = wave_best[w] > best ? wave_best[w] : best;
  const uint32_t g = (uint32_t)(best >> 32), v = 0xFFFFFFFFu - (uint32_t)best;
  const uint32_t k = ctl[SC_K];
  if (g == 0 || ctl[SC_FLAG] || k >= (uint32_t)n_views) { ctl[SC_DONE] = 1; return; }
  order[k] = (int32_t)v; gains[k] = (int64_t)g; selected[v] = 1;
  ctl[SC_K] = k + 1; ctl[SC_CUR] = v;
}

// M4, second half.  A face occurs once in the chosen view's list, so its flag has one writer.
template <bool HIST>
__global__ void __launch_bounds__(GR_SC_BLOCK) k_sc_apply(const int64_t *__restrict__ face_ptr, const int32_t *__restrict__ face_views,
                                                         const int64_t *__restrict__ vptr, const int32_t *__restrict__ vfaces,
                                                         int n_views, int64_t nnz, uint8_t *__restrict__ req,
                                                         int32_t *__restrict__ gain, const uint32_t *__restrict__ ctl) {
  extern __shared__ uint32_t sc_lds[];
  if (ctl[SC_DONE]) return;
  const int tid = threadIdx.x;
  const int32_t cur = (int32_t)ctl[SC_CUR];
  const int64_t beg = vptr[cur], len = vptr[cur + 1] - beg;
  if (blockIdx.x == 0 && tid == 0) gain[cur] = 0;   // no decrement below touches gain[cur]
  if ((int64_t)blockIdx.x * GR_SC_BLOCK >= len) return;
  if (HIST) {
    for (int v = tid; v < n_views; v += GR_SC_BLOCK) sc_lds[v] = 0;
    __syncthreads();
  }
  for (int64_t i = (int64_t)blockIdx.x * GR_SC_BLOCK + tid; i < len; i += (int64_t)gridDim.x * GR_SC_BLOCK) {
    const int32_t f = vfaces[beg + i];
    if (req[f] != 1) continue;   // not required, or covered already
    req[f] = 3;
    int64_t b, e;
    row_range(face_ptr, f, nnz, b, e);
    for (int64_t j = b; j < e; ++j) {
      const int32_t u = face_views[j];
      if (u == cur || (uint32_t)u >= (uint32_t)n_views) continue;
      if (HIST) atomicAdd(&sc_lds[u], 1u);
      else atomicSub(&gain[u], 1);
    }
  }
  if (!HIST) return;
  __syncthreads();
  for (int v = tid; v < n_views; v += GR_SC_BLOCK) {
    const uint32_t h = sc_lds[v];
    if (h) atomicSub(&gain[v], (int32_t)h);
  }
}

// M6: m[f] = selected views that see f, face-major
__global__ void __launch_bounds__(GR_SC_BLOCK) k_sc_fill_m(const int64_t *__restrict__ face_ptr, const int32_t *__restrict__ face_views,
                                                          int64_t F, int n_views, int64_t nnz, const uint8_t *__restrict__ selected,
                                                          int32_t *__restrict__ m) {
  for (int64_t f = (int64_t)blockIdx.x * GR_SC_BLOCK + threadIdx.x; f < F; f += (int64_t)gridDim.x * GR_SC_BLOCK) {
    int64_t b, e;
    row_range(face_ptr, f, nnz, b, e);
    int32_t n = 0;
    for (int64_t i = b; i < e; ++i) {
      const int32_t u = face_views[i];
      if ((uint32_t)u < (uint32_t)n_views) n += selected[u];
    }
    m[f] = n;
  }
}

// examined view number `step`: order[k - 1 - step].  red[step] starts at 1 (k_sc_init).
__global__ void __launch_bounds__(GR_SC_BLOCK) k_sc_prune_test(int step, const uint32_t *__restrict__ ctl, const int32_t *__restrict__ order,
                                                              const int64_t *__restrict__ vptr, const int32_t *__restrict__ vfaces,
                                                              const uint8_t *__restrict__ req, const int32_t *__restrict__ m,
                                                              int32_t *__restrict__ red) {
  const int idx = (int)ctl[SC_K] - 1 - step;
  if (idx < 0) return;
  const int32_t v = order[idx];
  const int64_t beg = vptr[v], len = vptr[v + 1] - beg;
  int needed = 0;
  for (int64_t i = (int64_t)blockIdx.x * GR_SC_BLOCK + threadIdx.x; i < len; i += (int64_t)gridDim.x * GR_SC_BLOCK) {
    const int32_t f = vfaces[beg + i];
    needed |= (req[f] & 1) && m[f] < 2;
  }
  if (needed) atomicAnd(&red[step], 0);
}

__global__ void __launch_bounds__(GR_SC_BLOCK) k_sc_prune_apply(int step, uint32_t *__restrict__ ctl, const int32_t *__restrict__ order,
                                                               const int64_t *__restrict__ vptr, const int32_t *__restrict__ vfaces,
                                                               int32_t *__restrict__ m, const int32_t *__restrict__ red,
                                                               uint8_t *__restrict__ selected, int32_t *__restrict__ pruned) {
  const int idx = (int)ctl[SC_K] - 1 - step;
  if (idx < 0 || !red[step]) return;
  const int32_t v = order[idx];
  const int64_t beg = vptr[v], len = vptr[v + 1] - beg;
  for (int64_t i = (int64_t)blockIdx.x * GR_SC_BLOCK + threadIdx.x; i < len; i += (int64_t)gridDim.x * GR_SC_BLOCK)
    m[vfaces[beg + i]] -= 1;   // a face occurs once in the list
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    selected[v] = 0;
    const uint32_t p = ctl[SC_P];   // launches of one stream run one after the other: the order examined
    pruned[p] = v;
    ctl[SC_P] = p + 1;
  }
}

__global__ void __launch_bounds__(GR_SC_BLOCK) k_sc_count_covered(const uint8_t *__restrict__ req, int64_t F, uint32_t *__restrict__ ctl) {
  u64 n = 0;
  for (int64_t f = (int64_t)blockIdx.x * GR_SC_BLOCK + threadIdx.x; f < F; f += (int64_t)gridDim.x * GR_SC_BLOCK) n += req[f] == 3;
  n = wave_sum_u64(n);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd((u64 *)(ctl + SC_NCOV), n);
}

__global__ void k_sc_finish(const uint32_t *__restrict__ ctl, int64_t batches, int64_t lds_histogram, int64_t *__restrict__ stats) {
  const u64 *wide = (const u64 *)ctl;   // (null: an empty problem)
  stats[GR_SETCOVER_STAT_REQUIRED] = ctl ? (int64_t)wide[SC_NREQ / 2] : 0;
  stats[GR_SETCOVER_STAT_COVERED] = ctl ? (int64_t)wide[SC_NCOV / 2] : 0;
  stats[GR_SETCOVER_STAT_SELECTED] = ctl ? ctl[SC_K] : 0;
  stats[GR_SETCOVER_STAT_PRUNED] = ctl ? ctl[SC_P] : 0;
  stats[GR_SETCOVER_STAT_BATCHES] = batches;
  stats[GR_SETCOVER_STAT_LDS_HISTOGRAM] = lds_histogram;
  for (int i = GR_SETCOVER_STAT_LDS_HISTOGRAM + 1; i < GR_SETCOVER_STAT_WORDS; ++i) stats[i] = 0;
}

}  // namespace

extern "C" {

int gr_set_cover(gr_ctx *c, const int64_t *face_ptr, const int32_t *face_views, int64_t nnz, int64_t F, int32_t n_views,
                 double min_observations, int flags, uint8_t *selected, int32_t *order, int64_t *gains, int32_t *pruned,
                 int64_t *stats, void *stream) {
  if (!c) return GR_EINVAL;
  if (F < 0 || F > 0x7FFFFFFFll || n_views < 0 || n_views > GR_SETCOVER_MAX_VIEWS || nnz < 0)
    return fail(c, GR_EINVAL, "gr_set_cover: bad shape F=%lld n_views=%d nnz=%lld (F < 2^31, n_views <= %d)", (long long)F,
                (int)n_views, (long long)nnz, (int)GR_SETCOVER_MAX_VIEWS);
  if (!(min_observations == min_observations))
    return fail(c, GR_EINVAL, "gr_set_cover: min_observations is not a number");
  if (!stats || !face_ptr || (nnz > 0 && !face_views) || (n_views > 0 && (!selected || !order || !gains || !pruned)))
    return fail(c, GR_EINVAL, "gr_set_cover: null arrays");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  const int N = n_views;
  const bool hist = N <= GR_SETCOVER_LDS_VIEWS && !(flags & GR_SETCOVER_GLOBAL_ATOMICS);
  if (N == 0 || F == 0) {   // nothing can be required or selected
    if (N > 0)
      hipLaunchKernelGGL(k_sc_init, dim3((unsigned)ceil_div(N, GR_SC_BLOCK)), dim3(GR_SC_BLOCK), 0, s, N, (uint32_t *)nullptr,
                         (int32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr, selected, order, gains, pruned);
    hipLaunchKernelGGL(k_sc_finish, dim3(1), dim3(1), 0, s, (const uint32_t *)nullptr, (int64_t)0, (int64_t)hist, stats);
    GR_HIP(c, hipGetLastError());
    return GR_OK;
  }
  // scratch: ctl | gain [N] | vcount [N] | red [N] | vptr [N + 1] | cursor [N] | m [F] | vfaces [nnz] | req [F]
  Carve cv;
  const auto o_ctl = cv.array<uint32_t>(GR_SC_CTL_WORDS);
  const auto o_gain = cv.array<int32_t>(N);
  const auto o_vcount = cv.array<uint32_t>(N);
  const auto o_red = cv.array<int32_t>(N);
  const auto o_vptr = cv.array<int64_t>((int64_t)N + 1);
  const auto o_cursor = cv.array<u64>(N);
  const auto o_m = cv.array<int32_t>(F), o_vfaces = cv.array<int32_t>(nnz);
  const auto o_req = cv.array<uint8_t>(F);
  int rc = stage_acquire(c, c->stage, cv.total(), s, "set-cover");
  if (rc != GR_OK) return rc;
  cv.base = c->stage.ptr;
  uint32_t *ctl = o_ctl(), *vcount = o_vcount();
  int32_t *gain = o_gain(), *red = o_red(), *m = o_m(), *vfaces = o_vfaces();
  int64_t *vptr = o_vptr();
  u64 *cursor = o_cursor();
  uint8_t *req = o_req();

  const double threshold = min_observations > 1.0 ? min_observations : 1.0;   // M2
  const unsigned setup_grid = (unsigned)std::min<int64_t>(ceil_div(F, GR_SC_BLOCK), GR_SC_MAX_GRID);
  const int64_t chunk = ceil_div(F, setup_grid);
  const unsigned walk_grid = (unsigned)std::min<int64_t>(ceil_div(F, GR_SC_BLOCK), GR_SC_MAX_WALK_GRID);   // a list holds at most F faces
  hipLaunchKernelGGL(k_sc_init, dim3((unsigned)ceil_div(std::max(N, (int)GR_SC_CTL_WORDS), GR_SC_BLOCK)), dim3(GR_SC_BLOCK), 0, s, N, ctl,
                     gain, vcount, red, selected, order, gains, pruned);
  if (hist) {
    hipLaunchKernelGGL(k_sc_rows<true>, dim3(setup_grid), dim3(GR_SC_BLOCK), (size_t)(8 * N), s, face_ptr, face_views, F, N, nnz, threshold,
                       req, vcount, gain, ctl);
    hipLaunchKernelGGL(k_sc_scan, dim3(1), dim3(GR_SC_BLOCK), 0, s, (const uint32_t *)vcount, N, vptr, cursor);
    hipLaunchKernelGGL(k_sc_scatter<true>, dim3(setup_grid), dim3(GR_SC_BLOCK), (size_t)(12 * N), s, face_ptr, face_views, F, chunk, N, nnz,
                       cursor, vfaces);
  } else {
    hipLaunchKernelGGL(k_sc_rows<false>, dim3(setup_grid), dim3(GR_SC_BLOCK), 0, s, face_ptr, face_views, F, N, nnz, threshold, req, vcount,
                       gain, ctl);
    hipLaunchKernelGGL(k_sc_scan, dim3(1), dim3(GR_SC_BLOCK), 0, s, (const uint32_t *)vcount, N, vptr, cursor);
    hipLaunchKernelGGL(k_sc_scatter<false>, dim3(setup_grid), dim3(GR_SC_BLOCK), 0, s, face_ptr, face_views, F, chunk, N, nnz, cursor,
                       vfaces);
  }
  GR_HIP(c, hipGetLastError());

  // the greedy stage: every pick before `done` selects another view, so N + 1 picks always reach it
  uint32_t ctl_h[GR_SC_CTL_WORDS] = {0};
  const int max_batches = (int)ceil_div((int64_t)N + 1, GR_SETCOVER_BATCH);
  int batches = 0;
  while (batches < max_batches) {
    for (int i = 0; i < GR_SETCOVER_BATCH; ++i) {
      hipLaunchKernelGGL(k_sc_pick, dim3(1), dim3(GR_SC_PICK_BLOCK), 0, s, (const int32_t *)gain, N, ctl, selected, order, gains);
      if (hist)
        hipLaunchKernelGGL(k_sc_apply<true>, dim3(walk_grid), dim3(GR_SC_BLOCK), (size_t)(4 * N), s, face_ptr, face_views,
                           (const int64_t *)vptr, (const int32_t *)vfaces, N, nnz, req, gain, (const uint32_t *)ctl);
      else
        hipLaunchKernelGGL(k_sc_apply<false>, dim3(walk_grid), dim3(GR_SC_BLOCK), 0, s, face_ptr, face_views, (const int64_t *)vptr,
                           (const int32_t *)vfaces, N, nnz, req, gain, (const uint32_t *)ctl);
    }
    ++batches;
    GR_HIP(c, hipGetLastError());
    GR_HIP(c, hipMemcpyAsync(ctl_h, ctl, sizeof(ctl_h), hipMemcpyDeviceToHost, s));
    GR_HIP(c, hipStreamSynchronize(s));
    if (ctl_h[SC_FLAG])
      return fail(c, GR_EINDEX, "gr_set_cover: a view index outside [0, %d) or a row pointer outside [0, %lld]", N, (long long)nnz);
    if (ctl_h[SC_DONE]) break;
  }
  if (!ctl_h[SC_DONE]) return fail(c, GR_EHIP, "gr_set_cover: the greedy stage did not end within %d batches", max_batches);

  const int k = (int)ctl_h[SC_K];
  if ((flags & GR_SETCOVER_PRUNE) && k > 0) {
    hipLaunchKernelGGL(k_sc_fill_m, dim3(setup_grid), dim3(GR_SC_BLOCK), 0, s, face_ptr, face_views, F, N, nnz, (const uint8_t *)selected, m);
    for (int step = 0; step < k; ++step) {
      hipLaunchKernelGGL(k_sc_prune_test, dim3(walk_grid), dim3(GR_SC_BLOCK), 0, s, step, (const uint32_t *)ctl, (const int32_t *)order,
                         (const int64_t *)vptr, (const int32_t *)vfaces, (const uint8_t *)req, (const int32_t *)m, red);
      hipLaunchKernelGGL(k_sc_prune_apply, dim3(walk_grid), dim3(GR_SC_BLOCK), 0, s, step, ctl, (const int32_t *)order,
                         (const int64_t *)vptr, (const int32_t *)vfaces, m, (const int32_t *)red, selected, pruned);
    }
  }
  hipLaunchKernelGGL(k_sc_count_covered, dim3(setup_grid), dim3(GR_SC_BLOCK), 0, s, (const uint8_t *)req, F, ctl);
  hipLaunchKernelGGL(k_sc_finish, dim3(1), dim3(1), 0, s, (const uint32_t *)ctl, (int64_t)batches, (int64_t)hist, stats);
  GR_HIP(c, hipGetLastError());
  GR_HIP(c, hipStreamSynchronize(s));   // the scratch is free on return
  return GR_OK;
}

}  // extern "C"
