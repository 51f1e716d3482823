// geograypher_amd/csrc/components.hip -- connected components of equally labelled faces on the mesh surface, and the sieve that
// merges components below a measure into their greatest labelled neighbour (gr_face_sieve; the rule-set is DESIGN.md section 8u,
// I1-I10).  Needs no uploaded mesh; its scratch is the stage arena.
//
// Shape.  ADJACENCY, once per call: k_sieve_keys gives every face that takes part three keys (lo << 32) | hi of its canonical
// corners with the face as the value, a face that does not (degenerate, or a corner outside [0, V)) three keys that sort behind all
// others; one radix sort over the 32 + bit_length(V) bits in use (cub_steps.hpp) puts the faces of an edge side by side.  A RUN of
// equal keys is an edge; an entry finds its run by walking the sorted keys to both sides, two entries of a run are edge-neighbours
// (I3: pairwise, a fan of k faces costs k^2 pair visits).  COMPONENTS, once per round: a union-find over the faces; k_cc_hook
// unites the two faces of every same-class pair of a run by hooking the LARGER root under the smaller with a compare-and-swap,
// halving paths on the way (parents only ever decrease: no cycle, and the smallest face of a component can never get a parent, so
// it is the root whatever the order of the pairs); k_cc_compress walks every face to its root.  MEASURES: 64-bit integer atomicAdd
// per component, pre-reduced in the wave: one component kept in registers across 16 chunks of 64 faces, the other lanes summed
// where they hold the same component in a row (a segmented suffix sum by shuffles).  Kernels that count stride over their items
// and count in registers: one atomic per wave of the launch and word.
// TARGETS: the order I6 is wider than 64 bits, so two atomic passes over the entries settle it: the largest measure among the
// labelled neighbour components (k_target_measure, atomicMax), then the lowest id among those (k_target_id, atomicMin).
// k_pointers decides per component whether it points; k_jump walks every pointer chain to its root and stores the root (a racing
// reader sees the old or the new pointer, both on its chain); k_relabel gives the faces of a pointing component the class of
// their root's first face -- a root does not point, so that word is not written in the round -- and counts the faces it changed,
// one atomic per wave.  The host reads that count back once per round.  Everything is integers; every atomic is a sum, a maximum
// or a minimum of integers, or a compare-and-swap whose outcome the result does not depend on: the outputs are the same bytes
// for every launch and arrival order.  No index is used that was not checked against its array first.
#include "cub_steps.hpp"
#include "geom_dev.hpp"
#include "gr_internal.hpp"

namespace {
using namespace grimpl;

typedef unsigned long long u64;

constexpr int SV_BLOCK = 256;
constexpr int SV_COUNT_GROUPS = 1024;   // workgroups of a kernel that counts: they stride over the items and count in registers, so a
                                        // word gets one atomic per wave of the LAUNCH, not of the items (an atomic per 64 items on one word
                                        // is a serial chain: 0.85 ms over C5's 5 M faces, measured)
constexpr int SV_MEASURE_CHUNKS = 16;   // consecutive 64-face chunks a wave of k_measure walks
constexpr int64_t SV_MAX = 0x7FFFFFFFll;   // F, V < SV_MAX; 3 F <= SV_MAX

enum {  // the call's control words in the arena
  CT_CHANGED = 0,   // faces the running round changed
  CT_NCOMP = 1,     // components of the current labelling
  CT_NSMALL = 2,    // ... that are small (I7)
  CT_DEGEN = 3,
  CT_MULTI = 4,
  CT_BAD = 5,
  CT_BEFORE = 6,    // CT_NCOMP of the first labelling
  CT_WORDS = 8
};

struct SieveHost {   // what the host knows when the statistics are written
  u64 rounds, faces_changed, cap;
};

__device__ __forceinline__ int32_t ld(const int32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ void st(int32_t *p, int32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }

// I1, I2: the three keys of every face, its normalised class, whether it takes part
__global__ __launch_bounds__(SV_BLOCK) void k_sieve_keys(const int32_t *__restrict__ faces, const int32_t *__restrict__ canon, int64_t F, int64_t V,
                                                        const int32_t *face_class, int32_t *class_out, u64 *__restrict__ keys,
                                                        int32_t *__restrict__ vals, uint8_t *__restrict__ live, u64 *ctl) {
  const int lane = (int)(threadIdx.x & 63);
  uint32_t n_bad = 0, n_degenerate = 0;   // per lane at most F / (SV_COUNT_GROUPS * SV_BLOCK) + 1: a wave's sum fits 32 bits
  for (int64_t f = (int64_t)blockIdx.x * SV_BLOCK + threadIdx.x; f < F; f += (int64_t)gridDim.x * SV_BLOCK) {
    bool bad = false, degenerate = false;
    int32_t v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = faces[3 * f + k];
      if (v[k] < 0 || v[k] >= V) { bad = true; v[k] = 0; }
      else if (canon) {
        v[k] = canon[v[k]];
        if (v[k] < 0 || v[k] >= V) { bad = true; v[k] = 0; }
      }
    }
    degenerate = !bad && (v[0] == v[1] || v[1] == v[2] || v[0] == v[2]);
    const bool takes_part = !bad && !degenerate;
    const u64 parked = (u64)V << 32;   // lo = V: behind every real key
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int32_t a = v[k], b = v[(k + 1) % 3];
      const u64 lo = (u64)(a < b ? a : b), hi = (u64)(a < b ? b : a);
      keys[3 * f + k] = takes_part ? ((lo << 32) | hi) : parked;
      vals[3 * f + k] = (int32_t)f;
    }
    live[f] = takes_part ? 1 : 0;
    const int32_t cl = face_class[f];
    class_out[f] = cl < 0 ? -1 : cl;   // (in place: a lane reads and writes its own word)
    n_bad += bad ? 1u : 0u;
    n_degenerate += degenerate ? 1u : 0u;
  }
  stat_add_u32(ctl, CT_DEGEN, n_degenerate, lane);
  stat_add_u32(ctl, CT_BAD, n_bad, lane);
}

// edges shared by more than two faces, counted at the head of their run
__global__ __launch_bounds__(SV_BLOCK) void k_sieve_fans(const u64 *__restrict__ keys, int64_t N, int64_t V, u64 *ctl) {
  uint32_t n_fans = 0;
  for (int64_t i = (int64_t)blockIdx.x * SV_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * SV_BLOCK) {
    const u64 k = keys[i];
    n_fans += ((int64_t)(k >> 32) != V && (i == 0 || keys[i - 1] != k) && i + 2 < N && keys[i + 2] == k) ? 1u : 0u;
  }
  stat_add_u32(ctl, CT_MULTI, n_fans, (int)(threadIdx.x & 63));
}

__global__ __launch_bounds__(SV_BLOCK) void k_round_init(int64_t F, int32_t *__restrict__ parent, u64 *__restrict__ meas, u64 *__restrict__ best_m,
                                                        int32_t *__restrict__ best_id) {
  const int64_t f = (int64_t)blockIdx.x * SV_BLOCK + threadIdx.x;
  if (f >= F) return;
  parent[f] = (int32_t)f;
  meas[f] = 0;
  best_m[f] = 0;
  best_id[f] = 0x7FFFFFFF;
}

__device__ __forceinline__ int32_t uf_find(int32_t *parent, int32_t x) {
  int32_t p = ld(parent + x);
  while (p != x) {   // p < x: halve the path
    const int32_t g = ld(parent + p);
    if (g != p) st(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ void uf_unite(int32_t *parent, int32_t a, int32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) { const int32_t t = a; a = b; b = t; }
    if (atomicCAS(parent + a, a, b) == a) return;   // a was still a root: hooked under the smaller one
  }
}

// I4: the pairs (entry i, an earlier entry of its run) of equal class
__global__ __launch_bounds__(SV_BLOCK) void k_cc_hook(const u64 *__restrict__ keys, const int32_t *__restrict__ sf, int64_t N, int64_t V,
                                                     const int32_t *__restrict__ cls, int32_t *parent) {
  const int64_t i = (int64_t)blockIdx.x * SV_BLOCK + threadIdx.x;
  if (i >= N) return;
  const u64 k = keys[i];
  if ((int64_t)(k >> 32) == V) return;
  const int32_t f = sf[i], cf = cls[f];
  for (int64_t j = i - 1; j >= 0 && keys[j] == k; --j) {
    const int32_t g = sf[j];
    if (cls[g] == cf) uf_unite(parent, f, g);
  }
}

__global__ __launch_bounds__(SV_BLOCK) void k_cc_compress(int64_t F, const int32_t *__restrict__ parent, const uint8_t *__restrict__ live,
                                                         int32_t *__restrict__ comp, u64 *ctl) {
  uint32_t n_roots = 0;
  for (int64_t f = (int64_t)blockIdx.x * SV_BLOCK + threadIdx.x; f < F; f += (int64_t)gridDim.x * SV_BLOCK) {
    int32_t r = -1;
    if (live[f]) {
      r = (int32_t)f;
      for (int32_t p = parent[r]; p != r; p = parent[r]) r = p;
      n_roots += r == (int32_t)f ? 1u : 0u;
    }
    comp[f] = r;
  }
  stat_add_u32(ctl, CT_NCOMP, n_roots, (int)(threadIdx.x & 63));
}

// I5.  A wave walks SV_MEASURE_CHUNKS consecutive chunks of 64 faces.  It KEEPS one component -- that of its first face, chosen
// anew when a chunk holds no face of it -- and sums that component's faces in registers across the chunks: one atomic per wave
// and kept component.  The other lanes are summed by rows, lanes in a row with the same component, by a segmented suffix sum, and
// the first lane of a row adds.  (Rows alone left the largest component of a speckled map with six atomics per 64 faces on ONE
// word: 4.3 ms over C5's 5 M faces, measured.)  Integer sums: the grouping does not show in the result.
__global__ __launch_bounds__(SV_BLOCK) void k_measure(int64_t F, const int32_t *__restrict__ comp, const int64_t *__restrict__ weights, u64 *meas) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t base = ((int64_t)blockIdx.x * (SV_BLOCK / 64) + (int64_t)(threadIdx.x >> 6)) * (64 * SV_MEASURE_CHUNKS);
  int32_t kept = -1;   // uniform over the wave, like kept_sum
  u64 kept_sum = 0;
  for (int k = 0; k < SV_MEASURE_CHUNKS && base + (int64_t)k * 64 < F; ++k) {
    const int64_t f = base + (int64_t)k * 64 + lane;
    const int32_t a = f < F ? comp[f] : -1;
    u64 w = a >= 0 ? (weights ? (u64)weights[f] : 1ull) : 0ull;
    if (!__ballot(a >= 0 && a == kept)) {   // no face of the kept component here: it is added, another one kept
      if (lane == 0 && kept >= 0) atomicAdd(meas + kept, kept_sum);
      const u64 have = __ballot(a >= 0);
      kept = have ? __shfl(a, __ffsll((long long)have) - 1) : -1;
      kept_sum = 0;
    }
    const bool is_kept = a >= 0 && a == kept;
    kept_sum += wave_sum_u64(is_kept ? w : 0ull);
    const int32_t b = is_kept ? -1 : a;   // a kept lane ends the rows on either side of it
    if (is_kept) w = 0;
    const int32_t before = __shfl_up(b, 1);
    const bool head = lane == 0 || before != b;
    const u64 heads = __ballot(head);
    const int mine = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));   // the head of this lane's row: the highest head at or below it
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const u64 other = __shfl_down(w, d);
      const int theirs = __shfl_down(mine, d);
      if (lane + d < 64 && theirs == mine) w += other;
    }
    if (head && b >= 0) atomicAdd(meas + b, w);
  }
  if (lane == 0 && kept >= 0) atomicAdd(meas + kept, kept_sum);
}

__device__ __forceinline__ bool is_small(u64 m, int32_t cl, int64_t min_measure, int fill) { return m < (u64)min_measure && (cl >= 0 || fill); }

__global__ __launch_bounds__(SV_BLOCK) void k_count_small(int64_t F, const int32_t *__restrict__ comp, const int32_t *__restrict__ cls,
                                                         const u64 *__restrict__ meas, int64_t min_measure, int fill, u64 *ctl) {
  uint32_t n_small = 0;
  for (int64_t f = (int64_t)blockIdx.x * SV_BLOCK + threadIdx.x; f < F; f += (int64_t)gridDim.x * SV_BLOCK)
    n_small += (comp[f] == (int32_t)f && is_small(meas[f], cls[f], min_measure, fill)) ? 1u : 0u;
  stat_add_u32(ctl, CT_NSMALL, n_small, (int)(threadIdx.x & 63));
}

// I8, the two passes: the labelled neighbour components of a small component, over the other entries of the entry's run.
// SECOND false: best_m[A] = max (m(B) + 1); SECOND true: best_id[A] = min B over those of that measure.
template <bool SECOND>
__global__ __launch_bounds__(SV_BLOCK) void k_target(const u64 *__restrict__ keys, const int32_t *__restrict__ sf, int64_t N, int64_t V,
                                                    const int32_t *__restrict__ comp, const int32_t *__restrict__ cls, const u64 *__restrict__ meas,
                                                    int64_t min_measure, int fill, u64 *best_m, int32_t *best_id) {
  const int64_t i = (int64_t)blockIdx.x * SV_BLOCK + threadIdx.x;
  if (i >= N) return;
  const u64 k = keys[i];
  if ((int64_t)(k >> 32) == V) return;
  const int32_t f = sf[i], a = comp[f];
  if (!is_small(meas[a], cls[f], min_measure, fill)) return;
  int64_t j = i;
  while (j > 0 && keys[j - 1] == k) --j;
  const u64 want = SECOND ? best_m[a] : 0;
  for (; j < N && keys[j] == k; ++j) {
    if (j == i) continue;
    const int32_t g = sf[j], b = comp[g];
    if (b == a || cls[g] < 0) continue;
    const u64 m1 = meas[b] + 1;
    if (!SECOND) atomicMax(best_m + a, m1);
    else if (m1 == want) atomicMin(best_id + a, b);
  }
}

// I8: a component's pointer, at its first face
__global__ __launch_bounds__(SV_BLOCK) void k_pointers(int64_t F, const int32_t *__restrict__ comp, const int32_t *__restrict__ cls,
                                                      const u64 *__restrict__ meas, const u64 *__restrict__ best_m, const int32_t *__restrict__ best_id,
                                                      int64_t min_measure, int fill, int32_t *__restrict__ ptr) {
  const int64_t f = (int64_t)blockIdx.x * SV_BLOCK + threadIdx.x;
  if (f >= F || comp[f] != (int32_t)f) return;
  int32_t to = (int32_t)f;
  const u64 m = meas[f], bm = best_m[f];
  if (bm != 0 && is_small(m, cls[f], min_measure, fill)) {
    const int32_t t = best_id[f];
    const u64 mt = bm - 1;
    if (cls[f] < 0 || mt > m || (mt == m && t < (int32_t)f)) to = t;
  }
  ptr[f] = to;
}

// I9: every pointer becomes the root of its chain
__global__ __launch_bounds__(SV_BLOCK) void k_jump(int64_t F, const int32_t *__restrict__ comp, int32_t *ptr) {
  const int64_t f = (int64_t)blockIdx.x * SV_BLOCK + threadIdx.x;
  if (f >= F || comp[f] != (int32_t)f) return;
  int32_t r = ld(ptr + f);
  if (r == (int32_t)f) return;
  for (int32_t p = ld(ptr + r); p != r; p = ld(ptr + r)) r = p;
  st(ptr + f, r);
}

__global__ __launch_bounds__(SV_BLOCK) void k_relabel(int64_t F, const int32_t *__restrict__ comp, const int32_t *__restrict__ ptr, int32_t *cls, u64 *ctl) {
  uint32_t n_changed = 0;
  for (int64_t f = (int64_t)blockIdx.x * SV_BLOCK + threadIdx.x; f < F; f += (int64_t)gridDim.x * SV_BLOCK) {
    const int32_t a = comp[f];
    if (a < 0) continue;
    const int32_t r = ptr[a];
    if (r == a) continue;
    const int32_t c = cls[r];   // r's component does not point: no lane writes this word
    if (c != cls[f]) { cls[f] = c; n_changed += 1u; }
  }
  stat_add_u32(ctl, CT_CHANGED, n_changed, (int)(threadIdx.x & 63));
}

// I10: every word of the statistics block
__global__ void k_sieve_stats(const u64 *__restrict__ ctl, SieveHost h, u64 *__restrict__ stats) {
  const int w = (int)threadIdx.x;
  if (w >= GR_SIEVE_STAT_WORDS) return;
  u64 v = 0;
  switch (w) {
    case GR_SIEVE_STAT_ROUNDS: v = h.rounds; break;
    case GR_SIEVE_STAT_COMPONENTS_BEFORE: v = ctl[CT_BEFORE]; break;
    case GR_SIEVE_STAT_COMPONENTS_AFTER: v = ctl[CT_NCOMP]; break;
    case GR_SIEVE_STAT_FACES_CHANGED: v = h.faces_changed; break;
    case GR_SIEVE_STAT_SMALL_LEFT: v = ctl[CT_NSMALL]; break;
    case GR_SIEVE_STAT_DEGENERATE: v = ctl[CT_DEGEN]; break;
    case GR_SIEVE_STAT_FAN_EDGES: v = ctl[CT_MULTI]; break;
    case GR_SIEVE_STAT_ROUND_CAP: v = h.cap; break;
    case GR_SIEVE_STAT_BAD_FACES: v = ctl[CT_BAD]; break;
    default: break;
  }
  stats[w] = v;
}

inline unsigned grid_of(int64_t n) { return (unsigned)ceil_div(n > 0 ? n : 1, SV_BLOCK); }
inline unsigned count_grid_of(int64_t n) { return std::min(grid_of(n), (unsigned)SV_COUNT_GROUPS); }

inline bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && na && nb && a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

extern "C" {

int gr_face_sieve(gr_ctx *c, const gr_face_sieve_args *args_h) {
  if (!c) return GR_EINVAL;
  if (!args_h) return fail(c, GR_EINVAL, "gr_face_sieve: null descriptor");
  const gr_face_sieve_args g = *args_h;   // read once, here
  const int64_t F = g.F, V = g.V;
  if (F < 0 || V < 0 || F >= SV_MAX || V >= SV_MAX || 3 * F > SV_MAX)
    return fail(c, GR_EINVAL, "gr_face_sieve: F=%lld, V=%lld: each in [0, 2^31 - 1), and 3 F <= 2^31 - 1", (long long)F, (long long)V);
  if (g.min_measure < 0 || g.max_rounds < 1)
    return fail(c, GR_EINVAL, "gr_face_sieve: min_measure=%lld, max_rounds=%d: min_measure >= 0 and max_rounds >= 1", (long long)g.min_measure,
                (int)g.max_rounds);
  if (!g.stats || (F > 0 && (!g.faces || !g.face_class || !g.class_out || !g.comp)) || (V > 0 && g.has_canon && !g.vertex_canon))
    return fail(c, GR_EINVAL, "gr_face_sieve: null arrays");
  const int32_t *canon = g.has_canon ? g.vertex_canon : nullptr;
  const size_t fb = sizeof(int32_t) * (size_t)F;
  const struct { const void *p; size_t n; const char *name; } ins[] = {
      {g.faces, 3 * fb, "faces"}, {g.face_class, fb, "face_class"}, {g.weights, 2 * fb, "weights"}, {canon, sizeof(int32_t) * (size_t)V, "vertex_canon"}};
  const struct { const void *p; size_t n; const char *name; } outs[] = {
      {g.class_out, fb, "class_out"}, {g.comp, fb, "comp"}, {g.stats, sizeof(uint64_t) * GR_SIEVE_STAT_WORDS, "stats"}};
  for (const auto &o : outs) {
    for (const auto &i : ins)
      if (overlaps(o.p, o.n, i.p, i.n) && !(o.p == (const void *)g.class_out && i.p == (const void *)g.face_class && o.p == i.p))
        return fail(c, GR_EINVAL, "gr_face_sieve: %s overlaps %s (class_out == face_class is the one overlap allowed)", o.name, i.name);
    for (const auto &q : outs)
      if (&q != &o && overlaps(o.p, o.n, q.p, q.n)) return fail(c, GR_EINVAL, "gr_face_sieve: %s overlaps %s", o.name, q.name);
  }
  hipStream_t s = (hipStream_t)g.stream;
  GR_HIP(c, hipSetDevice(c->device));

  const int64_t N = 3 * F;
  Plan p;
  const auto o_ctl = p.array<u64>(CT_WORDS);
  const auto o_live = p.array<uint8_t>(F);
  const auto o_skeys = p.array<u64>(N);
  const auto o_sf = p.array<int32_t>(N);
  const size_t mark = p.mark();   // the unsorted keys are dead once sorted: the arrays of the rounds lie over them
  const auto o_keys = p.array<u64>(N);
  const auto o_vals = p.array<int32_t>(N);
  p.rewind(mark);
  const auto o_parent = p.array<int32_t>(F), o_best_id = p.array<int32_t>(F), o_ptr = p.array<int32_t>(F);
  const auto o_meas = p.array<u64>(F), o_best_m = p.array<u64>(F);
  const SortPairs<u64, int32_t> sort(c, p, N, 32 + bit_length(V));
  GR_TRY(stage_acquire(c, c->stage, p.finish(), s, "face-sieve"));
  p.base = c->stage.ptr;
  u64 *ctl = o_ctl(), *skeys = o_skeys(), *meas = o_meas(), *best_m = o_best_m();
  int32_t *sf = o_sf(), *parent = o_parent(), *best_id = o_best_id(), *ptr = o_ptr();
  uint8_t *live = o_live();
  const dim3 block(SV_BLOCK), grid_f(grid_of(F)), grid_n(grid_of(N)), count_f(count_grid_of(F)), count_n(count_grid_of(N));
  const dim3 grid_m((unsigned)ceil_div(F > 0 ? F : 1, (int64_t)64 * SV_MEASURE_CHUNKS * (SV_BLOCK / 64)));
  const int fill = g.fill_unlabelled ? 1 : 0;

  GR_HIP(c, hipMemsetAsync(ctl, 0, sizeof(u64) * CT_WORDS, s));
  SieveHost h = {0, 0, 0};
  if (F > 0) {
    // adjacency, once
    hipLaunchKernelGGL(k_sieve_keys, count_f, block, 0, s, g.faces, canon, F, V, g.face_class, g.class_out, o_keys(), o_vals(), live, ctl);
    GR_HIP(c, hipGetLastError());
    GR_TRY(sort.run(o_keys(), skeys, o_vals(), sf, s));
    hipLaunchKernelGGL(k_sieve_fans, count_n, block, 0, s, (const u64 *)skeys, N, V, ctl);
    GR_HIP(c, hipGetLastError());
    for (int round = 0;; ++round) {
      // I4, I5 of the current labelling
      GR_HIP(c, hipMemsetAsync(ctl + CT_CHANGED, 0, sizeof(u64) * 3, s));   // CT_CHANGED, CT_NCOMP, CT_NSMALL
      hipLaunchKernelGGL(k_round_init, grid_f, block, 0, s, F, parent, meas, best_m, best_id);
      hipLaunchKernelGGL(k_cc_hook, grid_n, block, 0, s, (const u64 *)skeys, (const int32_t *)sf, N, V, (const int32_t *)g.class_out, parent);
      hipLaunchKernelGGL(k_cc_compress, count_f, block, 0, s, F, (const int32_t *)parent, (const uint8_t *)live, g.comp, ctl);
      hipLaunchKernelGGL(k_measure, grid_m, block, 0, s, F, (const int32_t *)g.comp, g.weights, meas);
      hipLaunchKernelGGL(k_count_small, count_f, block, 0, s, F, (const int32_t *)g.comp, (const int32_t *)g.class_out, (const u64 *)meas,
                         g.min_measure, fill, ctl);
      GR_HIP(c, hipGetLastError());
      if (round == 0) GR_HIP(c, hipMemcpyAsync(ctl + CT_BEFORE, ctl + CT_NCOMP, sizeof(u64), hipMemcpyDeviceToDevice, s));
      if (g.min_measure == 0 || round == g.max_rounds) break;
      // I8, I9
      hipLaunchKernelGGL((k_target<false>), grid_n, block, 0, s, (const u64 *)skeys, (const int32_t *)sf, N, V, (const int32_t *)g.comp,
                         (const int32_t *)g.class_out, (const u64 *)meas, g.min_measure, fill, best_m, best_id);
      hipLaunchKernelGGL((k_target<true>), grid_n, block, 0, s, (const u64 *)skeys, (const int32_t *)sf, N, V, (const int32_t *)g.comp,
                         (const int32_t *)g.class_out, (const u64 *)meas, g.min_measure, fill, best_m, best_id);
      hipLaunchKernelGGL(k_pointers, grid_f, block, 0, s, F, (const int32_t *)g.comp, (const int32_t *)g.class_out, (const u64 *)meas,
                         (const u64 *)best_m, (const int32_t *)best_id, g.min_measure, fill, ptr);
      hipLaunchKernelGGL(k_jump, grid_f, block, 0, s, F, (const int32_t *)g.comp, ptr);
      hipLaunchKernelGGL(k_relabel, count_f, block, 0, s, F, (const int32_t *)g.comp, (const int32_t *)ptr, g.class_out, ctl);
      GR_HIP(c, hipGetLastError());
      u64 changed = 0;
      GR_HIP(c, hipMemcpyAsync(&changed, ctl + CT_CHANGED, sizeof(changed), hipMemcpyDeviceToHost, s));
      GR_HIP(c, hipStreamSynchronize(s));   // the one wait of a round
      if (changed == 0) break;              // nothing pointed: comp and the counts are those of the final labelling
      h.rounds += 1;
      h.faces_changed += changed;
      if (round + 1 == g.max_rounds) h.cap = 1;
    }
  }
  hipLaunchKernelGGL(k_sieve_stats, dim3(1), dim3(64), 0, s, (const u64 *)ctl, h, (u64 *)g.stats);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

}  // extern "C"
