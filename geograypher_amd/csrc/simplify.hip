// geograypher_amd/csrc/simplify.hip -- gr_simplify_rings: exact Douglas-Peucker on the rings of a ring table (DESIGN.md section 8q,
// S1-S10).  Integers only, on the 1e-6 m grid; the same result on every run.
//
// Level-synchronous: no recursion, no stack.  Every ring is rotated so that its first anchor (S2) stands at the ring's first
// position; in that order a chain is an interval (lo, hi) of positions whose ends are kept, hi = the ring's end standing for the
// first anchor again.  Every vertex that is neither kept nor dropped is OPEN and knows its chain's ends.  A pass settles, for all
// open chains at once, the farthest interior vertex (S3, S4): every open vertex forms the three 64-bit limbs of w once
// (k_simp_round<0>), and five rounds of 64-bit atomicMax on the chain's words -- high, middle, low limb, then the tie-break
// (smallest x, smallest y, lowest source index) in two words -- leave one contender.  Lanes of a wave that share a chain reduce
// first (seg_max_u64): a chain costs one atomic per wave and round, and the first pass over a ring of a million vertices, ONE chain,
// runs on every compute unit.  The winner compares w with T^2 L2 and publishes the split or the chain's end (k_simp_publish); every
// open vertex then takes its new chain end or is dropped (k_simp_apply), and the host reads ONE word, the vertices still open.
// Passes repeat until none is: O(log n) of them on ordinary outlines, n - 1 at worst; each pass closes or splits every open chain.
// Then the kept vertices of every ring are counted and their doubled area is summed exactly (S6; 32-bit pieces in 64-bit words),
// collapsed rings are emptied, and the flags are compacted in input order (FlagScan of compact_dev.hpp).
#include "compact_dev.hpp"
#include "cub_steps.hpp"
#include "geom_dev.hpp"
#include "gr_internal.hpp"

using namespace grimpl;

namespace {

typedef unsigned long long u64;
typedef unsigned __int128 u128;

// (polygons.hip keeps its own copy of these three for k_points_in_region)
struct U256 { uint64_t w[4]; };   // little-endian limbs

// the full product of two unsigned 128-bit numbers, from 64-bit limbs
__device__ __forceinline__ U256 mul_128x128(u128 a, u128 b) {
  const uint64_t a0 = (uint64_t)a, a1 = (uint64_t)(a >> 64), b0 = (uint64_t)b, b1 = (uint64_t)(b >> 64);
  U256 r;
  r.w[0] = a0 * b0;
  u128 acc = (u128)__umul64hi(a0, b0) + (u128)(a0 * b1) + (u128)(a1 * b0);
  r.w[1] = (uint64_t)acc;
  acc = (acc >> 64) + (u128)__umul64hi(a0, b1) + (u128)__umul64hi(a1, b0) + (u128)(a1 * b1);
  r.w[2] = (uint64_t)acc;
  r.w[3] = (uint64_t)(acc >> 64) + __umul64hi(a1, b1);
  return r;
}
__device__ __forceinline__ bool le_256(const U256 &a, const U256 &b) {
  if (a.w[3] != b.w[3]) return a.w[3] < b.w[3];
  if (a.w[2] != b.w[2]) return a.w[2] < b.w[2];
  if (a.w[1] != b.w[1]) return a.w[1] < b.w[1];
  return a.w[0] <= b.w[0];
}

enum { SIMP_OPEN = 0, SIMP_KEPT = 1, SIMP_DROPPED = 2 };   // a position's state
enum { SIMP_ROUNDS = 5 };                                  // words of a chain's contest: w's limbs from the top, tie-break a, b
enum { SIMP_RING_WORDS = 5 };                              // per ring: kept vertices, then the doubled area in four 32-bit pieces
#define SIMP_IDX_MAX 0x7FFFFFFFll

// Segmented reductions over a wave whose lanes with equal keys stand side by side (a chain's open vertices, a ring's positions):
// an inclusive scan that stops at key changes; the LAST lane of every run (seg_tail) ends with the run's result.  Lanes that take
// no part carry the key -1 and a neutral value.  Called by all 64 lanes.
__device__ __forceinline__ bool seg_tail(int key, int lane) {
  const int next = __shfl_down(key, 1);
  return lane == 63 || next != key;
}
__device__ __forceinline__ u64 seg_max_u64(u64 v, int key, int lane) {
  for (int off = 1; off < 64; off <<= 1) {
    const u64 o = (u64)__shfl_up((long long)v, off);
    const int ok = __shfl_up(key, off);
    if (lane >= off && ok == key && o > v) v = o;
  }
  return v;
}
__device__ __forceinline__ u64 seg_sum_u64(u64 v, int key, int lane) {
  for (int off = 1; off < 64; off <<= 1) {
    const u64 o = (u64)__shfl_up((long long)v, off);
    const int ok = __shfl_up(key, off);
    if (lane >= off && ok == key) v += o;
  }
  return v;
}
// the chain's (or ring's) word takes the run's maximum: one atomic per run
__device__ __forceinline__ void seg_atomic_max(u64 *words, u64 v, int key, bool active, int lane) {
  const u64 m = seg_max_u64(active ? v : 0ull, active ? key : -1, lane);
  if (seg_tail(active ? key : -1, lane) && active) atomicMax(&words[key], m);
}

// The tie-break of S2 and S4 as two words whose MAXIMUM is the lexicographically smallest (x, y), then the lowest index:
// xi = 2^41 - x and yi = 2^41 - y lie in [0, 2^42]; a = xi << 21 | yi >> 22, b = (yi's low 22 bits) << 31 | (2^31 - 1 - index).
__device__ __forceinline__ u64 tie_a(int64_t x, int64_t y) {
  const u64 xi = (u64)(((int64_t)1 << 41) - x), yi = (u64)(((int64_t)1 << 41) - y);
  return xi << 21 | yi >> 22;
}
__device__ __forceinline__ u64 tie_b(int64_t y, int64_t index) {
  const u64 yi = (u64)(((int64_t)1 << 41) - y);
  return (yi & 0x3FFFFFull) << 31 | (u64)(SIMP_IDX_MAX - index);
}

// ring r's positions [s, e), clamped into [0, N]; false when it has fewer than 3 (S6: such a ring comes out empty)
__device__ __forceinline__ bool simp_ring(const int64_t *__restrict__ roff, int r, int64_t N, int64_t &s, int64_t &e) {
  const int64_t n = ring_span(roff, r, N, s);
  e = s + n;
  return n >= 3;
}

// ring [N] = the ring of vertex i, -1 when it is in none or in one of fewer than 3 vertices.  First anchor search (S2): ffx [R]
// takes 2^31 - 1 - (lowest fixed index), 0 when the ring has no fixed vertex; akey [2 R] word 0 takes the best tie_a.
__global__ __launch_bounds__(256) void k_simp_rings(const int64_t *__restrict__ rv, int64_t N, const int64_t *__restrict__ roff, int R,
                                                    const uint8_t *__restrict__ fixed, int32_t *__restrict__ ring,
                                                    u64 *__restrict__ ffx, u64 *__restrict__ akey) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int r = -1;
  bool fix = false;
  u64 ka = 0;
  if (i < N) {
    const int lo = (int)ring_of_slot(roff, 0, R, i);   // the last ring whose offset is <= i
    int64_t s, e;
    if (simp_ring(roff, lo, N, s, e) && i >= s && i < e) r = lo;
    ring[i] = r;
    if (r >= 0) {
      fix = fixed && fixed[i];
      ka = tie_a(rv[i * 2], rv[i * 2 + 1]);
    }
  }
  seg_atomic_max(akey, ka, 2 * r, r >= 0, lane);
  seg_atomic_max(ffx, (u64)(SIMP_IDX_MAX - i), r, fix, lane);
}
// second word of the anchor search: the best tie_b among the vertices that hold the best tie_a
__global__ __launch_bounds__(256) void k_simp_anchor_low(const int64_t *__restrict__ rv, int64_t N, const int32_t *__restrict__ ring,
                                                         u64 *__restrict__ akey) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int r = -1;
  bool act = false;
  u64 kb = 0;
  if (i < N) {
    r = ring[i];
    if (r >= 0 && tie_a(rv[i * 2], rv[i * 2 + 1]) == akey[2 * r]) { act = true; kb = tie_b(rv[i * 2 + 1], i); }
  }
  seg_atomic_max(akey, kb, 2 * r + 1, act, lane);
}

// The rotated order: vertex i of ring [s, e) goes to position s + (i - f) mod n, f the ring's first anchor.  P [N][2], src [N]
// (position -> vertex), state (pre-set to SIMP_DROPPED by the caller: a position no vertex takes stays out), and the marks of the
// two running maxima that give every position its nearest anchor on either side: m_lo [j] = j at an anchor, m_hi [N - 1 - j] =
// N - j at an anchor, 0 elsewhere.  A vertex outside every ring keeps its place and counts as a mark.
__global__ __launch_bounds__(256) void k_simp_rotate(const int64_t *__restrict__ rv, int64_t N, const int64_t *__restrict__ roff,
                                                     const uint8_t *__restrict__ fixed, const int32_t *__restrict__ ring,
                                                     const u64 *__restrict__ ffx, const u64 *__restrict__ akey,
                                                     int64_t *__restrict__ P, int32_t *__restrict__ src, uint8_t *__restrict__ state,
                                                     int32_t *__restrict__ m_lo, int32_t *__restrict__ m_hi) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int r = ring[i];
  int64_t dst = i;
  bool anchor = true;
  if (r >= 0) {
    int64_t s, e;
    (void)simp_ring(roff, r, N, s, e);
    const u64 ff = ffx[r];
    int64_t f = SIMP_IDX_MAX - (int64_t)(ff ? ff : (akey[2 * r + 1] & 0x7FFFFFFFull));
    if (f < s || f >= e) f = s;
    dst = s + (i >= f ? i - f : i - f + (e - s));
    anchor = ff ? fixed[i] != 0 : i == f;
    state[dst] = anchor ? SIMP_KEPT : SIMP_OPEN;
  }
  P[dst * 2] = rv[i * 2]; P[dst * 2 + 1] = rv[i * 2 + 1];
  src[dst] = (int32_t)i;
  m_lo[dst] = anchor ? (int32_t)dst : 0;
  m_hi[N - 1 - dst] = anchor ? (int32_t)(N - dst) : 0;
}

// s_lo, s_hi: the running maxima of the marks.  An open position takes its chain (lo, hi), an anchor the end of the chain it
// heads (nxt), everything clamped into the ring; *open counts the open positions.
__global__ __launch_bounds__(256) void k_simp_chains(int64_t N, const int64_t *__restrict__ roff, const int32_t *__restrict__ ring,
                                                     const int32_t *__restrict__ s_lo, const int32_t *__restrict__ s_hi,
                                                     uint8_t *__restrict__ state, int32_t *__restrict__ lo, int32_t *__restrict__ hi,
                                                     int32_t *__restrict__ nxt, u64 *__restrict__ open) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool is_open = false;
  if (j < N) {
    const int r = ring[j];
    if (r < 0) {
      state[j] = SIMP_DROPPED;
    } else {
      int64_t s, e;
      (void)simp_ring(roff, r, N, s, e);
      const int st = state[j];
      if (st == SIMP_OPEN) {
        lo[j] = (int32_t)min(max((int64_t)s_lo[j], s), j);
        hi[j] = (int32_t)min(max(N - (int64_t)s_hi[N - 1 - j], j), e);
        is_open = true;
      } else if (st == SIMP_KEPT) {
        nxt[j] = (int32_t)(j + 1 < e ? min(max(N - (int64_t)s_hi[N - 2 - j], j + 1), e) : e);
      }
    }
  }
  stat_count(open, 0, is_open, lane);
}

struct SimpPass {
  int64_t N;
  const int64_t *P;          // [N][2] positions in rotated order
  const int32_t *src;        // [N] position -> vertex
  const int64_t *roff;
  const int32_t *ring;
  uint8_t *state, *contend;  // [N]
  int32_t *lo, *hi, *nxt, *win;   // [N]; win [lo]: the chain's split position or -1
  u64 *W;                    // [N][3] the limbs of w of the open positions, low limb first
  u64 *best;                 // [SIMP_ROUNDS][N] the contest words of the chain headed by a position
  u64 *open;                 // [1]
  u64 *stats;
  u64 t2_lo, t2_hi;          // T^2
};

// the position that stands at chain end h: the ring's end means its first position
__device__ __forceinline__ int64_t simp_end(const SimpPass &a, int64_t j, int64_t h) {
  int64_t s, e;
  (void)simp_ring(a.roff, a.ring[j], a.N, s, e);
  return h >= e ? s : h;
}

// S3 for position j of chain (lo, hi): w's limbs, L2; true when the foot lies strictly inside the chord (the squared cross product)
__device__ __forceinline__ bool simp_w(const SimpPass &a, int64_t j, U256 &w, u128 &L2) {
  const int64_t ia = a.lo[j], ib = simp_end(a, j, a.hi[j]);
  const int64_t ax = a.P[ia * 2], ay = a.P[ia * 2 + 1], bx = a.P[ib * 2], by = a.P[ib * 2 + 1];
  const int64_t px = a.P[j * 2], py = a.P[j * 2 + 1];
  const int64_t ex = bx - ax, ey = by - ay, ux = px - ax, uy = py - ay;   // |.| <= 2^41: products below 2^83
  const i128 l2 = (i128)ex * ex + (i128)ey * ey, t = (i128)ux * ex + (i128)uy * ey;
  L2 = (u128)l2;
  const u128 du = (u128)((i128)ux * ux + (i128)uy * uy);
  if (l2 == 0) {
    w.w[0] = (uint64_t)du; w.w[1] = (uint64_t)(du >> 64); w.w[2] = 0; w.w[3] = 0;
    return false;
  }
  if (t <= 0) { w = mul_128x128(du, L2); return false; }
  if (t >= l2) {
    const int64_t vx = px - bx, vy = py - by;
    w = mul_128x128((u128)((i128)vx * vx + (i128)vy * vy), L2);
    return false;
  }
  const i128 c = (i128)ex * uy - (i128)ey * ux;
  const u128 m = (u128)(c < 0 ? -c : c);
  w = mul_128x128(m, m);
  return true;
}

// this position's word of round `round`
__device__ __forceinline__ u64 simp_key(const SimpPass &a, int64_t j, int round) {
  if (round < 3) return a.W[j * 3 + (2 - round)];
  if (round == 3) return tie_a(a.P[j * 2], a.P[j * 2 + 1]);
  return tie_b(a.P[j * 2 + 1], a.src[j]);
}

// One round of the contest.  Round 0: every open position forms w and enters; round k > 0: a contender stays when its word of
// round k - 1 is its chain's best.  Those in put their word of this round to the chain's.
template <int ROUND>
__global__ __launch_bounds__(256) void k_simp_round(SimpPass a) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool act = j < a.N && a.state[j] == SIMP_OPEN, wide = false;
  int head = -1;
  u64 k = 0;
  if (act) {
    head = a.lo[j];
    if (ROUND == 0) {
      U256 w;
      u128 L2;
      wide = simp_w(a, j, w, L2);
      a.W[j * 3] = w.w[0]; a.W[j * 3 + 1] = w.w[1]; a.W[j * 3 + 2] = w.w[2];
      k = w.w[2];
    } else {
      act = a.contend[j] && simp_key(a, j, ROUND - 1) == a.best[(int64_t)(ROUND - 1) * a.N + head];
      if (act) k = simp_key(a, j, ROUND);
    }
    a.contend[j] = act ? 1 : 0;
  }
  seg_atomic_max(a.best + (int64_t)ROUND * a.N, k, head, act, lane);
  if (ROUND == 0) stat_count(a.stats, GR_SIMPLIFY_STAT_WIDE, wide, lane);
}

// The one contender left in every chain decides (S4): w > T^2 L2 (w > T^2 on a chord of no length) keeps it -- win [lo] = its
// position, and the two chains it parts get their ends -- else the chain ends: win [lo] = -1.
__global__ __launch_bounds__(256) void k_simp_publish(SimpPass a) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j == 0) *a.open = 0;   // (the host has read the last pass's count)
  if (j >= a.N || a.state[j] != SIMP_OPEN || !a.contend[j]) return;
  const int head = a.lo[j];
  if (simp_key(a, j, SIMP_ROUNDS - 1) != a.best[(int64_t)(SIMP_ROUNDS - 1) * a.N + head]) return;
  U256 w, bound;
  u128 L2;
  (void)simp_w(a, j, w, L2);
  const u128 T2 = (u128)a.t2_hi << 64 | a.t2_lo;
  if (L2 == 0) { bound.w[0] = a.t2_lo; bound.w[1] = a.t2_hi; bound.w[2] = 0; bound.w[3] = 0; }
  else bound = mul_128x128(T2, L2);
  const bool keep = !le_256(w, bound);
  a.win[head] = keep ? (int32_t)j : -1;
  if (keep) { a.nxt[j] = a.hi[j]; a.nxt[head] = (int32_t)j; }
}

// Every open position reads its chain's outcome: dropped with the chain, kept as the split, or open in one of the two new chains.
// The kept one clears the contest words of both chains for the next pass.  *open counts the positions that stay open.
__global__ __launch_bounds__(256) void k_simp_apply(SimpPass a) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool still = false;
  if (j < a.N && a.state[j] == SIMP_OPEN) {
    const int head = a.lo[j];
    const int v = a.win[head];
    if (v < 0) {
      a.state[j] = SIMP_DROPPED;
    } else if (v == j) {
      a.state[j] = SIMP_KEPT;
      for (int k = 0; k < SIMP_ROUNDS; ++k) { a.best[(int64_t)k * a.N + head] = 0; a.best[(int64_t)k * a.N + j] = 0; }
    } else {
      if (j < v) a.hi[j] = v; else a.lo[j] = v;
      still = true;
    }
  }
  stat_count(a.open, 0, still, lane);
}

// S6: racc [R][SIMP_RING_WORDS]: the kept positions of every ring and the sum of cross(p - o, next - o) over them, o the ring's
// first anchor, `next` the next kept position: the doubled signed area, |term| < 2^84, at most 2^31 terms.  The 128 bits of a term
// (two's complement) go as four 32-bit pieces into four 64-bit sums, which cannot overflow; their weighted sum modulo 2^128 is exact.
__global__ __launch_bounds__(256) void k_simp_ring_sums(SimpPass a, u64 *__restrict__ racc) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int r = -1;
  u64 part[SIMP_RING_WORDS] = {0, 0, 0, 0, 0};
  if (j < a.N) {
    r = a.ring[j];
    if (r >= 0 && a.state[j] == SIMP_KEPT) {
      int64_t s, e;
      (void)simp_ring(a.roff, r, a.N, s, e);
      const int64_t nx = a.nxt[j], in = (nx >= e || nx < s) ? s : nx;
      const int64_t ox = a.P[s * 2], oy = a.P[s * 2 + 1];
      const int64_t px = a.P[j * 2] - ox, py = a.P[j * 2 + 1] - oy, qx = a.P[in * 2] - ox, qy = a.P[in * 2 + 1] - oy;
      const u128 term = (u128)((i128)px * qy - (i128)py * qx);
      part[0] = 1;
      part[1] = (u64)(term & 0xFFFFFFFFull); part[2] = (u64)((term >> 32) & 0xFFFFFFFFull);
      part[3] = (u64)((term >> 64) & 0xFFFFFFFFull); part[4] = (u64)((term >> 96) & 0xFFFFFFFFull);
    }
  }
  const bool tail = seg_tail(r, lane);
#pragma unroll
  for (int k = 0; k < SIMP_RING_WORDS; ++k) {
    const u64 sum = seg_sum_u64(part[k], r, lane);
    if (tail && r >= 0 && sum) atomicAdd(&racc[(int64_t)r * SIMP_RING_WORDS + k], sum);
  }
}

// a ring collapses when fewer than 3 of its vertices are kept or what is kept has no area
__device__ __forceinline__ bool simp_collapsed(const u64 *__restrict__ racc, int r) {
  const u64 *w = racc + (int64_t)r * SIMP_RING_WORDS;
  const u128 area = (u128)w[1] + ((u128)w[2] << 32) + ((u128)w[3] << 64) + ((u128)w[4] << 96);
  return w[0] < 3 || area == 0;
}

// flag [N] (zeroed by the caller), in INPUT order: 1 where the vertex is kept and its ring did not collapse.  Thread t also takes
// ring t's statistics.
__global__ __launch_bounds__(256) void k_simp_flags(SimpPass a, int R, const u64 *__restrict__ racc, int32_t *__restrict__ flag) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < a.N) {
    const int r = a.ring[t];
    const uint32_t i = (uint32_t)a.src[t];
    if (r >= 0 && a.state[t] == SIMP_KEPT && !simp_collapsed(racc, r) && i < (uint64_t)a.N) flag[i] = 1;
  }
  bool collapsed = false, small = false;
  if (t < R) {
    int64_t s, e;
    small = !simp_ring(a.roff, (int)t, a.N, s, e);
    collapsed = !small && simp_collapsed(racc, (int)t);
  }
  stat_count(a.stats, GR_SIMPLIFY_STAT_COLLAPSED, collapsed, lane);
  stat_count(a.stats, GR_SIMPLIFY_STAT_SHORT_RINGS, small, lane);
}

// S7 behind the scan: keep, kept_index (-1 behind the M kept), out_offsets [R + 1], the words kept vertices and passes
__global__ __launch_bounds__(256) void k_simp_write(int64_t N, const int64_t *__restrict__ roff, int64_t R,
                                                    const int32_t *__restrict__ flag, const int32_t *__restrict__ pos,
                                                    uint8_t *__restrict__ keep, int32_t *__restrict__ kept_index,
                                                    int64_t *__restrict__ out_offsets, u64 *__restrict__ stats, u64 passes) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t M = (int64_t)pos[N - 1] + flag[N - 1];
  if (t < N) {
    const int f = flag[t];
    keep[t] = f ? 1 : 0;
    if (f) kept_index[pos[t]] = (int32_t)t;
    if (t >= M) kept_index[t] = -1;
  }
  if (t <= R) {
    const int64_t o = t < R ? min(max(roff[t], (int64_t)0), N) : N;
    out_offsets[t] = o < N ? (int64_t)pos[o] : M;
  }
  if (t == 0) { stats[GR_SIMPLIFY_STAT_KEPT] = (u64)M; stats[GR_SIMPLIFY_STAT_PASSES] = passes; }
}

}  // namespace

extern "C" {

int gr_simplify_rings(gr_ctx *c, const int64_t *ring_vertices, int64_t N, const int64_t *ring_offsets, int64_t R,
                      const uint8_t *fixed, int64_t tol_steps, uint8_t *keep, int32_t *kept_index, int64_t *out_offsets,
                      uint64_t *stats, void *stream) {
  if (!c) return GR_EINVAL;
  if (N < 0 || R < 0 || N > 0x7FFFFFFFll - 1 || R > 0x7FFFFFFFll - 1)
    return fail(c, GR_EINVAL, "gr_simplify_rings: bad shape N=%lld R=%lld (both below 2^31 - 1)", (long long)N, (long long)R);
  if (tol_steps < 0 || tol_steps >= ((int64_t)1 << 40))
    return fail(c, GR_EINVAL, "gr_simplify_rings: tolerance T=%lld outside [0, 2^40) grid steps", (long long)tol_steps);
  if (!stats || !out_offsets || (R > 0 && !ring_offsets) || (N > 0 && (!ring_vertices || !keep || !kept_index)))
    return fail(c, GR_EINVAL, "gr_simplify_rings: null arrays");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  u64 *st = (u64 *)stats;
  GR_HIP(c, hipMemsetAsync(st, 0, sizeof(uint64_t) * GR_SIMPLIFY_STAT_WORDS, s));
  if (N == 0 || R == 0) {   // nothing to keep: every ring comes out empty
    GR_HIP(c, hipMemsetAsync(out_offsets, 0, sizeof(int64_t) * (size_t)(R + 1), s));
    if (N > 0) {
      GR_HIP(c, hipMemsetAsync(keep, 0, (size_t)N, s));
      GR_HIP(c, hipMemsetAsync(kept_index, 0xFF, sizeof(int32_t) * (size_t)N, s));
    }
    if (R > 0) {   // the R rings without a vertex are short rings
      const u64 short_rings = (u64)R;
      GR_HIP(c, hipMemcpyAsync(st + GR_SIMPLIFY_STAT_SHORT_RINGS, &short_rings, sizeof(short_rings), hipMemcpyHostToDevice, s));
      GR_HIP(c, hipStreamSynchronize(s));
    }
    return GR_OK;
  }

  // scratch: open [1] | ffx [R] akey [2 R] racc [5 R] | ring, src, lo, hi, nxt, win [N] | state, contend [N] | P [N][2] | W [N][3] |
  //          best [5][N] | then the marks and their running maxima m_lo, m_hi, s_lo, s_hi [N] -- or, behind the passes, the flags
  //          and their scan
  Plan p;
  const auto o_open = p.array<u64>(1);
  const auto o_rings = p.array<u64>((1 + 2 + SIMP_RING_WORDS) * R);
  const auto o_ring = p.array<int32_t>(N), o_src = p.array<int32_t>(N), o_lo = p.array<int32_t>(N), o_hi = p.array<int32_t>(N);
  const auto o_nxt = p.array<int32_t>(N), o_win = p.array<int32_t>(N);
  const auto o_state = p.array<uint8_t>(N), o_contend = p.array<uint8_t>(N);
  const auto o_P = p.array<int64_t>(2 * N);
  const auto o_W = p.array<u64>(3 * N), o_best = p.array<u64>((int64_t)SIMP_ROUNDS * N);
  const size_t phase = p.mark();
  const auto o_mlo = p.array<int32_t>(N), o_mhi = p.array<int32_t>(N), o_slo = p.array<int32_t>(N), o_shi = p.array<int32_t>(N);
  const InclusiveMax<int32_t> nearest(c, p, N);
  p.rewind(phase);
  const FlagScan fs(c, p, N);
  int rc = stage_acquire(c, c->stage, p.finish(), s, "simplify-rings");
  if (rc != GR_OK) return rc;
  p.base = c->stage.ptr;

  u64 *ffx = o_rings(), *akey = ffx + R, *racc = akey + 2 * R;
  const dim3 grid((unsigned)ceil_div(N, 256)), block(256);
  GR_HIP(c, hipMemsetAsync(o_open(), 0, sizeof(u64), s));
  GR_HIP(c, hipMemsetAsync(ffx, 0, sizeof(u64) * (size_t)((1 + 2 + SIMP_RING_WORDS) * R), s));
  GR_HIP(c, hipMemsetAsync(o_state(), SIMP_DROPPED, (size_t)N, s));
  GR_HIP(c, hipMemsetAsync(o_best(), 0, sizeof(u64) * (size_t)SIMP_ROUNDS * (size_t)N, s));
  // S2: rings, anchors, the rotated order, the first chains
  hipLaunchKernelGGL(k_simp_rings, grid, block, 0, s, ring_vertices, N, ring_offsets, (int)R, fixed, o_ring(), ffx, akey);
  hipLaunchKernelGGL(k_simp_anchor_low, grid, block, 0, s, ring_vertices, N, (const int32_t *)o_ring(), akey);
  hipLaunchKernelGGL(k_simp_rotate, grid, block, 0, s, ring_vertices, N, ring_offsets, fixed, (const int32_t *)o_ring(),
                     (const u64 *)ffx, (const u64 *)akey, o_P(), o_src(), o_state(), o_mlo(), o_mhi());
  GR_TRY(nearest.run(o_mlo(), o_slo(), s));
  GR_TRY(nearest.run(o_mhi(), o_shi(), s));
  hipLaunchKernelGGL(k_simp_chains, grid, block, 0, s, N, ring_offsets, (const int32_t *)o_ring(), (const int32_t *)o_slo(),
                     (const int32_t *)o_shi(), o_state(), o_lo(), o_hi(), o_nxt(), o_open());
  GR_HIP(c, hipGetLastError());

  SimpPass a;
  a.N = N; a.P = o_P(); a.src = o_src(); a.roff = ring_offsets; a.ring = o_ring(); a.state = o_state(); a.contend = o_contend();
  a.lo = o_lo(); a.hi = o_hi(); a.nxt = o_nxt(); a.win = o_win(); a.W = o_W(); a.best = o_best(); a.open = o_open(); a.stats = st;
  const u128 T2 = (u128)(uint64_t)tol_steps * (u128)(uint64_t)tol_steps;
  a.t2_lo = (u64)T2; a.t2_hi = (u64)(T2 >> 64);

  // S3, S4: passes until no position is open; every pass drops or splits every open chain, so there are at most N of them
  u64 open_h = 0;
  int64_t passes = 0;
  GR_HIP(c, hipMemcpyAsync(&open_h, o_open(), sizeof(open_h), hipMemcpyDeviceToHost, s));
  GR_HIP(c, hipStreamSynchronize(s));
  while (open_h > 0) {
    if (passes >= N) return fail(c, GR_EHIP, "gr_simplify_rings: %lld positions still open after %lld passes", (long long)open_h, (long long)passes);
    hipLaunchKernelGGL(k_simp_round<0>, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_simp_round<1>, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_simp_round<2>, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_simp_round<3>, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_simp_round<4>, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_simp_publish, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_simp_apply, grid, block, 0, s, a);
    GR_HIP(c, hipGetLastError());
    ++passes;
    GR_HIP(c, hipMemcpyAsync(&open_h, o_open(), sizeof(open_h), hipMemcpyDeviceToHost, s));
    GR_HIP(c, hipStreamSynchronize(s));
  }

  // S6, S7 (the flags overlay the marks, which are done with)
  GR_HIP(c, hipMemsetAsync(fs.flag(), 0, sizeof(int32_t) * (size_t)N, s));
  hipLaunchKernelGGL(k_simp_ring_sums, grid, block, 0, s, a, racc);
  hipLaunchKernelGGL(k_simp_flags, dim3((unsigned)ceil_div(std::max(N, R), 256)), block, 0, s, a, (int)R, (const u64 *)racc, fs.flag());
  GR_TRY(fs.scan.run(fs.flag(), fs.pos(), s));
  hipLaunchKernelGGL(k_simp_write, dim3((unsigned)ceil_div(std::max(N, R + 1), 256)), block, 0, s, N, ring_offsets, R,
                     (const int32_t *)fs.flag(), (const int32_t *)fs.pos(), keep, kept_index, out_offsets, st, (u64)passes);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

}  // extern "C"
