#pragma once
// geograypher_amd/csrc/geom_dev.hpp -- device helpers shared by the polygon, terrain and selection kernels (gfx950, wave64):
// the exact orientation sign, the ring table and its walk (RingTable, ring_span, ring_of_slot, edge_crossing and rule Z3's
// edge_crossing_strict), the checked face load, and the integer wave reductions behind every statistics word (stat_add,
// stat_add_u32, stat_max, stat_count, ring_stats).  HIP only; no floating point.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

typedef __int128 i128;

__device__ __forceinline__ i128 orient(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t cx, int64_t cy) {
  return (i128)(bx - ax) * (i128)(cy - ay) - (i128)(by - ay) * (i128)(cx - ax);   // |coordinates| <= 3 * 2^40: |products| < 2^87
}
__device__ __forceinline__ int sgn(i128 v) { return v > 0 ? 1 : (v < 0 ? -1 : 0); }

// The vertices [i0, i0 + n) of ring r, clamped: a bad offset table reads nothing outside the n_rv vertices.  A ring takes part
// when n >= 3.
__device__ __forceinline__ int64_t ring_span(const int64_t *__restrict__ roff, int r, int64_t n_rv, int64_t &i0) {
  i0 = min(max(roff[r], (int64_t)0), n_rv);
  return min(max(roff[r + 1], i0), n_rv) - i0;
}

// THE even-odd rule of the ring walks (P4 asks the same of 3 x centroid): a ray from (px, py) along +x, edges
// half-open in y -- a b is a candidate when exactly one of its ends has y <= py, so a horizontal edge never counts and a vertex
// on the ray counts for one of its two edges -- and a candidate counts when the point is strictly left of the edge taken
// upwards, by the sign of the 128-bit `orient`.  The point is on the boundary when that determinant is 0 inside the edge's
// closed box (a crossing edge with determinant 0 holds the point in its box).  All six arguments in one unit: a caller whose
// point is 3 x a centre scales the ring vertices by 3.
// Flips `parity` when the edge counts; returns true when BOUNDARY is asked for and the point is on the edge (the parity then
// means nothing).  Without BOUNDARY no box test is made and the determinant is formed for candidates only.
template <bool BOUNDARY>
__device__ __forceinline__ bool edge_crossing(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py, int &parity) {
  const bool cross = (ay > py) != (by > py);
  const bool in_box = BOUNDARY && min(ax, bx) <= px && px <= max(ax, bx) && min(ay, by) <= py && py <= max(ay, by);
  bool on = false;
  if (cross || in_box) {
    const i128 o = orient(ax, ay, bx, by, px, py);
    on = o == 0 && in_box;
    if (cross && (o > 0) == (by > ay)) parity ^= 1;
  }
  return on;
}

// Rule Z3: edge_crossing<false> with ONE difference.  That walk counts a point exactly ON an edge that runs
// downwards (determinant 0 is "not strictly right") and not one on an edge that runs upwards, so a cell centre on a vertical
// edge shared by two rows belongs to both of them or to neither.  Here a candidate counts only when the point is STRICTLY left
// of the edge taken upwards, whichever way the ring runs: the ray along +x meets an edge through the point itself never, a
// centre on a shared edge belongs to exactly one row, and rows that tile a region partition its cells.  Candidates are
// half-open in y exactly as there; the determinant is formed for candidates only.  NARROW: the caller's differences are all
// below 2^26, so the determinant fits int64; otherwise it is the 128-bit `orient`.  Both are exact.
template <bool NARROW = false>
__device__ __forceinline__ void edge_crossing_strict(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py, int &parity) {
  if ((ay > py) != (by > py)) {
    int s;
    if (NARROW) {
      const int64_t o = (bx - ax) * (py - ay) - (by - ay) * (px - ax);
      s = o > 0 ? 1 : (o < 0 ? -1 : 0);
    } else {
      s = sgn(orient(ax, ay, bx, by, px, py));
    }
    if (by > ay ? s > 0 : s < 0) parity ^= 1;
  }
}

// One ring table on the device (A1; Z1 and B1 without hole flags and boxes: both null there).
struct RingTable {
  const int64_t *rv, *roff, *pbox;
  const int32_t *rpoly, *rhole;
  int64_t n_rv, R, P;
};

// The ring that holds vertex slot i among the rings [r_lo, r_hi): the last ring whose first vertex is at or before i (rings of no
// vertex in front of it are passed over); the caller checks that the slot lies inside the span it then reads.
__device__ __forceinline__ int64_t ring_of_slot(const int64_t *__restrict__ roff, int64_t r_lo, int64_t r_hi, int64_t i) {
  int64_t lo = r_lo, hi = r_hi;   // the answer is in [lo, hi); roff[lo] <= i is the caller's
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (roff[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// The three vertex indices of face f; false when one is outside [0, V): such a face is reported, never dereferenced.  V < 2^31
// (every entry point checks it), so the indices are compared as unsigned 32-bit values: a negative one is a large one.
__device__ __forceinline__ bool load_face(const int32_t *__restrict__ faces, int64_t f, int64_t V, int64_t &v0, int64_t &v1,
                                          int64_t &v2) {
  const uint32_t a = (uint32_t)faces[f * 3], b = (uint32_t)faces[f * 3 + 1], c = (uint32_t)faces[f * 3 + 2];
  v0 = a; v1 = b; v2 = c;
  return max(a, max(b, c)) < (uint32_t)V;
}

// Butterflies over the 64 lanes: every lane ends with the result.  Integers, so the order does not matter.
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = (unsigned long long)__shfl_xor((long long)v, off);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off);
  return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {   // for lane values whose sum stays below 2^32
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
  return v;
}

// Statistics: ONE atomic per wave and word, none when the wave has nothing to report.  Called by all 64 lanes.
__device__ __forceinline__ void stat_add(unsigned long long *stats, int word, unsigned long long value, int lane) {
  const unsigned long long s = wave_sum_u64(value);
  if (lane == 0 && s) atomicAdd(&stats[word], s);
}
__device__ __forceinline__ void stat_add_u32(unsigned long long *stats, int word, uint32_t value, int lane) {   // sum < 2^32
  const uint32_t s = wave_sum_u32(value);
  if (lane == 0 && s) atomicAdd(&stats[word], (unsigned long long)s);
}
__device__ __forceinline__ void stat_max(unsigned long long *stats, int word, unsigned long long value, int lane) {
  const unsigned long long m = wave_max_u64(value);
  if (lane == 0 && m) atomicMax(&stats[word], m);
}
// stat_add of a lane's 0 or 1: a ballot and a population count instead of the butterfly
__device__ __forceinline__ void stat_count(unsigned long long *stats, int word, bool one, int lane) {
  const unsigned long long m = __ballot(one);
  if (lane == 0 && m) atomicAdd(&stats[word], (unsigned long long)__popcll(m));
}

// The ring words of a ring table's statistics, one lane per ring r (lanes with r >= R report nothing): the largest ring and the
// rings of fewer than 3 vertices, which take no part.  The two words are the caller's.  Called by all 64 lanes.
template <int LARGEST_RING, int RINGS_IGNORED>
__device__ __forceinline__ void ring_stats(const int64_t *__restrict__ roff, int64_t R, int64_t n_rv, int64_t r,
                                           unsigned long long *stats, int lane) {
  int64_t i0, n = 0;
  if (r < R) n = ring_span(roff, (int)r, n_rv, i0);
  stat_max(stats, LARGEST_RING, (unsigned long long)n, lane);
  stat_count(stats, RINGS_IGNORED, r < R && n < 3, lane);
}

}  // namespace
