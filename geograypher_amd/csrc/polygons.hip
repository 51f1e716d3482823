// geograypher_amd/csrc/polygons.hip -- label_polygons on the device: the weighted area every mesh face contributes to every
// polygon, summed per (polygon, class) (gr_polygon_class_weights; the rule-set is DESIGN.md "Polygon labels"), and the polygon row
// every face CENTRE lies in (gr_face_polygon_index; DESIGN.md "Vector textures"), and the region of interest: which points lie in
// a buffered union of polygon rows (gr_points_in_region) and the sub-mesh of the faces that touch them (gr_submesh_extract), at
// the end of the file; DESIGN.md "Region of interest"; and the outline rings of every class of a per-face labelling
// (gr_class_outlines; DESIGN.md "Class outlines") or of a sparse face x class membership (gr_member_outlines; DESIGN.md
// "Detection footprints"), behind them.  None needs an uploaded mesh: the caller hands over snapped integer
// coordinates.  The pieces the calls share are defined once: the ring span, the even-odd crossing rule, the checked face load and
// the statistics reductions (one integer atomic per wave and word) in geom_dev.hpp, the host's check of a ring table
// (check_ring_table) in front of the entry points.
//
// gr_polygon_class_weights:
// Shape: face-major, one face per lane.  The ring table is walked WAVE-UNIFORMLY: ring r, its polygon, the polygon's box and
// every ring vertex have the same address in all lanes (scalar loads), so the only divergence is the execution mask of the lanes
// whose box misses the polygon's -- and a wave none of whose faces meets the box skips the ring after one ballot.  A face's
// state across the rings of one polygon lives in registers; when the polygon changes the wave sums its lanes per class
// (butterfly, fixed order) and issues ONE f64 atomic per class present: a wave's faces share the polygon, so per-lane
// atomics would all land in one row of `weights`.
//   GR_POLY_WITHIN   exact: 128-bit integer orientation signs on the snapped coordinates decide "closed triangle inside the closed
//                    polygon region" as  no ring edge meets the triangle's open interior  AND  3 x centroid is inside (even-odd)
//   GR_POLY_OVERLAY  f64: the ring streamed vertex by vertex through the triangle's three half-planes (Sutherland-Hodgman with
//                    O(1) state per stage, no per-lane vertex arrays) into a shoelace sum, in coordinates relative to the
//                    triangle's first vertex
#include <functional>

#include "compact_dev.hpp"
#include "cub_steps.hpp"
#include "geom_dev.hpp"
#include "gr_internal.hpp"

using namespace grimpl;

namespace {

struct PolyArgs {   // the scalars of a call; the arrays are kernel parameters of their own, so that they can be __restrict__
  int64_t F;
  int64_t n_rv;
  int R, P, C, mode;
};

// v >= 0 as a double: exact below 2^64 when v has at most 53 significant bits, within an ulp above
__device__ __forceinline__ double to_double(i128 v) {
  const uint64_t hi = (uint64_t)(v >> 64), lo = (uint64_t)v;
  return hi == 0 ? (double)lo : (double)hi * 18446744073709551616.0 + (double)lo;
}

struct Tri {   // counter-clockwise
  int64_t x[3], y[3];
};

// Does the closed segment a b meet the OPEN interior of t?  Signs only.  The line through a, b passes through the interior iff
// it has vertices strictly on both sides; then one vertex p0 is alone on its side (the others weakly opposite), the line's
// chord of the triangle ends on p0's two edges, and a point of the line is inside the open chord iff it is strictly inside both
// of those edges' half-planes (f1, f2 > 0).  A point outside the open chord is behind one end (f1 <= 0) or the other (f2 <= 0):
// the segment meets the chord iff an end point is inside it or the two end points are behind different ends.
__device__ __forceinline__ bool edge_meets_interior(const Tri &t, int64_t ax, int64_t ay, int64_t bx, int64_t by) {
  const int s0 = sgn(orient(ax, ay, bx, by, t.x[0], t.y[0]));
  const int s1 = sgn(orient(ax, ay, bx, by, t.x[1], t.y[1]));
  const int s2 = sgn(orient(ax, ay, bx, by, t.x[2], t.y[2]));
  const int npos = (s0 > 0) + (s1 > 0) + (s2 > 0), nneg = (s0 < 0) + (s1 < 0) + (s2 < 0);
  if (npos == 0 || nneg == 0) return false;
  const int want = npos == 1 ? 1 : -1;
  const int k = s0 == want ? 0 : (s1 == want ? 1 : 2);
  int64_t p0x = t.x[0], p0y = t.y[0], p1x = t.x[1], p1y = t.y[1], p2x = t.x[2], p2y = t.y[2];   // selects, not indexed registers
  if (k == 1) { p0x = t.x[1]; p0y = t.y[1]; p1x = t.x[2]; p1y = t.y[2]; p2x = t.x[0]; p2y = t.y[0]; }
  if (k == 2) { p0x = t.x[2]; p0y = t.y[2]; p1x = t.x[0]; p1y = t.y[0]; p2x = t.x[1]; p2y = t.y[1]; }
  const int f1a = sgn(orient(p0x, p0y, p1x, p1y, ax, ay)), f2a = sgn(orient(p2x, p2y, p0x, p0y, ax, ay));
  const int f1b = sgn(orient(p0x, p0y, p1x, p1y, bx, by)), f2b = sgn(orient(p2x, p2y, p0x, p0y, bx, by));
  return (f1a > 0 && f2a > 0) || (f1b > 0 && f2b > 0) || (f1a <= 0 && f2b <= 0) || (f1b <= 0 && f2a <= 0);
}

// ---- overlay: streamed Sutherland-Hodgman.  Stage K clips against the half-plane left of the triangle's edge K; what it emits
// is put into stage K + 1, stage 3 is the shoelace sum.  Every stage keeps its first and its previous point with their side
// values, nothing else.  Operation order: side d = ex * (y - ay) - ey * (x - ax), inside iff d >= 0; crossing point
// of s -> p: t = ds / (ds - dp), s + t * (p - s); shoelace term of u -> v: ux * vy - vx * uy.
struct Clip {
  double ax, ay, ex, ey;
  double fx, fy, fd, px, py, pd;
  bool has;
};
struct ClipState {
  Clip k[3];
  double ofx, ofy, opx, opy, sum;   // the output ring's first and previous point, the running shoelace sum
  bool ohas;
};

template <int K> __device__ __forceinline__ void clip_put(ClipState &S, double x, double y);

template <int K> __device__ __forceinline__ void clip_edge(ClipState &S, double sx, double sy, double sd, double x, double y, double d) {
  const bool in = d >= 0.0, s_in = sd >= 0.0;
  if (in != s_in) {
    const double t = sd / (sd - d);
    clip_put<K + 1>(S, sx + t * (x - sx), sy + t * (y - sy));
  }
  if (in) clip_put<K + 1>(S, x, y);
}

template <int K> __device__ __forceinline__ void clip_put(ClipState &S, double x, double y) {
  if constexpr (K == 3) {
    if (!S.ohas) { S.ofx = x; S.ofy = y; S.ohas = true; }
    else S.sum += S.opx * y - x * S.opy;
    S.opx = x; S.opy = y;
  } else {
    Clip &k = S.k[K];
    const double d = k.ex * (y - k.ay) - k.ey * (x - k.ax);
    if (!k.has) { k.fx = x; k.fy = y; k.fd = d; k.has = true; }
    else clip_edge<K>(S, k.px, k.py, k.pd, x, y, d);
    k.px = x; k.py = y; k.pd = d;
  }
}

template <int K> __device__ __forceinline__ void clip_close(ClipState &S) {   // the closing edge previous -> first of every stage, in order
  if constexpr (K == 3) {
    if (S.ohas) S.sum += S.opx * S.ofy - S.ofx * S.opy;
  } else {
    Clip &k = S.k[K];
    if (k.has) clip_edge<K>(S, k.px, k.py, k.pd, k.fx, k.fy, k.fd);
    clip_close<K + 1>(S);
  }
}

// butterfly: every lane ends with the same sum, in a fixed order.  For the weights alone (flush_wave); counts are integers (stat_add)
__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Add `val` of the lanes with `has` into row[class], one atomic per class present in the wave.  Called by all 64 lanes.
__device__ __forceinline__ void flush_wave(double val, bool has, int cls, double *row, int lane) {
  unsigned long long m = __ballot(has);
  while (m) {
    const int leader = __ffsll((long long)m) - 1;
    const int cc = __shfl(cls, leader);
    const bool mine = has && cls == cc;
    const double v = wave_sum(mine ? val : 0.0);
    if (lane == leader) atomicAdd(row + cc, v);
    m &= ~__ballot(mine);
  }
}

// tri [F][6] snapped x0 y0 x1 y1 x2 y2; cls [F] (< 0: skip); wgt [F]; rv [n_rv][2] ring vertices; roff [R + 1]; rpoly [R]
// non-decreasing; rhole [R]; pbox [P][4] xmin ymin xmax ymax; weights [P][C]; stats [GR_POLY_STAT_WORDS]
__global__ __launch_bounds__(256) void k_polygon_weights(const int64_t *__restrict__ tri, const int32_t *__restrict__ cls_in,
                                                         const double *__restrict__ wgt, const int64_t *__restrict__ rv,
                                                         const int64_t *__restrict__ roff, const int32_t *__restrict__ rpoly,
                                                         const int32_t *__restrict__ rhole, const int64_t *__restrict__ pbox,
                                                         double *__restrict__ weights, unsigned long long *__restrict__ stats,
                                                         PolyArgs a) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  Tri t = {{0, 0, 0}, {0, 0, 0}};
  int cls = -1;
  double w = 0.0, area_t = 0.0;
  bool live = f < a.F;
  if (live) { cls = cls_in[f]; live = cls >= 0 && cls < a.C; }
  if (live) {
    const int64_t *p = tri + f * 6;
    t.x[0] = p[0]; t.y[0] = p[1]; t.x[1] = p[2]; t.y[1] = p[3]; t.x[2] = p[4]; t.y[2] = p[5];
    i128 o = orient(t.x[0], t.y[0], t.x[1], t.y[1], t.x[2], t.y[2]);
    if (o < 0) { o = -o; const int64_t sx = t.x[1], sy = t.y[1]; t.x[1] = t.x[2]; t.y[1] = t.y[2]; t.x[2] = sx; t.y[2] = sy; }
    live = o != 0;                       // a face the snap collapsed contributes nothing
    area_t = to_double(o) / 2e12;        // square metres: twice the area in 1e-12 m^2, one conversion, one division
    w = wgt[f];
  }
  // a face that takes no part pairs with no polygon (`live` gates in_poly below); its box is a placeholder
  const int64_t xlo = live ? min(t.x[0], min(t.x[1], t.x[2])) : 1, xhi = live ? max(t.x[0], max(t.x[1], t.x[2])) : 0;
  const int64_t ylo = live ? min(t.y[0], min(t.y[1], t.y[2])) : 1, yhi = live ? max(t.y[0], max(t.y[1], t.y[2])) : 0;
  const int64_t c3x = t.x[0] + t.x[1] + t.x[2], c3y = t.y[0] + t.y[1] + t.y[2];
  // overlay frame: metres relative to vertex 0 (the integer differences are exact)
  const double e1x = (double)(t.x[1] - t.x[0]) * 1e-6, e1y = (double)(t.y[1] - t.y[0]) * 1e-6;
  const double e2x = (double)(t.x[2] - t.x[0]) * 1e-6, e2y = (double)(t.y[2] - t.y[0]) * 1e-6;

  int cur = -1;              // polygon of the rings being walked (wave-uniform)
  bool in_poly = false;      // this lane's box overlaps its box
  bool meets = false;        // within: a ring edge met the open interior
  int parity = 0;            // within: crossings right of the centroid
  double acc = 0.0;          // overlay: shoelace sums of the polygon's rings, holes negative
  unsigned long long tested = 0, contributing = 0, largest = 0;

  auto flush = [&]() {
    if (cur < 0 || !__ballot(in_poly)) return;
    double val;
    bool has;
    if (a.mode == GR_POLY_WITHIN) { has = in_poly && !meets && (parity & 1); val = area_t * w; }
    else { const double area = 0.5 * acc; has = in_poly && area > 0.0; val = area * w; }
    contributing += has ? 1 : 0;
    flush_wave(val, has, cls, weights + (int64_t)cur * a.C, lane);
  };

  for (int r = 0; r < a.R; ++r) {
    const int p = rpoly[r];
    if (p != cur) {
      flush();
      cur = (p >= 0 && p < a.P) ? p : -1;
      meets = false; parity = 0; acc = 0.0; in_poly = false;
      if (cur >= 0) {
        const int64_t *b = pbox + (int64_t)cur * 4;
        in_poly = live && xlo <= b[2] && xhi >= b[0] && ylo <= b[3] && yhi >= b[1];
        tested += in_poly ? 1 : 0;
      }
    }
    int64_t i0;
    const int64_t n = ring_span(roff, r, a.n_rv, i0);
    largest = max(largest, (unsigned long long)n);
    if (cur < 0 || n < 3 || !__ballot(in_poly)) continue;
    const int64_t *v = rv + i0 * 2;
    if (!in_poly) continue;
    if (a.mode == GR_POLY_WITHIN) {
      int64_t ax = v[2 * (n - 1)], ay = v[2 * (n - 1) + 1];
      for (int64_t i = 0; i < n; ++i) {
        const int64_t bx = v[2 * i], by = v[2 * i + 1];
        edge_crossing<false>(3 * ax, 3 * ay, 3 * bx, 3 * by, c3x, c3y, parity);   // the centroid is on no edge unless `meets`
        // the edge's box against the face's: an edge that stays at or beyond a side of the box cannot reach the open interior
        if (!meets && max(ax, bx) > xlo && min(ax, bx) < xhi && max(ay, by) > ylo && min(ay, by) < yhi)
          meets = edge_meets_interior(t, ax, ay, bx, by);
        ax = bx; ay = by;
      }
    } else {
      ClipState S;
      S.k[0] = {0.0, 0.0, e1x, e1y, 0, 0, 0, 0, 0, 0, false};
      S.k[1] = {e1x, e1y, e2x - e1x, e2y - e1y, 0, 0, 0, 0, 0, 0, false};
      S.k[2] = {e2x, e2y, 0.0 - e2x, 0.0 - e2y, 0, 0, 0, 0, 0, 0, false};
      S.ofx = S.ofy = S.opx = S.opy = 0.0; S.sum = 0.0; S.ohas = false;
      for (int64_t i = 0; i < n; ++i)
        clip_put<0>(S, (double)(v[2 * i] - t.x[0]) * 1e-6, (double)(v[2 * i + 1] - t.y[0]) * 1e-6);
      clip_close<0>(S);
      acc = rhole[r] ? acc - S.sum : acc + S.sum;
    }
  }
  flush();

  stat_add(stats, GR_POLY_STAT_TESTED, tested, lane);
  stat_add(stats, GR_POLY_STAT_CONTRIBUTING, contributing, lane);
  if (f == 0) atomicMax(&stats[GR_POLY_STAT_LARGEST_RING], largest);   // the same in every lane of every wave: one writer
}

// ---- gr_face_polygon_index: the polygon row each face CENTRE lies in (DESIGN.md "Vector textures", V3-V5) -------------------------
struct FaceIndexArgs {
  int64_t F, V, n_rv, n_cp;
  int64_t gx0, gy0, cw, ch;   // the cell grid, in the 3 q units of the query point
  int R, P, nx, ny;
};

// V4: is (px, py) = 3 x centre in the closed region of row p?  On the boundary of any ring, or an odd parity over all rings
// (edge_crossing).  The rings of a row are consecutive in rpoly (non-decreasing): the first one by binary search.
__device__ __forceinline__ bool row_contains(const int64_t *__restrict__ rv, const int64_t *__restrict__ roff,
                                             const int32_t *__restrict__ rpoly, const FaceIndexArgs &a, int p, int64_t px, int64_t py) {
  int lo = 0, hi = a.R;
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (rpoly[mid] < p) lo = mid + 1; else hi = mid;
  }
  int parity = 0;
  for (int r = lo; r < a.R && rpoly[r] == p; ++r) {
    int64_t i0;
    const int64_t n = ring_span(roff, r, a.n_rv, i0);
    if (n < 3) continue;
    const int64_t *v = rv + i0 * 2;
    int64_t ax = 3 * v[2 * (n - 1)], ay = 3 * v[2 * (n - 1) + 1];
    for (int64_t i = 0; i < n; ++i) {
      const int64_t bx = 3 * v[2 * i], by = 3 * v[2 * i + 1];
      if (edge_crossing<true>(ax, ay, bx, by, px, py, parity)) return true;
      ax = bx; ay = by;
    }
  }
  return parity != 0;
}

// vq [V][2] snapped vertices; faces [F][3]; rv, roff, rpoly, pbox: the ring table; coff [nx ny + 1], cpoly [n_cp]: per cell the rows
// whose box meets it, DESCENDING; out [F]; stats [GR_FPI_STAT_WORDS].  One face per lane; the lane walks the list of ITS cell and
// stops at the first row that contains the centre (V5: the highest row wins).
__global__ __launch_bounds__(256) void k_face_polygon_index(const int64_t *__restrict__ vq, const int32_t *__restrict__ faces,
                                                            const int64_t *__restrict__ rv, const int64_t *__restrict__ roff,
                                                            const int32_t *__restrict__ rpoly, const int64_t *__restrict__ pbox,
                                                            const int64_t *__restrict__ coff, const int32_t *__restrict__ cpoly,
                                                            int32_t *__restrict__ out, unsigned long long *__restrict__ stats,
                                                            FaceIndexArgs a) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned long long tested = 0, longest = 0;
  bool labelled = false, bad = false;
  if (f < a.F) {
    int64_t v0, v1, v2;
    int found = -1;
    bad = !load_face(faces, f, a.V, v0, v1, v2);
    if (!bad) {
      const int64_t px = vq[v0 * 2] + vq[v1 * 2] + vq[v2 * 2], py = vq[v0 * 2 + 1] + vq[v1 * 2 + 1] + vq[v2 * 2 + 1];
      const int64_t dx = px - a.gx0, dy = py - a.gy0;
      const int64_t ix = dx >= 0 ? dx / a.cw : -1, iy = dy >= 0 ? dy / a.ch : -1;
      if (ix >= 0 && ix < a.nx && iy >= 0 && iy < a.ny) {   // a centre outside the grid is in no box
        const int64_t cell = iy * a.nx + ix;
        int64_t j0 = coff[cell], j1 = coff[cell + 1];
        j0 = min(max(j0, (int64_t)0), a.n_cp); j1 = min(max(j1, j0), a.n_cp);
        longest = (unsigned long long)(j1 - j0);
        for (int64_t j = j0; j < j1; ++j) {
          const int p = cpoly[j];
          if (p < 0 || p >= a.P) continue;
          const int64_t *b = pbox + (int64_t)p * 4;
          if (px < 3 * b[0] || px > 3 * b[2] || py < 3 * b[1] || py > 3 * b[3]) continue;
          ++tested;
          if (row_contains(rv, roff, rpoly, a, p, px, py)) { found = p; break; }
        }
      }
    }
    out[f] = found;
    labelled = found >= 0;
  }
  stat_add(stats, GR_FPI_STAT_TESTED, tested, lane);
  stat_count(stats, GR_FPI_STAT_LABELLED, labelled, lane);
  stat_max(stats, GR_FPI_STAT_LONGEST_LIST, longest, lane);
  stat_count(stats, GR_FPI_STAT_BAD_FACES, bad, lane);
}

// ---- gr_points_in_region: is a point in the union of the rows' closed regions, grown by D?  (DESIGN.md "Region of interest", Q3-Q4) ----
typedef unsigned __int128 u128;

struct RegionArgs {
  int64_t N, n_rv, D;
  int R, P;
};

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

#define GR_REGION_FAR ((int64_t)1 << 62)   // bound of the joint box of nothing: stays empty when grown by D < 2^40

// joint [4]: xmin ymin xmax ymax over the rows with a box (xmin <= xmax and ymin <= ymax).  One workgroup.
__global__ __launch_bounds__(256) void k_region_joint_box(const int64_t *__restrict__ pbox, int P, int64_t *__restrict__ joint) {
  __shared__ int64_t part[4][256];
  int64_t x0 = GR_REGION_FAR, y0 = GR_REGION_FAR, x1 = -GR_REGION_FAR, y1 = -GR_REGION_FAR;
  for (int p = (int)threadIdx.x; p < P; p += 256) {
    const int64_t *b = pbox + (int64_t)p * 4;
    if (b[0] <= b[2] && b[1] <= b[3]) { x0 = min(x0, b[0]); y0 = min(y0, b[1]); x1 = max(x1, b[2]); y1 = max(y1, b[3]); }
  }
  part[0][threadIdx.x] = x0; part[1][threadIdx.x] = y0; part[2][threadIdx.x] = x1; part[3][threadIdx.x] = y1;
  __syncthreads();
  if (threadIdx.x < 4) {
    const bool lo = threadIdx.x < 2;
    int64_t v = part[threadIdx.x][0];
    for (int i = 1; i < 256; ++i) v = lo ? min(v, part[threadIdx.x][i]) : max(v, part[threadIdx.x][i]);
    joint[threadIdx.x] = v;
  }
}

// pq [N][2] snapped points; rv, roff, rpoly, pbox: the ring table; joint [4] of k_region_joint_box; mask [N]; stats
// [GR_PIR_STAT_WORDS].  One point per lane; rows, rings and edges are walked WAVE-UNIFORMLY (every address of the table is the same
// in all lanes: scalar loads), the lanes differ only in their execution mask.  A lane is `contained` once it is on a ring or a row's
// crossings came out odd (Q3) and then takes no further part; `near` once an edge is within D (Q4), after which it only goes on
// counting crossings (the statistics tell the two apart).  The wave leaves the table when every lane is contained.
__global__ __launch_bounds__(256) void k_points_in_region(const int64_t *__restrict__ pq, const int64_t *__restrict__ rv,
                                                          const int64_t *__restrict__ roff, const int32_t *__restrict__ rpoly,
                                                          const int64_t *__restrict__ pbox, const int64_t *__restrict__ joint,
                                                          uint8_t *__restrict__ mask, unsigned long long *__restrict__ stats,
                                                          RegionArgs a) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t D = a.D;
  const u128 D2 = (u128)(uint64_t)D * (u128)(uint64_t)D;
  int64_t px = 0, py = 0;
  bool live = idx < a.N;
  if (live) {
    px = pq[idx * 2]; py = pq[idx * 2 + 1];
    live = px >= joint[0] - D && px <= joint[2] + D && py >= joint[1] - D && py <= joint[3] + D;   // most points of a mesh leave here
  }
  bool contained = false, near = false;
  unsigned long long wide = 0;
  int cur = -1;          // row of the rings being walked (wave-uniform)
  bool in_row = false;   // this lane's point is in the row's box grown by D, and was not contained when the row began
  int parity = 0;

  for (int r = 0; r < a.R; ++r) {
    const int p = rpoly[r];
    if (p != cur) {
      if (in_row && (parity & 1)) contained = true;
      in_row = false; parity = 0;
      if (!__ballot(live && !contained)) break;
      cur = (p >= 0 && p < a.P) ? p : -1;
      if (cur >= 0) {
        const int64_t *b = pbox + (int64_t)cur * 4;
        in_row = live && !contained && b[0] <= b[2] && b[1] <= b[3] && px >= b[0] - D && px <= b[2] + D && py >= b[1] - D &&
                 py <= b[3] + D;
      }
    }
    int64_t i0;
    const int64_t n = ring_span(roff, r, a.n_rv, i0);
    if (cur < 0 || n < 3 || !__ballot(in_row && !contained)) continue;
    const int64_t *v = rv + i0 * 2;
    int64_t ax = v[2 * (n - 1)], ay = v[2 * (n - 1) + 1];
    for (int64_t i = 0; i < n; ++i) {
      const int64_t bx = v[2 * i], by = v[2 * i + 1];
      if (in_row && !contained) {
        const int64_t exlo = min(ax, bx), exhi = max(ax, bx), eylo = min(ay, by), eyhi = max(ay, by);
        if (edge_crossing<true>(ax, ay, bx, by, px, py, parity)) contained = true;   // Q3; a point on the edge is contained at once
        // Q4: the distance to the closed edge against D, for an edge whose box grown by D holds the point
        if (D > 0 && !near && !contained && px >= exlo - D && px <= exhi + D && py >= eylo - D && py <= eyhi + D) {
          const int64_t ux = px - ax, uy = py - ay, ex = bx - ax, ey = by - ay;   // |.| < 2^42: products below 2^84
          const i128 t = (i128)ux * ex + (i128)uy * ey, L2 = (i128)ex * ex + (i128)ey * ey;
          if (t <= 0) {
            near = (u128)((i128)ux * ux + (i128)uy * uy) <= D2;
          } else if (t >= L2) {
            const int64_t wx = px - bx, wy = py - by;
            near = (u128)((i128)wx * wx + (i128)wy * wy) <= D2;
          } else {
            const i128 c = (i128)ex * uy - (i128)ey * ux;
            const u128 m = (u128)(c < 0 ? -c : c);
            ++wide;
            near = le_256(mul_128x128(m, m), mul_128x128(D2, (u128)L2));   // cross^2 <= D^2 L2: about 166 bits
          }
        }
      }
      ax = bx; ay = by;
    }
  }
  if (in_row && (parity & 1)) contained = true;
  if (idx < a.N) mask[idx] = (contained || near) ? 1 : 0;

  stat_count(stats, GR_PIR_STAT_INSIDE, contained || near, lane);
  stat_count(stats, GR_PIR_STAT_BUFFER_ONLY, near && !contained, lane);
  stat_add(stats, GR_PIR_STAT_WIDE, wide, lane);
}

// ---- gr_submesh_extract: the faces with a vertex in the mask, the vertices they use, renumbered in order (Q5, Q6) ------------------
// fflag [F], vused [V] (zeroed by the caller): 1 where kept.  A face that names a vertex outside [0, V) reads nothing and is counted.
__global__ __launch_bounds__(256) void k_submesh_flags(const uint8_t *__restrict__ mask, int64_t V, const int32_t *__restrict__ faces,
                                                       int64_t F, int32_t *__restrict__ fflag, int32_t *__restrict__ vused,
                                                       unsigned long long *__restrict__ counts) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (f < F) {
    int64_t v0, v1, v2;
    int keep = 0;
    bad = !load_face(faces, f, V, v0, v1, v2);
    if (!bad) {
      keep = (mask[v0] | mask[v1] | mask[v2]) ? 1 : 0;
      if (keep) { vused[v0] = 1; vused[v1] = 1; vused[v2] = 1; }   // every writer stores the same value
    }
    fflag[f] = keep;
  }
  stat_count(counts, 2, bad, lane);
}

// (k_submesh_write, the write kernel behind the two scans, is compact_dev.hpp's: gr_cluster_decimate compacts with it too)


// ---- gr_class_outlines: the outline rings of every class of a per-face labelling ---------------------
// Integers only.  Vertices are sorted by (x, y, index) (two stable radix passes) and every group of equal (x, y) takes its
// smallest index (X2); every taking-part face emits three directed edges over those ids, counter-clockwise by the exact sign of its
// doubled area (X3); the edges are sorted by (class, from, to), a run of equal edges looks its reverse up by binary search and keeps
// the surplus (X4); the surviving copies, still sorted, are the slots.  Sorting the slots by (class, to) lines the incoming copies of
// every (class, vertex) up with its outgoing ones, which are consecutive slots: position p of that order is followed by slot p
// (X5).  Pointer doubling over that permutation finds the smallest slot of every ring and every slot's distance to it (X6).
enum {   // 64-bit words at the front of the scratch: counts the host reads back
  GR_OUTL_HEAD_RUNS = 0,    // distinct (class, from, to) among the directed edges
  GR_OUTL_HEAD_EDGES = 1,   // surviving copies: slots
  GR_OUTL_HEAD_WORDS = 32   // 256 bytes
};

// key [V] = y of vertex i; idx [V] = i
__global__ __launch_bounds__(256) void k_outline_vertex_keys(const int64_t *__restrict__ vq, int64_t V, int64_t *__restrict__ key,
                                                             int32_t *__restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < V) { key[i] = vq[i * 2 + 1]; idx[i] = (int32_t)i; }
}
// key [V] = x of vertex idx[i]: the key of the second pass
__global__ __launch_bounds__(256) void k_outline_vertex_gather(const int64_t *__restrict__ vq, int64_t V, const int32_t *__restrict__ idx,
                                                               int64_t *__restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < V) key[i] = vq[(int64_t)idx[i] * 2];
}
// idx [V]: the vertices sorted by (x, y, index).  hp [V] = i where a group of equal (x, y) starts, else 0: its running maximum is
// the position of the group's first member.
__global__ __launch_bounds__(256) void k_outline_vertex_heads(const int64_t *__restrict__ vq, int64_t V, const int32_t *__restrict__ idx,
                                                              int32_t *__restrict__ hp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= V) return;
  bool head = i == 0;
  if (!head) {
    const int64_t a = idx[i - 1], b = idx[i];
    head = vq[a * 2] != vq[b * 2] || vq[a * 2 + 1] != vq[b * 2 + 1];
  }
  hp[i] = head ? (int32_t)i : 0;
}
__global__ __launch_bounds__(256) void k_outline_canon(int64_t V, const int32_t *__restrict__ idx, const int32_t *__restrict__ hp_max,
                                                       int32_t *__restrict__ canon) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < V) canon[idx[i]] = idx[hp_max[i]];   // the group's smallest index: the sort is stable
}

// X3.  pair [3 F], cl [3 F]: the directed edges of face f at 3 f .. 3 f + 2, from << 31 | to and the class; a face that takes no part
// writes three edges of the class n_classes, which sort behind every real one.  A face that names a vertex outside [0, V) reads nothing.
__global__ __launch_bounds__(256) void k_outline_face_edges(const int64_t *__restrict__ vq, int64_t V, const int32_t *__restrict__ faces,
                                                            int64_t F, const int32_t *__restrict__ face_class, int C,
                                                            const int32_t *__restrict__ canon, unsigned long long *__restrict__ pair,
                                                            uint32_t *__restrict__ cl, unsigned long long *__restrict__ stats) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false, no_class = false, flat = false, turned = false;
  if (f < F) {
    int64_t v0, v1, v2;
    bad = !load_face(faces, f, V, v0, v1, v2);
    const int cls = face_class[f];
    int64_t a = 0, b = 0, c = 0;
    bool live = false;
    no_class = !bad && (cls < 0 || cls >= C);
    if (!bad && !no_class) {
      a = canon[v0]; b = canon[v1]; c = canon[v2];
      const i128 o = orient(vq[a * 2], vq[a * 2 + 1], vq[b * 2], vq[b * 2 + 1], vq[c * 2], vq[c * 2 + 1]);
      flat = o == 0;
      turned = o < 0;
      if (turned) { const int64_t t = b; b = c; c = t; }
      live = !flat;
    }
    const uint32_t k = live ? (uint32_t)cls : (uint32_t)C;
    pair[f * 3] = live ? ((unsigned long long)a << 31 | (unsigned long long)b) : 0ull;
    pair[f * 3 + 1] = live ? ((unsigned long long)b << 31 | (unsigned long long)c) : 0ull;
    pair[f * 3 + 2] = live ? ((unsigned long long)c << 31 | (unsigned long long)a) : 0ull;
    cl[f * 3] = k; cl[f * 3 + 1] = k; cl[f * 3 + 2] = k;
  }
  stat_count(stats, GR_OUTL_STAT_NO_CLASS, no_class, lane);
  stat_count(stats, GR_OUTL_STAT_ZERO_AREA, flat, lane);
  stat_count(stats, GR_OUTL_STAT_TURNED, turned, lane);
  stat_count(stats, GR_OUTL_STAT_BAD_FACES, bad, lane);
}

// Y1-Y3 (gr_member_outlines).  pair [3 nnz], cl [3 nnz]: the directed edges of member m = (face, class) at 3 m .. 3 m + 2, as above.
// A wave owns 64 consecutive faces.  First a face per lane: its row [lo, hi) of the table, clamped into [0, nnz] (Y2), the index
// check, the canonical corners and the 128-bit orient -- once per face, however many classes it is in.  Then a member per lane over
// the wave's stretch of the table, [lo of its first face, hi of its last): the owner is the last lane whose row starts at or before
// m (six shuffles over the row starts, which rise in a well-formed table), its corners and state come by shuffle, and the stores of
// a wave are consecutive.  Rows of any length cost the same per member; every loop is bounded by the clamped stretch.  In a
// malformed table stretches may overlap or leave gaps: every index stays inside [0, nnz), the caller has pre-filled cl, the
// violations are counted in GR_OUTL_STAT_BAD_ROWS and the host stops behind this kernel's counts.
enum { MEMBER_BAD = 0, MEMBER_LIVE = 1, MEMBER_TURNED = 2, MEMBER_FLAT = 3 };
__global__ __launch_bounds__(256) void k_outline_member_edges(const int64_t *__restrict__ vq, int64_t V, const int32_t *__restrict__ faces,
                                                              int64_t F, const int64_t *__restrict__ face_ptr,
                                                              const int32_t *__restrict__ members, int64_t nnz, int C,
                                                              const int32_t *__restrict__ canon, unsigned long long *__restrict__ pair,
                                                              uint32_t *__restrict__ cl, unsigned long long *__restrict__ stats) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int32_t lo = 0, hi = 0, a = 0, b = 0, c = 0;
  int state = MEMBER_BAD;
  uint32_t bad_rows = 0, n_no_class = 0, n_flat = 0, n_turned = 0;
  bool bad = false;
  if (f == 0) bad_rows += (face_ptr[0] != 0) + (face_ptr[F] != nnz);
  if (f < F) {
    const int64_t p0 = face_ptr[f], p1 = face_ptr[f + 1];
    bad_rows += p1 < p0;
    const int64_t l = min(max(p0, (int64_t)0), nnz), h = min(max(p1, l), nnz);
    lo = (int32_t)l; hi = (int32_t)h;   // 3 nnz < 2^31
    int64_t v0, v1, v2;
    bad = !load_face(faces, f, V, v0, v1, v2);
    if (!bad) {
      a = canon[v0]; b = canon[v1]; c = canon[v2];
      const i128 o = orient(vq[(int64_t)a * 2], vq[(int64_t)a * 2 + 1], vq[(int64_t)b * 2], vq[(int64_t)b * 2 + 1], vq[(int64_t)c * 2],
                            vq[(int64_t)c * 2 + 1]);
      state = o == 0 ? MEMBER_FLAT : (o < 0 ? MEMBER_TURNED : MEMBER_LIVE);
      if (o < 0) { const int32_t t = b; b = c; c = t; }
    }
  }
  // the wave's stretch; a lane behind the last face owns the empty row at its end
  const int64_t wave_f0 = f - lane;
  const int n_valid = (int)min((int64_t)64, max(F - wave_f0, (int64_t)0));
  const int32_t wlo = __builtin_amdgcn_readfirstlane(lo);
  const int32_t last_hi = __shfl(hi, max(n_valid - 1, 0));
  const int32_t whi = __builtin_amdgcn_readfirstlane(n_valid > 0 ? last_hi : wlo);
  if (lane >= n_valid) { lo = whi; hi = whi; }
  for (int32_t base = wlo; base < whi; base += 64) {
    const int32_t m = base + lane;   // < 2^31 / 3 + 64
    int j = 0;
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) {
      const int32_t start = __shfl(lo, j + step);   // j + step <= 63
      if (start <= m) j += step;
    }
    const int32_t olo = __shfl(lo, j), ohi = __shfl(hi, j), oa = __shfl(a, j), ob = __shfl(b, j), oc = __shfl(c, j);
    const int ostate = __shfl(state, j);
    if (m < whi) {
      const int32_t cls = members[m];
      const bool in_row = m >= olo && m < ohi;   // always, in a well-formed table
      if (in_row && m > olo) bad_rows += members[m - 1] >= cls;   // Y2: strictly ascending
      bool live = false;
      if (in_row && ostate != MEMBER_BAD) {
        if (cls < 0 || cls >= C) ++n_no_class;
        else if (ostate == MEMBER_FLAT) ++n_flat;
        else { live = true; n_turned += ostate == MEMBER_TURNED; }
      }
      const uint32_t k = live ? (uint32_t)cls : (uint32_t)C;
      const unsigned long long ua = (uint32_t)oa, ub = (uint32_t)ob, uc = (uint32_t)oc;
      const int64_t e = (int64_t)m * 3;
      pair[e] = live ? (ua << 31 | ub) : 0ull;
      pair[e + 1] = live ? (ub << 31 | uc) : 0ull;
      pair[e + 2] = live ? (uc << 31 | ua) : 0ull;
      cl[e] = k; cl[e + 1] = k; cl[e + 2] = k;
    }
  }
  stat_add_u32(stats, GR_OUTL_STAT_NO_CLASS, n_no_class, lane);   // every sum is at most nnz < 2^30
  stat_add_u32(stats, GR_OUTL_STAT_ZERO_AREA, n_flat, lane);
  stat_add_u32(stats, GR_OUTL_STAT_TURNED, n_turned, lane);
  stat_count(stats, GR_OUTL_STAT_BAD_FACES, bad, lane);
  stat_add_u32(stats, GR_OUTL_STAT_BAD_ROWS, bad_rows, lane);
}

// pair, cl [n] sorted by (class, from, to).  flag [n] = 1 where a run of equal real edges starts.
__global__ __launch_bounds__(256) void k_outline_run_heads(const unsigned long long *__restrict__ pair, const uint32_t *__restrict__ cl,
                                                           int64_t n, int C, int32_t *__restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = cl[i];
  flag[i] = (c < (uint32_t)C && (i == 0 || cl[i - 1] != c || pair[i - 1] != pair[i])) ? 1 : 0;
}
// ex [n]: the exclusive sum of flag, the run of a head.  ustart [runs + 1]: where each run starts, and the end of the real edges.
__global__ __launch_bounds__(256) void k_outline_run_starts(const uint32_t *__restrict__ cl, int64_t n, int C,
                                                            const int32_t *__restrict__ flag, const int32_t *__restrict__ ex,
                                                            int32_t *__restrict__ ustart, unsigned long long *__restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || cl[i] >= (uint32_t)C) return;
  if (flag[i]) ustart[ex[i]] = (int32_t)i;
  if (i == n - 1 || cl[i + 1] >= (uint32_t)C) {   // the last real edge
    const int32_t runs = ex[i] + flag[i];
    ustart[runs] = (int32_t)(i + 1);
    head[GR_OUTL_HEAD_RUNS] = (unsigned long long)runs;
  }
}
// X4.  One run per lane: its n1 copies of (c, a -> b) against the n2 copies of (c, b -> a), found by binary search over the sorted
// edges; surv [run] = max(n1 - n2, 0) (zeroed by the caller behind the runs).
__global__ __launch_bounds__(256) void k_outline_cancel(const unsigned long long *__restrict__ pair, const uint32_t *__restrict__ cl,
                                                        const int32_t *__restrict__ ex, const int32_t *__restrict__ ustart,
                                                        const unsigned long long *__restrict__ head, int32_t *__restrict__ surv,
                                                        unsigned long long *__restrict__ stats) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t runs = (int64_t)head[GR_OUTL_HEAD_RUNS];
  int32_t n_cancel = 0;
  bool multi = false;
  if (u < runs) {
    const int32_t i0 = ustart[u], n1 = ustart[u + 1] - i0, n_real = ustart[runs];
    const uint32_t c = cl[i0];
    const unsigned long long p = pair[i0], a = p >> 31, b = p & 0x7FFFFFFFull, rp = b << 31 | a;
    int32_t lo = 0, hi = n_real;
    while (lo < hi) {
      const int32_t mid = (int32_t)(((uint32_t)lo + (uint32_t)hi) >> 1);
      const uint32_t cm = cl[mid];
      if (cm < c || (cm == c && pair[mid] < rp)) lo = mid + 1; else hi = mid;
    }
    int32_t n2 = 0;
    if (lo < n_real && cl[lo] == c && pair[lo] == rp) { const int32_t r = ex[lo]; n2 = ustart[r + 1] - ustart[r]; }   // lo is a head
    const int32_t n = n1 > n2 ? n1 - n2 : 0;
    surv[u] = n;
    if (a < b) n_cancel = n1 < n2 ? n1 : n2;   // once per unordered pair
    multi = n > 1;
  }
  stat_add_u32(stats, GR_OUTL_STAT_CANCELLED, (uint32_t)n_cancel, lane);   // all cancelled pairs together are fewer than 2^31
  stat_count(stats, GR_OUTL_STAT_MULTI, multi, lane);
}
// soff [run]: the exclusive sum of surv, the first slot of the run.  Writes the slots: efrom, ecls, and the key (class, to) with the
// slot as its value for the sort of X5.
__global__ __launch_bounds__(256) void k_outline_emit_edges(const unsigned long long *__restrict__ pair, const uint32_t *__restrict__ cl,
                                                            const int32_t *__restrict__ ustart, const int32_t *__restrict__ surv,
                                                            const int32_t *__restrict__ soff, int64_t runs, int32_t *__restrict__ efrom,
                                                            int32_t *__restrict__ ecls, unsigned long long *__restrict__ kin,
                                                            int32_t *__restrict__ vin) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= runs) return;
  const int32_t n = surv[u];
  if (n <= 0) return;
  const int32_t i0 = ustart[u], base = soff[u];
  const uint32_t c = cl[i0];
  const unsigned long long p = pair[i0];
  for (int32_t k = 0; k < n; ++k) {
    efrom[base + k] = (int32_t)(p >> 31);
    ecls[base + k] = (int32_t)c;
    kin[base + k] = (unsigned long long)c << 31 | (p & 0x7FFFFFFFull);
    vin[base + k] = base + k;
  }
}
// X5.  vin_s [E]: the slots sorted by (class, to), stably.  Every (class, vertex) has as many incoming as outgoing copies, and the
// outgoing ones are consecutive slots in the same order of (class, vertex): the slot at position p is followed by slot p.
__global__ __launch_bounds__(256) void k_outline_successor(const int32_t *__restrict__ vin_s, int64_t E, int32_t *__restrict__ succ,
                                                           int32_t *__restrict__ mn, int32_t *__restrict__ off) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= E) return;
  succ[vin_s[p]] = (int32_t)p;
  mn[p] = (int32_t)p; off[p] = 0;
}
// X6, one round of pointer doubling.  Before: nxt [s] is the slot `step` edges ahead of s, mn [s] the smallest slot among those `step`
// edges from s on, off [s] how far ahead it first occurs.  After (the other buffer): the same for 2 step.
__global__ __launch_bounds__(256) void k_outline_round(const int32_t *__restrict__ nxt, const int32_t *__restrict__ mn,
                                                       const int32_t *__restrict__ off, int32_t *__restrict__ nxt2,
                                                       int32_t *__restrict__ mn2, int32_t *__restrict__ off2, uint32_t step, int64_t E) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= E) return;
  const int32_t n = nxt[s], m1 = mn[s], m2 = mn[n];
  const bool far = m2 < m1;   // equal: the ring has been walked round, the first occurrence stays
  mn2[s] = far ? m2 : m1;
  off2[s] = far ? (int32_t)(step + (uint32_t)off[n]) : off[s];
  nxt2[s] = nxt[n];
}
// w [E + 1]: length << 32 | 1 at the leader of a ring (the slot that is its own minimum), else 0; the length is one more than the
// distance of the leader's successor to it.
__global__ __launch_bounds__(256) void k_outline_ring_words(const int32_t *__restrict__ succ, const int32_t *__restrict__ mn,
                                                            const int32_t *__restrict__ off, int64_t E, unsigned long long *__restrict__ w) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s > E) return;
  w[s] = (s < E && mn[s] == (int32_t)s) ? ((unsigned long long)((uint32_t)off[succ[s]] + 1u) << 32 | 1ull) : 0ull;
}
// ws [E + 1]: the exclusive sum of w: at a leader, first ring vertex << 32 | ring.  Writes the caller's buffers.
__global__ __launch_bounds__(256) void k_outline_emit_rings(const int32_t *__restrict__ mn, const int32_t *__restrict__ off,
                                                            const int32_t *__restrict__ efrom, const int32_t *__restrict__ ecls,
                                                            const unsigned long long *__restrict__ w,
                                                            const unsigned long long *__restrict__ ws, int64_t E,
                                                            int32_t *__restrict__ ring_vertices, int64_t *__restrict__ ring_offsets,
                                                            int32_t *__restrict__ ring_class) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= E) return;
  const int32_t l = mn[s];
  const unsigned long long wl = ws[l];
  const int64_t start = (int64_t)(wl >> 32), ring = (int64_t)(wl & 0xFFFFFFFFull), len = (int64_t)(w[l] >> 32);
  const int64_t rank = s == l ? 0 : len - (int64_t)off[s];
  if (rank >= 0 && rank < len && start + rank < E) ring_vertices[start + rank] = efrom[s];   // (always: a guard against a torn table)
  if (s == l) { ring_offsets[ring] = start; ring_class[ring] = ecls[s]; }
  if (s == 0) ring_offsets[(int64_t)(ws[E] & 0xFFFFFFFFull)] = E;
}

}  // namespace

// The ring table as every call here takes it: rv [n_rv][2], roff [R + 1], rpoly [R], pbox [P][4].  Its ranges and its pointers; the
// hole flags are the weights call's own.  The boxes are needed with a row; boxes_with_rings: with a ring (the weights call, which
// launches nothing without rings and has always taken the boxes so).
static int check_ring_table(gr_ctx *c, const char *name, int64_t n_rv, int64_t R, int64_t P, const int64_t *rv, const int64_t *roff,
                            const int32_t *rpoly, const int64_t *pbox, bool boxes_with_rings = false) {
  if (R < 0 || P < 0 || n_rv < 0 || R > 0x7FFFFFFF || P > 0x7FFFFFFF)
    return fail(c, GR_EINVAL, "%s: bad ring table R=%lld P=%lld ring vertices=%lld", name, (long long)R, (long long)P, (long long)n_rv);
  if (((boxes_with_rings ? R : P) > 0 && !pbox) || (R > 0 && (!roff || !rpoly || (n_rv > 0 && !rv)))) return fail(c, GR_EINVAL, "%s: null ring table", name);
  return GR_OK;
}

// The trace both outline calls share, defined behind them (X2, X4-X6; DESIGN.md sections 8i and 8l): canonical vertices, then
// `emit_edges(canon, pair, cl)` enqueues the one kernel in which they differ -- the N3 directed edges as from << 31 | to and the
// class, n_classes for an edge that takes no part --, then the two-pass edge sort, runs, cancellation, scratch B, successors,
// pointer doubling and the ring emit.
// member_rows: the edges come from a member table (Y2): cl is pre-filled with 0xFFFFFFFF, which no class reaches, so that a gap of
// a malformed table holds no uninitialised word, and GR_OUTL_STAT_BAD_ROWS is read at the first synchronisation: non-zero ends the
// call there with GR_OK, both totals 0 and nothing written but the statistics.
struct OutlineOut {
  int32_t *canon, *ring_vertices;
  int64_t *ring_offsets;
  int32_t *ring_class;
  int64_t cap, *n_edges_h, *n_rings_h;
  unsigned long long *stats;
};
static int outline_trace(gr_ctx *c, const char *name, const int64_t *verts_q, int64_t V, int64_t N3, int n_classes, bool member_rows,
                         const OutlineOut &out, hipStream_t s,
                         const std::function<void(const int32_t *, unsigned long long *, uint32_t *)> &emit_edges);

extern "C" {

int gr_polygon_class_weights(gr_ctx *c, const int64_t *tri, const int32_t *face_class, const double *face_weight, int64_t F,
                             const int64_t *ring_vertices, int64_t n_ring_vertices, const int64_t *ring_offsets,
                             const int32_t *ring_polygon, const int32_t *ring_is_hole, int64_t R, const int64_t *polygon_boxes,
                             int64_t P, int mode, int C, double *weights, uint64_t *stats, void *stream) {
  if (!c) return GR_EINVAL;
  if (F < 0 || C < 0 || F > 0x7FFFFFFFll * 256) return fail(c, GR_EINVAL, "gr_polygon_class_weights: bad shape F=%lld C=%d", (long long)F, C);
  int rc = check_ring_table(c, "gr_polygon_class_weights", n_ring_vertices, R, P, ring_vertices, ring_offsets, ring_polygon, polygon_boxes,
                            true);
  if (rc != GR_OK) return rc;
  if (mode != GR_POLY_WITHIN && mode != GR_POLY_OVERLAY)
    return fail(c, GR_EINVAL, "polygon-weights mode %d is neither GR_POLY_WITHIN nor GR_POLY_OVERLAY", mode);
  if (!stats || (P > 0 && C > 0 && !weights)) return fail(c, GR_EINVAL, "null polygon-weights outputs");
  if ((F > 0 && (!tri || !face_class || !face_weight)) || (R > 0 && !ring_is_hole))
    return fail(c, GR_EINVAL, "null polygon-weights arrays");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  if (P > 0 && C > 0) GR_HIP(c, hipMemsetAsync(weights, 0, sizeof(double) * (size_t)P * (size_t)C, s));
  GR_HIP(c, hipMemsetAsync(stats, 0, sizeof(uint64_t) * GR_POLY_STAT_WORDS, s));
  if (F == 0 || R == 0 || P == 0 || C == 0) return GR_OK;
  PolyArgs a;
  a.F = F; a.n_rv = n_ring_vertices; a.R = (int)R; a.P = (int)P; a.C = C; a.mode = mode;
  hipLaunchKernelGGL(k_polygon_weights, dim3((unsigned)ceil_div(F, 256)), dim3(256), 0, s, tri, face_class, face_weight, ring_vertices,
                     ring_offsets, ring_polygon, ring_is_hole, polygon_boxes, weights, (unsigned long long *)stats, a);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

int gr_face_polygon_index(gr_ctx *c, const int64_t *verts_q, int64_t V, const int32_t *faces, int64_t F,
                          const int64_t *ring_vertices, int64_t n_ring_vertices, const int64_t *ring_offsets,
                          const int32_t *ring_polygon, int64_t R, const int64_t *polygon_boxes, int64_t P, int64_t grid_x0,
                          int64_t grid_y0, int64_t cell_w, int64_t cell_h, int nx, int ny, const int64_t *cell_offsets,
                          const int32_t *cell_polygons, int64_t n_cell_polygons, int32_t *face_polygon, uint64_t *stats,
                          void *stream) {
  if (!c) return GR_EINVAL;
  if (F < 0 || V < 0 || n_cell_polygons < 0 || F > 0x7FFFFFFFll * 256 || V > 0x7FFFFFFFll)
    return fail(c, GR_EINVAL, "gr_face_polygon_index: bad shape F=%lld V=%lld", (long long)F, (long long)V);
  int rc = check_ring_table(c, "gr_face_polygon_index", n_ring_vertices, R, P, ring_vertices, ring_offsets, ring_polygon, polygon_boxes);
  if (rc != GR_OK) return rc;
  if (nx < 1 || ny < 1 || (int64_t)nx * ny > GR_FPI_MAX_CELLS || cell_w < 1 || cell_h < 1)
    return fail(c, GR_EINVAL, "gr_face_polygon_index: bad cell grid nx=%d ny=%d (1 <= nx ny <= %d) cell=%lld x %lld (>= 1)", nx, ny,
                (int)GR_FPI_MAX_CELLS, (long long)cell_w, (long long)cell_h);
  if (!stats || !cell_offsets || (F > 0 && (!faces || !face_polygon)) || (V > 0 && !verts_q) ||
      (n_cell_polygons > 0 && !cell_polygons))
    return fail(c, GR_EINVAL, "gr_face_polygon_index: null arrays");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  GR_HIP(c, hipMemsetAsync(stats, 0, sizeof(uint64_t) * GR_FPI_STAT_WORDS, s));
  if (F == 0) return GR_OK;
  FaceIndexArgs a;
  a.F = F; a.V = V; a.n_rv = n_ring_vertices; a.n_cp = n_cell_polygons;
  a.gx0 = grid_x0; a.gy0 = grid_y0; a.cw = cell_w; a.ch = cell_h;
  a.R = (int)R; a.P = (int)P; a.nx = nx; a.ny = ny;
  hipLaunchKernelGGL(k_face_polygon_index, dim3((unsigned)ceil_div(F, 256)), dim3(256), 0, s, verts_q, faces, ring_vertices,
                     ring_offsets, ring_polygon, polygon_boxes, cell_offsets, cell_polygons, face_polygon,
                     (unsigned long long *)stats, a);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

int gr_points_in_region(gr_ctx *c, const int64_t *points_q, int64_t N, const int64_t *ring_vertices, int64_t n_ring_vertices,
                        const int64_t *ring_offsets, const int32_t *ring_polygon, int64_t R, const int64_t *polygon_boxes,
                        int64_t P, int64_t D, uint8_t *mask, uint64_t *stats, void *stream) {
  if (!c) return GR_EINVAL;
  if (N < 0 || N > 0x7FFFFFFFll * 256) return fail(c, GR_EINVAL, "gr_points_in_region: bad shape N=%lld", (long long)N);
  int rc = check_ring_table(c, "gr_points_in_region", n_ring_vertices, R, P, ring_vertices, ring_offsets, ring_polygon, polygon_boxes);
  if (rc != GR_OK) return rc;
  if (D < 0 || D >= ((int64_t)1 << 40))
    return fail(c, GR_EINVAL, "gr_points_in_region: buffer D=%lld outside [0, 2^40) grid steps", (long long)D);
  if (!stats || (N > 0 && (!points_q || !mask))) return fail(c, GR_EINVAL, "gr_points_in_region: null arrays");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  GR_HIP(c, hipMemsetAsync(stats, 0, sizeof(uint64_t) * GR_PIR_STAT_WORDS, s));
  if (N == 0) return GR_OK;
  if (R == 0 || P == 0) {   // a region without rings holds nothing
    GR_HIP(c, hipMemsetAsync(mask, 0, (size_t)N, s));
    return GR_OK;
  }
  // scratch: joint box [4] i64
  Carve cv;
  const auto o_joint = cv.array<int64_t>(4);
  rc = stage_acquire(c, c->stage, cv.total(), s, "region");
  if (rc != GR_OK) return rc;
  cv.base = c->stage.ptr;
  int64_t *joint = o_joint();
  hipLaunchKernelGGL(k_region_joint_box, dim3(1), dim3(256), 0, s, polygon_boxes, (int)P, joint);
  RegionArgs a;
  a.N = N; a.n_rv = n_ring_vertices; a.D = D; a.R = (int)R; a.P = (int)P;
  hipLaunchKernelGGL(k_points_in_region, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, s, points_q, ring_vertices, ring_offsets,
                     ring_polygon, polygon_boxes, (const int64_t *)joint, mask, (unsigned long long *)stats, a);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

int gr_submesh_extract(gr_ctx *c, const uint8_t *mask, int64_t V, const int32_t *faces, int64_t F, int64_t *face_ids,
                       int64_t *point_ids, int32_t *new_faces, uint64_t *counts, void *stream) {
  if (!c) return GR_EINVAL;
  if (V < 0 || F < 0 || V > 0x7FFFFFFFll || F > 0x7FFFFFFFll)
    return fail(c, GR_EINVAL, "gr_submesh_extract: bad shape V=%lld F=%lld", (long long)V, (long long)F);
  if (!counts || (V > 0 && (!mask || !point_ids)) || (F > 0 && (!faces || !face_ids || !new_faces)))
    return fail(c, GR_EINVAL, "gr_submesh_extract: null arrays");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  GR_HIP(c, hipMemsetAsync(counts, 0, sizeof(uint64_t) * 3, s));
  if (F == 0) return GR_OK;   // no face: nothing is kept (a vertex no face uses is dropped)
  // scratch: fflag [F] | fpos [F] | vused [V] | vpos [V] | the scans' temporaries
  Plan p;
  const FlagScan fs(c, p, F), vs(c, p, V);
  int rc = stage_acquire(c, c->stage, p.finish(), s, "sub-mesh");
  if (rc != GR_OK) return rc;
  p.base = c->stage.ptr;
  GR_TRY(compact_begin(c, vs, s));
  hipLaunchKernelGGL(k_submesh_flags, dim3((unsigned)ceil_div(F, 256)), dim3(256), 0, s, mask, V, faces, F, fs.flag(), vs.flag(),
                     (unsigned long long *)counts);
  return compact_write(c, fs, vs, s, faces, face_ids, point_ids, new_faces, (unsigned long long *)counts);
}

int gr_class_outlines(gr_ctx *c, const int64_t *verts_q, int64_t V, const int32_t *faces, int64_t F, const int32_t *face_class,
                      int n_classes, int32_t *canon, int32_t *ring_vertices, int64_t *ring_offsets, int32_t *ring_class,
                      int64_t ring_vertex_cap, int64_t *n_edges_h, int64_t *n_rings_h, uint64_t *stats, void *stream) {
  if (!c) return GR_EINVAL;
  if (V < 0 || F < 0 || ring_vertex_cap < 0 || V > 0x7FFFFFFFll || F > 0x7FFFFFFFll / 3 || ring_vertex_cap > 0x7FFFFFFFll)
    return fail(c, GR_EINVAL, "gr_class_outlines: bad shape V=%lld F=%lld capacity=%lld (V < 2^31, 3 F < 2^31)", (long long)V,
                (long long)F, (long long)ring_vertex_cap);
  if (n_classes < 0 || n_classes > GR_OUTL_MAX_CLASSES)
    return fail(c, GR_EINVAL, "gr_class_outlines: n_classes=%d outside [0, %d]", n_classes, (int)GR_OUTL_MAX_CLASSES);
  if (!stats || !n_edges_h || !n_rings_h || (V > 0 && !verts_q) || (F > 0 && (!faces || !face_class)) ||
      (ring_vertex_cap > 0 && (!ring_vertices || !ring_offsets || !ring_class || (V > 0 && !canon))))
    return fail(c, GR_EINVAL, "gr_class_outlines: null arrays");
  *n_edges_h = 0; *n_rings_h = 0;
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  GR_HIP(c, hipMemsetAsync(stats, 0, sizeof(uint64_t) * GR_OUTL_STAT_WORDS, s));
  unsigned long long *st = (unsigned long long *)stats;
  const OutlineOut out{canon, ring_vertices, ring_offsets, ring_class, ring_vertex_cap, n_edges_h, n_rings_h, st};
  return outline_trace(c, "gr_class_outlines", verts_q, V, 3 * F, n_classes, false, out, s,
                       [&](const int32_t *canon_d, unsigned long long *pair, uint32_t *cl) {
                         hipLaunchKernelGGL(k_outline_face_edges, dim3((unsigned)ceil_div(F, 256)), dim3(256), 0, s, verts_q, V, faces, F,
                                            face_class, n_classes, canon_d, pair, cl, st);
                       });
}

int gr_member_outlines(gr_ctx *c, const int64_t *verts_q, int64_t V, const int32_t *faces, int64_t F, const int64_t *face_ptr,
                       const int32_t *face_members, int64_t nnz, int32_t n_classes, int32_t *canon, int32_t *ring_vertices,
                       int64_t *ring_offsets, int32_t *ring_class, int64_t ring_vertex_cap, int64_t *n_edges_h, int64_t *n_rings_h,
                       uint64_t *stats, void *stream) {
  if (!c) return GR_EINVAL;
  if (V < 0 || F < 0 || nnz < 0 || ring_vertex_cap < 0 || V > 0x7FFFFFFFll || F > 0x7FFFFFFFll || nnz > 0x7FFFFFFFll / 3 ||
      ring_vertex_cap > 0x7FFFFFFFll)
    return fail(c, GR_EINVAL, "gr_member_outlines: bad shape V=%lld F=%lld nnz=%lld capacity=%lld (V, F < 2^31, 3 nnz < 2^31)",
                (long long)V, (long long)F, (long long)nnz, (long long)ring_vertex_cap);
  if (n_classes < 0 || n_classes > GR_MEMBER_MAX_CLASSES)
    return fail(c, GR_EINVAL, "gr_member_outlines: n_classes=%d outside [0, %d]", n_classes, (int)GR_MEMBER_MAX_CLASSES);
  if (!stats || !n_edges_h || !n_rings_h || !face_ptr || (V > 0 && !verts_q) || (F > 0 && !faces) || (nnz > 0 && !face_members) ||
      (ring_vertex_cap > 0 && (!ring_vertices || !ring_offsets || !ring_class || (V > 0 && !canon))))
    return fail(c, GR_EINVAL, "gr_member_outlines: null arrays");
  *n_edges_h = 0; *n_rings_h = 0;
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  GR_HIP(c, hipMemsetAsync(stats, 0, sizeof(uint64_t) * GR_OUTL_STAT_WORDS, s));
  unsigned long long *st = (unsigned long long *)stats;
  const OutlineOut out{canon, ring_vertices, ring_offsets, ring_class, ring_vertex_cap, n_edges_h, n_rings_h, st};
  return outline_trace(c, "gr_member_outlines", verts_q, V, 3 * nnz, n_classes, true, out, s,
                       [&](const int32_t *canon_d, unsigned long long *pair, uint32_t *cl) {   // one block at least: the table's ends
                         hipLaunchKernelGGL(k_outline_member_edges, dim3((unsigned)std::max<int64_t>(ceil_div(F, 256), 1)), dim3(256), 0,
                                            s, verts_q, V, faces, F, face_ptr, face_members, nnz, n_classes, canon_d, pair, cl, st);
                       });
}

}  // extern "C"

static int outline_trace(gr_ctx *c, const char *name, const int64_t *verts_q, int64_t V, int64_t N3, int n_classes, bool member_rows,
                         const OutlineOut &out, hipStream_t s,
                         const std::function<void(const int32_t *, unsigned long long *, uint32_t *)> &emit_edges) {
  unsigned long long *st = out.stats;
  const int vbits = std::max(bit_length(V - 1), 1), cbits = std::max(bit_length(n_classes), 1);

  // scratch A, sized by V and N3: head | canon [V] | the vertex sort or the edge sort and its runs | hipcub's temporaries
  Plan pa;
  const auto o_head = pa.array<unsigned long long>(GR_OUTL_HEAD_WORDS);
  const auto o_canon = pa.array<int32_t>(V);
  const size_t phase = pa.mark();
  // vertex phase: key [V] i64 | key_s [V] i64 | idx [V] | idx_s [V] | hp [V] | hp_max [V]
  const auto key = pa.array<int64_t>(V), key_s = pa.array<int64_t>(V);
  const auto idx = pa.array<int32_t>(V), idx_s = pa.array<int32_t>(V), hp = pa.array<int32_t>(V), hpm = pa.array<int32_t>(V);
  const SortPairs<int64_t, int32_t> sort_vertex(c, pa, V, 64);   // both passes: by y, then by x
  const InclusiveMax<int32_t> head_max(c, pa, V);
  pa.rewind(phase);
  // edge phase: pair [N3] u64 | pair_s [N3] u64 | cl [N3] | cl_s [N3] | flag [N3] | ex [N3] | ustart, surv, soff [N3 + 1]
  const auto e_pair = pa.array<unsigned long long>(N3), e_pair_s = pa.array<unsigned long long>(N3);
  const auto e_cl = pa.array<uint32_t>(N3), e_cl_s = pa.array<uint32_t>(N3);
  const auto e_flag = pa.array<int32_t>(N3), e_ex = pa.array<int32_t>(N3);
  const auto e_ustart = pa.array<int32_t>(N3 + 1), e_surv = pa.array<int32_t>(N3 + 1), e_soff = pa.array<int32_t>(N3 + 1);
  const SortPairs<unsigned long long, uint32_t> sort_pair(c, pa, N3, 31 + vbits);
  const SortPairs<uint32_t, unsigned long long> sort_class(c, pa, N3, cbits);
  const ExclusiveSum<int32_t> scan_flag(c, pa, N3), scan_surv(c, pa, N3 > 0 ? N3 + 1 : 0);   // (no edge: no scan)
  int rc = stage_acquire(c, c->stage, pa.finish(), s, "class-outline");
  if (rc != GR_OK) return rc;
  pa.base = c->stage.ptr;
  unsigned long long *head = o_head();
  int32_t *canon_d = o_canon();
  GR_HIP(c, hipMemsetAsync(head, 0, sizeof(unsigned long long) * GR_OUTL_HEAD_WORDS, s));

  if (V > 0) {   // X2
    const dim3 grid((unsigned)ceil_div(V, 256));
    hipLaunchKernelGGL(k_outline_vertex_keys, grid, dim3(256), 0, s, verts_q, V, key(), idx());
    GR_TRY(sort_vertex.run(key(), key_s(), idx(), idx_s(), s));   // by y
    hipLaunchKernelGGL(k_outline_vertex_gather, grid, dim3(256), 0, s, verts_q, V, (const int32_t *)idx_s(), key());
    GR_TRY(sort_vertex.run(key(), key_s(), idx_s(), idx(), s));   // then by x, stably
    hipLaunchKernelGGL(k_outline_vertex_heads, grid, dim3(256), 0, s, verts_q, V, (const int32_t *)idx(), hp());
    GR_TRY(head_max.run(hp(), hpm(), s));
    hipLaunchKernelGGL(k_outline_canon, grid, dim3(256), 0, s, V, (const int32_t *)idx(), (const int32_t *)hpm(), canon_d);
    GR_HIP(c, hipGetLastError());
  }

  int64_t E = 0, R = 0, runs = 0;
  unsigned long long *pair = e_pair(), *pair_s = e_pair_s();
  uint32_t *cl = e_cl(), *cl_s = e_cl_s();
  int32_t *flag = e_flag(), *ex = e_ex(), *ustart = e_ustart(), *surv = e_surv(), *soff = e_soff();
  if (member_rows && N3 > 0) {   // Y2: no word of a gap is uninitialised
    GR_HIP(c, hipMemsetAsync(pair, 0, sizeof(unsigned long long) * (size_t)N3, s));
    GR_HIP(c, hipMemsetAsync(cl, 0xFF, sizeof(uint32_t) * (size_t)N3, s));
  }
  if (member_rows || N3 > 0) {   // X3 or Y3
    emit_edges((const int32_t *)canon_d, pair, cl);
    GR_HIP(c, hipGetLastError());
  }
  if (N3 > 0) {   // X4
    const dim3 ge((unsigned)ceil_div(N3, 256));
    GR_TRY(sort_pair.run(pair, pair_s, cl, cl_s, s));    // by (from, to)
    GR_TRY(sort_class.run(cl_s, cl, pair_s, pair, s));   // then by class, stably
    hipLaunchKernelGGL(k_outline_run_heads, ge, dim3(256), 0, s, (const unsigned long long *)pair, (const uint32_t *)cl, N3,
                       n_classes, flag);
    GR_TRY(scan_flag.run(flag, ex, s));
    GR_HIP(c, hipMemsetAsync(ustart, 0, sizeof(int32_t) * (size_t)(N3 + 1), s));
    GR_HIP(c, hipMemsetAsync(surv, 0, sizeof(int32_t) * (size_t)(N3 + 1), s));
    hipLaunchKernelGGL(k_outline_run_starts, ge, dim3(256), 0, s, (const uint32_t *)cl, N3, n_classes, (const int32_t *)flag,
                       (const int32_t *)ex, ustart, head);
    hipLaunchKernelGGL(k_outline_cancel, ge, dim3(256), 0, s, (const unsigned long long *)pair, (const uint32_t *)cl,
                       (const int32_t *)ex, (const int32_t *)ustart, (const unsigned long long *)head, surv, st);
    GR_TRY(scan_surv.run(surv, soff, s));
    GR_HIP(c, hipGetLastError());
  }
  if (member_rows || N3 > 0) {   // the first synchronisation
    unsigned long long runs_h = 0, bad_rows_h = 0;
    int32_t edges_h = 0;
    if (N3 > 0) {
      GR_HIP(c, hipMemcpyAsync(&runs_h, head + GR_OUTL_HEAD_RUNS, sizeof(runs_h), hipMemcpyDeviceToHost, s));
      GR_HIP(c, hipMemcpyAsync(&edges_h, soff + N3, sizeof(edges_h), hipMemcpyDeviceToHost, s));   // surv is 0 behind the runs: the total
    }
    if (member_rows) GR_HIP(c, hipMemcpyAsync(&bad_rows_h, st + GR_OUTL_STAT_BAD_ROWS, sizeof(bad_rows_h), hipMemcpyDeviceToHost, s));
    GR_HIP(c, hipStreamSynchronize(s));
    if (bad_rows_h) return GR_OK;   // Y2: a malformed table ends here; the caller reads the word
    runs = (int64_t)runs_h; E = (int64_t)edges_h;
    if (runs < 0 || runs > N3 || E < 0 || E > N3) return fail(c, GR_EHIP, "%s: inconsistent edge counts", name);
  }
  *out.n_edges_h = E;

  const bool fill = out.cap > 0;
  if (E == 0) {   // no outline: an empty table
    if (fill) {
      GR_HIP(c, hipMemsetAsync(out.ring_offsets, 0, sizeof(int64_t), s));
      if (V > 0) GR_HIP(c, hipMemcpyAsync(out.canon, canon_d, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToDevice, s));
    }
    GR_HIP(c, hipStreamSynchronize(s));   // the scratch is free on return
    return GR_OK;
  }

  // scratch B, sized by E: efrom | ecls | succ | two sets of (nxt, mn, off) | kin, kin_s [E + 1] u64 | hipcub's temporaries
  Plan pb;
  const auto b_from = pb.array<int32_t>(E), b_cls = pb.array<int32_t>(E), b_succ = pb.array<int32_t>(E);
  Slot<int32_t> b_set[2][3];
  for (int k = 0; k < 6; ++k) b_set[k / 3][k % 3] = pb.array<int32_t>(E);
  const auto b_kin = pb.array<unsigned long long>(E + 1), b_kin_s = pb.array<unsigned long long>(E + 1);
  const SortPairs<unsigned long long, int32_t> sort_edge(c, pb, E, 31 + cbits);
  const ExclusiveSum<unsigned long long> scan_words(c, pb, E + 1);
  rc = stage_acquire(c, c->stage_b, pb.finish(), s, "class-outline ring");
  if (rc != GR_OK) return rc;
  pb.base = c->stage_b.ptr;
  int32_t *efrom = b_from(), *ecls = b_cls(), *succ = b_succ();
  int32_t *set[2][3];
  for (int k = 0; k < 6; ++k) set[k / 3][k % 3] = b_set[k / 3][k % 3]();
  unsigned long long *kin = b_kin(), *kin_s = b_kin_s();
  int32_t *vin = set[1][0], *vin_s = set[1][1];   // free until the first round writes the second set
  const dim3 gE((unsigned)ceil_div(E, 256)), gE1((unsigned)ceil_div(E + 1, 256));
  hipLaunchKernelGGL(k_outline_emit_edges, dim3((unsigned)ceil_div(runs, 256)), dim3(256), 0, s, (const unsigned long long *)pair,
                     (const uint32_t *)cl, (const int32_t *)ustart, (const int32_t *)surv, (const int32_t *)soff, runs, efrom, ecls,
                     kin, vin);
  GR_TRY(sort_edge.run(kin, kin_s, vin, vin_s, s));   // X5
  hipLaunchKernelGGL(k_outline_successor, gE, dim3(256), 0, s, (const int32_t *)vin_s, E, succ, set[0][1], set[0][2]);
  // X6: round r reads the successor table first, then its own doubled pointers
  int cur = 0;
  for (int r = 0; ((int64_t)1 << r) < E; ++r) {
    const int32_t *nxt = r == 0 ? succ : set[cur][0];
    hipLaunchKernelGGL(k_outline_round, gE, dim3(256), 0, s, nxt, (const int32_t *)set[cur][1], (const int32_t *)set[cur][2],
                       set[cur ^ 1][0], set[cur ^ 1][1], set[cur ^ 1][2], (uint32_t)1 << r, E);
    cur ^= 1;
  }
  const int32_t *mn = set[cur][1], *off = set[cur][2];
  unsigned long long *w = kin, *ws = kin_s;
  hipLaunchKernelGGL(k_outline_ring_words, gE1, dim3(256), 0, s, (const int32_t *)succ, mn, off, E, w);
  GR_TRY(scan_words.run(w, ws, s));
  GR_HIP(c, hipGetLastError());
  unsigned long long total = 0;
  GR_HIP(c, hipMemcpyAsync(&total, ws + E, sizeof(total), hipMemcpyDeviceToHost, s));
  GR_HIP(c, hipStreamSynchronize(s));
  R = (int64_t)(total & 0xFFFFFFFFull);
  *out.n_rings_h = R;
  if ((int64_t)(total >> 32) != E || R < 1 || 3 * R > E)
    return fail(c, GR_EHIP, "%s: the rings hold %llu of %lld edges in %lld rings", name, total >> 32, (long long)E, (long long)R);
  if (!fill) return GR_OK;
  if (E > out.cap)
    return fail(c, GR_EOVERFLOW, "%s: %lld ring vertices in %lld rings, the buffers hold %lld: call again with that capacity", name,
                (long long)E, (long long)R, (long long)out.cap);
  hipLaunchKernelGGL(k_outline_emit_rings, gE, dim3(256), 0, s, mn, off, (const int32_t *)efrom, (const int32_t *)ecls,
                     (const unsigned long long *)w, (const unsigned long long *)ws, E, out.ring_vertices, out.ring_offsets,
                     out.ring_class);
  GR_HIP(c, hipGetLastError());
  if (V > 0) GR_HIP(c, hipMemcpyAsync(out.canon, canon_d, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToDevice, s));
  GR_HIP(c, hipStreamSynchronize(s));   // the last use of the scratch: free on return, as for gr_ray_pairs
  return GR_OK;
}
