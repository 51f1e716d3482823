#pragma once
// geograypher_amd/csrc/ray_dev.hpp -- the ray record and the clamped closest points of two segments: ONE device function for the
// ray-pair graph (rays.hip: k_ray_pairs holds their distance against the threshold) and for the community points
// (communities.hip: k_community_points averages them).  Float64, compiled without contraction like the rest of the library.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// what k_ray_prep derives per ray, once: 64 bytes, the unit of the B tile in LDS
struct RayRec {
  double sx, sy, sz;   // start
  double ux, uy, uz;   // (end - start) / mag: NaN for a zero-length segment (0 / 0), which therefore meets no threshold
  double mag;          // |end - start|
  int32_t id;          // image the ray came from
  int32_t pad;
};

// the record of ray i (k_ray_prep, k_comm_ray_prep)
__device__ __forceinline__ RayRec ray_record(const double *__restrict__ starts, const double *__restrict__ ends, int64_t i, int32_t id) {
  RayRec r;
  r.sx = starts[3 * i]; r.sy = starts[3 * i + 1]; r.sz = starts[3 * i + 2];
  const double dx = ends[3 * i] - r.sx, dy = ends[3 * i + 1] - r.sy, dz = ends[3 * i + 2] - r.sz;
  r.mag = sqrt((dx * dx + dy * dy) + dz * dz);
  r.ux = dx / r.mag; r.uy = dy / r.mag; r.uz = dz / r.mag;
  r.id = id; r.pad = 0;
  return r;
}

// np.clip(x, 0, hi) as far as the result can matter: a NaN x stays NaN (a NaN `hi` comes with NaN directions, which make
// every point NaN anyway)
__device__ __forceinline__ double clip0(double x, double hi) {
  x = x < 0.0 ? 0.0 : x;
  return x > hi ? hi : x;
}

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
  return (ax * bx + ay * by) + az * bz;
}

// The closest points of segment A (this lane's ray) and segment B, both clamped to their segments.
// Non-parallel rays: the closest points of the two infinite lines are at parameters t0 = det(t, uB, n) / |n|^2 along A and
// t1 = det(t, uA, n) / |n|^2 along B, n = uA x uB, t = b0 - a0; a parameter outside [0, mag] is clamped, and then the OTHER
// point is the projection of the clamped one onto its segment: first B from the clamped A, then A from the updated B.
// Parallel rays (|n|^2 exactly 0): B's end points are projected on A's axis (d0, d1, measured from a0); B wholly before a0 or
// wholly behind a1 pairs that end of A with B's nearer end, otherwise A's point is d0 clamped and B's the foot of the
// perpendicular.  `ends` is read in the parallel case only.
__device__ __forceinline__ void segment_closest_points(const RayRec &a, const RayRec &b, const double *__restrict__ ends, int64_t i,
                                                       int64_t j, double &pax, double &pay, double &paz, double &pbx, double &pby,
                                                       double &pbz) {
  const double cx = a.uy * b.uz - a.uz * b.uy, cy = a.uz * b.ux - a.ux * b.uz, cz = a.ux * b.uy - a.uy * b.ux;
  const double cn = sqrt((cx * cx + cy * cy) + cz * cz);
  double denom = cn * cn;
  const bool parallel = denom == 0.0;
  if (parallel) denom = 1.0;
  const double tx = b.sx - a.sx, ty = b.sy - a.sy, tz = b.sz - a.sz;
  const double detA = dot3(ty * b.uz - tz * b.uy, tz * b.ux - tx * b.uz, tx * b.uy - ty * b.ux, cx, cy, cz);
  const double detB = dot3(ty * a.uz - tz * a.uy, tz * a.ux - tx * a.uz, tx * a.uy - ty * a.ux, cx, cy, cz);
  const double t0 = detA / denom, t1 = detB / denom;
  const double t0c = clip0(t0, a.mag), t1c = clip0(t1, b.mag);
  pax = a.sx + t0c * a.ux; pay = a.sy + t0c * a.uy; paz = a.sz + t0c * a.uz;
  pbx = b.sx + t1c * b.ux; pby = b.sy + t1c * b.uy; pbz = b.sz + t1c * b.uz;
  const bool oob_a = (t0 < 0.0) | (t0 > a.mag), oob_b = (t1 < 0.0) | (t1 > b.mag);
  {
    const double d = clip0(dot3(pax - b.sx, pay - b.sy, paz - b.sz, b.ux, b.uy, b.uz), b.mag);
    const double qx = b.sx + d * b.ux, qy = b.sy + d * b.uy, qz = b.sz + d * b.uz;
    pbx = oob_a ? qx : pbx; pby = oob_a ? qy : pby; pbz = oob_a ? qz : pbz;
  }
  {
    const double d = clip0(dot3(pbx - a.sx, pby - a.sy, pbz - a.sz, a.ux, a.uy, a.uz), a.mag);
    const double qx = a.sx + d * a.ux, qy = a.sy + d * a.uy, qz = a.sz + d * a.uz;
    pax = oob_b ? qx : pax; pay = oob_b ? qy : pay; paz = oob_b ? qz : paz;
  }
  if (parallel) {
    const double b1x = ends[3 * j], b1y = ends[3 * j + 1], b1z = ends[3 * j + 2];
    const double base = dot3(a.ux, a.uy, a.uz, a.sx, a.sy, a.sz);
    const double d0 = dot3(a.ux, a.uy, a.uz, b.sx, b.sy, b.sz) - base;
    const double d1 = dot3(a.ux, a.uy, a.uz, b1x, b1y, b1z) - base;
    const bool before = (d0 <= 0.0) & (d1 <= 0.0);
    const bool after = (d0 >= a.mag) & (d1 >= a.mag);
    if (before | after) {
      const bool near0 = fabs(d0) < fabs(d1);
      pbx = near0 ? b.sx : b1x; pby = near0 ? b.sy : b1y; pbz = near0 ? b.sz : b1z;
      if (after) { pax = ends[3 * i]; pay = ends[3 * i + 1]; paz = ends[3 * i + 2]; }
      else { pax = a.sx; pay = a.sy; paz = a.sz; }
    } else {
      const double tm = clip0(d0, a.mag);
      pax = a.sx + tm * a.ux; pay = a.sy + tm * a.uy; paz = a.sz + tm * a.uz;
      const double gx = b.sx - pax, gy = b.sy - pay, gz = b.sz - paz;
      const double al = dot3(gx, gy, gz, a.ux, a.uy, a.uz);
      pbx = pax + (gx - al * a.ux); pby = pay + (gy - al * a.uy); pbz = paz + (gz - al * a.uz);
    }
  }
}

// ... and their distance: what k_ray_pairs holds against the threshold
__device__ __forceinline__ double segment_distance(const RayRec &a, const RayRec &b, const double *__restrict__ ends, int64_t i, int64_t j) {
  double pax, pay, paz, pbx, pby, pbz;
  segment_closest_points(a, b, ends, i, j, pax, pay, paz, pbx, pby, pbz);
  const double ex = pax - pbx, ey = pay - pby, ez = paz - pbz;
  return sqrt((ex * ex + ey * ey) + ez * ez);
}

}  // namespace
