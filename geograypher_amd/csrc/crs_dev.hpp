#pragma once
// geograypher_amd/csrc/crs_dev.hpp -- the conversion of ONE point between the WGS84 coordinate reference systems (rules G1-G8 of
// DESIGN.md "CRS reprojection"), shared by crs.hip (k_reproject_points: a row per lane) and raster_warp.hip (k_warp_raster: the centre
// of a destination cell).  The constants, the two sides of a conversion (CrsSide, CrsArgs), wrap_pi, clenshaw, taup_of, convert, and
// the host's crs_side, which fills a CrsSide from the ABI's gr_crs.  Every floating-point operation is a float64 operation rounded on
// its own (the units are compiled with -ffp-contract=off); sqrt and the division are correctly rounded, the device library's sin,
// cos, tan, atan, atan2, sinh, cosh, asinh and atanh are not.  The 13 series constants come from crs_constants.hpp, which
// tools/make_crs_constants.py writes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "crs_constants.hpp"
#include "geograster.h"

namespace {

constexpr double kA = 6378137.0;
constexpr double kF = 1.0 / 298.257223563;
constexpr double kE2 = kF * (2.0 - kF);
constexpr double kB = kA * (1.0 - kF);
constexpr double kEp2B = kE2 / (1.0 - kE2) * kB;   // e'^2 b
constexpr double kE2A = kE2 * kA;
constexpr double kOneF = 1.0 - kF;
constexpr double kOneE2 = 1.0 - kE2;
constexpr double kPi = 3.14159265358979323846;
constexpr double kDeg = kPi / 180.0;
constexpr double kRad = 180.0 / kPi;
constexpr double kPoleR = 0x1p-51;   // G7: this close to the pole in the (sinh eta', cos xi') plane IS the pole
__constant__ double c_alpha[6] = GR_CRS_ALPHA;
__constant__ double c_beta[6] = GR_CRS_BETA;

enum { ST_OK = 0, ST_NONFINITE = 1, ST_BEYOND = 2, ST_BAD_FACE = 3 };

struct CrsSide {
  int kind;
  double lon0;   // radians
  double ka;     // k0 A
  double fe, fn;
};
struct CrsArgs {
  int64_t N, V;
  int face_mode, has_pre;
  double ecc;    // sqrt(e^2): sqrt is not constexpr
  double pre[12];
  CrsSide from, to;
};

// G6: an angle into (-pi, pi]
__device__ __forceinline__ double wrap_pi(double d) {
  d = d - (2.0 * kPi) * floor((d + kPi) / (2.0 * kPi));
  return d <= -kPi ? d + 2.0 * kPi : (d > kPi ? d - 2.0 * kPi : d);
}

// G5: sum_j sign coef_j sin(2 j (x + i y)), Clenshaw in real arithmetic
__device__ __forceinline__ void clenshaw(const double *coef, double sign, double x, double y, double &re, double &im) {
  const double s0 = sin(2.0 * x), c0 = cos(2.0 * x), sh0 = sinh(2.0 * y), ch0 = cosh(2.0 * y);
  const double ar = 2.0 * (c0 * ch0), ai = -2.0 * (s0 * sh0);
  double y1r = 0.0, y1i = 0.0, y2r = 0.0, y2i = 0.0;
#pragma unroll
  for (int j = 5; j >= 0; --j) {
    const double tr = ((ar * y1r - ai * y1i) - y2r) + sign * coef[j];
    const double ti = (ar * y1i + ai * y1r) - y2i;
    y2r = y1r; y2i = y1i; y1r = tr; y1i = ti;
  }
  const double zr = s0 * ch0, zi = c0 * sh0;
  re = zr * y1r - zi * y1i;
  im = zr * y1i + zi * y1r;
}

// tan of the conformal latitude from tan of the geodetic one
__device__ __forceinline__ double taup_of(double tau, double ecc) {
  const double tau1 = sqrt(1.0 + tau * tau);
  const double sig = sinh(ecc * atanh(ecc * (tau / tau1)));
  return tau * sqrt(1.0 + sig * sig) - sig * tau1;
}

// One point (x, y, z) of `from` -> `to`, in place; the status of the row.
__device__ __forceinline__ int convert(double &x, double &y, double &z, const CrsArgs &a) {
  if (a.has_pre) {   // G1
    const double px = ((a.pre[0] * x + a.pre[1] * y) + a.pre[2] * z) + a.pre[3];
    const double py = ((a.pre[4] * x + a.pre[5] * y) + a.pre[6] * z) + a.pre[7];
    const double pz = ((a.pre[8] * x + a.pre[9] * y) + a.pre[10] * z) + a.pre[11];
    x = px; y = py; z = pz;
  }
  int status = (isfinite(x) && isfinite(y) && isfinite(z)) ? ST_OK : ST_NONFINITE;
  double phi, lam, h;
  if (a.from.kind == GR_CRS_ECEF) {   // G3
    const double p = sqrt(x * x + y * y);
    if (p == 0.0 && z == 0.0) status = ST_NONFINITE;
    double u = z * kA, v = p * kB;
    double r = sqrt(u * u + v * v);
    double sb = u / r, cb = v / r, s = 0.0, c = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      s = z + kEp2B * ((sb * sb) * sb);
      c = p - kE2A * ((cb * cb) * cb);
      u = kOneF * s; v = c;
      r = sqrt(u * u + v * v);
      sb = u / r; cb = v / r;
    }
    r = sqrt(s * s + c * c);
    const double sp = s / r, cp = c / r;
    phi = atan2(s, c);
    lam = p == 0.0 ? 0.0 : atan2(y, x);
    h = (p * cp + z * sp) - kA * sqrt(1.0 - kE2 * (sp * sp));
  } else if (a.from.kind == GR_CRS_GEOGRAPHIC) {
    if (!(fabs(y) <= 90.0) && status == ST_OK) status = ST_NONFINITE;
    phi = y * kDeg; lam = x * kDeg; h = z;
  } else {   // G7
    const double xi = (y - a.from.fn) / a.from.ka, eta = (x - a.from.fe) / a.from.ka;
    double dr, di;
    clenshaw(c_beta, -1.0, xi, eta, dr, di);
    const double xip = xi + dr, etap = eta + di;
    const double sh = sinh(etap), cx = cos(xip), sx = sin(xip);
    const double r = sqrt(sh * sh + cx * cx);
    const bool pole = r <= kPoleR;
    if (!pole && !(cx > 0.0) && status == ST_OK) status = ST_BEYOND;
    const double taup = sx / r;
    double tau = taup / kOneE2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double tau1 = sqrt(1.0 + tau * tau);
      const double sig = sinh(a.ecc * atanh(a.ecc * (tau / tau1)));
      const double ti = tau * sqrt(1.0 + sig * sig) - sig * tau1;
      tau = tau + ((taup - ti) / sqrt(1.0 + ti * ti)) * ((1.0 + kOneE2 * (tau * tau)) / (kOneE2 * tau1));
    }
    phi = pole ? (sx < 0.0 ? -kPi / 2.0 : kPi / 2.0) : atan(tau);
    lam = wrap_pi(a.from.lon0 + (pole ? 0.0 : atan2(sh, cx)));
    h = z;
  }
  if (a.to.kind == GR_CRS_ECEF) {   // G4
    const double sp = sin(phi), cp = cos(phi), sl = sin(lam), cl = cos(lam);
    const double n = kA / sqrt(1.0 - kE2 * (sp * sp));
    const double q = (n + h) * cp;
    x = q * cl; y = q * sl; z = (n * kOneE2 + h) * sp;
  } else if (a.to.kind == GR_CRS_GEOGRAPHIC) {
    x = wrap_pi(lam) * kRad; y = phi * kRad; z = h;
  } else {   // G5, G6
    const double d = wrap_pi(lam - a.to.lon0);
    if (!(fabs(d) < kPi / 2.0) && status == ST_OK) status = ST_BEYOND;
    const double taup = taup_of(tan(phi), a.ecc);
    const double cd = cos(d);
    const double xi = atan2(taup, cd);
    const double eta = asinh(sin(d) / sqrt(taup * taup + cd * cd));
    double dr, di;
    clenshaw(c_alpha, 1.0, xi, eta, dr, di);
    x = a.to.fe + a.to.ka * (eta + di);
    y = a.to.fn + a.to.ka * (xi + dr);
    z = h;
  }
  return status;
}

// false: an unknown kind, or a transverse Mercator with a parameter that is not finite or k0 <= 0
inline bool crs_side(const gr_crs *in, CrsSide &out) {
  out.kind = in->kind;
  out.lon0 = 0.0; out.ka = 1.0; out.fe = 0.0; out.fn = 0.0;
  if (in->kind == GR_CRS_ECEF || in->kind == GR_CRS_GEOGRAPHIC) return true;
  if (in->kind != GR_CRS_TM) return false;
  if (!(in->k0 > 0.0) || !std::isfinite(in->k0) || !std::isfinite(in->lon0) || !std::isfinite(in->false_easting) ||
      !std::isfinite(in->false_northing))
    return false;
  out.lon0 = in->lon0 * kDeg;
  out.ka = in->k0 * GR_CRS_RECT_RADIUS;
  out.fe = in->false_easting; out.fn = in->false_northing;
  return true;
}

}  // namespace
