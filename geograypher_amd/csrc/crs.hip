// geograypher_amd/csrc/crs.hip -- points between the WGS84 coordinate reference systems: ECEF (EPSG:4978), geographic (lon, lat in
// degrees, ellipsoidal height) and a transverse Mercator with explicit parameters (the UTM zones), one ellipsoid and no datum shift
// (gr_reproject_points; the rule-set is DESIGN.md "CRS reprojection", G1-G9).  Replaces the pyproj.Transformer of reproject_CRS,
// get_mesh_points_in_CRS and get_camera_location.  Needs no uploaded mesh and no context scratch.
//
// Shape: a map, one output row per lane in a grid-stride loop (k_sample_raster's).  A lane reads its point -- in face mode the three
// vertices of its face, each reprojected, then ((p0 + p1) + p2) / 3 --, applies the optional 3 x 4 pre-transform, converts to
// geographic radians (G3 / G7) and from there to the target (G4 / G5).  No loop depends on the data: Bowring's start and three
// refinements without a trigonometric call, six Krueger terms summed by Clenshaw in real arithmetic, three Newton steps from the
// conformal to the geodetic latitude.  Every floating-point operation is a float64 operation rounded on its own (the unit is
// compiled with -ffp-contract=off like the rest of the library), in the order G1-G8 write down; sqrt and the division are
// correctly rounded, the device library's sin, cos, tan, atan, atan2, sinh, cosh, asinh and atanh are NOT, so this stage agrees
// with its numpy statement within the tolerance of G9 and not bit for bit.  A row's result depends on the row alone: not on V, not
// on its position, not on scheduling.  Nothing is read through an index that was not checked (load_face).  The 13 series constants
// come from crs_constants.hpp, which tools/make_crs_constants.py writes.  The conversion of one point (CrsSide, CrsArgs, wrap_pi,
// clenshaw, taup_of, convert, crs_side) is crs_dev.hpp's, which raster_warp.hip includes as well.
#include "crs_dev.hpp"
#include "geom_dev.hpp"
#include "gr_internal.hpp"

namespace {
using namespace grimpl;

// pts [V][3]; faces [N][3] or null; out [N][3] (vertex mode: may be pts); stats [GR_CRS_STAT_WORDS].
__global__ __launch_bounds__(256) void k_reproject_points(const double *pts, const int32_t *__restrict__ faces, double *out,
                                                          unsigned long long *__restrict__ stats, CrsArgs a) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t stride = (int64_t)gridDim.x * 256;
  unsigned int n_nonfinite = 0, n_beyond = 0, n_bad = 0;   // per lane at most N / stride + 1 <= 2^18 + 1: a wave's sum fits 32 bits
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.N; i += stride) {
    double x, y, z;
    int status;
    if (a.face_mode) {   // G8
      int64_t v[3];
      status = load_face(faces, i, a.V, v[0], v[1], v[2]) ? ST_OK : ST_BAD_FACE;
      double q[3][3] = {};
      if (status == ST_OK) {
        bool nonfinite = false, beyond = false;
        for (int k = 0; k < 3; ++k) {
          q[k][0] = pts[v[k] * 3]; q[k][1] = pts[v[k] * 3 + 1]; q[k][2] = pts[v[k] * 3 + 2];
          const int st = convert(q[k][0], q[k][1], q[k][2], a);
          nonfinite |= st == ST_NONFINITE;
          beyond |= st == ST_BEYOND;
        }
        status = nonfinite ? ST_NONFINITE : (beyond ? ST_BEYOND : ST_OK);
      }
      x = ((q[0][0] + q[1][0]) + q[2][0]) / 3.0;
      y = ((q[0][1] + q[1][1]) + q[2][1]) / 3.0;
      z = ((q[0][2] + q[1][2]) + q[2][2]) / 3.0;
    } else {
      x = pts[i * 3]; y = pts[i * 3 + 1]; z = pts[i * 3 + 2];   // i < N = V
      status = convert(x, y, z, a);
    }
    if (status != ST_OK) x = y = z = nan;
    out[i * 3] = x; out[i * 3 + 1] = y; out[i * 3 + 2] = z;
    n_nonfinite += status == ST_NONFINITE ? 1u : 0u;
    n_beyond += status == ST_BEYOND ? 1u : 0u;
    n_bad += status == ST_BAD_FACE ? 1u : 0u;
  }
  stat_add_u32(stats, GR_CRS_STAT_NONFINITE, n_nonfinite, lane);
  stat_add_u32(stats, GR_CRS_STAT_BEYOND, n_beyond, lane);
  stat_add_u32(stats, GR_CRS_STAT_BAD_FACES, n_bad, lane);
}

}  // namespace

extern "C" {

int gr_reproject_points(gr_ctx *c, const double *points, int64_t V, const int32_t *faces, int64_t F, const double *pre16_h,
                        const gr_crs *from_h, const gr_crs *to_h, double *out, uint64_t *stats, void *stream) {
  if (!c) return GR_EINVAL;
  if (V < 0 || F < 0 || V > 0x7FFFFFFFll || F > 0x7FFFFFFFll * 256)
    return fail(c, GR_EINVAL, "gr_reproject_points: bad shape V=%lld F=%lld", (long long)V, (long long)F);
  if (!faces && F > 0) return fail(c, GR_EINVAL, "gr_reproject_points: null faces with F=%lld (vertex mode takes F = 0)", (long long)F);
  const int64_t N = faces ? F : V;
  if (!from_h || !to_h || !stats || (V > 0 && !points) || (N > 0 && !out)) return fail(c, GR_EINVAL, "gr_reproject_points: null arrays");
  if (faces && N > 0 && out == points) return fail(c, GR_EINVAL, "gr_reproject_points: in place only without faces");
  CrsArgs a;
  if (!crs_side(from_h, a.from))
    return fail(c, GR_EINVAL, "gr_reproject_points: bad source CRS (kind %d, k0 %g)", (int)from_h->kind, from_h->k0);
  if (!crs_side(to_h, a.to))
    return fail(c, GR_EINVAL, "gr_reproject_points: bad target CRS (kind %d, k0 %g)", (int)to_h->kind, to_h->k0);
  if (pre16_h && a.from.kind != GR_CRS_ECEF)
    return fail(c, GR_EINVAL, "gr_reproject_points: a pre-transform needs an ECEF source, got kind %d", a.from.kind);
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  GR_HIP(c, hipMemsetAsync(stats, 0, sizeof(uint64_t) * GR_CRS_STAT_WORDS, s));
  if (N == 0) return GR_OK;
  a.N = N; a.V = V;
  a.face_mode = faces ? 1 : 0;
  a.has_pre = pre16_h ? 1 : 0;
  for (int k = 0; k < 12; ++k) a.pre[k] = pre16_h ? pre16_h[k] : 0.0;
  a.ecc = std::sqrt(kE2);
  // grid-stride: enough workgroups to fill the chip several times over (GR_CRS_MAX_GROUPS of 256 lanes)
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(N, 256), GR_CRS_MAX_GROUPS);
  hipLaunchKernelGGL(k_reproject_points, dim3(grid), dim3(256), 0, s, points, faces, out, (unsigned long long *)stats, a);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

}  // extern "C"
