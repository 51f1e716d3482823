// geograypher_amd/csrc/terrain.hip -- raster samples under the mesh: the value of a (B, H, W) raster at every face centre or
// vertex, the height of the query point above band 0 and, optionally, the ground relabel of label_ground_class
// (gr_sample_raster; the rule-set is DESIGN.md "Raster samples", T1-T7).  Needs no uploaded mesh and no context scratch.
//
// Shape: a gather, one query per lane in a grid-stride loop.  A lane reads its three vertex indices and nine coordinates (one
// vertex in vertex mode), forms the centre, finds its cell with the six inverse coefficients and reads B samples.  Every
// floating-point operation is a float64 operation rounded on its own (the unit is compiled with -ffp-contract=off like the rest
// of the library), in the order T3-T6 write down, so that the results are bit-equal to numpy applying the same operations.
// The inside test is made on the DOUBLES, before anything is converted to an integer: NaN, infinities and 1e300 are outside.
// Nothing is read through an index that was not checked: a face with a vertex outside [0, V) reads no vertex and no sample
// (load_face).  The face load and the statistics reductions (integers, one atomic per wave and word) are geom_dev.hpp's.
#include "geom_dev.hpp"
#include "gr_internal.hpp"

namespace {
using namespace grimpl;

struct SampleArgs {
  int64_t N, V;
  int B, H, W;
  int face_mode;     // 1: a query per face (the centre of its three vertices), 0: a query per vertex
  int has_nodata;
  int only_existing; // relabel: only labels that are finite
  int relabel;       // 1: labels != null
  double ia, ib, ic, id, ie, jf;   // inverse transform: col = x ia + y ib + ic, row = x id + y ie + jf
  double nodata, fill, threshold, ground_id;
};

// pts [V][3]; faces [N][3] or null; data [B][H][W]; values [N][B], height [N], labels [N]: each may be null;
// stats [GR_RS_STAT_WORDS].
template <typename T>
__global__ __launch_bounds__(256) void k_sample_raster(const double *__restrict__ pts, const int32_t *__restrict__ faces,
                                                       const T *__restrict__ data, double *__restrict__ values,
                                                       double *__restrict__ height, double *__restrict__ labels,
                                                       unsigned long long *__restrict__ stats, SampleArgs a) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t stride = (int64_t)gridDim.x * 256;
  unsigned int n_inside = 0, n_nodata = 0, n_ground = 0, n_bad = 0;   // per lane at most N / stride + 1 <= 2^18 + 1 (the launcher's grid): a wave's sum fits 32 bits
  const double outside = a.has_nodata ? a.nodata : 0.0;   // T5: what a boundless read fills with
  const int64_t plane = (int64_t)a.H * a.W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.N; i += stride) {
    double x = 0.0, y = 0.0, z = 0.0;
    bool bad = false;
    if (a.face_mode) {
      int64_t v0, v1, v2;
      bad = !load_face(faces, i, a.V, v0, v1, v2);
      if (!bad) {
        const double *p0 = pts + v0 * 3, *p1 = pts + v1 * 3, *p2 = pts + v2 * 3;
        x = ((p0[0] + p1[0]) + p2[0]) / 3.0;   // T3
        y = ((p0[1] + p1[1]) + p2[1]) / 3.0;
        z = ((p0[2] + p1[2]) + p2[2]) / 3.0;
      }
    } else {
      x = pts[i * 3]; y = pts[i * 3 + 1]; z = pts[i * 3 + 2];   // i < N = V
    }
    // T4: the cell, decided on the doubles
    const double cf = floor((x * a.ia + y * a.ib) + a.ic), rf = floor((x * a.id + y * a.ie) + a.jf);
    const bool inside = !bad && cf >= 0.0 && cf < (double)a.W && rf >= 0.0 && rf < (double)a.H;
    const int64_t cell = inside ? (int64_t)rf * a.W + (int64_t)cf : 0;   // < H W: the conversion is of a value in range
    bool hit = false;
    double first = 0.0;
    for (int b = 0; b < a.B; ++b) {
      double v = inside ? (double)data[(int64_t)b * plane + cell] : outside;   // T5
      if (a.has_nodata && v == a.nodata) { v = a.fill; hit = true; }
      if (values) values[i * a.B + b] = v;
      if (b == 0) first = v;
    }
    // T6; a face that names a missing vertex has no height
    const double h = bad ? __builtin_nan("") : z - first;
    if (height) height[i] = h;
    if (a.relabel && h < a.threshold) {   // T7: NaN compares false
      if (!a.only_existing || isfinite(labels[i])) { labels[i] = a.ground_id; ++n_ground; }
    }
    n_inside += inside ? 1u : 0u;
    n_nodata += (hit && !bad) ? 1u : 0u;
    n_bad += bad ? 1u : 0u;
  }
  stat_add_u32(stats, GR_RS_STAT_INSIDE, n_inside, lane);
  stat_add_u32(stats, GR_RS_STAT_NODATA, n_nodata, lane);
  stat_add_u32(stats, GR_RS_STAT_GROUND, n_ground, lane);
  stat_add_u32(stats, GR_RS_STAT_BAD_FACES, n_bad, lane);
}

}  // namespace

extern "C" {

int gr_sample_raster(gr_ctx *c, const double *points, int64_t V, const int32_t *faces, int64_t F, const void *raster,
                     int raster_dtype, int B, int H, int W, const double *inverse6_h, int has_nodata, double nodata, double fill,
                     double *values, double *height, double *labels_inout, double threshold, double ground_id, int flags,
                     uint64_t *stats, void *stream) {
  if (!c) return GR_EINVAL;
  if (V < 0 || F < 0 || V > 0x7FFFFFFFll || F > 0x7FFFFFFFll * 256)
    return fail(c, GR_EINVAL, "gr_sample_raster: bad shape V=%lld F=%lld", (long long)V, (long long)F);
  if (B < 1 || H < 1 || W < 1) return fail(c, GR_EINVAL, "gr_sample_raster: bad raster shape B=%d H=%d W=%d (each >= 1)", B, H, W);
  if (raster_dtype != GR_DTYPE_F32 && raster_dtype != GR_DTYPE_F64)
    return fail(c, GR_EINVAL, "gr_sample_raster: raster dtype %d is not GR_DTYPE_F32 / GR_DTYPE_F64", raster_dtype);
  if (!faces && F > 0) return fail(c, GR_EINVAL, "gr_sample_raster: null faces with F=%lld (vertex mode takes F = 0)", (long long)F);
  if (!raster || !inverse6_h || !stats || (V > 0 && !points)) return fail(c, GR_EINVAL, "gr_sample_raster: null arrays");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  GR_HIP(c, hipMemsetAsync(stats, 0, sizeof(uint64_t) * GR_RS_STAT_WORDS, s));
  SampleArgs a;
  a.face_mode = faces ? 1 : 0;
  a.N = faces ? F : V; a.V = V;
  if (a.N == 0) return GR_OK;
  a.B = B; a.H = H; a.W = W;
  a.has_nodata = has_nodata ? 1 : 0;
  a.relabel = labels_inout ? 1 : 0;
  a.only_existing = (flags & GR_RS_FLAG_ONLY_EXISTING) ? 1 : 0;
  a.ia = inverse6_h[0]; a.ib = inverse6_h[1]; a.ic = inverse6_h[2]; a.id = inverse6_h[3]; a.ie = inverse6_h[4]; a.jf = inverse6_h[5];
  a.nodata = nodata; a.fill = fill; a.threshold = threshold; a.ground_id = ground_id;
  // grid-stride: enough workgroups to fill the chip several times over, not one per 256 queries of a 100 M face mesh
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(a.N, 256), 256 * 32);
  if (raster_dtype == GR_DTYPE_F32)
    hipLaunchKernelGGL(k_sample_raster<float>, dim3(grid), dim3(256), 0, s, points, faces, (const float *)raster, values, height,
                       labels_inout, (unsigned long long *)stats, a);
  else
    hipLaunchKernelGGL(k_sample_raster<double>, dim3(grid), dim3(256), 0, s, points, faces, (const double *)raster, values, height,
                       labels_inout, (unsigned long long *)stats, a);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

}  // extern "C"
