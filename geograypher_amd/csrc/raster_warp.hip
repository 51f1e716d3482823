// geograypher_amd/csrc/raster_warp.hip -- a georeferenced raster resampled onto a window of another grid, in the same or in another
// WGS84 CRS (gr_warp_raster; the rule-set is DESIGN.md section 8t, W1-W9).  Replaces rasterio.warp.reproject behind the reference's
// reproject_raster and the resampled read of load_downsampled_raster_data.  Needs no uploaded mesh and no context scratch.
//
// Shape: a map, one lane per destination cell.  A workgroup of 256 lanes takes a strip, 256 consecutive columns of ONE row of the
// window, so each of its four waves stores 64 consecutive cells of a band plane at a time; at most WARP_MAX_GROUPS workgroups
// stride over the strips and keep their counts in registers, so the statistics cost one atomic per wave and word at the end (an
// atomic per strip on the one word that every cell counts in is a serial chain: 12 ns each, measured).  A lane forms its cell's
// centre (W2), takes it to the source's CRS (W3: crs_dev.hpp's convert, the one k_reproject_points calls) and to source cell units
// (W4) ONCE, then walks the bands: a nearest sample (W5) or four taps (W6) per band, converted to the destination's type (W7).
// The same-CRS and the cross-CRS kernel are separate instantiations: the first is a handful of multiplications and is bound by
// memory, the second carries the conversion's registers and is bound by its float64 library calls.  The source and destination
// types are uniform run-time switches in the load and the store: a uint8 source is read as bytes.  Every floating-point operation
// is a float64 operation rounded on its own (-ffp-contract=off).  A cell's result depends on the cell alone (W9): no atomics on
// data, the statistics are integer sums.  Nothing is read through an index that was not checked against [0, H) x [0, W) on the
// doubles first; every cell of the window is stored.
#include "crs_dev.hpp"
#include "geom_dev.hpp"
#include "gr_internal.hpp"

namespace {
using namespace grimpl;

constexpr int WARP_SEG = 256;        // columns of a row per workgroup
constexpr int WARP_MAX_SIDE = 1 << 23;
constexpr int WARP_MAX_GROUPS = 8192;   // workgroups of the launch: they stride over the strips (GR_CRS_MAX_GROUPS' figure)

struct WarpArgs {
  const void *data;
  void *out;
  int B, H, W;
  int src_dtype, dst_dtype, has_nodata;
  int col_off, row_off, width, height;
  int segs;                 // strips per row of the window
  int64_t strips;           // segs * height
  double t[6];              // destination: x = (t0 col + t1 row) + t2, y = (t3 col + t4 row) + t5
  double inv[6];            // source: u = (i0 x + i1 y) + i2, v = (i3 x + i4 y) + i5
  double src_nodata, dst_nodata;
  CrsArgs crs;              // from: the destination's CRS, to: the source's
};

__device__ __forceinline__ double warp_load(const void *data, int dtype, int64_t i) {
  if (dtype == GR_DTYPE_U8) return (double)((const uint8_t *)data)[i];
  if (dtype == GR_DTYPE_F32) return (double)((const float *)data)[i];
  return ((const double *)data)[i];
}

// W7
__device__ __forceinline__ void warp_store(void *out, int dtype, int64_t i, double v) {
  if (dtype == GR_DTYPE_U8) {
    const double q = floor(v + 0.5);
    ((uint8_t *)out)[i] = !(q >= 0.0) ? (uint8_t)0 : (q > 255.0 ? (uint8_t)255 : (uint8_t)(int)q);
  } else if (dtype == GR_DTYPE_F32) {
    ((float *)out)[i] = (float)v;
  } else {
    ((double *)out)[i] = v;
  }
}

// data [B][H][W]; out [B][height][width]; stats [GR_WARP_STAT_WORDS].  A strip is 256 columns of a row of the window; the workgroups
// stride over the a.strips = segs * height strips.
template <bool CROSS, bool BILINEAR>
__global__ __launch_bounds__(256) void k_warp_raster(unsigned long long *__restrict__ stats, WarpArgs a) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t plane = (int64_t)a.H * a.W, oplane = (int64_t)a.height * a.width;
  const double W = (double)a.W, H = (double)a.H;
  // per lane at most strips / gridDim.x + 1 <= 2^18 + 1 cells (the launcher's grid): a wave's sum fits 32 bits
  unsigned int n_cells = 0, n_outside = 0, n_nonfinite = 0, n_beyond = 0, n_nodata = 0, n_den_zero = 0;
  for (int64_t strip = blockIdx.x; strip < a.strips; strip += gridDim.x) {
    const int r = (int)(strip / a.segs);                               // < height
    const int c = (int)(strip % a.segs) * WARP_SEG + (int)threadIdx.x;
    if (c >= a.width) continue;
    // W2: an integer below 2^23 in magnitude plus 0.5 is exact
    const double col = (double)(a.col_off + c) + 0.5, row = (double)(a.row_off + r) + 0.5;
    double xs = (a.t[0] * col + a.t[1] * row) + a.t[2];
    double ys = (a.t[3] * col + a.t[4] * row) + a.t[5];
    int status = ST_OK;
    if (CROSS) {   // W3
      double zs = 0.0;
      status = convert(xs, ys, zs, a.crs);
    }
    const double u = (a.inv[0] * xs + a.inv[1] * ys) + a.inv[2];   // W4
    const double v = (a.inv[3] * xs + a.inv[4] * ys) + a.inv[5];
    const int64_t o = (int64_t)r * a.width + c;
    bool outside = false, met_nodata = false, den_zero = false;
    if (!BILINEAR) {   // W5
      const double cf = floor(u), rf = floor(v);
      const bool inside = status == ST_OK && cf >= 0.0 && cf < W && rf >= 0.0 && rf < H;   // NaN compares false
      outside = status == ST_OK && !inside;
      const int64_t cell = inside ? (int64_t)rf * a.W + (int64_t)cf : 0;   // the conversion is of a value in range
      for (int b = 0; b < a.B; ++b) {
        double s = a.dst_nodata;
        if (inside) {
          s = warp_load(a.data, a.src_dtype, (int64_t)b * plane + cell);
          if ((a.has_nodata && s == a.src_nodata) || s != s) { s = a.dst_nodata; met_nodata = true; }
        }
        warp_store(a.out, a.dst_dtype, (int64_t)b * oplane + o, s);
      }
    } else {   // W6
      const double up = u - 0.5, vp = v - 0.5;
      const double c0 = floor(up), r0 = floor(vp);
      const double fx = up - c0, fy = vp - r0;
      const bool ok = status == ST_OK;
      const bool cin0 = ok && c0 >= 0.0 && c0 < W, cin1 = ok && c0 >= -1.0 && c0 < W - 1.0;
      const bool rin0 = r0 >= 0.0 && r0 < H, rin1 = r0 >= -1.0 && r0 < H - 1.0;
      const bool in[4] = {rin0 && cin0, rin0 && cin1, rin1 && cin0, rin1 && cin1};
      const bool any = in[0] || in[1] || in[2] || in[3];
      outside = ok && !any;
      // a tap outside the raster is never read: its index is the raster's first cell
      const int64_t ci0 = cin0 ? (int64_t)c0 : 0, ci1 = cin1 ? (int64_t)c0 + 1 : 0;
      const int64_t ri0 = rin0 ? (int64_t)r0 : 0, ri1 = rin1 ? (int64_t)r0 + 1 : 0;
      const int64_t at[4] = {ri0 * a.W + ci0, ri0 * a.W + ci1, ri1 * a.W + ci0, ri1 * a.W + ci1};
      const double gx = 1.0 - fx, gy = 1.0 - fy;
      const double w[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
      for (int b = 0; b < a.B; ++b) {
        double num = 0.0, den = 0.0;
        int taking = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!in[k]) continue;
          const double s = warp_load(a.data, a.src_dtype, (int64_t)b * plane + at[k]);
          if ((a.has_nodata && s == a.src_nodata) || s != s) { met_nodata = true; continue; }
          num = num + w[k] * s;
          den = den + w[k];
          ++taking;
        }
        double s = a.dst_nodata;
        if (any) {
          if (den == 0.0) den_zero = true;
          else s = taking == 4 ? num : num / den;
        }
        warp_store(a.out, a.dst_dtype, (int64_t)b * oplane + o, s);
      }
    }
    n_cells += 1u;
    n_outside += outside ? 1u : 0u;
    n_nonfinite += status == ST_NONFINITE ? 1u : 0u;
    n_beyond += status == ST_BEYOND ? 1u : 0u;
    n_nodata += met_nodata ? 1u : 0u;
    n_den_zero += den_zero ? 1u : 0u;
  }
  // one atomic per wave and word, none for a word the wave has nothing to report in
  stat_add_u32(stats, GR_WARP_STAT_CELLS, n_cells, lane);
  stat_add_u32(stats, GR_WARP_STAT_OUTSIDE, n_outside, lane);
  if (CROSS) {
    stat_add_u32(stats, GR_WARP_STAT_NONFINITE, n_nonfinite, lane);
    stat_add_u32(stats, GR_WARP_STAT_BEYOND, n_beyond, lane);
  }
  stat_add_u32(stats, GR_WARP_STAT_NODATA, n_nodata, lane);
  if (BILINEAR) stat_add_u32(stats, GR_WARP_STAT_DEN_ZERO, n_den_zero, lane);
}

bool finite6(const double *m) {
  for (int k = 0; k < 6; ++k)
    if (!std::isfinite(m[k])) return false;
  return true;
}

size_t dtype_bytes(int dtype) { return dtype == GR_DTYPE_U8 ? 1 : (dtype == GR_DTYPE_F32 ? 4 : 8); }
bool known_dtype(int dtype) { return dtype == GR_DTYPE_U8 || dtype == GR_DTYPE_F32 || dtype == GR_DTYPE_F64; }

}  // namespace

extern "C" {

int gr_warp_raster(gr_ctx *c, const gr_warp_raster_args *args_h) {
  if (!c) return GR_EINVAL;
  if (!args_h) return fail(c, GR_EINVAL, "gr_warp_raster: null descriptor");
  const gr_warp_raster_args g = *args_h;   // read once, here: the caller may reuse the descriptor when the call returns
  if (g.B < 1 || g.B > GR_WARP_MAX_BANDS || g.H < 1 || g.W < 1 || g.H >= WARP_MAX_SIDE || g.W >= WARP_MAX_SIDE)
    return fail(c, GR_EINVAL, "gr_warp_raster: bad source shape B=%d H=%d W=%d (1 <= B <= %d, 1 <= H, W < 2^23)", g.B, g.H, g.W, (int)GR_WARP_MAX_BANDS);
  if (!known_dtype(g.src_dtype) || !known_dtype(g.dst_dtype))
    return fail(c, GR_EINVAL, "gr_warp_raster: src_dtype=%d, dst_dtype=%d: each GR_DTYPE_U8, GR_DTYPE_F32 or GR_DTYPE_F64", g.src_dtype, g.dst_dtype);
  if (g.resampling != GR_WARP_NEAREST && g.resampling != GR_WARP_BILINEAR)
    return fail(c, GR_EINVAL, "gr_warp_raster: resampling=%d is neither GR_WARP_NEAREST nor GR_WARP_BILINEAR", g.resampling);
  GR_TRY(check_window(c, "gr_warp_raster", g.col_off, g.row_off, g.width, g.height));
  const int64_t segs = ceil_div((int64_t)g.width, (int64_t)WARP_SEG);
  if (segs * g.height > 0x7FFFFFFFll) return fail(c, GR_EINVAL, "gr_warp_raster: a window of %d x %d cells is too large for one call", g.width, g.height);
  if (!g.data || !g.out || !g.stats || !g.src_inverse6_h || !g.dst_transform6_h) return fail(c, GR_EINVAL, "gr_warp_raster: null arrays");
  if (!finite6(g.src_inverse6_h) || !finite6(g.dst_transform6_h)) return fail(c, GR_EINVAL, "gr_warp_raster: a transform coefficient is not finite");
  WarpArgs a;
  a.crs = CrsArgs();
  if (!g.same_crs) {
    if (!g.src_crs_h || !g.dst_crs_h) return fail(c, GR_EINVAL, "gr_warp_raster: null CRS with same_crs = 0");
    if (g.src_crs_h->kind == GR_CRS_ECEF || g.dst_crs_h->kind == GR_CRS_ECEF)
      return fail(c, GR_EINVAL, "gr_warp_raster: an ECEF side: a raster is planar or geographic");
    if (!crs_side(g.dst_crs_h, a.crs.from))
      return fail(c, GR_EINVAL, "gr_warp_raster: bad destination CRS (kind %d, k0 %g)", (int)g.dst_crs_h->kind, g.dst_crs_h->k0);
    if (!crs_side(g.src_crs_h, a.crs.to))
      return fail(c, GR_EINVAL, "gr_warp_raster: bad source CRS (kind %d, k0 %g)", (int)g.src_crs_h->kind, g.src_crs_h->k0);
    a.crs.ecc = std::sqrt(kE2);
  }
  const size_t src_item = dtype_bytes(g.src_dtype), dst_item = dtype_bytes(g.dst_dtype);
  if ((uintptr_t)g.data % src_item || (uintptr_t)g.out % dst_item || (uintptr_t)g.stats % 8)
    return fail(c, GR_EINVAL, "gr_warp_raster: a float64 array is not 8-byte aligned (or a float32 array not 4-byte)");
  const uintptr_t d0 = (uintptr_t)g.data, d1 = d0 + src_item * (size_t)g.B * (size_t)g.H * (size_t)g.W;
  const uintptr_t o0 = (uintptr_t)g.out, o1 = o0 + dst_item * (size_t)g.B * (size_t)g.height * (size_t)g.width;
  if (o0 < d1 && d0 < o1) return fail(c, GR_EINVAL, "gr_warp_raster: out overlaps data");
  a.data = g.data; a.out = g.out;
  a.B = g.B; a.H = g.H; a.W = g.W;
  a.src_dtype = g.src_dtype; a.dst_dtype = g.dst_dtype; a.has_nodata = g.has_src_nodata ? 1 : 0;
  a.col_off = g.col_off; a.row_off = g.row_off; a.width = g.width; a.height = g.height;
  a.segs = (int)segs; a.strips = segs * g.height;
  for (int k = 0; k < 6; ++k) { a.t[k] = g.dst_transform6_h[k]; a.inv[k] = g.src_inverse6_h[k]; }
  a.src_nodata = g.src_nodata; a.dst_nodata = g.dst_nodata;
  hipStream_t s = (hipStream_t)g.stream;
  GR_HIP(c, hipSetDevice(c->device));
  GR_HIP(c, hipMemsetAsync(g.stats, 0, sizeof(uint64_t) * GR_WARP_STAT_WORDS, s));
  const dim3 grid((unsigned)std::min<int64_t>(a.strips, WARP_MAX_GROUPS)), block(WARP_SEG);
  unsigned long long *stats = (unsigned long long *)g.stats;
  const bool bilinear = g.resampling == GR_WARP_BILINEAR;
  if (g.same_crs) {
    if (bilinear) hipLaunchKernelGGL((k_warp_raster<false, true>), grid, block, 0, s, stats, a);
    else hipLaunchKernelGGL((k_warp_raster<false, false>), grid, block, 0, s, stats, a);
  } else {
    if (bilinear) hipLaunchKernelGGL((k_warp_raster<true, true>), grid, block, 0, s, stats, a);
    else hipLaunchKernelGGL((k_warp_raster<true, false>), grid, block, 0, s, stats, a);
  }
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

}  // extern "C"
