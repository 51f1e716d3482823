// geograypher_amd/csrc/equirect.hip -- 360-degree photos: one perspective view resampled from a device-resident equirectangular
// image, oversampling and block mean fused (DESIGN.md "Equirectangular resampling").
#include "gr_internal.hpp"

using namespace grimpl;

namespace {

#define GR_EQ_CH 4  // channels one launch keeps in registers; more channels take further launches (c0)

struct EqArgs {
  const void *src;       // [H][W][C] interleaved, in the file dtype
  const double *x, *y;   // ray coordinates of the oversampled view's columns (nx) and rows (ny), utils/image.py:195-196
  const double *bounds;  // [C][2] normalised clip range of every channel
  void *out;             // [out_h][out_w][C]: f64, or the source dtype when os == 1
  uint8_t *mask;         // [H][W + 1] or null
  double *dbg;           // [2][ny][nx] or null
  double R[9];           // row-major rotation, rays are rotated as d @ R^T
  double vmin, vrange, nfill;
  int H, W, C, c0, nc;   // this launch: channels [c0, c0 + nc)
  int out_h, out_w, os, order;
};

template <typename T> __device__ __forceinline__ double eq_trunc(double v) { return v; }
template <> __device__ __forceinline__ double eq_trunc<uint8_t>(double v) { return (double)(int)v; }  // C truncation, as numpy's astype

// K9  perspective_from_equirectangular (utils/image.py:129-267) with flexible_inputs_warp (image.py:72-126, skimage.transform.warp
//     over scipy.ndimage.map_coordinates, "grid-constant") and downscale_local_mean fused: one work item owns one OUTPUT pixel and
//     walks its os x os samples row-major; neither the oversampled image nor its coordinate map exists.  Lanes run along output
//     columns: neighbouring lanes read neighbouring texels.  f64 throughout, every operation rounded on its own
//     (-ffp-contract=off), in the order DESIGN.md lists.
template <typename T>
__global__ __launch_bounds__(256) void k_equirect_view(EqArgs a) {
  const int px = blockIdx.x * 64 + threadIdx.x, py = blockIdx.y * 4 + threadIdx.y;
  if (px >= a.out_w || py >= a.out_h) return;
  const T *__restrict__ src = (const T *)a.src;
  const int64_t nx = (int64_t)a.out_w * a.os, ny = (int64_t)a.out_h * a.os;
  const double Hd = (double)a.H, Wd = (double)a.W;
  const double PI = 3.141592653589793, TWO_PI = 6.283185307179586;
  double lo[GR_EQ_CH], hi[GR_EQ_CH], sum[GR_EQ_CH];
#pragma unroll
  for (int c = 0; c < GR_EQ_CH; ++c) {
    sum[c] = 0.0;
    lo[c] = c < a.nc ? a.bounds[2 * (a.c0 + c)] : 0.0;
    hi[c] = c < a.nc ? a.bounds[2 * (a.c0 + c) + 1] : 0.0;
  }
  // normalised tap (r, c) of the image with column W = column 0 appended; outside of it: the fill
  auto tap = [&](double r, double c, int ch) -> double {
    if (!(r >= 0.0 && r < Hd && c >= 0.0 && c <= Wd)) return a.nfill;
    const int64_t ci = c == Wd ? 0 : (int64_t)c;
    return ((double)src[((int64_t)r * a.W + ci) * a.C + a.c0 + ch] - a.vmin) / a.vrange;
  };
  for (int sa = 0; sa < a.os; ++sa) {
    const int64_t row = (int64_t)py * a.os + sa;
    const double yy = -a.y[row];
    for (int sb = 0; sb < a.os; ++sb) {
      const int64_t col = (int64_t)px * a.os + sb;
      const double xx = a.x[col];
      const double n = sqrt((xx * xx + yy * yy) + 1.0);
      const double d0 = xx / n, d1 = yy / n, d2 = 1.0 / n;
      const double e0 = (d0 * a.R[0] + d1 * a.R[1]) + d2 * a.R[2];
      const double e1 = (d0 * a.R[3] + d1 * a.R[4]) + d2 * a.R[5];
      const double e2 = (d0 * a.R[6] + d1 * a.R[7]) + d2 * a.R[8];
      const double hor = atan2(e0, e2);
      const double alt = asin(fmin(fmax(e1, -1.0), 1.0));
      double i = (0.5 - alt / PI) * Hd;
      double j = (hor / TWO_PI + 0.5) * Wd;
      i = fmin(fmax(i, 0.0), Hd - 1.0);
      j = fmin(fmax(j, 0.0), Wd);
      if (a.dbg && a.c0 == 0) {
        a.dbg[row * nx + col] = i;
        a.dbg[ny * nx + row * nx + col] = j;
      }
      if (a.mask && a.c0 == 0) {
        const double ri = rint(i), rj = rint(j);  // round half to even, as numpy.round
        if (ri >= 0.0 && ri < Hd && rj >= 0.0 && rj <= Wd) a.mask[(int64_t)ri * (a.W + 1) + (int64_t)rj] = 1;
      }
      if (a.order == 0) {
        const double r = floor(i + 0.5), c = floor(j + 0.5);
#pragma unroll
        for (int ch = 0; ch < GR_EQ_CH; ++ch)
          if (ch < a.nc) sum[ch] += eq_trunc<T>(tap(r, c, ch) * a.vrange + a.vmin);
      } else {
        const double r0 = floor(i), c0 = floor(j);
        const double tr = i - r0, tc = j - c0;
        const double wr0 = 1.0 - tr, wr1 = tr, wc0 = 1.0 - tc, wc1 = tc;
#pragma unroll
        for (int ch = 0; ch < GR_EQ_CH; ++ch) {
          if (ch >= a.nc) continue;
          double t = tap(r0, c0, ch) * wr0 * wc0;
          t += tap(r0, c0 + 1.0, ch) * wr0 * wc1;
          t += tap(r0 + 1.0, c0, ch) * wr1 * wc0;
          t += tap(r0 + 1.0, c0 + 1.0, ch) * wr1 * wc1;
          t = fmin(fmax(t, lo[ch]), hi[ch]);
          sum[ch] += eq_trunc<T>(t * a.vrange + a.vmin);
        }
      }
    }
  }
  const int64_t o = ((int64_t)py * a.out_w + px) * a.C + a.c0;
  if (a.os == 1) {  // downscale_local_mean is skipped at factor 1: the sample in the source dtype
    T *out = (T *)a.out;
#pragma unroll
    for (int ch = 0; ch < GR_EQ_CH; ++ch)
      if (ch < a.nc) out[o + ch] = (T)sum[ch];
  } else {
    double *out = (double *)a.out;
    const double inv = (double)(a.os * a.os);
#pragma unroll
    for (int ch = 0; ch < GR_EQ_CH; ++ch)
      if (ch < a.nc) out[o + ch] = sum[ch] / inv;
  }
}

}  // namespace

extern "C" {

int gr_equirect_view(gr_ctx *c, const void *src, int dtype, int h_in, int w_in, int C, const double *x, const double *y,
                     const double *rotation_h, int out_h, int out_w, int oversample, int order, double value_min,
                     double value_range, const double *channel_bounds, void *out, uint8_t *mask, double *debug_ij,
                     void *stream) {
  if (!c) return GR_EINVAL;
  if (!src || !x || !y || !rotation_h || !channel_bounds || !out || h_in <= 0 || w_in <= 0 || C <= 0 || out_h <= 0 || out_w <= 0)
    return fail(c, GR_EINVAL, "bad equirectangular view args");
  if (h_in > (1 << 20) || w_in > (1 << 20) || oversample < 1 || oversample > 64 || (int64_t)out_h * oversample > (1 << 24) ||
      (int64_t)out_w * oversample > (1 << 24))
    return fail(c, GR_EINVAL, "equirectangular view: source %d x %d, view %d x %d at oversampling %d out of range", h_in, w_in,
                out_h, out_w, oversample);
  if (order != 0 && order != 1) return fail(c, GR_EINVAL, "interpolation order %d not supported (0 or 1)", order);
  if (dtype != GR_DTYPE_U8 && dtype != GR_DTYPE_F64)
    return fail(c, GR_EINVAL, "equirectangular source dtype %d not supported (GR_DTYPE_U8 or GR_DTYPE_F64)", dtype);
  if (!(value_range > 0.0) || !std::isfinite(value_range) || !std::isfinite(value_min))
    return fail(c, GR_EINVAL, "value_range must be positive and finite");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  EqArgs a;
  a.src = src; a.x = x; a.y = y; a.bounds = channel_bounds; a.out = out; a.mask = mask; a.dbg = debug_ij;
  for (int k = 0; k < 9; ++k) a.R[k] = rotation_h[k];
  a.vmin = value_min; a.vrange = value_range; a.nfill = (0.0 - value_min) / value_range;  // image.py:104 with fill 0
  a.H = h_in; a.W = w_in; a.C = C; a.out_h = out_h; a.out_w = out_w; a.os = oversample; a.order = order;
  const dim3 grid((unsigned)ceil_div(out_w, 64), (unsigned)ceil_div(out_h, 4)), block(64, 4);
  for (int c0 = 0; c0 < C; c0 += GR_EQ_CH) {
    a.c0 = c0; a.nc = std::min(GR_EQ_CH, C - c0);
    if (dtype == GR_DTYPE_U8) hipLaunchKernelGGL(k_equirect_view<uint8_t>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_equirect_view<double>, grid, block, 0, s, a);
    GR_HIP(c, hipGetLastError());
  }
  return GR_OK;
}

}  // extern "C"
