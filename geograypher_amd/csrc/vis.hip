// geograypher_amd/csrc/vis.hip -- pictures (gr_shade_view, gr_composite_labels; rules V1-V12 of DESIGN.md section 8s): one shaded,
// anti-aliased picture from an id plane and a depth plane of the raster path, and the reference's three-panel composite of a photo
// and a label image.  Neither call needs an uploaded mesh, scratch or a read-back: every kernel is enqueued on the descriptor's
// stream and the call returns.
//
// k_face_light, one lane per face (V3): the two-sided headlight |n.d| / |n| in float64 from float32 vertices, as a byte.
// k_shade (V4-V7): a workgroup of 256 lanes owns 16 x 16 output pixels.  It stages the (16 s + 2 r)^2 window of the depth plane in
// LDS, +inf outside the image, and every lane resolves the s^2 samples of its pixel in row-major order: the id from global memory,
// the colour and the light of the face by a gather, the eight neighbours at distance r from LDS in a fixed order.  float32 + - x /
// and comparisons only, every operation rounded on its own (the library is built without contraction, the division is correctly
// rounded), so numpy float32 gives every bit.
// k_composite (V8-V12): a workgroup owns up to 1024 pixels of one row.  A uint8 photo and a uint8 label strip come in through LDS
// by 16-byte words with a bytewise head and tail (a row of 3 w bytes starts at any alignment), the three output strips leave the
// same way; float64 inputs are read directly.  Per pixel float64, every operation rounded on its own, in the reference's order;
// byte / 255 comes from a table of 256 quotients a workgroup divides once.
#include <cmath>

#include "geom_dev.hpp"
#include "gr_internal.hpp"

namespace {
using namespace grimpl;

constexpr int SHADE_TILE = 16;                 // output pixels a side of a workgroup's tile
constexpr int SHADE_MAX_S = 4, SHADE_MAX_R = 16, SHADE_MAX_SIDE = 32768;
constexpr int COMP_SEG = 1024;                 // pixels of a row a workgroup composes
constexpr int COMP_STRIP = 3 * COMP_SEG + 16;  // bytes of an LDS strip: three bytes a pixel and the strip's offset in its 16-byte word
constexpr int COMP_MAX_TABLE = 1 << 24;

struct ShadeArgs {
  const int32_t *ids;      // [H s][W s]
  const float *depth;      // [H s][W s]
  const uint8_t *rgb;      // [F][3]
  const uint8_t *light;    // [F]
  uint8_t *out;            // [H][W][3]
  int64_t F;
  int32_t W, H, s, r, win, pitch;   // win = 16 s + 2 r samples a side of the window; pitch: its odd row length in LDS
  float k, bg[3];
};

struct CompositeArgs {
  const uint8_t *photo;    // [h][w][3] uint8 or float64
  const uint8_t *label;    // [h][w] or [h][w][3], uint8 or float64
  const double *table;     // [N][3]
  uint8_t *out;            // [h][3 w][3]
  int32_t w, h, N, segs;
  bool photo_u8, label_u8, label_rgb, discrete, grey;
  double shift, scale, w_label, w_photo;
};

// V3.  A face that names a vertex outside [0, V) or has no area takes shade 1.
__global__ __launch_bounds__(256) void k_face_light(const float *__restrict__ verts, const int32_t *__restrict__ faces, int64_t V, int64_t F,
                                                    double dx, double dy, double dz, double ambient, uint8_t *__restrict__ light) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  int64_t v0, v1, v2;
  double shade = 1.0;
  if (load_face(faces, f, V, v0, v1, v2)) {
    const double ax = verts[v0 * 3], ay = verts[v0 * 3 + 1], az = verts[v0 * 3 + 2];
    const double e1x = (double)verts[v1 * 3] - ax, e1y = (double)verts[v1 * 3 + 1] - ay, e1z = (double)verts[v1 * 3 + 2] - az;
    const double e2x = (double)verts[v2 * 3] - ax, e2y = (double)verts[v2 * 3 + 1] - ay, e2z = (double)verts[v2 * 3 + 2] - az;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    if (len != 0.0) shade = fabs((nx * dx + ny * dy) + nz * dz) / len;
  }
  const double v = floor((ambient + (1.0 - ambient) * shade) * 255.0 + 0.5);
  light[f] = v >= 255.0 ? 255 : (v >= 0.0 ? (uint8_t)v : 0);   // (a NaN, from vertices that are not finite: 0)
}

// V4-V7.  Dynamic LDS: win rows of `pitch` floats.
__global__ __launch_bounds__(256) void k_shade(ShadeArgs a) {
  extern __shared__ float s_z[];
  const int tid = (int)threadIdx.x, tx = tid & (SHADE_TILE - 1), ty = tid >> 4;
  const int64_t Ws = (int64_t)a.W * a.s, Hs = (int64_t)a.H * a.s;
  const int64_t wx0 = (int64_t)blockIdx.x * SHADE_TILE * a.s - a.r, wy0 = (int64_t)blockIdx.y * SHADE_TILE * a.s - a.r;
  for (int i = tid; i < a.win * a.win; i += 256) {
    const int wy = i / a.win, wx = i - wy * a.win;
    const int64_t gx = wx0 + wx, gy = wy0 + wy;
    s_z[wy * a.pitch + wx] = (gx >= 0 && gx < Ws && gy >= 0 && gy < Hs) ? a.depth[gy * Ws + gx] : INFINITY;   // V5: outside counts as +inf
  }
  __syncthreads();
  const int64_t ox = (int64_t)blockIdx.x * SHADE_TILE + tx, oy = (int64_t)blockIdx.y * SHADE_TILE + ty;
  if (ox >= a.W || oy >= a.H) return;
  float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;
  for (int sy = 0; sy < a.s; ++sy)
    for (int sx = 0; sx < a.s; ++sx) {
      const int32_t id = a.ids[(oy * a.s + sy) * Ws + (ox * a.s + sx)];
      float c0 = a.bg[0], c1 = a.bg[1], c2 = a.bg[2];
      if (id >= 0 && id < a.F) {   // V4: every other id is background
        float occl = 1.0f;
        if (a.k != 0.0f) {         // V5, V6
          const int at = (ty * a.s + sy + a.r) * a.pitch + (tx * a.s + sx + a.r), up = a.r * a.pitch;
          const float z = s_z[at];
          const int off[8] = {-up - a.r, -up, -up + a.r, -a.r, a.r, up - a.r, up, up + a.r};
          float sum = 0.0f;
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const float t = (z - s_z[at + off[q]]) / z;
            sum = sum + (t > 0.0f ? t : 0.0f);
          }
          occl = 1.0f / (1.0f + a.k * sum);
        }
        const float light = (float)a.light[id] / 255.0f;
        c0 = ((float)a.rgb[(int64_t)id * 3] * light) * occl;
        c1 = ((float)a.rgb[(int64_t)id * 3 + 1] * light) * occl;
        c2 = ((float)a.rgb[(int64_t)id * 3 + 2] * light) * occl;
      }
      acc0 = acc0 + c0; acc1 = acc1 + c1; acc2 = acc2 + c2;
    }
  const float n = (float)(a.s * a.s), acc[3] = {acc0, acc1, acc2};
  uint8_t *o = a.out + (oy * a.W + ox) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {   // V7
    const float v = floorf(acc[ch] / n + 0.5f);
    o[ch] = v >= 255.0f ? 255 : (v >= 0.0f ? (uint8_t)v : 0);
  }
}

// A strip of n bytes at g <-> LDS: byte i of the strip is lds[(g & 15) + i], so that the 16-byte words of the two agree.  The words
// that lie wholly inside the strip move as uint4, what is left in front and behind (at most 15 bytes each) bytewise: nothing
// outside [g, g + n) is read or written.
template <bool IN> __device__ __forceinline__ void comp_strip(uint8_t *g, int n, uint8_t *lds, int tid) {
  const int a = (int)((uintptr_t)g & 15), end = a + n;
  uint8_t *g0 = g - a;   // (an address, never dereferenced below g)
  const int first = min((a + 15) & ~15, end), last = max(end & ~15, first);
  for (int i = (first >> 4) + tid; i < (last >> 4); i += 256) {
    if (IN) ((uint4 *)lds)[i] = ((const uint4 *)g0)[i];
    else ((uint4 *)g0)[i] = ((const uint4 *)lds)[i];
  }
  if (tid < 16) {
    const int h = a + tid, t = last + tid;
    if (h < first) { if (IN) lds[h] = g0[h]; else g0[h] = lds[h]; }
    if (t < end) { if (IN) lds[t] = g0[t]; else g0[t] = lds[t]; }
  }
}

// V12: (v x 255) truncated to a byte as the reference's host does it: through int32, the low byte; 0 where v x 255 is no int32.
__device__ __forceinline__ uint8_t comp_byte(double v) {
  const double x = v * 255.0;
  if (!(x > -2147483649.0 && x < 2147483648.0)) return 0;
  return (uint8_t)(int32_t)x;
}

// V10: a float64 value through the colour table, as a matplotlib colormap of N rows takes it.
__device__ __forceinline__ void comp_float_colour(const CompositeArgs &a, double x, double &r, double &g, double &b) {
  double t = x * (double)a.N;
  if (t == (double)a.N) t = (double)(a.N - 1);
  r = g = b = 0.0;
  if (t != t) return;   // "bad": black
  const int idx = t < 0.0 ? 0 : (t >= (double)a.N ? a.N - 1 : (int)t);
  r = a.table[idx * 3]; g = a.table[idx * 3 + 1]; b = a.table[idx * 3 + 2];
}

__global__ __launch_bounds__(256) void k_composite(CompositeArgs a) {
  __shared__ __align__(16) uint8_t s_out[3][COMP_STRIP];
  __shared__ __align__(16) uint8_t s_photo[COMP_STRIP];
  __shared__ __align__(16) uint8_t s_label[COMP_STRIP];
  __shared__ double s_u8[256];
  const int tid = (int)threadIdx.x;
  const int64_t row = blockIdx.x / (unsigned)a.segs;
  const int seg0 = (int)(blockIdx.x % (unsigned)a.segs) * COMP_SEG, n = min(COMP_SEG, a.w - seg0);
  const int64_t p0 = row * a.w + seg0;   // the first pixel of the strip
  const int lch = a.label_rgb ? 3 : 1;
  s_u8[tid] = (double)tid / 255.0;
  int pa = 0, la = 0;
  if (a.photo_u8) {
    uint8_t *g = const_cast<uint8_t *>(a.photo) + p0 * 3;
    pa = (int)((uintptr_t)g & 15);
    comp_strip<true>(g, 3 * n, s_photo, tid);
  }
  if (a.label_u8) {
    uint8_t *g = const_cast<uint8_t *>(a.label) + p0 * lch;
    la = (int)((uintptr_t)g & 15);
    comp_strip<true>(g, lch * n, s_label, tid);
  }
  uint8_t *panel[3];
  int oa[3];
  for (int p = 0; p < 3; ++p) {
    panel[p] = a.out + (row * 9 + p * 3) * a.w + 3 * seg0;
    oa[p] = (int)((uintptr_t)panel[p] & 15);
  }
  __syncthreads();
  const double *photo64 = (const double *)a.photo, *label64 = (const double *)a.label;
  for (int k = tid; k < n; k += 256) {
    double c[3], l[3];
    for (int ch = 0; ch < 3; ++ch) c[ch] = a.photo_u8 ? s_u8[s_photo[pa + 3 * k + ch]] : photo64[(p0 + k) * 3 + ch];
    if (a.label_rgb) {   // V9: colours as they are, a byte divided by 255
      for (int ch = 0; ch < 3; ++ch) l[ch] = a.label_u8 ? s_u8[s_label[la + 3 * k + ch]] : label64[(p0 + k) * 3 + ch];
    } else if (a.label_u8 && a.discrete) {   // V10: the class indexes the table, clipped to its last row
      const int v = s_label[la + k], idx = min(v, a.N - 1);
      for (int ch = 0; ch < 3; ++ch) l[ch] = v == 0 ? 0.0 : a.table[idx * 3 + ch];
    } else {
      double x = a.label_u8 ? s_u8[s_label[la + k]] : label64[p0 + k];
      const bool null = x == 0.0 || !isfinite(x);   // V11: taken before the shift
      if (!a.discrete) x = (x - a.shift) / a.scale;
      comp_float_colour(a, x, l[0], l[1], l[2]);
      if (null) l[0] = l[1] = l[2] = 0.0;
    }
    const double grey = ((c[0] + c[1]) + c[2]) / 3.0;
    for (int ch = 0; ch < 3; ++ch) {
      const double base = a.grey ? grey : c[ch];
      s_out[0][oa[0] + 3 * k + ch] = comp_byte(l[ch]);
      s_out[1][oa[1] + 3 * k + ch] = comp_byte(c[ch]);
      s_out[2][oa[2] + 3 * k + ch] = comp_byte(a.w_photo * base + a.w_label * l[ch]);
    }
  }
  __syncthreads();
  for (int p = 0; p < 3; ++p) comp_strip<false>(panel[p], 3 * n, s_out[p], tid);
}

}  // namespace

extern "C" {

int gr_shade_view(gr_ctx *c, const gr_shade_args *args_h) {
  if (!c) return GR_EINVAL;
  if (!args_h) return fail(c, GR_EINVAL, "gr_shade_view: null descriptor");
  const gr_shade_args g = *args_h;   // read once, here: the caller may reuse the descriptor when the call returns
  const bool picture = g.width != 0 || g.height != 0, lights = g.verts || g.faces;
  if (!picture && !lights) return fail(c, GR_EINVAL, "gr_shade_view: neither a picture (width, height) nor face lights (verts, faces) asked for");
  if (g.F < 0 || g.F > 0x7FFFFFFFll - 1 || g.V < 0 || g.V > 0x7FFFFFFFll - 1)
    return fail(c, GR_EINVAL, "gr_shade_view: bad shape V=%lld F=%lld (both below 2^31 - 1)", (long long)g.V, (long long)g.F);
  if (lights) {
    if (g.F > 0 && (!g.faces || !g.face_light || (g.V > 0 && !g.verts))) return fail(c, GR_EINVAL, "gr_shade_view: null arrays (verts, faces, face_light)");
    if (!(std::isfinite(g.dir_x) && std::isfinite(g.dir_y) && std::isfinite(g.dir_z)) || !(g.ambient >= 0.0 && g.ambient <= 1.0))
      return fail(c, GR_EINVAL, "gr_shade_view: view direction (%g, %g, %g) not finite or ambient=%g outside [0, 1]", g.dir_x, g.dir_y, g.dir_z, g.ambient);
  }
  if (picture) {
    if (g.width < 1 || g.height < 1 || g.width > SHADE_MAX_SIDE || g.height > SHADE_MAX_SIDE)
      return fail(c, GR_EINVAL, "gr_shade_view: bad picture %d x %d (1 to %d a side)", g.width, g.height, SHADE_MAX_SIDE);
    if (g.supersample < 1 || g.supersample > SHADE_MAX_S || g.radius < 1 || g.radius > SHADE_MAX_R)
      return fail(c, GR_EINVAL, "gr_shade_view: supersample=%d outside [1, %d] or radius=%d outside [1, %d]", g.supersample, SHADE_MAX_S, g.radius,
                  SHADE_MAX_R);
    if (!(g.strength >= 0.0f) || !std::isfinite(g.strength)) return fail(c, GR_EINVAL, "gr_shade_view: strength=%g is not a finite number >= 0", (double)g.strength);
    if ((g.bg_r | g.bg_g | g.bg_b) < 0 || g.bg_r > 255 || g.bg_g > 255 || g.bg_b > 255)
      return fail(c, GR_EINVAL, "gr_shade_view: background (%d, %d, %d) outside [0, 255]", g.bg_r, g.bg_g, g.bg_b);
    if (!g.ids || !g.depth || !g.out || (g.F > 0 && (!g.face_rgb || !g.face_light))) return fail(c, GR_EINVAL, "gr_shade_view: null arrays");
  }
  hipStream_t s = (hipStream_t)g.stream;
  GR_HIP(c, hipSetDevice(c->device));
  if (lights && g.F > 0) {
    hipLaunchKernelGGL(k_face_light, dim3((unsigned)ceil_div(g.F, (int64_t)256)), dim3(256), 0, s, g.verts, g.faces, g.V, g.F, g.dir_x, g.dir_y,
                       g.dir_z, g.ambient, g.face_light);
    GR_HIP(c, hipGetLastError());
  }
  if (picture) {
    ShadeArgs a;
    a.ids = g.ids; a.depth = g.depth; a.rgb = g.face_rgb; a.light = g.face_light; a.out = g.out; a.F = g.F;
    a.W = g.width; a.H = g.height; a.s = g.supersample; a.r = g.radius;
    a.win = SHADE_TILE * a.s + 2 * a.r;
    a.pitch = a.win | 1;
    a.k = g.strength;
    a.bg[0] = (float)g.bg_r; a.bg[1] = (float)g.bg_g; a.bg[2] = (float)g.bg_b;
    const dim3 grid((unsigned)ceil_div(a.W, SHADE_TILE), (unsigned)ceil_div(a.H, SHADE_TILE));
    hipLaunchKernelGGL(k_shade, grid, dim3(256), sizeof(float) * (size_t)a.pitch * a.win, s, a);
    GR_HIP(c, hipGetLastError());
  }
  return GR_OK;
}

int gr_composite_labels(gr_ctx *c, const gr_composite_args *args_h) {
  if (!c) return GR_EINVAL;
  if (!args_h) return fail(c, GR_EINVAL, "gr_composite_labels: null descriptor");
  const gr_composite_args g = *args_h;
  if (g.width < 1 || g.height < 1) return fail(c, GR_EINVAL, "gr_composite_labels: bad image %d x %d", g.width, g.height);
  const int64_t segs = ceil_div((int64_t)g.width, (int64_t)COMP_SEG);
  if (segs * g.height > 0x7FFFFFFFll) return fail(c, GR_EINVAL, "gr_composite_labels: image %d x %d is too large", g.width, g.height);
  const bool photo_u8 = g.photo_dtype == GR_DTYPE_U8, label_u8 = g.label_dtype == GR_DTYPE_U8;
  if ((!photo_u8 && g.photo_dtype != GR_DTYPE_F64) || (!label_u8 && g.label_dtype != GR_DTYPE_F64))
    return fail(c, GR_EINVAL, "gr_composite_labels: photo_dtype=%d, label_dtype=%d: each GR_DTYPE_U8 or GR_DTYPE_F64", g.photo_dtype, g.label_dtype);
  if (g.label_channels != 1 && g.label_channels != 3) return fail(c, GR_EINVAL, "gr_composite_labels: label_channels=%d, neither 1 nor 3", g.label_channels);
  if (g.label_channels == 3 && label_u8 && g.discrete)
    return fail(c, GR_EINVAL, "gr_composite_labels: a uint8 colour label with discrete classes is not supported");
  if (g.label_channels == 1 && (g.table_rows < 1 || g.table_rows > COMP_MAX_TABLE || !g.table))
    return fail(c, GR_EINVAL, "gr_composite_labels: a colour table of %d rows (1 to %d) at %p", g.table_rows, COMP_MAX_TABLE, (const void *)g.table);
  if (!g.photo || !g.label || !g.out) return fail(c, GR_EINVAL, "gr_composite_labels: null arrays");
  if ((!photo_u8 && (uintptr_t)g.photo % 8) || (!label_u8 && (uintptr_t)g.label % 8) || (uintptr_t)g.table % 8)
    return fail(c, GR_EINVAL, "gr_composite_labels: a float64 array is not 8-byte aligned");
  GR_HIP(c, hipSetDevice(c->device));
  CompositeArgs a;
  a.photo = (const uint8_t *)g.photo; a.label = (const uint8_t *)g.label; a.table = g.table; a.out = g.out;
  a.w = g.width; a.h = g.height; a.N = g.table_rows; a.segs = (int32_t)segs;
  a.photo_u8 = photo_u8; a.label_u8 = label_u8; a.label_rgb = g.label_channels == 3; a.discrete = g.discrete != 0; a.grey = g.grey_overlay != 0;
  a.shift = g.shift; a.scale = g.scale; a.w_label = g.weight; a.w_photo = 1.0 - g.weight;
  hipLaunchKernelGGL(k_composite, dim3((unsigned)(segs * g.height)), dim3(256), 0, (hipStream_t)g.stream, a);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

}  // extern "C"
