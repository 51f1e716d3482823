// geograypher_amd/csrc/nadir.hip -- the top-down raster of a mesh (gr_nadir_raster, rules N1-N9 of DESIGN.md section 8r): per cell
// of a window of a georeferenced grid the face whose surface is highest at the cell's centre, and that height.  Needs no uploaded
// mesh; its scratch is the context's stage arena.
//
// Two walks over the same (face, cell) pairs and a finish.  Walk 0 takes, per cell, the 64-bit maximum of the order-preserving key
// of the height (atomicMax; the keys live in z_out, which is 8 bytes a cell); walk 1 takes the minimum of the face index among
// the pairs whose key equals the cell's maximum (atomicMin into face_out, which starts at 2^31 - 1).  An integer maximum and an
// integer minimum do not depend on the order of arrival (N6).  k_nadir_finish decodes the keys in place, writes -1 and NaN where
// no face came, and counts the covered cells.
//
// A walk is two kernels (N8).  k_nadir_faces, one lane per face: N3, the face's box of centre indices cut to the window, and --
// where the box holds at most small_cells centres, which is nearly every face of a survey mesh -- the cells themselves, in that
// lane.  In walk 0 the other faces go to a list (a ballot and one atomic per wave) with their item counts; the host reads the
// list's length and the item total back, scans the counts, and k_nadir_items gives every item of at most 64 columns x item_rows
// rows to a wave, one column per lane: item -> face by binary search in the scanned counts.  No lane loops over more than
// max(small_cells, item_rows) cells.
//
// Membership (N4) is Z3 (edge_crossing_strict of geom_dev.hpp) on the triangle as a ring of three vertices: the sign of an exact
// determinant, in int64 where the face spans fewer than 2^26 units on both axes (every product below 2^52) and through the
// 128-bit orient otherwise; both are exact, so the planes do not depend on small_cells, item_rows or the path.  The height (N5)
// is float64, every operation rounded on its own (the library is built without contraction), the division correctly rounded.
#include "cub_steps.hpp"
#include "geom_dev.hpp"
#include "gr_internal.hpp"

namespace {
using namespace grimpl;

typedef unsigned long long u64;

constexpr int NADIR_SMALL_DEFAULT = 256, NADIR_SMALL_MAX = 65536;     // the defaults: the best pair of the sweep in DESIGN.md 8r
constexpr int NADIR_ITEM_ROWS_DEFAULT = 16, NADIR_ITEM_ROWS_MAX = 1024;
constexpr int NADIR_ITEM_COLS = 64;                // one column per lane
constexpr int64_t NADIR_NARROW_SPAN = 1ll << 26;   // below it on both axes the determinants fit int64 (and double: N5)
constexpr int32_t NADIR_NO_FACE = 0x7FFFFFFF;      // face_out between the walks: above every face index
constexpr u64 NADIR_NAN_BITS = 0x7FF8000000000000ull;
constexpr unsigned NADIR_MAX_ITEM_GROUPS = 65536;  // workgroups of k_nadir_items; further items by stride

struct NadirArgs {
  const int64_t *vq;      // [V][2]
  const double *z;        // [V]
  const int32_t *faces;   // [F][3]
  int64_t V, F;
  int32_t col_off, row_off, width, height, small_cells, item_rows;
  u64 *keys;              // [height][width]: z_out between the walks
  int32_t *face_out;      // [height][width]
  u64 *stats;             // [GR_NADIR_STAT_WORDS]
  u64 *n_big;             // [1] faces on the list
  int32_t *big_face;      // [F] the list
  int64_t *big_cnt;       // [F + 1] items of every listed face
  const int64_t *big_off; // [n_big + 1] their exclusive sum
};

// A face that takes part: corners in the caller's order, the box of centre indices cut to the window (c0 <= c1, r0 <= r1).
struct Tri {
  int64_t ax, ay, bx, by, cx, cy;
  double za, zb, zc;
  int32_t c0, c1, r0, r1;
  bool narrow;
};

enum { NADIR_TAKES = 0, NADIR_BAD_INDEX, NADIR_NONFINITE, NADIR_ZERO_AREA, NADIR_EMPTY_BOX };

// N3 and the clipped box of face f < F.  Only NADIR_TAKES fills the whole of `t`.
__device__ __forceinline__ int nadir_classify(const NadirArgs &a, int64_t f, Tri &t) {
  int64_t v0, v1, v2;
  if (!load_face(a.faces, f, a.V, v0, v1, v2)) return NADIR_BAD_INDEX;
  t.za = a.z[v0]; t.zb = a.z[v1]; t.zc = a.z[v2];
  if (!(isfinite(t.za) && isfinite(t.zb) && isfinite(t.zc))) return NADIR_NONFINITE;
  t.ax = a.vq[v0 * 2]; t.ay = a.vq[v0 * 2 + 1];
  t.bx = a.vq[v1 * 2]; t.by = a.vq[v1 * 2 + 1];
  t.cx = a.vq[v2 * 2]; t.cy = a.vq[v2 * 2 + 1];
  if (orient(t.ax, t.ay, t.bx, t.by, t.cx, t.cy) == 0) return NADIR_ZERO_AREA;
  const int64_t x0 = min(t.ax, min(t.bx, t.cx)), x1 = max(t.ax, max(t.bx, t.cx));
  const int64_t y0 = min(t.ay, min(t.by, t.cy)), y1 = max(t.ay, max(t.by, t.cy));
  t.narrow = x1 - x0 < NADIR_NARROW_SPAN && y1 - y0 < NADIR_NARROW_SPAN;
  // the centres 65536 k + 32768 inside [x0, x1]: k from ceil((x0 - 32768) / 65536) to floor((x1 - 32768) / 65536); |k| < 2^24
  const int64_t c0 = max((x0 + 32767) >> 16, (int64_t)a.col_off), c1 = min((x1 - 32768) >> 16, (int64_t)a.col_off + a.width - 1);
  const int64_t r0 = max((y0 + 32767) >> 16, (int64_t)a.row_off), r1 = min((y1 - 32768) >> 16, (int64_t)a.row_off + a.height - 1);
  if (c0 > c1 || r0 > r1) return NADIR_EMPTY_BOX;
  t.c0 = (int32_t)c0; t.c1 = (int32_t)c1; t.r0 = (int32_t)r0; t.r1 = (int32_t)r1;
  return NADIR_TAKES;
}

// N4: Z3 over the face's three edges.  NARROW: every difference is below 2^26, the determinants fit int64.
template <bool NARROW> __device__ __forceinline__ bool nadir_inside(const Tri &t, int64_t px, int64_t py) {
  int parity = 0;
  edge_crossing_strict<NARROW>(t.ax, t.ay, t.bx, t.by, px, py, parity);
  edge_crossing_strict<NARROW>(t.bx, t.by, t.cx, t.cy, px, py, parity);
  edge_crossing_strict<NARROW>(t.cx, t.cy, t.ax, t.ay, px, py, parity);
  return parity != 0;
}

// N5 and N6: the key of the face's height at the centre, 0 where the pair is skipped (no finite height has key 0).
__device__ __forceinline__ u64 nadir_key(const Tri &t, int64_t px, int64_t py) {
  const double ex1 = (double)(t.bx - t.ax), ey1 = (double)(t.by - t.ay), ex2 = (double)(t.cx - t.ax), ey2 = (double)(t.cy - t.ay);
  const double dx = (double)(px - t.ax), dy = (double)(py - t.ay);
  const double D = ex1 * ey2 - ey1 * ex2, Nb = dx * ey2 - dy * ex2, Nc = ex1 * dy - ey1 * dx;
  if (D == 0.0) return 0;
  const double z = (t.za + (t.zb - t.za) * (Nb / D)) + (t.zc - t.za) * (Nc / D);
  if (!isfinite(z)) return 0;
  const u64 u = (u64)__double_as_longlong(z);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// One (face, cell) pair of walk WALK: membership, the key, the atomic.  Counts in walk 0 only.
template <int WALK, bool NARROW>
__device__ __forceinline__ void nadir_visit(const NadirArgs &a, const Tri &t, int32_t f, int32_t col, int32_t row, u64 &n_in,
                                            u64 &n_skip) {
  const int64_t px = 65536ll * col + 32768, py = 65536ll * row + 32768;   // Z2
  if (!nadir_inside<NARROW>(t, px, py)) return;
  const u64 key = nadir_key(t, px, py);
  if (WALK == 0) { ++n_in; if (!key) ++n_skip; }
  if (!key) return;
  const int64_t at = (int64_t)(row - a.row_off) * a.width + (col - a.col_off);   // inside the window: the box is cut to it
  if (WALK == 0) atomicMax(&a.keys[at], key);
  else if (a.keys[at] == key) atomicMin(&a.face_out[at], f);
}

// One lane per face: N3, the clipped box, the small faces' cells; walk 0 also counts and lists the larger faces.
template <int WALK> __global__ __launch_bounds__(256) void k_nadir_faces(NadirArgs a) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  Tri t;
  const int what = f < a.F ? nadir_classify(a, f, t) : -1;
  int64_t cells = 0, items = 0;
  if (what == NADIR_TAKES) {
    const int64_t w = (int64_t)t.c1 - t.c0 + 1, h = (int64_t)t.r1 - t.r0 + 1;
    cells = w * h;
    if (cells > a.small_cells) items = ceil_div(w, NADIR_ITEM_COLS) * ceil_div(h, a.item_rows);
  }
  u64 n_in = 0, n_skip = 0;
  if (what == NADIR_TAKES && items == 0) {   // at most small_cells cells
    for (int32_t row = t.r0; row <= t.r1; ++row)
      for (int32_t col = t.c0; col <= t.c1; ++col) {
        if (t.narrow) nadir_visit<WALK, true>(a, t, (int32_t)f, col, row, n_in, n_skip);
        else nadir_visit<WALK, false>(a, t, (int32_t)f, col, row, n_in, n_skip);
      }
  }
  if (WALK != 0) return;
  // the list of the larger faces: one atomic per wave that has any
  const u64 big = __ballot(items > 0);
  if (big) {
    const int leader = __ffsll((long long)big) - 1;
    long long base = 0;
    if (lane == leader) base = (long long)atomicAdd(a.n_big, (u64)__popcll(big));
    base = __shfl(base, leader);
    if (items > 0) {
      const int64_t at = base + __popcll(big & ((1ull << lane) - 1ull));   // below F: a face is listed once
      a.big_face[at] = (int32_t)f;
      a.big_cnt[at] = items;
    }
  }
  stat_count(a.stats, GR_NADIR_STAT_FACES, what == NADIR_TAKES || what == NADIR_EMPTY_BOX, lane);
  stat_count(a.stats, GR_NADIR_STAT_BAD_INDEX, what == NADIR_BAD_INDEX, lane);
  stat_count(a.stats, GR_NADIR_STAT_ZERO_AREA, what == NADIR_ZERO_AREA, lane);
  stat_count(a.stats, GR_NADIR_STAT_NONFINITE_Z, what == NADIR_NONFINITE, lane);
  stat_count(a.stats, GR_NADIR_STAT_EMPTY_BOX, what == NADIR_EMPTY_BOX, lane);
  stat_add(a.stats, GR_NADIR_STAT_ITEMS, (u64)items, lane);
  stat_add(a.stats, GR_NADIR_STAT_TESTS, (u64)cells, lane);
  stat_add(a.stats, GR_NADIR_STAT_INSIDE, n_in, lane);
  stat_add(a.stats, GR_NADIR_STAT_SKIPPED, n_skip, lane);
}

// One wave per item of a listed face: 64 columns x item_rows rows of its clipped box, one column per lane.
template <int WALK> __global__ __launch_bounds__(256) void k_nadir_items(NadirArgs a, int64_t n_big, int64_t n_items) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t n_waves = (int64_t)gridDim.x * 4;
  u64 n_in = 0, n_skip = 0;
  for (int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < n_items; item += n_waves) {   // wave-uniform
    // the last listed face k with big_off[k] <= item (every listed face has an item, so the offsets rise strictly)
    int64_t lo = 0, hi = n_big - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (a.big_off[mid] <= item) lo = mid; else hi = mid - 1;
    }
    const int64_t f = a.big_face[lo];
    Tri t;
    if (f < 0 || f >= a.F || nadir_classify(a, f, t) != NADIR_TAKES) continue;   // (never: the list holds faces that take part)
    const int64_t items_x = ceil_div((int64_t)t.c1 - t.c0 + 1, NADIR_ITEM_COLS), local = item - a.big_off[lo];
    const int64_t col = (int64_t)t.c0 + (local % items_x) * NADIR_ITEM_COLS + lane;
    const int64_t row0 = (int64_t)t.r0 + (local / items_x) * a.item_rows;
    if (col > t.c1) continue;
    const int64_t row1 = min(row0 + a.item_rows - 1, (int64_t)t.r1);   // row0 > r1 (a count that does not fit the box): no row
    for (int64_t row = row0; row <= row1; ++row) {
      if (t.narrow) nadir_visit<WALK, true>(a, t, (int32_t)f, (int32_t)col, (int32_t)row, n_in, n_skip);
      else nadir_visit<WALK, false>(a, t, (int32_t)f, (int32_t)col, (int32_t)row, n_in, n_skip);
    }
  }
  if (WALK != 0) return;
  stat_add(a.stats, GR_NADIR_STAT_INSIDE, n_in, lane);
  stat_add(a.stats, GR_NADIR_STAT_SKIPPED, n_skip, lane);
}

// N7: keys -> heights in place, -1 and NaN where no face came; one lane per cell, the grid capped.  Counts the covered cells.
__global__ __launch_bounds__(256) void k_nadir_finish(u64 *__restrict__ keys, int32_t *__restrict__ face_out, int64_t n_cells,
                                                      u64 *__restrict__ stats) {
  const int lane = (int)(threadIdx.x & 63);
  u64 covered = 0;   // wave-uniform
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n_cells; base += (int64_t)gridDim.x * 256) {   // workgroup-uniform
    const int64_t i = base + threadIdx.x;
    bool hit = false;
    if (i < n_cells) {
      const u64 key = keys[i];
      hit = key != 0;
      keys[i] = !hit ? NADIR_NAN_BITS : ((key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key);
      if (!hit) face_out[i] = -1;
    }
    covered += (u64)__popcll(__ballot(hit));
  }
  if (lane == 0 && covered) atomicAdd(&stats[GR_NADIR_STAT_COVERED], covered);
}

}  // namespace

extern "C" {

int gr_nadir_raster(gr_ctx *c, const int64_t *verts_q, const double *z, int64_t V, const int32_t *faces, int64_t F, int32_t col_off,
                    int32_t row_off, int32_t width, int32_t height, int32_t small_cells, int32_t item_rows, int32_t *face_out,
                    double *z_out, uint64_t *stats, void *stream) {
  if (!c) return GR_EINVAL;
  GR_TRY(check_window(c, "gr_nadir_raster", col_off, row_off, width, height));
  if (V < 0 || F < 0 || V > 0x7FFFFFFFll - 1 || F > 0x7FFFFFFFll - 1)
    return fail(c, GR_EINVAL, "gr_nadir_raster: bad shape V=%lld F=%lld (both below 2^31 - 1)", (long long)V, (long long)F);
  if (small_cells < 0 || small_cells > NADIR_SMALL_MAX || item_rows < 0 || item_rows > NADIR_ITEM_ROWS_MAX)
    return fail(c, GR_EINVAL, "gr_nadir_raster: small_cells=%d outside [0, %d] or item_rows=%d outside [0, %d]", small_cells,
                NADIR_SMALL_MAX, item_rows, NADIR_ITEM_ROWS_MAX);
  if (!face_out || !z_out || !stats || (V > 0 && (!verts_q || !z)) || (F > 0 && !faces))
    return fail(c, GR_EINVAL, "gr_nadir_raster: null arrays");
  if ((uintptr_t)z_out % 8) return fail(c, GR_EINVAL, "gr_nadir_raster: z_out is not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  const int64_t n_cells = (int64_t)width * height;
  u64 *st = (u64 *)stats, *keys = (u64 *)z_out;
  GR_HIP(c, hipMemsetAsync(st, 0, sizeof(uint64_t) * GR_NADIR_STAT_WORDS, s));
  GR_HIP(c, hipMemsetAsync(keys, 0, sizeof(u64) * (size_t)n_cells, s));   // key 0: no face yet
  GR_HIP(c, hipMemsetD32Async((hipDeviceptr_t)face_out, NADIR_NO_FACE, (size_t)n_cells, s));

  if (F > 0) {
    // scratch: n_big [1] | big_face [F] | big_cnt [F + 1] | big_off [F + 1] | the scan's temporaries
    Plan p;
    const auto o_n = p.array<u64>(1);
    const auto o_face = p.array<int32_t>(F);
    const auto o_cnt = p.array<int64_t>(F + 1), o_off = p.array<int64_t>(F + 1);
    const ExclusiveSum<int64_t> scan(c, p, F + 1);
    const int rc = stage_acquire(c, c->stage, p.finish(), s, "nadir-raster");
    if (rc != GR_OK) return rc;
    p.base = c->stage.ptr;

    NadirArgs a;
    a.vq = verts_q; a.z = z; a.faces = faces; a.V = V; a.F = F;
    a.col_off = col_off; a.row_off = row_off; a.width = width; a.height = height;
    a.small_cells = small_cells ? small_cells : NADIR_SMALL_DEFAULT;
    a.item_rows = item_rows ? item_rows : NADIR_ITEM_ROWS_DEFAULT;
    a.keys = keys; a.face_out = face_out; a.stats = st;
    a.n_big = o_n(); a.big_face = o_face(); a.big_cnt = o_cnt(); a.big_off = o_off();
    GR_HIP(c, hipMemsetAsync(o_n(), 0, sizeof(u64), s));
    const dim3 grid((unsigned)ceil_div(F, 256)), block(256);
    hipLaunchKernelGGL(k_nadir_faces<0>, grid, block, 0, s, a);
    GR_HIP(c, hipGetLastError());
    // the list's length and the item total: the one read-back of the call
    u64 n_big_h = 0, n_items_h = 0;
    GR_HIP(c, hipMemcpyAsync(&n_big_h, o_n(), sizeof(u64), hipMemcpyDeviceToHost, s));
    GR_HIP(c, hipMemcpyAsync(&n_items_h, st + GR_NADIR_STAT_ITEMS, sizeof(u64), hipMemcpyDeviceToHost, s));
    GR_HIP(c, hipStreamSynchronize(s));
    const int64_t n_big = (int64_t)n_big_h, n_items = (int64_t)n_items_h;
    if (n_big < 0 || n_big > F || n_items < n_big)
      return fail(c, GR_EHIP, "gr_nadir_raster: %lld faces listed with %lld items, of %lld faces", (long long)n_big, (long long)n_items, (long long)F);
    const dim3 item_grid((unsigned)std::min(ceil_div(n_items, 4), (int64_t)NADIR_MAX_ITEM_GROUPS));
    if (n_big > 0) {
      GR_HIP(c, hipMemsetAsync(o_cnt() + n_big, 0, sizeof(int64_t), s));
      GR_TRY(scan.run(o_cnt(), o_off(), s, n_big + 1));
      hipLaunchKernelGGL(k_nadir_items<0>, item_grid, block, 0, s, a, n_big, n_items);
    }
    hipLaunchKernelGGL(k_nadir_faces<1>, grid, block, 0, s, a);
    if (n_big > 0) hipLaunchKernelGGL(k_nadir_items<1>, item_grid, block, 0, s, a, n_big, n_items);
    GR_HIP(c, hipGetLastError());
  }
  const unsigned groups = (unsigned)std::min(ceil_div(n_cells, (int64_t)256), (int64_t)16384);
  hipLaunchKernelGGL(k_nadir_finish, dim3(groups), dim3(256), 0, s, keys, face_out, n_cells, st);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

}  // extern "C"
