// geograypher_amd/csrc/ortho.hip -- the orthomosaic baseline: overlapping tile predictions assembled into one class raster
// (gr_assemble_tiles, rules O1-O8), the class counts of the raster cells under every polygon row (gr_zonal_class_counts, rules
// Z1-Z7) and polygon rows burned into a label raster (gr_burn_polygons, rules B1-B7); the rule-sets are DESIGN.md section 8m.
// Needs no uploaded mesh and no context scratch.
//
// Assembly.  One lane per output pixel; a workgroup covers 64 x 4 pixels inside ONE bin of the host's bin table and stages that
// bin's tile records in LDS, ORTHO_CHUNK at a time, so a bin may list any number of tiles.  A lane keeps no per-class array (the
// unit is held to zero scratch): it walks the classes its covering tiles CARRY in ascending order.  A pass over the bin's records
// sums the weights of the pairs that carry the current class and finds the next carried class above it; classes nobody carries
// have count 0 and are stored as zeros between the carried ones.  The passes are workgroup-uniform (a lane without a further
// class idles through them), the sums are taken in the count type's own arithmetic in ascending list order -- the list is
// ascending in tile index, which fixes the float64 sums --, there is no atomic but the statistics words, and every output byte is
// stored once, by the lane that owns the pixel.
//
// Zonal counts.  A workgroup takes one work item: a polygon row and a block of at most 64 x 128 cells of its box.  Wave w owns
// the block's rows w, w + 4, ...: a row segment is one cell per lane, so every lane of a wave has the same py, the candidate test
// of the ring walk is wave-uniform and the 128-bit determinant is formed for candidate edges only (edge_crossing_strict of
// geom_dev.hpp).  The row's ring vertices are staged in LDS, ZONAL_CHUNK at a time (a ring of any length works); the parity of
// up to 32 rows per lane is kept in one word.
// Inside cells go into an LDS histogram of C words, then one 64-bit atomicAdd per class with a non-zero count: integers, so the
// order does not matter.  All integer; no floating point in that kernel.
//
// Polygon burn (gr_burn_polygons, rules B1-B7).  k_burn_rows is the zonal kernel up to the parity word -- the two share ONE ring
// walk, zonal_parity_walk --, over items in the coordinates of the parent grid restricted to a window of it.  A lane whose parity
// bit is set does one non-returning atomicMax of the row index into the window's row plane (set to -1 at the head of the call):
// the cells of an item are distinct, so nothing contends inside a workgroup, and an integer maximum does not depend on the order
// in which the rows arrive (B3: the highest row wins).  k_burn_values maps the row plane to bytes, one lane per cell.  All integer.
#include "geom_dev.hpp"
#include "gr_internal.hpp"

namespace {
using namespace grimpl;

constexpr int ORTHO_CHUNK = 128;   // tile records per LDS chunk
constexpr int ORTHO_SUB_W = 64, ORTHO_SUB_H = 4;   // the pixels of a workgroup: one wave per row
constexpr int ZONAL_CHUNK = 256;   // ring vertices per LDS chunk (one per lane of the workgroup, and the closing one)

struct TileRec {
  int32_t x0, y0, w, h;   // w = 0: the record takes no part (a bad index somewhere; nothing is read through it)
  int64_t poff, woff;
};

struct AssembleArgs {
  int64_t n_pred_bytes, T, n_weights, n_bin_entries, row0;
  int32_t n_tables, bin_side, bins_x, bins_y, width, n_rows, C, nodataval, subs_x, subs_y, by0;
};

template <typename CT> struct Acc;
template <> struct Acc<uint8_t> { typedef uint32_t type; __device__ static uint8_t fin(uint32_t v) { return (uint8_t)(v & 0xFFu); } };
template <> struct Acc<uint16_t> { typedef uint32_t type; __device__ static uint16_t fin(uint32_t v) { return (uint16_t)(v & 0xFFFFu); } };
template <> struct Acc<double> { typedef double type; __device__ static double fin(double v) { return v; } };

// preds: the tiles' predictions, concatenated (255, or any value >= C: ignored); pred_offsets [T + 1]; windows [T][4] col_off
// row_off width height in extent coordinates; tile_table [T]; weights: the tables in the count type, weight_offsets
// [n_tables + 1]; bin_ptr [bins_x bins_y + 1], bin_tiles: ascending tile indices per bin; classes [n_rows][width]; counts
// [C][n_rows][width] or null; stats [GR_ORTHO_STAT_WORDS].
template <typename CT>
__global__ __launch_bounds__(256) void k_assemble_tiles(const uint8_t *__restrict__ preds, const int64_t *__restrict__ pred_offsets,
                                                        const int32_t *__restrict__ windows, const int32_t *__restrict__ tile_table,
                                                        const CT *__restrict__ weights, const int64_t *__restrict__ weight_offsets,
                                                        const int64_t *__restrict__ bin_ptr, const int32_t *__restrict__ bin_tiles,
                                                        uint8_t *__restrict__ classes, CT *__restrict__ counts,
                                                        unsigned long long *__restrict__ stats, AssembleArgs a) {
  typedef typename Acc<CT>::type acc_t;
  __shared__ TileRec recs[ORTHO_CHUNK];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int bx = (int)blockIdx.x / a.subs_x, sx = (int)blockIdx.x % a.subs_x;
  const int by = a.by0 + (int)blockIdx.y / a.subs_y, sy = (int)blockIdx.y % a.subs_y;
  const int in_x = sx * ORTHO_SUB_W + lane, in_y = sy * ORTHO_SUB_H + (tid >> 6);
  const int64_t col = (int64_t)bx * a.bin_side + in_x, row = (int64_t)by * a.bin_side + in_y;
  const bool live = in_x < a.bin_side && in_y < a.bin_side && col < a.width && row >= a.row0 && row < a.row0 + a.n_rows;
  // the bin's list, clamped into the entries there are (O8)
  int64_t e0 = 0, e1 = 0;
  if (bx < a.bins_x && by < a.bins_y) {
    const int64_t b = (int64_t)by * a.bins_x + bx;
    e0 = min(max(bin_ptr[b], (int64_t)0), a.n_bin_entries);
    e1 = min(max(bin_ptr[b + 1], e0), a.n_bin_entries);
  }
  const int64_t n_list = e1 - e0;
  const bool one_chunk = n_list <= ORTHO_CHUNK;
  const int64_t plane = (int64_t)a.n_rows * a.width;
  const int64_t pix = live ? (row - a.row0) * a.width + col : 0;

  int cur = 256, nxt = 256;          // the class being summed, the next carried class above it; 256: none
  int next_store = 0;                // classes below it have their count stored
  int best_c = a.nodataval;
  acc_t best = 0;
  unsigned int covering = 0;
  for (int pass = 0;; ++pass) {
    if (pass > 0) {
      cur = nxt;
      if (!__syncthreads_or(cur < 256)) break;   // no lane of the workgroup has a further class
    }
    nxt = 256;
    acc_t total = 0;
    for (int64_t c0 = 0; c0 < n_list; c0 += ORTHO_CHUNK) {
      const int n_chunk = (int)min((int64_t)ORTHO_CHUNK, n_list - c0);
      if (pass == 0 || !one_chunk) {
        __syncthreads();   // the chunk before this one has been read by everybody
        if (tid < n_chunk) {
          TileRec r;
          r.x0 = r.y0 = r.w = r.h = 0; r.poff = r.woff = 0;
          const uint32_t t = (uint32_t)bin_tiles[e0 + c0 + tid];
          if ((int64_t)t < a.T) {
            const uint32_t k = (uint32_t)tile_table[t];
            const int32_t w = windows[(int64_t)t * 4 + 2], h = windows[(int64_t)t * 4 + 3];
            if (k < (uint32_t)a.n_tables && w > 0 && h > 0) {
              const int64_t n = (int64_t)w * h, po = pred_offsets[t], wo = weight_offsets[k];
              if (po >= 0 && po <= a.n_pred_bytes - n && wo >= 0 && wo <= a.n_weights - n) {
                r.x0 = windows[(int64_t)t * 4]; r.y0 = windows[(int64_t)t * 4 + 1]; r.w = w; r.h = h; r.poff = po; r.woff = wo;
              }
            }
          }
          recs[tid] = r;
        }
        __syncthreads();
      }
      if (live) {
        for (int j = 0; j < n_chunk; ++j) {
          const TileRec r = recs[j];
          const int64_t dx = col - r.x0, dy = row - r.y0;
          if (dx >= 0 && dx < r.w && dy >= 0 && dy < r.h) {   // never with w = 0
            const int64_t at = dy * r.w + dx;                 // < w h: inside the tile's predictions and its table
            const int v = (int)preds[r.poff + at];
            if (pass == 0) ++covering;
            if (v < a.C) {
              if (v == cur) total += (acc_t)weights[r.woff + at];
              else if (v > cur || pass == 0) nxt = min(nxt, v);
            }
          }
        }
      }
    }
    if (live && pass > 0 && cur < 256) {
      const CT count = Acc<CT>::fin(total);
      if (counts) {
        for (int c = next_store; c < cur; ++c) counts[(int64_t)c * plane + pix] = (CT)0;
        counts[(int64_t)cur * plane + pix] = count;
      }
      next_store = cur + 1;
      if ((acc_t)count > best) { best = (acc_t)count; best_c = cur; }   // strictly: the lowest class of the largest count
    }
  }
  if (live) {
    if (counts)
      for (int c = next_store; c < a.C; ++c) counts[(int64_t)c * plane + pix] = (CT)0;
    classes[pix] = (uint8_t)best_c;
  }
  const bool has_class = live && best > (acc_t)0;
  stat_count(stats, GR_ORTHO_STAT_WITH_CLASS, has_class, lane);
  stat_count(stats, GR_ORTHO_STAT_WITHOUT, live && !has_class, lane);
  stat_max(stats, GR_ORTHO_STAT_LONGEST_LIST, covering, lane);
  stat_add(stats, GR_ORTHO_STAT_PAIRS, covering, lane);
}

// The ring statistics of a ring table: one lane per ring (ring_stats of geom_dev.hpp); the words are GR_ZONAL_STAT_* or GR_BURN_STAT_*.
template <int LARGEST_RING, int RINGS_IGNORED>
__global__ __launch_bounds__(256) void k_zonal_ring_stats(const int64_t *__restrict__ roff, int64_t R, int64_t n_rv,
                                                          unsigned long long *__restrict__ stats) {
  ring_stats<LARGEST_RING, RINGS_IGNORED>(roff, R, n_rv, (int64_t)blockIdx.x * 256 + threadIdx.x, stats, (int)(threadIdx.x & 63));
}

// One work item of the zonal counts and of the burn, decoded: row p, the block of bw x bh cells from (col0, row0) in the
// coordinates of the parent grid, the rings [r_lo, r_hi) clamped to the rings there are.
struct CellItem { int64_t p; int col0, row0, bw, bh; int64_t r_lo, r_hi; };

// Item `index` of items [n][GR_ZONAL_ITEM_INTS]: polygon, col0, row0, width, height, first ring, one past the last ring.  False
// for an item that is malformed or leaves the window [col_off, col_off + width) x [row_off, row_off + height) (B7; the zonal
// counts' window is the raster, (0, 0, W, H)): the caller skips it whole, workgroup-uniform -- the host validates, the kernel
// reads nothing out of bounds (O8's rule).  The sums are taken in 64 bits.
__device__ __forceinline__ bool load_cell_item(const int32_t *__restrict__ items, int64_t index, int64_t P, int64_t R, int col_off,
                                               int row_off, int width, int height, CellItem &it) {
  const int32_t *w = items + index * GR_ZONAL_ITEM_INTS;
  it.p = w[0]; it.col0 = w[1]; it.row0 = w[2]; it.bw = w[3]; it.bh = w[4];
  it.r_lo = min(max((int64_t)w[5], (int64_t)0), R);
  it.r_hi = min(max((int64_t)w[6], it.r_lo), R);
  return it.p >= 0 && it.p < P && it.bw >= 1 && it.bh >= 1 && it.bw <= GR_ZONAL_BLOCK_W && it.bh <= GR_ZONAL_BLOCK_H &&
         it.col0 >= col_off && it.row0 >= row_off && (int64_t)it.col0 + it.bw <= (int64_t)col_off + width &&
         (int64_t)it.row0 + it.bh <= (int64_t)row_off + height;
}

// THE ring walk of the zonal counts and of the polygon burn (Z2, Z3 = B2): the parity word of this lane's cells of the item's
// block of bh <= 128 rows -- bit k: the centre of cell (row0 + wave + 4 k, col0 + lane) lies in row p under the even-odd rule
// (edge_crossing_strict of geom_dev.hpp, the 128-bit one) over the rings [r_lo, r_hi) that belong to p.  Called by the whole
// workgroup of 256 (it holds barriers); the ring vertices are staged in vx, vy (ZONAL_CHUNK + 1 words each), a chunk at a time.
// The caller waits at a barrier before it reuses the LDS.
__device__ __forceinline__ uint32_t zonal_parity_walk(const RingTable &t, const CellItem &it, int64_t *vx, int64_t *vy) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t px = 65536ll * (it.col0 + lane) + 32768;   // Z2
  uint32_t parity = 0;
  for (int64_t r = it.r_lo; r < it.r_hi; ++r) {
    if ((int64_t)t.rpoly[r] != it.p) continue;
    int64_t i0;
    const int64_t n = ring_span(t.roff, (int)r, t.n_rv, i0);
    if (n < 3) continue;
    for (int64_t k0 = 0; k0 < n; k0 += ZONAL_CHUNK) {
      const int n_chunk = (int)min((int64_t)ZONAL_CHUNK, n - k0);   // edges k0 + j -> k0 + j + 1 (the last one closes the ring)
      __syncthreads();
      if (tid <= n_chunk) {
        int64_t at = k0 + tid;
        if (at >= n) at -= n;   // only k0 + n_chunk == n wraps, to vertex 0
        vx[tid] = t.rv[(i0 + at) * 2];
        vy[tid] = t.rv[(i0 + at) * 2 + 1];
      }
      if (tid == 0 && n_chunk == ZONAL_CHUNK) {
        int64_t at = k0 + ZONAL_CHUNK;
        if (at >= n) at -= n;
        vx[ZONAL_CHUNK] = t.rv[(i0 + at) * 2];
        vy[ZONAL_CHUNK] = t.rv[(i0 + at) * 2 + 1];
      }
      __syncthreads();
      for (int k = 0; wave + 4 * k < it.bh; ++k) {
        const int64_t py = 65536ll * (it.row0 + wave + 4 * k) + 32768;
        int flips = 0;
        for (int j = 0; j < n_chunk; ++j) edge_crossing_strict(vx[j], vy[j], vx[j + 1], vy[j + 1], px, py, flips);
        parity ^= (uint32_t)(flips & 1) << k;
      }
    }
  }
  return parity;
}

struct ZonalArgs {
  int32_t H, W, nodata, C;
};

// raster [H][W]; t: the ring table, rv [n_rv][2] in 1/65536 of a cell (Z1), roff [R + 1], rpoly [R] non-decreasing, no hole flags
// and no boxes; items [n][GR_ZONAL_ITEM_INTS] (load_cell_item); counts [P][C]; stats [GR_ZONAL_STAT_WORDS].
__global__ __launch_bounds__(256) void k_zonal_class_counts(const uint8_t *__restrict__ raster, RingTable t,
                                                            const int32_t *__restrict__ items,
                                                            unsigned long long *__restrict__ counts,
                                                            unsigned long long *__restrict__ stats, ZonalArgs a) {
  __shared__ int64_t vx[ZONAL_CHUNK + 1], vy[ZONAL_CHUNK + 1];
  __shared__ uint32_t hist[GR_ZONAL_MAX_CLASSES];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  CellItem it;
  if (!load_cell_item(items, blockIdx.x, t.P, t.R, 0, 0, a.W, a.H, it)) return;
  const int64_t p = it.p;
  const int col0 = it.col0, row0 = it.row0, bw = it.bw, bh = it.bh;
  if (tid < a.C) hist[tid] = 0;   // C <= 256 = the workgroup
  // bit k: the row row0 + wave + 4 k
  const uint32_t parity = zonal_parity_walk(t, it, vx, vy);
  __syncthreads();   // the histogram is zeroed; the last chunk is read
  unsigned int n_in = 0, n_nodata = 0, n_over = 0, largest = 0;
  if (lane < bw) {
    for (int k = 0; wave + 4 * k < bh; ++k) {
      if (!((parity >> k) & 1u)) continue;
      const unsigned int v = raster[(int64_t)(row0 + wave + 4 * k) * a.W + col0 + lane];
      ++n_in;
      if ((int)v == a.nodata) { ++n_nodata; continue; }
      largest = max(largest, v + 1u);
      if ((int)v >= a.C) { ++n_over; continue; }
      atomicAdd(&hist[v], 1u);
    }
  }
  __syncthreads();
  if (tid < a.C && hist[tid]) atomicAdd(&counts[p * a.C + tid], (unsigned long long)hist[tid]);
  if (tid == 0) atomicAdd(&stats[GR_ZONAL_STAT_TESTED], (unsigned long long)bw * (unsigned long long)bh);
  stat_add_u32(stats, GR_ZONAL_STAT_INSIDE, n_in, lane);
  stat_add_u32(stats, GR_ZONAL_STAT_NODATA, n_nodata, lane);
  stat_add_u32(stats, GR_ZONAL_STAT_OVER, n_over, lane);
  stat_max(stats, GR_ZONAL_STAT_LARGEST_PLUS_1, largest, lane);
}

struct BurnArgs {
  int64_t P, n_cells;
  int32_t col_off, row_off, width, height, fill;
};

// The ring table as k_zonal_class_counts takes it; items in the coordinates of the PARENT grid (col0, row0 may be negative), each
// inside the window [col_off, col_off + width) x [row_off, row_off + height) (B1, B5); rows [height][width], -1 on entry;
// stats [GR_BURN_STAT_WORDS].
__global__ __launch_bounds__(256) void k_burn_rows(RingTable t, const int32_t *__restrict__ items, int32_t *__restrict__ rows,
                                                   unsigned long long *__restrict__ stats, BurnArgs a) {
  __shared__ int64_t vx[ZONAL_CHUNK + 1], vy[ZONAL_CHUNK + 1];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  CellItem it;
  if (!load_cell_item(items, blockIdx.x, t.P, t.R, a.col_off, a.row_off, a.width, a.height, it)) return;   // B7
  const int64_t p = it.p;
  const int col0 = it.col0, row0 = it.row0, bw = it.bw, bh = it.bh;
  const uint32_t parity = zonal_parity_walk(t, it, vx, vy);
  unsigned int n_in = 0;
  if (lane < bw) {
    const int64_t x = (int64_t)col0 + lane - a.col_off;   // in [0, width)
    for (int k = 0; wave + 4 * k < bh; ++k) {
      if (!((parity >> k) & 1u)) continue;
      const int64_t y = (int64_t)row0 + wave + 4 * k - a.row_off;   // in [0, height)
      atomicMax(&rows[y * a.width + x], (int)p);   // the result is not used: B3, the highest row, whatever the order
      ++n_in;
    }
  }
  if (tid == 0) atomicAdd(&stats[GR_BURN_STAT_TESTED], (unsigned long long)bw * (unsigned long long)bh);
  stat_add_u32(stats, GR_BURN_STAT_INSIDE, n_in, lane);
}

// B4: out = values[rows], `fill` where rows < 0 (or names no row); one lane per cell, the grid capped.  Counts the burned cells.
__global__ __launch_bounds__(256) void k_burn_values(const int32_t *__restrict__ rows, const uint8_t *__restrict__ values,
                                                     uint8_t *__restrict__ out, unsigned long long *__restrict__ stats, BurnArgs a) {
  const int lane = (int)(threadIdx.x & 63);
  unsigned long long burned = 0;   // wave-uniform
  for (int64_t base = (int64_t)blockIdx.x * 256; base < a.n_cells; base += (int64_t)gridDim.x * 256) {   // workgroup-uniform
    const int64_t i = base + threadIdx.x;
    bool hit = false;
    if (i < a.n_cells) {
      const int64_t p = rows[i];
      hit = p >= 0 && p < a.P;
      out[i] = hit ? values[p] : (uint8_t)a.fill;
    }
    burned += (unsigned long long)__popcll(__ballot(hit));
  }
  if (lane == 0 && burned) atomicAdd(&stats[GR_BURN_STAT_BURNED], burned);
}

}  // namespace

extern "C" {

int gr_assemble_tiles(gr_ctx *c, const uint8_t *preds, int64_t n_pred_bytes, const int64_t *pred_offsets, const int32_t *windows,
                      const int32_t *tile_table, int64_t T, const void *weights, int64_t n_weights, const int64_t *weight_offsets,
                      int32_t n_tables, int32_t count_dtype, const int64_t *bin_ptr, const int32_t *bin_tiles, int64_t n_bin_entries,
                      int32_t bin_side, int32_t bins_x, int32_t bins_y, int32_t width, int64_t row0, int32_t n_rows, int32_t C,
                      int32_t nodataval, uint8_t *classes, void *counts, uint64_t *stats, void *stream) {
  if (!c) return GR_EINVAL;
  if (n_pred_bytes < 0 || T < 0 || T > 0x7FFFFFFFll || n_weights < 0 || n_tables < 0 || n_bin_entries < 0 || row0 < 0 || n_rows < 0 ||
      width < 0)
    return fail(c, GR_EINVAL, "gr_assemble_tiles: negative size (or T >= 2^31)");
  if (C < 1 || C > GR_ORTHO_MAX_CLASSES) return fail(c, GR_EINVAL, "gr_assemble_tiles: C=%d outside [1, %d]", C, GR_ORTHO_MAX_CLASSES);
  if (nodataval < 0 || nodataval > 255) return fail(c, GR_EINVAL, "gr_assemble_tiles: nodataval=%d outside [0, 255]", nodataval);
  if (count_dtype != GR_COUNT_U8 && count_dtype != GR_COUNT_U16 && count_dtype != GR_COUNT_F64)
    return fail(c, GR_EINVAL, "gr_assemble_tiles: count type %d is not GR_COUNT_U8 / GR_COUNT_U16 / GR_COUNT_F64", count_dtype);
  if (bin_side < 1 || bins_x < 1 || bins_y < 1 || (int64_t)bins_x * bins_y > 0x7FFFFFFFll)
    return fail(c, GR_EINVAL, "gr_assemble_tiles: bad bin table side=%d bins=%d x %d", bin_side, bins_x, bins_y);
  if ((int64_t)bins_x * bin_side < width || (int64_t)bins_y * bin_side < row0 + n_rows)
    return fail(c, GR_EINVAL, "gr_assemble_tiles: %d x %d bins of side %d do not cover width %d, rows [%lld, %lld)", bins_x, bins_y,
                bin_side, width, (long long)row0, (long long)(row0 + n_rows));
  if (!stats || !bin_ptr || !pred_offsets || !weight_offsets || (T > 0 && (!windows || !tile_table)) || (n_pred_bytes > 0 && !preds) ||
      (n_weights > 0 && !weights) || (n_bin_entries > 0 && !bin_tiles) || ((int64_t)n_rows * width > 0 && !classes))
    return fail(c, GR_EINVAL, "gr_assemble_tiles: null arrays");
  AssembleArgs a;
  a.subs_x = (int)ceil_div(bin_side, ORTHO_SUB_W); a.subs_y = (int)ceil_div(bin_side, ORTHO_SUB_H);
  a.by0 = (int)(row0 / bin_side);
  const int64_t used_x = ceil_div(width, bin_side), used_y = n_rows > 0 ? (row0 + n_rows - 1) / bin_side - a.by0 + 1 : 0;
  const int64_t gx = used_x * a.subs_x, gy = used_y * a.subs_y;
  if (gx > 0x7FFFFFFFll || gy > 65535)
    return fail(c, GR_EINVAL, "gr_assemble_tiles: a band of %d rows is too tall for one launch (bin side %d)", n_rows, bin_side);
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  GR_HIP(c, hipMemsetAsync(stats, 0, sizeof(uint64_t) * GR_ORTHO_STAT_WORDS, s));
  if ((int64_t)n_rows * width == 0) return GR_OK;
  a.n_pred_bytes = n_pred_bytes; a.T = T; a.n_weights = n_weights; a.n_bin_entries = n_bin_entries; a.row0 = row0;
  a.n_tables = n_tables; a.bin_side = bin_side; a.bins_x = bins_x; a.bins_y = bins_y; a.width = width; a.n_rows = n_rows; a.C = C;
  a.nodataval = nodataval;
  const dim3 grid((unsigned)gx, (unsigned)gy), block(256);
  unsigned long long *st = (unsigned long long *)stats;
  if (count_dtype == GR_COUNT_U8)
    hipLaunchKernelGGL(k_assemble_tiles<uint8_t>, grid, block, 0, s, preds, pred_offsets, windows, tile_table, (const uint8_t *)weights,
                       weight_offsets, bin_ptr, bin_tiles, classes, (uint8_t *)counts, st, a);
  else if (count_dtype == GR_COUNT_U16)
    hipLaunchKernelGGL(k_assemble_tiles<uint16_t>, grid, block, 0, s, preds, pred_offsets, windows, tile_table, (const uint16_t *)weights,
                       weight_offsets, bin_ptr, bin_tiles, classes, (uint16_t *)counts, st, a);
  else
    hipLaunchKernelGGL(k_assemble_tiles<double>, grid, block, 0, s, preds, pred_offsets, windows, tile_table, (const double *)weights,
                       weight_offsets, bin_ptr, bin_tiles, classes, (double *)counts, st, a);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

int gr_zonal_class_counts(gr_ctx *c, const uint8_t *raster, int32_t H, int32_t W, int32_t nodata, const int64_t *ring_vertices,
                          int64_t n_ring_vertices, const int64_t *ring_offsets, const int32_t *ring_polygon, int64_t R, int64_t P,
                          const int32_t *items, int64_t n_items, int32_t C, uint64_t *counts, uint64_t *stats, void *stream) {
  if (!c) return GR_EINVAL;
  if (H < 1 || W < 1 || H >= (1 << 23) || W >= (1 << 23))
    return fail(c, GR_EINVAL, "gr_zonal_class_counts: raster %d x %d outside [1, 2^23)", H, W);
  GR_TRY(check_ring_table(c, "gr_zonal_class_counts", nullptr, ring_vertices, n_ring_vertices, ring_offsets, ring_polygon, nullptr, R,
                          nullptr, P, false));
  if (n_items < 0 || n_items > 0x7FFFFFFFll) return fail(c, GR_EINVAL, "gr_zonal_class_counts: a size is negative or not below 2^31");
  if (C < 1 || C > GR_ZONAL_MAX_CLASSES) return fail(c, GR_EINVAL, "gr_zonal_class_counts: C=%d outside [1, %d]", C, GR_ZONAL_MAX_CLASSES);
  if (!raster || !stats || (P > 0 && !counts) || (n_items > 0 && !items)) return fail(c, GR_EINVAL, "gr_zonal_class_counts: null arrays");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  GR_HIP(c, hipMemsetAsync(stats, 0, sizeof(uint64_t) * GR_ZONAL_STAT_WORDS, s));
  if (P > 0) GR_HIP(c, hipMemsetAsync(counts, 0, sizeof(uint64_t) * (size_t)P * (size_t)C, s));
  unsigned long long *st = (unsigned long long *)stats;
  if (R > 0) {
    hipLaunchKernelGGL((k_zonal_ring_stats<GR_ZONAL_STAT_LARGEST_RING, GR_ZONAL_STAT_RINGS_IGNORED>), dim3((unsigned)ceil_div(R, 256)), dim3(256), 0, s,
                       ring_offsets, R, n_ring_vertices, st);
    GR_HIP(c, hipGetLastError());
  }
  if (n_items == 0 || R == 0) return GR_OK;
  ZonalArgs a;
  a.H = H; a.W = W; a.nodata = nodata; a.C = C;
  const RingTable t{ring_vertices, ring_offsets, nullptr, ring_polygon, nullptr, n_ring_vertices, R, P};
  hipLaunchKernelGGL(k_zonal_class_counts, dim3((unsigned)n_items), dim3(256), 0, s, raster, t, items, (unsigned long long *)counts, st, a);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

int gr_burn_polygons(gr_ctx *c, const int64_t *ring_vertices, int64_t n_ring_vertices, const int64_t *ring_offsets,
                     const int32_t *ring_polygon, int64_t R, int64_t P, const uint8_t *values, const int32_t *items, int64_t n_items,
                     int32_t col_off, int32_t row_off, int32_t width, int32_t height, int32_t fill, int32_t *rows, uint8_t *out,
                     uint64_t *stats, void *stream) {
  if (!c) return GR_EINVAL;
  GR_TRY(check_window(c, "gr_burn_polygons", col_off, row_off, width, height));
  GR_TRY(check_ring_table(c, "gr_burn_polygons", nullptr, ring_vertices, n_ring_vertices, ring_offsets, ring_polygon, nullptr, R, nullptr,
                          P, false));
  if (n_items < 0 || n_items > 0x7FFFFFFFll) return fail(c, GR_EINVAL, "gr_burn_polygons: a size is negative or not below 2^31");
  if (fill < 0 || fill > 255) return fail(c, GR_EINVAL, "gr_burn_polygons: fill=%d outside [0, 255]", fill);
  if (!rows || !stats || (n_items > 0 && !items)) return fail(c, GR_EINVAL, "gr_burn_polygons: null arrays");
  if (out && P > 0 && !values) return fail(c, GR_EINVAL, "gr_burn_polygons: null values with an output plane");
  hipStream_t s = (hipStream_t)stream;
  const RingTable t{ring_vertices, ring_offsets, nullptr, ring_polygon, nullptr, n_ring_vertices, R, P};
  BurnArgs a;
  a.P = P; a.n_cells = (int64_t)width * height;
  a.col_off = col_off; a.row_off = row_off; a.width = width; a.height = height; a.fill = fill;
  GR_HIP(c, hipSetDevice(c->device));
  GR_HIP(c, hipMemsetAsync(stats, 0, sizeof(uint64_t) * GR_BURN_STAT_WORDS, s));
  GR_HIP(c, hipMemsetAsync(rows, 0xFF, sizeof(int32_t) * (size_t)a.n_cells, s));   // -1: no row
  unsigned long long *st = (unsigned long long *)stats;
  if (R > 0) {
    hipLaunchKernelGGL((k_zonal_ring_stats<GR_BURN_STAT_LARGEST_RING, GR_BURN_STAT_RINGS_IGNORED>), dim3((unsigned)ceil_div(R, 256)), dim3(256), 0, s,
                       ring_offsets, R, n_ring_vertices, st);
    GR_HIP(c, hipGetLastError());
  }
  if (n_items > 0 && R > 0) {
    hipLaunchKernelGGL(k_burn_rows, dim3((unsigned)n_items), dim3(256), 0, s, t, items, rows, st, a);
    GR_HIP(c, hipGetLastError());
  }
  if (out) {
    const unsigned groups = (unsigned)min(ceil_div(a.n_cells, (int64_t)256), (int64_t)GR_BURN_MAX_GROUPS);
    hipLaunchKernelGGL(k_burn_values, dim3(groups), dim3(256), 0, s, rows, values, out, st, a);
    GR_HIP(c, hipGetLastError());
  }
  return GR_OK;
}

}  // extern "C"
