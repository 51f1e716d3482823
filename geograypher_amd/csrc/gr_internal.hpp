#pragma once
// geograypher_amd/csrc/gr_internal.hpp -- what the translation units of libgeograster share: constants, the kernel
// argument blocks, the context, and the host-side helpers (error text, HIP-event spans, the context's device memory: Buf, reserve,
// release_all from device_buffer.hpp, instantiated here with DeviceMem; the stage arena: Scratch, stage_acquire; its layouts come
// from scratch_layout.hpp, the sorts and scans that run in it from cub_steps.hpp).
//   geograster.hip   context, options, learned binning table, the raster call (launch groups, side stream), status
//   mesh_upload.hip  gr_mesh_upload: Morton order, de-indexed soup, block bounds            (per upload); the tests' read-backs
//                    (gr_debug_read_upload, gr_debug_read_stage)
//   binning.hip      k_cull_blocks, k_setup_cull, k_clip_faces, entry compilation, exact-path scan / fill  (per view)
//   raster_tile.hip  k_raster_tile: the dominant kernel
//   project.hip      winners, votes, gathers, sparse pairs (label images, rectangle tables, polygon rings), finalize, argmax + their entry points
//   warp.hip         distortion warp, lens inversion (row f1)
//   resize.hip       photo down-scale of get_image (anti-aliased resize)
//   rays.hip         multiview detections: ray-pair graph (k_ray_prep, k_ray_pairs + radix sort), ray / boundary clip; no mesh needed
//   equirect.hip     360-degree photos: perspective views resampled from an equirectangular image (k_equirect_view)
//   cover.hip        covering meshes: bounds of a point set (k_points_bounds), highest / lowest member per grid cell (k_cover_grid); no mesh needed
//   polygons.hip     label_polygons: weighted face area per (polygon, class), exact containment or clipped overlay (k_polygon_weights); no mesh needed
//                    vector textures: the polygon row of every face centre through a cell index (k_face_polygon_index)
//                    region of interest: points in a buffered union of rows (k_points_in_region), the sub-mesh they select (k_submesh_flags, k_submesh_write + two scans)
//                    class outlines: canonical vertices (k_outline_canon), face edges (k_outline_face_edges), cancellation (k_outline_cancel), successors
//                    (k_outline_successor), leader and rank rounds (k_outline_round), ring emit (k_outline_emit_rings) + radix sorts and scans
//                    member outlines (detection footprints): the edges of the (face, class) members of a sparse table (k_outline_member_edges),
//                    then the trace of the class outlines (outline_trace, which both calls share)
//   terrain.hip      raster samples: the value of a raster under every face centre or vertex, height above it, ground relabel (k_sample_raster); no mesh needed
//   select.hip       image selection: greedy set cover over a face x view incidence (k_sc_rows, k_sc_scan, k_sc_scatter, k_sc_pick, k_sc_apply,
//                    k_sc_prune_test, k_sc_prune_apply); no mesh needed
//   crs.hip          CRS reprojection: points between WGS84 ECEF, geographic and transverse Mercator coordinates (k_reproject_points; the conversion
//                    of one point is crs_dev.hpp's, the constants crs_constants.hpp's, written by tools/make_crs_constants.py); no mesh needed
//   ortho.hip        orthomosaic baseline: tile predictions assembled into a class raster (k_assemble_tiles), class counts of the raster cells
//                    under polygon rows (k_zonal_class_counts, k_zonal_ring_stats), polygon rows burned into a label raster (k_burn_rows,
//                    k_burn_values; one ring walk with the counts, zonal_parity_walk, and one item decode, load_cell_item); no mesh needed
//   decimate.hip     mesh decimation by vertex clustering: cell keys and centre distances (k_decim_keys), cell heads (k_decim_heads),
//                    representatives (k_decim_scatter_rep), remapped faces (k_decim_faces), first face per triple (k_decim_face_flags)
//                    + radix sorts and scans; compacts with k_submesh_write; no mesh needed
//   overlap.hip      polygon-on-polygon overlap areas: candidate pairs of two box tables, count then fill (k_overlap_pairs_count,
//                    k_overlap_pairs_fill + a scan), the area of every pair as a signed sum over edge pairs (k_overlap_areas: one work item per
//                    workgroup, the a-tile as edge records in LDS), its partials added in item order (k_overlap_item_keys + a running
//                    maximum, k_overlap_reduce), table statistics (k_overlap_table_stats); float64, no atomics on it; no mesh needed
//   communities.hip  communities of the ray graph: a synchronous Louvain on integer weights -- directed entries (k_comm_edges), rows (k_comm_rows),
//                    the move kernel's three paths by row length (k_comm_move_wave, k_comm_move_group, k_comm_key_emit / _scores / _apply),
//                    tot and size (k_comm_tot_size), dense ranks and the coarse entries (k_comm_alive, k_comm_relabel), the ordered result
//                    (k_comm_members, k_comm_order_keys, k_comm_write_communities, k_comm_write_labels) + radix sorts, sums by key and scans;
//                    int64 sums only; no mesh needed
//   simplify.hip     ring simplification, an exact level-synchronous Douglas-Peucker: rings, anchors and the rotated order (k_simp_rings,
//                    k_simp_anchor_low, k_simp_rotate, k_simp_chains + two running maxima), a pass over all open chains (k_simp_round<0..4>:
//                    64-bit atomicMax rounds over the limbs of w and the tie-break, k_simp_publish, k_simp_apply; one word read back),
//                    collapse and output (k_simp_ring_sums, k_simp_flags, a FlagScan, k_simp_write); integers only; no mesh needed
//   nadir.hip        the top-down raster of a mesh (gr_nadir_raster): two walks over the (face, cell) pairs -- k_nadir_faces<0, 1>, a lane per face:
//                    N3, the clipped box of centres, the cells of the small faces, the list of the larger ones; k_nadir_items<0, 1>, a wave per
//                    item of a listed face -- a 64-bit atomicMax of the height's key, then an atomicMin of the face index where the key is the
//                    cell's maximum; k_nadir_finish decodes the keys in place; exact integer membership, float64 heights; no mesh needed
//   vis.hip          the pictures (gr_shade_view, gr_composite_labels): k_face_light, a lane per face; k_shade, a workgroup per 16 x 16 output pixels
//                    with the depth window and its halo in LDS, float32; k_composite, a workgroup per 1024 pixels of a row, byte strips through
//                    LDS by 16-byte words, float64; one host descriptor a call, no mesh, no scratch, no read-back
//   raster_warp.hip  raster -> raster (gr_warp_raster): k_warp_raster<cross-CRS, bilinear>, a lane per destination cell, a workgroup per 256 columns of a
//                    row; the cell centre through crs_dev.hpp's convert where the CRSs differ, a nearest sample or four taps per band; uint8, float32
//                    and float64 on either side; one host descriptor, no mesh, no scratch, no read-back
//   components.hip   the face sieve (gr_face_sieve): k_sieve_keys and one sort put the faces of an edge side by side; per round a union-find over the
//                    same-class pairs (k_cc_hook, k_cc_compress), integer measures (k_measure, k_count_small), the greatest labelled neighbour in
//                    two atomic passes (k_target), k_pointers, k_jump, k_relabel; one host descriptor, one word read back per round; no mesh needed
//   nearest.hip      nearest points (gr_nearest_points): k_nn_bounds, then per level k_nn_keys and one sort put the refs of a grid cell side by side,
//                    k_nn_gather lays their coordinates out in that order, k_nn_query walks the shells of cells round each query (a lower bound
//                    in the sorted keys per run of cells, no cell table) and lists the queries it could not settle for the next, coarser
//                    level; one host descriptor, the bounds and one word per level read back; no mesh needed
//   crs_dev.hpp      the conversion of one point between the WGS84 systems (G1-G8): CrsSide, CrsArgs, wrap_pi, clenshaw, taup_of, convert, crs_side
//                    (crs.hip, raster_warp.hip)
//   cub_steps.hpp    the hipcub calls of the stage calls, each declared once against the call's Plan: SortPairs, SortKeys, ExclusiveSum,
//                    InclusiveMax, RunLengthEncode, ReduceByKey (size query on construction, typed pointers on run)
//   compact_dev.hpp  FlagScan, compact_begin, compact_write, k_submesh_write: the scans and the write kernel of polygons.hip's sub-mesh and of decimate.hip;
//                    communities.hip ranks its surviving communities with FlagScan, simplify.hip compacts its kept ring vertices with it
//   geom_dev.hpp     device helpers of polygons.hip, terrain.hip, select.hip, crs.hip, ortho.hip, overlap.hip, simplify.hip and nadir.hip: orient, ring_span, edge_crossing (THE even-odd rule of
//                    k_polygon_weights, k_face_polygon_index and k_points_in_region), edge_crossing_strict (rule Z3: ortho.hip's ring walk, nadir.hip's faces),
//                    RingTable (ortho.hip, overlap.hip), ring_of_slot (overlap.hip, simplify.hip), load_face, stat_add / stat_add_u32 / stat_max / stat_count / ring_stats
//   (below)          the entry checks of the ring-table and grid-window calls: check_ring_table (ortho.hip, overlap.hip), check_window (ortho.hip, nadir.hip, raster_warp.hip)
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "geograster.h"
#include "device_buffer.hpp"
#include "scratch_layout.hpp"

// ------------------------------------------------------------------------------------------------------------------
// constants
// ------------------------------------------------------------------------------------------------------------------
#define GR_TILE 64          // tile width in pixels (a workgroup rasterizes 64x32 or 64x64 tiles out of LDS)
#define GR_TILE_LOG2 6
#define GR_MAX_BATCH 64     // views per launch group (amortises kernel boundaries and per-launch tails)
#define GR_ENT_Q 3          // int4 per compiled (face, tile) entry: 48 bytes, 12 words
#define GR_CTRL_HDR 8       // ctrl words before the tile arrays (GR_CTRL_* below)
#define GR_MAX_DIM 16384    // h, w limit (guard band and 16-bit bbox packing)
#define GR_BLOCK 64         // faces per block of the Morton-ordered soup: one wave, one bounding sphere
#define GR_BLOCK_VERTS 192  // distinct vertices a block can have (3 per face); a patch of a manifold mesh has about 48
namespace grimpl {

// The words of the overflow protocol, named once: kernels, host decode and the vote pass all index through these.
enum {  // header of a view's `ctrl` slot (BinArgs::ctrl); word 5 is unused
  GR_CTRL_RECORDS = 0,   // records (faces that survived culling; a clipped face several)
  GR_CTRL_ENTRIES = 1,   // (face, tile) entries of the view
  GR_CTRL_OVERFLOW = 2,  // != 0: the view's lists are incomplete; single-pass binning: the OR of GR_WHY_*
  GR_CTRL_WORK = 3,      // blocks that passed the frustum test (BinArgs::work)
  GR_CTRL_CLIP = 4,      // faces on the clip list (BinArgs::clip)
  GR_CTRL_MICRO = 6      // micro faces (pixel box at most 4 x 4)
};
enum {  // the call's statistics block (BinArgs::stats), summed / maximised over its views
  GR_ST_RECORDS = 0,      // records
  GR_ST_ENTRIES = 1,      // entries
  GR_ST_MAX_ENTRIES = 2,  // largest entry count: of a tile (single-pass binning), of a view (exact binning)
  GR_ST_OVERFLOW = 3,     // != 0: some view overflowed
  GR_ST_FIRST_GROUP = 4,  // first launch group that overflowed (~0: none)
  GR_ST_SHORT_MISS = 5,   // != 0: a face the 40-byte entry cannot hold (the caller repeats with 48 bytes)
  GR_ST_BLOCKS = 6,       // 64-face blocks that passed the frustum cull
  GR_ST_VISITS = 7,       // (view, 64-face group) pairs the vote passes visited
  GR_ST_MICRO = 8,        // micro faces
  GR_ST_REC_NEED = 9,     // records the most demanding view needs (exact binning)
  GR_ST_CAUSES = 10,      // the call's overflow causes, ORed (GR_WHY_*)
  GR_ST_WORDS = 11,       // words in use
  GR_ST_ALLOC = 16        // words allocated
};
enum {  // overflow causes (GR_CTRL_OVERFLOW, GR_ST_CAUSES; what gr_raster_overflow_causes reports as GR_CAUSE_*)
  GR_WHY_OUTGREW = GR_CAUSE_LIST_OUTGREW,    // a list outgrew its slots
  GR_WHY_SHORT_MISS = GR_CAUSE_SHORT_MISS,  // a face did not fit the 40-byte entry form
  GR_WHY_MET = GR_CAUSE_LISTS_MET,        // with micro lists: a tile's two lists met
  GR_WHY_ALL = GR_WHY_OUTGREW | GR_WHY_SHORT_MISS | GR_WHY_MET
};

struct BinArgs {
  uint32_t *ctrl;        // [slot][GR_CTRL_HDR + 4*Tcap]  header (GR_CTRL_*) | cntS[T] | cntB[T] | offset[T] | curB[T]
                         //   cntS: entries whose list position was handed out in k_setup_cull (faces touching <= 2x2 tiles)
                         //   cntB: entries of larger faces, placed by k_fill_compile behind the cntS block of their tile (exact path)
  int4 *rec;             // [slot][4][F]  plane0 {X0,Y0,X1,Y1} plane1 {X2,Y2,iz0,face} plane2 {A,B,jmin|jmax<<16,imin|imax<<16}
                         //               plane3 {list position in up to 4 tiles}
  const float *soup;     // [F][9] the three vertex positions of every face, in Morton order (built once per upload)
  const float *bvert;    // [ceil(F/64)][GR_BLOCK_VERTS][3] the DISTINCT vertices of every 64-face block, in order of first use
  const uint32_t *bidx;  // [F] positions of the face's three vertices in its block's list (8 bits each) | (distinct vertices - 1) << 24
  const int32_t *orig;   // [F] soup position -> face id of the caller's mesh
  const float4 *blk;     // [ceil(F/64)] bounding sphere (centre, radius) of each block of GR_BLOCK faces, local frame
  uint32_t *touched;     // fused aggregation: [slot][tw] a BYTE per group of 64 consecutive CALLER face ids that received a winner in the
                         // view (set by the tile kernel's epilogue beside its winner atomic; zeroed by the group's init kernel), or null
  int tw;                // words per slot of `touched`
  uint32_t *work;        // [slot][work_stride] blocks of this view that passed the frustum test (ctrl[GR_CTRL_WORK] = count)
  uint32_t *clip;        // [slot][F] soup faces that straddle the near plane / guard band (R7; ctrl[GR_CTRL_CLIP] = count)
  int64_t work_stride;
  int4 *comp;            // [slot][ent_cap][GR_ENT_Q]  compiled (face, tile) entries grouped by tile, 48 bytes each (ent40: 40 bytes
                         //                            each at the front of the same slot memory)
  uint8_t *nrow8;        // [slot][ent_cap] rows of each entry inside its tile (the tile kernel's scan input: a compact stream)
  unsigned long long *stats;  // [GR_ST_ALLOC] the call's statistics, GR_ST_WORDS in use (GR_ST_* above)
  int group;             // index of this launch group inside the call
  int64_t ctrl_stride;   // words per slot
  int64_t rec_stride;    // int4 per slot: four planes of rec_stride / 4 >= F records
  int64_t ent_cap;       // entries per slot
  int64_t F;
  int T, TX, TY, Tcap;   // Tcap: WORDS per counter array (the tile count rounded up to 4, times the counter stride)
  int clg;               // tile t's counters are cntS[cidx(a, t)], cntB[cidx(a, t)]: -1 = packed side by side; >= 0 = spread over 2^clg lines of
                         // 128 bytes, tile t in line t mod 2^clg at word t div 2^clg (2^clg >= T: every tile a line of its own)
  int h, w;
  int twl, thl;          // log2 of the tile width / height in pixels
  int cap_tile;          // > 0: single-pass binning, every tile owns cap_tile entry slots (list base = tile * cap_tile)
  int ent40;             // 1: entries are written in the SHORT form (40 bytes, store_entry below); single-pass binning only
  int count_micro;       // 1: K1 counts the view's micro faces (pixel box at most 4 x 4) for gr_raster_stats: calls that can still learn micro lists
  int micro;             // 1: (face, tile) pairs of at most 4 x 4 pixels go to the tile's second list (K1 / raster_one_tile); needs ent40
  int var;               // variant bits (GR_OPT_VARIANT, include/geograster.h)
  int gl_order;          // GR_OPT_VERTEX_ORDER: 1 = the second half of the vertex stage in an OpenGL pipeline's order of operations
#ifdef GR_STAMPS
  unsigned long long *stamps;  // diagnostic build: [16] cycles per tile-kernel phase, summed over waves (raster_tile.hip)
#endif
  int dbg;               // GR_OPT_DEBUG: GR_DBG_POISON_SLOTS (a TEST hook, results stay right): entry slots and row counts are poisoned with 0xFF
                         // before every launch group is binned
};

// word of tile t's counter inside a counter array (BinArgs::clg)
__device__ __forceinline__ int64_t cidx(const BinArgs &a, int t) {
  return a.clg < 0 ? (int64_t)t : (int64_t)((((uint32_t)t & ((1u << a.clg) - 1u)) << 5) | ((uint32_t)t >> a.clg));
}

// The SEGMENT of a tile under single-pass binning: cap_tile slots of entry memory (BinArgs::comp), written by k_setup_cull and
// k_clip_faces (binning.hip: store_entry, the record writer of k_setup_cull), read by the tile kernel (raster_tile.hip).  The slot memory is sized
// for full entries; short entries pack chunks of 64 at the front of the segment -- the 64 32-byte parts {s0 .. s7} first, then
// the 64 8-byte parts {s8, s9} --, and with micro lists the tile's second list grows from the segment's END, record p being
// the GR_MICRO_BYTES that end p records before it.
enum {
  GR_ENT_BYTES = GR_ENT_Q * 16,             // a full entry
  GR_ENT40_BYTES = 40,                      // a short entry (BinArgs::ent40)
  GR_CHUNK40_BYTES = 64 * GR_ENT40_BYTES,   // a chunk of 64 short entries: 2560
  GR_CHUNK40_TAIL = 64 * 32,                // ... where its 8-byte parts start: 2048
  GR_MICRO_BYTES = 32,                      // a micro record
  // the micro list's own bound: records that fill the whole segment, cap_tile * GR_ENT40_BYTES / GR_MICRO_BYTES = 5/4 cap_tile
  GR_MICRO_CAP_NUM = GR_ENT40_BYTES / 8,
  GR_MICRO_CAP_DEN = GR_MICRO_BYTES / 8
};
__device__ __forceinline__ uint32_t micro_cap(uint32_t cap_tile) { return cap_tile * GR_MICRO_CAP_NUM / GR_MICRO_CAP_DEN; }
__device__ __forceinline__ bool micro_fits(uint32_t n_rec, uint32_t cap_tile) {   // n_rec <= micro_cap(cap_tile), for a count that may be torn
  return n_rec * GR_MICRO_CAP_DEN <= cap_tile * GR_MICRO_CAP_NUM;
}
// slots of a segment that n_ent short entries (whole chunks from the front) and n_mic micro records (from the back) take together
__device__ __forceinline__ uint32_t seg_slots_used(uint32_t n_ent, uint32_t n_mic) {
  return ((n_ent + 63u) & ~63u) + (n_mic * GR_MICRO_BYTES + (GR_ENT40_BYTES - 1)) / GR_ENT40_BYTES;
}
// the box word of a micro record: first column (6 bits) | columns - 1 (2) | first row (6) | rows (3), inside the tile
struct MicroBox { int col0, dcol, row0, rows; };
__device__ __forceinline__ int pack_micro_box(int c0, int c1, int q0, int q1) { return c0 | ((c1 - c0) << 6) | (q0 << 8) | ((q1 - q0 + 1) << 14); }
__device__ __forceinline__ MicroBox unpack_micro_box(int box) { return {box & 63, (box >> 6) & 3, (box >> 8) & 63, (box >> 14) & 7}; }

struct RasterOut {
  int32_t *ids;      // [slot][h][w] or null
  float *depth;      // [slot][h][w] or null
  uint32_t *winner;  // fused projection: [slot][F] keys = (last pixel of the face in the view) + 1, or null
  uint8_t *touched;  // ... and [slot][4 tw] the byte map of the 64-face groups that hold a winner (BinArgs::touched)
  int64_t tb;        // bytes per slot of `touched`
  int64_t F;
  int compat;        // GR_FLAG_NEG1_IS_LAST_FACE
};

// A block of per-call device scratch and the stream of its last user (stage_acquire below).
struct Scratch : Buf<uint8_t> { hipStream_t last = nullptr; };

}  // namespace grimpl

struct gr_ctx {
  int device = 0;
  const float *verts = nullptr;
  const int32_t *faces = nullptr;
  int64_t V = 0, F = 0;
  // Device memory: every buffer is a Buf (device_buffer.hpp: pointer and element count), grown by reserve, named in each_buffer.
  // bin scratch
  grimpl::Buf<uint32_t> ctrl, work;
  grimpl::Buf<int4> rec, comp;
  grimpl::Buf<uint8_t> nrow8;
  grimpl::Buf<uint32_t> clip;      // [slot][F] clip lists (R7)
  grimpl::Buf<uint32_t> touched;   // fused aggregation: [2][slots][tw] group maps (a byte per 64 faces) of the launch groups in flight
  grimpl::Buf<uint32_t> visits;    // ... [F / 64] (view, group) pairs the vote passes of the current call visited (gr_raster_stats.chunk_visits)
  bool visits_pending = false;     // ... not added into the call's statistics yet (gr_raster_status does)
  uint32_t *cur_touched = nullptr; // the bitmap the next bin_batch fills (null: none)
  int cur_tw = 0;
  // the mesh buffers: one group (gr_mesh_upload: reserve_group), all five hold at least these lengths or all are empty
  grimpl::Buf<float4> blk;         // [ceil(F / GR_BLOCK)]
  grimpl::Buf<float> soup;         // [9 F]
  grimpl::Buf<float> bvert;        // [3 GR_BLOCK_VERTS ceil(F / GR_BLOCK)] distinct vertices per 64-face block (k_block_vertices)
  grimpl::Buf<uint32_t> bidx;      // [F] per soup face: its vertices' positions in the block's list
  grimpl::Buf<int32_t> orig;       // [F] soup position -> caller's face id (Morton order)
  grimpl::Buf<unsigned long long> stats;   // [GR_ST_ALLOC]
  grimpl::Buf<int> flag;           // [8] flag word + upload scratch (vertex bounds)
  int64_t ctrl_stride = 0, rec_stride = 0, work_stride = 0, ent_cap = 0, ent_cap_request = 0;
  int Tcap = 0, slots = 0, clg = -1;
  int64_t rec_F = 0;                   // records per plane and slot of the exact path (>= F)
  int64_t rec_cap_request = 0;         // ... asked for by a call whose clipped faces outgrew F records (gr_raster_status)
  // tuning knobs (gr_set_option)
  int opt_thl = 5;      // log2 tile height (5 or 6); width is 64.  64x32 tiles: 16 KiB of LDS, 8 workgroups per CU
  int opt_batch = GR_MAX_BATCH;
  int opt_dbg = 0;
  int opt_var = 0;
  int opt_gl_order = 0;  // GR_OPT_VERTEX_ORDER
  int opt_lds_pad = 0;   // extra dynamic LDS bytes per tile workgroup (occupancy experiments, GR_OPT_DEBUG_LDS)
  int opt_direct_cap = 512;  // single-pass binning: entry slots per tile (0 = always use the exact two-pass path)
  struct Learned { uint64_t mesh; int T, cap; bool full; bool micro = false; };
  Learned learned[8] = {};             // slots per tile learned from overflows -- and whether the image has faces the 40-byte entry
                                       // form cannot hold --, per (mesh signature, tile count); [n_learned % 8] is replaced next
  int n_learned = 0;
  bool share_learned = true;           // consult / feed the process-wide table (off once GR_OPT_DIRECT_CAP was set by hand, on
                                       // again only with GR_OPT_SHARE_LEARNED)
  uint64_t mesh_sig = 0;               // signature of the uploaded mesh: face count, vertex count, vertex bounds (gr_mesh_upload)
  // The binning configuration of the CURRENT raster call, resolved once at its top (resolve_binning): the process-wide table
  // can change under a running call (another context, another thread) -- sizing, allocation, the bin pass and the tile pass
  // of every launch group must agree on the slots per tile and on the entry form.
  int cur_cap = 0;                     // single-pass binning: slots per tile (0: exact two-pass binning)
  bool cur_ent40 = false;              // 40-byte entries
  bool cur_micro = false;              // micro lists (faces of at most 4 x 4 pixels on a second list per tile) for this call
  bool cur_count_micro = false;        // ... and whether this call counts micro faces (it can still learn the lists)
  bool cur_look = false;               // nothing learned about this (mesh, image size): the first launch group's counts are read
                                       // before its tile kernel runs (raster_views)
  int rebinned = 0;                    // times the last raster call started over after that look
  int causes = 0;                      // overflow causes the last raster call met, as read by that look and gr_raster_status
  bool stats_pending = false;          // the call's statistics have not been reset yet (the first launch group's init kernel does)
  bool defer_stats = false;            // this call's view totals (k_bin_stats) wait for gr_raster_status: one launch group, not fused, no look
  bool stats_deferred = false;         // ... and have not been added up yet
  grimpl::BinArgs deferred_args;               // ... with these arguments, for deferred_nb views
  int deferred_nb = 0;
  int64_t opt_budget_mb = 24 << 10;    // entry memory of one launch group (GR_OPT_DIRECT_BUDGET_MB)
  int last_T = 0, last_B = 0;          // tile count and launch-group size of the last raster call
  int last_n_views = 0;
  bool direct_ok = true;     // cleared when a tile overflowed its slots: later calls take the exact path
  bool last_direct = false;
  grimpl::Buf<uint32_t> winner;   // winner scratch (reserve_winner)
  // fused aggregation: the vote kernel of launch group g runs on a side stream beside the binning of group g + 1
  hipStream_t side = nullptr;
  hipEvent_t ev_raster[2] = {nullptr, nullptr}, ev_vote[2] = {nullptr, nullptr};
  grimpl::Buf<unsigned long long> stamps;  // GR_STAMPS (diagnostic build) only: phase cycles of the tile kernel, summed since the last read
  // The stage arena: the per-call scratch of every stage call (the mesh upload's sort, pair counts, ray pairs, resize, point
  // bounds, region, sub-mesh, class outlines, set cover), one call at a time, each carving what it needs from offset 0.
  grimpl::Scratch stage;
  grimpl::Scratch stage_b;             // gr_class_outlines alone: its second block is sized after a read-back, while the first is live
  hipStream_t last_stream = nullptr;   // of the last raster call (gr_raster_status reads its outcome there)
  std::vector<hipStream_t> used_streams;  // streams that work touching context scratch was enqueued on since the last quiesce
  // profiling
  bool profiling = false;
  struct Span { hipEvent_t a, b; int stage; bool own_a = true; };   // own_a false: `a` is the `b` of the span before (a chain of launch-attached stop events)
  hipEvent_t chain_ev = nullptr;       // the stop event of the latest instrumented launch of the running raster call (chain_stop)
  bool chain_first = false;
  std::vector<Span> spans;
  std::vector<hipEvent_t> pool;
  int prof_views = 0, prof_raster_launches = 0;
  char err[512] = {0};
  template <class V> void each_buffer(V &&v) {   // THE list of the context's device buffers (release_all in gr_ctx_destroy)
    v(ctrl); v(rec); v(comp); v(nrow8); v(work); v(clip); v(touched); v(visits); v(blk); v(soup); v(bvert); v(bidx); v(orig);
    v(stats); v(flag); v(winner); v(stamps); v(stage); v(stage_b);
  }
};

namespace grimpl {

inline int fail(gr_ctx *c, int code, const char *fmt, ...) {
  if (c) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c->err, sizeof(c->err), fmt, ap);
    va_end(ap);
  }
  return code;
}

#define GR_HIP(ctx, call)                                                                          \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess) return fail(ctx, GR_EHIP, "%s: %s", #call, hipGetErrorString(e_));       \
  } while (0)

enum { ST_SETUP = 0, ST_SCAN, ST_FILL, ST_RASTER, ST_PROJECT, ST_VOTE, ST_GATHER, ST_N };

inline hipEvent_t take_event(gr_ctx *c) {
  hipEvent_t e;
  if (!c->pool.empty()) { e = c->pool.back(); c->pool.pop_back(); return e; }
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

struct Timed {  // RAII span around a kernel group when profiling is on
  gr_ctx *c; hipStream_t s; int stage; hipEvent_t a = nullptr, b = nullptr;
  Timed(gr_ctx *c_, hipStream_t s_, int st) : c(c_), s(s_), stage(st) {
    if (c->profiling && st >= 0) { a = take_event(c); b = take_event(c); if (a) (void)hipEventRecord(a, s); }   // (st < 0: no span)
  }
  ~Timed() {
    if (c->profiling && a && b) { (void)hipEventRecord(b, s); gr_ctx::Span sp; sp.a = a; sp.b = b; sp.stage = stage; c->spans.push_back(sp); }
  }
};

// Spans whose events ride on kernel LAUNCHES (hipExtLaunchKernelGGL's stop event: the END of that kernel) instead of being
// recorded between kernels: an event record is a packet of its own on the stream and costs the kernels behind it 3.8 us -- four
// of them 1.65 % of a C2 step, 4.3 % of a quarter-scale one (tools/event_cost.py).  (The launch's START event is no use: it is
// stamped when the packet is taken up, while the kernel before it still runs.)  So the stages of a raster call are timed as a
// CHAIN of ends: chain_begin -> the end of the kernel in front of the first stage (k_bin_init); chain_stop(stage) -> the end of
// the stage's last kernel, the span [previous end, this end] -- the launch gap in front of a kernel is part of its span.
inline hipEvent_t chain_begin(gr_ctx *c) {
  if (c->chain_ev && c->chain_first) c->pool.push_back(c->chain_ev);   // a chain that was begun and never continued
  c->chain_ev = c->profiling ? take_event(c) : nullptr;
  c->chain_first = true;
  return c->chain_ev;
}
inline hipEvent_t chain_stop(gr_ctx *c, int stage) {
  if (!c->profiling || !c->chain_ev) return nullptr;
  hipEvent_t e = take_event(c);
  if (!e) return nullptr;
  gr_ctx::Span sp; sp.a = c->chain_ev; sp.b = e; sp.stage = stage; sp.own_a = c->chain_first;
  c->spans.push_back(sp);
  c->chain_first = false;
  c->chain_ev = e;
  return e;
}
inline void release_spans(gr_ctx *c) {   // events back to the pool
  if (c->chain_ev && c->chain_first) c->pool.push_back(c->chain_ev);
  c->chain_ev = nullptr; c->chain_first = false;
  for (auto &sp : c->spans) { if (sp.own_a) c->pool.push_back(sp.a); c->pool.push_back(sp.b); }
  c->spans.clear();
}
// launch KERNEL with (optional) start / stop events attached
#define GR_LAUNCH_EV(EVA, EVB, KERNEL, GRID, BLOCK, SHMEM, STREAM, ...)                                        \
  do {                                                                                                         \
    const hipEvent_t eva_ = (EVA), evb_ = (EVB);   /* evaluated ONCE: chain_stop takes an event and pushes a span */ \
    if (eva_ || evb_) hipExtLaunchKernelGGL(KERNEL, GRID, BLOCK, SHMEM, STREAM, eva_, evb_, 0, __VA_ARGS__);   \
    else hipLaunchKernelGGL(KERNEL, GRID, BLOCK, SHMEM, STREAM, __VA_ARGS__);                                  \
  } while (0)

__host__ __device__ inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }   // a >= 0, b > 0

// The sizes and pointers of ONE ring table at an entry point (`side`: "a" or "b" where the call takes two, else null): every count
// in [0, 2^31), no null array that a count says is read; hole flags and boxes are asked for with `with_holes_and_boxes` alone.
inline int check_ring_table(gr_ctx *c, const char *name, const char *side, const int64_t *rv, int64_t n_rv, const int64_t *roff,
                            const int32_t *rpoly, const int32_t *rhole, int64_t R, const int64_t *pbox, int64_t P, bool with_holes_and_boxes) {
  const char *of_table = side ? " of table " : "", *in_table = side ? " in table " : "";
  if (n_rv < 0 || R < 0 || P < 0 || n_rv > 0x7FFFFFFFll || R > 0x7FFFFFFFll || P > 0x7FFFFFFFll)
    return fail(c, GR_EINVAL, "%s: a size%s%s is negative or not below 2^31", name, of_table, side ? side : "");
  if (!roff || (n_rv > 0 && !rv) || (R > 0 && !rpoly) || (with_holes_and_boxes && ((R > 0 && !rhole) || (P > 0 && !pbox))))
    return fail(c, GR_EINVAL, "%s: null arrays%s%s", name, in_table, side ? side : "");
  return GR_OK;
}

// B1: a window of a cell grid -- not empty, its offsets inside (-2^23, 2^23), its far edges at or below 2^23.
inline int check_window(gr_ctx *c, const char *name, int32_t col_off, int32_t row_off, int32_t width, int32_t height) {
  const int32_t lim = 1 << 23;
  if (width < 1 || height < 1 || col_off <= -lim || row_off <= -lim || col_off >= lim || row_off >= lim ||
      (int64_t)col_off + width > lim || (int64_t)row_off + height > lim)
    return fail(c, GR_EINVAL, "%s: window %d x %d at (%d, %d) is empty or leaves (-2^23, 2^23]", name, width, height, col_off, row_off);
  return GR_OK;
}

// Before scratch is freed: wait for the work that can still use it -- the stream of the context's last call and its side
// stream -- not for the whole device (other contexts, the caller's own streams keep running).
inline void quiesce(gr_ctx *c) {
  for (hipStream_t st : c->used_streams) (void)hipStreamSynchronize(st);
  c->used_streams.clear();
  if (c->side) (void)hipStreamSynchronize(c->side);
}

inline void note_stream(gr_ctx *c, hipStream_t s) {
  for (hipStream_t st : c->used_streams)
    if (st == s) return;
  c->used_streams.push_back(s);
}

struct DeviceMem {   // the allocator policy of device_buffer.hpp for a context: the library's ONE allocation and ONE free
  gr_ctx *c;
  void *alloc(size_t bytes, const char *what) {
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { p = nullptr; (void)fail(c, GR_ENOMEM, "%s scratch allocation failed (%lld bytes)", what, (long long)bytes); }
    return p;
  }
  void free(void *p) { (void)hipFree(p); }
  void quiesce() { grimpl::quiesce(c); }
};

// The only way to stage scratch: `bytes` of `sc` for work that the caller enqueues on `s`.  The block's last user may have been
// another stream of the context and may have returned without waiting (gr_resize_image_f64, gr_mesh_upload, ...): it is waited
// for here, so calls of one context on different streams use the block in turn.  On one stream this adds nothing.
inline int stage_acquire(gr_ctx *c, Scratch &sc, size_t bytes, hipStream_t s, const char *what) {
  if (sc.ptr && sc.last != s) (void)hipStreamSynchronize(sc.last);   // (a block that was used: the null stream is a stream too)
  DeviceMem mem{c};
  if (const int rc = reserve(mem, sc, (int64_t)bytes, what)) return rc;
  note_stream(c, s);
  sc.last = s;
  // test hook (GR_DBG_POISON_STAGE, GR_DBG_POISON_STAGE_7F; 0xFF wins when both are set): the WHOLE block, not only `bytes` of it,
  // starts as garbage on the call's stream -- every word a stage reads is one it wrote itself, or the results show it
  if (c->opt_dbg & (GR_DBG_POISON_STAGE | GR_DBG_POISON_STAGE_7F)) {
    const int byte = (c->opt_dbg & GR_DBG_POISON_STAGE) ? 0xFF : 0x7F;
    if (sc.ptr && sc.have > 0 && hipMemsetAsync(sc.ptr, byte, (size_t)sc.have, s) != hipSuccess)
      return fail(c, GR_EHIP, "%s scratch: the poison memset failed", what);
  }
  return GR_OK;
}

// a step that answers GR_OK or has left its message in the context (cub_steps.hpp, compact_dev.hpp)
#define GR_TRY(step) do { const int rc_ = (step); if (rc_ != GR_OK) return rc_; } while (0)

// (the zeroes go out on the CALL's stream: a plain hipMemset runs on the null stream, which a non-blocking stream -- torch's
// side streams, one per device thread of a devices=[...] mesh -- does not wait for: the first view's winners could be wiped
// after they were written; found by tests/test_devices_kwarg.py with three contexts on one GPU)
inline int reserve_winner(gr_ctx *c, int64_t n, hipStream_t s) {
  DeviceMem mem{c};
  bool fresh;
  const int rc = reserve(mem, c->winner, n, "winner", &fresh);
  if (rc != GR_OK || !fresh || hipMemsetAsync(c->winner, 0, sizeof(uint32_t) * (size_t)n, s) == hipSuccess) return rc;
  release(mem, c->winner);   // (never a block that was not zeroed)
  return fail(c, GR_EHIP, "winner memset failed");
}

inline BinArgs make_args(gr_ctx *c, int h, int w, int slot0) {
  BinArgs a;
  a.ctrl_stride = c->ctrl_stride; a.rec_stride = c->rec_stride; a.ent_cap = c->ent_cap; a.F = c->F;
  a.work_stride = c->work_stride;
  a.ctrl = c->ctrl + slot0 * a.ctrl_stride; a.rec = c->rec + slot0 * a.rec_stride;
  a.comp = c->comp + slot0 * a.ent_cap * GR_ENT_Q; a.work = c->work + slot0 * a.work_stride;
  a.nrow8 = c->nrow8 + slot0 * a.ent_cap;
  a.stats = c->stats; a.blk = c->blk; a.soup = c->soup; a.orig = c->orig; a.bvert = c->bvert; a.bidx = c->bidx;
  a.touched = c->cur_touched; a.tw = c->cur_tw;
  a.clip = c->clip + slot0 * c->F;
  a.twl = GR_TILE_LOG2; a.thl = c->opt_thl;
  a.TX = (w + (1 << a.twl) - 1) >> a.twl; a.TY = (h + (1 << a.thl) - 1) >> a.thl; a.T = a.TX * a.TY; a.Tcap = c->Tcap; a.clg = c->clg;
  a.h = h; a.w = w; a.dbg = c->opt_dbg; a.var = c->opt_var; a.gl_order = c->opt_gl_order;
  a.cap_tile = c->cur_cap;          // the call's snapshot: every launch group, bin pass and tile pass alike
  a.ent40 = c->cur_ent40 ? 1 : 0;
  a.micro = c->cur_micro ? 1 : 0;   // resolved once per call (resolve_binning)
  a.count_micro = c->cur_count_micro ? 1 : 0;
  a.group = 0;
#ifdef GR_STAMPS
  a.stamps = c->stamps;
#endif
  return a;
}

inline int check_common(gr_ctx *c, int n_views, int h, int w) {
  if (!c) return GR_EINVAL;
  if (n_views < 0 || h <= 0 || w <= 0 || h > GR_MAX_DIM || w > GR_MAX_DIM)
    return fail(c, GR_EINVAL, "bad shape n_views=%d h=%d w=%d (limit %d)", n_views, h, w, GR_MAX_DIM);
  return GR_OK;
}

// launchers that live in other translation units
int bin_batch(gr_ctx *c, const float *cams, int nb, int h, int w, int slot0, int group, hipStream_t s);   // binning.hip
int tile_batch(gr_ctx *c, int nb, int h, int w, int slot0, RasterOut out, hipStream_t s);                 // raster_tile.hip
int bin_stats_deferred(gr_ctx *c, hipStream_t s);                                                         // binning.hip
int sum_visits(gr_ctx *c, hipStream_t s);                                                                 // binning.hip
void launch_vote_labels(gr_ctx *c, hipStream_t vs, uint32_t *win, const uint8_t *labels, int nb, int64_t F, int64_t P, int C,
                        uint32_t *votes, uint32_t *counts, int group, const uint32_t *touched, int tw);  // project.hip

}  // namespace grimpl
