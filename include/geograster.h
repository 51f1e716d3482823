/*
 * include/geograster.h -- C ABI of libgeograster (MI355X / gfx950 HIP implementation of geograypher's
 * image<->mesh projection hot path).
 *
 * This is the drop-in boundary.  The reference (pure Python) has no FFI for this path; the seam it offers is the
 * subclass-override plugin `pix2face` (geograypher/meshes/derived_meshes.py:642-650, precedent
 * TexturedPhotogrammetryMeshPyTorch3dRendering) plus the numpy stages that consume its output.  Each entry point
 * below names the reference lines it replaces; INTEGRATION.md shows the ctypes stub a reference maintainer adds.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer (hipMalloc / torch tensor .data_ptr()) unless its name ends in _h.
 *  - The caller allocates and owns all inputs and outputs.  The library allocates only per-context scratch
 *    (bin lists, per-face winners, one arena for the stage calls), grown lazily, freed by gr_ctx_destroy.
 *  - All work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the default stream) and is
 *    asynchronous.  No hidden synchronisation except: gr_ctx_create and gr_ctx_destroy (the whole device), gr_mesh_upload
 *    (index validation), scratch growth (hipMalloc/hipFree when a larger batch, image or mesh is first seen), the first
 *    launch group of a raster call on a (mesh, image size) the context has learned nothing about (its counts are read back
 *    once, GR_VAR_NO_LOOK switches that off), and the calls whose comment says "Synchronises `stream`": they read a count or
 *    a flag back, or return with their scratch free.  Such a call waits for `stream` alone, never for the device or for the
 *    null stream (tests/test_stream_contract_gpu.py runs every call with the null stream held).
 *  - Return value: 0 (GR_OK) or a negative GR_E* code; text via gr_last_error().  No C++ exception crosses the ABI.
 *  - A context belongs to one (device, host thread); distinct contexts are independent.
 *  - Calls of one context on different streams may be issued back to back: the stage calls share one scratch arena per
 *    context ("context scratch" below), and the library orders their use of it -- a call that finds the arena's last user
 *    on another stream waits for that stream first.  On one stream nothing is added.  The promise covers the stage arena
 *    ONLY: two raster calls (gr_raster_face_ids, gr_raster_project_labels_u8) of one context on two streams share the bin
 *    lists, the per-face winners and the statistics block, and nothing orders them -- the caller does, or uses a context
 *    per stream.
 */
#ifndef GEOGRASTER_H
#define GEOGRASTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GR_VERSION 126 /* 0.2.6: gr_warp_f64 order 1 reads `fill` at an infinite sampling coordinate (it wrote NaN); 0.2.5: gr_argmax_nonzero (float32 / float64 rows, numpy's pairwise row sum), F = 0 is an empty result; 0.2.4: gr_raster_overflow_causes; 0.2.3: the first launch group of an unknown (mesh, image size) is looked at before its tile kernel runs (gr_raster_stats.rebinned_groups); 0.2.2: micro lists (a fifth field in the learned-table file); 0.2.1: gr_learned_cache_clear; 0.2.0: gr_resize_image_f64, gr_learned_cache_file, mesh-signature keyed learned table */

enum {
  GR_OK = 0,
  GR_EINVAL = -1,    /* bad argument / shape                                                  */
  GR_EHIP = -2,      /* HIP runtime error (text in gr_last_error)                             */
  GR_ENOMEM = -3,    /* scratch allocation failed                                             */
  GR_ENOMESH = -4,   /* no mesh uploaded                                                      */
  GR_EINDEX = -5,    /* face index outside [0, V) found by gr_mesh_upload                     */
  GR_EOVERFLOW = -6, /* gr_raster_status: a tile list outgrew its slots, or a face did not fit
                        the 40-byte entry form -- the library has noted what the image needs;
                        repeat the call from view `views_done` on                              */
  GR_ENODEVICE = -7  /* no usable gfx950 device                                               */
};

/* flags for the projection / aggregation entry points */
enum {
  GR_FLAG_NEG1_IS_LAST_FACE = 1, /* reproduce meshes.py:1998-2001: pix2face == -1 writes the LAST face */
  GR_FLAG_DEFER_CHECK = 2        /* gr_project_index_pairs: do not synchronise; key_count then points to TWO 64-bit words,
                                    {pair count, error flag}: a value outside [0, n_classes) makes key_count[1] non-zero
                                    instead of failing the call (the caller reads both words once, at the end)          */
};

/* camera record: 16 floats per view, see DESIGN.md R0.
 *  [0..8]  R   cam_to_world rotation, row-major       (cameras.py:84, 446-477)
 *  [9..11] t   camera position (chunk-local frame)
 *  [12]    f_eff   focal length in pixels of the RENDERED image  = f * h / image_height
 *  [13,14] cxp,cyp principal point in pixels of the rendered image (pyvista path: w/2, h/2)
 *  [15]    near    faces with any vertex at camera depth <= near are discarded                 */
#define GR_CAM_FLOATS 16

typedef struct gr_ctx gr_ctx;

/* per-stage device times of the most recent profiled call, milliseconds (see gr_set_profiling) */
typedef struct gr_stage_times {
  float setup_ms;   /* k_setup_cull : transform + cull + record + tile counts      */
  float scan_ms;    /* k_scan_tiles                                                */
  float fill_ms;    /* k_fill_compile                                              */
  float raster_ms;  /* k_raster_tile (the dominant kernel)                         */
  float project_ms; /* k_winner_* : last-writer-wins pixel -> face                 */
  float vote_ms;    /* k_vote_*   : per-face accumulate                            */
  float gather_ms;  /* k_gather_texture                                            */
  int32_t raster_launches;
  int32_t views;
} gr_stage_times;

typedef struct gr_raster_stats {
  int64_t records;      /* faces that survived culling, summed over the views of the last call */
  int64_t entries;      /* (face, tile) pairs, summed over views                               */
  int64_t max_entries;  /* largest per-view entry count seen (capacity needed)                 */
  int64_t entry_cap;    /* current per-view capacity                                           */
  int32_t overflow;     /* != 0: some view exceeded entry_cap, output incomplete               */
  int32_t views_done;   /* leading views of the last call whose outputs / votes are complete    */
  int64_t blocks;       /* 64-face blocks that passed the per-view frustum cull, summed over views (single-pass binning):
                           what a culled pass has to read of the mesh is blocks x 64 x 36 B + 16 B per block tested   */
  int64_t chunk_visits; /* fused aggregation: (view, group of 64 consecutive caller face ids) pairs the vote passes visited, summed over
                           the call (a group is visited in the views whose tile pass produced a winner in it; each visit reads and
                           resets 64 winners: 64 x 8 B of k_vote_labels' algorithmic bytes)                               */
  int64_t rebinned_groups; /* times the last call binned its FIRST launch group again: a call for a mesh and image size the
                           library has learned nothing about reads that group's counts before its tile kernel runs (one host
                           round trip, once per mesh and image size) and, if a tile outgrew its slots, a face needs 48-byte
                           entries or micro lists pay, starts over with what it learned -- instead of a GR_EOVERFLOW retry  */
} gr_raster_stats;

int gr_version(void);

/* context -------------------------------------------------------------------------------------------------- */
int gr_ctx_create(int device, gr_ctx **out);
int gr_ctx_destroy(gr_ctx *ctx);
const char *gr_last_error(const gr_ctx *ctx);

/* Turn per-stage hipEvent timing on (1) or off (0).  When on, HIP events on `stream` delimit every kernel group;
 * gr_get_stage_times synchronises on them.  The stages of a raster call (set-up, tile kernel; scan / fill of the exact
 * binning) are delimited by stop events attached to the kernel launches themselves (hipExtLaunchKernelGGL): a stage runs
 * from the end of the kernel in front of it to the end of its last kernel, the launch gap in front of a kernel included --
 * timing costs the call 0.2 % this way, where events recorded between the kernels cost it 1.65 % (4.3 % on small images). */
int gr_set_profiling(gr_ctx *ctx, int enabled);

/* Tuning knobs (results never depend on them -- GR_OPT_VERTEX_ORDER excepted, which selects between two documented rule-sets --;
 * tests run every setting against the oracle). */
enum {
  GR_OPT_TILE_H_LOG2 = 2,   /* tile height: 5 (64x32, default) or 6 (64x64)                                  */
  GR_OPT_BATCH = 3,         /* views per launch group, 1..64 (default 64)                                    */
  GR_OPT_DIRECT_CAP = 6,    /* single-pass binning: entry slots per tile (default 512); 0 = always bin exactly
                               (count, scan, fill).  A call for a mesh and image size nothing is known about reads the
                               counts of its FIRST launch group before that group's tile kernel runs and starts over by
                               itself if they say so (gr_raster_stats.rebinned_groups); in any later group, or any later
                               call with more crowded views, a tile that outgrows its slots is reported by
                               gr_raster_status (GR_EOVERFLOW); the retry uses segments of the size that image needs
                               (remembered per mesh size and tile count, in the context and -- unless this option was
                               set by hand -- process-wide, so that another context for the same mesh and image size
                               starts with segments that fit) or, beyond 65536 slots, or 24 GB of entry memory for ONE
                               view, bins exactly.  Setting the option forgets what the context learned          */
  GR_OPT_VARIANT = 7,       /* mode bits, the OR of GR_VAR_* below (results identical; the parity tests run every one against the
                               oracle) */
  GR_OPT_SHARE_LEARNED = 8, /* 1 (default): consult and feed the process-wide table of learned slots per tile / entry forms
                               (and its file, gr_learned_cache_file); 0: this context learns for itself only.  Setting
                               GR_OPT_DIRECT_CAP by hand switches it off; this option switches it back on            */
  GR_OPT_DIRECT_BUDGET_MB = 9, /* entry memory one launch group may take, MiB (default 24576).  Scratch of the single-pass
                               binning = views per launch group (<= 64) x tiles x slots per tile x 48 B -- 9.3 GB for 64
                               views of 4000 x 3000 at the default 512 slots --; a launch group shrinks until it fits, and
                               an image whose learned slots would not fit even ONE view bins exactly instead (remembered
                               per mesh and image size like the slots themselves; other image sizes are not affected)   */
  GR_OPT_VERTEX_ORDER = 10, /* 0 (default): rule R1 of DESIGN.md -- s = c + (f q) (1 / q_z), X = floor(256 s + 0.5).  1: the same
                               perspective divide, viewport transform and snap in the ORDER OF OPERATIONS of an OpenGL pipeline, as
                               Mesa's llvmpipe -- the software GL of the reference's Dockerfile:6-13 -- executes them behind the camera
                               transform: clip = P q with P = (2 f / w, -2 f / h), ndc = clip * (1 / q_z), window = fma(ndc, size / 2,
                               size / 2), fixed = rint(256 (window - 0.5)), rows bottom-up.  The two orders put 3-12 % of the vertices
                               of a view on neighbouring 1/256 px steps, which decides 0.004 % of its pixels (95 % of the pixels on
                               which R1 and llvmpipe differ; the rest are faces llvmpipe clips at the image border:
                               profiles/r06_gl_residue.txt).  With 1 the library differs from llvmpipe on 14 of the 12 000 000 pixels
                               of a C2 view.  The principal point must be the window centre (cxp = w / 2, cyp = h / 2: the pyvista
                               camera of cameras.py:446-477), and the guard planes of the clipping (R7) bound the window coordinate,
                               |window| <= 16383, rows bottom-up, instead of R1's s; results depend on this option by design -- the oracle has the same
                               switch (oracle_raster.c R1-GL) and the parity tests run both                              */
  GR_OPT_DEBUG_LDS = 98,    /* extra dynamic LDS bytes per tile workgroup: lowers occupancy (timing experiments)     */
  GR_OPT_DEBUG = 99         /* test hooks, the OR of GR_DBG_* below (results stay right)                             */
};
/* bits of GR_OPT_VARIANT */
enum {
  GR_VAR_ONE_TILE = 1,        /* one tile per workgroup of the tile kernel (default: chains of four consecutive tiles in large
                                 launches of light tiles, rolling chains of 16 for the fused kernel)                       */
  GR_VAR_VOTES_INLINE = 4,    /* fused votes on the caller's stream (default: a side stream beside the next group's binning;
                                 the profiling scripts use it: rocprofv3 counter passes do not survive the side stream)    */
  GR_VAR_CHAINS = 16,         /* chains whatever the size of the launch (tests: small images through the chain kernels)    */
  GR_VAR_ENT48 = 128,         /* 48-byte entries always (default: 40-byte entries; images with faces of 93 pixels and more
                                 fall back to 48 bytes, remembered like the slots per tile)                                */
  GR_VAR_GENERAL_IDS = 512,   /* the general ids kernel (depth output, any width) also where the plain one would run       */
  GR_VAR_MICRO_NEVER = 4096,  /* micro lists never, ...                                                                    */
  GR_VAR_MICRO_ALWAYS = 8192, /* ... always (default: a call whose views show mostly faces of at most 4 x 4 pixels -- a mesh
                                 rendered at a fraction of its photos' resolution -- teaches the library to keep, for that
                                 mesh and image size, a second list per tile for such faces, which the tile kernel
                                 point-samples one face per lane)                                                          */
  GR_VAR_NO_LOOK = 16384,     /* no look at the first launch group's counts (every overflow goes through gr_raster_status) */
  GR_VAR_PACKED_COUNTERS = 131072 /* tile counters packed side by side whatever the image size (default: images of at most
                                 1024 tiles keep one counter per 128-byte line -- atomics on one line are served one after
                                 the other)                                                                                */
};
/* bits of GR_OPT_DEBUG */
enum {
  GR_DBG_POISON_SLOTS = 512,  /* entry slots and row counts are poisoned with 0xFF before every launch group is binned
                                 (tests/test_overflow_protocol.py)                                                         */
  GR_DBG_POISON_RAYS = 1024,  /* gr_ray_pairs poisons its scratch with 0xFF at the start of every call                      */
  GR_DBG_RAY_GRID_7 = 2048,   /* gr_ray_pairs' grid is capped at 7 workgroups, which stride over all tiles as a launch beyond
                                 2^20 tiles does (tests/test_ray_pairs.py)                                                 */
  GR_DBG_POISON_STAGE = 4096, /* every stage call fills the whole block of stage scratch it was given with 0xFF first      */
  GR_DBG_POISON_STAGE_7F = 8192 /* ... with 0x7F (0xFF wins when both are set; tests/test_stage_poison_gpu.py)            */
};
int gr_set_option(gr_ctx *ctx, int key, int value);

/* Persist what overflowed calls taught the library -- slots per tile and entry form per (mesh signature, tile count); the
 * signature is the face count, vertex count and vertex bounds of the upload -- in a small text file, so that a NEW process
 * starts with segments that fit (no GR_EOVERFLOW retry on its first call).  Reads `path_h` now (a missing file is fine) and
 * rewrites it whenever something new is learned (atomic rename).  Process-wide; NULL or "" switches persistence off.
 * The reference keeps its caches under CACHE_FOLDER (constants.py:18; pix2face's cache_folder argument, meshes.py:1683):
 * the Python binding points this at CACHE_FOLDER/geograster_learned.txt. */
int gr_learned_cache_file(const char *path_h);
/* Forget everything the PROCESS-WIDE table holds (contexts keep what they learned themselves; the file is not touched and the
 * file name stays set).  For callers that need a cold start -- a benchmark's "first process that ever sees the scene" leg, a
 * hermetic test -- after which gr_learned_cache_file(path) reads a file's entries into the empty table. */
int gr_learned_cache_clear(void);
int gr_get_stage_times(gr_ctx *ctx, gr_stage_times *out_h);

/* mesh -- replaces the per-view mesh + colour upload of meshes.py:1776-1817 (plotter.clear/add_mesh) and the
 * coordinate hand-over of meshes.py:1641-1676.  verts: V x 3 fp32 in the cameras' local frame; faces: F x 3 int32.
 * Borrowed: the caller keeps both alive until the next upload or gr_ctx_destroy.  Validates 0 <= index < V
 * (GR_EINDEX).  The library keeps its own de-indexed copy of the faces, ordered along a Morton curve of their
 * centroids; every id it reports is an index into the caller's `faces`, whatever their order.  Synchronises `stream`.
 * After GR_EINVAL or GR_EINDEX the previous mesh stays in use; an upload that fails later (GR_ENOMEM, GR_EHIP) leaves the context
 * WITHOUT a mesh: raster and project calls answer GR_ENOMESH until an upload succeeds. */
int gr_mesh_upload(gr_ctx *ctx, const float *verts, const int32_t *faces, int64_t V, int64_t F, void *stream);
/* For tests: what the last upload left behind, copied device to device into the caller's buffers (a null pointer skips that
 * product): orig [F] soup position -> caller's face; blk4 [ceil(F / 64)][4] the bounding sphere (centre, radius) of each block
 * of 64 soup faces; bvert [ceil(F / 64)][192][3] the distinct vertices of each block in order of first use (rows behind a
 * block's count are unspecified); bidx [F] a face's three positions in its block's list, 8 bits each, and the block's count - 1
 * in the top byte.  mesh_sig_h: the mesh signature, to a host word.  GR_ENOMESH without a mesh.  Synchronises `stream`. */
int gr_debug_read_upload(gr_ctx *ctx, int32_t *orig, float *blk4, float *bvert, uint32_t *bidx, uint64_t *mesh_sig_h, void *stream);
/* For tests: `n` bytes at `offset` of the context's stage scratch -- block 0: the stage arena, block 1: the second block of the
 * outline calls -- copied device to device into `out` (null, or n = 0: the size alone); size_h: the bytes the block holds now, to
 * a host word (0: never used).  GR_EINVAL for another block or a range outside it.  Synchronises `stream`. */
int gr_debug_read_stage(gr_ctx *ctx, int block, int64_t offset, int64_t n, uint8_t *out, int64_t *size_h, void *stream);

/* pix2face -- replaces meshes.py:1776-1836 (encode ids, VTK render, decode, background mask) for n_views
 * cameras of equal image size.  ids: n_views x h x w int32, background -1.  depth (may be NULL): n_views x h x w
 * fp32 camera-space depth of the visible face, +inf for background.  Rule-set: DESIGN.md R0-R7. */
int gr_raster_face_ids(gr_ctx *ctx, const float *cams, int n_views, int h, int w, int32_t *ids, float *depth,
                       void *stream);
/* Outcome of the last raster call (synchronises its stream; a call of one launch group that is not fused leaves its view totals
 * to be added up here, by one small kernel on that stream, instead of paying for them in every call).  GR_EOVERFLOW: the single-pass binning could not finish a launch
 * group -- a tile received more entries than its segment holds, or a face is too large (93 px and more) for the 40-byte
 * entries the call started with.  The first `views_done` views are final; the context (and the process-wide table, see
 * GR_OPT_DIRECT_CAP) now knows the segment size / entry form this mesh and image size need: call again for the remaining
 * views.  At most one such retry per cause for a given (mesh, image size). */
int gr_raster_status(gr_ctx *ctx, gr_raster_stats *out_h);
/* Why the last raster call overflowed, as far as gr_raster_status (and the look at a first launch group) read it: the OR of
 * GR_CAUSE_*; 0 after a call without overflow.  Host only: no device work, no synchronisation. */
enum {
  GR_CAUSE_LIST_OUTGREW = 1, /* a tile list outgrew its slots where it was stored (single-pass: compiled entries beyond the slots
                                per tile, micro records beyond 1.25 x the slots per tile; exact binning: a view's entry or record
                                list)                                                                                       */
  GR_CAUSE_SHORT_MISS = 2,   /* a face did not fit the 40-byte entry form                                                    */
  GR_CAUSE_LISTS_MET = 4     /* with micro lists: a tile's two lists, each within its own bound, together outgrew the tile's
                                segment (they met)                                                                          */
};
int gr_raster_overflow_causes(const gr_ctx *ctx);

/* render_flat gather -- replaces meshes.py:1921-1937: out[p,:] = face_tex[ids[p],:] where ids[p] != -1 else NaN.
 * ids: n_pix int32; face_tex: F x C f64; out: n_pix x C f64. */
int gr_gather_texture_f64(gr_ctx *ctx, const int32_t *ids, int64_t n_pix, const double *face_tex, int64_t F, int C,
                          double *out, void *stream);

/* The five gr_project_* calls below share their order of checks -- context and shape (GR_EINVAL), an uploaded mesh
 * (GR_ENOMESH), then the call's own arguments (GR_EINVAL); n_views == 0 is GR_OK behind all of them -- and their protocol:
 * the views are taken in launch groups of up to 64, per group one winner pass over the id images (per view the LAST pixel,
 * row-major, of each face wins), then the call's own pass over the winners. */

/* project_images + aggregate step for index labels -- replaces meshes.py:1987-2002 and 2057-2067 for the
 * one-hot label images of cameras/segmentor.py:33-42 + predictors/segmentor.py:37-69.
 * ids: n_views x h x w int32; labels: n_views x h x w uint8 class indices (>= C: all-zero one-hot row, still an
 * observation).  Per view the LAST pixel (row-major) of each face wins; votes[f*C + label] += 1 and counts[f] += 1
 * are ACCUMULATED into the caller's buffers (zero them before the first call). */
int gr_project_labels_u8(gr_ctx *ctx, const int32_t *ids, const uint8_t *labels, int n_views, int h, int w, int C,
                         uint32_t *votes, uint32_t *counts, int flags, void *stream);

/* same for continuous images (cameras.py:154-177 float images): img n_views x h x w x C f64 (NaN allowed).
 * sums[f*C+c] = nz(sums[f*C+c]) + nz(value) view by view, nz(NaN) = 0 -- np.nansum([summed, projection], axis=0) of
 * meshes.py:2060-2062 to the letter: a running sum that went NaN (+inf met -inf) counts as 0 at the next view of the call
 * or of the next call on the same buffers, whether that view shows the face or not; counts[f] += any(isfinite(row))
 * (2064-2067).
 * CONTRACT WHEN VIEWS ARE SHARDED over processes (geograypher_amd/distributed.py: rank r accumulates views r, r + N, ... into
 * its own buffers, the buffers are added with one all-reduce): counts are exact for any N; sums of FINITE inputs equal the
 * serial result within 1e-12 relative (addition order); for inputs with +-inf the recurrence above runs per rank over that
 * rank's views and the per-rank sums are then added, so a face that met +inf and -inf in views of DIFFERENT ranks ends NaN
 * where the serial reference -- which drops the NaN at the following view -- ends finite
 * (tests/test_distributed_gloo.py::test_float_aggregation_contract_for_non_finite_inputs_at_world_two). */
int gr_project_values_f64(gr_ctx *ctx, const int32_t *ids, const double *img, int n_views, int h, int w, int C,
                          double *sums, uint32_t *counts, int flags, void *stream);

/* project_images for ONE view, materialised like the reference generator yields it (meshes.py:1991-2002):
 * tex: F x C f64, NaN for faces no pixel maps to.  img: h x w x C f64. */
int gr_project_view_f64(gr_ctx *ctx, const int32_t *ids, const double *img, int h, int w, int C, double *tex,
                        int flags, void *stream);

/* fused pix2face + project_labels (ids never leave the chip unless ids_or_null != NULL): the
 * aggregate_projected_images fast path, meshes.py:2004-2084 over n_views cameras.  The tile rasterizer's epilogue feeds
 * the per-face winners straight from its LDS tile.  If gr_raster_status afterwards reports GR_EOVERFLOW, the votes of the
 * first gr_raster_stats.views_done views HAVE been folded into votes/counts and those of the remaining views have
 * not (the launch group that overflowed and every later one are skipped on the device): call again with the camera
 * records and label images from view `views_done` on.  No rollback of votes/counts is needed. */
int gr_raster_project_labels_u8(gr_ctx *ctx, const float *cams, const uint8_t *labels, int n_views, int h, int w,
                                int C, uint32_t *votes, uint32_t *counts, int32_t *ids_or_null, int flags,
                                void *stream);

/* save_renders epilogue (row f2) -- replaces meshes.py:1921-1937 + 2325-2337 in one pass: out[p,c] = uint8(tex[ids[p],c]),
 * with `null_value` where the pixel has no face or the value is < 0, > 255 or not finite.  out: n_pix x C uint8. */
int gr_gather_texture_u8(gr_ctx *ctx, const int32_t *ids, int64_t n_pix, const double *face_tex, int64_t F, int C,
                         int null_value, uint8_t *out, void *stream);

/* sparse index aggregation (row f3) -- replaces the loop body of TexturedPhotogrammetryMeshIndexPredictions
 * .aggregate_projected_images (derived_meshes.py:470-520) for single-channel images whose finite values are class
 * indices: per view the last pixel of each face wins (as project_images); a finite value v adds one observation:
 * counts[f] += 1 and the pair key f * n_classes + int(v) is appended to keys[*key_count ...] (device counter, capacity
 * key_cap; pairs beyond it are dropped but still counted in *key_count).  Calls APPEND: the caller zeroes *key_count and may
 * collect the pairs of many calls in one buffer before counting them once (gr_count_pairs).  Synchronises `stream` and
 * returns GR_EINDEX when a value is outside [0, n_classes) -- unless GR_FLAG_DEFER_CHECK is set: then the call only enqueues
 * work, key_count must point to two 64-bit words (both zeroed by the caller) and such a value makes key_count[1] non-zero.
 * A value v is a class index when -1 < v < n_classes (int(v) truncates); n_classes above 2^53 is GR_EINVAL. */
int gr_project_index_pairs(gr_ctx *ctx, const int32_t *ids, const double *img, int n_views, int h, int w,
                           int64_t n_classes, uint32_t *counts, uint64_t *keys, int64_t key_cap, uint64_t *key_count,
                           int flags, void *stream);
/* gr_project_index_pairs with the label image given as rectangles (detections, image IDs): same winners, flags, pair
 * keys, counts and class check, but the winner pixel (p / w, p % w) of a face takes the class of the LAST rectangle of its
 * view's list that contains it, and a pixel no rectangle contains is no observation.  No per-pixel label image exists.
 * rects: int32 rows {imin, jmin, imax, jmax, class} (half-open, in paint order; device memory, may be NULL when no view
 * has a rectangle); rect_offsets: n_views + 1 non-decreasing device int32, view v's rows are
 * [rect_offsets[v], rect_offsets[v + 1]) -- the caller guarantees they index rects.  Added without a GR_VERSION bump. */
int gr_project_rect_pairs(gr_ctx *ctx, const int32_t *ids, const int32_t *rects, const int32_t *rect_offsets,
                          int n_views, int h, int w, int64_t n_classes, uint32_t *counts, uint64_t *keys,
                          int64_t key_cap, uint64_t *key_count, int flags, void *stream);
/* gr_project_index_pairs for views whose label image is the MULTI-HOT mask of polygon rings (region detections): same
 * winners, flags, counts protocol and class check, but the winner pixel (p / w, p % w) of a face is one observation of EVERY
 * class that has at least one ring of the view containing it: one pair key f * n_classes + class per (face, class, view),
 * however many rings of the class contain the pixel, and counts[f] += 1 when any ring does.  Containment is
 * skimage.draw.polygon's rule in double (boundary pixels inside; DESIGN.md "Polygon detections").  No mask image exists.
 * boxes: int32 rows {imin, jmin, imax, jmax, class}, ring r's clipped candidate box, half-open, SORTED BY CLASS within each
 * view (an unsorted table emits a pair once per class run); vert_offsets: rings + 1 non-decreasing int32, ring r's vertices
 * are verts[vert_offsets[r] .. vert_offsets[r + 1]), double (row, col) pairs (a ring without vertices contains nothing);
 * poly_offsets: n_views + 1 non-decreasing int32, view v's rings are [poly_offsets[v], poly_offsets[v + 1]).  All device
 * memory; boxes and verts may be NULL when no view has a ring; the caller guarantees that the offsets index their tables.
 * A view may emit several pairs per face: the caller sizes key_cap (or reads *key_count, which counts dropped pairs too).
 * Added without a GR_VERSION bump. */
int gr_project_polygon_pairs(gr_ctx *ctx, const int32_t *ids, const int32_t *boxes, const int32_t *vert_offsets,
                             const double *verts, const int32_t *poly_offsets, int n_views, int h, int w, int64_t n_classes,
                             uint32_t *counts, uint64_t *keys, int64_t key_cap, uint64_t *key_count, int flags, void *stream);
/* multiplicity of every distinct pair key: radix sort + run-length encode (rocPRIM via hipcub) in context scratch.
 * unique_keys / pair_counts: capacity n.  *n_unique_h (host) receives the number of distinct keys.  Synchronises. */
int gr_count_pairs(gr_ctx *ctx, uint64_t *keys, int64_t n, uint64_t *unique_keys, uint32_t *pair_counts,
                   int64_t *n_unique_h, void *stream);

/* ray-pair graph of the multiview-detection workflow -- replaces the distance stage of calc_graph_weights
 * (utils/numeric.py:428-498: compute_approximate_ray_intersections(clamp=True), numeric.py:39-236, over 5000 x 5000 blocks, the
 * threshold, and the i < j / different-image filter of format_graph_edges, numeric.py:379-425).  starts, ends: n x 3 f64 segment
 * end points; ray_ids: n int32, the image each ray came from; n <= 8 388 608.  An EDGE is a pair i < j with
 * ray_ids[i] != ray_ids[j] whose clamped segment-to-segment distance d satisfies d <= threshold (a NaN d -- a zero-length
 * segment, NaN or infinite coordinates -- never does).  *total_h (HOST) receives the number of edges, whether or not they fit.
 * edge_i, edge_j (int32) and edge_d (f64), capacity edge_cap <= 2^31 - 1 each, receive the edges SORTED by (i, j) (rocPRIM radix
 * sort of the 64-bit key i << 32 | j), so the result does not depend on wave scheduling.  total > edge_cap: GR_EOVERFLOW and
 * the edge buffers hold NOTHING (they are not written); call again with edge_cap >= *total_h.  edge_cap == 0 (the buffers may
 * be NULL): the count alone.  The min_dist floor, the transform and the 1 / d weight of the reference stay on the host.
 * Uses context scratch (64 B per ray, 24 B per edge slot + the sort's) and synchronises `stream` twice: to read the count, and
 * again behind the sort, its last use of the scratch -- on return the edges are complete and the scratch is free, so calls on
 * different streams of one context follow each other.  Added without a GR_VERSION bump. */
int gr_ray_pairs(gr_ctx *ctx, const double *starts, const double *ends, const int32_t *ray_ids, int64_t n, double threshold,
                 int32_t *edge_i, int32_t *edge_j, double *edge_d, int64_t edge_cap, int64_t *total_h, void *stream);
/* The tile (row <= col) that has index `tile` in gr_ray_pairs' 1-D order of the upper triangle (one workgroup each, strided beyond
 * 2^20 tiles), for tiles_per_side (<= 32768) tiles of 256 rays a
 * side: the kernel's own decode of the row-major upper triangle, exposed so that it can be checked on the host.  No device work. */
int gr_ray_pairs_tile(int64_t tile, int64_t tiles_per_side, int64_t *row_h, int64_t *col_h);
/* ray / boundary-surface intersection of clip_line_segments (utils/geometric.py:210-222: pyvista's multi_ray_trace with
 * first_point=True, an Embree BVH) for a SMALL mesh, by brute force: origins, directions n x 3 f64; points V x 3 f64; faces
 * F x 3 int32 (a face with an index outside [0, V) is never hit), F <= 65536 -- more is GR_EINVAL: this is for a coarse covering
 * surface, not the photogrammetry mesh.  Double-sided Moller-Trumbore in f64, the nearest hit with t >= 0 along the infinite
 * ray.  hit: n int32 (1 / 0); t: n f64; hit_points: n x 3 f64 = origin + t direction (NaN where hit is 0).  Only enqueues work. */
int gr_rays_clip(gr_ctx *ctx, const double *origins, const double *directions, int64_t n, const double *points, int64_t V,
                 const int32_t *faces, int64_t F, int32_t *hit, double *t, double *hit_points, void *stream);
/* covering meshes -- the two calls behind export_covering_meshes (meshes/meshes.py:2399-2482), whose boundary surfaces
 * gr_rays_clip takes.  Neither needs an uploaded mesh; both only enqueue work.  Both visit rows 0, stride, 2 stride, ... of
 * points (V x 3 f64; stride >= 1: the reference's points[::subsample]); V <= 0 or stride < 1 is GR_EINVAL.  A visited row
 * with a NaN or infinite coordinate takes part in neither call's result.
 * gr_points_bounds replaces the four full-array min / max of meshes.py:2435-2436: bounds6 (6 f64) receives xmin xmax ymin ymax
 * zmin zmax over the visited finite rows (+inf / -inf when there is none), nonfinite (one uint64) the number of visited rows
 * that are not finite.  A reduction per workgroup into context scratch (64 KiB, allocated by the first call), then one
 * combine.  Added without a GR_VERSION bump. */
int gr_points_bounds(gr_ctx *ctx, const double *points, int64_t V, int64_t stride, double *bounds6, uint64_t *nonfinite,
                     void *stream);
/* gr_cover_grid replaces the N^2 masked passes over all points of meshes.py:2453-2469.  x_lo, x_hi, y_lo, y_hi: N f64 each,
 * the cells' bounds as the CALLER computed them (the reference's x_grid -+ cell_w_half, y_grid -+ cell_h_half, so that they are
 * its operands bit for bit); a row belongs to cell (xi, yi), flat index xi * N + yi, iff x_lo[xi] <= x <= x_hi[xi] and
 * y_lo[yi] <= y <= y_hi[yi] -- to one, two or four cells of a regular table, to every column of an axis of zero extent.
 * z_max, z_min (N x N f64): the largest / smallest z among the cell's members, NaN for a cell without any; count (N x N
 * uint32): its members.  All three are written by the call (in between z_max and z_min hold integer keys of the doubles,
 * which unsigned max / min atomics order); the results are exact and do not depend on scheduling, except that a cell whose
 * extreme is a zero may report either sign when both occur.  2 <= N <= 1024, else GR_EINVAL; accumulators in LDS for N <= 56,
 * global atomics above.  No context scratch.  Added without a GR_VERSION bump. */
int gr_cover_grid(gr_ctx *ctx, const double *points, int64_t V, int64_t stride, int N, const double *x_lo, const double *x_hi,
                  const double *y_lo, const double *y_hi, double *z_max, double *z_min, uint32_t *count, void *stream);

/* distortion warp of an image through a cached sampling map (row f1) -- replaces utils/image.py:72-126
 * (flexible_inputs_warp -> skimage.transform.warp, mode "constant") as called by cameras.py:1092-1156 for the face-id
 * image of pix2face (meshes.py:1842-1854).  map_rows/map_cols: h_out x w_out f64, the position to sample in `in` for
 * every output pixel (cameras.py:995-1062).  Nearest neighbour = floor(x + 0.5); samples outside `in` read `fill`.
 * reference_float_roundtrip != 0 reproduces the reference's rescale-to-[0,1]-and-back truncation bit for bit
 * (value_min = min(in.min(), fill), value_range = max(in.max(), fill) - value_min as the reference computes them). */
int gr_warp_nearest_i32(gr_ctx *ctx, const int32_t *in, int h_in, int w_in, const double *map_rows,
                        const double *map_cols, int h_out, int w_out, int32_t fill, int reference_float_roundtrip,
                        double value_min, double value_range, int32_t *out, void *stream);
/* same for float64 images with C interleaved channels; order 0 (nearest) or 1 (bilinear: the four taps at floor and
 * floor + 1, each reading `fill` outside `in` -- scipy's "grid-constant").  In all three kernels a NaN or infinite
 * coordinate reads `fill`. */
int gr_warp_f64(gr_ctx *ctx, const double *in, int h_in, int w_in, int C, const double *map_rows, const double *map_cols,
                int h_out, int w_out, int order, double fill, double *out, void *stream);

/* inverse of the lens model (row f1) -- replaces the host-side inversion of the forward distortion map by
 * scipy.interpolate.griddata on every `inversion_downsample`-th pixel (cameras.py:1045-1062, utils/indexing.py:87-150;
 * minutes at full resolution) with a dense Newton solve on the device: for every pixel (i, j) of the warped image of size
 * h x w (= int(image_height * image_scale) x int(image_width * image_scale)) the fractional pixel (row, col) of the
 * ideal image that the Metashape frame-camera model (derived_cameras.py:163-208) sends there, `fill` where that lies
 * outside the ideal image.  par_h (HOST pointer, 13 doubles): f, cx, cy, image_width, image_height, k1, k2, k3, k4, p1,
 * p2, b1, b2.  The forward map follows cameras.py:1012-1043 (model evaluated at the pixel index at scale 1, at
 * (index + 0.5) / scale otherwise).  map_rows / map_cols: h x w f64, the layout gr_warp_* consume. */
int gr_invert_distortion_f64(gr_ctx *ctx, const double *par_h, int h, int w, double image_scale, int max_iters,
                             double fill, double *map_rows, double *map_cols, void *stream);

/* get_image(image_scale) behind the file read -- replaces cameras.py:154-174: `image / 255.0` for uint8 images, then
 * skimage.transform.resize(image, (int(h * s), int(w * s))) with its defaults (order 1, mode "reflect", anti-aliasing
 * Gaussian sigma = (n_in / n_out - 1) / 2 per axis through scipy.ndimage.gaussian_filter(mode="mirror"), half-pixel-centre
 * sampling) -- called per view by project_images (meshes.py:1988 via cameras.py:866-867).  src: h_in x w_in x C image in its
 * FILE dtype (GR_DTYPE_*: the photo crosses the link as uint8, not as float64); divide_by_255 != 0 (uint8 only): values are
 * divided by 255.0 first, as get_image does; out: h_out x w_out x C f64.  Equal sizes: the conversion alone.  Agrees with
 * scikit-image 0.18.3 and with the >= 0.19 formulation (the pinned 0.21.0) to 1e-12 (tests/test_photo_resize.py).  Uses
 * context scratch (2 x h_out x w_in x C doubles). */
enum { GR_DTYPE_U8 = 0, GR_DTYPE_F32 = 1, GR_DTYPE_F64 = 2 };
int gr_resize_image_f64(gr_ctx *ctx, const void *src, int dtype, int h_in, int w_in, int C, int divide_by_255, int h_out,
                        int w_out, double *out, void *stream);

/* 360-degree photos -- replaces utils/image.py:129-267 (perspective_from_equirectangular: the ray grid, flexible_inputs_warp
 * of image.py:72-126 = skimage.transform.warp over scipy.ndimage.map_coordinates one channel at a time, then
 * downscale_local_mean) as driven per folder by entrypoints/equirectangular_to_cube_mapped.py:45-166.  Resamples ONE
 * perspective view of out_h x out_w pixels from the equirectangular image src (h_in x w_in x C interleaved, in its FILE dtype:
 * GR_DTYPE_U8 or GR_DTYPE_F64; GR_DTYPE_F32 is not built: GR_EINVAL), which stays on the device across the views of a photo.
 * Fused: every output pixel forms its oversample x oversample samples itself -- ray (x[col], -y[row], 1) normalised, rotated
 * by rotation_h (HOST pointer, 9 doubles, row-major: the matrix of rotate_by_roll_pitch_yaw), atan2 / asin to
 * (i, j) = ((0.5 - alt / pi) h_in, (hor / 2 pi + 0.5) w_in) clipped to [0, h_in - 1] x [0, w_in], sampled with column w_in
 * reading column 0 (order 1: bilinear, taps outside read the fill 0 as "grid-constant" does; order 0: floor(x + 0.5)), the
 * reference's value round trip ((v - value_min) / value_range, clip to channel_bounds (device, C x {lo, hi}), back, truncated
 * toward zero for uint8) -- and stores their mean as f64; oversample == 1 stores the sample in the source dtype.  x, y: DEVICE
 * f64 vectors of out_w * oversample and out_h * oversample ray coordinates, computed on the host as image.py:181-196 does.
 * value_range > 0 (an image without variation never reaches the device).  Optional: mask (h_in x (w_in + 1) bytes, zeroed by
 * the caller; every sample stores 1 at (rint(i), rint(j)); image.py:255-265, the fold of column w_in into column 0 is the
 * caller's) and debug_ij (2 x ny x nx f64: the (i, j) of every sample; for tests).  Only enqueues work.  Added without a
 * GR_VERSION bump. */
int gr_equirect_view(gr_ctx *ctx, const void *src, int dtype, int h_in, int w_in, int C, const double *x, const double *y,
                     const double *rotation_h, int out_h, int out_w, int oversample, int order, double value_min,
                     double value_range, const double *channel_bounds, void *out, uint8_t *mask, double *debug_ij,
                     void *stream);

/* finalise -- meshes.py:2069-2082: summed[counts==0] = NaN; average = summed / counts.
 * votes_u32 (F x C) is converted to f64 `summed`; average and summed are F x C f64, counts_f64 is F f64. */
int gr_finalize_votes(gr_ctx *ctx, const uint32_t *votes, const uint32_t *counts, int64_t F, int C, double *average,
                      double *summed, double *counts_f64, void *stream);
int gr_finalize_sums_f64(gr_ctx *ctx, double *sums_inout, const uint32_t *counts, int64_t F, int C, double *average,
                         double *counts_f64, void *stream);

/* find_argmax_nonzero_value -- utils/indexing.py:9-32 on an F x C C-contiguous array of dtype GR_DTYPE_F32 or
 * GR_DTYPE_F64: argmax per row as f64 (the first maximum; the first NaN wins), NaN when the row holds a non-finite value
 * or sums to zero -- summed in the array's own precision and in numpy's pairwise order (np.sum(array, axis=1)), so that
 * the zero test agrees with numpy's bit for bit.  F = 0 is an empty result.  gr_argmax_nonzero_f64 is the f64 form. */
int gr_argmax_nonzero(gr_ctx *ctx, const void *array, int dtype, int64_t F, int C, double *out, void *stream);
int gr_argmax_nonzero_f64(gr_ctx *ctx, const double *array, int64_t F, int C, double *out, void *stream);

/* label_polygons -- replaces the geopandas stage of meshes.py:1141-1306 (one shapely Polygon per face, gpd.sjoin / gpd.overlay,
 * weighted area, groupby) up to the per-(polygon, class) sums; the rule-set is DESIGN.md "Polygon labels".
 * Faces: tri F x 6 int64, the corners x0 y0 x1 y1 x2 y2 SNAPPED to integers (units of 1e-6 m, a common origin subtracted,
 * |value| <= 2^40; either winding; zero area: the face contributes nothing); face_class F int32, a value outside [0, C) skips
 * the face; face_weight F f64.  Rings: ring_vertices n_ring_vertices x 2 int64 in the same units and origin, no repeated closing
 * vertex; ring r is vertices ring_offsets[r] .. ring_offsets[r + 1] (R + 1 int64; fewer than 3 vertices: ignored), belongs to
 * row ring_polygon[r] (int32, NON-DECREASING in r: the rings of a polygon are consecutive; outside [0, P): ignored) and is a hole
 * where ring_is_hole[r] != 0 (int32).  For GR_POLY_OVERLAY every ring must be counter-clockwise.  polygon_boxes: P x 4 int64
 * xmin ymin xmax ymax over the polygon's rings.
 *   GR_POLY_WITHIN   a face adds area(snapped triangle) * weight to weights[p][class] iff the closed triangle lies in the closed
 *                    region of polygon p (exteriors minus holes, even-odd over its rings), decided exactly with integer signs
 *   GR_POLY_OVERLAY  every face adds area(triangle n polygon) * weight, the area clipped in f64 (Sutherland-Hodgman, the ring
 *                    against the triangle's three half-planes), exterior rings minus holes
 * weights: P x C f64, zeroed and written by the call; faces of one wave are summed in a fixed order, waves meet in f64 atomics,
 * so sums can differ in their last bits from run to run (the decisions cannot).  stats: GR_POLY_STAT_WORDS uint64 on the device.
 * Only enqueues work on `stream`; needs no uploaded mesh and no context scratch.  Added without a GR_VERSION bump. */
enum {
  GR_POLY_OVERLAY = 0,
  GR_POLY_WITHIN = 1
};
enum {
  GR_POLY_STAT_TESTED = 0,        /* (face, polygon) pairs whose boxes overlap                                       */
  GR_POLY_STAT_CONTRIBUTING = 1,  /* ... that added to `weights`                                                      */
  GR_POLY_STAT_LARGEST_RING = 2,  /* vertices of the largest ring                                                     */
  GR_POLY_STAT_WORDS = 4
};
int gr_polygon_class_weights(gr_ctx *ctx, const int64_t *tri, const int32_t *face_class, const double *face_weight, int64_t F,
                             const int64_t *ring_vertices, int64_t n_ring_vertices, const int64_t *ring_offsets,
                             const int32_t *ring_polygon, const int32_t *ring_is_hole, int64_t R,
                             const int64_t *polygon_boxes, int64_t P, int mode, int C, double *weights, uint64_t *stats,
                             void *stream);

/* Vector textures -- replaces the gpd.overlay of face centres against polygons in get_values_for_faces_from_vector
 * (meshes/meshes.py:990-1079): the polygon row each face centre lies in; the rule-set is DESIGN.md "Vector textures" (V1-V6).
 * verts_q: V x 2 int64 snapped vertices (units of 1e-6 m behind a common origin, |value| <= 2^40); faces: F x 3 int32.  The query
 * point of a face is the exact integer 3 x centre, the sum of its three vertices, formed on the device; ring vertices enter every
 * comparison times 3.  Ring table as for gr_polygon_class_weights (ring_polygon non-decreasing; hole flags are not needed: a row's
 * closed region is "on an edge or vertex of any of its rings, or an odd number of crossings over all of them").
 * Cell index over the polygon boxes, in the units of the query point: cell (ix, iy) covers grid_x0 + ix cell_w <= x < grid_x0 +
 * (ix + 1) cell_w, likewise in y, 0 <= ix < nx, 0 <= iy < ny; cell_offsets: nx ny + 1 int64, rising; cell_polygons
 * [cell_offsets[iy nx + ix] .. cell_offsets[iy nx + ix + 1]): the rows whose box meets the cell, in DESCENDING order.  A centre
 * outside the grid is in no row.  The lane of a face walks the list of the centre's cell -- box test, then the rings -- and stops at
 * the first row that contains the centre: face_polygon[f] (F int32, written by the call) is the HIGHEST such row, -1 for none.  The
 * result does not depend on the grid as long as every row is listed in every cell its box meets.
 * stats: GR_FPI_STAT_WORDS uint64 on the device.  A face with a vertex index outside [0, V) reads nothing, gets -1 and is counted
 * in GR_FPI_STAT_BAD_FACES; offsets and rows outside their tables are clamped or skipped.  GR_EINVAL (the message names
 * gr_face_polygon_index): null arrays, negative sizes, nx or ny < 1, nx ny > GR_FPI_MAX_CELLS, a cell size < 1.  Only enqueues work
 * on `stream`; needs no uploaded mesh and no context scratch.  Added without a GR_VERSION bump. */
enum {
  GR_FPI_STAT_TESTED = 0,        /* (face, row) pairs whose box holds the centre: ring walks started                  */
  GR_FPI_STAT_LABELLED = 1,      /* faces with a row                                                                  */
  GR_FPI_STAT_LONGEST_LIST = 2,  /* entries of the longest cell list a centre fell into                               */
  GR_FPI_STAT_BAD_FACES = 3,     /* faces with a vertex index outside [0, V)                                          */
  GR_FPI_STAT_WORDS = 4
};
enum {
  GR_FPI_MAX_CELLS = 16777216
};
int gr_face_polygon_index(gr_ctx *ctx, const int64_t *verts_q, int64_t V, const int32_t *faces, int64_t F,
                          const int64_t *ring_vertices, int64_t n_ring_vertices, const int64_t *ring_offsets,
                          const int32_t *ring_polygon, int64_t R, const int64_t *polygon_boxes, int64_t P, int64_t grid_x0,
                          int64_t grid_y0, int64_t cell_w, int64_t cell_h, int nx, int ny, const int64_t *cell_offsets,
                          const int32_t *cell_polygons, int64_t n_cell_polygons, int32_t *face_polygon, uint64_t *stats,
                          void *stream);

/* Region of interest -- replaces the gpd.overlay of every mesh vertex against the buffered ROI and VTK's extract_points in
 * select_mesh_ROI (meshes/meshes.py:646-731) and the buffered `within` of get_subset_ROI (cameras/cameras.py:1207-1273); the
 * rule-set is DESIGN.md "Region of interest" (Q1-Q6).
 * gr_points_in_region: points_q N x 2 int64 snapped points (units of 1e-6 m behind a common origin, |value| <= 2^40); ring table as
 * for gr_face_polygon_index (ring_polygon non-decreasing, a ring of fewer than 3 vertices is ignored, a row whose box is empty --
 * xmin > xmax -- holds nothing); D: the buffer in grid steps, 0 <= D < 2^40.  mask[i] (N uint8, written by the call) is 1 iff point
 * i lies in the closed region of ANY row (on an edge or vertex of one of its rings, or an odd number of crossings over the row's
 * rings: overlapping rows unite) or, with D > 0, within D of an edge of any ring, holes included -- decided exactly in integers,
 * the perpendicular case cross^2 <= D^2 |e|^2 through a 256-bit product.  Edges are visited in table order; a point stops being
 * tested against the buffer once an edge is within D and against everything once it is contained.
 * stats: GR_PIR_STAT_WORDS uint64 on the device.  GR_EINVAL (the message names gr_points_in_region): null arrays, negative sizes, D
 * outside [0, 2^40).  R = 0 or P = 0: an all-zero mask.  Only enqueues work on `stream`; needs no uploaded mesh; 32 bytes of
 * context scratch.  Added without a GR_VERSION bump. */
enum {
  GR_PIR_STAT_INSIDE = 0,       /* points in the region                                                              */
  GR_PIR_STAT_BUFFER_ONLY = 1,  /* ... that no row contains: within D of an edge only                                */
  GR_PIR_STAT_WIDE = 2,         /* 256-bit comparisons formed (the point's foot lies strictly inside the edge)       */
  GR_PIR_STAT_WORDS = 4
};
int gr_points_in_region(gr_ctx *ctx, const int64_t *points_q, int64_t N, const int64_t *ring_vertices, int64_t n_ring_vertices,
                        const int64_t *ring_offsets, const int32_t *ring_polygon, int64_t R, const int64_t *polygon_boxes,
                        int64_t P, int64_t D, uint8_t *mask, uint64_t *stats, void *stream);

/* gr_submesh_extract: mask V uint8 (non-zero: the vertex is selected); faces F x 3 int32.  A face is kept iff one of its vertices
 * is selected, a vertex iff a kept face uses it; both keep their order.  face_ids (capacity F int64) and point_ids (capacity V
 * int64): the ascending original indices of what is kept; new_faces (capacity F x 3 int32): the kept faces, indexing the kept
 * vertices.  counts: 3 uint64 on the device, written by the call: kept faces, kept vertices, faces with a vertex index outside
 * [0, V) -- such a face reads nothing and is not kept.  Entries behind the counts are not written.  Two exclusive scans
 * (hipcub::DeviceScan) between a flag kernel and a write kernel; flags, scans and temporaries live in context scratch.  GR_EINVAL
 * (the message names gr_submesh_extract): null arrays, negative sizes, V or F >= 2^31.  Only enqueues work on `stream`; needs no
 * uploaded mesh.  Added without a GR_VERSION bump. */
int gr_submesh_extract(gr_ctx *ctx, const uint8_t *mask, int64_t V, const int32_t *faces, int64_t F, int64_t *face_ids,
                       int64_t *point_ids, int32_t *new_faces, uint64_t *counts, void *stream);

/* Class outlines -- replaces the per-class unary_union of one shapely triangle per face in export_face_labels_vector
 * (meshes/meshes.py:1308-1445): the outline rings of every class of a per-face labelling, traced on the device; the rule-set is
 * DESIGN.md section 8i (X1-X8).  Integers only: the result is exact and does not depend on scheduling.
 * verts_q: V x 2 int64 snapped vertices (units of 1e-6 m behind a common origin, |value| <= 2^40); faces: F x 3 int32; face_class: F
 * int32; 0 <= n_classes <= GR_OUTL_MAX_CLASSES; V < 2^31 and 3 F < 2^31.  Vertices with equal (x, y) are one vertex, named by the
 * smallest of their indices (canon: V int32).  A face takes part iff 0 <= class < n_classes and its snapped triangle (over the canon
 * ids) has a non-zero area; a clockwise one is turned over.  Per class the directed edges a -> b and b -> a cancel in pairs; what is
 * left, sorted by (class, from, to), are the SLOTS; at every (class, vertex) the k-th incoming slot (by from) is followed by the
 * k-th outgoing one (by to), which closes the slots into rings.  A ring starts at its smallest slot, rings are ordered by that slot.
 * Outputs on the device: ring_vertices (capacity ring_vertex_cap int32: the `from` ids of the slots, ring after ring), ring_offsets
 * (capacity ring_vertex_cap / 3 + 1 int64; rings + 1 are written, the last is the number of ring vertices), ring_class (capacity
 * max(ring_vertex_cap / 3, 1) int32) -- a ring has at least 3 vertices.  *n_edges_h, *n_rings_h (HOST): the number of slots (= ring
 * vertices) and of rings, whether or not they fit.  More slots than ring_vertex_cap: GR_EOVERFLOW and NOTHING is written to the
 * four output arrays; call again with ring_vertex_cap >= *n_edges_h.  ring_vertex_cap == 0 (the four may be NULL): the counts
 * alone.  stats: GR_OUTL_STAT_WORDS uint64 on the device, always written.  A face with a vertex index outside [0, V) reads
 * nothing, takes no part and is counted in GR_OUTL_STAT_BAD_FACES only.  GR_EINVAL (the message names the call): null arrays,
 * negative sizes, V >= 2^31, 3 F >= 2^31, n_classes out of range.  Radix sorts and scans (hipcub) in context scratch (about 40 bytes
 * per vertex or 48 per face corner, 60 per slot); synchronises `stream` to read the counts and behind its last kernel, so the scratch
 * is free on return.  Added without a GR_VERSION bump. */
enum {
  GR_OUTL_STAT_NO_CLASS = 0,    /* faces whose class lies outside [0, n_classes)                                      */
  GR_OUTL_STAT_ZERO_AREA = 1,   /* faces with a class whose snapped triangle has no area                              */
  GR_OUTL_STAT_TURNED = 2,      /* clockwise faces that were turned over                                              */
  GR_OUTL_STAT_CANCELLED = 3,   /* pairs of opposite directed edges of one class that cancelled                       */
  GR_OUTL_STAT_MULTI = 4,       /* distinct (class, from, to) that survive in more than one copy                      */
  GR_OUTL_STAT_BAD_FACES = 5,   /* faces with a vertex index outside [0, V)                                           */
  GR_OUTL_STAT_BAD_ROWS = 6,    /* gr_member_outlines: violations of a well-formed member table (Y2); else 0          */
  GR_OUTL_STAT_WORDS = 8
};
enum {
  GR_OUTL_MAX_CLASSES = 65535,
  GR_MEMBER_MAX_CLASSES = 2147483646   /* 2^31 - 2: the sentinel class n_classes fits int32 */
};
int gr_class_outlines(gr_ctx *ctx, const int64_t *verts_q, int64_t V, const int32_t *faces, int64_t F, const int32_t *face_class,
                      int n_classes, int32_t *canon, int32_t *ring_vertices, int64_t *ring_offsets, int32_t *ring_class,
                      int64_t ring_vertex_cap, int64_t *n_edges_h, int64_t *n_rings_h, uint64_t *stats, void *stream);

/* Raster samples -- replaces the per-point rasterio.sample of get_values_from_raster_file, the subtraction of
 * get_height_above_ground and the masked write of label_ground_class (meshes/meshes.py:1449-1629): the value of a raster under
 * every face centre or vertex; the rule-set is DESIGN.md "Raster samples" (T1-T7).  Every operation is a float64 operation
 * rounded on its own, in the order written here.
 * points: V x 3 float64, in the raster's CRS.  faces: F x 3 int32 -- a query per face, the centre ((p0 + p1) + p2) / 3.0 per
 * component, formed on the device -- or NULL with F = 0: a query per vertex.  N is F or V accordingly.
 * raster: B x H x W of raster_dtype GR_DTYPE_F32 or GR_DTYPE_F64, C-contiguous.  inverse6_h (a HOST pointer): the inverse affine
 * transform (ia, ib, ic, id, ie, if): col = floor((x ia + y ib) + ic), row = floor((x id + y ie) + if); the query is inside iff
 * 0 <= col < W and 0 <= row < H, compared as doubles (NaN, infinities and huge coordinates are outside).  Sample of band b:
 * raster[b][row][col] widened to float64 inside, else nodata if has_nodata != 0, else 0.0; then a sample == nodata (has_nodata
 * only; a NaN nodata matches nothing) becomes `fill`.
 * Outputs, each may be NULL: values N x B float64; height N float64 = z of the query - the sample of band 0; labels_inout N
 * float64, rewritten in place: labels[i] = ground_id where height < threshold (NaN: never) and, with GR_RS_FLAG_ONLY_EXISTING in
 * `flags`, labels[i] is finite.  threshold, ground_id and flags are read only with labels_inout.
 * stats: GR_RS_STAT_WORDS uint64 on the device, written by the call.  A face with a vertex index outside [0, V) reads nothing:
 * its samples are those of a query outside the raster, its height is NaN, its label is kept, and it is counted in
 * GR_RS_STAT_BAD_FACES only.  GR_EINVAL (the message names gr_sample_raster): null points / raster / inverse6_h / stats, null faces
 * with F > 0, negative sizes, B, H or W < 1, another raster_dtype.  N = 0 is GR_OK.  Only enqueues work on `stream`; needs no
 * uploaded mesh and no context scratch.  Added without a GR_VERSION bump. */
enum {
  GR_RS_STAT_INSIDE = 0,     /* queries whose cell lies in the raster                                              */
  GR_RS_STAT_NODATA = 1,     /* queries with a sample that equalled nodata (those outside a raster with a nodata too) */
  GR_RS_STAT_GROUND = 2,     /* labels rewritten to ground_id                                                      */
  GR_RS_STAT_BAD_FACES = 3,  /* faces with a vertex index outside [0, V)                                           */
  GR_RS_STAT_WORDS = 4
};
enum {
  GR_RS_FLAG_ONLY_EXISTING = 1  /* relabel only labels that are finite (only_label_existing_labels) */
};
int gr_sample_raster(gr_ctx *ctx, const double *points, int64_t V, const int32_t *faces, int64_t F, const void *raster,
                     int raster_dtype, int B, int H, int W, const double *inverse6_h, int has_nodata, double nodata, double fill,
                     double *values, double *height, double *labels_inout, double threshold, double ground_id, int flags,
                     uint64_t *stats, void *stream);

/* Image selection -- replaces the SetCoverPy stage of entrypoints/annotation_image_selection.py:142-174: a small set of views that
 * together see every required face of a face x view incidence; the rule-set is DESIGN.md section 8j (M1-M8).  Integers only: the
 * result is exact and does not depend on scheduling.
 * The incidence is face-major CSR, all on the device: face_ptr F + 1 int64 (rising, face_ptr[0] = 0, face_ptr[F] = nnz), face_views
 * nnz int32, unique within a row; an entry means "the view sees the face", values play no part.  A face is required iff its row has
 * at least max(min_observations, 1) entries.  Greedy: while a view sees a required face that no selected view sees, the view that
 * sees most of them is selected, ties to the LOWEST view index.  With GR_SETCOVER_PRUNE in `flags` the selected views are then
 * examined last selected first, and one whose required faces are all seen by another selected view is deselected at once.
 * Outputs on the device, written by the call: selected n_views uint8 (the mask); order n_views int32 (the views in the order
 * selected, -1 behind them); gains n_views int64 (the faces each added, 0 behind them); pruned n_views int32 (the deselected views
 * in the order examined, -1 behind them); stats GR_SETCOVER_STAT_WORDS int64.  GR_SETCOVER_GLOBAL_ATOMICS in `flags` makes the
 * gain updates plain global atomics at every n_views (above GR_SETCOVER_LDS_VIEWS they always are; for measurements and tests: the
 * results are the same).  GR_EINDEX: a view index outside [0, n_views) or a row pointer outside [0, nnz], found on the device; the
 * outputs are then undefined.  GR_EINVAL (the message names gr_set_cover): null arrays, negative sizes, F >= 2^31, n_views >
 * GR_SETCOVER_MAX_VIEWS, a NaN threshold.  F = 0 or n_views = 0: an empty selection.  Pick / apply launches are enqueued
 * GR_SETCOVER_BATCH pairs at a time and `stream` is synchronised once per batch and behind the last kernel, so the context scratch
 * (about 9 bytes per face, 4 per entry, 28 per view) is free on return.  Needs no uploaded mesh.  Added without a GR_VERSION bump. */
enum {
  GR_SETCOVER_PRUNE = 1,           /* M6: drop selected views that the later picks made redundant                         */
  GR_SETCOVER_GLOBAL_ATOMICS = 2   /* no LDS histograms                                                                  */
};
enum {
  GR_SETCOVER_MAX_VIEWS = 65536,   /* n_views limit                                                                      */
  GR_SETCOVER_LDS_VIEWS = 4096,    /* n_views up to which a workgroup collects gain updates in an LDS histogram          */
  GR_SETCOVER_BATCH = 64           /* pick / apply pairs enqueued between two reads of the control words                 */
};
enum {
  GR_SETCOVER_STAT_REQUIRED = 0,       /* required faces                                                                 */
  GR_SETCOVER_STAT_COVERED = 1,        /* ... that a selected view sees: counted from the flags, equal to the above      */
  GR_SETCOVER_STAT_SELECTED = 2,       /* k: views the greedy stage selected                                             */
  GR_SETCOVER_STAT_PRUNED = 3,         /* p: views the prune stage deselected                                            */
  GR_SETCOVER_STAT_BATCHES = 4,        /* batches the greedy stage took                                                  */
  GR_SETCOVER_STAT_LDS_HISTOGRAM = 5,  /* 1: gain updates went through LDS histograms                                    */
  GR_SETCOVER_STAT_WORDS = 8
};
int gr_set_cover(gr_ctx *ctx, const int64_t *face_ptr, const int32_t *face_views, int64_t nnz, int64_t F, int32_t n_views,
                 double min_observations, int flags, uint8_t *selected, int32_t *order, int64_t *gains, int32_t *pruned,
                 int64_t *stats, void *stream);

/* CRS reprojection -- replaces the pyproj.Transformer of reproject_CRS and get_mesh_points_in_CRS (meshes/meshes.py:231-286,
 * 752-783), get_camera_location (cameras/cameras.py:212-242) and convert_CRS_3D_points (utils/geospatial.py:60-71) for the systems
 * on the WGS84 ellipsoid: points between ECEF (EPSG:4978), geographic coordinates and a transverse Mercator (the UTM zones); one
 * ellipsoid, no datum shift.  The rule-set is DESIGN.md "CRS reprojection" (G1-G9).  Every operation is a float64 operation rounded
 * on its own; the device library's trigonometric and hyperbolic functions are not correctly rounded, so the results are pinned by
 * the tolerance of G9 (a few 1e-9 m), not bit for bit.
 * A gr_crs names a system: kind GR_CRS_ECEF (X, Y, Z in metres), GR_CRS_GEOGRAPHIC (lon, lat in degrees, ellipsoidal height in
 * metres -- longitude FIRST) or GR_CRS_TM (easting, northing, height; lon0 in degrees, k0 > 0, false easting and northing in metres,
 * all finite; UTM zone z: lon0 = 6 z - 183, k0 = 0.9996, 500000, 0 north or 10000000 south).  The four parameters are read for
 * GR_CRS_TM only.  from_h and to_h are HOST pointers.
 * points: V x 3 float64 in `from`.  pre16_h (a HOST pointer, or NULL): a row-major 4 x 4 whose first three rows are applied to
 * every input row first, ((m0 x + m1 y) + m2 z) + m3 per component -- the cameras' local_to_epsg_4978 --, with an ECEF source only.
 * faces: F x 3 int32 -- an output row per face, ((p0 + p1) + p2) / 3.0 per component of its three REPROJECTED vertices, what
 * cell_centers() of the reprojected mesh gives -- or NULL with F = 0: an output row per vertex.  N is F or V accordingly.
 * out: N x 3 float64; without faces it may be `points` (in place).  Rows that cannot be converted are NaN in all three components
 * and counted once, in the first of these that applies: GR_CRS_STAT_BAD_FACES, a face with a vertex index outside [0, V) (nothing
 * is read through it); GR_CRS_STAT_NONFINITE, a non-finite coordinate (after the pre-transform), the ECEF origin or a latitude
 * outside [-90, 90] (for a face: in any of its vertices); GR_CRS_STAT_BEYOND, 90 degrees or more from the central meridian of a
 * transverse Mercator, source or target.  An ECEF point on the axis has longitude 0.  Longitudes come out in (-180, 180].
 * stats: GR_CRS_STAT_WORDS uint64 on the device, written by the call.  GR_EINVAL (the message names the call): null points / out /
 * from_h / to_h / stats, null faces with F > 0, negative sizes, V >= 2^31, an unknown kind, a k0 that is not > 0 or a parameter that
 * is not finite, pre16_h with a source that is not ECEF, faces with out == points.  N = 0 is GR_OK.  Only enqueues work on `stream`
 * (a grid-stride loop over at most GR_CRS_MAX_GROUPS workgroups of 256 lanes); needs no uploaded mesh and no context scratch.  Added
 * without a GR_VERSION bump. */
enum {
  GR_CRS_ECEF = 0,
  GR_CRS_GEOGRAPHIC = 1,
  GR_CRS_TM = 2
};
enum {
  GR_CRS_STAT_NONFINITE = 0,  /* rows with a non-finite coordinate, the ECEF origin, a latitude outside [-90, 90]         */
  GR_CRS_STAT_BEYOND = 1,     /* rows 90 degrees or more from a central meridian                                          */
  GR_CRS_STAT_BAD_FACES = 2,  /* faces with a vertex index outside [0, V)                                                 */
  GR_CRS_STAT_WORDS = 4
};
enum {
  GR_CRS_MAX_GROUPS = 8192    /* workgroups of the launch: 256 * GR_CRS_MAX_GROUPS rows per pass of the stride loop        */
};
typedef struct gr_crs {
  int32_t kind;           /* GR_CRS_ECEF, GR_CRS_GEOGRAPHIC, GR_CRS_TM */
  double lon0;            /* central meridian, degrees                 */
  double k0;              /* scale on the central meridian             */
  double false_easting;   /* metres                                    */
  double false_northing;  /* metres                                    */
} gr_crs;
int gr_reproject_points(gr_ctx *ctx, const double *points, int64_t V, const int32_t *faces, int64_t F, const double *pre16_h,
                        const gr_crs *from_h, const gr_crs *to_h, double *out, uint64_t *stats, void *stream);

/* The calls that came after this header's function list was closed are declared in companion headers, which this one brings in:
 * everything stays available through geograster.h. */
#include "geograster_outlines.h"

/* The orthomosaic baseline (geograster_ortho.h): the count types of the tile assembly and the words of its
 * statistics block, the work items and the statistics words of the zonal class counts. */
enum {
  GR_COUNT_U8 = 0,   /* counts and weights are uint8: sums modulo 2^8   */
  GR_COUNT_U16 = 1,  /* uint16: sums modulo 2^16                        */
  GR_COUNT_F64 = 2   /* float64: adds in ascending tile index           */
};
enum {
  GR_ORTHO_STAT_WITH_CLASS = 0,    /* pixels that took a class                                  */
  GR_ORTHO_STAT_WITHOUT = 1,       /* pixels written as nodataval                               */
  GR_ORTHO_STAT_LONGEST_LIST = 2,  /* the most tiles that cover one pixel                       */
  GR_ORTHO_STAT_PAIRS = 3,         /* (tile, pixel) pairs read                                  */
  GR_ORTHO_STAT_WORDS = 4
};
enum {
  GR_ORTHO_MAX_CLASSES = 255
};
enum {
  GR_ZONAL_STAT_TESTED = 0,          /* cells of the work items                                 */
  GR_ZONAL_STAT_INSIDE = 1,          /* (row, cell) pairs with the cell's centre in the row     */
  GR_ZONAL_STAT_NODATA = 2,          /* ... of them nodata                                      */
  GR_ZONAL_STAT_OVER = 3,            /* ... of them with a value >= C (counted nowhere else)    */
  GR_ZONAL_STAT_LARGEST_PLUS_1 = 4,  /* 1 + the largest value of an inside cell that is not nodata; 0 without one */
  GR_ZONAL_STAT_LARGEST_RING = 5,    /* the vertices of the largest ring                        */
  GR_ZONAL_STAT_RINGS_IGNORED = 6,   /* rings of fewer than 3 vertices                          */
  GR_ZONAL_STAT_WORDS = 8
};
enum {
  GR_ZONAL_MAX_CLASSES = 256,
  GR_ZONAL_ITEM_INTS = 7,    /* int32 values of a work item                                     */
  GR_ZONAL_BLOCK_W = 64,     /* the widest and the tallest block of cells a work item may name  */
  GR_ZONAL_BLOCK_H = 128
};
#include "geograster_ortho.h"

/* Mesh decimation by vertex clustering (geograster_decimate.h): the words of its statistics block.  The first
 * three are the counts of the sub-mesh extraction, in its order. */
enum {
  GR_DECIM_STAT_KEPT_FACES = 0,     /* faces of the decimated mesh                                            */
  GR_DECIM_STAT_KEPT_VERTICES = 1,  /* vertices of the decimated mesh                                         */
  GR_DECIM_STAT_BAD_FACES = 2,      /* faces with a vertex index outside [0, V) or a vertex without a cell    */
  GR_DECIM_STAT_CELLS = 3,          /* occupied cells                                                         */
  GR_DECIM_STAT_COLLAPSED = 4,      /* faces with two corners in one cell                                     */
  GR_DECIM_STAT_DUPLICATES = 5,     /* faces dropped behind an earlier face with the same three cells         */
  GR_DECIM_STAT_OUTSIDE = 6,        /* vertices outside the key range: q < 0 or a cell component >= 2^21      */
  GR_DECIM_STAT_WORDS = 8
};
#include "geograster_decimate.h"

/* Polygon rows burned into a label raster (geograster_burn.h): the words of the statistics block of the
 * burn and the workgroup cap of its value pass.  The work items are those of the zonal class counts (GR_ZONAL_ITEM_INTS,
 * GR_ZONAL_BLOCK_W, GR_ZONAL_BLOCK_H). */
enum {
  GR_BURN_STAT_TESTED = 0,         /* cells of the work items                                              */
  GR_BURN_STAT_INSIDE = 1,         /* (row, cell) memberships: the cell's centre lies in the row           */
  GR_BURN_STAT_BURNED = 2,         /* cells that took a row, counted by the value pass: 0 without `out`    */
  GR_BURN_STAT_LARGEST_RING = 3,   /* the vertices of the largest ring                                     */
  GR_BURN_STAT_RINGS_IGNORED = 4,  /* rings of fewer than 3 vertices                                       */
  GR_BURN_STAT_WORDS = 8
};
enum {
  GR_BURN_MAX_GROUPS = 8192        /* workgroups of the value pass: beyond it the lanes stride the plane   */
};
#include "geograster_burn.h"

/* Polygon-on-polygon overlap areas (geograster_overlap.h): the words of the statistics block, the
 * integers of a work item and the largest tiles an item may name. */
enum {
  GR_OVERLAP_STAT_PAIRS = 0,          /* pairs handed in                                                      */
  GR_OVERLAP_STAT_ITEMS = 1,          /* work items that ran                                                  */
  GR_OVERLAP_STAT_EDGE_PAIRS = 2,     /* edge pairs that took part: a common x-range of positive width (A3)   */
  GR_OVERLAP_STAT_VERTICAL = 3,       /* vertical edges of both tables, in rings of 3 or more vertices (A4)   */
  GR_OVERLAP_STAT_RINGS_IGNORED = 4,  /* rings of fewer than 3 vertices, both tables                          */
  GR_OVERLAP_STAT_LARGEST_RING = 5,   /* the vertices of the largest ring of either table                     */
  GR_OVERLAP_STAT_BAD_ITEMS = 6,      /* work items skipped whole (A8)                                        */
  GR_OVERLAP_STAT_WORDS = 8
};
enum {
  GR_OVERLAP_ITEM_INTS = 5,           /* pair, first edge slot and slots of row a, first slot and slots of row b */
  GR_OVERLAP_TILE_A = 256,            /* edge slots of row a in one item: the records of a workgroup's LDS    */
  GR_OVERLAP_TILE_B = 4096            /* edge slots of row b in one item: 16 per lane                         */
};
#include "geograster_overlap.h"

/* Communities of the ray graph (geograster_communities.h): flags, limits and the words of the
 * statistics block. */
enum {
  GR_COMM_FORCE_GROUP = 1,            /* every row that fits goes through the workgroup path (tests; same results)  */
  GR_COMM_FORCE_KEY = 2               /* every row goes through the key path (tests; same results)                  */
};
enum {
  GR_COMM_MAX_VERTICES = 8388608,     /* n limit, 2^23: that of gr_ray_pairs                                        */
  GR_COMM_MAX_EDGES = 1069547520,     /* 2^30 - 2^22; E stays below it: 2 E + n entries fit a 32-bit count          */
  GR_COMM_MAX_LEVELS = 64,            /* L11                                                                        */
  GR_COMM_LDS_ROW = 1024              /* entries of the longest row the workgroup path sorts in LDS                 */
};
enum {
  GR_COMM_CAP_SWEEPS = 1,             /* GR_COMM_STAT_CAPS: a level was ended by max_sweeps                         */
  GR_COMM_CAP_LEVELS = 2              /* ... the run was ended by GR_COMM_MAX_LEVELS                                */
};
enum {
  GR_COMM_STAT_LEVELS = 0,            /* levels that moved a vertex: those the labels are composed of               */
  GR_COMM_STAT_LEVELS_RUN = 1,        /* levels that ran: the one without a move, which is discarded, included      */
  GR_COMM_STAT_CAPS = 2,              /* the OR of GR_COMM_CAP_*                                                    */
  GR_COMM_STAT_ROWS_WAVE = 3,         /* rows the wave path handled, summed over all sweeps                         */
  GR_COMM_STAT_ROWS_GROUP = 4,        /* ... the workgroup path                                                     */
  GR_COMM_STAT_ROWS_KEY = 5,          /* ... the key path                                                           */
  GR_COMM_STAT_BAD_EDGES = 6,         /* edges that break L2                                                        */
  GR_COMM_STAT_COMMUNITIES = 7,       /* n_communities                                                              */
  GR_COMM_STAT_M2 = 8,                /* the sum of all directed entries: twice the sum of the weights              */
  GR_COMM_STAT_SWEEPS = 16,           /* GR_COMM_MAX_LEVELS words: sweeps of every level that ran                   */
  GR_COMM_STAT_MOVES = 80,            /* GR_COMM_MAX_LEVELS words: moves of every level that ran                    */
  GR_COMM_STAT_WORDS = 144
};
#include "geograster_communities.h"

/* Exact Douglas-Peucker on polygon rings (geograster_simplify.h): the words of the statistics block. */
enum {
  GR_SIMPLIFY_STAT_KEPT = 0,          /* vertices kept: M = out_offsets[R]                                          */
  GR_SIMPLIFY_STAT_COLLAPSED = 1,     /* rings of 3 or more vertices that came out empty (S6)                       */
  GR_SIMPLIFY_STAT_PASSES = 2,        /* passes: the depth of the deepest chain that had an interior vertex         */
  GR_SIMPLIFY_STAT_WIDE = 3,          /* distances compared beyond 128 bits: interior vertices whose foot lay       */
                                      /* strictly inside their chord (S3: the squared cross product), over all passes */
  GR_SIMPLIFY_STAT_SHORT_RINGS = 4,   /* input rings of fewer than 3 vertices, which come out empty                 */
  GR_SIMPLIFY_STAT_WORDS = 8
};
#include "geograster_simplify.h"

/* Top-down raster of a mesh (geograster_nadir.h): the words of the statistics block. */
enum {
  GR_NADIR_STAT_FACES = 0,            /* faces taking part (N3)                                                     */
  GR_NADIR_STAT_BAD_INDEX = 1,        /* faces that name a vertex outside [0, V)                                    */
  GR_NADIR_STAT_ZERO_AREA = 2,        /* faces whose snapped triangle has no area: vertical walls, needles          */
  GR_NADIR_STAT_NONFINITE_Z = 3,      /* faces with a z that is not finite                                          */
  GR_NADIR_STAT_EMPTY_BOX = 4,        /* faces taking part whose box holds no cell centre of the window             */
  GR_NADIR_STAT_ITEMS = 5,            /* items of the faces above small_cells (64 columns x item_rows rows each)    */
  GR_NADIR_STAT_TESTS = 6,            /* (face, cell) tests: the centres of the clipped boxes                       */
  GR_NADIR_STAT_INSIDE = 7,           /* (face, cell) memberships (N4)                                              */
  GR_NADIR_STAT_SKIPPED = 8,          /* memberships skipped by N5: denominator 0 or a height that is not finite    */
  GR_NADIR_STAT_COVERED = 9,          /* cells of the window that a face covers                                     */
  GR_NADIR_STAT_WORDS = 10
};
#include "geograster_nadir.h"

/* Pictures (geograster_vis.h): a shaded view from an id and a depth plane, the three-panel composite
 * of a photo and a label image.  Both calls take one descriptor, declared there. */
#include "geograster_vis.h"

/* Raster -> raster warp (geograster_warp.h): the resampling rules, the words of the statistics block
 * and the largest band count.  The call takes one descriptor, declared there. */
enum {
  GR_WARP_NEAREST = 0,
  GR_WARP_BILINEAR = 1
};
enum {
  GR_WARP_STAT_CELLS = 0,             /* cells of the window                                                        */
  GR_WARP_STAT_OUTSIDE = 1,           /* cells whose centre (nearest) or whose four taps (bilinear) miss the source */
  GR_WARP_STAT_NONFINITE = 2,         /* centres the CRS step refuses as not finite (GR_CRS_STAT_NONFINITE's rule)  */
  GR_WARP_STAT_BEYOND = 3,            /* centres 90 degrees or more from a central meridian                         */
  GR_WARP_STAT_NODATA = 4,            /* cells that met the source's nodata value or a NaN, in any band             */
  GR_WARP_STAT_DEN_ZERO = 5,          /* bilinear cells whose participating weights sum to 0, in any band           */
  GR_WARP_STAT_WORDS = 8
};
enum {
  GR_WARP_MAX_BANDS = 16
};
#include "geograster_warp.h"

/* Face sieve (geograster_components.h): the words of the statistics block.  The call takes one
 * descriptor, declared there. */
enum {
  GR_SIEVE_STAT_ROUNDS = 0,             /* rounds that changed a face                                                  */
  GR_SIEVE_STAT_COMPONENTS_BEFORE = 1,  /* components of the input labelling                                           */
  GR_SIEVE_STAT_COMPONENTS_AFTER = 2,   /* components of the final labelling (comp)                                    */
  GR_SIEVE_STAT_FACES_CHANGED = 3,      /* faces whose class a round changed, summed over the rounds                   */
  GR_SIEVE_STAT_SMALL_LEFT = 4,         /* small components (I7) of the final labelling                                */
  GR_SIEVE_STAT_DEGENERATE = 5,         /* faces with two equal corners                                                */
  GR_SIEVE_STAT_FAN_EDGES = 6,          /* edges shared by more than two faces                                         */
  GR_SIEVE_STAT_ROUND_CAP = 7,          /* 1: max_rounds rounds changed a face, the labelling may not be final         */
  GR_SIEVE_STAT_BAD_FACES = 8,          /* faces with a corner or a vertex_canon entry outside [0, V)                  */
  GR_SIEVE_STAT_WORDS = 9
};
#include "geograster_components.h"

/* Nearest points (geograster_nearest.h): the words of the statistics block.  The call takes one
 * descriptor, declared there. */
enum {
  GR_NN_STAT_REF_NONFINITE = 0,    /* ref rows with a NaN or infinite coordinate: they take no part                */
  GR_NN_STAT_QUERY_NONFINITE = 1,  /* query rows with one: index -1, dist2 NaN                                     */
  GR_NN_STAT_NO_ANSWER = 2,        /* queries whose index is -1 (non-finite, no ref, or none within max_distance)  */
  GR_NN_STAT_LEVELS = 3,           /* grid levels run                                                              */
  GR_NN_STAT_CARRIED = 4,          /* queries carried to a coarser level, summed over the levels                   */
  GR_NN_STAT_CELLS_PROBED = 5,     /* runs of cells looked up in the sorted keys                                   */
  GR_NN_STAT_CANDIDATES = 6,       /* distances evaluated                                                          */
  GR_NN_STAT_CELL_BITS = 7,        /* the cell side of the first level, the bits of the float64 (0: no level ran)  */
  GR_NN_STAT_RING_CAP = 8,         /* 1: a query was not settled within max_rings rings of some level             */
  GR_NN_STAT_WORDS = 9
};
#include "geograster_nearest.h"

#ifdef __cplusplus
}
#endif
#endif /* GEOGRASTER_H */
