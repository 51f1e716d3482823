"""ctypes binding of libgeograster (include/geograster.h) and the device backend the mesh class drives.

The library is the product: there is no CPU fallback.  Importing this module is cheap; the first use of
`HipRaster` loads `csrc/libgeograster.so` and raises `RuntimeError` when the shared object or a GPU is missing.
PyTorch-ROCm supplies device memory (tensors), streams and `torch.distributed`; no torch type crosses the C ABI,
only `tensor.data_ptr()` and the raw `hipStream_t` of the current torch stream.
"""
from __future__ import annotations

import ctypes
import threading
from collections import namedtuple
from pathlib import Path
from typing import Optional

import os as _os

import numpy as np

# GEOGRAYPHER_AMD_LIB: a diagnostic build of the same library (geograypher_amd.build.build_variant) instead of the product's
_LIB_PATH = Path(_os.environ.get("GEOGRAYPHER_AMD_LIB") or Path(__file__).resolve().parent / "csrc" / "libgeograster.so")
_lib = None

# The enumerators of include/geograster.h, name for name (tests/test_cabi.py parses the header and compares).
GR_OK = 0
GR_EINVAL = -1
GR_EHIP = -2
GR_ENOMEM = -3
GR_ENOMESH = -4
GR_EINDEX = -5
GR_EOVERFLOW = -6
GR_ENODEVICE = -7
GR_FLAG_NEG1_IS_LAST_FACE = 1
GR_FLAG_DEFER_CHECK = 2
GR_CAM_FLOATS = 16
GR_DTYPE_U8 = 0
GR_DTYPE_F32 = 1
GR_DTYPE_F64 = 2
# keys of set_option
GR_OPT_TILE_H_LOG2 = 2
GR_OPT_BATCH = 3
GR_OPT_DIRECT_CAP = 6
GR_OPT_VARIANT = 7
GR_OPT_SHARE_LEARNED = 8
GR_OPT_DIRECT_BUDGET_MB = 9
GR_OPT_VERTEX_ORDER = 10
GR_OPT_DEBUG_LDS = 98
GR_OPT_DEBUG = 99
# bits of GR_OPT_VARIANT
GR_VAR_ONE_TILE = 1
GR_VAR_VOTES_INLINE = 4
GR_VAR_CHAINS = 16
GR_VAR_ENT48 = 128
GR_VAR_GENERAL_IDS = 512
GR_VAR_MICRO_NEVER = 4096
GR_VAR_MICRO_ALWAYS = 8192
GR_VAR_NO_LOOK = 16384
GR_VAR_PACKED_COUNTERS = 131072
# bits of GR_OPT_DEBUG
GR_DBG_POISON_SLOTS = 512
GR_DBG_POISON_RAYS = 1024
GR_DBG_RAY_GRID_7 = 2048
GR_DBG_POISON_STAGE = 4096      # every stage call fills the whole block of stage scratch it was given with 0xFF first
GR_DBG_POISON_STAGE_7F = 8192   # ... with 0x7F (0xFF wins when both are set)
# bits of overflow_causes()
GR_CAUSE_LIST_OUTGREW = 1
GR_CAUSE_SHORT_MISS = 2
GR_CAUSE_LISTS_MET = 4
# mode of polygon_class_weights, words of its statistics block
GR_POLY_OVERLAY = 0
GR_POLY_WITHIN = 1
GR_POLY_STAT_TESTED = 0
GR_POLY_STAT_CONTRIBUTING = 1
GR_POLY_STAT_LARGEST_RING = 2
GR_POLY_STAT_WORDS = 4
# words of face_polygon_index's statistics block, the largest cell grid it takes
GR_FPI_STAT_TESTED = 0
GR_FPI_STAT_LABELLED = 1
GR_FPI_STAT_LONGEST_LIST = 2
GR_FPI_STAT_BAD_FACES = 3
GR_FPI_STAT_WORDS = 4
GR_FPI_MAX_CELLS = 16777216
# words of points_in_region's statistics block
GR_PIR_STAT_INSIDE = 0
GR_PIR_STAT_BUFFER_ONLY = 1
GR_PIR_STAT_WIDE = 2
GR_PIR_STAT_WORDS = 4
# words of class_outlines' statistics block, the most classes it takes
GR_OUTL_STAT_NO_CLASS = 0
GR_OUTL_STAT_ZERO_AREA = 1
GR_OUTL_STAT_TURNED = 2
GR_OUTL_STAT_CANCELLED = 3
GR_OUTL_STAT_MULTI = 4
GR_OUTL_STAT_BAD_FACES = 5
GR_OUTL_STAT_BAD_ROWS = 6   # member_outlines alone
GR_OUTL_STAT_WORDS = 8
GR_OUTL_MAX_CLASSES = 65535
GR_MEMBER_MAX_CLASSES = 2 ** 31 - 2   # member_outlines: the sentinel class n_classes fits int32
# words of sample_raster's statistics block, its relabel flag
GR_RS_STAT_INSIDE = 0
GR_RS_STAT_NODATA = 1
GR_RS_STAT_GROUND = 2
GR_RS_STAT_BAD_FACES = 3
GR_RS_STAT_WORDS = 4
GR_RS_FLAG_ONLY_EXISTING = 1
# gr_set_cover: flags, limits, stats words
GR_SETCOVER_PRUNE = 1
GR_SETCOVER_GLOBAL_ATOMICS = 2
GR_SETCOVER_MAX_VIEWS = 65536
GR_SETCOVER_LDS_VIEWS = 4096
GR_SETCOVER_BATCH = 64
GR_SETCOVER_STAT_REQUIRED = 0
GR_SETCOVER_STAT_COVERED = 1
GR_SETCOVER_STAT_SELECTED = 2
GR_SETCOVER_STAT_PRUNED = 3
GR_SETCOVER_STAT_BATCHES = 4
GR_SETCOVER_STAT_LDS_HISTOGRAM = 5
GR_SETCOVER_STAT_WORDS = 8
# gr_louvain_communities: flags, limits, stats words
GR_COMM_FORCE_GROUP = 1
GR_COMM_FORCE_KEY = 2
GR_COMM_MAX_VERTICES = 1 << 23
GR_COMM_MAX_EDGES = (1 << 30) - (1 << 22)
GR_COMM_MAX_LEVELS = 64
GR_COMM_LDS_ROW = 1024
GR_COMM_CAP_SWEEPS = 1
GR_COMM_CAP_LEVELS = 2
GR_COMM_STAT_LEVELS = 0
GR_COMM_STAT_LEVELS_RUN = 1
GR_COMM_STAT_CAPS = 2
GR_COMM_STAT_ROWS_WAVE = 3
GR_COMM_STAT_ROWS_GROUP = 4
GR_COMM_STAT_ROWS_KEY = 5
GR_COMM_STAT_BAD_EDGES = 6
GR_COMM_STAT_COMMUNITIES = 7
GR_COMM_STAT_M2 = 8
GR_COMM_STAT_SWEEPS = 16
GR_COMM_STAT_MOVES = 80
GR_COMM_STAT_WORDS = 144
# gr_reproject_points: coordinate kinds, stats words, the launch's workgroup cap
GR_CRS_ECEF = 0
GR_CRS_GEOGRAPHIC = 1
GR_CRS_TM = 2
GR_CRS_STAT_NONFINITE = 0
GR_CRS_STAT_BEYOND = 1
GR_CRS_STAT_BAD_FACES = 2
GR_CRS_STAT_WORDS = 4
GR_CRS_MAX_GROUPS = 8192
# the orthomosaic baseline: count types and stats words of gr_assemble_tiles, work items and stats words of gr_zonal_class_counts
GR_COUNT_U8 = 0
GR_COUNT_U16 = 1
GR_COUNT_F64 = 2
GR_ORTHO_STAT_WITH_CLASS = 0
GR_ORTHO_STAT_WITHOUT = 1
GR_ORTHO_STAT_LONGEST_LIST = 2
GR_ORTHO_STAT_PAIRS = 3
GR_ORTHO_STAT_WORDS = 4
GR_ORTHO_MAX_CLASSES = 255
GR_ZONAL_STAT_TESTED = 0
GR_ZONAL_STAT_INSIDE = 1
GR_ZONAL_STAT_NODATA = 2
GR_ZONAL_STAT_OVER = 3
GR_ZONAL_STAT_LARGEST_PLUS_1 = 4
GR_ZONAL_STAT_LARGEST_RING = 5
GR_ZONAL_STAT_RINGS_IGNORED = 6
GR_ZONAL_STAT_WORDS = 8
GR_ZONAL_MAX_CLASSES = 256
GR_ZONAL_ITEM_INTS = 7
GR_ZONAL_BLOCK_W = 64
GR_ZONAL_BLOCK_H = 128
# mesh decimation by vertex clustering: stats words of gr_cluster_decimate (the first three in submesh_extract's order)
GR_DECIM_STAT_KEPT_FACES = 0
GR_DECIM_STAT_KEPT_VERTICES = 1
GR_DECIM_STAT_BAD_FACES = 2
GR_DECIM_STAT_CELLS = 3
GR_DECIM_STAT_COLLAPSED = 4
GR_DECIM_STAT_DUPLICATES = 5
GR_DECIM_STAT_OUTSIDE = 6
GR_DECIM_STAT_WORDS = 8
# polygon rows burned into a label raster: stats words of gr_burn_polygons, the workgroup cap of its value pass
GR_BURN_STAT_TESTED = 0
GR_BURN_STAT_INSIDE = 1
GR_BURN_STAT_BURNED = 2
GR_BURN_STAT_LARGEST_RING = 3
GR_BURN_STAT_RINGS_IGNORED = 4
GR_BURN_STAT_WORDS = 8
GR_BURN_MAX_GROUPS = 8192
# polygon-on-polygon overlap areas: stats words of gr_polygon_overlap_areas, the integers of a work item, the largest tiles
GR_OVERLAP_STAT_PAIRS = 0
GR_OVERLAP_STAT_ITEMS = 1
GR_OVERLAP_STAT_EDGE_PAIRS = 2
GR_OVERLAP_STAT_VERTICAL = 3
GR_OVERLAP_STAT_RINGS_IGNORED = 4
GR_OVERLAP_STAT_LARGEST_RING = 5
GR_OVERLAP_STAT_BAD_ITEMS = 6
GR_OVERLAP_STAT_WORDS = 8
GR_OVERLAP_ITEM_INTS = 5
GR_OVERLAP_TILE_A = 256
GR_OVERLAP_TILE_B = 4096
# ring simplification: stats words of gr_simplify_rings (include/geograster_simplify.h)
GR_SIMPLIFY_STAT_KEPT = 0
GR_SIMPLIFY_STAT_COLLAPSED = 1
GR_SIMPLIFY_STAT_PASSES = 2
GR_SIMPLIFY_STAT_WIDE = 3
GR_SIMPLIFY_STAT_SHORT_RINGS = 4
GR_SIMPLIFY_STAT_WORDS = 8
# top-down raster of a mesh: stats words of gr_nadir_raster (include/geograster_nadir.h)
GR_NADIR_STAT_FACES = 0
GR_NADIR_STAT_BAD_INDEX = 1
GR_NADIR_STAT_ZERO_AREA = 2
GR_NADIR_STAT_NONFINITE_Z = 3
GR_NADIR_STAT_EMPTY_BOX = 4
GR_NADIR_STAT_ITEMS = 5
GR_NADIR_STAT_TESTS = 6
GR_NADIR_STAT_INSIDE = 7
GR_NADIR_STAT_SKIPPED = 8
GR_NADIR_STAT_COVERED = 9
GR_NADIR_STAT_WORDS = 10
# the raster -> raster warp of include/geograster_warp.h (gr_warp_raster)
GR_WARP_NEAREST = 0
GR_WARP_BILINEAR = 1
GR_WARP_STAT_CELLS = 0
GR_WARP_STAT_OUTSIDE = 1
GR_WARP_STAT_NONFINITE = 2
GR_WARP_STAT_BEYOND = 3
GR_WARP_STAT_NODATA = 4
GR_WARP_STAT_DEN_ZERO = 5
GR_WARP_STAT_WORDS = 8
GR_WARP_MAX_BANDS = 16
# the face sieve of include/geograster_components.h (gr_face_sieve)
GR_SIEVE_STAT_ROUNDS = 0
GR_SIEVE_STAT_COMPONENTS_BEFORE = 1
GR_SIEVE_STAT_COMPONENTS_AFTER = 2
GR_SIEVE_STAT_FACES_CHANGED = 3
GR_SIEVE_STAT_SMALL_LEFT = 4
GR_SIEVE_STAT_DEGENERATE = 5
GR_SIEVE_STAT_FAN_EDGES = 6
GR_SIEVE_STAT_ROUND_CAP = 7
GR_SIEVE_STAT_BAD_FACES = 8
GR_SIEVE_STAT_WORDS = 9
# the nearest-point call of include/geograster_nearest.h (gr_nearest_points)
GR_NN_STAT_REF_NONFINITE = 0
GR_NN_STAT_QUERY_NONFINITE = 1
GR_NN_STAT_NO_ANSWER = 2
GR_NN_STAT_LEVELS = 3
GR_NN_STAT_CARRIED = 4
GR_NN_STAT_CELLS_PROBED = 5
GR_NN_STAT_CANDIDATES = 6
GR_NN_STAT_CELL_BITS = 7
GR_NN_STAT_RING_CAP = 8
GR_NN_STAT_WORDS = 9


class StageTimes(ctypes.Structure):
    _fields_ = [
        ("setup_ms", ctypes.c_float),
        ("scan_ms", ctypes.c_float),
        ("fill_ms", ctypes.c_float),
        ("raster_ms", ctypes.c_float),
        ("project_ms", ctypes.c_float),
        ("vote_ms", ctypes.c_float),
        ("gather_ms", ctypes.c_float),
        ("raster_launches", ctypes.c_int32),
        ("views", ctypes.c_int32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class RasterStats(ctypes.Structure):
    _fields_ = [
        ("records", ctypes.c_int64),
        ("entries", ctypes.c_int64),
        ("max_entries", ctypes.c_int64),
        ("entry_cap", ctypes.c_int64),
        ("overflow", ctypes.c_int32),
        ("views_done", ctypes.c_int32),
        ("blocks", ctypes.c_int64),
        ("chunk_visits", ctypes.c_int64),
        ("rebinned_groups", ctypes.c_int64),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class Crs(ctypes.Structure):
    """gr_crs: kind (GR_CRS_*), and the four parameters of a transverse Mercator."""
    _fields_ = [
        ("kind", ctypes.c_int32),
        ("lon0", ctypes.c_double),
        ("k0", ctypes.c_double),
        ("false_easting", ctypes.c_double),
        ("false_northing", ctypes.c_double),
    ]


_vp, _i32, _i64, _f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
_i64p, _f64p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
# Every symbol include/geograster.h declares -> its argument types (tests check that the header declares and the library
# exports exactly these).  All return int, gr_last_error excepted.
_SIGNATURES = {
    "gr_version": [],
    "gr_ctx_create": [_i32, ctypes.POINTER(_vp)],
    "gr_ctx_destroy": [_vp],
    "gr_last_error": [_vp],
    "gr_set_profiling": [_vp, _i32],
    "gr_set_option": [_vp, _i32, _i32],
    "gr_learned_cache_file": [ctypes.c_char_p],
    "gr_learned_cache_clear": [],
    "gr_get_stage_times": [_vp, ctypes.POINTER(StageTimes)],
    "gr_mesh_upload": [_vp, _vp, _vp, _i64, _i64, _vp],
    "gr_debug_read_upload": [_vp, _vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_uint64), _vp],
    "gr_debug_read_stage": [_vp, _i32, _i64, _i64, _vp, _i64p, _vp],
    "gr_raster_face_ids": [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    "gr_raster_status": [_vp, ctypes.POINTER(RasterStats)],
    "gr_raster_overflow_causes": [_vp],
    "gr_gather_texture_f64": [_vp, _vp, _i64, _vp, _i64, _i32, _vp, _vp],
    "gr_project_labels_u8": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp],
    "gr_project_values_f64": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp],
    "gr_project_view_f64": [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp],
    "gr_raster_project_labels_u8": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp],
    "gr_gather_texture_u8": [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp],
    "gr_project_index_pairs": [_vp, _vp, _vp, _i32, _i32, _i32, _i64, _vp, _vp, _i64, _vp, _i32, _vp],
    "gr_project_rect_pairs": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i64, _vp, _vp, _i64, _vp, _i32, _vp],
    "gr_project_polygon_pairs": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i64, _vp, _vp, _i64, _vp, _i32, _vp],
    "gr_count_pairs": [_vp, _vp, _i64, _vp, _vp, _i64p, _vp],
    "gr_ray_pairs": [_vp, _vp, _vp, _vp, _i64, _f64, _vp, _vp, _vp, _i64, _i64p, _vp],
    "gr_ray_pairs_tile": [_i64, _i64, _i64p, _i64p],
    "gr_rays_clip": [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp],
    "gr_points_bounds": [_vp, _vp, _i64, _i64, _vp, _vp, _vp],
    "gr_cover_grid": [_vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "gr_warp_nearest_i32": [_vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32, ctypes.c_int32, _i32, _f64, _f64, _vp, _vp],
    "gr_warp_f64": [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _f64, _vp, _vp],
    "gr_invert_distortion_f64": [_vp, _f64p, _i32, _i32, _f64, _i32, _f64, _vp, _vp, _vp],
    "gr_resize_image_f64": [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp],
    "gr_equirect_view": [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _f64p, _i32, _i32, _i32, _i32, _f64, _f64, _vp, _vp, _vp,
                         _vp, _vp],
    "gr_finalize_votes": [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp],
    "gr_finalize_sums_f64": [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp],
    "gr_argmax_nonzero": [_vp, _vp, _i32, _i64, _i32, _vp, _vp],
    "gr_argmax_nonzero_f64": [_vp, _vp, _i64, _i32, _vp, _vp],
    "gr_polygon_class_weights": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp],
    "gr_face_polygon_index": [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _i32, _i32,
                              _vp, _vp, _i64, _vp, _vp, _vp],
    "gr_points_in_region": [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp],
    "gr_submesh_extract": [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "gr_class_outlines": [_vp, _vp, _i64, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _i64, _i64p, _i64p, _vp, _vp],
    "gr_sample_raster": [_vp, _vp, _i64, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _f64, _f64, _vp, _vp, _vp, _f64, _f64,
                         _i32, _vp, _vp],
    "gr_set_cover": [_vp, _vp, _vp, _i64, _i64, ctypes.c_int32, _f64, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "gr_reproject_points": [_vp, _vp, _i64, _vp, _i64, _vp, ctypes.POINTER(Crs), ctypes.POINTER(Crs), _vp, _vp, _vp],
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)
# ... and every symbol a companion header declares (include/geograster_outlines.h, which geograster.h includes): the same contract,
# checked by the tests of the calls themselves.
_COMPANION_SIGNATURES = {
    "gr_member_outlines": [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i64, _i64p, _i64p, _vp, _vp],
}
COMPANION_SYMBOLS = tuple(_COMPANION_SIGNATURES)
# ... and the calls of include/geograster_ortho.h (the orthomosaic baseline), under the same contract.
_ORTHO_SIGNATURES = {
    "gr_assemble_tiles": [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i32, _i32, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i64,
                          _i32, _i32, _i32, _vp, _vp, _vp, _vp],
    "gr_zonal_class_counts": [_vp, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _i64, _i64, _vp, _i64, _i32, _vp, _vp, _vp],
}
ORTHO_SYMBOLS = tuple(_ORTHO_SIGNATURES)
# ... and the calls of include/geograster_decimate.h (mesh decimation by vertex clustering), under the same contract.
_DECIMATE_SIGNATURES = {
    "gr_cluster_count": [_vp, _vp, _i64, _i64, _vp, _vp],
    "gr_cluster_decimate": [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
}
DECIMATE_SYMBOLS = tuple(_DECIMATE_SIGNATURES)
# ... and the call of include/geograster_burn.h (polygon rows burned into a label raster), under the same contract.
_BURN_SIGNATURES = {
    "gr_burn_polygons": [_vp, _vp, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
}
BURN_SYMBOLS = tuple(_BURN_SIGNATURES)
# ... and the calls of include/geograster_overlap.h (polygon-on-polygon overlap areas), under the same contract.
_OVERLAP_TABLE = [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64]   # one ring table: vertices, their number, offsets, polygons, holes, R, boxes, P
_OVERLAP_SIGNATURES = {
    "gr_polygon_box_pairs_count": [_vp, _vp, _i64, _vp, _i64, _vp, _vp],
    "gr_polygon_box_pairs_fill": [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp],
    "gr_polygon_overlap_areas": [_vp, *_OVERLAP_TABLE, *_OVERLAP_TABLE, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp],
}
OVERLAP_SYMBOLS = tuple(_OVERLAP_SIGNATURES)
# ... and the calls of include/geograster_communities.h (communities of the ray graph), under the same contract.
_COMMUNITIES_SIGNATURES = {
    "gr_louvain_communities": [_vp, _vp, _vp, _vp, _i64, _i64, _f64, ctypes.c_int32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "gr_community_points": [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp],
}
COMMUNITIES_SYMBOLS = tuple(_COMMUNITIES_SIGNATURES)
# ... and the call of include/geograster_simplify.h (exact Douglas-Peucker on polygon rings), under the same contract.
_SIMPLIFY_SIGNATURES = {
    "gr_simplify_rings": [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp],
}
SIMPLIFY_SYMBOLS = tuple(_SIMPLIFY_SIGNATURES)
# ... and the call of include/geograster_nadir.h (the top-down raster of a mesh), under the same contract.
_NADIR_SIGNATURES = {
    "gr_nadir_raster": [_vp, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
}
NADIR_SYMBOLS = tuple(_NADIR_SIGNATURES)


# ... and the two picture calls of include/geograster_vis.h, each of which takes ONE descriptor in host memory, the stream a field
# of it (tests/test_vis_host.py compares the two mirrors with the header field by field).
class ShadeArgs(ctypes.Structure):
    """gr_shade_args"""
    _fields_ = [
        ("ids", _vp), ("depth", _vp), ("face_rgb", _vp), ("face_light", _vp), ("verts", _vp), ("faces", _vp), ("out", _vp),
        ("stream", _vp),
        ("F", ctypes.c_int64), ("V", ctypes.c_int64),
        ("dir_x", ctypes.c_double), ("dir_y", ctypes.c_double), ("dir_z", ctypes.c_double), ("ambient", ctypes.c_double),
        ("strength", ctypes.c_float),
        ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("supersample", ctypes.c_int32), ("radius", ctypes.c_int32),
        ("bg_r", ctypes.c_int32), ("bg_g", ctypes.c_int32), ("bg_b", ctypes.c_int32),
    ]


class CompositeArgs(ctypes.Structure):
    """gr_composite_args"""
    _fields_ = [
        ("photo", _vp), ("label", _vp), ("table", _vp), ("out", _vp), ("stream", _vp),
        ("shift", ctypes.c_double), ("scale", ctypes.c_double), ("weight", ctypes.c_double),
        ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("table_rows", ctypes.c_int32), ("photo_dtype", ctypes.c_int32),
        ("label_dtype", ctypes.c_int32), ("label_channels", ctypes.c_int32), ("discrete", ctypes.c_int32),
        ("grey_overlay", ctypes.c_int32),
    ]


_VIS_SIGNATURES = {
    "gr_shade_view": [_vp, ctypes.POINTER(ShadeArgs)],
    "gr_composite_labels": [_vp, ctypes.POINTER(CompositeArgs)],
}
VIS_SYMBOLS = tuple(_VIS_SIGNATURES)
SHADE_MAX_SUPERSAMPLE = 4     # V1: the ranges gr_shade_view takes
SHADE_MAX_RADIUS = 16
SHADE_MAX_SIDE = 32768


# ... and the raster -> raster call of include/geograster_warp.h, under the same rule: ONE descriptor in host memory, the stream a field
# of it (tests/test_raster_warp_host.py compares the mirror with the header field by field).
class WarpRasterArgs(ctypes.Structure):
    """gr_warp_raster_args"""
    _fields_ = [
        ("data", _vp), ("out", _vp), ("stats", _vp), ("stream", _vp), ("src_inverse6_h", _vp), ("dst_transform6_h", _vp),
        ("src_crs_h", _vp), ("dst_crs_h", _vp),
        ("src_nodata", ctypes.c_double), ("dst_nodata", ctypes.c_double),
        ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("src_dtype", ctypes.c_int32), ("dst_dtype", ctypes.c_int32),
        ("has_src_nodata", ctypes.c_int32), ("col_off", ctypes.c_int32), ("row_off", ctypes.c_int32), ("width", ctypes.c_int32),
        ("height", ctypes.c_int32), ("resampling", ctypes.c_int32), ("same_crs", ctypes.c_int32),
    ]


_WARP_SIGNATURES = {
    "gr_warp_raster": [_vp, ctypes.POINTER(WarpRasterArgs)],
}
WARP_SYMBOLS = tuple(_WARP_SIGNATURES)
WARP_SIDE_LIMIT = 1 << 23     # W1: H, W of the source stay below it
WARP_RESAMPLING = {"nearest": GR_WARP_NEAREST, "bilinear": GR_WARP_BILINEAR}
WARP_STAT_NAMES = ("cells", "outside", "nonfinite", "beyond", "nodata", "den_zero")


# ... and the face-sieve call of include/geograster_components.h, under the same rule (tests/test_face_sieve_host.py compares the
# mirror with the header field by field).
class FaceSieveArgs(ctypes.Structure):
    """gr_face_sieve_args"""
    _fields_ = [
        ("faces", _vp), ("face_class", _vp), ("weights", _vp), ("vertex_canon", _vp), ("class_out", _vp), ("comp", _vp), ("stats", _vp),
        ("stream", _vp),
        ("F", ctypes.c_int64), ("V", ctypes.c_int64), ("min_measure", ctypes.c_int64),
        ("has_canon", ctypes.c_int32), ("fill_unlabelled", ctypes.c_int32), ("max_rounds", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


_COMPONENTS_SIGNATURES = {
    "gr_face_sieve": [_vp, ctypes.POINTER(FaceSieveArgs)],
}
COMPONENTS_SYMBOLS = tuple(_COMPONENTS_SIGNATURES)
SIEVE_SIZE_LIMIT = 2 ** 31 - 1      # F, V below it; 3 F at or below it
SIEVE_MEASURE_LIMIT = 2 ** 62       # I5: the sum of all weights stays below it
SIEVE_STAT_NAMES = ("rounds", "components_before", "components_after", "faces_changed", "small_left", "degenerate", "fan_edges",
                    "round_cap", "bad_faces")


# ... and the nearest-point call of include/geograster_nearest.h, under the same rule (tests/test_nearest_points_host.py compares
# the mirror with the header field by field).
class NearestArgs(ctypes.Structure):
    """gr_nearest_args"""
    _fields_ = [
        ("ref", _vp), ("query", _vp), ("index_out", _vp), ("dist2_out", _vp), ("stats", _vp), ("stream", _vp),
        ("R", ctypes.c_int64), ("Q", ctypes.c_int64), ("cell", ctypes.c_double), ("max_distance", ctypes.c_double),
        ("max_rings", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


_NEAREST_SIGNATURES = {
    "gr_nearest_points": [_vp, ctypes.POINTER(NearestArgs)],
}
NEAREST_SYMBOLS = tuple(_NEAREST_SIGNATURES)
NEAREST_SIZE_LIMIT = 2 ** 31 - 1      # R, Q below it
NEAREST_STAT_NAMES = ("ref_nonfinite", "query_nonfinite", "no_answer", "levels", "carried", "cells_probed", "candidates", "cell_bits",
                      "ring_cap")


def library_path() -> Path:
    return _LIB_PATH


def load_library() -> ctypes.CDLL:
    """Load libgeograster.so (built in-tree by `__graft_entry__.build()` / `geograypher_amd.build`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.is_file():
        raise RuntimeError(
            f"HIP extension missing: {_LIB_PATH} not found. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
            "geograypher_amd has no CPU fallback for the projection path."
        )
    # PyTorch-ROCm ships its own HIP runtime.  It has to be in the process BEFORE this library pulls in the system's: with the
    # library loaded first (e.g. __graft_entry__.build() and smoke() in one process) the later `import torch` leaves the
    # library's runtime without devices and gr_ctx_create answers GR_ENODEVICE.
    _torch()
    lib = ctypes.CDLL(str(_LIB_PATH))
    for name, argtypes in {**_SIGNATURES, **_COMPANION_SIGNATURES, **_ORTHO_SIGNATURES, **_DECIMATE_SIGNATURES, **_BURN_SIGNATURES,
                           **_OVERLAP_SIGNATURES, **_COMMUNITIES_SIGNATURES, **_SIMPLIFY_SIGNATURES, **_NADIR_SIGNATURES,
                           **_VIS_SIGNATURES, **_WARP_SIGNATURES, **_COMPONENTS_SIGNATURES, **_NEAREST_SIGNATURES}.items():
        fn = getattr(lib, name)
        fn.restype = ctypes.c_char_p if name == "gr_last_error" else _i32
        fn.argtypes = argtypes
    _lib = lib
    _attach_learned_cache(lib)
    return lib


def _attach_learned_cache(lib):
    """What overflowed raster calls taught the library (slots per tile, entry form per mesh and image size) is kept under
    the reference's CACHE_FOLDER (constants.py:18, the default of pix2face's `cache_folder`), so that a new process starts
    with bins that fit.  GEOGRAYPHER_AMD_CACHE=<dir> moves the file, GEOGRAYPHER_AMD_CACHE=off switches persistence off."""
    from geograypher_amd.constants import CACHE_FOLDER

    where = _os.environ.get("GEOGRAYPHER_AMD_CACHE", str(CACHE_FOLDER))
    if where.lower() in ("off", "0", ""):
        return
    try:
        Path(where).mkdir(parents=True, exist_ok=True)
        lib.gr_learned_cache_file(str(Path(where, "geograster_learned.txt")).encode())
    except OSError:
        pass  # a read-only home: learn per process, as before


def _torch():
    import torch

    return torch


class _StatsAccumulator:
    """Statistics of a checked raster call over its attempts: an attempt that overflowed contributes the views it
    completed (records and entries are summed over the views a call processed, so they are scaled by the completed share);
    `max_entries` is the largest per-tile (single-pass) or per-view (exact binning) count any attempt saw;
    `overflow_causes` the OR of every attempt's causes (GR_CAUSE_*)."""

    def __init__(self):
        self.records = 0.0
        self.entries = 0.0
        self.blocks = 0.0
        self.chunk_visits = 0.0
        self.max_entries = 0
        self.views = 0
        self.rebinned = 0
        self.causes = 0
        self.last = None

    def add(self, st: "RasterStats", n_views: int, partial: bool, causes: int = 0):
        done = int(st.views_done) if partial else n_views
        share = done / max(n_views, 1)
        self.records += st.records * share
        self.entries += st.entries * share
        self.blocks += st.blocks * share
        self.chunk_visits += st.chunk_visits * share
        self.max_entries = max(self.max_entries, int(st.max_entries))
        self.views += done
        self.rebinned += int(st.rebinned_groups)
        self.causes |= int(causes)
        self.last = st

    def result(self) -> dict:
        d = self.last.as_dict()
        d.update(records=int(round(self.records)), entries=int(round(self.entries)), max_entries=self.max_entries,
                 views_done=self.views, blocks=int(round(self.blocks)), chunk_visits=int(round(self.chunk_visits)),
                 rebinned_groups=self.rebinned, overflow_causes=self.causes)
        return d


def _flags(neg1_is_last_face: bool) -> int:
    return GR_FLAG_NEG1_IS_LAST_FACE if neg1_is_last_face else 0


def _require_gpu():
    if not _torch().cuda.is_available():
        raise RuntimeError(
            "geograypher_amd: no ROCm GPU visible (torch.cuda.is_available() is False). "
            "The projection path runs on MI355X only; there is no CPU fallback."
        )


def _ptr(t):
    """The device address of a tensor; None (a null pointer) for None."""
    return None if t is None else t.data_ptr()


def _float_kind(array):
    """float32 stays float32, everything else becomes float64: (the array, the name of that dtype, its GR_DTYPE_*).  A numpy
    array of another dtype is converted here, on the host (exact for the integer dtypes of a DTM or a vote array); a tensor is
    returned as it is, for `_dev` to convert."""
    if not isinstance(array, _torch().Tensor):
        array = np.asarray(array)
        if array.dtype != np.float32:
            array = array.astype(np.float64, copy=False)
    if str(array.dtype).endswith("float32"):
        return array, "float32", GR_DTYPE_F32
    return array, "float64", GR_DTYPE_F64


def _count_then_fill(name: str, attempt, cap: int, something_to_fill, check):
    """The count-then-fill protocol of gr_ray_pairs and gr_class_outlines over `attempt(cap) -> (rc, total, result)`: the
    library reports the total whatever room it was offered, so a first attempt that overflowed (GR_EOVERFLOW), or that offered
    none (cap 0) where `something_to_fill(total)`, is repeated exactly once, at max(total, 1), where it fits.  Every other code
    goes to `check(rc, name)` at once.  -> (the result of the attempt that fitted, the number of attempts)."""
    for attempts in (1, 2):
        rc, total, result = attempt(cap)
        if rc != GR_EOVERFLOW and not (rc == GR_OK and cap == 0 and something_to_fill(total)):
            check(rc, name)
            return result, attempts
        cap = max(int(total), 1)   # the library counted everything: the repeat fits exactly
    check(rc, name)
    raise RuntimeError(f"{name} reported two different totals for the same input")


POLYGON_RING_CHUNK = 512  # ring records per LDS chunk of gr_project_polygon_pairs (PAIR_CHUNK, csrc/project.hip)


# A ring table on the device (`HipRaster._ring_table`): tensors, `box` and `rh` None where the call takes none, and the counts.
RingTable = namedtuple("RingTable", "rv off rp box rh N R P")


# The checks of the tables `PairAccumulator` takes: plain functions of host arrays (no device, no library).
def _host_array(a) -> np.ndarray:
    """tensor or array -> host array"""
    return np.asarray(a.cpu() if isinstance(a, _torch().Tensor) else a)


def _check_offsets(offsets, n: int, total: int, owners: str, kind: str, rows: str, at_least_one: Optional[str] = None):
    """An offsets table over `n` owners (views, rings) of `total` rows (rectangles, rings, vertices): n + 1 entries that
    rise from 0 to total; with `at_least_one`, every owner has a row."""
    if offsets.shape[0] != n + 1:
        raise ValueError(f"{n} {owners} need {n + 1} {kind} offsets, got {offsets.shape[0]}")
    if offsets[0] != 0 or offsets[-1] != total or np.any(np.diff(offsets) < (1 if at_least_one else 0)):
        raise ValueError(f"{kind} offsets must rise from 0 to {total} (the number of {rows})"
                         + (f", at least one {at_least_one}" if at_least_one else ""))


def _check_int32(table, what: str):
    if table.size and (table.min() < np.iinfo(np.int32).min or table.max() > np.iinfo(np.int32).max):
        raise ValueError(f"{what} must fit in int32")


# The checks of the tables of the orthomosaic baseline: plain functions of host arrays.
def _count_kind(count_dtype):
    """np.uint8 / np.uint16 / float (or np.float64) -> (GR_COUNT_*, the numpy dtype, the torch dtype)."""
    torch = _torch()
    if count_dtype is float:
        count_dtype = np.float64
    try:
        dtype = np.dtype(count_dtype)
    except TypeError:
        dtype = None
    kinds = {np.dtype(np.uint8): (GR_COUNT_U8, torch.uint8), np.dtype(np.uint16): (GR_COUNT_U16, torch.uint16),
             np.dtype(np.float64): (GR_COUNT_F64, torch.float64)}
    if dtype not in kinds:
        raise ValueError(f"gr_assemble_tiles: count_dtype must be np.uint8, np.uint16 or float, got {count_dtype!r}")
    return kinds[dtype][0], dtype, kinds[dtype][1]


def check_assemble_tables(pred_offsets, windows, tile_table, weight_offsets, n_pred_bytes: int, n_weights: int, bin_ptr, bin_tiles,
                          bin_side: int, bins_x: int, bins_y: int, width: int, height: int, row0: int, n_rows: int, num_classes: int,
                          nodataval: int):
    """O8: everything gr_assemble_tiles reads through is in range -- ValueError naming the call otherwise."""
    name = "gr_assemble_tiles"
    if not 1 <= num_classes <= GR_ORTHO_MAX_CLASSES:
        raise ValueError(f"{name}: num_classes={num_classes} outside [1, {GR_ORTHO_MAX_CLASSES}]")
    if not 0 <= nodataval <= 255:
        raise ValueError(f"{name}: nodataval={nodataval} outside [0, 255]")
    if width < 0 or height < 0 or row0 < 0 or n_rows < 0 or row0 + n_rows > height or width >= 2 ** 31 or height >= 2 ** 31:
        raise ValueError(f"{name}: rows [{row0}, {row0 + n_rows}) of an extent of {height} rows x {width} columns")
    windows = np.asarray(windows, dtype=np.int64)
    tile_table = np.asarray(tile_table, dtype=np.int64).reshape(-1)
    pred_offsets = np.asarray(pred_offsets, dtype=np.int64).reshape(-1)
    weight_offsets = np.asarray(weight_offsets, dtype=np.int64).reshape(-1)
    T = tile_table.shape[0]
    if windows.shape != (T, 4):
        raise ValueError(f"{name}: {T} tiles need windows of shape ({T}, 4), got {windows.shape}")
    if weight_offsets.shape[0] < 1:
        raise ValueError(f"{name}: the weight offsets need at least one entry")
    _check_offsets(pred_offsets, T, n_pred_bytes, "tiles", f"{name}: prediction", "prediction bytes")
    n_tables = weight_offsets.shape[0] - 1
    _check_offsets(weight_offsets, n_tables, n_weights, "weight tables", f"{name}: weight", "weights")
    if T:
        col, row, w, h = windows.T
        if np.any(w < 1) or np.any(h < 1) or np.any(col < 0) or np.any(row < 0) or np.any(col + w > width) or np.any(row + h > height):
            bad = int(np.nonzero((w < 1) | (h < 1) | (col < 0) | (row < 0) | (col + w > width) | (row + h > height))[0][0])
            raise ValueError(f"{name}: window {bad} {tuple(int(v) for v in windows[bad])} is empty or leaves the {height} x {width} extent")
        if np.any(np.diff(pred_offsets) != w * h):
            bad = int(np.nonzero(np.diff(pred_offsets) != w * h)[0][0])
            raise ValueError(f"{name}: tile {bad} has {int(np.diff(pred_offsets)[bad])} prediction bytes for a window of {int(h[bad])} x {int(w[bad])}")
        if np.any(tile_table < 0) or np.any(tile_table >= n_tables):
            raise ValueError(f"{name}: a tile names a weight table outside [0, {n_tables})")
        if np.any(np.diff(weight_offsets)[tile_table] != w * h):
            bad = int(np.nonzero(np.diff(weight_offsets)[tile_table] != w * h)[0][0])
            raise ValueError(f"{name}: the weight table of tile {bad} does not have the {int(h[bad])} x {int(w[bad])} values of its window")
    if bin_side < 1 or bins_x < 1 or bins_y < 1 or bins_x * bin_side < width or bins_y * bin_side < height:
        raise ValueError(f"{name}: {bins_x} x {bins_y} bins of side {bin_side} do not cover the {height} x {width} extent")
    bin_ptr = np.asarray(bin_ptr, dtype=np.int64).reshape(-1)
    bin_tiles = np.asarray(bin_tiles, dtype=np.int64).reshape(-1)
    _check_offsets(bin_ptr, bins_x * bins_y, bin_tiles.shape[0], "bins", f"{name}: bin", "bin entries")
    if bin_tiles.size:
        if bin_tiles.min() < 0 or bin_tiles.max() >= T:
            raise ValueError(f"{name}: a bin entry is outside [0, {T})")
        rising = np.diff(bin_tiles) > 0
        rising[bin_ptr[1:-1][(bin_ptr[1:-1] > 0) & (bin_ptr[1:-1] < bin_tiles.shape[0])] - 1] = True   # across two bins: any order
        if not np.all(rising):
            raise ValueError(f"{name}: the tiles of a bin must be listed in strictly ascending index")


def zonal_nodata(nodata) -> int:
    """Z5: the nodata argument of gr_zonal_class_counts -- the value, or -1 (no cell is nodata) for None and for a value that no
    uint8 cell can hold."""
    if nodata is None or not np.isfinite(nodata) or nodata != int(nodata) or not 0 <= int(nodata) <= 255:
        return -1
    return int(nodata)


def check_zonal_tables(H: int, W: int, nodata, ring_vertices, ring_offsets, ring_polygon, n_polygons: int, items, num_classes: int):
    """Z1 / Z6: everything gr_zonal_class_counts reads through is in range -- ValueError naming the call otherwise."""
    name = "gr_zonal_class_counts"
    if not (1 <= H < 2 ** 23 and 1 <= W < 2 ** 23):
        raise ValueError(f"{name}: a raster of {H} x {W} cells is outside [1, 2^23) a side")
    if not 1 <= num_classes <= GR_ZONAL_MAX_CLASSES:
        raise ValueError(f"{name}: num_classes={num_classes} outside [1, {GR_ZONAL_MAX_CLASSES}]")
    _, R = _check_ring_table(name, ring_vertices, ring_offsets, ring_polygon, n_polygons)
    _check_cell_items(name, items, n_polygons, R, (0, 0, W, H), "raster")


BURN_WINDOW_LIMIT = 1 << 23   # B1: |offsets| of a burn window stay below it, its far edges at or below it


def _check_ring_table(name: str, ring_vertices, ring_offsets, ring_polygon, n_polygons: int, side: Optional[str] = None,
                      inclusive: bool = False):
    """What every ring table holds (Z1, B1, A1, S1) -- ValueError naming the call and the table's `side`, if any; -> (N, R).
    (N, 2) integer vertices with |coordinate| below 2^40 (cell units) or, `inclusive`, at or below it (the 1e-6 m grid), offsets
    rising from 0 to N, rows non-decreasing in [0, n_polygons) unless `ring_polygon` is None; N, R, P below 2^31."""
    of_table = f" of table {side}" if side else ""
    if not 0 <= n_polygons < 2 ** 31:
        raise ValueError(f"{name}: {n_polygons} polygon rows{of_table}")
    rv = np.asarray(ring_vertices)
    if rv.ndim != 2 or rv.shape[1] != 2 or rv.dtype.kind not in "iu":
        raise ValueError(f"{name}: {'the ring vertices' + of_table if side else 'ring vertices'} must be an (N, 2) integer array, "
                         f"got {rv.shape} {rv.dtype}")
    N = int(rv.shape[0])
    if N >= 2 ** 31:
        raise ValueError(f"{name}: {N} ring vertices{of_table}, not below 2^31")
    if rv.size:
        far = max(int(rv.max()), -int(rv.min()))
        if far > 2 ** 40 and inclusive:
            raise ValueError(f"{name}: a ring vertex{of_table} lies more than 2^40 grid steps from the {'common ' if side else ''}origin")
        if far >= 2 ** 40 and not inclusive:
            raise ValueError(f"{name}: a ring vertex{of_table} lies 2^40 / 65536 cells or more from the raster's corner")
    off = np.asarray(ring_offsets, dtype=np.int64).reshape(-1)
    rp = None if ring_polygon is None else np.asarray(ring_polygon, dtype=np.int64).reshape(-1)
    R = off.shape[0] - 1 if rp is None else rp.shape[0]
    _check_offsets(off, R, N, "rings", f"{name}: table {side}: ring" if side else f"{name}: ring", "ring vertices")
    if rp is not None and R and (rp.min() < 0 or rp.max() >= n_polygons or np.any(np.diff(rp) < 0)):
        raise ValueError(f"{name}: {'the ring_polygon' + of_table if side else 'ring_polygon'} must be non-decreasing inside [0, {n_polygons})")
    return N, R


def _check_window(name: str, col_off: int, row_off: int, width: int, height: int):
    """B1: a window of a cell grid is not empty and stays inside (-2^23, 2^23] -- ValueError naming the call."""
    lim = BURN_WINDOW_LIMIT
    if not (width >= 1 and height >= 1 and -lim < col_off < lim and -lim < row_off < lim and col_off + width <= lim and row_off + height <= lim):
        raise ValueError(f"{name}: a window of {width} x {height} cells at ({col_off}, {row_off}) is empty or leaves (-2^23, 2^23]")


def _check_cell_items(name: str, items, n_polygons: int, n_rings: int, window, inside: str):
    """Z6 / B5 / B7: every work item names a row, a block of at most GR_ZONAL_BLOCK_W x GR_ZONAL_BLOCK_H cells inside `window`
    (col_off, row_off, width, height; `inside` is its word in the message) and a ring range -- ValueError naming the call."""
    col_off, row_off, width, height = window
    it = np.asarray(items)
    if it.ndim != 2 or it.shape[1] != GR_ZONAL_ITEM_INTS or it.dtype.kind not in "iu":
        raise ValueError(f"{name}: work items must be (n, {GR_ZONAL_ITEM_INTS}) integers, got {it.shape} {it.dtype}")
    if it.shape[0]:
        p, c0, r0, w, h, lo, hi = it.astype(np.int64).T
        bad = ((p < 0) | (p >= n_polygons) | (w < 1) | (h < 1) | (w > GR_ZONAL_BLOCK_W) | (h > GR_ZONAL_BLOCK_H) | (c0 < col_off) | (r0 < row_off)
               | (c0 + w > col_off + width) | (r0 + h > row_off + height) | (lo < 0) | (hi < lo) | (hi > n_rings))
        if np.any(bad):
            k = int(np.nonzero(bad)[0][0])
            raise ValueError(f"{name}: work item {k} {tuple(int(v) for v in it[k])} names no polygon row, no block of at most "
                             f"{GR_ZONAL_BLOCK_W} x {GR_ZONAL_BLOCK_H} cells inside the {inside}, or no ring range")


def check_burn_tables(ring_vertices, ring_offsets, ring_polygon, n_polygons: int, values=None):
    """B1 / B7: the ring table and the values of a `PolygonBurner` are in range -- ValueError naming gr_burn_polygons; -> R."""
    name = "gr_burn_polygons"
    _, R = _check_ring_table(name, ring_vertices, ring_offsets, ring_polygon, int(n_polygons))
    if values is not None:
        v = np.asarray(values)
        if v.shape != (int(n_polygons),) or v.dtype.kind not in "iu" or (v.size and (v.min() < 0 or v.max() > 255)):
            raise ValueError(f"{name}: values must be ({int(n_polygons)},) integers in [0, 255], got {v.shape} {v.dtype}")
    return R


def check_burn_window(col_off: int, row_off: int, width: int, height: int, items, n_polygons: int, n_rings: int, fill: int = 255):
    """B1 / B5 / B7: the window is inside the bounds and every work item inside the window -- ValueError naming gr_burn_polygons."""
    name = "gr_burn_polygons"
    _check_window(name, col_off, row_off, width, height)
    if not 0 <= fill <= 255:
        raise ValueError(f"{name}: fill={fill} outside [0, 255]")
    _check_cell_items(name, items, n_polygons, n_rings, (col_off, row_off, width, height), "window")


class PolygonBurner:
    """One ring table on the device, burned into any number of windows of its parent grid (gr_burn_polygons).
    Made by `HipRaster.polygon_burner`, which checks the tables (`check_burn_tables`) and uploads them once."""

    def __init__(self, backend: "HipRaster", ring_vertices, ring_offsets, ring_polygon, n_polygons: int, values=None):
        rv_h, off_h, rp_h = (_host_array(x) for x in (ring_vertices, ring_offsets, ring_polygon))
        val_h = None if values is None else _host_array(values)
        self.backend = backend
        self.n_polygons = int(n_polygons)
        self.n_rings = check_burn_tables(rv_h, off_h, rp_h, self.n_polygons, val_h)
        self._rv, self._off, self._rp = backend._ring_table(ring_vertices, ring_offsets, ring_polygon, n_polygons=self.n_polygons)[:3]
        self._values = None if values is None else backend._dev(values, _torch().uint8).reshape(-1)

    def window(self, col_off: int, row_off: int, width: int, height: int, items, fill: int = 255, want_values: bool = True):
        """The window (col_off, row_off, width, height) of the parent grid; items (n, GR_ZONAL_ITEM_INTS) int32 of
        `utils.geometric.burn_work_items` for that window -> (rows (height, width) int32 tensor: the highest row that holds the
        cell's centre, -1 for none; out (height, width) uint8 tensor = values[rows], `fill` where none, or None without
        `want_values`; stats (GR_BURN_STAT_WORDS,) int64 tensor).  The items are validated on the host first (`check_burn_window`:
        ValueError).  Only enqueues."""
        torch = _torch()
        hip = self.backend
        col_off, row_off, width, height, fill = int(col_off), int(row_off), int(width), int(height), int(fill)
        check_burn_window(col_off, row_off, width, height, _host_array(items), self.n_polygons, self.n_rings, fill)
        if want_values and self._values is None:
            raise ValueError("gr_burn_polygons: this burner was made without values; ask for the rows alone (want_values=False)")
        it_t = hip._shaped(items, torch.int32, ("n", GR_ZONAL_ITEM_INTS), "work items")
        rows = hip._empty((height, width), torch.int32)
        out = hip._empty((height, width), torch.uint8) if want_values else None
        stats = hip._stats(GR_BURN_STAT_WORDS)
        hip._call("gr_burn_polygons", _ptr(self._rv if self._rv.numel() else None), int(self._rv.shape[0]), self._off.data_ptr(),
                  _ptr(self._rp if self.n_rings else None), self.n_rings, self.n_polygons,
                  _ptr(self._values if want_values and self.n_polygons else None), _ptr(it_t if it_t.numel() else None),
                  int(it_t.shape[0]), col_off, row_off, width, height, fill, rows.data_ptr(), _ptr(out), stats.data_ptr(), hip._stream())
        return rows, out, stats


OVERLAP_COORD_LIMIT = 1 << 40   # A1: |snapped coordinate| behind the common origin (utils.geometric.SNAP_LIMIT)


def _check_overlap_table(name: str, side: str, table) -> int:
    """A1 for one ring table (ring vertices, ring offsets, ring polygon, ring is hole, polygon boxes) -- ValueError naming the call; -> R."""
    if len(table) != 5:
        raise ValueError(f"{name}: table {side} must be (ring vertices, ring offsets, ring polygon, ring is hole, polygon boxes)")
    rv, off, rp, rh, box = (np.asarray(x) for x in table)
    if box.ndim != 2 or box.shape[1] != 4 or box.dtype.kind not in "iu":
        raise ValueError(f"{name}: the polygon boxes of table {side} must be a (P, 4) integer array, got {box.shape} {box.dtype}")
    P = box.shape[0]
    if P >= 2 ** 31 - 1:
        raise ValueError(f"{name}: table {side} has {P} polygon rows")
    _, R = _check_ring_table(name, rv, off, rp, P, side, inclusive=True)
    if box.size and np.abs(box.astype(np.int64)).max() > OVERLAP_COORD_LIMIT:
        raise ValueError(f"{name}: a polygon box of table {side} lies more than 2^40 grid steps from the common origin")
    if rh.reshape(-1).shape[0] != R or rh.dtype.kind not in "iub":
        raise ValueError(f"{name}: table {side} needs one integer hole flag per ring, got {rh.shape} {rh.dtype}")
    if rv.shape[0]:   # A3: the box of a row holds every vertex of the row (the baseline Y lies at or below both rows)
        row = np.repeat(rp.astype(np.int64).reshape(-1), np.diff(np.asarray(off, dtype=np.int64).reshape(-1)))
        b = box.astype(np.int64)[row]
        q = rv.astype(np.int64)
        if np.any((q[:, 0] < b[:, 0]) | (q[:, 1] < b[:, 1]) | (q[:, 0] > b[:, 2]) | (q[:, 1] > b[:, 3])):
            raise ValueError(f"{name}: a polygon box of table {side} does not hold every ring vertex of its row")
    return R


def check_overlap_tables(table_a, table_b):
    """A1: the two ring tables of a `PolygonOverlap`, each (ring vertices (N, 2), ring offsets (R + 1,), ring polygon (R,), ring is
    hole (R,), polygon boxes (P, 4)) as `PlanarPolygons.snapped` gives them behind ONE origin, are in range -- ValueError naming
    gr_polygon_overlap_areas; -> (R_a, R_b)."""
    name = "gr_polygon_overlap_areas"
    return _check_overlap_table(name, "a", table_a), _check_overlap_table(name, "b", table_b)


def _row_slot_ranges(ring_offsets, ring_polygon, n_polygons: int) -> np.ndarray:
    """(P, 2) int64: the first edge slot (= ring vertex) of every row and one past its last."""
    off = np.asarray(ring_offsets, dtype=np.int64).reshape(-1)
    rp = np.asarray(ring_polygon, dtype=np.int64).reshape(-1)
    rows = np.arange(int(n_polygons))
    return np.stack([off[np.searchsorted(rp, rows, "left")], off[np.searchsorted(rp, rows, "right")]], axis=1)


def check_overlap_items(pairs, items, offsets_a, rows_a, n_a: int, offsets_b, rows_b, n_b: int):
    """A8: the pairs name rows of both tables, and every work item names a pair -- the pairs in non-decreasing order --, 1 ..
    GR_OVERLAP_TILE_A consecutive edge slots of the pair's row of a and 1 .. GR_OVERLAP_TILE_B of its row of b -- ValueError naming
    gr_polygon_overlap_areas."""
    name = "gr_polygon_overlap_areas"
    pr = np.asarray(pairs)
    if pr.ndim != 2 or pr.shape[1] != 2 or pr.dtype.kind not in "iu":
        raise ValueError(f"{name}: pairs must be (n, 2) integers, got {pr.shape} {pr.dtype}")
    if pr.shape[0] >= 2 ** 31:
        raise ValueError(f"{name}: {pr.shape[0]} pairs, not below 2^31")
    pr = pr.astype(np.int64)
    if pr.shape[0] and (pr.min() < 0 or pr[:, 0].max() >= n_a or pr[:, 1].max() >= n_b):
        k = int(np.nonzero((pr[:, 0] < 0) | (pr[:, 0] >= n_a) | (pr[:, 1] < 0) | (pr[:, 1] >= n_b))[0][0])
        raise ValueError(f"{name}: pair {k} {tuple(int(v) for v in pr[k])} names no row of the {n_a} x {n_b} tables")
    it = np.asarray(items)
    if it.ndim != 2 or it.shape[1] != GR_OVERLAP_ITEM_INTS or it.dtype.kind not in "iu":
        raise ValueError(f"{name}: work items must be (n, {GR_OVERLAP_ITEM_INTS}) integers, got {it.shape} {it.dtype}")
    if it.shape[0] >= 2 ** 31:
        raise ValueError(f"{name}: {it.shape[0]} work items, not below 2^31")
    if not it.shape[0]:
        return
    p, a0, na, b0, nb = it.astype(np.int64).T
    bad = (p < 0) | (p >= pr.shape[0]) | (na < 1) | (na > GR_OVERLAP_TILE_A) | (nb < 1) | (nb > GR_OVERLAP_TILE_B)
    bad[1:] |= p[1:] < np.maximum.accumulate(p)[:-1]
    ok = np.nonzero(~bad)[0]
    ra, rb = _row_slot_ranges(offsets_a, rows_a, n_a)[pr[p[ok], 0]], _row_slot_ranges(offsets_b, rows_b, n_b)[pr[p[ok], 1]]
    bad[ok] = (a0[ok] < ra[:, 0]) | (a0[ok] + na[ok] > ra[:, 1]) | (b0[ok] < rb[:, 0]) | (b0[ok] + nb[ok] > rb[:, 1])
    if np.any(bad):
        k = int(np.nonzero(bad)[0][0])
        raise ValueError(f"{name}: work item {k} {tuple(int(v) for v in it[k])} names no pair, a pair below one in front of it, or no tile "
                         f"of at most {GR_OVERLAP_TILE_A} x {GR_OVERLAP_TILE_B} edge slots inside the pair's rows")


class PolygonOverlap:
    """Two ring tables on the device, behind one origin (gr_polygon_box_pairs_count / _fill, gr_polygon_overlap_areas; DESIGN.md 8o,
    A1-A9).  Made by `HipRaster.polygon_overlap`, which checks the tables (`check_overlap_tables`) and uploads them once."""

    def __init__(self, backend: "HipRaster", table_a, table_b):
        host = [[_host_array(x) for x in table] for table in (table_a, table_b)]
        check_overlap_tables(*host)
        self.backend = backend
        self.host = host                      # the host copies the item check walks (offsets and rows)
        self._a = backend._ring_table(table_a[0], table_a[1], table_a[2], table_a[4], table_a[3])
        self._b = backend._ring_table(table_b[0], table_b[1], table_b[2], table_b[4], table_b[3])

    def pairs(self):
        """(n, 2) int32 tensor: the candidate pairs (row of a, row of b) of rule A2, ascending by (a, b).  Reads the count back."""
        torch = _torch()
        hip = self.backend
        box_a, box_b, Pa, Pb = self._a.box, self._b.box, self._a.P, self._b.P
        offsets = hip._empty((Pa + 1,), torch.int64)
        hip._call("gr_polygon_box_pairs_count", _ptr(box_a if Pa else None), Pa, _ptr(box_b if Pb else None), Pb, offsets.data_ptr(),
                  hip._stream())
        n = int(offsets[Pa].item())
        if n >= 2 ** 31:
            raise ValueError(f"gr_polygon_box_pairs_fill: {n} candidate pairs, not below 2^31: split a table")
        pairs = hip._empty((n, 2), torch.int32)
        hip._call("gr_polygon_box_pairs_fill", _ptr(box_a if Pa else None), Pa, _ptr(box_b if Pb else None), Pb, offsets.data_ptr(),
                  _ptr(pairs if n else None), n, hip._stream())
        return pairs

    def areas(self, pairs, items):
        """pairs (n, 2) int32 (row of a, row of b), items (m, GR_OVERLAP_ITEM_INTS) int32 of `utils.geometric.overlap_work_items`
        for those pairs -> (area (n,) float64 tensor in grid steps squared, area_abs (n,) float64 tensor: the sum of the magnitudes
        of the terms, the scale of the bound of A6; stats (GR_OVERLAP_STAT_WORDS,) int64 tensor).  Pairs and items are validated on
        the host first (`check_overlap_items`: ValueError).  Only enqueues."""
        torch = _torch()
        hip = self.backend
        (_, off_a, rp_a, _, _), (_, off_b, rp_b, _, _) = self.host
        check_overlap_items(_host_array(pairs), _host_array(items), off_a, rp_a, self._a.P, off_b, rp_b, self._b.P)
        pr_t = hip._shaped(pairs, torch.int32, ("n", 2), "pairs")
        it_t = hip._shaped(items, torch.int32, ("m", GR_OVERLAP_ITEM_INTS), "work items")
        n = int(pr_t.shape[0])
        area, area_abs = hip._empty((n,), torch.float64), hip._empty((n,), torch.float64)
        stats = hip._stats(GR_OVERLAP_STAT_WORDS)
        hip._call("gr_polygon_overlap_areas", *self._table_args(self._a), *self._table_args(self._b), _ptr(pr_t if n else None), n,
                  _ptr(it_t if it_t.numel() else None), int(it_t.shape[0]), _ptr(area if n else None), _ptr(area_abs if n else None),
                  stats.data_ptr(), hip._stream())
        return area, area_abs, stats

    @staticmethod
    def _table_args(t):
        return (_ptr(t.rv if t.N else None), t.N, t.off.data_ptr(), _ptr(t.rp if t.R else None), _ptr(t.rh if t.R else None), t.R,
                _ptr(t.box if t.P else None), t.P)


SIMPLIFY_COORD_LIMIT = 1 << 40   # S1: |snapped coordinate| <= 2^40 (utils.geometric.SNAP_LIMIT); the tolerance stays below it
SIMPLIFY_GRID = 1e-6             # metres per grid step


def simplify_tol_steps(tol_meters) -> int:
    """S1: the tolerance in grid steps, T = rint(tol_meters / 1e-6) with 0 <= T < 2^40 -- ValueError naming gr_simplify_rings."""
    name = "gr_simplify_rings"
    try:
        tol = float(tol_meters)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: the tolerance must be a number of metres, got {tol_meters!r}") from None
    if not np.isfinite(tol) or tol < 0 or np.rint(tol / SIMPLIFY_GRID) >= SIMPLIFY_COORD_LIMIT:
        raise ValueError(f"{name}: the tolerance must be in [0, 2^40) grid steps of 1e-6 m, got {tol_meters!r} m")
    return int(np.rint(tol / SIMPLIFY_GRID))


def check_simplify_tables(ring_vertices, ring_offsets, tol_meters, fixed=None):
    """S1: the ring table, the fixed flags and the tolerance of `RingSimplifier.simplify` are in range -- ValueError naming
    gr_simplify_rings; -> (N, R, T)."""
    name = "gr_simplify_rings"
    off = np.asarray(ring_offsets)
    if off.ndim != 1 or off.shape[0] < 1 or off.dtype.kind not in "iu":
        raise ValueError(f"{name}: ring offsets must be an (R + 1,) integer array, got {off.shape} {off.dtype}")
    N, R = _check_ring_table(name, ring_vertices, off, None, 0, inclusive=True)
    if N >= 2 ** 31 - 1:
        raise ValueError(f"{name}: {N} ring vertices, not below 2^31 - 1")
    if fixed is not None:
        fx = np.asarray(fixed)
        if fx.shape != (N,) or fx.dtype.kind not in "iub":
            raise ValueError(f"{name}: fixed must be ({N},) flags, one per ring vertex, got {fx.shape} {fx.dtype}")
    return N, R, simplify_tol_steps(tol_meters)


class RingSimplifier:
    """Exact Douglas-Peucker on the rings of a snapped ring table (gr_simplify_rings).  Made by
    `HipRaster.ring_simplifier`.  Every output is allocated through the backend (`_empty`, `_stats`)."""

    def __init__(self, backend: "HipRaster"):
        self.backend = backend

    def simplify(self, ring_vertices, ring_offsets, tol_meters, fixed=None):
        """ring_vertices (N, 2) int64 on the 1e-6 m grid and ring_offsets (R + 1,) as `PlanarPolygons.snapped` gives them,
        tol_meters, fixed (N,) flags or None (S2) -> (keep (N,) uint8 tensor, kept_index (M,) int32 tensor: the kept vertices,
        ring after ring in input order, out_offsets (R + 1,) int64 tensor, stats (GR_SIMPLIFY_STAT_WORDS,) int64 tensor).  The
        tables are validated on the host first (`check_simplify_tables`: ValueError).  Reads M back."""
        torch = _torch()
        hip = self.backend
        N, R, T = check_simplify_tables(_host_array(ring_vertices), _host_array(ring_offsets), tol_meters,
                                        None if fixed is None else _host_array(fixed))
        rv_t = hip._shaped(ring_vertices, torch.int64, (N, 2), "ring vertices")
        off_t = hip._shaped(ring_offsets, torch.int64, (R + 1,), "ring offsets")
        fx_t = None if fixed is None else hip._shaped(fixed, torch.uint8, (N,), "fixed (one per ring vertex)")
        keep = hip._empty((N,), torch.uint8)
        kept_index = hip._empty((N,), torch.int32)
        out_offsets = hip._empty((R + 1,), torch.int64)
        stats = hip._stats(GR_SIMPLIFY_STAT_WORDS)
        hip._call("gr_simplify_rings", _ptr(rv_t if N else None), N, off_t.data_ptr(), R, _ptr(fx_t if N else None), T,
                  _ptr(keep if N else None), _ptr(kept_index if N else None), out_offsets.data_ptr(), stats.data_ptr(), hip._stream())
        M = int(out_offsets[R].item())
        return keep, kept_index[:M], out_offsets, stats


NADIR_COORD_LIMIT = 1 << 40      # N2: |vertex coordinate in 1/65536 of a cell| stays below it
NADIR_SMALL_CELLS_MAX = 65536    # N8: the largest small_cells and item_rows gr_nadir_raster takes (0: its defaults, 256 and 16)
NADIR_ITEM_ROWS_MAX = 1024


def check_nadir_tables(verts_q, z, faces):
    """N1 / N2: the vertex table and the faces of a `NadirRasterizer` are in shape and range -- ValueError naming gr_nadir_raster;
    -> (V, F).  Face indices are not looked at: the kernel counts the faces it refuses (N3) and `window` raises on them."""
    name = "gr_nadir_raster"
    vq, zz, ff = np.asarray(verts_q), np.asarray(z), np.asarray(faces)
    if vq.ndim != 2 or vq.shape[1] != 2 or vq.dtype.kind not in "iu":
        raise ValueError(f"{name}: vertices must be a (V, 2) integer array in 1/65536 of a cell, got {vq.shape} {vq.dtype}")
    V = int(vq.shape[0])
    if zz.shape != (V,) or zz.dtype.kind != "f":
        raise ValueError(f"{name}: z must be ({V},) floats, one per vertex, got {zz.shape} {zz.dtype}")
    if ff.ndim != 2 or ff.shape[1] != 3 or ff.dtype.kind not in "iu":
        raise ValueError(f"{name}: faces must be an (F, 3) integer array, got {ff.shape} {ff.dtype}")
    F = int(ff.shape[0])
    if V >= 2 ** 31 - 1 or F >= 2 ** 31 - 1:
        raise ValueError(f"{name}: {V} vertices and {F} faces, not both below 2^31 - 1")
    if vq.size and np.abs(vq.astype(np.int64)).max() >= NADIR_COORD_LIMIT:
        raise ValueError(f"{name}: a mesh vertex lies 2^40 / 65536 cells or more from the raster's corner")
    return V, F


def check_nadir_window(col_off: int, row_off: int, width: int, height: int, small_cells: int = 0, item_rows: int = 0):
    """N7 / N8: the window is inside B1's bounds, small_cells and item_rows inside theirs -- ValueError naming gr_nadir_raster."""
    name = "gr_nadir_raster"
    _check_window(name, col_off, row_off, width, height)
    if not 0 <= small_cells <= NADIR_SMALL_CELLS_MAX:
        raise ValueError(f"{name}: small_cells={small_cells} outside [0, {NADIR_SMALL_CELLS_MAX}]")
    if not 0 <= item_rows <= NADIR_ITEM_ROWS_MAX:
        raise ValueError(f"{name}: item_rows={item_rows} outside [0, {NADIR_ITEM_ROWS_MAX}]")


WARP_DTYPES = {"uint8": GR_DTYPE_U8, "float32": GR_DTYPE_F32, "float64": GR_DTYPE_F64}   # numpy / torch dtype name -> GR_DTYPE_*


def warp_numpy_dtype(dtype) -> np.dtype:
    """A numpy or torch dtype, or its name -> the numpy dtype, one of uint8, float32, float64 (W1); anything else: ValueError
    naming gr_warp_raster."""
    try:
        name = np.dtype(dtype).name
    except TypeError:
        name = str(dtype).replace("torch.", "")
    if name not in WARP_DTYPES:
        raise ValueError(f"gr_warp_raster: dtype {dtype} is not one of uint8, float32, float64")
    return np.dtype(name)


def warp_dst_nodata(dst_nodata, src_nodata, dst_dtype) -> float:
    """W1: the destination's nodata value: `dst_nodata`, else the source's, else NaN for a float destination and 0 for uint8.
    A uint8 destination needs an integer in [0, 255]: ValueError naming gr_warp_raster."""
    value = dst_nodata if dst_nodata is not None else src_nodata
    if value is None:
        value = 0.0 if np.dtype(dst_dtype) == np.uint8 else float("nan")
    value = float(value)
    if np.dtype(dst_dtype) == np.uint8 and not (0 <= value <= 255 and value == int(value)):
        raise ValueError(f"gr_warp_raster: dst_nodata={value!r} does not fit the uint8 destination (an integer in [0, 255])")
    return value


def check_warp_window(src_shape, col_off: int, row_off: int, width: int, height: int, dst_dtype=None):
    """W1: the source is (B, H, W) with 1 <= B <= GR_WARP_MAX_BANDS and 1 <= H, W < 2^23, the destination window inside B1's
    bounds and of at most 2^31 - 1 (row, 256 column) strips -- ValueError naming gr_warp_raster."""
    name = "gr_warp_raster"
    if len(src_shape) != 3:
        raise ValueError(f"{name}: the source must be (B, H, W) or (H, W), got {tuple(src_shape)}")
    B, H, W = (int(k) for k in src_shape)
    if not (1 <= B <= GR_WARP_MAX_BANDS and 1 <= H < WARP_SIDE_LIMIT and 1 <= W < WARP_SIDE_LIMIT):
        raise ValueError(f"{name}: a source of {B} x {H} x {W} is outside 1 <= B <= {GR_WARP_MAX_BANDS}, 1 <= H, W < 2^23")
    _check_window(name, int(col_off), int(row_off), int(width), int(height))
    if -(-int(width) // 256) * int(height) > 2 ** 31 - 1:
        raise ValueError(f"{name}: a window of {width} x {height} cells is too large for one call")
    if dst_dtype is not None:
        warp_numpy_dtype(dst_dtype)


def check_sieve_arguments(F: int, V: int, weights, min_measure, max_rounds) -> int:
    """The host checks of gr_face_sieve (I1, I5): sizes inside the call's limits, min_measure >= 0, max_rounds >= 1, `weights` (a
    host array or None) F integers, none negative, their sum below 2^62 -- ValueError naming gr_face_sieve.  -> min_measure as an
    int."""
    name = "gr_face_sieve"
    if not (0 <= F < SIEVE_SIZE_LIMIT and 0 <= V < SIEVE_SIZE_LIMIT and 3 * F <= SIEVE_SIZE_LIMIT):
        raise ValueError(f"{name}: F={F}, V={V}: each in [0, 2^31 - 1), and 3 F <= 2^31 - 1")
    if int(min_measure) != min_measure or int(min_measure) < 0 or int(min_measure) >= 2 ** 63:
        raise ValueError(f"{name}: min_measure={min_measure!r} is not an integer in [0, 2^63)")
    if int(max_rounds) < 1:
        raise ValueError(f"{name}: max_rounds={max_rounds!r} is below 1")
    if weights is not None:
        w = np.asarray(weights)
        if w.dtype.kind not in "iu" or w.shape != (F,):
            raise ValueError(f"{name}: weights must be ({F},) integers, got {w.shape} {w.dtype}")
        if F and int(w.min()) < 0:
            raise ValueError(f"{name}: a weight is negative")
        if F and int(w.max()) >= SIEVE_MEASURE_LIMIT:
            raise ValueError(f"{name}: a weight is not below 2^62")
        w = w.astype(np.int64)
        total = (int((w >> 32).sum()) << 32) + int((w & 0xFFFFFFFF).sum())      # exact: neither part sum leaves int64
        if total >= SIEVE_MEASURE_LIMIT:
            raise ValueError(f"{name}: the weights sum to {total}, not below 2^62")
    return int(min_measure)


class NadirRasterizer:
    """One mesh on the device -- vertices in cell units of a parent grid, their heights, the faces --, rastered from above into any
    number of windows of that grid (gr_nadir_raster).  Made by `HipRaster.nadir_rasterizer`, which checks
    the tables (`check_nadir_tables`) and uploads them once."""

    def __init__(self, backend: "HipRaster", verts_q, z, faces):
        torch = _torch()
        self.backend = backend
        self.V, self.F = check_nadir_tables(_host_array(verts_q), _host_array(z), _host_array(faces))
        self._vq = backend._shaped(verts_q, torch.int64, (self.V, 2), "vertices")
        self._z = backend._shaped(z, torch.float64, (self.V,), "z (one per vertex)")
        self._faces = backend._shaped(faces, torch.int32, (self.F, 3), "faces")

    def window(self, col_off: int, row_off: int, width: int, height: int, small_cells: int = 0, item_rows: int = 0):
        """The window (col_off, row_off, width, height) of the parent grid -> (face (height, width) int32 tensor: the face whose
        surface is highest at the cell's centre, -1 for none; z (height, width) float64 tensor: that height, NaN for none; stats
        (GR_NADIR_STAT_WORDS,) int64 tensor).  small_cells and item_rows steer the work decomposition alone (0: the defaults);
        the planes do not depend on them.  The window is validated on the host first (`check_nadir_window`: ValueError); a face
        that names a vertex outside [0, V) is a ValueError behind the call.  Waits for the call."""
        torch = _torch()
        hip = self.backend
        col_off, row_off, width, height = int(col_off), int(row_off), int(width), int(height)
        small_cells, item_rows = int(small_cells), int(item_rows)
        check_nadir_window(col_off, row_off, width, height, small_cells, item_rows)
        face = hip._empty((height, width), torch.int32)
        z = hip._empty((height, width), torch.float64)
        stats = hip._stats(GR_NADIR_STAT_WORDS)
        hip._call("gr_nadir_raster", _ptr(self._vq if self.V else None), _ptr(self._z if self.V else None), self.V,
                  _ptr(self._faces if self.F else None), self.F, col_off, row_off, width, height, small_cells, item_rows,
                  face.data_ptr(), z.data_ptr(), stats.data_ptr(), hip._stream())
        hip._check_faces("gr_nadir_raster", stats, GR_NADIR_STAT_BAD_INDEX, self.V)
        return face, z, stats


class PictureCalls:
    """The two picture calls on one backend (include/geograster_vis.h), behind `HipRaster.face_light`,
    `HipRaster.shade_view` and `HipRaster.composite_labels`, which document them.  Every output is allocated through the backend
    (`_empty`), every input goes through `_shaped`."""

    def __init__(self, backend: "HipRaster"):
        self.backend = backend

    def face_light(self, verts, faces, view_dir, ambient: float = 0.3):
        torch = _torch()
        hip = self.backend
        v = hip._shaped(verts, torch.float32, ("V", 3), "vertices")
        f = hip._shaped(faces, torch.int32, ("F", 3), "faces")
        d = [float(x) for x in np.asarray(view_dir, dtype=np.float64).reshape(3)]
        light = hip._empty((int(f.shape[0]),), torch.uint8)
        if f.shape[0]:
            args = ShadeArgs(face_light=light.data_ptr(), verts=_ptr(v if v.shape[0] else None), faces=f.data_ptr(),
                             stream=hip._stream().value, F=int(f.shape[0]), V=int(v.shape[0]), dir_x=d[0], dir_y=d[1], dir_z=d[2],
                             ambient=float(ambient))
            hip._call("gr_shade_view", ctypes.byref(args))
        return light

    def shade_view(self, ids, depth, face_rgb, face_light, supersample: int = 1, radius: Optional[int] = None, strength: float = 0.0,
                   background=(255, 255, 255)):
        torch = _torch()
        hip = self.backend
        s = int(supersample)
        if not 1 <= s <= SHADE_MAX_SUPERSAMPLE:
            raise ValueError(f"gr_shade_view: supersample={supersample} outside [1, {SHADE_MAX_SUPERSAMPLE}]")
        ids_t = hip._shaped(ids, torch.int32, ("Hs", "Ws"), "ids")
        depth_t = hip._shaped(depth, torch.float32, tuple(ids_t.shape), "depth (as ids)")
        if ids_t.shape[0] % s or ids_t.shape[1] % s or not ids_t.numel():
            raise ValueError(f"gr_shade_view: planes of {tuple(ids_t.shape)} samples are no picture at supersample={s}")
        rgb = hip._shaped(face_rgb, torch.uint8, ("F", 3), "face_rgb")
        light = hip._shaped(face_light, torch.uint8, (int(rgb.shape[0]),), "face_light (one per face)")
        H, W, F = int(ids_t.shape[0]) // s, int(ids_t.shape[1]) // s, int(rgb.shape[0])
        out = hip._empty((H, W, 3), torch.uint8)
        bg = [int(x) for x in background]
        args = ShadeArgs(ids=ids_t.data_ptr(), depth=depth_t.data_ptr(), face_rgb=_ptr(rgb if F else None),
                         face_light=_ptr(light if F else None), out=out.data_ptr(), stream=hip._stream().value, F=F, strength=float(strength),
                         width=W, height=H, supersample=s, radius=s if radius is None else int(radius), bg_r=bg[0], bg_g=bg[1],
                         bg_b=bg[2])
        hip._call("gr_shade_view", ctypes.byref(args))
        return out

    def composite_labels(self, photo, label, table=None, discrete: bool = False, shift: float = 0.0, scale: float = 1.0,
                         weight: float = 0.5, grey_overlay: bool = True):
        torch = _torch()
        hip = self.backend

        def kind(a):
            return torch.uint8 if str(a.dtype).endswith("uint8") else torch.float64

        photo_t = hip._shaped(photo, kind(photo), ("h", "w", 3), "photo")
        h, w = int(photo_t.shape[0]), int(photo_t.shape[1])
        channels = 3 if len(label.shape) == 3 else 1
        label_t = hip._shaped(label, kind(label), (h, w, 3) if channels == 3 else (h, w), "label (as the photo)")
        if channels == 3 and label_t.dtype == torch.uint8 and discrete:
            raise ValueError("gr_composite_labels: a uint8 colour label with discrete classes is not supported")
        if not h * w:
            raise ValueError(f"gr_composite_labels: an empty image {h} x {w}")
        table_t = None if channels == 3 else hip._shaped(table, torch.float64, ("N", 3), "colour table")
        out = hip._empty((h, 3 * w, 3), torch.uint8)
        args = CompositeArgs(photo=photo_t.data_ptr(), label=label_t.data_ptr(), table=_ptr(table_t), out=out.data_ptr(),
                             stream=hip._stream().value, shift=float(shift), scale=float(scale), weight=float(weight), width=w, height=h,
                             table_rows=0 if table_t is None else int(table_t.shape[0]),
                             photo_dtype=GR_DTYPE_U8 if photo_t.dtype == torch.uint8 else GR_DTYPE_F64,
                             label_dtype=GR_DTYPE_U8 if label_t.dtype == torch.uint8 else GR_DTYPE_F64, label_channels=channels,
                             discrete=int(bool(discrete)), grey_overlay=int(bool(grey_overlay)))
        hip._call("gr_composite_labels", ctypes.byref(args))
        return out


class RasterWarper:
    """The raster -> raster call on one backend (include/geograster_warp.h), behind `HipRaster.warp_raster`,
    which documents it.  Every output is allocated through the backend (`_empty`, `_stats`), the source goes through `_dev`."""

    def __init__(self, backend: "HipRaster"):
        self.backend = backend

    def warp(self, data, src_inverse, src_nodata, dst_transform, window, src_crs, dst_crs, resampling, dst_nodata, dst_dtype, out):
        from geograypher_amd.utils.geospatial import KIND_ECEF, crs_tuple

        torch = _torch()
        hip = self.backend
        if resampling not in WARP_RESAMPLING:
            raise ValueError(f"gr_warp_raster: resampling={resampling!r} is neither 'nearest' nor 'bilinear'")
        name = str(data.dtype).replace("torch.", "")
        d_t = hip._dev(data, getattr(torch, name if name in WARP_DTYPES else "float64"))
        if d_t.ndim == 2:
            d_t = d_t[None]
        src_name = str(d_t.dtype).replace("torch.", "")
        dst_np = np.dtype(src_name) if dst_dtype is None else warp_numpy_dtype(dst_dtype)
        col_off, row_off, width, height = (int(k) for k in window)
        check_warp_window(tuple(d_t.shape), col_off, row_off, width, height, dst_np)
        B, H, W = (int(k) for k in d_t.shape)
        nd = warp_dst_nodata(dst_nodata, src_nodata, dst_np)
        coeffs = []
        for what, six in (("src_inverse", src_inverse), ("dst_transform", dst_transform)):
            six = [float(k) for k in np.asarray(six, dtype=np.float64).reshape(-1)]
            if len(six) != 6 or not np.all(np.isfinite(six)):
                raise ValueError(f"gr_warp_raster: {what} has six finite coefficients, got {six}")
            coeffs.append((ctypes.c_double * 6)(*six))
        if (src_crs is None) != (dst_crs is None):
            raise ValueError("gr_warp_raster: src_crs and dst_crs are given together or not at all")
        sides = None
        if src_crs is not None:
            sides = [Crs(int(k), float(lon0), float(k0), float(fe), float(fn)) for k, lon0, k0, fe, fn in
                     (crs_tuple(src_crs), crs_tuple(dst_crs))]
            if KIND_ECEF in (sides[0].kind, sides[1].kind):
                raise ValueError("gr_warp_raster: an ECEF side: a raster is planar or geographic")
        dst_torch = getattr(torch, dst_np.name)
        if out is None:
            out = hip._empty((B, height, width), dst_torch)
        elif (not isinstance(out, torch.Tensor) or out.dtype != dst_torch or tuple(out.shape) != (B, height, width)
              or not out.is_contiguous() or out.device != d_t.device):
            raise ValueError(f"out must be a contiguous {dst_np.name} ({B}, {height}, {width}) tensor on {d_t.device}")
        stats = hip._stats(GR_WARP_STAT_WORDS)
        args = WarpRasterArgs(data=d_t.data_ptr(), out=out.data_ptr(), stats=stats.data_ptr(), stream=hip._stream().value,
                              src_inverse6_h=ctypes.addressof(coeffs[0]), dst_transform6_h=ctypes.addressof(coeffs[1]),
                              src_crs_h=None if sides is None else ctypes.addressof(sides[0]),
                              dst_crs_h=None if sides is None else ctypes.addressof(sides[1]),
                              src_nodata=0.0 if src_nodata is None else float(src_nodata), dst_nodata=nd, B=B, H=H, W=W,
                              src_dtype=WARP_DTYPES[src_name], dst_dtype=WARP_DTYPES[dst_np.name],
                              has_src_nodata=0 if src_nodata is None else 1, col_off=col_off, row_off=row_off, width=width,
                              height=height, resampling=WARP_RESAMPLING[resampling], same_crs=1 if sides is None else 0)
        hip._call("gr_warp_raster", ctypes.byref(args))
        return out, stats


class FaceSieve:
    """The face-sieve call on one backend (include/geograster_components.h), behind `HipRaster.face_sieve`,
    which documents it.  Every output is allocated through the backend (`_empty`, `_stats`), the inputs go through `_shaped` and `_dev`."""

    def __init__(self, backend: "HipRaster"):
        self.backend = backend

    def sieve(self, faces, classes, weights, min_measure, fill_unlabelled, vertex_canon, max_rounds, n_vertices, out):
        torch = _torch()
        hip = self.backend
        f_t = hip._shaped(faces, torch.int32, ("F", 3), "faces")
        F = int(f_t.shape[0])
        c_t = hip._shaped(classes, torch.int32, (F,), "classes (one per face)")
        canon_t = None if vertex_canon is None else hip._dev(vertex_canon, torch.int32).reshape(-1)
        if canon_t is not None:
            V = int(canon_t.shape[0])
        elif n_vertices is not None:
            V = int(n_vertices)
        else:
            V = int(f_t.max().item()) + 1 if F else 0
            if V < 0 or V >= SIEVE_SIZE_LIMIT:
                raise ValueError(f"gr_face_sieve: the faces name vertex {V - 1}")
        w_host = None
        if weights is not None:
            w_host = weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else np.asarray(weights)
        min_measure = check_sieve_arguments(F, V, w_host, min_measure, max_rounds)
        w_t = None if weights is None else hip._shaped(weights, torch.int64, (F,), "weights (one per face)")
        if out is not None and (not isinstance(out, torch.Tensor) or out.data_ptr() != c_t.data_ptr()):
            raise ValueError("out must be the classes themselves, a contiguous int32 tensor on the device (in place), or None")
        class_out = c_t if out is not None else hip._empty((F,), torch.int32)
        comp = hip._empty((F,), torch.int32)
        stats = hip._stats(GR_SIEVE_STAT_WORDS)
        args = FaceSieveArgs(faces=_ptr(f_t if F else None), face_class=_ptr(c_t if F else None), weights=_ptr(w_t if F else None),
                             vertex_canon=_ptr(canon_t if canon_t is not None and V else None), class_out=_ptr(class_out if F else None),
                             comp=_ptr(comp if F else None), stats=stats.data_ptr(), stream=hip._stream().value, F=F, V=V,
                             min_measure=min_measure, has_canon=0 if canon_t is None else 1, fill_unlabelled=1 if fill_unlabelled else 0,
                             max_rounds=int(max_rounds), reserved=0)
        hip._call("gr_face_sieve", ctypes.byref(args))
        return class_out, comp, stats


def check_nearest_arguments(R: int, Q: int, max_distance, cell, max_rings) -> tuple:
    """The host checks of gr_nearest_points (K4, K8): sizes inside the call's limits, max_distance None or >= 0 (not NaN), cell a
    finite size >= 0, max_rings >= 1 -- ValueError naming gr_nearest_points.  -> (max_distance as a float, +inf for None, cell,
    max_rings)."""
    name = "gr_nearest_points"
    if not (0 <= R < NEAREST_SIZE_LIMIT and 0 <= Q < NEAREST_SIZE_LIMIT):
        raise ValueError(f"{name}: R={R}, Q={Q}: each in [0, 2^31 - 1)")
    md = float("inf") if max_distance is None else float(max_distance)
    if not md >= 0:
        raise ValueError(f"{name}: max_distance={max_distance!r} is not a distance >= 0 (None: no limit)")
    cell = float(cell)
    if not (cell >= 0 and cell != float("inf")):
        raise ValueError(f"{name}: cell={cell!r} is not a finite size >= 0 (0: chosen by the call)")
    if int(max_rings) != max_rings or int(max_rings) < 1 or int(max_rings) >= 2 ** 31:
        raise ValueError(f"{name}: max_rings={max_rings!r} is not a whole number in [1, 2^31)")
    return md, cell, int(max_rings)


class NearestPoints:
    """The nearest-point call on one backend (include/geograster_nearest.h), behind
    `HipRaster.nearest_points`, which documents it.  Every output is allocated through the backend (`_empty`, `_stats`), the inputs
    go through `_shaped`."""

    def __init__(self, backend: "HipRaster"):
        self.backend = backend

    def query(self, ref, query, max_distance, cell, max_rings, return_dist2):
        torch = _torch()
        hip = self.backend
        r_t = hip._shaped(ref, torch.float64, ("R", 3), "ref")
        q_t = hip._shaped(query, torch.float64, ("Q", 3), "query")
        R, Q = int(r_t.shape[0]), int(q_t.shape[0])
        md, cell, max_rings = check_nearest_arguments(R, Q, max_distance, cell, max_rings)
        index = hip._empty((Q,), torch.int32)
        dist2 = hip._empty((Q,), torch.float64) if return_dist2 else None
        stats = hip._stats(GR_NN_STAT_WORDS)
        args = NearestArgs(ref=_ptr(r_t if R else None), query=_ptr(q_t if Q else None), index_out=_ptr(index if Q else None),
                           dist2_out=_ptr(dist2 if Q else None), stats=stats.data_ptr(), stream=hip._stream().value, R=R, Q=Q,
                           cell=cell, max_distance=md, max_rings=max_rings, reserved=0)
        hip._call("gr_nearest_points", ctypes.byref(args))
        return (index, dist2, stats) if return_dist2 else (index, stats)


class RayCommunities:
    """The two community calls of the multiview-detection workflow on one backend (include/geograster_communities.h; DESIGN.md
    section 8p), behind `HipRaster.louvain_communities` and `HipRaster.community_points`, which document them.  Every output is
    allocated through the backend (`_empty`, `_stats`)."""

    def __init__(self, backend: "HipRaster"):
        self.backend = backend

    def louvain(self, i, j, q, n: int, resolution: float, max_sweeps: int, force_path):
        b = self.backend
        torch = _torch()
        n = int(n)
        if force_path not in b._COMM_FORCE:
            raise ValueError(f"force_path must be None, 'group' or 'key', got {force_path!r}")
        if n < 0 or n > GR_COMM_MAX_VERTICES:
            raise ValueError(f"n must be in [0, {GR_COMM_MAX_VERTICES}], got {n}")
        i_t = b._edge_index(i, n, "edge i")
        E = int(i_t.shape[0])
        j_t = b._shaped(b._edge_index(j, n, "edge j"), torch.int32, (E,), "edge j (one per edge)")
        q_t = b._shaped(q, torch.int64, (E,), "edge weights (one per edge)")
        community = b._empty((max(n, 1),), torch.int32)
        size = b._empty((max(n, 1),), torch.int32)
        c_in, c_tot = b._empty((max(n, 1),), torch.int64), b._empty((max(n, 1),), torch.int64)
        stats = b._stats(GR_COMM_STAT_WORDS, zeroed=True)
        rc = b._rc("gr_louvain_communities", _ptr(i_t if E else None), _ptr(j_t if E else None), _ptr(q_t if E else None), E, n,
                      float(resolution), int(max_sweeps), b._COMM_FORCE[force_path], community.data_ptr(), size.data_ptr(),
                      c_in.data_ptr(), c_tot.data_ptr(), stats.data_ptr(), b._stream())
        st = [int(x) for x in stats.cpu().tolist()]
        b.last_bad_edges = st[GR_COMM_STAT_BAD_EDGES]
        if rc == GR_EINDEX:   # the input is wrong, not a position the caller asked for
            raise ValueError(f"gr_louvain_communities: {b.last_bad_edges} bad edges: " + b.lib.gr_last_error(b._ctx).decode("utf-8", "replace"))
        b._check(rc, "gr_louvain_communities")
        m, run = st[GR_COMM_STAT_COMMUNITIES], st[GR_COMM_STAT_LEVELS_RUN]
        record = {"community": community[:n].cpu().numpy(), "size": size[:m].cpu().numpy(), "in": c_in[:m].cpu().numpy(),
                  "tot": c_tot[:m].cpu().numpy()}
        record.update(n_communities=m, M2=st[GR_COMM_STAT_M2], levels=st[GR_COMM_STAT_LEVELS],
                      sweeps=st[GR_COMM_STAT_SWEEPS:GR_COMM_STAT_SWEEPS + run], moves=st[GR_COMM_STAT_MOVES:GR_COMM_STAT_MOVES + run],
                      caps_hit=st[GR_COMM_STAT_CAPS], bad_edges=st[GR_COMM_STAT_BAD_EDGES],
                      rows_per_path=[st[GR_COMM_STAT_ROWS_WAVE], st[GR_COMM_STAT_ROWS_GROUP], st[GR_COMM_STAT_ROWS_KEY]])
        return record

    def points(self, starts, ends, community, n_communities: int):
        b = self.backend
        torch = _torch()
        s_t = b._shaped(starts, torch.float64, ("N", 3), "starts")
        e_t = b._shaped(ends, torch.float64, s_t.shape, "ends")
        n, m = int(s_t.shape[0]), int(n_communities)
        c_t = b._shaped(b._edge_index(community, n, "community"), torch.int32, (n,), "community (one per ray)")
        if m < 0 or m > n:
            raise ValueError(f"n_communities must be in [0, {n}], got {m}")
        points = b._empty((m, 3), torch.float64)
        b._call("gr_community_points", _ptr(s_t if n else None), _ptr(e_t if n else None), _ptr(c_t if n else None), n, m,
                   _ptr(points if m else None), b._stream())
        return points


def polygon_pair_bounds(boxes, poly_offsets, n_faces: int) -> np.ndarray:
    """Upper bound of the pairs each view of a `gr_project_polygon_pairs` call can emit, from the ring table alone (int64,
    one per view): a face has one winning pixel per view and emits at most one pair per class, so a view with K distinct
    classes emits at most F * K; a ring can only be hit by a face whose pixel lies in its box, at most min(F, box area)
    faces, so the view emits at most the sum of that over its rings.  The bound is the smaller of the two."""
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 5)
    poly_offsets = np.asarray(poly_offsets, dtype=np.int64).reshape(-1)
    F = int(n_faces)
    area = np.clip(boxes[:, 2] - boxes[:, 0], 0, None) * np.clip(boxes[:, 3] - boxes[:, 1], 0, None)
    per_ring = np.minimum(area, F)
    out = np.zeros(poly_offsets.shape[0] - 1, dtype=np.int64)
    for v in range(out.shape[0]):
        a, b = int(poly_offsets[v]), int(poly_offsets[v + 1])
        out[v] = min(F * np.unique(boxes[a:b, 4]).size, int(per_ring[a:b].sum()))
    return out


class PairAccumulator:
    """Device-resident pair keys of the sparse index aggregation (derived_meshes.py:470-520).  Every `add` appends the
    keys `face * n_classes + class` of its views to one device buffer through `gr_project_index_pairs` with
    GR_FLAG_DEFER_CHECK (no synchronisation, no per-view sort, no host round trip); `finish` runs ONE radix sort +
    run-length encode over everything (`gr_count_pairs`) and returns (pair_keys, multiplicities) as int64 numpy arrays.
    A view of `add` / `add_rects` emits at most one pair per face, one of `add_polygons` at most `polygon_pair_bounds`, so
    the host knows an upper bound of the fill level without asking the device and nothing is ever dropped; when the buffer
    could overflow it is counted down to its distinct pairs (with their multiplicities, kept on the host) and reused.  A call
    over the buffer is split by views; a single view over it makes the buffer grow to that view's bound, up to MAX_KEYS
    (MemoryError beyond).  `cap` (keyword only) sets the buffer's size in keys instead of max(8 F, 2^20)."""

    MAX_KEYS = 1 << 28  # 2 GiB of keys: the most the buffer grows to for a single view

    def __init__(self, backend: "HipRaster", n_classes: int, counts, neg1_is_last_face: bool = True, *, cap=None):
        torch = _torch()
        self.b = backend
        self.n_classes = int(n_classes)
        self.counts = counts
        self.flags = _flags(neg1_is_last_face) | GR_FLAG_DEFER_CHECK
        self._fixed_cap = cap is not None
        self.cap = max(int(cap), 1) if self._fixed_cap else max(8 * backend.n_faces, 1 << 20)
        self.keys = backend._empty((self.cap,), torch.int64)
        self.key_count = backend._zeros((2,), torch.int64)  # {pair count, error flag} (GR_FLAG_DEFER_CHECK)
        self.bound = 0          # upper bound of the pairs in the buffer
        self.parts = []         # (keys, multiplicities) of earlier compactions, host
        self.compactions = 0
        self.grown = 0          # times the buffer grew to hold one view

    def _views(self, ids):
        """ids (n, h, w) or (h, w) -> (contiguous int32 (n, h, w) tensor on the device, n, h, w)"""
        ids_t, _ = self.b._view_batch(ids)
        return (ids_t, *(int(x) for x in ids_t.shape))

    def _upload(self, *tables):
        """Several int tables as ONE int32 upload: (the tensor, which must outlive the call's enqueue; a pointer per table)."""
        parts = [np.asarray(t).astype(np.int32).reshape(-1) for t in tables]
        table = self.b._dev(np.concatenate(parts), _torch().int32)
        starts = np.cumsum([0] + [p.size for p in parts[:-1]])
        return table, [table.data_ptr() + 4 * int(k) for k in starts]

    def _emit(self, name: str, *head):
        """lib.<name>(ctx, *head, <what every pair entry point takes behind its own arguments>)"""
        b = self.b
        b._call(name, *head, self.n_classes, self.counts.data_ptr(), self.keys.data_ptr(), self.cap, self.key_count.data_ptr(),
                self.flags, b._stream())

    def add(self, ids, img):
        ids_t, img_t = self.b._index_views(ids, img)
        ids_t, n, h, w = self._views(ids_t)
        if not self._make_room(n, lambda k: self.add(ids_t[k], img_t[k])):
            return
        self._emit("gr_project_index_pairs", ids_t.data_ptr(), img_t.data_ptr(), n, h, w)

    def add_rects(self, ids, rects, offsets):
        """`add` for views whose label image is a list of rectangles (`Segmentor.label_rectangles`): ids (n, h, w) or
        (h, w); rects int (R, 5) rows {imin, jmin, imax, jmax, class}, half-open and in paint order; offsets (n + 1,), view
        k's rows are rects[offsets[k]:offsets[k + 1]].  The tables go to the device as ONE small int32 upload; the label of a
        face's winning pixel is the class of the last rectangle containing it (`gr_project_rect_pairs`)."""
        ids_t, n, h, w = self._views(ids)
        rects = _host_array(rects).reshape(-1, 5)
        offsets = _host_array(offsets).reshape(-1)
        _check_offsets(offsets, n, rects.shape[0], "views", "rectangle", "rectangles")
        _check_int32(rects, "rectangle corners and classes")
        if not self._make_room(n, lambda k: self.add_rects(ids_t[k], rects[offsets[k]:offsets[k + 1]],
                                                           np.array([0, offsets[k + 1] - offsets[k]]))):
            return
        table, (offs_ptr, rects_ptr) = self._upload(offsets, rects)
        self._emit("gr_project_rect_pairs", ids_t.data_ptr(), rects_ptr, offs_ptr, n, h, w)

    def add_polygons(self, ids, boxes, vert_offsets, verts, poly_offsets):
        """`add` for views whose label image is the multi-hot mask of polygon rings (`Segmentor.label_regions`): ids (n, h, w)
        or (h, w); boxes int (R, 5) rows {imin, jmin, imax, jmax, class}, each ring's clipped candidate box, half-open, sorted
        by class within a view; vert_offsets (R + 1,), ring r's vertices are verts[vert_offsets[r]:vert_offsets[r + 1]];
        verts float64 (N, 2) (row, col); poly_offsets (n + 1,), view k's rings are boxes[poly_offsets[k]:poly_offsets[k + 1]].
        The tables go to the device as one int32 and one float64 upload; a face's winning pixel is one observation of every
        class with a ring that contains it (`gr_project_polygon_pairs`)."""
        ids_t, n, h, w = self._views(ids)
        boxes = _host_array(boxes).reshape(-1, 5)
        vert_offsets = _host_array(vert_offsets).reshape(-1)
        poly_offsets = _host_array(poly_offsets).reshape(-1)
        verts = np.ascontiguousarray(_host_array(verts), dtype=np.float64).reshape(-1, 2)
        R = boxes.shape[0]
        _check_offsets(poly_offsets, n, R, "views", "polygon", "rings")
        _check_offsets(vert_offsets, R, verts.shape[0], "rings", "vertex", "vertices", at_least_one="vertex per ring")
        _check_int32(boxes, "box corners and classes")
        _check_int32(vert_offsets, "vertex offsets")
        if boxes.size and (boxes[:, :2].min() < 0 or boxes[:, 2].max() > h or boxes[:, 3].max() > w):
            raise ValueError(f"boxes must be clipped to the ({h}, {w}) image")
        if R > 1:
            falls = np.nonzero(np.diff(boxes[:, 4]) < 0)[0] + 1   # a class may only fall where a new view starts
            if not np.isin(falls, poly_offsets).all():
                raise ValueError("the rings of a view must be sorted by class")

        def one_view(k):
            a, e = int(poly_offsets[k]), int(poly_offsets[k + 1])
            va, ve = int(vert_offsets[a]), int(vert_offsets[e])
            self.add_polygons(ids_t[k], boxes[a:e], vert_offsets[a:e + 1] - va, verts[va:ve], np.array([0, e - a]))

        if not self._make_room(n, one_view, polygon_pair_bounds(boxes, poly_offsets, self.b.n_faces)):
            return
        table, (offs_ptr, voffs_ptr, boxes_ptr) = self._upload(poly_offsets, vert_offsets, boxes)
        verts_t = self.b._dev(verts, _torch().float64)
        self._emit("gr_project_polygon_pairs", ids_t.data_ptr(), boxes_ptr, voffs_ptr, _ptr(verts_t if R else None),
                   offs_ptr, n, h, w)

    def _make_room(self, n: int, add_view, bounds=None) -> bool:
        """Room for the pairs of a call over n views: at most `bounds[k]` of view k, one per face where no bounds are given.
        A call that exceeds the buffer on its own is added view by view instead (`add_view(k)`) and False returned; otherwise
        the buffer is compacted first if the call could overflow it, `bound` counts the call in, and the caller makes it."""
        F = self.b.n_faces
        bounds = [F] * n if bounds is None else [int(x) for x in bounds]
        largest = max(bounds, default=0)
        if largest > self.cap:
            # a single view must fit: the mesh may be uploaded (or replaced by a larger one) after the accumulator was made,
            # a view of polygon rings may emit several pairs per face, or the caller chose a small buffer
            if largest > self.MAX_KEYS:
                raise MemoryError(f"one view may emit {largest} (face, class) pairs, more than the {self.MAX_KEYS} keys "
                                  "(2 GiB) the pair buffer grows to")
            self._compact()
            self.cap = largest if self._fixed_cap else max(largest, 8 * F, 1 << 20)
            self.keys = self.b._empty((self.cap,), _torch().int64)
            self.grown += 1
        total = sum(bounds)
        if total > self.cap:
            for k in range(n):
                add_view(k)
            return False
        if self.bound + total > self.cap:
            self._compact()
        self.bound += total
        return True

    def _compact(self):
        raw, bad = (int(x) for x in self.key_count.cpu().tolist())
        if bad:
            raise IndexError(f"gr_project_index_pairs / _rect_pairs / _polygon_pairs: an image value is not a class index in "
                             f"[0, {self.n_classes})")
        if raw > 0:
            self.parts.append(self.b._count_pairs(self.keys, raw))
            self.compactions += 1
        self.key_count.zero_()
        self.bound = 0

    def finish(self):
        self._compact()
        if not self.parts:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        if len(self.parts) == 1:
            return self.parts[0]
        keys = np.concatenate([p[0] for p in self.parts])
        mult = np.concatenate([p[1] for p in self.parts])
        uniq, inv = np.unique(keys, return_inverse=True)
        return uniq, np.bincount(inv, weights=mult, minlength=uniq.size).astype(np.int64)


_default_backends = {}
_default_backends_lock = threading.Lock()


def default_backend(device: Optional[int] = None):
    """One shared `HipRaster` per (device, host thread) for callers that are not handed a backend (camera-set warps, the
    down-scale of `get_image`).  A libgeograster context is not thread safe (include/geograster.h: one context per device and
    host thread): a loader thread that resizes photos while the caller's thread rasterizes gets a context of its own."""
    _require_gpu()
    dev = _torch().cuda.current_device() if device is None else int(device)
    key = (dev, threading.get_ident())
    with _default_backends_lock:
        if key not in _default_backends:
            _default_backends[key] = HipRaster(dev)
        return _default_backends[key]


class HipRaster:
    """Device backend: one libgeograster context on one GPU, operating on torch tensors.

    All methods take and return torch tensors that live on `self.device`; the Python mesh class converts to the
    numpy arrays the reference API promises only at its own boundary.
    """

    def __init__(self, device: Optional[int] = None):
        torch = _torch()
        self.lib = load_library()
        _require_gpu()
        if device is None:
            device = torch.cuda.current_device()
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        handle = ctypes.c_void_p()
        rc = self.lib.gr_ctx_create(self.device_index, ctypes.byref(handle))
        if rc != GR_OK:
            raise RuntimeError(f"gr_ctx_create(device={device}) failed with code {rc}")
        self._ctx = handle
        self._verts = None
        self._faces = None
        self.last_retries = 0
        self.last_stats = {}
        self.last_ray_pair_calls = 0   # library calls of the last `ray_pair_edges` / `class_outlines`: 1, or 2 when the first
        self.last_outline_calls = 0    # offer of room was too small (`_count_then_fill`)
        self.n_faces = 0
        self.n_verts = 0
        self.vertex_order = "r1"

    # -- plumbing ------------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            self.lib.gr_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        torch = _torch()
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, rc: int, what: str):
        if rc == GR_OK:
            return
        msg = self.lib.gr_last_error(self._ctx)
        msg = msg.decode("utf-8", "replace") if msg else ""
        if rc == GR_EINVAL:
            raise ValueError(f"{what}: {msg}")
        if rc == GR_EINDEX:
            raise IndexError(f"{what}: {msg}")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")

    def _rc(self, name: str, *args) -> int:
        """lib.<name>(ctx, *args) with this backend's device current -> the library's code, whatever it is."""
        with _torch().cuda.device(self.device):
            return getattr(self.lib, name)(self._ctx, *args)

    def _call(self, name: str, *args):
        """`_rc`, and a code other than GR_OK raises (`_check`)."""
        self._check(self._rc(name, *args), name)

    def _empty(self, shape, dtype):
        return _torch().empty(shape, dtype=dtype, device=self.device)

    def _zeros(self, shape, dtype):
        return _torch().zeros(shape, dtype=dtype, device=self.device)

    def _full(self, shape, value, dtype):
        return _torch().full(shape, value, dtype=dtype, device=self.device)

    def _stats(self, words: int, zeroed: bool = False):
        """The int64 statistics block of an entry point (GR_*_STAT_WORDS); `zeroed` where the call may be skipped."""
        return (self._zeros if zeroed else self._empty)((words,), _torch().int64)

    def _count_pairs(self, keys, n: int):
        """gr_count_pairs over the first n > 0 pair keys of a device buffer: (distinct keys, multiplicities), int64 numpy."""
        torch = _torch()
        uniq = self._empty((n,), torch.int64)
        mult = self._empty((n,), torch.int32)
        n_unique = ctypes.c_int64(0)
        self._call("gr_count_pairs", keys.data_ptr(), n, uniq.data_ptr(), mult.data_ptr(), ctypes.byref(n_unique),
                   self._stream())
        k = int(n_unique.value)
        return uniq[:k].cpu().numpy(), mult[:k].cpu().numpy().astype(np.int64)

    def _dev(self, array, dtype):
        """numpy / tensor -> contiguous tensor of `dtype` on this device (no copy when already there)."""
        torch = _torch()
        if isinstance(array, torch.Tensor):
            return array.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(array)).to(device=self.device, dtype=dtype).contiguous()

    def _ring_table(self, ring_vertices, ring_offsets, ring_polygon, polygon_boxes=None, ring_is_hole=None, n_polygons: int = 0):
        """A ring table on this device, its shapes checked: `RingTable` (ring vertices (N, 2) int64, offsets (R + 1,) int64, polygons
        (R,) int32, boxes (P, 4) int64 or None, hole flags (R,) int32 or None, N, R, P); without boxes P is `n_polygons`."""
        torch = _torch()
        rv_t = self._shaped(ring_vertices, torch.int64, ("N", 2), "ring vertices")
        rp_t = self._dev(ring_polygon, torch.int32).reshape(-1)
        R = int(rp_t.shape[0])
        off_t = self._shaped(ring_offsets, torch.int64, (R + 1,), "ring offsets (one more than ring polygons)")
        rh_t = None if ring_is_hole is None else self._shaped(ring_is_hole, torch.int32, (R,), "ring hole flags (one per ring polygon)")
        box_t = None if polygon_boxes is None else self._shaped(polygon_boxes, torch.int64, ("P", 4), "polygon boxes")
        return RingTable(rv_t, off_t, rp_t, box_t, rh_t, int(rv_t.shape[0]), R, int(n_polygons if box_t is None else box_t.shape[0]))

    def _shaped(self, array, dtype, pattern: tuple, name: str):
        """numpy / tensor -> contiguous tensor of `dtype` on this device whose shape fits `pattern`: an int is the length an axis
        must have, a letter stands for any length -- ("V", 3), (2, "H", "W"), (F,).  ValueError names the argument, the
        pattern and the shape it got."""
        t = self._dev(array, dtype)
        shape = t.shape
        fits = len(shape) == len(pattern)
        for k, n in zip(pattern, shape) if fits else ():
            if k != n and not isinstance(k, str):
                fits = False
        if not fits:
            want = ", ".join(str(k) for k in pattern) + ("," if len(pattern) == 1 else "")
            raise ValueError(f"{name} must be ({want}), got {tuple(shape)}")
        return t

    def _mesh_2d(self, verts_q, faces):
        """(verts_q (V, 2) int64, faces (F, 3) int32) on this device, checked."""
        torch = _torch()
        return self._shaped(verts_q, torch.int64, ("V", 2), "vertices"), self._shaped(faces, torch.int32, ("F", 3), "faces")

    def _points_faces(self, points, faces):
        """points (V, 3) float64 and faces (F, 3) int, or None for a row per vertex -> (points, faces or None on this device,
        checked; V; N, the rows of the result: F with faces, V without)."""
        torch = _torch()
        p_t = self._shaped(points, torch.float64, ("V", 3), "points")
        f_t = None if faces is None else self._shaped(faces, torch.int32, ("F", 3), "faces")
        V = int(p_t.shape[0])
        return p_t, f_t, V, V if f_t is None else int(f_t.shape[0])

    def _view_batch(self, ids, other=None, dtype=None, name: str = "", channels: bool = False):
        """(h, w) means one view: ids (N, h, w) or (h, w), and a companion array of the same shape (`channels`: with one more
        axis behind it) -> (ids (N, h, w) int32, the companion (N, h, w[, C]) in `dtype`, or None) on this device."""
        ids_t = self._dev(ids, _torch().int32)
        o_t = None if other is None else self._dev(other, dtype)
        if ids_t.ndim == 2:
            ids_t, o_t = ids_t[None], None if o_t is None else o_t[None]
        if ids_t.ndim != 3:
            raise ValueError(f"ids must be (N, h, w) or (h, w), got {tuple(ids_t.shape)}")
        if o_t is not None and (o_t.ndim != 3 + channels or o_t.shape[:3] != ids_t.shape):
            raise ValueError(f"ids {tuple(ids_t.shape)} and {name} {tuple(o_t.shape)} differ in shape")
        return ids_t, o_t

    def _check_faces(self, name: str, stats, word: int, V: int):
        """The one bad-face rule: read word `word` of a call's statistics block back (which waits for the call, unless the block
        is on the host already) and raise when it counted faces with a vertex index the kernel refused."""
        n_bad = int(stats[word].item())
        if n_bad:
            raise ValueError(f"{name}: {n_bad} faces name a vertex outside [0, {V})")

    def set_profiling(self, enabled: bool):
        self._check(self.lib.gr_set_profiling(self._ctx, 1 if enabled else 0), "gr_set_profiling")

    def set_option(self, key: int, value: int):
        """Tuning knobs of include/geograster.h, by name: key one of this module's GR_OPT_* (GR_OPT_TILE_H_LOG2,
        GR_OPT_BATCH, GR_OPT_DIRECT_CAP: 0 = exact binning, ...); GR_OPT_VARIANT takes the OR of GR_VAR_*, GR_OPT_DEBUG that
        of GR_DBG_*."""
        self._check(self.lib.gr_set_option(self._ctx, int(key), int(value)), "gr_set_option")

    def set_vertex_order(self, name: str):
        """"r1" (default): rule R1 of DESIGN.md; "gl": the perspective divide, viewport transform and snap in an OpenGL
        pipeline's order of operations (GR_OPT_VERTEX_ORDER: what Mesa's llvmpipe executes; the principal point must be the
        window centre).  The only option results depend on."""
        if name not in ("r1", "gl"):
            raise ValueError(f"vertex_order must be 'r1' or 'gl', got {name!r}")
        self.set_option(GR_OPT_VERTEX_ORDER, 1 if name == "gl" else 0)
        self.vertex_order = name

    def stage_times(self) -> dict:
        st = StageTimes()
        self._check(self.lib.gr_get_stage_times(self._ctx, ctypes.byref(st)), "gr_get_stage_times")
        return st.as_dict()

    # -- mesh ----------------------------------------------------------------------------------------------------
    def upload_mesh(self, verts, faces):
        """verts (V,3) float, faces (F,3) int in the cameras' local frame (meshes.py:1641-1676 output)."""
        torch = _torch()
        v = self._shaped(verts, torch.float32, ("V", 3), "mesh vertices")
        f = self._shaped(faces, torch.int32, ("F", 3), "mesh faces")
        self._call("gr_mesh_upload", v.data_ptr(), f.data_ptr(), v.shape[0], f.shape[0], self._stream())
        self._verts, self._faces = v, f  # borrowed by the library: keep alive
        self.n_verts, self.n_faces = int(v.shape[0]), int(f.shape[0])

    def debug_upload(self) -> dict:
        """For tests: what the last upload left on the device (gr_debug_read_upload) -- {"orig": (F,) int32, "blk": (B, 4)
        float32, "bvert": (B, 192, 3) float32, "bidx": (F,) int32 holding the library's uint32 words bit for bit, "mesh_sig":
        int}, B = ceil(F / 64).  RuntimeError (GR_ENOMESH) without a mesh."""
        torch = _torch()
        F = max(self.n_faces, 1)
        B = (F + 63) // 64
        orig, bidx = self._empty((F,), torch.int32), self._empty((F,), torch.int32)
        blk, bvert = self._empty((B, 4), torch.float32), self._empty((B, 192, 3), torch.float32)
        sig = ctypes.c_uint64(0)
        self._call("gr_debug_read_upload", orig.data_ptr(), blk.data_ptr(), bvert.data_ptr(), bidx.data_ptr(), ctypes.byref(sig),
                   self._stream())
        return {"orig": orig, "blk": blk, "bvert": bvert, "bidx": bidx, "mesh_sig": int(sig.value)}

    def debug_stage(self, block: int = 0, offset: int = 0, n: int = 0):
        """For tests: (`n` bytes at `offset` of the stage scratch as a (n,) uint8 tensor, the bytes the block holds now)
        (gr_debug_read_stage) -- block 0 is the stage arena, block 1 the second block of the outline calls; a negative `offset`
        counts from the block's end.  n = 0 asks for the size alone."""
        size = ctypes.c_int64(0)
        self._call("gr_debug_read_stage", int(block), 0, 0, None, ctypes.byref(size), self._stream())
        if offset < 0:
            offset += int(size.value)
        out = self._empty((int(n),), _torch().uint8)
        self._call("gr_debug_read_stage", int(block), int(offset), int(n), out.data_ptr() if n else None, ctypes.byref(size),
                   self._stream())
        return out, int(size.value)

    # -- pix2face ------------------------------------------------------------------------------------------------
    def raster_face_ids(self, cams, h: int, w: int, out=None, want_depth: bool = False, check: bool = True):
        """cams (N,16) camera records -> ids (N,h,w) int32 tensor [, depth (N,h,w) float32].

        `check=True` (default) reads the call's status back and repeats the unfinished views when a tile overflowed its
        bin segment (`last_retries`; the statistics of all attempts are summed in `last_stats`).  `check=False` only
        enqueues the work: nothing is known about its outcome -- `last_stats` says `{"unchecked": True}` -- and a view whose
        bins overflowed is INCOMPLETE until the caller asks `raster_status()`, which raises on overflow.  Use it only for
        repeats of a call that was sized with `check=True` on the same inputs."""
        torch = _torch()
        cams_t = self._shaped(cams, torch.float32, ("N", GR_CAM_FLOATS), "camera records")
        n = int(cams_t.shape[0])
        if out is None:
            out = self._empty((n, h, w), torch.int32)
        elif tuple(out.shape) != (n, h, w) or out.dtype != torch.int32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous int32 tensor of shape (N,h,w)")
        depth = self._empty((n, h, w), torch.float32) if want_depth else None
        self._checked_raster(n, check, lambda v0: self._call(
            "gr_raster_face_ids", cams_t[v0:].data_ptr(), n - v0, h, w, out[v0:].data_ptr(),
            _ptr(None if depth is None else depth[v0:]), self._stream()))
        return (out, depth) if want_depth else out

    def _checked_raster(self, n: int, check: bool, launch):
        """The attempts of a raster call over n views: `launch(v0)` enqueues views v0 .. n - 1.  With `check`, the status is
        read back and, while it says GR_EOVERFLOW, the call is repeated from the first unfinished view -- the library has
        recorded the need -- four attempts at most; `last_retries` and `last_stats` describe all of them."""
        v0 = 0
        self.last_retries = 0
        acc = _StatsAccumulator()
        for attempt in range(4):
            launch(v0)
            if not check:
                self.last_stats = {"unchecked": True}
                return
            st = RasterStats()
            rc = self.lib.gr_raster_status(self._ctx, ctypes.byref(st))
            causes = self.lib.gr_raster_overflow_causes(self._ctx)
            if rc != GR_EOVERFLOW or attempt == 3:
                self._check(rc, "gr_raster_status")
                acc.add(st, n - v0, partial=False, causes=causes)
                self.last_stats = acc.result()
                return
            acc.add(st, n - v0, partial=True, causes=causes)
            v0 += int(st.views_done)  # only the unfinished views are repeated
            self.last_retries += 1

    def raster_status(self) -> dict:
        st = RasterStats()
        self._check(self.lib.gr_raster_status(self._ctx, ctypes.byref(st)), "gr_raster_status")
        return st.as_dict()

    def overflow_causes(self) -> int:
        """Why the last raster call overflowed, as far as `raster_status()` (or the call's own check) has read it: the OR of
        GR_CAUSE_LIST_OUTGREW (a tile list outgrew its slots), GR_CAUSE_SHORT_MISS (a face missed the 40-byte entry form) and
        GR_CAUSE_LISTS_MET (a tile's entry and micro lists met); 0 for a call without overflow."""
        return int(self.lib.gr_raster_overflow_causes(self._ctx))

    # -- render_flat gather --------------------------------------------------------------------------------------
    def gather_texture(self, ids, face_texture):
        """ids (...,) int32 tensor, face_texture (F,C) -> (..., C) float64 tensor, NaN where ids == -1."""
        return self._gather("gr_gather_texture_f64", ids, face_texture, _torch().float64)

    def gather_texture_u8(self, ids, face_texture, null_value: int = 0):
        """save_renders epilogue: ids (...,) int32, face_texture (F,C) -> (..., C) uint8 tensor (meshes.py:2325-2337)."""
        return self._gather("gr_gather_texture_u8", ids, face_texture, _torch().uint8, int(null_value))

    def _gather(self, name: str, ids, face_texture, out_dtype, *null_value):
        torch = _torch()
        ids_t = self._dev(ids, torch.int32)
        tex = self._dev(face_texture, torch.float64)
        F, C = int(tex.shape[0]), int(tex.shape[1])
        out = self._empty(tuple(ids_t.shape) + (C,), out_dtype)
        self._call(name, ids_t.data_ptr(), ids_t.numel(), tex.data_ptr(), F, C, *null_value, out.data_ptr(), self._stream())
        return out

    def _index_views(self, ids, img):
        """The inputs of the index-pair path: ids (N,h,w) or (h,w), the class-index image of the same shape (a channel axis of
        one is dropped) -> contiguous (N,h,w) int32 and float64 tensors on this device."""
        img_t = self._dev(img, _torch().float64)
        if img_t.ndim == np.ndim(ids) + 1 and img_t.shape[-1] == 1:
            img_t = img_t[..., 0]   # (still contiguous: the axis had one element)
        return self._view_batch(ids, img_t, _torch().float64, "index image")

    def project_index_pairs(self, ids, img, n_classes: int, counts, neg1_is_last_face: bool = True):
        """Sparse index aggregation step (derived_meshes.py:470-520) for N views: ids (N,h,w) int32, img (N,h,w) float64
        with NaN = no prediction.  Accumulates counts (F,) and returns (pair_keys, multiplicities) int64 numpy arrays
        with pair key = face * n_classes + class."""
        torch = _torch()
        ids_t, img_t = self._index_views(ids, img)
        n, h, w = (int(x) for x in ids_t.shape)
        cap = n * self.n_faces
        keys = self._empty((max(cap, 1),), torch.int64)
        key_count = self._zeros((1,), torch.int64)
        self._call("gr_project_index_pairs", ids_t.data_ptr(), img_t.data_ptr(), n, h, w, int(n_classes),
                   counts.data_ptr(), keys.data_ptr(), cap, key_count.data_ptr(), _flags(neg1_is_last_face), self._stream())
        m = int(key_count.item())
        if m == 0:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        return self._count_pairs(keys, m)

    def new_pair_accumulator(self, n_classes: int, counts, neg1_is_last_face: bool = True, *, cap=None):
        """Sparse index aggregation over MANY views with the (face, class) pair keys kept on the device: `add(ids, img)` per
        view (or group of views) only enqueues work, `finish()` sorts and counts the pairs ONCE -- see `PairAccumulator`."""
        return PairAccumulator(self, n_classes, counts, neg1_is_last_face, cap=cap)

    # -- multiview detections: ray-pair graph, boundary clip -------------------------------------------------------
    CLIP_TRIANGLE_LIMIT = 65536  # triangles per gr_rays_clip call

    def ray_pair_count(self, starts, ends, ray_ids, threshold: float) -> int:
        """Number of edges `ray_pair_edges` would return (gr_ray_pairs with no edge buffer: the count alone)."""
        s_t, e_t, id_t = self._ray_inputs(starts, ends, ray_ids)
        total = ctypes.c_int64(0)
        self._call("gr_ray_pairs", s_t.data_ptr(), e_t.data_ptr(), id_t.data_ptr(), int(s_t.shape[0]), float(threshold),
                   None, None, None, 0, ctypes.byref(total), self._stream())
        return int(total.value)

    def ray_pair_edges(self, starts, ends, ray_ids, threshold: float, capacity: Optional[int] = None):
        """The ray-pair graph of calc_graph_weights (utils/numeric.py:428-498) before its host steps: starts, ends (N, 3)
        float64, ray_ids (N,) int (the image of each ray) -> (i, j, dist): int32, int32, float64 tensors of every pair
        i < j from different images whose clamped segment distance is <= threshold, sorted by (i, j).  Count-then-fill inside:
        the first call offers `capacity` edge slots (default max(8 N, 65536)); when the library reports more
        (`last_ray_pair_calls` == 2) the buffers are allocated at that total and the call repeated: the quadratic kernel then
        runs twice, so pass `capacity` where the number of edges is roughly known.  The library synchronises the stream: the
        result is complete on return."""
        torch = _torch()
        s_t, e_t, id_t = self._ray_inputs(starts, ends, ray_ids)
        n = int(s_t.shape[0])
        total = ctypes.c_int64(0)

        def attempt(cap):
            ei, ej, ed = (self._empty((max(cap, 1),), dtype) for dtype in (torch.int32, torch.int32, torch.float64))
            rc = self._rc("gr_ray_pairs", s_t.data_ptr(), e_t.data_ptr(), id_t.data_ptr(), n, float(threshold),
                          *(_ptr(t if cap else None) for t in (ei, ej, ed)), cap, ctypes.byref(total), self._stream())
            m = int(total.value)
            return rc, m, (ei[:m], ej[:m], ed[:m])

        self.last_ray_pair_calls = 0
        edges, self.last_ray_pair_calls = _count_then_fill(
            "gr_ray_pairs", attempt, max(8 * n, 1 << 16) if capacity is None else int(capacity), lambda m: m > 0, self._check)
        return edges

    def _ray_inputs(self, starts, ends, ray_ids):
        torch = _torch()
        s_t = self._shaped(starts, torch.float64, ("N", 3), "starts")
        e_t = self._shaped(ends, torch.float64, s_t.shape, "ends")
        id_t = self._shaped(ray_ids, torch.int32, (s_t.shape[0],), "ray ids (one per ray)")
        return s_t, e_t, id_t

    def clip_rays(self, origins, directions, points, faces):
        """Nearest intersection (t >= 0) of every ray with a small triangle mesh (gr_rays_clip; a boundary surface of
        clip_line_segments, utils/geometric.py:210-222): origins, directions (N, 3) float64, points (V, 3) float64, faces (F, 3)
        int -> (hit bool (N,), t float64 (N,), hit points float64 (N, 3); NaN where nothing is hit).  More than
        CLIP_TRIANGLE_LIMIT triangles is a ValueError."""
        torch = _torch()
        o_t = self._shaped(origins, torch.float64, ("N", 3), "origins")
        d_t = self._shaped(directions, torch.float64, o_t.shape, "directions")
        p_t = self._shaped(points, torch.float64, ("V", 3), "boundary points")
        f_t = self._shaped(faces, torch.int32, ("F", 3), "boundary faces")
        n = int(o_t.shape[0])
        hit = self._zeros((n,), torch.int32)
        t = self._full((n,), float("nan"), torch.float64)
        pts = self._full((n, 3), float("nan"), torch.float64)
        self._call("gr_rays_clip", o_t.data_ptr(), d_t.data_ptr(), n, p_t.data_ptr(), int(p_t.shape[0]), f_t.data_ptr(),
                   int(f_t.shape[0]), hit.data_ptr(), t.data_ptr(), pts.data_ptr(), self._stream())
        return hit.to(torch.bool), t, pts

    # -- multiview detections: communities of the ray graph --------------------------------------------------------
    COMM_MAX_VERTICES = GR_COMM_MAX_VERTICES   # n limit of gr_louvain_communities
    COMM_LDS_ROW = GR_COMM_LDS_ROW             # entries of the longest row its workgroup path takes (csrc/communities.hip)
    _COMM_FORCE = {None: 0, "group": GR_COMM_FORCE_GROUP, "key": GR_COMM_FORCE_KEY}

    def _edge_index(self, array, n: int, name: str):
        """An edge index array -> (E,) int32 on this device.  Wider integers are clamped to [-1, n] first, so that a value the
        cast would wrap stays outside [0, n) and is found by the device check."""
        torch = _torch()
        if not isinstance(array, torch.Tensor):
            array = torch.as_tensor(np.ascontiguousarray(array))
        if array.dtype != torch.int32:
            if array.dtype.is_floating_point or array.dtype == torch.bool:
                raise ValueError(f"{name} must be integers, got {array.dtype}")
            array = array.to(self.device).clamp(-1, n)
        return self._shaped(array, torch.int32, ("E",), name)

    def louvain_communities(self, i, j, q, n: int, resolution: float = 1.0, max_sweeps: int = 32, *, force_path=None):
        """gr_louvain_communities: the undirected edges i, j (E,) int, q (E,) int64 weights in
        [1, 2^31 - 1] of a graph of n vertices; numpy or device tensors, not modified -> the record {"community" (n,) int32, -1
        for a vertex without an edge; "size" (M,) int32, "in", "tot" (M,) int64 per community, by falling size, ties by the
        lowest member; "n_communities" M, "M2", "levels", "sweeps", "moves" (lists, one entry per level that ran: the last one
        moved nothing unless the level cap was hit), "caps_hit" (the OR of GR_COMM_CAP_*), "rows_per_path" [wave, workgroup,
        key], "bad_edges"} as numpy arrays and ints.  `force_path`: None, "group" or "key" sends every row the path can take
        through it (tests: same results).  A bad edge (i == j, an index outside [0, n), a weight outside the range) is found on
        the device and is a ValueError that names their number (`last_bad_edges`).  Waits for the device."""
        return RayCommunities(self).louvain(i, j, q, n, resolution, max_sweeps, force_path)

    def community_points(self, starts, ends, community, n_communities: int):
        """gr_community_points (L14): starts, ends (N, 3) float64, community (N,) int, -1 for a ray of no community -> (M, 3)
        float64 tensor: per community the mean of the closest points over all ordered pairs of distinct member segments (the
        reference's `intersection_average`), NaN for a community of one segment.  Two runs are bit-equal.  Waits for the device."""
        return RayCommunities(self).points(starts, ends, community, n_communities)

    # -- covering meshes: bounds of the points, extremes per grid cell ---------------------------------------------
    COVER_MAX_N = 1024   # grid points a side of gr_cover_grid
    COVER_LDS_N = 56     # ... up to which a workgroup keeps its accumulators in LDS (csrc/cover.hip)

    def _cover_points(self, points):
        return self._shaped(points, _torch().float64, ("V", 3), "points")

    def points_bounds(self, points, stride: int = 1):
        """gr_points_bounds: points (V, 3) float64, numpy or device tensor (a non-contiguous view is made contiguous), of which
        rows 0, stride, 2 stride, ... are visited -> (bounds (6,) float64 tensor xmin xmax ymin ymax zmin zmax over the
        visited finite rows, nonfinite (1,) int64 tensor: the visited rows with a NaN or infinite coordinate).  Only enqueues."""
        torch = _torch()
        p_t = self._cover_points(points)
        bounds = self._empty((6,), torch.float64)
        nonfinite = self._empty((1,), torch.int64)
        self._call("gr_points_bounds", p_t.data_ptr(), int(p_t.shape[0]), int(stride), bounds.data_ptr(), nonfinite.data_ptr(),
                   self._stream())
        return bounds, nonfinite

    def cover_grid(self, points, x_lo, x_hi, y_lo, y_hi, stride: int = 1):
        """gr_cover_grid (DESIGN.md "Covering meshes"): points as for `points_bounds`; x_lo, x_hi, y_lo, y_hi (N,) float64, the
        bounds of the grid cells per axis -> (z_max (N, N) float64, z_min (N, N) float64, count (N, N) int32 tensors), indexed
        [xi, yi]: the extremes of z over the visited rows with x_lo[xi] <= x <= x_hi[xi] and y_lo[yi] <= y <= y_hi[yi], NaN
        where count is 0.  Only enqueues."""
        torch = _torch()
        p_t = self._cover_points(points)
        tabs = [self._dev(t, torch.float64).reshape(-1) for t in (x_lo, x_hi, y_lo, y_hi)]
        N = int(tabs[0].shape[0])
        if any(int(t.shape[0]) != N for t in tabs):
            raise ValueError(f"the four bound tables must have one length, got {[int(t.shape[0]) for t in tabs]}")
        z_max = self._empty((N, N), torch.float64)
        z_min = self._empty((N, N), torch.float64)
        count = self._empty((N, N), torch.int32)   # uint32 payload
        self._call("gr_cover_grid", p_t.data_ptr(), int(p_t.shape[0]), int(stride), N, *(t.data_ptr() for t in tabs),
                   z_max.data_ptr(), z_min.data_ptr(), count.data_ptr(), self._stream())
        return z_max, z_min, count

    # -- image selection: greedy set cover over a face x view incidence --------------------------------------------
    SET_COVER_MAX_VIEWS = GR_SETCOVER_MAX_VIEWS   # n_views limit of gr_set_cover
    SET_COVER_LDS_VIEWS = GR_SETCOVER_LDS_VIEWS   # ... up to which the gain updates go through LDS histograms (csrc/select.hip)
    SET_COVER_BATCH = GR_SETCOVER_BATCH           # pick / apply pairs between two reads of the control words

    def set_cover(self, face_ptr, face_views, n_faces: int, n_views: int, min_observations=1, prune: bool = True, *,
                  return_tensor: bool = False, global_atomics: bool = False):
        """gr_set_cover: the face-major CSR of a face x view incidence -- face_ptr (n_faces + 1,)
        int64, face_views (nnz,) int32, unique within a row; numpy or device tensors -- -> the record {"selected" (n_views,)
        bool, "order" (k,) int32, "gains" (k,) int64, "pruned" (p,) int32, "n_required", "n_covered", "batches",
        "lds_histogram"} as numpy arrays and ints, or with `return_tensor` the arrays as device tensors.  A face is required iff
        at least max(min_observations, 1) views see it; the greedy choice takes the view that sees most uncovered required faces,
        ties to the lowest index; `prune` then drops selected views that later picks made redundant, last selected first.
        `global_atomics` switches the LDS histograms off (same results).  A view index outside [0, n_views) is a ValueError.
        The call waits for the device: the result is complete on return."""
        torch = _torch()
        n_faces, n_views = int(n_faces), int(n_views)
        ptr_t = self._dev(face_ptr, torch.int64).reshape(-1)
        views_t = self._dev(face_views, torch.int32).reshape(-1)
        if n_faces < 0 or n_views < 0 or int(ptr_t.shape[0]) != n_faces + 1:
            raise ValueError(f"face_ptr must hold n_faces + 1 = {n_faces + 1} offsets, got {int(ptr_t.shape[0])}")
        nnz = int(views_t.shape[0])
        selected, order, gains, pruned = (self._empty((max(n_views, 1),), dtype)
                                          for dtype in (torch.uint8, torch.int32, torch.int64, torch.int32))
        stats = self._stats(GR_SETCOVER_STAT_WORDS)
        flags = (GR_SETCOVER_PRUNE if prune else 0) | (GR_SETCOVER_GLOBAL_ATOMICS if global_atomics else 0)
        try:
            self._call("gr_set_cover", ptr_t.data_ptr(), _ptr(views_t if nnz else None), nnz, n_faces, n_views,
                       float(min_observations), flags, selected.data_ptr(), order.data_ptr(), gains.data_ptr(), pruned.data_ptr(),
                       stats.data_ptr(), self._stream())
        except IndexError as err:   # GR_EINDEX: the input is wrong, not a position the caller asked for
            raise ValueError(str(err)) from None
        st = [int(x) for x in stats.cpu().tolist()]
        k, p = st[GR_SETCOVER_STAT_SELECTED], st[GR_SETCOVER_STAT_PRUNED]
        record = {"selected": selected[:n_views].to(torch.bool), "order": order[:k], "gains": gains[:k], "pruned": pruned[:p]}
        if not return_tensor:
            record = {name: t.cpu().numpy() for name, t in record.items()}
        record.update(n_required=st[GR_SETCOVER_STAT_REQUIRED], n_covered=st[GR_SETCOVER_STAT_COVERED],
                      batches=st[GR_SETCOVER_STAT_BATCHES], lds_histogram=bool(st[GR_SETCOVER_STAT_LDS_HISTOGRAM]))
        return record

    # -- label_polygons: weighted face area per (polygon, class) ---------------------------------------------------
    def polygon_class_weights(self, tri, face_class, face_weight, ring_vertices, ring_offsets, ring_polygon, ring_is_hole,
                              polygon_boxes, n_classes: int, within: bool = True):
        """gr_polygon_class_weights (DESIGN.md "Polygon labels"): tri (F, 6) int64 snapped face corners, face_class (F,) int
        (< 0: skip), face_weight (F,) float64 -- numpy or device tensors --, and the snapped ring table of
        `PlanarPolygons.snapped` -> (weights (P, n_classes) float64 tensor, stats (GR_POLY_STAT_WORDS,) int64 tensor: pairs
        tested, pairs contributing, largest ring).  `within`: exact containment (sjoin), else clipped overlay.  Only enqueues."""
        torch = _torch()
        cls_t = self._dev(face_class, torch.int32)
        F, C = int(cls_t.shape[0]), int(n_classes)
        tri_t = self._shaped(tri, torch.int64, (F, 6), "face corners (a row per face class)")
        w_t = self._shaped(face_weight, torch.float64, (F,), "face weights (one per face class)")
        rv_t, off_t, rp_t, box_t, rh_t, n_rv, R, P = self._ring_table(ring_vertices, ring_offsets, ring_polygon, polygon_boxes,
                                                                      ring_is_hole)
        weights = self._empty((P, C), torch.float64)
        stats = self._stats(GR_POLY_STAT_WORDS)
        self._call("gr_polygon_class_weights", tri_t.data_ptr(), cls_t.data_ptr(), w_t.data_ptr(), F, rv_t.data_ptr(),
                   n_rv, off_t.data_ptr(), rp_t.data_ptr(), rh_t.data_ptr(), R, box_t.data_ptr(), P,
                   GR_POLY_WITHIN if within else GR_POLY_OVERLAY, C, weights.data_ptr(), stats.data_ptr(), self._stream())
        return weights, stats

    # -- vector textures: the polygon row of every face centre -----------------------------------------------------
    def face_polygon_index(self, verts_q, faces, ring_vertices, ring_offsets, ring_polygon, ring_is_hole, polygon_boxes,
                           cell_table, check: bool = True):
        """gr_face_polygon_index (DESIGN.md "Vector textures"): verts_q (V, 2) int64 snapped vertices, faces (F, 3) int, the
        snapped ring table of `PlanarPolygons.snapped` (the hole flags play no part: even-odd over all rings of a row) and
        cell_table = (grid (6,) int: x0 y0 cell_w cell_h nx ny, cell_offsets (nx ny + 1,) int64, cell_polygons int32) of
        `utils.geometric.polygon_cell_table` -- numpy or device tensors -> (face_polygon (F,) int32 tensor: the highest row whose
        closed region holds the face centre, -1 for none; stats (GR_FPI_STAT_WORDS,) int64 tensor: ring walks started, faces
        labelled, longest cell list met, faces with a vertex index outside [0, V)).  `check` (default) reads the statistics
        back and raises ValueError when a face names a vertex that does not exist; check=False only enqueues."""
        torch = _torch()
        vq_t, f_t = self._mesh_2d(verts_q, faces)
        rv_t, off_t, rp_t, box_t, _, n_rv, R, P = self._ring_table(ring_vertices, ring_offsets, ring_polygon, polygon_boxes)
        grid, cell_offsets, cell_polygons = cell_table
        grid = [int(v) for v in np.asarray(grid.cpu() if hasattr(grid, "detach") else grid).reshape(-1)]
        co_t = self._dev(cell_offsets, torch.int64)
        cp_t = self._dev(cell_polygons, torch.int32)
        if len(grid) != 6:
            raise ValueError(f"the cell grid is (x0, y0, cell_w, cell_h, nx, ny), got {len(grid)} values")
        x0, y0, cw, ch, nx, ny = grid
        # (the library checks the grid's ranges; the table's length has to fit the grid before its pointer is handed over)
        if 1 <= nx and 1 <= ny and nx * ny <= GR_FPI_MAX_CELLS and tuple(co_t.shape) != (nx * ny + 1,):
            raise ValueError(f"gr_face_polygon_index: a {nx} x {ny} cell grid needs {nx * ny + 1} cell offsets, got {tuple(co_t.shape)}")
        if abs(nx) >= 2 ** 31 or abs(ny) >= 2 ** 31:
            raise ValueError(f"gr_face_polygon_index: bad cell grid nx={nx} ny={ny}")
        F = int(f_t.shape[0])
        out = self._empty((F,), torch.int32)
        stats = self._stats(GR_FPI_STAT_WORDS)
        self._call("gr_face_polygon_index", vq_t.data_ptr(), int(vq_t.shape[0]), f_t.data_ptr(), F, rv_t.data_ptr(),
                   n_rv, off_t.data_ptr(), rp_t.data_ptr(), R, box_t.data_ptr(), P, x0, y0, cw, ch, nx, ny,
                   co_t.data_ptr(), cp_t.data_ptr(), int(cp_t.shape[0]), out.data_ptr(), stats.data_ptr(), self._stream())
        if check:
            self._check_faces("gr_face_polygon_index", stats, GR_FPI_STAT_BAD_FACES, int(vq_t.shape[0]))
        return out, stats

    # -- region of interest: points in a buffered union of polygon rows, the sub-mesh they select ----------------------
    def points_in_region(self, points_q, ring_vertices, ring_offsets, ring_polygon, ring_is_hole, polygon_boxes, buffer_steps: int = 0):
        """gr_points_in_region (DESIGN.md "Region of interest"): points_q (N, 2) int64 snapped points and the snapped ring table of
        `PlanarPolygons.snapped` (the hole flags play no part) -- numpy or device tensors --, buffer_steps the buffer D in grid
        steps, 0 <= D < 2^40 -> (mask (N,) bool tensor: the point lies in the closed region of some row or within D of an edge of
        some ring; stats (GR_PIR_STAT_WORDS,) int64 tensor: points inside, inside by the buffer only, 256-bit comparisons
        formed).  Only enqueues."""
        torch = _torch()
        pq_t = self._shaped(points_q, torch.int64, ("N", 2), "points")
        rv_t, off_t, rp_t, box_t, _, n_rv, R, P = self._ring_table(ring_vertices, ring_offsets, ring_polygon, polygon_boxes)
        D = int(buffer_steps)
        if not 0 <= D < 2 ** 40:
            raise ValueError(f"gr_points_in_region: buffer D={D} outside [0, 2^40) grid steps")
        N = int(pq_t.shape[0])
        mask = self._empty((N,), torch.uint8)
        stats = self._stats(GR_PIR_STAT_WORDS)
        self._call("gr_points_in_region", pq_t.data_ptr(), N, rv_t.data_ptr(), n_rv, off_t.data_ptr(),
                   rp_t.data_ptr(), R, box_t.data_ptr(), P, D, mask.data_ptr(), stats.data_ptr(), self._stream())
        return mask.to(torch.bool), stats

    def submesh_extract(self, mask, faces, check: bool = True):
        """gr_submesh_extract (DESIGN.md "Region of interest", Q5-Q6): mask (V,) bool or uint8 (the selected vertices), faces
        (F, 3) int -- numpy or device tensors -> (face_ids (n_faces,) int64, point_ids (n_points,) int64, new_faces (n_faces, 3)
        int32 tensors, counts (3,) int64 tensor: kept faces, kept vertices, faces with a vertex index outside [0, V)).  A face is
        kept iff one of its vertices is selected, a vertex iff a kept face uses it; the ids are the ascending original indices
        and new_faces indexes the kept vertices.  Reads the counts back (the results are cut to them); `check` (default) raises
        ValueError when a face names a vertex that does not exist."""
        torch = _torch()
        m_t = self._dev(mask, torch.bool).to(torch.uint8).reshape(-1)
        f_t = self._shaped(faces, torch.int32, ("F", 3), "faces")
        V, F = int(m_t.shape[0]), int(f_t.shape[0])
        face_ids = self._empty((F,), torch.int64)
        point_ids = self._empty((V,), torch.int64)
        new_faces = self._empty((F, 3), torch.int32)
        counts = self._empty((3,), torch.int64)
        self._call("gr_submesh_extract", m_t.data_ptr(), V, f_t.data_ptr(), F, face_ids.data_ptr(), point_ids.data_ptr(),
                   new_faces.data_ptr(), counts.data_ptr(), self._stream())
        on_host = counts.cpu()   # the one read of all three counts
        n_faces, n_points = int(on_host[0]), int(on_host[1])
        if check:
            self._check_faces("gr_submesh_extract", on_host, 2, V)
        return face_ids[:n_faces], point_ids[:n_points], new_faces[:n_faces], counts

    # -- mesh decimation: vertex clustering on a uniform grid ---------------------------------
    def to_device(self, array, dtype: str):
        """numpy / tensor -> contiguous tensor of the torch dtype named `dtype` ("int64", "int32", ...) on this device: what a
        caller that hands the same array to several calls uploads once."""
        return self._dev(array, getattr(_torch(), dtype))

    def cluster_count(self, verts_q, s: int) -> int:
        """gr_cluster_count: verts_q (V, 3) int64 snapped vertices behind their per-axis minimum -- numpy
        or a device tensor --, s the cell side in grid steps -> the number of occupied cells, read back (8 bytes): one probe of
        the search of `utils.geometric.cluster_cell_size`."""
        torch = _torch()
        vq_t = self._shaped(verts_q, torch.int64, ("V", 3), "vertices")
        cells = self._empty((1,), torch.int64)
        self._call("gr_cluster_count", vq_t.data_ptr(), int(vq_t.shape[0]), int(s), cells.data_ptr(), self._stream())
        return int(cells.item())

    def cluster_decimate(self, verts_q, faces, s: int, check: bool = True):
        """gr_cluster_decimate: verts_q (V, 3) int64 snapped vertices behind their per-axis minimum,
        faces (F, 3) int -- numpy or device tensors --, s the cell side in grid steps -> (rep (V,) int32: the representative of
        every vertex' cell, -1 outside the key range; face_ids (n_faces,) int64, point_ids (n_points,) int64, new_faces (n_faces,
        3) int32 tensors; stats (GR_DECIM_STAT_WORDS,) int64 tensor).  A face is dropped when two of its corners share a cell, or
        behind an earlier face with the same three cells; a representative is kept iff a kept face uses it; the ids are the
        ascending original indices and new_faces indexes the kept vertices.  Reads the statistics back once (the results are cut
        to its counts); `check` (default) raises ValueError when a face names a vertex that does not exist or that has no cell."""
        torch = _torch()
        vq_t = self._shaped(verts_q, torch.int64, ("V", 3), "vertices")
        f_t = self._shaped(faces, torch.int32, ("F", 3), "faces")
        V, F = int(vq_t.shape[0]), int(f_t.shape[0])
        rep = self._empty((V,), torch.int32)
        face_ids = self._empty((F,), torch.int64)
        point_ids = self._empty((V,), torch.int64)
        new_faces = self._empty((F, 3), torch.int32)
        stats = self._stats(GR_DECIM_STAT_WORDS)
        self._call("gr_cluster_decimate", vq_t.data_ptr(), V, f_t.data_ptr(), F, int(s), rep.data_ptr(), face_ids.data_ptr(),
                   point_ids.data_ptr(), new_faces.data_ptr(), stats.data_ptr(), self._stream())
        on_host = stats.cpu()   # the one read of all the words
        n_faces, n_points = int(on_host[GR_DECIM_STAT_KEPT_FACES]), int(on_host[GR_DECIM_STAT_KEPT_VERTICES])
        if check:
            self._check_faces("gr_cluster_decimate", on_host, GR_DECIM_STAT_BAD_FACES, V)
        return rep, face_ids[:n_faces], point_ids[:n_points], new_faces[:n_faces], on_host

    # -- class outlines: the rings around the faces of every class -------------------------------------------------
    def class_outlines(self, verts_q, faces, face_class, n_classes: int, capacity: Optional[int] = None, check: bool = True):
        """gr_class_outlines: verts_q (V, 2) int64 snapped vertices, faces (F, 3) int, face_class (F,)
        int (outside [0, n_classes): the face takes no part) -- numpy or device tensors -> (canon (V,) int32, ring_vertices (E,)
        int32 canonical vertex ids ring after ring, ring_offsets (R + 1,) int64, ring_class (R,) int32 tensors, stats
        (GR_OUTL_STAT_WORDS,) int64 tensor).  Count-then-fill as `ray_pair_edges`: the first call offers `capacity` ring vertices
        (default: F + 64); when the library reports more (`last_outline_calls` == 2) the buffers are allocated at that total and the
        call repeated.  The library synchronises: the result is complete on return.  `check` (default) raises ValueError when a
        face names a vertex that does not exist."""
        torch = _torch()
        vq_t, f_t = self._mesh_2d(verts_q, faces)
        c_t = self._dev(face_class, torch.int32).reshape(-1)
        V, F = int(vq_t.shape[0]), int(f_t.shape[0])
        if int(c_t.shape[0]) != F:
            raise ValueError(f"{F} faces need {F} classes, got {int(c_t.shape[0])}")
        if not 0 <= int(n_classes) <= GR_OUTL_MAX_CLASSES:
            raise ValueError(f"gr_class_outlines: n_classes={int(n_classes)} outside [0, {GR_OUTL_MAX_CLASSES}]")
        stats = self._stats(GR_OUTL_STAT_WORDS)
        n_edges, n_rings = ctypes.c_int64(0), ctypes.c_int64(0)

        def attempt(cap):
            canon = self._empty((V,), torch.int32)
            ring_vertices = self._empty((max(cap, 1),), torch.int32)
            ring_offsets = self._empty((cap // 3 + 1,), torch.int64)
            ring_class = self._empty((max(cap // 3, 1),), torch.int32)
            rc = self._rc("gr_class_outlines", vq_t.data_ptr(), V, f_t.data_ptr(), F, c_t.data_ptr(), int(n_classes),
                          *(_ptr(t if cap else None) for t in (canon, ring_vertices, ring_offsets, ring_class)), cap,
                          ctypes.byref(n_edges), ctypes.byref(n_rings), stats.data_ptr(), self._stream())
            E, R = int(n_edges.value), int(n_rings.value)
            return rc, E, (canon, ring_vertices[:E], ring_offsets[:R + 1], ring_class[:R], stats)

        cap = F + 64 if capacity is None else int(capacity)
        self.last_outline_calls = 0
        result, self.last_outline_calls = _count_then_fill("gr_class_outlines", attempt, cap, lambda E: E > 0 or V > 0, self._check)
        if check:
            self._check_faces("gr_class_outlines", stats, GR_OUTL_STAT_BAD_FACES, V)
        if cap == 0 and self.last_outline_calls == 1:
            result[2].zero_()   # ring_offsets of a call that had nothing to fill and no room to write the one 0
        return result

    def member_outlines(self, verts_q, faces, face_ptr, face_members, n_classes: int, capacity: Optional[int] = None,
                        check: bool = True):
        """gr_member_outlines: verts_q (V, 2) int64 snapped vertices, faces (F, 3) int and the
        face-major CSR of a face x class membership as `set_cover` takes it -- face_ptr (F + 1,) int64, face_members (nnz,) int32,
        strictly ascending within a row; a member outside [0, n_classes) takes no part -- numpy or device tensors -> the 5-tuple of
        `class_outlines`: the rings of every class, class after class, as `class_outlines` traces each class alone.  One library
        call whatever the number of classes (count-then-fill; the default offer is 3 nnz ring vertices, which always fits --
        a member contributes at most its 3 edges --: 20 bytes per member beside the 132 bytes of scratch the call takes per
        member anyway, where an offer that proved too small would cost a second whole trace; `capacity` offers less).  `check`
        (default) raises ValueError when a face names a vertex that does not exist or the table is malformed
        (GR_OUTL_STAT_BAD_ROWS; the library then wrote nothing); with check=False a malformed table gives an empty result and
        the non-zero word."""
        torch = _torch()
        vq_t, f_t = self._mesh_2d(verts_q, faces)
        ptr_t = self._dev(face_ptr, torch.int64).reshape(-1)
        mem_t = self._dev(face_members, torch.int32).reshape(-1)
        V, F, nnz = int(vq_t.shape[0]), int(f_t.shape[0]), int(mem_t.shape[0])
        if int(ptr_t.shape[0]) != F + 1:
            raise ValueError(f"gr_member_outlines: face_ptr must hold F + 1 = {F + 1} offsets, got {int(ptr_t.shape[0])}")
        if not 0 <= int(n_classes) <= GR_MEMBER_MAX_CLASSES:
            raise ValueError(f"gr_member_outlines: n_classes={int(n_classes)} outside [0, {GR_MEMBER_MAX_CLASSES}]")
        if 3 * nnz >= 2 ** 31:
            raise ValueError(f"gr_member_outlines: {nnz} members, one call takes fewer than 2^31 / 3")
        stats = self._stats(GR_OUTL_STAT_WORDS)
        n_edges, n_rings = ctypes.c_int64(0), ctypes.c_int64(0)

        def attempt(cap):
            canon = self._empty((V,), torch.int32)
            ring_vertices = self._empty((max(cap, 1),), torch.int32)
            ring_offsets = self._empty((cap // 3 + 1,), torch.int64)
            ring_class = self._empty((max(cap // 3, 1),), torch.int32)
            rc = self._rc("gr_member_outlines", vq_t.data_ptr(), V, f_t.data_ptr(), F, ptr_t.data_ptr(),
                          _ptr(mem_t if nnz else None), nnz, int(n_classes),
                          *(_ptr(t if cap else None) for t in (canon, ring_vertices, ring_offsets, ring_class)), cap,
                          ctypes.byref(n_edges), ctypes.byref(n_rings), stats.data_ptr(), self._stream())
            E, R = int(n_edges.value), int(n_rings.value)
            return rc, E, (canon, ring_vertices[:E], ring_offsets[:R + 1], ring_class[:R], stats)

        cap = 3 * nnz if capacity is None else int(capacity)
        self.last_outline_calls = 0
        result, self.last_outline_calls = _count_then_fill("gr_member_outlines", attempt, cap, lambda E: E > 0 or V > 0, self._check)
        on_host = stats.cpu()   # the one read of both words
        if check:
            self._check_faces("gr_member_outlines", on_host, GR_OUTL_STAT_BAD_FACES, V)
            n_bad = int(on_host[GR_OUTL_STAT_BAD_ROWS])
            if n_bad:
                raise ValueError(f"gr_member_outlines: {n_bad} violations of a well-formed member table (face_ptr rises from 0 to "
                                 f"{nnz}, the members of a row strictly ascend)")
        if int(on_host[GR_OUTL_STAT_BAD_ROWS]) or (cap == 0 and self.last_outline_calls == 1):
            result[2].zero_()   # ring_offsets of a call that wrote nothing: a malformed table, or nothing to fill and no room
        return result

    # -- raster samples: the value of a raster under every face centre or vertex -----------------------------------
    def sample_raster(self, points, faces, raster_data, inverse6, nodata, fill, *, want_values: bool = True,
                      want_height: bool = False, labels=None, threshold=None, ground_id=None, only_existing: bool = False,
                      check: bool = True):
        """gr_sample_raster (DESIGN.md "Raster samples"): points (V, 3) float64 in the raster's CRS; faces (F, 3) int for a query
        per face centre, None for a query per vertex; raster_data (B, H, W) or (H, W), float32 or float64 (anything else is
        converted to float64); inverse6: the six coefficients of the INVERSE transform (`PlanarRaster.inverse`); nodata a float or
        None; fill what a sample equal to nodata becomes -- numpy or device tensors -> (values (N, B) float64 tensor or None,
        height (N,) float64 tensor or None, labels or None, stats (GR_RS_STAT_WORDS,) int64 tensor).  `labels` ((N,) or (N, 1)
        float64) with `threshold` and `ground_id` are relabelled: a DEVICE float64 contiguous tensor is rewritten in place and
        returned, anything else is copied to the device first.  `check` (default) reads the statistics back and raises ValueError
        when a face names a vertex that does not exist; check=False only enqueues."""
        torch = _torch()
        p_t, f_t, V, N = self._points_faces(points, faces)
        raster_data, dtype_name, raster_dtype = _float_kind(raster_data)
        r_t = self._dev(raster_data, getattr(torch, dtype_name))
        if r_t.ndim == 2:
            r_t = r_t[None]
        if r_t.ndim != 3 or min(r_t.shape) < 1:
            raise ValueError(f"raster data must be (B, H, W) or (H, W) with no empty axis, got {tuple(r_t.shape)}")
        B, H, W = (int(v) for v in r_t.shape)
        inv = [float(v) for v in np.asarray(inverse6, dtype=np.float64).reshape(-1)]
        if len(inv) != 6:
            raise ValueError(f"the inverse transform has six coefficients, got {len(inv)}")
        inv_h = (ctypes.c_double * 6)(*inv)
        lab_t = None
        if labels is not None:
            if threshold is None or ground_id is None:
                raise ValueError("labels need threshold and ground_id")
            lab_t = self._dev(labels, torch.float64)
            if lab_t.numel() != N or lab_t.ndim > 2:
                raise ValueError(f"labels must be ({N},) or ({N}, 1), got {tuple(lab_t.shape)}")
        values = self._empty((N, B), torch.float64) if want_values else None
        height = self._empty((N,), torch.float64) if want_height else None
        stats = self._stats(GR_RS_STAT_WORDS, zeroed=True)
        if N > 0:   # (an empty tensor has no address: null faces would mean vertex mode)
            self._call("gr_sample_raster", p_t.data_ptr(), V, _ptr(f_t), 0 if f_t is None else N, r_t.data_ptr(),
                       raster_dtype, B, H, W, ctypes.addressof(inv_h), 0 if nodata is None else 1,
                       0.0 if nodata is None else float(nodata), float(fill), _ptr(values), _ptr(height), _ptr(lab_t),
                       float("nan") if threshold is None else float(threshold),
                       float("nan") if ground_id is None else float(ground_id),
                       GR_RS_FLAG_ONLY_EXISTING if only_existing else 0, stats.data_ptr(), self._stream())
            if check:
                self._check_faces("gr_sample_raster", stats, GR_RS_STAT_BAD_FACES, V)
        return values, height, lab_t, stats

    # -- CRS reprojection: points between the WGS84 systems ------------------------------------------------------------
    def reproject_points(self, points, from_crs, to_crs, faces=None, pre_transform=None, out=None, check: bool = True):
        """gr_reproject_points (DESIGN.md "CRS reprojection"): points (V, 3) float64 in `from_crs` -> ((N, 3) float64 device tensor
        in `to_crs`, stats (GR_CRS_STAT_WORDS,) int64 tensor).  from_crs / to_crs: what `geograypher_amd.utils.geospatial.WGS84CRS.parse`
        takes; geographic rows are (lon, lat, h) here whatever the authority's axis order.  faces (F, 3) int: a row per face, the
        mean of its reprojected vertices; None: a row per vertex.  pre_transform: a 4 x 4 applied to the input first (ECEF source
        only).  out: a device float64 (N, 3) contiguous tensor to write -- `points` itself (a device tensor, without faces)
        converts in place.  `check` (default) reads the statistics back and raises ValueError when a face names a vertex that does
        not exist; check=False only enqueues.  Rows that cannot be converted are NaN and counted in the statistics."""
        from geograypher_amd.utils.geospatial import crs_tuple

        torch = _torch()
        p_t, f_t, V, N = self._points_faces(points, faces)
        sides = [Crs(int(k), float(lon0), float(k0), float(fe), float(fn)) for k, lon0, k0, fe, fn in
                 (crs_tuple(from_crs), crs_tuple(to_crs))]
        pre_h = None
        if pre_transform is not None:
            pre = np.asarray(_host_array(pre_transform), dtype=np.float64)
            if pre.shape != (4, 4):
                raise ValueError(f"pre_transform must be (4, 4), got {pre.shape}")
            pre_h = (ctypes.c_double * 16)(*pre.reshape(-1).tolist())
        if out is None:
            out = self._empty((N, 3), torch.float64)
        elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != (N, 3)
              or not out.is_contiguous() or out.device != p_t.device):
            raise ValueError(f"out must be a contiguous float64 ({N}, 3) tensor on {p_t.device}")
        stats = self._stats(GR_CRS_STAT_WORDS, zeroed=True)
        if N > 0:   # (an empty tensor has no address: null faces would mean vertex mode)
            self._call("gr_reproject_points", _ptr(p_t if V else None), V, _ptr(f_t), 0 if f_t is None else N,
                       None if pre_h is None else ctypes.addressof(pre_h), ctypes.byref(sides[0]), ctypes.byref(sides[1]),
                       out.data_ptr(), stats.data_ptr(), self._stream())
            if check and f_t is not None:
                self._check_faces("gr_reproject_points", stats, GR_CRS_STAT_BAD_FACES, V)
        return out, stats

    # -- raster -> raster: a window of a destination grid resampled from a source raster (include/geograster_warp.h) --
    def warp_raster(self, data, src_inverse, src_nodata, dst_transform, window, *, src_crs=None, dst_crs=None,
                    resampling: str = "nearest", dst_nodata=None, dst_dtype=None, out=None):
        """gr_warp_raster (W1-W9): data (B, H, W) or (H, W), uint8, float32 or float64 (anything else is converted to float64),
        numpy or a device tensor; src_inverse: the six coefficients of the source's INVERSE transform (`PlanarRaster.inverse`);
        src_nodata a float or None; dst_transform: the six coefficients of the destination's parent grid; window (col_off, row_off,
        width, height) of it -> (out (B, height, width) device tensor of `dst_dtype` (default: the source's), stats
        (GR_WARP_STAT_WORDS,) int64 tensor).  src_crs, dst_crs: what `utils.geospatial.WGS84CRS.parse` takes, given together for a
        cross-CRS warp (geographic grids are lon, lat: x is the longitude) or both None where the grids share a CRS.  resampling
        "nearest" or "bilinear" (four taps, nodata taps left out and the rest renormalised).  dst_nodata: what a cell without a
        sample becomes (default: src_nodata, else NaN, 0 for uint8).  out: a contiguous device tensor of the result's shape and
        dtype to write.  Only enqueues."""
        return RasterWarper(self).warp(data, src_inverse, src_nodata, dst_transform, window, src_crs, dst_crs, resampling, dst_nodata,
                                       dst_dtype, out)

    # -- the face sieve: components of equally labelled faces, small ones merged into their greatest neighbour --
    def face_sieve(self, faces, classes, weights=None, min_measure=0, fill_unlabelled: bool = False, vertex_canon=None,
                   max_rounds: int = 64, n_vertices: Optional[int] = None, out=None):
        """gr_face_sieve (I1-I10): faces (F, 3) int, classes (F,) int (< 0: unlabelled), weights (F,) int64 >= 0 or None for 1 per
        face, numpy or device tensors -> (class_out (F,) int32 tensor, comp (F,) int32 tensor: the smallest face of the face's
        component in the final labelling, -1 for a face that takes no part, stats (GR_SIEVE_STAT_WORDS,) int64 tensor), on the
        call's stream.  min_measure = 0: the component labelling alone.  vertex_canon (V,) int: corner v stands for vertex_canon[v].
        V is len(vertex_canon), else `n_vertices`, else the largest corner + 1 (which reads the faces back).  out: the classes
        tensor itself, to sieve in place.  The weights are checked on the host first (none negative, sum < 2^62: ValueError).
        Waits for the stream once per round."""
        return FaceSieve(self).sieve(faces, classes, weights, min_measure, fill_unlabelled, vertex_canon, max_rounds, n_vertices, out)

    # -- nearest points: for every query row the nearest ref row, exact ---------------------------------------
    def nearest_points(self, ref, query, *, max_distance=None, cell: float = 0.0, max_rings: int = 2, return_dist2: bool = False):
        """gr_nearest_points (K1-K9): ref (R, 3), query (Q, 3) float64, numpy or device tensors -> (index (Q,) int32 tensor: the
        row of the nearest ref, the lowest among equally near ones, -1 where there is none; [dist2 (Q,) float64 tensor with
        `return_dist2`: K2's squared distance, NaN beside -1;] stats (GR_NN_STAT_WORDS,) int64 tensor), on the call's stream.
        Rows with a NaN or infinite coordinate take no part (ref) or get -1 (query).  max_distance: answers farther than it
        become -1 (one exactly at it stays).  cell (0: chosen by the call) and max_rings steer the search only, never the answer.
        Waits for the stream once for the bounds and once per grid level."""
        return NearestPoints(self).query(ref, query, max_distance, cell, max_rings, return_dist2)

    # -- the orthomosaic baseline: tile assembly, zonal class counts ----------------------------------------------------
    def assemble_tiles(self, preds, pred_offsets, windows, tile_table, weights, weight_offsets, count_dtype, bin_table,
                       width: int, height: int, num_classes: int, nodataval: int, row0: int = 0, n_rows: Optional[int] = None,
                       want_counts: bool = False):
        """gr_assemble_tiles: preds uint8 concatenated tile predictions (values that are no class: 255),
        pred_offsets (T + 1,) int64, windows (T, 4) int col_off row_off width height in extent coordinates, tile_table (T,) int,
        weights: the tables concatenated in `count_dtype` (np.uint8, np.uint16 or float), weight_offsets (n_tables + 1,) int64,
        bin_table = (bin_ptr, bin_tiles, bin_side, bins_x, bins_y) of `utils.geometric.tile_bin_table` -- numpy or device tensors
        -> (classes (n_rows, width) uint8 tensor, counts (C, n_rows, width) tensor of the count type or None, stats
        (GR_ORTHO_STAT_WORDS,) int64 tensor: pixels with a class, without, most tiles over a pixel, (tile, pixel) pairs read).
        The rows are [row0, row0 + n_rows) of the `height` rows of the extent (default: all).  The tables are validated on the
        host first (`check_assemble_tables`: ValueError).  Only enqueues."""
        torch = _torch()
        kind, np_dtype, t_dtype = _count_kind(count_dtype)
        n_rows = int(height) - int(row0) if n_rows is None else int(n_rows)
        bin_ptr, bin_tiles, bin_side, bins_x, bins_y = bin_table
        po_h, win_h, tt_h, wo_h, bp_h, bt_h = (_host_array(x) for x in (pred_offsets, windows, tile_table, weight_offsets, bin_ptr,
                                                                        bin_tiles))
        p_t = self._dev(preds, torch.uint8).reshape(-1)
        w_t = self._dev(weights, t_dtype).reshape(-1)
        check_assemble_tables(po_h, win_h, tt_h, wo_h, int(p_t.shape[0]), int(w_t.shape[0]), bp_h, bt_h, int(bin_side), int(bins_x),
                              int(bins_y), int(width), int(height), int(row0), n_rows, int(num_classes), int(nodataval))
        T = int(tt_h.shape[0])
        po_t, wo_t, bp_t = (self._dev(x, torch.int64).reshape(-1) for x in (pred_offsets, weight_offsets, bin_ptr))
        win_t, tt_t, bt_t = (self._dev(x, torch.int32).reshape(-1) for x in (windows, tile_table, bin_tiles))
        C = int(num_classes)
        classes = self._empty((n_rows, int(width)), torch.uint8)
        counts = self._empty((C, n_rows, int(width)), t_dtype) if want_counts else None
        stats = self._stats(GR_ORTHO_STAT_WORDS)
        self._call("gr_assemble_tiles", _ptr(p_t if p_t.numel() else None), int(p_t.shape[0]), po_t.data_ptr(),
                   _ptr(win_t if T else None), _ptr(tt_t if T else None), T, _ptr(w_t if w_t.numel() else None), int(w_t.shape[0]),
                   wo_t.data_ptr(), int(wo_t.shape[0]) - 1, kind, bp_t.data_ptr(), _ptr(bt_t if bt_t.numel() else None),
                   int(bt_t.shape[0]), int(bin_side), int(bins_x), int(bins_y), int(width), int(row0), n_rows, C, int(nodataval),
                   _ptr(classes if classes.numel() else None), _ptr(counts if counts is not None and counts.numel() else None),
                   stats.data_ptr(), self._stream())
        return classes, counts, stats

    def zonal_class_counts(self, raster, nodata, ring_vertices, ring_offsets, ring_polygon, n_polygons: int, items, num_classes: int):
        """gr_zonal_class_counts: raster (H, W) uint8, nodata an int in [0, 255] or None, the ring table in
        pixel coordinates times 65536 (`utils.geospatial.rings_to_cell_units`: ring_vertices (N, 2) int64, ring_offsets (R + 1,)
        int64, ring_polygon (R,) int non-decreasing), items (n, GR_ZONAL_ITEM_INTS) int32 of `utils.geometric.zonal_work_items` --
        numpy or device tensors -> (counts (n_polygons, num_classes) int64 tensor, stats (GR_ZONAL_STAT_WORDS,) int64 tensor).
        The tables are validated on the host first (`check_zonal_tables`: ValueError).  Only enqueues."""
        torch = _torch()
        if not isinstance(raster, torch.Tensor):
            raster = np.asarray(raster)
        if str(raster.dtype).split(".")[-1] != "uint8":
            raise ValueError(f"gr_zonal_class_counts: the raster must be uint8, got {raster.dtype}")
        r_t = self._shaped(raster, torch.uint8, ("H", "W"), "raster")
        H, W = int(r_t.shape[0]), int(r_t.shape[1])
        rv_h, off_h, rp_h, it_h = (_host_array(x) for x in (ring_vertices, ring_offsets, ring_polygon, items))
        P, C = int(n_polygons), int(num_classes)
        check_zonal_tables(H, W, nodata, rv_h, off_h, rp_h, P, it_h, C)
        t = self._ring_table(ring_vertices, ring_offsets, ring_polygon, n_polygons=P)
        it_t = self._shaped(items, torch.int32, ("n", GR_ZONAL_ITEM_INTS), "work items")
        counts = self._empty((P, C), torch.int64)
        stats = self._stats(GR_ZONAL_STAT_WORDS)
        self._call("gr_zonal_class_counts", r_t.data_ptr(), H, W, zonal_nodata(nodata),
                   _ptr(t.rv if t.N else None), t.N, t.off.data_ptr(), _ptr(t.rp if t.R else None), t.R, P,
                   _ptr(it_t if it_t.numel() else None), int(it_t.shape[0]), C, _ptr(counts if P else None), stats.data_ptr(),
                   self._stream())
        return counts, stats

    def polygon_burner(self, ring_vertices, ring_offsets, ring_polygon, n_polygons: int, values=None) -> "PolygonBurner":
        """A `PolygonBurner` over the ring table in cell units of a parent raster grid (`utils.geospatial.rings_to_cell_units`) and
        `values` (n_polygons,) integers in [0, 255], or None for a burner of row planes only: the tables are checked
        (`check_burn_tables`: ValueError naming gr_burn_polygons) and uploaded once; every `.window` call burns one window."""
        return PolygonBurner(self, ring_vertices, ring_offsets, ring_polygon, n_polygons, values)

    def polygon_overlap(self, table_a, table_b) -> "PolygonOverlap":
        """A `PolygonOverlap` over two ring tables behind ONE origin (`utils.geometric.snap_polygon_pair`), each the five arrays of
        `PlanarPolygons.snapped`: the tables are checked (`check_overlap_tables`: ValueError naming gr_polygon_overlap_areas) and
        uploaded once; `.pairs()` lists the candidate pairs, `.areas(pairs, items)` gives the overlap area of every pair."""
        return PolygonOverlap(self, table_a, table_b)

    def ring_simplifier(self) -> "RingSimplifier":
        """A `RingSimplifier` on this backend: `.simplify(ring_vertices, ring_offsets, tol_meters, fixed=None)` is the exact
        Douglas-Peucker of DESIGN.md 8q (`utils.geometric.simplify_rings` and the `simplified` methods go through it)."""
        return RingSimplifier(self)

    def nadir_rasterizer(self, verts_q, z, faces) -> "NadirRasterizer":
        """A `NadirRasterizer` over a mesh seen from above: verts_q (V, 2) int64, the vertices' x, y in 1/65536 of a cell of a
        parent raster grid (`utils.geospatial.points_to_cell_units`), z (V,) float64 and faces (F, 3) int32.  The tables are
        validated on the host (`check_nadir_tables`: ValueError naming gr_nadir_raster) and uploaded once; every
        `.window(col_off, row_off, width, height, small_cells=0, item_rows=0)` call rasters one window."""
        return NadirRasterizer(self, verts_q, z, faces)

    # -- pictures (include/geograster_vis.h) --------------------------------------------------------
    def face_light(self, verts, faces, view_dir, ambient: float = 0.3):
        """The two-sided headlight per face (V3): verts (V, 3) float32, faces (F, 3) int32, view_dir a unit vector in the
        vertices' frame -> (F,) uint8 tensor, floor((ambient + (1 - ambient) |n.d| / |n|) 255 + 0.5); 255 for a face without area."""
        return PictureCalls(self).face_light(verts, faces, view_dir, ambient)

    def shade_view(self, ids, depth, face_rgb, face_light, supersample: int = 1, radius: Optional[int] = None, strength: float = 0.0,
                   background=(255, 255, 255)):
        """One shaded, anti-aliased picture (V4-V7): ids (H s, W s) int32 and depth (H s, W s) float32 as `raster_face_ids(...,
        want_depth=True)` gives them for one view, face_rgb (F, 3) uint8, face_light (F,) uint8, s = supersample in 1 .. 4, the
        neighbour radius in samples (default: s), the occlusion strength (0: none) -> (H, W, 3) uint8 tensor.  ValueError
        for planes whose sides are no multiple of s, and for what the library refuses."""
        return PictureCalls(self).shade_view(ids, depth, face_rgb, face_light, supersample, radius, strength, background)

    def composite_labels(self, photo, label, table=None, discrete: bool = False, shift: float = 0.0, scale: float = 1.0,
                         weight: float = 0.5, grey_overlay: bool = True):
        """The three-panel composite (V8-V12): photo (h, w, 3) uint8 or float64, label (h, w) or (h, w, 3) uint8 or float64 (other
        dtypes become float64), table (N, 3) float64 for a one-channel label -> (h, 3 w, 3) uint8 tensor [label colours | photo |
        overlay].  `shift` and `scale` are the two scalars of a continuous label (`utils.visualization.create_composite` computes
        them).  ValueError for a uint8 colour label with discrete classes, and for shapes that do not fit."""
        return PictureCalls(self).composite_labels(photo, label, table, discrete, shift, scale, weight, grey_overlay)

    # -- projection / aggregation --------------------------------------------------------------------------------
    def new_vote_buffers(self, C: int):
        torch = _torch()
        votes = self._zeros((self.n_faces, C), torch.int32)  # uint32 payload
        counts = self._zeros((self.n_faces,), torch.int32)
        return votes, counts

    def project_labels(self, ids, labels, C: int, votes, counts, neg1_is_last_face: bool = True):
        """ids (N,h,w) int32, labels (N,h,w) uint8 class indices; accumulates into votes (F,C), counts (F,)."""
        ids_t, lab_t = self._view_batch(ids, labels, _torch().uint8, "labels")
        n, h, w = (int(x) for x in ids_t.shape)
        self._call("gr_project_labels_u8", ids_t.data_ptr(), lab_t.data_ptr(), n, h, w, C, votes.data_ptr(),
                   counts.data_ptr(), _flags(neg1_is_last_face), self._stream())

    def project_values(self, ids, img, sums, counts, neg1_is_last_face: bool = True):
        """ids (N,h,w) int32, img (N,h,w,C) float64; accumulates nansum into sums (F,C) and counts (F,)."""
        ids_t, img_t = self._view_batch(ids, img, _torch().float64, "img", channels=True)
        n, h, w = (int(x) for x in ids_t.shape)
        C = int(img_t.shape[-1])
        self._call("gr_project_values_f64", ids_t.data_ptr(), img_t.data_ptr(), n, h, w, C, sums.data_ptr(),
                   counts.data_ptr(), _flags(neg1_is_last_face), self._stream())

    def project_view(self, ids, img, neg1_is_last_face: bool = True):
        """One view of project_images: ids (h,w) int32, img (h,w,C) float64 -> (F,C) float64, NaN for unseen faces."""
        torch = _torch()
        ids_t = self._shaped(ids, torch.int32, ("h", "w"), "ids")
        h, w = (int(x) for x in ids_t.shape)
        img_t = self._shaped(img, torch.float64, (h, w, "C"), "img")
        C = int(img_t.shape[-1])
        tex = self._empty((self.n_faces, C), torch.float64)
        self._call("gr_project_view_f64", ids_t.data_ptr(), img_t.data_ptr(), h, w, C, tex.data_ptr(), _flags(neg1_is_last_face),
                   self._stream())
        return tex

    def raster_project_labels(self, cams, labels, C: int, votes, counts, ids_out=None, neg1_is_last_face: bool = True,
                              check: bool = True):
        """Fused pix2face + label projection for N views (aggregate_projected_images fast path): the face ids stay in
        the rasterizer's LDS tiles unless `ids_out` (N,h,w int32) is given.  Accumulates into votes / counts.
        `check` as in `raster_face_ids`: with `check=False` a launch group whose bins overflowed (and every later one) adds
        NO votes and nobody is told until `raster_status()` is asked."""
        torch = _torch()
        cams_t = self._dev(cams, torch.float32)
        lab_t = self._dev(labels, torch.uint8)
        n, h, w = (int(x) for x in lab_t.shape)
        if cams_t.shape[0] != n:
            raise ValueError(f"{cams_t.shape[0]} camera records for {n} label images")
        flags = _flags(neg1_is_last_face)
        # (after an overflow the votes of the first views_done views are in; the library skipped the rest on the device)
        self._checked_raster(n, check, lambda v0: self._call(
            "gr_raster_project_labels_u8", cams_t[v0:].data_ptr(), lab_t[v0:].data_ptr(), n - v0, h, w, C, votes.data_ptr(),
            counts.data_ptr(), _ptr(None if ids_out is None else ids_out[v0:]), flags, self._stream()))
        return ids_out

    # -- get_image(image_scale) behind the file read (row a5) -----------------------------------------------------
    _RESIZE_DTYPES = {"uint8": GR_DTYPE_U8, "float32": GR_DTYPE_F32, "float64": GR_DTYPE_F64}

    def resize_image(self, image, out_hw=None, divide_by_255: Optional[bool] = None):
        """cameras.py:154-174 on the device: `image` ((H,W) or (H,W,C); numpy or tensor, uint8 / float32 / float64, in the dtype
        its file holds) -> float64 tensor of shape out_hw (+ C): uint8 values are divided by 255.0 (`divide_by_255`, default:
        exactly when the dtype is uint8, as get_image does), then skimage.transform.resize with its defaults
        (gr_resize_image_f64: anti-aliasing Gaussian + order-1 sampling at half-pixel centres).  out_hw None or the input
        size: the conversion alone."""
        torch = _torch()
        if isinstance(image, torch.Tensor):
            t = image.to(self.device).contiguous()
        else:
            t = torch.as_tensor(np.ascontiguousarray(image)).to(self.device)
        if t.dtype == torch.bool:
            t = t.to(torch.uint8)
        name = str(t.dtype).replace("torch.", "")
        if name not in self._RESIZE_DTYPES:
            # every other dtype: widened to float64 first, values kept (scikit-image would rescale integer types by their
            # range and truncate the filtered image to the integer type; not reproduced: documented in DESIGN.md)
            t, name = t.to(torch.float64), "float64"
        if t.ndim not in (2, 3):
            raise ValueError(f"image must be (H,W) or (H,W,C), got shape {tuple(t.shape)}")
        h_in, w_in = int(t.shape[0]), int(t.shape[1])
        C = 1 if t.ndim == 2 else int(t.shape[2])
        h_out, w_out = (h_in, w_in) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        if divide_by_255 is None:
            divide_by_255 = name == "uint8"
        out = self._empty((h_out, w_out) + tuple(t.shape[2:]), torch.float64)
        self._call("gr_resize_image_f64", t.data_ptr(), self._RESIZE_DTYPES[name], h_in, w_in, C, 1 if divide_by_255 else 0,
                   h_out, w_out, out.data_ptr(), self._stream())
        return out

    # -- 360-degree photos: perspective views of an equirectangular image -------------------------------------------
    equirect_uploads = 0   # photos this backend sent to the device (equirect_upload): one per photo, however many views

    class EquirectSource:
        """An equirectangular photo resident on the device, with what every view of it needs (utils/image.py:89-104 and
        skimage's clip range): the file-dtype tensor, the value range and the per-channel normalised clip bounds."""

        def __init__(self, tensor, np_dtype, squeeze, vmin, vrange, bounds):
            self.tensor, self.np_dtype, self.squeeze = tensor, np_dtype, squeeze
            self.vmin, self.vrange, self.bounds = vmin, vrange, bounds
            self.shape = tuple(tensor.shape)

    def equirect_upload(self, equi_img):
        """(H, W) or (H, W, C) uint8 / float64 numpy image -> `EquirectSource`.  The photo crosses the link once, in its file
        dtype; its range and channel bounds are reduced on the device."""
        torch = _torch()
        img = np.asarray(equi_img)
        if img.dtype == bool:
            img = img.astype(np.uint8)
        if img.dtype not in (np.uint8, np.float64):
            raise NotImplementedError(f"equirectangular source dtype {img.dtype} is not supported (uint8 or float64)")
        if img.ndim not in (2, 3) or img.size == 0:
            raise ValueError(f"equi_img must be a non-empty (H, W) or (H, W, C) image, got shape {img.shape}")
        squeeze = img.ndim == 2
        t = torch.as_tensor(np.ascontiguousarray(img)).to(self.device)
        self.equirect_uploads += 1
        if squeeze:
            t = t[..., None]
        t = t.contiguous()
        C = int(t.shape[2])
        flat = t.reshape(-1, C)
        # exact in float64 for both dtypes: min / max select values, the normalisation below is image.py:102 on 2 C numbers
        ch = torch.stack([flat.min(dim=0).values, flat.max(dim=0).values], dim=1).to(torch.float64).cpu().numpy()
        vmin = min(float(ch[:, 0].min()), 0.0)
        vmax = max(float(ch[:, 1].max()), 0.0)
        vrange = vmax - vmin
        bounds = None
        if vrange > 0:
            norm = (ch - vmin) / vrange
            nfill = (0.0 - vmin) / vrange
            norm[:, 0] = np.minimum(norm[:, 0], nfill)
            norm[:, 1] = np.maximum(norm[:, 1], nfill)
            bounds = torch.as_tensor(np.ascontiguousarray(norm)).to(self.device)
        return self.EquirectSource(t, img.dtype, squeeze, vmin, vrange, bounds)

    def equirect_view(self, source, x, y, rot, output_size, oversample_factor: int = 1, order: int = 1,
                      return_mask: bool = False, return_debug: bool = False):
        """One perspective view of a device-resident equirectangular photo (gr_equirect_view; utils/image.py:129-267): numpy
        (out_h, out_w[, C]) -- float64, or the source dtype at oversample_factor 1 --, then the (H, W) bool sampling mask when
        asked for, then {"ij": (2, ny, nx) float64} when `return_debug`.  x, y: the host-computed ray coordinates of the
        oversampled view; rot: the 3 x 3 matrix of rotate_by_roll_pitch_yaw."""
        torch = _torch()
        if order not in (0, 1):
            raise NotImplementedError(f"warp_order {order} is not implemented on the device (0 or 1)")
        out_h, out_w = int(output_size[0]), int(output_size[1])
        os_ = int(oversample_factor)
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if len(x) != int(out_w * oversample_factor) or len(y) != int(out_h * oversample_factor) or os_ != oversample_factor:
            raise ValueError(f"ray grid of {len(y)} x {len(x)} samples does not match an output of {out_h} x {out_w} at "
                             f"oversampling {oversample_factor}")
        H, W, C = source.shape
        native = os_ == 1
        res = []
        with torch.cuda.device(self.device):
            mask = self._zeros((H, W + 1), torch.uint8) if return_mask else None
            dbg = self._empty((2, len(y), len(x)), torch.float64) if return_debug else None
            vrange, bounds = source.vrange, source.bounds
            if vrange == 0 and (return_mask or return_debug):   # the coordinates are still wanted: a unit range samples zeros
                vrange, bounds = 1.0, self._zeros((C, 2), torch.float64)
            if vrange == 0:   # image.py:94-97: no variation, the fill everywhere; nothing to launch
                out = self._zeros((out_h, out_w, C), source.tensor.dtype if native else torch.float64)
            else:
                out = self._empty((out_h, out_w, C), source.tensor.dtype if native else torch.float64)
                xy = torch.as_tensor(np.concatenate([x, y])).to(self.device)
                R = (ctypes.c_double * 9)(*[float(v) for v in np.asarray(rot, dtype=np.float64).reshape(9)])
                dtype = GR_DTYPE_U8 if source.np_dtype == np.uint8 else GR_DTYPE_F64
                self._call("gr_equirect_view", source.tensor.data_ptr(), dtype, H, W, C, xy.data_ptr(),
                           xy.data_ptr() + 8 * len(x), R, out_h, out_w, os_, int(order), source.vmin, vrange,
                           bounds.data_ptr(), out.data_ptr(), _ptr(mask), _ptr(dbg), self._stream())
            if mask is not None:   # image.py:261-265: the appended column belongs to column 0
                mask[:, 0] |= mask[:, W]
                mask = mask[:, :W]
        arr = out.cpu().numpy()
        res.append(arr[..., 0] if (source.squeeze or C == 1) else arr)
        if return_mask:
            res.append(mask.cpu().numpy().astype(bool))
        if return_debug:
            res.append({"ij": dbg.cpu().numpy()})
        return res[0] if len(res) == 1 else tuple(res)

    # -- distortion warp (row f1) --------------------------------------------------------------------------------
    def upload_map(self, inverse_map):
        """(2, H, W) float64 sampling map (rows, cols) -> device tensor."""
        return self._shaped(inverse_map, _torch().float64, (2, "H", "W"), "sampling map")

    LENS_PARAMS = ("f", "cx", "cy", "image_width", "image_height", "k1", "k2", "k3", "k4", "p1", "p2", "b1", "b2")

    def invert_distortion(self, params: dict, h: int, w: int, image_scale: float = 1.0, max_iters: int = 12,
                          fill: float = -1.0):
        """(2, h, w) float64 device map: for every pixel of the warped image the position to sample in the ideal image
        (gr_invert_distortion_f64: dense Newton inverse of the Metashape lens model; replaces the host griddata inversion
        of cameras.py:1045-1062)."""
        torch = _torch()
        unknown = set(params) - set(self.LENS_PARAMS)
        if unknown:
            raise ValueError(f"Unexpected distortion params found: {sorted(unknown)}")
        par = (ctypes.c_double * 13)(*[float(params.get(k, 0.0)) for k in self.LENS_PARAMS])
        out = self._empty((2, h, w), torch.float64)
        self._call("gr_invert_distortion_f64", par, int(h), int(w), float(image_scale), int(max_iters), float(fill),
                   out[0].data_ptr(), out[1].data_ptr(), self._stream())
        return out

    def warp_image(self, input_image, map_t, order: int = 1, fill_value: float = 0.0,
                   reference_float_roundtrip: bool = False):
        """Resample `input_image` ((I,J) or (I,J,C)) through the (2,H,W) device map: utils/image.py:72-126 on device.

        Integer images with order 0 are gathered as integers (gr_warp_nearest_i32); everything else goes through the
        float64 kernel and is cast back to the input dtype by truncation like the reference's `.astype(initial_dtype)`.
        A NaN or infinite sampling coordinate reads `fill_value`, in both orders.  numpy in -> numpy out, tensor in ->
        tensor out.

        reference_float_roundtrip=True (the reference's float rescale and truncation, bit for bit) exists in the int32
        kernel only: order 0, an integer image within the int32 range, an integer fill value.  Every other combination
        raises NotImplementedError instead of returning the exact gather under the flag's name."""
        torch = _torch()
        is_tensor = isinstance(input_image, torch.Tensor)
        img = input_image if is_tensor else np.asarray(input_image)
        if img.ndim not in (2, 3):
            raise ValueError(f"image must be (I,J) or (I,J,C), got shape {tuple(img.shape)}")
        np_dtype = None if is_tensor else img.dtype
        h_out, w_out = int(map_t.shape[1]), int(map_t.shape[2])
        h_in, w_in = int(img.shape[0]), int(img.shape[1])
        is_int = (not torch.is_floating_point(img)) if is_tensor else np.issubdtype(img.dtype, np.integer) or img.dtype == bool
        # utils/image.py:86-96: an image without variation (fill included) is returned as a constant of the INPUT shape
        if is_tensor:
            vmin, vmax = float(img.min()), float(img.max())
        else:
            vmin, vmax = float(np.min(img)), float(np.max(img))
        lo, hi = min(vmin, float(fill_value)), max(vmax, float(fill_value))
        if hi - lo == 0:
            if is_tensor:
                return torch.full_like(img.squeeze(), fill_value)
            return np.full_like(np.squeeze(img), fill_value=fill_value)
        small_int = is_int and -2**31 <= lo and hi < 2**31 and float(fill_value) == int(fill_value)
        if reference_float_roundtrip and not (small_int and order == 0):
            raise NotImplementedError("reference_float_roundtrip=True is reproduced only for order 0 on integer images "
                                      "within the int32 range with an integer fill value")
        with torch.cuda.device(self.device):
            if small_int and order == 0:
                src = self._dev(img, torch.int32)
                squeeze = src.ndim == 2
                if squeeze:
                    src = src[..., None]
                outs = []
                for ch in range(src.shape[2]):
                    plane = src[..., ch].contiguous()
                    out = self._empty((h_out, w_out), torch.int32)
                    self._call("gr_warp_nearest_i32", plane.data_ptr(), h_in, w_in, map_t[0].data_ptr(), map_t[1].data_ptr(),
                               h_out, w_out, int(fill_value), 1 if reference_float_roundtrip else 0, lo, hi - lo,
                               out.data_ptr(), self._stream())
                    outs.append(out)
                res = outs[0] if squeeze else torch.stack(outs, dim=-1)
            else:
                src = self._dev(img, torch.float64)
                squeeze = src.ndim == 2
                if squeeze:
                    src = src[..., None]
                src = src.contiguous()
                C = int(src.shape[2])
                res = self._empty((h_out, w_out, C), torch.float64)
                self._call("gr_warp_f64", src.data_ptr(), h_in, w_in, C, map_t[0].data_ptr(), map_t[1].data_ptr(), h_out,
                           w_out, int(order), float(fill_value), res.data_ptr(), self._stream())
                if squeeze:
                    res = res[..., 0]
        if is_tensor:
            return res.to(img.dtype)
        return np.squeeze(res.cpu().numpy().astype(np_dtype))

    def finalize_votes(self, votes, counts):
        """(votes, counts) -> average (F,C), summed (F,C), counts (F,) float64 tensors (meshes.py:2069-2082)."""
        torch = _torch()
        F, C = int(votes.shape[0]), int(votes.shape[1])
        avg = self._empty((F, C), torch.float64)
        summed = self._empty((F, C), torch.float64)
        cnt = self._empty((F,), torch.float64)
        self._call("gr_finalize_votes", votes.data_ptr(), counts.data_ptr(), F, C, avg.data_ptr(), summed.data_ptr(),
                   cnt.data_ptr(), self._stream())
        return avg, summed, cnt

    def finalize_sums(self, sums, counts):
        torch = _torch()
        F, C = int(sums.shape[0]), int(sums.shape[1])
        avg = self._empty((F, C), torch.float64)
        cnt = self._empty((F,), torch.float64)
        self._call("gr_finalize_sums_f64", sums.data_ptr(), counts.data_ptr(), F, C, avg.data_ptr(), cnt.data_ptr(),
                   self._stream())
        return avg, sums, cnt

    def argmax_nonzero(self, array):
        """utils/indexing.py:9-32 on device: (F,C) -> (F,) float64.  float32 stays float32, as numpy sums it; every other
        dtype is converted to float64 -- exact for the integer vote arrays this is given while their partial row sums stay
        below 2^53.  The row sum follows numpy's pairwise order for a C-contiguous array; a Fortran-ordered array (which
        numpy sums left to right) is made C-contiguous here and summed in that order."""
        torch = _torch()
        array, dtype_name, dtype = _float_kind(array)
        arr = self._dev(array, getattr(torch, dtype_name))
        F, C = int(arr.shape[0]), int(arr.shape[1])
        out = self._empty((F,), torch.float64)
        self._call("gr_argmax_nonzero", arr.data_ptr(), dtype, F, C, out.data_ptr(), self._stream())
        return out
