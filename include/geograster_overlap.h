/* geograster_overlap.h -- companion of geograster.h, which includes it inside its extern "C" block; do not include it on its own:
 * gr_ctx, the GR_* codes and the GR_OVERLAP_* enumerators are geograster.h's.  It holds the polygon-on-polygon overlap areas
 * (csrc/overlap.hip; the rule-set A1-A9 is DESIGN.md section 8o), which stand where the reference's get_overlap_vector
 * (utils/geospatial.py:221-329) calls gpd.overlay and its cf_from_vector_vector (utils/prediction_metrics.py:95-144) calls
 * shapely's intersection.  The binding keeps the signatures in a table of its own (`_OVERLAP_SIGNATURES`), which
 * tests/test_polygon_overlap_host.py compares with this file.  The calls only enqueue work on `stream`, need no uploaded mesh, use
 * the context's stage scratch (one call of a context at a time) and were added without a GR_VERSION bump.  All arrays are DEVICE
 * pointers. */
#ifndef GEOGRASTER_OVERLAP_H
#define GEOGRASTER_OVERLAP_H

/* The candidate pairs of two box tables (A2), count then fill.  boxes_a: Pa x 4 int64 xmin ymin xmax ymax, boxes_b likewise; a
 * pair (a, b) is two rows whose boxes overlap with positive width AND positive height: boxes that only touch give no pair, the
 * empty box (1, 1, 0, 0) pairs with nothing.
 * gr_polygon_box_pairs_count writes offsets (Pa + 1 int64): offsets[a] pairs lie in front of row a's, offsets[Pa] is their number.
 * gr_polygon_box_pairs_fill takes those offsets back and writes pairs (n_pairs x 2 int32: a, b), ascending by (a, b); a slice that
 * would leave the n_pairs pairs is cut there.  GR_EINVAL (the message names the call), before any device work: null arrays,
 * negative sizes, Pa or Pb >= 2^31 - 1, n_pairs >= 2^31. */
int gr_polygon_box_pairs_count(gr_ctx *ctx, const int64_t *boxes_a, int64_t Pa, const int64_t *boxes_b, int64_t Pb, int64_t *offsets,
                               void *stream);
int gr_polygon_box_pairs_fill(gr_ctx *ctx, const int64_t *boxes_a, int64_t Pa, const int64_t *boxes_b, int64_t Pb,
                              const int64_t *offsets, int32_t *pairs, int64_t n_pairs, void *stream);

/* area(a n b) for the pairs of two ring tables.  Each table as gr_polygon_class_weights takes it (A1): ring_vertices
 * (n_ring_vertices x 2 int64) on the 1e-6 m grid behind ONE integer origin common to both tables, |value| <= 2^40, no repeated
 * closing vertex; ring_offsets (R + 1 int64); ring_polygon (R int32, non-decreasing); ring_is_hole (R int32); every ring
 * counter-clockwise, holes included (as PlanarPolygons.snapped stores them); polygon_boxes (P x 4 int64 xmin ymin xmax ymax over
 * the row's rings).  Rings of fewer than 3 vertices are ignored and counted.
 * pairs: n_pairs x 2 int32 (row of a, row of b), in any order.
 * items: n_items x GR_OVERLAP_ITEM_INTS int32 (A8): the index of a pair, the first edge slot and the number of slots (1 ..
 * GR_OVERLAP_TILE_A) of its row of a, the first slot and the number of slots (1 .. GR_OVERLAP_TILE_B) of its row of b.  Edge slot
 * i runs from ring vertex i to the next vertex of ITS ring, the last slot of a ring to the ring's first vertex; a tile may start
 * or end inside a ring and span several rings of the row.  The items of a pair must together name every (slot of a, slot of b)
 * once, and the items must name their pairs in non-decreasing order.  An item that is malformed, names no pair, names a pair
 * below one in front of it, or names a slot outside its rows is skipped whole and counted.
 * area, area_abs: n_pairs f64, every word written: the signed sum of the edge-pair integrals (A5, A6) and the sum of their
 * magnitudes, 0 for a pair without an item; |area - exact| <= K 2^-53 area_abs with the K of DESIGN.md 8o.  Deterministic (A7):
 * no floating-point atomics; the two values of a pair do not depend on where the pair or its items stand in the launch.
 * stats: GR_OVERLAP_STAT_WORDS uint64, written by the call (A9).  GR_EINVAL (the message names the call), before any device
 * work: null arrays, negative sizes, a count >= 2^31. */
int gr_polygon_overlap_areas(gr_ctx *ctx, const int64_t *ring_vertices_a, int64_t n_ring_vertices_a, const int64_t *ring_offsets_a,
                             const int32_t *ring_polygon_a, const int32_t *ring_is_hole_a, int64_t R_a, const int64_t *polygon_boxes_a,
                             int64_t P_a, const int64_t *ring_vertices_b, int64_t n_ring_vertices_b, const int64_t *ring_offsets_b,
                             const int32_t *ring_polygon_b, const int32_t *ring_is_hole_b, int64_t R_b, const int64_t *polygon_boxes_b,
                             int64_t P_b, const int32_t *pairs, int64_t n_pairs, const int32_t *items, int64_t n_items, double *area,
                             double *area_abs, uint64_t *stats, void *stream);

#endif /* GEOGRASTER_OVERLAP_H */
