/* geograster_simplify.h -- companion of geograster.h, which includes it inside its extern "C" block; do not include it on its own:
 * gr_ctx, the GR_* codes and the GR_SIMPLIFY_STAT_* enumerators are geograster.h's.  It holds the exact Douglas-Peucker simplification of polygon rings
 * (csrc/simplify.hip; the rule-set S1-S10 is DESIGN.md section 8q), which stands where the reference simplifies with shapely:
 * the region of interest of load_mesh (meshes.py:695), the class polygons of export_face_labels_vector (meshes.py:1241, 1417) and
 * the 0.05 m of batched_unary_union (utils/geometric.py:70-77).  GEOS is on no machine this library is built for, so the rule-set
 * is its own and callers ask for it by name (simplify_method="douglas-peucker").  The binding keeps the signature in a table of
 * its own (`_SIMPLIFY_SIGNATURES`), which tests/test_ring_simplify_host.py compares with this file.  The call needs no uploaded
 * mesh, uses the context's stage scratch (one call of a context at a time), reads one word back per pass (S4) and was added without
 * a GR_VERSION bump.  All arrays are DEVICE pointers. */
#ifndef GEOGRASTER_SIMPLIFY_H
#define GEOGRASTER_SIMPLIFY_H

/* Simplifies every ring of a ring table (S1): ring_vertices (n_ring_vertices x 2 int64) on the 1e-6 m grid, |value| <= 2^40, no
 * repeated closing vertex; ring_offsets (R + 1 int64, from 0 to n_ring_vertices, non-decreasing -- the CALLER guarantees it; a
 * table that breaks it reads and writes nothing outside the arrays, and its results mean nothing); fixed: n_ring_vertices uint8 or
 * null, non-zero where a vertex must stay (S2: the anchors of its ring; a ring without one is anchored at its lexicographically
 * smallest vertex); tol_steps: the tolerance T in grid steps, 0 <= T < 2^40.  A vertex is kept when it is an anchor or the farthest
 * interior vertex of a chain whose distance to the chain's chord exceeds T (S3, S4: the distance to the closed segment, compared
 * exactly; ties go to the smallest (x, y), then to the lowest index); a ring of which fewer than 3 vertices or no area is left
 * comes out empty (S6).
 * keep: n_ring_vertices uint8, 1 where the vertex is in the output.  kept_index: n_ring_vertices int32: the first M entries are
 * the kept vertices, ring after ring in input order, the others -1.  out_offsets: R + 1 int64, the output rings in kept_index; M =
 * out_offsets[R].  stats: GR_SIMPLIFY_STAT_WORDS uint64.  Every word of the four is written.
 * Synchronises `stream` once per pass, to read one word back (S4), and returns with the passes done and the last kernels enqueued
 * on it.  GR_EINVAL (the message names gr_simplify_rings), before any device work: null arrays, negative sizes, n_ring_vertices or
 * R >= 2^31 - 1, T outside [0, 2^40). */
int gr_simplify_rings(gr_ctx *ctx, const int64_t *ring_vertices, int64_t n_ring_vertices, const int64_t *ring_offsets, int64_t R,
                      const uint8_t *fixed, int64_t tol_steps, uint8_t *keep, int32_t *kept_index, int64_t *out_offsets,
                      uint64_t *stats, void *stream);

#endif /* GEOGRASTER_SIMPLIFY_H */
