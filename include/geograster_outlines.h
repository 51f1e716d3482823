/* geograster_outlines.h -- companion of geograster.h, which includes it inside its extern "C" block; do not include it on its own:
 * gr_ctx, the GR_* codes and the GR_OUTL_* enumerators are geograster.h's.  It holds the outline calls added after geograster.h's
 * function list was closed (the C-ABI test pins that list and its binding table); the binding keeps their signatures in a table of
 * its own (`_COMPANION_SIGNATURES`), which tests/test_detection_footprints_host.py compares with this file. */
#ifndef GEOGRASTER_OUTLINES_H
#define GEOGRASTER_OUTLINES_H

/* Member outlines -- the outline rings of every class of a sparse face x class MEMBERSHIP (a face may be in any number of
 * classes): the detection footprints of project_detections, the ground footprint of every image from a visibility matrix; the
 * rule-set is DESIGN.md section 8l (Y1-Y5).  The trace behind the edge kernel is the one of gr_class_outlines.
 * face_ptr (F + 1 int64), face_members (nnz int32): a face-major CSR as gr_set_cover takes it; entry (f, c) says that face f
 * belongs to class c (no values).  Well-formed (Y2): face_ptr[0] == 0, face_ptr[F] == nnz, face_ptr non-decreasing, the members of
 * a row strictly ascending.  Every violation is counted in GR_OUTL_STAT_BAD_ROWS.  A malformed table causes no access out of
 * bounds and no read of uninitialised scratch: every row is clamped into [0, nnz], the class array is pre-filled with a word no
 * class reaches, AND the call stops at its first synchronisation when the word is non-zero: GR_OK, both totals 0, nothing written
 * but `stats`.  The caller reads the word.
 * A member takes part iff 0 <= c < n_classes, its face names existing vertices and the snapped triangle has a non-zero area;
 * GR_OUTL_STAT_NO_CLASS, _ZERO_AREA and _TURNED count MEMBERS (a member of a face with a bad index counts in none of them),
 * GR_OUTL_STAT_BAD_FACES counts faces.  The output equals the concatenation, in ascending class order, of what gr_class_outlines
 * returns for every class alone (Y5).  Outputs, capacity protocol, synchronisations and scratch as for gr_class_outlines (about 48
 * bytes per member corner).  Limits: V, F < 2^31, 3 nnz < 2^31, 0 <= n_classes <= GR_MEMBER_MAX_CLASSES.  GR_EINVAL (the message
 * names the call), before any device work: null arrays, negative sizes, a limit exceeded.  Added without a GR_VERSION bump. */
int gr_member_outlines(gr_ctx *ctx, const int64_t *verts_q, int64_t V, const int32_t *faces, int64_t F, const int64_t *face_ptr,
                       const int32_t *face_members, int64_t nnz, int32_t n_classes, int32_t *canon, int32_t *ring_vertices,
                       int64_t *ring_offsets, int32_t *ring_class, int64_t ring_vertex_cap, int64_t *n_edges_h, int64_t *n_rings_h,
                       uint64_t *stats, void *stream);

#endif /* GEOGRASTER_OUTLINES_H */
