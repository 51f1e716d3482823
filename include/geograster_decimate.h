/* geograster_decimate.h -- companion of geograster.h, which includes it inside its extern "C" block; do not include it on its own:
 * gr_ctx, the GR_* codes and the GR_DECIM_STAT_* enumerators are geograster.h's.  It holds the two calls of the mesh decimation
 * (csrc/decimate.hip; the rule-set D1-D9 is DESIGN.md section 8n), which stands where the reference decimates with VTK's quadric
 * decimation and carries vertex scalars over with a nearest-neighbour query (meshes/meshes.py:215-226, 288-323).  It is NOT that
 * algorithm: vertices are clustered on a uniform grid, in integers, and the kept vertices are a subset of the input's.  The binding
 * keeps the signatures in a table of its own (`_DECIMATE_SIGNATURES`), which tests/test_mesh_decimation_host.py compares with this
 * file.  Both calls only enqueue work on `stream`, need no uploaded mesh, keep every temporary in context scratch, and were added
 * without a GR_VERSION bump.  All arrays are DEVICE pointers. */
#ifndef GEOGRASTER_DECIMATE_H
#define GEOGRASTER_DECIMATE_H

/* verts_q: V x 3 int64 snapped vertices, units of 1e-6 m behind the per-axis minimum (q >= 0).  s: the cell side in grid steps,
 * 1 <= s <= 2^30.  Vertex i lies in cell c = q / s (floor: a vertex on a cell boundary belongs to the upper cell), key
 * cx << 42 | cy << 21 | cz; a vertex with q < 0 or a cell component >= 2^21 is OUTSIDE the key range and takes no cell.
 *
 * gr_cluster_count: *cells (1 uint64, written by the call) = the occupied cells: the probe of the search for a cell side. */
int gr_cluster_count(gr_ctx *ctx, const int64_t *verts_q, int64_t V, int64_t s, uint64_t *cells, void *stream);

/* gr_cluster_decimate: faces F x 3 int32.  rep (V int32, written by the call): the representative of every vertex' cell -- its
 * member with the smallest (d2, vertex index), d2 = sum over the axes of (2 (q - c s) - s)^2 --, -1 for a vertex outside the key
 * range.  Face (a, b, c) becomes (rep[a], rep[b], rep[c]); it is dropped when two of the three are equal (collapsed), and among the
 * surviving faces with the same SET of three representatives, whatever their winding, only the one with the lowest face index is
 * kept, with its own winding.  A face with a vertex index outside [0, V), or with a vertex outside the key range, reads nothing,
 * is counted in GR_DECIM_STAT_BAD_FACES and is dropped.  Kept faces keep their order; a representative is kept iff a kept face
 * uses it.  face_ids (capacity F int64) and point_ids (capacity V int64): the ascending original indices of what is kept;
 * new_faces (capacity F x 3 int32): the kept faces, indexing the kept vertices.  Entries behind the counts are not written.
 * stats: GR_DECIM_STAT_WORDS uint64, written by the call.  V = 0 or F = 0 is legal: nothing is kept (with V > 0, rep and the cell
 * count are still written).  Radix sorts and scans (hipcub) in context scratch, about 60 bytes per vertex or per face.
 * GR_EINVAL (the message names the call): null arrays, negative sizes, V or F >= 2^31, s outside [1, 2^30]. */
int gr_cluster_decimate(gr_ctx *ctx, const int64_t *verts_q, int64_t V, const int32_t *faces, int64_t F, int64_t s, int32_t *rep,
                        int64_t *face_ids, int64_t *point_ids, int32_t *new_faces, uint64_t *stats, void *stream);

#endif /* GEOGRASTER_DECIMATE_H */
