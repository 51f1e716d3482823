/* geograster_communities.h -- companion of geograster.h, which includes it inside its extern "C" block; do not include it on its own:
 * gr_ctx, the GR_* codes and the GR_COMM_* enumerators are geograster.h's.  It holds the communities of the ray graph of the
 * multiview-detection workflow (csrc/communities.hip; the rule-set L1-L14 is DESIGN.md section 8p), which stand where the
 * reference's calc_communities (utils/numeric.py:509-619) calls networkx.community.louvain_communities.  The binding keeps the
 * signatures in a table of its own (`_COMMUNITIES_SIGNATURES`), which tests/test_communities_host.py compares with this file.  The
 * calls need no uploaded mesh, use the context's stage scratch (one call of a context at a time) and were added without a
 * GR_VERSION bump.  All arrays are DEVICE pointers. */
#ifndef GEOGRASTER_COMMUNITIES_H
#define GEOGRASTER_COMMUNITIES_H

/* A synchronous, deterministic Louvain on integer weights (L2-L13).
 * edge_i, edge_j (E int32), edge_q (E int64): the undirected edges of a graph of n vertices, n <= GR_COMM_MAX_VERTICES,
 * E < GR_COMM_MAX_EDGES; i != j, both in [0, n), 1 <= q <= 2^31 - 1; duplicates in either orientation are summed.  The inputs are
 * not modified.  An edge that breaks these conditions is found on the device: it is counted in GR_COMM_STAT_BAD_EDGES and the
 * call answers GR_EINDEX, the outputs other than `stats` then being undefined.  Twice the sum of the weights must stay below 2^53
 * (GR_EINVAL otherwise, with GR_COMM_STAT_M2 written): every sum of the rule-set is then exact in int64 and converts to double
 * exactly.
 * resolution: gamma of L5.  max_sweeps >= 1: the sweeps of a level (L9).  flags: the OR of GR_COMM_FORCE_*, which change the path
 * a row takes through the move kernel and nothing else.
 * community (n int32): the community of every vertex, -1 for a vertex without an edge; communities are numbered by falling size,
 * ties by the ascending lowest member (L12).  comm_size (int32), comm_in, comm_tot (int64), n entries each, of which the first
 * n_communities are written: the members of every community, the sum of A_uv over its members (both directions: twice its inner
 * weight) and the sum of its members' degrees.  The modularity follows on the host: sum over c of in_c / M2 - gamma (tot_c / M2)^2.
 * stats: GR_COMM_STAT_WORDS int64, written by every call that got past its argument checks: levels, sweeps and moves per level,
 * caps hit (reported, not an error), rows per path, bad edges, n_communities, M2.
 * The result is a function of the arguments alone: no floating-point sum, no result that depends on the order of an atomic.
 * The call reads the move count of every sweep back (one stream synchronisation per sweep, three more per level) and returns with
 * `stream` idle.  GR_EINVAL (the message names the call), before any device work: null arrays, n or E outside their limits,
 * max_sweeps < 1, a NaN resolution. */
int gr_louvain_communities(gr_ctx *ctx, const int32_t *edge_i, const int32_t *edge_j, const int64_t *edge_q, int64_t E, int64_t n,
                           double resolution, int32_t max_sweeps, int flags, int32_t *community, int32_t *comm_size, int64_t *comm_in,
                           int64_t *comm_tot, int64_t *stats, void *stream);

/* One 3-D point per community (L14): the mean of pA and pB over all ordered pairs (A, B) of distinct member segments, pA and pB being
 * the clamped closest points of the two segments -- the device function gr_ray_pairs thresholds the distance of, the host form of
 * which is utils/numeric.py segment_closest_points; what the reference's intersection_average (utils/numeric.py:330-347) returns.
 * starts, ends (n x 3 f64), community (n int32: a value outside [0, n_communities) names no community, as the -1 of
 * gr_louvain_communities), n <= GR_COMM_MAX_VERTICES, n_communities <= n.  points (n_communities x 3 f64), every word written: NaN
 * for a community of fewer than two segments.  One workgroup per community; the order of the sum is fixed (lane-strided pairs,
 * then a fixed tree), so two runs are bit-equal.  Synchronises `stream` behind its kernel: the scratch is free on return.
 * GR_EINVAL (the message names the call), before any device work: null arrays, sizes outside their limits. */
int gr_community_points(gr_ctx *ctx, const double *starts, const double *ends, const int32_t *community, int64_t n, int64_t n_communities,
                        double *points, void *stream);

#endif /* GEOGRASTER_COMMUNITIES_H */
