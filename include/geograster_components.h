/* geograster_components.h -- companion of geograster.h, which includes it inside its extern "C" block; do not include it on its own:
 * gr_ctx, the GR_* codes and the GR_SIEVE_STAT_* enumerators are geograster.h's.  It holds the face-sieve call
 * (csrc/components.hip; the rule-set I1-I10 is DESIGN.md section 8u): the connected components of equally labelled faces over the
 * edge adjacency of a mesh, and the sieve that merges components below a measure into their greatest labelled neighbour.  The
 * binding keeps the signature in a table of its own (`_COMPONENTS_SIGNATURES`) and mirrors the structure (`FaceSieveArgs`);
 * tests/test_face_sieve_host.py compares both with this file.  Added without a GR_VERSION bump.
 *
 * The call takes its arguments in ONE descriptor in HOST memory, read once before the call returns, and the stream is a field of
 * it.  It is therefore not among the functions of these headers whose last parameter is `void *stream`, and the table of
 * tests/test_stream_contract_gpu.py does not list it.  It is NOT exempt from the stream contract of geograster.h: all work is
 * enqueued on `stream` and the call never touches another stream.  It synchronises `stream` once per round, to read one word back
 * (the faces the round changed), and returns with the last kernels enqueued: with min_measure == 0 it does not wait at all.
 * tests/test_stream_contract_components_gpu.py holds it to that.  The call needs no uploaded mesh; its scratch is the context's
 * stage arena (73 F bytes and the sort's temporaries). */
#ifndef GEOGRASTER_COMPONENTS_H
#define GEOGRASTER_COMPONENTS_H

/* All arrays are DEVICE pointers, C-contiguous.  Limits: F and V < 2^31 - 1, and 3 F <= 2^31 - 1.
 * I1  faces: F x 3 int32.  With has_canon != 0 corner v stands for vertex_canon[v] (V int32; it welds split seams), else for
 *     itself.  A face with two equal corners after that is degenerate: it is in no component (comp = -1), links nothing and never
 *     changes class.  A corner or a vertex_canon entry outside [0, V) is never used as an index: the face takes no part either and
 *     is counted in GR_SIEVE_STAT_BAD_FACES (the Python layer raises ValueError).
 * I2  face_class: F int32; any value < 0 means unlabelled and is -1 from here on, in class_out too.
 * I3  Every face that takes part has three edges, the unordered pairs of its (canonical) corners.  Faces that share an edge are
 *     edge-neighbours, pairwise, however many share it; sharing one vertex only is not adjacency.  (A fan of k faces on one edge
 *     costs k^2 pair visits per pass.)
 * I4  A component is the closure of "edge-neighbours of equal class" (unlabelled is a class here); comp[f] is its smallest face.
 * I5  weights: F int64, each >= 0, or null for 1 per face; m(A) is the sum over the faces of A.  The CALLER guarantees that the sum
 *     over all faces is below 2^62 and no weight negative (the binding checks both on the host).
 * I6  B is greater than A iff (m(B), -id(B)) > (m(A), -id(A)) lexicographically: among equal measures the lower id is greater.
 * I7  A component is small iff m < min_measure strictly and it is labelled, or unlabelled with fill_unlabelled != 0.  Without
 *     fill_unlabelled the unlabelled components are barriers: never small, never changed.
 * I8  For a small A, T(A) is the greatest labelled component edge-adjacent to A.  A labelled A points to T(A) iff T(A) is greater
 *     than A; an unlabelled A points to T(A) whenever it exists; every other component is a root; unlabelled components are never
 *     targets.  The pointers are acyclic.
 * I9  A round: every face of a pointing component takes the class the root of its pointer chain had at the start of the round
 *     (chains of any length resolve in one round); the components are recomputed.  Rounds repeat until one changes no face or
 *     max_rounds rounds have changed one (GR_SIEVE_STAT_ROUND_CAP = 1, not an error).  min_measure == 0: no round, the call is the
 *     component labelling alone.
 * I10 class_out: F int32 (class_out == face_class, in place, is allowed); comp: F int32, the components of the FINAL labelling;
 *     stats: GR_SIEVE_STAT_WORDS uint64.  Every word of the three is written.  The results do not depend on launch or arrival order.
 * GR_EINVAL (the message names gr_face_sieve), before any device work: a null descriptor, null arrays; F or V negative or out of
 * range; min_measure < 0; max_rounds < 1; class_out, comp or stats overlapping an input or each other, class_out == face_class
 * excepted. */
typedef struct gr_face_sieve_args {
  const int32_t *faces;
  const int32_t *face_class;
  const int64_t *weights;
  const int32_t *vertex_canon;
  int32_t *class_out;
  int32_t *comp;
  uint64_t *stats;
  void *stream;
  int64_t F;
  int64_t V;
  int64_t min_measure;
  int32_t has_canon;
  int32_t fill_unlabelled;
  int32_t max_rounds;
  int32_t reserved;
} gr_face_sieve_args;

int gr_face_sieve(gr_ctx *ctx, const gr_face_sieve_args *args_h);

#endif /* GEOGRASTER_COMPONENTS_H */
