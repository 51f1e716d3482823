#pragma once
// geograypher_amd/csrc/cub_steps.hpp -- the library steps of the stage calls (rocPRIM through hipcub), each stated ONCE: a step is
// declared against the call's Plan (scratch_layout.hpp) with its types, its element count and its bit range, which makes the size
// query and folds the answer into the plan's temporaries; run() is the real call, with typed pointers and the same types, count
// and bits, once the plan's block is acquired.  Runs of one shape share a declaration; a run may take fewer elements than declared,
// never more.  A step whose query failed refuses to run, with the query's message.  The only file of the library that calls hipcub.
#include <hipcub/hipcub.hpp>

#include "gr_internal.hpp"

namespace grimpl {

struct CubStep {
  gr_ctx *c;
  const Plan *plan;
  int n, rc = GR_OK;
  CubStep(gr_ctx *c_, const Plan &p, int64_t n_) : c(c_), plan(&p), n((int)(n_ > 0 ? n_ : 0)) {}
  int query(hipError_t e, const char *call) { return e == hipSuccess ? GR_OK : fail(c, GR_EHIP, "%s: %s", call, hipGetErrorString(e)); }
  // the element count of a run (count < 0: the declared one), or -1 with the context's message
  int run_count(const char *step, int64_t count) const {
    if (rc == GR_OK && count > n) (void)fail(c, GR_EINVAL, "%s: a run of %lld elements, %d declared", step, (long long)count, n);
    return rc != GR_OK || count > n ? -1 : count < 0 ? n : (int)count;
  }
};

// Declares a step: QUERY is the hipcub call with null temporaries, their size argument named cub_q.  No element: no query.
#define GR_CUB_DECLARE(QUERY) do { size_t cub_q = 0; if (n > 0) rc = query(QUERY, #QUERY); p.need(cub_q); } while (0)
// Runs a step: CALL is the hipcub call over m elements, with the plan's temporaries (hipcub may take more than it asked for).
#define GR_CUB_RUN(STEP, CALL)                                      \
  do {                                                              \
    const int m = run_count(STEP, count);                           \
    if (m < 0) return rc != GR_OK ? rc : GR_EINVAL;                 \
    void *tmp = plan->tmp();                                        \
    size_t tmp_bytes = plan->tmp_bytes;                             \
    GR_HIP(c, CALL);                                                \
    return GR_OK;                                                   \
  } while (0)

template <class K, class V> struct SortPairs : CubStep {   // stable, by the bits [0, bits) of the key
  int bits;
  SortPairs(gr_ctx *ctx, Plan &p, int64_t n_, int bits_) : CubStep(ctx, p, n_), bits(bits_) {
    GR_CUB_DECLARE(hipcub::DeviceRadixSort::SortPairs(nullptr, cub_q, (const K *)nullptr, (K *)nullptr, (const V *)nullptr, (V *)nullptr, n, 0, bits));
  }
  int run(const K *keys, K *keys_out, const V *values, V *values_out, hipStream_t s, int64_t count = -1) const {
    GR_CUB_RUN("SortPairs", hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, keys, keys_out, values, values_out, m, 0, bits, s));
  }
};

template <class K> struct SortKeys : CubStep {
  int bits;
  SortKeys(gr_ctx *ctx, Plan &p, int64_t n_, int bits_) : CubStep(ctx, p, n_), bits(bits_) {
    GR_CUB_DECLARE(hipcub::DeviceRadixSort::SortKeys(nullptr, cub_q, (const K *)nullptr, (K *)nullptr, n, 0, bits));
  }
  int run(const K *keys, K *keys_out, hipStream_t s, int64_t count = -1) const {
    GR_CUB_RUN("SortKeys", hipcub::DeviceRadixSort::SortKeys(tmp, tmp_bytes, keys, keys_out, m, 0, bits, s));
  }
};

template <class T> struct ExclusiveSum : CubStep {
  ExclusiveSum(gr_ctx *ctx, Plan &p, int64_t n_) : CubStep(ctx, p, n_) {
    GR_CUB_DECLARE(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_q, (const T *)nullptr, (T *)nullptr, n));
  }
  int run(const T *in, T *out, hipStream_t s, int64_t count = -1) const {
    GR_CUB_RUN("ExclusiveSum", hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, in, out, m, s));
  }
};

template <class T> struct InclusiveMax : CubStep {   // out [i] = the maximum of in [0 .. i]
  InclusiveMax(gr_ctx *ctx, Plan &p, int64_t n_) : CubStep(ctx, p, n_) {
    GR_CUB_DECLARE(hipcub::DeviceScan::InclusiveScan(nullptr, cub_q, (const T *)nullptr, (T *)nullptr, hipcub::Max(), n));
  }
  int run(const T *in, T *out, hipStream_t s, int64_t count = -1) const {
    GR_CUB_RUN("InclusiveMax", hipcub::DeviceScan::InclusiveScan(tmp, tmp_bytes, in, out, hipcub::Max(), m, s));
  }
};

template <class K, class Count> struct RunLengthEncode : CubStep {   // the runs of equal keys: each key once, its length, *n_runs
  RunLengthEncode(gr_ctx *ctx, Plan &p, int64_t n_) : CubStep(ctx, p, n_) {
    GR_CUB_DECLARE(hipcub::DeviceRunLengthEncode::Encode(nullptr, cub_q, (const K *)nullptr, (K *)nullptr, (Count *)nullptr, (int *)nullptr, n));
  }
  int run(const K *keys, K *unique, Count *lengths, int *n_runs, hipStream_t s, int64_t count = -1) const {
    GR_CUB_RUN("RunLengthEncode", hipcub::DeviceRunLengthEncode::Encode(tmp, tmp_bytes, keys, unique, lengths, n_runs, m, s));
  }
};

using Sum = hipcub::Sum;   // the Op of a ReduceByKey that adds

// the runs of equal keys: each key once, the values of its run folded with Op (associative; in run order), *n_runs
template <class K, class V, class Op> struct ReduceByKey : CubStep {
  ReduceByKey(gr_ctx *ctx, Plan &p, int64_t n_) : CubStep(ctx, p, n_) {
    GR_CUB_DECLARE(hipcub::DeviceReduce::ReduceByKey(nullptr, cub_q, (const K *)nullptr, (K *)nullptr, (const V *)nullptr, (V *)nullptr,
                                                     (int *)nullptr, Op(), n));
  }
  int run(const K *keys, K *unique, const V *values, V *folded, int *n_runs, hipStream_t s, int64_t count = -1) const {
    GR_CUB_RUN("ReduceByKey", hipcub::DeviceReduce::ReduceByKey(tmp, tmp_bytes, keys, unique, values, folded, n_runs, Op(), m, s));
  }
};

#undef GR_CUB_DECLARE
#undef GR_CUB_RUN

}  // namespace grimpl
