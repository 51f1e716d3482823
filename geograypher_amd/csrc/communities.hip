// geograypher_amd/csrc/communities.hip -- the communities of the ray graph of the multiview-detection workflow: a synchronous,
// deterministic Louvain on integer weights (rules L1-L13).  Every sum of weights is an int64 sum (atomics or
// sorted runs: both exact), every score is formed from exact integers by the same four rounded operations in every path, and ties go
// to the lowest community id: the result does not depend on scheduling, nor on which of the three move paths handled a row.
// Needs no uploaded mesh.
#include "compact_dev.hpp"
#include "cub_steps.hpp"
#include "gr_internal.hpp"
#include "dev_common.hpp"
#include "ray_dev.hpp"

using namespace grimpl;

#define GR_COMM_BLOCK 256
#define GR_COMM_WAVE_ROW 64   // rows up to this many entries: one wave per row
#define GR_COMM_POINTS_LDS 256   // members up to which k_community_points keeps a community's ray records in LDS

namespace {

typedef unsigned long long u64;

enum {  // the control words of a call (u64 each)
  CT_BAD = 0,       // edges that break L2
  CT_M2 = 1,        // the sum of all directed entries
  CT_MOVES = 2,     // moves of the sweep
  CT_ROWS_WAVE = 3, // rows of the level per path
  CT_ROWS_GROUP = 4,
  CT_ROWS_KEY = 5,
  CT_KEY_ENTRIES = 6,  // entries the key path sorts per sweep: len + 1 over its rows
  CT_NV2 = 7,       // vertices of the next level
  CT_NCOMM = 8,     // communities of the result
  CT_WORDS = 16
};
enum { PATH_WAVE = 0, PATH_GROUP = 1, PATH_KEY = 2 };

struct Cand { double s; int32_t c; int32_t pad; };   // a candidate of the key path: score, community
struct CandMax {   // the larger score, ties to the lower community id (associative and commutative)
  __host__ __device__ Cand operator()(const Cand &a, const Cand &b) const { return (a.s > b.s || (a.s == b.s && a.c < b.c)) ? a : b; }
};

__host__ __device__ inline int row_path(int64_t len, int flags) {
  if (len == 0) return PATH_WAVE;   // nothing to combine: the vertex stays
  if ((flags & GR_COMM_FORCE_KEY) || len > GR_COMM_LDS_ROW) return PATH_KEY;
  if (flags & GR_COMM_FORCE_GROUP) return PATH_GROUP;
  return len <= GR_COMM_WAVE_ROW ? PATH_WAVE : PATH_GROUP;
}

// L5: four operations, each rounded once (the library is built without contraction); e, k_v, T, M2 < 2^53 convert exactly
__device__ __forceinline__ double comm_score(int64_t e, int64_t kv, int64_t T, int64_t M2, double gamma) {
  return (double)e - ((gamma * (double)kv) * (double)T) / (double)M2;
}
__device__ __forceinline__ bool cand_better(double s, int32_t c, double sb, int32_t cb) { return s > sb || (s == sb && c < cb); }

// L6-L8: the community of v after sweep t, given the best candidate over ALL candidates (the own community a included)
__device__ __forceinline__ int32_t comm_choice(int32_t a, int32_t cb, double sb, double sown, int t, const int32_t *__restrict__ size) {
  bool move = cb != a && sb > sown;
  move = move && ((t & 1) ? cb > a : cb < a);                  // L7
  if (move && size[a] == 1 && size[cb] == 1) move = cb < a;    // L8
  return move ? cb : a;
}

__device__ __forceinline__ int64_t wave_sum_i64(int64_t x) {
  for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
  return x;
}

__device__ __forceinline__ void count_wave(bool flag, u64 *word, int lane) {
  const u64 mask = __ballot(flag);
  if (mask && lane == __ffsll((long long)mask) - 1) atomicAdd(word, (u64)__popcll(mask));
}

// L2: both directions of every edge as a key row << 32 | column and its weight; a bad edge is counted and parked under row n
__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_edges(const int32_t *__restrict__ ei, const int32_t *__restrict__ ej,
                                                              const int64_t *__restrict__ eq, int64_t E, int64_t n,
                                                              u64 *__restrict__ keys, int64_t *__restrict__ vals, u64 *__restrict__ ctl) {
  const int64_t e = (int64_t)blockIdx.x * GR_COMM_BLOCK + threadIdx.x;
  bool bad = false;
  if (e < E) {
    const int64_t i = ei[e], j = ej[e], q = eq[e];
    bad = i == j || i < 0 || i >= n || j < 0 || j >= n || q < 1 || q > 0x7FFFFFFFll;
    keys[2 * e] = bad ? (u64)n << 32 : ((u64)i << 32) | (u64)j;
    keys[2 * e + 1] = bad ? (u64)n << 32 : ((u64)j << 32) | (u64)i;
    vals[2 * e] = vals[2 * e + 1] = bad ? 0 : q;
  }
  count_wave(bad, ctl + CT_BAD, threadIdx.x & 63);
}

// L3: the unique entries of a level -> columns, row lengths (deg, zeroed, nv + 1 of them), row sums k (zeroed)
__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_rows(const u64 *__restrict__ ukeys, const int64_t *__restrict__ uvals, int64_t nnz,
                                                             int64_t nv, int32_t *__restrict__ col, u64 *__restrict__ deg, u64 *__restrict__ k,
                                                             u64 *__restrict__ m2) {
  const int64_t e = (int64_t)blockIdx.x * GR_COMM_BLOCK + threadIdx.x;
  int64_t w = 0;
  if (e < nnz) {
    const u64 key = ukeys[e];
    const int64_t r = (int64_t)(key >> 32);
    col[e] = (int32_t)(key & 0xFFFFFFFFull);
    if (r < nv) {
      w = uvals[e];
      atomicAdd(&deg[r], 1ull);
      atomicAdd(&k[r], (u64)w);
    }
  }
  if (m2) {   // the first level only: M2 is the same at every level
    w = wave_sum_i64(w);
    if ((threadIdx.x & 63) == 0 && w) atomicAdd(m2, (u64)w);
  }
}

// L4, and the path of every row of the level: the rows of the workgroup path on a list, len + 1 for the rows of the key path
__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_level_init(int64_t nv, const int64_t *__restrict__ rowptr, const u64 *__restrict__ k,
                                                                   int flags, int32_t *__restrict__ comm, u64 *__restrict__ tot,
                                                                   int32_t *__restrict__ size, int32_t *__restrict__ list_mid,
                                                                   int64_t *__restrict__ lenp1, u64 *__restrict__ ctl) {
  const int64_t v = (int64_t)blockIdx.x * GR_COMM_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int path = -1;
  int64_t len = 0;
  if (v < nv) {
    comm[v] = (int32_t)v;
    tot[v] = k[v];
    size[v] = 1;
    len = rowptr[v + 1] - rowptr[v];
    path = row_path(len, flags);
    lenp1[v] = path == PATH_KEY ? len + 1 : 0;
  }
  if (v == nv) lenp1[v] = 0;
  count_wave(path == PATH_WAVE, ctl + CT_ROWS_WAVE, lane);
  count_wave(path == PATH_KEY, ctl + CT_ROWS_KEY, lane);
  const u64 mid = __ballot(path == PATH_GROUP);
  if (mid) {
    const u64 base = wave_append(mid, ctl + CT_ROWS_GROUP, lane);
    if (path == PATH_GROUP) list_mid[base + (u64)wave_rank(mid, lane)] = (int32_t)v;
  }
  const int64_t ent = wave_sum_i64(path == PATH_KEY ? len + 1 : 0);
  if (lane == 0 && ent) atomicAdd(ctl + CT_KEY_ENTRIES, (u64)ent);
}

struct MoveArgs {
  const int64_t *rowptr;   // [nv + 1]
  const int32_t *col;      // [nnz]
  const int64_t *val;      // [nnz]
  const u64 *k;            // [nv]
  const int32_t *comm;     // [nv] the snapshot of the sweep
  const u64 *tot;          // [nv]
  const int32_t *size;     // [nv]
  u64 *ctl;
  int32_t *comm_new;       // [nv]
  double gamma;
  int64_t nv;
  int t, flags;
};

// The wave path: one wave per row of at most 64 entries, a neighbour per lane.  The distinct communities are peeled off one per
// round: the first lane still waiting names its community, the lanes of that community add their weights up (an integer wave sum)
// and retire.
__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_move_wave(MoveArgs m) {
  const int lane = threadIdx.x & 63;
  const int64_t v = (int64_t)blockIdx.x * (GR_COMM_BLOCK / 64) + (threadIdx.x >> 6);
  if (v >= m.nv) return;   // the whole wave
  const int64_t beg = m.rowptr[v], len = m.rowptr[v + 1] - beg;
  if (row_path(len, m.flags) != PATH_WAVE) return;
  const int32_t a = m.comm[v];
  const int64_t kv = (int64_t)m.k[v], M2 = (int64_t)m.ctl[CT_M2];
  int32_t cu = -1;
  int64_t w = 0, tc = 0;
  bool wait = false;
  if (lane < len) {
    const int32_t u = m.col[beg + lane];
    wait = u != v;
    cu = m.comm[u];
    w = m.val[beg + lane];
    tc = (int64_t)m.tot[cu];
  }
  int64_t e_own = 0;
  double sb = 0.0;
  int32_t cb = -1;
  u64 mask;
  while ((mask = __ballot(wait)) != 0) {
    const int leader = __ffsll((long long)mask) - 1;
    const int32_t c = __shfl(cu, leader);
    const int64_t T = __shfl(tc, leader);
    const bool mine = wait && cu == c;
    const int64_t e = wave_sum_i64(mine ? w : 0);
    wait = wait && !mine;
    if (c == a) { e_own = e; continue; }
    const double s = comm_score(e, kv, T, M2, m.gamma);
    if (cb < 0 || cand_better(s, c, sb, cb)) { sb = s; cb = c; }
  }
  if (lane != 0) return;
  const double sown = comm_score(e_own, kv, (int64_t)m.tot[a] - kv, M2, m.gamma);
  if (cb < 0 || !cand_better(sb, cb, sown, a)) { sb = sown; cb = a; }
  const int32_t to = comm_choice(a, cb, sb, sown, m.t, m.size);
  m.comm_new[v] = to;
  if (to != a) atomicAdd(m.ctl + CT_MOVES, 1ull);
}

// The workgroup path: one workgroup per row of at most GR_COMM_LDS_ROW entries.  The (community, weight) pairs are sorted by
// community in LDS (bitonic, padded to a power of two with a key behind every community), a segmented inclusive sum leaves the
// weight of every community at the last entry of its run, and the candidates are reduced over the workgroup.
__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_move_group(MoveArgs m, const int32_t *__restrict__ list_mid) {
  __shared__ uint32_t skey[GR_COMM_LDS_ROW];
  __shared__ int64_t sval[2][GR_COMM_LDS_ROW];
  __shared__ int64_t s_eown;
  __shared__ double s_best[GR_COMM_BLOCK / 64];
  __shared__ int32_t c_best[GR_COMM_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t v = list_mid[blockIdx.x];
  const int64_t beg = m.rowptr[v];
  const int len = (int)(m.rowptr[v + 1] - beg);   // 1 .. GR_COMM_LDS_ROW (row_path)
  int P = 64;
  while (P < len) P <<= 1;
  const int32_t a = m.comm[v];
  const int64_t kv = (int64_t)m.k[v], M2 = (int64_t)m.ctl[CT_M2];
  for (int idx = tid; idx < P; idx += GR_COMM_BLOCK) {
    uint32_t key = 0xFFFFFFFFu;
    int64_t w = 0;
    if (idx < len) {
      const int32_t u = m.col[beg + idx];
      if (u != v) { key = (uint32_t)m.comm[u]; w = m.val[beg + idx]; }
    }
    skey[idx] = key;
    sval[0][idx] = w;
  }
  if (tid == 0) s_eown = 0;
  for (int kk = 2; kk <= P; kk <<= 1)
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      __syncthreads();
      for (int idx = tid; idx < P; idx += GR_COMM_BLOCK) {
        const int other = idx ^ jj;
        if (other > idx) {
          const uint32_t ka = skey[idx], kb = skey[other];
          if ((ka > kb) == ((idx & kk) == 0)) {
            skey[idx] = kb; skey[other] = ka;
            const int64_t wa = sval[0][idx];
            sval[0][idx] = sval[0][other]; sval[0][other] = wa;
          }
        }
      }
    }
  __syncthreads();
  int src = 0;
  for (int d = 1; d < P; d <<= 1) {   // equal keys are contiguous: idx - d is in the run of idx iff their keys are equal
    for (int idx = tid; idx < P; idx += GR_COMM_BLOCK) {
      int64_t x = sval[src][idx];
      if (idx >= d && skey[idx - d] == skey[idx]) x += sval[src][idx - d];
      sval[src ^ 1][idx] = x;
    }
    __syncthreads();
    src ^= 1;
  }
  double sb = 0.0;
  int32_t cb = -1;
  for (int idx = tid; idx < P; idx += GR_COMM_BLOCK) {
    const uint32_t key = skey[idx];
    if (key == 0xFFFFFFFFu || (idx + 1 < P && skey[idx + 1] == key)) continue;   // the last entry of a run only
    const int32_t c = (int32_t)key;
    const int64_t e = sval[src][idx];
    if (c == a) { s_eown = e; continue; }
    const double s = comm_score(e, kv, (int64_t)m.tot[c], M2, m.gamma);
    if (cb < 0 || cand_better(s, c, sb, cb)) { sb = s; cb = c; }
  }
  for (int d = 32; d > 0; d >>= 1) {
    const double so = __shfl_xor(sb, d);
    const int32_t co = __shfl_xor(cb, d);
    if (co >= 0 && (cb < 0 || cand_better(so, co, sb, cb))) { sb = so; cb = co; }
  }
  if (lane == 0) { s_best[tid >> 6] = sb; c_best[tid >> 6] = cb; }
  __syncthreads();
  if (tid != 0) return;
  for (int wv = 1; wv < GR_COMM_BLOCK / 64; ++wv) {
    const double so = s_best[wv];
    const int32_t co = c_best[wv];
    if (co >= 0 && (cb < 0 || cand_better(so, co, sb, cb))) { sb = so; cb = co; }
  }
  const double sown = comm_score(s_eown, kv, (int64_t)m.tot[a] - kv, M2, m.gamma);
  if (cb < 0 || !cand_better(sb, cb, sown, a)) { sb = sown; cb = a; }
  const int32_t to = comm_choice(a, cb, sb, sown, m.t, m.size);
  m.comm_new[v] = to;
  if (to != a) atomicAdd(m.ctl + CT_MOVES, 1ull);
}

// The key path, step 1: the entries of its rows as keys v << 32 | comm[u] behind the row's offset, one more per row for the own
// community (weight 0: it is always scored); the diagonal entry is parked under row nv.
__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_key_emit(MoveArgs m, const u64 *__restrict__ ukeys, int64_t nnz,
                                                                 const int64_t *__restrict__ lenp1, const int64_t *__restrict__ loff,
                                                                 u64 *__restrict__ keys, int64_t *__restrict__ vals) {
  const int64_t e = (int64_t)blockIdx.x * GR_COMM_BLOCK + threadIdx.x;
  if (e >= nnz) return;
  const int64_t v = (int64_t)(ukeys[e] >> 32);
  if (v >= m.nv || lenp1[v] == 0) return;
  const int64_t beg = m.rowptr[v], pos = loff[v] + (e - beg);
  const int32_t u = m.col[e];
  keys[pos] = u != v ? ((u64)v << 32) | (u64)(uint32_t)m.comm[u] : (u64)m.nv << 32;
  vals[pos] = u != v ? m.val[e] : 0;
  if (e == beg) {
    keys[loff[v] + lenp1[v] - 1] = ((u64)v << 32) | (u64)(uint32_t)m.comm[v];
    vals[loff[v] + lenp1[v] - 1] = 0;
  }
}

// ... step 2, behind the sort and the sums per key: the score of every (vertex, community); entries behind the runs, and the run
// under row nv, become candidates that no vertex owns
__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_key_scores(MoveArgs m, const u64 *__restrict__ rkeys, const int64_t *__restrict__ rvals,
                                                                   const int *__restrict__ n_runs, int64_t count, int32_t *__restrict__ vk,
                                                                   Cand *__restrict__ cand, double *__restrict__ sown) {
  const int64_t i = (int64_t)blockIdx.x * GR_COMM_BLOCK + threadIdx.x;
  if (i >= count) return;
  Cand out = {-INFINITY, 0x7FFFFFFF, 0};
  int32_t vo = (int32_t)m.nv;
  if (i < *n_runs) {
    const u64 key = rkeys[i];
    const int64_t v = (int64_t)(key >> 32);
    if (v < m.nv) {
      const int32_t c = (int32_t)(key & 0xFFFFFFFFull), a = m.comm[v];
      const int64_t kv = (int64_t)m.k[v];
      out.s = comm_score(rvals[i], kv, (int64_t)m.tot[c] - (c == a ? kv : 0), (int64_t)m.ctl[CT_M2], m.gamma);
      out.c = c;
      vo = (int32_t)v;
      if (c == a) sown[v] = out.s;
    }
  }
  vk[i] = vo;
  cand[i] = out;
}

// ... step 3, behind the best candidate per vertex: the choice
__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_key_apply(MoveArgs m, const int32_t *__restrict__ vk2, const Cand *__restrict__ best,
                                                                  const int *__restrict__ n_runs, int64_t count, const double *__restrict__ sown) {
  const int64_t i = (int64_t)blockIdx.x * GR_COMM_BLOCK + threadIdx.x;
  bool moved = false;
  if (i < count && i < *n_runs && vk2[i] < m.nv) {
    const int32_t v = vk2[i], a = m.comm[v];
    const int32_t to = comm_choice(a, best[i].c, best[i].s, sown[v], m.t, m.size);
    m.comm_new[v] = to;
    moved = to != a;
  }
  count_wave(moved, m.ctl + CT_MOVES, threadIdx.x & 63);
}

// L9: all moves at once -- tot and size of the new communities (both zeroed), int64 atomics
__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_tot_size(int64_t nv, const int32_t *__restrict__ comm, const u64 *__restrict__ k,
                                                                 u64 *__restrict__ tot, int32_t *__restrict__ size) {
  const int64_t v = (int64_t)blockIdx.x * GR_COMM_BLOCK + threadIdx.x;
  if (v >= nv) return;
  const int32_t c = comm[v];
  atomicAdd(&tot[c], k[v]);
  atomicAdd(&size[c], 1);
}

__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_alive(int64_t nv, const int32_t *__restrict__ size, int32_t *__restrict__ flag) {
  const int64_t c = (int64_t)blockIdx.x * GR_COMM_BLOCK + threadIdx.x;
  if (c < nv) flag[c] = size[c] > 0;
}

// L11: the labels composed with the dense ranks, and the directed entries under their new (row, column)
__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_relabel(int64_t n, int64_t nv, int64_t nnz, const int32_t *__restrict__ comm,
                                                                const int32_t *__restrict__ flag, const int32_t *__restrict__ pos,
                                                                int32_t *__restrict__ label, const u64 *__restrict__ ukeys,
                                                                const int64_t *__restrict__ uvals, u64 *__restrict__ keys,
                                                                int64_t *__restrict__ vals, u64 *__restrict__ ctl) {
  const int64_t i = (int64_t)blockIdx.x * GR_COMM_BLOCK + threadIdx.x;
  if (i < n) label[i] = pos[comm[label[i]]];
  if (i < nnz) {
    const u64 key = ukeys[i];
    keys[i] = ((u64)(uint32_t)pos[comm[key >> 32]] << 32) | (u64)(uint32_t)pos[comm[key & 0xFFFFFFFFull]];
    vals[i] = uvals[i];
  }
  if (i == 0) ctl[CT_NV2] = (u64)(pos[nv - 1] + flag[nv - 1]);
}

__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_identity(int64_t n, int32_t *__restrict__ label) {
  const int64_t i = (int64_t)blockIdx.x * GR_COMM_BLOCK + threadIdx.x;
  if (i < n) label[i] = (int32_t)i;
}

// L12: members and lowest member of every final community (fsize zeroed, fmin filled with 0x7F bytes); a vertex without an edge
// is alone in a community of degree 0 and takes no part
__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_members(int64_t n, const int32_t *__restrict__ label, const u64 *__restrict__ k,
                                                                int32_t *__restrict__ fsize, int32_t *__restrict__ fmin) {
  const int64_t o = (int64_t)blockIdx.x * GR_COMM_BLOCK + threadIdx.x;
  if (o >= n) return;
  const int32_t L = label[o];
  if (k[L] == 0) return;
  atomicAdd(&fsize[L], 1);
  atomicMin(&fmin[L], (int32_t)o);
}

__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_order_keys(int64_t n, int64_t nvf, const int32_t *__restrict__ fsize,
                                                                   const int32_t *__restrict__ fmin, u64 *__restrict__ okey,
                                                                   int32_t *__restrict__ oval, u64 *__restrict__ ctl) {
  const int64_t L = (int64_t)blockIdx.x * GR_COMM_BLOCK + threadIdx.x;
  bool alive = false;
  if (L < nvf) {
    alive = fsize[L] > 0;
    okey[L] = alive ? ((u64)(n - fsize[L]) << 32) | (u64)(uint32_t)fmin[L] : (u64)(n + 1) << 32;   // falling size, then lowest member
    oval[L] = (int32_t)L;
  }
  count_wave(alive, ctl + CT_NCOMM, threadIdx.x & 63);
}

// L13: size, in (the diagonal of the final matrix: a binary search in the sorted row) and tot of every community, by its new number
__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_write_communities(int64_t nvf, const int32_t *__restrict__ oval2,
                                                                          const int32_t *__restrict__ fsize, const u64 *__restrict__ k,
                                                                          const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                          const int64_t *__restrict__ val, int32_t *__restrict__ newid,
                                                                          int32_t *__restrict__ out_size, int64_t *__restrict__ out_in,
                                                                          int64_t *__restrict__ out_tot) {
  const int64_t idx = (int64_t)blockIdx.x * GR_COMM_BLOCK + threadIdx.x;
  if (idx >= nvf) return;
  const int32_t L = oval2[idx];
  if (fsize[L] == 0) { newid[L] = -1; return; }
  newid[L] = (int32_t)idx;   // the communities with members come first
  int64_t lo = rowptr[L], hi = rowptr[L + 1];
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (col[mid] < L) lo = mid + 1; else hi = mid;
  }
  out_size[idx] = fsize[L];
  out_in[idx] = lo < rowptr[L + 1] && col[lo] == L ? val[lo] : 0;
  out_tot[idx] = (int64_t)k[L];
}

__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_write_labels(int64_t n, const int32_t *__restrict__ label, const u64 *__restrict__ k,
                                                                     const int32_t *__restrict__ newid, int32_t *__restrict__ community) {
  const int64_t o = (int64_t)blockIdx.x * GR_COMM_BLOCK + threadIdx.x;
  if (o >= n) return;
  community[o] = k ? (k[label[o]] ? newid[label[o]] : -1) : -1;   // (no k: a graph without an edge)
}

// -- L14: one point per community ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_ray_prep(const double *__restrict__ starts, const double *__restrict__ ends, int64_t n,
                                                                 const int32_t *__restrict__ community, int64_t M, RayRec *__restrict__ rec,
                                                                 uint32_t *__restrict__ keys, int32_t *__restrict__ rays) {
  const int64_t i = (int64_t)blockIdx.x * GR_COMM_BLOCK + threadIdx.x;
  if (i >= n) return;
  rec[i] = ray_record(starts, ends, i, 0);
  const int32_t cm = community[i];
  keys[i] = cm >= 0 && cm < M ? (uint32_t)cm : (uint32_t)M;   // a ray of no community sorts behind all of them
  rays[i] = (int32_t)i;
}

// the member lists: where the run of every community starts in the sorted (community, ray) pairs, and its length (zeroed)
__global__ void __launch_bounds__(GR_COMM_BLOCK) k_comm_member_runs(const uint32_t *__restrict__ skeys, int64_t n, int64_t M,
                                                                    int32_t *__restrict__ first, int32_t *__restrict__ count) {
  const int64_t p = (int64_t)blockIdx.x * GR_COMM_BLOCK + threadIdx.x;
  if (p >= n) return;
  const uint32_t cm = skeys[p];
  if (cm >= M) return;
  atomicAdd(&count[cm], 1);
  if (p == 0 || skeys[p - 1] != cm) first[cm] = (int32_t)p;
}

// One workgroup per community.  The m (m - 1) ordered pairs of distinct members are numbered row by row and dealt to the lanes
// with a stride of the workgroup; a lane adds pA then pB of its pairs in ascending order, the lanes of a wave are folded by a
// fixed butterfly, the waves in ascending order: the sum is the same in every run.
__global__ void __launch_bounds__(GR_COMM_BLOCK) k_community_points(const RayRec *__restrict__ rec, const double *__restrict__ ends,
                                                                    const int32_t *__restrict__ srays, const int32_t *__restrict__ first,
                                                                    const int32_t *__restrict__ count, double *__restrict__ points) {
  __shared__ RayRec members[GR_COMM_POINTS_LDS];
  __shared__ double part[GR_COMM_BLOCK / 64][3];
  const int tid = threadIdx.x;
  const int64_t cm = blockIdx.x;
  const int64_t m = count[cm];
  if (m < 2) {   // the mean of no pair
    if (tid < 3) points[3 * cm + tid] = NAN;
    return;
  }
  const int32_t *mine = srays + first[cm];
  const bool staged = m <= GR_COMM_POINTS_LDS;
  if (staged) {
    if (tid < m) members[tid] = rec[mine[tid]];
    __syncthreads();
  }
  double sx = 0.0, sy = 0.0, sz = 0.0;
  const int64_t pairs = m * (m - 1);
  for (int64_t t = tid; t < pairs; t += GR_COMM_BLOCK) {
    const int64_t ia = t / (m - 1), r = t - ia * (m - 1), ib = r + (r >= ia);
    const int64_t ra = mine[ia], rb = mine[ib];
    const RayRec a = staged ? members[ia] : rec[ra], b = staged ? members[ib] : rec[rb];
    double pax, pay, paz, pbx, pby, pbz;
    segment_closest_points(a, b, ends, ra, rb, pax, pay, paz, pbx, pby, pbz);
    sx += pax; sy += pay; sz += paz;
    sx += pbx; sy += pby; sz += pbz;
  }
  for (int d = 32; d > 0; d >>= 1) {
    sx += __shfl_xor(sx, d); sy += __shfl_xor(sy, d); sz += __shfl_xor(sz, d);
  }
  if ((tid & 63) == 0) { part[tid >> 6][0] = sx; part[tid >> 6][1] = sy; part[tid >> 6][2] = sz; }
  __syncthreads();
  if (tid < 3) {
    double total = part[0][tid];
    for (int w = 1; w < GR_COMM_BLOCK / 64; ++w) total += part[w][tid];
    points[3 * cm + tid] = total / (double)(2 * pairs);
  }
}

inline unsigned grid_of(int64_t n) { return (unsigned)ceil_div(n > 0 ? n : 1, GR_COMM_BLOCK); }

}  // namespace

extern "C" {

int gr_louvain_communities(gr_ctx *c, const int32_t *edge_i, const int32_t *edge_j, const int64_t *edge_q, int64_t E, int64_t n,
                           double resolution, int32_t max_sweeps, int flags, int32_t *community, int32_t *comm_size, int64_t *comm_in,
                           int64_t *comm_tot, int64_t *stats, void *stream) {
  if (!c) return GR_EINVAL;
  if (n < 0 || n > GR_COMM_MAX_VERTICES || E < 0 || E >= GR_COMM_MAX_EDGES || max_sweeps < 1 || !(resolution == resolution))
    return fail(c, GR_EINVAL, "gr_louvain_communities: bad arguments n=%lld E=%lld max_sweeps=%d (n <= %d, E < %d, max_sweeps >= 1)",
                (long long)n, (long long)E, (int)max_sweeps, (int)GR_COMM_MAX_VERTICES, (int)GR_COMM_MAX_EDGES);
  if (!stats || (E > 0 && (!edge_i || !edge_j || !edge_q)) || (n > 0 && (!community || !comm_size || !comm_in || !comm_tot)))
    return fail(c, GR_EINVAL, "gr_louvain_communities: null arrays");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  int64_t st[GR_COMM_STAT_WORDS] = {0};
  auto finish = [&](int code) -> int {   // the statistics block, then the stream is waited for: the scratch is free on return
    if (hipMemcpyAsync(stats, st, sizeof(st), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return fail(c, GR_EHIP, "gr_louvain_communities: writing the statistics failed");
    return code;
  };
  if (n == 0 && E == 0) return finish(GR_OK);

  const int64_t N2 = 2 * E, cap = N2 + n;   // directed entries; ... and one more per row on the key path
  const int bits = 32 + bit_length(n);      // rows 0 .. n (n: parked entries) above the column
  Plan p;
  const auto o_ctl = p.array<u64>(CT_WORDS);
  const auto o_runs = p.array<int>(4);
  const auto o_akeys = p.array<u64>(cap), o_bkeys = p.array<u64>(cap);
  const auto o_avals = p.array<int64_t>(cap), o_bvals = p.array<int64_t>(cap);
  const auto o_ukeys = p.array<u64>(N2);
  const auto o_uvals = p.array<int64_t>(N2);
  const auto o_col = p.array<int32_t>(N2);
  const auto o_deg = p.array<int64_t>(n + 1), o_rowptr = p.array<int64_t>(n + 1), o_lenp1 = p.array<int64_t>(n + 1), o_loff = p.array<int64_t>(n + 1);
  const auto o_k = p.array<u64>(n), o_tot = p.array<u64>(n);
  const auto o_comm0 = p.array<int32_t>(n), o_comm1 = p.array<int32_t>(n), o_size = p.array<int32_t>(n), o_label = p.array<int32_t>(n);
  const auto o_list = p.array<int32_t>(n), o_fsize = p.array<int32_t>(n), o_fmin = p.array<int32_t>(n), o_newid = p.array<int32_t>(n);
  const auto o_oval = p.array<int32_t>(n), o_oval2 = p.array<int32_t>(n);
  const auto o_okey = p.array<u64>(n), o_okey2 = p.array<u64>(n);
  const auto o_sown = p.array<double>(n);
  const auto o_vk = p.array<int32_t>(cap), o_vk2 = p.array<int32_t>(cap);
  const auto o_cand = p.array<Cand>(cap), o_cand2 = p.array<Cand>(cap);
  const FlagScan alive(c, p, n);
  const SortPairs<u64, int64_t> sort(c, p, cap, bits);
  const ReduceByKey<u64, int64_t, Sum> sums(c, p, cap);
  const ReduceByKey<int32_t, Cand, CandMax> argmax(c, p, cap);
  const ExclusiveSum<int64_t> offsets(c, p, n + 1);
  const SortPairs<u64, int32_t> order(c, p, n, 32 + bit_length(n + 1));
  int rc = stage_acquire(c, c->stage, p.finish(), s, "communities");
  if (rc != GR_OK) return rc;
  p.base = c->stage.ptr;
  u64 *ctl = o_ctl(), *akeys = o_akeys(), *bkeys = o_bkeys(), *ukeys = o_ukeys(), *k = o_k(), *tot = o_tot();
  int64_t *avals = o_avals(), *bvals = o_bvals(), *uvals = o_uvals(), *rowptr = o_rowptr(), *lenp1 = o_lenp1(), *loff = o_loff();
  int *runs = o_runs();
  int32_t *col = o_col(), *comm = o_comm0(), *comm_new = o_comm1(), *size = o_size(), *label = o_label();
  u64 ctl_h[CT_WORDS];
  int runs_h[4];

  GR_HIP(c, hipMemsetAsync(ctl, 0, sizeof(u64) * CT_WORDS, s));
  // the entries of a level: sorted by (row, column), equal keys summed -> ukeys, uvals, runs[0]; then the rows
  auto read_control = [&]() -> int {
    GR_HIP(c, hipMemcpyAsync(ctl_h, ctl, sizeof(ctl_h), hipMemcpyDeviceToHost, s));
    GR_HIP(c, hipMemcpyAsync(runs_h, runs, sizeof(runs_h), hipMemcpyDeviceToHost, s));
    GR_HIP(c, hipStreamSynchronize(s));
    return GR_OK;
  };
  auto sum_entries = [&](int64_t count) -> int {
    GR_HIP(c, hipMemsetAsync(runs, 0, sizeof(int) * 4, s));
    if (count == 0) return GR_OK;
    GR_TRY(sort.run(akeys, bkeys, avals, bvals, s, count));
    GR_TRY(sums.run(bkeys, ukeys, bvals, uvals, runs, s, count));
    return GR_OK;
  };
  auto build_rows = [&](int64_t nnz, int64_t nv, bool first) -> int {
    GR_HIP(c, hipMemsetAsync(o_deg(), 0, sizeof(int64_t) * (size_t)(nv + 1), s));
    GR_HIP(c, hipMemsetAsync(k, 0, sizeof(u64) * (size_t)nv, s));
    if (nnz > 0)
      hipLaunchKernelGGL(k_comm_rows, dim3(grid_of(nnz)), dim3(GR_COMM_BLOCK), 0, s, (const u64 *)ukeys, (const int64_t *)uvals, nnz, nv, col,
                         (u64 *)o_deg(), k, first ? ctl + CT_M2 : (u64 *)nullptr);
    GR_HIP(c, hipGetLastError());
    GR_TRY(offsets.run(o_deg(), rowptr, s, nv + 1));
    return GR_OK;
  };

  if (E > 0) hipLaunchKernelGGL(k_comm_edges, dim3(grid_of(E)), dim3(GR_COMM_BLOCK), 0, s, edge_i, edge_j, edge_q, E, n, akeys, avals, ctl);
  GR_HIP(c, hipGetLastError());
  GR_TRY(sum_entries(N2));
  GR_TRY(read_control());
  st[GR_COMM_STAT_BAD_EDGES] = (int64_t)ctl_h[CT_BAD];
  if (ctl_h[CT_BAD]) {
    (void)fail(c, GR_EINDEX, "gr_louvain_communities: %llu edges with i == j, an index outside [0, %lld) or a weight outside [1, 2^31)",
               ctl_h[CT_BAD], (long long)n);
    return finish(GR_EINDEX);
  }
  int64_t nnz = runs_h[0], nv = n;
  if (nnz == 0) {   // no edge: every vertex -1
    hipLaunchKernelGGL(k_comm_write_labels, dim3(grid_of(n)), dim3(GR_COMM_BLOCK), 0, s, n, (const int32_t *)nullptr, (const u64 *)nullptr,
                       (const int32_t *)nullptr, community);
    GR_HIP(c, hipGetLastError());
    return finish(GR_OK);
  }
  GR_TRY(build_rows(nnz, nv, true));
  hipLaunchKernelGGL(k_comm_identity, dim3(grid_of(n)), dim3(GR_COMM_BLOCK), 0, s, n, label);

  int levels = 0, caps = 0;
  bool ended = false;
  for (int level = 0; level < GR_COMM_MAX_LEVELS && !ended; ++level) {
    GR_HIP(c, hipMemsetAsync(ctl + CT_MOVES, 0, sizeof(u64) * (CT_KEY_ENTRIES - CT_MOVES + 1), s));
    hipLaunchKernelGGL(k_comm_level_init, dim3(grid_of(nv + 1)), dim3(GR_COMM_BLOCK), 0, s, nv, (const int64_t *)rowptr, (const u64 *)k, flags, comm,
                       tot, size, o_list(), lenp1, ctl);
    GR_HIP(c, hipGetLastError());
    GR_TRY(offsets.run(lenp1, loff, s, nv + 1));
    GR_TRY(read_control());
    if (level == 0) {
      st[GR_COMM_STAT_M2] = (int64_t)ctl_h[CT_M2];
      if (ctl_h[CT_M2] >= (1ull << 53)) {
        (void)fail(c, GR_EINVAL, "gr_louvain_communities: twice the sum of the weights is %llu, the limit is 2^53", ctl_h[CT_M2]);
        return finish(GR_EINVAL);
      }
    }
    const int64_t rows_wave = (int64_t)ctl_h[CT_ROWS_WAVE], rows_group = (int64_t)ctl_h[CT_ROWS_GROUP], rows_key = (int64_t)ctl_h[CT_ROWS_KEY];
    const int64_t key_entries = (int64_t)ctl_h[CT_KEY_ENTRIES];   // <= nnz + nv <= cap
    int64_t level_moves = 0, moved = 0;
    int t = 0;
    while (t < max_sweeps) {
      MoveArgs m = {rowptr, col, uvals, k, comm, tot, size, ctl, comm_new, resolution, nv, t, flags};
      GR_HIP(c, hipMemsetAsync(ctl + CT_MOVES, 0, sizeof(u64), s));
      GR_HIP(c, hipMemcpyAsync(comm_new, comm, sizeof(int32_t) * (size_t)nv, hipMemcpyDeviceToDevice, s));   // a vertex stays unless a path moves it
      if (rows_wave) hipLaunchKernelGGL(k_comm_move_wave, dim3((unsigned)ceil_div(nv, GR_COMM_BLOCK / 64)), dim3(GR_COMM_BLOCK), 0, s, m);
      if (rows_group) hipLaunchKernelGGL(k_comm_move_group, dim3((unsigned)rows_group), dim3(GR_COMM_BLOCK), 0, s, m, (const int32_t *)o_list());
      if (rows_key) {
        hipLaunchKernelGGL(k_comm_key_emit, dim3(grid_of(nnz)), dim3(GR_COMM_BLOCK), 0, s, m, (const u64 *)ukeys, nnz, (const int64_t *)lenp1,
                           (const int64_t *)loff, akeys, avals);
        GR_HIP(c, hipGetLastError());
        GR_TRY(sort.run(akeys, bkeys, avals, bvals, s, key_entries));
        GR_TRY(sums.run(bkeys, akeys, bvals, avals, runs + 1, s, key_entries));
        hipLaunchKernelGGL(k_comm_key_scores, dim3(grid_of(key_entries)), dim3(GR_COMM_BLOCK), 0, s, m, (const u64 *)akeys, (const int64_t *)avals,
                           (const int *)(runs + 1), key_entries, o_vk(), o_cand(), o_sown());
        GR_HIP(c, hipGetLastError());
        GR_TRY(argmax.run(o_vk(), o_vk2(), o_cand(), o_cand2(), runs + 2, s, key_entries));
        hipLaunchKernelGGL(k_comm_key_apply, dim3(grid_of(key_entries)), dim3(GR_COMM_BLOCK), 0, s, m, (const int32_t *)o_vk2(),
                           (const Cand *)o_cand2(), (const int *)(runs + 2), key_entries, (const double *)o_sown());
      }
      GR_HIP(c, hipMemsetAsync(tot, 0, sizeof(u64) * (size_t)nv, s));
      GR_HIP(c, hipMemsetAsync(size, 0, sizeof(int32_t) * (size_t)nv, s));
      hipLaunchKernelGGL(k_comm_tot_size, dim3(grid_of(nv)), dim3(GR_COMM_BLOCK), 0, s, nv, (const int32_t *)comm_new, (const u64 *)k, tot, size);
      GR_HIP(c, hipGetLastError());
      std::swap(comm, comm_new);
      GR_TRY(read_control());   // the one read of a sweep: its moves
      moved = (int64_t)ctl_h[CT_MOVES];
      level_moves += moved;
      st[GR_COMM_STAT_ROWS_WAVE] += rows_wave;
      st[GR_COMM_STAT_ROWS_GROUP] += rows_group;
      st[GR_COMM_STAT_ROWS_KEY] += rows_key;
      ++t;
      if (moved == 0) break;
    }
    st[GR_COMM_STAT_SWEEPS + level] = t;
    st[GR_COMM_STAT_MOVES + level] = level_moves;
    st[GR_COMM_STAT_LEVELS_RUN] = level + 1;
    if (level_moves == 0) { ended = true; break; }   // L10: the level is discarded
    if (moved != 0) caps |= GR_COMM_CAP_SWEEPS;
    ++levels;
    // L11
    hipLaunchKernelGGL(k_comm_alive, dim3(grid_of(nv)), dim3(GR_COMM_BLOCK), 0, s, nv, (const int32_t *)size, alive.flag());
    GR_HIP(c, hipGetLastError());
    GR_TRY(alive.scan.run(alive.flag(), alive.pos(), s, nv));
    hipLaunchKernelGGL(k_comm_relabel, dim3(grid_of(std::max(n, nnz))), dim3(GR_COMM_BLOCK), 0, s, n, nv, nnz, (const int32_t *)comm,
                       (const int32_t *)alive.flag(), (const int32_t *)alive.pos(), label, (const u64 *)ukeys, (const int64_t *)uvals, akeys, avals, ctl);
    GR_HIP(c, hipGetLastError());
    GR_TRY(sum_entries(nnz));
    GR_TRY(read_control());
    nnz = runs_h[0];
    nv = (int64_t)ctl_h[CT_NV2];
    GR_TRY(build_rows(nnz, nv, false));
  }
  if (!ended) caps |= GR_COMM_CAP_LEVELS;
  st[GR_COMM_STAT_LEVELS] = levels;
  st[GR_COMM_STAT_CAPS] = caps;

  // L12, L13: the final matrix has a row per community (and per vertex without an edge)
  GR_HIP(c, hipMemsetAsync(o_fsize(), 0, sizeof(int32_t) * (size_t)nv, s));
  GR_HIP(c, hipMemsetAsync(o_fmin(), 0x7F, sizeof(int32_t) * (size_t)nv, s));
  GR_HIP(c, hipMemsetAsync(ctl + CT_NCOMM, 0, sizeof(u64), s));
  hipLaunchKernelGGL(k_comm_members, dim3(grid_of(n)), dim3(GR_COMM_BLOCK), 0, s, n, (const int32_t *)label, (const u64 *)k, o_fsize(), o_fmin());
  hipLaunchKernelGGL(k_comm_order_keys, dim3(grid_of(nv)), dim3(GR_COMM_BLOCK), 0, s, n, nv, (const int32_t *)o_fsize(), (const int32_t *)o_fmin(),
                     o_okey(), o_oval(), ctl);
  GR_HIP(c, hipGetLastError());
  GR_TRY(order.run(o_okey(), o_okey2(), o_oval(), o_oval2(), s, nv));
  hipLaunchKernelGGL(k_comm_write_communities, dim3(grid_of(nv)), dim3(GR_COMM_BLOCK), 0, s, nv, (const int32_t *)o_oval2(), (const int32_t *)o_fsize(),
                     (const u64 *)k, (const int64_t *)rowptr, (const int32_t *)col, (const int64_t *)uvals, o_newid(), comm_size, comm_in, comm_tot);
  hipLaunchKernelGGL(k_comm_write_labels, dim3(grid_of(n)), dim3(GR_COMM_BLOCK), 0, s, n, (const int32_t *)label, (const u64 *)k,
                     (const int32_t *)o_newid(), community);
  GR_HIP(c, hipGetLastError());
  GR_TRY(read_control());
  st[GR_COMM_STAT_COMMUNITIES] = (int64_t)ctl_h[CT_NCOMM];
  return finish(GR_OK);
}

int gr_community_points(gr_ctx *c, const double *starts, const double *ends, const int32_t *community, int64_t n, int64_t n_communities,
                        double *points, void *stream) {
  if (!c) return GR_EINVAL;
  if (n < 0 || n > GR_COMM_MAX_VERTICES || n_communities < 0 || n_communities > n)
    return fail(c, GR_EINVAL, "gr_community_points: bad arguments n=%lld n_communities=%lld (n <= %d, n_communities <= n)", (long long)n,
                (long long)n_communities, (int)GR_COMM_MAX_VERTICES);
  if (n_communities == 0) return GR_OK;
  if (!starts || !ends || !community || !points) return fail(c, GR_EINVAL, "gr_community_points: null arrays");
  hipStream_t s = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  const int64_t M = n_communities;
  Plan p;
  const auto o_rec = p.array<RayRec>(n);
  const auto o_keys = p.array<uint32_t>(n), o_skeys = p.array<uint32_t>(n);
  const auto o_rays = p.array<int32_t>(n), o_srays = p.array<int32_t>(n);
  const auto o_first = p.array<int32_t>(M), o_count = p.array<int32_t>(M);
  const SortPairs<uint32_t, int32_t> sort(c, p, n, bit_length(M));   // stable: the members of a community in ascending order
  int rc = stage_acquire(c, c->stage, p.finish(), s, "community-points");
  if (rc != GR_OK) return rc;
  p.base = c->stage.ptr;
  GR_HIP(c, hipMemsetAsync(o_first(), 0, sizeof(int32_t) * (size_t)M, s));
  GR_HIP(c, hipMemsetAsync(o_count(), 0, sizeof(int32_t) * (size_t)M, s));
  hipLaunchKernelGGL(k_comm_ray_prep, dim3(grid_of(n)), dim3(GR_COMM_BLOCK), 0, s, starts, ends, n, community, M, o_rec(), o_keys(), o_rays());
  GR_HIP(c, hipGetLastError());
  GR_TRY(sort.run(o_keys(), o_skeys(), o_rays(), o_srays(), s));
  hipLaunchKernelGGL(k_comm_member_runs, dim3(grid_of(n)), dim3(GR_COMM_BLOCK), 0, s, (const uint32_t *)o_skeys(), n, M, o_first(), o_count());
  hipLaunchKernelGGL(k_community_points, dim3((unsigned)M), dim3(GR_COMM_BLOCK), 0, s, (const RayRec *)o_rec(), ends, (const int32_t *)o_srays(),
                     (const int32_t *)o_first(), (const int32_t *)o_count(), points);
  GR_HIP(c, hipGetLastError());
  GR_HIP(c, hipStreamSynchronize(s));   // the scratch is free on return
  return GR_OK;
}

}  // extern "C"
