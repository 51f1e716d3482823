// geograypher_amd/csrc/decimate.hip -- mesh decimation by vertex clustering on a uniform grid (gr_cluster_count, gr_cluster_decimate;
// the rule-set is DESIGN.md section 8n, D1-D9).  Needs no uploaded mesh.  Integers only: every result is a minimum, a flag or a
// sum of ones, and every order is that of a stable radix sort, so nothing depends on scheduling.
//
// Vertices (D2, D3): k_decim_keys gives vertex i its cell key cx << 42 | cy << 21 | cz and the squared distance d2 of its doubled
// offset to the cell's centre.  Two stable radix passes order the vertices by (key, d2, index): first by d2 (the input is in index
// order), then by key.  The first vertex of every run of equal keys (k_decim_heads) is the cell's representative; an inclusive
// maximum scan carries the head's position along its run and k_decim_scatter_rep writes rep[i].  A vertex outside the key range
// (q < 0 or a cell component >= 2^21) takes the key ~0, which no cell has: it sorts behind every cell, starts no run and has
// rep -1.  The probe (gr_cluster_count) is the key kernel, one SortKeys and the head count.
// The minimum of (d2, index) per cell is formed by the second sort, not by a keyed reduction or by atomics: the library's
// other stages already lean on DeviceRadixSort and DeviceScan alone, and no cell's 64-bit word is contended.
// Faces (D5-D7): k_decim_faces maps a face to its representatives, drops it when two agree (or when it names a vertex that does
// not exist or that has no cell) and packs the sorted triple lo < mid < hi as the major key lo << vbits | mid and the minor key
// hi.  Two stable passes (by hi, then by the major key) order the survivors by triple, equal triples by face index;
// k_decim_face_flags keeps the first face of every run and marks its three vertices.
// Compaction (D7, D8): the two exclusive scans and the write kernel of gr_submesh_extract (k_submesh_write, compact_dev.hpp) over the
// remapped faces.
// One lane per vertex or face, 256-lane workgroups, no LDS; every index is checked before it is used.
#include "compact_dev.hpp"
#include "cub_steps.hpp"
#include "geom_dev.hpp"
#include "gr_internal.hpp"

using namespace grimpl;

namespace {

typedef unsigned long long u64;

#define GR_DECIM_NO_CELL (~0ull)       // the key of a vertex outside the key range
#define GR_DECIM_CELL_LIMIT (1ll << 21)   // cells per axis

// key [V], and with d2 != null: d2 [V], idx [V] = i.  `outside` (or null): the word that counts the vertices outside the key range.
__global__ __launch_bounds__(256) void k_decim_keys(const int64_t *__restrict__ vq, int64_t V, int64_t s, u64 *__restrict__ key,
                                                    u64 *__restrict__ d2, int32_t *__restrict__ idx, u64 *__restrict__ outside) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool out = false;
  if (i < V) {
    u64 k = 0, d = 0;
    for (int a = 0; a < 3; ++a) {
      const int64_t q = vq[i * 3 + a];
      const int64_t c = q >= 0 ? q / s : GR_DECIM_CELL_LIMIT;
      if (c >= GR_DECIM_CELL_LIMIT) { out = true; continue; }
      const int64_t t = 2 * (q - c * s) - s;   // |t| <= s <= 2^30
      k = (k << 21) | (u64)c;
      d += (u64)(t * t);                        // < 3 * 2^60
    }
    key[i] = out ? GR_DECIM_NO_CELL : k;
    if (d2) { d2[i] = out ? 0ull : d; idx[i] = (int32_t)i; }
  }
  if (outside) stat_count(outside, 0, out, lane);
}

// dst [p] = src [order [p]]
__global__ __launch_bounds__(256) void k_decim_gather(const u64 *__restrict__ src, const int32_t *__restrict__ order, int64_t N,
                                                      u64 *__restrict__ dst) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < N) dst[p] = src[order[p]];
}

// key_s: the sorted keys.  Position p starts a cell when its key is a cell's and differs from the one before; hp [p] (or null) = p
// there, else 0.  *cells += the heads.
__global__ __launch_bounds__(256) void k_decim_heads(const u64 *__restrict__ key_s, int64_t V, int32_t *__restrict__ hp,
                                                     u64 *__restrict__ cells) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool head = false;
  if (p < V) {
    const u64 k = key_s[p];
    head = k != GR_DECIM_NO_CELL && (p == 0 || key_s[p - 1] != k);
    if (hp) hp[p] = head ? (int32_t)p : 0;
  }
  stat_count(cells, 0, head, lane);
}

// hpm [p]: the position of the head of p's run.  rep of the vertex at p = the vertex at that head; -1 outside the key range.
__global__ __launch_bounds__(256) void k_decim_scatter_rep(const u64 *__restrict__ key_s, const int32_t *__restrict__ idx_s,
                                                           const int32_t *__restrict__ hpm, int64_t V, int32_t *__restrict__ rep) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= V) return;
  rep[idx_s[p]] = key_s[p] == GR_DECIM_NO_CELL ? -1 : idx_s[hpm[p]];   // every vertex occurs once in idx_s: one writer
}

// D5: rf [f] = the three representatives (-1 where the face reads nothing), major [f] = lo << vbits | mid of the sorted triple of a
// surviving face, 1 << 2 vbits otherwise (behind every survivor), minor [f] = hi, fidx [f] = f.
__global__ __launch_bounds__(256) void k_decim_faces(const int32_t *__restrict__ faces, int64_t F, int64_t V,
                                                     const int32_t *__restrict__ rep, int vbits, int32_t *__restrict__ rf,
                                                     u64 *__restrict__ major, uint32_t *__restrict__ minor,
                                                     int32_t *__restrict__ fidx, u64 *__restrict__ stats) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false, collapsed = false;
  if (f < F) {
    int64_t v0, v1, v2;
    int32_t a = -1, b = -1, c = -1;
    bad = !load_face(faces, f, V, v0, v1, v2);
    if (!bad) {
      a = rep[v0]; b = rep[v1]; c = rep[v2];
      bad = a < 0 || b < 0 || c < 0;   // a vertex without a cell
    }
    if (bad) { a = -1; b = -1; c = -1; }
    collapsed = !bad && (a == b || b == c || a == c);
    rf[f * 3] = a; rf[f * 3 + 1] = b; rf[f * 3 + 2] = c;
    u64 mj = 1ull << (2 * vbits);
    uint32_t mn = 0;
    if (!bad && !collapsed) {
      const int32_t lo = min(a, min(b, c)), hi = max(a, max(b, c)), mid = (int32_t)((int64_t)a + b + c - lo - hi);
      mj = ((u64)(uint32_t)lo << vbits) | (u64)(uint32_t)mid;
      mn = (uint32_t)hi;
    }
    major[f] = mj; minor[f] = mn; fidx[f] = (int32_t)f;
  }
  stat_count(stats, GR_DECIM_STAT_COLLAPSED, collapsed, lane);
  stat_count(stats, GR_DECIM_STAT_BAD_FACES, bad, lane);
}

// D6: the faces in the order of (major, minor, face index).  The first of every run of equal triples is kept: fflag [its face] = 1
// and vused [its three representatives] = 1 (both zeroed by the caller).
__global__ __launch_bounds__(256) void k_decim_face_flags(const u64 *__restrict__ major_s, const int32_t *__restrict__ fidx_s,
                                                          const uint32_t *__restrict__ minor, const int32_t *__restrict__ rf, int64_t F,
                                                          int vbits, int32_t *__restrict__ fflag, int32_t *__restrict__ vused,
                                                          u64 *__restrict__ stats) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool duplicate = false;
  if (p < F) {
    const u64 mj = major_s[p];
    const int32_t f = fidx_s[p];
    if (mj != (1ull << (2 * vbits))) {   // a survivor of D5: its representatives are vertices
      duplicate = p > 0 && major_s[p - 1] == mj && minor[fidx_s[p - 1]] == minor[f];
      if (!duplicate) {
        fflag[f] = 1;
        for (int k = 0; k < 3; ++k) vused[rf[(int64_t)f * 3 + k]] = 1;   // every writer stores the same value
      }
    }
  }
  stat_count(stats, GR_DECIM_STAT_DUPLICATES, duplicate, lane);
}

int check_shape(gr_ctx *c, const char *name, const int64_t *verts_q, int64_t V, int64_t s) {
  if (V < 0 || V > 0x7FFFFFFFll) return fail(c, GR_EINVAL, "%s: bad shape V=%lld", name, (long long)V);
  if (s < 1 || s > (1ll << 30)) return fail(c, GR_EINVAL, "%s: cell side s=%lld outside [1, 2^30] grid steps", name, (long long)s);
  if (V > 0 && !verts_q) return fail(c, GR_EINVAL, "%s: null arrays", name);
  return GR_OK;
}

// bits of the largest d2 of cells of side s: d2 <= 3 s^2 < 2^(2 bit_length(s) + 2)
int d2_bits(int64_t s) { return std::min(2 * bit_length(s) + 2, 64); }

}  // namespace

extern "C" {

int gr_cluster_count(gr_ctx *c, const int64_t *verts_q, int64_t V, int64_t s, uint64_t *cells, void *stream) {
  if (!c) return GR_EINVAL;
  int rc = check_shape(c, "gr_cluster_count", verts_q, V, s);
  if (rc != GR_OK) return rc;
  if (!cells) return fail(c, GR_EINVAL, "gr_cluster_count: null arrays");
  hipStream_t st = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  GR_HIP(c, hipMemsetAsync(cells, 0, sizeof(uint64_t), st));
  if (V == 0) return GR_OK;
  // scratch: key [V] | key_s [V] | the sort's temporaries
  Plan p;
  const auto key = p.array<u64>(V), key_s = p.array<u64>(V);
  const SortKeys<u64> sort(c, p, V, 64);
  rc = stage_acquire(c, c->stage, p.finish(), st, "cluster-count");
  if (rc != GR_OK) return rc;
  p.base = c->stage.ptr;
  const dim3 grid((unsigned)ceil_div(V, 256));
  hipLaunchKernelGGL(k_decim_keys, grid, dim3(256), 0, st, verts_q, V, s, key(), (u64 *)nullptr, (int32_t *)nullptr, (u64 *)nullptr);
  GR_TRY(sort.run(key(), key_s(), st));
  hipLaunchKernelGGL(k_decim_heads, grid, dim3(256), 0, st, (const u64 *)key_s(), V, (int32_t *)nullptr, (u64 *)cells);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

int gr_cluster_decimate(gr_ctx *c, const int64_t *verts_q, int64_t V, const int32_t *faces, int64_t F, int64_t s, int32_t *rep,
                        int64_t *face_ids, int64_t *point_ids, int32_t *new_faces, uint64_t *stats, void *stream) {
  if (!c) return GR_EINVAL;
  int rc = check_shape(c, "gr_cluster_decimate", verts_q, V, s);
  if (rc != GR_OK) return rc;
  if (F < 0 || F > 0x7FFFFFFFll) return fail(c, GR_EINVAL, "gr_cluster_decimate: bad shape F=%lld", (long long)F);
  if (!stats || (V > 0 && (!rep || !point_ids)) || (F > 0 && (!faces || !face_ids || !new_faces)))
    return fail(c, GR_EINVAL, "gr_cluster_decimate: null arrays");
  hipStream_t st = (hipStream_t)stream;
  GR_HIP(c, hipSetDevice(c->device));
  u64 *stw = (u64 *)stats;
  GR_HIP(c, hipMemsetAsync(stw, 0, sizeof(uint64_t) * GR_DECIM_STAT_WORDS, st));
  if (V == 0 && F == 0) return GR_OK;
  const int vbits = std::max(bit_length(V - 1), 1), dbits = d2_bits(s);

  // scratch: vused [V] | vpos [V] | then the vertex phase: key, d2, alt [V] u64 | idx, idx_a, hp, hpm [V]
  //                                 or the face phase: rf [3 F] | major, major_a, major_s [F] u64 | minor, minor_s [F] | fidx, fidx_a,
  //                                                    fidx_s, fflag, fpos [F]               | hipcub's temporaries behind both
  Plan p;
  const FlagScan vs(c, p, V);
  const size_t phase = p.mark();
  const auto key = p.array<u64>(V), d2 = p.array<u64>(V), alt = p.array<u64>(V);
  const auto idx = p.array<int32_t>(V), idx_a = p.array<int32_t>(V), hp = p.array<int32_t>(V), hpm = p.array<int32_t>(V);
  const SortPairs<u64, int32_t> sort_d2(c, p, V, dbits), sort_key(c, p, V, 64);
  const InclusiveMax<int32_t> head_max(c, p, V);
  p.rewind(phase);
  const auto rf = p.array<int32_t>(3 * F);
  const auto major = p.array<u64>(F), major_a = p.array<u64>(F), major_s = p.array<u64>(F);
  const auto minor = p.array<uint32_t>(F), minor_s = p.array<uint32_t>(F);
  const auto fidx = p.array<int32_t>(F), fidx_a = p.array<int32_t>(F), fidx_s = p.array<int32_t>(F);
  const SortPairs<uint32_t, int32_t> sort_minor(c, p, F, vbits);
  const SortPairs<u64, int32_t> sort_major(c, p, F, 2 * vbits + 1);
  const FlagScan fs(c, p, F);
  rc = stage_acquire(c, c->stage, p.finish(), st, "cluster-decimate");
  if (rc != GR_OK) return rc;
  p.base = c->stage.ptr;

  if (V > 0) {   // D2, D3
    const dim3 grid((unsigned)ceil_div(V, 256));
    hipLaunchKernelGGL(k_decim_keys, grid, dim3(256), 0, st, verts_q, V, s, key(), d2(), idx(), stw + GR_DECIM_STAT_OUTSIDE);
    GR_TRY(sort_d2.run(d2(), alt(), idx(), idx_a(), st));     // by d2 (ties: by index)
    hipLaunchKernelGGL(k_decim_gather, grid, dim3(256), 0, st, (const u64 *)key(), (const int32_t *)idx_a(), V, d2());
    GR_TRY(sort_key.run(d2(), alt(), idx_a(), idx(), st));    // then by cell, stably
    hipLaunchKernelGGL(k_decim_heads, grid, dim3(256), 0, st, (const u64 *)alt(), V, hp(), stw + GR_DECIM_STAT_CELLS);
    GR_TRY(head_max.run(hp(), hpm(), st));
    hipLaunchKernelGGL(k_decim_scatter_rep, grid, dim3(256), 0, st, (const u64 *)alt(), (const int32_t *)idx(), (const int32_t *)hpm(), V, rep);
    GR_HIP(c, hipGetLastError());
  }
  if (F == 0) return GR_OK;   // no face: nothing is kept (D8)

  const dim3 gf((unsigned)ceil_div(F, 256));
  GR_TRY(compact_begin(c, vs, st));
  GR_HIP(c, hipMemsetAsync(fs.flag(), 0, sizeof(int32_t) * (size_t)F, st));
  hipLaunchKernelGGL(k_decim_faces, gf, dim3(256), 0, st, faces, F, V, (const int32_t *)rep, vbits, rf(), major(), minor(), fidx(), stw);   // D5
  GR_TRY(sort_minor.run(minor(), minor_s(), fidx(), fidx_a(), st));          // by hi
  hipLaunchKernelGGL(k_decim_gather, gf, dim3(256), 0, st, (const u64 *)major(), (const int32_t *)fidx_a(), F, major_a());
  GR_TRY(sort_major.run(major_a(), major_s(), fidx_a(), fidx_s(), st));      // then by (lo, mid), stably
  hipLaunchKernelGGL(k_decim_face_flags, gf, dim3(256), 0, st, (const u64 *)major_s(), (const int32_t *)fidx_s(), (const uint32_t *)minor(),
                     (const int32_t *)rf(), F, vbits, fs.flag(), vs.flag(), stw);                                            // D6
  // D7, D8; words GR_DECIM_STAT_KEPT_FACES, GR_DECIM_STAT_KEPT_VERTICES
  return compact_write(c, fs, vs, st, (const int32_t *)rf(), face_ids, point_ids, new_faces, stw);
}

}  // extern "C"
