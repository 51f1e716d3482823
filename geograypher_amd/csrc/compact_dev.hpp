#pragma once
// geograypher_amd/csrc/compact_dev.hpp -- the flag / scan / write compaction of a mesh, shared by gr_submesh_extract (polygons.hip)
// and gr_cluster_decimate (decimate.hip): both flag the kept faces and the vertices they use; compact_write scans the flags
// (ExclusiveSum, cub_steps.hpp) and k_submesh_write writes the kept faces and vertices in their original order.  HIP only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cub_steps.hpp"

namespace {

// fflag [F], vused [V]: 1 where kept; fpos, vpos: their exclusive sums.  `faces` names the vertices of every kept face (in range
// and used; the other rows are not read).  One thread per face and per vertex.  counts [0], [1] = kept faces, kept vertices.
__global__ __launch_bounds__(256) void k_submesh_write(const int32_t *__restrict__ faces, int64_t F, int64_t V,
                                                       const int32_t *__restrict__ fflag, const int32_t *__restrict__ fpos,
                                                       const int32_t *__restrict__ vused, const int32_t *__restrict__ vpos,
                                                       int64_t *__restrict__ face_ids, int64_t *__restrict__ point_ids,
                                                       int32_t *__restrict__ new_faces, unsigned long long *__restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < F && fflag[i]) {   // a kept face's vertices are in range and used
    const int64_t j = fpos[i];
    face_ids[j] = i;
    for (int k = 0; k < 3; ++k) new_faces[j * 3 + k] = vpos[faces[i * 3 + k]];
  }
  if (i < V && vused[i]) point_ids[vpos[i]] = i;
  if (i == 0) {
    counts[0] = F > 0 ? (unsigned long long)(fpos[F - 1] + fflag[F - 1]) : 0ull;
    counts[1] = V > 0 ? (unsigned long long)(vpos[V - 1] + vused[V - 1]) : 0ull;
  }
}

}  // namespace

namespace grimpl {
namespace {

// flag [n] | pos [n] of the faces or of the vertices, and the exclusive sum that takes the one to the other
struct FlagScan {
  int64_t n;
  Slot<int32_t> flag, pos;
  ExclusiveSum<int32_t> scan;
  FlagScan(gr_ctx *c, Plan &p, int64_t n_) : n(n_), flag(p.array<int32_t>(n_)), pos(p.array<int32_t>(n_)), scan(c, p, n_) {}
};

// The host side.  The caller declares a FlagScan of the faces and one of the vertices where its layout has them.  Behind the
// acquisition compact_begin zeroes vused (a face marks only the vertices it uses); the caller's kernel leaves fflag [f] set for
// every face; compact_write scans both and launches k_submesh_write over `tri`, the [F][3] rows whose vertices the kept faces name.
inline int compact_begin(gr_ctx *c, const FlagScan &v, hipStream_t s) {
  if (v.n > 0) GR_HIP(c, hipMemsetAsync(v.flag(), 0, sizeof(int32_t) * (size_t)v.n, s));
  return GR_OK;
}
inline int compact_write(gr_ctx *c, const FlagScan &f, const FlagScan &v, hipStream_t s, const int32_t *tri, int64_t *face_ids,
                         int64_t *point_ids, int32_t *new_faces, unsigned long long *counts) {
  GR_TRY(f.scan.run(f.flag(), f.pos(), s));
  if (v.n > 0) GR_TRY(v.scan.run(v.flag(), v.pos(), s));
  hipLaunchKernelGGL(k_submesh_write, dim3((unsigned)ceil_div(std::max(f.n, v.n), 256)), dim3(256), 0, s, tri, f.n, v.n,
                     (const int32_t *)f.flag(), (const int32_t *)f.pos(), (const int32_t *)v.flag(), (const int32_t *)v.pos(), face_ids,
                     point_ids, new_faces, counts);
  GR_HIP(c, hipGetLastError());
  return GR_OK;
}

}  // namespace
}  // namespace grimpl
