#pragma once
// geograypher_amd/csrc/compact_dev.hpp -- the write kernel of the flag / scan / write compaction of a mesh, shared by
// gr_submesh_extract (polygons.hip) and gr_cluster_decimate (decimate.hip): both flag the kept faces and the vertices they use,
// scan the flags (hipcub::DeviceScan::ExclusiveSum) and write the kept faces and vertices in their original order.  HIP only.
#include <hip/hip_runtime.h>

#include <cstdint>

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
