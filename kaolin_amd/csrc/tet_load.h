// The 16-byte loads of a tet's four vertex ids, shared by the tetrahedral pipelines (marching_tetrahedra.hip,
// subdivide_tetmesh.hip).  Every name lives in an unnamed namespace: each translation unit gets its own copy.
#pragma once
#include "common.h"

namespace {

struct MtTet {
  unsigned long long id[4];
};
__device__ __forceinline__ MtTet mt_load_tet(const int64_t* __restrict__ tets, long long t) {
  const ulonglong2* p = (const ulonglong2*)(tets + 4 * t);  // (T, 4) contiguous, 16-byte aligned base (checked on the host)
  const ulonglong2 lo = p[0], hi = p[1];
  MtTet r;
  r.id[0] = lo.x, r.id[1] = lo.y, r.id[2] = hi.x, r.id[3] = hi.y;
  return r;
}

}  // namespace
