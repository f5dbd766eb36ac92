// The stage walker of the SPC voxelizers, with the primitive's voxel test as a template parameter.
// Lifted out of mesh_to_spc.hip (launch shapes and every test's arithmetic unchanged: tests/test_mesh_to_spc.py is the guard) and
// shared with gs_to_spc.hip.
// Every name lives in an unnamed namespace: each translation unit gets its own copy.
//
// PRIM must provide
//   struct Data;                                                        what a lane keeps of a primitive (registers)
//   __device__ bool  load(int64_t id, Data*) const;                     false: id is outside the primitive table (nothing is emitted)
//   __device__ bool  test(const Data&, int x, int y, int z, int level) const;
#pragma once
#include "common.h"
#include "spc_octree.h"

namespace {

// ---- a stage: every proposal (voxel at level_from, primitive) walks its subtree down to level_to ------------------------
// EMIT = false: counts[i] = number of voxels at level_to that pass with all their ancestors;
// EMIT = true : writes them (ascending Morton code) at offsets[i]; a slot at or beyond `total` (the count pass's sum) is never
// written.  `tested` = the proposal's own level passed already.
// Eight lanes share a proposal: they test the eight children of the current node at once (one ballot), then the group
// descends into the survivors in child order, keeping the not-yet-visited children of each depth as 8 bits of one word
// (so level_to - level_from <= 4).  All groups of a wavefront run the same loop; a group that is done idles until the last one
// finishes.  The loop ends: every iteration either clears a bit of `rem`, or moves up, or retires the group.
template <bool EMIT, class PRIM>
__global__ __launch_bounds__(256) void spc_stage_kernel(int64_t n, PRIM prim, const int64_t* __restrict__ morton,
                                                        const int64_t* __restrict__ prim_id, int level_from, int level_to,
                                                        int tested, int* __restrict__ counts, const int64_t* __restrict__ offsets,
                                                        int64_t total, int64_t* __restrict__ morton_out,
                                                        int64_t* __restrict__ prim_id_out) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i = gid >> 3;
  const int k = (int)(gid & 7), grp = (threadIdx.x & 63) >> 3;
  bool active = i < n;
  int64_t t = 0, o = 0;
  typename PRIM::Data T = {};
  int cx = 0, cy = 0, cz = 0, count = 0, d = 0;
  unsigned rem = 0;  // 8 bits per depth: children still to visit
  bool expand = false;
  if (active) {
    t = prim_id[i];
    ms_to_point((uint64_t)morton[i], &cx, &cy, &cz);
    if (EMIT) o = offsets[i];
    if (!prim.load(t, &T)) {
      active = false;
    } else if (!(tested || prim.test(T, cx, cy, cz, level_from))) {
      active = false;
    } else if (level_from == level_to) {
      if (EMIT && k == 0 && o < total) {
        morton_out[o] = morton[i];
        prim_id_out[o] = t;
      }
      count = 1;
      active = false;
    } else {
      expand = true;
    }
  }
  while (__any(active)) {
    bool pass = false;
    int nx = 0, ny = 0, nz = 0;
    const int nl = level_from + d + 1;
    if (active && expand) {
      nx = 2 * cx + (k >> 2);
      ny = 2 * cy + ((k >> 1) & 1);
      nz = 2 * cz + (k & 1);
      pass = prim.test(T, nx, ny, nz, nl);
    }
    const unsigned long long bal = __ballot(pass);
    if (active) {
      if (expand) {
        unsigned mask = (unsigned)((bal >> (8 * grp)) & 0xFFull);
        if (nl == level_to) {
          if (EMIT && pass) {
            const int64_t q = o + count + __popc(mask & ((1u << k) - 1u));
            if (q < total) {
              morton_out[q] = (int64_t)ms_to_morton(nx, ny, nz);
              prim_id_out[q] = t;
            }
          }
          count += __popc(mask);
          mask = 0;
        }
        rem = (rem & ~(0xFFu << (8 * d))) | (mask << (8 * d));
        expand = false;
      }
      const unsigned todo = (rem >> (8 * d)) & 0xFFu;
      if (todo != 0u) {  // descend into the next surviving child
        const int c = __builtin_ctz(todo);
        rem &= ~(1u << (8 * d + c));
        cx = 2 * cx + (c >> 2);
        cy = 2 * cy + ((c >> 1) & 1);
        cz = 2 * cz + (c & 1);
        ++d;
        expand = true;
      } else if (d == 0) {
        active = false;
      } else {  // back to the parent
        --d;
        cx >>= 1;
        cy >>= 1;
        cz >>= 1;
      }
    }
  }
  if (!EMIT && i < n && k == 0) counts[i] = count;
}

}  // namespace
