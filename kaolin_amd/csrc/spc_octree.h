// The octree kernels that the two SPC builders share (mesh_to_spc.hip, spc.hip): the Morton layout, the parents of a level (code +
// children bitmap, from the run heads and scan of sort_scan.h) and the gather of the levels into one octree.  Every name lives
// in an unnamed namespace: each translation unit gets its own copy.
#pragma once
#include "common.h"

namespace {

// ---- Morton layout of spc_math.h:98-126: bit 3i = z_i, 3i+1 = y_i, 3i+2 = x_i ----------------------------------------
__device__ __forceinline__ uint64_t ms_spread3(uint64_t v) {  // 15 bits -> every third bit
  v &= 0x7FFFull;
  v = (v | (v << 32)) & 0x1F00000000FFFFull;
  v = (v | (v << 16)) & 0x1F0000FF0000FFull;
  v = (v | (v << 8)) & 0x100F00F00F00F00Full;
  v = (v | (v << 4)) & 0x10C30C30C30C30C3ull;
  v = (v | (v << 2)) & 0x1249249249249249ull;
  return v;
}
__device__ __forceinline__ uint64_t ms_to_morton(int x, int y, int z) {
  return (ms_spread3((uint64_t)x) << 2) | (ms_spread3((uint64_t)y) << 1) | ms_spread3((uint64_t)z);
}
__device__ __forceinline__ int ms_compact3(uint64_t v) {  // every third bit -> 15 bits
  v &= 0x1249249249249249ull;
  v = (v | (v >> 2)) & 0x10C30C30C30C30C3ull;
  v = (v | (v >> 4)) & 0x100F00F00F00F00Full;
  v = (v | (v >> 8)) & 0x1F0000FF0000FFull;
  v = (v | (v >> 16)) & 0x1F00000000FFFFull;
  v = (v | (v >> 32)) & 0x7FFFull;
  return (int)v;
}
__device__ __forceinline__ void ms_to_point(uint64_t m, int* x, int* y, int* z) {
  *x = ms_compact3(m >> 2);
  *y = ms_compact3(m >> 1);
  *z = ms_compact3(m);
}

__global__ __launch_bounds__(256) void ms_copy_words_kernel(int64_t n, const int64_t* __restrict__ a, int64_t* __restrict__ a_out,
                                                            const int64_t* __restrict__ b, int64_t* __restrict__ b_out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    a_out[i] = a[i];
    if (b != nullptr) b_out[i] = b[i];
  }
}

// ---- after the sort: one voxel per run of equal Morton codes, then the octree bottom-up --------------------------------
// sizes[0] = voxels, sizes[1 + l] = nodes of octree level l (root = level 0)
// nodes of the level above: parent code + children bitmap of every run of siblings (spc_cuda.cu:64-90)
__global__ __launch_bounds__(256) void ms_parents_kernel(const int64_t* __restrict__ n_ptr, const int64_t* __restrict__ m,
                                                         const int* __restrict__ flag, const int64_t* __restrict__ pos,
                                                         int64_t* __restrict__ m_out, unsigned char* __restrict__ bytes,
                                                         int64_t* __restrict__ size_out) {
  const int64_t n = *n_ptr;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && flag[i]) {
    unsigned code = 0;
    int64_t j = i;
    do {
      code |= 1u << ((unsigned)m[j] & 7u);
      ++j;
    } while (j < n && !flag[j]);
    m_out[pos[i]] = (int64_t)((uint64_t)m[i] >> 3);
    bytes[pos[i]] = (unsigned char)code;
  }
  if (i == 0) *size_out = n > 0 ? pos[n] : 0;
}

__global__ __launch_bounds__(256) void ms_gather_octree_kernel(int level, int64_t stride, const int64_t* __restrict__ sizes,
                                                               const unsigned char* __restrict__ level_bytes,
                                                               unsigned char* __restrict__ octree) {
  int64_t off = 0;
  for (int l = 0; l < level; ++l) {
    const int64_t nl = sizes[1 + l];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nl; i += (int64_t)gridDim.x * 256)
      octree[off + i] = level_bytes[(size_t)l * stride + i];
    off += nl;
  }
}

}  // namespace
