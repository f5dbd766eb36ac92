// What the sort-free grid pipelines (cubic_meshes.hip, mcube.hip, flexicubes.hip) share on top of block_scan.h.  Their classify
// kernels leave one count per workgroup and counter; a rank is then a prefix count:
//   * rows_scan_kernel     one workgroup per row of workgroup counts: exclusive scan in place, the row's total beside it
//   * bases_kernel         the int64 prefix over the batch items of the vertex and face totals (cubic meshes, marching cubes)
//   * the grid of a persistent kernel, and a grid value of u8 / f16 / f32 as float
// Every name lives in an unnamed namespace: each translation unit gets its own copy.
#pragma once
#include "block_scan.h"

namespace {

constexpr int COUNT_SCAN_THREADS = 1024;
constexpr int COUNT_SCAN_ITEMS = 8;  // consecutive counts per thread and round of the scan: 8192 workgroups per round
constexpr int BASES_THREADS = 256;   // batch items per round of the bases

// a float16 as its bits: the C ABI passes these grids as void*
struct half_bits {
  unsigned short bits;
};
__device__ __forceinline__ float grid_value(unsigned char v) { return (float)v; }
__device__ __forceinline__ float grid_value(float v) { return v; }
__device__ __forceinline__ float grid_value(half_bits v) { return __half2float(__ushort_as_half(v.bits)); }
__device__ __forceinline__ void grid_store(float* p, float v) { *p = v; }
__device__ __forceinline__ void grid_store(half_bits* p, float v) { p->bits = __half_as_ushort(__float2half(v)); }

// the workgroups of a persistent kernel over `blocks` rounds: at most 32 per CU, at least one
inline unsigned count_grid(long long blocks) {
  const long long cap = (long long)KAMD_NUM_CU * 32;
  return (unsigned)(blocks < 1 ? 1 : blocks < cap ? blocks : cap);
}

// row = blockIdx.x: counts[row * G .. + G) <- its exclusive scan, totals[row] <- its sum (the caller knows why it fits 32 bits)
__global__ __launch_bounds__(COUNT_SCAN_THREADS) void rows_scan_kernel(long long G, unsigned* __restrict__ counts,
                                                                       unsigned* __restrict__ totals) {
  __shared__ unsigned s_w[COUNT_SCAN_THREADS / 64 + 1];
  unsigned* row = counts + (long long)blockIdx.x * G;
  unsigned carry = 0u;
  for (long long base = 0; base < G; base += COUNT_SCAN_THREADS * COUNT_SCAN_ITEMS) {
    const long long first = base + (long long)threadIdx.x * COUNT_SCAN_ITEMS;
    unsigned c[COUNT_SCAN_ITEMS], sum = 0u;
#pragma unroll
    for (int e = 0; e < COUNT_SCAN_ITEMS; ++e) {
      c[e] = first + e < G ? row[first + e] : 0u;
      sum += c[e];
    }
    unsigned total;
    unsigned run = carry + block_exclusive(sum, s_w, &total);
#pragma unroll
    for (int e = 0; e < COUNT_SCAN_ITEMS; ++e) {
      if (first + e < G) row[first + e] = run;
      run += c[e];
    }
    carry += total;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}
inline void rows_scan(hipStream_t st, long long rows, long long G, unsigned* counts, unsigned* totals) {
  hipLaunchKernelGGL(rows_scan_kernel, dim3((unsigned)rows), dim3(COUNT_SCAN_THREADS), 0, st, G, counts, totals);
}

// an item has NC counters: its vertices, then NC - 1 kinds of faces.  bases[2 b], bases[2 b + 1] <- the vertices and the faces
// of the items before b (int64: the batch may exceed 2^31 rows).  One workgroup, the batch in rounds of BASES_THREADS items.
template <int NC>
__global__ __launch_bounds__(BASES_THREADS) void bases_kernel(long long B, const unsigned* __restrict__ totals,
                                                              long long* __restrict__ bases) {
  __shared__ long long s_w[BASES_THREADS / 64 + 1];
  long long carry_v = 0, carry_f = 0;
  for (long long base = 0; base < B; base += BASES_THREADS) {
    const long long b = base + threadIdx.x;
    long long nv = 0, nf = 0;
    if (b < B) {
      nv = totals[NC * b];
#pragma unroll
      for (int k = 1; k < NC; ++k) nf += totals[NC * b + k];
    }
    long long tv, tf;
    const long long ev = block_exclusive(nv, s_w, &tv);
    const long long ef = block_exclusive(nf, s_w, &tf);
    if (b < B) {
      bases[2 * b] = carry_v + ev;
      bases[2 * b + 1] = carry_f + ef;
    }
    carry_v += tv;
    carry_f += tf;
  }
}
template <int NC>
inline void batch_bases(hipStream_t st, long long B, const unsigned* totals, long long* bases) {
  hipLaunchKernelGGL((bases_kernel<NC>), dim3(1), dim3(BASES_THREADS), 0, st, B, totals, bases);
}

}  // namespace
