// The wavefront and workgroup scans every pipeline builds on: device functions only.  Every name lives in an unnamed namespace:
// each translation unit gets its own copy (the convention of sort_scan.h).
//   * wave_inclusive       the __shfl_up ladder over the 64 lanes, one value per lane
//   * block_inclusive      on top of it, one value per thread of a workgroup: the two-level scans of sort_scan.h, the pixel grid
//                          of deftet.hip and the cell grid of sided_distance_grid.hip
//   * block_exclusive      the same with the workgroup's total, reusable round after round: count_scan.h
//   * ballot_prefix        the prefix of a count of a few bits per lane from __ballot / __popcll: the ranks inside a workgroup of
//                          cubic_meshes.hip, mcube.hip and flexicubes.hip
#pragma once
#include "common.h"

namespace {

// inclusive sums over the lanes of a wavefront; lane = threadIdx.x & 63
template <typename V>
__device__ __forceinline__ V wave_inclusive(V v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const V o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// inclusive sums of one value per thread over the workgroup (the last thread's result is the total).  s_wave: blockDim.x / 64
// words, which the caller must not rewrite (a second scan included) before every thread has passed a barrier.
template <typename V>
__device__ __forceinline__ V block_inclusive(V v, V* s_wave) {
  const int lane = threadIdx.x & 63;
  const V inc = wave_inclusive(v, lane);
  const int wave = threadIdx.x >> 6;
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  V woff = 0;
  for (int w = 0; w < wave; ++w) woff += s_wave[w];
  return woff + inc;
}

// exclusive scan of one value per thread over the workgroup; *total = the sum.  s_w: (blockDim.x / 64 + 1) words.
template <typename V>
__device__ __forceinline__ V block_exclusive(V v, V* s_w, V* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const V incl = wave_inclusive(v, lane);
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  if (wave == 0) {
    const V w = lane < nw ? s_w[lane] : (V)0;
    const V wi = wave_inclusive(w, lane);
    if (lane < nw) s_w[lane] = wi - w;
    if (lane == nw - 1) s_w[nw] = wi;
  }
  __syncthreads();
  const V res = s_w[wave] + incl - v;
  *total = s_w[nw];
  __syncthreads();  // (s_w is rewritten by the next round)
  return res;
}

// a count of NB bits per thread: its sum over the lower lanes of the wavefront; the wavefront's sum to *s_wave_slot (the
// caller's slot of this wavefront, &s[wave]), to be read after a barrier
template <int NB>
__device__ __forceinline__ unsigned ballot_prefix(unsigned count, unsigned* s_wave_slot) {
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned prefix = 0u, sum = 0u;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const unsigned long long m = __ballot((count >> b) & 1u);
    prefix += (unsigned)__popcll(m & below) << b;
    sum += (unsigned)__popcll(m) << b;
  }
  if (lane == 0) *s_wave_slot = sum;
  return prefix;
}

}  // namespace
