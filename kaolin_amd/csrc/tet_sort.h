// The sort / scan / unique kernels that the tetrahedral pipelines share (marching_tetrahedra.hip, subdivide_tetmesh.hip):
// 16-byte tet loads, an exclusive scan of ints into int64 offsets, a stable 8-bit LSD radix sort of 64-bit keys alone, the
// heads / compaction of a sorted key list, and the rank of a key in the unique list.  Every name lives in an unnamed
// namespace: each translation unit gets its own copy.
#pragma once
#include "common.h"

namespace {

inline long long mt_cdiv(long long a, long long b) { return (a + b - 1) / b; }
inline unsigned mt_grid(long long items, int per_block) { return (unsigned)(items > 0 ? mt_cdiv(items, per_block) : 1); }

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

// ---- 3. exclusive scan of n ints into n + 1 int64 offsets (out[n] = total): sums of 1024-blocks, then apply -------------
__device__ __forceinline__ long long mt_block_inclusive(long long v, long long* s_wave) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  long long woff = 0;
  for (int k = 0; k < wave; ++k) woff += s_wave[k];
  return woff + inc;
}
__global__ __launch_bounds__(1024) void mt_scan_sums_kernel(long long n, const int* __restrict__ in, long long* __restrict__ sums) {
  __shared__ long long s_wave[16];
  const long long i = (long long)blockIdx.x * 1024 + threadIdx.x;
  const long long tot = mt_block_inclusive(i < n ? in[i] : 0, s_wave);
  if (threadIdx.x == 1023) sums[blockIdx.x] = tot;
}
__global__ __launch_bounds__(1024) void mt_scan_apply_kernel(long long n, const int* __restrict__ in,
                                                             const long long* __restrict__ sums, long long* __restrict__ out) {
  __shared__ long long s_wave[16];
  __shared__ long long s_off;
  long long part = 0;
  for (long long k = threadIdx.x; k < (long long)blockIdx.x; k += 1024) part += sums[k];
  const long long before = mt_block_inclusive(part, s_wave);
  if (threadIdx.x == 1023) s_off = before;
  __syncthreads();
  const long long off = s_off;
  __syncthreads();
  const long long i = (long long)blockIdx.x * 1024 + threadIdx.x;
  const long long v = i < n ? in[i] : 0;
  const long long inc = mt_block_inclusive(v, s_wave);
  if (i < n) out[i] = off + inc - v;
  if (i == n - 1) out[n] = off + inc;
}
int mt_scan(hipStream_t st, long long n, const int* in, long long* out, long long* sums) {  // n > 0
  const unsigned nb = mt_grid(n, 1024);
  hipLaunchKernelGGL(mt_scan_sums_kernel, dim3(nb), dim3(1024), 0, st, n, in, sums);
  hipLaunchKernelGGL(mt_scan_apply_kernel, dim3(nb), dim3(1024), 0, st, n, in, (const long long*)sums, out);
  return (int)hipGetLastError();
}

constexpr int MT_SORT_ITEMS = 8, MT_SORT_BLOCK = 256 * MT_SORT_ITEMS;

// ---- 5. stable LSD radix sort of the keys, 8 bits a pass ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void mt_sort_hist_kernel(long long n, const unsigned long long* __restrict__ keys, int shift,
                                                           long long nblk, int* __restrict__ hist) {
  __shared__ int s_h[256];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * MT_SORT_BLOCK;
#pragma unroll
  for (int r = 0; r < MT_SORT_ITEMS; ++r) {
    const long long e = base + r * 256 + threadIdx.x;
    if (e < n) atomicAdd(&s_h[(int)((keys[e] >> shift) & 255u)], 1);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * nblk + blockIdx.x] = s_h[threadIdx.x];
}
// ranks the keys of a block in their original order: wavefront by wavefront (the lanes sharing a digit found with eight ballots,
// lower lanes first), wavefronts and rounds of 256 in order through LDS counters
__global__ __launch_bounds__(256) void mt_sort_scatter_kernel(long long n, const unsigned long long* __restrict__ keys, int shift,
                                                              long long nblk, const long long* __restrict__ offs,
                                                              unsigned long long* __restrict__ keys_out) {
  __shared__ long long s_run[256];
  __shared__ int s_wc[4][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  s_run[tid] = offs[(size_t)tid * nblk + blockIdx.x];
#pragma unroll
  for (int w = 0; w < 4; ++w) s_wc[w][tid] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * MT_SORT_BLOCK;
  for (int r = 0; r < MT_SORT_ITEMS; ++r) {
    const long long e = base + r * 256 + tid;
    const bool on = e < n;
    const unsigned long long key = on ? keys[e] : 0ull;
    const int digit = (int)((key >> shift) & 255u);
    unsigned long long peers = __ballot(on);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const unsigned long long m = __ballot((digit >> bit) & 1);
      peers &= ((digit >> bit) & 1) ? m : ~m;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    if (on && rank == 0) s_wc[wave][digit] = __popcll(peers);
    __syncthreads();
    if (on) {
      long long pos = s_run[digit] + rank;
      for (int w = 0; w < wave; ++w) pos += s_wc[w][digit];
      keys_out[pos] = key;  // pos < n: the offsets are the scan of exactly these n keys' digit counts
    }
    __syncthreads();
    s_run[tid] += (s_wc[0][tid] + s_wc[1][tid]) + (s_wc[2][tid] + s_wc[3][tid]);
#pragma unroll
    for (int w = 0; w < 4; ++w) s_wc[w][tid] = 0;
    __syncthreads();
  }
}

// ---- 6. unique keys ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mt_heads_kernel(long long n, const unsigned long long* __restrict__ keys,
                                                       int* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) flags[i] = (i == 0 || keys[i - 1] != keys[i]) ? 1 : 0;
}
__global__ __launch_bounds__(256) void mt_unique_kernel(long long n, const unsigned long long* __restrict__ keys,
                                                        const int* __restrict__ flags, const long long* __restrict__ pos,
                                                        unsigned long long* __restrict__ uniq) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n && flags[i]) uniq[pos[i]] = keys[i];  // pos[i] < pos[n] <= n
}

__device__ __forceinline__ long long mt_rank(const unsigned long long* __restrict__ uniq, long long nu, unsigned long long key) {
  long long lo = 0, hi = nu;  // first element >= key; the key is present
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (uniq[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

}  // namespace
