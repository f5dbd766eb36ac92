// The scan / sort / unique primitives of every sort-based pipeline (marching tetrahedra, tet and Loop subdivision, the SPC octree
// build, the dual octree, mesh / Gaussians / point clouds to SPC, bf_recon, SPC ray tracing):
//   * a two-level scan of 64-bit sums over the workgroup scan of block_scan.h: an exclusive one of ints into n + 1 int64 offsets
//     whose length may live on the device, and an inclusive one into ints of the ints themselves or of the bit counts of bytes;
//   * a stable 8-bit LSD radix sort of 64-bit keys, alone or with a 64-bit value each, over a list of pass shifts;
//   * the heads of the runs of equal (shifted) keys, their scan, the compaction of the heads, and the rank of a key among them.
// The sizes of their scratch are sort_scan_host.h's.  Every name lives in an unnamed namespace: each translation unit gets its
// own copy.  int64_t / long long and uint64_t / unsigned long long are distinct types of one width and the pipelines spell
// their buffers either way: the host functions take any 8-byte integer (SS_IS_WORD) and the kernels see (unsigned) long long.
#pragma once
#include "block_scan.h"
#include "common.h"
#include "sort_scan_host.h"

namespace {

#define SS_IS_WORD(T) static_assert(sizeof(T) == 8, "a 64-bit integer buffer")

inline unsigned ss_grid(long long items, int per_block) { return (unsigned)(items > 0 ? ss_cdiv(items, per_block) : 1); }

// ---- the scan: block_inclusive (block_scan.h) over the 1024 threads of a workgroup, 64-bit sums ----------------------------------
// what an element adds to the sum: an int itself, a byte its bit count
__device__ __forceinline__ long long ss_scan_value(const int* in, long long i) { return in[i]; }
__device__ __forceinline__ long long ss_scan_value(const unsigned char* in, long long i) { return __popc((unsigned)in[i]); }

// two levels: the sums of the 1024-blocks, then every block adds the sums of the blocks before it to its own scan.
// n may live on the device (n_ptr != nullptr): entries at or beyond it count as 0
template <typename In>
__global__ __launch_bounds__(SS_SCAN_BLOCK) void ss_scan_sums_kernel(long long n_host, const long long* __restrict__ n_ptr,
                                                                     const In* __restrict__ in, long long* __restrict__ sums) {
  __shared__ long long s_wave[16];
  const long long n = n_ptr ? *n_ptr : n_host;
  const long long i = (long long)blockIdx.x * SS_SCAN_BLOCK + threadIdx.x;
  const long long tot = block_inclusive(i < n ? ss_scan_value(in, i) : 0, s_wave);
  if (threadIdx.x == SS_SCAN_BLOCK - 1) sums[blockIdx.x] = tot;
}
// the inclusive sum at element i = blockIdx.x * 1024 + threadIdx.x over all elements up to it; *own = the element's own value
template <typename In>
__device__ __forceinline__ long long ss_scan_apply(long long n, const In* __restrict__ in, const long long* __restrict__ sums,
                                                   long long* own) {
  __shared__ long long s_wave[16];
  __shared__ long long s_off;
  long long part = 0;
  for (int k = threadIdx.x; k < (int)blockIdx.x; k += SS_SCAN_BLOCK) part += sums[k];
  const long long before = block_inclusive(part, s_wave);
  if (threadIdx.x == SS_SCAN_BLOCK - 1) s_off = before;
  __syncthreads();
  const long long off = s_off;
  __syncthreads();
  const long long i = (long long)blockIdx.x * SS_SCAN_BLOCK + threadIdx.x;
  *own = i < n ? ss_scan_value(in, i) : 0;
  return off + block_inclusive(*own, s_wave);
}
// exclusive, n + 1 outputs: out[n] = the total (n == 0: out[0] = 0)
__global__ __launch_bounds__(SS_SCAN_BLOCK) void ss_scan_exclusive_kernel(long long n_host, const long long* __restrict__ n_ptr,
                                                                          const int* __restrict__ in,
                                                                          const long long* __restrict__ sums,
                                                                          long long* __restrict__ out) {
  const long long n = n_ptr ? *n_ptr : n_host;
  long long v;
  const long long inc = ss_scan_apply(n, in, sums, &v);
  const long long i = (long long)blockIdx.x * SS_SCAN_BLOCK + threadIdx.x;
  if (i < n) out[i] = inc - v;
  if (i == n - 1) out[n] = inc;
  if (n == 0 && i == 0) out[0] = 0;
}
// inclusive, n outputs; the caller knows that an int holds every sum
template <typename In>
__global__ __launch_bounds__(SS_SCAN_BLOCK) void ss_scan_inclusive_kernel(long long n, const In* __restrict__ in,
                                                                          const long long* __restrict__ sums, int* __restrict__ out) {
  long long v;
  const long long inc = ss_scan_apply(n, in, sums, &v);
  const long long i = (long long)blockIdx.x * SS_SCAN_BLOCK + threadIdx.x;
  if (i < n) out[i] = (int)inc;
}
// in[0 .. n) -> out[0 .. n], n = *n_ptr <= n_bound when n_ptr is given, else n_bound; sums: ss_scan_sums_entries(n_bound)
template <typename W>
int ss_scan(hipStream_t st, long long n_bound, const W* n_ptr, const int* in, W* out, W* sums) {
  SS_IS_WORD(W);
  const unsigned nb = ss_grid(n_bound, SS_SCAN_BLOCK);
  hipLaunchKernelGGL(ss_scan_sums_kernel<int>, dim3(nb), dim3(SS_SCAN_BLOCK), 0, st, n_bound, (const long long*)n_ptr, in,
                     (long long*)sums);
  hipLaunchKernelGGL(ss_scan_exclusive_kernel, dim3(nb), dim3(SS_SCAN_BLOCK), 0, st, n_bound, (const long long*)n_ptr, in,
                     (const long long*)sums, (long long*)out);
  return (int)hipGetLastError();
}
// In = int or unsigned char (bit counts); n > 0; sums: ss_scan_sums_entries(n)
template <typename In, typename W>
int ss_scan_inclusive(hipStream_t st, long long n, const In* in, int* out, W* sums) {
  SS_IS_WORD(W);
  const unsigned nb = ss_grid(n, SS_SCAN_BLOCK);
  hipLaunchKernelGGL(ss_scan_sums_kernel<In>, dim3(nb), dim3(SS_SCAN_BLOCK), 0, st, n, (const long long*)nullptr, in,
                     (long long*)sums);
  hipLaunchKernelGGL(ss_scan_inclusive_kernel<In>, dim3(nb), dim3(SS_SCAN_BLOCK), 0, st, n, in, (const long long*)sums, out);
  return (int)hipGetLastError();
}

// ---- stable LSD radix sort of 64-bit keys, 8 bits a pass ----------------------------------------------------------------------
// Per pass a digit histogram per block of 2 048 keys, ONE exclusive scan over the (digit, block) counts and a scatter that ranks
// the keys of a block in their original order (wavefront by wavefront: the lanes sharing a digit are found with eight ballots,
// lower lanes first; wavefronts and rounds of 256 in order through LDS counters), so equal keys keep their order.
constexpr int SS_SORT_ITEMS = SS_SORT_BLOCK / 256;
__global__ __launch_bounds__(256) void ss_sort_hist_kernel(long long n, const unsigned long long* __restrict__ keys, int shift,
                                                           long long nblk, int* __restrict__ hist) {
  __shared__ int s_h[256];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * SS_SORT_BLOCK;
#pragma unroll
  for (int r = 0; r < SS_SORT_ITEMS; ++r) {
    const long long e = base + r * 256 + threadIdx.x;
    if (e < n) atomicAdd(&s_h[(int)((keys[e] >> shift) & 255u)], 1);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * nblk + blockIdx.x] = s_h[threadIdx.x];
}
// PAIRS: every key carries a value; otherwise vals / vals_out are never touched
template <bool PAIRS>
__global__ __launch_bounds__(256) void ss_sort_scatter_kernel(long long n, const unsigned long long* __restrict__ keys,
                                                              const long long* __restrict__ vals, int shift, long long nblk,
                                                              const long long* __restrict__ offs,
                                                              unsigned long long* __restrict__ keys_out,
                                                              long long* __restrict__ vals_out) {
  __shared__ long long s_run[256];
  __shared__ int s_wc[4][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  s_run[tid] = offs[(size_t)tid * nblk + blockIdx.x];
#pragma unroll
  for (int w = 0; w < 4; ++w) s_wc[w][tid] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * SS_SORT_BLOCK;
  for (int r = 0; r < SS_SORT_ITEMS; ++r) {
    const long long e = base + r * 256 + tid;
    const bool on = e < n;
    const unsigned long long key = on ? keys[e] : 0ull;
    long long val = 0;
    if (PAIRS) val = on ? vals[e] : 0;
    const int digit = (int)((key >> shift) & 255u);
    // the lanes of this wavefront that hold the same digit (and a key at all)
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
      // a prefix sum of the histogram of the same n keys, so in [0, n) -- unless the keys changed between the two kernels
      if ((unsigned long long)pos < (unsigned long long)n) {  // 0 <= pos < n in one compare
        keys_out[pos] = key;
        if (PAIRS) vals_out[pos] = val;
      }
    }
    __syncthreads();
    s_run[tid] += (s_wc[0][tid] + s_wc[1][tid]) + (s_wc[2][tid] + s_wc[3][tid]);
#pragma unroll
    for (int w = 0; w < 4; ++w) s_wc[w][tid] = 0;
    __syncthreads();
  }
}
// the sort's scratch: ss_sort_hist_entries(n) ints, ss_sort_offs_entries(n) and at least ss_sort_sums_entries(n) words
struct SsSortWs {
  int* hist;
  long long *offs, *sums;
};
template <typename W>
inline SsSortWs ss_sort_ws(int* hist, W* offs, W* sums) {
  SS_IS_WORD(W);
  return SsSortWs{hist, (long long*)offs, (long long*)sums};
}

// n > 0 keys (keys_in), with their values when vals_in != nullptr, sorted by the digits at `passes`, stable, INTO (keys_dst,
// vals_dst); (keys_tmp, vals_tmp) is the other side of the ping-pong, and the last pass lands in dst.  The input is only read, and
// only by the first pass, so it may be one of the two sides -- the one the first pass does not write: `in == dst, through tmp`
// sorts in place with an even number of passes.  The other one is refused.  No passes: a copy (nothing to do in place).
template <typename K, typename V>
int ss_sort(hipStream_t st, long long n, const SsPasses& passes, const K* keys_in, const V* vals_in, K* keys_tmp, V* vals_tmp,
            K* keys_dst, V* vals_dst, const SsSortWs& w) {
  SS_IS_WORD(K);
  SS_IS_WORD(V);
  const bool pairs = vals_in != nullptr;
  if (passes.count < 0 || passes.count > SS_MAX_PASSES) return (int)hipErrorInvalidValue;
  if (passes.count == 0) {
    if (keys_in != keys_dst) KAMD_CHECK(hipMemcpyAsync(keys_dst, keys_in, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    if (pairs && vals_in != vals_dst) KAMD_CHECK(hipMemcpyAsync(vals_dst, vals_in, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    return 0;
  }
  if (keys_in == ((passes.count & 1) ? keys_dst : keys_tmp)) return (int)hipErrorInvalidValue;  // the first pass would write it
  const long long nblk = ss_sort_blocks(n);
  const unsigned long long* src_k = (const unsigned long long*)keys_in;
  const long long* src_v = (const long long*)vals_in;
  for (int k = 0; k < passes.count; ++k) {
    const bool to_dst = ((passes.count - 1 - k) & 1) == 0;
    unsigned long long* dst_k = (unsigned long long*)(to_dst ? keys_dst : keys_tmp);
    long long* dst_v = (long long*)(to_dst ? vals_dst : vals_tmp);
    hipLaunchKernelGGL(ss_sort_hist_kernel, dim3((unsigned)nblk), dim3(256), 0, st, n, src_k, passes.shift[k], nblk, w.hist);
    KAMD_CHECK(ss_scan(st, 256 * nblk, (const long long*)nullptr, w.hist, w.offs, w.sums));
    if (pairs)
      hipLaunchKernelGGL(ss_sort_scatter_kernel<true>, dim3((unsigned)nblk), dim3(256), 0, st, n, src_k, src_v, passes.shift[k],
                         nblk, (const long long*)w.offs, dst_k, dst_v);
    else
      hipLaunchKernelGGL(ss_sort_scatter_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, st, n, src_k, src_v, passes.shift[k],
                         nblk, (const long long*)w.offs, dst_k, dst_v);
    src_k = dst_k;
    src_v = dst_v;
  }
  return (int)hipGetLastError();
}
// the keys alone
template <typename K>
int ss_sort(hipStream_t st, long long n, const SsPasses& passes, const K* keys_in, K* keys_tmp, K* keys_dst, const SsSortWs& w) {
  return ss_sort(st, n, passes, keys_in, (const long long*)nullptr, keys_tmp, (long long*)nullptr, keys_dst, (long long*)nullptr, w);
}

// ---- unique: the heads of the runs of equal keys of a sorted list, compared above `shift` ------------------------------------------
__global__ __launch_bounds__(256) void ss_heads_kernel(long long n_host, const long long* __restrict__ n_ptr,
                                                       const unsigned long long* __restrict__ keys, int shift,
                                                       int* __restrict__ flags) {
  const long long n = n_ptr ? *n_ptr : n_host;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) flags[i] = (i == 0 || (keys[i - 1] >> shift) != (keys[i] >> shift)) ? 1 : 0;
}
template <typename K, typename W>
int ss_heads(hipStream_t st, long long n_bound, const W* n_ptr, const K* keys, int shift, int* flags) {
  SS_IS_WORD(K);
  SS_IS_WORD(W);
  hipLaunchKernelGGL(ss_heads_kernel, dim3(ss_grid(n_bound, 256)), dim3(256), 0, st, n_bound, (const long long*)n_ptr,
                     (const unsigned long long*)keys, shift, flags);
  return (int)hipGetLastError();
}
// flags[i] = key i starts a run; pos = their exclusive scan: the rank of every run, pos[n] = the number of runs.  n as in ss_scan
template <typename K, typename W>
int ss_heads_scan(hipStream_t st, long long n_bound, const W* n_ptr, const K* keys, int shift, int* flags, W* pos, W* sums) {
  KAMD_CHECK(ss_heads(st, n_bound, n_ptr, keys, shift, flags));
  return ss_scan(st, n_bound, n_ptr, (const int*)flags, pos, sums);
}
// the plain compaction: the head of run r to uniq[r]
__global__ __launch_bounds__(256) void ss_unique_kernel(long long n, const unsigned long long* __restrict__ keys,
                                                        const int* __restrict__ flags, const long long* __restrict__ pos,
                                                        unsigned long long* __restrict__ uniq) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n && flags[i]) uniq[pos[i]] = keys[i];  // pos[i] < pos[n] <= n
}
// n > 0 sorted keys -> their unique keys in uniq and, after ONE host read (the stream is synchronised), their number
inline int ss_unique(hipStream_t st, long long n, const unsigned long long* keys, int* flags, long long* pos, long long* sums,
                     unsigned long long* uniq, int64_t* host_count) {
  KAMD_CHECK(ss_heads_scan(st, n, (const long long*)nullptr, keys, 0, flags, pos, sums));
  hipLaunchKernelGGL(ss_unique_kernel, dim3(ss_grid(n, 256)), dim3(256), 0, st, n, keys, (const int*)flags, (const long long*)pos,
                     uniq);
  KAMD_CHECK(hipGetLastError());
  long long h = 0;
  KAMD_CHECK(hipMemcpyAsync(&h, pos + n, 8, hipMemcpyDeviceToHost, st));
  KAMD_CHECK(hipStreamSynchronize(st));
  *host_count = h;
  return 0;
}

// first element >= key of the ascending uniq[0 .. nu): the rank of a key that is present
__device__ __forceinline__ long long ss_rank(const unsigned long long* __restrict__ uniq, long long nu, unsigned long long key) {
  long long lo = 0, hi = nu;
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
