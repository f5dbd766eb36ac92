// The stage walker and the stable pair sort of the SPC voxelizers, with the primitive's voxel test as a template parameter.
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

// ---- stable LSD radix sort of (Morton code, primitive) pairs by code, 8 bits a pass ---------------------------------------------
// Per pass a digit histogram per block of 2 048 pairs, ONE exclusive scan over the (digit, block) counts (ms_scan) and a scatter
// that ranks the pairs of a block in their original order (wavefront by wavefront: the lanes sharing a digit are found with eight
// ballots, lower lanes first; wavefronts and rounds of 256 in order through LDS counters), so equal codes keep their order.  Every
// destination is a prefix sum of the histogram of the same n keys, so it lies in [0, n).
constexpr int SPC_SORT_ITEMS = 8, SPC_SORT_BLOCK = 256 * SPC_SORT_ITEMS;
__global__ __launch_bounds__(256) void spc_sort_hist_kernel(int64_t n, const uint64_t* __restrict__ keys, int shift, int nblk,
                                                            int* __restrict__ hist) {
  __shared__ int s_h[256];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * SPC_SORT_BLOCK;
#pragma unroll
  for (int r = 0; r < SPC_SORT_ITEMS; ++r) {
    const int64_t e = base + r * 256 + threadIdx.x;
    if (e < n) atomicAdd(&s_h[(int)((keys[e] >> shift) & 255u)], 1);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * nblk + blockIdx.x] = s_h[threadIdx.x];
}
__global__ __launch_bounds__(256) void spc_sort_scatter_kernel(int64_t n, const uint64_t* __restrict__ keys,
                                                               const int64_t* __restrict__ vals, int shift, int nblk,
                                                               const int64_t* __restrict__ offs, uint64_t* __restrict__ keys_out,
                                                               int64_t* __restrict__ vals_out) {
  __shared__ long long s_run[256];
  __shared__ int s_wc[4][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  s_run[tid] = offs[(size_t)tid * nblk + blockIdx.x];
#pragma unroll
  for (int w = 0; w < 4; ++w) s_wc[w][tid] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * SPC_SORT_BLOCK;
  for (int r = 0; r < SPC_SORT_ITEMS; ++r) {
    const int64_t e = base + r * 256 + tid;
    const bool on = e < n;
    const uint64_t key = on ? keys[e] : 0ull;
    const int64_t val = on ? vals[e] : 0;
    const int digit = (int)((key >> shift) & 255u);
    // the lanes of this wavefront that hold the same digit (and a pair at all)
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
      if (pos >= 0 && pos < n) {
        keys_out[pos] = key;
        vals_out[pos] = val;
      }
    }
    __syncthreads();
    s_run[tid] += (s_wc[0][tid] + s_wc[1][tid]) + (s_wc[2][tid] + s_wc[3][tid]);
#pragma unroll
    for (int w = 0; w < 4; ++w) s_wc[w][tid] = 0;
    __syncthreads();
  }
}
inline int spc_sort_blocks(int64_t n) { return (int)(((n > 0 ? n : 1) + SPC_SORT_BLOCK - 1) / SPC_SORT_BLOCK); }

// the sort's scratch for n pairs: (digit, block) counts (ints), their offsets (+ 1) and the scan's block sums
struct SpcSortWs {
  int* hist;
  int64_t *offs, *sums;
};
inline size_t spc_sort_hist_entries(int64_t n) { return (size_t)256 * (size_t)spc_sort_blocks(n); }

// n pairs (keys_in, vals_in) -> sorted by the low `bits` key bits, stable, into (keys_dst, vals_dst); (keys_tmp, vals_tmp) is the
// other side of the ping-pong.  The inputs are only read.  bits == 0: a copy.
inline int spc_sort_pairs(hipStream_t st, int64_t n, int bits, const uint64_t* keys_in, const int64_t* vals_in, uint64_t* keys_tmp,
                          int64_t* vals_tmp, uint64_t* keys_dst, int64_t* vals_dst, const SpcSortWs& w) {
  const int passes = (bits + 7) / 8;
  const int nblk = spc_sort_blocks(n);
  if (passes == 0) {
    unsigned cg = (unsigned)kamd_cdiv(n, 256);
    if (cg > (unsigned)KAMD_NUM_CU * 8u) cg = (unsigned)KAMD_NUM_CU * 8u;
    hipLaunchKernelGGL(ms_copy_words_kernel, dim3(cg), dim3(256), 0, st, n, (const int64_t*)keys_in, (int64_t*)keys_dst, vals_in,
                       vals_dst);
    return (int)hipGetLastError();
  }
  const uint64_t* src_k = keys_in;
  const int64_t* src_v = vals_in;
  for (int k = 0; k < passes; ++k) {  // the last pass lands in dst
    const bool to_dst = ((passes - 1 - k) & 1) == 0;
    uint64_t* dst_k = to_dst ? keys_dst : keys_tmp;
    int64_t* dst_v = to_dst ? vals_dst : vals_tmp;
    hipLaunchKernelGGL(spc_sort_hist_kernel, dim3(nblk), dim3(256), 0, st, n, src_k, 8 * k, nblk, w.hist);
    KAMD_CHECK(ms_scan(st, (int64_t)256 * nblk, nullptr, w.hist, w.offs, w.sums));
    hipLaunchKernelGGL(spc_sort_scatter_kernel, dim3(nblk), dim3(256), 0, st, n, src_k, src_v, 8 * k, nblk,
                       (const int64_t*)w.offs, dst_k, dst_v);
    src_k = dst_k;
    src_v = dst_v;
  }
  return (int)hipGetLastError();
}

}  // namespace
