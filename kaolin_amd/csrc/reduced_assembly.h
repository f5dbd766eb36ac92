// What the three reduced (Simplicits) energies of kaolin.physics share: physics.hip (the Neo-Hookean material), collisions.hip (the
// contact terms) and scene_forces.hip (gravity, floor, pins, inertia) each reduce per-row terms to the W = 4 H degrees of freedom
// of one axis, K[(h,b,n),(h',b',n')] = K_bb'[4 h + n][4 h' + n'], in the same way:
//   * grid (slice of rows, 64 x 64 tile of W x W), RA_THREADS threads; a workgroup walks its slice in chunks, each staged into LDS
//     images of stride RA_LS, and accumulates by v_mfma_f32_16x16x4_f32: wavefront w owns rows 16 w ... 16 w + 15 of the tile and
//     four 16-column blocks (ra_store_blocks is the way back from that register layout)
//   * g is summed by the workgroups of column tile 0, thread = (b, column): a chunk's rows pairwise (ra_pairwise), the chunks by a
//     compensated sum (ra_add).  A sequential chain of that many terms missed the tests' bound, so no caller may use one
//   * E is summed by the workgroup of tile (0, 0): compensated in the rows' leading lanes, then over them (ra_slice_energy)
//   * every slice stores ONE partial of K, g and E (RaPartials, sized and carved by ra_workspace); ra_finish_kernel adds the slices
//     in index order, mirrors (entry (i, j) and entry (j, i) read the same partials: K is symmetric to the bit) and scatters to
//     row 12 h + 4 b + n.  No atomics, no host read: the same bits on every call, capturable
//   * slices: min(most, ceil(RA_TARGET_GROUPS / tiles)) of them, ra_slice_len rows each: a multiple of the chunk, at least four
//   * H <= RA_MAX_H: the callers keep 12 H floats (z) in statically allocated LDS
// and, for the per-row term kernels: a grid of at most RA_TERM_BLOCKS workgroups, one energy partial each (ra_block_energy), added
// in index order by one thread (ra_sum_kernel).
// Each file keeps what differs: the per-row terms, how a chunk's rows are gathered and its LDS images built, the MFMA loop (its
// depth, whether the A operand is scaled in the register, a staged product), and which blocks (b, b') it computes (the Ra* layouts).
// Every name lives in an unnamed namespace: each translation unit gets its own copy, compiled with that file's flags.
#pragma once
#include "common.h"

namespace {

typedef float ra_f32x4 __attribute__((ext_vector_type(4)));

constexpr int RA_THREADS = 256;
constexpr int RA_TILE = 64;
constexpr int RA_LS = RA_TILE + 16;            // LDS row stride: lanes l and l + 16 read rows 80 dwords apart -> other banks
constexpr int RA_MAX_H = 128;
constexpr int RA_TARGET_GROUPS = 512;          // slices x tiles aimed at: two workgroups per CU
constexpr int RA_TERM_BLOCKS = 1024;           // most workgroups (= energy partials) of a per-row term kernel

// ---- sums -----------------------------------------------------------------------------------------------------------------------------
// sum += v with the rounding error of every earlier step carried in `comp` (Kahan; nothing here may be reassociated)
__device__ __forceinline__ void ra_add(float& sum, float& comp, float v) {
  const float y = v - comp, t = sum + y;
  comp = (t - sum) - y;
  sum = t;
}
__device__ __forceinline__ float ra_wave_sum(float v) {
#pragma unroll
  for (int m = 1; m < KAMD_WAVE; m <<= 1) v = v + __shfl_xor(v, m);
  return v;
}
// v[0 .. N) added pairwise: neighbours, then neighbours of the sums, ...
template <int N>
__device__ __forceinline__ float ra_pairwise(float (&v)[N]) {
#pragma unroll
  for (int w = 1; w < N; w <<= 1)
#pragma unroll
    for (int q = 0; q < N; q += 2 * w) v[q] = v[q] + v[q + w];
  return v[0];
}
// out[blockIdx.x] = the energy of a workgroup of RA_THREADS threads: wavefront butterfly -> LDS -> the four in this order
__device__ __forceinline__ void ra_block_energy(float e, float* out) {
  __shared__ float s_w[RA_THREADS / KAMD_WAVE];
  e = ra_wave_sum(e);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = e;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}
// out[0] = the partials added in index order
__global__ __launch_bounds__(KAMD_WAVE) void ra_sum_kernel(int n, const float* __restrict__ partial, float* __restrict__ out) {
  if (threadIdx.x != 0) return;
  float sum = 0.0f, comp = 0.0f;
  for (int k = 0; k < n; ++k) ra_add(sum, comp, partial[k]);
  out[0] = sum;
}
// the grid of a term kernel over n rows, `threads` a workgroup
inline int ra_term_blocks(int64_t n, int threads) {
  const int64_t blocks = (n + threads - 1) / threads;
  return (int)(blocks < RA_TERM_BLOCKS ? blocks : RA_TERM_BLOCKS);
}

// ---- pieces of the reduced kernels ------------------------------------------------------------------------------------------------------
struct RaPartials {
  float *Kp, *gp, *ep;   // (slice, blocks, W, W), (slice, 3, W), (slice)
};

// tile y of the lower triangle, row by row: tj <= ti
__device__ __forceinline__ void ra_lower_tile(int y, int& ti, int& tj) {
  ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= y) ++ti;
  tj = y - ti * (ti + 1) / 2;
}
// the accumulators of NB blocks -> the slice's part of Kp (slice, NB, W, W); of a diagonal tile only the 16 x 16 blocks on and under the
// diagonal.  (physics.hip skips whole blocks above the diagonal and keeps its own loop.)
template <int NB>
__device__ __forceinline__ void ra_store_blocks(const ra_f32x4 (&acc)[NB][4], float* Kp, int64_t slice, int W, int i0, int j0, int wave,
                                                int lane, bool diag) {
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    float* P = Kp + ((size_t)slice * NB + b) * (size_t)W * W;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
      if (!diag || cb <= wave) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = i0 + wave * 16 + (lane >> 4) * 4 + j, col = j0 + cb * 16 + (lane & 15);
          if (row < W && col < W) P[(size_t)row * W + col] = acc[b][cb][j];
        }
      }
  }
}
// *out = the slice's energy: the LEADERS lanes that carry one (each in a slot of its own) -> s_e -> thread 0, compensated
template <int LEADERS>
__device__ __forceinline__ void ra_slice_energy(float e_acc, bool leader, int slot, float* s_e, float* out) {
  __syncthreads();
  if (leader) s_e[slot] = e_acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float sum = 0.0f, comp = 0.0f;
    for (int q = 0; q < LEADERS; ++q) ra_add(sum, comp, s_e[q]);
    *out = sum;
  }
}

// ---- finish ---------------------------------------------------------------------------------------------------------------------------
// Which blocks K_bb' a slice's partial holds.  block() maps an entry (i, j) of K_bb' to the partial block that holds it, moving
// (i, j) to the stored side of the diagonal; -1: the entry is an exact zero.
struct RaSymmetricSix {   // K_b'b = K_bb'^T: the pairs b' <= b, of b == b' the lower triangle
  static constexpr int BLOCKS = 6;
  static __device__ __forceinline__ int block(int b, int bp, int64_t& i, int64_t& j) {
    if (b < bp || (b == bp && i < j)) {
      const int sb = b;
      const int64_t si = i;
      b = bp, bp = sb, i = j, j = si;
    }
    return b * (b + 1) / 2 + bp;
  }
};
struct RaFullNine {   // all (b, b'), each symmetric in itself: the lower triangle of every block
  static constexpr int BLOCKS = 9;
  static __device__ __forceinline__ int block(int b, int bp, int64_t& i, int64_t& j) {
    if (i < j) {
      const int64_t si = i;
      i = j, j = si;
    }
    return b * 3 + bp;
  }
};
struct RaDiagonalThree {   // the axes do not couple: b == b' only
  static constexpr int BLOCKS = 3;
  static __device__ __forceinline__ int block(int b, int bp, int64_t& i, int64_t& j) {
    if (b != bp) return -1;
    if (i < j) {
      const int64_t si = i;
      i = j, j = si;
    }
    return b;
  }
};

// the slices' partials added in index order -> K (D, D) (nullptr: none), g (D), E (1); D = 12 H, row = 12 h + 4 b + n
template <class LAYOUT>
__global__ __launch_bounds__(RA_THREADS) void ra_finish_kernel(int slices, int H, const float* __restrict__ Kp,
                                                               const float* __restrict__ gp, const float* __restrict__ ep,
                                                               float* __restrict__ K, float* __restrict__ g, float* __restrict__ E) {
  const int64_t D = 12 * (int64_t)H, W = 4 * (int64_t)H;
  const int64_t nK = K != nullptr ? D * D : 0, total = nK + D + 1;
  for (int64_t e = (int64_t)blockIdx.x * RA_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * RA_THREADS) {
    const float* src;
    int64_t step;
    if (e < nK) {
      const int64_t r = e / D, c = e - r * D;
      int64_t i = (r / 12) * 4 + (r & 3), j = (c / 12) * 4 + (c & 3);
      const int block = LAYOUT::block((int)(r % 12) / 4, (int)(c % 12) / 4, i, j);
      if (block < 0) {
        K[e] = 0.0f;
        continue;
      }
      src = Kp + ((size_t)block * W + i) * W + j;
      step = LAYOUT::BLOCKS * W * W;
    } else if (e < nK + D) {
      const int64_t r = e - nK;
      src = gp + ((r % 12) / 4) * W + (r / 12) * 4 + (r & 3);
      step = 3 * W;
    } else {
      src = ep;
      step = 1;
    }
    float sum = src[0];
    for (int s = 1; s < slices; ++s) sum = sum + src[(size_t)s * step];
    if (e < nK)
      K[e] = sum;
    else if (e < nK + D)
      g[e - nK] = sum;
    else
      E[0] = sum;
  }
}
template <class LAYOUT>
inline int ra_finish(hipStream_t st, size_t slices, int H, const RaPartials& p, float* K, float* g, float* E) {
  const int64_t D = 12 * (int64_t)H, total = (K != nullptr ? D * D : 0) + D + 1;
  int64_t blocks = (total + RA_THREADS - 1) / RA_THREADS;
  if (blocks > (int64_t)KAMD_NUM_CU * 16) blocks = (int64_t)KAMD_NUM_CU * 16;
  hipLaunchKernelGGL(ra_finish_kernel<LAYOUT>, dim3((unsigned)blocks), dim3(RA_THREADS), 0, st, (int)slices, H, (const float*)p.Kp,
                     (const float*)p.gp, (const float*)p.ep, K, g, E);
  KAMD_RETURN_LAST_ERROR();
}

// ---- host sizing ----------------------------------------------------------------------------------------------------------------------
inline int ra_tiles(int H) { return (4 * H + RA_TILE - 1) / RA_TILE; }
inline int ra_tri(int T) { return T * (T + 1) / 2; }
inline bool ra_sizes_ok(int64_t count, int H) { return count >= 0 && count <= 0x7FFFFFFFLL && H >= 1 && H <= RA_MAX_H; }
// rows per slice when `tiles` workgroups share a slice, the kernel walks chunks of `chunk` rows and takes at most `most` slices
inline int64_t ra_slice_len(int64_t count, int tiles, int chunk, int most) {
  int64_t slices = (RA_TARGET_GROUPS + tiles - 1) / tiles;
  if (slices > most) slices = most;
  const int64_t per = ((count + slices - 1) / slices + chunk - 1) / chunk * chunk;
  return per < 4 * chunk ? 4 * chunk : per;
}
inline size_t ra_slices(int64_t count, int64_t per) { return (size_t)((count + per - 1) / per); }
// the bytes of S slices' partials of `blocks` blocks each (K's only with `hessian`); given a workspace, its carve-up too
inline size_t ra_workspace(size_t S, int blocks, int H, int hessian, void* workspace = nullptr, RaPartials* out = nullptr) {
  const size_t W = 4 * (size_t)H;
  const size_t kb = hessian ? kamd_align16(S * blocks * W * W * sizeof(float)) : 0, gb = kamd_align16(S * 3 * W * sizeof(float));
  if (out != nullptr) {
    char* ws = (char*)workspace;
    out->Kp = hessian ? (float*)ws : nullptr, out->gp = (float*)(ws + kb), out->ep = (float*)(ws + kb + gb);
  }
  return kb + gb + kamd_align16(S * sizeof(float));
}

}  // namespace
