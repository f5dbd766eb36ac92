// Training the Simplicits skinning network on the GPU: the value-and-tangent forward pass of skinning_mlp.hip with every layer's
// pre-activations kept, and the reverse pass through it: gradients of all parameters from the gradients of (weights, weights_jac).
// float32, W = 16 NB <= 64 (the width training uses), no bounding box: training applies the network to the points as they are
// (xn = x, extent 1), and no constant handle: weights (N, H - 1), weights_jac (N, H - 1, 3).
//
// FORWARD, SAVING (sb_forward_kernel).  The layer recurrence of skinning_mlp.hip in the same arithmetic order (bias first, one matrix
// instruction per 4 reduction indices, step (j, i) reducing over k in {16 j + 4 g + i}; ELU by expm1f / expf), on the same work split:
// a workgroup of 4 wavefronts strides over tiles of 64 points, a wavefront owns 16 points and four column blocks (value, x, y, z
// tangents), lane l = 16 g + p holds feature 16 j + 4 g + i of point p in register i of block j.  One LDS image of the next matrix in
// lane order (float4 number (jo NB + j) 64 + l = Wmat[16 jo + p][16 j + 4 g ..+ 3]), two barriers a layer.  After each of the L + 1
// activated layers the accumulators y, s_x, s_y, s_z go to the stash as they lie in the registers:
//   float4 number ((((layer tiles + tile) 4 + wave) NB + j) 4 + c) 64 + lane          (int64; c = 0: y, c = 1 + d: s_d)
// 16 bytes a lane, consecutive lanes on consecutive 16 bytes, (L + 1) 4 W floats a point, whole tiles allocated; the lanes past N of
// the last tile neither store nor load (they read zeros).
//
// BACKWARD (sb_backward_kernel), the same split, the layers in reverse.  With e = elu'(y) and e2 = (y > 0 ? 0 : exp y), from the
// gradients (abar, tbar_d) of a layer's activations (a, t_d):
//   ybar = abar e + e2 sum_d tbar_d s_d,   sbar_d = tbar_d e                                           (lane-local, from the stash)
//   abar' = Wmat^T ybar,  tbar'_d = Wmat^T sbar_d   on v_mfma_f32_16x16x4_f32: ybar's register i of block jo is, as it stands, the B
//           operand of the step that reduces over output features {16 jo + 4 g + i}; A is the TRANSPOSED matrix, staged in LDS in
//           lane order: float4 number (ji nbo + jo) 64 + l = {Wmat[16 jo + 4 g + i][16 ji + p] : i = 0..3} (a strided gather from
//           global memory, 64 contiguous bytes per 16 lanes; one ds_read_b128 per lane for four steps).
//   The last layer's (ybar, sbar_d) are the incoming gradients, read from global memory in the accumulator's layout; its rows are
//   walked in chunks of NB blocks, so the image never exceeds W^2 floats.  The first layer has the closed form
//   dW0[f][d] = sum_p (ybar_f xn_d + sbar_fd), db0[f] = sum_p ybar_f.
//
// PARAMETER GRADIENTS, through LDS inside the backward kernel.  dWmat = sum_p (ybar (x) a + sum_d sbar_d (x) t_d) reduces over
// points, which the accumulators hold in lane & 15 where the matrix instruction reduces over lane >> 4.  One stream c at a time
// (value, then each tangent), the 64 points of the tile are written feature-major with a row of 68 floats into two images, ybar_c
// (up to W rows) and a_c (W rows): both the store (bank 16 g + p) and the transposed read (bank 4 r + g) are free of conflicts.
// Block pair q = jo NB + ji belongs to wavefront q mod 4, which reduces all 64 points and all 4 streams in its own accumulator (16
// steps a stream, points 4 q' + g): no sum across wavefronts.  Thread t < rows sums row t of the ybar image for the bias.  The
// wavefront that owns an element adds it to the workgroup's partial image in the workspace (first tile: writes); a finishing launch
// sums the images of the workgroups in order.  No atomics, no host read: the same inputs give the same bits.  LDS: W^2 + 2 * 68 W +
// 192 floats, 52 KiB at W = 64.
#include "common.h"
#include "../../include/kaolin_amd.h"

namespace {

typedef float sb_f32x4 __attribute__((ext_vector_type(4)));

constexpr int SB_THREADS = 256;
constexpr int SB_TILE = 64;                     // points of a workgroup's tile
constexpr int SB_MAX_W = 64, SB_MAX_H = 128;
constexpr int SB_MAX_GROUPS = KAMD_NUM_CU / 2;   // = partial gradient images of the backward
constexpr int SB_LD = 68;                       // floats of a row of the transposed operand images

struct SbArgs {
  const float *pts, *params, *grad_w, *grad_j;
  float *weights, *jac, *stash, *partial;
  int64_t N, tiles, P;   // P: floats of the packed parameters
  int L, H, HB;          // hidden layers, handles (the network has H - 1 outputs), 16-row blocks of the last layer
};

__device__ __forceinline__ sb_f32x4 sb_zero() { return sb_f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }

// blocks [0, nbo) of 16 rows of a row-major (rows, 16 NB) matrix -> the image in lane order; rows past `rows` are zeros
template <int NB>
__device__ __forceinline__ void sb_stage(float* img, const float* __restrict__ src, int rows, int nbo, int t) {
  const int lane = t & 63;
  for (int q = t >> 6; q < nbo * NB; q += 4) {
    const int row = 16 * (q / NB) + (lane & 15), col = 16 * (q % NB) + 4 * (lane >> 4);
    sb_f32x4 v = sb_zero();
    if (row < rows) v = *(const sb_f32x4*)(src + (size_t)row * (16 * NB) + col);
    ((sb_f32x4*)img)[q * 64 + lane] = v;
  }
}
// the transposed image of rows [row0, row0 + 16 nbo) of the same matrix
template <int NB>
__device__ __forceinline__ void sb_stage_t(float* img, const float* __restrict__ src, int row0, int rows, int nbo, int t) {
  const int lane = t & 63, p = lane & 15, g = lane >> 4;
  for (int q = t >> 6; q < nbo * NB; q += 4) {
    const int ji = q / nbo, jo = q % nbo;
    sb_f32x4 v = sb_zero();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = row0 + 16 * jo + 4 * g + i;
      if (row < rows) v[i] = src[(size_t)row * (16 * NB) + 16 * ji + p];
    }
    ((sb_f32x4*)img)[q * 64 + lane] = v;
  }
}

__device__ __forceinline__ int64_t sb_stash_index(int layer, int64_t tiles, int64_t tile, int wave, int nb, int j, int c, int lane) {
  return (((((int64_t)layer * tiles + tile) * 4 + wave) * nb + j) * 4 + c) * 64 + lane;
}

// a = elu(y), t_d = elu'(y) s_d, lane-local
template <int NB>
__device__ __forceinline__ void sb_elu(sb_f32x4 (&act)[NB][4], const sb_f32x4 (&out)[NB][4]) {
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float y = out[j][0][i];
      const bool pos = y > 0.0f;
      const float d = pos ? 1.0f : expf(y);
      act[j][0][i] = pos ? y : expm1f(y);
#pragma unroll
      for (int c = 1; c < 4; ++c) act[j][c][i] = d * out[j][c][i];
    }
}

template <int NB>
__global__ __launch_bounds__(SB_THREADS) void sb_forward_kernel(const SbArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sb_lds[];
  constexpr int W = 16 * NB;
  float* first = sb_lds;            // 4 W floats: (w_f0, w_f1, w_f2, b_f)
  float* img = sb_lds + 4 * W;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4;
  const int H = a.H, L = a.L;
  const size_t hidden = (size_t)W * W + W;

  for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    // the previous tile's last barrier has passed: both images are free
    if (t < W) {
      const float* w0 = a.params + 3 * t;
      ((sb_f32x4*)first)[t] = sb_f32x4{w0[0], w0[1], w0[2], a.params[3 * W + t]};
    }
    const float* src = a.params + 4 * W;   // the layer whose matrix is in the image
    sb_stage<NB>(img, src, L > 0 ? W : H - 1, L > 0 ? NB : a.HB, t);
    const int64_t p = tile * SB_TILE + wave * 16 + (lane & 15);
    const bool valid = p < a.N;
    float xn[3] = {0.0f, 0.0f, 0.0f};
    if (valid) {
#pragma unroll
      for (int d = 0; d < 3; ++d) xn[d] = a.pts[p * 3 + d];
    }
    __syncthreads();
    sb_f32x4 act[NB][4], out[NB][4];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const sb_f32x4 w = ((const sb_f32x4*)first)[16 * j + 4 * g + i];
        out[j][0][i] = fmaf(w[2], xn[2], fmaf(w[1], xn[1], fmaf(w[0], xn[0], w[3])));
#pragma unroll
        for (int d = 0; d < 3; ++d) out[j][1 + d][i] = w[d];
      }
    for (int s = 0;; ++s) {
      if (valid) {
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
          for (int c = 0; c < 4; ++c) ((sb_f32x4*)a.stash)[sb_stash_index(s, a.tiles, tile, wave, NB, j, c, lane)] = out[j][c];
      }
      sb_elu<NB>(act, out);
      if (s == L) break;
      // hidden layer s + 1: its matrix is in the image, its bias follows the matrix
#pragma unroll
      for (int jo = 0; jo < NB; ++jo) {
        out[jo][0] = *(const sb_f32x4*)(src + (size_t)W * W + 16 * jo + 4 * g);
#pragma unroll
        for (int c = 1; c < 4; ++c) out[jo][c] = sb_zero();
      }
#pragma unroll
      for (int jo = 0; jo < NB; ++jo)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const sb_f32x4 w = ((const sb_f32x4*)img)[(jo * NB + j) * 64 + lane];
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) out[jo][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i], act[j][c][i], out[jo][c], 0, 0, 0);
        }
      __syncthreads();   // every wavefront has read the image
      src += hidden;
      const bool last_next = s + 1 == L;
      sb_stage<NB>(img, src, last_next ? H - 1 : W, last_next ? a.HB : NB, t);
      __syncthreads();
    }

    // the last layer, one block of 16 outputs at a time: src is its matrix, (H - 1, W), its bias follows
    const float* bl = src + (size_t)(H - 1) * W;
    for (int jo = 0; jo < a.HB; ++jo) {
      const int h0 = 16 * jo + 4 * g;
      sb_f32x4 acc[4] = {sb_zero(), sb_zero(), sb_zero(), sb_zero()};
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (h0 + i < H - 1) acc[0][i] = bl[h0 + i];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const sb_f32x4 w = ((const sb_f32x4*)img)[(jo * NB + j) * 64 + lane];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i], act[j][c][i], acc[c], 0, 0, 0);
      }
      if (valid) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (h0 + i < H - 1) {
            a.weights[p * (H - 1) + h0 + i] = acc[0][i];
#pragma unroll
            for (int d = 0; d < 3; ++d) a.jac[(p * (H - 1) + h0 + i) * 3 + d] = acc[1 + d][i];
          }
      }
    }
    __syncthreads();   // every wavefront has read the last image before the next tile stages
  }
}

// (y, s_d) of a stashed layer -> registers; zeros in the lanes past N
template <int NB>
__device__ __forceinline__ void sb_load_stash(sb_f32x4 (&out)[NB][4], const SbArgs& a, int layer, int64_t tile, int wave, int lane,
                                              bool valid) {
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      out[j][c] = valid ? ((const sb_f32x4*)a.stash)[sb_stash_index(layer, a.tiles, tile, wave, NB, j, c, lane)] : sb_zero();
}

// (abar, tbar_d) in `grad`, (y, s_d) in `st` -> (ybar, sbar_d) in `top`
template <int NB>
__device__ __forceinline__ void sb_elu_backward(sb_f32x4 (&top)[NB][4], const sb_f32x4 (&grad)[NB][4], const sb_f32x4 (&st)[NB][4]) {
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float y = st[j][0][i];
      const bool pos = y > 0.0f;
      const float ex = pos ? 0.0f : expf(y);
      const float e = pos ? 1.0f : ex;
      const float ts = fmaf(grad[j][3][i], st[j][3][i], fmaf(grad[j][2][i], st[j][2][i], grad[j][1][i] * st[j][1][i]));
      top[j][0][i] = fmaf(ex, ts, grad[j][0][i] * e);
#pragma unroll
      for (int c = 1; c < 4; ++c) top[j][c][i] = grad[j][c][i] * e;
    }
}

// One pass of the parameter gradient: rows [row0, row0 + 16 nbo) of a (rows, W) matrix and of its bias.  top(jo, c): the lane's
// four values of stream c, features row0 + 16 jo + 4 g + i of its point (zeros past `rows` and past N).
template <int NB, class Top>
__device__ __forceinline__ void sb_dw_pass(float* ldsA, float* ldsB, Top top, const sb_f32x4 (&bot)[NB][4], int nbo, int row0, int rows,
                                           float* __restrict__ dW, float* __restrict__ db, bool first, int t) {
  constexpr int W = 16 * NB, PAIRS = (NB * NB + 3) / 4;
  const int lane = t & 63, wave = t >> 6, g = lane >> 4, r = lane & 15;
  sb_f32x4 acc[PAIRS];
#pragma unroll
  for (int k = 0; k < PAIRS; ++k) acc[k] = sb_zero();
  float bsum = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    __syncthreads();   // the previous stream's readers are done
#pragma unroll
    for (int jo = 0; jo < NB; ++jo)
      if (jo < nbo) {
        const sb_f32x4 v = top(jo, c);
#pragma unroll
        for (int i = 0; i < 4; ++i) ldsA[(16 * jo + 4 * g + i) * SB_LD + 16 * wave + r] = v[i];
      }
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) ldsB[(16 * j + 4 * g + i) * SB_LD + 16 * wave + r] = bot[j][c][i];
    __syncthreads();
    if (c == 0 && t < 16 * nbo) {
      for (int q = 0; q < SB_TILE; ++q) bsum += ldsA[t * SB_LD + q];
    }
#pragma unroll
    for (int k = 0; k < PAIRS; ++k) {
      const int q = wave + 4 * k;
      if (q < nbo * NB) {
        const float* pa = ldsA + (16 * (q / NB) + r) * SB_LD + g;
        const float* pb = ldsB + (16 * (q % NB) + r) * SB_LD + g;
#pragma unroll
        for (int s = 0; s < SB_TILE / 4; ++s) acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[4 * s], pb[4 * s], acc[k], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < PAIRS; ++k) {
    const int q = wave + 4 * k;
    if (q < nbo * NB) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = row0 + 16 * (q / NB) + 4 * g + i;
        if (row < rows) {
          float* d = dW + (size_t)row * W + 16 * (q % NB) + r;
          *d = first ? acc[k][i] : *d + acc[k][i];
        }
      }
    }
  }
  if (t < 16 * nbo && row0 + t < rows) db[row0 + t] = first ? bsum : db[row0 + t] + bsum;
}

template <int NB>
__global__ __launch_bounds__(SB_THREADS) void sb_backward_kernel(const SbArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sb_lds[];
  constexpr int W = 16 * NB;
  float* img = sb_lds;                    // W^2 floats: a transposed matrix, or a chunk of the last one
  float* ldsA = img + W * W;              // W rows of SB_LD
  float* ldsB = ldsA + W * SB_LD;         // W rows of SB_LD
  float* lx = ldsB + W * SB_LD;           // 3 x 64: the tile's points, coordinate-major
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4, r = lane & 15;
  const int L = a.L, HP = a.H - 1;
  const size_t hidden = (size_t)W * W + W;
  float* part = a.partial + (size_t)blockIdx.x * a.P;

  for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const bool first = tile == blockIdx.x;
    const int64_t p = tile * SB_TILE + wave * 16 + r;
    const bool valid = p < a.N;
    if (g == 0) {
#pragma unroll
      for (int d = 0; d < 3; ++d) lx[d * SB_TILE + 16 * wave + r] = valid ? a.pts[p * 3 + d] : 0.0f;
    }
    sb_f32x4 grad[NB][4], top[NB][4], bot[NB][4], st[NB][4];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) grad[j][c] = sb_zero();
    sb_load_stash<NB>(st, a, L, tile, wave, lane, valid);
    sb_elu<NB>(bot, st);

    // the last layer: (ybar, sbar_d) are the incoming gradients; its rows in chunks of NB blocks
    {
      const size_t off = 4 * W + (size_t)L * hidden;
      const float* gw = a.grad_w;
      const float* gj = a.grad_j;
      for (int row0 = 0; row0 < HP; row0 += W) {
        const int nbo = (HP - row0 + 15) / 16 < NB ? (HP - row0 + 15) / 16 : NB;
        auto incoming = [&](int jo, int c) {
          sb_f32x4 v = sb_zero();
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int h = row0 + 16 * jo + 4 * g + i;
            if (valid && h < HP) v[i] = c == 0 ? gw[p * HP + h] : gj[(p * HP + h) * 3 + (c - 1)];
          }
          return v;
        };
        __syncthreads();   // the image's readers are done
        sb_stage_t<NB>(img, a.params + off, row0, HP, nbo, t);
        __syncthreads();
#pragma unroll
        for (int jo = 0; jo < NB; ++jo)
          if (jo < nbo) {
            sb_f32x4 gb[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) gb[c] = incoming(jo, c);
#pragma unroll
            for (int ji = 0; ji < NB; ++ji) {
              const sb_f32x4 w = ((const sb_f32x4*)img)[(ji * nbo + jo) * 64 + lane];
#pragma unroll
              for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 4; ++c) grad[ji][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i], gb[c][i], grad[ji][c], 0, 0, 0);
            }
          }
        sb_dw_pass<NB>(ldsA, ldsB, incoming, bot, nbo, row0, HP, part + off, part + off + (size_t)HP * W, first, t);
      }
    }

    for (int l = L; l >= 1; --l) {
      const size_t off = 4 * W + (size_t)(l - 1) * hidden;
      sb_load_stash<NB>(st, a, l, tile, wave, lane, valid);
      sb_elu_backward<NB>(top, grad, st);
      sb_load_stash<NB>(st, a, l - 1, tile, wave, lane, valid);
      sb_elu<NB>(bot, st);
      __syncthreads();   // the image's readers are done
      sb_stage_t<NB>(img, a.params + off, 0, W, NB, t);
      __syncthreads();
#pragma unroll
      for (int ji = 0; ji < NB; ++ji)
#pragma unroll
        for (int c = 0; c < 4; ++c) grad[ji][c] = sb_zero();
#pragma unroll
      for (int jo = 0; jo < NB; ++jo)
#pragma unroll
        for (int ji = 0; ji < NB; ++ji) {
          const sb_f32x4 w = ((const sb_f32x4*)img)[(ji * NB + jo) * 64 + lane];
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) grad[ji][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i], top[jo][c][i], grad[ji][c], 0, 0, 0);
        }
      sb_dw_pass<NB>(ldsA, ldsB, [&](int jo, int c) { return top[jo][c]; }, bot, NB, 0, W, part + off, part + off + (size_t)W * W,
                     first, t);
    }

    // the first layer: y = W0 xn + b0, s_d = W0[:, d]
    sb_load_stash<NB>(st, a, 0, tile, wave, lane, valid);
    sb_elu_backward<NB>(top, grad, st);
    float sums[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // db0[t], dW0[t][0..2]
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      __syncthreads();
#pragma unroll
      for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) ldsA[(16 * j + 4 * g + i) * SB_LD + 16 * wave + r] = top[j][c][i];
      __syncthreads();
      if (t < W) {
        for (int q = 0; q < SB_TILE; ++q) {
          const float v = ldsA[t * SB_LD + q];
          if (c == 0) {
            sums[0] += v;
#pragma unroll
            for (int d = 0; d < 3; ++d) sums[1 + d] = fmaf(v, lx[d * SB_TILE + q], sums[1 + d]);
          } else {
            sums[c] += v;
          }
        }
      }
    }
    if (t < W) {
#pragma unroll
      for (int d = 0; d < 3; ++d) part[3 * t + d] = first ? sums[1 + d] : part[3 * t + d] + sums[1 + d];
      part[3 * W + t] = first ? sums[0] : part[3 * W + t] + sums[0];
    }
    __syncthreads();   // lx and the images are free for the next tile
  }
}

// grad_params[e] = the partial images summed in the order of the workgroups
__global__ __launch_bounds__(256) void sb_finish_kernel(int64_t P, int groups, const float* __restrict__ partial,
                                                        float* __restrict__ grad_params) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < P; e += (int64_t)gridDim.x * 256) {
    float s = partial[e];
    for (int k = 1; k < groups; ++k) s += partial[(size_t)k * P + e];
    grad_params[e] = s;
  }
}

bool sb_sizes_ok(int64_t N, int width, int num_layers, int num_handles) {
  return N >= 1 && width >= 16 && width <= SB_MAX_W && width % 16 == 0 && num_layers >= 0 && num_handles >= 2 &&
         num_handles <= SB_MAX_H;
}
int64_t sb_tiles(int64_t N) { return (N + SB_TILE - 1) / SB_TILE; }
int64_t sb_param_floats(int width, int num_layers, int num_handles) {
  return 4 * (int64_t)width + (int64_t)num_layers * ((int64_t)width * width + width) + (int64_t)(num_handles - 1) * (width + 1);
}
unsigned sb_groups(int64_t N) { return (unsigned)(sb_tiles(N) < SB_MAX_GROUPS ? sb_tiles(N) : SB_MAX_GROUPS); }

template <int NB>
void sb_launch_forward(hipStream_t st, unsigned groups, size_t lds, const SbArgs& a) {
  hipLaunchKernelGGL(sb_forward_kernel<NB>, dim3(groups), dim3(SB_THREADS), lds, st, a);
}
template <int NB>
void sb_launch_backward(hipStream_t st, unsigned groups, size_t lds, const SbArgs& a) {
  hipLaunchKernelGGL(sb_backward_kernel<NB>, dim3(groups), dim3(SB_THREADS), lds, st, a);
}

}  // namespace

extern "C" {

int kamd_physics_skinning_train_max_groups(void) { return SB_MAX_GROUPS; }

size_t kamd_physics_skinning_stash_workspace(int64_t N, int width, int num_layers) {
  if (!sb_sizes_ok(N, width, num_layers, 2)) return 0;
  return (size_t)(num_layers + 1) * (size_t)sb_tiles(N) * SB_TILE * 4 * (size_t)width * sizeof(float);
}

size_t kamd_physics_skinning_backward_workspace(int64_t N, int width, int num_layers, int num_handles) {
  if (!sb_sizes_ok(N, width, num_layers, num_handles)) return 0;
  return (size_t)sb_groups(N) * (size_t)sb_param_floats(width, num_layers, num_handles) * sizeof(float);
}

int kamd_physics_skinning_forward_save_f32(void* stream, int64_t N, int width, int num_layers, int num_handles, const float* pts,
                                           const float* params, float* weights, float* weights_jac, float* stash) {
  if (!sb_sizes_ok(N, width, num_layers, num_handles)) return (int)hipErrorInvalidValue;
  if (pts == nullptr || params == nullptr || weights == nullptr || weights_jac == nullptr || stash == nullptr)
    return (int)hipErrorInvalidValue;
  SbArgs a = {};
  a.pts = pts, a.params = params, a.weights = weights, a.jac = weights_jac, a.stash = stash;
  a.N = N, a.tiles = sb_tiles(N), a.P = sb_param_floats(width, num_layers, num_handles);
  a.L = num_layers, a.H = num_handles, a.HB = (num_handles - 1 + 15) / 16;
  const int rows = 16 * a.HB > width ? 16 * a.HB : width;
  const size_t lds = ((size_t)4 * width + (size_t)rows * width) * sizeof(float);   // at most 33 KiB
  hipStream_t st = (hipStream_t)stream;
  switch (width / 16) {
    case 1: sb_launch_forward<1>(st, sb_groups(N), lds, a); break;
    case 2: sb_launch_forward<2>(st, sb_groups(N), lds, a); break;
    case 3: sb_launch_forward<3>(st, sb_groups(N), lds, a); break;
    default: sb_launch_forward<4>(st, sb_groups(N), lds, a); break;
  }
  KAMD_RETURN_LAST_ERROR();
}

int kamd_physics_skinning_backward_f32(void* stream, int64_t N, int width, int num_layers, int num_handles, const float* pts,
                                       const float* params, const float* stash, const float* grad_weights,
                                       const float* grad_weights_jac, float* grad_params, void* workspace, size_t workspace_bytes) {
  if (!sb_sizes_ok(N, width, num_layers, num_handles)) return (int)hipErrorInvalidValue;
  if (pts == nullptr || params == nullptr || stash == nullptr || grad_weights == nullptr || grad_weights_jac == nullptr ||
      grad_params == nullptr || workspace == nullptr ||
      workspace_bytes < kamd_physics_skinning_backward_workspace(N, width, num_layers, num_handles))
    return (int)hipErrorInvalidValue;
  SbArgs a = {};
  a.pts = pts, a.params = params, a.stash = const_cast<float*>(stash), a.grad_w = grad_weights, a.grad_j = grad_weights_jac;
  a.partial = (float*)workspace;
  a.N = N, a.tiles = sb_tiles(N), a.P = sb_param_floats(width, num_layers, num_handles);
  a.L = num_layers, a.H = num_handles, a.HB = (num_handles - 1 + 15) / 16;
  const size_t lds = ((size_t)width * width + 2 * (size_t)width * SB_LD + 3 * SB_TILE) * sizeof(float);   // at most 52 KiB
  const unsigned groups = sb_groups(N);
  hipStream_t st = (hipStream_t)stream;
  switch (width / 16) {
    case 1: sb_launch_backward<1>(st, groups, lds, a); break;
    case 2: sb_launch_backward<2>(st, groups, lds, a); break;
    case 3: sb_launch_backward<3>(st, groups, lds, a); break;
    default: sb_launch_backward<4>(st, groups, lds, a); break;
  }
  int64_t blocks = (a.P + 255) / 256;
  if (blocks > (int64_t)KAMD_NUM_CU * 4) blocks = (int64_t)KAMD_NUM_CU * 4;
  hipLaunchKernelGGL(sb_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a.P, (int)groups, (const float*)workspace, grad_params);
  KAMD_RETURN_LAST_ERROR();
}
}
