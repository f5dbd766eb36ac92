// The Simplicits skinning network on the GPU: skinning weights and their spatial Jacobian of every point in ONE launch.  The reference
// evaluates the network twice (kaolin/physics/simplicits/network.py: forward, then torch.vmap(torch.func.jacrev(...)), H - 1 reverse
// sweeps with every activation in memory); this is one forward pass that carries the three tangents next to the value.  float32 only.
//
// THE NETWORK.  Linear(3, W), ELU, (Linear(W, W), ELU) x L, Linear(W, H - 1), on xn = (x - bb_min) / (bb_max - bb_min); a constant
// handle is appended: weights[p][H - 1] = 1, weights_jac[p][H - 1][:] = 0.  `params` is every Linear in order, row-major weight then
// bias: 4 W floats, then L times W^2 + W, then (H - 1) W + (H - 1).  W is a multiple of 16, so every weight row starts on 64 bytes.
//
// ARITHMETIC (-ffp-contract=off: every fused multiply-add is spelled; no packed float32 instructions):
//   ext_d = bb_max_d - bb_min_d,  xn_d = (x_d - bb_min_d) / ext_d                             (correctly rounded division)
//   first layer  y_f = fma(w_f2, xn_2, fma(w_f1, xn_1, fma(w_f0, xn_0, b_f)))  (bias first),  s_fd = w_fd / ext_d
//   ELU          a = y > 0 ? y : expm1f(y),   t_d = (y > 0 ? 1 : expf(y)) * s_d               (two library calls, each to its own ulp bound)
//   other layers y_f = b_f + sum_k w_fk a_k, s_fd = sum_k w_fk t_kd on v_mfma_f32_16x16x4_f32 (exact float32 products): the bias is
//                the accumulator's first value, then one matrix instruction per 4 reduction indices, which adds its 4 products to
//                the accumulator.  Step (j, i), j = 0 .. W/16 - 1 outer, i = 0 .. 3 inner, reduces over k in {16 j + 4 g + i : g = 0..3}.
//   The last layer has no ELU: weights[p][h] = y_h, weights_jac[p][h][d] = s_hd.
//   No workspace, no atomics, no host read: the same bits on every call, and capturable.
//
// WORK SPLIT.  A workgroup is 4 wavefronts and strides over tiles of 64 points; a wavefront owns 16 points.  The transposed product
// Y^T (features x columns) = Wmat (W_out x W_in) X^T (W_in x columns) has four 16-column blocks per wavefront: the value and the x, y, z
// tangents of the same 16 points.  In the 16x16x4 layout lane l = 16 g + p holds A[row p][k = g], B[k = g][column p] and
// D[row 4 g + i][column p] in register i, so register i of the accumulator block of output features 16 j .. 16 j + 15 holds feature
// 16 j + 4 g + i of point p: element (feature, point) of the value and of its three tangents sit in one lane and one register index of
// four blocks (the ELU coupling is lane-local), and that register is, as it stands, the B operand of the next layer's step (j, i)
// above.  The next layer walks its reduction in that order and takes the matching columns of its matrix as A: activations never leave
// the registers (W in, W out).
//
// WEIGHTS IN LDS, in the order the lanes read them: for output block jo and input block j, lane l needs Wmat[16 jo + p][16 j + 4 g + i],
// i = 0..3: 16 contiguous bytes of global memory.  The image holds them as float4 number (jo W/16 + j) 64 + l, so staging is one
// 16-byte global load and one 16-byte LDS store per lane, and the multiply reads one ds_read_b128 per lane for FOUR steps, consecutive
// lanes on consecutive 16 bytes: free of bank conflicts by construction, whatever the bank count, with no padding.  (A row-major image
// needs a padded stride s with {p s + 4 g} distinct modulo the banks and one 4-byte read per step; this takes a quarter of the reads.)
// Image: max(W, 16 ceil((H - 1) / 16)) W floats; the first layer's is 4 W floats, (w_f0, w_f1, w_f2, b_f) per feature.
// W <= 64: two images, the next layer's matrix is loaded into registers before this layer multiplies and stored into the other image
// after it: one barrier a layer.  W > 64: one image (64 KiB at W = 128), the store waits behind a second barrier.  Biases of hidden
// layers travel with the same prefetch, in registers.  Rows past H - 1 of the last layer are zeros in LDS and are not stored.
#include "common.h"
#include "../../include/kaolin_amd.h"

namespace {

typedef float sk_f32x4 __attribute__((ext_vector_type(4)));

constexpr int SK_THREADS = 256;
constexpr int SK_TILE = 64;                    // points of a workgroup's tile
constexpr int SK_MAX_W = 128, SK_MAX_H = 128;
constexpr int SK_MAX_GROUPS = 2 * KAMD_NUM_CU;  // two workgroups a CU are resident at W = 64 (registers)

struct SkArgs {
  const float *pts, *bb_min, *bb_max, *params;
  float *weights, *jac;
  int64_t N, tiles;
  int L, H, HB;      // hidden layers, handles, 16-row blocks of the last layer
  int image;         // floats of one LDS image
};

__device__ __forceinline__ sk_f32x4 sk_zero() { return sk_f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }

// rows [0, rows) of a row-major (rows, 16 NB) matrix -> registers, in image order: fragment q = jo NB + j of wavefront `wave` is
// pre[(q - wave) / 4]; rows past `rows` are zeros
template <int NB>
__device__ __forceinline__ void sk_prefetch(sk_f32x4 (&pre)[2 * NB], const float* __restrict__ src, int rows, int nq, int wave,
                                            int lane) {
#pragma unroll
  for (int k = 0; k < 2 * NB; ++k) {
    const int q = wave + 4 * k;
    pre[k] = sk_zero();
    if (q < nq) {
      const int row = 16 * (q / NB) + (lane & 15), col = 16 * (q % NB) + 4 * (lane >> 4);
      if (row < rows) pre[k] = *(const sk_f32x4*)(src + (size_t)row * (16 * NB) + col);
    }
  }
}
template <int NB>
__device__ __forceinline__ void sk_store_image(const sk_f32x4 (&pre)[2 * NB], float* img, int nq, int wave, int lane) {
#pragma unroll
  for (int k = 0; k < 2 * NB; ++k) {
    const int q = wave + 4 * k;
    if (q < nq) ((sk_f32x4*)img)[q * 64 + lane] = pre[k];
  }
}
// a = elu(y), t_d = elu'(y) s_d, lane-local; out -> act
template <int NB>
__device__ __forceinline__ void sk_elu(sk_f32x4 (&act)[NB][4], const sk_f32x4 (&out)[NB][4]) {
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
__global__ __launch_bounds__(SK_THREADS) void sk_mlp_kernel(const SkArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sk_lds[];
  constexpr int W = 16 * NB;
  constexpr bool TWO = NB <= 4;   // two images
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4;
  const int H = a.H, L = a.L;
  const size_t hidden = (size_t)W * W + W;
  float ext[3], lo[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) lo[d] = a.bb_min[d], ext[d] = a.bb_max[d] - lo[d];

  for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    // the previous tile's last barrier has passed: image 0 is free
    if (t < W) {
      const float* w0 = a.params + 3 * t;
      ((sk_f32x4*)sk_lds)[t] = sk_f32x4{w0[0], w0[1], w0[2], a.params[3 * W + t]};
    }
    const int64_t p = tile * SK_TILE + wave * 16 + (lane & 15);
    const bool valid = p < a.N;
    float xn[3] = {0.0f, 0.0f, 0.0f};
    if (valid) {
#pragma unroll
      for (int d = 0; d < 3; ++d) xn[d] = (a.pts[p * 3 + d] - lo[d]) / ext[d];
    }
    // stage 1 (a hidden layer, or the last one) on its way while the first layer runs
    sk_f32x4 pre[2 * NB], bias[NB];
    const float* src = a.params + 4 * W;
    int nq = (L > 0 ? NB : a.HB) * NB;
    sk_prefetch<NB>(pre, src, L > 0 ? W : H - 1, nq, wave, lane);
    if (L > 0) {
#pragma unroll
      for (int j = 0; j < NB; ++j) bias[j] = *(const sk_f32x4*)(src + (size_t)W * W + 16 * j + 4 * g);
    }
    __syncthreads();
    sk_f32x4 act[NB][4], out[NB][4];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const sk_f32x4 w = ((const sk_f32x4*)sk_lds)[16 * j + 4 * g + i];
        out[j][0][i] = fmaf(w[2], xn[2], fmaf(w[1], xn[1], fmaf(w[0], xn[0], w[3])));
#pragma unroll
        for (int d = 0; d < 3; ++d) out[j][1 + d][i] = w[d] / ext[d];
      }
    sk_elu<NB>(act, out);
    int cur = 0;   // the image read last
    if (!TWO) __syncthreads();
    cur = TWO ? 1 : 0;
    sk_store_image<NB>(pre, sk_lds + cur * a.image, nq, wave, lane);
    __syncthreads();

    for (int s = 1; s <= L; ++s) {
      const sk_f32x4* img = (const sk_f32x4*)(sk_lds + cur * a.image);
#pragma unroll
      for (int jo = 0; jo < NB; ++jo) {
        out[jo][0] = bias[jo];
#pragma unroll
        for (int c = 1; c < 4; ++c) out[jo][c] = sk_zero();
      }
      src += hidden;
      const bool last_next = s == L;
      nq = (last_next ? a.HB : NB) * NB;
      sk_prefetch<NB>(pre, src, last_next ? H - 1 : W, nq, wave, lane);
      if (!last_next) {
#pragma unroll
        for (int j = 0; j < NB; ++j) bias[j] = *(const sk_f32x4*)(src + (size_t)W * W + 16 * j + 4 * g);
      }
#pragma unroll
      for (int jo = 0; jo < NB; ++jo)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const sk_f32x4 w = img[(jo * NB + j) * 64 + lane];
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) out[jo][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i], act[j][c][i], out[jo][c], 0, 0, 0);
        }
      sk_elu<NB>(act, out);
      if (!TWO) __syncthreads();
      cur = TWO ? cur ^ 1 : 0;
      sk_store_image<NB>(pre, sk_lds + cur * a.image, nq, wave, lane);
      __syncthreads();
    }

    // the last layer, one block of 16 handles at a time: src is its matrix, (H - 1, W), its bias follows
    const sk_f32x4* img = (const sk_f32x4*)(sk_lds + cur * a.image);
    const float* bl = src + (size_t)(H - 1) * W;
    float* wp = a.weights + p * H;
    float* jp = a.jac + p * H * 3;
    for (int jo = 0; jo < a.HB; ++jo) {
      const int h0 = 16 * jo + 4 * g;
      sk_f32x4 acc[4] = {sk_zero(), sk_zero(), sk_zero(), sk_zero()};
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (h0 + i < H - 1) acc[0][i] = bl[h0 + i];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const sk_f32x4 w = img[(jo * NB + j) * 64 + lane];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i], act[j][c][i], acc[c], 0, 0, 0);
      }
      // the lane's 4 handles are 4 and 12 consecutive floats; the 4 lane groups of a point cover 64 and 192 consecutive bytes
      if (valid) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (h0 + i < H - 1) {
            wp[h0 + i] = acc[0][i];
#pragma unroll
            for (int d = 0; d < 3; ++d) jp[(h0 + i) * 3 + d] = acc[1 + d][i];
          }
      }
    }
    if (valid && g == 0) {   // the constant handle
      wp[H - 1] = 1.0f;
#pragma unroll
      for (int d = 0; d < 3; ++d) jp[(H - 1) * 3 + d] = 0.0f;
    }
    __syncthreads();   // every wavefront has read the last image before the next tile stages
  }
}

// the two activation functions alone (kamd_debug_skinning_elu)
__global__ __launch_bounds__(256) void sk_elu_probe_kernel(int64_t n, const float* __restrict__ y, float* __restrict__ elu,
                                                           float* __restrict__ delu) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const bool pos = y[e] > 0.0f;
    elu[e] = pos ? y[e] : expm1f(y[e]);
    delu[e] = pos ? 1.0f : expf(y[e]);
  }
}

template <int NB>
void sk_launch(hipStream_t st, unsigned groups, size_t lds, const SkArgs& a) {
  hipLaunchKernelGGL(sk_mlp_kernel<NB>, dim3(groups), dim3(SK_THREADS), lds, st, a);
}

}  // namespace

extern "C" {

int kamd_physics_skinning_max_groups(void) { return SK_MAX_GROUPS; }

int kamd_physics_skinning_mlp_f32(void* stream, int64_t N, int width, int num_layers, int num_handles, const float* pts,
                                  const float* bb_min, const float* bb_max, const float* params, float* weights, float* weights_jac) {
  if (N < 1 || width < 16 || width > SK_MAX_W || width % 16 != 0 || num_layers < 0 || num_handles < 2 || num_handles > SK_MAX_H)
    return (int)hipErrorInvalidValue;
  if (pts == nullptr || bb_min == nullptr || bb_max == nullptr || params == nullptr || weights == nullptr || weights_jac == nullptr)
    return (int)hipErrorInvalidValue;
  SkArgs a;
  a.pts = pts, a.bb_min = bb_min, a.bb_max = bb_max, a.params = params, a.weights = weights, a.jac = weights_jac;
  a.N = N, a.tiles = (N + SK_TILE - 1) / SK_TILE;
  a.L = num_layers, a.H = num_handles, a.HB = (num_handles - 1 + 15) / 16;
  const int rows = 16 * a.HB > width ? 16 * a.HB : width;
  a.image = rows * width;
  const size_t lds = (size_t)(width <= 64 ? 2 : 1) * a.image * sizeof(float);   // at most 64 KiB
  const unsigned groups = (unsigned)(a.tiles < SK_MAX_GROUPS ? a.tiles : SK_MAX_GROUPS);
  hipStream_t st = (hipStream_t)stream;
  switch (width / 16) {
    case 1: sk_launch<1>(st, groups, lds, a); break;
    case 2: sk_launch<2>(st, groups, lds, a); break;
    case 3: sk_launch<3>(st, groups, lds, a); break;
    case 4: sk_launch<4>(st, groups, lds, a); break;
    case 5: sk_launch<5>(st, groups, lds, a); break;
    case 6: sk_launch<6>(st, groups, lds, a); break;
    case 7: sk_launch<7>(st, groups, lds, a); break;
    default: sk_launch<8>(st, groups, lds, a); break;
  }
  KAMD_RETURN_LAST_ERROR();
}

int kamd_debug_skinning_elu(void* stream, int64_t n, const float* y, float* elu, float* delu) {
  if (n < 0 || (n > 0 && (y == nullptr || elu == nullptr || delu == nullptr))) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  int64_t blocks = (n + 255) / 256;
  if (blocks > (int64_t)KAMD_NUM_CU * 16) blocks = (int64_t)KAMD_NUM_CU * 16;
  hipLaunchKernelGGL(sk_elu_probe_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n, y, elu, delu);
  KAMD_RETURN_LAST_ERROR();
}
}
