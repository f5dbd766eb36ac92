// The Simplicits training losses on the GPU, forward and backward, fused: the elastic loss of N points under B random transforms of
// H' handles and the orthogonality loss of their weights.  float32.
//
//   F_pb = I + sum_h ( w_ph T_bh[:, :3] + (T_bh (x_p, 1)) (x) grad w_ph )                       (9 * 4 H' multiply-adds a pair)
//   le = scale_le sum_{p, b} [ (1 - s) Psi_lin(F_pb) + s Psi_neo(F_pb) ],   lo = scale_lo mean((W^T W - I)^2)
//   Psi_lin = mu |eps|^2 + lam / 2 tr(eps)^2, eps = (F + F^T) / 2 - I;  Psi_neo = mu / 2 (|F|^2 - 3) + lam / 2 (J - 1)^2 - mu (J - 1),
//   J and cof F from 2x2 minors (finite for an inverted F).  T = 0 gives F = I, both energies and both stresses exactly 0.
//
// Bound by launches and latency, not by arithmetic: spelled fmaf in the lane (-ffp-contract=off, no packed float32), no matrix
// instruction.  A thread owns a point; a workgroup of 256 strides over tiles of 256 points; `transforms` pass through LDS in chunks
// of whole transforms (24 KiB), read at one address by all lanes.
//
// FORWARD, in float64 from the float32 inputs on (a one-element output is one rounding: le and lo are the float32 nearest to what
// the inputs define; the kernel is bound by latency, and the gradient stays float32).  sl_forward_kernel: each thread sums its points' energies over b in order, a fixed tree sums the workgroup; for
// G = W^T W the tile's weights pass through LDS in chunks of at most 4096 floats and thread t owns the entries t, t + 256, ... of the
// workgroup's partial G, summing the chunk's points in order.  Partial image per workgroup: 1 + H'^2 doubles.  sl_finish_kernel (one
// workgroup) sums the images in the order of the workgroups: le, G - I (kept for the backward), lo.
// BACKWARD.  sl_backward_kernel recomputes F_pb, forms P = k [(1 - s)(2 mu eps + lam tr(eps) I) + s (mu F + (lam (J - 1) - mu) cof F)]
// with k = grad_le scale_le, and adds, b after b in order, to the point's own rows
//   grad_jac[p][h][j] += sum_i (T_bh (x_p, 1))_i P[i][j],      grad_w[p][h] += sum_ij T_bh[i][j] P[i][j]
// which are sum_n x~_n dM[h][n][j] and sum_j dM[h][j][j] of dM = sum_b T_b^T P_pb; grad_w starts from the orthogonality term
// grad_lo (4 scale_lo / H'^2) (W (G - I))[p][h].  A point's rows belong to one thread: no atomics, the same bits on every call.
// The upstream gradients are read on the device.  B == 0 computes the orthogonality loss alone (jac, pts, transforms, mu, lam unread).
#include "common.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr int SL_THREADS = 256;
constexpr int SL_T_FLOATS = 6144;   // LDS floats of a chunk of transforms: at least 4 transforms of 127 handles
constexpr int SL_W_FLOATS = 4096;   // LDS floats of a chunk of weights: at least 32 points of 127 handles
constexpr int SL_MAX_HP = 127;
constexpr int SL_MAX_GROUPS = 64;   // partial images of the forward
constexpr int SL_MAX_BACK_GROUPS = KAMD_NUM_CU * 4;

struct SlArgs {
  const float *w, *jac, *pts, *transforms, *mu, *lam, *gmi_in, *grad_le, *grad_lo;
  double* partial;
  float *grad_w, *grad_jac;
  int64_t N, tiles;
  int B, HP;
  float s, scale_le, scale_lo;
};

__device__ __forceinline__ float sl_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double sl_fma(double a, double b, double c) { return fma(a, b, c); }

// F of one point under one transform; T: the transform's H' 3x4 blocks in LDS.  R = float (backward) or double (forward)
template <class R>
__device__ __forceinline__ void sl_defo(R (&F)[9], const float* T, const float* __restrict__ w, const float* __restrict__ jac, int HP,
                                        R x, R y, R z) {
#pragma unroll
  for (int e = 0; e < 9; ++e) F[e] = (e % 4 == 0) ? R(1) : R(0);
  for (int h = 0; h < HP; ++h, T += 12) {
    const R wv = w[h], j0 = jac[3 * h], j1 = jac[3 * h + 1], j2 = jac[3 * h + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const R t0 = T[4 * i], t1 = T[4 * i + 1], t2 = T[4 * i + 2], t3 = T[4 * i + 3];
      const R tx = sl_fma(t2, z, sl_fma(t1, y, sl_fma(t0, x, t3)));
      F[3 * i] = sl_fma(tx, j0, sl_fma(wv, t0, F[3 * i]));
      F[3 * i + 1] = sl_fma(tx, j1, sl_fma(wv, t1, F[3 * i + 1]));
      F[3 * i + 2] = sl_fma(tx, j2, sl_fma(wv, t2, F[3 * i + 2]));
    }
  }
}

// cof F from 2x2 minors (row-major, C[3 i + j] = dJ / dF[i][j]) and J
template <class R>
__device__ __forceinline__ R sl_cofactor(R (&C)[9], const R (&F)[9]) {
  C[0] = sl_fma(F[4], F[8], -(F[5] * F[7])), C[1] = sl_fma(F[5], F[6], -(F[3] * F[8])), C[2] = sl_fma(F[3], F[7], -(F[4] * F[6]));
  C[3] = sl_fma(F[7], F[2], -(F[8] * F[1])), C[4] = sl_fma(F[8], F[0], -(F[6] * F[2])), C[5] = sl_fma(F[6], F[1], -(F[7] * F[0]));
  C[6] = sl_fma(F[1], F[5], -(F[2] * F[4])), C[7] = sl_fma(F[2], F[3], -(F[0] * F[5])), C[8] = sl_fma(F[0], F[4], -(F[1] * F[3]));
  return sl_fma(F[2], C[2], sl_fma(F[1], C[1], F[0] * C[0]));
}

// eps = (F + F^T) / 2 - I: its diagonal, its three off-diagonal entries (01, 02, 12) and its trace
template <class R>
__device__ __forceinline__ R sl_strain(R (&d)[3], R (&o)[3], const R (&F)[9]) {
  d[0] = F[0] - R(1), d[1] = F[4] - R(1), d[2] = F[8] - R(1);
  o[0] = R(0.5) * (F[1] + F[3]), o[1] = R(0.5) * (F[2] + F[6]), o[2] = R(0.5) * (F[5] + F[7]);
  return (d[0] + d[1]) + d[2];
}

// the forward's energies are float64 throughout: le is the float32 nearest to the sum of the float32 inputs' energies
__device__ __forceinline__ double sl_energy(const double (&F)[9], double mu, double lam, double s) {
  double d[3], o[3], C[9];
  const double tr = sl_strain(d, o, F);
  const double diag = fma(d[2], d[2], fma(d[1], d[1], d[0] * d[0])), off = fma(o[2], o[2], fma(o[1], o[1], o[0] * o[0]));
  const double lin = fma(mu, fma(2.0, off, diag), (0.5 * lam) * (tr * tr));
  const double Jm1 = sl_cofactor(C, F) - 1.0;
  double ff = 0.0;
#pragma unroll
  for (int e = 0; e < 9; ++e) ff = fma(F[e], F[e], ff);
  const double neo = fma(0.5 * mu, ff - 3.0, fma(0.5 * lam, Jm1 * Jm1, -(mu * Jm1)));
  return fma(1.0 - s, lin, s * neo);
}

// P = k [(1 - s)(2 mu eps + lam tr(eps) I) + s (mu F + (lam (J - 1) - mu) cof F)]
__device__ __forceinline__ void sl_stress(float (&P)[9], const float (&F)[9], float mu, float lam, float s, float k) {
  float d[3], o[3], C[9];
  const float tr = sl_strain(d, o, F);
  const float a = fmaf(lam, sl_cofactor(C, F) - 1.0f, -mu);
  const float kl = k * (1.0f - s), kn = k * s;
  const float eps[9] = {d[0], o[0], o[1], o[0], d[1], o[2], o[1], o[2], d[2]};
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const float lin = fmaf(2.0f * mu, eps[e], (e % 4 == 0) ? lam * tr : 0.0f);
    const float neo = fmaf(a, C[e], mu * F[e]);
    P[e] = fmaf(kl, lin, kn * neo);
  }
}

// a chunk of whole transforms -> LDS; returns how many
__device__ __forceinline__ int sl_stage_transforms(float* sT, const SlArgs& a, int b0, int t) {
  const int cb = SL_T_FLOATS / (12 * a.HP);
  const int nb = a.B - b0 < cb ? a.B - b0 : cb;
  __syncthreads();   // the previous chunk's readers are done
  for (int e = t; e < nb * a.HP * 12; e += SL_THREADS) sT[e] = a.transforms[(size_t)b0 * a.HP * 12 + e];
  __syncthreads();
  return nb;
}

__global__ __launch_bounds__(SL_THREADS) void sl_forward_kernel(const SlArgs a) {
  __shared__ float sT[SL_T_FLOATS];
  __shared__ float sW[SL_W_FLOATS];
  __shared__ double sRed[SL_THREADS];
  const int t = threadIdx.x, HP = a.HP, HH = HP * HP;
  const int cp = SL_W_FLOATS / HP < SL_THREADS ? SL_W_FLOATS / HP : SL_THREADS;   // points of a chunk of weights
  double* part = a.partial + (size_t)blockIdx.x * (HH + 1);
  double energy = 0.0;
  for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int64_t p = tile * SL_THREADS + t;
    const bool valid = p < a.N;
    float x = 0.0f, y = 0.0f, z = 0.0f, mu = 0.0f, lam = 0.0f;
    if (valid && a.B > 0) x = a.pts[p * 3], y = a.pts[p * 3 + 1], z = a.pts[p * 3 + 2], mu = a.mu[p], lam = a.lam[p];
    for (int b0 = 0; b0 < a.B;) {
      const int nb = sl_stage_transforms(sT, a, b0, t);
      if (valid) {
        for (int b = 0; b < nb; ++b) {
          double F[9];
          sl_defo<double>(F, sT + b * HP * 12, a.w + p * HP, a.jac + p * HP * 3, HP, x, y, z);
          energy += sl_energy(F, mu, lam, a.s);
        }
      }
      b0 += nb;
    }
    // G: the tile's weights in chunks of cp points; the floats past the end of `w` are zeros
    for (int c0 = 0; c0 < SL_THREADS; c0 += cp) {
      const int64_t base = tile * SL_THREADS + c0;
      if (base >= a.N) break;
      const int npts = SL_THREADS - c0 < cp ? SL_THREADS - c0 : cp;
      __syncthreads();   // the previous chunk's readers are done
      for (int e = t; e < npts * HP; e += SL_THREADS) {
        const int64_t idx = base * HP + e;
        sW[e] = idx < a.N * HP ? a.w[idx] : 0.0f;
      }
      __syncthreads();
      const bool first = tile == blockIdx.x && c0 == 0;
      for (int e = t; e < HH; e += SL_THREADS) {
        const int i = e / HP, j = e % HP;
        double acc = first ? 0.0 : part[1 + e];
        for (int q = 0; q < npts; ++q) acc = fma((double)sW[q * HP + i], (double)sW[q * HP + j], acc);
        part[1 + e] = acc;
      }
    }
  }
  sRed[t] = energy;
  __syncthreads();
  for (int s = SL_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) sRed[t] += sRed[t + s];
    __syncthreads();
  }
  if (t == 0) part[0] = sRed[0];
}

// out = (le, lo); gmi = G - I
__global__ __launch_bounds__(SL_THREADS) void sl_finish_kernel(int groups, int HP, const double* __restrict__ partial, double scale_le,
                                                               double scale_lo, float* __restrict__ le, float* __restrict__ lo,
                                                               float* __restrict__ gmi) {
  __shared__ double sRed[SL_THREADS];
  const int t = threadIdx.x, HH = HP * HP;
  double sq = 0.0;
  for (int e = t; e < HH; e += SL_THREADS) {
    double gsum = partial[1 + e];
    for (int k = 1; k < groups; ++k) gsum += partial[(size_t)k * (HH + 1) + 1 + e];
    const double d = gsum - ((e / HP == e % HP) ? 1.0 : 0.0);
    gmi[e] = (float)d;
    sq = fma(d, d, sq);
  }
  sRed[t] = sq;
  __syncthreads();
  for (int s = SL_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) sRed[t] += sRed[t + s];
    __syncthreads();
  }
  if (t == 0) {
    double energy = partial[0];
    for (int k = 1; k < groups; ++k) energy += partial[(size_t)k * (HH + 1)];
    *le = (float)(scale_le * energy);
    *lo = (float)(scale_lo * (sRed[0] / (double)HH));
  }
}

__global__ __launch_bounds__(SL_THREADS) void sl_backward_kernel(const SlArgs a) {
  __shared__ float sT[SL_T_FLOATS];
  const int t = threadIdx.x, HP = a.HP;
  const float k = a.B > 0 ? *a.grad_le * a.scale_le : 0.0f;
  const float ko = a.scale_lo != 0.0f ? *a.grad_lo * (4.0f * a.scale_lo / (float)(HP * HP)) : 0.0f;
  for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int64_t p = tile * SL_THREADS + t;
    const bool valid = p < a.N;
    const float* w = a.w + p * HP;
    float* gw = a.grad_w + p * HP;
    float* gj = a.grad_jac + p * HP * 3;
    float x = 0.0f, y = 0.0f, z = 0.0f, mu = 0.0f, lam = 0.0f;
    if (valid) {
      if (a.B > 0) x = a.pts[p * 3], y = a.pts[p * 3 + 1], z = a.pts[p * 3 + 2], mu = a.mu[p], lam = a.lam[p];
      // the orthogonality term starts the point's rows
      for (int h = 0; h < HP; ++h) {
        float acc = 0.0f;
        if (a.scale_lo != 0.0f) {
          for (int q = 0; q < HP; ++q) acc = fmaf(w[q], a.gmi_in[q * HP + h], acc);
        }
        gw[h] = ko * acc;
        gj[3 * h] = 0.0f, gj[3 * h + 1] = 0.0f, gj[3 * h + 2] = 0.0f;
      }
    }
    for (int b0 = 0; b0 < a.B;) {
      const int nb = sl_stage_transforms(sT, a, b0, t);
      if (valid) {
        for (int b = 0; b < nb; ++b) {
          const float* T = sT + b * HP * 12;
          float F[9], P[9];
          sl_defo<float>(F, T, w, a.jac + p * HP * 3, HP, x, y, z);
          sl_stress(P, F, mu, lam, a.s, k);
          for (int h = 0; h < HP; ++h, T += 12) {
            float tx[3], tp = 0.0f;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
              tx[i] = fmaf(T[4 * i + 2], z, fmaf(T[4 * i + 1], y, fmaf(T[4 * i], x, T[4 * i + 3])));
#pragma unroll
              for (int j = 0; j < 3; ++j) tp = fmaf(T[4 * i + j], P[3 * i + j], tp);
            }
            gw[h] += tp;
#pragma unroll
            for (int j = 0; j < 3; ++j) gj[3 * h + j] += fmaf(tx[2], P[6 + j], fmaf(tx[1], P[3 + j], tx[0] * P[j]));
          }
        }
      }
      b0 += nb;
    }
  }
}

bool sl_sizes_ok(int64_t N, int B, int HP) { return N >= 1 && B >= 0 && HP >= 1 && HP <= SL_MAX_HP; }
int64_t sl_tiles(int64_t N) { return (N + SL_THREADS - 1) / SL_THREADS; }
unsigned sl_groups(int64_t N) { return (unsigned)(sl_tiles(N) < SL_MAX_GROUPS ? sl_tiles(N) : SL_MAX_GROUPS); }

}  // namespace

extern "C" {

size_t kamd_physics_simplicits_loss_workspace(int64_t N, int num_weights) {
  if (!sl_sizes_ok(N, 0, num_weights)) return 0;
  return (size_t)sl_groups(N) * ((size_t)num_weights * num_weights + 1) * sizeof(double);
}

int kamd_physics_simplicits_loss_f32(void* stream, int64_t N, int B, int num_weights, const float* weights, const float* weights_jac,
                                     const float* pts, const float* transforms, const float* mu, const float* lam, float interp,
                                     double scale_le, double scale_lo, float* le, float* lo, float* gram_minus_identity, void* workspace,
                                     size_t workspace_bytes) {
  if (!sl_sizes_ok(N, B, num_weights) || weights == nullptr || le == nullptr || lo == nullptr || gram_minus_identity == nullptr ||
      workspace == nullptr || workspace_bytes < kamd_physics_simplicits_loss_workspace(N, num_weights))
    return (int)hipErrorInvalidValue;
  if (B > 0 && (weights_jac == nullptr || pts == nullptr || transforms == nullptr || mu == nullptr || lam == nullptr))
    return (int)hipErrorInvalidValue;
  SlArgs a = {};
  a.w = weights, a.jac = weights_jac, a.pts = pts, a.transforms = transforms, a.mu = mu, a.lam = lam;
  a.partial = (double*)workspace;
  a.N = N, a.tiles = sl_tiles(N), a.B = B, a.HP = num_weights, a.s = interp, a.scale_le = (float)scale_le, a.scale_lo = (float)scale_lo;
  const unsigned groups = sl_groups(N);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sl_forward_kernel, dim3(groups), dim3(SL_THREADS), 0, st, a);
  hipLaunchKernelGGL(sl_finish_kernel, dim3(1), dim3(SL_THREADS), 0, st, (int)groups, num_weights, (const double*)workspace, scale_le,
                     scale_lo, le, lo, gram_minus_identity);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_physics_simplicits_loss_backward_f32(void* stream, int64_t N, int B, int num_weights, const float* weights,
                                              const float* weights_jac, const float* pts, const float* transforms, const float* mu,
                                              const float* lam, float interp, float scale_le, float scale_lo,
                                              const float* gram_minus_identity, const float* grad_le, const float* grad_lo,
                                              float* grad_weights, float* grad_weights_jac) {
  if (!sl_sizes_ok(N, B, num_weights) || weights == nullptr || gram_minus_identity == nullptr || grad_le == nullptr ||
      grad_lo == nullptr || grad_weights == nullptr || grad_weights_jac == nullptr)
    return (int)hipErrorInvalidValue;
  if (B > 0 && (weights_jac == nullptr || pts == nullptr || transforms == nullptr || mu == nullptr || lam == nullptr))
    return (int)hipErrorInvalidValue;
  SlArgs a = {};
  a.w = weights, a.jac = weights_jac, a.pts = pts, a.transforms = transforms, a.mu = mu, a.lam = lam;
  a.gmi_in = gram_minus_identity, a.grad_le = grad_le, a.grad_lo = grad_lo, a.grad_w = grad_weights, a.grad_jac = grad_weights_jac;
  a.N = N, a.tiles = sl_tiles(N), a.B = B, a.HP = num_weights, a.s = interp, a.scale_le = scale_le, a.scale_lo = scale_lo;
  const unsigned groups = (unsigned)(a.tiles < SL_MAX_BACK_GROUPS ? a.tiles : SL_MAX_BACK_GROUPS);
  hipLaunchKernelGGL(sl_backward_kernel, dim3(groups), dim3(SL_THREADS), 0, (hipStream_t)stream, a);
  KAMD_RETURN_LAST_ERROR();
}
}
