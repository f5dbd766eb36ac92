// metrics.tetmesh: tetrahedron_volume, equivolume and amips, forward and backward, one fused kernel per direction (the reference is
// a chain of 10-20 torch kernels over (B, T, 4, 3) that materialise a T-sized intermediate each and keep it for backward,
// kaolin/metrics/tetmesh.py).  A thread owns a tet: it reads its 12 coordinates (and, for amips, its 3x3 inverse offset matrix)
// once and keeps everything else in registers; the backward kernels save nothing and recompute.
//
//     volume      ((A - D) . ((B - D) x (C - D))) / 6, signed
//                 backward, s = g / 6:  dA = s (b x c), dB = s (c x a), dC = s (a x b), dD = -(dA + dB + dC)   (a = A - D, ...)
//     equivolume  mean over the tets of |v - m|^p, m ONE element shared by the batch, p an integer in 1..16 (a multiply chain)
//                 backward: the volume's backward with g = go / T * p |v - m|^(p-1) sign(v - m) (sign(0) = 0, as torch.abs), and
//                 grad m = - the sum of those g over every tet of every item
//     amips       O = rows B - A, C - A, D - A; J = O M; e = tr(J J^T) / (det^2 + 1e-10)^(1/3) * (det >= 0)  (a product, not a
//                 select); the mean over the tets.  det and its derivative are the cofactor expansion: nothing divides by det
//                 backward: G = dE/dJ = (go / T) (2 J / den - (2/3) tr det (det^2 + eps)^(-4/3) cof(J)) * (det >= 0),
//                 dO = G M^T, dM = O^T G, dB dC dD = the rows of dO, dA = -(dB + dC + dD)
//
// MEMORY  Every kernel is bound by its compulsory bytes (float32: 48 read per tet; + 36 for M; + 48 / 36 written by a backward).
//   The 12 coordinates of a tet are three (float) or six (double) 16-byte loads when the base and the batch stride are 16-byte
//   aligned; the HOST picks that variant or the scalar one per call (template parameter ALIGNED).  M's 9 elements start at a
//   multiple of 36 / 72 bytes: scalar loads.  Offsets are 64-bit throughout.
// REDUCTIONS  (the two losses, and grad m) are deterministic and use no atomics and nothing that waits on another workgroup:
//   1. at most TM_REDUCE_BLOCKS workgroups per batch item walk the tets with a grid stride; a thread adds its terms in double,
//      then a wave reduction (shuffles), then LDS across the four waves, and ONE partial per workgroup goes to the workspace;
//   2. a second launch of one workgroup per result adds the partials in a fixed order in double and divides by T.
//   Two launches because the only way to finish inside the first is to know which workgroup is last -- a counter and a fence,
//   i.e. one workgroup waiting on the others' memory -- and that family of constructions is what this file stays away from.
// Nothing here reads back to the host or synchronises the stream: every operator captures into a graph.
#include "common.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr int TM_THREADS = 256;
constexpr long long TM_REDUCE_BLOCKS = 2048;  // partials per batch item: two resident sets of the 256 CUs at B = 1
constexpr long long TM_MAX_BLOCKS = 1ll << 20;
constexpr long long TM_MAX_BATCH_Y = 65535;

inline long long tm_cdiv(long long a, long long b) { return (a + b - 1) / b; }
inline long long tm_blocks(long long T, long long cap) {
  const long long n = tm_cdiv(T, TM_THREADS);
  return n < cap ? n : cap;
}

// ---- loads and stores of one tet (12 elements) ------------------------------------------------------------------------------
template <typename T, bool ALIGNED>
__device__ __forceinline__ void tm_load12(const T* __restrict__ p, T* x) {
  if constexpr (ALIGNED && sizeof(T) == 4) {
    const float4* q = (const float4*)p;
    const float4 u = q[0], v = q[1], w = q[2];
    x[0] = u.x, x[1] = u.y, x[2] = u.z, x[3] = u.w, x[4] = v.x, x[5] = v.y, x[6] = v.z, x[7] = v.w;
    x[8] = w.x, x[9] = w.y, x[10] = w.z, x[11] = w.w;
  } else if constexpr (ALIGNED) {
    const double2* q = (const double2*)p;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double2 u = q[i];
      x[2 * i] = u.x, x[2 * i + 1] = u.y;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) x[i] = p[i];
  }
}
template <typename T, bool ALIGNED>
__device__ __forceinline__ void tm_store12(T* __restrict__ p, const T* x) {
  if constexpr (ALIGNED && sizeof(T) == 4) {
    float4* q = (float4*)p;
    q[0] = make_float4(x[0], x[1], x[2], x[3]);
    q[1] = make_float4(x[4], x[5], x[6], x[7]);
    q[2] = make_float4(x[8], x[9], x[10], x[11]);
  } else if constexpr (ALIGNED) {
    double2* q = (double2*)p;
#pragma unroll
    for (int i = 0; i < 6; ++i) q[i] = make_double2(x[2 * i], x[2 * i + 1]);
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) p[i] = x[i];
  }
}

// ---- per-tet arithmetic ---------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void tm_cross(const T* b, const T* c, T* r) {
  r[0] = b[1] * c[2] - b[2] * c[1];
  r[1] = b[2] * c[0] - b[0] * c[2];
  r[2] = b[0] * c[1] - b[1] * c[0];
}
// a = A - D, b = B - D, c = C - D
template <typename T>
__device__ __forceinline__ void tm_edges_to_d(const T* x, T* a, T* b, T* c) {
#pragma unroll
  for (int k = 0; k < 3; ++k) a[k] = x[k] - x[9 + k], b[k] = x[3 + k] - x[9 + k], c[k] = x[6 + k] - x[9 + k];
}
template <typename T>
__device__ __forceinline__ T tm_volume(const T* x) {
  T a[3], b[3], c[3], n[3];
  tm_edges_to_d(x, a, b, c);
  tm_cross(b, c, n);
  return ((a[0] * n[0] + a[1] * n[1]) + a[2] * n[2]) / (T)6;
}
// the gradient of g * volume in the 12 coordinates
template <typename T>
__device__ __forceinline__ void tm_volume_grad(const T* x, T g, T* dx) {
  T a[3], b[3], c[3], na[3], nb[3], nc[3];
  tm_edges_to_d(x, a, b, c);
  tm_cross(b, c, na);
  tm_cross(c, a, nb);
  tm_cross(a, b, nc);
  const T s = g / (T)6;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    dx[k] = s * na[k], dx[3 + k] = s * nb[k], dx[6 + k] = s * nc[k];
    dx[9 + k] = -((dx[k] + dx[3 + k]) + dx[6 + k]);
  }
}
template <typename T>
__device__ __forceinline__ T tm_abs(T x) { return x < (T)0 ? -x : x; }
template <typename T>
__device__ __forceinline__ T tm_ipow(T a, int p) {  // a^p, p >= 0, as p - 1 multiplications
  T r = (T)1;
  for (int i = 0; i < p; ++i) r *= a;
  return r;
}

template <typename T>
__device__ __forceinline__ T tm_cbrt(T x);
template <>
__device__ __forceinline__ float tm_cbrt<float>(float x) { return cbrtf(x); }
template <>
__device__ __forceinline__ double tm_cbrt<double>(double x) { return cbrt(x); }

template <typename T>
struct TmJacobian {
  T o[9], j[9], cof[9], det, tr;
};
// O (rows B - A, C - A, D - A), J = O M, the cofactors of J, det J (expansion along row 0) and tr(J J^T)
template <typename T>
__device__ __forceinline__ void tm_jacobian(const T* x, const T* m, TmJacobian<T>& q) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) q.o[3 * i + k] = x[3 * (i + 1) + k] - x[k];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) q.j[3 * i + j] = (q.o[3 * i] * m[j] + q.o[3 * i + 1] * m[3 + j]) + q.o[3 * i + 2] * m[6 + j];
  const T* J = q.j;
  q.cof[0] = J[4] * J[8] - J[5] * J[7];
  q.cof[1] = J[5] * J[6] - J[3] * J[8];
  q.cof[2] = J[3] * J[7] - J[4] * J[6];
  q.cof[3] = J[2] * J[7] - J[1] * J[8];
  q.cof[4] = J[0] * J[8] - J[2] * J[6];
  q.cof[5] = J[1] * J[6] - J[0] * J[7];
  q.cof[6] = J[1] * J[5] - J[2] * J[4];
  q.cof[7] = J[2] * J[3] - J[0] * J[5];
  q.cof[8] = J[0] * J[4] - J[1] * J[3];
  q.det = (J[0] * q.cof[0] + J[1] * q.cof[1]) + J[2] * q.cof[2];
  T tr = (T)0;
#pragma unroll
  for (int i = 0; i < 9; ++i) tr += J[i] * J[i];
  q.tr = tr;
}

// ---- the sum of one value per thread over the workgroup, in a fixed order; every thread calls it and gets the sum --------------------
__device__ __forceinline__ double tm_block_sum(double v) {
  __shared__ double lanes[TM_THREADS / KAMD_WAVE];
#pragma unroll
  for (int o = KAMD_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, KAMD_WAVE);
  if ((threadIdx.x & (KAMD_WAVE - 1)) == 0) lanes[threadIdx.x / KAMD_WAVE] = v;
  __syncthreads();
  const double r = (lanes[0] + lanes[1]) + (lanes[2] + lanes[3]);
  __syncthreads();  // (the next call writes `lanes` again)
  return r;
}

// out[i] = (the partials [i n, (i + 1) n) added in a fixed order) / divisor; one workgroup per result
template <typename T>
__global__ __launch_bounds__(TM_THREADS) void tm_finish_kernel(const double* __restrict__ partials, long long n, double divisor,
                                                               T* __restrict__ out) {
  const double* p = partials + (long long)blockIdx.x * n;
  double acc = 0.0;
  for (long long i = threadIdx.x; i < n; i += TM_THREADS) acc += p[i];
  const double total = tm_block_sum(acc);
  if (threadIdx.x == 0) out[blockIdx.x] = (T)(total / divisor);
}

// ---- volume ---------------------------------------------------------------------------------------------------------------------
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(TM_THREADS) void tm_volume_forward_kernel(long long B, long long NT, const T* __restrict__ tv,
                                                                       long long bs, T* __restrict__ volumes) {
  const long long stride = (long long)gridDim.x * TM_THREADS;
  for (long long b = blockIdx.y; b < B; b += gridDim.y)
    for (long long t = (long long)blockIdx.x * TM_THREADS + threadIdx.x; t < NT; t += stride) {
      T x[12];
      tm_load12<T, ALIGNED>(tv + b * bs + t * 12, x);
      volumes[b * NT + t] = tm_volume(x);
    }
}

template <typename T, bool ALIGNED>
__global__ __launch_bounds__(TM_THREADS) void tm_volume_backward_kernel(long long B, long long NT, const T* __restrict__ tv,
                                                                        long long bs, const T* __restrict__ grad_volumes,
                                                                        T* __restrict__ grad_tv) {
  const long long stride = (long long)gridDim.x * TM_THREADS;
  for (long long b = blockIdx.y; b < B; b += gridDim.y)
    for (long long t = (long long)blockIdx.x * TM_THREADS + threadIdx.x; t < NT; t += stride) {
      T x[12], dx[12];
      tm_load12<T, ALIGNED>(tv + b * bs + t * 12, x);
      tm_volume_grad(x, grad_volumes[b * NT + t], dx);
      tm_store12<T, ALIGNED>(grad_tv + (b * NT + t) * 12, dx);
    }
}

// ---- equivolume -----------------------------------------------------------------------------------------------------------------
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(TM_THREADS) void tm_equivolume_forward_kernel(long long B, long long NT, const T* __restrict__ tv,
                                                                           long long bs, const T* __restrict__ mean, int power,
                                                                           double* __restrict__ partials) {
  const long long stride = (long long)gridDim.x * TM_THREADS;
  const T m = mean[0];
  for (long long b = blockIdx.y; b < B; b += gridDim.y) {
    double acc = 0.0;
    for (long long t = (long long)blockIdx.x * TM_THREADS + threadIdx.x; t < NT; t += stride) {
      T x[12];
      tm_load12<T, ALIGNED>(tv + b * bs + t * 12, x);
      acc += (double)tm_ipow(tm_abs(tm_volume(x) - m), power);
    }
    const double total = tm_block_sum(acc);
    if (threadIdx.x == 0) partials[b * gridDim.x + blockIdx.x] = total;
  }
}

// grad_tv and partials (for grad mean) may each be NULL: that gradient is then not computed
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(TM_THREADS) void tm_equivolume_backward_kernel(long long B, long long NT, const T* __restrict__ tv,
                                                                            long long bs, const T* __restrict__ mean, int power,
                                                                            const T* __restrict__ grad_loss, T* __restrict__ grad_tv,
                                                                            double* __restrict__ partials) {
  const long long stride = (long long)gridDim.x * TM_THREADS;
  const T m = mean[0];
  for (long long b = blockIdx.y; b < B; b += gridDim.y) {
    const T scale = grad_loss[b] / (T)NT * (T)power;
    double acc = 0.0;
    for (long long t = (long long)blockIdx.x * TM_THREADS + threadIdx.x; t < NT; t += stride) {
      T x[12], dx[12];
      tm_load12<T, ALIGNED>(tv + b * bs + t * 12, x);
      const T d = tm_volume(x) - m;
      const T sign = d > (T)0 ? (T)1 : (d < (T)0 ? (T)-1 : (T)0);
      const T g = scale * tm_ipow(tm_abs(d), power - 1) * sign;
      acc -= (double)g;
      if (grad_tv != nullptr) {
        tm_volume_grad(x, g, dx);
        tm_store12<T, ALIGNED>(grad_tv + (b * NT + t) * 12, dx);
      }
    }
    if (partials != nullptr) {  // (uniform over the grid)
      const double total = tm_block_sum(acc);
      if (threadIdx.x == 0) partials[b * gridDim.x + blockIdx.x] = total;
    }
  }
}

// ---- amips ----------------------------------------------------------------------------------------------------------------------
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(TM_THREADS) void tm_amips_forward_kernel(long long B, long long NT, const T* __restrict__ tv, long long bs,
                                                                      const T* __restrict__ inv, long long inv_bs,
                                                                      double* __restrict__ partials) {
  const long long stride = (long long)gridDim.x * TM_THREADS;
  for (long long b = blockIdx.y; b < B; b += gridDim.y) {
    double acc = 0.0;
    for (long long t = (long long)blockIdx.x * TM_THREADS + threadIdx.x; t < NT; t += stride) {
      T x[12], m[9];
      tm_load12<T, ALIGNED>(tv + b * bs + t * 12, x);
      const T* mp = inv + b * inv_bs + t * 9;
#pragma unroll
      for (int i = 0; i < 9; ++i) m[i] = mp[i];
      TmJacobian<T> q;
      tm_jacobian(x, m, q);
      const T den = tm_cbrt(q.det * q.det + (T)1e-10);
      acc += (double)(q.tr / den * (q.det >= (T)0 ? (T)1 : (T)0));
    }
    const double total = tm_block_sum(acc);
    if (threadIdx.x == 0) partials[b * gridDim.x + blockIdx.x] = total;
  }
}

// grad_tv (B, T, 4, 3) and grad_inv (B, T, 3, 3) may each be NULL
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(TM_THREADS) void tm_amips_backward_kernel(long long B, long long NT, const T* __restrict__ tv, long long bs,
                                                                       const T* __restrict__ inv, long long inv_bs,
                                                                       const T* __restrict__ grad_loss, T* __restrict__ grad_tv,
                                                                       T* __restrict__ grad_inv) {
  const long long stride = (long long)gridDim.x * TM_THREADS;
  for (long long b = blockIdx.y; b < B; b += gridDim.y) {
    const T s = grad_loss[b] / (T)NT;
    for (long long t = (long long)blockIdx.x * TM_THREADS + threadIdx.x; t < NT; t += stride) {
      T x[12], m[9], g[9];
      tm_load12<T, ALIGNED>(tv + b * bs + t * 12, x);
      const T* mp = inv + b * inv_bs + t * 9;
#pragma unroll
      for (int i = 0; i < 9; ++i) m[i] = mp[i];
      TmJacobian<T> q;
      tm_jacobian(x, m, q);
      const T det2 = q.det * q.det + (T)1e-10;
      const T den = tm_cbrt(det2);
      const T mask = q.det >= (T)0 ? (T)1 : (T)0;
      const T k2 = (T)2 / den, kc = ((T)2 / (T)3) * q.tr * q.det / (den * det2);
#pragma unroll
      for (int i = 0; i < 9; ++i) g[i] = s * (k2 * q.j[i] - kc * q.cof[i]) * mask;
      if (grad_tv != nullptr) {
        T dx[12];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int k = 0; k < 3; ++k) dx[3 * (i + 1) + k] = (g[3 * i] * m[3 * k] + g[3 * i + 1] * m[3 * k + 1]) + g[3 * i + 2] * m[3 * k + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k) dx[k] = -((dx[3 + k] + dx[6 + k]) + dx[9 + k]);
        tm_store12<T, ALIGNED>(grad_tv + (b * NT + t) * 12, dx);
      }
      if (grad_inv != nullptr) {
        T* out = grad_inv + (b * NT + t) * 9;
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
          for (int j = 0; j < 3; ++j) out[3 * k + j] = (q.o[k] * g[j] + q.o[3 + k] * g[3 + j]) + q.o[6 + k] * g[6 + j];
      }
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
inline bool tm_bad_extents(long long B, long long T, long long bs) {
  return B < 0 || T < 0 || bs < 0 || T > (1ll << 40) || B > (1ll << 31);
}
inline bool tm_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// 16-byte loads of a tet: the base and every batch item's start are 16-byte aligned (a tet's own offset, 48 / 96 bytes, is)
template <typename T>
inline bool tm_vector_loads(const T* tv, long long B, long long bs, const void* out) {
  return tm_aligned16(tv) && (B == 1 || (bs * (long long)sizeof(T)) % 16 == 0) && tm_aligned16(out);
}
inline dim3 tm_grid(long long B, long long T, long long cap) {
  return dim3((unsigned)tm_blocks(T, cap), (unsigned)(B < TM_MAX_BATCH_Y ? B : TM_MAX_BATCH_Y));
}
size_t tm_workspace_bytes(long long B, long long T) {
  if (B <= 0 || T <= 0 || tm_bad_extents(B, T, 0)) return 0;
  return (size_t)(B * tm_blocks(T, TM_REDUCE_BLOCKS)) * sizeof(double);
}

#define TM_LAUNCH(KERNEL, ALIGNED, GRID, ...)                                                                 \
  do {                                                                                                        \
    if (ALIGNED)                                                                                              \
      hipLaunchKernelGGL((KERNEL<T, true>), GRID, dim3(TM_THREADS), 0, st, __VA_ARGS__);                      \
    else                                                                                                      \
      hipLaunchKernelGGL((KERNEL<T, false>), GRID, dim3(TM_THREADS), 0, st, __VA_ARGS__);                     \
  } while (0)

template <typename T>
int tm_volume_forward(hipStream_t st, long long B, long long NT, const T* tv, long long bs, T* volumes) {
  if (tm_bad_extents(B, NT, bs)) return (int)hipErrorInvalidValue;
  if (B == 0 || NT == 0) return 0;
  if (tv == nullptr || volumes == nullptr) return (int)hipErrorInvalidValue;
  TM_LAUNCH(tm_volume_forward_kernel, tm_vector_loads(tv, B, bs, nullptr), tm_grid(B, NT, TM_MAX_BLOCKS), B, NT, tv, bs, volumes);
  KAMD_RETURN_LAST_ERROR();
}

template <typename T>
int tm_volume_backward(hipStream_t st, long long B, long long NT, const T* tv, long long bs, const T* grad_volumes, T* grad_tv) {
  if (tm_bad_extents(B, NT, bs)) return (int)hipErrorInvalidValue;
  if (B == 0 || NT == 0) return 0;
  if (tv == nullptr || grad_volumes == nullptr || grad_tv == nullptr) return (int)hipErrorInvalidValue;
  TM_LAUNCH(tm_volume_backward_kernel, tm_vector_loads(tv, B, bs, grad_tv), tm_grid(B, NT, TM_MAX_BLOCKS), B, NT, tv, bs,
            grad_volumes, grad_tv);
  KAMD_RETURN_LAST_ERROR();
}

template <typename T>
int tm_equivolume_forward(hipStream_t st, long long B, long long NT, const T* tv, long long bs, const T* mean, int power, T* loss,
                          void* workspace) {
  if (tm_bad_extents(B, NT, bs) || power < 1 || power > 16) return (int)hipErrorInvalidValue;
  if (B == 0 || NT == 0) return 0;
  if (tv == nullptr || mean == nullptr || loss == nullptr || workspace == nullptr) return (int)hipErrorInvalidValue;
  const dim3 grid = tm_grid(B, NT, TM_REDUCE_BLOCKS);
  double* partials = (double*)workspace;
  TM_LAUNCH(tm_equivolume_forward_kernel, tm_vector_loads(tv, B, bs, nullptr), grid, B, NT, tv, bs, mean, power, partials);
  hipLaunchKernelGGL((tm_finish_kernel<T>), dim3((unsigned)B), dim3(TM_THREADS), 0, st, (const double*)partials, (long long)grid.x,
                     (double)NT, loss);
  KAMD_RETURN_LAST_ERROR();
}

template <typename T>
int tm_equivolume_backward(hipStream_t st, long long B, long long NT, const T* tv, long long bs, const T* mean, int power,
                           const T* grad_loss, T* grad_tv, T* grad_mean, void* workspace) {
  if (tm_bad_extents(B, NT, bs) || power < 1 || power > 16) return (int)hipErrorInvalidValue;
  if (B == 0 || NT == 0 || (grad_tv == nullptr && grad_mean == nullptr)) return 0;
  if (tv == nullptr || mean == nullptr || grad_loss == nullptr || (grad_mean != nullptr && workspace == nullptr))
    return (int)hipErrorInvalidValue;
  // (without grad_mean nothing is reduced: the plain grid, a tet per thread)
  const dim3 grid = tm_grid(B, NT, grad_mean != nullptr ? TM_REDUCE_BLOCKS : TM_MAX_BLOCKS);
  double* partials = grad_mean != nullptr ? (double*)workspace : nullptr;
  TM_LAUNCH(tm_equivolume_backward_kernel, tm_vector_loads(tv, B, bs, grad_tv), grid, B, NT, tv, bs, mean, power, grad_loss, grad_tv,
            partials);
  if (grad_mean != nullptr)
    hipLaunchKernelGGL((tm_finish_kernel<T>), dim3(1), dim3(TM_THREADS), 0, st, (const double*)partials, B * (long long)grid.x, 1.0,
                       grad_mean);
  KAMD_RETURN_LAST_ERROR();
}

template <typename T>
int tm_amips_forward(hipStream_t st, long long B, long long NT, const T* tv, long long bs, const T* inv, long long inv_bs, T* loss,
                     void* workspace) {
  if (tm_bad_extents(B, NT, bs) || inv_bs < 0) return (int)hipErrorInvalidValue;
  if (B == 0 || NT == 0) return 0;
  if (tv == nullptr || inv == nullptr || loss == nullptr || workspace == nullptr) return (int)hipErrorInvalidValue;
  const dim3 grid = tm_grid(B, NT, TM_REDUCE_BLOCKS);
  double* partials = (double*)workspace;
  TM_LAUNCH(tm_amips_forward_kernel, tm_vector_loads(tv, B, bs, nullptr), grid, B, NT, tv, bs, inv, inv_bs, partials);
  hipLaunchKernelGGL((tm_finish_kernel<T>), dim3((unsigned)B), dim3(TM_THREADS), 0, st, (const double*)partials, (long long)grid.x,
                     (double)NT, loss);
  KAMD_RETURN_LAST_ERROR();
}

template <typename T>
int tm_amips_backward(hipStream_t st, long long B, long long NT, const T* tv, long long bs, const T* inv, long long inv_bs,
                      const T* grad_loss, T* grad_tv, T* grad_inv) {
  if (tm_bad_extents(B, NT, bs) || inv_bs < 0) return (int)hipErrorInvalidValue;
  if (B == 0 || NT == 0 || (grad_tv == nullptr && grad_inv == nullptr)) return 0;
  if (tv == nullptr || inv == nullptr || grad_loss == nullptr) return (int)hipErrorInvalidValue;
  TM_LAUNCH(tm_amips_backward_kernel, tm_vector_loads(tv, B, bs, grad_tv), tm_grid(B, NT, TM_MAX_BLOCKS), B, NT, tv, bs, inv, inv_bs,
            grad_loss, grad_tv, grad_inv);
  KAMD_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {

size_t kamd_tetmesh_reduce_workspace(int64_t B, int64_t T) { return tm_workspace_bytes(B, T); }

#define KAMD_TM_ENTRIES(SFX, CT)                                                                                                     \
  int kamd_tetmesh_volume_forward_##SFX(void* stream, int64_t B, int64_t T, const CT* tet_vertices, int64_t batch_stride,            \
                                        CT* volumes) {                                                                               \
    return tm_volume_forward<CT>((hipStream_t)stream, B, T, tet_vertices, batch_stride, volumes);                                    \
  }                                                                                                                                  \
  int kamd_tetmesh_volume_backward_##SFX(void* stream, int64_t B, int64_t T, const CT* tet_vertices, int64_t batch_stride,           \
                                         const CT* grad_volumes, CT* grad_tet_vertices) {                                            \
    return tm_volume_backward<CT>((hipStream_t)stream, B, T, tet_vertices, batch_stride, grad_volumes, grad_tet_vertices);           \
  }                                                                                                                                  \
  int kamd_tetmesh_equivolume_forward_##SFX(void* stream, int64_t B, int64_t T, const CT* tet_vertices, int64_t batch_stride,        \
                                            const CT* mean, int power, CT* loss, void* workspace) {                                  \
    return tm_equivolume_forward<CT>((hipStream_t)stream, B, T, tet_vertices, batch_stride, mean, power, loss, workspace);           \
  }                                                                                                                                  \
  int kamd_tetmesh_equivolume_backward_##SFX(void* stream, int64_t B, int64_t T, const CT* tet_vertices, int64_t batch_stride,       \
                                             const CT* mean, int power, const CT* grad_loss, CT* grad_tet_vertices, CT* grad_mean,   \
                                             void* workspace) {                                                                      \
    return tm_equivolume_backward<CT>((hipStream_t)stream, B, T, tet_vertices, batch_stride, mean, power, grad_loss,                 \
                                      grad_tet_vertices, grad_mean, workspace);                                                      \
  }                                                                                                                                  \
  int kamd_tetmesh_amips_forward_##SFX(void* stream, int64_t B, int64_t T, const CT* tet_vertices, int64_t batch_stride,             \
                                       const CT* inverse_offset_matrix, int64_t inverse_batch_stride, CT* loss, void* workspace) {   \
    return tm_amips_forward<CT>((hipStream_t)stream, B, T, tet_vertices, batch_stride, inverse_offset_matrix, inverse_batch_stride,  \
                                loss, workspace);                                                                                    \
  }                                                                                                                                  \
  int kamd_tetmesh_amips_backward_##SFX(void* stream, int64_t B, int64_t T, const CT* tet_vertices, int64_t batch_stride,            \
                                        const CT* inverse_offset_matrix, int64_t inverse_batch_stride, const CT* grad_loss,          \
                                        CT* grad_tet_vertices, CT* grad_inverse_offset_matrix) {                                     \
    return tm_amips_backward<CT>((hipStream_t)stream, B, T, tet_vertices, batch_stride, inverse_offset_matrix,                       \
                                 inverse_batch_stride, grad_loss, grad_tet_vertices, grad_inverse_offset_matrix);                    \
  }
KAMD_TM_ENTRIES(f32, float)
KAMD_TM_ENTRIES(f64, double)
#undef KAMD_TM_ENTRIES

}  // extern "C"
