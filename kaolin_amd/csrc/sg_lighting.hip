// Spherical-gaussian lighting (kaolin.render.lighting, DIB-R++ shading): the reduced SG inner product and its gradient.
//
// Row i is one "sg" lobe (in shading: a pixel), column j one "other" lobe (a light); a = amplitude (RGB), d = direction,
// s = sharpness:
//     v_ij = s_i d_i + s_j d_j,   um = |v_ij|,   lm = s_i + s_j
//     G_ij = (exp(um - lm) - exp(-um - lm)) / um             (= exp(um - lm) (1 - exp(-2 um)) / um)
//     out_i[c] = 2 pi a_i[c] sum_j a_j[c] G_ij
// With g = grad_out_i, ga_i = g (*) a_i, h_ij = ga_i . a_j and q_ij = h_ij G'(um) / um, G'(um) = ((E + E2) - G) / um:
//     row:     grad_a_i = 2 pi g (*) sum_j a_j G,   grad_d_i = 2 pi s_i Qr_i,   grad_s_i = 2 pi (Qr_i . d_i - ga_i . sum_j a_j G)
//     column:  grad_a_j = 2 pi A_j,   grad_d_j = 2 pi s_j Q_j,   grad_s_j = 2 pi (Q_j . d_j - a_j . A_j)
// where Qr_i = sum_j q v, Q_j = sum_i q v and A_j = sum_i ga_i G -- six sums per column, six per row.
//
// Forward: one lane per row; the light loop is wave-uniform (every lane reads the same light: the loads are uniform) and
// runs over j in order.  Backward: a persistent grid sized from the CU count and the row count only; per chunk of CL lights
// every lane keeps the 6 CL column sums of its rows in registers (grid-stride over the rows), the workgroup reduces them
// (wavefront shuffles, then LDS, fixed order) into a per-workgroup slab of the workspace, and a second launch folds the
// slabs in workgroup order.  Rows' gradients are written directly; with more than one chunk the row's running sums are
// carried in its own gradient slots by the lane that owns the row.  No atomics: the result is bit-identical run to run.
//
// Constant-lobe variant (sg_irradiance_inner_product / sg_diffuse_inner_product: the row lobe is cosine_lobe_sg(normal) =
// (1.17, normal, 2.133)): amplitude and sharpness are two scalars, the row side reads 12 bytes (plus the 12-byte gradient
// backward) and only grad_direction is written.
#include "common.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr int SG_THREADS = 256;
constexpr int SG_FWD_GROUPS_PER_CU = 8;
constexpr int SG_BWD_GROUPS_PER_CU = 2;   // ~230 VGPRs at CL = 32: two wavefronts per SIMD, i.e. two workgroups per CU
constexpr double SG_TWO_PI = 6.283185307179586476925286766559;

// exp and 1/sqrt: the hardware's v_exp_f32 (2^x, 1 ulp) and v_rsq_f32 (1 ulp) in f32; libm in f64
__device__ __forceinline__ float sg_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
__device__ __forceinline__ double sg_exp(double x) { return exp(x); }
__device__ __forceinline__ float sg_rsqrt(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ double sg_rsqrt(double x) { return 1.0 / sqrt(x); }

// Small um: G = 2 e^-lm sinh(um) / um and G'(um) / um = 2 e^-lm (um cosh um - sinh um) / um^3 lose all but a few bits to
// cancellation in the exponential form (E - E2 and (E + E2) - G are differences of nearly equal terms: a relative error of
// ~eps / um^2 in the gradient).  Below um = 1 both are their Taylor series in y = um^2, whose terms are all positive:
//     sinh(x) / x = sum_k x^2k / (2k + 1)!,     (x cosh x - sinh x) / x^3 = sum_k (2k + 2) x^2k / (2k + 3)!
// truncated where the next term is below the type's epsilon at y = 1.
__device__ __forceinline__ float sg_sinhc_series(float y) {
  float p = 1.f / 39916800.f;
  p = fma(p, y, 1.f / 362880.f);
  p = fma(p, y, 1.f / 5040.f);
  p = fma(p, y, 1.f / 120.f);
  p = fma(p, y, 1.f / 6.f);
  return fma(p, y, 1.f);
}
__device__ __forceinline__ float sg_dsinhc_series(float y) {
  float p = 1.f / 518918400.f;
  p = fma(p, y, 1.f / 3991680.f);
  p = fma(p, y, 1.f / 45360.f);
  p = fma(p, y, 1.f / 840.f);
  p = fma(p, y, 1.f / 30.f);
  return fma(p, y, 1.f / 3.f);
}
__device__ __forceinline__ double sg_sinhc_series(double y) {
  double p = 1. / 121645100408832000.;
  p = fma(p, y, 1. / 355687428096000.);
  p = fma(p, y, 1. / 1307674368000.);
  p = fma(p, y, 1. / 6227020800.);
  p = fma(p, y, 1. / 39916800.);
  p = fma(p, y, 1. / 362880.);
  p = fma(p, y, 1. / 5040.);
  p = fma(p, y, 1. / 120.);
  p = fma(p, y, 1. / 6.);
  return fma(p, y, 1.);
}
__device__ __forceinline__ double sg_dsinhc_series(double y) {
  double p = 20. / 51090942171709440000.;
  p = fma(p, y, 18. / 121645100408832000.);
  p = fma(p, y, 16. / 355687428096000.);
  p = fma(p, y, 14. / 1307674368000.);
  p = fma(p, y, 1. / 518918400.);
  p = fma(p, y, 1. / 3991680.);
  p = fma(p, y, 1. / 45360.);
  p = fma(p, y, 1. / 840.);
  p = fma(p, y, 1. / 30.);
  return fma(p, y, 1. / 3.);
}

// the pair's G (without 2 pi) and G'(um) / um; v = s_i d_i + s_j d_j.  The series branch is taken only by wavefronts with a
// lane at 0 < um < 1 (rare in shading: um >= |s_light - 2.133| for unit normals and lights).  um == 0 is left to the
// exponential form, which yields inf / NaN there as the reference does.  For that to be the same pairs as in the reference,
// v is the sum of the two ROUNDED products s_i d_i and s_j d_j (no fma): a lobe that is the exact mirror image of a light
// then gives v == 0 exactly, where an fma leaves the rounding residue of s_i d_i (um ~ 1e-8 s) and a finite result.
template <typename T>
__device__ __forceinline__ void sg_pair(T vx, T vy, T vz, T lm, T& G, T& dG_over_um) {
  const T um2 = fma(vz, vz, fma(vy, vy, vx * vx));
  const T r = sg_rsqrt(um2);
  const T um = um2 * r;
  const T E = sg_exp(um - lm), E2 = sg_exp(-um - lm);
  G = (E - E2) * r;
  dG_over_um = ((E + E2) - G) * r * r;
  const bool small = um2 > (T)0 && um2 < (T)1;
  if (__any(small)) {
    const T E0 = (T)2 * sg_exp(-lm);
    if (small) {
      G = E0 * sg_sinhc_series(um2);
      dG_over_um = E0 * sg_dsinhc_series(um2);
    }
  }
}

template <typename T>
__device__ __forceinline__ T sg_wave_sum(T x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

template <typename T, bool CONST_LOBE>
__global__ __launch_bounds__(SG_THREADS) void sg_reduced_forward_kernel(long long N, int M, const T* __restrict__ amp,
                                                                        const T* __restrict__ dir, const T* __restrict__ sharp,
                                                                        T lobe_amp, T lobe_sharp, const T* __restrict__ oamp,
                                                                        const T* __restrict__ odir,
                                                                        const T* __restrict__ osharp, T* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * SG_THREADS + threadIdx.x; i < N; i += (long long)gridDim.x * SG_THREADS) {
    const T dx = dir[i * 3 + 0], dy = dir[i * 3 + 1], dz = dir[i * 3 + 2];
    const T s = CONST_LOBE ? lobe_sharp : sharp[i];
    const T px = s * dx, py = s * dy, pz = s * dz;
    T ax = 0, ay = 0, az = 0;
    for (int j = 0; j < M; ++j) {   // wave-uniform, in order
      const T sj = osharp[j];
      T G, dG;
      sg_pair<T>(px + sj * odir[j * 3 + 0], py + sj * odir[j * 3 + 1], pz + sj * odir[j * 3 + 2], s + sj, G, dG);
      ax = fma(oamp[j * 3 + 0], G, ax);
      ay = fma(oamp[j * 3 + 1], G, ay);
      az = fma(oamp[j * 3 + 2], G, az);
    }
    const T tp = (T)SG_TWO_PI;
    if (CONST_LOBE) {
      const T k = tp * lobe_amp;
      out[i * 3 + 0] = k * ax;
      out[i * 3 + 1] = k * ay;
      out[i * 3 + 2] = k * az;
    } else {
      out[i * 3 + 0] = tp * amp[i * 3 + 0] * ax;
      out[i * 3 + 1] = tp * amp[i * 3 + 1] * ay;
      out[i * 3 + 2] = tp * amp[i * 3 + 2] * az;
    }
  }
}

// partial: (gridDim.x, M, 6) -- per workgroup and light {A_j xyz, Q_j xyz}.  Row gradients: written in the last chunk; before
// it, grad_amp holds the row's sum_j a_j G and grad_dir its Qr (the constant lobe needs only Qr).
template <typename T, bool CONST_LOBE, int CL>
__global__ __launch_bounds__(SG_THREADS) void sg_reduced_backward_kernel(
    long long N, int M, const T* __restrict__ grad_out, const T* __restrict__ amp, const T* __restrict__ dir,
    const T* __restrict__ sharp, T lobe_amp, T lobe_sharp, const T* __restrict__ oamp, const T* __restrict__ odir,
    const T* __restrict__ osharp, T* __restrict__ partial, T* __restrict__ g_amp, T* __restrict__ g_dir,
    T* __restrict__ g_sharp) {
  __shared__ T red[SG_THREADS / 64][CL * 6];
  const int nchunks = (M + CL - 1) / CL;
  const T tp = (T)SG_TWO_PI;
  for (int c = 0; c < nchunks; ++c) {
    const int j0 = c * CL, cn = min(CL, M - j0);
    const bool first = c == 0, last = c == nchunks - 1;
    T cA[CL][3], cQ[CL][3];
#pragma unroll
    for (int jj = 0; jj < CL; ++jj)
#pragma unroll
      for (int k = 0; k < 3; ++k) cA[jj][k] = cQ[jj][k] = 0;

    for (long long i = (long long)blockIdx.x * SG_THREADS + threadIdx.x; i < N; i += (long long)gridDim.x * SG_THREADS) {
      const T gx = grad_out[i * 3 + 0], gy = grad_out[i * 3 + 1], gz = grad_out[i * 3 + 2];
      const T dx = dir[i * 3 + 0], dy = dir[i * 3 + 1], dz = dir[i * 3 + 2];
      const T s = CONST_LOBE ? lobe_sharp : sharp[i];
      const T aix = CONST_LOBE ? lobe_amp : amp[i * 3 + 0];
      const T aiy = CONST_LOBE ? lobe_amp : amp[i * 3 + 1];
      const T aiz = CONST_LOBE ? lobe_amp : amp[i * 3 + 2];
      const T px = s * dx, py = s * dy, pz = s * dz;
      const T gax = gx * aix, gay = gy * aiy, gaz = gz * aiz;
      T rx = 0, ry = 0, rz = 0;      // sum_j a_j G     (general lobe only)
      T qx = 0, qy = 0, qz = 0;      // sum_j q v
      if (!first) {
        if (!CONST_LOBE) {
          rx = g_amp[i * 3 + 0];
          ry = g_amp[i * 3 + 1];
          rz = g_amp[i * 3 + 2];
        }
        qx = g_dir[i * 3 + 0];
        qy = g_dir[i * 3 + 1];
        qz = g_dir[i * 3 + 2];
      }
#pragma unroll
      for (int jj = 0; jj < CL; ++jj) {
        if (jj < cn) {   // wave-uniform
          const int j = j0 + jj;
          const T sj = osharp[j];
          const T ajx = oamp[j * 3 + 0], ajy = oamp[j * 3 + 1], ajz = oamp[j * 3 + 2];
          const T vx = px + sj * odir[j * 3 + 0], vy = py + sj * odir[j * 3 + 1], vz = pz + sj * odir[j * 3 + 2];
          T G, dG;
          sg_pair<T>(vx, vy, vz, s + sj, G, dG);
          const T h = fma(gaz, ajz, fma(gay, ajy, gax * ajx));
          const T q = h * dG;
          if (!CONST_LOBE) {
            rx = fma(ajx, G, rx);
            ry = fma(ajy, G, ry);
            rz = fma(ajz, G, rz);
          }
          qx = fma(q, vx, qx);
          qy = fma(q, vy, qy);
          qz = fma(q, vz, qz);
          cA[jj][0] = fma(gax, G, cA[jj][0]);
          cA[jj][1] = fma(gay, G, cA[jj][1]);
          cA[jj][2] = fma(gaz, G, cA[jj][2]);
          cQ[jj][0] = fma(q, vx, cQ[jj][0]);
          cQ[jj][1] = fma(q, vy, cQ[jj][1]);
          cQ[jj][2] = fma(q, vz, cQ[jj][2]);
        }
      }
      if (last) {
        const T ks = tp * s;
        g_dir[i * 3 + 0] = ks * qx;
        g_dir[i * 3 + 1] = ks * qy;
        g_dir[i * 3 + 2] = ks * qz;
        if (!CONST_LOBE) {
          g_amp[i * 3 + 0] = tp * gx * rx;
          g_amp[i * 3 + 1] = tp * gy * ry;
          g_amp[i * 3 + 2] = tp * gz * rz;
          const T qd = fma(qz, dz, fma(qy, dy, qx * dx)), gr = fma(gaz, rz, fma(gay, ry, gax * rx));
          g_sharp[i] = tp * (qd - gr);
        }
      } else {
        if (!CONST_LOBE) {
          g_amp[i * 3 + 0] = rx;
          g_amp[i * 3 + 1] = ry;
          g_amp[i * 3 + 2] = rz;
        }
        g_dir[i * 3 + 0] = qx;
        g_dir[i * 3 + 1] = qy;
        g_dir[i * 3 + 2] = qz;
      }
    }

    // this workgroup's column sums of the chunk: wavefront, then the four wavefronts in order
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int jj = 0; jj < CL; ++jj) {
      if (jj < cn) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const T a = sg_wave_sum(cA[jj][k]), q = sg_wave_sum(cQ[jj][k]);
          if (lane == 0) {
            red[wave][jj * 6 + k] = a;
            red[wave][jj * 6 + 3 + k] = q;
          }
        }
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < cn * 6) {
      T acc = red[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < SG_THREADS / 64; ++w) acc += red[w][threadIdx.x];
      partial[((size_t)blockIdx.x * M + j0) * 6 + threadIdx.x] = acc;
    }
    __syncthreads();
  }
}

// one wavefront per light: the slabs of the `groups` workgroups folded in a fixed order, then the column gradients
template <typename T>
__global__ __launch_bounds__(64) void sg_reduced_fold_kernel(int groups, int M, const T* __restrict__ partial,
                                                             const T* __restrict__ oamp, const T* __restrict__ odir,
                                                             const T* __restrict__ osharp, T* __restrict__ g_oamp,
                                                             T* __restrict__ g_odir, T* __restrict__ g_osharp) {
  const int j = blockIdx.x, lane = threadIdx.x;
  T v[6] = {0, 0, 0, 0, 0, 0};
  for (int b = lane; b < groups; b += 64) {
    const T* p = partial + ((size_t)b * M + j) * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] += p[k];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = sg_wave_sum(v[k]);
  if (lane == 0) {
    const T tp = (T)SG_TWO_PI;
    const T ax = oamp[j * 3 + 0], ay = oamp[j * 3 + 1], az = oamp[j * 3 + 2];
    const T dx = odir[j * 3 + 0], dy = odir[j * 3 + 1], dz = odir[j * 3 + 2];
    const T sj = osharp[j];
    g_oamp[j * 3 + 0] = tp * v[0];
    g_oamp[j * 3 + 1] = tp * v[1];
    g_oamp[j * 3 + 2] = tp * v[2];
    g_odir[j * 3 + 0] = tp * sj * v[3];
    g_odir[j * 3 + 1] = tp * sj * v[4];
    g_odir[j * 3 + 2] = tp * sj * v[5];
    const T qd = fma(v[5], dz, fma(v[4], dy, v[3] * dx)), aa = fma(v[2], az, fma(v[1], ay, v[0] * ax));
    g_osharp[j] = tp * (qd - aa);
  }
}

// workgroups of the backward launch: a function of the row count only (the slab layout and the fold order follow from it)
static inline int sg_backward_groups(long long N) {
  const long long g = (N + SG_THREADS - 1) / SG_THREADS;
  return (int)(g < (long long)KAMD_NUM_CU * SG_BWD_GROUPS_PER_CU ? g : (long long)KAMD_NUM_CU * SG_BWD_GROUPS_PER_CU);
}

template <typename T>
int sg_forward(hipStream_t st, long long N, int M, const T* amp, const T* dir, const T* sharp, double lobe_amp,
               double lobe_sharp, const T* oamp, const T* odir, const T* osharp, T* out) {
  if (N < 0 || M < 0) return (int)hipErrorInvalidValue;
  if (N == 0 || M == 0) return 0;
  const bool const_lobe = amp == nullptr && sharp == nullptr;
  if (!const_lobe && (amp == nullptr || sharp == nullptr)) return (int)hipErrorInvalidValue;
  long long groups = (N + SG_THREADS - 1) / SG_THREADS;
  if (groups > (long long)KAMD_NUM_CU * SG_FWD_GROUPS_PER_CU) groups = (long long)KAMD_NUM_CU * SG_FWD_GROUPS_PER_CU;
  if (const_lobe)
    hipLaunchKernelGGL((sg_reduced_forward_kernel<T, true>), dim3((unsigned)groups), dim3(SG_THREADS), 0, st, N, M, amp, dir,
                       sharp, (T)lobe_amp, (T)lobe_sharp, oamp, odir, osharp, out);
  else
    hipLaunchKernelGGL((sg_reduced_forward_kernel<T, false>), dim3((unsigned)groups), dim3(SG_THREADS), 0, st, N, M, amp,
                       dir, sharp, (T)0, (T)0, oamp, odir, osharp, out);
  KAMD_RETURN_LAST_ERROR();
}

template <typename T, bool CONST_LOBE, int CL>
void sg_backward_launch(hipStream_t st, int groups, long long N, int M, const T* grad_out, const T* amp, const T* dir,
                        const T* sharp, T lobe_amp, T lobe_sharp, const T* oamp, const T* odir, const T* osharp, T* partial,
                        T* g_amp, T* g_dir, T* g_sharp) {
  hipLaunchKernelGGL((sg_reduced_backward_kernel<T, CONST_LOBE, CL>), dim3(groups), dim3(SG_THREADS), 0, st, N, M, grad_out,
                     amp, dir, sharp, lobe_amp, lobe_sharp, oamp, odir, osharp, partial, g_amp, g_dir, g_sharp);
}

template <typename T, bool CONST_LOBE>
void sg_backward_dispatch(hipStream_t st, int groups, long long N, int M, const T* grad_out, const T* amp, const T* dir,
                          const T* sharp, T lobe_amp, T lobe_sharp, const T* oamp, const T* odir, const T* osharp, T* partial,
                          T* g_amp, T* g_dir, T* g_sharp) {
  // the chunk of lights held in registers: as few as cover M, at most 32 (f32) / 16 (f64) -- 6 CL sums per lane
  constexpr int CL_MAX = sizeof(T) == 4 ? 32 : 16;
  if (M <= 8)
    sg_backward_launch<T, CONST_LOBE, 8>(st, groups, N, M, grad_out, amp, dir, sharp, lobe_amp, lobe_sharp, oamp, odir, osharp,
                                         partial, g_amp, g_dir, g_sharp);
  else if (M <= 16 || CL_MAX == 16)
    sg_backward_launch<T, CONST_LOBE, 16>(st, groups, N, M, grad_out, amp, dir, sharp, lobe_amp, lobe_sharp, oamp, odir,
                                          osharp, partial, g_amp, g_dir, g_sharp);
  else
    sg_backward_launch<T, CONST_LOBE, CL_MAX>(st, groups, N, M, grad_out, amp, dir, sharp, lobe_amp, lobe_sharp, oamp, odir,
                                              osharp, partial, g_amp, g_dir, g_sharp);
}

template <typename T>
int sg_backward(hipStream_t st, long long N, int M, const T* grad_out, const T* amp, const T* dir, const T* sharp,
                double lobe_amp, double lobe_sharp, const T* oamp, const T* odir, const T* osharp, void* workspace, T* g_amp,
                T* g_dir, T* g_sharp, T* g_oamp, T* g_odir, T* g_osharp) {
  if (N < 0 || M < 0) return (int)hipErrorInvalidValue;
  if (N == 0 || M == 0) return 0;
  const bool const_lobe = amp == nullptr && sharp == nullptr;
  if (!const_lobe && (amp == nullptr || sharp == nullptr || g_amp == nullptr || g_sharp == nullptr))
    return (int)hipErrorInvalidValue;
  if (workspace == nullptr || g_dir == nullptr || g_oamp == nullptr || g_odir == nullptr || g_osharp == nullptr)
    return (int)hipErrorInvalidValue;
  const int groups = sg_backward_groups(N);
  T* partial = (T*)workspace;
  if (const_lobe)
    sg_backward_dispatch<T, true>(st, groups, N, M, grad_out, amp, dir, sharp, (T)lobe_amp, (T)lobe_sharp, oamp, odir, osharp,
                                  partial, nullptr, g_dir, nullptr);
  else
    sg_backward_dispatch<T, false>(st, groups, N, M, grad_out, amp, dir, sharp, (T)0, (T)0, oamp, odir, osharp, partial,
                                   g_amp, g_dir, g_sharp);
  KAMD_CHECK(hipGetLastError());
  hipLaunchKernelGGL((sg_reduced_fold_kernel<T>), dim3(M), dim3(64), 0, st, groups, M, (const T*)partial, oamp, odir, osharp,
                     g_oamp, g_odir, g_osharp);
  KAMD_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {

size_t kamd_sg_reduced_inner_product_backward_workspace(int64_t num_sg, int num_other, int elem_size) {
  if (num_sg <= 0 || num_other <= 0 || elem_size <= 0) return 0;
  return (size_t)sg_backward_groups((long long)num_sg) * (size_t)num_other * 6 * (size_t)elem_size;
}

#define KAMD_SG_ENTRY(SFX, T)                                                                                               \
  int kamd_sg_reduced_inner_product_forward_##SFX(void* stream, int64_t num_sg, int num_other, const T* amplitude,          \
                                                  const T* direction, const T* sharpness, double lobe_amplitude,           \
                                                  double lobe_sharpness, const T* other_amplitude,                         \
                                                  const T* other_direction, const T* other_sharpness, T* out) {            \
    return sg_forward<T>((hipStream_t)stream, (long long)num_sg, num_other, amplitude, direction, sharpness,                \
                         lobe_amplitude, lobe_sharpness, other_amplitude, other_direction, other_sharpness, out);          \
  }                                                                                                                         \
  int kamd_sg_reduced_inner_product_backward_##SFX(                                                                        \
      void* stream, int64_t num_sg, int num_other, const T* grad_out, const T* amplitude, const T* direction,              \
      const T* sharpness, double lobe_amplitude, double lobe_sharpness, const T* other_amplitude,                          \
      const T* other_direction, const T* other_sharpness, void* workspace, T* grad_amplitude, T* grad_direction,           \
      T* grad_sharpness, T* grad_other_amplitude, T* grad_other_direction, T* grad_other_sharpness) {                      \
    return sg_backward<T>((hipStream_t)stream, (long long)num_sg, num_other, grad_out, amplitude, direction, sharpness,    \
                          lobe_amplitude, lobe_sharpness, other_amplitude, other_direction, other_sharpness, workspace,    \
                          grad_amplitude, grad_direction, grad_sharpness, grad_other_amplitude, grad_other_direction,      \
                          grad_other_sharpness);                                                                            \
  }
KAMD_SG_ENTRY(f32, float)
KAMD_SG_ENTRY(f64, double)
#undef KAMD_SG_ENTRY

}  // extern "C"
