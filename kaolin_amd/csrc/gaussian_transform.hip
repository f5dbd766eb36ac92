// ops.gaussians.transform_gaussians / transform_shs, forward and backward, ONE kernel launch per direction (the reference is a
// chain of ~40 torch kernels with two scatter_add_ -- float atomics -- that assemble the 5x5 and 7x7 SH rotation matrices,
// kaolin/ops/gaussians/transforms.py).  No atomics, no workspace, no host read: the same bits on every call, capturable.
//
// PER GAUSSIAN, with A = transform[:3, :3], t = transform[:3, 3] (rotation_given: R = the 3x3 matrix as it is, SH only):
//     s_j = sqrt((A0j^2 + A1j^2) + A2j^2)            the column norms                      R_ij = A_ij / s_j
//     positions      ((A_i0 p0 + A_i1 p1) + A_i2 p2) + t_i
//     orientations   r (x) (q / |q|), r = quat(R) by the branch rule of kaolin_amd/math/quat.py, xyzw inside; a wxyz input and
//                    output are reordered.  |q| = sqrt(((x^2 + y^2) + z^2) + w^2)
//     scales         scales * s, or scales * (log(s) / scales + 1)
//     SH             band 0 copied; out_l = D^l in_l per channel, sum over j ascending from the product j = 0
//                    D^1[i][j] = R[perm i][perm j] * sign, perm = (1, 2, 0), sign = (-1)^(i + j)    (the 3DGS convention)
//                    D^2, D^3 = the term lists of sh_rotation_table.h (generated from the Ivanic-Ruedenberg recurrence):
//                    D[m][n] = (...((0 + (c d1) dp) + (c d1) dp) ...), terms in list order, c rounded once to T
//   -ffp-contract=off: one rounding per operation written here, no FMA; tests/gaussian_transforms_bruteforce.py counts them.
// BACKWARD recomputes the matrices from the transform:  grad_sh_l = (D^l)^T g_l (sum over i ascending), grad_positions = A^T g,
//   grad_scales = g s (g itself for log scales: the derivative of scales + log s), grad_orientations = the product's and the
//   normalisation's:  gu = L(r)^T g,  (gu - u (u . gu)) / |q|.  Each gradient only when its pointers are given.  The gradient with
//   respect to the transform is NOT built here (the Python layer runs its torch formulation for such calls).
//
// LANE MAPPING  A thread owns a Gaussian and keeps its matrices in registers (per-Gaussian transform) or reads them from LDS
//   (shared transform: thread 0 of every workgroup builds them ONCE, before the workgroup's loop over its tiles, with the very
//   same operations -- the two paths give the same bits).  The thread moves its own SH row between global memory and a private
//   LDS row with 16-byte accesses at a lane stride of one row (192 bytes at degree 3), rewrites it in place band by band (the
//   band's 3 (2l + 1) inputs in registers), and writes it back.  LDS rows are padded to an ODD number of elements: lane t reading
//   element j of its row hits bank (ROW t + j) mod 64, all different (double: 32 lanes an access, bank pairs from 2 ROW t mod 64, all
//   different too).  No barrier after the matrices.
//   MEASURED against the alternative this file first had -- the workgroup staging the 128 consecutive rows of its tile through LDS
//   with 16-byte loads at a 16-byte lane stride, three barriers a tile: the staged form was SLOWER in every degree-3 shape
//   (N = 2^22, float32, forward: 0.664 ms against 0.574 shared, 0.815 against 0.650 per Gaussian; profiles/
//   gaussian_transforms_time.jsonl, labels staged_rows / direct_rows).  A wavefront's 64 rows are one contiguous 12 KiB: every
//   cache line it touches is used whole, by 12 loads in a row of the same wave, so the strided form costs no memory traffic, and
//   the barriers at 2 waves a SIMD cost more than the tag lookups.  The staged form is deleted.  Several lanes per Gaussian was not
//   built or measured.  Degree 0 (3 elements a row) and the geometry (3 / 4 / 3 elements) are read directly: consecutive lanes
//   read consecutive 12 / 16 bytes.  Offsets are 64-bit.
#include "common.h"
#include "sh_rotation_table.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr int GT_THREADS = 128;
constexpr int GT_BLOCKS_PER_CU = 8;
// the matrices of one transform: A 0..8, t 9..11, column norms 12..14, their logs 15..17, quat(R) xyzw 18..21, D^1 22..30, D^2 31..55,
// D^3 56..104
constexpr int GT_A = 0, GT_T = 9, GT_S = 12, GT_LOG = 15, GT_Q = 18, GT_D1 = 22, GT_D2 = 31, GT_D3 = 56, GT_M = 105;
constexpr int GT_XYZW = 1, GT_LOG_SCALES = 2, GT_ROTATION_GIVEN = 4;

template <typename T>
struct GtArgs {
  long long N;
  const T* tf;
  long long tf_stride, tf_row;
  int flags;
  // forward: the inputs; backward: the gradients of the outputs (each may be NULL) and ori_in, the forward's orientations
  const T* pos;
  const T* ori;
  const T* scl;
  const T* sh;
  const T* ori_in;
  T* o_pos;
  T* o_ori;
  T* o_scl;
  T* o_sh;
  int vec;  // both SH bases are 16-byte aligned
};

__device__ __forceinline__ float gt_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double gt_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float gt_log(float x) { return logf(x); }
__device__ __forceinline__ double gt_log(double x) { return log(x); }

// M <- the matrices of the transform at tf (rows tf_row apart).  geom: A, t, the norms and quat(R) are needed; logs: log(norms)
template <typename T, int DEG>
__device__ __forceinline__ void gt_setup(const T* __restrict__ tf, long long tf_row, bool given, bool geom, bool logs, T* M) {
#pragma unroll
  for (int i = 0; i < GT_M; ++i) M[i] = (T)0;
  T r[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) r[3 * i + j] = tf[i * tf_row + j];
  if (!given) {
#pragma unroll
    for (int i = 0; i < 9; ++i) M[GT_A + i] = r[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const T s = gt_sqrt((r[j] * r[j] + r[3 + j] * r[3 + j]) + r[6 + j] * r[6 + j]);
      M[GT_S + j] = s;
      r[j] = r[j] / s, r[3 + j] = r[3 + j] / s, r[6 + j] = r[6 + j] / s;
    }
    if (geom) {
#pragma unroll
      for (int i = 0; i < 3; ++i) M[GT_T + i] = tf[i * tf_row + 3];
      if (logs) {
#pragma unroll
        for (int j = 0; j < 3; ++j) M[GT_LOG + j] = gt_log(M[GT_S + j]);
      }
      // quat(R), xyzw: the branch names the component that is taken positive
      const T tr = (r[0] + r[4]) + r[8];
      T x, y, z, w;
      if (tr > (T)0) {
        const T s = (T)0.5 / gt_sqrt(tr + (T)1);
        x = (r[7] - r[5]) * s, y = (r[2] - r[6]) * s, z = (r[3] - r[1]) * s, w = (T)0.25 / s;
      } else if (r[0] > r[4] && r[0] > r[8]) {
        const T s = (T)2 * gt_sqrt((((T)1 + r[0]) - r[4]) - r[8]);
        x = (T)0.25 * s, y = (r[1] + r[3]) / s, z = (r[2] + r[6]) / s, w = (r[7] - r[5]) / s;
      } else if (r[4] > r[8]) {
        const T s = (T)2 * gt_sqrt((((T)1 + r[4]) - r[0]) - r[8]);
        x = (r[1] + r[3]) / s, y = (T)0.25 * s, z = (r[5] + r[7]) / s, w = (r[2] - r[6]) / s;
      } else {
        const T s = (T)2 * gt_sqrt((((T)1 + r[8]) - r[0]) - r[4]);
        x = (r[2] + r[6]) / s, y = (r[5] + r[7]) / s, z = (T)0.25 * s, w = (r[3] - r[1]) / s;
      }
      M[GT_Q] = x, M[GT_Q + 1] = y, M[GT_Q + 2] = z, M[GT_Q + 3] = w;
    }
  }
  if constexpr (DEG >= 1) {
    T* d1 = M + GT_D1;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const T v = r[3 * ((i + 1) % 3) + (j + 1) % 3];
        d1[3 * i + j] = ((i + j) & 1) ? -v : v;
      }
    if constexpr (DEG >= 2) {
      T* d2 = M + GT_D2;
#define GT_TERM2(c, m, n, i, j, p, q) d2[(m) * 5 + (n)] = d2[(m) * 5 + (n)] + ((T)(c) * d1[(i) * 3 + (j)]) * d1[(p) * 3 + (q)];
      KAMD_SH_BAND2_TERMS(GT_TERM2)
#undef GT_TERM2
      if constexpr (DEG >= 3) {
        T* d3 = M + GT_D3;
#define GT_TERM3(c, m, n, i, j, p, q) d3[(m) * 7 + (n)] = d3[(m) * 7 + (n)] + ((T)(c) * d1[(i) * 3 + (j)]) * d2[(p) * 5 + (q)];
        KAMD_SH_BAND3_TERMS(GT_TERM3)
#undef GT_TERM3
      }
    }
  }
}

// band L of one row, in place: forward out_i = sum_j D[i][j] in_j, TRANSPOSED out_j = sum_i D[i][j] in_i; per channel
template <typename T, int L, bool TRANSPOSED>
__device__ __forceinline__ void gt_apply(const T* D, T* row) {
  constexpr int K = 2 * L + 1;
  T in[3 * K];
  T* band = row + 3 * L * L;
#pragma unroll
  for (int i = 0; i < 3 * K; ++i) in[i] = band[i];
#pragma unroll
  for (int i = 0; i < K; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      T acc = (TRANSPOSED ? D[i] : D[i * K]) * in[c];
#pragma unroll
      for (int j = 1; j < K; ++j) acc = acc + (TRANSPOSED ? D[j * K + i] : D[i * K + j]) * in[3 * j + c];
      band[3 * i + c] = acc;
    }
}

// quaternion at p (4 elements) -> xyzw
template <typename T>
__device__ __forceinline__ void gt_load_quat(const T* p, bool xyzw, T* q) {
  if (xyzw)
    q[0] = p[0], q[1] = p[1], q[2] = p[2], q[3] = p[3];
  else
    q[0] = p[1], q[1] = p[2], q[2] = p[3], q[3] = p[0];
}
template <typename T>
__device__ __forceinline__ void gt_store_quat(T* p, bool xyzw, const T* q) {
  if (xyzw)
    p[0] = q[0], p[1] = q[1], p[2] = q[2], p[3] = q[3];
  else
    p[1] = q[0], p[2] = q[1], p[3] = q[2], p[0] = q[3];
}
template <typename T>
__device__ __forceinline__ T gt_quat_norm(const T* q) {
  return gt_sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
}

// Gaussian g with the matrices M (registers, or LDS for a shared transform); row: its SH row in LDS (DEG >= 1)
template <typename T, int DEG, bool BWD>
__device__ __forceinline__ void gt_gaussian(const GtArgs<T>& a, long long g, const T* M, T* row) {
  const bool xyzw = (a.flags & GT_XYZW) != 0, logs = (a.flags & GT_LOG_SCALES) != 0;
  if constexpr (!BWD) {
    if (a.pos != nullptr) {
      const T p0 = a.pos[g * 3], p1 = a.pos[g * 3 + 1], p2 = a.pos[g * 3 + 2];
#pragma unroll
      for (int i = 0; i < 3; ++i)
        a.o_pos[g * 3 + i] = ((M[GT_A + 3 * i] * p0 + M[GT_A + 3 * i + 1] * p1) + M[GT_A + 3 * i + 2] * p2) + M[GT_T + i];
      T q[4], o[4];
      gt_load_quat(a.ori + g * 4, xyzw, q);
      const T nq = gt_quat_norm(q);
      const T ux = q[0] / nq, uy = q[1] / nq, uz = q[2] / nq, uw = q[3] / nq;
      const T rx = M[GT_Q], ry = M[GT_Q + 1], rz = M[GT_Q + 2], rw = M[GT_Q + 3];
      o[0] = ((rw * ux + rx * uw) + ry * uz) - rz * uy;
      o[1] = ((rw * uy + ry * uw) + rz * ux) - rx * uz;
      o[2] = ((rw * uz + rz * uw) + rx * uy) - ry * ux;
      o[3] = ((rw * uw - rx * ux) - ry * uy) - rz * uz;
      gt_store_quat(a.o_ori + g * 4, xyzw, o);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const T s = a.scl[g * 3 + j];
        a.o_scl[g * 3 + j] = logs ? s * (M[GT_LOG + j] / s + (T)1) : s * M[GT_S + j];
      }
    }
  } else {
    if (a.o_pos != nullptr) {
      const T g0 = a.pos[g * 3], g1 = a.pos[g * 3 + 1], g2 = a.pos[g * 3 + 2];
#pragma unroll
      for (int j = 0; j < 3; ++j) a.o_pos[g * 3 + j] = (M[GT_A + j] * g0 + M[GT_A + 3 + j] * g1) + M[GT_A + 6 + j] * g2;
    }
    if (a.o_scl != nullptr) {
#pragma unroll
      for (int j = 0; j < 3; ++j) a.o_scl[g * 3 + j] = logs ? a.scl[g * 3 + j] : a.scl[g * 3 + j] * M[GT_S + j];
    }
    if (a.o_ori != nullptr) {
      T q[4], G[4], gu[4], gq[4];
      gt_load_quat(a.ori_in + g * 4, xyzw, q);
      gt_load_quat(a.ori + g * 4, xyzw, G);
      const T nq = gt_quat_norm(q);
      const T u[4] = {q[0] / nq, q[1] / nq, q[2] / nq, q[3] / nq};
      const T rx = M[GT_Q], ry = M[GT_Q + 1], rz = M[GT_Q + 2], rw = M[GT_Q + 3];
      gu[0] = ((rw * G[0] + rz * G[1]) - ry * G[2]) - rx * G[3];
      gu[1] = ((rw * G[1] - rz * G[0]) + rx * G[2]) - ry * G[3];
      gu[2] = ((rw * G[2] + ry * G[0]) - rx * G[1]) - rz * G[3];
      gu[3] = ((rw * G[3] + rx * G[0]) + ry * G[1]) + rz * G[2];
      const T dot = ((u[0] * gu[0] + u[1] * gu[1]) + u[2] * gu[2]) + u[3] * gu[3];
#pragma unroll
      for (int k = 0; k < 4; ++k) gq[k] = (gu[k] - u[k] * dot) / nq;
      gt_store_quat(a.o_ori + g * 4, xyzw, gq);
    }
  }
  if (a.o_sh != nullptr) {
    if constexpr (DEG == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a.o_sh[g * 3 + c] = a.sh[g * 3 + c];
    }
    if constexpr (DEG >= 1) gt_apply<T, 1, BWD>(M + GT_D1, row);
    if constexpr (DEG >= 2) gt_apply<T, 2, BWD>(M + GT_D2, row);
    if constexpr (DEG >= 3) gt_apply<T, 3, BWD>(M + GT_D3, row);
  }
}

template <typename T>
struct GtVec;
template <>
struct GtVec<float> {
  typedef float4 type;
  static constexpr int N = 4;
};
template <>
struct GtVec<double> {
  typedef double2 type;
  static constexpr int N = 2;
};

// a thread moves its own row between global memory and its LDS row: 16-byte accesses when the base is 16-byte aligned and the row
// is a whole number of them (every row then starts at a multiple of 16 bytes), else element by element
template <typename T, int S3, bool TO_LDS>
__device__ __forceinline__ void gt_own_row(T* __restrict__ p, T* row, bool vec) {
  typedef typename GtVec<T>::type V;
  constexpr int NV = GtVec<T>::N;
  if (vec && S3 % NV == 0) {
#pragma unroll
    for (int v = 0; v < S3 / NV; ++v) {
      union {
        V v;
        T s[NV];
      } x;
      if constexpr (TO_LDS) x.v = ((const V*)p)[v];
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        if constexpr (TO_LDS)
          row[v * NV + k] = x.s[k];
        else
          x.s[k] = row[v * NV + k];
      }
      if constexpr (!TO_LDS) ((V*)p)[v] = x.v;
    }
  } else {
#pragma unroll
    for (int e = 0; e < S3; ++e) {
      if constexpr (TO_LDS)
        row[e] = p[e];
      else
        p[e] = row[e];
    }
  }
}

template <typename T, int DEG, bool SHARED, bool BWD>
__global__ __launch_bounds__(GT_THREADS) void gt_kernel(const GtArgs<T> a) {
  constexpr int S3 = 3 * (DEG + 1) * (DEG + 1);
  constexpr int ROW = S3 | 1;
  constexpr bool HAS_ROWS = DEG >= 1;
  __shared__ T rows[HAS_ROWS ? GT_THREADS * ROW : 1];
  __shared__ T mats[SHARED ? GT_M : 1];
  const bool given = (a.flags & GT_ROTATION_GIVEN) != 0, logs = (a.flags & GT_LOG_SCALES) != 0;
  const bool geom = BWD ? (a.o_pos != nullptr || a.o_ori != nullptr || a.o_scl != nullptr) : a.pos != nullptr;
  const bool with_rows = HAS_ROWS && a.o_sh != nullptr;
  if constexpr (SHARED) {
    if (threadIdx.x == 0) {
      T loc[GT_M];
      gt_setup<T, DEG>(a.tf, a.tf_row, given, geom, logs && !BWD, loc);
#pragma unroll
      for (int i = 0; i < GT_M; ++i) mats[i] = loc[i];
    }
    __syncthreads();
  }
  const long long tiles = (a.N + GT_THREADS - 1) / GT_THREADS;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long g0 = tile * GT_THREADS;
    const long long left = a.N - g0;
    const int nrows = left < GT_THREADS ? (int)left : GT_THREADS;
    T* row = rows + threadIdx.x * ROW;
    if ((int)threadIdx.x < nrows) {
      const long long g = g0 + threadIdx.x;
      if (with_rows) gt_own_row<T, S3, true>(const_cast<T*>(a.sh) + g * S3, row, a.vec != 0);
      if constexpr (SHARED) {
        gt_gaussian<T, DEG, BWD>(a, g, mats, row);
      } else {
        T loc[GT_M];
        gt_setup<T, DEG>(a.tf + g * a.tf_stride, a.tf_row, given, geom, logs && !BWD, loc);
        gt_gaussian<T, DEG, BWD>(a, g, loc, row);
      }
      if (with_rows) gt_own_row<T, S3, false>(a.o_sh + g * S3, row, a.vec != 0);
    }
  }
}

inline bool gt_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename T, bool BWD>
int gt_launch(hipStream_t st, GtArgs<T> a, int degree) {
  const bool given = (a.flags & GT_ROTATION_GIVEN) != 0;
  if (a.N < 0 || a.N > (1ll << 40) || degree < 0 || degree > 3 || (a.flags & ~7) != 0) return (int)hipErrorInvalidValue;
  if ((a.tf_row != 3 && a.tf_row != 4) || (a.tf_stride != 0 && a.tf_stride < 3 * a.tf_row)) return (int)hipErrorInvalidValue;
  if (a.N == 0) return 0;
  if (a.tf == nullptr) return (int)hipErrorInvalidValue;
  if ((a.sh == nullptr) != (a.o_sh == nullptr)) return (int)hipErrorInvalidValue;
  if constexpr (!BWD) {
    const int geom = (a.pos != nullptr) + (a.ori != nullptr) + (a.scl != nullptr) + (a.o_pos != nullptr) + (a.o_ori != nullptr) +
                     (a.o_scl != nullptr);
    if (geom != 0 && geom != 6) return (int)hipErrorInvalidValue;
    if (geom == 0 && a.sh == nullptr) return 0;
    if (geom != 0 && (given || a.tf_row != 4)) return (int)hipErrorInvalidValue;
  } else {
    if ((a.pos == nullptr) != (a.o_pos == nullptr) || (a.ori == nullptr) != (a.o_ori == nullptr) ||
        (a.scl == nullptr) != (a.o_scl == nullptr))
      return (int)hipErrorInvalidValue;
    if (a.o_ori != nullptr && a.ori_in == nullptr) return (int)hipErrorInvalidValue;
    const bool geom = a.o_pos != nullptr || a.o_ori != nullptr || a.o_scl != nullptr;
    if (!geom && a.sh == nullptr) return 0;
    if (geom && given) return (int)hipErrorInvalidValue;
  }
  if (a.sh == nullptr) degree = 0;
  a.vec = gt_aligned16(a.sh) && gt_aligned16(a.o_sh);
  const long long tiles = (a.N + GT_THREADS - 1) / GT_THREADS;
  const long long cap = (long long)KAMD_NUM_CU * GT_BLOCKS_PER_CU;
  const dim3 grid((unsigned)(tiles < cap ? tiles : cap));
  const bool shared = a.tf_stride == 0;
#define GT_CASE(DEG)                                                                                           \
  case DEG:                                                                                                    \
    if (shared)                                                                                                \
      hipLaunchKernelGGL((gt_kernel<T, DEG, true, BWD>), grid, dim3(GT_THREADS), 0, st, a);                    \
    else                                                                                                       \
      hipLaunchKernelGGL((gt_kernel<T, DEG, false, BWD>), grid, dim3(GT_THREADS), 0, st, a);                   \
    break;
  switch (degree) {
    GT_CASE(0)
    GT_CASE(1)
    GT_CASE(2)
    GT_CASE(3)
  }
#undef GT_CASE
  KAMD_RETURN_LAST_ERROR();
}

template <typename T>
int gt_forward(void* stream, int64_t N, int degree, int flags, const T* transform, int64_t transform_stride,
               int64_t transform_row_stride, const T* positions, const T* orientations, const T* scales, const T* sh, T* new_positions,
               T* new_orientations, T* new_scales, T* new_sh) {
  GtArgs<T> a{(long long)N, transform,    (long long)transform_stride, (long long)transform_row_stride, flags, positions,
              orientations, scales,       sh,                          nullptr,                         new_positions,
              new_orientations, new_scales, new_sh, 0};
  return gt_launch<T, false>((hipStream_t)stream, a, degree);
}
template <typename T>
int gt_backward(void* stream, int64_t N, int degree, int flags, const T* transform, int64_t transform_stride,
                int64_t transform_row_stride, const T* orientations, const T* grad_new_positions, const T* grad_new_orientations,
                const T* grad_new_scales, const T* grad_new_sh, T* grad_positions, T* grad_orientations, T* grad_scales, T* grad_sh) {
  GtArgs<T> a{(long long)N,          transform,       (long long)transform_stride, (long long)transform_row_stride, flags,
              grad_new_positions,    grad_new_orientations, grad_new_scales,       grad_new_sh,                     orientations,
              grad_positions,        grad_orientations, grad_scales,               grad_sh,                         0};
  return gt_launch<T, true>((hipStream_t)stream, a, degree);
}

}  // namespace

extern "C" {
int kamd_gaussian_transform_forward_f32(void* stream, int64_t N, int degree, int flags, const float* transform, int64_t transform_stride,
                                        int64_t transform_row_stride, const float* positions, const float* orientations,
                                        const float* scales, const float* sh, float* new_positions, float* new_orientations,
                                        float* new_scales, float* new_sh) {
  return gt_forward<float>(stream, N, degree, flags, transform, transform_stride, transform_row_stride, positions, orientations, scales,
                           sh, new_positions, new_orientations, new_scales, new_sh);
}
int kamd_gaussian_transform_forward_f64(void* stream, int64_t N, int degree, int flags, const double* transform, int64_t transform_stride,
                                        int64_t transform_row_stride, const double* positions, const double* orientations,
                                        const double* scales, const double* sh, double* new_positions, double* new_orientations,
                                        double* new_scales, double* new_sh) {
  return gt_forward<double>(stream, N, degree, flags, transform, transform_stride, transform_row_stride, positions, orientations, scales,
                            sh, new_positions, new_orientations, new_scales, new_sh);
}
int kamd_gaussian_transform_backward_f32(void* stream, int64_t N, int degree, int flags, const float* transform, int64_t transform_stride,
                                         int64_t transform_row_stride, const float* orientations, const float* grad_new_positions,
                                         const float* grad_new_orientations, const float* grad_new_scales, const float* grad_new_sh,
                                         float* grad_positions, float* grad_orientations, float* grad_scales, float* grad_sh) {
  return gt_backward<float>(stream, N, degree, flags, transform, transform_stride, transform_row_stride, orientations,
                            grad_new_positions, grad_new_orientations, grad_new_scales, grad_new_sh, grad_positions, grad_orientations,
                            grad_scales, grad_sh);
}
int kamd_gaussian_transform_backward_f64(void* stream, int64_t N, int degree, int flags, const double* transform, int64_t transform_stride,
                                         int64_t transform_row_stride, const double* orientations, const double* grad_new_positions,
                                         const double* grad_new_orientations, const double* grad_new_scales, const double* grad_new_sh,
                                         double* grad_positions, double* grad_orientations, double* grad_scales, double* grad_sh) {
  return gt_backward<double>(stream, N, degree, flags, transform, transform_stride, transform_row_stride, orientations,
                             grad_new_positions, grad_new_orientations, grad_new_scales, grad_new_sh, grad_positions, grad_orientations,
                             grad_scales, grad_sh);
}
}
