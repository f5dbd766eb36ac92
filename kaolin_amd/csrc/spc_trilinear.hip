// ops.spc feature grids: the dual octree (the hierarchy of voxel corners), the trinkets (the 8 corner indices and the parent of
// every voxel) and trilinear interpolation of corner features with both of its gradients ("SPC feature grids").
//
// Replaces kaolin/ops/spc/spc.py:343-490 (make_dual: a host loop over the levels with unique + argsort; make_trinkets: Python
// dictionaries of Morton codes), kaolin/ops/spc/points.py:172-341 (the interpolation's backward: a chain of torch operators) and
// kaolin/csrc/ops/spc/point_utils_cuda.cu:44-124 (the forward: one thread per sample looping over the feature dimension).  Here:
//   * make_dual: ALL levels in one pass -- one key `level << 48 | Morton(corner)` per (point, corner), the keys-only radix sort of
//     sort_scan.h over the 3 (max_level + 1) code bits and then the level bits, heads / scan, the level starts found by max_level + 2
//     binary searches on the device, ONE host read of them; a second entry point decodes the run heads to int16 rows;
//   * make_trinkets: one launch, a thread per (point, corner) searches the corner's code in its level's sorted dual range; the
//     thread of corner 0 also searches the parent `point >> 1` in the previous primary level.  Not found -> -1, never a read
//     outside a range;
//   * interpolation: lanes run along the feature dimension; a group of G = 2^k lanes (G = 64 at most) shares a sample (forward,
//     gradient by coords) or a voxel (gradient by feats), so that a corner gather, a store or an atomic add is one contiguous row
//     segment per group.  The forward takes 4 features a lane when D is a multiple of 4 (D = 16: 4 lanes a sample, 16 samples a
//     wavefront).  The lanes of a group read pidx, the point and the 8 trinkets at the same addresses: one request per group.
//     A pidx outside [0, num_points) or a trinket outside [0, num_feats) makes the sample a miss: zeros, nothing read or added.
// Arithmetic (the torch formulation repeats it operation by operation; the library is built without contraction): the local
// coordinate u = 2^level (c / 2 + 1 / 2) - p in double, rounded to float; 1 - u in double from the rounded u, rounded to float;
// the coefficients are float products (x y) z; the 8 products feat * coeff are added in corner order, in float (half and float
// features) or double (double features), and rounded once.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "common.h"
#include "sort_scan.h"
#include "spc_octree.h"
#include "spc_dual_host.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr unsigned long long SD_CODE_MASK = (1ull << SD_LEVEL_SHIFT) - 1ull;

inline unsigned sd_grid(int64_t items) {  // grid-stride kernels of 256 threads
  int64_t g = items > 0 ? (items + 255) / 256 : 1;
  if (g > (int64_t)KAMD_NUM_CU * 16) g = (int64_t)KAMD_NUM_CU * 16;
  return (unsigned)g;
}

// the level of point i and the [begin, end) of that level in `lv` -- a chain of compares on kernel arguments, no indexed access
__device__ __forceinline__ int sd_level_of(const SdLevels& lv, long long i) {
  int level = 0;
#pragma unroll
  for (int l = 1; l <= SD_MAX_LEVEL; ++l)
    if (l <= lv.max_level && i >= lv.first[l]) level = l;
  return level;
}
__device__ __forceinline__ void sd_range_of(const SdLevels& lv, int level, long long* begin, long long* end) {
  long long b = lv.first[0], e = lv.first[1];
#pragma unroll
  for (int l = 1; l <= SD_MAX_LEVEL; ++l)
    if (l == level) b = lv.first[l], e = lv.first[l + 1];
  *begin = b, *end = e;
}

// ---- make_dual -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sd_corner_keys_kernel(long long n, SdLevels lv, const int16_t* __restrict__ points,
                                                             unsigned long long* __restrict__ keys) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < 8 * n; e += (long long)gridDim.x * 256) {
    const long long i = e >> 3;
    const int j = (int)(e & 7);
    const unsigned long long level = (unsigned long long)sd_level_of(lv, i);
    const int x = points[3 * i] + (j >> 2), y = points[3 * i + 1] + ((j >> 1) & 1), z = points[3 * i + 2] + (j & 1);
    keys[e] = (level << SD_LEVEL_SHIFT) | ms_to_morton(x, y, z);  // the low 15 bits of a corner: 2^14 at level 14
  }
}
// thread l <= max_level: the first sorted key of level l or above, as a rank among the run heads (pos) -- the level's first dual
// point; thread max_level + 1: the number of dual points.  An empty level gets the start of the next one.
__global__ __launch_bounds__(64) void sd_level_starts_kernel(long long nk, int max_level, const unsigned long long* __restrict__ keys,
                                                             const long long* __restrict__ pos, long long* __restrict__ starts) {
  const int l = threadIdx.x;
  if (l > max_level + 1) return;
  long long lo = nk;
  if (l <= max_level) lo = ss_rank(keys, nk, (unsigned long long)l << SD_LEVEL_SHIFT);  // in [0, nk]
  starts[l] = pos[lo];  // pos has nk + 1 entries
}
__global__ __launch_bounds__(256) void sd_decode_kernel(long long nk, long long num_dual, const unsigned long long* __restrict__ keys,
                                                        const int* __restrict__ flags, const long long* __restrict__ pos,
                                                        int16_t* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nk; i += (long long)gridDim.x * 256) {
    if (!flags[i]) continue;
    const long long r = pos[i];
    if (r < 0 || r >= num_dual) continue;  // the row the host sized the result for
    int x, y, z;
    ms_to_point(keys[i] & SD_CODE_MASK, &x, &y, &z);
    out[3 * r] = (int16_t)x, out[3 * r + 1] = (int16_t)y, out[3 * r + 2] = (int16_t)z;
  }
}

struct SdWs {
  long long* sizes;
  unsigned long long *ka, *kb;
  int* flags;
  long long* pos;
  int* hist;
  long long *hoffs, *sums;
};
SdWs sd_ws(void* base, const SdLayout& l) {
  char* p = (char*)base;
  SdWs w;
  w.sizes = (long long*)(p + l.sizes);
  w.ka = (unsigned long long*)(p + l.keys_a);
  w.kb = (unsigned long long*)(p + l.keys_b);
  w.flags = (int*)(p + l.flags);
  w.pos = (long long*)(p + l.pos);
  w.hist = (int*)(p + l.hist);
  w.hoffs = (long long*)(p + l.hoffs);
  w.sums = (long long*)(p + l.sums);
  return w;
}

// ---- make_trinkets ---------------------------------------------------------------------------------------------------------------
// the index in [begin, end) of the point whose Morton code is `code`, -1 when there is none; the range is sorted by code
__device__ __forceinline__ long long sd_find(const int16_t* __restrict__ pts, long long begin, long long end, uint64_t code) {
  long long lo = begin, hi = end;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (ms_to_morton(pts[3 * mid], pts[3 * mid + 1], pts[3 * mid + 2]) < code)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (lo >= end) return -1;
  return ms_to_morton(pts[3 * lo], pts[3 * lo + 1], pts[3 * lo + 2]) == code ? lo : -1;
}
__global__ __launch_bounds__(256) void sd_trinkets_kernel(long long n, long long num_dual, SdLevels prim, SdLevels dual,
                                                          const int16_t* __restrict__ points, const int16_t* __restrict__ points_dual,
                                                          int* __restrict__ trinkets, int* __restrict__ parents) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < 8 * n; e += (long long)gridDim.x * 256) {
    const long long i = e >> 3;
    const int j = (int)(e & 7);
    const int level = sd_level_of(prim, i);
    const int px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
    long long b, en;
    sd_range_of(dual, level, &b, &en);
    b = b < 0 ? 0 : b;
    en = en > num_dual ? num_dual : en;  // the level's range lies inside the dual hierarchy
    const long long at = sd_find(points_dual, b, en, ms_to_morton(px + (j >> 2), py + ((j >> 1) & 1), pz + (j & 1)));
    trinkets[e] = at < 0 ? -1 : (int)(at - b);
    if (j == 0) {
      long long parent = -1;
      if (level > 0) {
        sd_range_of(prim, level - 1, &b, &en);
        b = b < 0 ? 0 : b;
        en = en > n ? n : en;
        parent = sd_find(points, b, en, ms_to_morton(px >> 1, py >> 1, pz >> 1));
      }
      parents[i] = (int)parent;
    }
  }
}

// ---- interpolation -----------------------------------------------------------------------------------------------------------------
template <typename T> struct SdAcc { typedef float type; };
template <> struct SdAcc<double> { typedef double type; };
__device__ __forceinline__ float sd_ld(const __half* p, int64_t i) { return __half2float(p[i]); }
__device__ __forceinline__ float sd_ld(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ double sd_ld(const double* p, int64_t i) { return p[i]; }
__device__ __forceinline__ void sd_st(__half* p, int64_t i, float v) { p[i] = __float2half(v); }
__device__ __forceinline__ void sd_st(float* p, int64_t i, float v) { p[i] = v; }
__device__ __forceinline__ void sd_st(double* p, int64_t i, double v) { p[i] = v; }

template <typename T> struct alignas(4 * sizeof(T)) SdVec4 { T v[4]; };

// u = 2^level (c / 2 + 1 / 2) - p and 1 - u of one axis
__device__ __forceinline__ void sd_local(float c, int p, int level, float* u, float* v) {
  *u = (float)((double)(1 << level) * ((double)c * 0.5 + 0.5) - (double)p);
  *v = (float)(1.0 - (double)*u);
}
// c000, c001, ..., c111: z fastest, the corner order of points_to_corners
__device__ __forceinline__ void sd_coeffs(const float* u, const float* v, float* c) {
  c[0] = (v[0] * v[1]) * v[2];
  c[1] = (v[0] * v[1]) * u[2];
  c[2] = (v[0] * u[1]) * v[2];
  c[3] = (v[0] * u[1]) * u[2];
  c[4] = (u[0] * v[1]) * v[2];
  c[5] = (u[0] * v[1]) * u[2];
  c[6] = (u[0] * u[1]) * v[2];
  c[7] = (u[0] * u[1]) * u[2];
}
// the voxel of a sample: its point and its 8 trinkets, or a miss.  Every lane of a group reads the same addresses.
struct SdVoxel {
  bool hit;
  int p[3];
  int t[8];
};
__device__ __forceinline__ SdVoxel sd_voxel(int64_t voxel, bool in_range, int64_t num_points, int64_t num_feats,
                                           const int* __restrict__ pidx, const int16_t* __restrict__ points,
                                           const int* __restrict__ trinkets) {
  SdVoxel x;
  x.hit = false;
  if (!in_range) return x;
  const int64_t pi = pidx[voxel];
  if (pi < 0 || pi >= num_points) return x;  // -1, or an index that is not a point
  const int4 lo = ((const int4*)(trinkets + 8 * pi))[0], hi = ((const int4*)(trinkets + 8 * pi))[1];
  x.t[0] = lo.x, x.t[1] = lo.y, x.t[2] = lo.z, x.t[3] = lo.w, x.t[4] = hi.x, x.t[5] = hi.y, x.t[6] = hi.z, x.t[7] = hi.w;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) ok = ok && x.t[k] >= 0 && (int64_t)x.t[k] < num_feats;  // a trinket that is not a feature row
  x.p[0] = points[3 * pi], x.p[1] = points[3 * pi + 1], x.p[2] = points[3 * pi + 2];
  x.hit = ok;
  return x;
}

// half and float coordinates take the interpolation's arithmetic; double coordinates keep every step in double
template <typename T>
__global__ __launch_bounds__(256) void sd_coeffs_kernel(int64_t n, int level, const T* __restrict__ coords,
                                                        const int16_t* __restrict__ points, T* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    if constexpr (sizeof(T) == 8) {
      double u[3], v[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        u[a] = (double)(1 << level) * (coords[3 * i + a] * 0.5 + 0.5) - (double)points[3 * i + a];
        v[a] = 1.0 - u[a];
      }
      out[8 * i] = (v[0] * v[1]) * v[2], out[8 * i + 1] = (v[0] * v[1]) * u[2];
      out[8 * i + 2] = (v[0] * u[1]) * v[2], out[8 * i + 3] = (v[0] * u[1]) * u[2];
      out[8 * i + 4] = (u[0] * v[1]) * v[2], out[8 * i + 5] = (u[0] * v[1]) * u[2];
      out[8 * i + 6] = (u[0] * u[1]) * v[2], out[8 * i + 7] = (u[0] * u[1]) * u[2];
    } else {
      float u[3], v[3], c[8];
#pragma unroll
      for (int a = 0; a < 3; ++a) sd_local((float)sd_ld(coords, 3 * i + a), points[3 * i + a], level, &u[a], &v[a]);
      sd_coeffs(u, v, c);
#pragma unroll
      for (int k = 0; k < 8; ++k) sd_st(out, 8 * i + k, c[k]);
    }
  }
}

// forward: group q of G lanes = sample q; lane g takes the features [V (g + G r), V (g + G r) + V) for r = 0, 1, ...
template <typename T, int V>
__global__ __launch_bounds__(256) void sd_interp_forward_kernel(int64_t samples, int64_t S, int64_t D, int lg, int level,
                                                                int64_t num_points, int64_t num_feats,
                                                                const float* __restrict__ coords, const int* __restrict__ pidx,
                                                                const int16_t* __restrict__ points, const int* __restrict__ trinkets,
                                                                const T* __restrict__ feats, T* __restrict__ out) {
  typedef typename SdAcc<T>::type A;
  const int G = 1 << lg;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t q = tid >> lg;  // G = 1 << lg
  const int g = (int)(tid & (G - 1));
  if (q >= samples) return;
  const SdVoxel x = sd_voxel(q / S, true, num_points, num_feats, pidx, points, trinkets);
  float c[8];
  if (x.hit) {
    float u[3], v[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) sd_local(coords[3 * q + a], x.p[a], level, &u[a], &v[a]);
    sd_coeffs(u, v, c);
  }
  for (int64_t d = (int64_t)V * g; d < D; d += (int64_t)V * G) {  // D % V == 0: a lane's V features lie inside the row
    A acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = (A)0;
    if (x.hit) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int64_t at = (int64_t)x.t[k] * D + d;
        if (V == 4) {
          const SdVec4<T> f = *(const SdVec4<T>*)(feats + at);
#pragma unroll
          for (int e = 0; e < V; ++e) {
            const A prod = (A)sd_ld(f.v, e) * (A)c[k];
            acc[e] = k == 0 ? prod : acc[e] + prod;
          }
        } else {
          const A prod = (A)sd_ld(feats, at) * (A)c[k];
          acc[0] = k == 0 ? prod : acc[0] + prod;
        }
      }
    }
    if (V == 4) {
      SdVec4<T> r;
#pragma unroll
      for (int e = 0; e < V; ++e) sd_st(r.v, e, acc[e]);
      *(SdVec4<T>*)(out + q * D + d) = r;
    } else {
      sd_st(out, q * D + d, acc[0]);
    }
  }
}

// gradient by feats: group i of G lanes = voxel i, lane g takes the features g, g + G, ...: the S samples of the voxel share the 8
// destination rows, so their contributions are summed in registers and every row gets one add per feature -- the lanes of a group
// add to consecutive addresses of one row.  B is the buffer's type: float for half and float features, double for double.
template <typename T, typename B>
__global__ __launch_bounds__(256) void sd_interp_backward_feats_kernel(int64_t N, int64_t S, int64_t D, int lg, int level,
                                                                       int64_t num_points, int64_t num_feats,
                                                                       const float* __restrict__ coords, const int* __restrict__ pidx,
                                                                       const int16_t* __restrict__ points,
                                                                       const int* __restrict__ trinkets, const T* __restrict__ grad_out,
                                                                       B* __restrict__ grad_feats) {
  const int G = 1 << lg;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i = tid >> lg;  // G = 1 << lg
  const int g = (int)(tid & (G - 1));
  if (i >= N) return;
  const SdVoxel x = sd_voxel(i, true, num_points, num_feats, pidx, points, trinkets);
  if (!x.hit) return;
  for (int64_t d = g; d < D; d += G) {
    B acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = (B)0;
    for (int64_t s = 0; s < S; ++s) {
      const int64_t q = i * S + s;
      float u[3], v[3], c[8];
#pragma unroll
      for (int a = 0; a < 3; ++a) sd_local(coords[3 * q + a], x.p[a], level, &u[a], &v[a]);
      sd_coeffs(u, v, c);
      const B go = (B)sd_ld(grad_out, q * D + d);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = acc[k] + (B)c[k] * go;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) kamd_atomic_add(grad_feats + (int64_t)x.t[k] * D + d, acc[k]);  // t[k] < num_feats, d < D
  }
}
__global__ __launch_bounds__(256) void sd_to_half_kernel(int64_t n, const float* __restrict__ in, __half* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = __float2half(in[i]);
}

// gradient by coords: group q of G lanes = sample q, lane g takes the features g, g + G, ...; with a_k = the 8 corner features of
// a channel and g its incoming gradient, the lane sums g * d(sum_k a_k c_k)/du over its channels and the group adds the lanes up
// (a butterfly of shuffles inside the group: every lane of a wavefront stays active up to there).  The derivative is the one by
// the LOCAL coordinate u -- the reference's convention.
template <typename T>
__global__ __launch_bounds__(256) void sd_interp_backward_coords_kernel(int64_t samples, int64_t S, int64_t D, int lg, int level,
                                                                        int64_t num_points, int64_t num_feats,
                                                                        const float* __restrict__ coords, const int* __restrict__ pidx,
                                                                        const int16_t* __restrict__ points,
                                                                        const int* __restrict__ trinkets, const T* __restrict__ feats,
                                                                        const T* __restrict__ grad_out, float* __restrict__ grad_coords) {
  typedef typename SdAcc<T>::type A;
  const int G = 1 << lg;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t q = tid >> lg;  // G = 1 << lg
  const int g = (int)(tid & (G - 1));
  const bool in_range = q < samples;
  const SdVoxel x = sd_voxel(in_range ? q / S : 0, in_range, num_points, num_feats, pidx, points, trinkets);
  A sum[3] = {(A)0, (A)0, (A)0};
  if (x.hit) {
    float u[3], v[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) sd_local(coords[3 * q + a], x.p[a], level, &u[a], &v[a]);
    // the weights of the four edges along an axis: products of the other two axes' (1 - u, u)
    const A yz[4] = {(A)(v[1] * v[2]), (A)(v[1] * u[2]), (A)(u[1] * v[2]), (A)(u[1] * u[2])};
    const A xz[4] = {(A)(v[0] * v[2]), (A)(v[0] * u[2]), (A)(u[0] * v[2]), (A)(u[0] * u[2])};
    const A xy[4] = {(A)(v[0] * v[1]), (A)(v[0] * u[1]), (A)(u[0] * v[1]), (A)(u[0] * u[1])};
    for (int64_t d = g; d < D; d += G) {
      A f[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = (A)sd_ld(feats, (int64_t)x.t[k] * D + d);
      const A go = (A)sd_ld(grad_out, q * D + d);
      const A dx = ((f[4] - f[0]) * yz[0] + (f[5] - f[1]) * yz[1]) + ((f[6] - f[2]) * yz[2] + (f[7] - f[3]) * yz[3]);
      const A dy = ((f[2] - f[0]) * xz[0] + (f[3] - f[1]) * xz[1]) + ((f[6] - f[4]) * xz[2] + (f[7] - f[5]) * xz[3]);
      const A dz = ((f[1] - f[0]) * xy[0] + (f[3] - f[2]) * xy[1]) + ((f[5] - f[4]) * xy[2] + (f[7] - f[6]) * xy[3]);
      sum[0] = sum[0] + go * dx;
      sum[1] = sum[1] + go * dy;
      sum[2] = sum[2] + go * dz;
    }
  }
  for (int off = G >> 1; off > 0; off >>= 1) {  // G divides 64: the partners of a lane are lanes of its own group
#pragma unroll
    for (int a = 0; a < 3; ++a) sum[a] = sum[a] + __shfl_xor(sum[a], off, 64);
  }
  if (in_range && g == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) grad_coords[3 * q + a] = (float)sum[a];  // a miss: the zeros it started from
  }
}

// log2 of the lanes per group: the smallest power of two that covers `items` (features, or vectors of 4 features), 64 at most
inline int sd_group_log2(int64_t items) {
  int lg = 0;
  while (lg < 6 && (1ll << lg) < items) ++lg;
  return lg;
}
inline bool sd_bad_interp(int64_t N, int64_t S, int64_t D, int level, int64_t num_points, int64_t num_feats) {
  return N < 0 || S < 1 || D < 1 || level < 0 || level > 15 || num_points < 0 || num_feats < 0 || N > (1ll << 40) / S ||
         D > (1ll << 31) || ((N * S + 3) / 4) > 0x7FFFFFFFll;  // groups of 64 lanes in blocks of 256 stay below 2^31 blocks
}

template <typename T>
int sd_coeffs_launch(void* stream, int64_t n, int level, const void* coords, const int16_t* points, void* out) {
  if (n < 0 || level < 0 || level > 15) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  hipLaunchKernelGGL((sd_coeffs_kernel<T>), dim3(sd_grid(n)), dim3(256), 0, (hipStream_t)stream, n, level, (const T*)coords, points,
                     (T*)out);
  KAMD_RETURN_LAST_ERROR();
}
template <typename T>
int sd_forward(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points, int64_t num_feats, const float* coords,
               const int32_t* pidx, const int16_t* points, const int32_t* trinkets, const void* feats, void* out) {
  if (sd_bad_interp(N, S, D, level, num_points, num_feats)) return (int)hipErrorInvalidValue;
  const int64_t samples = N * S;
  if (samples == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  // 4 features a lane need rows and bases that are whole vectors
  const bool vec = D % 4 == 0 && ((uintptr_t)feats % (4 * sizeof(T))) == 0 && ((uintptr_t)out % (4 * sizeof(T))) == 0;
  const int lg = sd_group_log2(vec ? D / 4 : D);
  const unsigned blocks = (unsigned)(((samples << lg) + 255) / 256);
  if (vec)
    hipLaunchKernelGGL((sd_interp_forward_kernel<T, 4>), dim3(blocks), dim3(256), 0, st, samples, S, D, lg, level, num_points,
                       num_feats, coords, pidx, points, trinkets, (const T*)feats, (T*)out);
  else
    hipLaunchKernelGGL((sd_interp_forward_kernel<T, 1>), dim3(blocks), dim3(256), 0, st, samples, S, D, lg, level, num_points,
                       num_feats, coords, pidx, points, trinkets, (const T*)feats, (T*)out);
  KAMD_RETURN_LAST_ERROR();
}
template <typename T, typename B>
int sd_backward_feats(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points, int64_t num_feats,
                      const float* coords, const int32_t* pidx, const int16_t* points, const int32_t* trinkets, const void* grad_out,
                      B* grad_feats) {
  if (sd_bad_interp(N, S, D, level, num_points, num_feats)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  KAMD_CHECK(kamd_zero_async(grad_feats, (size_t)num_feats * (size_t)D * sizeof(B), st));
  if (N == 0 || num_feats == 0) return 0;
  const int lg = sd_group_log2(D);
  hipLaunchKernelGGL((sd_interp_backward_feats_kernel<T, B>), dim3((unsigned)(((N << lg) + 255) / 256)), dim3(256), 0, st, N, S, D, lg,
                     level, num_points, num_feats, coords, pidx, points, trinkets, (const T*)grad_out, grad_feats);
  KAMD_RETURN_LAST_ERROR();
}
template <typename T>
int sd_backward_coords(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points, int64_t num_feats,
                       const float* coords, const int32_t* pidx, const int16_t* points, const int32_t* trinkets, const void* feats,
                       const void* grad_out, float* grad_coords) {
  if (sd_bad_interp(N, S, D, level, num_points, num_feats)) return (int)hipErrorInvalidValue;
  const int64_t samples = N * S;
  if (samples == 0) return 0;
  const int lg = sd_group_log2(D);
  hipLaunchKernelGGL((sd_interp_backward_coords_kernel<T>), dim3((unsigned)(((samples << lg) + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, samples, S, D, lg, level, num_points, num_feats, coords, pidx, points, trinkets,
                     (const T*)feats, (const T*)grad_out, grad_coords);
  KAMD_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {

size_t kamd_spc_dual_workspace(int64_t num_points, int max_level) { return sd_workspace_bytes(num_points, max_level); }

int kamd_spc_dual_build(void* stream, int64_t num_points, int max_level, const int16_t* points, const int64_t* host_first,
                        void* workspace, size_t workspace_bytes, int64_t* host_starts) {
  if (sd_bad_extents(num_points, max_level) || host_first == nullptr || host_starts == nullptr || workspace == nullptr)
    return (int)hipErrorInvalidValue;
  long long first[SD_MAX_LEVEL + 2];
  for (int l = 0; l <= max_level + 1; ++l) first[l] = host_first[l];
  SdLevels lv;
  if (!sd_levels(first, max_level, num_points, &lv)) return (int)hipErrorInvalidValue;
  const SdLayout lay = sd_layout(num_points);
  if (workspace_bytes < lay.bytes) return (int)hipErrorInvalidValue;
  const SdWs w = sd_ws(workspace, lay);
  hipStream_t st = (hipStream_t)stream;
  const long long nk = lay.keys;
  hipLaunchKernelGGL(sd_corner_keys_kernel, dim3(sd_grid(nk)), dim3(256), 0, st, (long long)num_points, lv, points, w.ka);
  const bool in_b = sd_sorted_in_b(max_level);  // (kamd_spc_dual_emit looks there too)
  unsigned long long* sorted = in_b ? w.kb : w.ka;
  KAMD_CHECK(ss_sort(st, nk, sd_passes(max_level), w.ka, in_b ? w.ka : w.kb, sorted, ss_sort_ws(w.hist, w.hoffs, w.sums)));
  KAMD_CHECK(ss_heads_scan(st, nk, (const long long*)nullptr, sorted, 0, w.flags, w.pos, w.sums));
  hipLaunchKernelGGL(sd_level_starts_kernel, dim3(1), dim3(64), 0, st, nk, max_level, (const unsigned long long*)sorted,
                     (const long long*)w.pos, w.sizes);
  KAMD_CHECK(hipGetLastError());
  // the one host read of the call: the level starts size the result and are the dual pyramid
  KAMD_CHECK(hipMemcpyAsync(host_starts, w.sizes, (size_t)(max_level + 2) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  KAMD_CHECK(hipStreamSynchronize(st));
  return 0;
}

int kamd_spc_dual_emit(void* stream, int64_t num_points, int max_level, const void* workspace, int64_t num_dual,
                       int16_t* points_dual) {
  if (sd_bad_extents(num_points, max_level) || workspace == nullptr || num_dual < 0) return (int)hipErrorInvalidValue;
  if (num_dual == 0) return 0;
  const SdLayout lay = sd_layout(num_points);
  const SdWs w = sd_ws(const_cast<void*>(workspace), lay);
  const unsigned long long* sorted = sd_sorted_in_b(max_level) ? w.kb : w.ka;
  hipLaunchKernelGGL(sd_decode_kernel, dim3(sd_grid(lay.keys)), dim3(256), 0, (hipStream_t)stream, lay.keys, (long long)num_dual,
                     sorted, (const int*)w.flags, (const long long*)w.pos, points_dual);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spc_trinkets(void* stream, int64_t num_points, int64_t num_dual, int max_level, const int16_t* points,
                      const int16_t* points_dual, const int64_t* host_first, const int64_t* host_first_dual, int32_t* trinkets,
                      int32_t* parents) {
  if (sd_bad_extents(num_points, max_level) || num_dual < 0 || host_first == nullptr || host_first_dual == nullptr)
    return (int)hipErrorInvalidValue;
  long long first[SD_MAX_LEVEL + 2], first_dual[SD_MAX_LEVEL + 2];
  for (int l = 0; l <= max_level + 1; ++l) first[l] = host_first[l], first_dual[l] = host_first_dual[l];
  SdLevels prim, dual;
  if (!sd_levels(first, max_level, num_points, &prim) || !sd_levels(first_dual, max_level, num_dual, &dual))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(sd_trinkets_kernel, dim3(sd_grid(8 * num_points)), dim3(256), 0, (hipStream_t)stream, (long long)num_points,
                     (long long)num_dual, prim, dual, points, points_dual, trinkets, parents);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spc_trilinear_coeffs_f16(void* stream, int64_t n, int level, const void* coords, const int16_t* points, void* coeffs) {
  return sd_coeffs_launch<__half>(stream, n, level, coords, points, coeffs);
}
int kamd_spc_trilinear_coeffs_f32(void* stream, int64_t n, int level, const float* coords, const int16_t* points, float* coeffs) {
  return sd_coeffs_launch<float>(stream, n, level, coords, points, coeffs);
}
int kamd_spc_trilinear_coeffs_f64(void* stream, int64_t n, int level, const double* coords, const int16_t* points, double* coeffs) {
  return sd_coeffs_launch<double>(stream, n, level, coords, points, coeffs);
}

int kamd_spc_interpolate_forward_f16(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points, int64_t num_feats,
                                     const float* coords, const int32_t* pidx, const int16_t* points, const int32_t* trinkets,
                                     const void* feats, void* out) {
  return sd_forward<__half>(stream, N, S, D, level, num_points, num_feats, coords, pidx, points, trinkets, feats, out);
}
int kamd_spc_interpolate_forward_f32(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points, int64_t num_feats,
                                     const float* coords, const int32_t* pidx, const int16_t* points, const int32_t* trinkets,
                                     const float* feats, float* out) {
  return sd_forward<float>(stream, N, S, D, level, num_points, num_feats, coords, pidx, points, trinkets, feats, out);
}
int kamd_spc_interpolate_forward_f64(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points, int64_t num_feats,
                                     const float* coords, const int32_t* pidx, const int16_t* points, const int32_t* trinkets,
                                     const double* feats, double* out) {
  return sd_forward<double>(stream, N, S, D, level, num_points, num_feats, coords, pidx, points, trinkets, feats, out);
}

int kamd_spc_interpolate_backward_feats_f16(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points,
                                            int64_t num_feats, const float* coords, const int32_t* pidx, const int16_t* points,
                                            const int32_t* trinkets, const void* grad_out, float* sums, void* grad_feats) {
  KAMD_CHECK((sd_backward_feats<__half, float>(stream, N, S, D, level, num_points, num_feats, coords, pidx, points, trinkets, grad_out,
                                                sums)));
  const int64_t n = num_feats * D;  // the float sums, rounded once
  if (n == 0) return 0;
  hipLaunchKernelGGL(sd_to_half_kernel, dim3(sd_grid(n)), dim3(256), 0, (hipStream_t)stream, n, (const float*)sums,
                     (__half*)grad_feats);
  KAMD_RETURN_LAST_ERROR();
}
int kamd_spc_interpolate_backward_feats_f32(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points,
                                            int64_t num_feats, const float* coords, const int32_t* pidx, const int16_t* points,
                                            const int32_t* trinkets, const float* grad_out, float* grad_feats) {
  return sd_backward_feats<float, float>(stream, N, S, D, level, num_points, num_feats, coords, pidx, points, trinkets, grad_out,
                                         grad_feats);
}
int kamd_spc_interpolate_backward_feats_f64(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points,
                                            int64_t num_feats, const float* coords, const int32_t* pidx, const int16_t* points,
                                            const int32_t* trinkets, const double* grad_out, double* grad_feats) {
  return sd_backward_feats<double, double>(stream, N, S, D, level, num_points, num_feats, coords, pidx, points, trinkets, grad_out,
                                           grad_feats);
}

int kamd_spc_interpolate_backward_coords_f16(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points,
                                             int64_t num_feats, const float* coords, const int32_t* pidx, const int16_t* points,
                                             const int32_t* trinkets, const void* feats, const void* grad_out, float* grad_coords) {
  return sd_backward_coords<__half>(stream, N, S, D, level, num_points, num_feats, coords, pidx, points, trinkets, feats, grad_out,
                                    grad_coords);
}
int kamd_spc_interpolate_backward_coords_f32(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points,
                                             int64_t num_feats, const float* coords, const int32_t* pidx, const int16_t* points,
                                             const int32_t* trinkets, const float* feats, const float* grad_out, float* grad_coords) {
  return sd_backward_coords<float>(stream, N, S, D, level, num_points, num_feats, coords, pidx, points, trinkets, feats, grad_out,
                                   grad_coords);
}
int kamd_spc_interpolate_backward_coords_f64(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points,
                                             int64_t num_feats, const float* coords, const int32_t* pidx, const int16_t* points,
                                             const int32_t* trinkets, const double* feats, const double* grad_out,
                                             float* grad_coords) {
  return sd_backward_coords<double>(stream, N, S, D, level, num_points, num_feats, coords, pidx, points, trinkets, feats, grad_out,
                                    grad_coords);
}

}  // extern "C"
