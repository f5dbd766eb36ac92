// render.spc: octree ray tracing and the packed ray operators ("SPC ray tracing").
//
// Replaces kaolin/csrc/render/spc/raytrace_cuda.cu:64-269 + :504-626 (decide / scan / subdivide per level, the (ray, node) list written
// and re-read at every level, one blocking read per level) with spc_render_utils.cuh:21-143 (the box test), and :327-502 + :680-802
// (one thread per pack over a `nonzero` index list, channels serially; float atomics in sum_reduce).  Here:
//   * ray tracing: one thread per ray walks its subtree depth-first, twice -- a count launch, the exclusive scan of sort_scan.h
//     (ints -> N + 1 int64 offsets, total in the last slot), ONE host read of the total, an emit launch that repeats the walk and
//     writes at the ray's offset.  4 launches whatever `level` is; no (ray, node) pair ever touches memory.  The depth-first
//     sequence of a ray is the sequence the reference's level-by-level expansion produces for it, and rays come out in input order.
//   * the walk state of a lane is, per level, two words in LDS laid out [level][lane] (conflict-free: the lane is the bank): the
//     node's child base `s`, and its byte | the not-yet-visited children in visit order | the octant code of the ray origin.
//   * packed operators: one thread per (pack, channel), channel fastest, found straight from `boundaries` -- the thread of a
//     pack's first element walks the pack sequentially in index order (reverse: from its end) in the tensor's own dtype.  No
//     index list, no host read, no atomics: scans are graph-capturable and the reductions bit-reproducible.
// The arithmetic of the box test is the contract: float32, every fused multiply-add spelled fmaf, -ffp-contract=off.
// Every data-derived index is compared with the size of the buffer it indexes before use (the list is in DESIGN.md).
#include <hip/hip_runtime.h>
#include "common.h"
#include "sort_scan.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr int RT_MAX_LEVEL = 15;  // KAOLIN_SPC_MAX_LEVELS (spc_math.h:38)
constexpr int RT_BLOCK = 64;      // one wavefront: a workgroup retires with its slowest ray

// the children j of a node in the order of (popcount(j ^ c), j) ascending, 3 bits each, the first in the low bits: the octant of
// the ray origin first, then its three face neighbours, ... (the rule reproduces raytrace_cuda.cu:48-57 exactly)
__host__ __device__ constexpr unsigned rt_order_row(int c) {
  unsigned row = 0;
  int k = 0;
  for (int pc = 0; pc <= 3; ++pc)
    for (int j = 0; j < 8; ++j) {
      const int t = j ^ c;
      if ((t & 1) + ((t >> 1) & 1) + ((t >> 2) & 1) == pc) row |= (unsigned)j << (3 * k++);
    }
  return row;
}

struct RtRay {
  float o[3], d[3], inv[3], sgn[3], half[3];
};

// ray_aabb (spc_render_utils.cuh:47-107) of the box of half width r around the centre that `rel` is relative to; flip = -1 gives
// the exit (the same function with the signs negated, :138-141).  > 0: distance, < 0: the origin is inside, 0: miss.
__device__ __forceinline__ float rt_box(const RtRay& R, const float* rel, float r, float flip) {
  const float cmax = fmaxf(fmaxf(fabsf(rel[0]), fabsf(rel[1])), fabsf(rel[2]));
  if (cmax < r) return -r;
  const float d0 = fmaf(r, flip * R.sgn[0], -rel[0]) * R.inv[0];
  const float d1 = fmaf(r, flip * R.sgn[1], -rel[1]) * R.inv[1];
  const float d2 = fmaf(r, flip * R.sgn[2], -rel[2]) * R.inv[2];
  const bool t0 = d0 >= 0.0f && fabsf(fmaf(R.d[1], d0, rel[1])) <= r && fabsf(fmaf(R.d[2], d0, rel[2])) <= r;
  const bool t1 = d1 >= 0.0f && fabsf(fmaf(R.d[0], d1, rel[0])) <= r && fabsf(fmaf(R.d[2], d1, rel[2])) <= r;
  const bool t2 = d2 >= 0.0f && fabsf(fmaf(R.d[0], d2, rel[0])) <= r && fabsf(fmaf(R.d[1], d2, rel[1])) <= r;
  const float d = t0 ? d0 : (t1 ? d1 : (t2 ? d2 : 0.0f));
  return d != 0.0f ? d : 0.0f;
}

// MODE 0: nuggets only, 1: + entry depth, 2: + entry and exit depth (a hit then also needs exit > 0, raytrace_cuda.cu:215).
// EMIT = false counts the hits of every ray; EMIT = true repeats the walk and writes them at offs[ray].
template <bool EMIT, int MODE>
__global__ __launch_bounds__(RT_BLOCK) void rt_walk_kernel(int64_t N, int level, int64_t num_bytes, int64_t num_points,
                                                           const unsigned char* __restrict__ octree, const int* __restrict__ exsum,
                                                           const int16_t* __restrict__ points, const float* __restrict__ origin,
                                                           const float* __restrict__ direction, int* __restrict__ counts,
                                                           const long long* __restrict__ offs, int64_t total,
                                                           int* __restrict__ nuggets, float* __restrict__ depths) {
  extern __shared__ unsigned s_state[];  // [2 * level][RT_BLOCK]: levels 0 .. level - 1 are descended, `level` is emitted
  __shared__ unsigned s_order[8];
  if (threadIdx.x < 8) s_order[threadIdx.x] = rt_order_row((int)threadIdx.x);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * RT_BLOCK + threadIdx.x;
  if (i >= N) return;
  RtRay R;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    R.o[k] = origin[3 * i + k];
    R.d[k] = direction[3 * i + k];
    R.inv[k] = (float)(1.0 / (double)R.d[k]);         // +-inf for a zero component, on purpose
    R.sgn[k] = signbit(R.d[k]) ? 1.0f : -1.0f;
    R.half[k] = fmaf(0.5f, R.o[k], 0.5f);             // the origin in [0, 1]: what the octant code compares
  }
  unsigned* S = s_state + threadIdx.x;
  int64_t out = 0, end = 0;
  if (EMIT) {
    out = offs[i];
    end = offs[i + 1];
    if (end > total) end = total;                      // the size of nuggets / depths
    if (out < 0) out = end;
  }
  int n = 0, sp = -1, l = 0;
  int64_t cand = 0;                                    // the root: point 0 of level 0
  bool have = num_points > 0;
  for (;;) {
    if (have) {
      have = false;
      const float r = __int_as_float((127 - l) << 23);  // 2^-l
      float rel[3], q[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float p = (float)points[3 * cand + k];   // cand < num_points (checked where it was formed)
        rel[k] = R.o[k] - fmaf(r, fmaf(2.0f, p, 1.0f), -1.0f);
        q[k] = r * (p + 0.5f);                         // exact: 16 bits times a power of two
      }
      const float d = rt_box(R, rel, r, 1.0f);
      if (l == level) {
        bool hit = d > 0.0f;
        float ex = 0.0f;
        if (MODE == 2 && hit) {
          ex = rt_box(R, rel, r, -1.0f);
          hit = ex > 0.0f;
        }
        if (hit) {
          if (EMIT) {
            const int64_t pos = out + n;
            if (pos < end) {
              nuggets[2 * pos] = (int)i;
              nuggets[2 * pos + 1] = (int)cand;
              if (MODE == 1) depths[pos] = d;
              if (MODE == 2) depths[2 * pos] = d, depths[2 * pos + 1] = ex;
            }
          }
          ++n;
        }
      } else if (d != 0.0f && cand < num_bytes) {      // a hit or an origin inside: descend; the node's byte exists
        const unsigned b = octree[cand];
        const unsigned s = cand > 0 ? (unsigned)exsum[cand - 1] : 0u;  // cand - 1 < num_bytes: exsum has num_bytes entries
        // the octant of the origin relative to the node centre: the sign of half - 2^-l (p + 0.5), compared exactly
        const unsigned c = (R.half[0] > q[0] ? 4u : 0u) | (R.half[1] > q[1] ? 2u : 0u) | (R.half[2] > q[2] ? 1u : 0u);
        const unsigned row = s_order[c];
        unsigned pm = 0;                               // bit k: the k-th child in visit order exists
#pragma unroll
        for (int k = 0; k < 8; ++k) pm |= ((b >> ((row >> (3 * k)) & 7u)) & 1u) << k;
        sp = l;                                        // l < level: inside the state
        S[(2 * sp) * RT_BLOCK] = s;
        S[(2 * sp + 1) * RT_BLOCK] = b | (pm << 8) | (c << 16);
      }
    }
    if (sp < 0) break;
    const unsigned word = S[(2 * sp + 1) * RT_BLOCK];
    const unsigned pm = (word >> 8) & 255u;
    if (pm == 0) {
      --sp;
      continue;
    }
    const int k = __ffs((int)pm) - 1;
    S[(2 * sp + 1) * RT_BLOCK] = word & ~(1u << (8 + k));
    const unsigned j = (s_order[(word >> 16) & 7u] >> (3 * k)) & 7u;
    const int64_t child = (int64_t)(int)S[(2 * sp) * RT_BLOCK] + __popc(word & 255u & ((2u << j) - 1u));
    if (child >= 0 && child < num_points) {            // the child's point; a failed guard ends this branch
      cand = child;
      l = sp + 1;
      have = true;
    }
  }
  if (!EMIT) counts[i] = n;
}

// workspace of a trace of N rays: counts (N ints) | offsets (N + 1 int64) | scan sums (int64)
struct RtWs {
  int* counts;
  long long *offs, *sums;
  size_t total_bytes;
};
RtWs rt_ws(void* base, int64_t N) {
  RtWs w;
  char* p = (char*)base;
  auto take = [&](size_t bytes) {
    char* r = p;
    p += (bytes + 255) & ~(size_t)255;
    return r;
  };
  const size_t nn = (size_t)(N > 0 ? N : 1);
  w.counts = (int*)take(nn * 4);
  w.offs = (long long*)take((nn + 1) * 8);
  w.sums = (long long*)take(ss_scan_sums_entries((long long)nn) * 8);
  w.total_bytes = (size_t)(p - (char*)base);
  return w;
}
bool rt_args_ok(int64_t N, int level, int64_t num_bytes, int64_t num_points) {
  return N > 0 && N <= 0x7FFFFFFFLL && level >= 0 && level <= RT_MAX_LEVEL && num_bytes >= 0 && num_points >= 0;
}
size_t rt_lds(int level) { return (size_t)2 * (size_t)(level > 0 ? level : 1) * RT_BLOCK * sizeof(unsigned); }

// ---- packed ray operators --------------------------------------------------------------------------------------------------------
template <bool PROD, typename T>
__device__ __forceinline__ T rp_op(T a, T b) {
  return PROD ? a * b : a + b;
}
// one thread per (element, channel); the threads of a pack's first element do the work.  Element 0 starts a pack whatever
// boundaries[0] says.  cumsum_cuda_kernel / cumprod_cuda_kernel and their reverses (raytrace_cuda.cu:392-502): inclusive copies the
// first element and then out[k] = in[k] op out[k - 1]; exclusive writes the identity first and then out[k] = in[k - 1] op out[k - 1].
template <typename T, bool PROD>
__global__ __launch_bounds__(256) void rp_scan_kernel(int64_t n, int64_t C, const T* __restrict__ in,
                                                      const unsigned char* __restrict__ bnd, int exclusive, int reverse,
                                                      T* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * C) return;
  const int64_t first = e / C, c = e - first * C;
  if (first != 0 && !bnd[first]) return;
  const T identity = PROD ? (T)1 : (T)0;
  if (!reverse) {
    T acc = exclusive ? identity : in[first * C + c];
    out[first * C + c] = acc;
    for (int64_t k = first + 1; k < n && !bnd[k]; ++k) {
      acc = rp_op<PROD>(in[(exclusive ? k - 1 : k) * C + c], acc);
      out[k * C + c] = acc;
    }
  } else {
    int64_t last = first;
    while (last + 1 < n && !bnd[last + 1]) ++last;
    T acc = exclusive ? identity : in[last * C + c];
    out[last * C + c] = acc;
    for (int64_t k = last - 1; k >= first; --k) {
      acc = rp_op<PROD>(in[(exclusive ? k + 1 : k) * C + c], acc);
      out[k * C + c] = acc;
    }
  }
}
// pack p = inclusive_sum[i] - 1 of element i; a pack starts where the sum changes.  Row p of out = the pack's elements
// accumulated from the first one on, in index order.
template <typename T, bool PROD>
__global__ __launch_bounds__(256) void rp_reduce_kernel(int64_t n, int64_t C, int64_t num_packs, const T* __restrict__ in,
                                                        const int* __restrict__ isum, T* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * C) return;
  const int64_t first = e / C, c = e - first * C;
  const int id = isum[first];
  if (first != 0 && isum[first - 1] == id) return;
  const int64_t pack = (int64_t)id - 1;
  if (pack < 0 || pack >= num_packs) return;           // the row of out
  T acc = in[first * C + c];
  for (int64_t k = first + 1; k < n && isum[k] == id; ++k) acc = rp_op<PROD>(acc, in[k * C + c]);
  out[pack * C + c] = acc;
}
bool rp_grid(int64_t n, int64_t C, unsigned* grid) {
  if (n < 0 || C < 0 || (C > 0 && n > 0x7FFFFFFFFFFFFFFFLL / C)) return false;
  const int64_t g = (n * C + 255) / 256;
  if (g > 0x7FFFFFFFLL) return false;
  *grid = (unsigned)g;
  return true;
}
template <typename T>
int rp_scan(void* stream, int64_t n, int64_t C, const T* feats, const uint8_t* boundaries, int prod, int exclusive, int reverse,
            T* out) {
  unsigned g;
  if (!rp_grid(n, C, &g)) return (int)hipErrorInvalidValue;
  if (g == 0) return 0;
  if (prod)
    hipLaunchKernelGGL((rp_scan_kernel<T, true>), dim3(g), dim3(256), 0, (hipStream_t)stream, n, C, feats, boundaries, exclusive,
                       reverse, out);
  else
    hipLaunchKernelGGL((rp_scan_kernel<T, false>), dim3(g), dim3(256), 0, (hipStream_t)stream, n, C, feats, boundaries, exclusive,
                       reverse, out);
  KAMD_RETURN_LAST_ERROR();
}
template <typename T>
int rp_reduce(void* stream, int64_t n, int64_t C, int64_t num_packs, const T* feats, const int32_t* inclusive_sum, int prod, T* out) {
  unsigned g;
  if (!rp_grid(n, C, &g) || num_packs < 0) return (int)hipErrorInvalidValue;
  if (g == 0 || num_packs == 0) return 0;
  if (prod)
    hipLaunchKernelGGL((rp_reduce_kernel<T, true>), dim3(g), dim3(256), 0, (hipStream_t)stream, n, C, num_packs, feats,
                       inclusive_sum, out);
  else
    hipLaunchKernelGGL((rp_reduce_kernel<T, false>), dim3(g), dim3(256), 0, (hipStream_t)stream, n, C, num_packs, feats,
                       inclusive_sum, out);
  KAMD_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {

size_t kamd_spc_raytrace_workspace(int64_t N) {
  if (N <= 0) return 0;
  return rt_ws(nullptr, N).total_bytes;
}

int kamd_spc_raytrace_count(void* stream, int64_t N, int level, int64_t num_bytes, int64_t num_points, const uint8_t* octree,
                            const int32_t* exsum, const int16_t* points, const float* origin, const float* direction, int with_exit,
                            void* workspace, int64_t* host_total) {
  if (!rt_args_ok(N, level, num_bytes, num_points) || workspace == nullptr || host_total == nullptr)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const RtWs w = rt_ws(workspace, N);
  const dim3 grid((unsigned)kamd_cdiv(N, RT_BLOCK));
  if (with_exit)
    hipLaunchKernelGGL((rt_walk_kernel<false, 2>), grid, dim3(RT_BLOCK), rt_lds(level), st, N, level, num_bytes, num_points, octree,
                       exsum, points, origin, direction, w.counts, (const long long*)nullptr, (int64_t)0, (int*)nullptr,
                       (float*)nullptr);
  else
    hipLaunchKernelGGL((rt_walk_kernel<false, 0>), grid, dim3(RT_BLOCK), rt_lds(level), st, N, level, num_bytes, num_points, octree,
                       exsum, points, origin, direction, w.counts, (const long long*)nullptr, (int64_t)0, (int*)nullptr,
                       (float*)nullptr);
  KAMD_CHECK(hipGetLastError());
  KAMD_CHECK(ss_scan(st, N, (const long long*)nullptr, w.counts, w.offs, w.sums));
  // the one host read of a trace: the number of hits sizes the results
  long long total = 0;
  KAMD_CHECK(hipMemcpyAsync(&total, w.offs + N, sizeof(long long), hipMemcpyDeviceToHost, st));
  KAMD_CHECK(hipStreamSynchronize(st));
  *host_total = (int64_t)total;
  return 0;
}

int kamd_spc_raytrace_emit(void* stream, int64_t N, int level, int64_t num_bytes, int64_t num_points, const uint8_t* octree,
                           const int32_t* exsum, const int16_t* points, const float* origin, const float* direction, int depth_mode,
                           const void* workspace, int64_t total, int32_t* nuggets, float* depths) {
  if (!rt_args_ok(N, level, num_bytes, num_points) || workspace == nullptr || total < 0 || depth_mode < 0 || depth_mode > 2)
    return (int)hipErrorInvalidValue;
  if (total == 0) return 0;
  if (nuggets == nullptr || (depth_mode > 0 && depths == nullptr)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const RtWs w = rt_ws(const_cast<void*>(workspace), N);
  const dim3 grid((unsigned)kamd_cdiv(N, RT_BLOCK));
#define RT_EMIT(MODE)                                                                                                             \
  hipLaunchKernelGGL((rt_walk_kernel<true, MODE>), grid, dim3(RT_BLOCK), rt_lds(level), st, N, level, num_bytes, num_points, octree, \
                     exsum, points, origin, direction, (int*)nullptr, (const long long*)w.offs, total, nuggets, depths)
  if (depth_mode == 0)
    RT_EMIT(0);
  else if (depth_mode == 1)
    RT_EMIT(1);
  else
    RT_EMIT(2);
#undef RT_EMIT
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spc_pack_scan_f32(void* stream, int64_t n, int64_t C, const float* feats, const uint8_t* boundaries, int prod, int exclusive,
                           int reverse, float* out) {
  return rp_scan<float>(stream, n, C, feats, boundaries, prod, exclusive, reverse, out);
}
int kamd_spc_pack_scan_f64(void* stream, int64_t n, int64_t C, const double* feats, const uint8_t* boundaries, int prod,
                           int exclusive, int reverse, double* out) {
  return rp_scan<double>(stream, n, C, feats, boundaries, prod, exclusive, reverse, out);
}
int kamd_spc_pack_reduce_f32(void* stream, int64_t n, int64_t C, int64_t num_packs, const float* feats, const int32_t* inclusive_sum,
                             int prod, float* out) {
  return rp_reduce<float>(stream, n, C, num_packs, feats, inclusive_sum, prod, out);
}
int kamd_spc_pack_reduce_f64(void* stream, int64_t n, int64_t C, int64_t num_packs, const double* feats,
                             const int32_t* inclusive_sum, int prod, double* out) {
  return rp_reduce<double>(stream, n, C, num_packs, feats, inclusive_sum, prod, out);
}

}  // extern "C"
