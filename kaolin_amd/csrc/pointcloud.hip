// ops.conversions.pointcloud: a point cloud -> the octree of an SPC level with the mean feature of every occupied cell
// (unbatched_pointcloud_to_spc), and batched point clouds -> occupancy grids (pointclouds_to_voxelgrids).
//
// The reference's versions are pure PyTorch (kaolin/ops/conversions/pointcloud.py): a row-wise unique, a sort, an index_add_ of
// doubles (float atomics: the last bits change from run to run) and, for the grids, a unique over (B P, 4) int64 rows.  Here:
//   * one thread per point quantises it (the operations of ops.spc.quantize_points, in their order) and writes (Morton key, index);
//   * the stable pair sort of sort_scan.h orders the pairs by key: the members of a cell stay in ascending input index;
//   * run heads, an exclusive scan and the run starts (U + 1);
//   * the octree from the sorted keys through kamd_spc_octree_build (its own head / scan / unique pass drops the duplicates, so
//     its ONE host read brings U and the level sizes together);
//   * the segmented mean, lanes along D, no atomics, in a fixed order (below).
// Every index that comes from data (a permutation entry, a run id, a run start) is compared with its buffer's size before use.
//
// Order of the mean.  The sorted positions are cut into chunks of PC_CHUNK.  A piece = the members of one run inside one chunk; a
// piece is summed in ascending position (= ascending input index), starting from 0.0, in double.  A run inside one chunk is its
// piece.  A run over several chunks k0 < ... < k1 has G = 64 / lanes-per-row partial sums: partial g starts from the run's piece
// in k0 (g = 0) or from 0.0 and adds the pieces in chunks k0 + 1 + g, k0 + 1 + g + G, ... in ascending order; the partials meet
// in a butterfly (xor of the group index by G / 2, ..., 1; every step adds two values, and a + b = b + a).  Then one division by
// the count in double, rint for the integer types, one cast.  Nothing depends on the launch or on timing.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include "common.h"
#include "sort_scan.h"
#include "spc_octree.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr int PC_MAX_LEVEL = 15;  // KAOLIN_SPC_MAX_LEVELS
constexpr int PC_CHUNK = 128;     // sorted positions per chunk of the mean

// ---- keys ------------------------------------------------------------------------------------------------------------------------
// ops.spc.quantize_points: floor(clamp(res * (x + 1.0) / 2.0, 0, res - 1)).short() -- x + 1 rounded in T, the two scalings by powers
// of two (exact unless they overflow, which the clamp then catches, as in torch), NaN stays NaN through the clamp and casts to 0.
__device__ __forceinline__ float pc_floor(float v) { return floorf(v); }
__device__ __forceinline__ double pc_floor(double v) { return floor(v); }
__device__ __forceinline__ float pc_rint(float v) { return rintf(v); }  // half to even
__device__ __forceinline__ double pc_rint(double v) { return rint(v); }
template <typename T>
__device__ __forceinline__ int pc_quantize(T x, T res, T top) {
  T t = x + (T)1.0;
  t = res * t;
  t = t / (T)2.0;
  if (t != t) return 0;
  t = t < (T)0.0 ? (T)0.0 : t;
  t = t > top ? top : t;
  return (int)pc_floor(t);
}
template <typename T>
__global__ __launch_bounds__(256) void pc_keys_kernel(int64_t n, int level, const T* __restrict__ points, int64_t stride_n,
                                                      int64_t stride_c, uint64_t* __restrict__ keys, int64_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const T res = (T)(1 << level), top = (T)((1 << level) - 1);
  const T* p = points + i * stride_n;
  const int x = pc_quantize<T>(p[0], res, top), y = pc_quantize<T>(p[stride_c], res, top), z = pc_quantize<T>(p[2 * stride_c], res, top);
  keys[i] = ms_to_morton(x, y, z);
  vals[i] = i;
}
// quantised already (half points go through quantize_points in torch): the low `level` bits of every coordinate
__global__ __launch_bounds__(256) void pc_keys_i16_kernel(int64_t n, int level, const int16_t* __restrict__ points,
                                                          uint64_t* __restrict__ keys, int64_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int mask = (1 << level) - 1;
  keys[i] = ms_to_morton(points[3 * i] & mask, points[3 * i + 1] & mask, points[3 * i + 2] & mask);
  vals[i] = i;
}

// starts[r] = first sorted position of run r, starts[U] = n (pos = the exclusive scan of the n head flags: pos[i] <= pos[n] <= n)
__global__ __launch_bounds__(256) void pc_starts_kernel(int64_t n, const int* __restrict__ flag, const int64_t* __restrict__ pos,
                                                        int64_t* __restrict__ starts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (flag[i]) {
    const int64_t r = pos[i];
    if (r >= 0 && r < n) starts[r] = i;  // guard: a run id outside the n + 1 starts
  }
  if (i == 0) {
    const int64_t u = pos[n];
    if (u >= 0 && u <= n) starts[u] = n;
  }
}

// workspace of the SPC build for n points (8-byte words unless noted): keys in | vals in | keys tmp | vals tmp | keys sorted | vals
// sorted | pos (n + 1) | starts (n + 1) | scan sums | flag (n ints) | the sort's scratch | the octree build's workspace
struct PcWs {
  uint64_t *k0, *kt, *ks;
  int64_t *v0, *vt, *vs, *pos, *starts, *sums;
  int* flag;
  SsSortWs sort;
  void* octree;
  size_t octree_bytes, total_bytes;
};
PcWs pc_ws(void* base, int64_t n, int level) {
  PcWs w;
  char* p = (char*)base;
  auto take = [&](size_t bytes) {
    char* r = p;
    p += (bytes + 255) & ~(size_t)255;
    return r;
  };
  const size_t n1 = (size_t)(n > 0 ? n : 1);
  w.k0 = (uint64_t*)take(n1 * 8);
  w.v0 = (int64_t*)take(n1 * 8);
  w.kt = (uint64_t*)take(n1 * 8);
  w.vt = (int64_t*)take(n1 * 8);
  w.ks = (uint64_t*)take(n1 * 8);
  w.vs = (int64_t*)take(n1 * 8);
  w.pos = (int64_t*)take((n1 + 1) * 8);
  w.starts = (int64_t*)take((n1 + 1) * 8);
  w.sums = (int64_t*)take(ss_scan_sums_entries((long long)n1) * 8);
  w.flag = (int*)take(n1 * 4);
  w.sort.hist = (int*)take(ss_sort_hist_entries(n) * 4);
  w.sort.offs = (long long*)take(ss_sort_offs_entries(n) * 8);
  w.sort.sums = (long long*)take(ss_sort_sums_entries(n) * 8);
  w.octree_bytes = kamd_spc_octree_workspace(n, level);
  w.octree = (void*)take(w.octree_bytes);
  w.total_bytes = (size_t)(p - (char*)base);
  return w;
}

// after the keys: sort, run starts, octree (the one host read)
int pc_build_tail(hipStream_t st, int64_t n, int level, const PcWs& w, int64_t* host_sizes) {
  KAMD_CHECK(hipGetLastError());
  KAMD_CHECK(ss_sort(st, n, ss_passes_low(3 * level), w.k0, w.v0, w.kt, w.vt, w.ks, w.vs, w.sort));
  const unsigned g = (unsigned)kamd_cdiv(n, 256);
  KAMD_CHECK(ss_heads_scan(st, n, (const int64_t*)nullptr, w.ks, 0, w.flag, w.pos, w.sums));
  hipLaunchKernelGGL(pc_starts_kernel, dim3(g), dim3(256), 0, st, n, (const int*)w.flag, (const int64_t*)w.pos, w.starts);
  KAMD_CHECK(hipGetLastError());
  // sorted = 1 skips the build's sort only: its head / scan / unique pass keeps one code per run of equal codes
  return kamd_spc_octree_build((void*)st, n, level, (const int64_t*)w.ks, 1, w.octree, w.octree_bytes, host_sizes);
}
bool pc_build_args(int64_t n, int level, const void* points, const void* workspace, size_t workspace_bytes, const int64_t* host_sizes) {
  if (n <= 0 || level < 1 || level > PC_MAX_LEVEL || points == nullptr || host_sizes == nullptr) return false;
  if ((n + 255) / 256 > 0x7FFFFFFFLL) return false;
  return workspace != nullptr && workspace_bytes >= pc_ws(nullptr, n, level).total_bytes;
}
template <typename T>
int pc_build(void* stream, int64_t n, int level, const T* points, int64_t stride_n, int64_t stride_c, void* workspace,
             size_t workspace_bytes, int64_t* host_sizes) {
  if (!pc_build_args(n, level, points, workspace, workspace_bytes, host_sizes)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const PcWs w = pc_ws(workspace, n, level);
  hipLaunchKernelGGL((pc_keys_kernel<T>), dim3(kamd_cdiv(n, 256)), dim3(256), 0, st, n, level, points, stride_n, stride_c, w.k0, w.v0);
  return pc_build_tail(st, n, level, w, host_sizes);
}

// ---- the segmented mean ----------------------------------------------------------------------------------------------------------
enum { PC_BOOL = 0, PC_U8, PC_I8, PC_I16, PC_I32, PC_I64, PC_F16, PC_F32, PC_F64, PC_NUM_DTYPES };

template <typename T> __device__ __forceinline__ double pc_load(const T* p) { return (double)*p; }
template <> __device__ __forceinline__ double pc_load<__half>(const __half* p) { return (double)__half2float(*p); }
template <> __device__ __forceinline__ double pc_load<bool>(const bool* p) { return *(const unsigned char*)p ? 1.0 : 0.0; }

// sum / count in double; integers and bool: rint (half to even); one cast (half through float, as torch's)
template <typename T> __device__ __forceinline__ void pc_store(T* p, double sum, int64_t count) { *p = (T)rint(sum / (double)count); }
template <> __device__ __forceinline__ void pc_store<double>(double* p, double sum, int64_t count) { *p = sum / (double)count; }
template <> __device__ __forceinline__ void pc_store<float>(float* p, double sum, int64_t count) { *p = (float)(sum / (double)count); }
template <> __device__ __forceinline__ void pc_store<__half>(__half* p, double sum, int64_t count) {
  *p = __float2half((float)(sum / (double)count));
}
template <> __device__ __forceinline__ void pc_store<bool>(bool* p, double sum, int64_t count) {
  *(unsigned char*)p = rint(sum / (double)count) != 0.0 ? 1 : 0;
}

// DL lanes (a power of two <= 64) share a chunk; a lane owns the columns lane, lane + DL, ...  Pieces of runs that lie inside the
// chunk go to `out`; the piece that continues a run from the chunk before goes to first[k], the piece of a run that goes on
// into the next chunk to last[k].  A chunk without a head is one piece: first[k].
template <typename T>
__global__ __launch_bounds__(256) void pc_mean_chunks_kernel(int64_t n, int64_t U, int64_t D, int DL, int64_t nchunks,
                                                             const T* __restrict__ feats, int64_t stride_n, int64_t stride_d,
                                                             const int64_t* __restrict__ perm, const int* __restrict__ flag,
                                                             const int64_t* __restrict__ pos, double* __restrict__ first,
                                                             double* __restrict__ last, T* __restrict__ out) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t k = gid / DL;
  const int lane = (int)(gid % DL);
  if (k >= nchunks) return;
  const int64_t j0 = k * PC_CHUNK, j1 = (j0 + PC_CHUNK < n) ? j0 + PC_CHUNK : n;
  const bool open_end = j1 < n && !flag[j1];  // the run of the last piece goes on
  for (int64_t d = lane; d < D; d += DL) {
    double acc = 0.0;
    int64_t head = -1;  // position of the head of the current piece's run, -1: it lies before the chunk
    int64_t idx_next = perm[j0];
    int head_next = flag[j0];
    for (int64_t j = j0; j < j1; ++j) {
      const int64_t idx = idx_next;
      const int is_head = head_next;
      if (j + 1 < j1) {
        idx_next = perm[j + 1];
        head_next = flag[j + 1];
      }
      // guard: a permutation entry outside the n feature rows adds nothing
      const double v = (idx >= 0 && idx < n) ? pc_load<T>(feats + idx * stride_n + d * stride_d) : 0.0;
      if (is_head) {
        if (j > j0) {
          if (head < 0) {
            first[k * D + d] = acc;
          } else {
            const int64_t r = pos[head];
            if (r >= 0 && r < U) pc_store<T>(out + r * D + d, acc, j - head);  // guard: a run id outside the U rows
          }
        }
        head = j;
        acc = 0.0;
      }
      acc += v;
    }
    if (head < 0) {
      first[k * D + d] = acc;
    } else if (open_end) {
      last[k * D + d] = acc;
    } else {
      const int64_t r = pos[head];
      if (r >= 0 && r < U) pc_store<T>(out + r * D + d, acc, j1 - head);
    }
  }
}

// one wavefront per chunk boundary b (position b * PC_CHUNK): the run that crosses it is finished here if this is the first
// boundary it crosses.  G = 64 / DL groups of DL lanes take the chunks after the first in turn.
template <typename T>
__global__ __launch_bounds__(256) void pc_mean_runs_kernel(int64_t n, int64_t U, int64_t D, int DL, int64_t nchunks,
                                                           const int* __restrict__ flag, const int64_t* __restrict__ pos,
                                                           const int64_t* __restrict__ starts, const double* __restrict__ first,
                                                           const double* __restrict__ last, T* __restrict__ out) {
  const int64_t b = ((int64_t)blockIdx.x * 256 + threadIdx.x) / 64 + 1;
  if (b >= nchunks) return;  // (the whole wavefront)
  const int64_t j = b * PC_CHUNK;
  if (j >= n || flag[j]) return;
  const int64_t r = pos[j] - 1;  // heads before j, the run's own included
  if (r < 0 || r >= U) return;   // guard: a run id outside the U + 1 starts
  const int64_t s = starts[r], e = starts[r + 1];
  if (!(s >= 0 && s < j && j < e && e <= n)) return;  // guard: run starts that do not enclose the boundary
  const int64_t k0 = b - 1;
  if (s < k0 * PC_CHUNK) return;  // an earlier boundary owns the run
  const int64_t k1 = (e - 1) / PC_CHUNK;
  const int wl = threadIdx.x & 63, G = 64 / DL, g = wl / DL, lane = wl % DL;
  for (int64_t d0 = 0; d0 < D; d0 += DL) {  // (uniform over the wavefront: the shuffles below meet all lanes)
    const int64_t d = d0 + lane;
    const bool on = d < D;
    double acc = (on && g == 0) ? last[k0 * D + d] : 0.0;
    if (on) {
#pragma unroll 4
      for (int64_t k = k0 + 1 + g; k <= k1; k += G) acc += first[k * D + d];
    }
    for (int off = 32; off >= DL; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (on && g == 0) pc_store<T>(out + r * D + d, acc, e - s);
  }
}

template <typename T>
int pc_mean(hipStream_t st, int64_t n, int64_t U, int64_t D, const void* feats, int64_t stride_n, int64_t stride_d, const PcWs& w,
            double* scratch, void* out) {
  int DL = 1;
  while (DL < 64 && DL < D) DL <<= 1;
  const int64_t nchunks = (n + PC_CHUNK - 1) / PC_CHUNK;
  double* first = scratch;
  double* last = scratch + (size_t)nchunks * (size_t)D;
  const int64_t blocks1 = (nchunks * DL + 255) / 256;
  if (blocks1 > 0x7FFFFFFFLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((pc_mean_chunks_kernel<T>), dim3((unsigned)blocks1), dim3(256), 0, st, n, U, D, DL, nchunks, (const T*)feats,
                     stride_n, stride_d, (const int64_t*)w.vs, (const int*)w.flag, (const int64_t*)w.pos, first, last, (T*)out);
  if (nchunks > 1) {
    const int64_t blocks2 = ((nchunks - 1) * 64 + 255) / 256;
    hipLaunchKernelGGL((pc_mean_runs_kernel<T>), dim3((unsigned)blocks2), dim3(256), 0, st, n, U, D, DL, nchunks, (const int*)w.flag,
                       (const int64_t*)w.pos, (const int64_t*)w.starts, (const double*)first, (const double*)last, (T*)out);
  }
  KAMD_RETURN_LAST_ERROR();
}

// ---- voxel grids -------------------------------------------------------------------------------------------------------------------
// the reference's arithmetic, every operation rounded in the points' dtype (half: computed in float and rounded to half after each
// operation, which is what torch does): round_half_even(((p - origin) / scale) * mult), mult = R - 1 rounded to the dtype.
__device__ __forceinline__ float pc_rnd(float v, const __half*) { return __half2float(__float2half(v)); }
__device__ __forceinline__ float pc_rnd(float v, const float*) { return v; }
__device__ __forceinline__ double pc_rnd(double v, const double*) { return v; }
__device__ __forceinline__ float pc_get(const __half* p, int64_t i) { return __half2float(p[i]); }
__device__ __forceinline__ float pc_get(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ double pc_get(const double* p, int64_t i) { return p[i]; }
__device__ __forceinline__ void pc_one(__half* p) { *p = __float2half(1.0f); }
__device__ __forceinline__ void pc_one(float* p) { *p = 1.0f; }
__device__ __forceinline__ void pc_one(double* p) { *p = 1.0; }

// one thread per point.  Dense: the value 1 with a plain store (threads that meet in a voxel store the same value).  Sparse: the
// voxel's bit with an atomic OR on the 32-bit word.  NaN and +-inf fail the range test.
template <typename T, bool SPARSE>
__global__ __launch_bounds__(256) void pc_voxel_kernel(int64_t total, int64_t P, int R, double mult_d, int64_t words,
                                                       const T* __restrict__ points, const T* __restrict__ origin,
                                                       const T* __restrict__ scale, void* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t b = i / P;
  const T* tag = nullptr;
  typedef decltype(pc_get(points, 0)) A;
  const A s = pc_get(scale, b), mult = (A)mult_d, top = (A)(R - 1);
  int64_t c[3];
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    A v = pc_rnd(pc_get(points, 3 * i + a) - pc_get(origin, 3 * b + a), tag);
    v = pc_rnd(v / s, tag);
    v = pc_rnd(v * mult, tag);
    v = pc_rint(v);
    ok = ok && v >= (A)0 && v <= top;  // (NaN: false)
    c[a] = ok ? (int64_t)v : 0;
  }
  if (!ok) return;
  const int64_t lin = (c[0] * R + c[1]) * R + c[2];  // < R^3: every index lies in [0, R - 1]
  if (SPARSE)
    atomicOr((unsigned*)out + b * words + (lin >> 5), 1u << (unsigned)(lin & 31));
  else
    pc_one((T*)out + b * (int64_t)R * R * R + lin);
}
template <typename T>
int pc_voxelgrids(void* stream, int64_t B, int64_t P, int R, double mult, const T* points, const T* origin, const T* scale, int sparse,
                  void* out) {
  if (B < 0 || P < 0 || R < 1 || R > 2048 || out == nullptr) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int64_t cells = (int64_t)R * R * R, words = (cells + 31) / 32, total = B * P;
  if (B == 0) return 0;
  KAMD_CHECK(kamd_zero_async(out, sparse ? (size_t)B * (size_t)words * 4 : (size_t)B * (size_t)cells * sizeof(T), st));
  if (total == 0) return 0;
  if (points == nullptr || origin == nullptr || scale == nullptr || (total + 255) / 256 > 0x7FFFFFFFLL) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (sparse)
    hipLaunchKernelGGL((pc_voxel_kernel<T, true>), grid, dim3(256), 0, st, total, P, R, mult, words, points, origin, scale, out);
  else
    hipLaunchKernelGGL((pc_voxel_kernel<T, false>), grid, dim3(256), 0, st, total, P, R, mult, words, points, origin, scale, out);
  KAMD_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {

size_t kamd_pointcloud_spc_workspace(int64_t n, int level) {
  if (n <= 0 || level < 1 || level > PC_MAX_LEVEL) return 0;
  return pc_ws(nullptr, n, level).total_bytes;
}

int kamd_pointcloud_spc_build_f32(void* stream, int64_t n, int level, const float* points, int64_t stride_n, int64_t stride_c,
                                  void* workspace, size_t workspace_bytes, int64_t* host_sizes) {
  return pc_build<float>(stream, n, level, points, stride_n, stride_c, workspace, workspace_bytes, host_sizes);
}
int kamd_pointcloud_spc_build_f64(void* stream, int64_t n, int level, const double* points, int64_t stride_n, int64_t stride_c,
                                  void* workspace, size_t workspace_bytes, int64_t* host_sizes) {
  return pc_build<double>(stream, n, level, points, stride_n, stride_c, workspace, workspace_bytes, host_sizes);
}
int kamd_pointcloud_spc_build_i16(void* stream, int64_t n, int level, const int16_t* points, void* workspace, size_t workspace_bytes,
                                  int64_t* host_sizes) {
  if (!pc_build_args(n, level, points, workspace, workspace_bytes, host_sizes)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const PcWs w = pc_ws(workspace, n, level);
  hipLaunchKernelGGL(pc_keys_i16_kernel, dim3(kamd_cdiv(n, 256)), dim3(256), 0, st, n, level, points, w.k0, w.v0);
  return pc_build_tail(st, n, level, w, host_sizes);
}

int kamd_pointcloud_spc_octree(void* stream, int64_t n, int level, const void* workspace, int64_t octree_bytes, uint8_t* octree) {
  if (n <= 0 || level < 1 || level > PC_MAX_LEVEL || workspace == nullptr) return (int)hipErrorInvalidValue;
  const PcWs w = pc_ws(const_cast<void*>(workspace), n, level);
  return kamd_spc_octree_gather(stream, n, level, w.octree, octree_bytes, octree);
}

size_t kamd_pointcloud_spc_mean_workspace(int64_t n, int64_t D) {
  if (n <= 0 || D <= 0) return 0;
  return (size_t)2 * (size_t)((n + PC_CHUNK - 1) / PC_CHUNK) * (size_t)D * sizeof(double);
}

int kamd_pointcloud_spc_mean(void* stream, int dtype, int64_t n, int level, int64_t U, int64_t D, const void* features,
                             int64_t stride_n, int64_t stride_d, const void* workspace, void* mean_workspace, void* out) {
  if (n <= 0 || level < 1 || level > PC_MAX_LEVEL || U <= 0 || U > n || D <= 0 || dtype < 0 || dtype >= PC_NUM_DTYPES)
    return (int)hipErrorInvalidValue;
  if (features == nullptr || workspace == nullptr || mean_workspace == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const PcWs w = pc_ws(const_cast<void*>(workspace), n, level);
  double* scratch = (double*)mean_workspace;
  switch (dtype) {
    case PC_BOOL: return pc_mean<bool>(st, n, U, D, features, stride_n, stride_d, w, scratch, out);
    case PC_U8: return pc_mean<uint8_t>(st, n, U, D, features, stride_n, stride_d, w, scratch, out);
    case PC_I8: return pc_mean<int8_t>(st, n, U, D, features, stride_n, stride_d, w, scratch, out);
    case PC_I16: return pc_mean<int16_t>(st, n, U, D, features, stride_n, stride_d, w, scratch, out);
    case PC_I32: return pc_mean<int32_t>(st, n, U, D, features, stride_n, stride_d, w, scratch, out);
    case PC_I64: return pc_mean<int64_t>(st, n, U, D, features, stride_n, stride_d, w, scratch, out);
    case PC_F16: return pc_mean<__half>(st, n, U, D, features, stride_n, stride_d, w, scratch, out);
    case PC_F32: return pc_mean<float>(st, n, U, D, features, stride_n, stride_d, w, scratch, out);
    default: return pc_mean<double>(st, n, U, D, features, stride_n, stride_d, w, scratch, out);
  }
}

int kamd_pointcloud_voxelgrids_f16(void* stream, int64_t B, int64_t P, int R, double mult, const void* points, const void* origin,
                                       const void* scale, int sparse, void* out) {
  return pc_voxelgrids<__half>(stream, B, P, R, mult, (const __half*)points, (const __half*)origin, (const __half*)scale, sparse, out);
}
int kamd_pointcloud_voxelgrids_f32(void* stream, int64_t B, int64_t P, int R, double mult, const float* points,
                                       const float* origin, const float* scale, int sparse, void* out) {
  return pc_voxelgrids<float>(stream, B, P, R, mult, points, origin, scale, sparse, out);
}
int kamd_pointcloud_voxelgrids_f64(void* stream, int64_t B, int64_t P, int R, double mult, const double* points,
                                       const double* origin, const double* scale, int sparse, void* out) {
  return pc_voxelgrids<double>(stream, B, P, R, mult, points, origin, scale, sparse, out);
}

}  // extern "C"
