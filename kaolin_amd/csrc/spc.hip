// ops.spc: the core of Kaolin's structured point cloud (SPC) operators -- Morton codes, octree build, scan, point generation, query
// and the dense conversion ("The SPC core").
//
// Replaces kaolin/csrc/ops/spc/spc_cuda.cu:33-178 (points / codes -> octree), scan_octrees.cu:34-105, generate_points.cu:28-78,
// query_cuda.cu:25-123 with spc_utils.cuh:28-102 (the walk), feature_grids_cuda.cu:28-135 and point_utils_cuda.cu:25-42.
//
// The reference drives every one of these from the host, level by level and item by item, with a blocking read in between
// (scan: one read per level and item; build: one per level; generate_points: one launch per level and item plus a host write).  Here:
//   * scan: popcount + inclusive scan over the whole batch (sums of 1024-blocks, then apply), ONE small kernel that walks every
//     item's levels through the sums on the device, a rebase that restarts the sums at every item, and one read of the pyramids;
//   * generate_points: one launch per level for the whole batch (grid.y = item), children written as int16 `2 * parent + bit`
//     straight from the parent's point -- no Morton array, no host read (the sizes are in the CPU pyramid);
//   * build: codes masked to 3 * level bits, the keys-only radix sort and run heads of sort_scan.h, parents / gather of spc_octree.h
//     (shared with mesh_to_spc.hip); all levels on the device, one read of the level sizes;
//   * query: one thread per query walks `level` dependent (byte, int) loads -- latency-bound by construction, nothing to tile;
//   * to_dense: zero fill + one thread per (point, channel); the points of a level are distinct, so plain stores.
// Every data-derived index is compared with the size of the buffer it indexes before use (the list is in DESIGN.md).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "common.h"
#include "sort_scan.h"
#include "spc_octree.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr int SP_MAX_LEVEL = 15;          // KAOLIN_SPC_MAX_LEVELS (spc_math.h:38)
constexpr int SP_PYR = SP_MAX_LEVEL + 2;  // columns of a full pyramid row
constexpr int SP_PYR_ITEM = 2 * SP_PYR + 1;  // ints per item read back: the (2, 17) pyramid, then the depth

inline unsigned sp_grid(int64_t items) {  // grid-stride kernels of 256 threads
  int64_t g = items > 0 ? (items + 255) / 256 : 1;
  if (g > (int64_t)KAMD_NUM_CU * 16) g = (int64_t)KAMD_NUM_CU * 16;
  return (unsigned)g;
}

// ---- points <-> Morton codes, corners --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sp_points_to_morton_kernel(int64_t n, const int16_t* __restrict__ p, int64_t* __restrict__ m) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    m[i] = (int64_t)ms_to_morton(p[3 * i], p[3 * i + 1], p[3 * i + 2]);  // the low 15 bits of a coordinate (spc_math.h:98-113)
}
__global__ __launch_bounds__(256) void sp_morton_to_points_kernel(int64_t n, const int64_t* __restrict__ m, int16_t* __restrict__ p) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int x, y, z;
    ms_to_point((uint64_t)m[i], &x, &y, &z);
    p[3 * i] = (int16_t)x;
    p[3 * i + 1] = (int16_t)y;
    p[3 * i + 2] = (int16_t)z;
  }
}
// one thread per (point, corner): corner j adds (j >> 2, (j >> 1) & 1, j & 1) (point_utils_cuda.cu:36-40)
__global__ __launch_bounds__(256) void sp_points_to_corners_kernel(int64_t n, const int16_t* __restrict__ p, int16_t* __restrict__ c) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n * 8; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e >> 3;
    const int j = (int)(e & 7);
    c[3 * e] = (int16_t)(p[3 * i] + (j >> 2));
    c[3 * e + 1] = (int16_t)(p[3 * i + 1] + ((j >> 1) & 1));
    c[3 * e + 2] = (int16_t)(p[3 * i + 2] + (j & 1));
  }
}

// ---- octree build ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sp_mask_codes_kernel(int64_t n, const int64_t* __restrict__ m, uint64_t mask,
                                                            int64_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = (int64_t)((uint64_t)m[i] & mask);
}
__global__ __launch_bounds__(256) void sp_unique_kernel(int64_t n, const int64_t* __restrict__ m, const int* __restrict__ flag,
                                                        const int64_t* __restrict__ pos, int64_t* __restrict__ um,
                                                        int64_t* __restrict__ sizes) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && flag[i]) um[pos[i]] = m[i];  // pos[i] < pos[n] <= n: the scan of these n flags
  if (i == 0) sizes[0] = pos[n];
}
// workspace of kamd_spc_octree_build for n codes at `level` (8-byte words unless noted):
//   sizes (16) | codes A (n) | codes B (n) | pos (n + 1) | scan sums | flag (n ints) | level bytes (level * n)
//   | the sort's scratch (sort_scan_host.h): (digit, block) counts (ints), their offsets and scan sums
struct SpWs {
  int64_t *sizes, *ka, *kb, *pos, *sums;
  int* flag;
  unsigned char* level_bytes;
  SsSortWs sort;
  size_t total_bytes;
};
SpWs sp_ws(void* base, int64_t n, int level) {
  SpWs w;
  char* p = (char*)base;
  auto take = [&](size_t bytes) {
    char* r = p;
    p += (bytes + 255) & ~(size_t)255;
    return r;
  };
  const size_t nn = (size_t)(n > 0 ? n : 1);
  w.sizes = (int64_t*)take(16 * 8);
  w.ka = (int64_t*)take(nn * 8);
  w.kb = (int64_t*)take(nn * 8);
  w.pos = (int64_t*)take(nn * 8 + 8);
  w.sums = (int64_t*)take(ss_scan_sums_entries((long long)nn) * 8);
  w.flag = (int*)take(nn * 4);
  w.level_bytes = (unsigned char*)take((size_t)(level > 0 ? level : 1) * nn);
  w.sort.hist = (int*)take(ss_sort_hist_entries(n) * 4);
  w.sort.offs = (long long*)take(ss_sort_offs_entries(n) * 8);
  w.sort.sums = (long long*)take(ss_sort_sums_entries(n) * 8);
  w.total_bytes = (size_t)(p - (char*)base);
  return w;
}

// ---- scan ---------------------------------------------------------------------------------------------------------------------------
// the bit counts of all bytes of the batch are summed inclusively over the WHOLE batch (ss_scan_inclusive of bytes); the pyramid
// kernel and the rebase make them per item.  total * 8 < 2^31 (checked by the caller), so an int holds every sum.
// one thread per item: scan_octrees.cu:80-96 on the device.  Level L holds g[first byte of level L - 1 ... ] so the item's sums are
// read at `prev`, the number of points above level L; the index is clamped to the item's last byte.
__global__ __launch_bounds__(256) void sp_pyramid_kernel(int64_t B, int64_t total, const int64_t* __restrict__ starts,
                                                         const int* __restrict__ g, int* __restrict__ pyr, int* __restrict__ base_out) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  int* P = pyr + b * SP_PYR_ITEM;
  for (int k = 0; k < SP_PYR_ITEM; ++k) P[k] = 0;
  int64_t s = starts[b], e = starts[b + 1];
  if (s < 0) s = 0;
  if (e > total) e = total;
  const int64_t len = e - s;
  int base = 0;
  if (len > 0) {  // (s < e <= total: s - 1 and s + idx below are inside g)
    base = s > 0 ? g[s - 1] : 0;
    P[0] = 1;
    P[SP_PYR + 1] = 1;
    int level = 1, prev = 0;
    while (level <= SP_MAX_LEVEL && (int64_t)P[SP_PYR + level] <= len) {
      int64_t idx = prev;
      if (idx > len - 1) idx = len - 1;
      const int cur = g[s + idx] - base;
      P[level] = cur - prev;
      P[SP_PYR + level + 1] = P[level] + P[SP_PYR + level];
      prev = cur;
      ++level;
    }
    P[2 * SP_PYR] = level - 1;
  }
  base_out[b] = base;
}
// exsum[i] = G[i] - G[start of i's item - 1]: the inclusive sum restarts at every item (in place)
__global__ __launch_bounds__(256) void sp_rebase_kernel(int64_t total, int64_t B, const int64_t* __restrict__ starts,
                                                        const int* __restrict__ base, int* __restrict__ exsum) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int64_t lo = 0, hi = B - 1;  // the last item whose start is <= i
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (starts[mid] <= i)
        lo = mid;
      else
        hi = mid - 1;
    }
    exsum[i] -= base[lo];
  }
}

// ---- generate_points: level l of every item in one launch --------------------------------------------------------------------------
// meta row of an item (W = 2 + 2 (max_level + 2) int64): first octree byte, first point, pyramid[0][:], pyramid[1][:].
// A node of level l is byte `pyramid[1][l] + j` of its octree and point of the same index; its children are the points
// exsum - popcount + 1 ... exsum (nodes_to_morton_cuda_kernel, spc_utils.cuh:187-207), written as 2 * parent + bit.
__global__ __launch_bounds__(256) void sp_generate_level_kernel(int l, int max_level, int64_t num_bytes, int64_t num_points,
                                                                const unsigned char* __restrict__ octrees,
                                                                const int* __restrict__ exsum, const int64_t* __restrict__ meta,
                                                                int16_t* __restrict__ points) {
  const int W = 2 + 2 * (max_level + 2);
  const int64_t* M = meta + (int64_t)blockIdx.y * W;
  const int64_t ostart = M[0], pstart = M[1];
  const int64_t cnt = M[2 + l], off = M[2 + (max_level + 2) + l];
  const int64_t len = M[2 + (max_level + 2) + max_level], npts = M[2 + (max_level + 2) + max_level + 1];
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < cnt; j += (int64_t)gridDim.x * 256) {
    const int64_t node = off + j, gb = ostart + node, pp = pstart + node;
    if (node < 0 || node >= len || node >= npts) continue;     // the node's byte and point lie in this item ...
    if (gb < 0 || gb >= num_bytes || pp < 0 || pp >= num_points) continue;  // ... and in the buffers
    int px = 0, py = 0, pz = 0;
    if (l == 0) {
      points[3 * pp] = 0, points[3 * pp + 1] = 0, points[3 * pp + 2] = 0;  // the root
    } else {
      px = points[3 * pp], py = points[3 * pp + 1], pz = points[3 * pp + 2];
    }
    const unsigned bits = octrees[gb];
    int64_t child = (int64_t)exsum[gb] - __popc(bits) + 1;  // the item's index of the first child's point
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (!((bits >> i) & 1u)) continue;
      const int64_t slot = pstart + child;
      if (child >= 1 && child < npts && slot >= 0 && slot < num_points) {  // the point's slot
        points[3 * slot] = (int16_t)(2 * px + (i >> 2));
        points[3 * slot + 1] = (int16_t)(2 * py + ((i >> 1) & 1));
        points[3 * slot + 2] = (int16_t)(2 * pz + (i & 1));
      }
      ++child;
    }
  }
}

// ---- query ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sp_load(const __half* p, int64_t i) { return __half2float(p[i]); }  // at::Half computes in float
__device__ __forceinline__ float sp_load(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ double sp_load(const double* p, int64_t i) { return p[i]; }

// query_cuda_kernel (query_cuda.cu:38-46): floor(0.5f * exp2f(level) * (q + 1.0f)) in the coordinate's own arithmetic (float for
// half and float, double for double); query_multiscale_cuda_kernel (:63-71): resolution * (q * 0.5 + 0.5) in double, TRUNCATED.
// A value that no int16 holds (NaN included) is a miss; then identify / identify_multiscale (spc_utils.cuh:28-102) with every
// `ord` compared with num_bytes before it indexes the octree (exsum has num_bytes entries too: ord - 1 < num_bytes).
template <typename T, bool MULTI>
__global__ __launch_bounds__(256) void sp_query_kernel(int64_t Q, int level, int64_t num_bytes, const unsigned char* __restrict__ octree,
                                                       const int* __restrict__ exsum, const T* __restrict__ coords,
                                                       int64_t* __restrict__ pidx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Q) return;
  int k[3];
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const auto q = sp_load(coords, 3 * i + c);
    if (MULTI) {
      const double v = (double)(1 << level) * ((double)q * 0.5 + 0.5);
      ok = ok && (v > -32769.0 && v < 32768.0);
      k[c] = ok ? (int)v : 0;
    } else {
      const float resolution = ldexpf(0.5f, level);  // = 0.5f * exp2f(level), exact
      const auto v = floor(resolution * (q + 1.0f));
      ok = ok && (v >= -32768 && v <= 32767);
      k[c] = ok ? (int)v : 0;
    }
  }
  const int maxval = (1 << level) - 1;
  ok = ok && k[0] >= 0 && k[1] >= 0 && k[2] >= 0 && k[0] <= maxval && k[1] <= maxval && k[2] <= maxval;
  int64_t* row = MULTI ? pidx + i * (int64_t)(level + 1) : pidx + i;
  if (!ok) {
    for (int j = 0; j <= (MULTI ? level : 0); ++j) row[j] = -1;
    return;
  }
  if (MULTI) row[0] = 0;
  int64_t ord = 0;
  for (int l = 0; l < level; ++l) {
    const int depth = level - l - 1;
    const unsigned child = (unsigned)((((k[0] >> depth) & 1) << 2) | (((k[1] >> depth) & 1) << 1) | ((k[2] >> depth) & 1));
    bool hit = false;
    if (ord >= 0 && ord < num_bytes) {
      const unsigned bits = octree[ord];
      if ((bits >> child) & 1u) {
        const int cnt = __popc(bits & ((2u << child) - 1u));
        ord = (ord == 0 ? 0 : (int64_t)exsum[ord - 1]) + cnt;
        hit = true;
      }
    }
    if (!hit) {
      if (MULTI) {
        for (int j = l; j < level; ++j) row[j + 1] = -1;
      } else {
        row[0] = -1;
      }
      return;
    }
    if (MULTI) row[l + 1] = ord;
  }
  if (!MULTI) row[0] = ord;
}
template <typename T, bool MULTI>
int sp_query(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree, const int32_t* exsum, const void* coords,
             int64_t* pidx) {
  if (level < 0 || level > SP_MAX_LEVEL || num_bytes < 0) return (int)hipErrorInvalidValue;
  if (Q <= 0) return 0;
  if ((Q + 255) / 256 > 0x7FFFFFFFLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((sp_query_kernel<T, MULTI>), dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Q, level,
                     num_bytes, octree, exsum, (const T*)coords, pidx);
  KAMD_RETURN_LAST_ERROR();
}

// ---- to_dense ------------------------------------------------------------------------------------------------------------------------
// meta: the B + 1 prefix of the items' rows at the level, then every item's first point of the level.  Row r of item b is point
// meta[B + 1 + b] + (r - meta[b]); its cell is grid[b][c][x][y][z] (ToDenseKernelForward, feature_grids_cuda.cu:28-43).
template <typename T, bool BACKWARD>
__global__ __launch_bounds__(256) void sp_to_dense_kernel(int64_t B, int64_t C, int E, int64_t rows, int64_t num_points,
                                                          const int16_t* __restrict__ points, const int64_t* __restrict__ meta,
                                                          const T* __restrict__ src, T* __restrict__ dst) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < rows * C; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / C, c = e - r * C;
    int64_t lo = 0, hi = B - 1;  // the last item whose first row is <= r
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (meta[mid] <= r)
        lo = mid;
      else
        hi = mid - 1;
    }
    const int64_t p = meta[B + 1 + lo] + (r - meta[lo]);
    bool ok = p >= 0 && p < num_points;  // the point's row
    int x = 0, y = 0, z = 0;
    if (ok) {
      x = points[3 * p], y = points[3 * p + 1], z = points[3 * p + 2];
      ok = x >= 0 && y >= 0 && z >= 0 && x < E && y < E && z < E;  // the cell
    }
    const int64_t cell = ((((int64_t)lo * C + c) * E + x) * E + y) * E + z;
    if (BACKWARD)
      dst[e] = ok ? src[cell] : (T)0;
    else if (ok)
      dst[cell] = src[e];
  }
}
template <typename T, bool BACKWARD>
int sp_to_dense(void* stream, int64_t B, int64_t C, int level, int64_t rows, int64_t num_points, const int16_t* points,
                const int64_t* meta, const T* src, T* dst) {
  if (level < 0 || level > SP_MAX_LEVEL || B < 0 || C < 0 || rows < 0) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int E = 1 << level;
  if (!BACKWARD) KAMD_CHECK(kamd_zero_async(dst, (size_t)B * (size_t)C * (size_t)E * E * E * sizeof(T), st));
  if (B == 0 || rows * C <= 0) return 0;
  hipLaunchKernelGGL((sp_to_dense_kernel<T, BACKWARD>), dim3(sp_grid(rows * C)), dim3(256), 0, st, B, C, E, rows, num_points, points,
                     meta, src, dst);
  KAMD_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {

int kamd_spc_points_to_morton(void* stream, int64_t n, const int16_t* points, int64_t* morton) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(sp_points_to_morton_kernel, dim3(sp_grid(n)), dim3(256), 0, (hipStream_t)stream, n, points, morton);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spc_morton_to_points(void* stream, int64_t n, const int64_t* morton, int16_t* points) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(sp_morton_to_points_kernel, dim3(sp_grid(n)), dim3(256), 0, (hipStream_t)stream, n, morton, points);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spc_points_to_corners(void* stream, int64_t n, const int16_t* points, int16_t* corners) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(sp_points_to_corners_kernel, dim3(sp_grid(n * 8)), dim3(256), 0, (hipStream_t)stream, n, points, corners);
  KAMD_RETURN_LAST_ERROR();
}

size_t kamd_spc_octree_workspace(int64_t n, int level) {
  if (n <= 0 || level < 1 || level > SP_MAX_LEVEL) return 0;
  return sp_ws(nullptr, n, level).total_bytes;
}

int kamd_spc_octree_build(void* stream, int64_t n, int level, const int64_t* morton, int sorted, void* workspace,
                          size_t workspace_bytes, int64_t* host_sizes) {
  if (n <= 0 || level < 1 || level > SP_MAX_LEVEL || host_sizes == nullptr) return (int)hipErrorInvalidValue;
  if ((n + 255) / 256 > 0x7FFFFFFFLL) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const SpWs w = sp_ws(workspace, n, level);
  if (workspace == nullptr || workspace_bytes < w.total_bytes) return (int)hipErrorInvalidValue;
  const unsigned g = (unsigned)kamd_cdiv(n, 256);
  // the 3 * level significant bits: what lies above them is not part of a point of this level
  hipLaunchKernelGGL(sp_mask_codes_kernel, dim3(sp_grid(n)), dim3(256), 0, st, n, morton, (1ull << (3 * level)) - 1ull, w.ka);
  int64_t* cur = w.ka;
  int64_t* nxt = w.kb;
  if (!sorted) {
    const SsPasses passes = ss_passes_low(3 * level);
    if (passes.count & 1) cur = w.kb, nxt = w.ka;  // where the last of an odd number of passes leaves the codes of A
    KAMD_CHECK(ss_sort(st, n, passes, w.ka, nxt, cur, w.sort));
  }
  // one code per run of equal codes (with `sorted` the input is unique already: every code is a head)
  KAMD_CHECK(ss_heads_scan(st, n, (const int64_t*)nullptr, cur, 0, w.flag, w.pos, w.sums));
  hipLaunchKernelGGL(sp_unique_kernel, dim3(g), dim3(256), 0, st, n, (const int64_t*)cur, (const int*)w.flag, (const int64_t*)w.pos,
                     nxt, w.sizes);
  {
    int64_t* t = cur;
    cur = nxt;
    nxt = t;
  }
  // level l - 1 from the codes of level l; the counts stay on the device (grids sized by the bound n)
  for (int l = level; l > 0; --l) {
    const int64_t* n_ptr = (l == level) ? w.sizes : w.sizes + 1 + l;
    KAMD_CHECK(ss_heads_scan(st, n, n_ptr, cur, 3, w.flag, w.pos, w.sums));
    hipLaunchKernelGGL(ms_parents_kernel, dim3(g), dim3(256), 0, st, n_ptr, (const int64_t*)cur, (const int*)w.flag,
                       (const int64_t*)w.pos, nxt, w.level_bytes + (size_t)(l - 1) * (size_t)n, w.sizes + 1 + (l - 1));
    int64_t* t = cur;
    cur = nxt;
    nxt = t;
  }
  KAMD_CHECK(hipGetLastError());
  // the one host read of the call: unique codes and nodes per level size the octree
  KAMD_CHECK(hipMemcpyAsync(host_sizes, w.sizes, (size_t)(1 + level) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  KAMD_CHECK(hipStreamSynchronize(st));
  return 0;
}

int kamd_spc_octree_gather(void* stream, int64_t n, int level, const void* workspace, int64_t octree_bytes, uint8_t* octree) {
  if (n <= 0 || level < 1 || level > SP_MAX_LEVEL) return (int)hipErrorInvalidValue;
  if (octree_bytes <= 0) return 0;
  const SpWs w = sp_ws(const_cast<void*>(workspace), n, level);
  // (octree_bytes is the sum of the level sizes the kernel reads from the workspace: the host read them from there)
  hipLaunchKernelGGL(ms_gather_octree_kernel, dim3(sp_grid(octree_bytes)), dim3(256), 0, (hipStream_t)stream, level, n,
                     (const int64_t*)w.sizes, (const unsigned char*)w.level_bytes, octree);
  KAMD_RETURN_LAST_ERROR();
}

size_t kamd_spc_scan_workspace(int64_t total_bytes, int64_t B) {
  if (total_bytes <= 0 || B <= 0) return 0;
  auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  return pad(ss_scan_sums_entries(total_bytes) * 8) + pad((size_t)B * SP_PYR_ITEM * 4) + pad((size_t)B * 4);
}

int kamd_spc_scan_octrees(void* stream, int64_t total_bytes, int64_t B, const uint8_t* octrees, const int64_t* starts,
                          int32_t* exsum, void* workspace, int32_t* host_pyramids) {
  if (total_bytes <= 0 || B <= 0 || total_bytes * 8 >= (1LL << 31) || workspace == nullptr || host_pyramids == nullptr)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  char* p = (char*)workspace;
  int64_t* sums = (int64_t*)p;
  p += pad(ss_scan_sums_entries(total_bytes) * 8);
  int* pyr = (int*)p;
  p += pad((size_t)B * SP_PYR_ITEM * 4);
  int* base = (int*)p;
  KAMD_CHECK(ss_scan_inclusive(st, total_bytes, octrees, exsum, sums));
  hipLaunchKernelGGL(sp_pyramid_kernel, dim3((unsigned)kamd_cdiv(B, 256)), dim3(256), 0, st, B, total_bytes, starts,
                     (const int*)exsum, pyr, base);
  hipLaunchKernelGGL(sp_rebase_kernel, dim3(sp_grid(total_bytes)), dim3(256), 0, st, total_bytes, B, starts, (const int*)base, exsum);
  KAMD_CHECK(hipGetLastError());
  // the one host read of the call, whatever B and the depth are
  KAMD_CHECK(hipMemcpyAsync(host_pyramids, pyr, (size_t)B * SP_PYR_ITEM * sizeof(int), hipMemcpyDeviceToHost, st));
  KAMD_CHECK(hipStreamSynchronize(st));
  return 0;
}

int kamd_spc_generate_points(void* stream, int64_t B, int max_level, int64_t num_bytes, int64_t num_points,
                             const uint8_t* octrees, const int32_t* exsum, const int64_t* meta, int64_t max_level_nodes,
                             int16_t* points) {
  if (max_level < 0 || max_level > SP_MAX_LEVEL || B < 0 || B > 65535) return (int)hipErrorInvalidValue;
  if (B == 0 || num_points <= 0 || max_level_nodes <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  // level l of every item: a level has at most 8^l nodes (and at most max_level_nodes, from the CPU pyramid)
  for (int l = 0; l < max_level; ++l) {
    int64_t nodes = max_level_nodes;
    if (3 * l < 40 && nodes > (1LL << (3 * l))) nodes = 1LL << (3 * l);
    hipLaunchKernelGGL(sp_generate_level_kernel, dim3(sp_grid(nodes), (unsigned)B), dim3(256), 0, st, l, max_level, num_bytes,
                       num_points, octrees, exsum, meta, points);
  }
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spc_query_f16(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree, const int32_t* exsum,
                       const void* coords, int64_t* pidx) {
  return sp_query<__half, false>(stream, Q, level, num_bytes, octree, exsum, coords, pidx);
}
int kamd_spc_query_f32(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree, const int32_t* exsum,
                       const float* coords, int64_t* pidx) {
  return sp_query<float, false>(stream, Q, level, num_bytes, octree, exsum, coords, pidx);
}
int kamd_spc_query_f64(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree, const int32_t* exsum,
                       const double* coords, int64_t* pidx) {
  return sp_query<double, false>(stream, Q, level, num_bytes, octree, exsum, coords, pidx);
}
int kamd_spc_query_multiscale_f16(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree,
                                  const int32_t* exsum, const void* coords, int64_t* pidx) {
  return sp_query<__half, true>(stream, Q, level, num_bytes, octree, exsum, coords, pidx);
}
int kamd_spc_query_multiscale_f32(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree,
                                  const int32_t* exsum, const float* coords, int64_t* pidx) {
  return sp_query<float, true>(stream, Q, level, num_bytes, octree, exsum, coords, pidx);
}
int kamd_spc_query_multiscale_f64(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree,
                                  const int32_t* exsum, const double* coords, int64_t* pidx) {
  return sp_query<double, true>(stream, Q, level, num_bytes, octree, exsum, coords, pidx);
}

int kamd_spc_to_dense_forward_f32(void* stream, int64_t B, int64_t C, int level, int64_t rows, int64_t num_points,
                                  const int16_t* points, const int64_t* meta, const float* features, float* grid) {
  return sp_to_dense<float, false>(stream, B, C, level, rows, num_points, points, meta, features, grid);
}
int kamd_spc_to_dense_forward_f64(void* stream, int64_t B, int64_t C, int level, int64_t rows, int64_t num_points,
                                  const int16_t* points, const int64_t* meta, const double* features, double* grid) {
  return sp_to_dense<double, false>(stream, B, C, level, rows, num_points, points, meta, features, grid);
}
int kamd_spc_to_dense_backward_f32(void* stream, int64_t B, int64_t C, int level, int64_t rows, int64_t num_points,
                                   const int16_t* points, const int64_t* meta, const float* grad_grid, float* grad_features) {
  return sp_to_dense<float, true>(stream, B, C, level, rows, num_points, points, meta, grad_grid, grad_features);
}
int kamd_spc_to_dense_backward_f64(void* stream, int64_t B, int64_t C, int level, int64_t rows, int64_t num_points,
                                   const int16_t* points, const int64_t* meta, const double* grad_grid, double* grad_features) {
  return sp_to_dense<double, true>(stream, B, C, level, rows, num_points, points, meta, grad_grid, grad_features);
}

}  // extern "C"
