// ops.mesh per-vertex sums and means of per-face-corner features (average_face_vertex_features, compute_vertex_normals, the sum of
// vertex_tangents) without atomics, in a fixed order.
//
// The reference (kaolin/ops/mesh/mesh.py average_face_vertex_features, trianglemesh.py vertex_tangents) adds with scatter_add_, once
// per corner slot: float atomics on a GPU.  On the CPU the same expression is a sequential sum, per vertex, over the corners that
// hold it in the order (corner slot k ascending, then face f ascending), one rounded addition per corner starting from +0, followed
// by ONE division by max(count, 1).  That order is the contract here:
//   * the topology, once per `faces` (kamd_vertex_corners_build): one thread per corner i = k F + f writes the key (i << 32) |
//     faces[f, k]; the stable keys-only sort of sort_scan.h over the low ceil(log2 V) bits groups the corners by vertex and keeps
//     equal vertices in ascending i; offsets[v] = the first sorted position whose vertex is >= v (a binary search: no scan, no
//     compaction), corners[j] = the high word of the j-th sorted key;
//   * every step (kamd_vertex_gather_*): ONE launch.  A group of g = min(64, next power of two >= N) lanes owns one (b, v), lanes
//     along N, and walks corners[offsets[v] .. offsets[v + 1]) in order.  No atomics, no reduction across corners;
//   * its gradient (kamd_vertex_gather_backward_*): ONE launch, grad[b, f, k, :] = grad_out[b, faces[f, k], :] (/ max(count, 1)).
// Every index that comes from data is compared with its buffer's size before use: a vertex id with V (the key kernel counts the ids
// outside [0, V) for the host and files them under vertex 0), a corner index with K F, an offset with K F.
#include <hip/hip_runtime.h>
#include "common.h"
#include "sort_scan.h"
#include "../../include/kaolin_amd.h"

namespace {

// faces[f, k] through its element strides; int32 or int64 entries
__device__ __forceinline__ long long vf_face(const void* faces, int wide, long long f, long long k, long long stride_f,
                                             long long stride_k) {
  const long long at = f * stride_f + k * stride_k;
  return wide ? ((const long long*)faces)[at] : (long long)((const int*)faces)[at];
}

// ---- the topology -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vf_keys_kernel(long long n, long long F, long long V, const void* __restrict__ faces, int wide,
                                                      long long stride_f, long long stride_k, unsigned long long* __restrict__ keys,
                                                      int* __restrict__ bad) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  long long v = vf_face(faces, wide, i % F, i / F, stride_f, stride_k);
  if (v < 0 || v >= V) {  // guard: a vertex id outside the V vertices is counted and filed under vertex 0
    atomicAdd(bad, 1);
    v = 0;
  }
  keys[i] = ((unsigned long long)i << 32) | (unsigned long long)v;
}
__global__ __launch_bounds__(64) void vf_clear_kernel(int* bad) {
  if (threadIdx.x == 0) *bad = 0;
}
// thread j < n: corners[j]; thread v <= V: offsets[v] = the first sorted position whose vertex (the low word) is >= v
__global__ __launch_bounds__(256) void vf_lists_kernel(long long n, long long V, const unsigned long long* __restrict__ sorted,
                                                       int* __restrict__ offsets, int* __restrict__ corners) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < n) {
    const unsigned long long c = sorted[t] >> 32;
    corners[t] = c < (unsigned long long)n ? (int)c : 0;  // guard: a corner index outside the K F corners
  }
  if (t <= V) {
    long long lo = 0, hi = n;  // the answer stays in [0, n] whatever the keys hold
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if ((long long)(sorted[mid] & 0xFFFFFFFFull) < t)
        lo = mid + 1;
      else
        hi = mid;
    }
    offsets[t] = (int)lo;
  }
}

// workspace for n corners: keys | the other side of the ping-pong | sorted keys | the sort's scratch | the count of bad ids
struct VfWs {
  unsigned long long *k0, *kt, *ks;
  SsSortWs sort;
  int* bad;
  size_t total_bytes;
};
VfWs vf_ws(void* base, long long n) {
  VfWs w;
  char* p = (char*)base;
  auto take = [&](size_t bytes) {
    char* r = p;
    p += (bytes + 255) & ~(size_t)255;
    return r;
  };
  const size_t n1 = (size_t)(n > 0 ? n : 1);
  w.k0 = (unsigned long long*)take(n1 * 8);
  w.kt = (unsigned long long*)take(n1 * 8);
  w.ks = (unsigned long long*)take(n1 * 8);
  w.sort.hist = (int*)take(ss_sort_hist_entries(n) * 4);
  w.sort.offs = (long long*)take(ss_sort_offs_entries(n) * 8);
  w.sort.sums = (long long*)take(ss_sort_sums_entries(n) * 8);
  w.bad = (int*)take(4);
  w.total_bytes = (size_t)(p - (char*)base);
  return w;
}
bool vf_extents(long long F, long long K, long long V) {
  return F > 0 && K > 0 && V > 0 && V < 0x7FFFFFFFLL && F < 0x7FFFFFFFLL && K < 0x7FFFFFFFLL && F * K < 0x7FFFFFFFLL;
}
int vf_bits(long long V) {  // ceil(log2 V): the bits that tell the ids 0 .. V - 1 apart
  int bits = 0;
  while (bits < 31 && (1LL << bits) < V) ++bits;
  return bits;
}

// ---- the gather -------------------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T vf_load(const T* __restrict__ feats, int c, unsigned n, unsigned F, long long stride_f, long long stride_k) {
  if ((unsigned)c >= n) return (T)0;  // guard: a corner index outside the K F corners adds nothing
  const unsigned k = (unsigned)c / F, f = (unsigned)c - k * F;
  return feats[(long long)f * stride_f + (long long)k * stride_k];
}
constexpr int VF_BATCH = 8;  // corners whose loads are issued together (a vertex of an ordinary mesh has 6: one batch)
// G lanes per (b, v); a lane owns the channels lane, lane + G, ...
template <typename T>
__global__ __launch_bounds__(256) void vf_gather_kernel(long long groups, int G, long long V, long long N, unsigned n, unsigned F,
                                                        const T* __restrict__ feats, long long stride_b, long long stride_f,
                                                        long long stride_k, long long stride_n, const int* __restrict__ offsets,
                                                        const int* __restrict__ corners, int mean, T* __restrict__ out) {
  const long long gid = ((long long)blockIdx.x * 256 + threadIdx.x) / G;
  const int lane = (int)(threadIdx.x % G);
  if (gid >= groups) return;
  const long long b = gid / V, v = gid - b * V;
  int s = offsets[v], e = offsets[v + 1];
  if (s < 0 || e < s || (unsigned)e > n) s = e = 0;  // guard: offsets outside the K F corners
  const T denom = (T)(e - s > 1 ? e - s : 1);
  for (long long d = lane; d < N; d += G) {
    const T* src = feats + b * stride_b + d * stride_n;
    T acc = (T)0;
    for (int j = s; j < e; j += VF_BATCH) {  // the loads of a batch of corners in flight; the additions stay in order
      int c[VF_BATCH];
      T x[VF_BATCH];
#pragma unroll
      for (int i = 0; i < VF_BATCH; ++i) c[i] = j + i < e ? corners[j + i] : -1;  // (-1: past the list, nothing is loaded)
#pragma unroll
      for (int i = 0; i < VF_BATCH; ++i) x[i] = vf_load(src, c[i], n, F, stride_f, stride_k);
#pragma unroll
      for (int i = 0; i < VF_BATCH; ++i)
        if (j + i < e) acc = acc + x[i];
    }
    out[(b * V + v) * N + d] = mean ? acc / denom : acc;
  }
}
template <typename T>
int vf_gather(void* stream, int64_t B, int64_t F, int64_t K, int64_t V, int64_t N, const T* feats, int64_t stride_b, int64_t stride_f,
              int64_t stride_k, int64_t stride_n, const int32_t* offsets, const int32_t* corners, int mean, T* out) {
  if (B <= 0 || N <= 0 || !vf_extents(F, K, V) || feats == nullptr || offsets == nullptr || corners == nullptr || out == nullptr)
    return (int)hipErrorInvalidValue;
  int G = 1;
  while (G < 64 && G < N) G <<= 1;
  const long long groups = B * V;
  const long long blocks = (groups * G + 255) / 256;
  if (groups / V != B || blocks > 0x7FFFFFFFLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((vf_gather_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, groups, G, (long long)V,
                     (long long)N, (unsigned)(F * K), (unsigned)F, feats, (long long)stride_b, (long long)stride_f,
                     (long long)stride_k, (long long)stride_n, offsets, corners, mean, out);
  KAMD_RETURN_LAST_ERROR();
}

// one thread per element of grad (B, F, K, N) contiguous
template <typename T>
__global__ __launch_bounds__(256) void vf_backward_kernel(long long total, long long F, long long K, long long V, long long N,
                                                          long long n, const T* __restrict__ grad_out, long long stride_b,
                                                          long long stride_v, long long stride_n, const void* __restrict__ faces,
                                                          int wide, long long fstride_f, long long fstride_k,
                                                          const int* __restrict__ offsets, int mean, T* __restrict__ grad) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long d = i % N, r = i / N, k = r % K, q = r / K, f = q % F, b = q / F;
  const long long v = vf_face(faces, wide, f, k, fstride_f, fstride_k);
  T g = (T)0;
  if (v >= 0 && v < V) {  // guard: a vertex id outside the V vertices takes no gradient
    g = grad_out[b * stride_b + v * stride_v + d * stride_n];
    if (mean) {
      const int s = offsets[v], e = offsets[v + 1];
      const long long count = (s >= 0 && e >= s && e <= n) ? e - s : 0;  // guard: offsets outside the K F corners
      g = g / (T)(count > 1 ? count : 1);
    }
  }
  grad[i] = g;
}
template <typename T>
int vf_backward(void* stream, int64_t B, int64_t F, int64_t K, int64_t V, int64_t N, const T* grad_out, int64_t stride_b,
                int64_t stride_v, int64_t stride_n, const void* faces, int faces_bytes, int64_t fstride_f, int64_t fstride_k,
                const int32_t* offsets, int mean, T* grad) {
  if (B <= 0 || N <= 0 || !vf_extents(F, K, V) || grad_out == nullptr || faces == nullptr || offsets == nullptr || grad == nullptr)
    return (int)hipErrorInvalidValue;
  if (faces_bytes != 4 && faces_bytes != 8) return (int)hipErrorInvalidValue;
  const long long n = F * K;
  if (B > 0x7FFFFFFFFFFFLL / n || B * n > 0x7FFFFFFFFFFFLL / N) return (int)hipErrorInvalidValue;
  const long long total = B * n * N, blocks = (total + 255) / 256;
  if (blocks > 0x7FFFFFFFLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((vf_backward_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, total, (long long)F,
                     (long long)K, (long long)V, (long long)N, n, grad_out, (long long)stride_b, (long long)stride_v,
                     (long long)stride_n, faces, faces_bytes == 8 ? 1 : 0, (long long)fstride_f, (long long)fstride_k, offsets, mean,
                     grad);
  KAMD_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {

size_t kamd_vertex_corners_workspace(int64_t F, int64_t K, int64_t V) {
  if (!vf_extents(F, K, V)) return 0;
  return vf_ws(nullptr, F * K).total_bytes;
}

int kamd_vertex_corners_build(void* stream, int64_t F, int64_t K, int64_t V, const void* faces, int faces_bytes, int64_t stride_f,
                              int64_t stride_k, void* workspace, size_t workspace_bytes, int32_t* offsets, int32_t* corners,
                              int32_t* host_bad) {
  if (!vf_extents(F, K, V) || faces == nullptr || offsets == nullptr || corners == nullptr || host_bad == nullptr)
    return (int)hipErrorInvalidValue;
  if (faces_bytes != 4 && faces_bytes != 8) return (int)hipErrorInvalidValue;
  const long long n = F * K;
  if (workspace == nullptr || workspace_bytes < vf_ws(nullptr, n).total_bytes) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const VfWs w = vf_ws(workspace, n);
  hipLaunchKernelGGL(vf_clear_kernel, dim3(1), dim3(64), 0, st, w.bad);
  hipLaunchKernelGGL(vf_keys_kernel, dim3(ss_grid(n, 256)), dim3(256), 0, st, n, (long long)F, (long long)V, faces,
                     faces_bytes == 8 ? 1 : 0, (long long)stride_f, (long long)stride_k, w.k0, w.bad);
  KAMD_CHECK(hipGetLastError());
  KAMD_CHECK(ss_sort(st, n, ss_passes_low(vf_bits(V)), w.k0, w.kt, w.ks, w.sort));
  const long long threads = n > V + 1 ? n : V + 1;
  hipLaunchKernelGGL(vf_lists_kernel, dim3(ss_grid(threads, 256)), dim3(256), 0, st, n, (long long)V,
                     (const unsigned long long*)w.ks, offsets, corners);
  KAMD_CHECK(hipGetLastError());
  int bad = 0;
  KAMD_CHECK(hipMemcpyAsync(&bad, w.bad, 4, hipMemcpyDeviceToHost, st));  // the one host read
  KAMD_CHECK(hipStreamSynchronize(st));
  *host_bad = bad;
  return 0;
}

int kamd_vertex_gather_f32(void* stream, int64_t B, int64_t F, int64_t K, int64_t V, int64_t N, const float* face_features,
                           int64_t stride_b, int64_t stride_f, int64_t stride_k, int64_t stride_n, const int32_t* offsets,
                           const int32_t* corners, int mean, float* out) {
  return vf_gather<float>(stream, B, F, K, V, N, face_features, stride_b, stride_f, stride_k, stride_n, offsets, corners, mean, out);
}
int kamd_vertex_gather_f64(void* stream, int64_t B, int64_t F, int64_t K, int64_t V, int64_t N, const double* face_features,
                           int64_t stride_b, int64_t stride_f, int64_t stride_k, int64_t stride_n, const int32_t* offsets,
                           const int32_t* corners, int mean, double* out) {
  return vf_gather<double>(stream, B, F, K, V, N, face_features, stride_b, stride_f, stride_k, stride_n, offsets, corners, mean, out);
}
int kamd_vertex_gather_backward_f32(void* stream, int64_t B, int64_t F, int64_t K, int64_t V, int64_t N, const float* grad_out,
                                    int64_t stride_b, int64_t stride_v, int64_t stride_n, const void* faces, int faces_bytes,
                                    int64_t faces_stride_f, int64_t faces_stride_k, const int32_t* offsets, int mean, float* grad) {
  return vf_backward<float>(stream, B, F, K, V, N, grad_out, stride_b, stride_v, stride_n, faces, faces_bytes, faces_stride_f,
                            faces_stride_k, offsets, mean, grad);
}
int kamd_vertex_gather_backward_f64(void* stream, int64_t B, int64_t F, int64_t K, int64_t V, int64_t N, const double* grad_out,
                                    int64_t stride_b, int64_t stride_v, int64_t stride_n, const void* faces, int faces_bytes,
                                    int64_t faces_stride_f, int64_t faces_stride_k, const int32_t* offsets, int mean, double* grad) {
  return vf_backward<double>(stream, B, F, K, V, N, grad_out, stride_b, stride_v, stride_n, faces, faces_bytes, faces_stride_f,
                             faces_stride_k, offsets, mean, grad);
}

}  // extern "C"
