// ops.mesh.subdivide_trianglemesh: one iteration of Loop subdivision with a per-vertex smoothing factor alpha (the reference is a
// row-wise torch.unique(dim=0), a second unique for the adjacency, a legacy sparse bmm, two further sorts and about twenty
// gathers, cats and masked adds per iteration, kaolin/ops/mesh/trianglemesh.py).
//
//     edge slots of a face (a, b, c)     ab bc ca, opposite corners c a b; an edge is the pair (min, max) of its ends, a
//                                        self-edge (v, v) included
//     E unique edges, numbered in ascending (min, max) order; edge e is the new vertex V + e
//     count[e]                           the face slots holding edge e
//     n[v]                               the unique edges holding v (a self-edge once; the neighbour sum then includes x[v])
//     old row v, n[v] > 0                (1 - alpha[v]) x[v] + alpha[v] / n[v] * sum of x[u] over the neighbours u; alpha given, or
//                                        5/8 - (3/8 + cos(2 pi / n) / 4)^2 (9/16 at n = 3); n[v] = 0: the row is copied
//     new row V + e, channels x y z alpha   count[e] == 2: (3 (x[lo] + x[hi]) + (x[opp0] + x[opp1])) / 8; else (x[lo] + x[hi]) / 2
//     new_faces, four rows per face      (b bc ab) (a ab ca) (c ca bc) (ca ab bc)
//
// TOPOLOGY (once per iteration: it does not depend on the batch)
//   1. sl_keys_kernel     the three keys min << 32 | max of face f at keys[3 f ..].
//   2. sort               sort_scan.h: stable 8-bit LSD radix sort of the keys alone, over the digits below ceil(log2 V) of either
//                         half only.
//   3. heads / scan / unique   the unique keys ARE the edge list.  The HOST reads E -- the one stream synchronisation.
//   4. sl_edges_kernel    unique keys -> edges (E, 2) int64 and the swapped keys max << 32 | min.
//      sl_emit_kernel     per face: ranks its three keys by binary search in the unique keys, writes its four child rows (six
//                         16-byte stores) and claims a slot of opp[e] for each opposite corner with an int atomic on count[e]
//                         (claims beyond the second only count).  Which corner lands in slot 0 is not fixed; the values add the
//                         two slots to each other first, so no bit depends on it.
//   5. second sort        of the E swapped keys: the transposed list.  sl_transposed_kernel turns it into (min end, edge id) rows,
//                         sl_runs_kernel into the per-vertex run starts of both lists and the valences: the neighbours of v are
//                         the max ends of the run of edges with min = v and the min ends of the run of swapped keys with max = v
//                         (a self-edge ends the second run and is skipped there).
// VALUES (per batch item; float and double)
//   forward   ONE launch, a thread per (row, channel) of (V + E, 3 or 4): gathers only, sums in list order; no atomics.
//   backward  sl_backward_gather_kernel: a thread per (vertex, channel): the vertex-rule terms and the terms of the edge ends are
//             gathers over the same two runs (the adjacency is symmetric); a plain store, which also initialises the result.
//             sl_backward_opp_kernel: the 1/8 terms of the opposite corners, one native fp atomic add per (edge, slot, channel).
// Every kernel is a plain bounded launch; none waits on another workgroup.
#include "common.h"
#include "sort_scan.h"
#include "subdivide_trianglemesh_host.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr unsigned long long SL_LOW = 0xffffffffull;

__device__ __forceinline__ unsigned long long sl_key(unsigned long long p, unsigned long long q) {
  return p < q ? (p << 32) | q : (q << 32) | p;
}

// ---- 1. keys --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sl_keys_kernel(const int64_t* __restrict__ faces, long long F,
                                                      unsigned long long* __restrict__ keys) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  // ids in [0, V), V < 2^32: the shim has checked the range
  const unsigned long long a = (unsigned long long)faces[3 * f], b = (unsigned long long)faces[3 * f + 1],
                           c = (unsigned long long)faces[3 * f + 2];
  keys[3 * f] = sl_key(a, b);
  keys[3 * f + 1] = sl_key(b, c);
  keys[3 * f + 2] = sl_key(c, a);
}

// ---- 4. results -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sl_edges_kernel(long long E, const unsigned long long* __restrict__ uniq,
                                                       int64_t* __restrict__ edges, unsigned long long* __restrict__ swapped) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const unsigned long long key = uniq[e];
  ((ulonglong2*)edges)[e] = make_ulonglong2(key >> 32, key & SL_LOW);
  swapped[e] = (key << 32) | (key >> 32);
}

__global__ __launch_bounds__(256) void sl_emit_kernel(const int64_t* __restrict__ faces, long long F, unsigned long long V,
                                                      const unsigned long long* __restrict__ uniq, long long E,
                                                      int64_t* __restrict__ new_faces, int* __restrict__ count,
                                                      int64_t* __restrict__ opp) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const unsigned long long a = (unsigned long long)faces[3 * f], b = (unsigned long long)faces[3 * f + 1],
                           c = (unsigned long long)faces[3 * f + 2];
  const unsigned long long k[3] = {sl_key(a, b), sl_key(b, c), sl_key(c, a)}, corner[3] = {c, a, b};
  unsigned long long r[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const long long e = ss_rank(uniq, E, k[s]);  // in [0, E): the key is one of the sorted keys
    r[s] = V + (unsigned long long)e;
    const int slot = atomicAdd(&count[e], 1);
    if (slot < 2) opp[2 * e + slot] = (int64_t)corner[s];
  }
  const unsigned long long ab = r[0], bc = r[1], ca = r[2];
  ulonglong2* out = (ulonglong2*)new_faces + 6 * f;  // rows 4 f .. 4 f + 3: 96 bytes from a 16-byte aligned base
  out[0] = make_ulonglong2(b, bc);
  out[1] = make_ulonglong2(ab, a);
  out[2] = make_ulonglong2(ab, ca);
  out[3] = make_ulonglong2(c, ca);
  out[4] = make_ulonglong2(bc, ca);
  out[5] = make_ulonglong2(ab, bc);
}

// ---- 5. the transposed list and the runs ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sl_transposed_kernel(long long E, const unsigned long long* __restrict__ uniq,
                                                            const unsigned long long* __restrict__ swapped,
                                                            int64_t* __restrict__ tlist) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= E) return;
  const unsigned long long key = swapped[j];  // max << 32 | min, the j-th in ascending order
  const long long e = ss_rank(uniq, E, (key << 32) | (key >> 32));
  ((ulonglong2*)tlist)[j] = make_ulonglong2(key & SL_LOW, (unsigned long long)e);
}

// first i in [0, n) whose key's high half is >= v
__device__ __forceinline__ long long sl_first_high(const unsigned long long* __restrict__ keys, long long n, unsigned long long v) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if ((keys[mid] >> 32) < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void sl_runs_kernel(long long V, long long E, const unsigned long long* __restrict__ uniq,
                                                      const unsigned long long* __restrict__ swapped, int64_t* __restrict__ runs,
                                                      int* __restrict__ valence) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const long long m0 = sl_first_high(uniq, E, (unsigned long long)v), m1 = sl_first_high(uniq, E, (unsigned long long)v + 1);
  const long long t0 = sl_first_high(swapped, E, (unsigned long long)v), t1 = sl_first_high(swapped, E, (unsigned long long)v + 1);
  ((ulonglong2*)runs)[v] = make_ulonglong2((unsigned long long)m0, (unsigned long long)t0);
  if (v == V - 1) ((ulonglong2*)runs)[V] = make_ulonglong2((unsigned long long)m1, (unsigned long long)t1);
  // the self-edge (v, v) is in both runs (it ends the second: v is the largest min end an edge with max = v can have)
  const bool self = t1 > t0 && (swapped[t1 - 1] & SL_LOW) == (unsigned long long)v;
  valence[v] = (int)((m1 - m0) + (t1 - t0) - (self ? 1 : 0));
}

// ---- values -----------------------------------------------------------------------------------------------------------------
struct SlTopo {
  const int64_t* edges;  // (E, 2) (min, max), ascending
  const int* count;      // (E)
  const int64_t* opp;    // (E, 2): the opposite corners of the first two face slots; read where count == 2 only
  const int64_t* tlist;  // (E, 2): (min end, edge id) in ascending (max, min) order
  const int64_t* runs;   // (V + 1, 2): where the runs of vertex v start in edges and in tlist
  const int* valence;    // (V)
};

__device__ __forceinline__ float sl_cos(float x) { return cosf(x); }
__device__ __forceinline__ double sl_cos(double x) { return cos(x); }
template <typename T>
__device__ __forceinline__ T sl_default_alpha(int n) {  // n > 0
  if (n == 3) return (T)0.5625;
  const T s = (T)0.375 + (T)0.25 * sl_cos((T)6.283185307179586 / (T)n);
  return (T)0.625 - s * s;
}

// x (B, V, 3) and alpha (B, V) or null (the default alpha), items `xbs` / `abs` elements apart; new_x (B, V + E, 3) and new_alpha
// (B, V + E), written when alpha is given.  Every id read from the topology is in [0, V) or [0, E): the topology stage made it.
template <typename T>
__global__ __launch_bounds__(256) void sl_forward_kernel(SlTopo tp, long long B, long long V, long long E, const T* __restrict__ X,
                                                         long long xbs, const T* __restrict__ A, long long abs_,
                                                         T* __restrict__ new_x, T* __restrict__ new_alpha) {
  const int C = A != nullptr ? 4 : 3;
  const long long R = V + E, j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= R * C) return;
  const long long row = j / C;
  const int ch = (int)(j - row * C);
  long long m0 = 0, m1 = 0, t0 = 0, t1 = 0, lo = 0, hi = 0, o0 = 0, o1 = 0;
  int n = 0;
  bool two = false;
  if (row < V) {
    if (ch < 3) {
      n = tp.valence[row];
      m0 = tp.runs[2 * row], t0 = tp.runs[2 * row + 1], m1 = tp.runs[2 * row + 2], t1 = tp.runs[2 * row + 3];
    }
  } else {
    const long long e = row - V;
    lo = tp.edges[2 * e], hi = tp.edges[2 * e + 1];
    two = tp.count[e] == 2;
    if (two) o0 = tp.opp[2 * e], o1 = tp.opp[2 * e + 1];
  }
  for (long long b = blockIdx.y; b < B; b += gridDim.y) {
    const T* x = X + b * xbs;
    const T* al = A != nullptr ? A + b * abs_ : nullptr;
    T out;
    if (row < V) {
      if (ch == 3) {
        out = al[row];
      } else {
        const T xv = x[row * 3 + ch];
        out = xv;
        if (n > 0) {
          T sum = (T)0;
          for (long long e = m0; e < m1; ++e) sum += x[tp.edges[2 * e + 1] * 3 + ch];
          for (long long k = t0; k < t1; ++k) {
            const long long u = tp.tlist[2 * k];
            if (u != row) sum += x[u * 3 + ch];
          }
          const T a = al != nullptr ? al[row] : sl_default_alpha<T>(n);
          out = ((T)1 - a) * xv + a / (T)n * sum;
        }
      }
    } else {
      const T ends = ch < 3 ? x[lo * 3 + ch] + x[hi * 3 + ch] : al[lo] + al[hi];
      if (two) {
        const T far = ch < 3 ? x[o0 * 3 + ch] + x[o1 * 3 + ch] : al[o0] + al[o1];
        out = (ends * (T)3 + far) * (T)0.125;
      } else {
        out = ends * (T)0.5;
      }
    }
    if (ch < 3)
      new_x[(b * R + row) * 3 + ch] = out;
    else
      new_alpha[b * R + row] = out;
  }
}

// GX (B, V + E, 3) and GA (B, V + E) or null: the incoming gradients; dx (B, V, 3) and da (B, V) or null: fully written.
template <typename T>
__global__ __launch_bounds__(256) void sl_backward_gather_kernel(SlTopo tp, long long B, long long V, long long E,
                                                                 const T* __restrict__ GX, const T* __restrict__ GA,
                                                                 const T* __restrict__ X, long long xbs, const T* __restrict__ A,
                                                                 long long abs_, T* __restrict__ dx, T* __restrict__ da) {
  const int C = da != nullptr ? 4 : 3;
  const long long R = V + E, j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= V * C) return;
  const long long v = j / C;
  const int ch = (int)(j - v * C);
  const int n = tp.valence[v];
  const long long m0 = tp.runs[2 * v], t0 = tp.runs[2 * v + 1], m1 = tp.runs[2 * v + 2], t1 = tp.runs[2 * v + 3];
  for (long long b = blockIdx.y; b < B; b += gridDim.y) {
    const T* gx = GX + b * R * 3;
    const T* ga = GA != nullptr ? GA + b * R : nullptr;
    const T* x = X + b * xbs;
    const T* al = A != nullptr ? A + b * abs_ : nullptr;
    T acc;
    if (ch < 3) {
      const T a = n > 0 ? (al != nullptr ? al[v] : sl_default_alpha<T>(n)) : (T)0;
      acc = ((T)1 - a) * gx[v * 3 + ch];
      for (long long e = m0; e < m1; ++e) {
        const long long u = tp.edges[2 * e + 1];
        const int nu = tp.valence[u];  // > 0: u is an end of edge e
        const T au = al != nullptr ? al[u] : sl_default_alpha<T>(nu);
        acc += au / (T)nu * gx[u * 3 + ch];
        acc += (tp.count[e] == 2 ? (T)0.375 : (T)0.5) * gx[(V + e) * 3 + ch];
      }
      for (long long k = t0; k < t1; ++k) {
        const long long u = tp.tlist[2 * k], e = tp.tlist[2 * k + 1];
        if (u != v) {
          const int nu = tp.valence[u];
          const T au = al != nullptr ? al[u] : sl_default_alpha<T>(nu);
          acc += au / (T)nu * gx[u * 3 + ch];
        }
        acc += (tp.count[e] == 2 ? (T)0.375 : (T)0.5) * gx[(V + e) * 3 + ch];  // (a self-edge holds v twice: once per run)
      }
    } else {
      acc = ga != nullptr ? ga[v] : (T)0;
      if (n > 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          T sum = (T)0;
          for (long long e = m0; e < m1; ++e) sum += x[tp.edges[2 * e + 1] * 3 + c];
          for (long long k = t0; k < t1; ++k) {
            const long long u = tp.tlist[2 * k];
            if (u != v) sum += x[u * 3 + c];
          }
          acc += gx[v * 3 + c] * (sum / (T)n - x[v * 3 + c]);
        }
      }
      if (ga != nullptr) {
        for (long long e = m0; e < m1; ++e) acc += (tp.count[e] == 2 ? (T)0.375 : (T)0.5) * ga[V + e];
        for (long long k = t0; k < t1; ++k) {
          const long long e = tp.tlist[2 * k + 1];
          acc += (tp.count[e] == 2 ? (T)0.375 : (T)0.5) * ga[V + e];
        }
      }
    }
    if (ch < 3)
      dx[(b * V + v) * 3 + ch] = acc;
    else
      da[b * V + v] = acc;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void sl_backward_opp_kernel(SlTopo tp, long long B, long long V, long long E,
                                                              const T* __restrict__ GX, const T* __restrict__ GA,
                                                              T* __restrict__ dx, T* __restrict__ da) {
  const int C = (da != nullptr && GA != nullptr) ? 4 : 3;
  const long long R = V + E, j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= E * C) return;
  const long long e = j / C;
  const int ch = (int)(j - e * C);
  if (tp.count[e] != 2) return;
  const long long o0 = tp.opp[2 * e], o1 = tp.opp[2 * e + 1];  // in [0, V): corners of checked faces
  for (long long b = blockIdx.y; b < B; b += gridDim.y) {
    if (ch < 3) {
      const T g = GX[(b * R + V + e) * 3 + ch] * (T)0.125;
      kamd_atomic_add(&dx[(b * V + o0) * 3 + ch], g);
      kamd_atomic_add(&dx[(b * V + o1) * 3 + ch], g);
    } else {
      const T g = GA[b * R + V + e] * (T)0.125;
      kamd_atomic_add(&da[b * V + o0], g);
      kamd_atomic_add(&da[b * V + o1], g);
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
inline SsSortWs sl_sort_ws(char* ws, const SlLayout& l) {
  return ss_sort_ws((int*)(ws + l.hist), (long long*)(ws + l.hoffs), (long long*)(ws + l.sums));
}
inline bool sl_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

int sl_edges(hipStream_t st, long long F, long long V, const int64_t* faces, void* workspace, int64_t* host_num_edges) {
  if (sl_bad_extents(F, V) || host_num_edges == nullptr) return (int)hipErrorInvalidValue;
  *host_num_edges = 0;
  if (F == 0 || V == 0) return 0;
  if (faces == nullptr || workspace == nullptr || ((uintptr_t)faces & 7) != 0 || sl_misaligned(workspace))
    return (int)hipErrorInvalidValue;
  const SlLayout l = sl_layout(F);
  char* ws = (char*)workspace;
  unsigned long long* keys = (unsigned long long*)(ws + l.keys_a);
  unsigned long long* uniq = (unsigned long long*)(ws + l.keys_b);

  hipLaunchKernelGGL(sl_keys_kernel, dim3(ss_grid(F, 256)), dim3(256), 0, st, faces, F, keys);
  KAMD_CHECK(hipGetLastError());
  KAMD_CHECK(ss_sort(st, l.n, ss_passes_halves(st_id_bits(V)), keys, uniq, keys, sl_sort_ws(ws, l)));  // in place, through keys_b
  return ss_unique(st, l.n, keys, (int*)(ws + l.flags), (long long*)(ws + l.pos), (long long*)(ws + l.sums), uniq, host_num_edges);
}

int sl_emit(hipStream_t st, long long F, long long V, const int64_t* faces, void* workspace, long long E, int64_t* edges,
            int64_t* new_faces, int* count, int64_t* opp, int64_t* tlist, int64_t* runs, int* valence) {
  if (sl_bad_extents(F, V) || E < 0 || E > 3 * F) return (int)hipErrorInvalidValue;
  if (F == 0 || V == 0 || E == 0) return 0;
  if (faces == nullptr || workspace == nullptr || edges == nullptr || new_faces == nullptr || count == nullptr || opp == nullptr ||
      tlist == nullptr || runs == nullptr || valence == nullptr)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)faces & 7) != 0 || sl_misaligned(workspace) || sl_misaligned(edges) || sl_misaligned(new_faces) ||
      sl_misaligned(opp) || sl_misaligned(tlist) || sl_misaligned(runs) || ((uintptr_t)count & 3) != 0 || ((uintptr_t)valence & 3) != 0)
    return (int)hipErrorInvalidValue;
  const SlLayout l = sl_layout(F);
  char* ws = (char*)workspace;
  unsigned long long* swapped = (unsigned long long*)(ws + l.keys_a);  // (the sorted 3 F keys are no longer needed)
  const unsigned long long* uniq = (const unsigned long long*)(ws + l.keys_b);
  KAMD_CHECK(kamd_zero_async(count, (size_t)E * 4, st));
  hipLaunchKernelGGL(sl_edges_kernel, dim3(ss_grid(E, 256)), dim3(256), 0, st, E, uniq, edges, swapped);
  hipLaunchKernelGGL(sl_emit_kernel, dim3(ss_grid(F, 256)), dim3(256), 0, st, faces, F, (unsigned long long)V, uniq, E, new_faces,
                     count, opp);
  KAMD_CHECK(hipGetLastError());
  KAMD_CHECK(ss_sort(st, E, ss_passes_halves(st_id_bits(V)), swapped, (unsigned long long*)(ws + l.keys_c), swapped,
                     sl_sort_ws(ws, l)));  // in place, through keys_c
  hipLaunchKernelGGL(sl_transposed_kernel, dim3(ss_grid(E, 256)), dim3(256), 0, st, E, uniq, (const unsigned long long*)swapped,
                     tlist);
  hipLaunchKernelGGL(sl_runs_kernel, dim3(ss_grid(V, 256)), dim3(256), 0, st, V, E, uniq, (const unsigned long long*)swapped, runs,
                     valence);
  KAMD_RETURN_LAST_ERROR();
}

// blocks of 256 over rows * 4 elements, or 0 when that many do not fit a launch
inline long long sl_blocks(long long rows) {
  const long long blocks = ss_cdiv(rows * 4, 256);
  return blocks < (1ll << 31) ? blocks : 0;
}
inline bool sl_bad_value_extents(long long B, long long V, long long E) {
  return B < 0 || V < 0 || E < 0 || V >= (1ll << 32) || E > (1ll << 37);
}
inline bool sl_bad_topo(const SlTopo& tp, long long V, long long E) {
  if (V > 0 && (tp.runs == nullptr || tp.valence == nullptr)) return true;
  return E > 0 && (tp.edges == nullptr || tp.count == nullptr || tp.opp == nullptr || tp.tlist == nullptr);
}

template <typename T>
int sl_forward(hipStream_t st, long long B, long long V, long long E, const T* vertices, long long vbs, const T* alpha,
               long long abs_, const SlTopo& tp, T* new_vertices, T* new_alpha) {
  if (sl_bad_value_extents(B, V, E) || vbs < 0 || abs_ < 0) return (int)hipErrorInvalidValue;
  if (B == 0 || V + E == 0) return 0;
  if (V == 0 || vertices == nullptr || new_vertices == nullptr || (alpha != nullptr && new_alpha == nullptr) || sl_bad_topo(tp, V, E))
    return (int)hipErrorInvalidValue;
  const long long blocks = sl_blocks(V + E);
  if (blocks == 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((sl_forward_kernel<T>), dim3((unsigned)blocks, (unsigned)(B < 1024 ? B : 1024)), dim3(256), 0, st, tp, B, V, E,
                     vertices, vbs, alpha, abs_, new_vertices, new_alpha);
  KAMD_RETURN_LAST_ERROR();
}

template <typename T>
int sl_backward(hipStream_t st, long long B, long long V, long long E, const T* grad_new_vertices, const T* grad_new_alpha,
                const T* vertices, long long vbs, const T* alpha, long long abs_, const SlTopo& tp, T* grad_vertices, T* grad_alpha) {
  if (sl_bad_value_extents(B, V, E) || vbs < 0 || abs_ < 0) return (int)hipErrorInvalidValue;
  if (B == 0 || V == 0) return 0;
  if (grad_new_vertices == nullptr || vertices == nullptr || grad_vertices == nullptr || (grad_alpha != nullptr && alpha == nullptr) ||
      sl_bad_topo(tp, V, E))
    return (int)hipErrorInvalidValue;
  const long long blocks_v = sl_blocks(V), blocks_e = sl_blocks(E);
  if (blocks_v == 0 || (E > 0 && blocks_e == 0)) return (int)hipErrorInvalidValue;
  const unsigned by = (unsigned)(B < 1024 ? B : 1024);
  hipLaunchKernelGGL((sl_backward_gather_kernel<T>), dim3((unsigned)blocks_v, by), dim3(256), 0, st, tp, B, V, E, grad_new_vertices,
                     grad_new_alpha, vertices, vbs, alpha, abs_, grad_vertices, grad_alpha);
  if (E > 0)
    hipLaunchKernelGGL((sl_backward_opp_kernel<T>), dim3((unsigned)blocks_e, by), dim3(256), 0, st, tp, B, V, E, grad_new_vertices,
                       grad_new_alpha, grad_vertices, grad_alpha);
  KAMD_RETURN_LAST_ERROR();
}

inline SlTopo sl_topo(const int64_t* edges, const int32_t* count, const int64_t* opp, const int64_t* tlist, const int64_t* runs,
                      const int32_t* valence) {
  SlTopo tp;
  tp.edges = edges, tp.count = count, tp.opp = opp, tp.tlist = tlist, tp.runs = runs, tp.valence = valence;
  return tp;
}

}  // namespace

extern "C" {

size_t kamd_subdivide_trianglemesh_workspace(int64_t F, int64_t V) { return sl_workspace_bytes(F, V); }
int kamd_subdivide_trianglemesh_edges(void* stream, int64_t F, int64_t V, const int64_t* faces, void* workspace,
                                      int64_t* host_num_edges) {
  return sl_edges((hipStream_t)stream, F, V, faces, workspace, host_num_edges);
}
int kamd_subdivide_trianglemesh_emit(void* stream, int64_t F, int64_t V, const int64_t* faces, void* workspace, int64_t num_edges,
                                     int64_t* edges, int64_t* new_faces, int32_t* count, int64_t* opp, int64_t* tlist, int64_t* runs,
                                     int32_t* valence) {
  return sl_emit((hipStream_t)stream, F, V, faces, workspace, num_edges, edges, new_faces, count, opp, tlist, runs, valence);
}

#define KAMD_SL_ENTRIES(SFX, CT)                                                                                                   \
  int kamd_trianglemesh_loop_forward_##SFX(void* stream, int64_t B, int64_t V, int64_t E, const CT* vertices,                      \
                                           int64_t vertices_batch_stride, const CT* alpha, int64_t alpha_batch_stride,            \
                                           const int64_t* edges, const int32_t* count, const int64_t* opp, const int64_t* tlist,   \
                                           const int64_t* runs, const int32_t* valence, CT* new_vertices, CT* new_alpha) {         \
    return sl_forward<CT>((hipStream_t)stream, B, V, E, vertices, vertices_batch_stride, alpha, alpha_batch_stride,                \
                          sl_topo(edges, count, opp, tlist, runs, valence), new_vertices, new_alpha);                              \
  }                                                                                                                                \
  int kamd_trianglemesh_loop_backward_##SFX(void* stream, int64_t B, int64_t V, int64_t E, const CT* grad_new_vertices,            \
                                            const CT* grad_new_alpha, const CT* vertices, int64_t vertices_batch_stride,          \
                                            const CT* alpha, int64_t alpha_batch_stride, const int64_t* edges,                    \
                                            const int32_t* count, const int64_t* opp, const int64_t* tlist, const int64_t* runs,   \
                                            const int32_t* valence, CT* grad_vertices, CT* grad_alpha) {                           \
    return sl_backward<CT>((hipStream_t)stream, B, V, E, grad_new_vertices, grad_new_alpha, vertices, vertices_batch_stride, alpha, \
                           alpha_batch_stride, sl_topo(edges, count, opp, tlist, runs, valence), grad_vertices, grad_alpha);       \
  }
KAMD_SL_ENTRIES(f32, float)
KAMD_SL_ENTRIES(f64, double)
#undef KAMD_SL_ENTRIES

}  // extern "C"
