// ops.mesh.subdivide_tetmesh: every tet split into eight through the midpoints of its six edges (the reference is
// torch.unique(dim=0, return_inverse=True) over the 6 T (min, max) edge rows and a chain of gathers, two cats and eight stacks,
// kaolin/ops/mesh/tetmesh.py).
//
//     edge slots of a tet (a, b, c, d)   ab ac ad bc bd cd; an edge is the pair (min, max) of its ends, a self-edge (v, v) included
//     E unique edges, numbered in ascending (min, max) order; edge e is the new vertex V + e
//     new row V + e                      (x[min] + x[max]) * 0.5: one rounded addition and an exact halving (-ffp-contract=off)
//     new_tets, eight blocks of T rows   (a ab ac ad) (b bc ab bd) (c ac bc cd) (d ad cd bd)
//                                        (ab ac ad bd) (ab ac bd bc) (cd ac bd ad) (cd ac bc bd)
//
// TOPOLOGY (once per call: it does not depend on the batch)
//   1. st_keys_kernel     THE pass over `tets` (two 16-byte loads per tet): the six keys min << 32 | max of tet t at keys[6 t ..],
//                         as three 16-byte stores.  Bound: 32 B read + 48 B written per tet.
//   2. sort               sort_scan.h: stable 8-bit LSD radix sort of the keys alone, over the digits below ceil(log2 V) of either
//                         half only (2 x ceil(bits / 8) passes; each reads the keys twice and scatters them once).  Most of the
//                         topology's traffic: 6 passes x 6 T x 24 B at V = 2.1 M.
//   3. heads / scan / unique   the first of every run of equal keys, compacted: the unique keys ARE the edge list.  The HOST reads
//                         E -- the one stream synchronisation of the call.
//   4. st_edges_kernel    unique keys -> edges (E, 2) int64, a 16-byte store per edge.
//      st_emit_kernel     per tet: re-reads the tet, ranks its six keys by binary search in the unique keys (ss_rank: ~log2 E
//                         dependent loads, the top levels from L2) and writes its row of each of the eight blocks as two 16-byte
//                         stores (256 B per tet; consecutive threads write consecutive rows of a block).  A permutation carried
//                         through the sort would replace the searches by 6 T x 8 B more traffic in each of the passes and a
//                         6 T scatter; the search reads a list that the sort has just left in L2 and keeps the sort keys-only.
// MIDPOINTS (per batch item; float and double)
//   forward   st_midpoints_forward_kernel: ONE launch writes both results, a thread per contiguous (row, channel) element of
//             new_vertices and then of new_features: rows [0, V) are copied, row V + e is the midpoint.  Bound: (V + E)(3 + D)
//             elements written, V (3 + D) + 2 E (3 + D) read (the gathers by `edges` hit rows a few edges apart: L2).
//   backward  grad x[b, v] = g[b, v] + 1/2 sum of g[b, V + e] over the unique edges holding v (a self-edge counts twice), in two
//             launches that touch disjoint terms:
//               st_midpoints_backward_min_kernel   `edges` is sorted by min, so the edges with min = v are one run, found by two
//                                                  binary searches: g[v] + the run's halves summed in edge order, a plain store
//                                                  (this also initialises the result: no zero fill)
//               st_midpoints_backward_max_kernel   the max side is scattered: one native fp32 / fp64 atomic add of g / 2 per
//                                                  (edge, channel) into the max end (~7 per element on a Kuhn grid).  Chosen over
//                                                  a transposed list, which would cost a second sort of E keys per topology.
// Every kernel is a plain bounded launch; none waits on another workgroup.
#include "common.h"
#include "sort_scan.h"
#include "tet_load.h"
#include "subdivide_tetmesh_host.h"
#include "../../include/kaolin_amd.h"

namespace {

__device__ __forceinline__ unsigned long long st_key(unsigned long long p, unsigned long long q) {
  return p < q ? (p << 32) | q : (q << 32) | p;
}
// the six keys of a tet in slot order ab ac ad bc bd cd
__device__ __forceinline__ void st_tet_keys(const MtTet& tet, unsigned long long* k) {
  k[0] = st_key(tet.id[0], tet.id[1]);
  k[1] = st_key(tet.id[0], tet.id[2]);
  k[2] = st_key(tet.id[0], tet.id[3]);
  k[3] = st_key(tet.id[1], tet.id[2]);
  k[4] = st_key(tet.id[1], tet.id[3]);
  k[5] = st_key(tet.id[2], tet.id[3]);
}

// ---- 1. keys --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void st_keys_kernel(const int64_t* __restrict__ tets, long long T,
                                                      unsigned long long* __restrict__ keys) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const MtTet tet = mt_load_tet(tets, t);  // ids in [0, V), V < 2^32: the shim has checked the range
  unsigned long long k[6];
  st_tet_keys(tet, k);
  ulonglong2* out = (ulonglong2*)(keys + 6 * t);  // 48 t bytes from a 16-byte aligned base
  out[0] = make_ulonglong2(k[0], k[1]);
  out[1] = make_ulonglong2(k[2], k[3]);
  out[2] = make_ulonglong2(k[4], k[5]);
}

// ---- 4. results -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void st_edges_kernel(long long E, const unsigned long long* __restrict__ uniq,
                                                       int64_t* __restrict__ edges) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const unsigned long long key = uniq[e];
  ((ulonglong2*)edges)[e] = make_ulonglong2(key >> 32, key & 0xffffffffull);
}

__global__ __launch_bounds__(256) void st_emit_kernel(const int64_t* __restrict__ tets, long long T, unsigned long long V,
                                                      const unsigned long long* __restrict__ uniq, long long E,
                                                      int64_t* __restrict__ new_tets) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const MtTet tet = mt_load_tet(tets, t);
  unsigned long long k[6], r[6];
  st_tet_keys(tet, k);
#pragma unroll
  for (int s = 0; s < 6; ++s) r[s] = V + (unsigned long long)ss_rank(uniq, E, k[s]);
  const unsigned long long a = tet.id[0], b = tet.id[1], c = tet.id[2], d = tet.id[3];
  const unsigned long long ab = r[0], ac = r[1], ad = r[2], bc = r[3], bd = r[4], cd = r[5];
  ulonglong2* out = (ulonglong2*)new_tets;  // row (block * T + t): 32 bytes, two 16-byte words
#define ST_ROW(BLOCK, P, Q, R, S)                             \
  out[2 * ((long long)(BLOCK) * T + t)] = make_ulonglong2(P, Q); \
  out[2 * ((long long)(BLOCK) * T + t) + 1] = make_ulonglong2(R, S);
  ST_ROW(0, a, ab, ac, ad)
  ST_ROW(1, b, bc, ab, bd)
  ST_ROW(2, c, ac, bc, cd)
  ST_ROW(3, d, ad, cd, bd)
  ST_ROW(4, ab, ac, ad, bd)
  ST_ROW(5, ab, ac, bd, bc)
  ST_ROW(6, cd, ac, bd, ad)
  ST_ROW(7, cd, ac, bc, bd)
#undef ST_ROW
}

// ---- midpoints --------------------------------------------------------------------------------------------------------------
// The two tensors of a call (positions, 3 channels; features, D channels; either may be absent) share one flat index: element j
// of a batch item is (row, channel) of the first tensor for j < rows * c0, of the second above.
template <typename T>
struct StPair {
  const T* in[2];   // forward: the inputs; backward: the incoming gradients (rows V + E)
  T* out[2];        // forward: the results (rows V + E); backward: the gradients of the inputs (rows V)
  long long in_batch_stride[2];
  int channels[2];  // 0: the tensor is absent
};

template <typename T>
__global__ __launch_bounds__(256) void st_midpoints_forward_kernel(StPair<T> p, long long B, long long V, long long E,
                                                                   const int64_t* __restrict__ edges) {
  const long long R = V + E, n0 = R * p.channels[0], n = n0 + R * p.channels[1];
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int w = j < n0 ? 0 : 1, C = p.channels[w];
  const long long k = w ? j - n0 : j, row = k / C, ch = k - row * C;
  const bool mid = row >= V;
  long long ia = k, ib = k;  // a copied row reads element k; a midpoint reads both ends of its edge (ids in [0, V): the shim's check)
  if (mid) {
    ia = edges[2 * (row - V)] * C + ch;
    ib = edges[2 * (row - V) + 1] * C + ch;
  }
  for (long long b = blockIdx.y; b < B; b += gridDim.y) {
    const T* x = p.in[w] + b * p.in_batch_stride[w];
    const T v = mid ? (x[ia] + x[ib]) * (T)0.5 : x[ia];
    p.out[w][b * R * C + k] = v;
  }
}

// first e in [0, E) with edges[e].min >= v
__device__ __forceinline__ long long st_first_min(const int64_t* __restrict__ edges, long long E, long long v) {
  long long lo = 0, hi = E;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (edges[2 * mid] < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

template <typename T>
__global__ __launch_bounds__(256) void st_midpoints_backward_min_kernel(StPair<T> p, long long B, long long V, long long E,
                                                                        const int64_t* __restrict__ edges) {
  const long long n0 = V * p.channels[0], n = n0 + V * p.channels[1];
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int w = j < n0 ? 0 : 1, C = p.channels[w];
  const long long k = w ? j - n0 : j, v = k / C, ch = k - v * C;
  const long long first = st_first_min(edges, E, v), last = st_first_min(edges, E, v + 1);
  for (long long b = blockIdx.y; b < B; b += gridDim.y) {
    const T* g = p.in[w] + b * p.in_batch_stride[w];
    T acc = g[k];
    for (long long e = first; e < last; ++e) acc += g[(V + e) * C + ch] * (T)0.5;
    p.out[w][b * V * C + k] = acc;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void st_midpoints_backward_max_kernel(StPair<T> p, long long B, long long V, long long E,
                                                                        const int64_t* __restrict__ edges) {
  const long long n0 = E * p.channels[0], n = n0 + E * p.channels[1];
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int w = j < n0 ? 0 : 1, C = p.channels[w];
  const long long k = w ? j - n0 : j, e = k / C, ch = k - e * C;
  const long long hi = edges[2 * e + 1];  // in [0, V): the shim's check
  for (long long b = blockIdx.y; b < B; b += gridDim.y) {
    const T* g = p.in[w] + b * p.in_batch_stride[w];
    kamd_atomic_add(&p.out[w][b * V * C + hi * C + ch], g[(V + e) * C + ch] * (T)0.5);
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
int st_edges(hipStream_t st, long long T, long long V, const int64_t* tets, void* workspace, int64_t* host_num_edges) {
  if (st_bad_extents(T, V) || host_num_edges == nullptr) return (int)hipErrorInvalidValue;
  *host_num_edges = 0;
  if (T == 0 || V == 0) return 0;
  if (tets == nullptr || workspace == nullptr || ((uintptr_t)tets & 15) != 0 || ((uintptr_t)workspace & 15) != 0)
    return (int)hipErrorInvalidValue;
  const StLayout l = st_layout(T);
  char* ws = (char*)workspace;
  unsigned long long* keys = (unsigned long long*)(ws + l.keys_a);
  unsigned long long* uniq = (unsigned long long*)(ws + l.keys_b);
  long long* sums = (long long*)(ws + l.sums);

  hipLaunchKernelGGL(st_keys_kernel, dim3(ss_grid(T, 256)), dim3(256), 0, st, tets, T, keys);
  KAMD_CHECK(hipGetLastError());
  KAMD_CHECK(ss_sort(st, l.n, ss_passes_halves(st_id_bits(V)), keys, uniq, keys,  // in place, through keys_b
                     ss_sort_ws((int*)(ws + l.hist), (long long*)(ws + l.hoffs), sums)));
  return ss_unique(st, l.n, keys, (int*)(ws + l.flags), (long long*)(ws + l.pos), sums, uniq, host_num_edges);
}

int st_emit(hipStream_t st, long long T, long long V, const int64_t* tets, const void* workspace, long long E, int64_t* edges,
            int64_t* new_tets) {
  if (st_bad_extents(T, V) || E < 0 || E > 6 * T) return (int)hipErrorInvalidValue;
  if (T == 0 || V == 0 || E == 0) return 0;
  if (tets == nullptr || workspace == nullptr || edges == nullptr || new_tets == nullptr || ((uintptr_t)tets & 15) != 0 ||
      ((uintptr_t)edges & 15) != 0 || ((uintptr_t)new_tets & 15) != 0)
    return (int)hipErrorInvalidValue;
  const unsigned long long* uniq = (const unsigned long long*)((const char*)workspace + st_layout(T).keys_b);
  hipLaunchKernelGGL(st_edges_kernel, dim3(ss_grid(E, 256)), dim3(256), 0, st, E, uniq, edges);
  hipLaunchKernelGGL(st_emit_kernel, dim3(ss_grid(T, 256)), dim3(256), 0, st, tets, T, (unsigned long long)V, uniq, E, new_tets);
  KAMD_RETURN_LAST_ERROR();
}

// blocks of 256 over `rows` rows of both tensors, or 0 when that many do not fit a launch
inline long long st_blocks(long long rows, long long channels) {
  if (rows > (1ll << 40) / (channels > 0 ? channels : 1)) return 0;
  const long long blocks = ss_cdiv(rows * channels, 256);
  return blocks < (1ll << 31) ? blocks : 0;
}
inline bool st_bad_midpoint_extents(long long B, long long V, long long E, long long D) {
  return B < 0 || V < 0 || E < 0 || D < 0 || V >= (1ll << 32) || D >= (1ll << 20) || E > (1ll << 38);
}

template <typename T>
int st_midpoints_forward(hipStream_t st, long long B, long long V, long long E, long long D, const T* vertices, long long vbs,
                         const T* features, long long fbs, const int64_t* edges, T* new_vertices, T* new_features) {
  if (st_bad_midpoint_extents(B, V, E, D) || vbs < 0 || fbs < 0) return (int)hipErrorInvalidValue;
  StPair<T> p;
  p.in[0] = vertices, p.out[0] = new_vertices, p.in_batch_stride[0] = vbs, p.channels[0] = vertices != nullptr ? 3 : 0;
  p.in[1] = features, p.out[1] = new_features, p.in_batch_stride[1] = fbs, p.channels[1] = features != nullptr ? (int)D : 0;
  const long long channels = p.channels[0] + p.channels[1];
  if (B == 0 || V + E == 0 || channels == 0) return 0;
  if ((p.channels[0] && new_vertices == nullptr) || (p.channels[1] && new_features == nullptr) || (E > 0 && edges == nullptr))
    return (int)hipErrorInvalidValue;
  const long long blocks = st_blocks(V + E, channels);
  if (blocks == 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((st_midpoints_forward_kernel<T>), dim3((unsigned)blocks, (unsigned)(B < 1024 ? B : 1024)), dim3(256), 0, st, p,
                     B, V, E, edges);
  KAMD_RETURN_LAST_ERROR();
}

template <typename T>
int st_midpoints_backward(hipStream_t st, long long B, long long V, long long E, long long D, const T* grad_new_vertices,
                          const T* grad_new_features, const int64_t* edges, T* grad_vertices, T* grad_features) {
  if (st_bad_midpoint_extents(B, V, E, D)) return (int)hipErrorInvalidValue;
  StPair<T> p;
  p.in[0] = grad_new_vertices, p.out[0] = grad_vertices, p.in_batch_stride[0] = (V + E) * 3;
  p.channels[0] = grad_new_vertices != nullptr ? 3 : 0;
  p.in[1] = grad_new_features, p.out[1] = grad_features, p.in_batch_stride[1] = (V + E) * D;
  p.channels[1] = grad_new_features != nullptr ? (int)D : 0;
  const long long channels = p.channels[0] + p.channels[1];
  if (B == 0 || V == 0 || channels == 0) return 0;
  if ((p.channels[0] && grad_vertices == nullptr) || (p.channels[1] && grad_features == nullptr) || (E > 0 && edges == nullptr))
    return (int)hipErrorInvalidValue;
  const long long blocks_v = st_blocks(V, channels), blocks_e = st_blocks(E, channels);
  if (blocks_v == 0 || (E > 0 && blocks_e == 0)) return (int)hipErrorInvalidValue;
  const dim3 by((unsigned)(B < 1024 ? B : 1024));
  hipLaunchKernelGGL((st_midpoints_backward_min_kernel<T>), dim3((unsigned)blocks_v, by.x), dim3(256), 0, st, p, B, V, E, edges);
  if (E > 0)
    hipLaunchKernelGGL((st_midpoints_backward_max_kernel<T>), dim3((unsigned)blocks_e, by.x), dim3(256), 0, st, p, B, V, E, edges);
  KAMD_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {

size_t kamd_subdivide_tetmesh_workspace(int64_t T, int64_t V) { return st_workspace_bytes(T, V); }
int kamd_subdivide_tetmesh_edges(void* stream, int64_t T, int64_t V, const int64_t* tets, void* workspace,
                                 int64_t* host_num_edges) {
  return st_edges((hipStream_t)stream, T, V, tets, workspace, host_num_edges);
}
int kamd_subdivide_tetmesh_emit(void* stream, int64_t T, int64_t V, const int64_t* tets, const void* workspace, int64_t num_edges,
                                int64_t* edges, int64_t* new_tets) {
  return st_emit((hipStream_t)stream, T, V, tets, workspace, num_edges, edges, new_tets);
}

#define KAMD_ST_ENTRIES(SFX, CT)                                                                                                  \
  int kamd_tetmesh_midpoints_forward_##SFX(void* stream, int64_t B, int64_t V, int64_t E, int64_t D, const CT* vertices,            \
                                           int64_t vertices_batch_stride, const CT* features, int64_t features_batch_stride,      \
                                           const int64_t* edges, CT* new_vertices, CT* new_features) {                            \
    return st_midpoints_forward<CT>((hipStream_t)stream, B, V, E, D, vertices, vertices_batch_stride, features,                   \
                                    features_batch_stride, edges, new_vertices, new_features);                                    \
  }                                                                                                                               \
  int kamd_tetmesh_midpoints_backward_##SFX(void* stream, int64_t B, int64_t V, int64_t E, int64_t D, const CT* grad_new_vertices,  \
                                            const CT* grad_new_features, const int64_t* edges, CT* grad_vertices,                 \
                                            CT* grad_features) {                                                                  \
    return st_midpoints_backward<CT>((hipStream_t)stream, B, V, E, D, grad_new_vertices, grad_new_features, edges, grad_vertices, \
                                     grad_features);                                                                              \
  }
KAMD_ST_ENTRIES(f32, float)
KAMD_ST_ENTRIES(f64, double)
#undef KAMD_ST_ENTRIES

}  // extern "C"
