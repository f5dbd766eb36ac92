// ops.conversions.marching_tetrahedra: the zero level set of a signed-distance field on a tetrahedral grid as a triangle mesh
// (one item of the batch per call; the reference is a chain of ~25 torch kernels, kaolin/ops/conversions/tetmesh.py).
//
//     occupied(v)  = sdf[v] > 0                       (0, -0.0, negative and NaN are not)
//     case(t)      = sum_k occupied(tets[t][k]) << k  (4 bits); a tet with 1..3 occupied corners is VALID and emits one
//                    triangle (1 or 3 corners) or two (2 corners)
//     vertices     = the unique crossing edges {a < b} of the valid tets (exactly one end occupied), ascending by (a, b):
//                    (p_a * (-s_b) + p_b * s_a) / (s_a + (-s_b)), four separately rounded operations (-ffp-contract=off)
//     faces        = the triangles of the one-triangle tets in tet order, then those of the two-triangle tets in tet order
//                    (two consecutive rows each), corners picked by mt_tri[case] from the tet's six edge slots
//
//   1. mt_occupancy_kernel   sdf > 0 packed into V bits (__ballot, one 64-bit word per wavefront): every later corner lookup
//                            is a bit test in a table that stays in L2 (262 KB for 2.1 M vertices).
//   2. mt_classify_kernel    THE pass over `tets` (32 bytes per tet as two 16-byte loads): the case of every tet as one byte,
//                            and per chunk of 1 024 tets the number of one- and two-triangle tets.  A tet with a corner outside
//                            [0, V) is case 0: nothing downstream ever indexes with an id this kernel has not compared with V.
//   3. ss_scan               exclusive scan of the chunk counts (both kinds in one array); the HOST reads the two totals.
//   4. mt_compact_kernel     re-reads the case bytes (1 byte per tet), ranks the valid tets of a chunk in tet order (ballots
//                            inside a wavefront, LDS across wavefronts) and writes (tet << 4 | case) into the one- or the
//                            two-triangle list, plus one key (a << 32 | b) per crossing edge of the tet (3 or 4).
//   5. sort                  stable 8-bit LSD radix sort of the keys alone (histogram per block of 2 048, one scan over the
//                            (digit, block) counts, ranked scatter), over the digits below ceil(log2 V) of either half only.
//   6. ss_unique             first of every run of equal keys, scan, compaction: the unique keys ARE the vertex list; the HOST
//                            reads their number.  (5 and 6: sort_scan.h)
//   7. mt_verts_kernel       per unique edge: the vertex and the (a, b) pair autograd keeps.
//      mt_faces_kernel       per valid tet: its rows of `faces` (and `tet_idx`); the rank of each of its crossing edges by
//                            binary search in the unique keys.
//   backward                 per unique edge, d = s_a - s_b, v as above:
//                              grad p_a += (-s_b / d) g     grad p_b += (s_a / d) g
//                              grad s_a += g . (p_b - v) / d     grad s_b += g . (v - p_a) / d
//                            with native fp32 / fp64 atomic adds into zeroed buffers (a vertex has ~10 incident crossing edges).
// Result sizes depend on the data: the two host reads synchronise the stream, so the operator cannot be captured in a graph
// (neither can the reference: torch.unique and boolean indexing synchronise).
#include "common.h"
#include "sort_scan.h"
#include "tet_load.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_ITEMS = 4;                        // tets per thread of the classify and compact kernels
constexpr int MT_CHUNK = MT_THREADS * MT_ITEMS;    // tets per workgroup: the unit of the count scan

// The six edge slots of a tet join its corners (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).
// case -> the edge slots of its triangle(s), corner by corner.  Derived from the reference's answers for the 16 sign patterns
// of one tet (tests/golden/marching_tetrahedra.npz `cases16`; tests/test_marching_tetrahedra_cpu.py rebuilds it from there).
__constant__ unsigned char mt_tri[16][6] = {
    {0, 0, 0, 0, 0, 0}, {1, 0, 2, 0, 0, 0}, {4, 0, 3, 0, 0, 0}, {1, 4, 2, 1, 3, 4}, {3, 1, 5, 0, 0, 0}, {2, 3, 0, 2, 5, 3},
    {1, 4, 0, 1, 5, 4}, {4, 2, 5, 0, 0, 0}, {4, 5, 2, 0, 0, 0}, {4, 1, 0, 4, 5, 1}, {3, 2, 0, 3, 5, 2}, {1, 3, 5, 0, 0, 0},
    {4, 1, 2, 4, 3, 1}, {3, 0, 4, 0, 0, 0}, {2, 0, 1, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};


// ---- the (T, V) workspace: what classify leaves for the later stages -----------------------------------------------------
struct MtLayout {
  long long nchunk, words;
  size_t bitmap, cases, counts, offs, sums, bytes;
};
MtLayout mt_layout(long long T, long long V) {
  MtLayout l;
  l.nchunk = ss_cdiv(T, MT_CHUNK);
  l.words = ss_cdiv(V, 64);
  size_t o = 0;
  l.bitmap = o, o += kamd_align16((size_t)l.words * 8);
  l.cases = o, o += kamd_align16((size_t)T);
  l.counts = o, o += kamd_align16((size_t)l.nchunk * 2 * 4);
  l.offs = o, o += kamd_align16(((size_t)l.nchunk * 2 + 1) * 8);
  l.sums = o, o += kamd_align16(ss_scan_sums_entries(l.nchunk * 2) * 8);
  l.bytes = o;
  return l;
}
// ---- the edge workspace, sized by the two counts the host has read -------------------------------------------------------
struct MtEdgeLayout {
  long long n;  // crossing-edge instances
  size_t entries, keys_a, keys_b, uniq, flags, pos, hist, hoffs, sums, bytes;
};
MtEdgeLayout mt_edge_layout(long long n_one, long long n_two) {
  MtEdgeLayout l;
  l.n = 3 * n_one + 4 * n_two;
  size_t o = 0;
  l.entries = o, o += kamd_align16((size_t)(n_one + n_two) * 8);
  l.keys_a = o, o += kamd_align16((size_t)l.n * 8);
  l.keys_b = o, o += kamd_align16((size_t)l.n * 8);
  l.uniq = o, o += kamd_align16((size_t)l.n * 8);
  l.flags = o, o += kamd_align16((size_t)l.n * 4);
  l.pos = o, o += kamd_align16(((size_t)l.n + 1) * 8);
  l.hist = o, o += kamd_align16(ss_sort_hist_entries(l.n) * 4);
  l.hoffs = o, o += kamd_align16(ss_sort_offs_entries(l.n) * 8);
  l.sums = o, o += kamd_align16(ss_sort_unique_sums_entries(l.n) * 8);
  l.bytes = o;
  return l;
}

// ---- 1. occupancy bits -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(MT_THREADS) void mt_occupancy_kernel(const T* __restrict__ sdf, long long V, long long words,
                                                                  unsigned long long* __restrict__ bitmap) {
  const int lane = threadIdx.x & 63;
  const long long nwaves = (long long)gridDim.x * (MT_THREADS / 64);
  for (long long w = (long long)blockIdx.x * (MT_THREADS / 64) + (threadIdx.x >> 6); w < words; w += nwaves) {  // (wave-uniform)
    const long long v = w * 64 + lane;
    const bool occ = v < V && sdf[v] > (T)0;  // NaN compares false
    const unsigned long long m = __ballot(occ);
    if (lane == 0) bitmap[w] = m;
  }
}

__device__ __forceinline__ bool mt_one_triangle(unsigned c) { return (__popc(c) & 1) != 0; }  // 1 or 3 corners occupied
__device__ __forceinline__ bool mt_two_triangles(unsigned c) { return __popc(c) == 2; }

// ---- 2. classify --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MT_THREADS) void mt_classify_kernel(const int64_t* __restrict__ tets, long long T, unsigned long long V,
                                                                 const unsigned long long* __restrict__ bitmap,
                                                                 unsigned char* __restrict__ cases, int* __restrict__ counts,
                                                                 long long nchunk) {
  __shared__ int s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * MT_CHUNK;
  MtTet tet[MT_ITEMS];
#pragma unroll
  for (int r = 0; r < MT_ITEMS; ++r) {  // all the loads of the thread in flight
    const long long t = base + r * MT_THREADS + threadIdx.x;
    if (t < T) tet[r] = mt_load_tet(tets, t);
  }
  int n1 = 0, n2 = 0;
#pragma unroll
  for (int r = 0; r < MT_ITEMS; ++r) {
    const long long t = base + r * MT_THREADS + threadIdx.x;
    unsigned c = 0;
    if (t < T) {
      // unsigned: a negative id is a huge one.  Out of range -> case 0, the tet is dropped
      const bool in_range = tet[r].id[0] < V && tet[r].id[1] < V && tet[r].id[2] < V && tet[r].id[3] < V;
      if (in_range) {
#pragma unroll
        for (int k = 0; k < 4; ++k) c |= (unsigned)((bitmap[tet[r].id[k] >> 6] >> (tet[r].id[k] & 63)) & 1ull) << k;
      }
      cases[t] = (unsigned char)c;
    }
    n1 += __popcll(__ballot(mt_one_triangle(c)));  // (c = 0 beyond T)
    n2 += __popcll(__ballot(mt_two_triangles(c)));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&s_cnt[0], n1);
    atomicAdd(&s_cnt[1], n2);
  }
  __syncthreads();
  if (threadIdx.x < 2) counts[threadIdx.x * nchunk + blockIdx.x] = s_cnt[threadIdx.x];
}

// ---- 4. compaction of the valid tets, in tet order, and their edge keys ------------------------------------------------------
// offs: the scanned chunk counts, [0, nchunk) the one-triangle tets before each chunk, [nchunk, 2 nchunk) the same for the
// two-triangle tets continuing the same running sum (offs[nchunk] = n_one).  Instance slots: 3 per one-triangle tet, then 4 per
// two-triangle tet; where a key lands does not matter (they are sorted next), only that every slot is written exactly once.
__global__ __launch_bounds__(MT_THREADS) void mt_compact_kernel(const int64_t* __restrict__ tets, long long T,
                                                                const unsigned char* __restrict__ cases,
                                                                const long long* __restrict__ offs, long long nchunk,
                                                                long long n_one, unsigned long long* __restrict__ entries,
                                                                unsigned long long* __restrict__ keys) {
  __shared__ int s_w[MT_ITEMS][2][MT_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  long long run1 = offs[blockIdx.x], run2 = offs[nchunk + blockIdx.x] - n_one;
  const long long base = (long long)blockIdx.x * MT_CHUNK;
#pragma unroll
  for (int r = 0; r < MT_ITEMS; ++r) {
    const long long t = base + r * MT_THREADS + threadIdx.x;
    const unsigned c = t < T ? cases[t] : 0u;
    const bool is1 = mt_one_triangle(c), is2 = mt_two_triangles(c);
    const unsigned long long b1 = __ballot(is1), b2 = __ballot(is2);
    if (lane == 0) {
      s_w[r][0][wave] = __popcll(b1);
      s_w[r][1][wave] = __popcll(b2);
    }
    __syncthreads();  // (a plane of s_w per round: one barrier a round)
    long long before1 = 0, before2 = 0, all1 = 0, all2 = 0;
#pragma unroll
    for (int w = 0; w < MT_THREADS / 64; ++w) {
      if (w < wave) before1 += s_w[r][0][w], before2 += s_w[r][1][w];
      all1 += s_w[r][0][w], all2 += s_w[r][1][w];
    }
    if (is1 || is2) {  // c != 0: classify has compared the four ids with V
      long long slot;
      if (is1) {
        const long long p = run1 + before1 + __popcll(b1 & below);
        entries[p] = ((unsigned long long)t << 4) | c;
        slot = 3 * p;
      } else {
        const long long p = run2 + before2 + __popcll(b2 & below);
        entries[n_one + p] = ((unsigned long long)t << 4) | c;
        slot = 3 * n_one + 4 * p;
      }
      const MtTet tet = mt_load_tet(tets, t);
#pragma unroll
      for (int s = 0; s < 6; ++s) {
        const int i = s < 3 ? 0 : (s < 5 ? 1 : 2), j = s < 3 ? s + 1 : (s < 5 ? s - 1 : 3);  // the slot's two corners
        if (((c >> i) ^ (c >> j)) & 1u) {
          const unsigned long long a = tet.id[i] < tet.id[j] ? tet.id[i] : tet.id[j];
          const unsigned long long b = tet.id[i] < tet.id[j] ? tet.id[j] : tet.id[i];
          keys[slot++] = (a << 32) | b;
        }
      }
    }
    run1 += all1;
    run2 += all2;
  }
}

// ---- 7. results -------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void mt_verts_kernel(long long nu, const unsigned long long* __restrict__ uniq,
                                                       const T* __restrict__ vertices, const T* __restrict__ sdf,
                                                       T* __restrict__ verts, int64_t* __restrict__ edges) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nu) return;
  const unsigned long long key = uniq[i];
  const long long a = (long long)(key >> 32), b = (long long)(key & 0xffffffffull);  // both < V: built from classified tets
  const T sa = sdf[a], nsb = -sdf[b];
  const T den = sa + nsb;
#pragma unroll
  for (int c = 0; c < 3; ++c) verts[3 * i + c] = (vertices[3 * a + c] * nsb + vertices[3 * b + c] * sa) / den;
  edges[2 * i] = a;
  edges[2 * i + 1] = b;
}

__global__ __launch_bounds__(256) void mt_faces_kernel(long long n_one, long long n_two, const unsigned long long* __restrict__ entries,
                                                       const int64_t* __restrict__ tets, const unsigned long long* __restrict__ uniq,
                                                       long long nu, int64_t* __restrict__ faces, int64_t* __restrict__ tet_idx) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_one + n_two) return;
  const unsigned long long ent = entries[e];
  const long long t = (long long)(ent >> 4);
  const unsigned c = (unsigned)(ent & 15u);
  const MtTet tet = mt_load_tet(tets, t);
  long long rk[6];
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const int i = s < 3 ? 0 : (s < 5 ? 1 : 2), j = s < 3 ? s + 1 : (s < 5 ? s - 1 : 3);
    rk[s] = 0;
    if (((c >> i) ^ (c >> j)) & 1u) {
      const unsigned long long a = tet.id[i] < tet.id[j] ? tet.id[i] : tet.id[j];
      const unsigned long long b = tet.id[i] < tet.id[j] ? tet.id[j] : tet.id[i];
      rk[s] = ss_rank(uniq, nu, (a << 32) | b);
    }
  }
  const bool two = e >= n_one;
  const long long row = two ? n_one + 2 * (e - n_one) : e;
  const int corners = two ? 6 : 3;
  for (int q = 0; q < corners; ++q) {
    const int s = mt_tri[c][q];
    long long r = rk[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) r = s == k ? rk[k] : r;
    faces[3 * row + q] = r;
  }
  if (tet_idx != nullptr) {
    tet_idx[row] = t;
    if (two) tet_idx[row + 1] = t;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void mt_backward_kernel(long long nu, unsigned long long V, const int64_t* __restrict__ edges,
                                                          const T* __restrict__ vertices, const T* __restrict__ sdf,
                                                          const T* __restrict__ grad_verts, T* __restrict__ grad_vertices,
                                                          T* __restrict__ grad_sdf) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nu) return;
  const unsigned long long a = (unsigned long long)edges[2 * i], b = (unsigned long long)edges[2 * i + 1];
  if (a >= V || b >= V) return;  // (the forward's own pairs never are)
  const T sa = sdf[a], sb = sdf[b];
  const T d = sa - sb;
  const T wa = -sb / d, wb = sa / d;
  T dot_b = (T)0, dot_a = (T)0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const T g = grad_verts[3 * i + c], pa = vertices[3 * a + c], pb = vertices[3 * b + c];
    const T v = (pa * -sb + pb * sa) / d;
    kamd_atomic_add(&grad_vertices[3 * a + c], wa * g);
    kamd_atomic_add(&grad_vertices[3 * b + c], wb * g);
    dot_b += g * (pb - v);
    dot_a += g * (v - pa);
  }
  kamd_atomic_add(&grad_sdf[a], dot_b / d);
  kamd_atomic_add(&grad_sdf[b], dot_a / d);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
bool mt_bad_extents(long long T, long long V) { return T < 0 || V < 0 || V >= (1ll << 32) || T >= (1ll << 59); }

template <typename T>
int mt_classify(hipStream_t st, long long nt, long long V, const int64_t* tets, const T* sdf, void* workspace,
                int64_t* host_counts) {
  if (mt_bad_extents(nt, V) || host_counts == nullptr) return (int)hipErrorInvalidValue;
  host_counts[0] = host_counts[1] = 0;
  if (nt == 0 || V == 0) return 0;
  if (tets == nullptr || sdf == nullptr || workspace == nullptr || ((uintptr_t)tets & 15) != 0 || ((uintptr_t)workspace & 15) != 0)
    return (int)hipErrorInvalidValue;
  const MtLayout l = mt_layout(nt, V);
  char* ws = (char*)workspace;
  unsigned long long* bitmap = (unsigned long long*)(ws + l.bitmap);
  int* counts = (int*)(ws + l.counts);
  long long* offs = (long long*)(ws + l.offs);
  long long blocks = ss_cdiv(l.words, MT_THREADS / 64);
  if (blocks > (long long)KAMD_NUM_CU * 8) blocks = (long long)KAMD_NUM_CU * 8;
  hipLaunchKernelGGL((mt_occupancy_kernel<T>), dim3((unsigned)blocks), dim3(MT_THREADS), 0, st, sdf, V, l.words, bitmap);
  hipLaunchKernelGGL(mt_classify_kernel, dim3((unsigned)l.nchunk), dim3(MT_THREADS), 0, st, tets, nt, (unsigned long long)V,
                     (const unsigned long long*)bitmap, (unsigned char*)(ws + l.cases), counts, l.nchunk);
  KAMD_CHECK(hipGetLastError());
  KAMD_CHECK(ss_scan(st, 2 * l.nchunk, (const long long*)nullptr, counts, offs, (long long*)(ws + l.sums)));
  long long h[2] = {0, 0};
  KAMD_CHECK(hipMemcpyAsync(&h[0], offs + l.nchunk, 8, hipMemcpyDeviceToHost, st));
  KAMD_CHECK(hipMemcpyAsync(&h[1], offs + 2 * l.nchunk, 8, hipMemcpyDeviceToHost, st));
  KAMD_CHECK(hipStreamSynchronize(st));
  host_counts[0] = h[0];
  host_counts[1] = h[1] - h[0];
  return 0;
}

// the bits of a vertex id: the digits of either key half above them are zero in every key
int mt_id_bits(long long V) {
  int nb = 1;
  while (nb < 32 && (1ll << nb) < V) ++nb;
  return nb;
}

int mt_edges(hipStream_t st, long long nt, long long V, const int64_t* tets, const void* workspace, long long n_one, long long n_two,
             void* edges_workspace, int64_t* host_num_unique) {
  if (mt_bad_extents(nt, V) || n_one < 0 || n_two < 0 || n_one + n_two > nt || host_num_unique == nullptr)
    return (int)hipErrorInvalidValue;
  *host_num_unique = 0;
  if (n_one + n_two == 0) return 0;
  if (tets == nullptr || workspace == nullptr || edges_workspace == nullptr || ((uintptr_t)tets & 15) != 0 ||
      ((uintptr_t)edges_workspace & 15) != 0)
    return (int)hipErrorInvalidValue;
  const MtLayout l = mt_layout(nt, V);
  const MtEdgeLayout el = mt_edge_layout(n_one, n_two);
  const char* ws = (const char*)workspace;
  char* ews = (char*)edges_workspace;
  unsigned long long* keys = (unsigned long long*)(ews + el.keys_a);
  unsigned long long* other = (unsigned long long*)(ews + el.keys_b);
  long long* sums = (long long*)(ews + el.sums);

  hipLaunchKernelGGL(mt_compact_kernel, dim3((unsigned)l.nchunk), dim3(MT_THREADS), 0, st, tets, nt,
                     (const unsigned char*)(ws + l.cases), (const long long*)(ws + l.offs), l.nchunk, n_one,
                     (unsigned long long*)(ews + el.entries), keys);
  KAMD_CHECK(hipGetLastError());
  KAMD_CHECK(ss_sort(st, el.n, ss_passes_halves(mt_id_bits(V)), keys, other, keys,  // in place, through `other`
                     ss_sort_ws((int*)(ews + el.hist), (long long*)(ews + el.hoffs), sums)));
  return ss_unique(st, el.n, keys, (int*)(ews + el.flags), (long long*)(ews + el.pos), sums,
                   (unsigned long long*)(ews + el.uniq), host_num_unique);
}

template <typename T>
int mt_emit(hipStream_t st, long long V, const int64_t* tets, const T* vertices, const T* sdf, const void* edges_workspace,
            long long n_one, long long n_two, long long nu, T* verts, int64_t* edges, int64_t* faces, int64_t* tet_idx) {
  if (V < 0 || V >= (1ll << 32) || n_one < 0 || n_two < 0 || nu < 0 || nu > 3 * n_one + 4 * n_two) return (int)hipErrorInvalidValue;
  if (n_one + n_two == 0 || nu == 0) return 0;
  if (tets == nullptr || vertices == nullptr || sdf == nullptr || edges_workspace == nullptr || verts == nullptr ||
      edges == nullptr || faces == nullptr || ((uintptr_t)tets & 15) != 0)
    return (int)hipErrorInvalidValue;
  const MtEdgeLayout el = mt_edge_layout(n_one, n_two);
  const char* ews = (const char*)edges_workspace;
  const unsigned long long* uniq = (const unsigned long long*)(ews + el.uniq);
  hipLaunchKernelGGL((mt_verts_kernel<T>), dim3(ss_grid(nu, 256)), dim3(256), 0, st, nu, uniq, vertices, sdf, verts, edges);
  hipLaunchKernelGGL(mt_faces_kernel, dim3(ss_grid(n_one + n_two, 256)), dim3(256), 0, st, n_one, n_two,
                     (const unsigned long long*)(ews + el.entries), tets, uniq, nu, faces, tet_idx);
  KAMD_RETURN_LAST_ERROR();
}

template <typename T>
int mt_backward(hipStream_t st, long long nu, long long V, const int64_t* edges, const T* vertices, const T* sdf,
                const T* grad_verts, T* grad_vertices, T* grad_sdf) {
  if (nu < 0 || V < 0 || V >= (1ll << 32)) return (int)hipErrorInvalidValue;
  if (nu == 0 || V == 0) return 0;
  if (edges == nullptr || vertices == nullptr || sdf == nullptr || grad_verts == nullptr || grad_vertices == nullptr ||
      grad_sdf == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((mt_backward_kernel<T>), dim3(ss_grid(nu, 256)), dim3(256), 0, st, nu, (unsigned long long)V, edges, vertices,
                     sdf, grad_verts, grad_vertices, grad_sdf);
  KAMD_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {

size_t kamd_marching_tetrahedra_workspace(int64_t T, int64_t V) {
  if (T <= 0 || V <= 0 || mt_bad_extents(T, V)) return 0;
  return mt_layout(T, V).bytes;
}
size_t kamd_marching_tetrahedra_edges_workspace(int64_t n_one, int64_t n_two) {
  if (n_one < 0 || n_two < 0 || n_one + n_two == 0) return 0;
  return mt_edge_layout(n_one, n_two).bytes;
}
int kamd_marching_tetrahedra_edges(void* stream, int64_t T, int64_t V, const int64_t* tets, const void* workspace, int64_t n_one,
                                   int64_t n_two, void* edges_workspace, int64_t* host_num_unique) {
  return mt_edges((hipStream_t)stream, T, V, tets, workspace, n_one, n_two, edges_workspace, host_num_unique);
}

#define KAMD_MT_ENTRIES(SFX, CT)                                                                                              \
  int kamd_marching_tetrahedra_classify_##SFX(void* stream, int64_t T, int64_t V, const int64_t* tets, const CT* sdf,           \
                                              void* workspace, int64_t* host_counts) {                                        \
    return mt_classify<CT>((hipStream_t)stream, T, V, tets, sdf, workspace, host_counts);                                     \
  }                                                                                                                           \
  int kamd_marching_tetrahedra_emit_##SFX(void* stream, int64_t V, const int64_t* tets, const CT* vertices, const CT* sdf,     \
                                          const void* edges_workspace, int64_t n_one, int64_t n_two, int64_t num_unique,      \
                                          CT* verts, int64_t* edges, int64_t* faces, int64_t* tet_idx) {                      \
    return mt_emit<CT>((hipStream_t)stream, V, tets, vertices, sdf, edges_workspace, n_one, n_two, num_unique, verts, edges,  \
                       faces, tet_idx);                                                                                       \
  }                                                                                                                           \
  int kamd_marching_tetrahedra_backward_##SFX(void* stream, int64_t num_edges, int64_t V, const int64_t* edges,                \
                                              const CT* vertices, const CT* sdf, const CT* grad_verts, CT* grad_vertices,     \
                                              CT* grad_sdf) {                                                                 \
    return mt_backward<CT>((hipStream_t)stream, num_edges, V, edges, vertices, sdf, grad_verts, grad_vertices, grad_sdf);     \
  }
KAMD_MT_ENTRIES(f32, float)
KAMD_MT_ENTRIES(f64, double)
#undef KAMD_MT_ENTRIES

}  // extern "C"
