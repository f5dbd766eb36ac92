// ops.gcn: the sparse (M, N) times batched dense (B, N, P) product of sparse_bmm and GraphConv as ONE gather per direction over lists
// built once per graph, without atomics and without a transposed copy of the activations.
//
// The reference (kaolin/ops/gcn.py) moves the dense operand to (N, B P), calls torch.sparse.mm (a library SpMM) and moves the result
// back; GraphConv adds a row-sum product, a division and the self term as kernels of their own.  Here:
//   * the lists, once per graph (kamd_gcn_lists_build): entry e of the COO tensor gives the keys (e << 32) | row and (e << 32) | col;
//     the stable keys-only sort of sort_scan.h over the low ceil(log2 M) (ceil(log2 N)) bits groups the entries by row (by column)
//     and keeps the entries of one row in COO order; offsets[r] = the first sorted position whose row is >= r (a binary search),
//     and the other index and the value of every entry are copied into list order.  The row lists serve the forward, the column
//     lists the gradient;
//   * every step (kamd_gcn_aggregate_*): ONE launch.  The dense operand is C = B P logical columns per node, read in place through
//     its strides, `vec` = 4 columns per lane where rows are 16-byte aligned and P % 4 == 0, else 1.  A wavefront is cut into
//     groups of G lanes, G = the smallest power of two >= min(ceil(C / vec), 64); a group owns one output row (P = 3, B = 1: 16 rows
//     per wavefront) and loops over chunks of G vec columns when C > vec G.  The group's lanes load G consecutive (index, value)
//     entries of the row, one per lane, and walk them with a lane broadcast inside the group: every index is fetched once per group
//     and chunk, there is no LDS and no barrier.  A longer row takes more such rounds in the same loop; no row is split.
//   * the contract: per output element a sequential sum over the row's entries in list order from +0, one rounded multiply and one
//     rounded add per entry (-ffp-contract=off); with `normalize` the row sum norm is the sequential sum of the values in the same
//     order and the result is sum / norm, ONE division (0 / 0 = NaN for a row without entries, as in the reference); the addend is
//     added last, once.  With src_norm every term reads x / src_norm[index] (the gradient of the normalised product).
// Every index that comes from data is compared with its buffer's size before use: a row or column with M or N (the key kernel counts
// the entries outside for the host and files them under 0), an entry with nnz, an offset with nnz, a list index with the source rows.
#include <hip/hip_runtime.h>
#include "common.h"
#include "sort_scan.h"
#include "../../include/kaolin_amd.h"

namespace {

// ---- the lists --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void gcn_clear_kernel(int* bad) {
  if (threadIdx.x == 0) *bad = 0;
}
// indices (2, nnz) int64 through its element strides -> the keys of both sorts
__global__ __launch_bounds__(256) void gcn_keys_kernel(long long nnz, long long M, long long N, const long long* __restrict__ indices,
                                                       long long stride_d, long long stride_e, unsigned long long* __restrict__ row_keys,
                                                       unsigned long long* __restrict__ col_keys, int* __restrict__ bad) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  long long r = indices[e * stride_e], c = indices[stride_d + e * stride_e];
  if (r < 0 || r >= M || c < 0 || c >= N) {  // guard: an entry outside the matrix is counted and filed under (0, 0)
    atomicAdd(bad, 1);
    r = c = 0;
  }
  row_keys[e] = ((unsigned long long)e << 32) | (unsigned long long)r;
  col_keys[e] = ((unsigned long long)e << 32) | (unsigned long long)c;
}
// thread j < nnz: the other index and the value of the j-th sorted entry; thread r <= R: offsets[r] = the first sorted position whose
// key (the low word) is >= r.  `other`: the row of indices the list holds (1: columns, for the row lists), below other_bound
template <typename W>
__global__ __launch_bounds__(256) void gcn_lists_kernel(long long nnz, long long R, const unsigned long long* __restrict__ sorted,
                                                        const long long* __restrict__ indices, long long other, long long other_bound,
                                                        long long stride_d, long long stride_e, const W* __restrict__ values,
                                                        long long stride_v, int* __restrict__ offsets, int* __restrict__ idx,
                                                        W* __restrict__ vals) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < nnz) {
    unsigned long long e = sorted[t] >> 32;
    if (e >= (unsigned long long)nnz) e = 0;  // guard: an entry index outside the nnz entries
    const long long o = indices[other * stride_d + (long long)e * stride_e];
    idx[t] = (o >= 0 && o < other_bound) ? (int)o : 0;  // guard: counted by the key kernel, the caller raises
    vals[t] = values[(long long)e * stride_v];
  }
  if (t <= R) {
    long long lo = 0, hi = nnz;  // the answer stays in [0, nnz] whatever the keys hold
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

// workspace for nnz entries: row keys | column keys | the other side of the ping-pong | sorted keys | the sort's scratch | bad count
struct GcnWs {
  unsigned long long *rk, *ck, *kt, *ks;
  SsSortWs sort;
  int* bad;
  size_t total_bytes;
};
GcnWs gcn_ws(void* base, long long nnz) {
  GcnWs w;
  char* p = (char*)base;
  auto take = [&](size_t bytes) {
    char* r = p;
    p += (bytes + 255) & ~(size_t)255;
    return r;
  };
  const size_t n1 = (size_t)(nnz > 0 ? nnz : 1);
  w.rk = (unsigned long long*)take(n1 * 8);
  w.ck = (unsigned long long*)take(n1 * 8);
  w.kt = (unsigned long long*)take(n1 * 8);
  w.ks = (unsigned long long*)take(n1 * 8);
  w.sort.hist = (int*)take(ss_sort_hist_entries(nnz) * 4);
  w.sort.offs = (long long*)take(ss_sort_offs_entries(nnz) * 8);
  w.sort.sums = (long long*)take(ss_sort_sums_entries(nnz) * 8);
  w.bad = (int*)take(4);
  w.total_bytes = (size_t)(p - (char*)base);
  return w;
}
bool gcn_extents(long long M, long long N, long long nnz) {
  return M > 0 && N > 0 && nnz > 0 && M < 0x7FFFFFFFLL && N < 0x7FFFFFFFLL && nnz < 0x7FFFFFFFLL;
}
int gcn_bits(long long n) {  // ceil(log2 n): the bits that tell the ids 0 .. n - 1 apart
  int bits = 0;
  while (bits < 31 && (1LL << bits) < n) ++bits;
  return bits;
}
// one direction: sorted keys -> offsets (R + 1), idx (nnz), vals (nnz)
template <typename W>
int gcn_lists(hipStream_t st, long long nnz, long long R, const GcnWs& w, const unsigned long long* keys, const long long* indices,
              long long other, long long other_bound, long long stride_d, long long stride_e, const void* values, long long stride_v,
              int* offsets, int* idx, void* vals) {
  KAMD_CHECK(ss_sort(st, nnz, ss_passes_low(gcn_bits(R)), keys, w.kt, w.ks, w.sort));
  const long long threads = nnz > R + 1 ? nnz : R + 1;
  hipLaunchKernelGGL((gcn_lists_kernel<W>), dim3(ss_grid(threads, 256)), dim3(256), 0, st, nnz, R, (const unsigned long long*)w.ks,
                     indices, other, other_bound, stride_d, stride_e, (const W*)values, stride_v, offsets, idx, (W*)vals);
  return (int)hipGetLastError();
}

// ---- the gather -------------------------------------------------------------------------------------------------------------------
constexpr int GCN_NORM = 1;     // divide by the row sum computed in the same pass
constexpr int GCN_ADD = 2;      // add the addend, last
constexpr int GCN_SRC_DIV = 4;  // every term reads x / src_norm[index]
constexpr int GCN_BLOCKS_PER_CU = 8;  // workgroups of 256 threads per CU, at most: the grid strides over the rows

template <typename T, int VEC>
struct alignas(VEC == 4 ? 16 : sizeof(T)) GcnVec {
  T v[VEC];
};

// G = 1 << gshift lanes per output row; a lane owns the vec columns lane, lane + G, ... of the Cv = B P / VEC.  The loops run on
// values the whole group shares (the row, its offsets, the chunk), so the lanes a broadcast reads are active with the reader; a
// lane without a column (`live`) walks along and only skips its loads and its store.
template <typename T, int VEC, int FLAGS>
__global__ __launch_bounds__(256) void gcn_aggregate_kernel(long long R, unsigned S, unsigned nnz, int gshift, long long Cv, long long P,
                                                            const int* __restrict__ offsets, const int* __restrict__ idx,
                                                            const T* __restrict__ vals, const T* __restrict__ x, long long xs_b,
                                                            long long xs_n, long long xs_p, const T* __restrict__ src_norm,
                                                            T* __restrict__ norm_out, const T* __restrict__ addend, long long as_b,
                                                            long long as_n, long long as_p, T* __restrict__ out) {
  using V = GcnVec<T, VEC>;
  const int G = 1 << gshift, lane = (int)threadIdx.x & (G - 1);
  const long long groups = ((long long)gridDim.x * 256) >> gshift;
  for (long long r = ((long long)blockIdx.x * 256 + threadIdx.x) >> gshift; r < R; r += groups) {
    int s = offsets[r], e = offsets[r + 1];
    if (s < 0 || e < s || (unsigned)e > nnz) s = e = 0;  // guard: offsets outside the nnz entries
    for (long long q0 = 0; q0 < Cv; q0 += G) {
      const long long q = q0 + lane;
      const bool live = q < Cv;
      const long long c = live ? q * VEC : 0, b = c / P, p = c - b * P;
      const T* src = x + b * xs_b + p * xs_p;
      V acc;
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc.v[k] = (T)0;
      T norm = (T)0;
      for (long long j = s; j < e; j += G) {  // a round: G entries of the row, one per lane (64 bits: e may be near 2^31)
        int my_idx = 0;
        T my_val = (T)0;
        if (j + lane < e) {
          my_idx = idx[j + lane];
          my_val = vals[j + lane];
        }
        const int count = e - j < G ? (int)(e - j) : G;
        for (int i = 0; i < count; ++i) {
          const int n = __shfl(my_idx, i, G);
          const T w = __shfl(my_val, i, G);
          if (FLAGS & GCN_NORM) norm = norm + w;
          if (live && (unsigned)n < S) {  // guard: an index outside the S source rows adds nothing
            V t = *(const V*)(src + (long long)n * xs_n);
            if (FLAGS & GCN_SRC_DIV) {
              const T d = src_norm[n];
#pragma unroll
              for (int k = 0; k < VEC; ++k) t.v[k] = t.v[k] / d;
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] + w * t.v[k];
          }
        }
      }
      if (live) {
        if (FLAGS & GCN_NORM) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] / norm;
        }
        if (FLAGS & GCN_ADD) {
          const V a = *(const V*)(addend + b * as_b + r * as_n + p * as_p);
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc.v[k] = acc.v[k] + a.v[k];
        }
        *(V*)(out + (b * R + r) * P + p) = acc;
      }
      if ((FLAGS & GCN_NORM) && norm_out != nullptr && q == 0) norm_out[r] = norm;
    }
  }
}

template <typename T, int VEC, int FLAGS>
void gcn_launch(hipStream_t st, unsigned blocks, long long R, long long S, long long nnz, int gshift, long long Cv, long long P,
                const int* offsets, const int* idx, const T* vals, const T* x, long long xs_b, long long xs_n, long long xs_p,
                const T* src_norm, T* norm_out, const T* addend, long long as_b, long long as_n, long long as_p, T* out) {
  hipLaunchKernelGGL((gcn_aggregate_kernel<T, VEC, FLAGS>), dim3(blocks), dim3(256), 0, st, R, (unsigned)S, (unsigned)nnz, gshift, Cv,
                     P, offsets, idx, vals, x, xs_b, xs_n, xs_p, src_norm, norm_out, addend, as_b, as_n, as_p, out);
}
bool gcn_aligned4(const void* p, long long stride_b, long long stride_n, long long stride_p) {
  return ((uintptr_t)p & 15) == 0 && stride_p == 1 && stride_b % 4 == 0 && stride_n % 4 == 0;
}
template <typename T>
int gcn_aggregate(void* stream, int64_t R, int64_t S, int64_t nnz, int64_t B, int64_t P, const int32_t* offsets, const int32_t* idx,
                  const T* vals, const T* x, int64_t xs_b, int64_t xs_n, int64_t xs_p, const T* src_norm, int normalize, T* norm_out,
                  const T* addend, int64_t as_b, int64_t as_n, int64_t as_p, T* out) {
  if (!gcn_extents(R, S, nnz) || B <= 0 || P <= 0 || offsets == nullptr || idx == nullptr || vals == nullptr || x == nullptr ||
      out == nullptr)
    return (int)hipErrorInvalidValue;
  if (B > 0x7FFFFFFFFFFFLL / P || B * P > 0x7FFFFFFFFFFFLL / R) return (int)hipErrorInvalidValue;
  const bool vec4 = P % 4 == 0 && gcn_aligned4(x, xs_b, xs_n, xs_p) && gcn_aligned4(out, R * P, P, 1) &&
                    (addend == nullptr || gcn_aligned4(addend, as_b, as_n, as_p));
  const long long Cv = B * P / (vec4 ? 4 : 1);
  int gshift = 0;
  while (gshift < 6 && (1LL << gshift) < Cv) ++gshift;
  long long blocks = ((R << gshift) + 255) / 256;
  if (blocks > (long long)KAMD_NUM_CU * GCN_BLOCKS_PER_CU) blocks = (long long)KAMD_NUM_CU * GCN_BLOCKS_PER_CU;
  const int flags = (normalize ? GCN_NORM : 0) | (addend != nullptr ? GCN_ADD : 0) | (src_norm != nullptr ? GCN_SRC_DIV : 0);
#define GCN_CASE(F)                                                                                                                 \
  case F:                                                                                                                           \
    if (vec4)                                                                                                                       \
      gcn_launch<T, 4, F>((hipStream_t)stream, (unsigned)blocks, R, S, nnz, gshift, Cv, P, offsets, idx, vals, x, xs_b, xs_n, xs_p,  \
                          src_norm, norm_out, addend, as_b, as_n, as_p, out);                                                       \
    else                                                                                                                            \
      gcn_launch<T, 1, F>((hipStream_t)stream, (unsigned)blocks, R, S, nnz, gshift, Cv, P, offsets, idx, vals, x, xs_b, xs_n, xs_p,  \
                          src_norm, norm_out, addend, as_b, as_n, as_p, out);                                                       \
    break;
  switch (flags) {
    GCN_CASE(0)
    GCN_CASE(1)
    GCN_CASE(2)
    GCN_CASE(3)
    GCN_CASE(4)
    GCN_CASE(5)
    GCN_CASE(6)
    GCN_CASE(7)
  }
#undef GCN_CASE
  KAMD_RETURN_LAST_ERROR();
}

// ---- normalize_adj ------------------------------------------------------------------------------------------------------------------
// one thread per row: the sequential sum of the row's values in list order
template <typename T>
__global__ __launch_bounds__(256) void gcn_row_sums_kernel(long long M, unsigned nnz, const int* __restrict__ offsets,
                                                           const T* __restrict__ vals, T* __restrict__ norm) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= M) return;
  int s = offsets[r], e = offsets[r + 1];
  if (s < 0 || e < s || (unsigned)e > nnz) s = e = 0;  // guard: offsets outside the nnz entries
  T sum = (T)0;
  for (int j = s; j < e; ++j) sum = sum + vals[j];
  norm[r] = sum;
}
// one thread per entry, in the COO's own order: values[e] / norm[row_e]
template <typename T>
__global__ __launch_bounds__(256) void gcn_scale_values_kernel(long long nnz, long long M, const long long* __restrict__ rows,
                                                               long long stride_e, const T* __restrict__ values, long long stride_v,
                                                               const T* __restrict__ norm, T* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  const long long r = rows[e * stride_e];
  const T v = values[e * stride_v];
  out[e] = (r >= 0 && r < M) ? v / norm[r] : v;  // guard: a row outside the M rows (the list build has raised for it)
}
template <typename T>
int gcn_row_sums(void* stream, int64_t M, int64_t nnz, const int32_t* offsets, const T* vals, T* norm) {
  if (!gcn_extents(M, 1, nnz) || offsets == nullptr || vals == nullptr || norm == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((gcn_row_sums_kernel<T>), dim3(ss_grid(M, 256)), dim3(256), 0, (hipStream_t)stream, (long long)M, (unsigned)nnz,
                     offsets, vals, norm);
  KAMD_RETURN_LAST_ERROR();
}
template <typename T>
int gcn_scale_values(void* stream, int64_t M, int64_t nnz, const int64_t* rows, int64_t stride_e, const T* values, int64_t stride_v,
                     const T* norm, T* out) {
  if (!gcn_extents(M, 1, nnz) || rows == nullptr || values == nullptr || norm == nullptr || out == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((gcn_scale_values_kernel<T>), dim3(ss_grid(nnz, 256)), dim3(256), 0, (hipStream_t)stream, (long long)nnz,
                     (long long)M, (const long long*)rows, (long long)stride_e, values, (long long)stride_v, norm, out);
  KAMD_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {

size_t kamd_gcn_lists_workspace(int64_t M, int64_t N, int64_t nnz) {
  if (!gcn_extents(M, N, nnz)) return 0;
  return gcn_ws(nullptr, nnz).total_bytes;
}

int kamd_gcn_lists_build(void* stream, int64_t M, int64_t N, int64_t nnz, const int64_t* indices, int64_t stride_d, int64_t stride_e,
                         const void* values, int value_bytes, int64_t stride_v, void* workspace, size_t workspace_bytes,
                         int32_t* row_offsets, int32_t* cols, void* row_vals, int32_t* col_offsets, int32_t* rows, void* col_vals,
                         int32_t* host_bad) {
  if (!gcn_extents(M, N, nnz) || indices == nullptr || values == nullptr || row_offsets == nullptr || cols == nullptr ||
      row_vals == nullptr || col_offsets == nullptr || rows == nullptr || col_vals == nullptr || host_bad == nullptr)
    return (int)hipErrorInvalidValue;
  if (value_bytes != 4 && value_bytes != 8) return (int)hipErrorInvalidValue;
  if (workspace == nullptr || workspace_bytes < gcn_ws(nullptr, nnz).total_bytes) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const GcnWs w = gcn_ws(workspace, nnz);
  const long long* ind = (const long long*)indices;
  hipLaunchKernelGGL(gcn_clear_kernel, dim3(1), dim3(64), 0, st, w.bad);
  hipLaunchKernelGGL(gcn_keys_kernel, dim3(ss_grid(nnz, 256)), dim3(256), 0, st, (long long)nnz, (long long)M, (long long)N, ind,
                     (long long)stride_d, (long long)stride_e, w.rk, w.ck, w.bad);
  KAMD_CHECK(hipGetLastError());
  if (value_bytes == 4) {
    KAMD_CHECK(gcn_lists<unsigned int>(st, nnz, M, w, w.rk, ind, 1, N, stride_d, stride_e, values, stride_v, row_offsets, cols, row_vals));
    KAMD_CHECK(gcn_lists<unsigned int>(st, nnz, N, w, w.ck, ind, 0, M, stride_d, stride_e, values, stride_v, col_offsets, rows, col_vals));
  } else {
    KAMD_CHECK(gcn_lists<unsigned long long>(st, nnz, M, w, w.rk, ind, 1, N, stride_d, stride_e, values, stride_v, row_offsets, cols,
                                             row_vals));
    KAMD_CHECK(gcn_lists<unsigned long long>(st, nnz, N, w, w.ck, ind, 0, M, stride_d, stride_e, values, stride_v, col_offsets, rows,
                                             col_vals));
  }
  int bad = 0;
  KAMD_CHECK(hipMemcpyAsync(&bad, w.bad, 4, hipMemcpyDeviceToHost, st));  // the one host read
  KAMD_CHECK(hipStreamSynchronize(st));
  *host_bad = bad;
  return 0;
}

int kamd_gcn_aggregate_f32(void* stream, int64_t R, int64_t S, int64_t nnz, int64_t B, int64_t P, const int32_t* offsets,
                           const int32_t* idx, const float* vals, const float* x, int64_t xs_b, int64_t xs_n, int64_t xs_p,
                           const float* src_norm, int normalize, float* norm_out, const float* addend, int64_t as_b, int64_t as_n,
                           int64_t as_p, float* out) {
  return gcn_aggregate<float>(stream, R, S, nnz, B, P, offsets, idx, vals, x, xs_b, xs_n, xs_p, src_norm, normalize, norm_out, addend,
                              as_b, as_n, as_p, out);
}
int kamd_gcn_aggregate_f64(void* stream, int64_t R, int64_t S, int64_t nnz, int64_t B, int64_t P, const int32_t* offsets,
                           const int32_t* idx, const double* vals, const double* x, int64_t xs_b, int64_t xs_n, int64_t xs_p,
                           const double* src_norm, int normalize, double* norm_out, const double* addend, int64_t as_b, int64_t as_n,
                           int64_t as_p, double* out) {
  return gcn_aggregate<double>(stream, R, S, nnz, B, P, offsets, idx, vals, x, xs_b, xs_n, xs_p, src_norm, normalize, norm_out, addend,
                               as_b, as_n, as_p, out);
}
int kamd_gcn_row_sums_f32(void* stream, int64_t M, int64_t nnz, const int32_t* offsets, const float* vals, float* norm) {
  return gcn_row_sums<float>(stream, M, nnz, offsets, vals, norm);
}
int kamd_gcn_row_sums_f64(void* stream, int64_t M, int64_t nnz, const int32_t* offsets, const double* vals, double* norm) {
  return gcn_row_sums<double>(stream, M, nnz, offsets, vals, norm);
}
int kamd_gcn_scale_values_f32(void* stream, int64_t M, int64_t nnz, const int64_t* rows, int64_t stride_e, const float* values,
                              int64_t stride_v, const float* norm, float* out) {
  return gcn_scale_values<float>(stream, M, nnz, rows, stride_e, values, stride_v, norm, out);
}
int kamd_gcn_scale_values_f64(void* stream, int64_t M, int64_t nnz, const int64_t* rows, int64_t stride_e, const double* values,
                              int64_t stride_v, const double* norm, double* out) {
  return gcn_scale_values<double>(stream, M, nnz, rows, stride_e, values, stride_v, norm, out);
}

}  // extern "C"
