// ops.spc sparse convolutions: conv3d and conv_transpose3d over the points of an octree level, forward and backward (DESIGN.md,
// "SPC convolutions").
//
// Replaces kaolin/csrc/ops/spc/convolution_cuda.cu and minkowski_conv.cu.  The reference builds, per batch item, a K x n table of
// neighbour indices, scans and compacts it, reads K sizes back one by one and then launches a gather-matmul-scatter kernel per
// kernel offset that adds into the output with float atomics.  Here an output row is a GATHER over its K neighbours, and so is
// every gradient row (the direct map from coarse to fine rows and the transposed map from fine to coarse rows hold the same
// (k, coarse, fine) triples), so the whole operator is, for the whole batch at once:
//   * map:    one thread per (kernel offset, row) walks the octree of the row's item down to the neighbour's level, like
//             sp_query_kernel of spc.hip, and writes the neighbour's packed row or -1 into an int32 (K, n) table;
//   * gather: a workgroup owns SC_ROWS rows x SC_COLS output channels, loops over the kernel offsets (skipping one that has no
//             neighbour in the tile), gathers the neighbours' rows into LDS with zeros for misses, multiplies by W[k] (or W[k]^T)
//             from LDS and accumulates in registers: v_mfma_f32_16x16x4_f32 for float, FMAs for double.  One store per output;
//   * wgrad:  grid (k, slice, tile of W[k]): a workgroup strides over its slice of the rows, gathers X[j] and G[map[k][j]] of the
//             hits into LDS (zeros for misses) and accumulates X^T G in registers; one partial per slice, and a finishing launch
//             sums the slices in index order.
// No compaction, no scan, no host read, no atomics: results are bit-identical from run to run.  Every element of every buffer that
// is read was written before (the map by its kernel, the partials by every (k, slice, tile) workgroup).
// Every data-derived index (octree byte, exsum entry, point, map entry) is compared with the size of its buffer before use.
#include <hip/hip_runtime.h>
#include "common.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr int SC_MAX_LEVEL = 15;
constexpr int SC_MAP_BLOCK = 256;   // threads of the map kernel, one (k, row) each
constexpr int SC_ROWS = 64;         // rows of an output tile of the gather kernel (and of W[k]'s tile in wgrad)
constexpr int SC_COLS = 64;         // output channels of a tile
constexpr int SC_SLICES = 32;       // row slices of the weight gradient
constexpr int SC_META = 6;          // int64 per item after the B + 1 row prefix, see sc_map_kernel
constexpr int SC_BS = SC_COLS + 16; // LDS row stride of a (depth, 64) tile: lanes l and l + 16 read rows 80 dwords apart -> other banks
constexpr int SC_APAD = 2;          // the gathered rows are kept (row, CK + 2): 16 rows x 2 channels of an MFMA operand on 32 banks

template <typename T> struct ScTile;
template <> struct ScTile<float> { static constexpr int CK = 32; };   // channels (gather) / rows (wgrad) staged per step
template <> struct ScTile<double> { static constexpr int CK = 16; };

typedef float sc_f32x4 __attribute__((ext_vector_type(4)));

// 16 bytes of T: the staging loads take them in one instruction where the row length and the base address allow it
template <typename T> struct ScVec;
template <> struct ScVec<float> { typedef float4 type; static constexpr int N = 4; };
template <> struct ScVec<double> { typedef double2 type; static constexpr int N = 2; };
template <typename T>
__device__ __forceinline__ bool sc_vec_ok(const T* base, int64_t row_length) {
  return (row_length % ScVec<T>::N) == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0;
}
// v = the 16 bytes at p (16-byte aligned) if ok, else zeros
template <typename T>
__device__ __forceinline__ void sc_load16(T* v, const T* p, bool ok) {
  typedef typename ScVec<T>::type V;
  if (ok) {
    *reinterpret_cast<V*>(v) = *reinterpret_cast<const V*>(p);
  } else {
#pragma unroll
    for (int i = 0; i < ScVec<T>::N; ++i) v[i] = (T)0;
  }
}

// ---- neighbour map -------------------------------------------------------------------------------------------------------------------
// meta: [0, B]: prefix of the rows per item; then per item: first octree byte, octree bytes, index in `points` of the item's first
// row point, index IN THE ITEM'S HIERARCHY of its first target-level point, target points of the item, packed row of its first
// target point.  Direct (transposed == 0): the target level is row_level + jump and the neighbour of row point p under offset v
// is (p << jump) + v.  Transposed: the target level is row_level - jump and the neighbour is (p - v) >> jump where p - v >= 0
// and divisible by 2^jump.  int32 arithmetic: |p| < 2^15, |v| <= 2^15, jump <= 15.
__global__ __launch_bounds__(SC_MAP_BLOCK) void sc_map_kernel(int transposed, int64_t B, int64_t n, int row_level, int jump,
                                                              int64_t num_bytes, int64_t num_points, int64_t num_targets,
                                                              const unsigned char* __restrict__ octrees,
                                                              const int* __restrict__ exsum, const int16_t* __restrict__ points,
                                                              const int16_t* __restrict__ kvec, const int64_t* __restrict__ meta,
                                                              int* __restrict__ map) {
  const int64_t i = (int64_t)blockIdx.x * SC_MAP_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int k = (int)blockIdx.y;
  int64_t lo = 0, hi = B - 1;  // the last item whose first row is <= i
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (meta[mid] <= i)
      lo = mid;
    else
      hi = mid - 1;
  }
  const int64_t* M = meta + (B + 1) + lo * SC_META;
  const int64_t ostart = M[0], nbytes = M[1], tfirst = M[3], tcount = M[4], trow = M[5];
  const int64_t pp = M[2] + (i - meta[lo]);
  int result = -1;
  if (pp >= 0 && pp < num_points) {
    const int target_level = transposed ? row_level - jump : row_level + jump;
    int c[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int p = points[3 * pp + a], v = kvec[3 * k + a];
      if (transposed) {
        const int u = p - v;
        ok = ok && u >= 0 && (u & ((1 << jump) - 1)) == 0;
        c[a] = u >> jump;
      } else {
        c[a] = p * (1 << jump) + v;
      }
      ok = ok && c[a] >= 0 && c[a] < (1 << target_level);
    }
    int64_t ord = 0;  // the walk of sp_query_kernel, inside the item's bytes
    for (int l = 0; ok && l < target_level; ++l) {
      const int depth = target_level - l - 1;
      const unsigned child = (unsigned)((((c[0] >> depth) & 1) << 2) | (((c[1] >> depth) & 1) << 1) | ((c[2] >> depth) & 1));
      ok = false;
      if (ord >= 0 && ord < nbytes && ostart + ord < num_bytes) {
        const unsigned bits = octrees[ostart + ord];
        if ((bits >> child) & 1u) {
          ord = (ord == 0 ? 0 : (int64_t)exsum[ostart + ord - 1]) + __popc(bits & ((2u << child) - 1u));
          ok = true;
        }
      }
    }
    if (ok) {
      const int64_t r = ord - tfirst;  // the point's rank in its level -> packed row
      if (r >= 0 && r < tcount && trow + r >= 0 && trow + r < num_targets) result = (int)(trow + r);
    }
  }
  map[(int64_t)k * n + i] = result;
}

// ---- tiles of the two GEMM kernels ---------------------------------------------------------------------------------------------------
// out[r][c] += sum_d L(d, r) * R[d][c], d < depth, r and c in [0, 64): R is a (depth, SC_BS) LDS image, L(d, r) = L[d * ld + r * lr]
// (the gather keeps its rows row-major, the weight gradient depth-major).  float: wave w owns rows 16 w ... 16 w + 15 and four
// 16-column blocks (four independent accumulators),
// mfma_f32_16x16x4f32: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], D[row 4 (l >> 4) + reg][col l & 15].
// double: thread t owns the 4 x 4 block at rows 4 (t >> 4), columns 4 (t & 15).
template <typename T>
struct ScAcc;
template <>
struct ScAcc<float> {
  sc_f32x4 v[4];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int b = 0; b < 4; ++b) v[b] = sc_f32x4{0.f, 0.f, 0.f, 0.f};
  }
  __device__ __forceinline__ void step(const float* L, int ld, int lr, const float* R, int depth) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane >> 4, r = lane & 15;
    for (int d = 0; d < depth; d += 4) {
      const float a = L[(d + q) * ld + (wave * 16 + r) * lr];
#pragma unroll
      for (int b = 0; b < 4; ++b) v[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, R[(d + q) * SC_BS + b * 16 + r], v[b], 0, 0, 0);
    }
  }
  // f(row in tile, column in tile, value)
  template <typename F>
  __device__ __forceinline__ void each(F f) const {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int j = 0; j < 4; ++j) f(wave * 16 + (lane >> 4) * 4 + j, b * 16 + (lane & 15), v[b][j]);
  }
};
template <>
struct ScAcc<double> {
  double v[4][4];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) v[a][b] = 0.0;
  }
  __device__ __forceinline__ void step(const double* L, int ld, int lr, const double* R, int depth) {
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    for (int d = 0; d < depth; ++d) {
      double l[4], r[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) l[a] = L[d * ld + (ty * 4 + a) * lr], r[a] = R[d * SC_BS + tx * 4 + a];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) v[a][b] = fma(l[a], r[b], v[a][b]);
    }
  }
  template <typename F>
  __device__ __forceinline__ void each(F f) const {
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) f(ty * 4 + a, tx * 4 + b, v[a][b]);
  }
};

// ---- gather-GEMM ---------------------------------------------------------------------------------------------------------------------
// Y[i][n0 ...] = sum_k A[map[k][i]][:] . B_k, B_k[c][col] = W[k][c][col] (W (K, C, N)) or, transpose_w, W[k][col][c] (W (K, N, C)).
// LDS: the gathered rows s_a[row][c] and s_b[c][col]; channels past C are zero in BOTH (so that
// nothing uninitialised meets a zero), a missed row is zero, columns past N are zero and never stored.
template <typename T>
__global__ __launch_bounds__(256) void sc_gather_kernel(int64_t n, int64_t K, int64_t a_rows, int64_t C, int64_t N, int transpose_w,
                                                        const int* __restrict__ map, const T* __restrict__ A,
                                                        const T* __restrict__ W, T* __restrict__ Y) {
  constexpr int CK = ScTile<T>::CK;
  constexpr int AS = CK + SC_APAD;
  constexpr int VN = ScVec<T>::N;
  typedef typename ScVec<T>::type V;
  __shared__ __align__(16) T s_a[SC_ROWS * AS];
  __shared__ __align__(16) T s_b[CK * SC_BS];
  __shared__ int s_map[SC_ROWS];
  const int t = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * SC_ROWS, n0 = (int64_t)blockIdx.y * SC_COLS;
  const bool vec_a = sc_vec_ok(A, C);                           // rows of A (and of W^T) in 16-byte pieces
  const bool vec_w = sc_vec_ok(W, transpose_w ? C : N);         // (C N is then a multiple too: every W[k] is aligned)
  ScAcc<T> acc;
  acc.clear();
  for (int64_t k = 0; k < K; ++k) {
    int m = -1;
    if (t < SC_ROWS && row0 + t < n) {
      m = map[k * n + row0 + t];
      if (m < 0 || (int64_t)m >= a_rows) m = -1;  // the row of A
    }
    __syncthreads();  // the previous offset's s_map and tiles are no longer read
    if (t < SC_ROWS) s_map[t] = m;
    if (!__syncthreads_or(m >= 0)) continue;  // no row of the tile has this neighbour
    const T* Wk = W + k * C * N;
    for (int64_t c0 = 0; c0 < C; c0 += CK) {
      if (c0 > 0) __syncthreads();
      if (vec_a) {
        for (int e = t; e < SC_ROWS * (CK / VN); e += 256) {  // lanes along the channels of a row, 16 bytes each
          const int r = e / (CK / VN), c = (e % (CK / VN)) * VN;
          const int mr = s_map[r];
          __align__(16) T v[VN];
          sc_load16(v, A + (int64_t)mr * C + c0 + c, mr >= 0 && c0 + c < C);
#pragma unroll
          for (int i = 0; i < VN; ++i) s_a[r * AS + c + i] = v[i];
        }
      } else {
        for (int e = t; e < SC_ROWS * CK; e += 256) {  // lanes along the channels of a row
          const int r = e / CK, c = e % CK;
          const int mr = s_map[r];
          s_a[r * AS + c] = (mr >= 0 && c0 + c < C) ? A[(int64_t)mr * C + c0 + c] : (T)0;
        }
      }
      if (transpose_w && vec_w) {
        for (int e = t; e < SC_COLS * (CK / VN); e += 256) {  // lanes along the columns: 16 bytes of a column's channels each
          const int col = e % SC_COLS, c = (e / SC_COLS) * VN;
          __align__(16) T v[VN];
          sc_load16(v, Wk + (n0 + col) * C + c0 + c, c0 + c < C && n0 + col < N);
#pragma unroll
          for (int i = 0; i < VN; ++i) s_b[(c + i) * SC_BS + col] = v[i];
        }
      } else if (transpose_w) {
        for (int e = t; e < SC_COLS * CK; e += 256) {  // 4 consecutive channels of a column per 4 lanes
          const int col = (e >> 2) & (SC_COLS - 1), c = (e & 3) + 4 * (e / (4 * SC_COLS));
          s_b[c * SC_BS + col] = (c0 + c < C && n0 + col < N) ? Wk[(n0 + col) * C + c0 + c] : (T)0;
        }
      } else if (vec_w) {
        for (int e = t; e < CK * (SC_COLS / VN); e += 256) {
          const int c = e / (SC_COLS / VN), col = (e % (SC_COLS / VN)) * VN;
          __align__(16) T v[VN];
          sc_load16(v, Wk + (c0 + c) * N + n0 + col, c0 + c < C && n0 + col < N);
          *reinterpret_cast<V*>(&s_b[c * SC_BS + col]) = *reinterpret_cast<const V*>(v);
        }
      } else {
        for (int e = t; e < SC_COLS * CK; e += 256) {
          const int c = e / SC_COLS, col = e % SC_COLS;
          s_b[c * SC_BS + col] = (c0 + c < C && n0 + col < N) ? Wk[(c0 + c) * N + n0 + col] : (T)0;
        }
      }
      __syncthreads();
      const int64_t left = C - c0;
      acc.step(s_a, 1, AS, s_b, left >= CK ? CK : (int)((left + 3) & ~(int64_t)3));
    }
  }
  acc.each([&](int r, int c, T value) {
    if (row0 + r < n && n0 + c < N) Y[(row0 + r) * N + n0 + c] = value;
  });
}

// ---- weight gradient -------------------------------------------------------------------------------------------------------------------
// partial[k][slice][ci][co] = sum over the rows j of the slice with a neighbour of X[j][ci] * G[map[k][j]][co]; grid (k, slice,
// tile of (cin, cout)).  LDS: s_x[j][ci], s_g[j][co] (depth = row); a missed row is zero in BOTH.
template <typename T>
__global__ __launch_bounds__(256) void sc_wgrad_kernel(int64_t n, int64_t g_rows, int64_t cin, int64_t cout, int64_t rows_per_slice,
                                                       const int* __restrict__ map, const T* __restrict__ X,
                                                       const T* __restrict__ G, T* __restrict__ partial) {
  constexpr int CK = ScTile<T>::CK;
  constexpr int VN = ScVec<T>::N;
  typedef typename ScVec<T>::type V;
  __shared__ __align__(16) T s_x[CK * SC_BS];
  __shared__ __align__(16) T s_g[CK * SC_BS];
  __shared__ int s_map[CK];
  const bool vec = sc_vec_ok(X, cin) && sc_vec_ok(G, cout);
  const int t = threadIdx.x;
  const int64_t k = blockIdx.x, slice = blockIdx.y;
  const int64_t tiles_out = (cout + SC_COLS - 1) / SC_COLS;
  const int64_t i0 = ((int64_t)blockIdx.z / tiles_out) * SC_ROWS, o0 = ((int64_t)blockIdx.z % tiles_out) * SC_COLS;
  int64_t j_end = (slice + 1) * rows_per_slice;
  if (j_end > n) j_end = n;
  ScAcc<T> acc;
  acc.clear();
  for (int64_t j0 = slice * rows_per_slice; j0 < j_end; j0 += CK) {
    int m = -1;
    if (t < CK && j0 + t < j_end) {
      m = map[k * n + j0 + t];
      if (m < 0 || (int64_t)m >= g_rows) m = -1;  // the row of G
    }
    __syncthreads();  // the previous step's s_map and tiles are no longer read
    if (t < CK) s_map[t] = m;
    if (!__syncthreads_or(m >= 0)) continue;  // no hit in these rows
    if (vec) {
      for (int e = t; e < CK * (SC_COLS / VN); e += 256) {  // 16 bytes of a row each
        const int j = e / (SC_COLS / VN), c = (e % (SC_COLS / VN)) * VN;
        const int mj = s_map[j];
        __align__(16) T x[VN], g[VN];
        sc_load16(x, X + (j0 + j) * cin + i0 + c, mj >= 0 && i0 + c < cin);
        sc_load16(g, G + (int64_t)mj * cout + o0 + c, mj >= 0 && o0 + c < cout);
        *reinterpret_cast<V*>(&s_x[j * SC_BS + c]) = *reinterpret_cast<const V*>(x);
        *reinterpret_cast<V*>(&s_g[j * SC_BS + c]) = *reinterpret_cast<const V*>(g);
      }
    } else {
      for (int e = t; e < CK * SC_BS; e += 256) {
        const int j = e / SC_BS, c = e % SC_BS;
        if (c >= SC_COLS) continue;
        const bool hit = s_map[j] >= 0;
        s_x[e] = (hit && i0 + c < cin) ? X[(j0 + j) * cin + i0 + c] : (T)0;
        s_g[e] = (hit && o0 + c < cout) ? G[(int64_t)s_map[j] * cout + o0 + c] : (T)0;
      }
    }
    __syncthreads();
    acc.step(s_x, SC_BS, 1, s_g, CK);
  }
  T* P = partial + (k * SC_SLICES + slice) * cin * cout;
  acc.each([&](int r, int c, T value) {
    if (i0 + r < cin && o0 + c < cout) P[(i0 + r) * cout + o0 + c] = value;
  });
}
// gW[k][e] = the slices' partials added in index order
template <typename T>
__global__ __launch_bounds__(256) void sc_wgrad_finish_kernel(int64_t K, int64_t per_k, const T* __restrict__ partial,
                                                              T* __restrict__ gW) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < K * per_k; e += (int64_t)gridDim.x * 256) {
    const int64_t k = e / per_k, r = e - k * per_k;
    const T* P = partial + k * SC_SLICES * per_k + r;
    T sum = P[0];
    for (int s = 1; s < SC_SLICES; ++s) sum += P[s * per_k];
    gW[e] = sum;
  }
}

inline bool sc_sizes_ok(int64_t n, int64_t K) { return n >= 0 && K >= 1 && K <= 65535 && n <= 0x7FFFFFFFLL / K; }

template <typename T>
int sc_gather(void* stream, int64_t n, int64_t K, int64_t a_rows, int64_t C, int64_t N, int transpose_w, const int32_t* map,
              const T* A, const T* W, T* Y) {
  if (!sc_sizes_ok(n, K) || a_rows < 0 || C < 1 || N < 1 || a_rows > 0x7FFFFFFFLL) return (int)hipErrorInvalidValue;
  const int64_t gy = (N + SC_COLS - 1) / SC_COLS;
  if (gy > 65535) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  hipLaunchKernelGGL((sc_gather_kernel<T>), dim3((unsigned)((n + SC_ROWS - 1) / SC_ROWS), (unsigned)gy), dim3(256), 0,
                     (hipStream_t)stream, n, K, a_rows, C, N, transpose_w, map, A, W, Y);
  KAMD_RETURN_LAST_ERROR();
}

template <typename T>
int sc_wgrad(void* stream, int64_t n, int64_t K, int64_t g_rows, int64_t cin, int64_t cout, const int32_t* map, const T* X,
             const T* G, void* workspace, size_t workspace_bytes, T* gW) {
  if (!sc_sizes_ok(n, K) || g_rows < 0 || g_rows > 0x7FFFFFFFLL || cin < 1 || cout < 1) return (int)hipErrorInvalidValue;
  const int64_t tiles = ((cin + SC_ROWS - 1) / SC_ROWS) * ((cout + SC_COLS - 1) / SC_COLS);
  if (tiles > 65535) return (int)hipErrorInvalidValue;
  if (workspace == nullptr || workspace_bytes < kamd_spc_conv_workspace(K, cin, cout, (int)sizeof(T))) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  constexpr int CK = ScTile<T>::CK;
  int64_t per = (n + SC_SLICES - 1) / SC_SLICES;  // rows per slice, a multiple of the staging depth
  per = (per + CK - 1) / CK * CK;
  if (per < CK) per = CK;
  hipLaunchKernelGGL((sc_wgrad_kernel<T>), dim3((unsigned)K, SC_SLICES, (unsigned)tiles), dim3(256), 0, st, n, g_rows, cin, cout, per,
                     map, X, G, (T*)workspace);
  int64_t blocks = (K * cin * cout + 255) / 256;
  if (blocks > (int64_t)KAMD_NUM_CU * 16) blocks = (int64_t)KAMD_NUM_CU * 16;
  hipLaunchKernelGGL((sc_wgrad_finish_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, st, K, cin * cout, (const T*)workspace, gW);
  KAMD_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {

int kamd_spc_conv_map(void* stream, int transposed, int64_t B, int64_t K, int64_t n, int row_level, int jump, int64_t num_bytes,
                      int64_t num_points, int64_t num_targets, const uint8_t* octrees, const int32_t* exsum, const int16_t* points,
                      const int16_t* kernel_vectors, const int64_t* meta, int32_t* map) {
  const int target_level = transposed ? row_level - jump : row_level + jump;
  if (!sc_sizes_ok(n, K) || B < 1 || jump < 0 || row_level < 0 || row_level > SC_MAX_LEVEL || target_level < 0 ||
      target_level > SC_MAX_LEVEL || num_bytes < 0 || num_points < 0 || num_targets < 0 || num_targets > 0x7FFFFFFFLL)
    return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  hipLaunchKernelGGL(sc_map_kernel, dim3((unsigned)((n + SC_MAP_BLOCK - 1) / SC_MAP_BLOCK), (unsigned)K), dim3(SC_MAP_BLOCK), 0,
                     (hipStream_t)stream, transposed, B, n, row_level, jump, num_bytes, num_points, num_targets, octrees, exsum,
                     points, kernel_vectors, meta, map);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spc_conv_gather_f32(void* stream, int64_t n, int64_t K, int64_t a_rows, int64_t C, int64_t N, int transpose_w,
                             const int32_t* map, const float* A, const float* W, float* Y) {
  return sc_gather<float>(stream, n, K, a_rows, C, N, transpose_w, map, A, W, Y);
}
int kamd_spc_conv_gather_f64(void* stream, int64_t n, int64_t K, int64_t a_rows, int64_t C, int64_t N, int transpose_w,
                             const int32_t* map, const double* A, const double* W, double* Y) {
  return sc_gather<double>(stream, n, K, a_rows, C, N, transpose_w, map, A, W, Y);
}

size_t kamd_spc_conv_workspace(int64_t K, int64_t cin, int64_t cout, int elem_bytes) {
  if (K < 1 || cin < 1 || cout < 1 || elem_bytes < 1) return 0;
  return (size_t)K * SC_SLICES * (size_t)cin * (size_t)cout * (size_t)elem_bytes;
}

int kamd_spc_conv_wgrad_f32(void* stream, int64_t n, int64_t K, int64_t g_rows, int64_t cin, int64_t cout, const int32_t* map,
                            const float* X, const float* G, void* workspace, size_t workspace_bytes, float* grad_weight) {
  return sc_wgrad<float>(stream, n, K, g_rows, cin, cout, map, X, G, workspace, workspace_bytes, grad_weight);
}
int kamd_spc_conv_wgrad_f64(void* stream, int64_t n, int64_t K, int64_t g_rows, int64_t cin, int64_t cout, const int32_t* map,
                            const double* X, const double* G, void* workspace, size_t workspace_bytes, double* grad_weight) {
  return sc_wgrad<double>(stream, n, K, g_rows, cin, cout, map, X, G, workspace, workspace_bytes, grad_weight);
}

}  // extern "C"
