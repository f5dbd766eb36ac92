// The linear solve of a Newton step on the reduced (Simplicits) Hessian: a blocked Cholesky factorisation A = L L^T of a symmetric
// positive definite float32 matrix of n <= 1536 = 12 * 128 rows and the two substitutions for one right-hand side (the reference
// calls torch.linalg.solve, a pivoted LU, in kaolin/physics/common/optimization.py).  -ffp-contract=off: every fused multiply-add
// below is spelled.  No atomics, every sum in one fixed order: the same bits on every call; no host read: capturable.
//
// PANELS of NB = 64 columns, T = ceil(n / 64) of them, right-looking.  The working copy Aw of the lower triangle lives in the workspace
// as T x T tiles of 64 x 64, each tile stored COLUMN-major (element (r, c) at c * 64 + r): that is the depth-major image both matrix
// operands below want, so a tile goes to LDS by a straight copy.  Past n a tile holds zeros with ones on the diagonal, so the factor of
// the padded matrix is blockdiag(L, I) and no kernel needs a bound inside the workspace.
//
// 0. spd_load_kernel, grid (T, T): a tile on or under the diagonal: A -> Aw through LDS (read along rows, written along columns;
//    a diagonal tile reads c <= r only and mirrors); a tile above it: zeros to L.  Sets info = 0.
// then, for every panel k:
// 1. spd_diag_kernel, ONE workgroup: Aw[k,k] -> LDS -> the registers of wavefront 0, lane i holding row i.  The 64 columns are
//    factored without a barrier: pivot and column by v_readlane (the lane index is a constant after unrolling), one division per
//    row, a rank-1 update of the columns to the right.  The first pivot that is <= 0 or not finite sets info = its 1-based column
//    and nothing is stored.  Then X = L_kk^-1 by forward substitution on the identity, lane c holding column c.  Both go back
//    through LDS (stride 65): L_kk to L (zeros above the diagonal, nothing past n), X transposed to slot k of the
//    workspace: V[m][c] = L_kk^-1[c][m], the depth-major image of the next kernel and the transpose the solve reads.
// 2. spd_update_kernel, one workgroup per tile (i, j), i >= j > k, four wavefronts: LDS images (stride 80: lanes l and l + 16 read
//    rows 80 dwords apart -> other banks) of V, Aw[i,k] and Aw[j,k].
//      L_i^T = L_kk^-1 Aw[i,k]^T   (wavefront w: rows 16 w .. 16 w + 15 of L_i^T = columns of L_i, depth 16 (w + 1): V is triangular)
//      L_j^T likewise (a diagonal tile: L_i alone)
//    by v_mfma_f32_16x16x4_f32, the accumulators written back over the two tile images (L_i^T, L_j^T are again depth-major images),
//      Aw[i,j] <- Aw[i,j] - L_i L_j^T   (the product of depth 64 is summed from zero and subtracted once: an entry of Aw is rounded
//                                       at its full size once a panel, not once a matrix instruction; measured, LL^T - A fell from
//                                       7.2 to 1.6 times LAPACK's at n = 1536.       A diagonal tile computes the 16 x 16 blocks on
//                                       and under the diagonal only)
//    one float4 per lane and block in and out.  The tiles of column j = k + 1 store L_i to L[i,k].
// solve: 3. spd_solve_kernel, ONE workgroup of 1024 threads, y and x in LDS.  Two fixed lane splits:
//      rows . vector: wavefront w owns rows 4 w .. 4 w + 3, its lanes stride over the columns (contiguous loads), butterfly
//      columns . vector: lane = column (contiguous loads), wavefront w sums rows w, w + 16, ...; the 16 partials are added in order
//    forward, block k up:  t = b_k - L[k, 0..k) y (rows)        y_k = L_kk^-1 t  = columns of V_k . t
//    backward, block k down: t = y_k - L[k+1.., k]^T x (columns)  x_k = L_kk^-T t = rows of V_k . t
//    After a failed factorisation (info != 0) every launch returns at once.
// LDS: load 16.3 KiB, diag 16.3 KiB (one buffer, L then X), update 60 KiB (three images), solve 10.3 KiB.
#include "common.h"
#include "../../include/kaolin_amd.h"

namespace {

typedef float spd_f32x4 __attribute__((ext_vector_type(4)));

constexpr int SPD_NB = 64;                 // panel width = tile side
constexpr int SPD_MAX_N = 1536;
constexpr int SPD_TILE = SPD_NB * SPD_NB;  // floats of a tile
constexpr int SPD_LS = SPD_NB + 16;        // stride of the update kernel's images
constexpr int SPD_PS = SPD_NB + 1;         // stride of the transposing buffers
constexpr int SPD_THREADS = 256;
constexpr int SPD_SOLVE_THREADS = 1024;
constexpr int SPD_SOLVE_WAVES = SPD_SOLVE_THREADS / KAMD_WAVE;
constexpr int SPD_SOLVE_ROWS = SPD_NB / SPD_SOLVE_WAVES;   // rows of a block per wavefront

inline int spd_tiles(int n) { return (n + SPD_NB - 1) / SPD_NB; }
inline bool spd_size_ok(int64_t n) { return n >= 1 && n <= SPD_MAX_N; }

struct SpdWork {
  float* V;    // (T, 64, 64): V[k][m][c] = L_kk^-1[c][m]
  float* Aw;   // (T, T) tiles, column-major inside
};
inline SpdWork spd_carve(void* workspace, int T) {
  SpdWork w;
  w.V = (float*)workspace;
  w.Aw = w.V + (size_t)T * SPD_TILE;
  return w;
}

__device__ __forceinline__ float spd_lane(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// ---- 0. A -> Aw, zeros above the diagonal of L ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SPD_THREADS) void spd_load_kernel(int n, int T, const float* __restrict__ A, float* __restrict__ L,
                                                               float* __restrict__ Aw, int* __restrict__ info) {
  __shared__ float s[SPD_NB * SPD_PS];
  const int t = threadIdx.x, ti = blockIdx.y, tj = blockIdx.x, i0 = ti * SPD_NB, j0 = tj * SPD_NB;
  if (ti == 0 && tj == 0 && t == 0) info[0] = 0;
  if (ti < tj) {
    for (int e = t; e < SPD_TILE; e += SPD_THREADS) {
      const int row = i0 + (e >> 6), col = j0 + (e & 63);
      if (row < n && col < n) L[(size_t)row * n + col] = 0.0f;
    }
    return;
  }
  for (int e = t; e < SPD_TILE; e += SPD_THREADS) {
    const int r = e >> 6, c = e & 63, row = i0 + r, col = j0 + c;
    float v = row == col ? 1.0f : 0.0f;
    if (row < n && col < n) v = col <= row ? A[(size_t)row * n + col] : 0.0f;
    s[r * SPD_PS + c] = v;
  }
  __syncthreads();
  float* tile = Aw + ((size_t)ti * T + tj) * SPD_TILE;
  for (int e = t; e < SPD_TILE; e += SPD_THREADS) {
    const int c = e >> 6, r = e & 63;
    tile[e] = (ti == tj && c > r) ? s[c * SPD_PS + r] : s[r * SPD_PS + c];
  }
}

// ---- 1. the diagonal block ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SPD_THREADS) void spd_diag_kernel(int n, int T, int k, float* __restrict__ L, SpdWork w,
                                                               int* __restrict__ info) {
  __shared__ float s[SPD_NB * SPD_PS];
  __shared__ int s_fail;
  if (info[0] != 0) return;
  const int t = threadIdx.x, k0 = k * SPD_NB;
  const float* tile = w.Aw + ((size_t)k * T + k) * SPD_TILE;
  for (int e = t; e < SPD_TILE; e += SPD_THREADS) s[(e >> 6) * SPD_PS + (e & 63)] = tile[e];   // s[c][r]
  __syncthreads();
  float a[SPD_NB], x[SPD_NB];
  int fail = 0;
  if (t < KAMD_WAVE) {
#pragma unroll
    for (int c = 0; c < SPD_NB; ++c) a[c] = s[c * SPD_PS + t];
    // lane i: row i.  Entries above the diagonal are never read
#pragma unroll
    for (int j = 0; j < SPD_NB; ++j) {
      const float p = spd_lane(a[j], j);
      if (fail == 0 && (!(p > 0.0f) || !(p <= 3.402823466e38f))) fail = j + 1;
      const float d = sqrtf(p);
      a[j] = t == j ? d : a[j] / d;
#pragma unroll
      for (int c = j + 1; c < SPD_NB; ++c) a[c] = fmaf(-a[j], spd_lane(a[j], c), a[c]);
    }
    // lane c: column c of X = L^-1, row by row
#pragma unroll
    for (int r = 0; r < SPD_NB; ++r) {
      float v = t == r ? 1.0f : 0.0f;
#pragma unroll
      for (int m = 0; m < r; ++m) v = fmaf(-spd_lane(a[m], r), x[m], v);
      x[r] = v / spd_lane(a[r], r);
    }
    if (t == 0) s_fail = fail;
  }
  __syncthreads();   // the tile is in registers: s is free
  if (s_fail != 0) {
    if (t == 0) info[0] = k0 + s_fail;
    return;
  }
  if (t < KAMD_WAVE) {
#pragma unroll
    for (int c = 0; c < SPD_NB; ++c) s[t * SPD_PS + c] = c <= t ? a[c] : 0.0f;   // s[r][c]
  }
  __syncthreads();
  for (int e = t; e < SPD_TILE; e += SPD_THREADS) {
    const int row = k0 + (e >> 6), col = k0 + (e & 63);
    if (row < n && col < n) L[(size_t)row * n + col] = s[(e >> 6) * SPD_PS + (e & 63)];
  }
  __syncthreads();
  if (t < KAMD_WAVE) {
#pragma unroll
    for (int r = 0; r < SPD_NB; ++r) s[t * SPD_PS + r] = x[r];   // s[m][c] = X[c][m]: lane m holds column m
  }
  __syncthreads();
  float* V = w.V + (size_t)k * SPD_TILE;
  for (int e = t; e < SPD_TILE; e += SPD_THREADS) V[e] = s[(e >> 6) * SPD_PS + (e & 63)];
}

// ---- 2. the trailing tiles ------------------------------------------------------------------------------------------------------------------
// tile y of the lower triangle, row by row: tj <= ti
__device__ __forceinline__ void spd_lower_tile(int y, int& ti, int& tj) {
  ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= y) ++ti;
  tj = y - ti * (ti + 1) / 2;
}
// a tile (or V) -> its image
__device__ __forceinline__ void spd_stage(const float* __restrict__ tile, float* image) {
  for (int e = threadIdx.x * 4; e < SPD_TILE; e += SPD_THREADS * 4) {
    const spd_f32x4 v = *(const spd_f32x4*)(tile + e);
    *(spd_f32x4*)(image + (e >> 6) * SPD_LS + (e & 63)) = v;
  }
}
// acc[rb] = rows 16 wave .. of V^T-image^T times the tile image: (L_X^T)[16 wave + 4 (lane >> 4) + reg][16 rb + (lane & 15)]
__device__ __forceinline__ void spd_panel_product(const float* s_V, const float* s_X, int wave, int lane, spd_f32x4 (&acc)[4]) {
  const int kq = lane >> 4, rr = lane & 15;
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) acc[rb] = spd_f32x4{0.f, 0.f, 0.f, 0.f};
  for (int d = 0; d < 16 * (wave + 1); d += 4) {
    const float av = s_V[(d + kq) * SPD_LS + wave * 16 + rr];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
      acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, s_X[(d + kq) * SPD_LS + rb * 16 + rr], acc[rb], 0, 0, 0);
  }
}
__device__ __forceinline__ void spd_keep_product(const spd_f32x4 (&acc)[4], float* s_X, int wave, int lane) {
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int j = 0; j < 4; ++j) s_X[(wave * 16 + (lane >> 4) * 4 + j) * SPD_LS + rb * 16 + (lane & 15)] = acc[rb][j];
}

__global__ __launch_bounds__(SPD_THREADS) void spd_update_kernel(int n, int T, int k, float* __restrict__ L, SpdWork w,
                                                                 const int* __restrict__ info) {
  __shared__ __attribute__((aligned(16))) float s_V[SPD_NB * SPD_LS], s_I[SPD_NB * SPD_LS], s_J[SPD_NB * SPD_LS];
  if (info[0] != 0) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int ti, tj;
  spd_lower_tile((int)blockIdx.x, ti, tj);
  ti += k + 1, tj += k + 1;
  const bool diag = ti == tj;
  spd_stage(w.V + (size_t)k * SPD_TILE, s_V);
  spd_stage(w.Aw + ((size_t)ti * T + k) * SPD_TILE, s_I);
  if (!diag) spd_stage(w.Aw + ((size_t)tj * T + k) * SPD_TILE, s_J);
  __syncthreads();
  spd_f32x4 li[4], lj[4];
  spd_panel_product(s_V, s_I, wave, lane, li);
  if (!diag) spd_panel_product(s_V, s_J, wave, lane, lj);
  __syncthreads();   // the tile images are no longer read
  spd_keep_product(li, s_I, wave, lane);
  if (!diag) spd_keep_product(lj, s_J, wave, lane);
  __syncthreads();
  if (tj == k + 1) {   // s_I[c][r] = L_i[r][c]; 16 rows a pass, 16 columns a row segment
    const int i0 = ti * SPD_NB, k0 = k * SPD_NB;
    for (int cb = 0; cb < 4; ++cb)
      for (int rp = 0; rp < SPD_NB; rp += SPD_THREADS / 16) {
        const int c = cb * 16 + (t & 15), r = rp + (t >> 4);
        if (i0 + r < n) L[(size_t)(i0 + r) * n + k0 + c] = s_I[c * SPD_LS + r];
      }
  }
  // Aw[i,j] -= L_i L_j^T
  const float* s_B = diag ? s_I : s_J;
  float* tile = w.Aw + ((size_t)ti * T + tj) * SPD_TILE;
  const int kq = lane >> 4, rr = lane & 15;
  spd_f32x4 acc[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) acc[cb] = spd_f32x4{0.f, 0.f, 0.f, 0.f};
  for (int d = 0; d < SPD_NB; d += 4) {
    const float av = s_I[(d + kq) * SPD_LS + wave * 16 + rr];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
      if (!diag || cb <= wave)
        acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, s_B[(d + kq) * SPD_LS + cb * 16 + rr], acc[cb], 0, 0, 0);
  }
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
    if (!diag || cb <= wave) {
      spd_f32x4* at = (spd_f32x4*)(tile + (cb * 16 + rr) * SPD_NB + wave * 16 + kq * 4);
      *at = *at - acc[cb];
    }
}

// ---- 3. the substitutions -----------------------------------------------------------------------------------------------------------------
// acc[q] = sum over c < len of M[(4 wave + q) ld + c] v[c], the same in every lane; rows >= rows_valid read nothing and give 0
__device__ __forceinline__ void spd_rows_dot(const float* __restrict__ M, size_t ld, int len, int rows_valid, const float* v,
                                             int wave, int lane, float (&acc)[SPD_SOLVE_ROWS]) {
#pragma unroll
  for (int q = 0; q < SPD_SOLVE_ROWS; ++q) acc[q] = 0.0f;
  for (int c = lane; c < len; c += KAMD_WAVE) {
    const float vc = v[c];
#pragma unroll
    for (int q = 0; q < SPD_SOLVE_ROWS; ++q) {
      const int r = wave * SPD_SOLVE_ROWS + q;
      if (r < rows_valid) acc[q] = fmaf(M[r * ld + c], vc, acc[q]);
    }
  }
#pragma unroll
  for (int m = 1; m < KAMD_WAVE; m <<= 1)
#pragma unroll
    for (int q = 0; q < SPD_SOLVE_ROWS; ++q) acc[q] = acc[q] + __shfl_xor(acc[q], m);
}
// s_p[wave][lane] = sum over r = wave, wave + 16, ... < len of M[r ld + lane] v[r]; columns >= cols_valid read nothing and give 0
__device__ __forceinline__ void spd_cols_dot(const float* __restrict__ M, size_t ld, int len, int cols_valid, const float* v,
                                             int wave, int lane, float* s_p) {
  float acc = 0.0f;
  if (lane < cols_valid)
    for (int r = wave; r < len; r += SPD_SOLVE_WAVES) acc = fmaf(M[r * ld + lane], v[r], acc);
  s_p[wave * SPD_NB + lane] = acc;
}
__device__ __forceinline__ float spd_partials(const float* s_p, int c) {
  float sum = s_p[c];
#pragma unroll
  for (int q = 1; q < SPD_SOLVE_WAVES; ++q) sum = sum + s_p[q * SPD_NB + c];
  return sum;
}

__global__ __launch_bounds__(SPD_SOLVE_THREADS) void spd_solve_kernel(int n, int T, const float* __restrict__ L,
                                                                      const float* __restrict__ b, float* __restrict__ x,
                                                                      const float* __restrict__ V, const int* __restrict__ info) {
  __shared__ float s_y[SPD_MAX_N], s_t[SPD_NB], s_p[SPD_SOLVE_WAVES * SPD_NB];
  if (info[0] != 0) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int e = t; e < T * SPD_NB; e += SPD_SOLVE_THREADS) s_y[e] = e < n ? b[e] : 0.0f;
  __syncthreads();
  float acc[SPD_SOLVE_ROWS];
  for (int k = 0; k < T; ++k) {
    const int k0 = k * SPD_NB, valid = n - k0 < SPD_NB ? n - k0 : SPD_NB;
    spd_rows_dot(L + (size_t)k0 * n, (size_t)n, k0, valid, s_y, wave, lane, acc);
    if (lane < SPD_SOLVE_ROWS) {
      const int r = wave * SPD_SOLVE_ROWS + lane;
      float sum = acc[0];
#pragma unroll
      for (int q = 1; q < SPD_SOLVE_ROWS; ++q) sum = lane == q ? acc[q] : sum;
      s_t[r] = s_y[k0 + r] - sum;
    }
    __syncthreads();
    spd_cols_dot(V + (size_t)k * SPD_TILE, SPD_NB, SPD_NB, SPD_NB, s_t, wave, lane, s_p);
    __syncthreads();
    if (t < SPD_NB) s_y[k0 + t] = spd_partials(s_p, t);
    __syncthreads();
  }
  for (int k = T - 1; k >= 0; --k) {
    const int k0 = k * SPD_NB, valid = n - k0 < SPD_NB ? n - k0 : SPD_NB, below = n - (k0 + SPD_NB);
    const size_t first = below > 0 ? (size_t)(k0 + SPD_NB) * n + k0 : 0;
    spd_cols_dot(L + first, (size_t)n, below, valid, s_y + k0 + SPD_NB, wave, lane, s_p);
    __syncthreads();
    if (t < SPD_NB) s_t[t] = s_y[k0 + t] - spd_partials(s_p, t);
    __syncthreads();
    spd_rows_dot(V + (size_t)k * SPD_TILE, SPD_NB, SPD_NB, SPD_NB, s_t, wave, lane, acc);
    if (lane < SPD_SOLVE_ROWS) {
      float sum = acc[0];
#pragma unroll
      for (int q = 1; q < SPD_SOLVE_ROWS; ++q) sum = lane == q ? acc[q] : sum;
      s_y[k0 + wave * SPD_SOLVE_ROWS + lane] = sum;
    }
    __syncthreads();
  }
  for (int e = t; e < n; e += SPD_SOLVE_THREADS) x[e] = s_y[e];
}

}  // namespace

extern "C" {

int kamd_spd_panel(void) { return SPD_NB; }
int kamd_spd_max_n(void) { return SPD_MAX_N; }

size_t kamd_spd_workspace(int64_t n) {
  if (!spd_size_ok(n)) return 0;
  const size_t T = (size_t)spd_tiles((int)n);
  return (T + T * T) * SPD_TILE * sizeof(float);
}

int kamd_spd_factor_f32(void* stream, int64_t n, const float* A, float* L, int* info, void* workspace) {
  if (!spd_size_ok(n) || A == nullptr || L == nullptr || info == nullptr || workspace == nullptr) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int T = spd_tiles((int)n);
  const SpdWork w = spd_carve(workspace, T);
  hipLaunchKernelGGL(spd_load_kernel, dim3((unsigned)T, (unsigned)T), dim3(SPD_THREADS), 0, st, (int)n, T, A, L, w.Aw, info);
  for (int k = 0; k < T; ++k) {
    hipLaunchKernelGGL(spd_diag_kernel, dim3(1), dim3(SPD_THREADS), 0, st, (int)n, T, k, L, w, info);
    const int m = T - 1 - k;
    if (m > 0)
      hipLaunchKernelGGL(spd_update_kernel, dim3((unsigned)(m * (m + 1) / 2)), dim3(SPD_THREADS), 0, st, (int)n, T, k, L, w,
                         (const int*)info);
  }
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spd_solve_f32(void* stream, int64_t n, const float* L, const float* b, float* x, const int* info, void* workspace) {
  if (!spd_size_ok(n) || L == nullptr || b == nullptr || x == nullptr || info == nullptr || workspace == nullptr)
    return (int)hipErrorInvalidValue;
  const int T = spd_tiles((int)n);
  const SpdWork w = spd_carve(workspace, T);
  hipLaunchKernelGGL(spd_solve_kernel, dim3(1), dim3(SPD_SOLVE_THREADS), 0, (hipStream_t)stream, (int)n, T, L, b, x,
                     (const float*)w.V, info);
  KAMD_RETURN_LAST_ERROR();
}
}
