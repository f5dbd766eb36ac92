// kaolin.physics scene forces on the GPU: gravity, a floor, pinned points (the reference's kaolin/physics/common/scene_forces.py, NVIDIA
// Warp kernels with atomic_add energies) and the inertia term 1/2 delta^T (B^T M B) delta of a backward-Euler Newton step (the
// reference stores B^T M B, simplicits/simulation.py), per point and reduced to the Simplicits degrees of freedom; float32 only.
//
// THE TERMS, per row: an energy e, a force f (3) and a DIAGONAL Hessian d (3).  x = x0 + dx.
//   gravity  (every point)   m = c_g rho vol:   e = m (g . x)             f = m g                    d = 0
//   floor    (every point, active iff x[a] < h, flipped: x[a] > h, strict)   v = c_f vol, t = x[a] - h:
//                                                e = v t^2                 f[a] = 2 v t               d[a] = 2 v
//   pin k    (one row per pin, on point i_k)     e = c_k |x - y_k|^2       f = 2 c_k (x - y_k)        d = 2 c_k on all axes
//   inertia  (every point, u = B_p delta)        e = 1/2 mass |u|^2        f = mass u                 d = mass on all axes
// Both derivatives are those of the energy written here (the reference negates the flipped floor's gradient and Hessian but not its
// energy).  -ffp-contract=off: every fused multiply-add below is spelled.
//
// 1. sf_terms_kernel: one class' terms on given dx, a thread per point, grid-stride.  The pins of a point are GATHERED: the pin
//    list arrives sorted by point (with each pin's place in the list), a thread finds its point's run by bisection and adds it in
//    order, so duplicate pins need no atomics and give the same bits every run.  Energy: thread (compensated) -> wavefront
//    butterfly -> LDS -> one partial per workgroup; one launch of one thread adds the <= 1024 partials in index order.
//
// 2. sf_reduced_kernel: with W = 4 H and m_p[4 h + n] = w[p][h] (x0_p, 1)[n], the row of the LBS Jacobian B that all three axes
//    share,   dx_p[b] = sum_i m_p[i] z[h(i)][b][n(i)],   u_p likewise from delta = (z - z_prev) - dt z_dot,
//      g[h][b][n]  = sum_rows f[b] m[4 h + n]
//      K_bb[i][j]  = sum_rows d[b] m[i] m[j]        three symmetric W x W rank updates of depth N + pins; K_bb' = 0 for b != b'
//    The row stream is the N points, then the pins (a pin row gathers x0 and the weights of its point; a pin index outside [0, N)
//    reads nothing and is a row of zeros).  The grid (tiles on or under the diagonal), the sums of g and E, the slices' partials and
//    their finish are those of reduced_assembly.h; the partials hold the three blocks of RaDiagonalThree, and the finish writes the
//    zero blocks.  The workgroup walks its slice in chunks of SF_CR = 32 rows.  Per chunk:
//      (a) z and delta are in LDS (staged once)
//      (b) 16 lanes per row (two passes of 16 rows) accumulate dx_p and u_p over the handles h = lane, lane + 16, ... and add up by
//          a butterfly inside their row of 16; the first lane classifies the floor and leaves e (kept), f, d, (x0, 1) and the
//          point's index in LDS
//      (c) all threads write the images of m, rows x 64 columns of the row tile and of the column tile (a diagonal tile: one image)
//      (d) for each axis b: acc[b] += (d[b] m_row)^T m_col, the A operand scaled in the register: no scaled image, no barrier
//          between the axes; 3 x 4 x 4 = 48 accumulator registers.  Blocks past W, and in a diagonal tile above the diagonal, are skipped.
//      g: f[b] m of the row tile; E: e, in the rows' first lanes.
//    HESS = false (a line search's energy and gradient): grid (slice, row tile), no column image, no MFMA.
//    LDS: 2 images of 32 x 80 floats (20 KiB) + z, delta 96 H bytes (12 KiB reserved) + f, d, x, index 1.4 KiB.
#include "reduced_assembly.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr int SF_CR = 32;                      // rows per chunk = GEMM depth of a chunk
constexpr int SF_TPR = 16;                     // lanes per row in stage (b)
constexpr int SF_PASS = RA_THREADS / SF_TPR;   // rows of one pass of stage (b)
constexpr int SF_MAX_SLICES = 128;

// the terms that live on the points; a null first pointer: that term is absent
struct SfScene {
  int64_t N;
  const float* x0;           // (N, 3)
  const float *rho, *gvol;   // gravity
  float g[3], cg;
  const float* fvol;         // floor
  float fh, cf;
  int axis, flip;
  const float* mass;         // inertia
};

__device__ __forceinline__ float sf_dot(const float* u, const float* v) { return fmaf(u[0], v[0], fmaf(u[1], v[1], u[2] * v[2])); }

// e, f, d of point p at x, u = B_p delta
__device__ __forceinline__ float sf_point(const SfScene& s, int64_t p, const float* x, const float* u, float* f, float* d) {
  float e = 0.0f;
#pragma unroll
  for (int b = 0; b < 3; ++b) f[b] = 0.0f, d[b] = 0.0f;
  if (s.rho != nullptr) {
    const float m = s.cg * s.rho[p] * s.gvol[p];
    e = m * sf_dot(s.g, x);
#pragma unroll
    for (int b = 0; b < 3; ++b) f[b] = m * s.g[b];
  }
  if (s.fvol != nullptr) {
    const float pa = s.axis == 0 ? x[0] : (s.axis == 1 ? x[1] : x[2]);
    if (s.flip ? pa > s.fh : pa < s.fh) {
      const float v = s.cf * s.fvol[p], t = pa - s.fh, v2 = 2.0f * v;
      e = fmaf(v * t, t, e);
#pragma unroll
      for (int b = 0; b < 3; ++b)
        if (b == s.axis) f[b] = fmaf(v2, t, f[b]), d[b] = v2;
    }
  }
  if (s.mass != nullptr) {
    const float m = s.mass[p];
    e = fmaf(0.5f * m, sf_dot(u, u), e);
#pragma unroll
    for (int b = 0; b < 3; ++b) f[b] = fmaf(m, u[b], f[b]), d[b] = d[b] + m;
  }
  return e;
}
// e += the energy of a pin of coefficient c at y on a point at x; f, d likewise
__device__ __forceinline__ void sf_pin(float c, const float* x, const float* y, float& e, float* f, float* d) {
  const float r[3] = {x[0] - y[0], x[1] - y[1], x[2] - y[2]}, c2 = 2.0f * c;
  e = fmaf(c, sf_dot(r, r), e);
#pragma unroll
  for (int b = 0; b < 3; ++b) f[b] = fmaf(c2, r[b], f[b]), d[b] = d[b] + c2;
}

// ---- 1. the terms of one class on given dx ----------------------------------------------------------------------------------------------
struct SfPins {
  int64_t P;
  const int *sorted, *order;   // the pins' points, ascending, and each one's place in the list; sorted == nullptr: the terms of SfScene
  const float* y;              // (P, 3), in list order
  float c;
};

// MODE 0: energy partials, 1: gradient (N, 3), 2: Hessian (N, 3, 3)
template <int MODE>
__global__ __launch_bounds__(RA_THREADS) void sf_terms_kernel(const SfScene s, const SfPins k, const float* __restrict__ dx,
                                                              float* __restrict__ out) {
  float e_acc = 0.0f, e_comp = 0.0f;
  for (int64_t p = (int64_t)blockIdx.x * RA_THREADS + threadIdx.x; p < s.N; p += (int64_t)gridDim.x * RA_THREADS) {
    const float x[3] = {s.x0[p * 3] + dx[p * 3], s.x0[p * 3 + 1] + dx[p * 3 + 1], s.x0[p * 3 + 2] + dx[p * 3 + 2]};
    const float u[3] = {0.0f, 0.0f, 0.0f};
    float e = 0.0f, f[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
    if (k.sorted != nullptr) {
      int64_t lo = 0, hi = k.P;   // the first pin of a point >= p
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (k.sorted[mid] < p) lo = mid + 1; else hi = mid;
      }
      for (; lo < k.P && k.sorted[lo] == p; ++lo) {
        const int j = k.order[lo];
        if (j < 0 || j >= k.P) continue;
        const float y[3] = {k.y[(int64_t)j * 3], k.y[(int64_t)j * 3 + 1], k.y[(int64_t)j * 3 + 2]};
        sf_pin(k.c, x, y, e, f, d);
      }
    } else {
      e = sf_point(s, p, x, u, f, d);
    }
    if (MODE == 0) ra_add(e_acc, e_comp, e);
    if (MODE == 1) {
#pragma unroll
      for (int b = 0; b < 3; ++b) out[p * 3 + b] = f[b];
    }
    if (MODE == 2) {
#pragma unroll
      for (int j = 0; j < 9; ++j) out[p * 9 + j] = (j % 4 == 0) ? d[j / 4] : 0.0f;
    }
  }
  if (MODE == 0) ra_block_energy(e_acc, out);
}

// ---- 2. the reduced terms ---------------------------------------------------------------------------------------------------------------
struct SfArgs {
  SfScene s;
  int64_t P, per;                  // pins, rows per slice
  const int* pin_idx;              // (P)
  const float *pin_y, *pin_c;      // (P, 3), (P)
  const float *z, *zp, *zd, *w;    // (12 H) each (zp == nullptr: no inertia), (N, H)
  float dt;
  int H, W;                        // handles, 4 H
  RaPartials part;                 // K's blocks: the axes
};

// m of the chunk's row q at column col (0 past W and for a row past the slice or without a point)
__device__ __forceinline__ float sf_m(const SfArgs& a, const int* s_p, const float* s_x, int q, int col) {
  const int p = s_p[q];
  if (col >= a.W || p < 0) return 0.0f;
  return a.w[(int64_t)p * a.H + (col >> 2)] * s_x[q * 4 + (col & 3)];
}

template <bool HESS>
__global__ __launch_bounds__(RA_THREADS) void sf_reduced_kernel(const SfArgs a) {
  __shared__ float s_MI[SF_CR * RA_LS], s_MJ[HESS ? SF_CR * RA_LS : 1];
  __shared__ float s_z[12 * RA_MAX_H], s_dl[12 * RA_MAX_H];
  __shared__ float s_f[SF_CR * 3], s_d[SF_CR * 3], s_x[SF_CR * 4], s_e[SF_PASS];
  __shared__ int s_p[SF_CR];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t slice = blockIdx.x;
  int ti = (int)blockIdx.y, tj = 0;
  if (HESS) ra_lower_tile((int)blockIdx.y, ti, tj);
  const int i0 = ti * RA_TILE, j0 = tj * RA_TILE, H = a.H, W = a.W;
  const bool diag = ti == tj, sums_g = tj == 0, sums_e = ti == 0 && tj == 0, inertia = a.zp != nullptr;
  const float* MJ = diag ? s_MI : s_MJ;
  const int64_t N = a.s.N, rows = N + a.P;
  const int64_t begin = slice * a.per, end = begin + a.per < rows ? begin + a.per : rows;
  for (int e = t; e < 12 * H; e += RA_THREADS) {
    const float zv = a.z[e];
    s_z[e] = zv;
    s_dl[e] = inertia ? (zv - a.zp[e]) - a.dt * a.zd[e] : 0.0f;
  }
  ra_f32x4 acc[3][4];
#pragma unroll
  for (int b = 0; b < 3; ++b)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[b][cb] = ra_f32x4{0.f, 0.f, 0.f, 0.f};
  float g_acc = 0.0f, g_comp = 0.0f, e_acc = 0.0f, e_comp = 0.0f;
  const int pl = t / SF_TPR, sub = t % SF_TPR;

  for (int64_t c0 = begin; c0 < end; c0 += SF_CR) {
    __syncthreads();  // z and delta are staged; the previous chunk's images and terms are no longer read
    // (b) the rows of the chunk
#pragma unroll 1
    for (int q = pl; q < SF_CR; q += SF_PASS) {
      const int64_t r = c0 + q;
      int64_t p = -1;
      if (r < end) {
        p = r;
        if (r >= N) {
          p = a.pin_idx[r - N];
          if (p < 0 || p >= N) p = -1;
        }
      }
      float xr[3] = {0.0f, 0.0f, 0.0f}, dx[3] = {0.0f, 0.0f, 0.0f}, u[3] = {0.0f, 0.0f, 0.0f};
      if (p >= 0) {
#pragma unroll
        for (int b = 0; b < 3; ++b) xr[b] = a.s.x0[p * 3 + b];
        const float* wp = a.w + p * H;
        for (int h = sub; h < H; h += SF_TPR) {
          const float w = wp[h];
          const float *zh = s_z + h * 12, *dh = s_dl + h * 12;
#pragma unroll
          for (int b = 0; b < 3; ++b) {
            dx[b] = fmaf(w, fmaf(zh[b * 4], xr[0], fmaf(zh[b * 4 + 1], xr[1], fmaf(zh[b * 4 + 2], xr[2], zh[b * 4 + 3]))), dx[b]);
            if (inertia)
              u[b] = fmaf(w, fmaf(dh[b * 4], xr[0], fmaf(dh[b * 4 + 1], xr[1], fmaf(dh[b * 4 + 2], xr[2], dh[b * 4 + 3]))), u[b]);
          }
        }
      }
#pragma unroll
      for (int m = 1; m < SF_TPR; m <<= 1)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          dx[b] = dx[b] + __shfl_xor(dx[b], m);
          if (inertia) u[b] = u[b] + __shfl_xor(u[b], m);
        }
      if (sub == 0) {
        float e = 0.0f, f[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
        if (p >= 0) {
          const float x[3] = {xr[0] + dx[0], xr[1] + dx[1], xr[2] + dx[2]};
          if (r < N) {
            e = sf_point(a.s, p, x, u, f, d);
          } else {
            const int64_t k = r - N;
            const float y[3] = {a.pin_y[k * 3], a.pin_y[k * 3 + 1], a.pin_y[k * 3 + 2]};
            sf_pin(a.pin_c[k], x, y, e, f, d);
          }
        }
#pragma unroll
        for (int b = 0; b < 3; ++b) s_f[q * 3 + b] = f[b], s_d[q * 3 + b] = d[b], s_x[q * 4 + b] = xr[b];
        s_x[q * 4 + 3] = 1.0f;
        s_p[q] = (int)p;
        if (sums_e) ra_add(e_acc, e_comp, e);
      }
    }
    __syncthreads();
    // (c) the images of m
    for (int e = t; e < SF_CR * RA_TILE; e += RA_THREADS) {
      const int q = e >> 6, col = e & 63;
      s_MI[q * RA_LS + col] = sf_m(a, s_p, s_x, q, i0 + col);
      if (HESS && !diag) s_MJ[q * RA_LS + col] = sf_m(a, s_p, s_x, q, j0 + col);
    }
    __syncthreads();
    if (sums_g && t < 3 * RA_TILE) {
      const int b = t >> 6;  // per row, then the chunk's rows pairwise, then onto the running sum with its error carried
      float v[SF_CR];
#pragma unroll
      for (int q = 0; q < SF_CR; ++q) v[q] = s_f[q * 3 + b] * s_MI[q * RA_LS + lane];
      ra_add(g_acc, g_comp, ra_pairwise(v));
    }
    // (d) lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], D[row 4 (l >> 4) + reg][col l & 15]
    if (HESS && i0 + wave * 16 < W) {
      const int kq = lane >> 4, rr = lane & 15;
      for (int d = 0; d < SF_CR; d += 4) {
        const float av = s_MI[(d + kq) * RA_LS + wave * 16 + rr];
        float as[3];
#pragma unroll
        for (int b = 0; b < 3; ++b) as[b] = av * s_d[(d + kq) * 3 + b];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
          if (j0 + cb * 16 < W && (!diag || cb <= wave)) {
            const float bv = MJ[(d + kq) * RA_LS + cb * 16 + rr];
#pragma unroll
            for (int b = 0; b < 3; ++b) acc[b][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[b], bv, acc[b][cb], 0, 0, 0);
          }
      }
    }
  }

  if (HESS) {
    ra_store_blocks(acc, a.part.Kp, slice, W, i0, j0, wave, lane, diag);
  }
  if (sums_g && t < 3 * RA_TILE && i0 + lane < W) a.part.gp[((size_t)slice * 3 + (t >> 6)) * W + i0 + lane] = g_acc;
  if (sums_e) ra_slice_energy<SF_PASS>(e_acc, sub == 0, pl, s_e, a.part.ep + slice);
}

inline int64_t sf_slice_rows(int64_t rows, int H) { return ra_slice_len(rows, ra_tri(ra_tiles(H)), SF_CR, SF_MAX_SLICES); }
inline SfScene sf_scene(int64_t N, const float* x0, const float* rho, const float* gvol, float gx, float gy, float gz, float cg,
                        const float* fvol, float fh, int axis, int flip, float cf, const float* mass) {
  SfScene s;
  s.N = N, s.x0 = x0, s.rho = rho, s.gvol = gvol, s.g[0] = gx, s.g[1] = gy, s.g[2] = gz, s.cg = cg;
  s.fvol = fvol, s.fh = fh, s.cf = cf, s.axis = axis, s.flip = flip != 0, s.mass = mass;
  return s;
}

}  // namespace

extern "C" {

size_t kamd_scene_terms_workspace(int64_t N) { return N > 0 ? kamd_align16((size_t)ra_term_blocks(N, RA_THREADS) * sizeof(float)) : 0; }

int kamd_scene_terms_f32(void* stream, int64_t N, const float* dx, const float* x0, const float* rho, const float* gvol, float gx,
                         float gy, float gz, const float* fvol, float floor_height, int floor_axis, int flip_floor, int64_t P,
                         const int* pins_sorted, const int* pins_order, const float* pinned_x, float coeff, float* energy,
                         float* gradient, float* hessian, void* workspace) {
  if (N < 0 || N > 0x7FFFFFFFLL || P < 0 || P > 0x7FFFFFFFLL) return (int)hipErrorInvalidValue;
  if (N == 0 || (energy == nullptr && gradient == nullptr && hessian == nullptr)) return 0;
  const int classes = (rho != nullptr) + (fvol != nullptr) + (pins_sorted != nullptr);
  if (dx == nullptr || x0 == nullptr || classes != 1 || (rho != nullptr && gvol == nullptr) ||
      (fvol != nullptr && (floor_axis < 0 || floor_axis > 2)) ||
      (pins_sorted != nullptr && (pins_order == nullptr || pinned_x == nullptr || P < 1)) || (energy != nullptr && workspace == nullptr))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const SfScene s = sf_scene(N, x0, rho, gvol, gx, gy, gz, coeff, fvol, floor_height, floor_axis, flip_floor, coeff, nullptr);
  SfPins k;
  k.P = P, k.sorted = pins_sorted, k.order = pins_order, k.y = pinned_x, k.c = coeff;
  const int blocks = ra_term_blocks(N, RA_THREADS);
  if (energy != nullptr) {
    hipLaunchKernelGGL(sf_terms_kernel<0>, dim3((unsigned)blocks), dim3(RA_THREADS), 0, st, s, k, dx, (float*)workspace);
    hipLaunchKernelGGL(ra_sum_kernel, dim3(1), dim3(KAMD_WAVE), 0, st, blocks, (const float*)workspace, energy);
  }
  if (gradient != nullptr) hipLaunchKernelGGL(sf_terms_kernel<1>, dim3((unsigned)blocks), dim3(RA_THREADS), 0, st, s, k, dx, gradient);
  if (hessian != nullptr) hipLaunchKernelGGL(sf_terms_kernel<2>, dim3((unsigned)blocks), dim3(RA_THREADS), 0, st, s, k, dx, hessian);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_scene_chunk_rows(void) { return SF_CR; }
int64_t kamd_scene_slice_rows(int64_t rows, int H) { return ra_sizes_ok(rows, H) ? sf_slice_rows(rows, H) : 0; }

size_t kamd_scene_reduced_workspace(int64_t rows, int H, int hessian) {
  if (!ra_sizes_ok(rows, H) || rows == 0) return 0;
  return ra_workspace(ra_slices(rows, sf_slice_rows(rows, H)), RaDiagonalThree::BLOCKS, H, hessian);
}

int kamd_scene_reduced_f32(void* stream, int64_t N, int64_t P, int H, const float* z, const float* x0, const float* weights,
                           const float* rho, const float* gvol, float gx, float gy, float gz, float gravity_coeff, const float* fvol,
                           float floor_height, int floor_axis, int flip_floor, float floor_coeff, const int* pinned_indices,
                           const float* pinned_x, const float* pinned_coeff, const float* mass, const float* z_prev,
                           const float* z_dot, float dt, int hessian, float* E, float* g, float* K, void* workspace,
                           size_t workspace_bytes) {
  if (N < 0 || P < 0 || N > 0x7FFFFFFFLL || P > 0x7FFFFFFFLL || !ra_sizes_ok(N + P, H) || N + P == 0)
    return (int)hipErrorInvalidValue;
  if (z == nullptr || x0 == nullptr || weights == nullptr || (rho != nullptr && gvol == nullptr) ||
      (fvol != nullptr && (floor_axis < 0 || floor_axis > 2)) ||
      (P > 0 && (pinned_indices == nullptr || pinned_x == nullptr || pinned_coeff == nullptr)) ||
      (mass != nullptr && (z_prev == nullptr || z_dot == nullptr)) || E == nullptr || g == nullptr || (hessian && K == nullptr) ||
      workspace == nullptr || workspace_bytes < kamd_scene_reduced_workspace(N + P, H, hessian))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  SfArgs a;
  a.s = sf_scene(N, x0, rho, gvol, gx, gy, gz, gravity_coeff, fvol, floor_height, floor_axis, flip_floor, floor_coeff, mass);
  a.P = P, a.per = sf_slice_rows(N + P, H), a.pin_idx = pinned_indices, a.pin_y = pinned_x, a.pin_c = pinned_coeff;
  a.z = z, a.zp = mass != nullptr ? z_prev : nullptr, a.zd = z_dot, a.w = weights, a.dt = dt, a.H = H, a.W = 4 * H;
  const size_t S = ra_slices(N + P, a.per);
  ra_workspace(S, RaDiagonalThree::BLOCKS, H, hessian, workspace, &a.part);
  const int T = ra_tiles(H);
  if (hessian)
    hipLaunchKernelGGL(sf_reduced_kernel<true>, dim3((unsigned)S, (unsigned)ra_tri(T)), dim3(RA_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL(sf_reduced_kernel<false>, dim3((unsigned)S, (unsigned)T), dim3(RA_THREADS), 0, st, a);
  return ra_finish<RaDiagonalThree>(st, S, H, a.part, hessian ? K : nullptr, g, E);
}
}
