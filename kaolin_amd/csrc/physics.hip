// kaolin.physics on the GPU: the Neo-Hookean material and the reduced (Simplicits) energy, gradient and Hessian.  The reference runs
// NVIDIA Warp kernels (kaolin/physics/materials/neohookean_elastic_material.py) and reduces the Hessian with a dense (9N, 12H)
// dFdz, N 9x9 blocks in memory, torch.bmm and torch.matmul (physics/utils/torch_utilities.py: hess_reduction); float32 only.
//
// THE TERMS, per point, F row-major (vec F index 3 b + m), J = det F, C = cof F = dJ/dF (2x2 minors, never inverse(F): finite
// for a singular or inverted F), a = lam (J - 1) - mu, s = vol * coeff:
//   Psi = mu / 2 (|F|^2 - 3) + lam / 2 (J - 1)^2 - mu (J - 1)       |F|^2 - 3 is summed as |F - I|^2 + 2 tr(F - I)
//   P   = mu F + a C
//   H   = mu I9 + lam vec(C) vec(C)^T + a dC/dF,   dC/dF[(i,j),(k,l)] = eps(i,k,x) eps(j,l,y) F[x][y]  (zero where i == k or j == l)
// all scaled by s.  -ffp-contract=off: every fused multiply-add below is spelled.
//
// 1. ph_material_kernel: the terms on given F.  One wavefront per workgroup, one lane per point, grid-stride.  The 9 gradient
//    and 81 Hessian values of the wavefront's 64 points go through an LDS image [point][81] (stride 81: lanes on distinct banks)
//    and leave as one contiguous run of dwords.  The energy stays in the lane over the stride loop, is added over the wavefront
//    by a butterfly, and one launch of one thread adds the <= 1024 workgroup partials in index order: no atomics, same bits
//    every run.
//
// 2. ph_reduced_kernel: with W = 4 H and Mcat_p the 3 x W matrix of all handles' M_{p,h} = grad w_{p,h} (x) (x, y, z, 1) + w_{p,h} [I3 | 0]
//    side by side, dFdz's block of point p is I3 (x) Mcat_p, so
//      F_p[b][m]   = delta + sum_i Mcat_p[m][i] z[h(i)][b][n(i)]
//      g[h][b][n]  = sum_p sum_m P_p[b][m] Mcat_p[m][4 h + n]
//      K_bb'[i][j] = sum_p sum_m (Mcat_p[m][i] * sum_m' H_p[(b,m),(b',m')] Mcat_p[m'][j])     nine W x W GEMMs of depth 3 N
//    and K[(h,b,n),(h',b',n')] = K_bb'[4 h + n][4 h' + n'].  K_b'b = K_bb'^T: the six pairs b' <= b are computed, and of the
//    three b == b' only the tiles on and under the diagonal.
//    The grid, the sums of g and E, the slices' partials and their finish are those of reduced_assembly.h; the partials hold the
//    six blocks of RaSymmetricSix.  The workgroup strides over its slice in chunks of PC = 16 points (depth 48).  Per chunk:
//      (a) z is in LDS (12 H floats, staged once).  16 lanes per point accumulate F_p over the handles h = lane, lane + 16, ...
//          and add up by a butterfly inside their row of 16; the first lane forms C, J, P (and Psi) and leaves F, C, P and
//          (mu s, lam s, a s) in LDS
//      (b) all threads build the two Mcat images in LDS, rows (point, m) x 64 columns of the row tile and of the column tile
//          (zeros for columns past W and points past the slice), and the 81 entries of every H_p from F and C
//      (c) for a pair (b, b'): R[(p, m)][j] = sum_m' H_p[(b,m),(b',m')] Mcat_p[m'][j] -> LDS
//      (d) acc[pair] += McatI^T R: 6 pairs x 4 blocks x 4 = 96 accumulator registers.  Row and column blocks past W are skipped.
//      g: P_p Mcat_p of the row tile; E: Psi, in the points' first lanes.
//    LDS: 3 images of 48 x 80 floats (45 KiB) + H_p 5 KiB + F, C, P, x 2.2 KiB + z 48 H bytes: H <= 128 keeps it under 64 KiB.
#include "reduced_assembly.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr int PH_PC = 16;                      // points per chunk
constexpr int PH_TPP = RA_THREADS / PH_PC;     // lanes per point in stage (a)
constexpr int PH_DEPTH = 3 * PH_PC;            // GEMM depth of a chunk
constexpr int PH_MAX_SLICES = 64;
constexpr int PH_PAIRS = RaSymmetricSix::BLOCKS;
__device__ constexpr int PH_B[PH_PAIRS] = {0, 1, 1, 2, 2, 2}, PH_BP[PH_PAIRS] = {0, 0, 1, 0, 1, 2};

// C = cof F: its rows are the cross products of F's other two rows; returns J = det F
__device__ __forceinline__ float ph_cofactor(const float* F, float* C) {
  C[0] = fmaf(F[4], F[8], -(F[5] * F[7]));
  C[1] = fmaf(F[5], F[6], -(F[3] * F[8]));
  C[2] = fmaf(F[3], F[7], -(F[4] * F[6]));
  C[3] = fmaf(F[7], F[2], -(F[8] * F[1]));
  C[4] = fmaf(F[8], F[0], -(F[6] * F[2]));
  C[5] = fmaf(F[6], F[1], -(F[7] * F[0]));
  C[6] = fmaf(F[1], F[5], -(F[2] * F[4]));
  C[7] = fmaf(F[2], F[3], -(F[0] * F[5]));
  C[8] = fmaf(F[0], F[4], -(F[1] * F[3]));
  return fmaf(F[0], C[0], fmaf(F[1], C[1], F[2] * C[2]));
}
// Psi; mu, lam already scaled by s
__device__ __forceinline__ float ph_energy(const float* F, float J, float mu, float lam) {
  float q = 0.0f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float d = (k % 4 == 0) ? F[k] - 1.0f : F[k];
    q = fmaf(d, d, q);
  }
  const float tr = ((F[0] - 1.0f) + (F[4] - 1.0f)) + (F[8] - 1.0f);
  const float i1m3 = fmaf(2.0f, tr, q), jm1 = J - 1.0f;
  return fmaf(0.5f * mu, i1m3, fmaf(0.5f * lam * jm1, jm1, -(mu * jm1)));
}
// entry (r, c) of H; mu, lam, a already scaled by s
__device__ __forceinline__ float ph_hess_entry(const float* F, const float* C, float mu, float lam, float a, int r, int c) {
  const int i = r / 3, j = r % 3, k = c / 3, l = c % 3;
  float v = (lam * C[r]) * C[c];
  if (r == c) v = v + mu;
  if (i != k && j != l) {
    const float f = F[(3 - i - k) * 3 + (3 - j - l)];
    const bool positive = (k == (i + 1) % 3) == (l == (j + 1) % 3);
    v = fmaf(positive ? a : -a, f, v);
  }
  return v;
}

// ---- 1. the material on given F ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KAMD_WAVE) void ph_material_kernel(int64_t N, const float* __restrict__ Fs, const float* __restrict__ mus,
                                                                const float* __restrict__ lams, const float* __restrict__ vols,
                                                                float coeff, float* __restrict__ partial, float* __restrict__ grad,
                                                                float* __restrict__ hess) {
  __shared__ float s_out[KAMD_WAVE * 81];
  const int lane = threadIdx.x;
  float e_acc = 0.0f, e_comp = 0.0f;
  for (int64_t base = (int64_t)blockIdx.x * KAMD_WAVE; base < N; base += (int64_t)gridDim.x * KAMD_WAVE) {
    const int64_t p = base + lane;
    const int count = (int)(N - base < KAMD_WAVE ? N - base : KAMD_WAVE);
    float F[9], C[9], mu = 0.0f, lam = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = (k % 4 == 0) ? 1.0f : 0.0f;
    if (p < N) {
#pragma unroll
      for (int k = 0; k < 9; ++k) F[k] = Fs[p * 9 + k];
      const float s = vols[p] * coeff;
      mu = mus[p] * s, lam = lams[p] * s;
    }
    const float J = ph_cofactor(F, C);
    const float a = fmaf(lam, J - 1.0f, -mu);
    if (partial != nullptr) ra_add(e_acc, e_comp, ph_energy(F, J, mu, lam));
    if (grad != nullptr) {
#pragma unroll
      for (int k = 0; k < 9; ++k) s_out[lane * 9 + k] = fmaf(mu, F[k], a * C[k]);
      __syncthreads();
      for (int e = lane; e < count * 9; e += KAMD_WAVE) grad[base * 9 + e] = s_out[e];
      __syncthreads();
    }
    if (hess != nullptr) {
#pragma unroll
      for (int r = 0; r < 9; ++r)
#pragma unroll
        for (int c = 0; c < 9; ++c) s_out[lane * 81 + r * 9 + c] = ph_hess_entry(F, C, mu, lam, a, r, c);
      __syncthreads();
      for (int e = lane; e < count * 81; e += KAMD_WAVE) hess[base * 81 + e] = s_out[e];
      __syncthreads();
    }
  }
  if (partial != nullptr) {
    e_acc = ra_wave_sum(e_acc);
    if (lane == 0) partial[blockIdx.x] = e_acc;
  }
}

// ---- 2. the reduced terms ---------------------------------------------------------------------------------------------------------------
struct PhArgs {
  const float *z, *pts, *w, *wj, *mu, *lam, *vol;
  float coeff;
  int64_t N, per;   // points, points per slice
  int H, W, T;      // handles, 4 H, tiles per side
  RaPartials part;  // K's blocks: the pairs
};

// Mcat_p[m][col] (0 past W or for a point past the slice); xs = (x, y, z, 1) of the point
__device__ __forceinline__ float ph_mcat(const PhArgs& a, int64_t p, bool ok, int m, int col, const float* xs) {
  if (!ok || col >= a.W) return 0.0f;
  const int h = col >> 2, n = col & 3;
  const float g = a.wj[(p * a.H + h) * 3 + m];
  return m == n ? fmaf(g, xs[n], a.w[p * a.H + h]) : g * xs[n];
}

template <bool HESS>
__global__ __launch_bounds__(RA_THREADS) void ph_reduced_kernel(const PhArgs a) {
  __shared__ float s_MI[PH_DEPTH * RA_LS], s_MJ[PH_DEPTH * RA_LS], s_R[PH_DEPTH * RA_LS];
  __shared__ float s_H[PH_PC * 81];
  __shared__ float s_z[12 * RA_MAX_H];
  __shared__ float s_F[PH_PC * 9], s_C[PH_PC * 9], s_P[PH_PC * 9], s_par[PH_PC * 4], s_x[PH_PC * 4], s_e[PH_PC];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t slice = blockIdx.x;
  const int ti = HESS ? (int)blockIdx.y / a.T : (int)blockIdx.y, tj = HESS ? (int)blockIdx.y % a.T : 0;
  const int i0 = ti * RA_TILE, j0 = tj * RA_TILE, H = a.H, W = a.W;
  const bool low = ti >= tj;              // on or under the diagonal: computes the three b == b' pairs too
  const bool sums_g = tj == 0, sums_e = ti == 0 && tj == 0;
  const float* MJ = (ti == tj) ? s_MI : s_MJ;
  for (int e = t; e < 12 * H; e += RA_THREADS) s_z[e] = a.z[e];
  const int64_t begin = slice * a.per, end = begin + a.per < a.N ? begin + a.per : a.N;
  ra_f32x4 acc[PH_PAIRS][4];
#pragma unroll
  for (int pr = 0; pr < PH_PAIRS; ++pr)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[pr][cb] = ra_f32x4{0.f, 0.f, 0.f, 0.f};
  float g_acc = 0.0f, g_comp = 0.0f, e_acc = 0.0f, e_comp = 0.0f;
  const int pl = t / PH_TPP, sub = t % PH_TPP;

  for (int64_t c0 = begin; c0 < end; c0 += PH_PC) {
    __syncthreads();  // z is staged; the previous chunk's images are no longer read
    // (a) F - I of point c0 + pl, over the handles sub, sub + 16, ...
    const int64_t p = c0 + pl;
    const bool valid = p < end;
    float F[9], x0 = 0.0f, x1 = 0.0f, x2 = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = 0.0f;
    if (valid) {
      x0 = a.pts[p * 3], x1 = a.pts[p * 3 + 1], x2 = a.pts[p * 3 + 2];
      const float* wp = a.w + p * H;
      const float* jp = a.wj + p * H * 3;
      for (int h = sub; h < H; h += PH_TPP) {
        const float w = wp[h], g0 = jp[h * 3], g1 = jp[h * 3 + 1], g2 = jp[h * 3 + 2];
        const float* zh = s_z + h * 12;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const float u = fmaf(zh[b * 4], x0, fmaf(zh[b * 4 + 1], x1, fmaf(zh[b * 4 + 2], x2, zh[b * 4 + 3])));
          F[b * 3] = fmaf(w, zh[b * 4], fmaf(u, g0, F[b * 3]));
          F[b * 3 + 1] = fmaf(w, zh[b * 4 + 1], fmaf(u, g1, F[b * 3 + 1]));
          F[b * 3 + 2] = fmaf(w, zh[b * 4 + 2], fmaf(u, g2, F[b * 3 + 2]));
        }
      }
    }
#pragma unroll
    for (int m = 1; m < PH_TPP; m <<= 1)
#pragma unroll
      for (int k = 0; k < 9; ++k) F[k] = F[k] + __shfl_xor(F[k], m);
    if (sub == 0) {
      float C[9], mu = 0.0f, lam = 0.0f;
      if (valid) {
        const float s = a.vol[p] * a.coeff;
        mu = a.mu[p] * s, lam = a.lam[p] * s;
      }
      F[0] = F[0] + 1.0f, F[4] = F[4] + 1.0f, F[8] = F[8] + 1.0f;
      const float J = ph_cofactor(F, C);
      const float as = fmaf(lam, J - 1.0f, -mu);
#pragma unroll
      for (int k = 0; k < 9; ++k) s_F[pl * 9 + k] = F[k], s_C[pl * 9 + k] = C[k], s_P[pl * 9 + k] = fmaf(mu, F[k], as * C[k]);
      s_par[pl * 4] = mu, s_par[pl * 4 + 1] = lam, s_par[pl * 4 + 2] = as;
      s_x[pl * 4] = x0, s_x[pl * 4 + 1] = x1, s_x[pl * 4 + 2] = x2, s_x[pl * 4 + 3] = 1.0f;
      if (sums_e) ra_add(e_acc, e_comp, ph_energy(F, J, mu, lam));
    }
    __syncthreads();
    // (b) the Mcat images and the Hessian blocks
    for (int e = t; e < PH_DEPTH * RA_TILE; e += RA_THREADS) {
      const int d = e >> 6, c = e & 63, q = d / 3, m = d - q * 3;
      const bool ok = c0 + q < end;
      s_MI[d * RA_LS + c] = ph_mcat(a, c0 + q, ok, m, i0 + c, s_x + q * 4);
      if (HESS && ti != tj) s_MJ[d * RA_LS + c] = ph_mcat(a, c0 + q, ok, m, j0 + c, s_x + q * 4);
    }
    if (HESS) {
      for (int e = t; e < PH_PC * 81; e += RA_THREADS) {
        const int q = e / 81, rc = e - q * 81;
        s_H[e] = ph_hess_entry(s_F + q * 9, s_C + q * 9, s_par[q * 4], s_par[q * 4 + 1], s_par[q * 4 + 2], rc / 9, rc % 9);
      }
    }
    __syncthreads();
    if (sums_g && t < 3 * RA_TILE) {
      const int b = t >> 6;  // per point, then the chunk's points pairwise, then onto the running sum with its error carried
      float v[PH_PC];
#pragma unroll
      for (int q = 0; q < PH_PC; ++q) {
        const float* Pq = s_P + q * 9 + b * 3;
        const float* Mq = s_MI + q * 3 * RA_LS + lane;
        v[q] = fmaf(Pq[0], Mq[0], fmaf(Pq[1], Mq[RA_LS], Pq[2] * Mq[2 * RA_LS]));
      }
      ra_add(g_acc, g_comp, ra_pairwise(v));
    }
    if (HESS) {
#pragma unroll
      for (int pr = 0; pr < PH_PAIRS; ++pr) {
        if (PH_B[pr] == PH_BP[pr] && !low) continue;
        // (c) R = H_p^{bb'} Mcat_p, column `lane`, points wave, wave + 4, ...
        for (int q = wave; q < PH_PC; q += RA_THREADS / KAMD_WAVE) {
          const float m0 = MJ[(q * 3) * RA_LS + lane], m1 = MJ[(q * 3 + 1) * RA_LS + lane], m2 = MJ[(q * 3 + 2) * RA_LS + lane];
          const float* Hq = s_H + q * 81 + PH_B[pr] * 27 + PH_BP[pr] * 3;
#pragma unroll
          for (int m = 0; m < 3; ++m)
            s_R[(q * 3 + m) * RA_LS + lane] = fmaf(Hq[m * 9], m0, fmaf(Hq[m * 9 + 1], m1, Hq[m * 9 + 2] * m2));
        }
        __syncthreads();
        // (d) lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], D[row 4 (l >> 4) + reg][col l & 15]
        if (i0 + wave * 16 < W) {
          const int kq = lane >> 4, r = lane & 15;
          for (int d = 0; d < PH_DEPTH; d += 4) {
            const float av = s_MI[(d + kq) * RA_LS + wave * 16 + r];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
              if (j0 + cb * 16 < W)
                acc[pr][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, s_R[(d + kq) * RA_LS + cb * 16 + r], acc[pr][cb], 0, 0, 0);
          }
        }
        __syncthreads();
      }
    }
  }

  if (HESS) {
#pragma unroll
    for (int pr = 0; pr < PH_PAIRS; ++pr) {
      if (PH_B[pr] == PH_BP[pr] && !low) continue;
      float* P = a.part.Kp + ((size_t)slice * PH_PAIRS + pr) * (size_t)W * W;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = i0 + wave * 16 + (lane >> 4) * 4 + j, col = j0 + cb * 16 + (lane & 15);
          if (row < W && col < W) P[(size_t)row * W + col] = acc[pr][cb][j];
        }
    }
  }
  if (sums_g && t < 3 * RA_TILE && i0 + lane < W) a.part.gp[((size_t)slice * 3 + (t >> 6)) * W + i0 + lane] = g_acc;
  if (sums_e) ra_slice_energy<PH_PC>(e_acc, sub == 0, pl, s_e, a.part.ep + slice);
}

inline int64_t ph_slice_points(int64_t N, int H) { return ra_slice_len(N, ra_tiles(H) * ra_tiles(H), PH_PC, PH_MAX_SLICES); }

}  // namespace

extern "C" {

size_t kamd_physics_neohookean_workspace(int64_t N) {
  return N > 0 ? kamd_align16((size_t)ra_term_blocks(N, KAMD_WAVE) * sizeof(float)) : 0;
}

int kamd_physics_neohookean_f32(void* stream, int64_t N, const float* defo_grads, const float* mu, const float* lam, const float* vol,
                                float coeff, float* energy, float* gradient, float* hessian, void* workspace) {
  if (N < 0) return (int)hipErrorInvalidValue;
  if (N == 0 || (energy == nullptr && gradient == nullptr && hessian == nullptr)) return 0;
  if (defo_grads == nullptr || mu == nullptr || lam == nullptr || vol == nullptr || (energy != nullptr && workspace == nullptr))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = ra_term_blocks(N, KAMD_WAVE);
  float* partial = energy != nullptr ? (float*)workspace : nullptr;
  hipLaunchKernelGGL(ph_material_kernel, dim3((unsigned)blocks), dim3(KAMD_WAVE), 0, st, N, defo_grads, mu, lam, vol, coeff, partial,
                     gradient, hessian);
  if (energy != nullptr) hipLaunchKernelGGL(ra_sum_kernel, dim3(1), dim3(KAMD_WAVE), 0, st, blocks, (const float*)partial, energy);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_physics_chunk_points(void) { return PH_PC; }
int kamd_physics_max_handles(void) { return RA_MAX_H; }
int64_t kamd_physics_slice_points(int64_t N, int H) { return ra_sizes_ok(N, H) ? ph_slice_points(N, H) : 0; }

size_t kamd_physics_reduced_workspace(int64_t N, int H, int hessian) {
  if (!ra_sizes_ok(N, H) || N == 0) return 0;
  return ra_workspace(ra_slices(N, ph_slice_points(N, H)), PH_PAIRS, H, hessian);
}

int kamd_physics_reduced_neohookean_f32(void* stream, int64_t N, int H, const float* z, const float* pts, const float* weights,
                                        const float* weights_jac, const float* mu, const float* lam, const float* vol, float coeff,
                                        int hessian, float* E, float* g, float* K, void* workspace, size_t workspace_bytes) {
  if (!ra_sizes_ok(N, H) || N == 0) return (int)hipErrorInvalidValue;
  if (z == nullptr || pts == nullptr || weights == nullptr || weights_jac == nullptr || mu == nullptr || lam == nullptr ||
      vol == nullptr || E == nullptr || g == nullptr || (hessian && K == nullptr) || workspace == nullptr ||
      workspace_bytes < kamd_physics_reduced_workspace(N, H, hessian))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  PhArgs a;
  a.z = z, a.pts = pts, a.w = weights, a.wj = weights_jac, a.mu = mu, a.lam = lam, a.vol = vol, a.coeff = coeff;
  a.N = N, a.per = ph_slice_points(N, H), a.H = H, a.W = 4 * H, a.T = ra_tiles(H);
  const size_t S = ra_slices(N, a.per);
  ra_workspace(S, PH_PAIRS, H, hessian, workspace, &a.part);
  if (hessian)
    hipLaunchKernelGGL(ph_reduced_kernel<true>, dim3((unsigned)S, (unsigned)(a.T * a.T)), dim3(RA_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL(ph_reduced_kernel<false>, dim3((unsigned)S, (unsigned)a.T), dim3(RA_THREADS), 0, st, a);
  return ra_finish<RaSymmetricSix>(st, S, H, a.part, hessian ? K : nullptr, g, E);
}
}
