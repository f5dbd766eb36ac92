// kaolin.physics.common.collisions on the GPU: contact detection between points, the per-contact barrier / friction terms and their
// reduction to the Simplicits degrees of freedom.  The reference runs NVIDIA Warp kernels (kaolin/physics/common/collisions.py): a
// hash grid query whose contact order is an atomic counter's, and a Hessian reduction through a dense (3 C, 12 H) Jacobian.
// float32 only.  -ffp-contract=off and no packed float32 instructions: every operation below rounds once, in the order written.
//
// 1. DETECTION.  pos = x0 + dx; a pair a < b is a contact iff  d = sqrt((ex ex + ey ey) + ez ez) <= R  for e = pos_a - pos_b,
//    not both points are static, and not (same object and |x0_a - x0_b|^2 < immune).  Stored: normal = e / d (0 when d == 0),
//    gap = dot(e, normal) normal, and -1 for the index of a static side.  The contacts leave sorted by (a, b).
//      cl_keys_kernel     pos, and per point the key (cx << 32 | cy << 16 | cz) of its cell, c = clamp(floor(p / S)) + 2^15, and
//                         its index as the value; a NaN or infinite point gets the key 2^48, beyond every cell.
//                         S = R (1 + 2^-6): two points with d <= R are at most R (1 + 4 u) apart on an axis, their quotients
//                         p / S carry an error of at most 2^-9 each below 2^15 cells, so their cells differ by at most
//                         R / S + 2^-8 < 1, that is by one; the clamp is monotone and keeps that.
//      ss_sort            (key, index), seven stable passes (48 cell bits and the no-cell bit): the points of a cell form a run
//      cl_count_kernel    one thread per point a: the nine (cx + i, cy + j, cz - 1 .. cz + 1) key ranges by two binary searches
//                         each, every b > a in them through the exact test -> count[a]
//      ss_scan            exclusive -> offs (N + 1)
//      cl_totals_kernel   total = offs[N], and emitted = offs[a* + 1] for the last a* with offs[a*] < max_pairs: every pair of
//                         the points up to a*, which holds the max_pairs smallest (a, b).  ONE host read of both.
//      cl_emit_kernel     the same walk for a <= a*: keys a << 32 | b at offs[a] ...
//      ss_sort            the keys alone, over the bits of N in either half
//      cl_finish_kernel   one thread per kept contact: indices, normal and gap from its key
//    No atomics, no flag polling, no grid barrier; every loop runs over a range read once.  Every index that comes from data (a
//    sorted id, a range of the binary search, an emit position, a and b of a key) is checked against its buffer's size.
//
// 2. THE TERMS of a contact (cl_contact), the reference's three kernels expression for expression: offset = (dx_a - dx0_a) + gap -
//    (dx_b - dx0_b), a static side's delta zero; rc = radius if side b is static else 2 radius; d_hat = dot(offset, n) / rc;
//    active for rp < d_hat <= 1; E = -(d_hat - 1)^2 log(d_hat - rp) + mu_fn dt h(|vt|) with the three friction regimes
//    (|vt| < 1e-4, < 1, >= 1) and the third-derivative chain term in the Hessian.  The Hessian is the derivative of the gradient,
//    which the reference's is not in two places: its stick regime divides vt vt^T by |vt| dt where the derivative has |vt|, and
//    its d3E takes d(barrier + dc / dp) as dbar - dc / dp^2 where it is dbar + (dp - dc) / dp^2.  cl_terms_kernel: one thread per contact,
//    grid-stride, one launch per quantity; the energy adds up wave -> LDS -> one partial per workgroup -> ra_sum_kernel, in order.
//
// 3. cl_reduced_kernel: with W = 4 H, xt = (x0, 1) and  m_c[4 h + n] = w[a][h] xt_a[n] - w[b][h] xt_b[n]  (a static side: zeros),
//    row 3 c + b of the collision Jacobian J = J_a - J_b holds m_c in the columns 12 h + 4 b + n, so
//      g[h][b][n]  = sum_c grad_c[b] m_c[4 h + n]
//      K_bb'[i][j] = sum_c H_c[b][b'] m_c[i] m_c[j]          nine W x W GEMMs of depth C
//    and K[(h,b,n),(h',b',n')] = K_bb'[4 h + n][4 h' + n'].  H_c is not symmetric (the friction cross terms), so all nine (b, b')
//    are computed; each K_bb' is symmetric in itself, so only the 64 x 64 tiles on and under the diagonal are, and of a diagonal
//    tile only the 16 x 16 blocks on and under it.
//    The grid, the sums of g and E, the slices' partials and their finish are those of reduced_assembly.h; the partials hold the nine
//    blocks of RaFullNine.  The workgroup strides over its slice in chunks of CC = 32 contacts.  Per chunk:
//      (a) thread q < 32 evaluates contact q: grad_c, H_c (and E) from the contact data -> LDS, with a, b and xt_a, xt_b
//      (b) all threads gather the weight rows through a, b into the LDS images of m for the tile's rows and for its columns
//          (zeros for a static side, past W and past the slice)
//      (c) v_mfma_f32_16x16x4_f32: lane l holds A[row l & 15][k = l >> 4] = m_c[row] H_c[b][b'] and B[k][col l & 15] = m_c[col],
//          c = 4 step + k: the scaling by H_c[b][b'] happens in the register (9 multiplies a step), no scaled image is written.
//          9 x 4 x 4 = 144 accumulator registers.
//      g: grad_c[b] m_c of the row tile; E: in the threads that evaluate the contacts.
//    The finish reads entry (i, j) and (j, i) of a block from the same partials: K[12 h + 4 b + n][12 h' + 4 b' + n'] equals
//    K[12 h' + 4 b + n'][12 h + 4 b' + n] to the bit.
//    LDS: 2 images of 32 x 80 floats (20 KiB) + 2.2 KiB of contact data.
#include "reduced_assembly.h"
#include "sort_scan.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr int CL_CC = 32;                      // contacts per chunk = GEMM depth of a chunk
constexpr int CL_MAX_SLICES = 128;
constexpr int CL_CELL_BITS = 16;
constexpr int CL_CELL_MAX = (1 << CL_CELL_BITS) - 1;
constexpr unsigned long long CL_NO_CELL = 1ull << (3 * CL_CELL_BITS);   // the key of a NaN or infinite point

struct ClParams {
  float coeff, radius, rp, mu, dt, nu;   // dt = dt * friction_reg, nu = friction_fluid * friction_reg, mu = friction
};

__device__ __forceinline__ float cl_dot(const float* u, const float* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// ---- 2. the terms of one contact -----------------------------------------------------------------------------------------------------
// offset of contact c; returns whether side b is static (index -1).  An index outside [0, N) counts as static.
__device__ __forceinline__ bool cl_offset(int64_t N, const float* __restrict__ dx, const float* __restrict__ dx0,
                                          const float* __restrict__ gaps, int a, int b, int64_t c, float* off) {
  const bool has_a = a >= 0 && a < N, has_b = b >= 0 && b < N;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float v = gaps[c * 3 + k];
    if (has_a) v = (dx[(int64_t)a * 3 + k] - dx0[(int64_t)a * 3 + k]) + v;
    if (has_b) v = v - (dx[(int64_t)b * 3 + k] - dx0[(int64_t)b * 3 + k]);
    off[k] = v;
  }
  return !has_b;
}

// returns coeff * E; g (3) and Hm (3 x 3 row-major) when asked for, each scaled by coeff, exact zeros for an inactive contact
template <bool GRAD, bool HESS>
__device__ __forceinline__ float cl_contact(const ClParams& p, const float* off, const float* n, bool static_b, float* g, float* Hm) {
  if (GRAD) g[0] = g[1] = g[2] = 0.0f;
  if (HESS) {
#pragma unroll
    for (int k = 0; k < 9; ++k) Hm[k] = 0.0f;
  }
  const float rc = (static_b ? 1.0f : 2.0f) * p.radius;
  const float d = cl_dot(off, n);
  const float d_hat = d / rc;
  if (!(p.rp < d_hat && d_hat <= 1.0f)) return 0.0f;
  const float dc = d_hat - 1.0f, dp = d_hat - p.rp;
  const float lg = logf(dp), barrier = 2.0f * lg;
  const float dE = -dc * (barrier + dc / dp);
  float vt[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) vt[k] = (off[k] - d * n[k]) / p.dt;
  const float vtn = sqrtf(cl_dot(vt, vt));
  const float mu_fn = -p.mu * dE / rc;
  const float h_vt = 0.5f * p.nu * vtn * vtn + (vtn < 1.0f ? vtn * vtn * (1.0f - vtn / 3.0f) : vtn - 1.0f / 3.0f);
  const float E = -(dc * dc) * lg + mu_fn * p.dt * h_vt;
  if (GRAD || HESS) {
    const float f1 = vtn < 1.0f ? 2.0f - vtn : 1.0f / vtn;
    const float dbar = 2.0f / dp, ddcdp = (dp - dc) / (dp * dp);
    const float d2E = -(barrier + dc / dp) - dc * (dbar + ddcdp);
    const float f1_nu = f1 + p.nu;
    if (GRAD) {
      const float gn = dE / rc, gt = mu_fn * f1_nu, gc = -p.mu * p.dt * h_vt * d2E / (rc * rc);
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] = p.coeff * ((gn * n[k] + gt * vt[k]) + gc * n[k]);
    }
    if (HESS) {
      const float eps = 1.0e-4f;
      const float hn = d2E / (rc * rc), mu_fn_p = -p.mu * d2E / rc;
      const float h_vt_p = vtn < 1.0f ? p.nu * vtn + 2.0f * vtn - vtn * vtn : p.nu * vtn + 1.0f;
      const float d2bar = -2.0f / (dp * dp), dddcdp = -2.0f * ddcdp / dp;
      const float df = dbar + ddcdp, dg = d2bar + dddcdp;
      const float d3E = -df - dg * dc - (dbar + ddcdp);
      const float chain = -p.mu * p.dt / (rc * rc);
      const float cross = mu_fn_p * f1_nu / rc, cn = d2E * h_vt_p, cnn = h_vt * d3E / rc;
      // the friction block: ft * (I - n n^T) + fv * vt vt^T
      float ft, fv;
      if (vtn < eps) {
        ft = mu_fn / p.dt * f1_nu, fv = 0.0f;
      } else if (vtn < 1.0f) {
        ft = mu_fn / p.dt * f1_nu, fv = -(mu_fn / p.dt) / vtn;
      } else {
        ft = mu_fn * (f1_nu / p.dt), fv = mu_fn * ((-1.0f / (vtn * vtn)) / (vtn * p.dt));
      }
      const float dv = vtn > eps ? 1.0f / (vtn * p.dt) : 0.0f;   // dvtn_doffset = vt * dv
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const float nn = n[i] * n[j];
          float h = hn * nn;
          h = h + (ft * ((i == j ? 1.0f : 0.0f) - nn) + fv * (vt[i] * vt[j]));
          h = h + cross * (vt[i] * n[j]);
          h = h + chain * (cn * (n[i] * (vt[j] * dv)) + cnn * nn);
          Hm[i * 3 + j] = p.coeff * h;
        }
    }
  }
  return p.coeff * E;
}

struct ClContacts {
  int64_t C, N;
  const float *dx, *dx0, *gaps, *nor;
  const int *ia, *ib;
};

// MODE 0: energy partials, 1: gradient (C, 3), 2: Hessian (C, 3, 3)
template <int MODE>
__global__ __launch_bounds__(RA_THREADS) void cl_terms_kernel(const ClContacts k, const ClParams p, float* __restrict__ out) {
  float e_acc = 0.0f, e_comp = 0.0f;
  for (int64_t c = (int64_t)blockIdx.x * RA_THREADS + threadIdx.x; c < k.C; c += (int64_t)gridDim.x * RA_THREADS) {
    float off[3], g[3], Hm[9];
    const float n[3] = {k.nor[c * 3], k.nor[c * 3 + 1], k.nor[c * 3 + 2]};
    const bool static_b = cl_offset(k.N, k.dx, k.dx0, k.gaps, k.ia[c], k.ib[c], c, off);
    const float e = cl_contact<MODE == 1, MODE == 2>(p, off, n, static_b, g, Hm);
    if (MODE == 0) ra_add(e_acc, e_comp, e);
    if (MODE == 1) {
#pragma unroll
      for (int j = 0; j < 3; ++j) out[c * 3 + j] = g[j];
    }
    if (MODE == 2) {
#pragma unroll
      for (int j = 0; j < 9; ++j) out[c * 9 + j] = Hm[j];
    }
  }
  if (MODE == 0) ra_block_energy(e_acc, out);
}

// ---- 1. detection -------------------------------------------------------------------------------------------------------------------------
struct ClDetect {
  int64_t N;
  const float *pos, *x0;
  const int *obj, *stat;
  float R, S, immune;
  long long max_pairs;
  const unsigned long long* cells;   // sorted cell keys
  const long long* ids;              // and the point of each
  const long long* offs;             // (N + 1) exclusive scan of the counts
};

__device__ __forceinline__ int cl_cell(float p, float S) {
  const float c = fminf(fmaxf(floorf(p / S), -32768.0f), 32767.0f);   // a NaN quotient (0 / 0) lands on the lower bound
  return (int)c + 32768;
}
__device__ __forceinline__ unsigned long long cl_key(int cx, int cy, int cz) {
  return ((unsigned long long)cx << (2 * CL_CELL_BITS)) | ((unsigned long long)cy << CL_CELL_BITS) | (unsigned long long)cz;
}

__global__ __launch_bounds__(256) void cl_keys_kernel(int64_t N, const float* __restrict__ x0, const float* __restrict__ dx, float S,
                                                      float* __restrict__ pos, unsigned long long* __restrict__ keys,
                                                      long long* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  float p[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = x0[i * 3 + k] + dx[i * 3 + k], pos[i * 3 + k] = p[k];
  const bool finite = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
  keys[i] = finite ? cl_key(cl_cell(p[0], S), cl_cell(p[1], S), cl_cell(p[2], S)) : CL_NO_CELL;
  vals[i] = i;
}

// first position of the ascending keys[0 .. n) whose key is >= key
__device__ __forceinline__ long long cl_lower_bound(const unsigned long long* __restrict__ keys, long long n, unsigned long long key) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (keys[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// the exact test of the pair (a, b), a < b
__device__ __forceinline__ bool cl_is_contact(const ClDetect& q, int64_t a, int64_t b, const float* pa) {
  float e[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) e[k] = pa[k] - q.pos[b * 3 + k];
  const float d = sqrtf(cl_dot(e, e));
  if (!(d <= q.R)) return false;   // a NaN or infinite point is in no contact
  if (q.stat[a] == 1 && q.stat[b] == 1) return false;
  if (q.obj[a] == q.obj[b]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = q.x0[a * 3 + k] - q.x0[b * 3 + k];
    if (cl_dot(e, e) < q.immune) return false;
  }
  return true;
}

// the contacts (a, b), b > a, of point a: counted, or written as keys at out[base ...] while below `room`
template <bool EMIT>
__device__ __forceinline__ int cl_walk(const ClDetect& q, int64_t a, unsigned long long* __restrict__ out, long long base, long long room) {
  const float pa[3] = {q.pos[a * 3], q.pos[a * 3 + 1], q.pos[a * 3 + 2]};
  if (!(isfinite(pa[0]) && isfinite(pa[1]) && isfinite(pa[2]))) return 0;
  const int cx = cl_cell(pa[0], q.S), cy = cl_cell(pa[1], q.S), cz = cl_cell(pa[2], q.S);
  const int zlo = cz > 0 ? cz - 1 : 0, zhi = cz < CL_CELL_MAX ? cz + 1 : CL_CELL_MAX;
  int count = 0;
  for (int ox = -1; ox <= 1; ++ox)
    for (int oy = -1; oy <= 1; ++oy) {
      const int nx = cx + ox, ny = cy + oy;
      if (nx < 0 || nx > CL_CELL_MAX || ny < 0 || ny > CL_CELL_MAX) continue;
      const long long lo = cl_lower_bound(q.cells, q.N, cl_key(nx, ny, zlo));
      const long long hi = cl_lower_bound(q.cells, q.N, cl_key(nx, ny, zhi) + 1ull);   // both in [0, N]
      for (long long t = lo; t < hi; ++t) {
        const long long b = q.ids[t];
        if (b <= a || b >= q.N) continue;
        if (!cl_is_contact(q, a, b, pa)) continue;
        if (EMIT) {
          const long long at = base + count;
          if (at >= 0 && at < room) out[at] = ((unsigned long long)a << 32) | (unsigned long long)b;
        }
        ++count;
      }
    }
  return count;
}

__global__ __launch_bounds__(256) void cl_count_kernel(const ClDetect q, int* __restrict__ counts) {
  const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (a < q.N) counts[a] = cl_walk<false>(q, a, nullptr, 0, 0);
}
// out[0] = all contacts, out[1] = those of the points whose exclusive offset is below max_pairs (exactly one thread finds it)
__global__ __launch_bounds__(256) void cl_totals_kernel(int64_t N, const long long* __restrict__ offs, long long max_pairs,
                                                        long long* __restrict__ out) {
  const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (a >= N) return;
  if (a == 0) out[0] = offs[N];
  if (offs[a] < max_pairs && (a == N - 1 || offs[a + 1] >= max_pairs)) out[1] = offs[a + 1];
}
__global__ __launch_bounds__(256) void cl_emit_kernel(const ClDetect q, unsigned long long* __restrict__ keys, long long emitted) {
  const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (a >= q.N) return;
  const long long base = q.offs[a];
  if (base < q.max_pairs) cl_walk<true>(q, a, keys, base, emitted);
}
__global__ __launch_bounds__(256) void cl_finish_contacts_kernel(const ClDetect q, long long kept, const unsigned long long* __restrict__ keys,
                                                                 int* __restrict__ ia, int* __restrict__ ib,
                                                                 float* __restrict__ normals, float* __restrict__ gaps,
                                                                 int* __restrict__ pair_objects) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= kept) return;
  const long long a = (long long)(keys[c] >> 32), b = (long long)(keys[c] & 0xFFFFFFFFull);
  float n[3] = {0.0f, 0.0f, 0.0f}, e[3] = {0.0f, 0.0f, 0.0f};
  int sa = -1, sb = -1, oa = -1, ob = -1;
  if (a < q.N && b < q.N) {   // keys are unsigned: no lower bound to check
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = q.pos[a * 3 + k] - q.pos[b * 3 + k];
    const float d = sqrtf(cl_dot(e, e));
    if (d != 0.0f) {
#pragma unroll
      for (int k = 0; k < 3; ++k) n[k] = e[k] / d;
    }
    sa = q.stat[a] == 1 ? -1 : (int)a, sb = q.stat[b] == 1 ? -1 : (int)b;
    oa = q.obj[a], ob = q.obj[b];
  }
  const float dn = cl_dot(e, n);
  ia[c] = sa, ib[c] = sb;
  if (pair_objects != nullptr) pair_objects[c * 2] = oa, pair_objects[c * 2 + 1] = ob;
#pragma unroll
  for (int k = 0; k < 3; ++k) normals[c * 3 + k] = n[k], gaps[c * 3 + k] = dn * n[k];
}

// the workspace of the count phase, kept for the emit phase
struct ClLayout {
  size_t pos, keys_a, keys_b, vals_a, vals_b, counts, offs, sums, hist, sort_offs, totals, bytes;
};
inline ClLayout cl_layout(int64_t N) {
  ClLayout l;
  size_t at = 0;
  const size_t n = (size_t)N;
  l.pos = at, at += kamd_align16(n * 3 * sizeof(float));
  l.keys_a = at, at += kamd_align16(n * 8);
  l.keys_b = at, at += kamd_align16(n * 8);
  l.vals_a = at, at += kamd_align16(n * 8);
  l.vals_b = at, at += kamd_align16(n * 8);
  l.counts = at, at += kamd_align16(n * sizeof(int));
  l.offs = at, at += kamd_align16((n + 1) * 8);
  l.sums = at, at += kamd_align16(ss_sort_unique_sums_entries(N) * 8);
  l.hist = at, at += kamd_align16(ss_sort_hist_entries(N) * sizeof(int));
  l.sort_offs = at, at += kamd_align16(ss_sort_offs_entries(N) * 8);
  l.totals = at, at += 16;
  l.bytes = at;
  return l;
}
// of the emit phase: the keys and their sort
struct ClEmitLayout {
  size_t keys_a, keys_b, sums, hist, sort_offs, bytes;
};
inline ClEmitLayout cl_emit_layout(int64_t M) {
  ClEmitLayout l;
  size_t at = 0;
  const size_t m = (size_t)M;
  l.keys_a = at, at += kamd_align16(m * 8);
  l.keys_b = at, at += kamd_align16(m * 8);
  l.sums = at, at += kamd_align16(ss_sort_sums_entries(M) * 8);
  l.hist = at, at += kamd_align16(ss_sort_hist_entries(M) * sizeof(int));
  l.sort_offs = at, at += kamd_align16(ss_sort_offs_entries(M) * 8);
  l.bytes = at;
  return l;
}
inline bool cl_points_ok(int64_t N) { return N >= 1 && N <= 0x7FFFFFFFLL; }
inline float cl_cell_edge(float R) { return R * 1.015625f; }
inline ClDetect cl_detect_args(int64_t N, const float* x0, const int* obj, const int* stat, float R, float immune, int64_t max_pairs,
                               char* ws, const ClLayout& l) {
  ClDetect q;
  q.N = N, q.pos = (const float*)(ws + l.pos), q.x0 = x0, q.obj = obj, q.stat = stat;
  q.R = R, q.S = cl_cell_edge(R), q.immune = immune, q.max_pairs = max_pairs;
  q.cells = (const unsigned long long*)(ws + l.keys_a), q.ids = (const long long*)(ws + l.vals_a);
  q.offs = (const long long*)(ws + l.offs);
  return q;
}

// ---- 3. the reduced terms ---------------------------------------------------------------------------------------------------------------
struct ClReduced {
  ClContacts k;
  ClParams p;
  const float *w, *x0;   // (N, H), (N, 3)
  int64_t per;           // contacts per slice
  int H, W, T;           // handles, 4 H, tiles per side
  RaPartials part;       // K's blocks: (b, b')
};

// m_q[col] of the chunk's contact q (0 past W, for a static side and for a contact past the slice)
__device__ __forceinline__ float cl_m(const ClReduced& r, const int* s_a, const int* s_b, const float* s_xa, const float* s_xb, int q,
                                      int col) {
  if (col >= r.W) return 0.0f;
  const int h = col >> 2, n = col & 3, a = s_a[q], b = s_b[q];
  const float va = a >= 0 ? r.w[(int64_t)a * r.H + h] * s_xa[q * 4 + n] : 0.0f;
  const float vb = b >= 0 ? r.w[(int64_t)b * r.H + h] * s_xb[q * 4 + n] : 0.0f;
  return va - vb;
}

template <bool HESS>
__global__ __launch_bounds__(RA_THREADS) void cl_reduced_kernel(const ClReduced r) {
  __shared__ float s_MI[CL_CC * RA_LS], s_MJ[CL_CC * RA_LS];
  __shared__ float s_H[CL_CC * 9], s_g[CL_CC * 3], s_xa[CL_CC * 4], s_xb[CL_CC * 4], s_e[CL_CC];
  __shared__ int s_a[CL_CC], s_b[CL_CC];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t slice = blockIdx.x;
  int ti = (int)blockIdx.y, tj = 0;
  if (HESS) ra_lower_tile((int)blockIdx.y, ti, tj);
  const int i0 = ti * RA_TILE, j0 = tj * RA_TILE, W = r.W;
  const bool diag = ti == tj, sums_g = tj == 0, sums_e = ti == 0 && tj == 0;
  const float* MJ = diag ? s_MI : s_MJ;
  const int64_t begin = slice * r.per, end = begin + r.per < r.k.C ? begin + r.per : r.k.C;
  ra_f32x4 acc[9][4];
#pragma unroll
  for (int pr = 0; pr < 9; ++pr)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[pr][cb] = ra_f32x4{0.f, 0.f, 0.f, 0.f};
  float g_acc = 0.0f, g_comp = 0.0f, e_acc = 0.0f, e_comp = 0.0f;

  for (int64_t c0 = begin; c0 < end; c0 += CL_CC) {
    __syncthreads();  // the previous chunk's images are no longer read
    // (a) the contacts of the chunk
    if (t < CL_CC) {
      const int64_t c = c0 + t;
      float g[3] = {0.0f, 0.0f, 0.0f}, Hm[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, e = 0.0f;
      int a = -1, b = -1;
      if (c < end) {
        float off[3];
        const float n[3] = {r.k.nor[c * 3], r.k.nor[c * 3 + 1], r.k.nor[c * 3 + 2]};
        a = r.k.ia[c], b = r.k.ib[c];
        const bool static_b = cl_offset(r.k.N, r.k.dx, r.k.dx0, r.k.gaps, a, b, c, off);
        e = cl_contact<true, HESS>(r.p, off, n, static_b, g, Hm);
        if (a < 0 || a >= r.k.N) a = -1;
        if (b < 0 || b >= r.k.N) b = -1;
      }
      s_a[t] = a, s_b[t] = b;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        s_g[t * 3 + k] = g[k];
        s_xa[t * 4 + k] = a >= 0 ? r.x0[(int64_t)a * 3 + k] : 0.0f;
        s_xb[t * 4 + k] = b >= 0 ? r.x0[(int64_t)b * 3 + k] : 0.0f;
      }
      s_xa[t * 4 + 3] = 1.0f, s_xb[t * 4 + 3] = 1.0f;
      if (HESS) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s_H[t * 9 + k] = Hm[k];
      }
      if (sums_e) ra_add(e_acc, e_comp, e);
    }
    __syncthreads();
    // (b) the images of m
    for (int e = t; e < CL_CC * RA_TILE; e += RA_THREADS) {
      const int q = e >> 6, col = e & 63;
      s_MI[q * RA_LS + col] = cl_m(r, s_a, s_b, s_xa, s_xb, q, i0 + col);
      if (HESS && !diag) s_MJ[q * RA_LS + col] = cl_m(r, s_a, s_b, s_xa, s_xb, q, j0 + col);
    }
    __syncthreads();
    if (sums_g && t < 3 * RA_TILE) {
      const int b = t >> 6;  // per contact, then the chunk's contacts pairwise, then onto the running sum with its error carried
      float v[CL_CC];
#pragma unroll
      for (int q = 0; q < CL_CC; ++q) v[q] = s_g[q * 3 + b] * s_MI[q * RA_LS + lane];
      ra_add(g_acc, g_comp, ra_pairwise(v));
    }
    // (c) lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], D[row 4 (l >> 4) + reg][col l & 15]
    if (HESS && i0 + wave * 16 < W) {
      const int kq = lane >> 4, rr = lane & 15;
      for (int d = 0; d < CL_CC; d += 4) {
        const float av = s_MI[(d + kq) * RA_LS + wave * 16 + rr];
        float as[9];
#pragma unroll
        for (int pr = 0; pr < 9; ++pr) as[pr] = av * s_H[(d + kq) * 9 + pr];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
          if (j0 + cb * 16 < W && (!diag || cb <= wave)) {
            const float bv = MJ[(d + kq) * RA_LS + cb * 16 + rr];
#pragma unroll
            for (int pr = 0; pr < 9; ++pr) acc[pr][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[pr], bv, acc[pr][cb], 0, 0, 0);
          }
      }
    }
  }

  if (HESS) {
    ra_store_blocks(acc, r.part.Kp, slice, W, i0, j0, wave, lane, diag);
  }
  if (sums_g && t < 3 * RA_TILE && i0 + lane < W) r.part.gp[((size_t)slice * 3 + (t >> 6)) * W + i0 + lane] = g_acc;
  if (sums_e) ra_slice_energy<CL_CC>(e_acc, t < CL_CC, t, s_e, r.part.ep + slice);
}

inline int64_t cl_slice_contacts(int64_t C, int H) { return ra_slice_len(C, ra_tri(ra_tiles(H)), CL_CC, CL_MAX_SLICES); }
inline ClParams cl_params(float coeff, float radius, float rp, float mu, float dt, float nu) {
  ClParams p;
  p.coeff = coeff, p.radius = radius, p.rp = rp, p.mu = mu, p.dt = dt, p.nu = nu;
  return p;
}

}  // namespace

extern "C" {

size_t kamd_collision_detect_workspace(int64_t N) { return cl_points_ok(N) ? cl_layout(N).bytes : 0; }

int kamd_collision_count_f32(void* stream, int64_t N, const float* dx, const float* x0, const int* obj_ids, const int* is_static,
                             float detection_radius, float immune_radius, int64_t max_pairs, void* workspace, size_t workspace_bytes,
                             int64_t* host_counts) {
  if (!cl_points_ok(N) || max_pairs < 1 || dx == nullptr || x0 == nullptr || obj_ids == nullptr || is_static == nullptr ||
      workspace == nullptr || host_counts == nullptr || workspace_bytes < cl_layout(N).bytes)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const ClLayout l = cl_layout(N);
  char* ws = (char*)workspace;
  const ClDetect q = cl_detect_args(N, x0, obj_ids, is_static, detection_radius, immune_radius, max_pairs, ws, l);
  unsigned long long *keys_a = (unsigned long long*)(ws + l.keys_a), *keys_b = (unsigned long long*)(ws + l.keys_b);
  long long *vals_a = (long long*)(ws + l.vals_a), *vals_b = (long long*)(ws + l.vals_b);
  long long *offs = (long long*)(ws + l.offs), *sums = (long long*)(ws + l.sums), *totals = (long long*)(ws + l.totals);
  int* counts = (int*)(ws + l.counts);
  const unsigned grid = ss_grid(N, 256);
  hipLaunchKernelGGL(cl_keys_kernel, dim3(grid), dim3(256), 0, st, N, x0, dx, q.S, (float*)(ws + l.pos), keys_b, vals_b);
  // an odd number of passes: from the b side, which the second pass reuses, into the a side
  KAMD_CHECK(ss_sort(st, N, ss_passes_low(3 * CL_CELL_BITS + 1), (const unsigned long long*)keys_b, (const long long*)vals_b, keys_b,
                     vals_b, keys_a, vals_a, ss_sort_ws((int*)(ws + l.hist), (long long*)(ws + l.sort_offs), sums)));
  hipLaunchKernelGGL(cl_count_kernel, dim3(grid), dim3(256), 0, st, q, counts);
  KAMD_CHECK(ss_scan(st, N, (const long long*)nullptr, (const int*)counts, offs, sums));
  hipLaunchKernelGGL(cl_totals_kernel, dim3(grid), dim3(256), 0, st, N, (const long long*)offs, (long long)max_pairs, totals);
  KAMD_CHECK(hipGetLastError());
  long long h[2] = {0, 0};
  KAMD_CHECK(hipMemcpyAsync(h, totals, 16, hipMemcpyDeviceToHost, st));
  KAMD_CHECK(hipStreamSynchronize(st));
  host_counts[0] = h[0], host_counts[1] = h[1];
  return 0;
}

size_t kamd_collision_emit_workspace(int64_t emitted) { return emitted >= 1 ? cl_emit_layout(emitted).bytes : 0; }

int kamd_collision_emit_f32(void* stream, int64_t N, const float* x0, const int* obj_ids, const int* is_static, float detection_radius,
                            float immune_radius, int64_t max_pairs, void* workspace, size_t workspace_bytes, int64_t emitted,
                            int64_t kept, void* emit_workspace, size_t emit_workspace_bytes, int* indices_a, int* indices_b,
                            float* normals, float* gaps, int* pair_objects) {
  if (!cl_points_ok(N) || max_pairs < 1 || emitted < 1 || kept < 1 || kept > emitted || kept > max_pairs || x0 == nullptr ||
      obj_ids == nullptr || is_static == nullptr || workspace == nullptr || workspace_bytes < cl_layout(N).bytes ||
      emit_workspace == nullptr || emit_workspace_bytes < cl_emit_layout(emitted).bytes || indices_a == nullptr ||
      indices_b == nullptr || normals == nullptr || gaps == nullptr)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const ClLayout l = cl_layout(N);
  const ClEmitLayout m = cl_emit_layout(emitted);
  char *ws = (char*)workspace, *es = (char*)emit_workspace;
  const ClDetect q = cl_detect_args(N, x0, obj_ids, is_static, detection_radius, immune_radius, max_pairs, ws, l);
  unsigned long long *keys_a = (unsigned long long*)(es + m.keys_a), *keys_b = (unsigned long long*)(es + m.keys_b);
  hipLaunchKernelGGL(cl_emit_kernel, dim3(ss_grid(N, 256)), dim3(256), 0, st, q, keys_a, (long long)emitted);
  int bits = 1;
  while (bits < 32 && ((int64_t)1 << bits) < N) ++bits;
  KAMD_CHECK(ss_sort(st, emitted, ss_passes_halves(bits), (const unsigned long long*)keys_a, keys_b, keys_a,
                     ss_sort_ws((int*)(es + m.hist), (long long*)(es + m.sort_offs), (long long*)(es + m.sums))));
  hipLaunchKernelGGL(cl_finish_contacts_kernel, dim3(ss_grid(kept, 256)), dim3(256), 0, st, q, (long long)kept,
                     (const unsigned long long*)keys_a, indices_a, indices_b, normals, gaps, pair_objects);
  KAMD_RETURN_LAST_ERROR();
}

size_t kamd_collision_terms_workspace(int64_t C) { return C > 0 ? kamd_align16((size_t)ra_term_blocks(C, RA_THREADS) * sizeof(float)) : 0; }

int kamd_collision_terms_f32(void* stream, int64_t C, int64_t N, const float* dx, const float* dx0, const float* gaps,
                             const float* normals, const int* indices_a, const int* indices_b, float coeff, float radius,
                             float barrier_ratio, float mu, float dt, float nu, float* energy, float* gradient, float* hessian,
                             void* workspace) {
  if (C < 0 || N < 0) return (int)hipErrorInvalidValue;
  if (C == 0 || (energy == nullptr && gradient == nullptr && hessian == nullptr)) return 0;
  if (dx == nullptr || dx0 == nullptr || gaps == nullptr || normals == nullptr || indices_a == nullptr || indices_b == nullptr ||
      (energy != nullptr && workspace == nullptr))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  ClContacts k;
  k.C = C, k.N = N, k.dx = dx, k.dx0 = dx0, k.gaps = gaps, k.nor = normals, k.ia = indices_a, k.ib = indices_b;
  const ClParams p = cl_params(coeff, radius, barrier_ratio, mu, dt, nu);
  const int blocks = ra_term_blocks(C, RA_THREADS);
  if (energy != nullptr) {
    hipLaunchKernelGGL(cl_terms_kernel<0>, dim3((unsigned)blocks), dim3(RA_THREADS), 0, st, k, p, (float*)workspace);
    hipLaunchKernelGGL(ra_sum_kernel, dim3(1), dim3(KAMD_WAVE), 0, st, blocks, (const float*)workspace, energy);
  }
  if (gradient != nullptr) hipLaunchKernelGGL(cl_terms_kernel<1>, dim3((unsigned)blocks), dim3(RA_THREADS), 0, st, k, p, gradient);
  if (hessian != nullptr) hipLaunchKernelGGL(cl_terms_kernel<2>, dim3((unsigned)blocks), dim3(RA_THREADS), 0, st, k, p, hessian);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_collision_chunk_contacts(void) { return CL_CC; }
int64_t kamd_collision_slice_contacts(int64_t C, int H) { return ra_sizes_ok(C, H) ? cl_slice_contacts(C, H) : 0; }

size_t kamd_collision_reduced_workspace(int64_t C, int H, int hessian) {
  if (!ra_sizes_ok(C, H) || C == 0) return 0;
  return ra_workspace(ra_slices(C, cl_slice_contacts(C, H)), RaFullNine::BLOCKS, H, hessian);
}

int kamd_collision_reduced_f32(void* stream, int64_t C, int64_t N, int H, const float* dx, const float* dx0, const float* gaps,
                               const float* normals, const int* indices_a, const int* indices_b, const float* weights,
                               const float* x0, float coeff, float radius, float barrier_ratio, float mu, float dt, float nu,
                               int hessian, float* E, float* g, float* K, void* workspace, size_t workspace_bytes) {
  if (!ra_sizes_ok(C, H) || N < 0 || N > 0x7FFFFFFFLL || C == 0) return (int)hipErrorInvalidValue;
  if (dx == nullptr || dx0 == nullptr || gaps == nullptr || normals == nullptr || indices_a == nullptr || indices_b == nullptr ||
      weights == nullptr || x0 == nullptr || E == nullptr || g == nullptr || (hessian && K == nullptr) || workspace == nullptr ||
      workspace_bytes < kamd_collision_reduced_workspace(C, H, hessian))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  ClReduced r;
  r.k.C = C, r.k.N = N, r.k.dx = dx, r.k.dx0 = dx0, r.k.gaps = gaps, r.k.nor = normals, r.k.ia = indices_a, r.k.ib = indices_b;
  r.p = cl_params(coeff, radius, barrier_ratio, mu, dt, nu);
  r.w = weights, r.x0 = x0, r.per = cl_slice_contacts(C, H), r.H = H, r.W = 4 * H, r.T = ra_tiles(H);
  const size_t S = ra_slices(C, r.per);
  ra_workspace(S, RaFullNine::BLOCKS, H, hessian, workspace, &r.part);
  if (hessian)
    hipLaunchKernelGGL(cl_reduced_kernel<true>, dim3((unsigned)S, (unsigned)ra_tri(r.T)), dim3(RA_THREADS), 0, st, r);
  else
    hipLaunchKernelGGL(cl_reduced_kernel<false>, dim3((unsigned)S, (unsigned)r.T), dim3(RA_THREADS), 0, st, r);
  return ra_finish<RaFullNine>(st, S, H, r.part, hessian ? K : nullptr, g, E);
}
}
