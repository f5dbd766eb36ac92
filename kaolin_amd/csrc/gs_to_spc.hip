// gs_to_voxelgrid: 3D Gaussians -> the voxels of an SPC level that their iso-surface ellipsoids overlap, one (voxel, Gaussian) pair
// per overlap, and the opacity of every pair integrated over step^3 samples of the voxel.
//
// Replaces kaolin/csrc/ops/conversions/gs_to_spc/gs_to_spc_cuda.cu (:146-309 the ellipsoid / voxel test, :360-470 the inverse
// covariance, contact points and AABB of a Gaussian, :557-717 the host loop, :719-804 the integral).
//
// The reference advances ONE octree level per round trip (decide -> cub scan -> read the count on the host -> allocate -> write 8
// children per survivor), then sorts with cub.  Here (the scheme of mesh_to_spc.hip, spc_stage.h):
//   * one thread per Gaussian prepares cov3d_invs, the AABB and the three contact points;
//   * eight lanes take a proposal and finish THREE levels of its subtree in registers; each stage is a count pass, a scan and an
//     emit pass, and the host reads one number per stage.  Every level is tested, the root included: the tests are not monotone;
//   * pairs leave the last stage ordered by (Gaussian, Morton code); the stable radix sort on the 3*level key bits makes that
//     (Morton code, Gaussian), the order of the reference's stable sort; run heads are the pack boundaries;
//   * the integral: eight lanes per pair share the step^2 (i, j) columns, a lane sums its columns in order and the eight partial
//     sums are combined by a fixed butterfly -- no atomics, the same bits every run.
// The voxel tests use the reference's expressions in its operand order, float and double where it has them, no fused multiply-add
// (-ffp-contract=off) except the fmaf it spells (arithmetic contract).  Bit-exact vs tests/gs_to_spc_bruteforce.py.
#include <float.h>
#include <hip/hip_runtime.h>
#include "common.h"
#include "sort_scan.h"
#include "spc_stage.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr int GS_STAGE_LEVELS = 3;  // levels finished per stage below the proposal's own
constexpr int GS_MAX_LEVEL = 15;    // KAOLIN_SPC_MAX_LEVELS
constexpr int GS_PREP = 15;         // floats per Gaussian next to cov3d_invs: AABB min, AABB max, three contact points

// ---- per Gaussian (gs_to_spc_cuda.cu:360-470) ---------------------------------------------------------------------------------
__device__ __forceinline__ void gs_mul3x3(const float (*a)[3], const float (*b)[3], float (*c)[3]) {  // spc_math.h:201-217
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[i][j] = a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j];
}
__global__ __launch_bounds__(256) void gs_prepare_kernel(int64_t G, const float* __restrict__ means, const float* __restrict__ scales,
                                                         const float* __restrict__ rots, float iso, float tol, int level,
                                                         float* __restrict__ cov_out, float* __restrict__ prep) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  const float voxel = 2.0f / (float)(1 << level);
  const float min_scale = tol * voxel;
  const float sx = fmaxf(scales[g * 3], min_scale), sy = fmaxf(scales[g * 3 + 1], min_scale), sz = fmaxf(scales[g * 3 + 2], min_scale);
  const double det_s = ((double)sx) * ((double)sy) * ((double)sz);
  const float S[3][3] = {{1.0f / sx, 0.0f, 0.0f}, {0.0f, 1.0f / sy, 0.0f}, {0.0f, 0.0f, 1.0f / sz}};
  const float r = rots[g * 4], x = rots[g * 4 + 1], y = rots[g * 4 + 2], z = rots[g * 4 + 3];
  const float R[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y + r * z), 2.f * (x * z - r * y)},
                         {2.f * (x * y - r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z + r * x)},
                         {2.f * (x * z + r * y), 2.f * (y * z - r * x), 1.f - 2.f * (x * x + y * y)}};
  float M[3][3], Mt[3][3], Sg[3][3];
  gs_mul3x3(S, R, M);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Mt[i][j] = M[j][i];
  gs_mul3x3(Mt, M, Sg);
  const float cov[6] = {Sg[0][0], Sg[0][1], Sg[0][2], Sg[1][1], Sg[1][2], Sg[2][2]};
#pragma unroll
  for (int k = 0; k < 6; ++k) cov_out[g * 6 + k] = cov[k];
  const double c0 = cov[0], c1 = cov[1], c2 = cov[2], c3 = cov[3], c4 = cov[4], c5 = cov[5];
  const double h0 = c3 * c5 - c4 * c4;
  const double h1 = c2 * c4 - c1 * c5;
  const double h2 = c1 * c4 - c2 * c3;
  const double h3 = c0 * c5 - c2 * c2;
  const double h4 = c1 * c2 - c0 * c4;
  const double h5 = c0 * c3 - c1 * c1;
  const double w[3] = {det_s * sqrt((double)iso / h0), det_s * sqrt((double)iso / h3), det_s * sqrt((double)iso / h5)};
  const double Q[3][3] = {{h0, h1, h2}, {h1, h3, h4}, {h2, h4, h5}};
  float pmin[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, pmax[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  float* out = prep + g * GS_PREP;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float p = (float)(w[i] * Q[i][k]);
      const float m = -1.0f * p;
      out[6 + 3 * i + k] = p;
      pmin[k] = fminf(fminf(pmin[k], p), m);
      pmax[k] = fmaxf(fmaxf(pmax[k], p), m);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    out[k] = pmin[k] + means[g * 3 + k];
    out[3 + k] = pmax[k] + means[g * 3 + k];
  }
}

// ---- per (voxel, Gaussian) (gs_to_spc_cuda.cu:146-309) -----------------------------------------------------------------------
__device__ bool gs_edge_test(float c0, float c1, float c2, float c3, float c4, float c5, float iso, float s, float t, float l,
                             float u) {
  const double a = c0;
  const double b = (double)(2.0f * (c1 * s + c2 * t));
  const double c = (double)((c3 * s * s + 2.0f * c4 * s * t + c5 * t * t) - iso);
  const double dcrm = fmax(b * b - 4.0 * a * c, 0.0);
  if (!(dcrm > 0.0)) return false;
  const double b2a = -0.5 * b / a;
  const double rdcrm = 0.5 * sqrt(dcrm) / a;
  const double r0 = b2a - rdcrm, r1 = b2a + rdcrm;
  return !((double)u <= r0 || r1 <= (double)l);
}
__device__ bool gs_face_test(const float* p, const float* q, float vs, int i, int j, int k, float o) {
  const float t = (float)((double)(q[i] - (p[i] + o)) / (2.0 * (double)q[i]));
  if (!(0.0f <= t && t <= 1.0f)) return false;
  const double f = 1.0 - 2.0 * (double)t;
  const float hj = (float)(f * (double)q[j]), hk = (float)(f * (double)q[k]);
  return p[j] <= hj && hj <= (p[j] + vs) && p[k] <= hk && hk <= (p[k] + vs);
}

struct GsPrim {
  struct Data {
    float mean[3], cov[6], ab0[3], ab1[3], cp[3][3];
  };
  int64_t G;
  const float *means, *cov, *prep;
  float iso;
  __device__ __forceinline__ bool load(int64_t id, Data* d) const {
    if (id < 0 || id >= G) return false;  // guard: a Gaussian id outside the tables yields nothing
#pragma unroll
    for (int k = 0; k < 3; ++k) d->mean[k] = means[id * 3 + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) d->cov[k] = cov[id * 6 + k];
    const float* p = prep + id * GS_PREP;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      d->ab0[k] = p[k];
      d->ab1[k] = p[3 + k];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) d->cp[i][k] = p[6 + 3 * i + k];
    return true;
  }
  // GSVoxelInOut: inside || (overlap && (face || edge))
  __device__ bool test(const Data& d, int x, int y, int z, int level) const {
    const float vs = 2.0f / (float)(1 << level);
    const float v[3] = {fmaf((float)x, vs, -1.0f), fmaf((float)y, vs, -1.0f), fmaf((float)z, vs, -1.0f)};
    if (v[0] <= d.ab0[0] && v[1] <= d.ab0[1] && v[2] <= d.ab0[2] && (v[0] + vs) >= d.ab1[0] && (v[1] + vs) >= d.ab1[1] &&
        (v[2] + vs) >= d.ab1[2])
      return true;
    if (d.ab1[0] < v[0] || d.ab1[1] < v[1] || d.ab1[2] < v[2]) return false;
    if (d.ab0[0] > (v[0] + vs) || d.ab0[1] > (v[1] + vs) || d.ab0[2] > (v[2] + vs)) return false;
    const float p[3] = {v[0] - d.mean[0], v[1] - d.mean[1], v[2] - d.mean[2]};
    if (gs_face_test(p, d.cp[0], vs, 0, 1, 2, 0.0f) || gs_face_test(p, d.cp[0], vs, 0, 1, 2, vs) ||
        gs_face_test(p, d.cp[1], vs, 1, 0, 2, 0.0f) || gs_face_test(p, d.cp[1], vs, 1, 0, 2, vs) ||
        gs_face_test(p, d.cp[2], vs, 2, 0, 1, 0.0f) || gs_face_test(p, d.cp[2], vs, 2, 0, 1, vs))
      return true;
    const float* C = d.cov;
    for (int i = 0; i < 4; ++i) {
      const float o1 = (i >> 1) ? vs : 0.0f, o2 = (i & 1) ? vs : 0.0f;
      if (gs_edge_test(C[0], C[1], C[2], C[3], C[4], C[5], iso, p[1] + o1, p[2] + o2, p[0], p[0] + vs)) return true;
      if (gs_edge_test(C[3], C[1], C[4], C[0], C[2], C[5], iso, p[0] + o1, p[2] + o2, p[1], p[1] + vs)) return true;
      if (gs_edge_test(C[5], C[2], C[4], C[0], C[1], C[3], iso, p[0] + o1, p[1] + o2, p[2], p[2] + vs)) return true;
    }
    return false;
  }
};

// ---- finish: pack boundaries (bytes) and int16 points of the sorted pairs ------------------------------------------------------
__global__ __launch_bounds__(256) void gs_points_kernel(int64_t n, const int64_t* __restrict__ m, const int* __restrict__ flag,
                                                        short* __restrict__ points, unsigned char* __restrict__ boundary) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int x, y, z;
  ms_to_point((uint64_t)m[i], &x, &y, &z);
  points[i * 3] = (short)x;
  points[i * 3 + 1] = (short)y;
  points[i * 3 + 2] = (short)z;
  boundary[i] = flag[i] ? 1 : 0;
}

// workspace of kamd_gs_to_spc_finish for n pairs: keys A (n) | vals A (n) | keys B (n) | flag (n ints) | the sort's scratch
// (sort_scan_host.h): (digit, block) counts (ints), their offsets and scan sums
struct GsWs {
  int64_t *ka, *va, *kb;
  int* flag;
  SsSortWs sort;
  size_t total_bytes;
};
GsWs gs_ws(void* base, int64_t n) {
  GsWs w;
  char* p = (char*)base;
  auto take = [&](size_t bytes) {
    char* r = p;
    p += (bytes + 255) & ~(size_t)255;
    return r;
  };
  const size_t n1 = (size_t)(n > 0 ? n : 1);
  w.ka = (int64_t*)take(n1 * 8);
  w.va = (int64_t*)take(n1 * 8);
  w.kb = (int64_t*)take(n1 * 8);
  w.flag = (int*)take(n1 * 4);
  w.sort.hist = (int*)take(ss_sort_hist_entries(n) * 4);
  w.sort.offs = (long long*)take(ss_sort_offs_entries(n) * 8);
  w.sort.sums = (long long*)take(ss_sort_sums_entries(n) * 8);
  w.total_bytes = (size_t)(p - (char*)base);
  return w;
}

// ---- the integral (gs_to_spc_cuda.cu:719-770) ---------------------------------------------------------------------------------
// GS_LANES lanes per pair; lane k takes the (i, j) columns k, k + GS_LANES, ... of the step^2 and sums each over its `step` samples
// in order; partial sums meet in a fixed butterfly (xor 4, 2, 1), so every lane ends with the same bits.
constexpr int GS_LANES = 8;
__global__ __launch_bounds__(256) void gs_integrate_kernel(int64_t n, int64_t G, const short* __restrict__ points,
                                                           const int64_t* __restrict__ gaus_id, const float* __restrict__ means,
                                                           const float* __restrict__ cov, const float* __restrict__ opacities,
                                                           float voxel, int step, float* __restrict__ values) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i = gid / GS_LANES;
  const int k = (int)(gid % GS_LANES);
  int64_t g = -1;
  if (i < n) g = gaus_id[i];
  const bool on = g >= 0 && g < G;  // guard: a Gaussian id outside the tables integrates nothing (the pair's value is 0)
  double sum = 0.0, alpha = 0.0;
  if (on) {
    const float fx = (float)((double)(voxel * (float)points[i * 3]) - 1.0);
    const float fy = (float)((double)(voxel * (float)points[i * 3 + 1]) - 1.0);
    const float fz = (float)((double)(voxel * (float)points[i * 3 + 2]) - 1.0);
    const float mx = means[g * 3], my = means[g * 3 + 1], mz = means[g * 3 + 2];
    const double c0 = cov[g * 6], c1 = cov[g * 6 + 1], c2 = cov[g * 6 + 2], c3 = cov[g * 6 + 3], c4 = cov[g * 6 + 4],
                 c5 = cov[g * 6 + 5];
    alpha = (double)opacities[g];
    const float step_size = voxel / (float)((step > 1) ? step - 1 : 1);
    const int columns = step * step;
    for (int ij = k; ij < columns; ij += GS_LANES) {
      const int a = ij / step, b = ij - a * step;
      const double vx = (double)((fx + (float)a * step_size) - mx);
      const double vy = (double)((fy + (float)b * step_size) - my);
      const double inter = c0 * vx * vx + 2.0 * c1 * vx * vy + c3 * vy * vy;
      const double tx = 2.0 * c2 * vx, ty = 2.0 * c4 * vy;
      double col = 0.0;
      for (int c = 0; c < step; ++c) {
        const double vz = (double)((fz + (float)c * step_size) - mz);
        col += exp(-0.5 * (inter + tx * vz + ty * vz + c5 * vz * vz));
      }
      sum += col;
    }
  }
  sum += __shfl_xor(sum, 4, 64);
  sum += __shfl_xor(sum, 2, 64);
  sum += __shfl_xor(sum, 1, 64);
  if (i < n && k == 0) {
    const double cube = (double)((unsigned)step * (unsigned)step * (unsigned)step);
    values[i] = on ? (float)(alpha * sum / cube) : 0.0f;
  }
}

}  // namespace

extern "C" {

int kamd_gs_to_spc_stage_levels(void) { return GS_STAGE_LEVELS; }

size_t kamd_gs_to_spc_prepare_workspace(int64_t G) { return (size_t)(G > 0 ? G : 0) * GS_PREP * sizeof(float); }

int kamd_gs_to_spc_prepare(void* stream, int64_t G, const float* means3D, const float* scales, const float* rotations, float iso,
                           float tol, int level, float* cov3d_invs, void* prepared) {
  if (G <= 0) return 0;
  if (level < 0 || level > GS_MAX_LEVEL) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gs_prepare_kernel, dim3(kamd_cdiv(G, 256)), dim3(256), 0, st, G, means3D, scales, rotations, iso, tol, level,
                     cov3d_invs, (float*)prepared);
  KAMD_RETURN_LAST_ERROR();
}

size_t kamd_gs_to_spc_scan_workspace(int64_t n) { return ss_scan_sums_entries(n) * 8; }

int kamd_gs_to_spc_stage_count(void* stream, int64_t n, int64_t G, const float* means3D, const float* cov3d_invs,
                               const void* prepared, float iso, const int64_t* morton, const int64_t* gaus_id, int level_from,
                               int level_to, int tested, int32_t* counts, int64_t* offsets, void* scan_workspace) {
  if (n <= 0) return 0;
  if (level_from < 0 || level_to < level_from || level_to > GS_MAX_LEVEL || level_to - level_from > GS_STAGE_LEVELS)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const GsPrim prim = {G, means3D, cov3d_invs, (const float*)prepared, iso};
  hipLaunchKernelGGL((spc_stage_kernel<false, GsPrim>), dim3(kamd_cdiv(n * 8, 256)), dim3(256), 0, st, n, prim, morton, gaus_id,
                     level_from, level_to, tested, counts, (const int64_t*)nullptr, (int64_t)0, (int64_t*)nullptr,
                     (int64_t*)nullptr);
  return ss_scan(st, n, (const int64_t*)nullptr, counts, offsets, (int64_t*)scan_workspace);
}

int kamd_gs_to_spc_stage_emit(void* stream, int64_t n, int64_t G, const float* means3D, const float* cov3d_invs,
                              const void* prepared, float iso, const int64_t* morton, const int64_t* gaus_id, int level_from,
                              int level_to, int tested, const int64_t* offsets, int64_t total, int64_t* morton_out,
                              int64_t* gaus_id_out) {
  if (n <= 0 || total <= 0) return 0;
  if (level_from < 0 || level_to < level_from || level_to > GS_MAX_LEVEL || level_to - level_from > GS_STAGE_LEVELS)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const GsPrim prim = {G, means3D, cov3d_invs, (const float*)prepared, iso};
  hipLaunchKernelGGL((spc_stage_kernel<true, GsPrim>), dim3(kamd_cdiv(n * 8, 256)), dim3(256), 0, st, n, prim, morton, gaus_id,
                     level_from, level_to, tested, (int*)nullptr, offsets, total, morton_out, gaus_id_out);
  KAMD_RETURN_LAST_ERROR();
}

size_t kamd_gs_to_spc_finish_workspace(int64_t n) { return gs_ws(nullptr, n).total_bytes; }

// pairs ordered by (Gaussian, code) -> ordered by (code, Gaussian): points, gaus_id, pack_boundary (one byte per pair)
int kamd_gs_to_spc_finish(void* stream, int64_t n, int level, const int64_t* morton, const int64_t* gaus_id, void* workspace,
                          size_t workspace_bytes, int16_t* points, int64_t* gaus_id_out, uint8_t* pack_boundary) {
  if (n <= 0) return 0;
  if (level < 0 || level > GS_MAX_LEVEL) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const GsWs w = gs_ws(workspace, n);
  if (workspace == nullptr || workspace_bytes < w.total_bytes) return (int)hipErrorInvalidValue;
  KAMD_CHECK(ss_sort(st, n, ss_passes_low(3 * level), morton, gaus_id, w.ka, w.va, w.kb, gaus_id_out, w.sort));
  const unsigned g = (unsigned)kamd_cdiv(n, 256);
  KAMD_CHECK(ss_heads(st, n, (const int64_t*)nullptr, w.kb, 0, w.flag));
  hipLaunchKernelGGL(gs_points_kernel, dim3(g), dim3(256), 0, st, n, (const int64_t*)w.kb, (const int*)w.flag, (short*)points,
                     (unsigned char*)pack_boundary);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_integrate_gs(void* stream, int64_t n, int64_t G, const int16_t* points, const int64_t* gaus_id, const float* means3D,
                      const float* cov3d_invs, const float* opacities, int level, int step, float* values) {
  if (n <= 0) return 0;
  if (level < 0 || level > GS_MAX_LEVEL || step < 1 || step > 1024) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const float voxel = 2.0f / (float)(1 << level);
  hipLaunchKernelGGL(gs_integrate_kernel, dim3(kamd_cdiv(n * GS_LANES, 256)), dim3(256), 0, st, n, G, (const short*)points, gaus_id,
                     means3D, cov3d_invs, opacities, voxel, step, values);
  KAMD_RETURN_LAST_ERROR();
}

}  // extern "C"
