// ops.spc Bayesian-fusion reconstruction: the operators behind bf_recon (depth min/max pyramid, the per-level oracles, the final
// probabilities / colours / normals, subdivide / compactify, the bottom-up octree + empty assembly, the two-tree merges), the
// empty-aware query, and bf_cells: the cells of a level that the empty-aware query does not call empty, enumerated with work
// proportional to the output ("Bayesian fusion").
//
// Replaces kaolin/csrc/ops/spc/bf_cuda.cu, recon_cuda.cu, the `empty` kernel of query_cuda.cu and `identify` with empty of
// spc_utils.cuh.  One thread per point / node / pixel everywhere: the cost of a frame is launches and read-backs, not arithmetic.
// The arithmetic contract: float32, one rounding per operation in the order written here, no FMA (the Makefile builds
// with -ffp-contract=off), correctly rounded divide and square root, so that a numpy float32 restatement reproduces every output
// bit for bit.  No atomics.  Every data-derived index is compared with the size of the buffer it indexes before use.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <float.h>
#include "common.h"
#include "sort_scan.h"
#include "spc_octree.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr int BF_MAX_LEVEL = 15;
constexpr float BF_NEAR = 0.15f;  // the near plane, compared in float

struct BfMat {  // T = M * cam, row major, computed on the host
  float m[16];
};

inline unsigned bf_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

// the published profile curve (3DV 2016): nine cubic Bezier segments, ordinates b / 255
__constant__ float BF_CURVE[9][4] = {
    {0.0f / 255.0f, 0.0f / 255.0f, 0.0f / 255.0f, 2.0f / 255.0f},     {2.0f / 255.0f, 4.0f / 255.0f, 8.0f / 255.0f, 16.0f / 255.0f},
    {16.0f / 255.0f, 24.0f / 255.0f, 36.0f / 255.0f, 48.0f / 255.0f}, {48.0f / 255.0f, 60.0f / 255.0f, 72.0f / 255.0f, 79.0f / 255.0f},
    {79.0f / 255.0f, 86.0f / 255.0f, 88.0f / 255.0f, 86.0f / 255.0f}, {86.0f / 255.0f, 84.0f / 255.0f, 78.0f / 255.0f, 72.0f / 255.0f},
    {72.0f / 255.0f, 66.0f / 255.0f, 60.0f / 255.0f, 56.0f / 255.0f}, {56.0f / 255.0f, 52.0f / 255.0f, 50.0f / 255.0f, 49.0f / 255.0f},
    {49.0f / 255.0f, 48.0f / 255.0f, 48.0f / 255.0f, 48.0f / 255.0f}};

// u = x + 3 in (0, 9]: the segment (clamped to the table, as a clamped fetch would) and the parameter t = u - trunc(u)
__device__ __forceinline__ const float* bf_segment(float x, float* t, float* s) {
  const float u = x + 3.0f;
  const float iu = truncf(u);
  *t = u - iu;
  *s = 1.0f - *t;
  int i = (int)iu;
  i = i < 0 ? 0 : (i > 8 ? 8 : i);
  return BF_CURVE[i];
}
__device__ __forceinline__ float bf_profile(float x) {
  if (!(x > -3.0f)) return 0.0f;  // NaN too
  if (x >= 6.0f) return 0.5f;
  float t, s;
  const float* c = bf_segment(x, &t, &s);
  return 2.65625f * (s * s * (s * c[0] + (3.0f * t) * c[1]) + t * t * ((3.0f * s) * c[2] + t * c[3]));
}
__device__ __forceinline__ float bf_profile_derivative(float x) {
  if (!(x > -3.0f) || x >= 6.0f) return 0.0f;
  float t, s;
  const float* c = bf_segment(x, &t, &s);
  const float a0 = s * c[0] + t * c[1], a1 = s * c[1] + t * c[2], a2 = s * c[2] + t * c[3];
  const float b0 = s * a0 + t * a1, b1 = s * a1 + t * a2;
  return 7.96875f * (b1 - b0);  // 2.65625 * 3
}

// [x y z 1] * T, summed left to right
__device__ __forceinline__ void bf_origin(const BfMat& T, const int16_t* __restrict__ p, float O[4]) {
  const float x = (float)p[0], y = (float)p[1], z = (float)p[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) O[j] = ((x * T.m[j] + y * T.m[4 + j]) + z * T.m[8 + j]) + T.m[12 + j];
}
// corner i: O, + row 0 if i & 4, then + row 1 if i & 2, then + row 2 if i & 1 -> (x / z, y / z, z)
__device__ __forceinline__ void bf_corner(const BfMat& T, const float O[4], int i, float q[3]) {
  float P[3] = {O[0], O[1], O[2]};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (i & 4) P[j] = P[j] + T.m[j];
    if (i & 2) P[j] = P[j] + T.m[4 + j];
    if (i & 1) P[j] = P[j] + T.m[8 + j];
  }
  q[0] = P[0] / P[2];
  q[1] = P[1] / P[2];
  q[2] = P[2];
}

// ---- depth pyramid ----------------------------------------------------------------------------------------------------------------------
// one thread per 2 x 2 block of the depth map: converts ray length to z depth in place (true_depth), writes the finest level
__global__ __launch_bounds__(256) void bf_mip_first_kernel(int64_t num, int half_w, float fx, float fy, float cx, float cy,
                                                           float max_depth, int true_depth, float* __restrict__ img,
                                                           float2* __restrict__ mip) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= num) return;
  const int x = 2 * (int)(i % half_w), y = 2 * (int)(i / half_w);
  const int64_t w = 2 * (int64_t)half_w;
  float d[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int px = x + (k & 1), py = y + (k >> 1);
    float v = img[py * w + px];
    if (true_depth && v != max_depth) {
      const float u = ((float)px - cx) / fx, t = ((float)py - cy) / fy;
      v = v * (1.0f / sqrtf((u * u + t * t) + 1.0f));
      img[py * w + px] = v;
    }
    d[k] = v;
  }
  mip[i] = make_float2(fminf(fminf(d[0], d[2]), fminf(d[1], d[3])), fmaxf(fmaxf(d[0], d[2]), fmaxf(d[1], d[3])));
}
__global__ __launch_bounds__(256) void bf_mip_next_kernel(int64_t num, int width, const float2* __restrict__ in,
                                                          float2* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= num) return;
  const int64_t x = 2 * (i % width), y = 2 * (i / width), w = 2 * (int64_t)width;
  const float2 a = in[y * w + x], b = in[y * w + x + 1], c = in[(y + 1) * w + x], e = in[(y + 1) * w + x + 1];
  out[i] = make_float2(fminf(fminf(a.x, c.x), fminf(b.x, e.x)), fmaxf(fmaxf(a.y, c.y), fmaxf(b.y, e.y)));
}

// ---- the per-level oracle -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bf_oracle_kernel(int64_t n, const int16_t* __restrict__ points, BfMat T, float sigma,
                                                        const float* __restrict__ depth, int h, int w, int mip_levels,
                                                        const float2* __restrict__ mip, int64_t mip_size, int64_t hw,
                                                        int* __restrict__ occ, int* __restrict__ state) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float O[4], lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  bf_origin(T, points + 3 * i, O);
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float q[3];
    bf_corner(T, O, c, q);
#pragma unroll
    for (int j = 0; j < 3; ++j) lo[j] = fminf(lo[j], q[j]), hi[j] = fmaxf(hi[j], q[j]);
  }
  const float fw = (float)w, fh = (float)h;
  int keep = 1, st = 2;  // straddling the border, too high up the pyramid or an index out of range: keep and split
  // (a coordinate that is NaN at every corner leaves lo = FLT_MAX > hi = -FLT_MAX: no extent to test, the voxel is kept)
  const bool ordered = lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2];
  if (!ordered) {
  } else if (lo[0] >= 0.0f && hi[0] < fw && lo[1] >= 0.0f && hi[1] < fh && lo[2] > BF_NEAR) {
    const float extent = fmaxf(hi[0] - lo[0], hi[1] - lo[1]);
    int m = 0;  // the smallest m with 2^m >= extent, by exact comparison
    while (m <= mip_levels && ldexpf(1.0f, m) < extent) ++m;
    if (m <= mip_levels) {
      const float inv = ldexpf(1.0f, -m);
      const int64_t xmin = (int64_t)(inv * lo[0]), ymin = (int64_t)(inv * lo[1]);
      const int64_t xmax = (int64_t)(inv * hi[0]), ymax = (int64_t)(inv * hi[1]);
      const int64_t stride = w >> m, rows = h >> m;
      if (xmin >= 0 && xmin <= xmax && xmax < stride && ymin >= 0 && ymin <= ymax && ymax < rows) {  // all four pixel indices
        float z0, z1;
        bool ok = true;
        if (m > 0) {
          const int64_t off = hw * (((int64_t)1 << (2 * (mip_levels - m))) - 1) / 3;
          ok = off >= 0 && off + rows * stride <= mip_size;
          if (ok) {
            const float2* D = mip + off;
            const float2 a = D[ymin * stride + xmin], b = D[ymin * stride + xmax], c = D[ymax * stride + xmin],
                         e = D[ymax * stride + xmax];
            z0 = fminf(fminf(a.x, b.x), fminf(c.x, e.x)) - sigma;
            z1 = fmaxf(fmaxf(a.y, b.y), fmaxf(c.y, e.y)) + 2.0f * sigma;
          }
        } else {
          const float a = depth[ymin * stride + xmin], b = depth[ymin * stride + xmax], c = depth[ymax * stride + xmin],
                      e = depth[ymax * stride + xmax];
          z0 = fminf(fminf(a, b), fminf(c, e)) - sigma;
          z1 = fmaxf(fmaxf(a, b), fmaxf(c, e)) + 2.0f * sigma;
        }
        if (ok) {
          keep = (z0 <= hi[2] && lo[2] <= z1) ? 1 : 0;
          st = z0 > hi[2] ? 0 : (z1 < lo[2] ? 1 : 2);
        }
      }
    }
  } else if (hi[0] < 0.0f || lo[0] > fw || hi[1] < 0.0f || lo[1] > fh || hi[2] < BF_NEAR) {
    keep = 0, st = 1;  // wholly outside the view: unseen
  }
  occ[i] = keep;
  state[i] = st;
}

__global__ __launch_bounds__(256) void bf_fill_kernel(int64_t n, int a, int b, int* __restrict__ occ, int* __restrict__ state) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) occ[i] = a, state[i] = b;
}

__global__ __launch_bounds__(256) void bf_oracle_final_kernel(int64_t n, const int16_t* __restrict__ points, BfMat T, float scale,
                                                              const float* __restrict__ depth, int h, int w, int* __restrict__ occ,
                                                              int* __restrict__ state, float* __restrict__ probs) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float O[4];
  bf_origin(T, points + 3 * i, O);
  const float fw = (float)w, fh = (float)h;
  float pmin = 1.0f, pmax = -1.0f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float q[3];
    bf_corner(T, O, c, q);
    float prob = 0.5f;
    if (q[0] >= 0.0f && q[0] < fw && q[1] >= 0.0f && q[1] < fh && q[2] > BF_NEAR) {
      const int64_t x = (int64_t)q[0], y = (int64_t)q[1];  // 0 <= x < w, 0 <= y < h by the comparisons above
      prob = bf_profile(scale * (q[2] - depth[y * w + x]));
    }
    pmin = fminf(pmin, prob);
    pmax = fmaxf(pmax, prob);
    if (c == 0) probs[i] = prob;
  }
  const bool empty = pmax == 0.0f, unseen = pmin == 0.5f && pmax == 0.5f;
  occ[i] = (empty || unseen) ? 0 : 1;
  state[i] = empty ? 0 : (unseen ? 1 : 2);
}

__device__ __forceinline__ unsigned bf_to_byte(float v) {  // truncation, saturated to [0, 255]; NaN -> 0
  if (!(v > 0.0f)) return 0u;
  return v >= 255.0f ? 255u : (unsigned)v;
}

__global__ __launch_bounds__(256) void bf_colors_final_kernel(int64_t n, const int16_t* __restrict__ points, BfMat T, float scale,
                                                              const float* __restrict__ image, const float* __restrict__ depth,
                                                              int h, int w, const float* __restrict__ probs,
                                                              unsigned char* __restrict__ colors, float* __restrict__ normals) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float Q[4];
  bf_origin(T, points + 3 * i, Q);
  const float qx = Q[0] / Q[2], qy = Q[1] / Q[2];
  uchar4 col = make_uchar4(64, 64, 64, 64);
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  // the pixel has all four neighbours: 1 <= x <= w - 2, 1 <= y <= h - 2
  if (qx >= 1.0f && qx < (float)(w - 1) && qy >= 1.0f && qy < (float)(h - 1) && Q[2] > BF_NEAR) {
    const int64_t x = (int64_t)qx, y = (int64_t)qy;
    const float prob = probs[i];
    if (prob == 0.0f) {
      col = make_uchar4(0, 0, 0, 0);
    } else if (prob != 0.5f) {
      const float* c = image + 3 * (y * w + x);
      col = make_uchar4((unsigned char)bf_to_byte(255.0f * c[2]), (unsigned char)bf_to_byte(255.0f * c[1]),
                        (unsigned char)bf_to_byte(255.0f * c[0]), 0);
      const float d00 = depth[y * w + x];
      const float du = 0.5f * (depth[y * w + x + 1] - depth[y * w + x - 1]);
      const float dv = 0.5f * (depth[(y + 1) * w + x] - depth[(y - 1) * w + x]);
      const float dprob = bf_profile_derivative(scale * (Q[2] - d00));
      const float zi = 1.0f / Q[2];
      const float wgt = (scale * dprob) * zi;
      const float hz = (wgt * zi) * ((Q[2] * Q[2] + Q[0] * du) + Q[1] * dv);
      const float hx = (-wgt) * du, hy = (-wgt) * dv;
      const float gx = (T.m[0] * hx + T.m[1] * hy) + T.m[2] * hz;
      const float gy = (T.m[4] * hx + T.m[5] * hy) + T.m[6] * hz;
      const float gz = (T.m[8] * hx + T.m[9] * hy) + T.m[10] * hz;
      const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
      const float ax = gx / len, ay = gy / len, az = gz / len;
      if (isfinite(ax) && isfinite(ay) && isfinite(az)) nx = ax, ny = ay, nz = az;  // (the reference leaves NaN)
    }
  }
  reinterpret_cast<uchar4*>(colors)[i] = col;
  normals[3 * i] = nx, normals[3 * i + 1] = ny, normals[3 * i + 2] = nz;
}

// ---- subdivide / compactify ---------------------------------------------------------------------------------------------------------------
template <bool SUBDIVIDE, typename Idx>
__global__ __launch_bounds__(256) void bf_compact_kernel(int64_t n, int64_t pass, const int16_t* __restrict__ in,
                                                         const int* __restrict__ insum, int16_t* __restrict__ out,
                                                         Idx* __restrict__ nvsum) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t slot = i == 0 ? 0 : insum[i - 1];
  if (slot == insum[i] || slot < 0 || slot >= pass) return;  // the scan-derived slot
  nvsum[slot] = (Idx)i;
  const int x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
  if (SUBDIVIDE) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      int16_t* o = out + 3 * (8 * slot + c);
      o[0] = (int16_t)(2 * x + (c >> 2)), o[1] = (int16_t)(2 * y + ((c >> 1) & 1)), o[2] = (int16_t)(2 * z + (c & 1));
    }
  } else {
    int16_t* o = out + 3 * slot;
    o[0] = (int16_t)x, o[1] = (int16_t)y, o[2] = (int16_t)z;
  }
}

// ---- bottom-up assembly ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bf_final_voxels_kernel(int64_t num_nodes, const int* __restrict__ state,
                                                              const int* __restrict__ nvsum, int64_t prev_size,
                                                              int* __restrict__ occ, int* __restrict__ prev_state,
                                                              unsigned char* __restrict__ octree, unsigned char* __restrict__ empty) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= num_nodes) return;
  unsigned o = 0, e = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int s = state[8 * i + c];
    if (s == 2) o |= 1u << c, e |= 1u << c;
    if (s == 1) e |= 1u << c;
  }
  const int64_t up = nvsum[i];
  if (up >= 0 && up < prev_size) prev_state[up] = o ? 2 : (e ? 1 : 0);
  occ[i] = o ? 1 : 0;
  octree[i] = (unsigned char)o;
  empty[i] = (unsigned char)e;
}
__global__ __launch_bounds__(256) void bf_compact_nodes_kernel(int64_t n, int64_t pass, const int* __restrict__ insum,
                                                               const unsigned char* __restrict__ in_o,
                                                               const unsigned char* __restrict__ in_e, unsigned char* __restrict__ out_o,
                                                               unsigned char* __restrict__ out_e) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t slot = i == 0 ? 0 : insum[i - 1];
  if (slot == insum[i] || slot < 0 || slot >= pass) return;
  out_o[slot] = in_o[i];
  out_e[slot] = in_e[i];
}

// ---- the empty-aware walk -------------------------------------------------------------------------------------------------------------------
// >= 0: the point's index; -1: empty space, outside the cube, or an index that leaves the buffers; -2 - depth: unseen, `depth`
// levels left below the node at which the walk stopped
__device__ __forceinline__ int bf_identify(int x, int y, int z, int level, int64_t num_bytes, const unsigned char* __restrict__ octree,
                                           const unsigned char* __restrict__ empty, const int* __restrict__ exsum) {
  const int maxval = (1 << level) - 1;
  if (x < 0 || y < 0 || z < 0 || x > maxval || y > maxval || z > maxval) return -1;
  int64_t ord = 0;
  for (int l = 0; l < level; ++l) {
    const int depth = level - l - 1;
    const unsigned child = (unsigned)((((x >> depth) & 1) << 2) | (((y >> depth) & 1) << 1) | ((z >> depth) & 1));
    if (ord < 0 || ord >= num_bytes) return -1;  // octree, empty and exsum all have num_bytes entries
    const unsigned bits = octree[ord];
    if (!((bits >> child) & 1u)) return ((empty[ord] >> child) & 1u) ? -2 - depth : -1;
    ord = (ord == 0 ? 0 : (int64_t)exsum[ord - 1]) + __popc(bits & ((2u << child) - 1u));
  }
  return (int)ord;
}

__global__ __launch_bounds__(256) void bf_merge_empty_kernel(int64_t n, const int16_t* __restrict__ p, int level, int64_t nb0,
                                                             int64_t nb1, const unsigned char* __restrict__ o0,
                                                             const unsigned char* __restrict__ o1, const unsigned char* __restrict__ e0,
                                                             const unsigned char* __restrict__ e1, const int* __restrict__ x0,
                                                             const int* __restrict__ x1, int* __restrict__ occ, int* __restrict__ state) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int a = bf_identify(p[3 * i], p[3 * i + 1], p[3 * i + 2], level, nb0, o0, e0, x0);
  const int b = bf_identify(p[3 * i], p[3 * i + 1], p[3 * i + 2], level, nb1, o1, e1, x1);
  const bool empty = a == -1 || b == -1, unseen = a < -1 && b < -1;
  occ[i] = (empty || unseen) ? 0 : 1;
  state[i] = empty ? 0 : (unseen ? 1 : 2);
}

struct BfTree {
  const unsigned char *octree, *empty;
  const int* exsum;
  const float* probs;
  const unsigned char* colors;
  int64_t num_bytes, offset, rows;
};
__global__ __launch_bounds__(256) void bf_merge_kernel(int64_t n, const int16_t* __restrict__ p, int level, BfTree A, BfTree B,
                                                       int* __restrict__ occ, int* __restrict__ state, float* __restrict__ probs,
                                                       unsigned char* __restrict__ colors) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int a = bf_identify(p[3 * i], p[3 * i + 1], p[3 * i + 2], level, A.num_bytes, A.octree, A.empty, A.exsum);
  const int b = bf_identify(p[3 * i], p[3 * i + 1], p[3 * i + 2], level, B.num_bytes, B.octree, B.empty, B.exsum);
  const int64_t ra = (int64_t)a - A.offset, rb = (int64_t)b - B.offset;  // the rows of probs / colors
  const bool ina = a >= 0 && ra >= 0 && ra < A.rows, inb = b >= 0 && rb >= 0 && rb < B.rows;
  const bool empty = a == -1 || b == -1 || (a >= 0 && !ina) || (b >= 0 && !inb), unseen = a < -1 && b < -1;
  int o = 0, s = empty ? 0 : 1;
  float pr = 0.0f;
  uchar4 col = make_uchar4(0, 0, 0, 0);
  if (!empty && !unseen) {
    const float p0 = ina ? A.probs[ra] : 0.5f, p1 = inb ? B.probs[rb] : 0.5f;
    pr = (p0 * p1) / (p0 * p1 + (1.0f - p0) * (1.0f - p1));
    col = ina ? reinterpret_cast<const uchar4*>(A.colors)[ra] : reinterpret_cast<const uchar4*>(B.colors)[rb];
    o = 1, s = 2;
  }
  occ[i] = o;
  state[i] = s;
  probs[i] = pr;
  reinterpret_cast<uchar4*>(colors)[i] = col;
}

__device__ __forceinline__ double bf_load(const __half* p, int64_t i) { return (double)__half2float(p[i]); }
__device__ __forceinline__ double bf_load(const float* p, int64_t i) { return (double)p[i]; }
__device__ __forceinline__ double bf_load(const double* p, int64_t i) { return p[i]; }
// floor(2^level * (q * 0.5 + 0.5)) in double for every coordinate type; a value no int16 holds (NaN included) is outside
template <typename T>
__global__ __launch_bounds__(256) void bf_query_kernel(int64_t Q, int level, int64_t num_bytes, const unsigned char* __restrict__ octree,
                                                       const unsigned char* __restrict__ empty, const int* __restrict__ exsum,
                                                       const T* __restrict__ coords, int* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Q) return;
  int k[3];
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double v = floor((double)(1 << level) * (bf_load(coords, 3 * i + c) * 0.5 + 0.5));
    ok = ok && (v >= -32768.0 && v <= 32767.0);
    k[c] = ok ? (int)v : -1;
  }
  out[i] = ok ? bf_identify(k[0], k[1], k[2], level, num_bytes, octree, empty, exsum) : -1;
}

// ---- bf_cells: the cells the empty-aware query does not call empty, in Morton order ------------------------------------------------------
// header (int64): [0 .. 16] first byte of every level, [17] K = cells below the root, [18] bytes the levels account for
constexpr int BF_HDR = 24;
__global__ void bf_cells_levels_kernel(int level, int64_t num_bytes, const int* __restrict__ exsum, int64_t* __restrict__ hdr) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t start = 0, count = num_bytes > 0 ? 1 : 0;
  for (int l = 0; l <= BF_MAX_LEVEL + 1; ++l) {
    hdr[l] = start;
    if (l >= level) continue;
    int64_t end = start + count;
    if (end > num_bytes) end = num_bytes;
    const int64_t below = (end > 0 ? (int64_t)exsum[end - 1] : 0) - (start > 0 ? (int64_t)exsum[start - 1] : 0);  // the set bits of level l
    start = end;
    count = below;
  }
  hdr[18] = hdr[level];
}
__device__ __forceinline__ int64_t bf_cells_of_bit(unsigned bits, unsigned mpty, int c, int64_t node, int depth_left, int64_t num_bytes,
                                                   const int* __restrict__ exsum, const int64_t* __restrict__ sub) {
  if ((bits >> c) & 1u) {
    if (depth_left == 0) return 1;
    const int64_t child = (node == 0 ? 0 : (int64_t)exsum[node - 1]) + __popc(bits & ((2u << c) - 1u));
    return (child > node && child < num_bytes) ? sub[child] : 0;  // a child lies after its parent
  }
  return ((mpty >> c) & 1u) ? ((int64_t)1 << (3 * depth_left)) : 0;
}
// level d of the tree (d = level - 1 first): sub[node] = the cells below the node
__global__ __launch_bounds__(256) void bf_cells_count_kernel(int d, int level, int64_t num_bytes, const unsigned char* __restrict__ octree,
                                                             const unsigned char* __restrict__ empty, const int* __restrict__ exsum,
                                                             int64_t* __restrict__ hdr, int64_t* __restrict__ sub) {
  const int64_t first = hdr[d], last = hdr[d + 1] < num_bytes ? hdr[d + 1] : num_bytes;
  for (int64_t node = first + (int64_t)blockIdx.x * 256 + threadIdx.x; node < last; node += (int64_t)gridDim.x * 256) {
    const unsigned bits = octree[node], mpty = empty[node];
    int64_t total = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) total += bf_cells_of_bit(bits, mpty, c, node, level - 1 - d, num_bytes, exsum, sub);
    sub[node] = total;
    if (node == 0) hdr[17] = total;
  }
}
// one thread per output cell: the walk from the root that skips whole subtrees by their counts
__global__ __launch_bounds__(256) void bf_cells_emit_kernel(int64_t K, int level, int64_t num_bytes, const unsigned char* __restrict__ octree,
                                                            const unsigned char* __restrict__ empty, const int* __restrict__ exsum,
                                                            const int64_t* __restrict__ sub, int16_t* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= K) return;
  int64_t rem = j, node = 0;
  uint64_t code = 0;
  bool found = false;
  for (int d = 0; d < level && !found; ++d) {
    if (node < 0 || node >= num_bytes) break;
    const unsigned bits = octree[node], mpty = empty[node];
    const int left = level - 1 - d;
    int c = 0;
    int64_t cnt = 0;
    for (; c < 8; ++c) {
      cnt = bf_cells_of_bit(bits, mpty, c, node, left, num_bytes, exsum, sub);
      if (rem < cnt) break;
      rem -= cnt;
    }
    if (c == 8) break;  // (the counts and the tree disagree: leave the row zero)
    code = (code << 3) | (uint64_t)c;
    if ((bits >> c) & 1u) {
      if (left == 0) found = true;
      node = (node == 0 ? 0 : (int64_t)exsum[node - 1]) + __popc(bits & ((2u << c) - 1u));
    } else {  // inside an unseen block: the remainder is the cell's Morton code within it
      code = (code << (3 * left)) | (uint64_t)rem;
      found = true;
    }
  }
  int x = 0, y = 0, z = 0;
  if (found) ms_to_point(code, &x, &y, &z);
  out[3 * j] = (int16_t)x, out[3 * j + 1] = (int16_t)y, out[3 * j + 2] = (int16_t)z;
}

template <typename T>
int bf_query(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree, const uint8_t* empty, const int32_t* exsum,
             const void* coords, int32_t* out) {
  if (level < 0 || level > BF_MAX_LEVEL || num_bytes < 0) return (int)hipErrorInvalidValue;
  if (Q <= 0) return 0;
  hipLaunchKernelGGL((bf_query_kernel<T>), dim3(bf_blocks(Q)), dim3(256), 0, (hipStream_t)stream, Q, level, num_bytes, octree, empty,
                     exsum, (const T*)coords, out);
  KAMD_RETURN_LAST_ERROR();
}

BfMat bf_mat(const float* T16) {
  BfMat T;
  for (int k = 0; k < 16; ++k) T.m[k] = T16[k];
  return T;
}

}  // namespace

extern "C" {

int64_t kamd_spc_bf_mip_size(int h, int w, int mip_levels) {
  if (h <= 0 || w <= 0 || mip_levels < 1 || mip_levels > 15) return -1;
  const int s = 1 << mip_levels;
  if (h % s || w % s) return -1;
  return (int64_t)(h / s) * (w / s) * ((((int64_t)1 << (2 * mip_levels)) - 1) / 3);
}

int kamd_spc_bf_build_mip2d(void* stream, int h, int w, int mip_levels, float fx, float fy, float cx, float cy, float max_depth,
                            int true_depth, float* depth, float* mip) {
  if (kamd_spc_bf_mip_size(h, w, mip_levels) < 0) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int64_t hw = (int64_t)(h >> mip_levels) * (w >> mip_levels);
  float2* M = reinterpret_cast<float2*>(mip);
  int width = w / 2;
  int64_t num = hw << (2 * (mip_levels - 1));
  hipLaunchKernelGGL(bf_mip_first_kernel, dim3(bf_blocks(num)), dim3(256), 0, st, num, width, fx, fy, cx, cy, max_depth, true_depth,
                     depth, M + hw * ((((int64_t)1 << (2 * (mip_levels - 1))) - 1) / 3));
  for (int l = mip_levels - 2; l >= 0; --l) {
    width /= 2;
    num = hw << (2 * l);
    hipLaunchKernelGGL(bf_mip_next_kernel, dim3(bf_blocks(num)), dim3(256), 0, st, num, width,
                       (const float2*)(M + hw * ((((int64_t)1 << (2 * (l + 1))) - 1) / 3)), M + hw * ((((int64_t)1 << (2 * l)) - 1) / 3));
  }
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spc_bf_oracle(void* stream, int64_t n, const int16_t* points, int level, const float* T16, float sigma, const float* depth,
                       int h, int w, int mip_levels, const float* mip, int32_t* occupancy, int32_t* state) {
  const int64_t size = kamd_spc_bf_mip_size(h, w, mip_levels);
  if (size < 0 || level < 0 || level > BF_MAX_LEVEL || T16 == nullptr) return (int)hipErrorInvalidValue;
  if (n <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (level == 0)
    hipLaunchKernelGGL(bf_fill_kernel, dim3(bf_blocks(n)), dim3(256), 0, st, n, 1, 2, occupancy, state);
  else
    hipLaunchKernelGGL(bf_oracle_kernel, dim3(bf_blocks(n)), dim3(256), 0, st, n, points, bf_mat(T16), sigma, depth, h, w, mip_levels,
                       reinterpret_cast<const float2*>(mip), size, (int64_t)(h >> mip_levels) * (w >> mip_levels), occupancy, state);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spc_bf_oracle_final(void* stream, int64_t n, const int16_t* points, int level, const float* T16, float sigma,
                             const float* depth, int h, int w, int32_t* occupancy, int32_t* state, float* probabilities) {
  if (level < 0 || level > BF_MAX_LEVEL || T16 == nullptr || h <= 0 || w <= 0 || sigma == 0.0f) return (int)hipErrorInvalidValue;
  if (n <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (level == 0) {
    KAMD_CHECK(kamd_zero_async(probabilities, (size_t)n * sizeof(float), st));
    hipLaunchKernelGGL(bf_fill_kernel, dim3(bf_blocks(n)), dim3(256), 0, st, n, 1, 2, occupancy, state);
  } else {
    hipLaunchKernelGGL(bf_oracle_final_kernel, dim3(bf_blocks(n)), dim3(256), 0, st, n, points, bf_mat(T16), 3.0f / sigma, depth, h, w,
                       occupancy, state, probabilities);
  }
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spc_bf_colors_final(void* stream, int64_t n, const int16_t* points, const float* T16, float sigma, const float* image,
                             const float* depth, int h, int w, const float* probabilities, uint8_t* colors, float* normals) {
  if (T16 == nullptr || h <= 0 || w <= 0 || !(sigma > 0.0f)) return (int)hipErrorInvalidValue;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(bf_colors_final_kernel, dim3(bf_blocks(n)), dim3(256), 0, (hipStream_t)stream, n, points, bf_mat(T16), 1.0f / sigma,
                     image, depth, h, w, probabilities, colors, normals);
  KAMD_RETURN_LAST_ERROR();
}

size_t kamd_spc_bf_scan_workspace(int64_t n) { return n > 0 ? ss_scan_sums_entries(n) * 8 : 0; }

int kamd_spc_bf_inclusive_sum(void* stream, int64_t n, const int32_t* in, int32_t* out, void* workspace) {
  if (n <= 0) return 0;
  if (workspace == nullptr) return (int)hipErrorInvalidValue;
  return ss_scan_inclusive((hipStream_t)stream, n, in, out, (int64_t*)workspace);
}

int kamd_spc_bf_subdivide(void* stream, int64_t n, int64_t pass, const int16_t* points, const int32_t* insum, int16_t* new_points,
                          int32_t* nvsum) {
  if (n <= 0 || pass <= 0) return 0;
  hipLaunchKernelGGL((bf_compact_kernel<true, int>), dim3(bf_blocks(n)), dim3(256), 0, (hipStream_t)stream, n, pass, points, insum,
                     new_points, nvsum);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spc_bf_compactify(void* stream, int64_t n, int64_t pass, const int16_t* points, const int32_t* insum, int16_t* new_points,
                           int64_t* nvsum) {
  if (n <= 0 || pass <= 0) return 0;
  hipLaunchKernelGGL((bf_compact_kernel<false, int64_t>), dim3(bf_blocks(n)), dim3(256), 0, (hipStream_t)stream, n, pass, points, insum,
                     new_points, nvsum);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spc_bf_process_final_voxels(void* stream, int64_t num_nodes, const int32_t* state, const int32_t* nvsum, int64_t prev_size,
                                     int32_t* occupancies, int32_t* prev_state, uint8_t* octree, uint8_t* empty) {
  if (num_nodes <= 0) return 0;
  hipLaunchKernelGGL(bf_final_voxels_kernel, dim3(bf_blocks(num_nodes)), dim3(256), 0, (hipStream_t)stream, num_nodes, state, nvsum,
                     prev_size, occupancies, prev_state, octree, empty);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spc_bf_compactify_nodes(void* stream, int64_t n, int64_t pass, const int32_t* insum, const uint8_t* octree, const uint8_t* empty,
                                 uint8_t* new_octree, uint8_t* new_empty) {
  if (n <= 0 || pass <= 0) return 0;
  hipLaunchKernelGGL(bf_compact_nodes_kernel, dim3(bf_blocks(n)), dim3(256), 0, (hipStream_t)stream, n, pass, insum, octree, empty,
                     new_octree, new_empty);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spc_bf_merge_empty(void* stream, int64_t n, const int16_t* points, int level, int64_t num_bytes0, int64_t num_bytes1,
                            const uint8_t* octree0, const uint8_t* octree1, const uint8_t* empty0, const uint8_t* empty1,
                            const int32_t* exsum0, const int32_t* exsum1, int32_t* occupancy, int32_t* state) {
  if (level < 0 || level > BF_MAX_LEVEL || num_bytes0 < 0 || num_bytes1 < 0) return (int)hipErrorInvalidValue;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(bf_merge_empty_kernel, dim3(bf_blocks(n)), dim3(256), 0, (hipStream_t)stream, n, points, level, num_bytes0,
                     num_bytes1, octree0, octree1, empty0, empty1, exsum0, exsum1, occupancy, state);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spc_bf_merge(void* stream, int64_t n, const int16_t* points, int level, int64_t num_bytes0, int64_t num_bytes1,
                      const uint8_t* octree0, const uint8_t* octree1, const uint8_t* empty0, const uint8_t* empty1, const int32_t* exsum0,
                      const int32_t* exsum1, int64_t offset0, int64_t offset1, int64_t rows0, int64_t rows1, const float* probs0,
                      const float* probs1, const uint8_t* colors0, const uint8_t* colors1, int32_t* occupancy, int32_t* state,
                      float* probabilities, uint8_t* colors) {
  if (level < 0 || level > BF_MAX_LEVEL || num_bytes0 < 0 || num_bytes1 < 0 || rows0 < 0 || rows1 < 0) return (int)hipErrorInvalidValue;
  if (n <= 0) return 0;
  const BfTree A{octree0, empty0, exsum0, probs0, colors0, num_bytes0, offset0, rows0};
  const BfTree B{octree1, empty1, exsum1, probs1, colors1, num_bytes1, offset1, rows1};
  hipLaunchKernelGGL(bf_merge_kernel, dim3(bf_blocks(n)), dim3(256), 0, (hipStream_t)stream, n, points, level, A, B, occupancy, state,
                     probabilities, colors);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_spc_bf_query_f16(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree, const uint8_t* empty,
                          const int32_t* exsum, const void* coords, int32_t* out) {
  return bf_query<__half>(stream, Q, level, num_bytes, octree, empty, exsum, coords, out);
}
int kamd_spc_bf_query_f32(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree, const uint8_t* empty,
                          const int32_t* exsum, const float* coords, int32_t* out) {
  return bf_query<float>(stream, Q, level, num_bytes, octree, empty, exsum, coords, out);
}
int kamd_spc_bf_query_f64(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree, const uint8_t* empty,
                          const int32_t* exsum, const double* coords, int32_t* out) {
  return bf_query<double>(stream, Q, level, num_bytes, octree, empty, exsum, coords, out);
}

struct BfCellsWs {
  int64_t *hdr, *sums, *sub;
  int* exsum;
  size_t total_bytes;
};
static BfCellsWs bf_cells_ws(void* base, int64_t num_bytes) {
  BfCellsWs w;
  char* p = (char*)base;
  auto take = [&](size_t bytes) {
    char* r = p;
    p += (bytes + 255) & ~(size_t)255;
    return r;
  };
  const size_t nn = (size_t)(num_bytes > 0 ? num_bytes : 1);
  w.hdr = (int64_t*)take(BF_HDR * 8);
  w.sums = (int64_t*)take(ss_scan_sums_entries((long long)nn) * 8);
  w.exsum = (int*)take(nn * 4);
  w.sub = (int64_t*)take(nn * 8);
  w.total_bytes = (size_t)(p - (char*)base);
  return w;
}

size_t kamd_spc_bf_cells_workspace(int64_t num_bytes) { return num_bytes > 0 ? bf_cells_ws(nullptr, num_bytes).total_bytes : 0; }

// counts the cells: host2 receives {K, the bytes that `level` levels of the tree account for}; the one host read of bf_cells
int kamd_spc_bf_cells_count(void* stream, int64_t num_bytes, int level, const uint8_t* octree, const uint8_t* empty, void* workspace,
                            int64_t* host2) {
  if (num_bytes <= 0 || level < 1 || level > BF_MAX_LEVEL || num_bytes * 8 >= (1LL << 31) || workspace == nullptr || host2 == nullptr)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const BfCellsWs w = bf_cells_ws(workspace, num_bytes);
  KAMD_CHECK(ss_scan_inclusive(st, num_bytes, octree, w.exsum, w.sums));
  hipLaunchKernelGGL(bf_cells_levels_kernel, dim3(1), dim3(64), 0, st, level, num_bytes, (const int*)w.exsum, w.hdr);
  unsigned g = bf_blocks(num_bytes);
  if (g > KAMD_NUM_CU * 16u) g = KAMD_NUM_CU * 16u;
  for (int d = level - 1; d >= 0; --d)  // the level sizes stay on the device: every launch is sized by the bound num_bytes
    hipLaunchKernelGGL(bf_cells_count_kernel, dim3(g), dim3(256), 0, st, d, level, num_bytes, octree, empty, (const int*)w.exsum, w.hdr,
                       w.sub);
  KAMD_CHECK(hipGetLastError());
  KAMD_CHECK(hipMemcpyAsync(host2, w.hdr + 17, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  KAMD_CHECK(hipStreamSynchronize(st));
  return 0;
}

int kamd_spc_bf_cells_emit(void* stream, int64_t num_bytes, int level, const uint8_t* octree, const uint8_t* empty, const void* workspace,
                           int64_t K, int16_t* cells) {
  if (num_bytes <= 0 || level < 1 || level > BF_MAX_LEVEL || workspace == nullptr) return (int)hipErrorInvalidValue;
  if (K <= 0) return 0;
  if ((K + 255) / 256 > 0x7FFFFFFFLL) return (int)hipErrorInvalidValue;
  const BfCellsWs w = bf_cells_ws(const_cast<void*>(workspace), num_bytes);
  hipLaunchKernelGGL(bf_cells_emit_kernel, dim3(bf_blocks(K)), dim3(256), 0, (hipStream_t)stream, K, level, num_bytes, octree, empty,
                     (const int*)w.exsum, (const int64_t*)w.sub, cells);
  KAMD_RETURN_LAST_ERROR();
}

}  // extern "C"
