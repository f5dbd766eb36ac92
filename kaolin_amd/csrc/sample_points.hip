// ops.mesh face_areas / sample_points (kaolin/ops/mesh/trianglemesh.py:30-311) as a short pipeline; the reference runs about twenty
// small torch launches per call (three index_select, a Categorical with its validation reads, multinomial, three gather, two rand,
// the blend).  The contract (DESIGN.md "ops.mesh.sample_points"):
//   * areas: x = v0 - v1, y = v1 - v2, a = (x2 y3 - x3 y2)^2, b = (x3 y1 - x1 y3)^2, c = (x1 y2 - x2 y1)^2, sqrt((a + b) + c) 0.5, one
//     rounding per operation (-ffp-contract=off) and a correctly rounded square root: the bits of the torch expression on the CPU;
//   * cdf: the inclusive float64 sum of an item's areas in a FIXED order (sp_cdf_*: a tile of SP_SCAN_TILE areas per workgroup, every
//     thread SP_SCAN_PER_THREAD consecutive ones in sequence; one workgroup per item scans the tiles' totals; an add pass -- three
//     plain launches, no look-back, no flag, no workgroup waits for another);
//   * face choice: total = cdf[last], t = min(r total, nextbelow(total)), the first face of the item with cdf[f] > t: ten steps of the
//     search in a coarse table of the item's cdf in LDS, the rest in global memory.  A fixed-order parallel sum is not monotone to the
//     last bit, so a face whose area is not positive is never returned: the search moves on to the nearest face with area > 0;
//   * points / features: u = sqrt(uv0), w0 = 1 - u, w1 = u (1 - uv1), w2 = u uv1, (w0 v0 + w1 v1) + w2 v2, one rounding each;
//   * an item whose total is not a positive finite number: NaN points and features, the item's first face as the choice.
// Items: batched (items == nullptr) item b is faces [0, F) of `faces`, vertices b of (B, V, 3), areas / cdf row b of (B, F); packed
// (items = B rows (face_begin, face_end, vertex_base) of int64) item b is faces [face_begin, face_end) of the F packed faces, whose
// ids count from vertex_base in the V packed vertices, areas / cdf (F).  Every index that comes from data is compared with its
// buffer's size before use: an item's face range with F, a vertex id (+ base) with V, a face choice with F.
#include <hip/hip_runtime.h>
#include "common.h"
#include "block_scan.h"
#include "sample_points.h"
#include "../../include/kaolin_amd.h"

namespace {

struct SpMesh {
  long long B, F, V;
  const long long* items;  // nullptr: batched
  const long long* faces;
  long long fs_f, fs_k;
  long long vs_b, vs_v, vs_c;
};
struct SpItem {
  long long fb, fe;     // the item's faces in `faces`
  long long vbase;      // added to its vertex ids
  long long voff;       // element offset of its vertices
  long long abase;      // areas / cdf of face f at abase + f
};
__device__ __forceinline__ SpItem sp_item(const SpMesh& m, long long b) {
  SpItem it;
  if (m.items == nullptr) {
    it.fb = 0, it.fe = m.F, it.vbase = 0, it.voff = b * m.vs_b, it.abase = b * m.F;
  } else {
    long long fb = m.items[3 * b], fe = m.items[3 * b + 1];
    if (fb < 0) fb = 0;  // guard: a face range outside the F faces
    if (fe > m.F) fe = m.F;
    if (fe < fb) fe = fb;
    it.fb = fb, it.fe = fe, it.vbase = m.items[3 * b + 2], it.voff = 0, it.abase = 0;
  }
  return it;
}
// the three corners of face f of the item; false when a vertex id falls outside the V vertices (guard)
template <typename T>
__device__ __forceinline__ bool sp_corners(const SpMesh& m, const SpItem& it, const T* __restrict__ vertices, long long f,
                                           long long id[3], T v[3][3]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    id[k] = m.faces[f * m.fs_f + k * m.fs_k] + it.vbase;
    if (id[k] < 0 || id[k] >= m.V) ok = false, id[k] = 0;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) v[k][c] = vertices[it.voff + id[k] * m.vs_v + c * m.vs_c];
  return ok;
}
// correctly rounded (hipcc's default for sqrtf; the __fsqrt_rn of the HIP headers is the native approximation)
__device__ __forceinline__ float sp_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double sp_sqrt(double x) { return sqrt(x); }
template <typename T>
__device__ __forceinline__ T sp_nan();
template <>
__device__ __forceinline__ float sp_nan<float>() { return __int_as_float(0x7fc00000); }
template <>
__device__ __forceinline__ double sp_nan<double>() { return __longlong_as_double(0x7ff8000000000000LL); }

// packed: the item that holds face f (the first whose face_end is above f), or -1
__device__ __forceinline__ long long sp_item_of_face(const SpMesh& m, long long f) {
  long long lo = 0, hi = m.B - 1;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (m.items[3 * mid + 1] > f)
      hi = mid;
    else
      lo = mid + 1;
  }
  return (m.items[3 * lo] <= f && f < m.items[3 * lo + 1]) ? lo : -1;
}
// thread i of B F (batched) or F (packed) -> its item and face; false: no such face
__device__ __forceinline__ bool sp_face_of_thread(const SpMesh& m, long long i, long long* b, long long* f) {
  if (m.items == nullptr) {
    if (i >= m.B * m.F) return false;
    *b = i / m.F, *f = i - *b * m.F;
    return true;
  }
  if (i >= m.F) return false;
  *f = i, *b = sp_item_of_face(m, i);
  return true;
}

// ---- areas ------------------------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void sp_area_terms(const T v[3][3], T x[3], T y[3], T d[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = v[0][c] - v[1][c], y[c] = v[1][c] - v[2][c];
  d[0] = x[1] * y[2] - x[2] * y[1];
  d[1] = x[2] * y[0] - x[0] * y[2];
  d[2] = x[0] * y[1] - x[1] * y[0];
}
template <typename T>
__global__ __launch_bounds__(256) void sp_areas_kernel(SpMesh m, const T* __restrict__ vertices, T* __restrict__ areas) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  long long b, f;
  if (!sp_face_of_thread(m, i, &b, &f)) return;
  T area = sp_nan<T>();  // a face of no item, or with a vertex id outside the vertices
  if (b >= 0) {
    const SpItem it = sp_item(m, b);
    long long id[3];
    T v[3][3], x[3], y[3], d[3];
    if (sp_corners(m, it, vertices, f, id, v)) {
      sp_area_terms(v, x, y, d);
      area = sp_sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) * (T)0.5;
    }
  }
  areas[i] = area;
}
// grad_corners (B F | F, 3, 3): the reference's autograd expression, operation by operation (0 * inf = NaN at a zero-area face)
template <typename T>
__global__ __launch_bounds__(256) void sp_areas_backward_kernel(SpMesh m, const T* __restrict__ vertices,
                                                                const T* __restrict__ grad_areas, long long gs_b, long long gs_f,
                                                                T* __restrict__ grad_corners) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  long long b, f;
  if (!sp_face_of_thread(m, i, &b, &f)) return;
  T gv[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) gv[k][c] = (T)0;
  if (b >= 0) {
    const SpItem it = sp_item(m, b);
    long long id[3];
    T v[3][3], x[3], y[3], d[3];
    if (sp_corners(m, it, vertices, f, id, v)) {
      sp_area_terms(v, x, y, d);
      const T g = grad_areas[(m.items == nullptr ? b : 0) * gs_b + f * gs_f];
      const T root = sp_sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
      const T gs = (g * (T)0.5) / ((T)2 * root);
      const T g0 = gs * ((T)2 * d[0]), g1 = gs * ((T)2 * d[1]), g2 = gs * ((T)2 * d[2]);
      const T gx[3] = {g2 * y[1] - g1 * y[2], g0 * y[2] - g2 * y[0], g1 * y[0] - g0 * y[1]};
      const T gy[3] = {g1 * x[2] - g2 * x[1], g2 * x[0] - g0 * x[2], g0 * x[1] - g1 * x[0]};
#pragma unroll
      for (int c = 0; c < 3; ++c) gv[0][c] = gx[c], gv[1][c] = gy[c] - gx[c], gv[2][c] = -gy[c];
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) grad_corners[i * 9 + k * 3 + c] = gv[k][c];
}

// ---- cdf --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double sp_area_at(const void* areas, int wide, long long at) {
  return wide ? ((const double*)areas)[at] : (double)((const float*)areas)[at];
}
// workgroup (item, tile): cdf <- the inclusive sums inside the tile, partials[item, tile] <- the tile's total
__global__ __launch_bounds__(SP_SCAN_THREADS) void sp_cdf_tiles_kernel(SpMesh m, long long tiles, const void* __restrict__ areas,
                                                                       int wide, double* __restrict__ cdf,
                                                                       double* __restrict__ partials) {
  __shared__ double s_w[SP_SCAN_THREADS / 64 + 1];
  const long long b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
  const SpItem it = sp_item(m, b);
  const long long i0 = it.fb + t * SP_SCAN_TILE + (long long)threadIdx.x * SP_SCAN_PER_THREAD;
  double s[SP_SCAN_PER_THREAD];
  double run = 0.0;
#pragma unroll
  for (int k = 0; k < SP_SCAN_PER_THREAD; ++k) {
    const double a = i0 + k < it.fe ? sp_area_at(areas, wide, it.abase + i0 + k) : 0.0;
    run = run + a;
    s[k] = run;
  }
  double total;
  const double off = block_exclusive(run, s_w, &total);
#pragma unroll
  for (int k = 0; k < SP_SCAN_PER_THREAD; ++k)
    if (i0 + k < it.fe) cdf[it.abase + i0 + k] = off + s[k];
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}
// workgroup item: partials[item, :] <- their exclusive sums
__global__ __launch_bounds__(SP_SCAN_THREADS) void sp_cdf_partials_kernel(long long tiles, double* __restrict__ partials) {
  __shared__ double s_w[SP_SCAN_THREADS / 64 + 1];
  double* p = partials + (long long)blockIdx.x * tiles;
  double carry = 0.0;
  for (long long c = 0; c < tiles; c += SP_SCAN_THREADS) {
    const long long i = c + threadIdx.x;
    const double v = i < tiles ? p[i] : 0.0;
    double total;
    const double ex = block_exclusive(v, s_w, &total);
    if (i < tiles) p[i] = carry + ex;
    carry = carry + total;
  }
}
__global__ __launch_bounds__(SP_SCAN_THREADS) void sp_cdf_add_kernel(SpMesh m, long long tiles, const double* __restrict__ partials,
                                                                     double* __restrict__ cdf) {
  const long long b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
  if (t == 0) return;  // (its offset is +0)
  const SpItem it = sp_item(m, b);
  const double off = partials[blockIdx.x];
  const long long base = it.fb + t * SP_SCAN_TILE;
#pragma unroll
  for (int k = 0; k < SP_SCAN_PER_THREAD; ++k) {
    const long long i = base + (long long)k * SP_SCAN_THREADS + threadIdx.x;
    if (i < it.fe) cdf[it.abase + i] = off + cdf[it.abase + i];
  }
}
long long sp_tiles(long long max_faces) { return (max_faces + SP_SCAN_TILE - 1) / SP_SCAN_TILE; }

// ---- sampling ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void sp_weights(T uv0, T uv1, T w[3]) {
  const T u = sp_sqrt(uv0);
  w[0] = (T)1 - u;
  w[1] = u * ((T)1 - uv1);
  w[2] = u * uv1;
}
// an item samples when its total area is a positive finite number
__device__ __forceinline__ bool sp_live(double total) { return total > 0.0 && total < __longlong_as_double(0x7ff0000000000000LL); }

// The blend of D feature channels per sample, same expression as the points.  LANES: the lanes of the wavefront walk the channels of
// one sample after another (every lane of the wavefront must call this); else a loop in the sample's thread.
template <typename T, bool LANES, typename Body>
__device__ __forceinline__ void sp_for_channels(long long D, bool valid, long long f, long long row, const T w[3], Body body) {
  if (!LANES) {
    if (valid)
      for (long long d = 0; d < D; ++d) body(f, row, w[0], w[1], w[2], d);
    return;
  }
  const int lane = threadIdx.x & 63;
  int G = SP_FEATURE_LANE_GROUP;
  while (G < 64 && G < D) G <<= 1;
  const int per = 64 / G, sub = lane / G, d0 = lane - sub * G;
  for (int j = 0; j < 64; j += per) {
    const int src = j + sub;
    const int vj = __shfl((int)valid, src, 64);
    const long long fj = __shfl(f, src, 64), rj = __shfl(row, src, 64);
    const T w0 = __shfl(w[0], src, 64), w1 = __shfl(w[1], src, 64), w2 = __shfl(w[2], src, 64);
    if (vj)
      for (long long d = d0; d < D; d += G) body(fj, rj, w0, w1, w2, d);
  }
}

// one thread per (item, sample); a workgroup never straddles two items
template <typename T, bool LANES>
__global__ __launch_bounds__(SP_SAMPLE_THREADS) void sp_sample_kernel(SpMesh m, long long N, long long D, long long blocks_per_item,
                                                                      const T* __restrict__ vertices, const void* __restrict__ areas,
                                                                      int wide, const double* __restrict__ cdf,
                                                                      const double* __restrict__ r, const T* __restrict__ uv,
                                                                      const T* __restrict__ feats, long long ff_b, long long ff_f,
                                                                      long long ff_k, long long ff_d, T* __restrict__ points,
                                                                      long long* __restrict__ choices, T* __restrict__ features) {
  __shared__ double s_tab[SP_TABLE];
  const long long b = blockIdx.x / blocks_per_item;
  const long long n = (blockIdx.x - b * blocks_per_item) * SP_SAMPLE_THREADS + threadIdx.x;
  const SpItem it = sp_item(m, b);
  const long long Fi = it.fe - it.fb;
  const double* c = cdf + it.abase + it.fb;  // the item's cdf, c[0 .. Fi)
  // the coarse table: entry k = the cdf at the end of the k-th run of `step` faces
  const long long step = Fi > 0 ? (Fi + SP_TABLE - 1) / SP_TABLE : 1;
  const long long entries = Fi > 0 ? (Fi + step - 1) / step : 0;  // <= SP_TABLE
  for (long long k = threadIdx.x; k < entries; k += SP_SAMPLE_THREADS) {
    const long long e = (k + 1) * step - 1;
    s_tab[k] = c[e < Fi ? e : Fi - 1];
  }
  const double total = Fi > 0 ? c[Fi - 1] : 0.0;
  __syncthreads();
  const bool valid = n < N;
  const bool live = sp_live(total);
  const long long row = b * N + (valid ? n : 0);
  long long f = it.fb;
  T w[3] = {sp_nan<T>(), sp_nan<T>(), sp_nan<T>()};
  if (valid && live) {
    double t = r[row] * total;
    const double below = __longlong_as_double(__double_as_longlong(total) - 1);  // nextbelow of a positive finite number
    if (!(t < below)) t = below;
    long long lo = 0, hi = entries - 1;
    while (lo < hi) {  // LDS: the run that holds the face
      const long long mid = (lo + hi) >> 1;
      if (s_tab[mid] > t)
        hi = mid;
      else
        lo = mid + 1;
    }
    hi = (lo + 1) * step < Fi ? (lo + 1) * step - 1 : Fi - 1;
    lo = lo * step;
    while (lo < hi) {  // global: the face inside the run; lo and hi stay inside [0, Fi)
      const long long mid = (lo + hi) >> 1;
      if (c[mid] > t)
        hi = mid;
      else
        lo = mid + 1;
    }
    // the sums are not monotone to the last bit: a face without area is passed over for the nearest one with area
    if (!(sp_area_at(areas, wide, it.abase + it.fb + lo) > 0.0)) {
      long long g = lo + 1;
      while (g < Fi && !(sp_area_at(areas, wide, it.abase + it.fb + g) > 0.0)) ++g;
      if (g >= Fi) {
        g = lo - 1;
        while (g >= 0 && !(sp_area_at(areas, wide, it.abase + it.fb + g) > 0.0)) --g;
      }
      if (g >= 0 && g < Fi) lo = g;
    }
    f = it.fb + lo;
    sp_weights(uv[2 * row], uv[2 * row + 1], w);
  }
  if (valid) {
    T p[3] = {sp_nan<T>(), sp_nan<T>(), sp_nan<T>()};
    if (live) {
      long long id[3];
      T v[3][3];
      if (sp_corners(m, it, vertices, f, id, v)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = (w[0] * v[0][k] + w[1] * v[1][k]) + w[2] * v[2][k];
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) points[row * 3 + k] = p[k];
    choices[row] = f;
  }
  if (D > 0) {
    const long long nF = m.F;
    sp_for_channels<T, LANES>(D, valid, f, row, w, [&](long long fj, long long rj, T w0, T w1, T w2, long long d) {
      T out = sp_nan<T>();
      if (fj >= 0 && fj < nF) {  // guard
        const T* src = feats + b * ff_b + fj * ff_f + d * ff_d;
        out = (w0 * src[0] + w1 * src[ff_k]) + w2 * src[2 * ff_k];
      }
      features[rj * D + d] = out;
    });
  }
}

// one thread per (item, sample): w_k g added to the three vertices and the three feature rows of the chosen face
template <typename T, bool LANES>
__global__ __launch_bounds__(SP_SAMPLE_THREADS) void sp_sample_backward_kernel(SpMesh m, long long N, long long D,
                                                                               long long blocks_per_item,
                                                                               const double* __restrict__ cdf,
                                                                               const T* __restrict__ uv,
                                                                               const long long* __restrict__ choices,
                                                                               const T* __restrict__ grad_points,
                                                                               const T* __restrict__ grad_features,
                                                                               T* __restrict__ grad_vertices,
                                                                               T* __restrict__ grad_face_features) {
  const long long b = blockIdx.x / blocks_per_item;
  const long long n = (blockIdx.x - b * blocks_per_item) * SP_SAMPLE_THREADS + threadIdx.x;
  const SpItem it = sp_item(m, b);
  const double total = it.fe > it.fb ? cdf[it.abase + it.fe - 1] : 0.0;
  bool valid = n < N && sp_live(total);  // (the NaN of an item without area does not depend on the inputs)
  const long long row = b * N + (n < N ? n : 0);
  long long f = 0;
  T w[3] = {(T)0, (T)0, (T)0};
  if (valid) {
    f = choices[row];
    if (f < it.fb || f >= it.fe) valid = false;  // guard: a face choice outside the item's faces
  }
  if (valid) {
    sp_weights(uv[2 * row], uv[2 * row + 1], w);
    if (grad_vertices != nullptr) {
      long long id[3];
      bool ok = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        id[k] = m.faces[f * m.fs_f + k * m.fs_k] + it.vbase;
        if (id[k] < 0 || id[k] >= m.V) ok = false;  // guard
      }
      if (ok) {
        const long long base = m.items == nullptr ? b * m.V : 0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
          for (int cc = 0; cc < 3; ++cc) kamd_atomic_add(&grad_vertices[(base + id[k]) * 3 + cc], w[k] * grad_points[row * 3 + cc]);
      }
    }
  }
  if (D > 0 && grad_face_features != nullptr) {
    const long long nF = m.F;
    sp_for_channels<T, LANES>(D, valid, f, row, w, [&](long long fj, long long rj, T w0, T w1, T w2, long long d) {
      const T g = grad_features[rj * D + d];
      T* dst = grad_face_features + ((b * nF + fj) * 3) * D + d;
      kamd_atomic_add(dst, w0 * g);
      kamd_atomic_add(dst + D, w1 * g);
      kamd_atomic_add(dst + 2 * D, w2 * g);
    });
  }
}

// ---- hosts ------------------------------------------------------------------------------------------------------------------------
bool sp_mesh(SpMesh* m, int64_t B, int64_t F, int64_t V, const int64_t* items, const int64_t* faces, int64_t fs_f, int64_t fs_k,
             int64_t vs_b, int64_t vs_v, int64_t vs_c) {
  if (B <= 0 || F <= 0 || V <= 0 || faces == nullptr) return false;
  if (F > 0x3FFFFFFFFFFFLL / B || V > 0x3FFFFFFFFFFFLL / B) return false;
  m->B = B, m->F = F, m->V = V, m->items = (const long long*)items, m->faces = (const long long*)faces;
  m->fs_f = fs_f, m->fs_k = fs_k, m->vs_b = vs_b, m->vs_v = vs_v, m->vs_c = vs_c;
  return true;
}
long long sp_face_threads(const SpMesh& m) { return m.items == nullptr ? m.B * m.F : m.F; }

template <typename T>
int sp_areas(void* stream, const SpMesh& m, const T* vertices, T* areas) {
  if (vertices == nullptr || areas == nullptr) return (int)hipErrorInvalidValue;
  const long long blocks = (sp_face_threads(m) + 255) / 256;
  if (blocks > 0x7FFFFFFFLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((sp_areas_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, m, vertices, areas);
  KAMD_RETURN_LAST_ERROR();
}
template <typename T>
int sp_areas_backward(void* stream, const SpMesh& m, const T* vertices, const T* grad_areas, int64_t gs_b, int64_t gs_f,
                      T* grad_corners) {
  if (vertices == nullptr || grad_areas == nullptr || grad_corners == nullptr) return (int)hipErrorInvalidValue;
  const long long blocks = (sp_face_threads(m) + 255) / 256;
  if (blocks > 0x7FFFFFFFLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((sp_areas_backward_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, m, vertices, grad_areas,
                     (long long)gs_b, (long long)gs_f, grad_corners);
  KAMD_RETURN_LAST_ERROR();
}
int sp_cdf(void* stream, int64_t B, int64_t F, int64_t max_faces, const int64_t* items, const void* areas, int wide, double* cdf,
           void* workspace, size_t workspace_bytes) {
  if (B <= 0 || F <= 0 || F > 0x3FFFFFFFFFFFLL / B || areas == nullptr || cdf == nullptr || max_faces <= 0 || max_faces > F)
    return (int)hipErrorInvalidValue;
  SpMesh m = {};  // (only the items are read)
  m.B = B, m.F = F, m.items = (const long long*)items;
  const long long tiles = sp_tiles(max_faces), blocks = B * tiles;
  if (blocks > 0x7FFFFFFFLL || workspace == nullptr || workspace_bytes < (size_t)blocks * 8) return (int)hipErrorInvalidValue;
  double* partials = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sp_cdf_tiles_kernel, dim3((unsigned)blocks), dim3(SP_SCAN_THREADS), 0, st, m, tiles, areas, wide, cdf, partials);
  KAMD_CHECK(hipGetLastError());
  if (tiles > 1) {
    hipLaunchKernelGGL(sp_cdf_partials_kernel, dim3((unsigned)B), dim3(SP_SCAN_THREADS), 0, st, tiles, partials);
    KAMD_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sp_cdf_add_kernel, dim3((unsigned)blocks), dim3(SP_SCAN_THREADS), 0, st, m, tiles, (const double*)partials, cdf);
  }
  KAMD_RETURN_LAST_ERROR();
}
template <typename T>
int sp_sample(void* stream, const SpMesh& m, int64_t N, int64_t D, const T* vertices, const void* areas, int areas_bytes,
              const double* cdf, const double* r, const T* uv, const T* feats, int64_t ff_b, int64_t ff_f, int64_t ff_k, int64_t ff_d,
              T* points, int64_t* choices, T* features) {
  if (N <= 0 || D < 0 || vertices == nullptr || areas == nullptr || cdf == nullptr || r == nullptr || uv == nullptr ||
      points == nullptr || choices == nullptr || (areas_bytes != 4 && areas_bytes != 8))
    return (int)hipErrorInvalidValue;
  if (D > 0 && (feats == nullptr || features == nullptr || m.items != nullptr)) return (int)hipErrorInvalidValue;
  const long long per = (N + SP_SAMPLE_THREADS - 1) / SP_SAMPLE_THREADS;
  if (per > 0x7FFFFFFFLL / m.B || N > 0x3FFFFFFFFFFFLL / m.B || (D > 0 && m.B * N > 0x3FFFFFFFFFFFLL / D))
    return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)(m.B * per)), block(SP_SAMPLE_THREADS);
  hipStream_t st = (hipStream_t)stream;
  const int wide = areas_bytes == 8 ? 1 : 0;
  // (experiment builds measure the switch: profiles/sample_points_time.jsonl)
  if (D >= kamd_env_int("KAMD_SP_LANES_FROM", SP_FEATURE_LANES_FROM))
    hipLaunchKernelGGL((sp_sample_kernel<T, true>), grid, block, 0, st, m, (long long)N, (long long)D, per, vertices, areas, wide, cdf, r,
                       uv, feats, (long long)ff_b, (long long)ff_f, (long long)ff_k, (long long)ff_d, points, (long long*)choices,
                       features);
  else
    hipLaunchKernelGGL((sp_sample_kernel<T, false>), grid, block, 0, st, m, (long long)N, (long long)D, per, vertices, areas, wide, cdf,
                       r, uv, feats, (long long)ff_b, (long long)ff_f, (long long)ff_k, (long long)ff_d, points, (long long*)choices,
                       features);
  KAMD_RETURN_LAST_ERROR();
}
template <typename T>
int sp_sample_backward(void* stream, const SpMesh& m, int64_t N, int64_t D, const double* cdf, const T* uv, const int64_t* choices,
                       const T* grad_points, const T* grad_features, T* grad_vertices, T* grad_face_features) {
  if (N <= 0 || D < 0 || cdf == nullptr || uv == nullptr || choices == nullptr) return (int)hipErrorInvalidValue;
  if (grad_vertices != nullptr && grad_points == nullptr) return (int)hipErrorInvalidValue;
  if (grad_face_features != nullptr && (grad_features == nullptr || D <= 0 || m.items != nullptr)) return (int)hipErrorInvalidValue;
  if (grad_vertices == nullptr && grad_face_features == nullptr) return 0;
  const long long per = (N + SP_SAMPLE_THREADS - 1) / SP_SAMPLE_THREADS;
  if (per > 0x7FFFFFFFLL / m.B || N > 0x3FFFFFFFFFFFLL / m.B || (D > 0 && m.B * N > 0x3FFFFFFFFFFFLL / D) ||
      (D > 0 && m.B * m.F > 0x3FFFFFFFFFFFLL / (3 * D)))
    return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)(m.B * per)), block(SP_SAMPLE_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (D >= kamd_env_int("KAMD_SP_LANES_FROM", SP_FEATURE_LANES_FROM) && grad_face_features != nullptr)
    hipLaunchKernelGGL((sp_sample_backward_kernel<T, true>), grid, block, 0, st, m, (long long)N, (long long)D, per, cdf, uv,
                       (const long long*)choices, grad_points, grad_features, grad_vertices, grad_face_features);
  else
    hipLaunchKernelGGL((sp_sample_backward_kernel<T, false>), grid, block, 0, st, m, (long long)N, (long long)D, per, cdf, uv,
                       (const long long*)choices, grad_points, grad_features, grad_vertices, grad_face_features);
  KAMD_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {

int kamd_face_areas_f32(void* stream, int64_t B, int64_t F, int64_t V, const int64_t* items, const float* vertices, int64_t vs_b,
                        int64_t vs_v, int64_t vs_c, const int64_t* faces, int64_t fs_f, int64_t fs_k, float* areas) {
  SpMesh m;
  if (!sp_mesh(&m, B, F, V, items, faces, fs_f, fs_k, vs_b, vs_v, vs_c)) return (int)hipErrorInvalidValue;
  return sp_areas<float>(stream, m, vertices, areas);
}
int kamd_face_areas_f64(void* stream, int64_t B, int64_t F, int64_t V, const int64_t* items, const double* vertices, int64_t vs_b,
                        int64_t vs_v, int64_t vs_c, const int64_t* faces, int64_t fs_f, int64_t fs_k, double* areas) {
  SpMesh m;
  if (!sp_mesh(&m, B, F, V, items, faces, fs_f, fs_k, vs_b, vs_v, vs_c)) return (int)hipErrorInvalidValue;
  return sp_areas<double>(stream, m, vertices, areas);
}
int kamd_face_areas_backward_f32(void* stream, int64_t B, int64_t F, int64_t V, const int64_t* items, const float* vertices,
                                 int64_t vs_b, int64_t vs_v, int64_t vs_c, const int64_t* faces, int64_t fs_f, int64_t fs_k,
                                 const float* grad_areas, int64_t gs_b, int64_t gs_f, float* grad_corners) {
  SpMesh m;
  if (!sp_mesh(&m, B, F, V, items, faces, fs_f, fs_k, vs_b, vs_v, vs_c)) return (int)hipErrorInvalidValue;
  return sp_areas_backward<float>(stream, m, vertices, grad_areas, gs_b, gs_f, grad_corners);
}
int kamd_face_areas_backward_f64(void* stream, int64_t B, int64_t F, int64_t V, const int64_t* items, const double* vertices,
                                 int64_t vs_b, int64_t vs_v, int64_t vs_c, const int64_t* faces, int64_t fs_f, int64_t fs_k,
                                 const double* grad_areas, int64_t gs_b, int64_t gs_f, double* grad_corners) {
  SpMesh m;
  if (!sp_mesh(&m, B, F, V, items, faces, fs_f, fs_k, vs_b, vs_v, vs_c)) return (int)hipErrorInvalidValue;
  return sp_areas_backward<double>(stream, m, vertices, grad_areas, gs_b, gs_f, grad_corners);
}

size_t kamd_sample_cdf_workspace(int64_t B, int64_t F) {
  if (B <= 0 || F <= 0 || sp_tiles(F) > 0x7FFFFFFFLL / B) return 0;
  return (size_t)(B * sp_tiles(F)) * 8;
}
int kamd_sample_cdf_f32(void* stream, int64_t B, int64_t F, int64_t max_faces, const int64_t* items, const float* areas, double* cdf,
                        void* workspace, size_t workspace_bytes) {
  return sp_cdf(stream, B, F, max_faces, items, areas, 0, cdf, workspace, workspace_bytes);
}
int kamd_sample_cdf_f64(void* stream, int64_t B, int64_t F, int64_t max_faces, const int64_t* items, const double* areas, double* cdf,
                        void* workspace, size_t workspace_bytes) {
  return sp_cdf(stream, B, F, max_faces, items, areas, 1, cdf, workspace, workspace_bytes);
}

int kamd_sample_points_f32(void* stream, int64_t B, int64_t F, int64_t V, int64_t N, int64_t D, const int64_t* items,
                           const float* vertices, int64_t vs_b, int64_t vs_v, int64_t vs_c, const int64_t* faces, int64_t fs_f,
                           int64_t fs_k, const void* areas, int areas_bytes, const double* cdf, const double* r, const float* uv,
                           const float* face_features, int64_t ff_b, int64_t ff_f, int64_t ff_k, int64_t ff_d, float* points,
                           int64_t* face_choices, float* features) {
  SpMesh m;
  if (!sp_mesh(&m, B, F, V, items, faces, fs_f, fs_k, vs_b, vs_v, vs_c)) return (int)hipErrorInvalidValue;
  return sp_sample<float>(stream, m, N, D, vertices, areas, areas_bytes, cdf, r, uv, face_features, ff_b, ff_f, ff_k, ff_d, points,
                          face_choices, features);
}
int kamd_sample_points_f64(void* stream, int64_t B, int64_t F, int64_t V, int64_t N, int64_t D, const int64_t* items,
                           const double* vertices, int64_t vs_b, int64_t vs_v, int64_t vs_c, const int64_t* faces, int64_t fs_f,
                           int64_t fs_k, const void* areas, int areas_bytes, const double* cdf, const double* r, const double* uv,
                           const double* face_features, int64_t ff_b, int64_t ff_f, int64_t ff_k, int64_t ff_d, double* points,
                           int64_t* face_choices, double* features) {
  SpMesh m;
  if (!sp_mesh(&m, B, F, V, items, faces, fs_f, fs_k, vs_b, vs_v, vs_c)) return (int)hipErrorInvalidValue;
  return sp_sample<double>(stream, m, N, D, vertices, areas, areas_bytes, cdf, r, uv, face_features, ff_b, ff_f, ff_k, ff_d, points,
                           face_choices, features);
}
int kamd_sample_points_backward_f32(void* stream, int64_t B, int64_t F, int64_t V, int64_t N, int64_t D, const int64_t* items,
                                    const int64_t* faces, int64_t fs_f, int64_t fs_k, const double* cdf, const float* uv,
                                    const int64_t* face_choices, const float* grad_points, const float* grad_features,
                                    float* grad_vertices, float* grad_face_features) {
  SpMesh m;
  if (!sp_mesh(&m, B, F, V, items, faces, fs_f, fs_k, 0, 0, 0)) return (int)hipErrorInvalidValue;
  return sp_sample_backward<float>(stream, m, N, D, cdf, uv, face_choices, grad_points, grad_features, grad_vertices,
                                   grad_face_features);
}
int kamd_sample_points_backward_f64(void* stream, int64_t B, int64_t F, int64_t V, int64_t N, int64_t D, const int64_t* items,
                                    const int64_t* faces, int64_t fs_f, int64_t fs_k, const double* cdf, const double* uv,
                                    const int64_t* face_choices, const double* grad_points, const double* grad_features,
                                    double* grad_vertices, double* grad_face_features) {
  SpMesh m;
  if (!sp_mesh(&m, B, F, V, items, faces, fs_f, fs_k, 0, 0, 0)) return (int)hipErrorInvalidValue;
  return sp_sample_backward<double>(stream, m, N, D, cdf, uv, face_choices, grad_points, grad_features, grad_vertices,
                                    grad_face_features);
}

}  // extern "C"
