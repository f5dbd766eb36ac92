// ops.pointcloud.farthest_point_sampling: k dependent rounds of "N distance updates + one arg-max" per cloud.  The reference runs
// NVIDIA Warp kernels around a radix sort (kaolin/ops/pointcloud.py:98-535) and its result depends on the order of a CAS race; this
// file computes ONE rule (below) with two work splits that give the same indices.
//
// THE RULE, per cloud, d(a, b) = (dx*dx + dy*dy) + dz*dz in float32, one rounding per operation (-ffp-contract=off, no fma spelled):
//   centre   float64 sum of the points whose three coordinates are finite / their count, rounded to float32; (0, 0, 0) when there
//            is no such point or the result is not finite
//   first    D_i = d(p_i, centre) if finite else -1; first = arg-max D, lowest index on ties
//   then     D_i = d(p_i, p_first) if finite else -1; D_first = -2 (taken)
//   round    s = arg-max D, lowest index on ties; out <- s; D_s = -2; D_i = min(D_i, d(p_i, p_s)) where that d is finite
//   (an inf or NaN d is never below D_i, so the round's "where finite" is the plain comparison d < D_i)
// D is compared as a 64-bit key, orderable(D) << 32 | (0xFFFFFFFF - index): an unsigned max is "largest D, lowest index" in one
// reduction, keys of different points differ, and D is never NaN.  Padding slots hold -3 and are never reached (k <= N).
//
// 1. fps_block<P>, N <= 1024 P, P in {1, 2, 4, 8, 16}: ONE workgroup of 1024 threads per cloud (16 wavefronts, one CU), grid = B.
//    Thread t owns points t + 1024 j: their coordinates and running D stay in 4 P VGPRs for the whole call; after the initial load
//    nothing but the k output indices touches global memory.  A round:
//      every thread updates its P distances against the selected point and keeps its best (D, slot, xyz; strict > over ascending
//      slots = lowest index);  wavefront max of the key: 4 DPP steps inside the rows of 16 lanes, then 4 v_readlane;  the lane that
//      owns the maximum writes {key, x, y, z} to LDS slot [round parity][wavefront];  ONE __syncthreads();  every wavefront reads
//      the 16 slots (lane & 15), reduces them with the same 4 DPP steps and takes the winner's coordinates from the winning slot.
//    The slots are double-buffered by parity: a wavefront can only write parity p again after the barrier of the round between,
//    which every wavefront reaches after its reads of p.  The selected point is never fetched by index from global memory.
//    The centre uses the same shape: float64 partial sums and a count per wavefront through LDS, added in wavefront order.
// 2. fps_round, N above the block limit: one launch per round, enqueued by a loop in the entry point; the launch boundary is the
//    only synchronisation (no grid barrier, no spinning, no atomics).  G = ceil(N / 2048) workgroups of 256 threads x B; D lives
//    in the workspace.  Launch r: every workgroup reduces the G partials {key, x, y, z} launch r - 1 wrote (redundantly, in one
//    fixed order, buffer double-buffered by parity), workgroup 0 stores the index, each updates its own 2048 distances and writes
//    its own partial.  Launch 0 adds the G float64 centre partials of a leading launch (every workgroup, same order) and SETS D.
//    k + 2 launches, no host read, no synchronisation: capturable.
#include "common.h"
#include "../../include/kaolin_amd.h"

namespace {

typedef unsigned long long u64;

constexpr int FB_THREADS = 1024, FB_WAVES = FB_THREADS / KAMD_WAVE;
constexpr int FB_MAX_P = 16;
constexpr int FB_LIMIT = FB_THREADS * FB_MAX_P;  // the largest N of the block path
constexpr int FR_THREADS = 256, FR_WAVES = FR_THREADS / KAMD_WAVE, FR_ITEMS = 8, FR_SLICE = FR_THREADS * FR_ITEMS;
constexpr float FPS_INVALID = -1.0f, FPS_TAKEN = -2.0f, FPS_PADDED = -3.0f;

struct FpsSlot {
  u64 key;
  float x, y, z;
  unsigned int pad;
};

__device__ __forceinline__ float fps_dist(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}
__device__ __forceinline__ bool fps_finite(float v) { return __builtin_isfinite(v); }

__device__ __forceinline__ u64 fps_key(float d, unsigned int index) {
  const unsigned int u = __float_as_uint(d);
  const unsigned int o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((u64)o << 32) | (u64)(0xFFFFFFFFu - index);
}
__device__ __forceinline__ unsigned int fps_key_index(u64 key) { return 0xFFFFFFFFu - (unsigned int)key; }

template <int CTRL>
__device__ __forceinline__ u64 fps_dpp(u64 v) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned int)v, CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned int)(v >> 32), CTRL, 0xF, 0xF, false);
  return ((u64)(unsigned int)hi << 32) | (u64)(unsigned int)lo;
}
__device__ __forceinline__ u64 fps_max(u64 a, u64 b) { return a > b ? a : b; }
// the maximum over the lane's row of 16 lanes, in every lane of the row; all lanes active.  lane ^ 1, lane ^ 2 make the quads
// uniform; row_ror:4 and row_ror:8 then bring the three other quads in
__device__ __forceinline__ u64 fps_row_max(u64 v) {
  v = fps_max(v, fps_dpp<0xB1>(v));   // quad_perm [1, 0, 3, 2]
  v = fps_max(v, fps_dpp<0x4E>(v));   // quad_perm [2, 3, 0, 1]
  v = fps_max(v, fps_dpp<0x124>(v));  // row_ror:4
  v = fps_max(v, fps_dpp<0x128>(v));  // row_ror:8
  return v;
}
__device__ __forceinline__ u64 fps_readlane(u64 v, int lane) {
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)v, lane);
  const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(v >> 32), lane);
  return ((u64)hi << 32) | lo;
}
// the maximum over the wavefront, wave-uniform; all 64 lanes active
__device__ __forceinline__ u64 fps_wave_max(u64 v) {
  v = fps_row_max(v);
  return fps_max(fps_max(fps_readlane(v, 15), fps_readlane(v, 31)), fps_max(fps_readlane(v, 47), fps_readlane(v, 63)));
}
__device__ __forceinline__ double fps_wave_sum(double v) {
#pragma unroll
  for (int m = 1; m < KAMD_WAVE; m <<= 1) v = v + __shfl_xor(v, m);
  return v;
}
// float64 sums of the finite points and their count -> the centre of the rule
__device__ __forceinline__ void fps_centre(double sx, double sy, double sz, double n, float& cx, float& cy, float& cz) {
  cx = (float)(sx / n), cy = (float)(sy / n), cz = (float)(sz / n);
  if (!(n > 0.0) || !fps_finite(cx) || !fps_finite(cy) || !fps_finite(cz)) cx = cy = cz = 0.0f;
}

// ---- 1. one workgroup per cloud, everything in registers ------------------------------------------------------------------------
template <int P>
struct FbState {
  float x[P], y[P], z[P], D[P];
};

// SET: D <- d or -1 (padding -3); else D <- min(D, d).  taken >= 0: that point's D <- -2
template <int P, bool SET>
__device__ __forceinline__ void fb_update(FbState<P>& s, int t, int N, float qx, float qy, float qz, int taken) {
  const int taken_slot = (taken >= 0 && (taken & (FB_THREADS - 1)) == t) ? (taken >> 10) : -1;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const float d = fps_dist(s.x[j], s.y[j], s.z[j], qx, qy, qz);
    float v;
    if constexpr (SET)
      v = (t + FB_THREADS * j < N) ? (fps_finite(d) ? d : FPS_INVALID) : FPS_PADDED;
    else
      v = d < s.D[j] ? d : s.D[j];
    s.D[j] = (j == taken_slot) ? FPS_TAKEN : v;
  }
}

// arg-max of D over the workgroup -> its index, and its coordinates in (qx, qy, qz); one barrier
template <int P>
__device__ __forceinline__ int fb_select(const FbState<P>& s, int t, FpsSlot (*slots)[FB_WAVES], int parity, float& qx, float& qy,
                                         float& qz) {
  float bd = s.D[0], bx = s.x[0], by = s.y[0], bz = s.z[0];
  int bj = 0;
#pragma unroll
  for (int j = 1; j < P; ++j) {
    const bool up = s.D[j] > bd;
    bd = up ? s.D[j] : bd, bx = up ? s.x[j] : bx, by = up ? s.y[j] : by, bz = up ? s.z[j] : bz, bj = up ? j : bj;
  }
  const u64 key = fps_key(bd, (unsigned int)(t + FB_THREADS * bj));
  const u64 top = fps_wave_max(key);
  FpsSlot* mine = slots[parity];
  if (key == top) {
    FpsSlot w;
    w.key = key, w.x = bx, w.y = by, w.z = bz, w.pad = 0;
    mine[t >> 6] = w;
  }
  __syncthreads();
  const u64 best = fps_row_max(mine[t & (FB_WAVES - 1)].key);
  const int sel = __builtin_amdgcn_readfirstlane((int)fps_key_index(best));
  const FpsSlot* win = mine + ((sel & (FB_THREADS - 1)) >> 6);
  qx = win->x, qy = win->y, qz = win->z;
  return sel;
}

template <int P>
__global__ __launch_bounds__(FB_THREADS) void fps_block_kernel(const float* __restrict__ points, int64_t* __restrict__ out, int N,
                                                                int k) {
  __shared__ FpsSlot slots[2][FB_WAVES];
  __shared__ double sums[FB_WAVES][4];
  const int t = threadIdx.x;
  const float* p = points + (size_t)blockIdx.x * (size_t)N * 3;
  int64_t* o = out + (size_t)blockIdx.x * (size_t)k;
  FbState<P> s;
  double sx = 0.0, sy = 0.0, sz = 0.0, n = 0.0;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int i = t + FB_THREADS * j;
    s.x[j] = s.y[j] = s.z[j] = 0.0f;
    if (i < N) {
      s.x[j] = p[(size_t)i * 3], s.y[j] = p[(size_t)i * 3 + 1], s.z[j] = p[(size_t)i * 3 + 2];
      if (fps_finite(s.x[j]) && fps_finite(s.y[j]) && fps_finite(s.z[j]))
        sx = sx + (double)s.x[j], sy = sy + (double)s.y[j], sz = sz + (double)s.z[j], n = n + 1.0;
    }
  }
  sx = fps_wave_sum(sx), sy = fps_wave_sum(sy), sz = fps_wave_sum(sz), n = fps_wave_sum(n);
  if ((t & 63) == 0) sums[t >> 6][0] = sx, sums[t >> 6][1] = sy, sums[t >> 6][2] = sz, sums[t >> 6][3] = n;
  __syncthreads();
  sx = sy = sz = n = 0.0;
#pragma unroll
  for (int w = 0; w < FB_WAVES; ++w) sx = sx + sums[w][0], sy = sy + sums[w][1], sz = sz + sums[w][2], n = n + sums[w][3];
  float qx, qy, qz;
  fps_centre(sx, sy, sz, n, qx, qy, qz);

  fb_update<P, true>(s, t, N, qx, qy, qz, -1);
  int sel = fb_select<P>(s, t, slots, 0, qx, qy, qz);
  if (t == 0) o[0] = sel;
  if (k == 1) return;
  fb_update<P, true>(s, t, N, qx, qy, qz, sel);
  sel = fb_select<P>(s, t, slots, 1, qx, qy, qz);
  if (t == 0) o[1] = sel;
  for (int r = 2; r < k; ++r) {
    fb_update<P, false>(s, t, N, qx, qy, qz, sel);
    sel = fb_select<P>(s, t, slots, r & 1, qx, qy, qz);
    if (t == 0) o[r] = sel;
  }
}

// ---- 2. one launch per round --------------------------------------------------------------------------------------------------------
struct FrArgs {
  const float* points;
  int64_t* out;
  float* D;           // (B, N)
  FpsSlot* partial;   // (2, B, G)
  double* sums;       // (B, G, 4)
  int N, k, G;
};

__global__ __launch_bounds__(FR_THREADS) void fps_round_centre_kernel(const FrArgs a) {
  __shared__ double part[FR_WAVES][4];
  const int t = threadIdx.x, g = blockIdx.x, b = blockIdx.y;
  const float* p = a.points + (size_t)b * (size_t)a.N * 3;
  double sx = 0.0, sy = 0.0, sz = 0.0, n = 0.0;
#pragma unroll
  for (int j = 0; j < FR_ITEMS; ++j) {
    const long long i = (long long)g * FR_SLICE + j * FR_THREADS + t;
    if (i < a.N) {
      const float x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
      if (fps_finite(x) && fps_finite(y) && fps_finite(z)) sx = sx + (double)x, sy = sy + (double)y, sz = sz + (double)z, n = n + 1.0;
    }
  }
  sx = fps_wave_sum(sx), sy = fps_wave_sum(sy), sz = fps_wave_sum(sz), n = fps_wave_sum(n);
  if ((t & 63) == 0) part[t >> 6][0] = sx, part[t >> 6][1] = sy, part[t >> 6][2] = sz, part[t >> 6][3] = n;
  __syncthreads();
  if (t < 4) {
    double v = part[0][t];
#pragma unroll
    for (int w = 1; w < FR_WAVES; ++w) v = v + part[w][t];
    a.sums[((size_t)b * a.G + g) * 4 + t] = v;
  }
}

// the workgroup's maximum of `key` (0: none), with that key's coordinates, in every thread; one barrier
__device__ __forceinline__ u64 fr_block_max(u64 key, float& x, float& y, float& z, FpsSlot* slots) {
  const int t = threadIdx.x;
  const u64 top = fps_wave_max(key);
  if (key == top && (key != 0 || (t & 63) == 0)) {
    FpsSlot w;
    w.key = key, w.x = x, w.y = y, w.z = z, w.pad = 0;
    slots[t >> 6] = w;
  }
  __syncthreads();
  int win = 0;
  u64 best = slots[0].key;
#pragma unroll
  for (int w = 1; w < FR_WAVES; ++w) {
    const u64 v = slots[w].key;
    if (v > best) best = v, win = w;
  }
  x = slots[win].x, y = slots[win].y, z = slots[win].z;
  return best;
}

// launch r of 0..k: r == 0 centre -> D; r >= 1 the selection of launch r - 1 -> out[r - 1], then (r < k) D and the next partial
__global__ __launch_bounds__(FR_THREADS) void fps_round_kernel(const FrArgs a, int r) {
  __shared__ FpsSlot slots_in[FR_WAVES], slots_out[FR_WAVES];
  __shared__ double part[FR_WAVES * 4];
  const int t = threadIdx.x, g = blockIdx.x, b = blockIdx.y;
  float qx, qy, qz;
  long long taken = -1;
  if (r == 0) {
    const double* sums = a.sums + (size_t)b * a.G * 4;
    double sx = 0.0, sy = 0.0, sz = 0.0, n = 0.0;
    for (int h = t; h < a.G; h += FR_THREADS) sx = sx + sums[h * 4], sy = sy + sums[h * 4 + 1], sz = sz + sums[h * 4 + 2], n = n + sums[h * 4 + 3];
    sx = fps_wave_sum(sx), sy = fps_wave_sum(sy), sz = fps_wave_sum(sz), n = fps_wave_sum(n);
    if ((t & 63) == 0) part[(t >> 6) * 4] = sx, part[(t >> 6) * 4 + 1] = sy, part[(t >> 6) * 4 + 2] = sz, part[(t >> 6) * 4 + 3] = n;
    __syncthreads();
    sx = sy = sz = n = 0.0;
#pragma unroll
    for (int w = 0; w < FR_WAVES; ++w) sx = sx + part[w * 4], sy = sy + part[w * 4 + 1], sz = sz + part[w * 4 + 2], n = n + part[w * 4 + 3];
    fps_centre(sx, sy, sz, n, qx, qy, qz);
  } else {
    const FpsSlot* in = a.partial + ((size_t)((r - 1) & 1) * gridDim.y + b) * a.G;
    u64 key = 0;
    qx = qy = qz = 0.0f;
    for (int h = t; h < a.G; h += FR_THREADS) {
      const FpsSlot v = in[h];
      if (v.key > key) key = v.key, qx = v.x, qy = v.y, qz = v.z;
    }
    key = fr_block_max(key, qx, qy, qz, slots_in);
    taken = (long long)fps_key_index(key);
    if (g == 0 && t == 0) a.out[(size_t)b * a.k + (r - 1)] = taken;
    if (r == a.k) return;
  }
  const float* p = a.points + (size_t)b * (size_t)a.N * 3;
  float* D = a.D + (size_t)b * (size_t)a.N;
  const bool set = r < 2;
  u64 key = 0;
  float bx = 0.0f, by = 0.0f, bz = 0.0f;
#pragma unroll
  for (int j = 0; j < FR_ITEMS; ++j) {
    const long long i = (long long)g * FR_SLICE + j * FR_THREADS + t;
    if (i < a.N) {
      const float x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
      const float d = fps_dist(x, y, z, qx, qy, qz);
      float v;
      if (set) {
        v = fps_finite(d) ? d : FPS_INVALID;
      } else {
        const float old = D[i];
        v = d < old ? d : old;
      }
      if (i == taken) v = FPS_TAKEN;
      D[i] = v;
      const u64 ki = fps_key(v, (unsigned int)i);
      if (ki > key) key = ki, bx = x, by = y, bz = z;
    }
  }
  key = fr_block_max(key, bx, by, bz, slots_out);
  if (t == 0) {
    FpsSlot w;
    w.key = key, w.x = bx, w.y = by, w.z = bz, w.pad = 0;
    a.partial[((size_t)(r & 1) * gridDim.y + b) * a.G + g] = w;
  }
}

inline int fr_groups(int N) { return kamd_cdiv(N, FR_SLICE); }

int fps_block(hipStream_t st, int B, int N, int k, const float* points, int64_t* out) {
  const dim3 grid((unsigned)B), block(FB_THREADS);
  if (N <= FB_THREADS)
    hipLaunchKernelGGL(fps_block_kernel<1>, grid, block, 0, st, points, out, N, k);
  else if (N <= FB_THREADS * 2)
    hipLaunchKernelGGL(fps_block_kernel<2>, grid, block, 0, st, points, out, N, k);
  else if (N <= FB_THREADS * 4)
    hipLaunchKernelGGL(fps_block_kernel<4>, grid, block, 0, st, points, out, N, k);
  else if (N <= FB_THREADS * 8)
    hipLaunchKernelGGL(fps_block_kernel<8>, grid, block, 0, st, points, out, N, k);
  else
    hipLaunchKernelGGL(fps_block_kernel<16>, grid, block, 0, st, points, out, N, k);
  KAMD_RETURN_LAST_ERROR();
}

int fps_rounds(hipStream_t st, int B, int N, int k, const float* points, int64_t* out, void* workspace) {
  if (workspace == nullptr || B > 65535) return (int)hipErrorInvalidValue;
  const int G = fr_groups(N);
  char* ws = (char*)workspace;
  FrArgs a;
  a.points = points, a.out = out, a.N = N, a.k = k, a.G = G;
  a.D = (float*)ws;
  ws += kamd_align16((size_t)B * N * sizeof(float));
  a.partial = (FpsSlot*)ws;
  ws += kamd_align16((size_t)2 * B * G * sizeof(FpsSlot));
  a.sums = (double*)ws;
  const dim3 grid((unsigned)G, (unsigned)B), block(FR_THREADS);
  hipLaunchKernelGGL(fps_round_centre_kernel, grid, block, 0, st, a);
  for (int r = 0; r < k; ++r) hipLaunchKernelGGL(fps_round_kernel, grid, block, 0, st, a, r);
  hipLaunchKernelGGL(fps_round_kernel, dim3(1, (unsigned)B), block, 0, st, a, k);
  KAMD_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {
size_t kamd_fps_workspace(int B, int N, int k, int path) {
  if (B <= 0 || N <= 0 || k <= 0 || path == 1 || (path == 0 && N <= FB_LIMIT)) return 0;
  const size_t G = (size_t)fr_groups(N);
  return kamd_align16((size_t)B * N * sizeof(float)) + kamd_align16((size_t)2 * B * G * sizeof(FpsSlot)) +
         kamd_align16((size_t)B * G * 4 * sizeof(double));
}

int kamd_fps_block_limit(void) { return FB_LIMIT; }

int kamd_fps_f32(void* stream, int B, int N, int k, const float* points, int64_t* out, void* workspace, int path) {
  if (B < 0 || N < 0 || k < 0 || k > N || path < 0 || path > 2) return (int)hipErrorInvalidValue;
  if (B == 0 || k == 0) return 0;
  if (points == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
  if (path == 1 && N > FB_LIMIT) return (int)hipErrorInvalidValue;
  if (path == 1 || (path == 0 && N <= FB_LIMIT)) return fps_block((hipStream_t)stream, B, N, k, points, out);
  return fps_rounds((hipStream_t)stream, B, N, k, points, out, workspace);
}
}
