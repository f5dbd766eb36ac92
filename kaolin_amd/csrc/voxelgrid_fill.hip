// ops.voxelgrid.fill: an exact 6-connected flood fill of the empty space around the walls of a dense (N, X, Y, Z) grid.
//
//     wall(v)  = value != 0            (0.4, -1 and NaN are walls; -0.0 is empty)
//     outside  = the empty voxels with a path of face-adjacent empty voxels to an empty voxel of the six boundary faces
//     result   = NOT outside           (the walls and every enclosed cavity), one bool per voxel
//
// State: two bit grids in the workspace, `wall` and `outside`, the contiguous Z axis packed into 32-bit words: voxel
// (n, x, y, z) is bit (z & 31) of word ((n X + x) Y + y) W + (z >> 5), W = ceil(Z / 32).  A row is a whole number of words, so
// no word spans two rows or two batch items; the padding bits of a row's last word are walls.  At 256^3 either grid is 2 MB.
//
//   1. vf_pack_kernel      one pass over the dense input (any strides): a wavefront reads 64 voxels of a row, one per lane, and
//                          __ballot makes their two wall words; `outside` starts as the empty voxels of the boundary faces.
//   2. vf_pass_kernel      repeated: a workgroup owns a brick of 16 x 16 rows x 8 words (256 voxels of Z), one row segment per
//                          thread, held in REGISTERS; the segments are mirrored in LDS with a halo of the four neighbouring
//                          row planes read once from the global bit grid.  Each iteration ORs in the four X / Y neighbours'
//                          words and then floods along Z through whole runs of empty bits: with e = the empty bits and
//                          s = the seeds, (e + s) carries every seed to the end of its run, so e & ((e + s) ^ e) is the flood
//                          towards the high bits, bit 31 is the carry into the next word, and the same on the bit-reversed
//                          words floods the other way (one sweep up and one down close a row).  The brick iterates to ITS
//                          fixed point (__syncthreads_or), writes back the segments that changed and raises `last_changed`.
//                          A brick reads its neighbours only through the global grid; what it reads may be older than what
//                          another workgroup of the same launch has just written, which is harmless: the set only grows, any
//                          state read is a subset of the answer, and kernel boundaries publish everything.
//   3. vf_unpack_kernel    one pass writing NOT outside as bytes (16 per lane when Z allows).
//
// Termination: one monotone word, `last_changed` = the number of the last pass in which a brick changed (0 = the pack kernel,
// which seeds the boundary).  Pass p (1, 2, ...) works only if last_changed >= p - 1, i.e. its predecessor changed something,
// and raises the word to p (atomicMax) when one of its bricks changes; otherwise it returns at once and writes nothing, so
// every later pass is idle too and nothing ever has to be cleared.  (A workgroup of pass p that reads the word while others
// raise it sees p - 1 or p: it works either way.)  A pass in which no brick changed anything saw the final state everywhere:
// that is the fixed point, for every grid, after as many passes as the longest corridor needs -- no constant bounds them.
// The host enqueues a batch of passes (2, then 4, then VF_POLL each), reads the word back, and goes on while the batch's last
// pass changed something: the call synchronises its stream and cannot be captured in a graph.  No grid-wide barrier, no
// cooperative launch: a workgroup never waits for another.
#include "common.h"
#include "profile.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr int VF_THREADS = 256;
constexpr int VF_BX = 16, VF_BY = 16;  // rows of a brick along X and Y (one thread per row)
constexpr int VF_WZ = 8;               // words of a row segment (256 voxels of Z)
constexpr int VF_POLL = 8;             // most passes enqueued between two host reads of `last_changed`
constexpr int VF_CTRL_WORDS = 16;      // [0] last_changed, [1] passes that worked; 64 bytes in all

struct vf_half {
  unsigned short bits;
};
template <typename T>
__device__ __forceinline__ bool vf_is_wall(T v) {
  return v != (T)0;
}
template <>
__device__ __forceinline__ bool vf_is_wall<vf_half>(vf_half v) {
  return (v.bits & 0x7fffu) != 0;  // everything but +-0, NaN included
}

template <typename T>
__global__ __launch_bounds__(VF_THREADS) void vf_pack_kernel(const T* __restrict__ in, long long sn, long long sx, long long sy,
                                                             long long sz, int X, int Y, int Z, int W, long long rows,
                                                             unsigned* __restrict__ wall, unsigned* __restrict__ outside,
                                                             unsigned* __restrict__ ctrl) {
  if (blockIdx.x == 0 && threadIdx.x < 2) ctrl[threadIdx.x] = 0u;
  const int lane = threadIdx.x & 63;
  const int chunks = (Z + 63) >> 6;
  const long long nwaves = (long long)gridDim.x * (VF_THREADS / 64);
  for (long long row = (long long)blockIdx.x * (VF_THREADS / 64) + (threadIdx.x >> 6); row < rows; row += nwaves) {
    const long long t = row / Y;
    const int y = (int)(row - t * Y);
    const long long n = t / X;
    const int x = (int)(t - n * X);
    const T* src = in + n * sn + x * sx + y * sy;
    const bool face = x == 0 || x == X - 1 || y == 0 || y == Y - 1;
    for (int c0 = 0; c0 < chunks; c0 += 4) {  // four loads in flight per lane (a 256-voxel row is one round)
      bool w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int z = (c0 + j) * 64 + lane;
        w[j] = true;  // padding is wall
        if (z < Z) w[j] = vf_is_wall(src[z * sz]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = c0 + j;
        if (c >= chunks) break;  // (uniform)
        const unsigned long long m = __ballot(w[j]);
        const int k = 2 * c + lane;
        if (lane < 2 && k < W) {
          const unsigned wm = lane ? (unsigned)(m >> 32) : (unsigned)m;
          unsigned seed = face ? ~0u : 0u;
          if (k == 0) seed |= 1u;
          if (k == ((Z - 1) >> 5)) seed |= 1u << ((Z - 1) & 31);
          wall[row * W + k] = wm;
          outside[row * W + k] = seed & ~wm;
        }
      }
    }
  }
}

// towards the high bits: the seeds `s` (a subset of the empty bits `e`) flood to the end of their runs of empty bits
__device__ __forceinline__ unsigned vf_flood_up(unsigned e, unsigned s) { return s | (e & ((e + s) ^ e)); }

__global__ __launch_bounds__(VF_THREADS) void vf_pass_kernel(int X, int Y, int W, int bricks_x, int bricks_y, int bricks_z,
                                                             long long bricks, const unsigned* __restrict__ wall,
                                                             unsigned* outside, unsigned* ctrl, unsigned pass) {
  // [x + 1][y + 1][word]; the odd row length spreads the 16 threads of a y run over the banks
  __shared__ unsigned s_out[VF_BX + 2][VF_BY + 2][VF_WZ + 1];
  if (ctrl[0] + 1u < pass) return;  // the pass before changed nothing: the fixed point is reached (uniform over the grid)
  if (blockIdx.x == 0 && threadIdx.x == 0) ctrl[1] += 1;
  const int tx = threadIdx.x >> 4, ty = threadIdx.x & 15;  // adjacent threads: adjacent y = adjacent rows in memory
  for (long long b = blockIdx.x; b < bricks; b += gridDim.x) {
    long long r = b;
    const int bz = (int)(r % bricks_z);
    r /= bricks_z;
    const int by = (int)(r % bricks_y);
    r /= bricks_y;
    const int bx = (int)(r % bricks_x);
    const long long n = r / bricks_x;
    const int x0 = bx * VF_BX, y0 = by * VF_BY, w0 = bz * VF_WZ;
    const int x = x0 + tx, y = y0 + ty;
    const bool valid = x < X && y < Y;
    const long long base = ((n * X + x) * Y + y) * W;  // only dereferenced when valid

    unsigned wl[VF_WZ], o[VF_WZ];
#pragma unroll
    for (int k = 0; k < VF_WZ; ++k) {
      const bool in = valid && w0 + k < W;
      wl[k] = in ? wall[base + w0 + k] : ~0u;
      o[k] = in ? outside[base + w0 + k] : 0u;
      s_out[tx + 1][ty + 1][k] = o[k];
    }
    // the two bits across the segment's ends along Z
    const unsigned below = (valid && w0 > 0) ? outside[base + w0 - 1] >> 31 : 0u;
    const unsigned above = (valid && w0 + VF_WZ < W) ? outside[base + w0 + VF_WZ] & 1u : 0u;
    // halo: the row planes x0 - 1, x0 + 16, y0 - 1, y0 + 16 (no corners: connectivity is by faces); outside the array: nothing
    for (int i = threadIdx.x; i < 4 * 16 * VF_WZ; i += VF_THREADS) {
      const int side = i >> 7, j = (i >> 3) & 15, k = i & 7;
      int hx, hy, lx, ly;
      if (side < 2) {
        lx = side == 0 ? 0 : VF_BX + 1;
        ly = j + 1;
      } else {
        lx = j + 1;
        ly = side == 2 ? 0 : VF_BY + 1;
      }
      hx = x0 + lx - 1;
      hy = y0 + ly - 1;
      unsigned v = 0u;
      if (hx >= 0 && hx < X && hy >= 0 && hy < Y && w0 + k < W) v = outside[((n * X + hx) * Y + hy) * W + w0 + k];
      s_out[lx][ly][k] = v;
    }

    unsigned mine = 0u;  // this thread's segment differs from what it loaded
    bool brick_changed = false;
    for (;;) {
      __syncthreads();
      unsigned no[VF_WZ];
#pragma unroll
      for (int k = 0; k < VF_WZ; ++k) {
        const unsigned nb = s_out[tx][ty + 1][k] | s_out[tx + 2][ty + 1][k] | s_out[tx + 1][ty][k] | s_out[tx + 1][ty + 2][k];
        no[k] = o[k] | (nb & ~wl[k]);
      }
      unsigned c = below;
#pragma unroll
      for (int k = 0; k < VF_WZ; ++k) {
        const unsigned e = ~wl[k];
        no[k] = vf_flood_up(e, no[k] | (c & e));
        c = no[k] >> 31;
      }
      c = above;
#pragma unroll
      for (int k = VF_WZ - 1; k >= 0; --k) {
        const unsigned e = __brev(~wl[k]);
        const unsigned f = vf_flood_up(e, __brev(no[k]) | (c & e));
        c = f >> 31;
        no[k] = __brev(f);
      }
      unsigned ch = 0u;
#pragma unroll
      for (int k = 0; k < VF_WZ; ++k) {
        ch |= no[k] ^ o[k];
        o[k] = no[k];
      }
      mine |= ch;
      if (!__syncthreads_or(ch != 0u)) break;  // (every thread has read LDS by now)
      brick_changed = true;
      if (ch != 0u) {
#pragma unroll
        for (int k = 0; k < VF_WZ; ++k) s_out[tx + 1][ty + 1][k] = o[k];
      }
    }
    if (mine != 0u) {  // (implies valid: a segment outside the array is all wall)
#pragma unroll
      for (int k = 0; k < VF_WZ; ++k)
        if (w0 + k < W) outside[base + w0 + k] = o[k];
    }
    if (brick_changed && threadIdx.x == 0) atomicMax(&ctrl[0], pass);
  }
}

// bits 0..3 -> bytes 0..3 (the four shifted copies do not overlap)
__device__ __forceinline__ unsigned vf_spread4(unsigned b) { return ((b & 0xFu) * 0x00204081u) & 0x01010101u; }

template <int VEC>
__global__ __launch_bounds__(VF_THREADS) void vf_unpack_kernel(const unsigned* __restrict__ outside, int Z, int W, long long rows,
                                                               unsigned char* __restrict__ out) {
  const int per_row = Z / VEC;
  const long long total = rows * per_row, stride = (long long)gridDim.x * VF_THREADS;
  for (long long i = (long long)blockIdx.x * VF_THREADS + threadIdx.x; i < total; i += stride) {
    const long long row = i / per_row;
    const int z0 = (int)(i - row * per_row) * VEC;
    const unsigned b = ~outside[row * W + (z0 >> 5)] >> (z0 & 31);
    unsigned char* dst = out + row * Z + z0;
    if (VEC == 1)
      *dst = (unsigned char)(b & 1u);
    else if (VEC == 4)
      *(unsigned*)dst = vf_spread4(b);
    else
      *(uint4*)dst = make_uint4(vf_spread4(b), vf_spread4(b >> 4), vf_spread4(b >> 8), vf_spread4(b >> 12));
  }
}

unsigned vf_blocks(long long work_items, int per_block, int blocks_per_cu) {
  long long blocks = (work_items + per_block - 1) / per_block;
  const long long cap = (long long)KAMD_NUM_CU * blocks_per_cu;
  return (unsigned)(blocks < cap ? (blocks > 0 ? blocks : 1) : cap);
}

template <typename T>
int vf_fill(hipStream_t st, long long N, int X, int Y, int Z, const T* in, long long sn, long long sx, long long sy, long long sz,
            unsigned char* out, void* workspace, int* host_stats) {
  if (N < 0 || X < 0 || Y < 0 || Z < 0) return (int)hipErrorInvalidValue;
  if (host_stats != nullptr) host_stats[0] = host_stats[1] = host_stats[2] = 0;
  if (N == 0 || X == 0 || Y == 0 || Z == 0) return 0;
  if (in == nullptr || out == nullptr || workspace == nullptr) return (int)hipErrorInvalidValue;
  const int W = (Z + 31) / 32;
  const long long rows = N * X * Y;
  unsigned* ctrl = (unsigned*)workspace;
  unsigned* wall = ctrl + VF_CTRL_WORDS;
  unsigned* outside = wall + rows * W;

  KAMD_LAUNCH_TIMED(kamd::K_VOXFILL_PACK, (vf_pack_kernel<T>), dim3(vf_blocks(rows, VF_THREADS / 64, 16)), dim3(VF_THREADS), 0, st,
                    in, sn, sx, sy, sz, X, Y, Z, W, rows, wall, outside, ctrl);
  KAMD_CHECK(hipGetLastError());

  const int bricks_x = kamd_cdiv(X, VF_BX), bricks_y = kamd_cdiv(Y, VF_BY), bricks_z = kamd_cdiv(W, VF_WZ);
  const long long bricks = N * bricks_x * bricks_y * bricks_z;
  const unsigned pass_blocks = vf_blocks(bricks, 1, 16);
  // One changing pass and the one that confirms it are the common case (a shell whose outside is reached along Z): the
  // first batch is 2 passes, then 4, then VF_POLL each.  The read lands in pageable memory (the runtime stages 8 bytes
  // through its own pinned buffer); the stream synchronise that follows is the cost of a poll either way.
  unsigned h[2] = {0u, 0u};
  unsigned pass = 0;
  int polls = 0, batch = 2;
  do {
    if (pass > 0x7fffff00u) return (int)hipErrorInvalidValue;  // (2^31 passes: no grid that fits in memory needs them)
    for (int i = 0; i < batch; ++i) {
      ++pass;
      KAMD_LAUNCH_TIMED(kamd::K_VOXFILL_PASS, vf_pass_kernel, dim3(pass_blocks), dim3(VF_THREADS), 0, st, X, Y, W, bricks_x,
                        bricks_y, bricks_z, bricks, (const unsigned*)wall, outside, ctrl, pass);
    }
    KAMD_CHECK(hipGetLastError());
    KAMD_CHECK(hipMemcpyAsync(h, ctrl, sizeof(h), hipMemcpyDeviceToHost, st));
    KAMD_CHECK(hipStreamSynchronize(st));
    ++polls;
    batch = batch * 2 < VF_POLL ? batch * 2 : VF_POLL;
  } while (h[0] >= pass);  // the last pass launched changed something
  if (host_stats != nullptr) {
    host_stats[0] = (int)h[1];
    host_stats[1] = (int)pass;
    host_stats[2] = polls;
  }

  if (Z % 16 == 0 && ((uintptr_t)out & 15) == 0)
    KAMD_LAUNCH_TIMED(kamd::K_VOXFILL_UNPACK, (vf_unpack_kernel<16>), dim3(vf_blocks(rows * (Z / 16), VF_THREADS, 16)),
                      dim3(VF_THREADS), 0, st, (const unsigned*)outside, Z, W, rows, out);
  else if (Z % 4 == 0 && ((uintptr_t)out & 3) == 0)
    KAMD_LAUNCH_TIMED(kamd::K_VOXFILL_UNPACK, (vf_unpack_kernel<4>), dim3(vf_blocks(rows * (Z / 4), VF_THREADS, 16)),
                      dim3(VF_THREADS), 0, st, (const unsigned*)outside, Z, W, rows, out);
  else
    KAMD_LAUNCH_TIMED(kamd::K_VOXFILL_UNPACK, (vf_unpack_kernel<1>), dim3(vf_blocks(rows * Z, VF_THREADS, 16)), dim3(VF_THREADS), 0,
                      st, (const unsigned*)outside, Z, W, rows, out);
  KAMD_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {

size_t kamd_voxelgrid_fill_workspace(int64_t N, int X, int Y, int Z) {
  if (N <= 0 || X <= 0 || Y <= 0 || Z <= 0) return 0;
  const size_t words = (size_t)N * (size_t)X * (size_t)Y * (size_t)((Z + 31) / 32);
  return (size_t)VF_CTRL_WORDS * 4 + 2 * words * 4;
}

#define KAMD_VF_ENTRY(SFX, CT, T)                                                                                            \
  int kamd_voxelgrid_fill_##SFX(void* stream, int64_t N, int X, int Y, int Z, const CT* voxelgrids, int64_t stride_n,         \
                                int64_t stride_x, int64_t stride_y, int64_t stride_z, uint8_t* filled, void* workspace,     \
                                int32_t* host_stats) {                                                                      \
    return vf_fill<T>((hipStream_t)stream, (long long)N, X, Y, Z, (const T*)voxelgrids, (long long)stride_n,                \
                      (long long)stride_x, (long long)stride_y, (long long)stride_z, filled, workspace, host_stats);        \
  }
KAMD_VF_ENTRY(u8, uint8_t, unsigned char)
KAMD_VF_ENTRY(i32, int32_t, int)
KAMD_VF_ENTRY(i64, int64_t, long long)
KAMD_VF_ENTRY(f16, void, vf_half)
KAMD_VF_ENTRY(f32, float, float)
KAMD_VF_ENTRY(f64, double, double)
#undef KAMD_VF_ENTRY

}  // extern "C"
