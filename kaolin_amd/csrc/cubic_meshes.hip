// ops.conversions.voxelgrids_to_cubic_meshes: one quad (or two triangles) per exposed voxel face of a dense (B, X, Y, Z) grid,
// the lattice corners merged into shared vertices -- without a sort.
//
//     v(x, y, z)   = the voxel's value as float32, 0 outside the grid
//     face, axis d = a pair of adjacent voxels lo, hi = lo + e_d with r = rint(v(hi) - v(lo)) != 0 (half to even); inverted
//                    (opposite winding) when r == -1.  Its location is the lattice point hi, its quad the unit lattice square
//                    between the two voxels: that point and three EARLIER lattice points.
//     vertex       = a lattice point (i, j, k), 0 <= i <= X ..., that is a corner of some face: one of the 12 pairs among the 8
//                    voxels around it has r != 0.
//
// Every vertex is a point of the L = (X+1)(Y+1)(Z+1) lattice, so lattice order IS "unique, sorted"; the reference's face order
// (axis, then the raster order of the location) is a raster order too.  A rank is a prefix count of a flag:
//
//   1. cm_classify_kernel   one thread per lattice point (z fastest: a wavefront reads runs of contiguous rows), the 8 voxels
//                           around it through the input's strides.  Writes one code byte per point -- bits 0..2 face of axis d,
//                           3..5 inverted, 6 vertex -- and four counts per workgroup (vertices, faces of axis 0, 1, 2) from
//                           __ballot / __popcll and an LDS sum.  A workgroup never straddles two items.  No atomics.
//   2. rows_scan_kernel     (count_scan.h) one workgroup per (item, counter): exclusive scan of the workgroup counts in place,
//                           the total of the row beside it.  bases_kernel<4>: the int64 prefix over the items of the vertex
//                           and quad totals.
//      The host reads the B x 4 totals (ONE synchronising copy for the whole batch) and allocates the outputs.
//   3. cm_vertices_kernel   rank = workgroup offset + ballot prefix inside the workgroup; writes the float3 and the rank into an
//                           int32 array over the lattice (only at the vertices: nothing else is ever gathered).
//   4. cm_faces_kernel      per face bit: the row is the axis offset + the rank within the axis, the four corner ranks are
//                           gathered from the int32 array, int64 rows written directly.
//
// All four read the code byte, so the counts of step 1 and the ranks of steps 3 and 4 agree whatever the values (NaN included).
// Everything is a plain store at an index computed from prefix counts: bit-identical run to run, on any stream.
#include "common.h"
#include "count_scan.h"
#include "profile.h"
#include "../../include/kaolin_amd.h"

namespace {

constexpr int CM_THREADS = 256;
constexpr int CM_WAVES = CM_THREADS / 64;

// the workspace: [totals B x 4 u32][bases B x 2 i64][counts B x 4 x G u32][ranks B x L i32][codes B x L u8], 16-byte aligned parts
struct CmLayout {
  long long L, G, blocks;  // lattice points and workgroups per item; workgroups of the batch
  size_t totals, bases, counts, ranks, codes, bytes;
};
// false: nothing to do (an empty batch) or a lattice the 32-bit indices do not cover
bool cm_layout(long long B, int X, int Y, int Z, CmLayout* lay) {
  if (B <= 0 || X < 0 || Y < 0 || Z < 0) return false;
  const long long lim = (1ll << 31) - 1;
  const long long yz = ((long long)Y + 1) * ((long long)Z + 1);
  if (yz > lim || ((long long)X + 1) > lim / yz) return false;
  lay->L = ((long long)X + 1) * yz;
  lay->G = (lay->L + CM_THREADS - 1) / CM_THREADS;
  if (B > lim / (lay->G > 4 ? lay->G : 4)) return false;  // (the grids: B G and B x 4 workgroups)
  lay->blocks = B * lay->G;
  size_t o = 0;
  lay->totals = o, o += kamd_align16((size_t)B * 4 * 4);
  lay->bases = o, o += kamd_align16((size_t)B * 2 * 8);
  lay->counts = o, o += kamd_align16((size_t)B * 4 * (size_t)lay->G * 4);
  lay->ranks = o, o += kamd_align16((size_t)B * (size_t)lay->L * 4);
  lay->codes = o, o += kamd_align16((size_t)B * (size_t)lay->L);
  lay->bytes = o;
  return true;
}

// the number of set flags in the threads before this one of the workgroup (s_waves: CM_WAVES words per flag, synchronised here)
template <int NF>
__device__ __forceinline__ void cm_block_prefix(const bool (&flag)[NF], unsigned (&prefix)[NF], unsigned (*s_waves)[CM_WAVES]) {
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int f = 0; f < NF; ++f) prefix[f] = ballot_prefix<1>(flag[f] ? 1u : 0u, &s_waves[f][wave]);
  __syncthreads();
#pragma unroll
  for (int f = 0; f < NF; ++f)
    for (int w = 0; w < wave; ++w) prefix[f] += s_waves[f][w];
}

template <typename T>
__global__ __launch_bounds__(CM_THREADS) void cm_classify_kernel(const T* __restrict__ in, long long sn, long long sx, long long sy,
                                                                 long long sz, int X, int Y, int Z, unsigned L, long long G,
                                                                 long long blocks, unsigned char* __restrict__ codes,
                                                                 unsigned* __restrict__ counts) {
  __shared__ unsigned s_waves[4][CM_WAVES];
  const unsigned Z1 = (unsigned)Z + 1u, Y1 = (unsigned)Y + 1u;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const long long item = blk / G, g = blk - item * G;
    const unsigned p = (unsigned)g * CM_THREADS + threadIdx.x;  // (L < 2^31: no wrap)
    unsigned code = 0u;
    if (p < L) {
      const unsigned t = p / Z1;
      const int k = (int)(p - t * Z1), i = (int)(t / Y1), j = (int)(t - (unsigned)i * Y1);
      const T* src = in + item * sn;
      float v[2][2][2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int x = i - 1 + a, y = j - 1 + b, z = k - 1 + c;
            v[a][b][c] = 0.f;
            if (x >= 0 && x < X && y >= 0 && y < Y && z >= 0 && z < Z) v[a][b][c] = grid_value(src[x * sx + y * sy + z * sz]);
          }
      bool any = false;
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          any = any || rintf(v[1][b][c] - v[0][b][c]) != 0.f;
          any = any || rintf(v[b][1][c] - v[b][0][c]) != 0.f;
          any = any || rintf(v[b][c][1] - v[b][c][0]) != 0.f;
        }
      const float r[3] = {rintf(v[1][0][0] - v[0][0][0]), rintf(v[0][1][0] - v[0][0][0]), rintf(v[0][0][1] - v[0][0][0])};
#pragma unroll
      for (int d = 0; d < 3; ++d) code |= (r[d] != 0.f ? 1u << d : 0u) | (r[d] == -1.f ? 8u << d : 0u);
      code |= any ? 64u : 0u;
      codes[item * L + p] = (unsigned char)code;
    }
    const unsigned bit[4] = {64u, 1u, 2u, 4u};  // the order of the counters: vertices, faces of axis 0, 1, 2
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const unsigned long long m = __ballot((code & bit[f]) != 0u);
      if (lane == 0) s_waves[f][wave] = (unsigned)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x < 4) {
      unsigned sum = 0u;
      for (int w = 0; w < CM_WAVES; ++w) sum += s_waves[threadIdx.x][w];
      counts[(item * 4 + threadIdx.x) * G + g] = sum;
    }
    __syncthreads();  // (s_waves is rewritten by the next round)
  }
}

__global__ __launch_bounds__(CM_THREADS) void cm_vertices_kernel(int Y, int Z, unsigned L, long long G, long long blocks,
                                                                 const unsigned char* __restrict__ codes,
                                                                 const unsigned* __restrict__ offsets,
                                                                 const long long* __restrict__ bases, int* __restrict__ ranks,
                                                                 float* __restrict__ verts) {
  __shared__ unsigned s_waves[1][CM_WAVES];
  const unsigned Z1 = (unsigned)Z + 1u, Y1 = (unsigned)Y + 1u;
  for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const long long item = blk / G, g = blk - item * G;
    const unsigned p = (unsigned)g * CM_THREADS + threadIdx.x;
    const bool flag[1] = {p < L && (codes[item * L + p] & 64u) != 0u};
    unsigned prefix[1];
    cm_block_prefix<1>(flag, prefix, s_waves);
    if (flag[0]) {
      const unsigned rank = offsets[item * 4 * G + g] + prefix[0];
      const unsigned t = p / Z1;
      const unsigned k = p - t * Z1, i = t / Y1, j = t - i * Y1;
      ranks[item * L + p] = (int)rank;
      float* o = verts + (bases[2 * item] + rank) * 3;
      o[0] = (float)i;
      o[1] = (float)j;
      o[2] = (float)k;
    }
    __syncthreads();  // (s_waves is rewritten by the next round)
  }
}

// The quad of a face of axis d at the lattice point p, corners in the reference's order (its templates, pinned by the docstring
// example of the Python function): offsets from p in lattice points, sx = (Y+1)(Z+1), sy = Z+1.
//   axis 0: (0,-1,-1) (0,0,-1) (0,0,0) (0,-1,0)     axis 1: (-1,0,-1) (-1,0,0) (0,0,0) (0,0,-1)     axis 2: (-1,-1,0) (0,-1,0) (0,0,0) (-1,0,0)
// An inverted quad is the same one reversed; triangles are corners [0,3,1] (row n) and [2,1,3] (row N + n) of the quad.
template <bool TRI>
__global__ __launch_bounds__(CM_THREADS) void cm_faces_kernel(int Y, int Z, unsigned L, long long G, long long blocks,
                                                              const unsigned char* __restrict__ codes,
                                                              const unsigned* __restrict__ offsets,
                                                              const unsigned* __restrict__ totals,
                                                              const long long* __restrict__ bases, const int* __restrict__ ranks,
                                                              long long* __restrict__ faces) {
  __shared__ unsigned s_waves[3][CM_WAVES];
  const int sy = Z + 1, sx = (Y + 1) * (Z + 1);
  const int corner[3][4] = {{-sy - 1, -1, 0, -sy}, {-sx - 1, -sx, 0, -1}, {-sx - sy, -sy, 0, -sx}};
  for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const long long item = blk / G, g = blk - item * G;
    const unsigned p = (unsigned)g * CM_THREADS + threadIdx.x;
    const unsigned code = p < L ? codes[item * L + p] : 0u;
    const bool flag[3] = {(code & 1u) != 0u, (code & 2u) != 0u, (code & 4u) != 0u};
    unsigned prefix[3];
    cm_block_prefix<3>(flag, prefix, s_waves);
    if ((code & 7u) != 0u) {
      const unsigned n0 = totals[4 * item + 1], n1 = totals[4 * item + 2], n2 = totals[4 * item + 3];
      const long long N = (long long)n0 + n1 + n2;
      const long long axis_first[3] = {0, (long long)n0, (long long)n0 + n1};
      const int* rk = ranks + item * L + p;
      long long* out = faces + bases[2 * item + 1] * (TRI ? 6 : 4);
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        if (!flag[d]) continue;
        const long long n = axis_first[d] + offsets[(item * 4 + 1 + d) * G + g] + prefix[d];
        long long q[4];
        const bool inv = (code & (8u << d)) != 0u;
#pragma unroll
        for (int c = 0; c < 4; ++c) q[c] = rk[corner[d][c]];
        if (inv) {
          long long s = q[0];
          q[0] = q[3], q[3] = s;
          s = q[1];
          q[1] = q[2], q[2] = s;
        }
        if (TRI) {
          long long* a = out + n * 3;
          long long* b = out + (N + n) * 3;
          a[0] = q[0], a[1] = q[3], a[2] = q[1];
          b[0] = q[2], b[1] = q[1], b[2] = q[3];
        } else {
          long long* a = out + n * 4;
          a[0] = q[0], a[1] = q[1], a[2] = q[2], a[3] = q[3];
        }
      }
    }
    __syncthreads();  // (s_waves is rewritten by the next round)
  }
}

template <typename T>
int cm_classify(hipStream_t st, long long B, int X, int Y, int Z, const T* in, long long sn, long long sx, long long sy,
                long long sz, void* workspace) {
  CmLayout lay;
  if (!cm_layout(B, X, Y, Z, &lay) || workspace == nullptr) return (int)hipErrorInvalidValue;
  if (in == nullptr && (long long)X * Y * Z != 0) return (int)hipErrorInvalidValue;
  char* ws = (char*)workspace;
  KAMD_LAUNCH_TIMED(kamd::K_CUBIC_CLASSIFY, (cm_classify_kernel<T>), dim3(count_grid(lay.blocks)), dim3(CM_THREADS), 0, st, in, sn, sx,
                    sy, sz, X, Y, Z, (unsigned)lay.L, lay.G, lay.blocks, (unsigned char*)(ws + lay.codes),
                    (unsigned*)(ws + lay.counts));
  KAMD_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {

size_t kamd_cubic_meshes_workspace(int64_t B, int X, int Y, int Z) {
  CmLayout lay;
  return cm_layout((long long)B, X, Y, Z, &lay) ? lay.bytes : 0;
}

int kamd_cubic_meshes_classify_u8(void* stream, int64_t B, int X, int Y, int Z, const uint8_t* voxelgrids, int64_t stride_n,
                                  int64_t stride_x, int64_t stride_y, int64_t stride_z, void* workspace) {
  return cm_classify<unsigned char>((hipStream_t)stream, (long long)B, X, Y, Z, voxelgrids, (long long)stride_n,
                                    (long long)stride_x, (long long)stride_y, (long long)stride_z, workspace);
}
int kamd_cubic_meshes_classify_f16(void* stream, int64_t B, int X, int Y, int Z, const void* voxelgrids, int64_t stride_n,
                                   int64_t stride_x, int64_t stride_y, int64_t stride_z, void* workspace) {
  return cm_classify<half_bits>((hipStream_t)stream, (long long)B, X, Y, Z, (const half_bits*)voxelgrids, (long long)stride_n,
                              (long long)stride_x, (long long)stride_y, (long long)stride_z, workspace);
}
int kamd_cubic_meshes_classify_f32(void* stream, int64_t B, int X, int Y, int Z, const float* voxelgrids, int64_t stride_n,
                                   int64_t stride_x, int64_t stride_y, int64_t stride_z, void* workspace) {
  return cm_classify<float>((hipStream_t)stream, (long long)B, X, Y, Z, voxelgrids, (long long)stride_n, (long long)stride_x,
                            (long long)stride_y, (long long)stride_z, workspace);
}

int kamd_cubic_meshes_scan(void* stream, int64_t B, int X, int Y, int Z, void* workspace, uint32_t* host_totals) {
  CmLayout lay;
  if (!cm_layout((long long)B, X, Y, Z, &lay) || workspace == nullptr || host_totals == nullptr) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  unsigned* totals = (unsigned*)(ws + lay.totals);
  {
    kamd::ProfScope prof(kamd::K_CUBIC_SCAN, st);
    // a row = one counter of one item; its total is at most the L < 2^31 lattice points
    rows_scan(st, (long long)B * 4, lay.G, (unsigned*)(ws + lay.counts), totals);
    batch_bases<4>(st, (long long)B, (const unsigned*)totals, (long long*)(ws + lay.bases));
  }
  KAMD_CHECK(hipGetLastError());
  // the one host read of the call: the B x 4 totals size the outputs
  KAMD_CHECK(hipMemcpyAsync(host_totals, totals, (size_t)B * 4 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  KAMD_CHECK(hipStreamSynchronize(st));
  return 0;
}

int kamd_cubic_meshes_emit_vertices(void* stream, int64_t B, int X, int Y, int Z, void* workspace, float* verts) {
  CmLayout lay;
  if (!cm_layout((long long)B, X, Y, Z, &lay) || workspace == nullptr || verts == nullptr) return (int)hipErrorInvalidValue;
  char* ws = (char*)workspace;
  KAMD_LAUNCH_TIMED(kamd::K_CUBIC_VERTICES, cm_vertices_kernel, dim3(count_grid(lay.blocks)), dim3(CM_THREADS), 0, (hipStream_t)stream, Y,
                    Z, (unsigned)lay.L, lay.G, lay.blocks, (const unsigned char*)(ws + lay.codes),
                    (const unsigned*)(ws + lay.counts), (const long long*)(ws + lay.bases), (int*)(ws + lay.ranks), verts);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_cubic_meshes_emit_faces(void* stream, int64_t B, int X, int Y, int Z, const void* workspace, int is_trimesh,
                                 int64_t* faces) {
  CmLayout lay;
  if (!cm_layout((long long)B, X, Y, Z, &lay) || workspace == nullptr || faces == nullptr) return (int)hipErrorInvalidValue;
  const char* ws = (const char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (is_trimesh)
    KAMD_LAUNCH_TIMED(kamd::K_CUBIC_FACES, (cm_faces_kernel<true>), dim3(count_grid(lay.blocks)), dim3(CM_THREADS), 0, st, Y, Z,
                      (unsigned)lay.L, lay.G, lay.blocks, (const unsigned char*)(ws + lay.codes),
                      (const unsigned*)(ws + lay.counts), (const unsigned*)(ws + lay.totals),
                      (const long long*)(ws + lay.bases), (const int*)(ws + lay.ranks), (long long*)faces);
  else
    KAMD_LAUNCH_TIMED(kamd::K_CUBIC_FACES, (cm_faces_kernel<false>), dim3(count_grid(lay.blocks)), dim3(CM_THREADS), 0, st, Y, Z,
                      (unsigned)lay.L, lay.G, lay.blocks, (const unsigned char*)(ws + lay.codes),
                      (const unsigned*)(ws + lay.counts), (const unsigned*)(ws + lay.totals),
                      (const long long*)(ws + lay.bases), (const int*)(ws + lay.ranks), (long long*)faces);
  KAMD_RETURN_LAST_ERROR();
}

}  // extern "C"
