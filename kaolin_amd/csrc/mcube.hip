// ops.conversions.voxelgrids_to_trianglemeshes: marching cubes over a dense (B, X, Y, Z) grid, the sibling of cubic_meshes.hip.
//
//     field        = the grid's values as float32 with an implicit border of zeros (never materialised): lattice point q holds
//                    voxel q - 1, or 0 outside.  `border == 0` (the reference's unbatched operator): the grid as given, point q
//                    holds voxel q.
//     cell p       = the cube whose corner 0 is the lattice point p; corners, edges and the case byte as in mcube_table.h
//                    (bit k set iff value(corner k) < iso; NaN is not below).
//     vertex       = a crossed lattice edge.  It belongs to the cell at its LOWER end, as one of the three edges leaving that
//                    cell's corner 0 (along dim0, dim1, dim2): own bits bit0^bit4, bit0^bit3, bit0^bit1 of the case byte.
//                    Vertex order = raster order of that cell, then the axis.
//     position     = along dim0: p_lo + (iso - f_lo) / (f_hi - f_lo); along dim1 and dim2: p_hi - (iso - f_hi) / (f_lo - f_hi)
//                    (the reference kernel's operands; one correctly rounded division, one rounded add or subtract).
//
// The lattice has one cell per point that is the lower end of some edge: (X+1)(Y+1)(Z+1) cells with the border, X Y Z points
// without it -- there the points of the last layer of an axis own edges but are no real cells: the field repeats past them
// (such an edge is never crossed) and they get no triangles.
//
//   1. mc_classify_kernel   one thread per cell (dim2 fastest), the 8 values through the input's strides.  Writes the case byte and
//                           two counts per workgroup (own vertices, triangles) from __ballot / __popcll and an LDS sum.  A
//                           workgroup never straddles two items.  No atomics.
//   2. rows_scan_kernel     (count_scan.h) one workgroup per (item, counter): exclusive scan of the workgroup counts in place,
//                           the total beside it.  bases_kernel<2>: the int64 prefix over the items.  The host reads the B x 2
//                           totals (ONE synchronising copy for the whole batch) and allocates the outputs.
//   3. mc_vertices_kernel   first rank = workgroup offset + ballot prefix; writes the cell's float3s and its first rank into an
//                           int32 array over the lattice (only where the cell owns a vertex: nothing else is ever gathered).
//   4. mc_faces_kernel      walks the cell's table row (the 4 KB table sits in LDS: lanes index it divergently).  An edge id maps
//                           to its owning neighbour cell and axis; the vertex id is that cell's first rank + its own bits below
//                           the axis.  int64 rows written directly.
//   mc_backward_kernel      one thread per grid value gathers over its six incident lattice edges in a fixed order (dim0 -, dim0 +,
//                           dim1 -, dim1 +, dim2 -, dim2 +), float32 accumulation, no atomics.
//
// Every step reads the case byte, so counts, ranks and ids agree whatever the values (NaN included).  Everything is a plain store
// at an index computed from prefix counts: bit-identical run to run, on any stream.  Indices derived from data (vertex rows, face
// rows, the owner cell) are compared with their buffer's size before use.
#include "common.h"
#include "count_scan.h"
#include "../../include/kaolin_amd.h"

#define KAMD_MCUBE_QUALIFIER __device__ const
#include "mcube_table.h"

namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_WAVES = MC_THREADS / 64;

// per cell edge: the corner at its lower end as (dim0, dim1, dim2) offsets from the cell and the edge's axis, 5 bits each:
// offset0 << 4 | offset1 << 3 | offset2 << 2 | axis, edge e at bits [5 e, 5 e + 5).  Edges (0,1) (1,2) (2,3) (3,0) (4,5) (5,6)
// (6,7) (7,4) (0,4) (1,5) (2,6) (3,7) of corners 0:(0,0,0) 1:(0,0,1) 2:(0,1,1) 3:(0,1,0) 4:(1,0,0) 5:(1,0,1) 6:(1,1,1) 7:(1,1,0).
constexpr unsigned long long mc_edge(int e, int o0, int o1, int o2, int axis) {
  return (unsigned long long)(o0 << 4 | o1 << 3 | o2 << 2 | axis) << (5 * e);
}
constexpr unsigned long long MC_EDGES = mc_edge(0, 0, 0, 0, 2) | mc_edge(1, 0, 0, 1, 1) | mc_edge(2, 0, 1, 0, 2) | mc_edge(3, 0, 0, 0, 1) |
                                        mc_edge(4, 1, 0, 0, 2) | mc_edge(5, 1, 0, 1, 1) | mc_edge(6, 1, 1, 0, 2) | mc_edge(7, 1, 0, 0, 1) |
                                        mc_edge(8, 0, 0, 0, 0) | mc_edge(9, 0, 0, 1, 0) | mc_edge(10, 0, 1, 1, 0) | mc_edge(11, 0, 1, 0, 0);

// the own bits of a cell (axis a at bit a) from its case byte
__device__ __forceinline__ unsigned mc_own(unsigned code) {
  return ((code ^ (code >> 4)) & 1u) | (((code ^ (code >> 3)) & 1u) << 1) | (((code ^ (code >> 1)) & 1u) << 2);
}

template <typename T>
struct McGrid {
  const T* in;
  long long sn, sx, sy, sz;  // element strides
  int X, Y, Z;               // the grid
  int NX, NY, NZ;            // the lattice
  int border;
};

// the field at the lattice point (q0, q1, q2), q >= 0
template <typename T>
__device__ __forceinline__ float mc_fetch(const McGrid<T>& gr, const T* src, int q0, int q1, int q2) {
  int x, y, z;
  if (gr.border) {
    x = q0 - 1, y = q1 - 1, z = q2 - 1;
    if (x < 0 || x >= gr.X || y < 0 || y >= gr.Y || z < 0 || z >= gr.Z) return 0.f;
  } else {
    x = q0 < gr.X ? q0 : gr.X - 1, y = q1 < gr.Y ? q1 : gr.Y - 1, z = q2 < gr.Z ? q2 : gr.Z - 1;
  }
  return grid_value(src[x * gr.sx + y * gr.sy + z * gr.sz]);
}

// the workspace: [totals B x 2 u32][bases B x 2 i64][counts B x 2 x G u32][ranks B x L i32][codes B x L u8], 16-byte aligned parts
struct McLayout {
  int NX, NY, NZ;
  long long L, G, blocks;  // cells and workgroups per item; workgroups of the batch
  size_t totals, bases, counts, ranks, codes, bytes;
};
// false: nothing to do (an empty batch or grid) or a lattice whose 3 L possible vertices the 32-bit indices do not cover
bool mc_layout(long long B, int X, int Y, int Z, int border, McLayout* lay) {
  if (B <= 0 || X < 1 || Y < 1 || Z < 1) return false;
  const long long lim = ((1ll << 31) - 1) / 3;
  const long long nx = (long long)X + (border ? 1 : 0), ny = (long long)Y + (border ? 1 : 0), nz = (long long)Z + (border ? 1 : 0);
  if (ny * nz > lim || nx > lim / (ny * nz)) return false;
  lay->NX = (int)nx, lay->NY = (int)ny, lay->NZ = (int)nz;
  lay->L = nx * ny * nz;
  lay->G = (lay->L + MC_THREADS - 1) / MC_THREADS;
  if (B > ((1ll << 31) - 1) / (lay->G > 2 ? lay->G : 2)) return false;  // (the grids: B G and B x 2 workgroups)
  lay->blocks = B * lay->G;
  size_t o = 0;
  lay->totals = o, o += kamd_align16((size_t)B * 2 * 4);
  lay->bases = o, o += kamd_align16((size_t)B * 2 * 8);
  lay->counts = o, o += kamd_align16((size_t)B * 2 * (size_t)lay->G * 4);
  lay->ranks = o, o += kamd_align16((size_t)B * (size_t)lay->L * 4);
  lay->codes = o, o += kamd_align16((size_t)B * (size_t)lay->L);
  lay->bytes = o;
  return true;
}

template <typename T>
__global__ __launch_bounds__(MC_THREADS) void mc_classify_kernel(McGrid<T> gr, float iso, unsigned L, long long G, long long blocks,
                                                                 unsigned char* __restrict__ codes, unsigned* __restrict__ counts) {
  __shared__ unsigned s_waves[2][MC_WAVES];
  __shared__ unsigned char s_ntri[256];
  s_ntri[threadIdx.x] = kamd_mcube_num_triangles[threadIdx.x];
  __syncthreads();
  const unsigned NZ = (unsigned)gr.NZ, NY = (unsigned)gr.NY;
  for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const long long item = blk / G, g = blk - item * G;
    const unsigned p = (unsigned)g * MC_THREADS + threadIdx.x;  // (L < 2^31: no wrap)
    unsigned nv = 0u, nt = 0u;
    if (p < L) {
      const unsigned t = p / NZ;
      const int k = (int)(p - t * NZ), i = (int)(t / NY), j = (int)(t - (unsigned)i * NY);
      const T* src = gr.in + item * gr.sn;
      unsigned code = 0u;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        // corners 0:(0,0,0) 1:(0,0,1) 2:(0,1,1) 3:(0,1,0) 4:(1,0,0) 5:(1,0,1) 6:(1,1,1) 7:(1,1,0)
        const int o0 = c >> 2, o1 = (c >> 1) & 1, o2 = (c ^ (c >> 1)) & 1;
        code |= mc_fetch(gr, src, i + o0, j + o1, k + o2) < iso ? 1u << c : 0u;
      }
      codes[item * L + p] = (unsigned char)code;
      nv = (unsigned)__popc(mc_own(code));
      const bool real = gr.border || (i < gr.NX - 1 && j < gr.NY - 1 && k < gr.NZ - 1);
      nt = real ? s_ntri[code] : 0u;
    }
    const int wave = threadIdx.x >> 6;
    ballot_prefix<2>(nv, &s_waves[0][wave]);
    ballot_prefix<3>(nt, &s_waves[1][wave]);
    __syncthreads();
    if (threadIdx.x < 2) {
      unsigned sum = 0u;
      for (int w = 0; w < MC_WAVES; ++w) sum += s_waves[threadIdx.x][w];
      counts[(item * 2 + threadIdx.x) * G + g] = sum;
    }
    __syncthreads();  // (s_waves is rewritten by the next round)
  }
}

template <typename T>
__global__ __launch_bounds__(MC_THREADS) void mc_vertices_kernel(McGrid<T> gr, float iso, unsigned L, long long G, long long blocks,
                                                                 const unsigned char* __restrict__ codes,
                                                                 const unsigned* __restrict__ offsets,
                                                                 const long long* __restrict__ bases, int* __restrict__ ranks,
                                                                 float* __restrict__ verts, long long verts_rows) {
  __shared__ unsigned s_waves[MC_WAVES];
  const unsigned NZ = (unsigned)gr.NZ, NY = (unsigned)gr.NY;
  const int wave = threadIdx.x >> 6;
  for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const long long item = blk / G, g = blk - item * G;
    const unsigned p = (unsigned)g * MC_THREADS + threadIdx.x;
    const unsigned own = p < L ? mc_own(codes[item * L + p]) : 0u;
    unsigned prefix = ballot_prefix<2>((unsigned)__popc(own), &s_waves[wave]);
    __syncthreads();
    for (int w = 0; w < wave; ++w) prefix += s_waves[w];
    if (own != 0u) {
      const unsigned rank = offsets[item * 2 * G + g] + prefix;  // the cell's first vertex within its item
      ranks[item * L + p] = (int)rank;
      const unsigned t = p / NZ;
      const int k = (int)(p - t * NZ), i = (int)(t / NY), j = (int)(t - (unsigned)i * NY);
      const T* src = gr.in + item * gr.sn;
      const float f = mc_fetch(gr, src, i, j, k);
      long long row = bases[2 * item] + rank;
      if (own & 1u) {
        const float h = mc_fetch(gr, src, i + 1, j, k);
        if (row < verts_rows) {
          float* o = verts + row * 3;
          o[0] = (float)i + (iso - f) / (h - f);
          o[1] = (float)j;
          o[2] = (float)k;
        }
        ++row;
      }
      if (own & 2u) {
        const float h = mc_fetch(gr, src, i, j + 1, k);
        if (row < verts_rows) {
          float* o = verts + row * 3;
          o[0] = (float)i;
          o[1] = (float)(j + 1) - (iso - h) / (f - h);
          o[2] = (float)k;
        }
        ++row;
      }
      if (own & 4u) {
        const float h = mc_fetch(gr, src, i, j, k + 1);
        if (row < verts_rows) {
          float* o = verts + row * 3;
          o[0] = (float)i;
          o[1] = (float)j;
          o[2] = (float)(k + 1) - (iso - h) / (f - h);
        }
      }
    }
    __syncthreads();  // (s_waves is rewritten by the next round)
  }
}

__global__ __launch_bounds__(MC_THREADS) void mc_faces_kernel(int NX, int NY, int NZ, int border, unsigned L, long long G,
                                                              long long blocks, const unsigned char* __restrict__ codes,
                                                              const unsigned* __restrict__ offsets,
                                                              const long long* __restrict__ bases, const int* __restrict__ ranks,
                                                              long long* __restrict__ faces, long long faces_rows) {
  __shared__ unsigned char s_table[256 * KAMD_MCUBE_ROW];
  __shared__ unsigned char s_ntri[256];
  __shared__ unsigned s_waves[MC_WAVES];
  for (int n = threadIdx.x; n < 256 * KAMD_MCUBE_ROW; n += MC_THREADS) s_table[n] = kamd_mcube_table[n];
  s_ntri[threadIdx.x] = kamd_mcube_num_triangles[threadIdx.x];
  __syncthreads();
  const int wave = threadIdx.x >> 6;
  const unsigned sx = (unsigned)NY * (unsigned)NZ;
  for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const long long item = blk / G, g = blk - item * G;
    const unsigned p = (unsigned)g * MC_THREADS + threadIdx.x;
    unsigned code = 0u, nt = 0u;
    if (p < L) {
      code = codes[item * L + p];
      const unsigned t = p / (unsigned)NZ;
      const int k = (int)(p - t * (unsigned)NZ), i = (int)(t / (unsigned)NY), j = (int)(t - (unsigned)i * (unsigned)NY);
      const bool real = border || (i < NX - 1 && j < NY - 1 && k < NZ - 1);
      nt = real ? s_ntri[code] : 0u;
    }
    unsigned prefix = ballot_prefix<3>(nt, &s_waves[wave]);
    __syncthreads();
    for (int w = 0; w < wave; ++w) prefix += s_waves[w];
    if (nt != 0u) {
      long long row = bases[2 * item + 1] + offsets[(item * 2 + 1) * G + g] + prefix;
      const unsigned char* tri = s_table + code * KAMD_MCUBE_ROW;
      const unsigned char* cd = codes + item * L;
      const int* rk = ranks + item * L;
      for (unsigned t = 0; t < nt; ++t, ++row) {
        long long id[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const unsigned e = tri[3 * t + c];
          const unsigned q = e < 12u ? (unsigned)(MC_EDGES >> (5u * e)) & 31u : 0u;
          const unsigned owner = p + ((q >> 4) & 1u) * sx + ((q >> 3) & 1u) * (unsigned)NZ + ((q >> 2) & 1u);
          id[c] = 0;
          if (owner < L) id[c] = (long long)rk[owner] + __popc(mc_own(cd[owner]) & ((1u << (q & 3u)) - 1u));
        }
        if (row < faces_rows) {
          long long* o = faces + row * 3;
          o[0] = id[0], o[1] = id[1], o[2] = id[2];
        }
      }
    }
    __syncthreads();  // (s_waves is rewritten by the next round)
  }
}

// grad[b, x, y, z] = sum over the six lattice edges at the voxel of grad_verts[vertex of the edge, axis] * d position / d value.
// On an edge from A to B (dim0: A = low end; dim1, dim2: A = high end) the position is p_A + s (iso - f_A) / (f_B - f_A),
// s = +1 / -1, so d/df_A = s (iso - f_B) / d^2 and d/df_B = -s (iso - f_A) / d^2 with d = f_B - f_A: in both cases
// +-(iso - f_other) / d^2, + when the voxel is the edge's low end.  Six rounded operations per term (iso - f_other, d, d d: 3,
// the quotient: 5, times the gradient: 6), then five additions.
template <typename T>
__global__ __launch_bounds__(MC_THREADS) void mc_backward_kernel(McGrid<T> gr, float iso, unsigned L, long long total,
                                                                 const unsigned char* __restrict__ codes,
                                                                 const long long* __restrict__ bases, const int* __restrict__ ranks,
                                                                 const float* __restrict__ grad_verts, long long verts_rows,
                                                                 T* __restrict__ grad) {
  const long long stride = (long long)gridDim.x * MC_THREADS;
  const unsigned step[3] = {(unsigned)gr.NY * (unsigned)gr.NZ, (unsigned)gr.NZ, 1u};
  for (long long n = (long long)blockIdx.x * MC_THREADS + threadIdx.x; n < total; n += stride) {
    long long r = n;
    const int z = (int)(r % gr.Z);
    r /= gr.Z;
    const int y = (int)(r % gr.Y);
    r /= gr.Y;
    const int x = (int)(r % gr.X);
    const long long item = r / gr.X;
    const T* src = gr.in + item * gr.sn;
    const int q[3] = {x + 1, y + 1, z + 1};  // the voxel's lattice point
    const unsigned p = ((unsigned)q[0] * (unsigned)gr.NY + (unsigned)q[1]) * (unsigned)gr.NZ + (unsigned)q[2];
    const float f = grid_value(src[x * gr.sx + y * gr.sy + z * gr.sz]);
    const unsigned char* cd = codes + item * L;
    const int* rk = ranks + item * L;
    const long long base = bases[2 * item];
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int up = 0; up < 2; ++up) {
        // up == 0: the edge that ends at the voxel (the voxel is its high end); up == 1: the edge that leaves it
        const unsigned lower = up ? p : p - step[a];
        if (lower >= L) continue;
        const unsigned own = mc_own(cd[lower]);
        if (((own >> a) & 1u) == 0u) continue;
        const long long row = base + rk[lower] + __popc(own & ((1u << a) - 1u));
        if (row < 0 || row >= verts_rows) continue;
        const int o = up ? 1 : -1;
        const float other = mc_fetch(gr, src, q[0] + (a == 0 ? o : 0), q[1] + (a == 1 ? o : 0), q[2] + (a == 2 ? o : 0));
        // A -> B: dim0 low -> high, dim1 and dim2 high -> low
        const bool self_is_a = (a == 0) == (up == 1);
        const float d = self_is_a ? other - f : f - other;
        const float term = grad_verts[row * 3 + a] * ((iso - other) / (d * d));
        acc += up ? term : -term;
      }
    grid_store(grad + n, acc);
  }
}

template <typename T>
bool mc_make_grid(long long B, int X, int Y, int Z, int border, const T* in, long long sn, long long sx, long long sy, long long sz,
                  McLayout* lay, McGrid<T>* gr) {
  if (!mc_layout(B, X, Y, Z, border, lay) || in == nullptr) return false;
  *gr = McGrid<T>{in, sn, sx, sy, sz, X, Y, Z, lay->NX, lay->NY, lay->NZ, border ? 1 : 0};
  return true;
}

template <typename T>
int mc_classify(hipStream_t st, long long B, int X, int Y, int Z, int border, const T* in, long long sn, long long sx, long long sy,
                long long sz, float iso, void* workspace) {
  McLayout lay;
  McGrid<T> gr;
  if (!mc_make_grid(B, X, Y, Z, border, in, sn, sx, sy, sz, &lay, &gr) || workspace == nullptr || !(iso == iso))
    return (int)hipErrorInvalidValue;
  char* ws = (char*)workspace;
  hipLaunchKernelGGL((mc_classify_kernel<T>), dim3(count_grid(lay.blocks)), dim3(MC_THREADS), 0, st, gr, iso, (unsigned)lay.L, lay.G,
                     lay.blocks, (unsigned char*)(ws + lay.codes), (unsigned*)(ws + lay.counts));
  KAMD_RETURN_LAST_ERROR();
}

template <typename T>
int mc_emit_vertices(hipStream_t st, long long B, int X, int Y, int Z, int border, const T* in, long long sn, long long sx,
                     long long sy, long long sz, float iso, void* workspace, float* verts, long long verts_rows) {
  McLayout lay;
  McGrid<T> gr;
  if (!mc_make_grid(B, X, Y, Z, border, in, sn, sx, sy, sz, &lay, &gr) || workspace == nullptr || verts == nullptr || verts_rows < 0)
    return (int)hipErrorInvalidValue;
  char* ws = (char*)workspace;
  hipLaunchKernelGGL((mc_vertices_kernel<T>), dim3(count_grid(lay.blocks)), dim3(MC_THREADS), 0, st, gr, iso, (unsigned)lay.L, lay.G,
                     lay.blocks, (const unsigned char*)(ws + lay.codes), (const unsigned*)(ws + lay.counts),
                     (const long long*)(ws + lay.bases), (int*)(ws + lay.ranks), verts, verts_rows);
  KAMD_RETURN_LAST_ERROR();
}

template <typename T>
int mc_backward(hipStream_t st, long long B, int X, int Y, int Z, const T* in, long long sn, long long sx, long long sy, long long sz,
                float iso, const void* workspace, const float* grad_verts, long long verts_rows, T* grad) {
  McLayout lay;
  McGrid<T> gr;
  if (!mc_make_grid(B, X, Y, Z, 1, in, sn, sx, sy, sz, &lay, &gr) || workspace == nullptr || grad == nullptr || verts_rows < 0 ||
      (grad_verts == nullptr && verts_rows > 0))
    return (int)hipErrorInvalidValue;
  const char* ws = (const char*)workspace;
  const long long total = B * X * Y * Z;
  hipLaunchKernelGGL((mc_backward_kernel<T>), dim3(count_grid((total + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0, st, gr, iso,
                     (unsigned)lay.L, total, (const unsigned char*)(ws + lay.codes), (const long long*)(ws + lay.bases),
                     (const int*)(ws + lay.ranks), grad_verts, verts_rows, grad);
  KAMD_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {

size_t kamd_mcube_workspace(int64_t B, int X, int Y, int Z, int border) {
  McLayout lay;
  return mc_layout((long long)B, X, Y, Z, border, &lay) ? lay.bytes : 0;
}

int kamd_mcube_classify_u8(void* stream, int64_t B, int X, int Y, int Z, int border, const uint8_t* voxelgrids, int64_t stride_n,
                           int64_t stride_x, int64_t stride_y, int64_t stride_z, float iso_value, void* workspace) {
  return mc_classify<unsigned char>((hipStream_t)stream, (long long)B, X, Y, Z, border, voxelgrids, (long long)stride_n,
                                    (long long)stride_x, (long long)stride_y, (long long)stride_z, iso_value, workspace);
}
int kamd_mcube_classify_f16(void* stream, int64_t B, int X, int Y, int Z, int border, const void* voxelgrids, int64_t stride_n,
                            int64_t stride_x, int64_t stride_y, int64_t stride_z, float iso_value, void* workspace) {
  return mc_classify<half_bits>((hipStream_t)stream, (long long)B, X, Y, Z, border, (const half_bits*)voxelgrids, (long long)stride_n,
                              (long long)stride_x, (long long)stride_y, (long long)stride_z, iso_value, workspace);
}
int kamd_mcube_classify_f32(void* stream, int64_t B, int X, int Y, int Z, int border, const float* voxelgrids, int64_t stride_n,
                            int64_t stride_x, int64_t stride_y, int64_t stride_z, float iso_value, void* workspace) {
  return mc_classify<float>((hipStream_t)stream, (long long)B, X, Y, Z, border, voxelgrids, (long long)stride_n,
                            (long long)stride_x, (long long)stride_y, (long long)stride_z, iso_value, workspace);
}

int kamd_mcube_scan(void* stream, int64_t B, int X, int Y, int Z, int border, void* workspace, uint32_t* host_totals) {
  McLayout lay;
  if (!mc_layout((long long)B, X, Y, Z, border, &lay) || workspace == nullptr || host_totals == nullptr)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  unsigned* totals = (unsigned*)(ws + lay.totals);
  // a row = one counter of one item; its total is at most 5 triangles (or 3 vertices) per cell: <= 5 L < 2^32
  rows_scan(st, (long long)B * 2, lay.G, (unsigned*)(ws + lay.counts), totals);
  batch_bases<2>(st, (long long)B, (const unsigned*)totals, (long long*)(ws + lay.bases));
  KAMD_CHECK(hipGetLastError());
  // the one host read of the call: the B x 2 totals size the outputs
  KAMD_CHECK(hipMemcpyAsync(host_totals, totals, (size_t)B * 2 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  KAMD_CHECK(hipStreamSynchronize(st));
  return 0;
}

int kamd_mcube_emit_vertices_u8(void* stream, int64_t B, int X, int Y, int Z, int border, const uint8_t* voxelgrids, int64_t stride_n,
                                int64_t stride_x, int64_t stride_y, int64_t stride_z, float iso_value, void* workspace, float* verts,
                                int64_t verts_rows) {
  return mc_emit_vertices<unsigned char>((hipStream_t)stream, (long long)B, X, Y, Z, border, voxelgrids, (long long)stride_n,
                                         (long long)stride_x, (long long)stride_y, (long long)stride_z, iso_value, workspace, verts,
                                         (long long)verts_rows);
}
int kamd_mcube_emit_vertices_f16(void* stream, int64_t B, int X, int Y, int Z, int border, const void* voxelgrids, int64_t stride_n,
                                 int64_t stride_x, int64_t stride_y, int64_t stride_z, float iso_value, void* workspace, float* verts,
                                 int64_t verts_rows) {
  return mc_emit_vertices<half_bits>((hipStream_t)stream, (long long)B, X, Y, Z, border, (const half_bits*)voxelgrids, (long long)stride_n,
                                   (long long)stride_x, (long long)stride_y, (long long)stride_z, iso_value, workspace, verts,
                                   (long long)verts_rows);
}
int kamd_mcube_emit_vertices_f32(void* stream, int64_t B, int X, int Y, int Z, int border, const float* voxelgrids, int64_t stride_n,
                                 int64_t stride_x, int64_t stride_y, int64_t stride_z, float iso_value, void* workspace, float* verts,
                                 int64_t verts_rows) {
  return mc_emit_vertices<float>((hipStream_t)stream, (long long)B, X, Y, Z, border, voxelgrids, (long long)stride_n,
                                 (long long)stride_x, (long long)stride_y, (long long)stride_z, iso_value, workspace, verts,
                                 (long long)verts_rows);
}

int kamd_mcube_emit_faces(void* stream, int64_t B, int X, int Y, int Z, int border, const void* workspace, int64_t* faces,
                          int64_t faces_rows) {
  McLayout lay;
  if (!mc_layout((long long)B, X, Y, Z, border, &lay) || workspace == nullptr || faces == nullptr || faces_rows < 0)
    return (int)hipErrorInvalidValue;
  const char* ws = (const char*)workspace;
  hipLaunchKernelGGL(mc_faces_kernel, dim3(count_grid(lay.blocks)), dim3(MC_THREADS), 0, (hipStream_t)stream, lay.NX, lay.NY, lay.NZ,
                     border ? 1 : 0, (unsigned)lay.L, lay.G, lay.blocks, (const unsigned char*)(ws + lay.codes),
                     (const unsigned*)(ws + lay.counts), (const long long*)(ws + lay.bases), (const int*)(ws + lay.ranks),
                     (long long*)faces, (long long)faces_rows);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_mcube_backward_f16(void* stream, int64_t B, int X, int Y, int Z, const void* voxelgrids, int64_t stride_n, int64_t stride_x,
                            int64_t stride_y, int64_t stride_z, float iso_value, const void* workspace, const float* grad_verts,
                            int64_t verts_rows, void* grad_voxelgrids) {
  return mc_backward<half_bits>((hipStream_t)stream, (long long)B, X, Y, Z, (const half_bits*)voxelgrids, (long long)stride_n,
                              (long long)stride_x, (long long)stride_y, (long long)stride_z, iso_value, workspace, grad_verts,
                              (long long)verts_rows, (half_bits*)grad_voxelgrids);
}
int kamd_mcube_backward_f32(void* stream, int64_t B, int X, int Y, int Z, const float* voxelgrids, int64_t stride_n, int64_t stride_x,
                            int64_t stride_y, int64_t stride_z, float iso_value, const void* workspace, const float* grad_verts,
                            int64_t verts_rows, float* grad_voxelgrids) {
  return mc_backward<float>((hipStream_t)stream, (long long)B, X, Y, Z, voxelgrids, (long long)stride_n, (long long)stride_x,
                            (long long)stride_y, (long long)stride_z, iso_value, workspace, grad_verts, (long long)verts_rows,
                            grad_voxelgrids);
}

}  // extern "C"
