// ops.conversions.FlexiCubes: differentiable dual marching cubes over a voxel grid, float32 ("FlexiCubes").
//
//     cube c       = 8 vertex ids cube_idx[c][k], corner k = x + 2 y + 4 z, read through the tensor's strides; the cubes of a
//                    (rx, ry, rz) grid are laid out x ry rz + y rz + z (the ambiguity rule reads a neighbour by position)
//     case         = bit k set iff sdf(corner k) < 0 (NaN is not below); a surface cube has a case other than 0 and 255
//     group        = the crossed edges of one loop of the case (flexicubes_table.h): one dual vertex
//     orders       = the reference's: dual vertices by count class (1..4 dual vertices in the cube) ascending, then cube, then
//                    group; L_dev one entry per (dual vertex, edge) in class, cube, group, edge order; quads by the rank of their
//                    grid edge among the pairs (first id, second id) as written, the quads whose first end has sdf > 0 first
//
//   1. fc_classify_kernel   one thread per cube: 8 sdf values -> case byte; a marked case recomputes the case of the cube across
//                           its ambiguous face and inverts (255 - case) when that one is marked too.  Per workgroup and count
//                           class the number of cubes and of incidences, from __ballot / __popcll.  No atomics.
//      rows_scan_kernel     (count_scan.h) one workgroup per counter: exclusive scan in place, the total beside it.  HOST READ 1:
//                           the 8 totals and the index-error flag.
//   2. fc_compact_kernel    surface cube s (rank over all classes) -> (cube, case, first dual vertex, first incidence), and its
//                           12 pairs key = first id << 32 | second id, value = 12 s + edge.
//      ss_sort              the stable pair sort of sort_scan.h over 2 ceil(log2 V) bits: runs of equal edges, cubes ascending.
//      fc_runs_kernel       a run of exactly four on a crossed edge = a quad (flag at its head), and whether it is flipped.
//      ss_scan x 2          the quad's rank in edge order and among the flipped ones.  HOST READ 2: the number of quads.
//      (the surface-edge ranks themselves are never materialised: nothing reads them, the sorted order is their order)
//   3. fc_faces_kernel      the four dual vertices of a quad (first dual vertex of the cube + group of the edge), the flip
//                           partition, the triangles as int64 rows, and quad_of[12 s + edge] = 4 quad + corner for the backward.
//   4. fc_forward_kernel    one thread per surface cube, looping over its groups: the normalisation of the weights fused in,
//                           sums sequential in edge order, plain stores.  One thread per cube rather than per dual vertex: the
//                           alpha row of a cube feeds all its groups, so its owner can write that row's gradient with plain
//                           stores in the backward, and 5 cubes in 6 have one group anyway.
//      fc_centers_kernel    training: one thread per quad, the weighted centre vertex.
//   fc_backward_kernel      one thread per surface cube; recomputes from the inputs.  The cotangent of a dual vertex gathers the
//                           centres of its quads through quad_of (no atomics); beta, alpha and gamma rows are written by their
//                           owner; the shared grid vertices and sdf values take float atomic adds (run-to-run variation of
//                           rounding size in those two gradients).
//
// Every index derived from data is compared with its buffer's size before use: vertex ids with V (outside: the flag is raised,
// the value is never read), surface ranks with S, dual-vertex ids with NVD, incidence rows with NINC, quad rows with Q, the group
// of an edge with the case's group count.  Not capturable in a graph: two host reads size the outputs.
#include "common.h"
#include "../../include/kaolin_amd.h"
#include "count_scan.h"
#include "sort_scan.h"

#define KAMD_FLEXICUBES_QUALIFIER __device__ const
#include "flexicubes_table.h"

namespace {

constexpr int FC_THREADS = 256;
constexpr int FC_WAVES = FC_THREADS / 64;
constexpr int FC_COUNTERS = 8;  // per count class k = 1..4: cubes (k - 1), incidences (4 + k - 1)
constexpr int FC_TOTALS = 16;   // the 8 totals, the index-error flag at FC_FLAG
constexpr int FC_FLAG = 8;

// the corners of cube edge e, 3 bits each at bits [3 e, 3 e + 3): the first ends and the second ends
constexpr unsigned long long fc_corners(int c0, int c1, int c2, int c3, int c4, int c5, int c6, int c7, int c8, int c9, int c10, int c11) {
  return (unsigned long long)c0 | (unsigned long long)c1 << 3 | (unsigned long long)c2 << 6 | (unsigned long long)c3 << 9 |
         (unsigned long long)c4 << 12 | (unsigned long long)c5 << 15 | (unsigned long long)c6 << 18 | (unsigned long long)c7 << 21 |
         (unsigned long long)c8 << 24 | (unsigned long long)c9 << 27 | (unsigned long long)c10 << 30 | (unsigned long long)c11 << 33;
}
// edges (0,1) (1,5) (4,5) (0,4) (2,3) (3,7) (6,7) (2,6) (2,0) (3,1) (7,5) (6,4)
constexpr unsigned long long FC_FIRST = fc_corners(0, 1, 4, 0, 2, 3, 6, 2, 2, 3, 7, 6);
constexpr unsigned long long FC_SECOND = fc_corners(1, 5, 5, 4, 3, 7, 7, 6, 0, 1, 5, 4);
__device__ __forceinline__ int fc_first(int e) { return (int)(FC_FIRST >> (3 * e)) & 7; }
__device__ __forceinline__ int fc_second(int e) { return (int)(FC_SECOND >> (3 * e)) & 7; }

__device__ __forceinline__ unsigned fc_num_groups(unsigned long long row) { return (unsigned)(row >> 48) & 15u; }
__device__ __forceinline__ unsigned fc_group_of(unsigned long long row, int e) { return (unsigned)(row >> (4 * e)) & 15u; }
__device__ __forceinline__ unsigned fc_num_incidences(unsigned long long row) {
  unsigned n = 0u;
#pragma unroll
  for (int e = 0; e < 12; ++e) n += fc_group_of(row, e) != 15u ? 1u : 0u;
  return n;
}

struct FcGrid {
  const float* sdf;
  const long long* cube_idx;
  long long st_cube, st_corner;
  long long V, C;
};

__device__ __forceinline__ bool fc_valid(long long id, long long V) { return (unsigned long long)id < (unsigned long long)V; }
__device__ __forceinline__ long long fc_id(const FcGrid& gr, long long c, int k) { return gr.cube_idx[c * gr.st_cube + k * gr.st_corner]; }

// the case byte of cube c (c < C); an id outside [0, V) raises the flag and counts as not below
__device__ __forceinline__ unsigned fc_case(const FcGrid& gr, long long c, unsigned* flag) {
  unsigned code = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const long long id = fc_id(gr, c, k);
    if (!fc_valid(id, gr.V)) {
      *flag = 1u;
      continue;
    }
    code |= gr.sdf[id] < 0.f ? 1u << k : 0u;
  }
  return code;
}

// the 8 prefixes of a thread within its workgroup (class k at [k - 1] and [4 + k - 1]); s_waves: wavefront sums
__device__ __forceinline__ void fc_block_prefixes(unsigned groups, unsigned incidences, unsigned (*s_waves)[FC_WAVES], unsigned* prefix) {
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 1; k <= 4; ++k) {
    prefix[k - 1] = ballot_prefix<1>(groups == (unsigned)k ? 1u : 0u, &s_waves[k - 1][wave]);
    prefix[4 + k - 1] = ballot_prefix<4>(groups == (unsigned)k ? incidences : 0u, &s_waves[4 + k - 1][wave]);
  }
}

__global__ __launch_bounds__(FC_THREADS) void fc_classify_kernel(FcGrid gr, int rx, int ry, int rz, long long G,
                                                                 unsigned char* __restrict__ codes, unsigned* __restrict__ counts,
                                                                 unsigned* __restrict__ totals) {
  __shared__ unsigned s_waves[FC_COUNTERS][FC_WAVES];
  for (long long g = blockIdx.x; g < G; g += gridDim.x) {
    const long long c = g * FC_THREADS + threadIdx.x;
    unsigned groups = 0u, incidences = 0u;
    if (c < gr.C) {
      unsigned flag = 0u;
      unsigned code = fc_case(gr, c, &flag);
      const unsigned amb = kamd_flexicubes_ambiguous[code];
      if (amb != 0u) {
        // the cube across the ambiguous face: axis (amb - 1) / 2, side (amb - 1) & 1
        const int axis = (int)(amb - 1u) >> 1, step = ((amb - 1u) & 1u) ? 1 : -1;
        const long long yz = (long long)ry * rz;
        int p[3] = {(int)(c / yz), (int)((c / rz) % ry), (int)(c % rz)};
        p[axis] += step;
        if (p[0] >= 0 && p[0] < rx && p[1] >= 0 && p[1] < ry && p[2] >= 0 && p[2] < rz) {
          const long long other = ((long long)p[0] * ry + p[1]) * rz + p[2];
          if (other < gr.C && kamd_flexicubes_ambiguous[fc_case(gr, other, &flag)] != 0u) code = 255u - code;
        }
      }
      if (flag) totals[FC_FLAG] = 1u;  // (every writer stores the same value)
      codes[c] = (unsigned char)code;
      const unsigned long long row = kamd_flexicubes_groups[code];
      groups = fc_num_groups(row);
      incidences = fc_num_incidences(row);
    }
    unsigned prefix[FC_COUNTERS];
    fc_block_prefixes(groups, incidences, s_waves, prefix);
    __syncthreads();
    if (threadIdx.x < FC_COUNTERS) {
      unsigned sum = 0u;
      for (int w = 0; w < FC_WAVES; ++w) sum += s_waves[threadIdx.x][w];
      counts[threadIdx.x * G + g] = sum;
    }
    __syncthreads();  // (s_waves is rewritten by the next round)
  }
}

// surf[s] = (cube, case, first dual vertex, first incidence); keys / vals [12 s + e]
__global__ __launch_bounds__(FC_THREADS) void fc_compact_kernel(FcGrid gr, long long G, long long S, const unsigned char* __restrict__ codes,
                                                                const unsigned* __restrict__ offsets, const unsigned* __restrict__ totals,
                                                                int4* __restrict__ surf, unsigned long long* __restrict__ keys,
                                                                long long* __restrict__ vals) {
  __shared__ unsigned s_waves[FC_COUNTERS][FC_WAVES];
  const int wave = threadIdx.x >> 6;
  // where the dual vertices and the incidences of a count class start
  unsigned vd_base[5], inc_base[5];
  vd_base[1] = 0u, inc_base[1] = 0u;
#pragma unroll
  for (int k = 2; k <= 4; ++k) {
    vd_base[k] = vd_base[k - 1] + (unsigned)(k - 1) * totals[k - 2];
    inc_base[k] = inc_base[k - 1] + totals[4 + k - 2];
  }
  for (long long g = blockIdx.x; g < G; g += gridDim.x) {
    const long long c = g * FC_THREADS + threadIdx.x;
    unsigned code = 0u, groups = 0u, incidences = 0u;
    if (c < gr.C) {
      code = codes[c];
      const unsigned long long row = kamd_flexicubes_groups[code];
      groups = fc_num_groups(row);
      incidences = fc_num_incidences(row);
    }
    unsigned prefix[FC_COUNTERS];
    fc_block_prefixes(groups, incidences, s_waves, prefix);
    __syncthreads();
    if (groups >= 1u && groups <= 4u) {
      unsigned rank[FC_COUNTERS];  // over the whole grid, per counter
#pragma unroll
      for (int n = 0; n < FC_COUNTERS; ++n) {
        rank[n] = offsets[n * G + g] + prefix[n];
        for (int w = 0; w < wave; ++w) rank[n] += s_waves[n][w];
      }
      const long long s = (long long)rank[0] + rank[1] + rank[2] + rank[3];  // the surface cubes before this one
      if (s < S) {
        const int k = (int)groups;
        surf[s] = make_int4((int)c, (int)code, (int)(vd_base[k] + groups * rank[k - 1]), (int)(inc_base[k] + rank[4 + k - 1]));
#pragma unroll
        for (int e = 0; e < 12; ++e) {
          long long a = fc_id(gr, c, fc_first(e)), b = fc_id(gr, c, fc_second(e));
          if (!fc_valid(a, gr.V)) a = 0;  // (flagged by the classify kernel: the host raises before anything reads these)
          if (!fc_valid(b, gr.V)) b = 0;
          keys[s * 12 + e] = (unsigned long long)a << 32 | (unsigned long long)b;
          vals[s * 12 + e] = s * 12 + e;
        }
      }
    }
    __syncthreads();  // (s_waves is rewritten by the next round)
  }
}

// at the head i of a run of exactly four equal keys whose edge is crossed: is_quad[i] = 1, is_flipped[i] = the first end has sdf > 0
__global__ __launch_bounds__(FC_THREADS) void fc_runs_kernel(long long n, long long V, const float* __restrict__ sdf,
                                                             const unsigned long long* __restrict__ keys, int* __restrict__ is_quad,
                                                             int* __restrict__ is_flipped) {
  const long long i = (long long)blockIdx.x * FC_THREADS + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = keys[i];
  int quad = 0, flipped = 0;
  const bool head = i == 0 || keys[i - 1] != key;
  if (head && i + 3 < n && keys[i + 3] == key && (i + 4 == n || keys[i + 4] != key)) {
    const long long a = (long long)(key >> 32), b = (long long)(key & 0xffffffffull);
    if (a < V && b < V) {
      const float sa = sdf[a], sb = sdf[b];
      quad = (sa < 0.f) != (sb < 0.f) ? 1 : 0;
      flipped = quad && sa > 0.f ? 1 : 0;
    }
  }
  is_quad[i] = quad;
  is_flipped[i] = flipped;
}

__device__ __forceinline__ float fc_tanh_weight(const float* w, long long i, float scale) { return w ? tanhf(w[i]) * scale + 1.f : 1.f; }
__device__ __forceinline__ float fc_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }
__device__ __forceinline__ float fc_gamma_weight(const float* w, long long c, float scale) {
  return w ? fc_sigmoid(w[c]) * scale + (1.f - scale) / 2.f : 1.f;
}

__global__ __launch_bounds__(FC_THREADS) void fc_faces_kernel(long long n, long long C, long long S, long long NVD, long long Q,
                                                              const float* __restrict__ gamma, float scale, int training,
                                                              const int4* __restrict__ surf, const long long* __restrict__ vals,
                                                              const int* __restrict__ is_quad, const int* __restrict__ is_flipped,
                                                              const long long* __restrict__ pos_quad,
                                                              const long long* __restrict__ pos_flipped, int* __restrict__ quads,
                                                              int* __restrict__ quad_of, long long* __restrict__ faces,
                                                              long long faces_rows) {
  const long long i = (long long)blockIdx.x * FC_THREADS + threadIdx.x;
  if (i >= n || !is_quad[i] || i + 3 >= n) return;
  const long long q = pos_quad[i], f = pos_flipped[i], num_flipped = pos_flipped[n];
  const long long row = is_flipped[i] ? f : num_flipped + (q - f);
  if (row < 0 || row >= Q) return;
  int vd[4];
  float gm[4];
  long long val[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    val[j] = vals[i + j];
    const long long s = val[j] / 12;
    const int e = (int)(val[j] - s * 12);
    vd[j] = -1, gm[j] = 1.f;
    if (s < 0 || s >= S) continue;
    const int4 rec = surf[s];
    const unsigned long long tab = kamd_flexicubes_groups[rec.y & 255];
    const unsigned grp = fc_group_of(tab, e);
    if (grp >= fc_num_groups(tab) || (long long)rec.z + grp >= NVD || rec.x < 0 || rec.x >= C) continue;
    vd[j] = rec.z + (int)grp;
    gm[j] = fc_gamma_weight(gamma, rec.x, scale);
  }
  if (vd[0] < 0 || vd[1] < 0 || vd[2] < 0 || vd[3] < 0) return;  // (never: the runs hold crossed edges of surface cubes)
  // the four cubes ascending -> the quad's corners: [0, 1, 3, 2] when flipped, else [2, 3, 1, 0]
  const int o0 = is_flipped[i] ? 0 : 2, o1 = is_flipped[i] ? 1 : 3, o2 = is_flipped[i] ? 3 : 1, o3 = is_flipped[i] ? 2 : 0;
  const int v0 = vd[o0], v1 = vd[o1], v2 = vd[o2], v3 = vd[o3];
  quads[row * 4 + 0] = v0, quads[row * 4 + 1] = v1, quads[row * 4 + 2] = v2, quads[row * 4 + 3] = v3;
  quad_of[val[o0]] = (int)(row * 4 + 0);  // (val < 12 S: checked above)
  quad_of[val[o1]] = (int)(row * 4 + 1);
  quad_of[val[o2]] = (int)(row * 4 + 2);
  quad_of[val[o3]] = (int)(row * 4 + 3);
  if (training) {
    if (row * 4 + 3 >= faces_rows) return;
    const long long centre = NVD + row;
    long long* o = faces + row * 12;
    o[0] = v0, o[1] = v1, o[2] = centre;
    o[3] = v1, o[4] = v2, o[5] = centre;
    o[6] = v2, o[7] = v3, o[8] = centre;
    o[9] = v3, o[10] = v0, o[11] = centre;
  } else {
    if (row * 2 + 1 >= faces_rows) return;
    long long* o = faces + row * 6;
    if (gm[o0] * gm[o2] > gm[o1] * gm[o3]) {
      o[0] = v0, o[1] = v1, o[2] = v2;
      o[3] = v0, o[4] = v2, o[5] = v3;
    } else {
      o[0] = v0, o[1] = v1, o[2] = v3;
      o[3] = v3, o[4] = v1, o[5] = v2;
    }
  }
}

// ---- numerics ------------------------------------------------------------------------------------------------------------------
struct FcWeights {
  const float *beta, *alpha, *gamma;  // raw, (C, 12), (C, 8), (C,), contiguous; nullptr = ones
  float scale;
};

// one crossed edge of a cube: its ends (a: first, b: second), their positions, sdf values and alpha weights, its beta weight
struct FcEdge {
  long long a, b;
  float x0[3], x1[3], s0, s1, al0, al1, be;
  float w0, w1, den;     // the weights (s1 al1, -(s0 al0)) of the ends and their sum
  float ue[3], zc[3];    // the weighted point of the edge and its plain zero crossing
};
__device__ __forceinline__ bool fc_load_edge(const FcGrid& gr, const float* __restrict__ x, const FcWeights& w, long long c, int e, FcEdge* ed) {
  const int ka = fc_first(e), kb = fc_second(e);
  ed->a = fc_id(gr, c, ka), ed->b = fc_id(gr, c, kb);
  if (!fc_valid(ed->a, gr.V) || !fc_valid(ed->b, gr.V)) return false;
  ed->s0 = gr.sdf[ed->a], ed->s1 = gr.sdf[ed->b];
  ed->al0 = fc_tanh_weight(w.alpha, c * 8 + ka, w.scale), ed->al1 = fc_tanh_weight(w.alpha, c * 8 + kb, w.scale);
  ed->be = fc_tanh_weight(w.beta, c * 12 + e, w.scale);
  ed->w0 = ed->s1 * ed->al1, ed->w1 = -(ed->s0 * ed->al0);
  ed->den = ed->w0 + ed->w1;
  const float z1 = -ed->s0, zden = ed->s1 + z1;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    ed->x0[d] = x[ed->a * 3 + d], ed->x1[d] = x[ed->b * 3 + d];
    ed->ue[d] = (ed->x0[d] * ed->w0 + ed->x1[d] * ed->w1) / ed->den;
    ed->zc[d] = (ed->x0[d] * ed->s1 + ed->x1[d] * z1) / zden;
  }
  return true;
}

// the edges of group g of a case, ascending -> slots[0 .. n)
__device__ __forceinline__ int fc_group_edges(unsigned long long tab, unsigned g, int* slots) {
  int n = 0;
#pragma unroll
  for (int e = 0; e < 12; ++e)
    if (fc_group_of(tab, e) == g && n < 7) slots[n++] = e;
  return n;
}

// the dual vertex of a group: sum ue beta / sum beta, sequential in edge order
__device__ __forceinline__ void fc_dual_vertex(const FcGrid& gr, const float* __restrict__ x, const FcWeights& w, long long c, const int* slots,
                                               int n, float* vd, float* beta_sum) {
  float acc[3] = {0.f, 0.f, 0.f}, bs = 0.f;
  for (int j = 0; j < n; ++j) {
    FcEdge ed;
    if (!fc_load_edge(gr, x, w, c, slots[j], &ed)) continue;
#pragma unroll
    for (int d = 0; d < 3; ++d) acc[d] += ed.ue[d] * ed.be;
    bs += ed.be;
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) vd[d] = acc[d] / bs;
  *beta_sum = bs;
}
__device__ __forceinline__ float fc_distance(const float* p, const float* q) {
  const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  return sqrtf(dx * dx + dy * dy + dz * dz);
}

__global__ __launch_bounds__(FC_THREADS) void fc_forward_kernel(FcGrid gr, const float* __restrict__ x, FcWeights w, long long S,
                                                                long long NVD, long long NINC, const int4* __restrict__ surf,
                                                                float* __restrict__ verts, float* __restrict__ vd_gamma,
                                                                float* __restrict__ l_dev) {
  const long long s = (long long)blockIdx.x * FC_THREADS + threadIdx.x;
  if (s >= S) return;
  const int4 rec = surf[s];
  const long long c = rec.x;
  if (c < 0 || c >= gr.C) return;
  const unsigned long long tab = kamd_flexicubes_groups[rec.y & 255];
  const unsigned groups = fc_num_groups(tab);
  const float gm = fc_gamma_weight(w.gamma, c, w.scale);
  long long inc = rec.w;
  for (unsigned g = 0; g < groups && g < 4u; ++g) {
    int slots[7];
    const int n = fc_group_edges(tab, g, slots);
    const long long v = (long long)rec.z + g;
    if (v < 0 || v >= NVD || inc < 0 || inc + n > NINC) return;
    float vd[3], bs;
    fc_dual_vertex(gr, x, w, c, slots, n, vd, &bs);
    verts[v * 3 + 0] = vd[0], verts[v * 3 + 1] = vd[1], verts[v * 3 + 2] = vd[2];
    vd_gamma[v] = gm;
    // L_dev = |dist - mean dist| of the plain zero crossings
    float sum = 0.f;
    for (int j = 0; j < n; ++j) {
      FcEdge ed;
      float dist = 0.f;
      if (fc_load_edge(gr, x, w, c, slots[j], &ed)) dist = fc_distance(ed.zc, vd);
      l_dev[inc + j] = dist;
      sum += dist;
    }
    const float mean = sum / (float)n;
    for (int j = 0; j < n; ++j) l_dev[inc + j] = fabsf(l_dev[inc + j] - mean);
    inc += n;
  }
}

// the centre of quad q: ((v0 + v2) / 2 g02 + (v1 + v3) / 2 g13) / ((g02 + g13) + 1e-8) -> verts[NVD + q]
__global__ __launch_bounds__(FC_THREADS) void fc_centers_kernel(long long NVD, long long Q, const int* __restrict__ quads,
                                                                const float* __restrict__ vd_gamma, float* __restrict__ verts) {
  const long long q = (long long)blockIdx.x * FC_THREADS + threadIdx.x;
  if (q >= Q) return;
  int v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = quads[q * 4 + j];
    if (v[j] < 0 || v[j] >= NVD) return;
  }
  const float g02 = vd_gamma[v[0]] * vd_gamma[v[2]], g13 = vd_gamma[v[1]] * vd_gamma[v[3]];
  const float wsum = (g02 + g13) + 1e-8f;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float p02 = (verts[v[0] * 3ll + d] + verts[v[2] * 3ll + d]) / 2.f, p13 = (verts[v[1] * 3ll + d] + verts[v[3] * 3ll + d]) / 2.f;
    verts[(NVD + q) * 3 + d] = (p02 * g02 + p13 * g13) / wsum;
  }
}

// One thread per surface cube.  Per group, with vd = acc / B, acc = sum ue_j be_j, B = sum be_j, d_j = |zc_j - vd|, m = mean d_j,
// L_j = |d_j - m| and the cotangents gV (of vd, plus what the centres of its quads send back) and gL_j:
//     sg_j = sign(d_j - m),  t = sum gL_j sg_j,  gd_j = gL_j sg_j - t / n,  gzc_j = gd_j (zc_j - vd) / d_j  (0 where d_j = 0)
//     gvd  = gV - sum gzc_j
//     gue_j = gvd be_j / B,  gbe_j = gvd . (ue_j - vd) / B
// and through p = (x0 w0 + x1 w1) / (w0 + w1) (p = ue with w = (s1 al1, -s0 al0), p = zc with w = (s1, -s0)):
//     gx0 = gp w0 / den,  gx1 = gp w1 / den,  gw0 = gp . (x0 - p) / den,  gw1 = gp . (x1 - p) / den
__global__ __launch_bounds__(FC_THREADS) void fc_backward_kernel(FcGrid gr, const float* __restrict__ x, FcWeights w, int training, long long S,
                                                                 long long NVD, long long NINC, long long Q, const int4* __restrict__ surf,
                                                                 const int* __restrict__ quads, const int* __restrict__ quad_of,
                                                                 const float* __restrict__ verts, const float* __restrict__ vd_gamma,
                                                                 const float* __restrict__ g_verts, const float* __restrict__ g_ldev,
                                                                 float* __restrict__ gx, float* __restrict__ gs, float* __restrict__ g_beta,
                                                                 float* __restrict__ g_alpha, float* __restrict__ g_gamma) {
  const long long s = (long long)blockIdx.x * FC_THREADS + threadIdx.x;
  if (s >= S) return;
  const int4 rec = surf[s];
  const long long c = rec.x;
  if (c < 0 || c >= gr.C) return;
  const unsigned long long tab = kamd_flexicubes_groups[rec.y & 255];
  const unsigned groups = fc_num_groups(tab);
  long long inc = rec.w;
  float gg = 0.f;  // the cotangent of the cube's normalised gamma
  for (unsigned g = 0; g < groups && g < 4u; ++g) {
    int slots[7];
    const int n = fc_group_edges(tab, g, slots);
    const long long v = (long long)rec.z + g;
    if (v < 0 || v >= NVD || inc < 0 || inc + n > NINC) return;
    float vd[3], bs;
    fc_dual_vertex(gr, x, w, c, slots, n, vd, &bs);
    float gvd[3] = {g_verts[v * 3 + 0], g_verts[v * 3 + 1], g_verts[v * 3 + 2]};
    if (training) {
      // the centres of the quads of this dual vertex: d centre / d v_m = pair / (2 wsum), d centre / d pair = (P - centre) / wsum
      for (int j = 0; j < n; ++j) {
        const int at = quad_of[s * 12 + slots[j]];
        if (at < 0) continue;
        const long long q = at >> 2;
        const int m = at & 3;
        if (q >= Q) continue;
        int qv[4];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          qv[k] = quads[q * 4 + k];
          ok = ok && qv[k] >= 0 && qv[k] < NVD;
        }
        if (!ok) continue;
        const float g02 = vd_gamma[qv[0]] * vd_gamma[qv[2]], g13 = vd_gamma[qv[1]] * vd_gamma[qv[3]];
        const float wsum = (g02 + g13) + 1e-8f;
        const float pair = (m & 1) ? g13 : g02;
        const int opposite = qv[m ^ 2];
        float dot = 0.f;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const float gc = g_verts[(NVD + q) * 3 + d];
          gvd[d] += gc * (pair / (2.f * wsum));
          const float p = (verts[qv[m] * 3ll + d] + verts[opposite * 3ll + d]) / 2.f;
          dot += gc * (p - verts[(NVD + q) * 3 + d]);
        }
        gg += dot / wsum * vd_gamma[opposite];
      }
    }
    // the distances, their mean and t
    float dist[7], sum = 0.f;
    for (int j = 0; j < n; ++j) {
      FcEdge ed;
      dist[j] = fc_load_edge(gr, x, w, c, slots[j], &ed) ? fc_distance(ed.zc, vd) : 0.f;
      sum += dist[j];
    }
    const float mean = sum / (float)n;
    float t = 0.f;
    for (int j = 0; j < n; ++j) {
      const float diff = dist[j] - mean;
      t += g_ldev[inc + j] * (diff > 0.f ? 1.f : diff < 0.f ? -1.f : 0.f);
    }
    // the zero crossings' branch; gvd collects - sum gzc_j
    for (int j = 0; j < n; ++j) {
      FcEdge ed;
      if (!fc_load_edge(gr, x, w, c, slots[j], &ed)) continue;
      const float diff = dist[j] - mean;
      const float gd = g_ldev[inc + j] * (diff > 0.f ? 1.f : diff < 0.f ? -1.f : 0.f) - t / (float)n;
      const float z1 = -ed.s0, zden = ed.s1 + z1;
      float gw0 = 0.f, gw1 = 0.f;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float gzc = dist[j] > 0.f ? gd * ((ed.zc[d] - vd[d]) / dist[j]) : 0.f;
        gvd[d] -= gzc;
        atomicAdd(gx + ed.a * 3 + d, gzc * (ed.s1 / zden));
        atomicAdd(gx + ed.b * 3 + d, gzc * (z1 / zden));
        gw0 += gzc * (ed.x0[d] - ed.zc[d]);
        gw1 += gzc * (ed.x1[d] - ed.zc[d]);
      }
      atomicAdd(gs + ed.b, gw0 / zden);   // w0 = s1
      atomicAdd(gs + ed.a, -(gw1 / zden));  // w1 = -s0
    }
    // the dual vertex' branch
    for (int j = 0; j < n; ++j) {
      FcEdge ed;
      const int e = slots[j];
      if (!fc_load_edge(gr, x, w, c, e, &ed)) continue;
      float gbe = 0.f, gw0 = 0.f, gw1 = 0.f;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float gue = gvd[d] * (ed.be / bs);
        gbe += gvd[d] * (ed.ue[d] - vd[d]);
        atomicAdd(gx + ed.a * 3 + d, gue * (ed.w0 / ed.den));
        atomicAdd(gx + ed.b * 3 + d, gue * (ed.w1 / ed.den));
        gw0 += gue * (ed.x0[d] - ed.ue[d]);
        gw1 += gue * (ed.x1[d] - ed.ue[d]);
      }
      gw0 /= ed.den, gw1 /= ed.den;
      atomicAdd(gs + ed.b, gw0 * ed.al1);      // w0 = s1 al1
      atomicAdd(gs + ed.a, -(gw1 * ed.al0));   // w1 = -(s0 al0)
      if (w.beta) {
        const float th = tanhf(w.beta[c * 12 + e]);
        g_beta[c * 12 + e] = gbe / bs * (w.scale * (1.f - th * th));  // (an edge belongs to one group: a plain store)
      }
      if (w.alpha) {
        // rows of g_alpha arrive zeroed; this thread is the only writer of row c
        const int ka = fc_first(e), kb = fc_second(e);
        const float t0 = tanhf(w.alpha[c * 8 + ka]), t1 = tanhf(w.alpha[c * 8 + kb]);
        g_alpha[c * 8 + kb] += gw0 * ed.s1 * (w.scale * (1.f - t1 * t1));
        g_alpha[c * 8 + ka] += -(gw1 * ed.s0) * (w.scale * (1.f - t0 * t0));
      }
    }
    inc += n;
  }
  if (training && w.gamma) {
    const float sg = fc_sigmoid(w.gamma[c]);
    g_gamma[c] = gg * (w.scale * sg * (1.f - sg));
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// the first workspace: [totals 16 u32][counts 8 x G u32][codes C u8]
struct FcLayout {
  long long G;
  size_t totals, counts, codes, bytes;
};
bool fc_layout(long long C, FcLayout* lay) {
  if (C <= 0 || C > ((1ll << 31) - 1) / 12) return false;  // 12 C incidences and pairs at most: 32-bit ranks
  lay->G = (C + FC_THREADS - 1) / FC_THREADS;
  size_t o = 0;
  lay->totals = o, o += kamd_align16(FC_TOTALS * 4);
  lay->counts = o, o += kamd_align16((size_t)FC_COUNTERS * (size_t)lay->G * 4);
  lay->codes = o, o += kamd_align16((size_t)C);
  lay->bytes = o;
  return true;
}
// the second: the pairs of n = 12 S edges, both sides of the sort's ping-pong, the flags and their scans, the sort's scratch
struct FcEdgeLayout {
  long long n;
  size_t keys, keys_tmp, vals, vals_tmp, is_quad, is_flipped, pos_quad, pos_flipped, hist, offs, sums, bytes;
};
bool fc_edge_layout(long long S, FcEdgeLayout* lay) {
  if (S <= 0 || S > ((1ll << 31) - 1) / 12) return false;
  const long long n = S * 12;
  lay->n = n;
  size_t o = 0;
  lay->keys = o, o += kamd_align16((size_t)n * 8);
  lay->keys_tmp = o, o += kamd_align16((size_t)n * 8);
  lay->vals = o, o += kamd_align16((size_t)n * 8);
  lay->vals_tmp = o, o += kamd_align16((size_t)n * 8);
  lay->is_quad = o, o += kamd_align16((size_t)n * 4);
  lay->is_flipped = o, o += kamd_align16((size_t)n * 4);
  lay->pos_quad = o, o += kamd_align16((size_t)(n + 1) * 8);
  lay->pos_flipped = o, o += kamd_align16((size_t)(n + 1) * 8);
  lay->hist = o, o += kamd_align16(ss_sort_hist_entries(n) * 4);
  lay->offs = o, o += kamd_align16(ss_sort_offs_entries(n) * 8);
  lay->sums = o, o += kamd_align16(ss_sort_unique_sums_entries(n) * 8);
  lay->bytes = o;
  return true;
}

bool fc_make_grid(int64_t V, int64_t C, const float* sdf, const int64_t* cube_idx, int64_t st_cube, int64_t st_corner, FcGrid* gr) {
  if (V <= 0 || V >= (1ll << 31) || C <= 0 || sdf == nullptr || cube_idx == nullptr) return false;
  *gr = FcGrid{sdf, (const long long*)cube_idx, (long long)st_cube, (long long)st_corner, (long long)V, (long long)C};
  return true;
}
int fc_bits(long long V) {
  int bits = 1;
  while (bits < 32 && (1ll << bits) < V) ++bits;
  return bits;
}

}  // namespace

extern "C" {

size_t kamd_flexicubes_workspace(int64_t C) {
  FcLayout lay;
  return fc_layout((long long)C, &lay) ? lay.bytes : 0;
}

int kamd_flexicubes_classify(void* stream, int64_t V, int64_t C, int rx, int ry, int rz, const float* sdf, const int64_t* cube_idx,
                             int64_t stride_cube, int64_t stride_corner, void* workspace, uint32_t* host_totals) {
  FcLayout lay;
  FcGrid gr;
  if (!fc_layout((long long)C, &lay) || !fc_make_grid(V, C, sdf, cube_idx, stride_cube, stride_corner, &gr) || workspace == nullptr ||
      host_totals == nullptr || rx < 1 || ry < 1 || rz < 1 || (long long)rx * ry * rz != (long long)C)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  unsigned* totals = (unsigned*)(ws + lay.totals);
  KAMD_CHECK(hipMemsetAsync(totals, 0, FC_TOTALS * 4, st));
  hipLaunchKernelGGL(fc_classify_kernel, dim3(count_grid(lay.G)), dim3(FC_THREADS), 0, st, gr, rx, ry, rz, lay.G,
                     (unsigned char*)(ws + lay.codes), (unsigned*)(ws + lay.counts), totals);
  // a row = one counter; its total is at most the 12 C incidences: <= 12 C < 2^31
  rows_scan(st, FC_COUNTERS, lay.G, (unsigned*)(ws + lay.counts), totals);
  KAMD_CHECK(hipGetLastError());
  // host read 1: the sizes of the surface and the index-error flag
  KAMD_CHECK(hipMemcpyAsync(host_totals, totals, (FC_FLAG + 1) * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  KAMD_CHECK(hipStreamSynchronize(st));
  return 0;
}

size_t kamd_flexicubes_edges_workspace(int64_t S) {
  FcEdgeLayout lay;
  return fc_edge_layout((long long)S, &lay) ? lay.bytes : 0;
}

int kamd_flexicubes_edges(void* stream, int64_t V, int64_t C, int64_t S, const float* sdf, const int64_t* cube_idx, int64_t stride_cube,
                          int64_t stride_corner, const void* workspace, int32_t* surf, void* edges_workspace, int64_t* host_num_quads) {
  FcLayout lay;
  FcEdgeLayout el;
  FcGrid gr;
  if (!fc_layout((long long)C, &lay) || !fc_edge_layout((long long)S, &el) || S > C ||
      !fc_make_grid(V, C, sdf, cube_idx, stride_cube, stride_corner, &gr) || workspace == nullptr || surf == nullptr ||
      edges_workspace == nullptr || host_num_quads == nullptr)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const char* ws = (const char*)workspace;
  char* ew = (char*)edges_workspace;
  unsigned long long* keys = (unsigned long long*)(ew + el.keys);
  long long* vals = (long long*)(ew + el.vals);
  // a rank the kernels would not reach stays a pair of (0, 0) edges with value 0: in range whatever happens
  KAMD_CHECK(hipMemsetAsync(ew + el.keys, 0, (size_t)el.n * 8, st));
  KAMD_CHECK(hipMemsetAsync(ew + el.vals, 0, (size_t)el.n * 8, st));
  KAMD_CHECK(hipMemsetAsync(surf, 0xFF, (size_t)S * 16, st));
  hipLaunchKernelGGL(fc_compact_kernel, dim3(count_grid(lay.G)), dim3(FC_THREADS), 0, st, gr, lay.G, (long long)S,
                     (const unsigned char*)(ws + lay.codes), (const unsigned*)(ws + lay.counts), (const unsigned*)(ws + lay.totals),
                     (int4*)surf, keys, vals);
  KAMD_CHECK(hipGetLastError());
  const SsSortWs sw = ss_sort_ws((int*)(ew + el.hist), (long long*)(ew + el.offs), (long long*)(ew + el.sums));
  KAMD_CHECK(ss_sort(st, el.n, ss_passes_halves(fc_bits((long long)V)), keys, vals, (unsigned long long*)(ew + el.keys_tmp),
                     (long long*)(ew + el.vals_tmp), keys, vals, sw));
  int* is_quad = (int*)(ew + el.is_quad);
  int* is_flipped = (int*)(ew + el.is_flipped);
  long long* pos_quad = (long long*)(ew + el.pos_quad);
  long long* pos_flipped = (long long*)(ew + el.pos_flipped);
  hipLaunchKernelGGL(fc_runs_kernel, dim3(ss_grid(el.n, FC_THREADS)), dim3(FC_THREADS), 0, st, el.n, (long long)V, sdf,
                     (const unsigned long long*)keys, is_quad, is_flipped);
  KAMD_CHECK(hipGetLastError());
  KAMD_CHECK(ss_scan(st, el.n, (const long long*)nullptr, (const int*)is_quad, pos_quad, (long long*)(ew + el.sums)));
  KAMD_CHECK(ss_scan(st, el.n, (const long long*)nullptr, (const int*)is_flipped, pos_flipped, (long long*)(ew + el.sums)));
  // host read 2: the number of quads
  long long h = 0;
  KAMD_CHECK(hipMemcpyAsync(&h, pos_quad + el.n, 8, hipMemcpyDeviceToHost, st));
  KAMD_CHECK(hipStreamSynchronize(st));
  *host_num_quads = h;
  return 0;
}

int kamd_flexicubes_faces(void* stream, int64_t C, int64_t S, int64_t num_vd, int64_t num_quads, const float* gamma, float weight_scale,
                          int training, const int32_t* surf, const void* edges_workspace, int32_t* quads, int32_t* quad_of,
                          int64_t* faces, int64_t faces_rows) {
  FcEdgeLayout el;
  if (!fc_edge_layout((long long)S, &el) || C <= 0 || num_vd < S || num_vd > 4 * S || num_quads <= 0 || num_quads > el.n / 4 ||
      surf == nullptr || edges_workspace == nullptr || quads == nullptr || quad_of == nullptr || faces == nullptr ||
      faces_rows != num_quads * (training ? 4 : 2))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const char* ew = (const char*)edges_workspace;
  KAMD_CHECK(hipMemsetAsync(quad_of, 0xFF, (size_t)el.n * 4, st));
  KAMD_CHECK(hipMemsetAsync(quads, 0xFF, (size_t)num_quads * 16, st));
  hipLaunchKernelGGL(fc_faces_kernel, dim3(ss_grid(el.n, FC_THREADS)), dim3(FC_THREADS), 0, st, el.n, (long long)C, (long long)S,
                     (long long)num_vd, (long long)num_quads, gamma, weight_scale, training ? 1 : 0, (const int4*)surf,
                     (const long long*)(ew + el.vals), (const int*)(ew + el.is_quad), (const int*)(ew + el.is_flipped),
                     (const long long*)(ew + el.pos_quad), (const long long*)(ew + el.pos_flipped), quads, quad_of, (long long*)faces,
                     (long long)faces_rows);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_flexicubes_forward(void* stream, int64_t V, int64_t C, int64_t S, int64_t num_vd, int64_t num_incidences, const float* vertices,
                            const float* sdf, const int64_t* cube_idx, int64_t stride_cube, int64_t stride_corner, const float* beta,
                            const float* alpha, const float* gamma, float weight_scale, const int32_t* surf, float* out_vertices,
                            float* vd_gamma, float* l_dev) {
  FcGrid gr;
  if (!fc_make_grid(V, C, sdf, cube_idx, stride_cube, stride_corner, &gr) || S <= 0 || S > C || num_vd < S || num_vd > 4 * S ||
      num_incidences < 3 * num_vd || num_incidences > 12 * S || vertices == nullptr || surf == nullptr || out_vertices == nullptr ||
      vd_gamma == nullptr || l_dev == nullptr)
    return (int)hipErrorInvalidValue;
  const FcWeights w = {beta, alpha, gamma, weight_scale};
  hipLaunchKernelGGL(fc_forward_kernel, dim3(ss_grid(S, FC_THREADS)), dim3(FC_THREADS), 0, (hipStream_t)stream, gr, vertices, w, (long long)S,
                     (long long)num_vd, (long long)num_incidences, (const int4*)surf, out_vertices, vd_gamma, l_dev);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_flexicubes_centers(void* stream, int64_t num_vd, int64_t num_quads, const int32_t* quads, const float* vd_gamma,
                            float* out_vertices) {
  if (num_vd <= 0 || num_quads <= 0 || quads == nullptr || vd_gamma == nullptr || out_vertices == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(fc_centers_kernel, dim3(ss_grid(num_quads, FC_THREADS)), dim3(FC_THREADS), 0, (hipStream_t)stream, (long long)num_vd,
                     (long long)num_quads, quads, vd_gamma, out_vertices);
  KAMD_RETURN_LAST_ERROR();
}

int kamd_flexicubes_backward(void* stream, int64_t V, int64_t C, int64_t S, int64_t num_vd, int64_t num_incidences, int64_t num_quads,
                             const float* vertices, const float* sdf, const int64_t* cube_idx, int64_t stride_cube, int64_t stride_corner,
                             const float* beta, const float* alpha, const float* gamma, float weight_scale, int training,
                             const int32_t* surf, const int32_t* quads, const int32_t* quad_of, const float* out_vertices,
                             const float* vd_gamma, const float* grad_vertices, const float* grad_l_dev, float* grad_x, float* grad_sdf,
                             float* grad_beta, float* grad_alpha, float* grad_gamma) {
  FcGrid gr;
  if (!fc_make_grid(V, C, sdf, cube_idx, stride_cube, stride_corner, &gr) || S <= 0 || S > C || num_vd < S || num_vd > 4 * S ||
      num_incidences < 3 * num_vd || num_incidences > 12 * S || num_quads < 0 || vertices == nullptr || surf == nullptr ||
      out_vertices == nullptr || vd_gamma == nullptr || grad_vertices == nullptr || grad_l_dev == nullptr || grad_x == nullptr ||
      grad_sdf == nullptr || (beta != nullptr && grad_beta == nullptr) || (alpha != nullptr && grad_alpha == nullptr) ||
      (training && gamma != nullptr && grad_gamma == nullptr) || (training && num_quads > 0 && (quads == nullptr || quad_of == nullptr)))
    return (int)hipErrorInvalidValue;
  const FcWeights w = {beta, alpha, gamma, weight_scale};
  hipLaunchKernelGGL(fc_backward_kernel, dim3(ss_grid(S, FC_THREADS)), dim3(FC_THREADS), 0, (hipStream_t)stream, gr, vertices, w,
                     (training && num_quads > 0) ? 1 : 0, (long long)S, (long long)num_vd, (long long)num_incidences, (long long)num_quads,
                     (const int4*)surf, quads, quad_of, out_vertices, vd_gamma, grad_vertices, grad_l_dev, grad_x, grad_sdf, grad_beta,
                     grad_alpha, grad_gamma);
  KAMD_RETURN_LAST_ERROR();
}

}  // extern "C"
