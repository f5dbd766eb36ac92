// ---- exact sweep over Hilbert-ordered tiles (included by triangle_distance.hip, inside its anonymous namespace) -------------
// The all-pairs kernel spends its time REJECTING faces: 11 VALU per (point, face) for the per-face sphere test, 5e10 pairs
// at C5.  Here faces and queries are both ordered along the Hilbert curve of their position (a counting sort on the curve's
// first 21 bits -- 128^3 cells -- of our own: ts_keys_count / ts_scan_* / ts_scatter; the order inside a cell is irrelevant, the
// search is exact whatever the order), faces are grouped into tiles of 64 consecutive ones with a bounding sphere per tile, and a
// workgroup of 256 consecutive queries
//   A. derives, from the tile spheres alone, an upper bound U on its nearest distance (some face of tile t lies within
//      |p - c_t| + r_t): no face is evaluated to get a tight bound, however far the query is from the surface;
//   B. marks, 64 tiles per step, the tiles whose sphere comes closer than min(best, U) for ANY of its queries (one barrier
//      per 64 tiles), and only those are staged in LDS and walked with the per-face sphere test + td_eval() of the all-pairs
//      kernel.  Neighbouring queries need the same few tiles, so a wavefront touches a few percent of the faces.
// Bounds: a tile carries its sphere AND a slab (unit mean normal n, half thickness t = max |n . (x - c)| over its vertices):
// every point x of the tile satisfies |p - x| >= |n . (p - c)| - t, so lb = max(|p - c| - r, |n . (p - c)| - t).  Seen from
// the concave side of a curved surface the sphere bound alone admits a wide cap of nearly equidistant tiles (a query at half
// the radius inside a sphere: 8 % of all tiles); the slab bound cuts it to the tiles actually under the query (0.5 %).  The
// same idea per face: |un . (p - centroid)| (the distance to the face's plane) is tested after the face sphere and before
// the closest-point evaluation.
// A query is seeded with face 0 exactly as the reference does; every evaluation is td_eval() on the same face record and
// ties go to the lower face index explicitly, so dist / face_idx / dist_type are identical to the all-pairs result.  Culling
// is conservative: the bounds carry the same 0.1 % + 1e-5 |p| head-room as the per-face sphere test.
PHASE_TABLE(g_phase_ts)
// the sweep's work counters of the last call made while they were switched on (kamd_triangle_distance_work_counters)
static int g_ts_stats_on = 0;
static unsigned long long g_ts_stats_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
constexpr int TS_MORTON_G = 1024;
// a query whose bound admits more tiles than this gets a workgroup of its own (ts_hard_kernel).  Measured at 1M x 50k with
// the slab bounds (profiles/r02i_ts_modes.txt): 48 -> 1 613 hard queries, 8.6 ms; 195 (the value of the sphere-only bounds)
// -> 20 ms, one lane evaluating ~10 000 faces serially while its workgroup waits; 16 -> 300k hard queries, 45 ms.  With the
// lane = face mode, the candidate lists and ts_hard_kernel starting from the sweep's bound (profiles/r02l_ts.txt):
// 32 -> 5.56 ms (sweep 4.1 + hard 1.1), 48 -> 5.95 ms, 24 -> 10.5 ms
// Round 3 (profiles/r03x_ts_hard_*.txt): the hard kernel takes a WAVEFRONT per query (one bound tightening over all the tile
// chunks, four times the queries in flight: 1.75x faster per hard query than a workgroup each), and the best threshold
// depends on how many queries there are to fill the sweep's workgroups with: 65k-100k queries 2.5-2.6 ms at 32 vs 1.5-1.7 at
// 6-8; 200k 2.96 vs 2.6 at 12; from 400k on 32 again (1M: 4.9 ms; 16: 8.1).
// blocks per run of the sweep's XCD-aware block order (ts_xcd_block); experiment builds: KAMD_TS_XCD_CHUNK = run + 1, 9999 = eighths
// Measured at 1M x 50k (profiles/r05b_ts_xcd_ab.txt, sweep kernel): identity 4.17-4.22 ms, runs of 1 / 4 / 8 / 16 / 32 / 64 / 128 blocks
// 4.19 / 4.06 / 4.15 / 4.13 / 4.19 / 4.39 / 4.30, eighths 4.41-4.54 (the curve's heavy stretches land on single XCDs): the sweep is
// bound by instructions, not by where its tiles come from; runs of 4 keep neighbours together at no cost in balance
inline int ts_xcd_chunk() {
  const int v = kamd_env_int("KAMD_TS_XCD_CHUNK", 5) - 1;
  return v == 9998 ? -1 : v;
}
inline int ts_hard_threshold(int N, int ntiles) {
  (void)ntiles;
  const int dflt = N < 131072 ? 8 : (N < 300000 ? 12 : 32);
  return kamd_env_int("KAMD_TS_HARD_THRESHOLD", dflt);
}

__device__ __forceinline__ unsigned int ts_spread10(unsigned int v) {  // 10 bits -> every third bit
  v &= 0x3FFu;
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}
// 30-bit HILBERT index of a cell of the 1024^3 grid over the face centres (Skilling's transpose form, then bit interleave).
// Unlike the Z-order, consecutive indices are always adjacent cells: 64 consecutive faces of a surface make a compact
// patch (offline, unit sphere of 50k faces: median tile radius 0.070 vs 0.081, a quarter fewer faces admitted per query).
__device__ __forceinline__ unsigned int ts_morton(const kamd::Box& bx, float x, float y, float z) {
  unsigned int X[3];
  X[0] = (unsigned int)kamd::sdg_axis_cell(x, bx.lo[0], bx.inv[0], TS_MORTON_G);
  X[1] = (unsigned int)kamd::sdg_axis_cell(y, bx.lo[1], bx.inv[1], TS_MORTON_G);
  X[2] = (unsigned int)kamd::sdg_axis_cell(z, bx.lo[2], bx.inv[2], TS_MORTON_G);
#pragma unroll
  for (unsigned int Q = 512u; Q > 1u; Q >>= 1) {
    const unsigned int P = Q - 1u;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (X[i] & Q) {
        X[0] ^= P;
      } else {
        const unsigned int t = (X[0] ^ X[i]) & P;
        X[0] ^= t;
        X[i] ^= t;
      }
    }
  }
  X[1] ^= X[0];
  X[2] ^= X[1];
  unsigned int t = 0;
#pragma unroll
  for (unsigned int Q = 512u; Q > 1u; Q >>= 1)
    if (X[2] & Q) t ^= Q - 1u;
  X[0] ^= t;
  X[1] ^= t;
  X[2] ^= t;
  return (ts_spread10(X[0]) << 2) | (ts_spread10(X[1]) << 1) | ts_spread10(X[2]);
}

// Counting sort along the curve: a bucket = a cell of the 128^3 grid (the first 21 bits of the 30-bit Hilbert index); faces that
// no bound culls or that are tested by their own slab (td_prep_kernel: infinite / negative radius) go to one more bucket behind
// all others, so that they fill the LAST tiles instead of giving the tiles of their neighbours an infinite radius.
// Round 6 (ADVICE r05): the number of buckets follows the problem -- 2^bits with bits = ceil(log2(max(N, F))) + 2 in 12..21 (four
// buckets per element: the order inside a bucket is arbitrary, so buckets should stay nearly private) -- instead of 2^21 whatever the
// sizes: a 2 048-face mesh cleared 16 MB and scanned 4 M counters per call.  C5 (1 M queries) keeps 21 bits.
constexpr int TS_BUCKET_BITS_MAX = 21;
inline int ts_bucket_bits(int N, int F) {
  const int m = N > F ? N : F;
  int bits = 2;
  while (bits < 40 && (1ll << (bits - 2)) < (long long)m) ++bits;
  return bits < 12 ? 12 : (bits > TS_BUCKET_BITS_MAX ? TS_BUCKET_BITS_MAX : bits);
}
constexpr int TS_SCAN_BLOCK = 1024;  // entries a scan workgroup owns

struct TsWs {
  void* rec_sorted;  // the face records in curve order: a tile's 64 records are contiguous
  float *bbox_part, *centres, *radius, *tile_sphere;
  int *fcount, *qcount;  // per bucket: count, then (in place) start
  int *ftotals, *qtotals;  // per scan block
  int2 *fcr, *qcr;       // per element {bucket, rank inside the bucket}
  int *fidx, *qidx;      // the sorted orders: position -> original index
  int *hard_count, *hard_list;
  unsigned long long* stats;  // measurement counters (KAMD_TS_STATS)
  size_t zero_bytes;     // from fcount on: both count arrays and the hard-query counter, cleared by one fill per call
  size_t total;
};
inline TsWs ts_layout(char* base, int N, int F, int esz) {
  TsWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = base + off;
    off += (bytes + 255) & ~(size_t)255;
    return r;
  };
  const int ntiles = (F + TD_TILE - 1) / TD_TILE;
  w.rec_sorted = (void*)take((size_t)F * TD_REC * esz);
  w.bbox_part = (float*)take((size_t)kamd::SDG_NB * 6 * 4);
  w.centres = (float*)take((size_t)F * 12);
  w.radius = (float*)take((size_t)F * 4);
  w.tile_sphere = (float*)take((size_t)ntiles * 32);  // {c, r} {n, t}
  const size_t z0 = off;
  const int ts_nb = 1 << ts_bucket_bits(N, F);
  w.fcount = (int*)take((size_t)(ts_nb + 1) * 4);
  w.qcount = (int*)take((size_t)ts_nb * 4);
  w.hard_count = (int*)take(4);
  w.zero_bytes = off - z0;
  const int nsb = (ts_nb + 1 + TS_SCAN_BLOCK - 1) / TS_SCAN_BLOCK;
  w.ftotals = (int*)take((size_t)nsb * 4);
  w.qtotals = (int*)take((size_t)nsb * 4);
  w.fcr = (int2*)take((size_t)F * 8);
  w.qcr = (int2*)take((size_t)N * 8);
  w.fidx = (int*)take((size_t)F * 4);
  w.qidx = (int*)take((size_t)N * 4);
  w.stats = (unsigned long long*)take(64);
  w.hard_list = (int*)take((size_t)N * 4);
  w.total = off;
  return w;
}

// bucket + rank of every face and query (the rank is what the counting atomicAdd returns: the order inside a bucket is the
// order of arrival, which nothing depends on)
template <typename T>
__global__ __launch_bounds__(256) void ts_keys_count_kernel(int F, int N, int nb, int bucket_bits, const float* __restrict__ centres,
                                                            const float* __restrict__ radius, const float* __restrict__ part,
                                                            const T* __restrict__ points, int* __restrict__ fcount,
                                                            int* __restrict__ qcount, int2* __restrict__ fcr, int2* __restrict__ qcr) {
  __shared__ kamd::Box s_box;
  if (threadIdx.x == 0) s_box = kamd::sdg_box(part, 0, nb, TS_MORTON_G);
  __syncthreads();
  const int TS_NB = 1 << bucket_bits;  // (the tail bucket's number)
  const int nfb = (F + 255) / 256;
  if ((int)blockIdx.x < nfb) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    const bool have = f < F;
    const bool tail = have && !(radius[f] < INFINITY);
    // the tail bucket is ONE address: a wavefront's tail faces arrive with one atomic
    const unsigned long long tm = __ballot(tail);
    int tbase = 0;
    if (tm != 0ull) {
      const int lane = threadIdx.x & 63, leader = __ffsll((long long)tm) - 1;
      if (lane == leader) tbase = atomicAdd(fcount + TS_NB, __popcll(tm));
      tbase = __shfl(tbase, leader, 64) + __popcll(tm & ((1ull << lane) - 1ull));
    }
    if (have) {
      if (tail) {
        fcr[f] = make_int2(TS_NB, tbase);
      } else {
        const int bk = (int)(ts_morton(s_box, centres[(size_t)f * 3], centres[(size_t)f * 3 + 1], centres[(size_t)f * 3 + 2]) >> (30 - bucket_bits));
        fcr[f] = make_int2(bk, atomicAdd(fcount + bk, 1));
      }
    }
  } else {
    const int i = ((int)blockIdx.x - nfb) * 256 + threadIdx.x;
    if (i < N) {
      const int bk = (int)(ts_morton(s_box, (float)points[(size_t)i * 3], (float)points[(size_t)i * 3 + 1], (float)points[(size_t)i * 3 + 2]) >> (30 - bucket_bits));
      qcr[i] = make_int2(bk, atomicAdd(qcount + bk, 1));
    }
  }
}

// exclusive scan of the two count arrays, in place, in two launches: every block of TS_SCAN_BLOCK entries leaves its total, then
// adds up the totals in front of it and scans its own entries (blockIdx.y: 0 = faces, 1 = queries)
__global__ __launch_bounds__(256) void ts_scan_totals_kernel(const int* __restrict__ fcount, int nf, const int* __restrict__ qcount, int nq,
                                                             int* __restrict__ ftotals, int* __restrict__ qtotals) {
  __shared__ int s_w[4];
  const int* cnt = blockIdx.y == 0 ? fcount : qcount;
  const int n = blockIdx.y == 0 ? nf : nq;
  const int base = blockIdx.x * TS_SCAN_BLOCK;
  if (base >= n) return;
  int v = 0;
#pragma unroll
  for (int k = 0; k < TS_SCAN_BLOCK / 256; ++k) {
    const int i = base + k * 256 + (int)threadIdx.x;
    v += i < n ? cnt[i] : 0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) (blockIdx.y == 0 ? ftotals : qtotals)[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}
__global__ __launch_bounds__(256) void ts_scan_apply_kernel(int* __restrict__ fcount, int nf, int* __restrict__ qcount, int nq,
                                                            const int* __restrict__ ftotals, const int* __restrict__ qtotals) {
  __shared__ int s_w[4], s_w2[4];
  int* cnt = blockIdx.y == 0 ? fcount : qcount;
  const int n = blockIdx.y == 0 ? nf : nq;
  const int* tot = blockIdx.y == 0 ? ftotals : qtotals;
  const int base = blockIdx.x * TS_SCAN_BLOCK;
  if (base >= n) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int before = 0;
  for (int k = threadIdx.x; k < (int)blockIdx.x; k += 256) before += tot[k];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) before += __shfl_xor(before, d, 64);
  if (lane == 0) s_w[wave] = before;
  // a thread owns TS_SCAN_BLOCK / 256 consecutive entries
  constexpr int PER = TS_SCAN_BLOCK / 256;
  int v[PER], sum = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = base + (int)threadIdx.x * PER + k;
    v[k] = i < n ? cnt[i] : 0;
    sum += v[k];
  }
  const int inc = wave_inclusive(sum, lane);
  if (lane == 63) s_w2[wave] = inc;
  __syncthreads();
  int off = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]) + inc - sum;
  for (int w = 0; w < wave; ++w) off += s_w2[w];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = base + (int)threadIdx.x * PER + k;
    if (i < n) cnt[i] = off;
    off += v[k];
  }
}
__global__ __launch_bounds__(256) void ts_scatter_kernel(int F, int N, const int* __restrict__ fstart, const int* __restrict__ qstart,
                                                         const int2* __restrict__ fcr, const int2* __restrict__ qcr,
                                                         int* __restrict__ fidx, int* __restrict__ qidx) {
  const int nfb = (F + 255) / 256;
  if ((int)blockIdx.x < nfb) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < F) {
      const int2 cr = fcr[f];
      fidx[fstart[cr.x] + cr.y] = f;
    }
  } else {
    const int i = ((int)blockIdx.x - nfb) * 256 + threadIdx.x;
    if (i < N) {
      const int2 cr = qcr[i];
      qidx[qstart[cr.x] + cr.y] = i;
    }
  }
}

// Workgroups are dealt to the eight XCDs round robin (workgroup w runs on XCD w % 8), each with an L2 of its own.  The queries
// are in curve order: when XCD x takes the x-th EIGHTH of them instead of every eighth workgroup, the tiles its workgroups stage
// are an eighth of the mesh -- they stay in that XCD's 4 MB of L2 instead of all 8 MB of records passing through every L2.
__device__ __forceinline__ int ts_xcd_block(int w, int n, int chunk) {
  // chunk = 0: the identity (neighbours on the curve run side by side on all eight XCDs); chunk = C: XCD x takes runs of C
  // consecutive blocks (blocks [8 C k + C x, + C) for k = 0, 1, ...): locality inside a run, the curve's heavy stretches still
  // spread over all XCDs; chunk < 0: XCD x takes the x-th eighth of the curve
  if (chunk == 0) return w;
  const int x = w % 8, j = w / 8;
  if (chunk < 0) {
    const int per = n / 8, rem = n % 8;
    return x * per + (x < rem ? x : rem) + j;
  }
  const int full = (n / (8 * chunk)) * (8 * chunk);  // the blocks that make whole rounds of 8 runs; the rest keep their place
  if (w >= full) return w;
  return ((j / chunk) * 8 + x) * chunk + (j % chunk);
}

// one wavefront per tile of 64 curve-consecutive faces: centre = mean of the face-sphere centres, radius = the farthest
// face sphere (with rounding head-room); a non-finite member makes the radius non-finite and the tile is never culled.
// Slab: n = normalised sum of the faces' unit normals, t = the farthest vertex from the plane through the centre.
template <typename T>
__global__ __launch_bounds__(64) void ts_tile_spheres_kernel(int F, const int* __restrict__ f_sorted, const T* __restrict__ rec,
                                                             const float* __restrict__ centres, const float* __restrict__ radius,
                                                             float* __restrict__ tile_sphere) {
  const int t = blockIdx.x, lane = threadIdx.x;
  const int k = t * TD_TILE + lane;
  const bool have = k < F;
  const int f = have ? f_sorted[k] : 0;
  float cx = have ? centres[(size_t)f * 3] : 0.f, cy = have ? centres[(size_t)f * 3 + 1] : 0.f;
  float cz = have ? centres[(size_t)f * 3 + 2] : 0.f, n = have ? 1.f : 0.f;
  const T* r0 = rec + (size_t)f * TD_REC;
  float ux = have ? (float)r0[33] : 0.f, uy = have ? (float)r0[34] : 0.f, uz = have ? (float)r0[35] : 0.f;
  // (a face whose normal is exactly zero has a NaN unit normal and keeps its sphere, td_prep_kernel: it must not cost its
  // neighbours their slab)
  if (!(fabsf(ux) <= 2.f && fabsf(uy) <= 2.f && fabsf(uz) <= 2.f)) ux = uy = uz = 0.f;
  float sx = cx, sy = cy, sz = cz;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    sx += __shfl_xor(sx, d, 64);
    sy += __shfl_xor(sy, d, 64);
    sz += __shfl_xor(sz, d, 64);
    n += __shfl_xor(n, d, 64);
    ux += __shfl_xor(ux, d, 64);
    uy += __shfl_xor(uy, d, 64);
    uz += __shfl_xor(uz, d, 64);
  }
  const float mx = sx / n, my = sy / n, mz = sz / n;
  const float dx = cx - mx, dy = cy - my, dz = cz - mz;
  float r = have ? sqrtf(dx * dx + dy * dy + dz * dz) + radius[f] : 0.f;
  if (have && !(r == r)) r = INFINITY;  // NaN member: never culled (fmaxf below would drop the NaN)
  const float ulen = sqrtf(ux * ux + uy * uy + uz * uz);
  const bool slab = ulen > 1e-20f && ulen < 3.0e38f;  // false for NaN too
  const float nx = slab ? ux / ulen : 0.f, ny = slab ? uy / ulen : 0.f, nz = slab ? uz / ulen : 0.f;
  float th = 0.f;
  if (have) {
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const float h = fabsf(nx * ((float)r0[v * 3] - mx) + ny * ((float)r0[v * 3 + 1] - my) + nz * ((float)r0[v * 3 + 2] - mz));
      th = (h > th || !(h == h)) ? h : th;  // a NaN vertex poisons the thickness: the slab test then never culls
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    r = fmaxf(r, __shfl_xor(r, d, 64));
    const float o = __shfl_xor(th, d, 64);
    th = (o > th || !(o == o)) ? o : th;
  }
  if (lane == 0) {
    const float mag = fabsf(mx) + fabsf(my) + fabsf(mz);
    const bool finite_r = r < 3.0e38f;
    tile_sphere[(size_t)t * 8 + 0] = mx;
    tile_sphere[(size_t)t * 8 + 1] = my;
    tile_sphere[(size_t)t * 8 + 2] = mz;
    tile_sphere[(size_t)t * 8 + 3] = r * 1.00001f + 1e-6f * mag + 1e-30f;
    tile_sphere[(size_t)t * 8 + 4] = finite_r ? nx : 0.f;
    tile_sphere[(size_t)t * 8 + 5] = finite_r ? ny : 0.f;
    tile_sphere[(size_t)t * 8 + 6] = finite_r ? nz : 0.f;
    // float rounding of n . (p - c) and of the vertices' offsets: relative 1e-5 of the thickness and of the coordinates
    tile_sphere[(size_t)t * 8 + 7] = finite_r ? th * 1.00001f + 4e-6f * (mag + r) + 1e-30f : 0.f;
  }
}

// lower bound on the distance from p to any face of tile t (and, optionally, the upper bound on the distance to its
// nearest face).  NaN / inf bounds compare false against `> reach`: such a tile is kept.
template <typename T>
__device__ __forceinline__ T ts_tile_lb(const float* __restrict__ tile_sphere, int t, V3<T> p, T* ub, int mode = 0) {
  const float4 s = reinterpret_cast<const float4*>(tile_sphere)[2 * t];
  const float4 n = reinterpret_cast<const float4*>(tile_sphere)[2 * t + 1];
  const T dx = p.x - (T)s.x, dy = p.y - (T)s.y, dz = p.z - (T)s.z;
  const T dist = td_sqrt(dx * dx + dy * dy + dz * dz);
  if (ub != nullptr) *ub = dist + (T)s.w;
  const T lb = dist - (T)s.w;
  const T h = td_abs(dx * (T)n.x + dy * (T)n.y + dz * (T)n.z) - (T)n.w;
  return (h > lb && !(mode & 1)) ? h : lb;
}
// records are staged with an odd word stride: in lane = face mode (below) every lane reads its own record, and a stride of
// TD_REC = 40 words would put 16 lanes on each LDS bank
constexpr int TS_LDS_REC = TD_REC + 1;
constexpr int TS_CAND_CAP = 2048;  // tiles a workgroup's candidate list holds (more: the workgroup scans every tile)
__device__ __forceinline__ float ts_bcast(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ double ts_bcast(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

template <typename T>
__global__ __launch_bounds__(256) void ts_sort_records_kernel(int F, const int* __restrict__ f_sorted, const T* __restrict__ rec,
                                                              T* __restrict__ rec_sorted) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)F * TD_REC) return;
  const size_t k = i / TD_REC;
  rec_sorted[i] = rec[(size_t)f_sorted[k] * TD_REC + (i - k * TD_REC)];
}

template <typename T, int NT>
__global__ __launch_bounds__(NT) void ts_sweep_kernel(int N, int F, const T* __restrict__ points,
                                                              const T* __restrict__ rec, const T* __restrict__ rec_sorted,
                                                              const int* __restrict__ q_sorted,
                                                              const int* __restrict__ f_sorted,
                                                              const float* __restrict__ tile_sphere, int* __restrict__ hard_count,
                                                              int* __restrict__ hard_list, int hard_threshold, int mode, int few, int xcd_chunk,
                                                              unsigned long long* __restrict__ stats, T* __restrict__ out_dist, int64_t* __restrict__ out_idx,
                                                              int32_t* __restrict__ out_type) {
  __shared__ __attribute__((aligned(16))) T tile[TD_TILE * TS_LDS_REC];
  __shared__ int s_fid[TD_TILE];
  __shared__ unsigned long long s_need;
  __shared__ float s_box6[6][NT / 64], s_umin[NT / 64];
  __shared__ int s_cand[TS_CAND_CAP];
  __shared__ int s_ncand;
  PHASE_DECL;
  const int ntiles = (F + TD_TILE - 1) / TD_TILE;
  const int slot = ts_xcd_block(blockIdx.x, gridDim.x, xcd_chunk) * NT + threadIdx.x;
  const bool live = slot < N;
  const int qi = live ? q_sorted[slot] : 0;
  const V3<T> p = live ? ld3(points + (size_t)qi * 3) : mk<T>(0, 0, 0);
  const T pmag = (T)1e-5 * max3abs(p);
  // seed: face 0 unconditionally (unbatched_triangle_distance_cuda.cu:303,309)
  int best_type;
  T best = td_eval<T>(rec, p, &best_type);
  int best_face = 0;
  T bound = td_sqrt(best) * (T)1.001 + pmag;   // NaN seed: every comparison below is false, the seed sticks
  bool search = live && best == best;
  // 0. The workgroup's queries are Hilbert neighbours: the tiles ANY of them can need are a small subset of the mesh.  With
  // c, qr the bounding sphere of the searching queries: every query q has a face within U = min_t(|c - c_t| + r_t) + qr, its
  // reach never exceeds U * 1.001 + pmag, and lb_t(q) >= lb_t(c) - qr (both bounds are 1-Lipschitz) -- so the tiles with
  // lb_t(c) - qr above that are out for the whole workgroup.  256 threads test the tiles once; the per-query scans below
  // (three of them) then walk the candidate list instead of all tiles.
  const int lane_ = threadIdx.x & 63, wave_ = threadIdx.x >> 6;
  float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool odd = false;
  if (search) {
    const float pf[3] = {(float)p.x, (float)p.y, (float)p.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      blo[a] = bhi[a] = pf[a];
      odd = odd || !(fabsf(pf[a]) < 3.0e38f);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      blo[a] = fminf(blo[a], __shfl_xor(blo[a], d, 64));
      bhi[a] = fmaxf(bhi[a], __shfl_xor(bhi[a], d, 64));
    }
    if (lane_ == 0) {
      s_box6[a][wave_] = blo[a];
      s_box6[3 + a][wave_] = bhi[a];
    }
  }
  if (threadIdx.x == 0) s_ncand = 0;
  const bool any_odd = __syncthreads_or(odd);
  V3<float> qc;
  float qr;
  {
    float lo3[3], hi3[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo3[a] = s_box6[a][0];
      hi3[a] = s_box6[3 + a][0];
#pragma unroll
      for (int w = 1; w < NT / 64; ++w) {
        lo3[a] = fminf(lo3[a], s_box6[a][w]);
        hi3[a] = fmaxf(hi3[a], s_box6[3 + a][w]);
      }
    }
    qc = mk<float>(0.5f * (lo3[0] + hi3[0]), 0.5f * (lo3[1] + hi3[1]), 0.5f * (lo3[2] + hi3[2]));
    const float ex = hi3[0] - lo3[0], ey = hi3[1] - lo3[1], ez = hi3[2] - lo3[2];
    const float mag = fmaxf(fmaxf(fabsf(lo3[0]), fabsf(hi3[0])), fmaxf(fmaxf(fabsf(lo3[1]), fabsf(hi3[1])), fmaxf(fabsf(lo3[2]), fabsf(hi3[2]))));
    qr = 0.5f * sqrtf(ex * ex + ey * ey + ez * ez) * 1.0001f + 2e-6f * mag;  // (float copies of the points: 6e-8 relative)
    float u = INFINITY;
    for (int t = threadIdx.x; t < ntiles; t += NT) {
      float ub;
      (void)ts_tile_lb<float>(tile_sphere, t, qc, &ub, mode);
      u = fminf(u, ub);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) u = fminf(u, __shfl_xor(u, d, 64));
    if (lane_ == 0) s_umin[wave_] = u;
    __syncthreads();
    u = s_umin[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) u = fminf(u, s_umin[w]);
    // reach <= (u + qr) * 1.001 + 1e-5 * |p|; a little more for the float arithmetic of this pass
    const float thresh = ((u + qr) * 1.001f + 1e-5f * (mag + qr) + qr) * 1.0001f + 2e-6f * mag;
    if (lo3[0] <= hi3[0] && !any_odd) {  // (no searching query: no candidates)
      for (int t = threadIdx.x; t < ntiles; t += NT)
        if (!(ts_tile_lb<float>(tile_sphere, t, qc, nullptr, mode) > thresh)) {
          const int pos = atomicAdd(&s_ncand, 1);
          if (pos < TS_CAND_CAP) s_cand[pos] = t;
        }
    }
    __syncthreads();
  }
  PHASE_MARK(0);
  // a query with a non-finite coordinate, or more candidates than the list holds: every tile, as before
  const bool all_tiles = any_odd || s_ncand > TS_CAND_CAP;
  const int nc = all_tiles ? ntiles : s_ncand;
#define TS_TILE_AT(c) (all_tiles ? (c) : __builtin_amdgcn_readfirstlane(s_cand[(c)]))  // c is wave-uniform: scalar loads follow
  // A. upper bound on the nearest distance from the tile spheres alone
  T reach = bound;
  if (search) {
    T U = INFINITY;
    int tU = 0;
    for (int c = 0; c < nc; ++c) {
      const int t = TS_TILE_AT(c);
      T ub;
      (void)ts_tile_lb<T>(tile_sphere, t, p, &ub, mode);
      if (ub < U) {
        U = ub;
        tU = t;
      }
    }
    const T ur = U * (T)1.001 + pmag;
    if (ur < reach) reach = ur;
    PHASE_MARK(1);
    // ... and the faces of that tile right away (each lane its own tile, records straight from global memory): the bound
    // is then the true nearest distance, or close to it, BEFORE the sweep decides which tiles it needs -- tiles are swept
    // in Morton order, not nearest first, and a loose bound lets every face within it through the sphere test
    {
      const int f0 = tU * TD_TILE, cnt = min(TD_TILE, F - f0);
      for (int k = 0; k < cnt; ++k) {
        const T* r = rec_sorted + (size_t)(f0 + k) * TD_REC;
        const V3<T> pc = p - ld3(r + 36);
        if (td_face_far<T, true>(r, pc, dot(pc, pc), reach, mode)) continue;
        const int f = f_sorted[f0 + k];
        int type;
        const float dist = td_eval<T>(r, p, &type);
        if (dist < best || (dist == best && f < best_face)) {
          best = dist;
          best_type = type;
          best_face = f;
          bound = td_sqrt(best) * (T)1.001 + pmag;
          if (bound < reach) reach = bound;
        }
      }
    }
    PHASE_MARK(2);
    // a query nearly equidistant from a large part of the mesh (deep inside / far outside a closed surface) needs many
    // tiles whatever the search: a single lane would hold its workgroup for milliseconds, so it is handed to
    // ts_hard_kernel, where a whole workgroup shares one query
    int n_need = 0;
    for (int c = 0; c < nc; ++c) n_need += (ts_tile_lb<T>(tile_sphere, TS_TILE_AT(c), p, nullptr, mode) > reach) ? 0 : 1;
    if (stats != nullptr) {
      atomicAdd(stats + 5, (unsigned long long)n_need);
      if (n_need > 48) atomicAdd(stats + 6, 1ull);
    }
    // (one append per wavefront, not per query: tens of thousands of returning atomics on ONE address serialise at ~20 ns each)
    const bool is_hard = n_need > hard_threshold;
    const unsigned long long hard_mask = __ballot(is_hard);
    int hard_base = 0;
    if (hard_mask != 0ull) {
      const int leader = __ffsll((long long)hard_mask) - 1;
      if ((int)(threadIdx.x & 63) == leader) hard_base = atomicAdd(hard_count, __popcll(hard_mask));
      hard_base = __shfl(hard_base, leader, 64);
    }
    if (is_hard) {
      hard_list[hard_base + __popcll(hard_mask & ((1ull << (threadIdx.x & 63)) - 1ull))] = qi;
      search = false;
      // what this lane found so far (the seed, the faces of its best tile) goes with the query: ts_hard_kernel starts from
      // that bound instead of face 0's (which admits nearly every tile)
      out_dist[qi] = best;
      out_idx[qi] = best_face;
      out_type[qi] = best_type;
    }
  }
  PHASE_MARK(3);
  const bool writes = live && (search || !(best == best));  // a hard query is written by ts_hard_kernel
  // B. the tiles some query of this workgroup still needs, 64 at a time
  for (int t0 = 0; t0 < nc; t0 += 64) {
    unsigned long long need = 0ull;
    if (search) {
      const int nt = min(64, nc - t0);
      for (int j = 0; j < nt; ++j)
        need |= (ts_tile_lb<T>(tile_sphere, TS_TILE_AT(t0 + j), p, nullptr, mode) > reach) ? 0ull : (1ull << j);  // NaN / inf bound: kept
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) need |= __shfl_xor(need, d, 64);
    __syncthreads();  // the previous step's readers are done with s_need / the tile
    if (threadIdx.x == 0) s_need = 0ull;
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && need != 0ull) atomicOr(&s_need, need);
    __syncthreads();
    PHASE_MARK(4);
    unsigned long long todo = s_need;
    if (stats != nullptr && threadIdx.x == 0) atomicAdd(stats + 0, (unsigned long long)__popcll(todo));
    // (Round 5, measured and dropped: the NEXT tile's records requested into registers while the current one is walked -- a quarter of
    // the kernel's wave time is the wait for a tile's 10 KB between the two barriers, profiles/r05i_ts_sweep_phases.txt -- costs
    // 30 VGPRs, 6 -> 4 waves per SIMD: 4.83 vs 4.35 ms at 1M x 50k, profiles/r05j_ts_prefetch_ab.txt.  Kept from it: one barrier
    // less per tile, the face ids are copied with the records.)
    while (todo != 0ull) {
      const int j = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const int tj = TS_TILE_AT(t0 + j);
      const int f0 = tj * TD_TILE, cnt = min(TD_TILE, F - f0);
      __syncthreads();  // the previous tile's walkers are done with the LDS copy
      if ((int)threadIdx.x < cnt) s_fid[threadIdx.x] = f_sorted[f0 + threadIdx.x];
      for (int k = threadIdx.x; k < cnt * TD_REC; k += NT) tile[k + k / TD_REC] = rec_sorted[(size_t)f0 * TD_REC + k];
      __syncthreads();
      PHASE_MARK(5);
      // does any query of this wavefront still need the tile (the bound may have tightened since it was marked)?
      bool mine = false;
      if (search) mine = !(ts_tile_lb<T>(tile_sphere, tj, p, nullptr, mode) > reach);
      const unsigned long long mm = __ballot(mine);
      if (mm == 0ull) continue;
      if (stats != nullptr && (threadIdx.x & 63) == 0) atomicAdd(stats + 1, 1ull);
      if (stats != nullptr && mine) atomicAdd(stats + 2, 1ull);
      if (__popcll(mm) <= few) {
        // Few of the wavefront's queries want this tile (typically ONE: a query nearly equidistant from a large part of
        // the mesh needs tiles none of its neighbours do).  lane = query would walk the 64 faces for a single active lane --
        // and that lane serially through every tile it needs: milliseconds for one query.  Here lane = FACE instead: each
        // wanting query in turn is broadcast, the 64 faces are evaluated at once and the winner (smaller distance, then
        // smaller face index: the reference's order) is reduced across the wavefront and handed to the owner lane.
        const int lane = threadIdx.x & 63;
        for (unsigned long long m2 = mm; m2 != 0ull; m2 &= m2 - 1ull) {
          const int j = __ffsll((long long)m2) - 1;
          const V3<T> pj = mk<T>(ts_bcast(p.x, j), ts_bcast(p.y, j), ts_bcast(p.z, j));
          const T reach_j = ts_bcast(reach, j);
          float dist = INFINITY;
          int f = 0x7fffffff, type = 0;
          if (lane < cnt) {
            const T* r = tile + lane * TS_LDS_REC;
            const V3<T> pc = pj - ld3(r + 36);
            if (!td_face_far<T, true>(r, pc, dot(pc, pc), reach_j, mode)) {
              const float d = td_eval<T>(r, pj, &type);
              if (d == d) {  // a NaN distance never wins (only face 0 may seed with one)
                dist = d;
                f = s_fid[lane];
              }
            }
          }
#pragma unroll
          for (int sh = 32; sh >= 1; sh >>= 1) {
            const float od = __shfl_xor(dist, sh, 64);
            const int of = __shfl_xor(f, sh, 64), ot = __shfl_xor(type, sh, 64);
            if (od < dist || (od == dist && of < f)) {
              dist = od;
              f = of;
              type = ot;
            }
          }
          if (lane == j && f != 0x7fffffff && (dist < best || (dist == best && f < best_face))) {
            best = dist;
            best_type = type;
            best_face = f;
            bound = td_sqrt(best) * (T)1.001 + pmag;
            if (bound < reach) reach = bound;
          }
        }
        PHASE_MARK(7);
        continue;
      }
      for (int k = 0; k < cnt; ++k) {
        const T* r = tile + k * TS_LDS_REC;
        const V3<T> pc = p - ld3(r + 36);
        const T d2c = dot(pc, pc);
        // false for NaN / inf: then the face is evaluated
        const bool skip = !mine || td_face_far<T, true>(r, pc, d2c, reach, mode);
        if (!__any(!skip)) continue;
        if (stats != nullptr && (threadIdx.x & 63) == 0) atomicAdd(stats + 3, 1ull);
        if (skip) continue;
        if (stats != nullptr) atomicAdd(stats + 4, 1ull);
        int type;
        const float dist = td_eval<T>(r, p, &type);
        const int f = s_fid[k];
        if (dist < best || (dist == best && f < best_face)) {
          best = dist;
          best_type = type;
          best_face = f;
          bound = td_sqrt(best) * (T)1.001 + pmag;
          if (bound < reach) reach = bound;
        }
      }
      PHASE_MARK(6);
    }
  }
  PHASE_MARK(8);
  if (writes) {
    out_dist[qi] = best;
    out_idx[qi] = best_face;
    out_type[qi] = best_type;
  }
  PHASE_FLUSH(g_phase_ts);
#undef TS_TILE_AT
}

// one workgroup per hard query; lane = face of a tile (record read straight from global memory); the candidates of a tile are reduced across the wavefront with the reference's order (smaller distance,
// then smaller face index), the four wavefronts are merged at the end
template <typename T>
__global__ __launch_bounds__(TD_THREADS) void ts_hard_kernel(int F, const T* __restrict__ points, const T* __restrict__ rec,
                                                             const T* __restrict__ rec_sorted, const int* __restrict__ f_sorted,
                                                             const float* __restrict__ tile_sphere,
                                                             const int* __restrict__ hard_count,
                                                             const int* __restrict__ hard_list, int mode,
                                                             T* __restrict__ out_dist, int64_t* __restrict__ out_idx,
                                                             int32_t* __restrict__ out_type) {
  const int ntiles = (F + TD_TILE - 1) / TD_TILE;
  const int nhard = *hard_count;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // a WAVEFRONT per hard query: it walks all the 64-tile chunks itself, so every chunk is tested against the bound the
  // earlier ones left, four queries are in flight per workgroup, and nothing is merged through LDS (round 2 gave a query a
  // workgroup -- four wavefronts, each with a bound of its own, merged at the end: 1.75x slower per hard query, r03x)
  constexpr int WPG = TD_THREADS / 64;
  for (int q = blockIdx.x * WPG + wave; q < nhard; q += gridDim.x * WPG) {
    const int qi = hard_list[q];
    const V3<T> p = ld3(points + (size_t)qi * 3);
    const T pmag = (T)1e-5 * max3abs(p);
    int best_type = out_type[qi];
    T best = out_dist[qi];
    int best_face = (int)out_idx[qi];
    T reach = td_sqrt(best) * (T)1.001 + pmag;
    for (int c0 = 0; c0 < ntiles; c0 += 64) {
      bool near_ = false;
      if (c0 + lane < ntiles) near_ = !(ts_tile_lb<T>(tile_sphere, c0 + lane, p, nullptr, mode) > reach);
      for (unsigned long long m = __ballot(near_); m != 0ull; m &= m - 1ull) {
        const int t = c0 + __ffsll((long long)m) - 1;
        if (ts_tile_lb<T>(tile_sphere, t, p, nullptr, mode) > reach) continue;  // wave-uniform: the bound has tightened
        const int k = t * TD_TILE + lane;
        float dist = INFINITY;
        int f = 0x7fffffff, type = 0;
        if (k < F) {
          const T* r = rec_sorted + (size_t)k * TD_REC;
          const V3<T> pc = p - ld3(r + 36);
          if (!td_face_far<T, true>(r, pc, dot(pc, pc), reach, mode)) {
            const float d = td_eval<T>(r, p, &type);
            if (d == d) {
              dist = d;
              f = f_sorted[k];
            }
          }
        }
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) {
          const float od = __shfl_xor(dist, sh, 64);
          const int of = __shfl_xor(f, sh, 64), ot = __shfl_xor(type, sh, 64);
          if (od < dist || (od == dist && of < f)) {
            dist = od;
            f = of;
            type = ot;
          }
        }
        if (f != 0x7fffffff && ((T)dist < best || ((T)dist == best && f < best_face))) {
          best = dist;
          best_face = f;
          best_type = type;
          const T b = td_sqrt(best) * (T)1.001 + pmag;
          if (b < reach) reach = b;
        }
      }
    }
    if (lane == 0) {
      out_dist[qi] = best;
      out_idx[qi] = best_face;
      out_type[qi] = best_type;
    }
  }
}

template <typename T>
int ts_forward_launch(hipStream_t st, int N, int F, const T* points, const T* faces, T* dist, int64_t* face_idx,
                      int32_t* dist_type, void* workspace) {
  T* rec = (T*)workspace;
  const TdReseed rs = td_reseed_layout((char*)workspace + td_align((size_t)F * TD_REC * sizeof(T)), N, F);
  const TsWs w = ts_layout((char*)workspace + td_align((size_t)F * TD_REC * sizeof(T)) + td_reseed_bytes(N, F), N, F, (int)sizeof(T));
  const int nb = kamd_cdiv(F, 4096) < kamd::SDG_NB ? kamd_cdiv(F, 4096) : kamd::SDG_NB;
  const int ntiles = kamd_cdiv(F, TD_TILE);
  {
    kamd::ProfScope prof_(kamd::K_TD_PREP, st);
    KAMD_CHECK(kamd_zero_async(w.fcount, w.zero_bytes, st));
    hipLaunchKernelGGL(td_prep_kernel<T>, dim3(kamd_cdiv(F, 256)), dim3(256), 0, st, F, faces, rec, w.centres, w.radius, rs.blk_flag,
                       rs.queue_count);
    hipLaunchKernelGGL(kamd::sdg_bbox, dim3(nb, 1), dim3(256), 0, st, F, w.centres, w.bbox_part);
    const int bucket_bits = ts_bucket_bits(N, F), TS_NB = 1 << bucket_bits;
    hipLaunchKernelGGL(ts_keys_count_kernel<T>, dim3(kamd_cdiv(F, 256) + kamd_cdiv(N, 256)), dim3(256), 0, st, F, N, nb, bucket_bits, (const float*)w.centres,
                       (const float*)w.radius, (const float*)w.bbox_part, points, w.fcount, w.qcount, w.fcr, w.qcr);
    const int nsb = kamd_cdiv(TS_NB + 1, TS_SCAN_BLOCK);
    hipLaunchKernelGGL(ts_scan_totals_kernel, dim3(nsb, 2), dim3(256), 0, st, (const int*)w.fcount, TS_NB + 1, (const int*)w.qcount, TS_NB,
                       w.ftotals, w.qtotals);
    hipLaunchKernelGGL(ts_scan_apply_kernel, dim3(nsb, 2), dim3(256), 0, st, w.fcount, TS_NB + 1, w.qcount, TS_NB, (const int*)w.ftotals,
                       (const int*)w.qtotals);
    hipLaunchKernelGGL(ts_scatter_kernel, dim3(kamd_cdiv(F, 256) + kamd_cdiv(N, 256)), dim3(256), 0, st, F, N, (const int*)w.fcount,
                       (const int*)w.qcount, (const int2*)w.fcr, (const int2*)w.qcr, w.fidx, w.qidx);
    hipLaunchKernelGGL(ts_tile_spheres_kernel<T>, dim3(ntiles), dim3(64), 0, st, F, (const int*)w.fidx, (const T*)rec,
                       (const float*)w.centres, (const float*)w.radius, w.tile_sphere);
    hipLaunchKernelGGL(ts_sort_records_kernel<T>, dim3(kamd_cdiv((long long)F * TD_REC, 256)), dim3(256), 0, st, F,
                       (const int*)w.fidx, (const T*)rec, (T*)w.rec_sorted);
  }
  KAMD_CHECK(hipGetLastError());
  const int ts_mode = kamd_env_int("KAMD_TS_MODE", 0);  // measurement knob: 1 = no tile slabs, 2 = no face planes
  const bool ts_stats = g_ts_stats_on != 0 || kamd_env_int("KAMD_TS_STATS", 0) != 0;  // (kamd_triangle_distance_work_counters: bench.py's VALU figure)
  if (ts_stats) KAMD_CHECK(kamd_zero_async(w.stats, 64, st));
  {
    kamd::ProfScope prof_(kamd::K_TD_MAIN, st);
    // queries per workgroup: neighbours share staged tiles (fewer, larger workgroups stage less in total), but a workgroup
    // pays for the union of its queries' tiles and small inputs need enough workgroups to fill the GPU
    // (profiles/r02q_ts_threads.txt, 50k faces: 100k queries 3.3 / 2.8 / 2.6 ms with 256 / 128 / 64; 1M queries 5.5 / 5.6 / 6.9)
    const int nt = kamd_test_env_int("KAMD_TS_THREADS", N <= 200000 ? 64 : (N <= 500000 ? 128 : 256));
    auto sweep = nt == 64 ? ts_sweep_kernel<T, 64> : (nt == 128 ? ts_sweep_kernel<T, 128> : ts_sweep_kernel<T, 256>);
    const int nthreads = nt == 64 ? 64 : (nt == 128 ? 128 : 256);
    hipLaunchKernelGGL(sweep, dim3(kamd_cdiv(N, nthreads)), dim3(nthreads), 0, st, N, F, points, (const T*)rec,
                       (const T*)w.rec_sorted, (const int*)w.qidx, (const int*)w.fidx, (const float*)w.tile_sphere, w.hard_count, w.hard_list,
                       ts_hard_threshold(N, ntiles), ts_mode, kamd_env_int("KAMD_TS_FEW", 32) - 1, ts_xcd_chunk(), ts_stats ? w.stats : nullptr, dist, face_idx, dist_type);
  }
  {
    kamd::ProfScope prof_(kamd::K_TD_FINAL, st);
    // static shares of the hard list: as for the soft mask's persistent kernels, two resident sets' worth of workgroups
    // balance better than one (profiles/r02_ts_hard_grid.txt: 4 / 8 / 12 / 16 / 32 per CU: 1.20 / 1.05 / 0.84 / 0.88 / 0.80 ms)
    static const int hard_per_cu = kamd_env_int("KAMD_TS_HARD_PER_CU", 16);
    hipLaunchKernelGGL(ts_hard_kernel<T>, dim3(KAMD_NUM_CU * hard_per_cu), dim3(TD_THREADS), 0, st, F, points, (const T*)rec,
                       (const T*)w.rec_sorted, (const int*)w.fidx, (const float*)w.tile_sphere, (const int*)w.hard_count, (const int*)w.hard_list, ts_mode, dist,
                       face_idx, dist_type);
  }
  if (ts_stats) {  // debugging aid: synchronous read-back
    unsigned long long h[8] = {0};
    int nh = 0;
    (void)hipStreamSynchronize(st);
    (void)hipMemcpy(h, w.stats, 64, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&nh, w.hard_count, 4, hipMemcpyDeviceToHost);
    for (int i = 0; i < 7; ++i) g_ts_stats_last[i] = h[i];
    g_ts_stats_last[7] = (unsigned long long)nh;
    if (g_ts_stats_on == 0)  // (the environment knob of experiment builds: print)
      fprintf(stderr, "[kamd] ts stats N=%d F=%d: tiles staged (per workgroup) %llu, tile walks (per wave) %llu, (query, tile) pairs %llu, "
            "face steps (per wave) %llu, closest-point evaluations %llu, hard queries %d, sum of tiles needed per query %llu, queries needing > 48 tiles %llu\n",
            N, F, h[0], h[1], h[2], h[3], h[4], nh, h[5], h[6]);
  }
  KAMD_CHECK(hipGetLastError());
  return td_reseed_launch<T>(st, N, F, points, (const T*)rec, rs, dist, face_idx, dist_type);
}
