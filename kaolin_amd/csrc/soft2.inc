// DIB-R soft mask over tile face lists (tile_lists.h) -- included by dibr_soft_mask.hip inside its anonymous namespace.
//
// Work items are 16 x 4-pixel sub-tiles that hold an uncovered pixel within reach of an enlarged face box (queued by the
// rasterizer's tile kernel in the fused path, by soft_items_kernel otherwise).  C4 (8 views x 1024^2, 50k faces): 5.8k
// items carry all 5.1M (pixel, face) hits.  The kernels of this path are bound by instruction issue, not by memory
// (rocprofv3 SQ counters, profiles/r02c_*), so the work is split by kind:
//   soft_select_kernel   one WAVEFRONT per item, integer / box work only: which faces does every pixel accept?
//     1. the 32 x 32 tile's entries ({64-face block, mask}) and the mesh's big faces are put in ascending block order
//        through a block bitmap in LDS (rank = popcount below; entries of one block OR together) -- ascending bit order
//        inside ascending blocks is the ascending face order of the reference's per-pixel loop
//        (dibr_soft_mask_cuda.cu:80-172);
//     2. faces are streamed 64 at a time (lane = face ordinal: binary search in the popcount prefix + bit select),
//        culled against the extent of the item's uncovered pixels (one 16-byte box load) and compacted in order;
//     3. per 64 candidates, lane = face forms the sub-tile's pixel mask from 16 column + 4 row tests, a 64 x 64 bit
//        transpose hands every pixel its faces, each pixel accepts its first (knum - hits so far) in order, a
//        transpose back gives, lane = face, the pixels that accepted it, and a scan lays the (pixel, face) pairs out
//        FACE-MAJOR in the item's segment of the pair list.
//   soft_eval_kernel     one 256-thread workgroup per item, one thread per accepted pair, no dependence between pairs:
//        the distance / probability arithmetic of the reference, with the per-edge divisor's reciprocal (a double
//        divide) read from the face record (computed once per face by the bin kernel, not per pair).  Probabilities are
//        also parked pixel-major in LDS, and wavefront 0 folds each pixel's prod(1 - prob) in hit order
//        (dibr_soft_mask_cuda.cu:174-179) once the item's pairs are done.
// Same expressions per (pixel, face), same hit order per pixel, same product order as the reference: soft_mask is
// bit-identical to the oracle.  The compact hit list is face-major inside an item, which lets the backward kernel sum
// the pixels of a face with register shuffles before it touches memory.

#ifndef KAMD_S2_ECAP
#define KAMD_S2_ECAP 192  // build knobs for experiments
#endif
#ifndef KAMD_SELECT_MIN_WAVES
#define KAMD_SELECT_MIN_WAVES 5
#endif
#ifndef KAMD_SELECT_EXPAND
#define KAMD_SELECT_EXPAND 1  // the slot of a streamed face by scatter + running maximum (0: binary search per face)
#endif
#ifndef KAMD_SELECT_STREAM
#define KAMD_SELECT_STREAM 2  // faces streamed per step = 64 x this (box loads in flight per lane).  With every chunk gathering its own boxes
                              // (rounds 2-6): 4 was the fastest (8 / 16: 95 / 131 VGPRs, 68.9 / 82.7 vs 63.3 us).  With the chunks' boxes parked /
                              // requested ahead (s2_select_item, step 2): 4 -> 2 at C4 select + rounds 49.0 -> 47.9 us (48.7 before the change),
                              // shuffled knot 271 -> 265 (275 before), knot 227 -> 223 (224): profiles/r06zw_soft_select_box_prefetch_ab.txt
#endif
#ifndef KAMD_SOFT_NT
#define KAMD_SOFT_NT 2  // the hit list is streamed (nontemporal): 0 = plain, 1 = eval's stores + the backward's loads, 2 = + eval's pair loads (step 0.503-0.509 / 0.501 / 0.496 ms)
#endif
typedef int s2_i32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int s2_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int2 s2_load_pair(const int2* p, bool stream) {
  if (stream) {
    const s2_i32x2 v = __builtin_nontemporal_load(reinterpret_cast<const s2_i32x2*>(p));
    return make_int2(v.x, v.y);
  }
  return *p;
}
constexpr int S2_STREAM = KAMD_SELECT_STREAM;
constexpr int S2_ECAP = KAMD_S2_ECAP;                 // (pseudo-)entries of a tile ordered in LDS (more: scan the whole mesh)
constexpr int S2_BITWORDS = 256;             // block bitmap words at most: meshes of up to 8192 blocks (524k faces) per batch item
// the words a launch really needs (the bitmap and its prefix are dynamic LDS: 2 x this many words).  The select kernels' workgroup is
// ONE wavefront, so LDS per workgroup is what bounds the wavefronts a CU holds: 6.6 KB with the full table = 6 per SIMD; a 50 000-face
// mesh needs 28 words, 4.8 KB = 8 per SIMD -- scenes with many light items (the knot: 37 600) are bound by exactly that.
inline int s2_bitwords_of(int F) {
  const long long nblk = ((long long)(F > 0 ? F : 1) + 63) / 64 + 1;  // (a mesh's first packed face need not start a block)
  long long w = ((nblk + 31) / 32 + 3) & ~3ll;
  return (int)(w < 4 ? 4 : (w > S2_BITWORDS ? S2_BITWORDS : w));
}
#ifndef KAMD_EVAL_THREADS
#define KAMD_EVAL_THREADS 256  // build knob for experiments
#endif
constexpr int S2_EVAL_THREADS = KAMD_EVAL_THREADS;
#ifndef KAMD_EVAL_WAVES
#define KAMD_EVAL_WAVES 0  // waves per SIMD the fp32 eval kernel is compiled for (0: the compiler's choice, 72 VGPRs = 7; 8 spills 36 bytes)
#endif
constexpr int S2_LDS_KMAX = 128;             // knum up to which the eval kernel folds the products from LDS
constexpr int WORK_HEADER_WORDS = tl::WORK_HEADER;  // work[s * COUNTER_STRIDE], s = 0..7: per-shard item counts; items (uint4) follow the header

// Hits of the autograd path (no K-buffers).  The select kernel leaves the accepted (pixel, face) pairs SEGMENTED, item by item
// (item i owns pair[i*64*K, i*64*K + item_count[i]), face-major); the eval kernel evaluates them and appends the finished hits
// to a flat list (every item takes a contiguous range of its shard: one atomic per item) of self-contained records, which
// the backward kernel streams without looking at items at all -- rounds of 256 consecutive hits, evenly dealt.
constexpr int FLAT_SHARDS = 64;                // the flat list is FLAT_SHARDS lists: an item appends to shard (item % FLAT_SHARDS).  (ONE
                                               // append counter made the eval kernel 5x slower: same-address device atomics complete one
                                               // at a time, ~50 ns each, and there is one per item)
constexpr int FLAT_COUNT_WORD = tl::WORK_FLAT_WORD;  // work[FLAT_COUNT_WORD + s * COUNTER_STRIDE]: records in shard s (zeroed with the worklist header;
                                                     // one counter per 128-byte line: atomics on one line complete one at a time)
static_assert(FLAT_COUNT_WORD + FLAT_SHARDS * tl::COUNTER_STRIDE <= tl::WORK_HEADER, "worklist header too small");
constexpr unsigned int FLAT_KEY_BITS = 29;     // rec.x = (b * F + face) | (which-of-six << 29): B * F < 2^29
constexpr unsigned int FLAT_KEY_MASK = (1u << FLAT_KEY_BITS) - 1u;
// records a shard must be able to hold: every item id is in [0, n_items) and ids are dealt round-robin
__host__ __device__ inline size_t flat_shard_cap(size_t n_items, int K) {
  return ((n_items + FLAT_SHARDS - 1) / FLAT_SHARDS) * 64 * (size_t)(K > 0 ? K : 0);
}
template <typename T>
struct HitList2 {
  int2* pair;          // segmented: {face (mesh-relative), (pixel of the sub-tile 0..63) << 16 | the hit's rank among the pixel's hits}
  T* prob;             // flat: probability of hit i
  uint2* rec;          // flat: {(b * F + face) | which << 29, row << 16 | col}
  int* item_count;     // indexed by item id = (tile * B + b) * 16 + sub
  unsigned int* flat_count;   // [FLAT_SHARDS * COUNTER_STRIDE], shard s at s * COUNTER_STRIDE
  size_t shard_cap;           // shard s owns the flat records [s * shard_cap, s * shard_cap + flat_count[s])
};

struct WorkView {
  unsigned int end[tl::WORK_SHARDS];  // inclusive prefix sums of the shard counts (read once per kernel)
  const uint4* items;                 // WORK_SHARDS x shard_cap {item id, unc.lo, unc.hi, 0}
  unsigned int shard_cap;
};
__device__ __forceinline__ WorkView work_view(const unsigned int* __restrict__ work, unsigned int shard_cap) {
  WorkView wv;
  unsigned int run = 0;
#pragma unroll
  for (int s = 0; s < tl::WORK_SHARDS; ++s) {
    run += min(work[s * tl::COUNTER_STRIDE], shard_cap);
    wv.end[s] = run;
  }
  wv.items = reinterpret_cast<const uint4*>(work + WORK_HEADER_WORDS);
  wv.shard_cap = shard_cap;
  return wv;
}
// g-th item of the concatenated shards -> its record; false past the end
__device__ __forceinline__ bool work_fetch(const WorkView& wv, unsigned int g, uint4* out) {
  if (g >= wv.end[tl::WORK_SHARDS - 1]) return false;
  int s = 0;
  unsigned int before = 0;
#pragma unroll
  for (int i = 0; i < tl::WORK_SHARDS - 1; ++i)
    if (g >= wv.end[i]) {
      s = i + 1;
      before = wv.end[i];
    }
  *out = wv.items[(size_t)s * wv.shard_cap + (g - before)];
  return true;
}
__device__ __forceinline__ unsigned int work_total(const WorkView& wv) { return wv.end[tl::WORK_SHARDS - 1]; }

// The persistent kernels' own enumeration: place w = (shard w % WORK_SHARDS, position w / WORK_SHARDS).  A place's address does
// not depend on the shard counts, so a workgroup requests its first item TOGETHER with the counts instead of after them -- one
// dependent round trip less per workgroup, and most workgroups of the search take one item.  A place past its shard's count
// holds no item.  (Uniform per workgroup: scalar loads.)
struct WorkCounts {
  unsigned int n[tl::WORK_SHARDS];
  unsigned int places;  // WORK_SHARDS * (the longest shard's count): every item lies at a place below this
};
__device__ __forceinline__ WorkCounts work_counts(const unsigned int* __restrict__ work, unsigned int shard_cap) {
  WorkCounts wc;
  unsigned int longest = 0u;
#pragma unroll
  for (int s = 0; s < tl::WORK_SHARDS; ++s) {
    wc.n[s] = min(work[s * tl::COUNTER_STRIDE], shard_cap);
    longest = max(longest, wc.n[s]);
  }
  wc.places = longest * tl::WORK_SHARDS;
  return wc;
}
__device__ __forceinline__ const uint4* work_place(const unsigned int* __restrict__ work, unsigned int shard_cap, unsigned int w) {
  const unsigned int pos = min(w / tl::WORK_SHARDS, shard_cap - 1u);  // (clamped: a speculative read stays inside the buffer)
  return reinterpret_cast<const uint4*>(work + WORK_HEADER_WORDS) + (size_t)(w % tl::WORK_SHARDS) * shard_cap + pos;
}
__device__ __forceinline__ bool work_place_holds(const WorkCounts& wc, unsigned int w) {
  unsigned int n = 0u;
#pragma unroll
  for (int s = 0; s < tl::WORK_SHARDS; ++s) n = (w % tl::WORK_SHARDS) == (unsigned int)s ? wc.n[s] : n;
  return w / tl::WORK_SHARDS < n;
}

// r-th (0-based) set bit of m (r < popcount(m))
__device__ __forceinline__ int select_bit64(unsigned long long m, int r) {
  unsigned int w = (unsigned int)m;
  int pos = 0, c = __popc(w);
  if (r >= c) {
    r -= c;
    pos = 32;
    w = (unsigned int)(m >> 32);
  }
  c = __popc(w & 0xFFFFu);
  if (r >= c) { r -= c; pos += 16; w >>= 16; }
  w &= 0xFFFFu;
  c = __popc(w & 0xFFu);
  if (r >= c) { r -= c; pos += 8; w >>= 8; }
  w &= 0xFFu;
  c = __popc(w & 0xFu);
  if (r >= c) { r -= c; pos += 4; w >>= 4; }
  w &= 0xFu;
  c = __popc(w & 3u);
  if (r >= c) { r -= c; pos += 2; w >>= 2; }
  w &= 3u;
  if (r >= (int)(w & 1u)) pos += 1;
  return pos;
}

// line coefficients of an edge and the divisor (down + EPS) of its foot point (dibr_soft_mask_cuda.cu:112-125)
template <typename T>
__device__ __forceinline__ void edge_coeffs(T x1, T y1, T x2, T y2, EdgeInv<T>* e, double* den) {
  const T A = y2 - y1, Bc = x1 - x2, C = x2 * y1 - x1 * y2;
  const T down = A * A + Bc * Bc;
  e->A = A;
  e->B = Bc;
  e->C = C;
  e->AA = A * A;
  e->BB = Bc * Bc;
  e->AB = A * Bc;
  e->AC = A * C;
  e->BC = Bc * C;
  *den = (double)down + DIBR_EPS;
}

// ---- classification from a given selected_face_idx (the standalone soft-mask operators) ---------------------------------
// One 256-thread workgroup per 16 x 16 pixels (wavefront = 16 x 4 sub-tile), the same grouping as the rasterizer's tile
// kernel: covered pixels get 1, uncovered ones 0 (the search overwrites the band), sub-tiles with uncovered pixels within
// reach of an enlarged box are queued.
template <typename T>
__global__ __launch_bounds__(256) void soft_items_kernel(int B, int H, int W, int has_faces, const int64_t* __restrict__ sel_idx,
                                                         T* __restrict__ soft_mask, uint8_t* __restrict__ hit_count,
                                                         tl::Lists LS, int tiles_x_r, unsigned int* work, unsigned int shard_cap) {
  __shared__ unsigned long long s_item_unc[4];
  const int b = blockIdx.x % B, tile = blockIdx.x / B;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile_x = (tile % tiles_x_r) * tl::R_TILE, tile_y = (tile / tiles_x_r) * tl::R_TILE;
  const int sub_x = tile_x, sub_y = tile_y + wave * SUB_H;
  const int col = sub_x + (lane & 15), row = sub_y + (lane >> 4);
  const bool in_image = col < W && row < H;
  const size_t p = ((size_t)b * H + row) * W + col;
  const bool uncovered = in_image && (int)sel_idx[in_image ? p : 0] < 0;
  if (in_image) {
    soft_mask[p] = uncovered ? (T)(1.0 - 1.0) : (T)1.0;
    if (hit_count) hit_count[p] = 0;
  }
  const unsigned long long unc = __ballot(uncovered);
  tl::queue_items(unc, has_faces != 0, B, b, tile_x, tile_y, wave, lane, LS.sub_touched, LS.big_count, LS.tiles_x, LS.ntiles,
                  reinterpret_cast<uint4*>(work + WORK_HEADER_WORDS), work, shard_cap, s_item_unc);
}

PHASE_TABLE(g_phase_select)

// decoded work item
struct ItemGeom {
  int item, b, sub_x, sub_y;
  unsigned long long unc;
};
__device__ __forceinline__ ItemGeom item_geom(const uint4& wrec, int B, int tiles_x_s) {
  ItemGeom g;
  g.item = (int)wrec.x;
  g.unc = ((unsigned long long)wrec.z << 32) | wrec.y;
  const int ss = g.item % tl::S_SUBS;
  g.b = (g.item / tl::S_SUBS) % B;
  const int st = g.item / (tl::S_SUBS * B);
  g.sub_x = (st % tiles_x_s) * tl::S_TILE + (ss & 1) * SUB_W;
  g.sub_y = (st / tiles_x_s) * tl::S_TILE + (ss >> 1) * SUB_H;
  return g;
}

template <typename T>
struct Select2Args {
  int B, F, H, W, K;
  float multiplier;
  const T* rec;              // soft records, tl::rec_s_scalars scalars per face
  tl::Lists L;               // soft pass lists
  const unsigned int* work;
  unsigned int shard_cap;
  unsigned short* pixcnt;    // [item * 64 + pixel]: hits the pixel accepted
  HitList2<T> list;          // compact form: pair + item_count are written here
  int64_t* idx_out;          // K-buffer form (reference contract): close_face_idx
  uint8_t* hit_count;        // K-buffer form, optional
  // the places of the items whose tile holds more entries than the kernel orders at once: appended by soft_select_kernel, taken
  // by soft_select_rounds_kernel (nullptr: such items scan their whole mesh)
  unsigned int* over_count;  // zeroed
  unsigned int* over_list;   // [work places]
  // the items' records {item id, unc.lo, unc.hi, pairs} dealt into S2_CLASSES lists by their pair count, heaviest class first: what
  // soft_eval_kernel walks (written by soft_select_rounds_kernel, which runs after every item has its count)
  unsigned int* ord_count;   // [S2_CLASSES * tl::COUNTER_STRIDE], zeroed: a 128-byte line per class
  uint4* ord_list;           // [S2_CLASSES * ord_cap]
  unsigned int ord_cap;      // work places
  int bitwords;              // words of the block bitmap in LDS (s2_bitwords_of(F); the launches pass 2 x 4 x this many bytes of dynamic LDS)
};
constexpr int S2_CLASSES = 4;
constexpr unsigned int S2_HANDED_OVER = 0xFFFFFFFFu;  // fourth word of the work record of an item the main launch handed to the rounds launch
__device__ __forceinline__ int s2_class_of(unsigned int pairs) { return pairs >= 768u ? 0 : (pairs >= 256u ? 1 : (pairs >= 1u ? 2 : 3)); }

// the select kernel's LDS tables (generic pointers: the kernel's own, inlined copy of the item code resolves them to LDS instructions)
template <typename T>
struct S2Tables {
  unsigned int* eblk;
  unsigned long long* emask;
  int* epfx;
  unsigned int* bits;
  int* wpfx;
  int* cand;
  Box4<T>* box0;  // the boxes of the candidates cand[0 .. 63]
  int* spos;
  T* px;
  T* py;
};

// One work item (a 16 x 4 sub-tile with uncovered pixels within reach of some enlarged box) by one wavefront.
template <typename T, bool LEAN, bool ROUNDS>
__device__ __forceinline__ void s2_select_item(const Select2Args<T>& a, const S2Tables<T>& t, const uint4 wrec, const unsigned int wi_) {
  const int lane = threadIdx.x;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  const int B = a.B, F = a.F, K = a.K;
  const float multiplier = a.multiplier;
  PHASE_DECL;
  const ItemGeom ig = item_geom(wrec, B, a.L.tiles_x);
  const int item = ig.item, b = ig.b, sub_x = ig.sub_x, sub_y = ig.sub_y;
  const unsigned long long unc = ig.unc;
  const int st = item / (tl::S_SUBS * B);
  const int col = sub_x + (lane & 15), row = sub_y + (lane >> 4);
  const bool uncovered = ((unc >> lane) & 1ull) != 0ull;  // (bits exist for pixels inside the image only)
  const size_t p1 = ((size_t)b * a.H + row) * a.W + col;
  const long long first_b = (long long)b * F;
  const size_t seg_base = (size_t)item * 64 * (size_t)K;

  const T x0 = pixel_x(multiplier, a.W, col);
  const T y0 = pixel_y(multiplier, a.H, row);
  __syncthreads();  // the previous item is done with the LDS tables
  if (lane < SUB_W) t.px[lane] = x0;
  if ((lane & 15) == 0) t.py[lane >> 4] = y0;
  T ux_min = uncovered ? x0 : (T)INFINITY, ux_max = uncovered ? x0 : (T)-INFINITY;
  T uy_min = uncovered ? y0 : (T)INFINITY, uy_max = uncovered ? y0 : (T)-INFINITY;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    ux_min = fmin(ux_min, __shfl_xor(ux_min, d, 64));
    ux_max = fmax(ux_max, __shfl_xor(ux_max, d, 64));
    uy_min = fmin(uy_min, __shfl_xor(uy_min, d, 64));
    uy_max = fmax(uy_max, __shfl_xor(uy_max, d, 64));
  }

  // per-PIXEL state lives in the lane that owns the pixel
  int kid = 0;
  bool active = uncovered && K > 0;
  int item_pairs = 0;

  // ---- 1. the tile's candidate faces in ascending order.  The tile's entries ({64-face block, mask}: those that reach this item's
  // sub-tile) and its mesh's big faces are ranked by block through a bitmap over the mesh's blocks (rank = set bits below) and merged
  // per block into S2_ECAP ordered slots.  ROUNDS (round 5): a tile with more entries than slots -- a mesh whose face order has no
  // locality leaves one face per entry, thousands per tile; a view with many big faces -- takes them in rounds of S2_ECAP
  // consecutive ranks, streaming its entries from memory once for the bitmap and once per round (before, such a tile scanned every
  // face of its mesh: the knot scene with shuffled faces, soft_select 746 us -> 322).
  const tl::TileSrc src = tl::tile_src(a.L, b, st);
  const unsigned int n_big = a.L.big_count[b];
  const long long blk0 = first_b >> 6;
  const long long nblk = ((first_b + F - 1) >> 6) - blk0 + 1;
  if constexpr (!ROUNDS) {
    if (a.over_list != nullptr && !src.brute && src.n + n_big > (unsigned int)S2_ECAP && nblk <= (long long)a.bitwords * 32) {
      if (lane == 0) {
        a.over_list[atomicAdd(a.over_count, 1u)] = wi_;
        const_cast<uint4*>(work_place(a.work, a.shard_cap, wi_))->w = S2_HANDED_OVER;
      }
      return;  // (the rounds launch takes the item)
    }
  }
  const bool brute = src.brute || (!ROUNDS && src.n + n_big > (unsigned int)S2_ECAP) || nblk > (long long)a.bitwords * 32;
  const int n_e = brute ? 0 : (int)(src.n + n_big);
  int n_u = 0;   // distinct blocks
  int n_f = F;
  PHASE_MARK(0);
  // entry e of the tile's pseudo-list: block and (0 when it does not reach this item's sub-tile) face mask
  auto entry_of = [&](int e, unsigned int* blk_out) -> unsigned long long {
    if (e < (int)src.n) {
      const uint4 en = tl::tile_entry(a.L, src, (unsigned int)e);
      *blk_out = en.x;
      // an entry whose faces do not reach this item's sub-tile contributes nothing: most of a tile's ~1 400
      // candidates are never streamed
      return ((en.y >> (item & (tl::S_SUBS - 1))) & 1u) ? (((unsigned long long)en.w << 32) | en.z) : 0ull;
    }
    const unsigned int* be = a.L.big_list + 3 * ((size_t)first_b + (size_t)(e - (int)src.n));  // (the mesh's big faces, merged per block)
    *blk_out = be[0];
    return ((unsigned long long)be[2] << 32) | be[1];
  };
  auto rank_of = [&](unsigned int bk) -> int {
    const unsigned int rel = (unsigned int)(bk - blk0);
    return t.wpfx[rel >> 5] + __popc(t.bits[rel >> 5] & ((1u << (rel & 31u)) - 1u));
  };
  // inclusive popcount prefix over the first n ordered slots -> the faces they hold
  auto prefix_slots = [&](int n) -> int {
    int carry = 0;
    for (int e0 = 0; e0 < n; e0 += 64) {
      const int e = e0 + lane;
      const int c = e < n ? __popcll(t.emask[e]) : 0;
      const int inc = wave_inclusive_scan(c);
      if (e < n) t.epfx[e] = carry + inc;
      carry += __shfl(inc, 63, 64);
    }
    __syncthreads();
    return carry;
  };
  if (!brute) {
    const int nw = (int)((nblk + 31) >> 5);
    for (int w = lane; w < nw; w += 64) t.bits[w] = 0u;
    if (!ROUNDS)
      for (int e = lane; e < n_e; e += 64) t.emask[e] = 0ull;
    __syncthreads();
    unsigned int blk[ROUNDS ? 1 : S2_ECAP / 64];  // (the common tile: its entries stay in registers between the bitmap and the slots)
    unsigned long long mask[ROUNDS ? 1 : S2_ECAP / 64];
    if constexpr (!ROUNDS) {
#pragma unroll
      for (int i = 0; i < S2_ECAP / 64; ++i) {
        const int e = i * 64 + lane;
        blk[i] = 0u;
        mask[i] = 0ull;
        if (e < n_e) {
          mask[i] = entry_of(e, &blk[i]);
          const unsigned int rel = (unsigned int)(blk[i] - blk0);
          if (mask[i] != 0ull) atomicOr(&t.bits[rel >> 5], 1u << (rel & 31u));
        }
      }
    } else {
      for (int e = lane; e < n_e; e += 64) {
        unsigned int bk;
        const unsigned long long m = entry_of(e, &bk);
        const unsigned int rel = (unsigned int)(bk - blk0);
        if (m != 0ull) atomicOr(&t.bits[rel >> 5], 1u << (rel & 31u));
      }
    }
    __syncthreads();
    {  // exclusive popcount prefix over the bitmap words
      int carry = 0;
      for (int w0 = 0; w0 < nw; w0 += 64) {
        const int w = w0 + lane;
        const int c = w < nw ? __popc(t.bits[w]) : 0;
        const int inc = wave_inclusive_scan(c);
        if (w < nw) t.wpfx[w] = carry + inc - c;
        carry += __shfl(inc, 63, 64);
      }
      n_u = carry;
    }
    __syncthreads();
    if constexpr (!ROUNDS) {
#pragma unroll
      for (int i = 0; i < S2_ECAP / 64; ++i) {
        const int e = i * 64 + lane;
        if (e < n_e && mask[i] != 0ull) {
          const int rank = rank_of(blk[i]);
          t.eblk[rank] = blk[i];
          atomicOr(&t.emask[rank], mask[i]);  // a big face next to its wavefront's entry: same block, masks OR together
        }
      }
      __syncthreads();
      n_f = prefix_slots(n_u);
    }
  }
  // ROUNDS: the ordered slots of the ranks [base, base + S2_ECAP)
  auto fill_round = [&](int base) -> int {
    const int n_ur = min(S2_ECAP, n_u - base);
    for (int e = lane; e < n_ur; e += 64) t.emask[e] = 0ull;
    __syncthreads();
    for (int e = lane; e < n_e; e += 64) {
      unsigned int bk;
      const unsigned long long m = entry_of(e, &bk);
      if (m == 0ull) continue;
      const int rank = rank_of(bk) - base;
      if (rank >= 0 && rank < S2_ECAP) {
        t.eblk[rank] = bk;
        atomicOr(&t.emask[rank], m);
      }
    }
    __syncthreads();
    return prefix_slots(n_ur);
  };
  const int n_rounds = (ROUNDS && !brute) ? (n_u + S2_ECAP - 1) / S2_ECAP : 1;

  PHASE_MARK(1);
  // ---- 3. one chunk of n (<= 64) candidates, ascending in t.cand; returns true when every pixel is saturated
  // lane = face forms its pixel mask, ONE 64 x 64 bit transpose hands every pixel its faces, each pixel accepts its first
  // (knum - hits so far) in order; then a wave-uniform loop over the faces that some pixel accepted: the compare that
  // asks "did my pixel accept face k" leaves, as its scalar result, the face's pixels -- every accepting lane stores its
  // pair at (pairs so far + accepting lanes below it): FACE-MAJOR, pixels ascending inside a face, coalesced, no LDS, no
  // barrier (the round-2 form -- transpose back, 2-byte codes per pair staged in LDS by a per-lane loop over up to 64 set
  // bits, copy-out -- spent a third of the kernel there).
  auto process_chunk = [&](int c0, int n, const Box4<T>& bb) -> bool {  // (bb: the box of candidate c0 + lane)
    PHASE_MARK(2);
    unsigned long long inside = 0ull;  // lane = face: the item's uncovered pixels whose centre its box holds
    int fid = 0;
    if (lane < n) {
      fid = (int)(t.cand[c0 + lane] - first_b);
      unsigned cols = 0, rows = 0;
#pragma unroll
      for (int c = 0; c < SUB_W; ++c) {
        const T x = t.px[c];
        cols |= ((x < bb.x0) | (x >= bb.x1)) ? 0u : (1u << c);
      }
#pragma unroll
      for (int r = 0; r < SUB_H; ++r) {
        const T y = t.py[r];
        rows |= ((y < bb.y0) | (y >= bb.y1)) ? 0u : (1u << r);
      }
#pragma unroll
      for (int r = 0; r < SUB_H; ++r) inside |= ((rows >> r) & 1u) ? ((unsigned long long)cols << (SUB_W * r)) : 0ull;
      inside &= unc;
    }
    PHASE_MARK(3);
    const unsigned long long hm = wave_transpose64(inside);  // lane = pixel: the chunk's faces (ascending) holding its centre
    const int cnt = active ? min(__popcll(hm), K - kid) : 0;
    unsigned long long r = hm;
    for (int i = 0; i < cnt; ++i) r &= r - 1ull;
    const unsigned long long acc = hm & ~r;
    const unsigned int acc_lo = (unsigned int)acc, acc_hi = (unsigned int)(acc >> 32);
    int y = (lane << 16) | kid;  // the pair's second word: (pixel << 16) | rank; the rank advances with every accepted face
    kid += cnt;
    if (kid >= K) active = false;
    PHASE_MARK(4);
    {
      const unsigned int any_lo = tl::wave_or_u32(acc_lo), any_hi = tl::wave_or_u32(acc_hi);  // faces some pixel accepted
      for (int half = 0; half < 2; ++half) {
        const unsigned int word = half ? acc_hi : acc_lo;
        for (unsigned int todo = half ? any_hi : any_lo; todo != 0u; todo &= todo - 1u) {  // (wave-uniform)
          const int kb = __ffs((int)todo) - 1;
          const unsigned int bit = __builtin_amdgcn_ubfe(word, (unsigned int)kb, 1u);
          const bool mine = bit != 0u;
          const unsigned long long m = __ballot(mine);
          const int fk = __builtin_amdgcn_readlane(fid, half * 32 + kb);
          if (mine) {
            if (LEAN) {
              // (the lanes below this one that accepted the face: two mbcnt instructions; the pair's byte offset in the item's
              // segment fits 32 bits -- 64 * K pairs of 8 bytes -- so the store takes a scalar base and a 32-bit lane offset)
              const unsigned int below = __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
              const unsigned int off = ((unsigned int)item_pairs + below) * (unsigned int)sizeof(int2);
              *reinterpret_cast<int2*>(reinterpret_cast<char*>(a.list.pair + seg_base) + off) = make_int2(fk, y);
            } else {
              a.idx_out[p1 * K + (y & 0xFFFF)] = fk;
            }
            ++y;
          }
          item_pairs += __popcll(m);
        }
      }
    }
    PHASE_MARK(5);
    return !__any(active);
  };

  // ---- 2. stream the faces (S2_STREAM x 64 per step: that many box loads in flight per lane), cull, compact in order
  int ncand = 0;
  bool done = false;
  Box4<T> left_box = Box4<T>{0, 0, 0, 0};  // lane < ncand: the box of left-over candidate `lane`
  for (int rd = 0; rd < n_rounds && !done; ++rd) {
  int n_ur = n_u;  // ordered slots of this round
  if (ROUNDS && !brute) {
    n_ur = min(S2_ECAP, n_u - rd * S2_ECAP);
    n_f = fill_round(rd * S2_ECAP);
  }
  // (the rounds launch only: its tiles fill all S2_ECAP slots round after round -- shuffled knot 109 -> 99 us; the common item's few
  // slots are found faster by the search: C4 -1 us, knot +7, profiles/r06x_*)
  constexpr bool EXPAND = KAMD_SELECT_EXPAND != 0 && ROUNDS;
  // Which ordered slot holds the j-th face of the round: the slots scatter themselves to the positions of their FIRST faces, a running
  // maximum over the positions (DPP row shifts) hands every lane its slot.  (Rounds 2-5: a binary search over the slots' prefix per
  // face, eight dependent LDS reads, one search after the other for the S2_STREAM faces of a lane.)
  int sstart[S2_ECAP / 64];  // first face of the slots lane, lane + 64, ... (a slot past the round's: never inside a step)
#pragma unroll
  for (int e = 0; e < S2_ECAP / 64; ++e) {
    const int sl = e * 64 + lane;
    sstart[e] = (EXPAND && !brute && sl < n_ur) ? (sl > 0 ? t.epfx[sl - 1] : 0) : 0x7fffffff;
  }
  int slot_carry = 0;  // (slot + 1) of the face before the step's first
  for (int j0 = 0; j0 < n_f && !done; j0 += 64 * S2_STREAM) {
    int id[S2_STREAM];
    bool keep[S2_STREAM];
    int slot_of[S2_STREAM] = {};
    if (EXPAND && !brute) {
#pragma unroll
      for (int i = 0; i < S2_STREAM; ++i) t.spos[i * 64 + lane] = 0;
      __syncthreads();
#pragma unroll
      for (int e = 0; e < S2_ECAP / 64; ++e)
        if (sstart[e] >= j0 && sstart[e] < j0 + 64 * S2_STREAM) t.spos[sstart[e] - j0] = e * 64 + lane + 1;
      __syncthreads();
#pragma unroll
      for (int i = 0; i < S2_STREAM; ++i) {
        int v = t.spos[i * 64 + lane];
        v = max(v, row_shr<1>(v));
        v = max(v, row_shr<2>(v));
        v = max(v, row_shr<4>(v));
        v = max(v, row_shr<8>(v));
        const int t0 = __builtin_amdgcn_readlane(v, 15), t1 = __builtin_amdgcn_readlane(v, 31), t2 = __builtin_amdgcn_readlane(v, 47);
        v = max(v, lane >= 16 ? t0 : 0);
        v = max(v, lane >= 32 ? t1 : 0);
        v = max(v, lane >= 48 ? t2 : 0);
        v = max(v, slot_carry);
        slot_of[i] = v - 1;
        slot_carry = __builtin_amdgcn_readlane(v, 63);
      }
    }
#pragma unroll
    for (int i = 0; i < S2_STREAM; ++i) {
      const int j = j0 + i * 64 + lane;
      id[i] = 0;
      if (j < n_f) {
        if (brute) {
          id[i] = (int)(first_b + j);
        } else {
          int lo = 0;
          if constexpr (EXPAND) {
            lo = slot_of[i];
          } else {
            int hi = n_ur;
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (t.epfx[mid] > j) hi = mid; else lo = mid + 1;
            }
          }
          const int rr = j - (lo > 0 ? t.epfx[lo - 1] : 0);
          id[i] = (int)(t.eblk[lo] * 64u) + select_bit64(t.emask[lo], rr);
        }
      }
    }
    Box4<T> bb[S2_STREAM];
#pragma unroll
    for (int i = 0; i < S2_STREAM; ++i) {
      keep[i] = false;
      bb[i] = Box4<T>{0, 0, 0, 0};
      if (j0 + i * 64 + lane < n_f) {
        bb[i] = *reinterpret_cast<const Box4<T>*>(tl::soft_box<T>(a.rec, (size_t)id[i]));
        keep[i] = !((ux_max < bb[i].x0) | (ux_min >= bb[i].x1) | (uy_max < bb[i].y0) | (uy_min >= bb[i].y1));
      }
    }
    __syncthreads();  // process_chunk / the move below are done with t.cand and t.box0
    // The boxes of the step's FIRST chunk are parked in LDS as they are compacted (the left-over's, requested when it was moved, have
    // arrived behind this step's own loads); the boxes of every further chunk are requested before the chunk in front of it is
    // processed.  (Rounds 2-6: every chunk began with a gather of its 64 boxes -- a memory round trip in the item's dependent chain
    // per chunk, on top of the step's own.)
    if (lane < ncand) t.box0[lane] = left_box;
#pragma unroll
    for (int i = 0; i < S2_STREAM; ++i) {
      const unsigned long long m = __ballot(keep[i]);
      const int pos = ncand + __popcll(m & lt_mask);
      if (keep[i]) {
        t.cand[pos] = id[i];
        if (pos < 64) t.box0[pos] = bb[i];
      }
      ncand += __popcll(m);
    }
    __syncthreads();
    const bool last = rd == n_rounds - 1 && j0 + 64 * S2_STREAM >= n_f;  // (a round's left-over candidates go first in the next one)
    int c0 = 0;
    Box4<T> cur = t.box0[lane];
    while (ncand - c0 >= 64 || (last && ncand - c0 > 0)) {
      const int n = min(64, ncand - c0);
      Box4<T> nxt = Box4<T>{0, 0, 0, 0};
      if (c0 + 64 + lane < ncand) nxt = *reinterpret_cast<const Box4<T>*>(tl::soft_box<T>(a.rec, (size_t)t.cand[c0 + 64 + lane]));
      done = process_chunk(c0, n, cur);
      cur = nxt;
      c0 += n;
      if (done) break;
    }
    // the left-over (< 64 candidates) goes to the front; `cur` holds their boxes (requested as the chunk after the last one processed)
    const int rest = done ? 0 : ncand - c0;
    const int moved = lane < rest ? t.cand[c0 + lane] : 0;
    __syncthreads();
    if (lane < rest) t.cand[lane] = moved;
    left_box = cur;
    ncand = rest;
  }
  }
  PHASE_MARK(2);
  a.pixcnt[(size_t)item * 64 + lane] = (unsigned short)(kid > 65535 ? 65535 : kid);
  if (lane == 0) {
    if (LEAN) a.list.item_count[item] = item_pairs;
    // ... and in the item's record (its fourth word), where the eval kernel finds it with the item: one round trip less.  An item of
    // the rounds launch deals its record into the eval kernel's lists itself (the dealing pass of that launch skips it)
    if (!ROUNDS) {
      const_cast<uint4*>(work_place(a.work, a.shard_cap, wi_))->w = (unsigned int)item_pairs;
    } else if (a.ord_list != nullptr) {
      const int c = s2_class_of((unsigned int)item_pairs);
      const unsigned int pos = atomicAdd(a.ord_count + c * tl::COUNTER_STRIDE, 1u);
      if (pos < a.ord_cap) a.ord_list[(size_t)c * a.ord_cap + pos] = make_uint4(wrec.x, wrec.y, wrec.z, (unsigned int)item_pairs);
    }
  }
  if (!LEAN && uncovered && a.hit_count) a.hit_count[p1] = (uint8_t)(kid > 255 ? 255 : kid);
  PHASE_MARK(6);
  PHASE_FLUSH(g_phase_select);
}
#define KAMD_S2_TABLES                                                                                                       \
  __shared__ unsigned int s_eblk[S2_ECAP];                                                                                  \
  __shared__ unsigned long long s_emask[S2_ECAP];                                                                           \
  __shared__ int s_epfx[S2_ECAP];                                                                                           \
  extern __shared__ __attribute__((aligned(16))) unsigned int s_union[]; /* 2 * a.bitwords words (s2_bitwords_of: by the mesh's size) */ \
  __shared__ int s_cand[64 + S2_STREAM * 64];                                                                               \
  __shared__ Box4<T> s_box0[64];                                                                                            \
  __shared__ T s_px[SUB_W], s_py[SUB_H];                                                                                    \
  const S2Tables<T> t{s_eblk, s_emask, s_epfx, s_union, reinterpret_cast<int*>(s_union + a.bitwords), s_cand, s_box0, s_cand + 64 /* spos: free while a step looks its slots up (fewer than 64 candidates are left over) */, s_px, s_py}

template <typename T, bool LEAN>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(KAMD_SELECT_MIN_WAVES, 8))) void soft_select_kernel(Select2Args<T> a) {
  KAMD_S2_TABLES;
  uint4 wrec = a.shard_cap ? *work_place(a.work, a.shard_cap, blockIdx.x) : make_uint4(0u, 0u, 0u, 0u);  // (speculative: see work_counts)
  const WorkCounts wc = work_counts(a.work, a.shard_cap);
  for (unsigned int wi_ = blockIdx.x; wi_ < wc.places; wi_ += gridDim.x) {
    if (wi_ != blockIdx.x) wrec = *work_place(a.work, a.shard_cap, wi_);
    if (!work_place_holds(wc, wi_)) continue;
    s2_select_item<T, LEAN, false>(a, t, wrec, wi_);
  }
}
// The items the kernel above handed over (tiles with more entries than ordered slots), in rounds.  A launch of its own: the rounds'
// extra loop level costs the common item 25 % when it shares the kernel above, which sits at its register limit (inlined: 53 vs 42 us
// at C4; out of line, a call: 50 -- its stack makes every wavefront of the launch a scratch wavefront).  A small persistent grid: with
// nothing handed over (every scene whose face order has some locality) each workgroup reads one counter and leaves.
// The launch also DEALS the items for the eval kernel: with 2 048 of its workgroups resident and 5 800 (C4) to 52 000 (the knot) items of
// very different weight, the eval launch ends with whatever heavy items come last (taking the places backwards: C4 -3 us, knot +8 --
// profiles/r05ag_eval_order_ab.txt).  Every item has its pair count when this launch starts, so a lane per work place copies the place's
// record into one of S2_CLASSES lists by that count -- one atomic per wavefront and class -- and the eval kernel walks the lists from the
// heaviest class down: longest processing time first.
constexpr int S2_ROUNDS_GRID = 4096;
template <typename T, bool LEAN>
__global__ __launch_bounds__(64) void soft_select_rounds_kernel(Select2Args<T> a) {
  KAMD_S2_TABLES;
  const int lane = threadIdx.x;
  if (a.ord_list != nullptr) {
    // (S2_DEAL places per lane and step: one returning atomic per wavefront, class and 64 * S2_DEAL places -- with one place per lane the
    // knot's 52 000 items queued 3 300 atomics on the counters' line: 100 us)
    constexpr int S2_DEAL = 4;
    const WorkCounts wc = work_counts(a.work, a.shard_cap);
    for (unsigned int w0 = blockIdx.x * (64u * S2_DEAL); w0 < wc.places; w0 += gridDim.x * (64u * S2_DEAL)) {
      uint4 r[S2_DEAL];
      int c[S2_DEAL];
#pragma unroll
      for (int i = 0; i < S2_DEAL; ++i) {
        const unsigned int w = w0 + (unsigned int)(i * 64 + lane);
        r[i] = make_uint4(0u, 0u, 0u, 0u);
        c[i] = -1;  // no item
        if (w < wc.places && work_place_holds(wc, w)) {
          r[i] = *work_place(a.work, a.shard_cap, w);
          if (r[i].w != S2_HANDED_OVER) c[i] = s2_class_of(r[i].w);
        }
      }
#pragma unroll
      for (int cls = 0; cls < S2_CLASSES; ++cls) {
        unsigned long long m[S2_DEAL];
        int total = 0;
#pragma unroll
        for (int i = 0; i < S2_DEAL; ++i) {
          m[i] = __ballot(c[i] == cls);
          total += __popcll(m[i]);
        }
        if (total == 0) continue;  // (uniform)
        unsigned int base = 0u;
        if (lane == 0) base = atomicAdd(a.ord_count + cls * tl::COUNTER_STRIDE, (unsigned int)total);
        base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
#pragma unroll
        for (int i = 0; i < S2_DEAL; ++i) {
          const unsigned int pos = base + (unsigned int)__popcll(m[i] & ((1ull << lane) - 1ull));
          if (c[i] == cls && pos < a.ord_cap) a.ord_list[(size_t)cls * a.ord_cap + pos] = r[i];
          base += (unsigned int)__popcll(m[i]);
        }
      }
    }
  }
  const unsigned int n = *a.over_count;
  for (unsigned int i = blockIdx.x; i < n; i += gridDim.x) {
    const unsigned int wi_ = a.over_list[i];
    s2_select_item<T, LEAN, true>(a, t, *work_place(a.work, a.shard_cap, wi_), wi_);
  }
}
#undef KAMD_S2_TABLES

template <typename T>
struct Eval2Args {
  int B, F, H, W, K;
  float sigmainv, multiplier;
  double inv_mult2;          // 1 / multiplier^2 (soft_pair_prob)
  const T* rec;
  int tiles_x_s;
  const unsigned int* work;
  unsigned int shard_cap;
  const unsigned short* pixcnt;
  T* soft_mask;
  HitList2<T> list;          // compact form: pair / item_count are read, prob / type written
  T* prob_out;               // K-buffer form: idx is read, prob / type written
  const int64_t* idx_out;
  uint8_t* type_out;
  T* prob_pm;                // pixel-major copy of the probabilities when knum > S2_LDS_KMAX (folded by soft_fold_kernel)
  uint4* zero_p;             // fused dibr_rasterization: the backward's gradient buffer, cleared here (zero_n16 16-byte chunks):
  size_t zero_n16;           // off the critical path, where the forward's first fill launch would hold up the binning
  const unsigned int* span_src;  // fused dibr_rasterization: the covered-row spans (tl::Lists::row_span, workspace; nullptr: none) are
  unsigned int* span_dst;        // copied next to the worklist, which outlives the workspace: the backward's tile kernel starts
  int span_n;                    // from the same rows
  unsigned int* magic_dst;       // fused dibr_rasterization: where the layout signature goes (tl::WORK_MAGIC_WORD; nullptr: none)
  unsigned int magic;
  const unsigned int* ord_count; // the items dealt by pair count (soft_select_rounds_kernel): S2_CLASSES counts, tl::COUNTER_STRIDE words apart,
  const uint4* ord_list;         // and lists of ord_cap records each
  unsigned int ord_cap;
};

// probability of one (pixel, face) pair and which of the six distances gave it
// the part of a face's soft record a (pixel, face) probability needs: the six image coordinates and the three edges'
// reciprocals; loading it is split from the arithmetic so that callers can fetch a round ahead
template <typename T>
struct SoftFace {
  T v[6];
  double rcp[3];
};
template <typename T>
__device__ __forceinline__ SoftFace<T> soft_face_load(const T* __restrict__ body) {  // (tl::soft_body of the face)
  const Rec4<T> q1 = reinterpret_cast<const Rec4<T>*>(body)[0], q2 = reinterpret_cast<const Rec4<T>*>(body)[1];
  const double* rc = reinterpret_cast<const double*>(body + 8);
  return SoftFace<T>{{q1.a, q1.b, q1.c, q1.d, q2.a, q2.b}, {rc[0], rc[1], rc[2]}};
}
// `inv_mult2` = 1 / multiplier^2 as a double.  The reference's exponent is sigmainv * d2 / multiplier / multiplier
// (dibr_soft_mask_cuda.cu:161): two IEEE divisions by a launch constant, ~20 instructions of a kernel whose time is its vector
// instructions.  The probability is compared at 1e-5, not bit for bit (exp() itself differs between libraries), so the
// quotient is ONE double product rounded to T -- within one ulp of the twice-rounded reference value.  Everything that
// decides an INTEGER output (the six distances and their first minimum, closest_of_six) keeps the reference's arithmetic.
template <typename T>
__device__ __forceinline__ T soft_pair_prob(const SoftFace<T>& sf, T xu, T yu, float sigmainv, float multiplier, double inv_mult2, int* which) {
  EdgeInv<T> e[3];
  double den[3];
#pragma unroll
  for (int q = 0; q < 3; ++q)
    edge_coeffs<T>(sf.v[q * 2], sf.v[q * 2 + 1], sf.v[((q + 1) % 3) * 2], sf.v[((q + 1) % 3) * 2 + 1], &e[q], &den[q]);
  const T d2 = closest_of_six<T>(sf.v, e, den, sf.rcp, xu, yu, multiplier, which);
  const T zz = (T)((double)(T)(sigmainv * d2) * inv_mult2);
  return dibr_exp<T>(-zz);
}
template <typename T>
__device__ __forceinline__ T soft_pair_prob(const T* __restrict__ frec, T xu, T yu, float sigmainv, float multiplier, double inv_mult2, int* which) {
  return soft_pair_prob<T>(soft_face_load<T>(frec), xu, yu, sigmainv, multiplier, inv_mult2, which);
}

template <typename T, bool LEAN, bool LDS_FOLD>
#if KAMD_EVAL_WAVES > 0
__global__ __launch_bounds__(S2_EVAL_THREADS, (sizeof(T) == 4 ? KAMD_EVAL_WAVES : 4)) void soft_eval_kernel(Eval2Args<T> a) {
#else
__global__ __launch_bounds__(S2_EVAL_THREADS) void soft_eval_kernel(Eval2Args<T> a) {
#endif
  constexpr int RSB = tl::rec_s_body_scalars((int)sizeof(T));
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  T* s_prP = reinterpret_cast<T*>(s_dyn);  // [64 * K] pixel-major probabilities of the item (LDS_FOLD)
  __shared__ unsigned int s_flat_base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (size_t i = (size_t)blockIdx.x * S2_EVAL_THREADS + tid; i < a.zero_n16; i += (size_t)gridDim.x * S2_EVAL_THREADS)
    a.zero_p[i] = make_uint4(0u, 0u, 0u, 0u);
  if (blockIdx.x == 0 && a.span_dst != nullptr)
    for (int i = tid; i < a.span_n; i += S2_EVAL_THREADS) a.span_dst[i] = a.span_src != nullptr ? a.span_src[i] : 0u;
  if (blockIdx.x == 0 && tid == 0 && a.magic_dst != nullptr) *a.magic_dst = a.magic;
  // the items as soft_select_rounds_kernel dealt them: S2_CLASSES lists by pair count, walked from the heaviest class down
  static_assert(S2_CLASSES == 4, "four class counts");
  const unsigned int e0 = min(a.ord_count[0], a.ord_cap), e1 = e0 + min(a.ord_count[tl::COUNTER_STRIDE], a.ord_cap),
                     e2 = e1 + min(a.ord_count[2 * tl::COUNTER_STRIDE], a.ord_cap), e3 = e2 + min(a.ord_count[3 * tl::COUNTER_STRIDE], a.ord_cap);
  const int K = a.K;
  for (unsigned int g = blockIdx.x; g < e3; g += gridDim.x) {
    const unsigned int c = (g >= e0 ? 1u : 0u) + (g >= e1 ? 1u : 0u) + (g >= e2 ? 1u : 0u);
    const unsigned int pos = g - (c == 0u ? 0u : (c == 1u ? e0 : (c == 2u ? e1 : e2)));
    const uint4 wrec = a.ord_list[(size_t)c * a.ord_cap + pos];
    const ItemGeom ig = item_geom(wrec, a.B, a.tiles_x_s);
    // the pixels' hit counts are needed by the fold at the very end: requested now, they arrive behind everything else
    int my_hits = 0;
    if (LDS_FOLD && wave == 0) my_hits = (int)a.pixcnt[(size_t)ig.item * 64 + lane];
    const size_t seg_base = (size_t)ig.item * 64 * (size_t)K;
    const T* mesh_rec = tl::soft_body<T>(a.rec, (size_t)a.B * a.F, (size_t)ig.b * a.F);  // bodies of this mesh's faces
    __syncthreads();  // the previous item's fold is done with s_prP (and every thread has read s_flat_base)
    if (LEAN) {
      const int n = (int)wrec.w;  // (the select kernel left the item's pair count in its record: a.list.item_count[ig.item])
      // the item's range in the flat list: one returning atomic per item, issued before the loads it can hide behind
      unsigned int my_base = 0u;
      const unsigned int shard = (unsigned int)ig.item % (unsigned int)FLAT_SHARDS;
      if (tid == 0 && n > 0) my_base = atomicAdd(a.list.flat_count + shard * tl::COUNTER_STRIDE, (unsigned int)n);
      size_t base = 0;
      const unsigned int key0 = (unsigned int)ig.b * (unsigned int)a.F;
      // (Measured and dropped: the load pipeline of the backward kernel here -- pair records two rounds ahead,
      // face records one -- needs 80 instead of 32 VGPRs, occupancy 6 instead of 8: 55.8 vs 50.6 us; the pair record alone a
      // round ahead: no change, 50.5 us.)
      for (int t0 = 0; t0 < n; t0 += S2_EVAL_THREADS) {  // (uniform per workgroup)
        const int t = t0 + tid;
        const bool on = t < n;
        T pr = 0;
        int which = 0;
        int2 pr_ = make_int2(0, 0);
        if (on) {
          pr_ = s2_load_pair(a.list.pair + seg_base + t, KAMD_SOFT_NT >= 2);
          const SoftFace<T> sf = soft_face_load<T>(mesh_rec + (size_t)pr_.x * RSB);
          const int u = pr_.y >> 16;
          pr = soft_pair_prob<T>(sf, pixel_x(a.multiplier, a.W, ig.sub_x + (u & 15)), pixel_y(a.multiplier, a.H, ig.sub_y + (u >> 4)),
                                 a.sigmainv, a.multiplier, a.inv_mult2, &which);
        }
        if (t0 == 0) {
          if (tid == 0) s_flat_base = my_base;
          __syncthreads();
          base = (size_t)shard * a.list.shard_cap + s_flat_base;
        }
        if (on) {
          const int u = pr_.y >> 16, slot = pr_.y & 0xFFFF;
          const unsigned int ucol = (unsigned int)(ig.sub_x + (u & 15)), urow = (unsigned int)(ig.sub_y + (u >> 4));
          const uint2 rec = make_uint2((key0 + (unsigned int)pr_.x) | ((unsigned int)which << FLAT_KEY_BITS), (urow << 16) | ucol);
          if (KAMD_SOFT_NT >= 1) {
            __builtin_nontemporal_store(pr, a.list.prob + base + t);
            s2_u32x2 rv;
            rv.x = rec.x;
            rv.y = rec.y;
            __builtin_nontemporal_store(rv, reinterpret_cast<s2_u32x2*>(a.list.rec + base + t));
          } else {
            a.list.prob[base + t] = pr;
            a.list.rec[base + t] = rec;
          }
          if (LDS_FOLD)
            s_prP[u * K + slot] = pr;
          else
            a.prob_pm[seg_base + (size_t)u * K + slot] = pr;
        }
      }
    } else {
      // K-buffer form: the select kernel stored the accepted faces in close_face_idx; walk the item's (pixel, slot) grid
      for (int q = tid; q < 64 * K; q += S2_EVAL_THREADS) {
        const int u = q / K, slot = q - u * K;
        if (slot >= (int)a.pixcnt[(size_t)ig.item * 64 + u]) continue;
        const int ucol = ig.sub_x + (u & 15), urow = ig.sub_y + (u >> 4);
        const size_t o = (((size_t)ig.b * a.H + urow) * a.W + ucol) * K + slot;
        const int fid = (int)a.idx_out[o];
        int which;
        const T pr = soft_pair_prob<T>(mesh_rec + (size_t)fid * RSB, pixel_x(a.multiplier, a.W, ucol),
                                       pixel_y(a.multiplier, a.H, urow), a.sigmainv, a.multiplier, a.inv_mult2, &which);
        a.prob_out[o] = pr;
        a.type_out[o] = (uint8_t)(which + 1);
        if (LDS_FOLD) s_prP[q] = pr;
      }
    }
    if (LDS_FOLD) {
      __syncthreads();
      if (wave == 0 && ((ig.unc >> lane) & 1ull) != 0ull) {
        // prod(1 - prob) in hit order (dibr_soft_mask_cuda.cu:174-179)
        const int n = my_hits;
        T all = 1.0;
        for (int j = 0; j < n; ++j) all = (T)((double)all * (1.0 - (double)s_prP[lane * K + j]));
        const int col = ig.sub_x + (lane & 15), row = ig.sub_y + (lane >> 4);
        a.soft_mask[((size_t)ig.b * a.H + row) * a.W + col] = (T)(1.0 - (double)all);
      }
    }
  }
}

// knum > S2_LDS_KMAX: the products are folded from memory by a second launch (one wavefront per item)
template <typename T, bool LEAN>
__global__ __launch_bounds__(64) void soft_fold_kernel(Eval2Args<T> a) {
  const int lane = threadIdx.x;
  const WorkView wv = work_view(a.work, a.shard_cap);
  const unsigned int n_work = work_total(wv);
  const int K = a.K;
  for (unsigned int wi_ = blockIdx.x; wi_ < n_work; wi_ += gridDim.x) {
    uint4 wrec;
    if (!work_fetch(wv, wi_, &wrec)) break;
    const ItemGeom ig = item_geom(wrec, a.B, a.tiles_x_s);
    if (((ig.unc >> lane) & 1ull) == 0ull) continue;
    const int col = ig.sub_x + (lane & 15), row = ig.sub_y + (lane >> 4);
    const size_t p1 = ((size_t)ig.b * a.H + row) * a.W + col;
    const T* src = LEAN ? a.prob_pm + (size_t)ig.item * 64 * (size_t)K + (size_t)lane * K : a.prob_out + p1 * K;
    const int n = (int)a.pixcnt[(size_t)ig.item * 64 + lane];
    T all = 1.0;
    for (int j = 0; j < n; ++j) all = (T)((double)all * (1.0 - (double)src[j]));
    a.soft_mask[p1] = (T)(1.0 - (double)all);
  }
}

// orders a wavefront's own LDS traffic (writes by some lanes, reads by others) without a workgroup barrier
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- K4, flat-list form --------------------------------------------------------------------------------------------------
// One lane per recorded hit, rounds of 256 consecutive records of the flat list dealt round-robin to persistent workgroups:
// every load of the list is a coalesced stream, every workgroup gets the same number of hits (the segmented form walked
// ITEMS: 1.4 items per workgroup, each a chain of five dependent round trips for three or four rounds of arithmetic).
// The eval kernel wrote an item's hits face-major, so the hits of a face sit in consecutive lanes: their six
// vertex-coordinate contributions are summed inside rows of 16 lanes with DPP row shifts (register moves) and only the
// last lane of a run issues global atomics -- no LDS table, no hash probes, ~6x fewer memory atomics than one per hit.
//
// The kernel is VALU-bound (33.7 M vector instructions for the 5.1 M hits of C4 in round 3: the issue time of the chip's 1 024
// SIMDs, 55 of its 59 us), so round 4 cut instructions, not waits.  The reference divides every contribution by `multiplier`
// and forms dLdz and the edge case's 1 / (down + EPS) with IEEE double divisions (dibr_soft_mask_cuda.cu:283-347): two
// ~30-instruction double divisions and up to four ~10-instruction float divisions per hit.  Gradients are compared at 1e-5,
// not bit for bit, so
//   * the two double quotients are products with rcp64(): v_rcp_f64 + two Newton steps (four fmas) -- within 2 ulp of the
//     correctly rounded DOUBLE reciprocal; rounded to float afterwards the result is the reference's except in ~1e-8 of the
//     cases, and then by one float ulp;
//   * 1 / multiplier is folded into dLdz while it is still a double (one more product before the rounding to T): every
//     contribution is then dLdz_m * (geometry) -- one rounding where the reference has two;
//   * the view b = key / F is an exact integer division by multiplication (one mul_hi + one correction; the float estimate it
//     replaces was only provably right for B < 2^22: ADVICE r03).
__device__ __forceinline__ double rcp64(double x) {
  const double r0 = __builtin_amdgcn_rcp(x);
  double r = __builtin_fma(__builtin_fma(-x, r0, 1.0), r0, r0);
  r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
  // x = +-inf (a `down` that overflowed, vertices at infinity): 1 / x is +-0, but the Newton step forms inf * 0 = NaN -- keep the
  // hardware's own answer wherever the refined one is not a number (also x = 0 and NaN: +-inf and NaN, as the division gives)
  return r == r ? r : r0;
}
// key / F for key < 2^29: q' = mulhi(key, ceil(2^32 / F)) is floor(key / F) or one more (F >= 2; the host passes 0 for F == 1)
__device__ __forceinline__ int flat_view_of(unsigned int key, unsigned int F, unsigned int f_magic, int* rem) {
  if (f_magic == 0u) {
    *rem = 0;
    return (int)key;
  }
  unsigned int q = __umulhi(key, f_magic);
  int r = (int)(key - q * F);
  if (r < 0) {
    --q;
    r += (int)F;
  }
  *rem = r;
  return (int)q;
}
inline unsigned int flat_view_magic(int F) { return F <= 1 ? 0u : (unsigned int)((0x100000000ull + (unsigned long long)F - 1ull) / (unsigned long long)F); }

// SW ("scaled weights", weighted_sum's backward fused in): `grad` holds the loss weights W and the incoming gradient of pixel p is
// *grad_scale * W[p] -- the product weighted_sum2_backward_kernel would have stored, formed at the hits' pixels only.
template <typename T, bool SW>
__global__ __launch_bounds__(256) void soft_mask_backward_flat_kernel(
    int H, int W, int F, unsigned int f_magic, const T* __restrict__ grad, const T* __restrict__ soft_mask, HitList2<T> list,
    const T* __restrict__ img, T img_scale, float sigmainv, float multiplier, double inv_multiplier, T* __restrict__ g_img,
    unsigned int* __restrict__ bigwork /* work + tl::WORK_BIGHASH_WORD of the fused operator's work buffer, or nullptr */,
    const T* __restrict__ grad_scale /* SW only */) {
  __shared__ int s_runf[4][64];
  __shared__ T s_runv[4][64 * 6];
  // the hot faces' terms go to this XCD's copy of their records (tile_lists.h, WORK_BIGHASH_WORD); uniform, fp32 only
  __shared__ unsigned int s_bigbits[tl::BIG_HASH_SLOTS / 32];  // which slots of the hot faces' table are taken
  const bool use_side = sizeof(T) == 4 && bigwork != nullptr && tl::big_hash_usable(bigwork[0]);
  if (use_side && threadIdx.x < tl::BIG_HASH_SLOTS / 32) s_bigbits[threadIdx.x] = bigwork[tl::BIG_HASH_BITS_OFF + threadIdx.x];  // (read after the barrier below)
  const int lane = threadIdx.x & 63, rl = lane & 15, wave = threadIdx.x >> 6;
  // rounds of 256 records, shard after shard: s_end[s] = rounds of the shards 0..s
  __shared__ unsigned int s_end[FLAT_SHARDS];
  __shared__ unsigned int s_cnt[FLAT_SHARDS];
  if (threadIdx.x < 64) {
    static_assert(FLAT_SHARDS == 64, "one wavefront scans the shard counts");
    const unsigned int c = min(list.flat_count[threadIdx.x * tl::COUNTER_STRIDE], (unsigned int)list.shard_cap);
    s_cnt[threadIdx.x] = c;
    s_end[threadIdx.x] = (unsigned int)wave_inclusive_scan((int)((c + 255u) >> 8));
  }
  __syncthreads();
  const unsigned int rounds = s_end[FLAT_SHARDS - 1];
  const double neg_sigma = -1.0 * (double)sigmainv;
  const T gs = SW ? *grad_scale : (T)1;  // (uniform: a scalar load)
  // Software pipeline over the rounds: a hit's gathers (gradient, mask, the face's vertices) depend on its record, and the
  // arithmetic on the gathers -- two memory round trips per round.  Records are loaded two rounds ahead (stage A), gathers
  // one round ahead (stage B), and the arithmetic of a round runs with both in flight.
  struct StageA {
    uint2 rec;
    T pr;
  };
  struct StageB {
    int key, e;
    unsigned int rc;
    T pr, dLdp, all, x1, y1, x2, y2;
  };
  unsigned int a_shard = 0u;  // (global rounds are asked for in ascending order: the shard pointer only moves forward; uniform)
  auto load_a = [&](unsigned int r) {
    StageA a{make_uint2(0xFFFFFFFFu, 0u), (T)0};
    if (r < rounds) {
      while (r >= s_end[a_shard]) ++a_shard;
      const unsigned int r_in = r - (a_shard > 0u ? s_end[a_shard - 1u] : 0u);
      const unsigned int i = r_in * 256u + threadIdx.x;
      if (i < s_cnt[a_shard]) {
        const size_t t = (size_t)a_shard * list.shard_cap + i;
        if (KAMD_SOFT_NT >= 1) {
          const s2_u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const s2_u32x2*>(list.rec + t));
          a.rec = make_uint2(v.x, v.y);
          a.pr = __builtin_nontemporal_load(list.prob + t);
        } else {
          a.rec = list.rec[t];
          a.pr = list.prob[t];
        }
      }
    }
    return a;
  };
  auto load_b = [&](const StageA& a) {
    StageB v{-1, 0, 0u, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0};
    if (a.rec.x != 0xFFFFFFFFu) {
      v.key = (int)(a.rec.x & FLAT_KEY_MASK);
      v.e = (int)(a.rec.x >> FLAT_KEY_BITS);
      v.rc = a.rec.y;
      v.pr = a.pr;
      int rem;
      const int b = flat_view_of((unsigned int)v.key, (unsigned int)F, f_magic, &rem);
      const size_t pix = ((size_t)b * H + (a.rec.y >> 16)) * W + (a.rec.y & 0xFFFFu);
      v.dLdp = SW ? gs * grad[pix] : grad[pix];
      v.all = soft_mask[pix];
      const size_t s6 = (size_t)v.key * 6;
      const int o = v.e >= 3 ? (v.e - 3) * 2 : v.e * 2;
      v.x1 = img[s6 + o];
      v.y1 = img[s6 + o + 1];
      if (v.e < 3) {
        const int o2 = v.e == 2 ? 0 : o + 2;
        v.x2 = img[s6 + o2];
        v.y2 = img[s6 + o2 + 1];
      }
    }
    return v;
  };
  const unsigned int G = gridDim.x;
  StageA sa = load_a(blockIdx.x);
  StageB sb = load_b(sa);
  sa = load_a(blockIdx.x + G);
  for (unsigned int r = blockIdx.x; r < rounds; r += G) {  // (uniform per workgroup)
    const StageB cur = sb;
    if (r + G < rounds) sb = load_b(sa);
    if (r + 2u * G < rounds) sa = load_a(r + 2u * G);
    int f = cur.key;
    T vals[6] = {0, 0, 0, 0, 0, 0};
    if (f >= 0) {
      const int e = cur.e;
      const T x0 = pixel_x(multiplier, W, (int)(cur.rc & 0xFFFFu));
      const T y0 = pixel_y(multiplier, H, (int)(cur.rc >> 16));
      // dLdz = -sigmainv * dLdp * (1 - mask) / (1 - prob + EPS) * prob, in double as the reference (dibr_soft_mask_cuda.cu:283-284),
      // the quotient as a product with rcp64, and 1 / multiplier -- which the reference applies to every contribution
      // (:299-302,339-347) -- folded in before the rounding to T
      const double dz = neg_sigma * (double)cur.dLdp * (1.0 - (double)cur.all) * rcp64(1.0 - (double)cur.pr + DIBR_EPS) * (double)cur.pr;
      const T dLdz = (T)(dz * inv_multiplier);
      const int o = e >= 3 ? (e - 3) * 2 : e * 2;
      int o2 = -2;
      T c0, c1, c2 = 0, c3 = 0;
      const T x1 = cur.x1 * img_scale, y1 = cur.y1 * img_scale;
      if (e >= 3) {
        c0 = dLdz * 2 * (x1 - x0);
        c1 = dLdz * 2 * (y1 - y0);
      } else {
        o2 = e == 2 ? 0 : o + 2;
        const T x2 = cur.x2 * img_scale, y2 = cur.y2 * img_scale;
        const T A = y2 - y1, Bc = x1 - x2, C = x2 * y1 - x1 * y2;
        const T up = A * x0 + Bc * y0 + C;
        const T down = A * A + Bc * Bc;
        // the reference divides four times by the double (down + EPS) (dibr_soft_mask_cuda.cu:318-327): one reciprocal,
        // four double products, each rounded to T as the quotients are
        const double rden = rcp64((double)down + DIBR_EPS);
        const T d2 = (T)((double)(T)(up * up) * rden);
        const T dzdA = (T)((double)(T)(2 * (x0 * up - d2 * A)) * rden);
        const T dzdB = (T)((double)(T)(2 * (y0 * up - d2 * Bc)) * rden);
        const T dzdC = (T)((double)(T)(2 * up) * rden);
        c0 = dLdz * (dzdB - y2 * dzdC);
        c1 = dLdz * (x2 * dzdC - dzdA);
        c2 = dLdz * (y1 * dzdC - dzdB);
        c3 = dLdz * (dzdA - x1 * dzdC);
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) vals[i] = i == o ? c0 : (i == o + 1 ? c1 : (i == o2 ? c2 : (i == o2 + 1 ? c3 : (T)0)));
    }
    // runs of equal f (= b * F + face) inside a row of 16 lanes: segmented inclusive sum, the last lane of a run holds its total
    const int prev_f = row_shr<1>(f);
    const int next_f = row_shl<1>(f);
    const bool run_start = rl == 0 || prev_f != f;
    int start_lane = run_start ? rl : 0;
    {
      int o;
      o = row_shr<1>(start_lane); if (rl >= 1) start_lane = max(start_lane, o);
      o = row_shr<2>(start_lane); if (rl >= 2) start_lane = max(start_lane, o);
      o = row_shr<4>(start_lane); if (rl >= 4) start_lane = max(start_lane, o);
      o = row_shr<8>(start_lane); if (rl >= 8) start_lane = max(start_lane, o);
    }
#define KAMD_SB_STAGE(DD)                                        \
    {                                                          \
      const bool take = rl >= DD && start_lane <= rl - DD;     \
      _Pragma("unroll") for (int i = 0; i < 6; ++i) {          \
        const T o = row_shr<DD>(vals[i]);                      \
        if (take) vals[i] += o;                                \
      }                                                        \
    }
    KAMD_SB_STAGE(1)
    KAMD_SB_STAGE(2)
    KAMD_SB_STAGE(4)
    KAMD_SB_STAGE(8)
#undef KAMD_SB_STAGE
    const bool run_end = f >= 0 && (rl == 15 || next_f != f);
    // The run totals leave through LDS so that ONE atomic instruction carries all six coordinates of a face in six
    // consecutive lanes: 24 contiguous bytes = one L2 atomic request per face instead of six (issued coordinate by
    // coordinate, every instruction touched a different cache line per lane: measured 55 us of the first version's 130).
    const unsigned long long ends = __ballot(run_end);
    const int n_ends = __popcll(ends);
    // (every wavefront owns its staging rows: wavefront-level ordering is all that is needed, n_ends differs per wave)
    wave_lds_sync();
    if (run_end) {
      const int q = __popcll(ends & ((1ull << lane) - 1ull));
      s_runf[wave][q] = f;
#pragma unroll
      for (int i = 0; i < 6; ++i) s_runv[wave][q * 6 + i] = vals[i];
    }
    wave_lds_sync();
    // A run split by a 16-lane row boundary leaves up to four consecutive pieces of the same face: the last piece
    // collects the others (reads only: no write hazards), the others stay silent.
    if (!use_side) {
      for (int j = lane; j < n_ends * 6; j += 64) {
        const int q = j / 6, c = j - q * 6;
        const int fr = s_runf[wave][q];
        if (q + 1 < n_ends && s_runf[wave][q + 1] == fr) continue;
        T v = s_runv[wave][j];
        for (int k = 1; k <= 3 && q - k >= 0 && s_runf[wave][q - k] == fr; ++k) v += s_runv[wave][(q - k) * 6 + c];
        if (v != (T)0) kamd_atomic_add(g_img + (size_t)fr * 6 + c, v);
      }
    } else {
      // The same loop with the hot faces' look-up (tile_lists.h, WORK_BIGHASH_WORD).  A hot face reaches most pixels of an item: its
      // run crosses a 16-lane row.  Only such runs are looked up (a probe per run end: shuffled knot +10 us), first in the table's
      // occupancy bits (LDS), then in the table; a hot face's total goes to the record of this workgroup's XCD.  (Whatever the form
      // of this branch -- in the loop above, a copy as here, out of line, its operands fetched late -- the launch WITHOUT hot faces,
      // C4's, takes 49.7 instead of 47.3 us, and 47.3 again when the branch is compiled out: profiles/r06zv_*.)
      T* const side = reinterpret_cast<T*>(bigwork + (tl::WORK_BIGSIDE_WORD - tl::WORK_BIGHASH_WORD)) +
                      (size_t)(blockIdx.x & (tl::BIG_SIDE_COPIES - 1)) * tl::BIG_HASH_SLOTS * 8;
      for (int j = lane; j < n_ends * 6; j += 64) {
        const int q = j / 6, c = j - q * 6;
        const int fr = s_runf[wave][q];
        if (q + 1 < n_ends && s_runf[wave][q + 1] == fr) continue;
        T v = s_runv[wave][j];
        int k = 1;  // (ends as the number of pieces)
        for (; k <= 3 && q - k >= 0 && s_runf[wave][q - k] == fr; ++k) v += s_runv[wave][(q - k) * 6 + c];
        if (v != (T)0) {
          T* dst = g_img + (size_t)fr * 6 + c;
          if (k > 1) {
            const unsigned int h = tl::big_hash_of((unsigned int)fr);
            if ((s_bigbits[h >> 5] >> (h & 31u)) & 1u) {  // (a key's home slot is taken whenever the key is in the table)
              const int slot = tl::big_hash_find(bigwork, (unsigned int)fr);
              if (slot >= 0) dst = side + (size_t)slot * 8 + c;
            }
          }
          kamd_atomic_add(dst, v);
        }
      }
    }
  }
}
