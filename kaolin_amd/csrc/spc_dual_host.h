// Host arithmetic of ops.spc.unbatched_make_dual / unbatched_make_trinkets (csrc/spc_trilinear.hip): the key layout, the radix
// passes a depth needs, the level offsets that travel as kernel arguments and the layout of the workspace.  Plain C++ without a
// HIP include, so that a host-only program can run it under a sanitizer (tools/check_spc_dual_host.cpp); every count that can
// reach 8 * num_points is 64 bits wide.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sort_scan_host.h"

constexpr int SD_MAX_LEVEL = 14;          // a corner of level l reaches 2^l: l + 1 bits per axis, 15 at most (int16, 45-bit codes)
constexpr int SD_LEVEL_SHIFT = 48;        // key = level << 48 | Morton code of the corner
constexpr int SD_SIZES_WORDS = 32;        // the words read back: SD_MAX_LEVEL + 2 level starts, padded

inline size_t sd_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// 8 n keys in workgroups of 256 stay below 2^31 workgroups
inline bool sd_bad_extents(long long n, int max_level) {
  return n < 1 || n > (1ll << 35) || max_level < 0 || max_level > SD_MAX_LEVEL;
}

inline int sd_code_bits(int max_level) { return 3 * (max_level + 1); }
// 8-bit LSD passes over the code bits, then ONE pass at SD_LEVEL_SHIFT over the level (4 bits) -- none for a lone root level
inline int sd_code_passes(int max_level) { return ss_passes(sd_code_bits(max_level)); }
inline int sd_level_passes(int max_level) { return max_level > 0 ? 1 : 0; }
// shift of pass k (k < sd_code_passes + sd_level_passes); the digits between the code bits and bit 48 are all zero
inline int sd_pass_shift(int max_level, int k) { return k < sd_code_passes(max_level) ? 8 * k : SD_LEVEL_SHIFT; }
inline SsPasses sd_passes(int max_level) {
  SsPasses p = {sd_code_passes(max_level) + sd_level_passes(max_level), {0}};
  for (int k = 0; k < p.count; ++k) p.shift[k] = sd_pass_shift(max_level, k);
  return p;
}

// first[l] = index of the first point of level l, first[max_level + 1] = the number of points, every later entry repeats it: the
// row pyramid[1] of a pyramid.  `ok` is false for a row that does not start at 0, decreases, or does not end at `n`.
struct SdLevels {
  long long first[SD_MAX_LEVEL + 2];
  int max_level;
};
inline bool sd_levels(const long long* pyramid_row1, int max_level, long long n, SdLevels* out) {
  if (max_level < 0 || max_level > SD_MAX_LEVEL) return false;
  out->max_level = max_level;
  bool ok = pyramid_row1[0] == 0 && pyramid_row1[max_level + 1] == n;
  for (int l = 0; l <= SD_MAX_LEVEL + 1; ++l) {
    out->first[l] = l <= max_level + 1 ? pyramid_row1[l] : pyramid_row1[max_level + 1];
    if (l > 0 && out->first[l] < out->first[l - 1]) ok = false;
  }
  return ok;
}

// sizes: the level starts of the dual, read back once.  keys_a / keys_b: the 8 n keys and the sort's other buffer.  flags / pos:
// heads of the runs of equal keys and their exclusive scan (pos[8 n] = dual points).  hist / hoffs / sums: the sort's (digit,
// block) counts, their offsets, and the scans' block sums.
struct SdLayout {
  long long keys, nsb;  // keys, sort blocks
  size_t sizes, keys_a, keys_b, flags, pos, hist, hoffs, sums, bytes;
};
inline SdLayout sd_layout(long long n) {
  SdLayout l;
  l.keys = 8 * n;
  l.nsb = ss_sort_blocks(l.keys);
  size_t o = 0;
  l.sizes = o, o += sd_align((size_t)SD_SIZES_WORDS * 8);
  l.keys_a = o, o += sd_align((size_t)l.keys * 8);
  l.keys_b = o, o += sd_align((size_t)l.keys * 8);
  l.flags = o, o += sd_align((size_t)l.keys * 4);
  l.pos = o, o += sd_align(((size_t)l.keys + 1) * 8);
  l.hist = o, o += sd_align(ss_sort_hist_entries(l.keys) * 4);
  l.hoffs = o, o += sd_align(ss_sort_offs_entries(l.keys) * 8);
  l.sums = o, o += sd_align(ss_sort_unique_sums_entries(l.keys) * 8);
  l.bytes = o;
  return l;
}
inline size_t sd_workspace_bytes(long long n, int max_level) {
  if (sd_bad_extents(n, max_level)) return 0;
  return sd_layout(n).bytes;
}
// which of the two key buffers holds the sorted keys: the build sorts keys_a into the one an odd number of passes leaves them in
inline bool sd_sorted_in_b(int max_level) { return (sd_passes(max_level).count & 1) != 0; }
