// Host arithmetic of the shared scan / radix sort (csrc/sort_scan.h): the block sizes, the pass shifts of a sort and the entries
// of its scratch.  Every workspace layout takes its sort and scan sizes from here.  Plain C++ without a HIP include, so that a
// host-only program can run it under a sanitizer (tools/check_sort_scan_host.cpp); every count is 64 bits wide.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int SS_SCAN_BLOCK = 1024;  // ints per workgroup of a scan
constexpr int SS_SORT_BLOCK = 2048;  // keys per workgroup of the radix sort
constexpr int SS_MAX_PASSES = 8;     // 8 bits a pass, 64-bit keys

inline long long ss_cdiv(long long a, long long b) { return (a + b - 1) / b; }

// block sums of a scan of n ints (one per workgroup, and room to spare: the largest of the formulas the layouts once had)
inline size_t ss_scan_sums_entries(long long n) { return (size_t)ss_cdiv(n > 0 ? n : 0, SS_SCAN_BLOCK) + 2; }

// the sort's scratch for n keys: (digit, block) counts (ints), their exclusive scan (+ 1, int64) and that scan's block sums (int64)
inline long long ss_sort_blocks(long long n) { return ss_cdiv(n > 0 ? n : 1, SS_SORT_BLOCK); }
inline size_t ss_sort_hist_entries(long long n) { return (size_t)256 * (size_t)ss_sort_blocks(n); }
inline size_t ss_sort_offs_entries(long long n) { return ss_sort_hist_entries(n) + 1; }
inline size_t ss_sort_sums_entries(long long n) { return ss_scan_sums_entries((long long)ss_sort_hist_entries(n)); }
// block sums that serve both the sort of n keys and a scan over the n keys themselves (the heads of their runs)
inline size_t ss_sort_unique_sums_entries(long long n) {
  const long long hn = (long long)ss_sort_hist_entries(n);
  return ss_scan_sums_entries(hn > n ? hn : n);
}

// the shifts of a sort's passes, least significant digit first
struct SsPasses {
  int count;
  int shift[SS_MAX_PASSES];
};
inline int ss_passes(int bits) { return (bits + 7) / 8; }
// the low `bits` bits of the key: 0, 8, ... < bits (none for bits == 0)
inline SsPasses ss_passes_low(int bits) {
  SsPasses p = {0, {0}};
  for (int s = 0; s < bits && p.count < SS_MAX_PASSES; s += 8) p.shift[p.count++] = s;
  return p;
}
// the low `bits` bits (<= 32) of either 32-bit half, the low half first: an even number of passes
inline SsPasses ss_passes_halves(int bits) {
  SsPasses p = {0, {0}};
  for (int half = 0; half < 2; ++half)
    for (int s = 0; s < bits && s < 32; s += 8) p.shift[p.count++] = 32 * half + s;
  return p;
}
