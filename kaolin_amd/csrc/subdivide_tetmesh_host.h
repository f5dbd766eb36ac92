// Host arithmetic of ops.mesh.subdivide_tetmesh (csrc/subdivide_tetmesh.hip): which extents the pipeline takes, how many radix
// passes a vertex count needs, and the layout of the topology workspace.  Plain C++ without a HIP include, so that a host-only
// program can run it under a sanitizer (tools/check_subdivide_tetmesh_host.cpp); every count that can reach 6 T is 64 bits wide.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sort_scan_host.h"

// V < 2^32: an id is one half of a 64-bit key.  T <= 2^35: 6 T keys in workgroups of 256 stay below 2^31 workgroups.
inline bool st_bad_extents(long long T, long long V) { return T < 0 || V < 0 || V >= (1ll << 32) || T > (1ll << 35); }

// the bits of a vertex id: the digits of either key half above them are zero in every key
inline int st_id_bits(long long V) {
  int nb = 1;
  while (nb < 32 && (1ll << nb) < V) ++nb;
  return nb;
}
// 8-bit passes over one half of the keys; the sort runs this many over the max half, then as many over the min half
// (ss_passes_halves)
inline int st_passes_per_half(long long V) { return ss_passes(st_id_bits(V)); }

inline size_t st_align(size_t x) { return (x + 15) & ~(size_t)15; }

// keys_a: the 6 T keys, sorted in place (through keys_b); keys_b: after the sort, the unique keys.  flags / pos: heads of the
// runs of equal keys and their exclusive scan (pos[n] = E).  hist / hoffs / sums: the sort's (digit, block) counts and the scans'
// block sums.
struct StLayout {
  long long n, nsb;  // keys, sort blocks
  size_t keys_a, keys_b, flags, pos, hist, hoffs, sums, bytes;
};
inline StLayout st_layout(long long T) {
  StLayout l;
  l.n = 6 * T;
  l.nsb = ss_sort_blocks(l.n);
  size_t o = 0;
  l.keys_a = o, o += st_align((size_t)l.n * 8);
  l.keys_b = o, o += st_align((size_t)l.n * 8);
  l.flags = o, o += st_align((size_t)l.n * 4);
  l.pos = o, o += st_align(((size_t)l.n + 1) * 8);
  l.hist = o, o += st_align(ss_sort_hist_entries(l.n) * 4);
  l.hoffs = o, o += st_align(ss_sort_offs_entries(l.n) * 8);
  l.sums = o, o += st_align(ss_sort_unique_sums_entries(l.n) * 8);
  l.bytes = o;
  return l;
}
inline size_t st_workspace_bytes(long long T, long long V) {
  if (T <= 0 || V <= 0 || st_bad_extents(T, V)) return 0;
  return st_layout(T).bytes;
}
