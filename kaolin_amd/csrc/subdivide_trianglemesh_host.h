// Host arithmetic of ops.mesh.subdivide_trianglemesh (csrc/subdivide_trianglemesh.hip): which extents the pipeline takes and
// the layout of the topology workspace (the radix passes a vertex count needs are subdivide_tetmesh_host.h's).  Plain C++
// without a HIP include, so that a host-only program can run it under a sanitizer
// (tools/check_subdivide_trianglemesh_host.cpp); every count that can reach 3 F is 64 bits wide.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "subdivide_tetmesh_host.h"  // st_id_bits, st_passes_per_half, st_align: the same keys, the same rules

// V < 2^32: an id is one half of a 64-bit key.  F <= 2^35: 3 F keys in workgroups of 256 stay below 2^31 workgroups.
inline bool sl_bad_extents(long long F, long long V) { return F < 0 || V < 0 || V >= (1ll << 32) || F > (1ll << 35); }

// keys_a: the 3 F keys min << 32 | max, sorted in place (through keys_b); after the host has read E, the E swapped keys
// max << 32 | min, sorted in place (through keys_c): the transposed edge list.  keys_b: after the first sort, the unique keys.
// keys_c: the second sort's other buffer (E <= 3 F keys).  flags / pos: heads of the runs of equal keys and their exclusive scan
// (pos[n] = E).  hist / hoffs / sums: the sorts' (digit, block) counts and the scans' block sums.
struct SlLayout {
  long long n, nsb;  // keys, sort blocks
  size_t keys_a, keys_b, keys_c, flags, pos, hist, hoffs, sums, bytes;
};
inline SlLayout sl_layout(long long F) {
  SlLayout l;
  l.n = 3 * F;
  l.nsb = ss_sort_blocks(l.n);
  size_t o = 0;
  l.keys_a = o, o += st_align((size_t)l.n * 8);
  l.keys_b = o, o += st_align((size_t)l.n * 8);
  l.keys_c = o, o += st_align((size_t)l.n * 8);
  l.flags = o, o += st_align((size_t)l.n * 4);
  l.pos = o, o += st_align(((size_t)l.n + 1) * 8);
  l.hist = o, o += st_align(ss_sort_hist_entries(l.n) * 4);
  l.hoffs = o, o += st_align(ss_sort_offs_entries(l.n) * 8);
  l.sums = o, o += st_align(ss_sort_unique_sums_entries(l.n) * 8);
  l.bytes = o;
  return l;
}
inline size_t sl_workspace_bytes(long long F, long long V) {
  if (F <= 0 || V <= 0 || sl_bad_extents(F, V)) return 0;
  return sl_layout(F).bytes;
}
