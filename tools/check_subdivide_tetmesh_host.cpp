// Host-side check of the arithmetic in kaolin_amd/csrc/subdivide_tetmesh_host.h (workspace layout, radix passes) at the extents
// where a 32-bit count would overflow.  Stand-alone, no GPU:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/check_subdivide_tetmesh_host.cpp -o /tmp/check_subdivide_tetmesh_host && /tmp/check_subdivide_tetmesh_host
// (with hipcc: -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined).  Prints one line per (T, V) and
// "host arithmetic OK"; exits non-zero on a failed expectation.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../kaolin_amd/csrc/subdivide_tetmesh_host.h"

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "line %d: expectation failed: %s\n", __LINE__, #cond); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

int main() {
  const long long Ts[] = {0, 1, (1ll << 31) / 6 + 1};
  const long long Vs[] = {1, 1ll << 16, (1ll << 32) - 1};
  const int bits[] = {1, 16, 32}, passes[] = {1, 2, 4};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      const long long T = Ts[i], V = Vs[j];
      EXPECT(!st_bad_extents(T, V));
      EXPECT(st_id_bits(V) == bits[j] && st_passes_per_half(V) == passes[j]);
      const size_t bytes = st_workspace_bytes(T, V);
      const StLayout l = st_layout(T);
      printf("T=%lld V=%lld: keys=%lld sort_blocks=%lld id_bits=%d passes=2x%d workspace=%zu bytes\n", T, V, l.n, l.nsb,
             st_id_bits(V), st_passes_per_half(V), bytes);
      if (T == 0) {
        EXPECT(bytes == 0);
        continue;
      }
      EXPECT(l.n == 6 * T && l.nsb == (l.n + SS_SORT_BLOCK - 1) / SS_SORT_BLOCK && bytes == l.bytes);
      // the buffers, in order, each 16-byte aligned and large enough, none overlapping the next
      const size_t off[] = {l.keys_a, l.keys_b, l.flags, l.pos, l.hist, l.hoffs, l.sums, l.bytes};
      const size_t need[] = {(size_t)l.n * 8, (size_t)l.n * 8, (size_t)l.n * 4, ((size_t)l.n + 1) * 8, (size_t)l.nsb * 256 * 4,
                             ((size_t)l.nsb * 256 + 1) * 8, 8};
      for (int k = 0; k < 7; ++k) EXPECT(off[k] % 16 == 0 && off[k + 1] >= off[k] + need[k]);
      EXPECT(bytes >= (size_t)l.n * 28);  // 8 + 8 + 4 + 8 bytes a key: more than 2^32 for the large T, no 32-bit wrap
      if (T == 1) {                       // the layout used as offsets into a real buffer
        std::vector<unsigned char> buffer(bytes, 0);
        for (int k = 0; k < 7; ++k) buffer[off[k]] = 1, buffer[off[k] + need[k] - 1] = 1;
      }
    }
  }
  EXPECT(st_bad_extents(-1, 1) && st_bad_extents(1, -1) && st_bad_extents(1, 1ll << 32) && st_bad_extents((1ll << 35) + 1, 1));
  EXPECT(st_workspace_bytes(5, 1ll << 32) == 0 && st_workspace_bytes(5, 0) == 0);
  EXPECT(st_id_bits((1ll << 16) + 1) == 17 && st_passes_per_half((1ll << 16) + 1) == 3 && st_passes_per_half(70001) == 3);
  EXPECT(st_passes_per_half(256) == 1 && st_passes_per_half(257) == 2 && st_passes_per_half(1ll << 24) == 3);
  printf("host arithmetic OK\n");
  return 0;
}
