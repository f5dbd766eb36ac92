// Host-side check of the arithmetic in kaolin_amd/csrc/subdivide_trianglemesh_host.h (workspace layout; the radix passes come
// from subdivide_tetmesh_host.h) at the extents where a 32-bit count would overflow.  Stand-alone, no GPU:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/check_subdivide_trianglemesh_host.cpp -o /tmp/check_subdivide_trianglemesh_host && \
//         /tmp/check_subdivide_trianglemesh_host
// (with hipcc: -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined).  Prints one line per (F, V) and
// "host arithmetic OK"; exits non-zero on a failed expectation.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../kaolin_amd/csrc/subdivide_trianglemesh_host.h"

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "line %d: expectation failed: %s\n", __LINE__, #cond); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

int main() {
  const long long Fs[] = {0, 1, 720, (1ll << 31) / 3 + 1};
  const long long Vs[] = {1, 1ll << 16, (1ll << 32) - 1};
  const int bits[] = {1, 16, 32}, passes[] = {1, 2, 4};
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 3; ++j) {
      const long long F = Fs[i], V = Vs[j];
      EXPECT(!sl_bad_extents(F, V));
      EXPECT(st_id_bits(V) == bits[j] && st_passes_per_half(V) == passes[j]);
      const size_t bytes = sl_workspace_bytes(F, V);
      const SlLayout l = sl_layout(F);
      printf("F=%lld V=%lld: keys=%lld sort_blocks=%lld id_bits=%d passes=2x%d workspace=%zu bytes\n", F, V, l.n, l.nsb,
             st_id_bits(V), st_passes_per_half(V), bytes);
      if (F == 0) {
        EXPECT(bytes == 0);
        continue;
      }
      EXPECT(l.n == 3 * F && l.nsb == (l.n + SS_SORT_BLOCK - 1) / SS_SORT_BLOCK && bytes == l.bytes);
      // the buffers, in order, each 16-byte aligned and large enough, none overlapping the next; the second sort (E <= 3 F
      // keys) fits the buffers sized for the first
      const size_t off[] = {l.keys_a, l.keys_b, l.keys_c, l.flags, l.pos, l.hist, l.hoffs, l.sums, l.bytes};
      const size_t need[] = {(size_t)l.n * 8, (size_t)l.n * 8, (size_t)l.n * 8, (size_t)l.n * 4, ((size_t)l.n + 1) * 8,
                             (size_t)l.nsb * 256 * 4, ((size_t)l.nsb * 256 + 1) * 8,
                             ((size_t)ss_cdiv(l.nsb * 256 > l.n ? l.nsb * 256 : l.n, 1024) + 1) * 8};
      for (int k = 0; k < 8; ++k) EXPECT(off[k] % 16 == 0 && off[k + 1] >= off[k] + need[k]);
      EXPECT(bytes >= (size_t)l.n * 36);  // 8 + 8 + 8 + 4 + 8 bytes a key: more than 2^32 for the large F, no 32-bit wrap
      if (F <= 720) {                     // the layout used as offsets into a real buffer
        std::vector<unsigned char> buffer(bytes, 0);
        for (int k = 0; k < 8; ++k) buffer[off[k]] = 1, buffer[off[k] + need[k] - 1] = 1;
      }
    }
  }
  EXPECT(sl_bad_extents(-1, 1) && sl_bad_extents(1, -1) && sl_bad_extents(1, 1ll << 32) && sl_bad_extents((1ll << 35) + 1, 1));
  EXPECT(sl_workspace_bytes(5, 1ll << 32) == 0 && sl_workspace_bytes(5, 0) == 0);
  printf("host arithmetic OK\n");
  return 0;
}
