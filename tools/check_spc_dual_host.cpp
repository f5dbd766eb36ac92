// Host-side check of the arithmetic in kaolin_amd/csrc/spc_dual_host.h (key width and radix passes per depth, level offsets from
// a pyramid row, workspace layout) at every depth and at the extents where a 32-bit count would overflow.  Stand-alone, no GPU:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/check_spc_dual_host.cpp -o /tmp/check_spc_dual_host && /tmp/check_spc_dual_host
// Prints one line per point count and "host arithmetic OK"; exits non-zero on a failed expectation.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../kaolin_amd/csrc/spc_dual_host.h"

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "line %d: expectation failed: %s\n", __LINE__, #cond); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

int main() {
  // the sort: every code bit is covered by a pass, the level pass comes last and reads bits 48..55, where only the level lives
  for (int L = 0; L <= SD_MAX_LEVEL; ++L) {
    const int code = sd_code_passes(L), all = code + sd_level_passes(L);
    EXPECT(sd_code_bits(L) == 3 * (L + 1) && 8 * code >= sd_code_bits(L) && 8 * (code - 1) < sd_code_bits(L));
    EXPECT(8 * code <= SD_LEVEL_SHIFT && sd_code_bits(L) <= 45 && (L >> 8) == 0);
    for (int k = 0; k < all; ++k) EXPECT(sd_pass_shift(L, k) == (k < code ? 8 * k : SD_LEVEL_SHIFT));
    EXPECT(sd_level_passes(L) == (L > 0 ? 1 : 0) && sd_sorted_in_b(L) == (all % 2 == 1));
    const SsPasses p = sd_passes(L);  // what the sort is given: the same shifts, ascending, within the key
    EXPECT(p.count == all && p.count <= SS_MAX_PASSES);
    for (int k = 0; k < all; ++k) EXPECT(p.shift[k] == sd_pass_shift(L, k) && p.shift[k] <= 56 && (k == 0 || p.shift[k] > p.shift[k - 1]));
    EXPECT(!sd_bad_extents(1, L));
  }
  EXPECT(sd_code_passes(0) == 1 && sd_code_passes(1) == 1 && sd_code_passes(2) == 2 && sd_code_passes(14) == 6);
  EXPECT(sd_bad_extents(1, SD_MAX_LEVEL + 1) && sd_bad_extents(1, -1) && sd_bad_extents(0, 3) && sd_bad_extents((1ll << 35) + 1, 3));
  EXPECT(sd_workspace_bytes(5, 15) == 0 && sd_workspace_bytes(0, 3) == 0);

  // level offsets: the row is copied, padded with the point count, and checked
  {
    const long long row[] = {0, 1, 3, 10};  // max_level 2, 10 points
    SdLevels lv;
    EXPECT(sd_levels(row, 2, 10, &lv) && lv.max_level == 2);
    for (int l = 0; l <= SD_MAX_LEVEL + 1; ++l) EXPECT(lv.first[l] == (l <= 3 ? row[l] : 10));
    EXPECT(!sd_levels(row, 2, 11, &lv));  // does not end at the point count
    const long long down[] = {0, 4, 3, 10}, late[] = {1, 2, 3, 10};
    EXPECT(!sd_levels(down, 2, 10, &lv) && !sd_levels(late, 2, 10, &lv));
    EXPECT(!sd_levels(row, SD_MAX_LEVEL + 1, 10, &lv) && !sd_levels(row, -1, 10, &lv));
    long long deep[SD_MAX_LEVEL + 2];
    for (int l = 0; l <= SD_MAX_LEVEL + 1; ++l) deep[l] = l;  // the chain to the deepest level
    EXPECT(sd_levels(deep, SD_MAX_LEVEL, SD_MAX_LEVEL + 1, &lv) && lv.first[SD_MAX_LEVEL + 1] == SD_MAX_LEVEL + 1);
  }

  // the workspace: every buffer 256-byte aligned and large enough, none overlapping the next
  const long long ns[] = {1, 255, 256, 257, 1ll << 20, (1ll << 28) + 1, 1ll << 35};
  for (int i = 0; i < 7; ++i) {
    const long long n = ns[i];
    const SdLayout l = sd_layout(n);
    const size_t bytes = sd_workspace_bytes(n, 9);
    printf("n=%lld: keys=%lld sort_blocks=%lld workspace=%zu bytes\n", n, l.keys, l.nsb, bytes);
    EXPECT(l.keys == 8 * n && l.nsb == (l.keys + SS_SORT_BLOCK - 1) / SS_SORT_BLOCK && bytes == l.bytes);
    const long long scan_max = l.nsb * 256 > l.keys ? l.nsb * 256 : l.keys;
    const size_t off[] = {l.sizes, l.keys_a, l.keys_b, l.flags, l.pos, l.hist, l.hoffs, l.sums, l.bytes};
    const size_t need[] = {(size_t)(SD_MAX_LEVEL + 2) * 8, (size_t)l.keys * 8, (size_t)l.keys * 8, (size_t)l.keys * 4,
                           ((size_t)l.keys + 1) * 8, (size_t)l.nsb * 256 * 4, ((size_t)l.nsb * 256 + 1) * 8,
                           ((size_t)ss_cdiv(scan_max, 1024) + 1) * 8};
    for (int k = 0; k < 8; ++k) EXPECT(off[k] % 256 == 0 && off[k + 1] >= off[k] + need[k]);
    EXPECT(bytes >= (size_t)l.keys * 28);  // 8 + 8 + 4 + 8 bytes a key: more than 2^32 for the large n, no 32-bit wrap
    if (n <= 257) {                        // the layout used as offsets into a real buffer
      std::vector<unsigned char> buffer(bytes, 0);
      for (int k = 0; k < 8; ++k) buffer[off[k]] = 1, buffer[off[k] + need[k] - 1] = 1;
    }
  }
  printf("host arithmetic OK\n");
  return 0;
}
