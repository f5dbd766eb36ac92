// Host-side check of the arithmetic in kaolin_amd/csrc/sort_scan_host.h (sort blocks, scratch entries, pass shifts) at the block
// edges and at the extents where a 32-bit count would overflow.  Stand-alone, no GPU:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/check_sort_scan_host.cpp -o /tmp/check_sort_scan_host && /tmp/check_sort_scan_host
// Prints one line per key count and "host arithmetic OK"; exits non-zero on a failed expectation.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../kaolin_amd/csrc/sort_scan_host.h"

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "line %d: expectation failed: %s\n", __LINE__, #cond); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

int main() {
  EXPECT(SS_SORT_BLOCK == 2048 && SS_SORT_BLOCK % 256 == 0 && SS_SCAN_BLOCK == 1024 && SS_MAX_PASSES * 8 == 64);

  // the scratch of a sort of n keys and of a scan of n ints: one histogram row per digit and block, one offset more, one block
  // sum per scan workgroup at least; 64-bit counts throughout (6 * 2^35 keys: the largest a pipeline accepts)
  const long long ns[] = {0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 4097, (1ll << 31) + 1, (1ll << 32) + 2049, 6 * (1ll << 35)};
  for (int i = 0; i < 12; ++i) {
    const long long n = ns[i], nb = ss_sort_blocks(n), hn = (long long)ss_sort_hist_entries(n);
    printf("n=%lld: sort_blocks=%lld hist=%lld scan_sums=%zu sort_sums=%zu\n", n, nb, hn, ss_scan_sums_entries(n),
           ss_sort_sums_entries(n));
    EXPECT(nb >= 1 && nb * SS_SORT_BLOCK >= n && (nb - 1) * SS_SORT_BLOCK < (n > 0 ? n : 1));
    EXPECT(hn == 256 * nb && (long long)ss_sort_offs_entries(n) == hn + 1);
    // a scan of m ints launches max(1, ceil(m / 1024)) workgroups, each writing one block sum
    const long long scans[] = {n, hn};
    const size_t have[] = {ss_scan_sums_entries(n), ss_sort_sums_entries(n)};
    for (int k = 0; k < 2; ++k) {
      const long long groups = scans[k] > 0 ? ss_cdiv(scans[k], SS_SCAN_BLOCK) : 1;
      EXPECT((long long)have[k] >= groups && (long long)have[k] <= groups + 2);
      EXPECT(have[k] >= (size_t)(scans[k] / 1024 + 2));  // not below what the layouts had before
    }
    EXPECT(ss_sort_unique_sums_entries(n) >= ss_sort_sums_entries(n) && ss_sort_unique_sums_entries(n) >= ss_scan_sums_entries(n));
    if (n <= 4097) {  // the entries used as sizes of real buffers, touched at both ends
      std::vector<int> hist(ss_sort_hist_entries(n), 0);
      std::vector<long long> offs(ss_sort_offs_entries(n), 0), sums(ss_sort_sums_entries(n), 0);
      hist[256 * nb - 1] = 1, offs[256 * nb] = 1, sums[ss_cdiv(256 * nb, SS_SCAN_BLOCK) - 1] = 1;
    }
  }
  EXPECT(ss_scan_sums_entries(-5) == 2 && ss_sort_blocks(-5) == 1);
  EXPECT(ss_sort_hist_entries(6 * (1ll << 35)) * 4 > (1ull << 32));  // bytes beyond 32 bits, no wrap

  // the pass lists: low bits; either half; ascending shifts, every bit of the range covered once, nothing beyond the key
  for (int bits = 0; bits <= 64; ++bits) {
    const SsPasses p = ss_passes_low(bits);
    EXPECT(p.count == ss_passes(bits) && p.count <= SS_MAX_PASSES && 8 * p.count >= bits && (bits == 0 || 8 * (p.count - 1) < bits));
    for (int k = 0; k < p.count; ++k) EXPECT(p.shift[k] == 8 * k);
  }
  for (int bits = 1; bits <= 32; ++bits) {
    const SsPasses p = ss_passes_halves(bits);
    const int per = ss_passes(bits);
    EXPECT(p.count == 2 * per && p.count % 2 == 0 && p.count <= SS_MAX_PASSES);
    for (int k = 0; k < p.count; ++k) EXPECT(p.shift[k] == (k < per ? 8 * k : 32 + 8 * (k - per)) && p.shift[k] <= 56);
  }
  EXPECT(ss_passes_low(0).count == 0 && ss_passes_low(45).count == 6 && ss_passes_halves(32).shift[7] == 56);
  EXPECT(ss_passes_halves(40).count == 8);  // clamped to a half: never more than SS_MAX_PASSES entries
  printf("host arithmetic OK\n");
  return 0;
}
