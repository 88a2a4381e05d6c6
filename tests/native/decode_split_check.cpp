// Checks the key/value-cache decode helpers of csrc/fcsa_dispatch.h on the CPU (decode_splits, decode_window, decode_len,
// decode_groups_fast).  Built and run by tests/test_kvcache_cpu.py with g++.
//   * the split count lies in [1, kDecodeMaxSplits] and gives every split at least decode_min_split_keys(D) keys of max_k (or is 1);
//   * the grid covers the CUs (>= cu_count workgroups) whenever the cache is long enough for that many splits;
//   * for every length L in [0, capacity] and every split count, the windows of the splits tile [0, L) exactly, in order, without
//     overlap, each inside [0, L) and starting on a 32-key block;
//   * decode_len clamps any table entry (negative, huge) into [0, capacity];
//   * decode_groups_fast (the in-register group reduction) holds for every divisor of D = 16, 32, 64, 128 and, at D = 96, for all but
//     groups 2, 4, 8, 16, 32 (widths 48, 24, 12, 6, 3), which the kernel's LDS form handles.
// Prints "ok <cases>"; exits 1 at the first failure.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "fcsa_dispatch.h"

using namespace fcsa;

static long g_cases = 0;
#define CHECK(cond, ...)                                                        \
  do {                                                                          \
    ++g_cases;                                                                  \
    if (!(cond)) {                                                              \
      std::fprintf(stderr, "FAILED %s: ", #cond);                               \
      std::fprintf(stderr, __VA_ARGS__);                                        \
      std::fprintf(stderr, "\n");                                               \
      std::exit(1);                                                             \
    }                                                                           \
  } while (0)

int main() {
  const int dims[] = {16, 32, 64, 96, 128};
  const int cus_list[] = {256, 304, 80};
  std::mt19937 rng(1234);
  for (int cus : cus_list)
    for (int D : dims)
      for (int64_t B : {1, 2, 8, 32, 1024})
        for (int Hk : {1, 8, 32})
          for (int rt : {1, 2, 8})
            for (int max_k : {0, 1, 31, 100, 1024, 8192, 32768, 131072, 1 << 20}) {
              const int s = decode_splits(B, Hk, rt, max_k, D, cus);
              CHECK(s >= 1 && s <= kDecodeMaxSplits, "s=%d", s);
              CHECK(s == 1 || (int64_t)s * decode_min_split_keys(D) <= max_k, "s=%d max_k=%d D=%d", s, max_k, D);
              const int64_t base = B * Hk * rt;
              const int64_t room = std::max(1, max_k / decode_min_split_keys(D));
              // long enough for the splits that would cover the chip: the grid does
              if (room * base >= cus && kDecodeMaxSplits * base >= cus) CHECK(base * s >= cus, "B=%lld Hk=%d rt=%d max_k=%d s=%d", (long long)B, Hk, rt, max_k, s);
            }
  // windows tile [0, L) for every L in [0, capacity]
  for (int splits : {1, 2, 3, 7, 32, 64, 128})
    for (int cap : {0, 1, 31, 32, 33, 300, 1000, 4096}) {
      for (int L = 0; L <= cap; ++L) {
        int next = 0;
        for (int s = 0; s < splits; ++s) {
          int lo = -1, n = -1;
          decode_window(L, s, splits, lo, n);
          CHECK(lo >= 0 && n >= 0 && lo + n <= L, "L=%d s=%d lo=%d n=%d", L, s, lo, n);
          CHECK(n == 0 || lo % kDecodeBlock == 0, "lo=%d", lo);
          CHECK(n == 0 || lo == next, "L=%d s=%d lo=%d next=%d", L, s, lo, next);
          next = lo + n > next ? lo + n : next;
        }
        CHECK(next == L, "L=%d splits=%d covered %d", L, splits, next);
      }
    }
  // table entries clamp into [0, capacity]
  for (int i = 0; i < 20000; ++i) {
    const int cap = (int)(rng() % 5000);
    const int64_t raw = (int64_t)(rng() % 20000) - 10000 + (i % 7 == 0 ? (int64_t)1 << 40 : 0);
    const int nn = (int)(rng() % 40);
    const int L = decode_len(true, raw, nn, cap);
    CHECK(L >= 0 && L <= cap, "L=%d cap=%d", L, cap);
    CHECK(decode_len(false, raw, nn, cap) == cap, "null table");
    if (raw >= 0 && raw + nn <= cap) CHECK(L == raw + nn, "well-formed entry reproduced");
  }
  // groups: which widths the kernel reduces in registers; the rest (D = 96 only) take its LDS form
  for (int unit : {8, 4})
    for (int D : dims)
      for (int g = 1; g <= D; ++g) {
        if (D % g != 0) {
          CHECK(!decode_groups_fast(D, g, unit), "D=%d groups=%d is not a divisor", D, g);
          continue;
        }
        const bool straddles = D == 96 && (g == 2 || g == 4 || g == 8 || g == 16 || g == 32);
        CHECK(decode_groups_fast(D, g, unit) == !straddles, "D=%d groups=%d unit=%d", D, g, unit);
      }
  std::printf("ok %ld\n", g_cases);
  return 0;
}
