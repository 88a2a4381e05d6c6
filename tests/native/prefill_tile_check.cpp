// Checks the tile lookup and the key range of the prefill kernel (csrc/fcsa_dispatch.h: prefill_slots, prefill_base, prefill_tile,
// prefill_kend) on the CPU.  Built and run by tests/test_prefill_tiles_cpu.py with g++ (also with -fsanitize=address,undefined).  For random
// well-formed tables cu[0 .. B] (empty sequences, single tokens, chunks of several tiles), G in {1, 3, 4, 5, 8} and the tile heights 128
// (the kernel's) and 16 (where prefill_tile must agree with ragged_tile):
//   * the flat slots [0, prefill_slots) map onto exactly the set {(b, rt) : rt < ceil(G * N_b / rows)}, each pair once, with the sequence's
//     own start and length; every other slot is idle, and empty sequences own nothing;
//   * the slot count floor(G * total_q / rows) + B is never below the number of tiles, and no slot at or beyond it is live;
//   * malformed tables (random entries, negative, beyond total, decreasing) keep every start / length inside [0, total] and every
//     sequence index inside [0, B);
//   * the key range [0, kend) of every tile -- and of every 32-row wave share of it -- equals a brute-force "one past the last key any of
//     its rows sees" over the token-major rows r = i * G + g, with and without causal, for L below, at and above N (N_b > L_b included) and
//     L = 0; kend never leaves [0, L].
// The functions are constexpr: one table is also checked at compile time.
// Prints "ok <cases>"; exits 1 at the first failure.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <utility>
#include <vector>

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

// compile time: N_b = 40, 0, 100 with G = 4 -> 160, 0, 400 rows -> tiles 2, 0, 4 in floor(560 / 128) + 3 = 7 slots (bases 0, 2, 3)
constexpr int32_t kCu[4] = {0, 40, 40, 140};
constexpr bool static_case() {
  int b = 0, rt = 0, st = 0, len = 0;
  if (prefill_slots(140, 3, 4, 128) != 7) return false;
  if (!prefill_tile(kCu, 3, 140, 4, 128, 1, b, rt, st, len) || b != 0 || rt != 1 || st != 0 || len != 40) return false;
  if (prefill_tile(kCu, 3, 140, 4, 128, 2, b, rt, st, len)) return false;                      // the empty sequence's slot
  if (!prefill_tile(kCu, 3, 140, 4, 128, 3, b, rt, st, len) || b != 2 || rt != 0 || st != 40 || len != 100) return false;
  if (!prefill_tile(kCu, 3, 140, 4, 128, 6, b, rt, st, len) || b != 2 || rt != 3) return false;
  // 100 tokens against 300 cached positions, G = 4: tile 0 holds tokens 0 .. 31, the last of them sees keys 0 .. 231
  return prefill_kend(300, 100, 4, 0, 128, true) == 232 && prefill_kend(300, 100, 4, 0, 128, false) == 300 &&
         prefill_kend(300, 100, 4, 384, 128, true) == 300 && prefill_kend(8, 40, 4, 0, 128, true) == 0 && prefill_kend(0, 5, 1, 0, 128, false) == 0;
}
static_assert(static_case(), "prefill_tile / prefill_kend at compile time");

// one past the last key any of the rows [first, first + count) sees: token i = r / G sees key j iff j < L and (no causal or j <= L - N + i)
static int brute_kend(int L, int N, int G, int64_t first, int count, bool causal) {
  int kend = 0;
  for (int64_t r = first; r < first + count && r < (int64_t)G * N; ++r) {
    const int i = (int)(r / G);
    for (int j = L - 1; j >= 0; --j) {
      if (!causal || j <= L - N + i) { kend = std::max(kend, j + 1); break; }
    }
  }
  return kend;
}

int main() {
  std::mt19937 rng(1234);
  const int groups[] = {1, 3, 4, 5, 8};
  const int heights[] = {kPrefillRows, kDecodeRows};
  for (int iter = 0; iter < 1500; ++iter) {
    const int B = 1 + (int)(rng() % (iter % 10 == 0 ? 200 : 12));
    std::vector<int32_t> cu(B + 1, 0);
    for (int b = 0; b < B; ++b) {
      const unsigned kind = rng() % 8;
      const int n = kind == 0 ? 0 : kind <= 2 ? 1 : kind == 3 ? 2 + (int)(rng() % 30) : kind <= 5 ? (int)(rng() % 200) : (int)(rng() % 1500);
      cu[b + 1] = cu[b] + n;
    }
    const int64_t total = cu[B];
    for (int G : groups)
      for (int rows : heights) {
        const int64_t slots = prefill_slots(total, B, G, rows);
        CHECK(slots == (int64_t)G * total / rows + B, "slots");
        int64_t tiles = 0;
        for (int b = 0; b < B; ++b) tiles += ((int64_t)G * (cu[b + 1] - cu[b]) + rows - 1) / rows;
        CHECK(tiles <= slots, "B=%d G=%d rows=%d tiles=%lld slots=%lld", B, G, rows, (long long)tiles, (long long)slots);
        std::set<std::pair<int, int>> seen;
        for (int64_t s = 0; s < slots; ++s) {
          int b = -1, rt = -1, st = -1, len = -1;
          const bool live = prefill_tile(cu.data(), B, total, G, rows, s, b, rt, st, len);
          if (rows == kDecodeRows) {      // the closed-form base of ragged_tile with the tile height as a parameter
            int b2 = -1, rt2 = -1, st2 = -1, len2 = -1;
            const bool live2 = ragged_tile(cu.data(), B, total, G, s, b2, rt2, st2, len2);
            CHECK(live == live2 && b == b2 && rt == rt2 && st == st2 && len == len2, "slot %lld: prefill_tile at 16 rows != ragged_tile", (long long)s);
          }
          if (!live) continue;
          CHECK(b >= 0 && b < B, "b=%d", b);
          CHECK(st == cu[b] && len == cu[b + 1] - cu[b], "slot %lld: span (%d, %d) of sequence %d", (long long)s, st, len, b);
          CHECK(len > 0, "an empty sequence owns slot %lld", (long long)s);
          CHECK(rt >= 0 && (int64_t)rt * rows < (int64_t)G * len, "slot %lld: row tile %d of %d rows", (long long)s, rt, G * len);
          CHECK(seen.insert({b, rt}).second, "slot %lld: (%d, %d) twice", (long long)s, b, rt);
        }
        CHECK((int64_t)seen.size() == tiles, "B=%d G=%d rows=%d: %zu of %lld tiles found", B, G, rows, seen.size(), (long long)tiles);
        for (int64_t s = slots; s < slots + 3; ++s) {
          int b, rt, st, len;
          CHECK(!prefill_tile(cu.data(), B, total, G, rows, s, b, rt, st, len), "slot %lld beyond the bound is live", (long long)s);
        }
      }
  }
  // malformed tables: everything stays inside the tensors
  for (int iter = 0; iter < 3000; ++iter) {
    const int B = 1 + (int)(rng() % 12);
    const int64_t total = rng() % 2000;
    std::vector<int32_t> cu(B + 1);
    for (auto& c : cu) c = (int32_t)(rng() % 6000) - 2000 + (rng() % 9 == 0 ? (1 << 30) : 0) - (rng() % 11 == 0 ? (1 << 30) : 0);
    for (int G : groups) {
      const int64_t slots = prefill_slots(total, B, G, kPrefillRows);
      for (int64_t s = 0; s < slots; ++s) {
        int b = -1, rt = -1, st = -1, len = -1;
        const bool live = prefill_tile(cu.data(), B, total, G, kPrefillRows, s, b, rt, st, len);
        CHECK(b >= 0 && b < B, "b=%d", b);
        CHECK(st >= 0 && len >= 0 && (int64_t)st + len <= total, "span (%d, %d) outside [0, %lld]", st, len, (long long)total);
        if (live) CHECK(rt >= 0 && (int64_t)rt * kPrefillRows < (int64_t)G * len, "row tile %d of %d rows", rt, G * len);
      }
    }
  }
  // the key range of every tile and of every wave's 32 rows of it, against brute force
  for (int iter = 0; iter < 600; ++iter) {
    const int G = groups[rng() % 5];
    const unsigned kind = rng() % 6;
    const int N = kind == 0 ? 1 : kind == 1 ? 1 + (int)(rng() % 40) : 1 + (int)(rng() % 300);
    const unsigned lk = rng() % 6;
    const int L = lk == 0 ? 0 : lk == 1 ? (int)(rng() % (N + 1)) : lk == 2 ? N : N + (int)(rng() % 700);      // N > L, N == L, N < L
    const int tiles = (G * N + kPrefillRows - 1) / kPrefillRows;
    for (int causal = 0; causal < 2; ++causal)
      for (int rt = 0; rt <= tiles; ++rt) {      // rt == tiles: a tile without rows
        const int64_t first = (int64_t)rt * kPrefillRows;
        const int kend = prefill_kend(L, N, G, first, kPrefillRows, causal != 0);
        CHECK(kend >= 0 && kend <= L, "kend %d outside [0, %d]", kend, L);
        CHECK(kend == brute_kend(L, N, G, first, kPrefillRows, causal != 0), "L=%d N=%d G=%d rt=%d causal=%d: kend %d, brute force %d", L, N, G, rt,
              causal, kend, brute_kend(L, N, G, first, kPrefillRows, causal != 0));
        int widest = 0;
        for (int w = 0; w < 4; ++w) {
          const int wk = prefill_kend(L, N, G, first + 32 * w, 32, causal != 0);
          CHECK(wk == brute_kend(L, N, G, first + 32 * w, 32, causal != 0), "L=%d N=%d G=%d rt=%d wave %d causal=%d: kend %d", L, N, G, rt, w, causal, wk);
          widest = std::max(widest, wk);
        }
        CHECK(widest == kend, "the widest wave range %d is not the tile's %d", widest, kend);
      }
  }
  std::printf("ok %ld\n", g_cases);
  return 0;
}
