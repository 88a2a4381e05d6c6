// Checks the tile-lookup rule of a ragged decode step (csrc/fcsa_dispatch.h: ragged_slots, ragged_base, ragged_tile, ragged_seq_of) on
// the CPU.  Built and run by tests/test_kvcache_ragged_cpu.py with g++.  For random well-formed tables cu[0 .. B] (empty sequences, single
// tokens, a few tokens, long chunks) and every group width G:
//   * the flat slots [0, ragged_slots) map onto exactly the set {(b, rt) : rt < ceil(G * N_b / 16)}, each pair once, with the sequence's
//     own start and length; every other slot is idle, and empty sequences own nothing;
//   * the slot count floor(G * total_q / 16) + B (the bound the grid is sized with) is never below the number of tiles, and no slot at
//     or beyond it is live;
//   * ragged_seq_of finds, for every packed row, the sequence whose span holds it;
//   * malformed tables (random entries, negative, beyond total, decreasing) keep every start / length inside [0, total] and every
//     sequence index inside [0, B).
// The functions are constexpr: one table is also checked at compile time.
// Prints "ok <cases>"; exits 1 at the first failure.
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

// compile time: N_b = 1, 0, 5 with G = 4 -> tiles 1, 0, 2 in 1 + 3 = 4 slots (bases 0, 1, 2)
constexpr int32_t kCu[4] = {0, 1, 1, 6};
constexpr bool static_case() {
  int b = 0, rt = 0, st = 0, len = 0;
  if (ragged_slots(6, 3, 4) != 4) return false;
  if (!ragged_tile(kCu, 3, 6, 4, 0, b, rt, st, len) || b != 0 || rt != 0 || st != 0 || len != 1) return false;
  if (ragged_tile(kCu, 3, 6, 4, 1, b, rt, st, len)) return false;                      // the empty sequence's slot
  if (!ragged_tile(kCu, 3, 6, 4, 2, b, rt, st, len) || b != 2 || rt != 0 || st != 1 || len != 5) return false;
  if (!ragged_tile(kCu, 3, 6, 4, 3, b, rt, st, len) || b != 2 || rt != 1) return false;
  return ragged_seq_of(kCu, 3, 6, 0) == 0 && ragged_seq_of(kCu, 3, 6, 1) == 2 && ragged_seq_of(kCu, 3, 6, 5) == 2;
}
static_assert(static_case(), "ragged_tile at compile time");

int main() {
  std::mt19937 rng(4321);
  const int groups[] = {1, 2, 3, 4, 8, 16, 32, 64};
  for (int iter = 0; iter < 3000; ++iter) {
    const int B = 1 + (int)(rng() % (iter % 10 == 0 ? 300 : 20));
    std::vector<int32_t> cu(B + 1, 0);
    for (int b = 0; b < B; ++b) {
      const unsigned kind = rng() % 8;
      const int n = kind == 0 ? 0 : kind <= 4 ? 1 : kind == 5 ? 2 + (int)(rng() % 7) : kind == 6 ? (int)(rng() % 40) : (int)(rng() % 600);
      cu[b + 1] = cu[b] + n;
    }
    const int64_t total = cu[B];
    for (int G : groups) {
      const int64_t slots = ragged_slots(total, B, G);
      CHECK(slots == (int64_t)G * total / 16 + B, "slots");
      int64_t tiles = 0;
      for (int b = 0; b < B; ++b) tiles += ((int64_t)G * (cu[b + 1] - cu[b]) + 15) / 16;
      CHECK(tiles <= slots, "B=%d G=%d tiles=%lld slots=%lld", B, G, (long long)tiles, (long long)slots);
      std::set<std::pair<int, int>> seen;
      for (int64_t s = 0; s < slots; ++s) {
        int b = -1, rt = -1, st = -1, len = -1;
        if (!ragged_tile(cu.data(), B, total, G, s, b, rt, st, len)) continue;
        CHECK(b >= 0 && b < B, "b=%d", b);
        CHECK(st == cu[b] && len == cu[b + 1] - cu[b], "slot %lld: span (%d, %d) of sequence %d", (long long)s, st, len, b);
        CHECK(len > 0, "an empty sequence owns slot %lld", (long long)s);
        CHECK(rt >= 0 && (int64_t)rt * 16 < (int64_t)G * len, "slot %lld: row tile %d of %d rows", (long long)s, rt, G * len);
        CHECK(seen.insert({b, rt}).second, "slot %lld: (%d, %d) twice", (long long)s, b, rt);
      }
      CHECK((int64_t)seen.size() == tiles, "B=%d G=%d: %zu of %lld tiles found", B, G, seen.size(), (long long)tiles);
      // no tile at or beyond the bound
      for (int64_t s = slots; s < slots + 3; ++s) {
        int b, rt, st, len;
        CHECK(!ragged_tile(cu.data(), B, total, G, s, b, rt, st, len), "slot %lld beyond the bound is live", (long long)s);
      }
    }
    for (int64_t tok = 0; tok < total; ++tok) {
      const int b = ragged_seq_of(cu.data(), B, total, tok);
      CHECK(b >= 0 && b < B && cu[b] <= tok && tok < cu[b + 1], "row %lld -> sequence %d", (long long)tok, b);
    }
  }
  // malformed tables: everything stays inside the tensors
  for (int iter = 0; iter < 3000; ++iter) {
    const int B = 1 + (int)(rng() % 12);
    const int64_t total = rng() % 200;
    std::vector<int32_t> cu(B + 1);
    for (auto& c : cu) c = (int32_t)(rng() % 600) - 200 + (rng() % 9 == 0 ? (1 << 30) : 0) - (rng() % 11 == 0 ? (1 << 30) : 0);
    for (int G : {1, 4, 32}) {
      const int64_t slots = ragged_slots(total, B, G);
      for (int64_t s = 0; s < slots; ++s) {
        int b = -1, rt = -1, st = -1, len = -1;
        const bool live = ragged_tile(cu.data(), B, total, G, s, b, rt, st, len);
        CHECK(b >= 0 && b < B, "b=%d", b);
        CHECK(st >= 0 && len >= 0 && (int64_t)st + len <= total, "span (%d, %d) outside [0, %lld]", st, len, (long long)total);
        if (live) CHECK(rt >= 0 && (int64_t)rt * 16 < (int64_t)G * len, "row tile %d of %d rows", rt, G * len);
      }
    }
    for (int64_t tok = 0; tok < total; ++tok) {
      const int b = ragged_seq_of(cu.data(), B, total, tok);
      CHECK(b >= 0 && b < B, "row %lld -> sequence %d", (long long)tok, b);
    }
  }
  std::printf("ok %ld\n", g_cases);
  return 0;
}
