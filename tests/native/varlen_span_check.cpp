// Checks the packed-sequence helpers of csrc/fcsa_dispatch.h on the CPU (seq_span, seq_pair_idle) and the form rules for packed
// problems.  Built and run by tests/test_varlen_cpu.py with g++.
//   * every span lies inside [0, total) and is at most max_len long, for random, malformed and extreme tables (64-bit entries included);
//   * a well-formed table whose spans fit max_len is reproduced exactly;
//   * over the max-sized grid (sequences x heads x tile_pairs(tile_count(max_len))), the workgroups that do not exit early (seq_pair_idle)
//     run every (sequence, head, tile) exactly once -- row tiles and key tiles, causal and not;
//   * choose_forward / choose_dq / choose_dkv never give a packed problem Fwd2, Fwd3 or the group sweep, at 256, 304 and 80 CUs.
// Prints the number of checked cases; exits 1 at the first failure.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
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

static void check_inside(int64_t lo, int64_t hi, int total, int max_len) {
  int start = -1, len = -1;
  seq_span(lo, hi, total, max_len, start, len);
  CHECK(start >= 0 && start <= total && len >= 0 && len <= std::max(max_len, 0) && (int64_t)start + len <= total,
        "lo %lld hi %lld total %d max %d -> start %d len %d", (long long)lo, (long long)hi, total, max_len, start, len);
}

// the work of one (sequence, head) under the early-exit rule: every tile once
static void check_grid(const std::vector<int>& lens, int n_heads, int tile, int causal, bool rows) {
  const int S = (int)lens.size();
  int max_len = 0;
  for (int l : lens) max_len = std::max(max_len, l);
  const int pairs = tile_pairs(tile_count(max_len, tile), causal);
  std::vector<std::vector<int>> seen(S);
  for (int s = 0; s < S; ++s) seen[s].assign((size_t)n_heads * tile_count(lens[s], tile), 0);
  for (int id = 0; id < S * n_heads * pairs; ++id) {
    int bh = -1, pair = -1;
    block_work(id, S * n_heads, pairs, bh, pair);
    const int s = bh / n_heads, h = bh % n_heads;
    int start = 0, len = 0;
    int64_t cu_lo = 0;
    for (int t = 0; t < s; ++t) cu_lo += lens[t];
    seq_span(cu_lo, cu_lo + lens[s], 1 << 30, max_len, start, len);
    if (seq_pair_idle(pair, len, tile, causal)) continue;
    const int tiles = tile_count(len, tile);
    for (int pass = 0; pass < pair_passes(tiles, pair, causal); ++pass) {
      const int t = pass_tile(tiles, pair, pass, causal, rows);
      CHECK(t >= 0 && t < tiles, "s %d pair %d pass %d tiles %d", s, pair, pass, tiles);
      ++seen[s][(size_t)h * tiles + t];
    }
  }
  for (int s = 0; s < S; ++s)
    for (size_t i = 0; i < seen[s].size(); ++i)
      CHECK(seen[s][i] == 1, "sequence %d (len %d) head-tile %zu ran %d times (tile %d causal %d)", s, lens[s], i, seen[s][i], tile, causal);
}

int main() {
  std::mt19937_64 rng(12345);
  // random and malformed tables: anything in [-2^40, 2^40], decreasing entries, entries past the total
  for (int it = 0; it < 200000; ++it) {
    const int total = (int)(rng() % 5000), max_len = (int)(rng() % 3000) - 5;
    auto pick = [&]() -> int64_t {
      switch (rng() % 4) {
        case 0: return (int64_t)(rng() % (uint64_t)(total + 10)) - 5;
        case 1: return (int64_t)(rng() >> 23) - ((int64_t)1 << 40);
        case 2: return (int64_t)(rng() % 2 ? INT32_MAX : INT32_MIN);
        default: return (int64_t)(rng() % (uint64_t)(total + 1));
      }
    };
    check_inside(pick(), pick(), total, max_len);
  }
  // well-formed tables: reproduced exactly
  for (int it = 0; it < 2000; ++it) {
    const int S = 1 + (int)(rng() % 600);
    std::vector<int64_t> cu(S + 1, 0);
    int max_len = 0;
    for (int s = 0; s < S; ++s) {
      const int l = (rng() % 5 == 0) ? 0 : (int)(rng() % 700);
      cu[s + 1] = cu[s] + l;
      max_len = std::max(max_len, l);
    }
    const int total = (int)cu[S];
    for (int s = 0; s < S; ++s) {
      int start = -1, len = -1;
      seq_span(cu[s], cu[s + 1], total, max_len + (int)(rng() % 3), start, len);
      CHECK(start == cu[s] && len == cu[s + 1] - cu[s], "sequence %d of %d", s, S);
    }
  }
  // early exit over the max-sized grid
  const std::vector<std::vector<int>> mixes = {
      {0}, {1}, {128}, {129, 0, 1, 127, 128}, {4096, 16, 16, 16, 0, 300}, {777, 1000, 33, 256, 257, 511, 512, 513}};
  for (const auto& lens : mixes)
    for (int heads : {1, 3, 8})
      for (int tile : {64, 128, 256})
        for (int causal : {0, 1})
          for (bool rows : {true, false}) check_grid(lens, heads, tile, causal, rows);
  for (int it = 0; it < 40; ++it) {
    std::vector<int> lens(1 + rng() % 40);
    for (int& l : lens) l = (int)(rng() % 1500);
    check_grid(lens, 1 + (int)(rng() % 8), 128, (int)(rng() % 2), rng() % 2 == 0);
  }
  // form rules: never Fwd2 / Fwd3 / the group sweep for a packed problem
  for (int cus : {256, 304, 80})
    for (int es : {2, 4})
      for (int D : {16, 32, 64, 96, 128})
        for (int64_t bh : {1, 8, 64, 256, 4096, 1 << 15})
          for (int len : {1, 100, 1024, 8192, 16384})
            for (int causal : {0, 1})
              for (int dyn : {0, 1}) {
                FwdProblem f{es, D, bh, len, len, causal != 0, false, false, dyn != 0, 1, (int64_t)D * es, (int64_t)D * es, (int64_t)D * es, 1};
                f.varlen = true;
                const FwdForm ff = choose_forward(f, cus);
                CHECK(ff != FwdForm::Fwd2 && ff != FwdForm::Fwd3, "cus %d es %d D %d bh %lld len %d causal %d", cus, es, D, (long long)bh, len, causal);
                BwdProblem b{es, D, bh, len, len, causal != 0, false, 1, true};
                b.varlen = true;
                (void)choose_dq(b, cus);
                CHECK(choose_dkv(b, cus) != DkvForm::Sweep, "cus %d es %d D %d bh %lld len %d", cus, es, D, (long long)bh, len);
              }
  std::printf("ok %ld cases\n", g_cases);
  return 0;
}
