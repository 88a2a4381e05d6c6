// Checks the routing partition and the windowed key range of an engine step (csrc/fcsa_dispatch.h: step_is_chunk over ragged_tile and
// prefill_tile, prefill_kstart, prefill_win_kend) on the CPU.  Built and run by tests/test_step_launches_cpu.py with g++ (also with
// -fsanitize=address,undefined: a stand-alone program).
//   * For random tables -- well-formed ones and malformed ones (non-decreasing entries that are negative or beyond total_q: what
//     ragged_cu clamps) -- G in {1, 3, 4, 5, 8} and thresholds 0, 1, 16, 127, 128, 129, 512 and beyond G * total_q: with N_b the clamped row
//     count of sequence b (max(cu(b + 1), cu(b)) - cu(b)), every (sequence, row) with row < G * N_b is claimed by exactly one tile of exactly
//     one of the two tile maps -- a 16-row tile of the decode map when G * N_b < chunk_rows, a 128-row tile of the chunk map otherwise -- and
//     no tile of either map claims anything else.  The combine's test (ragged_seq_of, then the same clamped count) agrees for every packed
//     row of a well-formed table.
//   * The key range [prefill_kstart, prefill_win_kend) of every 128-row tile contains every key visible to any of its rows under the ragged
//     kernel's test (key < L, key <= last_key + hi, key >= last_key - lo, last_key = L - N + token); the start is a multiple of the 64-key
//     stage and no later than the first visible key; each wave's 32-row end is the brute-force one and the widest wave end is the tile's;
//     with both sides open (or hi = 0: causal) the range is prefill_kend's from key 0.
// Prints "ok <cases>"; exits 1 at the first failure.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
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

// compile time: 130 tokens against 193 positions, G = 4, window (64, 5): tile 1 starts at token 32 (last_key 95): keys 31 .. 100 for its
// first token, so the start is stage 0; tile 4 (token 128, last_key 191) starts at key 127 -> stage 64
static_assert(prefill_kstart(193, 130, 4, 128, 64) == 0 && prefill_kstart(193, 130, 4, 512, 64) == 64 && prefill_kstart(193, 130, 4, 512, kWinOpen) == 0, "");
static_assert(prefill_win_kend(193, 130, 4, 0, 128, 5) == 63 + 31 + 5 + 1 && prefill_win_kend(193, 130, 4, 512, 128, 5) == 193, "");
static_assert(prefill_win_kend(193, 130, 4, 0, 128, 0) == prefill_kend(193, 130, 4, 0, 128, true), "");
static_assert(prefill_win_kend(193, 130, 4, 0, 128, kWinOpen) == 193 && prefill_win_kend(0, 5, 1, 0, 128, 3) == 0, "");
static_assert(step_is_chunk(8, 16, 128) && !step_is_chunk(8, 16, 129) && step_is_chunk(4, 0, 0) && !step_is_chunk(4, 1 << 20, 1 << 30), "");

static void partition(const std::vector<int32_t>& cu, int B, int64_t total, int G, int chunk_rows, bool well_formed) {
  // (sequence, row) -> how often each map claims it
  std::map<std::pair<int, int64_t>, std::pair<int, int>> claims;
  const int64_t dslots = ragged_slots(total, B, G), cslots = prefill_slots(total, B, G, kPrefillRows);
  for (int64_t s = 0; s < dslots; ++s) {
    int b = -1, rt = -1, st = -1, len = -1;
    if (!ragged_tile(cu.data(), B, total, G, s, b, rt, st, len) || step_is_chunk(G, len, chunk_rows)) continue;
    for (int64_t r = (int64_t)rt * kDecodeRows; r < (int64_t)(rt + 1) * kDecodeRows && r < (int64_t)G * len; ++r) ++claims[{b, r}].first;
  }
  for (int64_t s = 0; s < cslots; ++s) {
    int b = -1, rt = -1, st = -1, len = -1;
    if (!prefill_tile(cu.data(), B, total, G, kPrefillRows, s, b, rt, st, len) || !step_is_chunk(G, len, chunk_rows)) continue;
    for (int64_t r = (int64_t)rt * kPrefillRows; r < (int64_t)(rt + 1) * kPrefillRows && r < (int64_t)G * len; ++r) ++claims[{b, r}].second;
  }
  int64_t rows = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t st = ragged_cu(cu[b], total), en = std::max(ragged_cu(cu[b + 1], total), st), n = en - st;
    const bool chunk = step_is_chunk(G, n, chunk_rows);
    for (int64_t r = 0; r < (int64_t)G * n; ++r, ++rows) {
      const auto it = claims.find({b, r});
      CHECK(it != claims.end(), "B=%d G=%d t=%d: row %lld of sequence %d (N %lld) is claimed by no tile", B, G, chunk_rows, (long long)r, b, (long long)n);
      CHECK(it->second.first == (chunk ? 0 : 1) && it->second.second == (chunk ? 1 : 0), "B=%d G=%d t=%d: row %lld of sequence %d: %d decode, %d chunk claims",
            B, G, chunk_rows, (long long)r, b, it->second.first, it->second.second);
    }
  }
  CHECK((int64_t)claims.size() == rows, "B=%d G=%d t=%d: %zu claims for %lld rows", B, G, chunk_rows, claims.size(), (long long)rows);
  if (!well_formed) return;
  // the combine: packed row tok -> its sequence -> the same decision as the tile that wrote its partials
  for (int64_t tok = 0; tok < total; ++tok) {
    const int b = ragged_seq_of(cu.data(), B, total, tok);
    const int64_t st = ragged_cu(cu[b], total), en = std::max(ragged_cu(cu[b + 1], total), st);
    CHECK(st <= tok && tok < en, "row %lld is not in sequence %d", (long long)tok, b);
    CHECK(claims.at({b, (tok - st)}).first == (step_is_chunk(G, en - st, chunk_rows) ? 0 : 1), "the combine and the decode tiles disagree on row %lld", (long long)tok);
  }
}

static bool visible(int L, int last_key, int lo, int hi, int key) { return key < L && key <= last_key + hi && key >= last_key - lo; }

int main() {
  std::mt19937 rng(4321);
  const int groups[] = {1, 3, 4, 5, 8};
  for (int iter = 0; iter < 90; ++iter) {
    const bool well_formed = iter % 3 != 0;
    const int B = 1 + (int)(rng() % (iter % 10 == 0 ? 60 : 10));
    std::vector<int32_t> cu(B + 1, 0);
    int64_t total;
    if (well_formed) {
      for (int b = 0; b < B; ++b) {
        const unsigned kind = rng() % 8;
        const int n = kind == 0 ? 0 : kind <= 2 ? 1 : kind == 3 ? 2 + (int)(rng() % 30) : kind <= 5 ? (int)(rng() % 200) : (int)(rng() % 700);
        cu[b + 1] = cu[b] + n;
      }
      total = cu[B];
    } else {
      total = rng() % 900;
      // non-decreasing entries that leave [0, total] at both ends, far out at times: ragged_cu's clamp makes a table of them
      for (auto& c : cu) c = (int32_t)(rng() % (total + 1600)) - 800;
      std::sort(cu.begin(), cu.end());
      if (rng() % 3 == 0) cu[0] = -(1 << 30);
      if (rng() % 3 == 0) cu[B] = 1 << 30;
    }
    for (int G : groups) {
      const int64_t beyond = std::min<int64_t>((int64_t)G * total + 1, INT32_MAX);
      for (int t : {0, 1, 16, 127, 128, 129, 512, (int)beyond, 1 << 30}) partition(cu, B, total, G, t, well_formed);
    }
  }
  // the windowed key range of every tile and of every wave's 32 rows of it
  const int sides[] = {0, 1, 5, 31, 32, 63, 64, 65, 200, kWinOpen};
  for (int iter = 0; iter < 300; ++iter) {
    const int G = groups[rng() % 5];
    const unsigned kind = rng() % 6;
    const int N = kind == 0 ? 1 : kind == 1 ? 1 + (int)(rng() % 40) : 1 + (int)(rng() % 300);
    const unsigned lk = rng() % 6;
    const int L = lk == 0 ? 0 : lk == 1 ? (int)(rng() % (N + 1)) : lk == 2 ? N : N + (int)(rng() % 700);
    const int lo = sides[rng() % 10], hi = sides[rng() % 10];
    const int tiles = (G * N + kPrefillRows - 1) / kPrefillRows;
    for (int rt = 0; rt <= tiles; ++rt) {      // rt == tiles: a tile without rows
      const int64_t first = (int64_t)rt * kPrefillRows;
      const int kstart = prefill_kstart(L, N, G, first, lo), kend = prefill_win_kend(L, N, G, first, kPrefillRows, hi);
      CHECK(kstart >= 0 && kstart % kPrefillStage == 0 && kend >= 0 && kend <= L, "L=%d N=%d: range [%d, %d)", L, N, kstart, kend);
      if (lo >= kWinOpen) CHECK(kstart == 0, "an open left side starts at %d", kstart);
      if (hi >= kWinOpen || hi == 0) CHECK(kend == prefill_kend(L, N, G, first, kPrefillRows, hi == 0), "an open or causal right side ends at %d", kend);
      int widest = 0;
      for (int w = 0; w < 4; ++w) {
        int brute = 0;
        for (int64_t r = first + 32 * w; r < first + 32 * (w + 1) && r < (int64_t)G * N; ++r) {
          const int last_key = L - N + (int)(r / G);
          for (int key = 0; key < L; ++key) {
            if (!visible(L, last_key, lo, hi, key)) continue;
            CHECK(key >= kstart && key < kend, "L=%d N=%d G=%d lo=%d hi=%d rt=%d: key %d of row %lld outside [%d, %d)", L, N, G, lo, hi, rt, key, (long long)r, kstart, kend);
          }
          // the end ignores the left side, as prefill_kend does: one past the last key the right side and L allow
          brute = std::max(brute, (int)std::min<int64_t>(std::max<int64_t>((int64_t)last_key + std::min(hi, kWinOpen) + 1, 0), L));
        }
        const int wk = prefill_win_kend(L, N, G, first + 32 * w, 32, hi);
        CHECK(wk == brute, "L=%d N=%d G=%d hi=%d rt=%d wave %d: end %d, brute force %d", L, N, G, hi, rt, w, wk, brute);
        widest = std::max(widest, wk);
      }
      CHECK(widest == kend, "the widest wave end %d is not the tile's %d", widest, kend);
      // the start is tight to one stage: the stage before it holds no key the tile's first token sees
      if (kstart > 0 && first < (int64_t)G * N) {
        const int last_key = L - N + (int)(first / G);
        CHECK(last_key - lo >= kstart && last_key - lo < kstart + kPrefillStage, "start %d for a first key of %d", kstart, last_key - lo);
      }
    }
  }
  std::printf("ok %ld\n", g_cases);
  return 0;
}
