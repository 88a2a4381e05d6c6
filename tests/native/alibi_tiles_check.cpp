// The tile-ownership functions of csrc/fcsa_dispatch.h under the window sides a call with alibi_slopes launches with: every call with
// slopes is a windowed launch, also where win_normalise calls the window Full -- sides (kWinOpen, kWinOpen) -- or Causal -- (kWinOpen, 0) --
// which window_tiles_check.cpp leaves to the un-windowed kernels and does not walk.  Same brute-force comparison against the visibility
// matrix, for those two kinds only (N > M under causal included: rows without a visible key); also that no intermediate of the kernels'
// index arithmetic leaves the int range with open sides.  Built and run by tests/test_alibi_train_cpu.py with g++.
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

static bool visible(int N, int M, int i, int j, int left, int right, bool causal) {
  const int d = M - N, r = causal ? 0 : right;
  return (left < 0 || j >= i + d - left) && (r < 0 || j <= i + d + r);
}

static void check_problem(int N, int M, int left, int right, bool causal, int bm, int bn, int bmq, int bnk) {
  int lo, hi;
  const WinKind kind = win_normalise(N, M, causal, left, right, lo, hi);
  std::vector<char> vis((size_t)N * M);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < M; ++j) vis[(size_t)i * M + j] = visible(N, M, i, j, left, right, causal);
  // normalisation: Full / Causal hide exactly what the un-windowed / causal problem hides
  if (kind == WinKind::Window) return;      // (window_tiles_check.cpp)
  CHECK(lo == kWinOpen && (hi == kWinOpen || hi == 0), "sides of a %s launch: %d %d", kind == WinKind::Full ? "full" : "causal", lo, hi);
  CHECK((int64_t)N + M + 2 * (int64_t)kWinOpen + 4096 < INT32_MAX, "index range");      // the largest |diff|, |dlo| plus a tile: no int overflow
  auto any = [&](int i0, int i1, int j0, int j1) {
    for (int i = i0; i < std::min(i1, N); ++i)
      for (int j = j0; j < std::min(j1, M); ++j)
        if (vis[(size_t)i * M + j]) return true;
    return false;
  };
  auto all = [&](int i0, int i1, int j0, int j1) {      // every pair of real rows x the whole key tile (keys past M count as hidden)
    if (j1 > M) return false;
    for (int i = i0; i < std::min(i1, N); ++i)
      for (int j = j0; j < j1; ++j)
        if (!vis[(size_t)i * M + j]) return false;
    return true;
  };
  // ---- forward / dQ: row tiles of bm rows, key tiles of bn keys
  for (int m0 = 0; m0 < N; m0 += bm) {
    int k_lo, len;
    win_key_window(N, M, m0, bm, lo, hi, bn, k_lo, len);
    CHECK(k_lo % bn == 0 && k_lo >= 0 && len >= 0 && k_lo + len <= M, "window N %d M %d m0 %d: [%d, +%d)", N, M, m0, k_lo, len);
    const int diff = M - N + hi - k_lo, dlo = M - N - lo - k_lo;
    const int nt = key_tiles(len, m0, bm, diff, 1, bn);
    CHECK(nt == tile_count(len, bn), "nt %d len %d", nt, len);
    for (int t = 0; t < tile_count(M, bn); ++t) {
      const bool visited = len > 0 && t >= k_lo / bn && t < k_lo / bn + nt;
      CHECK(visited == any(m0, m0 + bm, t * bn, (t + 1) * bn), "N %d M %d (%d, %d) causal %d bm %d bn %d: row tile %d key tile %d visited %d", N, M, left,
            right, causal, bm, bn, m0 / bm, t, visited);
    }
    for (int mw = m0; mw < m0 + bm; mw += 32) {      // the waves' 32-row slices
      int a, b;
      win_unmasked_tiles(len, nt, mw, 32, diff, dlo, bn, a, b);
      CHECK(0 <= a && a <= b && b <= nt, "unmasked [%d, %d) of %d", a, b, nt);
      for (int t = 0; t < nt; ++t) {
        const int j0 = k_lo + t * bn;
        if (t >= a && t < b) CHECK(all(mw, mw + 32, j0, j0 + bn), "N %d M %d (%d, %d) causal %d: rows %d.. key tile at %d runs unmasked", N, M, left, right, causal, mw, j0);
        // the kernels' skip tests (no valid pair for the wave) must never skip a visible pair
        const bool skip = (t * bn > mw + 31 + diff) || (t * bn + bn - 1 < mw + dlo);
        if (skip) CHECK(!any(mw, mw + 32, j0, j0 + bn), "N %d M %d (%d, %d): rows %d.. key tile at %d skipped", N, M, left, right, mw, j0);
      }
    }
  }
  // ---- dK/dV: key tiles of bnk keys, query tiles of bmq rows
  for (int n0 = 0; n0 < M; n0 += bnk) {
    int t0, t1;
    win_query_tiles(N, M, n0, bnk, lo, hi, bmq, t0, t1);
    CHECK(0 <= t0 && t0 <= t1 && t1 <= tile_count(N, bmq), "query tiles [%d, %d)", t0, t1);
    for (int t = 0; t < tile_count(N, bmq); ++t)
      CHECK((t >= t0 && t < t1) == any(t * bmq, (t + 1) * bmq, n0, n0 + bnk), "N %d M %d (%d, %d) causal %d bmq %d bnk %d: key tile %d query tile %d", N, M,
            left, right, causal, bmq, bnk, n0 / bnk, t);
    const int diff = M - N + hi, dlo = M - N - lo;
    for (int nw = n0; nw < n0 + bnk; nw += 32) {
      for (const int halves : {1, 2}) {      // (2: the query-split form, each wave half on its half of every staged tile)
        const int bms = bmq / halves;
        if (bms % 32 != 0) continue;
        for (int hq = 0; hq < bmq; hq += bms) {
          int a, b;
          win_unmasked_query_tiles(t0, t1, n0 + bnk <= M, nw, hq, bms, bmq, diff, dlo, a, b);
          CHECK(t0 <= a && a <= b && b <= t1, "unmasked query tiles [%d, %d) of [%d, %d)", a, b, t0, t1);
          for (int t = t0; t < t1; ++t) {
            const int i0 = t * bmq + hq;
            bool full = nw + 32 <= M;
            for (int i = i0; full && i < std::min(i0 + bms, N); ++i)
              for (int j = nw; j < nw + 32; ++j) full = full && vis[(size_t)i * M + j];
            if (t >= a && t < b) CHECK(full, "N %d M %d (%d, %d) causal %d: keys %d.. rows %d.. run unmasked", N, M, left, right, causal, nw, i0);
            const bool skip = (i0 + bms - 1 + diff < nw) || (i0 > nw + 31 - dlo);
            if (skip) {
              bool seen = false;
              for (int i = i0; i < std::min(i0 + bms, N); ++i)
                for (int j = nw; j < std::min(nw + 32, M); ++j) seen = seen || vis[(size_t)i * M + j];
              CHECK(!seen, "N %d M %d (%d, %d): keys %d.. rows %d.. skipped", N, M, left, right, nw, i0);
            }
          }
        }
      }
    }
  }
}

int main() {
  std::mt19937 rng(4321);
  const int lens[] = {1, 2, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 257, 300, 511, 512, 513, 777, 1000};
  const int bms[] = {128, 256}, bmqs[] = {32, 64, 128}, bnks[] = {128, 256};
  auto pick = [&](const auto& a) { return a[rng() % (sizeof(a) / sizeof(a[0]))]; };
  for (int it = 0; it < 3000; ++it) {
    const int N = it % 7 == 0 ? 1 + (int)(rng() % 900) : pick(lens), M = it % 5 == 0 ? 1 + (int)(rng() % 900) : pick(lens);
    const bool causal = (it & 1) != 0;
    // sides that hide nothing: unbounded, or past the problem's corner (causal: any right side)
    const int left = it % 3 == 0 ? -1 : M - 1 + (int)(rng() % 50), right = it % 4 == 0 ? -1 : causal ? (int)(rng() % 300) : N - 1 + (int)(rng() % 50);
    check_problem(N, M, left, right, causal, pick(bms), 64, pick(bmqs), pick(bnks));
  }
  std::printf("%ld checks ok\n", g_cases);
  return 0;
}
