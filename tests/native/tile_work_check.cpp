// Checks the tile-ownership functions of csrc/fcsa_dispatch.h on the CPU: which (batch*head, tile) pairs and which split window every
// workgroup of a row-tile (forward, dQ) or key-tile (dK/dV) launch owns.  Built and run by tests/test_dispatch_cpu.py with g++.
//   * block_work is a bijection from the grid [0, batch_heads * tile_pairs) onto (batch*head, pair);
//   * the passes of all pairs visit every tile exactly once, the heavy tile first;
//   * for every tile the split windows are disjoint and cover exactly what the tile sees: causal forward / dQ the keys up to the tile's
//     diagonal, causal dK/dV the query tiles from the diagonal down, non-causal everything.
// Prints the number of checked cases; exits 1 at the first failure.
#include <cstdio>
#include <cstdlib>
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

static const int kLens[] = {1, 2, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 257, 300, 511, 512, 513, 777, 1000,
                            1024, 1100, 2047, 2048, 3000, 4133};
static const int kTiles[] = {32, 64, 128, 256};
static const int kBh[] = {1, 2, 3, 5, 7, 8, 12, 16, 24, 40, 64};

// grid -> (bh, pair) is one-to-one and onto; the pairs' passes cover the tiles once, heavy first
static void check_pairs(int n_bh, int len, int tile, bool causal) {
  const int tiles = tile_count(len, tile), pairs = tile_pairs(tiles, causal);
  CHECK(tile_workgroups(n_bh, len, tile, causal) == (int64_t)n_bh * pairs, "bh %d len %d tile %d causal %d", n_bh, len, tile, causal);
  std::vector<int> seen((size_t)n_bh * pairs, 0);
  for (int id = 0; id < n_bh * pairs; ++id) {
    int bh = -1, pair = -1;
    block_work(id, n_bh, pairs, bh, pair);
    CHECK(bh >= 0 && bh < n_bh && pair >= 0 && pair < pairs, "id %d bh %d len %d tile %d causal %d", id, n_bh, len, tile, causal);
    CHECK(++seen[(size_t)bh * pairs + pair] == 1, "id %d bh %d len %d tile %d causal %d", id, n_bh, len, tile, causal);
  }
  for (const bool rows : {true, false}) {
    std::vector<int> visits(tiles, 0);
    for (int pr = 0; pr < pairs; ++pr) {
      const int np = pair_passes(tiles, pr, causal);
      CHECK(np == 1 || np == 2, "pair %d len %d tile %d", pr, len, tile);
      for (int pass = 0; pass < np; ++pass) {
        const int t = pass_tile(tiles, pr, pass, causal, rows);
        CHECK(t >= 0 && t < tiles, "pair %d pass %d len %d tile %d", pr, pass, len, tile);
        ++visits[t];
      }
      if (np == 2) {      // row tiles: the high one first; key tiles: the low one first
        const int t0 = pass_tile(tiles, pr, 0, causal, rows), t1 = pass_tile(tiles, pr, 1, causal, rows);
        CHECK(rows ? t0 > t1 : t0 < t1, "pair %d len %d tile %d rows %d", pr, len, tile, rows);
      }
    }
    for (int t = 0; t < tiles; ++t) CHECK(visits[t] == 1, "tile %d of %d visited %d times (len %d causal %d)", t, tiles, visits[t], len, causal);
  }
}

// forward / dQ: the keys each split of row tile [m0, m0 + bm) runs over; 64-key tiles as in the kernels
static void check_key_windows(int N, int M, int bm, bool causal, int splits) {
  const int bn = 64;
  for (int m0 = 0; m0 < N; m0 += bm) {
    std::vector<int> hits(M, 0);
    for (int s = 0; s < splits; ++s) {
      int lo = -1, len = -1;
      if (causal) key_split_causal(N, M, m0, bm, s, splits, bn, lo, len);
      else key_split(M, s, splits, bn, lo, len);
      CHECK(lo >= 0 && len >= 0 && (len == 0 || lo + len <= M), "N %d M %d m0 %d split %d/%d", N, M, m0, s, splits);
      // the kernel's key tiles over the window, and the causal mask of the tile's last row inside them
      const int nt = key_tiles(len, m0, bm, M - N - lo, causal, bn);
      CHECK(nt >= 0 && (nt == 0 || (nt - 1) * bn < len), "N %d M %d m0 %d split %d/%d nt %d", N, M, m0, s, splits, nt);
      for (int j = lo; j < lo + std::min(len, nt * bn); ++j)
        if (!causal || j <= m0 + bm - 1 + M - N) ++hits[j];
    }
    for (int j = 0; j < M; ++j) {
      const bool visible = !causal || j <= m0 + bm - 1 + M - N;
      CHECK(hits[j] == (visible ? 1 : 0), "key %d seen %d times: N %d M %d m0 %d bm %d causal %d splits %d", j, hits[j], N, M, m0, bm, causal, splits);
    }
  }
}

// dK/dV: the query tiles each split of key tile [n0, n0 + bnk) runs over
static void check_query_windows(int N, int M, int bnk, int bmq, bool causal, int splits) {
  const int qt = tile_count(N, bmq), diff = M - N;
  for (int n0 = 0; n0 < M; n0 += bnk) {
    std::vector<int> hits(qt, 0);
    for (int s = 0; s < splits; ++s) {
      int lo = -1, hi = -1;
      if (causal) query_split_causal(qt, diagonal_tile(n0, diff, bmq), s, splits, lo, hi);
      else query_split(qt, s, splits, lo, hi);
      CHECK(lo >= 0 && (hi <= lo || hi <= qt), "N %d M %d n0 %d split %d/%d", N, M, n0, s, splits);
      for (int t = lo; t < hi; ++t) ++hits[t];
    }
    // query i sees key j when j <= i + diff: the tile's first key n0 sees the most queries
    for (int t = 0; t < qt; ++t) {
      const bool visible = !causal || std::min(N, (t + 1) * bmq) - 1 >= n0 - diff;
      CHECK(hits[t] == (visible ? 1 : 0), "query tile %d seen %d times: N %d M %d n0 %d bnk %d bmq %d causal %d splits %d", t, hits[t], N, M,
            n0, bnk, bmq, causal, splits);
    }
  }
}

int main() {
  for (const bool causal : {false, true})
    for (const int tile : kTiles)
      for (const int len : kLens) {
        for (const int n_bh : kBh) check_pairs(n_bh, len, tile, causal);
        for (const int M : {len, len + 1, std::max(1, len - 1), len / 3 + 1, 2 * len + 7})      // diagonals off the tile grid by 1 too
          for (int splits = 1; splits <= 16; ++splits) {
            check_key_windows(len, M, tile, causal, splits);
            for (const int bmq : {32, 64, 128}) check_query_windows(len, M, tile, bmq, causal, splits);
          }
      }
  std::printf("ok %ld checks\n", g_cases);
  return 0;
}
