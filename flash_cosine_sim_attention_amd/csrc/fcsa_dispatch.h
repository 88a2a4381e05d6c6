// fcsa_dispatch.h -- which kernel form, and how many split workgroups, every problem gets, and which tiles each workgroup owns.  The
// launchers (fcsa_fwd.hip, fcsa_bwd.hip) and the C ABI (fcsa_capi.hip) ask these functions and carry out the answer; nothing else decides.
// Pure, and free of HIP: the CU count and the debug knobs are arguments (callers pass cu_count(), forward_wide128_mode(-1),
// kv_group_mode(-1)), so a g++ program can include it.  The kernels call the constexpr functions of the tile-ownership section.
// Sweep builds (-DFCSA_VAR_SPLIT_ENV, tools/form_sweep.py, split_sweep.py, split_fuzz.py) let environment variables override each choice;
// the product build reads none (sweep_env below is a constant -1 there).
#pragma once
#include <stdint.h>
#include <algorithm>
#include <cmath>

#include "../../include/fcsa.h"
#ifdef FCSA_VAR_SPLIT_ENV
#include "dev/fcsa_sweep_env.h"
namespace fcsa {
inline int sweep_env(const char* name) { return fcsa_dev::env_int(name); }      // -1: not set
constexpr bool kSweepBuild = true;
}  // namespace fcsa
#else
namespace fcsa {
constexpr int sweep_env(const char*) { return -1; }
constexpr bool kSweepBuild = false;
}  // namespace fcsa
#endif

namespace fcsa {

constexpr int kDq2WBytes = 128;      // row bytes D*ES up to which the dQ kernel runs its 8-wave form (two waves / SIMD, one workgroup per CU)
constexpr int kDkv2WBytes = 128;     // same for the dKV kernel

// ---- which forms are compiled (element size es, head dim D, bias) --------------------------------------------------------------------
// "Lean" form of the 32-rows-per-wave forward for 16-bit rows of 129 .. 256 bytes (D = 96, 128) without bias: nothing is prefetched
// across blocks -- K row fragments and V transposed fragments are requested per 32-key block, next to their MFMAs -- so the wave
// fits 256 registers and TWO waves share a SIMD (eight waves per CU), the partner hiding the LDS latency the prefetches hid.
// The round-2 form prefetched a whole tile's K fragments and ran one wave per SIMD at these widths (397 registers at D = 128);
// measured on MI355X (C3 at D = 128, profiles/r03_*): see DESIGN.md section 6.
// It only pays when two waves per SIMD are actually resident -- an 8-wave workgroup per CU, or two 4-wave workgroups -- so it is a
// kernel template parameter chosen at launch; small grids keep the prefetching one-wave form.
constexpr bool fwd_lean(int es, int D, bool bias) { return es == 2 && !bias && D * es > 128 && D * es <= 256; }
// Key-split forward (fwd_kernel<.., KSPLIT>): 128-row workgroups of 8 waves whose halves split the keys; 16-bit, bias launches up to D = 64
constexpr bool fwd_ksplit(int es, int D, bool bias) { return es == 2 && (!bias || D <= 64); }
// key-split forms of the backward kernels (bwd_dq_kernel<.., KSPLIT>, bwd_dkv_kernel<.., QSPLIT>): 16-bit, no bias
constexpr bool bwd_ksplit(int es, int D, bool bias) { return es == 2 && !bias && D <= 128; }
// Two waves per SIMD (<= 256 registers) for the dQ kernel (template parameter TWO): always for rows up to 128 bytes, and -- round 3 --
// for 16-bit rows up to 256 bytes (D = 96, 128) in the 4-wave form WHEN the grid puts two 128-row workgroups on every CU, whose waves
// then hide each other's LDS latency.  Those widths ran one wave per SIMD before (435 registers at D = 128), at ~40 % of what the same
// kernel reaches at D = 64; smaller grids still do (a lone wave is better off with the pipelined tile).
constexpr bool dq_can_two_waves(int es, int D) { return D * es <= (es == 2 ? 256 : 128); }
// Group-sweep dK/dV (grouped-query attention): compiled for the 8-wave forms of 16-bit D = 64 (pipelined ring tile) and D = 128 (lean
// tile), the forms choose_dkv picks for key grids that cover the chip.
constexpr bool dkv_has_sweep(int es, int D, bool bias) { return es == 2 && !bias && (D == 64 || D == 128); }
// fwd2_kernel (64 rows per wave, no bias / key mask / per-row shift): D = 32 in the product; sweep builds also time D = 16 and 64
constexpr bool fwd2_compiled(int es, int D) { return es == 2 && (D == 32 || (kSweepBuild && D <= 64)); }

// ---- forms -----------------------------------------------------------------------------------------------------------------------------
enum class FwdForm { Rows8, Lean8, KSplit8, Waves4, Fwd2, Fwd3 };     // 8-wave rows, 8-wave lean, key-split 8 waves, 4 waves, fwd2, fwd3
enum class DqForm { Waves4, Waves4Two, Waves8, KSplit8 };            // 4 waves, 4 waves two-wave tile, 8 waves, key-split 8 waves
enum class DkvForm { Waves4, Waves8, Lean8, QSplit8, Sweep };        // 4 waves, 8 waves, 8-wave lean, query-split 8 waves, group sweep

// ---- the work of one workgroup of a row-tile (forward, dQ) or key-tile (dK/dV) launch ------------------------------------------------
// The launchers' grids, the kernels' decoding of blockIdx and the cost model below all use these.  constexpr: the kernels call them too.
// Under causal masking a tile's work grows with its distance from the start of the diagonal, and a workgroup runs start to finish on one
// CU, so causal launches give each workgroup a PAIR of tiles (T-1-pair, pair): constant work per workgroup.  Non-causal: one tile each.
constexpr int tile_count(int len, int tile) { return (len + tile - 1) / tile; }
constexpr int tile_pairs(int tiles, int causal) { return causal ? (tiles + 1) / 2 : tiles; }
constexpr int pair_passes(int tiles, int pair, int causal) { return (causal && (tiles - 1 - pair) != pair) ? 2 : 1; }
// tile of pass `pass`, the heavy one first: row tiles (rows) the high tile T-1-pair, key tiles the low tile `pair`
constexpr int pass_tile(int tiles, int pair, int pass, int causal, bool rows) {
  return causal ? (rows ? (pass == 0 ? tiles - 1 - pair : pair) : (pass == 0 ? pair : tiles - 1 - pair)) : pair;
}

// block id -> (batch*head index, pair).  Blocks are dispatched round-robin over the 8 XCDs (block b -> XCD b % 8); keep all tiles of one
// (batch, head) on one XCD so its K/V (or Q/dO) panel stays in that XCD's private 4 MiB L2.  Pure speed choice: any placement is correct.
constexpr void block_work(int id, int n_bh, int pairs, int& bh, int& pair) {
  if ((n_bh & 7) == 0) {
    const int xcd = id & 7, slot = id >> 3;
    bh = (slot / pairs) * 8 + xcd;
    pair = slot % pairs;
  } else {
    bh = id / pairs;
    pair = id % pairs;
  }
}

// Split launches (gridDim.y = splits > 1): workgroup `split` sees only its window of the keys (forward, dQ: keys [lo, lo + len)) or of the
// query tiles (dK/dV: tiles [lo, hi), empty when hi <= lo).
// non-causal forward / dQ: the whole key range, in `bn`-key tiles
constexpr void key_split(int M, int split, int splits, int bn, int& lo, int& len) {
  const int tps = ((M + bn - 1) / bn + splits - 1) / splits;      // key tiles per split
  lo = split * tps * bn;
  len = std::max(std::min(lo + tps * bn, M) - lo, 0);
}
// causal forward / dQ: the keys [0, vis) of the row tile [m0, m0 + bm), up to its diagonal
constexpr void key_split_causal(int N, int M, int m0, int bm, int split, int splits, int bn, int& lo, int& len) {
  const int vis = std::max(std::min(m0 + bm + M - N, M), 0);
  const int tps = std::max(((vis + bn - 1) / bn + splits - 1) / splits, 1);
  lo = std::min(M, split * tps * bn);
  len = std::max(std::min(lo + tps * bn, M) - lo, 0);
}
// `bn`-key tiles the row tile [m0, m0 + bm) runs over a window of `len` keys; diff = M - N - (the window's first key)
constexpr int key_tiles(int len, int m0, int bm, int diff, int causal, int bn) {
  int last_key = len - 1;
  if (causal) last_key = std::min(m0 + bm - 1 + diff, last_key);
  return last_key < 0 ? 0 : last_key / bn + 1;
}
// dK/dV, non-causal: all `tiles` query tiles
constexpr void query_split(int tiles, int split, int splits, int& lo, int& hi) {
  const int tps = (tiles + splits - 1) / splits;      // query tiles per split
  lo = split * tps;
  hi = std::min(lo + tps, tiles);
}
// dK/dV, causal: the first query tile of size `bmq` the key tile from key n0 sees (diff = M - N) ...
constexpr int diagonal_tile(int n0, int diff, int bmq) { return std::max(n0 - diff, 0) / bmq; }
// ... and the query tiles [first, tiles) from there down
constexpr void query_split_causal(int tiles, int first, int split, int splits, int& lo, int& hi) {
  const int tps = std::max((tiles - first + splits - 1) / splits, 1);
  lo = std::min(first + split * tps, tiles);
  hi = std::min(lo + tps, tiles);
}

// Sliding-window launches (fcsa_forward_window / fcsa_backward_window): query i of N sees key j of M iff
//   i + (M - N) - lo <= j <= i + (M - N) + hi
// with lo / hi the normalised sides of the window (win_normalise: kWinOpen for an unbounded side).  The kernels run such a launch as a causal
// one whose diagonal is moved by `hi` (diff = M - N + hi; an open right side leaves nothing to mask there) plus a second, mirrored
// diagonal on the left: per row tile (key tile) the loop and the streams start at the band's first tile and end at its last, and only the
// tiles an edge crosses take the per-logit select.  The causal pairing of tiles (tile_pairs) is kept: a pair is two tiles of about
// lo + hi + tile positions each, so it neither helps nor hurts, and the grids, varlen_bind and block_work stay the ones of a causal launch.
constexpr int kWinOpen = 1 << 28;
// The host's normalisation (include/fcsa.h, fcsa_window): a side that reaches past the problem's corner -- right >= N - 1: query 0 sees key
// M - 1; left >= M - 1: query N - 1 sees key 0 -- is open; causal makes the right side 0.  Then (open, open) is the un-windowed problem and
// (open, 0) the causal one, which today's kernels serve; everything else is a windowed launch.
enum class WinKind { Full, Causal, Window };
constexpr WinKind win_normalise(int N, int M, bool causal, int left, int right, int& lo, int& hi) {
  hi = causal ? 0 : (right < 0 || right >= N - 1) ? kWinOpen : right;
  lo = (left < 0 || left >= M - 1) ? kWinOpen : left;
  return lo != kWinOpen ? WinKind::Window : hi == kWinOpen ? WinKind::Full : hi == 0 ? WinKind::Causal : WinKind::Window;
}
// forward / dQ: the keys [k_lo, k_lo + len) the row tile [m0, m0 + bm) runs over -- from the `bn`-key tile that holds the first key its
// first row sees to the last key its last row sees; len == 0: no row of the tile sees a key
constexpr void win_key_window(int N, int M, int m0, int bm, int lo, int hi, int bn, int& k_lo, int& len) {
  const int d = M - N, r1 = std::min(m0 + bm, N) - 1;
  const int first = std::max(m0 + d - lo, 0), last = std::min(r1 + d + hi, M - 1);
  k_lo = 0;
  len = 0;
  if (r1 < m0 || last < first) return;
  k_lo = first / bn * bn;
  len = last + 1 - k_lo;
}
// ... and of its `nt` tiles (numbered from k_lo) the range [a, b) that needs no select for the `rows` rows from row mw: whole tiles
// inside the window's keys, at or left of the first row's right edge (diff = M - N + hi - k_lo), at or right of the last row's left edge
// (dlo = M - N - lo - k_lo).  Tiles [0, a) and [b, nt) take the per-logit select.
constexpr void win_unmasked_tiles(int len, int nt, int mw, int rows, int diff, int dlo, int bn, int& a, int& b) {
  const int hi_t = std::min(len / bn, std::max(0, mw + diff + 1) / bn);
  const int edge = mw + rows - 1 + dlo;
  a = std::min(edge <= 0 ? 0 : (edge + bn - 1) / bn, nt);
  b = std::max(a, std::min(hi_t, nt));
}
// dK/dV: the query tiles [t0, t1) of `bmq` rows the key tile [n0, n0 + bnk) sees (empty: t0 == t1 == 0)
constexpr void win_query_tiles(int N, int M, int n0, int bnk, int lo, int hi, int bmq, int& t0, int& t1) {
  const int d = M - N, k1 = std::min(n0 + bnk, M) - 1;
  const int first = std::max(n0 - d - hi, 0), last = std::min(k1 - d + lo, N - 1);
  t0 = 0;
  t1 = 0;
  if (k1 < n0 || last < first) return;
  t0 = first / bmq;
  t1 = last / bmq + 1;
}
// ... and of those the range [a, b) that needs no select for the 32 keys from key nw against rows [hq, hq + bms) of every tile (whole:
// the key tile lies inside M): below the last key's right-edge diagonal (diff = M - N + hi), above the first key's left-edge one
// (dlo = M - N - lo).  Tiles [t0, a) and [b, t1) take the per-logit select.
constexpr void win_unmasked_query_tiles(int t0, int t1, bool whole, int nw, int hq, int bms, int bmq, int diff, int dlo, int& a, int& b) {
  a = t1;
  b = t1;
  if (!whole) return;
  a = std::min(t1, std::max(t0, (nw + 31 - diff - hq + bmq - 1) / bmq));
  const int64_t x = (int64_t)nw - dlo - hq - bms + 1;
  b = std::min<int64_t>(t1, std::max<int64_t>(a, x < 0 ? 0 : x / bmq + 1));
}
// Variable-length launches (packed sequences, fcsa_forward_varlen / fcsa_backward_varlen): sequence s owns the packed rows
// [cu[s], cu[s + 1]).  The grid is the dense one for (batch = sequences, len = max_len); each workgroup reads its sequence's two table
// entries and works on that span.  The span is clamped so that ANY table contents stay inside the `total` packed rows: a malformed table
// gives wrong rows, never an access outside the tensors.  lo / hi are the raw entries cu[s], cu[s + 1].
constexpr void seq_span(int64_t lo, int64_t hi, int total, int max_len, int& start, int& len) {
  const int64_t st = std::min(std::max(lo, (int64_t)0), (int64_t)total);
  const int64_t en = std::min(std::max(hi, st), (int64_t)total);
  start = (int)st;
  len = (int)std::min(en - st, (int64_t)std::max(max_len, 0));
}
// A workgroup of a variable-length launch whose pair index lies beyond its own sequence's tile pairs (the grid is sized by the longest
// sequence) has no work and exits at once
constexpr bool seq_pair_idle(int pair, int len, int tile, int causal) { return pair >= tile_pairs(tile_count(len, tile), causal); }

// ---- decoding against a key/value cache (fcsa_forward_kvcache, csrc/fcsa_decode.hip) ----------------------------------------------------
// One single-wave workgroup per (batch, K/V head, row tile, key split).  The rows of a tile are the G = H / Hk query heads x N queries
// of one K/V head (16 per tile, the M of mfma_f32_16x16x32), so each K/V byte leaves HBM once per row tile.  The key range of sequence b
// (its own L_b, read on the device) is cut into `splits` windows of whole 32-key blocks; an empty window writes a zero partial.
constexpr int kDecodeRows = 16;            // query rows per tile
constexpr int kDecodeBlock = 32;           // keys per step of the key loop
constexpr int kDecodeMaxSplits = 128;
constexpr int kDecodeWavesPerCu = 8;       // the grid aims at this many waves per CU
constexpr int decode_row_tiles(int groups_x_queries) { return (groups_x_queries + kDecodeRows - 1) / kDecodeRows; }
// fewest keys a split is given: 64 KiB of 16-bit K + V rows (128 keys at D = 128)
constexpr int decode_min_split_keys(int D) { return std::max(16384 / std::max(D, 1), kDecodeBlock); }
// Split count: enough workgroups for kDecodeWavesPerCu waves per CU, each split at least decode_min_split_keys(D) keys of the longest
// sequence (max_k), at most kDecodeMaxSplits.
inline int decode_splits(int64_t batch, int kv_heads, int row_tiles, int max_k, int D, int cus) {
  const int64_t base = batch * (int64_t)kv_heads * row_tiles;
  if (base <= 0 || max_k <= 0) return 1;
  int64_t s = ((int64_t)cus * kDecodeWavesPerCu + base - 1) / base;
  s = std::min<int64_t>(s, std::max(1, max_k / decode_min_split_keys(D)));
  s = std::min<int64_t>(s, kDecodeMaxSplits);
  return (int)std::max<int64_t>(s, 1);
}
// Window of split `split` over a sequence of `len` keys: [lo, lo + n), whole 32-key blocks except at the sequence's end.
constexpr void decode_window(int len, int split, int splits, int& lo, int& n) {
  const int per = (std::max(len, 0) + splits - 1) / std::max(splits, 1);
  const int chunk = (per + kDecodeBlock - 1) / kDecodeBlock * kDecodeBlock;
  lo = std::min(split * chunk, std::max(len, 0));
  n = std::max(std::min(lo + chunk, len) - lo, 0);
}
// Cached positions of a sequence after the append, from the raw device table entry (NULL table: every sequence full)
constexpr int decode_len(bool has_table, int64_t cached, int new_len, int capacity) {
  const int64_t c = has_table ? std::min<int64_t>(std::max<int64_t>(cached, 0), capacity) : capacity;
  return (int)std::min<int64_t>(c + std::max(new_len, 0), capacity);
}
// l2norm groups the decode kernel reduces in registers, across the four lanes of a row: one group, or `D / groups` features dividing the
// lane's fragment of `unit` elements (8 for 16-bit, 4 for float32), or that fragment times a power of two.  Every other width (only
// possible at D = 96: 48, 24, 12, 6 or 3 features) takes the kernel form that sums each group's squares through LDS.
constexpr bool decode_groups_fast(int D, int groups, int unit) {
  if (groups < 1 || D % groups != 0) return false;
  const int gs = D / groups;
  if (groups == 1 || unit % gs == 0) return true;
  if (gs % unit != 0) return false;
  const int u = gs / unit;
  return (u & (u - 1)) == 0;
}

// Sliding window (win_normalise: lo keys to the left): the N queries of a sequence of `len` keys are its last N positions, so its rows read
// the keys from win_decode_first on (a whole 32-key block boundary), and the split count is sized by the keys a sequence can read
constexpr int win_decode_first(int len, int N, int lo) {
  return lo >= kWinOpen ? 0 : std::max(len - N - lo, 0) / kDecodeBlock * kDecodeBlock;
}
constexpr int win_decode_keys(int max_k, int N, int lo) {
  return lo >= kWinOpen ? max_k : (int)std::min<int64_t>(max_k, (int64_t)lo + N + kDecodeBlock - 1);
}

// Ragged decode steps (fcsa_forward_kvcache_varlen): sequence b brings N_b = cu[b + 1] - cu[b] packed query rows, so a K/V head of it has
// ceil(G * N_b / 16) row tiles.  The grid has ragged_slots(total_q, B, G) = floor(G * total_q / 16) + B flat tile slots per K/V head, and
// sequence b's tiles sit from slot ragged_base(cu[b], b, G) = floor(G * cu[b] / 16) + b on.  Consecutive bases differ by
// floor(G cu[b + 1] / 16) - floor(G cu[b] / 16) + 1 >= floor(G N_b / 16) + 1 >= ceil(G N_b / 16): the tiles of a sequence never reach the next
// base, and the bases grow strictly with b, so a workgroup finds its sequence by a binary search over the table alone (no prefix sums, no
// prologue launch); a slot between a sequence's last tile and the next base is idle (at most B of them, one per sequence).
// Table entries are clamped into [0, total] (ragged_cu), so ANY table contents keep every row index inside the packed tensors.
constexpr int64_t ragged_cu(int64_t raw, int64_t total) { return std::min(std::max(raw, (int64_t)0), total); }
constexpr int64_t ragged_base(int64_t cu_b, int b, int G) { return (int64_t)G * cu_b / kDecodeRows + b; }
constexpr int64_t ragged_slots(int64_t total_q, int64_t B, int G) { return (int64_t)G * total_q / kDecodeRows + B; }
// The sequence that owns packed row `tok`: the last b with cu[b] <= tok (empty sequences share their start with the next one and own
// nothing).  B >= 1.
constexpr int ragged_seq_of(const int32_t* cu, int B, int64_t total, int64_t tok) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (ragged_cu(cu[mid], total) <= tok) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// Slot -> (sequence b, row tile rt of its G * len rows, first packed row `start`, rows `len`); false: the slot is idle.  B >= 1.
constexpr bool ragged_tile(const int32_t* cu, int B, int64_t total, int G, int64_t slot, int& b, int& rt, int& start, int& len) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (ragged_base(ragged_cu(cu[mid], total), mid, G) <= slot) lo = mid; else hi = mid - 1;
  }
  const int64_t st = ragged_cu(cu[lo], total), en = std::max(ragged_cu(cu[lo + 1], total), st);
  const int64_t t = slot - ragged_base(st, lo, G);
  b = lo;
  start = (int)st;
  len = (int)(en - st);
  rt = (int)t;
  return t >= 0 && t < ((int64_t)G * (en - st) + kDecodeRows - 1) / kDecodeRows;
}

// Prefill against the cache (fcsa_forward_kvcache_prefill, csrc/fcsa_prefill.hip): the same flat slots with the tile height `rows` as a
// parameter (kPrefillRows for the kernel).  The argument above holds for any height: consecutive bases differ by at least
// floor(G N_b / rows) + 1 >= ceil(G N_b / rows).  The rows of a sequence's K/V head are ordered TOKEN-major here, r = i * G + g, so a tile
// covers consecutive tokens and its causal key range is tight.
constexpr int kPrefillRows = 128;          // query rows per workgroup: 4 waves x 2 MFMA tiles of 16
constexpr int kPrefillStage = 64;          // keys per LDS stage (two 32-key blocks of the decode key loop)
constexpr int64_t prefill_base(int64_t cu_b, int b, int G, int rows) { return (int64_t)G * cu_b / rows + b; }
constexpr int64_t prefill_slots(int64_t total_q, int64_t B, int G, int rows) { return (int64_t)G * total_q / rows + B; }
// Slot -> (sequence b, row tile rt of its G * len rows, first packed row `start`, rows `len`); false: the slot is idle.  B >= 1.
constexpr bool prefill_tile(const int32_t* cu, int B, int64_t total, int G, int rows, int64_t slot, int& b, int& rt, int& start, int& len) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (prefill_base(ragged_cu(cu[mid], total), mid, G, rows) <= slot) lo = mid; else hi = mid - 1;
  }
  const int64_t st = ragged_cu(cu[lo], total), en = std::max(ragged_cu(cu[lo + 1], total), st);
  const int64_t t = slot - prefill_base(st, lo, G, rows);
  b = lo;
  start = (int)st;
  len = (int)(en - st);
  rt = (int)t;
  return t >= 0 && t < ((int64_t)G * (en - st) + rows - 1) / rows;
}
// The key range [0, kend) that the rows [first, first + count) of a sequence's K/V head visit (token-major rows, N tokens against L cached
// positions): every key without `causal`; under it, one past the last key visible to the last token among the rows (bottom-right
// alignment: token i sees keys j <= L - N + i), clamped to [0, L].  Rows at or beyond G * N do not count.
constexpr int prefill_kend(int L, int N, int G, int64_t first, int count, bool causal) {
  const int64_t last = std::min(first + count, (int64_t)G * N) - 1;
  if (last < first || L <= 0) return 0;
  if (!causal) return L;
  return (int)std::min<int64_t>(std::max<int64_t>((int64_t)L - N + last / G + 1, 0), L);
}
// Under a sliding window (the ragged kernel's sides: lo / hi keys left / right of a token's own position, kWinOpen for an open side, causal
// as hi = 0) the same rows visit [prefill_kstart, prefill_win_kend).  The start is the first key the first token among the rows sees,
// rounded down to a whole LDS stage, so the 32-key blocks a tile walks are the absolute ones the ragged kernel walks from win_decode_first
// (a multiple of 32).  The end is prefill_kend's under an open or causal right side, and one past the last key the last token sees otherwise.
constexpr int prefill_kstart(int L, int N, int G, int64_t first, int lo) {
  if (lo >= kWinOpen) return 0;
  return (int)(std::max<int64_t>((int64_t)L - N + first / G - lo, 0) / kPrefillStage * kPrefillStage);
}
constexpr int prefill_win_kend(int L, int N, int G, int64_t first, int count, int hi) {
  if (hi >= kWinOpen || hi == 0) return prefill_kend(L, N, G, first, count, hi == 0);
  const int64_t last = std::min(first + count, (int64_t)G * N) - 1;
  if (last < first || L <= 0) return 0;
  return (int)std::min<int64_t>(std::max<int64_t>((int64_t)L - N + last / G + hi + 1, 0), L);
}
// An engine step (fcsa_forward_kvcache_step): a sequence of N rows takes the chunk kernel iff G * N >= chunk_rows, the decode kernels
// otherwise.  Both sides evaluate this one function on the N their tile maps give them (ragged_tile, prefill_tile: the same clamped entries).
constexpr bool step_is_chunk(int G, int64_t N, int chunk_rows) { return (int64_t)G * N >= chunk_rows; }
constexpr int kStepChunkRows = 1024;       // the default threshold: G * N_b of eight 128-row tiles (profiles/step_ab.txt)

// ---- log-sum-exp of a decoded row, and merging attention states (fcsa_forward_kvcache_lse, fcsa_merge_states) --------------------------
// The two functions below call expf / log / log2, which are no constant expressions: they are host functions for the C++ compiler
// (tests/native/merge_states_check.cpp) and host + device functions for hipcc (decode_combine_lse*, merge_states_kernel).
#if defined(__HIPCC__)
#define FCSA_HOST_DEVICE __host__ __device__
#else
#define FCSA_HOST_DEVICE
#endif
constexpr int kMergeMaxStates = 8;
// Natural-log LSE of a row from what the decode combine holds: M (the row's exponent reference in log2 units: its reconciled max, or the
// constant shift) and l = sum 2^(s - M) over the visible keys, UNCLAMPED.  sum exp(s_nat) = 2^M * l, so lse = ln 2 * (M + log2 l); a row
// without a visible key (M == -inf, or l == 0 under the constant shift) is -inf exactly, never NaN.  Once per row, so in double.
FCSA_HOST_DEVICE inline float decode_row_lse(float M, float l) {
  if (!(M > -INFINITY) || !(l > 0.f)) return -INFINITY;
  return (float)(0.6931471805599453 * ((double)M + log2((double)l)));
}
// Weights of S attention states of one row (S <= kMergeMaxStates): M = max_s lse[s]; every state empty (M == -inf): all weights 0,
// lse_out = -inf, returns 0.  Else w[s] = exp(lse[s] - M) -- exactly 0 for an empty state -- and lse_out = M + log(W) with W = sum_s w[s],
// which is returned.  The caller forms o = (sum over the states with w[s] != 0 of w[s] * o_s) / W: a state of weight 0 is SKIPPED, not
// multiplied, so whatever its o_s holds (NaN included) cannot leak.  One state, or one state beside empty ones: w = 1, W = 1, so o and lse
// come back bit for bit.
FCSA_HOST_DEVICE inline float merge_row_weights(const float* lse, int S, float* w, float& lse_out) {
  float M = -INFINITY;
  for (int s = 0; s < S; ++s) M = lse[s] > M ? lse[s] : M;
  if (!(M > -INFINITY)) {
    for (int s = 0; s < S; ++s) w[s] = 0.f;
    lse_out = -INFINITY;
    return 0.f;
  }
  float W = 0.f;
  for (int s = 0; s < S; ++s) {
    w[s] = lse[s] > -INFINITY ? expf(lse[s] - M) : 0.f;
    W += w[s];
  }
  lse_out = M + logf(W);
  return W;
}

// workgroups of `tile`-position tiles over `len` positions for `batch_heads` (batch x heads)
inline int64_t tile_workgroups(int64_t batch_heads, int len, int tile, bool causal) {
  return batch_heads * tile_pairs(tile_count(len, tile), causal);
}

// Waves per workgroup of the row-tile (key-tile) kernels: 8 (one 256-position workgroup per CU) when that still gives every CU a
// workgroup, else 4 (two 128-position workgroups per CU).  Both keep two waves per SIMD; with 8 the K / V (Q / dO) tiles are staged once
// per CU instead of twice, i.e. half the global loads and LDS stores per wave (C3: forward -6%).
// tail: the last-round rule below -- 1 for the forward and dK/dV, 2 for dQ, 0 none
inline int tile_waves(int64_t batch_heads, int len, bool causal, bool bits16, int tail, int cus) {
  const int64_t w256 = tile_workgroups(batch_heads, len, 256, causal);
  // More 256-position workgroups than CUs, 16-bit (round 6, profiles/r06_form_sweep_big*.txt): the LAST round decides.  A last round that
  // fills at most ~55 % of the CUs costs the 8-wave form a whole 256-position workgroup time; as 4-wave workgroups (two per CU) the same
  // tail is 128-position workgroups running alone on their CUs: forward (rows <= 128 bytes) -4 ... -11 % at 264 ... 384 and 544 ... 640
  // workgroups on 256 CUs, -6 ... -8 % at 800 and 1088; dK/dV -5 ... -9 % at the same counts (D = 128 lean form against the pipelined
  // 4-wave form: -8 ... -12 % at 264 ... 352).  Full or nearly full last rounds (C3: exactly 256) keep the 8-wave form.  dQ: the 4-wave
  // form wins whenever the last round is not full (-3 ... -25 %); with whole rounds the 8-wave form is ahead (C3, one round: 6 %;
  // (8,8,4096,64) causal, two rounds: 4 %, profiles/r06_ab_forms_tail.txt).
  if (bits16 && tail != 0 && w256 > cus) {
    const int64_t rem = w256 % cus;
    if (tail == 2) return rem != 0 ? 4 : 8;
    return (rem != 0 && rem * 20 <= (int64_t)cus * 11) ? 4 : 8;
  }
  if (w256 >= cus * 7 / 8) return 8;
  // 16-bit types (round 6, tools/form_sweep.py): once the 128-position tiles outnumber the CUs -- where the key-split 8-wave forms would
  // need a second round of workgroups -- the 256-position 8-wave workgroup wins from 132 workgroups on 256 CUs up, not only from 7/8 of
  // the CUs: rows <= 128 bytes forward (against two 4-wave workgroups per CU) -5 ... -9 %, dQ -3 ... -10 %, dK/dV -10 ... -20 %
  // (profiles/r06_form_sweep_d64_b.txt); D = 96 / 128 lean forward against the key-split form -25 ... -35 %, lean dK/dV -15 ... -20 %
  // (profiles/r06_form_sweep_d128_b.txt)
  if (bits16 && tile_workgroups(batch_heads, len, 128, causal) > cus) return 8;
  return 4;
}

// The key-split forward where it is compiled: rows wider than 128 bytes always (the 4-wave form runs one wave per SIMD there whatever the
// grid), narrower rows while its workgroups (128-row tiles x splits) fit one round
inline bool fwd_ksplit_pays(int es, int D, int64_t workgroups, int cus) { return D * es > 128 || workgroups <= cus; }

// ---- forward -------------------------------------------------------------------------------------------------------------------------
struct FwdProblem {
  int es, D;
  int64_t batch_heads;
  int N, M;
  bool causal, bias, mask, dyn;
  int splits;
  int64_t q_row_bytes, k_row_bytes, v_row_bytes;      // row strides of q, k, v (the 32-bit offsets of fwd3)
  int wide128_mode;                                   // fcsa_debug_forward_form: 0 = never fwd3
  bool varlen = false;                                // packed sequences (seq_span), sliding window: no Fwd2 / Fwd3, no key split
};

// fwd3_kernel (fcsa_fwd3.hip): 16-bit D = 128, static exponent shift, no bias, no key mask, no key split, a grid of 256-row (causal: paired)
// workgroups that covers the chip -- or, from 2048 keys, more than half of it -- K / V slices addressable with 32-bit offsets.
inline bool fwd3_applies(const FwdProblem& f, int cus) {
  if (f.D != 128 || f.es != 2 || f.bias || f.mask || f.dyn || f.splits > 1 || f.wide128_mode == 0) return false;
  if (tile_workgroups(f.batch_heads, f.N, 256, f.causal) < cus * 7 / 8) {
    // round 6 (tools/form_sweep.py, profiles/r06_form_sweep_d128_b.txt): also where the 128-row tiles outnumber the CUs (132 ... 223 of
    // these workgroups on 256 CUs) and the pass is long enough for its prologue: 31 - 36 % faster than the key-split lean form there, and
    // ahead of the 256-row lean form from 2048 keys (level at 1024 keys up to ~176 workgroups, behind beyond)
    if (tile_workgroups(f.batch_heads, f.N, 128, f.causal) <= cus || f.M < 2048) return false;
  }
  if ((int64_t)(f.M + 64 * 6) * f.k_row_bytes >= 0x7fffffffLL || (int64_t)(f.M + 64 * 6) * f.v_row_bytes >= 0x7fffffffLL) return false;
  return (int64_t)(f.N + 256) * f.q_row_bytes < 0x7fffffffLL;
}

// fwd2_kernel against the 32-row kernel (measured on MI355X, bf16, B4 H8: tools/fwd_ab.py, tools/form_sweep.py).  It needs enough 256-row
// workgroups to cover the 256 CUs.  Rounds 2 - 3 measured it ahead where the MFMA share of a tile is large or the sequence is long
// (D = 32 / 64 non-causal: +3..22%; causal N = 8192: +5%; D = 96 against the ONE-wave narrow kernel of round 2: +25..34%); with causal
// masking and short sequences its 256-row diagonal granularity costs more than the halved LDS traffic saves (N = 4096: -6%, N = 1024:
// -20%).  Round 6 (tools/form_sweep.py, profiles/r06_form_sweep_*.txt): since round 4 (row sums on the VALU, LDS-DMA staging) the 32-row
// kernel at two waves per SIMD beats this one at D = 64 -- non-causal (4,8,4096) 135 vs 156 us, (8,8,2048) 74 vs 88, causal (4,8,8192)
// 273 vs 324 -- and at D = 16 (causal 8192: 155 vs 165); at D = 32 this kernel still wins on long key ranges (causal (4,8,8192) 183 vs
// 198, non-causal (2,8,8192) 172 vs 178; level at 2048 - 4096 keys, 7 % behind at 1024).  D = 96: the lean two-wave kernel (round 3).
inline bool fwd2_applies(const FwdProblem& f) {
  if (f.es != 2 || f.D != 32 || f.bias || f.dyn || f.splits > 1 || f.mask) return false;
  if (tile_workgroups(f.batch_heads, f.N, 256, f.causal) < 224) return false;
  return f.causal ? f.N >= 8192 : f.M >= 4096;
}

// Sweep builds: FCSA_FWD_FORM = 1 row tiles of 8 waves (16-bit D = 96 / 128: lean), 2 key-split 8 waves, 3 four waves, 4 the 64-rows-per-wave
// kernel (16-bit D <= 64), 5 the D = 128 64-rows-per-wave kernel whatever the grid; any value > 0 rules out the automatic fwd2 / fwd3.
// FCSA_KSPLIT = 0 / 1 forces the key-split form off / on where it is compiled.
inline FwdForm choose_forward(const FwdProblem& f, int cus) {
  const int env = sweep_env("FCSA_FWD_FORM"), env_ks = sweep_env("FCSA_KSPLIT");
  const bool plain = !f.bias && !f.mask && !f.dyn && f.splits <= 1 && !f.varlen;
  if (f.varlen) {
    // packed sequences: the 32-rows-per-wave forms only, the same rules (the caller never splits them: f.splits == 1)
  } else if (env > 0) {
    if (env == 5 && f.D == 128 && f.es == 2 && plain) return FwdForm::Fwd3;
    if (env == 4 && fwd2_compiled(f.es, f.D) && plain) return FwdForm::Fwd2;
  } else {
    if (fwd3_applies(f, cus)) return FwdForm::Fwd3;
    if (fwd2_applies(f)) return FwdForm::Fwd2;
  }
  const bool narrow = f.D * f.es <= 128, lean = fwd_lean(f.es, f.D, f.bias);
  const bool ksplit = fwd_ksplit(f.es, f.D, f.bias) &&
      (env_ks >= 0 ? env_ks != 0 : fwd_ksplit_pays(f.es, f.D, tile_workgroups(f.batch_heads, f.N, 128, f.causal) * std::max(f.splits, 1), cus));
  if (!f.dyn && f.splits > 1) return ksplit ? FwdForm::KSplit8 : FwdForm::Waves4;      // split-key path: 128-row tiles x key ranges
  if (!f.dyn && fwd_ksplit(f.es, f.D, f.bias) && (narrow || lean) && env >= 1 && env <= 3)
    return env == 1 ? (narrow ? FwdForm::Rows8 : FwdForm::Lean8) : env == 2 ? FwdForm::KSplit8 : FwdForm::Waves4;
  // rows <= 128 bytes: two waves per SIMD whatever the grid (<= 256 registers with all prefetches); the lean form needs its partner wave:
  // one 8-wave workgroup per CU (a grid with two 4-wave workgroups per CU always has that)
  if (narrow && tile_waves(f.batch_heads, f.N, f.causal, f.es == 2, 1, cus) == 8) return FwdForm::Rows8;
  if (!narrow && lean && tile_waves(f.batch_heads, f.N, f.causal, true, 0, cus) == 8) return FwdForm::Lean8;
  return ksplit ? FwdForm::KSplit8 : FwdForm::Waves4;
}

// ---- dQ ------------------------------------------------------------------------------------------------------------------------------
struct BwdProblem {
  int es, D;
  int64_t batch_heads;
  int N, M;
  bool causal, bias;
  int splits;           // dq_splits / dkv_splits of the launch
  bool kv_sweep;        // the dK/dV launch runs the group sweep (dkv_sweep below, decided by the C ABI)
  bool varlen = false;  // packed sequences (seq_span), sliding window: never a split form or the group sweep
  bool window = false;  // sliding window (the windowed kernel entry points)
};

// Sweep builds: FCSA_DQ_FORM = 1 row tiles of 8 waves (16-bit D = 96 / 128: four waves, two-wave tile), 2 key-split 8 waves (D = 96 / 128:
// causal only), 3 four waves
inline DqForm choose_dq(const BwdProblem& b, int cus) {
  if (b.splits > 1 && !b.varlen) return DqForm::Waves4;       // split-key path: 128-row tiles x key ranges (the key-split form measured level there)
  const bool narrow = b.D * b.es <= kDq2WBytes, two = dq_can_two_waves(b.es, b.D) && !b.bias;
  // sliding window, rows wider than 128 bytes: the one-wave pipelined form.  The two-wave tile sits at its 256 registers there, and with the
  // window's second diagonal and third loop segment it spills into the tile loops (16-bit D = 128: 240 registers to scratch, the
  // backward twice the time per tile of the dense causal call, profiles/window_ab.txt)
  if (b.window && !narrow) return DqForm::Waves4;
  if (const int env = sweep_env("FCSA_DQ_FORM"); bwd_ksplit(b.es, b.D, b.bias) && (narrow || two)) {
    if (env == 1) return narrow ? DqForm::Waves8 : DqForm::Waves4Two;
    if (env == 2 && (narrow || b.causal)) return DqForm::KSplit8;
    if (env == 3) return DqForm::Waves4;
  }
  const int64_t wgs128 = tile_workgroups(b.batch_heads, b.N, 128, b.causal);
  if (narrow) {
    if (tile_waves(b.batch_heads, b.N, b.causal, b.es == 2, 2, cus) == 8) return DqForm::Waves8;
    // at most one 128-row workgroup per CU: its wave halves split the keys
    if (bwd_ksplit(b.es, b.D, false) && wgs128 <= cus) return DqForm::KSplit8;
  } else if (two) {
    // two waves per SIMD need two 128-row workgroups on every CU; smaller grids keep the one-wave (pipelined) form
    // (bias launches keep the one-wave form too: their two-wave instantiation spills 17 registers and was never measured ahead)
    // (round 6: from MORE 128-row workgroups than CUs on -- rounds 3 - 5 asked for 7/4 of the CUs; at 264 ... 416 workgroups on 256 CUs the
    //  two-wave tile is 19 - 28 % faster than the one-wave and key-split forms: profiles/r06_form_sweep_d128_b.txt)
    if (wgs128 > cus) return DqForm::Waves4Two;
    // fewer: the same tile, 8 waves on 128 rows.  Causal launches only: 256-byte rows have no non-causal instantiation of the two-wave tile
    // (GENERAL_ONLY in launch_dq_nw), and the general one measured +6 % there against the one-wave pipelined form
    if (bwd_ksplit(b.es, b.D, b.bias) && b.causal) return DqForm::KSplit8;
  }
  return DqForm::Waves4;
}

// ---- dK / dV -------------------------------------------------------------------------------------------------------------------------
// Grouped-query K/V: the group sweep takes a problem where it is compiled and its grid -- batch x K/V heads x 256-key tiles -- gets the 8-wave
// form by the rule above (mode, fcsa_debug_kv_group_form: 0 never, 1 by that rule, 2 wherever compiled)
inline bool dkv_sweep(int es, int D, int64_t batch_kv_heads, int M, bool causal, int mode, int cus) {
  if (!dkv_has_sweep(es, D, false) || mode <= 0) return false;
  return mode >= 2 || tile_waves(batch_kv_heads, M, causal, true, 1, cus) == 8;
}

// Sweep builds: FCSA_DKV_FORM = 1 key tiles of 8 waves (16-bit D = 96 / 128: lean), 2 query-split 8 waves (D <= 64), 3 four waves
inline DkvForm choose_dkv(const BwdProblem& b, int cus) {
  if (b.kv_sweep && !b.varlen) return DkvForm::Sweep;
  if (b.splits > 1 && !b.varlen) return DkvForm::Waves4;      // split-query path: 128-key tiles x query ranges
  const bool narrow = b.D * b.es <= kDkv2WBytes, lean = b.es == 2 && !b.bias && !narrow && b.D * b.es <= 256;
  if (const int env = sweep_env("FCSA_DKV_FORM"); (narrow && bwd_ksplit(b.es, b.D, b.bias)) || lean) {
    if (env == 1) return narrow ? DkvForm::Waves8 : DkvForm::Lean8;
    if (env == 2 && narrow) return DkvForm::QSplit8;
    if (env == 3) return DkvForm::Waves4;
  }
  if (narrow) {
    if (tile_waves(b.batch_heads, b.M, b.causal, b.es == 2, 1, cus) == 8) return DkvForm::Waves8;
    // at most one 128-key workgroup per CU: its wave halves split the queries (from 512 queries: below, the four or fewer 128-row tiles of
    // a pass do not pay for the hand-over -- 23.5 vs 24.7 us at N = 333 / 777)
    if (bwd_ksplit(b.es, b.D, false) && b.N >= 512 && tile_workgroups(b.batch_heads, b.M, 128, b.causal) <= cus) return DkvForm::QSplit8;
  } else if (lean) {
    // lean form (two waves per SIMD, V fragments from the LDS) where an 8-wave workgroup per CU still covers the chip; smaller grids keep
    // the one-wave pipelined form.  (Two 4-wave workgroups per CU would do as well, but a grid with >= 448 of those always has >= 224 of
    // the 8-wave ones.)
    if (tile_waves(b.batch_heads, b.M, b.causal, true, 1, cus) == 8) return DkvForm::Lean8;
  }
  return DkvForm::Waves4;
}

// ---- split counts (forward keys / dQ keys / dK-dV queries) -------------------------------------------------------------------------
// Where a problem's 128-position tiles (causal, since round 6: PAIRS of tiles) cannot fill the chip, several workgroups share one tile's
// loop range and write f32 partials that a second pass (fwd_combine_kernel / finalize) sums.  How many: rounds 2 - 5 took "enough
// workgroups for two per CU"; since round 6 the count is the argmin of a small cost model over s = 1 .. 16 (16-bit types; float32 keeps
// the old rule).  The model prices, in microseconds on MI355X, what a launch with s splits costs:
//   * the form the launchers run for that count: form A = the 8-wave one-workgroup-per-CU forms (forward: wave halves split the keys,
//     fwd_ksplit_pays; backward: whatever runs un-split), else 4-wave workgroups, one per CU (form B) or -- rows <= 128 bytes and more
//     workgroups than CUs -- two per CU (form C);
//   * a workgroup's time t0 + c * positions, t0 and c growing with D (the exponentials do not shrink with it: floor);
//   * rounds of workgroups over the slots, a partly filled last round at alpha + (1 - alpha) * fill;
//   * the second pass: a launch + s partial slabs read once.
// Constants: least squares in log space over tools/split_sweep.py tables of 27 shapes x 7 counts per kernel, D = 16 .. 128
// (profiles/r06_split_sweep_*.txt; tools/split_model_fit.py prints them and the table below).  Mean / worst regret of the model's choice
// against the measured best: forward 0.9 / 10.9 %, dQ 0.3 / 4.5 %, dK/dV 0.2 / 3.6 %; the rule it replaces: 11.2 / 44 %, 8.9 / 42 %,
// 11.8 / 52 % (it split 160 .. 224 tiles of a 2048-position problem three or four ways where the un-split 8-wave form is 30 - 50 %
// faster, and took counts that leave a quarter-full last round).  The ONE definition both the workspace sizes and the launches use.
struct SplitModel { double tA, cA, tB, cB, tC, cC, a0, b0, k0, k1, alpha; int slabs, extra; };
constexpr SplitModel kSplitFwd = {5.57, 8.68, 3.61, 11.8, 5.77, 16.1, 0.0, 0.536, 7.77, 0.177, 0.585, 1, 1};
constexpr SplitModel kSplitDq  = {11.3, 9.94, 2.35, 12.5, 1.0, 20.9, 0.369, 0.244, 12.2, 0.455, 0.526, 1, 0};
constexpr SplitModel kSplitDkv = {11.5, 12.0, 2.25, 15.5, 1.0, 26.6, 0.11, 0.281, 13.5, 0.34, 0.528, 2, 0};
// tiles: 128-position tiles the un-split grid has; rows: rows of ONE partial slab; len: positions the split loop runs over
inline double split_cost(const SplitModel& m, int D, int64_t tiles, int64_t rows, int len, int s, int cus, bool form_a) {
  const bool wide = D * 2 > 128;
  const double ft = m.a0 + (1.0 - m.a0) * D / 64.0, fc = m.b0 + (1.0 - m.b0) * std::max(0.44, D / 64.0);
  const int64_t tot = tiles * s;
  double t0 = m.tA, c = m.cA;
  int64_t slots = cus;
  if (!form_a) {
    if (wide || tot <= cus) { t0 = m.tB; c = m.cB; }
    else { t0 = m.tC; c = m.cC; slots = 2 * (int64_t)cus; }
  }
  const double per = t0 * ft + c * fc * ((double)len / s) / 1024.0;
  const int64_t full = tot / slots, rem = tot % slots;
  const double rounds = full == 0 ? 1.0 : (double)full + (rem == 0 ? 0.0 : m.alpha + (1.0 - m.alpha) * (double)rem / (double)slots);
  const double second = s == 1 ? 0.0 : m.k0 + m.k1 * m.slabs * (double)s * (double)rows * (D + m.extra) * 4.0 / 1e6;
  return rounds * per + second;
}
// 16-bit problems.  fwd: a split forward runs the key-split form where choose_forward takes it, else 4-wave workgroups; the backward's
// split launches always run 4-wave workgroups (un-split = form A)
inline int best_split(const SplitModel& m, bool fwd, int D, int64_t tiles, int64_t rows, int len, int cus) {
  if (tiles <= 0 || tiles >= cus) return 1;
  int best = 1;
  double best_cost = split_cost(m, D, tiles, rows, len, 1, cus, true);
  for (int s = 2; s <= 16 && len / s >= 512; ++s) {
    const bool form_a = fwd && fwd_ksplit(2, D, false) && fwd_ksplit_pays(2, D, tiles * s, cus);
    const double cost = split_cost(m, D, tiles, rows, len, s, cus, form_a);
    if (cost < best_cost) { best_cost = cost; best = s; }
  }
  return best;
}
// the rule of rounds 2 - 5, still used for float32: two 4-wave workgroups per CU where those run two waves per SIMD (rows <= 128 bytes)
inline int split_by_target(const fcsa_problem& p, int64_t wgs, int len, int cus) {
  const int target = ((p.dtype == FCSA_F32 ? 4 : 2) * p.dim_head <= 128 ? 2 : 1) * cus;
  if (wgs <= 0 || wgs >= target / 2) return 1;
  int64_t s = (target + wgs - 1) / wgs;
  if (s > 16) s = 16;
  if (s > len / 512) s = len / 512;
  return s >= 2 ? (int)s : 1;
}
// sweep builds: FCSA_SPLITS / FCSA_DQ_SPLITS / FCSA_DKV_SPLITS = the count, clamped to 16 and to 64 positions per split
inline int sweep_splits(const char* name, int len) {
  const int v = sweep_env(name);
  return v >= 1 ? std::min(std::min(v, 16), std::max(1, len / 64)) : 0;
}

// Split-key forward: only where the 128-row tiles (causal: pairs of them) cannot fill the chip, the static exponent shift applies (dyn
// false: partials with a common shift add up exactly) and every split keeps >= 512 keys.  Causal (round 6): the workgroups are PAIRS of
// 128-row tiles (constant work: about k_len + 128 keys each); where the pairs cannot fill the chip -- one sequence of 4096 with 8 heads is
// 128 pairs on 256 CUs, and takes as long as two sequences -- each row tile's key range (up to its diagonal) is split.  16-bit only (the
// form rule of the model); the count from the same model with the pair as the tile.
inline int forward_splits(const fcsa_problem& p, bool dyn, int cus) {
  const bool bits16 = p.dtype != FCSA_F32;
  const int64_t bh = (int64_t)p.batch * p.heads, wgs = tile_workgroups(bh, p.q_len, 128, p.causal);
  if (dyn || (p.causal && (!bits16 || p.q_len < 256)) || wgs <= 0) return 1;
  if (const int v = sweep_splits("FCSA_SPLITS", p.k_len)) return v;
  if (bits16) return best_split(kSplitFwd, true, p.dim_head, wgs, bh * p.q_len, p.k_len, cus);
  return split_by_target(p, wgs, p.k_len, cus);
}

// Split-key dQ: every split keeps >= 512 keys.  C4 (1 x 8 heads x 1024 queries, 8192 keys): 64 row tiles, 8 splits.  Causal (round 6),
// like the forward: the workgroups are PAIRS of 128-row tiles; where the pairs cannot fill the chip each row tile's key range (up to its
// diagonal) is split.  16-bit only.
inline int backward_dq_splits(const fcsa_problem& p, int cus) {
  const bool bits16 = p.dtype != FCSA_F32;
  if (!p.causal || (bits16 && p.q_len >= 256))
    if (const int v = sweep_splits("FCSA_DQ_SPLITS", p.k_len)) return v;
  if (p.causal && (!bits16 || p.q_len < 256)) return 1;
  const int64_t bh = (int64_t)p.batch * p.heads, wgs = tile_workgroups(bh, p.q_len, 128, p.causal);
  if (bits16) return best_split(kSplitDq, false, p.dim_head, wgs, bh * p.q_len, p.k_len, cus);
  return split_by_target(p, wgs, p.k_len, cus);
}

// Split-query dK/dV: the mirror image -- few keys, many queries (B * H * ceil(M / 128) key tiles cannot fill the chip), every split keeps
// >= 512 queries.  Partial dK^ / dV go to f32 slabs [batch * heads][split][M][D] and the finalize kernel sums them (and applies the l2norm
// backward to dK^).  Single-headed and grouped K/V (round 6) split like any other problem: their per-head slabs simply become heads x
// splits slabs for the same finalize launch.  Causal (round 6): the workgroups are PAIRS of 128-key tiles; where the pairs cannot fill the
// chip each key tile's query range (from its diagonal down: at most k_len queries) is split.  16-bit only.
inline int backward_dkv_splits(const fcsa_problem& p, int cus) {
  const bool bits16 = p.dtype != FCSA_F32;
  if (!p.causal || (bits16 && p.k_len >= 256))
    if (const int v = sweep_splits("FCSA_DKV_SPLITS", p.q_len)) return v;
  if (p.causal && (!bits16 || p.k_len < 256)) return 1;
  const int64_t bh = (int64_t)p.batch * p.heads, wgs = tile_workgroups(bh, p.k_len, 128, p.causal);
  if (bits16) return best_split(kSplitDkv, false, p.dim_head, wgs, bh * p.k_len, p.causal ? std::min(p.q_len, p.k_len) : p.q_len, cus);
  return split_by_target(p, wgs, p.q_len, cus);
}

}  // namespace fcsa
