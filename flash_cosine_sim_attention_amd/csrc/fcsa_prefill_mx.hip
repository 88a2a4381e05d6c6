// fcsa_prefill_mx.hip -- a prompt chunk against an MXFP4 key/value cache (fcsa_forward_kvcache_mx_prefill, include/fcsa.h; DESIGN.md
// section 4.7.10).
//
//   prefill_mx_kernel   the frame of prefill_kernel (fcsa_prefill.hip): one 4-wave workgroup per (128-row tile slot, K/V head), rows
//                       token-major (r = i * G + g), two 16-row MFMA tiles per wave, the keys [0, kend) of the tile (prefill_kend) through
//                       LDS in 64-key stages, double-buffered.  The stage is this kernel's own:
//                       LOADS  wave w owns the stage's keys 16 w ... 16 w + 15 in decode_mx_kernel's "quarter row per lane" layout: lane
//                              (c, g) loads the contiguous D / 8 code bytes of quarter g of key c -- one 16-byte load that is one MX block at
//                              D = 128, one 8-byte load (half a block) at D = 64 -- and its scale byte, for K and for V alike, under the
//                              load rule (clamped_first, clamped_off).  A stage is D / 32 + D / 32 + 2 registers per lane, so TWO stages are
//                              held ahead in registers: stage s + 2 is requested before the math of stage s and converted after the math
//                              of stage s + 1.  The requests are unconditional (a stage beyond the end requests the last stage
//                              again), so the loop has no branch between a request and its use.
//                       K      converted to float32 with the scale folded in (v_cvt_scalef32_pk_f32_fp4), normalised by
//                              mx_group_normalise, rounded once to the type -- exactly decode_mx_kernel's values -- and written to the
//                              stage ONCE PER WORKGROUP (the decode kernel: once per 16 rows); without l2norm the codes go straight to
//                              the type.  The stage row is in feature order, so the fragment of MFMA step t of lane (x, hi) -- features
//                              hi D / 4 + 8 t + j, the decode kernel's permutation -- is the 16 bytes at hi D / 2 + 16 t of row x.
//                       V      the lane's chunk is one MX block (D = 64: half of one) of key c: converted straight to the type, the scale
//                              applied there, into the row-major padded rows pv_block reads transposed.
//                       Per wave, 32-key block and row tile the math is decode_mx_kernel's (the same MFMA steps in the same order, its
//                       visibility test, softmax_step, pv_block) and the epilogue is decode_combine_body's at one split, so o and lse are
//                       bit for bit those of fcsa_forward_kvcache_mx with one key split.  Every K^ fragment and transposed V read feeds
//                       both row tiles of the wave.
// The append before it is launch_kv_append_mx with the same parameter block.  16-bit types, D = 64 / 128 only.
#include "fcsa_common.cuh"
#include "fcsa_decode_common.cuh"
#include "fcsa_mx_common.cuh"

#include <type_traits>

namespace fcsa {

namespace {

constexpr int kMxWaves = 4;
constexpr int kMxTiles = kPrefillRows / kDecodeRows / kMxWaves;      // 16-row MFMA tiles per wave

// LDS plan, for the kernel and its launcher: two stage buffers, each K^ [64][PITCH] then V [64][PITCH], both in the type and in feature
// order at the pitch pv_block reads.  Bank arithmetic (64 banks of 4 bytes; a 16-byte access is served 16 lanes at a time): PITCH is
// 2 D + 16 bytes = 68 dwords at D = 128 and 36 at D = 64.  The 16 lanes of a pass are the 16 keys x of one quarter hi, at dword
// PITCH / 4 * x + const: 68 x = 4 x (mod 64) and 36 x = 4 * (9 x) (mod 64), 9 odd, so the 16 four-dword accesses start at the 16 distinct
// multiples of 4 and cover each bank once -- for the K^ fragment reads (const = hi D / 8 + 4 t), for the K^ and V writes of a stage (the
// same addresses, written by the lane that read them from the cache) alike.  So K^ needs no pitch of its own.
template <int D> struct PrefillMxLds {
  static constexpr int PITCH = kKvPitch<D, 2>;
  static constexpr int TILE = kPrefillStage * PITCH;
  static constexpr int BUF = 2 * TILE;
  static constexpr int BYTES = 2 * BUF;
};

// A wave's 16 keys of a stage in registers, as codes: lane (c, g) holds quarter g of key first16 + c -- NS words of eight codes and the
// scale byte of the MX block they lie in -- of K and of V.
template <typename T, int D> struct PrefillMxRegs {
  static constexpr int NS = D / 32;                   // MFMA steps of a 16-key half = words of codes per lane and key
  static constexpr int Q = D / 4;                     // features of a quarter: one MX block at D = 128, half of one at D = 64
  uint32_t k[NS], v[NS];
  uint32_t ks, vs;

  // the 16 positions from first16 of a sequence of L >= 1, under the load rule (clamped_first, clamped_off): no position at or beyond L is read
  FCSA_DEV void load(const DecodeParams& p, const DecodeMx& mx, int b, int kvh, int first16, int L, int lane) {
    const int c = lane & 15, g = lane >> 4;
    const int first = clamped_first(first16, L);
    const int off = clamped_off(first16 + c, first, L);
    load_words<NS>(cache_base(p, p.kc, b, kvh, first) + (int64_t)off * p.kc.sn + g * (Q / 2), k);
    load_words<NS>(cache_base(p, p.vc, b, kvh, first) + (int64_t)off * p.vc.sn + g * (Q / 2), v);
    ks = *reinterpret_cast<const uint8_t*>(cache_base(p, mx.ks, b, kvh, first) + (int64_t)off * mx.ks.sn + g * Q / 32);
    vs = *reinterpret_cast<const uint8_t*>(cache_base(p, mx.vs, b, kvh, first) + (int64_t)off * mx.vs.sn + g * Q / 32);
  }

  // K^ (converted, normalised and rounded as decode_mx_kernel does before its first product) and V in the type -> row `row` of a stage
  // buffer; live: the key is below L (the V of another row is zero, as the decode kernel leaves it)
  FCSA_DEV void store(char* buf, int row, int lane, bool live, bool l2norm, int gs) const {
    typedef PrefillMxLds<D> LP;
    char* kdst = buf + row * LP::PITCH + (lane >> 4) * (Q * 2);
    const float vscale = mx_scale(vs), kscale = mx_scale(ks);
#pragma unroll
    for (int t = 0; t < NS; ++t) *reinterpret_cast<u32x4*>(kdst + LP::TILE + 16 * t) = mx_word<T>(live ? v[t] : 0u, vscale);
    if (l2norm) {
      float xk[NS][8];
#pragma unroll
      for (int t = 0; t < NS; ++t) mx_word_f32(k[t], kscale, xk[t]);
      mx_group_normalise<NS>(xk, gs, lane);
#pragma unroll
      for (int t = 0; t < NS; ++t) *reinterpret_cast<u32x4*>(kdst + 16 * t) = pack<T>(xk[t], 1.f);      // k^ rounded to the type, once
    } else {
#pragma unroll
      for (int t = 0; t < NS; ++t) *reinterpret_cast<u32x4*>(kdst + 16 * t) = mx_word<T>(k[t], kscale);
    }
  }
};

// Waves per SIMD the register allocation aims at: two (two workgroups per CU, at most 256 registers) -- every instantiation fits without
// scratch (profiles/mxfp4_prefill_resources.txt): the stage in flight is codes, a quarter of the registers of the 16-bit kernel's.
template <typename T, int D> constexpr int kPrefillMxWavesPerSimd = 2;

// EDITORS: this kernel exists a SECOND time below, as step_prefill_mx_body (the chunk side of an engine step), and the two must stay bit for
// bit alike: a change to the stage loop, the math or the epilogue here is made there as well.
template <typename T, int D, bool DYN>
__global__ __launch_bounds__(64 * kMxWaves, (kPrefillMxWavesPerSimd<T, D>)) void prefill_mx_kernel(DecodeRaggedParams p, DecodeMx mx, DecodeLseOut lo) {
  typedef PrefillMxLds<D> LP;
  typedef PrefillMxRegs<T, D> R;
  constexpr int NS = R::NS, Q = R::Q, FB = D / 16, NR = kMxTiles;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int lane = threadIdx.x & 63, x = lane & 15, hi = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kvh = blockIdx.x % p.Hk;
  int b, rt, q0, N;
  if (!prefill_tile(p.cu_q, p.B, p.total_q, p.G, kPrefillRows, blockIdx.x / p.Hk, b, rt, q0, N)) return;
  const int L = decode_len(p.seqlens != nullptr, p.seqlens != nullptr ? p.seqlens[b] : 0, p.append ? N : 0, p.capacity);
  const int64_t row0 = (int64_t)rt * kPrefillRows;
  // the tile's keys [0, kend); a wave stops at the last key its own 32 rows see, but loads its share of every stage and joins every barrier
  const int kend = prefill_kend(L, N, p.G, row0, kPrefillRows, p.causal != 0);
  const int wave_kend = prefill_kend(L, N, p.G, row0 + wave * (NR * kDecodeRows), NR * kDecodeRows, p.causal != 0);
  const int gs = D / p.groups;

  // this lane's query rows, one per row tile, in the keys' order: unit t of lane (x, hi) holds features hi Q + 8 t ... + 7
  int last_key[NR];
  u32x4 qf[NR][NS];
#pragma unroll
  for (int r2 = 0; r2 < NR; ++r2) {
    const int64_t r = row0 + (wave * NR + r2) * kDecodeRows + x;
    const bool row_ok = r < (int64_t)p.G * N;
    const int g = row_ok ? (int)(r % p.G) : 0, qi = row_ok ? (int)(r / p.G) : 0;
    last_key[r2] = L - N + qi;                 // causal: key j is visible iff j <= last_key
    float xq[NS][8];
    const char* qrow = p.q.p + (int64_t)(kvh * p.G + g) * p.q.sh + (int64_t)(q0 + qi) * p.q.sn + hi * Q * 2;
#pragma unroll
    for (int t = 0; t < NS; ++t) {
      const u32x4 u = row_ok ? *reinterpret_cast<const u32x4*>(qrow + 16 * t) : u32x4{0u, 0u, 0u, 0u};
      unpack<T>(u, xq[t]);
    }
    if (p.l2norm) mx_group_normalise<NS>(xq, gs, lane);
#pragma unroll
    for (int t = 0; t < NS; ++t) qf[r2][t] = pack<T>(xq[t], p.l2norm ? p.c1 : 1.f);      // c1 * q^, one rounding
  }
  const float smul = p.l2norm ? 1.f : p.c1;

  f32x4 acc[NR][FB];
  float m[NR], l[NR];
#pragma unroll
  for (int r2 = 0; r2 < NR; ++r2) {
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) acc[r2][fb] = f32x4{0.f, 0.f, 0.f, 0.f};
    m[r2] = DYN ? -INFINITY : p.c2;
    l[r2] = 0.f;
  }

  const int stages = (kend + kPrefillStage - 1) / kPrefillStage;
  const int my_row = wave * 16 + x;              // the stage row this lane loads
  const bool l2norm = p.l2norm != 0;

  // the math of stage st (in buffer st & 1): decode_mx_kernel's block step for both row tiles
  auto math = [&](int st) {
    const char* kst = smem + (st & 1) * LP::BUF;
    const char* vst = kst + LP::TILE;
#pragma unroll
    for (int blk = 0; blk < kPrefillStage / kDecodeBlock; ++blk) {
      const int kb = st * kPrefillStage + blk * kDecodeBlock;
      if (kb >= wave_kend) break;
      // S^T = K^ Q^T for the two 16-key halves: s[r2][sb][rr] = logit of key kb + 16 sb + 4 hi + rr for row x of tile r2 (log2 units)
      f32x4 s[NR][2];
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) {
#pragma unroll
        for (int r2 = 0; r2 < NR; ++r2) s[r2][sb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NS; ++t) {
          const u32x4 kf = *reinterpret_cast<const u32x4*>(kst + (blk * kDecodeBlock + 16 * sb + x) * LP::PITCH + hi * (Q * 2) + 16 * t);
#pragma unroll
          for (int r2 = 0; r2 < NR; ++r2) s[r2][sb] = Unit<T>::mfma(kf, qf[r2][t], s[r2][sb]);
        }
      }
      u32x4 pb[NR];
#pragma unroll
      for (int r2 = 0; r2 < NR; ++r2) {
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int key = kb + 16 * sb + 4 * hi + rr;
            const bool vis = key < L && (!p.causal || key <= last_key[r2]);
            s[r2][sb][rr] = vis ? s[r2][sb][rr] * smul : -INFINITY;
          }
        f32x4 pr[2];
        softmax_step<DYN>(s[r2], m[r2], l[r2], acc[r2], p.c2, pr);
        // k-slot (hi, e) of the P~V product is key 16 (e >> 2) + 4 hi + (e & 3): P~ is used where the first product left it
        pb[r2][0] = Traits<T>::pack2(pr[0][0], pr[0][1]);
        pb[r2][1] = Traits<T>::pack2(pr[0][2], pr[0][3]);
        pb[r2][2] = Traits<T>::pack2(pr[1][0], pr[1][1]);
        pb[r2][3] = Traits<T>::pack2(pr[1][2], pr[1][3]);
      }
      pv_block<T, D, NR>(vst, blk * kDecodeBlock, x, hi, pb, acc);
    }
  };
  // One stage of the loop.  On entry buffer st & 1 holds stage st, `have` the codes of stage st + 1 (requested one or two steps ago) and
  // `fetch` is free: request stage st + 2, do the math of stage st, convert stage st + 1 into the other buffer (last read before the
  // barrier that ended the previous step).
  auto step = [&](int st, R& have, R& fetch) {
    fetch.load(p, mx, b, kvh, min(st + 2, stages - 1) * kPrefillStage + wave * 16, L, lane);      // (past the end: the last stage again)
    math(st);
    if (st + 1 < stages) have.store(smem + ((st + 1) & 1) * LP::BUF, my_row, lane, (st + 1) * kPrefillStage + my_row < L, l2norm, gs);
    __syncthreads();
  };
  if (stages > 0) {      // (so L >= 1: what the load rule needs)
    R ra, rb;
    ra.load(p, mx, b, kvh, wave * 16, L, lane);
    rb.load(p, mx, b, kvh, min(1, stages - 1) * kPrefillStage + wave * 16, L, lane);
    ra.store(smem, my_row, lane, my_row < L, l2norm, gs);
    __syncthreads();
    for (int st = 0; st < stages; st += 2) {
      step(st, rb, ra);
      if (st + 1 >= stages) break;
      step(st + 1, ra, rb);
    }
  }

  // Row x of tile r2: O^T[16 fb + 4 hi + rr][x] in acc[r2][fb][rr].  The combine of its one split (decode_combine_body's functions), in
  // registers.  The row's head and token are worked out again here (from an opaque lane id), so that no address lives through the key loop.
  const int xe = opaque(lane) & 15, hie = opaque(lane) >> 4;
#pragma unroll
  for (int r2 = 0; r2 < NR; ++r2) {
    float ls = l[r2];
    ls += __shfl_xor(ls, 16, 64);
    ls += __shfl_xor(ls, 32, 64);
    const int64_t r = row0 + (wave * NR + r2) * kDecodeRows + xe;
    if (r >= (int64_t)p.G * N) continue;
    const int h = kvh * p.G + (int)(r % p.G);
    const int64_t tok = q0 + r / p.G;
    const float M = m[r2];
    const bool any = M != -INFINITY;
    const float w = combine_weight(M, M);      // the one split's weight: 1
    float lsum = 0.f;
    if (any) lsum += w * ls;
    const float inv = combine_inv(p.dyn != 0, lsum, p.l_eps);
    char* dst = p.o.p + (int64_t)h * p.o.sh + tok * p.o.sn + 4 * hie * 2;
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      if (any) a += w * acc[r2][fb];
      a *= inv;
      *reinterpret_cast<u32x2*>(dst + 16 * fb * 2) = u32x2{Traits<T>::pack2(a[0], a[1]), Traits<T>::pack2(a[2], a[3])};
    }
    if (lo.lse != nullptr && hie == 0) lo.lse[(int64_t)h * lo.sh + tok * lo.sn] = decode_row_lse(M, lsum);
  }
}

// ... and of the chunk side of an engine step (step_prefill_mx_kernel, rotary_prefill_mx_kernel; profiles/mxfp4_step_resources.txt): two
// everywhere -- the routing test adds nothing to the key loop, and the rotation's registers (a unit's exchanged words, eight angles) are dead
// before it starts.
template <typename T, int D, bool ROTARY> constexpr int kStepPrefillMxWavesPerSimd = 2;

// The chunk side of an engine step (step_prefill_mx_kernel, rotary_prefill_mx_kernel; fcsa_forward_kvcache_mx_step):
// prefill_mx_kernel written a SECOND time, because that kernel keeps its text -- the same statements in the same order, so a chunk-routed
// row is that kernel's bit for bit -- with two additions.  A workgroup whose sequence is no chunk (step_is_chunk) exits: those rows are the
// step decode kernel's.  ROTARY: the RAW query rows are rotated by the table row of their position (mx_rotary_row, as
// step_decode_mx_body<ROTARY>) in the per-tile prologue, before the l2norm, for both row tiles of the wave.
template <typename T, int D, bool DYN, bool ROTARY>
FCSA_DEV void step_prefill_mx_body(const DecodeStepParams& p, const DecodeMx& mx, const DecodeLseOut& lo, const DecodeRotary& ro) {
  typedef PrefillMxLds<D> LP;
  typedef PrefillMxRegs<T, D> R;
  constexpr int NS = R::NS, Q = R::Q, FB = D / 16, NR = kMxTiles;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int lane = threadIdx.x & 63, x = lane & 15, hi = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kvh = blockIdx.x % p.Hk;
  int b, rt, q0, N;
  if (!prefill_tile(p.cu_q, p.B, p.total_q, p.G, kPrefillRows, blockIdx.x / p.Hk, b, rt, q0, N)) return;
  if (!step_is_chunk(p.G, N, p.chunk_rows)) return;
  const int L = decode_len(p.seqlens != nullptr, p.seqlens != nullptr ? p.seqlens[b] : 0, p.append ? N : 0, p.capacity);
  const int64_t row0 = (int64_t)rt * kPrefillRows;
  // the tile's keys [0, kend); a wave stops at the last key its own 32 rows see, but loads its share of every stage and joins every barrier
  const int kend = prefill_kend(L, N, p.G, row0, kPrefillRows, p.causal != 0);
  const int wave_kend = prefill_kend(L, N, p.G, row0 + wave * (NR * kDecodeRows), NR * kDecodeRows, p.causal != 0);
  const int gs = D / p.groups;

  // this lane's query rows, one per row tile, in the keys' order: unit t of lane (x, hi) holds features hi Q + 8 t ... + 7
  int last_key[NR];
  u32x4 qf[NR][NS];
#pragma unroll
  for (int r2 = 0; r2 < NR; ++r2) {
    const int64_t r = row0 + (wave * NR + r2) * kDecodeRows + x;
    const bool row_ok = r < (int64_t)p.G * N;
    const int g = row_ok ? (int)(r % p.G) : 0, qi = row_ok ? (int)(r / p.G) : 0;
    last_key[r2] = L - N + qi;                 // causal: key j is visible iff j <= last_key
    float xq[NS][8];
    [[maybe_unused]] u32x4 raw[NS];
    const char* qrow = p.q.p + (int64_t)(kvh * p.G + g) * p.q.sh + (int64_t)(q0 + qi) * p.q.sn + hi * Q * 2;
#pragma unroll
    for (int t = 0; t < NS; ++t) {
      const u32x4 u = row_ok ? *reinterpret_cast<const u32x4*>(qrow + 16 * t) : u32x4{0u, 0u, 0u, 0u};
      if constexpr (ROTARY) raw[t] = u;
      unpack<T>(u, xq[t]);
    }
    if constexpr (ROTARY) mx_rotary_row<T, NS>(raw, xq, ro, last_key[r2], lane);
    if (p.l2norm) mx_group_normalise<NS>(xq, gs, lane);
#pragma unroll
    for (int t = 0; t < NS; ++t) qf[r2][t] = pack<T>(xq[t], p.l2norm ? p.c1 : 1.f);      // c1 * q^, one rounding
  }
  const float smul = p.l2norm ? 1.f : p.c1;

  f32x4 acc[NR][FB];
  float m[NR], l[NR];
#pragma unroll
  for (int r2 = 0; r2 < NR; ++r2) {
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) acc[r2][fb] = f32x4{0.f, 0.f, 0.f, 0.f};
    m[r2] = DYN ? -INFINITY : p.c2;
    l[r2] = 0.f;
  }

  const int stages = (kend + kPrefillStage - 1) / kPrefillStage;
  const int my_row = wave * 16 + x;              // the stage row this lane loads
  const bool l2norm = p.l2norm != 0;

  // the math of stage st (in buffer st & 1): decode_mx_kernel's block step for both row tiles
  auto math = [&](int st) {
    const char* kst = smem + (st & 1) * LP::BUF;
    const char* vst = kst + LP::TILE;
#pragma unroll
    for (int blk = 0; blk < kPrefillStage / kDecodeBlock; ++blk) {
      const int kb = st * kPrefillStage + blk * kDecodeBlock;
      if (kb >= wave_kend) break;
      // S^T = K^ Q^T for the two 16-key halves: s[r2][sb][rr] = logit of key kb + 16 sb + 4 hi + rr for row x of tile r2 (log2 units)
      f32x4 s[NR][2];
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) {
#pragma unroll
        for (int r2 = 0; r2 < NR; ++r2) s[r2][sb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NS; ++t) {
          const u32x4 kf = *reinterpret_cast<const u32x4*>(kst + (blk * kDecodeBlock + 16 * sb + x) * LP::PITCH + hi * (Q * 2) + 16 * t);
#pragma unroll
          for (int r2 = 0; r2 < NR; ++r2) s[r2][sb] = Unit<T>::mfma(kf, qf[r2][t], s[r2][sb]);
        }
      }
      u32x4 pb[NR];
#pragma unroll
      for (int r2 = 0; r2 < NR; ++r2) {
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int key = kb + 16 * sb + 4 * hi + rr;
            const bool vis = key < L && (!p.causal || key <= last_key[r2]);
            s[r2][sb][rr] = vis ? s[r2][sb][rr] * smul : -INFINITY;
          }
        f32x4 pr[2];
        softmax_step<DYN>(s[r2], m[r2], l[r2], acc[r2], p.c2, pr);
        // k-slot (hi, e) of the P~V product is key 16 (e >> 2) + 4 hi + (e & 3): P~ is used where the first product left it
        pb[r2][0] = Traits<T>::pack2(pr[0][0], pr[0][1]);
        pb[r2][1] = Traits<T>::pack2(pr[0][2], pr[0][3]);
        pb[r2][2] = Traits<T>::pack2(pr[1][0], pr[1][1]);
        pb[r2][3] = Traits<T>::pack2(pr[1][2], pr[1][3]);
      }
      pv_block<T, D, NR>(vst, blk * kDecodeBlock, x, hi, pb, acc);
    }
  };
  // One stage of the loop.  On entry buffer st & 1 holds stage st, `have` the codes of stage st + 1 (requested one or two steps ago) and
  // `fetch` is free: request stage st + 2, do the math of stage st, convert stage st + 1 into the other buffer (last read before the
  // barrier that ended the previous step).
  auto step = [&](int st, R& have, R& fetch) {
    fetch.load(p, mx, b, kvh, min(st + 2, stages - 1) * kPrefillStage + wave * 16, L, lane);      // (past the end: the last stage again)
    math(st);
    if (st + 1 < stages) have.store(smem + ((st + 1) & 1) * LP::BUF, my_row, lane, (st + 1) * kPrefillStage + my_row < L, l2norm, gs);
    __syncthreads();
  };
  if (stages > 0) {      // (so L >= 1: what the load rule needs)
    R ra, rb;
    ra.load(p, mx, b, kvh, wave * 16, L, lane);
    rb.load(p, mx, b, kvh, min(1, stages - 1) * kPrefillStage + wave * 16, L, lane);
    ra.store(smem, my_row, lane, my_row < L, l2norm, gs);
    __syncthreads();
    for (int st = 0; st < stages; st += 2) {
      step(st, rb, ra);
      if (st + 1 >= stages) break;
      step(st + 1, ra, rb);
    }
  }

  // Row x of tile r2: O^T[16 fb + 4 hi + rr][x] in acc[r2][fb][rr].  The combine of its one split (decode_combine_body's functions), in
  // registers.  The row's head and token are worked out again here (from an opaque lane id), so that no address lives through the key loop.
  const int xe = opaque(lane) & 15, hie = opaque(lane) >> 4;
#pragma unroll
  for (int r2 = 0; r2 < NR; ++r2) {
    float ls = l[r2];
    ls += __shfl_xor(ls, 16, 64);
    ls += __shfl_xor(ls, 32, 64);
    const int64_t r = row0 + (wave * NR + r2) * kDecodeRows + xe;
    if (r >= (int64_t)p.G * N) continue;
    const int h = kvh * p.G + (int)(r % p.G);
    const int64_t tok = q0 + r / p.G;
    const float M = m[r2];
    const bool any = M != -INFINITY;
    const float w = combine_weight(M, M);      // the one split's weight: 1
    float lsum = 0.f;
    if (any) lsum += w * ls;
    const float inv = combine_inv(p.dyn != 0, lsum, p.l_eps);
    char* dst = p.o.p + (int64_t)h * p.o.sh + tok * p.o.sn + 4 * hie * 2;
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      if (any) a += w * acc[r2][fb];
      a *= inv;
      *reinterpret_cast<u32x2*>(dst + 16 * fb * 2) = u32x2{Traits<T>::pack2(a[0], a[1]), Traits<T>::pack2(a[2], a[3])};
    }
    if (lo.lse != nullptr && hie == 0) lo.lse[(int64_t)h * lo.sh + tok * lo.sn] = decode_row_lse(M, lsum);
  }
}

// The two entry points of launch_prefill_mx_step.
template <typename T, int D, bool DYN>
__global__ __launch_bounds__(64 * kMxWaves, (kStepPrefillMxWavesPerSimd<T, D, false>)) void step_prefill_mx_kernel(DecodeStepParams p, DecodeMx mx,
                                                                                                                 DecodeLseOut lo) {
  step_prefill_mx_body<T, D, DYN, false>(p, mx, lo, DecodeRotary{});
}
template <typename T, int D, bool DYN>
__global__ __launch_bounds__(64 * kMxWaves, (kStepPrefillMxWavesPerSimd<T, D, true>)) FCSA_NO_PK_F32 void rotary_prefill_mx_kernel(
    DecodeStepParams p, DecodeMx mx, DecodeLseOut lo, DecodeRotary ro) {
  step_prefill_mx_body<T, D, DYN, true>(p, mx, lo, ro);
}

}  // namespace

// One 4-wave workgroup per (row-tile slot of 128 rows, K/V head): p.slots = fcsa::prefill_slots(total_q, B, G, kPrefillRows), one split, no
// workspace.  lse: nullptr, or where the rows' log-sum-exp goes as well.  A ragged step on an MXFP4 cache only (no fp8, no step form).
hipError_t launch_prefill_mx(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeMx& mx, const DecodeLseOut* lse, hipStream_t s) {
  if (f.fp8 || f.step || !f.ragged) return hipErrorInvalidValue;
  if (p.l2norm && !mx_groups_ok(D, p.groups)) return hipErrorInvalidValue;
  return dispatch_chunk(dtype, D, [&](auto td) -> hipError_t {
    using T = typename decltype(td)::T;
    constexpr int DD = decltype(td)::D;
    constexpr int LDS = PrefillMxLds<DD>::BYTES;
    if ((int64_t)p.slots * p.Hk <= 0) return hipSuccess;
    const dim3 grid((unsigned)((int64_t)p.slots * p.Hk)), block(64 * kMxWaves);
    const DecodeLseOut lo = lse != nullptr ? *lse : DecodeLseOut{};
    return p.dyn ? launch_part<prefill_mx_kernel<T, DD, true>, LDS>(grid, block, s, p, mx, lo)
                 : launch_part<prefill_mx_kernel<T, DD, false>, LDS>(grid, block, s, p, mx, lo);
  });
}

// launch_prefill_mx's grid, block and LDS on the step entry points (fcsa_forward_kvcache_mx_step): the workgroups of decode-routed sequences
// exit at once.  rotary: nullptr, or the tables the prologue rotates q by (rotary_dim D, or 64 at D = 128).
hipError_t launch_prefill_mx_step(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeMx& mx, const DecodeRotary* rotary,
                                  const DecodeLseOut* lse, hipStream_t s) {
  if (f.fp8 || !f.step || !f.ragged || !mx_rotary_ok(D, rotary)) return hipErrorInvalidValue;
  if (p.l2norm && !mx_groups_ok(D, p.groups)) return hipErrorInvalidValue;
  return dispatch_chunk(dtype, D, [&](auto td) -> hipError_t {
    using T = typename decltype(td)::T;
    constexpr int DD = decltype(td)::D;
    constexpr int LDS = PrefillMxLds<DD>::BYTES;
    if ((int64_t)p.slots * p.Hk <= 0) return hipSuccess;
    const dim3 grid((unsigned)((int64_t)p.slots * p.Hk)), block(64 * kMxWaves);
    const DecodeLseOut lo = lse != nullptr ? *lse : DecodeLseOut{};
    auto go = [&](auto dyn) -> hipError_t {
      constexpr bool DY = decltype(dyn)::value;
      if (rotary != nullptr) return launch_part<rotary_prefill_mx_kernel<T, DD, DY>, LDS>(grid, block, s, p, mx, lo, *rotary);
      return launch_part<step_prefill_mx_kernel<T, DD, DY>, LDS>(grid, block, s, p, mx, lo);
    };
    return p.dyn ? go(std::true_type{}) : go(std::false_type{});
  });
}

}  // namespace fcsa
