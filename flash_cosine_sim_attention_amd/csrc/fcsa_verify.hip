// fcsa_verify.hip -- the verify step of a speculative decoder, and a short prompt chunk, against a float16 / bfloat16 / fp8 (e4m3fn) key/value
// cache: 64-row tiles with key splits (fcsa_forward_kvcache_verify, include/fcsa.h).
//
//   verify_kernel   G * N_b = 32 ... 256 rows per K/V head against a long cache.  decode_tree_kernel / decode_ragged_kernel (fcsa_decode.hip)
//                   re-read and re-normalise every key once per 16 rows; prefill_kernel (fcsa_prefill.hip) shares the keys over 128 rows but
//                   cannot split them.  This kernel sits between, as verify_mx_kernel does for MXFP4 caches: one 4-wave workgroup per
//                   (64-row tile slot, K/V head, key split), rows token-major (r = i * G + g, so the G heads of a token share its
//                   visibility word), ONE 16-row MFMA tile per wave.
//                   KEYS   the split's range [lo, end) of the sequence's L_b keys is the decode kernels' (decode_window: whole 32-key blocks
//                          from the same lo), walked in 64-key stages through double-buffered LDS (PrefillLds' layout and pitch).
//                   STAGE  wave w loads the stage's keys 16 w ... 16 w + 15, key on lane & 15 and feature quarter on lane >> 4 -- 16 bytes per
//                          fragment of a 16-bit cache, 8 bytes of codes of an fp8 one, for K and V alike -- under the load rule
//                          (clamped_first, clamped_off) with the split's `end` as the bound, and holds TWO stages ahead in registers.  K is
//                          normalised by group_normalise, rounded once to the type and written to LDS ONCE PER WORKGROUP (64 rows); V goes in
//                          raw (fp8: converted to the type, exactly).
//                   MATH   per wave and 32-key block decode_body's: the same MFMA steps in the same order, softmax_step, pv_block -- so at
//                          equal split counts the partials are the ragged / tree kernel's bit for bit, in both exponent regimes.
//                   MASK   with words: decode_tree_kernel's rule -- with P = L - N, key < end && (key < P || (N <= 64 ? bit key - P of the
//                          row's word : key <= last_key)).  Without: the ragged kernel's -- `causal` (bottom-right: key <= last_key) or every
//                          key.  Both are ONE test: causal is the rule of a sequence whose words do not count, and "every key" that of a word
//                          of all ones.  A block that ends at or before min(P, end) takes a wave-uniform branch around the selects.
//                   STOP   `causal` without words: a wave does no math beyond the last key its 16 rows see, and the workgroup walks no stage
//                          beyond the last key its tile sees (prefill_kend) -- a block skipped this way is one whose every P~ is 0.
//                   END    the decode kernel's partials (ws_o, ws_ml, [splits][total_q * H] rows); launch_decode_combine finishes (v_scale of
//                          an fp8 cache is its to apply).
//                   SYNC   every wave of a workgroup that enters the stage loop loads its 16 keys and passes every barrier, whether its row
//                          tile has rows or not: the stage count is a function of workgroup-uniform values only.  An idle slot returns, and
//                          an empty range skips the loop, as a whole workgroup.
// The append before the kernel is launch_kv_append's ragged form with the same parameter block.  16-bit types, D = 64 / 128 only.
#include "fcsa_common.cuh"
#include "fcsa_decode_common.cuh"

#include <type_traits>

namespace fcsa {

namespace {

constexpr int kVerifyWaves = 4;
constexpr int kVerifyStage = kPrefillStage;      // keys per LDS stage: two 32-key blocks of the decode key loop
static_assert(kVerifyRows == kVerifyWaves * kDecodeRows, "one 16-row MFMA tile per wave");
static_assert(kVerifyStage == kVerifyWaves * 16, "a wave loads 16 keys of a stage");

// LDS plan, for the kernel and its launcher: PrefillLds' -- two stage buffers, each K^ [64][PITCH] then V [64][PITCH], both in the type, at
// the pitch pv_block reads.  69632 bytes at D = 128 (two workgroups per CU), 36864 at D = 64.
template <int D> struct VerifyLds {
  static constexpr int PITCH = kKvPitch<D, 2>;
  static constexpr int TILE = kVerifyStage * PITCH;
  static constexpr int BUF = 2 * TILE;
  static constexpr int BYTES = 2 * BUF;
};

// A wave's 16 keys of a stage in registers: lane (x, hi) holds features (4 j + hi) * 8 ... + 7 of key first16 + x of K and of V (FP8: the
// same features as one-byte codes).
template <typename T, int D, bool FP8> struct VerifyRegs {
  static constexpr int NJ = D / 32;
  static constexpr int CES = FP8 ? 1 : 2;                          // bytes of a cache element
  typedef std::conditional_t<FP8, u32x2, u32x4> Frag;
  Frag k[NJ], v[NJ];

  // The wave's 16 positions of the stage that starts at `stage0` (lo plus a multiple of 64, below `end`), under the load rule with the
  // split's end as the bound: no position at or beyond `end` is read, and the V of such a position is zero (as the decode kernel leaves
  // it).  own = stage0 + 16 wave can lie beyond the end (and, next to 2^31, beyond int): it is formed in 64 bits and clamped before
  // anything is indexed with it.  end >= 1.
  FCSA_DEV void load(const DecodeParams& p, int b, int kvh, int stage0, int wave, int end, int lane) {
    const int x = lane & 15, hi = lane >> 4;
    const int64_t own = (int64_t)stage0 + 16 * wave;
    const int first = own < end ? clamped_first((int)own, end) : ((end - 1) & ~15);
    const bool below = own + x < end;
    const int off = below ? clamped_off((int)own + x, first, end) : end - 1 - first;
    const char* krow = cache_base(p, p.kc, b, kvh, first) + (int64_t)off * p.kc.sn;
    const char* vrow = cache_base(p, p.vc, b, kvh, first) + (int64_t)off * p.vc.sn;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int f = (4 * j + hi) * 8;
      k[j] = *reinterpret_cast<const Frag*>(krow + f * CES);
      const Frag val = *reinterpret_cast<const Frag*>(vrow + f * CES);
      v[j] = below ? val : Frag{};
    }
  }

  // K^ (normalised and rounded as decode_body does before its first product) and raw V -> row `row` of a stage buffer
  // FP8: V's codes converted to T (exact); K's codes times kscale under l2norm (decode_body<FP8>: otherwise kscale is in the logit multiplier)
  FCSA_DEV void store(char* buf, int row, int lane, bool l2norm, int gs, float kscale) const {
    typedef VerifyLds<D> LP;
    const int hi = lane >> 4;
    char* kdst = buf + row * LP::PITCH + hi * 16;
    float xk[NJ][8];
    if constexpr (FP8) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        float xv[8];
        unpack_fp8(v[j], xv);
        *reinterpret_cast<u32x4*>(kdst + LP::TILE + 64 * j) = pack<T>(xv, 1.f);
        unpack_fp8(k[j], xk[j]);
      }
      if (l2norm) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int e = 0; e < 8; ++e) xk[j][e] *= kscale;
      }
    } else {
#pragma unroll
      for (int j = 0; j < NJ; ++j) *reinterpret_cast<u32x4*>(kdst + LP::TILE + 64 * j) = v[j];
#pragma unroll
      for (int j = 0; j < NJ; ++j) unpack<T>(k[j], xk[j]);
    }
    if (l2norm) group_normalise<NJ, 8>(xk, gs, D);
#pragma unroll
    for (int j = 0; j < NJ; ++j) *reinterpret_cast<u32x4*>(kdst + 64 * j) = pack<T>(xk[j], 1.f);      // k^ rounded to the type, once
  }
};

// Waves per SIMD the register allocation aims at: two (two workgroups per CU, what the LDS of D = 128 allows) -- every instantiation fits
// without scratch (profiles/verify_resources.txt).
constexpr int kVerifyWavesPerSimd = 2;

template <typename T, int D, bool DYN, bool FP8>
__global__ __launch_bounds__(64 * kVerifyWaves, kVerifyWavesPerSimd) void verify_kernel(DecodeRaggedParams p, DecodeTreeMask tm) {
  typedef VerifyLds<D> LP;
  typedef VerifyRegs<T, D, FP8> R;
  constexpr int NJ = R::NJ, FB = D / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int lane = threadIdx.x & 63, x = lane & 15, hi = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int id = blockIdx.x;
  const int split = id % p.splits;
  id /= p.splits;
  const int kvh = id % p.Hk;
  int b, rt, q0, N;
  if (!prefill_tile(p.cu_q, p.B, p.total_q, p.G, kVerifyRows, id / p.Hk, b, rt, q0, N)) return;      // an idle slot: the whole workgroup
  const int L = decode_len(p.seqlens != nullptr, p.seqlens != nullptr ? p.seqlens[b] : 0, p.append ? N : 0, p.capacity);
  int lo, n;
  decode_window(L, split, p.splits, lo, n);
  const int end = lo + n;
  const int P = L - N;                                // the first position of the step
  const bool masked = tm.words != nullptr;
  const bool stop_early = !masked && p.causal != 0;
  // whether the row's word decides the keys from P on -- a tree of at most 64 tokens, or no mask and no `causal` (a word of all ones) -- or
  // the causal rule does: a tree of more tokens than a word has bits, or `causal`
  const bool use_bits = masked ? N <= kCompactSlots : p.causal == 0;
  const bool open = !masked && p.causal == 0;         // every key below `end` is visible: no block needs the selects for the step's sake
  const int gs = D / p.groups;
  const int64_t row0 = (int64_t)rt * kVerifyRows;

  // The keys the workgroup walks, [lo, stop), and those the wave does math on, [lo, wave_stop): the split's, cut under stop_early at the
  // last key the tile's (the wave's) last token sees.  A wave without rows has wave_stop = 0: no math.  Both are uniform where they steer.
  const int stop = min(end, prefill_kend(L, N, p.G, row0, kVerifyRows, stop_early));
  const int wave_stop = min(end, prefill_kend(L, N, p.G, row0 + wave * kDecodeRows, kDecodeRows, stop_early));

  // this lane's query row: the column of every MFMA result
  const int64_t r = row0 + wave * kDecodeRows + x;
  const bool row_ok = r < (int64_t)p.G * N;
  const int g = row_ok ? (int)(r % p.G) : 0, qi = row_ok ? (int)(r / p.G) : 0;
  uint64_t word = ~(uint64_t)0;
  if (masked) word = row_ok ? tm.words[q0 + qi] : 0;      // (no bit for a row the tile does not have)
  u32x4 qf[NJ];
  {
    float xq[NJ][8];
    const char* qrow = p.q.p + (int64_t)(kvh * p.G + g) * p.q.sh + (int64_t)(q0 + qi) * p.q.sn;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int f = (4 * j + hi) * 8;
      const u32x4 u = row_ok ? *reinterpret_cast<const u32x4*>(qrow + f * 2) : u32x4{0u, 0u, 0u, 0u};
      unpack<T>(u, xq[j]);
    }
    if (p.l2norm) group_normalise<NJ, 8>(xq, gs, D);
#pragma unroll
    for (int j = 0; j < NJ; ++j) qf[j] = pack<T>(xq[j], p.l2norm ? p.c1 : 1.f);      // c1 * q^, one rounding
  }
  float smul = p.l2norm ? 1.f : p.c1;
  float kscale = 1.f;
  if constexpr (FP8) {
    kscale = p.k_scale[(int64_t)b * p.ks_b + (int64_t)kvh * p.ks_h];
    if (!p.l2norm) smul *= kscale;
  }

  f32x4 acc[FB];
#pragma unroll
  for (int fb = 0; fb < FB; ++fb) acc[fb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = DYN ? -INFINITY : p.c2, l = 0.f;

  const int stages = stop > lo ? (stop - lo + kVerifyStage - 1) / kVerifyStage : 0;
  const int my_row = wave * 16 + x;              // the stage row this lane loads
  const bool l2norm = p.l2norm != 0;

  // the math of stage st (in buffer st & 1): decode_body's block step for the wave's row tile, over the blocks the wave has
  auto math = [&](int st) {
    const char* kst = smem + (st & 1) * LP::BUF;
    const char* vst = kst + LP::TILE;
    const int kb0 = lo + st * kVerifyStage;      // below stop
#pragma unroll
    for (int blk = 0; blk < kVerifyStage / kDecodeBlock; ++blk) {
      if (blk * kDecodeBlock >= (int64_t)wave_stop - kb0) break;      // (a block the wave does not have; asked this way, kb below never passes end)
      const int kb = kb0 + blk * kDecodeBlock;
      // the distances from kb that the visibility test compares against, in 64 bits: P can be far below 0 and kb next to 2^31
      const int64_t to_end = (int64_t)end - kb, to_step = open ? to_end : (int64_t)P - kb;
      // S^T = K^ Q^T for the two 16-key halves: s[sb][rr] = logit of key kb + 16 sb + 4 hi + rr for row x (log2 units)
      f32x4 s[2];
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) {
        s[sb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const u32x4 kf = *reinterpret_cast<const u32x4*>(kst + (blk * kDecodeBlock + 16 * sb + x) * LP::PITCH + (4 * j + hi) * 16);
          s[sb] = Unit<T>::mfma(kf, qf[j], s[sb]);
        }
      }
      if (min(to_end, to_step) >= kDecodeBlock) {      // the whole block lies before the step and inside the split: no select (wave-uniform)
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) s[sb][rr] = s[sb][rr] * smul;
      } else {
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int off = 16 * sb + 4 * hi + rr;      // key = kb + off
            const bool vis = off < to_end && (off < to_step || (use_bits ? ((word >> ((off - to_step) & 63)) & 1) != 0 : off <= to_step + qi));
            s[sb][rr] = vis ? s[sb][rr] * smul : -INFINITY;
          }
      }
      f32x4 pr[2];
      softmax_step<DYN>(s, m, l, acc, p.c2, pr);
      // k-slot (hi, e) of the P~V product is key 16 (e >> 2) + 4 hi + (e & 3): P~ is used where the first product left it
      u32x4 pb;
      pb[0] = Traits<T>::pack2(pr[0][0], pr[0][1]);
      pb[1] = Traits<T>::pack2(pr[0][2], pr[0][3]);
      pb[2] = Traits<T>::pack2(pr[1][0], pr[1][1]);
      pb[3] = Traits<T>::pack2(pr[1][2], pr[1][3]);
      pv_block<T, D, 1>(vst, blk * kDecodeBlock, x, hi, &pb, &acc);
    }
  };
  // One stage of the loop.  On entry buffer st & 1 holds stage st, `have` the rows of stage st + 1 (requested one or two steps ago) and
  // `fetch` is free: request stage st + 2 (past the end: the last stage again, so no branch lies between a request and its use), do the
  // math of stage st, normalise stage st + 1 into the other buffer (last read before the barrier that ended the previous step).  Nothing
  // here depends on the wave or the lane but the math: every wave passes the barrier of every step.
  auto step = [&](int st, R& have, R& fetch) {
    fetch.load(p, b, kvh, lo + min(st + 2, stages - 1) * kVerifyStage, wave, end, lane);
    math(st);
    if (st + 1 < stages) have.store(smem + ((st + 1) & 1) * LP::BUF, my_row, lane, l2norm, gs, kscale);
    __syncthreads();
  };
  if (stages > 0) {      // (so end >= 1: what the load rule needs)
    R ra, rb;
    ra.load(p, b, kvh, lo, wave, end, lane);
    rb.load(p, b, kvh, lo + min(1, stages - 1) * kVerifyStage, wave, end, lane);
    ra.store(smem, my_row, lane, l2norm, gs, kscale);
    __syncthreads();
    for (int st = 0; st < stages; st += 2) {
      step(st, rb, ra);
      if (st + 1 >= stages) break;
      step(st + 1, ra, rb);
    }
  }

  // partials of row x, as decode_body's ragged form leaves them for the combine: [total_q, H] rows.  The row's head and token are worked
  // out again here (from an opaque lane id), so that no address lives through the key loop.
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const int xe = opaque(lane) & 15, hie = opaque(lane) >> 4;
  const int64_t re = row0 + wave * kDecodeRows + xe;
  if (re < (int64_t)p.G * N) {
    const int h = kvh * p.G + (int)(re % p.G);
    const int64_t rows = (int64_t)p.total_q * p.H, row = (q0 + re / p.G) * p.H + h;
    float* wo = p.ws_o + ((int64_t)split * rows + row) * D;
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) *reinterpret_cast<f32x4*>(wo + 16 * fb + 4 * hie) = acc[fb];
    if (hie == 0) *reinterpret_cast<f32x2*>(p.ws_ml + ((int64_t)split * rows + row) * 2) = f32x2{m, l};
  }
}

}  // namespace

// One 4-wave workgroup per (64-row tile slot, K/V head, key split): p.slots = fcsa::prefill_slots(total_q, B, G, kVerifyRows), p.splits and
// the workspace from the decode split rule fed that slot count.  tree.words: the visibility words, or nullptr -- p.causal then decides.
hipError_t launch_verify(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeTreeMask& tree, hipStream_t s) {
  if (f.step || !f.ragged) return hipErrorInvalidValue;
  if (tree.words != nullptr && p.causal) return hipErrorInvalidValue;
  return dispatch_chunk(dtype, D, [&](auto td) -> hipError_t {
    using T = typename decltype(td)::T;
    constexpr int DD = decltype(td)::D;
    constexpr int LDS = VerifyLds<DD>::BYTES;
    if (p.l2norm && !decode_groups_fast(DD, p.groups, 8)) return hipErrorInvalidValue;
    const int64_t wgs = (int64_t)p.slots * p.Hk * p.splits;
    if (wgs <= 0) return hipSuccess;
    const dim3 grid((unsigned)wgs), block(64 * kVerifyWaves);
    auto go = [&](auto dyn) -> hipError_t {
      constexpr bool DY = decltype(dyn)::value;
      if (f.fp8) return launch_part<verify_kernel<T, DD, DY, true>, LDS>(grid, block, s, p, tree);
      return launch_part<verify_kernel<T, DD, DY, false>, LDS>(grid, block, s, p, tree);
    };
    return p.dyn ? go(std::true_type{}) : go(std::false_type{});
  });
}

}  // namespace fcsa
