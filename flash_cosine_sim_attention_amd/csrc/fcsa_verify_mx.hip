// fcsa_verify_mx.hip -- the verify step of a speculative decoder against an MXFP4 key/value cache: tree attention with key splits
// (fcsa_forward_kvcache_mx_tree, include/fcsa.h), and the compaction of the accepted path (fcsa_kvcache_mx_compact).
//
//   verify_mx_kernel      A verify step brings N_b = 8 ... 64 tokens per sequence: G * N_b = 32 ... 256 rows per K/V head against a long
//                         cache.  decode_mx_kernel converts and normalises every key once per 16 rows; prefill_mx_kernel shares the keys
//                         over 128 rows but cannot split them.  This kernel sits between: one 4-wave workgroup per (64-row tile slot, K/V
//                         head, key split), rows token-major (r = i * G + g, so the G heads of a token share its visibility word), ONE
//                         16-row MFMA tile per wave.
//                         KEYS   the split's range [lo, end) of the sequence's L_b keys is decode_mx_kernel's (decode_window: whole 32-key
//                                blocks from the same lo), walked in 64-key stages through double-buffered LDS.
//                         STAGE  the chunk kernel's scheme: wave w loads the stage's keys 16 w ... 16 w + 15 in the "quarter row per lane"
//                                layout -- lane (c, g) the contiguous D / 8 code bytes of quarter g of key c and its scale byte, for K and V
//                                alike, under the load rule (clamped_first, clamped_off, with the split's `end` as the bound) -- and two
//                                stages are held ahead in registers as codes.  K is converted with the scale folded in, normalised by
//                                mx_group_normalise, rounded once to the type and written to LDS ONCE PER WORKGROUP (64 rows); V goes
//                                straight to the type, into the rows pv_block reads transposed.
//                         MATH   per wave and 32-key block decode_mx_kernel's: the same MFMA steps on the same feature permutation in the
//                                same order, softmax_step, pv_block -- so at equal split counts the partials are that kernel's bit for bit.
//                         MASK   decode_tree_kernel's rule: with P = L - N, key < end && (key < P || (N <= 64 ? bit key - P of the row's
//                                word : key <= last_key)).  A block that ends at or before P is visible to every row: a wave-uniform branch
//                                skips the selects there (on a long cache that is almost every block).
//                         END    the decode kernel's partials (ws_o, ws_ml, [splits][total_q * H] rows); launch_decode_combine finishes.
//   kv_compact_mx_kernel  kv_compact_kernel's moves on the four tensors of an MXFP4 cache: one workgroup per (sequence, K/V head) reads every
//                         accepted source row -- D / 2 code bytes and D / 32 scale bytes, of K and of V -- into LDS, passes a barrier, writes.
// The append before the kernel is launch_kv_append_mx with the same parameter block.  16-bit types, D = 64 / 128 only.
#include "fcsa_common.cuh"
#include "fcsa_decode_common.cuh"
#include "fcsa_mx_common.cuh"

#include <type_traits>

namespace fcsa {

namespace {

constexpr int kVerifyWaves = 4;
constexpr int kVerifyStage = kPrefillStage;      // keys per LDS stage: two 32-key blocks of the decode key loop
static_assert(kVerifyRows == kVerifyWaves * kDecodeRows, "one 16-row MFMA tile per wave");

// LDS plan, for the kernel and its launcher: the chunk kernel's (PrefillMxLds, fcsa_prefill_mx.hip) -- two stage buffers, each K^ [64][PITCH]
// then V [64][PITCH], both in the type and in feature order at the pitch pv_block reads.  Its bank arithmetic holds unchanged: PITCH is
// 2 D + 16 bytes = 68 dwords at D = 128 and 36 at D = 64, and the 16 lanes of a pass are the 16 keys x of one quarter at dword
// PITCH / 4 * x + const, which start at the 16 distinct multiples of 4 modulo 64 -- for the fragment reads and the stage writes alike.
// 69632 bytes at D = 128 (two workgroups per CU), 36864 at D = 64.
template <int D> struct VerifyMxLds {
  static constexpr int PITCH = kKvPitch<D, 2>;
  static constexpr int TILE = kVerifyStage * PITCH;
  static constexpr int BUF = 2 * TILE;
  static constexpr int BYTES = 2 * BUF;
};

// A wave's 16 keys of a stage in registers, as codes: lane (c, g) holds quarter g of key first16 + c -- NS words of eight codes and the
// scale byte of the MX block they lie in -- of K and of V.
template <typename T, int D> struct VerifyMxRegs {
  static constexpr int NS = D / 32;                   // MFMA steps of a 16-key half = words of codes per lane and key
  static constexpr int Q = D / 4;                     // features of a quarter: one MX block at D = 128, half of one at D = 64
  uint32_t k[NS], v[NS];
  uint32_t ks, vs;

  // The wave's 16 positions of the stage that starts at `stage0` (a multiple of 32 below `end`), under the load rule with the split's end
  // as the bound: no position at or beyond `end` is read.  own = stage0 + 16 wave can lie beyond the end (and, next to 2^31, beyond int):
  // it is formed in 64 bits and clamped before anything is indexed with it.
  FCSA_DEV void load(const DecodeParams& p, const DecodeMx& mx, int b, int kvh, int stage0, int wave, int end, int lane) {
    const int c = lane & 15, g = lane >> 4;
    const int64_t own = (int64_t)stage0 + 16 * wave;
    const int first = own < end ? clamped_first((int)own, end) : ((end - 1) & ~15);
    const int off = own + c < end ? clamped_off((int)own + c, first, end) : end - 1 - first;
    load_words<NS>(cache_base(p, p.kc, b, kvh, first) + (int64_t)off * p.kc.sn + g * (Q / 2), k);
    load_words<NS>(cache_base(p, p.vc, b, kvh, first) + (int64_t)off * p.vc.sn + g * (Q / 2), v);
    ks = *reinterpret_cast<const uint8_t*>(cache_base(p, mx.ks, b, kvh, first) + (int64_t)off * mx.ks.sn + g * Q / 32);
    vs = *reinterpret_cast<const uint8_t*>(cache_base(p, mx.vs, b, kvh, first) + (int64_t)off * mx.vs.sn + g * Q / 32);
  }

  // K^ (converted, normalised and rounded as decode_mx_kernel does before its first product) and V in the type -> row `row` of a stage
  // buffer; live: the key is below the split's end (the V of another row is zero, as the decode kernel leaves it)
  FCSA_DEV void store(char* buf, int row, int lane, bool live, bool l2norm, int gs) const {
    typedef VerifyMxLds<D> LP;
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

// Waves per SIMD the register allocation aims at: two (two workgroups per CU) -- every instantiation fits without scratch
// (profiles/mxfp4_tree_resources.txt).
constexpr int kVerifyMxWavesPerSimd = 2;

template <typename T, int D, bool DYN>
__global__ __launch_bounds__(64 * kVerifyWaves, kVerifyMxWavesPerSimd) void verify_mx_kernel(DecodeRaggedParams p, DecodeMx mx, DecodeTreeMask tm) {
  typedef VerifyMxLds<D> LP;
  typedef VerifyMxRegs<T, D> R;
  constexpr int NS = R::NS, Q = R::Q, FB = D / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int lane = threadIdx.x & 63, x = lane & 15, hi = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int id = blockIdx.x;
  const int split = id % p.splits;
  id /= p.splits;
  const int kvh = id % p.Hk;
  int b, rt, q0, N;
  if (!prefill_tile(p.cu_q, p.B, p.total_q, p.G, kVerifyRows, id / p.Hk, b, rt, q0, N)) return;
  const int L = decode_len(p.seqlens != nullptr, p.seqlens != nullptr ? p.seqlens[b] : 0, p.append ? N : 0, p.capacity);
  int lo, n;
  decode_window(L, split, p.splits, lo, n);
  const int end = lo + n;
  const int P = L - N;                                // the first position of the step
  const bool use_bits = N <= kCompactSlots;           // more step tokens than a word has bits: the words are ignored, the sequence is causal
  const int gs = D / p.groups;

  // this lane's query row (the column of every MFMA result), in the keys' order: unit t of lane (x, hi) holds features hi Q + 8 t ... + 7
  const int64_t r = (int64_t)rt * kVerifyRows + wave * kDecodeRows + x;
  const bool row_ok = r < (int64_t)p.G * N;
  const int g = row_ok ? (int)(r % p.G) : 0, qi = row_ok ? (int)(r / p.G) : 0;
  const uint64_t word = row_ok ? tm.words[q0 + qi] : 0;      // (no bit for a row the tile does not have)
  u32x4 qf[NS];
  {
    float xq[NS][8];
    const char* qrow = p.q.p + (int64_t)(kvh * p.G + g) * p.q.sh + (int64_t)(q0 + qi) * p.q.sn + hi * Q * 2;
#pragma unroll
    for (int t = 0; t < NS; ++t) {
      const u32x4 u = row_ok ? *reinterpret_cast<const u32x4*>(qrow + 16 * t) : u32x4{0u, 0u, 0u, 0u};
      unpack<T>(u, xq[t]);
    }
    if (p.l2norm) mx_group_normalise<NS>(xq, gs, lane);
#pragma unroll
    for (int t = 0; t < NS; ++t) qf[t] = pack<T>(xq[t], p.l2norm ? p.c1 : 1.f);      // c1 * q^, one rounding
  }
  const float smul = p.l2norm ? 1.f : p.c1;

  f32x4 acc[FB];
#pragma unroll
  for (int fb = 0; fb < FB; ++fb) acc[fb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = DYN ? -INFINITY : p.c2, l = 0.f;

  const int stages = (n + kVerifyStage - 1) / kVerifyStage;
  const int my_row = wave * 16 + x;              // the stage row this lane loads
  const bool l2norm = p.l2norm != 0;

  // the math of stage st (in buffer st & 1): decode_mx_kernel's block step for the wave's row tile, over the blocks the split has
  auto math = [&](int st) {
    const char* kst = smem + (st & 1) * LP::BUF;
    const char* vst = kst + LP::TILE;
    const int kb0 = lo + st * kVerifyStage;      // below end
#pragma unroll
    for (int blk = 0; blk < kVerifyStage / kDecodeBlock; ++blk) {
      if (blk * kDecodeBlock >= end - kb0) break;      // (a block the split does not have; asked this way, kb below never passes end)
      const int kb = kb0 + blk * kDecodeBlock;
      // the distances from kb that the visibility test compares against, in 64 bits: P can be far below 0 and kb next to 2^31
      const int64_t to_end = (int64_t)end - kb, to_step = (int64_t)P - kb;
      // S^T = K^ Q^T for the two 16-key halves: s[sb][rr] = logit of key kb + 16 sb + 4 hi + rr for row x (log2 units)
      f32x4 s[2];
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) {
        s[sb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NS; ++t) {
          const u32x4 kf = *reinterpret_cast<const u32x4*>(kst + (blk * kDecodeBlock + 16 * sb + x) * LP::PITCH + hi * (Q * 2) + 16 * t);
          s[sb] = Unit<T>::mfma(kf, qf[t], s[sb]);
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
  // whether stage row `row` of stage st holds a key of the split
  auto live = [&](int st, int row) { return (int64_t)st * kVerifyStage + row < n; };
  // One stage of the loop.  On entry buffer st & 1 holds stage st, `have` the codes of stage st + 1 (requested one or two steps ago) and
  // `fetch` is free: request stage st + 2 (past the end: the last stage again, so no branch lies between a request and its use), do the
  // math of stage st, convert stage st + 1 into the other buffer (last read before the barrier that ended the previous step).
  auto step = [&](int st, R& have, R& fetch) {
    fetch.load(p, mx, b, kvh, lo + min(st + 2, stages - 1) * kVerifyStage, wave, end, lane);
    math(st);
    if (st + 1 < stages) have.store(smem + ((st + 1) & 1) * LP::BUF, my_row, lane, live(st + 1, my_row), l2norm, gs);
    __syncthreads();
  };
  if (stages > 0) {      // (so end >= 1: what the load rule needs)
    R ra, rb;
    ra.load(p, mx, b, kvh, lo, wave, end, lane);
    rb.load(p, mx, b, kvh, lo + min(1, stages - 1) * kVerifyStage, wave, end, lane);
    ra.store(smem, my_row, lane, live(0, my_row), l2norm, gs);
    __syncthreads();
    for (int st = 0; st < stages; st += 2) {
      step(st, rb, ra);
      if (st + 1 >= stages) break;
      step(st + 1, ra, rb);
    }
  }

  // partials of row x, as decode_mx_kernel's ragged form leaves them for the combine: [total_q, H] rows.  The row's head and token are
  // worked out again here (from an opaque lane id), so that no address lives through the key loop.
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const int xe = opaque(lane) & 15, hie = opaque(lane) >> 4;
  const int64_t re = (int64_t)rt * kVerifyRows + wave * kDecodeRows + xe;
  if (re < (int64_t)p.G * N) {
    const int h = kvh * p.G + (int)(re % p.G);
    const int64_t rows = (int64_t)p.total_q * p.H, row = (q0 + re / p.G) * p.H + h;
    float* wo = p.ws_o + ((int64_t)split * rows + row) * D;
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) *reinterpret_cast<f32x4*>(wo + 16 * fb + 4 * hie) = acc[fb];
    if (hie == 0) *reinterpret_cast<f32x2*>(p.ws_ml + ((int64_t)split * rows + row) * 2) = f32x2{m, l};
  }
}

// ---- compaction of the accepted path of a tree step on an MXFP4 cache (fcsa_kvcache_mx_compact) ----------------------------------------
// kv_compact_kernel's contract (fcsa_decode.hip) on four tensors: move i takes the row at position start + accepted[b, i] to start + i --
// the D / 2 code bytes and the D / 32 scale bytes, of K and of V -- start = clamp(cache_seqlens[b], 0, capacity).  One workgroup owns ALL
// moves of a (sequence, K/V head) pair, reads every source row into LDS, passes a barrier and only then writes, so a destination that is
// another move's source is safe.  A row of codes is row_bytes / 16 chunks of 16 bytes, and chunk ch is exactly MX block ch: the thread that
// moves a chunk moves its scale byte.  The tables are clamped -- num_accepted to [0, A], indices to [0, kCompactSlots) -- and a move whose
// source or destination is at or beyond the capacity is skipped.  Static LDS: 2 * 64 moves * (64 + 4) bytes = 8704, and the 64 source positions.
constexpr int kMxMaxRowBytes = 64;      // code bytes of a row at D = 128
__global__ __launch_bounds__(256) void kv_compact_mx_kernel(DecodeParams p, DecodeMx mx, CompactParams c) {
  __shared__ __attribute__((aligned(16))) char codes[2 * kCompactSlots * kMxMaxRowBytes];
  __shared__ uint8_t scales[2 * kCompactSlots * kMxMaxRowBytes / 16];
  __shared__ int src_pos[kCompactSlots];          // the cache position move i reads, or -1: no move
  const int kvh = blockIdx.x % p.Hk, b = blockIdx.x / p.Hk;
  const int64_t start = min(max((int64_t)p.seqlens[b], (int64_t)0), (int64_t)p.capacity);
  if (threadIdx.x < kCompactSlots) {
    const int i = threadIdx.x;
    const int n = min(max(c.num_accepted[b], 0), c.A);
    int sp = -1;
    if (i < n) {
      const int t = min(max(c.accepted[(int64_t)b * c.accepted_stride + i], 0), kCompactSlots - 1);
      if (t != i && start + t < p.capacity && start + i < p.capacity) sp = (int)(start + t);
    }
    src_pos[i] = sp;
  }
  __syncthreads();
  const int cpr = c.row_bytes / 16;               // 16-byte chunks of a row of codes = its scale bytes
  const int total = 2 * c.A * cpr;                // chunk id = (tensor * A + move) * cpr + chunk
  for (int id = threadIdx.x; id < total; id += 256) {
    const int ch = id % cpr, i = id / cpr % c.A, sp = src_pos[i];
    const bool is_k = id / cpr < c.A;
    if (sp >= 0) {
      *reinterpret_cast<u32x4*>(codes + id * 16) = *reinterpret_cast<const u32x4*>(cache_base(p, is_k ? p.kc : p.vc, b, kvh, sp) + ch * 16);
      scales[id] = *reinterpret_cast<const uint8_t*>(cache_base(p, is_k ? mx.ks : mx.vs, b, kvh, sp) + ch);
    }
  }
  __syncthreads();
  for (int id = threadIdx.x; id < total; id += 256) {
    const int ch = id % cpr, i = id / cpr % c.A;
    const bool is_k = id / cpr < c.A;
    if (src_pos[i] >= 0) {
      *reinterpret_cast<u32x4*>(cache_base(p, is_k ? p.kc : p.vc, b, kvh, (int)(start + i)) + ch * 16) = *reinterpret_cast<const u32x4*>(codes + id * 16);
      *reinterpret_cast<uint8_t*>(cache_base(p, is_k ? mx.ks : mx.vs, b, kvh, (int)(start + i)) + ch) = scales[id];
    }
  }
}

}  // namespace

// One 4-wave workgroup per (64-row tile slot, K/V head, key split): p.slots = fcsa::prefill_slots(total_q, B, G, kVerifyRows), p.splits and
// the workspace from the decode split rule fed that slot count.  A ragged step on an MXFP4 cache only (no fp8, no step form).
hipError_t launch_verify_mx(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeMx& mx, const DecodeTreeMask& tree, hipStream_t s) {
  if (f.fp8 || f.step || !f.ragged) return hipErrorInvalidValue;
  if (p.l2norm && !mx_groups_ok(D, p.groups)) return hipErrorInvalidValue;
  return dispatch_chunk(dtype, D, [&](auto td) -> hipError_t {
    using T = typename decltype(td)::T;
    constexpr int DD = decltype(td)::D;
    constexpr int LDS = VerifyMxLds<DD>::BYTES;
    const int64_t wgs = (int64_t)p.slots * p.Hk * p.splits;
    if (wgs <= 0) return hipSuccess;
    const dim3 grid((unsigned)wgs), block(64 * kVerifyWaves);
    return p.dyn ? launch_part<verify_mx_kernel<T, DD, true>, LDS>(grid, block, s, p, mx, tree)
                 : launch_part<verify_mx_kernel<T, DD, false>, LDS>(grid, block, s, p, mx, tree);
  });
}

hipError_t launch_kv_compact_mx(const DecodeParams& cache, const DecodeMx& mx, const CompactParams& c, hipStream_t s) {
  if (c.A < 1 || c.A > kCompactSlots || c.row_bytes < 16 || c.row_bytes > kMxMaxRowBytes || c.row_bytes % 16 != 0) return hipErrorInvalidValue;
  if ((int64_t)cache.B * cache.Hk <= 0) return hipSuccess;
  hipLaunchKernelGGL(kv_compact_mx_kernel, dim3((unsigned)((int64_t)cache.B * cache.Hk)), dim3(256), 0, s, cache, mx, c);
  return hipGetLastError();
}

}  // namespace fcsa
