// fcsa_decode_mx.hip -- decoding against an MXFP4 key/value cache (fcsa_forward_kvcache_mx, include/fcsa.h).
//
// The cache holds OCP MX v1.0 MXFP4: two e2m1 codes per byte (low nibble = the even feature) and one e8m0 scale byte per 32 consecutive
// features of a position, read clamped to [113, 139] -- inside that range every value e2m1(code) * 2^(s - 127) is exact in f16 and in bf16,
// so both MFMA products get the operands a 16-bit cache holding those values would feed, and the 16-bit combine kernels finish the call.
//
//   kv_append_mx_kernel   one thread per 32-feature block of a new row: amax, the scale byte, sixteen code bytes (v_cvt_scalef32_pk_fp4_f32
//                         on the clamped, pre-scaled values), for K and for V -- one 16-byte store and one byte store each
//   decode_mx_kernel      the decode frame -- one wave per (sequence, K/V head, 16-row tile, key split), 32-key blocks, S^T = K^ Q^T and
//                         O^T = V^T P~^T on mfma_f32_16x16x32, softmax_step / pv_block / the partials of fcsa_decode_common.cuh -- around a
//                         key loop of its own, "quarter row per lane": lane (c, g) of a 16-key half (c = lane % 16, g = lane / 16) loads
//                         the CONTIGUOUS quarter [g D/4, (g + 1) D/4) of key c -- D/8 bytes, at D = 128 one 16-byte load that is exactly
//                         one MX block -- and MFMA step t contracts the features g D/4 + 8 t + j.  That order is a permutation of the
//                         features; the query fragments, loaded once, use the same one.  Every 8-feature step lies inside one MX block
//                         (8 divides 32), so a step takes one scale, folded into the conversion (v_cvt_scalef32_pk_f32_fp4).
//                         K: with l2norm the float32 values are normalised (the sum of squares crosses the key's four lanes, or stays
//                         inside the l2norm group) and rounded once to the type, as 16-bit keys are; without it the codes go straight to
//                         the type (v_cvt_scalef32_pk_{f16,bf16}_fp4).  V: a lane's 16-byte chunk is one MX block of one key; it is
//                         converted straight to the type on the way into the LDS block that pv_block reads transposed.
// The conversions, the word loads and mx_group_normalise are fcsa_mx_common.cuh's, shared with the chunk kernel (fcsa_prefill_mx.hip).
#include "fcsa_common.cuh"
#include "fcsa_decode_common.cuh"
#include "fcsa_mx_common.cuh"

#include <type_traits>

namespace fcsa {
namespace {

// What a lane holds of a 32-key block.  K: per 16-key half its quarter of key c -- NT = D / 32 words of codes and the scale bytes of the
// MX blocks they lie in (one; D = 96: a quarter of 24 features can touch two blocks, so one per word).  V: 16-byte chunk c = lane + 64 t of
// the block's 32 D / 32 chunks is MX block c % (D / 32) of key c / (D / 32), with its scale byte.
// Per block and lane at D = 128: two 16-byte K loads and two byte loads, two 16-byte V loads and two byte loads.
template <int D> struct MxRegs {
  static constexpr int NT = D / 32;                   // MFMA steps of a 16-key half = words of codes per lane and key
  static constexpr int Q = D / 4;                     // features of a quarter
  static constexpr int NS = D == 96 ? NT : 1;         // K scale bytes per lane and key
  static constexpr int CPR = D / 32;                  // 16-byte chunks (= MX blocks) of a row of codes
  static constexpr int VTOT = kDecodeBlock * CPR;
  static constexpr int VCH = (VTOT + 63) / 64;
  uint32_t k[2][NT];
  uint32_t ks[2][NS];
  u32x4 v[VCH];
  uint32_t vs[VCH];

  // the 32-key block from `kb`, each 16-key half under the load rule (clamped_first, clamped_off): every position read is below `end`
  FCSA_DEV void load(const DecodeParams& p, const DecodeMx& mx, int b, int kvh, int kb, int end, int lane) {
    const int c = lane & 15, g = lane >> 4;
    int first[2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      first[sb] = clamped_first(kb + 16 * sb, end);
      const int off = clamped_off(kb + 16 * sb + c, first[sb], end);
      load_words<NT>(cache_base(p, p.kc, b, kvh, first[sb]) + (int64_t)off * p.kc.sn + g * (Q / 2), k[sb]);
      const uint8_t* srow = reinterpret_cast<const uint8_t*>(cache_base(p, mx.ks, b, kvh, first[sb]) + (int64_t)off * mx.ks.sn);
#pragma unroll
      for (int t = 0; t < NS; ++t) ks[sb][t] = srow[(g * Q + 8 * t) / 32];
    }
#pragma unroll
    for (int t = 0; t < VCH; ++t) {
      const int ci = lane + 64 * t, kk = ci / CPR, ch = ci % CPR, sb = kk >> 4;
      v[t] = u32x4{0u, 0u, 0u, 0u};
      vs[t] = 127u;
      if (ci < VTOT && kb + kk < end) {
        const int off = clamped_off(kb + kk, first[sb], end);
        v[t] = *reinterpret_cast<const u32x4*>(cache_base(p, p.vc, b, kvh, first[sb]) + (int64_t)off * p.vc.sn + ch * 16);
        vs[t] = *reinterpret_cast<const uint8_t*>(cache_base(p, mx.vs, b, kvh, first[sb]) + (int64_t)off * mx.vs.sn + ch);
      }
    }
  }
};

// RAGGED: packed queries with per-sequence counts (ragged_tile: idle slots exit at once); otherwise N rows per sequence.  Both forms carry
// the window sides, open ones (kWinOpen; causal: win_hi = 0) for a call without a window.
// EDITORS: the ragged form of this kernel exists a SECOND time below, as step_decode_mx_body (the decode side of an engine step), and the
// two must stay bit for bit alike: a change to the key loop, the visibility test or the partials here is made there as well.
template <typename T, int D, bool DYN, bool RAGGED>
__global__ __launch_bounds__(64) void decode_mx_kernel(DecodeRaggedParams p, DecodeMx mx) {
  typedef MxRegs<D> R;
  constexpr int NT = R::NT, Q = R::Q, CPR = R::CPR, VCH = R::VCH;
  constexpr int FB = D / 16;
  constexpr int PITCH = kKvPitch<D, 2>;
  extern __shared__ __attribute__((aligned(16))) char smem[];      // one 32-key V block in T, rows of D elements padded by 16 bytes

  const int lane = threadIdx.x, x = lane & 15, hi = lane >> 4;
  int id = blockIdx.x;
  const int split = id % p.splits;
  id /= p.splits;
  int rt, kvh, b, N, q0 = 0, new_len;
  if constexpr (RAGGED) {
    kvh = id % p.Hk;
    if (!ragged_tile(p.cu_q, p.B, p.total_q, p.G, id / p.Hk, b, rt, q0, N)) return;
    new_len = p.append ? N : 0;
  } else {
    rt = id % p.row_tiles;
    id /= p.row_tiles;
    kvh = id % p.Hk, b = id / p.Hk;
    N = p.N;
    new_len = p.new_len;
  }
  const int L = decode_len(p.seqlens != nullptr, p.seqlens != nullptr ? p.seqlens[b] : 0, new_len, p.capacity);
  int lo, n;
  const int first = win_decode_first(L, N, p.win_lo);
  decode_window(L - first, split, p.splits, lo, n);
  lo += first;
  const int end = lo + n;

  // this lane's query row: the column of every MFMA result
  const int r = rt * kDecodeRows + x;
  const bool row_ok = r < p.G * N;
  const int g = row_ok ? r / N : 0, qi = row_ok ? r % N : 0;
  const int h = kvh * p.G + g;
  const int last_key = L - N + qi;
  const int gs = D / p.groups;

  // the query in the keys' order: unit t of lane (x, hi) holds features hi Q + 8 t ... + 7
  u32x4 qf[NT];
  {
    float xq[NT][8];
    const char* qrow = p.q.p + (RAGGED ? 0 : (int64_t)b * p.q.sb) + (int64_t)h * p.q.sh + (int64_t)(q0 + qi) * p.q.sn + hi * Q * 2;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const u32x4 u = row_ok ? *reinterpret_cast<const u32x4*>(qrow + 16 * t) : u32x4{0u, 0u, 0u, 0u};
      unpack<T>(u, xq[t]);
    }
    if (p.l2norm) mx_group_normalise<NT>(xq, gs, lane);
#pragma unroll
    for (int t = 0; t < NT; ++t) qf[t] = pack<T>(xq[t], p.l2norm ? p.c1 : 1.f);
  }
  const float smul = p.l2norm ? 1.f : p.c1;

  f32x4 acc[FB];
#pragma unroll
  for (int fb = 0; fb < FB; ++fb) acc[fb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = DYN ? -INFINITY : p.c2, l = 0.f;

  R cur, nxt;
  if (n > 0) cur.load(p, mx, b, kvh, lo, end, lane);
  for (int kb = lo; kb < end; kb += kDecodeBlock) {
    if (kb + kDecodeBlock < end) nxt.load(p, mx, b, kvh, kb + kDecodeBlock, end, lane);
    // S^T = K^ Q^T for the two 16-key halves: s[sb][rr] = logit of key kb + 16 sb + 4 hi + rr for row x (log2 units)
    f32x4 s[2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      u32x4 kf[NT];
      if (p.l2norm) {
        float xk[NT][8];
#pragma unroll
        for (int t = 0; t < NT; ++t) mx_word_f32(cur.k[sb][t], mx_scale(cur.ks[sb][R::NS == 1 ? 0 : t]), xk[t]);
        mx_group_normalise<NT>(xk, gs, lane);
#pragma unroll
        for (int t = 0; t < NT; ++t) kf[t] = pack<T>(xk[t], 1.f);       // k^ rounded to the type, as the l2norm kernel writes it
      } else {
#pragma unroll
        for (int t = 0; t < NT; ++t) kf[t] = mx_word<T>(cur.k[sb][t], mx_scale(cur.ks[sb][R::NS == 1 ? 0 : t]));
      }
      s[sb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < NT; ++t) s[sb] = Unit<T>::mfma(kf[t], qf[t], s[sb]);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int key = kb + 16 * sb + 4 * hi + rr;
        const bool vis = key < end && key <= last_key + p.win_hi && key >= last_key - p.win_lo;
        s[sb][rr] = vis ? s[sb][rr] * smul : -INFINITY;
      }
    }
    f32x4 pr[2];
    softmax_step<DYN>(s, m, l, acc, p.c2, pr);

    // V block -> LDS in T (row-major, padded rows): a chunk of 16 code bytes becomes 32 elements, then O^T += V^T P~^T
#pragma unroll
    for (int t = 0; t < VCH; ++t) {
      const int ci = lane + 64 * t;
      if (R::VTOT % 64 == 0 || ci < R::VTOT) {
        const float vscale = mx_scale(cur.vs[t]);
        u32x4* dst = reinterpret_cast<u32x4*>(smem + (ci / CPR) * PITCH + (ci % CPR) * 64);
#pragma unroll
        for (int w = 0; w < 4; ++w) dst[w] = mx_word<T>(cur.v[t][w], vscale);
      }
    }
    __syncthreads();
    u32x4 pb;
    pb[0] = Traits<T>::pack2(pr[0][0], pr[0][1]);
    pb[1] = Traits<T>::pack2(pr[0][2], pr[0][3]);
    pb[2] = Traits<T>::pack2(pr[1][0], pr[1][1]);
    pb[3] = Traits<T>::pack2(pr[1][2], pr[1][3]);
    pv_block<T, D, 1>(smem, 0, x, hi, &pb, &acc);
    __syncthreads();
    cur = nxt;
  }

  // partials of row x, as the 16-bit decode kernel leaves them for the combine: [B, H, N] rows; RAGGED: [total_q, H]
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (row_ok) {
    int64_t rows, row;
    if constexpr (RAGGED) {
      rows = (int64_t)p.total_q * p.H;
      row = (int64_t)(q0 + qi) * p.H + h;
    } else {
      rows = (int64_t)p.B * p.H * N;
      row = ((int64_t)b * p.H + h) * N + qi;
    }
    float* wo = p.ws_o + ((int64_t)split * rows + row) * D;
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) *reinterpret_cast<f32x4*>(wo + 16 * fb + 4 * hi) = acc[fb];
    if (hi == 0) *reinterpret_cast<f32x2*>(p.ws_ml + ((int64_t)split * rows + row) * 2) = f32x2{m, l};
  }
}

// The decode side of an engine step (step_decode_mx_kernel, rotary_decode_mx_kernel; fcsa_forward_kvcache_mx_step):
// decode_mx_kernel's ragged form, written a SECOND time because that kernel keeps its text -- the same statements in the same order from
// the key loop on, so a decode-routed row is that kernel's bit for bit -- with two additions in front of it.  The workgroups leave the
// sequences of step_is_chunk to the chunk kernel (fcsa_prefill_mx.hip) and exit as soon as they know their sequence.  ROTARY: the RAW query
// row is rotated by the table row of its position last_key (mx_rotary_row) between the unpack and the l2norm, in float32 and in registers.
template <typename T, int D, bool DYN, bool ROTARY>
FCSA_DEV void step_decode_mx_body(const DecodeStepParams& p, const DecodeMx& mx, const DecodeRotary& ro) {
  static_assert(D == 64 || D == 128, "the step kernels exist where the chunk kernel does");
  typedef MxRegs<D> R;
  constexpr int NT = R::NT, Q = R::Q, CPR = R::CPR, VCH = R::VCH;
  constexpr int FB = D / 16;
  constexpr int PITCH = kKvPitch<D, 2>;
  extern __shared__ __attribute__((aligned(16))) char smem[];      // one 32-key V block in T, rows of D elements padded by 16 bytes

  const int lane = threadIdx.x, x = lane & 15, hi = lane >> 4;
  int id = blockIdx.x;
  const int split = id % p.splits;
  id /= p.splits;
  int rt, b, N, q0 = 0;
  const int kvh = id % p.Hk;
  if (!ragged_tile(p.cu_q, p.B, p.total_q, p.G, id / p.Hk, b, rt, q0, N)) return;
  if (step_is_chunk(p.G, N, p.chunk_rows)) return;
  const int L = decode_len(p.seqlens != nullptr, p.seqlens != nullptr ? p.seqlens[b] : 0, p.append ? N : 0, p.capacity);
  int lo, n;
  const int first = win_decode_first(L, N, p.win_lo);
  decode_window(L - first, split, p.splits, lo, n);
  lo += first;
  const int end = lo + n;

  // this lane's query row: the column of every MFMA result
  const int r = rt * kDecodeRows + x;
  const bool row_ok = r < p.G * N;
  const int g = row_ok ? r / N : 0, qi = row_ok ? r % N : 0;
  const int h = kvh * p.G + g;
  const int last_key = L - N + qi;
  const int gs = D / p.groups;

  // the query in the keys' order: unit t of lane (x, hi) holds features hi Q + 8 t ... + 7
  u32x4 qf[NT];
  {
    float xq[NT][8];
    [[maybe_unused]] u32x4 raw[NT];
    const char* qrow = p.q.p + (int64_t)h * p.q.sh + (int64_t)(q0 + qi) * p.q.sn + hi * Q * 2;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const u32x4 u = row_ok ? *reinterpret_cast<const u32x4*>(qrow + 16 * t) : u32x4{0u, 0u, 0u, 0u};
      if constexpr (ROTARY) raw[t] = u;
      unpack<T>(u, xq[t]);
    }
    if constexpr (ROTARY) mx_rotary_row<T, NT>(raw, xq, ro, last_key, lane);
    if (p.l2norm) mx_group_normalise<NT>(xq, gs, lane);
#pragma unroll
    for (int t = 0; t < NT; ++t) qf[t] = pack<T>(xq[t], p.l2norm ? p.c1 : 1.f);
  }
  const float smul = p.l2norm ? 1.f : p.c1;

  f32x4 acc[FB];
#pragma unroll
  for (int fb = 0; fb < FB; ++fb) acc[fb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = DYN ? -INFINITY : p.c2, l = 0.f;

  R cur, nxt;
  if (n > 0) cur.load(p, mx, b, kvh, lo, end, lane);
  for (int kb = lo; kb < end; kb += kDecodeBlock) {
    if (kb + kDecodeBlock < end) nxt.load(p, mx, b, kvh, kb + kDecodeBlock, end, lane);
    // S^T = K^ Q^T for the two 16-key halves: s[sb][rr] = logit of key kb + 16 sb + 4 hi + rr for row x (log2 units)
    f32x4 s[2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      u32x4 kf[NT];
      if (p.l2norm) {
        float xk[NT][8];
#pragma unroll
        for (int t = 0; t < NT; ++t) mx_word_f32(cur.k[sb][t], mx_scale(cur.ks[sb][R::NS == 1 ? 0 : t]), xk[t]);
        mx_group_normalise<NT>(xk, gs, lane);
#pragma unroll
        for (int t = 0; t < NT; ++t) kf[t] = pack<T>(xk[t], 1.f);       // k^ rounded to the type, as the l2norm kernel writes it
      } else {
#pragma unroll
        for (int t = 0; t < NT; ++t) kf[t] = mx_word<T>(cur.k[sb][t], mx_scale(cur.ks[sb][R::NS == 1 ? 0 : t]));
      }
      s[sb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < NT; ++t) s[sb] = Unit<T>::mfma(kf[t], qf[t], s[sb]);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int key = kb + 16 * sb + 4 * hi + rr;
        const bool vis = key < end && key <= last_key + p.win_hi && key >= last_key - p.win_lo;
        s[sb][rr] = vis ? s[sb][rr] * smul : -INFINITY;
      }
    }
    f32x4 pr[2];
    softmax_step<DYN>(s, m, l, acc, p.c2, pr);

    // V block -> LDS in T (row-major, padded rows): a chunk of 16 code bytes becomes 32 elements, then O^T += V^T P~^T
#pragma unroll
    for (int t = 0; t < VCH; ++t) {
      const int ci = lane + 64 * t;
      if (R::VTOT % 64 == 0 || ci < R::VTOT) {
        const float vscale = mx_scale(cur.vs[t]);
        u32x4* dst = reinterpret_cast<u32x4*>(smem + (ci / CPR) * PITCH + (ci % CPR) * 64);
#pragma unroll
        for (int w = 0; w < 4; ++w) dst[w] = mx_word<T>(cur.v[t][w], vscale);
      }
    }
    __syncthreads();
    u32x4 pb;
    pb[0] = Traits<T>::pack2(pr[0][0], pr[0][1]);
    pb[1] = Traits<T>::pack2(pr[0][2], pr[0][3]);
    pb[2] = Traits<T>::pack2(pr[1][0], pr[1][1]);
    pb[3] = Traits<T>::pack2(pr[1][2], pr[1][3]);
    pv_block<T, D, 1>(smem, 0, x, hi, &pb, &acc);
    __syncthreads();
    cur = nxt;
  }

  // partials of row x, as decode_mx_kernel's ragged form leaves them for the combine: [total_q, H] rows
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (row_ok) {
    const int64_t rows = (int64_t)p.total_q * p.H, row = (int64_t)(q0 + qi) * p.H + h;
    float* wo = p.ws_o + ((int64_t)split * rows + row) * D;
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) *reinterpret_cast<f32x4*>(wo + 16 * fb + 4 * hi) = acc[fb];
    if (hi == 0) *reinterpret_cast<f32x2*>(p.ws_ml + ((int64_t)split * rows + row) * 2) = f32x2{m, l};
  }
}

// The two entry points of launch_decode_mx_step.  The rotating one takes FCSA_NO_PK_F32: compiled both ways, it needs 173 / 174 registers
// with the attribute and 186 / 187 without at D = 128 (profiles/mxfp4_step_resources.txt).
template <typename T, int D, bool DYN>
__global__ __launch_bounds__(64) void step_decode_mx_kernel(DecodeStepParams p, DecodeMx mx) {
  step_decode_mx_body<T, D, DYN, false>(p, mx, DecodeRotary{});
}
template <typename T, int D, bool DYN>
__global__ __launch_bounds__(64) FCSA_NO_PK_F32 void rotary_decode_mx_kernel(DecodeStepParams p, DecodeMx mx, DecodeRotary ro) {
  step_decode_mx_body<T, D, DYN, true>(p, mx, ro);
}

// ---- the append -------------------------------------------------------------------------------------------------------------------------
// One 32-feature block (64 source bytes of T) -> its scale byte and sixteen code bytes, in float32:
//   e = clamp(floor(log2(amax)) - 2, -14, 12), floor(log2) being amax's exponent field (amax = 0 and float32 subnormals: -14);
//   scale byte = e + 127;  code = e2m1_rne(clamp(x * 2^-e, -6, 6)).
// The clamp is explicit and the multiply by the power of two exact, so the pack conversion (scale operand 1.0) only rounds a value inside
// the e2m1 range to nearest, ties to the even code.
// (The rotating append, kv_append_mx_rotary_kernel, states the same rule a second time in mx_quantise_values: a change here is made there.)
template <typename T> FCSA_DEV void mx_quantise_block(const char* src, char* codes, uint8_t* scale) {
  float x[4][8];
  float amax = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    unpack<T>(*reinterpret_cast<const u32x4*>(src + 16 * w), x[w]);
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(x[w][e]));
  }
  const int e = min(max((int)((__builtin_bit_cast(uint32_t, amax) >> 23) & 0xffu) - 129, -14), 12);
  const float inv = as_f32((uint32_t)(127 - e) << 23);
  u32x4 out;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    float y[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) y[i] = fminf(fmaxf(x[w][i] * inv, -6.f), 6.f);
    uint32_t c = 0u;
    c = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(c, y[0], y[1], 1.f, 0);
    c = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(c, y[2], y[3], 1.f, 1);
    c = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(c, y[4], y[5], 1.f, 2);
    c = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(c, y[6], y[7], 1.f, 3);
    out[w] = c;
  }
  *reinterpret_cast<u32x4*>(codes) = out;
  *scale = (uint8_t)(e + 127);
}

// One thread per MX block of a new row of a K/V head, K and V alike.  Where the row goes is the family's rule: position
// clamp(cache_seqlens[b], 0, capacity) + i, dropped at or beyond the capacity (every row, when seqlens is null); its address is cache_base.
// RAGGED: packed row `tok` of kn / vn [total_q, Hk, D], slot tok - cu_q[b] of its sequence; otherwise row tn of [B, Hk, new_len, D].
template <typename T, int D, bool RAGGED>
__global__ __launch_bounds__(256) void kv_append_mx_kernel(DecodeRaggedParams p, DecodeMx mx) {
  constexpr int CPR = D / 32;
  const int64_t total = (RAGGED ? (int64_t)p.total_q : (int64_t)p.B * p.new_len) * p.Hk * CPR;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int ch = (int)(t % CPR);
  int64_t rest = t / CPR;
  const int kvh = (int)(rest % p.Hk);
  rest /= p.Hk;
  int b;
  int64_t i;
  const char *ksrc, *vsrc;
  if constexpr (RAGGED) {
    const int64_t tok = rest;
    b = ragged_seq_of(p.cu_q, p.B, p.total_q, tok);
    const int64_t q0 = ragged_cu(p.cu_q[b], p.total_q), q1 = ragged_cu(p.cu_q[b + 1], p.total_q);
    if (tok < q0 || tok >= q1) return;          // (a malformed table: the row belongs to no sequence)
    i = tok - q0;
    ksrc = p.kn.p + (int64_t)kvh * p.kn.sh + tok * p.kn.sn;
    vsrc = p.vn.p + (int64_t)kvh * p.vn.sh + tok * p.vn.sn;
  } else {
    i = rest % p.new_len;
    b = (int)(rest / p.new_len);
    ksrc = p.kn.p + (int64_t)b * p.kn.sb + (int64_t)kvh * p.kn.sh + i * p.kn.sn;
    vsrc = p.vn.p + (int64_t)b * p.vn.sb + (int64_t)kvh * p.vn.sh + i * p.vn.sn;
  }
  const int64_t start = p.seqlens != nullptr ? min(max((int64_t)p.seqlens[b], (int64_t)0), (int64_t)p.capacity) : (int64_t)p.capacity;
  if (start + i >= p.capacity) return;
  const int pos = (int)(start + i);
  mx_quantise_block<T>(ksrc + ch * 64, cache_base(p, p.kc, b, kvh, pos) + ch * 16, reinterpret_cast<uint8_t*>(cache_base(p, mx.ks, b, kvh, pos)) + ch);
  mx_quantise_block<T>(vsrc + ch * 64, cache_base(p, p.vc, b, kvh, pos) + ch * 16, reinterpret_cast<uint8_t*>(cache_base(p, mx.vs, b, kvh, pos)) + ch);
}

// kv_append_mx_kernel's ragged form with a rotary embedding of K (launch_kv_append_mx_rotary): one launch unpacks k_new to float32, rotates it
// by the table row of the slot it is appended at (rotary_at) and quantises the ROTATED values -- the per-block amax included -- so no
// rotated 16-bit k_new exists and the keys are rounded once, to their codes.  Thread `ch` of a (row, K/V head) quantises V block ch
// unrotated.  K: with split pairs thread ch < rotary_dim / 64 does BOTH block ch and its partner block ch + rotary_dim / 64, and the
// thread of the partner block does no K work at all (it idles after its V block: half the K threads of a rotated row do double work, the
// price of reading every source byte and table value once); an interleaved block is self-contained, and a block at or beyond rotary_dim
// is quantised as before.  Every code and scale byte is written once, by mx_quantise_values' stores.  The kernel has not been timed alone.
// The arithmetic is rotary_unit's: t = fl(partner * sin), then one fused multiply-add.  Rows at or beyond the capacity are neither
// rotated nor written.
// mx_quantise_block's rule on the block's 32 float32 values in registers (amax is taken AFTER the rotation): a second statement of that
// rule, because kv_append_mx_kernel keeps its instruction text -- sharing one function reordered it.  A change to either is made to both.
template <typename T> FCSA_DEV void mx_load_block(const char* src, float (&x)[4][8]) {
#pragma unroll
  for (int w = 0; w < 4; ++w) unpack<T>(*reinterpret_cast<const u32x4*>(src + 16 * w), x[w]);
}
FCSA_DEV void mx_quantise_values(const float (&x)[4][8], char* codes, uint8_t* scale) {
  float amax = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w)
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(x[w][e]));
  const int e = min(max((int)((__builtin_bit_cast(uint32_t, amax) >> 23) & 0xffu) - 129, -14), 12);
  const float inv = as_f32((uint32_t)(127 - e) << 23);
  u32x4 out;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    float y[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) y[i] = fminf(fmaxf(x[w][i] * inv, -6.f), 6.f);
    uint32_t c = 0u;
    c = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(c, y[0], y[1], 1.f, 0);
    c = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(c, y[2], y[3], 1.f, 1);
    c = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(c, y[4], y[5], 1.f, 2);
    c = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(c, y[6], y[7], 1.f, 3);
    out[w] = c;
  }
  *reinterpret_cast<u32x4*>(codes) = out;
  *scale = (uint8_t)(e + 127);
}
template <typename T, int D>
__global__ __launch_bounds__(256) FCSA_NO_PK_F32 void kv_append_mx_rotary_kernel(DecodeRaggedParams p, DecodeMx mx, DecodeRotary ro) {
  constexpr int CPR = D / 32;
  const int64_t total = (int64_t)p.total_q * p.Hk * CPR;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int ch = (int)(t % CPR);
  const int64_t rest = t / CPR;
  const int kvh = (int)(rest % p.Hk);
  const int64_t tok = rest / p.Hk;
  const int b = ragged_seq_of(p.cu_q, p.B, p.total_q, tok);
  const int64_t q0 = ragged_cu(p.cu_q[b], p.total_q), q1 = ragged_cu(p.cu_q[b + 1], p.total_q);
  if (tok < q0 || tok >= q1) return;          // (a malformed table: the row belongs to no sequence)
  const int64_t start = p.seqlens != nullptr ? min(max((int64_t)p.seqlens[b], (int64_t)0), (int64_t)p.capacity) : (int64_t)p.capacity;
  if (start + (tok - q0) >= p.capacity) return;
  const int pos = (int)(start + (tok - q0));
  const char* ksrc = p.kn.p + (int64_t)kvh * p.kn.sh + tok * p.kn.sn;
  const char* vsrc = p.vn.p + (int64_t)kvh * p.vn.sh + tok * p.vn.sn;
  char* kdst = cache_base(p, p.kc, b, kvh, pos);
  uint8_t* ksdst = reinterpret_cast<uint8_t*>(cache_base(p, mx.ks, b, kvh, pos));
  mx_quantise_block<T>(vsrc + ch * 64, cache_base(p, p.vc, b, kvh, pos) + ch * 16, reinterpret_cast<uint8_t*>(cache_base(p, mx.vs, b, kvh, pos)) + ch);
  const float* c = ro.cos + rotary_at(ro, pos);
  const float* s = ro.sin + rotary_at(ro, pos);
  const int blocks = ro.rotary_dim / 32, away = blocks / 2;      // rotated blocks, and those between split partners
  float x[4][8];
  if (ch >= blocks) {
    mx_quantise_block<T>(ksrc + ch * 64, kdst + ch * 16, ksdst + ch);
  } else if (ro.interleaved) {
    mx_load_block<T>(ksrc + ch * 64, x);
    float r[4][8];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const f32x4 cv = *reinterpret_cast<const f32x4*>(c + 16 * ch + 4 * w), sv = *reinterpret_cast<const f32x4*>(s + 16 * ch + 4 * w);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a = x[w][2 * e], bb = x[w][2 * e + 1];
        r[w][2 * e] = fmaf(a, cv[e], -(bb * sv[e]));
        r[w][2 * e + 1] = fmaf(bb, cv[e], a * sv[e]);
      }
    }
    mx_quantise_values(r, kdst + ch * 16, ksdst + ch);
  } else if (ch < away) {
    float y[4][8], rx[4][8], ry[4][8];
    mx_load_block<T>(ksrc + ch * 64, x);
    mx_load_block<T>(ksrc + (ch + away) * 64, y);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x4 cv = *reinterpret_cast<const f32x4*>(c + 32 * ch + 8 * w + 4 * h), sv = *reinterpret_cast<const f32x4*>(s + 32 * ch + 8 * w + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a = x[w][4 * h + e], bb = y[w][4 * h + e];
          rx[w][4 * h + e] = fmaf(a, cv[e], -(bb * sv[e]));
          ry[w][4 * h + e] = fmaf(bb, cv[e], a * sv[e]);
        }
      }
    }
    mx_quantise_values(rx, kdst + ch * 16, ksdst + ch);
    mx_quantise_values(ry, kdst + (ch + away) * 16, ksdst + ch + away);
  }
}

// the 16-bit types x D 32 / 64 / 96 / 128 x ragged or not: fn(TypeDim<T, D>, RAGGED); everything else hipErrorInvalidValue
template <typename F> hipError_t dispatch_mx(int dtype, int D, DecodeForm f, F&& fn) {
  if (f.fp8 || f.step) return hipErrorInvalidValue;
  return dispatch_dtype_d(dtype, D, [&](auto td) -> hipError_t {
    if constexpr (Traits<typename decltype(td)::T>::ES == 2 && decltype(td)::D % 32 == 0) {
      return f.ragged ? fn(td, std::true_type{}) : fn(td, std::false_type{});
    } else {
      return hipErrorInvalidValue;
    }
  });
}

}  // namespace

hipError_t launch_kv_append_mx(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeMx& mx, hipStream_t s) {
  return dispatch_mx(dtype, D, f, [&](auto td, auto ragged) -> hipError_t {
    using T = typename decltype(td)::T;
    constexpr int DD = decltype(td)::D;
    constexpr bool RAGGED = decltype(ragged)::value;
    const int64_t threads = (RAGGED ? (int64_t)p.total_q : (int64_t)p.B * p.new_len) * p.Hk * (DD / 32);
    if (threads <= 0 || (RAGGED && p.B <= 0)) return hipSuccess;
    return launch_part<kv_append_mx_kernel<T, DD, RAGGED>, 0>(dim3((unsigned)((threads + 255) / 256)), dim3(256), s, p, mx);
  });
}

hipError_t launch_decode_mx(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeMx& mx, hipStream_t s) {
  if (p.l2norm && !mx_groups_ok(D, p.groups)) return hipErrorInvalidValue;
  return dispatch_mx(dtype, D, f, [&](auto td, auto ragged) -> hipError_t {
    using T = typename decltype(td)::T;
    constexpr int DD = decltype(td)::D;
    constexpr bool RAGGED = decltype(ragged)::value;
    constexpr int LDS = kDecodeBlock * kKvPitch<DD, 2>;
    const int64_t wgs = (RAGGED ? (int64_t)p.slots : (int64_t)p.B * p.row_tiles) * p.Hk * p.splits;
    if (wgs <= 0) return hipSuccess;
    const dim3 grid((unsigned)wgs), block(64);
    return p.dyn ? launch_part<decode_mx_kernel<T, DD, true, RAGGED>, LDS>(grid, block, s, p, mx)
                 : launch_part<decode_mx_kernel<T, DD, false, RAGGED>, LDS>(grid, block, s, p, mx);
  });
}

// ---- an engine step on an MXFP4 cache (fcsa_forward_kvcache_mx_step) ---------------------------------------------------------------------
hipError_t launch_kv_append_mx_rotary(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeMx& mx, const DecodeRotary& rotary,
                                      hipStream_t s) {
  if (f.fp8 || !f.ragged || !f.step || !mx_rotary_ok(D, &rotary)) return hipErrorInvalidValue;
  return dispatch_chunk(dtype, D, [&](auto td) -> hipError_t {
    using T = typename decltype(td)::T;
    constexpr int DD = decltype(td)::D;
    const int64_t threads = (int64_t)p.total_q * p.Hk * (DD / 32);
    if (threads <= 0 || p.B <= 0) return hipSuccess;
    return launch_part<kv_append_mx_rotary_kernel<T, DD>, 0>(dim3((unsigned)((threads + 255) / 256)), dim3(256), s, p, mx, rotary);
  });
}

hipError_t launch_decode_mx_step(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeMx& mx, const DecodeRotary* rotary,
                                 hipStream_t s) {
  if (f.fp8 || !f.ragged || !f.step || !mx_rotary_ok(D, rotary)) return hipErrorInvalidValue;
  if (p.l2norm && !mx_groups_ok(D, p.groups)) return hipErrorInvalidValue;
  return dispatch_chunk(dtype, D, [&](auto td) -> hipError_t {
    using T = typename decltype(td)::T;
    constexpr int DD = decltype(td)::D;
    constexpr int LDS = kDecodeBlock * kKvPitch<DD, 2>;
    const int64_t wgs = (int64_t)p.slots * p.Hk * p.splits;
    if (wgs <= 0) return hipSuccess;
    const dim3 grid((unsigned)wgs), block(64);
    auto go = [&](auto dyn) -> hipError_t {
      constexpr bool DY = decltype(dyn)::value;
      if (rotary != nullptr) return launch_part<rotary_decode_mx_kernel<T, DD, DY>, LDS>(grid, block, s, p, mx, *rotary);
      return launch_part<step_decode_mx_kernel<T, DD, DY>, LDS>(grid, block, s, p, mx);
    };
    return p.dyn ? go(std::true_type{}) : go(std::false_type{});
  });
}

}  // namespace fcsa
