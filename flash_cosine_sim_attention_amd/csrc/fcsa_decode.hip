// fcsa_decode.hip -- decoding against a key/value cache (fcsa_forward_kvcache, include/fcsa.h).
//
//   kv_append_kernel      k_new / v_new -> the cache slots [cache_seqlens[b], + new_len) below the capacity (through the block table when paged)
//   decode_kernel         one single-wave workgroup per (batch, K/V head, row tile, key split): the G = H / Hk query heads x N queries
//                         of the K/V head are the 16 rows of a tile, so each K/V byte is read once per row tile.  Keys stream straight
//                         from the cache into registers (one 16-byte load per lane and fragment), are l2-normalised there, and
//                         S^T = K^ Q^T runs on mfma_f32_16x16x32 (float32: 16x16x4) with the query row on the lane.  V goes through a
//                         wave-private LDS block for the transposed reads of O^T = V^T P~^T.  Partials (P~V, row max, row sum) in f32.
//                         The softmax step, the P~V product and the combine weight are functions of fcsa_decode_common.cuh (prefill too).
//   decode_combine_kernel reconciles the splits of every row (a per-split row max in the per-row-shift regime, a common shift
//                         otherwise) and normalises.
//   decode_combine_lse*   the same combine, also writing the rows' log-sum-exp (fcsa_forward_kvcache_lse): one body (decode_combine_body)
//                         behind every combine entry point, the LSE forms as entry points of their own.
// A ragged step (fcsa_forward_kvcache_varlen: packed queries, per-sequence counts) has entry points of its own as well --
// kv_append_ragged_kernel, decode_ragged[_fp8]_kernel (decode_body with RAGGED), decode_combine_ragged_kernel.
// An fp8 cache (fcsa_forward_kvcache_quant: one-byte OCP e4m3fn codes and a float32 scale per (batch, K/V head)) has entry points of its
// own -- kv_append_fp8_kernel, decode_fp8_kernel (decode_body with FP8), decode_combine_fp8_kernel -- so the kernels above are what
// they were.  A lane reads 8 key bytes per fragment (the same features as its 16-bit fragment) and converts them with v_cvt_pk_f32_fp8;
// every code is exact in f16 and bf16, so the operands of both MFMA products are what a 16-bit cache holding the codes would feed.
// An engine step (fcsa_forward_kvcache_step) has the decode and combine entry points of its decode side here --
// step_decode[_fp8]_kernel (decode_body with STEP), step_combine[_lse]_kernel -- and its chunk side in fcsa_prefill.hip.
// A tree step (fcsa_forward_kvcache_tree) is a ragged step whose decode launch reads a 64-bit visibility word per
// packed row -- decode_tree[_fp8]_kernel (decode_body with TREE; launch_decode_tree) -- between the ragged call's own append and combine;
// kv_compact_kernel (fcsa_kvcache_compact; launch_kv_compact) then moves the accepted path to the front of the slots the step appended.
// A call with a linear position bias (fcsa_forward_kvcache_alibi) is a ragged or engine step whose decode launch
// reads a slope per (sequence, head) -- alibi_decode[_fp8]_kernel (decode_body with ALIBI; launch_decode_alibi), per-row-shift regime only.
// The append is written once for every form: where a new row goes (append_pos: the cache_seqlens clamp and the drop at the capacity), the
// address of that position (cache_base of fcsa_decode_common.cuh, the readers' own rule) and the row write (append_chunk: a copy, or the
// quantisation of an fp8 cache).  The three append entry points are the index decomposition of their layout and calls to those.
// Host side: three launchers at the end of the file, one per job -- launch_kv_append, launch_decode, launch_decode_combine -- over one
// parameter block (DecodeStepParams, fcsa_kernels.h).  Each dispatches dtype, head dim and form (fp8, ragged, step) once, works out its
// grid once, and hands the entry point it picks the part of the block that entry point declares (launch_part, fcsa_decode_common.cuh).
#include "fcsa_common.cuh"
#include "fcsa_decode_common.cuh"

#include <cmath>
#include <type_traits>

namespace fcsa {

FCSA_TRACE_SITE(decode)

namespace {

// LDS plan of the decode kernel, for the kernel and its launcher: one 32-key V block, rows of D elements padded by 16 bytes; the form for
// group widths that straddle a lane's fragment (GEN) adds a float32 scratch of 16 rows x D squares and 16 rows x D group sums behind it
template <int D, int ES, bool GEN> struct DecodeLds {
  static constexpr int PITCH = kKvPitch<D, ES>;
  static constexpr int VBYTES = kDecodeBlock * PITCH;
  static constexpr int NORM = GEN ? 2 * kDecodeRows * D * 4 : 0;
  static constexpr int BYTES = VBYTES + NORM;
};

// Any group width (the GEN form: D = 96 with 48, 24, 12, 6 or 3 features per group, which straddle the lanes' fragments): each lane
// writes its squares to row (lane & 15) of an LDS scratch, the four lanes of the row sum every fourth group, and each element reads its
// group's sum back.  Same formula as group_normalise; only the order of the additions differs.
template <int NJ, int UE, int D> FCSA_DEV void group_normalise_lds(float (&x)[NJ][UE], int gs, float* scratch, int lane) {
  const int r = lane & 15, hi = lane >> 4;
  float* sq = scratch + r * D;
  float* gsum = scratch + kDecodeRows * D + r * D;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int f0 = (4 * j + hi) * UE;
    if (f0 < D) {
#pragma unroll
      for (int e = 0; e < UE; ++e) sq[f0 + e] = x[j][e] * x[j][e];
    }
  }
  __syncthreads();
  const int groups = D / gs;
  for (int g = hi; g < groups; g += 4) {
    float t = 0.f;
    for (int i = 0; i < gs; ++i) t += sq[g * gs + i];
    gsum[g] = t;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int f0 = (4 * j + hi) * UE;
#pragma unroll
    for (int e = 0; e < UE; ++e)
      if (f0 < D) x[j][e] *= 1.f / fmaxf(sqrtf(gsum[(f0 + e) / gs]), 1e-12f);
  }
  __syncthreads();      // the next row set rewrites the scratch
}

// FP8: the cache holds one-byte codes -- a K fragment is 8 bytes, a 16-byte V chunk 16 features (at D = 16 half the lanes have none)
template <typename T, int D, bool FP8 = false> struct DecodeRegs {
  static constexpr int ES = Traits<T>::ES;
  static constexpr int CES = FP8 ? 1 : ES;                         // bytes of a cache element
  static constexpr int UE = Unit<T>::UE;
  static constexpr int NJ = ES == 2 ? (D + 31) / 32 : D / 16;     // fragments of a row per lane
  static constexpr int CPR = D * CES / 16;                         // 16-byte chunks of a row
  static constexpr int VTOT = kDecodeBlock * CPR;                  // V chunks of a 32-key block
  static constexpr int VCH = (VTOT + 63) / 64;                     // ... per lane
  typedef std::conditional_t<FP8, u32x2, u32x4> KFrag;
  KFrag k[2][NJ];
  u32x4 v[VCH];

  // the 32-key block from `kb`, each 16-key half under the load rule (clamped_first, clamped_off)
  FCSA_DEV void load(const DecodeParams& p, int b, int kvh, int kb, int end, int lane) {
    const int x = lane & 15, hi = lane >> 4;
    const char* kbase[2];
    const char* vbase[2];
    int first[2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      first[sb] = clamped_first(kb + 16 * sb, end);
      kbase[sb] = cache_base(p, p.kc, b, kvh, first[sb]);
      vbase[sb] = cache_base(p, p.vc, b, kvh, first[sb]);
    }
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      const char* row = kbase[sb] + (int64_t)clamped_off(kb + 16 * sb + x, first[sb], end) * p.kc.sn;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int f = (4 * j + hi) * UE;
        k[sb][j] = f < D ? *reinterpret_cast<const KFrag*>(row + f * CES) : KFrag{};
      }
    }
#pragma unroll
    for (int t = 0; t < VCH; ++t) {
      const int c = lane + 64 * t, kk = c / CPR, ch = c % CPR, sb = kk >> 4;
      if constexpr (VTOT % 64 != 0) {
        if (c >= VTOT) { v[t] = u32x4{0u, 0u, 0u, 0u}; continue; }
      }
      const int off = clamped_off(kb + kk, sb ? first[1] : first[0], end);
      const u32x4 val = *reinterpret_cast<const u32x4*>((sb ? vbase[1] : vbase[0]) + (int64_t)off * p.vc.sn + ch * 16);
      v[t] = kb + kk < end ? val : u32x4{0u, 0u, 0u, 0u};
    }
  }
};

// WIN (decode_win_kernel): a sliding window -- the key range of the sequence starts at the 32-key block that holds the first key its
// first query sees (win_decode_first) instead of 0, and the window's two bounds join the visibility test
// FP8 (decode_fp8_kernel): an e4m3fn cache.  K: with l2norm the codes are scaled by k_scale, normalised and rounded as 16-bit keys are;
// without it the exact codes are the operands and k_scale joins the float32 logit multiplier.  V: converted to T on the way into LDS
// (exact); v_scale is applied by the combine.
// RAGGED (decode_ragged_kernel, decode_ragged_fp8_kernel): a ragged step -- packed queries, sequence b with its own N_b rows.  The
// workgroup is a (row-tile slot, K/V head, split); it finds its sequence and row tile in the table (ragged_tile: idle slots exit at once)
// and from there on runs the code below with N = N_b.  Always WIN, with open sides when the call has no window.
// STEP (step_decode_kernel, step_decode_fp8_kernel): the decode side of an engine step -- a ragged step whose workgroups leave the sequences
// of step_is_chunk to the chunk kernel (fcsa_prefill.hip) and exit as soon as they know their sequence.
// TREE (decode_tree_kernel, decode_tree_fp8_kernel): a tree step -- a ragged step without a window whose rows bring a 64-bit word each
// (tm.words, loaded once per lane next to last_key).  With P = L - N: a key before the step (key < P) is visible to every row, the step's
// token t (key P + t) iff bit t of the row's word is set; a sequence with N > 64 ignores its words and is causal.  Only the per-logit test
// differs from the ragged form: key range, splits, loads, both products and the partials are its own.
// ALIBI (alibi_decode_kernel, alibi_decode_fp8_kernel): a ragged or step form in the per-row-shift regime whose logits gain the linear
// position bias -slope[b, h] * |last_key - key| (al.slopes; alibi_slope / alibi_logit of fcsa_decode_common.cuh): the slope is loaded once per
// lane row, the float distance to the block once per block, and the bias joins the logit where the scale does, so the row max includes it.
template <typename T, int D, bool DYN, bool GEN, bool WIN, bool FP8 = false, bool RAGGED = false, bool STEP = false, bool TREE = false, bool ALIBI = false>
FCSA_DEV void decode_body(const std::conditional_t<STEP, DecodeStepParams, std::conditional_t<RAGGED, DecodeRaggedParams,
                                                   std::conditional_t<FP8, DecodeFp8Params, std::conditional_t<WIN, DecodeWinParams, DecodeParams>>>>& p,
                          const DecodeTreeMask& tm = DecodeTreeMask{}, const DecodeAlibi& al = DecodeAlibi{}) {
  static_assert(!FP8 || Traits<T>::ES == 2, "an fp8 cache is read with 16-bit queries");
  static_assert(!RAGGED || WIN, "the ragged entry points carry the window fields");
  static_assert(!STEP || RAGGED, "a step is a ragged step");
  static_assert(!TREE || (RAGGED && !STEP), "a tree step is a ragged step");
  static_assert(!ALIBI || (RAGGED && DYN && !TREE), "a position bias comes with the ragged and step forms, in the per-row-shift regime");
  typedef DecodeRegs<T, D, FP8> R;
  typedef DecodeLds<D, R::ES, GEN> LP;
  constexpr int ES = R::ES, UE = R::UE, NJ = R::NJ, CPR = R::CPR, VCH = R::VCH;
  constexpr int FB = D / 16;                       // 16-feature blocks of O^T
  constexpr bool PREFETCH = ES == 2;               // 16-bit: the next block's loads are in flight during this block's math
  extern __shared__ __attribute__((aligned(16))) char smem[];
  TraceRec<TraceSite_decode, kTraceWg, 0, false> tr;
  tr.start();

  const int lane = threadIdx.x, x = lane & 15, hi = lane >> 4;
  int id = blockIdx.x;
  const int split = id % p.splits;
  id /= p.splits;
  int rt, kvh, b, N, q0 = 0, new_len;     // q0: the sequence's first packed row (RAGGED)
  if constexpr (RAGGED) {
    kvh = id % p.Hk;
    if (!ragged_tile(p.cu_q, p.B, p.total_q, p.G, id / p.Hk, b, rt, q0, N)) return;
    if constexpr (STEP) {
      if (step_is_chunk(p.G, N, p.chunk_rows)) return;
    }
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
  if constexpr (WIN) {
    const int first = win_decode_first(L, N, p.win_lo);
    decode_window(L - first, split, p.splits, lo, n);
    lo += first;
  } else {
    decode_window(L, split, p.splits, lo, n);
  }
  const int end = lo + n;

  // this lane's query row: the column of every MFMA result
  const int r = rt * kDecodeRows + x;
  const bool row_ok = r < p.G * N;
  const int g = row_ok ? r / N : 0, qi = row_ok ? r % N : 0;
  const int h = kvh * p.G + g;
  const int last_key = L - N + qi;               // causal: key j is visible iff j <= last_key
  // TREE: the row's word (no bit for a row the tile does not have), the first position of the step and whether the words count
  [[maybe_unused]] uint64_t word = 0;
  [[maybe_unused]] const int P = L - N;
  [[maybe_unused]] const bool use_bits = N <= kCompactSlots;
  if constexpr (TREE) {
    if (row_ok) word = tm.words[q0 + qi];
  }
  [[maybe_unused]] float nslope = 0.f;
  if constexpr (ALIBI) nslope = alibi_slope(al, b, h);
  const int gs = D / p.groups;
  float* norm_scratch = reinterpret_cast<float*>(smem + LP::VBYTES);
  auto normalise = [&](float (&xr)[NJ][UE]) {
    if constexpr (GEN) group_normalise_lds<NJ, UE, D>(xr, gs, norm_scratch, lane);
    else group_normalise<NJ, UE>(xr, gs, D);
  };

  u32x4 qf[NJ];
  {
    float xq[NJ][UE];
    const char* qrow = p.q.p + (RAGGED ? 0 : (int64_t)b * p.q.sb) + (int64_t)h * p.q.sh + (int64_t)(q0 + qi) * p.q.sn;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int f = (4 * j + hi) * UE;
      const u32x4 u = (row_ok && f < D) ? *reinterpret_cast<const u32x4*>(qrow + f * ES) : u32x4{0u, 0u, 0u, 0u};
      unpack<T>(u, xq[j]);
    }
    if (p.l2norm) normalise(xq);
#pragma unroll
    for (int j = 0; j < NJ; ++j) qf[j] = pack<T>(xq[j], p.l2norm ? p.c1 : 1.f);     // c1 * q^, one rounding (the dense kernels' qn)
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

  R cur, nxt;
  if (PREFETCH && n > 0) cur.load(p, b, kvh, lo, end, lane);
  for (int kb = lo; kb < end; kb += kDecodeBlock) {
    if constexpr (PREFETCH) {
      if (kb + kDecodeBlock < end) nxt.load(p, b, kvh, kb + kDecodeBlock, end, lane);
    } else {
      cur.load(p, b, kvh, kb, end, lane);
    }
    // S^T = K^ Q^T for the two 16-key halves: s[sb][rr] = logit of key kb + 16 sb + 4 hi + rr for row x (log2 units)
    f32x4 s[2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      float xk[NJ][UE];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if constexpr (FP8) unpack_fp8(cur.k[sb][j], xk[j]);
        else unpack<T>(cur.k[sb][j], xk[j]);
      }
      if constexpr (FP8) {
        if (p.l2norm) {
#pragma unroll
          for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < UE; ++e) xk[j][e] *= kscale;
        }
      }
      if (p.l2norm) normalise(xk);
      [[maybe_unused]] float d0 = 0.f;             // ALIBI: from the row's position to the first key this lane holds of the block
      if constexpr (ALIBI) d0 = (float)(last_key - kb - 4 * hi);
      s[sb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const u32x4 kf = pack<T>(xk[j], 1.f);       // k^ rounded to the type, as the l2norm kernel writes it
        if constexpr (ES == 2) {
          s[sb] = Unit<T>::mfma(kf, qf[j], s[sb]);
        } else {
#pragma unroll
          for (int t = 0; t < 4; ++t) s[sb] = __builtin_amdgcn_mfma_f32_16x16x4f32(as_f32(kf[t]), as_f32(qf[j][t]), s[sb], 0, 0, 0);
        }
      }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int key = kb + 16 * sb + 4 * hi + rr;
        bool vis = key < end && (!p.causal || key <= last_key);
        if constexpr (WIN) vis = key < end && key <= last_key + p.win_hi && key >= last_key - p.win_lo;
        if constexpr (TREE) vis = key < end && (key < P || (use_bits ? ((word >> ((key - P) & 63)) & 1) != 0 : key <= last_key));
        if constexpr (ALIBI) s[sb][rr] = vis ? alibi_logit(s[sb][rr], smul, nslope, d0, 16 * sb + rr) : -INFINITY;
        else s[sb][rr] = vis ? s[sb][rr] * smul : -INFINITY;
      }
    }
    f32x4 pr[2];
    softmax_step<DYN>(s, m, l, acc, p.c2, pr);

    // V block -> LDS (row-major, padded rows), then O^T += V^T P~^T
#pragma unroll
    for (int t = 0; t < VCH; ++t) {
      const int c = lane + 64 * t;
      if constexpr (FP8) {
        if (R::VTOT % 64 == 0 || c < R::VTOT) {
          u32x4 w[2];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)cur.v[t][e], false), b2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)cur.v[t][e], true);
            w[e >> 1][2 * (e & 1)] = Traits<T>::pack2(a[0], a[1]);
            w[e >> 1][2 * (e & 1) + 1] = Traits<T>::pack2(b2[0], b2[1]);
          }
          u32x4* dst = reinterpret_cast<u32x4*>(smem + (c / CPR) * LP::PITCH + (c % CPR) * 32);
          dst[0] = w[0];
          dst[1] = w[1];
        }
      } else {
        *reinterpret_cast<u32x4*>(smem + (c / CPR) * LP::PITCH + (c % CPR) * 16) = cur.v[t];
      }
    }
    __syncthreads();
    if constexpr (ES == 2) {
      // k-slot (hi, e) of the P~V product is key 16 (e >> 2) + 4 hi + (e & 3): P~ is used where the first product left it
      u32x4 pb;
      pb[0] = Traits<T>::pack2(pr[0][0], pr[0][1]);
      pb[1] = Traits<T>::pack2(pr[0][2], pr[0][3]);
      pb[2] = Traits<T>::pack2(pr[1][0], pr[1][1]);
      pb[3] = Traits<T>::pack2(pr[1][2], pr[1][3]);
      pv_block<T, D, 1>(smem, 0, x, hi, &pb, &acc);
    } else {
#pragma unroll
      for (int fb = 0; fb < FB; ++fb)
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const float a = *reinterpret_cast<const float*>(smem + (16 * sb + 4 * hi + rr) * LP::PITCH + (16 * fb + x) * 4);
            acc[fb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, pr[sb][rr], acc[fb], 0, 0, 0);
          }
    }
    __syncthreads();
    if constexpr (PREFETCH) cur = nxt;
  }

  // partials of row x: O^T[16 fb + 4 hi + rr][x] in acc[fb][rr]; the row sum over the four lanes of the row
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (row_ok) {
    // partial rows: [B, H, N]; RAGGED: [total_q, H]
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
  tr.finish(Trace{}, 0, false, 0);
}

template <typename T, int D, bool DYN, bool GEN>
__global__ __launch_bounds__(64) void decode_kernel(DecodeParams p) {
  decode_body<T, D, DYN, GEN, false>(p);
}
// the sliding-window form (launch_decode, p.window): an entry point of its own, so that decode_kernel's instantiations are what they were
template <typename T, int D, bool DYN, bool GEN>
__global__ __launch_bounds__(64) void decode_win_kernel(DecodeWinParams p) {
  decode_body<T, D, DYN, GEN, true>(p);
}

template <typename T, int D, bool DYN, bool GEN, bool WIN>
__global__ __launch_bounds__(64) void decode_fp8_kernel(DecodeFp8Params p) {
  decode_body<T, D, DYN, GEN, WIN, true>(p);
}

// the ragged step (launch_decode with the ragged form): one entry point per cache type, with or without a window
template <typename T, int D, bool DYN, bool GEN>
__global__ __launch_bounds__(64) void decode_ragged_kernel(DecodeRaggedParams p) {
  decode_body<T, D, DYN, GEN, true, false, true>(p);
}
template <typename T, int D, bool DYN, bool GEN>
__global__ __launch_bounds__(64) void decode_ragged_fp8_kernel(DecodeRaggedParams p) {
  decode_body<T, D, DYN, GEN, true, true, true>(p);
}
// a tree step (launch_decode_tree): the ragged entry points' block, and the visibility words as a second argument
template <typename T, int D, bool DYN, bool GEN>
__global__ __launch_bounds__(64) void decode_tree_kernel(DecodeRaggedParams p, DecodeTreeMask tm) {
  decode_body<T, D, DYN, GEN, true, false, true, false, true>(p, tm);
}
template <typename T, int D, bool DYN, bool GEN>
__global__ __launch_bounds__(64) void decode_tree_fp8_kernel(DecodeRaggedParams p, DecodeTreeMask tm) {
  decode_body<T, D, DYN, GEN, true, true, true, false, true>(p, tm);
}
// a call with a linear position bias (launch_decode_alibi): the ragged entry points' block or, with STEP, the step entry points', and the
// slopes as a second argument.  The per-row-shift regime only.
template <typename T, int D, bool GEN, bool STEP>
__global__ __launch_bounds__(64) void alibi_decode_kernel(std::conditional_t<STEP, DecodeStepParams, DecodeRaggedParams> p, DecodeAlibi al) {
  decode_body<T, D, true, GEN, true, false, true, STEP, false, true>(p, DecodeTreeMask{}, al);
}
template <typename T, int D, bool GEN, bool STEP>
__global__ __launch_bounds__(64) void alibi_decode_fp8_kernel(std::conditional_t<STEP, DecodeStepParams, DecodeRaggedParams> p, DecodeAlibi al) {
  decode_body<T, D, true, GEN, true, true, true, STEP, false, true>(p, DecodeTreeMask{}, al);
}
// the decode side of an engine step (launch_decode with the step form): 16-bit types and D = 64 / 128, where every group width is reduced in registers
template <typename T, int D, bool DYN>
__global__ __launch_bounds__(64) void step_decode_kernel(DecodeStepParams p) {
  decode_body<T, D, DYN, false, true, false, true, true>(p);
}
template <typename T, int D, bool DYN>
__global__ __launch_bounds__(64) void step_decode_fp8_kernel(DecodeStepParams p) {
  decode_body<T, D, DYN, false, true, true, true, true>(p);
}

// The combine of one row's splits, shared by every combine entry point: o = sum_s 2^(m_s - M) P~V_s / sum_s 2^(m_s - M) l_s (static
// regime: every m_s is the common shift, weight 1).
// FP8: the cache's values are v_scale * code, so the row's v_scale joins the normaliser.
// RAGGED: partial row (tok, h) of the [total_q, H] rows goes to packed row `tok` of o; an fp8 cache's v_scale is that of the sequence
// owning the row (ragged_seq_of).
// LSE (decode_combine_lse*_kernel, fcsa_forward_kvcache_lse): the thread of the row's first four features also writes the row's
// log-sum-exp, from M and the UNCLAMPED l (decode_row_lse).  The statements that make o are the same either way.
// STEP (step_combine[_lse]_kernel): the rows of the sequences of step_is_chunk are the chunk kernel's: their threads exit before they read
// a partial (none was written).
template <typename T, int D, bool FP8, bool RAGGED, bool LSE, bool STEP = false, typename P>
FCSA_DEV void decode_combine_body(const P& p, const DecodeLseOut& lo) {
  constexpr int ES = Traits<T>::ES;
  constexpr int TPR = D / 4;                       // threads per row: four features each
  int64_t rows;
  if constexpr (RAGGED) rows = (int64_t)p.total_q * p.H;
  else rows = (int64_t)p.B * p.H * p.N;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / TPR;
  const int c = (int)(t % TPR);
  if (row >= rows) return;
  if constexpr (STEP) {
    const int64_t tok = row / p.H;
    const int b = ragged_seq_of(p.cu_q, p.B, p.total_q, tok);
    const int64_t q0 = ragged_cu(p.cu_q[b], p.total_q), q1 = max(ragged_cu(p.cu_q[b + 1], p.total_q), q0);      // ragged_tile's N_b
    if (step_is_chunk(p.G, q1 - q0, p.chunk_rows)) return;
  }
  float M = -INFINITY;
  for (int s = 0; s < p.splits; ++s) M = fmaxf(M, p.ws_ml[(s * rows + row) * 2]);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float l = 0.f;
  if (M != -INFINITY) {
    for (int s = 0; s < p.splits; ++s) {
      const f32x2 ml = *reinterpret_cast<const f32x2*>(p.ws_ml + (s * rows + row) * 2);
      const float w = combine_weight(ml[0], M);
      l += w * ml[1];
      acc += w * *reinterpret_cast<const f32x4*>(p.ws_o + (s * rows + row) * D + 4 * c);
    }
  }
  const float inv = combine_inv(p.dyn != 0, l, p.l_eps);
  int h;
  char* dst;
  if constexpr (RAGGED) {
    const int64_t tok = row / p.H;
    h = (int)(row % p.H);
    if constexpr (FP8) {
      const int b = ragged_seq_of(p.cu_q, p.B, p.total_q, tok);
      acc *= inv * p.v_scale[(int64_t)b * p.vs_b + (int64_t)(h / p.G) * p.vs_h];
    } else {
      acc *= inv;
    }
    dst = p.o.p + (int64_t)h * p.o.sh + tok * p.o.sn + 4 * c * ES;
    if constexpr (LSE) {
      if (c == 0) lo.lse[(int64_t)h * lo.sh + tok * lo.sn] = decode_row_lse(M, l);
    }
  } else {
    const int i = (int)(row % p.N);
    const int64_t bh = row / p.N;
    h = (int)(bh % p.H);
    const int b = (int)(bh / p.H);
    if constexpr (FP8) acc *= inv * p.v_scale[(int64_t)b * p.vs_b + (int64_t)(h / p.G) * p.vs_h];
    else acc *= inv;
    dst = p.o.p + (int64_t)b * p.o.sb + (int64_t)h * p.o.sh + (int64_t)i * p.o.sn + 4 * c * ES;
    if constexpr (LSE) {
      if (c == 0) lo.lse[(int64_t)b * lo.sb + (int64_t)h * lo.sh + (int64_t)i * lo.sn] = decode_row_lse(M, l);
    }
  }
  if constexpr (ES == 4) {
    *reinterpret_cast<f32x4*>(dst) = acc;
  } else {
    *reinterpret_cast<u32x2*>(dst) = u32x2{Traits<T>::pack2(acc[0], acc[1]), Traits<T>::pack2(acc[2], acc[3])};
  }
}

template <typename T, int D>
__global__ __launch_bounds__(256) void decode_combine_kernel(DecodeParams p) {
  decode_combine_body<T, D, false, false, false>(p, DecodeLseOut{});
}
// decode_combine_kernel for an fp8 cache (16-bit T)
template <typename T, int D>
__global__ __launch_bounds__(256) void decode_combine_fp8_kernel(DecodeFp8Params p) {
  decode_combine_body<T, D, true, false, false>(p, DecodeLseOut{});
}
// the combines that also write the rows' log-sum-exp: entry points of their own, so that the ones above are what they were
template <typename T, int D>
__global__ __launch_bounds__(256) void decode_combine_lse_kernel(DecodeParams p, DecodeLseOut lo) {
  decode_combine_body<T, D, false, false, true>(p, lo);
}
template <typename T, int D>
__global__ __launch_bounds__(256) void decode_combine_lse_fp8_kernel(DecodeFp8Params p, DecodeLseOut lo) {
  decode_combine_body<T, D, true, false, true>(p, lo);
}

// 16 elements of T (two 16-byte chunks) -> 16 e4m3fn codes: e4m3_rne(clamp(x / scale, -448, 448)).  The divide is the correctly rounded
// float32 one; the clamp is explicit, so saturation does not hang on the conversion's overflow mode; NaN passes the clamp as NaN.
template <typename T> FCSA_DEV u32x4 quantise16(const u32x4& a, const u32x4& b, float scale) {
  u32x4 out;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const u32x4& src = w < 2 ? a : b;
    float x[4] = {Traits<T>::lo(src[2 * (w & 1)]), Traits<T>::hi(src[2 * (w & 1)]), Traits<T>::lo(src[2 * (w & 1) + 1]), Traits<T>::hi(src[2 * (w & 1) + 1])};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float y = x[e] / scale;
      x[e] = y != y ? y : fminf(fmaxf(y, -448.f), 448.f);
    }
    int code = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0, false);
    code = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], code, true);
    out[w] = (uint32_t)code;
  }
  return out;
}

// ---- the append: one rule for where a new row goes, one row write, three entry points -----------------------------------------------
// Where new row `i` of sequence b goes: position clamp(cache_seqlens[b], 0, capacity) + i.  False: the row is dropped -- its position is at
// or beyond the capacity (every row, when seqlens is null: every sequence is full).  A position it gives is inside [0, capacity).
FCSA_DEV bool append_pos(const DecodeParams& p, int b, int64_t i, int& pos) {
  const int64_t start = p.seqlens != nullptr ? min(max((int64_t)p.seqlens[b], (int64_t)0), (int64_t)p.capacity) : (int64_t)p.capacity;
  if (start + i >= p.capacity) return false;
  pos = (int)(start + i);
  return true;
}

// 16-byte chunk `ch` of cache position `pos` (cache_base) of K and of V from the new rows at ksrc / vsrc: a copy, or (FP8, P = the fp8
// block) the codes of 32 source bytes under the (b, kvh) scales
template <typename T, bool FP8, typename P>
FCSA_DEV void append_chunk(const P& p, int b, int kvh, int pos, int ch, const char* ksrc, const char* vsrc) {
  u32x4* kdst = reinterpret_cast<u32x4*>(cache_base(p, p.kc, b, kvh, pos) + ch * 16);
  u32x4* vdst = reinterpret_cast<u32x4*>(cache_base(p, p.vc, b, kvh, pos) + ch * 16);
  if constexpr (FP8) {
    const u32x4* ks = reinterpret_cast<const u32x4*>(ksrc + ch * 32);
    const u32x4* vs = reinterpret_cast<const u32x4*>(vsrc + ch * 32);
    *kdst = quantise16<T>(ks[0], ks[1], p.k_scale[(int64_t)b * p.ks_b + (int64_t)kvh * p.ks_h]);
    *vdst = quantise16<T>(vs[0], vs[1], p.v_scale[(int64_t)b * p.vs_b + (int64_t)kvh * p.vs_h]);
  } else {
    *kdst = *reinterpret_cast<const u32x4*>(ksrc + ch * 16);
    *vdst = *reinterpret_cast<const u32x4*>(vsrc + ch * 16);
  }
}

// A rectangular append: one thread per 16 bytes WRITTEN of new row tn of (b, kvh) -- a 16-byte chunk of the row, or (FP8) 32 bytes of it
// that become 16 codes
template <typename T, int D, bool FP8, typename P>
FCSA_DEV void kv_append_body(const P& p) {
  constexpr int CPR = FP8 ? D / 16 : D * Traits<T>::ES / 16;
  const int64_t total = (int64_t)p.B * p.Hk * p.new_len * CPR;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int ch = (int)(t % CPR);
  int64_t rest = t / CPR;
  const int tn = (int)(rest % p.new_len);
  rest /= p.new_len;
  const int kvh = (int)(rest % p.Hk), b = (int)(rest / p.Hk);
  int pos;
  if (!append_pos(p, b, tn, pos)) return;
  append_chunk<T, FP8>(p, b, kvh, pos, ch, p.kn.p + (int64_t)b * p.kn.sb + (int64_t)kvh * p.kn.sh + (int64_t)tn * p.kn.sn,
                       p.vn.p + (int64_t)b * p.vn.sb + (int64_t)kvh * p.vn.sh + (int64_t)tn * p.vn.sn);
}
template <typename T, int D>
__global__ __launch_bounds__(256) void kv_append_kernel(DecodeParams p) {
  kv_append_body<T, D, false>(p);
}
template <typename T, int D>
__global__ __launch_bounds__(256) void kv_append_fp8_kernel(DecodeFp8Params p) {
  kv_append_body<T, D, true>(p);
}

// decode_combine_kernel / decode_combine_fp8_kernel for a ragged step, and the form that also writes the log-sum-exp of every packed row
template <typename T, int D, bool FP8>
__global__ __launch_bounds__(256) void decode_combine_ragged_kernel(DecodeRaggedParams p) {
  decode_combine_body<T, D, FP8, true, false>(p, DecodeLseOut{});
}
template <typename T, int D, bool FP8>
__global__ __launch_bounds__(256) void decode_combine_lse_ragged_kernel(DecodeRaggedParams p, DecodeLseOut lo) {
  decode_combine_body<T, D, FP8, true, true>(p, lo);
}

// the combine of an engine step's decode side (launch_decode_combine with the step form)
template <typename T, int D, bool FP8>
__global__ __launch_bounds__(256) void step_combine_kernel(DecodeStepParams p) {
  decode_combine_body<T, D, FP8, true, false, true>(p, DecodeLseOut{});
}
template <typename T, int D, bool FP8>
__global__ __launch_bounds__(256) void step_combine_lse_kernel(DecodeStepParams p, DecodeLseOut lo) {
  decode_combine_body<T, D, FP8, true, true, true>(p, lo);
}

// kv_append_kernel / kv_append_fp8_kernel for a ragged step: one thread per 16 bytes written of packed row `tok` of kn / vn ([total_q, Hk,
// D]); the thread finds the row's sequence in the table and writes slot cache_seqlens[b] + (tok - cu_q[b])
template <typename T, int D, bool FP8>
__global__ __launch_bounds__(256) void kv_append_ragged_kernel(DecodeRaggedParams p) {
  constexpr int CPR = FP8 ? D / 16 : D * Traits<T>::ES / 16;
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
  int pos;
  if (!append_pos(p, b, tok - q0, pos)) return;
  append_chunk<T, FP8>(p, b, kvh, pos, ch, p.kn.p + (int64_t)kvh * p.kn.sh + tok * p.kn.sn, p.vn.p + (int64_t)kvh * p.vn.sh + tok * p.vn.sn);
}

// ---- compaction of the accepted path of a tree step (fcsa_kvcache_compact) -----------------------------------------------------------
// One workgroup owns ALL moves of a (sequence, K/V head) pair: move i takes the row at position start + accepted[b, i] to start + i, K and
// V alike, start = clamp(cache_seqlens[b], 0, capacity).  Destination i of one move can be the source of another (accepted = [1, 2, 3, ...]
// shifts everything by one), so the workgroup reads every source row into LDS, passes a barrier and only then writes: no move is split
// across workgroups, and no write can reach a row another move still has to read.  Rows are bytes (16-byte chunks): every cache type, fp8
// codes included.  The tables are clamped -- num_accepted to [0, A], indices to [0, kCompactSlots) -- and a move whose source or
// destination is at or beyond the capacity is skipped, so nothing outside [start, start + kCompactSlots) is written whatever they hold.
// Dynamic LDS: 2 * A * row_bytes (K then V, move-major).
__global__ __launch_bounds__(256) void kv_compact_kernel(DecodeParams p, CompactParams c) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
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
  const int cpr = c.row_bytes / 16;               // 16-byte chunks of a row
  const int total = 2 * c.A * cpr;                // chunk id = (tensor * A + move) * cpr + chunk
  for (int id = threadIdx.x; id < total; id += 256) {
    const int ch = id % cpr, i = id / cpr % c.A, sp = src_pos[i];
    if (sp >= 0)
      *reinterpret_cast<u32x4*>(smem + (int64_t)id * 16) = *reinterpret_cast<const u32x4*>(cache_base(p, id / cpr < c.A ? p.kc : p.vc, b, kvh, sp) + ch * 16);
  }
  __syncthreads();
  for (int id = threadIdx.x; id < total; id += 256) {
    const int ch = id % cpr, i = id / cpr % c.A;
    if (src_pos[i] >= 0)
      *reinterpret_cast<u32x4*>(cache_base(p, id / cpr < c.A ? p.kc : p.vc, b, kvh, (int)(start + i)) + ch * 16) = *reinterpret_cast<const u32x4*>(smem + (int64_t)id * 16);
  }
}

int64_t blocks_of(int64_t threads) { return (threads + 255) / 256; }

// ---- the launchers: one per job (append, decode, combine) over every form of the call ----------------------------------------------
// The one dtype / head-dim / form dispatch: fn(TypeDim<T, D>, FP8, RAGGED), the flags as std::bool_constant.  An fp8 cache exists for the
// 16-bit types only, so nothing with FP8 is instantiated for float32.  f.step (an engine step) stays a run-time flag: each launcher picks
// the step entry points under `if constexpr (kStepKernels<...>)`, so they are instantiated where they exist and nowhere else.
template <typename F> hipError_t dispatch_decode(int dtype, int D, DecodeForm f, F&& fn) {
  if (f.step && !f.ragged) return hipErrorInvalidValue;      // a step is a ragged step
  return dispatch_dtype_d(dtype, D, [&](auto td) -> hipError_t {
    using Y = std::true_type;
    using N = std::false_type;
    if (f.fp8) {
      if constexpr (Traits<typename decltype(td)::T>::ES == 2) return f.ragged ? fn(td, Y{}, Y{}) : fn(td, Y{}, N{});
      else return hipErrorInvalidValue;
    }
    return f.ragged ? fn(td, N{}, Y{}) : fn(td, N{}, N{});
  });
}
// the step entry points exist for ragged calls where the chunk kernel does (16-bit types, D = 64 / 128: every group width is reduced in
// registers there, so there is no GEN form of them)
template <typename T, int D, bool RAGGED, bool GEN = false> constexpr bool kStepKernels = RAGGED && !GEN && kHasChunkKernel<T, D>;

}  // namespace

// one thread per 16 bytes WRITTEN of an appended row (an fp8 row is D bytes); ragged: the packed rows bring one key and value each.  The
// append of an engine step is the ragged call's (f.step is not looked at).
hipError_t launch_kv_append(int dtype, int D, DecodeForm f, const DecodeStepParams& p, hipStream_t s) {
  return dispatch_decode(dtype, D, f, [&](auto td, auto fp8, auto ragged) -> hipError_t {
    using T = typename decltype(td)::T;
    constexpr int DD = decltype(td)::D;
    constexpr bool FP8 = decltype(fp8)::value, RAGGED = decltype(ragged)::value;
    constexpr int CHUNKS = FP8 ? DD / 16 : DD * Traits<T>::ES / 16;
    const int64_t threads = (RAGGED ? (int64_t)p.total_q : (int64_t)p.B * p.new_len) * p.Hk * CHUNKS;
    if (threads <= 0 || (RAGGED && p.B <= 0)) return hipSuccess;
    const dim3 grid((unsigned)blocks_of(threads)), block(256);
    if constexpr (RAGGED) return launch_part<kv_append_ragged_kernel<T, DD, FP8>, 0>(grid, block, s, p);
    else if constexpr (FP8) return launch_part<kv_append_fp8_kernel<T, DD>, 0>(grid, block, s, p);
    else return launch_part<kv_append_kernel<T, DD>, 0>(grid, block, s, p);
  });
}

// one single-wave workgroup per (K/V head, row tile, key split): row_tiles per sequence, or the flat slots of a ragged step.  f.step: the
// step entry points over the slots of the FULL table (the slots of chunk sequences exit at once); nothing to launch without a workgroup.
hipError_t launch_decode(int dtype, int D, DecodeForm f, const DecodeStepParams& p, hipStream_t s) {
  return dispatch_decode(dtype, D, f, [&](auto td, auto fp8, auto ragged) -> hipError_t {
    using T = typename decltype(td)::T;
    constexpr int DD = decltype(td)::D;
    constexpr int ES = Traits<T>::ES;
    constexpr bool FP8 = decltype(fp8)::value, RAGGED = decltype(ragged)::value;
    if (f.step && !kStepKernels<T, DD, RAGGED>) return hipErrorInvalidValue;
    const int64_t wgs = (RAGGED ? (int64_t)p.slots : (int64_t)p.B * p.row_tiles) * p.Hk * p.splits;
    const dim3 grid((unsigned)wgs), block(64);
    auto go = [&](auto dyn, auto gen) -> hipError_t {
      constexpr bool DY = decltype(dyn)::value, GN = decltype(gen)::value;
      constexpr int LDS = DecodeLds<DD, ES, GN>::BYTES;
      if constexpr (kStepKernels<T, DD, RAGGED, GN>) {
        if (f.step) {
          if (wgs <= 0) return hipSuccess;
          if constexpr (FP8) return launch_part<step_decode_fp8_kernel<T, DD, DY>, LDS>(grid, block, s, p);
          else return launch_part<step_decode_kernel<T, DD, DY>, LDS>(grid, block, s, p);
        }
      }
      if constexpr (RAGGED && FP8) return launch_part<decode_ragged_fp8_kernel<T, DD, DY, GN>, LDS>(grid, block, s, p);
      else if constexpr (RAGGED) return launch_part<decode_ragged_kernel<T, DD, DY, GN>, LDS>(grid, block, s, p);
      else if constexpr (FP8) return p.window ? launch_part<decode_fp8_kernel<T, DD, DY, GN, true>, LDS>(grid, block, s, p)
                                              : launch_part<decode_fp8_kernel<T, DD, DY, GN, false>, LDS>(grid, block, s, p);
      else return p.window ? launch_part<decode_win_kernel<T, DD, DY, GN>, LDS>(grid, block, s, p)
                           : launch_part<decode_kernel<T, DD, DY, GN>, LDS>(grid, block, s, p);
    };
    using Y = std::true_type;
    using N = std::false_type;
    // group widths that straddle the lanes' fragments exist at D = 96 only (decode_groups_fast holds for every divisor of the others)
    if (p.l2norm && !decode_groups_fast(DD, p.groups, Unit<T>::UE)) {
      if constexpr (DD == 96) return p.dyn ? go(Y{}, Y{}) : go(N{}, Y{});
      else return hipErrorInvalidValue;
    }
    return p.dyn ? go(Y{}, N{}) : go(N{}, N{});
  });
}

// one thread per four features of an output row; lse: nullptr, or the entry points that also write the rows' log-sum-exp.  f.step: the
// step entry points (the rows of chunk sequences exit at once); nothing to launch without a sequence.
hipError_t launch_decode_combine(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeLseOut* lse, hipStream_t s) {
  return dispatch_decode(dtype, D, f, [&](auto td, auto fp8, auto ragged) -> hipError_t {
    using T = typename decltype(td)::T;
    constexpr int DD = decltype(td)::D;
    constexpr bool FP8 = decltype(fp8)::value, RAGGED = decltype(ragged)::value;
    if (f.step && !kStepKernels<T, DD, RAGGED>) return hipErrorInvalidValue;
    const int64_t threads = (RAGGED ? (int64_t)p.total_q : (int64_t)p.B * p.N) * p.H * (DD / 4);
    if (threads <= 0 || (f.step && p.B <= 0)) return hipSuccess;
    const dim3 grid((unsigned)blocks_of(threads)), block(256);
    if constexpr (kStepKernels<T, DD, RAGGED>) {
      if (f.step) return lse != nullptr ? launch_part<step_combine_lse_kernel<T, DD, FP8>, 0>(grid, block, s, p, *lse)
                                        : launch_part<step_combine_kernel<T, DD, FP8>, 0>(grid, block, s, p);
    }
    if (lse != nullptr) {
      if constexpr (RAGGED) return launch_part<decode_combine_lse_ragged_kernel<T, DD, FP8>, 0>(grid, block, s, p, *lse);
      else if constexpr (FP8) return launch_part<decode_combine_lse_fp8_kernel<T, DD>, 0>(grid, block, s, p, *lse);
      else return launch_part<decode_combine_lse_kernel<T, DD>, 0>(grid, block, s, p, *lse);
    }
    if constexpr (RAGGED) return launch_part<decode_combine_ragged_kernel<T, DD, FP8>, 0>(grid, block, s, p);
    else if constexpr (FP8) return launch_part<decode_combine_fp8_kernel<T, DD>, 0>(grid, block, s, p);
    else return launch_part<decode_combine_kernel<T, DD>, 0>(grid, block, s, p);
  });
}

// launch_decode's ragged form on the entry points that take the visibility words: the same workgroups, block and LDS
hipError_t launch_decode_tree(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeTreeMask& tree, hipStream_t s) {
  if (!f.ragged || f.step || tree.words == nullptr) return hipErrorInvalidValue;
  return dispatch_decode(dtype, D, f, [&](auto td, auto fp8, auto ragged) -> hipError_t {
    using T = typename decltype(td)::T;
    constexpr int DD = decltype(td)::D;
    constexpr int ES = Traits<T>::ES;
    constexpr bool FP8 = decltype(fp8)::value, RAGGED = decltype(ragged)::value;
    if constexpr (!RAGGED) {
      return hipErrorInvalidValue;
    } else {
      const int64_t wgs = (int64_t)p.slots * p.Hk * p.splits;
      const dim3 grid((unsigned)wgs), block(64);
      auto go = [&](auto dyn, auto gen) -> hipError_t {
        constexpr bool DY = decltype(dyn)::value, GN = decltype(gen)::value;
        constexpr int LDS = DecodeLds<DD, ES, GN>::BYTES;
        if constexpr (FP8) return launch_part<decode_tree_fp8_kernel<T, DD, DY, GN>, LDS>(grid, block, s, p, tree);
        else return launch_part<decode_tree_kernel<T, DD, DY, GN>, LDS>(grid, block, s, p, tree);
      };
      using Y = std::true_type;
      using N = std::false_type;
      if (p.l2norm && !decode_groups_fast(DD, p.groups, Unit<T>::UE)) {
        if constexpr (DD == 96) return p.dyn ? go(Y{}, Y{}) : go(N{}, Y{});
        else return hipErrorInvalidValue;
      }
      return p.dyn ? go(Y{}, N{}) : go(N{}, N{});
    }
  });
}

// launch_decode's ragged form -- or, where the step kernels exist, its step form: f.step must say which (one form per problem is
// compiled) -- on the entry points that take the slopes: the same workgroups, block and LDS.  The per-row-shift regime only.
hipError_t launch_decode_alibi(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeAlibi& alibi, hipStream_t s) {
  if (!f.ragged || !p.dyn || alibi.slopes == nullptr) return hipErrorInvalidValue;
  return dispatch_decode(dtype, D, f, [&](auto td, auto fp8, auto ragged) -> hipError_t {
    using T = typename decltype(td)::T;
    constexpr int DD = decltype(td)::D;
    constexpr int ES = Traits<T>::ES;
    constexpr bool FP8 = decltype(fp8)::value, RAGGED = decltype(ragged)::value;
    if constexpr (!RAGGED) {
      return hipErrorInvalidValue;
    } else {
      constexpr bool STEP = kStepKernels<T, DD, RAGGED>;
      if (f.step != STEP) return hipErrorInvalidValue;
      const int64_t wgs = (int64_t)p.slots * p.Hk * p.splits;
      if (wgs <= 0) return hipSuccess;
      const dim3 grid((unsigned)wgs), block(64);
      auto go = [&](auto gen) -> hipError_t {
        constexpr bool GN = decltype(gen)::value;
        constexpr int LDS = DecodeLds<DD, ES, GN>::BYTES;
        if constexpr (FP8) return launch_part<alibi_decode_fp8_kernel<T, DD, GN, STEP>, LDS>(grid, block, s, p, alibi);
        else return launch_part<alibi_decode_kernel<T, DD, GN, STEP>, LDS>(grid, block, s, p, alibi);
      };
      if (p.l2norm && !decode_groups_fast(DD, p.groups, Unit<T>::UE)) {
        if constexpr (DD == 96) return go(std::true_type{});
        else return hipErrorInvalidValue;
      }
      return go(std::false_type{});
    }
  });
}

// one workgroup per (sequence, K/V head); the LDS limit is raised once per device to the largest stage (64 rows of 512 bytes, twice)
hipError_t launch_kv_compact(const DecodeParams& cache, const CompactParams& c, hipStream_t s) {
  constexpr int kMaxRowBytes = 512;
  if (c.A < 1 || c.A > kCompactSlots || c.row_bytes < 16 || c.row_bytes % 16 != 0 || c.row_bytes > kMaxRowBytes) return hipErrorInvalidValue;
  if (cache.B <= 0 || cache.Hk <= 0) return hipSuccess;
  static std::atomic<uint64_t> done{0};
  if (hipError_t e = ensure_dynamic_lds(kv_compact_kernel, 2 * kCompactSlots * kMaxRowBytes, done); e != hipSuccess) return e;
  hipLaunchKernelGGL(kv_compact_kernel, dim3((unsigned)((int64_t)cache.B * cache.Hk)), dim3(256), (size_t)2 * c.A * c.row_bytes, s, cache, c);
  return hipGetLastError();
}

}  // namespace fcsa
