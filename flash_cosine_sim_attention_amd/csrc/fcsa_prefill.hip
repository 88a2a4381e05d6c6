// fcsa_prefill.hip -- a prompt chunk against the key/value cache (fcsa_forward_kvcache_prefill, include/fcsa.h).
//
//   prefill_kernel   one 4-wave workgroup per (row-tile slot, K/V head): 128 token-major rows (r = i * G + g) of one sequence's K/V head, two
//                    16-row MFMA tiles per wave.  The keys [0, kend) of the tile (prefill_kend: under `causal` it stops at the last key the
//                    tile's last token sees) go through LDS in 64-key stages, double-buffered: wave w loads the stage's keys 16 w ... 16 w + 15
//                    in the decode kernel's register layout (key on lane & 15, feature quarter on lane >> 4), l2-normalises them with the
//                    decode kernel's group_normalise, rounds them to the type and writes K^ -- once per workgroup, not once per 16 rows --
//                    and V raw.  The next stage's global loads are in flight during the current stage's math.
//                    Per wave, 32-key block and row tile the math is decode_body's (S^T = K^ Q^T on mfma_f32_16x16x32 with the query row on
//                    the lane, its mask and P~ pack, and the same functions of fcsa_decode_common.cuh: softmax_step, pv_block), and the
//                    epilogue is decode_combine_body's (combine_weight, combine_inv) at one split, so o and lse are bit for bit those of
//                    the ragged call with one key split.  Every K^ fragment and transposed V read from LDS feeds both row tiles of the wave.
//   step_prefill_kernel  the chunk side of an engine step (fcsa_forward_kvcache_step): the same body (prefill_body)
//                    with up to three additions.  STEP: a workgroup whose sequence is no chunk (step_is_chunk) exits -- those rows are the
//                    step decode kernels'.  WIN: the ragged kernel's visibility test, and a key range that starts at the LDS stage holding the
//                    first key the tile's first token sees (prefill_kstart).  FP8: an e4m3fn cache -- a lane loads 8 bytes per K and V fragment,
//                    K becomes K^ exactly as decode_body<FP8> makes it, V's codes are converted to the type on the way into LDS, and the
//                    epilogue multiplies by v_scale as decode_combine_body<FP8> does.
//   alibi_prefill_kernel  the chunk side of a call with a linear position bias (fcsa_forward_kvcache_alibi): the
//                    windowed step form in the per-row-shift regime with ALIBI -- the slopes as a third kernel argument (launch_prefill_alibi).
// The append before it is the ragged call's (launch_kv_append with the same parameter block).  16-bit types, D = 64 / 128 only.
// Host side: one launcher, launch_prefill, for both entry points -- one copy of the refusals and of the grid; the form (DecodeForm::step,
// fp8, and the window sides of the block) picks the entry point, which gets the part of the block it declares (launch_part).
#include "fcsa_common.cuh"
#include "fcsa_decode_common.cuh"

#include <cmath>
#include <type_traits>

namespace fcsa {

namespace {

constexpr int kPrefillWaves = 4;
constexpr int kPrefillTiles = kPrefillRows / kDecodeRows / kPrefillWaves;     // 16-row MFMA tiles per wave

// LDS plan, for the kernel and its launcher: two stage buffers, each K^ [64][PITCH] then V [64][PITCH] at the pitch pv_block reads
template <int D> struct PrefillLds {
  static constexpr int PITCH = kKvPitch<D, 2>;
  static constexpr int TILE = kPrefillStage * PITCH;
  static constexpr int BUF = 2 * TILE;
  static constexpr int BYTES = 2 * BUF;
};

// A wave's 16 keys of a stage in registers: lane (x, hi) holds features (4 j + hi) * 8 ... + 7 of key `first16 + x` of K and of V
// FP8: the same features as one-byte codes (DecodeRegs<T, D, true>'s K layout, for K and V alike)
template <typename T, int D, bool FP8 = false> struct PrefillRegs {
  static constexpr int NJ = D / 32;
  static constexpr int CES = FP8 ? 1 : 2;                          // bytes of a cache element
  typedef std::conditional_t<FP8, u32x2, u32x4> Frag;
  Frag k[NJ], v[NJ];

  // the 16 positions from first16 of a sequence of L, under the load rule (clamped_first, clamped_off)
  FCSA_DEV void load(const DecodeParams& p, int b, int kvh, int first16, int L, int lane) {
    const int x = lane & 15, hi = lane >> 4;
    const int first = clamped_first(first16, L);
    const int off = clamped_off(first16 + x, first, L);
    const char* krow = cache_base(p, p.kc, b, kvh, first) + (int64_t)off * p.kc.sn;
    const char* vrow = cache_base(p, p.vc, b, kvh, first) + (int64_t)off * p.vc.sn;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int f = (4 * j + hi) * 8;
      k[j] = *reinterpret_cast<const Frag*>(krow + f * CES);
      const Frag val = *reinterpret_cast<const Frag*>(vrow + f * CES);
      v[j] = first16 + x < L ? val : Frag{};
    }
  }

  // K^ (normalised and rounded as decode_body does before its first product) and raw V -> row `row` of a stage buffer
  // FP8: V's codes converted to T (exact); K's codes times kscale under l2norm (decode_body<FP8>: otherwise kscale is in the logit multiplier)
  FCSA_DEV void store(char* buf, int row, int lane, bool l2norm, int gs, float kscale = 1.f) const {
    constexpr int PITCH = PrefillLds<D>::PITCH;
    const int hi = lane >> 4;
    float xk[NJ][8];
    if constexpr (FP8) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        float xv[8];
        unpack_fp8(v[j], xv);
        *reinterpret_cast<u32x4*>(buf + PrefillLds<D>::TILE + row * PITCH + (4 * j + hi) * 16) = pack<T>(xv, 1.f);
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
      for (int j = 0; j < NJ; ++j) *reinterpret_cast<u32x4*>(buf + PrefillLds<D>::TILE + row * PITCH + (4 * j + hi) * 16) = v[j];
#pragma unroll
      for (int j = 0; j < NJ; ++j) unpack<T>(k[j], xk[j]);
    }
    if (l2norm) group_normalise<NJ, 8>(xk, gs, D);
#pragma unroll
    for (int j = 0; j < NJ; ++j) *reinterpret_cast<u32x4*>(buf + row * PITCH + (4 * j + hi) * 16) = pack<T>(xk[j], 1.f);
  }
};

// Waves per SIMD the register allocation aims at: two (two workgroups per CU, at most 256 registers) wherever that leaves no scratch.  The
// f16 D = 128 instantiations take 257 - 259 registers and spill 1 - 9 of them when held to 256 (bf16: 253 - 255, none), so they run one wave
// per SIMD.
template <typename T, int D> constexpr int kPrefillWavesPerSimd = (std::is_same_v<T, F16> && D == 128) ? 1 : 2;

// ... and of the step forms (step_prefill_kernel): the plain and windowed forms as above (f16 D = 128: 257 - 260 registers); an fp8 cache's
// key and value fragments are half as wide in registers, and every fp8 form stays below 256 (247 - 249 at D = 128, no scratch)
template <typename T, int D, bool WIN, bool FP8> constexpr int kStepPrefillWavesPerSimd = FP8 ? 2 : kPrefillWavesPerSimd<T, D>;

// ... and of the forms with a position bias (alibi_prefill_kernel; profiles/alibi_resources.txt): the slopes and the float distances take the
// bf16 D = 128 form on a 16-bit cache past 256 registers too (24 bytes of scratch when held to them), so both 16-bit-cache forms at D = 128 run
// one wave per SIMD; the fp8 forms stay at 253, no scratch
template <typename T, int D, bool FP8> constexpr int kAlibiPrefillWavesPerSimd = (!FP8 && D == 128) ? 1 : 2;

// ALIBI (alibi_prefill_kernel): the windowed step form in the per-row-shift regime whose logits gain the linear position bias of
// decode_body<ALIBI> -- the same two functions (alibi_slope, alibi_logit), the slope once per lane row, the float distance once per block.
template <typename T, int D, bool DYN, bool STEP = false, bool WIN = false, bool FP8 = false, bool ALIBI = false>
FCSA_DEV void prefill_body(const std::conditional_t<STEP, DecodeStepParams, DecodeRaggedParams>& p, const DecodeLseOut& lo,
                           const DecodeAlibi& al = DecodeAlibi{}) {
  static_assert(STEP || (!WIN && !FP8), "windows and fp8 caches come with the step entry points");
  static_assert(!ALIBI || (STEP && WIN && DYN), "a position bias comes with the windowed step form, in the per-row-shift regime");
  typedef PrefillLds<D> LP;
  typedef PrefillRegs<T, D, FP8> R;
  constexpr int NJ = R::NJ, FB = D / 16, NT = kPrefillTiles;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int lane = threadIdx.x & 63, x = lane & 15, hi = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kvh = blockIdx.x % p.Hk;
  int b, rt, q0, N;
  if (!prefill_tile(p.cu_q, p.B, p.total_q, p.G, kPrefillRows, blockIdx.x / p.Hk, b, rt, q0, N)) return;
  if constexpr (STEP) {
    if (!step_is_chunk(p.G, N, p.chunk_rows)) return;
  }
  const int L = decode_len(p.seqlens != nullptr, p.seqlens != nullptr ? p.seqlens[b] : 0, p.append ? N : 0, p.capacity);
  const int64_t row0 = (int64_t)rt * kPrefillRows;
  // the tile's keys [kstart, kend): kstart a whole number of stages (0 without a window)
  int kstart = 0, kend, wave_kend;
  // a wave stops at the last key its own 32 rows see; it still loads its share of every stage and joins every barrier
  if constexpr (WIN) {
    kstart = prefill_kstart(L, N, p.G, row0, p.win_lo);
    kend = prefill_win_kend(L, N, p.G, row0, kPrefillRows, p.win_hi);
    wave_kend = prefill_win_kend(L, N, p.G, row0 + wave * (NT * kDecodeRows), NT * kDecodeRows, p.win_hi);
  } else {
    kend = prefill_kend(L, N, p.G, row0, kPrefillRows, p.causal != 0);
    wave_kend = prefill_kend(L, N, p.G, row0 + wave * (NT * kDecodeRows), NT * kDecodeRows, p.causal != 0);
  }
  const int gs = D / p.groups;

  // this lane's query rows, one per row tile: the column of every MFMA result
  int last_key[NT];
  [[maybe_unused]] float nslope[NT];
  u32x4 qf[NT][NJ];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int64_t r = row0 + (wave * NT + t) * kDecodeRows + x;
    const bool row_ok = r < (int64_t)p.G * N;
    const int g = row_ok ? (int)(r % p.G) : 0, qi = row_ok ? (int)(r / p.G) : 0;
    last_key[t] = L - N + qi;                  // causal: key j is visible iff j <= last_key
    if constexpr (ALIBI) nslope[t] = alibi_slope(al, b, kvh * p.G + g);
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
    for (int j = 0; j < NJ; ++j) qf[t][j] = pack<T>(xq[j], p.l2norm ? p.c1 : 1.f);     // c1 * q^, one rounding
  }
  float smul = p.l2norm ? 1.f : p.c1;
  float kscale = 1.f;
  if constexpr (FP8) {
    kscale = p.k_scale[(int64_t)b * p.ks_b + (int64_t)kvh * p.ks_h];
    if (!p.l2norm) smul *= kscale;
  }

  f32x4 acc[NT][FB];
  float m[NT], l[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) acc[t][fb] = f32x4{0.f, 0.f, 0.f, 0.f};
    m[t] = DYN ? -INFINITY : p.c2;
    l[t] = 0.f;
  }

  int stages = (kend + kPrefillStage - 1) / kPrefillStage;
  if constexpr (WIN) stages = kend > kstart ? (kend - kstart + kPrefillStage - 1) / kPrefillStage : 0;
  const int my_row = wave * 16 + x;              // the stage row this lane loads
  R regs;
  if (stages > 0) {
    regs.load(p, b, kvh, kstart + wave * 16, L, lane);
    if constexpr (FP8) regs.store(smem, my_row, lane, p.l2norm != 0, gs, kscale);
    else regs.store(smem, my_row, lane, p.l2norm != 0, gs);
  }
  __syncthreads();
  for (int st = 0; st < stages; ++st) {
    const bool more = st + 1 < stages;
    if (more) regs.load(p, b, kvh, kstart + (st + 1) * kPrefillStage + wave * 16, L, lane);
    const char* ks = smem + (st & 1) * LP::BUF;
    const char* vs = ks + LP::TILE;
#pragma unroll
    for (int blk = 0; blk < kPrefillStage / kDecodeBlock; ++blk) {
      const int kb = kstart + st * kPrefillStage + blk * kDecodeBlock;
      if (kb >= wave_kend) break;
      // S^T = K^ Q^T for the two 16-key halves: s[t][sb][rr] = logit of key kb + 16 sb + 4 hi + rr for row x of tile t (log2 units)
      f32x4 s[NT][2];
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) {
#pragma unroll
        for (int t = 0; t < NT; ++t) s[t][sb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const u32x4 kf = *reinterpret_cast<const u32x4*>(ks + (blk * kDecodeBlock + 16 * sb + x) * LP::PITCH + (4 * j + hi) * 16);
#pragma unroll
          for (int t = 0; t < NT; ++t) s[t][sb] = Unit<T>::mfma(kf, qf[t][j], s[t][sb]);
        }
      }
      u32x4 pb[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        [[maybe_unused]] float d0 = 0.f;           // ALIBI: from the row's position to the first key this lane holds of the block
        if constexpr (ALIBI) d0 = (float)(last_key[t] - kb - 4 * hi);
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int key = kb + 16 * sb + 4 * hi + rr;
            bool vis = key < L && (!p.causal || key <= last_key[t]);
            if constexpr (WIN) vis = key < L && key <= last_key[t] + p.win_hi && key >= last_key[t] - p.win_lo;
            if constexpr (ALIBI) s[t][sb][rr] = vis ? alibi_logit(s[t][sb][rr], smul, nslope[t], d0, 16 * sb + rr) : -INFINITY;
            else s[t][sb][rr] = vis ? s[t][sb][rr] * smul : -INFINITY;
          }
        f32x4 pr[2];
        softmax_step<DYN>(s[t], m[t], l[t], acc[t], p.c2, pr);
        // k-slot (hi, e) of the P~V product is key 16 (e >> 2) + 4 hi + (e & 3): P~ is used where the first product left it
        pb[t][0] = Traits<T>::pack2(pr[0][0], pr[0][1]);
        pb[t][1] = Traits<T>::pack2(pr[0][2], pr[0][3]);
        pb[t][2] = Traits<T>::pack2(pr[1][0], pr[1][1]);
        pb[t][3] = Traits<T>::pack2(pr[1][2], pr[1][3]);
      }
      pv_block<T, D, NT>(vs, blk * kDecodeBlock, x, hi, pb, acc);
    }
    // the other buffer was last read before the barrier that ended the previous iteration
    if constexpr (FP8) {
      if (more) regs.store(smem + ((st + 1) & 1) * LP::BUF, my_row, lane, p.l2norm != 0, gs, kscale);
    } else {
      if (more) regs.store(smem + ((st + 1) & 1) * LP::BUF, my_row, lane, p.l2norm != 0, gs);
    }
    __syncthreads();
  }

  // Row x of tile t: O^T[16 fb + 4 hi + rr][x] in acc[t][fb][rr].  The combine of its one split (decode_combine_body's functions), in registers.
  // The row's head and token are worked out again here (from an opaque lane id), so that no address lives through the key loop.
  const int xe = opaque(lane) & 15, hie = opaque(lane) >> 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    float ls = l[t];
    ls += __shfl_xor(ls, 16, 64);
    ls += __shfl_xor(ls, 32, 64);
    const int64_t r = row0 + (wave * NT + t) * kDecodeRows + xe;
    if (r >= (int64_t)p.G * N) continue;
    const int h = kvh * p.G + (int)(r % p.G);
    const int64_t tok = q0 + r / p.G;
    const float M = m[t];
    const bool any = M != -INFINITY;
    const float w = combine_weight(M, M);      // the one split's weight: 1
    float lsum = 0.f;
    if (any) lsum += w * ls;
    float inv = combine_inv(p.dyn != 0, lsum, p.l_eps);
    if constexpr (FP8) inv = inv * p.v_scale[(int64_t)b * p.vs_b + (int64_t)kvh * p.vs_h];      // decode_combine_body<FP8>: acc *= inv * v_scale
    char* dst = p.o.p + (int64_t)h * p.o.sh + tok * p.o.sn + 4 * hie * 2;
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      if (any) a += w * acc[t][fb];
      a *= inv;
      *reinterpret_cast<u32x2*>(dst + 16 * fb * 2) = u32x2{Traits<T>::pack2(a[0], a[1]), Traits<T>::pack2(a[2], a[3])};
    }
    if (lo.lse != nullptr && hie == 0) lo.lse[(int64_t)h * lo.sh + tok * lo.sn] = decode_row_lse(M, lsum);
  }
}

template <typename T, int D, bool DYN>
__global__ __launch_bounds__(64 * kPrefillWaves, (kPrefillWavesPerSimd<T, D>)) void prefill_kernel(DecodeRaggedParams p, DecodeLseOut lo) {
  prefill_body<T, D, DYN>(p, lo);
}

// The chunk side of an engine step: entry points of their own, so that prefill_kernel's instantiations are what they were.  Un-windowed
// calls on 16-bit caches take the plain form (WIN = false: prefill_kernel's code behind the routing test); an fp8 cache always takes the
// windowed form, with open sides when the call has no window, as the ragged kernel does.
template <typename T, int D, bool DYN, bool WIN, bool FP8>
__global__ __launch_bounds__(64 * kPrefillWaves, (kStepPrefillWavesPerSimd<T, D, WIN, FP8>)) void step_prefill_kernel(DecodeStepParams p, DecodeLseOut lo) {
  prefill_body<T, D, DYN, true, WIN, FP8>(p, lo);
}

// The chunk side of a call with a linear position bias (launch_prefill_alibi): the windowed step form with the slopes as a third argument.
template <typename T, int D, bool FP8>
__global__ __launch_bounds__(64 * kPrefillWaves, (kAlibiPrefillWavesPerSimd<T, D, FP8>)) void alibi_prefill_kernel(DecodeStepParams p, DecodeLseOut lo,
                                                                                                                 DecodeAlibi al) {
  prefill_body<T, D, true, true, true, FP8, true>(p, lo, al);
}

}  // namespace

// One 4-wave workgroup per (row-tile slot of 128 rows, K/V head): p.slots = fcsa::prefill_slots(total_q, B, G, kPrefillRows).  lse: nullptr,
// or where the rows' log-sum-exp goes as well.  f.step: the chunk side of an engine step (the workgroups of decode sequences exit at
// once), which has the forms for a window and an fp8 cache; without it an fp8 cache is refused -- prefill_kernel has no such form.
hipError_t launch_prefill(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeLseOut* lse, hipStream_t s) {
  if (f.fp8 && !f.step) return hipErrorInvalidValue;
  return dispatch_chunk(dtype, D, [&](auto td) -> hipError_t {
    using T = typename decltype(td)::T;
    constexpr int DD = decltype(td)::D;
    constexpr int LDS = PrefillLds<DD>::BYTES;
    if (p.l2norm && !decode_groups_fast(DD, p.groups, 8)) return hipErrorInvalidValue;
    if ((int64_t)p.slots * p.Hk <= 0) return hipSuccess;
    const dim3 grid((unsigned)((int64_t)p.slots * p.Hk)), block(64 * kPrefillWaves);
    const DecodeLseOut lo = lse != nullptr ? *lse : DecodeLseOut{};
    // the window test is needed when a side is bounded on the left or strictly inside on the right (open and causal sides are prefill_kernel's)
    const bool win = p.win_lo < kWinOpen || (p.win_hi < kWinOpen && !(p.causal && p.win_hi == 0));
    auto go = [&](auto dyn) -> hipError_t {
      constexpr bool DY = decltype(dyn)::value;
      if (!f.step) return launch_part<prefill_kernel<T, DD, DY>, LDS>(grid, block, s, p, lo);
      if (f.fp8) return launch_part<step_prefill_kernel<T, DD, DY, true, true>, LDS>(grid, block, s, p, lo);
      if (win) return launch_part<step_prefill_kernel<T, DD, DY, true, false>, LDS>(grid, block, s, p, lo);
      return launch_part<step_prefill_kernel<T, DD, DY, false, false>, LDS>(grid, block, s, p, lo);
    };
    return p.dyn ? go(std::true_type{}) : go(std::false_type{});
  });
}

// launch_prefill's step form on the entry points that take the slopes: the same grid, block and LDS; always the windowed form, with the
// sides of the block (open ones where the call has no window)
hipError_t launch_prefill_alibi(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeAlibi& alibi, const DecodeLseOut* lse, hipStream_t s) {
  if (!f.step || !f.ragged || !p.dyn || alibi.slopes == nullptr) return hipErrorInvalidValue;
  return dispatch_chunk(dtype, D, [&](auto td) -> hipError_t {
    using T = typename decltype(td)::T;
    constexpr int DD = decltype(td)::D;
    constexpr int LDS = PrefillLds<DD>::BYTES;
    if (p.l2norm && !decode_groups_fast(DD, p.groups, 8)) return hipErrorInvalidValue;
    if ((int64_t)p.slots * p.Hk <= 0) return hipSuccess;
    const dim3 grid((unsigned)((int64_t)p.slots * p.Hk)), block(64 * kPrefillWaves);
    const DecodeLseOut lo = lse != nullptr ? *lse : DecodeLseOut{};
    if (f.fp8) return launch_part<alibi_prefill_kernel<T, DD, true>, LDS>(grid, block, s, p, lo, alibi);
    return launch_part<alibi_prefill_kernel<T, DD, false>, LDS>(grid, block, s, p, lo, alibi);
  });
}

}  // namespace fcsa
