// fcsa_decode_common.cuh -- the device code shared by fcsa_decode.hip (the single-wave decode kernels) and fcsa_prefill.hip (the multi-wave
// prefill kernel), whose results must agree bit for bit: what is here is written once and both call it (DESIGN.md 4.7.4 lists what is
// still written in both).  A row in registers: Unit, unpack / pack, unpack_fp8 (an e4m3fn cache), group_normalise.  Reading the cache: cache_base, clamped_first / clamped_off,
// kKvPitch.  A 32-key block step: softmax_step, pv_block.  The end of a row: combine_weight, combine_inv.  Host side: launch_part (every
// entry point gets the slice of the call's block it declares) and dispatch_chunk (the one f16 / bf16 x D 64 / 128 ladder).
// Each translation unit gets its own internal copies (anonymous namespace).
#pragma once
#include "fcsa_common.cuh"

namespace fcsa {
namespace {

// the lane's fragment of a row: NJ units of UE elements, unit j holds features (4 j + hi) * UE ... + UE - 1 (hi = lane >> 4)
template <typename T> struct Unit;
template <> struct Unit<BF16> {
  static constexpr int UE = 8;
  static FCSA_DEV f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};
template <> struct Unit<F16> {
  static constexpr int UE = 8;
  static FCSA_DEV f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};
template <> struct Unit<F32> {
  static constexpr int UE = 4;
};

template <typename T> FCSA_DEV void unpack(const u32x4& u, float (&x)[Unit<T>::UE]) {
  if constexpr (Traits<T>::ES == 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = as_f32(u[e]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) { x[2 * e] = Traits<T>::lo(u[e]); x[2 * e + 1] = Traits<T>::hi(u[e]); }
  }
}
template <typename T> FCSA_DEV u32x4 pack(const float (&x)[Unit<T>::UE], float mul) {
  u32x4 u;
  if constexpr (Traits<T>::ES == 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) u[e] = __builtin_bit_cast(uint32_t, x[e] * mul);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) u[e] = Traits<T>::pack2(x[2 * e] * mul, x[2 * e + 1] * mul);
  }
  return u;
}

// eight e4m3fn codes (byte e of the pair = element e) -> their exact float32 values
FCSA_DEV void unpack_fp8(const u32x2& u, float (&x)[8]) {
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)u[w], false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)u[w], true);
    x[4 * w] = a[0]; x[4 * w + 1] = a[1]; x[4 * w + 2] = b[0]; x[4 * w + 3] = b[1];
  }
}

// Grouped l2norm of one row held by the four lanes x, x + 16, x + 32, x + 48 (x = lane & 15): x *= 1 / max(||group||, 1e-12), the l2norm
// kernel's formula.  gs = features per group (decode_groups_fast: one group, a divisor of UE, or UE times a power of two).  Every lane runs
// every shuffle (gs is uniform).
template <int NJ, int UE> FCSA_DEV void group_normalise(float (&x)[NJ][UE], int gs, int D) {
  float ss[NJ][UE];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int e = 0; e < UE; ++e) ss[j][e] = x[j][e] * x[j][e];
  if (gs == D) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int e = 0; e < UE; ++e) t += ss[j][e];
    t += __shfl_xor(t, 16, 64);
    t += __shfl_xor(t, 32, 64);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int e = 0; e < UE; ++e) ss[j][e] = t;
  } else if (gs <= UE) {
#pragma unroll
    for (int s = 1; s < UE; s *= 2) {
      if (s < gs) {
        float n[NJ][UE];
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int e = 0; e < UE; ++e) n[j][e] = ss[j][e] + ss[j][e ^ s];
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int e = 0; e < UE; ++e) ss[j][e] = n[j][e];
      }
    }
  } else {
    const int units = gs / UE;
    float u[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      u[j] = 0.f;
#pragma unroll
      for (int e = 0; e < UE; ++e) u[j] += ss[j][e];
    }
    if (units >= 2) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) u[j] += __shfl_xor(u[j], 16, 64);
    }
    if (units >= 4) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) u[j] += __shfl_xor(u[j], 32, 64);
    }
#pragma unroll
    for (int s = 1; s < NJ; s *= 2) {
      if (4 * s < units) {
        float n[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) n[j] = (j ^ s) < NJ ? u[j] + u[j ^ s] : u[j];
#pragma unroll
        for (int j = 0; j < NJ; ++j) u[j] = n[j];
      }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int e = 0; e < UE; ++e) ss[j][e] = u[j];
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int e = 0; e < UE; ++e) x[j][e] *= 1.f / fmaxf(sqrtf(ss[j][e]), 1e-12f);
}

// THE address rule of the caches, for the kernels that read them and the append kernels that write them: cache position `pos` (in
// [0, capacity)) of sequence b, K/V head kvh -- through the block table when the cache is paged, the block id clamped to the pool, and
// contiguous otherwise.  The readers call it once per 16 positions, with a uniform multiple of 16 (pages are multiples of 16 positions, so
// the 16 keys of a fragment never straddle two pages).
FCSA_DEV char* cache_base(const DecodeParams& p, const View& v, int b, int kvh, int pos) {
  if (p.table != nullptr) {
    int blk = p.table[(int64_t)b * p.table_stride + pos / p.page];
    blk = min(max(blk, 0), p.num_blocks - 1);
    return v.p + (int64_t)blk * v.sb + (int64_t)kvh * v.sh + (int64_t)(pos % p.page) * v.sn;
  }
  return v.p + (int64_t)b * v.sb + (int64_t)kvh * v.sh + (int64_t)pos * v.sn;
}

// The load rule: a position at or beyond `end` reads position end - 1 (in bounds) and its V is zeroed.  clamped_first: what to hand cache_base
// for the 16 positions from first16 (one lookup per 16 positions).  clamped_off: the distance of position `pos` of those 16 from it.
FCSA_DEV int clamped_first(int first16, int end) { return min(first16, (end - 1) & ~15); }
FCSA_DEV int clamped_off(int pos, int first, int end) { return min(pos, end - 1) - first; }

// Bytes between two rows of a K^ / V block in LDS: D elements padded by 16 bytes.  The transposed V reads (pv_block) address a 32-key
// block at this pitch, in the decode kernel's LDS (DecodeLds) and in the prefill kernel's (PrefillLds) alike.
template <int D, int ES> constexpr int kKvPitch = D * ES + 16;

// The softmax step of one 32-key block for one row: s = the lane's masked logits (log2 units), m / l / acc = the row's running shift, row
// sum (this lane's share) and O^T.  DYN: the row maximum over the row's four lanes joins m, and acc and l are rescaled to it; otherwise the
// shift is the constant c2.  pr = P~ = 2^(s - shift).
template <bool DYN, int FB> FCSA_DEV void softmax_step(const f32x4 (&s)[2], float& m, float& l, f32x4 (&acc)[FB], float c2, f32x4 (&pr)[2]) {
  float shift = c2;
  if constexpr (DYN) {
    float bm = fmaxf(fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3])), fmaxf(fmaxf(s[1][0], s[1][1]), fmaxf(s[1][2], s[1][3])));
    bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
    bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
    const float mn = fmaxf(m, bm);
    shift = mn == -INFINITY ? 0.f : mn;
    const float alpha = fast_exp2(m - shift);      // 0 while the row has seen no key
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) acc[fb] *= alpha;
    l *= alpha;
    m = mn;
  }
#pragma unroll
  for (int sb = 0; sb < 2; ++sb)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      pr[sb][rr] = fast_exp2(s[sb][rr] - shift);
      l += pr[sb][rr];
    }
}

// The linear position bias of the ALIBI forms (fcsa_forward_kvcache_alibi), for both kernels.  alibi_slope: -slope * log2(e) of the row's
// (sequence, head), loaded once per lane row.  alibi_logit: the biased logit in log2 units, s * smul - slope * log2(e) * |d0 - c|, where d0 is
// the float distance from the row's position to a point of the key block (hoisted by the caller) and c the key's offset from that point: one
// subtract and one fma (the |.| is an operand modifier) on top of the multiply every form does.  Distances are integers in float32, exact
// below 2^24, and the product with the slope is rounded once, inside the fma.
FCSA_DEV float alibi_slope(const DecodeAlibi& al, int b, int h) { return -(al.slopes[(int64_t)b * al.sb + (int64_t)h * al.sh] * 1.4426950408889634f); }
FCSA_DEV float alibi_logit(float s, float smul, float nslope, float d0, int c) { return fmaf(nslope, fabsf(d0 - (float)c), s * smul); }

// O^T += V^T P~^T for the 32-key block of 16-bit V at rows row0 ... row0 + 31 of `v` in LDS (pitch kKvPitch<D, 2>): lane 4q + p of the
// 16-lane group hi (x = lane & 15 = 4q + p) addresses key 4 hi + q, features 16 fb + 4p ... + 3; lane x receives feature 16 fb + x.  Every
// transposed read feeds the NT row tiles pb[0 .. NT) -> acc[0 .. NT).
template <typename T, int D, int NT> FCSA_DEV void pv_block(const char* v, int row0, int x, int hi, const u32x4* pb, f32x4 (*acc)[D / 16]) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  constexpr int PITCH = kKvPitch<D, 2>;
  const char* a0 = v + (row0 + 4 * hi + (x >> 2)) * PITCH + 8 * (x & 3);
#pragma unroll
  for (int fb = 0; fb < D / 16; ++fb) {
    const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 32 * fb));
    const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 16 * PITCH + 32 * fb));
    const u32x2 u0 = __builtin_bit_cast(u32x2, v0), u1 = __builtin_bit_cast(u32x2, v1);
    const u32x4 vf = u32x4{u0[0], u0[1], u1[0], u1[1]};
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t][fb] = Unit<T>::mfma(vf, pb[t], acc[t][fb]);
  }
}

// The combine of a row: a split's partials (row shift m_s, row sum l_s, P~V) join l and acc with the weight 2^(m_s - M), M = the largest m_s
// of the row (static regime: every m_s is the common shift, weight 1); the normaliser is 1 / l (0 for a row that saw no key) in the
// per-row-shift regime, 1 / max(l, l_eps) otherwise
FCSA_DEV float combine_weight(float m_s, float M) { return exp2f(m_s - M); }
FCSA_DEV float combine_inv(bool dyn, float l, float l_eps) { return dyn ? (l > 0.f ? 1.f / l : 0.f) : 1.f / fmaxf(l, l_eps); }

// ---- host side: what the launchers of both files share ------------------------------------------------------------------------------
// The parameter block a kernel entry point takes, and the launch of `Kernel` with that part of the call's one block (a base-class slice;
// LDS > 0: dynamic LDS, raised once per device) -- so no launcher can hand an entry point another block than the one it declares.
template <typename P, typename... More> P block_of(void (*)(P, More...));
template <auto Kernel, int LDS, typename... More>
hipError_t launch_part(dim3 grid, dim3 block, hipStream_t s, const DecodeStepParams& p, const More&... more) {
  using P = decltype(block_of(Kernel));
  if constexpr (LDS > 0) {
    return launch_with_lds<Kernel>(grid, block, LDS, s, static_cast<const P&>(p), more...);
  } else {
    hipLaunchKernelGGL(Kernel, grid, block, 0, s, static_cast<const P&>(p), more...);
    return hipGetLastError();
  }
}

// Where the chunk kernel -- and with it every kernel of an engine step -- is compiled: the 16-bit types at D = 64 / 128.  dispatch_chunk:
// fn(TypeDim<T, D>) there, hipErrorInvalidValue for every other problem.
template <typename T, int D> constexpr bool kHasChunkKernel = Traits<T>::ES == 2 && (D == 64 || D == 128);
template <typename F> hipError_t dispatch_chunk(int dtype, int D, F&& fn) {
  return dispatch_dtype_d(dtype, D, [&](auto td) -> hipError_t {
    if constexpr (kHasChunkKernel<typename decltype(td)::T, decltype(td)::D>) return fn(td);
    else return hipErrorInvalidValue;
  });
}

}  // namespace
}  // namespace fcsa
