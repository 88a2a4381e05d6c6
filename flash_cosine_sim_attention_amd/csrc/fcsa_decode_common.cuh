// fcsa_decode_common.cuh -- the device helpers that the kernels reading a key/value cache share: the lane's fragment of a row (Unit),
// its unpack / pack, the grouped l2norm across the four lanes of a row (group_normalise) and the address of a cache position
// (cache_base).  Included by fcsa_decode.hip (the single-wave decode kernels) and fcsa_prefill.hip (the multi-wave prefill kernel), which
// must normalise and round a key to the same bits.  Each translation unit gets its own internal copies (anonymous namespace).
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

// Address of cache position `first` (a multiple of 16, uniform) of sequence b, K/V head kvh: a block-table lookup per 16 positions
// (pages are multiples of 16 positions, so the 16 keys of a fragment never straddle two pages).  Block ids are clamped to the pool.
FCSA_DEV const char* cache_base(const DecodeParams& p, const View& v, int b, int kvh, int first) {
  if (p.table != nullptr) {
    int blk = p.table[(int64_t)b * p.table_stride + first / p.page];
    blk = min(max(blk, 0), p.num_blocks - 1);
    return v.p + (int64_t)blk * v.sb + (int64_t)kvh * v.sh + (int64_t)(first % p.page) * v.sn;
  }
  return v.p + (int64_t)b * v.sb + (int64_t)kvh * v.sh + (int64_t)first * v.sn;
}

}  // namespace
}  // namespace fcsa
