// fcsa_mx_common.cuh -- the device code shared by fcsa_decode_mx.hip (the single-wave MXFP4 decode kernel) and fcsa_prefill_mx.hip (the
// multi-wave MXFP4 chunk kernel), whose results must agree bit for bit: reading a scale byte, converting a word of eight e2m1 codes, loading
// a lane's words and the grouped l2norm of a row in the "quarter row per lane" layout are written once and both call them.
// Each translation unit gets its own internal copies (anonymous namespace).
#pragma once
#include "fcsa_common.cuh"
#include "fcsa_decode_common.cuh"

#include <type_traits>

namespace fcsa {
namespace {

// 2^(s - 127) for the scale byte s, read clamped to [113, 139]
FCSA_DEV float mx_scale(uint32_t s) { return as_f32(min(max(s, 113u), 139u) << 23); }

// the two codes of byte B of `w` times `s` -> a packed pair of T
template <typename T, int B> FCSA_DEV uint32_t mx_pair(uint32_t w, float s) {
  if constexpr (std::is_same_v<T, F16>) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, B));
  else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, B));
}
// the eight codes of one word (eight consecutive features) times `s`: as eight elements of T (exact), or as float32
template <typename T> FCSA_DEV u32x4 mx_word(uint32_t w, float s) {
  return u32x4{mx_pair<T, 0>(w, s), mx_pair<T, 1>(w, s), mx_pair<T, 2>(w, s), mx_pair<T, 3>(w, s)};
}
FCSA_DEV void mx_word_f32(uint32_t w, float s, float (&x)[8]) {
  const f32x2 a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, 0), b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, 1);
  const f32x2 c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, 2), d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, 3);
  x[0] = a[0]; x[1] = a[1]; x[2] = b[0]; x[3] = b[1]; x[4] = c[0]; x[5] = c[1]; x[6] = d[0]; x[7] = d[1];
}

// NT words from a 4 NT-byte aligned address: one load of that width (three words: a pair and one)
template <int NT> FCSA_DEV void load_words(const char* src, uint32_t (&w)[NT]) {
  if constexpr (NT == 4) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(src);
    w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
  } else if constexpr (NT == 2) {
    const u32x2 v = *reinterpret_cast<const u32x2*>(src);
    w[0] = v[0]; w[1] = v[1];
  } else {
#pragma unroll
    for (int t = 0; t < NT; ++t) w[t] = *reinterpret_cast<const uint32_t*>(src + 4 * t);
  }
}

// Grouped l2norm of a row in the quarter layout -- lane g = lane >> 4 of the row's four lanes holds the features [g Q, (g + 1) Q), Q = 8 NT,
// as NT units of eight: x *= 1 / max(||group||, 1e-12), the l2norm kernel's formula.  gs = features per group: D, or a multiple of 8
// (mx_groups_ok).  One group: the sum crosses the four lanes; whole quarters per group: it crosses one or no lane pair; whole groups per
// quarter: it stays in the lane; anything else (D = 96 with 16 or 32 features per group, which straddle the quarters of 24): every lane
// collects the row's 4 NT unit sums and adds those of its units' groups.  gs is uniform: every lane runs every shuffle.
template <int NT> FCSA_DEV void mx_group_normalise(float (&x)[NT][8], int gs, int lane) {
  constexpr int Q = 8 * NT;
  const int g = lane >> 4;
  float u[NT], ss[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    u[t] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) u[t] += x[t][e] * x[t][e];
  }
  if (gs % Q == 0) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) s += u[t];
    if (gs >= 2 * Q) s += __shfl_xor(s, 16, 64);
    if (gs >= 4 * Q) s += __shfl_xor(s, 32, 64);
#pragma unroll
    for (int t = 0; t < NT; ++t) ss[t] = s;
  } else if (Q % gs == 0) {
    const int m = gs / 8;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      ss[t] = 0.f;
#pragma unroll
      for (int t2 = 0; t2 < NT; ++t2) ss[t] += t2 / m == t / m ? u[t2] : 0.f;
    }
  } else {
    const int m = gs / 8;
#pragma unroll
    for (int t = 0; t < NT; ++t) ss[t] = 0.f;
#pragma unroll
    for (int h = 0; h < 4; ++h)
#pragma unroll
      for (int t2 = 0; t2 < NT; ++t2) {
        const float v = __shfl(u[t2], (lane & 15) + 16 * h, 64);
#pragma unroll
        for (int t = 0; t < NT; ++t) ss[t] += (h * NT + t2) / m == (g * NT + t) / m ? v : 0.f;
      }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float r = 1.f / fmaxf(sqrtf(ss[t]), 1e-12f);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[t][e] *= r;
  }
}

// the rotary embedding's shapes for the three launchers of an MXFP4 engine step: no tables, or rotary_dim D, or 64 at D = 128
inline bool mx_rotary_ok(int D, const DecodeRotary* r) {
  return r == nullptr || (r->cos != nullptr && r->sin != nullptr && r->rows >= 1 && (r->rotary_dim == D || (r->rotary_dim == 64 && D == 128)));
}

// The rotary embedding of a RAW query row in the quarter layout (the ROTARY forms of both kernels): raw[t] = the
// eight 16-bit features g Q + 8 t ... + 7 of lane g = lane >> 4 as loaded, x[t] = their float32 values, rotated in place by the table row of
// `pos` (rotary_at: clamped).  Interleaved pairs (2 f, 2 f + 1) lie inside a unit.  A split pair (f, f + rotary_dim / 2) does NOT stay on the
// lane as it does in the 16-bit kernels' layout: the partner of feature g Q + 8 t + e is the same element of the same unit of the lane
// (rotary_dim / 2) / Q quarters away -- two (lane ^ 32) where rotary_dim is dim_head at 128 and at 64, one (lane ^ 16) for rotary_dim 64 at
// dim_head 128, whose quarters 2 and 3 pass through.  So a unit's partners arrive with ONE exchange of its four raw words (ds_bpermute: no
// LDS traffic, no second global read), before the unpack.  Every lane runs every exchange: the mask is uniform, and rows the tile does not
// have hold zeros.  As in rotary_unit, partner, angle and sign are SELECTED by the uniform layout flags, element e becoming
// fma(x, cos, +-fl(partner * sin)), so the row stays in registers.
template <typename T, int NT> FCSA_DEV void mx_rotary_row(const u32x4 (&raw)[NT], float (&x)[NT][8], const DecodeRotary& ro, int pos, int lane) {
  constexpr int Q = 8 * NT;
  const bool il = ro.interleaved != 0;
  const int half = ro.rotary_dim / 2, g = lane >> 4;
  const int away = (half / Q) * 16;                 // lanes between split partners
  const float* c = ro.cos + rotary_at(ro, pos);
  const float* s = ro.sin + rotary_at(ro, pos);
  float r[NT][8];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int f0 = g * Q + 8 * t;                   // the unit's first feature
    const bool active = f0 < ro.rotary_dim, second = f0 >= half;
    u32x4 pw;
#pragma unroll
    for (int w = 0; w < 4; ++w) pw[w] = (uint32_t)__shfl_xor((int)raw[t][w], away, 64);
    float y[8];
    unpack<T>(pw, y);
    const int at = !active ? 0 : il ? f0 / 2 : f0 - (second ? half : 0);      // (a pass-through unit loads angles it does not use, in range)
    const f32x4 c0 = *reinterpret_cast<const f32x4*>(c + at), s0 = *reinterpret_cast<const f32x4*>(s + at);
    const f32x4 c1 = *reinterpret_cast<const f32x4*>(c + at + (il ? 0 : 4)), s1 = *reinterpret_cast<const f32x4*>(s + at + (il ? 0 : 4));
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float ce = il ? c0[e >> 1] : (e < 4 ? c0[e & 3] : c1[e & 3]);
      const float se = il ? s0[e >> 1] : (e < 4 ? s0[e & 3] : s1[e & 3]);
      const float partner = il ? x[t][e ^ 1] : y[e];
      const bool plus = il ? (e & 1) != 0 : second;      // the pair's second feature: x sin + y cos
      const float ps = partner * se;
      const float rot = fmaf(x[t][e], ce, plus ? ps : -ps);
      r[t][e] = active ? rot : x[t][e];
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int e = 0; e < 8; ++e) x[t][e] = r[t][e];
}

}  // namespace
}  // namespace fcsa
