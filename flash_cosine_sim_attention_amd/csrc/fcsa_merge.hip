// fcsa_merge.hip -- merging attention states (fcsa_merge_states, include/fcsa.h).
//
//   merge_states_kernel   S <= 8 states (o_s, lse_s) of the same rows, each over its own keys -> (o, lse) over the union.  One thread per
//                         four features of a row, like the decode combine: it reads the row's S log-sum-exps, takes the weights from
//                         merge_row_weights (csrc/fcsa_dispatch.h: the row maximum, w_s = exp(lse_s - M), the empty-state rule), sums
//                         w_s * o_s over the states of non-zero weight in float32, divides by W once and rounds once.  The state
//                         pointers and strides sit in the parameter block; loads and stores are 8 bytes (16-bit) or 16 bytes (float32).
//   merge_states_backward_kernel   its backward (fcsa_merge_states_backward): 16 lanes per row, see the kernel.
#include "fcsa_common.cuh"

#include <cmath>

namespace fcsa {

namespace {

template <typename T>
__global__ __launch_bounds__(256) void merge_states_kernel(MergeParams p) {
  constexpr int ES = Traits<T>::ES;
  const int tpr = p.D / 4;                         // threads per row: four features each
  const int64_t rows = (int64_t)p.n0 * p.n1 * p.n2;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / tpr;
  const int c = (int)(t % tpr);
  if (row >= rows) return;
  const int64_t i2 = row % p.n2, i01 = row / p.n2;
  const int64_t i1 = i01 % p.n1, i0 = i01 / p.n1;
  float lse[kMergeMaxStates], w[kMergeMaxStates];
#pragma unroll
  for (int s = 0; s < kMergeMaxStates; ++s)
    lse[s] = s < p.S ? p.lse_in[s].lse[i0 * p.lse_in[s].sb + i1 * p.lse_in[s].sh + i2 * p.lse_in[s].sn] : -INFINITY;
  float lse_row;
  const float W = merge_row_weights(lse, p.S, w, lse_row);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  bool first = true;                               // (the first product is assigned, not added to +0: a lone state's -0 stays -0)
#pragma unroll
  for (int s = 0; s < kMergeMaxStates; ++s) {
    if (s < p.S && w[s] != 0.f) {                  // a state of weight 0 is skipped: whatever its o_s holds cannot leak
      const char* src = p.o_in[s].p + i0 * p.o_in[s].sb + i1 * p.o_in[s].sh + i2 * p.o_in[s].sn + 4 * c * ES;
      f32x4 x;
      if constexpr (ES == 4) {
        x = *reinterpret_cast<const f32x4*>(src);
      } else {
        const u32x2 u = *reinterpret_cast<const u32x2*>(src);
        x = f32x4{Traits<T>::lo(u[0]), Traits<T>::hi(u[0]), Traits<T>::lo(u[1]), Traits<T>::hi(u[1])};
      }
      if (first) acc = w[s] * x;
      else acc += w[s] * x;
      first = false;
    }
  }
  if (W > 0.f) acc /= W;                           // (every state empty: acc is 0 and stays 0)
  char* dst = p.o.p + i0 * p.o.sb + i1 * p.o.sh + i2 * p.o.sn + 4 * c * ES;
  if constexpr (ES == 4) {
    *reinterpret_cast<f32x4*>(dst) = acc;
  } else {
    *reinterpret_cast<u32x2*>(dst) = u32x2{Traits<T>::pack2(acc[0], acc[1]), Traits<T>::pack2(acc[2], acc[3])};
  }
  if (c == 0) p.lse.lse[i0 * p.lse.sb + i1 * p.lse.sh + i2 * p.lse.sn] = lse_row;
}

// One 16-byte chunk of a row as four (float32) or eight (16-bit) floats
template <typename T>
struct Chunk {
  static constexpr int ES = Traits<T>::ES, N = 16 / ES;
  float f[N];
  FCSA_DEV void load(const char* src) {
    const u32x4 u = *reinterpret_cast<const u32x4*>(src);
    if constexpr (ES == 4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = __uint_as_float(u[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        f[2 * e] = Traits<T>::lo(u[e]);
        f[2 * e + 1] = Traits<T>::hi(u[e]);
      }
    }
  }
  FCSA_DEV void store(char* dst) const {
    u32x4 u;
    if constexpr (ES == 4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) u[e] = __float_as_uint(f[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) u[e] = Traits<T>::pack2(f[2 * e], f[2 * e + 1]);
    }
    *reinterpret_cast<u32x4*>(dst) = u;
  }
};

// merge_states_backward_kernel: with a_s = w_s / W the merge is o = sum_s a_s o_s, lse = M + log W, so
//   d o_s = a_s * d_o   (rounded once)      d lse_s = a_s * (d_lse + <d_o, o_s> - sum_t a_t <d_o, o_t>)
// kMergeBwdLanes = 16 lanes own a row and loop over its 16-byte chunks; 256 threads = 16 rows per block, so a row's lanes always lie in
// one wave (the forward's D / 4 threads per row would let a D = 96 row straddle two).  <d_o, o_s> is summed per lane in float32 and
// reduced over the 16 lanes with xor shuffles: no LDS, no atomics, one fixed order.  The weights are merge_row_weights', as in the
// forward.  A state of weight 0 gets d o_s = 0 and d lse_s = 0 exactly and its o_s is never read; every state empty: everything 0.
constexpr int kMergeBwdLanes = 16;
template <typename T>
__global__ __launch_bounds__(256) void merge_states_backward_kernel(MergeBwdParams p) {
  constexpr int ES = Traits<T>::ES;
  const int chunks = p.D * ES / 16;
  const int64_t rows = (int64_t)p.n0 * p.n1 * p.n2;
  const int64_t row = (int64_t)blockIdx.x * (256 / kMergeBwdLanes) + threadIdx.x / kMergeBwdLanes;
  const int c = threadIdx.x % kMergeBwdLanes;
  if (row >= rows) return;                         // (the 16 lanes of a row leave together: the shuffles below stay inside a row)
  const int64_t i2 = row % p.n2, i01 = row / p.n2;
  const int64_t i1 = i01 % p.n1, i0 = i01 / p.n1;
  float lse[kMergeMaxStates], w[kMergeMaxStates], dot[kMergeMaxStates];
#pragma unroll
  for (int s = 0; s < kMergeMaxStates; ++s) {
    lse[s] = s < p.S ? p.lse_in[s].lse[i0 * p.lse_in[s].sb + i1 * p.lse_in[s].sh + i2 * p.lse_in[s].sn] : -INFINITY;
    dot[s] = 0.f;
    w[s] = 0.f;                                    // (merge_row_weights fills the first S)
  }
  float lse_row;
  const float W = merge_row_weights(lse, p.S, w, lse_row);
  const char* go = p.d_o.p + i0 * p.d_o.sb + i1 * p.d_o.sh + i2 * p.d_o.sn;
  for (int ch = c; ch < chunks; ch += kMergeBwdLanes) {
    Chunk<T> g;
    g.load(go + ch * 16);
#pragma unroll
    for (int s = 0; s < kMergeMaxStates; ++s) {
      if (s < p.S && w[s] != 0.f) {                // a state of weight 0 is never read
        Chunk<T> x;
        x.load(p.o_in[s].p + i0 * p.o_in[s].sb + i1 * p.o_in[s].sh + i2 * p.o_in[s].sn + ch * 16);
#pragma unroll
        for (int e = 0; e < Chunk<T>::N; ++e) dot[s] += g.f[e] * x.f[e];
      }
    }
  }
  float mean = 0.f;                                // sum_t a_t <d_o, o_t>
#pragma unroll
  for (int s = 0; s < kMergeMaxStates; ++s) {
#pragma unroll
    for (int m = kMergeBwdLanes / 2; m >= 1; m >>= 1) dot[s] += __shfl_xor(dot[s], m, kMergeBwdLanes);
    w[s] = W > 0.f ? w[s] / W : 0.f;               // a_s from here on
    if (w[s] != 0.f) mean += w[s] * dot[s];
  }
  const float gl = p.d_lse.lse != nullptr ? p.d_lse.lse[i0 * p.d_lse.sb + i1 * p.d_lse.sh + i2 * p.d_lse.sn] : 0.f;
  for (int ch = c; ch < chunks; ch += kMergeBwdLanes) {
    Chunk<T> g;
    g.load(go + ch * 16);
#pragma unroll
    for (int s = 0; s < kMergeMaxStates; ++s) {
      if (s < p.S) {
        Chunk<T> y;
#pragma unroll
        for (int e = 0; e < Chunk<T>::N; ++e) y.f[e] = w[s] != 0.f ? w[s] * g.f[e] : 0.f;
        y.store(p.d_o_in[s].p + i0 * p.d_o_in[s].sb + i1 * p.d_o_in[s].sh + i2 * p.d_o_in[s].sn + ch * 16);
      }
    }
  }
  if (c == 0) {
#pragma unroll
    for (int s = 0; s < kMergeMaxStates; ++s)
      if (s < p.S)
        p.d_lse_in[s].lse[i0 * p.d_lse_in[s].sb + i1 * p.d_lse_in[s].sh + i2 * p.d_lse_in[s].sn] = w[s] != 0.f ? w[s] * (gl + dot[s] - mean) : 0.f;
  }
}

}  // namespace

hipError_t launch_merge_states_backward(int dtype, const MergeBwdParams& p, hipStream_t s) {
  const int64_t rows = (int64_t)p.n0 * p.n1 * p.n2;
  if (rows <= 0) return hipSuccess;
  const int per = 256 / kMergeBwdLanes;
  const dim3 grid((unsigned)((rows + per - 1) / per));
  if (dtype == 2) hipLaunchKernelGGL((merge_states_backward_kernel<BF16>), grid, dim3(256), 0, s, p);
  else if (dtype == 1) hipLaunchKernelGGL((merge_states_backward_kernel<F16>), grid, dim3(256), 0, s, p);
  else if (dtype == 0) hipLaunchKernelGGL((merge_states_backward_kernel<F32>), grid, dim3(256), 0, s, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_merge_states(int dtype, const MergeParams& p, hipStream_t s) {
  const int64_t threads = (int64_t)p.n0 * p.n1 * p.n2 * (p.D / 4);
  if (threads <= 0) return hipSuccess;
  const dim3 grid((unsigned)((threads + 255) / 256));
  if (dtype == 2) hipLaunchKernelGGL((merge_states_kernel<BF16>), grid, dim3(256), 0, s, p);
  else if (dtype == 1) hipLaunchKernelGGL((merge_states_kernel<F16>), grid, dim3(256), 0, s, p);
  else if (dtype == 0) hipLaunchKernelGGL((merge_states_kernel<F32>), grid, dim3(256), 0, s, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace fcsa
