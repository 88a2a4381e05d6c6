// fcsa_merge.hip -- merging attention states (fcsa_merge_states, include/fcsa.h).
//
//   merge_states_kernel   S <= 8 states (o_s, lse_s) of the same rows, each over its own keys -> (o, lse) over the union.  One thread per
//                         four features of a row, like the decode combine: it reads the row's S log-sum-exps, takes the weights from
//                         merge_row_weights (csrc/fcsa_dispatch.h: the row maximum, w_s = exp(lse_s - M), the empty-state rule), sums
//                         w_s * o_s over the states of non-zero weight in float32, divides by W once and rounds once.  The state
//                         pointers and strides sit in the parameter block; loads and stores are 8 bytes (16-bit) or 16 bytes (float32).
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

}  // namespace

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
