// fcsa_state.hip -- the rows' log-sum-exp of a training forward (fcsa_attention_lse, include/fcsa.h).
//
//   state_lse_kernel   one thread per query row: reads the row's saved normaliser inv_l and writes lse = ln 2 * (c2 - L), with
//                      L = log2(inv_l) (constant shift: inv_l = 1 / max(l, eps), c2 = shift * log2(e)) or L = inv_l itself (per-row
//                      shift: the forward saved the log2, c2 = 0) -- the value every backward kernel seeds its S accumulator with,
//                      negated.  Where the constant-shift clamp acts (l < eps) this is ln(max(l, eps)) + shift: consistent with the o
//                      the forward returned (o * exp(lse) is the un-normalised sum), unlike the decode LSE, which is unclamped.
//                      A row WITHOUT a visible key gets exactly -inf, decided from the geometry (its inv_l is 1 / eps, or 1: a finite
//                      number): query i of N sees the keys [max(i + M - N - lo, 0), min(i + M - N + hi, M - 1)] -- lo / hi the sides
//                      win_normalise gives (kWinOpen for an open side, hi = 0 under causal) -- and the row is empty when that interval
//                      is.  Packed calls: one block per (sequence, head, 256 rows of the longest sequence); each block takes its
//                      sequence's (N_s, M_s) from the tables, clamped by seq_span, so no table contents lead outside the buffers.
#include "fcsa_common.cuh"

#include <cmath>

namespace fcsa {

namespace {

__global__ __launch_bounds__(256) void state_lse_kernel(StateLseParams p) {
  const int rb = (p.N + 255) / 256;                // row blocks per (sequence, head)
  const int64_t blk = blockIdx.x;
  const int r0 = (int)(blk % rb) * 256;
  const int64_t bh = blk / rb;
  const int h = (int)(bh % p.H), b = (int)(bh / p.H);
  int N = p.N, M = p.M;
  int64_t in_at = ((int64_t)b * p.H + h) * p.N;    // inv_l [B, H, N]
  int64_t out_at = (int64_t)b * p.out.sb + (int64_t)h * p.out.sh;
  if (p.seq.cu_q != nullptr) {                     // packed: inv_l [1, H, total_q]; out [token, head]
    int q0, k0;
    seq_span(p.seq.cu_q[b], p.seq.cu_q[b + 1], p.seq.total_q, p.N, q0, N);
    seq_span(p.seq.cu_k[b], p.seq.cu_k[b + 1], p.seq.total_k, p.M, k0, M);
    in_at = (int64_t)h * p.seq.total_q + q0;
    out_at = (int64_t)h * p.out.sh + (int64_t)q0 * p.out.sn;
  }
  const int i = r0 + (int)threadIdx.x;
  if (i >= N) return;
  const int64_t d = (int64_t)i + M - N;
  const int64_t first = d - p.win_lo > 0 ? d - p.win_lo : 0;
  const int64_t last = d + p.win_hi < (int64_t)M - 1 ? d + p.win_hi : (int64_t)M - 1;
  float lse = -INFINITY;
  if (last >= first) {                             // once per row, so in double (as decode_row_lse)
    const float x = p.inv_l[in_at + i];
    const double L = p.invl_log2 ? (double)x : log2((double)x);
    lse = (float)(0.6931471805599453 * ((double)p.c2 - L));
  }
  p.out.lse[out_at + (int64_t)i * p.out.sn] = lse;
}

}  // namespace

hipError_t launch_state_lse(const StateLseParams& p, hipStream_t s) {
  if (p.B <= 0 || p.H <= 0 || p.N <= 0) return hipSuccess;
  const int64_t blocks = (int64_t)p.B * p.H * ((p.N + 255) / 256);
  if (blocks > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(state_lse_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace fcsa
