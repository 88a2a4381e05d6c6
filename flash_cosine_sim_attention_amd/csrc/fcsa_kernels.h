// fcsa_kernels.h -- host-side launch interface between the C ABI (fcsa_capi.hip) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>

#include "fcsa_dispatch.h"

namespace fcsa {

// [B, H, L, D] view with BYTE strides; feature dim contiguous.
struct View {
  char*   p;
  int64_t sb, sh, sn;
};

// Packed variable-length sequences (fcsa_forward_varlen / fcsa_backward_varlen), or all null for a dense launch.  A varlen launch has
// B = sequences, N / M = the longest query / key span, views whose sb is ignored and per-row buffers laid out [1, H, total, ...]; each
// workgroup binds itself to its sequence's span first (varlen_bind, fcsa_common.cuh) and then runs the dense code on it.
struct SeqTable {
  const int32_t* cu_q;      // [B + 1] device, or nullptr: dense launch
  const int32_t* cu_k;      // [B + 1] device
  int total_q, total_k;     // packed rows of q (o, dq, ...) and of k (v, dk, ...)
};

struct FwdParams {
  View q, k, v, o;          // q,k: already normalised (or raw when !l2norm)
  float* inv_l;             // [B,H,N] or nullptr; dyn: log2(1 / sum_j exp(S_ij)), else 1 / max(rowsum, l_eps)
  const uint8_t* mask;      // [B,M] or nullptr
  const char* bias;         // [Hb,N,M] contiguous, element type = dtype, or nullptr
  int B, H, N, M;
  int kv_group;             // query heads per K/V head: query head h reads K/V head h / kv_group (1: Hk == H, or a stride-0 head view)
  int causal, bias_batch;
  float c1;                 // scale * log2(e)
  float c2;                 // shift * log2(e)      (P~ = exp2(c1 * qk - c2))
  float bias_c;             // log2(e)              (bias enters as bias * log2e)
  float l_eps;              // clamp of the row sum: 1e-10 (cu:83) rescaled by exp(scale - shift)
  int q_scaled;             // 1: q already carries the factor c1 (fused l2norm writes c1 * q^); 0: the kernel applies it
  int dyn;                  // 1: per-row exponent reference, kept online by the kernel (online_recentre); c2 is 0 then
  int q_raw;                // 1 (16-bit types, fusable groups): q is the RAW query; the kernel prologue does its grouped l2norm,
                            //    folds c1 in, and publishes the saved state of the backward:
  char* qn_out;             //    [B,H,N,D] contiguous c1 * q^ (dtype), or nullptr when no backward follows
  float* rq_out;            //    [B,H,N,G] 1 / max(||q_group||, eps), or nullptr when no backward follows
  int G, lgm;               //    groups; log2(group size / 8)
  float norm_eps;
  int splits;               // > 1: the key range is split over gridDim.y workgroups that write un-normalised partials
  float* ws_o;              // [splits][B*H][N][D] f32 partial P~V
  float* ws_l;              // [splits][B*H][N]    f32 partial row sums
  SeqTable seq;             // packed sequences (seq.cu_q != nullptr): no split, no bias, no key mask
};
// What the launchers take: FwdParams plus the sliding window.  The windowed kernels (fwd_win_kernel) get the whole block; every other
// kernel is launched with the FwdParams part alone, so its kernel arguments -- and its code -- are what they were without the feature.
struct FwdWinParams : FwdParams {
  int window = 0;           // 1: sliding window (causal is 1 then, no split, no bias, no key mask); sides as win_normalise gives them:
  int win_lo = 0, win_hi = 0;   //    query i sees key j iff i + M - N - win_lo <= j <= i + M - N + win_hi
};

struct BwdParams {
  View q, k, v, o, d_out;   // q,k normalised
  View dq;                  // [B,H,N,D]  dtype, or f32 slab when dq_f32
  View dk, dv;              // [B,H,M,D]  (per q-head!) dtype or f32 slabs; kv_sweep: the final [B,Hk,M,D] outputs
  int dq_f32, dk_f32, dv_f32;   // element type of the gradient outputs above: 1 = float32
  const float* inv_l;       // [B,H,N]: 1 / rowsum, or log2 of it (invl_log2: the forward ran its per-row-shift form)
  int invl_log2;
  float* delta;             // [B,H,N] scratch: written by the dq kernel, read by the dkv kernel
  const uint8_t* mask;
  const char* bias;
  void* d_bias;             // [Hb,N,M] in the bias dtype, written once per element by bwd_dbias_kernel, or nullptr
  int dq_splits;            // > 1: the dQ kernel splits the KEY range over gridDim.y workgroups that write partial f32 slabs
  int64_t dq_split_stride;  //      byte distance between the slabs of consecutive splits (dq then views slab 0)
  int dkv_splits;           // > 1: the dK/dV kernel splits the QUERY range over gridDim.y workgroups, partial f32 slabs
  int64_t dkv_split_stride; //      byte distance between the dk (and dv) slabs of consecutive splits
  int B, H, N, M;
  int kv_group;             // query heads per K/V head (see FwdParams)
  int kv_sweep;             // 1: the dK/dV kernel runs its group-sweep form -- one workgroup per (batch, K/V head, key tile) walks the kv_group
                            //    query heads of its group and writes the summed dK / dV once (16-bit, no bias, no split; kv_group > 1)
  int causal, bias_batch;
  float c1, c2, bias_c;
  float scale;
  int q_scaled;             // see FwdParams
  // fused l2norm backward in the epilogues (group size multiple of 8 with a power-of-two number of 8-blocks):
  const float* rq;          // [B,H,N,G] inverse norms of q, or nullptr: dq kernel writes plain dQ^ (dtype or f32 slab)
  const float* rk;          // [B,Hk,M,G] inverse norms of k, or nullptr (set for Hk == H and for the group sweep only)
  int G, lgm;               // groups; log2(group size / 8)
  float norm_eps;           // 1e-12
  SeqTable seq;             // packed sequences (seq.cu_q != nullptr): no split, no bias, no key mask, no group sweep
  const float* dlse = nullptr;   // [B,H,N] like inv_l: the gradient of the rows' log-sum-exp (fcsa_backward_state), or nullptr: none.  The dQ
                            //    kernel publishes delta - dlse (d lse_i / d s_ij = P_ij, so dS = P (dP - (delta - dlse))); every reader of
                            //    delta gets it from there.  (Last field: the ones above keep their places.)
};
struct BwdWinParams : BwdParams {      // (see FwdWinParams; bwd_dq_win_kernel / bwd_dkv_win_kernel)
  int window = 0;
  int win_lo = 0, win_hi = 0;
};

// The slopes of a linear position bias in the training kernels (fcsa_forward_alibi / fcsa_backward_alibi): a second kernel argument of the
// entry points that apply it (fwd_alibi_kernel, bwd_dq_alibi_kernel, bwd_dkv_alibi_kernel), as DecodeAlibi is of the cached ones -- the
// blocks above, and the kernels launched with them alone, are what they were.  The logit of key j for query i gains
// -slopes[b * sb + h * sh] * |i + M - N - j| (natural units; b: batch entry or packed sequence, h: QUERY head).  ELEMENT strides; sb = 0: [H].
struct TrainAlibi {
  const float* slopes;              // device
  int64_t sb, sh;
};

struct NormParams {         // grouped l2norm forward:  x -> xn, inv_norm
  View x;                   // [B,H,L,D]
  char* xn;                 // contiguous [B,H,L,D]
  float* inv_norm;          // contiguous [B,H,L,G] or nullptr
  int B, H, L, D, G;
  float eps;
  float out_scale;          // xn = out_scale * x / max(||x||, eps)   (c1 for q in the fused path, else 1)
};

struct NormBwdParams {      // dx = reduce_heads(slab) then (optionally) l2norm backward
  const char* slab;         // [B,HS,L,D] contiguous; element type f32 (slab_f32) or dtype
  int slab_f32;
  int HS;                   // heads in the slab: output head ho sums the contiguous slab heads [ho * HS / HO, (ho + 1) * HS / HO)
  const char* xn;           // contiguous [B,HO,L,D] normalised input (dtype) or nullptr (no norm)
  const float* inv_norm;    // [B,HO,L,G]
  View dx;                  // [B,HO,L,D] out (dtype)
  int B, HO, L, D, G;
  float eps;
  float xn_scale;           // x^ = xn_scale * xn   (1/c1 when xn was written with out_scale = c1)
};

// Decoding against a key/value cache (fcsa_forward_kvcache and its _window, _quant, _varlen, _lse, _prefill and _step forms;
// csrc/fcsa_decode.hip, csrc/fcsa_prefill.hip).  The C ABI fills ONE block per call -- DecodeStepParams, the most derived of the chain
// below -- and the launchers hand every kernel entry point the part of it that entry point takes (a base-class slice), so the kernel
// arguments of each entry point -- and its code -- are what they were before the later features existed.  Views carry BYTE strides; kc / vc are the caches (sb = batch stride, or block stride when
// `table` is set), kn / vn the appended rows [B, Hk, new_len, D].
struct DecodeParams {        // decode_kernel, kv_append_kernel, decode_combine[_lse]_kernel
  View q, o;                // [B, H, N, D]
  View kc, vc;              // caches
  View kn, vn;              // new rows (append kernel only)
  const int32_t* seqlens;   // [B] tokens cached before the append, or nullptr: every sequence full
  const int32_t* table;     // [B, capacity / page] block ids, or nullptr: contiguous cache
  int64_t table_stride;     // elements between table rows
  int capacity, page, num_blocks, new_len;
  int B, H, Hk, G, N;       // G = H / Hk query heads per K/V head; rows of a tile: r = g * N + i
  int row_tiles, splits;
  int causal, l2norm, groups;
  float c1;                 // scale * log2(e)
  float c2;                 // static exponent shift * log2(e) (dyn == 0)
  float l_eps;              // row-sum clamp of the static regime
  int dyn;                  // 1: per-row running max (the per-row-shift regime), kept per split and reconciled by the combine
  float* ws_o;              // [splits][B*H*N][D] f32 partial P~V
  float* ws_ml;             // [splits][B*H*N][2] f32 (row max in log2 units, row sum)
};
struct DecodeWinParams : DecodeParams {      // decode_win_kernel (see FwdWinParams)
  int window = 0;           // 1: sliding window, sides as win_normalise gives them (causal: win_hi = 0):
  int win_lo = 0, win_hi = 0;   //    the query at position t sees key j iff t - win_lo <= j <= t + win_hi
};
// An fp8 cache (fcsa_forward_kvcache_quant): kc / vc hold one-byte OCP e4m3fn codes (views in bytes), and the cache means
// k_scale[b, kvh] * code, v_scale[b, kvh] * code.
struct DecodeFp8Params : DecodeWinParams {   // kv_append_fp8_kernel, decode_fp8_kernel, decode_combine[_lse]_fp8_kernel
  const float* k_scale = nullptr;   // element [b * ks_b + kvh * ks_h]; a stride of 0 broadcasts
  const float* v_scale = nullptr;
  int64_t ks_b = 0, ks_h = 0, vs_b = 0, vs_h = 0;
};
// A ragged decode step (fcsa_forward_kvcache_varlen): q / o are packed [total_q, H, D] views and kn / vn packed [total_q, Hk, D] ones (sb
// unused), sequence b owning the packed rows [cu_q[b], cu_q[b + 1]).  N, new_len and row_tiles of the base block are 0 and unused: every
// workgroup takes its sequence's own row count from the table (fcsa::ragged_tile).  The window fields are always live: open sides
// (kWinOpen; causal: win_hi = 0) for a call without a window, so one decode entry point per cache type serves every call.  The four
// fields below are 0 in a rectangular call.
struct DecodeRaggedParams : DecodeFp8Params {   // kv_append_ragged_kernel, decode_ragged[_fp8]_kernel, decode_combine[_lse]_ragged_kernel
  const int32_t* cu_q = nullptr;    // [B + 1] device
  int total_q = 0;                  // packed rows of q, o, kn, vn
  int slots = 0;                    // flat row-tile slots per K/V head: fcsa::ragged_slots(total_q, B, G)
  int append = 0;                   // 1: every query row brings its key and value (L_b counts them)
};
// The rows' log-sum-exp as a second result of a decode call (fcsa_forward_kvcache_lse): a second kernel argument of the combine entry
// points that write it (decode_combine_lse*_kernel), so that the parameter blocks above -- and the kernels launched with them alone --
// are what they were.  ELEMENT strides: [b, h, i] at b * sb + h * sh + i * sn (ragged: [tok, h] at h * sh + tok * sn).
struct DecodeLseOut {
  float*  lse;
  int64_t sb, sh, sn;
};
// The per-row visibility words of a tree step (fcsa_forward_kvcache_tree): a second kernel argument of the decode entry points that read
// them (decode_tree[_fp8]_kernel), as DecodeLseOut is of the combines -- the blocks above, and the kernels launched with them alone, are
// what they were.  words[tok]: bit t set = packed row `tok` sees token t of its own sequence's step (cache position L_b - N_b + t).
struct DecodeTreeMask {
  const uint64_t* words;            // [total_q] device
};
// The per-head slopes of a linear position bias (fcsa_forward_kvcache_alibi): a second kernel argument of the entry points that apply it
// (alibi_decode[_fp8]_kernel, alibi_prefill_kernel), as DecodeTreeMask is of the tree entry points.  The logit of key j for the query at
// position pos = L_b - N_b + i gains -slopes[b * sb + h * sh] * |pos - j| (natural units).  ELEMENT strides; sb = 0: one row for every sequence.
struct DecodeAlibi {
  const float* slopes;              // device
  int64_t sb, sh;
};
// An engine step (fcsa_forward_kvcache_step): the ragged step's block plus the routing threshold.  Sequence b takes the chunk kernel
// (step_prefill_kernel) iff G * N_b >= chunk_rows and the decode kernels (step_decode[_fp8]_kernel, step_combine[_lse]_kernel) otherwise;
// all of them evaluate that on the device from the clamped table (ragged_cu), so every row is written by exactly one of them.
struct DecodeStepParams : DecodeRaggedParams {   // step_decode[_fp8]_kernel, step_combine[_lse]_kernel, step_prefill_kernel
  int chunk_rows = 0;               // 0 outside a step
};
// The launch layer of the whole family: the C ABI fills ONE block per call, DecodeStepParams -- the most derived type -- and four
// launchers, one per job, each dispatch dtype, head dim and form once and hand the entry point they pick the base-class slice it declares.
// fp8: an e4m3fn cache (q, o and the appended rows f16 or bf16; float32 is refused); ragged: a ragged step; step: an engine step, which is
// a ragged step (step without ragged: hipErrorInvalidValue) and exists for the 16-bit types at D = 64 / 128 (anything else:
// hipErrorInvalidValue); the window of a rectangular call is p.window; lse: nullptr, or where the rows' log-sum-exp goes as well.
struct DecodeForm { bool fp8, ragged, step; };
hipError_t launch_kv_append(int dtype, int D, DecodeForm f, const DecodeStepParams& p, hipStream_t s);      // (a step's append is the ragged call's)
hipError_t launch_decode(int dtype, int D, DecodeForm f, const DecodeStepParams& p, hipStream_t s);
hipError_t launch_decode_combine(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeLseOut* lse, hipStream_t s);
// The decode launch of a tree step (fcsa_forward_kvcache_tree): launch_decode's ragged form -- the same grid, LDS and block -- on the entry
// points that take the visibility words (decode_tree[_fp8]_kernel).  f.ragged must be set and f.step clear (hipErrorInvalidValue).  The
// append and the combine of a tree step are launch_kv_append and launch_decode_combine, unchanged.
hipError_t launch_decode_tree(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeTreeMask& tree, hipStream_t s);
// Compaction of the accepted path of a tree step (fcsa_kvcache_compact; kv_compact_kernel in csrc/fcsa_decode.hip): rows of the caches
// are moved as bytes inside the window [cache_seqlens[b], cache_seqlens[b] + kCompactSlots) of every sequence.  The caches, seqlens,
// table, capacity, page, num_blocks, B and Hk of `cache` address them (cache_base); row_bytes = bytes of one cached row (a multiple of 16).
constexpr int kCompactSlots = 64;   // step tokens a tree can have: the bits of a visibility word
struct CompactParams {
  const int32_t* accepted;          // [B, A] device: step-token indices, strictly increasing over the first num_accepted[b]
  const int32_t* num_accepted;      // [B] device
  int64_t accepted_stride;          // elements between the rows of `accepted`
  int A;                            // 1 <= A <= kCompactSlots
  int row_bytes;
};
hipError_t launch_kv_compact(const DecodeParams& cache, const CompactParams& c, hipStream_t s);
// A prompt chunk against the cache (fcsa_forward_kvcache_prefill, and with f.step the chunk side of an engine step; csrc/fcsa_prefill.hip):
// the block with slots = fcsa::prefill_slots(total_q, B, G, kPrefillRows), one split and no workspace; f16 / bf16, D = 64 / 128 (anything
// else: hipErrorInvalidValue).  One kernel writes o and, where lse is not nullptr, the rows' log-sum-exp.  An fp8 cache and a window come
// with f.step only (fp8 without it: hipErrorInvalidValue).
hipError_t launch_prefill(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeLseOut* lse, hipStream_t s);
// The decode and chunk launches of a call with a linear position bias (fcsa_forward_kvcache_alibi): launch_decode's ragged or step form and
// launch_prefill's step form -- the same grids, LDS and blocks -- on the entry points that take the slopes.  They exist in the per-row-shift
// regime only (p.dyn must be set) and always carry the window sides, open where the call has none; f.ragged must be set, and f.step exactly
// where the step kernels exist (16-bit types, D = 64 / 128: one decode form per problem is compiled); hipErrorInvalidValue otherwise.  Append and combine are launch_kv_append / launch_decode_combine.
hipError_t launch_decode_alibi(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeAlibi& alibi, hipStream_t s);
hipError_t launch_prefill_alibi(int dtype, int D, DecodeForm f, const DecodeStepParams& p, const DecodeAlibi& alibi, const DecodeLseOut* lse, hipStream_t s);

// Merging attention states (fcsa_merge_states, csrc/fcsa_merge.hip): S states (o_s, lse_s) of the rows [n0, n1, n2] -> (o, lse).  o views
// carry BYTE strides, lse views ELEMENT strides.
struct MergeParams {
  View         o_in[8];
  DecodeLseOut lse_in[8];
  View         o;
  DecodeLseOut lse;
  int n0, n1, n2, D, S;
};
hipError_t launch_merge_states(int dtype, const MergeParams& p, hipStream_t s);
// Its backward (fcsa_merge_states_backward): the gradients (d_o, d_lse) of the merged state -> (d_o_in[s], d_lse_in[s]) of every state.
// d_lse.lse == nullptr: no gradient for the merged lse (0).
struct MergeBwdParams {
  View         o_in[8];
  DecodeLseOut lse_in[8];
  View         d_o;
  DecodeLseOut d_lse;
  View         d_o_in[8];
  DecodeLseOut d_lse_in[8];
  int n0, n1, n2, D, S;
};
hipError_t launch_merge_states_backward(int dtype, const MergeBwdParams& p, hipStream_t s);

// The rows' log-sum-exp of a training forward from its saved inv_l (fcsa_attention_lse, csrc/fcsa_state.hip).  B / N / M as in FwdParams
// (packed: sequences and the longest spans); inv_l [B, H, N] (packed: [1, H, total_q]); out in ELEMENT strides ([b, h, i], packed
// [tok, h]); win_lo / win_hi: the sides win_normalise gives -- (kWinOpen, kWinOpen) no mask, (kWinOpen, 0) causal.
struct StateLseParams {
  const float* inv_l;
  DecodeLseOut out;
  int B, H, N, M;
  int win_lo, win_hi;
  float c2;                 // shift * log2(e) (0 with invl_log2)
  int invl_log2;            // inv_l holds log2 of the normaliser (the per-row-shift regime)
  SeqTable seq;
};
hipError_t launch_state_lse(const StateLseParams& p, hipStream_t s);

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE property of a kernel: raise it once per (instantiation, device).
// `done` is the instantiation's bit mask of devices that have it (one static per launcher); thread safe, idempotent.
template <typename K>
static inline hipError_t ensure_dynamic_lds(K kern, size_t lds, std::atomic<uint64_t>& done) {
  int dev = 0;
  if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
  const uint64_t bit = (dev >= 0 && dev < 64) ? (1ull << dev) : 0ull;        // devices >= 64: set it on every launch
  if (bit != 0 && (done.load(std::memory_order_acquire) & bit) != 0) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess && bit != 0) done.fetch_or(bit, std::memory_order_release);
  return e;
}

// Launch one kernel instantiation with `lds` bytes of dynamic LDS, raising its limit first (once per device: the static belongs to the
// instantiation).  The kernels take their parameter block(s) by value.
template <auto Kernel, typename... Args>
static inline hipError_t launch_with_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args&... args) {
  static std::atomic<uint64_t> done{0};
  if (hipError_t e = ensure_dynamic_lds(Kernel, lds, done); e != hipSuccess) return e;
  hipLaunchKernelGGL(Kernel, grid, block, lds, s, args...);
  return hipGetLastError();
}

// Compute units of the CURRENT device: what every "does this grid cover the chip" threshold of the launchers and of the C ABI's split
// rules is a multiple of.  Cached per device id (a process may drive unlike devices, e.g. partitioned CPX modes); a query that fails is
// answered with 256 and NOT remembered (host-only callers: workspace-size queries in the CPU tests; a process that asks before its
// device is usable gets the real number the next time).  The workspace size a caller is told and the launch that uses it agree as long
// as both run with the same current device.
inline int cu_count() {
  static std::atomic<int> cached[64];
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();      // a host without a device: do not leave a sticky error behind
    return 256;
  }
  const bool slot = dev >= 0 && dev < 64;
  if (slot) {
    const int n = cached[dev].load(std::memory_order_relaxed);
    if (n > 0) return n;
  }
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
    (void)hipGetLastError();
    return 256;
  }
  if (slot) cached[dev].store(cus, std::memory_order_relaxed);
  return cus;
}

// dtype: 1 = f16, 2 = bf16 (fcsa_dtype); returns hipError_t of the launch
hipError_t launch_forward(int dtype, int D, const FwdWinParams& p, hipStream_t s);
// The same launches with a linear position bias (fcsa_forward_alibi / fcsa_backward_alibi): windowed launches only (p.window set, open
// sides where the call has no window; no bias, key mask, split or group sweep) on the entry points that take the slopes.
hipError_t launch_forward_alibi(int dtype, int D, const FwdWinParams& p, const TrainAlibi& al, hipStream_t s);
hipError_t launch_backward_dq_alibi(int dtype, int D, const BwdWinParams& p, const TrainAlibi& al, hipStream_t s);
hipError_t launch_backward_dkv_alibi(int dtype, int D, const BwdWinParams& p, const TrainAlibi& al, hipStream_t s);
// fcsa_fwd3.hip: the 64-rows-per-wave, one-wave-per-SIMD forward for 16-bit D = 128 (launch_forward dispatches to it)
int forward_wide128_mode(int set);      // debug knob behind fcsa_debug_forward_form: set < 0 queries; returns the previous value
hipError_t launch_forward_wide128(int dtype, const FwdParams& p, hipStream_t s);
hipError_t launch_backward_dq(int dtype, int D, const BwdWinParams& p, hipStream_t s);
hipError_t launch_backward_dbias(int dtype, int D, const BwdParams& p, hipStream_t s);   // d_bias from recomputed dS tiles (after dq: needs delta)
hipError_t launch_backward_dkv(int dtype, int D, const BwdWinParams& p, hipStream_t s);
int kv_group_mode(int set);             // debug knob behind fcsa_debug_kv_group_form: set < 0 queries; returns the previous value
hipError_t launch_l2norm(int dtype, const NormParams& p, hipStream_t s);
hipError_t launch_l2norm_pair(int dtype, const NormParams& a, const NormParams& b, hipStream_t s);   // q and k in one grid
hipError_t launch_l2norm_bwd(int dtype, const NormBwdParams& p, hipStream_t s);
hipError_t launch_l2norm_bwd_pair(int dtype, const NormBwdParams& a, const NormBwdParams& b, hipStream_t s);   // two passes, one grid
hipError_t launch_l2norm_bwd_triple(int dtype, const NormBwdParams& a, const NormBwdParams& b, const NormBwdParams& c, hipStream_t s);   // three

}  // namespace fcsa
