// fcsa_capi.hip -- the C ABI of libfcsa_hip.so (include/fcsa.h): validation, workspace carving and
// launch sequencing.  Replaces the reference's host launchers + pybind module (cu:1630-1933) and
// dispatch.h (dh:38-73): unsupported dtypes / head dims are REJECTED with an error instead of the
// reference's silent no-op default branch (dh:50-52), nothing synchronises the device (cf. cu:1745,
// cu:1889) and every launch goes to the caller's stream (cf. the default-stream launches cu:1720).
#include "../../include/fcsa.h"
#include "fcsa_kernels.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

namespace {

thread_local std::string g_err;
constexpr float kLog2e = 1.4426950408889634f;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int elem_size(int dtype) { return dtype == FCSA_F32 ? 4 : 2; }

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

bool dim_ok(int d) { return d == 16 || d == 32 || d == 64 || d == 96 || d == 128; }   // cu:84 allowed_dim_heads

int check_problem(const fcsa_problem& p) {
  if (p.dtype != FCSA_F16 && p.dtype != FCSA_BF16 && p.dtype != FCSA_F32)
    return fail(FCSA_ERR_UNSUPPORTED, "unsupported dtype %d (expected f32=0, f16=1, bf16=2)", p.dtype);
  if (!dim_ok(p.dim_head))
    return fail(FCSA_ERR_UNSUPPORTED, "dim_head %d not in {16, 32, 64, 96, 128}", p.dim_head);
  if (p.batch < 0 || p.heads < 0 || p.q_len < 0 || p.k_len < 0)
    return fail(FCSA_ERR_INVALID_ARG, "negative size (B=%d H=%d N=%d M=%d)", p.batch, p.heads, p.q_len, p.k_len);
  if (p.kv_heads < 1 ? p.heads != 0 || p.kv_heads != 0 : p.heads % p.kv_heads != 0)
    return fail(FCSA_ERR_INVALID_ARG, "kv_heads must divide heads (%d), got %d", p.heads, p.kv_heads);
  if (p.l2norm_qk) {
    if (p.groups < 1 || p.dim_head % p.groups != 0)
      return fail(FCSA_ERR_INVALID_ARG, "groups (%d) must divide dim_head (%d)", p.groups, p.dim_head);
    if (p.dtype == FCSA_F16 && fabsf(p.scale) * kLog2e > 60000.f)
      return fail(FCSA_ERR_UNSUPPORTED, "float16: scale %g puts scale * log2(e) * q^ outside the type", (double)p.scale);
  } else if (p.groups != 1) {
    return fail(FCSA_ERR_INVALID_ARG, "groups must be 1 when l2norm_qk is 0");
  }
  if (!(p.scale == p.scale) || std::isinf(p.scale)) return fail(FCSA_ERR_INVALID_ARG, "scale is NaN or infinite");
  return FCSA_OK;
}

int check_tensor(const char* name, const fcsa_tensor& t, int es, bool required) {
  if (t.ptr == nullptr) return required ? fail(FCSA_ERR_INVALID_ARG, "%s: null pointer", name) : FCSA_OK;
  if ((reinterpret_cast<uintptr_t>(t.ptr) & 15) != 0) return fail(FCSA_ERR_INVALID_ARG, "%s: base not 16-byte aligned", name);
  const int64_t m = 16 / es;
  if (t.stride0 % m || t.stride1 % m || t.stride2 % m)
    return fail(FCSA_ERR_INVALID_ARG, "%s: strides (%lld, %lld, %lld) must keep rows 16-byte aligned", name,
                (long long)t.stride0, (long long)t.stride1, (long long)t.stride2);
  // the kernels address the rows of a 256-row tile with 32-bit byte offsets (buffer loads): keep a tile below 1 GiB
  if (t.stride2 < 0 || t.stride2 * es > (int64_t)(0x3fffffff / 256))
    return fail(FCSA_ERR_UNSUPPORTED, "%s: row stride %lld elements is negative or above 4 MiB", name, (long long)t.stride2);
  return FCSA_OK;
}

fcsa::View view(const fcsa_tensor& t, int es, bool zero_head_stride = false) {
  fcsa::View v;
  v.p = static_cast<char*>(t.ptr);
  v.sb = t.stride0 * es;
  v.sh = zero_head_stride ? 0 : t.stride1 * es;
  v.sn = t.stride2 * es;
  return v;
}

fcsa::View contiguous_view(void* p, int64_t heads, int64_t len, int64_t d, int es, bool zero_head_stride = false) {
  fcsa::View v;
  v.p = static_cast<char*>(p);
  v.sb = heads * len * d * es;
  v.sh = zero_head_stride ? 0 : len * d * es;
  v.sn = d * es;
  return v;
}

// Exponent shift (natural-log units): P~ = exp(s - shift).  Any shift gives the same O; only the saved
// inv_l carries it, and forward / backward derive it identically from the problem description.
//   * l2norm_qk == 0 (the reference extension's contract, q,k pre-normalised by the caller): shift = scale,
//     exactly cu:1216, so inv_l has the reference's values.
//   * fused l2norm: the logit lies in [-bound, +bound], bound = |scale| * groups.
//       f16 : shift = bound - 10  ->  P~ <= e^10 = 22026 < 65504, and typical P~ (logit ~ 0) stays in
//             f16's NORMAL range even for large scale (with the reference's shift, scale = 16 puts exp(-16)
//             = 1e-7 into f16 subnormals and the output error grows 10x).
//       bf16 / f32 (8-bit exponent): every P~ must stay a normal f32 and a row sum (up to ~1e5 keys of it) below f32's top:
//             exp(s - shift) in [e^-85, e^65]  <=>  shift in [bound - 65, 85 - bound], non-empty for bound <= 75.  The shift is
//             the reference's (= scale) wherever that lies in the interval, else the nearest end.  (Round 2 used
//             max(scale, bound - 40): the same values for bound <= 42, but it sent 60 < bound <= 75 -- C5 at the default scale 8 --
//             through the two-pass dynamic form, and it kept the reference's underflow for groups = 1, scale > 42.)
// A static shift only works while the whole logit range fits the exponent range of the type P~ is rounded to.  Real rows peak
// far below the theoretical bound once groups > 1 (found by the fuzz test: f16, groups >= 4, scale >= 8 underflowed every P~ of a
// row to 0; the reference's shift = scale overflows there instead).
// Beyond the safe range the forward kernel finds each row's max logit first and shifts by that ("dynamic"); what it saves
// for the backward is then log2(1 / sum_j exp(S_ij)) -- the value the backward kernels seed their S accumulators with anyway --
// so nothing ever holds exp() of the full logit range and there is no limit on scale * groups.
constexpr float kStaticTop = 65.f, kStaticBottom = 85.f;      // exp(s - shift) stays within [e^-85, e^65] (bf16 / f32)
// An additive bias makes the exponent unbounded.  bf16 / f32 absorb it inside the static window (e^-85 ... e^65 leaves +-20 around any
// shift; a strongly negative bias underflows to an exact 0 weight).  f16 does not: its static shift puts the largest logit at e^10 of a
// 65504 range, so a bias of +1.1 on such a logit overflowed P~ to inf (found by an exploratory fuzz seed in round 3: f16, scale 1, bias
// ~ N(0, 0.5)).  f16 problems WITH a bias therefore always take the per-row-reference form (whose online max includes the bias).
// bf16 / f32 WITH a bias: the static window only has room for the bias while the logits themselves leave it: with shift = scale the
// largest exponent is (bound - scale) + bias, and e^88 is f32's top (inf -> NaN rows).  Up to bound = scale * groups = 40 that leaves
// a positive bias at least +45 of headroom on top of ln(M) for the row sum (the documented limit of the static form, include/fcsa.h);
// beyond it -- round 3 drew the line at 60, where the headroom was down to +23 ... +36 (round 4 advice) -- problems with a bias take
// the per-row form, whose online reference includes the bias and has no limit at all.
constexpr float kStaticBoundBias = 40.f;
bool dynamic_shift(const fcsa_problem& p, bool has_bias) {
  if (!p.l2norm_qk) return false;
  const float bound = fabsf(p.scale) * (float)p.groups;
  if (p.dtype == FCSA_F16) return has_bias || bound > 11.f;
  return 2.f * bound > kStaticTop + kStaticBottom || (has_bias && bound > kStaticBoundBias);
}

float exponent_shift(const fcsa_problem& p, bool has_bias) {
  if (!p.l2norm_qk) return p.scale;
  if (dynamic_shift(p, has_bias)) return 0.f;
  const float bound = fabsf(p.scale) * (float)p.groups;
  if (p.dtype == FCSA_F16) return bound - 10.f;
  const float lo = bound - kStaticTop, hi = kStaticBottom - bound;
  return p.scale < lo ? lo : (p.scale > hi ? hi : p.scale);
}

// Row-sum clamp: the reference clamps l at 1e-10 (cu:83, cu:1239) with shift = scale; with another shift the
// same clamp in the reference's units is 1e-10 * exp(scale - shift) (kept inside f32's normal range).
float rowsum_eps(const fcsa_problem& p, bool has_bias) {
  if (dynamic_shift(p, has_bias)) return 1e-30f;          // row sums are >= 1 there (the max element contributes exp(0))
  float e = 1e-10f * expf(p.scale - exponent_shift(p, has_bias));
  if (!(e > 1e-37f)) e = 1e-37f;
  if (e > 1e30f) e = 1e30f;
  return e;
}

int log2_blocks_per_group(const fcsa_problem& p) {     // log2(group size / 8), or -1 if not a power of two of 8-blocks
  const int dg = p.dim_head / (p.groups > 0 ? p.groups : 1);
  if (dg % 8 != 0) return -1;
  int m = dg / 8, lg = 0;
  while ((1 << lg) < m) ++lg;
  // ONE group over the whole head (groups = 1) may be any number of 8-blocks: the fused forms sum over the power-of-two lane / k-step
  // block that contains the row, and the padding positions of that block contribute nothing (RowEpilogue: lanes c >= D / 8 hold 0;
  // finish_q_frags: k-steps >= KS do not exist).  D = 96: 12 blocks -> 4.  (Round 6; until then D = 96 took the slab + finalize path.)
  if (p.groups <= 1) return lg;
  return (1 << lg) == m ? lg : -1;
}
bool fusable_groups(const fcsa_problem& p) { return log2_blocks_per_group(p) >= 0; }

// What a backward call runs: split counts, which gradients go through f32 slabs + the finalize kernel, fused l2norm, group sweep.
struct BwdPlan {
  bool fuse_norm;         // the l2norm backward is fused into the dQ / dK/dV epilogues (every group 8 * 2^k features wide)
  bool kv_sweep;          // grouped-query K/V: the dK/dV kernel sums each K/V head's group in registers (no dk / dv slabs)
  int dq_splits;          // > 1: split-key dQ kernel, dq_splits partial slabs
  int dkv_splits;         // > 1: split-query dK/dV kernel, dkv_splits partial dk / dv slabs each
  bool dq_slab, dk_slab, dv_slab;
};
// What the plan depends on beyond the problem: whether the call has an attn_bias, and whether (batch, head) is one flat index of the dq
// (dk and dv) outputs -- the finalize kernel sums split slabs per (batch * head) row block.
struct BwdCall { bool bias, dq_flat, dkv_flat; };

// call == nullptr: the most any call of the problem needs, which the workspace is sized for.  varlen: packed sequences (p is then the
// [1, H, total, D] problem of the packed rows), which take neither a split nor the group sweep
BwdPlan bwd_plan(const fcsa_problem& p, const BwdCall* call, bool varlen = false) {
  BwdPlan b;
  const int cus = fcsa::cu_count();
  // K/V heads fewer than query heads (single-headed or grouped): the dK/dV kernel writes per-query-head f32 slabs that the finalize kernel
  // sums over each K/V head's group -- except for the group sweep, which runs where dkv_sweep says so for a bias-free launch with
  // epilogues that finish the job (no l2norm groups that need the finalize kernel).  A launch with an attn_bias takes the slab route.
  const bool grouped = p.kv_heads != p.heads;
  const bool sweep = !varlen && p.kv_heads > 1 && grouped && (p.l2norm_qk == 0 || fusable_groups(p)) &&
                     fcsa::dkv_sweep(elem_size(p.dtype), p.dim_head, (int64_t)p.batch * p.kv_heads, p.k_len, p.causal != 0, fcsa::kv_group_mode(-1), cus);
  b.kv_sweep = sweep && call != nullptr && !call->bias;
  // the l2norm backward is fused into the dQ / dKV epilogues when every group is 8 * 2^k features wide; otherwise (odd group sizes) the
  // kernels write f32 slabs that the finalize kernel differentiates
  b.fuse_norm = p.l2norm_qk != 0 && fusable_groups(p);
  const bool norm_slab = p.l2norm_qk != 0 && !b.fuse_norm;
  // split dQ: flat dq, and causal splits only in bias-free kernels; split dK/dV: flat dk / dv (or per-query-head slabs anyway), bias-free,
  // never with the group sweep
  b.dq_splits = varlen || (call != nullptr && !(call->dq_flat && !(p.causal && call->bias))) ? 1 : fcsa::backward_dq_splits(p, cus);
  b.dkv_splits = varlen || sweep || (call != nullptr && !((call->dkv_flat || grouped) && !call->bias)) ? 1 : fcsa::backward_dkv_splits(p, cus);
  b.dq_slab = b.dq_splits > 1 || norm_slab;
  b.dk_slab = !b.kv_sweep && (b.dkv_splits > 1 || grouped || norm_slab);
  b.dv_slab = !b.kv_sweep && (b.dkv_splits > 1 || grouped);
  return b;
}

// workspace: delta [B,H,N] f32, then the slabs of the largest plan
struct BwdLayout { size_t delta, dq_slab, dk_slab, dv_slab, total; };
BwdLayout bwd_layout(const fcsa_problem& p, bool varlen = false) {
  const BwdPlan b = bwd_plan(p, nullptr, varlen);
  const size_t qn = (size_t)p.batch * p.heads * p.q_len;
  const size_t kn = (size_t)p.batch * p.heads * p.k_len;      // slabs are per q-head
  BwdLayout L;
  size_t off = 0;
  L.delta = off;   off = align_up(off + qn * 4, 256);
  L.dq_slab = off; off = align_up(off + (b.dq_slab ? qn * p.dim_head * 4 * (size_t)b.dq_splits : 0), 256);
  L.dk_slab = off; off = align_up(off + (b.dk_slab ? kn * p.dim_head * 4 * (size_t)b.dkv_splits : 0), 256);
  L.dv_slab = off; off = align_up(off + (b.dv_slab ? kn * p.dim_head * 4 * (size_t)b.dkv_splits : 0), 256);
  L.total = off;
  return L;
}

int launch_check(hipError_t e, const char* what) {
  if (e != hipSuccess) return fail(FCSA_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
  return FCSA_OK;
}

// ---- optional per-kernel timing (fcsa_profile_*) -------------------------------------------------
struct TimedLaunch { const char* name; hipEvent_t start, stop; };
std::mutex g_prof_mu;
std::atomic<bool> g_prof_on{false};       // read lock-free on every launch; the mutex only guards the record list
std::vector<TimedLaunch> g_prof;

// run one kernel launch, bracketed by events on ITS stream when profiling is enabled
template <typename F> int timed(const char* name, const char* what, hipStream_t s, F&& launch) {
  if (!g_prof_on.load(std::memory_order_relaxed)) return launch_check(launch(), what);
  TimedLaunch t{name, nullptr, nullptr};
  if (hipEventCreate(&t.start) != hipSuccess || hipEventCreate(&t.stop) != hipSuccess)
    return fail(FCSA_ERR_LAUNCH, "%s: hipEventCreate failed", what);
  (void)hipEventRecord(t.start, s);
  const hipError_t e = launch();
  (void)hipEventRecord(t.stop, s);
  { std::lock_guard<std::mutex> g(g_prof_mu); g_prof.push_back(t); }
  return launch_check(e, what);
}

// Packed variable-length sequences (fcsa_varlen): the table is checked as far as the host can see it (never its device contents), and
// the call is described by the problem of the packed rows -- batch 1, q_len = total_q, k_len = total_k -- which the row kernels (l2norm,
// its backward, finalize), the workspace layout and the zero-size rules use unchanged; only the attention launches get the sequence
// table, with B = sequences and N / M = the longest spans (a.p.q_len / k_len).
int check_varlen(const fcsa_problem& p, const fcsa_varlen* v, bool mask, bool bias) {
  if (v == nullptr) return fail(FCSA_ERR_INVALID_ARG, "varlen: null sequence table");
  if (mask || bias) return fail(FCSA_ERR_INVALID_ARG, "varlen: mask and attn_bias are not supported with packed sequences");
  if (v->total_q < 0 || v->total_k < 0 || v->total_q > INT32_MAX || v->total_k > INT32_MAX)
    return fail(FCSA_ERR_INVALID_ARG, "varlen: total_q / total_k (%lld, %lld) outside [0, 2^31)", (long long)v->total_q, (long long)v->total_k);
  if (p.batch > 0 && (v->cu_seqlens_q == nullptr || v->cu_seqlens_k == nullptr))
    return fail(FCSA_ERR_INVALID_ARG, "varlen: null cu_seqlens");
  if ((int64_t)p.heads * (v->total_q > v->total_k ? v->total_q : v->total_k) > INT32_MAX)
    return fail(FCSA_ERR_UNSUPPORTED, "varlen: heads x packed rows above 2^31");
  return FCSA_OK;
}
fcsa_problem packed_problem(const fcsa_problem& p, const fcsa_varlen& v) {
  fcsa_problem d = p;
  d.batch = 1;
  d.q_len = (int32_t)v.total_q;
  d.k_len = (int32_t)v.total_k;
  return d;
}
// a varlen call: the table and the caller's problem (batch = sequences, q_len / k_len = the longest spans)
struct VarlenCall { const fcsa_varlen* t; int batch, max_q, max_k; };
fcsa::SeqTable seq_table(const fcsa_varlen* v) {      // nullptr: a dense call
  if (v == nullptr) return fcsa::SeqTable{nullptr, nullptr, 0, 0};
  return fcsa::SeqTable{v->cu_seqlens_q, v->cu_seqlens_k, (int)v->total_q, (int)v->total_k};
}
fcsa_tensor packed(fcsa_tensor t) {       // stride0 of a packed tensor is meaningless: one "batch" of total rows
  t.stride0 = 0;
  return t;
}

// a sliding-window call after the host's normalisation (fcsa::win_normalise): the sides as the kernels take them
struct WindowCall { int lo, hi; };
int check_window(const fcsa_window* w, bool mask, bool bias) {
  if (w == nullptr) return fail(FCSA_ERR_INVALID_ARG, "window: null window");
  if (w->left < -1 || w->right < -1) return fail(FCSA_ERR_INVALID_ARG, "window: left / right (%d, %d) must be >= 0, or -1 for unbounded", w->left, w->right);
  if (mask || bias) return fail(FCSA_ERR_INVALID_ARG, "window: mask and attn_bias are not supported with a sliding window");
  return FCSA_OK;
}

// the checks of a call with slopes (fcsa_forward_alibi / fcsa_backward_alibi): its options, its window where it has one, the slopes
int check_alibi(const fcsa_problem& p, const fcsa_varlen* seqs, const fcsa_window* w, const fcsa_alibi* al, bool mask, bool bias) {
  if (mask || bias) return fail(FCSA_ERR_INVALID_ARG, "alibi: mask and attn_bias are not supported with alibi_slopes");
  if (w != nullptr) {
    if (int rc = check_window(w, false, false)) return rc;
  }
  if (al == nullptr || al->slopes == nullptr) return fail(FCSA_ERR_INVALID_ARG, "alibi: null slopes");
  if ((reinterpret_cast<uintptr_t>(al->slopes) & 3) != 0) return fail(FCSA_ERR_INVALID_ARG, "alibi: slopes not 4-byte aligned");
  if (al->reserved != 0) return fail(FCSA_ERR_INVALID_ARG, "alibi: reserved must be 0");
  if (seqs == nullptr && !p.causal && p.q_len > p.k_len)
    return fail(FCSA_ERR_INVALID_ARG, "alibi: a non-causal call needs q_len <= k_len (%d > %d): rows with pos_i < 0 have no key at distance 0", p.q_len, p.k_len);
  return FCSA_OK;
}

// split-key forward (fcsa::forward_splits: bias-free launches only): the count, and its workspace -- partial P~V, then partial row sums
int forward_splits(const fcsa_problem& p) {
  if (p.batch <= 0 || p.heads <= 0 || p.q_len <= 0 || p.dim_head <= 0) return 1;
  return fcsa::forward_splits(p, dynamic_shift(p, false), fcsa::cu_count());
}
size_t forward_ws_bytes(const fcsa_problem& p, int splits) {
  if (splits <= 1) return 0;
  const size_t rows = (size_t)splits * p.batch * p.heads * p.q_len;
  return align_up(rows * p.dim_head * 4, 256) + align_up(rows * 4, 256);
}

// Zero-size problems (empty tensors: what torch hands over has NULL data pointers then).  batch, heads or q_len == 0: the forward has no
// output element; k_len == 0: every query row is a row without a valid key, for which the kernels' semantics are o = 0 (cu:1239) and
// finite (zero) gradients.  Nothing is launched; the outputs that DO have elements are zero-filled on the caller's stream, row by row
// (any strides).  The reference launches a zero-sized grid there (a CUDA error it prints and ignores, cu:17-28).
int zero_rows(const char* name, const fcsa_tensor& t, int es, int B, int H, int L, int D, hipStream_t s) {
  if (B <= 0 || H <= 0 || L <= 0) return FCSA_OK;
  if (int rc = check_tensor(name, t, es, true)) return rc;
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < H; ++h) {
      char* base = static_cast<char*>(t.ptr) + ((int64_t)b * t.stride0 + (int64_t)h * t.stride1) * es;
      const hipError_t e = t.stride2 == D ? hipMemsetAsync(base, 0, (size_t)L * D * es, s)
                                          : hipMemset2DAsync(base, (size_t)t.stride2 * es, 0, (size_t)D * es, (size_t)L, s);
      if (e != hipSuccess) return fail(FCSA_ERR_LAUNCH, "%s: zero fill failed: %s", name, hipGetErrorString(e));
    }
  return FCSA_OK;
}

// ---- the training calls (fcsa_forward, fcsa_backward and their _varlen, _window, _alibi and _state forms) -------------------------------
// One description of a training call, TrainCall, and one implementation per direction (train_forward, train_backward) behind the nine
// entry points: what an entry point adds to the plain call is an optional part of the description.
enum class TrainNeeds { Nothing, Seqs, Window, Slopes };      // the part an entry point requires: NULL there is refused, not "absent"
struct TrainCall {
  TrainNeeds needs;
  const fcsa_forward_args* fwd;           // the caller's arguments: of train_forward ...
  const fcsa_backward_args* bwd;          // ... or of train_backward
  const fcsa_varlen* seqs;                // packed sequences, or NULL
  const fcsa_window* w;                   // a sliding window as the caller gave it, or NULL
  const fcsa_alibi* alibi = nullptr;      // the slopes of a linear position bias (TrainNeeds::Slopes)
  const float* d_lse = nullptr;           // the LSE gradient of fcsa_backward_state, or NULL
};

// The window of a training call as the kernels take it (fcsa::win_normalise, on the caller's lengths: a packed call's longest spans).
// true: a windowed launch (the windowed kernel forms; the plan of a packed call: no split, no group sweep) with the sides in `win`.
// false: no window, or one that hides nothing, which is the un-windowed or the causal call: p.causal then says which.  A call with slopes
// always keeps sides -- (open, open) and (open, 0) included, which the windowed kernel forms serve like any other pair.
bool train_window(fcsa_problem& p, const fcsa_window* w, bool slopes, WindowCall& win) {
  if (w == nullptr && !slopes) return false;
  const fcsa::WinKind kind = fcsa::win_normalise(p.q_len, p.k_len, p.causal != 0, w != nullptr ? w->left : -1, w != nullptr ? w->right : -1, win.lo, win.hi);
  if (slopes || kind == fcsa::WinKind::Window) return true;
  p.causal = kind == fcsa::WinKind::Causal ? 1 : 0;
  return false;
}

// What the launches take of a call's options
struct TrainLaunch {
  bool slopes, windowed, packed;
  fcsa::TrainAlibi al;      // slopes
  WindowCall win;           // windowed
  VarlenCall vl;            // packed
};

// What every training call starts with, once and in this order: the problem; the checks of its options -- the slopes with their window, or
// the window, then the sequence table --; the window's normalisation; the packing, after which p is the problem of the packed rows.
int train_options(const TrainCall& c, fcsa_problem& p, bool mask, bool bias, TrainLaunch& t) {
  if (int rc = check_problem(p)) return rc;
  t.slopes = c.needs == TrainNeeds::Slopes;
  if (t.slopes) {
    if (int rc = check_alibi(p, c.seqs, c.w, c.alibi, mask, bias)) return rc;
    t.al = fcsa::TrainAlibi{c.alibi->slopes, c.alibi->stride_b, c.alibi->stride_h};
  } else if (c.w != nullptr || c.needs == TrainNeeds::Window) {
    if (int rc = check_window(c.w, mask, bias)) return rc;
  }
  t.windowed = train_window(p, c.w, t.slopes, t.win);
  t.packed = c.seqs != nullptr || c.needs == TrainNeeds::Seqs;
  if (t.packed) {
    if (int rc = check_varlen(p, c.seqs, mask, bias)) return rc;
    t.vl = {c.seqs, p.batch, p.q_len, p.k_len};
    p = packed_problem(p, *c.seqs);
  }
  return FCSA_OK;
}

// The backward workspace of a (p, seqs, window, slopes?) call: that of the launch train_backward makes of it.  (With slopes the window
// plays no part: always the plan of a windowed launch.)
size_t bwd_workspace(fcsa_problem p, const fcsa_varlen* seqs, const fcsa_window* w, bool slopes) {
  if (seqs != nullptr && (seqs->total_q < 0 || seqs->total_k < 0)) return 0;
  WindowCall win;
  const bool windowed = train_window(p, w, slopes, win);
  if (seqs != nullptr) p = packed_problem(p, *seqs);
  return bwd_layout(p, seqs != nullptr || windowed).total;
}

int train_forward(const TrainCall& c) {
  if (c.fwd == nullptr) return fail(FCSA_ERR_INVALID_ARG, "null args");
  fcsa_forward_args call = *c.fwd;      // the call as the launches see it: a collapsed window's `causal`, a packed call's problem and views
  TrainLaunch t;
  if (int rc = train_options(c, call.p, call.mask != nullptr, call.attn_bias != nullptr, t)) return rc;
  if (t.packed) { call.q = packed(call.q); call.k = packed(call.k); call.v = packed(call.v); call.o = packed(call.o); }
  const fcsa_forward_args* a = &call;
  const fcsa_problem& p = a->p;
  if (p.causal && a->mask != nullptr) return fail(FCSA_ERR_INVALID_ARG, "mask should not be given if causal (cu:1675)");
  const int es = elem_size(p.dtype);
  if (p.batch == 0 || p.heads == 0 || p.q_len == 0) return FCSA_OK;      // no output element (k-side saved state is not needed by a backward either)
  if (p.k_len == 0) {                                                     // rows without a key: o = 0; inv_l = 1 (never read: the backward below has no key to visit)
    hipStream_t s0 = static_cast<hipStream_t>(a->stream);
    if (int rc = zero_rows("o", a->o, es, p.batch, p.heads, p.q_len, p.dim_head, s0)) return rc;
    if (a->inv_l != nullptr) {
      const float one = 1.f;
      uint32_t bits; memcpy(&bits, &one, 4);
      if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a->inv_l), (int)bits, (size_t)p.batch * p.heads * p.q_len, s0) != hipSuccess)
        return fail(FCSA_ERR_LAUNCH, "inv_l: fill failed");
    }
    return FCSA_OK;
  }
  if (int rc = check_tensor("q", a->q, es, true)) return rc;
  if (int rc = check_tensor("k", a->k, es, true)) return rc;
  if (int rc = check_tensor("v", a->v, es, true)) return rc;
  if (int rc = check_tensor("o", a->o, es, true)) return rc;
  hipStream_t s = static_cast<hipStream_t>(a->stream);
  const bool single = p.kv_heads == 1 && p.heads > 1;      // one K/V head: stride-0 head views; grouped K/V: kv_group query heads per K/V head

  fcsa::FwdWinParams fp;
  fp.kv_group = single ? 1 : p.heads / p.kv_heads;
  bool fuse_q = false;
  fp.q = view(a->q, es);
  fp.k = view(a->k, es, single);
  fp.v = view(a->v, es, single);
  fp.o = view(a->o, es);
  if (p.l2norm_qk) {
    const fcsa_norm_state& n = a->norm;
    if (n.kn == nullptr) return fail(FCSA_ERR_INVALID_ARG, "l2norm_qk needs the norm.kn buffer");
    if (n.qn == nullptr && fcsa_forward_needs_qn(&p, a->inv_l != nullptr || n.rq != nullptr))
      return fail(FCSA_ERR_INVALID_ARG, "l2norm_qk needs the norm.qn buffer for this problem (fcsa_forward_needs_qn)");
    fcsa::NormParams nq, nk;
    nq.eps = nk.eps = 1e-12f;
    nq.D = nk.D = p.dim_head; nq.G = nk.G = p.groups;
    nq.x = fp.q; nq.xn = static_cast<char*>(n.qn); nq.inv_norm = n.rq;
    nq.B = p.batch; nq.H = p.heads; nq.L = p.q_len;
    nq.out_scale = p.scale * kLog2e;       // qn = c1 * q^ (one rounding): the kernels then need no per-logit multiply
    nk.x = view(a->k, es); nk.xn = static_cast<char*>(n.kn); nk.inv_norm = n.rk;
    nk.B = p.batch; nk.H = p.kv_heads; nk.L = p.k_len;
    nk.out_scale = 1.f;
    // 16-bit types with group sizes of 8 * 2^k: q is normalised in the forward kernel's prologue (load_q_frags), which also
    // writes qn / rq for the backward; only k takes the HBM pass.  Otherwise both go through the row kernel.
    fuse_q = p.dtype != FCSA_F32 && fusable_groups(p);
    if (fuse_q) {
      if (int rc = timed("l2norm", "l2norm(k)", s, [&] { return fcsa::launch_l2norm(p.dtype, nk, s); })) return rc;
    } else {
      if (int rc = timed("l2norm", "l2norm(q,k)", s, [&] { return fcsa::launch_l2norm_pair(p.dtype, nq, nk, s); })) return rc;
    }
    if (!fuse_q) fp.q = contiguous_view(n.qn, p.heads, p.q_len, p.dim_head, es);
    fp.k = contiguous_view(n.kn, p.kv_heads, p.k_len, p.dim_head, es, single);
  }
  fp.inv_l = a->inv_l;
  fp.mask = a->mask;
  fp.bias = static_cast<const char*>(a->attn_bias);
  fp.B = p.batch; fp.H = p.heads; fp.N = p.q_len; fp.M = p.k_len;
  fp.seq = seq_table(t.packed ? t.vl.t : nullptr);
  if (t.packed) { fp.B = t.vl.batch; fp.N = t.vl.max_q; fp.M = t.vl.max_k; }      // the sequences and their longest spans
  fp.causal = p.causal; fp.bias_batch = p.bias_batch_dim;
  if (t.windowed) { fp.window = 1; fp.win_lo = t.win.lo; fp.win_hi = t.win.hi; fp.causal = 1; }      // (a causal launch with moved diagonals: fcsa_dispatch.h)
  fp.c1 = p.scale * kLog2e;
  const bool has_bias = a->attn_bias != nullptr;
  fp.c2 = exponent_shift(p, has_bias) * kLog2e;
  fp.bias_c = kLog2e;
  fp.l_eps = rowsum_eps(p, has_bias);
  fp.q_scaled = p.l2norm_qk ? 1 : 0;
  fp.q_raw = fuse_q ? 1 : 0;
  fp.qn_out = fuse_q ? static_cast<char*>(a->norm.qn) : nullptr;
  fp.rq_out = fuse_q ? a->norm.rq : nullptr;
  fp.G = p.groups; fp.lgm = fuse_q ? log2_blocks_per_group(p) : 0; fp.norm_eps = 1e-12f;
  fp.dyn = dynamic_shift(p, has_bias) ? 1 : 0;      // then inv_l holds log2 of the normaliser
  fp.splits = 1; fp.ws_o = nullptr; fp.ws_l = nullptr;
  if (a->workspace != nullptr && a->attn_bias == nullptr && !t.packed && !t.windowed) {      // (packed and windowed launches never split)
    const int sp = forward_splits(p);
    if (sp > 1 && a->workspace_bytes >= forward_ws_bytes(p, sp) && (reinterpret_cast<uintptr_t>(a->workspace) & 255) == 0) {
      const size_t rows = (size_t)sp * p.batch * p.heads * p.q_len;
      fp.splits = sp;
      fp.ws_o = static_cast<float*>(a->workspace);
      fp.ws_l = reinterpret_cast<float*>(static_cast<char*>(a->workspace) + align_up(rows * p.dim_head * 4, 256));
    }
  }
  if (t.slopes) return timed("fwd", "forward", s, [&] { return fcsa::launch_forward_alibi(p.dtype, p.dim_head, fp, t.al, s); });
  return timed("fwd", "forward", s, [&] { return fcsa::launch_forward(p.dtype, p.dim_head, fp, s); });
}

int train_backward(const TrainCall& c) {
  if (c.bwd == nullptr) return fail(FCSA_ERR_INVALID_ARG, "null args");
  fcsa_backward_args call = *c.bwd;      // the call as the launches see it, as in train_forward
  TrainLaunch t;
  if (int rc = train_options(c, call.p, call.mask != nullptr, call.attn_bias != nullptr || call.d_bias != nullptr, t)) return rc;
  if (t.packed) {
    call.d_out = packed(call.d_out); call.o = packed(call.o); call.q = packed(call.q); call.k = packed(call.k); call.v = packed(call.v);
    call.dq = packed(call.dq); call.dk = packed(call.dk); call.dv = packed(call.dv);
  }
  const fcsa_backward_args* a = &call;
  const fcsa_problem& p = a->p;
  if (p.causal && a->mask != nullptr) return fail(FCSA_ERR_INVALID_ARG, "mask should not be given if causal (cu:1675)");
  const int es = elem_size(p.dtype);
  if (p.batch == 0 || p.heads == 0) return FCSA_OK;                        // every gradient is empty
  if (p.q_len == 0 || p.k_len == 0) {                                      // no (query, key) pair: the gradients that have elements are zero (d_bias has none)
    hipStream_t s0 = static_cast<hipStream_t>(a->stream);
    if (int rc = zero_rows("dq", a->dq, es, p.batch, p.heads, p.q_len, p.dim_head, s0)) return rc;
    if (int rc = zero_rows("dk", a->dk, es, p.batch, p.kv_heads, p.k_len, p.dim_head, s0)) return rc;
    return zero_rows("dv", a->dv, es, p.batch, p.kv_heads, p.k_len, p.dim_head, s0);
  }
  if (int rc = check_tensor("d_out", a->d_out, es, true)) return rc;
  if (int rc = check_tensor("o", a->o, es, true)) return rc;
  if (int rc = check_tensor("v", a->v, es, true)) return rc;
  if (int rc = check_tensor("dq", a->dq, es, true)) return rc;
  if (int rc = check_tensor("dk", a->dk, es, true)) return rc;
  if (int rc = check_tensor("dv", a->dv, es, true)) return rc;
  if (!p.l2norm_qk) {
    if (int rc = check_tensor("q", a->q, es, true)) return rc;
    if (int rc = check_tensor("k", a->k, es, true)) return rc;
  } else if (a->norm.qn == nullptr || a->norm.kn == nullptr || a->norm.rq == nullptr || a->norm.rk == nullptr) {
    return fail(FCSA_ERR_INVALID_ARG, "l2norm_qk backward needs norm.qn, norm.kn, norm.rq, norm.rk from forward");
  }
  if (a->inv_l == nullptr) return fail(FCSA_ERR_INVALID_ARG, "inv_l: null pointer");
  if (a->attn_bias == nullptr && a->d_bias != nullptr) return fail(FCSA_ERR_INVALID_ARG, "d_bias without attn_bias");
  const bool no_split = t.packed || t.windowed;
  const BwdLayout L = bwd_layout(p, no_split);
  if (a->workspace == nullptr || a->workspace_bytes < L.total)
    return fail(FCSA_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", a->workspace_bytes, L.total);
  if ((reinterpret_cast<uintptr_t>(a->workspace) & 255) != 0) return fail(FCSA_ERR_WORKSPACE, "workspace not 256-byte aligned");

  hipStream_t s = static_cast<hipStream_t>(a->stream);
  const bool single = p.kv_heads == 1 && p.heads > 1;      // stride-0 K/V head views
  const bool grouped = p.kv_heads != p.heads;             // single-headed or grouped-query K/V: dk / dv are sums over query heads
  const BwdCall bc = {a->attn_bias != nullptr, a->dq.stride0 == (int64_t)p.heads * a->dq.stride1,
                      a->dk.stride0 == (int64_t)p.heads * a->dk.stride1 && a->dv.stride0 == (int64_t)p.heads * a->dv.stride1};
  const BwdPlan plan = bwd_plan(p, &bc, no_split);
  const int dq_splits = plan.dq_splits, dkv_splits = plan.dkv_splits;
  const bool dq_slab = plan.dq_slab, dk_slab = plan.dk_slab, dv_slab = plan.dv_slab;
  char* ws = static_cast<char*>(a->workspace);

  fcsa::BwdWinParams bp;
  bp.kv_group = single ? 1 : p.heads / p.kv_heads;
  bp.kv_sweep = plan.kv_sweep ? 1 : 0;
  if (p.l2norm_qk) {
    bp.q = contiguous_view(a->norm.qn, p.heads, p.q_len, p.dim_head, es);
    bp.k = contiguous_view(a->norm.kn, p.kv_heads, p.k_len, p.dim_head, es, single);
  } else {
    bp.q = view(a->q, es);
    bp.k = view(a->k, es, single);
  }
  bp.v = view(a->v, es, single);
  bp.o = view(a->o, es);
  bp.d_out = view(a->d_out, es);
  const bool want_dbias = a->attn_bias != nullptr && a->d_bias != nullptr;
  bp.dq_splits = dq_splits;
  bp.dq_split_stride = (int64_t)p.q_len * p.dim_head * 4;
  bp.dkv_splits = dkv_splits;
  bp.dkv_split_stride = (int64_t)p.k_len * p.dim_head * 4;
  bp.dq_f32 = dq_slab;
  bp.dk_f32 = dk_slab;
  bp.dv_f32 = dv_slab;
  if (dq_splits > 1) {          // slab layout [batch * heads][split][N][D]: (b, h) block stride = splits * N * D floats
    bp.dq.p = ws + L.dq_slab;
    bp.dq.sn = (int64_t)p.dim_head * 4;
    bp.dq.sh = (int64_t)dq_splits * p.q_len * p.dim_head * 4;
    bp.dq.sb = (int64_t)p.heads * bp.dq.sh;
  } else {
    bp.dq = dq_slab ? contiguous_view(ws + L.dq_slab, p.heads, p.q_len, p.dim_head, 4) : view(a->dq, es);
  }
  if (dkv_splits > 1) {         // slab layout [batch * heads][split][M][D], like the split dq slabs
    bp.dk.p = ws + L.dk_slab;
    bp.dk.sn = (int64_t)p.dim_head * 4;
    bp.dk.sh = (int64_t)dkv_splits * p.k_len * p.dim_head * 4;
    bp.dk.sb = (int64_t)p.heads * bp.dk.sh;
    bp.dv = bp.dk;
    bp.dv.p = ws + L.dv_slab;
  } else {
    bp.dk = dk_slab ? contiguous_view(ws + L.dk_slab, p.heads, p.k_len, p.dim_head, 4) : view(a->dk, es);
    bp.dv = dv_slab ? contiguous_view(ws + L.dv_slab, p.heads, p.k_len, p.dim_head, 4) : view(a->dv, es);
  }
  bp.inv_l = a->inv_l;
  bp.delta = reinterpret_cast<float*>(ws + L.delta);
  bp.dlse = c.d_lse;
  bp.mask = a->mask;
  bp.bias = static_cast<const char*>(a->attn_bias);
  bp.d_bias = a->d_bias;
  bp.B = p.batch; bp.H = p.heads; bp.N = p.q_len; bp.M = p.k_len;
  bp.seq = seq_table(t.packed ? t.vl.t : nullptr);
  if (t.packed) { bp.B = t.vl.batch; bp.N = t.vl.max_q; bp.M = t.vl.max_k; }
  bp.causal = p.causal; bp.bias_batch = p.bias_batch_dim;
  if (t.windowed) { bp.window = 1; bp.win_lo = t.win.lo; bp.win_hi = t.win.hi; bp.causal = 1; }
  bp.c1 = p.scale * kLog2e;
  bp.c2 = exponent_shift(p, a->attn_bias != nullptr) * kLog2e;
  bp.invl_log2 = dynamic_shift(p, a->attn_bias != nullptr) ? 1 : 0;
  bp.bias_c = kLog2e;
  bp.scale = p.scale;
  bp.q_scaled = p.l2norm_qk ? 1 : 0;
  bp.G = p.groups; bp.lgm = plan.fuse_norm ? log2_blocks_per_group(p) : 0; bp.norm_eps = 1e-12f;
  bp.rq = (plan.fuse_norm && dq_splits <= 1) ? a->norm.rq : nullptr;    // fused: dq kernel writes the final dq
  bp.rk = (plan.fuse_norm && (!grouped || plan.kv_sweep) && dkv_splits <= 1) ? a->norm.rk : nullptr;          // fused: dkv kernel writes the final dk

  // 1. dQ (also publishes delta), 2. dK/dV, 3. head reduction + l2norm backward where needed
  if (t.slopes) {
    if (int rc = timed("bwd_dq", "backward dq", s, [&] { return fcsa::launch_backward_dq_alibi(p.dtype, p.dim_head, bp, t.al, s); })) return rc;
    if (int rc = timed("bwd_dkv", "backward dkv", s, [&] { return fcsa::launch_backward_dkv_alibi(p.dtype, p.dim_head, bp, t.al, s); })) return rc;
  } else {
    if (int rc = timed("bwd_dq", "backward dq", s, [&] { return fcsa::launch_backward_dq(p.dtype, p.dim_head, bp, s); })) return rc;
    if (int rc = timed("bwd_dkv", "backward dkv", s, [&] { return fcsa::launch_backward_dkv(p.dtype, p.dim_head, bp, s); })) return rc;
  }
  if (want_dbias) {      // d_bias from recomputed dS tiles; needs delta, which the dQ kernel published
    if (int rc = timed("bwd_dbias", "backward d_bias", s, [&] { return fcsa::launch_backward_dbias(p.dtype, p.dim_head, bp, s); })) return rc;
  }

  fcsa::NormBwdParams nb;
  nb.eps = 1e-12f;
  nb.D = p.dim_head;
  nb.B = p.batch;
  nb.xn_scale = 1.f;
  if (dq_splits > 1) {          // sum the split slabs ("heads" of a flat (batch * head) batch), then the l2norm backward if any
    nb.B = p.batch * p.heads;
    nb.slab = ws + L.dq_slab; nb.slab_f32 = 1; nb.HS = dq_splits; nb.HO = 1; nb.L = p.q_len;
    if (p.l2norm_qk) { nb.xn = static_cast<const char*>(a->norm.qn); nb.inv_norm = a->norm.rq; nb.G = p.groups; nb.xn_scale = 1.f / (p.scale * kLog2e); }
    else             { nb.xn = nullptr; nb.inv_norm = nullptr; nb.G = 1; }
    nb.dx = view(a->dq, es);
    nb.dx.sb = nb.dx.sh;          // flat (batch * head) index: stride0 == heads * stride1 (checked above)
    nb.dx.sh = 0;
  } else if (dq_slab) {
    nb.slab = ws + L.dq_slab; nb.slab_f32 = 1; nb.HS = p.heads; nb.HO = p.heads; nb.L = p.q_len;
    nb.xn = static_cast<const char*>(a->norm.qn); nb.inv_norm = a->norm.rq; nb.G = p.groups;
    nb.xn_scale = 1.f / (p.scale * kLog2e);           // qn holds c1 * q^
    nb.dx = view(a->dq, es);
  }
  // (the dq pass is launched below, together with the dk / dv passes where there are any: one grid instead of two or three)
  const fcsa::NormBwdParams nq = nb;
  nb.B = p.batch;
  fcsa::NormBwdParams nk = nb, nv = nb;
  if (dk_slab) {
    nk.slab = ws + L.dk_slab; nk.slab_f32 = 1; nk.HS = p.heads; nk.HO = p.kv_heads; nk.L = p.k_len;
    nk.xn_scale = 1.f;
    if (p.l2norm_qk) { nk.xn = static_cast<const char*>(a->norm.kn); nk.inv_norm = a->norm.rk; nk.G = p.groups; }
    else             { nk.xn = nullptr; nk.inv_norm = nullptr; nk.G = 1; }
    nk.dx = view(a->dk, es);
  }
  if (dv_slab) {
    nv.slab = ws + L.dv_slab; nv.slab_f32 = 1; nv.HS = p.heads; nv.HO = p.kv_heads; nv.L = p.k_len;
    nv.xn = nullptr; nv.inv_norm = nullptr; nv.G = 1; nv.xn_scale = 1.f;
    nv.dx = view(a->dv, es);
  }
  if (dkv_splits > 1) {         // the splits are the "heads" of a flat (batch * head) batch, summed down to one
    for (fcsa::NormBwdParams* n : {&nk, &nv}) {
      if (grouped) {              // slabs [batch][heads x splits][M][D]: each K/V head sums its group's heads x splits
        n->HS = p.heads * dkv_splits; n->HO = p.kv_heads;
        continue;
      }
      n->B = p.batch * p.heads; n->HS = dkv_splits; n->HO = 1;
      n->dx.sb = n->dx.sh;        // flat (batch * head) index: stride0 == heads * stride1 (checked above)
      n->dx.sh = 0;
    }
  }
  if (dq_slab && dk_slab && dv_slab) {      // causal problems on small grids (dQ and dK/dV both split), split dQ with single-headed K/V: one launch
    if (int rc = timed("finalize", "finalize dq+dk+dv", s, [&] { return fcsa::launch_l2norm_bwd_triple(p.dtype, nq, nk, nv, s); })) return rc;
  } else if (dq_slab && dk_slab) {          // l2norm groups that are not 8 * 2^k features wide
    if (int rc = timed("finalize", "finalize dq+dk", s, [&] { return fcsa::launch_l2norm_bwd_pair(p.dtype, nq, nk, s); })) return rc;
  } else {
    if (dq_slab) {
      if (int rc = timed("finalize", "finalize dq", s, [&] { return fcsa::launch_l2norm_bwd(p.dtype, nq, s); })) return rc;
    }
    if (dk_slab && dv_slab) {      // single-headed K/V, split-query dK/dV: both reductions in one launch
      if (int rc = timed("finalize", "finalize dk+dv", s, [&] { return fcsa::launch_l2norm_bwd_pair(p.dtype, nk, nv, s); })) return rc;
    } else if (dk_slab) {
      if (int rc = timed("finalize", "finalize dk", s, [&] { return fcsa::launch_l2norm_bwd(p.dtype, nk, s); })) return rc;
    } else if (dv_slab) {
      if (int rc = timed("finalize", "finalize dv", s, [&] { return fcsa::launch_l2norm_bwd(p.dtype, nv, s); })) return rc;
    }
  }
  // Two degenerate problems whose dq and dk are EXACTLY zero, and for which the kernels' arithmetic is not meaningful:
  //   scale == 0: the logits do not depend on q, k.  The kernels carry c1 = scale * log2(e) folded into the saved q^ and undo it with
  //     1 / c1 in the l2norm backward and the dK^ epilogue: 0 * inf = NaN.
  //   l2norm groups of ONE feature (groups == dim_head): x^ = sign(x), whose derivative is zero; the tangent-space projection
  //     r (g - x^ <g, x^>) is then a pure cancellation that the 16-bit rounding of c1 * q^ leaves at 2^-11 |g| / |x| -- unbounded for
  //     elements near zero (measured 0.7 against an exact 0).
  // The reference's autograd through F.normalize / scale * sim gives zeros in both; dv (and d_bias) are what the kernels wrote.
  if (p.scale == 0.f || (p.l2norm_qk && p.groups == p.dim_head)) {
    if (int rc = zero_rows("dq", a->dq, es, p.batch, p.heads, p.q_len, p.dim_head, s)) return rc;
    if (int rc = zero_rows("dk", a->dk, es, p.batch, p.kv_heads, p.k_len, p.dim_head, s)) return rc;
  }
  return FCSA_OK;
}

}  // namespace

extern "C" {

const char* fcsa_last_error(void) { return g_err.c_str(); }

int fcsa_profile_enable(int32_t enable) {
  g_prof_on.store(enable != 0, std::memory_order_relaxed);
  return FCSA_OK;
}

int fcsa_profile_collect(fcsa_kernel_stat* stats, int32_t capacity) {
  std::vector<TimedLaunch> rec;
  { std::lock_guard<std::mutex> g(g_prof_mu); rec.swap(g_prof); }
  std::vector<fcsa_kernel_stat> agg;
  for (TimedLaunch& t : rec) {
    float ms = 0.f;
    const bool ok = hipEventSynchronize(t.stop) == hipSuccess && hipEventElapsedTime(&ms, t.start, t.stop) == hipSuccess;
    (void)hipEventDestroy(t.start);
    (void)hipEventDestroy(t.stop);
    if (!ok) continue;
    fcsa_kernel_stat* st = nullptr;
    for (auto& a : agg) if (strcmp(a.name, t.name) == 0) st = &a;
    if (st == nullptr) {
      fcsa_kernel_stat n;
      memset(&n, 0, sizeof(n));
      strncpy(n.name, t.name, sizeof(n.name) - 1);
      n.min_ms = ms; n.max_ms = ms;
      agg.push_back(n);
      st = &agg.back();
    }
    st->calls += 1;
    st->total_ms += ms;
    if (ms < st->min_ms) st->min_ms = ms;
    if (ms > st->max_ms) st->max_ms = ms;
  }
  if (stats != nullptr)
    for (int i = 0; i < (int)agg.size() && i < capacity; ++i) stats[i] = agg[i];
  return (int)agg.size();
}

int fcsa_debug(char* buf, size_t buf_bytes) {
  if (buf != nullptr && buf_bytes > 0) {
    snprintf(buf, buf_bytes,
             "libfcsa_hip abi=%d arch=gfx950 dtypes=f32,f16,bf16 dim_head=16,32,64,96,128 "
             "kernels=l2norm,l2norm_pair,fwd(32 rows/wave; lean two-wave form at D=96/128),fwd2(64 rows/wave),fwd3(D=128: 64 rows/wave, 1 wave/SIMD),fwd_ksplit(128 rows, wave halves split the keys),fwd_split+combine,"
             "fwd_dyn(per-row shift),bwd_dq(+split-key; key-split form on 8 waves),bwd_dkv(+lean; query-split form on 8 waves; grouped-query K/V head sweep),bwd_dbias,finalize,kv_append+decode+decode_combine(kv cache),"
             "window(fwd_win,bwd_dq_win,bwd_dkv_win,decode_win: sliding-window forms),"
             "kv_append_fp8+decode_fp8+decode_combine_fp8(e4m3fn kv cache, f16/bf16 queries),"
             "kv_append_ragged+decode_ragged+decode_combine_ragged(+_fp8: packed queries with per-sequence counts against the kv cache),"
             "decode_tree(+_fp8: a per-row bit set over the step's tokens, tree attention for speculative decoding)+kv_compact(the accepted path to the front of its slots) kv_heads=divisors of heads",
             FCSA_ABI_VERSION);
  }
  return FCSA_ABI_VERSION;
}

int fcsa_debug_forward_form(int32_t form) { return fcsa::forward_wide128_mode(form); }

int fcsa_debug_kv_group_form(int32_t form) { return fcsa::kv_group_mode(form); }

int fcsa_l2norm(int32_t dtype, int32_t batch, int32_t heads, int32_t len, int32_t dim_head, int32_t groups,
                const fcsa_tensor* x, void* xn, float* inv_norm, void* stream) {
  if (dtype != FCSA_F16 && dtype != FCSA_BF16 && dtype != FCSA_F32) return fail(FCSA_ERR_UNSUPPORTED, "fcsa_l2norm: dtype %d not supported", dtype);
  if (batch < 0 || heads < 0 || len < 0) return fail(FCSA_ERR_INVALID_ARG, "fcsa_l2norm: negative size (B=%d H=%d L=%d)", batch, heads, len);
  if (batch == 0 || heads == 0 || len == 0) return FCSA_OK;      // no row: nothing to launch (empty tensors carry NULL pointers)
  if (x == nullptr || xn == nullptr) return fail(FCSA_ERR_INVALID_ARG, "fcsa_l2norm: null argument");
  if (dim_head <= 0 || dim_head % 8 != 0) return fail(FCSA_ERR_UNSUPPORTED, "fcsa_l2norm: dim_head %d must be a multiple of 8", dim_head);
  if (dim_head > 512) return fail(FCSA_ERR_UNSUPPORTED, "fcsa_l2norm: dim_head %d > 512", dim_head);
  if (groups < 1 || dim_head % groups != 0) return fail(FCSA_ERR_INVALID_ARG, "fcsa_l2norm: groups (%d) must divide dim_head (%d)", groups, dim_head);
  const int es = elem_size(dtype);
  if (int rc = check_tensor("x", *x, es, true)) return rc;
  fcsa::NormParams np;
  np.x = view(*x, es);
  np.xn = static_cast<char*>(xn);
  np.inv_norm = inv_norm;
  np.B = batch; np.H = heads; np.L = len; np.D = dim_head; np.G = groups;
  np.eps = 1e-12f;                                        // F.normalize default (flash_cosine_sim_attention.py:46)
  np.out_scale = 1.f;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return timed("l2norm", "l2norm", s, [&] { return fcsa::launch_l2norm(dtype, np, s); });
}

size_t fcsa_forward_workspace_bytes(const fcsa_problem* p) { return p == nullptr ? 0 : forward_ws_bytes(*p, forward_splits(*p)); }

int fcsa_forward_needs_qn(const fcsa_problem* p, int32_t need_backward) {
  if (p == nullptr || !p->l2norm_qk) return 0;
  if (need_backward) return 1;
  return (p->dtype != FCSA_F32 && fusable_groups(*p)) ? 0 : 1;
}

// ---- the training calls: each entry point is its description, handed to train_forward / train_backward
int fcsa_forward(const fcsa_forward_args* a) { return train_forward({TrainNeeds::Nothing, a, nullptr, nullptr, nullptr}); }
int fcsa_forward_varlen(const fcsa_forward_args* a, const fcsa_varlen* seqs) { return train_forward({TrainNeeds::Seqs, a, nullptr, seqs, nullptr}); }
int fcsa_forward_window(const fcsa_forward_args* a, const fcsa_varlen* seqs, const fcsa_window* w) {
  return train_forward({TrainNeeds::Window, a, nullptr, seqs, w});
}
int fcsa_forward_alibi(const fcsa_forward_args* a, const fcsa_varlen* seqs, const fcsa_window* w, const fcsa_alibi* al) {
  return train_forward({TrainNeeds::Slopes, a, nullptr, seqs, w, al});
}
size_t fcsa_forward_alibi_workspace_bytes(const fcsa_problem*, const fcsa_varlen*, const fcsa_window*) { return 0; }

int fcsa_backward(const fcsa_backward_args* a) { return train_backward({TrainNeeds::Nothing, nullptr, a, nullptr, nullptr}); }
int fcsa_backward_varlen(const fcsa_backward_args* a, const fcsa_varlen* seqs) { return train_backward({TrainNeeds::Seqs, nullptr, a, seqs, nullptr}); }
int fcsa_backward_window(const fcsa_backward_args* a, const fcsa_varlen* seqs, const fcsa_window* w) {
  return train_backward({TrainNeeds::Window, nullptr, a, seqs, w});
}
int fcsa_backward_alibi(const fcsa_backward_args* a, const fcsa_varlen* seqs, const fcsa_window* w, const fcsa_alibi* al) {
  return train_backward({TrainNeeds::Slopes, nullptr, a, seqs, w, al});
}
// attention states: every option is optional, and the call looks at what it cannot take before anything else
int fcsa_backward_state(const fcsa_backward_args* a, const fcsa_varlen* seqs, const fcsa_window* w, const float* d_lse) {
  if (a == nullptr) return fail(FCSA_ERR_INVALID_ARG, "backward_state: null args");
  if (a->mask != nullptr || a->attn_bias != nullptr || a->d_bias != nullptr)
    return fail(FCSA_ERR_INVALID_ARG, "backward_state: mask, attn_bias and d_bias are not supported with attention states (the log-sum-exp)");
  return train_backward({TrainNeeds::Nothing, nullptr, a, seqs, w, nullptr, d_lse});
}

size_t fcsa_backward_workspace_bytes(const fcsa_problem* p) { return p == nullptr ? 0 : bwd_workspace(*p, nullptr, nullptr, false); }
size_t fcsa_backward_varlen_workspace_bytes(const fcsa_problem* p, const fcsa_varlen* seqs) {
  return p == nullptr || seqs == nullptr ? 0 : bwd_workspace(*p, seqs, nullptr, false);
}
size_t fcsa_backward_window_workspace_bytes(const fcsa_problem* p, const fcsa_varlen* seqs, const fcsa_window* w) {
  return p == nullptr || w == nullptr ? 0 : bwd_workspace(*p, seqs, w, false);
}
size_t fcsa_backward_alibi_workspace_bytes(const fcsa_problem* p, const fcsa_varlen* seqs, const fcsa_window*) {
  return p == nullptr ? 0 : bwd_workspace(*p, seqs, nullptr, true);
}
}  // extern "C"

namespace {

// ---- decoding against a key/value cache (fcsa_forward_kvcache and its _window, _quant, _varlen and _lse forms) ------------------------
// One description of a decode call, one plan and one implementation (decode_call) behind the five entry points: what an entry point adds
// to the plain call is an optional part of the description.
struct DecodeCall {
  const fcsa_forward_args* a;
  const fcsa_kvcache* kv;
  const fcsa_varlen* seqs;            // a ragged step (fcsa_forward_kvcache_varlen): packed queries with per-sequence counts, or NULL
  const fcsa_kvcache_quant* qz;       // an fp8 cache (fcsa_forward_kvcache_quant), or NULL
  const fcsa_window* w;               // a sliding window as the caller gave it, or NULL
  const fcsa_lse_out* lse;            // where the combine also writes the rows' log-sum-exp (fcsa_forward_kvcache_lse), or NULL
  const fcsa_kvcache_step* step = nullptr;      // an engine step (fcsa_forward_kvcache_step): the routing of a ragged step, or NULL
  const fcsa_tree_mask* tree = nullptr;         // a tree step (fcsa_forward_kvcache_tree): the visibility words of a ragged step, or NULL
  const fcsa_alibi* alibi = nullptr;            // a linear position bias (fcsa_forward_kvcache_alibi) on a ragged or engine step, or NULL
};

// The window of a decode call as the kernels take it.  A rectangular call is normalised (fcsa::win_normalise): a window that hides nothing
// is fcsa_forward_kvcache itself (windowed == 0) with `causal` saying which of its two forms.  A ragged step does no collapsing (every
// sequence has its own N_b and L_b): its one entry point per cache type always gets sides, open ones (kWinOpen; causal: hi = 0) for a call
// without a window.
struct DecodeWindow {
  int windowed, lo, hi, causal;
  int reach() const { return windowed ? lo : fcsa::kWinOpen; }      // the left side the split rule counts keys with
};
DecodeWindow decode_window(const fcsa_problem& p, const fcsa_kvcache& kv, bool ragged, const fcsa_window* w) {
  if (ragged) {
    const int lo = w == nullptr || w->left < 0 ? fcsa::kWinOpen : std::min(w->left, fcsa::kWinOpen);
    const int hi = p.causal ? 0 : (w == nullptr || w->right < 0 ? fcsa::kWinOpen : std::min(w->right, fcsa::kWinOpen));
    return {1, lo, hi, p.causal};
  }
  if (w == nullptr) return {0, 0, 0, p.causal};
  int lo, hi;
  const int max_k = std::min(std::max(p.k_len, 0), std::max(kv.capacity, 0));
  const fcsa::WinKind kind = fcsa::win_normalise(p.q_len, max_k, p.causal != 0, w->left, w->right, lo, hi);
  if (kind == fcsa::WinKind::Window) return {1, lo, hi, p.causal};
  return {0, 0, 0, kind == fcsa::WinKind::Causal ? 1 : 0};
}

// The plan of a decode call: the row tiles of a K/V head -- rectangular: row_tiles per sequence over its G x N rows; ragged: fcsa::ragged_slots
// flat slots over all sequences (sized from total_q, never from batch x max_seqlen_q) -- the split count of the key range over them
// (fcsa::decode_splits) and the workspace: f32 partial P~V, then (row max, row sum), of every split of every row.  A pure function of the
// shapes and the CU count, never of device table contents.  win_lo: DecodeWindow::reach().
// decode_rows (an engine step): an upper bound on the packed rows the decode kernel is given, which sizes the split count in place of
// total_q (< 0: total_q, the ragged call's plan); the slots and the workspace rows stay those of the full table.
struct DecodePlan { int row_tiles; int64_t slots; int splits; size_t ws_ml, total; };
DecodePlan decode_plan(const fcsa_problem& p, const fcsa_kvcache& kv, const fcsa_varlen* seqs, int win_lo, int64_t decode_rows = -1) {
  DecodePlan d;
  const int G = p.kv_heads > 0 ? p.heads / p.kv_heads : 0;
  const int max_k = fcsa::win_decode_keys(std::min(std::max(p.k_len, 0), std::max(kv.capacity, 0)), std::max(p.q_len, 0), win_lo);
  size_t rows;
  if (seqs != nullptr) {
    const int64_t total_q = std::max<int64_t>(seqs->total_q, 0);
    d.row_tiles = 0;
    d.slots = fcsa::ragged_slots(total_q, std::max(p.batch, 0), G);
    const int64_t split_slots = decode_rows < 0 ? d.slots : fcsa::ragged_slots(std::min(decode_rows, total_q), std::max(p.batch, 0), G);
    d.splits = fcsa::decode_splits(1, p.kv_heads, (int)std::min<int64_t>(split_slots, INT32_MAX), max_k, p.dim_head, fcsa::cu_count());
    rows = (size_t)total_q * std::max(p.heads, 0);
  } else {
    d.row_tiles = std::max(fcsa::decode_row_tiles(G * p.q_len), 1);
    d.slots = 0;
    d.splits = fcsa::decode_splits(p.batch, p.kv_heads, d.row_tiles, max_k, p.dim_head, fcsa::cu_count());
    rows = (size_t)std::max(p.batch, 0) * std::max(p.heads, 0) * std::max(p.q_len, 0);
  }
  d.ws_ml = align_up(rows * d.splits * std::max(p.dim_head, 0) * 4, 256);
  d.total = rows == 0 ? 0 : d.ws_ml + align_up(rows * d.splits * 8, 256);
  return d;
}
size_t decode_workspace_bytes(const fcsa_problem* p, const fcsa_kvcache* kv, const fcsa_varlen* seqs, const fcsa_window* w) {
  if (p == nullptr || kv == nullptr) return 0;
  return decode_plan(*p, *kv, seqs, decode_window(*p, *kv, seqs != nullptr, w).reach()).total;
}

// the paged-table fields of a cache (capacity already known to be >= 0), for every call that takes one; who: the message prefix
int check_cache_table(const char* who, const fcsa_kvcache& kv) {
  if (kv.block_table == nullptr)
    return kv.page_size == 0 ? FCSA_OK : fail(FCSA_ERR_INVALID_ARG, "%s: page_size %d without a block_table", who, kv.page_size);
  if (kv.page_size <= 0 || kv.page_size % 16 != 0) return fail(FCSA_ERR_INVALID_ARG, "%s: page_size %d must be a positive multiple of 16", who, kv.page_size);
  if (kv.capacity % kv.page_size != 0) return fail(FCSA_ERR_INVALID_ARG, "%s: capacity %d is not a whole number of pages of %d", who, kv.capacity, kv.page_size);
  if (kv.capacity > 0 && kv.num_blocks < 1) return fail(FCSA_ERR_INVALID_ARG, "%s: paged cache without blocks", who);
  if (kv.block_table_stride < kv.capacity / kv.page_size)
    return fail(FCSA_ERR_INVALID_ARG, "%s: block_table row stride %lld below %d entries", who, (long long)kv.block_table_stride, kv.capacity / kv.page_size);
  return FCSA_OK;
}

// cache_es: bytes of a cache element (0: the problem's type; 1: an fp8 cache, fcsa_forward_kvcache_quant)
int check_kvcache(const fcsa_forward_args* a, const fcsa_kvcache* kv, int cache_es = 0) {
  if (a == nullptr || kv == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache: null argument");
  const fcsa_problem& p = a->p;
  if (int rc = check_problem(p)) return rc;
  if (a->inv_l != nullptr || a->mask != nullptr || a->attn_bias != nullptr)
    return fail(FCSA_ERR_INVALID_ARG, "kvcache: inv_l, mask and attn_bias must be NULL (forward only, no mask or bias)");
  if (kv->capacity < 0 || kv->new_len < 0) return fail(FCSA_ERR_INVALID_ARG, "kvcache: negative capacity (%d) or new_len (%d)", kv->capacity, kv->new_len);
  if (int rc = check_cache_table("kvcache", *kv)) return rc;
  const int es = elem_size(p.dtype);
  const bool rows = p.batch > 0 && p.heads > 0 && p.q_len > 0;
  const bool cache = p.batch > 0 && kv->capacity > 0;
  const int ces = cache_es > 0 ? cache_es : es;
  if (rows) {
    if (int rc = check_tensor("q", a->q, es, true)) return rc;
    if (int rc = check_tensor("o", a->o, es, true)) return rc;
  }
  if (cache) {
    if (int rc = check_tensor("k_cache", kv->k_cache, ces, true)) return rc;
    if (int rc = check_tensor("v_cache", kv->v_cache, ces, true)) return rc;
  }
  if (cache && kv->new_len > 0) {
    if (int rc = check_tensor("k_new", kv->k_new, es, true)) return rc;
    if (int rc = check_tensor("v_new", kv->v_new, es, true)) return rc;
  }
  if (rows) {
    const DecodePlan d = decode_plan(p, *kv, nullptr, fcsa::kWinOpen);
    if ((int64_t)p.batch * p.kv_heads * d.row_tiles * d.splits > INT32_MAX) return fail(FCSA_ERR_UNSUPPORTED, "kvcache: grid above 2^31 workgroups");
  }
  return FCSA_OK;
}

// an fp8 cache: what is checked before anything else, then the cache checks with one-byte elements
int check_quant(const fcsa_forward_args* a, const fcsa_kvcache* kv, const fcsa_kvcache_quant* qz) {
  if (a == nullptr || kv == nullptr || qz == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_quant: null argument");
  if (qz->cache_dtype != FCSA_CACHE_E4M3)
    return fail(FCSA_ERR_UNSUPPORTED, "kvcache_quant: cache type %d not supported (expected FCSA_CACHE_E4M3 = %d, OCP e4m3fn)", qz->cache_dtype, FCSA_CACHE_E4M3);
  if (a->p.dtype == FCSA_F32) return fail(FCSA_ERR_UNSUPPORTED, "kvcache_quant: float32 queries with an fp8 cache are not supported (f16 or bf16)");
  if (qz->k_scale == nullptr || qz->v_scale == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_quant: null k_scale / v_scale");
  return check_kvcache(a, kv, 1);
}

// a ragged step: its own arguments, then the equal-N checks on the problem of the packed rows
int check_kvcache_varlen(const DecodeCall& c) {
  const fcsa_forward_args* a = c.a;
  const fcsa_kvcache* kv = c.kv;
  const fcsa_varlen* seqs = c.seqs;
  if (a == nullptr || kv == nullptr || seqs == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_varlen: null argument");
  if (seqs->total_q < 0 || seqs->total_q > INT32_MAX) return fail(FCSA_ERR_INVALID_ARG, "kvcache_varlen: total_q (%lld) outside [0, 2^31)", (long long)seqs->total_q);
  if (a->p.batch > 0 && seqs->cu_seqlens_q == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_varlen: null cu_seqlens_q");
  if (kv->new_len != 0 && kv->new_len != 1) return fail(FCSA_ERR_INVALID_ARG, "kvcache_varlen: new_len (%d) is a flag here: 0 (no append) or 1 (every query row brings its key and value)", kv->new_len);
  if (c.w != nullptr)
    if (int rc = check_window(c.w, false, false)) return rc;
  // the equal-N checks, on the problem of the packed rows (q_len = total_q: which tensors must be there) with packed views
  fcsa_forward_args pa = *a;
  fcsa_kvcache pk = *kv;
  pa.q = packed(pa.q); pa.o = packed(pa.o);
  pk.k_new = packed(pk.k_new); pk.v_new = packed(pk.v_new);
  pa.p.q_len = (int32_t)seqs->total_q;
  pa.p.batch = std::min(a->p.batch, 1);
  pk.new_len = kv->new_len != 0 && seqs->total_q > 0 ? 1 : 0;
  if (a->p.q_len < 0) return fail(FCSA_ERR_INVALID_ARG, "kvcache_varlen: negative max_seqlen_q (%d)", a->p.q_len);
  if ((int64_t)std::max(a->p.heads, 0) * seqs->total_q > INT32_MAX) return fail(FCSA_ERR_UNSUPPORTED, "kvcache_varlen: heads x packed rows above 2^31");
  return c.qz != nullptr ? check_quant(&pa, &pk, c.qz) : check_kvcache(&pa, &pk);
}

// the fcsa_profile_* name and the launch-error label of each launch, by [ragged][fp8] (and [lse] for the combine)
struct LaunchName { const char* name; const char* what; };
constexpr LaunchName kAppendName[2][2] = {{{"kv_append", "kv append"}, {"kv_append_fp8", "kv append (fp8)"}},
                                          {{"kv_append_ragged", "kv append (ragged)"}, {"kv_append_ragged_fp8", "kv append (ragged)"}}};
constexpr LaunchName kDecodeName[2][2] = {{{"decode", "decode"}, {"decode_fp8", "decode (fp8)"}},
                                          {{"decode_ragged", "decode (ragged)"}, {"decode_ragged_fp8", "decode (ragged)"}}};
constexpr LaunchName kCombineName[2][2][2] = {
    {{{"decode_combine", "decode combine"}, {"decode_combine_lse", "decode combine (lse)"}},
     {{"decode_combine_fp8", "decode combine (fp8)"}, {"decode_combine_lse_fp8", "decode combine (lse, fp8)"}}},
    {{{"decode_combine_ragged", "decode combine (ragged)"}, {"decode_combine_lse_ragged", "decode combine (lse, ragged)"}},
     {{"decode_combine_ragged_fp8", "decode combine (ragged)"}, {"decode_combine_lse_ragged_fp8", "decode combine (lse, ragged)"}}}};

// One fill of the most derived block: every kernel gets the part it takes (fcsa_kernels.h).  A ragged step has packed q / o / k_new /
// v_new views, per-sequence row counts in place of N / row_tiles / new_len, and an lse view without a batch stride.  chunk_rows stays 0:
// the routing threshold is the engine step's to set.
fcsa::DecodeStepParams decode_params(const DecodeCall& c, const DecodeWindow& win, const DecodePlan& d) {
  const bool ragged = c.seqs != nullptr, fp8 = c.qz != nullptr;
  const fcsa_forward_args* a = c.a;
  const fcsa_kvcache* kv = c.kv;
  const fcsa_problem& p = a->p;
  const int es = elem_size(p.dtype), ces = fp8 ? 1 : es;
  auto rows_view = [&](const fcsa_tensor& t) { return view(ragged ? packed(t) : t, es); };
  fcsa::DecodeStepParams dp{};
  dp.q = rows_view(a->q);
  dp.o = rows_view(a->o);
  dp.kc = view(kv->k_cache, ces);
  dp.vc = view(kv->v_cache, ces);
  dp.kn = rows_view(kv->k_new);
  dp.vn = rows_view(kv->v_new);
  dp.seqlens = kv->cache_seqlens;
  dp.table = kv->block_table;
  dp.table_stride = kv->block_table_stride;
  dp.capacity = kv->capacity;
  dp.page = kv->block_table != nullptr ? kv->page_size : 0;
  dp.num_blocks = kv->num_blocks;
  dp.new_len = ragged ? 0 : kv->new_len;
  dp.B = p.batch; dp.H = p.heads; dp.Hk = p.kv_heads; dp.G = p.heads / p.kv_heads; dp.N = ragged ? 0 : p.q_len;
  dp.row_tiles = d.row_tiles; dp.splits = d.splits;
  dp.causal = win.causal; dp.l2norm = p.l2norm_qk; dp.groups = p.l2norm_qk ? p.groups : 1;
  dp.c1 = p.scale * kLog2e;
  dp.c2 = exponent_shift(p, false) * kLog2e;
  dp.l_eps = rowsum_eps(p, false);
  dp.dyn = dynamic_shift(p, false) ? 1 : 0;
  dp.ws_o = static_cast<float*>(a->workspace);
  dp.ws_ml = a->workspace != nullptr ? reinterpret_cast<float*>(static_cast<char*>(a->workspace) + d.ws_ml) : nullptr;
  dp.window = win.windowed; dp.win_lo = win.lo; dp.win_hi = win.hi;
  if (fp8) {
    dp.k_scale = c.qz->k_scale; dp.v_scale = c.qz->v_scale;
    dp.ks_b = c.qz->k_scale_stride0; dp.ks_h = c.qz->k_scale_stride1;
    dp.vs_b = c.qz->v_scale_stride0; dp.vs_h = c.qz->v_scale_stride1;
  }
  if (ragged) {
    dp.cu_q = c.seqs->cu_seqlens_q;
    dp.total_q = (int)c.seqs->total_q;
    dp.slots = (int)d.slots;
    dp.append = kv->new_len != 0 ? 1 : 0;
  }
  if (c.alibi != nullptr) {
    // device slopes of any sign cannot be bounded here: always the per-row-shift regime, as a dense call with a bias it cannot bound
    dp.c2 = 0.f;
    dp.l_eps = 1e-30f;
    dp.dyn = 1;
  }
  return dp;
}

// ---- what the three call functions below (decode_call, prefill_call, step_call) do in the same words ---------------------------------
// the rows' log-sum-exp as the kernels take it; packed: [tok, h] rows, no batch stride
fcsa::DecodeLseOut lse_view(const fcsa_lse_out& l, bool packed = false) { return {l.lse, packed ? 0 : l.stride0, l.stride1, l.stride2}; }

// where the chunk kernel (fcsa_prefill.hip) and the step kernels exist: the 16-bit types at dim_head 64 / 128
bool has_chunk_kernel(const fcsa_problem& p) { return p.dtype != FCSA_F32 && (p.dim_head == 64 || p.dim_head == 128); }

// the workspace of the split partials: d.total bytes, 256-byte aligned
int check_workspace(const char* who, const fcsa_forward_args& a, const DecodePlan& d) {
  if (a.workspace == nullptr || a.workspace_bytes < d.total)
    return fail(FCSA_ERR_WORKSPACE, "%s: workspace too small: %zu < %zu bytes", who, a.workspace_bytes, d.total);
  if ((reinterpret_cast<uintptr_t>(a.workspace) & 255) != 0) return fail(FCSA_ERR_WORKSPACE, "%s: workspace not 256-byte aligned", who);
  return FCSA_OK;
}

// the append (before anything reads the cache: same stream), where the call brings rows and the cache has room for any
int append_launch(const DecodeCall& c, fcsa::DecodeForm form, const fcsa::DecodeStepParams& dp, hipStream_t s) {
  if (c.kv->new_len <= 0 || c.kv->capacity <= 0) return FCSA_OK;
  const LaunchName& n = kAppendName[form.ragged][form.fp8];
  return timed(n.name, n.what, s, [&] { return fcsa::launch_kv_append(c.a->p.dtype, c.a->p.dim_head, form, dp, s); });
}

// c.alibi (a linear position bias): the slopes as the kernels take them, and the names of the launches that apply them
fcsa::DecodeAlibi alibi_view(const fcsa_alibi& al) { return {al.slopes, al.stride_b, al.stride_h}; }
constexpr LaunchName kAlibiDecodeName[2] = {{"alibi_decode", "decode (alibi)"}, {"alibi_decode_fp8", "decode (alibi, fp8)"}};
constexpr LaunchName kAlibiPrefillName[2] = {{"alibi_prefill", "prefill (alibi)"}, {"alibi_prefill_fp8", "prefill (alibi, fp8)"}};

// the decode launch of a ragged or engine step under the name `plain`; c.alibi: the entry points that take the slopes, under their own name
int decode_launch(const LaunchName& plain, const DecodeCall& c, fcsa::DecodeForm form, const fcsa::DecodeStepParams& dp, hipStream_t s) {
  const fcsa_problem& p = c.a->p;
  if (c.alibi == nullptr) return timed(plain.name, plain.what, s, [&] { return fcsa::launch_decode(p.dtype, p.dim_head, form, dp, s); });
  const LaunchName& n = kAlibiDecodeName[form.fp8];
  const fcsa::DecodeAlibi al = alibi_view(*c.alibi);
  return timed(n.name, n.what, s, [&] { return fcsa::launch_decode_alibi(p.dtype, p.dim_head, form, dp, al, s); });
}

// the chunk launch under the name `plain`: the call's block with 128-row slots, one split and no workspace; c.alibi: as in decode_launch
int chunk_launch(const LaunchName& plain, const DecodeCall& c, fcsa::DecodeForm form, fcsa::DecodeStepParams dp, int64_t slots, hipStream_t s) {
  dp.slots = (int)slots;
  dp.splits = 1;
  dp.ws_o = nullptr;
  dp.ws_ml = nullptr;
  const fcsa::DecodeLseOut lo = c.lse != nullptr ? lse_view(*c.lse, true) : fcsa::DecodeLseOut{};
  const fcsa::DecodeLseOut* lse = c.lse != nullptr ? &lo : nullptr;
  if (c.alibi == nullptr)
    return timed(plain.name, plain.what, s, [&] { return fcsa::launch_prefill(c.a->p.dtype, c.a->p.dim_head, form, dp, lse, s); });
  const LaunchName& n = kAlibiPrefillName[form.fp8];
  const fcsa::DecodeAlibi al = alibi_view(*c.alibi);
  return timed(n.name, n.what, s, [&] { return fcsa::launch_prefill_alibi(c.a->p.dtype, c.a->p.dim_head, form, dp, al, lse, s); });
}

// c.tree (a tree step): the ragged call without a window and without `causal` -- its checks, plan, workspace, append and combine -- with the
// decode launch on the entry points that read the visibility words.
constexpr LaunchName kTreeName[2] = {{"decode_tree", "decode (tree)"}, {"decode_tree_fp8", "decode (tree)"}};
int decode_call(const DecodeCall& c) {
  const bool ragged = c.seqs != nullptr, fp8 = c.qz != nullptr;
  // the checks, once; a rectangular call's window comes after its cache checks, a ragged step's among its own arguments
  if (ragged) {
    if (int rc = check_kvcache_varlen(c)) return rc;
  } else {
    if (int rc = fp8 ? check_quant(c.a, c.kv, c.qz) : check_kvcache(c.a, c.kv)) return rc;
    if (c.w != nullptr)
      if (int rc = check_window(c.w, false, false)) return rc;
  }
  const fcsa_forward_args* a = c.a;
  const fcsa_kvcache* kv = c.kv;
  const fcsa_problem& p = a->p;
  const DecodeWindow win = decode_window(p, *kv, ragged, c.w);
  const DecodePlan d = decode_plan(p, *kv, c.seqs, win.reach());
  if (ragged && d.slots * std::max(p.kv_heads, 1) * d.splits > INT32_MAX) return fail(FCSA_ERR_UNSUPPORTED, "kvcache_varlen: grid above 2^31 workgroups");
  if (p.batch == 0) return FCSA_OK;
  if (ragged && c.seqs->total_q == 0) return FCSA_OK;      // no packed row: nothing to append, nothing to write
  const bool rows = p.heads > 0 && (ragged || p.q_len > 0);
  if (rows)
    if (int rc = check_workspace(ragged ? "kvcache_varlen" : "kvcache", *a, d)) return rc;
  const fcsa::DecodeStepParams dp = decode_params(c, win, d);
  const fcsa::DecodeLseOut lo = c.lse != nullptr ? lse_view(*c.lse, ragged) : fcsa::DecodeLseOut{};
  // 1. the append, 2. the split partials, 3. their combine
  const fcsa::DecodeForm form = {fp8, ragged};
  hipStream_t s = static_cast<hipStream_t>(a->stream);
  if (int rc = append_launch(c, form, dp, s)) return rc;
  if (!rows) return FCSA_OK;
  if (c.tree != nullptr) {
    const LaunchName& n = kTreeName[fp8];
    const fcsa::DecodeTreeMask tm = {c.tree->mask};
    if (int rc = timed(n.name, n.what, s, [&] { return fcsa::launch_decode_tree(p.dtype, p.dim_head, form, dp, tm, s); })) return rc;
  } else {
    if (int rc = decode_launch(kDecodeName[ragged][fp8], c, form, dp, s)) return rc;
  }
  const LaunchName& m = kCombineName[ragged][fp8][c.lse != nullptr];
  return timed(m.name, m.what, s, [&] { return fcsa::launch_decode_combine(p.dtype, p.dim_head, form, dp, c.lse != nullptr ? &lo : nullptr, s); });
}

// A prompt chunk against the cache (fcsa_forward_kvcache_prefill): the ragged step's checks, its append with the parameter block the ragged
// call fills, then one launch of the multi-wave kernel (fcsa_prefill.hip) with 128-row slots, one split and no workspace.
int prefill_call(const DecodeCall& c) {
  if (int rc = check_kvcache_varlen(c)) return rc;
  const fcsa_problem& p = c.a->p;
  if (!has_chunk_kernel(p))
    return p.dtype == FCSA_F32
               ? fail(FCSA_ERR_UNSUPPORTED, "kvcache_prefill: float32 is not supported (f16 or bf16; fcsa_forward_kvcache_varlen takes float32)")
               : fail(FCSA_ERR_UNSUPPORTED, "kvcache_prefill: dim_head %d is not supported (64 or 128; fcsa_forward_kvcache_varlen takes the others)", p.dim_head);
  const int G = p.heads / p.kv_heads;
  const int64_t slots = fcsa::prefill_slots(c.seqs->total_q, std::max(p.batch, 0), G, fcsa::kPrefillRows);
  if (slots * p.kv_heads > INT32_MAX) return fail(FCSA_ERR_UNSUPPORTED, "kvcache_prefill: grid above 2^31 workgroups");
  if (p.batch == 0 || c.seqs->total_q == 0) return FCSA_OK;      // no packed row: nothing to append, nothing to write
  if (p.heads > 0 && c.lse != nullptr && c.lse->lse == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_prefill: lse: null pointer");
  const DecodeWindow win = decode_window(p, *c.kv, true, nullptr);
  const fcsa::DecodeStepParams dp = decode_params(c, win, decode_plan(p, *c.kv, c.seqs, win.reach()));
  const fcsa::DecodeForm form = {false, true};
  hipStream_t s = static_cast<hipStream_t>(c.a->stream);
  if (int rc = append_launch(c, form, dp, s)) return rc;
  if (p.heads <= 0) return FCSA_OK;
  return chunk_launch({"prefill", "prefill"}, c, form, dp, slots, s);
}

// An engine step (fcsa_forward_kvcache_step): the ragged step's description with the `step` part -- its checks, its window, its plan with the
// split count sized by the decode-routed rows, its append; then the step decode and combine launches over the full table and the chunk
// launch over 128-row slots, each skipped where the caller promises it has no work.  Where the chunk kernel is not compiled for the problem
// the call is decode_call.
static_assert(fcsa::kStepChunkRows == FCSA_STEP_CHUNK_ROWS, "the default threshold of include/fcsa.h");
int check_step(const fcsa_kvcache_step* st) {
  if (st == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_step: null argument");
  if ((st->no_decode != 0 && st->no_decode != 1) || (st->no_chunk != 0 && st->no_chunk != 1) || st->reserved != 0)
    return fail(FCSA_ERR_INVALID_ARG, "kvcache_step: no_decode (%d) and no_chunk (%d) are flags (0 or 1) and reserved (%d) is 0", st->no_decode,
                st->no_chunk, st->reserved);
  if (st->max_decode_tokens > INT32_MAX) return fail(FCSA_ERR_INVALID_ARG, "kvcache_step: max_decode_tokens (%lld) above 2^31", (long long)st->max_decode_tokens);
  return FCSA_OK;
}
// the decode-rows bound of the plan: nothing under no_decode, else the caller's bound or total_q
int64_t step_decode_rows(const fcsa_kvcache_step& st, const fcsa_varlen& seqs) {
  const int64_t total_q = std::max<int64_t>(seqs.total_q, 0);
  if (st.no_decode) return 0;
  return st.max_decode_tokens < 0 ? total_q : std::min<int64_t>(st.max_decode_tokens, total_q);
}
DecodePlan step_plan(const fcsa_problem& p, const fcsa_kvcache& kv, const fcsa_varlen& seqs, const fcsa_kvcache_step& st, int win_lo) {
  DecodePlan d = decode_plan(p, kv, &seqs, win_lo, step_decode_rows(st, seqs));
  if (st.no_decode) { d.splits = 1; d.ws_ml = 0; d.total = 0; }      // no decode launch: no partials
  return d;
}
constexpr LaunchName kStepDecodeName[2] = {{"step_decode", "step decode"}, {"step_decode_fp8", "step decode (fp8)"}};
constexpr LaunchName kStepCombineName[2][2] = {{{"step_combine", "step combine"}, {"step_combine_lse", "step combine (lse)"}},
                                               {{"step_combine_fp8", "step combine (fp8)"}, {"step_combine_lse_fp8", "step combine (lse, fp8)"}}};

int step_call(const DecodeCall& c) {
  if (int rc = check_kvcache_varlen(c)) return rc;
  if (int rc = check_step(c.step)) return rc;
  const fcsa_forward_args* a = c.a;
  const fcsa_kvcache* kv = c.kv;
  const fcsa_problem& p = a->p;
  const fcsa_kvcache_step& st = *c.step;
  const bool rows = p.batch > 0 && p.heads > 0 && c.seqs->total_q > 0;
  if (rows && c.lse != nullptr && c.lse->lse == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_step: lse: null pointer");
  if (!has_chunk_kernel(p)) return decode_call({c.a, c.kv, c.seqs, c.qz, c.w, c.lse, nullptr, nullptr, c.alibi});
  const bool fp8 = c.qz != nullptr;
  const DecodeWindow win = decode_window(p, *kv, true, c.w);
  const DecodePlan d = step_plan(p, *kv, *c.seqs, st, win.reach());
  const int G = p.heads / p.kv_heads;
  const int64_t chunk_slots = fcsa::prefill_slots(c.seqs->total_q, std::max(p.batch, 0), G, fcsa::kPrefillRows);
  if (d.slots * std::max(p.kv_heads, 1) * d.splits > INT32_MAX || chunk_slots * std::max(p.kv_heads, 1) > INT32_MAX)
    return fail(FCSA_ERR_UNSUPPORTED, "kvcache_step: grid above 2^31 workgroups");
  if (p.batch == 0 || c.seqs->total_q == 0) return FCSA_OK;      // no packed row: nothing to append, nothing to write
  if (rows && !st.no_decode)
    if (int rc = check_workspace("kvcache_step", *a, d)) return rc;
  fcsa::DecodeStepParams sp = decode_params(c, win, d);
  sp.chunk_rows = st.chunk_rows < 0 ? fcsa::kStepChunkRows : st.chunk_rows;
  const fcsa::DecodeLseOut lo = c.lse != nullptr ? lse_view(*c.lse, true) : fcsa::DecodeLseOut{};
  const fcsa::DecodeForm form = {fp8, true, true};
  hipStream_t s = static_cast<hipStream_t>(a->stream);
  // 1. the ragged call's append, once
  if (int rc = append_launch(c, form, sp, s)) return rc;
  if (!rows) return FCSA_OK;
  // 2. the decode-routed sequences: split partials and their combine over the slots and rows of the full table
  if (!st.no_decode) {
    if (int rc = decode_launch(kStepDecodeName[fp8], c, form, sp, s)) return rc;
    const LaunchName& m = kStepCombineName[fp8][c.lse != nullptr];
    if (int rc = timed(m.name, m.what, s, [&] { return fcsa::launch_decode_combine(p.dtype, p.dim_head, form, sp, c.lse != nullptr ? &lo : nullptr, s); }))
      return rc;
  }
  // 3. the chunk-routed sequences
  if (!st.no_chunk)
    if (int rc = chunk_launch({"step_prefill", "step prefill"}, c, form, sp, chunk_slots, s)) return rc;
  return FCSA_OK;
}

}  // namespace

extern "C" {

int fcsa_forward_kvcache_step(const fcsa_forward_args* a, const fcsa_kvcache* kv, const fcsa_varlen* seqs, const fcsa_kvcache_quant* qz,
                              const fcsa_window* w, const fcsa_kvcache_step* step, const fcsa_lse_out* lse) {
  if (a == nullptr || kv == nullptr || seqs == nullptr || step == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_step: null argument");
  return step_call({a, kv, seqs, qz, w, lse, step});
}
size_t fcsa_forward_kvcache_step_workspace_bytes(const fcsa_problem* p, const fcsa_kvcache* kv, const fcsa_varlen* seqs, const fcsa_kvcache_quant*,
                                                 const fcsa_window* w, const fcsa_kvcache_step* step) {
  if (p == nullptr || kv == nullptr || seqs == nullptr || step == nullptr) return 0;
  if (!has_chunk_kernel(*p)) return decode_workspace_bytes(p, kv, seqs, w);
  return step_plan(*p, *kv, *seqs, *step, decode_window(*p, *kv, true, w).reach()).total;
}

int fcsa_forward_kvcache(const fcsa_forward_args* a, const fcsa_kvcache* kv) { return decode_call({a, kv, nullptr, nullptr, nullptr, nullptr}); }
size_t fcsa_forward_kvcache_workspace_bytes(const fcsa_problem* p, const fcsa_kvcache* kv) { return decode_workspace_bytes(p, kv, nullptr, nullptr); }

int fcsa_forward_kvcache_window(const fcsa_forward_args* a, const fcsa_kvcache* kv, const fcsa_window* w) {
  if (w == nullptr) return check_window(w, false, false);
  return decode_call({a, kv, nullptr, nullptr, w, nullptr});
}
size_t fcsa_forward_kvcache_window_workspace_bytes(const fcsa_problem* p, const fcsa_kvcache* kv, const fcsa_window* w) {
  return w == nullptr ? 0 : decode_workspace_bytes(p, kv, nullptr, w);
}

int fcsa_forward_kvcache_quant(const fcsa_forward_args* a, const fcsa_kvcache* kv, const fcsa_kvcache_quant* qz, const fcsa_window* w) {
  if (qz == nullptr) return check_quant(a, kv, qz);
  return decode_call({a, kv, nullptr, qz, w, nullptr});
}
// (the split rule counts keys: an fp8 cache needs what the 16-bit call needs)
size_t fcsa_forward_kvcache_quant_workspace_bytes(const fcsa_problem* p, const fcsa_kvcache* kv, const fcsa_kvcache_quant* qz, const fcsa_window* w) {
  return qz == nullptr ? 0 : decode_workspace_bytes(p, kv, nullptr, w);
}

int fcsa_forward_kvcache_varlen(const fcsa_forward_args* a, const fcsa_kvcache* kv, const fcsa_varlen* seqs, const fcsa_kvcache_quant* qz,
                                const fcsa_window* w) {
  if (seqs == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_varlen: null argument");
  return decode_call({a, kv, seqs, qz, w, nullptr});
}
size_t fcsa_forward_kvcache_varlen_workspace_bytes(const fcsa_problem* p, const fcsa_kvcache* kv, const fcsa_varlen* seqs,
                                                   const fcsa_kvcache_quant*, const fcsa_window* w) {
  return seqs == nullptr ? 0 : decode_workspace_bytes(p, kv, seqs, w);
}

// ---- the decode calls with the rows' log-sum-exp (fcsa_forward_kvcache_lse), and merging attention states (fcsa_merge_states) ----------
// Each route is the corresponding entry point's call description with `lse` added: the same checks, window normalisation, plan and append /
// decode launches, so o and the caches are that entry point's bit for bit.
int fcsa_forward_kvcache_lse(const fcsa_forward_args* a, const fcsa_kvcache* kv, const fcsa_varlen* seqs, const fcsa_kvcache_quant* qz,
                             const fcsa_window* w, const fcsa_lse_out* lse) {
  if (a == nullptr || kv == nullptr || lse == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_lse: null argument");
  const bool rows = a->p.batch > 0 && a->p.heads > 0 && (seqs != nullptr ? seqs->total_q > 0 : a->p.q_len > 0);
  if (rows && lse->lse == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_lse: lse: null pointer");
  return decode_call({a, kv, seqs, qz, w, lse});
}

int fcsa_forward_kvcache_tree(const fcsa_forward_args* a, const fcsa_kvcache* kv, const fcsa_varlen* seqs, const fcsa_kvcache_quant* qz,
                              const fcsa_tree_mask* tree, const fcsa_lse_out* lse) {
  if (a == nullptr || kv == nullptr || seqs == nullptr || tree == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_tree: null argument");
  if (a->p.causal != 0) return fail(FCSA_ERR_INVALID_ARG, "kvcache_tree: causal must be 0 (the mask states the visibility)");
  if (tree->reserved != 0) return fail(FCSA_ERR_INVALID_ARG, "kvcache_tree: reserved (%lld) is 0", (long long)tree->reserved);
  const bool rows = a->p.batch > 0 && a->p.heads > 0 && seqs->total_q > 0;
  if (rows && tree->mask == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_tree: mask: null pointer");
  if ((reinterpret_cast<uintptr_t>(tree->mask) & 7) != 0) return fail(FCSA_ERR_INVALID_ARG, "kvcache_tree: mask not 8-byte aligned");
  if (rows && lse != nullptr && lse->lse == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_tree: lse: null pointer");
  return decode_call({a, kv, seqs, qz, nullptr, lse, nullptr, tree});
}

int fcsa_forward_kvcache_alibi(const fcsa_forward_args* a, const fcsa_kvcache* kv, const fcsa_varlen* seqs, const fcsa_kvcache_quant* qz,
                               const fcsa_window* w, const fcsa_kvcache_step* step, const fcsa_alibi* alibi, const fcsa_lse_out* lse) {
  if (a == nullptr || kv == nullptr || seqs == nullptr || step == nullptr || alibi == nullptr)
    return fail(FCSA_ERR_INVALID_ARG, "kvcache_alibi: null argument");
  if (alibi->slopes == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_alibi: slopes: null pointer");
  if ((reinterpret_cast<uintptr_t>(alibi->slopes) & 3) != 0) return fail(FCSA_ERR_INVALID_ARG, "kvcache_alibi: slopes not 4-byte aligned");
  if (alibi->reserved != 0) return fail(FCSA_ERR_INVALID_ARG, "kvcache_alibi: reserved (%lld) is 0", (long long)alibi->reserved);
  return step_call({a, kv, seqs, qz, w, lse, step, nullptr, alibi});
}

int fcsa_kvcache_compact(const fcsa_kvcache* kv, int32_t batch, int32_t kv_heads, int32_t dim_head, int32_t elem_bytes, const int32_t* accepted,
                         int64_t accepted_stride, int32_t max_accepted, const int32_t* num_accepted, void* stream) {
  if (kv == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_compact: null argument");
  if (batch < 0 || kv_heads < 0) return fail(FCSA_ERR_INVALID_ARG, "kvcache_compact: negative size (B=%d Hk=%d)", batch, kv_heads);
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return fail(FCSA_ERR_UNSUPPORTED, "kvcache_compact: elem_bytes %d not in {1, 2, 4}", elem_bytes);
  if (!dim_ok(dim_head)) return fail(FCSA_ERR_UNSUPPORTED, "kvcache_compact: dim_head %d not in {16, 32, 64, 96, 128}", dim_head);
  if (max_accepted < 1 || max_accepted > fcsa::kCompactSlots)
    return fail(FCSA_ERR_INVALID_ARG, "kvcache_compact: max_accepted (%d) outside [1, %d]", max_accepted, fcsa::kCompactSlots);
  if (accepted_stride < max_accepted) return fail(FCSA_ERR_INVALID_ARG, "kvcache_compact: accepted row stride %lld below %d entries", (long long)accepted_stride, max_accepted);
  if (kv->capacity < 0) return fail(FCSA_ERR_INVALID_ARG, "kvcache_compact: negative capacity (%d)", kv->capacity);
  if (int rc = check_cache_table("kvcache_compact", *kv)) return rc;
  if (batch == 0 || kv_heads == 0 || kv->capacity == 0) return FCSA_OK;      // no row to move
  if (accepted == nullptr || num_accepted == nullptr || kv->cache_seqlens == nullptr)
    return fail(FCSA_ERR_INVALID_ARG, "kvcache_compact: null accepted, num_accepted or cache_seqlens");
  if (int rc = check_tensor("k_cache", kv->k_cache, elem_bytes, true)) return rc;
  if (int rc = check_tensor("v_cache", kv->v_cache, elem_bytes, true)) return rc;
  if ((int64_t)batch * kv_heads > INT32_MAX) return fail(FCSA_ERR_UNSUPPORTED, "kvcache_compact: grid above 2^31 workgroups");
  fcsa::DecodeParams dp{};
  dp.kc = view(kv->k_cache, elem_bytes);
  dp.vc = view(kv->v_cache, elem_bytes);
  dp.seqlens = kv->cache_seqlens;
  dp.table = kv->block_table;
  dp.table_stride = kv->block_table_stride;
  dp.capacity = kv->capacity;
  dp.page = kv->block_table != nullptr ? kv->page_size : 0;
  dp.num_blocks = kv->num_blocks;
  dp.B = batch; dp.Hk = kv_heads;
  const fcsa::CompactParams cp = {accepted, num_accepted, accepted_stride, max_accepted, dim_head * elem_bytes};
  hipStream_t s = static_cast<hipStream_t>(stream);
  return timed("kv_compact", "kv compact", s, [&] { return fcsa::launch_kv_compact(dp, cp, s); });
}

int fcsa_forward_kvcache_prefill(const fcsa_forward_args* a, const fcsa_kvcache* kv, const fcsa_varlen* seqs, const fcsa_lse_out* lse) {
  if (a == nullptr || kv == nullptr || seqs == nullptr) return fail(FCSA_ERR_INVALID_ARG, "kvcache_prefill: null argument");
  return prefill_call({a, kv, seqs, nullptr, nullptr, lse});
}

int fcsa_merge_states(const fcsa_merge_args* a) {
  static_assert(FCSA_MERGE_MAX_STATES == fcsa::kMergeMaxStates && sizeof(a->o_in) / sizeof(a->o_in[0]) == FCSA_MERGE_MAX_STATES, "fcsa_merge_args");
  if (a == nullptr) return fail(FCSA_ERR_INVALID_ARG, "merge_states: null args");
  if (a->dtype != FCSA_F32 && a->dtype != FCSA_F16 && a->dtype != FCSA_BF16) return fail(FCSA_ERR_UNSUPPORTED, "merge_states: dtype %d not supported", a->dtype);
  if (a->states < 1 || a->states > FCSA_MERGE_MAX_STATES)
    return fail(FCSA_ERR_INVALID_ARG, "merge_states: %d states outside [1, %d] (merge more in two steps)", a->states, FCSA_MERGE_MAX_STATES);
  if (a->size0 < 0 || a->size1 < 0 || a->size2 < 0) return fail(FCSA_ERR_INVALID_ARG, "merge_states: negative size");
  // rows 16-byte aligned: whole 16-byte chunks per row, 4 float32 or 8 16-bit features
  const int per16 = 16 / elem_size(a->dtype);
  if (a->dim_head < per16 || a->dim_head % per16 != 0)
    return fail(FCSA_ERR_UNSUPPORTED, "merge_states: dim_head %d is not a positive multiple of %d (16-byte rows)", a->dim_head, per16);
  const int64_t rows = (int64_t)a->size0 * a->size1 * a->size2;
  if (rows == 0) return FCSA_OK;
  if (rows * (a->dim_head / 4) > (int64_t)INT32_MAX * 256) return fail(FCSA_ERR_UNSUPPORTED, "merge_states: grid above 2^31 workgroups");
  const int es = elem_size(a->dtype);
  fcsa::MergeParams mp;
  for (int s = 0; s < FCSA_MERGE_MAX_STATES; ++s) {
    const int t = std::min(s, a->states - 1);      // (the unused slots repeat the last state: never read, never null)
    if (s < a->states) {
      if (int rc = check_tensor("merge_states: o_in", a->o_in[s], es, true)) return rc;
      if (a->lse_in[s].lse == nullptr) return fail(FCSA_ERR_INVALID_ARG, "merge_states: lse_in[%d]: null pointer", s);
    }
    mp.o_in[s] = view(a->o_in[t], es);
    mp.lse_in[s] = lse_view(a->lse_in[t]);
  }
  if (int rc = check_tensor("merge_states: o", a->o, es, true)) return rc;
  if (a->lse.lse == nullptr) return fail(FCSA_ERR_INVALID_ARG, "merge_states: lse: null pointer");
  mp.o = view(a->o, es);
  mp.lse = lse_view(a->lse);
  mp.n0 = a->size0; mp.n1 = a->size1; mp.n2 = a->size2; mp.D = a->dim_head; mp.S = a->states;
  hipStream_t s = static_cast<hipStream_t>(a->stream);
  return timed("merge_states", "merge states", s, [&] { return fcsa::launch_merge_states(a->dtype, mp, s); });
}

// ---- attention states for training: the log-sum-exp of a forward call, read off its inv_l, and the merge's backward -------------------
int fcsa_attention_lse(const fcsa_problem* pp, const float* inv_l, const fcsa_varlen* seqs, const fcsa_window* w, const fcsa_lse_out* lse_out,
                       void* stream) {
  if (pp == nullptr || lse_out == nullptr) return fail(FCSA_ERR_INVALID_ARG, "attention_lse: null argument");
  const fcsa_problem& p = *pp;
  if (int rc = check_problem(p)) return rc;
  if (seqs != nullptr) {
    if (int rc = check_varlen(p, seqs, false, false)) return rc;
  }
  if (w != nullptr) {
    if (int rc = check_window(w, false, false)) return rc;
  }
  if (p.batch == 0 || p.heads == 0 || p.q_len == 0 || (seqs != nullptr && seqs->total_q == 0)) return FCSA_OK;      // no row
  if (lse_out->lse == nullptr) return fail(FCSA_ERR_INVALID_ARG, "attention_lse: lse_out: null pointer");
  if (inv_l == nullptr) return fail(FCSA_ERR_INVALID_ARG, "attention_lse: inv_l: null pointer");
  fcsa::StateLseParams sp;
  sp.inv_l = inv_l;
  sp.out = lse_view(*lse_out);
  sp.B = p.batch; sp.H = p.heads; sp.N = p.q_len; sp.M = p.k_len;
  // the sides as every windowed launch takes them: (open, open) no mask, (open, 0) causal
  (void)fcsa::win_normalise(p.q_len, p.k_len, p.causal != 0, w != nullptr ? w->left : -1, w != nullptr ? w->right : -1, sp.win_lo, sp.win_hi);
  sp.c2 = exponent_shift(p, false) * kLog2e;
  sp.invl_log2 = dynamic_shift(p, false) ? 1 : 0;
  sp.seq = seq_table(seqs);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return timed("state_lse", "state lse", s, [&] { return fcsa::launch_state_lse(sp, s); });
}

int fcsa_merge_states_backward(const fcsa_merge_backward_args* a) {
  if (a == nullptr) return fail(FCSA_ERR_INVALID_ARG, "merge_states_backward: null args");
  if (a->dtype != FCSA_F32 && a->dtype != FCSA_F16 && a->dtype != FCSA_BF16)
    return fail(FCSA_ERR_UNSUPPORTED, "merge_states_backward: dtype %d not supported", a->dtype);
  if (a->states < 1 || a->states > FCSA_MERGE_MAX_STATES)
    return fail(FCSA_ERR_INVALID_ARG, "merge_states_backward: %d states outside [1, %d]", a->states, FCSA_MERGE_MAX_STATES);
  if (a->size0 < 0 || a->size1 < 0 || a->size2 < 0) return fail(FCSA_ERR_INVALID_ARG, "merge_states_backward: negative size");
  const int per16 = 16 / elem_size(a->dtype);
  if (a->dim_head < per16 || a->dim_head % per16 != 0)
    return fail(FCSA_ERR_UNSUPPORTED, "merge_states_backward: dim_head %d is not a positive multiple of %d (16-byte rows)", a->dim_head, per16);
  const int64_t rows = (int64_t)a->size0 * a->size1 * a->size2;
  if (rows == 0) return FCSA_OK;
  if (rows / 16 > (int64_t)INT32_MAX - 1) return fail(FCSA_ERR_UNSUPPORTED, "merge_states_backward: grid above 2^31 workgroups");
  const int es = elem_size(a->dtype);
  fcsa::MergeBwdParams mp;
  for (int s = 0; s < FCSA_MERGE_MAX_STATES; ++s) {
    const int t = std::min(s, a->states - 1);      // (the unused slots repeat the last state: never read, never written, never null)
    if (s < a->states) {
      if (int rc = check_tensor("merge_states_backward: o_in", a->o_in[s], es, true)) return rc;
      if (int rc = check_tensor("merge_states_backward: d_o_in", a->d_o_in[s], es, true)) return rc;
      if (a->lse_in[s].lse == nullptr || a->d_lse_in[s].lse == nullptr)
        return fail(FCSA_ERR_INVALID_ARG, "merge_states_backward: lse_in[%d] / d_lse_in[%d]: null pointer", s, s);
    }
    mp.o_in[s] = view(a->o_in[t], es);
    mp.lse_in[s] = lse_view(a->lse_in[t]);
    mp.d_o_in[s] = view(a->d_o_in[t], es);
    mp.d_lse_in[s] = lse_view(a->d_lse_in[t]);
  }
  if (int rc = check_tensor("merge_states_backward: d_o", a->d_o, es, true)) return rc;
  mp.d_o = view(a->d_o, es);
  mp.d_lse = lse_view(a->d_lse);
  mp.n0 = a->size0; mp.n1 = a->size1; mp.n2 = a->size2; mp.D = a->dim_head; mp.S = a->states;
  hipStream_t s = static_cast<hipStream_t>(a->stream);
  return timed("merge_states_bwd", "merge states backward", s, [&] { return fcsa::launch_merge_states_backward(a->dtype, mp, s); });
}
}  // extern "C"
