// fcsa_torch.cpp -- compiled PyTorch binding of the C ABI (include/fcsa.h): the counterpart of the reference's pybind module
// (flash_cosine_sim_attention_cuda.cu:1928-1933) and of the tensor handling of its host launchers (cu:1630-1698, cu:1752-1827).
//
// Host-only C++ (no device code): shape canonicalisation, argument checks (TORCH_CHECK -> Python exceptions instead of the
// reference's compiled-out asserts), output / saved-state allocation with ATen, then ONE call into libfcsa_hip.so on the current
// HIP stream of q's device.  Registered as dispatcher ops (TORCH_LIBRARY) so that the Python wrapper is a thin
// autograd.Function over `torch.ops.fcsa.*` -- cheap per call, and traceable by torch.compile (fake kernels are registered in
// Python, flash_cosine_sim_attention_amd/_torch_ops.py).  No torch type crosses into libfcsa_hip.so: the boundary stays the C ABI.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <c10/util/accumulate.h>
#include <torch/csrc/autograd/custom_function.h>
#include <torch/library.h>

#include <dlfcn.h>

#include <atomic>
#include <cmath>
#include <cstring>
#include <chrono>
#include <tuple>
#include <type_traits>
#include <utility>

#include "../../include/fcsa.h"

namespace {

// The C ABI is called through pointers so that measurement tools can swap in another build of the same ABI at run time
// (fcsa_torch_use_library, tools/ab_libs.py: interleaved A/B of kernel variants in ONE process).  Default: the library this
// module is linked against.  Every entry point is named once, here -- X(member, exported symbol, required) -- and the members
// (typed by the declarations of include/fcsa.h), the dlsym pass and the "required" check of fcsa_torch_use_library derive from
// the list.  An optional one is null when a swapped-in library does not export it; the ops that need it then raise (need_abi).
#define FCSA_ABI(X)                                                                       \
  X(forward, fcsa_forward, true)                                                          \
  X(backward, fcsa_backward, true)                                                        \
  X(forward_ws, fcsa_forward_workspace_bytes, true)                                       \
  X(backward_ws, fcsa_backward_workspace_bytes, true)                                     \
  X(needs_qn, fcsa_forward_needs_qn, true)                                                \
  X(last_error, fcsa_last_error, true)                                                    \
  /* packed sequences */                                                                  \
  X(forward_varlen, fcsa_forward_varlen, false)                                           \
  X(backward_varlen, fcsa_backward_varlen, false)                                         \
  X(backward_varlen_ws, fcsa_backward_varlen_workspace_bytes, false)                      \
  /* decoding against a key/value cache */                                                \
  X(forward_kvcache, fcsa_forward_kvcache, false)                                         \
  X(forward_kvcache_ws, fcsa_forward_kvcache_workspace_bytes, false)                      \
  /* sliding window */                                                                    \
  X(forward_window, fcsa_forward_window, false)                                           \
  X(backward_window, fcsa_backward_window, false)                                         \
  X(backward_window_ws, fcsa_backward_window_workspace_bytes, false)                      \
  X(forward_kvcache_window, fcsa_forward_kvcache_window, false)                           \
  X(forward_kvcache_window_ws, fcsa_forward_kvcache_window_workspace_bytes, false)        \
  /* fp8 key/value cache */                                                               \
  X(forward_kvcache_quant, fcsa_forward_kvcache_quant, false)                             \
  X(forward_kvcache_quant_ws, fcsa_forward_kvcache_quant_workspace_bytes, false)          \
  /* ragged decode steps (packed queries with per-sequence counts) */                     \
  X(forward_kvcache_varlen, fcsa_forward_kvcache_varlen, false)                           \
  X(forward_kvcache_varlen_ws, fcsa_forward_kvcache_varlen_workspace_bytes, false)        \
  /* the decode calls with the rows' log-sum-exp, and merging attention states */         \
  X(forward_kvcache_lse, fcsa_forward_kvcache_lse, false)                                 \
  X(merge_states, fcsa_merge_states, false)                                               \
  /* prompt chunks against the cache (the multi-wave prefill kernel) */                   \
  X(forward_kvcache_prefill, fcsa_forward_kvcache_prefill, false)                         \
  /* attention states for training: the forward's log-sum-exp, its gradient, the merge's backward */ \
  X(attention_lse, fcsa_attention_lse, false)                                             \
  X(backward_state, fcsa_backward_state, false)                                           \
  X(merge_states_backward, fcsa_merge_states_backward, false)                             \
  /* the engine step: chunks and decodes routed in one call */                            \
  X(forward_kvcache_step, fcsa_forward_kvcache_step, false)                               \
  X(forward_kvcache_step_ws, fcsa_forward_kvcache_step_workspace_bytes, false)        \
  /* tree attention for speculative decoding, and the compaction of the accepted path */ \
  X(forward_kvcache_tree, fcsa_forward_kvcache_tree, false)                               \
  X(kvcache_compact, fcsa_kvcache_compact, false)                                         \
  /* a linear position bias (ALiBi) on the engine step */                                 \
  X(forward_kvcache_alibi, fcsa_forward_kvcache_alibi, false)                             \
  /* the same bias in the training kernels, forward and backward */                       \
  X(forward_alibi, fcsa_forward_alibi, false)                                             \
  X(backward_alibi, fcsa_backward_alibi, false)                                           \
  X(backward_alibi_ws, fcsa_backward_alibi_workspace_bytes, false)

struct Abi {
#define X(member, symbol, required) decltype(&symbol) member = &symbol;
  FCSA_ABI(X)
#undef X
} g_abi;

// an op refuses to run when the loaded library lacks an entry point it needs
void need_abi(const char* who, const char* symbols, bool present) {
  TORCH_CHECK(present, who, ": the loaded libfcsa_hip.so does not export ", symbols);
}
template <class... Fn>
void need_abi(const char* who, const char* symbols, Fn... members) { need_abi(who, symbols, ((members != nullptr) && ...)); }

using at::Tensor;
using c10::optional;

// Host-time accounting of the two dense ops (tools/host_overhead.py; small problems are bound by host time per call, not by the
// kernels): nanoseconds spent in [0] forward checks / canonicalisation, [1] forward allocations, [2] fcsa_forward (validation +
// launches), [3..5] the same for backward, [6] forward calls, [7] backward calls.  Two clock reads per section, always on for a
// dense call; the packed calls share the bodies and leave the counters alone (on == false).
std::atomic<uint64_t> g_host_ns[8];
struct Lap {
  const bool on;
  std::chrono::steady_clock::time_point t;
  explicit Lap(bool dense) : on(dense) {
    if (on) t = std::chrono::steady_clock::now();
  }
  void mark(int slot) {
    if (!on) return;
    const auto n = std::chrono::steady_clock::now();
    g_host_ns[slot].fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(n - t).count(), std::memory_order_relaxed);
    t = n;
  }
  void count(int slot) {
    if (on) g_host_ns[slot].fetch_add(1, std::memory_order_relaxed);
  }
};

int dtype_code(at::ScalarType t) {
  switch (t) {
    case at::kFloat: return FCSA_F32;
    case at::kHalf: return FCSA_F16;
    case at::kBFloat16: return FCSA_BF16;
    default: TORCH_CHECK_TYPE(false, "unsupported dtype ", t, "; expected float32, float16 or bfloat16");
  }
  return -1;
}

// rows 16-byte aligned and the feature dim contiguous: consumed in place (e.g. the `b n (h d) -> b h n d` views of
// transformer.py:100); anything else is made contiguous
bool rows_ok(const Tensor& t) {
  const int64_t m = 16 / t.element_size();
  if (t.stride(-1) != 1 || (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) != 0) return false;
  for (int64_t d = 0; d + 1 < t.dim(); ++d)
    if (t.stride(d) % m != 0) return false;
  return true;
}
Tensor prep(const Tensor& t) { return rows_ok(t) ? t : t.contiguous(); }

// Which dims of a tensor give the ABI's (stride0, stride1, stride2) = (batch, head, position) strides; a feature dim may follow them.
struct Layout {
  int batch, head, pos;      // batch < 0: no such dim (stride0 = 0, ignored by the library)
};
constexpr Layout kDense{0, 1, 2};       // [B, H, N, D], [B, H, N]
constexpr Layout kPacked{-1, 1, 0};     // packed [total, H, D], [total, H]: stride1 = head stride, stride2 = token stride
constexpr Layout kRows3{-1, 0, 1};      // merge_states, which has no heads: a 3-D state's rows as [1, size(0), size(1)]

// the strided view of `t` that the library takes: V = fcsa_tensor, or fcsa_lse_out for a float32 tensor without the feature dim
template <class V = fcsa_tensor>
V strided(const Tensor& t, Layout l = kDense) {
  V v;
  if constexpr (std::is_same_v<V, fcsa_lse_out>) v.lse = t.data_ptr<float>();
  else v.ptr = t.data_ptr();
  v.stride0 = l.batch < 0 ? 0 : t.stride(l.batch);
  v.stride1 = t.stride(l.head);
  v.stride2 = t.stride(l.pos);
  return v;
}

void check(int rc, const char* what) {
  TORCH_CHECK(rc == FCSA_OK, what, " failed (status ", rc, "): ", g_abi.last_error());
}

void* stream_of(const Tensor& t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

// ---- the dense and the packed calls ---------------------------------------------------------------------------------------------------------
// One canonicalised call, dense -- q [B, H, N, D], k / v [B, Hk, M, D] -- or packed variable-length sequences (fcsa_forward_varlen /
// fcsa_backward_varlen): q [total_q, H, D], k / v [total_k, Hk, D], cu_seqlens_* int32 [S + 1] on q's device.  The tables are passed to the
// library as they are: their contents are never read on the host (the Python wrapper validates host tables before they are moved to the
// device).  canonicalise / canonicalise_varlen build it and the op function adds the options it has; everything after them (forward_body,
// backward_body, the choice of the C function: kTrainEntries) exists once and reads the description.
struct Call {
  Tensor q, k, v;                 // rows ok
  optional<Tensor> mask, bias;    // dense only; contiguous
  Tensor cu_q, cu_k;              // packed only; contiguous
  bool merged = false;            // dense only: q came with batch and heads merged, [B * H, N, D]
  at::DimVector rows_q, rows_k;   // leading dims of the q-side / k-side saved tensors: (B, H, N) / (B, Hk, M); packed (H, total_q) / (Hk, total_k)
  int64_t D = 0, groups = 1;      // groups as the caller gave it (p.groups is 1 without l2norm_qk)
  fcsa_problem p;
  fcsa_varlen table{};            // packed only: cu_q / cu_k as the library takes them
  // what some calls have
  optional<fcsa_window> win;      // a sliding window (Win's checks passed)
  optional<fcsa_alibi> alibi;     // the slopes of a linear position bias (TrainSlopes' checks passed)
  const Tensor* d_lse = nullptr;  // backward only: the gradient of the rows' log-sum-exp (attention_state_backward)
  bool packed() const { return cu_q.defined(); }
  Layout layout() const { return packed() ? kPacked : kDense; }
  const fcsa_varlen* seqs() const { return packed() ? &table : nullptr; }
  const fcsa_window* window() const { return win ? &*win : nullptr; }
};

void set_problem(Call& c, at::ScalarType dt, int64_t batch, int64_t q_len, int64_t k_len, bool bias_batch, double scale, bool causal,
                 bool l2norm_qk, int64_t groups) {
  c.D = c.q.size(-1);
  c.groups = groups;
  c.p.dtype = dtype_code(dt);
  c.p.batch = (int32_t)batch; c.p.heads = (int32_t)c.q.size(1); c.p.kv_heads = (int32_t)c.k.size(1);
  c.p.q_len = (int32_t)q_len; c.p.k_len = (int32_t)k_len; c.p.dim_head = (int32_t)c.D;
  c.p.causal = causal; c.p.bias_batch_dim = bias_batch; c.p.l2norm_qk = l2norm_qk;
  c.p.groups = l2norm_qk ? (int32_t)groups : 1;
  c.p.scale = (float)scale;
}

Call canonicalise(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& mask, const optional<Tensor>& bias,
                  bool bias_batch, double scale, bool causal, bool l2norm_qk, int64_t groups) {
  TORCH_CHECK(q.is_cuda(), "flash_cosine_sim_attention_amd: q, k, v must be GPU tensors (HIP kernels only, no CPU fallback)");
  auto same_dev = [&](const char* name, const Tensor& t) {
    TORCH_CHECK_VALUE(t.device() == q.device(), name, " is on ", t.device(), " but q is on ", q.device(), ": all tensors must live on q's GPU");
  };
  same_dev("k", k);
  same_dev("v", v);
  if (mask.has_value()) same_dev("mask", *mask);
  if (bias.has_value()) same_dev("attn_bias", *bias);
  TORCH_CHECK_TYPE(q.scalar_type() == k.scalar_type() && q.scalar_type() == v.scalar_type(), "q, k, v must share a dtype, got ",
                   q.scalar_type(), ", ", k.scalar_type(), ", ", v.scalar_type());
  dtype_code(q.scalar_type());
  TORCH_CHECK_VALUE(!(causal && mask.has_value()), "mask should not be supplied if causality is needed");       // fcsa.py:88, cu:1675
  Call c;
  c.merged = q.dim() == 3;
  if (c.merged) {
    TORCH_CHECK_VALUE(k.dim() == 3 && v.dim() == 3, "if batch and heads are merged for queries, keys and values must also have 3 dimensions");
    bias_batch = true;                                                                                            // cu:1652
    c.q = q.unsqueeze(1);
  } else {
    TORCH_CHECK_VALUE(q.dim() == 4, "q must have 3 or 4 dimensions, got ", q.dim());
    c.q = q;
  }
  c.k = k.dim() == 3 ? k.unsqueeze(1) : k;
  c.v = v.dim() == 3 ? v.unsqueeze(1) : v;
  TORCH_CHECK_VALUE(c.k.dim() == 4 && c.v.dim() == 4, "k and v must have 3 or 4 dimensions");
  const int64_t B = c.q.size(0), H = c.q.size(1), N = c.q.size(2), D = c.q.size(3), Hk = c.k.size(1), M = c.k.size(2);
  TORCH_CHECK_VALUE(c.v.sizes() == c.k.sizes(), "k and v must have the same shape, got ", k.sizes(), " and ", v.sizes());
  TORCH_CHECK_VALUE(c.k.size(3) == D, "query, key, value dimensions must be the same");                            // cu:1673
  TORCH_CHECK_VALUE(D == 16 || D == 32 || D == 64 || D == 96 || D == 128,
                    "only dimensions (16, 32, 64, 96, 128) allowed for now, got ", D);                              // cu:1674
  TORCH_CHECK_VALUE(c.k.size(0) == B, "batch mismatch between q (", B, ") and k/v (", c.k.size(0), ")");
  // grouped-query attention: query head h reads K/V head h / (H / Hk); single-headed (Hk == 1) and Hk == H are the two ends
  TORCH_CHECK_VALUE(Hk == H || (Hk >= 1 && H % Hk == 0),
                    "k/v heads must divide q heads (", H, "): grouped-query attention needs H % Hk == 0, got Hk = ", Hk);
  if (mask.has_value()) {
    TORCH_CHECK_VALUE(mask->scalar_type() == at::kBool && mask->dim() == 2 && mask->size(0) == B && mask->size(1) == M,
                      "mask must be a bool tensor of shape (", B, ", ", M, "), got ", mask->scalar_type(), " ", mask->sizes());
    c.mask = mask->contiguous();
  }
  if (bias.has_value()) {
    const int64_t lead = bias_batch ? B : H;
    TORCH_CHECK_VALUE(bias->dim() == 3 && bias->size(0) == lead && bias->size(1) == N && bias->size(2) == M,
                      "attn_bias must have shape (", lead, ", ", N, ", ", M, "), got ", bias->sizes());
    TORCH_CHECK_TYPE(bias->scalar_type() == q.scalar_type(), "attn_bias must have the dtype of q");
    c.bias = bias->contiguous();
  }
  c.q = prep(c.q); c.k = prep(c.k); c.v = prep(c.v);
  c.rows_q = {B, H, N};
  c.rows_k = {B, Hk, M};
  set_problem(c, q.scalar_type(), B, N, M, bias_batch, scale, causal, l2norm_qk, groups);
  return c;
}

Call canonicalise_varlen(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q, const Tensor& cu_k, int64_t max_q,
                         int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups) {
  need_abi("flash_cosine_sim_attention_varlen", "fcsa_forward_varlen / fcsa_backward_varlen", g_abi.forward_varlen, g_abi.backward_varlen,
           g_abi.backward_varlen_ws);
  TORCH_CHECK(q.is_cuda(), "flash_cosine_sim_attention_varlen: q, k, v must be GPU tensors (HIP kernels only, no CPU fallback)");
  for (const auto& [name, t] : {std::pair<const char*, const Tensor*>{"k", &k}, {"v", &v}, {"cu_seqlens_q", &cu_q}, {"cu_seqlens_k", &cu_k}})
    TORCH_CHECK_VALUE(t->device() == q.device(), name, " is on ", t->device(), " but q is on ", q.device(), ": all tensors must live on q's GPU");
  TORCH_CHECK_TYPE(q.scalar_type() == k.scalar_type() && q.scalar_type() == v.scalar_type(), "q, k, v must share a dtype, got ",
                   q.scalar_type(), ", ", k.scalar_type(), ", ", v.scalar_type());
  dtype_code(q.scalar_type());
  TORCH_CHECK_VALUE(q.dim() == 3 && k.dim() == 3 && v.dim() == 3, "varlen: q, k, v must be packed [total, heads, dim_head] tensors");
  TORCH_CHECK_VALUE(v.sizes() == k.sizes(), "k and v must have the same shape, got ", k.sizes(), " and ", v.sizes());
  TORCH_CHECK_TYPE(cu_q.scalar_type() == at::kInt && cu_k.scalar_type() == at::kInt, "cu_seqlens_q / cu_seqlens_k must be int32");
  TORCH_CHECK_VALUE(cu_q.dim() == 1 && cu_k.dim() == 1 && cu_q.numel() >= 1 && cu_q.numel() == cu_k.numel(),
                    "cu_seqlens_q and cu_seqlens_k must be 1-D of the same length (sequences + 1), got ", cu_q.sizes(), " and ", cu_k.sizes());
  const int64_t S = cu_q.numel() - 1, TQ = q.size(0), H = q.size(1), D = q.size(2), TK = k.size(0), Hk = k.size(1);
  TORCH_CHECK_VALUE(k.size(2) == D, "query, key, value dimensions must be the same");
  TORCH_CHECK_VALUE(D == 16 || D == 32 || D == 64 || D == 96 || D == 128, "only dimensions (16, 32, 64, 96, 128) allowed for now, got ", D);
  TORCH_CHECK_VALUE(Hk >= 1 && H % Hk == 0, "k/v heads must divide q heads (", H, "), got ", Hk);
  TORCH_CHECK_VALUE(max_q >= 0 && max_k >= 0 && max_q <= INT32_MAX && max_k <= INT32_MAX && S <= INT32_MAX,
                    "max_seqlen_q / max_seqlen_k must lie in [0, 2^31), got ", max_q, ", ", max_k);
  TORCH_CHECK_VALUE(H * std::max(TQ, TK) <= INT32_MAX, "varlen: heads x packed rows must stay below 2^31");
  Call c;
  c.q = prep(q); c.k = prep(k); c.v = prep(v);
  c.cu_q = cu_q.contiguous(); c.cu_k = cu_k.contiguous();
  c.rows_q = {H, TQ};
  c.rows_k = {Hk, TK};
  c.table = {c.cu_q.data_ptr<int32_t>(), c.cu_k.data_ptr<int32_t>(), TQ, TK};
  set_problem(c, q.scalar_type(), S, max_q, max_k, false, scale, causal, l2norm_qk, groups);
  return c;
}

at::DimVector with_last(at::DimVector rows, int64_t last) {
  rows.push_back(last);
  return rows;
}

// sliding window of a call (window ops): the library's struct, after the checks every window op shares; nullptr: no window
struct Win {
  fcsa_window w;
  Win(int64_t left, int64_t right) {
    need_abi("sliding window", "fcsa_forward_window / fcsa_backward_window", g_abi.forward_window, g_abi.backward_window, g_abi.backward_window_ws,
             g_abi.forward_kvcache_window, g_abi.forward_kvcache_window_ws);
    TORCH_CHECK_VALUE(left >= -1 && right >= -1, "window_size (", left, ", ", right, "): each side must be >= 0, or -1 for unbounded");
    w.left = (int32_t)std::min<int64_t>(left, INT32_MAX);
    w.right = (int32_t)std::min<int64_t>(right, INT32_MAX);
  }
};
Call windowed(Call c, const optional<fcsa_window>& w) {
  c.win = w;
  return c;
}
// window sides where a window is optional: (-1, -1) is the un-windowed call (nullopt), anything else passes Win's checks
struct OptWin {
  optional<fcsa_window> w;
  OptWin(int64_t left, int64_t right) { if (!(left == -1 && right == -1)) w = Win(left, right).w; }
  const fcsa_window* ptr() const { return w.has_value() ? &*w : nullptr; }
};

// The entry points of the family, one row each: the forward and backward symbols (as errors name them), the forward call, the backward
// workspace and the backward call (d_lse: the float32 lse gradient in inv_l's layout).  The one place that knows which C function serves
// which call; the slopes' entry points take the window as it is, NULL included.
struct TrainEntry {
  const char *forward_symbol, *backward_symbol;
  int (*forward)(const fcsa_forward_args&, const Call&);
  size_t (*backward_ws)(const Call&);      // null: that of the call without d_lse
  int (*backward)(const fcsa_backward_args&, const Call&, const float* d_lse);
};
enum TrainRoute { kPlainCall, kPackedCall, kWindowCall, kSlopesCall, kStateCall };
const TrainEntry kTrainEntries[] = {
    {"fcsa_forward", "fcsa_backward", [](const fcsa_forward_args& a, const Call&) { return g_abi.forward(&a); },
     [](const Call& c) { return g_abi.backward_ws(&c.p); }, [](const fcsa_backward_args& a, const Call&, const float*) { return g_abi.backward(&a); }},
    {"fcsa_forward_varlen", "fcsa_backward_varlen", [](const fcsa_forward_args& a, const Call& c) { return g_abi.forward_varlen(&a, c.seqs()); },
     [](const Call& c) { return g_abi.backward_varlen_ws(&c.p, c.seqs()); },
     [](const fcsa_backward_args& a, const Call& c, const float*) { return g_abi.backward_varlen(&a, c.seqs()); }},
    {"fcsa_forward_window", "fcsa_backward_window", [](const fcsa_forward_args& a, const Call& c) { return g_abi.forward_window(&a, c.seqs(), c.window()); },
     [](const Call& c) { return g_abi.backward_window_ws(&c.p, c.seqs(), c.window()); },
     [](const fcsa_backward_args& a, const Call& c, const float*) { return g_abi.backward_window(&a, c.seqs(), c.window()); }},
    {"fcsa_forward_alibi", "fcsa_backward_alibi",
     [](const fcsa_forward_args& a, const Call& c) { return g_abi.forward_alibi(&a, c.seqs(), c.window(), &*c.alibi); },
     [](const Call& c) { return g_abi.backward_alibi_ws(&c.p, c.seqs(), c.window()); },
     [](const fcsa_backward_args& a, const Call& c, const float*) { return g_abi.backward_alibi(&a, c.seqs(), c.window(), &*c.alibi); }},
    /* kStateCall: a backward with d_lse */ {nullptr, "fcsa_backward_state", nullptr, nullptr,
     [](const fcsa_backward_args& a, const Call& c, const float* d_lse) { return g_abi.backward_state(&a, c.seqs(), c.window(), d_lse); }},
};
TrainRoute train_route(const Call& c, bool d_lse) { return c.alibi ? kSlopesCall : d_lse ? kStateCall : c.win ? kWindowCall : c.packed() ? kPackedCall : kPlainCall; }

// (o, inv_l, qn, kn, rq, rk): o shaped like q; inv_l float32 [rows_q]; qn [rows_q, D], kn [rows_k, D] in q's dtype; rq / rk float32
// [rows_q, G] / [rows_k, G].  The saved-state tensors are empty (numel 0) where they are not produced.
using Saved = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>;

Saved forward_body(const Call& c, bool need_backward, Lap& lap) {
  const bool l2norm_qk = c.p.l2norm_qk != 0;
  TORCH_CHECK_VALUE(!l2norm_qk || (c.groups >= 1 && c.D % c.groups == 0), "groups (", c.groups, ") must divide the head dimension (", c.D, ")");
  c10::DeviceGuard guard(c.q.device());
  lap.mark(0);
  const auto opt = c.q.options();
  const auto f32 = opt.dtype(at::kFloat);
  fcsa_forward_args a;
  a.p = c.p;
  Tensor o = at::empty(c.q.sizes(), opt);
  Tensor none = at::empty({0}, f32);
  Tensor inv_l = need_backward ? at::empty(c.rows_q, f32) : none;
  Tensor qn = at::empty({0}, opt), kn = qn, rq = none, rk = none;
  if (l2norm_qk) {
    // An inference call (need_backward false) gets kn only -- and qn where q takes the row kernel (fcsa_forward_needs_qn): the
    // 16-bit forward kernels then write nothing but `o` (the reference's need_store_rowsum == false path, cu:1086, cu:1241).
    fcsa_problem rows = c.p;
    if (c.packed()) {      // the question is asked of the packed rows: batch 1, q_len = total_q
      rows.batch = 1; rows.q_len = (int32_t)c.q.size(0); rows.k_len = (int32_t)c.k.size(0);
    }
    if (g_abi.needs_qn(&rows, need_backward ? 1 : 0) != 0) qn = at::empty(with_last(c.rows_q, c.D), opt);
    kn = at::empty(with_last(c.rows_k, c.D), opt);
    if (need_backward) {
      rq = at::empty(with_last(c.rows_q, c.groups), f32);
      rk = at::empty(with_last(c.rows_k, c.groups), f32);
    }
  }
  const Layout l = c.layout();
  a.q = strided(c.q, l); a.k = strided(c.k, l); a.v = strided(c.v, l); a.o = strided(o, l);
  a.inv_l = need_backward ? inv_l.data_ptr<float>() : nullptr;
  a.mask = c.mask.has_value() ? static_cast<const uint8_t*>(c.mask->data_ptr()) : nullptr;
  a.attn_bias = c.bias.has_value() ? c.bias->data_ptr() : nullptr;
  a.norm.qn = qn.numel() > 0 ? qn.data_ptr() : nullptr;
  a.norm.kn = l2norm_qk ? kn.data_ptr() : nullptr;
  a.norm.rq = (l2norm_qk && need_backward) ? rq.data_ptr<float>() : nullptr;
  a.norm.rk = (l2norm_qk && need_backward) ? rk.data_ptr<float>() : nullptr;
  Tensor ws;
  a.workspace = nullptr; a.workspace_bytes = 0;
  if (!c.packed() && !c.alibi) {      // packed sequences and calls with slopes never split the key range
    size_t need = g_abi.forward_ws(&a.p);      // 0 unless the key range is split (grids that cannot fill the chip)
    if (c.win) {      // a window that IS the un-windowed or the causal call splits like that call: room for either
      fcsa_problem other = a.p;
      other.causal = !other.causal;
      need = std::max(need, g_abi.forward_ws(&other));
    }
    if (need > 0) {
      ws = at::empty({(int64_t)need}, opt.dtype(at::kByte));
      a.workspace = ws.data_ptr(); a.workspace_bytes = need;
    }
  }
  a.stream = stream_of(c.q);
  lap.mark(1);
  const TrainEntry& e = kTrainEntries[train_route(c, false)];
  check(e.forward(a, c), e.forward_symbol);
  lap.mark(2);
  lap.count(6);
  if (c.merged) o = o.squeeze(1);                                                                                  // cu:1740-1741
  return std::make_tuple(o, inv_l, qn, kn, rq, rk);
}

Saved forward(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& mask, const optional<Tensor>& attn_bias,
              bool attn_bias_batch_dim, double scale, bool causal, bool l2norm_qk, int64_t groups, bool need_backward) {
  Lap lap(true);
  return forward_body(canonicalise(q, k, v, mask, attn_bias, attn_bias_batch_dim, scale, causal, l2norm_qk, groups), need_backward, lap);
}
// the window ops take their sides as they are ((-1, -1) is a window too) and check them before their tensors
Saved window_forward(const Tensor& q, const Tensor& k, const Tensor& v, double scale, bool causal, bool l2norm_qk, int64_t groups,
                     bool need_backward, int64_t left, int64_t right) {
  const Win win(left, right);
  Lap lap(true);
  return forward_body(windowed(canonicalise(q, k, v, c10::nullopt, c10::nullopt, false, scale, causal, l2norm_qk, groups), win.w), need_backward, lap);
}
Saved varlen_forward(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q, const Tensor& cu_k, int64_t max_q, int64_t max_k,
                     double scale, bool causal, bool l2norm_qk, int64_t groups, bool need_backward) {
  Lap lap(false);
  return forward_body(canonicalise_varlen(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups), need_backward, lap);
}
Saved varlen_window_forward(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q, const Tensor& cu_k, int64_t max_q,
                            int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups, bool need_backward, int64_t left,
                            int64_t right) {
  Lap lap(false);
  const Win win(left, right);
  return forward_body(windowed(canonicalise_varlen(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups), win.w), need_backward, lap);
}

// (dq, dk, dv, d_bias) in the shapes / dtype of the canonical inputs; d_bias (dense only) is empty when not requested and undefined for a
// packed call
using Grads = std::tuple<Tensor, Tensor, Tensor, Tensor>;

Grads backward_body(const Call& c, const Tensor& d_out, const Tensor& o, const Tensor& inv_l, const Tensor& qn, const Tensor& kn, const Tensor& rq,
                    const Tensor& rk, bool need_bias_grad, Lap& lap) {
  const bool l2norm_qk = c.p.l2norm_qk != 0;
  const at::ScalarType dt = c.q.scalar_type();
  const auto dev = c.q.device();
  c10::DeviceGuard guard(dev);
  const auto opt = c.q.options();
  Tensor oc = o, doc = d_out;
  if (!c.packed()) {
    if (oc.dim() == 3) oc = oc.unsqueeze(1);
    if (doc.dim() == 3) doc = doc.unsqueeze(1);
    // A broadcast gradient (`out.sum().backward()`, the reference's own timing protocol, benchmark.py:46-48: one scalar expanded with
    // all strides 0) is not materialised at [B,H,N,D]: one contiguous feature row is, and the kernels read it with a row pitch of 0.
    bool broadcast = doc.numel() > 0;
    for (int64_t d = 0; d < doc.dim(); ++d) broadcast = broadcast && (doc.stride(d) == 0 || doc.size(d) == 1);
    if (broadcast && doc.dim() == 4) {
      Tensor row = doc.as_strided({doc.size(3)}, {0}).to(dt).contiguous();                             // [D], a D-element copy kernel
      doc = row.as_strided(doc.sizes(), {0, 0, 0, 1});
    }
  }
  oc = prep(oc);
  if (doc.scalar_type() != dt) doc = doc.to(dt);
  doc = prep(doc);
  TORCH_CHECK_VALUE(doc.sizes() == oc.sizes(), "d_out must have the shape of the output");
  TORCH_CHECK_VALUE(oc.sizes() == c.q.sizes(), "o does not belong to these inputs");
  // these ops are public (torch.ops.fcsa.backward, ext.backward): everything a kernel dereferences is checked, not only its size
  auto saved_ok = [&](const char* name, const Tensor& t, at::ScalarType st, const at::DimVector& rows, int64_t last) {
    const int64_t numel = c10::multiply_integers(rows) * last;
    TORCH_CHECK_VALUE(t.defined() && t.device() == dev && t.scalar_type() == st && t.numel() == numel && t.is_contiguous(),
                      name, " does not belong to these inputs (expected a contiguous ", st, " tensor of ", numel, " elements on ", dev, ")");
  };
  TORCH_CHECK_TYPE(oc.scalar_type() == dt && oc.device() == dev, "o must have the dtype and device of q");
  TORCH_CHECK_VALUE(doc.device() == dev, "d_out is on ", doc.device(), " but q is on ", dev);
  saved_ok("inv_l", inv_l, at::kFloat, c.rows_q, 1);
  if (l2norm_qk) {
    saved_ok("qn", qn, dt, c.rows_q, c.D);
    saved_ok("kn", kn, dt, c.rows_k, c.D);
    saved_ok("rq", rq, at::kFloat, c.rows_q, c.groups);
    saved_ok("rk", rk, at::kFloat, c.rows_k, c.groups);
  }
  // the gradient of the rows' log-sum-exp (attention_state_backward), brought into inv_l's layout whatever its strides: float32
  // contiguous [B, H, N], packed [H, total_q] from the public [total_q, H]
  Tensor gl;
  if (c.d_lse != nullptr) {
    need_abi("attention_state_backward", "fcsa_backward_state", g_abi.backward_state);
    gl = c.packed() ? c.d_lse->transpose(0, 1) : *c.d_lse;
    TORCH_CHECK_VALUE(gl.device() == dev && gl.sizes() == at::IntArrayRef(c.rows_q), "d_lse must have the shape of lse on q's device");
    gl = gl.to(at::kFloat).contiguous();
  }
  lap.mark(3);
  Tensor dq = at::empty(c.q.sizes(), opt);
  Tensor dk = at::empty(c.k.sizes(), opt);
  Tensor dv = at::empty(c.k.sizes(), opt);
  // d_bias in the bias dtype, every element written once by the library: no zero-fill, no f32 tensor, no cast pass (cf. cu:1827, cu:1912)
  Tensor db;
  if (!c.packed()) db = (c.bias.has_value() && need_bias_grad) ? at::empty(c.bias->sizes(), opt) : at::empty({0}, opt);
  fcsa_backward_args a;
  a.p = c.p;
  const TrainEntry& e = kTrainEntries[train_route(c, gl.defined())];
  size_t wsb = (e.backward_ws != nullptr ? e : kTrainEntries[train_route(c, false)]).backward_ws(c);
  if (wsb < 256) wsb = 256;
  Tensor ws = at::empty({(int64_t)wsb}, opt.dtype(at::kByte));      // the caching allocator
  const Layout l = c.layout();
  a.d_out = strided(doc, l); a.o = strided(oc, l);
  a.inv_l = inv_l.data_ptr<float>();
  a.q = strided(c.q, l); a.k = strided(c.k, l); a.v = strided(c.v, l);
  a.mask = c.mask.has_value() ? static_cast<const uint8_t*>(c.mask->data_ptr()) : nullptr;
  a.attn_bias = c.bias.has_value() ? c.bias->data_ptr() : nullptr;
  a.norm.qn = l2norm_qk ? qn.data_ptr() : nullptr;
  a.norm.kn = l2norm_qk ? kn.data_ptr() : nullptr;
  a.norm.rq = l2norm_qk ? rq.data_ptr<float>() : nullptr;
  a.norm.rk = l2norm_qk ? rk.data_ptr<float>() : nullptr;
  a.dq = strided(dq, l); a.dk = strided(dk, l); a.dv = strided(dv, l);
  a.d_bias = (db.defined() && db.numel() > 0) ? db.data_ptr() : nullptr;
  a.workspace = ws.data_ptr(); a.workspace_bytes = wsb;
  a.stream = stream_of(c.q);
  lap.mark(4);
  check(e.backward(a, c, gl.defined() ? gl.data_ptr<float>() : nullptr), e.backward_symbol);
  lap.mark(5);
  lap.count(7);
  return std::make_tuple(dq, dk, dv, db);
}

// the dense gradients in the shapes the caller's q, k, v came in (merged batch-heads, 3-D k / v)
Grads dense_backward(const Tensor& d_out, const Tensor& o, const Tensor& inv_l, const Tensor& q, const Tensor& k, const Tensor& v,
                     const optional<Tensor>& mask, const optional<Tensor>& attn_bias, const Tensor& qn, const Tensor& kn, const Tensor& rq,
                     const Tensor& rk, bool attn_bias_batch_dim, double scale, bool causal, bool l2norm_qk, int64_t groups, bool need_bias_grad,
                     const optional<fcsa_window>& win) {
  Lap lap(true);
  auto [dq, dk, dv, db] = backward_body(windowed(canonicalise(q, k, v, mask, attn_bias, attn_bias_batch_dim, scale, causal, l2norm_qk, groups), win),
                                        d_out, o, inv_l, qn, kn, rq, rk, need_bias_grad, lap);
  return std::make_tuple(dq.reshape(q.sizes()), dk.reshape(k.sizes()), dv.reshape(v.sizes()), db);
}
Grads backward(const Tensor& d_out, const Tensor& o, const Tensor& inv_l, const Tensor& q, const Tensor& k, const Tensor& v,
               const optional<Tensor>& mask, const optional<Tensor>& attn_bias, const Tensor& qn, const Tensor& kn, const Tensor& rq,
               const Tensor& rk, bool attn_bias_batch_dim, double scale, bool causal, bool l2norm_qk, int64_t groups, bool need_bias_grad) {
  return dense_backward(d_out, o, inv_l, q, k, v, mask, attn_bias, qn, kn, rq, rk, attn_bias_batch_dim, scale, causal, l2norm_qk, groups,
                        need_bias_grad, c10::nullopt);
}

// (dq, dk, dv) shaped like q, k, v
using Grads3 = std::tuple<Tensor, Tensor, Tensor>;
Grads3 first3(const Grads& g) { return std::make_tuple(std::get<0>(g), std::get<1>(g), std::get<2>(g)); }

Grads3 window_backward(const Tensor& d_out, const Tensor& o, const Tensor& inv_l, const Tensor& q, const Tensor& k, const Tensor& v,
                       const Tensor& qn, const Tensor& kn, const Tensor& rq, const Tensor& rk, double scale, bool causal, bool l2norm_qk,
                       int64_t groups, int64_t left, int64_t right) {
  const Win win(left, right);
  return first3(dense_backward(d_out, o, inv_l, q, k, v, c10::nullopt, c10::nullopt, qn, kn, rq, rk, false, scale, causal, l2norm_qk, groups, false,
                               win.w));
}
Grads3 varlen_backward(const Tensor& d_out, const Tensor& o, const Tensor& inv_l, const Tensor& q, const Tensor& k, const Tensor& v,
                       const Tensor& cu_q, const Tensor& cu_k, const Tensor& qn, const Tensor& kn, const Tensor& rq, const Tensor& rk,
                       int64_t max_q, int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups) {
  Lap lap(false);
  return first3(backward_body(canonicalise_varlen(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups), d_out, o, inv_l, qn, kn, rq,
                              rk, false, lap));
}
Grads3 varlen_window_backward(const Tensor& d_out, const Tensor& o, const Tensor& inv_l, const Tensor& q, const Tensor& k, const Tensor& v,
                              const Tensor& cu_q, const Tensor& cu_k, const Tensor& qn, const Tensor& kn, const Tensor& rq, const Tensor& rk,
                              int64_t max_q, int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups, int64_t left,
                              int64_t right) {
  Lap lap(false);
  const Win win(left, right);
  return first3(backward_body(windowed(canonicalise_varlen(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups), win.w), d_out, o,
                              inv_l, qn, kn, rq, rk, false, lap));
}

// ---- autograd in C++ (reference: the Python autograd.Function FlashCosineSimAttention, flash_cosine_sim_attention.py:245-302).
// A Python Function costs ~60 us of interpreter / engine hand-over per forward+backward; this node costs a few.  forward and
// backward go through the dispatcher by op name (fcsa::forward / fcsa::backward, ...), so torch.compile traces them with the fake kernels.
//
// One node for the four differentiable ops.  A family names its op pair and what rides along besides q, k, v: Extra, the tensors
// between v and the scalars; Scalars, up to need_backward; Window, the scalars after it.  With them
//   the forward op  takes (q, k, v, Extra..., Scalars..., need_backward, Window...)                 -- the attention op's arguments and the flag,
//   the backward op takes (d_out, o, inv_l, q, k, v, Extra..., qn, kn, rq, rk, Scalars..., Window...) -- with need_bias_grad after Scalars where
// the family has a bias gradient.  Everything is resolved at compile time: the calls are the typed dispatcher calls of the four former nodes.
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

struct DenseOps {
  static constexpr const char* forward_name = "fcsa::forward";
  static constexpr const char* backward_name = "fcsa::backward";
  static constexpr auto fwd = &forward;
  static constexpr auto bwd = &backward;
  using Extra = std::tuple<optional<Tensor>, optional<Tensor>>;      // mask, attn_bias
  using Scalars = std::tuple<bool, double, bool, bool, int64_t>;     // attn_bias_batch_dim, scale, causal, l2norm_qk, groups
  using Window = std::tuple<>;
  static constexpr bool bias_grad = true;
};
struct VarlenOps {
  static constexpr const char* forward_name = "fcsa::varlen_forward";
  static constexpr const char* backward_name = "fcsa::varlen_backward";
  static constexpr auto fwd = &varlen_forward;
  static constexpr auto bwd = &varlen_backward;
  using Extra = std::tuple<Tensor, Tensor>;                                    // cu_seqlens_q, cu_seqlens_k
  using Scalars = std::tuple<int64_t, int64_t, double, bool, bool, int64_t>;   // max_seqlen_q, max_seqlen_k, scale, causal, l2norm_qk, groups
  using Window = std::tuple<>;
  static constexpr bool bias_grad = false;
};
struct WindowOps {
  static constexpr const char* forward_name = "fcsa::window_forward";
  static constexpr const char* backward_name = "fcsa::window_backward";
  static constexpr auto fwd = &window_forward;
  static constexpr auto bwd = &window_backward;
  using Extra = std::tuple<>;
  using Scalars = std::tuple<double, bool, bool, int64_t>;      // scale, causal, l2norm_qk, groups
  using Window = std::tuple<int64_t, int64_t>;                  // window_left, window_right
  static constexpr bool bias_grad = false;
};
struct VarlenWindowOps {
  static constexpr const char* forward_name = "fcsa::varlen_window_forward";
  static constexpr const char* backward_name = "fcsa::varlen_window_backward";
  static constexpr auto fwd = &varlen_window_forward;
  static constexpr auto bwd = &varlen_window_backward;
  using Extra = VarlenOps::Extra;
  using Scalars = VarlenOps::Scalars;
  using Window = WindowOps::Window;
  static constexpr bool bias_grad = false;
};

// a tuple's elements by reference (the argument lists below are concatenations of such tuples: nothing is copied)
template <class... T>
std::tuple<const T&...> refs(const std::tuple<T...>& t) {
  return std::apply([](const T&... e) { return std::tie(e...); }, t);
}

template <class F>
auto forward_args(const Tensor& q, const Tensor& k, const Tensor& v, const typename F::Extra& x, const typename F::Scalars& s, bool need,
                  const typename F::Window& w) {
  return std::tuple_cat(std::tie(q, k, v), refs(x), refs(s), std::make_tuple(need), refs(w));      // references to the arguments, the flag by value
}

// the dispatcher op `name`, typed like the function that implements it
template <class Fn>
auto typed_op(const char* name, Fn*) {
  return c10::Dispatcher::singleton().findSchemaOrThrow(name, "").typed<Fn>();
}

// an extra tensor as a saved variable (an absent optional: undefined), and back in the type the backward op takes it in
Tensor saveable(const Tensor& t) { return t; }
Tensor saveable(const optional<Tensor>& t) { return t.has_value() ? *t : Tensor(); }
template <class T>
T restored(const Tensor& t) {
  if constexpr (std::is_same_v<T, Tensor>) return t;
  else return t.defined() ? T(t) : T();
}
template <class X, size_t... I>
X restored_tuple(const variable_list& saved, size_t at, std::index_sequence<I...>) {
  return X{restored<std::tuple_element_t<I, X>>(saved[at + I])...};
}

template <class F>
struct AttentionNode : public torch::autograd::Function<AttentionNode<F>> {
  using Extra = typename F::Extra;
  using Scalars = typename F::Scalars;
  using Window = typename F::Window;
  static constexpr size_t kExtra = std::tuple_size_v<Extra>;

  // attn_bias is an argument of its own so that the engine sees the one extra tensor that takes a gradient; Extra holds it too (dense op)
  static Tensor forward(AutogradContext* ctx, const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& attn_bias, const Extra& x,
                        const Scalars& s, const Window& w) {
    // (Function::apply runs this with grad mode OFF: the no_grad case is decided by the caller, differentiable())
    const bool bias_grad = attn_bias.has_value() && attn_bias->requires_grad();
    const bool need = q.requires_grad() || k.requires_grad() || v.requires_grad() || bias_grad;                    // cu:1689
    at::AutoDispatchBelowADInplaceOrView guard;
    static auto op = typed_op(F::forward_name, F::fwd);
    auto r = std::apply([](const auto&... a) { return op.call(a...); }, forward_args<F>(q, k, v, x, s, need, w));
    if (need) {
      variable_list save{std::get<0>(r), std::get<1>(r), q, k, v, std::get<2>(r), std::get<3>(r), std::get<4>(r), std::get<5>(r)};
      std::apply([&](const auto&... e) { (save.push_back(saveable(e)), ...); }, x);
      ctx->save_for_backward(std::move(save));
      ctx->saved_data["scalars"] = c10::IValue(s);
      if constexpr (std::tuple_size_v<Window> > 0) ctx->saved_data["window"] = c10::IValue(w);
      ctx->saved_data["bias_grad"] = bias_grad;
    }
    return std::get<0>(r);
  }

  // one entry per forward argument: q, k, v, attn_bias, and nothing for Extra, Scalars, Window
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto t = ctx->get_saved_variables();      // o, inv_l, q, k, v, qn, kn, rq, rk, Extra...
    const Extra x = restored_tuple<Extra>(t, 9, std::make_index_sequence<kExtra>());
    const Scalars s = ctx->saved_data["scalars"].template to<Scalars>();
    Window w;
    if constexpr (std::tuple_size_v<Window> > 0) w = ctx->saved_data["window"].template to<Window>();
    const bool bias_grad = ctx->saved_data["bias_grad"].toBool();
    static auto op = typed_op(F::backward_name, F::bwd);
    auto call = [](const auto&... a) { return op.call(a...); };
    const auto head = std::tuple_cat(std::tie(grads[0], t[0], t[1], t[2], t[3], t[4]), refs(x), std::tie(t[5], t[6], t[7], t[8]), refs(s));
    if constexpr (F::bias_grad) {
      auto g = std::apply(call, std::tuple_cat(head, std::tie(bias_grad), refs(w)));
      return {std::get<0>(g), std::get<1>(g), std::get<2>(g), bias_grad ? std::get<3>(g) : Tensor(), Tensor(), Tensor(), Tensor()};
    } else {
      auto g = std::apply(call, std::tuple_cat(head, refs(w)));
      return {std::get<0>(g), std::get<1>(g), std::get<2>(g), Tensor(), Tensor(), Tensor(), Tensor()};
    }
  }
};

// no autograd (inference / inputs that do not require grad): forward without saved state
template <class F>
Tensor inference(const Tensor& q, const Tensor& k, const Tensor& v, const typename F::Extra& x, const typename F::Scalars& s,
                 const typename F::Window& w) {
  return std::get<0>(std::apply(F::fwd, forward_args<F>(q, k, v, x, s, false, w)));
}

template <class F>
Tensor differentiable(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& attn_bias, const typename F::Extra& x,
                      const typename F::Scalars& s, const typename F::Window& w) {
  // under torch.no_grad() nothing will ever call backward, whatever the inputs' requires_grad says: take the inference path
  // (no saved state, no inv_l / inverse-norm / normalised-q writes), like a Python Function's ctx.needs_input_grad would
  const bool tracked = at::GradMode::is_enabled() &&
                       (q.requires_grad() || k.requires_grad() || v.requires_grad() || (attn_bias.has_value() && attn_bias->requires_grad()));
  if (!tracked) {
    at::AutoDispatchBelowADInplaceOrView guard;
    return inference<F>(q, k, v, x, s, w);
  }
  return AttentionNode<F>::apply(q, k, v, attn_bias, x, s, w);
}

// the registered entry points (the dispatcher wants one function per op and key): CUDA key -> *_plain, Autograd key -> *_autograd
Tensor attention_plain(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& mask, const optional<Tensor>& attn_bias,
                       bool attn_bias_batch_dim, double scale, bool causal, bool l2norm_qk, int64_t groups) {
  return inference<DenseOps>(q, k, v, {mask, attn_bias}, {attn_bias_batch_dim, scale, causal, l2norm_qk, groups}, {});
}
Tensor attention_autograd(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& mask, const optional<Tensor>& attn_bias,
                          bool attn_bias_batch_dim, double scale, bool causal, bool l2norm_qk, int64_t groups) {
  return differentiable<DenseOps>(q, k, v, attn_bias, {mask, attn_bias}, {attn_bias_batch_dim, scale, causal, l2norm_qk, groups}, {});
}
Tensor varlen_attention_plain(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q, const Tensor& cu_k, int64_t max_q,
                              int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups) {
  return inference<VarlenOps>(q, k, v, {cu_q, cu_k}, {max_q, max_k, scale, causal, l2norm_qk, groups}, {});
}
Tensor varlen_attention_autograd(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q, const Tensor& cu_k, int64_t max_q,
                                 int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups) {
  return differentiable<VarlenOps>(q, k, v, c10::nullopt, {cu_q, cu_k}, {max_q, max_k, scale, causal, l2norm_qk, groups}, {});
}
Tensor window_attention_plain(const Tensor& q, const Tensor& k, const Tensor& v, double scale, bool causal, bool l2norm_qk, int64_t groups,
                              int64_t left, int64_t right) {
  return inference<WindowOps>(q, k, v, {}, {scale, causal, l2norm_qk, groups}, {left, right});
}
Tensor window_attention_autograd(const Tensor& q, const Tensor& k, const Tensor& v, double scale, bool causal, bool l2norm_qk, int64_t groups,
                                 int64_t left, int64_t right) {
  return differentiable<WindowOps>(q, k, v, c10::nullopt, {}, {scale, causal, l2norm_qk, groups}, {left, right});
}
Tensor varlen_window_attention_plain(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q, const Tensor& cu_k, int64_t max_q,
                                     int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
  return inference<VarlenWindowOps>(q, k, v, {cu_q, cu_k}, {max_q, max_k, scale, causal, l2norm_qk, groups}, {left, right});
}
Tensor varlen_window_attention_autograd(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q, const Tensor& cu_k, int64_t max_q,
                                        int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
  return differentiable<VarlenWindowOps>(q, k, v, c10::nullopt, {cu_q, cu_k}, {max_q, max_k, scale, causal, l2norm_qk, groups}, {left, right});
}


// ---- decoding against a key/value cache (fcsa_forward_kvcache and the entry points built on it) ---------------------------------------
// q [B, H, N, D]; k_cache / v_cache [B, Hk, capacity, D] or, with a block_table, [num_blocks, Hk, page_size, D] (any strides with the
// feature dim contiguous: they are written in place, so they are never copied); k_new / v_new [B, Hk, N_new, D]; cache_seqlens int32 [B]
// and block_table int32 [B, max_blocks] on q's device.  Table contents are never read on the host: the call does not synchronise.
// cu_q: a ragged step -- q [total_q, H, D] packed by the int32 table cu_q [B + 1], k_new / v_new [total_q, Hk, D], max_seqlen_q an upper
// bound on the rows of a sequence; o is shaped like q.
//
// One description of a call, CacheCall: every op function fills the members it has and hands it to kvcache_call, which runs the checks
// (cache_checks), fills the library's structs (fill_lib_call) and dispatches through the one table of entry points (kEntries).
enum class Route { Plain, Prefill, Step, Tree, Alibi };

struct CacheCall {
  // what every op has
  const Tensor &q, &k_cache, &v_cache;
  const optional<Tensor> &k_new, &v_new, &cache_seqlens, &block_table;
  int64_t max_seqlen_k; double scale; bool causal, l2norm_qk; int64_t groups;
  // what some have
  const fcsa_window* win = nullptr;                       // a sliding window
  const Tensor *k_scale = nullptr, *v_scale = nullptr;    // an e4m3fn cache (its codes as uint8 tensors) with its two scale tensors
  const Tensor* cu_q = nullptr; int64_t max_seqlen_q = 0; // a ragged step: packed q [total_q, H, D], with the bound on a sequence's rows
  bool lse = false;                                       // the rows' log-sum-exp as a second result
  Route route = Route::Plain;
  fcsa_kvcache_step step{};                               // Step, Alibi: the routing fields
  const Tensor* extra = nullptr;                          // Tree: tree_mask; Alibi: alibi_slopes
  bool ragged() const { return cu_q != nullptr; }
  bool fp8() const { return k_scale != nullptr; }
};

const Tensor* ptr(const optional<Tensor>& t) { return t.has_value() ? &*t : nullptr; }

void set_scales(CacheCall& c, const optional<Tensor>& k_scale, const optional<Tensor>& v_scale) {
  TORCH_CHECK_VALUE(k_scale.has_value() == v_scale.has_value(), "k_scale and v_scale must be given together");
  c.k_scale = ptr(k_scale); c.v_scale = ptr(v_scale);
}

// the routing fields of an engine step (chunk_rows / max_decode_tokens < 0: the library's default / total_q; no_decode, no_chunk: the
// caller's promises, which skip a launch)
fcsa_kvcache_step step_fields(int64_t chunk_rows, int64_t max_decode_tokens, bool no_decode, bool no_chunk) {
  TORCH_CHECK_VALUE(chunk_rows >= -1, "chunk_rows must be a non-negative integer (or -1: the default), got ", chunk_rows);
  TORCH_CHECK_VALUE(max_decode_tokens >= -1, "max_decode_tokens must be a non-negative integer (or -1: total_q), got ", max_decode_tokens);
  fcsa_kvcache_step st{};
  st.chunk_rows = (int32_t)std::min<int64_t>(chunk_rows, INT32_MAX);
  st.max_decode_tokens = std::min<int64_t>(max_decode_tokens, INT32_MAX);
  st.no_decode = no_decode; st.no_chunk = no_chunk;
  return st;
}

// The geometry of a cache that serves B sequences, contiguous or paged by block_table: the table's checks, the capacity, and the table
// fields of fcsa_kvcache.  The forward calls say "batch" and count q's sequences, kvcache_compact says "sequences" and counts accepted's.
struct Geometry {
  Tensor tab;      // block_table, contiguous; undefined for a contiguous cache
  int64_t capacity = 0, page = 0, num_blocks = 0;
  void fill(fcsa_kvcache& kv) const {
    kv.capacity = (int32_t)capacity; kv.page_size = (int32_t)page; kv.num_blocks = (int32_t)num_blocks;
    kv.block_table = tab.defined() ? tab.data_ptr<int32_t>() : nullptr;
    kv.block_table_stride = tab.defined() ? tab.size(1) : 0;
  }
};
template <class SameDev>
Geometry cache_geometry(const Tensor& k_cache, const optional<Tensor>& block_table, int64_t B, const SameDev& same_dev, const char* rows,
                        const char* counted) {
  Geometry g;
  g.capacity = k_cache.size(2);
  if (block_table.has_value()) {
    same_dev("block_table", *block_table);
    TORCH_CHECK_TYPE(block_table->scalar_type() == at::kInt, "block_table must be int32");
    TORCH_CHECK_VALUE(block_table->dim() == 2 && block_table->size(0) == B, "block_table must be [", rows, ", max_blocks]");
    g.page = k_cache.size(2); g.num_blocks = k_cache.size(0); g.capacity = block_table->size(1) * g.page;
    g.tab = block_table->contiguous();
  } else {
    TORCH_CHECK_VALUE(k_cache.size(0) == B, "batch mismatch between ", counted, " (", B, ") and the caches (", k_cache.size(0), ")");
  }
  return g;
}

// What the checks of a call return: the canonical tensors, kept alive until the call has been issued, and the sizes read off them.
struct CacheKeep {
  Tensor q, cu, words, slopes, kn, vn, sl;
  Geometry g;
  int64_t B = 0, H = 0, N = 0, D = 0, Hk = 0, new_len = 0;      // ragged: N is the number of packed rows
};

CacheKeep cache_checks(const CacheCall& c) {
  const Tensor &q = c.q, &k_cache = c.k_cache, &v_cache = c.v_cache;
  const bool ragged = c.ragged();
  CacheKeep k;
  TORCH_CHECK(q.is_cuda(), "flash_cosine_sim_attention_with_kvcache: q and the caches must be GPU tensors (HIP kernels only)");
  auto same_dev = [&](const char* name, const Tensor& t) {
    TORCH_CHECK_VALUE(t.device() == q.device(), name, " is on ", t.device(), " but q is on ", q.device(), ": all tensors must live on q's GPU");
  };
  same_dev("k_cache", k_cache);
  same_dev("v_cache", v_cache);
  if (c.fp8()) {
    // the codes travel as bytes (the Python entry point passes float8_e4m3fn caches as their uint8 views: the dispatcher's own machinery
    // -- opcheck, functionalisation -- runs arithmetic on mutated arguments, which float8 tensors do not support)
    TORCH_CHECK_TYPE(k_cache.scalar_type() == at::kByte && v_cache.scalar_type() == at::kByte,
                     "kvcache_fp8_forward takes the e4m3fn codes of both caches as uint8 tensors (cache.view(torch.uint8)), got ",
                     k_cache.scalar_type(), " and ", v_cache.scalar_type());
    TORCH_CHECK_TYPE(q.scalar_type() == at::kHalf || q.scalar_type() == at::kBFloat16,
                     "fp8 caches take float16 or bfloat16 queries, got ", q.scalar_type());
  } else {
    TORCH_CHECK_TYPE(q.scalar_type() == k_cache.scalar_type() && q.scalar_type() == v_cache.scalar_type(), "q, k_cache, v_cache must share a dtype");
  }
  dtype_code(q.scalar_type());
  TORCH_CHECK_VALUE(q.dim() == (ragged ? 3 : 4) && k_cache.dim() == 4 && v_cache.dim() == 4,
                    ragged ? "q must be a packed [total_q, heads, dim_head] tensor and k_cache, v_cache must have 4 dimensions"
                           : "q, k_cache, v_cache must have 4 dimensions");
  TORCH_CHECK_VALUE(k_cache.sizes() == v_cache.sizes(), "k_cache and v_cache must have the same shape");
  if (ragged) {
    const Tensor& cu_q = *c.cu_q;
    same_dev("cu_seqlens_q", cu_q);
    TORCH_CHECK_TYPE(cu_q.scalar_type() == at::kInt, "cu_seqlens_q must be int32");
    TORCH_CHECK_VALUE(cu_q.dim() == 1 && cu_q.numel() >= 1, "cu_seqlens_q must be 1-D with sequences + 1 entries, got ", cu_q.sizes());
    TORCH_CHECK_VALUE(c.max_seqlen_q >= 0 && c.max_seqlen_q <= INT32_MAX, "max_seqlen_q must lie in [0, 2^31), got ", c.max_seqlen_q);
    TORCH_CHECK_VALUE(q.size(0) * std::max<int64_t>(q.size(1), 1) <= INT32_MAX, "heads x packed rows must stay below 2^31");
    k.cu = cu_q.contiguous();
  }
  if (c.route == Route::Tree) {
    const Tensor& tree = *c.extra;
    TORCH_CHECK_TYPE(tree.scalar_type() == at::kLong, "tree_mask must be int64, got ", tree.scalar_type());
    same_dev("tree_mask", tree);
    TORCH_CHECK_VALUE(tree.dim() == 1 && tree.size(0) == q.size(0), "tree_mask must be [total_q] (", q.size(0), "), packed like q, got ", tree.sizes());
    k.words = tree.contiguous();
  }
  if (c.route == Route::Alibi) {
    const Tensor& alibi = *c.extra;
    TORCH_CHECK_TYPE(alibi.scalar_type() == at::kFloat, "alibi_slopes must be float32, got ", alibi.scalar_type());
    same_dev("alibi_slopes", alibi);
    const int64_t seqs_n = k.cu.numel() - 1;
    TORCH_CHECK_VALUE((alibi.dim() == 1 && alibi.size(0) == q.size(1)) || (alibi.dim() == 2 && alibi.size(0) == seqs_n && alibi.size(1) == q.size(1)),
                      "alibi_slopes must be [heads] (", q.size(1), ") or [sequences, heads] (", seqs_n, ", ", q.size(1), "), got ", alibi.sizes());
    k.slopes = alibi;      // any strides: the kernels take element strides, and a view keeps in-place updates visible to a captured graph
  }
  const int64_t B = k.B = ragged ? k.cu.numel() - 1 : q.size(0), H = k.H = q.size(1), N = k.N = ragged ? q.size(0) : q.size(2);
  const int64_t D = k.D = q.size(-1), Hk = k.Hk = k_cache.size(1);
  TORCH_CHECK_VALUE(k_cache.size(3) == D, "query, key, value dimensions must be the same");
  TORCH_CHECK_VALUE(D == 16 || D == 32 || D == 64 || D == 96 || D == 128, "only dimensions (16, 32, 64, 96, 128) allowed for now, got ", D);
  TORCH_CHECK_VALUE(Hk >= 1 && H % Hk == 0, "k/v heads must divide q heads (", H, "), got ", Hk);
  TORCH_CHECK_VALUE(!c.l2norm_qk || (c.groups >= 1 && D % c.groups == 0), "groups (", c.groups, ") must divide the head dimension (", D, ")");
  TORCH_CHECK_VALUE(rows_ok(k_cache) && rows_ok(v_cache), "k_cache / v_cache: the feature dim must be contiguous and rows 16-byte aligned "
                    "(the caches are updated in place, so they are not copied)");
  k.g = cache_geometry(k_cache, c.block_table, B, same_dev, "batch", "q");
  if (k.g.tab.defined()) {      // the page rule (kvcache_compact leaves it to the library)
    TORCH_CHECK_VALUE(k.g.page > 0 && k.g.page % 16 == 0, "page_size (", k.g.page, ") must be a positive multiple of 16");
    TORCH_CHECK_VALUE(k.g.num_blocks >= 1, "a paged cache needs at least one block");
  }
  TORCH_CHECK_VALUE(k.g.capacity <= INT32_MAX, "cache capacity must stay below 2^31");
  const optional<Tensor>&k_new = c.k_new, &v_new = c.v_new;
  TORCH_CHECK_VALUE(k_new.has_value() == v_new.has_value(), "k_new and v_new must be given together");
  if (k_new.has_value()) {
    same_dev("k_new", *k_new);
    same_dev("v_new", *v_new);
    TORCH_CHECK_TYPE(k_new->scalar_type() == q.scalar_type() && v_new->scalar_type() == q.scalar_type(), "k_new / v_new must have q's dtype");
    if (ragged) {
      TORCH_CHECK_VALUE(k_new->dim() == 3 && k_new->sizes() == v_new->sizes() && k_new->size(0) == N && k_new->size(1) == Hk && k_new->size(2) == D,
                        "k_new / v_new must be packed [total_q, kv_heads, dim_head] like q, got ", k_new->sizes(), " and ", v_new->sizes());
    } else {
      TORCH_CHECK_VALUE(k_new->dim() == 4 && k_new->sizes() == v_new->sizes() && k_new->size(0) == B && k_new->size(1) == Hk && k_new->size(3) == D,
                        "k_new / v_new must be [batch, kv_heads, N_new, dim_head], got ", k_new->sizes(), " and ", v_new->sizes());
    }
    k.new_len = ragged ? 1 : k_new->size(2);
    k.kn = prep(*k_new);
    k.vn = prep(*v_new);
  }
  if (c.cache_seqlens.has_value()) {
    const Tensor& cache_seqlens = *c.cache_seqlens;
    same_dev("cache_seqlens", cache_seqlens);
    TORCH_CHECK_TYPE(cache_seqlens.scalar_type() == at::kInt, "cache_seqlens must be int32");
    TORCH_CHECK_VALUE(cache_seqlens.dim() == 1 && cache_seqlens.size(0) == B, "cache_seqlens must be [batch]");
    k.sl = cache_seqlens.contiguous();
  }
  TORCH_CHECK_VALUE(c.max_seqlen_k >= 0, "max_seqlen_k must be non-negative");
  if (c.fp8()) {
    // float32 [], [Hk] or [B, Hk] on q's device
    for (const auto& [name, t] : {std::pair<const char*, const Tensor*>{"k_scale", c.k_scale}, {"v_scale", c.v_scale}}) {
      same_dev(name, *t);
      TORCH_CHECK_TYPE(t->scalar_type() == at::kFloat, name, " must be float32");
      const bool ok = t->dim() == 0 || (t->dim() == 1 && t->size(0) == Hk) || (t->dim() == 2 && t->size(0) == B && t->size(1) == Hk);
      TORCH_CHECK_VALUE(ok, name, " must have shape [], [", Hk, "] or [", B, ", ", Hk, "], got ", t->sizes());
    }
  }
  k.q = prep(q);
  return k;
}

// What one call hands to the library: the structs of include/fcsa.h, filled from the call and its canonical tensors.
struct LibCall {
  fcsa_forward_args a; fcsa_kvcache kv; fcsa_varlen seqs; fcsa_lse_out lo;
  fcsa_kvcache_quant qz; fcsa_tree_mask tree; fcsa_alibi alibi;
  const fcsa_window* win; const fcsa_kvcache_step* step;
  bool ragged, fp8;
  const fcsa_kvcache_quant* quant() const { return fp8 ? &qz : nullptr; }
};

// everything but the workspace and the lse, which kvcache_call allocates once the entry point has sized the former
void fill_lib_call(LibCall& l, const CacheCall& c, const CacheKeep& k, const Tensor& o) {
  const Layout ql = c.ragged() ? kPacked : kDense;      // of q, o, k_new, v_new and the lse
  std::memset(&l, 0, sizeof(l));
  l.ragged = c.ragged(); l.fp8 = c.fp8(); l.win = c.win;
  l.step = c.route == Route::Step || c.route == Route::Alibi ? &c.step : nullptr;
  fcsa_problem& p = l.a.p;
  p.dtype = dtype_code(c.q.scalar_type());
  p.batch = (int32_t)k.B; p.heads = (int32_t)k.H; p.kv_heads = (int32_t)k.Hk;
  p.q_len = (int32_t)(l.ragged ? c.max_seqlen_q : k.N); p.k_len = (int32_t)std::min<int64_t>(c.max_seqlen_k, k.g.capacity); p.dim_head = (int32_t)k.D;
  p.causal = c.causal; p.bias_batch_dim = 0; p.l2norm_qk = c.l2norm_qk;
  p.groups = c.l2norm_qk ? (int32_t)c.groups : 1;
  p.scale = (float)c.scale;
  l.a.q = strided(k.q, ql); l.a.o = strided(o, ql); l.a.stream = stream_of(c.q);
  l.kv.k_cache = strided(c.k_cache); l.kv.v_cache = strided(c.v_cache);
  k.g.fill(l.kv);
  l.kv.new_len = (int32_t)k.new_len;
  l.kv.cache_seqlens = k.sl.defined() ? k.sl.data_ptr<int32_t>() : nullptr;
  if (k.kn.defined() && k.new_len > 0) { l.kv.k_new = strided(k.kn, ql); l.kv.v_new = strided(k.vn, ql); }
  if (l.ragged) { l.seqs.cu_seqlens_q = k.cu.data_ptr<int32_t>(); l.seqs.total_q = k.N; }
  if (l.fp8) {      // float32 [], [Hk] or [B, Hk]: element strides of (batch, K/V head), 0 where the scale broadcasts
    const Tensor &ks = *c.k_scale, &vs = *c.v_scale;
    l.qz = {FCSA_CACHE_E4M3, ks.data_ptr<float>(), vs.data_ptr<float>(), ks.dim() == 2 ? ks.stride(0) : 0, ks.dim() >= 1 ? ks.stride(-1) : 0,
            vs.dim() == 2 ? vs.stride(0) : 0, vs.dim() >= 1 ? vs.stride(-1) : 0};
  }
  if (k.words.defined()) l.tree.mask = reinterpret_cast<const uint64_t*>(k.words.data_ptr<int64_t>());
  if (k.slopes.defined()) {
    l.alibi.slopes = k.slopes.data_ptr<float>();
    l.alibi.stride_b = k.slopes.dim() == 2 ? k.slopes.stride(0) : 0;
    l.alibi.stride_h = k.slopes.stride(-1);
  }
}

// The entry points of the family, one row each: the symbol (as errors name it), who asks for it when the loaded library lacks it, whether
// the library has it, the workspace it needs and the call itself.  The one place that knows which C function serves which call.
struct EntryPoint {
  const char *symbol, *who;
  bool (*present)();
  size_t (*workspace)(const LibCall&);      // null: that of the call without the lse
  int (*run)(const LibCall&);
};
enum Entry { kKvcache, kWindow, kQuant, kVarlen, kLse, kPrefill, kStep, kTree, kAlibi };
const EntryPoint kEntries[] = {
    /* kKvcache */ {"fcsa_forward_kvcache", "flash_cosine_sim_attention_with_kvcache",
                    [] { return g_abi.forward_kvcache != nullptr && g_abi.forward_kvcache_ws != nullptr; },
                    [](const LibCall& l) { return g_abi.forward_kvcache_ws(&l.a.p, &l.kv); },
                    [](const LibCall& l) { return g_abi.forward_kvcache(&l.a, &l.kv); }},
    /* kWindow */ {"fcsa_forward_kvcache_window", "sliding window",
                   [] { return g_abi.forward_kvcache_window != nullptr && g_abi.forward_kvcache_window_ws != nullptr; },
                   [](const LibCall& l) { return g_abi.forward_kvcache_window_ws(&l.a.p, &l.kv, l.win); },
                   [](const LibCall& l) { return g_abi.forward_kvcache_window(&l.a, &l.kv, l.win); }},
    /* kQuant */ {"fcsa_forward_kvcache_quant", "flash_cosine_sim_attention_with_kvcache",
                  [] { return g_abi.forward_kvcache_quant != nullptr && g_abi.forward_kvcache_quant_ws != nullptr; },
                  [](const LibCall& l) { return g_abi.forward_kvcache_quant_ws(&l.a.p, &l.kv, &l.qz, l.win); },
                  [](const LibCall& l) { return g_abi.forward_kvcache_quant(&l.a, &l.kv, &l.qz, l.win); }},
    /* kVarlen */ {"fcsa_forward_kvcache_varlen", "flash_cosine_sim_attention_varlen_with_kvcache",
                   [] { return g_abi.forward_kvcache_varlen != nullptr && g_abi.forward_kvcache_varlen_ws != nullptr; },
                   [](const LibCall& l) { return g_abi.forward_kvcache_varlen_ws(&l.a.p, &l.kv, &l.seqs, l.quant(), l.win); },
                   [](const LibCall& l) { return g_abi.forward_kvcache_varlen(&l.a, &l.kv, &l.seqs, l.quant(), l.win); }},
    /* kLse: every Plain call with the lse */ {"fcsa_forward_kvcache_lse", "return_lse", [] { return g_abi.forward_kvcache_lse != nullptr; }, nullptr,
     [](const LibCall& l) { return g_abi.forward_kvcache_lse(&l.a, &l.kv, l.ragged ? &l.seqs : nullptr, l.quant(), l.win, &l.lo); }},
    /* kPrefill: no workspace */ {"fcsa_forward_kvcache_prefill", "flash_cosine_sim_attention_prefill_with_kvcache",
     [] { return g_abi.forward_kvcache_prefill != nullptr; },
     [](const LibCall&) { return (size_t)0; }, [](const LibCall& l) { return g_abi.forward_kvcache_prefill(&l.a, &l.kv, &l.seqs, &l.lo); }},
    /* kStep */ {"fcsa_forward_kvcache_step", "flash_cosine_sim_attention_step_with_kvcache",
                 [] { return g_abi.forward_kvcache_step != nullptr && g_abi.forward_kvcache_step_ws != nullptr; },
                 [](const LibCall& l) { return g_abi.forward_kvcache_step_ws(&l.a.p, &l.kv, &l.seqs, l.quant(), l.win, l.step); },
                 [](const LibCall& l) { return g_abi.forward_kvcache_step(&l.a, &l.kv, &l.seqs, l.quant(), l.win, l.step, &l.lo); }},
    /* kTree: the ragged call's workspace */ {"fcsa_forward_kvcache_tree", "tree_mask", [] { return g_abi.forward_kvcache_tree != nullptr; },
     [](const LibCall& l) { return g_abi.forward_kvcache_varlen_ws(&l.a.p, &l.kv, &l.seqs, l.quant(), l.win); },
     [](const LibCall& l) { return g_abi.forward_kvcache_tree(&l.a, &l.kv, &l.seqs, l.quant(), &l.tree, &l.lo); }},
    /* kAlibi: the step's workspace */ {"fcsa_forward_kvcache_alibi", "alibi_slopes", [] { return g_abi.forward_kvcache_alibi != nullptr; },
     [](const LibCall& l) { return g_abi.forward_kvcache_step_ws(&l.a.p, &l.kv, &l.seqs, l.quant(), l.win, l.step); },
     [](const LibCall& l) { return g_abi.forward_kvcache_alibi(&l.a, &l.kv, &l.seqs, l.quant(), l.win, l.step, &l.alibi, &l.lo); }},
};

// the entry point of a Plain call without the lse: by the ragged / fp8 / window facts
Entry plain_entry(const CacheCall& c) { return c.ragged() ? kVarlen : c.fp8() ? kQuant : c.win != nullptr ? kWindow : kKvcache; }
constexpr Entry kOfRoute[] = {kKvcache /* Plain: by the facts instead */, kPrefill, kStep, kTree, kAlibi};      // in Route's order
static_assert(sizeof(kEntries) / sizeof(kEntries[0]) == kAlibi + 1 && sizeof(kOfRoute) / sizeof(kOfRoute[0]) == (int)Route::Alibi + 1,
              "kEntries has one row per Entry, in its order, and kOfRoute one entry per Route");
Entry entry_of(const CacheCall& c) { return c.route != Route::Plain ? kOfRoute[(int)c.route] : c.lse ? kLse : plain_entry(c); }
// a call needs its own entry point and those of the calls it is built on
void need_entries(const CacheCall& c, Entry own) {
  auto need = [](Entry e) { need_abi(kEntries[e].who, kEntries[e].symbol, kEntries[e].present()); };
  if (c.route != Route::Plain) need(own);
  if (c.lse) need(kLse);
  if (c.ragged()) need(kVarlen);
  need(kKvcache);
  if (c.fp8()) need(kQuant);
  need(own);
}

// (o, lse): lse float32 [B, H, N], or [total_q, H] for a ragged step; undefined unless the call asks for it
std::tuple<Tensor, Tensor> kvcache_call(const CacheCall& c) {
  const Entry own = entry_of(c);
  need_entries(c, own);
  const CacheKeep k = cache_checks(c);
  c10::DeviceGuard guard(c.q.device());
  const auto opts = c.q.options();
  Tensor o = c.ragged() ? at::empty({k.N, k.H, k.D}, opts) : at::empty({k.B, k.H, k.N, k.D}, opts);
  LibCall l;
  fill_lib_call(l, c, k, o);
  const EntryPoint& e = kEntries[own];
  const size_t wsb = (e.workspace != nullptr ? e : kEntries[plain_entry(c)]).workspace(l);
  Tensor ws, lse;
  if (wsb > 0) {
    ws = at::empty({(int64_t)wsb}, opts.dtype(at::kByte));      // the caching allocator
    l.a.workspace = ws.data_ptr(); l.a.workspace_bytes = wsb;
  }
  if (c.lse) {
    lse = c.ragged() ? at::empty({k.N, k.H}, opts.dtype(at::kFloat)) : at::empty({k.B, k.H, k.N}, opts.dtype(at::kFloat));
    l.lo = strided<fcsa_lse_out>(lse, c.ragged() ? kPacked : kDense);
  }
  check(e.run(l), e.symbol);
  return {o, lse};
}

Tensor kvcache_forward(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const optional<Tensor>& k_new, const optional<Tensor>& v_new,
                       const optional<Tensor>& cache_seqlens, const optional<Tensor>& block_table, int64_t max_seqlen_k, double scale, bool causal,
                       bool l2norm_qk, int64_t groups) {
  return std::get<0>(kvcache_call({q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, max_seqlen_k, scale, causal, l2norm_qk, groups}));
}
Tensor kvcache_window_forward(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const optional<Tensor>& k_new,
                              const optional<Tensor>& v_new, const optional<Tensor>& cache_seqlens, const optional<Tensor>& block_table,
                              int64_t max_seqlen_k, double scale, bool causal, bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
  const Win win(left, right);      // this op takes its sides as they are: (-1, -1) is a window too
  CacheCall c{q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, max_seqlen_k, scale, causal, l2norm_qk, groups};
  c.win = &win.w;
  return std::get<0>(kvcache_call(c));
}

// an e4m3fn cache: window sides of (-1, -1) are the un-windowed call
Tensor kvcache_fp8_forward(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const optional<Tensor>& k_new, const optional<Tensor>& v_new,
                           const optional<Tensor>& cache_seqlens, const optional<Tensor>& block_table, const Tensor& k_scale, const Tensor& v_scale,
                           int64_t max_seqlen_k, double scale, bool causal, bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
  const OptWin win(left, right);
  CacheCall c{q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, max_seqlen_k, scale, causal, l2norm_qk, groups};
  c.win = win.ptr(); c.k_scale = &k_scale; c.v_scale = &v_scale;
  return std::get<0>(kvcache_call(c));
}

// a ragged step: packed q [total_q, H, D] with cu_seqlens_q [B + 1]; k_scale / v_scale given: an e4m3fn cache (its codes as uint8 tensors);
// window sides of (-1, -1): no window
Tensor kvcache_varlen_forward(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const Tensor& cu_seqlens_q, const optional<Tensor>& k_new,
                              const optional<Tensor>& v_new, const optional<Tensor>& cache_seqlens, const optional<Tensor>& block_table,
                              const optional<Tensor>& k_scale, const optional<Tensor>& v_scale, int64_t max_seqlen_q, int64_t max_seqlen_k, double scale,
                              bool causal, bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
  CacheCall c{q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, max_seqlen_k, scale, causal, l2norm_qk, groups};
  set_scales(c, k_scale, v_scale);
  const OptWin win(left, right);
  c.win = win.ptr(); c.cu_q = &cu_seqlens_q; c.max_seqlen_q = max_seqlen_q;
  return std::get<0>(kvcache_call(c));
}

// Every decode route with the rows' log-sum-exp as a second result (return_lse=True): cu_seqlens_q given: a ragged step; k_scale / v_scale
// given: an e4m3fn cache (its codes as uint8 tensors); window sides of (-1, -1): no window.  o and the caches are what the op of that
// route gives, bit for bit; lse is float32 [B, H, N] ([total_q, H] for a ragged step).
std::tuple<Tensor, Tensor> kvcache_lse_forward(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const optional<Tensor>& cu_seqlens_q,
                                               const optional<Tensor>& k_new, const optional<Tensor>& v_new, const optional<Tensor>& cache_seqlens,
                                               const optional<Tensor>& block_table, const optional<Tensor>& k_scale, const optional<Tensor>& v_scale,
                                               int64_t max_seqlen_q, int64_t max_seqlen_k, double scale, bool causal, bool l2norm_qk, int64_t groups,
                                               int64_t left, int64_t right) {
  CacheCall c{q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, max_seqlen_k, scale, causal, l2norm_qk, groups};
  set_scales(c, k_scale, v_scale);
  const OptWin win(left, right);
  c.win = win.ptr(); c.cu_q = ptr(cu_seqlens_q); c.max_seqlen_q = max_seqlen_q; c.lse = true;
  return kvcache_call(c);
}

// A prompt chunk against the cache on the multi-wave prefill kernel: kvcache_lse_forward's ragged step without scales and window sides.
// f16 / bf16 and D = 64 / 128 only (the library refuses the rest).
std::tuple<Tensor, Tensor> kvcache_prefill_forward(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const Tensor& cu_seqlens_q,
                                                   const optional<Tensor>& k_new, const optional<Tensor>& v_new, const optional<Tensor>& cache_seqlens,
                                                   const optional<Tensor>& block_table, int64_t max_seqlen_q, int64_t max_seqlen_k, double scale,
                                                   bool causal, bool l2norm_qk, int64_t groups) {
  CacheCall c{q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, max_seqlen_k, scale, causal, l2norm_qk, groups};
  c.cu_q = &cu_seqlens_q; c.max_seqlen_q = max_seqlen_q; c.lse = true; c.route = Route::Prefill;
  return kvcache_call(c);
}

// An engine step: kvcache_lse_forward's ragged step with the routing fields of fcsa_kvcache_step.  slopes given (kvcache_alibi_forward): the
// step with a linear position bias (float32 [H] or [B, H] on q's device, never read on the host), through fcsa_forward_kvcache_alibi.
// c: the call with the members every op has.
std::tuple<Tensor, Tensor> step_call(CacheCall c, const Tensor* slopes, const Tensor& cu_seqlens_q, const optional<Tensor>& k_scale,
                                     const optional<Tensor>& v_scale, int64_t max_seqlen_q, int64_t left, int64_t right, int64_t chunk_rows,
                                     int64_t max_decode_tokens, bool no_decode, bool no_chunk) {
  set_scales(c, k_scale, v_scale);
  c.step = step_fields(chunk_rows, max_decode_tokens, no_decode, no_chunk);
  const OptWin win(left, right);
  c.win = win.ptr(); c.cu_q = &cu_seqlens_q; c.max_seqlen_q = max_seqlen_q; c.lse = true;
  c.route = slopes != nullptr ? Route::Alibi : Route::Step; c.extra = slopes;
  return kvcache_call(c);
}
std::tuple<Tensor, Tensor> kvcache_step_forward(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const Tensor& cu_seqlens_q,
                                                const optional<Tensor>& k_new, const optional<Tensor>& v_new, const optional<Tensor>& cache_seqlens,
                                                const optional<Tensor>& block_table, const optional<Tensor>& k_scale, const optional<Tensor>& v_scale,
                                                int64_t max_seqlen_q, int64_t max_seqlen_k, double scale, bool causal, bool l2norm_qk, int64_t groups,
                                                int64_t left, int64_t right, int64_t chunk_rows, int64_t max_decode_tokens, bool no_decode,
                                                bool no_chunk) {
  return step_call({q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, max_seqlen_k, scale, causal, l2norm_qk, groups}, nullptr,
                   cu_seqlens_q, k_scale, v_scale, max_seqlen_q, left, right, chunk_rows, max_decode_tokens, no_decode, no_chunk);
}
std::tuple<Tensor, Tensor> kvcache_alibi_forward(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const Tensor& cu_seqlens_q,
                                                 const Tensor& alibi_slopes, const optional<Tensor>& k_new, const optional<Tensor>& v_new,
                                                 const optional<Tensor>& cache_seqlens, const optional<Tensor>& block_table,
                                                 const optional<Tensor>& k_scale, const optional<Tensor>& v_scale, int64_t max_seqlen_q,
                                                 int64_t max_seqlen_k, double scale, bool causal, bool l2norm_qk, int64_t groups, int64_t left,
                                                 int64_t right, int64_t chunk_rows, int64_t max_decode_tokens, bool no_decode, bool no_chunk) {
  return step_call({q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, max_seqlen_k, scale, causal, l2norm_qk, groups}, &alibi_slopes,
                   cu_seqlens_q, k_scale, v_scale, max_seqlen_q, left, right, chunk_rows, max_decode_tokens, no_decode, no_chunk);
}

// A tree step: kvcache_lse_forward's ragged step without a window and without `causal`, the visibility of the step's own tokens given per
// packed row by tree_mask (int64 [total_q], read as unsigned 64-bit words).
std::tuple<Tensor, Tensor> kvcache_tree_forward(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const Tensor& cu_seqlens_q,
                                                const Tensor& tree_mask, const optional<Tensor>& k_new, const optional<Tensor>& v_new,
                                                const optional<Tensor>& cache_seqlens, const optional<Tensor>& block_table,
                                                const optional<Tensor>& k_scale, const optional<Tensor>& v_scale, int64_t max_seqlen_q,
                                                int64_t max_seqlen_k, double scale, bool l2norm_qk, int64_t groups) {
  CacheCall c{q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, max_seqlen_k, scale, false, l2norm_qk, groups};
  set_scales(c, k_scale, v_scale);
  c.cu_q = &cu_seqlens_q; c.max_seqlen_q = max_seqlen_q; c.lse = true; c.route = Route::Tree; c.extra = &tree_mask;
  return kvcache_call(c);
}

// kvcache_keep_accepted: the rows cache_seqlens[b] + accepted[b, i] of both caches move to cache_seqlens[b] + i (i < num_accepted[b]), in
// place, as bytes (any cache dtype; fp8 codes as their uint8 views).  Tables int32 on the caches' device, never read on the host.
void kvcache_compact(const Tensor& k_cache, const Tensor& v_cache, const Tensor& cache_seqlens, const Tensor& accepted, const Tensor& num_accepted,
                     const optional<Tensor>& block_table) {
  need_abi("kvcache_keep_accepted", "fcsa_kvcache_compact", g_abi.kvcache_compact);
  TORCH_CHECK(k_cache.is_cuda(), "kvcache_keep_accepted: the caches must be GPU tensors (HIP kernels only)");
  auto same_dev = [&](const char* name, const Tensor& t) {
    TORCH_CHECK_VALUE(t.device() == k_cache.device(), name, " is on ", t.device(), " but k_cache is on ", k_cache.device());
  };
  same_dev("v_cache", v_cache);
  TORCH_CHECK_TYPE(k_cache.scalar_type() == v_cache.scalar_type(), "k_cache and v_cache must share a dtype");
  TORCH_CHECK_VALUE(k_cache.dim() == 4 && k_cache.sizes() == v_cache.sizes(), "k_cache and v_cache must have 4 dimensions and the same shape");
  const int64_t es = k_cache.element_size(), D = k_cache.size(3), Hk = k_cache.size(1);
  TORCH_CHECK_TYPE(es == 1 || es == 2 || es == 4, "cache elements of 1, 2 or 4 bytes, got ", k_cache.scalar_type());
  TORCH_CHECK_VALUE(rows_ok(k_cache) && rows_ok(v_cache), "k_cache / v_cache: the feature dim must be contiguous and rows 16-byte aligned "
                    "(the caches are updated in place, so they are not copied)");
  same_dev("cache_seqlens", cache_seqlens);
  same_dev("accepted", accepted);
  same_dev("num_accepted", num_accepted);
  TORCH_CHECK_TYPE(cache_seqlens.scalar_type() == at::kInt && accepted.scalar_type() == at::kInt && num_accepted.scalar_type() == at::kInt,
                   "cache_seqlens, accepted and num_accepted must be int32");
  TORCH_CHECK_VALUE(accepted.dim() == 2 && accepted.size(1) >= 1 && accepted.size(1) <= 64, "accepted must be [sequences, A] with 1 <= A <= 64, got ",
                    accepted.sizes());
  const int64_t B = accepted.size(0);
  TORCH_CHECK_VALUE(cache_seqlens.dim() == 1 && cache_seqlens.size(0) == B && num_accepted.dim() == 1 && num_accepted.size(0) == B,
                    "cache_seqlens and num_accepted must be [", B, "]");
  const Geometry g = cache_geometry(k_cache, block_table, B, same_dev, "sequences", "accepted");
  TORCH_CHECK_VALUE(g.capacity <= INT32_MAX, "cache capacity must stay below 2^31");
  if (B == 0 || Hk == 0 || g.capacity == 0) return;
  c10::DeviceGuard guard(k_cache.device());
  const Tensor sl = cache_seqlens.contiguous(), acc = accepted.stride(1) == 1 ? accepted : accepted.contiguous(), na = num_accepted.contiguous();
  fcsa_kvcache kv;
  std::memset(&kv, 0, sizeof(kv));
  kv.k_cache = strided(k_cache);
  kv.v_cache = strided(v_cache);
  g.fill(kv);
  kv.cache_seqlens = sl.data_ptr<int32_t>();
  check(g_abi.kvcache_compact(&kv, (int32_t)B, (int32_t)Hk, (int32_t)D, (int32_t)es, acc.data_ptr<int32_t>(), acc.stride(0), (int32_t)acc.size(1),
                              na.data_ptr<int32_t>(), stream_of(k_cache)),
        "fcsa_kvcache_compact");
}

// merge_attention_states: S <= 8 states (o_s [..., D] 4-D or [total_q, H, D], lse_s float32 without the feature dim) -> fresh contiguous
// (o, lse).  The states are read in place through their strides (feature dim contiguous, rows 16-byte aligned; anything else is copied).
std::tuple<Tensor, Tensor> merge_states(at::TensorList os, at::TensorList lses) {
  need_abi("merge_attention_states", "fcsa_merge_states", g_abi.merge_states);
  const int64_t S = (int64_t)os.size();
  TORCH_CHECK_VALUE(S >= 1 && S <= FCSA_MERGE_MAX_STATES && (int64_t)lses.size() == S,
                    "merge_states takes 1 to ", FCSA_MERGE_MAX_STATES, " states and as many lses, got ", S, " and ", lses.size());
  const Tensor& o0 = os[0];
  TORCH_CHECK(o0.is_cuda(), "merge_states: GPU tensors only (HIP kernels only)");
  TORCH_CHECK_VALUE(o0.dim() == 3 || o0.dim() == 4, "merge_states: os must be 4-D [..., D] or 3-D [total_q, H, D], got ", o0.sizes());
  const int64_t D = o0.size(-1);
  const int64_t per16 = 16 / o0.element_size();      // rows are whole 16-byte chunks
  TORCH_CHECK_VALUE(D >= per16 && D % per16 == 0, "merge_states: the feature dim (", D, ") must be a positive multiple of ", per16);
  c10::DeviceGuard guard(o0.device());
  fcsa_merge_args a;
  std::memset(&a, 0, sizeof(a));
  a.dtype = dtype_code(o0.scalar_type());
  const Layout l = o0.dim() == 3 ? kRows3 : kDense;
  for (int64_t d = 0; d + 1 < o0.dim(); ++d) TORCH_CHECK_VALUE(o0.size(d) <= INT32_MAX, "merge_states: sizes must stay below 2^31");
  a.size0 = l.batch < 0 ? 1 : (int32_t)o0.size(l.batch);
  a.size1 = (int32_t)o0.size(l.head);
  a.size2 = (int32_t)o0.size(l.pos);
  a.dim_head = (int32_t)D;
  a.states = (int32_t)S;
  std::vector<Tensor> keep;
  keep.reserve((size_t)S);
  const auto lead = o0.sizes().slice(0, o0.dim() - 1);
  for (int64_t s = 0; s < S; ++s) {
    const Tensor& o = os[s];
    const Tensor& ls = lses[s];
    TORCH_CHECK_VALUE(o.device() == o0.device() && ls.device() == o0.device(), "merge_states: every tensor must live on the first one's GPU");
    TORCH_CHECK_TYPE(o.scalar_type() == o0.scalar_type(), "merge_states: os must share a dtype, got ", o0.scalar_type(), " and ", o.scalar_type());
    TORCH_CHECK_VALUE(o.sizes() == o0.sizes(), "merge_states: os must share a shape, got ", o0.sizes(), " and ", o.sizes());
    TORCH_CHECK_TYPE(ls.scalar_type() == at::kFloat, "merge_states: lses must be float32, got ", ls.scalar_type());
    TORCH_CHECK_VALUE(ls.sizes() == lead, "merge_states: an lse must have its o's shape without the feature dim, ", lead, ", got ", ls.sizes());
    keep.push_back(prep(o));
    a.o_in[s] = strided(keep.back(), l);
    a.lse_in[s] = strided<fcsa_lse_out>(ls, l);
  }
  Tensor o = at::empty(o0.sizes(), o0.options());
  Tensor lse = at::empty(lead, o0.options().dtype(at::kFloat));
  a.o = strided(o, l);
  a.lse = strided<fcsa_lse_out>(lse, l);
  a.stream = stream_of(o0);
  if (o.numel() > 0) check(g_abi.merge_states(&a), "fcsa_merge_states");
  return {o, lse};
}

// ---- attention states for training (namespace fcsa_state): the forward's log-sum-exp as a second differentiable result, and a
// differentiable merge.  One op family serves the dense, the local and the packed operator: cu_seqlens given: packed q [total_q, H, D];
// window sides of (-1, -1): no window.  o, the saved state and -- with no gradient for the lse -- dq, dk, dv are those of the op of that
// route, bit for bit: the same forward_body / backward_body, the same launches.
// (o, lse, inv_l, qn, kn, rq, rk): lse float32 [B, H, N], packed [total_q, H].  The saved state is always produced: the lse is read off inv_l.
using StateSaved = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>;

// The slopes of a linear position bias in training (alibi_train ops): float32 [H] or [B, H] (B: batch, packed: sequences) on q's device,
// any strides, never read on the host.  There is no slope gradient.
struct TrainSlopes {
  fcsa_alibi a{};
  TrainSlopes(const Call& c, const Tensor& slopes) {
    need_abi("flash_cosine_sim_attention_alibi", "fcsa_forward_alibi / fcsa_backward_alibi", g_abi.forward_alibi, g_abi.backward_alibi, g_abi.backward_alibi_ws);
    TORCH_CHECK_TYPE(slopes.scalar_type() == at::kFloat, "alibi_slopes must be float32, got ", slopes.scalar_type());
    TORCH_CHECK_VALUE(slopes.device() == c.q.device(), "alibi_slopes is on ", slopes.device(), " but q is on ", c.q.device(),
                      ": all tensors must live on q's GPU");
    const int64_t H = c.p.heads, B = c.p.batch;
    TORCH_CHECK_VALUE((slopes.dim() == 1 && slopes.size(0) == H) || (slopes.dim() == 2 && slopes.size(0) == B && slopes.size(1) == H),
                      "alibi_slopes must be [heads] (", H, ") or [", c.packed() ? "sequences" : "batch", ", heads] (", B, ", ", H, "), got ", slopes.sizes());
    TORCH_CHECK_VALUE(c.packed() || c.p.causal || c.p.q_len <= c.p.k_len, "alibi_slopes: a non-causal call needs q_len <= k_len, got ", c.p.q_len,
                      " > ", c.p.k_len, " (rows with a negative position have no key at distance 0)");
    a.slopes = slopes.numel() > 0 ? slopes.data_ptr<float>() : nullptr;
    a.stride_b = slopes.dim() == 2 ? slopes.stride(0) : 0;
    a.stride_h = slopes.stride(-1);
    a.reserved = 0;
  }
};

// The call of the ops that take dense or packed q, k, v with an optional window and optional slopes (attention_state, alibi_train): the
// window's checks, then the tensors', then the slopes'.
Call option_call(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& cu_q, const optional<Tensor>& cu_k, int64_t max_q,
                 int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups, int64_t left, int64_t right, const Tensor* slopes) {
  const OptWin win(left, right);
  TORCH_CHECK_VALUE(cu_q.has_value() == cu_k.has_value(), "cu_seqlens_q and cu_seqlens_k must be given together");
  TORCH_CHECK_VALUE(cu_q.has_value() || (q.dim() == 4 && k.dim() == 4 && v.dim() == 4),
                    "attention_state takes 4-D q, k, v, or packed 3-D ones with cu_seqlens");
  Call c = cu_q.has_value() ? canonicalise_varlen(q, k, v, *cu_q, *cu_k, max_q, max_k, scale, causal, l2norm_qk, groups)
                            : canonicalise(q, k, v, c10::nullopt, c10::nullopt, false, scale, causal, l2norm_qk, groups);
  c.win = win.w;
  if (slopes != nullptr) c.alibi = TrainSlopes(c, *slopes).a;
  return c;
}

StateSaved attention_state_forward(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& cu_q, const optional<Tensor>& cu_k,
                                   int64_t max_q, int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups, int64_t left,
                                   int64_t right) {
  need_abi("attention_state", "fcsa_attention_lse", g_abi.attention_lse);
  const Call c = option_call(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, left, right, nullptr);
  Lap lap(false);
  auto [o, inv_l, qn, kn, rq, rk] = forward_body(c, true, lap);
  c10::DeviceGuard guard(c.q.device());
  const auto f32 = c.q.options().dtype(at::kFloat);
  Tensor lse = c.packed() ? at::empty({c.q.size(0), c.q.size(1)}, f32) : at::empty(c.rows_q, f32);
  if (lse.numel() > 0) {
    // Which normaliser the lse is read off.  The 16-bit forward's row sum adds the P~ values ROUNDED to the type, so
    // ln(l) carries up to one unit roundoff u of the type.  With l2norm_qk the rounding of the operands c1 q^, k^ already moves every logit
    // by up to 2 u |scale| groups, and the row sum's u disappears in that.  Where it does not -- the caller's q, k ARE the operands
    // (l2norm_qk off), or |scale| groups < 1/2 -- the lse is taken from the inv_l of a second, float32 forward on the same values: float32
    // row sums of un-rounded P~.  o, the saved state and every gradient stay those of the 16-bit call.
    const bool exact = c.p.dtype != FCSA_F32 && (c.p.l2norm_qk == 0 || 2.0 * std::fabs(scale) * (double)c.p.groups < 1.0);
    Call c32;
    Tensor inv_l32;
    if (exact) {
      c32 = option_call(q.to(at::kFloat), k.to(at::kFloat), v.to(at::kFloat), cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, left, right,
                        nullptr);
      Lap lap32(false);
      inv_l32 = std::get<1>(forward_body(c32, true, lap32));
    }
    const Call& lc = exact ? c32 : c;
    const fcsa_lse_out lo = strided<fcsa_lse_out>(lse, c.layout());
    check(g_abi.attention_lse(&lc.p, (exact ? inv_l32 : inv_l).data_ptr<float>(), c.seqs(), c.window(), &lo, stream_of(c.q)), "fcsa_attention_lse");
  }
  return std::make_tuple(o, lse, inv_l, qn, kn, rq, rk);
}

// d_out / d_lse: the gradients of o / lse; an absent d_out is zeros, an absent d_lse runs the backward of the op without the lse, bit for bit
Grads3 attention_state_backward(const optional<Tensor>& d_out, const optional<Tensor>& d_lse, const Tensor& o, const Tensor& inv_l, const Tensor& q,
                                const Tensor& k, const Tensor& v, const optional<Tensor>& cu_q, const optional<Tensor>& cu_k, const Tensor& qn,
                                const Tensor& kn, const Tensor& rq, const Tensor& rk, int64_t max_q, int64_t max_k, double scale, bool causal,
                                bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
  Call c = option_call(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, left, right, nullptr);
  c.d_lse = ptr(d_lse);
  Lap lap(false);
  const Tensor go = d_out.has_value() ? *d_out : at::zeros_like(o);
  return first3(backward_body(c, go, o, inv_l, qn, kn, rq, rk, false, lap));
}

using StateScalars = std::tuple<int64_t, int64_t, double, bool, bool, int64_t, int64_t, int64_t>;   // max_q, max_k, scale, causal, l2norm_qk, groups, left, right

struct AttentionStateNode : public torch::autograd::Function<AttentionStateNode> {
  static variable_list forward(AutogradContext* ctx, const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& cu_q,
                               const optional<Tensor>& cu_k, const StateScalars& s) {
    ctx->set_materialize_grads(false);      // an absent gradient stays absent: no lse gradient -> the existing backward, bit for bit
    at::AutoDispatchBelowADInplaceOrView guard;
    static auto op = typed_op("fcsa_state::attention_state_forward", &attention_state_forward);
    auto r = std::apply([&](const auto&... e) { return op.call(q, k, v, cu_q, cu_k, e...); }, s);
    ctx->save_for_backward({std::get<0>(r), std::get<2>(r), q, k, v, std::get<3>(r), std::get<4>(r), std::get<5>(r), std::get<6>(r),
                            saveable(cu_q), saveable(cu_k)});
    ctx->saved_data["scalars"] = c10::IValue(s);
    return {std::get<0>(r), std::get<1>(r)};
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto t = ctx->get_saved_variables();      // o, inv_l, q, k, v, qn, kn, rq, rk, cu_q, cu_k
    const StateScalars s = ctx->saved_data["scalars"].to<StateScalars>();
    static auto op = typed_op("fcsa_state::attention_state_backward", &attention_state_backward);
    const optional<Tensor> go = restored<optional<Tensor>>(grads[0]), gl = restored<optional<Tensor>>(grads[1]);
    const optional<Tensor> cu_q = restored<optional<Tensor>>(t[9]), cu_k = restored<optional<Tensor>>(t[10]);
    auto g = std::apply([&](const auto&... e) { return op.call(go, gl, t[0], t[1], t[2], t[3], t[4], cu_q, cu_k, t[5], t[6], t[7], t[8], e...); }, s);
    return {std::get<0>(g), std::get<1>(g), std::get<2>(g), Tensor(), Tensor(), Tensor()};
  }
};

std::tuple<Tensor, Tensor> attention_state_plain(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& cu_q,
                                                 const optional<Tensor>& cu_k, int64_t max_q, int64_t max_k, double scale, bool causal,
                                                 bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
  auto r = attention_state_forward(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, left, right);
  return {std::get<0>(r), std::get<1>(r)};
}
std::tuple<Tensor, Tensor> attention_state_autograd(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& cu_q,
                                                    const optional<Tensor>& cu_k, int64_t max_q, int64_t max_k, double scale, bool causal,
                                                    bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
  if (!(at::GradMode::is_enabled() && (q.requires_grad() || k.requires_grad() || v.requires_grad()))) {
    at::AutoDispatchBelowADInplaceOrView guard;
    return attention_state_plain(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, left, right);
  }
  auto r = AttentionStateNode::apply(q, k, v, cu_q, cu_k, StateScalars{max_q, max_k, scale, causal, l2norm_qk, groups, left, right});
  return {r[0], r[1]};
}

// ---- a linear position bias in training (namespace fcsa_alibi_train): one op family for the dense, the local and the packed operator, as
// attention_state is -- cu_seqlens given: packed q [total_q, H, D]; window sides of (-1, -1): no window -- through the same option_call /
// forward_body / backward_body, with the slopes (TrainSlopes) handed to fcsa_forward_alibi / fcsa_backward_alibi.
Saved alibi_train_forward(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& alibi_slopes, const optional<Tensor>& cu_q,
                          const optional<Tensor>& cu_k, int64_t max_q, int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups,
                          int64_t left, int64_t right, bool need_backward) {
  Lap lap(false);
  return forward_body(option_call(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, left, right, &alibi_slopes), need_backward, lap);
}
Grads3 alibi_train_backward(const Tensor& d_out, const Tensor& o, const Tensor& inv_l, const Tensor& q, const Tensor& k, const Tensor& v,
                            const Tensor& alibi_slopes, const optional<Tensor>& cu_q, const optional<Tensor>& cu_k, const Tensor& qn,
                            const Tensor& kn, const Tensor& rq, const Tensor& rk, int64_t max_q, int64_t max_k, double scale, bool causal,
                            bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
  Lap lap(false);
  return first3(backward_body(option_call(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, left, right, &alibi_slopes), d_out, o,
                              inv_l, qn, kn, rq, rk, false, lap));
}

// the family's node is AttentionNode: need_backward is true whenever it runs, and there is no bias gradient
struct AlibiTrainOps {
  static constexpr const char* forward_name = "fcsa_alibi_train::forward";
  static constexpr const char* backward_name = "fcsa_alibi_train::backward";
  static constexpr auto fwd = &alibi_train_forward;
  static constexpr auto bwd = &alibi_train_backward;
  using Extra = std::tuple<Tensor, optional<Tensor>, optional<Tensor>>;      // alibi_slopes, cu_seqlens_q, cu_seqlens_k
  using Scalars = StateScalars;
  using Window = std::tuple<>;
  static constexpr bool bias_grad = false;
};

Tensor alibi_train_attention_plain(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& alibi_slopes, const optional<Tensor>& cu_q,
                                   const optional<Tensor>& cu_k, int64_t max_q, int64_t max_k, double scale, bool causal, bool l2norm_qk,
                                   int64_t groups, int64_t left, int64_t right) {
  return std::get<0>(alibi_train_forward(q, k, v, alibi_slopes, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, left, right, false));
}
Tensor alibi_train_attention_autograd(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& alibi_slopes, const optional<Tensor>& cu_q,
                                      const optional<Tensor>& cu_k, int64_t max_q, int64_t max_k, double scale, bool causal, bool l2norm_qk,
                                      int64_t groups, int64_t left, int64_t right) {
  TORCH_CHECK_VALUE(!alibi_slopes.requires_grad(), "alibi_slopes must not require grad: there is no slope gradient (fixed slopes only)");
  if (!(at::GradMode::is_enabled() && (q.requires_grad() || k.requires_grad() || v.requires_grad()))) {
    at::AutoDispatchBelowADInplaceOrView guard;      // (through the dispatcher again, below autograd: fake tensors reach the fake kernel)
    static auto op = typed_op("fcsa_alibi_train::attention", &alibi_train_attention_plain);
    return op.call(q, k, v, alibi_slopes, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, left, right);
  }
  return AttentionNode<AlibiTrainOps>::apply(q, k, v, optional<Tensor>(), AlibiTrainOps::Extra{alibi_slopes, cu_q, cu_k},
                                             StateScalars{max_q, max_k, scale, causal, l2norm_qk, groups, left, right}, AlibiTrainOps::Window{});
}

// merge_state: merge_states (the same function: the forward kernel, bit for bit) with a backward.
// merge_state_backward: (d_o?, d_lse?, os, lses) -> (d_os, d_lses); an absent d_o is zeros, an absent d_lse is no gradient for the lse.
std::tuple<std::vector<Tensor>, std::vector<Tensor>> merge_state_backward(const optional<Tensor>& d_o, const optional<Tensor>& d_lse, at::TensorList os,
                                                                          at::TensorList lses) {
  need_abi("merge_attention_states_with_grad", "fcsa_merge_states_backward", g_abi.merge_states_backward);
  const int64_t S = (int64_t)os.size();
  TORCH_CHECK_VALUE(S >= 1 && S <= FCSA_MERGE_MAX_STATES && (int64_t)lses.size() == S,
                    "merge_state_backward takes 1 to ", FCSA_MERGE_MAX_STATES, " states and as many lses, got ", S, " and ", lses.size());
  const Tensor& o0 = os[0];
  TORCH_CHECK(o0.is_cuda(), "merge_state_backward: GPU tensors only (HIP kernels only)");
  TORCH_CHECK_VALUE(o0.dim() == 3 || o0.dim() == 4, "merge_state_backward: os must be 4-D [..., D] or 3-D [total_q, H, D], got ", o0.sizes());
  const int64_t D = o0.size(-1);
  const int64_t per16 = 16 / o0.element_size();
  TORCH_CHECK_VALUE(D >= per16 && D % per16 == 0, "merge_state_backward: the feature dim (", D, ") must be a positive multiple of ", per16);
  c10::DeviceGuard guard(o0.device());
  fcsa_merge_backward_args a;
  std::memset(&a, 0, sizeof(a));
  a.dtype = dtype_code(o0.scalar_type());
  const Layout l = o0.dim() == 3 ? kRows3 : kDense;
  for (int64_t d = 0; d + 1 < o0.dim(); ++d) TORCH_CHECK_VALUE(o0.size(d) <= INT32_MAX, "merge_state_backward: sizes must stay below 2^31");
  a.size0 = l.batch < 0 ? 1 : (int32_t)o0.size(l.batch);
  a.size1 = (int32_t)o0.size(l.head);
  a.size2 = (int32_t)o0.size(l.pos);
  a.dim_head = (int32_t)D;
  a.states = (int32_t)S;
  const auto lead = o0.sizes().slice(0, o0.dim() - 1);
  const auto f32 = o0.options().dtype(at::kFloat);
  std::vector<Tensor> keep, d_os, d_lses;
  for (int64_t s = 0; s < S; ++s) {
    const Tensor& o = os[s];
    const Tensor& ls = lses[s];
    TORCH_CHECK_VALUE(o.device() == o0.device() && ls.device() == o0.device(), "merge_state_backward: every tensor must live on the first one's GPU");
    TORCH_CHECK_TYPE(o.scalar_type() == o0.scalar_type() && ls.scalar_type() == at::kFloat, "merge_state_backward: os must share a dtype and lses be float32");
    TORCH_CHECK_VALUE(o.sizes() == o0.sizes() && ls.sizes() == lead, "merge_state_backward: os must share a shape and every lse have it without the feature dim");
    keep.push_back(prep(o));
    d_os.push_back(at::empty(o0.sizes(), o0.options()));
    d_lses.push_back(at::empty(lead, f32));
    a.o_in[s] = strided(keep.back(), l);
    a.lse_in[s] = strided<fcsa_lse_out>(ls, l);
    a.d_o_in[s] = strided(d_os.back(), l);
    a.d_lse_in[s] = strided<fcsa_lse_out>(d_lses.back(), l);
  }
  Tensor go = d_o.has_value() ? *d_o : at::zeros(o0.sizes(), o0.options());
  TORCH_CHECK_VALUE(go.sizes() == o0.sizes() && go.device() == o0.device(), "merge_state_backward: d_o must have the shape of o on its device");
  if (go.scalar_type() != o0.scalar_type()) go = go.to(o0.scalar_type());
  go = prep(go);
  a.d_o = strided(go, l);
  Tensor gl;
  if (d_lse.has_value()) {
    TORCH_CHECK_VALUE(d_lse->sizes() == lead && d_lse->device() == o0.device(), "merge_state_backward: d_lse must have the shape of lse on its device");
    gl = d_lse->to(at::kFloat);
    a.d_lse = strided<fcsa_lse_out>(gl, l);
  }
  a.stream = stream_of(o0);
  if (o0.numel() > 0) check(g_abi.merge_states_backward(&a), "fcsa_merge_states_backward");
  return {d_os, d_lses};
}

struct MergeStateNode : public torch::autograd::Function<MergeStateNode> {
  static variable_list forward(AutogradContext* ctx, at::TensorList os, at::TensorList lses) {
    ctx->set_materialize_grads(false);
    at::AutoDispatchBelowADInplaceOrView guard;
    static auto op = typed_op("fcsa::merge_states", &merge_states);
    auto r = op.call(os, lses);
    variable_list save(os.begin(), os.end());
    save.insert(save.end(), lses.begin(), lses.end());
    ctx->save_for_backward(std::move(save));
    return {std::get<0>(r), std::get<1>(r)};
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto t = ctx->get_saved_variables();      // os..., lses...
    const size_t S = t.size() / 2;
    static auto op = typed_op("fcsa_state::merge_state_backward", &merge_state_backward);
    auto g = op.call(restored<optional<Tensor>>(grads[0]), restored<optional<Tensor>>(grads[1]), at::TensorList(t.data(), S),
                     at::TensorList(t.data() + S, S));
    variable_list out = std::get<0>(g);
    out.insert(out.end(), std::get<1>(g).begin(), std::get<1>(g).end());
    return out;
  }
};

std::tuple<Tensor, Tensor> merge_state_autograd(at::TensorList os, at::TensorList lses) {
  bool tracked = false;
  for (const Tensor& t : os) tracked = tracked || t.requires_grad();
  for (const Tensor& t : lses) tracked = tracked || t.requires_grad();
  if (!(at::GradMode::is_enabled() && tracked)) {
    at::AutoDispatchBelowADInplaceOrView guard;
    return merge_states(os, lses);
  }
  auto r = MergeStateNode::apply(os, lses);
  return {r[0], r[1]};
}

}  // namespace

// Measurement hook: read (and reset) the host-time counters above.
extern "C" void fcsa_torch_host_ns(uint64_t* out8) {
  for (int i = 0; i < 8; ++i) out8[i] = g_host_ns[i].exchange(0, std::memory_order_relaxed);
}

// Measurement hook (not part of the operator surface): route the ops to another build of libfcsa_hip.so.  Returns 0 on success.
extern "C" int fcsa_torch_use_library(const char* path) {
  void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (h == nullptr) return -1;
  Abi a;
  bool complete = true;      // optional entry points stay null where the library lacks them, and only the ops that need them refuse to run
#define X(member, symbol, required)                                     \
  a.member = reinterpret_cast<decltype(a.member)>(dlsym(h, #symbol)); \
  complete = complete && (a.member != nullptr || !(required));
  FCSA_ABI(X)
#undef X
  if (!complete) { dlclose(h); return -2; }
  // Only libraries of THIS ABI: the binding allocates for the struct layouts and buffer contracts of include/fcsa.h as compiled in
  // (e.g. ABI 3 writes d_bias once in the bias dtype into an uninitialised buffer; an ABI-2 library would accumulate float32 into
  // it -- twice the buffer's size for the 16-bit types).  -3: the library reports another version.
  auto dbg = reinterpret_cast<int (*)(char*, size_t)>(dlsym(h, "fcsa_debug"));
  if (!dbg || dbg(nullptr, 0) != FCSA_ABI_VERSION) { dlclose(h); return -3; }
  g_abi = a;
  return 0;
}

TORCH_LIBRARY(fcsa, m) {
  m.def("forward(Tensor q, Tensor k, Tensor v, Tensor? mask, Tensor? attn_bias, bool attn_bias_batch_dim, float scale, bool causal, "
        "bool l2norm_qk, int groups, bool need_backward) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("backward(Tensor d_out, Tensor o, Tensor inv_l, Tensor q, Tensor k, Tensor v, Tensor? mask, Tensor? attn_bias, Tensor qn, Tensor kn, "
        "Tensor rq, Tensor rk, bool attn_bias_batch_dim, float scale, bool causal, bool l2norm_qk, int groups, bool need_bias_grad) "
        "-> (Tensor, Tensor, Tensor, Tensor)");
  // the operator itself: differentiable w.r.t. q, k, v, attn_bias (Autograd kernel below)
  m.def("attention(Tensor q, Tensor k, Tensor v, Tensor? mask, Tensor? attn_bias, bool attn_bias_batch_dim, float scale, bool causal, "
        "bool l2norm_qk, int groups) -> Tensor");
  // packed variable-length sequences (cu_seqlens): q [total_q, H, D], k / v [total_k, Hk, D]
  m.def("varlen_forward(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, int max_seqlen_q, int max_seqlen_k, "
        "float scale, bool causal, bool l2norm_qk, int groups, bool need_backward) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("varlen_backward(Tensor d_out, Tensor o, Tensor inv_l, Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, "
        "Tensor qn, Tensor kn, Tensor rq, Tensor rk, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, "
        "int groups) -> (Tensor, Tensor, Tensor)");
  m.def("varlen_attention(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, int max_seqlen_q, int max_seqlen_k, "
        "float scale, bool causal, bool l2norm_qk, int groups) -> Tensor");
  // decoding against a key/value cache (forward only): appends k_new / v_new to the caches in place, then attends
  m.def("kvcache_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor? k_new, Tensor? v_new, Tensor? cache_seqlens, "
        "Tensor? block_table, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups) -> Tensor");
  // sliding-window (local) attention: the ops above with window_left / window_right (-1: unbounded); no mask, no attn_bias
  m.def("window_forward(Tensor q, Tensor k, Tensor v, float scale, bool causal, bool l2norm_qk, int groups, bool need_backward, "
        "int window_left, int window_right) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("window_backward(Tensor d_out, Tensor o, Tensor inv_l, Tensor q, Tensor k, Tensor v, Tensor qn, Tensor kn, Tensor rq, Tensor rk, "
        "float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> (Tensor, Tensor, Tensor)");
  m.def("window_attention(Tensor q, Tensor k, Tensor v, float scale, bool causal, bool l2norm_qk, int groups, int window_left, "
        "int window_right) -> Tensor");
  m.def("varlen_window_forward(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, int max_seqlen_q, int max_seqlen_k, "
        "float scale, bool causal, bool l2norm_qk, int groups, bool need_backward, int window_left, int window_right) "
        "-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("varlen_window_backward(Tensor d_out, Tensor o, Tensor inv_l, Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, "
        "Tensor qn, Tensor kn, Tensor rq, Tensor rk, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, "
        "int groups, int window_left, int window_right) -> (Tensor, Tensor, Tensor)");
  m.def("varlen_window_attention(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, int max_seqlen_q, int max_seqlen_k, "
        "float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> Tensor");
  m.def("kvcache_window_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor? k_new, Tensor? v_new, Tensor? cache_seqlens, "
        "Tensor? block_table, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> Tensor");
  // an fp8 (e4m3fn) cache, its codes as uint8 tensors: k_scale / v_scale float32 [], [Hk] or [B, Hk]; the append quantises k_new / v_new
  m.def("kvcache_fp8_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor? k_new, Tensor? v_new, Tensor? cache_seqlens, "
        "Tensor? block_table, Tensor k_scale, Tensor v_scale, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, "
        "int window_left, int window_right) -> Tensor");
  // a ragged step: q [total_q, H, D] and k_new / v_new [total_q, Hk, D] packed by cu_seqlens_q [B + 1]; k_scale / v_scale: an fp8 cache
  m.def("kvcache_varlen_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cu_seqlens_q, Tensor? k_new, Tensor? v_new, "
        "Tensor? cache_seqlens, Tensor? block_table, Tensor? k_scale, Tensor? v_scale, int max_seqlen_q, int max_seqlen_k, float scale, "
        "bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> Tensor");
  // every decode route with the rows' log-sum-exp (float32 [B, H, N]; ragged: [total_q, H]) as a second result
  m.def("kvcache_lse_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor? cu_seqlens_q, Tensor? k_new, Tensor? v_new, "
        "Tensor? cache_seqlens, Tensor? block_table, Tensor? k_scale, Tensor? v_scale, int max_seqlen_q, int max_seqlen_k, float scale, "
        "bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> (Tensor, Tensor)");
  // attention states over disjoint key sets of the same queries -> the state over the union
  m.def("merge_states(Tensor[] os, Tensor[] lses) -> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(fcsa, CUDA, m) {       // ROCm builds of PyTorch dispatch HIP tensors under the CUDA key
  m.impl("forward", &forward);
  m.impl("backward", &backward);
  m.impl("attention", &attention_plain);
  m.impl("varlen_forward", &varlen_forward);
  m.impl("varlen_backward", &varlen_backward);
  m.impl("varlen_attention", &varlen_attention_plain);
  m.impl("kvcache_forward", &kvcache_forward);
  m.impl("window_forward", &window_forward);
  m.impl("window_backward", &window_backward);
  m.impl("window_attention", &window_attention_plain);
  m.impl("varlen_window_forward", &varlen_window_forward);
  m.impl("varlen_window_backward", &varlen_window_backward);
  m.impl("varlen_window_attention", &varlen_window_attention_plain);
  m.impl("kvcache_window_forward", &kvcache_window_forward);
  m.impl("kvcache_fp8_forward", &kvcache_fp8_forward);
  m.impl("kvcache_varlen_forward", &kvcache_varlen_forward);
  m.impl("kvcache_lse_forward", &kvcache_lse_forward);
  m.impl("merge_states", &merge_states);
}

// The prefill op has a namespace of its own: the op set of `fcsa` is pinned.  Forward only: no Autograd kernel.
TORCH_LIBRARY(fcsa_prefill, m) {
  m.def("kvcache_prefill_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cu_seqlens_q, Tensor? k_new, Tensor? v_new, "
        "Tensor? cache_seqlens, Tensor? block_table, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, "
        "int groups) -> (Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(fcsa_prefill, CUDA, m) { m.impl("kvcache_prefill_forward", &kvcache_prefill_forward); }

// The engine step, likewise in a namespace of its own.  Forward only: no Autograd kernel.
TORCH_LIBRARY(fcsa_step, m) {
  m.def("kvcache_step_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cu_seqlens_q, Tensor? k_new, Tensor? v_new, "
        "Tensor? cache_seqlens, Tensor? block_table, Tensor? k_scale, Tensor? v_scale, int max_seqlen_q, int max_seqlen_k, float scale, "
        "bool causal, bool l2norm_qk, int groups, int window_left, int window_right, int chunk_rows, int max_decode_tokens, bool no_decode, "
        "bool no_chunk) -> (Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(fcsa_step, CUDA, m) { m.impl("kvcache_step_forward", &kvcache_step_forward); }

// tree attention for speculative decoding in a namespace of its own, as above
TORCH_LIBRARY(fcsa_tree, m) {
  m.def("kvcache_tree_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cu_seqlens_q, Tensor tree_mask, Tensor? k_new, "
        "Tensor? v_new, Tensor? cache_seqlens, Tensor? block_table, Tensor? k_scale, Tensor? v_scale, int max_seqlen_q, int max_seqlen_k, "
        "float scale, bool l2norm_qk, int groups) -> (Tensor, Tensor)");
  m.def("kvcache_compact(Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cache_seqlens, Tensor accepted, Tensor num_accepted, "
        "Tensor? block_table) -> ()");
}
TORCH_LIBRARY_IMPL(fcsa_tree, CUDA, m) {
  m.impl("kvcache_tree_forward", &kvcache_tree_forward);
  m.impl("kvcache_compact", &kvcache_compact);
}

// the engine step with a linear position bias, likewise.  Forward only: no Autograd kernel.
TORCH_LIBRARY(fcsa_alibi, m) {
  m.def("kvcache_alibi_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cu_seqlens_q, Tensor alibi_slopes, Tensor? k_new, "
        "Tensor? v_new, Tensor? cache_seqlens, Tensor? block_table, Tensor? k_scale, Tensor? v_scale, int max_seqlen_q, int max_seqlen_k, "
        "float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right, int chunk_rows, int max_decode_tokens, "
        "bool no_decode, bool no_chunk) -> (Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(fcsa_alibi, CUDA, m) { m.impl("kvcache_alibi_forward", &kvcache_alibi_forward); }

// Attention states for training, in a namespace of their own (the op set of `fcsa` is pinned): the attention op with the rows'
// log-sum-exp as a second differentiable result -- dense, local (window sides other than (-1, -1)) or packed (cu_seqlens given) -- and
// the differentiable merge, each with its forward and backward op.
TORCH_LIBRARY(fcsa_state, m) {
  m.def("attention_state_forward(Tensor q, Tensor k, Tensor v, Tensor? cu_seqlens_q, Tensor? cu_seqlens_k, int max_seqlen_q, int max_seqlen_k, "
        "float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) "
        "-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("attention_state_backward(Tensor? d_out, Tensor? d_lse, Tensor o, Tensor inv_l, Tensor q, Tensor k, Tensor v, Tensor? cu_seqlens_q, "
        "Tensor? cu_seqlens_k, Tensor qn, Tensor kn, Tensor rq, Tensor rk, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, "
        "bool l2norm_qk, int groups, int window_left, int window_right) -> (Tensor, Tensor, Tensor)");
  m.def("attention_state(Tensor q, Tensor k, Tensor v, Tensor? cu_seqlens_q, Tensor? cu_seqlens_k, int max_seqlen_q, int max_seqlen_k, "
        "float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> (Tensor, Tensor)");
  m.def("merge_state_backward(Tensor? d_o, Tensor? d_lse, Tensor[] os, Tensor[] lses) -> (Tensor[], Tensor[])");
  m.def("merge_state(Tensor[] os, Tensor[] lses) -> (Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(fcsa_state, CUDA, m) {
  m.impl("attention_state_forward", &attention_state_forward);
  m.impl("attention_state_backward", &attention_state_backward);
  m.impl("attention_state", &attention_state_plain);
  m.impl("merge_state_backward", &merge_state_backward);
  m.impl("merge_state", &merge_states);
}
TORCH_LIBRARY_IMPL(fcsa_state, Autograd, m) {
  m.impl("attention_state", &attention_state_autograd);
  m.impl("merge_state", &merge_state_autograd);
}

// The training calls with a linear position bias, in a namespace of their own (the op sets of `fcsa` and `fcsa_alibi` are pinned): forward,
// backward, and the differentiable attention op -- dense, local or packed, as in fcsa_state.
TORCH_LIBRARY(fcsa_alibi_train, m) {
  m.def("forward(Tensor q, Tensor k, Tensor v, Tensor alibi_slopes, Tensor? cu_seqlens_q, Tensor? cu_seqlens_k, int max_seqlen_q, "
        "int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right, bool need_backward) "
        "-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("backward(Tensor d_out, Tensor o, Tensor inv_l, Tensor q, Tensor k, Tensor v, Tensor alibi_slopes, Tensor? cu_seqlens_q, "
        "Tensor? cu_seqlens_k, Tensor qn, Tensor kn, Tensor rq, Tensor rk, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, "
        "bool l2norm_qk, int groups, int window_left, int window_right) -> (Tensor, Tensor, Tensor)");
  m.def("attention(Tensor q, Tensor k, Tensor v, Tensor alibi_slopes, Tensor? cu_seqlens_q, Tensor? cu_seqlens_k, int max_seqlen_q, "
        "int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> Tensor");
}
TORCH_LIBRARY_IMPL(fcsa_alibi_train, CUDA, m) {
  m.impl("forward", &alibi_train_forward);
  m.impl("backward", &alibi_train_backward);
  m.impl("attention", &alibi_train_attention_plain);
}
TORCH_LIBRARY_IMPL(fcsa_alibi_train, Autograd, m) { m.impl("attention", &alibi_train_attention_autograd); }

TORCH_LIBRARY_IMPL(fcsa, Autograd, m) {
  m.impl("attention", &attention_autograd);
  m.impl("varlen_attention", &varlen_attention_autograd);
  m.impl("window_attention", &window_attention_autograd);
  m.impl("varlen_window_attention", &varlen_window_attention_autograd);
}
