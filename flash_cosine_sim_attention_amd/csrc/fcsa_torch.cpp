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
#include <torch/csrc/autograd/custom_function.h>
#include <torch/library.h>

#include <dlfcn.h>

#include <atomic>
#include <cstring>
#include <chrono>
#include <tuple>

#include "../../include/fcsa.h"

namespace {

// The C ABI is called through pointers so that measurement tools can swap in another build of the same ABI at run time
// (fcsa_torch_use_library, tools/ab_libs.py: interleaved A/B of kernel variants in ONE process).  Default: the library this
// module is linked against.
struct Abi {
  int (*forward)(const fcsa_forward_args*) = &fcsa_forward;
  int (*backward)(const fcsa_backward_args*) = &fcsa_backward;
  size_t (*forward_ws)(const fcsa_problem*) = &fcsa_forward_workspace_bytes;
  size_t (*backward_ws)(const fcsa_problem*) = &fcsa_backward_workspace_bytes;
  int (*needs_qn)(const fcsa_problem*, int32_t) = &fcsa_forward_needs_qn;
  const char* (*last_error)(void) = &fcsa_last_error;
  // packed sequences: null when a library swapped in by fcsa_torch_use_library does not export them (the varlen ops then raise)
  int (*forward_varlen)(const fcsa_forward_args*, const fcsa_varlen*) = &fcsa_forward_varlen;
  int (*backward_varlen)(const fcsa_backward_args*, const fcsa_varlen*) = &fcsa_backward_varlen;
  size_t (*backward_varlen_ws)(const fcsa_problem*, const fcsa_varlen*) = &fcsa_backward_varlen_workspace_bytes;
  // decoding against a key/value cache: null in a swapped-in library that does not export it (the kvcache op then raises)
  int (*forward_kvcache)(const fcsa_forward_args*, const fcsa_kvcache*) = &fcsa_forward_kvcache;
  size_t (*forward_kvcache_ws)(const fcsa_problem*, const fcsa_kvcache*) = &fcsa_forward_kvcache_workspace_bytes;
  // sliding window: null in a swapped-in library that does not export it (the window ops then raise)
  int (*forward_window)(const fcsa_forward_args*, const fcsa_varlen*, const fcsa_window*) = &fcsa_forward_window;
  int (*backward_window)(const fcsa_backward_args*, const fcsa_varlen*, const fcsa_window*) = &fcsa_backward_window;
  size_t (*backward_window_ws)(const fcsa_problem*, const fcsa_varlen*, const fcsa_window*) = &fcsa_backward_window_workspace_bytes;
  int (*forward_kvcache_window)(const fcsa_forward_args*, const fcsa_kvcache*, const fcsa_window*) = &fcsa_forward_kvcache_window;
  size_t (*forward_kvcache_window_ws)(const fcsa_problem*, const fcsa_kvcache*, const fcsa_window*) = &fcsa_forward_kvcache_window_workspace_bytes;
  // fp8 key/value cache: null in a swapped-in library that does not export it (the fp8 op then raises)
  int (*forward_kvcache_quant)(const fcsa_forward_args*, const fcsa_kvcache*, const fcsa_kvcache_quant*, const fcsa_window*) = &fcsa_forward_kvcache_quant;
  size_t (*forward_kvcache_quant_ws)(const fcsa_problem*, const fcsa_kvcache*, const fcsa_kvcache_quant*, const fcsa_window*) =
      &fcsa_forward_kvcache_quant_workspace_bytes;
  // ragged decode steps (packed queries with per-sequence counts): likewise
  int (*forward_kvcache_varlen)(const fcsa_forward_args*, const fcsa_kvcache*, const fcsa_varlen*, const fcsa_kvcache_quant*, const fcsa_window*) =
      &fcsa_forward_kvcache_varlen;
  size_t (*forward_kvcache_varlen_ws)(const fcsa_problem*, const fcsa_kvcache*, const fcsa_varlen*, const fcsa_kvcache_quant*, const fcsa_window*) =
      &fcsa_forward_kvcache_varlen_workspace_bytes;
  // the decode calls with the rows' log-sum-exp, and merging attention states: likewise
  int (*forward_kvcache_lse)(const fcsa_forward_args*, const fcsa_kvcache*, const fcsa_varlen*, const fcsa_kvcache_quant*, const fcsa_window*,
                             const fcsa_lse_out*) = &fcsa_forward_kvcache_lse;
  int (*merge_states)(const fcsa_merge_args*) = &fcsa_merge_states;
} g_abi;

using at::Tensor;
using c10::optional;

// Host-time accounting of the two ops (tools/host_overhead.py; small problems are bound by host time per call, not by the
// kernels): nanoseconds spent in [0] forward checks / canonicalisation, [1] forward allocations, [2] fcsa_forward (validation +
// launches), [3..5] the same for backward, [6] forward calls, [7] backward calls.  Two clock reads per section, always on.
std::atomic<uint64_t> g_host_ns[8];
struct Lap {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void mark(int slot) {
    const auto n = std::chrono::steady_clock::now();
    g_host_ns[slot].fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(n - t).count(), std::memory_order_relaxed);
    t = n;
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

fcsa_tensor view4(const Tensor& t) {
  fcsa_tensor v;
  v.ptr = t.data_ptr();
  v.stride0 = t.stride(0);
  v.stride1 = t.stride(1);
  v.stride2 = t.stride(2);
  return v;
}

struct Canon {
  Tensor q, k, v;                 // 4-D, rows ok
  optional<Tensor> mask, bias;    // contiguous
  bool bias_batch, merged;
  int64_t B, H, Hk, N, M, D;
};

Canon canonicalise(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& mask, const optional<Tensor>& bias,
                   bool bias_batch, bool causal) {
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
  Canon c;
  c.merged = q.dim() == 3;
  c.bias_batch = bias_batch;
  if (c.merged) {
    TORCH_CHECK_VALUE(k.dim() == 3 && v.dim() == 3, "if batch and heads are merged for queries, keys and values must also have 3 dimensions");
    c.bias_batch = true;                                                                                          // cu:1652
    c.q = q.unsqueeze(1);
  } else {
    TORCH_CHECK_VALUE(q.dim() == 4, "q must have 3 or 4 dimensions, got ", q.dim());
    c.q = q;
  }
  c.k = k.dim() == 3 ? k.unsqueeze(1) : k;
  c.v = v.dim() == 3 ? v.unsqueeze(1) : v;
  TORCH_CHECK_VALUE(c.k.dim() == 4 && c.v.dim() == 4, "k and v must have 3 or 4 dimensions");
  c.B = c.q.size(0); c.H = c.q.size(1); c.N = c.q.size(2); c.D = c.q.size(3);
  c.Hk = c.k.size(1); c.M = c.k.size(2);
  TORCH_CHECK_VALUE(c.v.sizes() == c.k.sizes(), "k and v must have the same shape, got ", k.sizes(), " and ", v.sizes());
  TORCH_CHECK_VALUE(c.k.size(3) == c.D, "query, key, value dimensions must be the same");                          // cu:1673
  TORCH_CHECK_VALUE(c.D == 16 || c.D == 32 || c.D == 64 || c.D == 96 || c.D == 128,
                    "only dimensions (16, 32, 64, 96, 128) allowed for now, got ", c.D);                            // cu:1674
  TORCH_CHECK_VALUE(c.k.size(0) == c.B, "batch mismatch between q (", c.B, ") and k/v (", c.k.size(0), ")");
  // grouped-query attention: query head h reads K/V head h / (H / Hk); single-headed (Hk == 1) and Hk == H are the two ends
  TORCH_CHECK_VALUE(c.Hk == c.H || (c.Hk >= 1 && c.H % c.Hk == 0),
                    "k/v heads must divide q heads (", c.H, "): grouped-query attention needs H % Hk == 0, got Hk = ", c.Hk);
  if (mask.has_value()) {
    TORCH_CHECK_VALUE(mask->scalar_type() == at::kBool && mask->dim() == 2 && mask->size(0) == c.B && mask->size(1) == c.M,
                      "mask must be a bool tensor of shape (", c.B, ", ", c.M, "), got ", mask->scalar_type(), " ", mask->sizes());
    c.mask = mask->contiguous();
  }
  if (bias.has_value()) {
    const int64_t lead = c.bias_batch ? c.B : c.H;
    TORCH_CHECK_VALUE(bias->dim() == 3 && bias->size(0) == lead && bias->size(1) == c.N && bias->size(2) == c.M,
                      "attn_bias must have shape (", lead, ", ", c.N, ", ", c.M, "), got ", bias->sizes());
    TORCH_CHECK_TYPE(bias->scalar_type() == q.scalar_type(), "attn_bias must have the dtype of q");
    c.bias = bias->contiguous();
  }
  c.q = prep(c.q); c.k = prep(c.k); c.v = prep(c.v);
  return c;
}

fcsa_problem problem(const Canon& c, at::ScalarType dt, bool causal, bool l2norm_qk, int64_t groups, double scale) {
  fcsa_problem p;
  p.dtype = dtype_code(dt);
  p.batch = (int32_t)c.B; p.heads = (int32_t)c.H; p.kv_heads = (int32_t)c.Hk;
  p.q_len = (int32_t)c.N; p.k_len = (int32_t)c.M; p.dim_head = (int32_t)c.D;
  p.causal = causal; p.bias_batch_dim = c.bias_batch; p.l2norm_qk = l2norm_qk;
  p.groups = l2norm_qk ? (int32_t)groups : 1;
  p.scale = (float)scale;
  return p;
}

void check(int rc, const char* what) {
  TORCH_CHECK(rc == FCSA_OK, what, " failed (status ", rc, "): ", g_abi.last_error());
}

void* stream_of(const Tensor& t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

// (o, inv_l, qn, kn, rq, rk); the saved-state tensors are empty (numel 0) where they are not produced
// sliding window of a call (window ops): the library's struct, after the checks every window op shares; nullptr: no window
struct Win {
  fcsa_window w;
  Win(int64_t left, int64_t right) {
    TORCH_CHECK(g_abi.forward_window != nullptr && g_abi.backward_window != nullptr && g_abi.backward_window_ws != nullptr &&
                g_abi.forward_kvcache_window != nullptr && g_abi.forward_kvcache_window_ws != nullptr,
                "sliding window: the loaded libfcsa_hip.so does not export fcsa_forward_window / fcsa_backward_window");
    TORCH_CHECK_VALUE(left >= -1 && right >= -1, "window_size (", left, ", ", right, "): each side must be >= 0, or -1 for unbounded");
    w.left = (int32_t)std::min<int64_t>(left, INT32_MAX);
    w.right = (int32_t)std::min<int64_t>(right, INT32_MAX);
  }
};

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> forward_impl(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& mask,
                                                                         const optional<Tensor>& attn_bias, bool attn_bias_batch_dim, double scale,
                                                                         bool causal, bool l2norm_qk, int64_t groups, bool need_backward,
                                                                         const fcsa_window* win) {
  Lap lap;
  const Canon c = canonicalise(q, k, v, mask, attn_bias, attn_bias_batch_dim, causal);
  TORCH_CHECK_VALUE(!l2norm_qk || (groups >= 1 && c.D % groups == 0), "groups (", groups, ") must divide the head dimension (", c.D, ")");
  c10::DeviceGuard guard(q.device());
  lap.mark(0);
  const auto opt = q.options();
  const auto f32 = opt.dtype(at::kFloat);
  fcsa_forward_args a;
  a.p = problem(c, q.scalar_type(), causal, l2norm_qk, groups, scale);
  Tensor o = at::empty({c.B, c.H, c.N, c.D}, opt);
  Tensor none = at::empty({0}, f32);
  Tensor inv_l = need_backward ? at::empty({c.B, c.H, c.N}, f32) : none;
  Tensor qn = at::empty({0}, opt), kn = qn, rq = none, rk = none;
  if (l2norm_qk) {
    // An inference call (need_backward false) gets kn only -- and qn where q takes the row kernel (fcsa_forward_needs_qn): the
    // 16-bit forward kernels then write nothing but `o` (the reference's need_store_rowsum == false path, cu:1086, cu:1241).
    if (g_abi.needs_qn(&a.p, need_backward ? 1 : 0) != 0) qn = at::empty({c.B, c.H, c.N, c.D}, opt);
    kn = at::empty({c.B, c.Hk, c.M, c.D}, opt);
    if (need_backward) {
      rq = at::empty({c.B, c.H, c.N, groups}, f32);
      rk = at::empty({c.B, c.Hk, c.M, groups}, f32);
    }
  }
  a.q = view4(c.q); a.k = view4(c.k); a.v = view4(c.v); a.o = view4(o);
  a.inv_l = need_backward ? inv_l.data_ptr<float>() : nullptr;
  a.mask = c.mask.has_value() ? static_cast<const uint8_t*>(c.mask->data_ptr()) : nullptr;
  a.attn_bias = c.bias.has_value() ? c.bias->data_ptr() : nullptr;
  a.norm.qn = qn.numel() > 0 ? qn.data_ptr() : nullptr;
  a.norm.kn = l2norm_qk ? kn.data_ptr() : nullptr;
  a.norm.rq = (l2norm_qk && need_backward) ? rq.data_ptr<float>() : nullptr;
  a.norm.rk = (l2norm_qk && need_backward) ? rk.data_ptr<float>() : nullptr;
  Tensor ws;
  a.workspace = nullptr; a.workspace_bytes = 0;
  size_t fws = g_abi.forward_ws(&a.p);      // 0 unless the key range is split (grids that cannot fill the chip)
  if (win != nullptr) {      // a window that IS the un-windowed or the causal call splits like that call: room for either
    fcsa_problem other = a.p;
    other.causal = !other.causal;
    fws = std::max(fws, g_abi.forward_ws(&other));
  }
  if (const size_t need = fws; need > 0) {
    ws = at::empty({(int64_t)need}, opt.dtype(at::kByte));
    a.workspace = ws.data_ptr(); a.workspace_bytes = need;
  }
  a.stream = stream_of(q);
  lap.mark(1);
  if (win != nullptr) check(g_abi.forward_window(&a, nullptr, win), "fcsa_forward_window");
  else check(g_abi.forward(&a), "fcsa_forward");
  lap.mark(2);
  g_host_ns[6].fetch_add(1, std::memory_order_relaxed);
  if (c.merged) o = o.squeeze(1);                                                                                  // cu:1740-1741
  return std::make_tuple(o, inv_l, qn, kn, rq, rk);
}
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> forward(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& mask,
                                                                    const optional<Tensor>& attn_bias, bool attn_bias_batch_dim, double scale,
                                                                    bool causal, bool l2norm_qk, int64_t groups, bool need_backward) {
  return forward_impl(q, k, v, mask, attn_bias, attn_bias_batch_dim, scale, causal, l2norm_qk, groups, need_backward, nullptr);
}
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> window_forward(const Tensor& q, const Tensor& k, const Tensor& v, double scale, bool causal,
                                                                           bool l2norm_qk, int64_t groups, bool need_backward, int64_t left,
                                                                           int64_t right) {
  const Win win(left, right);
  return forward_impl(q, k, v, c10::nullopt, c10::nullopt, false, scale, causal, l2norm_qk, groups, need_backward, &win.w);
}

// (dq, dk, dv, d_bias) in the shapes / dtype of the inputs; d_bias is empty when not requested
std::tuple<Tensor, Tensor, Tensor, Tensor> backward_impl(const Tensor& d_out, const Tensor& o, const Tensor& inv_l, const Tensor& q, const Tensor& k,
                                                         const Tensor& v, const optional<Tensor>& mask, const optional<Tensor>& attn_bias,
                                                         const Tensor& qn, const Tensor& kn, const Tensor& rq, const Tensor& rk,
                                                         bool attn_bias_batch_dim, double scale, bool causal, bool l2norm_qk, int64_t groups,
                                                         bool need_bias_grad, const fcsa_window* win) {
  Lap lap;
  const Canon c = canonicalise(q, k, v, mask, attn_bias, attn_bias_batch_dim, causal);
  c10::DeviceGuard guard(q.device());
  const auto opt = q.options();
  Tensor o4 = prep(o.dim() == 3 ? o.unsqueeze(1) : o);
  Tensor do4 = d_out.dim() == 3 ? d_out.unsqueeze(1) : d_out;
  // A broadcast gradient (`out.sum().backward()`, the reference's own timing protocol, benchmark.py:46-48: one scalar expanded with
  // all strides 0) is not materialised at [B,H,N,D]: one contiguous feature row is, and the kernels read it with a row pitch of 0.
  bool broadcast = do4.numel() > 0;
  for (int64_t d = 0; d < do4.dim(); ++d) broadcast = broadcast && (do4.stride(d) == 0 || do4.size(d) == 1);
  if (broadcast && do4.dim() == 4) {
    Tensor row = do4.as_strided({do4.size(3)}, {0}).to(q.scalar_type()).contiguous();                  // [D], a D-element copy kernel
    do4 = row.as_strided(do4.sizes(), {0, 0, 0, 1});
  }
  if (do4.scalar_type() != q.scalar_type()) do4 = do4.to(q.scalar_type());
  do4 = prep(do4);
  TORCH_CHECK_VALUE(do4.sizes() == o4.sizes(), "d_out must have the shape of the output");
  TORCH_CHECK_VALUE(o4.size(0) == c.B && o4.size(1) == c.H && o4.size(2) == c.N && o4.size(3) == c.D, "o does not belong to these inputs");
  // this op is public (torch.ops.fcsa.backward, ext.backward): everything a kernel dereferences is checked, not only its size
  auto saved_ok = [&](const char* name, const Tensor& t, at::ScalarType st, int64_t numel) {
    TORCH_CHECK_VALUE(t.defined() && t.device() == q.device() && t.scalar_type() == st && t.numel() == numel && t.is_contiguous(),
                      name, " does not belong to these inputs (expected a contiguous ", st, " tensor of ", numel, " elements on ", q.device(), ")");
  };
  TORCH_CHECK_TYPE(o4.scalar_type() == q.scalar_type() && o4.device() == q.device(), "o must have the dtype and device of q");
  TORCH_CHECK_VALUE(do4.device() == q.device(), "d_out is on ", do4.device(), " but q is on ", q.device());
  saved_ok("inv_l", inv_l, at::kFloat, c.B * c.H * c.N);
  if (l2norm_qk) {
    saved_ok("qn", qn, q.scalar_type(), c.B * c.H * c.N * c.D);
    saved_ok("kn", kn, q.scalar_type(), c.B * c.Hk * c.M * c.D);
    saved_ok("rq", rq, at::kFloat, c.B * c.H * c.N * groups);
    saved_ok("rk", rk, at::kFloat, c.B * c.Hk * c.M * groups);
  }
  lap.mark(3);
  Tensor dq = at::empty({c.B, c.H, c.N, c.D}, opt);
  Tensor dk = at::empty({c.B, c.Hk, c.M, c.D}, opt);
  Tensor dv = at::empty({c.B, c.Hk, c.M, c.D}, opt);
  // d_bias in the bias dtype, every element written once by the library: no zero-fill, no f32 tensor, no cast pass (cf. cu:1827, cu:1912)
  Tensor db = (c.bias.has_value() && need_bias_grad) ? at::empty(c.bias->sizes(), opt) : at::empty({0}, opt);
  fcsa_backward_args a;
  a.p = problem(c, q.scalar_type(), causal, l2norm_qk, groups, scale);
  size_t wsb = win != nullptr ? g_abi.backward_window_ws(&a.p, nullptr, win) : g_abi.backward_ws(&a.p);
  if (wsb < 256) wsb = 256;
  Tensor ws = at::empty({(int64_t)wsb}, opt.dtype(at::kByte));
  a.d_out = view4(do4); a.o = view4(o4);
  a.inv_l = inv_l.data_ptr<float>();
  a.q = view4(c.q); a.k = view4(c.k); a.v = view4(c.v);
  a.mask = c.mask.has_value() ? static_cast<const uint8_t*>(c.mask->data_ptr()) : nullptr;
  a.attn_bias = c.bias.has_value() ? c.bias->data_ptr() : nullptr;
  a.norm.qn = l2norm_qk ? qn.data_ptr() : nullptr;
  a.norm.kn = l2norm_qk ? kn.data_ptr() : nullptr;
  a.norm.rq = l2norm_qk ? rq.data_ptr<float>() : nullptr;
  a.norm.rk = l2norm_qk ? rk.data_ptr<float>() : nullptr;
  a.dq = view4(dq); a.dk = view4(dk); a.dv = view4(dv);
  a.d_bias = db.numel() > 0 ? db.data_ptr() : nullptr;
  a.workspace = ws.data_ptr(); a.workspace_bytes = wsb;
  a.stream = stream_of(q);
  lap.mark(4);
  if (win != nullptr) check(g_abi.backward_window(&a, nullptr, win), "fcsa_backward_window");
  else check(g_abi.backward(&a), "fcsa_backward");
  lap.mark(5);
  g_host_ns[7].fetch_add(1, std::memory_order_relaxed);
  return std::make_tuple(dq.reshape(q.sizes()), dk.reshape(k.sizes()), dv.reshape(v.sizes()), db);
}
std::tuple<Tensor, Tensor, Tensor, Tensor> backward(const Tensor& d_out, const Tensor& o, const Tensor& inv_l, const Tensor& q, const Tensor& k,
                                                    const Tensor& v, const optional<Tensor>& mask, const optional<Tensor>& attn_bias,
                                                    const Tensor& qn, const Tensor& kn, const Tensor& rq, const Tensor& rk,
                                                    bool attn_bias_batch_dim, double scale, bool causal, bool l2norm_qk, int64_t groups,
                                                    bool need_bias_grad) {
  return backward_impl(d_out, o, inv_l, q, k, v, mask, attn_bias, qn, kn, rq, rk, attn_bias_batch_dim, scale, causal, l2norm_qk, groups,
                       need_bias_grad, nullptr);
}
std::tuple<Tensor, Tensor, Tensor> window_backward(const Tensor& d_out, const Tensor& o, const Tensor& inv_l, const Tensor& q, const Tensor& k,
                                                   const Tensor& v, const Tensor& qn, const Tensor& kn, const Tensor& rq, const Tensor& rk,
                                                   double scale, bool causal, bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
  const Win win(left, right);
  auto g = backward_impl(d_out, o, inv_l, q, k, v, c10::nullopt, c10::nullopt, qn, kn, rq, rk, false, scale, causal, l2norm_qk, groups, false, &win.w);
  return std::make_tuple(std::get<0>(g), std::get<1>(g), std::get<2>(g));
}


// ---- packed variable-length sequences (fcsa_forward_varlen / fcsa_backward_varlen) ----------------------------------------------------
// q [total_q, H, D], k / v [total_k, Hk, D], cu_seqlens_* int32 [S + 1] on q's device.  The tables are passed to the library as they are:
// their contents are never read on the host (the Python wrapper validates host tables before they are moved to the device).
struct VCanon {
  Tensor q, k, v, cu_q, cu_k;     // rows ok; tables contiguous
  int64_t S, H, Hk, TQ, TK, D;
};

VCanon canonicalise_varlen(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q, const Tensor& cu_k, int64_t max_q,
                           int64_t max_k) {
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
  VCanon c;
  c.S = cu_q.numel() - 1;
  c.TQ = q.size(0); c.H = q.size(1); c.D = q.size(2);
  c.TK = k.size(0); c.Hk = k.size(1);
  TORCH_CHECK_VALUE(k.size(2) == c.D, "query, key, value dimensions must be the same");
  TORCH_CHECK_VALUE(c.D == 16 || c.D == 32 || c.D == 64 || c.D == 96 || c.D == 128,
                    "only dimensions (16, 32, 64, 96, 128) allowed for now, got ", c.D);
  TORCH_CHECK_VALUE(c.Hk >= 1 && c.H % c.Hk == 0, "k/v heads must divide q heads (", c.H, "), got ", c.Hk);
  TORCH_CHECK_VALUE(max_q >= 0 && max_k >= 0 && max_q <= INT32_MAX && max_k <= INT32_MAX && c.S <= INT32_MAX,
                    "max_seqlen_q / max_seqlen_k must lie in [0, 2^31), got ", max_q, ", ", max_k);
  TORCH_CHECK_VALUE(c.H * std::max(c.TQ, c.TK) <= INT32_MAX, "varlen: heads x packed rows must stay below 2^31");
  c.q = prep(q); c.k = prep(k); c.v = prep(v);
  c.cu_q = cu_q.contiguous(); c.cu_k = cu_k.contiguous();
  return c;
}

fcsa_problem varlen_problem(const VCanon& c, at::ScalarType dt, int64_t max_q, int64_t max_k, bool causal, bool l2norm_qk, int64_t groups,
                            double scale) {
  fcsa_problem p;
  p.dtype = dtype_code(dt);
  p.batch = (int32_t)c.S; p.heads = (int32_t)c.H; p.kv_heads = (int32_t)c.Hk;
  p.q_len = (int32_t)max_q; p.k_len = (int32_t)max_k; p.dim_head = (int32_t)c.D;
  p.causal = causal; p.bias_batch_dim = 0; p.l2norm_qk = l2norm_qk;
  p.groups = l2norm_qk ? (int32_t)groups : 1;
  p.scale = (float)scale;
  return p;
}

fcsa_varlen varlen_table(const VCanon& c) {
  fcsa_varlen t;
  t.cu_seqlens_q = c.cu_q.data_ptr<int32_t>();
  t.cu_seqlens_k = c.cu_k.data_ptr<int32_t>();
  t.total_q = c.TQ; t.total_k = c.TK;
  return t;
}

// packed [total, heads, D] -> the ABI's view: stride0 ignored, stride1 = head stride, stride2 = token stride
fcsa_tensor packed3(const Tensor& t) {
  fcsa_tensor v;
  v.ptr = t.data_ptr();
  v.stride0 = 0;
  v.stride1 = t.stride(1);
  v.stride2 = t.stride(0);
  return v;
}

void need_varlen_abi() {
  TORCH_CHECK(g_abi.forward_varlen != nullptr && g_abi.backward_varlen != nullptr && g_abi.backward_varlen_ws != nullptr,
              "flash_cosine_sim_attention_varlen: the loaded libfcsa_hip.so does not export fcsa_forward_varlen / fcsa_backward_varlen");
}

// (o, inv_l, qn, kn, rq, rk): o [total_q, H, D]; inv_l [H, total_q]; qn [H, total_q, D], kn [Hk, total_k, D], rq / rk [.., G]; empty where
// not produced
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> varlen_forward_impl(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q,
                                                                                const Tensor& cu_k, int64_t max_q, int64_t max_k, double scale,
                                                                                bool causal, bool l2norm_qk, int64_t groups, bool need_backward,
                                                                                const fcsa_window* win) {
  need_varlen_abi();
  const VCanon c = canonicalise_varlen(q, k, v, cu_q, cu_k, max_q, max_k);
  TORCH_CHECK_VALUE(!l2norm_qk || (groups >= 1 && c.D % groups == 0), "groups (", groups, ") must divide the head dimension (", c.D, ")");
  c10::DeviceGuard guard(q.device());
  const auto opt = q.options();
  const auto f32 = opt.dtype(at::kFloat);
  fcsa_forward_args a;
  a.p = varlen_problem(c, q.scalar_type(), max_q, max_k, causal, l2norm_qk, groups, scale);
  const fcsa_varlen t = varlen_table(c);
  Tensor o = at::empty({c.TQ, c.H, c.D}, opt);
  Tensor none = at::empty({0}, f32);
  Tensor inv_l = need_backward ? at::empty({c.H, c.TQ}, f32) : none;
  Tensor qn = at::empty({0}, opt), kn = qn, rq = none, rk = none;
  if (l2norm_qk) {
    fcsa_problem pp = a.p;      // fcsa_forward_needs_qn of the packed rows (batch 1, q_len = total_q)
    pp.batch = 1; pp.q_len = (int32_t)c.TQ; pp.k_len = (int32_t)c.TK;
    if (g_abi.needs_qn(&pp, need_backward ? 1 : 0) != 0) qn = at::empty({c.H, c.TQ, c.D}, opt);
    kn = at::empty({c.Hk, c.TK, c.D}, opt);
    if (need_backward) {
      rq = at::empty({c.H, c.TQ, groups}, f32);
      rk = at::empty({c.Hk, c.TK, groups}, f32);
    }
  }
  a.q = packed3(c.q); a.k = packed3(c.k); a.v = packed3(c.v); a.o = packed3(o);
  a.inv_l = need_backward ? inv_l.data_ptr<float>() : nullptr;
  a.mask = nullptr;
  a.attn_bias = nullptr;
  a.norm.qn = qn.numel() > 0 ? qn.data_ptr() : nullptr;
  a.norm.kn = (l2norm_qk && kn.numel() > 0) ? kn.data_ptr() : nullptr;
  a.norm.rq = (l2norm_qk && need_backward) ? rq.data_ptr<float>() : nullptr;
  a.norm.rk = (l2norm_qk && need_backward) ? rk.data_ptr<float>() : nullptr;
  a.workspace = nullptr; a.workspace_bytes = 0;      // packed sequences never split the key range
  a.stream = stream_of(q);
  if (win != nullptr) check(g_abi.forward_window(&a, &t, win), "fcsa_forward_window");
  else check(g_abi.forward_varlen(&a, &t), "fcsa_forward_varlen");
  return std::make_tuple(o, inv_l, qn, kn, rq, rk);
}
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> varlen_forward(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q,
                                                                           const Tensor& cu_k, int64_t max_q, int64_t max_k, double scale,
                                                                           bool causal, bool l2norm_qk, int64_t groups, bool need_backward) {
  return varlen_forward_impl(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, need_backward, nullptr);
}
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> varlen_window_forward(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q,
                                                                                  const Tensor& cu_k, int64_t max_q, int64_t max_k, double scale,
                                                                                  bool causal, bool l2norm_qk, int64_t groups, bool need_backward,
                                                                                  int64_t left, int64_t right) {
  const Win win(left, right);
  return varlen_forward_impl(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, need_backward, &win.w);
}

// (dq, dk, dv) shaped like q, k, v
std::tuple<Tensor, Tensor, Tensor> varlen_backward_impl(const Tensor& d_out, const Tensor& o, const Tensor& inv_l, const Tensor& q, const Tensor& k,
                                                        const Tensor& v, const Tensor& cu_q, const Tensor& cu_k, const Tensor& qn, const Tensor& kn,
                                                        const Tensor& rq, const Tensor& rk, int64_t max_q, int64_t max_k, double scale, bool causal,
                                                        bool l2norm_qk, int64_t groups, const fcsa_window* win) {
  need_varlen_abi();
  const VCanon c = canonicalise_varlen(q, k, v, cu_q, cu_k, max_q, max_k);
  c10::DeviceGuard guard(q.device());
  const auto opt = q.options();
  Tensor o3 = prep(o);
  Tensor do3 = d_out.scalar_type() != q.scalar_type() ? d_out.to(q.scalar_type()) : d_out;
  do3 = prep(do3);
  TORCH_CHECK_VALUE(o3.dim() == 3 && o3.size(0) == c.TQ && o3.size(1) == c.H && o3.size(2) == c.D, "o does not belong to these inputs");
  TORCH_CHECK_VALUE(do3.sizes() == o3.sizes(), "d_out must have the shape of the output");
  TORCH_CHECK_TYPE(o3.scalar_type() == q.scalar_type() && o3.device() == q.device(), "o must have the dtype and device of q");
  TORCH_CHECK_VALUE(do3.device() == q.device(), "d_out is on ", do3.device(), " but q is on ", q.device());
  auto saved_ok = [&](const char* name, const Tensor& t, at::ScalarType st, int64_t numel) {
    TORCH_CHECK_VALUE(t.defined() && t.device() == q.device() && t.scalar_type() == st && t.numel() == numel && t.is_contiguous(),
                      name, " does not belong to these inputs (expected a contiguous ", st, " tensor of ", numel, " elements on ", q.device(), ")");
  };
  saved_ok("inv_l", inv_l, at::kFloat, c.H * c.TQ);
  if (l2norm_qk) {
    saved_ok("qn", qn, q.scalar_type(), c.H * c.TQ * c.D);
    saved_ok("kn", kn, q.scalar_type(), c.Hk * c.TK * c.D);
    saved_ok("rq", rq, at::kFloat, c.H * c.TQ * groups);
    saved_ok("rk", rk, at::kFloat, c.Hk * c.TK * groups);
  }
  Tensor dq = at::empty({c.TQ, c.H, c.D}, opt);
  Tensor dk = at::empty({c.TK, c.Hk, c.D}, opt);
  Tensor dv = at::empty({c.TK, c.Hk, c.D}, opt);
  fcsa_backward_args a;
  a.p = varlen_problem(c, q.scalar_type(), max_q, max_k, causal, l2norm_qk, groups, scale);
  const fcsa_varlen t = varlen_table(c);
  size_t wsb = win != nullptr ? g_abi.backward_window_ws(&a.p, &t, win) : g_abi.backward_varlen_ws(&a.p, &t);
  if (wsb < 256) wsb = 256;
  Tensor ws = at::empty({(int64_t)wsb}, opt.dtype(at::kByte));      // the caching allocator
  a.d_out = packed3(do3); a.o = packed3(o3);
  a.inv_l = inv_l.numel() > 0 ? inv_l.data_ptr<float>() : nullptr;
  a.q = packed3(c.q); a.k = packed3(c.k); a.v = packed3(c.v);
  a.mask = nullptr;
  a.attn_bias = nullptr;
  a.norm.qn = (l2norm_qk && qn.numel() > 0) ? qn.data_ptr() : nullptr;
  a.norm.kn = (l2norm_qk && kn.numel() > 0) ? kn.data_ptr() : nullptr;
  a.norm.rq = (l2norm_qk && rq.numel() > 0) ? rq.data_ptr<float>() : nullptr;
  a.norm.rk = (l2norm_qk && rk.numel() > 0) ? rk.data_ptr<float>() : nullptr;
  a.dq = packed3(dq); a.dk = packed3(dk); a.dv = packed3(dv);
  a.d_bias = nullptr;
  a.workspace = ws.data_ptr(); a.workspace_bytes = wsb;
  a.stream = stream_of(q);
  if (win != nullptr) check(g_abi.backward_window(&a, &t, win), "fcsa_backward_window");
  else check(g_abi.backward_varlen(&a, &t), "fcsa_backward_varlen");
  return std::make_tuple(dq, dk, dv);
}
std::tuple<Tensor, Tensor, Tensor> varlen_backward(const Tensor& d_out, const Tensor& o, const Tensor& inv_l, const Tensor& q, const Tensor& k,
                                                   const Tensor& v, const Tensor& cu_q, const Tensor& cu_k, const Tensor& qn, const Tensor& kn,
                                                   const Tensor& rq, const Tensor& rk, int64_t max_q, int64_t max_k, double scale, bool causal,
                                                   bool l2norm_qk, int64_t groups) {
  return varlen_backward_impl(d_out, o, inv_l, q, k, v, cu_q, cu_k, qn, kn, rq, rk, max_q, max_k, scale, causal, l2norm_qk, groups, nullptr);
}
std::tuple<Tensor, Tensor, Tensor> varlen_window_backward(const Tensor& d_out, const Tensor& o, const Tensor& inv_l, const Tensor& q, const Tensor& k,
                                                          const Tensor& v, const Tensor& cu_q, const Tensor& cu_k, const Tensor& qn,
                                                          const Tensor& kn, const Tensor& rq, const Tensor& rk, int64_t max_q, int64_t max_k,
                                                          double scale, bool causal, bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
  const Win win(left, right);
  return varlen_backward_impl(d_out, o, inv_l, q, k, v, cu_q, cu_k, qn, kn, rq, rk, max_q, max_k, scale, causal, l2norm_qk, groups, &win.w);
}

// ---- autograd in C++ (reference: the Python autograd.Function FlashCosineSimAttention, flash_cosine_sim_attention.py:245-302).
// A Python Function costs ~60 us of interpreter / engine hand-over per forward+backward; this node costs a few.  forward and
// backward go through the dispatcher (fcsa::forward / fcsa::backward), so torch.compile traces them with the fake kernels.
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

struct AttentionFn : public torch::autograd::Function<AttentionFn> {
  static Tensor forward(AutogradContext* ctx, const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& mask,
                        const optional<Tensor>& attn_bias, bool attn_bias_batch_dim, double scale, bool causal, bool l2norm_qk,
                        int64_t groups) {
    // (Function::apply runs this with grad mode OFF: the no_grad case is decided by the caller, attention_autograd)
    const bool bias_grad = attn_bias.has_value() && attn_bias->requires_grad();
    const bool need = q.requires_grad() || k.requires_grad() || v.requires_grad() || bias_grad;                    // cu:1689
    at::AutoDispatchBelowADInplaceOrView guard;
    static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("fcsa::forward", "")
        .typed<std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>(const Tensor&, const Tensor&, const Tensor&, const optional<Tensor>&,
                                                                           const optional<Tensor>&, bool, double, bool, bool, int64_t, bool)>();
    auto r = op.call(q, k, v, mask, attn_bias, attn_bias_batch_dim, scale, causal, l2norm_qk, groups, need);
    if (need) {
      ctx->save_for_backward({std::get<0>(r), std::get<1>(r), q, k, v, mask.has_value() ? *mask : Tensor(),
                              attn_bias.has_value() ? *attn_bias : Tensor(), std::get<2>(r), std::get<3>(r), std::get<4>(r), std::get<5>(r)});
      ctx->saved_data["bias_batch"] = attn_bias_batch_dim;
      ctx->saved_data["scale"] = scale;
      ctx->saved_data["causal"] = causal;
      ctx->saved_data["l2norm_qk"] = l2norm_qk;
      ctx->saved_data["groups"] = groups;
      ctx->saved_data["bias_grad"] = bias_grad;
    }
    return std::get<0>(r);
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto s = ctx->get_saved_variables();
    const optional<Tensor> mask = s[5].defined() ? optional<Tensor>(s[5]) : c10::nullopt;
    const optional<Tensor> bias = s[6].defined() ? optional<Tensor>(s[6]) : c10::nullopt;
    const bool bias_grad = ctx->saved_data["bias_grad"].toBool();
    static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("fcsa::backward", "")
        .typed<std::tuple<Tensor, Tensor, Tensor, Tensor>(const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&,
                                                          const optional<Tensor>&, const optional<Tensor>&, const Tensor&, const Tensor&,
                                                          const Tensor&, const Tensor&, bool, double, bool, bool, int64_t, bool)>();
    auto g = op.call(grads[0], s[0], s[1], s[2], s[3], s[4], mask, bias, s[7], s[8], s[9], s[10], ctx->saved_data["bias_batch"].toBool(),
                     ctx->saved_data["scale"].toDouble(), ctx->saved_data["causal"].toBool(), ctx->saved_data["l2norm_qk"].toBool(),
                     ctx->saved_data["groups"].toInt(), bias_grad);
    return {std::get<0>(g), std::get<1>(g), std::get<2>(g), Tensor(), bias_grad ? std::get<3>(g) : Tensor(), Tensor(), Tensor(), Tensor(),
            Tensor(), Tensor()};
  }
};

Tensor attention_autograd(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& mask, const optional<Tensor>& attn_bias,
                          bool attn_bias_batch_dim, double scale, bool causal, bool l2norm_qk, int64_t groups) {
  // under torch.no_grad() nothing will ever call backward, whatever the inputs' requires_grad says: take the inference path
  // (no saved state, no inv_l / inverse-norm / normalised-q writes), like a Python Function's ctx.needs_input_grad would
  const bool tracked = at::GradMode::is_enabled() &&
                       (q.requires_grad() || k.requires_grad() || v.requires_grad() || (attn_bias.has_value() && attn_bias->requires_grad()));
  if (!tracked) {
    at::AutoDispatchBelowADInplaceOrView guard;
    return std::get<0>(forward(q, k, v, mask, attn_bias, attn_bias_batch_dim, scale, causal, l2norm_qk, groups, false));
  }
  return AttentionFn::apply(q, k, v, mask, attn_bias, attn_bias_batch_dim, scale, causal, l2norm_qk, groups);
}

// no autograd (inference / inputs that do not require grad): forward without saved state
Tensor attention_plain(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& mask, const optional<Tensor>& attn_bias,
                       bool attn_bias_batch_dim, double scale, bool causal, bool l2norm_qk, int64_t groups) {
  return std::get<0>(forward(q, k, v, mask, attn_bias, attn_bias_batch_dim, scale, causal, l2norm_qk, groups, false));
}


// the differentiable varlen op: the same node pattern as AttentionFn, over fcsa::varlen_forward / fcsa::varlen_backward
struct VarlenAttentionFn : public torch::autograd::Function<VarlenAttentionFn> {
  static Tensor forward(AutogradContext* ctx, const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q, const Tensor& cu_k,
                        int64_t max_q, int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups) {
    at::AutoDispatchBelowADInplaceOrView guard;
    static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("fcsa::varlen_forward", "")
        .typed<std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>(const Tensor&, const Tensor&, const Tensor&, const Tensor&,
                                                                           const Tensor&, int64_t, int64_t, double, bool, bool, int64_t, bool)>();
    auto r = op.call(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, true);
    ctx->save_for_backward({std::get<0>(r), std::get<1>(r), q, k, v, cu_q, cu_k, std::get<2>(r), std::get<3>(r), std::get<4>(r), std::get<5>(r)});
    ctx->saved_data["max_q"] = max_q;
    ctx->saved_data["max_k"] = max_k;
    ctx->saved_data["scale"] = scale;
    ctx->saved_data["causal"] = causal;
    ctx->saved_data["l2norm_qk"] = l2norm_qk;
    ctx->saved_data["groups"] = groups;
    return std::get<0>(r);
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto s = ctx->get_saved_variables();
    static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("fcsa::varlen_backward", "")
        .typed<std::tuple<Tensor, Tensor, Tensor>(const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&,
                                                  const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&,
                                                  int64_t, int64_t, double, bool, bool, int64_t)>();
    auto g = op.call(grads[0], s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], s[9], s[10], ctx->saved_data["max_q"].toInt(),
                     ctx->saved_data["max_k"].toInt(), ctx->saved_data["scale"].toDouble(), ctx->saved_data["causal"].toBool(),
                     ctx->saved_data["l2norm_qk"].toBool(), ctx->saved_data["groups"].toInt());
    return {std::get<0>(g), std::get<1>(g), std::get<2>(g), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

Tensor varlen_attention_autograd(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q, const Tensor& cu_k, int64_t max_q,
                                 int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups) {
  const bool tracked = at::GradMode::is_enabled() && (q.requires_grad() || k.requires_grad() || v.requires_grad());
  if (!tracked) {
    at::AutoDispatchBelowADInplaceOrView guard;
    return std::get<0>(varlen_forward(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, false));
  }
  return VarlenAttentionFn::apply(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups);
}

Tensor varlen_attention_plain(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q, const Tensor& cu_k, int64_t max_q,
                              int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups) {
  return std::get<0>(varlen_forward(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, false));
}


// the differentiable sliding-window ops: the same node pattern, over fcsa::window_forward / window_backward and their varlen twins
struct WindowAttentionFn : public torch::autograd::Function<WindowAttentionFn> {
  static Tensor forward(AutogradContext* ctx, const Tensor& q, const Tensor& k, const Tensor& v, double scale, bool causal, bool l2norm_qk,
                        int64_t groups, int64_t left, int64_t right) {
    at::AutoDispatchBelowADInplaceOrView guard;
    static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("fcsa::window_forward", "")
        .typed<std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>(const Tensor&, const Tensor&, const Tensor&, double, bool, bool, int64_t,
                                                                           bool, int64_t, int64_t)>();
    auto r = op.call(q, k, v, scale, causal, l2norm_qk, groups, true, left, right);
    ctx->save_for_backward({std::get<0>(r), std::get<1>(r), q, k, v, std::get<2>(r), std::get<3>(r), std::get<4>(r), std::get<5>(r)});
    ctx->saved_data["scale"] = scale;
    ctx->saved_data["causal"] = causal;
    ctx->saved_data["l2norm_qk"] = l2norm_qk;
    ctx->saved_data["groups"] = groups;
    ctx->saved_data["left"] = left;
    ctx->saved_data["right"] = right;
    return std::get<0>(r);
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto s = ctx->get_saved_variables();
    static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("fcsa::window_backward", "")
        .typed<std::tuple<Tensor, Tensor, Tensor>(const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&,
                                                  const Tensor&, const Tensor&, const Tensor&, const Tensor&, double, bool, bool, int64_t, int64_t,
                                                  int64_t)>();
    auto g = op.call(grads[0], s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], ctx->saved_data["scale"].toDouble(),
                     ctx->saved_data["causal"].toBool(), ctx->saved_data["l2norm_qk"].toBool(), ctx->saved_data["groups"].toInt(),
                     ctx->saved_data["left"].toInt(), ctx->saved_data["right"].toInt());
    return {std::get<0>(g), std::get<1>(g), std::get<2>(g), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

Tensor window_attention_plain(const Tensor& q, const Tensor& k, const Tensor& v, double scale, bool causal, bool l2norm_qk, int64_t groups,
                              int64_t left, int64_t right) {
  return std::get<0>(window_forward(q, k, v, scale, causal, l2norm_qk, groups, false, left, right));
}

Tensor window_attention_autograd(const Tensor& q, const Tensor& k, const Tensor& v, double scale, bool causal, bool l2norm_qk, int64_t groups,
                                 int64_t left, int64_t right) {
  const bool tracked = at::GradMode::is_enabled() && (q.requires_grad() || k.requires_grad() || v.requires_grad());
  if (!tracked) {
    at::AutoDispatchBelowADInplaceOrView guard;
    return window_attention_plain(q, k, v, scale, causal, l2norm_qk, groups, left, right);
  }
  return WindowAttentionFn::apply(q, k, v, scale, causal, l2norm_qk, groups, left, right);
}

struct VarlenWindowAttentionFn : public torch::autograd::Function<VarlenWindowAttentionFn> {
  static Tensor forward(AutogradContext* ctx, const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q, const Tensor& cu_k,
                        int64_t max_q, int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
    at::AutoDispatchBelowADInplaceOrView guard;
    static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("fcsa::varlen_window_forward", "")
        .typed<std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>(const Tensor&, const Tensor&, const Tensor&, const Tensor&,
                                                                           const Tensor&, int64_t, int64_t, double, bool, bool, int64_t, bool,
                                                                           int64_t, int64_t)>();
    auto r = op.call(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, true, left, right);
    ctx->save_for_backward({std::get<0>(r), std::get<1>(r), q, k, v, cu_q, cu_k, std::get<2>(r), std::get<3>(r), std::get<4>(r), std::get<5>(r)});
    ctx->saved_data["max_q"] = max_q;
    ctx->saved_data["max_k"] = max_k;
    ctx->saved_data["scale"] = scale;
    ctx->saved_data["causal"] = causal;
    ctx->saved_data["l2norm_qk"] = l2norm_qk;
    ctx->saved_data["groups"] = groups;
    ctx->saved_data["left"] = left;
    ctx->saved_data["right"] = right;
    return std::get<0>(r);
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto s = ctx->get_saved_variables();
    static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("fcsa::varlen_window_backward", "")
        .typed<std::tuple<Tensor, Tensor, Tensor>(const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&,
                                                  const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&,
                                                  int64_t, int64_t, double, bool, bool, int64_t, int64_t, int64_t)>();
    auto g = op.call(grads[0], s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], s[9], s[10], ctx->saved_data["max_q"].toInt(),
                     ctx->saved_data["max_k"].toInt(), ctx->saved_data["scale"].toDouble(), ctx->saved_data["causal"].toBool(),
                     ctx->saved_data["l2norm_qk"].toBool(), ctx->saved_data["groups"].toInt(), ctx->saved_data["left"].toInt(),
                     ctx->saved_data["right"].toInt());
    return {std::get<0>(g), std::get<1>(g), std::get<2>(g), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(),
            Tensor(), Tensor()};
  }
};

Tensor varlen_window_attention_plain(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q, const Tensor& cu_k, int64_t max_q,
                                     int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
  return std::get<0>(varlen_window_forward(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, false, left, right));
}

Tensor varlen_window_attention_autograd(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_q, const Tensor& cu_k, int64_t max_q,
                                        int64_t max_k, double scale, bool causal, bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
  const bool tracked = at::GradMode::is_enabled() && (q.requires_grad() || k.requires_grad() || v.requires_grad());
  if (!tracked) {
    at::AutoDispatchBelowADInplaceOrView guard;
    return varlen_window_attention_plain(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, left, right);
  }
  return VarlenWindowAttentionFn::apply(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, l2norm_qk, groups, left, right);
}


// ---- decoding against a key/value cache (fcsa_forward_kvcache) --------------------------------------------------------------------------
// q [B, H, N, D]; k_cache / v_cache [B, Hk, capacity, D] or, with a block_table, [num_blocks, Hk, page_size, D] (any strides with the
// feature dim contiguous: they are written in place, so they are never copied); k_new / v_new [B, Hk, N_new, D]; cache_seqlens int32 [B]
// and block_table int32 [B, max_blocks] on q's device.  Table contents are never read on the host: the call does not synchronise.
// cu_q (kvcache_varlen_forward): a ragged step -- q [total_q, H, D] packed by the int32 table cu_q [B + 1], k_new / v_new [total_q, Hk, D],
// max_seqlen_q an upper bound on the rows of a sequence; o is shaped like q.
Tensor kvcache_forward_impl(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const optional<Tensor>& k_new, const optional<Tensor>& v_new,
                            const optional<Tensor>& cache_seqlens, const optional<Tensor>& block_table, int64_t max_seqlen_k, double scale, bool causal,
                            bool l2norm_qk, int64_t groups, const fcsa_window* win, const Tensor* k_scale = nullptr, const Tensor* v_scale = nullptr,
                            const Tensor* cu_q = nullptr, int64_t max_seqlen_q = 0, Tensor* lse_out = nullptr) {
  const bool ragged = cu_q != nullptr;
  TORCH_CHECK(lse_out == nullptr || g_abi.forward_kvcache_lse != nullptr,
              "return_lse: the loaded libfcsa_hip.so does not export fcsa_forward_kvcache_lse");
  TORCH_CHECK(!ragged || (g_abi.forward_kvcache_varlen != nullptr && g_abi.forward_kvcache_varlen_ws != nullptr),
              "flash_cosine_sim_attention_varlen_with_kvcache: the loaded libfcsa_hip.so does not export fcsa_forward_kvcache_varlen");
  const bool fp8 = k_scale != nullptr;      // an e4m3fn cache with its two scale tensors (kvcache_fp8_forward)
  TORCH_CHECK(g_abi.forward_kvcache != nullptr && g_abi.forward_kvcache_ws != nullptr,
              "flash_cosine_sim_attention_with_kvcache: the loaded libfcsa_hip.so does not export fcsa_forward_kvcache");
  TORCH_CHECK(!fp8 || (g_abi.forward_kvcache_quant != nullptr && g_abi.forward_kvcache_quant_ws != nullptr),
              "flash_cosine_sim_attention_with_kvcache: the loaded libfcsa_hip.so does not export fcsa_forward_kvcache_quant");
  TORCH_CHECK(q.is_cuda(), "flash_cosine_sim_attention_with_kvcache: q and the caches must be GPU tensors (HIP kernels only)");
  auto same_dev = [&](const char* name, const Tensor& t) {
    TORCH_CHECK_VALUE(t.device() == q.device(), name, " is on ", t.device(), " but q is on ", q.device(), ": all tensors must live on q's GPU");
  };
  same_dev("k_cache", k_cache);
  same_dev("v_cache", v_cache);
  if (fp8) {
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
  Tensor cu;
  if (ragged) {
    same_dev("cu_seqlens_q", *cu_q);
    TORCH_CHECK_TYPE(cu_q->scalar_type() == at::kInt, "cu_seqlens_q must be int32");
    TORCH_CHECK_VALUE(cu_q->dim() == 1 && cu_q->numel() >= 1, "cu_seqlens_q must be 1-D with sequences + 1 entries, got ", cu_q->sizes());
    TORCH_CHECK_VALUE(max_seqlen_q >= 0 && max_seqlen_q <= INT32_MAX, "max_seqlen_q must lie in [0, 2^31), got ", max_seqlen_q);
    TORCH_CHECK_VALUE(q.size(0) * std::max<int64_t>(q.size(1), 1) <= INT32_MAX, "heads x packed rows must stay below 2^31");
    cu = cu_q->contiguous();
  }
  // ragged: N is the number of packed rows
  const int64_t B = ragged ? cu.numel() - 1 : q.size(0), H = q.size(1), N = ragged ? q.size(0) : q.size(2), D = q.size(-1), Hk = k_cache.size(1);
  TORCH_CHECK_VALUE(k_cache.size(3) == D, "query, key, value dimensions must be the same");
  TORCH_CHECK_VALUE(D == 16 || D == 32 || D == 64 || D == 96 || D == 128, "only dimensions (16, 32, 64, 96, 128) allowed for now, got ", D);
  TORCH_CHECK_VALUE(Hk >= 1 && H % Hk == 0, "k/v heads must divide q heads (", H, "), got ", Hk);
  TORCH_CHECK_VALUE(!l2norm_qk || (groups >= 1 && D % groups == 0), "groups (", groups, ") must divide the head dimension (", D, ")");
  TORCH_CHECK_VALUE(rows_ok(k_cache) && rows_ok(v_cache), "k_cache / v_cache: the feature dim must be contiguous and rows 16-byte aligned "
                    "(the caches are updated in place, so they are not copied)");
  const bool paged = block_table.has_value();
  int64_t capacity = k_cache.size(2), page = 0, num_blocks = 0;
  fcsa_kvcache kv;
  if (paged) {
    same_dev("block_table", *block_table);
    TORCH_CHECK_TYPE(block_table->scalar_type() == at::kInt, "block_table must be int32");
    TORCH_CHECK_VALUE(block_table->dim() == 2 && block_table->size(0) == B, "block_table must be [batch, max_blocks]");
    page = k_cache.size(2);
    num_blocks = k_cache.size(0);
    capacity = block_table->size(1) * page;
    TORCH_CHECK_VALUE(page > 0 && page % 16 == 0, "page_size (", page, ") must be a positive multiple of 16");
    TORCH_CHECK_VALUE(num_blocks >= 1, "a paged cache needs at least one block");
  } else {
    TORCH_CHECK_VALUE(k_cache.size(0) == B, "batch mismatch between q (", B, ") and the caches (", k_cache.size(0), ")");
  }
  TORCH_CHECK_VALUE(capacity <= INT32_MAX, "cache capacity must stay below 2^31");
  Tensor tab = paged ? block_table->contiguous() : Tensor();
  Tensor kn, vn;
  TORCH_CHECK_VALUE(k_new.has_value() == v_new.has_value(), "k_new and v_new must be given together");
  int64_t new_len = 0;
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
    new_len = ragged ? 1 : k_new->size(2);
    kn = prep(*k_new);
    vn = prep(*v_new);
  }
  Tensor sl;
  if (cache_seqlens.has_value()) {
    same_dev("cache_seqlens", *cache_seqlens);
    TORCH_CHECK_TYPE(cache_seqlens->scalar_type() == at::kInt, "cache_seqlens must be int32");
    TORCH_CHECK_VALUE(cache_seqlens->dim() == 1 && cache_seqlens->size(0) == B, "cache_seqlens must be [batch]");
    sl = cache_seqlens->contiguous();
  }
  TORCH_CHECK_VALUE(max_seqlen_k >= 0, "max_seqlen_k must be non-negative");
  c10::DeviceGuard guard(q.device());
  const Tensor q4 = prep(q);
  Tensor o = ragged ? at::empty({N, H, D}, q.options()) : at::empty({B, H, N, D}, q.options());
  fcsa_forward_args a;
  std::memset(&a, 0, sizeof(a));
  a.p.dtype = dtype_code(q.scalar_type());
  a.p.batch = (int32_t)B; a.p.heads = (int32_t)H; a.p.kv_heads = (int32_t)Hk;
  a.p.q_len = (int32_t)(ragged ? max_seqlen_q : N); a.p.k_len = (int32_t)std::min<int64_t>(max_seqlen_k, capacity); a.p.dim_head = (int32_t)D;
  a.p.causal = causal; a.p.bias_batch_dim = 0; a.p.l2norm_qk = l2norm_qk;
  a.p.groups = l2norm_qk ? (int32_t)groups : 1;
  a.p.scale = (float)scale;
  a.q = ragged ? packed3(q4) : view4(q4);
  a.o = ragged ? packed3(o) : view4(o);
  kv.k_cache = view4(k_cache);
  kv.v_cache = view4(v_cache);
  kv.capacity = (int32_t)capacity;
  kv.page_size = (int32_t)page;
  kv.num_blocks = (int32_t)num_blocks;
  kv.new_len = (int32_t)new_len;
  kv.cache_seqlens = sl.defined() ? sl.data_ptr<int32_t>() : nullptr;
  kv.block_table = paged ? tab.data_ptr<int32_t>() : nullptr;
  kv.block_table_stride = paged ? tab.size(1) : 0;
  fcsa_tensor none;
  std::memset(&none, 0, sizeof(none));
  kv.k_new = kn.defined() && new_len > 0 ? (ragged ? packed3(kn) : view4(kn)) : none;
  kv.v_new = vn.defined() && new_len > 0 ? (ragged ? packed3(vn) : view4(vn)) : none;
  fcsa_varlen seqs;
  std::memset(&seqs, 0, sizeof(seqs));
  if (ragged) {
    seqs.cu_seqlens_q = cu.data_ptr<int32_t>();
    seqs.total_q = N;
  }
  fcsa_kvcache_quant qz;
  std::memset(&qz, 0, sizeof(qz));
  Tensor ks, vs;
  if (fp8) {
    // float32 [], [Hk] or [B, Hk] on q's device: element strides of (batch, K/V head), 0 where the scale broadcasts
    auto scale_of = [&](const char* name, const Tensor& t, int64_t& s0, int64_t& s1) {
      same_dev(name, t);
      TORCH_CHECK_TYPE(t.scalar_type() == at::kFloat, name, " must be float32");
      const bool ok = t.dim() == 0 || (t.dim() == 1 && t.size(0) == Hk) || (t.dim() == 2 && t.size(0) == B && t.size(1) == Hk);
      TORCH_CHECK_VALUE(ok, name, " must have shape [], [", Hk, "] or [", B, ", ", Hk, "], got ", t.sizes());
      s0 = t.dim() == 2 ? t.stride(0) : 0;
      s1 = t.dim() == 2 ? t.stride(1) : t.dim() == 1 ? t.stride(0) : 0;
      return t;
    };
    ks = scale_of("k_scale", *k_scale, qz.k_scale_stride0, qz.k_scale_stride1);
    vs = scale_of("v_scale", *v_scale, qz.v_scale_stride0, qz.v_scale_stride1);
    qz.cache_dtype = FCSA_CACHE_E4M3;
    qz.k_scale = ks.data_ptr<float>();
    qz.v_scale = vs.data_ptr<float>();
  }
  const size_t wsb = ragged ? g_abi.forward_kvcache_varlen_ws(&a.p, &kv, &seqs, fp8 ? &qz : nullptr, win)
                     : fp8 ? g_abi.forward_kvcache_quant_ws(&a.p, &kv, &qz, win)
                         : win != nullptr ? g_abi.forward_kvcache_window_ws(&a.p, &kv, win) : g_abi.forward_kvcache_ws(&a.p, &kv);
  Tensor ws;
  if (wsb > 0) {
    ws = at::empty({(int64_t)wsb}, q.options().dtype(at::kByte));      // the caching allocator
    a.workspace = ws.data_ptr();
    a.workspace_bytes = wsb;
  }
  a.stream = stream_of(q);
  if (lse_out != nullptr) {
    // float32 [B, H, N], or [total_q, H] for a ragged step; the workspace is that of the call without it
    *lse_out = ragged ? at::empty({N, H}, q.options().dtype(at::kFloat)) : at::empty({B, H, N}, q.options().dtype(at::kFloat));
    fcsa_lse_out lo;
    lo.lse = lse_out->data_ptr<float>();
    lo.stride0 = ragged ? 0 : lse_out->stride(0);
    lo.stride1 = lse_out->stride(1);
    lo.stride2 = ragged ? lse_out->stride(0) : lse_out->stride(2);
    check(g_abi.forward_kvcache_lse(&a, &kv, ragged ? &seqs : nullptr, fp8 ? &qz : nullptr, win, &lo), "fcsa_forward_kvcache_lse");
    return o;
  }
  if (ragged) check(g_abi.forward_kvcache_varlen(&a, &kv, &seqs, fp8 ? &qz : nullptr, win), "fcsa_forward_kvcache_varlen");
  else if (fp8) check(g_abi.forward_kvcache_quant(&a, &kv, &qz, win), "fcsa_forward_kvcache_quant");
  else if (win != nullptr) check(g_abi.forward_kvcache_window(&a, &kv, win), "fcsa_forward_kvcache_window");
  else check(g_abi.forward_kvcache(&a, &kv), "fcsa_forward_kvcache");
  return o;
}
Tensor kvcache_forward(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const optional<Tensor>& k_new, const optional<Tensor>& v_new,
                       const optional<Tensor>& cache_seqlens, const optional<Tensor>& block_table, int64_t max_seqlen_k, double scale, bool causal,
                       bool l2norm_qk, int64_t groups) {
  return kvcache_forward_impl(q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, max_seqlen_k, scale, causal, l2norm_qk, groups, nullptr);
}
Tensor kvcache_window_forward(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const optional<Tensor>& k_new,
                              const optional<Tensor>& v_new, const optional<Tensor>& cache_seqlens, const optional<Tensor>& block_table,
                              int64_t max_seqlen_k, double scale, bool causal, bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
  const Win win(left, right);
  return kvcache_forward_impl(q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, max_seqlen_k, scale, causal, l2norm_qk, groups, &win.w);
}

// an e4m3fn cache: window sides of (-1, -1) are the un-windowed call
Tensor kvcache_fp8_forward(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const optional<Tensor>& k_new, const optional<Tensor>& v_new,
                           const optional<Tensor>& cache_seqlens, const optional<Tensor>& block_table, const Tensor& k_scale, const Tensor& v_scale,
                           int64_t max_seqlen_k, double scale, bool causal, bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
  const Win win(left, right);
  return kvcache_forward_impl(q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, max_seqlen_k, scale, causal, l2norm_qk, groups,
                              left == -1 && right == -1 ? nullptr : &win.w, &k_scale, &v_scale);
}

// a ragged step: packed q [total_q, H, D] with cu_seqlens_q [B + 1]; k_scale / v_scale given: an e4m3fn cache (its codes as uint8 tensors);
// window sides of (-1, -1): no window
Tensor kvcache_varlen_forward(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const Tensor& cu_seqlens_q, const optional<Tensor>& k_new,
                              const optional<Tensor>& v_new, const optional<Tensor>& cache_seqlens, const optional<Tensor>& block_table,
                              const optional<Tensor>& k_scale, const optional<Tensor>& v_scale, int64_t max_seqlen_q, int64_t max_seqlen_k, double scale,
                              bool causal, bool l2norm_qk, int64_t groups, int64_t left, int64_t right) {
  TORCH_CHECK_VALUE(k_scale.has_value() == v_scale.has_value(), "k_scale and v_scale must be given together");
  const Win win(left, right);
  return kvcache_forward_impl(q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, max_seqlen_k, scale, causal, l2norm_qk, groups,
                              left == -1 && right == -1 ? nullptr : &win.w, k_scale.has_value() ? &*k_scale : nullptr,
                              v_scale.has_value() ? &*v_scale : nullptr, &cu_seqlens_q, max_seqlen_q);
}

// Every decode route with the rows' log-sum-exp as a second result (return_lse=True): cu_seqlens_q given: a ragged step; k_scale / v_scale
// given: an e4m3fn cache (its codes as uint8 tensors); window sides of (-1, -1): no window.  o and the caches are what the op of that
// route gives, bit for bit; lse is float32 [B, H, N] ([total_q, H] for a ragged step).
std::tuple<Tensor, Tensor> kvcache_lse_forward(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const optional<Tensor>& cu_seqlens_q,
                                               const optional<Tensor>& k_new, const optional<Tensor>& v_new, const optional<Tensor>& cache_seqlens,
                                               const optional<Tensor>& block_table, const optional<Tensor>& k_scale, const optional<Tensor>& v_scale,
                                               int64_t max_seqlen_q, int64_t max_seqlen_k, double scale, bool causal, bool l2norm_qk, int64_t groups,
                                               int64_t left, int64_t right) {
  TORCH_CHECK_VALUE(k_scale.has_value() == v_scale.has_value(), "k_scale and v_scale must be given together");
  const bool windowed = !(left == -1 && right == -1);
  fcsa_window w;
  if (windowed) w = Win(left, right).w;
  Tensor lse;
  Tensor o = kvcache_forward_impl(q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, max_seqlen_k, scale, causal, l2norm_qk, groups,
                                  windowed ? &w : nullptr, k_scale.has_value() ? &*k_scale : nullptr, v_scale.has_value() ? &*v_scale : nullptr,
                                  cu_seqlens_q.has_value() ? &*cu_seqlens_q : nullptr, max_seqlen_q, &lse);
  return {o, lse};
}

// merge_attention_states: S <= 8 states (o_s [..., D] 4-D or [total_q, H, D], lse_s float32 without the feature dim) -> fresh contiguous
// (o, lse).  The states are read in place through their strides (feature dim contiguous, rows 16-byte aligned; anything else is copied).
std::tuple<Tensor, Tensor> merge_states(at::TensorList os, at::TensorList lses) {
  TORCH_CHECK(g_abi.merge_states != nullptr, "merge_attention_states: the loaded libfcsa_hip.so does not export fcsa_merge_states");
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
  const bool packed = o0.dim() == 3;
  for (int64_t d = 0; d + 1 < o0.dim(); ++d) TORCH_CHECK_VALUE(o0.size(d) <= INT32_MAX, "merge_states: sizes must stay below 2^31");
  a.size0 = packed ? 1 : (int32_t)o0.size(0);
  a.size1 = (int32_t)o0.size(packed ? 0 : 1);
  a.size2 = (int32_t)o0.size(packed ? 1 : 2);
  a.dim_head = (int32_t)D;
  a.states = (int32_t)S;
  std::vector<Tensor> keep;
  keep.reserve((size_t)S);
  const auto lead = o0.sizes().slice(0, o0.dim() - 1);
  for (int64_t s = 0; s < S; ++s) {
    const Tensor& o = os[s];
    const Tensor& l = lses[s];
    TORCH_CHECK_VALUE(o.device() == o0.device() && l.device() == o0.device(), "merge_states: every tensor must live on the first one's GPU");
    TORCH_CHECK_TYPE(o.scalar_type() == o0.scalar_type(), "merge_states: os must share a dtype, got ", o0.scalar_type(), " and ", o.scalar_type());
    TORCH_CHECK_VALUE(o.sizes() == o0.sizes(), "merge_states: os must share a shape, got ", o0.sizes(), " and ", o.sizes());
    TORCH_CHECK_TYPE(l.scalar_type() == at::kFloat, "merge_states: lses must be float32, got ", l.scalar_type());
    TORCH_CHECK_VALUE(l.sizes() == lead, "merge_states: an lse must have its o's shape without the feature dim, ", lead, ", got ", l.sizes());
    keep.push_back(prep(o));
    const Tensor& oc = keep.back();
    a.o_in[s].ptr = oc.data_ptr();
    a.o_in[s].stride0 = packed ? 0 : oc.stride(0);
    a.o_in[s].stride1 = oc.stride(packed ? 0 : 1);
    a.o_in[s].stride2 = oc.stride(packed ? 1 : 2);
    a.lse_in[s].lse = l.data_ptr<float>();
    a.lse_in[s].stride0 = packed ? 0 : l.stride(0);
    a.lse_in[s].stride1 = l.stride(packed ? 0 : 1);
    a.lse_in[s].stride2 = l.stride(packed ? 1 : 2);
  }
  Tensor o = at::empty(o0.sizes(), o0.options());
  Tensor lse = at::empty(lead, o0.options().dtype(at::kFloat));
  a.o.ptr = o.data_ptr();
  a.o.stride0 = packed ? 0 : o.stride(0);
  a.o.stride1 = o.stride(packed ? 0 : 1);
  a.o.stride2 = o.stride(packed ? 1 : 2);
  a.lse.lse = lse.data_ptr<float>();
  a.lse.stride0 = packed ? 0 : lse.stride(0);
  a.lse.stride1 = lse.stride(packed ? 0 : 1);
  a.lse.stride2 = lse.stride(packed ? 1 : 2);
  a.stream = stream_of(o0);
  if (o.numel() > 0) check(g_abi.merge_states(&a), "fcsa_merge_states");
  return {o, lse};
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
  a.forward = reinterpret_cast<decltype(a.forward)>(dlsym(h, "fcsa_forward"));
  a.backward = reinterpret_cast<decltype(a.backward)>(dlsym(h, "fcsa_backward"));
  a.forward_ws = reinterpret_cast<decltype(a.forward_ws)>(dlsym(h, "fcsa_forward_workspace_bytes"));
  a.backward_ws = reinterpret_cast<decltype(a.backward_ws)>(dlsym(h, "fcsa_backward_workspace_bytes"));
  a.needs_qn = reinterpret_cast<decltype(a.needs_qn)>(dlsym(h, "fcsa_forward_needs_qn"));
  a.last_error = reinterpret_cast<decltype(a.last_error)>(dlsym(h, "fcsa_last_error"));
  // optional: a build without packed-sequence support leaves them null, and only the varlen ops refuse to run
  a.forward_varlen = reinterpret_cast<decltype(a.forward_varlen)>(dlsym(h, "fcsa_forward_varlen"));
  a.backward_varlen = reinterpret_cast<decltype(a.backward_varlen)>(dlsym(h, "fcsa_backward_varlen"));
  a.backward_varlen_ws = reinterpret_cast<decltype(a.backward_varlen_ws)>(dlsym(h, "fcsa_backward_varlen_workspace_bytes"));
  a.forward_kvcache = reinterpret_cast<decltype(a.forward_kvcache)>(dlsym(h, "fcsa_forward_kvcache"));
  a.forward_kvcache_ws = reinterpret_cast<decltype(a.forward_kvcache_ws)>(dlsym(h, "fcsa_forward_kvcache_workspace_bytes"));
  a.forward_window = reinterpret_cast<decltype(a.forward_window)>(dlsym(h, "fcsa_forward_window"));
  a.backward_window = reinterpret_cast<decltype(a.backward_window)>(dlsym(h, "fcsa_backward_window"));
  a.backward_window_ws = reinterpret_cast<decltype(a.backward_window_ws)>(dlsym(h, "fcsa_backward_window_workspace_bytes"));
  a.forward_kvcache_window = reinterpret_cast<decltype(a.forward_kvcache_window)>(dlsym(h, "fcsa_forward_kvcache_window"));
  a.forward_kvcache_window_ws = reinterpret_cast<decltype(a.forward_kvcache_window_ws)>(dlsym(h, "fcsa_forward_kvcache_window_workspace_bytes"));
  a.forward_kvcache_quant = reinterpret_cast<decltype(a.forward_kvcache_quant)>(dlsym(h, "fcsa_forward_kvcache_quant"));
  a.forward_kvcache_quant_ws = reinterpret_cast<decltype(a.forward_kvcache_quant_ws)>(dlsym(h, "fcsa_forward_kvcache_quant_workspace_bytes"));
  a.forward_kvcache_varlen = reinterpret_cast<decltype(a.forward_kvcache_varlen)>(dlsym(h, "fcsa_forward_kvcache_varlen"));
  a.forward_kvcache_varlen_ws = reinterpret_cast<decltype(a.forward_kvcache_varlen_ws)>(dlsym(h, "fcsa_forward_kvcache_varlen_workspace_bytes"));
  a.forward_kvcache_lse = reinterpret_cast<decltype(a.forward_kvcache_lse)>(dlsym(h, "fcsa_forward_kvcache_lse"));
  a.merge_states = reinterpret_cast<decltype(a.merge_states)>(dlsym(h, "fcsa_merge_states"));
  if (!a.forward || !a.backward || !a.forward_ws || !a.backward_ws || !a.needs_qn || !a.last_error) { dlclose(h); return -2; }
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

TORCH_LIBRARY_IMPL(fcsa, Autograd, m) {
  m.impl("attention", &attention_autograd);
  m.impl("varlen_attention", &varlen_attention_autograd);
  m.impl("window_attention", &window_attention_autograd);
  m.impl("varlen_window_attention", &varlen_window_attention_autograd);
}
