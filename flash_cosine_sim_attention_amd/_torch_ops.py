"""Loads the compiled PyTorch binding (`_fcsa_torch.so`, csrc/fcsa_torch.cpp) and registers what the dispatcher needs besides
the kernels: fake (meta) implementations so that `torch.compile` can trace `torch.ops.fcsa.forward / backward` without running
them.  The binding is host-only C++ over the C ABI of libfcsa_hip.so (include/fcsa.h); it replaces the reference's pybind
module (flash_cosine_sim_attention_cuda.cu:1928-1933).  There is no fallback: a missing binding raises ImportError."""
from __future__ import annotations

import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
BINDING_PATH = os.path.join(_HERE, "_fcsa_torch.so")
_loaded = False


def load():
    global _loaded
    if _loaded:
        return torch.ops.fcsa
    if not os.path.exists(BINDING_PATH):
        raise ImportError(f"{BINDING_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or `make -C flash_cosine_sim_attention_amd/csrc`).  There is no non-HIP fallback for GPU tensors.")
    torch.ops.load_library(BINDING_PATH)
    alt = os.environ.get("FCSA_LIB")          # measurement only: route the ops to another build of the same C ABI (A/B runs)
    if alt:
        import ctypes
        if ctypes.CDLL(BINDING_PATH).fcsa_torch_use_library(alt.encode()) != 0:
            raise ImportError(f"FCSA_LIB={alt}: not a loadable build of libfcsa_hip.so")
    _register_fakes()
    _loaded = True
    return torch.ops.fcsa


def _canon_dims(q, k):
    merged = q.dim() == 3
    B, H, N, D = (q.shape[0], 1, q.shape[1], q.shape[2]) if merged else q.shape
    Hk, M = (1, k.shape[1]) if k.dim() == 3 else (k.shape[1], k.shape[2])
    return merged, B, H, Hk, N, M, D


def _saved_state(q, rows_q, rows_k, D, l2norm_qk, groups, need_backward):
    """(inv_l, qn, kn, rq, rk) as the binding returns them; rows_q / rows_k: the leading dims of the q-side / k-side saved tensors --
    (B, H, N) / (B, Hk, M) for a dense call, (H, total_q) / (Hk, total_k) for packed rows (a batch-1 problem).  Empty where not produced."""
    f32 = dict(device=q.device, dtype=torch.float32)
    none32, none = q.new_empty((0,), dtype=torch.float32), q.new_empty((0,))
    inv_l = torch.empty(rows_q, **f32) if need_backward else none32
    # (an inference call of the 16-bit kernels saves no normalised q: fcsa_forward_needs_qn, include/fcsa.h)
    blocks = (D // groups) // 8          # fcsa_capi.hip log2_blocks_per_group: 8 * 2^k features per group, or ONE group of any width (D = 96)
    fusable = D % groups == 0 and (D // groups) % 8 == 0 and (blocks & (blocks - 1) == 0 or groups == 1)
    qn = q.new_empty((*rows_q, D)) if (l2norm_qk and (need_backward or q.dtype == torch.float32 or not fusable)) else none
    kn = q.new_empty((*rows_k, D)) if l2norm_qk else none
    rq = torch.empty((*rows_q, groups), **f32) if (l2norm_qk and need_backward) else none32
    rk = torch.empty((*rows_k, groups), **f32) if (l2norm_qk and need_backward) else none32
    return inv_l, qn, kn, rq, rk


# ops whose one result is shaped like q, their first argument (the cache ops mutate their caches in place: declared by the schema's
# (a!) / (b!)), and ops that return (dq, dk, dv) shaped like (q, k, v), which follow (d_out, o, inv_l)
_LIKE_Q = ("attention", "varlen_attention", "window_attention", "varlen_window_attention", "kvcache_forward", "kvcache_window_forward",
           "kvcache_fp8_forward", "kvcache_varlen_forward")
_LIKE_QKV = ("varlen_backward", "window_backward", "varlen_window_backward")
# the cache ops that return (o, lse), by qualified name (the later ones live in namespaces of their own): o shaped like q, their first
# argument; lse float32 [B, H, N], or [total_q, H] for a ragged step (q [total_q, H, D])
_O_LSE = ("fcsa::kvcache_lse_forward", "fcsa_prefill::kvcache_prefill_forward", "fcsa_step::kvcache_step_forward",
          "fcsa_tree::kvcache_tree_forward", "fcsa_alibi::kvcache_alibi_forward")


def _register_fakes():
    for op in _LIKE_Q:
        @torch.library.register_fake("fcsa::" + op)
        def _(*args):
            return args[0].new_empty(args[0].shape)

    for op in _LIKE_QKV:
        @torch.library.register_fake("fcsa::" + op)
        def _(*args):
            return tuple(t.new_empty(t.shape) for t in args[3:6])

    @torch.library.register_fake("fcsa::forward")
    def _(q, k, v, mask, attn_bias, attn_bias_batch_dim, scale, causal, l2norm_qk, groups, need_backward):
        merged, B, H, Hk, N, M, D = _canon_dims(q, k)
        return (q.new_empty(q.shape), *_saved_state(q, (B, H, N), (B, Hk, M), D, l2norm_qk, groups, need_backward))

    @torch.library.register_fake("fcsa::varlen_forward")
    def _(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, scale, causal, l2norm_qk, groups, need_backward):
        return (q.new_empty(q.shape), *_saved_state(q, (q.shape[1], q.shape[0]), (k.shape[1], k.shape[0]), q.shape[2], l2norm_qk, groups, need_backward))

    # sliding-window ops: the shapes of their un-windowed twins
    @torch.library.register_fake("fcsa::window_forward")
    def _(q, k, v, scale, causal, l2norm_qk, groups, need_backward, window_left, window_right):
        B, H, N, D = q.shape
        return (q.new_empty(q.shape), *_saved_state(q, (B, H, N), (B, k.shape[1], k.shape[2]), D, l2norm_qk, groups, need_backward))

    @torch.library.register_fake("fcsa::varlen_window_forward")
    def _(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, scale, causal, l2norm_qk, groups, need_backward, window_left,
          window_right):
        return (q.new_empty(q.shape), *_saved_state(q, (q.shape[1], q.shape[0]), (k.shape[1], k.shape[0]), q.shape[2], l2norm_qk, groups, need_backward))

    for op in _O_LSE:
        @torch.library.register_fake(op)
        def _(q, *args):
            return q.new_empty(q.shape), q.new_empty(q.shape[:-1], dtype=torch.float32)

    @torch.library.register_fake("fcsa_tree::kvcache_compact")
    def _(k_cache, v_cache, cache_seqlens, accepted, num_accepted, block_table):
        return None

    @torch.library.register_fake("fcsa::merge_states")
    def _(os, lses):
        return os[0].new_empty(os[0].shape), os[0].new_empty(os[0].shape[:-1], dtype=torch.float32)

    # attention states for training (namespace fcsa_state): lse float32 [B, H, N], packed [total_q, H]; the saved state always
    def _state_rows(q, k):
        packed = q.dim() == 3
        return ((q.shape[1], q.shape[0]), (k.shape[1], k.shape[0])) if packed else (tuple(q.shape[:3]), tuple(k.shape[:3]))

    @torch.library.register_fake("fcsa_state::attention_state_forward")
    def _(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, scale, causal, l2norm_qk, groups, window_left, window_right):
        rows_q, rows_k = _state_rows(q, k)
        return (q.new_empty(q.shape), q.new_empty(q.shape[:-1], dtype=torch.float32),
                *_saved_state(q, rows_q, rows_k, q.shape[-1], l2norm_qk, groups, True))

    @torch.library.register_fake("fcsa_state::attention_state")
    def _(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, scale, causal, l2norm_qk, groups, window_left, window_right):
        return q.new_empty(q.shape), q.new_empty(q.shape[:-1], dtype=torch.float32)

    @torch.library.register_fake("fcsa_state::attention_state_backward")
    def _(d_out, d_lse, o, inv_l, q, k, v, cu_seqlens_q, cu_seqlens_k, qn, kn, rq, rk, max_seqlen_q, max_seqlen_k, scale, causal, l2norm_qk,
          groups, window_left, window_right):
        return q.new_empty(q.shape), k.new_empty(k.shape), v.new_empty(v.shape)

    # the training calls with a linear position bias (namespace fcsa_alibi_train): the shapes of the fcsa_state ops without the lse
    @torch.library.register_fake("fcsa_alibi_train::forward")
    def _(q, k, v, alibi_slopes, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, scale, causal, l2norm_qk, groups, window_left,
          window_right, need_backward):
        rows_q, rows_k = _state_rows(q, k)
        return (q.new_empty(q.shape), *_saved_state(q, rows_q, rows_k, q.shape[-1], l2norm_qk, groups, need_backward))

    @torch.library.register_fake("fcsa_alibi_train::attention")
    def _(q, k, v, alibi_slopes, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, scale, causal, l2norm_qk, groups, window_left,
          window_right):
        return q.new_empty(q.shape)

    @torch.library.register_fake("fcsa_alibi_train::backward")
    def _(d_out, o, inv_l, q, k, v, alibi_slopes, cu_seqlens_q, cu_seqlens_k, qn, kn, rq, rk, max_seqlen_q, max_seqlen_k, scale, causal,
          l2norm_qk, groups, window_left, window_right):
        return q.new_empty(q.shape), k.new_empty(k.shape), v.new_empty(v.shape)

    @torch.library.register_fake("fcsa_state::merge_state")
    def _(os, lses):
        return os[0].new_empty(os[0].shape), os[0].new_empty(os[0].shape[:-1], dtype=torch.float32)

    @torch.library.register_fake("fcsa_state::merge_state_backward")
    def _(d_o, d_lse, os, lses):
        return ([o.new_empty(o.shape) for o in os], [o.new_empty(o.shape[:-1], dtype=torch.float32) for o in os])

    @torch.library.register_fake("fcsa::backward")
    def _(d_out, o, inv_l, q, k, v, mask, attn_bias, qn, kn, rq, rk, attn_bias_batch_dim, scale, causal, l2norm_qk, groups,
          need_bias_grad):
        db = attn_bias.new_empty(attn_bias.shape) if (attn_bias is not None and need_bias_grad) else q.new_empty((0,))
        return q.new_empty(q.shape), k.new_empty(k.shape), v.new_empty(v.shape), db
