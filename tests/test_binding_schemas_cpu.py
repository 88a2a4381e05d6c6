"""The operator surface of the compiled PyTorch binding (csrc/fcsa_torch.cpp), pinned: the set of ops under `torch.ops.fcsa`, the
schema of each, and which of them carry an Autograd kernel.  No GPU is needed: loading the binding registers the ops.

SCHEMAS is a literal record of the binding as it stood before its host front ends were folded into one per call family.  It is never
regenerated from the code under test: an op added on purpose gets its line added by hand, and any other difference is a regression."""
import os

import pytest
import torch

SCHEMAS = {
    "attention":
        "fcsa::attention(Tensor q, Tensor k, Tensor v, Tensor? mask, Tensor? attn_bias, bool attn_bias_batch_dim, float scale, bool causal, bool l2norm_qk, int groups) -> Tensor",
    "backward":
        "fcsa::backward(Tensor d_out, Tensor o, Tensor inv_l, Tensor q, Tensor k, Tensor v, Tensor? mask, Tensor? attn_bias, Tensor qn, Tensor kn, Tensor rq, Tensor rk, bool attn_bias_batch_dim, float scale, bool causal, bool l2norm_qk, int groups, bool need_bias_grad) -> (Tensor, Tensor, Tensor, Tensor)",
    "forward":
        "fcsa::forward(Tensor q, Tensor k, Tensor v, Tensor? mask, Tensor? attn_bias, bool attn_bias_batch_dim, float scale, bool causal, bool l2norm_qk, int groups, bool need_backward) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)",
    "kvcache_forward":
        "fcsa::kvcache_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor? k_new, Tensor? v_new, Tensor? cache_seqlens, Tensor? block_table, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups) -> Tensor",
    "kvcache_fp8_forward":
        "fcsa::kvcache_fp8_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor? k_new, Tensor? v_new, Tensor? cache_seqlens, Tensor? block_table, Tensor k_scale, Tensor v_scale, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> Tensor",
    "kvcache_lse_forward":
        "fcsa::kvcache_lse_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor? cu_seqlens_q, Tensor? k_new, Tensor? v_new, Tensor? cache_seqlens, Tensor? block_table, Tensor? k_scale, Tensor? v_scale, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> (Tensor, Tensor)",
    "kvcache_varlen_forward":
        "fcsa::kvcache_varlen_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cu_seqlens_q, Tensor? k_new, Tensor? v_new, Tensor? cache_seqlens, Tensor? block_table, Tensor? k_scale, Tensor? v_scale, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> Tensor",
    "kvcache_window_forward":
        "fcsa::kvcache_window_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor? k_new, Tensor? v_new, Tensor? cache_seqlens, Tensor? block_table, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> Tensor",
    "merge_states":
        "fcsa::merge_states(Tensor[] os, Tensor[] lses) -> (Tensor, Tensor)",
    "varlen_attention":
        "fcsa::varlen_attention(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups) -> Tensor",
    "varlen_backward":
        "fcsa::varlen_backward(Tensor d_out, Tensor o, Tensor inv_l, Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, Tensor qn, Tensor kn, Tensor rq, Tensor rk, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups) -> (Tensor, Tensor, Tensor)",
    "varlen_forward":
        "fcsa::varlen_forward(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, bool need_backward) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)",
    "varlen_window_attention":
        "fcsa::varlen_window_attention(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> Tensor",
    "varlen_window_backward":
        "fcsa::varlen_window_backward(Tensor d_out, Tensor o, Tensor inv_l, Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, Tensor qn, Tensor kn, Tensor rq, Tensor rk, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> (Tensor, Tensor, Tensor)",
    "varlen_window_forward":
        "fcsa::varlen_window_forward(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, bool need_backward, int window_left, int window_right) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)",
    "window_attention":
        "fcsa::window_attention(Tensor q, Tensor k, Tensor v, float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> Tensor",
    "window_backward":
        "fcsa::window_backward(Tensor d_out, Tensor o, Tensor inv_l, Tensor q, Tensor k, Tensor v, Tensor qn, Tensor kn, Tensor rq, Tensor rk, float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> (Tensor, Tensor, Tensor)",
    "window_forward":
        "fcsa::window_forward(Tensor q, Tensor k, Tensor v, float scale, bool causal, bool l2norm_qk, int groups, bool need_backward, int window_left, int window_right) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)",
}

# the differentiable ops: a C++ autograd node over their forward / backward pair
DIFFERENTIABLE = {"attention", "varlen_attention", "window_attention", "varlen_window_attention"}


@pytest.fixture(scope="module")
def fc():
    from flash_cosine_sim_attention_amd import _lib, _torch_ops
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_torch_ops.BINDING_PATH):
        _lib.build()
    return _torch_ops.load()


def _registered():
    return {n.split("::", 1)[1].split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith("fcsa::")}


def test_op_set(fc):
    assert _registered() == set(SCHEMAS)


@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_schema(fc, name):
    op = getattr(fc, name)
    assert op.overloads() == ["default"]
    assert str(op.default._schema) == SCHEMAS[name]


def test_autograd_kernels(fc):
    assert DIFFERENTIABLE <= set(SCHEMAS)
    with_kernel = {n for n in SCHEMAS if torch._C._dispatch_has_kernel_for_dispatch_key("fcsa::" + n, "Autograd")}
    assert with_kernel == DIFFERENTIABLE
