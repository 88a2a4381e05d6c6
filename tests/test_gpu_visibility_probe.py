"""The visibility probe on the GPU (tests/visibility_probe.py): every kernel form on inputs whose softmax is exactly uniform, so that the
result is a pure function of the set of visible (query, key) pairs and ONE hidden or leaked pair -- at a causal diagonal, a window edge,
a sequence boundary of a packed batch, the end of a split's key window, a page boundary or a cache_seqlens clamp -- moves an element by
more than its bar.  The randn inputs of the other GPU tests leave such a pair ~1 / M of a row, inside the 16-bit bars.

Tables: window_cases.DENSE_CASES (flash_cosine_sim_attention_local), window_cases.PACKED_CASES and varlen_form_cases.CASES
(flash_cosine_sim_attention_varlen), visibility_probe.DENSE_PLAIN_CASES (flash_cosine_sim_attention with a key mask or causal, every dense
form: test_visibility_probe_cpu.py checks the launches), window_cases.DECODE_CASES and visibility_probe.DECODE_PLAIN_CASES (the cache calls
with return_lse=True: lse decodes the count of visible keys), visibility_probe.PREFIX_CASES (the shared-prefix step),
visibility_probe.BIAS_CASES (flash_cosine_sim_attention with an attn_bias of -inf / per-row constants that requires grad: the BIAS = 1
kernels and bwd_dbias_kernel, d_bias = R dS element by element).  A table case with
l2norm groups g > 1 runs with groups = 1 and scale * g (same bound, exponent regime and form: the form never depends on the grouping).
Bars: derived in visibility_probe.py's docstring -- o 2 eps, gradients 4 eps relative to the terms' absolute sum, float32 the rtol of
tests/tolerances.py, lse 4 eps_f32 max(1, |lse|) -- not calibrated.  Which (case, quantity) pairs cannot decide a single pair in 8
significant bits is computed on the CPU (test_visibility_probe_cpu.py); they are compared at the same bars here.
Each test is one call plus one backward; the float64 expectation is computed once per distinct visibility matrix."""
import pytest
import torch

import visibility_probe as VP
import window_cases as W

pytestmark = pytest.mark.gpu


def _judge(dtype, name, comparisons):
    fails = VP.judge(dtype, name, comparisons)
    assert not fails, (name, fails)


@pytest.mark.parametrize("name,dtype,D,B,H,Hk,N,M,left,right,kw", W.DENSE_CASES, ids=[c[0] for c in W.DENSE_CASES])
def test_probe_local(name, dtype, D, B, H, Hk, N, M, left, right, kw):
    scale, l2 = VP.probe_scale(kw)
    _judge(dtype, name, VP.run_dense(dtype, D, B, H, Hk, N, M, scale, l2, "cuda", kw.get("causal", False), (left, right), seed=len(name)))


PACKED = VP.packed_cases()


@pytest.mark.parametrize("name,dtype,D,lq,lk,H,Hk,mx,kw,window", PACKED, ids=[c[0] for c in PACKED])
def test_probe_packed(name, dtype, D, lq, lk, H, Hk, mx, kw, window):
    """the empty and one-row spans of the ragged core included"""
    scale, l2 = VP.probe_scale(kw)
    _judge(dtype, name, VP.run_packed(dtype, D, H, Hk, lq, lk, scale, l2, "cuda", kw.get("causal", False), window, mx, seed=len(name)))


@pytest.mark.parametrize("case", VP.DENSE_PLAIN_CASES, ids=[c[0] for c in VP.DENSE_PLAIN_CASES])
def test_probe_dense(case):
    """every dense form (the D = 32 64-rows-per-wave forward: forward only); the debug knobs (64-rows-per-wave D = 128 forward off / on, group sweep off / wherever compiled) are restored"""
    from flash_cosine_sim_attention_amd import _lib
    name, dtype, D, B, H, Hk, N, M, variant, kw, ff, kf, grads = case
    scale, l2 = VP.probe_scale(kw)
    _, mask, causal = VP.dense_plain_vis(case)
    prev = _lib.forward_form(ff), _lib.kv_group_form(kf)
    try:
        got = VP.run_dense(dtype, D, B, H, Hk, N, M, scale, l2, "cuda", causal, None, mask, seed=len(name), grads=grads)
        torch.cuda.synchronize()
    finally:
        _lib.forward_form(prev[0]), _lib.kv_group_form(prev[1])
    _judge(dtype, name, got)


@pytest.mark.parametrize("case", VP.BIAS_CASES, ids=[c[0] for c in VP.BIAS_CASES])
def test_probe_bias(case):
    """attn_bias as a per-(slice, query, key) visibility (-inf / a per-row constant): o, dq, dk, dv and d_bias of every kernel form a
    problem with a bias can launch, per-head and per-batch, at every read and write path of the bias (M % 8, M % 4, odd, 31 / 33, a
    misaligned pointer).  d_bias is R dS element by element: exactly 0 on every hidden pair, above 16 tiny on every other."""
    name, dtype = case[:2]
    got, bias, geom = VP.run_dense_bias(case, "cuda")
    torch.cuda.synchronize()
    _judge(dtype, name, got)
    assert bias.grad.dtype == bias.dtype and bias.grad.shape == bias.shape
    assert bool(torch.isfinite(bias.grad).all())
    hidden = torch.as_tensor(~geom).to(bias.grad.device).expand_as(bias.grad)
    assert bool((bias.grad[hidden] == 0).all()), "d_bias is not exactly 0 on a pair that causal or the key mask hides"


DECODE = VP.decode_cases()


@pytest.mark.parametrize("name,dtype,D,H,Hk,N,cap,page,lens,n_new,counts,causal,fp8,kw,window", DECODE, ids=[c[0] for c in DECODE])
def test_probe_decode(name, dtype, D, H, Hk, N, cap, page, lens, n_new, counts, causal, fp8, kw, window):
    """contiguous and paged (shuffled table) caches, appends (the appended keys carry their position's class, the slots they land in held
    a wrong one), cache_seqlens of 0, 1, page -+ 1 and the capacity, N of 1, 5, 17, ragged steps, fp8 caches (1.0 and the powers of two
    are exact e4m3 codes; k_scale, v_scale powers of two), 2048 keys in up to 16 splits and a length that ends inside a 32-key block"""
    scale, l2 = VP.probe_scale(kw)
    _judge(dtype, name, VP.run_decode(dtype, D, H, Hk, N, cap, page, lens, n_new, counts, causal, fp8, scale, l2, "cuda", window,
                                      kw.get("append", True), seed=len(name)))


@pytest.mark.parametrize("case", VP.PREFIX_CASES, ids=[c[0] for c in VP.PREFIX_CASES])
def test_probe_shared_prefix(case):
    """rectangular and packed, causal and not, prefix lengths of 1, page - 1 and page + 1, a sequence with N_b = L_b + 1"""
    _judge(case[1], case[0], VP.run_prefix(*case[1:], "cuda", seed=len(case[0])))
