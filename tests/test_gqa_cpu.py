"""Grouped-query attention (K/V heads Hk dividing the query heads H) on the host side: what the C ABI accepts and how much workspace it
asks for, the debug knob of the dK/dV form, and the CPU paths of the public API (`flash_cosine_sim_attention` on CPU tensors and
`plain_cosine_sim_attention`).  No kernel is launched by any call here: the C ABI calls are zero-size problems or size queries."""
import ctypes as C
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from flash_cosine_sim_attention_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _problem(**kw):
    from flash_cosine_sim_attention_amd import _lib
    d = dict(dtype=_lib.FCSA_BF16, batch=2, heads=8, kv_heads=2, q_len=100, k_len=120, dim_head=64, causal=0,
             bias_batch_dim=0, l2norm_qk=0, groups=1, scale=8.0)
    d.update(kw)
    return _lib.Problem(*[d[f[0]] for f in _lib.Problem._fields_])


def _zero_rows_forward(lib, prob):
    """fcsa_forward on a problem without query rows: validation runs, nothing is launched, no pointer is read"""
    from flash_cosine_sim_attention_amd import _lib
    t = _lib.Tensor(None, 0, 0, 0)
    args = _lib.ForwardArgs(prob, t, t, t, t, None, None, None, _lib.NormState(None, None, None, None), None, 0, None)
    return lib.fcsa_forward(C.byref(args))


def test_cabi_accepts_divisor_kv_heads(lib):
    assert _zero_rows_forward(lib, _problem(heads=8, kv_heads=2, q_len=0)) == 0
    assert _zero_rows_forward(lib, _problem(heads=8, kv_heads=4, q_len=0, dtype=0)) == 0
    assert _zero_rows_forward(lib, _problem(heads=12, kv_heads=3, q_len=0, dtype=1)) == 0
    # the two ends keep working
    assert _zero_rows_forward(lib, _problem(heads=8, kv_heads=8, q_len=0)) == 0
    assert _zero_rows_forward(lib, _problem(heads=8, kv_heads=1, q_len=0)) == 0


@pytest.mark.parametrize("heads,kv_heads", [(8, 3), (2, 3), (8, 0), (8, -2)])
def test_cabi_rejects_non_divisor_kv_heads(lib, heads, kv_heads):
    rc = _zero_rows_forward(lib, _problem(heads=heads, kv_heads=kv_heads, q_len=0))
    assert rc == -1 and b"kv_heads" in lib.fcsa_last_error()


def test_backward_workspace_of_grouped_problem(lib):
    """delta [B,H,N] f32, then per-QUERY-head f32 dk / dv slabs [B,H,M,D] for the slab route (the finalize kernel sums each K/V head's
    group).  The group-sweep kernel needs no slab, but a launch with an attn_bias takes the slab route, so the size keeps them."""
    from flash_cosine_sim_attention_amd import _lib
    al = lambda x: (x + 255) // 256 * 256
    B, H, Hk, N, M, D = 2, 8, 2, 100, 120, 64
    slabs = al(B * H * N * 4) + 2 * al(B * H * M * D * 4)
    prev = _lib.kv_group_form(1)
    try:
        for form in (0, 1, 2):
            _lib.kv_group_form(form)
            for dtype in (0, 1, 2):
                p = _problem(batch=B, heads=H, kv_heads=Hk, q_len=N, k_len=M, dim_head=D, dtype=dtype)
                assert lib.fcsa_backward_workspace_bytes(C.byref(p)) == slabs, (form, dtype)
            p = _problem(batch=B, heads=H, kv_heads=Hk, q_len=N, k_len=M, dim_head=D, l2norm_qk=1)
            assert lib.fcsa_backward_workspace_bytes(C.byref(p)) == slabs
        # Hk == H is unchanged: delta only
        p = _problem(batch=B, heads=H, kv_heads=H, q_len=N, k_len=M, dim_head=D)
        assert lib.fcsa_backward_workspace_bytes(C.byref(p)) == al(B * H * N * 4)
    finally:
        _lib.kv_group_form(prev)


def test_kv_group_form_knob_round_trips():
    from flash_cosine_sim_attention_amd import _lib
    start = _lib.kv_group_form(-1)
    assert start == 1                                   # automatic by default
    try:
        assert _lib.kv_group_form(0) == 1
        assert _lib.kv_group_form(-1) == 0
        assert _lib.kv_group_form(2) == 0
        assert _lib.kv_group_form(-5) == 2              # negative: query only
        assert _lib.kv_group_form(1) == 2
    finally:
        _lib.kv_group_form(start)
    assert _lib.kv_group_form(-1) == start


def test_debug_string_mentions_grouped_kv(lib):
    buf = C.create_string_buffer(2048)
    assert lib.fcsa_debug(buf, len(buf)) == 4           # ABI version unchanged
    assert b"kv_heads=divisors of heads" in buf.value


def _inputs(B, H, Hk, N, M, D, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, N, D, generator=g).to(dtype)
    k = torch.randn(B, Hk, M, D, generator=g).to(dtype)
    v = torch.randn(B, Hk, M, D, generator=g).to(dtype)
    return q, k, v


@pytest.mark.parametrize("Hk", [2, 4])
@pytest.mark.parametrize("causal", [False, True])
def test_cpu_operator_equals_expanded_kv(Hk, causal):
    import flash_cosine_sim_attention_amd as F
    B, H, N, M, D = 2, 8, 37, 53, 32
    q, k, v = _inputs(B, H, Hk, N, M, D)
    ke, ve = k.repeat_interleave(H // Hk, dim=1), v.repeat_interleave(H // Hk, dim=1)
    for kw in (dict(causal=causal), dict(causal=causal, groups=4), dict(causal=causal, l2norm_qk=False, scale=0.3)):
        got = F.flash_cosine_sim_attention(q, k, v, **kw)
        ref = F.flash_cosine_sim_attention(q, ke, ve, **kw)
        assert got.shape == (B, H, N, D)
        torch.testing.assert_close(got, ref, rtol=1.2e-7, atol=1e-7)
        plain = F.plain_cosine_sim_attention(q, k, v, **kw)
        plain_ref = F.plain_cosine_sim_attention(q, ke, ve, **kw)
        torch.testing.assert_close(plain, plain_ref, rtol=1.2e-7, atol=1e-7)
        # and the two CPU implementations agree with each other
        torch.testing.assert_close(got, plain, rtol=2e-5, atol=2e-5)


def test_cpu_operator_grouped_with_mask_and_bias():
    import flash_cosine_sim_attention_amd as F
    B, H, Hk, N, M, D = 2, 6, 3, 20, 33, 16
    q, k, v = _inputs(B, H, Hk, N, M, D, seed=3)
    g = torch.Generator().manual_seed(7)
    mask = torch.rand(B, M, generator=g) > 0.3
    ke, ve = k.repeat_interleave(H // Hk, dim=1), v.repeat_interleave(H // Hk, dim=1)
    for bias, batch_dim in ((torch.randn(H, N, M, generator=g), False), (torch.randn(B, N, M, generator=g), True)):
        kw = dict(mask=mask, attn_bias=bias, attn_bias_batch_dim=batch_dim)
        torch.testing.assert_close(F.flash_cosine_sim_attention(q, k, v, **kw), F.flash_cosine_sim_attention(q, ke, ve, **kw),
                                   rtol=1.2e-7, atol=1e-7)
        torch.testing.assert_close(F.plain_cosine_sim_attention(q, k, v, **kw), F.plain_cosine_sim_attention(q, ke, ve, **kw),
                                   rtol=1.2e-7, atol=1e-7)


def test_cpu_operator_grouped_16bit():
    import flash_cosine_sim_attention_amd as F
    q, k, v = _inputs(1, 4, 2, 24, 40, 64, dtype=torch.bfloat16, seed=5)
    ke, ve = k.repeat_interleave(2, dim=1), v.repeat_interleave(2, dim=1)
    assert torch.equal(F.flash_cosine_sim_attention(q, k, v, causal=True), F.flash_cosine_sim_attention(q, ke, ve, causal=True))


@pytest.mark.parametrize("H,Hk", [(8, 3), (2, 3), (6, 4)])
def test_cpu_non_divisor_kv_heads_is_an_error(H, Hk):
    import flash_cosine_sim_attention_amd as F
    q, k, v = _inputs(1, H, Hk, 8, 8, 16)
    with pytest.raises(ValueError, match="k/v heads must divide q heads"):
        F.flash_cosine_sim_attention(q, k, v)
    with pytest.raises(ValueError, match="k/v heads must divide q heads"):
        F.plain_cosine_sim_attention(q, k, v)


def test_cpu_merged_batch_heads_still_needs_3d_kv():
    import flash_cosine_sim_attention_amd as F
    q = torch.randn(4, 8, 16)
    k = torch.randn(2, 2, 8, 16)
    with pytest.raises(ValueError, match="3 dimensions"):
        F.flash_cosine_sim_attention(q, k, k)
