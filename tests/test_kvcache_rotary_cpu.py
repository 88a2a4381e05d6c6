"""flash_cosine_sim_attention_rotary_with_kvcache without a GPU: without tables it is the step call; bad tables are refused in Python and
at the C ABI before any launch; the CPU path agrees with the float64 oracle on float64-rotated q and k_new."""
import ctypes as C

import numpy as np
import pytest
import torch

import flash_cosine_sim_attention_amd as F
from flash_cosine_sim_attention_amd import _lib
from rotary_reference import rotate, tables
from test_kvcache_alibi_cpu import _band, _bits
from test_kvcache_prefill_cpu import _problem

rotary = F.flash_cosine_sim_attention_rotary_with_kvcache
COUNTS, CACHED = [1, 0, 5, 40], [0, 17, 30, 3]
H, HK, D, CAP = 6, 2, 64, 64


def test_without_tables_it_is_the_step_call_and_bad_tables_are_refused():
    q, kc, vc, cu, kn, vn, lens, _ = _problem(torch.bfloat16, D, H, HK, COUNTS, CACHED, CAP, 0, 3)
    outs = [fn(q, kc.clone(), vc.clone(), cu, kn, vn, cache_seqlens=lens, causal=True, return_lse=True, chunk_rows=7)
            for fn in (rotary, F.flash_cosine_sim_attention_step_with_kvcache)]
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*outs))
    cos, sin = tables(CAP, D)
    call = lambda c, s, t=(q, kc, vc, kn, vn): rotary(t[0], t[1].clone(), t[2].clone(), cu, t[3], t[4], cache_seqlens=lens, rotary_cos=c, rotary_sin=s)
    for exc, match, args in ((ValueError, "given together", (cos, None)), (TypeError, "float32", (cos.double(), sin.double())),
                             (ValueError, "same shape", (cos, sin[:-1])), (ValueError, "rotary_dim", (cos[:, :16], sin[:, :16])),
                             (ValueError, "finite", (cos, torch.full_like(sin, float("nan")))),
                             (ValueError, "beyond the 40 rows", (cos[:40], sin[:40])),
                             (TypeError, "float16 or bfloat16", (cos, sin, [t.float() for t in (q, kc, vc, kn, vn)]))):
        with pytest.raises(exc, match=match):
            call(*args)
    q32, k32, v32, _, kn32, vn32, _, _ = _problem(torch.bfloat16, 32, H, HK, COUNTS, CACHED, CAP, 0, 5)
    with pytest.raises(ValueError, match="head dimensions 64 and 128"):
        call(cos[:, :16], sin[:, :16], (q32, k32, v32, kn32, vn32))


def test_c_entry_refuses_before_any_launch():
    lib = _lib.load()
    assert "fcsa_forward_kvcache_rotary" in _lib.EXPORTS and lib.fcsa_debug(None, 0) == 4 == _lib.ABI_VERSION      # additive
    assert C.sizeof(_lib.Rotary) == 48
    fa, kv, seqs, st = _lib.ForwardArgs(), _lib.KvCache(), _lib.Varlen(), _lib.KvCacheStep()
    kv.capacity, seqs.total_q, seqs.cu_seqlens_q = 64, 5, 4096
    fa.q = fa.o = _lib.Tensor(1 << 20, 0, 64, 8 * 64)                                  # (synthetic addresses: every call is refused before any launch)
    kv.k_cache = kv.v_cache = _lib.Tensor(1 << 24, 2 * 64 * 64, 64 * 64, 64)

    def call(ro, dtype=torch.bfloat16, dim=64, step=st):
        fa.p = _lib.problem(dtype, (2, 8, 2, 4, 64, dim), True, False, True, 1, 8.0)
        return lib.fcsa_forward_kvcache_rotary(C.byref(fa), C.byref(kv), C.byref(seqs), None, None, C.byref(step), ro, None), lib.fcsa_last_error()
    good = dict(cos=1 << 22, sin=1 << 23, rows=64, stride_row=32, rotary_dim=64, interleaved=0, reserved=0)
    R = lambda **kw: C.byref(_lib.Rotary(**{**good, **kw}))
    unsupported, msg = call(R(), dtype=torch.float32)
    assert unsupported not in (0, -1) and b"float32 is not supported" in msg
    rc, msg = call(R(), dim=32)
    assert rc == unsupported and b"dim_head 32 is not supported" in msg
    for ro, text in ((None, b"null argument"), (R(cos=None), b"null pointer"), (R(sin=None), b"null pointer"), (R(cos=(1 << 22) + 4), b"16-byte aligned"),
                     (R(stride_row=33), b"16-byte aligned"), (R(reserved=9), b"reserved"), (R(rows=0), b"rows"), (R(rotary_dim=32), b"rotary_dim"),
                     (R(rotary_dim=128), b"rotary_dim 128 is not supported at dim_head 64"), (R(interleaved=2), b"flag")):
        rc, msg = call(ro)
        assert rc == -1 and text in msg, text
    rc, msg = call(R(), step=_lib.KvCacheStep(128, 2, -1, 0, 0))      # with good tables the step call's own checks follow
    assert rc == -1 and b"are flags" in msg


@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("kw", [dict(causal=True), dict(causal=False, window_size=(9, 2), groups=2)], ids=["causal", "window_groups"])
def test_cpu_path_against_the_float64_oracle(kw, interleaved):
    """bf16.  Appended keys: one rounding of the float64 rotation r, 2^-8 |r|, plus float32 evaluation, 2^-21 (|x| + |y|).  o and lse against
    the oracle on the float64-rotated q and the cache the call left.  The CPU path rounds k^ to the cache type (q^ stays float32): a logit is
    off by at most e = scale * groups * 2^-9, lse by e + 2e-5 (float32 arithmetic, as in the ALiBi file), o by (exp(2 e) - 1) max|v| + 2^-8 |ref| + 2e-5."""
    from oracle import cosine_sim_oracle as O
    q, kc, vc, cu, kn, vn, lens, _ = _problem(torch.bfloat16, D, H, HK, COUNTS, CACHED, CAP, 0, 7)
    cos, sin = tables(CAP, D, random=True)
    o, lse = rotary(q, kc, vc, cu, kn, vn, cache_seqlens=lens, return_lse=True, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved, **kw)
    (left, right), groups, cq = kw.get("window_size", (-1, -1)), kw.get("groups", 1), cu.tolist()
    npf, e = (lambda t: t.double().numpy()), 8.0 * groups * 2.0 ** -9
    for b, n in enumerate(COUNTS):
        if n == 0:
            continue
        L, rows = CACHED[b] + n, slice(cq[b], cq[b + 1])
        pos = np.arange(CACHED[b], L)
        r, mag = (t.transpose(1, 0, 2) for t in rotate(kn[rows], pos, cos, sin, interleaved))      # [Hk, n, D]
        assert (np.abs(npf(kc[b, :, CACHED[b]:L]) - r) <= 2.0 ** -8 * np.abs(r) + 2.0 ** -21 * mag).all(), b
        qb = rotate(q[rows], pos, cos, sin, interleaved)[0].transpose(1, 0, 2)[None]
        kb, vb = (np.repeat(npf(t[b, :, :L])[None], H // HK, axis=1) for t in (kc, vc))
        bias = np.repeat(_band(n, L, left, right, kw["causal"]), H, axis=0)
        ref = O.attention_forward_stats(qb, kb, vb, scale=8.0, groups=groups, causal=kw["causal"], l2norm_qk=True, attn_bias=bias, eps=1e-300)[0][0]
        got = npf(o[rows].permute(1, 0, 2))
        assert (np.abs(got - ref) <= 2.0 ** -8 * np.abs(ref) + np.expm1(2 * e) * np.abs(vb).max() + 2e-5).all(), (b, np.abs(got - ref).max())
        s = 8.0 * np.einsum("bhid,bhjd->bhij", O.l2norm(qb, groups), O.l2norm(kb, groups))[0] + bias
        ref_lse = np.log(np.exp(s - s.max(-1, keepdims=True)).sum(-1)) + s.max(-1)
        assert np.abs(npf(lse[rows]).T - ref_lse).max() <= e + 2e-5, b
