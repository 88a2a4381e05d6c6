"""The engine step against MXFP4 caches without a GPU (flash_cosine_sim_attention_mxfp4_step_with_kvcache): the public name, the op and its
fake kernel, the C symbol, the CPU-tensor path against the dequantise-and-compose route, and the refusals."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import flash_cosine_sim_attention_amd as F
from flash_cosine_sim_attention_amd import _lib, _torch_ops, cpu
from rotary_reference import rotate, tables

FN = F.flash_cosine_sim_attention_mxfp4_step_with_kvcache
COUNTS, CACHED, CAP, H, HK = [0, 1, 5, 40], [0, 17, 30, 9], 64, 4, 2
CU = torch.tensor([0, 0, 1, 6, 46], dtype=torch.int32)


def _make(D, dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    (kc, ks), (vc, vs) = F.mxfp4_quantize(rnd(len(COUNTS), HK, CAP, D)), F.mxfp4_quantize(rnd(len(COUNTS), HK, CAP, D))
    return rnd(46, H, D).to(dtype), [kc, vc, ks, vs], rnd(46, HK, D).to(dtype), rnd(46, HK, D).to(dtype)


def test_public_name_op_and_symbol():
    assert "flash_cosine_sim_attention_mxfp4_step_with_kvcache" in F.__all__
    assert {"fcsa_forward_kvcache_mx_step", "fcsa_forward_kvcache_mx_step_workspace_bytes"} <= set(_lib.EXPORTS)
    assert all(hasattr(_lib.load(), s) for s in ("fcsa_forward_kvcache_mx_step", "fcsa_forward_kvcache_mx_step_workspace_bytes"))
    _torch_ops.load()
    name = "fcsa_mx_step::kvcache_mxfp4_step_forward"
    assert torch._C._dispatch_has_kernel_for_dispatch_key(name, "CUDA")
    assert not any(torch._C._dispatch_has_kernel_for_dispatch_key(name, k) for k in ("Autograd", "CPU"))
    for want_lse in (False, True):      # the fake kernel: o like q, the lse empty unless asked for
        with FakeTensorMode():
            q, kc, ks = torch.empty(8, 4, 64, dtype=torch.bfloat16), torch.empty(2, 2, 32, 32, dtype=torch.uint8), torch.empty(2, 2, 32, 2, dtype=torch.uint8)
            o, lse = torch.ops.fcsa_mx_step.kvcache_mxfp4_step_forward(q, kc, kc, ks, ks, torch.empty(3, dtype=torch.int32), None, None, False, None, None,
                                                                       None, None, 8, 32, 8.0, True, True, 1, -1, -1, 128, -1, False, False, want_lse)
            assert o.shape == q.shape and o.dtype == q.dtype and lse.shape == ((8, 4) if want_lse else (0,)) and lse.dtype == torch.float32


@pytest.mark.parametrize("D,rotary_dim,interleaved", [(64, None, False), (64, 64, False), (128, 128, True), (128, 64, False), (32, None, False)])
def test_cpu_path_is_the_composed_route(D, rotary_dim, interleaved):
    """rotate k_new and q in float32 (tests/rotary_reference.py, an implementation of its own), quantise and append, dequantise, cpu.py:
    the bytes and results of the hand-composed route.  The reference rotation is fused -- fl(x cos +- fl(y sin)) -- and the CPU path's
    torch arithmetic rounds both products, so a rotated value can differ by one float32 ulp (2^-24 relative).  A code changes only where
    that ulp straddles an e2m1 rounding boundary, about 2^-20 of the elements at the grid's 2^-4 relative spacing: with 46 x 2 x D values,
    0.01 codes are expected to differ.  Condition: the V bytes and every scale byte are equal, and at most 2 K codes differ, each by one
    e2m1 step; o and lse are then compared on the path's own caches."""
    q, mx, kn, vn = _make(D, seed=D)
    rot = {} if rotary_dim is None else dict(zip(("rotary_cos", "rotary_sin"), tables(CAP, rotary_dim, random=True)), rotary_interleaved=interleaved)
    got = [t.clone() for t in mx]
    o, lse = FN(q, *got, CU, kn, vn, torch.tensor(CACHED, dtype=torch.int32), causal=True, return_lse=True, chunk_rows=16, **rot)
    qr, kr = q, kn      # (without tables nothing is rotated: q goes to cpu.py in its own type)
    if rot:
        slots = [s + i for n, s in zip(COUNTS, CACHED) for i in range(n)]      # (an append: the query's position is its key's slot)
        qr, kr = (torch.from_numpy(rotate(t, slots, rot["rotary_cos"], rot["rotary_sin"], interleaved, float32=True)[0]).float() for t in (q, kn))
    want = [t.clone() for t in mx]
    (kc, ks), (vc, vs) = F.mxfp4_quantize(kr), F.mxfp4_quantize(vn)
    for b, (n, s) in enumerate(zip(COUNTS, CACHED)):
        for i in range(n):
            for dst, src in zip(want, (kc, vc, ks, vs)):
                dst[b, :, s + i] = src[int(CU[b]) + i]
    assert all(torch.equal(got[i], want[i]) for i in (1, 2, 3))      # V codes, K scales, V scales
    nib = lambda t: torch.stack((t & 15, t >> 4), -1).long()
    step = (nib(got[0]) - nib(want[0])).abs()
    assert int((step > 0).sum()) <= (2 if rot else 0) and int(step.max()) <= 1, (int((step > 0).sum()), int(step.max()))
    dense = (F.mxfp4_dequantize(got[0], got[2], q.dtype), F.mxfp4_dequantize(got[1], got[3], q.dtype))
    o_ref, lse_ref = cpu.attention_forward_kvcache_varlen_cpu(qr, *dense, CU, None, None, [s + n for s, n in zip(CACHED, COUNTS)], causal=True,
                                                              return_lse=True)
    assert o.dtype == q.dtype
    if not rot:
        assert torch.equal(o, o_ref.to(q.dtype)) and torch.equal(lse, lse_ref)
    else:      # q differs from the reference's by an ulp of float32 at most: one rounding of the bf16 output, and the lse far inside 1e-5
        torch.testing.assert_close(o.float(), o_ref.float(), atol=2.0 ** -9, rtol=2.0 ** -7)
        torch.testing.assert_close(lse, lse_ref, atol=1e-5, rtol=0)


def test_refusals():
    q, mx, kn, vn = _make(64)
    sl = torch.tensor(CACHED, dtype=torch.int32)
    cos, sin = tables(CAP, 64)
    with pytest.raises(ValueError, match="flash_cosine_sim_attention_mxfp4_with_kvcache takes equal-N"):
        FN(q[None].transpose(1, 2), *mx, None, cache_seqlens=sl)
    for D in (32, 96):      # tables need dim_head 64 or 128
        q2, mx2, kn2, vn2 = _make(D)
        with pytest.raises(ValueError, match="64 and 128"):
            FN(q2, *mx2, CU, kn2, vn2, sl, rotary_cos=cos, rotary_sin=sin)
    with pytest.raises(TypeError, match="float16 or bfloat16"):
        FN(q.float(), *mx, CU, kn.float(), vn.float(), sl)
    with pytest.raises(TypeError, match="float16 or bfloat16"):
        FN(q.float(), *mx, CU, kn.float(), vn.float(), sl, rotary_cos=cos, rotary_sin=sin)
    with pytest.raises(ValueError, match="same shape"):
        FN(q, *mx, CU, kn, vn, sl, rotary_cos=cos, rotary_sin=sin[:-1])
    with pytest.raises(ValueError, match="given together"):
        FN(q, *mx, CU, kn, vn, sl, rotary_cos=cos)
    with pytest.raises(ValueError, match="beyond the 40 rows"):      # sequence 3 reaches position 48
        FN(q, *mx, CU, kn, vn, sl, rotary_cos=cos[:40], rotary_sin=sin[:40])
