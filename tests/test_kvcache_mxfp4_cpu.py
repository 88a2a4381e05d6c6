"""MXFP4 caches without a GPU: the plain-torch helpers (mxfp4_quantize / mxfp4_dequantize), the refusals of the Python front end, the
forward-only CPU path of flash_cosine_sim_attention_mxfp4_with_kvcache against the float64 oracle, and the op's schema."""
import pytest
import torch

import test_gpu_kvcache as TK


def _F():
    import flash_cosine_sim_attention_amd as F
    return F


def _blocks(seed=0):
    """blocks of 32 values of many sizes: below the smallest scale, around 1, and beyond the largest"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(4, 40, 64, generator=g) * torch.exp2(torch.randint(-20, 18, (4, 40, 2, 1), generator=g).float()).expand(-1, -1, -1, 32).flatten(-2)


def test_helpers_round_trip_and_half_a_grid_step():
    F, x = _F(), _blocks()
    x[0, 0, :32] = 0.0
    codes, scales = F.mxfp4_quantize(x)
    assert codes.shape == (4, 40, 32) and scales.shape == (4, 40, 2) and codes.dtype == scales.dtype == torch.uint8
    assert int(scales.min()) == 113 and int(scales.max()) == 139 and int(scales[0, 0, 0]) == 113
    d = F.mxfp4_dequantize(codes, scales)
    again = F.mxfp4_quantize(d)
    assert torch.equal(again[0] & 0x77, codes & 0x77) and torch.equal(again[1], scales)      # (a value rounded to zero keeps its sign bit only)
    assert torch.equal(F.mxfp4_dequantize(*again), d)
    for dt in (torch.float16, torch.bfloat16):      # every cache value is exact in both 16-bit types
        assert torch.equal(F.mxfp4_dequantize(codes, scales, dt).float(), d)
    # block by block: the rule saturates at 6 * 2^e, and inside the grid the error is at most half the step at the value -- 0.5 * 2^e below
    # 2 * 2^e, 2^e below 4 * 2^e, 2 * 2^e above
    unit = torch.exp2(scales.float() - 127).repeat_interleave(32, dim=-1)
    inside = torch.minimum(torch.maximum(x, -6 * unit), 6 * unit)
    step = torch.where(inside.abs() < 2 * unit, 0.5 * unit, torch.where(inside.abs() < 4 * unit, unit, 2 * unit))
    assert bool(((d - inside).abs() <= step / 2).all())
    # the scale byte is read clamped
    assert torch.equal(F.mxfp4_dequantize(codes, torch.full_like(scales, 0)), F.mxfp4_dequantize(codes, torch.full_like(scales, 113)))
    assert torch.equal(F.mxfp4_dequantize(codes, torch.full_like(scales, 255)), F.mxfp4_dequantize(codes, torch.full_like(scales, 139)))


def _call(B=2, H=4, Hk=2, N=2, D=64, cap=32, dt=torch.bfloat16, seed=1):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    return (rnd(B, H, N, D).to(dt), *_F().mxfp4_quantize(rnd(B, Hk, cap, D)), *_F().mxfp4_quantize(rnd(B, Hk, cap, D)))      # q, kc, ks, vc, vs


REFUSALS = {
    "d16": (lambda a: dict(q=a["q"][..., :16], k_cache=a["k_cache"][..., :8], v_cache=a["v_cache"][..., :8]), ValueError, "32, 64, 96 or 128"),
    "f32_q": (lambda a: dict(q=a["q"].float()), TypeError, "float16 or bfloat16"),
    "scale_shape": (lambda a: dict(k_block_scale=a["k_block_scale"][:, :, :-1]), ValueError, "k_block_scale must be"),
    "scale_dtype": (lambda a: dict(v_block_scale=a["v_block_scale"].float()), TypeError, "v_block_scale must be a torch.uint8"),
    "groups": (lambda a: dict(groups=16), ValueError, "multiple of 8 features"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals(case):
    q, kc, ks, vc, vs = _call()
    args = dict(q=q, k_cache=kc, v_cache=vc, k_block_scale=ks, v_block_scale=vs, cache_seqlens=8)
    change, exc, text = REFUSALS[case]
    args.update(change(args))
    with pytest.raises(exc, match=text):
        _F().flash_cosine_sim_attention_mxfp4_with_kvcache(**args)


@pytest.mark.parametrize("fn", ["flash_cosine_sim_attention_with_kvcache", "flash_cosine_sim_attention_varlen_with_kvcache",
                                "flash_cosine_sim_attention_step_with_kvcache", "flash_cosine_sim_attention_tree_with_kvcache"])
def test_the_other_cache_functions_refuse_uint8_caches(fn):
    q, kc, _, vc, _ = _call()
    packed = fn != "flash_cosine_sim_attention_with_kvcache"
    args = (q[0].transpose(0, 1), kc, vc, torch.tensor([0, 1, 2], dtype=torch.int32)) if packed else (q, kc, vc)
    with pytest.raises(TypeError, match="flash_cosine_sim_attention_mxfp4_with_kvcache"):
        getattr(_F(), fn)(*args)


@pytest.mark.parametrize("ragged", [False, True], ids=["equal_n", "ragged"])
@pytest.mark.parametrize("paged,groups", [(False, 1), (True, 1), (False, 4)], ids=["contiguous", "paged", "groups4"])
def test_cpu_path_equals_the_oracle(ragged, paged, groups):
    """the append lands in the caller's caches as bytes, and o (and the lse's shape) is the oracle's on the dequantised caches"""
    F, (B, H, Hk, N, D, cap, page) = _F(), (2, 4, 2, 2, 64, 32, 16)
    q, kc, ks, vc, vs = _call(B=4 if paged else B, cap=page if paged else cap)
    table = torch.tensor([[3, 1], [0, 2]], dtype=torch.int32) if paged else None
    g = torch.Generator().manual_seed(2)
    kn, vn = torch.randn(B, Hk, N, D, generator=g).bfloat16(), torch.randn(B, Hk, N, D, generator=g).bfloat16()
    seq, q = [5, 30], q[:B]
    kw = dict(cache_seqlens=torch.tensor(seq, dtype=torch.int32), block_table=table, causal=True, return_lse=True, groups=groups, scale=8.0 / groups)
    if ragged:
        pack = lambda t: t.transpose(1, 2).flatten(0, 1)
        o, lse = F.flash_cosine_sim_attention_mxfp4_with_kvcache(pack(q), kc, vc, ks, vs, cu_seqlens_q=torch.tensor([0, N, 2 * N], dtype=torch.int32),
                                                                 k_new=pack(kn), v_new=pack(vn), **kw)
        o, lse = o.unflatten(0, (B, N)).transpose(1, 2), lse.unflatten(0, (B, N)).transpose(1, 2)
    else:
        o, lse = F.flash_cosine_sim_attention_mxfp4_with_kvcache(q, kc, vc, ks, vs, k_new=kn, v_new=vn, **kw)
    assert lse.shape == (B, H, N) and bool(torch.isfinite(lse).all())
    kseq, vseq = TK._seqs(F.mxfp4_dequantize(kc, ks), F.mxfp4_dequantize(vc, vs), [s + N for s in seq], table)
    for b in range(B):      # the appended slots hold what mxfp4_quantize gives
        want = F.mxfp4_dequantize(*F.mxfp4_quantize(kn[b]))
        assert torch.equal(kseq[b][:, seq[b]:], want)
    TK._verify("bf16", o, q, kseq, vseq, dict(causal=True, groups=groups, scale=8.0 / groups), f"mxfp4/cpu_{ragged}_{paged}_{groups}")


def test_op_schema():
    from flash_cosine_sim_attention_amd import _torch_ops
    _torch_ops.load()
    assert str(torch.ops.fcsa_mx.kvcache_mxfp4_forward.default._schema) == (
        "fcsa_mx::kvcache_mxfp4_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor(c!) k_block_scale, Tensor(d!) v_block_scale, "
        "Tensor? cu_seqlens_q, Tensor? k_new, Tensor? v_new, Tensor? cache_seqlens, Tensor? block_table, int max_seqlen_q, int max_seqlen_k, "
        "float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right, bool return_lse) -> (Tensor, Tensor)")
