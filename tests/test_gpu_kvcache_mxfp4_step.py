"""The engine step against MXFP4 caches on the GPU (flash_cosine_sim_attention_mxfp4_step_with_kvcache, fcsa_forward_kvcache_mx_step: the STEP /
ROTARY forms of csrc/fcsa_decode_mx.hip and csrc/fcsa_prefill_mx.hip, and kv_append_mx_rotary_kernel).

One packed batch, N_b = (0, 1, 5, 64, 65, 130) on cache lengths (0, 17, 70, 200, 31, 129), H 4 / Hk 2, pages of 16 behind a shuffled table,
chunk_rows = 128: G * N_b = 128, 130, 260 take the chunk kernel (one, two and three 128-row tiles), the others the decode kernel.
Without tables the rows are the two existing MXFP4 calls' BIT FOR BIT (max_seqlen_k = 1: one key split everywhere).  With tables the appended
bytes are mxfp4_quantize of the float32 rotation rotary_reference.py states, and o / lse meet the existing 16-bit bars against the float64
oracle on the dequantised caches as the call left them, q rotated in the reference."""
import numpy as np
import pytest
import torch

import cases
import flash_cosine_sim_attention_amd as F
import lse_reference as R
import test_gpu_kvcache as TK
import test_gpu_kvcache_alibi as TA
import test_gpu_kvcache_ragged as TR
import tolerances as T
import tolerances_lse as TL
from rotary_reference import rotate, tables

pytestmark = pytest.mark.gpu

DT = TK.DT
_cu, _i32, _bits, _paged, _np = TR._cu, TR._i32, TR._bits, TR._paged, TK._np
COUNTS, CACHED, CAP, H, HK, CHUNK = [0, 1, 5, 64, 65, 130], [0, 17, 70, 200, 31, 129], 272, 4, 2, 128
CU = [0, 0, 1, 6, 70, 135, 265]
NAMES = ("k codes", "v codes", "k scales", "v scales")


def _make(dtype, D, seed):
    """packed q, the paged caches (k codes, v codes, k scales, v scales) and their table, packed k_new / v_new"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32)
    (kc, ks), (vc, vs) = F.mxfp4_quantize(rnd(len(COUNTS), HK, CAP, D)), F.mxfp4_quantize(rnd(len(COUNTS), HK, CAP, D))
    (kc, vc, table), (ks, vs, _) = _paged(kc, vc, 16, seed=seed), _paged(ks, vs, 16, seed=seed)
    return rnd(CU[-1], H, D).to(DT[dtype]), (kc, vc, ks, vs), table.cuda(), rnd(CU[-1], HK, D).to(DT[dtype]), rnd(CU[-1], HK, D).to(DT[dtype])


def _call(fn, q, mx, table, kn, vn, **kw):
    """fn on clones of the four cache tensors: (o, lse, the caches afterwards)"""
    mx = [t.clone() for t in mx]
    with torch.no_grad():
        o, lse = fn(q, *mx, _cu(COUNTS), kn, vn, _i32(CACHED), block_table=table, return_lse=True, **kw)
    torch.cuda.synchronize()
    return o, lse, mx


def _same(what, got, ref, rows=slice(None)):
    for name, x, y in zip(("o", "lse"), got[:2], ref[:2]):
        assert torch.equal(_bits(x[rows]), _bits(y[rows])), f"{what}: {name} differs in {int((_bits(x[rows]) != _bits(y[rows])).sum())} elements"
    for name, x, y in zip(NAMES, got[2], ref[2]):
        assert torch.equal(x, y), f"{what}: {name} differ"


ROUTED = [(dt, d, c, {}, False) for dt in ("bf16", "f16") for d in (64, 128) for c in (False, True)]
ROUTED += [("f16", 128, True, dict(groups=2, scale=4.0), False),
           ("bf16", 32, True, {}, True), ("f16", 128, True, dict(window_size=(40, -1)), True)]      # no chunk form: every sequence decodes


@pytest.mark.parametrize("dtype,D,causal,kw,all_decode", ROUTED, ids=lambda v: str(v).replace(" ", ""))
def test_routing_is_bitwise_the_two_calls(dtype, D, causal, kw, all_decode):
    q, mx, table, kn, vn = _make(dtype, D, seed=D + causal)
    kw = dict(kw, causal=causal, max_seqlen_k=1)
    step = lambda rows: _call(F.flash_cosine_sim_attention_mxfp4_step_with_kvcache, q, mx, table, kn, vn, chunk_rows=rows, **kw)
    dec = _call(F.flash_cosine_sim_attention_mxfp4_with_kvcache, q, mx, table, kn, vn, **kw)
    routed = step(CHUNK)
    assert torch.isfinite(routed[0]).all() and not torch.equal(routed[2][0], mx[0])      # (the append wrote)
    if all_decode:
        _same("all decode", routed, dec)
        _same("all decode, chunk_rows 0", step(0), dec)
        return
    pre = _call(F.flash_cosine_sim_attention_mxfp4_prefill_with_kvcache, q, mx, table, kn, vn, **kw)
    _same("decode-routed rows", routed, dec, slice(0, CU[3]))
    _same("chunk-routed rows", routed, pre, slice(CU[3], CU[6]))
    _same("chunk_rows 0", step(0), pre)
    _same("chunk_rows above every G * N_b", step(10 ** 6), dec)


def _exact_tables(rows, rotary_dim):
    """cos, sin in {0, +-1}: quarter turns, where the rotation is a signed permutation and every arithmetic order gives the same bits"""
    k = torch.randint(0, 4, (rows, rotary_dim // 2), generator=torch.Generator().manual_seed(rotary_dim))
    return torch.tensor([1.0, 0.0, -1.0, 0.0])[k], torch.tensor([0.0, 1.0, 0.0, -1.0])[k]


ROTARY = [("bf16", 128, 128, False, True), ("f16", 128, 128, True, True), ("f16", 64, 64, False, True), ("bf16", 64, 64, True, True),
          ("bf16", 128, 64, False, True), ("f16", 128, 64, True, True),
          ("f16", 128, 128, False, False), ("bf16", 64, 64, True, False), ("bf16", 128, 64, True, False)]      # not causal: the same positions


@pytest.mark.parametrize("angles", ["exact", "general"])
@pytest.mark.parametrize("dtype,D,rotary_dim,interleaved,causal", ROTARY)
def test_rotary_append_bytes_and_attention(dtype, D, rotary_dim, interleaved, causal, angles):
    """the appended code and scale bytes equal mxfp4_quantize of the float32-rotated k_new (v: of v_new), every other byte is untouched,
    and o / lse meet the 16-bit bars against the float64 oracle on the dequantised caches with q rotated in the reference -- query i at
    position L_b - N_b + i whether or not the call is causal"""
    q, mx, table, kn, vn = _make(dtype, D, seed=D + rotary_dim + interleaved)
    cos, sin = _exact_tables(CAP, rotary_dim) if angles == "exact" else tables(CAP, rotary_dim, random=True)
    kw = dict(causal=causal, chunk_rows=CHUNK, rotary_cos=cos.cuda(), rotary_sin=sin.cuda(), rotary_interleaved=interleaved)
    o, lse, after = _call(F.flash_cosine_sim_attention_mxfp4_step_with_kvcache, q, mx, table, kn, vn, **kw)
    slots = [s + i for n, s in zip(COUNTS, CACHED) for i in range(n)]
    kr = torch.from_numpy(rotate(kn, slots, cos, sin, interleaved, float32=True)[0]).float().cuda()
    want = (*F.mxfp4_quantize(kr), *F.mxfp4_quantize(vn))                    # k codes, k scales, v codes, v scales
    expect = [t.clone() for t in mx]
    for b, (n, s) in enumerate(zip(COUNTS, CACHED)):
        for i in range(n):
            blk, off = int(table[b, (s + i) // 16]), (s + i) % 16
            for dst, src in zip((expect[0], expect[2], expect[1], expect[3]), want):
                dst[blk, :, off] = src[CU[b] + i]
    for name, x, y in zip(NAMES, after, expect):
        assert torch.equal(x, y), f"{name}: {int((x != y).sum())} bytes differ"
    # attention: the caches as the call left them, dequantised (exact in the type); q rotated in float64 (raw) and float32 (operands)
    lens = [s + n for s, n in zip(CACHED, COUNTS)]
    kd, vd = F.mxfp4_dequantize(after[0], after[2], DT[dtype]), F.mxfp4_dequantize(after[1], after[3], DT[dtype])
    kseq, vseq = ([_np(x) for x in t] for t in TK._seqs(kd, vd, lens, table.cpu()))
    qp = [L - n + i for n, L in zip(COUNTS, lens) for i in range(n)]
    label, got = f"mxfp4_step/{dtype}/{D}/{rotary_dim}/{int(interleaved)}/{int(causal)}/{angles}", _np(lse)
    for tag, f32, cond, lbar in (("raw", False, cases.logit_cond(dtype, 8.0, 1, True), R.derived_lse_bound(dtype, 8.0, 1, True)),
                                 ("operands", True, 1.0, TL.LSE_TOL[dtype])):
        qr = torch.from_numpy(rotate(q, qp, cos, sin, interleaved, float32=f32)[0])
        ref_o, ref_l = TA._reference(qr, COUNTS, kseq, vseq, dict(causal=causal), torch.zeros(H), dtype if f32 else None, with_lse=True)
        TK._check(dtype, o, ref_o, f"{label}/{tag}", cond)
        seen = np.isfinite(ref_l)
        assert (np.isneginf(got) == ~seen).all(), label
        assert T.check(f"{label}/lse-{tag}", dtype, float(np.abs(got - ref_l)[seen].max()), lbar), tag


def test_opcheck_schema_and_fake_kernel():
    q, mx, table, kn, vn = _make("bf16", 64, seed=1)
    cos, sin = (t.cuda() for t in tables(CAP, 64))
    args = (q, *(t.contiguous() for t in mx), _cu(COUNTS), cos, sin, False, kn, vn, _i32(CACHED), table, 130, CAP, 8.0, True, True, 1, -1, -1, CHUNK, -1,
            False, False, True)
    torch.library.opcheck(torch.ops.fcsa_mx_step.kvcache_mxfp4_step_forward.default, args, test_utils=("test_schema", "test_faketensor"))


def test_captured_in_a_graph_with_device_tables():
    """captured once with device tables and rotary tables; every replay (the second after cache_seqlens changed ON THE DEVICE) equals the eager call"""
    q, mx, table, kn, vn = _make("bf16", 128, seed=5)
    cos, sin = (t.cuda() for t in tables(CAP, 128, random=True))
    cu, sl = _cu(COUNTS), _i32(CACHED)
    f = lambda mx_: F.flash_cosine_sim_attention_mxfp4_step_with_kvcache(q, *mx_, cu, kn, vn, sl, block_table=table, max_seqlen_q=130, max_seqlen_k=CAP,
                                                                          causal=True, return_lse=True, chunk_rows=CHUNK, rotary_cos=cos, rotary_sin=sin)
    captured, eager = list(mx), [t.clone() for t in mx]
    with torch.no_grad():
        f([t.clone() for t in mx])                                    # warm-up (allocator, the kernels' LDS attribute)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            o, lse = f(captured)
        for lens in (CACHED, [3, 0, 64, 100, 142, 16]):
            sl.copy_(torch.tensor(lens, dtype=torch.int32))
            g.replay()
            o_ref, lse_ref = f(eager)
            torch.cuda.synchronize()
            assert torch.equal(_bits(o), _bits(o_ref)) and torch.equal(_bits(lse), _bits(lse_ref)), lens
            assert all(torch.equal(a, b) for a, b in zip(captured, eager)), lens
