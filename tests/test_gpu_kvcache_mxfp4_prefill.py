"""Prompt chunks against MXFP4 caches on the GPU (flash_cosine_sim_attention_mxfp4_prefill_with_kvcache, fcsa_forward_kvcache_mx_prefill: the
multi-wave kernel of csrc/fcsa_prefill_mx.hip).

The results are those of flash_cosine_sim_attention_mxfp4_with_kvcache BIT FOR BIT wherever that call runs one key split (o, lse, both code
caches, both scale tensors): the reference gets max_seqlen_k = 1, and every case asserts from the workspace query that this means one split.
Then the float64 oracle on the dequantised caches as the call left them (every cache value is exact in f16 / bf16: the 16-bit bars)."""
import ctypes as C

import pytest
import torch

import flash_cosine_sim_attention_amd as F
import test_gpu_kvcache as TK
import test_gpu_kvcache_ragged as TR

pytestmark = pytest.mark.gpu

DT = TK.DT
_cu, _i32, _bits, _paged = TR._cu, TR._i32, TR._bits, TR._paged

N_B = [1, 0, 5, 16, 37, 1, 130, 300]
CACHED = [0, 17, 300, 5, 0, 1023, 200, 650]


def _make(dtype, H, Hk, D, counts, cap, seed, append=True, qmul=1.0):
    """packed q, the caches (k codes, v codes, k scales, v scales) [B, Hk, cap, .] in the functions' order, packed k_new / v_new"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32)
    (kc, ks), (vc, vs) = F.mxfp4_quantize(rnd(len(counts), Hk, cap, D)), F.mxfp4_quantize(rnd(len(counts), Hk, cap, D))
    new = [rnd(sum(counts), Hk, D).to(DT[dtype]) if append else None for _ in range(2)]
    return (rnd(sum(counts), H, D) * qmul).to(DT[dtype]), (kc, vc, ks, vs), *new


def _assert_one_split(dtype, B, H, Hk, D, total_q, capacity, page, causal, append, l2norm, groups, scale):
    """with max_seqlen_k = 1 the MXFP4 call's workspace is that of ONE split (total_q * H rows of D + 2 floats, parts rounded to 256 bytes)"""
    from flash_cosine_sim_attention_amd import _lib
    prob = _lib.problem(DT[dtype], (B, H, Hk, total_q, 1, D), causal, False, l2norm, groups, scale)
    kv, mx = _lib.KvCache(), _lib.KvCacheMx()
    kv.capacity, kv.page_size, kv.num_blocks, kv.new_len = capacity, page, (B * (capacity // page) if page else 0), int(append)
    mx.format = _lib.FCSA_CACHE_MXFP4
    seqs = _lib.Varlen(None, None, total_q, 0)
    got = int(_lib.load().fcsa_forward_kvcache_mx_workspace_bytes(C.byref(prob), C.byref(kv), C.byref(mx), C.byref(seqs), None))
    rows, al = total_q * H, lambda n: (n + 255) // 256 * 256
    assert got == al(rows * D * 4) + al(rows * 8) < al(2 * rows * D * 4), (got, rows, D)


def _compare(dtype, q, mx, counts, kn, vn, cached, table=None, host=False, **kw):
    """both calls on clones of the four cache tensors: the bits of o, lse and all four afterwards.  Returns the new call's (o, lse, caches)."""
    (total, H, D), Hk, page = q.shape, mx[0].shape[1], mx[0].shape[2] if table is not None else 0
    capacity = table.shape[1] * page if table is not None else mx[0].shape[2]
    _assert_one_split(dtype, len(counts), H, Hk, D, total, capacity, page, kw.get("causal", False), kn is not None, kw.get("l2norm_qk", True),
                      kw.get("groups", 1), kw.get("scale", 8.0))
    dev = "cpu" if host else "cuda"
    cu, sl, tab = _cu(counts, dev), _i32(cached, dev), None if table is None else table.to(dev)
    ref, new = [t.clone() for t in mx], [t.clone() for t in mx]      # (a transposed view stays one: clone keeps the strides)
    with torch.no_grad():
        o_ref, lse_ref = F.flash_cosine_sim_attention_mxfp4_with_kvcache(q, *ref, cu, kn, vn, sl, block_table=tab, max_seqlen_k=1, return_lse=True, **kw)
        o, lse = F.flash_cosine_sim_attention_mxfp4_prefill_with_kvcache(q, *new, cu, kn, vn, sl, block_table=tab, return_lse=True, **kw)
    torch.cuda.synchronize()
    assert o.shape == q.shape and o.dtype == q.dtype and lse.shape == (total, H) and lse.dtype == torch.float32
    for name, x, y in (("o", o, o_ref), ("lse", lse, lse_ref), *zip(("k codes", "v codes", "k scales", "v scales"), new, ref)):
        assert torch.equal(_bits(x), _bits(y)), f"{name} differs in {int((_bits(x) != _bits(y)).sum())} elements"
    return o, lse, new


MIXED = [(dt, d, h, hk, c) for dt in ("bf16", "f16") for d in (64, 128) for h, hk in ((8, 8), (8, 2), (5, 1)) for c in (False, True)]


@pytest.mark.parametrize("dtype,D,H,Hk,causal", MIXED)
def test_bitwise_mixed_batch(dtype, D, H, Hk, causal):
    q, mx, kn, vn = _make(dtype, H, Hk, D, N_B, 1200, seed=D + 8 * H + Hk + causal)
    o, lse, new = _compare(dtype, q, mx, N_B, kn, vn, CACHED, causal=causal)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all() and not torch.equal(new[0], mx[0])      # (the append wrote)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [130, 159, 160, 161, 191, 192, 193, 257])
def test_bitwise_stage_and_block_edges(L, causal):
    """one sequence, a 130-row chunk (two tiles at G = 1) appended so that the total length lies around the 32-key blocks and 64-key stages"""
    for dtype, D in (("bf16", 128), ("f16", 64)):
        q, mx, kn, vn = _make(dtype, 2, 2, D, [130], 320, seed=L + D)
        _compare(dtype, q, mx, [130], kn, vn, [L - 130], causal=causal)


@pytest.mark.parametrize("layout", ["contiguous", "paged16", "paged16_transposed", "paged16_host"])
@pytest.mark.parametrize("dtype,D,causal", [("bf16", 128, True), ("f16", 64, False)])
def test_bitwise_layouts(layout, dtype, D, causal):
    """pages of 16, shuffled table: the pool [num_blocks, Hk, page, .] and the vLLM [num_blocks, page, Hk, .] one transposed; host tables"""
    q, mx, kn, vn = _make(dtype, 8, 2, D, N_B, 1216, seed=D + len(layout))
    table = None
    if layout != "contiguous":
        (kc, vc, table), (ks, vs, table2) = _paged(mx[0], mx[1], 16, seed=D), _paged(mx[2], mx[3], 16, seed=D)
        assert torch.equal(table, table2)
        mx = (kc, vc, ks, vs) if layout != "paged16" else tuple(t.contiguous() for t in (kc, vc, ks, vs))
    _compare(dtype, q, mx, N_B, kn, vn, CACHED, table=table, host=layout.endswith("host"), causal=causal)


# every path of mx_group_normalise at both head dims (four lanes, a lane pair, in the lane, inside a quarter), l2norm off, per-row shift
RAW = dict(l2norm_qk=False, scale=2.0 ** -9)
REGIMES = [("bf16", 128, {}), ("f16", 128, dict(groups=2, scale=4.0)), ("bf16", 128, dict(groups=4, scale=2.0)), ("f16", 128, dict(groups=16, scale=0.5)),
           ("f16", 64, {}), ("bf16", 64, dict(groups=2, scale=4.0)), ("f16", 64, dict(groups=4, scale=2.0)), ("bf16", 64, dict(groups=8, scale=1.0)),
           ("bf16", 128, RAW), ("f16", 64, RAW), ("f16", 128, dict(scale=16.0)), ("f16", 64, dict(groups=4, scale=4.0)), ("bf16", 64, dict(scale=120.0))]


@pytest.mark.parametrize("dtype,D,kw", REGIMES, ids=[f"{c[0]}_d{c[1]}_" + "_".join(f"{k}{v}" for k, v in c[2].items()) for c in REGIMES])
def test_bitwise_groups_and_regimes(dtype, D, kw):
    counts, cached = [3, 130, 40], [50, 70, 0]
    q, mx, kn, vn = _make(dtype, 4, 2, D, counts, 256, seed=D + len(kw), qmul=2.0 ** -8 if kw is RAW else 1.0)
    _compare(dtype, q, mx, counts, kn, vn, cached, causal=True, **kw)


def _oracle(dtype, q, mx, counts, kn, vn, cached, table, causal, label, **verify_kw):
    with torch.no_grad():
        o = F.flash_cosine_sim_attention_mxfp4_prefill_with_kvcache(q, *mx, _cu(counts), kn, vn, _i32(cached), block_table=table.cuda(), causal=causal)
    torch.cuda.synchronize()
    kd, vd = F.mxfp4_dequantize(mx[0], mx[2], DT[dtype]), F.mxfp4_dequantize(mx[1], mx[3], DT[dtype])
    ks, vs = TK._seqs(kd, vd, [s + n for s, n in zip(cached, counts)], table)
    TR._verify(dtype, o, q, counts, ks, vs, dict(causal=causal), label, **verify_kw)


ORACLE = [(dt, d, N_B, CACHED, 1216, c, True) for dt in ("bf16", "f16") for d in (64, 128) for c in (False, True)]
ORACLE.append(("bf16", 128, [1024], [0], 1024, True, False))      # one 1024-token chunk into an empty cache: the operand-faithful pass


@pytest.mark.parametrize("dtype,D,counts,cached,cap,causal,raw", ORACLE, ids=[f"{c[0]}_d{c[1]}_n{sum(c[2])}_{c[5]}" for c in ORACLE])
def test_oracle_on_the_dequantised_paged_cache(dtype, D, counts, cached, cap, causal, raw):
    q, mx, kn, vn = _make(dtype, 8, 2, D, counts, cap, seed=3 * D + causal)
    (kc, vc, table), (ks, vs, _) = _paged(mx[0], mx[1], 16, seed=D), _paged(mx[2], mx[3], 16, seed=D)
    _oracle(dtype, q, (kc, vc, ks, vs), counts, kn, vn, cached, table, causal, f"mxfp4_prefill_{dtype}_d{D}_{sum(counts)}_{causal}", raw=raw)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype,scale", [("bf16", 8.0), ("f16", 16.0), ("bf16", 120.0)])
def test_rows_without_a_visible_key(dtype, scale, causal):
    """sequence 0 has L = 0; under causal 32 of sequence 1's 40 tokens stand in front of its 8 keys: o = 0, lse = -inf, both regimes"""
    q, mx, _, _ = _make(dtype, 4, 2, 128, [5, 40], 64, seed=int(scale), append=False)
    o, lse, _ = _compare(dtype, q, mx, [5, 40], None, None, [0, 8], causal=causal, scale=scale)
    blind = 5 + 32 if causal else 5
    assert torch.isneginf(lse[:blind]).all() and (_bits(o[:blind]) == 0).all() and torch.isfinite(lse[blind:]).all() and torch.isfinite(o).all()


def test_captured_in_a_graph_with_device_tables():
    """captured once with device tables; every replay (the second after cache_seqlens changed ON THE DEVICE) equals the eager call bitwise"""
    counts = [1, 0, 37, 300]
    q, mx, kn, vn = _make("bf16", 8, 2, 128, counts, 1216, seed=9)
    (kc, vc, table), (ks, vs, _) = _paged(mx[0], mx[1], 16, seed=2), _paged(mx[2], mx[3], 16, seed=2)
    table, cu, sl = table.cuda(), _cu(counts), _i32([100, 7, 0, 650])
    f = lambda mx_: F.flash_cosine_sim_attention_mxfp4_prefill_with_kvcache(q, *mx_, cu, kn, vn, sl, block_table=table, max_seqlen_q=300,
                                                                             max_seqlen_k=1216, causal=True, return_lse=True)
    captured, eager = [kc, vc, ks, vs], [t.clone() for t in (kc, vc, ks, vs)]
    with torch.no_grad():
        f([t.clone() for t in captured])                              # warm-up (allocator, the kernel's LDS attribute)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            o, lse = f(captured)
        for lens in ([100, 7, 0, 650], [31, 64, 5, 916]):
            sl.copy_(torch.tensor(lens, dtype=torch.int32))
            g.replay()
            o_ref, lse_ref = f(eager)
            torch.cuda.synchronize()
            assert torch.equal(_bits(o), _bits(o_ref)) and torch.equal(_bits(lse), _bits(lse_ref)), lens
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(captured, eager)), lens
