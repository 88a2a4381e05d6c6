"""Prompt chunks against the key/value cache on the GPU (flash_cosine_sim_attention_prefill_with_kvcache, fcsa_forward_kvcache_prefill: the
multi-wave kernel of csrc/fcsa_prefill.hip).

The contract: the results are those of flash_cosine_sim_attention_varlen_with_kvcache, BIT FOR BIT wherever that call runs one key split
-- o, lse and the caches after the append.  The reference of the bitwise tests is that call with max_seqlen_k = 1 (the bound only sizes
the launch; at max_k = 1 fcsa::decode_splits gives 1 for any grid), and every case asserts that precondition from the ragged workspace
query instead of assuming it.  A float64 oracle that shares nothing with the decode kernels (the policy and bars of
test_gpu_kvcache_ragged._verify), the visibility probe, a bounds check on caller-owned strided buffers through the C ABI, HIP-graph
capture with device tables and the empty sizes follow."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import test_gpu_kvcache as TK
import test_gpu_kvcache_ragged as TR
import visibility_probe as VP
from test_gpu_buffer_bounds import Arena, FILL

pytestmark = pytest.mark.gpu

DT = TK.DT
_cu, _i32, _bits, _paged = TR._cu, TR._i32, TR._bits, TR._paged

# the mixed batch: a first token into an empty cache, an empty sequence, a few tokens, 16 and 37 tokens (less than a 128-row tile at every
# G), a plain decode deep in the cache, a chunk of more than one tile at G = 1 and one of several tiles at every G
N_B = [1, 0, 5, 16, 37, 1, 130, 300]
CACHED = [0, 17, 300, 5, 0, 1023, 200, 650]
CAPACITY = 1200


def _F():
    import flash_cosine_sim_attention_amd as F
    return F


def _prefill(*a, **kw):
    return _F().flash_cosine_sim_attention_prefill_with_kvcache(*a, **kw)


def _ragged(*a, **kw):
    return _F().flash_cosine_sim_attention_varlen_with_kvcache(*a, **kw)


def _align(n):
    return (n + 255) // 256 * 256


def _assert_one_split(dtype, B, H, Hk, D, total_q, capacity, page, causal, append, l2norm=True, groups=1, scale=8.0):
    """The precondition of the bitwise comparison: for this problem with max_seqlen_k = 1 the ragged call's workspace is that of ONE split
    -- the f32 partials of total_q * H rows, D + 2 floats each (each of the two parts rounded up to the library's 256-byte alignment) --
    and two splits would need more."""
    from flash_cosine_sim_attention_amd import _lib
    lib = _lib.load()
    prob = _lib.problem(DT[dtype], (B, H, Hk, total_q, 1, D), causal, False, l2norm, groups, scale)
    kv = _lib.KvCache()
    kv.capacity, kv.page_size, kv.num_blocks, kv.new_len = capacity, page, (B * (capacity // page) if page else 0), int(append)
    seqs = _lib.Varlen(None, None, total_q, 0)
    got = int(lib.fcsa_forward_kvcache_varlen_workspace_bytes(C.byref(prob), C.byref(kv), C.byref(seqs), None, None))
    rows = total_q * H
    assert got == _align(rows * D * 4) + _align(rows * 8) < _align(2 * rows * D * 4), (got, rows, D)
    assert rows % 32 != 0 or got == rows * (D + 2) * 4


def _compare(dtype, q, kc, vc, counts, kn, vn, cached, table=None, host_tables=False, page=0, check_lse_false=False, **kw):
    """both calls on clones of the caches: the bits of o, lse and both caches afterwards.  Returns the prefill call's (o, lse, kc, vc)."""
    total, H, D = q.shape
    Hk = kc.shape[1]
    capacity = table.shape[1] * kc.shape[2] if table is not None else kc.shape[2]
    _assert_one_split(dtype, len(counts), H, Hk, D, total, capacity, kc.shape[2] if table is not None else 0, kw.get("causal", False),
                      kn is not None, kw.get("l2norm_qk", True), kw.get("groups", 1), kw.get("scale", 8.0))
    dev = "cpu" if host_tables else "cuda"
    cu, sl = _cu(counts, dev), _i32(cached, dev)
    tab = None if table is None else table.to(dev)
    k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()      # (a transposed view stays one: clone keeps the strides)
    assert k1.stride() == kc.stride()
    with torch.no_grad():
        o_ref, lse_ref = _ragged(q, k1, v1, cu, kn, vn, sl, block_table=tab, max_seqlen_k=1, return_lse=True, **kw)
        o, lse = _prefill(q, k2, v2, cu, kn, vn, sl, block_table=tab, return_lse=True, **kw)
        if check_lse_false:
            k3, v3 = kc.clone(), vc.clone()
            o3 = _prefill(q, k3, v3, cu, kn, vn, sl, block_table=tab, **kw)
    torch.cuda.synchronize()
    assert o.shape == q.shape and o.dtype == q.dtype and lse.shape == (total, H) and lse.dtype == torch.float32
    # NaN-filled guard slots compare as bits, like everything else
    assert torch.equal(_bits(o), _bits(o_ref)), f"o differs in {int((_bits(o) != _bits(o_ref)).sum())} elements"
    assert torch.equal(_bits(lse), _bits(lse_ref)), f"lse differs in {int((_bits(lse) != _bits(lse_ref)).sum())} elements"
    assert torch.equal(_bits(k2), _bits(k1)) and torch.equal(_bits(v2), _bits(v1)), "the caches differ after the append"
    if check_lse_false:
        assert torch.equal(_bits(o3), _bits(o)) and torch.equal(_bits(k3), _bits(k2)) and torch.equal(_bits(v3), _bits(v2))
    return o, lse, k2, v2


# ---- 4. bit for bit against the ragged call forced to one split ---------------------------------------------------------------------------

HEADS = [(8, 8), (8, 2), (8, 1), (6, 2), (5, 1)]
MIXED = [(f"{dt}_d{d}_h{h}_hk{hk}_{'causal' if c else 'full'}", dt, d, h, hk, c)
         for dt in ("bf16", "f16") for d in (64, 128) for h, hk in HEADS for c in (False, True)]


@pytest.mark.parametrize("name,dtype,D,H,Hk,causal", MIXED, ids=[c[0] for c in MIXED])
def test_bitwise_mixed_batch(name, dtype, D, H, Hk, causal):
    q, kc, vc, kn, vn = TR._inputs(dtype, H, Hk, D, N_B, CAPACITY, seed=sum(map(ord, name)))
    o, lse, k2, v2 = _compare(dtype, q, kc, vc, N_B, kn, vn, CACHED, causal=causal)
    assert torch.equal(_bits(k2), _bits(TR._appended(kc, kn, N_B, CACHED))) and torch.equal(_bits(v2), _bits(TR._appended(vc, vn, N_B, CACHED)))
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()


@pytest.mark.parametrize("dtype,D,H,Hk", [("bf16", 128, 8, 2), ("f16", 64, 6, 2)])
@pytest.mark.parametrize("causal", [False, True])
def test_bitwise_mixed_batch_without_append(dtype, D, H, Hk, causal):
    """L_b = cache_seqlens[b]: under causal the 300-token chunk against 650 positions and the 130-token one against 200; sequence 0 and 4
    (nothing cached) have no visible key at all"""
    q, kc, vc, _, _ = TR._inputs(dtype, H, Hk, D, N_B, CAPACITY, seed=D + H, append=False)
    o, lse, _, _ = _compare(dtype, q, kc, vc, N_B, None, None, CACHED, causal=causal, check_lse_false=True)
    cu = _cu(N_B, "cpu").tolist()
    for b in (0, 4):
        assert (o[cu[b]:cu[b + 1]] == 0).all() and torch.isneginf(lse[cu[b]:cu[b + 1]]).all()


EDGE_L = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193]


@pytest.fixture(scope="module")
def edge_inputs():
    """one sequence, H 8 / Hk 2 (G = 4: 130 tokens are 520 rows, five tiles), D 128 and D 64, capacity 256; shared and left unchanged"""
    out = {}
    for dtype, D in (("bf16", 128), ("f16", 64)):
        g = torch.Generator(device="cuda").manual_seed(D)
        rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32).to(DT[dtype])
        out[dtype] = (rnd(130, 8, D), rnd(1, 2, 256, D), rnd(1, 2, 256, D))
    return out


@pytest.mark.parametrize("L", EDGE_L)
def test_bitwise_stage_and_block_edges(edge_inputs, L):
    """sequence lengths around the 32-key blocks and the 64-key stages, a single token and a chunk of min(L, 130), causal and not"""
    for dtype, (q, kc, vc) in edge_inputs.items():
        for N in (1, min(L, 130)):
            for causal in (False, True):
                o, lse, _, _ = _compare(dtype, q[:N].contiguous(), kc, vc, [N], None, None, [L], causal=causal)
                assert torch.isfinite(lse).all(), (dtype, L, N, causal)


@pytest.mark.parametrize("dtype,scale", [("bf16", 8.0), ("f16", 16.0), ("bf16", 120.0)])
def test_rows_without_a_visible_key(edge_inputs, dtype, scale):
    """N = 40 against L = 8 under causal: tokens 0 .. 31 see nothing -- lse = -inf and o = 0 exactly, in both exponent regimes -- and
    return_lse=False gives the same o bits"""
    q, kc, vc = edge_inputs["bf16" if dtype == "bf16" else "f16"]
    o, lse, _, _ = _compare(dtype, q[:40].contiguous(), kc, vc, [40], None, None, [8], causal=True, scale=scale, check_lse_false=True)
    assert torch.isneginf(lse[:32]).all() and (_bits(o[:32]) == 0).all()
    assert torch.isfinite(lse[32:]).all() and torch.isfinite(o).all() and (o[32:].float().abs().sum(-1) > 0).all()


LAYOUTS = [("paged16_device", 16, False), ("paged64_device", 64, False), ("paged16_host", 16, True), ("contiguous_transposed_device", 0, False),
           ("contiguous_transposed_host", 0, True)]


@pytest.mark.parametrize("name,page,host", LAYOUTS, ids=[c[0] for c in LAYOUTS])
@pytest.mark.parametrize("dtype,D,causal", [("bf16", 128, True), ("f16", 64, False)])
def test_bitwise_layouts(name, page, host, dtype, D, causal):
    """The vLLM layouts passed transposed -- pages of 16 and 64 through a shuffled table over a pool whose spare blocks are NaN, and a
    contiguous [B, capacity, Hk, D] buffer -- with NaN in every slot at or beyond L_b, device and host tables."""
    H, Hk, cap = 8, 2, 1216                       # a whole number of 64-position pages
    q, kc, vc, kn, vn = TR._inputs(dtype, H, Hk, D, N_B, cap, seed=page + D)
    for b, (s, n) in enumerate(zip(CACHED, N_B)):
        kc[b, :, s + n:] = float("nan")
        vc[b, :, s + n:] = float("nan")
    table = None
    if page:
        kc, vc, table = _paged(kc, vc, page, seed=page)
    else:
        kc, vc = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (kc, vc))
        assert kc.stride(1) == D and kc.stride(2) == Hk * D
    o, lse, _, _ = _compare(dtype, q, kc, vc, N_B, kn, vn, CACHED, table=table, host_tables=host, causal=causal)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all(), "a NaN behind a sequence's length reached the output"


REGIMES = [("f16_scale16_per_row", "f16", dict(scale=16.0)), ("bf16_scale120_per_row", "bf16", dict(scale=120.0)),
           ("f16_scale4_static", "f16", dict(scale=4.0)), ("bf16_groups2", "bf16", dict(groups=2, scale=4.0)),
           ("f16_groups4", "f16", dict(groups=4, scale=2.0)), ("bf16_groups16", "bf16", dict(groups=16, scale=1.0)),
           ("f16_groups16_per_row", "f16", dict(groups=16, scale=1.0)), ("bf16_no_l2norm", "bf16", dict(l2norm_qk=False, scale=1.0)),
           ("f16_no_l2norm", "f16", dict(l2norm_qk=False, scale=1.0))]


@pytest.mark.parametrize("name,dtype,kw", REGIMES, ids=[c[0] for c in REGIMES])
@pytest.mark.parametrize("D", [64, 128])
def test_bitwise_regimes(name, dtype, kw, D):
    """both exponent regimes, the l2norm group widths inside a lane's fragment (16 groups), of one fragment and of several, l2norm off"""
    q, kc, vc, kn, vn = TR._inputs(dtype, 8, 2, D, N_B, CAPACITY, seed=sum(map(ord, name)) + D)
    q, kc = TK._unit_normalised(q, kc, kw.get("groups", 1), kw.get("l2norm_qk", True))
    _, kn = TK._unit_normalised(q, kn, 1, kw.get("l2norm_qk", True))
    o, lse, _, _ = _compare(dtype, q, kc, vc, N_B, kn, vn, CACHED, causal=True, **kw)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()


# ---- 5. the float64 oracle ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_oracle_mixed_batch(dtype, D, causal):
    H, Hk = 8, 2
    q, kc, vc, kn, vn = TR._inputs(dtype, H, Hk, D, N_B, CAPACITY, seed=3 * D + causal)
    kc, vc, table = _paged(kc, vc, 16, seed=D)
    with torch.no_grad():
        o = _prefill(q, kc, vc, _cu(N_B), kn, vn, _i32(CACHED), block_table=table.cuda(), causal=causal)
    torch.cuda.synchronize()
    ks, vs = TK._seqs(kc, vc, [s + n for s, n in zip(CACHED, N_B)], table)
    TR._verify(dtype, o, q, N_B, ks, vs, dict(causal=causal), f"prefill_{dtype}_d{D}_{'causal' if causal else 'full'}")


def test_oracle_1024_token_chunk_into_an_empty_paged_cache():
    """one causal chunk of 1024 tokens appended into an empty paged-16 cache, H 8 / Hk 2, D 128, bf16: 32 row tiles whose key ranges grow
    from 32 to 1024 keys.  The operand-faithful pass, as in test_ragged_many_splits_long_cache."""
    H, Hk, D, N = 8, 2, 128, 1024
    q, kc, vc, kn, vn = TR._inputs("bf16", H, Hk, D, [N], N, seed=77)
    kc, vc, table = _paged(kc, vc, 16, seed=5)
    with torch.no_grad():
        o = _prefill(q, kc, vc, _cu([N]), kn, vn, _i32([0]), block_table=table.cuda(), causal=True)
    torch.cuda.synchronize()
    ks, vs = TK._seqs(kc, vc, [N], table)
    assert torch.equal(_bits(ks[0]), _bits(kn.permute(1, 0, 2))) and torch.equal(_bits(vs[0]), _bits(vn.permute(1, 0, 2)))
    TR._verify("bf16", o, q, [N], ks, vs, dict(causal=True), "prefill_chunk_1024", raw=False)


# ---- 6. the visibility probe ------------------------------------------------------------------------------------------------------------------

PROBE = [c for c in VP.decode_cases() if c[10] is not None and not c[12] and c[1] in ("bf16", "f16") and c[2] in (64, 128) and c[14] == (-1, -1)]
for _i, (_page, _causal, _append) in enumerate([(p, c, a) for p in (16, 0) for c in (True, False) for a in (True, False)]):
    _dtype, _D = (("bf16", 64), ("f16", 128))[(_i // 2 + _i) % 2]      # each pair with append and without, causal and not
    PROBE.append((f"chunk_{_dtype}_d{_D}_p{_page}_{'append' if _append else 'read'}_{'causal' if _causal else 'full'}", _dtype, _D, 8, 2, 0, 288, _page,
                  [0, 31, 33, 100, 1, 70], 0, [1, 0, 5, 17, 3, 200], _causal, False, dict(append=_append), (-1, -1)))


def test_the_probe_table_has_the_ragged_cases_the_kernel_takes():
    assert len(PROBE) == 8 + 2 and {c[0] for c in PROBE} >= {"ragged_bf16_d64_p0_append_causal", "ragged_f16_d128_p32_append_full"}


@pytest.mark.parametrize("name,dtype,D,H,Hk,N,cap,page,lens,n_new,counts,causal,fp8,kw,window", PROBE, ids=[c[0] for c in PROBE])
def test_probe_prefill(monkeypatch, name, dtype, D, H, Hk, N, cap, page, lens, n_new, counts, causal, fp8, kw, window):
    """visibility_probe.run_decode with the ragged call's name bound to the new function (the signatures match): a single hidden or leaked
    key moves a count the probe's bars decide"""
    ns = types.SimpleNamespace(flash_cosine_sim_attention_varlen_with_kvcache=_F().flash_cosine_sim_attention_prefill_with_kvcache)
    monkeypatch.setattr(VP, "_F", lambda: ns)
    scale, l2 = VP.probe_scale(kw)
    fails = VP.judge(dtype, name, VP.run_decode(dtype, D, H, Hk, N, cap, page, lens, n_new, counts, causal, fp8, scale, l2, "cuda", window,
                                                kw.get("append", True), seed=len(name)))
    assert not fails, (name, fails)


# ---- 7. caller-owned strided buffers through the C ABI ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D,H,Hk,page", [("bf16", 128, 8, 2, 16), ("f16", 64, 5, 1, 0)])
def test_prefill_call_stays_inside_its_buffers(dtype, D, H, Hk, page):
    """q, k_new, v_new, the caches and the tables inside one arena pre-filled with 0xFF bytes, guard bands between them; o and lse are
    STRIDED views of larger buffers (rows D + 8 elements apart, spare rows before and after; lse with spare columns): no guard byte
    changes, every element the call does not own keeps its fill, the inputs keep their bits, every owned element is written, and the
    result is the Python call's."""
    from flash_cosine_sim_attention_amd import _lib
    lib = _lib.load()
    dt = DT[dtype]
    es = 2
    counts, cached, cap = [1, 0, 37, 130], [5, 40, 0, 100], 256
    B, total = len(counts), sum(counts)
    mb = cap // page if page else 0
    nb = B * mb + 2
    cache_elems = (nb * page if page else B * cap) * Hk * D
    ar = Arena((total + 5) * H * (D + 8) * es + (total + 5) * (H + 3) * 4 + (total * H * D + 2 * total * Hk * D + 2 * cache_elems) * es
               + 4 * (2 * B + 1 + B * max(mb, 1)) + 30 * (4096 + 256))
    g = torch.Generator(device="cuda").manual_seed(D)

    def rnd(shape):
        t = ar.take(shape, dt)
        t.copy_(torch.randn(shape, device="cuda", dtype=torch.float32, generator=g).to(dt))
        return t

    q, kn, vn = rnd((total, H, D)), rnd((total, Hk, D)), rnd((total, Hk, D))
    kc, vc = (rnd((nb, Hk, page, D)), rnd((nb, Hk, page, D))) if page else (rnd((B, Hk, cap, D)), rnd((B, Hk, cap, D)))
    cu, sl = ar.take((B + 1,), torch.int32), ar.take((B,), torch.int32)
    cu.copy_(_cu(counts)), sl.copy_(_i32(cached))
    table = None
    if page:
        table = ar.take((B, mb), torch.int32)
        table.copy_(torch.randperm(nb, generator=torch.Generator().manual_seed(1))[:B * mb].reshape(B, mb).to(torch.int32))
    o_full, lse_full = ar.take((total + 5, H, D + 8), dt), ar.take((total + 5, H + 3), torch.float32)
    o, lse = o_full[2:2 + total, :, :D], lse_full[3:3 + total, 1:1 + H]
    inputs = [q, kn, vn, cu, sl] + ([table] if page else [])
    before = [t.clone() for t in inputs]
    k_ref, v_ref = kc.clone(), vc.clone()

    prob = _lib.problem(dt, (B, H, Hk, max(counts), cap, D), True, False, True, 1, 8.0)
    kv = _lib.KvCache()
    kv.capacity, kv.page_size, kv.num_blocks, kv.new_len = cap, page, nb if page else 0, 1
    packed = lambda t: _lib.Tensor(t.data_ptr(), 0, t.stride(1), t.stride(0))
    kv.k_cache, kv.v_cache = _lib.tensor4(kc), _lib.tensor4(vc)
    kv.k_new, kv.v_new = packed(kn), packed(vn)
    kv.cache_seqlens = sl.data_ptr()
    if page:
        kv.block_table, kv.block_table_stride = table.data_ptr(), mb
    seqs = _lib.Varlen(cu.data_ptr(), None, total, 0)
    none = _lib.Tensor(None, 0, 0, 0)
    fa = _lib.ForwardArgs(prob, packed(q), none, none, packed(o), None, None, None, _lib.NormState(None, None, None, None), None, 0,
                          torch.cuda.current_stream().cuda_stream)
    lo = _lib.LseOut(lse.data_ptr(), 0, lse.stride(1), lse.stride(0))
    _lib.check(lib.fcsa_forward_kvcache_prefill(C.byref(fa), C.byref(kv), C.byref(seqs), C.byref(lo)), "fcsa_forward_kvcache_prefill")
    torch.cuda.synchronize()
    assert ar.guards_intact(), "a byte outside the call's buffers was written"
    for t, b in zip(inputs, before):
        assert torch.equal(t, b), "an input changed"
    # what the call owns is written (no 0xFF pattern: NaN in both types), what it does not own keeps the fill
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    own = torch.zeros_like(o_full, dtype=torch.bool)
    own[2:2 + total, :, :D] = True
    assert (o_full.view(torch.int16)[~own] == -1).all(), "an element of the o buffer outside the view was written"
    own = torch.zeros_like(lse_full, dtype=torch.bool)
    own[3:3 + total, 1:1 + H] = True
    assert (lse_full.view(torch.int32)[~own] == -1).all(), "an element of the lse buffer outside the view was written"
    with torch.no_grad():
        o_py, lse_py = _prefill(q, k_ref, v_ref, cu, kn, vn, sl, block_table=table, causal=True, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(o), _bits(o_py)) and torch.equal(_bits(lse), _bits(lse_py))
    assert torch.equal(_bits(kc), _bits(k_ref)) and torch.equal(_bits(vc), _bits(v_ref))
    assert FILL == 0xFF


# ---- 8. HIP-graph capture ---------------------------------------------------------------------------------------------------------------------

def test_prefill_captured_in_a_graph_with_device_tables():
    """device cu_seqlens_q, cache_seqlens and block_table with both bounds given: the call does not synchronise, so it is captured once and
    replayed; after cache_seqlens changes ON THE DEVICE the replay follows it.  Each replay equals the eager call on the same tables and
    the same cache contents, bit for bit (o, lse, caches)."""
    dtype, H, Hk, D, cap = "bf16", 8, 2, 128, 1216
    counts = [1, 0, 37, 300]
    q, kc, vc, kn, vn = TR._inputs(dtype, H, Hk, D, counts, cap, seed=9)
    kc, vc, table = _paged(kc, vc, 16, seed=2)
    table, cu = table.cuda(), _cu(counts)
    sl = _i32([100, 7, 0, 650])
    f = lambda k_, v_: _prefill(q, k_, v_, cu, kn, vn, sl, block_table=table, max_seqlen_q=300, max_seqlen_k=cap, causal=True, return_lse=True)
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            f(kc.clone(), vc.clone())                                # warm-up (allocator, the kernel's LDS attribute)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        k_eager, v_eager = kc.clone(), vc.clone()
        with torch.cuda.graph(g):
            o, lse = f(kc, vc)
        for step, lens in enumerate(([100, 7, 0, 650], [31, 64, 5, 916], [0, 0, 1179, 0])):
            sl.copy_(torch.tensor(lens, dtype=torch.int32))
            g.replay()
            o_ref, lse_ref = f(k_eager, v_eager)
            torch.cuda.synchronize()
            assert torch.equal(_bits(o), _bits(o_ref)) and torch.equal(_bits(lse), _bits(lse_ref)), step
            assert torch.equal(_bits(kc), _bits(k_eager)) and torch.equal(_bits(vc), _bits(v_eager)), step


# ---- 9. zero sizes ----------------------------------------------------------------------------------------------------------------------------

def test_zero_sizes():
    H, Hk, D, cap = 8, 2, 64, 64
    g = torch.Generator(device="cuda").manual_seed(0)
    kc = torch.randn(3, Hk, cap, D, device="cuda", generator=g).to(torch.bfloat16)
    vc = torch.randn(3, Hk, cap, D, device="cuda", generator=g).to(torch.bfloat16)
    k0, v0 = kc.clone(), vc.clone()
    q = torch.empty(0, H, D, device="cuda", dtype=torch.bfloat16)
    kn = torch.empty(0, Hk, D, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        # every N_b = 0 (so total_q = 0): three sequences, with (empty) rows to append and without; then no sequence at all (B = 0)
        o, lse = _prefill(q, kc, vc, _cu([0, 0, 0]), kn, kn.clone(), _i32([0, 5, 64]), causal=True, return_lse=True)
        assert o.shape == (0, H, D) and o.dtype == torch.bfloat16 and lse.shape == (0, H) and lse.dtype == torch.float32
        o = _prefill(q, kc, vc, _cu([0, 0, 0]), cache_seqlens=_i32([0, 5, 64]))
        assert o.shape == (0, H, D)
        o, lse = _prefill(q, kc[:0], vc[:0], _cu([]), kn, kn.clone(), _i32([]), return_lse=True)
        assert o.shape == (0, H, D) and lse.shape == (0, H)
        # sequences without rows beside one that has some
        q5 = torch.randn(5, H, D, device="cuda", generator=g).to(torch.bfloat16)
        o, lse, _, _ = _compare("bf16", q5, kc, vc, [0, 5, 0], None, None, [3, 5, 64])
        assert torch.isfinite(o).all()
    torch.cuda.synchronize()
    assert torch.equal(_bits(kc), _bits(k0)) and torch.equal(_bits(vc), _bits(v0))
