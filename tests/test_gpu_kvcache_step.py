"""The engine step against the key/value cache on the GPU (flash_cosine_sim_attention_step_with_kvcache, fcsa_forward_kvcache_step): every
sequence of a packed batch on the kernel built for its row count -- the ragged decode kernel below chunk_rows, the multi-wave chunk kernel
from it on -- with one append.

The contract: o, lse and both caches are those of flash_cosine_sim_attention_varlen_with_kvcache; a chunk-routed sequence's rows are bit
for bit that call's rows at ONE key split, a decode-routed sequence's rows bit for bit that call's rows at the same split count.  So with
max_seqlen_k = 1 (one split everywhere; the precondition is asserted from the ragged workspace query, as in
test_gpu_kvcache_prefill._assert_one_split) the whole result is bit-identical for every chunk_rows.  The bitwise tests run that
comparison over thresholds, fp8 caches, windows, regimes and layouts; the kernels actually launched are read back from the profile hook;
real split counts are judged against the float64 oracle under the bars of test_gpu_kvcache_ragged._verify; the visibility probe, caller-owned
strided buffers through the C ABI, HIP-graph capture with changing routes and the empty sizes follow."""
import ctypes as C
import types

import pytest
import torch

import test_gpu_kvcache as TK
import test_gpu_kvcache_fp8 as T8
import test_gpu_kvcache_lse as TL
import test_gpu_kvcache_prefill as TP
import test_gpu_kvcache_ragged as TR
import visibility_probe as VP
from test_gpu_buffer_bounds import Arena, FILL

pytestmark = pytest.mark.gpu

DT = TK.DT
_cu, _i32, _bits, _paged = TR._cu, TR._i32, TR._bits, TR._paged
N_B, CACHED, CAPACITY = TP.N_B, TP.CACHED, TP.CAPACITY
E4M3 = torch.float8_e4m3fn
THRESHOLDS = [0, 128, 129, 512, 10 ** 9]


def _F():
    import flash_cosine_sim_attention_amd as F
    return F


def _step(*a, **kw):
    return _F().flash_cosine_sim_attention_step_with_kvcache(*a, **kw)


def _ragged(*a, **kw):
    return _F().flash_cosine_sim_attention_varlen_with_kvcache(*a, **kw)


def _poison(q):
    """NaN-filled blocks of the sizes of o and lse, freed again: the allocator hands them to the op's outputs, so a row that no kernel
    writes shows as NaN (the C-ABI test below pre-fills its own buffers and does not depend on the allocator)"""
    junk = [torch.full(q.shape, float("nan"), device=q.device, dtype=q.dtype), torch.full(q.shape[:2], float("nan"), device=q.device)]
    del junk


def _compare(dtype, q, kc, vc, counts, kn, vn, cached, chunk_rows, table=None, host_tables=False, quant=None, **kw):
    """the ragged call at one split and the step call on clones of the caches: the bits of o, lse and both caches afterwards.  Returns the
    step call's (o, lse, kc, vc)."""
    total, H, D = q.shape
    Hk = kc.shape[1]
    page = kc.shape[2] if table is not None else 0
    capacity = table.shape[1] * page if table is not None else kc.shape[2]
    TP._assert_one_split(dtype, len(counts), H, Hk, D, total, capacity, page, kw.get("causal", False), kn is not None,
                         kw.get("l2norm_qk", True), kw.get("groups", 1), kw.get("scale", 8.0))
    dev = "cpu" if host_tables else "cuda"
    cu, sl = _cu(counts, dev), _i32(cached, dev)
    tab = None if table is None else table.to(dev)
    quant = quant or {}
    typed = (lambda t: t.view(E4M3)) if quant else (lambda t: t)
    k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    assert k1.stride() == kc.stride()
    with torch.no_grad():
        o_ref, lse_ref = _ragged(q, typed(k1), typed(v1), cu, kn, vn, sl, block_table=tab, max_seqlen_k=1, return_lse=True, **quant, **kw)
        _poison(q)
        o, lse = _step(q, typed(k2), typed(v2), cu, kn, vn, sl, block_table=tab, max_seqlen_k=1, return_lse=True, chunk_rows=chunk_rows,
                       **quant, **kw)
    torch.cuda.synchronize()
    assert o.shape == q.shape and o.dtype == q.dtype and lse.shape == (total, H) and lse.dtype == torch.float32
    assert torch.equal(_bits(o), _bits(o_ref)), f"o differs in {int((_bits(o) != _bits(o_ref)).sum())} elements (chunk_rows {chunk_rows})"
    assert torch.equal(_bits(lse), _bits(lse_ref)), f"lse differs in {int((_bits(lse) != _bits(lse_ref)).sum())} elements (chunk_rows {chunk_rows})"
    assert torch.equal(_bits(k2), _bits(k1)) and torch.equal(_bits(v2), _bits(v1)), "the caches differ after the append"
    return o, lse, k2, v2


# ---- bit for bit against the ragged call at one split ---------------------------------------------------------------------------------------

MIXED = TP.MIXED


@pytest.mark.parametrize("name,dtype,D,H,Hk,causal", MIXED, ids=[c[0] for c in MIXED])
def test_bitwise_mixed_batch_over_thresholds(name, dtype, D, H, Hk, causal):
    """the prefill tests' batch with append, at every threshold: 128 has the 16-token sequence exactly on it at G = 8, 129 sends it the other
    way, 0 and 10**9 are the one-kernel extremes"""
    q, kc, vc, kn, vn = TR._inputs(dtype, H, Hk, D, N_B, CAPACITY, seed=sum(map(ord, name)))
    for t in THRESHOLDS:
        o, lse, k2, v2 = _compare(dtype, q, kc, vc, N_B, kn, vn, CACHED, t, causal=causal)
        assert torch.isfinite(o).all() and torch.isfinite(lse).all(), t
    assert torch.equal(_bits(k2), _bits(TR._appended(kc, kn, N_B, CACHED))) and torch.equal(_bits(v2), _bits(TR._appended(vc, vn, N_B, CACHED)))


@pytest.mark.parametrize("dtype,D,H,Hk", [("bf16", 128, 8, 2), ("f16", 64, 6, 2), ("bf16", 64, 8, 8)])
@pytest.mark.parametrize("causal", [False, True])
def test_bitwise_mixed_batch_without_append(dtype, D, H, Hk, causal):
    q, kc, vc, _, _ = TR._inputs(dtype, H, Hk, D, N_B, CAPACITY, seed=D + H, append=False)
    cu = _cu(N_B, "cpu").tolist()
    for t in THRESHOLDS + [None]:
        o, lse, _, _ = _compare(dtype, q, kc, vc, N_B, None, None, CACHED, t, causal=causal)
        for b in (0, 4):      # nothing cached: no visible key at all
            assert (o[cu[b]:cu[b + 1]] == 0).all() and torch.isneginf(lse[cu[b]:cu[b + 1]]).all()


FP8 = [(f"{dt}_d{d}_{'l2norm' if l2 else 'raw'}_p{page}_{scales}", dt, d, l2, page, scales)
       for dt, d in (("bf16", 128), ("f16", 64), ("bf16", 64), ("f16", 128)) for l2 in (True, False)
       for page, scales in ((16, "per_seq_head"), (0, "per_head"), (0, "scalar"))]


@pytest.mark.parametrize("name,dtype,D,l2norm,page,scales", FP8, ids=[c[0] for c in FP8])
def test_bitwise_fp8_cache(name, dtype, D, l2norm, page, scales):
    """an e4m3fn cache with distinct scales per (sequence, K/V head), per K/V head and as scalars, l2norm on and off, paged and contiguous,
    with the quantising append (the codes in the caches equal the ragged call's): every sequence on the chunk kernel (0), and routed (128)"""
    H, Hk, cap = 8, 2, 1216
    q, kc, vc, kn, vn = TR._inputs(dtype, H, Hk, D, N_B, cap, seed=sum(map(ord, name)))
    kw = dict(causal=True)
    if not l2norm:
        q, kc = TK._unit_normalised(q, kc, 1, False)
        _, kn = TK._unit_normalised(q, kn, 1, False)
        kw.update(l2norm_qk=False, scale=1.0)
    (kc, ks), (vc, vs) = T8._quantise(kc), T8._quantise(vc)
    spread = 1 + torch.arange(ks.numel(), device="cuda", dtype=torch.float32).view_as(ks) / 16      # every (sequence, K/V head) its own value
    ks, vs = ks * spread, vs * spread.flip(0)
    assert ks.shape == (len(N_B), Hk) and ks.unique().numel() == ks.numel() and vs.unique().numel() == vs.numel()
    if scales == "per_head":
        ks, vs = ks[3].contiguous(), vs[5].contiguous()
    elif scales == "scalar":
        ks, vs = ks[3, 1].clone(), vs[5, 0].clone()
    kc, vc = kc.view(torch.uint8), vc.view(torch.uint8)
    table = None
    if page:
        kc, vc, table = _paged(kc, vc, page, seed=D)
    for t in (0, 128):
        o, lse, k2, v2 = _compare(dtype, q, kc, vc, N_B, kn, vn, CACHED, t, table=table, quant=dict(k_scale=ks, v_scale=vs), **kw)
        assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    assert not torch.equal(k2, kc)


EDGE_L = TP.EDGE_L
edge_inputs = TP.edge_inputs


@pytest.mark.parametrize("L", EDGE_L)
def test_bitwise_windows_on_the_chunk_kernel(edge_inputs, L):
    """one sequence of 130 tokens (five tiles at G = 4) against L cached positions, no append, every sequence on the chunk kernel: window
    starts on and off the 32-key and the 64-key boundaries, tiles whose first stage is not stage 0, a bounded right side, and (130 > L under
    causal, or a window that ends before key 0) rows without a visible key"""
    for dtype, (q, kc, vc) in edge_inputs.items():
        for left in (0, 1, 31, 32, 63, 64, 65, 200):
            for right in (0, 5, -1):
                for causal in (False, True):
                    o, lse, _, _ = _compare(dtype, q, kc, vc, [130], None, None, [L], 0, causal=causal, window_size=(left, right))
                    if causal and L < 130:
                        assert torch.isneginf(lse[:130 - L]).all() and (_bits(o[:130 - L]) == 0).all()


@pytest.mark.parametrize("dtype,D", [("bf16", 128), ("f16", 64)])
def test_bitwise_window_and_fp8_together(dtype, D):
    H, Hk, cap = 8, 2, 1216
    q, kc, vc, kn, vn = TR._inputs(dtype, H, Hk, D, N_B, cap, seed=D)
    (kc, ks), (vc, vs) = T8._quantise(kc), T8._quantise(vc)
    kc, vc, table = _paged(kc.view(torch.uint8), vc.view(torch.uint8), 16, seed=3)
    for t, window, causal in ((0, (100, 0), False), (128, (65, -1), True), (0, (31, 5), False)):
        _compare(dtype, q, kc, vc, N_B, kn, vn, CACHED, t, table=table, quant=dict(k_scale=ks, v_scale=vs), causal=causal, window_size=window)


@pytest.mark.parametrize("name,dtype,kw", TP.REGIMES, ids=[c[0] for c in TP.REGIMES])
@pytest.mark.parametrize("D", [64, 128])
def test_bitwise_regimes(name, dtype, kw, D):
    q, kc, vc, kn, vn = TR._inputs(dtype, 8, 2, D, N_B, CAPACITY, seed=sum(map(ord, name)) + D)
    q, kc = TK._unit_normalised(q, kc, kw.get("groups", 1), kw.get("l2norm_qk", True))
    _, kn = TK._unit_normalised(q, kn, 1, kw.get("l2norm_qk", True))
    for t in (128, None):
        o, lse, _, _ = _compare(dtype, q, kc, vc, N_B, kn, vn, CACHED, t, causal=True, **kw)
        assert torch.isfinite(o).all() and torch.isfinite(lse).all()


@pytest.mark.parametrize("name,page,host", TP.LAYOUTS, ids=[c[0] for c in TP.LAYOUTS])
@pytest.mark.parametrize("dtype,D,causal", [("bf16", 128, True), ("f16", 64, False)])
def test_bitwise_layouts(name, page, host, dtype, D, causal):
    """the vLLM layouts passed transposed, NaN in every slot at or beyond L_b, device and host tables (a host table also skips a launch)"""
    H, Hk, cap = 8, 2, 1216
    q, kc, vc, kn, vn = TR._inputs(dtype, H, Hk, D, N_B, cap, seed=page + D)
    for b, (s, n) in enumerate(zip(CACHED, N_B)):
        kc[b, :, s + n:] = float("nan")
        vc[b, :, s + n:] = float("nan")
    table = None
    if page:
        kc, vc, table = _paged(kc, vc, page, seed=page)
    else:
        kc, vc = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (kc, vc))
    for t in (0, 128, 10 ** 9):
        o, lse, _, _ = _compare(dtype, q, kc, vc, N_B, kn, vn, CACHED, t, table=table, host_tables=host, causal=causal)
        assert torch.isfinite(o).all() and torch.isfinite(lse).all(), "a NaN behind a sequence's length reached the output"


# ---- the routing is observed ------------------------------------------------------------------------------------------------------------------

def _launched(fn):
    from flash_cosine_sim_attention_amd import _lib
    torch.cuda.synchronize()
    _lib.profile_collect()
    _lib.profile_enable(True)
    try:
        with torch.no_grad():
            fn()
        torch.cuda.synchronize()
        return [s["name"] for s in _lib.profile_collect()]
    finally:
        _lib.profile_enable(False)


def test_the_kernels_launched_follow_the_routing():
    H, Hk, D = 8, 2, 128
    q, kc, vc, kn, vn = TR._inputs("bf16", H, Hk, D, N_B, CAPACITY, seed=1)
    call = lambda dev, t, **kw: _step(q, kc.clone(), vc.clone(), _cu(N_B, dev), kn, vn, _i32(CACHED, dev), chunk_rows=t, **kw)
    for dev in ("cuda", "cpu"):
        # (the op always computes the lse, as the prefill op does: the combine is the lse form with return_lse or without)
        assert _launched(lambda: call(dev, 128)) == ["kv_append_ragged", "step_decode", "step_combine_lse", "step_prefill"]
    assert _launched(lambda: call("cpu", 128, return_lse=True)) == ["kv_append_ragged", "step_decode", "step_combine_lse", "step_prefill"]
    assert _launched(lambda: call("cpu", 10 ** 9)) == ["kv_append_ragged", "step_decode", "step_combine_lse"]
    assert _launched(lambda: call("cpu", 0)) == ["kv_append_ragged", "step_prefill"]
    assert _launched(lambda: call("cuda", 0)) == ["kv_append_ragged", "step_decode", "step_combine_lse", "step_prefill"]      # a device table: both
    (k8, ks), (v8, vs) = T8._quantise(kc), T8._quantise(vc)
    got = _launched(lambda: _step(q, k8.clone(), v8.clone(), _cu(N_B), kn, vn, _i32(CACHED), k_scale=ks, v_scale=vs, chunk_rows=128))
    assert got == ["kv_append_ragged_fp8", "step_decode_fp8", "step_combine_lse_fp8", "step_prefill"]
    # no chunk kernel for float32 (or D = 96): the ragged call's launches, nothing else
    f32 = [t.float() for t in (q, kc, vc, kn, vn)]
    got = _launched(lambda: _step(f32[0], f32[1], f32[2], _cu(N_B), f32[3], f32[4], _i32(CACHED), chunk_rows=0))
    assert got == ["kv_append_ragged", "decode_ragged", "decode_combine_lse_ragged"]
    q96, kc96, vc96, kn96, vn96 = TR._inputs("bf16", H, Hk, 96, N_B, CAPACITY, seed=2)
    got = _launched(lambda: _step(q96, kc96, vc96, _cu(N_B, "cpu"), kn96, vn96, _i32(CACHED, "cpu"), chunk_rows=10 ** 9, return_lse=True))
    assert got == ["kv_append_ragged", "decode_ragged", "decode_combine_lse_ragged"]


# ---- real split counts ------------------------------------------------------------------------------------------------------------------------

def _step_workspace(dtype, B, H, Hk, D, total_q, max_k, capacity, causal, chunk_rows, bound, no_decode=0, no_chunk=0):
    from flash_cosine_sim_attention_amd import _lib
    lib = _lib.load()
    prob = _lib.problem(DT[dtype], (B, H, Hk, total_q, max_k, D), causal, False, True, 1, 8.0)
    kv = _lib.KvCache()
    kv.capacity, kv.new_len = capacity, 1
    seqs = _lib.Varlen(None, None, total_q, 0)
    st = _lib.KvCacheStep(chunk_rows, no_decode, bound, no_chunk, 0)
    return int(lib.fcsa_forward_kvcache_step_workspace_bytes(C.byref(prob), C.byref(kv), C.byref(seqs), None, None, C.byref(st)))


SPLITS = [("mixed_bf16_d128", "bf16", 128, N_B, CACHED, CAPACITY, False), ("mixed_f16_d64", "f16", 64, N_B, CACHED, CAPACITY, False),
          ("deep_decodes_bf16_d128", "bf16", 128, [1, 1, 4, 1, 200, 1], [1023, 1000, 1019, 512, 300, 1023], 1024, False),
          ("deep_decodes_fp8_f16_d128", "f16", 128, [1, 1, 4, 1, 200, 1], [1023, 1000, 1019, 512, 300, 1023], 1024, True)]


@pytest.mark.parametrize("name,dtype,D,counts,cached,cap,fp8", SPLITS, ids=[c[0] for c in SPLITS])
def test_real_split_counts_against_the_oracle(name, dtype, D, counts, cached, cap, fp8):
    """max_seqlen_k = the capacity: the decode side runs more than one key split (asserted from the workspace query).  o against the float64
    oracle under the ragged tests' policy and bars (fp8: on the values the codes mean, as the fp8 tests do); the chunk-routed rows are still
    bit-equal to the ragged call at one split."""
    H, Hk = 8, 2
    total = sum(counts)
    q, kc, vc, kn, vn = TR._inputs(dtype, H, Hk, D, counts, cap, seed=len(name))
    one = TP._align(total * H * D * 4) + TP._align(total * H * 8)
    assert _step_workspace(dtype, len(counts), H, Hk, D, total, cap, cap, True, 128, -1) >= TP._align(2 * total * H * D * 4) > one
    quant = {}
    typed = lambda t: t
    if fp8:
        (kc, ks), (vc, vs) = T8._quantise(kc), T8._quantise(vc)
        quant, typed = dict(k_scale=ks, v_scale=vs), (lambda t: t.view(E4M3))
        kc, vc = kc.view(torch.uint8), vc.view(torch.uint8)
    cu, sl = _cu(counts), _i32(cached)
    k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    with torch.no_grad():
        o_ref, lse_ref = _ragged(q, typed(k1), typed(v1), cu, kn, vn, sl, max_seqlen_k=1, causal=True, return_lse=True, **quant)
        _poison(q)
        o, lse = _step(q, typed(k2), typed(v2), cu, kn, vn, sl, max_seqlen_k=cap, causal=True, return_lse=True, chunk_rows=128, **quant)
    torch.cuda.synchronize()
    assert torch.equal(_bits(k2), _bits(k1)) and torch.equal(_bits(v2), _bits(v1))
    cul = _cu(counts, "cpu").tolist()
    chunk_rows_ = [i for b, n in enumerate(counts) if (H // Hk) * n >= 128 for i in range(cul[b], cul[b + 1])]
    assert chunk_rows_ and torch.equal(_bits(o[chunk_rows_]), _bits(o_ref[chunk_rows_])) and torch.equal(_bits(lse[chunk_rows_]), _bits(lse_ref[chunk_rows_]))
    lens = [s + n for s, n in zip(cached, counts)]
    if fp8:
        ks_, vs_ = T8._seqs(k2.view(E4M3), v2.view(E4M3), quant["k_scale"], quant["v_scale"], lens)
    else:
        ks_, vs_ = TK._seqs(k2, v2, lens)
    TR._verify(dtype, o, q, counts, ks_, vs_, dict(causal=True), "step_" + name)
    for b, n in enumerate(counts):      # the lse under test_gpu_kvcache_lse.check_lse, per sequence as test_lse_ragged does
        if n:
            qb = q[cul[b]:cul[b + 1]].permute(1, 0, 2).unsqueeze(0)
            kb = ks_[b].cpu().numpy() if fp8 else ks_[b]
            TL.check_lse(dtype, lse[cul[b]:cul[b + 1]].permute(1, 0).unsqueeze(0), qb, [kb], dict(causal=True), f"step_{name}_seq{b}")


# ---- the visibility probe ---------------------------------------------------------------------------------------------------------------------

# the ragged decode cases the chunk kernel takes (fp8 and windowed ones included, where the table has them), the prefill tests' chunk
# cases, and those again on an fp8 cache and under a window (bounded on both sides; bounded on the left under causal)
PROBE = [c for c in VP.decode_cases() if c[10] is not None and c[1] in ("bf16", "f16") and c[2] in (64, 128)]
_CHUNKS = [c for c in TP.PROBE if c[0].startswith("chunk_")]
PROBE += [c for c in _CHUNKS if c not in PROBE]
PROBE += [("fp8_" + c[0], *c[1:12], True, *c[13:]) for c in _CHUNKS[::2]]
PROBE += [("window_" + c[0], *c[1:14], (33, 0) if c[11] else (70, 5)) for c in _CHUNKS[1::2]]
PROBE += [("fp8_window_" + c[0], *c[1:12], True, c[13], (64, -1)) for c in _CHUNKS[:1]]


def test_the_probe_table_has_the_fp8_and_windowed_ragged_cases():
    assert sum(bool(c[12]) for c in PROBE) >= 5 and sum(c[14] != (-1, -1) for c in PROBE) >= 5 and len(PROBE) >= len(TP.PROBE) + 9
    assert len({c[0] for c in PROBE}) == len(PROBE)


@pytest.mark.parametrize("chunk_rows", [0, None])
@pytest.mark.parametrize("name,dtype,D,H,Hk,N,cap,page,lens,n_new,counts,causal,fp8,kw,window", PROBE, ids=[c[0] for c in PROBE])
def test_probe_step(monkeypatch, chunk_rows, name, dtype, D, H, Hk, N, cap, page, lens, n_new, counts, causal, fp8, kw, window):
    step = _F().flash_cosine_sim_attention_step_with_kvcache
    ns = types.SimpleNamespace(flash_cosine_sim_attention_varlen_with_kvcache=lambda *a, **k: step(*a, chunk_rows=chunk_rows, **k))
    monkeypatch.setattr(VP, "_F", lambda: ns)
    scale, l2 = VP.probe_scale(kw)
    fails = VP.judge(dtype, name, VP.run_decode(dtype, D, H, Hk, N, cap, page, lens, n_new, counts, causal, fp8, scale, l2, "cuda", window,
                                                kw.get("append", True), seed=len(name)))
    assert not fails, (name, fails)


# ---- caller-owned strided buffers through the C ABI -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,dtype,D,H,Hk,page,fp8,window", [("fp8_paged", "bf16", 128, 8, 2, 16, True, None),
                                                               ("window", "f16", 64, 5, 1, 0, False, (70, 3))])
def test_step_call_stays_inside_its_buffers(name, dtype, D, H, Hk, page, fp8, window):
    """q, k_new, v_new, the caches, the scales and the tables inside one arena pre-filled with 0xFF bytes with guard bands between them; o
    and lse are strided views of larger buffers; the workspace has exactly the size the query gives.  No guard byte changes, what the call
    does not own keeps its fill, every owned element is written (0xFF.. is NaN in every type here), and the result is the Python call's."""
    from flash_cosine_sim_attention_amd import _lib
    lib = _lib.load()
    dt = DT[dtype]
    counts, cached, cap = [1, 0, 37, 130, 3], [5, 40, 0, 100, 200], 256
    B, total = len(counts), sum(counts)
    mb = cap // page if page else 0
    nb = B * mb + 2
    ces = 1 if fp8 else 2
    cache_elems = (nb * page if page else B * cap) * Hk * D
    prob = _lib.problem(dt, (B, H, Hk, max(counts), cap, D), True, False, True, 1, 8.0)
    kv = _lib.KvCache()
    kv.capacity, kv.page_size, kv.num_blocks, kv.new_len = cap, page, nb if page else 0, 1
    seqs = _lib.Varlen(None, None, total, 0)
    st = _lib.KvCacheStep(128, 0, -1, 0, 0)
    win = _lib.Window(*window) if window else None
    winp = C.byref(win) if window else None
    wsb = int(lib.fcsa_forward_kvcache_step_workspace_bytes(C.byref(prob), C.byref(kv), C.byref(seqs), None, winp, C.byref(st)))
    assert wsb >= total * H * (D + 2) * 4
    ar = Arena((total + 5) * H * (D + 8) * 2 + (total + 5) * (H + 3) * 4 + (total * H * D + 2 * total * Hk * D) * 2 + 2 * cache_elems * ces
               + 4 * (2 * B + 1 + B * max(mb, 1)) + 8 * B * Hk + wsb + 40 * (4096 + 256))
    g = torch.Generator(device="cuda").manual_seed(D)

    def rnd(shape):
        t = ar.take(shape, dt)
        t.copy_(torch.randn(shape, device="cuda", dtype=torch.float32, generator=g).to(dt))
        return t

    q, kn, vn = rnd((total, H, D)), rnd((total, Hk, D)), rnd((total, Hk, D))
    cshape = (nb, Hk, page, D) if page else (B, Hk, cap, D)
    quant = {}
    if fp8:
        kc, vc = ar.take(cshape, torch.uint8), ar.take(cshape, torch.uint8)
        kc.copy_(torch.randint(0, 0x78, cshape, device="cuda", generator=g, dtype=torch.uint8))      # finite positive codes
        vc.copy_(torch.randint(0, 0x78, cshape, device="cuda", generator=g, dtype=torch.uint8))
        ks, vs = ar.take((B, Hk), torch.float32), ar.take((B, Hk), torch.float32)
        ks.copy_(torch.rand(B, Hk, device="cuda", generator=g) + 0.5), vs.copy_(torch.rand(B, Hk, device="cuda", generator=g) + 0.5)
        quant = dict(k_scale=ks, v_scale=vs)
    else:
        kc, vc = rnd(cshape), rnd(cshape)
    cu, sl = ar.take((B + 1,), torch.int32), ar.take((B,), torch.int32)
    cu.copy_(_cu(counts)), sl.copy_(_i32(cached))
    table = None
    if page:
        table = ar.take((B, mb), torch.int32)
        table.copy_(torch.randperm(nb, generator=torch.Generator().manual_seed(1))[:B * mb].reshape(B, mb).to(torch.int32))
    o_full, lse_full = ar.take((total + 5, H, D + 8), dt), ar.take((total + 5, H + 3), torch.float32)
    o, lse = o_full[2:2 + total, :, :D], lse_full[3:3 + total, 1:1 + H]
    ws = ar.take((wsb,), torch.uint8)
    assert ws.data_ptr() % 256 == 0
    inputs = [q, kn, vn, cu, sl] + ([table] if page else []) + list(quant.values())
    before = [t.clone() for t in inputs]
    k_ref, v_ref = kc.clone(), vc.clone()

    packed = lambda t: _lib.Tensor(t.data_ptr(), 0, t.stride(1), t.stride(0))
    kv.k_cache, kv.v_cache = _lib.tensor4(kc), _lib.tensor4(vc)
    kv.k_new, kv.v_new = packed(kn), packed(vn)
    kv.cache_seqlens = sl.data_ptr()
    if page:
        kv.block_table, kv.block_table_stride = table.data_ptr(), mb
    seqs = _lib.Varlen(cu.data_ptr(), None, total, 0)
    none = _lib.Tensor(None, 0, 0, 0)
    fa = _lib.ForwardArgs(prob, packed(q), none, none, packed(o), None, None, None, _lib.NormState(None, None, None, None), ws.data_ptr(), wsb,
                          torch.cuda.current_stream().cuda_stream)
    lo = _lib.LseOut(lse.data_ptr(), 0, lse.stride(1), lse.stride(0))
    qz = None
    if fp8:
        qz = _lib.KvCacheQuant()
        qz.cache_dtype, qz.k_scale, qz.v_scale = _lib.FCSA_CACHE_E4M3, ks.data_ptr(), vs.data_ptr()
        qz.k_scale_stride0, qz.k_scale_stride1, qz.v_scale_stride0, qz.v_scale_stride1 = Hk, 1, Hk, 1
    _lib.check(lib.fcsa_forward_kvcache_step(C.byref(fa), C.byref(kv), C.byref(seqs), C.byref(qz) if fp8 else None, winp, C.byref(st),
                                             C.byref(lo)), "fcsa_forward_kvcache_step")
    torch.cuda.synchronize()
    assert ar.guards_intact(), "a byte outside the call's buffers was written"
    for t, b in zip(inputs, before):
        assert torch.equal(t, b), "an input changed"
    assert torch.isfinite(o).all() and not torch.isnan(lse).all() and not torch.isnan(lse).any()
    own = torch.zeros_like(o_full, dtype=torch.bool)
    own[2:2 + total, :, :D] = True
    assert (o_full.view(torch.int16)[~own] == -1).all(), "an element of the o buffer outside the view was written"
    own = torch.zeros_like(lse_full, dtype=torch.bool)
    own[3:3 + total, 1:1 + H] = True
    assert (lse_full.view(torch.int32)[~own] == -1).all(), "an element of the lse buffer outside the view was written"
    typed = (lambda t: t.view(E4M3)) if fp8 else (lambda t: t)
    with torch.no_grad():
        o_py, lse_py = _step(q, typed(k_ref), typed(v_ref), cu, kn, vn, sl, block_table=table, max_seqlen_q=max(counts), causal=True,
                             return_lse=True, chunk_rows=128, window_size=window or (-1, -1), **quant)
    torch.cuda.synchronize()
    assert torch.equal(_bits(o), _bits(o_py)) and torch.equal(_bits(lse), _bits(lse_py))
    assert torch.equal(_bits(kc), _bits(k_ref)) and torch.equal(_bits(vc), _bits(v_ref))
    assert FILL == 0xFF


# ---- HIP-graph capture ------------------------------------------------------------------------------------------------------------------------

def test_step_captured_in_a_graph_with_device_tables_that_change_the_routes():
    """device cu_seqlens_q, cache_seqlens and block_table with every bound given: captured once and replayed; the table contents change ON
    THE DEVICE so that other sequences are the chunks.  Each replay equals the ragged call at one split on the same tables and cache
    contents, bit for bit (o, lse, caches)."""
    dtype, H, Hk, D, cap, total = "bf16", 8, 2, 128, 1216, 338
    q, _, _, kn, vn = TR._inputs(dtype, H, Hk, D, [total], 1, seed=9)
    _, kc, vc, _, _ = TR._inputs(dtype, H, Hk, D, [0, 0, 0, 0], cap, seed=10)
    kc, vc, table = _paged(kc, vc, 16, seed=2)
    table = table.cuda()
    cu, sl = _cu([1, 0, 37, 300]), _i32([100, 7, 0, 650])
    f = lambda k_, v_: _step(q, k_, v_, cu, kn, vn, sl, block_table=table, max_seqlen_q=total, max_seqlen_k=1, causal=True, return_lse=True,
                             chunk_rows=128, max_decode_tokens=total)
    ref = lambda k_, v_: _ragged(q, k_, v_, cu, kn, vn, sl, block_table=table, max_seqlen_q=total, max_seqlen_k=1, causal=True, return_lse=True)
    TP._assert_one_split(dtype, 4, H, Hk, D, total, cap, 16, True, True)
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            f(kc.clone(), vc.clone())                                # warm-up (allocator, the kernels' LDS attribute)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        k_eager, v_eager = kc.clone(), vc.clone()
        with torch.cuda.graph(g):
            o, lse = f(kc, vc)
        steps = (([1, 0, 37, 300], [100, 7, 0, 650]), ([300, 1, 0, 37], [31, 64, 5, 916]), ([32, 31, 33, 242], [0, 0, 1179, 0]),
                 ([1, 1, 1, 335], [500, 0, 3, 20]))
        for step, (counts, lens) in enumerate(steps):
            cu.copy_(_cu(counts)), sl.copy_(_i32(lens))
            g.replay()
            o_ref, lse_ref = ref(k_eager, v_eager)
            torch.cuda.synchronize()
            assert torch.equal(_bits(o), _bits(o_ref)) and torch.equal(_bits(lse), _bits(lse_ref)), step
            assert torch.equal(_bits(kc), _bits(k_eager)) and torch.equal(_bits(vc), _bits(v_eager)), step


# ---- zero sizes -------------------------------------------------------------------------------------------------------------------------------

def test_zero_sizes():
    H, Hk, D, cap = 8, 2, 64, 64
    g = torch.Generator(device="cuda").manual_seed(0)
    kc = torch.randn(3, Hk, cap, D, device="cuda", generator=g).to(torch.bfloat16)
    vc = torch.randn(3, Hk, cap, D, device="cuda", generator=g).to(torch.bfloat16)
    k0, v0 = kc.clone(), vc.clone()
    q = torch.empty(0, H, D, device="cuda", dtype=torch.bfloat16)
    kn = torch.empty(0, Hk, D, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        for t in (None, 0, 10 ** 9):
            # every N_b = 0 (so total_q = 0), with (empty) rows to append and without; then no sequence at all (B = 0)
            o, lse = _step(q, kc, vc, _cu([0, 0, 0]), kn, kn.clone(), _i32([0, 5, 64]), causal=True, return_lse=True, chunk_rows=t)
            assert o.shape == (0, H, D) and o.dtype == torch.bfloat16 and lse.shape == (0, H) and lse.dtype == torch.float32
            assert _step(q, kc, vc, _cu([0, 0, 0]), cache_seqlens=_i32([0, 5, 64]), chunk_rows=t).shape == (0, H, D)
            o, lse = _step(q, kc[:0], vc[:0], _cu([]), kn, kn.clone(), _i32([]), return_lse=True, chunk_rows=t)
            assert o.shape == (0, H, D) and lse.shape == (0, H)
            # H = 0: rows without heads
            q0 = torch.empty(5, 0, D, device="cuda", dtype=torch.bfloat16)
            o, lse = _step(q0, kc, vc, _cu([0, 5, 0]), cache_seqlens=_i32([3, 5, 64]), return_lse=True, chunk_rows=t)
            assert o.shape == (5, 0, D) and lse.shape == (5, 0)
            # sequences without rows beside one that has some
            q5 = torch.randn(5, H, D, device="cuda", generator=g).to(torch.bfloat16)
            o, lse, _, _ = _compare("bf16", q5, kc, vc, [0, 5, 0], None, None, [3, 5, 64], t)
            assert torch.isfinite(o).all()
    torch.cuda.synchronize()
    assert torch.equal(_bits(kc), _bits(k0)) and torch.equal(_bits(vc), _bits(v0))
