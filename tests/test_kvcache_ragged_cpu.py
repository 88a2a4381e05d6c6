"""Ragged decode steps without a GPU (flash_cosine_sim_attention_varlen_with_kvcache, fcsa_forward_kvcache_varlen): the CPU path against a
per-sequence loop over flash_cosine_sim_attention_with_kvcache (outputs and cache contents equal), the Python validation of host tables,
the C ABI's argument checks (fake pointers, never dereferenced), exports and header, the workspace formula, and the tile-lookup rule of
csrc/fcsa_dispatch.h (tests/native/ragged_tile_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

import flash_cosine_sim_attention_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
kv = F.flash_cosine_sim_attention_with_kvcache

# the mixed batch of the feature's description: a first token into an empty cache, an empty sequence, a few speculative tokens, exactly one
# row tile, a ragged chunk, a plain decode deep in a long cache, a prompt chunk of several row tiles
N_B = [1, 0, 5, 16, 37, 1, 130]
CACHED = [0, 17, 300, 5, 0, 1023, 200]
CAPACITY = 1200


def ragged():
    return F.flash_cosine_sim_attention_varlen_with_kvcache


def _cu(counts):
    c = [0]
    for n in counts:
        c.append(c[-1] + n)
    return torch.tensor(c, dtype=torch.int32)


def _batch(H, Hk, D, counts, cap, seed, dtype=torch.float32, page=None):
    """(q, k_new, v_new packed; caches contiguous [B, Hk, cap, D], or a shuffled pool [nb, Hk, page, D] with its block table)"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(dtype)
    B, total = len(counts), sum(counts)
    q, kn, vn = r(total, H, D), r(total, Hk, D), r(total, Hk, D)
    kc, vc = r(B, Hk, cap, D), r(B, Hk, cap, D)
    if page is None:
        return q, kn, vn, kc, vc, None
    mb = cap // page
    nb = B * mb + 3
    table = torch.randperm(nb, generator=g)[:B * mb].reshape(B, mb).to(torch.int32)
    pk, pv = torch.zeros(nb, Hk, page, D, dtype=dtype), torch.zeros(nb, Hk, page, D, dtype=dtype)
    for b in range(B):
        for i in range(mb):
            pk[int(table[b, i])] = kc[b, :, i * page:(i + 1) * page]
            pv[int(table[b, i])] = vc[b, :, i * page:(i + 1) * page]
    return q, kn, vn, pk, pv, table


def _loop(q, kc, vc, cu, kn, vn, cached, table, scales=None, **kw):
    """The only alternative without the feature: one flash_cosine_sim_attention_with_kvcache call per sequence, on its own cache."""
    out = torch.zeros_like(q)
    c = cu.tolist()
    for b in range(len(c) - 1):
        lo, hi = c[b], c[b + 1]
        rows = lambda t: None if t is None else t[lo:hi].permute(1, 0, 2).unsqueeze(0)
        sl = None if cached is None else torch.tensor([cached[b]], dtype=torch.int32)
        quant = {} if scales is None else dict(k_scale=scales[0][b:b + 1], v_scale=scales[1][b:b + 1])
        if table is None:
            o = kv(rows(q), kc[b:b + 1], vc[b:b + 1], rows(kn), rows(vn), sl, **quant, **kw)
        else:
            o = kv(rows(q), kc, vc, rows(kn), rows(vn), sl, block_table=table[b:b + 1], **quant, **kw)
        out[lo:hi] = o[0].permute(1, 0, 2)
    return out


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("Hk", [4, 1])
def test_cpu_path_equals_per_sequence_loop(paged, causal, Hk):
    H, D = 4, 32
    q, kn, vn, kc, vc, table = _batch(H, Hk, D, N_B, CAPACITY, seed=3 + Hk, page=16 if paged else None)
    cu, sl = _cu(N_B), torch.tensor(CACHED, dtype=torch.int32)
    kc2, vc2 = kc.clone(), vc.clone()
    o = ragged()(q, kc, vc, cu, kn, vn, sl, block_table=table, causal=causal, scale=4)
    ref = _loop(q, kc2, vc2, cu, kn, vn, CACHED, table, causal=causal, scale=4)
    assert o.shape == q.shape and torch.equal(o, ref)
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)
    assert sl.tolist() == CACHED                       # cache_seqlens is not advanced
    if not paged:                                      # the appended slots, and nothing else
        c = cu.tolist()
        for b, (s, n) in enumerate(zip(CACHED, N_B)):
            assert torch.equal(kc[b, :, s:s + n], kn[c[b]:c[b + 1]].permute(1, 0, 2))
            assert torch.equal(vc[b, :, s:s + n], vn[c[b]:c[b + 1]].permute(1, 0, 2))


def test_cpu_window_fp8_and_no_append():
    H, Hk, D = 4, 2, 32
    cu = _cu(N_B)
    # a window (64, 0), per sequence
    q, kn, vn, kc, vc, _ = _batch(H, Hk, D, N_B, CAPACITY, seed=11)
    kc2, vc2 = kc.clone(), vc.clone()
    sl = torch.tensor(CACHED, dtype=torch.int32)
    o = ragged()(q, kc, vc, cu, kn, vn, sl, window_size=(64, 0))
    assert torch.equal(o, _loop(q, kc2, vc2, cu, kn, vn, CACHED, None, window_size=(64, 0)))
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)
    # an fp8 cache with per-(sequence, head) scales: the append quantises
    q, kn, vn, kc, vc, _ = _batch(H, Hk, D, N_B, CAPACITY, seed=12, dtype=torch.bfloat16)
    ks, vs = torch.rand(len(N_B), Hk) * 0.02 + 0.005, torch.rand(len(N_B), Hk) * 0.02 + 0.005
    kc8, vc8 = F.cpu.quantise_e4m3(kc, ks[:, :, None, None]), F.cpu.quantise_e4m3(vc, vs[:, :, None, None])
    kc9, vc9 = kc8.clone(), vc8.clone()
    o = ragged()(q, kc8, vc8, cu, kn, vn, sl, causal=True, k_scale=ks, v_scale=vs)
    ref = _loop(q, kc9, vc9, cu, kn, vn, CACHED, None, scales=(ks, vs), causal=True)
    assert torch.equal(o, ref)
    assert torch.equal(kc8.view(torch.uint8), kc9.view(torch.uint8)) and torch.equal(vc8.view(torch.uint8), vc9.view(torch.uint8))
    # no append: L_b = cache_seqlens[b]; under causal N_b > L_b leaves the first N_b - L_b rows without a visible key (0), L_b == 0 all
    q, _, _, kc, vc, _ = _batch(H, Hk, D, N_B, CAPACITY, seed=13)
    before = kc.clone()
    o = ragged()(q, kc, vc, cu, cache_seqlens=sl, causal=True)
    assert torch.equal(o, _loop(q, kc, vc, cu, None, None, CACHED, None, causal=True))
    assert torch.equal(kc, before)
    c = cu.tolist()
    assert (o[c[0]:c[1]] == 0).all() and (o[c[4]:c[5]] == 0).all()          # L_b == 0
    assert (o[c[3]:c[3] + 16 - 5] == 0).all() and (o[c[3] + 16 - 5:c[4]] != 0).any()      # N_b = 16 > L_b = 5
    # cache_seqlens None: every sequence full
    full = ragged()(q, kc, vc, cu)
    assert torch.equal(full, _loop(q, kc, vc, cu, None, None, None, None))
    assert torch.equal(full, ragged()(q, kc, vc, cu, cache_seqlens=CAPACITY))


def test_host_validation_errors():
    H, Hk, D = 4, 2, 16
    counts, cap = [1, 3, 0], 32
    q, kn, vn, kc, vc, _ = _batch(H, Hk, D, counts, cap, seed=1)
    cu, sl = _cu(counts), torch.tensor([3, 4, 5], dtype=torch.int32)
    f = ragged()
    f(q, kc, vc, cu, kn, vn, sl)                       # the valid call
    for bad in ([1, 1, 4, 4], [0, 1, 4, 5], [0, 3, 2, 4]):          # start, end, order
        with pytest.raises(ValueError, match="cu_seqlens_q"):
            f(q, kc, vc, torch.tensor(bad, dtype=torch.int32), kn, vn, sl)
    with pytest.raises(TypeError, match="cu_seqlens_q"):
        f(q, kc, vc, cu.long(), kn, vn, sl)
    with pytest.raises(TypeError, match="cu_seqlens_q"):
        f(q, kc, vc, [0, 1, 4, 4], kn, vn, sl)
    with pytest.raises(ValueError, match="capacity"):
        f(q, kc, vc, cu, kn, vn, torch.tensor([3, cap - 2, 5], dtype=torch.int32))          # 30 + 3 new tokens > 32
    f(q, kc, vc, cu, cache_seqlens=torch.tensor([3, cap, 5], dtype=torch.int32))             # ... fine without the append
    f(q, kc, vc, cu, kn, vn, torch.tensor([3, cap - 3, cap], dtype=torch.int32))            # an empty sequence appends nothing
    with pytest.raises(ValueError, match="capacity"):
        f(q, kc, vc, cu, kn, vn, torch.tensor([-1, 4, 5], dtype=torch.int32))
    with pytest.raises(ValueError, match="cache_seqlens"):
        f(q, kc, vc, cu, kn, vn)                       # None = every sequence full: no slot left to append to
    with pytest.raises(TypeError, match="cache_seqlens"):
        f(q, kc, vc, cu, kn, vn, torch.tensor([3, 4], dtype=torch.int32))
    with pytest.raises(ValueError, match="together"):
        f(q, kc, vc, cu, kn, None, sl)
    with pytest.raises(ValueError, match="packed like q"):
        f(q, kc, vc, cu, kn[:-1], vn[:-1], sl)
    with pytest.raises(ValueError, match="packed"):
        f(q.unsqueeze(0), kc, vc, cu, kn, vn, sl)
    with pytest.raises(ValueError, match="batch mismatch"):
        f(q, kc[:2], vc[:2], cu, kn, vn, sl)
    with pytest.raises(ValueError, match="heads"):
        f(torch.zeros(4, 3, D), kc, vc, cu)
    with pytest.raises(ValueError, match="max_seqlen_q"):
        f(q, kc, vc, cu, kn, vn, sl, max_seqlen_q=-1)
    with pytest.raises(ValueError, match="max_seqlen_k"):
        f(q, kc, vc, cu, kn, vn, sl, max_seqlen_k=1.5)
    with pytest.raises(ValueError, match="window_size"):
        f(q, kc, vc, cu, kn, vn, sl, window_size=(-2, 0))
    with pytest.raises(RuntimeError, match="forward-only"):
        f(q.clone().requires_grad_(), kc, vc, cu, kn, vn, sl)
    with pytest.raises(RuntimeError, match="forward-only"):
        f(q, kc, vc, cu, kn.clone().requires_grad_(), vn, sl)
    with torch.no_grad():
        f(q.clone().requires_grad_(), kc, vc, cu, kn, vn, sl)
    with pytest.raises(TypeError, match="scale"):
        f(q, kc, vc, cu, kn, vn, sl, k_scale=1.0)      # scales belong to fp8 caches
    # paged: page size, table shape, block ids
    pool = torch.zeros(8, Hk, 16, D)
    tab = torch.tensor([[0, 1], [2, 3], [4, 5]], dtype=torch.int32)
    f(q, pool, pool.clone(), cu, kn, vn, sl, block_table=tab)
    with pytest.raises(ValueError, match="page_size"):
        f(q, torch.zeros(8, Hk, 24, D), torch.zeros(8, Hk, 24, D), cu, kn, vn, sl, block_table=tab)
    with pytest.raises(TypeError, match="block_table"):
        f(q, pool, pool.clone(), cu, kn, vn, sl, block_table=tab[:2])
    with pytest.raises(ValueError, match="block_table"):
        f(q, pool, pool.clone(), cu, kn, vn, sl, block_table=torch.tensor([[0, 1], [8, 3], [4, 5]], dtype=torch.int32))
    # bounds never change the result
    a = f(q, kc.clone(), vc.clone(), cu, kn, vn, sl, causal=True)
    b = f(q, kc.clone(), vc.clone(), cu, kn, vn, sl, causal=True, max_seqlen_q=1, max_seqlen_k=2)
    assert torch.equal(a, b)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from flash_cosine_sim_attention_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _problem(**kw):
    from flash_cosine_sim_attention_amd import _lib
    d = dict(dtype=_lib.FCSA_BF16, batch=4, heads=8, kv_heads=2, q_len=16, k_len=4096, dim_head=128, causal=1,
             bias_batch_dim=0, l2norm_qk=1, groups=1, scale=8.0)
    d.update(kw)
    return _lib.Problem(*[d[f[0]] for f in _lib.Problem._fields_])


def _args(prob, inv_l=None, mask=None, bias=None):
    from flash_cosine_sim_attention_amd import _lib
    t = _lib.Tensor(0x1000, 0, 128, 1024)             # fake, never dereferenced: validation fails first
    return _lib.ForwardArgs(prob, t, t, t, t, inv_l, mask, bias, _lib.NormState(None, None, None, None), None, 0, None)


def _cache(**kw):
    from flash_cosine_sim_attention_amd import _lib
    t = _lib.Tensor(0x10000, 4096 * 256, 4096 * 128, 128)
    d = dict(k_cache=t, v_cache=t, capacity=4096, page_size=0, num_blocks=0, new_len=0, cache_seqlens=None, block_table=None,
             block_table_stride=0, k_new=_lib.Tensor(0, 0, 0, 0), v_new=_lib.Tensor(0, 0, 0, 0))
    d.update(kw)
    return _lib.KvCache(*[d[f[0]] for f in _lib.KvCache._fields_])


def _seqs(total_q=20, cu=0x4000):
    from flash_cosine_sim_attention_amd import _lib
    return _lib.Varlen(cu, None, total_q, 0)


def test_exports_header_and_abi_version(lib):
    from flash_cosine_sim_attention_amd import _lib
    for name in ("fcsa_forward_kvcache_varlen", "fcsa_forward_kvcache_varlen_workspace_bytes"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert name + "(" in open(_lib.HEADER).read()
    assert _lib.ABI_VERSION == 4 and lib.fcsa_debug(None, 0) == 4
    buf = C.create_string_buffer(4096)
    lib.fcsa_debug(buf, 4096)
    assert b"decode_ragged" in buf.value
    assert "flash_cosine_sim_attention_varlen_with_kvcache" in F.__all__


def test_struct_layouts_unchanged(tmp_path):
    """The new declarations reuse the existing structs: sizeof / offsetof of each as gcc sees include/fcsa.h == the ctypes mirrors."""
    from flash_cosine_sim_attention_amd import _lib
    structs = {"fcsa_kvcache": _lib.KvCache, "fcsa_varlen": _lib.Varlen, "fcsa_kvcache_quant": _lib.KvCacheQuant, "fcsa_window": _lib.Window,
               "fcsa_forward_args": _lib.ForwardArgs}
    lines = []
    for name, cls in structs.items():
        lines.append(f"  printf(\"%zu\\n\", sizeof({name}));\n")
        lines += [f"  printf(\"%zu\\n\", offsetof({name}, {f[0]}));\n" for f in cls._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fcsa.h\"\nint main(void) {\n" + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    expect = []
    for cls in structs.values():
        expect += [C.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_]
    assert out == expect
    assert [f[0] for f in _lib.Varlen._fields_] == ["cu_seqlens_q", "cu_seqlens_k", "total_q", "total_k"]


def test_cabi_argument_checks(lib):
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
    from flash_cosine_sim_attention_amd import _lib
    call = lambda a, c, s, qz=None, w=None: lib.fcsa_forward_kvcache_varlen(C.byref(a) if a is not None else None, C.byref(c) if c is not None else None,
                                                                            C.byref(s) if s is not None else None, qz, w)
    ok_args = _args(_problem())
    assert call(None, _cache(), _seqs()) == INVALID and call(ok_args, None, _seqs()) == INVALID and call(ok_args, _cache(), None) == INVALID
    for kw in (dict(inv_l=0x2000), dict(mask=0x2000), dict(bias=0x2000)):
        assert call(_args(_problem(), **kw), _cache(), _seqs()) == INVALID and b"NULL" in lib.fcsa_last_error(), kw
    assert call(ok_args, _cache(), _seqs(cu=None)) == INVALID and b"cu_seqlens_q" in lib.fcsa_last_error()
    assert call(ok_args, _cache(), _seqs(total_q=-1)) == INVALID and b"total_q" in lib.fcsa_last_error()
    assert call(ok_args, _cache(new_len=2), _seqs()) == INVALID and b"flag" in lib.fcsa_last_error()
    assert call(ok_args, _cache(new_len=1), _seqs()) == INVALID and b"k_new" in lib.fcsa_last_error()
    assert call(ok_args, _cache(page_size=16), _seqs()) == INVALID and b"block_table" in lib.fcsa_last_error()
    assert call(ok_args, _cache(block_table=0x3000, page_size=24, num_blocks=8, block_table_stride=256), _seqs()) == INVALID
    assert call(ok_args, _cache(), _seqs(), None, C.byref(_lib.Window(-2, 0))) == INVALID and b"window" in lib.fcsa_last_error()
    assert call(_args(_problem(q_len=-1)), _cache(), _seqs()) == INVALID
    assert call(_args(_problem(dim_head=48)), _cache(), _seqs()) == UNSUPPORTED
    qz = _lib.KvCacheQuant(_lib.FCSA_CACHE_E4M3, 0x5000, 0x6000, 0, 0, 0, 0)
    assert call(_args(_problem(dtype=_lib.FCSA_F32)), _cache(), _seqs(), C.byref(qz)) == UNSUPPORTED
    assert call(ok_args, _cache(), _seqs(), C.byref(_lib.KvCacheQuant(7, 0x5000, 0x6000, 0, 0, 0, 0))) == UNSUPPORTED
    # valid calls: only the workspace is missing -- with and without window / quant / append, every D = 96 group width
    kn = _lib.Tensor(0x20000, 0, 128, 256)
    for c, qq, w in ((_cache(), None, None), (_cache(new_len=1, k_new=kn, v_new=kn, cache_seqlens=0x7000), None, None),
                     (_cache(), C.byref(qz), None), (_cache(), None, C.byref(_lib.Window(64, 0))), (_cache(), C.byref(qz), C.byref(_lib.Window(-1, 5)))):
        assert call(ok_args, c, _seqs(), qq, w) == WORKSPACE and b"workspace" in lib.fcsa_last_error()
    for groups in (2, 4, 8, 16, 32):
        assert call(_args(_problem(dim_head=96, groups=groups)), _cache(), _seqs()) == WORKSPACE
    # nothing to do, nothing dereferenced: no sequence, no packed row
    assert call(_args(_problem(batch=0)), _cache(), _seqs(total_q=0)) == 0
    assert call(ok_args, _cache(), _seqs(total_q=0)) == 0


def test_workspace_formula(lib):
    """[splits][total_q * H][D] f32 partials + [splits][total_q * H][2] f32 (max, sum), each 256-byte aligned.  The split count is
    decode_splits over Hk * (floor(G * total_q / 16) + B) workgroups -- pinned on shapes where it does not depend on the CU count -- and
    depends on total_q, never on B * max_seqlen_q."""
    al = lambda x: (x + 255) // 256 * 256
    def ws(B, H, Hk, total, D, cap, max_q=1, k_len=None, window=None):
        from flash_cosine_sim_attention_amd import _lib
        p = _problem(batch=B, heads=H, kv_heads=Hk, q_len=max_q, k_len=cap if k_len is None else k_len, dim_head=D)
        w = None if window is None else C.byref(_lib.Window(*window))
        return lib.fcsa_forward_kvcache_varlen_workspace_bytes(C.byref(p), C.byref(_cache(capacity=cap)), C.byref(_seqs(total_q=total)), None, w)
    expect = lambda rows, D, s: al(rows * s * D * 4) + al(rows * s * 8)
    assert ws(1, 1, 1, 1, 128, 5 * 128) == expect(1, 128, 5)                     # the keys-per-split minimum binds (128 keys at D = 128)
    assert ws(1, 1, 1, 1, 64, 100) == expect(1, 64, 1)
    assert ws(1, 2, 1, 3, 32, 1 << 22) == expect(6, 32, 128)                     # one slot, a long cache: the cap of 128 splits
    assert ws(2048, 8, 8, 4096, 128, 1 << 20) == expect(4096 * 8, 128, 1)        # 8 * (256 + 2048) workgroups: one split on any chip
    assert ws(1, 1, 1, 1, 128, 1 << 20, k_len=2 * 128) == expect(1, 128, 2)      # max_seqlen_k sizes the splits, clamped to the capacity
    assert ws(1, 1, 1, 1, 128, 3 * 128, k_len=1 << 30) == expect(1, 128, 3)
    # max_seqlen_q changes nothing without a window; under one it bounds the keys a sequence reads: min(max_k, left + max_q + 31)
    assert ws(1, 1, 1, 5, 128, 1 << 20, max_q=1) == ws(1, 1, 1, 5, 128, 1 << 20, max_q=5)
    assert ws(1, 1, 1, 4, 128, 1 << 20, max_q=4, window=(600, 0)) == expect(4, 128, (600 + 4 + 31) // 128)
    assert ws(1, 1, 1, 4, 128, 1 << 20, max_q=4, window=(-1, 0)) == ws(1, 1, 1, 4, 128, 1 << 20, max_q=4)
    assert ws(4, 8, 2, 0, 128, 4096) == 0
    assert lib.fcsa_forward_kvcache_varlen_workspace_bytes(None, None, None, None, None) == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_ragged_tile_lookup_rule(tmp_path):
    """tests/native/ragged_tile_check.cpp: for random tables the flat slots map onto exactly {(b, rt) : rt < ceil(G N_b / 16)}, each once;
    the bound floor(G total_q / 16) + B is never exceeded; empty sequences own nothing; malformed tables stay inside the tensors."""
    exe = str(tmp_path / "ragged_tile_check")
    b = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "flash_cosine_sim_attention_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "ragged_tile_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]
