"""Decoding against a key/value cache without a GPU: the CPU path of flash_cosine_sim_attention_with_kvcache against
plain_cosine_sim_attention per sequence, the Python validation, the C ABI's argument checks (fake pointers, never dereferenced), the
struct layout against gcc, the workspace formula and the split / window rules of csrc/fcsa_dispatch.h (tests/native/decode_split_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

import flash_cosine_sim_attention_amd as F
from flash_cosine_sim_attention_amd.ops import plain_cosine_sim_attention

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
kv = F.flash_cosine_sim_attention_with_kvcache


def _expected(q, kc, vc, lens, **kw):
    """plain_cosine_sim_attention of every sequence over its first L_b positions (K/V repeated over each query-head group); rows without a
    visible key are 0 (plain_cosine_sim_attention averages the values there)."""
    B, H = q.shape[:2]
    out = torch.zeros_like(q)
    for b, L in enumerate(lens):
        if L == 0:
            continue
        G = H // kc.shape[1]
        kb = kc[b:b + 1, :, :L].repeat_interleave(G, 1)
        vb = vc[b:b + 1, :, :L].repeat_interleave(G, 1)
        out[b:b + 1] = plain_cosine_sim_attention(q[b:b + 1], kb, vb, **kw)
        if kw.get("causal"):                          # rows without a visible key (L_b - N + i < 0) are 0, as in the dense op
            out[b, :, :max(q.shape[2] - L, 0)] = 0
    return out


def _data(B, H, Hk, N, cap, D, n_new, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    q, kc, vc = r(B, H, N, D), r(B, Hk, cap, D), r(B, Hk, cap, D)
    kn, vn = (r(B, Hk, n_new, D), r(B, Hk, n_new, D)) if n_new else (None, None)
    return q, kc, vc, kn, vn


@pytest.mark.parametrize("Hk", [4, 2, 1])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("N,n_new", [(1, 1), (3, 3), (4, 0), (2, 5)])
def test_cpu_semantics_append_ragged_causal(Hk, causal, N, n_new):
    B, H, cap, D = 4, 4, 48, 32
    q, kc, vc, kn, vn = _data(B, H, Hk, N, cap, D, n_new, seed=N * 10 + n_new + Hk)
    seq = [0, 1, 20, cap - n_new]                    # ragged, including L_b = n_new (0 when nothing is appended) and full capacity
    kc0, vc0 = kc.clone(), vc.clone()
    sl = torch.tensor(seq, dtype=torch.int32)
    o = kv(q, kc, vc, kn, vn, sl, causal=causal, scale=4)
    assert sl.tolist() == seq                         # cache_seqlens is not advanced
    for b, s in enumerate(seq):                       # the append position, nothing else touched
        if n_new:
            assert torch.equal(kc[b, :, s:s + n_new], kn[b]) and torch.equal(vc[b, :, s:s + n_new], vn[b])
        assert torch.equal(kc[b, :, :s], kc0[b, :, :s]) and torch.equal(kc[b, :, s + n_new:], kc0[b, :, s + n_new:])
        assert torch.equal(vc[b, :, :s], vc0[b, :, :s]) and torch.equal(vc[b, :, s + n_new:], vc0[b, :, s + n_new:])
    lens = [s + n_new for s in seq]
    ref = _expected(q, kc, vc, lens, causal=causal, scale=4)
    assert torch.allclose(o, ref, atol=2e-6, rtol=1e-5)
    if n_new == 0:
        assert (o[0] == 0).all()                      # L_b == 0: o = 0


@pytest.mark.parametrize("kw", [dict(groups=2, scale=8), dict(l2norm_qk=False, scale=1), dict(groups=4, scale=120)])
def test_cpu_groups_scales(kw):
    q, kc, vc, kn, vn = _data(2, 8, 2, 2, 40, 64, 2, seed=5)
    seq = [10, 30]
    o = kv(q, kc, vc, kn, vn, torch.tensor(seq, dtype=torch.int32), causal=True, **kw)
    ref = _expected(q, kc, vc, [s + 2 for s in seq], causal=True, **kw)
    assert torch.allclose(o, ref, atol=2e-5, rtol=1e-4)


def test_cpu_paged_equals_contiguous_and_int_seqlens():
    B, H, Hk, N, D, page, mb = 3, 4, 2, 2, 32, 16, 4
    cap = page * mb
    q, kc, vc, kn, vn = _data(B, H, Hk, N, cap, D, N, seed=3)
    seq = [0, 21, cap - N]
    perm = torch.randperm(B * mb + 3, generator=torch.Generator().manual_seed(1))[:B * mb].reshape(B, mb).to(torch.int32)
    pool_k = torch.full((B * mb + 3, Hk, page, D), float("nan"))
    pool_v = pool_k.clone()
    for b in range(B):
        for i in range(mb):
            pool_k[int(perm[b, i])] = kc[b, :, i * page:(i + 1) * page]
            pool_v[int(perm[b, i])] = vc[b, :, i * page:(i + 1) * page]
    sl = torch.tensor(seq, dtype=torch.int32)
    oc = kv(q, kc, vc, kn, vn, sl, causal=True)
    op = kv(q, pool_k, pool_v, kn, vn, sl, block_table=perm, causal=True)
    assert torch.equal(oc, op)
    unused = sorted(set(range(B * mb + 3)) - set(perm.flatten().tolist()))
    assert torch.isnan(pool_k[unused]).all()
    # an int cache_seqlens is the same length for every sequence
    q2, kc2, vc2, _, _ = _data(2, 4, 4, 1, 40, 16, 0, seed=9)
    assert torch.equal(kv(q2, kc2, vc2, cache_seqlens=17), kv(q2, kc2, vc2, cache_seqlens=torch.tensor([17, 17], dtype=torch.int32)))
    assert torch.equal(kv(q2, kc2, vc2), kv(q2, kc2, vc2, cache_seqlens=40))


def test_cpu_transposed_cache_layout():
    B, H, Hk, N, D, cap = 2, 4, 2, 1, 32, 30
    q, kc, vc, kn, vn = _data(B, H, Hk, N, cap, D, 1, seed=4)
    kt, vt = kc.transpose(1, 2).contiguous().transpose(1, 2), vc.transpose(1, 2).contiguous().transpose(1, 2)   # [B, L, Hk, D] storage
    sl = torch.tensor([4, 12], dtype=torch.int32)
    assert torch.equal(kv(q, kc, vc, kn, vn, sl), kv(q, kt, vt, kn, vn, sl))
    assert torch.equal(kc, kt) and torch.equal(vc, vt)


def test_validation_errors():
    q, kc, vc, kn, vn = _data(2, 4, 2, 1, 32, 16, 1)
    sl = torch.tensor([3, 4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="forward-only"):
        kv(q.clone().requires_grad_(), kc, vc, kn, vn, sl)
    with pytest.raises(RuntimeError, match="forward-only"):
        kv(q, kc, vc, kn.clone().requires_grad_(), vn, sl)
    with torch.no_grad():                             # grad mode off: inputs that require grad are fine
        kv(q.clone().requires_grad_(), kc, vc, kn, vn, sl)
    with pytest.raises(ValueError, match="together"):
        kv(q, kc, vc, kn, None, sl)
    with pytest.raises(ValueError, match="page_size"):
        kv(q, torch.zeros(4, 2, 24, 16), torch.zeros(4, 2, 24, 16), block_table=torch.zeros(2, 1, dtype=torch.int32), cache_seqlens=1)
    with pytest.raises(ValueError, match="capacity"):
        kv(q, kc, vc, kn, vn, torch.tensor([3, 32], dtype=torch.int32))
    with pytest.raises(ValueError, match="capacity"):
        kv(q, kc, vc, kn, vn, torch.tensor([-1, 2], dtype=torch.int32))
    with pytest.raises(ValueError, match="block_table"):
        kv(q, torch.zeros(4, 2, 16, 16), torch.zeros(4, 2, 16, 16), block_table=torch.tensor([[0, 4], [1, 2]], dtype=torch.int32),
           cache_seqlens=20)
    with pytest.raises(ValueError, match="heads"):
        kv(torch.zeros(2, 3, 1, 16), kc, vc)
    with pytest.raises(ValueError, match="cache_seqlens"):
        kv(q, kc, vc, kn, vn)                         # None = every sequence full: no slot left to append to


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from flash_cosine_sim_attention_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _problem(**kw):
    from flash_cosine_sim_attention_amd import _lib
    d = dict(dtype=_lib.FCSA_BF16, batch=2, heads=8, kv_heads=2, q_len=1, k_len=4096, dim_head=128, causal=1,
             bias_batch_dim=0, l2norm_qk=1, groups=1, scale=8.0)
    d.update(kw)
    return _lib.Problem(*[d[f[0]] for f in _lib.Problem._fields_])


def _args(prob, inv_l=None, mask=None, bias=None):
    from flash_cosine_sim_attention_amd import _lib
    t = _lib.Tensor(0x1000, 1024, 512, 64)            # fake, never dereferenced: validation fails first
    return _lib.ForwardArgs(prob, t, t, t, t, inv_l, mask, bias, _lib.NormState(None, None, None, None), None, 0, None)


def _cache(**kw):
    from flash_cosine_sim_attention_amd import _lib
    t = _lib.Tensor(0x10000, 4096 * 256, 4096 * 128, 128)
    d = dict(k_cache=t, v_cache=t, capacity=4096, page_size=0, num_blocks=0, new_len=0, cache_seqlens=None, block_table=None,
             block_table_stride=0, k_new=_lib.Tensor(0, 0, 0, 0), v_new=_lib.Tensor(0, 0, 0, 0))
    d.update(kw)
    return _lib.KvCache(*[d[f[0]] for f in _lib.KvCache._fields_])


def test_cabi_argument_checks(lib):
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
    for kw in (dict(inv_l=0x2000), dict(mask=0x2000), dict(bias=0x2000)):
        rc = lib.fcsa_forward_kvcache(C.byref(_args(_problem(), **kw)), C.byref(_cache()))
        assert rc == INVALID and b"NULL" in lib.fcsa_last_error(), kw
    rc = lib.fcsa_forward_kvcache(C.byref(_args(_problem())), None)
    assert rc == INVALID
    rc = lib.fcsa_forward_kvcache(C.byref(_args(_problem())), C.byref(_cache(block_table=0x3000, page_size=24, num_blocks=8,
                                                                             block_table_stride=256)))
    assert rc == INVALID and b"page_size" in lib.fcsa_last_error()
    rc = lib.fcsa_forward_kvcache(C.byref(_args(_problem())), C.byref(_cache(block_table=0x3000, page_size=32, num_blocks=0,
                                                                             block_table_stride=128)))
    assert rc == INVALID and b"blocks" in lib.fcsa_last_error()
    rc = lib.fcsa_forward_kvcache(C.byref(_args(_problem())), C.byref(_cache(page_size=16)))
    assert rc == INVALID and b"block_table" in lib.fcsa_last_error()
    rc = lib.fcsa_forward_kvcache(C.byref(_args(_problem())), C.byref(_cache(new_len=2)))
    assert rc == INVALID and b"k_new" in lib.fcsa_last_error()
    for groups in (2, 4, 8, 16, 32):             # D = 96 widths that straddle a lane's fragment: accepted (only the workspace is missing)
        rc = lib.fcsa_forward_kvcache(C.byref(_args(_problem(dim_head=96, groups=groups))), C.byref(_cache()))
        assert rc == WORKSPACE, (groups, lib.fcsa_last_error())
    rc = lib.fcsa_forward_kvcache(C.byref(_args(_problem(dim_head=96, groups=5))), C.byref(_cache()))
    assert rc == INVALID and b"groups" in lib.fcsa_last_error()
    rc = lib.fcsa_forward_kvcache(C.byref(_args(_problem(dim_head=48))), C.byref(_cache()))
    assert rc == UNSUPPORTED
    rc = lib.fcsa_forward_kvcache(C.byref(_args(_problem())), C.byref(_cache()))      # valid, but no workspace
    assert rc == WORKSPACE and b"workspace" in lib.fcsa_last_error()
    # zero-size batch: nothing to do, nothing dereferenced
    assert lib.fcsa_forward_kvcache(C.byref(_args(_problem(batch=0))), C.byref(_cache())) == 0


def test_workspace_formula(lib):
    """[splits][B * H * N][D] f32 partials + [splits][B * H * N][2] f32 (max, sum), each 256-byte aligned, with the split count pinned
    on shapes where it does not depend on the CU count: the keys-per-split minimum binds (few workgroups, a short cache), the workgroups
    alone exceed 8 per CU of any chip up to 1024 CUs (one split), or the 128-split cap binds (one workgroup, a long cache)."""
    al = lambda x: (x + 255) // 256 * 256
    def ws(B, H, Hk, N, D, cap, k_len=None):
        p = _problem(batch=B, heads=H, kv_heads=Hk, q_len=N, k_len=cap if k_len is None else k_len, dim_head=D)
        return lib.fcsa_forward_kvcache_workspace_bytes(C.byref(p), C.byref(_cache(capacity=cap)))
    expect = lambda B, H, N, D, s: al(B * H * N * s * D * 4) + al(B * H * N * s * 8)
    # min keys per split = max(16384 / D, 32): 128 keys at D = 128, 1024 at D = 16
    assert ws(1, 1, 1, 1, 128, 5 * 128) == expect(1, 1, 1, 128, 5)
    assert ws(1, 4, 1, 4, 16, 3 * 1024 + 7) == expect(1, 4, 4, 16, 3)          # G * N = 16: one row tile
    assert ws(1, 1, 1, 1, 64, 100) == expect(1, 1, 1, 64, 1)                    # shorter than one split's minimum
    assert ws(1024, 8, 8, 1, 128, 1 << 20) == expect(1024, 8, 1, 128, 1)      # 8192 workgroups: one split
    assert ws(1, 2, 1, 3, 32, 1 << 22) == expect(1, 2, 3, 32, 128)             # one workgroup, a long cache: the cap
    # max_seqlen_k below the capacity sizes the grid (it is clamped to the capacity)
    assert ws(1, 1, 1, 1, 128, 1 << 20, k_len=2 * 128) == expect(1, 1, 1, 128, 2)
    assert ws(1, 1, 1, 1, 128, 3 * 128, k_len=1 << 30) == expect(1, 1, 1, 128, 3)
    assert lib.fcsa_forward_kvcache_workspace_bytes(C.byref(_problem(q_len=0)), C.byref(_cache())) == 0
    assert lib.fcsa_forward_kvcache_workspace_bytes(None, None) == 0


def test_struct_layout_matches_c_compiler(tmp_path):
    """sizeof / offsetof of fcsa_kvcache as gcc sees include/fcsa.h == the ctypes mirror in _lib.py."""
    from flash_cosine_sim_attention_amd import _lib
    prog = tmp_path / "layout.c"
    fields = [f[0] for f in _lib.KvCache._fields_]
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fcsa.h\"\nint main(void) {\n"
                    "  printf(\"%zu\\n\", sizeof(fcsa_kvcache));\n"
                    + "".join(f"  printf(\"%zu\\n\", offsetof(fcsa_kvcache, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert out[0] == C.sizeof(_lib.KvCache)
    assert out[1:] == [getattr(_lib.KvCache, f).offset for f in fields]
    assert fields == ["k_cache", "v_cache", "capacity", "page_size", "num_blocks", "new_len", "cache_seqlens", "block_table",
                      "block_table_stride", "k_new", "v_new"]


def test_exports_and_abi_version(lib):
    from flash_cosine_sim_attention_amd import _lib
    assert "fcsa_forward_kvcache" in _lib.EXPORTS and "fcsa_forward_kvcache_workspace_bytes" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 4 and lib.fcsa_debug(None, 0) == 4


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_decode_split_rules(tmp_path):
    """tests/native/decode_split_check.cpp: bounded split count with a minimum of keys per split, a grid that covers the CUs when the
    cache is long enough, windows that tile [0, L_b) for every L_b in [0, capacity], clamped table entries, the groups rule."""
    exe = str(tmp_path / "decode_split_check")
    b = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "flash_cosine_sim_attention_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "decode_split_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]
