"""Attention states without a GPU: return_lse of the two cache functions on the CPU path against float64 numpy, merge_attention_states and
flash_cosine_sim_attention_with_shared_prefix on CPU tensors, the Python argument checks, the C ABI's additions (exports, header mirror,
argument checks on fake pointers that are never dereferenced) and the shared merge arithmetic of csrc/fcsa_dispatch.h
(tests/native/merge_states_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import flash_cosine_sim_attention_amd as F
import lse_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_INF = float("-inf")
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    from flash_cosine_sim_attention_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _r(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g)


def test_exports_and_header_mirror(lib):
    from flash_cosine_sim_attention_amd import _lib
    assert {"flash_cosine_sim_attention_with_shared_prefix", "merge_attention_states"} <= set(F.__all__)
    assert callable(F.merge_attention_states) and callable(F.flash_cosine_sim_attention_with_shared_prefix)
    assert {"fcsa_forward_kvcache_lse", "fcsa_merge_states"} <= set(_lib.EXPORTS)
    assert hasattr(lib, "fcsa_forward_kvcache_lse") and hasattr(lib, "fcsa_merge_states")
    assert _lib.ABI_VERSION == 4 and lib.fcsa_debug(None, 0) == 4          # additive: the version stays
    assert [n for n, _ in _lib.LseOut._fields_] == ["lse", "stride0", "stride1", "stride2"] and C.sizeof(_lib.LseOut) == 32
    names = [n for n, _ in _lib.MergeArgs._fields_]
    assert names == ["dtype", "size0", "size1", "size2", "dim_head", "states", "o_in", "lse_in", "o", "lse", "stream"]
    assert _lib.MERGE_MAX_STATES == 8 and len(_lib.MergeArgs().o_in) == 8 and len(_lib.MergeArgs().lse_in) == 8


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_new_struct_layout_matches_c_compiler(tmp_path):
    from flash_cosine_sim_attention_amd import _lib
    prog = tmp_path / "layout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "fcsa.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(fcsa_lse_out), sizeof(fcsa_merge_args), offsetof(fcsa_merge_args, o_in),
         offsetof(fcsa_merge_args, lse_in), offsetof(fcsa_merge_args, o), offsetof(fcsa_merge_args, lse), offsetof(fcsa_merge_args, stream));
  printf("%zu %zu %zu %zu\n", sizeof(fcsa_forward_args), sizeof(fcsa_kvcache), sizeof(fcsa_kvcache_quant), sizeof(fcsa_varlen));
  return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    M = _lib.MergeArgs
    assert list(map(int, out[0].split())) == [C.sizeof(_lib.LseOut), C.sizeof(M), M.o_in.offset, M.lse_in.offset, M.o.offset, M.lse.offset,
                                              M.stream.offset]
    assert list(map(int, out[1].split())) == [C.sizeof(_lib.ForwardArgs), C.sizeof(_lib.KvCache), C.sizeof(_lib.KvCacheQuant), C.sizeof(_lib.Varlen)]


def test_cabi_argument_checks(lib):
    from flash_cosine_sim_attention_amd import _lib
    p = _lib.problem(torch.bfloat16, (2, 8, 2, 1, 64, 64))
    args = _lib.ForwardArgs()
    args.p = p
    args.q = _lib.Tensor(0x1000, 512, 64, 64)
    args.o = _lib.Tensor(0x2000, 512, 64, 64)
    kv = _lib.KvCache()
    kv.k_cache, kv.v_cache, kv.capacity = _lib.Tensor(0x10000, 8192, 4096, 64), _lib.Tensor(0x20000, 8192, 4096, 64), 64
    lse = _lib.LseOut(0x3000, 8, 1, 1)
    f = lib.fcsa_forward_kvcache_lse
    assert f(C.byref(args), C.byref(kv), None, None, None, None) == INVALID and b"null" in lib.fcsa_last_error()
    assert f(None, C.byref(kv), None, None, None, C.byref(lse)) == INVALID
    assert f(C.byref(args), C.byref(kv), None, None, None, C.byref(_lib.LseOut())) == INVALID and b"lse" in lib.fcsa_last_error()
    # like the entry points it mirrors: a non-NULL inv_l is refused, and a valid call without a workspace stops at the workspace check
    args.inv_l = 0x4000
    assert f(C.byref(args), C.byref(kv), None, None, None, C.byref(lse)) == INVALID and b"inv_l" in lib.fcsa_last_error()
    assert lib.fcsa_forward_kvcache(C.byref(args), C.byref(kv)) == INVALID
    args.inv_l = None
    assert f(C.byref(args), C.byref(kv), None, None, None, C.byref(lse)) == -4 and b"workspace" in lib.fcsa_last_error()
    assert f(C.byref(args), C.byref(kv), None, None, C.byref(_lib.Window(-3, 0)), C.byref(lse)) == INVALID
    seqs = _lib.Varlen(0x5000, None, 2, 0)
    kv.new_len = 2
    assert f(C.byref(args), C.byref(kv), C.byref(seqs), None, None, C.byref(lse)) == INVALID and b"flag" in lib.fcsa_last_error()
    # fcsa_merge_states
    m = lib.fcsa_merge_states
    a = _lib.MergeArgs()
    a.dtype, a.size0, a.size1, a.size2, a.dim_head, a.states = 2, 2, 8, 1, 64, 9
    assert m(None) == INVALID
    assert m(C.byref(a)) == INVALID and b"two steps" in lib.fcsa_last_error()
    a.states = 0
    assert m(C.byref(a)) == INVALID
    a.states, a.dim_head = 2, 6
    assert m(C.byref(a)) == UNSUPPORTED and b"dim_head" in lib.fcsa_last_error()
    a.dim_head, a.dtype = 64, 7
    assert m(C.byref(a)) == UNSUPPORTED and b"dtype" in lib.fcsa_last_error()
    a.dtype = 2
    assert m(C.byref(a)) == INVALID and b"null" in lib.fcsa_last_error()              # o_in[0] has no pointer
    a.o_in[0] = _lib.Tensor(0x1008, 512, 64, 64)
    assert m(C.byref(a)) == INVALID and b"aligned" in lib.fcsa_last_error()
    a.size0 = 0
    assert m(C.byref(a)) == 0                                                        # no rows: nothing to do


def test_python_argument_checks():
    r = _r(0)
    o, l = r(2, 3, 4, 16), r(2, 3, 4)
    with pytest.raises(ValueError, match="two steps"):
        F.merge_attention_states([o] * 9, [l] * 9)
    with pytest.raises(ValueError):
        F.merge_attention_states([], [])
    with pytest.raises(ValueError):
        F.merge_attention_states([o, o], [l])
    with pytest.raises(ValueError, match="shape"):
        F.merge_attention_states([o, r(2, 3, 5, 16)], [l, l])
    with pytest.raises(ValueError, match="shape"):
        F.merge_attention_states([o], [r(2, 3, 5)])
    with pytest.raises(TypeError, match="dtype"):
        F.merge_attention_states([o, o.half()], [l, l])
    with pytest.raises(TypeError, match="float32"):
        F.merge_attention_states([o], [l.double()])
    with pytest.raises(TypeError):
        F.merge_attention_states([o.double()], [l.double()])
    with pytest.raises(ValueError):
        F.merge_attention_states([r(3, 16)], [r(3)])
    with pytest.raises(RuntimeError, match="forward-only"):
        F.merge_attention_states([o.clone().requires_grad_()], [l])
    q, pk, kc = r(2, 4, 1, 16), r(1, 2, 32, 16), r(2, 2, 64, 16)
    sp = F.flash_cosine_sim_attention_with_shared_prefix
    with pytest.raises(ValueError, match="window"):
        sp(q, pk, pk, kc, kc, cache_seqlens=3, window_size=(8, 0))
    with pytest.raises(ValueError, match="prefix_len"):
        sp(q, pk, pk, kc, kc, prefix_len=33, cache_seqlens=3)
    with pytest.raises(ValueError, match="one sequence"):
        sp(q, kc, kc, kc, kc, cache_seqlens=3)
    with pytest.raises(TypeError):
        sp(q, pk, pk, kc, kc, prefix_len=2.0, cache_seqlens=3)
    with pytest.raises(ValueError, match="N_b <= L_b"):           # a query inside the prefix under causal: N_b > L_b + 1
        sp(r(2, 4, 3, 16), pk, pk, kc, kc, cache_seqlens=torch.tensor([5, 1], dtype=torch.int32), causal=True)
    with pytest.raises(ValueError, match="N_b <= L_b"):           # ... an append shorter than the queries does not lift it
        sp(r(2, 4, 16, 16), pk, pk, kc, kc, k_new=r(2, 2, 1, 16), v_new=r(2, 2, 1, 16), cache_seqlens=0, causal=True)
    # N_b = L_b + 1 is fine (the first query sees the prefix alone): one query on an empty own cache, and 3 queries behind 2 positions
    o_edge = sp(q, pk, pk, kc, kc, cache_seqlens=0, causal=True)
    assert float((o_edge - F.flash_cosine_sim_attention_with_kvcache(q, pk.expand(2, -1, -1, -1), pk.expand(2, -1, -1, -1))).abs().max()) <= 2e-6
    sp(r(2, 4, 3, 16), pk, pk, kc, kc, cache_seqlens=torch.tensor([5, 2], dtype=torch.int32), causal=True)
    # return_lse is a bool: a window_size passed positionally by an older caller lands on it and is refused, not read as a flag
    for fn, args in ((F.flash_cosine_sim_attention_with_kvcache, (q, kc, kc)),
                     (F.flash_cosine_sim_attention_varlen_with_kvcache, (r(2, 4, 16), kc, kc, torch.tensor([0, 1, 2], dtype=torch.int32)))):
        with pytest.raises(TypeError, match="return_lse"):
            fn(*args, cache_seqlens=3, return_lse=(8, 0))
    with pytest.raises(ValueError, match="multiple of 8"):        # 16-bit rows are whole 16-byte chunks
        F.merge_attention_states([r(2, 3, 4, 12).half()], [r(2, 3, 4)])
    F.merge_attention_states([r(2, 3, 4, 12)], [r(2, 3, 4)])       # float32: a multiple of 4
    o1, l1 = F.flash_cosine_sim_attention_with_kvcache(q, kc, kc, cache_seqlens=3, return_lse=True)
    assert l1.shape == (2, 4, 1) and l1.dtype == torch.float32


CPU_CASES = [dict(), dict(causal=True), dict(scale=16.0, groups=2), dict(l2norm_qk=False, scale=0.5, causal=True), dict(window_size=(9, 0))]


@pytest.mark.parametrize("kw", CPU_CASES, ids=lambda kw: "_".join(f"{k}{v}" for k, v in kw.items()) or "default")
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_path_lse_against_float64(kw, dtype):
    r = _r(3)
    B, H, Hk, N, D, cap, n_new = 3, 4, 2, 3, 32, 70, 2
    q, kc, vc, kn, vn = (t.to(dtype) for t in (r(B, H, N, D), r(B, Hk, cap, D), r(B, Hk, cap, D), r(B, Hk, n_new, D), r(B, Hk, n_new, D)))
    cached = [0, 17, cap - n_new]
    kc2, vc2 = kc.clone(), vc.clone()
    o_plain = F.flash_cosine_sim_attention_with_kvcache(q, kc2, vc2, kn, vn, torch.tensor(cached, dtype=torch.int32), **kw)
    o, lse = F.flash_cosine_sim_attention_with_kvcache(q, kc, vc, kn, vn, torch.tensor(cached, dtype=torch.int32), return_lse=True, **kw)
    assert torch.equal(o, o_plain) and torch.equal(kc, kc2) and torch.equal(vc, vc2)
    assert lse.shape == (B, H, N) and lse.dtype == torch.float32 and not torch.isnan(lse).any()
    okw = {k: v for k, v in kw.items() if k != "window_size"}
    win = kw.get("window_size", (-1, -1))
    for b, c in enumerate(cached):
        # the CPU path normalises in float32 and rounds q^, k^ back to the dtype before the product: do the same for the reference's inputs
        qb, kb = q[b], kc[b, :, :c + n_new]
        if okw.get("l2norm_qk", True):
            from flash_cosine_sim_attention_amd.cpu import normalise_groups
            qb, kb = normalise_groups(qb, okw.get("groups", 1)), normalise_groups(kb, okw.get("groups", 1))
        ref = R.lse_rows(qb.double().numpy(), kb.double().numpy(), window=win, **{**okw, "l2norm_qk": False})
        got = lse[b].double().numpy()
        assert np.array_equal(np.isneginf(got), np.isneginf(ref))
        live = np.isfinite(ref)
        assert np.abs(got[live] - ref[live]).max(initial=0.0) <= 2e-5, (kw, b)
    # the ragged function: every sequence's rows equal the equal-N call on that sequence alone
    counts = [1, 0, 4]
    cu = torch.tensor([0, 1, 1, 5], dtype=torch.int32)
    qp, knp, vnp = (t.to(dtype) for t in (r(5, H, D), r(5, Hk, D), r(5, Hk, D)))
    sl = torch.tensor([0, 17, 30], dtype=torch.int32)
    kc3, vc3 = kc.clone(), vc.clone()
    op, lp = F.flash_cosine_sim_attention_varlen_with_kvcache(qp, kc3, vc3, cu, knp, vnp, sl, return_lse=True, **kw)
    assert lp.shape == (5, H) and lp.dtype == torch.float32
    for b, (lo, n) in enumerate(zip([0, 1, 1], counts)):
        if n == 0:
            continue
        rows = lambda t: t[lo:lo + n].transpose(0, 1).unsqueeze(0)
        ob, lb = F.flash_cosine_sim_attention_with_kvcache(rows(qp), kc[b:b + 1].clone(), vc[b:b + 1].clone(), rows(knp), rows(vnp),
                                                           sl[b:b + 1], return_lse=True, **kw)
        assert torch.equal(rows(op), ob) and torch.equal(lp[lo:lo + n].transpose(0, 1).unsqueeze(0), lb)


def test_cpu_empty_rows_are_minus_inf():
    r = _r(4)
    q, kc = r(2, 4, 16, 16), r(2, 2, 64, 16)
    o, lse = F.flash_cosine_sim_attention_with_kvcache(q, kc, kc, cache_seqlens=torch.tensor([0, 5], dtype=torch.int32), causal=True, return_lse=True)
    assert (lse[0] == NEG_INF).all() and (o[0] == 0).all()
    assert (lse[1, :, :11] == NEG_INF).all() and torch.isfinite(lse[1, :, 11:]).all() and (o[1, :, :11] == 0).all()
    o, lse = F.flash_cosine_sim_attention_with_kvcache(q[:, :, :2], kc, kc, cache_seqlens=40, window_size=(0, 0), return_lse=True)
    assert torch.isfinite(lse).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_merge_identities_cpu(dtype):
    r = _r(5)
    a, la = r(2, 3, 5, 16).to(dtype), 3 * r(2, 3, 5)
    o, lse = F.merge_attention_states([a], [la])
    assert torch.equal(o, a) and torch.equal(lse, la) and o.is_contiguous() and lse.is_contiguous()
    a.view(-1)[::7] = -0.0                                         # signed zeros survive: compare bits, not values
    bits = lambda t: t.view({2: torch.int16, 4: torch.int32}[t.element_size()])
    o, lse = F.merge_attention_states([a], [la])
    assert torch.equal(bits(o), bits(a))
    nan_o, empty = torch.full_like(a, float("nan")), torch.full_like(la, NEG_INF)
    for os, lses in (([a, nan_o], [la, empty]), ([nan_o, a], [empty, la]), ([nan_o, a, nan_o], [empty, la, empty])):
        o, lse = F.merge_attention_states(os, lses)
        assert torch.equal(bits(o), bits(a)) and torch.equal(lse, la)
    o, lse = F.merge_attention_states([nan_o, nan_o], [empty, empty])
    assert (o == 0).all() and (lse == NEG_INF).all()
    # S states against float64, through strided views, 4-D and packed 3-D
    os = [r(2, 5, 3, 16).to(dtype).transpose(1, 2) for _ in range(8)]
    lses = [(3 * r(3, 2, 5)).permute(1, 0, 2) for _ in range(8)]
    lses[2][0, 1] = NEG_INF
    os[2][0, 1] = float("nan")
    for S in (2, 3, 8):
        o, lse = F.merge_attention_states(os[:S], lses[:S])
        ro, rl = R.merge_reference([t.double().numpy() for t in os[:S]], [t.double().numpy() for t in lses[:S]])
        u = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dtype]
        assert (np.abs(o.double().numpy() - ro) <= u * np.abs(ro) + 2.0 ** -19 * 4).all()
        assert np.abs(lse.double().numpy() - rl).max() <= 1e-5
        o3, lse3 = F.merge_attention_states([t.flatten(0, 1) for t in os[:S]], [t.flatten(0, 1) for t in lses[:S]])
        assert torch.equal(o3, o.flatten(0, 1)) and torch.equal(lse3, lse.flatten(0, 1))


def test_one_attention_over_two_calls_cpu():
    r = _r(6)
    B, H, Hk, N, D, L = 2, 4, 2, 2, 32, 150      # (N = 2: under causal every query sees the whole first part for every cut <= L - N + 1)
    q, kc, vc = r(B, H, N, D), r(B, Hk, 160, D), r(B, Hk, 160, D)
    kv = F.flash_cosine_sim_attention_with_kvcache
    for causal in (False, True):
        whole, lse_whole = kv(q, kc, vc, cache_seqlens=L, causal=causal, return_lse=True)
        for cuts in ((1,), (32,), (77,), (149,), (32, 77)):
            edges = [0, *cuts, L]
            states = [kv(q, kc[:, :, lo:hi], vc[:, :, lo:hi], causal=causal and hi == L, return_lse=True) for lo, hi in zip(edges[:-1], edges[1:])]
            o, lse = F.merge_attention_states([s[0] for s in states], [s[1] for s in states])
            assert float((o - whole).abs().max()) <= 2e-6 and float((lse - lse_whole).abs().max()) <= 4e-6, (causal, cuts)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("P", [0, 45])
def test_shared_prefix_cpu(P, causal):
    r = _r(7)
    B, H, Hk, N, D, cap = 3, 4, 2, 2, 32, 64
    q, pk, pv, kc, vc, kn, vn = r(B, H, N, D), r(1, Hk, 48, D), r(1, Hk, 48, D), r(B, Hk, cap, D), r(B, Hk, cap, D), r(B, Hk, N, D), r(B, Hk, N, D)
    own = torch.tensor([0, 17, 40], dtype=torch.int32)
    fk = torch.cat([pk[:, :, :P].expand(B, -1, -1, -1), kc], dim=2).contiguous()
    fv = torch.cat([pv[:, :, :P].expand(B, -1, -1, -1), vc], dim=2).contiguous()
    pk0, kc_s, vc_s = pk.clone(), kc.clone(), vc.clone()
    sp = F.flash_cosine_sim_attention_with_shared_prefix
    o, lse = sp(q, pk, pv, kc, vc, prefix_len=P, k_new=kn, v_new=vn, cache_seqlens=own, causal=causal, return_lse=True)
    plain, lse_plain = F.flash_cosine_sim_attention_with_kvcache(q, fk, fv, kn, vn, own + P, causal=causal, return_lse=True)
    suffix, lse_suffix = F.flash_cosine_sim_attention_with_kvcache(q, kc_s, vc_s, kn, vn, own, causal=causal, return_lse=True)
    assert torch.equal(kc, kc_s) and torch.equal(vc, vc_s) and torch.equal(pk, pk0)
    assert float((o - plain).abs().max()) <= 2e-6 and float((lse - lse_plain).abs().max()) <= 4e-6
    if P == 0:
        assert torch.equal(o, suffix) and torch.equal(lse, lse_suffix)
    # a one-element tensor prefix_len, and the packed form with N_b = [1, 0, 4]
    o_t = sp(q, pk, pv, kc_s.clone(), vc_s.clone(), prefix_len=torch.tensor([P], dtype=torch.int32), k_new=kn, v_new=vn, cache_seqlens=own, causal=causal)
    assert o_t.shape == q.shape and float((o_t - plain).abs().max()) <= 2e-6
    cu = torch.tensor([0, 1, 1, 5], dtype=torch.int32)
    qp, knp, vnp = r(5, H, D), r(5, Hk, D), r(5, Hk, D)
    fk2, fv2 = fk.clone(), fv.clone()
    op, lp = sp(qp, pk, pv, kc_s.clone(), vc_s.clone(), prefix_len=P, cu_seqlens_q=cu, k_new=knp, v_new=vnp, cache_seqlens=own, causal=causal, return_lse=True)
    pp, lpp = F.flash_cosine_sim_attention_varlen_with_kvcache(qp, fk2, fv2, cu, knp, vnp, own + P, causal=causal, return_lse=True)
    assert op.shape == qp.shape and lp.shape == (5, H)
    assert float((op - pp).abs().max()) <= 2e-6 and float((lp - lpp).abs().max()) <= 4e-6


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_merge_arithmetic_native(tmp_path):
    """tests/native/merge_states_check.cpp: one state and a state beside empty ones come back bit for bit, all states empty give (0, -inf)
    without a NaN, an empty state's NaN o never leaks, random merges against long double, and the LSE of a decoded row."""
    exe = str(tmp_path / "merge_states_check")
    b = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "flash_cosine_sim_attention_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "merge_states_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]
