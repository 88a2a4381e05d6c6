"""CPU-only checks of packed variable-length sequences (fcsa_forward_varlen / fcsa_backward_varlen, flash_cosine_sim_attention_varlen):
the new symbols and their ctypes layout, the C ABI's argument validation (no kernel is launched by any call here), the workspace size,
the CPU forward path against the float64 oracle per sequence, and the span clamp / early-exit / form rules of csrc/fcsa_dispatch.h
through a g++ program (tests/native/varlen_span_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import cosine_sim_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARLEN_SYMBOLS = ("fcsa_forward_varlen", "fcsa_backward_varlen", "fcsa_backward_varlen_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    from flash_cosine_sim_attention_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_varlen_symbols_exported(lib):
    from flash_cosine_sim_attention_amd import _lib
    for n in VARLEN_SYMBOLS:
        assert n in _lib.EXPORTS
        assert hasattr(lib, n)


def test_varlen_struct_layout_matches_c_compiler(tmp_path):
    from flash_cosine_sim_attention_amd import _lib
    prog = tmp_path / "layout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "fcsa.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(fcsa_varlen), offsetof(fcsa_varlen, cu_seqlens_q), offsetof(fcsa_varlen, cu_seqlens_k),
         offsetof(fcsa_varlen, total_q), offsetof(fcsa_varlen, total_k));
  return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    V = _lib.Varlen
    assert got == [C.sizeof(V), V.cu_seqlens_q.offset, V.cu_seqlens_k.offset, V.total_q.offset, V.total_k.offset]


def _args(lib, dtype=torch.bfloat16, S=3, H=2, Hk=2, max_q=8, max_k=8, D=64, total_q=20, total_k=20):
    """Forward / backward argument blocks with fake (never dereferenced) device addresses: validation runs before any launch."""
    from flash_cosine_sim_attention_amd import _lib
    prob = _lib.problem(dtype, (S, H, Hk, max_q, max_k, D), True, False, True, 1, 8.0)
    fake = 1 << 32
    t = lambda: _lib.Tensor(fake, 0, D, H * D)
    norm = _lib.NormState(fake, fake, fake, fake)
    fa = _lib.ForwardArgs(prob, t(), t(), t(), t(), fake, None, None, norm, None, 0, None)
    ba = _lib.BackwardArgs(prob, t(), t(), fake, t(), t(), t(), None, None, norm, t(), t(), t(), None, fake, 1 << 30, None)
    seqs = _lib.Varlen(fake, fake, total_q, total_k)
    return fa, ba, seqs


def test_varlen_validation_errors(lib):
    INVALID, UNSUPPORTED = -1, -2
    fa, ba, seqs = _args(lib)
    fa.mask = 1 << 32
    assert lib.fcsa_forward_varlen(C.byref(fa), C.byref(seqs)) == INVALID
    assert b"mask" in lib.fcsa_last_error()
    fa, ba, seqs = _args(lib)
    fa.attn_bias = 1 << 32
    assert lib.fcsa_forward_varlen(C.byref(fa), C.byref(seqs)) == INVALID
    ba.attn_bias = 1 << 32
    assert lib.fcsa_backward_varlen(C.byref(ba), C.byref(seqs)) == INVALID
    fa, ba, seqs = _args(lib)
    ba.d_bias = 1 << 32
    assert lib.fcsa_backward_varlen(C.byref(ba), C.byref(seqs)) == INVALID
    for field in ("cu_seqlens_q", "cu_seqlens_k"):
        fa, ba, seqs = _args(lib)
        setattr(seqs, field, None)
        assert lib.fcsa_forward_varlen(C.byref(fa), C.byref(seqs)) == INVALID
        assert lib.fcsa_backward_varlen(C.byref(ba), C.byref(seqs)) == INVALID
        assert b"cu_seqlens" in lib.fcsa_last_error()
    fa, ba, seqs = _args(lib)
    assert lib.fcsa_forward_varlen(C.byref(fa), None) == INVALID
    for field in ("total_q", "total_k"):
        fa, ba, seqs = _args(lib)
        setattr(seqs, field, -1)
        assert lib.fcsa_forward_varlen(C.byref(fa), C.byref(seqs)) == INVALID
        assert lib.fcsa_backward_varlen(C.byref(ba), C.byref(seqs)) == INVALID
    for field in ("q_len", "k_len"):          # max_seqlen_q / max_seqlen_k
        fa, ba, seqs = _args(lib)
        setattr(fa.p, field, -1)
        setattr(ba.p, field, -1)
        assert lib.fcsa_forward_varlen(C.byref(fa), C.byref(seqs)) == INVALID
        assert lib.fcsa_backward_varlen(C.byref(ba), C.byref(seqs)) == INVALID
    fa, ba, seqs = _args(lib)
    fa.p.dtype = ba.p.dtype = 7
    assert lib.fcsa_forward_varlen(C.byref(fa), C.byref(seqs)) == UNSUPPORTED
    assert lib.fcsa_backward_varlen(C.byref(ba), C.byref(seqs)) == UNSUPPORTED


def _align(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("H,Hk,groups,D", [(8, 8, 1, 64), (8, 2, 1, 64), (4, 1, 1, 128), (4, 4, 2, 96), (8, 8, 1, 32)])
def test_varlen_workspace_matches_slab_layout(lib, H, Hk, groups, D):
    """delta [1, H, total_q] f32, then the f32 slabs of the packed rows: dq and dk ([1, H, total_q or total_k, D]) where the l2norm
    backward cannot be fused (groups that are not 8 * 2^k features wide), dk / dv per query head where K/V has fewer heads.  Never a split: the
    problem below would split dQ and dK/dV as a dense [1, H, total_q / total_k] call."""
    from flash_cosine_sim_attention_amd import _lib
    TQ, TK = 4000, 300
    prob = _lib.problem(torch.bfloat16, (5, H, Hk, 900, 100, D), False, False, True, groups, 8.0)
    seqs = _lib.Varlen(None, None, TQ, TK)
    got = lib.fcsa_backward_varlen_workspace_bytes(C.byref(prob), C.byref(seqs))
    fused = (D // groups) % 8 == 0 and (groups == 1 or ((D // groups) // 8) & ((D // groups) // 8 - 1) == 0)
    slab_k = _align(H * TK * D * 4)
    want = _align(H * TQ * 4) + (0 if fused else _align(H * TQ * D * 4)) + (slab_k if (Hk != H or not fused) else 0) \
        + (slab_k if Hk != H else 0)
    assert got == want
    assert lib.fcsa_backward_varlen_workspace_bytes(C.byref(prob), None) == 0


def _oracle_packed(q, k, v, lq, lk, **kw):
    ro = np.zeros(q.shape)
    cq, ck = np.concatenate([[0], np.cumsum(lq)]), np.concatenate([[0], np.cumsum(lk)])
    G = q.shape[1] // k.shape[1]
    for s in range(len(lq)):
        if lq[s] == 0 or lk[s] == 0:
            continue
        qs = q[cq[s]:cq[s + 1]].double().numpy().transpose(1, 0, 2)[None]
        ks, vs = (np.repeat(x[ck[s]:ck[s + 1]].double().numpy().transpose(1, 0, 2)[None], G, axis=1) for x in (k, v))
        o, _ = O.attention_forward_stats(qs, ks, vs, **kw)
        ro[cq[s]:cq[s + 1]] = o[0].transpose(1, 0, 2)
    return ro


@pytest.mark.parametrize("lq,lk,Hk,kw", [
    ([0, 1, 129, 70, 3], None, 2, dict(causal=True)),
    ([40, 0, 90], [60, 12, 0], 2, dict()),
    ([200, 5], [100, 30], 1, dict(causal=True, groups=2, scale=4.0)),
    ([50, 7], [51, 8], 4, dict(l2norm_qk=False, scale=1.0)),
])
def test_varlen_cpu_forward_matches_oracle_per_sequence(lq, lk, Hk, kw):
    import flash_cosine_sim_attention_amd as F
    lk = lq if lk is None else lk
    g = torch.Generator().manual_seed(4)
    H, D = 4, 32
    q, k, v = torch.randn(sum(lq), H, D, generator=g), torch.randn(sum(lk), Hk, D, generator=g), torch.randn(sum(lk), Hk, D, generator=g)
    if not kw.get("l2norm_qk", True):
        q, k = torch.nn.functional.normalize(q, dim=-1), torch.nn.functional.normalize(k, dim=-1)
    cu = lambda ls: torch.tensor(np.concatenate([[0], np.cumsum(ls)]), dtype=torch.int32)
    o = F.flash_cosine_sim_attention_varlen(q, k, v, cu(lq), cu(lk), **kw)
    assert o.shape == q.shape and o.dtype == q.dtype
    np.testing.assert_allclose(o.double().numpy(), _oracle_packed(q, k, v, lq, lk, **kw), atol=2e-5, rtol=1e-4)
    # the same rows as one dense CPU call per sequence
    cq = np.concatenate([[0], np.cumsum(lq)])
    ck = np.concatenate([[0], np.cumsum(lk)])
    for s in range(len(lq)):
        if lq[s] == 0:
            continue
        dense = F.flash_cosine_sim_attention(q[cq[s]:cq[s + 1]].permute(1, 0, 2)[None], k[ck[s]:ck[s + 1]].permute(1, 0, 2)[None],
                                             v[ck[s]:ck[s + 1]].permute(1, 0, 2)[None], **kw)
        assert torch.equal(o[cq[s]:cq[s + 1]], dense[0].permute(1, 0, 2))


def test_varlen_python_validation():
    import flash_cosine_sim_attention_amd as F
    q = torch.randn(9, 2, 32)
    good = torch.tensor([0, 4, 9], dtype=torch.int32)
    with pytest.raises(ValueError, match="start at 0"):
        F.flash_cosine_sim_attention_varlen(q, q, q, torch.tensor([1, 4, 9], dtype=torch.int32), good)
    with pytest.raises(ValueError, match="non-decreasing"):
        F.flash_cosine_sim_attention_varlen(q, q, q, good, torch.tensor([0, 10, 9], dtype=torch.int32))
    with pytest.raises(ValueError, match="longer than max_seqlen"):
        F.flash_cosine_sim_attention_varlen(q, q, q, good, good, max_seqlen_k=4)
    with pytest.raises(TypeError, match="int32"):
        F.flash_cosine_sim_attention_varlen(q, q, q, good.long(), good)
    with pytest.raises(ValueError, match="same length"):
        F.flash_cosine_sim_attention_varlen(q, q, q, good, torch.tensor([0, 9], dtype=torch.int32))
    with pytest.raises(ValueError, match="packed"):
        F.flash_cosine_sim_attention_varlen(q[None], q, q, good, good)
    with pytest.raises(RuntimeError, match="forward-only"):
        F.flash_cosine_sim_attention_varlen(q.clone().requires_grad_(), q, q, good, good)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_varlen_span_clamp_early_exit_and_forms(tmp_path):
    """tests/native/varlen_span_check.cpp: spans stay inside [0, total) for any table, well-formed tables are reproduced, the early-exit
    rule runs every (sequence, tile) once over the max-sized grid, and no packed problem gets Fwd2 / Fwd3 / the group sweep"""
    exe = str(tmp_path / "varlen_span_check")
    b = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "flash_cosine_sim_attention_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "varlen_span_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]
