"""CPU-only checks of sliding-window attention (fcsa_forward_window / fcsa_backward_window / fcsa_forward_kvcache_window,
flash_cosine_sim_attention_local and the window_size keyword of the packed and decode functions): the symbols and the ctypes layout of
fcsa_window, the C ABI's argument validation (no kernel is launched by any call here), the host's normalisation rules, the CPU forward
path against the float64 oracle with the window as a 0 / -inf bias, and the tile-ownership functions of csrc/fcsa_dispatch.h through a
g++ program (tests/native/window_tiles_check.cpp)."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import cosine_sim_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fcsa_forward_window", "fcsa_backward_window", "fcsa_backward_window_workspace_bytes", "fcsa_forward_kvcache_window",
           "fcsa_forward_kvcache_window_workspace_bytes")
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from flash_cosine_sim_attention_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def band(N, M, left, right, causal):
    """the window as an additive bias [1, N, M]: 0 inside the band, -inf outside"""
    i = np.arange(N)[:, None] + (M - N)
    j = np.arange(M)[None]
    ok = np.ones((N, M), bool)
    if left >= 0:
        ok &= j >= i - left
    r = 0 if causal else right
    if r >= 0:
        ok &= j <= i + r
    return np.where(ok, 0.0, -np.inf)[None]


def test_window_symbols_exported_and_abi_version_unchanged(lib):
    from flash_cosine_sim_attention_amd import _lib
    for n in SYMBOLS:
        assert n in _lib.EXPORTS and hasattr(lib, n)
    assert lib.fcsa_debug(None, 0) == 4 and _lib.ABI_VERSION == 4
    buf = C.create_string_buffer(2048)
    lib.fcsa_debug(buf, 2048)
    assert b"window(" in buf.value


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_window_struct_layout_matches_c_compiler(tmp_path):
    from flash_cosine_sim_attention_amd import _lib
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fcsa.h"\nint main(void) {\n'
                    '  printf("%zu %zu %zu\\n", sizeof(fcsa_window), offsetof(fcsa_window, left), offsetof(fcsa_window, right));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    Wn = _lib.Window
    assert got == [C.sizeof(Wn), Wn.left.offset, Wn.right.offset] == [8, 0, 4]


def _args(dtype=torch.bfloat16, B=2, H=2, Hk=2, N=300, M=300, D=64, causal=False):
    """argument blocks with fake (never dereferenced) device addresses: validation runs before any launch"""
    from flash_cosine_sim_attention_amd import _lib
    prob = _lib.problem(dtype, (B, H, Hk, N, M, D), causal, False, True, 1, 8.0)
    fake = 1 << 32
    t = lambda: _lib.Tensor(fake, H * N * D, N * D, D)
    norm = _lib.NormState(fake, fake, fake, fake)
    fa = _lib.ForwardArgs(prob, t(), t(), t(), t(), fake, None, None, norm, None, 0, None)
    ba = _lib.BackwardArgs(prob, t(), t(), fake, t(), t(), t(), None, None, norm, t(), t(), t(), None, fake, 1 << 30, None)
    return fa, ba


def test_window_validation_errors(lib):
    from flash_cosine_sim_attention_amd import _lib
    for bad in ((-2, 0), (0, -2), (-5, -5)):
        fa, ba = _args()
        w = _lib.Window(*bad)
        assert lib.fcsa_forward_window(C.byref(fa), None, C.byref(w)) == INVALID
        assert b"window" in lib.fcsa_last_error()
        assert lib.fcsa_backward_window(C.byref(ba), None, C.byref(w)) == INVALID
    w = _lib.Window(10, 0)
    fa, ba = _args()
    assert lib.fcsa_forward_window(C.byref(fa), None, None) == INVALID
    assert lib.fcsa_backward_window(C.byref(ba), None, None) == INVALID
    for field in ("mask", "attn_bias"):
        fa, ba = _args()
        setattr(fa, field, 1 << 32)
        setattr(ba, field, 1 << 32)
        assert lib.fcsa_forward_window(C.byref(fa), None, C.byref(w)) == INVALID
        assert b"sliding window" in lib.fcsa_last_error()
        assert lib.fcsa_backward_window(C.byref(ba), None, C.byref(w)) == INVALID
    fa, ba = _args()
    ba.d_bias = 1 << 32
    assert lib.fcsa_backward_window(C.byref(ba), None, C.byref(w)) == INVALID
    # even a window that hides nothing refuses a mask: the restriction is the entry point's, not the kernels'
    fa, ba = _args()
    fa.mask = 1 << 32
    assert lib.fcsa_forward_window(C.byref(fa), None, C.byref(_lib.Window(-1, -1))) == INVALID
    assert lib.fcsa_backward_window_workspace_bytes(None, None, C.byref(w)) == 0


def test_window_workspace_follows_the_normalisation(lib):
    """a window that IS the un-windowed or the causal call asks for that call's backward workspace; a real window for the unsplit plan"""
    from flash_cosine_sim_attention_amd import _lib
    for causal in (False, True):
        prob = _lib.problem(torch.bfloat16, (1, 8, 8, 1024, 8192, 64), causal, False, True, 1, 8.0)      # a shape whose dQ is split
        plain = lib.fcsa_backward_workspace_bytes(C.byref(prob))
        for hidden_nothing in ((-1, -1), (8191, 1023), (9000, -1)):
            assert lib.fcsa_backward_window_workspace_bytes(C.byref(prob), None, C.byref(_lib.Window(*hidden_nothing))) == plain
        unsplit = lib.fcsa_backward_window_workspace_bytes(C.byref(prob), None, C.byref(_lib.Window(100, 0)))
        assert 0 < unsplit < plain
    causal_prob = _lib.problem(torch.bfloat16, (1, 8, 8, 1024, 8192, 64), True, False, True, 1, 8.0)
    prob = _lib.problem(torch.bfloat16, (1, 8, 8, 1024, 8192, 64), False, False, True, 1, 8.0)
    assert lib.fcsa_backward_window_workspace_bytes(C.byref(prob), None, C.byref(_lib.Window(-1, 0))) == \
        lib.fcsa_backward_workspace_bytes(C.byref(causal_prob))


def test_public_api_of_the_window():
    import flash_cosine_sim_attention_amd as F
    assert "flash_cosine_sim_attention_local" in F.__all__
    sig = inspect.signature(F.flash_cosine_sim_attention_local)
    assert list(sig.parameters) == ["q", "k", "v", "window_size", "scale", "groups", "causal", "l2norm_qk"]
    assert [sig.parameters[n].default for n in ("scale", "groups", "causal", "l2norm_qk")] == [8, 1, False, True]
    for fn in (F.flash_cosine_sim_attention_varlen, F.flash_cosine_sim_attention_with_kvcache):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "window_size" and last.default == (-1, -1)


def test_python_argument_validation():
    import flash_cosine_sim_attention_amd as F
    q, k, v = (torch.randn(1, 2, 8, 16) for _ in range(3))
    for bad in ((-2, 0), (0, -2), (1.5, 0), (0, 2.0), (True, 0), 3, (1, 2, 3), None):
        with pytest.raises(ValueError):
            F.flash_cosine_sim_attention_local(q, k, v, bad)
    with pytest.raises(ValueError):
        F.flash_cosine_sim_attention_local(q[0], k[0], v[0], (1, 1))
    cu = torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(ValueError):
        F.flash_cosine_sim_attention_varlen(torch.randn(8, 2, 16), torch.randn(8, 2, 16), torch.randn(8, 2, 16), cu, cu, window_size=(0, -3))
    with pytest.raises(ValueError):
        F.flash_cosine_sim_attention_with_kvcache(q, torch.zeros(1, 2, 32, 16), torch.zeros(1, 2, 32, 16), cache_seqlens=8, window_size=(2.5, 0))
    with pytest.raises(RuntimeError):
        F.flash_cosine_sim_attention_local(q.clone().requires_grad_(), k, v, (1, 1))      # the CPU path is forward-only
    from flash_cosine_sim_attention_amd import cpu
    with pytest.raises(ValueError):
        cpu.attention_forward_cpu(q, k, v, mask=torch.ones(1, 8, dtype=torch.bool), window_size=(1, 1))
    with pytest.raises(ValueError):
        cpu.attention_forward_cpu(q, k, v, attn_bias=torch.zeros(2, 8, 8), window_size=(1, 1))
    with pytest.raises(ValueError):      # any window, as the C ABI: also one with an open left side
        cpu.attention_forward_cpu(q, k, v, mask=torch.ones(1, 8, dtype=torch.bool), window_size=(-1, 5))
    cpu.attention_forward_cpu(q, k, v, mask=torch.ones(1, 8, dtype=torch.bool), window_size=(-1, -1))
    # one rule for the sides in every entry: any integer type, no bool, no float
    assert torch.equal(F.flash_cosine_sim_attention_local(q, k, v, (np.int64(2), np.int32(1))), F.flash_cosine_sim_attention_local(q, k, v, (2, 1)))
    with pytest.raises(ValueError):
        cpu.window_sides((2.0, 1), False)


CPU_CASES = [(N, M, left, right, causal) for (N, M) in ((50, 50), (40, 90), (90, 40), (300, 300), (257, 700), (50, 20))
             for (left, right, causal) in ((0, 0, False), (1, -1, False), (31, 0, True), (64, 1, False), (-1, 5, False), (300, 200, True), (129, 64, False))]


@pytest.mark.parametrize("N,M,left,right,causal", CPU_CASES)
def test_cpu_path_matches_the_oracle(N, M, left, right, causal):
    import flash_cosine_sim_attention_amd as F
    g = torch.Generator().manual_seed(N * 1000 + M + left)
    q, k, v = torch.randn(2, 4, N, 32, generator=g), torch.randn(2, 2, M, 32, generator=g), torch.randn(2, 2, M, 32, generator=g)
    o = F.flash_cosine_sim_attention_local(q, k, v, (left, right), causal=causal, scale=6.0).double().numpy()
    rep = lambda t: np.repeat(t.double().numpy(), 2, axis=1)
    ro, _ = O.attention_forward_stats(q.double().numpy(), rep(k), rep(v), attn_bias=np.repeat(band(N, M, left, right, causal), 4, axis=0),
                                      scale=6.0, causal=causal)
    assert np.isfinite(o).all()
    assert np.abs(o - ro).max() <= 2e-5
    no_key = (band(N, M, left, right, causal)[0] == 0).sum(axis=1) == 0
    assert (o[:, :, no_key] == 0).all()
    # small row / key blocks: the band's first and last block of every row block, and the blocks between them
    from flash_cosine_sim_attention_amd import cpu
    o2 = cpu.attention_forward_cpu(q, k, v, scale=6.0, causal=causal, window_size=(left, right), row_block=32, key_block=16).double().numpy()
    assert np.abs(o2 - ro).max() <= 2e-5


def test_cpu_packed_and_decode_paths():
    import flash_cosine_sim_attention_amd as F
    g = torch.Generator().manual_seed(5)
    lq, lk = [0, 7, 130, 40], [5, 0, 100, 77]
    cu = lambda ls: torch.tensor(np.concatenate([[0], np.cumsum(ls)]), dtype=torch.int32)
    q, k, v = torch.randn(sum(lq), 2, 16, generator=g), torch.randn(sum(lk), 2, 16, generator=g), torch.randn(sum(lk), 2, 16, generator=g)
    o = F.flash_cosine_sim_attention_varlen(q, k, v, cu(lq), cu(lk), causal=True, window_size=(20, 0))
    assert torch.equal(F.flash_cosine_sim_attention_varlen(q, k, v, cu(lq), cu(lk), causal=True, window_size=(-1, -1)),
                       F.flash_cosine_sim_attention_varlen(q, k, v, cu(lq), cu(lk), causal=True))
    cq, ck = np.concatenate([[0], np.cumsum(lq)]), np.concatenate([[0], np.cumsum(lk)])
    for s in range(4):
        if not lq[s]:
            continue
        qs = q[cq[s]:cq[s + 1]].permute(1, 0, 2)[None]
        if not lk[s]:
            assert (o[cq[s]:cq[s + 1]] == 0).all()
            continue
        ks, vs = (t[ck[s]:ck[s + 1]].permute(1, 0, 2)[None] for t in (k, v))
        ref = F.flash_cosine_sim_attention_local(qs, ks, vs, (20, 0), causal=True)
        assert torch.equal(o[cq[s]:cq[s + 1]], ref[0].permute(1, 0, 2))
    # decode: the N queries are the last N cached positions
    kc, vc = torch.randn(2, 2, 64, 16, generator=g), torch.randn(2, 2, 64, 16, generator=g)
    qd = torch.randn(2, 4, 3, 16, generator=g)
    lens = torch.tensor([60, 9], dtype=torch.int32)
    od = F.flash_cosine_sim_attention_with_kvcache(qd, kc, vc, cache_seqlens=lens, causal=True, window_size=(10, 0))
    for b, L in enumerate((60, 9)):
        ref = F.flash_cosine_sim_attention_local(qd[b:b + 1], kc[b:b + 1, :, :L], vc[b:b + 1, :, :L], (10, 0), causal=True)
        assert torch.equal(od[b:b + 1], ref)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_window_tile_ownership(tmp_path):
    """skipping, not just masking (tests/native/window_tiles_check.cpp): the tiles a workgroup visits are exactly those with a visible
    pair, forward / dQ and dK/dV agree on them, the unmasked class holds fully visible tiles only, no skip test drops a visible pair"""
    exe = str(tmp_path / "window_tiles_check")
    b = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "flash_cosine_sim_attention_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "window_tiles_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("checks ok"), r.stderr[-2000:]
