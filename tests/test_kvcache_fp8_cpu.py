"""An fp8 (e4m3fn) key/value cache without a GPU: the quantising append of the CPU path byte for byte, CPU attention on codes against
the existing CPU call on float32 caches holding scale * code (exact: one code path after dequantisation), every refusal of the Python
entry point, and the C ABI of fcsa_forward_kvcache_quant -- struct layout against gcc, exported symbols, argument checks with fake
pointers (never dereferenced) and the workspace formula."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import flash_cosine_sim_attention_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
kv = F.flash_cosine_sim_attention_with_kvcache
E4M3 = torch.float8_e4m3fn


def _rule(x, s):
    """the append rule, as the issue states it"""
    return (x.float() / s).clamp(-448, 448).to(E4M3).view(torch.uint8)


def _scale4(s, B, Hk):
    """a scale argument (float, [], [Hk], [B, Hk]) as [B, Hk, 1, 1] float32"""
    t = s if isinstance(s, torch.Tensor) else torch.tensor(float(s))
    return t.float().expand(B, Hk)[:, :, None, None]


def _special_rows(dtype, s, D):
    """values whose quotient by s lands beyond +-448, on rounding ties (between adjacent codes, normal and subnormal), in the subnormal
    range, below half the smallest subnormal, and on +-0"""
    codes = torch.arange(256, dtype=torch.uint8).view(E4M3).float()
    fin = codes[torch.isfinite(codes)]
    pos = torch.sort(fin[fin >= 0]).values
    ties = (pos[:-1] + pos[1:]) / 2                                  # exact midpoints of neighbouring codes (subnormals included)
    vals = torch.cat([torch.tensor([0.0, -0.0, 449.0, 1e4, -1e4, 464.0, -464.0, 2.0 ** -9, 2.0 ** -10, 2.0 ** -11, 3 * 2.0 ** -11,
                                    -(2.0 ** -10), 1e-8, -1e-8]), ties, -ties, pos, -pos])
    x = (vals * s).to(dtype)
    n = (x.numel() + D - 1) // D * D
    return torch.cat([x, torch.zeros(n - x.numel(), dtype=dtype)]).view(-1, D)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("s", [1.0, 0.37, 2.0 ** -4])
def test_append_rule_bytes_guards_and_capacity(dtype, s):
    B, Hk, D, cap = 2, 2, 16, 96
    rows = _special_rows(dtype, s, D)
    n_new = rows.shape[0] // (B * Hk)
    kn = rows[:B * Hk * n_new].view(B, Hk, n_new, D).clone()
    vn = kn.flip(2).clone()
    g = torch.Generator().manual_seed(1)
    # guard values around the caches: one arena, the caches a window inside it
    arena = torch.randint(0, 256, (2, 64 + B * Hk * cap * D + 64), dtype=torch.uint8, generator=g)
    arena0 = arena.clone()
    kc = arena[0, 64:-64].view(B, Hk, cap, D).view(E4M3)
    vc = arena[1, 64:-64].view(B, Hk, cap, D).view(E4M3)
    seq = [3, cap - n_new + 2]                                      # the second sequence runs 2 slots past the capacity: dropped
    ks, vs = torch.tensor([[s, 2 * s], [s / 2, s]]), torch.tensor(s)
    q = torch.zeros(B, 2, 1, D, dtype=dtype)
    # (host lengths are validated against the capacity by the entry point, so the overflowing append goes through the CPU module)
    from flash_cosine_sim_attention_amd import cpu
    cpu.attention_forward_kvcache_cpu(q, kc, vc, kn, vn, seq, k_scale=ks, v_scale=vs.expand(B, Hk))
    exp = arena0.clone()
    ek, ev = exp[0, 64:-64].view(B, Hk, cap, D), exp[1, 64:-64].view(B, Hk, cap, D)
    for b, st in enumerate(seq):
        m = min(n_new, cap - st)
        ek[b, :, st:st + m] = _rule(kn[b, :, :m], ks[b][:, None, None])
        ev[b, :, st:st + m] = _rule(vn[b, :, :m], vs)
    assert torch.equal(arena, exp)
    assert torch.equal(arena[:, :64], arena0[:, :64]) and torch.equal(arena[:, -64:], arena0[:, -64:])
    # the rule itself: saturation at +-448 (0x7e / 0xfe), never NaN for a finite input; NaN stays NaN
    assert _rule(torch.tensor([1e4, -1e4, 449.0]).to(dtype), 1.0).tolist() == [0x7e, 0xfe, 0x7e]
    nan = cpu.quantise_e4m3(torch.tensor([float("nan")], dtype=dtype), torch.tensor(s)).view(torch.uint8)
    assert int(nan[0]) & 0x7f == 0x7f


def test_append_through_the_entry_point():
    B, H, Hk, N, D, cap = 2, 4, 2, 3, 32, 40
    g = torch.Generator().manual_seed(2)
    kn, vn = torch.randn(B, Hk, N, D, generator=g).bfloat16() * 3, torch.randn(B, Hk, N, D, generator=g).bfloat16() * 600
    kc = torch.zeros(B, Hk, cap, D).to(E4M3)
    vc = torch.zeros(B, Hk, cap, D).to(E4M3)
    q = torch.randn(B, H, N, D, generator=g).bfloat16()
    sl = torch.tensor([0, cap - N], dtype=torch.int32)
    ks, vs = torch.tensor([0.5, 0.01]), 1.25
    kv(q, kc, vc, kn, vn, sl, k_scale=ks, v_scale=vs)
    assert sl.tolist() == [0, cap - N]
    for b, st in enumerate(sl.tolist()):
        assert torch.equal(kc.view(torch.uint8)[b, :, st:st + N], _rule(kn[b], ks[:, None, None]))
        assert torch.equal(vc.view(torch.uint8)[b, :, st:st + N], _rule(vn[b], vs))
    assert int((vc.view(torch.uint8) & 0x7f).max()) == 0x7e          # 600 * randn / 1.25 saturates somewhere, and never becomes NaN


def _codes(shape, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    c[(c & 0x7f) == 0x7f] = 0x3c                                     # no NaN codes in the valid part
    return c.view(E4M3)


SCALES = [("float", lambda B, Hk: (0.37, 1.5)),
          ("hk", lambda B, Hk: (torch.linspace(0.1, 0.9, Hk), torch.linspace(2.0, 0.5, Hk))),
          ("b_hk", lambda B, Hk: (torch.linspace(0.05, 1.1, B * Hk).view(B, Hk), torch.linspace(3.0, 0.25, B * Hk).view(B, Hk))),
          ("none", lambda B, Hk: (None, None))]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("sname,mk", SCALES, ids=[s[0] for s in SCALES])
@pytest.mark.parametrize("kw", [dict(), dict(causal=True), dict(causal=True, window_size=(9, 0)), dict(window_size=(4, 2), l2norm_qk=False, scale=0.05)],
                         ids=["full", "causal", "window_causal", "window_no_l2norm"])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_cpu_attention_equals_float32_caches(dtype, sname, mk, kw, paged):
    B, H, Hk, N, D, page, mb = 3, 4, 2, 2, 32, 16, 3
    cap = page * mb
    ks, vs = mk(B, Hk)
    q = torch.randn(B, H, N, D, generator=torch.Generator().manual_seed(5)).to(dtype)
    seq = [0, 17, cap - N]
    kn = torch.randn(B, Hk, N, D, generator=torch.Generator().manual_seed(6)).to(dtype)
    vn = torch.randn(B, Hk, N, D, generator=torch.Generator().manual_seed(7)).to(dtype)
    sl = torch.tensor(seq, dtype=torch.int32)
    ks4 = _scale4(1.0 if ks is None else ks, B, Hk)
    vs4 = _scale4(1.0 if vs is None else vs, B, Hk)
    if not paged:
        kc, vc = _codes((B, Hk, cap, D), 8), _codes((B, Hk, cap, D), 9)
        o = kv(q, kc, vc, kn, vn, sl, k_scale=ks, v_scale=vs, **kw)
        k32, v32 = kc.float() * ks4, vc.float() * vs4                 # after the append: the caches as the call left them
        ref = kv(q.float(), k32, v32, None, None, torch.tensor([s + N for s in seq], dtype=torch.int32), **kw)
    else:
        nb = B * mb + 2
        table = torch.randperm(nb, generator=torch.Generator().manual_seed(3))[:B * mb].reshape(B, mb).to(torch.int32)
        # the vLLM layout [num_blocks, page, Hk, D], passed transposed
        kc, vc = _codes((nb, page, Hk, D), 8).transpose(1, 2), _codes((nb, page, Hk, D), 9).transpose(1, 2)
        o = kv(q, kc, vc, kn, vn, sl, block_table=table, k_scale=ks, v_scale=vs, **kw)
        k32, v32 = torch.zeros(nb, Hk, page, D), torch.zeros(nb, Hk, page, D)
        for b in range(B):                                           # every block belongs to one sequence: its scale
            for i in range(mb):
                blk = int(table[b, i])
                k32[blk], v32[blk] = kc[blk].float() * ks4[b], vc[blk].float() * vs4[b]
        ref = kv(q.float(), k32, v32, None, None, torch.tensor([s + N for s in seq], dtype=torch.int32), block_table=table, **kw)
    assert o.dtype == dtype and torch.equal(o, ref.to(dtype))
    assert torch.isfinite(o).all() and (o[1:].float().abs().sum() > 0)


def test_refusals_name_the_problem():
    B, H, Hk, N, D, cap = 1, 2, 2, 1, 16, 32
    q = torch.zeros(B, H, N, D, dtype=torch.bfloat16)
    c8 = torch.zeros(B, Hk, cap, D).to(E4M3)
    c16 = torch.zeros(B, Hk, cap, D, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="one fp8 cache and one"):
        kv(q, c8, c16, cache_seqlens=4)
    with pytest.raises(TypeError, match="one fp8 cache and one"):
        kv(q, c16, c8, cache_seqlens=4)
    for bad in (torch.float8_e4m3fnuz, torch.float8_e5m2):
        with pytest.raises(TypeError, match="not supported"):
            kv(q, c16.to(bad), c16.to(bad), cache_seqlens=4)
    for kw in (dict(k_scale=0.5), dict(v_scale=torch.tensor(0.5)), dict(k_scale=1.0, v_scale=1.0)):
        with pytest.raises(TypeError, match="scales belong to"):
            kv(q, c16, c16, cache_seqlens=4, **kw)
    with pytest.raises(TypeError, match="float16 or bfloat16"):
        kv(q.float(), c8, c8, cache_seqlens=4)
    # the scales themselves
    for bad in (0.0, -1.0, float("inf"), float("nan"), torch.tensor([1.0, 0.0]), torch.tensor([float("nan"), 1.0])):
        with pytest.raises(ValueError, match="finite and > 0"):
            kv(q, c8, c8, cache_seqlens=4, k_scale=bad)
        with pytest.raises(ValueError, match="finite and > 0"):
            kv(q, c8, c8, cache_seqlens=4, v_scale=bad)
    for bad in (torch.ones(3), torch.ones(2, 2), torch.ones(2, dtype=torch.float64), "1.0"):
        with pytest.raises(TypeError, match="k_scale"):
            kv(q, c8, c8, cache_seqlens=4, k_scale=bad)
    with pytest.raises(TypeError, match="k_new must have q's dtype"):
        kv(q, c8, c8, torch.zeros(B, Hk, 1, D), torch.zeros(B, Hk, 1, D), cache_seqlens=4)
    # and what is accepted
    assert kv(q, c8, c8, cache_seqlens=4, k_scale=torch.ones(Hk), v_scale=torch.ones(B, Hk)).shape == q.shape


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


def _args(prob):
    from flash_cosine_sim_attention_amd import _lib
    t = _lib.Tensor(0x1000, 1024, 512, 64)            # fake, never dereferenced: validation fails first
    return _lib.ForwardArgs(prob, t, t, t, t, None, None, None, _lib.NormState(None, None, None, None), None, 0, None)


def _cache(**kw):
    from flash_cosine_sim_attention_amd import _lib
    t = _lib.Tensor(0x10000, 4096 * 256, 4096 * 128, 128)      # one-byte elements: [B, Hk, 4096, 128]
    d = dict(k_cache=t, v_cache=t, capacity=4096, page_size=0, num_blocks=0, new_len=0, cache_seqlens=None, block_table=None,
             block_table_stride=0, k_new=_lib.Tensor(0, 0, 0, 0), v_new=_lib.Tensor(0, 0, 0, 0))
    d.update(kw)
    return _lib.KvCache(*[d[f[0]] for f in _lib.KvCache._fields_])


def _quant(**kw):
    from flash_cosine_sim_attention_amd import _lib
    d = dict(cache_dtype=_lib.FCSA_CACHE_E4M3, k_scale=0x20000, v_scale=0x20100, k_scale_stride0=2, k_scale_stride1=1, v_scale_stride0=0,
             v_scale_stride1=0)
    d.update(kw)
    return _lib.KvCacheQuant(*[d[f[0]] for f in _lib.KvCacheQuant._fields_])


def test_struct_layout_matches_c_compiler(tmp_path):
    from flash_cosine_sim_attention_amd import _lib
    prog = tmp_path / "layout.c"
    fields = [f[0] for f in _lib.KvCacheQuant._fields_]
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fcsa.h\"\nint main(void) {\n"
                    "  printf(\"%zu\\n\", sizeof(fcsa_kvcache_quant));\n"
                    + "".join(f"  printf(\"%zu\\n\", offsetof(fcsa_kvcache_quant, {f}));\n" for f in fields)
                    + "  printf(\"%d\\n\", FCSA_CACHE_E4M3);\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert out[0] == C.sizeof(_lib.KvCacheQuant)
    assert out[1:-1] == [getattr(_lib.KvCacheQuant, f).offset for f in fields]
    assert out[-1] == _lib.FCSA_CACHE_E4M3
    assert fields == ["cache_dtype", "k_scale", "v_scale", "k_scale_stride0", "k_scale_stride1", "v_scale_stride0", "v_scale_stride1"]


def test_exports_and_abi_version(lib):
    from flash_cosine_sim_attention_amd import _lib
    for sym in ("fcsa_forward_kvcache_quant", "fcsa_forward_kvcache_quant_workspace_bytes"):
        assert sym in _lib.EXPORTS and hasattr(lib, sym)
    assert _lib.ABI_VERSION == 4 and lib.fcsa_debug(None, 0) == 4
    buf = C.create_string_buffer(2048)
    lib.fcsa_debug(buf, 2048)
    for name in (b"kv_append_fp8", b"decode_fp8", b"decode_combine_fp8"):
        assert name in buf.value


def test_cabi_argument_checks(lib):
    from flash_cosine_sim_attention_amd import _lib
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
    call = lambda a, c, z, w=None: lib.fcsa_forward_kvcache_quant(None if a is None else C.byref(a), None if c is None else C.byref(c),
                                                                  None if z is None else C.byref(z), None if w is None else C.byref(w))
    assert call(_args(_problem()), _cache(), None) == INVALID and b"null" in lib.fcsa_last_error()
    assert call(_args(_problem()), None, _quant()) == INVALID
    assert call(None, _cache(), _quant()) == INVALID
    for t in (0, 2, -1):
        assert call(_args(_problem()), _cache(), _quant(cache_dtype=t)) == UNSUPPORTED and b"cache type" in lib.fcsa_last_error()
    assert call(_args(_problem(dtype=_lib.FCSA_F32)), _cache(), _quant()) == UNSUPPORTED and b"float32" in lib.fcsa_last_error()
    assert call(_args(_problem()), _cache(), _quant(k_scale=None)) == INVALID and b"scale" in lib.fcsa_last_error()
    assert call(_args(_problem()), _cache(), _quant(v_scale=None)) == INVALID and b"scale" in lib.fcsa_last_error()
    # the checks of the 16-bit call still hold, with one-byte cache elements: rows 16 BYTES apart are fine, 8 are not
    assert call(_args(_problem(dim_head=16)), _cache(k_cache=_lib.Tensor(0x10000, 4096 * 32, 4096 * 16, 16)), _quant()) == WORKSPACE
    assert call(_args(_problem(dim_head=16)), _cache(k_cache=_lib.Tensor(0x10000, 4096 * 32, 4096 * 16, 24)), _quant()) == INVALID
    assert call(_args(_problem()), _cache(page_size=16), _quant()) == INVALID and b"block_table" in lib.fcsa_last_error()
    assert call(_args(_problem()), _cache(new_len=2), _quant()) == INVALID and b"k_new" in lib.fcsa_last_error()
    assert call(_args(_problem(dim_head=48)), _cache(), _quant()) == UNSUPPORTED
    assert call(_args(_problem()), _cache(), _quant(), _lib.Window(-2, 0)) == INVALID
    for groups in (2, 4, 8, 16, 32):             # the straddling D = 96 widths are accepted
        assert call(_args(_problem(dim_head=96, groups=groups)), _cache(), _quant()) == WORKSPACE, groups
    for dt in (_lib.FCSA_BF16, _lib.FCSA_F16):   # valid, but no workspace -- un-windowed and windowed
        assert call(_args(_problem(dtype=dt)), _cache(), _quant()) == WORKSPACE and b"workspace" in lib.fcsa_last_error()
        assert call(_args(_problem(dtype=dt)), _cache(), _quant(), _lib.Window(100, 0)) == WORKSPACE
    assert call(_args(_problem(batch=0)), _cache(), _quant()) == 0


def test_workspace_formula_is_the_16bit_calls(lib):
    """decode_splits counts keys, so an fp8 call splits -- and sizes its workspace -- as the 16-bit call on the same problem does."""
    from flash_cosine_sim_attention_amd import _lib
    al = lambda x: (x + 255) // 256 * 256
    expect = lambda B, H, N, D, s: al(B * H * N * s * D * 4) + al(B * H * N * s * 8)
    def both(B, H, Hk, N, D, cap, win=None):
        p, c, z = _problem(batch=B, heads=H, kv_heads=Hk, q_len=N, k_len=cap, dim_head=D), _cache(capacity=cap), _quant()
        w = None if win is None else C.byref(_lib.Window(*win))
        q8 = lib.fcsa_forward_kvcache_quant_workspace_bytes(C.byref(p), C.byref(c), C.byref(z), w)
        b16 = (lib.fcsa_forward_kvcache_workspace_bytes(C.byref(p), C.byref(c)) if win is None
               else lib.fcsa_forward_kvcache_window_workspace_bytes(C.byref(p), C.byref(c), w))
        assert q8 == b16, (B, H, Hk, N, D, cap, win)
        return q8
    assert both(1, 1, 1, 1, 128, 5 * 128) == expect(1, 1, 1, 128, 5)
    assert both(1, 4, 1, 4, 16, 3 * 1024 + 7) == expect(1, 4, 4, 16, 3)
    assert both(1024, 8, 8, 1, 128, 1 << 20) == expect(1024, 8, 1, 128, 1)
    assert both(1, 2, 1, 3, 32, 1 << 22) == expect(1, 2, 3, 32, 128)
    assert both(1, 1, 1, 1, 128, 1 << 20, win=(255, 0)) == expect(1, 1, 1, 128, 2)      # 256 + 31 keys a sequence can read: two splits
    both(3, 8, 2, 3, 96, 30000)
    both(3, 8, 2, 3, 64, 30000, win=(1000, 0))
    assert lib.fcsa_forward_kvcache_quant_workspace_bytes(None, None, None, None) == 0
