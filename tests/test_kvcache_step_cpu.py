"""flash_cosine_sim_attention_step_with_kvcache without a GPU: its signature is the ragged call's plus the two routing keywords, CPU tensors
give exactly what the ragged CPU path gives for every chunk_rows (contiguous and paged caches, append, causal, return_lse, an fp8 cache, a
window), bad routing keywords and everything the ragged call refuses are refused, the op lives in a namespace of its own with a pinned
schema and no Autograd kernel, and the C ABI exports, declares and lays out the new entry points and struct as the header says."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

import flash_cosine_sim_attention_amd as F
from flash_cosine_sim_attention_amd import _lib, _torch_ops
from test_kvcache_prefill_cpu import _problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
step = F.flash_cosine_sim_attention_step_with_kvcache
ragged = F.flash_cosine_sim_attention_varlen_with_kvcache
STEP_NAME, RAGGED_NAME = "flash_cosine_sim_attention_step_with_kvcache", "flash_cosine_sim_attention_varlen_with_kvcache"

SCHEMA = ("fcsa_step::kvcache_step_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cu_seqlens_q, Tensor? k_new, Tensor? v_new, "
          "Tensor? cache_seqlens, Tensor? block_table, Tensor? k_scale, Tensor? v_scale, int max_seqlen_q, int max_seqlen_k, float scale, "
          "bool causal, bool l2norm_qk, int groups, int window_left, int window_right, int chunk_rows, int max_decode_tokens, bool no_decode, "
          "bool no_chunk) -> (Tensor, Tensor)")


def test_signature_is_the_ragged_calls_plus_the_routing_keywords():
    mine, theirs = inspect.signature(step).parameters, inspect.signature(ragged).parameters
    assert list(mine) == list(theirs) + ["chunk_rows", "max_decode_tokens"]
    assert all(mine[n] == theirs[n] for n in theirs)
    assert mine["chunk_rows"].default is None and mine["max_decode_tokens"].default is None
    assert STEP_NAME in F.__all__
    doc = " ".join(step.__doc__.split())
    # what it is for, the two single-kernel calls, the routing rule
    assert "continuous-batching engine" in doc and RAGGED_NAME in doc and "flash_cosine_sim_attention_prefill_with_kvcache" in doc
    assert "iff G * N_b >= chunk_rows" in doc


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


COUNTS, CACHED = [1, 0, 5, 40], [0, 17, 30, 3]


@pytest.mark.parametrize("chunk_rows", [None, 0, 7, 10 ** 9])
@pytest.mark.parametrize("form", ["plain", "fp8", "window"])
@pytest.mark.parametrize("page,append,causal", [(0, True, False), (16, True, True), (0, False, True), (16, False, False)])
def test_cpu_tensors_take_the_ragged_cpu_path(page, append, causal, form, chunk_rows):
    """same arguments through both functions: o, lse and the caches afterwards are equal bit for bit, whatever chunk_rows says"""
    q, kc, vc, cu, kn, vn, lens, table = _problem(torch.bfloat16, 64, 6, 2, COUNTS, CACHED, 64, page, 3)
    kw = dict(cache_seqlens=lens, block_table=table, scale=6, groups=2, causal=causal)
    if form == "fp8":
        kc, vc = (kc.float() * 40).to(torch.float8_e4m3fn), (vc.float() * 40).to(torch.float8_e4m3fn)
        kw.update(k_scale=torch.tensor([0.02, 0.03]), v_scale=0.025)
    if form == "window":
        kw.update(window_size=(9, -1 if causal else 2))
    outs = []
    for fn, extra in ((step, dict(chunk_rows=chunk_rows, max_decode_tokens=3)), (ragged, {})):
        k1, v1 = kc.clone(), vc.clone()
        with torch.no_grad():
            o, lse = fn(q, k1, v1, cu, kn if append else None, vn if append else None, return_lse=True, **kw, **extra)
            o2 = fn(q, k1.clone(), v1.clone(), cu, kn if append else None, vn if append else None, **kw, **extra)
        outs.append((o, lse, k1, v1, o2))
    for a, b in zip(*outs):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))
    o, lse = outs[0][0], outs[0][1]
    assert lse.dtype == torch.float32 and lse.shape == (q.shape[0], q.shape[1])
    if append:
        assert not torch.equal(_bits(outs[0][2]), _bits(kc))      # the append landed in the cache it was given
    if causal and not append and form != "window":      # 40 tokens against 3 cached positions: rows without a visible key
        assert torch.isneginf(lse[6:6 + 37]).all() and (o[6:6 + 37] == 0).all()


def _args(dtype=torch.bfloat16, D=64):
    q, kc, vc, cu, kn, vn, lens, table = _problem(torch.float32, D, 4, 2, [3, 2], [5, 0], 16, 0, 1)
    return (q.to(dtype), kc.to(dtype), vc.to(dtype), cu, kn.to(dtype), vn.to(dtype)), dict(cache_seqlens=lens)


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 64), (torch.float32, 64), (torch.bfloat16, 96)])
def test_bad_routing_keywords_are_refused(dtype, D):
    """type- and range-checked also where there is no chunk kernel (float32, D = 96) and the values are otherwise ignored"""
    a, kw = _args(dtype, D)
    with torch.no_grad():
        for name in ("chunk_rows", "max_decode_tokens"):
            with pytest.raises(ValueError, match=f"{name} must be None or a non-negative integer, got -1"):
                step(*a, **kw, **{name: -1})
            for bad in (1.5, "x", True, torch.tensor(3)):
                with pytest.raises(TypeError, match=f"{name} must be None or a non-negative integer"):
                    step(*a, **kw, **{name: bad})
        for good in (0, 1, 10 ** 12):
            assert step(*a, **kw, chunk_rows=good, max_decode_tokens=good).shape == a[0].shape


def _refusal(fn, *a, **kw):
    with pytest.raises(Exception) as e:
        fn(*a, **kw)
    return type(e.value), str(e.value)


def test_what_the_ragged_call_refuses_is_refused_with_its_message():
    a, kw = _args()
    q, kc, vc, cu, kn, vn = a
    bad_calls = [
        ((q[0], kc, vc, cu, kn, vn), kw),                                                          # q's rank
        ((q, kc, vc[:, :, :8], cu, kn, vn), kw),                                                   # cache shapes
        ((q, kc, vc, cu.long(), kn, vn), kw),                                                      # the table's type
        ((q, kc, vc, torch.tensor([0, 4, 3], dtype=torch.int32), kn, vn), kw),                     # a host table that does not end at total_q
        ((q, kc, vc, cu, kn[:4], vn[:4]), kw),                                                     # the packed new rows
        ((q, kc, vc, cu, kn, None), kw),
        ((q, kc, vc, cu, kn, vn), dict(cache_seqlens=torch.tensor([15, 0], dtype=torch.int32))),   # beyond the capacity
        ((q, kc, vc, cu, kn, vn), dict(cache_seqlens=None)),                                       # nothing to append to
        ((q, kc, vc, cu, kn, vn), dict(kw, max_seqlen_q=-1)),
        ((q, kc, vc, cu, kn, vn), dict(kw, max_seqlen_k=1.5)),
        ((q, kc, vc, cu, kn, vn), dict(kw, return_lse=1)),
        ((q, kc, vc, cu, kn, vn), dict(kw, window_size=(1, 2, 3))),
        ((q, kc, vc, cu, kn, vn), dict(kw, k_scale=1.0)),                                          # scales without fp8 caches
        ((q, kc.to(torch.float8_e4m3fn), vc, cu, kn, vn), kw),                                     # one fp8 cache
        ((q.float(), kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn), cu, kn.float(), vn.float()), kw),      # float32 against fp8
        ((q, kc[:, :1].expand(-1, 3, -1, -1), vc[:, :1].expand(-1, 3, -1, -1), cu, kn, vn), kw),   # K/V heads that do not divide
    ]
    with torch.no_grad():
        for args, kwargs in bad_calls:
            kind, text = _refusal(ragged, *args, **kwargs)
            assert _refusal(step, *args, **kwargs) == (kind, text.replace(RAGGED_NAME, STEP_NAME)), (text,)
    # gradients
    kind, text = _refusal(ragged, q.clone().requires_grad_(), kc, vc, cu, kn, vn, **kw)
    assert kind is RuntimeError and "forward-only" in text
    assert _refusal(step, q.clone().requires_grad_(), kc, vc, cu, kn, vn, **kw) == (kind, text.replace(RAGGED_NAME, STEP_NAME))
    assert _refusal(step, q, kc, vc, cu, kn.clone().requires_grad_(), vn, **kw)[0] is RuntimeError


def test_the_op_has_its_own_namespace_a_pinned_schema_and_no_autograd_kernel():
    _torch_ops.load()
    names = {n for n in torch._C._dispatch_get_all_op_names() if n.startswith("fcsa_step::")}
    assert {n.split(".")[0] for n in names} == {"fcsa_step::kvcache_step_forward"}
    op = torch.ops.fcsa_step.kvcache_step_forward
    assert op.overloads() == ["default"]
    assert str(op.default._schema) == SCHEMA
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("fcsa_step::kvcache_step_forward", "Autograd")
    assert torch._C._dispatch_has_kernel_for_dispatch_key("fcsa_step::kvcache_step_forward", "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("fcsa_step::kvcache_step_forward", "CPU")
    others = torch._C._dispatch_get_all_op_names()
    assert not any(n.startswith(("fcsa::kvcache_step", "fcsa_prefill::kvcache_step")) for n in others)


def test_fake_kernel_gives_the_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    _torch_ops.load()
    with FakeTensorMode():
        q = torch.empty(7, 8, 128, dtype=torch.float16)
        kc = torch.empty(2, 2, 64, 128, dtype=torch.uint8)
        cu = torch.empty(3, dtype=torch.int32)
        s = torch.empty(2, 2)
        o, lse = torch.ops.fcsa_step.kvcache_step_forward(q, kc, kc.clone(), cu, None, None, None, None, s, s, 7, 64, 8.0, True, True, 1, 40, -1,
                                                          512, -1, False, False)
    assert o.shape == (7, 8, 128) and o.dtype == torch.float16 and lse.shape == (7, 8) and lse.dtype == torch.float32


def test_c_abi_exports_and_declares_the_entry_points():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fcsa.h")).read()
    for sym in ("fcsa_forward_kvcache_step", "fcsa_forward_kvcache_step_workspace_bytes"):
        assert sym in _lib.EXPORTS and hasattr(lib, sym)
        assert re.search(r"^(int|size_t)\s+" + sym + r"\(", header, flags=re.M), sym
    assert lib.fcsa_debug(None, 0) == 4 == _lib.ABI_VERSION      # additive: the ABI version stays
    assert _lib.STEP_CHUNK_ROWS > 0 and f"#define FCSA_STEP_CHUNK_ROWS {_lib.STEP_CHUNK_ROWS}" in header
    # null arguments: refused with a message; the workspace query answers 0
    assert lib.fcsa_forward_kvcache_step(None, None, None, None, None, None, None) == -1
    assert b"kvcache_step: null argument" in lib.fcsa_last_error()
    fa, kv, seqs, st = _lib.ForwardArgs(), _lib.KvCache(), _lib.Varlen(), _lib.KvCacheStep()
    for args in ((None, kv, seqs, st), (fa, None, seqs, st), (fa, kv, None, st), (fa, kv, seqs, None)):
        ptr = [None if x is None else C.byref(x) for x in args]
        assert lib.fcsa_forward_kvcache_step(ptr[0], ptr[1], ptr[2], None, None, ptr[3], None) == -1
        assert b"kvcache_step: null argument" in lib.fcsa_last_error()
    assert lib.fcsa_forward_kvcache_step_workspace_bytes(None, None, None, None, None, None) == 0
    # the promises are flags
    fa.p = _lib.problem(torch.bfloat16, (2, 8, 2, 4, 64, 64), True, False, True, 1, 8.0)
    kv.capacity = 64
    seqs.total_q = 5
    seqs.cu_seqlens_q = 4096
    fa.q = fa.o = _lib.Tensor(1 << 20, 0, 64, 8 * 64)                                  # (synthetic addresses: the call is refused before any launch)
    kv.k_cache = kv.v_cache = _lib.Tensor(1 << 24, 2 * 64 * 64, 64 * 64, 64)
    bad = _lib.KvCacheStep(128, 2, -1, 0, 0)
    assert lib.fcsa_forward_kvcache_step(C.byref(fa), C.byref(kv), C.byref(seqs), None, None, C.byref(bad), None) == -1
    assert b"are flags" in lib.fcsa_last_error()
    for text in ("A promise is TRUSTED", "nothing is ever accessed out of bounds", '"step_decode[_fp8]"', '"step_prefill"', "FCSA_ABI_VERSION stays 4"):
        assert text in " ".join(header.replace("\n *", " ").split()), text


def test_workspace_is_a_function_of_shapes_and_the_bound():
    """the split count is sized by the decode-rows bound (fewer rows: more splits, so more workspace per row), total_q when there is none; the
    no_decode promise needs no workspace; float32 gets the ragged call's answer"""
    lib = _lib.load()

    def ws(dtype, bound, no_decode=0, D=128, max_k=8192):
        prob = _lib.problem(dtype, (64, 32, 8, 512, max_k, D), True, False, True, 1, 8.0)
        kv = _lib.KvCache()
        kv.capacity, kv.new_len = 8192, 1
        seqs = _lib.Varlen(None, None, 575, 0)
        st = _lib.KvCacheStep(-1, no_decode, bound, 0, 0)
        got = int(lib.fcsa_forward_kvcache_step_workspace_bytes(C.byref(prob), C.byref(kv), C.byref(seqs), None, None, C.byref(st)))
        theirs = int(lib.fcsa_forward_kvcache_varlen_workspace_bytes(C.byref(prob), C.byref(kv), C.byref(seqs), None, None))
        return got, theirs

    full, ragged_ws = ws(torch.bfloat16, -1)
    assert full == ragged_ws == ws(torch.bfloat16, 575)[0] == ws(torch.bfloat16, 10 ** 6)[0]
    assert ws(torch.bfloat16, 63)[0] > full and ws(torch.bfloat16, 63)[0] % full == 0
    assert ws(torch.bfloat16, 63, no_decode=1)[0] == 0
    assert ws(torch.bfloat16, 63, max_k=1)[0] == ws(torch.bfloat16, -1, max_k=1)[0]      # one split whatever the bound
    f32, f32_ragged = ws(torch.float32, 63)
    assert f32 == f32_ragged == ws(torch.float32, 63, no_decode=1)[0]
    d96, d96_ragged = ws(torch.bfloat16, 63, D=96)
    assert d96 == d96_ragged


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_struct_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of fcsa_kvcache_step as gcc sees include/fcsa.h == the ctypes mirror"""
    S = _lib.KvCacheStep
    fields = [n for n, _ in S._fields_]
    assert fields == ["chunk_rows", "no_decode", "max_decode_tokens", "no_chunk", "reserved"]
    lines = ['  printf("%zu\\n", sizeof(fcsa_kvcache_step));\n'] + [f'  printf("%zu\\n", offsetof(fcsa_kvcache_step, {f}));\n' for f in fields]
    prog = tmp_path / "layout.c"
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fcsa.h\"\nint main(void) {\n" + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert C.sizeof(S) == 24
