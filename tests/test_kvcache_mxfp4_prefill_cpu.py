"""Prompt chunks against MXFP4 caches without a GPU: the signature and refusals of flash_cosine_sim_attention_mxfp4_prefill_with_kvcache, the
op's schema, the C entry point's declaration and refusals, and the CPU path (the MXFP4 call's, so the results are equal by definition)."""
import ctypes as C
import inspect
import os

import pytest
import torch

import flash_cosine_sim_attention_amd as F
from flash_cosine_sim_attention_amd import _lib, _torch_ops

DECODE = "flash_cosine_sim_attention_mxfp4_with_kvcache"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(H=4, Hk=2, D=64, cap=32, dt=torch.bfloat16):
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g)
    (kc, ks), (vc, vs) = F.mxfp4_quantize(rnd(2, Hk, cap, D)), F.mxfp4_quantize(rnd(2, Hk, cap, D))
    return dict(q=rnd(8, H, D).to(dt), k_cache=kc, v_cache=vc, k_block_scale=ks, v_block_scale=vs, cu_seqlens_q=torch.tensor([0, 3, 8], dtype=torch.int32),
                k_new=rnd(8, Hk, D).to(dt), v_new=rnd(8, Hk, D).to(dt), cache_seqlens=torch.tensor([7, 20], dtype=torch.int32))


REFUSALS = {      # what the decode call takes is refused by naming it
    "d32": (lambda a: {k: a[k][..., :a[k].shape[-1] // 2] for k in ("q", "k_cache", "v_cache", "k_block_scale", "v_block_scale", "k_new", "v_new")}, ValueError,
            "dim_head 64 or 128, got 32: " + DECODE),
    "d96": (lambda a: dict(q=torch.zeros(8, 4, 96, dtype=torch.bfloat16)), ValueError, "got 96: " + DECODE),
    "window_left": (lambda a: dict(window_size=(4, -1)), ValueError, "hides keys.*" + DECODE),
    "window_right": (lambda a: dict(window_size=(-1, 0)), ValueError, "hides keys.*" + DECODE),
    "f32_q": (lambda a: dict(q=a["q"].float()), TypeError, "float16 or bfloat16 q.*" + DECODE),
    "q_4d": (lambda a: dict(q=a["q"][None]), ValueError, "packed queries.*" + DECODE),
    "no_cu": (lambda a: dict(cu_seqlens_q=None), ValueError, "cu_seqlens_q=None.*" + DECODE),
    "groups": (lambda a: dict(groups=16), ValueError, "multiple of 8 features"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals(case):
    args = _args()
    change, exc, text = REFUSALS[case]
    args.update(change(args))
    with pytest.raises(exc, match=text):
        F.flash_cosine_sim_attention_mxfp4_prefill_with_kvcache(**args)


def test_signature_export_and_op():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert inspect.signature(F.flash_cosine_sim_attention_mxfp4_prefill_with_kvcache) == inspect.signature(getattr(F, DECODE))
    assert "flash_cosine_sim_attention_mxfp4_prefill_with_kvcache" in F.__all__
    _torch_ops.load()
    name, op = "fcsa_mx::kvcache_mxfp4_prefill_forward", torch.ops.fcsa_mx.kvcache_mxfp4_prefill_forward
    assert str(op.default._schema) == str(torch.ops.fcsa_mx.kvcache_mxfp4_forward.default._schema).replace("fcsa_mx::kvcache_mxfp4_forward(", name + "(")
    assert torch._C._dispatch_has_kernel_for_dispatch_key(name, "CUDA") and not torch._C._dispatch_has_kernel_for_dispatch_key(name, "Autograd")
    for want_lse in (False, True):      # the fake kernel: o like q, the lse empty unless asked for
        with FakeTensorMode():
            q, kc, ks, cu = (torch.empty(s, dtype=d) for s, d in (((8, 4, 64), torch.bfloat16), ((2, 2, 32, 32), torch.uint8), ((2, 2, 32, 2), torch.uint8),
                                                                  ((3,), torch.int32)))
            o, lse = op(q, kc, kc.clone(), ks, ks.clone(), cu, None, None, None, None, 8, 32, 8.0, True, True, 1, -1, -1, want_lse)
        assert o.shape == (8, 4, 64) and o.dtype == torch.bfloat16 and lse.shape == ((8, 4) if want_lse else (0,)) and lse.dtype == torch.float32


def test_c_abi_entry_point():
    lib = _lib.load()
    assert "fcsa_forward_kvcache_mx_prefill" in _lib.EXPORTS and hasattr(lib, "fcsa_forward_kvcache_mx_prefill")
    assert lib.fcsa_debug(None, 0) == 4      # additive: the ABI version stays
    header = " ".join(open(os.path.join(ROOT, "include", "fcsa.h")).read().split())
    assert ("int fcsa_forward_kvcache_mx_prefill(const fcsa_forward_args* args, const fcsa_kvcache* cache, const fcsa_kvcache_mx* mx, "
            "const fcsa_varlen* seqs, const fcsa_window* window, const fcsa_lse_out* lse_out);") in header and "NO WORKSPACE" in header
    call = lib.fcsa_forward_kvcache_mx_prefill
    assert call(None, None, None, None, None, None) == -1 and b"kvcache_mx_prefill: null argument" in lib.fcsa_last_error()
    none = _lib.Tensor(None, 0, 0, 0)
    mx, seqs, kv = _lib.KvCacheMx(_lib.FCSA_CACHE_MXFP4, none, none), _lib.Varlen(None, None, 0, 0), _lib.KvCache()

    def run(D=64, mx=mx, seqs=seqs, win=None, causal=False):
        prob = _lib.problem(torch.bfloat16, (0, 4, 2, 0, 0, D), causal)
        fa = _lib.ForwardArgs(prob, none, none, none, none, None, None, None, _lib.NormState(None, None, None, None), None, 0, None)
        return call(C.byref(fa), C.byref(kv), C.byref(mx), None if seqs is None else C.byref(seqs), None if win is None else C.byref(win), None), lib.fcsa_last_error()

    assert run()[0] == 0      # an empty batch passes every check and launches nothing
    for kw, code, text in ((dict(seqs=None), -1, b"fcsa_forward_kvcache_mx takes equal-N calls"), (dict(mx=_lib.KvCacheMx(7, none, none)), -2, b"format 7"),
                           (dict(D=32), -2, b"dim_head 32 is not supported (64 or 128; fcsa_forward_kvcache_mx"),
                           (dict(win=_lib.Window(8, -1)), -2, b"hides keys"), (dict(win=_lib.Window(-1, 3)), -2, b"hides keys")):
        rc, msg = run(**kw)
        assert rc == code and text in msg, (kw, rc, msg)
    assert run(win=_lib.Window(-1, 3), causal=True)[0] == 0      # causal caps the right side: nothing hidden


@pytest.mark.parametrize("kw", [dict(causal=True), dict(groups=4, scale=2.0, return_lse=True), dict(l2norm_qk=False, scale=0.125, return_lse=True)])
def test_cpu_path_is_the_decode_calls(kw):
    a, b = _args(), _args()
    new, ref = F.flash_cosine_sim_attention_mxfp4_prefill_with_kvcache(**a, **kw), getattr(F, DECODE)(**b, **kw)
    for x, y in zip(new if isinstance(new, tuple) else (new,), ref if isinstance(ref, tuple) else (ref,)):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    for k in ("k_cache", "v_cache", "k_block_scale", "v_block_scale"):
        assert torch.equal(a[k], b[k]) and not torch.equal(a[k], _args()[k])      # the append landed, identically
