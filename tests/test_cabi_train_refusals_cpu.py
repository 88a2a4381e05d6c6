"""The refusals of the C ABI's training entry points (csrc/fcsa_capi.hip), through ctypes and without a GPU.

fcsa_forward, fcsa_forward_varlen, fcsa_forward_window, fcsa_forward_alibi, their backward twins, fcsa_backward_state and
fcsa_attention_lse share one front end: null check, the problem, the checks of the options a call brings (sliding window, slopes, packed
sequences), then the buffers.  REFUSALS is a literal table of (entry point, broken arguments, return code, substring of
fcsa_last_error()); the substrings are copied by hand from the source.  Rows with two broken arguments fix the order of the checks: the
fault named is the one that stands first.  Every pointer is a fake aligned address that is never dereferenced: each row fails
validation before anything is launched.

Shapes: B 2, H 4, Hk 2, N = M = 16, D 64, bfloat16; packed: 3 rows in two sequences."""
import ctypes as C
import os

import pytest

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4


@pytest.fixture(scope="module")
def lib():
    from flash_cosine_sim_attention_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


PROBLEM = dict(dtype=2, batch=2, heads=4, kv_heads=2, q_len=16, k_len=16, dim_head=64, causal=0, bias_batch_dim=0, l2norm_qk=0, groups=1,
               scale=8.0)
PTR = 0x10000          # a 256-byte aligned fake address
NULL_T = (None, 0, 0, 0)
WS_DENSE = 512 + 2 * 32768      # delta [2, 4, 16] float32, then per-query-head dk and dv slabs [2, 4, 16, 64] float32 (grouped K/V)
WS_PACKED = 256 + 2 * 3072      # the same for the packed rows [1, 4, 3]


def _struct(cls, **kw):
    from flash_cosine_sim_attention_amd import _lib
    return getattr(_lib, cls)(**kw)


def _tensor(spec=(0x1000, 4096, 1024, 64)):
    return _struct("Tensor", ptr=spec[0], stride0=spec[1], stride1=spec[2], stride2=spec[3])


def _build(entry, broken):
    """the ctypes arguments of `entry`: valid ones, with `broken` applied"""
    from flash_cosine_sim_attention_amd import _lib
    b = dict(broken)
    backward = "backward" in entry
    packed_entry, window_entry, alibi_entry = entry.endswith("_varlen"), entry.endswith("_window"), entry.endswith("_alibi")
    p = _lib.Problem(**{k: b.pop(k, v) for k, v in PROBLEM.items()})
    seqs = b.pop("seqs", {} if packed_entry else None)
    if seqs is not None:
        seqs = _lib.Varlen(**{**dict(cu_seqlens_q=0x4000, cu_seqlens_k=0x4100, total_q=3, total_k=3), **seqs})
    w = b.pop("w", (4, 0) if window_entry else None)
    if w is not None:
        w = _lib.Window(*w)
    al = b.pop("al", {} if alibi_entry else None)
    if al is not None:
        al = _lib.Alibi(**{**dict(slopes=0x5000, stride_b=0, stride_h=1, reserved=0), **al})
    ref = lambda s: None if s is None else C.byref(s)
    if entry == "fcsa_attention_lse":
        lo = b.pop("lse_out", {})
        if lo is not None:
            lo = _lib.LseOut(**{**dict(lse=0x6000, stride0=64, stride1=16, stride2=1), **lo})
        args = (None if b.pop("p", 1) is None else C.byref(p), b.pop("inv_l", 0x3000), ref(seqs), ref(w), ref(lo), None)
        assert not b, b
        return args
    norm = _lib.NormState(**b.pop("norm", {}))
    if backward:
        a = _lib.BackwardArgs(p=p, inv_l=b.pop("inv_l", 0x3000), mask=b.pop("mask", None), attn_bias=b.pop("attn_bias", None), norm=norm,
                              d_bias=b.pop("d_bias", None), workspace=b.pop("workspace", PTR), workspace_bytes=b.pop("workspace_bytes", 1 << 30))
        names = ("d_out", "o", "q", "k", "v", "dq", "dk", "dv")
    else:
        a = _lib.ForwardArgs(p=p, inv_l=b.pop("inv_l", None), mask=b.pop("mask", None), attn_bias=b.pop("attn_bias", None), norm=norm)
        names = ("q", "k", "v", "o")
    for n in names:
        setattr(a, n, _tensor(b.pop(n)) if n in b else _tensor())
    a_ref = None if b.pop("args", 1) is None else C.byref(a)
    tail = {"": (), "_varlen": (ref(seqs),), "_window": (ref(seqs), ref(w)), "_alibi": (ref(seqs), ref(w), ref(al)),
            "_state": (ref(seqs), ref(w), b.pop("d_lse", None))}[entry[len("fcsa_backward" if backward else "fcsa_forward"):]]
    assert not b, b
    return (a_ref,) + tail


F, FV, FW, FA = "fcsa_forward", "fcsa_forward_varlen", "fcsa_forward_window", "fcsa_forward_alibi"
B, BV, BW, BA, BS = "fcsa_backward", "fcsa_backward_varlen", "fcsa_backward_window", "fcsa_backward_alibi", "fcsa_backward_state"
LSE = "fcsa_attention_lse"
EVERY = (F, FV, FW, FA, B, BV, BW, BA, BS, LSE)

NULL_ARGS = "null args"
DIM_HEAD = "dim_head 48 not in {16, 32, 64, 96, 128}"
VARLEN_OPTIONS = "varlen: mask and attn_bias are not supported with packed sequences"
VARLEN_TOTALS = "varlen: total_q / total_k (-1, 3) outside [0, 2^31)"
VARLEN_ROWS = "varlen: heads x packed rows above 2^31"
WINDOW_SIDES = "window: left / right (-2, 0) must be >= 0, or -1 for unbounded"
WINDOW_OPTIONS = "window: mask and attn_bias are not supported with a sliding window"
ALIBI_OPTIONS = "alibi: mask and attn_bias are not supported with alibi_slopes"
ALIBI_NULL = "alibi: null slopes"
ALIBI_ALIGN = "alibi: slopes not 4-byte aligned"
ALIBI_RESERVED = "alibi: reserved must be 0"
ALIBI_LENGTHS = "alibi: a non-causal call needs q_len <= k_len (16 > 8): rows with pos_i < 0 have no key at distance 0"
MASK_CAUSAL = "mask should not be given if causal (cu:1675)"
STATE_OPTIONS = "backward_state: mask, attn_bias and d_bias are not supported with attention states (the log-sum-exp)"
NORM_BACKWARD = "l2norm_qk backward needs norm.qn, norm.kn, norm.rq, norm.rk from forward"
WS_SMALL = lambda need: "workspace too small: 0 < %d bytes" % need
WS_ALIGN = "workspace not 256-byte aligned"

# (entry point, {argument: its broken value}, return code, substring of fcsa_last_error())
REFUSALS = [
    # ---- null arguments
    *[(e, dict(args=None), INVALID, "backward_state: null args" if e == BS else NULL_ARGS) for e in EVERY if e != LSE],
    (LSE, dict(p=None), INVALID, "attention_lse: null argument"),
    (LSE, dict(lse_out=None), INVALID, "attention_lse: null argument"),
    # ---- the problem: every refusal on the two plain calls, one on every other entry point
    *[(e, broken, rc, text) for e in (F, B) for broken, rc, text in (
        (dict(dtype=7), UNSUPPORTED, "unsupported dtype 7 (expected f32=0, f16=1, bf16=2)"),
        (dict(dim_head=48), UNSUPPORTED, DIM_HEAD),
        (dict(batch=-1), INVALID, "negative size (B=-1 H=4 N=16 M=16)"),
        (dict(kv_heads=3), INVALID, "kv_heads must divide heads (4), got 3"),
        (dict(kv_heads=0), INVALID, "kv_heads must divide heads (4), got 0"),
        (dict(l2norm_qk=1, groups=5), INVALID, "groups (5) must divide dim_head (64)"),
        (dict(l2norm_qk=1, dtype=1, scale=50000.0), UNSUPPORTED, "float16: scale 50000 puts scale * log2(e) * q^ outside the type"),
        (dict(groups=2), INVALID, "groups must be 1 when l2norm_qk is 0"),
        (dict(scale=float("nan")), INVALID, "scale is NaN or infinite"),
        (dict(scale=float("inf")), INVALID, "scale is NaN or infinite"))],
    *[(e, dict(dim_head=48), UNSUPPORTED, DIM_HEAD) for e in EVERY if e not in (F, B)],
    *[(e, dict(dim_head=48, seqs={}), UNSUPPORTED, DIM_HEAD) for e in (FW, FA, BW, BA, BS, LSE)],
    # ---- packed sequences
    (FV, dict(seqs=None), INVALID, "varlen: null sequence table"),
    (BV, dict(seqs=None), INVALID, "varlen: null sequence table"),
    (FV, dict(mask=PTR), INVALID, VARLEN_OPTIONS),
    (FV, dict(attn_bias=PTR), INVALID, VARLEN_OPTIONS),
    (BV, dict(mask=PTR), INVALID, VARLEN_OPTIONS),
    (BV, dict(attn_bias=PTR), INVALID, VARLEN_OPTIONS),
    (BV, dict(d_bias=PTR), INVALID, VARLEN_OPTIONS),
    *[(e, dict(seqs=dict(total_q=-1)), INVALID, VARLEN_TOTALS) for e in (FV, FW, FA, BV, BW, BA, BS, LSE)],
    (FV, dict(seqs=dict(total_k=-1)), INVALID, "varlen: total_q / total_k (3, -1) outside [0, 2^31)"),
    (BV, dict(seqs=dict(total_k=1 << 31)), INVALID, "varlen: total_q / total_k (3, 2147483648) outside [0, 2^31)"),
    *[(e, dict(seqs=dict(cu_seqlens_q=None)), INVALID, "varlen: null cu_seqlens") for e in (FV, FW, FA, BV, BW, BA, BS, LSE)],
    (FV, dict(seqs=dict(cu_seqlens_k=None)), INVALID, "varlen: null cu_seqlens"),
    *[(e, dict(seqs=dict(total_k=1 << 30)), UNSUPPORTED, VARLEN_ROWS) for e in (FV, FW, FA, BV, BW, BA, BS, LSE)],
    # ---- the sliding window
    (FW, dict(w=None), INVALID, "window: null window"),
    (BW, dict(w=None), INVALID, "window: null window"),
    (FW, dict(w=None, seqs={}), INVALID, "window: null window"),
    *[(e, dict(w=(-2, 0)), INVALID, WINDOW_SIDES) for e in (FW, FA, BW, BA, BS, LSE)],
    *[(e, dict(w=(-2, 0), seqs={}), INVALID, WINDOW_SIDES) for e in (FW, FA, BW, BA, BS, LSE)],
    (FW, dict(w=(0, -2)), INVALID, "window: left / right (0, -2) must be >= 0, or -1 for unbounded"),
    (FW, dict(mask=PTR), INVALID, WINDOW_OPTIONS),
    (FW, dict(attn_bias=PTR), INVALID, WINDOW_OPTIONS),
    (BW, dict(mask=PTR), INVALID, WINDOW_OPTIONS),
    (BW, dict(attn_bias=PTR), INVALID, WINDOW_OPTIONS),
    (BW, dict(d_bias=PTR), INVALID, WINDOW_OPTIONS),
    (FW, dict(mask=PTR, w=(-1, -1)), INVALID, WINDOW_OPTIONS),      # (a window that hides nothing is refused the same way)
    # ---- the slopes
    (FA, dict(mask=PTR), INVALID, ALIBI_OPTIONS),
    (FA, dict(attn_bias=PTR), INVALID, ALIBI_OPTIONS),
    (BA, dict(mask=PTR), INVALID, ALIBI_OPTIONS),
    (BA, dict(attn_bias=PTR), INVALID, ALIBI_OPTIONS),
    (BA, dict(d_bias=PTR), INVALID, ALIBI_OPTIONS),
    *[(e, broken, INVALID, text) for e in (FA, BA) for broken, text in (
        (dict(al=None), ALIBI_NULL),
        (dict(al=dict(slopes=None)), ALIBI_NULL),
        (dict(al=dict(slopes=0x5002)), ALIBI_ALIGN),
        (dict(al=dict(reserved=1)), ALIBI_RESERVED),
        (dict(al=dict(reserved=1), seqs={}), ALIBI_RESERVED),
        (dict(k_len=8), ALIBI_LENGTHS),
        (dict(k_len=8, w=(4, 0)), ALIBI_LENGTHS))],
    # ---- mask with causal
    (F, dict(causal=1, mask=PTR), INVALID, MASK_CAUSAL),
    (B, dict(causal=1, mask=PTR), INVALID, MASK_CAUSAL),
    # ---- the forward's buffers
    (F, dict(q=NULL_T), INVALID, "q: null pointer"),
    (F, dict(k=NULL_T), INVALID, "k: null pointer"),
    (F, dict(v=(0x1004, 4096, 1024, 64)), INVALID, "v: base not 16-byte aligned"),
    (F, dict(o=(0x1000, 4096, 1020, 64)), INVALID, "o: strides (4096, 1020, 64) must keep rows 16-byte aligned"),
    (F, dict(q=(0x1000, 0, 0, 1 << 22)), UNSUPPORTED, "q: row stride 4194304 elements is negative or above 4 MiB"),
    (F, dict(l2norm_qk=1), INVALID, "l2norm_qk needs the norm.kn buffer"),
    (F, dict(l2norm_qk=1, norm=dict(kn=PTR), inv_l=0x3000), INVALID, "l2norm_qk needs the norm.qn buffer for this problem (fcsa_forward_needs_qn)"),
    (F, dict(l2norm_qk=1, norm=dict(kn=PTR), dtype=0), INVALID, "l2norm_qk needs the norm.qn buffer for this problem (fcsa_forward_needs_qn)"),
    (FV, dict(l2norm_qk=1), INVALID, "l2norm_qk needs the norm.kn buffer"),
    (FW, dict(l2norm_qk=1), INVALID, "l2norm_qk needs the norm.kn buffer"),
    (FW, dict(l2norm_qk=1, seqs={}), INVALID, "l2norm_qk needs the norm.kn buffer"),
    (FA, dict(l2norm_qk=1), INVALID, "l2norm_qk needs the norm.kn buffer"),
    (FA, dict(l2norm_qk=1, seqs={}, w=(4, 0)), INVALID, "l2norm_qk needs the norm.kn buffer"),
    (FV, dict(o=NULL_T), INVALID, "o: null pointer"),
    (FW, dict(k=NULL_T), INVALID, "k: null pointer"),
    (FA, dict(v=NULL_T), INVALID, "v: null pointer"),
    (FA, dict(k_len=8, seqs={}, q=NULL_T), INVALID, "q: null pointer"),      # (a packed call has no q_len <= k_len rule: its lengths are on the device)
    (FA, dict(k_len=8, causal=1, q=NULL_T), INVALID, "q: null pointer"),     # (nor has a causal one)
    # ---- the backward's buffers, then its workspace
    (B, dict(d_out=NULL_T), INVALID, "d_out: null pointer"),
    (B, dict(dv=(0x1008, 4096, 1024, 64)), INVALID, "dv: base not 16-byte aligned"),
    (B, dict(q=NULL_T), INVALID, "q: null pointer"),
    (B, dict(l2norm_qk=1), INVALID, NORM_BACKWARD),
    (B, dict(l2norm_qk=1, norm=dict(qn=PTR, kn=PTR, rq=PTR)), INVALID, NORM_BACKWARD),
    (B, dict(inv_l=None), INVALID, "inv_l: null pointer"),
    (B, dict(d_bias=PTR), INVALID, "d_bias without attn_bias"),
    (B, dict(workspace_bytes=0), WORKSPACE, WS_SMALL(WS_DENSE)),
    (B, dict(workspace=None), WORKSPACE, "workspace too small: 1073741824 < %d bytes" % WS_DENSE),
    (B, dict(workspace=PTR + 16), WORKSPACE, WS_ALIGN),
    (B, dict(attn_bias=PTR, d_bias=PTR, workspace_bytes=0), WORKSPACE, WS_SMALL(WS_DENSE)),
    *[(e, dict(inv_l=None), INVALID, "inv_l: null pointer") for e in (BV, BW, BA, BS)],
    *[(e, dict(l2norm_qk=1), INVALID, NORM_BACKWARD) for e in (BV, BW, BA, BS)],
    *[(e, dict(workspace_bytes=0), WORKSPACE, WS_SMALL(WS_DENSE)) for e in (BW, BA, BS)],
    *[(e, dict(workspace_bytes=0, seqs={}), WORKSPACE, WS_SMALL(WS_PACKED)) for e in (BV, BW, BA, BS)],
    *[(e, dict(workspace=PTR + 16), WORKSPACE, WS_ALIGN) for e in (BV, BW, BA, BS)],
    (BW, dict(workspace_bytes=0, w=(-1, -1)), WORKSPACE, WS_SMALL(WS_DENSE)),      # a window that hides nothing: the un-windowed call
    (BW, dict(workspace_bytes=0, w=(-1, 0), seqs={}), WORKSPACE, WS_SMALL(WS_PACKED)),      # ... and the causal one
    (BA, dict(workspace_bytes=0, w=(4, 0), seqs={}), WORKSPACE, WS_SMALL(WS_PACKED)),
    (BS, dict(workspace_bytes=0, w=(4, 0)), WORKSPACE, WS_SMALL(WS_DENSE)),
    (BS, dict(workspace_bytes=0, w=(4, 0), seqs={}, d_lse=PTR), WORKSPACE, WS_SMALL(WS_PACKED)),
    (BA, dict(k_len=8, seqs={}, workspace_bytes=0), WORKSPACE, WS_SMALL(WS_PACKED)),
    # ---- attention states
    (BS, dict(mask=PTR), INVALID, STATE_OPTIONS),
    (BS, dict(attn_bias=PTR), INVALID, STATE_OPTIONS),
    (BS, dict(d_bias=PTR), INVALID, STATE_OPTIONS),
    (LSE, dict(lse_out=dict(lse=None)), INVALID, "attention_lse: lse_out: null pointer"),
    (LSE, dict(inv_l=None), INVALID, "attention_lse: inv_l: null pointer"),
    (LSE, dict(inv_l=None, seqs={}, w=(4, 0)), INVALID, "attention_lse: inv_l: null pointer"),
    # ---- two faults at once: the one named stands first
    (FW, dict(args=None, w=None), INVALID, NULL_ARGS),
    (FV, dict(dim_head=48, seqs=None), UNSUPPORTED, DIM_HEAD),
    (FW, dict(dim_head=48, w=None), UNSUPPORTED, DIM_HEAD),
    (FA, dict(dim_head=48, al=None), UNSUPPORTED, DIM_HEAD),
    (BS, dict(dim_head=48, mask=PTR), INVALID, STATE_OPTIONS),      # (the state call looks at its options before the problem)
    (FW, dict(w=(-2, 0), seqs=dict(total_q=-1)), INVALID, WINDOW_SIDES),      # a windowed packed call: the window before the table
    (BW, dict(w=(-2, 0), seqs=dict(total_q=-1)), INVALID, WINDOW_SIDES),
    (BS, dict(w=(-2, 0), seqs=dict(total_q=-1)), INVALID, WINDOW_SIDES),
    (LSE, dict(w=(-2, 0), seqs=dict(total_q=-1)), INVALID, VARLEN_TOTALS),    # (fcsa_attention_lse: the table before the window)
    (FW, dict(w=(-2, 0), mask=PTR), INVALID, WINDOW_SIDES),
    (BW, dict(w=None, mask=PTR), INVALID, "window: null window"),
    (FW, dict(mask=PTR, seqs=dict(total_q=-1)), INVALID, WINDOW_OPTIONS),
    (FV, dict(mask=PTR, seqs=dict(total_q=-1)), INVALID, VARLEN_OPTIONS),
    (BV, dict(seqs=dict(total_q=-1, cu_seqlens_q=None)), INVALID, VARLEN_TOTALS),
    (FV, dict(seqs=dict(cu_seqlens_q=None, total_k=1 << 30)), INVALID, "varlen: null cu_seqlens"),
    (FA, dict(mask=PTR, al=None), INVALID, ALIBI_OPTIONS),          # a call with slopes: the mask before the slopes
    (BA, dict(d_bias=PTR, al=None), INVALID, ALIBI_OPTIONS),
    (FA, dict(mask=PTR, w=(-2, 0)), INVALID, ALIBI_OPTIONS),
    (FA, dict(w=(-2, 0), al=None), INVALID, WINDOW_SIDES),          # ... the window before the slopes
    (BA, dict(w=(-2, 0), al=dict(reserved=1)), INVALID, WINDOW_SIDES),
    (FA, dict(al=dict(slopes=None, reserved=1)), INVALID, ALIBI_NULL),
    (FA, dict(al=dict(slopes=0x5002, reserved=1)), INVALID, ALIBI_ALIGN),
    (BA, dict(al=dict(reserved=1), k_len=8), INVALID, ALIBI_RESERVED),
    (FA, dict(al=dict(reserved=1), seqs=dict(total_q=-1)), INVALID, ALIBI_RESERVED),      # ... and the slopes before the table
    (BA, dict(k_len=8, seqs=dict(total_q=-1)), INVALID, VARLEN_TOTALS),
    (F, dict(causal=1, mask=PTR, k=NULL_T), INVALID, MASK_CAUSAL),
    (F, dict(k=NULL_T, l2norm_qk=1), INVALID, "k: null pointer"),
    (B, dict(causal=1, mask=PTR, dq=NULL_T), INVALID, MASK_CAUSAL),
    (B, dict(dq=NULL_T, inv_l=None), INVALID, "dq: null pointer"),
    (B, dict(l2norm_qk=1, inv_l=None), INVALID, NORM_BACKWARD),
    (B, dict(inv_l=None, d_bias=PTR), INVALID, "inv_l: null pointer"),
    (B, dict(d_bias=PTR, workspace_bytes=0), INVALID, "d_bias without attn_bias"),
    (B, dict(workspace_bytes=0, workspace=PTR + 16), WORKSPACE, WS_SMALL(WS_DENSE)),
    (BV, dict(inv_l=None, workspace_bytes=0), INVALID, "inv_l: null pointer"),
    (LSE, dict(lse_out=dict(lse=None), inv_l=None), INVALID, "attention_lse: lse_out: null pointer"),
]


def _id(row):
    return "-".join([row[0][len("fcsa_"):], *row[1]])


def test_every_entry_point_has_rows():
    assert {r[0] for r in REFUSALS} == set(EVERY)


@pytest.mark.parametrize("row", REFUSALS, ids=[f"{i:03d}-{_id(r)}" for i, r in enumerate(REFUSALS)])
def test_refusal(lib, row):
    entry, broken, code, text = row
    rc = getattr(lib, entry)(*_build(entry, broken))
    assert (rc, text in lib.fcsa_last_error().decode()) == (code, True), (rc, lib.fcsa_last_error())


def test_calls_without_a_row_return_ok_before_any_buffer(lib):
    """a size of zero ends a call after its checks and before any pointer is looked at"""
    for entry in (F, FV, FW, FA, B, BV, BW, BA, BS, LSE):
        broken = dict(heads=0, kv_heads=0, q=NULL_T, k=NULL_T, v=NULL_T, o=NULL_T) if entry != LSE else dict(heads=0, kv_heads=0, inv_l=None)
        assert getattr(lib, entry)(*_build(entry, broken)) == OK, (entry, lib.fcsa_last_error())
    assert lib.fcsa_attention_lse(*_build(LSE, dict(seqs=dict(total_q=0), inv_l=None))) == OK
    assert lib.fcsa_forward_window(*_build(FW, dict(heads=0, kv_heads=0, w=(-2, 0)))) == INVALID      # ... and never before them


def _workspace_args(p=1, seqs=None, w=None, **problem):
    from flash_cosine_sim_attention_amd import _lib
    ref = lambda s: None if s is None else C.byref(s)
    prob = _lib.Problem(**{**PROBLEM, **problem})
    table = None if seqs is None else _lib.Varlen(**{**dict(cu_seqlens_q=0x4000, cu_seqlens_k=0x4100, total_q=3, total_k=3), **seqs})
    return (None if p is None else C.byref(prob), ref(table), ref(None if w is None else _lib.Window(*w)))


def test_backward_workspace_functions_on_null_and_negative_totals(lib):
    plain, varlen = lib.fcsa_backward_workspace_bytes, lib.fcsa_backward_varlen_workspace_bytes
    window, alibi = lib.fcsa_backward_window_workspace_bytes, lib.fcsa_backward_alibi_workspace_bytes
    assert plain(None) == 0
    assert varlen(*_workspace_args(p=None, seqs={})[:2]) == 0
    assert varlen(*_workspace_args()[:2]) == 0                                      # no table
    assert varlen(*_workspace_args(seqs=dict(total_q=-1))[:2]) == 0
    assert varlen(*_workspace_args(seqs=dict(total_k=-1))[:2]) == 0
    assert window(*_workspace_args(p=None, w=(4, 0))) == 0
    assert window(*_workspace_args()) == 0                                          # no window
    assert window(*_workspace_args(seqs={})) == 0
    assert window(*_workspace_args(seqs=dict(total_q=-1), w=(4, 0))) == 0
    assert window(*_workspace_args(seqs=dict(total_k=-1), w=(-1, -1))) == 0
    assert alibi(*_workspace_args(p=None, seqs={}, w=(4, 0))) == 0
    assert alibi(*_workspace_args(seqs=dict(total_q=-1))) == 0
    assert alibi(*_workspace_args(seqs=dict(total_k=-1), w=(4, 0))) == 0
    # and what they return for the calls of the table above
    assert plain(_workspace_args()[0]) == window(*_workspace_args(w=(4, 0))) == alibi(*_workspace_args()) == WS_DENSE
    assert varlen(*_workspace_args(seqs={})[:2]) == window(*_workspace_args(seqs={}, w=(4, 0))) == alibi(*_workspace_args(seqs={})) == WS_PACKED


def test_backward_workspace_by_form(lib):
    """One rule for the four functions.  A windowed launch has the plan of a packed call (no split, no group sweep); a window that hides
    nothing is the un-windowed or the causal call and is sized like it; a call with slopes is always a windowed launch, whatever its
    window.  The problem splits its dQ eight ways un-windowed (tests/test_cabi_cpu.py::test_split_counts_follow_the_measured_tables)."""
    al = lambda x: (x + 255) // 256 * 256
    big = dict(dtype=1, batch=1, heads=8, kv_heads=8, q_len=1024, k_len=8192, l2norm_qk=1)
    split, unsplit = al(8 * 1024 * 4) + al(8 * 8 * 1024 * 64 * 4), al(8 * 1024 * 4)
    window, alibi = lib.fcsa_backward_window_workspace_bytes, lib.fcsa_backward_alibi_workspace_bytes
    assert lib.fcsa_backward_workspace_bytes(_workspace_args(**big)[0]) == split
    assert window(*_workspace_args(w=(4, 0), **big)) == unsplit
    assert window(*_workspace_args(w=(-1, -1), **big)) == split
    assert window(*_workspace_args(w=(8191, 1023), **big)) == split              # sides that reach every key: hides nothing
    assert window(*_workspace_args(w=(8190, 1023), **big)) == unsplit
    for w in (None, (4, 0), (-1, -1)):
        assert alibi(*_workspace_args(w=w, **big)) == unsplit
    packed = dict(seqs=dict(total_q=100, total_k=120))
    rows = al(8 * 100 * 4)
    assert lib.fcsa_backward_varlen_workspace_bytes(*_workspace_args(**packed, **big)[:2]) == rows
    assert window(*_workspace_args(w=(-1, -1), **packed, **big)) == window(*_workspace_args(w=(4, 0), **packed, **big)) == rows
    assert alibi(*_workspace_args(w=(-1, -1), **packed, **big)) == alibi(*_workspace_args(**packed, **big)) == rows
