"""The refusals of the compiled binding's training ops (csrc/fcsa_torch.cpp), reached through torch.ops directly.

The Python functions of ops.py check their arguments first, so the binding's own TORCH_CHECKs are shadowed in every other test: nothing
else pins their exception types, their messages or the order in which they stand.  REFUSALS is a literal table of (op, broken arguments,
exception type, message substring); the substrings are copied by hand from the binding's source.  Rows with two broken arguments fix the
order of the checks: the fault named is the one that stands first.

Shapes: B 2, H 4, Hk 2, N = M = 16, D 64, bfloat16; packed: 3 rows in two sequences (counts 1 and 2).  Every row raises before anything
is launched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, HK, N, D, TOTAL = 2, 4, 2, 16, 64, 3
DT = torch.bfloat16


# ---- broken arguments: each maps the valid argument to a broken one
CPU = lambda t: t.cpu()
AS = lambda dtype: (lambda t: t.to(dtype))
NONE = lambda t: None
SHAPE = lambda *shape: (lambda t: t.new_zeros(shape))
WITH_GRAD = lambda t: t.clone().requires_grad_()


def _valid(op, packed=False):
    """keyword arguments that `op` accepts, by the names of its schema"""
    dev = "cuda"
    packed = packed or "varlen" in op
    rows_q, rows_k = ((H, TOTAL), (HK, TOTAL)) if packed else ((B, H, N), (B, HK, N))
    q = torch.zeros((TOTAL, H, D) if packed else (B, H, N, D), device=dev, dtype=DT)
    k = torch.zeros((TOTAL, HK, D) if packed else (B, HK, N, D), device=dev, dtype=DT)
    cu = torch.tensor([0, 1, 3], dtype=torch.int32, device=dev) if packed else None
    windowed = op.startswith("fcsa::")      # the window ops take their sides as they are; (-1, -1) is "no window" to the others
    pool = dict(q=q, k=k, v=k.clone(), d_out=q.clone(), o=q.clone(), d_lse=None, mask=None, attn_bias=None, attn_bias_batch_dim=False,
                inv_l=torch.ones(rows_q, device=dev), qn=torch.zeros(rows_q + (D,), device=dev, dtype=DT),
                kn=torch.zeros(rows_k + (D,), device=dev, dtype=DT), rq=torch.ones(rows_q + (1,), device=dev),
                rk=torch.ones(rows_k + (1,), device=dev), cu_seqlens_q=cu, cu_seqlens_k=None if cu is None else cu.clone(),
                max_seqlen_q=2 if packed else 0, max_seqlen_k=2 if packed else 0, scale=8.0, causal=False, l2norm_qk=True, groups=1,
                need_backward=True, need_bias_grad=False, window_left=4 if windowed else -1, window_right=0 if windowed else -1,
                alibi_slopes=torch.ones(H, device=dev))
    return {a.name: pool[a.name] for a in _op(op)._schema.arguments}


FWD, BWD, ATT = "fcsa::forward", "fcsa::backward", "fcsa::attention"
VF, VB, VA = "fcsa::varlen_forward", "fcsa::varlen_backward", "fcsa::varlen_attention"
WF, WB, WA = "fcsa::window_forward", "fcsa::window_backward", "fcsa::window_attention"
VWF, VWB, VWA = "fcsa::varlen_window_forward", "fcsa::varlen_window_backward", "fcsa::varlen_window_attention"
SF, SB, SA = "fcsa_state::attention_state_forward", "fcsa_state::attention_state_backward", "fcsa_state::attention_state"
AF, AB, AA = "fcsa_alibi_train::forward", "fcsa_alibi_train::backward", "fcsa_alibi_train::attention"
EVERY = (FWD, BWD, ATT, VF, VB, VA, WF, WB, WA, VWF, VWB, VWA, SF, SB, SA, AF, AB, AA)
PACKED = dict(packed=True)

GPU_ONLY = "flash_cosine_sim_attention_amd: q, k, v must be GPU tensors (HIP kernels only, no CPU fallback)"
GPU_ONLY_PACKED = "flash_cosine_sim_attention_varlen: q, k, v must be GPU tensors (HIP kernels only, no CPU fallback)"
SHARE = "q, k, v must share a dtype, got BFloat16, Float, BFloat16"
DOUBLE = "unsupported dtype Double; expected float32, float16 or bfloat16"
DIMS = "only dimensions (16, 32, 64, 96, 128) allowed for now, got 48"
SAME_SHAPE = "k and v must have the same shape, got"
SAME_D = "query, key, value dimensions must be the same"
KV_HEADS = "k/v heads must divide q heads (4): grouped-query attention needs H % Hk == 0, got Hk = 3"
MASK_CAUSAL = "mask should not be supplied if causality is needed"
PACKED_3D = "varlen: q, k, v must be packed [total, heads, dim_head] tensors"
CU_INT32 = "cu_seqlens_q / cu_seqlens_k must be int32"
CU_LENGTHS = "cu_seqlens_q and cu_seqlens_k must be 1-D of the same length (sequences + 1), got [3] and [4]"
MAX_SEQLEN = "max_seqlen_q / max_seqlen_k must lie in [0, 2^31), got -1, 2"
TOGETHER = "cu_seqlens_q and cu_seqlens_k must be given together"
STATE_4D = "attention_state takes 4-D q, k, v, or packed 3-D ones with cu_seqlens"
WINDOW = "window_size (-2, 0): each side must be >= 0, or -1 for unbounded"
GROUPS = "groups (5) must divide the head dimension (64)"
SLOPES_F32 = "alibi_slopes must be float32, got Double"
SLOPES_DEVICE = "alibi_slopes is on cpu but q is on cuda:0: all tensors must live on q's GPU"
SLOPES_SHAPE = "alibi_slopes must be [heads] (4) or [batch, heads] (2, 4), got [3]"
SLOPES_SHAPE_PACKED = "alibi_slopes must be [heads] (4) or [sequences, heads] (2, 4), got [3]"
SLOPES_LENGTHS = "alibi_slopes: a non-causal call needs q_len <= k_len, got 16 > 8 (rows with a negative position have no key at distance 0)"
SLOPES_GRAD = "alibi_slopes must not require grad: there is no slope gradient (fixed slopes only)"
D_OUT_SHAPE = "d_out must have the shape of the output"
O_SHAPE = "o does not belong to these inputs"
O_TYPE = "o must have the dtype and device of q"
D_OUT_DEVICE = "d_out is on cpu but q is on cuda:0"
SAVED = lambda name, dtype, numel: f"{name} does not belong to these inputs (expected a contiguous {dtype} tensor of {numel} elements on cuda:0)"
INV_L, INV_L_PACKED = SAVED("inv_l", "Float", B * H * N), SAVED("inv_l", "Float", H * TOTAL)
QN, KN = SAVED("qn", "BFloat16", B * H * N * D), SAVED("kn", "BFloat16", B * HK * N * D)
RQ, RK = SAVED("rq", "Float", B * H * N), SAVED("rk", "Float", B * HK * N)
D_LSE = "d_lse must have the shape of lse on q's device"
SHORT_KV = dict(k=SHAPE(B, HK, 8, D), v=SHAPE(B, HK, 8, D))
BAD_WINDOW = dict(window_left=-2, window_right=0)

# (op, options of _valid, {argument: how to break it, or a plain value to pass}, exception type, substring of the message)
REFUSALS = [
    # ---- canonicalise: the dense calls
    *[(op, {}, dict(q=CPU), RuntimeError, GPU_ONLY) for op in (FWD, BWD, ATT, WF, WB, WA, SF, SB, SA, AF, AB, AA)],
    (FWD, {}, dict(k=CPU), ValueError, "k is on cpu but q is on cuda:0: all tensors must live on q's GPU"),
    (BWD, {}, dict(v=CPU), ValueError, "v is on cpu but q is on cuda:0"),
    (FWD, {}, dict(mask=lambda t: torch.ones(B, N, dtype=torch.bool)), ValueError, "mask is on cpu but q is on cuda:0"),
    (ATT, {}, dict(attn_bias=lambda t: torch.zeros(H, N, N, dtype=DT)), ValueError, "attn_bias is on cpu but q is on cuda:0"),
    *[(op, {}, dict(k=AS(torch.float32)), TypeError, SHARE) for op in (FWD, BWD, WF, SF, AB)],
    (FWD, {}, dict(q=AS(torch.float64), k=AS(torch.float64), v=AS(torch.float64)), TypeError, DOUBLE),
    (FWD, {}, dict(causal=True, mask=lambda t: torch.ones(B, N, dtype=torch.bool, device="cuda")), ValueError, MASK_CAUSAL),
    (BWD, {}, dict(causal=True, mask=lambda t: torch.ones(B, N, dtype=torch.bool, device="cuda")), ValueError, MASK_CAUSAL),
    (FWD, {}, dict(q=SHAPE(B * H, N, D)), ValueError, "if batch and heads are merged for queries, keys and values must also have 3 dimensions"),
    (FWD, {}, dict(q=SHAPE(1, B, H, N, D)), ValueError, "q must have 3 or 4 dimensions, got 5"),
    (FWD, {}, dict(k=SHAPE(1, B, HK, N, D)), ValueError, "k and v must have 3 or 4 dimensions"),
    *[(op, {}, dict(v=SHAPE(B, HK, N + 1, D)), ValueError, SAME_SHAPE) for op in (FWD, BWD, WA, SA, AF)],
    (FWD, {}, dict(k=SHAPE(B, HK, N, 32), v=SHAPE(B, HK, N, 32)), ValueError, SAME_D),
    *[(op, {}, dict(q=SHAPE(B, H, N, 48), k=SHAPE(B, HK, N, 48), v=SHAPE(B, HK, N, 48)), ValueError, DIMS) for op in (FWD, WB, SB, AA)],
    (FWD, {}, dict(k=SHAPE(3, HK, N, D), v=SHAPE(3, HK, N, D)), ValueError, "batch mismatch between q (2) and k/v (3)"),
    *[(op, {}, dict(k=SHAPE(B, 3, N, D), v=SHAPE(B, 3, N, D)), ValueError, KV_HEADS) for op in (FWD, BWD, WF, SF, AF)],
    (FWD, {}, dict(mask=lambda t: torch.ones(B, N + 1, dtype=torch.bool, device="cuda")), ValueError, "mask must be a bool tensor of shape (2, 16), got Bool [2, 17]"),
    (FWD, {}, dict(mask=lambda t: torch.ones(B, N, dtype=torch.uint8, device="cuda")), ValueError, "mask must be a bool tensor of shape (2, 16), got Byte [2, 16]"),
    (FWD, {}, dict(attn_bias=lambda t: torch.zeros(B, N, N, dtype=DT, device="cuda")), ValueError, "attn_bias must have shape (4, 16, 16), got [2, 16, 16]"),
    (FWD, {}, dict(attn_bias=lambda t: torch.zeros(H, N, N, dtype=DT, device="cuda"), attn_bias_batch_dim=True), ValueError,
     "attn_bias must have shape (2, 16, 16), got [4, 16, 16]"),
    (BWD, {}, dict(attn_bias=lambda t: torch.zeros(H, N, N, device="cuda")), TypeError, "attn_bias must have the dtype of q"),
    *[(op, {}, dict(groups=5), ValueError, GROUPS) for op in (FWD, ATT, WF, SF, AF)],
    (VF, {}, dict(groups=5), ValueError, GROUPS),
    # ---- canonicalise_varlen: the packed calls
    *[(op, {}, dict(q=CPU), RuntimeError, GPU_ONLY_PACKED) for op in (VF, VB, VA, VWF, VWB, VWA)],
    *[(op, PACKED, dict(q=CPU), RuntimeError, GPU_ONLY_PACKED) for op in (SF, SB, SA, AF, AB, AA)],
    (VF, {}, dict(v=CPU), ValueError, "v is on cpu but q is on cuda:0"),
    *[(op, {}, dict(cu_seqlens_q=CPU), ValueError, "cu_seqlens_q is on cpu but q is on cuda:0") for op in (VF, VB, VWA)],
    (SF, PACKED, dict(cu_seqlens_k=CPU), ValueError, "cu_seqlens_k is on cpu but q is on cuda:0"),
    *[(op, {}, dict(k=AS(torch.float32)), TypeError, SHARE) for op in (VF, VWB)],
    (VA, {}, dict(q=AS(torch.float64), k=AS(torch.float64), v=AS(torch.float64)), TypeError, DOUBLE),
    *[(op, {}, dict(q=SHAPE(1, TOTAL, H, D)), ValueError, PACKED_3D) for op in (VF, VB, VWF)],
    (AF, PACKED, dict(k=SHAPE(1, TOTAL, HK, D)), ValueError, PACKED_3D),
    (VF, {}, dict(v=SHAPE(TOTAL + 1, HK, D)), ValueError, SAME_SHAPE),
    *[(op, {}, dict(cu_seqlens_k=AS(torch.int64)), TypeError, CU_INT32) for op in (VF, VB, VA, VWF)],
    (AB, PACKED, dict(cu_seqlens_q=AS(torch.int64)), TypeError, CU_INT32),
    *[(op, {}, dict(cu_seqlens_k=SHAPE(4)), ValueError, CU_LENGTHS) for op in (VF, VWB)],
    (SB, PACKED, dict(cu_seqlens_k=SHAPE(4)), ValueError, CU_LENGTHS),
    (VF, {}, dict(cu_seqlens_q=SHAPE(1, 3), cu_seqlens_k=SHAPE(1, 3)), ValueError, "must be 1-D of the same length (sequences + 1), got [1, 3] and [1, 3]"),
    (VF, {}, dict(k=SHAPE(TOTAL, HK, 32), v=SHAPE(TOTAL, HK, 32)), ValueError, SAME_D),
    (VF, {}, dict(q=SHAPE(TOTAL, H, 48), k=SHAPE(TOTAL, HK, 48), v=SHAPE(TOTAL, HK, 48)), ValueError, DIMS),
    *[(op, {}, dict(k=SHAPE(TOTAL, 3, D), v=SHAPE(TOTAL, 3, D)), ValueError, "k/v heads must divide q heads (4), got 3") for op in (VF, VB, VWA)],
    *[(op, {}, dict(max_seqlen_q=-1), ValueError, MAX_SEQLEN) for op in (VF, VB, VA, VWF, VWB)],
    (AF, PACKED, dict(max_seqlen_q=-1), ValueError, MAX_SEQLEN),
    (VF, {}, dict(max_seqlen_k=1 << 31), ValueError, "max_seqlen_q / max_seqlen_k must lie in [0, 2^31), got 2, 2147483648"),
    # ---- the ops that take dense or packed tensors
    *[(op, PACKED, dict(cu_seqlens_k=NONE), ValueError, TOGETHER) for op in (SF, SB, SA, AF, AB, AA)],
    *[(op, {}, dict(cu_seqlens_q=lambda t: torch.tensor([0, 1, 3], dtype=torch.int32, device="cuda")), ValueError, TOGETHER) for op in (SF, AF)],
    *[(op, PACKED, dict(cu_seqlens_q=NONE, cu_seqlens_k=NONE), ValueError, STATE_4D) for op in (SF, SB, SA, AF, AB, AA)],
    (SF, {}, dict(k=SHAPE(B * HK, N, D), v=SHAPE(B * HK, N, D)), ValueError, STATE_4D),
    # ---- the window
    *[(op, {}, BAD_WINDOW, ValueError, WINDOW) for op in (WF, WB, WA, VWF, VWB, VWA, SF, SB, SA, AF, AB, AA)],
    *[(op, PACKED, BAD_WINDOW, ValueError, WINDOW) for op in (SF, SB, AF, AB)],
    (WF, {}, dict(window_left=-1, window_right=-2), ValueError, "window_size (-1, -2): each side must be >= 0, or -1 for unbounded"),
    (SF, {}, dict(window_left=0, window_right=-3), ValueError, "window_size (0, -3): each side must be >= 0, or -1 for unbounded"),
    # ---- the slopes
    *[(op, {}, dict(alibi_slopes=AS(torch.float64)), TypeError, SLOPES_F32) for op in (AF, AB, AA)],
    *[(op, {}, dict(alibi_slopes=CPU), ValueError, SLOPES_DEVICE) for op in (AF, AB, AA)],
    *[(op, {}, dict(alibi_slopes=SHAPE(3)), ValueError, SLOPES_SHAPE) for op in (AF, AB, AA)],
    *[(op, {}, dict(alibi_slopes=SHAPE(3, H)), ValueError, "alibi_slopes must be [heads] (4) or [batch, heads] (2, 4), got [3, 4]") for op in (AF, AB)],
    *[(op, PACKED, dict(alibi_slopes=SHAPE(3)), ValueError, SLOPES_SHAPE_PACKED) for op in (AF, AB, AA)],
    *[(op, {}, SHORT_KV, ValueError, SLOPES_LENGTHS) for op in (AF, AA)],
    (AB, {}, SHORT_KV, ValueError, SLOPES_LENGTHS),
    (AA, {}, dict(alibi_slopes=WITH_GRAD), ValueError, SLOPES_GRAD),
    (AA, PACKED, dict(alibi_slopes=WITH_GRAD), ValueError, SLOPES_GRAD),
    # ---- backward_body: d_out, o and the saved state
    *[(op, {}, dict(d_out=SHAPE(B, H, N + 1, D)), ValueError, D_OUT_SHAPE) for op in (BWD, WB, SB, AB)],
    *[(op, {}, dict(d_out=SHAPE(TOTAL + 1, H, D)), ValueError, D_OUT_SHAPE) for op in (VB, VWB)],
    *[(op, {}, dict(d_out=SHAPE(B, H, N + 1, D), o=SHAPE(B, H, N + 1, D)), ValueError, O_SHAPE) for op in (BWD, WB, SB, AB)],
    (VB, {}, dict(d_out=SHAPE(TOTAL + 1, H, D), o=SHAPE(TOTAL + 1, H, D)), ValueError, O_SHAPE),
    *[(op, {}, dict(o=AS(torch.float32)), TypeError, O_TYPE) for op in (BWD, VB, WB, VWB, SB, AB)],
    (BWD, {}, dict(o=CPU), TypeError, O_TYPE),
    *[(op, {}, dict(d_out=CPU), ValueError, D_OUT_DEVICE) for op in (BWD, VB, SB, AB)],
    *[(op, {}, dict(inv_l=SHAPE(B, H, N + 1)), ValueError, INV_L) for op in (BWD, WB, SB, AB)],
    *[(op, {}, dict(inv_l=SHAPE(H, TOTAL + 1)), ValueError, INV_L_PACKED) for op in (VB, VWB)],
    *[(op, PACKED, dict(inv_l=SHAPE(H, TOTAL + 1)), ValueError, INV_L_PACKED) for op in (SB, AB)],
    (BWD, {}, dict(inv_l=AS(DT)), ValueError, INV_L),
    (BWD, {}, dict(inv_l=CPU), ValueError, INV_L),
    (BWD, {}, dict(inv_l=lambda t: t.new_zeros(B, N, H).transpose(1, 2)), ValueError, INV_L),
    *[(op, {}, dict(qn=SHAPE(B, H, N, 32)), ValueError, QN) for op in (BWD, WB, SB, AB)],
    *[(op, {}, dict(kn=AS(torch.float32)), ValueError, KN) for op in (BWD, SB)],
    *[(op, {}, dict(rq=SHAPE(B, H, N, 2)), ValueError, RQ) for op in (BWD, AB)],
    *[(op, {}, dict(rk=AS(DT)), ValueError, RK) for op in (BWD, WB)],
    (VB, {}, dict(rk=SHAPE(HK, TOTAL + 1, 1)), ValueError, SAVED("rk", "Float", HK * TOTAL)),
    (BWD, {}, dict(groups=2, rq=SHAPE(B, H, N, 1)), ValueError, SAVED("rq", "Float", B * H * N * 2)),
    # ---- the gradient of the log-sum-exp
    (SB, {}, dict(d_lse=lambda t: torch.zeros(B, H, N + 1, device="cuda")), ValueError, D_LSE),
    (SB, {}, dict(d_lse=lambda t: torch.zeros(B, H, N)), ValueError, D_LSE),
    (SB, PACKED, dict(d_lse=lambda t: torch.zeros(H, TOTAL, device="cuda")), ValueError, D_LSE),      # [total_q, H] is its public layout
    # ---- two faults at once: the one named stands first
    (FWD, {}, dict(q=CPU, k=AS(torch.float32)), RuntimeError, GPU_ONLY),
    (FWD, {}, dict(k=lambda t: t.float().cpu()), ValueError, "k is on cpu but q is on cuda:0"),
    (FWD, {}, dict(k=AS(torch.float32), causal=True, mask=lambda t: torch.ones(B, N, dtype=torch.bool, device="cuda")), TypeError, SHARE),
    (FWD, {}, dict(causal=True, mask=lambda t: torch.ones(B, N + 1, dtype=torch.bool, device="cuda")), ValueError, MASK_CAUSAL),
    (FWD, {}, dict(q=SHAPE(B, H, N, 48), k=SHAPE(3, HK, N, 48), v=SHAPE(3, HK, N, 48)), ValueError, DIMS),
    (FWD, {}, dict(k=SHAPE(3, 3, N, D), v=SHAPE(3, 3, N, D)), ValueError, "batch mismatch between q (2) and k/v (3)"),
    (FWD, {}, dict(groups=5, q=SHAPE(B, H, N, 48), k=SHAPE(B, HK, N, 48), v=SHAPE(B, HK, N, 48)), ValueError, DIMS),
    (BWD, {}, dict(groups=5, d_out=SHAPE(B, H, N + 1, D)), ValueError, D_OUT_SHAPE),      # (the backward has no groups check of its own)
    (VF, {}, dict(cu_seqlens_q=lambda t: t.long().cpu()), ValueError, "cu_seqlens_q is on cpu but q is on cuda:0"),
    (VF, {}, dict(q=SHAPE(1, TOTAL, H, D), cu_seqlens_q=AS(torch.int64)), ValueError, PACKED_3D),
    (VF, {}, dict(cu_seqlens_q=AS(torch.int64), cu_seqlens_k=SHAPE(4)), TypeError, CU_INT32),
    (VF, {}, dict(cu_seqlens_k=SHAPE(4), max_seqlen_q=-1), ValueError, CU_LENGTHS),
    (VB, {}, dict(max_seqlen_q=-1, inv_l=SHAPE(H, TOTAL + 1)), ValueError, MAX_SEQLEN),
    *[(op, {}, dict(BAD_WINDOW, q=CPU), ValueError, WINDOW) for op in (WF, WB, VWF, VWB, SF, SB, AF, AB)],      # the window before the tensors
    *[(op, PACKED, dict(BAD_WINDOW, cu_seqlens_k=NONE), ValueError, WINDOW) for op in (SF, SB, AF, AB)],
    *[(op, PACKED, dict(cu_seqlens_k=NONE, q=CPU), ValueError, TOGETHER) for op in (SF, SB, AF, AB)],
    *[(op, {}, dict(BAD_WINDOW, alibi_slopes=AS(torch.float64)), ValueError, WINDOW) for op in (AF, AB)],
    *[(op, {}, dict(q=CPU, alibi_slopes=AS(torch.float64)), RuntimeError, GPU_ONLY) for op in (AF, AB)],          # ... and the tensors before the slopes
    *[(op, {}, dict(groups=5, alibi_slopes=SHAPE(3)), ValueError, SLOPES_SHAPE) for op in (AF, AA)],
    (AF, {}, dict(alibi_slopes=lambda t: t.double().cpu()), TypeError, SLOPES_F32),
    (AF, {}, dict(alibi_slopes=lambda t: t.new_zeros(3).cpu()), ValueError, SLOPES_DEVICE),
    (AF, {}, dict(alibi_slopes=SHAPE(3), **SHORT_KV), ValueError, SLOPES_SHAPE),
    (AA, {}, dict(BAD_WINDOW, alibi_slopes=lambda t: t.double().requires_grad_()), ValueError, SLOPES_GRAD),      # the autograd key's own check
    (AA, {}, dict(alibi_slopes=WITH_GRAD, q=CPU), ValueError, SLOPES_GRAD),
    (AB, {}, dict(alibi_slopes=SHAPE(3), inv_l=SHAPE(B, H, N + 1)), ValueError, SLOPES_SHAPE),      # the slopes before the saved state
    (AB, {}, dict(alibi_slopes=SHAPE(3), d_out=SHAPE(B, H, N + 1, D)), ValueError, SLOPES_SHAPE),
    (BWD, {}, dict(d_out=SHAPE(B, H, N + 1, D), inv_l=SHAPE(B, H, N + 1)), ValueError, D_OUT_SHAPE),
    (BWD, {}, dict(o=AS(torch.float32), d_out=CPU), TypeError, O_TYPE),
    (BWD, {}, dict(d_out=CPU, inv_l=SHAPE(B, H, N + 1)), ValueError, D_OUT_DEVICE),
    (BWD, {}, dict(inv_l=SHAPE(B, H, N + 1), qn=SHAPE(B, H, N, 32)), ValueError, INV_L),
    (BWD, {}, dict(qn=SHAPE(B, H, N, 32), kn=AS(torch.float32)), ValueError, QN),
    (BWD, {}, dict(kn=AS(torch.float32), rq=SHAPE(B, H, N, 2)), ValueError, KN),
    (BWD, {}, dict(rq=SHAPE(B, H, N, 2), rk=AS(DT)), ValueError, RQ),
    (SB, {}, dict(inv_l=SHAPE(B, H, N + 1), d_lse=lambda t: torch.zeros(B, H, N + 1, device="cuda")), ValueError, INV_L),      # the saved state before d_lse
    (SB, {}, dict(rk=AS(DT), d_lse=lambda t: torch.zeros(B, H, N + 1, device="cuda")), ValueError, RK),
    (SB, {}, dict(BAD_WINDOW, d_lse=lambda t: torch.zeros(B, H, N + 1, device="cuda")), ValueError, WINDOW),
]


def _id(row):
    op, options, broken = row[:3]
    return "-".join([op.replace("::", "."), *options, *broken])


def _op(name):
    from flash_cosine_sim_attention_amd import _torch_ops
    _torch_ops.load()
    namespace, op = name.split("::")
    return getattr(getattr(torch.ops, namespace), op).default


def test_every_training_op_has_rows():
    assert {r[0] for r in REFUSALS} == set(EVERY)


@pytest.mark.parametrize("row", REFUSALS, ids=[f"{i:03d}-{_id(r)}" for i, r in enumerate(REFUSALS)])
def test_refusal(row):
    name, options, broken, exc, message = row
    kw = _valid(name, **options)
    for arg, how in broken.items():
        assert arg in kw, arg
        kw[arg] = how(kw[arg]) if callable(how) else how
    with pytest.raises(exc) as e:
        _op(name)(**kw)
    assert type(e.value) is exc, type(e.value)
    assert message in str(e.value), str(e.value)
