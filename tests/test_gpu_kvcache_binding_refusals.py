"""The refusals of the compiled binding's key/value-cache ops (csrc/fcsa_torch.cpp), reached through torch.ops directly.

The Python functions of ops.py check their arguments first, so the binding's own TORCH_CHECKs are shadowed in every other test: nothing
else pins their exception types, their messages or the order in which they stand.  REFUSALS is a literal table of (op, broken arguments,
exception type, message substring); the substrings are copied by hand from the binding's source.  Rows with two broken arguments fix the
order of the checks: the fault named is the one that stands first.

Shapes: B 2, H 4, Hk 2, D 64, bfloat16; a capacity of 32, contiguous or as two pages of 16 per sequence; N 1, or 3 packed rows (counts
1 and 2).  Every row raises before anything is launched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, HK, D, CAP, PAGE = 2, 4, 2, 64, 32, 16
DT = torch.bfloat16


# ---- broken arguments: each maps the valid argument to a broken one
CPU = lambda t: t.cpu()
AS = lambda dtype: (lambda t: t.to(dtype))
NONE = lambda t: None
CACHE3 = lambda t: t.new_zeros((3,) + tuple(t.shape[1:]))               # a contiguous cache of 3 sequences: a batch mismatch
PAGE8 = lambda t: t.new_zeros((t.shape[0], t.shape[1], 8, t.shape[3]))  # a paged pool with pages of 8
ROWS3 = lambda t: t.new_zeros((3, t.shape[1]))                          # a block_table of 3 rows: a batch mismatch
LEN4 = lambda t: t.new_zeros((4,))                                      # a tree_mask of 4 words for 3 packed rows
SHAPE3 = lambda t: t.new_zeros((3,))                                    # slopes that are neither [4] nor [2, 4]
COLS65 = lambda t: t.new_zeros((t.shape[0], 65))                        # accepted with 65 columns
ONES = lambda t: torch.ones(HK, device="cuda")                          # a scale where none was given


def _valid(op, paged=False, append=False, ragged=None, fp8=False):
    """keyword arguments that `op` accepts"""
    dev = "cuda"
    name = op.split("::")[1]
    if ragged is None:
        ragged = name not in ("kvcache_forward", "kvcache_window_forward", "kvcache_fp8_forward", "kvcache_lse_forward")
    fp8 = fp8 or name == "kvcache_fp8_forward"
    cache = (2 * B, HK, PAGE, D) if paged else (B, HK, CAP, D)
    kw = dict(k_cache=torch.zeros(cache, device=dev, dtype=torch.uint8 if fp8 else DT),
              v_cache=torch.zeros(cache, device=dev, dtype=torch.uint8 if fp8 else DT),
              cache_seqlens=torch.full((B,), 8, dtype=torch.int32, device=dev),
              block_table=torch.arange(2 * B, dtype=torch.int32, device=dev).view(B, 2) if paged else None)
    if name == "kvcache_compact":
        kw.update(accepted=torch.zeros(B, 3, dtype=torch.int32, device=dev), num_accepted=torch.ones(B, dtype=torch.int32, device=dev))
        return kw
    q = torch.zeros((3, H, D) if ragged else (B, H, 1, D), device=dev, dtype=DT)
    new = torch.zeros((3, HK, D) if ragged else (B, HK, 1, D), device=dev, dtype=DT) if append else None
    kw.update(q=q, k_new=new, v_new=None if new is None else new.clone(), max_seqlen_k=CAP, scale=8.0, l2norm_qk=True, groups=1)
    if name != "kvcache_tree_forward":
        kw.update(causal=True)
    if ragged or name == "kvcache_lse_forward":
        kw.update(cu_seqlens_q=torch.tensor([0, 1, 3], dtype=torch.int32, device=dev) if ragged else None, max_seqlen_q=2 if ragged else 0)
    if name == "kvcache_fp8_forward":
        kw.update(k_scale=torch.ones(HK, device=dev), v_scale=torch.ones(HK, device=dev))
    elif name not in ("kvcache_forward", "kvcache_window_forward", "kvcache_prefill_forward"):
        kw.update(k_scale=torch.ones(HK, device=dev) if fp8 else None, v_scale=torch.ones(HK, device=dev) if fp8 else None)
    if name not in ("kvcache_forward", "kvcache_prefill_forward", "kvcache_tree_forward"):
        kw.update(window_left=-1, window_right=-1)
    if name in ("kvcache_step_forward", "kvcache_alibi_forward"):
        kw.update(chunk_rows=-1, max_decode_tokens=-1, no_decode=False, no_chunk=False)
    if name == "kvcache_tree_forward":
        kw.update(tree_mask=torch.full((3,), -1, dtype=torch.int64, device=dev))
    if name == "kvcache_alibi_forward":
        kw.update(alibi_slopes=torch.ones(H, device=dev))
    return kw


FWD, WIN, FP8, VARLEN, LSE = ("fcsa::kvcache_forward", "fcsa::kvcache_window_forward", "fcsa::kvcache_fp8_forward",
                              "fcsa::kvcache_varlen_forward", "fcsa::kvcache_lse_forward")
PREFILL, STEP, TREE, ALIBI, COMPACT = ("fcsa_prefill::kvcache_prefill_forward", "fcsa_step::kvcache_step_forward",
                                       "fcsa_tree::kvcache_tree_forward", "fcsa_alibi::kvcache_alibi_forward", "fcsa_tree::kvcache_compact")

GPU_ONLY = "q and the caches must be GPU tensors"
TOGETHER_NEW = "k_new and v_new must be given together"
TOGETHER_SCALES = "k_scale and v_scale must be given together"
CODES = "takes the e4m3fn codes of both caches as uint8 tensors"
PAGE_RULE = "page_size (8) must be a positive multiple of 16"
MISMATCH = "batch mismatch between q (2) and the caches (3)"
CHUNK_ROWS = "chunk_rows must be a non-negative integer (or -1: the default), got -2"

# (op, options of _valid, {argument: how to break it, or a plain value to pass}, exception type, substring of the message)
REFUSALS = [
    # ---- the equal-N ops
    (FWD, {}, dict(q=CPU), RuntimeError, GPU_ONLY),
    (FWD, {}, dict(k_cache=CPU), ValueError, "k_cache is on cpu but q is on cuda:0"),
    (FWD, {}, dict(v_cache=CPU), ValueError, "v_cache is on cpu but q is on cuda:0"),
    (FWD, {}, dict(cache_seqlens=CPU), ValueError, "cache_seqlens is on cpu but q is on cuda:0"),
    (FWD, {}, dict(cache_seqlens=AS(torch.int64)), TypeError, "cache_seqlens must be int32"),
    (FWD, dict(paged=True), dict(block_table=AS(torch.int64)), TypeError, "block_table must be int32"),
    (FWD, dict(paged=True), dict(block_table=ROWS3), ValueError, "block_table must be [batch, max_blocks]"),
    (FWD, dict(paged=True), dict(k_cache=PAGE8, v_cache=PAGE8), ValueError, PAGE_RULE),
    (FWD, dict(append=True), dict(v_new=NONE), ValueError, TOGETHER_NEW),
    (FWD, {}, dict(k_cache=CACHE3, v_cache=CACHE3), ValueError, MISMATCH),
    (WIN, {}, dict(q=CPU), RuntimeError, GPU_ONLY),
    (WIN, {}, dict(cache_seqlens=AS(torch.int64)), TypeError, "cache_seqlens must be int32"),
    (WIN, dict(paged=True), dict(k_cache=PAGE8, v_cache=PAGE8), ValueError, PAGE_RULE),
    (WIN, dict(append=True), dict(v_new=NONE), ValueError, TOGETHER_NEW),
    (FP8, {}, dict(k_cache=AS(DT), v_cache=AS(DT)), TypeError, CODES),
    (FP8, {}, dict(k_scale=CPU), ValueError, "k_scale is on cpu but q is on cuda:0"),
    (FP8, {}, dict(cache_seqlens=AS(torch.int64)), TypeError, "cache_seqlens must be int32"),
    (FP8, {}, dict(k_cache=CACHE3, v_cache=CACHE3), ValueError, MISMATCH),
    (LSE, {}, dict(q=CPU), RuntimeError, GPU_ONLY),
    (LSE, {}, dict(k_scale=ONES), ValueError, TOGETHER_SCALES),
    (LSE, {}, dict(k_scale=ONES, v_scale=ONES), TypeError, CODES),
    (LSE, {}, dict(cache_seqlens=AS(torch.int64)), TypeError, "cache_seqlens must be int32"),
    (LSE, dict(ragged=True), dict(cu_seqlens_q=AS(torch.int64)), TypeError, "cu_seqlens_q must be int32"),
    (LSE, dict(paged=True), dict(k_cache=PAGE8, v_cache=PAGE8), ValueError, PAGE_RULE),
    # ---- the packed ops
    (VARLEN, {}, dict(q=CPU), RuntimeError, GPU_ONLY),
    (VARLEN, {}, dict(cu_seqlens_q=CPU), ValueError, "cu_seqlens_q is on cpu but q is on cuda:0"),
    (VARLEN, {}, dict(cu_seqlens_q=AS(torch.int64)), TypeError, "cu_seqlens_q must be int32"),
    (VARLEN, {}, dict(cache_seqlens=AS(torch.int64)), TypeError, "cache_seqlens must be int32"),
    (VARLEN, dict(paged=True), dict(block_table=AS(torch.int64)), TypeError, "block_table must be int32"),
    (VARLEN, dict(paged=True), dict(k_cache=PAGE8, v_cache=PAGE8), ValueError, PAGE_RULE),
    (VARLEN, {}, dict(v_scale=ONES), ValueError, TOGETHER_SCALES),
    (VARLEN, {}, dict(k_scale=ONES, v_scale=ONES), TypeError, CODES),
    (VARLEN, dict(append=True), dict(k_new=NONE), ValueError, TOGETHER_NEW),
    (VARLEN, {}, dict(k_cache=CACHE3, v_cache=CACHE3), ValueError, MISMATCH),
    (PREFILL, {}, dict(q=CPU), RuntimeError, GPU_ONLY),
    (PREFILL, {}, dict(cu_seqlens_q=AS(torch.int64)), TypeError, "cu_seqlens_q must be int32"),
    (PREFILL, {}, dict(cache_seqlens=AS(torch.int64)), TypeError, "cache_seqlens must be int32"),
    (PREFILL, dict(paged=True), dict(block_table=AS(torch.int64)), TypeError, "block_table must be int32"),
    (PREFILL, dict(append=True), dict(v_new=NONE), ValueError, TOGETHER_NEW),
    (PREFILL, {}, dict(k_cache=CACHE3, v_cache=CACHE3), ValueError, MISMATCH),
    (STEP, {}, dict(q=CPU), RuntimeError, GPU_ONLY),
    (STEP, {}, dict(chunk_rows=-2), ValueError, CHUNK_ROWS),
    (STEP, {}, dict(k_scale=ONES), ValueError, TOGETHER_SCALES),
    (STEP, {}, dict(k_scale=ONES, v_scale=ONES), TypeError, CODES),
    (STEP, {}, dict(cu_seqlens_q=AS(torch.int64)), TypeError, "cu_seqlens_q must be int32"),
    (STEP, {}, dict(cache_seqlens=AS(torch.int64)), TypeError, "cache_seqlens must be int32"),
    (STEP, dict(paged=True), dict(k_cache=PAGE8, v_cache=PAGE8), ValueError, PAGE_RULE),
    (STEP, dict(append=True), dict(v_new=NONE), ValueError, TOGETHER_NEW),
    (STEP, {}, dict(k_cache=CACHE3, v_cache=CACHE3), ValueError, MISMATCH),
    (TREE, {}, dict(q=CPU), RuntimeError, GPU_ONLY),
    (TREE, {}, dict(tree_mask=AS(torch.int32)), TypeError, "tree_mask must be int64, got Int"),
    (TREE, {}, dict(tree_mask=CPU), ValueError, "tree_mask is on cpu but q is on cuda:0"),
    (TREE, {}, dict(tree_mask=LEN4), ValueError, "tree_mask must be [total_q] (3), packed like q, got [4]"),
    (TREE, {}, dict(v_scale=ONES), ValueError, TOGETHER_SCALES),
    (TREE, {}, dict(cu_seqlens_q=AS(torch.int64)), TypeError, "cu_seqlens_q must be int32"),
    (TREE, dict(paged=True), dict(block_table=AS(torch.int64)), TypeError, "block_table must be int32"),
    (TREE, dict(append=True), dict(v_new=NONE), ValueError, TOGETHER_NEW),
    (ALIBI, {}, dict(q=CPU), RuntimeError, GPU_ONLY),
    (ALIBI, {}, dict(alibi_slopes=AS(torch.float64)), TypeError, "alibi_slopes must be float32, got Double"),
    (ALIBI, {}, dict(alibi_slopes=CPU), ValueError, "alibi_slopes is on cpu but q is on cuda:0"),
    (ALIBI, {}, dict(alibi_slopes=SHAPE3), ValueError, "alibi_slopes must be [heads] (4) or [sequences, heads] (2, 4), got [3]"),
    (ALIBI, {}, dict(chunk_rows=-2), ValueError, CHUNK_ROWS),
    (ALIBI, {}, dict(k_scale=ONES), ValueError, TOGETHER_SCALES),
    (ALIBI, {}, dict(cache_seqlens=AS(torch.int64)), TypeError, "cache_seqlens must be int32"),
    (ALIBI, dict(paged=True), dict(k_cache=PAGE8, v_cache=PAGE8), ValueError, PAGE_RULE),
    (ALIBI, {}, dict(k_cache=CACHE3, v_cache=CACHE3), ValueError, MISMATCH),
    # ---- the compaction of the accepted path: the caches come first, and the page rule is the library's
    (COMPACT, {}, dict(k_cache=CPU), RuntimeError, "kvcache_keep_accepted: the caches must be GPU tensors"),
    (COMPACT, {}, dict(v_cache=CPU), ValueError, "v_cache is on cpu but k_cache is on cuda:0"),
    (COMPACT, {}, dict(accepted=CPU), ValueError, "accepted is on cpu but k_cache is on cuda:0"),
    (COMPACT, {}, dict(cache_seqlens=AS(torch.int64)), TypeError, "cache_seqlens, accepted and num_accepted must be int32"),
    (COMPACT, {}, dict(accepted=COLS65), ValueError, "accepted must be [sequences, A] with 1 <= A <= 64, got [2, 65]"),
    (COMPACT, dict(paged=True), dict(block_table=AS(torch.int64)), TypeError, "block_table must be int32"),
    (COMPACT, dict(paged=True), dict(block_table=ROWS3), ValueError, "block_table must be [sequences, max_blocks]"),
    (COMPACT, dict(paged=True), dict(k_cache=PAGE8, v_cache=PAGE8), RuntimeError,
     "fcsa_kvcache_compact failed (status -1): kvcache_compact: page_size 8 must be a positive multiple of 16"),
    (COMPACT, {}, dict(k_cache=CACHE3, v_cache=CACHE3), ValueError, "batch mismatch between accepted (2) and the caches (3)"),
    # ---- two faults at once: the one named stands first
    (FWD, dict(append=True), dict(q=CPU, v_new=NONE), RuntimeError, GPU_ONLY),
    (FWD, dict(append=True), dict(v_new=NONE, cache_seqlens=AS(torch.int64)), ValueError, TOGETHER_NEW),
    (FWD, dict(paged=True), dict(block_table=AS(torch.int64), cache_seqlens=AS(torch.int64)), TypeError, "block_table must be int32"),
    (FWD, dict(paged=True, append=True), dict(k_cache=PAGE8, v_cache=PAGE8, v_new=NONE), ValueError, PAGE_RULE),
    (FP8, {}, dict(k_cache=AS(DT), v_cache=AS(DT), k_scale=CPU), TypeError, CODES),
    (FP8, {}, dict(k_scale=CPU, cache_seqlens=AS(torch.int64)), TypeError, "cache_seqlens must be int32"),
    (LSE, {}, dict(k_scale=ONES, q=CPU), ValueError, TOGETHER_SCALES),
    (VARLEN, {}, dict(v_scale=ONES, cu_seqlens_q=AS(torch.int64)), ValueError, TOGETHER_SCALES),
    (VARLEN, dict(paged=True), dict(cu_seqlens_q=AS(torch.int64), block_table=AS(torch.int64)), TypeError, "cu_seqlens_q must be int32"),
    (VARLEN, dict(append=True), dict(k_cache=CACHE3, v_cache=CACHE3, v_new=NONE), ValueError, MISMATCH),
    (STEP, {}, dict(k_scale=ONES, chunk_rows=-2), ValueError, TOGETHER_SCALES),
    (STEP, {}, dict(chunk_rows=-2, q=CPU), ValueError, CHUNK_ROWS),
    (TREE, {}, dict(tree_mask=lambda t: t.to(torch.int32).cpu()), TypeError, "tree_mask must be int64, got Int"),
    (TREE, {}, dict(tree_mask=LEN4, cache_seqlens=AS(torch.int64)), ValueError, "tree_mask must be [total_q] (3), packed like q, got [4]"),
    (TREE, {}, dict(cu_seqlens_q=AS(torch.int64), tree_mask=AS(torch.int32)), TypeError, "cu_seqlens_q must be int32"),
    (ALIBI, {}, dict(chunk_rows=-2, alibi_slopes=AS(torch.float64)), ValueError, CHUNK_ROWS),
    (ALIBI, dict(paged=True), dict(alibi_slopes=SHAPE3, k_cache=PAGE8, v_cache=PAGE8), ValueError, "alibi_slopes must be [heads] (4)"),
    (ALIBI, {}, dict(cu_seqlens_q=AS(torch.int64), alibi_slopes=AS(torch.float64)), TypeError, "cu_seqlens_q must be int32"),
    (COMPACT, dict(paged=True), dict(accepted=COLS65, block_table=AS(torch.int64)), ValueError, "accepted must be [sequences, A] with 1 <= A <= 64"),
    (COMPACT, dict(paged=True), dict(cache_seqlens=AS(torch.int64), block_table=ROWS3), TypeError,
     "cache_seqlens, accepted and num_accepted must be int32"),
]


def _id(row):
    op, options, broken = row[:3]
    return "-".join([op.split("::")[1], *options, *broken])


def _op(name):
    from flash_cosine_sim_attention_amd import _torch_ops
    _torch_ops.load()
    namespace, op = name.split("::")
    return getattr(getattr(torch.ops, namespace), op)


def test_every_cache_op_has_rows():
    assert {r[0] for r in REFUSALS} == {FWD, WIN, FP8, VARLEN, LSE, PREFILL, STEP, TREE, ALIBI, COMPACT}


@pytest.mark.parametrize("row", REFUSALS, ids=[f"{i:02d}-{_id(r)}" for i, r in enumerate(REFUSALS)])
def test_refusal(row):
    name, options, broken, exc, message = row
    kw = _valid(name, **options)
    before = {k: (v.clone() if isinstance(v, torch.Tensor) and k in ("k_cache", "v_cache") else None) for k, v in kw.items()}
    for arg, how in broken.items():
        assert arg in kw, arg
        kw[arg] = how(kw[arg]) if callable(how) else how
    with pytest.raises(exc) as e:
        _op(name)(**kw)
    assert type(e.value) is exc, type(e.value)
    assert message in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for k in ("k_cache", "v_cache"):      # refused before anything was launched: the caches that stayed in place are untouched
        if kw[k].shape == before[k].shape and kw[k].device == before[k].device and kw[k].dtype == before[k].dtype:
            assert torch.equal(kw[k], before[k])
