"""Tree attention for speculative decoding without a GPU: flash_cosine_sim_attention_tree_with_kvcache, the ragged call with tree_mask as
one more keyword (its signature says so, and without a mask it is the ragged call; the CPU path gives the
causal call for the chain mask and the plain call for all bits set, bit for bit; a random tree equals a float64 softmax over the explicit
boolean matrix; a sequence of more than 64 tokens is causal), every host refusal, the C ABI's refusals, exports and header text, the pinned
schemas of the fcsa_tree namespace with their fake kernels, kvcache_keep_accepted on CPU tensors, and the visibility probe on the CPU path
with the decidability condition of the GPU probe's table."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import flash_cosine_sim_attention_amd as F
import tolerances as T
import tree_cases as TC
import visibility_probe as VP
from flash_cosine_sim_attention_amd import _lib, _torch_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ragged = F.flash_cosine_sim_attention_varlen_with_kvcache
tree = F.flash_cosine_sim_attention_tree_with_kvcache
keep = F.kvcache_keep_accepted

TREE_SCHEMA = ("fcsa_tree::kvcache_tree_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cu_seqlens_q, Tensor tree_mask, "
               "Tensor? k_new, Tensor? v_new, Tensor? cache_seqlens, Tensor? block_table, Tensor? k_scale, Tensor? v_scale, int max_seqlen_q, "
               "int max_seqlen_k, float scale, bool l2norm_qk, int groups) -> (Tensor, Tensor)")
COMPACT_SCHEMA = ("fcsa_tree::kvcache_compact(Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cache_seqlens, Tensor accepted, "
                  "Tensor num_accepted, Tensor? block_table) -> ()")


def _i32(x):
    return torch.tensor(x, dtype=torch.int32)


def _problem(counts, cached, cap, H=4, Hk=2, D=32, dtype=torch.float32, page=0, seed=0):
    """packed q, new rows and caches (contiguous, or a shuffled pool of pages with its table)"""
    g = torch.Generator().manual_seed(seed)
    B, total = len(counts), sum(counts)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dtype)
    q, kn, vn = rnd(total, H, D), rnd(total, Hk, D), rnd(total, Hk, D)
    kc, vc = rnd(B, Hk, cap, D), rnd(B, Hk, cap, D)
    table = None
    if page:
        nb = cap // page
        table = torch.randperm(B * nb + 2, generator=g)[:B * nb].reshape(B, nb).to(torch.int32)
        pools = []
        for c in (kc, vc):
            pool = torch.zeros(B * nb + 2, Hk, page, D, dtype=dtype)
            for b in range(B):
                for i in range(nb):
                    pool[int(table[b, i])] = c[b, :, i * page:(i + 1) * page]
            pools.append(pool)
        kc, vc = pools
    return q, kc, vc, kn, vn, table


def _call(p, counts, cached, **kw):
    q, kc, vc, kn, vn, table = p
    kc, vc = kc.clone(), vc.clone()
    with torch.no_grad():
        o, lse = (tree if "tree_mask" in kw else ragged)(q, kc, vc, TC.cu_of(counts), kn, vn, _i32(cached), block_table=table, return_lse=True, **kw)
    return o, lse, kc, vc


def test_signature_is_the_ragged_calls_plus_tree_mask_and_without_a_mask_it_is_that_call():
    mine, theirs = inspect.signature(tree).parameters, inspect.signature(ragged).parameters
    assert list(mine) == list(theirs) + ["tree_mask"] and all(mine[n] == theirs[n] for n in theirs) and mine["tree_mask"].default is None
    assert "tree_mask" not in theirs          # the ragged call's own signature is pinned elsewhere and stays
    assert "flash_cosine_sim_attention_tree_with_kvcache" in F.__all__
    counts, cached = [1, 0, 5, 16], [0, 17, 30, 5]
    p = _problem(counts, cached, 64, seed=1)
    q, kc, vc, kn, vn, _ = p
    for kw in (dict(causal=True), dict(window_size=(4, 0), scale=4.0), dict()):
        outs = []
        for fn in (tree, ragged):
            k1, v1 = kc.clone(), vc.clone()
            with torch.no_grad():
                outs.append((*fn(q, k1, v1, TC.cu_of(counts), kn, vn, _i32(cached), return_lse=True, **kw), k1, v1))
        assert _same(*outs)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("page", [0, 16], ids=["contiguous", "paged"])
def test_chain_is_causal_and_all_ones_is_plain_bit_for_bit(page):
    counts, cached, cap = [1, 0, 5, 16, 37, 64], [0, 17, 30, 5, 0, 60], 128
    for kw in (dict(), dict(scale=16.0, groups=2), dict(l2norm_qk=False, scale=1.0)):
        p = _problem(counts, cached, cap, page=page, seed=3)
        assert _same(_call(p, counts, cached, tree_mask=TC.as_int64(TC.words_of("chain", counts)), **kw), _call(p, counts, cached, causal=True, **kw))
        assert _same(_call(p, counts, cached, tree_mask=TC.as_int64(TC.words_of("full", counts)), **kw), _call(p, counts, cached, causal=False, **kw))


def test_chain_without_an_append_and_more_rows_than_keys():
    """no append: L_b = cache_seqlens[b]; N_b > L_b puts the first rows' positions below 0, which do not exist"""
    counts, cached, cap = [3, 20, 40, 2], [0, 5, 40, 64], 64
    q, kc, vc, _, _, _ = _problem(counts, cached, cap, seed=5)
    run = lambda **kw: tree(q, kc, vc, TC.cu_of(counts), cache_seqlens=_i32(cached), return_lse=True, **kw)
    with torch.no_grad():
        assert _same(run(tree_mask=TC.as_int64(TC.words_of("chain", counts))), run(causal=True))
        assert _same(run(tree_mask=TC.as_int64(TC.words_of("full", counts))), run())
        o, lse = run(tree_mask=torch.zeros(sum(counts), dtype=torch.int64))
    assert (o[:3] == 0).all() and torch.isneginf(lse[:3]).all()          # an empty cache and no bit set: o = 0, lse = -inf


def _float64_reference(q, kseq, vseq, vis, scale):
    """softmax(scale * q^ k^T) v in float64 over the boolean matrix vis [N, L], one sequence: q [N, H, D], kseq / vseq [Hk, L, D]"""
    H, G = q.shape[1], q.shape[1] // kseq.shape[0]
    qh = torch.nn.functional.normalize(q.double().permute(1, 0, 2), dim=-1)
    kh = torch.nn.functional.normalize(kseq.double(), dim=-1).repeat_interleave(G, 0)
    s = (scale * qh @ kh.transpose(1, 2)).masked_fill(~torch.as_tensor(vis)[None], float("-inf"))
    some = torch.as_tensor(vis).any(1)[None, :, None]
    p = torch.where(some, torch.softmax(torch.where(some, s, torch.zeros_like(s)), -1), torch.zeros_like(s))
    lse = torch.where(some[..., 0], torch.logsumexp(torch.where(some, s, torch.zeros_like(s)), -1), torch.full(s.shape[:2], float("-inf"), dtype=torch.float64))
    return (p @ vseq.double().repeat_interleave(G, 0)).permute(1, 0, 2), lse.permute(1, 0)


@pytest.mark.parametrize("kind", ["tree", "bits"])
def test_random_masks_equal_the_float64_softmax_over_the_boolean_matrix(kind):
    """float32 tensors on the float32 CPU path against float64: the project's float32 forward bars (tolerances.FWD_TOL)"""
    counts, cached, cap = [1, 5, 16, 37, 64, 7], [0, 30, 5, 0, 60, 40], 128
    p = _problem(counts, cached, cap, seed=11)
    words = TC.words_of(kind, counts, seed=2)
    o, lse, kc, vc = _call(p, counts, cached, tree_mask=TC.as_int64(words))
    cu = TC.cu_of(counts).tolist()
    atol, rtol, _ = T.FWD_TOL["f32"]
    for b, own in enumerate(TC.split_words(words, counts)):
        L = cached[b] + counts[b]
        vis = TC.visibility(own, counts[b], L)
        ref_o, ref_l = _float64_reference(p[0][cu[b]:cu[b + 1]], kc[b, :, :L], vc[b, :, :L], vis, 8.0)
        got_o, got_l = o[cu[b]:cu[b + 1]].double(), lse[cu[b]:cu[b + 1]].double()
        assert bool(((got_o - ref_o).abs() <= atol + rtol * ref_o.abs()).all()), (kind, b, float((got_o - ref_o).abs().max()))
        dead = torch.isneginf(ref_l)
        assert torch.equal(torch.isneginf(got_l), dead)
        assert bool(((got_l - ref_l)[~dead].abs() <= atol + rtol * ref_l[~dead].abs()).all()), (kind, b)


def test_a_sequence_of_more_than_64_tokens_is_causal():
    counts, cached, cap = [3, 70, 5], [10, 20, 0], 128
    p = _problem(counts, cached, cap, seed=7)
    rng = np.random.default_rng(0)
    words = TC.chain(3) + TC.random_bits(70, rng) + TC.chain(5)          # garbage in the words of the long sequence
    assert _same(_call(p, counts, cached, tree_mask=TC.as_int64(words)), _call(p, counts, cached, causal=True))


def test_host_refusals():
    counts, cached, cap = [2, 3], [4, 0], 16
    q, kc, vc, kn, vn, _ = _problem(counts, cached, cap)
    cu, sl, mask = TC.cu_of(counts), _i32(cached), TC.as_int64(TC.words_of("chain", counts))
    run = lambda **kw: tree(q, kc.clone(), vc.clone(), cu, kn, vn, sl, **kw)
    with torch.no_grad():
        assert run(tree_mask=mask).shape == q.shape
        with pytest.raises(ValueError, match="causal"):
            run(tree_mask=mask, causal=True)
        for window in ((4, -1), (-1, 0), (2, 2)):
            with pytest.raises(ValueError, match="window"):
                run(tree_mask=mask, window_size=window)
        for bad in (mask.to(torch.int32), mask.double(), mask.tolist(), 3):
            with pytest.raises(TypeError, match="int64"):
                run(tree_mask=bad)
        for bad in (mask[:-1], mask.reshape(1, -1), torch.zeros(6, dtype=torch.int64)):
            with pytest.raises(ValueError, match="shape"):
                run(tree_mask=bad)
        with pytest.raises(ValueError, match="is on"):
            run(tree_mask=mask.to("meta"))
        # the other cache calls do not take a mask ...
        for fn in (ragged, F.flash_cosine_sim_attention_prefill_with_kvcache, F.flash_cosine_sim_attention_step_with_kvcache):
            with pytest.raises(TypeError, match="tree_mask"):
                fn(q.half(), kc.half(), vc.half(), cu, kn.half(), vn.half(), sl, tree_mask=mask)
        with pytest.raises(TypeError, match="tree_mask"):
            F.flash_cosine_sim_attention_with_kvcache(q[:2].permute(1, 0, 2)[None], kc[:1], vc[:1], tree_mask=mask)
        with pytest.raises(TypeError, match="tree_mask"):
            F.flash_cosine_sim_attention_with_shared_prefix(q, kc, vc, kc, vc, tree_mask=mask)
    # ... and the docs of the calls a step can come from say which call does
    for fn in (ragged, F.flash_cosine_sim_attention_with_kvcache, F.flash_cosine_sim_attention_with_shared_prefix):
        assert "tree_mask" in fn.__doc__ and "`flash_cosine_sim_attention_tree_with_kvcache`" in fn.__doc__, fn.__name__
    doc = " ".join(tree.__doc__.split())
    assert "per-row bit set" in doc and "N_b > 64" in doc and "kvcache_keep_accepted" in doc and "arange(B + 1) * N" in doc
    assert "prefill, engine-step and shared-prefix calls take none" in doc
    assert "kvcache_keep_accepted" in F.__all__


def _tree_args():
    """a well-formed fcsa_forward_kvcache_tree call on synthetic addresses (refused before any launch)"""
    fa, kv, seqs = _lib.ForwardArgs(), _lib.KvCache(), _lib.Varlen()
    fa.p = _lib.problem(torch.bfloat16, (2, 8, 2, 4, 64, 64), False, False, True, 1, 8.0)
    kv.capacity = 64
    seqs.total_q = 5
    seqs.cu_seqlens_q = 4096
    fa.q = fa.o = _lib.Tensor(1 << 20, 0, 64, 8 * 64)
    kv.k_cache = kv.v_cache = _lib.Tensor(1 << 24, 2 * 64 * 64, 64 * 64, 64)
    return fa, kv, seqs, _lib.TreeMask(1 << 16, 0)


def test_c_abi_refusals_exports_and_header():
    lib = _lib.load()
    INVALID = -1
    header = open(os.path.join(ROOT, "include", "fcsa.h")).read()
    for sym in ("fcsa_forward_kvcache_tree", "fcsa_kvcache_compact"):
        assert sym in _lib.EXPORTS and hasattr(lib, sym)
        assert re.search(r"^int\s+" + sym + r"\(", header, flags=re.M), sym
    assert lib.fcsa_debug(None, 0) == 4 == _lib.ABI_VERSION          # additive: the ABI version stays
    buf = C.create_string_buffer(8192)
    lib.fcsa_debug(buf, 8192)
    assert b"decode_tree" in buf.value and b"kv_compact" in buf.value
    flat = " ".join(header.replace("\n *", " ").split())
    for text in ('"decode_tree[_fp8]"', '"kv_compact"', "bit t of its word is set", "N_b > 64", "passes a barrier and then writes",
                 "fcsa_forward_kvcache_varlen_workspace_bytes(p, cache, seqs, quant, NULL)"):
        assert text in flat, text
    # NULL arguments, tree among them
    fa, kv, seqs, tm = _tree_args()
    ref = lambda x: None if x is None else C.byref(x)
    for args in ((None, kv, seqs, tm), (fa, None, seqs, tm), (fa, kv, None, tm), (fa, kv, seqs, None)):
        assert lib.fcsa_forward_kvcache_tree(ref(args[0]), ref(args[1]), ref(args[2]), None, ref(args[3]), None) == INVALID
        assert b"kvcache_tree: null argument" in lib.fcsa_last_error()
    call = lambda: lib.fcsa_forward_kvcache_tree(C.byref(fa), C.byref(kv), C.byref(seqs), None, C.byref(tm), None)
    tm.mask = None
    assert call() == INVALID and b"mask: null pointer" in lib.fcsa_last_error()
    # causal != 0
    fa, kv, seqs, tm = _tree_args()
    fa.p.causal = 1
    assert call() == INVALID and b"causal must be 0" in lib.fcsa_last_error()
    # bad alignment: the mask (8 bytes), a tensor (16 bytes), the workspace (256 bytes)
    fa, kv, seqs, tm = _tree_args()
    tm.mask = (1 << 16) + 4
    assert call() == INVALID and b"mask not 8-byte aligned" in lib.fcsa_last_error()
    fa, kv, seqs, tm = _tree_args()
    fa.q = _lib.Tensor((1 << 20) + 8, 0, 64, 8 * 64)
    assert call() == INVALID and b"16-byte aligned" in lib.fcsa_last_error()
    fa, kv, seqs, tm = _tree_args()
    need = int(lib.fcsa_forward_kvcache_varlen_workspace_bytes(C.byref(fa.p), C.byref(kv), C.byref(seqs), None, None))
    fa.workspace, fa.workspace_bytes = (1 << 28) + 64, need
    assert need > 0 and call() == -4 and b"not 256-byte aligned" in lib.fcsa_last_error()
    fa.workspace, fa.workspace_bytes = 1 << 28, need - 1
    assert call() == -4 and b"workspace too small" in lib.fcsa_last_error()
    tm.reserved = 1
    assert call() == INVALID and b"reserved" in lib.fcsa_last_error()
    # the compaction
    compact = lambda kv, A=4, es=2, D=64, acc=1 << 12, stride=4, num=1 << 13: lib.fcsa_kvcache_compact(ref(kv), 2, 2, D, es, acc, stride, A, num, None)
    assert compact(None) == INVALID and b"kvcache_compact: null argument" in lib.fcsa_last_error()
    _, kv, _, _ = _tree_args()
    kv.cache_seqlens = 1 << 14
    for kwargs, text in ((dict(A=0), b"max_accepted"), (dict(A=65, stride=65), b"max_accepted"), (dict(stride=3), b"row stride"), (dict(acc=None), b"null accepted"),
                         (dict(num=None), b"null accepted")):
        assert compact(kv, **kwargs) == INVALID and text in lib.fcsa_last_error(), text
    assert compact(kv, es=3) == -2 and compact(kv, D=48) == -2
    kv.k_cache = _lib.Tensor((1 << 24) + 2, 2 * 64 * 64, 64 * 64, 64)
    assert compact(kv) == INVALID and b"16-byte aligned" in lib.fcsa_last_error()


def test_the_ops_have_their_own_namespace_pinned_schemas_and_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    _torch_ops.load()
    names = {n.split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith("fcsa_tree::")}
    assert names == {"fcsa_tree::kvcache_tree_forward", "fcsa_tree::kvcache_compact"}
    assert str(torch.ops.fcsa_tree.kvcache_tree_forward.default._schema) == TREE_SCHEMA
    assert str(torch.ops.fcsa_tree.kvcache_compact.default._schema) == COMPACT_SCHEMA
    for name in names:
        assert torch._C._dispatch_has_kernel_for_dispatch_key(name, "CUDA")
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(name, "Autograd") and not torch._C._dispatch_has_kernel_for_dispatch_key(name, "CPU")
    assert not any(n.startswith(("fcsa::kvcache_tree", "fcsa::kvcache_compact")) for n in torch._C._dispatch_get_all_op_names())
    with FakeTensorMode():
        q = torch.empty(7, 8, 128, dtype=torch.float16)
        kc = torch.empty(2, 2, 64, 128, dtype=torch.uint8)
        cu, mask, s = torch.empty(3, dtype=torch.int32), torch.empty(7, dtype=torch.int64), torch.empty(2, 2)
        o, lse = torch.ops.fcsa_tree.kvcache_tree_forward(q, kc, kc.clone(), cu, mask, None, None, None, None, s, s, 7, 64, 8.0, True, 1)
        none = torch.ops.fcsa_tree.kvcache_compact(kc, kc.clone(), torch.empty(2, dtype=torch.int32), torch.empty(2, 4, dtype=torch.int32),
                                                   torch.empty(2, dtype=torch.int32), None)
    assert o.shape == (7, 8, 128) and o.dtype == torch.float16 and lse.shape == (7, 8) and lse.dtype == torch.float32 and none is None


# ---- kvcache_keep_accepted on CPU tensors -----------------------------------------------------------------------------------------------

PATHS = {"identity": list(range(64)), "shift_by_one": list(range(1, 64)), "scattered": [0, 5, 6, 40, 63], "none": []}


def _gathered(cache, table, b, start, path):
    """the 64 slots of sequence b after the moves, computed with a torch gather on the sequence's own positions"""
    page = cache.shape[2]
    pos = lambda t: (b, t) if table is None else (int(table[b, t // page]), t % page)
    rows = torch.stack([cache[pos(start + t)[0], :, pos(start + t)[1]] for t in range(64)])          # [64, Hk, D]
    out = rows.clone()
    for i, t in enumerate(path):
        out[i] = rows[t]
    return out, [pos(start + t) for t in range(64)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float8_e4m3fn], ids=["f32", "bf16", "fp8"])
@pytest.mark.parametrize("page", [0, 16], ids=["contiguous", "paged"])
def test_keep_accepted_on_cpu_tensors(dtype, page):
    B, start, cap = len(PATHS), 10, 96
    src = torch.float32 if dtype == torch.float8_e4m3fn else dtype
    _, kc, vc, _, _, table = _problem([1] * B, [start] * B, cap, Hk=2, D=16, dtype=src, page=page, seed=9)
    kc, vc = kc.to(dtype), vc.to(dtype)
    raw = lambda t: t.view(torch.uint8) if dtype == torch.float8_e4m3fn else t
    before = raw(kc).clone(), raw(vc).clone()
    A = 64
    accepted = torch.zeros(B, A, dtype=torch.int32)
    for b, path in enumerate(PATHS.values()):
        accepted[b, :len(path)] = _i32(path)
    num = _i32([len(p) for p in PATHS.values()])
    assert keep(kc, vc, _i32([start] * B), accepted, num, block_table=table) is None
    for cache, old in zip((raw(kc), raw(vc)), before):
        expect = old.clone()
        for b, path in enumerate(PATHS.values()):
            rows, where = _gathered(old, table, b, start, path)
            for t, (blk, slot) in enumerate(where):
                expect[blk, :, slot] = rows[t]
        assert torch.equal(cache, expect)          # the moved rows, and every other byte of the cache unchanged


def test_keep_accepted_refuses_bad_host_tables():
    kc, vc = torch.zeros(2, 2, 96, 16), torch.zeros(2, 2, 96, 16)
    sl, ok, n = _i32([10, 0]), _i32([[0, 2, 5], [1, 2, 3]]), _i32([3, 2])
    assert keep(kc, vc, sl, ok, n) is None
    for acc, num, kind in ((_i32([[0, 2, 2], [1, 2, 3]]), n, ValueError),            # not strictly increasing
                           (_i32([[0, 5, 2], [1, 2, 3]]), n, ValueError),
                           (_i32([[0, 2, 64], [1, 2, 3]]), n, ValueError),           # outside [0, 64)
                           (_i32([[-1, 2, 5], [1, 2, 3]]), n, ValueError),
                           (ok, _i32([4, 2]), ValueError),                           # num_accepted > A
                           (ok, _i32([3, -1]), ValueError),
                           (ok.long(), n, TypeError), (ok, n.long(), TypeError), (ok[0], n, TypeError), (ok, n[:1], TypeError),
                           (torch.zeros(2, 65, dtype=torch.int32), n, ValueError), (torch.zeros(2, 0, dtype=torch.int32), n, ValueError)):
        with pytest.raises(kind):
            keep(kc, vc, sl, acc, num)
    with pytest.raises(ValueError):
        keep(kc, vc[:, :1], sl, ok, n)
    with pytest.raises(TypeError):
        keep(kc, vc, sl.long(), ok, n)
    with pytest.raises(ValueError):
        keep(kc, vc, _i32([10, 97]), ok, n)
    with pytest.raises(ValueError):
        keep(kc[:1], vc[:1], sl, ok, n)


# ---- the visibility probe on the CPU path ---------------------------------------------------------------------------------------------------

PROBES = [(dtype, D, kind) for dtype, D in TC.PROBE_TYPES for kind in ("tree", "bits", "chain")]


@pytest.mark.parametrize("dtype,D,kind", PROBES, ids=[f"{t}_d{d}_{k}" for t, d, k in PROBES])
def test_probe_on_the_cpu_path_and_every_sequence_decidable(dtype, D, kind):
    """The table of the GPU probe (tree_cases.N_B against CACHED) through the CPU path: o and lse are the closed-form counts of
    visibility_probe.expected.  The CPU path computes in float32, so it is probed in float32 (paged for the tree masks), and for the random
    bit sets of the 16-bit cases through an fp8 cache with 16-bit queries, whose keys it normalises in float32 as well.  EVERY (dtype, D,
    sequence) the GPU probes must be decidable for o in the GPU's dtype -- a condition without exceptions: 4 types x 7 non-empty sequences
    x 3 masks."""
    fp8 = kind == "bits" and dtype != "f32"
    comparisons, views = TC.run_probe(dtype if fp8 else "f32", D, 8, 8, kind, "cpu", page=16 if kind == "tree" else 0, fp8=fp8, operand_dtype="f32")
    assert not VP.judge(dtype if fp8 else "f32", f"tree_cpu_{dtype}_d{D}_{kind}", comparisons)
    for b, vis in enumerate(views):
        if TC.N_B[b]:
            assert VP.decidable(vis, dtype, "o", D, 8.0, True), (dtype, D, kind, b)
