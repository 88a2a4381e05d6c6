"""The visibility probe without a GPU (tests/visibility_probe.py): the probe notices every single hidden or leaked pair, the package's
forward-only CPU path passes it on every surface it has (the visibility builders are written from the docstrings of ops.py, so this is an
independent check of cpu.py as well), every GPU case of test_gpu_visibility_probe.py is decidable for single pairs up to a stated cap,
the probe's dense table launches every dense kernel form at 256 CUs (launch recorder), and its bias table every form the golden launch
file shows for a problem with a bias; the bias probe's closed form (d_bias = R dS) against float64 autograd, and its teeth."""
import os
import shutil

import numpy as np
import pytest
import torch

import test_decode_launches_cpu as DL
import test_dispatch_cpu as R
import visibility_probe as VP
import window_cases as W

CAP = 0.10      # the share of (case, quantity) pairs of a table that may be non-decidable: a condition, not a measurement


# ---- 1. the probe itself ---------------------------------------------------------------------------------------------------------------------

SMALL = [(N, M, kind) for N in (1, 5) for M in (1, 15, 16, 17) for kind in ("full", "causal", "mask", "window")]


def _small_vis(N, M, kind):
    if kind == "mask":
        mask = np.ones(M, bool)
        mask[M // 2] = M == 1
        return VP.vis_dense(N, M, mask=mask)
    return VP.vis_dense(N, M, causal=kind == "causal", window=(3, 1) if kind == "window" else (-1, -1))


@pytest.mark.parametrize("l2norm", [True, False], ids=["l2norm", "unit_inputs"])
def test_closed_form_matches_autograd(l2norm):
    """the closed form of `expected` against torch float64 autograd through the l2norm, rows without a visible key included"""
    for D in (16, 32):
        for vis in (VP.vis_dense(7, 20, causal=True), VP.vis_dense(20, 7, causal=True), VP.vis_dense(9, 33, window=(5, 2)),
                    VP.vis_dense(6, 40, mask=VP.key_mask(40, 3)), VP.vis_dense(35, 35, window=(0, 0)), VP.vis_dense(3, D)):
            # (float32's 1 / sqrt(2): the closed form projects with the ROUNDED k^ as the kernels do, autograd with the unit vector -- they
            #  agree to that rounding, 3e-8 here and below every bar in the 16-bit types)
            e, a = VP.expected(vis, D, "f32", 8.0, l2norm), VP.expected_autograd(vis, D, "f32", 8.0, l2norm)
            for name in ("o", "dq", "dk", "dv"):
                assert np.abs(e[name] - a[name]).max() <= 1e-6, (D, vis.shape, name)
                assert (np.abs(e[name]) <= e["mag_" + name] * (1 + 1e-12) + 1e-300).all(), (D, vis.shape, name)
            dead = ~vis.any(1)
            assert (e["o"][dead] == 0).all() and (e["dq"][dead] == 0).all() and np.isneginf(e["lse"][dead]).all()
    assert np.abs(VP.expected(VP.vis_dense(9, 33, window=(5, 2)), 16, "f32")["dq"]).max() > 0.1


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_every_single_pair_flip_moves_o_dq_and_dv(dtype):
    """mutation test: small problems with 1, D - 1, D and D + 1 keys (D = 16); EVERY single-pair flip, hidden or leaked, moves the float64
    expectation of o, of dq and of dv -- each on its own -- by more than 1.5 x its bar.  dq cannot see a flip between no key and one key
    on any input (visibility_probe.decidable); every other flip it must."""
    D = 16
    for N, M, kind in SMALL:
        vis = _small_vis(N, M, kind)
        e0 = VP.expected(vis, D, dtype)
        for i in range(N):
            for j in range(M):
                flipped = vis.copy()
                flipped[i, j] = not flipped[i, j]
                e1 = VP.expected(flipped, D, dtype)
                for q in ("o", "dq", "dv"):
                    if q == "dq" and max(vis[i].sum(), flipped[i].sum()) <= 1:
                        continue
                    moved = np.abs(e1[q] - e0[q]) >= 1.5 * VP.bar(dtype, q) * e0["mag_" + q] + VP.tiny(dtype)
                    assert moved.any(), (N, M, kind, i, j, q)
        for q in ("o", "dq", "dv"):
            assert VP.decidable(vis, dtype, q, D), (N, M, kind, q)


def test_builders_agree_with_each_other():
    """the causal cut is the window (-1, 0); a packed batch and a ragged step are their sequences one by one"""
    for N, M in ((1, 1), (5, 17), (17, 5), (40, 40), (3, 130)):
        assert np.array_equal(VP.vis_causal(N, M), VP.vis_window(N, M, -1, 0))
        assert np.array_equal(VP.vis_dense(N, M, causal=True, window=(4, 7)), VP.vis_window(N, M, 4, 0))
        assert np.array_equal(VP.vis_dense(N, M, causal=True), VP.vis_cache(N, M - 2, 2, causal=True))
        i, j = np.arange(N)[:, None], np.arange(M)[None, :]
        assert np.array_equal(VP.vis_causal(N, M), j - (M - N) <= i)
    lq, lk = [0, 3, 9], [4, 0, 20]
    for got, (n, m) in zip(VP.vis_spans(lq, lk, True, (5, 0)), zip(lq, lk)):
        assert got.shape == (n, m) and np.array_equal(got, VP.vis_dense(n, m, True, (5, 0)))
    for append in (True, False):
        for got, n, c in zip(VP.vis_ragged([1, 0, 5], [0, 7, 3], append, True), [1, 0, 5], [0, 7, 3]):
            assert np.array_equal(got, VP.vis_dense(n, c + (n if append else 0), True))
    assert VP.vis_shared_prefix(3, VP.vis_causal(2, 1)).tolist() == [[True, True, True, False], [True, True, True, True]]


def test_decidable_knows_its_limit():
    """8 significant bits cannot separate one key among thousands: the limit the decidability test below counts"""
    assert VP.decidable(VP.vis_dense(4, 300, causal=True), "bf16", "o", 16)
    assert not VP.decidable(VP.vis_dense(4, 3000, causal=True), "bf16", "o", 16)
    assert VP.decidable(VP.vis_dense(4, 3000, causal=True), "f32", "o", 16)
    assert not VP.decidable(VP.vis_dense(4, 3000, causal=True), "bf16", "dq", 64)


def test_check_refuses_a_wrong_pair():
    """the comparison side: the float64 expectation of a problem with one pair flipped fails `check` against the right one in every dtype,
    and a value that should be exactly 0 may not be anything else"""
    vis = VP.vis_dense(40, 300, causal=True)
    wrong = vis.copy()
    wrong[17, 277] = False
    for dtype in ("bf16", "f16", "f32"):
        e0, e1 = VP.expected(vis, 64, dtype), VP.expected(wrong, 64, dtype)
        for q in ("o", "dq", "dv"):
            assert VP.check(dtype, torch.from_numpy(e0[q]), e0[q], "self", q, e0["mag_" + q])[0]
            assert not VP.check(dtype, torch.from_numpy(e1[q]), e0[q], "flip", q, e0["mag_" + q])[0], (dtype, q)
        few = VP.expected(VP.vis_dense(40, 40, causal=True), 64, dtype)["o"]
        leak = few.copy()
        leak[0, 63] = 1e-3
        assert few[0, 63] == 0 and not VP.check(dtype, torch.from_numpy(leak), few, "leak", "o")[0]
        lse = e0["lse"].copy()
        assert VP.check_lse(dtype, torch.from_numpy(lse), e0["lse"], "self")[0]
        lse[3] = np.log(np.exp(lse[3]) * (1 + 1.0 / e0["cnt"][3]))             # one key more
        assert not VP.check_lse(dtype, torch.from_numpy(lse), e0["lse"], "count")[0]


# ---- 1b. the bias probe: closed form, teeth --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("l2norm", [True, False], ids=["l2norm", "unit_inputs"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_bias_closed_form_matches_autograd(causal, l2norm):
    """o, dq, dk, dv and d_bias = dS of `expected` over (bias pattern & geometry) against torch float64 autograd with the bias (-inf / a
    per-row constant) as a leaf added to the logits, at 1e-12; no NaN comes out of the -inf entries.  (With the l2norm, dk of the closed
    form projects with the ROUNDED k^ as the kernels do: it agrees to that rounding, as in test_closed_form_matches_autograd.)"""
    D = 16
    for N, M in ((20, 37), (37, 20), (33, 33), (5, 70)):
        pattern = VP.bias_vis(3, N, M, D, causal, N + M)
        bias = VP.bias_values(pattern, VP.bias_rows(3, N, N + M))
        geom = VP.vis_dense(N, M, causal)
        for s in range(3):
            e = VP.expected(pattern[s] & geom, D, "f32", 8.0, l2norm)
            a = VP.expected_autograd(geom, D, "f32", 8.0, l2norm, bias=bias[s])
            assert all(np.isfinite(x).all() for x in a.values())
            for name, ref in (("o", "o"), ("dq", "dq"), ("dk", "dk"), ("dv", "dv"), ("ds", "d_bias")):
                tol = 1e-6 if name == "dk" and l2norm else 1e-12
                assert np.abs(e[name] - a[ref]).max() <= tol, (N, M, s, name)
            assert (np.abs(e["ds"]) <= e["mag_ds"] * (1 + 1e-12)).all() and (e["ds"][~(pattern[s] & geom)] == 0).all()
            assert (a["d_bias"][~(pattern[s] & geom)] == 0).all()
    assert np.abs(e["ds"]).max() > 1e-3


def _teeth_case(dtype, causal):
    return (f"teeth_{dtype}_{'causal' if causal else 'full'}", dtype, 64, 2, 3, 3, 140, 200, "causal_n<m" if causal else "plain", dict(), False, False, False)


def _rounded(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(VP.DT[dtype]).double()


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_check_refuses_a_wrong_bias(dtype):
    """teeth: a "result" that is the float64 expectation of a wrongly read bias, rounded to the dtype, fails `check` for o AND for d_bias:
    the bias rolled by one column, by one row, the next slice's pattern, the two 16-key halves of one 32-key block swapped in one row, a
    single pair flipped at column M - 1, at the first column of the last 64-key tile and in row N - 1; under causal a pair flipped on
    the diagonal and a pair leaked one above it (the geometry's own off-by-one: there the mutation is of the effective visibility).
    For d_bias alone: one value moved to the neighbouring column, a non-zero value at a hidden pair, and the zeros of a 64-key tile above
    the causal diagonal extended one tile to the left."""
    N, M = 140, 200
    for causal in (False, True):
        case = _teeth_case(dtype, causal)
        eff, pattern, geom, _, _ = VP.bias_case_vis(case)
        e0 = VP.bias_expected(case, eff)
        for q in ("o", "d_bias"):
            assert VP.check(dtype, _rounded(e0[q], dtype), e0[q], "self", "o" if q == "o" else "dbias", e0["mag_" + q])[0]

        def single(i, j, of=None):
            x = (pattern if of is None else of).copy()
            x[0, i, j] = not x[0, i, j]
            return x

        diff, i0 = M - N, N - 5
        swapped = pattern.copy()
        swapped[0, i0, 64:80], swapped[0, i0, 80:96] = pattern[0, i0, 80:96], pattern[0, i0, 64:80]
        assert not np.array_equal(swapped[0, i0], pattern[0, i0])
        mutants = {"column": np.roll(pattern, 1, axis=2) & geom[None], "row": np.roll(pattern, 1, axis=1) & geom[None],
                   "slice": np.roll(pattern, -1, axis=0) & geom[None], "halves": swapped & geom[None],
                   "last_row": single(N - 1, 100) & geom[None]}
        if causal:
            mutants["diagonal"] = single(70, 70 + diff) & geom[None]
            mutants["above_diagonal"] = single(70, 71 + diff, of=eff)
            assert not geom[70, 71 + diff] and mutants["above_diagonal"][0, 70, 71 + diff]
        else:
            mutants["last_column"] = single(77, M - 1) & geom[None]
            mutants["last_tile"] = single(77, (M - 1) // 64 * 64) & geom[None]
        for label, wrong in mutants.items():
            assert not np.array_equal(wrong, eff), label
            e1 = VP.bias_expected(case, wrong, g=e0["g"])
            for q in ("o", "d_bias"):
                ok = VP.check(dtype, _rounded(e1[q], dtype), e0[q], label, "o" if q == "o" else "dbias", e0["mag_" + q])[0]
                assert not ok, (dtype, causal, label, q)
        # d_bias alone
        ref = e0["d_bias"]
        i, j = next((i, j) for i in range(60, N) for j in range(1, diff + i if causal else M - 1) if ref[0, i, j] != 0 and ref[0, i, j + 1] == 0)
        moved = ref.copy()
        moved[0, i, j], moved[0, i, j + 1] = 0.0, ref[0, i, j]
        leak = ref.copy()
        leak[0, i, j + 1] = np.abs(ref[ref != 0]).min()
        wrongs = {"moved": moved, "hidden": leak}
        if causal:
            j0 = next(j for j in range(0, M, 64) if j > 127 + diff)                 # the first skipped key tile of the first 128-row tile
            early = ref.copy()
            early[:, :128, j0 - 64:j0] = 0.0
            assert np.abs(ref[:, :128, j0 - 64:j0]).max() > 0
            wrongs["tile_skip"] = early
        for label, wrong in wrongs.items():
            assert not VP.check(dtype, _rounded(wrong, dtype), ref, label, "dbias", e0["mag_d_bias"])[0], (dtype, causal, label)


# ---- 2. cpu.py on every surface, float32 -----------------------------------------------------------------------------------------------------

def _ok(name, comparisons, dtype="f32"):
    fails = VP.judge(dtype, name, comparisons)
    assert not fails, (name, fails)


@pytest.mark.parametrize("N,M,causal,window,masked", [
    (40, 70, False, None, True), (33, 129, True, None, False), (129, 33, True, None, False), (64, 64, True, None, False),
    (70, 70, False, (5, 0), False), (40, 90, False, (17, 3), False), (90, 40, True, (200, 0), False), (50, 50, False, (-1, 2), False),
    (50, 50, False, (0, -1), False), (30, 60, False, (0, 0), False)])
def test_cpu_path_dense_and_local(N, M, causal, window, masked):
    D = (16, 32, 64)[(N + M) % 3]
    mask = VP.key_mask(M, N) if masked else None
    for scale, l2 in ((8.0, True), (80.0, True), (1.0, False)):
        _ok(f"cpu_dense_n{N}m{M}", VP.run_dense("f32", D, 2, 4, (4, 2, 1)[N % 3], N, M, scale, l2, "cpu", causal, window, mask, seed=N, grads=False))


CPU_BIAS = [("cpu_bias_plain", "f32", 32, 2, 4, 2, 129, 257, "plain", dict(), False, False, False),
            ("cpu_bias_causal_perbatch", "f32", 64, 2, 4, 1, 127, 132, "causal_n<m", dict(scale=80.0), True, False, False),
            ("cpu_bias_causal_tall", "f32", 16, 2, 4, 4, 260, 127, "causal_n>m", dict(), False, True, False),
            ("cpu_bias_mask", "f32", 32, 1, 8, 2, 33, 128, "mask", dict(l2norm_qk=False, scale=1.0), False, False, True)]


@pytest.mark.parametrize("case", CPU_BIAS, ids=[c[0] for c in CPU_BIAS])
def test_cpu_path_bias(case):
    """attn_bias of -inf / per-row constants on BIAS_CASES-style shapes (per-head and per-batch, causal at both signs of M - N, a key
    mask, the offsets variant, a view one element into a buffer): o at its bar"""
    _ok(case[0], VP.run_dense_bias(case, "cpu", grads=False)[0])


@pytest.mark.parametrize("causal,window", [(False, (-1, -1)), (True, (-1, -1)), (True, (6, 0)), (False, (3, 4)), (False, (40, -1))])
def test_cpu_path_varlen(causal, window):
    lq, lk = [0, 1, 7, 33, 64, 20, 5], [5, 9, 0, 31, 64, 70, 1]
    _ok("cpu_varlen", VP.run_packed("f32", 32, 4, 2, lq, lk, 8.0, True, "cpu", causal, window, seed=3, grads=False))


@pytest.mark.parametrize("page", [0, 16])
@pytest.mark.parametrize("N,n_new,causal,window", [(1, 0, False, (-1, -1)), (5, 5, True, (-1, -1)), (17, 1, True, (-1, -1)), (5, 0, False, (7, 2)),
                                                   (3, 3, True, (20, 0))])
def test_cpu_path_kvcache(page, N, n_new, causal, window):
    lens = [0, 1, 15, 17, 64 - n_new]
    _ok("cpu_kvcache", VP.run_decode("f32", 32, 4, 2, N, 64, page, lens, n_new, None, causal, False, 8.0, True, "cpu", window, seed=N))


@pytest.mark.parametrize("page,append,causal,window", [(0, True, True, (-1, -1)), (16, False, True, (-1, -1)), (16, True, False, (9, 0)), (0, False, False, (-1, -1))])
def test_cpu_path_ragged_kvcache(page, append, causal, window):
    _ok("cpu_ragged", VP.run_decode("f32", 16, 8, 2, 0, 64, page, [0, 15, 17, 40, 1], 0, [1, 0, 5, 17, 3], causal, False, 8.0, True, "cpu", window, append, seed=5))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("page,counts", [(0, None), (16, None), (16, [1, 0, 5, 17, 3])])
def test_cpu_path_fp8_cache(dtype, page, counts):
    """the CPU path dequantises to float32 and normalises there, so its logit is float32's; o is rounded to the 16-bit q dtype"""
    got = VP.run_decode(dtype, 32, 4, 2, 5, 64, page, [0, 1, 15, 17, 40], 5, counts, True, True, 8.0, True, "cpu", seed=7, operand_dtype="f32")
    _ok("cpu_fp8", got, dtype)


@pytest.mark.parametrize("case", VP.PREFIX_CASES[::2], ids=[c[0] for c in VP.PREFIX_CASES[::2]])
def test_cpu_path_shared_prefix(case):
    _ok(case[0], VP.run_prefix("f32", *case[2:], "cpu"))


@pytest.mark.parametrize("cut", [1, 16, 38])
def test_cpu_path_merge_attention_states(cut):
    """one attention over two cache calls on disjoint key ranges, merged: the expectation of the whole (cut <= L - N + 1: under causal
    every query sees the whole first part)"""
    import flash_cosine_sim_attention_amd as F
    D, H, Hk, N, L = 32, 4, 2, 3, 40
    kc, vc, _ = VP._cache("f32", D, 1, Hk, L, 0, [L], True, 11)
    q, _, _ = VP.probe_queries("f32", (1, H), N, D, True, 12)
    os, lses = zip(*(F.flash_cosine_sim_attention_with_kvcache(q, kc[:, :, lo:hi], vc[:, :, lo:hi], causal=last, return_lse=True)
                     for lo, hi, last in ((0, cut, False), (cut, L, True))))
    o, lse = F.merge_attention_states(os, lses)
    e = VP.expected(VP.vis_cache(N, L, 0, causal=True), D, "f32", grads=False)
    _ok("cpu_merge", [("o", "merge", o, e["o"], e["o"]), ("lse", "merge", lse, e["lse"], None)])


# ---- 3. decidability of every GPU case -------------------------------------------------------------------------------------------------------

def _table_report(table, rows):
    """rows: (case name, quantity, decidable).  Prints the non-decidable pairs and asserts the cap."""
    bad = [(n, q) for n, q, ok in rows if not ok]
    print(f"{table}: {len(bad)} of {len(rows)} (case, quantity) pairs are not decidable for single pairs")
    for n, q in bad:
        print(f"  {table} {n} {q}")
    assert len(bad) <= CAP * len(rows), (table, len(bad), len(rows), bad[:10])
    return bad


def _dense_rows(cases, vis_of, quantities=lambda case: ("o", "dq", "dv")):
    rows = []
    for case in cases:
        name, dtype, D = case[:3]
        vis, scale, l2 = vis_of(case)
        rows += [(name, q, VP.decidable(vis, dtype, q, D, scale, l2, seed=len(name))) for q in quantities(case)]
    return rows


def window_dense_rows():
    return _dense_rows(W.DENSE_CASES, lambda c: (VP.vis_dense(c[6], c[7], c[10].get("causal", False), (c[8], c[9])), *VP.probe_scale(c[10])))


def dense_plain_rows():
    return _dense_rows(VP.DENSE_PLAIN_CASES, lambda c: (VP.dense_plain_vis(c)[0], *VP.probe_scale(c[9])),
                       lambda c: ("o", "dq", "dv") if c[12] else ("o",))      # (forward-only cases)


def packed_rows():
    rows, memo = [], {}
    for name, dtype, D, lq, lk, H, Hk, mx, kw, window in VP.packed_cases():
        scale, l2 = VP.probe_scale(kw)
        for q in ("o", "dq", "dv"):
            ok = True
            for n, m in sorted(set(zip(lq, lk))):
                key = (dtype, D, n, m, scale, l2, kw.get("causal", False), window, q)
                if n and m and key not in memo:
                    memo[key] = VP.decidable(VP.vis_dense(n, m, kw.get("causal", False), window), dtype, q, D, scale, l2, seed=n + m)
                ok &= memo.get(key, True)
            rows.append((name, q, ok))
    return rows


def decode_rows():
    rows = []
    for name, dtype, D, H, Hk, N, cap, page, lens, n_new, counts, causal, fp8, kw, window in VP.decode_cases():
        scale, l2 = VP.probe_scale(kw)
        per = counts if counts is not None else [N] * len(lens)
        new = [n if kw.get("append", True) else 0 for n in per] if counts is not None else [n_new] * len(lens)
        ok = all(VP.decidable(VP.vis_cache(n, c, a, causal, window, cap), dtype, "o", D, scale, l2, seed=c) for n, c, a in zip(per, lens, new) if n)
        rows.append((name, "o", ok))
    return rows


def prefix_rows():
    rows = []
    for name, dtype, D, H, Hk, N, counts, cached, append, P, paged, causal in VP.PREFIX_CASES:
        per = counts if counts is not None else [N] * len(cached)
        ok = True
        for n, c in zip(per, cached):
            if n:
                vis = VP.vis_shared_prefix(P, VP.vis_cache(n, c, n if append else 0, causal))
                ok &= VP.decidable(vis, dtype, "o", D, seed=c)
        rows.append((name, "o", ok))
    return rows


def bias_rows():
    """o and dv of the first and the last slice of every bias case (dq makes no single-pair claim on this table: visibility_probe.
    _bias_cases; d_bias decides every pair by construction: test_bias_cases_separate_every_d_bias_element_from_zero)"""
    rows = []
    for case in VP.BIAS_CASES:
        name, dtype, D = case[:3]
        eff = VP.bias_case_vis(case)[0]
        scale, l2 = VP.probe_scale(case[9])
        rows += [(name, q, all(VP.decidable(eff[s], dtype, q, D, scale, l2, seed=len(name) + s) for s in (0, len(eff) - 1))) for q in ("o", "dv")]
    return rows


TABLES = {"window_dense": window_dense_rows, "dense_plain": dense_plain_rows, "packed": packed_rows, "decode": decode_rows, "prefix": prefix_rows,
          "bias": bias_rows}


@pytest.mark.parametrize("table", sorted(TABLES))
def test_gpu_cases_are_decidable_up_to_the_cap(table):
    """Every GPU case of test_gpu_visibility_probe.py: a sampled single-pair flip at a visibility boundary moves the expectation of o, of dq
    and of dv (decode and prefix calls: o) by >= 1.5 x the bar.  At most 10 % of a table's (case, quantity) pairs may fail that: bf16 at
    D = 16 / 32 whose rows see more than ~20 (D - 1) keys, rows at a band's corner that see no key of their own class (dS = 0 there), and
    -- dq under a key mask -- the rare flip of a key that shares its feature 1 + j % (D - 1) with the row's diagonal key, whose term is
    cnt times larger.  Those pairs are still compared at the bar on the GPU; only the single-pair
    claim is dropped for them.  The list is printed (and recorded in profiles/visibility_probe_margins.txt)."""
    _table_report(table, TABLES[table]())


def test_bias_cases_separate_every_d_bias_element_from_zero():
    """d_bias decides every single pair of the bias table: the element of a flipped pair moves between exactly 0 (expectation and mag 0:
    the kernel must write 0 up to tiny) and a value whose size is at least 16 tiny -- after the power-of-two factor on do in float16.  Also
    what the table promises about itself: sizes, the key lengths of every read and write path, the variants and regimes."""
    for case in VP.BIAS_CASES:
        name, dtype, D, B, H, Hk, N, M = case[:8]
        eff, pattern, geom = VP.bias_case_vis(case)[:3]
        e = VP.bias_expected(case, eff)
        ref = e["d_bias"]
        assert (ref[~eff] == 0).all() and (e["mag_d_bias"][~eff] == 0).all(), name
        # (a visible pair whose dS is exactly 0 -- a row of keys of one class only -- says nothing; there must be few)
        assert (ref[eff] != 0).mean() > 0.99, (name, (ref[eff] != 0).mean())
        assert np.abs(ref[ref != 0]).min() >= 16 * VP.tiny(dtype), (name, np.abs(ref[ref != 0]).min())
        assert np.abs(ref).max() * 4 < torch.finfo(VP.DT[dtype]).max and e["g"] == 2.0 ** round(np.log2(e["g"])), name
        assert N * M <= 620_000 and len(eff) <= 30, name
        live = geom.any(1)
        cls = (np.arange(N) + M - N) % D
        own = eff & (np.arange(M)[None, None, :] % D == cls[None, :, None])
        can = (geom & (np.arange(M)[None, :] % D == cls[:, None])).any(1)
        assert own.any(2)[:, live & can].all(), name
        assert not np.array_equal(eff[0], eff[-1]) or len(eff) == 1, name
    table = VP.BIAS_CASES
    assert {(c[1], c[2]) for c in table} >= set(VP.BIAS_TYPES)
    keys = {c[7] for c in table}
    assert {128, 256, 1104, 132, 260, 1100, 127, 257, 31, 33} <= keys and any(c[6] % 32 for c in table)
    assert set(VP.LENGTHS) <= {c[6] for c in table} | keys
    for dtype, D in VP.BIAS_TYPES:
        assert {c[8] for c in table if (c[1], c[2]) == (dtype, D)} >= set(VP.BIAS_VARIANTS), (dtype, D)
        assert any(c[10] for c in table if (c[1], c[2]) == (dtype, D)) and any(not c[10] for c in table if (c[1], c[2]) == (dtype, D))
    mis = [c for c in table if c[12]]
    assert {c[1] == "f32" for c in mis} == {True, False} and all(c[7] % 8 == 0 for c in mis)
    assert any(c[1] == "bf16" and c[9].get("scale") == 80.0 for c in table) and any(c[9].get("l2norm_qk") is False for c in table)
    assert {c[5] for c in table if c[4] == 8} >= {1, 2, 8}
    for dtype in ("bf16", "f16", "f32"):
        assert any(c[11] and c[1] == dtype and (c[0][:-len("_offsets")],) == (d[0],) for c in table for d in table), dtype


# ---- 4. the dense table reaches every dense form (launch recorder, 256 CUs) ----------------------------------------------------------------

def forms(line):
    """the forms of fcsa_dispatch.h a recorded dense line launched, from the kernels' template arguments (fwd_kernel<T, D, NW, BIAS, DYN, LEAN,
    KM, KSPLIT>, bwd_dq_kernel<T, D, NW, BIAS, SUB, TWO, KM, KSPLIT>, bwd_dkv_kernel<T, D, NW, BMQ, BIAS, LEAN, KM, RING, QSPLIT, SWEEP>) and
    the split counts of the launch ("s<forward>" / "s<dq>,<dkv>")"""
    out = set()
    fields = line.split()
    hk, h = int(fields[5]), int(fields[4])
    for part in line.split(" |", 1)[1].replace(" | ", "; ").split(";"):
        p = part.split()
        if not p or "<" not in p[0]:
            continue
        kernel, args = p[0].split("<")
        a = args.rstrip(">").split(",")
        if kernel == "fwd3":
            out.add("fwd:Fwd3")
        elif kernel == "fwd2":
            out.add("fwd:Fwd2")
        elif kernel == "fwd":
            nw, lean, ksplit = int(a[2]), a[5] == "1", a[7] == "1"
            wide = int(a[1]) * (4 if a[0] == "f" else 2) > 128
            out.add("fwd:" + ("KSplit8" if ksplit else "Waves4" if nw == 4 else "Lean8" if wide and lean else "Rows8"))
            if int(p[4].lstrip("s")) > 1:
                out.add("fwd:split-key")
            if a[1] == "128" and a[0] != "f" and wide and lean and not ksplit and fields[16] == "0":
                out.add("fwd:Lean8-in-place-of-Fwd3")
        elif kernel == "bwd_dq":
            nw, two, ksplit = int(a[2]), a[5] == "1", a[7] == "1"
            wide = int(a[1]) * (4 if a[0] == "f" else 2) > 128
            out.add("dq:" + ("KSplit8" if ksplit else "Waves8" if nw == 8 else "Waves4Two" if two and wide else "Waves4"))
            if int(p[4].lstrip("s").split(",")[0]) > 1:
                out.add("dq:split-key")
        elif kernel == "bwd_dkv":
            nw, lean, qsplit, sweep = int(a[2]), a[5] == "1", a[8] == "1", a[9] == "1"
            out.add("dkv:" + ("Sweep" if sweep else "QSplit8" if qsplit else "Lean8" if lean and nw == 8 else "Waves8" if nw == 8 else "Waves4"))
            if int(p[4].split(",")[1]) > 1:
                out.add("dkv:split-query")
            if 1 < hk < h and not sweep:
                out.add("dkv:group-slabs")
            if hk == 1 and h > 1:
                out.add("dkv:single-headed")
    return out


DENSE_FORMS = {"fwd:Waves4", "fwd:Rows8", "fwd:Lean8", "fwd:KSplit8", "fwd:Fwd2", "fwd:Fwd3", "fwd:Lean8-in-place-of-Fwd3", "fwd:split-key",
               "dq:Waves4", "dq:Waves4Two", "dq:Waves8", "dq:KSplit8", "dq:split-key",
               "dkv:Waves4", "dkv:Waves8", "dkv:Lean8", "dkv:QSplit8", "dkv:Sweep", "dkv:split-query", "dkv:group-slabs", "dkv:single-headed"}
# what a form cannot take, by the rules of fcsa_dispatch.h: fwd3_applies / fwd2_applies refuse a key mask (and under one the lean form is
# simply Lean8); a causal split-query dK/dV needs >= 1024 of BOTH queries and keys (best_split over min(N, M) with >= 512 per split), so its
# cases have N = M +- 1 and the few-tile grids of the split-key launches (forward, dQ) need far more keys than queries
NO_MASK = {"fwd:Fwd2", "fwd:Fwd3", "fwd:Lean8-in-place-of-Fwd3"}


def dense_plain_recorder_line(case, cus=256):
    """the launch recorder's input line of the probe's copy of a case (groups = 1, scale * groups)"""
    name, dtype, D, B, H, Hk, N, M, variant, kw, ff, kf, grads = case
    scale, l2 = VP.probe_scale(kw)
    return R.line(cus, W.DTYPE_CODE[dtype], D, B, H, Hk, N, M, int(variant.startswith("causal")), int(variant == "mask"), 0, int(l2), 1, scale,
                  ff=ff, kf=kf)


def test_forms_names_every_enumerator_of_the_dispatch():
    """DENSE_FORMS holds every FwdForm / DqForm / DkvForm of fcsa_dispatch.h, so a new form cannot stay outside the table unnoticed"""
    import re
    text = open(os.path.join(R.ROOT, "flash_cosine_sim_attention_amd", "csrc", "fcsa_dispatch.h")).read()
    for enum, prefix in (("FwdForm", "fwd"), ("DqForm", "dq"), ("DkvForm", "dkv")):
        names = [n.strip() for n in re.search(r"enum class %s \{([^}]*)\}" % enum, text).group(1).split(",")]
        assert len(names) >= 4 and {f"{prefix}:{n}" for n in names} <= DENSE_FORMS, (enum, names)


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"), reason="needs g++ and the HIP headers")
def test_dense_probe_table_launches_every_dense_form(tmp_path):
    """the probe's dense table at 256 CUs: every forward, dQ and dK/dV form the dispatch can give a dense problem without a bias, under a
    key mask, under causal at N < M and under causal at N > M -- each on its own, but for what a form cannot take (NO_MASK above) -- with
    the debug knobs the GPU test sets (the recorder sets them per line, so nothing is left changed)"""
    assert os.path.exists(R.LIB), "libfcsa_hip.so is not built"
    log = R.record(R.build_recorder(tmp_path), R.LIB, [dense_plain_recorder_line(c) for c in VP.DENSE_PLAIN_CASES]).splitlines()
    assert len(log) == len(VP.DENSE_PLAIN_CASES) and not any(" rc " in ln for ln in log)
    seen = {"mask": set(), "causal_n<m": set(), "causal_n>m": set(), "plain": set()}
    for case, ln in zip(VP.DENSE_PLAIN_CASES, log):
        assert (case[6] < case[7]) == (case[8] != "causal_n>m") or not case[8].startswith("causal"), case[0]
        seen[case[8]] |= forms(ln)
    assert DENSE_FORMS - NO_MASK <= seen["mask"], sorted(DENSE_FORMS - NO_MASK - seen["mask"])
    assert NO_MASK <= seen["plain"], sorted(NO_MASK - seen["plain"])
    for side in ("causal_n<m", "causal_n>m"):
        assert DENSE_FORMS <= seen[side], (side, sorted(DENSE_FORMS - seen[side]))


def bias_recorder_line(case, cus=256):
    """the launch recorder's input line of a BIAS_CASES entry: bias field 1 for a per-head bias, 2 for a per-batch one"""
    name, dtype, D, B, H, Hk, N, M, variant, kw, batch = case[:11]
    scale, l2 = VP.probe_scale(kw)
    return R.line(cus, W.DTYPE_CODE[dtype], D, B, H, Hk, N, M, int(variant.startswith("causal")), int(variant == "mask"), 2 if batch else 1, int(l2), 1,
                  scale)


def golden_bias_forms(cus=256):
    """{form label: set of "full" / "causal"} over the dense lines of the golden file that carry a bias at `cus` CUs"""
    out = {}
    for ln in open(R.GOLDEN):
        f = ln.split(" |", 1)[0].split()
        if "varlen" in f or int(f[0]) != cus or f[10] == "0":
            continue
        for label in forms(ln):
            out.setdefault(label, set()).add("causal" if f[8] == "1" else "full")
    return out


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"), reason="needs g++ and the HIP headers")
def test_bias_probe_table_launches_every_form_a_bias_can_take(tmp_path):
    """the bias table at 256 CUs against the golden file: every form label any bias line of tests/golden/dispatch_launches.txt launches
    at 256 CUs is launched by the table -- with a bias alone, with a key mask, and, where the golden file shows the label under causal at
    all, under causal at N < M and at N > M (the split-key dQ launch it shows without causal only: with a bias the dispatch gives it to no
    causal problem of a size this table allows) -- and by a per-batch bias at least once per kernel; every (dtype, D) launches bwd_dbias
    per-head and per-batch, every case launches it"""
    assert os.path.exists(R.LIB), "libfcsa_hip.so is not built"
    want = golden_bias_forms()
    assert {"fwd:Rows8", "fwd:KSplit8", "fwd:Waves4", "dq:Waves8", "dq:KSplit8", "dq:Waves4", "dq:split-key", "dkv:QSplit8"} <= set(want), sorted(want)
    log = R.record(R.build_recorder(tmp_path), R.LIB, [bias_recorder_line(c) for c in VP.BIAS_CASES]).splitlines()
    assert len(log) == len(VP.BIAS_CASES) and not any(" rc " in ln for ln in log)
    seen = {v: set() for v in VP.BIAS_VARIANTS}
    per_batch, dbias = set(), set()
    for case, ln in zip(VP.BIAS_CASES, log):
        name, dtype, D, B, H, Hk, N, M, variant = case[:9]
        assert (N < M) == (variant != "causal_n>m") or not variant.startswith("causal"), name
        seen[variant] |= forms(ln)
        assert f"bwd_dbias<{dict(f32='f', f16='h', bf16='b')[dtype]},{D}>" in ln, name
        dbias.add((dtype, D, case[10]))
        if case[10]:
            per_batch |= forms(ln)
    for label, where in sorted(want.items()):
        for variant in VP.BIAS_VARIANTS:
            if variant.startswith("causal") and "causal" not in where:
                continue
            assert label in seen[variant], (label, variant)
    assert {lb.split(":")[0] for lb in per_batch} == {"fwd", "dq", "dkv"}, sorted(per_batch)
    for dtype, D in VP.BIAS_TYPES:
        assert {(dtype, D, False), (dtype, D, True)} <= dbias, (dtype, D)
    assert {"dkv:group-slabs", "dkv:single-headed"} <= seen["plain"] | seen["mask"] | seen["causal_n<m"] | seen["causal_n>m"]


# ---- 5. the decode table launches what its docstrings say (decode launch recorder, 256 CUs) -------------------------------------------------

@pytest.mark.skipif(shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"), reason="needs g++ and the HIP headers")
def test_decode_probe_table_launches_every_launcher_and_sixteen_splits(tmp_path):
    """every non-windowed decode case through fcsa_forward_kvcache_lse as the Python call makes it (max_seqlen_k = the capacity): the three
    launchers of the shared host path (decode / decode_fp8 / decode_ragged[_fp8]) with their appends and LSE combines, and the many-splits
    cases at 16 splits of 128 keys, so that the second sequence's length 2035 (2034 + 1) ends inside the last split's last 32-key block"""
    assert os.path.exists(R.LIB), "libfcsa_hip.so is not built"
    lines = []
    for name, dtype, D, H, Hk, N, cap, page, lens, n_new, counts, causal, fp8, kw in VP.DECODE_PLAIN_CASES:
        scale, l2 = VP.probe_scale(kw)
        ragged = counts is not None
        new = int(kw.get("append", True)) if ragged else n_new
        lines.append(DL.call(W.DTYPE_CODE[dtype], D, len(lens), H, Hk, max(counts) if ragged else N, cap, cap, page, new, int(causal), int(l2), 1, scale,
                             fp8=int(fp8), ragged=sum(counts) if ragged else None, lse=1))
    blocks = R.record(DL.build_recorder(tmp_path), R.LIB, lines).split("\n256 ")
    assert len(blocks) == len(lines) and not any("\n  rc " in b for b in blocks)
    kernels = set()
    for case, block in zip(VP.DECODE_PLAIN_CASES, blocks):
        names = [ln.split()[1].split("<")[0] for ln in block.splitlines()[1:]]
        kernels |= set(names)
        fp8, ragged, appends = case[12], case[10] is not None, (case[13].get("append", True) if case[10] is not None else case[9] > 0)
        tail = ("_ragged" if ragged else "") + ("_fp8" if fp8 else "")
        want = (["kv_append" + (tail if not (ragged and fp8) else "_ragged")] if appends else []) + ["decode" + tail, "decode_combine_lse" + (("_ragged" if ragged else "_fp8" if fp8 else ""))]
        assert names == want, (case[0], names, want)
        splits = {int(f.split("=")[1]) for f in block.split() if f.startswith("splits=")}
        assert len(splits) == 1, case[0]
        if "splits" in case[0]:
            assert splits == {16} and case[6] == 2048 and min(case[8]) + case[9] == 2035 and 2035 % 32, (case[0], splits)
    assert {"decode", "decode_fp8", "decode_ragged", "decode_ragged_fp8", "kv_append", "kv_append_fp8", "kv_append_ragged", "decode_combine_lse",
            "decode_combine_lse_fp8", "decode_combine_lse_ragged"} <= kernels, sorted(kernels)
