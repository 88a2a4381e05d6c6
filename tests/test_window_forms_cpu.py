"""Every windowed kernel instantiation a sliding-window call can reach is launched by the GPU parity table -- checked without a GPU by a
launch recorder with a window field (tests/native/window_launch_recorder.cpp: the stub HIP runtime of launch_recorder.cpp under its own
driver).  The reachable set is what a sweep over dtype x head dim x grid size x shift regime launches at 256 CUs; the share of it the
table of tests/window_cases.py (test_gpu_window.py runs it against the float64 oracle) may leave out is zero."""
import itertools
import os
import shutil
import subprocess

import pytest

import test_dispatch_cpu as R
import window_cases as W

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"), reason="needs g++ and the HIP headers")

WIN = ("fwd_win<", "bwd_dq_win<", "bwd_dkv_win<")
DECODE_WIN = "decode_win<"


@pytest.fixture(scope="module")
def recorder(tmp_path_factory):
    assert os.path.exists(R.LIB), "libfcsa_hip.so is not built"
    exe = os.path.join(str(tmp_path_factory.mktemp("window_recorder")), "window_launch_recorder")
    cmd = ["g++", "-O1", "-std=c++17", "-rdynamic", "-D__HIP_PLATFORM_AMD__=1", "-I/opt/rocm/include",
           "-I" + os.path.join(R.ROOT, "flash_cosine_sim_attention_amd", "csrc"),
           os.path.join(R.ROOT, "tests", "native", "window_launch_recorder.cpp"), "-o", exe, "-ldl"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    return exe


def launches(line):
    assert " rc " not in line, line
    parts = line.split(" |", 1)[1].replace(" | ", "; ").split(";")
    return [p.split() for p in (x.strip() for x in parts) if p and not p.startswith("ws ")]


def launched(log):
    """{kernel instantiation: the first recorded line that launches it}"""
    out = {}
    for ln in log.splitlines():
        for part in launches(ln):
            out.setdefault(part[0], ln)
    return out


def reachable_grid():
    """batch x heads on both sides of every threshold of tile_waves / choose_* (7/8 of the CUs, the CU count, a last round filled up to /
    beyond 55 %), one / two / five pairs of 128-row tiles, both shift regimes"""
    for dtype, D, bh, L, per_row in itertools.product(W.DTYPES, W.DIMS, (1, 8, 64, 100, 128, 129, 150, 223, 224, 240, 256, 257, 300, 396, 400, 512),
                                                      (300, 600, 1100), (False, True)):
        kw = W.per_row_kwargs(dtype, 0) if per_row else {}
        yield W.recorder_line(dtype, D, 1, bh, bh, L, L, 100, 0, dict(kw, causal=True))


def test_window_cases_launch_every_reachable_windowed_instantiation(recorder):
    reachable = {k: v for k, v in launched(R.record(recorder, R.LIB, list(reachable_grid()))).items() if k.startswith(WIN)}
    assert all(any(k.startswith(p) for k in reachable) for p in WIN)
    log = R.record(recorder, R.LIB, [W.recorder_line(*c[1:]) for c in W.DENSE_CASES])
    assert len(log.splitlines()) == len(W.DENSE_CASES)
    covered = launched(log)
    missing = sorted(set(reachable) - set(covered))
    assert not missing, f"{len(missing)} of {len(reachable)} reachable windowed instantiations are launched by no case of window_cases.py:\n" + \
        "\n".join(f"  {k}   (e.g. {reachable[k].split(' |')[0]})" for k in missing)
    # and every table case that is a window after normalisation launches windowed kernels only
    for case, ln in zip(W.DENSE_CASES, log.splitlines()):
        names = [p[0] for p in launches(ln) if p[0].startswith(("fwd", "bwd_dq", "bwd_dkv"))]
        assert len(names) == 3, (case[0], ln)
        assert len({n.startswith(WIN) for n in names}) == 1, (case[0], names)


def decode_reachable_grid():
    """decode calls over dtype x head dim x shift regime x l2norm group width (one group, lane-fragment groups, and the D = 96 widths that
    straddle a lane's fragment) x unit-norm inputs, N in {1, 5}"""
    for dtype, D, per_row, N in itertools.product(W.DTYPES, W.DIMS, (False, True), (1, 5)):
        top = 16.0 if dtype == "f16" else 80.0
        for groups in sorted({1, 2, 3, D // 8, D // 4} & {g for g in range(1, D + 1) if D % g == 0}):
            kw = dict(groups=groups, scale=(top if per_row else 8.0) / groups, causal=True)
            yield W.recorder_line(dtype, D, 4, 8, 2, N, 4096, 200, 0, kw, tail=" decode 4096 0 1")
        yield W.recorder_line(dtype, D, 4, 8, 2, N, 4096, 200, 0, dict(l2norm_qk=False, scale=1.0, causal=True), tail=" decode 4096 64 0")


def test_decode_cases_launch_every_reachable_windowed_decode_instantiation(recorder):
    reachable = {k: v for k, v in launched(R.record(recorder, R.LIB, list(decode_reachable_grid()))).items() if k.startswith(DECODE_WIN)}
    assert len(reachable) >= 3 * 5 * 2 and any(k.endswith(",1>") for k in reachable), sorted(reachable)      # (incl. the general-groups form)
    log = R.record(recorder, R.LIB, [W.decode_recorder_line(*c[1:]) for c in W.DECODE_CASES])
    assert len(log.splitlines()) == len(W.DECODE_CASES)
    covered = launched(log)
    missing = sorted(set(reachable) - set(covered))
    assert not missing, f"{len(missing)} of {len(reachable)} reachable decode_win instantiations are launched by no case of window_cases.DECODE_CASES:\n" + \
        "\n".join(f"  {k}   (e.g. {reachable[k].split(' |')[0]})" for k in missing)
    for case, ln in zip(W.DECODE_CASES, log.splitlines()):      # every decode case of the table is a real window: the windowed kernel runs
        assert any(p[0].startswith(DECODE_WIN) for p in launches(ln)), (case[0], ln)


def test_normalised_windows_launch_todays_kernels(recorder):
    """(-1, -1), (-1, 0), causal with any right side and windows that reach past the corners launch exactly what the un-windowed /
    causal call launches (same instantiation, grid, block, LDS); a real window launches the windowed entry points on a causal grid"""
    base = ("bf16", 64, 2, 4, 4, 300, 300)
    def rec(left, right, causal):
        return [tuple(p[:4]) for p in launches(R.record(recorder, R.LIB, [W.recorder_line(*base, left, right, dict(causal=causal))]).splitlines()[0])]
    full, causal = rec(-1, -1, False), rec(-1, -1, True)
    assert full != causal and not any(p[0].startswith(WIN) for p in full + causal)
    assert rec(299, 299, False) == full and rec(5000, -1, False) == full and rec(-1, 299, False) == full
    assert rec(-1, 0, False) == causal and rec(299, 0, False) == causal and rec(-1, 7, True) == causal and rec(300, 200, True) == causal
    win = rec(298, -1, False)
    assert [p[0].split("<")[0] for p in win if p[0].startswith(("fwd", "bwd"))] == ["fwd_win", "bwd_dq_win", "bwd_dkv_win"]
    assert [p[1] for p in win if p[0].startswith("fwd_win")] == [p[1] for p in causal if p[0].startswith("fwd<")]


def test_packed_and_decode_lines(recorder):
    """packed windowed calls launch the windowed entry points on the packed grid; a windowed decode sizes its split count by the keys a
    sequence reads (left + N), and a window that hides nothing is the plain decode call"""
    packed = W.recorder_line("bf16", 64, 12, 4, 4, 600, 600, 50, 0, dict(causal=True), tail=" varlen 12 3000 3000")
    names = [p[0] for p in launches(R.record(recorder, R.LIB, [packed]).splitlines()[0])]
    assert sum(n.startswith(WIN) for n in names) == 3, names
    dec = lambda left: launches(R.record(recorder, R.LIB, [W.recorder_line("bf16", 128, 1, 32, 8, 1, 32768, left, -1, dict(causal=True),
                                                                          tail=" decode 32768 0 1")]).splitlines()[0])
    grid = lambda ls: [int(p[1].split("x")[0]) for p in ls if p[0].startswith("decode") and p[2] == "64"][0]
    plain, hidden_nothing, window = dec(-1), dec(32767), dec(4096)
    assert plain == hidden_nothing and any(p[0].startswith("decode<") for p in plain) and any(p[0].startswith(DECODE_WIN) for p in window)
    assert grid(window) < grid(plain) and grid(window) >= 8 * 16, (grid(window), grid(plain))
