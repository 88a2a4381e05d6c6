"""Every `*_alibi_kernel` instantiation a call with alibi_slopes can reach is launched by the GPU case table -- checked without a GPU by a
launch recorder for fcsa_forward_alibi / fcsa_backward_alibi (tests/native/alibi_launch_recorder.cpp: the stub HIP runtime of
launch_recorder.cpp under its own driver), in the manner of test_window_forms_cpu.py.  The reachable set is what a sweep over dtype x head
dim x grid size x shift regime launches at 256 CUs; the share of it the table of tests/alibi_train_cases.py (test_gpu_alibi_train.py runs
it against the float64 oracle) may leave out is zero."""
import itertools
import os
import shutil
import subprocess

import pytest

import alibi_train_cases as A
import test_dispatch_cpu as R
import window_cases as W
from test_window_forms_cpu import launched, launches
from test_window_forms_cpu import recorder as window_recorder      # (the module-scoped fixture that builds window_launch_recorder.cpp)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"), reason="needs g++ and the HIP headers")

ALIBI = ("fwd_alibi<", "bwd_dq_alibi<", "bwd_dkv_alibi<")


@pytest.fixture(scope="module")
def recorder(tmp_path_factory):
    assert os.path.exists(R.LIB), "libfcsa_hip.so is not built"
    exe = os.path.join(str(tmp_path_factory.mktemp("alibi_recorder")), "alibi_launch_recorder")
    cmd = ["g++", "-O1", "-std=c++17", "-rdynamic", "-D__HIP_PLATFORM_AMD__=1", "-I/opt/rocm/include",
           "-I" + os.path.join(R.ROOT, "flash_cosine_sim_attention_amd", "csrc"),
           os.path.join(R.ROOT, "tests", "native", "alibi_launch_recorder.cpp"), "-o", exe, "-ldl"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    return exe


def reachable_grid():
    """test_window_forms_cpu.py::reachable_grid without a window, causal and not: batch x heads on both sides of every threshold of
    tile_waves / choose_*, one / two / five pairs of 128-row tiles, both shift regimes"""
    for dtype, D, bh, L, per_row, causal in itertools.product(W.DTYPES, W.DIMS, (1, 8, 64, 100, 128, 129, 150, 223, 224, 240, 256, 257, 300, 396, 400, 512),
                                                              (300, 600, 1100), (False, True), (True, False)):
        kw = W.per_row_kwargs(dtype, 0) if per_row else {}
        yield A.recorder_line(dtype, D, 1, bh, bh, L, L, -1, -1, dict(kw, causal=causal))


def test_alibi_cases_launch_every_reachable_alibi_instantiation(recorder):
    reachable = {k: v for k, v in launched(R.record(recorder, R.LIB, list(reachable_grid()))).items() if k.startswith(ALIBI)}
    assert all(sum(k.startswith(p) for k in reachable) >= 15 for p in ALIBI), sorted(reachable)
    log = R.record(recorder, R.LIB, [A.recorder_line(*c[1:]) for c in A.DENSE_CASES])
    assert len(log.splitlines()) == len(A.DENSE_CASES)
    covered = launched(log)
    missing = sorted(set(reachable) - set(covered))
    assert not missing, f"{len(missing)} of {len(reachable)} reachable alibi instantiations are launched by no case of alibi_train_cases.py:\n" + \
        "\n".join(f"  {k}   (e.g. {reachable[k].split(' |')[0]})" for k in missing)
    # every case of the table -- whatever its window normalises to -- launches the three entry points that take the slopes, and nothing splits
    for case, ln in zip(A.DENSE_CASES, log.splitlines()):
        names = [p for p in launches(ln) if p[0].startswith(("fwd", "bwd_dq", "bwd_dkv"))]
        assert [p[0].split("<")[0] for p in names] == ["fwd_alibi", "bwd_dq_alibi", "bwd_dkv_alibi"], (case[0], ln)
        assert all(p[1].endswith("x1") for p in names), (case[0], ln)


def test_a_call_with_slopes_is_a_windowed_launch_whatever_its_window(recorder, window_recorder):
    """no window, causal, a window past the corners, a real window: the alibi entry points; on a real window with the template arguments,
    grid, block and LDS of the windowed call's kernels"""
    base = ("bf16", 64, 2, 8, 2, 300, 300)
    kernels = lambda exe, line: [tuple(p[:4]) for p in launches(R.record(exe, R.LIB, [line]).splitlines()[0]) if p[0].startswith(("fwd", "bwd_dq", "bwd_dkv"))]
    for left, right, causal in ((-1, -1, False), (-1, -1, True), (5000, -1, False), (64, 0, True), (129, 64, False)):
        mine = kernels(recorder, A.recorder_line(*base, left, right, dict(causal=causal)))
        assert [p[0].split("<")[0] for p in mine] == ["fwd_alibi", "bwd_dq_alibi", "bwd_dkv_alibi"]
    mine = kernels(recorder, A.recorder_line(*base, 64, 0, dict(causal=True)))
    theirs = kernels(window_recorder, W.recorder_line(*base, 64, 0, dict(causal=True)))
    assert [p[0].split("<")[0] for p in theirs] == ["fwd_win", "bwd_dq_win", "bwd_dkv_win"]
    assert [p[1:] for p in mine] == [p[1:] for p in theirs]
    assert [p[0].split("<")[1] for p in mine] == [p[0].split("<")[1] for p in theirs]


def test_packed_lines(recorder):
    packed = A.recorder_line("bf16", 64, 12, 4, 4, 600, 600, -1, -1, dict(causal=True), tail=" varlen 12 3000 3000")
    names = [p[0] for p in launches(R.record(recorder, R.LIB, [packed]).splitlines()[0])]
    assert sum(n.startswith(ALIBI) for n in names) == 3, names
