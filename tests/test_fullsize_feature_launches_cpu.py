"""What the full-size cases launch, pinned without a GPU (the window launch recorder of test_window_forms_cpu.py).

tests/golden/fullsize_feature_launches.txt holds, for every case of tests/fullsize_feature_cases.py and every problem of
test_gpu_address_range.py, the kernel instantiations, grids and split counts the library launches at 256 CUs: a dispatch change that
silently moves the shapes the README advertises to other kernels shows up as a diff of it.  Its last block lists the (instantiation,
workgroups) pairs no case of the short tables (window_cases.py, varlen_form_cases.py) launches -- what the full-size table adds.

The address-range tests compare a call far from its tensor's base with the same call on compact data, bit for bit: the two share one
recorder line by construction (same dtype, D, batch x heads, lengths), so the same instantiation, grid and splits.  That is an argument,
not a recording: the recorder is given no batch, block or position stride, so the fixture cannot show that one leaves the dispatch alone.
ASSUMPTION to re-check when fcsa_dispatch.h grows a rule that reads a stride: today the one dispatch rule
that reads a STRIDE is fwd3_applies (the D = 128 64-rows-per-wave forward has no re-open of its 32-bit tile offset): checked here on both
sides of its 0x7fffffff bound, and for the 1 MiB-pitch problem of test_gpu_address_range.py.

    python tests/test_fullsize_feature_launches_cpu.py     prints the fixture for the built library
"""
import os
import shutil
import subprocess
import sys
import tempfile

import pytest

import fullsize_feature_cases as FC
import test_dispatch_cpu as R
import varlen_form_cases as VF
import window_cases as W
from test_window_forms_cpu import launches, recorder  # noqa: F401  (the window recorder fixture)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"), reason="needs g++ and the HIP headers")

GOLDEN = os.path.join(R.ROOT, "tests", "golden", "fullsize_feature_launches.txt")


def _pairs(log):
    """{(instantiation, workgroups)} of the attention and decode kernels of recorded lines"""
    return {(p[0], p[1]) for ln in log.splitlines() for p in launches(ln) if p[0].startswith(("fwd", "bwd_dq", "bwd_dkv", "decode"))}


def fixture_text(exe):
    cases = FC.all_lines() + FC.address_lines()
    log = R.record(exe, R.LIB, [ln for _, ln in cases]).splitlines()
    assert len(log) == len(cases)
    out = [f"{name} :: {ln}" for (name, _), ln in zip(cases, log)]
    short = [W.recorder_line(*c[1:]) for c in W.DENSE_CASES] + [W.decode_recorder_line(*c[1:]) for c in W.DECODE_CASES]
    for name, dtype, D, lq, lk, H, Hk, mx, kw in VF.CASES:
        short.append(W.recorder_line(dtype, D, len(lq), H, Hk, mx or max(lq), mx or max(lk), -1, -1, kw, tail=f" varlen {len(lq)} {sum(lq)} {sum(lk)}"))
    new = sorted(_pairs("\n".join(log[:len(FC.all_lines())])) - _pairs(R.record(exe, R.LIB, short)))
    out.append("# (instantiation, workgroups) of the full-size table that no case of window_cases.py / varlen_form_cases.py launches:")
    out += [f"#   {k} {g}" for k, g in new]
    return "\n".join(out) + "\n"


def test_fullsize_cases_launch_what_the_fixture_pins(recorder):
    got = fixture_text(recorder)
    want = open(GOLDEN).read()
    if got != want:
        diff = [f"- {a}\n+ {b}" for a, b in zip(want.splitlines(), got.splitlines()) if a != b]
        pytest.fail(f"{len(diff)} lines differ from tests/golden/fullsize_feature_launches.txt (regenerate it with this file's main if the "
                    "dispatch change is intended):\n" + "\n".join(diff[:10]))
    for ln in got.splitlines():
        assert " rc " not in ln, ln


def test_every_fullsize_case_runs_its_operator(recorder):
    """window cases launch the three windowed kernels, packed cases the packed grid (windowed where a window is set), decode cases the
    decode kernel with tens of key splits over the 32k cache"""
    log = dict(zip([n for n, _ in FC.all_lines()], R.record(recorder, R.LIB, [ln for _, ln in FC.all_lines()]).splitlines()))
    for c in FC.WINDOW_CASES:
        assert [p[0].split("<")[0] for p in launches(log[c[0]]) if p[0].startswith(("fwd", "bwd"))] == ["fwd_win", "bwd_dq_win", "bwd_dkv_win"], c[0]
    for c in FC.PACKED_CASES:
        names = [p[0].split("<")[0] for p in launches(log[c[0]]) if p[0].startswith(("fwd", "bwd_d"))]
        assert names == (["fwd_win", "bwd_dq_win", "bwd_dkv_win"] if c[7] != (-1, -1) else ["fwd", "bwd_dq", "bwd_dkv"]), (c[0], names)
    for c in FC.DECODE_CASES:
        grid = [int(p[1].split("x")[0]) for p in launches(log[c[0]]) if p[0].startswith(("decode<", "decode_win<"))]
        B, Hk = c[3], c[5]
        assert len(grid) == 1 and grid[0] >= 8 * B * Hk, (c[0], grid)          # (>= 8 key splits per (sequence, K/V head))


@pytest.fixture(scope="module")
def plain_recorder(tmp_path_factory):
    assert os.path.exists(R.LIB), "libfcsa_hip.so is not built"
    return R.build_recorder(tmp_path_factory.mktemp("recorder"))


def _forward(exe, line):
    ln = R.record(exe, R.LIB, [line]).splitlines()[0]
    assert " rc " not in ln, ln
    return [p.split()[0] for p in ln.split(" | ", 1)[1].replace(" | ", "; ").split("; ") if p.startswith("fwd")][0]


def test_fwd3_kernel_is_left_at_its_32bit_offset_bound(plain_recorder):
    """fwd3_applies: (M + 384) rows of K / V (and (N + 256) of Q) must stay below 0x7fffffff bytes from the slice base.  At a 1 MiB row
    pitch that is M + 384 <= 2047: M = 1663 still takes fwd3_kernel, M = 1664 must not; likewise at the bound counted in bytes for a
    pitch that does not divide it; and the chip-filling 1 MiB-pitch problem of test_gpu_address_range.py launches exactly what its
    contiguous twin launches with the 64-rows-per-wave forward switched off (which is how that test gets identical bits)."""
    line = lambda M, rs, ff=1, B=32, H=8, N=256: R.line(256, 2, 128, B, H, H, N, M, 1, l2=1, rowstride=rs, ff=ff)
    assert _forward(plain_recorder, line(1663, FC.PITCH)).startswith("fwd3<")
    assert _forward(plain_recorder, line(1664, FC.PITCH)).startswith("fwd<")
    rs = 768 * 1024          # (M + 384) * rs crosses 0x7fffffff between M + 384 = 2730 and 2731
    assert (2730 * rs < 0x7fffffff <= 2731 * rs)
    assert _forward(plain_recorder, line(2730 - 384, rs)).startswith("fwd3<")
    assert _forward(plain_recorder, line(2731 - 384, rs)).startswith("fwd<")
    H, rows = FC.ADDR_PITCH_FWD3
    rec = lambda rs, ff: R.record(plain_recorder, R.LIB, [line(rows, rs, ff, 1, H, rows)]).splitlines()[0].split(" | ", 1)[1]
    assert "fwd3<" in rec(0, 1) and "fwd3<" not in rec(FC.PITCH, 1)
    assert rec(FC.PITCH, 1) == rec(0, 0)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "window_launch_recorder")
        subprocess.run(["g++", "-O1", "-std=c++17", "-rdynamic", "-D__HIP_PLATFORM_AMD__=1", "-I/opt/rocm/include",
                        "-I" + os.path.join(R.ROOT, "flash_cosine_sim_attention_amd", "csrc"),
                        os.path.join(R.ROOT, "tests", "native", "window_launch_recorder.cpp"), "-o", exe, "-ldl"], check=True)
        sys.stdout.write(fixture_text(exe))
