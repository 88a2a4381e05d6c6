"""The ragged GPU cases of tests/varlen_form_cases.py launch every kernel instantiation a packed-sequence call can reach -- checked without a
GPU by the launch recorder of test_dispatch_cpu.py.  The reachable set is what the varlen block of the recorder's grid launches at 256 CUs
(every dtype x head dim x causal x shift / l2norm mode x K/V grouping on both sides of each dispatch threshold); each instantiation it names
(attention kernels as short_name prints them, l2norm / finalize kernels included) must be launched by at least one case of the table that
test_gpu_varlen.py::test_varlen_forms runs against the float64 oracle."""
import os
import shutil

import pytest

import test_dispatch_cpu as R
from varlen_form_cases import BIT_CASES, BOUNDS_CASES, CASES

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"), reason="needs g++ and the HIP headers")

DTYPE_CODE = {"f32": 0, "f16": 1, "bf16": 2}


def case_line(dtype, D, lq, lk, H, Hk, mx, kw):
    """the recorder line of one case: the problem flash_cosine_sim_attention_varlen hands the C ABI"""
    l2 = kw.get("l2norm_qk", True)
    N, M = (max(lq), max(lk)) if mx is None else (mx, mx)
    return R.line(256, DTYPE_CODE[dtype], D, len(lq), H, Hk, N, M, int(kw.get("causal", False)), 0, 0, int(l2),
                  kw.get("groups", 1), kw.get("scale", 8.0), packed=(sum(lq), sum(lk)))


def attention_launches(log_line):
    """[(instantiation, grid, block)] of the attention kernels of one recorded line"""
    parts = log_line.split(" | ", 1)[1].replace(" | ", "; ").split("; ")[1:]
    return [tuple(p.split()[:3]) for p in parts if p.startswith(("fwd<", "bwd_dq<", "bwd_dkv<"))]


def launched(log):
    """{kernel instantiation: the first recorded line that launches it}"""
    out = {}
    for ln in log.splitlines():
        assert " rc " not in ln, ln
        for part in ln.split(" | ", 1)[1].replace(" | ", "; ").split("; ")[1:]:
            out.setdefault(part.split()[0], ln)
    return out


@pytest.fixture(scope="module")
def recorder(tmp_path_factory):
    assert os.path.exists(R.LIB), "libfcsa_hip.so is not built"
    return R.build_recorder(tmp_path_factory.mktemp("recorder"))


def test_varlen_cases_launch_every_reachable_instantiation(recorder):
    reachable = launched(R.record(recorder, R.LIB, list(dict.fromkeys(R.varlen_grid()))))
    assert any(k.startswith("fwd<") for k in reachable) and any(k.startswith("bwd_dkv<") for k in reachable)
    log = R.record(recorder, R.LIB, [case_line(*c[1:]) for c in CASES])
    assert len(log.splitlines()) == len(CASES)
    covered = launched(log)
    missing = sorted(set(reachable) - set(covered))
    assert not missing, f"{len(missing)} of {len(reachable)} reachable instantiations are launched by no case of varlen_form_cases.py:\n" + \
        "\n".join(f"  {k}   (e.g. {reachable[k].split(' |')[0]})" for k in missing)


def test_varlen_case_table_keeps_its_edges():
    """every case carries the ragged core: empty and one-row spans, t - 1, t, t + 1 for t = 128 and 256, three 256-position tiles, and
    N_s != M_s both ways; max_seqlen is exact in some cases and inflated in others"""
    inflated = set()
    for name, dtype, D, lq, lk, H, Hk, mx, kw in CASES:
        assert len(lq) == len(lk) and H % Hk == 0, name
        pairs = list(zip(lq, lk))
        assert any(n == 0 and m > 0 for n, m in pairs) and any(n > 0 and m == 0 for n, m in pairs), name
        assert any(n == 1 and m > 1 for n, m in pairs) and any(m == 1 and n > 1 for n, m in pairs), name
        for t in (128, 256):
            assert {t - 1, t, t + 1} <= set(lq) and {t - 1, t, t + 1} <= set(lk), name
        assert any(min(n, m) > 2 * 256 for n, m in pairs), name
        assert any(n > m > 0 for n, m in pairs) and any(0 < n < m for n, m in pairs), name
        assert mx is None or mx >= max(lq + lk), name
        inflated.add(mx is not None)
    assert inflated == {True, False}
    assert len({c[0] for c in CASES}) == len(CASES)


def test_bit_cases_launch_the_dense_eight_wave_instantiations(recorder):
    """the packed call and the dense call of each bit-for-bit case launch the same attention kernels on the same grids (dense D = 128:
    the 64-rows-per-wave forward off, as the GPU test sets it), and those are the 8-wave row / key tiles or the two-wave dQ tile"""
    for name, dtype, S, H, L, D, causal in BIT_CASES:
        ff = 0 if D == 128 else 1
        dense = R.line(256, DTYPE_CODE[dtype], D, S, H, H, L, L, int(causal), 0, 0, 1, ff=ff)
        packed = R.line(256, DTYPE_CODE[dtype], D, S, H, H, L, L, int(causal), 0, 0, 1, ff=ff, packed=(S * L, S * L))
        log = R.record(recorder, R.LIB, [dense, packed]).splitlines()
        assert len(log) == 2 and not any(" rc " in ln for ln in log), log
        got_dense, got_packed = (attention_launches(ln) for ln in log)
        assert got_dense == got_packed, (name, got_dense, got_packed)
        fwd, dq, dkv = got_packed
        assert fwd[2] == "512" and dkv[2] == "512", (name, got_packed)
        assert dq[2] == "512" or ",4,0,1,1," in dq[0], (name, got_packed)      # 8 waves, or the 4-wave two-wave (TWO) tile


def test_bounds_cases_take_the_eight_wave_forms(recorder):
    log = R.record(recorder, R.LIB, [case_line(dt, D, lq, lk, H, Hk, None, kw) for _, dt, lq, lk, H, Hk, D, kw in BOUNDS_CASES])
    lines = log.splitlines()
    assert len(lines) == len(BOUNDS_CASES)
    for case, ln in zip(BOUNDS_CASES, lines):
        assert " rc " not in ln, ln
        fwd, dq, dkv = attention_launches(ln)
        assert fwd[2] == "512" and dkv[2] == "512", (case[0], ln)
        assert dq[2] == "512" or ",4,0,1,1," in dq[0], (case[0], ln)      # 8 waves, or the 4-wave two-wave (TWO) tile
    assert any(",4,0,1,1," in attention_launches(ln)[1][0] for ln in lines)      # f16_d128_lean8_two_wave_dq: the two-wave dQ tile


def test_malformed_varlen_line_is_reported(recorder):
    """a varlen line the recorder cannot run prints an error line rather than vanishing from the log"""
    bad = R.line(256, 2, 64, 3, 2, 2, 100, 100, packed=(150, 150)).replace(" varlen 3 ", " varlen 4 ")
    log = R.record(recorder, R.LIB, [bad, case_line(*CASES[0][1:])]).splitlines()
    assert len(log) == 2 and " rc -1 malformed varlen line" in log[0] and " rc " not in log[1], log
