"""What every key/value-cache decode entry point launches, pinned without a GPU (tests/native/decode_launch_recorder.cpp: the stub HIP
runtime of launch_recorder.cpp under a driver that calls fcsa_forward_kvcache, _window, _quant, _varlen and _lse and prints the
parameter block of every launch).

tests/golden/decode_launches.txt holds, for every call of CASES, the workspace size, each launch (instantiation, grid, block, LDS), the
fields of the parameter block it is launched with, and the code and message of a refused call.  The host side of the decode family is
pure bookkeeping -- which of three kernels, which slice of one parameter block, which grid -- so a change to it that is meant to leave
behaviour alone must leave this file alone, byte for byte.  A call with two faults at once is not in the table: only which of the two is
reported first could differ there.

    python tests/test_decode_launches_cpu.py     prints the fixture for the built library
"""
import os
import shutil
import subprocess
import sys
import tempfile

import pytest

import test_dispatch_cpu as R

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"), reason="needs g++ and the HIP headers")

GOLDEN = os.path.join(R.ROOT, "tests", "golden", "decode_launches.txt")
F32, F16, BF16 = 0, 1, 2


def call(dtype, D, B, H, Hk, N, max_k, capacity, page=0, new_len=0, causal=1, l2=1, groups=1, scale=8.0, window=None, fp8=0, ragged=None,
         lse=0, ws=1, fault="", cus=256):
    """one recorder input line; window = (left, right) or None; ragged = total_q or None (N is max_seqlen_q then)"""
    left, right = window if window is not None else (0, 0)
    return (f"{cus} {dtype} {D} {B} {H} {Hk} {N} {ragged if ragged is not None else 0} {max_k} {capacity} {page} {new_len} {causal} {l2} {groups} "
            f"{scale:g} {int(window is not None)} {left} {right} {fp8} {int(ragged is not None)} {lse} {ws} {fault}".rstrip() + "\n")


def _cases():
    c = []
    add = lambda name, *a, **kw: c.append((name, call(*a, **kw)))
    # the five entry points (and the LSE one on its four routes), contiguous and paged caches, the three types
    add("plain bf16", BF16, 64, 4, 8, 2, 1, 256, 256, new_len=1)
    add("plain f16 paged", F16, 128, 4, 8, 2, 1, 1024, 1024, page=64)
    add("plain f32 append 5", F32, 64, 2, 4, 4, 5, 300, 512, new_len=5)
    add("plain f32 paged non-causal", F32, 32, 3, 6, 3, 1, 500, 512, page=16, causal=0, new_len=1)
    add("window bf16", BF16, 64, 4, 8, 2, 1, 4096, 4096, new_len=1, window=(200, -1))
    add("window f32 paged two-sided", F32, 64, 2, 4, 2, 5, 2048, 2048, page=128, causal=0, window=(100, 2))
    add("quant bf16", BF16, 64, 4, 8, 2, 1, 256, 256, new_len=1, fp8=1)
    add("quant f16 paged window append 5", F16, 128, 2, 8, 2, 5, 4096, 4096, page=64, new_len=5, window=(300, -1), fp8=1)
    add("varlen bf16", BF16, 64, 4, 8, 2, 3, 256, 256, new_len=1, ragged=7)
    add("varlen f32 paged no append", F32, 64, 3, 4, 4, 4, 1000, 1024, page=32, ragged=9)
    add("varlen f16 fp8 paged", F16, 128, 4, 8, 2, 2, 2048, 2048, page=64, new_len=1, fp8=1, ragged=6)
    add("lse plain", BF16, 64, 4, 8, 2, 1, 256, 256, new_len=1, lse=1)
    add("lse plain f32", F32, 64, 2, 4, 4, 5, 300, 512, new_len=5, lse=1)
    add("lse window", F16, 64, 4, 8, 2, 1, 4096, 4096, window=(200, -1), lse=1)
    add("lse fp8", BF16, 128, 4, 8, 2, 1, 1024, 1024, page=64, new_len=1, fp8=1, lse=1)
    add("lse fp8 window", F16, 64, 2, 8, 2, 2, 4096, 4096, window=(150, 0), fp8=1, lse=1)
    add("lse ragged", BF16, 64, 4, 8, 2, 3, 256, 256, new_len=1, ragged=7, lse=1)
    add("lse ragged fp8 window", F16, 64, 4, 8, 2, 3, 4096, 4096, new_len=1, ragged=7, fp8=1, window=(100, -1), lse=1)
    # head dims and l2norm group widths (D = 96, groups = 8: the width that straddles a lane's fragment), l2norm off
    for t, dtype in (("bf16", BF16), ("f32", F32)):
        add(f"D16 groups 2 {t}", dtype, 16, 2, 4, 2, 1, 512, 512, groups=2)
        add(f"D96 groups 1 {t}", dtype, 96, 2, 4, 2, 1, 512, 512)
        add(f"D96 groups 8 {t}", dtype, 96, 2, 4, 2, 1, 512, 512, groups=8, scale=1.0)
        add(f"D96 groups 8 per-row {t}", dtype, 96, 2, 4, 2, 1, 512, 512, groups=8, scale=10.0, window=(64, -1))
        add(f"D128 groups 4 {t}", dtype, 128, 2, 4, 2, 1, 512, 512, groups=4, scale=2.0)
        add(f"D64 no l2norm {t}", dtype, 64, 2, 4, 2, 1, 512, 512, l2=0, scale=1.0)
    add("D96 groups 8 fp8", F16, 96, 2, 4, 2, 1, 512, 512, groups=8, scale=1.0, fp8=1, new_len=1)
    add("D96 groups 8 fp8 per-row window", BF16, 96, 2, 4, 2, 1, 512, 512, groups=8, scale=10.0, fp8=1, window=(64, -1))
    add("D96 groups 8 ragged", BF16, 96, 2, 4, 2, 2, 512, 512, groups=8, scale=1.0, ragged=3)
    add("D96 groups 8 ragged fp8 per-row", F16, 96, 2, 4, 2, 2, 512, 512, groups=8, scale=2.0, ragged=3, fp8=1, new_len=1)
    add("D16 fp8", BF16, 16, 2, 4, 2, 1, 512, 512, fp8=1, new_len=1)
    add("D32 ragged fp8 no l2norm", F16, 32, 2, 4, 2, 2, 512, 512, l2=0, scale=1.0, ragged=3, fp8=1)
    # both exponent regimes: bf16 / f32 leave the static one above scale * groups = 75, f16 above 11
    add("bf16 scale 80", BF16, 64, 4, 8, 2, 1, 256, 256, scale=80.0)
    add("f32 scale 80 lse", F32, 64, 4, 8, 2, 1, 256, 256, scale=80.0, lse=1)
    add("f16 scale 11", F16, 64, 4, 8, 2, 1, 256, 256, scale=11.0)
    add("f16 scale 16", F16, 64, 4, 8, 2, 1, 256, 256, scale=16.0)
    add("f16 scale 16 fp8 lse", F16, 64, 4, 8, 2, 1, 256, 256, scale=16.0, fp8=1, lse=1)
    add("bf16 scale 80 ragged lse", BF16, 64, 4, 8, 2, 3, 256, 256, scale=80.0, ragged=7, lse=1)
    add("bf16 negative scale", BF16, 64, 4, 8, 2, 1, 256, 256, scale=-50.0)
    # windows that are the full call and the causal call after normalisation (decode<, the un-windowed split count, the collapsed causal
    # flag), through each entry point that takes one; ragged calls keep open sides instead
    long = (BF16, 128, 1, 32, 8, 1, 32768, 32768)
    add("long plain", *long)
    add("long window real", *long, window=(4096, -1))
    add("long window hides nothing", *long, window=(32767, -1))
    add("window collapses to full", BF16, 64, 2, 4, 2, 3, 512, 512, causal=0, window=(-1, -1))
    add("window collapses to full, finite sides", BF16, 64, 2, 4, 2, 3, 512, 512, causal=0, window=(511, 2))
    add("window collapses to causal", BF16, 64, 2, 4, 2, 3, 512, 512, causal=0, window=(-1, 0))
    add("causal window collapses to causal", BF16, 64, 2, 4, 2, 3, 512, 512, window=(600, 5))
    add("quant window collapses to causal", F16, 64, 2, 4, 2, 3, 512, 512, causal=0, window=(-1, 0), fp8=1, new_len=1)
    add("quant window collapses to full", F16, 64, 2, 4, 2, 3, 512, 512, causal=0, window=(-1, -1), fp8=1)
    add("lse window collapses to causal", F32, 64, 2, 4, 2, 3, 512, 512, causal=0, window=(-1, 0), lse=1)
    add("lse long window hides nothing", *long, window=(32767, -1), lse=1)
    add("ragged causal no window", BF16, 64, 4, 8, 2, 3, 4096, 4096, ragged=7)
    add("ragged non-causal no window", BF16, 64, 4, 8, 2, 3, 4096, 4096, causal=0, ragged=7)
    add("ragged window", BF16, 64, 4, 8, 2, 3, 4096, 4096, ragged=7, window=(100, -1))
    add("ragged non-causal two-sided window", F32, 64, 4, 8, 2, 3, 4096, 4096, causal=0, ragged=7, window=(100, 1))
    add("ragged non-causal open window", F16, 64, 4, 8, 2, 3, 4096, 4096, causal=0, ragged=7, window=(-1, -1), fp8=1)
    # empty and degenerate sizes
    add("B = 0", BF16, 64, 0, 8, 2, 1, 256, 256, new_len=1)
    add("B = 0 ragged", BF16, 64, 0, 8, 2, 1, 256, 256, new_len=1, ragged=0, ws=0)
    add("N = 0: append only", BF16, 64, 2, 8, 2, 0, 256, 256, new_len=2, ws=0)
    add("N = 0: append only, fp8", F16, 64, 2, 8, 2, 0, 256, 256, page=64, new_len=2, fp8=1, ws=0)
    add("N = 0: append only, lse", F32, 64, 2, 8, 2, 0, 256, 256, new_len=1, lse=1, ws=0, fault="null_lse")
    add("N = 0, no append", BF16, 64, 2, 8, 2, 0, 256, 256, ws=0)
    add("capacity 0", BF16, 64, 2, 8, 2, 1, 256, 0, new_len=1)
    add("capacity 0 ragged fp8", F16, 64, 2, 8, 2, 2, 256, 0, new_len=1, ragged=3, fp8=1)
    add("max_seqlen_k 0", BF16, 64, 2, 8, 2, 1, 0, 256)
    add("total_q = 0", BF16, 64, 3, 8, 2, 2, 256, 256, new_len=1, ragged=0, ws=0)
    add("total_q = 0 lse", BF16, 64, 3, 8, 2, 2, 256, 256, ragged=0, lse=1, ws=0, fault="null_lse")
    add("a batch with an empty sequence", BF16, 64, 3, 8, 2, 2, 256, 256, new_len=1, ragged=2)
    # split counts: a short cache (1), a long one below and above 16 rows per K/V head, other CU counts
    add("short cache", BF16, 128, 1, 32, 8, 1, 64, 64)
    add("long, 32 rows per K/V head", BF16, 128, 1, 64, 4, 2, 32768, 32768)
    add("long fp8 append", F16, 128, 2, 32, 8, 1, 32768, 32768, page=256, new_len=1, fp8=1)
    add("long ragged", BF16, 128, 4, 32, 8, 4, 32768, 32768, new_len=1, ragged=9)
    add("long ragged, 32 rows per K/V head", BF16, 128, 2, 64, 4, 2, 32768, 32768, ragged=4, lse=1)
    add("long at 304 CUs", BF16, 128, 1, 32, 8, 1, 32768, 32768, cus=304)
    add("long ragged at 80 CUs", F16, 64, 2, 16, 2, 3, 16384, 16384, ragged=5, fp8=1, cus=80)
    # refused calls: one fault each
    add("refused: f32 with fp8", F32, 64, 4, 8, 2, 1, 256, 256, fp8=1)
    add("refused: cache type", BF16, 64, 4, 8, 2, 1, 256, 256, fp8=1, fault="cache_type")
    add("refused: null scales", BF16, 64, 4, 8, 2, 1, 256, 256, fp8=1, fault="null_scales")
    add("refused: null scales, ragged", BF16, 64, 4, 8, 2, 3, 256, 256, fp8=1, ragged=7, fault="null_scales")
    add("refused: page_size without a table", BF16, 64, 4, 8, 2, 1, 256, 256, page=64, fault="no_table")
    add("refused: ragged new_len 2", BF16, 64, 4, 8, 2, 3, 256, 256, new_len=2, ragged=7)
    add("refused: window (-2, 0)", BF16, 64, 4, 8, 2, 1, 256, 256, window=(-2, 0))
    add("refused: window (-2, 0), quant", BF16, 64, 4, 8, 2, 1, 256, 256, window=(-2, 0), fp8=1)
    add("refused: window (-2, 0), ragged", BF16, 64, 4, 8, 2, 3, 256, 256, window=(-2, 0), ragged=7)
    add("refused: window (-2, 0), lse", BF16, 64, 4, 8, 2, 1, 256, 256, window=(-2, 0), lse=1)
    add("refused: workspace too small", BF16, 64, 4, 8, 2, 1, 256, 256, ws=2)
    add("refused: workspace too small, ragged", BF16, 64, 4, 8, 2, 3, 256, 256, ragged=7, ws=2)
    add("refused: no workspace, lse fp8", BF16, 64, 4, 8, 2, 1, 256, 256, fp8=1, lse=1, ws=0)
    add("refused: workspace misaligned", BF16, 64, 4, 8, 2, 1, 256, 256, ws=3)
    add("refused: workspace misaligned, ragged", BF16, 64, 4, 8, 2, 3, 256, 256, ragged=7, ws=3)
    add("refused: null lse with rows", BF16, 64, 4, 8, 2, 1, 256, 256, lse=1, fault="null_lse")
    add("refused: null lse with rows, ragged", BF16, 64, 4, 8, 2, 3, 256, 256, ragged=7, lse=1, fault="null_lse")
    add("refused: null cu_seqlens_q", BF16, 64, 4, 8, 2, 3, 256, 256, ragged=7, fault="null_cu")
    add("refused: dim_head 48", BF16, 48, 4, 8, 2, 1, 256, 256)
    add("refused: capacity not whole pages", BF16, 64, 4, 8, 2, 1, 256, 200, page=64)
    return c


CASES = _cases()


def build_recorder(out_dir):
    exe = os.path.join(str(out_dir), "decode_launch_recorder")
    cmd = ["g++", "-O1", "-std=c++17", "-rdynamic", "-D__HIP_PLATFORM_AMD__=1", "-I/opt/rocm/include",
           "-I" + os.path.join(R.ROOT, "flash_cosine_sim_attention_amd", "csrc"),
           os.path.join(R.ROOT, "tests", "native", "decode_launch_recorder.cpp"), "-o", exe, "-ldl"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    return exe


def fixture_text(exe, lib=R.LIB):
    """every case as "# name", then the recorder's block for it (the call and its workspace, one line per launch, the refusal)"""
    log = R.record(exe, lib, [ln for _, ln in CASES])
    out, i = [], -1
    for ln in log.splitlines():
        if not ln.startswith("  "):
            i += 1
            out.append(f"# {CASES[i][0]}")
        out.append(ln)
    assert i == len(CASES) - 1, (i, len(CASES))
    return "\n".join(out) + "\n"


@pytest.fixture(scope="module")
def recorder(tmp_path_factory):
    assert os.path.exists(R.LIB), "libfcsa_hip.so is not built"
    return build_recorder(tmp_path_factory.mktemp("decode_recorder"))


def test_decode_calls_launch_what_the_fixture_pins(recorder):
    got = fixture_text(recorder).splitlines()
    want = open(GOLDEN).read().splitlines()
    diff = [f"- {a}\n+ {b}" for a, b in zip(want, got) if a != b]
    assert not diff and len(got) == len(want), (
        f"{len(diff)} lines differ from tests/golden/decode_launches.txt ({len(want)} lines, now {len(got)}): the decode host path does not "
        "launch what it launched when the fixture was recorded\n" + "\n".join(diff[:6]))


def test_the_table_reaches_every_entry_point_and_form(recorder):
    """the fixture is worth what its table covers: every kernel family x (fp8, ragged, lse) form, the general-groups form, both regimes,
    decode< for collapsed windows, and refusals with their messages"""
    text = open(GOLDEN).read()
    for name in ("kv_append<", "kv_append_fp8<", "kv_append_ragged<", "decode<", "decode_win<", "decode_fp8<", "decode_ragged<", "decode_ragged_fp8<",
                 "decode_combine<", "decode_combine_fp8<", "decode_combine_ragged<", "decode_combine_lse<", "decode_combine_lse_fp8<",
                 "decode_combine_lse_ragged<"):
        assert "; " + name in text, name
    blocks = dict(zip([n for n, _ in CASES], text.split("# ")[1:]))
    assert len(blocks) == len(CASES)
    assert "decode<b,96,0,1>" in blocks["D96 groups 8 bf16"] and "decode_win<f,96,1,1>" in blocks["D96 groups 8 per-row f32"]
    assert "decode_ragged_fp8<h,96,1,1>" in blocks["D96 groups 8 ragged fp8 per-row"]
    for name in ("window collapses to full", "window collapses to causal", "quant window collapses to causal", "lse long window hides nothing"):
        assert "decode_win<" not in blocks[name] and "window=1" not in blocks[name], name
    assert " causal=0 " in blocks["window collapses to full"] and " causal=1 " in blocks["window collapses to causal"]
    plain, same = blocks["long plain"], blocks["long window hides nothing"]
    assert plain.split("\n", 2)[2] == same.split("\n", 2)[2]
    assert "; decode<" not in blocks["N = 0: append only"] and "; kv_append<" in blocks["N = 0: append only"]
    refused = [n for n in blocks if n.startswith("refused")]
    assert len(refused) >= 10 and all("\n  rc -" in blocks[n] and "; " not in blocks[n].split("\n", 2)[2] for n in refused)
    assert sum("\n  rc " in b for b in blocks.values()) == len(refused)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        sys.stdout.write(fixture_text(build_recorder(d), *sys.argv[1:2]))
