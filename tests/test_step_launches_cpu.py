"""What fcsa_forward_kvcache_step launches, pinned without a GPU, and the arithmetic behind its routing.

tests/native/step_launch_recorder.cpp (the stub HIP runtime of launch_recorder.cpp under a driver that runs every call through the ragged
entry point AND the step entry point) gives, for every call of CASES, each launch of the step call -- instantiation, grid, block, LDS and
the fields of its parameter block -- the workspace the two calls ask for, whether the append is the ragged call's, whether ALL launches are
(float32, D = 96), and the code and message of a refused call: tests/golden/step_launches.txt.

    python tests/test_step_launches_cpu.py     prints the fixture for the built library

tests/native/step_tile_check.cpp checks the routing partition of the two tile maps and the windowed key range by brute force, once as an
optimised build and once under AddressSanitizer and UBSan (a stand-alone program)."""
import os
import shutil
import subprocess
import sys
import tempfile

import pytest

import test_dispatch_cpu as R
from flash_cosine_sim_attention_amd import _lib

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"), reason="needs g++ and the HIP headers")

GOLDEN = os.path.join(R.ROOT, "tests", "golden", "step_launches.txt")
F32, F16, BF16 = 0, 1, 2
CSRC = os.path.join(R.ROOT, "flash_cosine_sim_attention_amd", "csrc")


def call(dtype, D, B, H, Hk, max_q, total_q, max_k, capacity, page=0, append=1, causal=1, l2=1, groups=1, scale=8.0, lse=0, fp8=0, window=None,
         chunk_rows=-1, bound=-1, no_decode=0, no_chunk=0, fault="", cus=256):
    left, right = window or (0, 0)
    return (f"{cus} {dtype} {D} {B} {H} {Hk} {max_q} {total_q} {max_k} {capacity} {page} {append} {causal} {l2} {groups} {scale:g} {lse} {fp8} "
            f"{int(window is not None)} {left} {right} {chunk_rows} {bound} {no_decode} {no_chunk} {fault}".rstrip() + "\n")


# the mixed batch of the measurements: 63 decodes and one 512-token chunk, H 32 / Hk 8, D 128, pages of 16
MIXED = (BF16, 128, 64, 32, 8, 512, 575, 4096, 4096)


def _cases():
    c = []
    add = lambda name, *a, **kw: c.append((name, call(*a, **kw)))
    add("mixed default threshold", *MIXED, page=16)
    add("mixed threshold 128 bound 63", *MIXED, page=16, chunk_rows=128, bound=63)
    add("mixed threshold 0", *MIXED, page=16, chunk_rows=0)
    add("mixed threshold beyond", *MIXED, page=16, chunk_rows=10 ** 9)
    add("mixed 80 CUs", *MIXED, page=16, chunk_rows=128, bound=63, cus=80)
    add("fp8", *MIXED, page=16, fp8=1, bound=63)
    add("fp8 lse per-row f16", F16, 64, 4, 8, 2, 300, 430, 1200, 1200, fp8=1, lse=1, scale=16.0, chunk_rows=128)
    add("the default threshold is the header's", *MIXED, page=16, chunk_rows=_lib.STEP_CHUNK_ROWS)
    add("window", *MIXED, page=16, window=(1024, -1), bound=63)
    add("window right side non-causal", F16, 128, 4, 8, 2, 300, 430, 1200, 1200, causal=0, window=(64, 5))
    add("right side 0 non-causal", BF16, 64, 4, 8, 8, 300, 430, 1200, 1200, causal=0, window=(-1, 0))
    add("window that is open: the plain form", BF16, 64, 4, 8, 8, 300, 430, 1200, 1200, window=(-1, -1))
    add("fp8 window", BF16, 64, 4, 8, 2, 300, 430, 1200, 1200, fp8=1, window=(100, -1))
    add("lse", *MIXED, page=16, lse=1, bound=63)
    add("non-causal per-row", BF16, 128, 4, 8, 2, 300, 430, 1200, 1200, causal=0, scale=120.0)
    add("no append groups 2", F16, 64, 4, 6, 2, 300, 430, 1200, 1200, append=0, groups=2, scale=4.0)
    add("promise: no decode", *MIXED, page=16, chunk_rows=0, bound=0, no_decode=1)
    add("promise: no chunk", *MIXED, page=16, chunk_rows=10 ** 9, no_chunk=1)
    add("promise: no decode, no workspace given", *MIXED, page=16, chunk_rows=0, no_decode=1, fault="no_workspace")
    add("float32 is the ragged call", F32, 64, 4, 8, 2, 300, 430, 1200, 1200, chunk_rows=0, bound=5, no_decode=1)
    add("float32 lse window", F32, 32, 4, 8, 2, 300, 430, 1200, 1200, lse=1, window=(64, 0))
    add("D 96 is the ragged call", BF16, 96, 4, 8, 2, 300, 430, 1200, 1200, page=16, chunk_rows=128, no_chunk=1)
    add("D 96 fp8 is the ragged call", F16, 96, 4, 8, 2, 300, 430, 1200, 1200, fp8=1, lse=1)
    add("B = 0", BF16, 64, 0, 8, 2, 1, 0, 256, 256)
    add("total_q = 0", BF16, 64, 3, 8, 2, 2, 0, 256, 256, lse=1, fault="null_lse")
    add("capacity 0", BF16, 64, 2, 8, 2, 2, 3, 256, 0)
    add("refused: null step", *MIXED, page=16, fault="null_step")
    add("refused: null cu_seqlens_q", *MIXED, page=16, fault="null_cu")
    add("refused: null lse with rows", *MIXED, page=16, lse=1, fault="null_lse")
    add("refused: no workspace", *MIXED, page=16, fault="no_workspace")
    add("refused: a promise of 2", *MIXED, page=16, no_decode=2)
    add("refused: new_len 2", *MIXED, page=16, append=2)
    add("refused: float32 with an fp8 cache", F32, 64, 4, 8, 2, 300, 430, 1200, 1200, fp8=1)
    add("refused: window left below -1", *MIXED, page=16, window=(-2, 0))
    add("refused: capacity not whole pages", BF16, 64, 2, 8, 2, 300, 430, 1200, 1200, page=64)
    return c


CASES = _cases()


def build_recorder(out_dir):
    exe = os.path.join(str(out_dir), "step_launch_recorder")
    cmd = ["g++", "-O1", "-std=c++17", "-rdynamic", "-D__HIP_PLATFORM_AMD__=1", "-I/opt/rocm/include", "-I" + CSRC,
           os.path.join(R.ROOT, "tests", "native", "step_launch_recorder.cpp"), "-o", exe, "-ldl"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    return exe


def fixture_text(exe, lib=R.LIB):
    """every case as "# name", then the recorder's block for it"""
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
def blocks(tmp_path_factory):
    assert os.path.exists(R.LIB), "libfcsa_hip.so is not built"
    text = fixture_text(build_recorder(tmp_path_factory.mktemp("step_recorder")))
    return text, dict(zip([n for n, _ in CASES], text.split("# ")[1:]))


def test_step_calls_launch_what_the_fixture_pins(blocks):
    got = blocks[0].splitlines()
    want = open(GOLDEN).read().splitlines()
    diff = [f"- {a}\n+ {b}" for a, b in zip(want, got) if a != b]
    assert not diff and len(got) == len(want), (
        f"{len(diff)} lines differ from tests/golden/step_launches.txt ({len(want)} lines, now {len(got)})\n" + "\n".join(diff[:6]))


def _launches(block):
    return [ln[4:].split(" ")[0] for ln in block.splitlines() if ln.startswith("  ; ")]


def _field(line, name):
    return line.split(f" {name}=")[1].split(" ")[0]


def test_the_launches_and_their_order(blocks):
    text, by = blocks
    assert "DIFFERS" not in text
    # the append once, decode and combine, then the chunk launch
    assert _launches(by["mixed default threshold"]) == ["kv_append_ragged<b,128,0>", "step_decode<b,128,0>", "step_combine<b,128,0>", "step_prefill<b,128,0,0,0>"]
    assert _launches(by["lse"])[2] == "step_combine_lse<b,128,0>"
    assert _launches(by["fp8"]) == ["kv_append_ragged<b,128,1>", "step_decode_fp8<b,128,0>", "step_combine<b,128,1>", "step_prefill<b,128,0,1,1>"]
    assert _launches(by["fp8 lse per-row f16"])[1:] == ["step_decode_fp8<h,64,1>", "step_combine_lse<h,64,1>", "step_prefill<h,64,1,1,1>"]
    # the windowed chunk form only where a side hides something; an fp8 cache always takes it
    assert _launches(by["window"])[-1] == "step_prefill<b,128,0,1,0>"
    assert _launches(by["window right side non-causal"])[-1] == "step_prefill<h,128,0,1,0>"
    assert _launches(by["right side 0 non-causal"])[-1] == "step_prefill<b,64,0,1,0>"
    assert _launches(by["window that is open: the plain form"])[-1] == "step_prefill<b,64,0,0,0>"
    assert _launches(by["fp8 window"])[-1] == "step_prefill<b,64,0,1,1>"
    assert _launches(by["non-causal per-row"])[-1] == "step_prefill<b,128,1,0,0>"
    assert _launches(by["no append groups 2"])[0].startswith("step_decode<") and "append: none" in by["no append groups 2"]
    # the promises skip a launch
    assert _launches(by["promise: no decode"]) == ["kv_append_ragged<b,128,0>", "step_prefill<b,128,0,0,0>"]
    assert "workspace 0 " in by["promise: no decode"] and _launches(by["promise: no decode, no workspace given"]) == _launches(by["promise: no decode"])
    assert _launches(by["promise: no chunk"]) == ["kv_append_ragged<b,128,0>", "step_decode<b,128,0>", "step_combine<b,128,0>"]
    # empty calls launch nothing; a cache without capacity has nothing to append
    for name in ("B = 0", "total_q = 0"):
        assert not _launches(by[name]) and "rc " not in by[name]
    assert _launches(by["capacity 0"])[0].startswith("step_decode<")
    appended = [n for n, b in by.items() if "append: same as the ragged call" in b]
    assert len(appended) >= 19


def test_grids_splits_and_the_threshold(blocks):
    _, by = blocks
    B, H, Hk, total, G = 64, 32, 8, 575, 4
    lines = lambda name: [ln for ln in by[name].splitlines() if ln.startswith("  ; ")]
    for name, threshold in (("mixed default threshold", "default"), ("mixed threshold 128 bound 63", 128), ("mixed threshold 0", 0),
                            ("mixed threshold beyond", 10 ** 9)):
        _, dec, comb, pre = lines(name)
        splits = int(_field(dec, "splits"))
        dslots, cslots = G * total // 16 + B, G * total // 128 + B
        assert f" {dslots * Hk * splits}x1 64 " in dec and _field(dec, "slots") == str(dslots)
        assert f" {cslots * Hk}x1 256 69632 " in pre and _field(pre, "slots") == str(cslots) and _field(pre, "splits") == "1"
        assert " ws_o=(nil) ws_ml=(nil) " in pre and " ws_o=0x" in dec
        assert f" {(total * H * 32 + 255) // 256}x1 256 0 " in comb
        for ln in (dec, comb, pre):
            assert _field(ln, "chunk_rows") == str(threshold) and _field(ln, "total_q") == str(total)
    # (the fixture does not pin the default: it reads "default" where the block holds FCSA_STEP_CHUNK_ROWS for a request of < 0)
    strip = lambda ln: ln.split(" chunk_rows=")[0]
    assert [strip(l) for l in lines("the default threshold is the header's")] == [strip(l) for l in lines("mixed default threshold")]
    assert _field(lines("the default threshold is the header's")[1], "chunk_rows") == str(_lib.STEP_CHUNK_ROWS)
    # the split count is sized by the decode-rows bound: 63 rows need more splits than 575 to fill the chip, and the workspace follows
    full, few = (int(_field(lines(n)[1], "splits")) for n in ("mixed default threshold", "mixed threshold 128 bound 63"))
    assert few > full >= 1
    ws = lambda name: [int(x.strip("()")) for x in by[name].split("  workspace ")[1].split("\n")[0].split() if x.strip("()").isdigit()]
    assert ws("mixed default threshold")[0] == ws("mixed default threshold")[1]      # no bound: the ragged call's plan
    assert ws("mixed threshold 128 bound 63")[0] == ws("mixed default threshold")[0] // full * few
    assert int(_field(lines("mixed 80 CUs")[1], "splits")) < few
    # the ragged window sides: open ones for a call without a window, causal as hi = 0
    pre = lines("mixed default threshold")[-1]
    assert _field(pre, "win_lo") == "268435456" and _field(pre, "win_hi") == "0" and _field(pre, "causal") == "1"
    assert _field(lines("window")[-1], "win_lo") == "1024"
    assert _field(lines("window right side non-causal")[-1], "win_hi") == "5"
    assert " k_scale=0x" in lines("fp8")[-1] and " k_scale=(nil)" in pre
    assert " lse=0x" in lines("lse")[-1] and " lse=0x" in lines("lse")[2] and " lse=(nil)/0/0/0" in pre


def test_where_there_is_no_chunk_kernel_the_call_is_the_ragged_call(blocks):
    _, by = blocks
    for name in ("float32 is the ragged call", "float32 lse window", "D 96 is the ragged call", "D 96 fp8 is the ragged call"):
        assert "launches: the ragged call's" in by[name], name
        assert all(l.startswith(("kv_append_ragged", "decode_ragged", "decode_combine")) for l in _launches(by[name])) and len(_launches(by[name])) == 3
        got, theirs = by[name].split("  workspace ")[1].split("\n")[0].replace("(ragged ", "").rstrip(")").split()
        assert got == theirs != "0"
    assert sum("launches: the ragged call's" in b for b in by.values()) == 4


def test_refusals(blocks):
    _, by = blocks
    refused = {n: b for n, b in by.items() if n.startswith("refused")}
    assert len(refused) == 9 and sum("\n  rc " in b for b in by.values()) == 9
    assert all(not _launches(b) for b in refused.values())
    UNSUPPORTED, INVALID, WORKSPACE = -2, -1, -4
    want = {"refused: null step": (INVALID, "kvcache_step: null argument"), "refused: null cu_seqlens_q": (INVALID, "null cu_seqlens_q"),
            "refused: null lse with rows": (INVALID, "kvcache_step: lse: null pointer"),
            "refused: no workspace": (WORKSPACE, "kvcache_step: workspace too small"), "refused: a promise of 2": (INVALID, "are flags"),
            "refused: new_len 2": (INVALID, "new_len (2) is a flag"), "refused: float32 with an fp8 cache": (UNSUPPORTED, "float32 queries with an fp8 cache"),
            "refused: window left below -1": (INVALID, "window"), "refused: capacity not whole pages": (INVALID, "whole number of pages")}
    for name, (code, msg) in want.items():
        assert f"\n  rc {code} " in refused[name] and msg in refused[name], (name, refused[name])


def _run_check(tmp_path, name, flags):
    exe = str(tmp_path / name)
    src = os.path.join(R.ROOT, "tests", "native", "step_tile_check.cpp")
    b = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + CSRC, src, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.stdout[-500:], r.stderr[-2000:])
    return int(r.stdout.split()[1])


def test_routing_partition_and_windowed_key_range(tmp_path):
    """random tables (malformed ones that ragged_cu clamps included) at nine thresholds: every (sequence, row) is claimed by exactly one tile
    of exactly one of the two tile maps, and the combine agrees; every tile's [start, end) holds every key visible to any of its rows"""
    assert _run_check(tmp_path, "step_tile_check", ["-O2"]) > 1000000


def test_routing_partition_under_sanitizers(tmp_path):
    """the same stand-alone program under -fsanitize=address,undefined: no report.  Skipped only where this g++ cannot link the sanitizer
    runtimes at all."""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main() { return 0; }",
                           capture_output=True, text=True, timeout=120)
    if probe.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtimes")
    assert _run_check(tmp_path, "step_tile_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]) > 1000000


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        sys.stdout.write(fixture_text(build_recorder(d), *sys.argv[1:2]))
