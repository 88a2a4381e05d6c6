"""What fcsa_forward_kvcache_prefill launches, pinned without a GPU (tests/native/prefill_launch_recorder.cpp: the stub HIP runtime of
launch_recorder.cpp under a driver that runs every call through the ragged entry point AND the prefill entry point).

tests/golden/prefill_launches.txt holds, for every call of CASES, each launch of the prefill call (instantiation, grid, block, LDS and the
fields of its parameter block), whether its "kv_append_ragged" launch is, text for text, the one the ragged entry point makes for the same
arguments, and the code and message of a refused call.

    python tests/test_prefill_launches_cpu.py     prints the fixture for the built library
"""
import os
import shutil
import subprocess
import sys
import tempfile

import pytest

import test_dispatch_cpu as R

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"), reason="needs g++ and the HIP headers")

GOLDEN = os.path.join(R.ROOT, "tests", "golden", "prefill_launches.txt")
F32, F16, BF16 = 0, 1, 2


def call(dtype, D, B, H, Hk, max_q, total_q, max_k, capacity, page=0, append=1, causal=1, l2=1, groups=1, scale=8.0, lse=0, fault="", cus=256):
    return (f"{cus} {dtype} {D} {B} {H} {Hk} {max_q} {total_q} {max_k} {capacity} {page} {append} {causal} {l2} {groups} {scale:g} {lse} {fault}"
            .rstrip() + "\n")


def _cases():
    c = []
    add = lambda name, *a, **kw: c.append((name, call(*a, **kw)))
    # the eight instantiations: type x head dim x exponent regime (bf16 leaves the static one above scale * groups = 75, f16 above 11)
    add("bf16 D128", BF16, 128, 4, 32, 8, 1024, 2500, 4096, 4096, page=16)
    add("bf16 D64", BF16, 64, 4, 8, 8, 1024, 2500, 4096, 4096)
    add("f16 D128", F16, 128, 2, 8, 2, 300, 430, 1216, 1216, page=64, lse=1)
    add("f16 D64", F16, 64, 2, 6, 2, 300, 430, 1200, 1200)
    add("bf16 D128 per-row", BF16, 128, 2, 8, 2, 300, 430, 1200, 1200, scale=120.0)
    add("bf16 D64 per-row lse", BF16, 64, 2, 8, 2, 300, 430, 1200, 1200, scale=120.0, lse=1)
    add("f16 D128 per-row", F16, 128, 2, 8, 2, 300, 430, 1200, 1200, scale=16.0, page=16)
    add("f16 D64 per-row", F16, 64, 2, 8, 2, 300, 430, 1200, 1200, scale=16.0)
    # the grid: floor(G * total_q / 128) + B slots per K/V head, whatever the bounds and the CU count say
    add("G = 3", BF16, 64, 8, 6, 2, 300, 490, 1200, 1200)
    add("G = 5, one K/V head", BF16, 128, 8, 5, 1, 300, 490, 1200, 1200)
    add("one token per sequence", BF16, 128, 64, 32, 8, 1, 64, 4096, 4096, page=16)
    add("bounds of 1", BF16, 128, 4, 32, 8, 1, 2500, 1, 4096, page=16)
    add("80 CUs", BF16, 128, 4, 32, 8, 1024, 2500, 4096, 4096, page=16, cus=80)
    # no append, non-causal, groups, l2norm off
    add("no append", BF16, 128, 4, 32, 8, 1024, 2500, 4096, 4096, page=16, append=0)
    add("non-causal lse", F16, 64, 4, 8, 2, 1024, 2500, 4096, 4096, causal=0, lse=1)
    add("groups 16", BF16, 128, 2, 8, 2, 300, 430, 1200, 1200, groups=16, scale=1.0)
    add("groups 2", F16, 64, 2, 8, 2, 300, 430, 1200, 1200, groups=2, scale=4.0)
    add("no l2norm", BF16, 64, 2, 8, 2, 300, 430, 1200, 1200, l2=0, scale=1.0)
    # empty and degenerate sizes
    add("B = 0", BF16, 64, 0, 8, 2, 1, 0, 256, 256)
    add("total_q = 0", BF16, 64, 3, 8, 2, 2, 0, 256, 256)
    add("total_q = 0 lse", BF16, 64, 3, 8, 2, 2, 0, 256, 256, lse=1, fault="null_lse")
    add("capacity 0", BF16, 64, 2, 8, 2, 2, 3, 256, 0)
    # refused calls: one fault each
    add("refused: float32", F32, 64, 2, 8, 2, 300, 430, 1200, 1200)
    add("refused: dim_head 16", BF16, 16, 2, 8, 2, 300, 430, 1200, 1200)
    add("refused: dim_head 32", F16, 32, 2, 8, 2, 300, 430, 1200, 1200)
    add("refused: dim_head 96", BF16, 96, 2, 8, 2, 300, 430, 1200, 1200)
    add("refused: dim_head 48", BF16, 48, 2, 8, 2, 300, 430, 1200, 1200)
    add("refused: new_len 2", BF16, 64, 2, 8, 2, 300, 430, 1200, 1200, append=2)
    add("refused: null seqs", BF16, 64, 2, 8, 2, 300, 430, 1200, 1200, fault="null_seqs")
    add("refused: null cu_seqlens_q", BF16, 64, 2, 8, 2, 300, 430, 1200, 1200, fault="null_cu")
    add("refused: null lse with rows", BF16, 64, 2, 8, 2, 300, 430, 1200, 1200, lse=1, fault="null_lse")
    add("refused: page_size without a table", BF16, 64, 2, 8, 2, 300, 430, 1200, 1216, page=64, fault="no_table")
    add("refused: capacity not whole pages", BF16, 64, 2, 8, 2, 300, 430, 1200, 1200, page=64)
    add("refused: kv_heads do not divide heads", BF16, 64, 2, 8, 3, 300, 430, 1200, 1200)
    add("refused: groups do not divide dim_head", BF16, 64, 2, 8, 2, 300, 430, 1200, 1200, groups=3)
    return c


CASES = _cases()


def build_recorder(out_dir):
    exe = os.path.join(str(out_dir), "prefill_launch_recorder")
    cmd = ["g++", "-O1", "-std=c++17", "-rdynamic", "-D__HIP_PLATFORM_AMD__=1", "-I/opt/rocm/include",
           "-I" + os.path.join(R.ROOT, "flash_cosine_sim_attention_amd", "csrc"),
           os.path.join(R.ROOT, "tests", "native", "prefill_launch_recorder.cpp"), "-o", exe, "-ldl"]
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
    text = fixture_text(build_recorder(tmp_path_factory.mktemp("prefill_recorder")))
    return text, dict(zip([n for n, _ in CASES], text.split("# ")[1:]))


def test_prefill_calls_launch_what_the_fixture_pins(blocks):
    got = blocks[0].splitlines()
    want = open(GOLDEN).read().splitlines()
    diff = [f"- {a}\n+ {b}" for a, b in zip(want, got) if a != b]
    assert not diff and len(got) == len(want), (
        f"{len(diff)} lines differ from tests/golden/prefill_launches.txt ({len(want)} lines, now {len(got)})\n" + "\n".join(diff[:6]))


def test_the_append_is_the_ragged_calls_append(blocks):
    """the same inputs through fcsa_forward_kvcache_varlen / _lse: the kv_append_ragged launch line and every parameter field identical; a call
    that passes no workspace launches the same things"""
    text, by_name = blocks
    assert "DIFFERS" not in text and "DIFFERENT" not in text
    appended = [n for n, b in by_name.items() if "append: same as the ragged call" in b]
    assert len(appended) >= 15 and all("\n  ; kv_append_ragged<" in by_name[n] for n in appended)
    assert "append: none" in by_name["no append"] and "kv_append" not in by_name["no append"]
    assert text.count("without a workspace: the same launches") >= 15


def test_the_prefill_launch(blocks):
    """grid = (floor(G total_q / 128) + B) x Hk workgroups of 256 threads, the LDS of two stage buffers, one split, no workspace, the regime
    in the instantiation; empty calls launch nothing"""
    _, by_name = blocks
    launch = lambda name: next(ln for ln in by_name[name].splitlines() if ln.startswith("  ; prefill<"))
    lds = {64: 2 * 2 * 64 * (64 * 2 + 16), 128: 2 * 2 * 64 * (128 * 2 + 16)}
    assert lds[128] == 69632
    for name, inst, G, total_q, B, Hk, D in (("bf16 D128", "b,128,0", 4, 2500, 4, 8, 128), ("bf16 D64", "b,64,0", 1, 2500, 4, 8, 64),
                                            ("f16 D128", "h,128,0", 4, 430, 2, 2, 128), ("f16 D64", "h,64,0", 3, 430, 2, 2, 64),
                                            ("bf16 D128 per-row", "b,128,1", 4, 430, 2, 2, 128), ("bf16 D64 per-row lse", "b,64,1", 4, 430, 2, 2, 64),
                                            ("f16 D128 per-row", "h,128,1", 4, 430, 2, 2, 128), ("f16 D64 per-row", "h,64,1", 4, 430, 2, 2, 64),
                                            ("G = 3", "b,64,0", 3, 490, 8, 2, 64), ("G = 5, one K/V head", "b,128,0", 5, 490, 8, 1, 128),
                                            ("one token per sequence", "b,128,0", 4, 64, 64, 8, 128), ("80 CUs", "b,128,0", 4, 2500, 4, 8, 128)):
        ln = launch(name)
        slots = G * total_q // 128 + B
        assert ln.startswith(f"  ; prefill<{inst}> {slots * Hk}x1 256 {lds[D]} "), (name, ln[:80])
        assert f" slots={slots} " in ln and " splits=1 " in ln and " ws_o=(nil) ws_ml=(nil) " in ln and f" total_q={total_q} " in ln, (name, ln)
        assert f" dyn={inst[-1]} " in ln and " N=0 row_tiles=0 " in ln
    assert launch("bounds of 1").split(" q=")[0] == launch("bf16 D128").split(" q=")[0]      # the bounds size nothing
    assert " lse=(nil)/0/0/0" in launch("bf16 D128") and " lse=0x" in launch("f16 D128") and "/0/1/8" in launch("f16 D128")
    assert " append=0" in launch("no append") and " append=1" in launch("bf16 D128")
    assert " causal=0 " in launch("non-causal lse") and " win_hi=268435456 " in launch("non-causal lse")
    assert " groups=16 " in launch("groups 16") and " l2norm=0 groups=1 " in launch("no l2norm")
    for name in ("B = 0", "total_q = 0", "total_q = 0 lse"):
        assert "\n  ; " not in by_name[name] and "rc " not in by_name[name], name
    assert "; prefill<" in by_name["capacity 0"] and "kv_append" not in by_name["capacity 0"]


def test_refusals(blocks):
    """each refused form: its code and a message that says what is wrong; nothing is launched"""
    _, by_name = blocks
    refused = {n: b for n, b in by_name.items() if n.startswith("refused")}
    assert len(refused) == 13 and sum("\n  rc " in b for b in by_name.values()) == 13
    assert all("\n  ; " not in b for b in refused.values())
    UNSUPPORTED, INVALID = -2, -1
    want = {"refused: float32": (UNSUPPORTED, "float32 is not supported"), "refused: dim_head 16": (UNSUPPORTED, "dim_head 16 is not supported"),
            "refused: dim_head 32": (UNSUPPORTED, "dim_head 32 is not supported"), "refused: dim_head 96": (UNSUPPORTED, "dim_head 96 is not supported"),
            "refused: new_len 2": (INVALID, "new_len (2) is a flag"), "refused: null seqs": (INVALID, "kvcache_prefill: null argument"),
            "refused: null cu_seqlens_q": (INVALID, "null cu_seqlens_q"), "refused: null lse with rows": (INVALID, "kvcache_prefill: lse: null pointer"),
            "refused: page_size without a table": (INVALID, "without a block_table"), "refused: capacity not whole pages": (INVALID, "whole number of pages")}
    for name, (code, msg) in want.items():
        assert f"\n  rc {code} " in refused[name] and msg in refused[name], (name, refused[name])
    assert "fcsa_forward_kvcache_varlen takes" in refused["refused: float32"] and "fcsa_forward_kvcache_varlen takes" in refused["refused: dim_head 96"]


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        sys.stdout.write(fixture_text(build_recorder(d), *sys.argv[1:2]))
