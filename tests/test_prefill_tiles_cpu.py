"""The tile lookup and the key range of the prefill kernel without a GPU (csrc/fcsa_dispatch.h: prefill_slots, prefill_tile, prefill_kend),
checked by tests/native/prefill_tile_check.cpp -- once as an optimised build and once under AddressSanitizer and UBSan (a stand-alone
program: the sanitizers' runtimes are linked in)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "prefill_tile_check.cpp")
INC = "-I" + os.path.join(ROOT, "flash_cosine_sim_attention_amd", "csrc")


def _run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    b = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, INC, SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.stdout[-500:], r.stderr[-2000:])
    return int(r.stdout.split()[1])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_prefill_tile_lookup_and_key_range(tmp_path):
    """Random tables with G in {1, 3, 4, 5, 8} and N_b including 0: the slots map onto exactly {(b, rt)}, each once, within the slot bound;
    at 16 rows the lookup is ragged_tile; malformed tables stay inside the tensors; every tile's (and wave's) key range equals brute force,
    causal or not, N_b > L_b included."""
    assert _run(tmp_path, "prefill_tile_check", ["-O2"]) > 100000


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_prefill_tile_lookup_under_sanitizers(tmp_path):
    """the same program under -fsanitize=address,undefined: no report (a report ends it with a non-zero status).  Skipped -- and the
    sanitizer claim then unverified on that machine -- only where this g++ cannot link the sanitizer runtimes at all."""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main() { return 0; }",
                           capture_output=True, text=True, timeout=120)
    if probe.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtimes")
    assert _run(tmp_path, "prefill_tile_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]) > 100000
