"""The development trace builds (csrc/fcsa_trace.h: -DFCSA_TRACE, -DFCSA_TRACE_WG, -DFCSA_TRACE_BAR) still compile, without warnings,
and export exactly the readers tools/trace_*.py load.  No product build defines these macros, so nothing else compiles them.
hipcc cross-compiles gfx950 without a GPU; the nine -DFCSA_DEV_ONLY objects take about half a minute on four compilers."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flash_cosine_sim_attention_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NM = shutil.which("llvm-nm", path="/opt/rocm/llvm/bin") or shutil.which("nm")
# the Makefile's CXXFLAGS
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
         "-mllvm", "-amdgpu-mfma-vgpr-form", "-DFCSA_DEV_ONLY"]


def _readers(sites, phase=True, wg=True, bar=False):
    out = set()
    for s in sites:
        if phase:
            out.add("fcsa_trace_read_" + s)
        if wg:
            out |= {"fcsa_trace_read_wg_" + s, "fcsa_trace_read_pass_" + s}
        if bar:
            out.add("fcsa_trace_read_bar_" + s)
    return out


# (source, mode) -> the fcsa_trace_read_* symbols the object defines.  -DFCSA_TRACE implies -DFCSA_TRACE_WG; the wide forward
# (fcsa_fwd3) records phases only.
EXPECTED = {
    ("fcsa_fwd", "FCSA_TRACE"): _readers(["fwd"]),
    ("fcsa_fwd", "FCSA_TRACE_WG"): _readers(["fwd"], phase=False),
    ("fcsa_fwd", "FCSA_TRACE_BAR"): _readers(["fwd"], phase=False, wg=False, bar=True),
    ("fcsa_fwd3", "FCSA_TRACE"): {"fcsa_trace_read_fwd3"},
    ("fcsa_fwd3", "FCSA_TRACE_WG"): set(),
    ("fcsa_fwd3", "FCSA_TRACE_BAR"): set(),
    ("fcsa_bwd", "FCSA_TRACE"): _readers(["dq", "dkv"]),
    ("fcsa_bwd", "FCSA_TRACE_WG"): _readers(["dq", "dkv"], phase=False),
    ("fcsa_bwd", "FCSA_TRACE_BAR"): _readers(["dq", "dkv"], phase=False, wg=False, bar=True),
}


@pytest.mark.skipif(not os.path.exists(HIPCC) or NM is None, reason="needs hipcc and nm")
def test_trace_builds_compile_cleanly_and_export_their_readers(tmp_path):
    def build(key):
        src, mode = key
        obj = str(tmp_path / ("%s.%s.o" % (src, mode)))
        r = subprocess.run([HIPCC] + FLAGS + ["-D" + mode, "-c", src + ".hip", "-o", obj], capture_output=True, text=True, cwd=CSRC,
                           timeout=600)
        syms = None
        if r.returncode == 0:
            nm = subprocess.run([NM, "--defined-only", obj], capture_output=True, text=True, timeout=60, check=True)
            syms = {ln.split()[-1] for ln in nm.stdout.splitlines() if ln.split() and ln.split()[-1].startswith("fcsa_trace_read_")}
        return key, r, syms

    with ThreadPoolExecutor(max_workers=4) as pool:
        results = list(pool.map(build, sorted(EXPECTED)))
    for key, r, syms in results:
        assert r.returncode == 0, "%s -D%s failed:\n%s" % (key[0], key[1], r.stderr[-3000:])
        assert "warning" not in r.stderr, "%s -D%s warns:\n%s" % (key[0], key[1], r.stderr[-3000:])
        assert syms == EXPECTED[key], "%s -D%s exports %s" % (key[0], key[1], sorted(syms))
