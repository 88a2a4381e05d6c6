#!/usr/bin/env python3
"""Instruction text of every kernel of two builds of libfcsa_hip.so (no GPU): the gfx950 code objects bundled in each library are
disassembled (llvm-objdump -d) and compared symbol by symbol, line by line, with addresses, raw encodings, labels and comments stripped.
Prints how many symbols both builds have, how many of those differ, how many instructions were compared, and how many symbols are new.
The companion of tools/kernel_meta_diff.py, which compares registers, spills, scratch and LDS.
usage: kernel_isa_diff.py OLD.so NEW.so"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin/"


def kernels(lib):
    """{symbol: (sha256 of its instruction text, instructions)} over the gfx950 code objects bundled in `lib`"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        data = open(lib, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        pos, n = data.find(magic), 0
        while pos >= 0:
            nxt = data.find(magic, pos + 1)
            blob, co = os.path.join(d, f"bundle{n}"), os.path.join(d, f"co{n}")
            open(blob, "wb").write(data[pos:nxt if nxt >= 0 else len(data)])
            r = subprocess.run([LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                f"--input={blob}", f"--output={co}"], capture_output=True)
            if r.returncode == 0 and os.path.getsize(co) > 0:
                text = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], capture_output=True, text=True).stdout
                cur = None
                for ln in text.splitlines():
                    m = re.match(r"^[0-9a-f]* ?<(.+)>:$", ln)
                    if m:
                        cur = out.setdefault(m.group(1), [hashlib.sha256(), 0])
                        continue
                    ins = re.sub(r"<[^>]*>", "", re.sub(r"\s*//.*$", "", ln)).strip()
                    if cur is not None and ins:
                        cur[0].update((ins + "\n").encode())
                        cur[1] += 1
            pos, n = nxt, n + 1
    return {k: (v[0].hexdigest(), v[1]) for k, v in out.items()}


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    both = [k for k in old if k in new]
    differ = [k for k in both if old[k] != new[k]]
    print(f"symbols: {len(old)} in the first build, {len(new)} in the second, {len(both)} in both; instruction text differs: {len(differ)}; "
          f"instructions compared: {sum(old[k][1] for k in both)}; only in the first: {len(old) - len(both)}; only in the second: {len(new) - len(both)}")
    for k in differ:
        print(f"  DIFFERS {k}: {old[k][1]} -> {new[k][1]} instructions")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
