#!/usr/bin/env python3
"""Registers, spills, scratch and LDS of every kernel of two builds of libfcsa_hip.so, from the code-object metadata (no GPU): the kernels
of the first build that the second one has with other numbers, the kernels only one of them has, and a summary of the new ones.
usage: kernel_meta_diff.py OLD.so NEW.so [substring of the new kernels to list]"""
import re, subprocess, sys, tempfile, os

KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(lib):
    """{mangled name: {key: value}} over the gfx950 code objects bundled in `lib`"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        data = open(lib, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        pos, n = data.find(magic), 0
        while pos >= 0:
            nxt = data.find(magic, pos + 1)
            blob = os.path.join(d, f"bundle{n}")
            open(blob, "wb").write(data[pos:nxt if nxt >= 0 else len(data)])
            co = os.path.join(d, f"co{n}")
            r = subprocess.run(["/opt/rocm/llvm/bin/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                f"--input={blob}", f"--output={co}"], capture_output=True, text=True)
            if r.returncode == 0 and os.path.getsize(co) > 0:
                notes = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
                for ent in re.split(r"\n  - (?=\.agpr_count:)", notes)[1:]:
                    nm = re.search(r"^    \.name:\s*(\S+)", ent, flags=re.M)
                    if nm:
                        out[nm.group(1)] = {k: int(m.group(1)) for k in KEYS for m in [re.search(r"^(?:    |)\." + k + r":\s*(\d+)", ent, flags=re.M)] if m}
            pos, n = nxt, n + 1
    return out


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, res))


if __name__ == "__main__":
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    show = sys.argv[3] if len(sys.argv) > 3 else None
    common = sorted(set(old) & set(new))
    diff = [k for k in common if old[k] != new[k]]
    print(f"kernels: {len(old)} in {os.path.basename(sys.argv[1])}, {len(new)} in {os.path.basename(sys.argv[2])}, {len(common)} in both; "
          f"{len(diff)} of those differ in {', '.join(KEYS)}")
    dm = demangle(diff + sorted(set(old) - set(new)))
    for k in diff:
        print("  DIFFERS", dm[k][:160], {x: (old[k].get(x), new[k].get(x)) for x in KEYS if old[k].get(x) != new[k].get(x)})
    for k in sorted(set(old) - set(new)):
        print("  GONE   ", dm[k][:160])
    added = sorted(set(new) - set(old))
    spilled = [k for k in added if new[k].get("vgpr_spill_count", 0) or new[k].get("private_segment_fixed_size", 0)]
    print(f"new kernels: {len(added)}; with VGPR spills or scratch: {len(spilled)}")
    dn = demangle(added)
    for k in added:
        if k in spilled or (show and show in dn[k]):
            print("  NEW    ", dn[k][:150], {x: new[k].get(x) for x in ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")})
