#!/usr/bin/env python3
"""Registers, spills, scratch and occupancy of every *_alibi_kernel instantiation of a build of libfcsa_hip.so next to its windowed
sibling (the *_win_kernel instantiation with the same template arguments), from the code-object metadata (no GPU).
usage: alibi_train_resources.py [libfcsa_hip.so]   (prints the table of profiles/alibi_train_resources.txt)"""
import os, re, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_meta_diff import kernels, demangle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def waves_per_simd(k):
    """occupancy by registers alone: 512 unified registers per lane and SIMD, allocated in blocks of 8, at most 8 waves"""
    regs = max(k.get("vgpr_count", 0) + 0, 1)
    return min(8, 512 // (-(-regs // 8) * 8))


if __name__ == "__main__":
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "flash_cosine_sim_attention_amd", "libfcsa_hip.so")
    ks = kernels(lib)
    names = demangle(sorted(ks))
    by_name = {names[m]: ks[m] for m in ks}
    rows, worse = [], 0
    for nm in sorted(by_name):
        m = re.match(r"void fcsa::(fwd|bwd_dq|bwd_dkv)_alibi_kernel<(.*)>\(", nm)
        if not m:
            continue
        sib = next((x for x in by_name if x.startswith(f"void fcsa::{m.group(1)}_win_kernel<{m.group(2)}>(")), None)
        a, w = by_name[nm], by_name.get(sib, {})
        f = lambda k, key: k.get(key, -1)
        spills_a, spills_w = f(a, "vgpr_spill_count"), f(w, "vgpr_spill_count")
        worse += spills_a > spills_w or f(a, "private_segment_fixed_size") > f(w, "private_segment_fixed_size")
        rows.append(f"{m.group(1) + '_alibi<' + m.group(2).replace('fcsa::', '') + '>':<58} {f(a, 'vgpr_count'):>5} {f(a, 'agpr_count'):>5} {spills_a:>6} "
                    f"{f(a, 'sgpr_spill_count'):>6} {f(a, 'private_segment_fixed_size'):>7} {waves_per_simd(a):>5} | {f(w, 'vgpr_count'):>5} {f(w, 'agpr_count'):>5} "
                    f"{spills_w:>6} {f(w, 'sgpr_spill_count'):>6} {f(w, 'private_segment_fixed_size'):>7} {waves_per_simd(w):>5}")
    print("# tools/alibi_train_resources.py: every *_alibi_kernel instantiation | its *_win_kernel sibling (same template arguments)")
    print("# vgpr = registers per lane (VGPR + AGPR, the unified file), agpr = of those AGPRs, vspill / sspill = spilled VGPRs / SGPRs, scratch = bytes")
    print("# per lane, w/simd = waves per SIMD the register count allows (512 per lane and SIMD, blocks of 8)")
    print(f"{'kernel':<58} {'vgpr':>5} {'agpr':>5} {'vspill':>6} {'sspill':>6} {'scratch':>7} {'w/simd':>5} | {'vgpr':>5} {'agpr':>5} {'vspill':>6} {'sspill':>6} {'scratch':>7} {'w/simd':>5}")
    print("\n".join(rows))
    print(f"# {len(rows)} instantiations; with more spilled VGPRs or more scratch than the windowed sibling: {worse}")
