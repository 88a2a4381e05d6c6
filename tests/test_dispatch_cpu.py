"""Which kernel every problem launches, checked without a GPU.  tests/native/launch_recorder.cpp is a stub HIP runtime plus a driver: it
calls fcsa_forward / fcsa_backward of the built libfcsa_hip.so with fake device addresses and prints, one line per problem, the workspace
sizes and every launch (kernel instantiation, grid, block, dynamic LDS, the dispatch fields of its parameters).
tests/golden/dispatch_launches.txt holds those lines for 252 problems that together launch every kernel instantiation, every split path and
the group sweep at 256, 304 and 80 CUs, followed by a block of packed-sequence problems (fcsa_forward_varlen / fcsa_backward_varlen, lines
ending "varlen S total_q total_k"): varlen_cover() of varlen_grid(), every instantiation those reach at 256 CUs and every workgroup count
of the grid's threshold shapes; a dispatch change shows up as a diff of it.

    python tests/test_dispatch_cpu.py LIB [--full | --varlen]     prints the lines of LIB for the golden problems (or the full grid, or
                                                                  the varlen block) to stdout
"""
import itertools
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dispatch_launches.txt")
LIB = os.path.join(ROOT, "flash_cosine_sim_attention_amd", "libfcsa_hip.so")
CUS = (256, 304, 80)
DIMS = (16, 32, 64, 96, 128)


def build_recorder(out_dir):
    exe = os.path.join(str(out_dir), "launch_recorder")
    cmd = ["g++", "-O1", "-std=c++17", "-rdynamic", "-D__HIP_PLATFORM_AMD__=1", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "flash_cosine_sim_attention_amd", "csrc"), os.path.join(ROOT, "tests", "native", "launch_recorder.cpp"),
           "-o", exe, "-ldl"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    return exe


def record(exe, lib, problems):
    r = subprocess.run([exe, lib], input="".join(problems), capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def line(cus, dtype, D, B, H, Hk, N, M, causal=0, mask=0, bias=0, l2=0, groups=1, scale=8.0, layout=0, rowstride=0, ff=1, kf=1, packed=None):
    """one recorder input line; packed = (total_q, total_k): B packed sequences of at most N / M rows (fcsa_forward_varlen)"""
    tail = "" if packed is None else f" varlen {B} {packed[0]} {packed[1]}"
    return f"{cus} {dtype} {D} {B} {H} {Hk} {N} {M} {causal} {mask} {bias} {l2} {groups} {scale:g} {layout} {rowstride} {ff} {kf}{tail}\n"


def knobs(dtype, D, H, Hk):
    """(forward form, kv-group form) settings worth recording: the defaults, plus each other value where the knob has an effect"""
    out = [(1, 1)]
    if dtype != 0 and D == 128:
        out.append((0, 1))
    if 1 < Hk < H:
        out += [(1, 0), (1, 2)]
    return out


def full_grid():
    """Every dtype x head dim x masking x bias x l2norm x K/V grouping on a few shapes, and a reduced set of those on shapes that straddle
    every threshold of the dispatch (7/8 of the CUs, the CU count, a last round filled ~55 %, 512 positions per split, 2048 keys and the
    32-bit offset limit of the D = 128 wide forward, N != M) -- at 256, 304 and 80 CUs."""
    # (causal, mask), bias (0 none, 1 per head, 2 per batch), (l2norm, groups or -1: non-fusable D // 4, scale: 80 = per-row shift)
    modes = ((0, 0), (0, 1), (1, 0))
    norms = ((0, 1, 8.0), (1, 1, 8.0), (1, 1, 80.0), (1, -1, 8.0))
    for cus in CUS:
        shapes = [(1, 8, 200, 300), (2, 8, 1024, 1024), (4, 8, 4096, 4096), (1, 8, 1024, 8192), (16, 8, 512, 512), (cus // 8, 8, 256, 2048)]
        for dtype, D, (causal, mask), bias, (l2, g, scale), hk, (B, H, N, M) in itertools.product(
                (0, 1, 2), DIMS, modes, (0, 1, 2), norms, (1, 8, 2), shapes):
            groups = (D // 4 if g < 0 else g) if l2 else 1
            for ff, kf in knobs(dtype, D, H, hk if hk <= H else H):
                yield line(cus, dtype, D, B, H, hk, N, M, causal, mask, bias, l2, groups, scale, ff=ff, kf=kf)
        # threshold shapes: workgroup counts of 256-position tiles around each boundary, made of B x H with H = 1 (exact counts) or 8 (GQA)
        targets = {1, 2, 3}
        for f in (1 / 8, 1 / 4, 1 / 2, 7 / 8, 1, 1.25, 1.5, 1.55, 1.6, 2, 2.55, 3):
            for d in (-1, 0, 1):
                targets.add(max(1, int(cus * f) + d))
        shapes = set()
        for t in sorted(targets):
            for n, ms in ((256, (256, 1000, 1024, 2048, 8192)), (512, (512, 1100, 2047)), (1024, (1024, 4096)), (4096, (4096, 1024)), (8192, (8192,))):
                tiles = (n + 255) // 256
                if t % tiles == 0 or t < tiles:
                    bh = max(1, t // tiles)
                    for m in ms:
                        shapes.add((bh, 1, n, m))
                        shapes.add(((bh + 7) // 8, 8, n, m))
        for dtype, D, causal, bias, (l2, scale), hk, (B, H, N, M) in itertools.product(
                (0, 1, 2), DIMS, (0, 1), (0, 1), ((0, 8.0), (1, 80.0)), ("H", "H/4"), sorted(shapes)):
            Hk = H if hk == "H" else H // 4
            if Hk < 1:
                continue
            for ff, kf in knobs(dtype, D, H, Hk):
                yield line(cus, dtype, D, B, H, Hk, N, M, causal, 0, bias, l2, 1, scale, ff=ff, kf=kf)
        # the 32-bit offset limit of the D = 128 wide forward: 1 MiB rows put (M + 384) rows of K past 2^31 bytes from M = 1664 on
        for dtype, causal, (B, H, N, M) in itertools.product((1, 2), (0, 1), ((cus // 8, 8, 256, 1600), (cus // 8, 8, 256, 1700),
                                                                          (cus // 4, 8, 512, 2048), (cus // 16, 8, 2048, 2048))):
            for rs in (0, 1 << 20):
                yield line(cus, dtype, 128, B, H, H, N, M, causal, rowstride=rs)
        # outputs whose (batch, head) is not one flat index ([B, L, H, D]): the split paths that need it step aside
        for dtype, D, causal, hk, (B, H, N, M) in itertools.product((0, 2), (64, 128), (0, 1), (8, 1, 2), ((1, 8, 1024, 8192), (1, 8, 8192, 1024))):
            yield line(cus, dtype, D, B, H, hk, N, M, causal, layout=1)
    yield from varlen_grid()


def varlen_grid(cus=256):
    """Packed sequences (fcsa_forward_varlen / fcsa_backward_varlen): every dtype x head dim x causal x shift / l2norm mode x K/V grouping
    on grids of S sequences x H heads x the tiles of max_seqlen on both sides of each threshold of tile_waves and choose_* -- the 7/8 of
    the CUs of an 8-wave grid, the CU count of 128-position tiles, a last round of 256-position tiles filled up to / beyond 55 %, and the
    >= 512 queries of the query-split dK/dV.  The dispatch reads only S x H and max_seqlen; the packed totals size the row kernels."""
    # (l2norm, groups or -1: non-fusable D // 4, scale: 80 = per-row shift)
    norms = ((0, 1, 1.0), (1, 1, 8.0), (1, 1, 80.0), (1, -1, 8.0))
    targets = {1, 2}
    for f in (1 / 2, 7 / 8, 1, 1.5, 1.55, 1.6, 2, 3):
        for d in (-1, 0, 1):
            targets.add(max(1, int(cus * f) + d))
    shapes = set()
    for t in sorted(targets):
        for n, ms in ((256, (256, 1000)), (512, (512, 300)), (1024, (1024, 2048))):
            tiles = (n + 255) // 256
            if t % tiles == 0 or t < tiles:
                s = max(1, t // tiles)
                for m in ms:
                    shapes.add((s, 1, n, m))
                    if s % 8 == 0:
                        shapes.add((s // 8, 8, n, m))
    for dtype, D, causal, (l2, g, scale), hk, (S, H, N, M) in itertools.product(
            (0, 1, 2), DIMS, (0, 1), norms, ("H", "H/4", "1"), sorted(shapes)):
        Hk = {"H": H, "H/4": H // 4, "1": 1}[hk]
        if Hk < 1 or (hk != "H" and H == 1):
            continue
        groups = (D // 4 if g < 0 else g) if l2 else 1
        yield line(cus, dtype, D, S, H, Hk, N, M, causal, 0, 0, l2, groups, scale, packed=(S * N // 2 + 1, S * M // 2 + 1))


def varlen_cover(log):
    """the lines of a recorded varlen_grid() the golden file keeps: a greedy cover of every kernel instantiation they launch and, per class
    of rows (element size, rows <= 128 bytes), every count of 256-position workgroups over the queries and over the keys"""
    def features(ln):
        f = ln.split()
        dtype, D, S, H, N, M, causal = (int(x) for x in (f[1], f[2], f[3], f[4], f[6], f[7], f[8]))
        rows = (dtype != 0, D * (4 if dtype == 0 else 2) <= 128)
        out = {p.split()[0] for p in ln.split(" | ", 1)[1].replace(" | ", "; ").split("; ")[1:]}
        for side, n in (("q", N), ("k", M)):
            t = (n + 255) // 256
            out.add((side, rows, S * H * ((t + 1) // 2 if causal else t)))
        return out
    lines = log.splitlines(keepends=True)
    feats = [features(ln) for ln in lines]
    todo, keep = set().union(*feats), []
    while todo:
        i = max(range(len(lines)), key=lambda j: (len(feats[j] & todo), -j))
        keep.append(i)
        todo -= feats[i]
    return [lines[i] for i in sorted(keep, key=lambda j: [float(x) for x in lines[j].split(" |")[0].split() if x != "varlen"])]


def parse(log):
    """{problem: its recorded line}"""
    return {ln.split(" |", 1)[0] + "\n": ln for ln in log.splitlines(keepends=True)}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_dispatch_header_is_host_only(tmp_path):
    """csrc/fcsa_dispatch.h compiles with plain g++ and no HIP headers (product and sweep builds)"""
    src = tmp_path / "t.cpp"
    src.write_text('#include "fcsa_dispatch.h"\n'
                   "int main() { fcsa::FwdProblem f{2, 64, 32, 4096, 4096, true, false, false, false, 1, 128, 128, 128, 1};\n"
                   "  return fcsa::choose_forward(f, 256) == fcsa::FwdForm::Rows8 ? 0 : 1; }\n")
    for extra in ([], ["-DFCSA_VAR_SPLIT_ENV"]):
        b = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *extra, "-I" + os.path.join(ROOT, "flash_cosine_sim_attention_amd", "csrc"),
                            str(src), "-o", str(tmp_path / "t")], capture_output=True, text=True, timeout=300)
        assert b.returncode == 0, b.stderr[-2000:]
        assert subprocess.run([str(tmp_path / "t")], timeout=60).returncode == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_tile_ownership(tmp_path):
    """the tile-ownership functions of csrc/fcsa_dispatch.h (tests/native/tile_work_check.cpp): the block mapping is a bijection onto
    (batch*head, pair), the passes visit every tile once, and each tile's split windows are disjoint and cover what the tile sees"""
    exe = str(tmp_path / "tile_work_check")
    b = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "flash_cosine_sim_attention_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "tile_work_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"), reason="needs g++ and the HIP headers")
def test_launches_match_golden(tmp_path):
    assert os.path.exists(LIB), "libfcsa_hip.so is not built"
    golden = open(GOLDEN).read()
    want = parse(golden)
    assert len(want) >= 200
    got = parse(record(build_recorder(tmp_path), LIB, list(want)))
    diff = [k for k in want if got.get(k) != want[k]]
    assert not diff, f"{len(diff)} of {len(want)} problems launch differently, first:\n--- golden\n{want[diff[0]]}--- now\n{got.get(diff[0])}"


if __name__ == "__main__":
    import tempfile
    lib = os.path.abspath(sys.argv[1])
    problems = list(dict.fromkeys(full_grid())) if "--full" in sys.argv else list(dict.fromkeys(varlen_grid())) if "--varlen" in sys.argv \
        else list(parse(open(GOLDEN).read()))
    with tempfile.TemporaryDirectory() as d:
        log = record(build_recorder(d), lib, problems)
        sys.stdout.write("".join(varlen_cover(log)) if "--varlen" in sys.argv else log)
