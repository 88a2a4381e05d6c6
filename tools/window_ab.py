#!/usr/bin/env python3
"""Sliding-window attention against what a caller runs without it, interleaved in ONE process: (a) the windowed call of this build,
(b) the dense causal call of another build of libfcsa_hip.so (the parent commit's: libfcsa_hip_<tag>.so), (c) that build's attn_bias route
on the 0 / -inf band; forward and forward + backward, median of --rounds rounds (device events around at least --steps calls and at least
20 ms of work, behind one untimed call that keeps the queue busy while the host enqueues).  (b) is taken twice per round, each time
after the ops were routed to the other library and back, and the run-to-run spread of a row is the largest deviation of those 2 x rounds
timings from their median: it covers switching libraries, which is what separates (a) from (b).  Conditions are judged with that spread
and nothing else.  Beside each row the share of key tiles the windowed forward visits, computed by the tile-ownership functions of
csrc/fcsa_dispatch.h themselves (a g++ helper built on the fly) for the row tile of the form that is launched; then per-kernel times of
one forward + backward (fcsa_profile_*), two float16 per-row-shift rows, and the decode rows of profiles/decode_ab.txt under a window.
usage: window_ab.py [--rounds R] [--steps S] [--tag parent] [--quick]"""
import argparse, ctypes, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flash_cosine_sim_attention_amd as F
from flash_cosine_sim_attention_amd import _lib, _torch_ops

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--tag", default="parent")
ap.add_argument("--quick", action="store_true", help="N = 4096 only")
a = ap.parse_args()
_torch_ops.load()
binding = ctypes.CDLL(_torch_ops.BINDING_PATH)
pkg = os.path.join(ROOT, "flash_cosine_sim_attention_amd")
LIBS = {"new": os.path.join(pkg, "libfcsa_hip.so"), "old": os.path.join(pkg, f"libfcsa_hip_{a.tag}.so")}


def use(which):
    rc = binding.fcsa_torch_use_library(LIBS[which].encode())
    assert rc == 0, (which, rc)


_steps = {}


def timed(fn, key=None):
    """us per call; `key` remembers the step count of a (shape, path) so that every round times the same amount of work"""
    steps = _steps.get(key)
    if steps is None:
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); fn(); e1.record()
        torch.cuda.synchronize()
        steps = max(a.steps, int(20e3 / max(e0.elapsed_time(e1) * 1e3 / 2, 1.0)) + 1)
        if key is not None:
            _steps[key] = steps
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()                      # untimed: the device is busy while the host enqueues the first timed call
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def spread_of(xs):
    m = statistics.median(xs)
    return max(abs(x - m) for x in xs) / m


_HELPER = r"""
#include <cstdio>
#include <cstdlib>
#include "fcsa_dispatch.h"
using namespace fcsa;
int main(int, char** argv) {      // D N left batch_heads cus -> row tile, key tiles visited windowed / causal
  const int D = atoi(argv[1]), N = atoi(argv[2]), left = atoi(argv[3]), bh = atoi(argv[4]), cus = atoi(argv[5]);
  FwdProblem f = {2, D, bh, N, N, true, false, false, false, 1, 2 * D, 2 * D, 2 * D, 1, true};
  const FwdForm form = choose_forward(f, cus);
  const int bm = (form == FwdForm::Rows8 || form == FwdForm::Lean8) ? 256 : 128, bn = 64;
  int lo, hi;
  win_normalise(N, N, true, left, 0, lo, hi);
  long win = 0, causal = 0;
  for (int m0 = 0; m0 < N; m0 += bm) {
    int k_lo, len;
    win_key_window(N, N, m0, bm, lo, hi, bn, k_lo, len);
    win += key_tiles(len, m0, bm, N - N + hi - k_lo, 1, bn);
    causal += key_tiles(N, m0, bm, 0, 1, bn);
  }
  std::printf("%d %ld %ld\n", bm, win, causal);
}
"""
_helper_exe = None


def tile_share(D, N, left, bh=32, cus=256):
    """(row tile of the launched form, key tiles visited windowed / causal) from fcsa_dispatch.h itself"""
    global _helper_exe
    import subprocess, tempfile
    if _helper_exe is None:
        d = tempfile.mkdtemp()
        open(os.path.join(d, "h.cpp"), "w").write(_HELPER)
        _helper_exe = os.path.join(d, "h")
        subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(pkg, "csrc"), os.path.join(d, "h.cpp"), "-o", _helper_exe], check=True)
    bm, win, causal = (int(x) for x in subprocess.run([_helper_exe, str(D), str(N), str(left), str(bh), str(cus)], check=True, capture_output=True,
                                                      text=True).stdout.split())
    return bm, win / causal


def kernel_times(which, fn, steps=5):
    """{kernel: mean us} of one call of fn on library `which` (fcsa_profile_*: an event pair around every launch)"""
    lib = ctypes.CDLL(LIBS[which])
    lib.fcsa_profile_enable.argtypes = [ctypes.c_int32]
    lib.fcsa_profile_collect.argtypes = [ctypes.POINTER(_lib.KernelStat), ctypes.c_int32]
    use(which)
    fn(); torch.cuda.synchronize()
    lib.fcsa_profile_enable(1)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    arr = (_lib.KernelStat * 16)()
    n = lib.fcsa_profile_collect(arr, 16)
    lib.fcsa_profile_enable(0)
    return {arr[i].name.decode(): arr[i].total_ms * 1e3 / steps for i in range(min(max(n, 0), 16))}


def band_bias(H, N, left, dt):
    i = torch.arange(N, device="cuda")[:, None]
    j = torch.arange(N, device="cuda")[None]
    ok = (j <= i) & (j >= i - left)
    b = torch.zeros(N, N, device="cuda", dtype=dt).masked_fill_(~ok, float("-inf"))
    return b.expand(H, N, N).contiguous()


def dense_rows():
    print(f"# tools/window_ab.py --rounds {a.rounds} --steps {a.steps}: bf16, (4, 8, N, D), causal, window (left, 0); median us per call")
    print("# a = windowed call (this build); b = dense causal call (parent build); c = parent build, attn_bias route on the 0 / -inf band")
    print("# spread = largest deviation of the 2 x rounds timings of b from their median, each taken after a switch of library; tiles = key tiles")
    print("# visited, windowed / causal (row tile of the launched form: 256 rows on these grids)")
    print(f"{'D':>4} {'N':>6} {'left':>5} {'tiles':>6} | {'a fwd':>8} {'b fwd':>8} {'b/a':>6} {'spread':>7} {'c fwd':>9} | {'a f+b':>8} {'b f+b':>8} {'b/a':>6} {'spread':>7} {'c f+b':>9}")
    verdict, perk = [], []
    dt = torch.bfloat16
    for D in (64, 128):
        for N in ((4096,) if a.quick else (4096, 8192, 16384)):
            q, k, v = (torch.randn(4, 8, N, D, device="cuda", dtype=dt, requires_grad=True) for _ in range(3))
            do = torch.randn(4, 8, N, D, device="cuda", dtype=dt)
            for left in (256, 1024, 4096):
                bias = band_bias(8, N, left, dt) if N <= 8192 else None

                def fwd(kind):
                    with torch.no_grad():
                        if kind == "a":
                            return F.flash_cosine_sim_attention_local(q, k, v, (left, 0), causal=True)
                        if kind == "b":
                            return F.flash_cosine_sim_attention(q, k, v, causal=True)
                        return F.flash_cosine_sim_attention(q, k, v, attn_bias=bias)

                def fb(kind):
                    if kind == "a":
                        o = F.flash_cosine_sim_attention_local(q, k, v, (left, 0), causal=True)
                    elif kind == "b":
                        o = F.flash_cosine_sim_attention(q, k, v, causal=True)
                    else:
                        o = F.flash_cosine_sim_attention(q, k, v, attn_bias=bias)
                    o.backward(do)
                    q.grad = k.grad = v.grad = None

                t = {k_: [] for k_ in ("af", "bf", "bf2", "cf", "ab", "bb", "bb2", "cb")}
                for r in range(a.rounds + 1):      # round 0 warms every path up
                    for kind, lib in (("a", "new"), ("b", "old"), ("c", "old"), ("b2", "old")):
                        if kind == "c" and bias is None:
                            continue
                        if kind == "b2":
                            use("new")      # (the repeat of b also follows a switch of library)
                        use(lib)
                        kk = kind[0]
                        f_us, b_us = timed(lambda: fwd(kk), (D, N, left, kk, "f")), timed(lambda: fb(kk), (D, N, left, kk, "b"))
                        if r:
                            t[kind[0] + "f" + kind[1:]].append(f_us)
                            t[kind[0] + "b" + kind[1:]].append(b_us)
                use("new")
                med = {k_: (statistics.median(x) if x else float("nan")) for k_, x in t.items()}
                sp_f, sp_b = spread_of(t["bf"] + t["bf2"]), spread_of(t["bb"] + t["bb2"])
                med["bf"], med["bb"] = statistics.median(t["bf"] + t["bf2"]), statistics.median(t["bb"] + t["bb2"])
                print(f"{D:>4} {N:>6} {left:>5} {tile_share(D, N, left)[1]:>6.2f} | {med['af']:>8.1f} {med['bf']:>8.1f} {med['bf'] / med['af']:>6.2f} {sp_f:>7.1%} {med['cf']:>9.1f} | "
                      f"{med['ab']:>8.1f} {med['bb']:>8.1f} {med['bb'] / med['ab']:>6.2f} {sp_b:>7.1%} {med['cb']:>9.1f}", flush=True)
                if left <= N // 4:
                    verdict.append((D, N, left, med["af"] < med["bf"] * (1 - sp_f), med["ab"] < med["bb"] * (1 - sp_b)))
                elif left >= N:
                    verdict.append((D, N, left, abs(med["af"] - med["bf"]) <= med["bf"] * sp_f, abs(med["ab"] - med["bb"]) <= med["bb"] * sp_b))
                if N == 16384 or (N == 4096 and left == 4096):      # per kernel, one forward + backward: the long rows, and the row where a IS b
                    ka, kb = kernel_times("new", lambda: fb("a")), kernel_times("old", lambda: fb("b"))
                    perk.append(f"{D:>4} {N:>6} {left:>5} | a: " + "  ".join(f"{k_} {v_:.1f}" for k_, v_ in sorted(ka.items())) +
                                " | b: " + "  ".join(f"{k_} {v_:.1f}" for k_, v_ in sorted(kb.items())))
                    use("new")
                del bias
            del q, k, v, do
    bad = [x[:3] + (("fwd",) if not x[3] else ()) + (("fwd+bwd",) if not x[4] else ()) for x in verdict if not (x[3] and x[4])]
    print(f"condition (left <= N / 4: a faster than b by more than the row's spread; left >= N: equal within it), forward and forward + backward, "
          f"{len(verdict)} rows: {'met on all' if not bad else 'NOT met on ' + str(bad)}")
    print("# per kernel, us per launch, one forward + backward (event pair around every launch; a = windowed, b = dense causal of the parent build)")
    for ln in perk:
        print(ln)


def per_row_rows():
    print("# float16, scale 16 (the per-row-shift regime: fwd_win<.., DYN> forms), (4, 8, 8192, D), window (1024, 0), same protocol")
    print(f"{'D':>4} | {'a fwd':>8} {'b fwd':>8} {'b/a':>6} {'spread':>7} | {'a f+b':>8} {'b f+b':>8} {'b/a':>6} {'spread':>7}")
    dt, N, left = torch.float16, 8192, 1024
    for D in (64, 128):
        q, k, v = (torch.randn(4, 8, N, D, device="cuda", dtype=dt, requires_grad=True) for _ in range(3))
        do = torch.randn(4, 8, N, D, device="cuda", dtype=dt)

        def call(kind, grad):
            with torch.enable_grad() if grad else torch.no_grad():
                o = F.flash_cosine_sim_attention_local(q, k, v, (left, 0), causal=True, scale=16.0) if kind == "a" else \
                    F.flash_cosine_sim_attention(q, k, v, causal=True, scale=16.0)
                if grad:
                    o.backward(do)
                    q.grad = k.grad = v.grad = None

        t = {x: [] for x in ("af", "bf", "ab", "bb")}
        for r in range(a.rounds + 1):
            for kind, lib in (("a", "new"), ("b", "old"), ("b", "old")):
                use("new"); use(lib)
                f_us, b_us = timed(lambda: call(kind, False), ("pr", D, kind, "f")), timed(lambda: call(kind, True), ("pr", D, kind, "b"))
                if r:
                    t[kind + "f"].append(f_us); t[kind + "b"].append(b_us)
        use("new")
        m = {x: statistics.median(y) for x, y in t.items()}
        print(f"{D:>4} | {m['af']:>8.1f} {m['bf']:>8.1f} {m['bf'] / m['af']:>6.2f} {spread_of(t['bf']):>7.1%} | {m['ab']:>8.1f} {m['bb']:>8.1f} "
              f"{m['bb'] / m['ab']:>6.2f} {spread_of(t['bb']):>7.1%}", flush=True)


def decode_rows():
    print("# decode: bf16, causal, N = 1, left = 4096 against the parent build's full-length call; GB/s over the K + V bytes a windowed call reads; copy rate 6300 GB/s")
    print(f"{'shape':<24} {'a us':>8} {'b us':>8} {'b/a':>6} {'spread':>7} {'read MB':>8} {'GB/s':>7} {'% copy':>7}")
    dt = torch.bfloat16
    for B in (1, 8):
        H, Hk, L, D, left = 32, 8, 32768, 128, 4096
        q = torch.randn(B, H, 1, D, device="cuda", dtype=dt)
        kc, vc = (torch.randn(B, Hk, L, D, device="cuda", dtype=dt) for _ in range(2))
        with torch.no_grad():
            fa = lambda: F.flash_cosine_sim_attention_with_kvcache(q, kc, vc, causal=True, window_size=(left, 0))
            fb = lambda: F.flash_cosine_sim_attention_with_kvcache(q, kc, vc, causal=True)
            ta, tb, tb2 = [], [], []
            for r in range(a.rounds + 1):
                use("new"); x = timed(fa, ("dec", B, "a"))
                use("old"); y = timed(fb, ("dec", B, "b")); use("new"); use("old"); y2 = timed(fb, ("dec", B, "b"))
                if r:
                    ta.append(x); tb.append(y); tb2.append(y2)
            use("new")
        ma, mb = statistics.median(ta), statistics.median(tb)
        sp = spread_of(tb + tb2)
        mb = statistics.median(tb + tb2)
        mb_read = B * Hk * (left + 1 + 31) * D * 2 * 2 / 1e6
        print(f"B{B} H{H} Hk{Hk} L32k D{D:<8} {ma:>8.1f} {mb:>8.1f} {mb / ma:>6.2f} {sp:>7.1%} {mb_read:>8.1f} {mb_read / ma * 1e3:>7.0f} {mb_read / ma * 1e3 / 6300:>7.1%}",
              flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    dense_rows()
    per_row_rows()
    decode_rows()
