#!/usr/bin/env python3
"""Bitwise A/B of the training front end against another build of libfcsa_hip.so (the parent commit's).

One forward + backward per route -- dense, dense with attn_bias, local, packed, packed local, attention states with and without an lse
gradient, ALiBi dense, local and packed -- with seeded inputs, at B 2, H 4, Hk 2, N = M = 16 (packed: 3 rows in two sequences) and at
N = M = 300 (more than one tile), D 64, bfloat16.  Each library runs in a process of its own (FCSA_LIB routes the ops to it), which
writes every output and gradient to a file; this process compares the two files with torch.equal.  Three processes in all, each child
under its own time limit.

    python tools/train_front_end_ab.py --other path/to/parent/libfcsa_hip.so [--out DIR]"""
import argparse, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def routes(N, lens):
    """{route: tensors} of one shape: N = M rows per batch entry, `lens` the sequence lengths of the packed calls"""
    import torch
    sys.path.insert(0, ROOT)
    import flash_cosine_sim_attention_amd as F
    B, H, HK, D, dev, dt = 2, 4, 2, 64, "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(1234 + N)
    rand = lambda *s: torch.randn(*s, device=dev, dtype=dt, generator=g)
    cu = torch.tensor([0] + [sum(lens[:i + 1]) for i in range(len(lens))], dtype=torch.int32, device=dev)
    total, longest, window = sum(lens), max(lens), (max(N // 3, 1), 0)
    slopes = torch.tensor([2.0 ** -(h + 1) for h in range(H)], device=dev)
    packed = dict(cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=longest, max_seqlen_k=longest)
    out = {}

    def run(name, fn, shape_q, shape_k, bias=None, d_lse=False):
        q, k, v = rand(*shape_q).requires_grad_(), rand(*shape_k).requires_grad_(), rand(*shape_k).requires_grad_()
        r = fn(q, k, v) if bias is None else fn(q, k, v, bias)
        o, lse = r if isinstance(r, tuple) else (r, None)
        grads = [rand(*o.shape)] + ([torch.randn(lse.shape, device=dev, generator=g)] if d_lse else [])
        torch.autograd.backward([o] + ([lse] if d_lse else []), grads)
        out[name] = [t.detach().cpu() for t in (o, lse, q.grad, k.grad, v.grad, None if bias is None else bias.grad) if t is not None]

    dq, dk, pq, pk = (B, H, N, D), (B, HK, N, D), (total, H, D), (total, HK, D)
    run("dense", lambda q, k, v: F.flash_cosine_sim_attention(q, k, v), dq, dk)
    run("dense causal", lambda q, k, v: F.flash_cosine_sim_attention(q, k, v, causal=True), dq, dk)
    run("dense with bias", lambda q, k, v, b: F.flash_cosine_sim_attention(q, k, v, attn_bias=b), dq, dk, bias=rand(H, N, N).requires_grad_())
    run("window", lambda q, k, v: F.flash_cosine_sim_attention_local(q, k, v, window), dq, dk)
    run("window that hides nothing", lambda q, k, v: F.flash_cosine_sim_attention_local(q, k, v, (-1, 0)), dq, dk)
    run("packed", lambda q, k, v: F.flash_cosine_sim_attention_varlen(q, k, v, causal=True, **packed), pq, pk)
    run("packed window", lambda q, k, v: F.flash_cosine_sim_attention_varlen(q, k, v, window_size=window, **packed), pq, pk)
    run("state", lambda q, k, v: F.flash_cosine_sim_attention_with_lse(q, k, v, causal=True), dq, dk)
    run("state with d_lse", lambda q, k, v: F.flash_cosine_sim_attention_with_lse(q, k, v, causal=True), dq, dk, d_lse=True)
    run("state window packed with d_lse", lambda q, k, v: F.flash_cosine_sim_attention_with_lse(q, k, v, window_size=window, **packed), pq, pk, d_lse=True)
    run("alibi dense", lambda q, k, v: F.flash_cosine_sim_attention_alibi(q, k, v, slopes, causal=True), dq, dk)
    run("alibi window", lambda q, k, v: F.flash_cosine_sim_attention_alibi(q, k, v, slopes, window_size=window), dq, dk)
    run("alibi packed", lambda q, k, v: F.flash_cosine_sim_attention_alibi(q, k, v, slopes, causal=True, **packed), pq, pk)
    torch.cuda.synchronize()
    return out


def child(path):
    import torch
    torch.save({f"N={N}: {name}": ts for N, lens in ((16, (1, 2)), (300, (120, 180))) for name, ts in routes(N, lens).items()}, path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="the libfcsa_hip.so to compare this tree's against")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help="where the two result files go (default: a temporary directory)")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    import torch
    out = a.out or tempfile.mkdtemp()
    os.makedirs(out, exist_ok=True)
    files = {}
    for label, lib in (("this tree", None), ("other", os.path.abspath(a.other))):
        files[label] = os.path.join(out, "train_ab_" + label.replace(" ", "_") + ".pt")
        env = {k: v for k, v in os.environ.items() if k != "FCSA_LIB"}
        if lib is not None:
            env["FCSA_LIB"] = lib
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", files[label]], env=env, check=True, timeout=240)
    mine, other = torch.load(files["this tree"]), torch.load(files["other"])
    assert mine.keys() == other.keys()
    print(f"bitwise A/B of the training routes: this tree's libfcsa_hip.so against {a.other}")
    bad = 0
    for name in mine:
        same = len(mine[name]) == len(other[name]) and all(torch.equal(x, y) for x, y in zip(mine[name], other[name]))
        finite = all(bool(torch.isfinite(x.float()).logical_or(torch.isneginf(x.float())).all()) for x in mine[name])
        bad += not (same and finite)
        print(f"  {name:44s} {len(mine[name])} tensors  {'equal' if same else 'DIFFERENT'}{'' if finite else '  NOT FINITE'}")
    print("all equal" if not bad else f"{bad} routes differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
