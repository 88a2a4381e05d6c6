#!/usr/bin/env python3
"""Where does the per-call host time of a tiny forward+backward go?  (B4 H8 N128 D64 bf16 causal: the GPU work is ~40 us, so
every number here is host-bound.)  Prints us per call for nested slices of the call path, the same for SDPA, and then every call of the
key/value-cache family."""
import os, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flash_cosine_sim_attention_amd as F
from flash_cosine_sim_attention_amd import _torch_ops
fc = _torch_ops.load()
N = int(sys.argv[1]) if len(sys.argv) > 1 else 128
q, k, v = (torch.randn(4, 8, N, 64, device="cuda", dtype=torch.bfloat16, requires_grad=True) for _ in range(3))
qd, kd, vd = q.detach(), k.detach(), v.detach()
do = torch.randn_like(qd)
def bench(name, fn, n=300):
    for _ in range(30): fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize()
    print(f"{name:58s} {(time.perf_counter() - t0) / n * 1e6:8.1f} us")
bench("torch.ops.fcsa.forward (no backward state)", lambda: fc.forward(qd, kd, vd, None, None, False, 8.0, True, True, 1, False))
bench("torch.ops.fcsa.forward (with backward state)", lambda: fc.forward(qd, kd, vd, None, None, False, 8.0, True, True, 1, True))
st = fc.forward(qd, kd, vd, None, None, False, 8.0, True, True, 1, True)
bench("torch.ops.fcsa.backward", lambda: fc.backward(do, st[0], st[1], qd, kd, vd, None, None, st[2], st[3], st[4], st[5], False, 8.0, True, True, 1, False))
bench("flash_cosine_sim_attention, no grad", lambda: F.flash_cosine_sim_attention(qd, kd, vd, causal=True))
bench("flash_cosine_sim_attention, grad (forward only)", lambda: F.flash_cosine_sim_attention(q, k, v, causal=True))
def fb():
    q.grad = k.grad = v.grad = None
    F.flash_cosine_sim_attention(q, k, v, causal=True).backward(do)
import ctypes
_b = ctypes.CDLL(_torch_ops.BINDING_PATH)
_cnt = (ctypes.c_uint64 * 8)()
_b.fcsa_torch_host_ns(_cnt)                    # reset the binding's host-time counters
bench("forward + backward(dO)", fb)
_b.fcsa_torch_host_ns(_cnt)
nf, nb = max(_cnt[6], 1), max(_cnt[7], 1)
print("   inside the binding, us per call: forward checks %.1f | allocations %.1f | fcsa_forward %.1f || backward checks %.1f | allocations %.1f | fcsa_backward %.1f"
      % (_cnt[0] / nf / 1e3, _cnt[1] / nf / 1e3, _cnt[2] / nf / 1e3, _cnt[3] / nb / 1e3, _cnt[4] / nb / 1e3, _cnt[5] / nb / 1e3))
def fbs():
    q.grad = k.grad = v.grad = None
    F.flash_cosine_sim_attention(q, k, v, causal=True).sum().backward()
bench("forward + sum().backward()   [benchmark.py protocol]", fbs)
def sd():
    q.grad = k.grad = v.grad = None
    torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True).sum().backward()
bench("SDPA forward + sum().backward()", sd)
bench("SDPA forward only (grad)", lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True))
bench("torch.empty x 6", lambda: [torch.empty(4, 8, N, 64, device="cuda", dtype=torch.bfloat16) for _ in range(6)])
# The training operators that take an option -- a window, packed sequences, the lse, slopes -- forward + backward on the same problem (the
# packed call: the same rows as 4 sequences of N), device tables and max_seqlen given: no call reads a device tensor on the host
tq, tk, tv = (t.detach().transpose(1, 2).reshape(4 * N, 8, 64).contiguous().requires_grad_() for t in (q, k, v))
tdo = do.transpose(1, 2).reshape(4 * N, 8, 64).contiguous()
tcu = torch.arange(5, dtype=torch.int32, device="cuda") * N
tslopes = torch.tensor([2.0 ** -(h + 1) for h in range(8)], device="cuda")
def train(fn, leaves, g):
    def run():
        for t in leaves: t.grad = None
        fn().backward(g)
    return run
bench("flash_cosine_sim_attention_local, forward + backward", train(lambda: F.flash_cosine_sim_attention_local(q, k, v, (N // 2, 0), causal=True), (q, k, v), do))
bench("flash_cosine_sim_attention_varlen, forward + backward",
      train(lambda: F.flash_cosine_sim_attention_varlen(tq, tk, tv, tcu, tcu, max_seqlen_q=N, max_seqlen_k=N, causal=True), (tq, tk, tv), tdo))
bench("flash_cosine_sim_attention_with_lse, forward + backward", train(lambda: F.flash_cosine_sim_attention_with_lse(q, k, v, causal=True)[0], (q, k, v), do))
bench("flash_cosine_sim_attention_alibi, forward + backward", train(lambda: F.flash_cosine_sim_attention_alibi(q, k, v, tslopes, causal=True), (q, k, v), do))
# Decoding against a key/value cache is launch-bound (an append-free step is two launches of a few us), so the host time of its call path
# is part of its speed: B4 H8 Hk2 N1 D64 bf16 against a full cache of 256 positions, device tables and max_seqlen_k given (no call
# reads a device tensor on the host)
B, H, Hk, D, L = 4, 8, 2, 64, 256
dq = torch.randn(B, H, 1, D, device="cuda", dtype=torch.bfloat16)
kc, vc = (torch.randn(B, Hk, L, D, device="cuda", dtype=torch.bfloat16) for _ in range(2))
k8, v8 = kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)
ones = torch.ones(B, Hk, device="cuda")
step = dict(cache_seqlens=torch.full((B,), L, dtype=torch.int32, device="cuda"), max_seqlen_k=L, causal=True)
pq = dq.reshape(B, H, D)                      # the same queries packed [total_q, H, D], one per sequence
cu = torch.arange(B + 1, dtype=torch.int32, device="cuda")
bench("kvcache decode", lambda: F.flash_cosine_sim_attention_with_kvcache(dq, kc, vc, **step))
bench("kvcache decode, fp8 cache", lambda: F.flash_cosine_sim_attention_with_kvcache(dq, k8, v8, k_scale=ones, v_scale=ones, **step))
bench("kvcache decode, ragged step", lambda: F.flash_cosine_sim_attention_varlen_with_kvcache(pq, kc, vc, cu, max_seqlen_q=1, **step))
bench("kvcache decode, return_lse", lambda: F.flash_cosine_sim_attention_with_kvcache(dq, kc, vc, return_lse=True, **step))
# the packed calls on the same tiny problem: one query row per sequence, so every line is two or three launches
bench("kvcache engine step", lambda: F.flash_cosine_sim_attention_step_with_kvcache(pq, kc, vc, cu, max_seqlen_q=1, **step))
bench("kvcache prefill", lambda: F.flash_cosine_sim_attention_prefill_with_kvcache(pq, kc, vc, cu, max_seqlen_q=1, **step))
chain = torch.ones(B, dtype=torch.int64, device="cuda")      # one token per sequence: bit 0, the chain mask
tree = dict(step, causal=False)
bench("kvcache tree step, chain mask", lambda: F.flash_cosine_sim_attention_tree_with_kvcache(pq, kc, vc, cu, max_seqlen_q=1, tree_mask=chain, **tree))
slopes = torch.tensor([2.0 ** -(h + 1) for h in range(H)], device="cuda")
bench("kvcache engine step, alibi_slopes", lambda: F.flash_cosine_sim_attention_alibi_with_kvcache(pq, kc, vc, cu, max_seqlen_q=1, alibi_slopes=slopes, **step))
# the compaction after a tree step: the first two of four drafted tokens kept (they stay where they are; the launch is the same)
seqlens = torch.full((B,), L - 4, dtype=torch.int32, device="cuda")
accepted = torch.arange(4, dtype=torch.int32, device="cuda").repeat(B, 1)
kept = torch.full((B,), 2, dtype=torch.int32, device="cuda")
bench("kvcache_keep_accepted", lambda: F.kvcache_keep_accepted(kc, vc, seqlens, accepted, kept))
