#!/usr/bin/env python3
"""The bits of the key/value-cache calls on a fixed, seeded table of small cases: per case the SHA-256 of o, of the log-sum-exp where the
call returns one, and of both caches after the append.  For refactors of fcsa_decode.hip / fcsa_prefill.hip / fcsa_decode_common.cuh that
must not move a bit: the bitwise tests compare one kernel of a build with another kernel of the same build, so a change common to both
passes them all.  Run once per library, each in its own process, and compare the two outputs as text:
    FCSA_LIB=.../libfcsa_hip_parent.so python tools/decode_bits.py > parent.txt;  python tools/decode_bits.py > new.txt;  cmp parent.txt new.txt
The table reaches: bf16 / f16 / float32 decode at D 16, 64, 96 (groups 4: the LDS form of the l2norm) and 128, both exponent regimes, l2norm
off, causal and not, G = 1 and 4, sequence lengths 0, 1, 31, 32, 33, 63, 64, 65, 129, rows without a visible key, a window, an fp8 cache, a
ragged batch (counts 1, 4, 0, 37), a paged cache with a shuffled table, caches long enough for tens of key splits, and the prefill kernel
(D 64 / 128) on the same lengths, the ragged batch and a 130-token chunk on 70 cached keys, and the engine step on a batch (counts 1, 4, 0,
37, 130) that takes both routes: 16-bit and fp8 caches, paged, windowed, and with the decode or the chunk launch skipped.  Digests are cut to 16 hex digits per tensor;
the last line is the SHA-256 over all the uncut ones.  Nothing is asserted: this is no test.
usage: decode_bits.py [--only SUBSTRING]"""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flash_cosine_sim_attention_amd as F  # noqa: E402

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
EDGES = [1, 31, 32, 33, 63, 64, 65, 129]
# scale per dtype: the static regime, the per-row-shift regime (as test_kvcache_regimes / test_bitwise_regimes choose them)
SCALES = {"bf16": (8.0, 120.0), "f16": (4.0, 16.0), "f32": (8.0, 120.0)}
ALL = hashlib.sha256()


def digest(t):
    if t.dtype in (torch.float8_e4m3fn,):
        t = t.view(torch.uint8)
    raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
    d = hashlib.sha256(raw).hexdigest()
    ALL.update(d.encode())
    return d[:16]


def show(name, **tensors):
    print(f"{name:58s} " + " ".join(f"{k}={digest(v)}" for k, v in tensors.items()), flush=True)


class Rnd:
    def __init__(self, name, dtype):
        self.g = torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(name.encode()).digest()[:7], "big"))
        self.dt = DT[dtype]

    def __call__(self, *shape, unit=False):
        x = torch.randn(*shape, generator=self.g, dtype=torch.float32)
        if unit:      # l2norm off: rows of unit length, so that the logits keep their usual range
            x = torch.nn.functional.normalize(x, dim=-1)
        return x.to(self.dt).cuda()


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def paged(kc, vc, page, seed):
    """[B, Hk, cap, D] -> a pool [B * cap / page + 3, Hk, page, D] behind a shuffled table (the spare blocks hold NaN)"""
    B, Hk, cap, D = kc.shape
    mb = cap // page
    perm = torch.randperm(B * mb + 3, generator=torch.Generator().manual_seed(seed))[:B * mb].reshape(B, mb).to(torch.int32)
    pools = []
    for c in (kc, vc):
        pool = torch.full((B * mb + 3, Hk, page, D), float("nan"), device="cuda", dtype=c.dtype)
        pool[perm.flatten().long().cuda()] = c.view(B, Hk, mb, page, D).transpose(1, 2).reshape(B * mb, Hk, page, D)
        pools.append(pool)
    return pools[0], pools[1], perm.cuda()


def decode(name, dtype, D, H, Hk, N, lens, append, cap=160, page=0, fp8=False, **kw):
    """flash_cosine_sim_attention_with_kvcache, without and with return_lse (two sets of combine entry points), on clones of the caches;
    lens = the sequence lengths after the append"""
    r = Rnd(name, dtype)
    unit = not kw.get("l2norm_qk", True)
    B = len(lens)
    q, kc, vc = r(B, H, N, D, unit=unit), r(B, Hk, cap, D, unit=unit), r(B, Hk, cap, D)
    kn, vn = (r(B, Hk, N, D, unit=unit), r(B, Hk, N, D)) if append else (None, None)
    sl = i32([max(L - (N if append else 0), 0) for L in lens])
    table = None
    if page:
        kc, vc, table = paged(kc, vc, page, seed=D)
    if fp8:
        kc, vc = (c.float().clamp(-448, 448).to(torch.float8_e4m3fn) for c in (kc, vc))
        kw = dict(kw, k_scale=torch.linspace(0.5, 2.0, B * Hk).view(B, Hk).cuda(), v_scale=torch.linspace(2.0, 0.25, B * Hk).view(B, Hk).cuda())
    with torch.no_grad():
        k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
        o = F.flash_cosine_sim_attention_with_kvcache(q, k1, v1, kn, vn, sl, block_table=table, **kw)
        o2, lse = F.flash_cosine_sim_attention_with_kvcache(q, k2, v2, kn, vn, sl, block_table=table, return_lse=True, **kw)
    torch.cuda.synchronize()
    show(name, o=o, o_lse=o2, lse=lse, k=k1, v=v1)


def packed(name, fn, dtype, D, H, Hk, counts, cached, append, cap=256, page=0, fp8=False, host_cu=False, **kw):
    """a packed step through fn (the ragged decode call, the prefill call or the engine step) with return_lse; cached = positions before
    the append; host_cu: the table on the host (the engine step then skips the launch that would find no sequence)"""
    r = Rnd(name, dtype)
    unit = not kw.get("l2norm_qk", True)
    B, total = len(counts), sum(counts)
    q, kc, vc = r(total, H, D, unit=unit), r(B, Hk, cap, D, unit=unit), r(B, Hk, cap, D)
    kn, vn = (r(total, Hk, D, unit=unit), r(total, Hk, D)) if append else (None, None)
    cu = i32([0] + [sum(counts[:b + 1]) for b in range(B)])
    if host_cu:
        cu = cu.cpu()
    table = None
    if page:
        kc, vc, table = paged(kc, vc, page, seed=D)
    if fp8:
        kc, vc = (c.float().clamp(-448, 448).to(torch.float8_e4m3fn) for c in (kc, vc))
        kw = dict(kw, k_scale=1.5, v_scale=torch.linspace(2.0, 0.25, B * Hk).view(B, Hk).cuda())
    with torch.no_grad():
        o, lse = fn(q, kc, vc, cu, kn, vn, i32(cached), block_table=table, return_lse=True, **kw)
    torch.cuda.synchronize()
    show(name, o=o, lse=lse, k=kc, v=vc)


def cases():
    ragged, prefill = F.flash_cosine_sim_attention_varlen_with_kvcache, F.flash_cosine_sim_attention_prefill_with_kvcache
    # the decode kernels: every dtype and head dim, both regimes, the block edges with an append (N = 3: lengths below 3 become 3) and
    # without one (length 0; lengths 1 under causal leave rows 0 and 1 without a visible key)
    i = 0
    for dtype in ("bf16", "f16", "f32"):
        for D, groups in ((16, 1), (64, 1), (96, 4), (128, 1)):
            for regime, scale in zip(("static", "per_row"), SCALES[dtype]):
                i += 1
                causal, Hk = i % 2 == 0, (4, 1)[(i // 2) % 2]
                for append in (True, False):
                    yield decode, (f"decode_{dtype}_d{D}_g{groups}_{regime}_{'causal' if causal else 'full'}_G{4 // Hk}_{'append' if append else 'read'}",
                                   dtype, D, 4, Hk, 3, [0] + EDGES, append), dict(scale=scale, groups=groups, causal=causal)
    for dtype, D in (("bf16", 64), ("f16", 128), ("f32", 64)):
        for causal in (False, True):
            yield decode, (f"decode_{dtype}_d{D}_no_l2norm_{'causal' if causal else 'full'}", dtype, D, 4, 1, 2, [0] + EDGES, not causal), \
                dict(scale=2.0, l2norm_qk=False, causal=causal)
    yield decode, ("decode_bf16_d64_window_20_5", "bf16", 64, 4, 1, 3, [0] + EDGES, True), dict(window_size=(20, 5))
    yield decode, ("decode_f16_d128_window_40_causal", "f16", 128, 4, 4, 2, [0] + EDGES, False), dict(window_size=(40, -1), causal=True, scale=16.0)
    yield decode, ("decode_bf16_d128_fp8", "bf16", 128, 4, 1, 3, [0] + EDGES, True), dict(fp8=True, causal=True)
    yield decode, ("decode_f16_d64_fp8_per_row_no_l2norm", "f16", 64, 4, 4, 1, [0] + EDGES, True), dict(fp8=True, scale=16.0, l2norm_qk=False)
    yield decode, ("decode_bf16_d64_paged16", "bf16", 64, 8, 2, 2, [0] + EDGES, True), dict(page=16, causal=True)
    yield decode, ("decode_f32_d128_paged32", "f32", 128, 4, 4, 1, [0] + EDGES, True), dict(page=32, scale=120.0)
    # tens of key splits (test_kvcache_many_splits_long_cache's shape)
    for dtype, D in (("bf16", 32), ("f16", 16), ("f32", 32)):
        for tag, kw in (("causal", dict(causal=True)), ("scale16_groups2", dict(scale=16.0, groups=2))):
            yield decode, (f"decode_{dtype}_d{D}_many_splits_{tag}", dtype, D, 4, 1, 3, [20000, 7777, 555], True), dict(cap=20000, **kw)
    # the ragged step and the prefill kernel on the same problems: a mixed batch, the block edges, a chunk with ragged tiles, waves and stages
    for call, fn in (("ragged", ragged), ("prefill", prefill)):
        for dtype in ("bf16", "f16"):
            for D in (64, 128):
                for regime, scale in zip(("static", "per_row"), SCALES[dtype]):
                    i += 1
                    causal, Hk = i % 2 == 0, (8, 2)[(i // 2) % 2]
                    tag = f"{call}_{dtype}_d{D}_{regime}_{'causal' if causal else 'full'}_G{8 // Hk}"
                    yield packed, (tag + "_mixed", fn, dtype, D, 8, Hk, [1, 4, 0, 37], [0, 17, 5, 63], True), dict(scale=scale, causal=causal)
                    yield packed, (tag + "_edges_append", fn, dtype, D, 8, Hk, [1] * 8, [L - 1 for L in EDGES], True), dict(scale=scale, causal=causal)
                    yield packed, (tag + "_edges_read", fn, dtype, D, 8, Hk, [3] * 9, [0] + EDGES, False), dict(scale=scale, causal=causal)
                    yield packed, (tag + "_130_on_70", fn, dtype, D, 8, Hk, [130], [70], True), dict(scale=scale, causal=not causal)
        yield packed, (f"{call}_bf16_d128_groups4_paged16", fn, "bf16", 128, 8, 2, [1, 4, 0, 37], [0, 17, 5, 63], True), \
            dict(groups=4, scale=2.0, causal=True, page=16)
        yield packed, (f"{call}_f16_d64_no_l2norm", fn, "f16", 64, 8, 8, [130], [70], True), dict(l2norm_qk=False, scale=1.0, causal=True)
    yield packed, ("ragged_bf16_d96_groups4_mixed", ragged, "bf16", 96, 8, 2, [1, 4, 0, 37], [0, 17, 5, 63], True), dict(groups=4, causal=True)
    yield packed, ("ragged_f32_d64_mixed", ragged, "f32", 64, 4, 1, [1, 4, 0, 37], [0, 17, 5, 63], True), dict(scale=120.0, causal=True)
    yield packed, ("ragged_f16_d128_fp8_mixed", ragged, "f16", 128, 8, 2, [1, 4, 0, 37], [0, 17, 5, 63], True), dict(fp8=True, causal=True)
    yield packed, ("ragged_bf16_d64_window_mixed", ragged, "bf16", 64, 8, 2, [1, 4, 0, 37], [0, 17, 5, 63], True), dict(window_size=(20, 0))
    # the engine step: G = 4, so chunk_rows = 128 sends the sequences of 37 and 130 rows to the chunk kernel and those of 1 and 4 rows to
    # the decode kernels; a host table with chunk_rows 0 / above every count skips the decode / the chunk launch (no_decode / no_chunk)
    step = F.flash_cosine_sim_attention_step_with_kvcache
    mixed = ([1, 4, 0, 37, 130], [0, 17, 5, 63, 70], True)
    yield packed, ("step_bf16_d64_static_causal_mixed", step, "bf16", 64, 8, 2, *mixed), dict(chunk_rows=128, causal=True)
    yield packed, ("step_f16_d128_per_row_full_mixed", step, "f16", 128, 8, 2, *mixed), dict(chunk_rows=128, scale=16.0)
    yield packed, ("step_f16_d128_fp8_mixed", step, "f16", 128, 8, 2, *mixed), dict(chunk_rows=128, fp8=True, causal=True)
    yield packed, ("step_bf16_d64_fp8_paged16_mixed", step, "bf16", 64, 8, 2, *mixed), dict(chunk_rows=128, fp8=True, page=16)
    yield packed, ("step_bf16_d64_window_mixed", step, "bf16", 64, 8, 2, *mixed), dict(chunk_rows=128, window_size=(20, 0))
    yield packed, ("step_bf16_d128_no_decode", step, "bf16", 128, 8, 2, *mixed), dict(chunk_rows=0, host_cu=True, causal=True)
    yield packed, ("step_f16_d64_no_chunk", step, "f16", 64, 8, 2, *mixed), dict(chunk_rows=10 ** 6, host_cu=True, causal=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_bits.py runs the GPU kernels: no GPU visible")
    for fn, args, kw in cases():
        if a.only in args[0]:
            fn(*args, **kw)
    print("all", ALL.hexdigest())


if __name__ == "__main__":
    main()
