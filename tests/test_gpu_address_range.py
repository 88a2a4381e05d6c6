"""The packed, cached and windowed calls far from their tensors' bases: beyond 4 GiB (every per-slice base has to be 64-bit: the
`first * sn` of varlen_rebase and the per-row buffers moved by `qrow`, the block-table lookup times `sb` of cache_base) and along the
kernels' 32-bit tile offsets (a byte offset per tile that is re-opened once it passes 1 GiB; a windowed key range STARTS at k_lo, so
its first offset is already large).

Every comparison is BIT FOR BIT against the same call on compact data -- same dtype, D, batch x heads and lengths, so the same
instantiation, grid and splits (test_fullsize_feature_launches_cpu.py records one line for both); only the addresses differ.  The two
exceptions are the slice-only runs of the packed and the dense > 4 GiB tensors (other grids), which are judged like the whole tensor by
the existing bars against a float64 slice.  "The same launches" rests on one assumption: the dispatch reads no stride except in
fwd3_applies (the row pitch), which test_fullsize_feature_launches_cpu.py checks -- the recorder is given no batch, block or position
stride.  Each test makes one float64-slice check, so "both wrong the same way" is excluded.
The shapes live in tests/fullsize_feature_cases.py (ADDR_*)."""
import pytest
import torch

import fullsize_feature_cases as FC
import fullsize_reference as FR
import test_gpu_fullsize_features as TF

pytestmark = pytest.mark.gpu

DT = FR.DT
INT = {"bf16": torch.int16, "f16": torch.int16, "f32": torch.int32}
GIB = 2 ** 30


def _F():
    import flash_cosine_sim_attention_amd as F
    return F


def _rand(shape, dtype, g):
    return torch.randn(shape, device="cuda", dtype=torch.float32, generator=g).to(DT[dtype])


def _same_bytes(a, b, dtype, chunk=512):
    """integer views (NaN compares equal), in chunks of the first dimension"""
    ia, ib = a.view(INT[dtype]), b.view(INT[dtype])
    return all(torch.equal(ia[i:i + chunk], ib[i:i + chunk]) for i in range(0, a.shape[0], chunk))


# ---- paged pool beyond 4 GiB (float32: beyond 2^31 elements) ------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,nb,lines", FC.ADDR_POOLS, ids=[p[0] for p in FC.ADDR_POOLS])
def test_paged_pool_beyond_4_gib(dtype, nb, lines):
    """K and V pools in vLLM's [num_blocks, page, Hk, D] layout passed as .transpose(1, 2); the block tables use block 0, the blocks on
    both sides of the 2 GiB and 4 GiB (float32: and 8 GiB) lines and the last block; every block outside the table is NaN.  N = 1 and
    N = 5 (the second under a window), appends that land in the last block and across two far blocks.  Identical bits to the same
    sequences in a compact pool with a renumbered table; the appended slots hold k_new / v_new; every other byte of the pools is unchanged."""
    page, Hk, H, D = FC.ADDR_PAGE, FC.ADDR_HK, FC.ADDR_H, FC.ADDR_D
    es = torch.empty((), dtype=DT[dtype]).element_size()
    TF._need(4.5 * nb * page * Hk * D * es / GIB + 4)
    g = torch.Generator(device="cuda").manual_seed(nb)
    table = FC.addr_pool_table(nb, lines)
    used = sorted(b for row in table for b in row)
    raw_k = torch.full((nb, page, Hk, D), float("nan"), device="cuda", dtype=DT[dtype])
    raw_v = torch.full((nb, page, Hk, D), float("nan"), device="cuda", dtype=DT[dtype])
    assert raw_k.numel() * es > 4.4 * GIB and (dtype != "f32" or raw_k.numel() > 2 ** 31)
    assert used[-1] * page * Hk * D * es > 4 * GIB
    for blk in used:
        raw_k[blk], raw_v[blk] = _rand((page, Hk, D), dtype, g), _rand((page, Hk, D), dtype, g)
    small_k, small_v = raw_k[used].clone(), raw_v[used].clone()
    small_table = torch.tensor([[used.index(b) for b in row] for row in table], dtype=torch.int32)
    big_table = torch.tensor(table, dtype=torch.int32)
    want_k, want_v = raw_k.clone(), raw_v.clone()
    j = TF.Judge(f"paged_pool_{dtype}", dtype)
    for N, n_new, lens, window, kw in FC.ADDR_POOL_CALLS:
        q, kn, vn = _rand((3, H, N, D), dtype, g), _rand((3, Hk, n_new, D), dtype, g), _rand((3, Hk, n_new, D), dtype, g)
        o_far = TF._decode(q, raw_k.transpose(1, 2), raw_v.transpose(1, 2), kn, vn, lens, big_table, window, kw)
        o_near = TF._decode(q, small_k.transpose(1, 2), small_v.transpose(1, 2), kn, vn, lens, small_table, window, kw)
        assert torch.isfinite(o_far).all()
        assert torch.equal(o_far, o_near), (dtype, N, "the far pool gives other bits than the compact pool")
        for b, n0 in enumerate(lens):
            for t in range(n_new):
                blk, slot = table[b][(n0 + t) // page], (n0 + t) % page
                assert torch.equal(raw_k[blk, slot], kn[b, :, t]) and torch.equal(raw_v[blk, slot], vn[b, :, t]), (dtype, N, b, t)
                want_k[blk, slot], want_v[blk, slot] = kn[b, :, t], vn[b, :, t]
        assert _same_bytes(raw_k, want_k, dtype) and _same_bytes(raw_v, want_v, dtype), "a byte of the pool outside the appended slots changed"
        assert torch.equal(small_k, raw_k[used]) and torch.equal(small_v, raw_v[used])
        # one float64 slice: sequence 0 (its last block is the pool's last), the last K/V head
        L, hk = lens[0] + n_new, Hk - 1
        ks, vs = (FR.sequence_of_cache(c.transpose(1, 2), 0, L, big_table) for c in (raw_k, raw_v))
        G = H // Hk
        TF.compare_slice(j, "address/paged", f"N={N}", dtype, kw, window, (o_far[0, hk * G:(hk + 1) * G],), (q[0, hk * G:(hk + 1) * G], ks[hk], vs[hk]))
    j.done()


def test_contiguous_cache_beyond_4_gib():
    """a [B, Hk, capacity, D] bf16 cache of 4.8 GB read through a batch-strided view (sequences 0, 35 and 70: the last one lies past the
    4 GiB line) against a contiguous copy of those three sequences"""
    c = FC.ADDR_CONTIG
    B, Hk, H, D, cap = c["B"], FC.ADDR_HK, FC.ADDR_H, FC.ADDR_D, c["cap"]
    TF._need(24)
    g = torch.Generator(device="cuda").manual_seed(7)
    big_k, big_v = _rand((B, Hk, cap, D), "bf16", g), _rand((B, Hk, cap, D), "bf16", g)
    far_k, far_v = big_k[::c["step"]], big_v[::c["step"]]
    assert far_k.shape[0] == 3 and far_k.stride(0) * 2 * 2 > 4 * GIB and big_k.numel() * 2 > 4.4 * GIB
    near_k, near_v = far_k.contiguous(), far_v.contiguous()
    want_k, want_v = big_k.clone(), big_v.clone()
    q, kn, vn = _rand((3, H, 1, D), "bf16", g), _rand((3, Hk, 1, D), "bf16", g), _rand((3, Hk, 1, D), "bf16", g)
    kw = dict(causal=True)
    o_far = TF._decode(q, far_k, far_v, kn, vn, c["lens"], None, (-1, -1), kw)
    o_near = TF._decode(q, near_k, near_v, kn, vn, c["lens"], None, (-1, -1), kw)
    assert torch.isfinite(o_far).all() and torch.equal(o_far, o_near)
    for b, n0 in enumerate(c["lens"]):
        assert torch.equal(far_k[b, :, n0], kn[b, :, 0]) and torch.equal(far_v[b, :, n0], vn[b, :, 0])
        want_k[b * c["step"], :, n0], want_v[b * c["step"], :, n0] = kn[b, :, 0], vn[b, :, 0]
    assert _same_bytes(big_k, want_k, "bf16", 4) and _same_bytes(big_v, want_v, "bf16", 4), "a byte of the cache outside the appended slots changed"
    j = TF.Judge("contiguous_cache", "bf16")
    G = H // Hk
    TF.compare_slice(j, "address/contiguous-cache", "[2,7]", "bf16", kw, (-1, -1), (o_far[2, -G:],), (q[2, -G:], far_k[2, -1, :cap], far_v[2, -1, :cap]))
    j.done()


# ---- packed tensors beyond 4 GiB ----------------------------------------------------------------------------------------------------------

def test_packed_tensors_beyond_4_gib():
    """q, k, v, dO [total, 32, 128] bf16 of 4.8 GB each: the first sequence, the one that straddles the 4 GiB line and the last two (whose
    rows lie beyond it, in q / k / v / dO / o, the gradients and the saved qn_out / kn_out; the one-float-per-(head, row) buffers rq / rk /
    inv_l / delta are moved by the same qrow, up to 1.9e7 rows, but hold 75 MB and cannot reach 4 GiB below the library's refusal of
    heads x packed rows >= 2^31), forward and backward, against a float64 slice -- and the packed call on those sequences alone (another grid: the one place with two instantiations), judged the same."""
    lens, check = FC.ADDR_PACKED, FC.ADDR_PACKED_CHECK
    H, D = 32, 128
    TF._need(80)
    g = torch.Generator(device="cuda").manual_seed(43)
    total = sum(lens)
    q, k, v, do = (_rand((total, H, D), "bf16", g) for _ in range(4))
    assert q.numel() * 2 > 4.4 * GIB
    cu = TF.TV._cu(lens)
    off = cu.tolist()
    assert off[check[1]] * H * D * 2 < 4 * GIB < off[check[1] + 1] * H * D * 2 and off[check[2]] * H * D * 2 > 4 * GIB
    kw = dict(causal=True)
    got = TF._run_packed(q, k, v, do, cu, cu, None, (-1, -1), kw)
    for t in got:
        assert torch.isfinite(t).all()
    rows = torch.cat([torch.arange(off[s], off[s + 1], device="cuda") for s in check])
    alone_lens = [lens[s] for s in check]
    cua = TF.TV._cu(alone_lens)
    alone = TF._run_packed(q[rows], k[rows], v[rows], do[rows], cua, cua, None, (-1, -1), kw)
    offa = cua.tolist()
    j = TF.Judge("packed_beyond_4gib", "bf16")
    for i, s in enumerate(check):
        for h in (0, H - 1):
            for name, res, sl in (("whole", got, slice(off[s], off[s + 1])), ("alone", alone, slice(offa[i], offa[i + 1]))):
                side = lambda t: t[sl][:, h:h + 1].permute(1, 0, 2)
                ins = slice(off[s], off[s + 1])
                TF.compare_slice(j, "address/packed-" + name, f"[seq {s} ({lens[s]}),{h}]", "bf16", kw, (-1, -1),
                                 (side(res[0]), side(res[1]), res[2][sl][:, h], res[3][sl][:, h]),
                                 (q[ins][:, h:h + 1].permute(1, 0, 2), k[ins][:, h], v[ins][:, h], do[ins][:, h:h + 1].permute(1, 0, 2)),
                                 factor=TF.short_factor(lens[s]), few_keys=lens[s] <= 8)
    j.done()


# ---- windowed dense call beyond 4 GiB -------------------------------------------------------------------------------------------------------

def test_windowed_dense_tensors_beyond_4_gib():
    """the shape of test_tensors_beyond_4_gib_address_the_last_head_correctly under window_size = (1024, 0): the first, a middle and the
    last (batch, head) against a float64 slice, and against the slice-only run (another grid) by the same bars"""
    B, H, N, D, window = FC.ADDR_DENSE
    TF._need(80)
    g = torch.Generator(device="cuda").manual_seed(41)
    q, k, v, do = (_rand((B, H, N, D), "bf16", g) for _ in range(4))
    assert q.numel() * 2 > 4.4 * GIB
    kw = dict(causal=True)
    got = TF._run_local(q, k, v, do, window, kw)
    j = TF.Judge("window_dense_beyond_4gib", "bf16")
    for b, h in ((0, 0), (B // 2, 3), (B - 1, H - 1)):
        sl = (slice(b, b + 1), slice(h, h + 1))
        alone = TF._run_local(q[sl], k[sl], v[sl], do[sl], window, kw)
        for name, res in (("whole", tuple(t[b, h] for t in got)), ("alone", tuple(t[0, 0] for t in alone))):
            TF.compare_slice(j, "address/window-dense-" + name, f"[{b},{h}]", "bf16", kw, window, (res[0][None], res[1][None], res[2], res[3]),
                             (q[b, h][None], k[b, h], v[b, h], do[b, h][None]))
    j.done()


# ---- 32-bit tile offsets: rows 1 MiB apart ---------------------------------------------------------------------------------------------------

def _wide(shape, dtype, g, amp=1.0):
    """a [..., rows, D] tensor whose rows are FC.PITCH bytes apart (a view of a padded backing tensor), random data"""
    pad = FC.PITCH // torch.empty((), dtype=DT[dtype]).element_size()
    view = torch.empty(tuple(shape[:-1]) + (pad,), device="cuda", dtype=DT[dtype])[..., :shape[-1]]
    view.copy_(_rand(shape, dtype, g) * amp)
    assert not view.is_contiguous() and view.stride(-2) * view.element_size() == FC.PITCH
    return view


def _bits_equal(a, b, what):
    for x, y, nm in zip(a, b, ("o", "dq", "dk", "dv")):
        assert torch.isfinite(x).all(), (what, nm)
        assert torch.equal(x, y), (what, nm, "the strided call gives other bits than the contiguous copy")


@pytest.mark.parametrize("rows,D,window,kw", FC.ADDR_PITCH_DENSE, ids=[f"n{c[0]}_d{c[1]}_w{c[2][0]}_{c[2][1]}" for c in FC.ADDR_PITCH_DENSE])
def test_window_walks_the_32bit_tile_offsets(rows, D, window, kw):
    """dense windowed call, rows 1 MiB apart: the key range of a row tile starts at k_lo x 1 MiB from the slice base -- beyond 1 GiB, 2 GiB
    and (4608 rows) 4 GiB.  Identical bits to contiguous copies, o and all three gradients."""
    TF._need(rows * 4 / 1024 + 4)
    g = torch.Generator(device="cuda").manual_seed(rows + D)
    amp = 1.0 if kw.get("l2norm_qk", True) else 0.35
    q, k, v, do = (_wide((1, 1, rows, D), "bf16", g, amp) for _ in range(4))
    assert (rows - 1 - window[0]) * FC.PITCH > (4 if rows > 4400 else 1) * GIB and rows * FC.PITCH > 2 * GIB
    far = TF._run_local(q, k, v, do, window, kw)
    near = TF._run_local(q.contiguous(), k.contiguous(), v.contiguous(), do.contiguous(), window, kw)
    _bits_equal(far, near, "dense window")
    j = TF.Judge(f"pitch_dense_n{rows}_d{D}", "bf16")
    TF.compare_slice(j, "address/pitch-window", "", "bf16", kw, window, tuple(t[0, 0][None] if i < 2 else t[0, 0] for i, t in enumerate(far)),
                     (q[0, 0][None], k[0, 0], v[0, 0], do[0, 0][None]))
    j.done()


@pytest.mark.parametrize("window", [(-1, -1), (300, 0)], ids=["plain", "w300"])
def test_packed_sequences_walk_the_32bit_tile_offsets(window):
    """a packed batch whose backing is [total, 1, pad]: the sequences begin beyond 1, 2 and 4 GiB"""
    lens = FC.ADDR_PITCH_PACKED
    TF._need(sum(lens) * 4 / 1024 + 4)
    g = torch.Generator(device="cuda").manual_seed(11)
    q, k, v, do = (_wide((sum(lens), 1, 64), "bf16", g) for _ in range(4))
    cu = TF.TV._cu(lens)
    off = cu.tolist()
    assert off[1] * FC.PITCH > GIB and off[2] * FC.PITCH > 2 * GIB and off[3] * FC.PITCH > 4 * GIB
    kw = dict(causal=True)
    far = TF._run_packed(q, k, v, do, cu, cu, None, window, kw)
    near = TF._run_packed(q.contiguous(), k.contiguous(), v.contiguous(), do.contiguous(), cu, cu, None, window, kw)
    _bits_equal(far, near, "packed")
    j = TF.Judge(f"pitch_packed_{window[0]}", "bf16")
    sl = slice(off[3], off[4])
    TF.compare_slice(j, "address/pitch-packed", "[seq 3]", "bf16", kw, window, (far[0][sl].permute(1, 0, 2), far[1][sl].permute(1, 0, 2), far[2][sl][:, 0], far[3][sl][:, 0]),
                     (q[sl].permute(1, 0, 2), k[sl][:, 0], v[sl][:, 0], do[sl].permute(1, 0, 2)))
    j.done()


@pytest.mark.parametrize("window", [(-1, -1), (300, 0)], ids=["plain", "w300"])
def test_decode_walks_a_cache_whose_positions_are_1_mib_apart(window):
    c = FC.ADDR_PITCH_DECODE
    cap, N, n_new, lens = c["cap"], c["N"], c["n_new"], c["lens"]
    TF._need(cap * 2 / 1024 + 4)
    g = torch.Generator(device="cuda").manual_seed(13)
    kc, vc = _wide((1, 1, cap, 128), "bf16", g), _wide((1, 1, cap, 128), "bf16", g)
    assert lens[0] * FC.PITCH > 4 * GIB
    q, kn, vn = _rand((1, 4, N, 128), "bf16", g), _rand((1, 1, n_new, 128), "bf16", g), _rand((1, 1, n_new, 128), "bf16", g)
    near_k, near_v = kc.contiguous(), vc.contiguous()
    kw = dict(causal=True)
    o_far = TF._decode(q, kc, vc, kn, vn, lens, None, window, kw)
    o_near = TF._decode(q, near_k, near_v, kn, vn, lens, None, window, kw)
    assert torch.isfinite(o_far).all() and torch.equal(o_far, o_near)
    assert torch.equal(kc, near_k) and torch.equal(vc, near_v) and torch.equal(kc[0, :, lens[0]:lens[0] + n_new], kn[0])
    j = TF.Judge(f"pitch_decode_{window[0]}", "bf16")
    L = lens[0] + n_new
    TF.compare_slice(j, "address/pitch-decode", "", "bf16", kw, window, (o_far[0],), (q[0], kc[0, 0, :L], vc[0, 0, :L]))
    j.done()


def test_dense_d128_at_the_pitch_leaves_the_wide_forward():
    """the dense UN-windowed D = 128 call on a chip-filling grid (256 heads inside one row pitch) with rows 1 MiB apart: fwd3_kernel has no
    re-open of its 32-bit tile offset, so fwd3_applies must send it to the kernel that has one
    (test_fullsize_feature_launches_cpu.py::test_fwd3_kernel_is_left_at_its_32bit_offset_bound checks the launches).  Identical bits to
    contiguous copies run with the 64-rows-per-wave forward switched off -- the same launches, as that test shows."""
    from flash_cosine_sim_attention_amd import _lib
    H, rows = FC.ADDR_PITCH_FWD3
    D = 128
    TF._need(rows * 4 / 1024 + 8)
    g = torch.Generator(device="cuda").manual_seed(17)

    def wide():
        pad = FC.PITCH // 2
        backing = torch.empty((rows, pad), device="cuda", dtype=torch.bfloat16)
        view = backing[:, :H * D].view(rows, H, D).permute(1, 0, 2)[None]
        view.copy_(_rand((1, H, rows, D), "bf16", g))
        assert view.stride(2) * 2 == FC.PITCH
        return view

    q, k, v, do = wide(), wide(), wide(), wide()

    def run(q, k, v, do):
        q, k, v = (t.detach().requires_grad_() for t in (q, k, v))
        o = _F().flash_cosine_sim_attention(q, k, v, causal=True)
        o.backward(do)
        torch.cuda.synchronize()
        return o.detach(), q.grad, k.grad, v.grad

    far = run(q, k, v, do)
    prev = _lib.forward_form(0)
    try:
        near = run(q.contiguous(), k.contiguous(), v.contiguous(), do.contiguous())
    finally:
        _lib.forward_form(prev)
    _bits_equal(far, near, "dense D = 128 at the pitch")
    j = TF.Judge("pitch_dense_d128_unwindowed", "bf16")
    h = H - 1
    TF.compare_slice(j, "address/pitch-dense", f"[0,{h}]", "bf16", dict(causal=True), (-1, -1), (far[0][0, h][None], far[1][0, h][None], far[2][0, h], far[3][0, h]),
                     (q[0, h][None], k[0, h], v[0, h], do[0, h][None]))
    j.done()
