"""What the rotary tests (test_gpu_kvcache_rotary.py, test_kvcache_rotary_cpu.py) share: the tables and the rotation, in numpy."""
import numpy as np
import torch


def tables(rows, rotary_dim, random=False):
    """float32 (cos, sin) [rows, rotary_dim / 2]: theta = 10000, or unrelated random angles, which no sin / cos swap or sign error survives"""
    half = rotary_dim // 2
    ang = (np.random.default_rng(7).uniform(-np.pi, np.pi, (rows, half)) if random
           else np.arange(rows)[:, None] * 10000.0 ** (-np.arange(half) / half)[None])
    return torch.tensor(np.cos(ang), dtype=torch.float32), torch.tensor(np.sin(ang), dtype=torch.float32)


def rotate(x, pos, cos, sin, interleaved, float32=False):
    """x [n, heads, D] (torch) -> (its rotation by table row clamp(pos[i]) as float64, |x| + |y| of every rotated element and 0 elsewhere).
    float32: evaluated as the kernels do -- t = fl(partner * sin), then ONE fused multiply-add fl(x * cos +- t) -- for the operand-faithful
    reference; otherwise exact float64 arithmetic on the same float32 tables."""
    out, half = x.detach().cpu().double().numpy(), cos.shape[1]
    rows = np.clip(np.asarray(pos), 0, cos.shape[0] - 1)
    c, s = cos.double().numpy()[rows][:, None], sin.double().numpy()[rows][:, None]
    ia, ib = (slice(0, 2 * half, 2), slice(1, 2 * half, 2)) if interleaved else (slice(0, half), slice(half, 2 * half))
    a, b, mag = out[..., ia].copy(), out[..., ib].copy(), np.zeros(out.shape)
    fl = (lambda v: v.astype(np.float32).astype(np.float64)) if float32 else (lambda v: v)      # (products of float32 values are exact in float64)
    out[..., ia], out[..., ib] = fl(a * c - fl(b * s)), fl(b * c + fl(a * s))
    mag[..., ia] = mag[..., ib] = np.abs(a) + np.abs(b)
    return out, mag
