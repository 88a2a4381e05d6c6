"""bench.py --dump-outputs: the sample of the headline step's outputs is the same (batch, head) slices on every call, float32, exact
copies of those slices, and within the 64 MB limit at the headline shape; --steps below 1 is refused before anything runs."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_sample_is_fixed_exact_and_bounded(tmp_path):
    w = bench.WORKLOAD
    shp = (w["B"], w["H"], w["N"], w["D"])
    g = torch.Generator().manual_seed(0)
    outs = {n: torch.randn(shp, generator=g).to(torch.bfloat16) for n in ("o", "dq", "dk", "dv")}
    arrays, picked = bench.dump_sample(outs)
    again, picked2 = bench.dump_sample(outs)
    assert picked == picked2 and len(set(picked)) == bench.DUMP_SLICES and picked == sorted(picked)
    assert all(0 <= i < w["B"] * w["H"] for i in picked)
    assert sum(a.nbytes for a in arrays.values()) <= bench.DUMP_LIMIT_BYTES
    for n, a in arrays.items():
        assert a.dtype == np.float32 and a.shape == (bench.DUMP_SLICES, w["N"], w["D"])
        assert np.array_equal(a, again[n])
        for j, i in enumerate(picked):
            assert np.array_equal(a[j], outs[n][i // w["H"], i % w["H"]].float().numpy())
    bench.write_dump(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == ["dk.npy", "dq.npy", "dv.npy", "o.npy"]
    for n, a in arrays.items():
        assert np.array_equal(np.load(tmp_path / "d" / (n + ".npy")), a)


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr, r.stderr[-2000:]
