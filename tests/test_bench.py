"""bench.py's own contract: a plain run prints only the headline (the extra measurements wait for --full),
and --dump-outputs writes what the last timed step computed, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_sample_is_fixed_and_bounded(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(3)
    ts = [torch.randn(10, generator=g), None, torch.randn(300, 200, generator=g), torch.randn(7, generator=g)]
    s = bench.sample_of(ts)
    n = bench.SAMPLE_PER_TENSOR
    assert s.shape == (10 + n + 7,)
    assert torch.equal(s, bench.sample_of(ts))                       # fixed positions
    assert torch.equal(s[:10], ts[0]) and torch.equal(s[-7:], ts[3])  # small tensors whole
    big = ts[2].reshape(-1)
    pos = bench._seeded_positions(big.numel(), n, 2)
    assert torch.equal(s[10:10 + n], big[pos])
    huge = torch.arange(bench.SAMPLE_PER_ARRAY + 5, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path), {"s": s, "huge": huge, "loss": torch.tensor([1.5, 2.5])})
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["huge", "loss", "s"]
    assert got["s"].dtype == np.float32 and np.array_equal(got["s"], s.numpy())
    assert got["loss"].tolist() == [1.5, 2.5]
    assert got["huge"].dtype == np.float64 and got["huge"].shape == (bench.SAMPLE_PER_ARRAY,)


def _bench(outdir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--batch", "2", "--dump-outputs", str(outdir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(outdir / f) for f in sorted(os.listdir(outdir))}


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    d, outs = _bench(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert abs(d["value"] - 2 * 2 * 1.0 / (d["ms_per_step"] * 1e-3)) < 1e-2 * d["value"]
    # a plain run times the headline only
    assert all(d[k] is None for k in ("roofline", "exact_fp32", "frozen_weights", "fast_mode", "cpu_baseline"))
    assert sorted(outs) == ["d_grad_sample", "d_losses", "g_grad_sample", "g_losses"]
    assert outs["d_losses"].shape == (2,) and outs["g_losses"].shape == (5,)
    for k, a in outs.items():
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), k
    assert sum(a.nbytes for a in outs.values()) <= 64 << 20
    # same arguments, same inputs: a second run computes the same step up to the summation order of the
    # atomics (measured at B = 2 and 64: losses to 3e-7, gradient samples to 3e-4 of their largest entry)
    _, again = _bench(tmp_path / "b")
    for k, a in outs.items():
        b = again[k]
        tol = 5e-3 if k.endswith("_sample") else 1e-4
        assert a.shape == b.shape, k
        assert np.abs(a - b).max() <= tol * np.abs(a).max(), (k, float(np.abs(a - b).max()))
