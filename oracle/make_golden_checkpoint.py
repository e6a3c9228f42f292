"""Generate tests/golden/checkpoint_avg.npz by running the REAL reference checkpoint averaging
(flow2gan/checkpoint.py: average_checkpoints_with_averaged_model, average_checkpoints) in the build
container.

TEST INFRASTRUCTURE.  Builds the two checkpoint files of
tests/test_host_side.py::test_checkpoint_roundtrip_and_model_averaging (same seeds, same update
sequence, written by flow2gan_amd.checkpoint) and stores what the reference's functions return for
them: `range/<key>` (mean over (4, 8] from the two running averages) and `plain/<key>` (plain mean
of the "model" entries).
"""
from __future__ import annotations

import copy
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, ROOT]
import ref_shims  # noqa: E402

ref_shims.install()
from flow2gan import checkpoint as rck  # noqa: E402

from flow2gan_amd import checkpoint as ck  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "checkpoint_avg.npz")


def _small_net(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 2))


def write_files(d):
    """The test's two checkpoints (batches 4 and 8 of 8, averaged every 2)."""
    cur = _small_net(1)
    avg = copy.deepcopy(cur).to(torch.float64)
    files = []
    period = 2
    for b in range(1, 9):
        with torch.no_grad():
            for p in cur.parameters():
                p.add_(0.1 * torch.randn_like(p))
        if b % period == 0:
            ck.update_averaged_model({"average_period": period, "batch_idx_train": b}, cur, avg)
        if b in (4, 8):
            f = os.path.join(d, f"checkpoint-{b}.pt")
            ck.save_checkpoint(f, cur, model_avg=avg, params={"batch_idx_train": b, "epoch": 1})
            files.append(f)
    return files


def main():
    with tempfile.TemporaryDirectory() as d:
        files = write_files(d)
        rng = rck.average_checkpoints_with_averaged_model(files[0], files[1])
        plain = rck.average_checkpoints(files)
    out = {f"range/{k}": v.numpy() for k, v in rng.items()}
    out.update({f"plain/{k}": v.numpy() for k, v in plain.items()})
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, sorted(out))


if __name__ == "__main__":
    main()
