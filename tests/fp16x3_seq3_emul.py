"""CPU emulation of the fp16x3 tap-walking GEMM over STRIDED windows of a halo map (csrc/gemm_f16p3.hip): the
arithmetic, images, scales and bound of tests/fp16x3_seq_emul.py -- a window never leaves its sequence whatever its
stride, so one power-of-two scale per sequence leaves every output row's sum exactly -- with the window stride added.

  window     row (s, p) = positions first + step * p ... + taps of sequence s
  bound      3 * 2^-22 |a| |b| per product + 2^-28 amax_seq sum_k |w[n,k]| per output (fp16x3_emul.BOUND, FLOOR)
"""
import torch

import fp16x3_seq_emul as seq
from fp16x3_emul import BOUND, FLOOR

split = seq.split
image = seq.image


def windows(x, P0, taps, step, first=0):
    """(S * P0, taps * C): row (s, p) = positions first + step * p ... + taps of sequence s of the map x (S, Hp, C)"""
    S, Hp, Cc = x.shape
    last = first + step * (P0 - 1)
    return torch.stack([x[:, first + t:last + t + 1:step] for t in range(taps)], 2).reshape(S * P0, taps * Cc)


def gemm(x, w, P0, taps, step, first=0, flush=False):
    """float64 windows(x) w^T in the kernel's arithmetic (the fp32 accumulation replaced by exact sums); x (S, Hp, C)
    the map, w (N, taps * C) the weights"""
    S, Hp, Cc = x.shape
    ha, la, ra = split(x.reshape(S, Hp * Cc), flush)
    hb, lb, rb = split(w, flush)
    ha, la = (windows(t.view(S, Hp, Cc).double(), P0, taps, step, first) for t in (ha, la))
    hb, lb = hb.double(), lb.double()
    acc0 = ha @ hb.t()
    acc1 = ha @ lb.t() + la @ hb.t()
    return (acc0 + acc1 * 2.0 ** -11) * ra.double().repeat_interleave(P0)[:, None] * rb.double()[None, :]


def bound(x, w, P0, taps, step, first=0, rel=BOUND):
    """per output: rel * (|A| |B|^T) + 2^-28 * amax_seq(row) * sum_k |w[n,k]|"""
    S = x.shape[0]
    mag = windows(x.double().abs(), P0, taps, step, first) @ w.double().abs().t()
    amax = x.double().abs().reshape(S, -1).amax(1).repeat_interleave(P0)
    return rel * mag + FLOOR * amax[:, None] * w.double().abs().sum(1)[None, :], mag
