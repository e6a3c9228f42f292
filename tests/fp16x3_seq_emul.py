"""CPU emulation of the fp16x3 tap-walking GEMM (include/flow2gan_hip.h: f2g_split_f16x2_seq, f2g_operand.split 7):
tests/fp16x3_emul.py's arithmetic with the "row" of split() read as a whole RUN -- a sequence of a halo map (all its
positions x channels) or a row of the weight matrix -- and the GEMM over stride-1 windows of the map.

  run scale  s = 2^(14 - floor(log2 max|x|)) over the run, as fp16x3_emul.split
  image      every aligned slab of 32 floats = its 32 hi halves, then its 32 lo halves (128 bytes, the buffer's own
             addressing)
  product    acc0 += hi_a hi_b, acc1 += hi_a lo_b + lo_a hi_b, v = (acc0 + 2^-11 acc1) / s_a[row / P0] / s_b[col]
  bound      3 * 2^-22 |a| |b| per product + 2^-28 amax_seq sum_k |w[n,k]| per output: an element 2^-28 below its
             sequence's largest is subnormal (or zero) in hi, whether or not the matrix pipe flushes subnormals
"""
import torch

import fp16x3_emul as emul
from fp16x3_emul import BOUND, FLOOR


def split(x, flush=False):
    """(hi, lo, rscale) of the runs x (nruns, n): fp16x3_emul.split with one scale per run"""
    return emul.split(x.reshape(x.shape[0], -1), flush)


def image(x):
    """the f2g_split_f16x2_seq image of the runs x (nruns, n), n % 32 == 0, as int32 words (nruns, n), and the
    reciprocal scales"""
    hi, lo, rs = split(x)
    runs, n = hi.shape
    img = torch.cat([hi.view(torch.int16).view(runs, n // 32, 32), lo.view(torch.int16).view(runs, n // 32, 32)], dim=2)
    return img.contiguous().view(torch.int32).view(runs, n), rs


def windows(x, P0, taps, first=0):
    """(S * P0, taps * C): row (s, p) = positions first + p ... + taps of sequence s of the map x (S, Hp, C)"""
    S, Hp, Cc = x.shape
    return torch.stack([x[:, first + t:first + t + P0] for t in range(taps)], 2).reshape(S * P0, taps * Cc)


def gemm(x, w, P0, taps, first=0, flush=False):
    """float64 windows(x) w^T in the kernel's arithmetic (the fp32 accumulation replaced by exact sums); x (S, Hp, C)
    the map, w (N, taps * C) the weights"""
    S, Hp, Cc = x.shape
    ha, la, ra = split(x.reshape(S, Hp * Cc), flush)
    hb, lb, rb = split(w, flush)
    ha, la = (windows(t.view(S, Hp, Cc).double(), P0, taps, first) for t in (ha, la))
    hb, lb = hb.double(), lb.double()
    acc0 = ha @ hb.t()
    acc1 = ha @ lb.t() + la @ hb.t()
    return (acc0 + acc1 * 2.0 ** -11) * ra.double().repeat_interleave(P0)[:, None] * rb.double()[None, :]


def bound(x, w, P0, taps, first=0, rel=BOUND):
    """per output: rel * (|A| |B|^T) + 2^-28 * amax_seq(row) * sum_k |w[n,k]|"""
    S = x.shape[0]
    mag = windows(x.double().abs(), P0, taps, first) @ w.double().abs().t()
    amax = x.double().abs().reshape(S, -1).amax(1).repeat_interleave(P0)
    return rel * mag + FLOOR * amax[:, None] * w.double().abs().sum(1)[None, :], mag
