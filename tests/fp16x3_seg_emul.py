"""CPU emulation of the fp16x3 tap-walking GEMM that scales its map INSIDE the kernel (csrc/gemm_f16p3n.hip,
f2g_operand.split 8): stride-3 windows of five positions over a halo map, step by step as the kernel does it.

  row group  `group` consecutive output rows (the kernel's tile: 128)
  segment    the positions the rows of ONE sequence inside one row group read: rows p_a .. p_b of sequence s read
             positions first + 3 p_a .. first + 3 p_b + 4, every one of them by some window
  scale      s = 2^(14 - floor(log2 max|x|)) over the segment, exponent clamp / all-zero / non-finite rules of
             fp16x3_emul.split (a segment is a "row" there)
  pieces     y = x s, hi = fp16(y), lo = fp16(2^11 (y - hi)); the weights: one scale per weight row, as
             f2g_split_f16x2_seq makes them
  products   acc0 += hi_a hi_b, acc1 += hi_a lo_b + lo_a hi_b       (three MFMAs; lo lo dropped)
  rescale    v = (acc0 + 2^-11 acc1) / s_segment[row] / s_b[col]

A scale never spans two sequences and a window never leaves its sequence, so every output row has exactly one scale.

  bound      per output: 3 * 2^-22 sum |a| |w|                             (residual of either piece, the dropped lo lo)
                         + 2^-28 (amax_segment sum_k |w[n,k]|              (map elements subnormal in hi)
                                  + wmax_n sum |a|)                         (weight elements subnormal in hi)
             amax_segment <= amax_sequence: the per-sequence floor of tests/fp16x3_seq3_emul.py is an upper bound.
"""
import torch

import fp16x3_emul as emul
from fp16x3_emul import BOUND, FLOOR

TAPS, STEP = 5, 3


def segments(S, P0, group):
    """[(first output row, sequence, p_a, p_b)]: the segments of every row group of the S * P0 output rows, in order"""
    out = []
    for m0 in range(0, S * P0, group):
        r, end = m0, min(m0 + group, S * P0)
        while r < end:
            s, p = divmod(r, P0)
            n = min(P0 - p, end - r)
            out.append((r, s, p, p + n - 1))
            r += n
    return out


def segment_windows(seg, n):
    """(n, TAPS * C): row i = positions 3 i ... 3 i + 4 of the segment seg (3 n + 2, C)"""
    return torch.stack([seg[t:t + STEP * (n - 1) + 1:STEP] for t in range(TAPS)], 1).reshape(n, -1)


def gemm(x, w, P0, group, first=0):
    """(float64 windows(x) w^T in the kernel's arithmetic, the fp32 accumulation replaced by exact sums;
    amax_segment of every output row).  x (S, Hp, C) the map, w (N, 5 C) the weights"""
    S, Hp, Cc = x.shape
    hb, lb, rb = emul.split(w)
    hb, lb, rb = hb.double(), lb.double(), rb.double()
    out = torch.empty(S * P0, w.shape[0], dtype=torch.float64)
    amax = torch.empty(S * P0, dtype=torch.float64)
    for r, s, pa, pb in segments(S, P0, group):
        n = pb - pa + 1
        seg = x[s, first + STEP * pa:first + STEP * pb + TAPS].float()
        hi, lo, rs = emul.split(seg.reshape(1, -1))           # ONE scale for the segment
        ha = segment_windows(hi.view(-1, Cc).double(), n)
        la = segment_windows(lo.view(-1, Cc).double(), n)
        acc0 = ha @ hb.t()
        acc1 = ha @ lb.t() + la @ hb.t()
        out[r:r + n] = (acc0 + acc1 * 2.0 ** -11) * rs.double() * rb[None, :]
        amax[r:r + n] = seg.double().abs().max()
    return out, amax


def windows(x, P0, first=0):
    """(S * P0, 5 C): row (s, p) = positions first + 3 p ... + 5 of sequence s of the map x (S, Hp, C)"""
    last = first + STEP * (P0 - 1)
    return torch.stack([x[:, first + t:last + t + 1:STEP] for t in range(TAPS)], 2).reshape(x.shape[0] * P0, -1)


def bound(x, w, P0, amax_segment, first=0):
    """per output: 3 * 2^-22 sum |a| |w| + 2^-28 (amax_segment(row) sum_k |w[n,k]| + wmax_n sum |a(row)|)"""
    a, wd = windows(x.double().abs(), P0, first), w.double().abs()
    mag = a @ wd.t()
    floor = amax_segment[:, None] * wd.sum(1)[None, :] + a.sum(1)[:, None] * wd.amax(1)[None, :]
    return BOUND * mag + FLOOR * floor, mag
