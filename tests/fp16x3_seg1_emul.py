"""CPU emulation of the fp16x3 tap-walking GEMM over STRIDE-1 windows that scales its map INSIDE the kernel
(csrc/gemm_f16pn.hip, f2g_operand.split 8): windows of `taps` (2 or 1) positions over a halo map, step by step as the
kernel does it.  tests/fp16x3_seg_emul.py is the same for the stride-3 kernel.

  row group  `group` consecutive output rows (the kernel's tile: 128)
  segment    the positions the rows of ONE sequence inside one row group read: rows p_a .. p_b of sequence s read
             positions first + p_a .. first + p_b + taps - 1, every one of them by some window: n + taps - 1
             positions for n rows
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
             amax_segment <= amax_sequence: the per-sequence floor of tests/fp16x3_seq_emul.py is an upper bound.

tile_geometry() and entry_place() restate the kernel's index arithmetic -- the entries of a tile and the multiply-shift
that stands for the division by a segment's length -- so that the host test can walk every case the host rule admits.
"""
import torch

import fp16x3_emul as emul
from fp16x3_emul import BOUND, FLOOR

NSEG, TILE = 17, 128        # the kernel's table of segments per tile and its tile


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


def segment_windows(seg, n, taps):
    """(n, taps * C): row i = positions i ... i + taps - 1 of the segment seg (n + taps - 1, C)"""
    return torch.stack([seg[t:t + n] for t in range(taps)], 1).reshape(n, -1)


def gemm(x, w, P0, taps, group, first=0):
    """(float64 windows(x) w^T in the kernel's arithmetic, the fp32 accumulation replaced by exact sums;
    amax_segment of every output row).  x (S, Hp, C) the map, w (N, taps C) the weights"""
    S, Hp, Cc = x.shape
    hb, lb, rb = emul.split(w)
    hb, lb, rb = hb.double(), lb.double(), rb.double()
    out = torch.empty(S * P0, w.shape[0], dtype=torch.float64)
    amax = torch.empty(S * P0, dtype=torch.float64)
    for r, s, pa, pb in segments(S, P0, group):
        n = pb - pa + 1
        seg = x[s, first + pa:first + pb + taps].float()
        hi, lo, rs = emul.split(seg.reshape(1, -1))           # ONE scale for the segment
        ha = segment_windows(hi.view(-1, Cc).double(), n, taps)
        la = segment_windows(lo.view(-1, Cc).double(), n, taps)
        acc0 = ha @ hb.t()
        acc1 = ha @ lb.t() + la @ hb.t()
        out[r:r + n] = (acc0 + acc1 * 2.0 ** -11) * rs.double() * rb[None, :]
        amax[r:r + n] = seg.double().abs().max()
    return out, amax


def windows(x, P0, taps, first=0):
    """(S * P0, taps C): row (s, p) = positions first + p ... + taps - 1 of sequence s of the map x (S, Hp, C)"""
    return torch.stack([x[:, first + t:first + t + P0] for t in range(taps)], 2).reshape(x.shape[0] * P0, -1)


def bound(x, w, P0, taps, amax_segment, first=0):
    """per output: 3 * 2^-22 sum |a| |w| + 2^-28 (amax_segment(row) sum_k |w[n,k]| + wmax_n sum |a(row)|)"""
    a, wd = windows(x.double().abs(), P0, taps, first), w.double().abs()
    mag = a @ wd.t()
    floor = amax_segment[:, None] * wd.sum(1)[None, :] + a.sum(1)[:, None] * wd.amax(1)[None, :]
    return BOUND * mag + FLOOR * floor, mag


# ---- the kernel's index arithmetic
def tile_geometry(M, P0, taps, m0):
    """(sq0, rl0, E0, EP, L) of the tile whose first row is m0, as gemm_h3pn_kernel computes them: its first sequence
    and window, the entries of its first segment, of a whole sequence's segment, and of all its segments"""
    sq0, rl0 = divmod(m0, P0)
    nval = min(M - m0, TILE)
    n0 = min(P0 - rl0, nval)
    nfull, part = divmod(nval - n0, P0)
    EP, E0 = P0 + taps - 1, n0 + taps - 1
    return sq0, rl0, E0, EP, E0 + nfull * EP + (part + taps - 1 if part else 0)


def entry_place(e, rl0, E0, EP):
    """(segment, position behind its sequence's first window start) of staged entry e -- the quotient by EP as the
    kernel takes it: a multiplication by ceil(2^16 / EP) and a shift"""
    if e < E0:
        return 0, e + rl0
    e2 = e - E0
    k = 1 + ((e2 * ((65536 + EP - 1) // EP)) >> 16)
    return k, e2 - (k - 1) * EP


def row_entry(r, P0, sq0, rl0, E0, EP):
    """the first staged entry of output row r's window"""
    sq, rl = divmod(r, P0)
    return rl - rl0 if sq == sq0 else E0 + (sq - sq0 - 1) * EP + rl
