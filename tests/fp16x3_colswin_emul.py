"""CPU emulation of the fp16x3 tap-walking weight gradient (include/flow2gan_hip.h: f2g_gemm_desc.precision 4 with
form 2 and a window operand B; csrc/gemm_f16wt.hip), step by step as the route does it:

  images     f2g_split_f16x2_cols of the gradient g (R, Cout) and of the WHOLE halo map x (R, Cin), halo rows included
             (tests/fp16x3_cols_emul.py: one power-of-two scale per column)
  windows    tap t of reduction row r reads map row r + t - pad -- a shift of ROWS, zeros before and behind the map:
             the column scales are the same for every tap
  sums       acc0[co, t, ci] = sum_r hi_g hi_x, acc1 = sum_r (hi_g lo_x + lo_g hi_x)
  rescale    gw[co, t * Cin + ci] = (acc0 + 2^-11 acc1) / s_g[co] / s_x[ci]
"""
import torch

import fp16x3_cols_emul as cols


def pieces(x):
    """(hi, lo, rscale) read back out of the column image's words: float64 (rows, cols) each, float32 (cols,)"""
    img, rs = cols.image(x)
    rows, n = x.shape
    halves = img.contiguous().view(torch.int16).view(rows, n // 4, 8)
    hi = halves[:, :, :4].reshape(rows, n).contiguous().view(torch.float16)
    lo = halves[:, :, 4:].reshape(rows, n).contiguous().view(torch.float16)
    return hi.double(), lo.double(), rs


def shifted(m, by):
    """rows r -> m[r + by], zeros where r + by leaves the matrix"""
    out = torch.zeros_like(m)
    R = m.shape[0]
    lo, hi = max(0, -by), min(R, R - by)
    if hi > lo:
        out[lo:hi] = m[lo + by:hi + by]
    return out


def windows(x, pad, taps=5):
    """(R, taps * Cin): what the window operand addresses, x_win[r, t * Cin + ci] = x[r + t - pad, ci]"""
    return torch.cat([shifted(x, t - pad) for t in range(taps)], dim=1)


def tap_wgrad(g, x, pad, taps=5):
    """float64 gw (Cout, taps * Cin) in the route's arithmetic, the fp32 accumulation replaced by exact sums"""
    hg, lg, rg = pieces(g)
    hx, lx, rx = pieces(x)
    out = []
    for t in range(taps):
        hxt, lxt = shifted(hx, t - pad), shifted(lx, t - pad)
        acc0 = hg.t() @ hxt
        acc1 = hg.t() @ lxt + lg.t() @ hxt
        out.append((acc0 + acc1 * 2.0 ** -11) * rg.double()[:, None] * rx.double()[None, :])
    return torch.cat(out, dim=1)
