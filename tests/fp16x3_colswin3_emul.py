"""CPU emulation of the fp16x3 tap-walking weight gradient of a STRIDED layer (include/flow2gan_hip.h:
f2g_gemm_desc.precision 4 with form 2 and a stride-3 window operand B; csrc/gemm_f16ws.hip), step by step as the route
does it:

  images     f2g_split_f16x2_cols of the gradient g (nseq * hp, Cout) and of the WHOLE halo map x (nseq * hp_in, Cin),
             halo rows included (tests/fp16x3_colswin_emul.py: pieces -- one power-of-two scale per column)
  windows    tap t of reduction row (s, p) reads map row s * hp_in + step * p + t - pad -- tap and stride only select
             ROWS, zeros before and behind the map: the column scales are the same for every tap, position, sequence
  sums       acc0[co, t, ci] = sum_(s, p) hi_g hi_x, acc1 = sum_(s, p) (hi_g lo_x + lo_g hi_x)
  rescale    gw[co, t * Cin + ci] = (acc0 + 2^-11 acc1) / s_g[co] / s_x[ci]
"""
import torch

import fp16x3_colswin_emul as win


def rows_of(nseq, hp_in, hp, pad, step, t):
    """flat map row of every reduction row (s, p) under tap t, and whether it lies inside the map"""
    s = torch.arange(nseq).repeat_interleave(hp)
    p = torch.arange(hp).repeat(nseq)
    r = s * hp_in + step * p + t - pad
    return r, (r >= 0) & (r < nseq * hp_in)


def gathered(m, r, ok):
    out = torch.zeros(r.numel(), m.shape[1], dtype=m.dtype)
    out[ok] = m[r[ok]]
    return out


def windows3(x, nseq, hp_in, hp, pad, step=3, taps=5):
    """(nseq * hp, taps * Cin): what the window operand addresses, x_win[(s, p), t * Cin + ci] = x[s * hp_in + step * p
    + t - pad, ci], zero outside [0, nseq * hp_in)"""
    assert x.shape[0] == nseq * hp_in
    return torch.cat([gathered(x, *rows_of(nseq, hp_in, hp, pad, step, t)) for t in range(taps)], dim=1)


def tap3_wgrad(g, x, nseq, hp_in, hp, pad, step=3, taps=5):
    """float64 gw (Cout, taps * Cin) in the route's arithmetic, the fp32 accumulation replaced by exact sums"""
    assert g.shape[0] == nseq * hp
    hg, lg, rg = win.pieces(g)
    hx, lx, rx = win.pieces(x)
    out = []
    for t in range(taps):
        r, ok = rows_of(nseq, hp_in, hp, pad, step, t)
        hxt, lxt = gathered(hx, r, ok), gathered(lx, r, ok)
        acc0 = hg.t() @ hxt
        acc1 = hg.t() @ lxt + lg.t() @ hxt
        out.append((acc0 + acc1 * 2.0 ** -11) * rg.double()[:, None] * rx.double()[None, :])
    return torch.cat(out, dim=1)
