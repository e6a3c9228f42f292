"""CPU emulation of the fp16x3 weight gradient of the MPD's 32 -> 128 layer, scaled inside the kernel
(include/flow2gan_hip.h: f2g_gemm_desc.precision 4 with form 2 and both operands marked split = 8;
csrc/gemm_f16wsn.hip): tests/fp16x3_conv32w_emul.py's running-scale arithmetic on the walk of
tests/fp16x3_colswin3_emul.py's windows.

  slabs        R = 16 gradient rows of one sequence and the 3 * 15 + 5 = 50 map rows they touch (map row of staged row
               q: s * hp_in + 3 * p0 - pad + q); units are numbered sequence-major, nseq * ceil(hp / 16) in all
  blocks       partition(units): min(512, max(1, units // 16)) blocks, block b the units [b * units // blocks, (b + 1) *
               units // blocks) -- at most two blocks per CU, at least 16 slabs = 256 reduction rows each unless the grid
               is one block
  slab max     over every staged float that lies inside the buffer: the gradient rows p0 .. min(p0 + 16, hp) - 1, the
               map rows of the 50 that lie in [0, nseq * hp_in) -- halo rows and rows of the neighbouring sequences
               included; the zeros substituted outside do not count
  running max  m_run = 0 at a block's first slab; before slab T is split m_run = max(m_run, m_T), where a slab whose
               maximum m_T is zero or not finite leaves it alone; scale s = 2^(14 - floor(log2 m_run)), exponent clamped
               to +-126, s = 1 for m_run = 0
  product      acc0 += hi_g hi_x, acc1 += hi_g lo_x + lo_g hi_x under the scales in force; the stored sums follow every
               change of scale by exact powers of two, so gw = sum_T (acc0_T + 2^-11 acc1_T) / s_x,T / s_g,T
  bound        3 * 2^-22 sum |g||x| + 2^-28 sum_T (xrun_T sum_{rows in T} |g| + grun_T sum_{rows in T} |x_win|) per
               output, xrun_T / grun_T the running maxima in force at slab T; window rows outside the buffer do not
               count

g is (nseq * hp, Cout), x the whole halo map (nseq * hp_in, Cin); the result is (Cout, 5 * Cin) = [co][tap][ci].  The
sums are exact (float64) where the kernel accumulates in fp32.
"""
import torch

import fp16x3_emul as emul
from fp16x3_colswin3_emul import gathered, rows_of, windows3
from fp16x3_emul import BOUND, FLOOR, running_max, scale_exponents      # running_max(m, bounds = partition(units))

R = 16                  # gradient rows of a slab
STEP, TAPS = 3, 5
XR = (R - 1) * STEP + TAPS
MAX_BLOCKS = 2 * 256    # two per CU
MIN_UNITS = 256 // R    # 256 reduction rows


def partition(units):
    """the launch rule: the first unit of every block and, last, `units` -- blocks + 1 numbers"""
    blocks = min(MAX_BLOCKS, max(1, units // MIN_UNITS))
    return [b * units // blocks for b in range(blocks + 1)]


def nslab_of(hp):
    return -(-hp // R)


def unit_of_rows(nseq, hp):
    """the unit (slab number in walk order) of every reduction row (s, p)"""
    s = torch.arange(nseq).repeat_interleave(hp)
    p = torch.arange(hp).repeat(nseq)
    return s * nslab_of(hp) + p // R


def slab_maxima(g, x, nseq, hp_in, hp, pad):
    """(mx, mg) float32 (units,): the largest magnitude among the staged floats of every slab that lie inside the
    buffers (NaN where a staged float is NaN, inf where one is inf)"""
    ns = nslab_of(hp)
    xrows = nseq * hp_in
    ga = g.float().abs().amax(1).view(nseq, hp)
    xa = x.float().abs().amax(1)
    mx, mg = torch.zeros(nseq * ns), torch.zeros(nseq * ns)
    for s in range(nseq):
        for k in range(ns):
            p0 = k * R
            mg[s * ns + k] = ga[s, p0:min(p0 + R, hp)].max()
            lo = s * hp_in + STEP * p0 - pad
            a, b = max(lo, 0), min(lo + XR, xrows)
            mx[s * ns + k] = xa[a:b].max() if b > a else 0.0
    return mx, mg


def walk(g, x, nseq, hp_in, hp, pad):
    """the running maxima xrun, grun (units,) and the scale exponents sx, sg (units,) in force at each slab, and the
    partition `bounds`"""
    mx, mg = slab_maxima(g, x, nseq, hp_in, hp, pad)
    bounds = partition(mx.numel())
    xrun, grun = running_max(mx, bounds), running_max(mg, bounds)
    return dict(bounds=bounds, mx=mx, mg=mg, xrun=xrun, grun=grun, sx=scale_exponents(xrun), sg=scale_exponents(grun))


def _pieces(t, sexp, flush):
    """(hi, lo) float64 of the rows t (rows, C) under the scales 2^sexp (rows,); flush: subnormal pieces read as zero"""
    hi, lo = emul.pieces(t.float() * torch.ldexp(torch.ones(t.shape[0]), sexp)[:, None], flush)
    return hi.double(), lo.double()


def wgrad(g, x, nseq, hp_in, hp, pad, flush=False):
    """float64 gw (Cout, 5 * Cin) in the kernel's arithmetic.  A reduction row is split at the scales of its slab -- a map
    row that two slabs stage is split twice, once at each slab's scale"""
    assert g.shape[0] == nseq * hp and x.shape[0] == nseq * hp_in
    w = walk(g, x, nseq, hp_in, hp, pad)
    unit = unit_of_rows(nseq, hp)
    sx, sg = w["sx"][unit], w["sg"][unit]
    hg, lg = _pieces(g, sg, flush)
    # the two reciprocal scales of the row's slab, folded into its gradient pieces (exact powers of two in float64)
    r = torch.ldexp(torch.ones(unit.numel(), dtype=torch.float64), -(sx + sg))[:, None]
    out = []
    for t in range(TAPS):
        rows, ok = rows_of(nseq, hp_in, hp, pad, STEP, t)
        hx, lx = _pieces(gathered(x.float(), rows, ok), sx, flush)
        acc0 = (hg * r).t() @ hx
        acc1 = (hg * r).t() @ lx + (lg * r).t() @ hx
        out.append(acc0 + acc1 * 2.0 ** -11)
    return torch.cat(out, dim=1)


def exact_wgrad(g, x, nseq, hp_in, hp, pad):
    return g.double().t() @ windows3(x.double(), nseq, hp_in, hp, pad)


def bound_wgrad(g, x, nseq, hp_in, hp, pad, rel=BOUND):
    """(bound, sum |g||x|) per output (Cout, 5 * Cin); the running maxima weigh the rows of their slabs"""
    w = walk(g, x, nseq, hp_in, hp, pad)
    unit = unit_of_rows(nseq, hp)
    xrun, grun = w["xrun"].double()[unit][:, None], w["grun"].double()[unit][:, None]
    ga = g.double().abs()
    mag, floor = [], []
    for t in range(TAPS):
        rows, ok = rows_of(nseq, hp_in, hp, pad, STEP, t)
        xt = gathered(x.double().abs(), rows, ok)
        mag.append(ga.t() @ xt)
        sum_g = (ga * xrun * ok[:, None]).sum(0)             # (Cout,): the rows whose tap lies inside the buffer
        sum_x = (xt * grun).sum(0)                           # (Cin,)
        floor.append(sum_g[:, None] + sum_x[None, :])
    mag = torch.cat(mag, dim=1)
    return rel * mag + FLOOR * torch.cat(floor, dim=1), mag
