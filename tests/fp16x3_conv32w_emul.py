"""CPU emulation of the fp16x3 weight gradient of the MRD band convolutions (include/flow2gan_hip.h:
f2g_conv32_s2_wgrad_h3; csrc/conv32h3w.hip): tests/fp16x3_emul.py's arithmetic with ONE MONOTONE RUNNING SCALE per
operand and block in place of a row's scale.

  tiles        8 x 16 or 16 x 8 output pixels over (H, Wout) (fp16x3_conv32_emul.pick_tiles), numbered sequence-major,
               then tile row, then tile column
  blocks       per = ceil(ntiles / 256) consecutive tiles each, ceil(ntiles / per) blocks
  x patch      the forward kernel's: rows h0 - 1 .. h0 + TH, input columns 2 w0 - 4 .. 2 w0 + 2 TW + 2, zeros outside
  g tile       the TH x TW gradient tile, zeros outside the map
  running max  m_run = 0 at a block's first tile; before tile T is split m_run = max(m_run, m_T), where a tile whose
               maximum m_T is zero or not finite leaves it alone; scale s = 2^(14 - floor(log2 m_run)), exponent clamped
               to +-126, s = 1 for m_run = 0
  product      acc0 += hi_g hi_x, acc1 += hi_g lo_x + lo_g hi_x under the scales in force; the stored sums follow every
               change of scale by exact powers of two, so gw = sum_T (acc0_T + 2^-11 acc1_T) / s_x,T / s_g,T
  bound        3 * 2^-22 sum |g||x| + 2^-28 sum_T (xrun_T sum_{px in T} |g_px,co| + grun_T sum_{px in T} |x_px->tap,ci|)
               per output, xrun_T / grun_T the running maxima in force at tile T; pixels and taps outside the map do
               not count

Maps are (S, H, W, 32) channels-last; gradients of the weight come as (32, 27 * 32) = [co][tap][ci], the layout the
kernel accumulates into.  The sums are exact (float64) where the kernel accumulates in fp32.
"""
import torch
import torch.nn.functional as F

import fp16x3_emul as emul
from fp16x3_conv32_emul import fwd_patches, pick_tiles, wout_of
from fp16x3_emul import BOUND, FLOOR, scale_exponents

BLOCKS = 256


def grad_tiles(g, th, tw, nh, nw):
    """(S, nh, nw, th, tw, C) tiles of the gradient map g (S, H, Wout, C), zeros outside the map"""
    S, H, W, Cc = g.shape
    big = torch.zeros(S, nh * th, nw * tw, Cc, dtype=g.dtype)
    big[:, :H, :W] = g
    return big.view(S, nh, th, nw, tw, Cc).permute(0, 1, 3, 2, 4, 5)


def _untile(t, H, W):
    S, nh, nw, th, tw, Cc = t.shape
    return t.permute(0, 1, 3, 2, 4, 5).reshape(S, nh * th, nw * tw, Cc)[:, :H, :W]


def partition(ntiles):
    """(per, blocks) of the launch rule"""
    per = max(1, -(-ntiles // BLOCKS))
    return per, -(-ntiles // per)


def running_max(m):
    """the running maximum in force at every tile of the walk: m (ntiles,) float32 tile maxima in walk order ->
    (ntiles,) float32; a zero, inf or NaN tile maximum leaves it alone; every block starts at 0"""
    n = m.numel()
    per, blocks = partition(n)
    return emul.running_max(m, [min(b * per, n) for b in range(blocks + 1)])


def walk(x, g):
    """The block's walk over the tiles of x (S, H, Win, 32) and g (S, H, Wout, 32): a dict of th, tw, nh, nw, per,
    blocks, the patches xp (ntiles, TH + 2, 2 TW + 7, 32) and gradient tiles gt (ntiles, TH, TW, 32) in walk order, the
    running maxima xrun, grun (ntiles,) and the scale exponents sx, sg (ntiles,) in force at each tile"""
    S, H, Win, Cc = x.shape
    th, tw, xp = fwd_patches(x.float())
    _, _, nh, nw = pick_tiles(H, wout_of(Win))
    gt = grad_tiles(g.float(), th, tw, nh, nw)
    nt = S * nh * nw
    xp, gt = xp.reshape(nt, *xp.shape[3:]), gt.reshape(nt, th, tw, Cc)
    xrun = running_max(xp.abs().amax((1, 2, 3)))
    grun = running_max(gt.abs().amax((1, 2, 3)))
    per, blocks = partition(nt)
    return dict(th=th, tw=tw, nh=nh, nw=nw, per=per, blocks=blocks, xp=xp, gt=gt, xrun=xrun, grun=grun,
                sx=scale_exponents(xrun), sg=scale_exponents(grun))


def _split(t, sexp, flush):
    """(hi, lo) float64 of the tiles t (ntiles, ...) under the scales 2^sexp (ntiles,); flush: subnormal pieces read
    as zero (a matrix pipe that flushes its inputs)"""
    s = torch.ldexp(torch.ones(t.shape[0]), sexp).view(-1, *([1] * (t.dim() - 1)))
    hi, lo = emul.pieces(t * s, flush)
    return hi.double(), lo.double()


def _wg_tiles(xp, gt):
    """sum over the tiles of the valid-convolution weight gradient: xp (n, TH + 2, 2 TW + 7, Ci), gt (n, TH, TW, Co)
    float64 -> (Co, 27 * Ci) [co][tap][ci]"""
    co, ci = gt.shape[-1], xp.shape[-1]
    gw = torch.nn.grad.conv2d_weight(xp.permute(0, 3, 1, 2), (co, ci, 3, 9), gt.permute(0, 3, 1, 2), stride=(1, 2))
    return gw.permute(0, 2, 3, 1).reshape(co, 27 * ci)


def wgrad(x, g, flush=False):
    """float64 weight gradient (32, 27 * 32) of x (S, H, Win, 32), g (S, H, Wout, 32) in the kernel's arithmetic"""
    w = walk(x, g)
    hx, lx = _split(w["xp"], w["sx"], flush)
    hg, lg = _split(w["gt"], w["sg"], flush)
    # the two reciprocal scales of tile T, folded into its gradient pieces (exact powers of two in float64)
    r = torch.ldexp(torch.ones(hg.shape[0], dtype=torch.float64), -(w["sx"] + w["sg"])).view(-1, 1, 1, 1)
    acc0 = _wg_tiles(hx, hg * r)
    acc1 = _wg_tiles(lx, hg * r) + _wg_tiles(hx, lg * r)
    return acc0 + acc1 * 2.0 ** -11


def exact_wgrad(x, g):
    """float64 autograd: the gradient of the conv's weight as (Co, 27 * Ci) [co][tap][ci]; x (S, H, Win, Ci),
    g (S, H, Wout, Co)"""
    co, ci = g.shape[-1], x.shape[-1]
    w = torch.zeros(co, ci, 3, 9, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().permute(0, 3, 1, 2), w, stride=(1, 2), padding=(1, 4)).backward(g.double().permute(0, 3, 1, 2))
    return w.grad.permute(0, 2, 3, 1).reshape(co, 27 * ci)


def running_maps(x, g):
    """(xrun, grun) as (S, H, Wout, 1) float64 maps: the running maxima in force at the tile that owns each pixel"""
    S, H = x.shape[:2]
    Wout = wout_of(x.shape[2])
    w = walk(x, g)
    out = []
    for run in (w["xrun"], w["grun"]):
        t = run.double().view(S, w["nh"], w["nw"], 1, 1, 1).expand(S, w["nh"], w["nw"], w["th"], w["tw"], 1)
        out.append(_untile(t, H, Wout))
    return out


def bound_wgrad(x, g, rel=BOUND):
    """(bound, sum |g||x|) per output (32, 27 * 32).  sum_{px in T} |g_px,co| over the pixels whose tap lies inside the
    map is the weight gradient against an all-ones input channel, sum_{px in T} |x_px->tap,ci| the one of an all-ones
    gradient channel; the running maxima weigh the pixels of their tiles"""
    mag = exact_wgrad(x.abs(), g.abs())
    xrun, grun = running_maps(x, g)
    sum_g = exact_wgrad(torch.ones_like(x[..., :1]), g.abs().double() * xrun)       # (32, 27): [co][tap]
    sum_x = exact_wgrad(x.abs(), grun)                                              # (1, 27 * 32): [tap][ci]
    floor = sum_g.view(32, 27, 1) + sum_x.view(1, 27, 32)
    return rel * mag + FLOOR * floor.reshape(32, 27 * 32), mag
