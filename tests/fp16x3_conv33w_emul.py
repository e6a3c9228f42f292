"""CPU emulation of the fp16x3 weight gradient of the (3, 3) fifth layer of an MRD band stack (include/flow2gan_hip.h:
f2g_conv33_wgrad_h3; csrc/conv33h3w.hip): tests/fp16x3_emul.py's arithmetic with ONE MONOTONE RUNNING SCALE per
operand and block, as tests/fp16x3_conv32w_emul.py, on the walk of conv33_wgrad6_kernel.

  tiles        R whole rows (fp16x3_conv33_emul.pick_rows), tiles_h = ceil(H / R) per sequence, numbered sequence-major
  blocks       grid = min(ntiles, 256); tile t belongs to block t % grid and is its step t // grid
  x patch      rows h0 - 1 .. h0 + R of the map, all W columns (fp16x3_conv33_emul.patches: the kernel's zero border
               columns and rows outside the map hold no float of the map and do not count)
  g tile       the R x W gradient rows, zeros below the map
  running max  m_run = 0 at a block's first step; before tile T is split m_run = max(m_run, m_T), where a tile whose
               maximum m_T is zero or not finite leaves it alone; scale s = 2^(14 - floor(log2 m_run)), exponent clamped
               to +-126, s = 1 for m_run = 0
  product      acc0 += hi_g hi_x, acc1 += hi_g lo_x + lo_g hi_x under the scales in force; the stored sums follow every
               change of scale by exact powers of two, so gw = sum_T (acc0_T + 2^-11 acc1_T) / s_x,T / s_g,T, a tile's
               sums being the weight gradient of its patch and gradient rows, valid over the rows and zero-padded over
               the columns
  bound        3 * 2^-22 sum |g||x| + 2^-28 sum_T (xrun_T sum_{px in T} |g_px,co| + grun_T sum_{px in T} |x_px+tap,ci|)
               per output, xrun_T / grun_T the running maxima in force at tile T; pixels whose tap lies outside the map
               do not count

Maps are (S, H, W, 32) channels-last; gradients of the weight come as (32, 9 * 32) = [co][tap][ci], the layout the
kernel accumulates into.  The sums are exact (float64) where the kernel accumulates in fp32.
"""
import torch
import torch.nn.functional as F

import fp16x3_emul as emul
from fp16x3_conv32w_emul import _split
from fp16x3_conv33_emul import patches, pick_rows
from fp16x3_emul import BOUND, FLOOR, scale_exponents

BLOCKS = 256


def grad_tiles(g, R):
    """(S, tiles_h, R, W, C) tiles of the gradient map g (S, H, W, C), zeros below the map"""
    S, H, W, Cc = g.shape
    nh = -(-H // R)
    big = torch.zeros(S, nh * R, W, Cc, dtype=g.dtype)
    big[:, :H] = g
    return big.view(S, nh, R, W, Cc)


def partition(ntiles):
    """(grid, steps) of the launch rule: grid blocks, the longest walk has `steps` tiles"""
    grid = max(1, min(ntiles, BLOCKS))
    return grid, -(-ntiles // grid)


def block_tiles(ntiles, b):
    """the tiles block b walks, in its order"""
    return list(range(b, ntiles, partition(ntiles)[0]))


def running_max(m):
    """the running maximum in force at every tile: m (ntiles,) float32 tile maxima in tile order -> (ntiles,) float32;
    block t % grid meets tile t at its step t // grid; a zero, inf or NaN tile maximum leaves the running maximum alone;
    every block starts at 0"""
    n = m.numel()
    grid, steps = partition(n)
    padded = torch.zeros(steps * grid, dtype=m.dtype)
    padded[:n] = m
    # (block, step) is the walk order: every block one segment
    return emul.running_max(padded.view(steps, grid).t(), [0, steps]).t().reshape(-1)[:n]


def walk(x, g):
    """The blocks' walk over the tiles of x and g (S, H, W, 32): a dict of R, nh, grid, steps, the patches xp (ntiles,
    R + 2, W, 32) and gradient tiles gt (ntiles, R, W, 32) in tile order, the running maxima xrun, grun (ntiles,) and the
    scale exponents sx, sg (ntiles,) in force at each tile"""
    S, H, W, Cc = x.shape
    R, xp = patches(x.float())
    gt = grad_tiles(g.float(), R)
    nh = xp.shape[1]
    nt = S * nh
    xp, gt = xp.reshape(nt, R + 2, W, Cc), gt.reshape(nt, R, W, Cc)
    xrun = running_max(xp.abs().amax((1, 2, 3)))
    grun = running_max(gt.abs().amax((1, 2, 3)))
    grid, steps = partition(nt)
    return dict(R=R, nh=nh, grid=grid, steps=steps, xp=xp, gt=gt, xrun=xrun, grun=grun, sx=scale_exponents(xrun),
                sg=scale_exponents(grun))


def _wg_tiles(xp, gt):
    """sum over the tiles of the weight gradient, valid over the rows and zero-padded over the columns: xp (n, R + 2, W,
    Ci), gt (n, R, W, Co) float64 -> (Co, 9 * Ci) [co][tap][ci]"""
    co, ci = gt.shape[-1], xp.shape[-1]
    gw = torch.nn.grad.conv2d_weight(xp.permute(0, 3, 1, 2), (co, ci, 3, 3), gt.permute(0, 3, 1, 2), padding=(0, 1))
    return gw.permute(0, 2, 3, 1).reshape(co, 9 * ci)


def wgrad(x, g, flush=False):
    """float64 weight gradient (32, 9 * 32) of x, g (S, H, W, 32) in the kernel's arithmetic"""
    w = walk(x, g)
    hx, lx = _split(w["xp"], w["sx"], flush)
    hg, lg = _split(w["gt"], w["sg"], flush)
    # the two reciprocal scales of tile T, folded into its gradient pieces (exact powers of two in float64)
    r = torch.ldexp(torch.ones(hg.shape[0], dtype=torch.float64), -(w["sx"] + w["sg"])).view(-1, 1, 1, 1)
    acc0 = _wg_tiles(hx, hg * r)
    acc1 = _wg_tiles(lx, hg * r) + _wg_tiles(hx, lg * r)
    return acc0 + acc1 * 2.0 ** -11


def exact_wgrad(x, g):
    """float64 autograd: the gradient of the conv's weight as (Co, 9 * Ci) [co][tap][ci]; x (S, H, W, Ci), g (S, H,
    W, Co)"""
    co, ci = g.shape[-1], x.shape[-1]
    w = torch.zeros(co, ci, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().permute(0, 3, 1, 2), w, padding=(1, 1)).backward(g.double().permute(0, 3, 1, 2))
    return w.grad.permute(0, 2, 3, 1).reshape(co, 9 * ci)


def running_maps(x, g):
    """(xrun, grun) as (S, H, 1, 1) float64 maps: the running maxima in force at the tile that owns each row"""
    S, H = x.shape[:2]
    w = walk(x, g)
    return [run.double().view(S, w["nh"], 1).expand(S, w["nh"], w["R"]).reshape(S, -1)[:, :H, None, None]
            for run in (w["xrun"], w["grun"])]


def bound_wgrad(x, g, rel=BOUND):
    """(bound, sum |g||x|) per output (32, 9 * 32).  sum_{px in T} |g_px,co| over the pixels whose tap lies inside the
    map is the weight gradient against an all-ones input channel, sum_{px in T} |x_px+tap,ci| the one of an all-ones
    gradient channel; the running maxima weigh the rows of their tiles"""
    mag = exact_wgrad(x.abs(), g.abs())
    xrun, grun = running_maps(x, g)
    sum_g = exact_wgrad(torch.ones_like(x[..., :1]), g.abs().double() * xrun)       # (32, 9): [co][tap]
    sum_x = exact_wgrad(x.abs(), grun.expand(*x.shape[:3], 1))                      # (1, 9 * 32): [tap][ci]
    floor = sum_g.view(32, 9, 1) + sum_x.view(1, 9, 32)
    return rel * mag + FLOOR * floor.reshape(32, 9 * 32), mag
