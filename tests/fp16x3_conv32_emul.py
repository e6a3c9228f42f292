"""CPU emulation of the fp16x3 MRD band convolutions (include/flow2gan_hip.h: f2g_conv32_desc.precision 4;
csrc/conv32h3.hip): tests/fp16x3_emul.py's arithmetic with the "row" of split() read as ONE TILE'S STAGED PATCH
(every float of it, halo pixels included, zeros where the patch leaves the map) for the activations and as the WHOLE
weight matrix for the weights.

  tile pick    8 x 16 or 16 x 8 output pixels, whichever wastes fewer pixels of the map (c32_pick_tiles): over
               (H, Wout) in the forward, over (H, (Win + 1) / 2) positions m in the data gradient, where a tile is
               its positions x both column parities x = 2 m + E of the input
  patch        forward: rows h0 - 1 .. h0 + TH, input columns 2 w0 - 4 .. 2 w0 + 2 TW + 2  ((TH + 2) x (2 TW + 7))
               data gradient: rows h0 - 1 .. h0 + TH, gradient columns m0 - 2 .. m0 + TW + 1  ((TH + 2) x (TW + 4))
  product      acc0 += hi_a hi_w, acc1 += hi_a lo_w + lo_a hi_w, v = (acc0 + 2^-11 acc1) / s_patch / s_w
  bound        3 * 2^-22 sum |a||w| + 2^-28 (amax_patch sum_k |w_k| + wmax sum_k |a_k|) per output, k over the
               output's own reduction (taps and positions outside the map do not count)

Maps are (S, H, W, 32) channels-last, weights (32 co, 32 ci, 3, 9) as torch.nn.Conv2d holds them.  The sums are exact
(float64) where the kernels accumulate in fp32.
"""
import torch
import torch.nn.functional as F

import fp16x3_emul as emul
from fp16x3_emul import BOUND, FLOOR

KH, KW = 3, 9


def wout_of(Win):
    return (Win - 1) // 2 + 1


def pick_tiles(H, W):
    """(TH, TW, tiles_h, tiles_w) as c32_pick_tiles: 16 x 8 only where it wastes strictly less"""
    def waste(th, tw):
        return -(-H // th) * th * (-(-W // tw) * tw)
    th, tw = (16, 8) if waste(16, 8) < waste(8, 16) else (8, 16)
    return th, tw, -(-H // th), -(-W // tw)


def _patches(x, th, tw, tiles_h, tiles_w, col0, step, width):
    """(S, tiles_h, tiles_w, th + 2, width, C) patches of the map x (S, H, W, C): rows h0 - 1 .. h0 + th of tile row
    h0 = th * i, columns step * tw * j + col0 ... + width, zeros outside the map"""
    S, H, W, Cc = x.shape
    top, left = 1, -col0
    Hp, Wp = tiles_h * th + 2, step * tw * (tiles_w - 1) + width
    big = torch.zeros(S, Hp, max(Wp, W + left), Cc, dtype=x.dtype)
    big[:, top:top + H, left:left + W] = x
    rows = [big[:, th * i:th * i + th + 2] for i in range(tiles_h)]
    return torch.stack([torch.stack([r[:, :, step * tw * j:step * tw * j + width] for j in range(tiles_w)], 1)
                        for r in rows], 1)


def fwd_patches(x):
    """the forward tiles of x (S, H, Win, 32): (TH, TW, patches (S, tiles_h, tiles_w, TH + 2, 2 TW + 7, 32))"""
    S, H, Win, Cc = x.shape
    th, tw, nh, nw = pick_tiles(H, wout_of(Win))
    return th, tw, _patches(x, th, tw, nh, nw, -(KW - 1) // 2, 2, 2 * tw + 7)


def dgrad_patches(g, Win):
    """the data-gradient tiles of g (S, H, Wout, 32): (TH, TW, patches (S, tiles_h, tiles_w, TH + 2, TW + 4, 32))"""
    S, H, Wout, Cc = g.shape
    th, tw, nh, nw = pick_tiles(H, (Win + 1) // 2)
    return th, tw, _patches(g, th, tw, nh, nw, -2, 1, tw + 4)


def _untile(t, H, W):
    """(S, tiles_h, tiles_w, th, tw, C) -> (S, H, W, C)"""
    S, nh, nw, th, tw, Cc = t.shape
    return t.permute(0, 1, 3, 2, 4, 5).reshape(S, nh * th, nw * tw, Cc)[:, :H, :W]


def split_weight(w, flush=False):
    """(hi, lo) as float16 conv weights (co, ci, 3, 9) and the reciprocal scale of the WHOLE matrix"""
    hi, lo, rs = emul.split(w.reshape(1, -1), flush)
    return hi.view(w.shape), lo.view(w.shape), rs


def weight_image(w2d):
    """the image the kernels read of a contiguous weight matrix (27648 floats, either layout): int32 words of the
    one-run f2g_split_f16x2_seq image and the reciprocal scale"""
    from fp16x3_seq_emul import image
    img, rs = image(w2d.reshape(1, -1))
    return img.view(-1), rs


def _split_patches(p, flush):
    """pieces of every patch under its own scale: (hi, lo) float64 like p, rs (S, tiles_h, tiles_w) float64"""
    n = p.shape[:3]
    hi, lo, rs = emul.split(p.reshape(n[0] * n[1] * n[2], -1), flush)
    return hi.view(p.shape).double(), lo.view(p.shape).double(), rs.view(n).double()


def _conv_tiles(p, w, transposed):
    """float64 valid convolution of the patches p (S, nh, nw, rows, cols, C) with w: the tiles' outputs
    (S, nh, nw, TH, TW or 2 TW, C)"""
    S, nh, nw, r, c, Cc = p.shape
    q = p.reshape(S * nh * nw, r, c, Cc).permute(0, 3, 1, 2)
    if transposed:
        # out[r', c'] = sum g[r, c] w[r' - r, c' - 2 c]: tile row h - h0 = r' - 2, input column x - 2 m0 = c' - 8
        o = F.conv_transpose2d(q, w, stride=(1, 2))[:, :, 2:r, 8:8 + 2 * (c - 4)]
    else:
        o = F.conv2d(q, w, stride=(1, 2))
    return o.permute(0, 2, 3, 1).reshape(S, nh, nw, o.shape[2], o.shape[3], Cc)


def _run(patches, w, H, W, transposed, flush):
    hw, lw, rsw = split_weight(w, flush)
    hw, lw = hw.double(), lw.double()
    ha, la, rs = _split_patches(patches, flush)
    acc0 = _conv_tiles(ha, hw, transposed)
    acc1 = _conv_tiles(ha, lw, transposed) + _conv_tiles(la, hw, transposed)
    v = (acc0 + acc1 * 2.0 ** -11) * rs[..., None, None, None] * rsw.double()
    return _untile(v, H, W)


def fwd(x, w, flush=False):
    """float64 conv (no bias, no activation) of x (S, H, Win, 32) in the kernel's arithmetic -> (S, H, Wout, 32)"""
    _, _, p = fwd_patches(x)
    return _run(p, w, x.shape[1], wout_of(x.shape[2]), False, flush)


def dgrad(g, w, Win, flush=False):
    """float64 data gradient of g (S, H, Wout, 32) in the kernel's arithmetic -> (S, H, Win, 32)"""
    _, _, p = dgrad_patches(g, Win)
    return _run(p, w, g.shape[1], Win, True, flush)


def patch_amax_fwd(x):
    """(S, H, Wout, 1): the largest magnitude of the patch of the tile that owns each output pixel"""
    th, tw, p = fwd_patches(x)
    a = p.abs().amax((3, 4, 5))[..., None, None, None].expand(*p.shape[:3], th, tw, 1)
    return _untile(a, x.shape[1], wout_of(x.shape[2])).double()


def patch_amax_dgrad(g, Win):
    """(S, H, Win, 1): the same for the data gradient (both column parities of a tile share its patch)"""
    th, tw, p = dgrad_patches(g, Win)
    a = p.abs().amax((3, 4, 5))[..., None, None, None].expand(*p.shape[:3], th, 2 * tw, 1)
    return _untile(a, g.shape[1], Win).double()


def exact_fwd(x, w):
    """float64 conv of x (S, H, Win, C) with w (co, ci, 3, 9), stride (1, 2), padding (1, 4), channels-last"""
    return F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), stride=(1, 2), padding=(1, 4)).permute(0, 2, 3, 1)


def exact_dgrad(g, w, Win):
    """float64 data gradient of that conv: g (S, H, Wout, C) -> (S, H, Win, C)"""
    opad = Win - 1 - 2 * (g.shape[2] - 1)
    return F.conv_transpose2d(g.double().permute(0, 3, 1, 2), w.double(), stride=(1, 2), padding=(1, 4),
                              output_padding=(0, opad)).permute(0, 2, 3, 1)


def bound_fwd(x, w, rel=BOUND):
    """(bound, sum |a||w|) per output of the forward.  sum_k |w_k| over an output's own reduction is the conv of an
    all-ones map (the same for every sequence), sum_k |a_k| the conv with an all-ones kernel (one output channel)"""
    mag = exact_fwd(x.abs(), w.abs())
    sum_w = exact_fwd(torch.ones_like(x[:1]), w.abs())
    sum_a = exact_fwd(x.abs(), torch.ones_like(w[:1]))
    return rel * mag + FLOOR * (patch_amax_fwd(x) * sum_w + float(w.abs().max()) * sum_a), mag


def bound_dgrad(g, w, Win, rel=BOUND):
    """(bound, sum |g||w|) per output of the data gradient"""
    mag = exact_dgrad(g.abs(), w.abs(), Win)
    sum_w = exact_dgrad(torch.ones_like(g[:1]), w.abs(), Win)
    sum_g = exact_dgrad(g.abs(), torch.ones_like(w[:, :1]), Win)
    return rel * mag + FLOOR * (patch_amax_dgrad(g, Win) * sum_w + float(w.abs().max()) * sum_g), mag
