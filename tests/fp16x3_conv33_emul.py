"""CPU emulation of the fp16x3 (3, 3) fifth layer of an MRD band stack (include/flow2gan_hip.h: f2g_conv33_fwd at
f2g_conv32_desc.precision 4; csrc/conv33h3.hip): tests/fp16x3_emul.py's arithmetic with the "row" of split() read as
ONE TILE'S STAGED PATCH (every float of it, the halo rows included, zeros where the patch leaves the map) for the
activations and as the WHOLE weight matrix for the weights.

  row pick     a tile is R whole rows: R = min(256 // W, H), shrunk while (R + 2) * (W + 2) > 352 (c33_pick_rows)
  patch        rows h0 - 1 .. h0 + R of the map, all W columns ((R + 2) x W; the kernel's zero border columns hold
               no float of the map and do not count)
  product      acc0 += hi_a hi_w, acc1 += hi_a lo_w + lo_a hi_w, v = (acc0 + 2^-11 acc1) / s_patch / s_w
  data grad.   the same kernel over the gradient map with the weights [ci][8 - tap][co]: one scale for the whole
               matrix, so the pieces of the re-laid matrix are the re-laid pieces
  bound        3 * 2^-22 sum |a||w| + 2^-28 (amax_patch sum_k |w_k| + wmax sum_k |a_k|) per output, k over the
               output's own reduction (taps outside the map do not count)

Maps are (S, H, W, 32) channels-last, weights (32 co, 32 ci, 3, 3) as torch.nn.Conv2d holds them.  The sums are exact
(float64) where the kernel accumulates in fp32.
"""
import torch
import torch.nn.functional as F

import fp16x3_emul as emul
from fp16x3_emul import BOUND, FLOOR

P33 = 352


def pick_rows(H, W):
    """rows per tile as c33_pick_rows (W <= 112)"""
    R = min(256 // W, H)
    while R > 1 and (R + 2) * (W + 2) > P33:
        R -= 1
    assert R >= 1 and (R + 2) * (W + 2) <= P33, (H, W)
    return R


def patches(x):
    """(R, patches (S, tiles_h, R + 2, W, C)) of the map x (S, H, W, C): rows h0 - 1 .. h0 + R of tile h0 = R * i,
    zeros outside the map"""
    S, H, W, Cc = x.shape
    R = pick_rows(H, W)
    nh = -(-H // R)
    big = torch.zeros(S, nh * R + 2, W, Cc, dtype=x.dtype)
    big[:, 1:1 + H] = x
    return R, torch.stack([big[:, R * i:R * i + R + 2] for i in range(nh)], 1)


def flipped(w):
    """the data gradient's weights as a forward conv's: [ci][co][2 - dh][2 - dw]"""
    return w.permute(1, 0, 2, 3).flip(2, 3).contiguous()


def split_weight(w, flush=False):
    """(hi, lo) as conv weights like w and the reciprocal scale of the WHOLE matrix"""
    hi, lo, rs = emul.split(w.reshape(1, -1), flush)
    return hi.view(w.shape), lo.view(w.shape), rs


def weight_image(w2d):
    """the image the kernel reads of a contiguous weight matrix (9216 floats, either layout): int32 words of the
    one-run f2g_split_f16x2_seq image and the reciprocal scale"""
    from fp16x3_seq_emul import image
    img, rs = image(w2d.reshape(1, -1))
    return img.view(-1), rs


def _split_patches(p, flush):
    """pieces of every patch under its own scale: (hi, lo) float64 like p, rs (S, tiles_h) float64"""
    n = p.shape[:2]
    hi, lo, rs = emul.split(p.reshape(n[0] * n[1], -1), flush)
    return hi.view(p.shape).double(), lo.view(p.shape).double(), rs.view(n).double()


def _conv_tiles(p, w):
    """float64 convolution of the patches p (S, nh, R + 2, W, C) with w, valid over the rows and zero-padded over the
    columns: the tiles' outputs (S, nh, R, W, C)"""
    S, nh, r, c, Cc = p.shape
    o = F.conv2d(p.reshape(S * nh, r, c, Cc).permute(0, 3, 1, 2), w, padding=(0, 1))
    return o.permute(0, 2, 3, 1).reshape(S, nh, r - 2, c, Cc)


def fwd(x, w, flush=False):
    """float64 conv (no bias, no activation) of x (S, H, W, 32) in the kernel's arithmetic -> (S, H, W, 32)"""
    S, H, W, Cc = x.shape
    hw, lw, rsw = split_weight(w, flush)
    hw, lw = hw.double(), lw.double()
    _, p = patches(x)
    ha, la, rs = _split_patches(p, flush)
    acc0 = _conv_tiles(ha, hw)
    acc1 = _conv_tiles(ha, lw) + _conv_tiles(la, hw)
    v = (acc0 + acc1 * 2.0 ** -11) * rs[..., None, None, None] * rsw.double()
    return v.reshape(S, -1, W, Cc)[:, :H]


def dgrad(g, w, flush=False):
    """float64 data gradient of g (S, H, W, 32) in the kernel's arithmetic -> (S, H, W, 32)"""
    return fwd(g, flipped(w), flush)


def patch_amax(x):
    """(S, H, 1, 1): the largest magnitude of the patch of the tile that owns each output row"""
    S, H = x.shape[:2]
    R, p = patches(x)
    a = p.abs().amax((2, 3, 4))[..., None].expand(S, p.shape[1], R)
    return a.reshape(S, -1)[:, :H, None, None].double()


def exact_fwd(x, w):
    """float64 conv of x (S, H, W, C) with w (co, ci, 3, 3), padding (1, 1), channels-last"""
    return F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=(1, 1)).permute(0, 2, 3, 1)


def exact_dgrad(g, w):
    """float64 data gradient of that conv: g (S, H, W, C) -> (S, H, W, C)"""
    return F.conv_transpose2d(g.double().permute(0, 3, 1, 2), w.double(), padding=(1, 1)).permute(0, 2, 3, 1)


def bound_fwd(x, w, rel=BOUND):
    """(bound, sum |a||w|) per output of the forward.  sum_k |w_k| over an output's own reduction is the conv of an
    all-ones map (the same for every sequence), sum_k |a_k| the conv with an all-ones kernel (one output channel)"""
    mag = exact_fwd(x.abs(), w.abs())
    sum_w = exact_fwd(torch.ones_like(x[:1]), w.abs())
    sum_a = exact_fwd(x.abs(), torch.ones_like(w[:1]))
    return rel * mag + FLOOR * (patch_amax(x) * sum_w + float(w.abs().max()) * sum_a), mag


def bound_dgrad(g, w, rel=BOUND):
    """(bound, sum |g||w|) per output of the data gradient"""
    return bound_fwd(g, flipped(w), rel)
