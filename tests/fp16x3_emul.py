"""CPU emulation of the fp16x3 GEMM arithmetic (include/flow2gan_hip.h: f2g_split_f16x2, f2g_gemm_desc.precision 4),
step by step as the kernels do it: the oracle of the split kernel (bit for bit) and of the error bound.

  row scale  s = 2^(14 - floor(log2 max|x|)), exponent clamped to +-126; s = 1 for an all-zero or non-finite row
  pieces     y = x s, hi = fp16(y), lo = fp16(2^11 (y - hi))        (round to nearest even)
  product    acc0 += hi_a hi_b, acc1 += hi_a lo_b + lo_a hi_b, v = (acc0 + 2^-11 acc1) / s_a[row] / s_b[col]
"""
import torch

BOUND = 3 * 2.0 ** -22      # per product, of |a| |b|: one 2^-22 per operand's residual, one for the dropped lo lo


def split(x):
    """(hi, lo, rscale) of the rows of the fp32 matrix x: two float16 matrices and 1 / s per row (float32)"""
    x = x.float()
    amax = x.abs().amax(dim=1)                       # (a NaN in the row makes amax NaN)
    scaled = torch.isfinite(amax) & (amax > 0)
    _, ex = torch.frexp(torch.where(scaled, amax, torch.ones_like(amax)))     # amax = m 2^ex, m in [0.5, 1)
    sexp = (14 - (ex - 1)).clamp(-126, 126)
    sexp = torch.where(scaled, sexp, torch.zeros_like(sexp))
    one = torch.ones_like(amax)
    s, rs = torch.ldexp(one, sexp), torch.ldexp(one, -sexp)
    y = x * s[:, None]
    hi = y.to(torch.float16)
    lo = ((y - hi.float()) * 2048.0).to(torch.float16)
    return hi, lo, rs


def image(x):
    """the f2g_split_f16x2 image of x (rows, K) as int32 words, (rows, K): every aligned group of four floats =
    its four hi halves, then its four lo halves"""
    hi, lo, rs = split(x)
    rows, K = x.shape
    img = torch.cat([hi.view(torch.int16).view(rows, K // 4, 4), lo.view(torch.int16).view(rows, K // 4, 4)], dim=2)
    return img.contiguous().view(torch.int32).view(rows, K), rs


def gemm(A, B):
    """float64 A B^T in the kernel's arithmetic (the fp32 accumulation replaced by exact sums)"""
    ha, la, ra = split(A)
    hb, lb, rb = split(B)
    ha, la, hb, lb = ha.double(), la.double(), hb.double(), lb.double()
    acc0 = ha @ hb.t()
    acc1 = ha @ lb.t() + la @ hb.t()
    return (acc0 + acc1 * 2.0 ** -11) * ra.double()[:, None] * rb.double()[None, :]
