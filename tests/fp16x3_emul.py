"""CPU emulation of the fp16x3 GEMM arithmetic (include/flow2gan_hip.h: f2g_split_f16x2, f2g_gemm_desc.precision 4),
step by step as the kernels do it: the oracle of the split kernel (bit for bit) and of the error bound, and the
arithmetic core of every other tests/fp16x3_*_emul.py -- the scale rule, the two pieces, the subnormal flush and the
running maximum are defined here once; what belongs to one kernel's walk stays in that kernel's emulator.

  row scale  s = 2^(14 - floor(log2 max|x|)), exponent clamped to +-126; s = 1 for an all-zero or non-finite row
  pieces     y = x s, hi = fp16(y), lo = fp16(2^11 (y - hi))        (round to nearest even)
  product    acc0 += hi_a hi_b, acc1 += hi_a lo_b + lo_a hi_b, v = (acc0 + 2^-11 acc1) / s_a[row] / s_b[col]
"""
import torch

BOUND = 3 * 2.0 ** -22      # per product, of |a| |b|: one 2^-22 per operand's residual, one for the dropped lo lo
FLOOR = 2.0 ** -28          # of the largest magnitude under a shared scale: an element that far below it is subnormal
                            # (or zero) in hi, whether or not the matrix pipe flushes subnormals


def flush_subnormals(h):
    """an fp16 tensor with its subnormal values replaced by zero (a matrix pipe that flushes its inputs)"""
    return torch.where(h.float().abs() < 2.0 ** -14, torch.zeros_like(h), h)


def scale_exponents(amax):
    """sexp of f2g_f16_scales for the maxima `amax` (float32): s = 2^sexp with sexp = 14 - floor(log2 amax) clamped to
    +-126, 0 for a zero or non-finite maximum (a NaN in the data makes its maximum NaN)"""
    live = torch.isfinite(amax) & (amax > 0)
    _, ex = torch.frexp(torch.where(live, amax, torch.ones_like(amax)))       # amax = m 2^ex, m in [0.5, 1)
    sexp = (14 - (ex - 1)).clamp(-126, 126)
    return torch.where(live, sexp, torch.zeros_like(sexp))


def pieces(y, flush=False):
    """(hi, lo) float16 of the already-scaled fp32 tensor y; flush: subnormal pieces read as zero"""
    hi = y.to(torch.float16)
    lo = ((y - hi.float()) * 2048.0).to(torch.float16)
    if flush:
        hi, lo = flush_subnormals(hi), flush_subnormals(lo)
    return hi, lo


def running_max(m, bounds):
    """the running maximum in force at every step of a walk: m (..., n) float32 maxima in walk order along the last
    dimension, bounds = the first step of every segment and, last, n -> the same shape; every segment starts at 0 and a
    zero, inf or NaN maximum leaves the running maximum alone"""
    counted = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    out = torch.empty_like(counted)
    for a, b in zip(bounds[:-1], bounds[1:]):
        out[..., a:b] = counted[..., a:b].cummax(dim=-1).values
    return out


def split(x, flush=False):
    """(hi, lo, rscale) of the rows of the fp32 matrix x: two float16 matrices and 1 / s per row (float32)"""
    x = x.float()
    amax = x.abs().amax(dim=1)
    sexp, one = scale_exponents(amax), torch.ones_like(amax)
    hi, lo = pieces(x * torch.ldexp(one, sexp)[:, None], flush)
    return hi, lo, torch.ldexp(one, -sexp)


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
