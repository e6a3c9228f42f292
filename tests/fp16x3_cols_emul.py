"""CPU emulation of the column image of the fp16x3 weight gradient (include/flow2gan_hip.h: f2g_split_f16x2_cols,
f2g_gemm_desc.precision 4 with form 2): tests/fp16x3_emul.py with "row" read as "column".

  column scale  s[c] = 2^(14 - floor(log2 max_r |x[r, c]|)), clamped as the row scale is
  pieces        y = x s, hi = fp16(y), lo = fp16(2^11 (y - hi))
  product       C[m, n] = (sum_r hi_a hi_b + 2^-11 sum_r (hi_a lo_b + lo_a hi_b)) / s_a[m] / s_b[n]
"""
import torch

import fp16x3_emul as emul


def image(x):
    """the f2g_split_f16x2_cols image of x (rows, cols) as int32 words, (rows, cols), and the reciprocal column
    scales: emul.split of the transpose, re-laid in chunks of four consecutive columns of a row -- four hi halves,
    then four lo halves"""
    hi, lo, rs = emul.split(x.t())
    rows, cols = x.shape
    hi, lo = hi.t().contiguous(), lo.t().contiguous()
    img = torch.cat([hi.view(torch.int16).view(rows, cols // 4, 4), lo.view(torch.int16).view(rows, cols // 4, 4)],
                    dim=2)
    return img.contiguous().view(torch.int32).view(rows, cols), rs


def wgrad(A, B):
    """float64 A^T B (A: (R, M), B: (R, N)) in the kernel's arithmetic, the fp32 accumulation replaced by exact sums"""
    return emul.gemm(A.t(), B.t())
