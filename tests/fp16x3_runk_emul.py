"""CPU emulation of the fp16x3 weight gradient over two plain fp32 K-major matrices, both scaled inside the kernel
(include/flow2gan_hip.h: f2g_gemm_desc.precision 4 with form 2 and both operands marked split = 10;
csrc/gemm_f16wn.hip): tests/fp16x3_conv32w_emul.py's running-scale arithmetic on gemm_h3w_kernel's walk.

  tiles        128 x 128 outputs: column tile tm of A (R, M), column tile tn of B (R, N); the last tile of either may
               be partial
  K chunks     f2g_launch_h3w's rule: kchunk = ceil(ceil(R / split_k) / 32) * 32 reduction rows per block, ceil(R /
               kchunk) blocks per tile; a block walks its chunk in slabs of 32 rows (the last slab of the last chunk may
               be ragged)
  slab max     per operand, over the slab's floats of the tile's columns that lie inside the matrix
  running max  m_run = 0 at a block's first slab; before slab T is split m_run = max(m_run, m_T), where a slab whose
               maximum m_T is zero or not finite leaves it alone; scale s = 2^(14 - floor(log2 m_run)), exponent clamped
               to +-126, s = 1 for m_run = 0
  product      acc0 += hi_a hi_b, acc1 += hi_a lo_b + lo_a hi_b under the scales in force; the stored sums follow every
               change of scale by exact powers of two, so c = sum_T (acc0_T + 2^-11 acc1_T) / s_a,T / s_b,T
  bound        3 * 2^-22 sum |a||b| + 2^-28 sum_T (brun_T sum_{r in T} |a| + arun_T sum_{r in T} |b|) per output, arun_T /
               brun_T the running maxima in force at slab T of the output's tiles

The sums are exact (float64) where the kernel accumulates in fp32.  A's scales depend on (tm, chunk) alone and B's on
(tn, chunk): every block that shares a column tile and a chunk walks the same maxima.
"""
import torch

import fp16x3_emul as emul
from fp16x3_emul import BOUND, FLOOR, scale_exponents

TILE = 128              # output rows / columns of a block
SLAB = 32               # reduction rows of a slab


def kchunk_of(R, split_k=1):
    """reduction rows per block (a multiple of SLAB) and the number of blocks along K"""
    per_block = -(-R // max(1, split_k))
    kchunk = -(-per_block // SLAB) * SLAB
    return kchunk, -(-R // kchunk)


def slab_of_rows(R):
    """the slab (counted over the whole reduction: chunks are whole slabs) of every reduction row"""
    return torch.arange(R) // SLAB


def slab_maxima(x):
    """(tiles, slabs) float32: the largest magnitude of every slab of every 128-column tile of x (R, cols) -- NaN
    where a float of it is NaN, inf where one is inf"""
    R, cols = x.shape
    nslab, ntile = -(-R // SLAB), -(-cols // TILE)
    rowmax = torch.stack([x[:, t * TILE:(t + 1) * TILE].float().abs().amax(1) for t in range(ntile)])     # (tiles, R)
    padded = torch.zeros(ntile, nslab * SLAB)
    padded[:, :R] = rowmax
    m = padded.view(ntile, nslab, SLAB)
    # (amax propagates NaN; an inf beside a NaN: NaN -- either way the slab is not counted)
    return m.amax(2)


def running_max(m, R, split_k=1):
    """the running maximum in force at every slab: m (tiles, slabs) float32 -> the same shape; a zero, inf or NaN slab
    maximum leaves it alone; every K chunk starts at 0"""
    kchunk, chunks = kchunk_of(R, split_k)
    per = kchunk // SLAB
    return emul.running_max(m, [min(z * per, m.shape[1]) for z in range(chunks + 1)])


def walk(a, b, split_k=1):
    """slab maxima ma / mb (tiles, slabs), the running maxima arun / brun in force at each slab and the scale exponents
    sa / sb, of a (R, M) and b (R, N)"""
    R = a.shape[0]
    assert b.shape[0] == R
    ma, mb = slab_maxima(a), slab_maxima(b)
    arun, brun = running_max(ma, R, split_k), running_max(mb, R, split_k)
    return dict(ma=ma, mb=mb, arun=arun, brun=brun, sa=scale_exponents(arun), sb=scale_exponents(brun),
                kchunk=kchunk_of(R, split_k)[0])


def _rows_of(per_slab, x):
    """per_slab (tiles, slabs) -> (R, cols): the value of every element's column tile and row's slab"""
    R, cols = x.shape
    return per_slab[:, slab_of_rows(R)].t()[:, torch.arange(cols) // TILE]


def _pieces(x, sexp, flush):
    """(hi, lo) float64 of x (R, cols) under the scales 2^sexp (R, cols: constant over a tile's slab)"""
    hi, lo = emul.pieces(x.float() * torch.ldexp(torch.ones(x.shape), sexp), flush)
    return hi.double(), lo.double()


def wgrad(a, b, split_k=1, flush=False):
    """float64 c (M, N) = a^T b in the kernel's arithmetic: every element is split at the scale of its tile's slab, the
    two reciprocal scales are folded into the pieces (exact powers of two in float64)"""
    w = walk(a, b, split_k)
    sa, sb = _rows_of(w["sa"], a), _rows_of(w["sb"], b)
    ha, la = _pieces(a, sa, flush)
    hb, lb = _pieces(b, sb, flush)
    ra, rb = torch.ldexp(torch.ones(a.shape, dtype=torch.float64), -sa), torch.ldexp(
        torch.ones(b.shape, dtype=torch.float64), -sb)
    ha, la, hb, lb = ha * ra, la * ra, hb * rb, lb * rb
    return ha.t() @ hb + (ha.t() @ lb + la.t() @ hb) * 2.0 ** -11


def exact_wgrad(a, b):
    return a.double().t() @ b.double()


def bound(a, b, split_k=1, rel=BOUND):
    """(bound, sum |a||b|) per output (M, N); the running maxima weigh the rows of their slabs"""
    w = walk(a, b, split_k)
    R, M = a.shape
    N = b.shape[1]
    slab = slab_of_rows(R)
    aa, ba = a.double().abs(), b.double().abs()
    mag = aa.t() @ ba
    # sum_r brun[tn(n), T(r)] |a[r, m]| -> (M, tiles of N) -> the column's tile; likewise for b
    fa = (aa.t() @ w["brun"].double()[:, slab].t())[:, torch.arange(N) // TILE]
    fb = (ba.t() @ w["arun"].double()[:, slab].t())[:, torch.arange(M) // TILE].t()
    return rel * mag + FLOOR * (fa + fb), mag


PATTERNS = ("normal", "rising", "falling", "loud_column", "zero_first", "zero_a", "zero_b")


def inputs(pattern, R, M, N, seed=0):
    """fp32 operands a (R, M), b (R, N) on the CPU, the same for the host and the GPU tests:
    normal       N(0, 1), b scaled by R^-1/2
    rising       rows rising over six decades in both operands: the scales move in most slabs
    falling      rows falling over six decades: the later slabs run under their block's first maxima (the floor term)
    loud_column  one column of each operand 10^4 times its neighbours
    zero_first   the first two slabs zero in both operands: the walk starts at m_run = 0, scale 1
    zero_a / zero_b   that operand all zero"""
    assert pattern in PATTERNS
    g = torch.Generator().manual_seed(1000 * seed + 7 * R + 3 * M + N)
    a = torch.randn(R, M, generator=g)
    b = torch.randn(R, N, generator=g) * R ** -0.5
    if pattern in ("rising", "falling"):
        f = torch.logspace(-3, 3, R)
        if pattern == "falling":
            f = f.flip(0)
        a, b = a * f[:, None], b * f[:, None]
    elif pattern == "loud_column":
        a[:, min(5, M - 1)] *= 1e4
        b[:, N // 2] *= 1e4
    elif pattern == "zero_first":
        a[:2 * SLAB] = 0.0
        b[:2 * SLAB] = 0.0
    elif pattern == "zero_a":
        a.zero_()
    elif pattern == "zero_b":
        b.zero_()
    return a, b


# ---- the cases of tests/test_hip_gemm_f16_wgradn.py (tests/test_fp16x3_wgradn_host.py holds the emulation to `bound`
# and `bound` to the GPU tolerance on every one of them) ---------------------------------------------------------------
# (R, M, N): a partial slab, exactly one, an odd and an even slab count, a ragged last slab; partial tiles in both
# directions; (97, 260, 132): six tiles, partial in both directions
SHAPES = [(R, M, N) for R in (1, 31, 32, 33, 64, 777) for M in (4, 96, 128, 132) for N in (32, 128, 160)] + \
    [(97, 260, 132)]
MAGNITUDE_SHAPES = [(160, 128, 128), (777, 132, 160)]
SPLIT_K = 3             # at R = 777: chunks of 288 / 288 / 201 rows, the last slab ragged


def gpu_cases():
    """every (pattern, (R, M, N), split_k) the GPU file launches"""
    out = [("normal", s, 1) for s in SHAPES]
    out += [(p, s, 1) for s in MAGNITUDE_SHAPES for p in PATTERNS]
    out += [("normal", MAGNITUDE_SHAPES[1], SPLIT_K), ("rising", MAGNITUDE_SHAPES[1], SPLIT_K)]
    return out


def refusals(spare):
    """name -> [(object, field, value)] ("+": added to the field): every descriptor the kernel declines, one change of
    the base descriptor each (tests/test_hip_gemm_f16_wgradn.py launches the same list)"""
    big_rows = 0x7ff00000 // (4 * 136) - 32 + 1            # (rows + 32) * ld * 4 >= 0x7ff00000 at ld = 136
    return {
        "only_a": [("B", "split", 0)], "only_b": [("A", "split", 0)],
        "rscale_a": [("A", "rscale", spare)], "rscale_b": [("B", "rscale", spare)],
        "cols_mod_4": [("A", "cols", 130)], "ld_mod_4": [("B", "seq_stride+", 2)], "ld_lt_cols": [("A", "seq_stride", 128)],
        "base_plus_4": [("A", "base+", 4)], "rows_differ": [("B", "rows+", -1)],
        "b_window": [("B", "P0", 8), ("B", "step0", 1)],
        "alpha": [("A", "alpha", spare)], "lrelu_src": [("A", "lrelu_src", spare)],
        "c_bf16": [("E", "c_bf16", 1)], "x3_out": [("E", "x3_out", spare)], "colsum_part_ld": [("E", "colsum_part_ld", 4)],
        "prelu_slope": [("E", "prelu_slope", spare)], "mask_src": [("E", "mask_src", spare)],
        "aux_without_alpha_n": [("E", "aux", spare), ("E", "ldaux", 256)],
        "split_k_without_atomic": [("d", "split_k", 2), ("E", "atomic", 0)],
        "extent": [("A", "rows", big_rows), ("B", "rows", big_rows)],
    }


def apply(d, sets):
    for o, field, v in sets:
        obj = {"A": d.A, "B": d.B, "E": d.E, "d": d}[o]
        if field.endswith("+"):
            field = field[:-1]
            v = getattr(obj, field) + v
        setattr(obj, field, v)
    return d
