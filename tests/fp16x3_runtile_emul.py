"""CPU emulation of the fp16x3 pointwise GEMM over the fp32 activation matrix itself, scaled inside the kernel
(include/flow2gan_hip.h: f2g_gemm_desc.precision 4 with form 0 and operand A marked split = 9; csrc/gemm_f16n.hip):
tests/fp16x3_emul.py's arithmetic with the running scale of tests/fp16x3_conv32w_emul.py on the tile walk of the plain
GEMM.

  tiles        TILE = 128 output rows own one scale; the reduction walks slabs of SLAB = 32 columns
  slab max     m_T = the largest magnitude among the floats of rows [128 i, 128 i + 128) x columns [32 T, 32 T + 32)
               that lie inside the matrix (rows past M do not count)
  running max  m_run = 0 at slab 0; before slab T is split m_run = max(m_run, m_T), where a slab whose maximum is zero
               or not finite leaves it alone; scale s = 2^(14 - floor(log2 m_run)), exponent clamped to +-126, s = 1 for
               m_run = 0
  product      acc0 += hi_a hi_w, acc1 += hi_a lo_w + lo_a hi_w with A's pieces under the scale in force; when the
               scale moves both sums are multiplied by the exact power of two s_new / s_old first;
               v = (acc0 + 2^-11 acc1) / s_last / s_w[col], the weights under fp16x3_emul.split's scale per row
  bound        3 * 2^-22 sum_k |a||w| + 2^-28 sum_T arun_T sum_{k in T} |w_k| per output, arun_T the running maximum in
               force at slab T of the row's tile.  Rows share their tile's scale: a row quiet against its tile sees the
               second term

A is (M, K), W (N, K), the result (M, N).  The sums are exact (float64) where the kernel accumulates in fp32.  The input
builders at the end are shared by the CPU and the GPU tests, which therefore see the same tensors."""
import torch

import fp16x3_emul as emul
from fp16x3_emul import BOUND, FLOOR, scale_exponents

TILE, SLAB = 128, 32


def slab_maxima(A):
    """(tiles, slabs) float32: the largest magnitude of every (row tile, slab) of A (NaN where an element is NaN, inf
    where one is inf)"""
    M, K = A.shape
    nt, ns = -(-M // TILE), K // SLAB
    a = torch.zeros(nt * TILE, K)
    a[:M] = A.float().abs()
    return a.view(nt, TILE, ns, SLAB).amax(dim=(1, 3))


def running_max(m):
    """the running maximum in force at every slab: m (tiles, slabs) -> the same shape; a zero, inf or NaN slab maximum
    leaves it alone; every tile starts at 0"""
    return emul.running_max(m, [0, m.shape[1]])


def walk(A):
    """the slab maxima m, the running maxima arun and the scale exponents sexp in force, all (tiles, slabs)"""
    m = slab_maxima(A)
    arun = running_max(m)
    return dict(m=m, arun=arun, sexp=scale_exponents(arun))


def _rows(t, M):
    """a per-tile quantity (tiles, ...) for every row (M, ...)"""
    return t.repeat_interleave(TILE, dim=0)[:M]


def gemm(A, W, flush=False):
    """float64 A W^T in the kernel's arithmetic, slab by slab with the accumulator bookkeeping of the running scale;
    flush: subnormal pieces read as zero (a matrix pipe that flushes its inputs)"""
    M, K = A.shape
    sexp = _rows(walk(A)["sexp"], M)                              # (M, slabs)
    hb, lb, rb = emul.split(W, flush)
    hb, lb = hb.double(), lb.double()
    acc0 = torch.zeros(M, W.shape[0], dtype=torch.float64)
    acc1 = torch.zeros_like(acc0)
    prev = torch.zeros(M, dtype=sexp.dtype)
    one = torch.ones(M, dtype=torch.float64)
    for t in range(K // SLAB):
        k = slice(t * SLAB, (t + 1) * SLAB)
        f = torch.ldexp(one, sexp[:, t] - prev)[:, None]          # s_new / s_old: an exact power of two
        acc0, acc1 = acc0 * f, acc1 * f
        prev = sexp[:, t]
        hi, lo = emul.pieces(A[:, k].float() * torch.ldexp(torch.ones(M), sexp[:, t])[:, None], flush)
        hi, lo = hi.double(), lo.double()
        acc0 = acc0 + hi @ hb[:, k].t()
        acc1 = acc1 + hi @ lb[:, k].t() + lo @ hb[:, k].t()
    return (acc0 + acc1 * 2.0 ** -11) * torch.ldexp(one, -prev)[:, None] * rb.double()[None, :]


def bound(A, W, rel=BOUND, arun=None):
    """(bound, sum |a||w|) per output (M, N); arun: the running maxima in force where they are not walk(A)'s (a matrix
    whose non-finite row the reference replaced)"""
    M, K = A.shape
    mag = A.double().abs() @ W.double().abs().t()
    wslab = W.double().abs().view(W.shape[0], K // SLAB, SLAB).sum(2)          # (N, slabs)
    arun = walk(A)["arun"] if arun is None else arun
    floor = _rows(arun.double() @ wslab.t(), M)
    return rel * mag + FLOOR * floor, mag


def tile_amax(A):
    """(M,) float64: the largest finite magnitude of every row's 128-row tile"""
    return _rows(running_max(slab_maxima(A))[:, -1].double(), A.shape[0])


# ------------------------------------------------------------------ the inputs of the CPU and the GPU tests
SHAPES = [(1, 32, 8),            # one slab: the prologue's nt == 1 path
          (128, 64, 128),
          (129, 96, 130),        # partial tiles both ways, an odd slab count
          (300, 160, 200),
          (640, 2304, 256)]      # 72 slabs
PATTERNS = ["normal", "rising", "falling", "loud_row", "zero_tile", "zero_lead", "zero_mid", "spread"]


def inputs(pattern, M, K, N, seed=0):
    """A (M, K) and W (N, K), float32 on the CPU.  normal: N(0, 1); rising / falling: slab maxima over six decades along
    K (the scale moves at every slab / the floor term applies); loud_row: one row 1e6 above its quiet tile; zero_tile:
    an all-zero 128-row tile; zero_lead: all-zero leading slabs (m_run = 0); zero_mid: an all-zero slab between loud
    ones; spread: per-element exponents drawn from 2^-20 .. 1"""
    g = torch.Generator().manual_seed(1000 * PATTERNS.index(pattern) + M + 3 * K + 7 * N + seed)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * K ** -0.5
    ns = K // SLAB
    if pattern == "rising":
        A = (A.view(M, ns, SLAB) * torch.logspace(-3, 3, ns)[None, :, None]).reshape(M, K)
    elif pattern == "falling":
        A = (A.view(M, ns, SLAB) * torch.logspace(3, -3, ns)[None, :, None]).reshape(M, K)
    elif pattern == "loud_row":
        A = A * 1e-3
        A[min(M - 1, 133)] *= 1e6
    elif pattern == "zero_tile":
        t = min(1, (M - 1) // TILE)
        A[t * TILE:(t + 1) * TILE] = 0.0
    elif pattern == "zero_lead":
        A[:, :max(1, ns // 2) * SLAB] = 0.0
    elif pattern == "zero_mid":
        t = ns // 2
        A[:, t * SLAB:(t + 1) * SLAB] = 0.0
    elif pattern == "spread":
        A = A * torch.ldexp(torch.ones(M, K), torch.randint(-20, 1, (M, K), generator=g))
    else:
        assert pattern == "normal"
    return A.contiguous(), W.contiguous()
