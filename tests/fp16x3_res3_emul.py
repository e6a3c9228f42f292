"""CPU restatement of the ONE-launch data gradient of Conv2d(Cin -> Cout, (5, 1), stride (3, 1), padding (2, 0)) over
its three stride residues (csrc/gemm_f16pn3.hip, gemm_h3pn3_kernel; f2g_epilogue.col_fold / seq_live).

  identity   with Hout = ceil(Hin / 3), input row h = 3 q + rho receives
                 rho = 0: g[q] w[2]      rho = 1: g[q] w[3] + g[q + 1] w[0]      rho = 2: g[q] w[4] + g[q + 1] w[1]
             (g[Hout] = 0: the halo row), so rows 3 q .. 3 q + 2 of the result are the 3 Cin columns of ONE forward GEMM
             over the windows [g[q], g[q + 1]] against
                 Wc[rho Cin + ci][j Cout + co] = w[co][ci][t(rho, j)],  t = (2, -), (3, 0), (4, 1),  block (0, 1) zero
  cut        column c of row q is real only while 3 Cin q + c < Cin Hin: for Hin % 3 != 0 the last row of a sequence
             computes values for map rows behind the sequence's end (live_columns)
  arithmetic the kernel's, per 128-row tile: tests/fp16x3_seg1_emul.py with taps = 2 and Wc as the weight -- one scale
             per segment over the two-tap run, hi / lo pieces, two accumulator sets, rescale by the segment's and the
             weight row's reciprocal scales (weight rows: tests/fp16x3_seq_emul.py's image, one scale per row).  The
             kernel never multiplies the zero block; zeros split into zeros, so the sums are the same
  bound      the family's: 3 * 2^-22 sum |g||w| + 2^-28 amax_segment sum |w| per output (seg1.bound).  The one-tap
             residue lives under the scale of a segment that also holds g[q + 1]: amax_segment <= amax_seq covers it
"""
import torch
import torch.nn.functional as F

import fp16x3_seg1_emul as seg1
from fp16x3_emul import BOUND, FLOOR    # noqa: F401 -- the tests read them from here (one floor: the per-sequence
                                        # one the GPU tests use bounds the per-segment one)

TAPS = ((2, None), (3, 0), (4, 1))      # t(rho, j): the tap through which g[q + j] reaches row 3 q + rho


def combined_weight(w):
    """Wc (3 Cin, 2 Cout) of the conv weight w (Cout, Cin, 5, 1)"""
    Cout, Cin = w.shape[:2]
    wc = torch.zeros(3 * Cin, 2 * Cout, dtype=w.dtype)
    for rho, taps in enumerate(TAPS):
        for j, t in enumerate(taps):
            if t is not None:
                wc[rho * Cin:(rho + 1) * Cin, j * Cout:(j + 1) * Cout] = w[:, :, t, 0].t()
    return wc


def autograd_dgrad(g, w, Hin):
    """d/dx of sum(conv2d(x, w) * g) by torch.autograd in the dtype of g: g (S, Hout, Cout) channels-last -> (S, Hin,
    Cin) channels-last"""
    S, Hout, Cout = g.shape
    x = torch.zeros(S, w.shape[1], Hin, 1, dtype=g.dtype, requires_grad=True)
    y = F.conv2d(x, w.to(g.dtype), stride=(3, 1), padding=(2, 0))
    assert y.shape == (S, Cout, Hout, 1)
    y.backward(g.permute(0, 2, 1)[..., None])
    return x.grad[..., 0].permute(0, 2, 1).contiguous()


def halo_map(g):
    """(S, Hout + 1, Cout): g with the zero row the last window's second position reads"""
    return torch.cat([g, torch.zeros_like(g[:, :1])], 1)


def fused_rows(gmap, wc, P0):
    """(S, P0, 3 Cin) = windows [g[q], g[q + 1]] of the map (S, >= P0 + 1, Cout) against Wc, in the map's dtype"""
    return (seg1.windows(gmap, P0, 2) @ wc.to(gmap.dtype).t()).view(gmap.shape[0], P0, -1)


def live_columns(P0, Hin, Cin=32):
    """per row q of a sequence: the columns of its 3 Cin in front of seq_live = Cin Hin (the kernel's LDS word)"""
    return [max(0, min(3 * Cin, Cin * Hin - 3 * Cin * q)) for q in range(P0)]


def seq_live_ok(P0, Hin, Cin=32):
    """the host rule: the cut lies in the last row of a sequence and leaves it at least one channel group"""
    live = Cin * Hin
    return live % Cin == 0 and 3 * Cin * (P0 - 1) < live <= 3 * Cin * P0


def split_live(rows, Hin):
    """(the (S, Hin, Cin) data gradient, the cut tail (S, 3 Cin P0 - Cin Hin)) of fused_rows' result"""
    S, P0, n3 = rows.shape
    Cin = n3 // 3
    flat = rows.reshape(S, P0 * n3)
    return flat[:, :Cin * Hin].reshape(S, Hin, Cin), flat[:, Cin * Hin:]


def gemm(gmap, wc, P0, group=128):
    """the kernel's arithmetic for every tile of `group` rows: (float64 (S P0, 3 Cin), amax_segment per row)"""
    return seg1.gemm(gmap, wc, P0, 2, group)


def bound(gmap, wc, P0, amax_segment):
    """(per-output bound, sum |g||w|)"""
    return seg1.bound(gmap, wc, P0, 2, amax_segment)


# ---- the descriptors gemm_h3pn3_kernel declines: one change each of the descriptor it runs, (any valid pointer) ->
# change(descriptor).  tests/test_fp16x3_tapn3_host.py asks the host code, tests/test_hip_gemm_f16_tapn3.py launches them
def _set(obj, **kw):
    def change(d):
        for k, v in kw.items():
            setattr(getattr(d, obj) if obj else d, k, v)
    return change


REFUSALS = {
    # the epilogue terms the kernel does not have (p: any valid pointer)
    "bias": lambda p: _set("E", bias=p), "lrelu_slope": lambda p: _set("E", lrelu_slope=0.1),
    "aux": lambda p: _set("E", aux=p, ldaux=96, alpha_n=p), "res": lambda p: _set("E", res=p, ldres=96),
    "colsum_alpha": lambda p: _set("E", colsum_alpha=p), "prelu_slope": lambda p: _set("E", prelu_slope=p),
    "prelu_out": lambda p: _set("E", prelu_out=p, ld_prelu_out=96), "scale": lambda p: _set("E", scale=2.0),
    "atomic": lambda p: _set("E", atomic=1), "accumulate": lambda p: _set("E", accumulate=1),
    "c_bf16": lambda p: _set("E", c_bf16=1), "x3_out": lambda p: _set("E", x3_out=p),
    "colsum_part_ld": lambda p: _set("E", colsum_part_ld=96), "split_k": lambda p: _set("", split_k=2),
    # the fold and the cut
    "col_fold=0": lambda p: _set("E", col_fold=0), "col_fold=16": lambda p: _set("E", col_fold=16),
    "seq_live=0": lambda p: _set("E", seq_live=0), "seq_live%32": lambda p: _set("E", seq_live=32 * 299 + 8),
    "seq_live short": lambda p: _set("E", seq_live=96 * 99), "seq_live long": lambda p: _set("E", seq_live=96 * 100 + 32),
    "P0o": lambda p: _set("E", P0o=99), "no row map": lambda p: _set("E", P0o=0), "row_stride_o": lambda p: _set("E", row_stride_o=128),
    # the operand
    "step0": lambda p: _set("A", step0=3), "pad0": lambda p: _set("A", pad0=1), "unmarked": lambda p: _set("A", split=0),
    "image of A": lambda p: _set("A", split=7, rscale=p), "misaligned": lambda p: _set("A", base=p + 4),
    "form 2": lambda p: _set("", form=2), "precision 3": lambda p: _set("", precision=3),
}
