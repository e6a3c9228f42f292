"""fp16x3 pointwise GEMM over the fp32 activation matrix itself, scaled per 128-row tile inside the kernel
(csrc/gemm_f16n.hip) -- the part that needs no GPU: the error bound of the running tile scale on its emulation
(tests/fp16x3_runtile_emul.py) against float64 on the inputs the GPU tests use, with and without subnormal pieces; an inf
staying in its row and leaving the tile's scale alone; the route's tunable; and the host side of the built library
answering for the descriptors of the new kernel (f2g_operand.split = 9)."""
import ctypes as C
import os

import pytest
import torch

import fp16x3_runtile_emul as emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(p, s) for s in emul.SHAPES for p in emul.PATTERNS]
_REF = {}


def _case(pattern, shape):
    """the inputs, the float64 product and the bound of a case, computed once"""
    key = (pattern, shape)
    if key not in _REF:
        A, W = emul.inputs(pattern, *shape)
        tol, _ = emul.bound(A, W)
        _REF[key] = (A, W, A.double() @ W.double().t(), tol)
    return _REF[key]


def _ratio(err, tol):
    """err / tol, with 0 / 0 = 0 (the outputs of an all-zero tile are exact) and anything else over 0 = inf"""
    inf = torch.full_like(err, float("inf"))
    return torch.where(tol > 0, err / tol, torch.where(err == 0, torch.zeros_like(err), inf))


@pytest.mark.parametrize("flush", [False, True])
@pytest.mark.parametrize("pattern,shape", CASES)
def test_emulated_arithmetic_keeps_the_bound(pattern, shape, flush):
    """the check that the inputs suit the bound: every element, with the pieces as they are and with subnormal pieces
    flushed"""
    A, W, want, tol = _case(pattern, shape)
    got = emul.gemm(A, W, flush=flush)
    assert torch.isfinite(got).all()
    worst = float(_ratio((got - want).abs(), tol).max())
    print(f"{pattern} {shape} flush={flush}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, (pattern, shape, flush, worst)


def test_the_patterns_do_what_they_say():
    """rising: the scale moves at every slab; falling: it never moves after the first; zero_lead: m_run = 0 over the
    leading slabs; zero_mid and zero_tile: a zero slab / tile leaves the scale alone (scale 1 for the zero tile)"""
    M, K, N = 300, 160, 200
    w = emul.walk(emul.inputs("rising", M, K, N)[0])
    assert bool((w["sexp"][:, 1:] < w["sexp"][:, :-1]).all())
    w = emul.walk(emul.inputs("falling", M, K, N)[0])
    assert bool((w["sexp"] == w["sexp"][:, :1]).all())
    w = emul.walk(emul.inputs("zero_lead", M, K, N)[0])
    assert bool((w["arun"][:, :2] == 0).all()) and bool((w["sexp"][:, :2] == 0).all()) and bool((w["arun"][:, 2:] > 0).all())
    w = emul.walk(emul.inputs("zero_mid", M, K, N)[0])
    assert bool((w["m"][:, 2] == 0).all()) and bool((w["arun"][:, 2] == w["arun"][:, 1]).all())
    w = emul.walk(emul.inputs("zero_tile", M, K, N)[0])
    assert bool((w["arun"][1] == 0).all()) and bool((w["sexp"][1] == 0).all()) and bool((w["arun"][0] > 0).all())
    A, _ = emul.inputs("loud_row", M, K, N)
    assert float(emul.tile_amax(A)[128]) > 1e5 * float(A[128].abs().max())


def test_an_inf_stays_in_its_row_and_leaves_the_scale():
    M, K, N = 300, 160, 200
    A, W = emul.inputs("normal", M, K, N)
    A0 = A.clone()
    A[130, 40] = float("inf")
    A0[130] = 0.0                                  # (the float64 reference of the other rows does not see the inf)
    w, w0 = emul.walk(A), emul.walk(A0)
    assert torch.equal(w["sexp"][[0, 2]], w0["sexp"][[0, 2]])
    # slab 1 of tile 1 holds the inf: its maximum is not finite and the running maximum steps over it
    assert float(w["m"][1, 1]) == float("inf") and float(w["arun"][1, 1]) == float(w["arun"][1, 0])
    assert bool(torch.isfinite(w["arun"]).all())
    got = emul.gemm(A, W)
    own = torch.zeros(M, dtype=torch.bool)
    own[130] = True
    assert not bool(torch.isfinite(got[130]).any())
    assert bool(torch.isfinite(got[~own]).all())
    tol, _ = emul.bound(A0, W, arun=w["arun"])      # (the scales in force are those of the matrix WITH the row)
    want = A0.double() @ W.double().t()
    assert float(_ratio((got - want).abs()[~own], tol[~own]).max()) <= 1.0


def test_the_route_is_a_tunable_and_off_by_default():
    from flow2gan_amd import _opts, ops
    assert "fp16x3_plainn_min_n" in _opts._ASKED
    assert "fp16x3_plainn_min_n" in _opts.__doc__
    assert ops.FP16X3_PLAINN_MIN_N == ops.FP16X3_TAP_OFF
    assert ops.FP16X3_PLAINN_LAUNCHES >= 0
    assert "`fp16x3_plainn_min_n`" in open(os.path.join(ROOT, "README.md")).read()


def test_f2g_opts_sets_the_tunable(monkeypatch):
    """F2G_OPTS="fp16x3_plainn_min_n=..." reaches the declaration in ops.py (the value is typed like the default)"""
    from flow2gan_amd import _opts, ops
    monkeypatch.setattr(_opts, "_OPTS", _opts._parse("FP16X3_PLAINN_MIN_N=384, fp16x3_min_n=7"))
    assert _opts.opt("fp16x3_plainn_min_n", ops.FP16X3_TAP_OFF) == 384
    monkeypatch.setattr(_opts, "_OPTS", _opts._parse("fp16x3_min_n=7"))
    assert _opts.opt("fp16x3_plainn_min_n", ops.FP16X3_TAP_OFF) == ops.FP16X3_TAP_OFF


def _descriptor(ops, keep, M=300, K=160, N=200, ld=None):
    """the operands of ops.mat for a pointwise layer, over host memory: the host checks never read through the
    pointers"""
    ld = K + 4 if ld is None else ld
    a, w, out = torch.zeros(8 + min(M, 512) * ld), torch.zeros(N * K + N), torch.zeros(min(M, 512) * N)
    keep += [a, w, out]
    d = ops.GemmDesc()
    A, B = d.A, d.B
    A.base, A.rows, A.cols, A.P1, A.P0, A.seglen, A.L1 = a.data_ptr(), M, K, 1, 1, K, 1
    A.unit, A.L0u, A.seq_stride = 1, K, ld
    B.base, B.rows, B.cols, B.P1, B.P0, B.seglen, B.L1 = w.data_ptr(), N, K, 1, 1, K, 1
    B.unit, B.L0u, B.seq_stride = 1, K, K
    d.E.C, d.E.ldc = out.data_ptr(), N
    d.form, d.split_k, d.precision = 0, 1, 4
    return d


def _imaged(d, keep):
    """B as its f2g_split_f16x2 image with scales (host pointers: never read)"""
    d.B.split, d.B.rscale = 5, keep[-2].data_ptr() + 4 * d.B.rows * d.B.cols
    return d


def test_the_library_answers_for_the_new_kernels_descriptors():
    """the built library's f2g_gemm_f16_ok and f2g_gemm_colsum_part_rows (host code: nothing is launched): 2 with B
    fp32, 1 with B's image and rscale, 0 for what the kernel declines.  On the commit before the kernel the marked
    descriptor is answered 0 (9 was no operand mark)."""
    from flow2gan_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "flow2gan_hip.h")).read()
    assert '"h3n<ep=all>"' in hdr and "gemm_h3n_kernel" in hdr
    lib = C.CDLL(_lib.LIB_PATH)
    lib.f2g_gemm_f16_ok.restype = C.c_int
    keep = []
    ok = lambda d: lib.f2g_gemm_f16_ok(C.byref(d))
    d = _descriptor(ops, keep)
    d.A.split = 9
    assert ok(d) == 2                                   # "once B is replaced by its image"
    assert lib.f2g_gemm_colsum_part_rows(C.byref(d)) == 0
    _imaged(d, keep)
    assert ok(d) == 1
    assert lib.f2g_gemm_colsum_part_rows(C.byref(d)) == 0
    d.B.rscale = None
    assert ok(d) == 0                                   # an image without its scales
    for shape in emul.SHAPES:                           # every shape of the GPU tests, ld > K
        dd = _imaged(_descriptor(ops, keep, *shape), keep)
        dd.A.split = 9
        assert ok(dd) == 1, shape

    def declined(change, **kw):
        dd = _imaged(_descriptor(ops, keep, **kw), keep)
        dd.A.split = 9
        assert kw or ok(dd) == 1      # (without keywords: the accepted descriptor, then one change)
        change(dd)
        return ok(dd) == 0

    spare = keep[0].data_ptr()
    assert declined(lambda dd: setattr(dd.A, "rscale", spare))           # there is no image of A: no scales
    assert declined(lambda dd: setattr(dd, "split_k", 2))
    assert declined(lambda dd: setattr(dd.E, "x3_out", spare))
    assert declined(lambda dd: setattr(dd.E, "colsum_part_ld", 204))
    assert declined(lambda dd: setattr(dd.E, "c_bf16", 1))
    # the epilogue combinations f2g_gemm refuses for every kernel
    assert declined(lambda dd: (setattr(dd.E, "prelu_slope", spare), setattr(dd.E, "accumulate", 1)))
    assert declined(lambda dd: (setattr(dd.E, "prelu_slope", spare), setattr(dd.E, "atomic", 1)))
    assert declined(lambda dd: (setattr(dd.E, "prelu_slope", spare), setattr(dd.E, "P0o", 10)))
    assert declined(lambda dd: (setattr(dd.E, "mask_src", spare), setattr(dd.E, "accumulate", 1)))
    assert declined(lambda dd: setattr(dd.E, "aux", spare))              # (without alpha_n)
    assert declined(lambda dd: setattr(dd.A, "alpha", spare))
    assert declined(lambda dd: None, K=48, ld=48)                        # K % 32
    assert declined(lambda dd: None, K=16, ld=16)
    assert declined(lambda dd: None, K=4128, ld=4128)                    # K > F2G_F16_MAX_K
    assert not declined(lambda dd: None, K=4096, ld=4096)
    assert declined(lambda dd: setattr(dd.A, "base", dd.A.base + 4))     # alignment
    assert declined(lambda dd: None, ld=162)
    assert declined(lambda dd: setattr(dd.A, "seq_stride", 128))         # rows that overlap
    assert declined(lambda dd: None, M=(1 << 20), K=512, ld=512)         # the 32-bit offset limit
    assert not declined(lambda dd: None, M=(1 << 20) - 2048, K=512, ld=512)
    assert declined(lambda dd: setattr(dd.B, "cols", 128))               # the reductions differ
    assert declined(lambda dd: setattr(dd.B, "split", 7))                # another kernel's image
    assert declined(lambda dd: setattr(dd.B, "split", 9))                # the mark belongs to A
    assert declined(lambda dd: setattr(dd, "form", 2))
    assert declined(lambda dd: setattr(dd, "form", 1))
    # a window operand so marked (stride-1 windows of 5 positions over a halo map)
    assert declined(lambda dd: (setattr(dd.A, "P0", 100), setattr(dd.A, "step0", 1), setattr(dd.A, "unit", 32),
                                setattr(dd.A, "seq_stride", 104 * 32), setattr(dd.A, "L0u", 104 * 32)))


def test_other_descriptors_keep_their_answers():
    """the same descriptor unmarked, as images, and a split-8 plain descriptor answer as before the mark existed"""
    from flow2gan_amd import _lib, ops
    lib = C.CDLL(_lib.LIB_PATH)
    lib.f2g_gemm_f16_ok.restype = C.c_int
    keep = []
    ok = lambda d: lib.f2g_gemm_f16_ok(C.byref(d))
    d = _descriptor(ops, keep)
    assert ok(d) == 2                                   # both fp32: gemm_h3_kernel once both are images
    _imaged(d, keep)
    assert ok(d) == 0                                   # mixed: A fp32 and unmarked, B an image
    d.A.split, d.A.rscale = 5, keep[0].data_ptr()
    assert ok(d) == 1                                   # both images
    assert lib.f2g_gemm_colsum_part_rows(C.byref(d)) == 0
    d = _descriptor(ops, keep)
    d.A.split = 8                                       # the halo-map mark on a plain matrix: no kernel's
    assert ok(d) == 0
    _imaged(d, keep)
    assert ok(d) == 0
    d.B.split = 7
    assert ok(d) == 0
    d = _descriptor(ops, keep)
    d.form, d.E.atomic = 2, 1
    d.B.seq_stride = d.B.cols
    d.A.rows = d.B.rows = 200
    d.A.split = d.B.split = 9                           # the mark means nothing at form 2
    assert ok(d) == 0
