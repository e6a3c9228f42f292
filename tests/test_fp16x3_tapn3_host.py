"""The one-launch fp16x3 data gradient over the three stride residues of the MPD's 32 -> 128 layer
(csrc/gemm_f16pn3.hip) -- the part that needs no GPU: the identity behind it against torch.autograd in float64 for
Hin % 3 = 0, 1, 2, the error bound of the kernel's arithmetic on its emulation (tests/fp16x3_res3_emul.py), the cut
(seq_live) and its host rule, the two new fields of f2g_epilogue, the route's tunable, and the host side of the built
library answering for the kernel's descriptor and for each refusal."""
import ctypes as C
import os
import warnings

import pytest
import torch

import fp16x3_res3_emul as emul
from fp16x3_res3_emul import REFUSALS

CIN, COUT = 32, 128
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layer(S, Hin, seed, dtype=torch.float64):
    """an upstream gradient g (S, Hout, 128) with sequence magnitudes from 1e-3 to 1e3 and the layer's weight"""
    gen = torch.Generator().manual_seed(seed)
    Hout = -(-Hin // 3)
    g = torch.randn(S, Hout, COUT, generator=gen, dtype=dtype) * torch.logspace(-3, 3, S, dtype=dtype)[:, None, None]
    w = torch.randn(COUT, CIN, 5, 1, generator=gen, dtype=dtype) * (5 * CIN) ** -0.5
    return g, w, Hout


# ------------------------------------------------------------------ the identity and the cut
@pytest.mark.parametrize("Hin", [8, 9, 10, 24, 25, 26])
def test_one_gemm_over_two_position_windows_is_the_data_gradient(Hin):
    """float64: the live part of the 96-column GEMM is autograd's gradient of F.conv2d to 1e-13 of its scale; for
    Hin % 3 != 0 the cut part is NOT zero -- stored, it would land in the halo rows"""
    g, w, Hout = _layer(4, Hin, Hin)
    want = emul.autograd_dgrad(g, w, Hin)
    rows = emul.fused_rows(emul.halo_map(g), emul.combined_weight(w), Hout)
    got, cut = emul.split_live(rows, Hin)
    scale = want.abs().amax((1, 2), keepdim=True)
    assert float(((got - want).abs() / scale).max()) < 1e-13
    assert cut.shape[1] == CIN * (3 * Hout - Hin)
    if Hin % 3:
        assert bool((cut.abs().amax(1) > 0).all())
    assert emul.seq_live_ok(Hout, Hin)


def test_the_combined_weight_has_one_zero_block():
    _, w, _ = _layer(1, 9, 1)
    wc = emul.combined_weight(w)
    assert wc.shape == (96, 256)
    assert bool((wc[:CIN, COUT:] == 0).all()) and int((wc == 0).sum()) == CIN * COUT
    assert torch.equal(wc[CIN + 5, COUT + 7], w[7, 5, 0, 0]) and torch.equal(wc[2 * CIN + 5, 7], w[7, 5, 4, 0])


@pytest.mark.parametrize("Hin", [22, 23, 24, 298, 299, 300])
def test_seq_live_arithmetic(Hin):
    """live columns per row: 96 for every row but the last, whose 32 (Hin - 3 (P0 - 1)) are 32, 64 or 96; the host
    rule holds for P0 = ceil(Hin / 3) and for no other P0"""
    P0 = -(-Hin // 3)
    live = emul.live_columns(P0, Hin)
    assert live[:-1] == [96] * (P0 - 1) and live[-1] == {1: 32, 2: 64, 0: 96}[Hin % 3]
    assert sum(live) == CIN * Hin
    assert emul.seq_live_ok(P0, Hin) and not emul.seq_live_ok(P0 + 1, Hin) and not emul.seq_live_ok(P0 - 1, Hin)


# ------------------------------------------------------------------ the kernel's arithmetic
@pytest.mark.parametrize("Hin", [22, 80, 298, 300])
def test_emulated_arithmetic_keeps_the_bound(Hin):
    """fp32 inputs through the kernel's steps (segment scale over the two-tap run, pieces, two accumulator sets,
    rescale) against float64: every LIVE output within 3 * 2^-22 sum |g||w| + 2^-28 (amax_segment sum |w| + ...)"""
    P0 = -(-Hin // 3)
    S = max(3, -(-300 // P0))
    g, w, _ = _layer(S, Hin, 7 * Hin, torch.float32)
    gmap, wc = emul.halo_map(g), emul.combined_weight(w)
    got, amax = emul.gemm(gmap, wc, P0)
    tol, _ = emul.bound(gmap, wc, P0, amax)
    want = emul.fused_rows(gmap.double(), wc.double(), P0).view(S * P0, 96)
    live = torch.tensor(emul.live_columns(P0, Hin)).repeat(S)[:, None] > torch.arange(96)[None, :]
    err = (got - want).abs()
    assert torch.isfinite(got).all()
    worst = float((err / tol)[live & (tol > 0)].max())
    print(f"Hin {Hin}: worst live error / bound {worst:.3f}")
    assert worst <= 1.0 and bool((err[tol == 0] == 0).all())
    # ... and the live part is the layer's data gradient
    dg, _ = emul.split_live(got.view(S, P0, 96), Hin)
    ref = emul.autograd_dgrad(g.double(), w.double(), Hin)
    tl, _ = emul.split_live(tol.view(S, P0, 96), Hin)
    assert bool(((dg - ref).abs() <= tl + 1e-13 * ref.abs().amax((1, 2), keepdim=True)).all())


def test_the_one_tap_residue_under_a_loud_second_position():
    """g[q + 1] 2^40 times g[q]: residue 0 reads g[q] alone but lives under the segment's scale, where g[q] is subnormal
    in its hi piece -- its error is within the floor term of the bound, amax_segment sum |w|, and far above 3 * 2^-22 of
    its own products"""
    g, w, Hout = _layer(3, 24, 5, torch.float32)
    g[:, 1::2] *= 2.0 ** 40
    gmap, wc = emul.halo_map(g), emul.combined_weight(w)
    got, amax = emul.gemm(gmap, wc, Hout)
    tol, mag = emul.bound(gmap, wc, Hout, amax)
    err = (got - emul.fused_rows(gmap.double(), wc.double(), Hout).view(-1, 96)).abs()
    assert float((err / tol).max()) <= 1.0
    quiet = err[0::2, :CIN]                 # residue 0 of the rows whose own position is the quiet one
    assert float((quiet / (emul.BOUND * mag[0::2, :CIN])).max()) > 1.0


# ------------------------------------------------------------------ the descriptor's new fields
def test_epilogue_fields_are_last_and_zero_by_default():
    from flow2gan_amd import _lib
    names = [f[0] for f in _lib.Epilogue._fields_]
    assert names[-2:] == ["col_fold", "seq_live"] and names[-3] == "colsum_part_ld"
    assert _lib.Epilogue.col_fold.offset == _lib.Epilogue.colsum_part_ld.offset + 8
    assert _lib.Epilogue.seq_live.offset == _lib.Epilogue.col_fold.offset + 8
    assert C.sizeof(_lib.Epilogue) == _lib.Epilogue.seq_live.offset + 8
    e = _lib.Epilogue()
    assert e.col_fold == 0 and e.seq_live == 0
    assert bytes(e) == bytes(C.sizeof(_lib.Epilogue))          # a fresh descriptor: all zero, the new fields included
    hdr = open(os.path.join(ROOT, "include", "flow2gan_hip.h")).read()
    tail = hdr[hdr.index("int64_t colsum_part_ld;"):hdr.index("} f2g_epilogue;")]
    assert tail.index("int32_t col_fold;") < tail.index("int64_t seq_live;")
    assert '"h3pn3"' in hdr and "gemm_h3pn3_kernel" in hdr


# ------------------------------------------------------------------ the tunable
def test_the_route_is_a_tunable_and_off_by_default():
    from flow2gan_amd import _opts, ops
    assert "fp16x3_tapn3_min_rows" in _opts._ASKED
    assert "fp16x3_tapn3_min_rows" in _opts.__doc__
    assert ops.FP16X3_TAPN3_MIN_ROWS == ops.FP16X3_TAP_OFF
    assert ops.FP16X3_TAPN3_LAUNCHES >= 0
    assert "`fp16x3_tapn3_min_rows`" in open(os.path.join(ROOT, "README.md")).read()
    routes = ops._FP16X3_ROUTES[0, "fold3"]
    assert [r.threshold for r in routes] == ["FP16X3_TAPN3_MIN_ROWS"] and routes[0].marks == (8, 0)
    assert routes[0].counter == "FP16X3_TAPN3_LAUNCHES" and routes[0].needs == 2 and not routes[0].x3_out


def test_f2g_opts_sets_the_tunable_and_the_name_is_known(monkeypatch):
    from flow2gan_amd import _opts, ops
    monkeypatch.setattr(_opts, "_OPTS", _opts._parse("FP16X3_TAPN3_MIN_ROWS=4096, fp16x3_tapn_min_rows=7"))
    assert _opts.opt("fp16x3_tapn3_min_rows", ops.FP16X3_TAP_OFF) == 4096
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert _opts.warn_unknown(lambda name: False) == []     # (no warning for the new name)
    monkeypatch.setattr(_opts, "_OPTS", _opts._parse("fp16x3_tapn_min_rows=7"))
    assert _opts.opt("fp16x3_tapn3_min_rows", ops.FP16X3_TAP_OFF) == ops.FP16X3_TAP_OFF


def test_the_python_predicate(monkeypatch):
    """the route's own test of a call: 128-channel windows of two positions, 96 weight rows, no atomics, no split, no
    three-piece image (over host tensors: ops.ptr refuses them, the predicate only compares addresses)"""
    from flow2gan_amd import ops
    monkeypatch.setattr(ops, "ptr", lambda t: None if t is None else t.data_ptr())
    claims = ops._FP16X3_ROUTES[0, "fold3"][0].claims
    S, P0 = 3, 100
    t = torch.zeros(S * (P0 + 4) * COUT)
    w = torch.zeros(96, 256)
    A = ops.win1d(t, S, P0 + 4, COUT, P0, 1, -2, 2)
    assert claims(A, ops.mat(w), False, 1, False)
    assert not claims(A, ops.mat(w), True, 1, False) and not claims(A, ops.mat(w), False, 2, False)
    assert not claims(A, ops.mat(w), False, 1, True)
    assert not claims(A, ops.mat(w[:32]), False, 1, False)
    assert not claims(ops.win1d(t, S, P0 + 4, COUT, P0, 1, -2, 1), ops.mat(w[:, :128]), False, 1, False)
    assert not claims(ops.win1d(t, 2 * S, P0 + 4, 64, P0, 1, -2, 2), ops.mat(w[:, :128]), False, 1, False)


# ------------------------------------------------------------------ the built library's host side
def _descriptor(ops, keep, S=3, P0=100, Hin=299, unit=COUT, n=96, taps=2, front=2):
    """the operands of fused_disc._conv1d_dgrad3 over host memory: the host checks never read through the pointers"""
    Hp = front + P0 + 2        # (front = HALO = 2: the halo layout; a window's second position is one behind the rows)
    flat, w = torch.zeros(S * Hp * unit), torch.zeros(n + 1, taps * unit)
    out = torch.zeros(S * (Hin + 4) * CIN)
    keep += [flat, w, out]
    d = ops.GemmDesc()
    A, B = d.A, d.B
    A.base, A.rows, A.cols, A.P1, A.P0, A.seglen, A.L1 = flat.data_ptr(), S * P0, taps * unit, 1, P0, taps * unit, 1
    A.step0, A.pad0, A.unit, A.L0u, A.seq_stride = 1, -front, unit, Hp * unit, Hp * unit
    B.base, B.rows, B.cols, B.P1, B.P0, B.seglen, B.L1 = w.data_ptr(), n, taps * unit, 1, 1, taps * unit, 1
    B.unit, B.L0u, B.seq_stride = 1, taps * unit, taps * unit
    B.split, B.rscale = 7, w.data_ptr() + 4 * n * taps * unit
    E = d.E
    E.C, E.ldc = out.data_ptr(), 96
    E.P0o, E.seq_stride_o, E.row_stride_o, E.off_o = P0, (Hin + 4) * CIN, 96, 2 * CIN
    E.col_fold, E.seq_live = CIN, CIN * Hin
    d.form, d.split_k, d.precision = 0, 1, 4
    d.A.split = 8
    return d


@pytest.fixture
def host_lib():
    from flow2gan_amd import _lib, ops
    lib = C.CDLL(_lib.LIB_PATH)
    lib.f2g_gemm_f16_ok.restype = C.c_int
    was = _lib.set_option("x6p", 2)
    try:
        yield ops, _lib, (lambda d: lib.f2g_gemm_f16_ok(C.byref(d))), lib
    finally:
        _lib.set_option("x6p", was)


def test_the_library_answers_for_the_kernels_descriptor(host_lib):
    """f2g_gemm_f16_ok (host code: nothing is launched): 1 with B's image, 2 with B fp32, 0 without the image's
    scales; no partial column-sum rows; the x6p grid option as for gemm_h3pn_kernel.  Before the kernel existed the
    descriptor was answered 0 (N = 96 is too wide for gemm_h3pn_kernel)."""
    ops, _lib, ok, lib = host_lib
    keep = []
    for Hin in (298, 299, 300):
        d = _descriptor(ops, keep, Hin=Hin)
        assert ok(d) == 1, Hin
        assert lib.f2g_gemm_colsum_part_rows(C.byref(d)) == 0
    d.B.split, d.B.rscale = 0, None
    assert ok(d) == 2
    d.B.split = 7
    assert ok(d) == 0
    d = _descriptor(ops, keep, front=0)
    assert ok(d) == 1
    _lib.set_option("x6p", 1)
    assert ok(_descriptor(ops, keep)) == 0
    assert ok(_descriptor(ops, keep, S=256, P0=128, Hin=384)) == 1
    _lib.set_option("x6p", 0)
    assert ok(_descriptor(ops, keep, S=256, P0=128, Hin=384)) == 0


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_the_library_declines(host_lib, what):
    ops, _lib, ok, lib = host_lib
    keep = []
    d = _descriptor(ops, keep)
    assert ok(d) == 1
    REFUSALS[what](keep[0].data_ptr())(d)
    assert ok(d) == 0


@pytest.mark.parametrize("kw", [dict(unit=64), dict(n=32), dict(n=64), dict(taps=1), dict(taps=3), dict(S=75, P0=4, Hin=12)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_the_library_declines_other_shapes(host_lib, kw):
    """folded and cut, but not the kernel's shape: 0 -- H3_TAPN never sees a descriptor that sets the fields"""
    ops, _lib, ok, lib = host_lib
    keep = []
    assert ok(_descriptor(ops, keep, **kw)) == 0


def test_descriptors_without_the_fields_keep_their_answers(host_lib):
    """col_fold == 0 and seq_live == 0: the residue data gradients of gemm_h3pn_kernel answer as before, and the
    96-column descriptor without the fields is nobody's"""
    ops, _lib, ok, lib = host_lib
    keep = []
    d = _descriptor(ops, keep, n=32)
    d.E.col_fold, d.E.seq_live = 0, 0
    d.E.row_stride_o = 96
    assert ok(d) == 1
    d.E.seq_live = 32 * 299
    assert ok(d) == 0
    d = _descriptor(ops, keep)
    d.E.col_fold, d.E.seq_live = 0, 0
    assert ok(d) == 0
