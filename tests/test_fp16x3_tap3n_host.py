"""fp16x3 over stride-3 windows of five positions of a 32-channel halo map, scaled per sequence segment inside the
kernel (csrc/gemm_f16p3n.hip) -- the part that needs no GPU: the error bound of the segment scale on its emulation
(tests/fp16x3_seg_emul.py) against float64, for row groups of 64 and 128 rows and 16, 6 and 2 segments per 128 rows
(P0 = 8, 27, 100; the kernel's table holds the 17 a group that starts inside a sequence of 8 could touch);
the route's tunable; and the host side of the built library answering for the operand code the header newly declares
(f2g_operand.split = 8)."""
import ctypes as C
import os
import re

import pytest
import torch

import fp16x3_seg_emul as emul

CC, N = 32, 128
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(P0, seed, extra=2):
    """a map of enough sequences for three 128-row groups, sequences over 60 decades (as
    tests/fp16x3_gpu.py: case), and the layer's weights"""
    S = max(3, -(-300 // P0))
    Hp = emul.STEP * (P0 - 1) + emul.TAPS + extra
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, Hp, CC, generator=g) * torch.logspace(-30, 30, S)[:, None, None]
    w = torch.randn(N, emul.TAPS * CC, generator=g) * (emul.TAPS * CC) ** -0.5
    return x, w


def _ratio(err, tol):
    """err / tol, with 0 / 0 = 0 (the outputs of an all-zero sequence are exact) and anything else over 0 = inf"""
    inf = torch.full_like(err, float("inf"))
    return torch.where(tol > 0, err / tol, torch.where(err == 0, torch.zeros_like(err), inf))


def _worst(x, w, P0, group, rows=None):
    got, amax = emul.gemm(x, w, P0, group)
    want = emul.windows(x.double(), P0) @ w.double().t()
    tol, _ = emul.bound(x, w, P0, amax)
    rows = slice(None) if rows is None else rows
    err = (got - want).abs()[rows]
    assert torch.isfinite(got[rows]).all()
    return float(_ratio(err, tol[rows]).max())


@pytest.mark.parametrize("group", [64, 128])
@pytest.mark.parametrize("P0", [8, 27, 100])
def test_emulated_arithmetic_keeps_the_bound(P0, group):
    x, w = _inputs(P0, 100 * P0 + group)
    nseg = max(len([1 for r, *_ in emul.segments(x.shape[0], P0, 128) if m0 <= r < m0 + 128])
               for m0 in range(0, x.shape[0] * P0, 128))
    assert nseg == {8: 16, 27: 6, 100: 2}[P0]      # (P0 = 8 divides the group: 16 of the 17 the kernel's table holds)
    worst = _worst(x, w, P0, group)
    print(f"P0 {P0}, groups of {group}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, (P0, group, worst)


def test_segments_per_group_stay_within_the_kernels_table():
    """the host rule P0 >= 8 admits at most 17 segments per 128 rows -- reached when a group starts inside a sequence"""
    most = 0
    for P0 in (8, 9, 27, 100):
        for S in (40, 41):
            segs = emul.segments(S, P0, 128)
            most = max(most, max(sum(1 for r, *_ in segs if m0 <= r < m0 + 128) for m0 in range(0, S * P0, 128)))
            assert all(emul.STEP * (pb - pa + 1) + 2 >= emul.TAPS for _, _, pa, pb in segs)
    assert most == 16          # (8 | 128: aligned; 9: 128 / 9 + 2 = 16)
    assert 2 + 126 // 8 == 17


@pytest.mark.parametrize("group", [64, 128])
def test_an_all_zero_sequence(group):
    x, w = _inputs(27, 7)
    x[3] = 0.0
    got, _ = emul.gemm(x, w, 27, group)
    assert bool((got[3 * 27:4 * 27] == 0).all())
    assert _worst(x, w, 27, group) <= 1.0


@pytest.mark.parametrize("group", [64, 128])
def test_an_inf_touches_its_own_sequence_only(group):
    P0 = 27
    x, w = _inputs(P0, 9)
    x[4, 40, 5] = float("inf")
    clean = torch.ones(x.shape[0] * P0, dtype=torch.bool)
    clean[4 * P0:5 * P0] = False
    xs = x.clone()
    xs[4] = 0.0               # (the float64 reference of the other sequences' rows does not see the inf)
    got, amax = emul.gemm(x, w, P0, group)
    want = emul.windows(xs.double(), P0) @ w.double().t()
    tol, _ = emul.bound(xs, w, P0, torch.where(clean, amax, torch.zeros_like(amax)))
    assert torch.isfinite(got[clean]).all()
    assert float(_ratio((got - want).abs()[clean], tol[clean]).max()) <= 1.0
    assert not torch.isfinite(got[~clean]).all()


def test_the_route_is_a_tunable_and_off_by_default():
    from flow2gan_amd import _opts, ops
    assert "fp16x3_tap3n_min_rows" in _opts._ASKED
    assert "fp16x3_tap3n_min_rows" in _opts.__doc__
    assert ops.FP16X3_TAP3N_MIN_ROWS == ops.FP16X3_TAP_OFF
    assert ops.FP16X3_TAP3N_LAUNCHES >= 0


def test_the_library_answers_for_the_operand_code_the_header_declares():
    """include/flow2gan_hip.h declares f2g_operand.split = 8; the built library's f2g_gemm_f16_ok and
    f2g_gemm_colsum_part_rows (host code: nothing is launched) answer for it"""
    from flow2gan_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "flow2gan_hip.h")).read()
    assert re.search(r"\* 8: \(operand A of a precision-4, form-0 launch only\)", hdr)
    assert '"h3p3n<taps=5,step=3>"' in hdr
    S, P0, Hp = 3, 100, 3 * 99 + 5 + 2
    flat, w, out = torch.zeros(S * Hp * CC), torch.zeros(N, 5 * CC), torch.zeros(S * P0, N)
    d = ops.GemmDesc()
    # (the operands of ops.win1d / ops.mat, over host memory: the host checks never read through the pointers)
    A, B = d.A, d.B
    A.base, A.rows, A.cols, A.P1, A.P0, A.seglen, A.L1 = flat.data_ptr(), S * P0, 5 * CC, 1, P0, 5 * CC, 1
    A.step0, A.pad0, A.unit, A.L0u, A.seq_stride = 3, 0, CC, Hp * CC, Hp * CC
    B.base, B.rows, B.cols, B.P1, B.P0, B.seglen, B.L1 = w.data_ptr(), N, 5 * CC, 1, 1, 5 * CC, 1
    B.unit, B.L0u, B.seq_stride = 1, 5 * CC, 5 * CC
    d.E.C, d.E.ldc = out.data_ptr(), N
    d.form, d.split_k, d.precision = 0, 1, 4
    lib = C.CDLL(_lib.LIB_PATH)
    lib.f2g_gemm_f16_ok.restype = C.c_int
    was = _lib.set_option("x6p", 2)
    try:
        assert lib.f2g_gemm_f16_ok(C.byref(d)) == 0          # unit == 32 at stride 3, unmarked: as before
        d.A.split = 8
        assert lib.f2g_gemm_f16_ok(C.byref(d)) == 2          # "once B is replaced by its image"
        assert lib.f2g_gemm_colsum_part_rows(C.byref(d)) == 2 * ((S * P0 + 127) // 128)
        d.B.split, d.B.rscale = 7, out.data_ptr()
        assert lib.f2g_gemm_f16_ok(C.byref(d)) == 1
        d.A.P0, d.A.rows = 4, S * P0
        assert lib.f2g_gemm_f16_ok(C.byref(d)) == 0
    finally:
        _lib.set_option("x6p", was)
