"""fp16x3 over stride-1 windows of two or one positions of a 128-channel halo map onto at most 32 columns, scaled per
sequence segment inside the kernel (csrc/gemm_f16pn.hip) -- the part that needs no GPU: the error bound of the segment
scale on its emulation (tests/fp16x3_seg1_emul.py) against float64, for taps 2 and 1 and 16, 6 and 2 segments per 128
rows (P0 = 8, 27, 100); the kernel's index arithmetic inside its tables (17 segments, 145 staged positions per tile);
the route's tunable; and the host side of the built library answering for the descriptors of the new kernel."""
import ctypes as C
import os

import pytest
import torch

import fp16x3_seg1_emul as emul

CC, N = 128, 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(P0, taps, seed, extra=2):
    """a map of enough sequences for three 128-row groups, sequence magnitudes from 1e-3 to 1e3 (a scale taken from
    the wrong sequence is wrong by orders of magnitude), and the layer's weights"""
    S = max(3, -(-300 // P0))
    Hp = P0 + taps - 1 + extra
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, Hp, CC, generator=g) * torch.logspace(-3, 3, S)[:, None, None]
    w = torch.randn(N, taps * CC, generator=g) * (taps * CC) ** -0.5
    return x, w


def _ratio(err, tol):
    """err / tol, with 0 / 0 = 0 (the outputs of an all-zero sequence are exact) and anything else over 0 = inf"""
    inf = torch.full_like(err, float("inf"))
    return torch.where(tol > 0, err / tol, torch.where(err == 0, torch.zeros_like(err), inf))


def _worst(x, w, P0, taps, rows=None):
    got, amax = emul.gemm(x, w, P0, taps, 128)
    want = emul.windows(x.double(), P0, taps) @ w.double().t()
    tol, _ = emul.bound(x, w, P0, taps, amax)
    rows = slice(None) if rows is None else rows
    err = (got - want).abs()[rows]
    assert torch.isfinite(got[rows]).all()
    return float(_ratio(err, tol[rows]).max())


@pytest.mark.parametrize("taps", [2, 1])
@pytest.mark.parametrize("P0", [8, 27, 100])
def test_emulated_arithmetic_keeps_the_bound(P0, taps):
    x, w = _inputs(P0, taps, 100 * P0 + taps)
    nseg = max(len([1 for r, *_ in emul.segments(x.shape[0], P0, 128) if m0 <= r < m0 + 128])
               for m0 in range(0, x.shape[0] * P0, 128))
    assert nseg == {8: 16, 27: 6, 100: 2}[P0]      # (P0 = 8 divides the group: 16 of the 17 the kernel's table holds)
    worst = _worst(x, w, P0, taps)
    print(f"P0 {P0}, taps {taps}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, (P0, taps, worst)


@pytest.mark.parametrize("taps", [2, 1])
def test_a_tiles_segments_and_entries_stay_within_the_kernels_tables(taps):
    """the host rule P0 >= 8 admits at most 17 segments and 128 + 17 (taps - 1) staged positions per tile; every entry
    the kernel places by its multiply-shift lies where the walk over the segments puts it, and every tap of every
    valid row reads a staged entry of its own sequence"""
    most_seg = most_L = 0
    sizes = [(P0, S) for P0 in list(range(8, 41)) + [63, 64, 65, 100, 127, 128, 129, 144, 145, 146] for S in (1, 3, 41)]
    sizes += [(P0, S) for P0 in (255, 1000, 65535, 70000) for S in (1, 2)]
    for P0, S in sizes:
        M = S * P0
        tiles = {}
        for seg in emul.segments(S, P0, 128):
            tiles.setdefault(seg[0] // 128 * 128, []).append(seg)
        for m0, segs in tiles.items():
            sq0, rl0, E0, EP, L = emul.tile_geometry(M, P0, taps, m0)
            want, where = [], {}
            for r, s, pa, pb in segs:
                for p in range(pa, pb + 1):
                    where[r + p - pa] = (len(want) + p - pa, s)
                want += [(s - sq0, p) for p in range(pa, pb + taps)]
            assert L == len(want) and rl0 == want[0][1]
            assert [emul.entry_place(e, rl0, E0, EP) for e in range(L)] == want
            for r, (entry, s) in where.items():
                assert emul.row_entry(r, P0, sq0, rl0, E0, EP) == entry
                assert all(want[entry + t][0] == s - sq0 for t in range(taps))
            most_seg, most_L = max(most_seg, want[-1][0] + 1), max(most_L, L)
    # (reached: 16 -- 8 | 128 keeps P0 = 8 aligned, and P0 = 9 gives 1 + 14 + 1; the kernel's table holds the 17 of a
    # tile that started inside a sequence of 8)
    assert most_seg == 16 <= emul.NSEG == 2 + 126 // 8
    assert most_L == 128 + 16 * (taps - 1) <= 128 + emul.NSEG * (taps - 1) <= 145


@pytest.mark.parametrize("taps", [2, 1])
def test_an_all_zero_sequence(taps):
    x, w = _inputs(27, taps, 7)
    x[3] = 0.0
    got, _ = emul.gemm(x, w, 27, taps, 128)
    assert bool((got[3 * 27:4 * 27] == 0).all())
    assert _worst(x, w, 27, taps) <= 1.0


@pytest.mark.parametrize("taps", [2, 1])
def test_an_inf_touches_its_own_segment_only(taps):
    """P0 = 100: sequence 1 is rows 100 .. 199, its segments rows 100 .. 127 and 128 .. 199; an inf at position 50
    (read by rows 149 - taps + 1 .. 150) makes rows of the second segment non-finite and of no other"""
    P0 = 100
    x, w = _inputs(P0, taps, 9)
    x[1, 50, 5] = float("inf")
    own = torch.zeros(x.shape[0] * P0, dtype=torch.bool)
    own[128:200] = True
    xs = x.clone()
    xs[1, 50, 5] = 0.0        # (the float64 reference of the other rows does not see the inf)
    got, amax = emul.gemm(x, w, P0, taps, 128)
    want = emul.windows(xs.double(), P0, taps) @ w.double().t()
    tol, _ = emul.bound(xs, w, P0, taps, torch.where(own, torch.zeros_like(amax), amax))
    assert torch.isfinite(got[~own]).all()
    assert float(_ratio((got - want).abs()[~own], tol[~own]).max()) <= 1.0
    assert not torch.isfinite(got[150]).all()


def test_the_route_is_a_tunable_and_off_by_default():
    from flow2gan_amd import _opts, ops
    assert "fp16x3_tapn_min_rows" in _opts._ASKED
    assert "fp16x3_tapn_min_rows" in _opts.__doc__
    assert ops.FP16X3_TAPN_MIN_ROWS == ops.FP16X3_TAP_OFF
    assert ops.FP16X3_TAPN_LAUNCHES >= 0
    assert "`fp16x3_tapn_min_rows`" in open(os.path.join(ROOT, "README.md")).read()


def test_f2g_opts_sets_the_tunable(monkeypatch):
    """F2G_OPTS="fp16x3_tapn_min_rows=..." reaches the declaration in ops.py (the value is typed like the default)"""
    from flow2gan_amd import _opts, ops
    monkeypatch.setattr(_opts, "_OPTS", _opts._parse("FP16X3_TAPN_MIN_ROWS=4096, fp16x3_tap3n_min_rows=7"))
    assert _opts.opt("fp16x3_tapn_min_rows", ops.FP16X3_TAP_OFF) == 4096
    monkeypatch.setattr(_opts, "_OPTS", _opts._parse("fp16x3_tap3n_min_rows=7"))
    assert _opts.opt("fp16x3_tapn_min_rows", ops.FP16X3_TAP_OFF) == ops.FP16X3_TAP_OFF


def _descriptor(ops, taps, keep, S=3, P0=100, unit=CC, n=N):
    """the operands of ops.win1d / ops.mat for the layer's residue data gradient, over host memory: the host checks
    never read through the pointers"""
    Hp = P0 + taps - 1 + 2
    flat, w, out = torch.zeros(S * Hp * unit), torch.zeros(n, taps * unit), torch.zeros(S * P0, n)
    keep += [flat, w, out]
    d = ops.GemmDesc()
    A, B = d.A, d.B
    A.base, A.rows, A.cols, A.P1, A.P0, A.seglen, A.L1 = flat.data_ptr(), S * P0, taps * unit, 1, P0, taps * unit, 1
    A.step0, A.pad0, A.unit, A.L0u, A.seq_stride = 1, 0, unit, Hp * unit, Hp * unit
    B.base, B.rows, B.cols, B.P1, B.P0, B.seglen, B.L1 = w.data_ptr(), n, taps * unit, 1, 1, taps * unit, 1
    B.unit, B.L0u, B.seq_stride = 1, taps * unit, taps * unit
    d.E.C, d.E.ldc = out.data_ptr(), n
    d.form, d.split_k, d.precision = 0, 1, 4
    d.A.split = 8
    return d


@pytest.mark.parametrize("taps", [2, 1])
def test_the_library_answers_for_the_new_kernels_descriptors(taps):
    """the built library's f2g_gemm_f16_ok and f2g_gemm_colsum_part_rows (host code: nothing is launched): 2 with B
    fp32, 1 with B's image, 0 for what the kernel declines -- and the same descriptor unmarked keeps the answer it
    had.  On the commit before the kernel the marked descriptor is answered 0 (stride-1 windows were not a user of
    f2g_operand.split = 8)."""
    from flow2gan_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "flow2gan_hip.h")).read()
    assert '"h3pn<taps=2>"' in hdr and '"h3pn<taps=1>"' in hdr and "gemm_h3pn_kernel" in hdr
    lib = C.CDLL(_lib.LIB_PATH)
    lib.f2g_gemm_f16_ok.restype = C.c_int
    keep = []
    ok = lambda d: lib.f2g_gemm_f16_ok(C.byref(d))
    was = _lib.set_option("x6p", 2)
    try:
        d = _descriptor(ops, taps, keep)
        assert ok(d) == 2                                   # "once B is replaced by its image"
        assert lib.f2g_gemm_colsum_part_rows(C.byref(d)) == 0
        d.B.split, d.B.rscale = 7, keep[-1].data_ptr()
        assert ok(d) == 1
        assert lib.f2g_gemm_colsum_part_rows(C.byref(d)) == 0
        d.B.rscale = None
        assert ok(d) == 0                                   # an image without its scales
        d.B.rscale = keep[-1].data_ptr()
        d.A.pad0 = -2                                       # (as production hands it: windows from inside the halo)
        d.A.L0u = d.A.seq_stride = d.A.seq_stride + 2 * CC
        assert ok(d) == 1

        def declined(change, **kw):
            dd = _descriptor(ops, taps, keep, **kw)
            dd.B.split, dd.B.rscale = 7, keep[-1].data_ptr()
            assert kw or ok(dd) == 1      # (without keywords: the accepted descriptor, then one change)
            change(dd)
            return ok(dd) == 0

        assert declined(lambda dd: None, unit=64)
        assert declined(lambda dd: setattr(dd.A, "step0", 2))
        assert declined(lambda dd: None, n=40)
        assert declined(lambda dd: None, S=75, P0=4)
        assert declined(lambda dd: setattr(dd.A, "pad0", 1))
        assert declined(lambda dd: setattr(dd.E, "x3_out", keep[0].data_ptr()))
        assert declined(lambda dd: setattr(dd.E, "colsum_part_ld", 32))
        assert declined(lambda dd: setattr(dd.E, "accumulate", 1))
        assert declined(lambda dd: setattr(dd.E, "scale", 2.0))
        assert declined(lambda dd: setattr(dd, "split_k", 2))
        # three positions: cols == 3 * 128
        d3 = _descriptor(ops, 3, keep)
        d3.B.split, d3.B.rscale = 7, keep[-1].data_ptr()
        assert ok(d3) == 0
        # x6p = 1: only grids of at least 256 row tiles
        _lib.set_option("x6p", 1)
        dd = _descriptor(ops, taps, keep)
        assert ok(dd) == 0
        big = _descriptor(ops, taps, keep, S=256, P0=128)
        assert ok(big) == 2
        _lib.set_option("x6p", 0)
        assert ok(big) == 0
    finally:
        _lib.set_option("x6p", was)
