"""Host-side checks of the fp16x3 weight gradient of the MPD's 32 -> 128 layer, scaled inside the kernel
(csrc/gemm_f16wsn.hip): the error bound of the arithmetic with one monotone running scale per operand and block, over
the emulation (tests/fp16x3_runwin3_emul.py), the partition of the walk, the walk of the running scales, the Python-side
tunable and counter, and the built library's answers for the layer's descriptor (host code: nothing is launched).

The bound, per output:  3 * 2^-22 sum |g||x| + 2^-28 sum_T (xrun_T sum_{rows in T} |g| + grun_T sum_{rows in T} |x_win|)."""
import ctypes as C

import pytest
import torch

import fp16x3_runwin3_emul as emul

HALO, PAD, CIN, COUT = 2, 6, 32, 128


def hout_of(hin):
    return (hin - 1) // 3 + 1


def halo(v):
    """(S, H, C) -> the flat halo layout (S * (H + 2 HALO), C) with zero halo rows"""
    out = torch.zeros(v.shape[0], v.shape[1] + 2 * HALO, v.shape[2], dtype=v.dtype)
    out[:, HALO:HALO + v.shape[1]] = v
    return out.reshape(-1, v.shape[2])


def layer(S, hin, how, seed, cout=COUT):
    """(g, x, geometry) of the layer with sequence magnitudes `how`"""
    gen = torch.Generator().manual_seed(seed)
    gv, xv = torch.randn(S, hout_of(hin), cout, generator=gen), torch.randn(S, hin, CIN, generator=gen)
    mags = {"flat": torch.ones(S), "rising": torch.logspace(-3, 3, S), "falling": torch.logspace(3, -3, S)}[how]
    gv, xv = gv * mags[:, None, None], xv * mags[:, None, None]
    return halo(gv), halo(xv), (S, hin + 2 * HALO, hout_of(hin) + 2 * HALO, PAD)


# (S, Hin): Hp = 7 (one partial slab), 17, 104 (seven slabs; 40 sequences = 280 units on 17 blocks)
SHAPES = [(5, 7), (6, 37), (40, 300)]


@pytest.mark.parametrize("S,hin", SHAPES)
@pytest.mark.parametrize("how", ["flat", "rising", "falling"])
def test_bound_holds(S, hin, how):
    g, x, geo = layer(S, hin, how, seed=hin, cout=24)
    assert geo[2] in (7, 17, 104)
    got, want = emul.wgrad(g, x, *geo), emul.exact_wgrad(g, x, *geo)
    bnd, mag = emul.bound_wgrad(g, x, *geo)
    err = (got - want).abs()
    print(f"[h3wsn emul] {how} {(S, hin)}: {float((err / bnd).max()):.3f} of the bound, "
          f"{float((err / (emul.BOUND * mag)).max()):.3f} of 3 * 2^-22 alone")
    assert torch.isfinite(got).all()
    assert bool((err <= bnd).all())


def test_emulation_agrees_with_float64_on_exact_inputs():
    """small integers split exactly under any power-of-two scale: windows, slabs and the layout of the result have no
    room to hide behind a tolerance"""
    for S, hin in [(1, 7), (3, 37), (2, 82), (7, 132)]:
        gen = torch.Generator().manual_seed(hin)
        gv = torch.randint(-8, 9, (S, hout_of(hin), 16), generator=gen).float()
        xv = torch.randint(-8, 9, (S, hin, CIN), generator=gen).float()
        geo = (S, hin + 2 * HALO, hout_of(hin) + 2 * HALO, PAD)
        assert torch.equal(emul.wgrad(halo(gv), halo(xv), *geo), emul.exact_wgrad(halo(gv), halo(xv), *geo)), (S, hin)


def test_partition():
    """every unit once, at most 512 blocks, at least 16 slabs = 256 reduction rows per block unless the grid is one
    block"""
    for units in range(1, 3001):
        b = emul.partition(units)
        assert b[0] == 0 and b[-1] == units and len(b) - 1 <= emul.MAX_BLOCKS
        sizes = [q - p for p, q in zip(b[:-1], b[1:])]
        assert sum(sizes) == units and min(sizes) >= 1
        assert len(sizes) == 1 or min(sizes) * emul.R >= 256, units
    assert len(emul.partition(31)) - 1 == 1 and len(emul.partition(32)) - 1 == 2
    assert emul.partition(280)[:3] == [0, 16, 32] and len(emul.partition(280)) - 1 == 17
    assert len(emul.partition(1050)) - 1 == 65 and len(emul.partition(21376)) - 1 == 512


def test_the_running_scale_only_falls():
    """(40, 300): 280 slabs on 17 blocks.  A quiet sequence then a loud one lowers the scale; loud then quiet keeps it.
    An all-zero leading slab leaves m_run at 0 = scale 1, a NaN slab leaves the scale in force; every block starts at
    scale 1"""
    S, hin = 40, 300
    hp_in, hp = hin + 2 * HALO, hout_of(hin) + 2 * HALO
    quiet, loud = 2.0 ** -10, 2.0 ** 5
    xv = torch.ones(S, hin, CIN)
    xv[0::2], xv[1::2] = quiet, loud
    gv = torch.ones(S, hout_of(hin), COUT)
    g, x = halo(gv), halo(xv)
    g.view(S, hp, COUT)[0, :16] = 0.0                     # the first slab of block 0
    g.view(S, hp, COUT)[0, 40] = float("nan")             # its third slab
    w = emul.walk(g, x, S, hp_in, hp, PAD)
    b = w["bounds"]
    assert b[:3] == [0, 16, 32]
    assert w["sg"][:4].tolist() == [0, 14, 14, 14]        # zero slab: scale 1; the NaN slab: the scale in force
    assert w["grun"][2] == 1.0 and not torch.isfinite(w["mg"][2])
    sx = w["sx"]
    assert sx[0] == 14 + 10 and sx[5] == 14 + 10           # sequence 0 is quiet ...
    assert sx[6] == 14 - 5                                 # ... but its last slab stages the first rows of sequence 1
    assert sx[7] == 14 - 5 and sx[14] == 14 - 5            # sequence 1 is loud; sequence 2 (quiet) keeps its scale
    assert sx[16] == 14 + 10                               # block 1 starts over, inside the quiet sequence 2
    for p, q in zip(b[:-1], b[1:]):
        assert bool((sx[p + 1:q] <= sx[p:q - 1]).all())


def test_tunable_and_counter():
    from flow2gan_amd import _opts, ops
    assert "fp16x3_tapw3n_min_rows" in _opts._ASKED and "fp16x3_tapw3n_min_rows" in _opts.__doc__
    assert ops.FP16X3_TAPW3N_MIN_ROWS == ops.FP16X3_TAP_OFF
    assert isinstance(ops.FP16X3_TAPW3N_LAUNCHES, int)


def _descriptor(ops, keep, S=3, hin=300, cin=CIN, cout=COUT, taps=5):
    """the operands of ops.wgrad over ops.win1d(..., unbounded=True) for the layer, over host memory: the host checks
    never read through the pointers"""
    hp_in, hp = hin + 2 * HALO, hout_of(hin) + 2 * HALO
    g, x, out = torch.zeros(S * hp, cout), torch.zeros(S * hp_in * cin), torch.zeros(cout, taps * cin)
    keep += [g, x, out]
    d = ops.GemmDesc()
    A, B = d.A, d.B
    A.base, A.rows, A.cols, A.P1, A.P0, A.seglen, A.L1 = g.data_ptr(), S * hp, cout, 1, 1, cout, 1
    A.unit, A.L0u, A.seq_stride = 1, cout, cout
    B.base, B.rows, B.cols, B.P1, B.P0, B.seglen, B.L1 = x.data_ptr(), S * hp, taps * cin, 1, hp, taps * cin, 1
    B.step0, B.pad0, B.unit, B.L0u, B.seq_stride, B.unbounded = 3, PAD, cin, hp_in * cin, hp_in * cin, 1
    d.E.C, d.E.ldc, d.E.atomic = out.data_ptr(), taps * cin, 1
    d.form, d.split_k, d.precision = 2, 1, 4
    d.A.split = d.B.split = 8
    return d


def test_the_library_answers_for_the_layers_descriptor():
    """the built library's f2g_gemm_f16_ok (host code: nothing is launched): 1 for the layer's descriptor, 0 for
    everything the kernel declines -- and the same descriptor unmarked, or as split-6 images, keeps the answer it had"""
    from flow2gan_amd import _lib, ops
    lib = C.CDLL(_lib.LIB_PATH)
    lib.f2g_gemm_f16_ok.restype = C.c_int
    keep = []
    ok = lambda d: lib.f2g_gemm_f16_ok(C.byref(d))
    assert ok(_descriptor(ops, keep)) == 1
    spare = torch.zeros(256)

    def changed(**kw):
        d = _descriptor(ops, keep, **{k: v for k, v in kw.items() if k in ("cin", "cout", "taps")})
        for k, v in kw.items():
            if k in ("cin", "cout", "taps"):
                continue
            obj, field = k.split("_", 1)
            setattr({"A": d.A, "B": d.B, "E": d.E, "d": d}[obj], field, v)
        return d

    refusals = [dict(A_split=0), dict(B_split=0), dict(A_rscale=spare.data_ptr()), dict(B_rscale=spare.data_ptr()),
                dict(cin=64), dict(cout=256), dict(B_step0=1), dict(taps=3), dict(B_unbounded=0), dict(B_pad0=2),
                dict(E_bias=spare.data_ptr()), dict(E_scale=0.5), dict(E_atomic=0), dict(E_atomic=0, E_accumulate=1),
                dict(d_precision=0), dict(d_precision=1), dict(d_precision=2), dict(d_precision=3), dict(B_pad0=9)]
    for kw in refusals:
        assert ok(changed(**kw)) == 0, kw
    # unmarked, the 32-channel window operand is the stride-3 column-image kernel's candidate, which declines it
    assert ok(changed(A_split=0, B_split=0)) == 0
    assert ok(changed(A_split=6, B_split=6, A_rscale=spare.data_ptr(), B_rscale=spare.data_ptr())) == 0
