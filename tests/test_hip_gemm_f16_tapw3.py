"""fp16x3 tap-walking weight gradient of the stride-3 layers on the GPU: gemm_h3ws_kernel<5, 3> against float64 over
guarded outputs (the helpers of tests/test_hip_gemm_routes.py; the gradient sits in a NaN-poisoned buffer, the map is an
unbounded operand: exactly its buffer), the descriptors it must decline, ops.wgrad's routing, and one period of the MPD
against the CPU oracle with forward and weight gradient of both stride-3 layers in the fp16x3 arithmetic.

Geometry of a layer conv(k = 5, stride = 3, padding = 2), Hout = (Hin - 1) // 3 + 1: the gradient map has Hp = Hout + 4
rows per sequence, the input map HpIn = Hin + 4 (+ spare rows), both with zero halo rows; step0 = 3, pad0 = 6.

Tolerance of the GEMM cases: tests/test_hip_gemm_f16.py's, |got - want| <= 1.8e-6 * (|g|^T |x_win| + |what the output
held|) per element: tap and stride only select rows of the map, so a power-of-two scale per column of the whole map
leaves the sum over rows exactly (tests/fp16x3_colswin3_emul.py) and the per-product bound is 3 * 2^-22, beside the
suite's 1e-6 for exact-class fp32 accumulation.  The kernel's slab is 16 gradient rows: the slab-edge shapes are Hp =
7, 16, 17, 32."""
import pytest
import torch

import fp16x3_colswin3_emul as win3_emul
from fp16x3_gpu import (HALO, TOL, assert_declined, f16_ok, fp16x3_mode, hout_of, maps, maps_s1, operands, operands_s1,
                        ops, ran, same_bits, subdisc_against_oracle)
from test_hip_gemm_routes import DEV, Out, check, last_kernel, launch, make_desc, products, rnd, run

pytestmark = pytest.mark.gpu

NAME = "h3ws<taps=5,step=3>"
STEP = 3
SHAPES = [(128, 128, 1, 7, 0),        # Hp = 7: one partial slab, windows overhanging both buffer ends
          (128, 128, 1, 34, 0),       # Hp = 16: exactly one slab, the tightest fit 3 Hout = Hin + 2
          (128, 128, 3, 37, 0),       # Hp = 17
          (128, 128, 2, 82, 0),       # Hp = 32
          (256, 256, 7, 131, 0),      # tiles beyond the first, several sequences in one block
          (256, 256, 7, 132, 0),      # Hin a multiple of 3
          (128, 256, 40, 300, 0),     # 4160 reduction rows: several sequence chunks, rescale before the atomic add
          (512, 1024, 2, 81, 0),      # the 512 -> 1024 layer at period 11: Hp = 31
          (128, 128, 3, 37, 3)]       # three spare zero rows behind every sequence of the map: the sequence base is
                                      # s * HpIn, not 3 * Hp


@pytest.fixture
def fp16x3(ops):
    """the fp16x3 mode; thresholds and the mode are restored afterwards (the tests assign the thresholds themselves)"""
    names = ("FP16X3_TAPW3_MIN_ROWS", "FP16X3_TAPW_MIN_ROWS", "FP16X3_TAP_MIN_ROWS", "FP16X3_TAP3_MIN_ROWS",
             "FP16X3_WGRAD_MIN_ROWS", "X6_MIN_K")
    with fp16x3_mode(ops, *names):
        yield ops


def is_h3ws(ops):
    return ran(ops, NAME)


# ------------------------------------------------------------------ kernel against float64
@pytest.mark.parametrize("Cin,Cout,S,Hin,extra", SHAPES)
def test_stride3_tap_wgrad_shapes_against_float64(ops, Cin, Cout, S, Hin, extra):
    """every case accumulates onto a finite non-zero output"""
    x, gy = maps(Cin, Cout, S, Hin, seed=S + Hin, extra=extra)
    A, B = operands(ops, x, gy)
    d, out = run(ops, A, B, Cout, 5 * Cin, form=2, precision=4, tol=TOL, seed=Hin, epi=dict(atomic=True))
    assert is_h3ws(ops) and f16_ok(ops, d) == 1


def test_stride3_tap_wgrad_magnitudes_against_float64(ops):
    """per-element magnitudes over 2^-20..1 in both operands, the map's channels over 60 decades: one scale per
    channel of the map, the two reciprocals applied one after the other"""
    Cin, Cout, S, Hin = 128, 128, 3, 82
    x, gy = maps(Cin, Cout, S, Hin, seed=31)
    gen = torch.Generator().manual_seed(32)
    x *= torch.ldexp(torch.ones(x.shape), torch.randint(-20, 1, x.shape, generator=gen)).to(DEV)
    gy *= torch.ldexp(torch.ones(gy.shape), torch.randint(-20, 1, gy.shape, generator=gen)).to(DEV)
    x *= torch.logspace(-30, 30, Cin, device=DEV)[None, None, :]
    A, B = operands(ops, x, gy)
    d, out = run(ops, A, B, Cout, 5 * Cin, form=2, precision=4, tol=TOL, seed=33, epi=dict(atomic=True))
    assert is_h3ws(ops) and f16_ok(ops, d) == 1


def test_three_launches_give_the_same_bits(ops):
    """a single-chunk case: 7 sequences of Hp = 48 rows are 336 reduction rows, and the launcher cuts sequence chunks
    only while each keeps at least 256 rows (two chunks would have 192 and 144), so the grid's z is 1 and every output
    element receives one atomic add.  (The library reports the kernel's name, not its grid.)"""
    Cin, Cout, S, Hin, _ = SHAPES[4]
    assert S * (hout_of(Hin) + 2 * HALO) == 336
    x, gy = maps(Cin, Cout, S, Hin, seed=41)
    A, B = operands(ops, x, gy)
    c0 = rnd(Cout, 5 * Cin, seed=42)

    def go():
        out = Out(Cout, 5 * Cin, c0)
        launch(ops, A, B, out, form=2, precision=4, atomic=True)
        assert is_h3ws(ops)
        return out.flat.view(torch.int32).clone()

    same_bits(go)


def test_inf_in_one_channel_stays_in_its_output_columns(ops):
    """(tap t reads the map rows congruent to t - pad0 modulo 3 only: three consecutive rows hold the inf, so that every
    tap reads one)"""
    Cin, Cout, S, Hin = 128, 128, 2, 82
    x, gy = maps(Cin, Cout, S, Hin, seed=51)
    chan = 37
    x0 = x.clone()
    x0[:, :, chan] = 0.0
    A0, B0 = operands(ops, x0, gy, images=False)            # (the float64 reference reads finite values)
    x[1, HALO + 11:HALO + 14, chan] = float("inf")
    A, B = operands(ops, x, gy)
    c0 = rnd(Cout, 5 * Cin, seed=52)
    out = Out(Cout, 5 * Cin, c0)
    launch(ops, A, B, out, form=2, precision=4, atomic=True)
    assert is_h3ws(ops)
    out.guards_ok()
    got = out.got()
    cols = torch.arange(5 * Cin, device=DEV)
    tainted = cols % Cin == chan
    assert not bool(torch.isfinite(got[:, tainted]).any()), "a finite value in an output column of the inf's channel"
    want, mag = products(A0, B0, 2, False)
    want, mag = want + c0.double(), mag + c0.double().abs()
    check(got[:, ~tainted], want[:, ~tainted], mag[:, ~tainted], TOL, "columns beside the inf's channel")


# ------------------------------------------------------------------ refusals
DECLINED = ["bounded", "unit32", "step2", "taps3", "overhang", "no_scales_a", "no_scales_b", "split5_a", "split7_a",
            "split5_b", "split7_b", "bias", "scale", "plain_store", "accumulate", "other_precisions"]


@pytest.mark.parametrize("what", DECLINED)
def test_descriptors_the_kernel_declines(ops, what):
    """f2g_gemm_f16_ok == 0 and F2G_EINVAL from f2g_gemm -- never another kernel; the output stays untouched"""
    Cin, Cout, S, Hin = (32 if what == "unit32" else 128), 128, 2, 82
    taps = 3 if what == "taps3" else 5
    if what == "overhang":      # a stride-1 geometry (P0 = HpIn = 32, pad0 = 2) with step0 flipped to 3 below
        A, B = operands_s1(ops, *maps_s1(Cin, Cout, S, 28, seed=61))
    else:
        A, B = operands(ops, *maps(Cin, Cout, S, Hin, seed=61), taps=taps)
    out = Out(Cout, taps * Cin)
    bias = rnd(taps * Cin, seed=62) if what == "bias" else None
    d = make_desc(ops, A, B, out, form=2, precision=4, atomic=what not in ("plain_store", "accumulate"),
                  accumulate=what == "accumulate", bias=bias, scale=0.5 if what == "scale" else 0.0)
    if what == "bounded":
        d.B.unbounded = 0
    elif what == "step2":
        d.B.step0 = 2
    elif what == "overhang":
        assert f16_ok(ops, d) == 1      # (the stride-1 kernel's descriptor)
        d.B.step0 = 3
    elif what == "no_scales_a":
        d.A.rscale = None
    elif what == "no_scales_b":
        d.B.rscale = None
    elif what.startswith("split"):
        setattr(d.A if what.endswith("_a") else d.B, "split", int(what[5]))
    precisions = (0, 1, 2, 3) if what == "other_precisions" else (4,)
    for prec in precisions:
        d.precision = prec
        assert_declined(ops, d, out)
    if what == "other_precisions":      # (the descriptor itself is one the kernel runs)
        d.precision = 4
        assert f16_ok(ops, d) == 1


def test_fp32_operands_would_qualify_but_are_not_launched(ops):
    A, B = operands(ops, *maps(128, 128, 2, 82, seed=71), images=False)
    out = Out(128, 5 * 128)
    d = make_desc(ops, A, B, out, form=2, precision=4, atomic=True)
    assert_declined(ops, d, out, ok=2)


# ------------------------------------------------------------------ ops.wgrad
def counters(ops):
    return (ops.FP16X3_TAPW3_LAUNCHES, ops.FP16X3_TAPW_LAUNCHES, ops.FP16X3_LAUNCHES, ops.FP16X3_WGRAD_LAUNCHES,
            ops.FP16X3_TAP_LAUNCHES, ops.FP16X3_TAP3_LAUNCHES)


@pytest.mark.parametrize("S,Hin", [(7, 131), (40, 300)])
def test_ops_wgrad_takes_the_kernel_from_its_threshold_on(fp16x3, S, Hin):
    """the construction of tests/test_hip_ops.py::test_wgrad_unbounded_windows"""
    ops = fp16x3
    Cin, Cout = 128, 256
    ops.X6_MIN_K = 32
    g0 = rnd(Cout, 5 * Cin, seed=3)

    def go(stv):
        Hout = (Hin + 4 - 5) // stv + 1
        Hp = Hout + 2 * HALO
        x = torch.zeros(S, Hin + 2 * HALO, Cin, device=DEV)
        x[:, HALO:HALO + Hin] = rnd(S, Hin, Cin, seed=1)
        gy = torch.zeros(S, Hp, Cout, device=DEV)
        gy[:, HALO:HALO + Hout] = rnd(S, Hout, Cout, seed=2)
        X = ops.win1d(x, S, Hin + 2 * HALO, Cin, Hp, stv, HALO * stv, 5, unbounded=True)
        assert X.unbounded == 1
        out = g0.clone()
        ops.wgrad(gy.reshape(S * Hp, Cout), Cout, Cout, X, out)
        torch.cuda.synchronize()
        return x, gy, out

    ops.FP16X3_TAPW3_MIN_ROWS = 1
    n0 = counters(ops)
    x, gy, out = go(3)
    assert counters(ops) == (n0[0] + 1,) + n0[1:] and is_h3ws(ops)
    Hp = gy.shape[1]
    xw = win3_emul.windows3(x.reshape(-1, Cin).double().cpu(), S, Hin + 2 * HALO, Hp, HALO * STEP).to(DEV)
    g2 = gy.reshape(-1, Cout).double()
    want, mag = g0.double() + g2.t() @ xw, g0.double().abs() + g2.abs().t() @ xw.abs()
    check(out.double(), want, mag, TOL, "ops.wgrad onto a previous g_out")
    # a stride-1 call never raises the new counter (it stays with the bf16x6 kernel: its own route is off)
    n1 = counters(ops)
    go(1)
    assert counters(ops) == n1 and last_kernel(ops) == "leanw6t<step=1>"
    # the default threshold -- also with the plain and the stride-1 weight-gradient routes lowered: neither may take a
    # stride-3 window operand -- and the bf16x6 mode: the bf16x6 kernel as before
    ops.FP16X3_TAPW3_MIN_ROWS = ops.FP16X3_TAP_OFF
    _, _, out = go(3)
    assert counters(ops) == n1 and last_kernel(ops) == "leanw6s<step=3>"
    check(out.double(), want, mag, TOL, "route off")
    ops.FP16X3_WGRAD_MIN_ROWS = ops.FP16X3_TAPW_MIN_ROWS = 1
    go(3)
    assert counters(ops) == n1 and last_kernel(ops) == "leanw6s<step=3>"
    ops.FP16X3_TAPW3_MIN_ROWS = 1
    ops.set_gemm_precision("bf16x6")
    go(3)
    assert counters(ops) == n1 and last_kernel(ops) == "leanw6s<step=3>"


# ------------------------------------------------------------------ one period of the MPD against the CPU oracle
def test_mpd_period_against_oracle(fp16x3, lib_option):
    """the construction of tests/test_hip_gemm_f16_tapw.py::test_mpd_period_against_oracle (period 2, that file's
    tolerance) with all four tap routes on: forward and weight gradient of the 128 -> 512 and 512 -> 1024 layers run in
    the fp16x3 arithmetic; the new counter stays 0 with the new tunable back at its default"""
    ops = fp16x3
    lib_option("x6p", 2)
    ops.FP16X3_TAP_MIN_ROWS = ops.FP16X3_TAP3_MIN_ROWS = ops.FP16X3_TAPW_MIN_ROWS = ops.FP16X3_TAPW3_MIN_ROWS = 1
    r = subdisc_against_oracle(ops, "mpd", ("FP16X3_TAPW3_LAUNCHES",),
                               "mpd period 2, fp16x3 tap routes and both tap-walking weight gradients")
    tapw3 = r.fwd[0] + r.bwd[0]
    print(f"[h3ws] period {r.sub.period}: {tapw3} launches on the stride-3 tap-walking weight gradient")
    assert tapw3 >= 2, "a stride-3 layer's weight gradient never reached the kernel"
    ops.FP16X3_TAPW3_MIN_ROWS = ops.FP16X3_TAP_OFF
    assert r.rerun() == ((0,), (0,))
