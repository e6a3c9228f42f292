"""fp16x3 tap-walking weight gradient on the GPU: gemm_h3wt_kernel<5> against float64 over guarded outputs (the helpers
of tests/test_hip_gemm_routes.py; the gradient sits in a NaN-poisoned buffer, the map is an unbounded operand: exactly
its buffer), the descriptors it must decline, ops.wgrad's routing, and one period of the MPD against the CPU oracle
with the fifth layer's forward, data gradient and weight gradient all in the fp16x3 arithmetic.

Tolerance of the GEMM cases: tests/test_hip_gemm_f16.py's, |got - want| <= 1.8e-6 * (|g|^T |x_win| + |what the output
held|) per element: the taps shift rows of the map, so a power-of-two scale per column of the whole map leaves every
tap's sum over rows exactly (tests/fp16x3_colswin_emul.py) and the per-product bound is 3 * 2^-22, beside the suite's
1e-6 for exact-class fp32 accumulation."""
import pytest
import torch

import fp16x3_colswin_emul as win_emul
from fp16x3_gpu import HALO, TOL, assert_declined, f16_ok, fp16x3_mode, ops, ran, same_bits, subdisc_against_oracle
from fp16x3_gpu import maps_s1 as maps
from fp16x3_gpu import operands_s1 as operands
from test_hip_gemm_routes import DEV, Out, _halo_x, check, last_kernel, launch, make_desc, products, rnd, run

pytestmark = pytest.mark.gpu

NAME = "h3wt<taps=5>"
SHAPES = [(128, 128, 1, 3),        # K = 7: one partial slab, windows overhang both buffer ends
          (128, 128, 1, 28),       # K = 32: exactly one slab
          (128, 128, 3, 7),        # K = 33
          (128, 128, 2, 28),       # K = 64: an even slab count
          (256, 256, 7, 131),      # ci and co tiles beyond the first, slabs straddling sequence ends
          (128, 256, 40, 300)]     # K = 12160: the launcher's several K chunks, rescale before the atomic add


@pytest.fixture
def fp16x3(ops):
    """the fp16x3 mode; thresholds and the mode are restored afterwards (the tests assign the thresholds themselves)"""
    names = ("FP16X3_TAPW_MIN_ROWS", "FP16X3_TAP_MIN_ROWS", "FP16X3_WGRAD_MIN_ROWS", "X6_MIN_K")
    with fp16x3_mode(ops, *names):
        yield ops


def is_h3wt(ops):
    return ran(ops, NAME)


# ------------------------------------------------------------------ kernel against float64
@pytest.mark.parametrize("Cin,Cout,S,Hin", SHAPES)
def test_tap_wgrad_shapes_against_float64(ops, Cin, Cout, S, Hin):
    """every case accumulates onto a finite non-zero output"""
    x, gy = maps(Cin, Cout, S, Hin, seed=S + Hin)
    A, B = operands(ops, x, gy)
    d, out = run(ops, A, B, Cout, 5 * Cin, form=2, precision=4, tol=TOL, seed=Hin, epi=dict(atomic=True))
    assert is_h3wt(ops) and f16_ok(ops, d) == 1


def test_tap_wgrad_magnitudes_against_float64(ops):
    """per-element magnitudes over 2^-20..1 in both operands, the map's channels over 60 decades: one scale per
    channel of the map, the two reciprocals applied one after the other"""
    Cin, Cout, S, Hin = 128, 128, 3, 28
    x, gy = maps(Cin, Cout, S, Hin, seed=31)
    gen = torch.Generator().manual_seed(32)
    x *= torch.ldexp(torch.ones(x.shape), torch.randint(-20, 1, x.shape, generator=gen)).to(DEV)
    gy *= torch.ldexp(torch.ones(gy.shape), torch.randint(-20, 1, gy.shape, generator=gen)).to(DEV)
    x *= torch.logspace(-30, 30, Cin, device=DEV)[None, None, :]
    A, B = operands(ops, x, gy)
    d, out = run(ops, A, B, Cout, 5 * Cin, form=2, precision=4, tol=TOL, seed=33, epi=dict(atomic=True))
    assert is_h3wt(ops) and f16_ok(ops, d) == 1


def test_three_launches_give_the_same_bits(ops):
    """a single-chunk case (K = 945 < 1024 rows: every output element receives one atomic add)"""
    Cin, Cout, S, Hin = SHAPES[4]
    x, gy = maps(Cin, Cout, S, Hin, seed=41)
    A, B = operands(ops, x, gy)
    c0 = rnd(Cout, 5 * Cin, seed=42)

    def go():
        out = Out(Cout, 5 * Cin, c0)
        launch(ops, A, B, out, form=2, precision=4, atomic=True)
        assert is_h3wt(ops)
        return out.flat.view(torch.int32).clone()

    same_bits(go)


def test_inf_in_one_channel_stays_in_its_output_columns(ops):
    Cin, Cout, S, Hin = 128, 128, 2, 28
    x, gy = maps(Cin, Cout, S, Hin, seed=51)
    chan = 37
    x0 = x.clone()
    x0[:, :, chan] = 0.0
    A0, B0 = operands(ops, x0, gy, images=False)            # (the float64 reference reads finite values)
    x[1, HALO + 11, chan] = float("inf")
    A, B = operands(ops, x, gy)
    c0 = rnd(Cout, 5 * Cin, seed=52)
    out = Out(Cout, 5 * Cin, c0)
    launch(ops, A, B, out, form=2, precision=4, atomic=True)
    assert is_h3wt(ops)
    out.guards_ok()
    got = out.got()
    cols = torch.arange(5 * Cin, device=DEV)
    tainted = cols % Cin == chan
    assert not bool(torch.isfinite(got[:, tainted]).any()), "a finite value in an output column of the inf's channel"
    want, mag = products(A0, B0, 2, False)
    want, mag = want + c0.double(), mag + c0.double().abs()
    check(got[:, ~tainted], want[:, ~tainted], mag[:, ~tainted], TOL, "columns beside the inf's channel")


# ------------------------------------------------------------------ refusals
DECLINED = ["bounded", "unit32", "step3", "taps3", "no_scales_a", "no_scales_b", "split5_a", "split7_a", "split5_b",
            "split7_b", "bias", "scale", "plain_store", "accumulate", "other_precisions"]


@pytest.mark.parametrize("what", DECLINED)
def test_descriptors_the_kernel_declines(ops, what):
    """f2g_gemm_f16_ok == 0 and F2G_EINVAL from f2g_gemm -- never another kernel; the output stays untouched"""
    Cin, Cout, S, Hin = (32 if what == "unit32" else 128), 128, 2, 28
    taps = 3 if what == "taps3" else 5
    x, gy = maps(Cin, Cout, S, Hin, seed=61)
    A, B = operands(ops, x, gy, taps=taps)
    out = Out(Cout, taps * Cin)
    bias = rnd(taps * Cin, seed=62) if what == "bias" else None
    d = make_desc(ops, A, B, out, form=2, precision=4, atomic=what not in ("plain_store", "accumulate"),
                  accumulate=what == "accumulate", bias=bias, scale=0.5 if what == "scale" else 0.0)
    if what == "bounded":
        d.B.unbounded = 0
    elif what == "step3":
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
    x, gy = maps(128, 128, 2, 28, seed=71)
    A, B = operands(ops, x, gy, images=False)
    out = Out(128, 5 * 128)
    d = make_desc(ops, A, B, out, form=2, precision=4, atomic=True)
    assert_declined(ops, d, out, ok=2)


# ------------------------------------------------------------------ ops.wgrad
def counters(ops):
    return ops.FP16X3_TAPW_LAUNCHES, ops.FP16X3_LAUNCHES, ops.FP16X3_WGRAD_LAUNCHES, ops.FP16X3_TAP_LAUNCHES


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
        x = _halo_x(S, Hin, Cin, HALO, 1)
        gy = torch.zeros(S, Hp, Cout, device=DEV)
        gy[:, HALO:HALO + Hout] = rnd(S, Hout, Cout, seed=2)
        X = ops.win1d(x, S, Hin + 2 * HALO, Cin, Hp, stv, HALO * stv, 5, unbounded=True)
        assert X.unbounded == 1
        out = g0.clone()
        ops.wgrad(gy.reshape(S * Hp, Cout), Cout, Cout, X, out)
        torch.cuda.synchronize()
        return x, gy, out

    ops.FP16X3_TAPW_MIN_ROWS = 1
    n0 = counters(ops)
    x, gy, out = go(1)
    assert counters(ops) == (n0[0] + 1,) + n0[1:] and is_h3wt(ops)
    # (the gradient map's halo rows are zero, so reading past a sequence's ends adds nothing: plain row shifts)
    xw = win_emul.windows(x.reshape(-1, Cin).double(), HALO)
    g2 = gy.reshape(-1, Cout).double()
    want, mag = g0.double() + g2.t() @ xw, g0.double().abs() + g2.abs().t() @ xw.abs()
    check(out.double(), want, mag, TOL, "ops.wgrad onto a previous g_out")
    # the default threshold (also with the plain weight-gradient route lowered: it must not take a window operand),
    # a stride-3 layer, and the bf16x6 mode: the bf16x6 kernels as before
    n1 = counters(ops)
    ops.FP16X3_TAPW_MIN_ROWS, ops.FP16X3_WGRAD_MIN_ROWS = ops.FP16X3_TAP_OFF, 1
    _, _, out = go(1)
    assert counters(ops) == n1 and last_kernel(ops) == "leanw6t<step=1>"
    check(out.double(), want, mag, TOL, "route off")
    ops.FP16X3_TAPW_MIN_ROWS = 1
    go(3)
    assert counters(ops) == n1 and last_kernel(ops) == "leanw6s<step=3>"
    ops.set_gemm_precision("bf16x6")
    go(1)
    assert counters(ops) == n1 and last_kernel(ops) == "leanw6t<step=1>"


# ------------------------------------------------------------------ one period of the MPD against the CPU oracle
def test_mpd_period_against_oracle(fp16x3, lib_option):
    """the construction of tests/test_hip_gemm_f16_tap.py::test_mpd_period_against_oracle (period 2, that file's
    tolerance) with the tap route and the tap-walking weight gradient both on: the fifth layer's forward, data gradient
    and weight gradient all run in the fp16x3 arithmetic; the counter stays 0 with the route off"""
    ops = fp16x3
    lib_option("x6p", 2)
    ops.FP16X3_TAP_MIN_ROWS = ops.FP16X3_TAPW_MIN_ROWS = 1
    r = subdisc_against_oracle(ops, "mpd", ("FP16X3_TAP_LAUNCHES", "FP16X3_TAPW_LAUNCHES"),
                               "mpd period 2, fp16x3 tap route and tap-walking weight gradient")
    tap, tapw = (f + b for f, b in zip(r.fwd, r.bwd))
    print(f"[h3wt] period {r.sub.period}: {tap} launches on the tap route, {tapw} on the tap-walking weight gradient")
    assert tap >= 2, "the fifth layer's forward and data gradient never reached the tap route"
    assert tapw >= 1, "the fifth layer's weight gradient never reached the kernel"
    ops.FP16X3_TAPW_MIN_ROWS = ops.FP16X3_TAP_OFF
    tap, tapw = (f + b for f, b in zip(*r.rerun()))
    assert tap >= 2 and tapw == 0
