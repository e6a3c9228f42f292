"""fp16x3 weight gradient of the MPD's 32 -> 128 layer, scaled inside the kernel, on the GPU: gemm_h3wsn_kernel<5, 3>
(csrc/gemm_f16wsn.hip) against float64 over guarded outputs (the helpers of tests/fp16x3_gpu.py and
tests/test_hip_gemm_routes.py; the gradient sits in a NaN-poisoned buffer, the map is an unbounded operand: exactly its
buffer), the scale moves of a block's walk, the descriptors it must decline, ops.wgrad's routing, and one period of the
MPD against the CPU oracle with the layer's weight gradient on the kernel.  Cin = 32 and Cout = 128 throughout.

Tolerance per element, the family's: |got - want| <= 1.8e-6 * (|g|^T |x_win| + |what the output held|) + 2^-28 * (xmax
sum |g| + gmax sum |x_win|).  The second term is the floor of the kernel's bound (tests/fp16x3_runwin3_emul.py: an
element 2^-28 below the running maximum in force is subnormal in hi) with the operands' GLOBAL maxima in place of the
running ones: a running maximum never exceeds them, so the tolerance does not depend on the grid."""
import ctypes as C
import math

import pytest
import torch

from fp16x3_emul import FLOOR
from fp16x3_gpu import (HALO, TOL, assert_declined, f16_ok, fp16x3_mode, hout_of, maps, maps_s1, operands, operands_s1,
                        ops, ran, same_bits, subdisc_against_oracle)
from test_hip_gemm_routes import DEV, Out, last_kernel, make_desc, rnd

pytestmark = pytest.mark.gpu

NAME = "h3wsn<taps=5,step=3>"
STEP = 3
CIN, COUT = 32, 128
SHAPES = [(1, 7, 0),          # Hp = 7: one partial slab, windows overhanging both buffer ends
          (1, 34, 0),         # Hp = 16: exactly one slab, the tightest fit 3 Hout = Hin + 2
          (3, 37, 0),         # Hp = 17
          (2, 82, 0),         # Hp = 32
          (7, 131, 0),
          (7, 132, 0),        # Hin a multiple of 3
          (3, 37, 3),         # three spare zero rows behind every sequence of the map: the sequence base is s * HpIn
          (40, 300, 0),       # 280 units on 17 blocks: block ranges cut sequences
          (150, 300, 0)]      # 1050 units: more than twice any admissible grid, every block walks several units across
                              # sequence boundaries


@pytest.fixture
def fp16x3(ops):
    """the fp16x3 mode; thresholds and the mode are restored afterwards (the tests assign the thresholds themselves)"""
    names = ("FP16X3_TAPW3N_MIN_ROWS", "FP16X3_TAPW3_MIN_ROWS", "FP16X3_TAPW_MIN_ROWS", "FP16X3_TAP_MIN_ROWS",
             "FP16X3_TAP3_MIN_ROWS", "FP16X3_WGRAD_MIN_ROWS", "X6_MIN_K")
    with fp16x3_mode(ops, *names):
        yield ops


def is_h3wsn(ops):
    return ran(ops, NAME)


# ------------------------------------------------------------------ operands, launch, reference
def ops_of(ops, x, gy, **kw):
    """the fp32 operands themselves (tests/fp16x3_gpu.py: operands, without its images)"""
    return operands(ops, x, gy, images=False, **kw)


def desc8(ops, A, B, out, **kw):
    """the launch's descriptor: form 2, precision 4, atomic, both operands marked split = 8"""
    kw.setdefault("atomic", True)
    d = make_desc(ops, A, B, out, form=2, precision=4, **kw)
    d.A.split = d.B.split = 8
    return d


def launch8(ops, A, B, out):
    d = desc8(ops, A, B, out)
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    assert is_h3wsn(ops) and f16_ok(ops, d) == 1
    return d


def reference(A, B, c0):
    """float64 (want, tolerance) per element of c0 + g^T x_win"""
    a, b = A.dense(), B.dense()
    mag = a.abs().t() @ b.abs() + c0.double().abs()
    floor = FLOOR * (b.abs().max() * a.abs().sum(0)[:, None] + a.abs().max() * b.abs().sum(0)[None, :])
    return c0.double() + a.t() @ b, TOL * mag + floor


def check(got, want, tol, what):
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    err = (got - want).abs()
    bad = err > tol + 1e-30
    worst = float((err / (tol + 1e-30)).max())
    print(f"[h3wsn] {what}: worst error {worst:.3f} of the tolerance")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements off, worst {worst:.3f} of the tolerance"


def run8(ops, x, gy, seed, what):
    """one launch onto a finite non-zero guarded output against float64; returns the output"""
    A, B = ops_of(ops, x, gy)
    c0 = rnd(COUT, 5 * CIN, seed=seed)
    out = Out(COUT, 5 * CIN, c0)
    launch8(ops, A, B, out)
    out.guards_ok()
    want, tol = reference(A, B, c0)
    check(out.got(), want, tol, what)
    return out


# ------------------------------------------------------------------ kernel against float64
@pytest.mark.parametrize("S,Hin,extra", SHAPES)
def test_shapes_against_float64(ops, S, Hin, extra):
    """every case accumulates onto a finite non-zero output"""
    x, gy = maps(CIN, COUT, S, Hin, seed=S + Hin, extra=extra)
    run8(ops, x, gy, Hin, f"(S, Hin, extra) = {(S, Hin, extra)}")


def seq_scaled(S, Hin, seed, factors):
    x, gy = maps(CIN, COUT, S, Hin, seed=seed)
    f = factors.to(DEV)[:, None, None]
    return x * f, gy * f


@pytest.mark.parametrize("how", ["rising", "falling", "zero_first"])
def test_scale_moves(ops, how):
    """(40, 300): 17 blocks of 16 or 17 slabs, a sequence is 7 slabs -- every block walks two or three sequences.
    rising: every new sequence lowers both scales, the stored sums are rescaled; falling: the later sequences run under
    their block's first maxima, which is what the floor term is for; zero_first: the walk starts at m_run = 0, scale 1"""
    S, Hin = 40, 300
    mags = torch.logspace(-3, 3, S)
    if how == "falling":
        mags = mags.flip(0)
    if how == "zero_first":
        mags = torch.ones(S)
        mags[0] = 0.0
    x, gy = seq_scaled(S, Hin, 21, mags)
    run8(ops, x, gy, 22, how)


def test_all_zero_operands_leave_the_output_bits(ops):
    S, Hin = 3, 37
    x, gy = maps(CIN, COUT, S, Hin, seed=23)
    A, B = ops_of(ops, x * 0.0, gy * 0.0)
    c0 = rnd(COUT, 5 * CIN, seed=24)
    out = Out(COUT, 5 * CIN, c0)
    before = out.flat.view(torch.int32).clone()
    launch8(ops, A, B, out)
    assert torch.equal(out.flat.view(torch.int32), before)


def test_magnitudes_against_float64(ops):
    """per-element magnitudes over 2^-20..1 in both operands (no spread over the channels: one scalar scale per operand
    cannot serve 60 decades, and the bound says so)"""
    S, Hin = 3, 82
    x, gy = maps(CIN, COUT, S, Hin, seed=31)
    gen = torch.Generator().manual_seed(32)
    x *= torch.ldexp(torch.ones(x.shape), torch.randint(-20, 1, x.shape, generator=gen)).to(DEV)
    gy *= torch.ldexp(torch.ones(gy.shape), torch.randint(-20, 1, gy.shape, generator=gen)).to(DEV)
    run8(ops, x, gy, 33, "element magnitudes 2^-20..1")


def test_three_launches_give_the_same_bits(ops):
    """a single-block case: 7 sequences of Hp = 48 rows are 21 slabs, fewer than two blocks' 32, so every output element
    receives one atomic add.  (The library reports the kernel's name, not its grid.)"""
    S, Hin = 7, 131
    assert S * math.ceil((hout_of(Hin) + 2 * HALO) / 16) == 21
    x, gy = maps(CIN, COUT, S, Hin, seed=41)
    A, B = ops_of(ops, x, gy)
    c0 = rnd(COUT, 5 * CIN, seed=42)

    def go():
        out = Out(COUT, 5 * CIN, c0)
        launch8(ops, A, B, out)
        return out.flat.view(torch.int32).clone()

    same_bits(go)


def test_inf_in_one_channel_stays_in_its_output_columns(ops):
    """(tap t reads the map rows congruent to t - pad0 modulo 3 only: three consecutive rows hold the inf, so that every
    tap reads one.)  The slab that stages the inf keeps the scale in force"""
    S, Hin = 2, 82
    x, gy = maps(CIN, COUT, S, Hin, seed=51)
    chan = 17
    x0 = x.clone()
    x0[:, :, chan] = 0.0
    A0, B0 = ops_of(ops, x0, gy)                            # (the float64 reference reads finite values)
    x[1, HALO + 11:HALO + 14, chan] = float("inf")
    A, B = ops_of(ops, x, gy)
    c0 = rnd(COUT, 5 * CIN, seed=52)
    out = Out(COUT, 5 * CIN, c0)
    launch8(ops, A, B, out)
    out.guards_ok()
    got = out.got()
    tainted = torch.arange(5 * CIN, device=DEV) % CIN == chan
    assert not bool(torch.isfinite(got[:, tainted]).any()), "a finite value in an output column of the inf's channel"
    want, tol = reference(A0, B0, c0)
    check(got[:, ~tainted], want[:, ~tainted], tol[:, ~tainted], "columns beside the inf's channel")


# ------------------------------------------------------------------ refusals
DECLINED = ["only_a", "only_b", "rscale_a", "rscale_b", "unit64", "cols256", "step1", "taps3", "bounded", "overhang",
            "bias", "scale", "plain_store", "accumulate", "other_precisions"]


@pytest.mark.parametrize("what", DECLINED)
def test_descriptors_the_kernel_declines(ops, what):
    """f2g_gemm_f16_ok == 0 and F2G_EINVAL from f2g_gemm -- never another kernel; the output stays untouched"""
    Cin, Cout, S, Hin = (64 if what == "unit64" else CIN), (256 if what == "cols256" else COUT), 2, 82
    taps = 3 if what == "taps3" else 5
    if what == "overhang":      # a stride-1 geometry (P0 = HpIn = 32, pad0 = 2) with step0 flipped to 3 below
        A, B = operands_s1(ops, *maps_s1(Cin, Cout, S, 28, seed=61), images=False)
    else:
        A, B = ops_of(ops, *maps(Cin, Cout, S, Hin, seed=61), taps=taps)
    out = Out(Cout, taps * Cin)
    bias = rnd(taps * Cin, seed=62) if what == "bias" else None
    d = desc8(ops, A, B, out, atomic=what not in ("plain_store", "accumulate"), accumulate=what == "accumulate",
              bias=bias, scale=0.5 if what == "scale" else 0.0)
    scales = rnd(Cout + taps * Cin, seed=63)
    if what == "only_a":
        d.B.split = 0
    elif what == "only_b":
        d.A.split = 0
    elif what == "rscale_a":
        d.A.rscale = scales.data_ptr()
    elif what == "rscale_b":
        d.B.rscale = scales.data_ptr()
    elif what == "step1":
        d.B.step0 = 1
    elif what == "bounded":
        d.B.unbounded = 0
    elif what == "overhang":
        d.B.step0 = 3
    precisions = (0, 1, 2, 3) if what == "other_precisions" else (4,)
    for prec in precisions:
        d.precision = prec
        assert_declined(ops, d, out)
    if what == "other_precisions":      # (the descriptor itself is one the kernel runs)
        d.precision = 4
        assert f16_ok(ops, d) == 1


# ------------------------------------------------------------------ ops.wgrad
def counters(ops):
    return (ops.FP16X3_TAPW3N_LAUNCHES, ops.FP16X3_TAPW3_LAUNCHES, ops.FP16X3_TAPW_LAUNCHES, ops.FP16X3_LAUNCHES,
            ops.FP16X3_WGRAD_LAUNCHES, ops.FP16X3_TAP_LAUNCHES, ops.FP16X3_TAP3_LAUNCHES)


def test_ops_wgrad_takes_the_kernel_from_its_threshold_on(fp16x3):
    """the construction of tests/test_hip_gemm_f16_tapw3.py's routing test on the 32 -> 128 layer"""
    ops = fp16x3
    S, Hin = 7, 131
    ops.X6_MIN_K = 32
    g0 = rnd(COUT, 5 * CIN, seed=3)
    Hout = hout_of(Hin)
    Hp = Hout + 2 * HALO
    x = torch.zeros(S, Hin + 2 * HALO, CIN, device=DEV)
    x[:, HALO:HALO + Hin] = rnd(S, Hin, CIN, seed=1)
    gy = torch.zeros(S, Hp, COUT, device=DEV)
    gy[:, HALO:HALO + Hout] = rnd(S, Hout, COUT, seed=2)

    def go():
        X = ops.win1d(x, S, Hin + 2 * HALO, CIN, Hp, STEP, HALO * STEP, 5, unbounded=True)
        assert X.unbounded == 1
        out = g0.clone()
        ops.wgrad(gy.reshape(S * Hp, COUT), COUT, COUT, X, out)
        torch.cuda.synchronize()
        return out.double()

    A, B = ops_of(ops, x, gy)
    want, tol = reference(A, B, g0)
    off = ops.FP16X3_TAP_OFF
    # every fp16x3 weight-gradient route off: the kernel the parent commit launches
    ops.FP16X3_TAPW3N_MIN_ROWS = ops.FP16X3_TAPW3_MIN_ROWS = ops.FP16X3_TAPW_MIN_ROWS = off
    ops.FP16X3_WGRAD_MIN_ROWS = ops.FP16X3_WGRAD_OFF
    n0 = counters(ops)
    check(go(), want, tol, "every route off")
    before = last_kernel(ops)
    assert counters(ops) == n0 and before and not before.startswith("h3")
    # the new route from its threshold on
    ops.FP16X3_TAPW3N_MIN_ROWS = 1
    got = go()
    assert counters(ops) == (n0[0] + 1,) + n0[1:] and is_h3wsn(ops)
    check(got, want, tol, "ops.wgrad onto a previous g_out")
    # the default threshold, also with the plain, stride-1 and stride-3 column routes lowered: none may take the
    # 32-channel window operand
    n1 = counters(ops)
    ops.FP16X3_TAPW3N_MIN_ROWS = off
    check(go(), want, tol, "route off")
    assert counters(ops) == n1 and last_kernel(ops) == before
    ops.FP16X3_WGRAD_MIN_ROWS = ops.FP16X3_TAPW_MIN_ROWS = ops.FP16X3_TAPW3_MIN_ROWS = 1
    check(go(), want, tol, "route off, the column routes on")
    assert counters(ops) == n1 and last_kernel(ops) == before
    # the bf16x6 mode: the same
    ops.FP16X3_TAPW3N_MIN_ROWS = 1
    ops.set_gemm_precision("bf16x6")
    check(go(), want, tol, "bf16x6 mode")
    assert counters(ops) == n1 and last_kernel(ops) == before


# ------------------------------------------------------------------ one period of the MPD against the CPU oracle
def test_mpd_period_against_oracle(fp16x3, lib_option):
    """the construction and the tolerance of tests/test_hip_gemm_f16_tapw3.py::test_mpd_period_against_oracle (period 2)
    with all tap routes plus the new one on: the 32 -> 128 layer's weight gradient runs on gemm_h3wsn_kernel; the new
    counter stays 0 with the new tunable back at its default"""
    ops = fp16x3
    lib_option("x6p", 2)
    ops.FP16X3_TAP_MIN_ROWS = ops.FP16X3_TAP3_MIN_ROWS = ops.FP16X3_TAPW_MIN_ROWS = ops.FP16X3_TAPW3_MIN_ROWS = 1
    ops.FP16X3_TAPW3N_MIN_ROWS = 1
    r = subdisc_against_oracle(ops, "mpd", ("FP16X3_TAPW3N_LAUNCHES",),
                               "mpd period 2, fp16x3 tap routes and the three tap-walking weight gradients")
    n = r.fwd[0] + r.bwd[0]
    print(f"[h3wsn] period {r.sub.period}: {n} launches on the in-kernel-scaled stride-3 weight gradient")
    assert n >= 1, "the 32 -> 128 layer's weight gradient never reached the kernel"
    ops.FP16X3_TAPW3N_MIN_ROWS = ops.FP16X3_TAP_OFF
    assert r.rerun() == ((0,), (0,))
