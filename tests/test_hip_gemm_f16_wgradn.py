"""fp16x3 weight gradient over two plain fp32 matrices, both scaled inside the kernel, on the GPU: gemm_h3wn_kernel
(csrc/gemm_f16wn.hip) against float64 over NaN-poisoned operands (ld > cols) and guarded outputs (the helpers of
tests/test_hip_gemm_routes.py), the scale moves of a block's walk, how the result lands, the descriptors it must
decline, ops.wgrad's routing and a generator's stage-1 step against the CPU oracle with the weight gradients on the
kernel.  f2g_gemm is called by hand with both operands marked split = 10 unless a test says ops.wgrad.  The inputs are
tests/fp16x3_runk_emul.py's: tests/test_fp16x3_wgradn_host.py holds the arithmetic's bound inside the tolerance below
on every case of this file.

Tolerance per element, the form of tests/test_hip_gemm_f16_tapw3n.py: |got - want| <= TOL * (|a|^T |b| + |what the
output held| + |bias|) + 2^-28 * (bmax sum_r |a| + amax sum_r |b|), TOL = tests/test_hip_gemm_f16.py's 1.8e-6, the
maxima over the whole operands (finite values): a running maximum never exceeds them, so the tolerance does not depend
on the grid."""
import ctypes as C

import pytest
import torch

import fp16x3_runk_emul as emul
from fp16x3_emul import FLOOR
from fp16x3_gpu import TOL, assert_declined, f16_ok, fp16x3_mode, ops, ran, same_bits, stage1_against_oracle
from test_hip_gemm_routes import DEV, Out, last_kernel, make_desc, plain, rnd

pytestmark = pytest.mark.gpu

NAME = "h3wn"


@pytest.fixture
def fp16x3(ops):
    """the fp16x3 mode; thresholds and the mode are restored afterwards (the tests assign the thresholds themselves)"""
    names = ("FP16X3_WGRADN_MIN_ROWS", "FP16X3_WGRAD_MIN_ROWS", "FP16X3_MIN_K", "FP16X3_MIN_N")
    with fp16x3_mode(ops, *names):
        yield ops


def is_h3wn(ops):
    return ran(ops, NAME)


# ------------------------------------------------------------------ operands, launch, reference
def operands(ops, a, b):
    """the fp32 operands themselves inside NaN buffers, ld = cols + 4"""
    return plain(ops, a.to(DEV)), plain(ops, b.to(DEV))


def desc10(ops, A, B, out, **kw):
    """the launch's descriptor: form 2, precision 4, both operands marked split = 10"""
    d = make_desc(ops, A, B, out, form=2, precision=4, **kw)
    d.A.split = d.B.split = 10
    return d


def launch10(ops, A, B, out, **kw):
    d = desc10(ops, A, B, out, **kw)
    assert f16_ok(ops, d) == 1
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    assert is_h3wn(ops)
    return d


def reference(a, b, c0=None, bias=None, scale=1.0):
    """float64 (want, tolerance) per element of c0 + scale * a^T b + bias; a, b the finite values"""
    a, b = a.double().to(DEV), b.double().to(DEV)
    aa, ba = a.abs(), b.abs()
    want, mag = scale * (a.t() @ b), abs(scale) * (aa.t() @ ba)
    floor = abs(scale) * FLOOR * (ba.max() * aa.sum(0)[:, None] + aa.max() * ba.sum(0)[None, :])
    if bias is not None:
        want, mag = want + bias.double()[None], mag + bias.double().abs()[None]
    if c0 is not None:
        want, mag = want + c0.double(), mag + c0.double().abs()
    return want, TOL * mag + floor


def check(got, want, tol, what):
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    err = (got - want).abs()
    bad = err > tol + 1e-30
    worst = float((err / (tol + 1e-30)).max())
    print(f"[h3wn] {what}: worst error {worst:.3f} of the tolerance")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements off, worst {worst:.3f} of the tolerance"


def run10(ops, a, b, what, c0=None, **kw):
    """one launch -- a plain store onto a sentinel-guarded NaN output unless c0 is given -- against float64"""
    A, B = operands(ops, a, b)
    M, N = a.shape[1], b.shape[1]
    out = Out(M, N) if c0 is None else Out(M, N, c0)
    launch10(ops, A, B, out, **kw)
    out.guards_ok()
    want, tol = reference(a, b, c0, kw.get("bias"), kw.get("scale") or 1.0)
    check(out.got(), want, tol, what)
    return out


# ------------------------------------------------------------------ kernel against float64
@pytest.mark.parametrize("R,M,N", emul.SHAPES)
def test_shapes_against_float64(ops, R, M, N):
    """a partial slab, exactly one, an odd and an even slab count, a ragged last slab; partial tiles in both
    directions; (97, 260, 132): six tiles.  The ld padding of both operands is NaN, the output preset to a sentinel"""
    a, b = emul.inputs("normal", R, M, N)
    run10(ops, a, b, f"(R, M, N) = {(R, M, N)}")


@pytest.mark.parametrize("R,M,N", emul.MAGNITUDE_SHAPES)
@pytest.mark.parametrize("pattern", [p for p in emul.PATTERNS if not p.startswith("zero_") or p == "zero_first"])
def test_magnitude_patterns_against_float64(ops, pattern, R, M, N):
    """rising: the scales move in most slabs and the stored sums follow (a kernel that does not follow them overflows
    fp16); falling: the floor term; loud_column: a column quiet against its tile; zero_first: the walk starts at
    m_run = 0, scale 1"""
    a, b = emul.inputs(pattern, R, M, N)
    run10(ops, a, b, f"{pattern} {(R, M, N)}")


@pytest.mark.parametrize("R,M,N", emul.MAGNITUDE_SHAPES)
@pytest.mark.parametrize("pattern", ["zero_a", "zero_b"])
@pytest.mark.parametrize("how", ["store", "accumulate"])
def test_an_all_zero_operand_leaves_exact_values(ops, pattern, how, R, M, N):
    """store: exactly zero; accumulate: the preset bits"""
    a, b = emul.inputs(pattern, R, M, N)
    A, B = operands(ops, a, b)
    c0 = rnd(M, N, seed=R) if how == "accumulate" else None
    out = Out(M, N) if c0 is None else Out(M, N, c0)
    before = out.flat.view(torch.int32).clone()
    launch10(ops, A, B, out, accumulate=how == "accumulate")
    out.guards_ok()
    if how == "accumulate":
        assert torch.equal(out.flat.view(torch.int32), before)
    else:
        assert not bool(out.got().any())


# ------------------------------------------------------------------ how the result lands
@pytest.mark.parametrize("how", ["store", "accumulate", "atomic"])
def test_stores_onto_a_finite_output(ops, how):
    R, M, N = emul.MAGNITUDE_SHAPES[1]
    a, b = emul.inputs("normal", R, M, N)
    c0 = None if how == "store" else rnd(M, N, seed=5)
    kw = {} if how == "store" else {how: True}
    run10(ops, a, b, how, c0=c0, scale=0.75, **kw)


@pytest.mark.parametrize("pattern", ["normal", "rising"])
def test_atomic_split_k_with_a_ragged_last_slab(ops, pattern):
    """R = 777 in three chunks of 288 / 288 / 201 rows: every block walks its own scales, the rescaled partial tiles are
    added atomically; the bias enters once"""
    R, M, N = emul.MAGNITUDE_SHAPES[1]
    assert emul.kchunk_of(R, emul.SPLIT_K) == (288, 3)
    a, b = emul.inputs(pattern, R, M, N)
    bias = rnd(N, seed=9) * float(a.abs().max())
    run10(ops, a, b, f"split_k = 3, {pattern}", c0=rnd(M, N, seed=6), atomic=True, split_k=emul.SPLIT_K, bias=bias)


def test_three_launches_give_the_same_bits(ops):
    R, M, N = emul.MAGNITUDE_SHAPES[1]
    A, B = operands(ops, *emul.inputs("rising", R, M, N))

    def go():
        out = Out(M, N)
        launch10(ops, A, B, out)
        return out.flat.view(torch.int32).clone()

    same_bits(go)


@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_a_non_finite_input_stays_in_its_output_line(ops, side, value):
    """the slab that stages it keeps the scale in force; row m of the output (A[r, m]) or column n (B[r, n]) is not
    finite, every other element is finite and within the tolerance"""
    R, M, N = emul.MAGNITUDE_SHAPES[1]
    a, b = emul.inputs("normal", R, M, N)
    a0, b0 = a.clone(), b.clone()
    r, line = 401, 7
    if side == "A":
        a[r, line], a0[:, line] = value, 0.0
    else:
        b[r, line], b0[:, line] = value, 0.0
    A, B = operands(ops, a, b)
    out = Out(M, N)
    launch10(ops, A, B, out)
    out.guards_ok()
    got = out.got()
    want, tol = reference(a0, b0)                           # (the float64 reference reads finite values)
    if side == "A":
        keep = torch.arange(M, device=DEV) != line
        assert not bool(torch.isfinite(got[line]).any()), "a finite value in the output row of the non-finite input"
        check(got[keep], want[keep], tol[keep], f"rows beside {value}'s")
    else:
        keep = torch.arange(N, device=DEV) != line
        assert not bool(torch.isfinite(got[:, line]).any()), "a finite value in the output column of the input"
        check(got[:, keep], want[:, keep], tol[:, keep], f"columns beside {value}'s")


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("what", list(emul.refusals(0)))
def test_descriptors_the_kernel_declines(ops, what):
    """f2g_gemm_f16_ok == 0 and F2G_EINVAL from f2g_gemm -- never another kernel; the output stays untouched.
    (extent: the descriptor alone, rows that no memory stands behind -- nothing is launched)"""
    R, M, N = 160, 132, 160
    A, B = operands(ops, *emul.inputs("normal", R, M, N))
    assert A.o.seq_stride == 136 and B.o.seq_stride == 164
    out = Out(M, N)
    spare = rnd(max(M, N) * 256, seed=1)
    assert f16_ok(ops, desc10(ops, A, B, out)) == 1          # (the one change below is what it declines)
    d = emul.apply(desc10(ops, A, B, out), emul.refusals(spare.data_ptr())[what])
    assert_declined(ops, d, out)


# ------------------------------------------------------------------ ops.wgrad
def counters(ops):
    return (ops.FP16X3_WGRADN_LAUNCHES, ops.FP16X3_WGRAD_LAUNCHES, ops.FP16X3_LAUNCHES, ops.FP16X3_PLAINN_LAUNCHES)


def test_ops_wgrad_takes_the_kernel_from_its_threshold_on(fp16x3):
    ops = fp16x3
    R, M, N = 300, 132, 160
    dy, x = emul.inputs("normal", R, M, N)
    dy, x = dy.to(DEV), x.to(DEV)
    g0 = rnd(M, N, seed=3)
    want, tol = reference(dy, x, g0)
    ops.FP16X3_WGRAD_MIN_ROWS, ops.FP16X3_WGRADN_MIN_ROWS = ops.FP16X3_WGRAD_OFF, 1
    g = g0.clone()
    torch.cuda.synchronize()
    n0, mem0 = counters(ops), torch.cuda.memory_allocated()
    ops.wgrad(dy, M, M, ops.mat(x), g)
    mem1 = torch.cuda.memory_allocated()
    torch.cuda.synchronize()
    assert counters(ops) == (n0[0] + 1,) + n0[1:] and is_h3wn(ops)
    assert mem1 == mem0, "the route allocated device memory"
    check(g.double(), want, tol, "ops.wgrad onto a previous g_out")
    # above its threshold, and in the bf16x6 mode: not taken
    ops.FP16X3_WGRADN_MIN_ROWS = R + 1
    g = g0.clone()
    ops.wgrad(dy, M, M, ops.mat(x), g)
    torch.cuda.synchronize()
    assert counters(ops) == (n0[0] + 1,) + n0[1:] and last_kernel(ops) != NAME
    check(g.double(), want, tol, "below the threshold")
    ops.FP16X3_WGRADN_MIN_ROWS = 1
    ops.set_gemm_precision("bf16x6")
    ops.wgrad(dy, M, M, ops.mat(x), g0.clone())
    assert counters(ops) == (n0[0] + 1,) + n0[1:] and last_kernel(ops) != NAME


def test_ops_wgrad_runs_a_130_column_operand_as_before(fp16x3):
    """cols % 4 != 0: the library declines, the marks are cleared, the launch is the bf16x6 mode's and the counter stays"""
    ops = fp16x3
    R, M, N = 300, 130, 160
    dy, x = rnd(R, M, seed=1), rnd(R, N, seed=2, scale=R ** -0.5)
    g0 = rnd(M, N, seed=3)
    want, tol = reference(dy, x, g0)
    ops.FP16X3_WGRAD_MIN_ROWS = ops.FP16X3_WGRAD_OFF

    def go(rows):
        ops.FP16X3_WGRADN_MIN_ROWS = rows
        g = g0.clone()
        ops.wgrad(dy, M, M, ops.mat(x), g)
        torch.cuda.synchronize()
        return g, last_kernel(ops)

    n0 = counters(ops)
    off, before = go(ops.FP16X3_TAP_OFF)
    on, after = go(1)
    assert counters(ops) == n0 and after == before and not after.startswith("h3")
    assert torch.equal(on.view(torch.int32), off.view(torch.int32))
    check(on.double(), want, tol, "130 columns")


def test_the_default_is_the_bf16x6_launch_bit_for_bit(fp16x3):
    """shipped tunables in the fp16x3 mode: ops.wgrad's output equals, bit for bit, the launch of the bf16x6 mode --
    the routing with this route's code path absent -- and no fp16x3 counter moves.  (300 rows: one K chunk, so every
    output element receives one atomic add and the bits are reproducible)"""
    ops = fp16x3
    R, M, N = 300, 132, 160
    assert ops.split_for(R, 4) == 1
    assert ops.FP16X3_WGRADN_MIN_ROWS == ops.FP16X3_TAP_OFF and ops.FP16X3_WGRAD_MIN_ROWS == ops.FP16X3_WGRAD_OFF
    dy, x = rnd(R, M, seed=1), rnd(R, N, seed=2, scale=R ** -0.5)
    g0 = rnd(M, N, seed=3)

    def go():
        g = g0.clone()
        ops.wgrad(dy, M, M, ops.mat(x), g)
        torch.cuda.synchronize()
        return g.view(torch.int32), last_kernel(ops)

    n0 = counters(ops)
    got, name = go()
    assert counters(ops) == n0 and not name.startswith("h3")
    ops.set_gemm_precision("bf16x6")
    want, name6 = go()
    assert counters(ops) == n0 and name6 == name
    assert torch.equal(got, want)


# ------------------------------------------------------------------ model level, against the CPU oracle
def test_stage1_against_oracle_with_in_kernel_scaled_weight_gradients(fp16x3):
    """the construction and the tolerances of tests/test_hip_gemm_f16_wgrad.py::
    test_stage1_against_oracle_with_fp16x3_weight_gradients (the TINY config, B = 3, odd T; forward and data gradients
    on the fp16x3 kernel from K = 32 and one output column on) with this route on and the image route off"""
    ops = fp16x3
    ops.FP16X3_MIN_K, ops.FP16X3_MIN_N = 32, 1
    ops.FP16X3_WGRAD_MIN_ROWS, ops.FP16X3_WGRADN_MIN_ROWS = ops.FP16X3_WGRAD_OFF, 1
    r = stage1_against_oracle(ops, ("FP16X3_LAUNCHES", "FP16X3_WGRADN_LAUNCHES", "FP16X3_WGRAD_LAUNCHES"))
    print(f"fp16x3 launches: forward {r.fwd[0]}, data gradients {r.bwd[0]}, in-kernel-scaled weight gradients "
          f"{r.bwd[1]}")
    assert r.fwd[0] > 0 and r.bwd[0] > 0, "forward or data gradients never reached the fp16x3 kernel"
    assert r.bwd[1] > 0, "the backward pass never reached gemm_h3wn_kernel"
    assert r.bwd[2] == 0, "the image route took a weight gradient"
