"""fp16x3 on the GPU: the split kernel bit for bit against its emulation (tests/fp16x3_emul.py), gemm_h3_kernel
against float64 over poisoned operands and guarded outputs (the helpers of tests/test_hip_gemm_routes.py), the
descriptors it must decline, a generator's stage-1 step and inference against the CPU oracle, and the weight images
of the derived-weight cache following their weights.

Tolerance of the GEMM cases: |got - want| <= 1.8e-6 * (|A| |B|^T + |epilogue terms|) per element = the suite's 1e-6
for exact-class fp32 accumulation plus the arithmetic's 3 * 2^-22 = 7.2e-7 per product."""
import ctypes as C

import pytest
import torch

import fp16x3_emul as emul
from fp16x3_gpu import (EINVAL, TOL, as_image, assert_declined, cached_image, f16_ok, fp16x3_mode, image_follows_weight,
                        ops, ran, same_bits, stage1_against_oracle)
from fp16x3_gpu import mode_name    # noqa: F401 -- tools/fp16x3_*_shapes.py read the mode's name from this module
from test_hip_gemm_routes import (DEV, EPI, NAN, SENT, Out, Vec, check, expect, last_kernel, launch, make_desc,
                                  plain, products, rnd, run, win1)

pytestmark = pytest.mark.gpu

NAME = "h3<ep=all>"


@pytest.fixture
def fp16x3(ops):
    """the mode with the kernel reachable from K = 32 and one output column on"""
    with fp16x3_mode(ops, "FP16X3_MIN_K", "FP16X3_MIN_N"):
        ops.FP16X3_MIN_K, ops.FP16X3_MIN_N = 32, 1
        yield ops


# ------------------------------------------------------------------ split kernel
def special_rows(rows, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g)
    spread = torch.ldexp(torch.ones(rows, K), torch.randint(-20, 1, (rows, K), generator=g))
    if rows == 2:                       # the long rows: per-element 2^-20 ... 1, and a row of huge values
        x[0] *= spread[0]
        x[1] *= 1e30
        return x
    x[0] = 0.0                          # all zero
    x[1] = 0.0
    x[1, K // 2 + 1] = -3.7e-3          # a single non-zero element
    x[2] = x[2].clamp(-1.9, 1.9)
    x[2, 5] = 2.0                       # amax exactly a power of two
    x[3] *= spread[3] * 1e-30           # tiny, with the per-element exponent range
    x[4] *= 1e30                        # huge
    if rows > 5:
        x[5:] *= spread[5:]
        x[7] = -x[7].abs().clamp(max=0.99)
        x[7, 0] = -1.0                  # a NEGATIVE power-of-two amax
        x[8] *= 2.0 ** -130             # subnormal floats: the clamped scale
    return x


@pytest.mark.parametrize("rows,K,ld", [(5, 32, 32), (33, 160, 176), (2, 2304, 2304)])
def test_split_is_bit_identical_to_the_emulation(ops, rows, K, ld):
    x = special_rows(rows, K, 7 * rows + K)
    pre, tail = 8, 3 * ld + 5
    src = torch.full((pre + rows * ld + tail,), NAN)
    src[pre:pre + rows * ld].view(rows, ld)[:, :K] = x
    src = src.to(DEV)
    dst = torch.full_like(src, SENT)
    rs = torch.full((rows + 8,), SENT, device=DEV)
    ops.call("f2g_split_f16x2", dst.data_ptr() + 4 * pre, rs.data_ptr() + 16, src.data_ptr() + 4 * pre, ld, rows, K)
    torch.cuda.synchronize()
    want_img, want_rs = emul.image(x)
    got = dst.cpu()
    body = got[pre:pre + rows * ld].view(rows, ld)
    assert torch.equal(body[:, :K].contiguous().view(torch.int32), want_img), \
        f"{int((body[:, :K].contiguous().view(torch.int32) != want_img).sum())} words differ"
    assert torch.equal(rs.cpu()[4:4 + rows].view(torch.int32), want_rs.view(torch.int32))
    # nothing else was written: the ld padding, the floats before the first and after the last row, the scales' guards
    assert bool((body[:, K:] == SENT).all()) and bool((got[:pre] == SENT).all())
    assert bool((got[pre + rows * ld:] == SENT).all())
    assert bool((rs.cpu()[:4] == SENT).all()) and bool((rs.cpu()[4 + rows:] == SENT).all())
    # in place (dst = src) gives the same image
    ops.call("f2g_split_f16x2", src.data_ptr() + 4 * pre, rs.data_ptr() + 16, src.data_ptr() + 4 * pre, ld, rows, K)
    torch.cuda.synchronize()
    inplace = src.cpu()[pre:pre + rows * ld].view(rows, ld)[:, :K].contiguous().view(torch.int32)
    assert torch.equal(inplace, want_img)


def test_split_declines_what_it_cannot_keep_in_registers(ops):
    buf = torch.zeros(2 * 8192, device=DEV)
    rs = torch.zeros(8, device=DEV)
    lib, st = ops.L.lib, ops.L.stream_ptr()
    for ld, rows, K in ((8192, 2, 4128), (48, 2, 48), (28, 2, 32), (34, 2, 32)):
        assert lib.f2g_split_f16x2(buf.data_ptr(), rs.data_ptr(), buf.data_ptr(), ld, rows, K, st) == EINVAL
    assert lib.f2g_split_f16x2(buf.data_ptr() + 4, rs.data_ptr(), buf.data_ptr(), 32, 2, 32, st) == EINVAL
    assert lib.f2g_split_f16x2(buf.data_ptr(), rs.data_ptr(), buf.data_ptr(), 4096, 2, 4096, st) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ GEMM against float64
def operands(ops, M, N, K, seed, scale_a=1.0):
    A = as_image(ops, plain(ops, rnd(M, K, seed=seed, scale=scale_a)))
    B = as_image(ops, plain(ops, rnd(N, K, seed=seed + 50, scale=K ** -0.5)))
    return A, B


@pytest.mark.parametrize("K", [32, 64, 160, 2304])
@pytest.mark.parametrize("N", [32, 96, 128, 160])
@pytest.mark.parametrize("M", [1, 127, 128, 129, 300])
def test_gemm_shapes_against_float64(ops, M, N, K):
    """one slab, an even and an odd slab count, a long reduction; partial tiles in both directions, a single row"""
    A, B = operands(ops, M, N, K, seed=M + 3 * N + K)
    d, out = run(ops, A, B, M, N, epi=dict(bias=True), precision=4, tol=TOL, seed=K)
    assert ran(ops, NAME)
    assert f16_ok(ops, d) == 1


@pytest.mark.parametrize("ep", sorted(EPI) + ["atomic"])
def test_gemm_epilogues_against_float64(ops, ep):
    """bias + residual * gamma + leaky ReLU; PReLU backward with both column sums; row-mapped store; scaled,
    accumulating store; atomic accumulation"""
    M, N, K = 129, 160, 160
    A, B = operands(ops, M, N, K, seed=11)
    epi = dict(bias=True, atomic=True) if ep == "atomic" else EPI[ep]
    run(ops, A, B, M, N, epi=epi, precision=4, tol=TOL, seed=23)
    assert last_kernel(ops) == NAME


@pytest.mark.parametrize("two", [False, True])
def test_gemm_fused_prelu_against_float64(ops, two):
    """PReLU of the result: into C, or -- with prelu_out -- C keeps the pre-activation"""
    M, N, K = 129, 160, 160
    A, B = operands(ops, M, N, K, seed=12)
    bias, slope = rnd(N, seed=1), 0.25 + 0.1 * rnd(N, seed=2)
    out, pout = Out(M, N), Out(M, N)
    d = make_desc(ops, A, B, out, precision=4, bias=bias)
    d.E.prelu_slope = slope.data_ptr()
    if two:
        d.E.prelu_out, d.E.ld_prelu_out = pout.flat.data_ptr() + 4 * pout.base, pout.ldc
    assert f16_ok(ops, d) == 1
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    assert last_kernel(ops) == NAME
    out.guards_ok()
    pout.guards_ok()
    acc, mag = products(A, B, 0, False)
    v, m, _, _ = expect(acc, mag, bias=bias)
    p = torch.where(v > 0, v, slope.double()[None] * v)
    if two:
        check(out.got(), v, m, TOL, "pre-activation")
        check(pout.got(), p, m, TOL, "activation")
    else:
        check(out.got(), p, m, TOL, "activation")


@pytest.mark.parametrize("fm", [False, True])
def test_gemm_mask_epilogue_against_float64(ops, fm):
    """leaky-ReLU backward of the layer below (+ feature-matching term) with the column sums of the result"""
    M, N, K = 129, 160, 160
    A, B = operands(ops, M, N, K, seed=13)
    out = Out(M, N)
    y = rnd(M, out.ldc, seed=3)
    ref = rnd(M, out.ldc, seed=4)
    wdev = torch.tensor([0.5], device=DEV)
    cs = Vec(N, 5)
    d = make_desc(ops, A, B, out, precision=4, colsum=cs)
    d.E.mask_src, d.E.mask_slope = y.data_ptr(), 0.1
    if fm:
        d.E.fm_ref, d.E.fm_w, d.E.fm_wdev = ref.data_ptr(), 0.3, wdev.data_ptr()
    assert f16_ok(ops, d) == 1
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    assert last_kernel(ops) == NAME
    out.guards_ok()
    v, m = products(A, B, 0, False)
    yy = y[:, :N].double()
    if fm:
        v = v + 0.3 * 0.5 * torch.sign(yy - ref[:, :N].double())
        m = m + 0.15
    mult = torch.where(yy > 0, torch.ones_like(yy), torch.full_like(yy, 0.1))
    v, m = v * mult, m * mult
    check(out.got(), v, m, TOL, "masked gradient")
    check(cs.got(), cs.init.double() + v.sum(0), cs.init.double().abs() + m.sum(0), TOL, "colsum")


def test_gemm_three_launches_give_the_same_bits(ops):
    M, N, K = 129, 160, 160
    A, B = operands(ops, M, N, K, seed=14)
    bias = rnd(N, seed=6)

    def go():
        out = Out(M, N)
        launch(ops, A, B, out, precision=4, bias=bias)
        assert last_kernel(ops) == NAME
        return out.flat.view(torch.int32).clone()

    same_bits(go)


def test_gemm_rows_over_many_decades_against_float64(ops):
    """rows of A from 1e-30 to 1e+30: the two reciprocal scales are applied one after the other"""
    M, N, K = 129, 160, 160
    x = rnd(M, K, seed=15) * torch.logspace(-30, 30, M, device=DEV)[:, None]
    A = as_image(ops, plain(ops, x))
    B = as_image(ops, plain(ops, rnd(N, K, seed=16)))
    run(ops, A, B, M, N, precision=4, tol=TOL, seed=3)
    assert last_kernel(ops) == NAME


def test_gemm_inf_row_stays_in_its_row(ops):
    M, N, K = 129, 160, 160
    x = rnd(M, K, seed=17)
    x[5, 7] = float("inf")
    A = plain(ops, x)
    x0 = x.clone()
    x0[5] = 0.0
    A0 = plain(ops, x0)                     # (the float64 reference reads finite values)
    as_image(ops, A)
    B = as_image(ops, plain(ops, rnd(N, K, seed=18)))
    out = Out(M, N)
    launch(ops, A, B, out, precision=4)
    assert last_kernel(ops) == NAME
    out.guards_ok()
    got = out.got()
    assert not bool(torch.isfinite(got[5]).any()), "a finite value in the row of the inf"
    keep = torch.arange(M, device=DEV) != 5
    want, mag = products(A0, B, 0, False)
    check(got[keep], want[keep], mag[keep], TOL, "rows beside the inf row")


DECLINED = ["windowed", "k48", "x3_out", "split_k", "mixed", "fp32", "bf16_out", "no_scales"]


@pytest.mark.parametrize("what", DECLINED)
def test_descriptors_the_kernel_declines(ops, what):
    """f2g_gemm_f16_ok != 1 and F2G_EINVAL from f2g_gemm -- never another kernel; the output stays untouched"""
    M, N, K = 129, 160, 48 if what == "k48" else 160
    if what == "windowed":
        A = win1(ops, rnd(3, 45, 32, seed=1), L_out=41, step=1, pad=0, taps=5)
        scales = torch.ones(A.o.rows, device=DEV)
        A.o.split, A.o.rscale = 5, scales.data_ptr()
        B = as_image(ops, plain(ops, rnd(N, K, seed=2)))
    elif what == "k48":
        A, B = plain(ops, rnd(M, K, seed=1)), plain(ops, rnd(N, K, seed=2))
        scales = torch.ones(M + N, device=DEV)
        for op in (A, B):
            op.o.split, op.o.rscale = 5, scales.data_ptr()
    else:
        A, B = operands(ops, M, N, K, seed=19)
    out = Out(A.o.rows, N)
    d = make_desc(ops, A, B, out, precision=4)
    spare = torch.zeros(8, device=DEV)
    if what == "x3_out":
        d.E.x3_out = spare.data_ptr()
    elif what == "split_k":
        d.split_k = 2
        d.E.atomic = 1
    elif what == "mixed":
        d.B.split = 1
    elif what == "fp32":                # the fp32 tensors themselves: "would qualify", but not launched as they are
        d.A.base, d.A.split, d.A.rscale = A.flat.data_ptr() + 4 * A.off, 0, None
        d.B.base, d.B.split, d.B.rscale = B.flat.data_ptr() + 4 * B.off, 0, None
    elif what == "bf16_out":
        d.E.c_bf16 = 1
    elif what == "no_scales":
        d.A.rscale = None
    assert_declined(ops, d, out, ok=2 if what == "fp32" else 0)
    if what in ("mixed",):              # ... and the images are refused at every other precision
        for prec in (0, 1, 2, 3):
            d.precision = prec
            assert ops.L.lib.f2g_gemm(C.byref(d), ops.L.stream_ptr()) == EINVAL
            d.B.split = 5
            assert ops.L.lib.f2g_gemm(C.byref(d), ops.L.stream_ptr()) == EINVAL
            d.B.split = 1
        torch.cuda.synchronize()


def test_colsum_part_rows_is_zero_for_the_kernel(ops):
    A, B = operands(ops, 129, 160, 160, seed=20)
    d = make_desc(ops, A, B, Out(129, 160), precision=4)
    assert ops.L.lib.f2g_gemm_colsum_part_rows(C.byref(d)) == 0
    d.E.colsum_part_ld = 164
    assert f16_ok(ops, d) == 0


# ------------------------------------------------------------------ ops.gemm
def test_ops_gemm_takes_the_kernel_and_marks_a_requested_x3_image_bad(fp16x3):
    ops = fp16x3
    M, N, K = 300, 160, 160
    x, w, bias = rnd(M, K, seed=1), torch.nn.Parameter(rnd(N, K, seed=2, scale=K ** -0.5)), rnd(N, seed=3)
    out = torch.full((M, N), NAN, device=DEV)
    out._f2g_x3_buf = torch.empty(M * N * 3, device=DEV, dtype=torch.bfloat16)
    n0 = ops.FP16X3_LAUNCHES
    ops.gemm(ops.mat(x), ops.mat(w), out, bias=bias, x3_out=True)
    assert ops.FP16X3_LAUNCHES == n0 + 1 and last_kernel(ops) == NAME
    assert getattr(out, "_f2g_x3_bad", False) and getattr(out, "_f2g_x3", None) is None
    want = x.double() @ w.detach().double().t() + bias.double()[None]
    mag = x.double().abs() @ w.detach().double().abs().t() + bias.double().abs()[None]
    check(out.double(), want, mag, TOL, "ops.gemm")
    # a data gradient (form 1) through the cached transpose counts as form 0
    g = rnd(M, N, seed=4)
    gx = torch.full((M, K), NAN, device=DEV)
    ops.gemm(ops.mat(g), ops.mat(w), gx, form=1)
    assert ops.FP16X3_LAUNCHES == n0 + 2 and last_kernel(ops) == NAME
    check(gx.double(), g.double() @ w.detach().double(), g.double().abs() @ w.detach().double().abs(), TOL, "dgrad")
    # below either threshold, and in the plain bf16x6 mode: the kernel is not used
    for k, n in ((192, 1), (32, 161)):
        ops.FP16X3_MIN_K, ops.FP16X3_MIN_N = k, n
        ops.gemm(ops.mat(x), ops.mat(w), out, bias=bias)
        assert ops.FP16X3_LAUNCHES == n0 + 2 and last_kernel(ops) != NAME
    ops.FP16X3_MIN_K, ops.FP16X3_MIN_N = 32, 160
    ops.gemm(ops.mat(x), ops.mat(w), out, bias=bias)
    assert ops.FP16X3_LAUNCHES == n0 + 3 and last_kernel(ops) == NAME
    n0 += 1
    ops.set_gemm_precision("bf16x6")
    ops.gemm(ops.mat(x), ops.mat(w), out, bias=bias)
    assert ops.FP16X3_LAUNCHES == n0 + 2 and last_kernel(ops) != NAME


def test_weight_images_follow_their_weights(fp16x3):
    """after a raw-pointer update (the optimizer's way: bump_weight_epoch + the batched rebuild_derived) and after
    an autograd-visible in-place update, the next launch reads a rebuilt image and rebuilt scales"""
    ops = fp16x3
    M, N, K = 129, 160, 160
    x, w = rnd(M, K, seed=1), torch.nn.Parameter(rnd(N, K, seed=2))
    out = torch.empty(M, N, device=DEV)

    def launch_and_check(what):
        n0 = ops.FP16X3_LAUNCHES
        ops.gemm(ops.mat(x), ops.mat(w), out)
        assert ops.FP16X3_LAUNCHES == n0 + 1 and last_kernel(ops) == NAME
        wd = w.detach().double()
        check(out.double(), x.double() @ wd.t(), x.double().abs() @ wd.abs().t(), TOL, what)
        img, rs = cached_image(ops, w)
        want_img, want_rs = emul.image(w.detach().cpu())
        assert torch.equal(img, want_img) and torch.equal(rs, want_rs), f"{what}: the cached image is stale"
        return out.clone()

    image_follows_weight(ops, w, launch_and_check)


# ------------------------------------------------------------------ model level, against the CPU oracle
def test_stage1_and_infer_against_oracle(fp16x3):
    """the construction of test_hip_generator.py::test_stage1_against_oracle_other_shape (B = 3, odd T) with widths
    whose pointwise reductions are all multiples of 32, at that test's tolerances; 4-step inference <= 1e-4 RMS"""
    r = stage1_against_oracle(fp16x3, ("FP16X3_LAUNCHES",), infer=True)
    print(f"fp16x3 launches: forward {r.fwd[0]}, backward {r.bwd[0]}, inference {r.inf[0]}")
    assert r.fwd[0] > 0, "the forward pass never reached the fp16x3 kernel"
    assert r.bwd[0] > 0, "the backward pass never reached the fp16x3 kernel"
