"""fp16x3 weight gradients on the GPU: f2g_split_f16x2_cols bit for bit against its emulation
(tests/fp16x3_cols_emul.py), gemm_h3w_kernel against float64 over poisoned operands and guarded outputs (the helpers
of tests/test_hip_gemm_routes.py), the descriptors it must decline, ops.wgrad's routing, and a generator's stage-1
step against the CPU oracle with forward, data gradient and weight gradient all in the one arithmetic.

Tolerance of the GEMM cases: tests/test_hip_gemm_f16.py's, |got - want| <= 1.8e-6 * (|A|^T |B| + |what the output
held|) per element: a power-of-two scale per column leaves the sum over rows exactly, so the per-product bound is the
forward kernel's 3 * 2^-22, beside the suite's 1e-6 for exact-class fp32 accumulation."""
import pytest
import torch

import fp16x3_cols_emul as cols_emul
from fp16x3_gpu import (EINVAL, TOL, as_cols_image, assert_declined, f16_ok, fp16x3_mode, ops, ran, same_bits,
                        stage1_against_oracle)
from test_hip_gemm_routes import DEV, NAN, SENT, Out, check, last_kernel, launch, make_desc, plain, products, rnd, run, win1

pytestmark = pytest.mark.gpu

NAME = "h3w"


@pytest.fixture
def fp16x3(ops):
    """the mode with all three of its thresholds lowered: forward kernel from K = 32 and one output column on, the
    weight-gradient kernel from one reduction row on"""
    with fp16x3_mode(ops, "FP16X3_MIN_K", "FP16X3_MIN_N", "FP16X3_WGRAD_MIN_ROWS"):
        ops.FP16X3_MIN_K, ops.FP16X3_MIN_N, ops.FP16X3_WGRAD_MIN_ROWS = 32, 1, 1
        yield ops


# ------------------------------------------------------------------ the column image
def special_cols(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g)
    x *= torch.ldexp(torch.ones(rows, cols), torch.randint(-20, 1, (rows, cols), generator=g))
    x[:, 0] = 0.0                               # all zero
    x[:, 1] = 0.0
    x[rows // 2, 1] = -3.7e-3                   # a single non-zero element
    x[:, 2] = x[:, 2].clamp(-1.9, 1.9)
    x[min(3, rows - 1), 2] = 2.0                # amax exactly a power of two
    x[:, 3] = -x[:, 3].abs().clamp(max=0.99)
    x[0, 3] = -1.0                              # a NEGATIVE power-of-two amax
    x[:, 4] *= 1e-30                            # tiny
    x[:, 5] *= 1e30                             # huge
    x[:, 6] *= 2.0 ** -130                      # subnormal floats: the clamped scale
    x[rows - 1, 7] = float("inf")               # one inf: scale 1, the column stays as it is
    x[rows // 3, 8] = NAN                       # one NaN: likewise
    return x


def same_nan(words):
    """int32 image words with every NaN half replaced by one pattern: which NaN (sign, payload) a conversion or
    inf - inf yields is the one thing the CPU and the GPU need not agree on"""
    h = words.contiguous().view(torch.int16).clone()
    h[(h & 0x7fff) > 0x7c00] = 0x7e00
    return h


@pytest.mark.parametrize("rows,cols,ld", [(5, 32, 32), (33, 160, 176), (4100, 132, 136)])
def test_column_image_is_bit_identical_to_the_emulation(ops, rows, cols, ld):
    """(4100, 132, 136): the maxima cross blocks, the column count is no multiple of 32"""
    x = special_cols(rows, cols, 7 * rows + cols)
    pre, tail = 8, 3 * ld + 4
    src = torch.full((pre + rows * ld + tail,), NAN)
    src[pre:pre + rows * ld].view(rows, ld)[:, :cols] = x
    src = src.to(DEV)
    dst = torch.full_like(src, SENT)
    rs = torch.full((cols + 8,), SENT, device=DEV)
    work = torch.full((cols + 8,), 0x5a5a5a5a, device=DEV, dtype=torch.int32)
    want_img, want_rs = cols_emul.image(x)

    def body_of(buf):
        return buf.cpu()[pre:pre + rows * ld].view(rows, ld)

    bits = []
    for _ in range(3):                          # ... and three calls give the same bits
        ops.call("f2g_split_f16x2_cols", dst.data_ptr() + 4 * pre, rs.data_ptr() + 16, work.data_ptr() + 16,
                 src.data_ptr() + 4 * pre, ld, rows, cols)
        torch.cuda.synchronize()
        bits.append((dst.view(torch.int32).clone(), rs.view(torch.int32).clone()))
    assert all(torch.equal(b[0], bits[0][0]) and torch.equal(b[1], bits[0][1]) for b in bits[1:])
    got, body = dst.cpu(), body_of(dst)
    got_img = body[:, :cols].contiguous().view(torch.int32)
    nan_half = (want_img.contiguous().view(torch.int16) & 0x7fff) > 0x7c00
    assert int(nan_half.sum()) >= 2, "test bug: the inf and NaN columns yield NaN halves"
    differ = same_nan(got_img) != same_nan(want_img)
    assert not bool(differ.any()), f"{int(differ.sum())} halves differ"
    assert torch.equal(rs.cpu()[4:4 + cols].view(torch.int32), want_rs.view(torch.int32))
    # nothing else was written: the ld padding, the floats before the first and after the last row, the guards of the
    # scales and of the scratch words
    assert bool((body[:, cols:] == SENT).all()) and bool((got[:pre] == SENT).all())
    assert bool((got[pre + rows * ld:] == SENT).all())
    assert bool((rs.cpu()[:4] == SENT).all()) and bool((rs.cpu()[4 + cols:] == SENT).all())
    assert bool((work.cpu()[:4] == 0x5a5a5a5a).all()) and bool((work.cpu()[4 + cols:] == 0x5a5a5a5a).all())
    # in place (dst = src) gives the same image
    ops.call("f2g_split_f16x2_cols", src.data_ptr() + 4 * pre, rs.data_ptr() + 16, work.data_ptr() + 16,
             src.data_ptr() + 4 * pre, ld, rows, cols)
    torch.cuda.synchronize()
    inplace = body_of(src)[:, :cols].contiguous().view(torch.int32)
    assert torch.equal(inplace, got_img)
    assert bool(torch.isnan(body_of(src)[:, cols:]).all())


def test_column_image_declines_what_it_cannot_address(ops):
    buf = torch.zeros(4 * 64 + 8, device=DEV)
    rs = torch.zeros(64, device=DEV)
    work = torch.zeros(64, device=DEV, dtype=torch.int32)
    lib, st = ops.L.lib, ops.L.stream_ptr()
    p, r, w = buf.data_ptr(), rs.data_ptr(), work.data_ptr()
    for ld, rows, cols in ((64, 2, 30), (64, 2, 0), (28, 2, 32), (34, 2, 32), (64, 0, 32), (64, -1, 32)):
        assert lib.f2g_split_f16x2_cols(p, r, w, p, ld, rows, cols, st) == EINVAL, (ld, rows, cols)
    assert lib.f2g_split_f16x2_cols(p + 4, r, w, p, 64, 2, 32, st) == EINVAL
    assert lib.f2g_split_f16x2_cols(p, r, w, p + 8, 64, 2, 32, st) == EINVAL
    for args in ((None, r, w, p), (p, None, w, p), (p, r, None, p), (p, r, w, None)):
        assert lib.f2g_split_f16x2_cols(*args, 64, 2, 32, st) == EINVAL
    assert lib.f2g_split_f16x2_cols(p, r, w, p, 64, 4, 64, st) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ GEMM against float64
def operands(ops, R, M, N, seed, scale_a=1.0):
    A = as_cols_image(ops, plain(ops, rnd(R, M, seed=seed) * scale_a))
    B = as_cols_image(ops, plain(ops, rnd(R, N, seed=seed + 50, scale=R ** -0.5)))
    return A, B


def is_h3w(ops):
    return ran(ops, NAME)


@pytest.mark.parametrize("N", [32, 128, 160])
@pytest.mark.parametrize("M", [4, 96, 128, 132])
@pytest.mark.parametrize("R", [1, 31, 32, 33, 64, 777])
def test_wgrad_shapes_against_float64(ops, R, M, N):
    """a partial slab, exactly one, an odd and an even slab count; partial tiles in both directions; plain stores"""
    A, B = operands(ops, R, M, N, seed=R + 3 * M + N)
    d, out = run(ops, A, B, M, N, form=2, precision=4, tol=TOL, seed=R)
    assert is_h3w(ops) and f16_ok(ops, d) == 1


@pytest.mark.parametrize("how,split_k", [("accumulate", 1), ("atomic", 1), ("atomic", 3)])
@pytest.mark.parametrize("M,N", [(132, 160), (128, 128)])
def test_wgrad_stores_onto_a_finite_output(ops, how, split_k, M, N):
    """accumulating and atomic stores onto what the output held; three chunks of the reduction rescaled, then added"""
    A, B = operands(ops, 777, M, N, seed=21)
    d, out = run(ops, A, B, M, N, form=2, precision=4, tol=TOL, seed=5, split_k=split_k, epi={how: True, "scale": 0.75})
    assert is_h3w(ops) and f16_ok(ops, d) == 1


def test_wgrad_columns_over_many_decades_against_float64(ops):
    """columns of A from 1e-30 to 1e+30: one scale per column, the two reciprocals applied one after the other"""
    R, M, N = 160, 132, 160
    A = as_cols_image(ops, plain(ops, rnd(R, M, seed=15) * torch.logspace(-30, 30, M, device=DEV)[None, :]))
    B = as_cols_image(ops, plain(ops, rnd(R, N, seed=16)))
    run(ops, A, B, M, N, form=2, precision=4, tol=TOL, seed=3)
    assert is_h3w(ops)


def test_wgrad_inf_stays_in_its_output_row(ops):
    R, M, N = 160, 132, 160
    x = rnd(R, M, seed=17)
    x0 = x.clone()
    x0[:, 7] = 0.0
    A0 = plain(ops, x0)                         # (the float64 reference reads finite values)
    x[5, 7] = float("inf")
    A = as_cols_image(ops, plain(ops, x))
    B = as_cols_image(ops, plain(ops, rnd(R, N, seed=18)))
    out = Out(M, N)
    launch(ops, A, B, out, form=2, precision=4)
    assert is_h3w(ops)
    out.guards_ok()
    got = out.got()
    assert not bool(torch.isfinite(got[7]).any()), "a finite value in the output row of the inf"
    keep = torch.arange(M, device=DEV) != 7
    want, mag = products(A0, B, 2, False)
    check(got[keep], want[keep], mag[keep], TOL, "rows beside the inf's")


def test_wgrad_three_launches_give_the_same_bits(ops):
    A, B = operands(ops, 777, 132, 160, seed=14)

    def go():
        out = Out(132, 160)
        launch(ops, A, B, out, form=2, precision=4)
        assert is_h3w(ops)
        return out.flat.view(torch.int32).clone()

    same_bits(go)


DECLINED = ["windowed", "split5", "no_scales", "bf16_out", "m_mod_4", "other_precisions", "form0", "split_k_plain"]


@pytest.mark.parametrize("what", DECLINED)
def test_descriptors_the_kernel_declines(ops, what):
    """f2g_gemm_f16_ok == 0 and F2G_EINVAL from f2g_gemm -- never another kernel; the output stays untouched"""
    R, M, N = 160, 132, 160
    form = 0 if what == "form0" else 2
    if what == "form0":                 # (extents that form 0 accepts: a reduction of whole slabs over the columns)
        M = 160
    A, B = operands(ops, R, M, N, seed=19)
    if what == "windowed":
        B = win1(ops, rnd(4, 44, 32, seed=1), L_out=40, step=1, pad=0, taps=5)         # 160 rows x 160 columns
        scales = torch.ones(B.o.cols, device=DEV)
        B.o.split, B.o.rscale = 6, scales.data_ptr()
    if what == "m_mod_4":               # (130 columns of the image of 132)
        M = A.o.cols = 130
    out = Out(A.o.rows if form == 0 else M, B.o.rows if form == 0 else N)
    d = make_desc(ops, A, B, out, form=form, precision=4)
    if what == "split5":
        d.B.split = 5
    elif what == "no_scales":
        d.A.rscale = None
    elif what == "bf16_out":
        d.E.c_bf16 = 1
    elif what == "split_k_plain":       # (a split reduction needs atomic stores)
        d.split_k = 3
    precisions = (0, 1, 2, 3) if what == "other_precisions" else (4,)
    for prec in precisions:
        d.precision = prec
        assert_declined(ops, d, out)
    if what == "other_precisions":      # (the descriptor itself is one the kernel runs)
        d.precision = 4
        assert f16_ok(ops, d) == 1


def test_fp32_operands_would_qualify_but_are_not_launched(ops):
    R, M, N = 160, 132, 160
    A, B = plain(ops, rnd(R, M, seed=1)), plain(ops, rnd(R, N, seed=2))
    out = Out(M, N)
    d = make_desc(ops, A, B, out, form=2, precision=4)
    assert_declined(ops, d, out, ok=2)


# ------------------------------------------------------------------ ops.wgrad
def test_ops_wgrad_takes_the_kernel_from_its_threshold_on(fp16x3):
    ops = fp16x3
    R, M, N = 300, 132, 160
    dy, x = rnd(R, M, seed=1), rnd(R, N, seed=2)
    g0 = rnd(M, N, seed=3)
    want = g0.double() + dy.double().t() @ x.double()
    mag = g0.double().abs() + dy.double().abs().t() @ x.double().abs()
    g = g0.clone()
    n0, f0 = ops.FP16X3_WGRAD_LAUNCHES, ops.FP16X3_LAUNCHES
    ops.wgrad(dy, M, M, ops.mat(x), g)
    torch.cuda.synchronize()
    assert ops.FP16X3_WGRAD_LAUNCHES == n0 + 1 and ops.FP16X3_LAUNCHES == f0 and is_h3w(ops)
    check(g.double(), want, mag, TOL, "ops.wgrad onto a previous g_out")
    # below the threshold, with the route disabled (the default) and in the plain bf16x6 mode: the kernel is not used
    for rows in (R + 1, ops.FP16X3_WGRAD_OFF):
        ops.FP16X3_WGRAD_MIN_ROWS = rows
        g = g0.clone()
        ops.wgrad(dy, M, M, ops.mat(x), g)
        assert ops.FP16X3_WGRAD_LAUNCHES == n0 + 1 and last_kernel(ops) != NAME
        check(g.double(), want, mag, TOL, "below the threshold")
    ops.FP16X3_WGRAD_MIN_ROWS = R
    ops.wgrad(dy, M, M, ops.mat(x), g0.clone())
    assert ops.FP16X3_WGRAD_LAUNCHES == n0 + 2 and last_kernel(ops) == NAME
    ops.set_gemm_precision("bf16x6")
    ops.wgrad(dy, M, M, ops.mat(x), g0.clone())
    assert ops.FP16X3_WGRAD_LAUNCHES == n0 + 2 and last_kernel(ops) != NAME


# ------------------------------------------------------------------ model level, against the CPU oracle
def test_stage1_against_oracle_with_fp16x3_weight_gradients(fp16x3):
    """the construction of test_hip_gemm_f16.py::test_stage1_and_infer_against_oracle (the TINY config, B = 3, odd T)
    with the weight-gradient threshold lowered as well, at that test's tolerances: forward, data gradient and weight
    gradient of the pointwise convolutions all run in the fp16x3 arithmetic"""
    r = stage1_against_oracle(fp16x3, ("FP16X3_LAUNCHES", "FP16X3_WGRAD_LAUNCHES"))
    print(f"fp16x3 launches: forward {r.fwd[0]}, data gradients {r.bwd[0]}, weight gradients {r.bwd[1]}")
    assert r.fwd[0] > 0 and r.bwd[0] > 0, "forward or data gradients never reached the fp16x3 kernel"
    assert r.bwd[1] > 0, "the backward pass never reached the fp16x3 weight-gradient kernel"
