"""fp16x3 pointwise GEMM over the fp32 activation matrix itself on the GPU (csrc/gemm_f16n.hip: gemm_h3n_kernel, operand
A marked f2g_operand.split = 9): every shape and magnitude pattern of tests/fp16x3_runtile_emul.py against float64 per
element over poisoned operands and guarded outputs (the helpers of tests/test_hip_gemm_routes.py), the epilogues the
generator uses, reproducibility, zero and non-finite input, the descriptors it must decline, the route through ops.gemm,
the cached weight image following its weight, and a generator's stage-1 step and inference against the CPU oracle.

Tolerance of the GEMM cases: |got - want| <= 1.8e-6 * sum |a||w| (tests/test_hip_gemm_f16.py: the suite's 1e-6 for
exact-class fp32 accumulation plus the arithmetic's 3 * 2^-22 per product) + 2^-28 * (largest |a| of the row's 128-row
tile) * sum_k |w|: rows share their tile's scale."""
import ctypes as C

import pytest
import torch

import fp16x3_emul
import fp16x3_runtile_emul as emul
from fp16x3_gpu import (EINVAL, TOL, as_image, assert_declined, cached_image, f16_ok, fp16x3_mode, image_follows_weight,
                        mode_name, ops, ran, same_bits, stage1_against_oracle)
from test_hip_gemm_routes import (DEV, EPI, NAN, SENT, Out, Vec, check, expect, last_kernel, launch, make_desc, plain,
                                  products, rnd, run, win1)

pytestmark = pytest.mark.gpu

NAME = "h3n<ep=all>"
H3_NAME = "h3<ep=all>"          # the image route's kernel (tests/test_hip_gemm_f16.py)
CASES = [(p, s) for s in emul.SHAPES for p in emul.PATTERNS]


@pytest.fixture
def plainn_route(ops):
    """the fp16x3 mode with the new route on from one output column and K = 32"""
    with fp16x3_mode(ops, "FP16X3_MIN_K", "FP16X3_MIN_N", "FP16X3_PLAINN_MIN_N"):
        ops.FP16X3_MIN_K, ops.FP16X3_PLAINN_MIN_N = 32, 1
        yield ops


def marked(ops, x):
    """the fp32 matrix x inside a NaN buffer (rows >= M and the columns K .. ld are NaN), marked split = 9"""
    A = plain(ops, x.to(DEV))
    A.o.split, A.o.rscale = 9, None
    return A


def weights(ops, w):
    return as_image(ops, plain(ops, w.to(DEV)))


def operands(ops, M, N, K, seed):
    return marked(ops, rnd(M, K, seed=seed)), weights(ops, rnd(N, K, seed=seed + 50, scale=K ** -0.5))


# ------------------------------------------------------------------ float64 per element
@pytest.mark.parametrize("pattern,shape", CASES)
def test_gemm_against_float64(ops, pattern, shape):
    M, K, N = shape
    x, w = emul.inputs(pattern, M, K, N)
    A, B = marked(ops, x), weights(ops, w)
    assert A.o.seq_stride > K
    out = Out(M, N)
    d = launch(ops, A, B, out, precision=4)
    assert ran(ops, NAME)
    assert f16_ok(ops, d) == 1
    out.guards_ok()
    want, mag = products(A, B, 0, False)
    floor = emul.tile_amax(x).to(DEV)[:, None] * w.double().abs().sum(1).to(DEV)[None, :]
    tol = TOL * mag + emul.FLOOR * floor
    got = out.got()
    assert torch.isfinite(got).all()
    err = (got - want).abs()
    # (err / tol, with 0 / 0 = 0: the outputs of an all-zero tile are exact)
    worst = float(torch.where(tol > 0, err / tol, torch.where(err == 0, 0.0, float("inf"))).max())
    print(f"{pattern} {shape}: worst error / tolerance {worst:.3f}")
    assert worst <= 1.0, (pattern, shape, worst, int((err > tol).sum()))


# ------------------------------------------------------------------ epilogues
@pytest.mark.parametrize("ep", ["plain", "bias"] + sorted(EPI) + ["atomic"])
def test_gemm_epilogues_against_float64(ops, ep):
    """plain; bias; bias + residual * gamma + leaky ReLU; PReLU backward with both column sums; row-mapped store;
    scaled, accumulating store; atomic accumulation"""
    M, N, K = 129, 160, 160
    A, B = operands(ops, M, N, K, seed=11)
    epi = {"plain": {}, "bias": dict(bias=True), "atomic": dict(bias=True, atomic=True)}.get(ep) \
        if isinstance(ep, str) else EPI[ep]
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


def test_gemm_mask_epilogue_against_float64(ops):
    """leaky-ReLU backward of the layer below with the column sums of the result"""
    M, N, K = 129, 160, 160
    A, B = operands(ops, M, N, K, seed=13)
    out = Out(M, N)
    y = rnd(M, out.ldc, seed=3)
    cs = Vec(N, 5)
    d = make_desc(ops, A, B, out, precision=4, colsum=cs)
    d.E.mask_src, d.E.mask_slope = y.data_ptr(), 0.1
    assert f16_ok(ops, d) == 1
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    assert last_kernel(ops) == NAME
    out.guards_ok()
    v, m = products(A, B, 0, False)
    yy = y[:, :N].double()
    mult = torch.where(yy > 0, torch.ones_like(yy), torch.full_like(yy, 0.1))
    v, m = v * mult, m * mult
    check(out.got(), v, m, TOL, "masked gradient")
    check(cs.got(), cs.init.double() + v.sum(0), cs.init.double().abs() + m.sum(0), TOL, "colsum")


def test_gemm_three_launches_give_the_same_bits(ops):
    M, K, N = 300, 160, 200
    x, w = emul.inputs("rising", M, K, N)
    A, B = marked(ops, x), weights(ops, w)
    bias = rnd(N, seed=6)

    def go():
        out = Out(M, N)
        launch(ops, A, B, out, precision=4, bias=bias)
        assert last_kernel(ops) == NAME
        return out.flat.view(torch.int32).clone()

    same_bits(go)


def test_gemm_zero_input_gives_the_epilogue_of_zero(ops):
    M, N, K = 129, 160, 160
    A, B = marked(ops, torch.zeros(M, K)), weights(ops, rnd(N, K, seed=3).cpu())
    bias = rnd(N, seed=4)
    out = Out(M, N)
    launch(ops, A, B, out, precision=4, bias=bias)
    assert last_kernel(ops) == NAME
    out.guards_ok()
    assert torch.equal(out.view()[:, :N], bias[None, :].expand(M, N))


def test_gemm_inf_stays_in_its_row(ops):
    M, K, N = 300, 160, 200
    x, w = emul.inputs("normal", M, K, N)
    x0 = x.clone()
    x[130, 40] = float("inf")
    x0[130] = 0.0                           # (the float64 reference reads finite values)
    A, A0, B = marked(ops, x), marked(ops, x0), weights(ops, w)
    out = Out(M, N)
    launch(ops, A, B, out, precision=4)
    assert last_kernel(ops) == NAME
    out.guards_ok()
    got = out.got()
    assert not bool(torch.isfinite(got[130]).any()), "a finite value in the row of the inf"
    keep = torch.arange(M, device=DEV) != 130
    want, mag = products(A0, B, 0, False)
    floor = emul.tile_amax(x0).to(DEV)[:, None] * w.double().abs().sum(1).to(DEV)[None, :]
    check(got[keep], want[keep], (mag + emul.FLOOR / TOL * floor)[keep], TOL, "rows beside the inf row")


# ------------------------------------------------------------------ refusals
DECLINED = ["a_rscale", "split_k", "x3_out", "colsum_part_ld", "bf16_out", "prelu_accumulate", "mask_atomic", "alpha",
            "k48", "k4128", "misaligned", "windowed", "b_fp32", "b_no_scales", "b_marked", "form2"]


@pytest.mark.parametrize("what", DECLINED)
def test_descriptors_the_kernel_declines(ops, what):
    """f2g_gemm_f16_ok != 1 and F2G_EINVAL from f2g_gemm -- never another kernel; the output stays untouched"""
    M, N = 129, 160
    K = {"k48": 48, "k4128": 4128}.get(what, 160)
    spare = torch.ones(max(M, N) + 8, device=DEV)
    if what == "windowed":
        A = win1(ops, rnd(3, 45, 32, seed=1), L_out=41, step=1, pad=0, taps=5)
        A.o.split = 9
        B = weights(ops, rnd(N, K, seed=2).cpu())
    elif what in ("k48", "k4128"):
        A, B = marked(ops, rnd(M, K, seed=1).cpu()), plain(ops, rnd(N, K, seed=2))
        B.o.split, B.o.rscale = 5, spare.data_ptr()
    else:
        A, B = operands(ops, M, N, K, seed=19)
    out = Out(A.o.rows, N)
    d = make_desc(ops, A, B, out, precision=4)
    if what == "a_rscale":
        d.A.rscale = spare.data_ptr()
    elif what == "split_k":
        d.split_k, d.E.atomic = 2, 1
    elif what == "x3_out":
        d.E.x3_out = spare.data_ptr()
    elif what == "colsum_part_ld":
        d.E.colsum_part_ld = 164
    elif what == "bf16_out":
        d.E.c_bf16 = 1
    elif what == "prelu_accumulate":
        d.E.prelu_slope, d.E.accumulate = spare.data_ptr(), 1
    elif what == "mask_atomic":
        d.E.mask_src, d.E.atomic = spare.data_ptr(), 1
    elif what == "alpha":
        d.A.alpha = spare.data_ptr()
    elif what == "misaligned":
        d.A.base += 4
    elif what == "b_fp32":                  # "would qualify once B is its image", but not launched as it is
        d.B.base, d.B.split, d.B.rscale = B.flat.data_ptr() + 4 * B.off, 0, None
    elif what == "b_no_scales":
        d.B.rscale = None
    elif what == "b_marked":
        d.B.base, d.B.split, d.B.rscale = B.flat.data_ptr() + 4 * B.off, 9, None
    elif what == "form2":
        d.form, d.E.atomic = 2, 1
    assert_declined(ops, d, out, ok=2 if what == "b_fp32" else 0)
    if what == "b_no_scales":               # ... and the mark is refused at every other precision
        d.B.rscale = B.rs.data_ptr() + 16
        assert f16_ok(ops, d) == 1
        for prec in (0, 1, 2, 3):
            d.precision = prec
            assert ops.L.lib.f2g_gemm(C.byref(d), ops.L.stream_ptr()) == EINVAL
        torch.cuda.synchronize()
        assert bool((out.flat[~torch.isnan(out.flat)] == SENT).all())


def test_colsum_part_rows_is_zero_for_the_kernel(ops):
    A, B = operands(ops, 129, 160, 160, seed=20)
    d = make_desc(ops, A, B, Out(129, 160), precision=4)
    assert f16_ok(ops, d) == 1
    assert ops.L.lib.f2g_gemm_colsum_part_rows(C.byref(d)) == 0


# ------------------------------------------------------------------ ops.gemm
def test_ops_gemm_takes_the_route_and_counts_it(plainn_route, monkeypatch):
    ops = plainn_route
    M, K, N = 300, 160, 192
    x, w0 = emul.inputs("rising", M, K, N)
    x, w, bias = x.to(DEV), torch.nn.Parameter(w0.to(DEV)), rnd(N, seed=3)
    out = torch.full((M, N), NAN, device=DEV)
    ops._f16_operand(ops.mat(w))            # (the weight's cached image: built before the launches are watched)
    seen, images = [], []
    real_call = ops.call

    def watch_call(name, *args):
        if name == "f2g_gemm":
            d = args[0]._obj                # (C.byref's object: the descriptor as it is launched)
            seen.append((d.A.base, d.A.split, bool(d.A.rscale), d.B.split, bool(d.B.rscale)))
        if name.startswith("f2g_split"):
            images.append(name)
        return real_call(name, *args)

    def go(**kw):
        out.fill_(NAN)
        ops.gemm(ops.mat(x), ops.mat(w), out, bias=bias, **kw)
        torch.cuda.synchronize()

    n0, i0 = ops.FP16X3_PLAINN_LAUNCHES, ops.FP16X3_LAUNCHES
    with monkeypatch.context() as mp:
        mp.setattr(ops, "call", watch_call)
        go()
    assert ops.FP16X3_PLAINN_LAUNCHES == n0 + 1 and ops.FP16X3_LAUNCHES == i0 and last_kernel(ops) == NAME
    # no per-call image of A: the launch reads the caller's matrix itself, and nothing built an image meanwhile
    assert seen == [(x.data_ptr(), 9, False, 5, True)]
    assert images == []
    wd = w.detach().double()
    want = x.double() @ wd.t() + bias.double()[None]
    floor = emul.tile_amax(x.cpu()).to(DEV)[:, None] * wd.abs().sum(1)[None, :]
    mag = x.double().abs() @ wd.abs().t() + bias.double().abs()[None] + emul.FLOOR / TOL * floor
    check(out.double(), want, mag, TOL, "ops.gemm")
    # a data gradient (form 1) through the cached transpose counts as form 0
    g = rnd(M, N, seed=4)
    gx = torch.full((M, K), NAN, device=DEV)
    ops.gemm(ops.mat(g), ops.mat(w), gx, form=1)
    assert ops.FP16X3_PLAINN_LAUNCHES == n0 + 2 and last_kernel(ops) == NAME
    check(gx.double(), g.double() @ wd, g.double().abs() @ wd.abs() + emul.FLOOR / TOL *
          emul.tile_amax(g.cpu()).to(DEV)[:, None] * wd.abs().sum(0)[None, :], TOL, "dgrad")
    # below the threshold: the image route (its own threshold allowing) takes the launch, as before the route existed
    ops.FP16X3_PLAINN_MIN_N, ops.FP16X3_MIN_N = N + 1, 1
    go()
    assert ops.FP16X3_PLAINN_LAUNCHES == n0 + 2 and ops.FP16X3_LAUNCHES == i0 + 1 and last_kernel(ops) == H3_NAME
    ops.FP16X3_PLAINN_MIN_N = N
    go()
    assert ops.FP16X3_PLAINN_LAUNCHES == n0 + 3 and last_kernel(ops) == NAME
    # what the library declines falls through with the mark cleared: K % 32 != 0 goes the bf16x6 way
    x2, w2, out2 = rnd(M, 176, seed=8), torch.nn.Parameter(rnd(N, 176, seed=9, scale=0.1)), torch.empty(M, N, device=DEV)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "call", watch_call)
        ops.gemm(ops.mat(x2), ops.mat(w2), out2)
        torch.cuda.synchronize()
    assert ops.FP16X3_PLAINN_LAUNCHES == n0 + 3 and last_kernel(ops) not in (NAME, H3_NAME)
    assert seen[-1][1] == 0 and images == []
    w2d = w2.detach().double()
    check(out2.double(), x2.double() @ w2d.t(), x2.double().abs() @ w2d.abs().t(), TOL, "the bf16x6 launch")
    ops.set_gemm_precision("bf16x6")
    go()
    assert ops.FP16X3_PLAINN_LAUNCHES == n0 + 3 and last_kernel(ops) not in (NAME, H3_NAME)


def test_the_default_leaves_every_launch_as_it_was(ops):
    """with the tunable at its default the counter stays and the output of the fp16x3 mode is bit-identical to the
    image route's launch made by hand"""
    was = mode_name(ops)
    keep = ops.FP16X3_MIN_K, ops.FP16X3_MIN_N
    assert ops.FP16X3_PLAINN_MIN_N == ops.FP16X3_TAP_OFF
    M, K, N = 300, 160, 200
    x, w0 = emul.inputs("spread", M, K, N)
    x, w, bias = x.to(DEV), torch.nn.Parameter(w0.to(DEV)), rnd(N, seed=3)
    out = torch.full((M, N), NAN, device=DEV)
    ops.set_gemm_precision("fp16x3")
    ops.FP16X3_MIN_K, ops.FP16X3_MIN_N = 32, 1
    try:
        n0, i0 = ops.FP16X3_PLAINN_LAUNCHES, ops.FP16X3_LAUNCHES
        ops.gemm(ops.mat(x), ops.mat(w), out, bias=bias)
        torch.cuda.synchronize()
        assert ops.FP16X3_PLAINN_LAUNCHES == n0 and ops.FP16X3_LAUNCHES == i0 + 1 and last_kernel(ops) == H3_NAME
    finally:
        ops.FP16X3_MIN_K, ops.FP16X3_MIN_N = keep
        ops.set_gemm_precision(was)
    # today's launch, by hand: both operands as f2g_split_f16x2 images on gemm_h3_kernel
    A, B = as_image(ops, plain(ops, x)), as_image(ops, plain(ops, w.detach()))
    ref = Out(M, N)
    launch(ops, A, B, ref, precision=4, bias=bias)
    assert last_kernel(ops) == H3_NAME
    assert torch.equal(ref.view()[:, :N].contiguous().view(torch.int32), out.view(torch.int32))


def test_weight_images_follow_their_weights(plainn_route):
    """after a raw-pointer update (the optimizer's way: bump_weight_epoch + the batched rebuild_derived) and after
    an autograd-visible in-place update, the next launch reads a rebuilt image and rebuilt scales"""
    ops = plainn_route
    M, N, K = 129, 160, 160
    x, w = rnd(M, K, seed=1), torch.nn.Parameter(rnd(N, K, seed=2))
    out = torch.empty(M, N, device=DEV)
    floor_a = emul.tile_amax(x.cpu()).to(DEV)[:, None]

    def launch_and_check(what):
        n0 = ops.FP16X3_PLAINN_LAUNCHES
        ops.gemm(ops.mat(x), ops.mat(w), out)
        assert ops.FP16X3_PLAINN_LAUNCHES == n0 + 1 and last_kernel(ops) == NAME
        wd = w.detach().double()
        mag = x.double().abs() @ wd.abs().t() + emul.FLOOR / TOL * floor_a * wd.abs().sum(1)[None, :]
        check(out.double(), x.double() @ wd.t(), mag, TOL, what)
        img, rs = cached_image(ops, w)
        want_img, want_rs = fp16x3_emul.image(w.detach().cpu())
        assert torch.equal(img, want_img) and torch.equal(rs, want_rs), f"{what}: the cached image is stale"
        return out.clone()

    image_follows_weight(ops, w, launch_and_check)


# ------------------------------------------------------------------ model level, against the CPU oracle
def test_stage1_and_infer_against_oracle(plainn_route):
    """tests/test_hip_gemm_f16.py's construction and tolerances (those of tests/test_hip_generator.py) with the route
    on: the stage-1 loss, all gradients and 4-step inference; forward and backward both reach the new kernel and the
    image route takes nothing"""
    ops = plainn_route
    r = stage1_against_oracle(ops, ("FP16X3_PLAINN_LAUNCHES", "FP16X3_LAUNCHES"), infer=True)
    print(f"launches on the route: forward {r.fwd[0]}, backward {r.bwd[0]}, inference {r.inf[0]}; on the image route: "
          f"{r.fwd[1] + r.bwd[1] + r.inf[1]}")
    assert r.fwd[0] > 0, "the forward pass never reached the kernel"
    assert r.bwd[0] > 0, "the backward pass never reached the kernel"
    assert r.fwd[1] == r.bwd[1] == r.inf[1] == 0, "the image route took a launch"
