"""fp16x3 over stride-1 windows of a halo map on the GPU: f2g_split_f16x2_seq bit for bit against its emulation
(tests/fp16x3_seq_emul.py), gemm_h3p_kernel<5 / 2> against float64 over poisoned operands and guarded outputs (the
helpers of tests/test_hip_gemm_routes.py), the descriptors it must decline, the weight images of the derived-weight
cache following their weights, and one period of the MPD against the CPU oracle.

Tolerance of the GEMM cases, per element: 1.8e-6 * (|A| |B|^T + |epilogue terms|) -- the suite's 1e-6 for exact-class
fp32 accumulation plus the arithmetic's 3 * 2^-22 per product, as tests/test_hip_gemm_f16.py -- plus the floor term of
the per-sequence scale, 2^-28 amax_seq(row) sum_k |w[n,k]|, carried through the epilogue like a product's scale."""
import ctypes as C

import pytest
import torch

import fp16x3_seq_emul as emul
from fp16x3_gpu import (EINVAL, TOL, any_grid, assert_declined, case, f16_ok, fp16x3_mode, image_follows_weight, ops,
                        ran, same_bits, scale_rows, subdisc_against_oracle)
from test_hip_gemm_routes import DEV, NAN, SENT, Out, Vec, check, expect, last_kernel, make_desc, rnd

pytestmark = pytest.mark.gpu

SHAPES = [(5, 64, 64, 128),      # 320 rows: one full and one quarter row tile
          (7, 50, 96, 128),      # a wave group's 128 rows straddle three sequences; three channel slabs
          (5, 64, 64, 160)]      # a partial column tile


@pytest.fixture
def tap_route_rows(ops, any_grid):
    """the fp16x3 mode as shipped with the two settings the end-to-end test names: FP16X3_TAP_MIN_ROWS = 1 and the
    library option x6p = 2"""
    with fp16x3_mode(ops, "FP16X3_TAP_MIN_ROWS", "X6_MIN_K"):
        ops.FP16X3_TAP_MIN_ROWS = 1
        yield ops


@pytest.fixture
def tap_route(tap_route_rows):
    """... and reductions from 32 on (the ops.gemm cases have 64 channels: K = 320 and 128)"""
    tap_route_rows.X6_MIN_K = 32
    return tap_route_rows


# ------------------------------------------------------------------ the image
def special_runs(nseq, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(nseq, n, generator=g)
    x *= torch.ldexp(torch.ones(nseq, n), torch.randint(-20, 1, (nseq, n), generator=g))
    if nseq >= 6:
        x[0] = 0.0                          # an all-zero run
        x[1] = -x[1].abs().clamp(max=0.99)
        x[1, n // 2 + 3] = -1.0             # a NEGATIVE power-of-two amax
        x[2] *= 1e30                        # huge
        x[3] *= 2.0 ** -130                 # subnormal floats: the clamped scale
    return x


@pytest.mark.parametrize("nseq,n,ld", [(6, 96, 128),            # the special runs, runs apart
                                       (3, 8192 + 352, 8544),   # not a multiple of a block's pass of 8192 floats
                                       (2, 5120, 5120)])        # the weight row of the 1024-channel layer
def test_seq_image_is_bit_identical_to_the_emulation(ops, nseq, n, ld):
    x = special_runs(nseq, n, 3 * nseq + n)
    pre, tail = 32, 64
    src = torch.full((pre + nseq * ld + tail,), NAN)
    src[pre:pre + nseq * ld].view(nseq, ld)[:, :n] = x
    src = src.to(DEV)
    dst = torch.full_like(src, SENT)
    rs = torch.full((nseq + 8,), SENT, device=DEV)
    ops.call("f2g_split_f16x2_seq", dst.data_ptr() + 4 * pre, rs.data_ptr() + 16, src.data_ptr() + 4 * pre, ld, nseq, n)
    torch.cuda.synchronize()
    want_img, want_rs = emul.image(x)
    got = dst.cpu()
    body = got[pre:pre + nseq * ld].view(nseq, ld)
    words = body[:, :n].contiguous().view(torch.int32)
    assert torch.equal(words, want_img), f"{int((words != want_img).sum())} words differ"
    assert torch.equal(rs.cpu()[4:4 + nseq].view(torch.int32), want_rs.view(torch.int32))
    # nothing outside the runs was written: between the runs, before the first, after the last, the scales' guards
    assert bool((body[:, n:] == SENT).all()) and bool((got[:pre] == SENT).all())
    assert bool((got[pre + nseq * ld:] == SENT).all())
    assert bool((rs.cpu()[:4] == SENT).all()) and bool((rs.cpu()[4 + nseq:] == SENT).all())
    assert bool(torch.equal(src.cpu()[pre:pre + nseq * ld].view(nseq, ld)[:, :n], x)), "the source was written"


def test_seq_image_declines_what_it_cannot_lay_out(ops):
    buf, dst = torch.zeros(4096, device=DEV), torch.zeros(4096, device=DEV)
    rs = torch.zeros(8, device=DEV)
    lib, st = ops.L.lib, ops.L.stream_ptr()
    for ld, nseq, n in ((64, 2, 48), (48, 2, 32), (32, 2, 64), (64, -1, 64), (64, 2, 16)):
        assert lib.f2g_split_f16x2_seq(dst.data_ptr(), rs.data_ptr(), buf.data_ptr(), ld, nseq, n, st) == EINVAL
    assert lib.f2g_split_f16x2_seq(dst.data_ptr() + 4, rs.data_ptr(), buf.data_ptr(), 64, 2, 64, st) == EINVAL
    assert lib.f2g_split_f16x2_seq(buf.data_ptr(), rs.data_ptr(), buf.data_ptr(), 64, 2, 64, st) == EINVAL     # in place
    assert lib.f2g_split_f16x2_seq(dst.data_ptr(), rs.data_ptr(), buf.data_ptr(), 64, 2, 64, st) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ GEMM against float64
@pytest.mark.parametrize("taps", [5, 2])
@pytest.mark.parametrize("S,P0,Cc,N", SHAPES)
def test_forward_epilogue_against_float64(ops, any_grid, S, P0, Cc, N, taps):
    """bias + leaky ReLU (the forward's epilogue), plain store"""
    c = case(ops, S, P0, Cc, N, taps, seed=S + N)
    bias = rnd(N, seed=1) * 1e-3
    out = Out(c.M, N)
    d = make_desc(ops, c.A, c.B, out, precision=4, bias=bias, lrelu=0.1)
    assert f16_ok(ops, d) == 1
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    assert ran(ops, f"h3p<taps={taps}>")
    out.guards_ok()
    want, m, _, _ = expect(c.acc, c.mag, bias=bias, lrelu=0.1)
    check(out.got(), want, m, TOL, "forward")
    # the same descriptor over the fp32 operands: "would run once both are replaced by their images"
    d.A.base, d.A.split, d.A.rscale = c.A.flat.data_ptr() + 4 * c.A.off, 0, None
    d.B.base, d.B.split, d.B.rscale = c.B.flat.data_ptr() + 4 * c.B.off, 0, None
    assert f16_ok(ops, d) == 2
    assert ops.L.lib.f2g_gemm(C.byref(d), ops.L.stream_ptr()) == EINVAL


@pytest.mark.parametrize("taps", [5, 2])
@pytest.mark.parametrize("S,P0,Cc,N", SHAPES)
def test_data_gradient_epilogue_against_float64(ops, any_grid, S, P0, Cc, N, taps):
    """row map + leaky-ReLU backward mask + feature-matching term + column sums (the data gradient's epilogue): the
    sums once by atomics, once as partial rows"""
    c = case(ops, S, P0, Cc, N, taps, seed=2 * S + N)
    ldo = N + 8
    rowmap = (P0, (P0 + 4) * ldo, ldo, 2 * ldo)         # a halo map of the output
    out = Out(c.M, N, rowmap=rowmap)
    y_full, ref_full = rnd(out.flat.numel(), seed=3), rnd(out.flat.numel(), seed=4)
    wdev = torch.tensor([0.5], device=DEV)
    fmw = 0.3 * 1e-3
    cs = Vec(N, 5)
    d = make_desc(ops, c.A, c.B, out, precision=4, colsum=cs)
    d.E.mask_src, d.E.mask_slope = y_full.data_ptr() + 4 * out.base, 0.1
    d.E.fm_ref, d.E.fm_w, d.E.fm_wdev = ref_full.data_ptr() + 4 * out.base, fmw, wdev.data_ptr()
    assert f16_ok(ops, d) == 1
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    assert ran(ops, f"h3p<taps={taps}>")
    out.guards_ok()
    yy, rr = y_full[out.offs].double(), ref_full[out.offs].double()
    v = c.acc + fmw * 0.5 * torch.sign(yy - rr)
    m = c.mag + fmw * 0.5
    mult = torch.where(yy > 0, torch.ones_like(yy), torch.full_like(yy, 0.1))
    v, m = v * mult, m * mult
    check(out.got(), v, m, TOL, "masked gradient")
    check(cs.got(), cs.init.double() + v.sum(0), cs.init.double().abs() + m.sum(0), TOL, "colsum")
    # partial rows: one per 64 output rows of whole 256-row tiles, plain stores
    nrows = ops.L.lib.f2g_gemm_colsum_part_rows(C.byref(d))
    assert nrows == 4 * ((c.M + 255) // 256)
    parts = torch.full((nrows + 2, N), SENT, device=DEV)
    out2 = Out(c.M, N, rowmap=rowmap)
    d.E.C = out2.flat.data_ptr() + 4 * out2.base
    d.E.colsum, d.E.colsum_part_ld = parts.data_ptr() + 4 * N, N
    assert f16_ok(ops, d) == 1
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    out2.guards_ok()
    assert torch.equal(out2.got(), out.got())
    assert bool((parts[0] == SENT).all()) and bool((parts[-1] == SENT).all())
    check(parts[1:-1].double().sum(0), v.sum(0), m.sum(0), TOL, "partial column sums")


@pytest.mark.parametrize("taps", [5, 2])
def test_x3_out_is_the_image_of_the_result(ops, any_grid, taps):
    """E.x3_out: the three-piece bf16 image of the contiguous output, for the bf16x6 consumers"""
    S, P0, Cc, N = SHAPES[0]
    c = case(ops, S, P0, Cc, N, taps, seed=9)
    guard = 64
    flat = torch.full((guard + c.M * N + guard,), SENT, device=DEV)
    flat[guard:guard + c.M * N] = NAN
    img = torch.full((guard + c.M * N * 3 + guard,), 1.0, device=DEV, dtype=torch.bfloat16)
    out = Out(c.M, N)
    d = make_desc(ops, c.A, c.B, out, precision=4, bias=rnd(N, seed=2) * 1e-3)
    d.E.C, d.E.ldc = flat.data_ptr() + 4 * guard, N
    d.E.x3_out = img.data_ptr() + 2 * guard
    assert f16_ok(ops, d) == 1
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    assert last_kernel(ops) == f"h3p<taps={taps}>"
    assert bool((flat[:guard] == SENT).all()) and bool((flat[guard + c.M * N:] == SENT).all())
    assert bool((img[:guard] == 1.0).all()) and bool((img[guard + c.M * N * 3:] == 1.0).all())
    res = flat[guard:guard + c.M * N].clone()
    assert torch.isfinite(res).all()
    want = ops.x3_flat_image(res)
    torch.cuda.synchronize()
    assert torch.equal(img[guard:guard + c.M * N * 3].view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("taps", [5, 2])
def test_x3_out_of_a_row_mapped_masked_data_gradient(ops, any_grid, taps):
    """the production use of E.x3_out: a data gradient landing in a halo map through the row map, with the
    leaky-ReLU mask and the column sums -- the image of the whole contiguous map (zero halo rows included, as
    x3_reserve leaves them) equals a fresh x3_flat_image of it"""
    S, P0, Cc, N = SHAPES[1]
    c = case(ops, S, P0, Cc, N, taps, seed=21)
    Hp, guard = P0 + 4, 64
    rowmap = (P0, Hp * N, N, 2 * N)
    flat = torch.full((guard + S * Hp * N + guard,), SENT, device=DEV)
    body = flat[guard:guard + S * Hp * N].view(S, Hp, N)
    body[:] = NAN
    body[:, :2] = 0.0
    body[:, Hp - 2:] = 0.0
    img = torch.full((guard + S * Hp * N * 3 + guard,), 1.0, device=DEV, dtype=torch.bfloat16)
    img[guard:guard + S * Hp * N * 3] = 0.0
    y = rnd(S * Hp * N, seed=5)
    cs = Vec(N, 6)
    d = make_desc(ops, c.A, c.B, Out(c.M, N), precision=4, colsum=cs)
    d.E.C, d.E.ldc = flat.data_ptr() + 4 * guard, N
    d.E.P0o, d.E.seq_stride_o, d.E.row_stride_o, d.E.off_o = rowmap
    d.E.mask_src, d.E.mask_slope = y.data_ptr(), 0.1
    d.E.x3_out = img.data_ptr() + 2 * guard
    assert f16_ok(ops, d) == 1
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    assert last_kernel(ops) == f"h3p<taps={taps}>"
    assert bool((flat[:guard] == SENT).all()) and bool((flat[guard + S * Hp * N:] == SENT).all())
    assert bool((img[:guard] == 1.0).all()) and bool((img[guard + S * Hp * N * 3:] == 1.0).all())
    assert bool((body[:, :2] == 0).all()) and bool((body[:, Hp - 2:] == 0).all()), "a halo row was written"
    yy = y.view(S, Hp, N)[:, 2:2 + P0].reshape(c.M, N).double()
    mult = torch.where(yy > 0, torch.ones_like(yy), torch.full_like(yy, 0.1))
    v, m = c.acc * mult, c.mag * mult
    check(body[:, 2:2 + P0].reshape(c.M, N).double(), v, m, TOL, "row-mapped masked gradient")
    check(cs.got(), cs.init.double() + v.sum(0), cs.init.double().abs() + m.sum(0), TOL, "colsum")
    want = ops.x3_flat_image(body.reshape(-1).clone())
    torch.cuda.synchronize()
    assert torch.equal(img[guard:guard + S * Hp * N * 3].view(torch.int16), want.view(torch.int16))


def test_three_launches_give_the_same_bits(ops, any_grid):
    c = case(ops, *SHAPES[1], 5, seed=4)

    def go():
        out = Out(c.M, c.N)
        d = make_desc(ops, c.A, c.B, out, precision=4)
        ops.call("f2g_gemm", C.byref(d))
        torch.cuda.synchronize()
        return out.flat.view(torch.int32).clone()

    same_bits(go)


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("what", ["taps3", "stride3", "staged", "c32", "no_scales", "grid"])
def test_descriptors_the_kernel_declines(ops, lib_option, what):
    """f2g_gemm_f16_ok == 0 and F2G_EINVAL from f2g_gemm -- never another kernel; the output stays untouched"""
    lib_option("x6p", 1 if what == "grid" else 2)      # ("grid": the default option keeps small grids off the kernel)
    S, P0, Cc, N = SHAPES[0]
    kw = dict(taps3=dict(taps=3), stride3=dict(taps=5, step=3), staged=dict(taps=5, extra=40),
              c32=dict(taps=5), no_scales=dict(taps=5), grid=dict(taps=5))[what]
    c = case(ops, S, P0, 32 if what == "c32" else Cc, N, **kw)
    out = Out(c.M, N)
    d = make_desc(ops, c.A, c.B, out, precision=4)
    if what == "no_scales":
        d.A.rscale = None
    assert_declined(ops, d, out)
    for prec in (0, 1, 2, 3):           # ... and the images are refused at every other precision
        d.precision = prec
        assert ops.L.lib.f2g_gemm(C.byref(d), ops.L.stream_ptr()) == EINVAL


# ------------------------------------------------------------------ ops.gemm
def ops_case(ops, taps, seed):
    S, P0, Cc, N = SHAPES[0]
    Hp = P0 + taps - 1
    x = rnd(S, Hp, Cc, seed=seed) * torch.logspace(-3, 3, S, device=DEV)[:, None, None]
    flat = torch.full((S * Hp * Cc + 256 * Cc,), NAN, device=DEV)
    flat[:S * Hp * Cc] = x.reshape(-1)
    a = torch.stack([x[:, i:i + P0] for i in range(taps)], 2).reshape(S * P0, taps * Cc).double()
    amax = x.double().abs().reshape(S, -1).amax(1).repeat_interleave(P0)
    return flat, a, amax, (S, Hp, Cc, P0, N)


@pytest.mark.parametrize("taps", [5, 2])
def test_ops_gemm_takes_the_route_and_counts_it(tap_route, taps):
    ops = tap_route
    flat, a, amax, (S, Hp, Cc, P0, N) = ops_case(ops, taps, 3)
    w, bias = torch.nn.Parameter(rnd(N, taps * Cc, seed=7, scale=0.1)), rnd(N, seed=8)
    out = torch.full((S * P0, N), NAN, device=DEV)

    def go():
        ops.gemm(ops.win1d(flat, S, Hp, Cc, P0, 1, 0, taps), ops.mat(w), out, bias=bias, lrelu=0.1)
        torch.cuda.synchronize()

    n0 = ops.FP16X3_TAP_LAUNCHES
    go()
    assert ops.FP16X3_TAP_LAUNCHES == n0 + 1 and last_kernel(ops) == f"h3p<taps={taps}>"
    wd = w.detach().double()
    mag = a.abs() @ wd.abs().t() + emul.FLOOR * amax[:, None] * wd.abs().sum(1)[None, :] / TOL
    want, m, _, _ = expect(a @ wd.t(), mag, bias=bias, lrelu=0.1)
    check(out.double(), want, m, TOL, "ops.gemm")
    # below the threshold, with the route off, and in the plain bf16x6 mode: the bf16x6 kernels
    for rows in (S * P0 + 1, ops.FP16X3_TAP_OFF):
        ops.FP16X3_TAP_MIN_ROWS = rows
        go()
        assert ops.FP16X3_TAP_LAUNCHES == n0 + 1 and not last_kernel(ops).startswith("h3p")
    ops.FP16X3_TAP_MIN_ROWS = S * P0
    go()
    assert ops.FP16X3_TAP_LAUNCHES == n0 + 2 and last_kernel(ops) == f"h3p<taps={taps}>"
    ops.set_gemm_precision("bf16x6")
    go()
    assert ops.FP16X3_TAP_LAUNCHES == n0 + 2 and not last_kernel(ops).startswith("h3p")


def test_weight_images_follow_their_weights(tap_route):
    """after a raw-pointer update (the optimizer's way: bump_weight_epoch + the batched rebuild_derived) and after
    an autograd-visible in-place update, the next launch reads a rebuilt image and rebuilt scales"""
    ops = tap_route
    taps = 5
    flat, a, amax, (S, Hp, Cc, P0, N) = ops_case(ops, taps, 5)
    w = torch.nn.Parameter(rnd(N, taps * Cc, seed=2))
    out = torch.empty(S * P0, N, device=DEV)

    def launch_and_check(what):
        n0 = ops.FP16X3_TAP_LAUNCHES
        ops.gemm(ops.win1d(flat, S, Hp, Cc, P0, 1, 0, taps), ops.mat(w), out)
        assert ops.FP16X3_TAP_LAUNCHES == n0 + 1 and last_kernel(ops) == "h3p<taps=5>"
        wd = w.detach().double()
        mag = a.abs() @ wd.abs().t() + emul.FLOOR * amax[:, None] * wd.abs().sum(1)[None, :] / TOL
        check(out.double(), a @ wd.t(), mag, TOL, what)
        buf = ops._f16_seq_operand(ops.mat(w))._keep[0]
        torch.cuda.synchronize()
        K = taps * Cc
        img, rs = buf[:N * K].cpu().view(torch.int32).view(N, K), buf[N * K:N * K + N].cpu()
        want_img, want_rs = emul.image(w.detach().cpu())
        assert torch.equal(img, want_img) and torch.equal(rs, want_rs), f"{what}: the cached image is stale"
        return out.clone()

    image_follows_weight(ops, w, launch_and_check)


def test_images_of_re_laid_weights_follow_their_weights(tap_route):
    """the MPD's chains: the image hangs under a packed copy of the conv weight (pack -> f16x2seq).  When
    rebuild_derived replays the chain, the image's own launch must come behind the batched re-layout it reads (it
    flushes the open batch in front of itself): the packed copy, the image and the scales follow the weight"""
    ops = tap_route
    from flow2gan_amd import fused_disc as FD
    taps = 5
    flat, a, amax, (S, Hp, Cc, P0, N) = ops_case(ops, taps, 6)
    w = torch.nn.Parameter(rnd(N, Cc, taps, 1, seed=3))
    out = torch.empty(S * P0, N, device=DEV)
    K = taps * Cc

    def launch_and_check(what, launch=True):
        wp = ops.derived(w, "pack", FD.pack_conv_weight)
        if launch:
            n0 = ops.FP16X3_TAP_LAUNCHES
            ops.gemm(ops.win1d(flat, S, Hp, Cc, P0, 1, 0, taps), ops.mat(wp), out)
            assert ops.FP16X3_TAP_LAUNCHES == n0 + 1 and last_kernel(ops) == "h3p<taps=5>"
        buf = ops._f16_seq_operand(ops.mat(wp))._keep[0]
        torch.cuda.synchronize()
        packed = w.detach().permute(0, 2, 3, 1).reshape(N, K).cpu()
        assert torch.equal(wp.cpu(), packed), f"{what}: the packed copy is stale"
        img, rs = buf[:N * K].cpu().view(torch.int32).view(N, K), buf[N * K:N * K + N].cpu()
        want_img, want_rs = emul.image(packed)
        assert torch.equal(img, want_img) and torch.equal(rs, want_rs), f"{what}: the cached image is stale"
        if launch:
            wd = packed.double().to(DEV)
            mag = a.abs() @ wd.abs().t() + emul.FLOOR * amax[:, None] * wd.abs().sum(1)[None, :] / TOL
            check(out.double(), a @ wd.t(), mag, TOL, what)
        return buf

    first = launch_and_check("first launch")
    scale_rows(w)
    ops.bump_weight_epoch([w])
    replayed = ops.rebuild_derived([w])
    assert replayed >= 2 or not ops.EAGER_REBUILD          # (the packed copy and the image under it)
    # what the replay itself left in the cache, before any launch asks for it again
    second = launch_and_check("straight after the batched rebuild", launch=False)
    assert second is not first or not ops.EAGER_REBUILD
    launch_and_check("after the raw-pointer update")


# ------------------------------------------------------------------ one period of the MPD against the CPU oracle
def test_mpd_period_against_oracle(tap_route_rows):
    """the period-2 sub-discriminator (stride-1 fifth layer) at the shapes of tests/test_hip_disc_autograd.py: score,
    feature maps, input gradient and every parameter gradient against the oracle at that file's tolerance; the route
    counts the fifth layer's forward and its data gradient (and the two-tap residues of the layer below), and
    nothing when it is off"""
    ops = tap_route_rows
    r = subdisc_against_oracle(ops, "mpd", ("FP16X3_TAP_LAUNCHES",), "mpd period 2, fp16x3 tap route")
    print(f"[h3p] period {r.sub.period}: {r.fwd[0]} forward and {r.bwd[0]} backward launches on the route")
    assert r.fwd[0] >= 1, "the fifth layer's forward never reached the kernel"
    assert r.bwd[0] >= 1, "the fifth layer's data gradient never reached the kernel"
    ops.FP16X3_TAP_MIN_ROWS = ops.FP16X3_TAP_OFF
    assert r.rerun() == ((0,), (0,))
