"""fp16x3 over STRIDE-3 windows of five positions of a halo map on the GPU (csrc/gemm_f16p3.hip, gemm_h3p3_kernel):
against float64 over poisoned operands and guarded outputs with the helpers of tests/fp16x3_gpu.py (which
take the window stride and the extra positions behind a sequence's last window) and tests/test_hip_gemm_routes.py,
the descriptors it must decline, the ops.gemm route with its tunable and counter, the cached weight image following
its weight, and one period of the MPD against the CPU oracle.

Tolerance, per element, as tests/test_hip_gemm_f16_tap.py: 1.8e-6 * (|A| |B|^T + |epilogue terms|) plus the floor term
of the per-sequence scale, 2^-28 amax_seq(row) sum_k |w[n,k]|, carried through the epilogue like a product's scale.

The kernel stages only the positions some window reads, so the distance between two sequences costs it nothing: its
staging bound is 130 + 126 / P0 <= 144 entries per residue plane (a group's 128 rows, one entry more per sequence they
touch, one for the taps' overhang).  The descriptor that breaks it has P0 = 8; a map with 40 unread positions behind
every sequence is accepted and computed (test_distance_between_sequences_is_free)."""
import ctypes as C

import pytest
import torch

import fp16x3_seq3_emul as emul
from fp16x3_gpu import (EINVAL, TOL, any_grid, assert_declined, case, f16_ok, fp16x3_mode, image_follows_weight, ops,
                        ran, same_bits, subdisc_against_oracle)
from test_hip_gemm_routes import DEV, NAN, SENT, Out, Vec, check, expect, last_kernel, make_desc, rnd

pytestmark = pytest.mark.gpu

STEP, TAPS = 3, 5
NAME = "h3p<taps=5,step=3>"
SHAPES = [(3, 100, 128, 128, 2),     # 300 rows: one full 256-row tile and a partial one whose second group is empty
          (9, 27, 128, 160, 2),      # Hp = 85, the production period-11 geometry: a group's 128 rows straddle five
                                     # sequences; a partial column tile
          (4, 70, 256, 128, 4)]      # eight channel slabs, the largest seam


@pytest.fixture
def tap3_route(ops, any_grid):
    """the fp16x3 mode as shipped, with FP16X3_TAP3_MIN_ROWS = 1 and the library option x6p = 2"""
    with fp16x3_mode(ops, "FP16X3_TAP3_MIN_ROWS"):
        ops.FP16X3_TAP3_MIN_ROWS = 1
        yield ops


_CASES = {}


def shared_case(ops, i):
    """the operands, images and float64 products of SHAPES[i], made once (nothing below writes them)"""
    if i not in _CASES:
        S, P0, Cc, N, extra = SHAPES[i]
        _CASES[i] = case(ops, S, P0, Cc, N, TAPS, seed=S + N, step=STEP, extra=extra)
    return _CASES[i]


def halo_rowmap(P0, ld):
    return (P0, (P0 + 4) * ld, ld, 2 * ld)


# ------------------------------------------------------------------ GEMM against float64
def forward_check(ops, c, P0, N):
    bias = rnd(N, seed=1) * 1e-3
    out = Out(c.M, N, rowmap=halo_rowmap(P0, N + 8))
    d = make_desc(ops, c.A, c.B, out, precision=4, bias=bias, lrelu=0.1)
    assert f16_ok(ops, d) == 1
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    assert ran(ops, NAME)
    out.guards_ok()
    want, m, _, _ = expect(c.acc, c.mag, bias=bias, lrelu=0.1)
    check(out.got(), want, m, TOL, "forward")
    return d


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_forward_epilogue_against_float64(ops, any_grid, i):
    """bias + leaky ReLU + halo row map (the forward's epilogue)"""
    S, P0, Cc, N, extra = SHAPES[i]
    c = shared_case(ops, i)
    d = forward_check(ops, c, P0, N)
    # the same descriptor over the fp32 operands: "would run once both are replaced by their images"
    d.A.base, d.A.split, d.A.rscale = c.A.flat.data_ptr() + 4 * c.A.off, 0, None
    d.B.base, d.B.split, d.B.rscale = c.B.flat.data_ptr() + 4 * c.B.off, 0, None
    assert f16_ok(ops, d) == 2
    assert ops.L.lib.f2g_gemm(C.byref(d), ops.L.stream_ptr()) == EINVAL


def test_distance_between_sequences_is_free(ops, any_grid):
    """40 positions no window reads behind every sequence's last window: accepted, and the same arithmetic"""
    S, P0, Cc, N, _ = SHAPES[0]
    forward_check(ops, case(ops, S, P0, Cc, N, TAPS, seed=11, step=STEP, extra=40), P0, N)


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_column_sums_mask_and_feature_matching_against_float64(ops, any_grid, i):
    """row map + leaky-ReLU backward mask + feature-matching term + column sums: the sums once by atomics, once as
    partial rows"""
    S, P0, Cc, N, extra = SHAPES[i]
    c = shared_case(ops, i)
    rowmap = halo_rowmap(P0, N + 8)
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
    assert ran(ops, NAME)
    out.guards_ok()
    yy, rr = y_full[out.offs].double(), ref_full[out.offs].double()
    v = c.acc + fmw * 0.5 * torch.sign(yy - rr)
    m = c.mag + fmw * 0.5
    mult = torch.where(yy > 0, torch.ones_like(yy), torch.full_like(yy, 0.1))
    v, m = v * mult, m * mult
    check(out.got(), v, m, TOL, "masked output")
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


def test_x3_out_of_the_row_mapped_forward(ops, any_grid):
    """the production use of E.x3_out: a forward landing in a halo map through the row map -- the image of the whole
    contiguous map (zero halo rows included, as x3_reserve leaves them) equals a fresh x3_flat_image of it, and the
    halo rows stay untouched"""
    S, P0, Cc, N, extra = SHAPES[1]
    c = shared_case(ops, 1)
    Hp, guard = P0 + 4, 64
    flat = torch.full((guard + S * Hp * N + guard,), SENT, device=DEV)
    body = flat[guard:guard + S * Hp * N].view(S, Hp, N)
    body[:] = NAN
    body[:, :2] = 0.0
    body[:, Hp - 2:] = 0.0
    img = torch.full((guard + S * Hp * N * 3 + guard,), 1.0, device=DEV, dtype=torch.bfloat16)
    img[guard:guard + S * Hp * N * 3] = 0.0
    bias = rnd(N, seed=2) * 1e-3
    d = make_desc(ops, c.A, c.B, Out(c.M, N), precision=4, bias=bias, lrelu=0.1)
    d.E.C, d.E.ldc = flat.data_ptr() + 4 * guard, N
    d.E.P0o, d.E.seq_stride_o, d.E.row_stride_o, d.E.off_o = halo_rowmap(P0, N)
    d.E.x3_out = img.data_ptr() + 2 * guard
    assert f16_ok(ops, d) == 1
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    assert last_kernel(ops) == NAME
    assert bool((flat[:guard] == SENT).all()) and bool((flat[guard + S * Hp * N:] == SENT).all())
    assert bool((img[:guard] == 1.0).all()) and bool((img[guard + S * Hp * N * 3:] == 1.0).all())
    assert bool((body[:, :2] == 0).all()) and bool((body[:, Hp - 2:] == 0).all()), "a halo row was written"
    want, m, _, _ = expect(c.acc, c.mag, bias=bias, lrelu=0.1)
    check(body[:, 2:2 + P0].reshape(c.M, N).double(), want, m, TOL, "row-mapped forward")
    image = ops.x3_flat_image(body.reshape(-1).clone())
    torch.cuda.synchronize()
    assert torch.equal(img[guard:guard + S * Hp * N * 3].view(torch.int16), image.view(torch.int16))


def test_three_launches_give_the_same_bits(ops, any_grid):
    c = shared_case(ops, 1)

    def go():
        out = Out(c.M, c.N)
        d = make_desc(ops, c.A, c.B, out, precision=4)
        ops.call("f2g_gemm", C.byref(d))
        torch.cuda.synchronize()
        assert last_kernel(ops) == NAME
        return out.flat.view(torch.int32).clone()

    same_bits(go)


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("what", ["step2", "taps2", "staged", "no_scales", "pad0", "grid"])
def test_descriptors_the_kernel_declines(ops, lib_option, what):
    """f2g_gemm_f16_ok == 0 and F2G_EINVAL from f2g_gemm -- never another kernel; the output stays untouched"""
    lib_option("x6p", 1 if what == "grid" else 2)      # ("grid": the default option keeps small grids off the kernel)
    S, P0, Cc, N, extra = SHAPES[0]
    if what == "staged":        # 40 sequences of 8 windows: 130 + 126 / 8 = 145 entries per plane, one too many
        S, P0 = 40, 8
    kw = dict(taps=2 if what == "taps2" else TAPS, step=2 if what == "step2" else STEP, extra=extra)
    c = case(ops, S, P0, Cc, N, **kw)
    out = Out(c.M, N)
    d = make_desc(ops, c.A, c.B, out, precision=4)
    if what == "no_scales":
        d.A.rscale = None
    if what == "pad0":
        d.A.pad0 = 1
    assert_declined(ops, d, out)


# ------------------------------------------------------------------ ops.gemm
def ops_case(ops, seed):
    S, P0, Cc, N, extra = SHAPES[0]
    Hp = STEP * (P0 - 1) + TAPS + extra
    x = rnd(S, Hp, Cc, seed=seed) * torch.logspace(-3, 3, S, device=DEV)[:, None, None]
    flat = torch.full((S * Hp * Cc + 256 * Cc,), NAN, device=DEV)
    flat[:S * Hp * Cc] = x.reshape(-1)
    a = emul.windows(x, P0, TAPS, STEP).double()
    amax = x.double().abs().reshape(S, -1).amax(1).repeat_interleave(P0)
    return flat, a, amax, (S, Hp, Cc, P0, N)


def test_ops_gemm_takes_the_route_and_counts_it(tap3_route):
    ops = tap3_route
    flat, a, amax, (S, Hp, Cc, P0, N) = ops_case(ops, 3)
    w, bias = torch.nn.Parameter(rnd(N, TAPS * Cc, seed=7, scale=0.1)), rnd(N, seed=8)
    out = torch.full((S * P0, N), NAN, device=DEV)

    def go():
        ops.gemm(ops.win1d(flat, S, Hp, Cc, P0, STEP, 0, TAPS), ops.mat(w), out, bias=bias, lrelu=0.1)
        torch.cuda.synchronize()

    n0, t0 = ops.FP16X3_TAP3_LAUNCHES, ops.FP16X3_TAP_LAUNCHES
    go()
    assert ops.FP16X3_TAP3_LAUNCHES == n0 + 1 and last_kernel(ops) == NAME
    wd = w.detach().double()
    mag = a.abs() @ wd.abs().t() + emul.FLOOR * amax[:, None] * wd.abs().sum(1)[None, :] / TOL
    want, m, _, _ = expect(a @ wd.t(), mag, bias=bias, lrelu=0.1)
    check(out.double(), want, m, TOL, "ops.gemm")
    # below the threshold, with the route off, and in the plain bf16x6 mode: the bf16x6 kernels
    for rows in (S * P0 + 1, ops.FP16X3_TAP_OFF):
        ops.FP16X3_TAP3_MIN_ROWS = rows
        go()
        assert ops.FP16X3_TAP3_LAUNCHES == n0 + 1 and not last_kernel(ops).startswith("h3p")
    ops.FP16X3_TAP3_MIN_ROWS = S * P0
    go()
    assert ops.FP16X3_TAP3_LAUNCHES == n0 + 2 and last_kernel(ops) == NAME
    ops.set_gemm_precision("bf16x6")
    go()
    assert ops.FP16X3_TAP3_LAUNCHES == n0 + 2 and not last_kernel(ops).startswith("h3p")
    assert ops.FP16X3_TAP_LAUNCHES == t0        # (the stride-1 route never saw these windows)


def test_weight_images_follow_their_weights(tap3_route):
    """after a raw-pointer update (the optimizer's way: bump_weight_epoch + the batched rebuild_derived) and after
    an autograd-visible in-place update, the next launch reads a rebuilt image and rebuilt scales"""
    ops = tap3_route
    flat, a, amax, (S, Hp, Cc, P0, N) = ops_case(ops, 5)
    w = torch.nn.Parameter(rnd(N, TAPS * Cc, seed=2))
    out = torch.empty(S * P0, N, device=DEV)

    def launch_and_check(what):
        n0 = ops.FP16X3_TAP3_LAUNCHES
        ops.gemm(ops.win1d(flat, S, Hp, Cc, P0, STEP, 0, TAPS), ops.mat(w), out)
        assert ops.FP16X3_TAP3_LAUNCHES == n0 + 1 and last_kernel(ops) == NAME
        wd = w.detach().double()
        mag = a.abs() @ wd.abs().t() + emul.FLOOR * amax[:, None] * wd.abs().sum(1)[None, :] / TOL
        check(out.double(), a @ wd.t(), mag, TOL, what)
        buf = ops._f16_seq_operand(ops.mat(w))._keep[0]
        torch.cuda.synchronize()
        K = TAPS * Cc
        img, rs = buf[:N * K].cpu().view(torch.int32).view(N, K), buf[N * K:N * K + N].cpu()
        want_img, want_rs = emul.image(w.detach().cpu())
        assert torch.equal(img, want_img) and torch.equal(rs, want_rs), f"{what}: the cached image is stale"
        return out.clone()

    image_follows_weight(ops, w, launch_and_check)


# ------------------------------------------------------------------ one period of the MPD against the CPU oracle
def test_mpd_period_against_oracle(tap3_route):
    """the period-2 sub-discriminator at the shapes of tests/test_hip_disc_autograd.py (its 128 -> 512 and 512 -> 1024
    layers run 112 and 38 windows per sequence): score, feature maps, input gradient and every parameter gradient
    against the oracle at that file's tolerance; the route counts one forward launch per stride-3 layer with 128 and
    512 input channels, and nothing when it is off"""
    ops = tap3_route
    r = subdisc_against_oracle(ops, "mpd", ("FP16X3_TAP3_LAUNCHES",), "mpd period 2, fp16x3 stride-3 tap route")
    print(f"[h3p3] period {r.sub.period}: {r.fwd[0]} forward launches on the route")
    assert r.fwd[0] >= 2, "a stride-3 layer's forward never reached the kernel"
    ops.FP16X3_TAP3_MIN_ROWS = ops.FP16X3_TAP_OFF
    assert r.rerun()[0] == (0,)
