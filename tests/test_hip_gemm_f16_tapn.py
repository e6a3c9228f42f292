"""fp16x3 over STRIDE-1 windows of two or one positions of a 128-channel halo map onto at most 32 columns, scaled per
sequence segment INSIDE the kernel (csrc/gemm_f16pn.hip, gemm_h3pn_kernel<2 / 1>; f2g_operand.split = 8): against
float64 over poisoned operands and guarded outputs with the helpers of tests/fp16x3_gpu.py and
tests/test_hip_gemm_routes.py, the descriptors it must decline, the ops.gemm route with its tunable and counter, the
cached weight image following its weight, and one period of the MPD against the CPU oracle.

The A operand is the fp32 map itself: no image, no rscale.  Everything no window of a valid row reads -- the positions
in front of a sequence's first window, the positions behind its last, the buffer behind the last sequence -- is NaN:
one of them entering a segment's maximum or the LDS would show in every output of that segment.

Tolerance, per element, as tests/test_hip_gemm_f16_tap.py: 1.8e-6 * (|A| |B|^T + |epilogue terms|) plus the floor term
2^-28 amax_seq(row) sum_k |w[n,k]| carried through the epilogue like a product's scale; a segment's maximum is at most
its sequence's, so the per-sequence floor bounds the per-segment one (tests/fp16x3_seg1_emul.py has the exact bound)."""
import ctypes as C

import pytest
import torch

import fp16x3_seq_emul as emul
from fp16x3_gpu import (EINVAL, TOL, any_grid, assert_declined, case, f16_ok, fp16x3_mode, image_follows_weight, ops,
                        ran, same_bits, seq_image, subdisc_against_oracle, watching_gemm_calls)
from test_hip_gemm_routes import DEV, NAN, Out, Vec, check, expect, last_kernel, make_desc, products, rnd

pytestmark = pytest.mark.gpu

CC = 128
SHAPES = [(3, 100, 32, 0, 0),        # 300 rows: two full 128-row tiles and a partial one; two segments per tile
          (9, 27, 24, 2, 0),         # a tile's rows straddle five or six sequences; N < 32
          (40, 8, 32, 0, 0),         # the most segments per tile the host rule admits
          (5, 64, 32, 3, 2),         # pad0 = -2, as production hands it: two halo positions in front of the windows
          (70, 1000, 32, 0, 0)]      # 547 row tiles: more than the 512 blocks of the persistent walk
SMALL = range(len(SHAPES) - 1)


def name_of(taps):
    return f"h3pn<taps={taps}>"


@pytest.fixture
def tapn_route(ops, any_grid):
    """the fp16x3 mode as shipped, with FP16X3_TAPN_MIN_ROWS = 1, the library option x6p = 2, and the bf16x6 rule for
    tall 32-column GEMMs (gemm_x6n_kernel) lowered to the test's row counts"""
    with fp16x3_mode(ops, "FP16X3_TAPN_MIN_ROWS", "X6F_TALL_ROWS"):
        ops.FP16X3_TAPN_MIN_ROWS = 1
        ops.X6F_TALL_ROWS = 1024
        yield ops


def seg_case(ops, S, P0, N, taps, seed=0, extra=0, front=0, Cc=CC, step=1):
    """case() of tests/fp16x3_gpu.py with A left the fp32 map and marked split = 8, the windows `front`
    positions into their sequences (pad0 = -front), the positions no window reads poisoned, and B replaced by its
    f2g_split_f16x2_seq image"""
    c = case(ops, S, P0, Cc, N, taps, seed=seed, step=step, extra=extra + front, images=False)
    if front:
        c.A.o.pad0 = -front
        amax = c.x.double().abs().reshape(S, -1).amax(1).repeat_interleave(P0)
        floor = emul.FLOOR * amax[:, None] * c.w.double().abs().sum(1)[None, :]
        c.acc, mag = products(c.A, c.B, 0, False)
        c.mag = mag + floor / TOL
    view = c.A.flat[:S * c.Hp * Cc].view(S, c.Hp, Cc)          # (the float64 products are made already)
    view[:, :front] = NAN
    view[:, front + step * (P0 - 1) + taps:] = NAN
    c.A.o.split = 8
    seq_image(ops, c.B, N, taps * Cc, c.B.o.seq_stride)
    return c


_CASES = {}


def shared_case(ops, i, taps):
    """the operands, the weight image and the float64 products of SHAPES[i], made once (nothing below writes them)"""
    if (i, taps) not in _CASES:
        S, P0, N, extra, front = SHAPES[i]
        _CASES[i, taps] = seg_case(ops, S, P0, N, taps, seed=S + N, extra=extra, front=front)
    return _CASES[i, taps]


def residue_rowmap(P0, ld):
    """rows of stride residue 1 of a halo map of 3 P0 rows (+ 2 halo rows either side), `ld` floats per row"""
    return (P0, (3 * P0 + 4) * ld, 3 * ld, (2 + 1) * ld)


# ------------------------------------------------------------------ GEMM against float64
@pytest.mark.parametrize("taps", [2, 1])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_bias_and_leaky_relu_through_a_stride_3_row_map(ops, any_grid, i, taps):
    """bias + leaky ReLU into every third row of a halo map whose other rows -- the halo rows, the other residues' --
    stay untouched; then the same descriptor with B left fp32"""
    S, P0, N, extra, front = SHAPES[i]
    c = shared_case(ops, i, taps)
    bias = rnd(N, seed=1) * 1e-3
    out = Out(c.M, N, rowmap=residue_rowmap(P0, N + 8))
    d = make_desc(ops, c.A, c.B, out, precision=4, bias=bias, lrelu=0.1)
    assert d.A.split == 8 and not d.A.rscale and d.A.pad0 == -front
    assert f16_ok(ops, d) == 1
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    assert ran(ops, name_of(taps))
    out.guards_ok()
    want, m, _, _ = expect(c.acc, c.mag, bias=bias, lrelu=0.1)
    check(out.got(), want, m, TOL, "forward")
    d.B.base, d.B.split, d.B.rscale = c.B.flat.data_ptr() + 4 * c.B.off, 0, None
    assert f16_ok(ops, d) == 2          # "would run once B is replaced by its image"
    assert ops.L.lib.f2g_gemm(C.byref(d), ops.L.stream_ptr()) == EINVAL


@pytest.mark.parametrize("taps", [2, 1])
@pytest.mark.parametrize("i", SMALL)
def test_mask_feature_matching_and_column_sums_against_float64(ops, any_grid, i, taps):
    """row map + leaky-ReLU backward mask + feature-matching term + column sums (by atomics: the kernel writes no
    partial rows, and a descriptor that asks for them is refused)"""
    S, P0, N, extra, front = SHAPES[i]
    c = shared_case(ops, i, taps)
    out = Out(c.M, N, rowmap=residue_rowmap(P0, N + 8))
    y_full, ref_full = rnd(out.flat.numel(), seed=3), rnd(out.flat.numel(), seed=4)
    wdev = torch.tensor([0.5], device=DEV)
    fmw = 0.3 * 1e-3
    cs = Vec(N, 5)
    d = make_desc(ops, c.A, c.B, out, precision=4, colsum=cs)
    d.E.mask_src, d.E.mask_slope = y_full.data_ptr() + 4 * out.base, 0.1
    d.E.fm_ref, d.E.fm_w, d.E.fm_wdev = ref_full.data_ptr() + 4 * out.base, fmw, wdev.data_ptr()
    assert f16_ok(ops, d) == 1
    assert ops.L.lib.f2g_gemm_colsum_part_rows(C.byref(d)) == 0
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    assert ran(ops, name_of(taps))
    out.guards_ok()
    yy, rr = y_full[out.offs].double(), ref_full[out.offs].double()
    v = c.acc + fmw * 0.5 * torch.sign(yy - rr)
    m = c.mag + fmw * 0.5
    mult = torch.where(yy > 0, torch.ones_like(yy), torch.full_like(yy, 0.1))
    v, m = v * mult, m * mult
    check(out.got(), v, m, TOL, "masked gradient")
    check(cs.got(), cs.init.double() + v.sum(0), cs.init.double().abs() + m.sum(0), TOL, "colsum")
    before = out.flat.clone()
    d.E.colsum_part_ld = N
    assert f16_ok(ops, d) == 0
    assert ops.L.lib.f2g_gemm(C.byref(d), ops.L.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(out.flat.view(torch.int32), before.view(torch.int32))


@pytest.mark.parametrize("taps", [2, 1])
@pytest.mark.parametrize("i", [1, 2])
def test_three_launches_give_the_same_bits(ops, any_grid, i, taps):
    c = shared_case(ops, i, taps)

    def go():
        out = Out(c.M, c.N)
        d = make_desc(ops, c.A, c.B, out, precision=4)
        ops.call("f2g_gemm", C.byref(d))
        torch.cuda.synchronize()
        assert last_kernel(ops) == name_of(taps)
        return out.flat.view(torch.int32).clone()

    same_bits(go)


@pytest.mark.parametrize("taps", [2, 1])
def test_an_inf_stays_in_its_own_sequence(ops, any_grid, taps):
    """an inf in sequence 4 of nine (rows 108 .. 134: two segments, either side of a tile boundary) sets the scale of
    the segment that reads it to 1 and makes rows of that sequence non-finite; every other sequence's rows stay within
    tolerance"""
    S, P0, N = 9, 27, 32
    c = seg_case(ops, S, P0, N, taps, seed=21)
    c.A.flat[:S * c.Hp * CC].view(S, c.Hp, CC)[4, 10, 77] = float("inf")
    out = Out(c.M, N)
    d = make_desc(ops, c.A, c.B, out, precision=4)
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    assert last_kernel(ops) == name_of(taps)
    out.guards_ok()
    clean = torch.ones(c.M, dtype=torch.bool, device=DEV)
    clean[4 * P0:5 * P0] = False
    got = out.got()
    check(got[clean], c.acc[clean], c.mag[clean], TOL, "the other sequences")
    assert not bool(torch.isfinite(got[4 * P0 + 10]).all())


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("what", ["unit64", "step2", "taps3", "N=40", "P0=4", "pad0=1", "misaligned", "grid", "x3_out",
                                  "unmarked"])
def test_descriptors_the_kernel_declines(ops, lib_option, what):
    """f2g_gemm_f16_ok == 0 and F2G_EINVAL from f2g_gemm -- never another kernel; the output stays untouched"""
    lib_option("x6p", 1 if what == "grid" else 2)      # ("grid": the default option keeps small grids off the kernel)
    S, P0, N = (75, 4, 32) if what == "P0=4" else (3, 100, 40 if what == "N=40" else 32)
    c = seg_case(ops, S, P0, N, 3 if what == "taps3" else 2, Cc=64 if what == "unit64" else CC,
                 step=2 if what == "step2" else 1)
    out = Out(c.M, N)
    d = make_desc(ops, c.A, c.B, out, precision=4)
    if what == "pad0=1":
        d.A.pad0 = 1
    if what == "misaligned":
        d.A.base += 4
    if what == "x3_out":
        image = torch.zeros(4096, device=DEV, dtype=torch.bfloat16)     # (never written: the launch is refused)
        d.E.x3_out = image.data_ptr()
    if what == "unmarked":
        # A.split == 0 beside B's image: the stride-1 image kernel's candidate, which asks for images of both
        d.A.split = 0
    assert_declined(ops, d, out)


# ------------------------------------------------------------------ ops.gemm
def ops_case(ops, taps, seed, front=2):
    """the residue data gradient as fused_disc._conv1d_dgrad hands it: windows `front` positions into the sequences
    of a contiguous map (S, Hp, 128), a stride-3 row map into a 32-channel halo map"""
    S, P0, N = 12, 100, 32
    Hp = front + P0 + taps - 1
    x = rnd(S, Hp, CC, seed=seed) * torch.logspace(-3, 3, S, device=DEV)[:, None, None]
    x[:, :front] = 0.0      # (halo rows: zero in the MPD maps -- the route's Python side asks for an initialised buffer)
    flat = torch.full((S * Hp * CC + 256 * CC,), NAN, device=DEV)
    flat[:S * Hp * CC] = x.reshape(-1)
    a = torch.stack([x[:, front + t:front + t + P0] for t in range(taps)], 2).reshape(S * P0, taps * CC).double()
    amax = x.double().abs().reshape(S, -1).amax(1).repeat_interleave(P0)
    return flat, a, amax, (S, Hp, P0, N, front)


def halo_out(S, P0, N):
    """a zeroed 32-channel halo map of 3 P0 rows per sequence and the offsets residue 1's rows land on"""
    Hx = 3 * P0 + 4
    gx = torch.zeros(S * Hx, N, device=DEV)
    rm = (P0, Hx * N, 3 * N, 3 * N)
    rows = (torch.arange(S, device=DEV)[:, None] * Hx + 3 + 3 * torch.arange(P0, device=DEV)[None, :]).reshape(-1)
    return gx, rm, rows


@pytest.mark.parametrize("taps", [2, 1])
def test_ops_gemm_takes_the_route_and_counts_it(tapn_route, monkeypatch, taps):
    ops = tapn_route
    flat, a, amax, (S, Hp, P0, N, front) = ops_case(ops, taps, 3)
    w = torch.nn.Parameter(rnd(N, taps * CC, seed=7, scale=0.1))
    gx, rm, rows = halo_out(S, P0, N)
    ops._f16_seq_operand(ops.mat(w))        # (the weight's cached image: built before the launches are watched)
    def go():
        gx.zero_()
        ops.gemm(ops.win1d(flat, S, Hp, CC, P0, 1, -front, taps), ops.mat(w), gx, rowmap=rm)
        torch.cuda.synchronize()

    n0, t0, t3 = ops.FP16X3_TAPN_LAUNCHES, ops.FP16X3_TAP_LAUNCHES, ops.FP16X3_TAP3N_LAUNCHES
    with watching_gemm_calls(ops, monkeypatch, "split_f16_seq") as (seen, images):
        go()
    assert ops.FP16X3_TAPN_LAUNCHES == n0 + 1 and last_kernel(ops) == name_of(taps)
    # no per-call image of A: the launch reads the caller's map itself, and nothing built an image meanwhile
    assert seen == [(flat.data_ptr(), 8, False, 7, True)]
    assert images == []
    wd = w.detach().double()
    mag = a.abs() @ wd.abs().t() + emul.FLOOR * amax[:, None] * wd.abs().sum(1)[None, :] / TOL
    check(gx[rows].double(), a @ wd.t(), mag, TOL, "ops.gemm")
    others = torch.ones(gx.shape[0], dtype=torch.bool, device=DEV)
    others[rows] = False
    assert bool((gx[others] == 0).all()), "a row of another residue or a halo row was written"
    # below the threshold and with the route off: the same call lands on the bf16x6 kernel of this launch
    for nrows in (S * P0 + 1, ops.FP16X3_TAP_OFF):
        ops.FP16X3_TAPN_MIN_ROWS = nrows
        go()
        assert ops.FP16X3_TAPN_LAUNCHES == n0 + 1 and last_kernel(ops) == "x6n"
        check(gx[rows].double(), a @ wd.t(), mag, TOL, "the bf16x6 launch")
    ops.FP16X3_TAPN_MIN_ROWS = S * P0
    go()
    assert ops.FP16X3_TAPN_LAUNCHES == n0 + 2 and last_kernel(ops) == name_of(taps)
    ops.set_gemm_precision("bf16x6")
    go()
    assert ops.FP16X3_TAPN_LAUNCHES == n0 + 2 and last_kernel(ops) == "x6n"
    assert ops.FP16X3_TAP_LAUNCHES == t0 and ops.FP16X3_TAP3N_LAUNCHES == t3    # (the other tap routes never saw them)


def test_weight_images_follow_their_weights(tapn_route):
    """after a raw-pointer update (the optimizer's way: bump_weight_epoch + the batched rebuild_derived) and after
    an autograd-visible in-place update, the next launch reads a rebuilt image and rebuilt scales"""
    ops = tapn_route
    taps = 2
    flat, a, amax, (S, Hp, P0, N, front) = ops_case(ops, taps, 5)
    w = torch.nn.Parameter(rnd(N, taps * CC, seed=2))
    gx, rm, rows = halo_out(S, P0, N)

    def launch_and_check(what):
        n0 = ops.FP16X3_TAPN_LAUNCHES
        ops.gemm(ops.win1d(flat, S, Hp, CC, P0, 1, -front, taps), ops.mat(w), gx, rowmap=rm)
        assert ops.FP16X3_TAPN_LAUNCHES == n0 + 1 and last_kernel(ops) == name_of(taps)
        wd = w.detach().double()
        mag = a.abs() @ wd.abs().t() + emul.FLOOR * amax[:, None] * wd.abs().sum(1)[None, :] / TOL
        check(gx[rows].double(), a @ wd.t(), mag, TOL, what)
        buf = ops._f16_seq_operand(ops.mat(w))._keep[0]
        torch.cuda.synchronize()
        K = taps * CC
        img, rs = buf[:N * K].cpu().view(torch.int32).view(N, K), buf[N * K:N * K + N].cpu()
        want_img, want_rs = emul.image(w.detach().cpu())
        assert torch.equal(img, want_img) and torch.equal(rs, want_rs), f"{what}: the cached image is stale"
        return gx[rows].clone()

    image_follows_weight(ops, w, launch_and_check)


# ------------------------------------------------------------------ one period of the MPD against the CPU oracle
def test_mpd_period_against_oracle(tapn_route):
    """the period-2 sub-discriminator at the shapes of tests/test_hip_disc_autograd.py: score, feature maps, input
    gradient and every parameter gradient against the oracle at that file's tolerance; a backward counts three launches
    on the route (the stride residues of the 32 -> 128 layer's data gradient), a forward none, and nothing when it is
    off"""
    ops = tapn_route
    r = subdisc_against_oracle(ops, "mpd", ("FP16X3_TAPN_LAUNCHES",),
                               "mpd period 2, fp16x3 in-kernel-scaled residue data gradients")
    print(f"[h3pn] period {r.sub.period}: {r.fwd[0]} forward and {r.bwd[0]} backward launches on the route")
    assert r.fwd[0] == 0 and r.bwd[0] == 3, "the three residue data gradients of the 32 -> 128 layer"
    ops.FP16X3_TAPN_MIN_ROWS = ops.FP16X3_TAP_OFF
    assert r.rerun() == ((0,), (0,))
