"""The one-launch fp16x3 data gradient over the three stride residues of the MPD's 32 -> 128 layer (csrc/gemm_f16pn3.hip,
gemm_h3pn3_kernel; f2g_epilogue.col_fold / seq_live): against float64 per element over poisoned operands and guarded
outputs with the helpers of tests/test_hip_gemm_routes.py, tests/fp16x3_gpu.py and
tests/test_hip_gemm_f16_tapn.py, the descriptors it must decline, the route of fused_disc._conv1d_dgrad with its
tunable and counter -- off by default, where the data gradient stays the three launches bit for bit --, the cached
image of the combined weight following its weight, and one period of the MPD against the CPU oracle.

The A operand is the fp32 map itself: everything no window of a valid row reads is NaN.  The output is the 32-channel
halo map inside a sentinel buffer: the halo rows AND the elements behind seq_live -- which the last row of a sequence
computes when Hin % 3 != 0 -- must keep their sentinel.

Tolerance, per element, as tests/test_hip_gemm_f16_tapn.py: 1.8e-6 * (|A| |B|^T + |epilogue terms|) plus the floor
term 2^-28 amax_seq(row) sum_k |w[n,k]| (tests/fp16x3_res3_emul.py has the bound; nothing new)."""
import ctypes as C
import types

import pytest
import torch

import fp16x3_res3_emul as res3
import fp16x3_seq_emul as emul
from fp16x3_gpu import (EINVAL, TOL, any_grid, f16_ok, fp16x3_mode, halo_windows, image_follows_weight, mode_name, ops,
                        ran, seq_image, subdisc_against_oracle)
from fp16x3_res3_emul import REFUSALS
from test_hip_gemm_routes import DEV, NAN, SENT, Out, Vec, check, last_kernel, make_desc, plain, products, rnd

pytestmark = pytest.mark.gpu


CC, CIN, N3 = 128, 32, 96
SHAPES = [(3, 100, 300, 0),          # no cut; two full 128-row tiles and a partial one
          (3, 100, 298, 0),          # Hin % 3 = 1: 64 floats cut per sequence
          (9, 27, 80, 0),            # Hin % 3 = 2; a tile's rows straddle five or six sequences
          (40, 8, 22, 0),            # the most segments per tile the host rule admits
          (5, 64, 191, 2),           # pad0 = -2, as production hands it
          (70, 1000, 2999, 0)]       # 547 row tiles: more than the 512 blocks of the persistent walk
SMALL = range(len(SHAPES) - 1)
NAME = "h3pn3"


def fold_case(ops, S, P0, Hin, seed=0, front=0):
    """A: windows [g[q], g[q + 1]] `front` positions into the sequences of a map whose sequences span 60 decades,
    left fp32 and marked split = 8, poisoned wherever no window reads; B: a 96 x 256 weight with the kernel's zero
    block, as its f2g_split_f16x2_seq image; float64 products, their scale with the floor term, the live elements"""
    assert res3.seq_live_ok(P0, Hin)
    Hp = front + P0 + 1
    x = rnd(S, Hp, CC, seed=seed + 2) * torch.logspace(-30, 30, S, device=DEV)[:, None, None]
    w = rnd(N3, 2 * CC, seed=seed + 50, scale=(2 * CC) ** -0.5)
    w[:CIN, CC:] = 0.0
    A = halo_windows(ops, x, P0, 2)
    A.o.pad0 = -front
    B = plain(ops, w, pad=0)
    amax = x.double().abs().reshape(S, -1).amax(1).repeat_interleave(P0)
    floor = emul.FLOOR * amax[:, None] * w.double().abs().sum(1)[None, :]
    acc, mag = products(A, B, 0, False)
    view = A.flat[:S * Hp * CC].view(S, Hp, CC)
    view[:, :front] = NAN
    view[:, front + P0 + 1:] = NAN
    A.o.split = 8
    seq_image(ops, B, N3, 2 * CC, B.o.seq_stride)
    live = torch.tensor(res3.live_columns(P0, Hin), device=DEV).repeat(S)[:, None] > torch.arange(N3, device=DEV)[None]
    return types.SimpleNamespace(A=A, B=B, x=x, w=w, acc=acc, mag=mag + floor / TOL, M=S * P0, S=S, P0=P0, Hin=Hin,
                                 Hp=Hp, front=front, live=live)


_CASES = {}


def shared_case(ops, i):
    """the operands, the weight image and the float64 products of SHAPES[i], made once (nothing below writes them)"""
    if i not in _CASES:
        S, P0, Hin, front = SHAPES[i]
        _CASES[i] = fold_case(ops, S, P0, Hin, seed=S + Hin, front=front)
    return _CASES[i]


def halo_out(c):
    """the 32-channel halo map of the case inside a sentinel buffer: NaN where the launch must store, the sentinel in
    the halo rows and -- put back here -- behind seq_live"""
    out = Out(c.M, N3, rowmap=(c.P0, (c.Hin + 4) * CIN, N3, 2 * CIN))
    out.flat[out.offs[~c.live]] = SENT
    return out


def fold_desc(ops, c, out, **kw):
    d = make_desc(ops, c.A, c.B, out, precision=4, **kw)
    d.E.col_fold, d.E.seq_live = CIN, CIN * c.Hin
    return d


def check_live(c, out, want, mag, what):
    """the guard elements, the halo rows and the cut elements keep their sentinel; every live element within TOL"""
    out.guards_ok()
    flat = out.flat[out.offs]
    assert bool((flat[~c.live] == SENT).all()), f"{what}: an element behind seq_live was written"
    check(flat[c.live].double(), want[c.live], mag[c.live], TOL, what)


# ------------------------------------------------------------------ GEMM against float64
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_three_residues_in_one_launch_against_float64(ops, any_grid, i):
    c = shared_case(ops, i)
    out = halo_out(c)
    d = fold_desc(ops, c, out)
    assert d.A.split == 8 and not d.A.rscale and d.A.pad0 == -c.front
    assert f16_ok(ops, d) == 1
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    assert ran(ops, NAME)
    check_live(c, out, c.acc, c.mag, "data gradient")
    if i == 0:
        d.B.base, d.B.split, d.B.rscale = c.B.flat.data_ptr() + 4 * c.B.off, 0, None
        assert f16_ok(ops, d) == 2          # "would run once B is replaced by its image"
        assert ops.L.lib.f2g_gemm(C.byref(d), ops.L.stream_ptr()) == EINVAL


@pytest.mark.parametrize("i", SMALL)
def test_mask_feature_matching_and_folded_column_sums_against_float64(ops, any_grid, i):
    """leaky-ReLU backward mask + feature-matching term at the output's own address, and the 32 column sums over all
    three residue groups of the live elements (by atomics, at the tolerance gemm_h3pn_kernel's sums have)"""
    c = shared_case(ops, i)
    out = halo_out(c)
    y_full, ref_full = rnd(out.flat.numel(), seed=3), rnd(out.flat.numel(), seed=4)
    wdev = torch.tensor([0.5], device=DEV)
    fmw = 0.3 * 1e-3
    cs = Vec(CIN, 5)
    d = fold_desc(ops, c, out, colsum=cs)
    d.E.mask_src, d.E.mask_slope = y_full.data_ptr() + 4 * out.base, 0.1
    d.E.fm_ref, d.E.fm_w, d.E.fm_wdev = ref_full.data_ptr() + 4 * out.base, fmw, wdev.data_ptr()
    assert f16_ok(ops, d) == 1
    assert ops.L.lib.f2g_gemm_colsum_part_rows(C.byref(d)) == 0
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    assert last_kernel(ops) == NAME
    yy, rr = y_full[out.offs].double(), ref_full[out.offs].double()
    v = c.acc + fmw * 0.5 * torch.sign(yy - rr)
    m = c.mag + fmw * 0.5
    mult = torch.where(yy > 0, torch.ones_like(yy), torch.full_like(yy, 0.1))
    v, m = v * mult, m * mult
    check_live(c, out, v, m, "masked gradient")
    zero = torch.zeros_like(v)
    vs = torch.where(c.live, v, zero).view(c.M, 3, CIN).sum((0, 1))
    ms = torch.where(c.live, m, zero).view(c.M, 3, CIN).sum((0, 1))
    check(cs.got(), cs.init.double() + vs, cs.init.double().abs() + ms, TOL, "folded colsum")


@pytest.mark.parametrize("i", [1, 2])
def test_two_launches_give_the_same_bits(ops, any_grid, i):
    c = shared_case(ops, i)
    bits = []
    for _ in range(2):
        out = halo_out(c)
        d = fold_desc(ops, c, out)
        ops.call("f2g_gemm", C.byref(d))
        torch.cuda.synchronize()
        assert last_kernel(ops) == NAME
        bits.append(out.flat.view(torch.int32).clone())
    assert torch.equal(bits[0], bits[1])


def test_an_inf_stays_in_its_own_sequence(ops, any_grid):
    """an inf in sequence 4 of nine (rows 108 .. 134: two segments, either side of a tile boundary) makes rows of that
    sequence non-finite -- in all three residue groups -- and of no other"""
    S, P0, Hin = 9, 27, 80
    c = fold_case(ops, S, P0, Hin, seed=21)
    c.A.flat[:S * c.Hp * CC].view(S, c.Hp, CC)[4, 10, 77] = float("inf")
    out = halo_out(c)
    ops.call("f2g_gemm", C.byref(fold_desc(ops, c, out)))
    torch.cuda.synchronize()
    assert last_kernel(ops) == NAME
    out.guards_ok()
    clean = c.live.clone()
    clean[4 * P0:5 * P0] = False
    got = out.flat[out.offs]
    check(got[clean].double(), c.acc[clean], c.mag[clean], TOL, "the other sequences")
    row = got[4 * P0 + 10]
    assert all(not bool(torch.isfinite(row[g * CIN:(g + 1) * CIN]).all()) for g in range(3))


# ------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def refusal_case(ops):
    return fold_case(ops, 3, 100, 299, seed=31)


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_descriptors_the_kernel_declines(ops, any_grid, refusal_case, what):
    """f2g_gemm_f16_ok == 0 and F2G_EINVAL from f2g_gemm -- never another kernel; the output stays untouched"""
    c = refusal_case
    out = halo_out(c)
    before = out.flat.clone()
    d = fold_desc(ops, c, out)
    assert f16_ok(ops, d) == 1
    REFUSALS[what](before.data_ptr())(d)        # (a valid device pointer; the launch is refused, nothing reads it)
    assert f16_ok(ops, d) == 0
    assert ops.L.lib.f2g_gemm(C.byref(d), ops.L.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert last_kernel(ops) == ""
    assert torch.equal(out.flat.view(torch.int32), before.view(torch.int32))


def test_the_fields_are_refused_at_every_other_precision(ops):
    """two plain fp32 matrices, which the exact-fp32 kernels run: with col_fold or seq_live set the launch is
    F2G_EINVAL at every precision but 4 (and at 4, above: unless it is the kernel's own shape)"""
    A, B = plain(ops, rnd(64, 128, seed=1)), plain(ops, rnd(32, 128, seed=2))
    for precision in (0, 1, 2, 3):
        for fold, live in ((32, 0), (0, 64)):
            out = Out(64, 32)
            d = make_desc(ops, A, B, out, precision=precision)
            d.E.col_fold, d.E.seq_live = fold, live
            assert ops.L.lib.f2g_gemm(C.byref(d), ops.L.stream_ptr()) == EINVAL
            assert b"never run elsewhere" in ops.L.lib.f2g_last_error()
            torch.cuda.synchronize()
            assert last_kernel(ops) == "" and bool((out.flat[~torch.isnan(out.flat)] == SENT).all())
    d = make_desc(ops, A, B, out, precision=0)
    assert ops.L.lib.f2g_gemm(C.byref(d), ops.L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert last_kernel(ops) != ""


# ------------------------------------------------------------------ fused_disc._conv1d_dgrad
@pytest.fixture
def tapn3_route(ops, any_grid):
    """the fp16x3 mode as shipped, with FP16X3_TAPN3_MIN_ROWS = 1 and the library option x6p = 2"""
    with fp16x3_mode(ops, "FP16X3_TAPN3_MIN_ROWS"):
        ops.FP16X3_TAPN3_MIN_ROWS = 1
        yield ops


def layer_case(S, Hin, seed):
    """the 32 -> 128 layer's data gradient as the backward walk hands it: g_pre (S, Hout + 4, 128) with zero halo
    rows and sequence magnitudes over six decades, the conv weight as a parameter, the activation the gradient lands on"""
    from flow2gan_amd.fused_disc import HALO
    Hout = -(-Hin // 3)
    g = rnd(S, Hout, CC, seed=seed) * torch.logspace(-3, 3, S, device=DEV)[:, None, None]
    g_pre = torch.zeros(S, Hout + 2 * HALO, CC, device=DEV)
    g_pre[:, HALO:HALO + Hout] = g
    w = torch.nn.Parameter(rnd(CC, CIN, 5, 1, seed=seed + 1, scale=(5 * CIN) ** -0.5))
    y = rnd(S * (Hin + 2 * HALO), CIN, seed=seed + 2)
    return g, g_pre.view(-1, CC), w, y, Hout


def dgrad(FD, c, S, Hin, colsum=None):
    g, g_pre, w, y, Hout = c
    return FD._conv1d_dgrad(g_pre, S, Hout, CC, w, 3, 2, Hin, mask=(y, 0, 0.1), colsum=colsum)


def float64_dgrad(c, S, Hin):
    """(masked data gradient in the halo layout (S, Hin, 32), its scale with the floor term, both float64) through
    torch.autograd of F.conv2d on the CPU"""
    from flow2gan_amd.fused_disc import HALO
    g, _, w, y, Hout = c
    gd, wd = g.double().cpu(), w.detach().double().cpu()
    want = res3.autograd_dgrad(gd, wd, Hin)
    mag = res3.autograd_dgrad(gd.abs(), wd.abs(), Hin)
    wsum = res3.combined_weight(wd.abs()).sum(1).view(3, CIN)
    hres = torch.arange(Hin) % 3
    mag = mag + emul.FLOOR * gd.abs().amax((1, 2))[:, None, None] * wsum[hres][None] / TOL
    yy = y.view(S, Hin + 2 * HALO, CIN)[:, HALO:HALO + Hin].double().cpu()
    mult = torch.where(yy > 0, torch.ones_like(yy), torch.full_like(yy, 0.1))
    return (want * mult).to(DEV), (mag * mult).to(DEV)


@pytest.mark.parametrize("mode", ["bf16x6", "fp16x3"])
def test_default_off_the_data_gradient_is_the_three_launches_bit_for_bit(ops, mode):
    """the tunable at its default: fused_disc._conv1d_dgrad issues the residue launches of the loop it always had --
    restated here call by call --, the results agree bit for bit, and the counter stays 0"""
    from flow2gan_amd import fused_disc as FD
    assert ops.FP16X3_TAPN3_MIN_ROWS == ops.FP16X3_TAP_OFF
    S, Hin = 12, 299
    c = layer_case(S, Hin, 3)
    g, g_pre, w, y, Hout = c
    was = mode_name(ops)
    ops.set_gemm_precision(mode)
    try:
        n0 = ops.FP16X3_TAPN3_LAUNCHES
        got = dgrad(FD, c, S, Hin)
        gx = FD._halo_rows(S, Hin, CIN, g_pre.device)
        for rho, j0, nt, e0, Lq in FD._residues(5, 3, 2, Hin):
            A = ops.win1d(g_pre, S, Hout + 2 * FD.HALO, CC, Lq, 1, (nt - 1) - e0 - FD.HALO, nt)
            rm = (Lq, (Hin + 2 * FD.HALO) * CIN, 3 * CIN, (FD.HALO + rho) * CIN)
            ops.gemm(A, ops.mat(FD._dgrad_weight(w, 3, j0, nt)), gx, rowmap=rm, mask=(y, 0, 0.1))
            assert last_kernel(ops) != NAME
        torch.cuda.synchronize()
        assert ops.FP16X3_TAPN3_LAUNCHES == n0
        assert torch.equal(got.view(torch.int32), gx.view(torch.int32))
    finally:
        ops.set_gemm_precision(was)


@pytest.mark.parametrize("Hin", [299, 300])
def test_conv1d_dgrad_takes_one_launch_and_counts_it(tapn3_route, Hin):
    """with the tunable at 1: ONE f2g_gemm for the data gradient, on the kernel, over the caller's map itself and the
    cached image of the combined weight; the result against torch.autograd of F.conv2d in float64 -- which also holds
    the permute4 / copy3 / fill recipe of the combined weight to the layer --, the halo rows still zero, the bias
    gradient's 32 sums right; below the threshold and in the bf16x6 mode the loop runs"""
    ops = tapn3_route
    from flow2gan_amd import fused_disc as FD
    S = 12
    c = layer_case(S, Hin, 5)
    g, g_pre, w, y, Hout = c
    want, mag = float64_dgrad(c, S, Hin)
    n0 = ops.FP16X3_TAPN3_LAUNCHES
    colsum = torch.zeros(CIN, device=DEV)
    launches = []
    real_call = ops.call
    ops.call = lambda name, *a: (launches.append(name), real_call(name, *a))[1]
    try:
        FD._dgrad_weight3(w), ops._f16_seq_operand(ops.mat(FD._dgrad_weight3(w)))      # (cached before the count)
        del launches[:]
        gx = dgrad(FD, c, S, Hin, colsum)
    finally:
        ops.call = real_call
    torch.cuda.synchronize()
    assert ops.FP16X3_TAPN3_LAUNCHES == n0 + 1 and last_kernel(ops) == NAME
    assert launches.count("f2g_gemm") == 1 and "f2g_split_f16x2_seq" not in launches
    view = gx.view(S, Hin + 4, CIN)
    assert bool((view[:, :2] == 0).all()) and bool((view[:, 2 + Hin:] == 0).all()), "a halo row was written"
    check(view[:, 2:2 + Hin].double(), want, mag, TOL, "data gradient against autograd")
    check(colsum.double(), want.sum((0, 1)), mag.sum((0, 1)), TOL, "bias gradient")
    for rows, mode in ((S * Hout + 1, "fp16x3"), (1, "bf16x6")):
        ops.FP16X3_TAPN3_MIN_ROWS = rows
        ops.set_gemm_precision(mode)
        gx = dgrad(FD, c, S, Hin)
        assert ops.FP16X3_TAPN3_LAUNCHES == n0 + 1 and last_kernel(ops) != NAME
        check(gx.view(S, Hin + 4, CIN)[:, 2:2 + Hin].double(), want, mag, TOL, "the three launches")


def test_the_combined_weights_image_follows_its_weight(tapn3_route):
    """after a raw-pointer update (the optimizer's way: bump_weight_epoch + the batched rebuild_derived, which
    replays the permute4 / copy3 / fill recipe) and after an autograd-visible in-place update, the next launch reads
    a rebuilt combined weight, image and scales"""
    ops = tapn3_route
    from flow2gan_amd import fused_disc as FD
    S, Hin = 12, 298
    c = layer_case(S, Hin, 9)
    w = c[2]

    def launch_and_check(what):
        n0 = ops.FP16X3_TAPN3_LAUNCHES
        gx = dgrad(FD, c, S, Hin)
        assert ops.FP16X3_TAPN3_LAUNCHES == n0 + 1 and last_kernel(ops) == NAME
        want, mag = float64_dgrad(c, S, Hin)
        got = gx.view(S, Hin + 4, CIN)[:, 2:2 + Hin].clone()
        check(got.double(), want, mag, TOL, what)
        wc = FD._dgrad_weight3(w)
        buf = ops._f16_seq_operand(ops.mat(wc))._keep[0]
        torch.cuda.synchronize()
        assert torch.equal(wc.cpu(), res3.combined_weight(w.detach().cpu())), f"{what}: the combined weight is stale"
        K = 2 * CC
        img, rs = buf[:N3 * K].cpu().view(torch.int32).view(N3, K), buf[N3 * K:N3 * K + N3].cpu()
        want_img, want_rs = emul.image(wc.cpu())
        assert torch.equal(img, want_img) and torch.equal(rs, want_rs), f"{what}: the cached image is stale"
        return got

    image_follows_weight(ops, w, launch_and_check)


# ------------------------------------------------------------------ one period of the MPD against the CPU oracle
def test_mpd_period_against_oracle(tapn3_route):
    """the period-2 sub-discriminator at the shapes of tests/test_hip_disc_autograd.py: score, feature maps, input
    gradient and every parameter gradient against the oracle at that file's tolerance; a backward counts ONE launch
    on the route (the data gradient of the 32 -> 128 layer), a forward none, and nothing when it is off"""
    ops = tapn3_route
    r = subdisc_against_oracle(ops, "mpd", ("FP16X3_TAPN3_LAUNCHES",),
                               "mpd period 2, fp16x3 one-launch data gradient of the 32 -> 128 layer")
    print(f"[h3pn3] period {r.sub.period}: {r.fwd[0]} forward and {r.bwd[0]} backward launches on the route")
    assert r.fwd[0] == 0 and r.bwd[0] == 1, "one launch for the data gradient of the 32 -> 128 layer"
    ops.FP16X3_TAPN3_MIN_ROWS = ops.FP16X3_TAP_OFF
    assert r.rerun() == ((0,), (0,))
