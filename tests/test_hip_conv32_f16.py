"""conv32h3.hip on the GPU: the fp16x3 MRD band convolutions (f2g_conv32_desc.precision 4) that scale each tile's
patch inside the kernel, against float64 conv2d and its autograd (the references of tests/test_hip_conv32_regw.py).

What the structure can get wrong, at the smallest shapes that show it: a wrong two-piece fragment, patch offset or
piece order (one k step at a time), a scale from the wrong tile of a block's walk or from the previous launch
(sequences many binades apart), where the patch's maximum is looked for (halo pixels, zeros, a NaN), blocks with few
tiles, the reduction's order, the strided / offset gradient input with every epilogue, the descriptors the entry
points must refuse, the Python routing with its two tunables and counters, the cached weight image following its
weight, and one MRD window end to end against the CPU oracle.

Tolerance, per element: 1.8e-6 * sum |a||w| (the TOL of the fp16x3 GPU tests: the suite's 1e-6 for fp32 accumulation
plus the arithmetic's 3 * 2^-22 per product) + 2^-28 (amax_patch sum_k |w_k| + wmax sum_k |a_k|), the floor term of the
tile-wide scale (tests/fp16x3_conv32_emul.py).  Column sums: 1e-4 * max |want|.  Shapes are (S, H, Win).
"""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import fp16x3_conv32_emul as emul
from fp16x3_gpu import EINVAL, TOL, fp16x3_mode, image_follows_weight, library, subdisc_against_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOPE = 0.1


@pytest.fixture
def ops():
    """the fp16x3 mode with both band-conv tunables on; mode and tunables restored afterwards"""
    with fp16x3_mode(library(), "FP16X3_CONV32_FWD", "FP16X3_CONV32_DGRAD") as o:
        o.FP16X3_CONV32_FWD = o.FP16X3_CONV32_DGRAD = True
        yield o


def g(t):
    return t.to(DEV).contiguous()


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


W = rnd(32, 32, 3, 9, seed=2, scale=0.05)          # [co][ci][dh][j]
B = rnd(32, seed=3)


def packed(w):
    """(forward matrix [co][tap][ci], data-gradient tiles [tap][ci][co])"""
    return (w.permute(0, 2, 3, 1).reshape(32, 27 * 32).contiguous(),
            w.permute(2, 3, 1, 0).reshape(27, 32, 32).contiguous())


def wout_of(Win):
    return (Win - 1) // 2 + 1


def ref_fwd(x, w, b):
    """x (S, H, Win, 32) -> float64 (S, H, Wout, 32)"""
    y = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), stride=(1, 2), padding=(1, 4))
    return F.leaky_relu(y, SLOPE).permute(0, 2, 3, 1)


def ref_dgrad(gy, w, Win):
    """gy (S, H, Wout, 32) -> float64 (S, H, Win, 32), by autograd"""
    S, H = gy.shape[:2]
    x = torch.zeros(S, 32, H, Win, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), None, stride=(1, 2), padding=(1, 4)).backward(gy.permute(0, 3, 1, 2).double())
    return x.grad.permute(0, 2, 3, 1)


def tol_fwd(x, w, b):
    return emul.bound_fwd(x, w, rel=TOL)[0] + TOL * b.double().abs()


def tol_dgrad(gy, w, Win):
    return emul.bound_dgrad(gy, w, Win, rel=TOL)[0]


def seq_scales(S):
    """sequence s times 2^((7 s mod 41) - 20): neighbouring tiles of a block's walk lie many binades apart"""
    return torch.ldexp(torch.ones(S), (7 * torch.arange(S)) % 41 - 20)[:, None, None, None]


@functools.lru_cache(maxsize=None)
def case(S, H, Win, seed=0, spread=False):
    """Inputs, float64 references and per-element tolerances of one shape with the module's weights: computed once,
    shared, not modified."""
    Wout = wout_of(Win)
    x, gy = rnd(S, H, Win, 32, seed=11 + seed), rnd(S, H, Wout, 32, seed=14 + seed)
    if spread:
        x, gy = x * seq_scales(S), gy * seq_scales(S).flip(0)
    yact = rnd(S, H, Win, 32, seed=15 + seed)
    yact = torch.where(yact > 0, yact, SLOPE * yact)       # an activation map: leaky_relu(pre)
    factor = torch.where(yact > 0, 1.0, SLOPE).double()
    gx = ref_dgrad(gy, W, Win)
    return dict(x=x, gy=gy, yact=yact, factor=factor, y=ref_fwd(x, W, B), y_tol=tol_fwd(x, W, B), gx=gx,
                gx_tol=tol_dgrad(gy, W, Win))


def close(got, want, tol, name):
    got = got.detach().cpu().double().reshape(want.shape)
    err = (got - want).abs()
    bad = ~(err <= tol)                                     # (a NaN fails)
    worst = float((err / tol)[tol > 0].max()) if bool((tol > 0).any()) else 0.0
    print(f"[conv32 fp16x3] {name}: worst error {worst:.3f} of the tolerance")
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements beyond the tolerance, worst {worst:.3f} of it"


def close_sums(got, want, name):
    scale = want.abs().max().item() + 1e-30
    err = (got.detach().cpu().double() - want).abs().max().item()
    assert err <= 1e-4 * scale, f"{name}: max err {err:.3e} vs scale {scale:.3e}"


def run_fwd(ops, x, wp, b=B):
    S, H, Win = x.shape[:3]
    Wout = wout_of(Win)
    y = torch.full((S * H * Wout, 32), 7.0, device=DEV)
    n0 = ops.FP16X3_CONV32_FWD_LAUNCHES
    ops.conv32_s2_fwd(g(x).view(-1, 32), S, H, Win, Wout, wp, g(b), SLOPE, y)
    assert ops.FP16X3_CONV32_FWD_LAUNCHES == n0 + 1
    return y


def run_dgrad(ops, gy, Win, wT, **kw):
    """gy: the gradient map (S, H, Wout, 32), or a wider map that holds it (g_off / g_line / g_seq in kw)"""
    S, H, Wout = gy.shape[0], gy.shape[1], wout_of(Win)
    gx = torch.full((S * H * Win, 32), 7.0, device=DEV)
    n0 = ops.FP16X3_CONV32_DGRAD_LAUNCHES
    ops.conv32_s2_dgrad(g(gy).view(-1, 32), S, H, Win, Wout, wT, gx, **kw)
    assert ops.FP16X3_CONV32_DGRAD_LAUNCHES == n0 + 1
    return gx


def all_three(ops, c, Win, wp, wT, tag):
    """forward, plain data gradient, masked data gradient with column sums"""
    close(run_fwd(ops, c["x"], wp), c["y"], c["y_tol"], f"forward, {tag}")
    close(run_dgrad(ops, c["gy"], Win, wT), c["gx"], c["gx_tol"], f"data gradient, {tag}")
    cs = torch.zeros(32, device=DEV)
    gm = run_dgrad(ops, c["gy"], Win, wT, mask=(g(c["yact"]).view(-1, 32), 0, SLOPE), colsum=cs)
    want = c["gx"] * c["factor"]
    close(gm, want, c["gx_tol"] * c["factor"], f"masked data gradient, {tag}")
    close_sums(cs, want.reshape(-1, 32).sum(0), f"column sums, {tag}")


# ------------------------------------------------------------------ 1. one k step at a time
def test_one_k_step_at_a_time(ops):
    """All weights zero except one (tap, channel half) of the 54: the WHOLE result is compared, so a wrong hi / lo
    fragment, patch offset or piece order, or a contribution from a k step that should be silent, all fail.  The data
    gradient's k-step halves are halves of the OUTPUT channels: both kinds of half are walked.  (2, 9, 21): a partial
    tile on every edge."""
    S, H, Win = 2, 9, 21
    c = case(S, H, Win)
    for tap in range(27):
        for half in range(2):
            sl = slice(16 * half, 16 * half + 16)
            w = torch.zeros_like(W)
            w[:, sl, tap // 9, tap % 9] = W[:, sl, tap // 9, tap % 9]
            wp, wT = packed(w)
            close(run_fwd(ops, c["x"], g(wp)), ref_fwd(c["x"], w, B), tol_fwd(c["x"], w, B),
                  f"forward, tap {tap} half {half}")
            close(run_dgrad(ops, c["gy"], Win, g(wT)), ref_dgrad(c["gy"], w, Win), tol_dgrad(c["gy"], w, Win),
                  f"data gradient, tap {tap} input half {half}")
            w = torch.zeros_like(W)
            w[sl, :, tap // 9, tap % 9] = W[sl, :, tap // 9, tap % 9]
            wp, wT = packed(w)
            close(run_dgrad(ops, c["gy"], Win, g(wT)), ref_dgrad(c["gy"], w, Win), tol_dgrad(c["gy"], w, Win),
                  f"data gradient, tap {tap} output half {half}")


# ------------------------------------------------------------------ 2. scales from the wrong tile or launch
@pytest.mark.parametrize("S,H,Win", [(34, 47, 77), (70, 47, 39), (70, 24, 63)])
def test_scales_belong_to_their_tile_and_launch(ops, S, H, Win):
    """Persistent blocks walk several tiles: (34, 47, 77) and (70, 47, 39) on 16 x 8 tiles (510 and 630 of them on 256
    blocks), (70, 24, 63) on 8 x 16 ones (420).  Sequence s is multiplied by 2^((7 s mod 41) - 20), so a scale carried
    over from the previous tile of a block's walk, or from the previous launch, is off by many binades and shows as inf
    or as lost bits.  Then the same weights with a second, different input in a second launch."""
    wp, wT = (g(t) for t in packed(W))
    for seed in (0, 1):
        all_three(ops, case(S, H, Win, seed, True), Win, wp, wT, f"launch {seed}")


# ------------------------------------------------------------------ 3. few tiles, degenerate widths
@pytest.mark.parametrize("S,H,Win", [(1, 5, 2), (2, 9, 1), (2, 16, 16), (2, 8, 64)])
def test_few_tiles_and_degenerate_widths(ops, S, H, Win):
    """One partial tile with Wout = 1; Win = 1 (the odd column parity is empty); tile-exact 16 x 8 and 8 x 16."""
    wp, wT = (g(t) for t in packed(W))
    all_three(ops, case(S, H, Win), Win, wp, wT, "few tiles")


# ------------------------------------------------------------------ 4. where the maximum sits
def test_zero_image_gives_the_bias_exactly(ops):
    S, H, Win = 2, 9, 21
    wp, wT = (g(t) for t in packed(W))
    y = run_fwd(ops, torch.zeros(S, H, Win, 32), wp)
    want = F.leaky_relu(B, SLOPE).expand(S * H * wout_of(Win), 32)
    assert torch.equal(y.cpu(), want)
    gx = run_dgrad(ops, torch.zeros(S, H, wout_of(Win), 32), Win, wT)
    assert torch.equal(gx.cpu(), torch.zeros(S * H * Win, 32))


def test_maximum_in_the_halo_of_a_tile(ops):
    """(2, 9, 63): 8 x 16 tiles, two per row.  Sequence 0 is zero except for ONE pixel of 2^20 that belongs to the
    second tile's columns and lies in the first tile's halo (inside its patch): a maximum taken over a tile's own
    columns alone would give the first tile scale 2^14 / 0 and send 2^20 out of fp16's range."""
    S, H, Win = 2, 9, 63
    Wout = wout_of(Win)
    wp, wT = (g(t) for t in packed(W))
    x, gy = rnd(S, H, Win, 32, seed=5), rnd(S, H, Wout, 32, seed=6)
    x[0], gy[0] = 0.0, 0.0
    x[0, 3, 34, 7] = 2.0 ** 20        # input column 34: the centre of output column 17, in the window of column 15
    gy[0, 3, 17, 7] = 2.0 ** 20       # gradient column 17: read by positions m = 15 .. 19
    y = run_fwd(ops, x, wp)
    assert bool(torch.isfinite(y).all())
    close(y, ref_fwd(x, W, B), tol_fwd(x, W, B), "forward, maximum in the halo")
    gx = run_dgrad(ops, gy, Win, wT)
    assert bool(torch.isfinite(gx).all())
    close(gx, ref_dgrad(gy, W, Win), tol_dgrad(gy, W, Win), "data gradient, maximum in the halo")


def test_a_nan_pixel_stays_in_its_windows_and_tiles(ops):
    """One NaN pixel: every output whose window holds it is NaN, and the outputs of the tiles whose patch does not
    hold it stay within tolerance (the tiles that stage it unscaled promise nothing else)."""
    S, H, Win = 2, 20, 63
    Wout = wout_of(Win)
    wp, wT = (g(t) for t in packed(W))
    x, gy = rnd(S, H, Win, 32, seed=7), rnd(S, H, Wout, 32, seed=8)
    x[1, 9, 30, 5] = float("nan")
    gy[1, 9, 14, 5] = float("nan")
    hole_x, hole_g = torch.isnan(x).float(), torch.isnan(gy).float()
    ones = torch.ones_like(W)
    for what, got, holds, tiles, want, tol in (
            ("forward", run_fwd(ops, x, wp), emul.exact_fwd(hole_x, ones) > 0, torch.isnan(emul.patch_amax_fwd(x)),
             ref_fwd(x.nan_to_num(0.0), W, B), tol_fwd(x.nan_to_num(0.0), W, B)),
            ("data gradient", run_dgrad(ops, gy, Win, wT), emul.exact_dgrad(hole_g, ones, Win) > 0,
             torch.isnan(emul.patch_amax_dgrad(gy, Win)), ref_dgrad(gy.nan_to_num(0.0), W, Win),
             tol_dgrad(gy.nan_to_num(0.0), W, Win))):
        got = got.cpu().double().reshape(want.shape)
        assert bool(holds.any()) and bool((tiles.expand_as(holds) | ~holds).all())
        assert bool(torch.isnan(got[holds]).all()), f"{what}: a window that holds the NaN is not NaN"
        other = ~tiles.expand_as(holds)
        assert bool(other.any())
        err = (got - want).abs()
        assert bool((err[other] <= tol[other]).all()), f"{what}: the NaN reached another tile"


# ------------------------------------------------------------------ 5. bit-reproducible
def test_fixed_reduction_order_is_bit_reproducible(ops):
    S, H, Win = 34, 47, 77
    wp, wT = (g(t) for t in packed(W))
    c = case(S, H, Win, 0, True)
    assert torch.equal(run_fwd(ops, c["x"], wp), run_fwd(ops, c["x"], wp))
    assert torch.equal(run_dgrad(ops, c["gy"], Win, wT), run_dgrad(ops, c["gy"], Win, wT))


# ------------------------------------------------------------------ 6. strided, offset gradient input, every epilogue
@pytest.mark.parametrize("S,H,Win", [(3, 11, 13), (24, 94, 77)])
def test_strided_offset_gradient_with_every_epilogue(ops, S, H, Win):
    """The data gradient reads a band's slice of a wider concatenated map (g_off, g_line, g_seq set), as fused_disc
    calls it: mask only, then mask plus the feature-matching term, both with column sums.  The neighbouring bands'
    columns are 2^10 louder: they are outside the map and must not reach the patch's maximum (nor its windows)."""
    Wout = wout_of(Win)
    wp, wT = (g(t) for t in packed(W))
    c = case(S, H, Win)
    lo, Wtot = 5, Wout + 9                                  # the band's first column / the map's width
    wide = rnd(S, H, Wtot, 32, seed=21) * 1024.0
    wide[:, :, lo:lo + Wout] = c["gy"]
    yreal = rnd(S, H, Win, 32, seed=16)
    wdev = torch.tensor([0.7])
    for use_fm in (False, True):
        want, tol = c["gx"].clone(), c["gx_tol"].clone()
        if use_fm:
            want = want + 0.25 * 0.7 * torch.sign(c["yact"].double() - yreal.double())
            tol = tol + TOL * 0.25 * 0.7
        want, tol = want * c["factor"], tol * c["factor"]
        cs = torch.zeros(32, device=DEV)
        gx = run_dgrad(ops, wide, Win, wT, g_seq=H * Wtot * 32, g_line=Wtot * 32, g_off=lo * 32,
                       mask=(g(c["yact"]).view(-1, 32), 0, SLOPE),
                       fm=(g(yreal).view(-1, 32), 0, 0.25, g(wdev)) if use_fm else None, colsum=cs)
        close(gx, want, tol, f"strided data gradient (fm={use_fm})")
        close_sums(cs, want.reshape(-1, 32).sum(0), f"column sums (fm={use_fm})")


# ------------------------------------------------------------------ 7. refusals
def test_refusals(ops):
    S, H, Win = 2, 9, 21
    Wout = wout_of(Win)
    lib, st = ops.L.lib, ops.L.stream_ptr()
    wp, wT = (g(t) for t in packed(W))
    x, gy = g(rnd(S * H * Win, 32, seed=1)), g(rnd(S * H * Wout, 32, seed=2))
    img_f, img_d = ops.conv32_f16_image(wp), ops.conv32_f16_image(wT)
    y = torch.full((S * H * Wout * 32 + 64,), 7.0, device=DEV)
    gx = torch.full((S * H * Win * 32 + 64,), 7.0, device=DEV)

    def desc(fwd):
        d = ops.L.Conv32Desc()
        d.S, d.H, d.Win, d.Wout, d.precision = S, H, Win, Wout, 4
        if fwd:
            d.x, d.x_seq, d.x_line = x.data_ptr(), H * Win * 32, Win * 32
            d.w, d.y, d.y_seq, d.y_line = img_f.data_ptr(), y.data_ptr(), H * Wout * 32, Wout * 32
        else:
            d.x, d.x_seq, d.x_line = gy.data_ptr(), H * Wout * 32, Wout * 32
            d.w, d.y, d.y_seq, d.y_line = img_d.data_ptr(), gx.data_ptr(), H * Win * 32, Win * 32
        return d

    for fwd, fn, out in ((True, lib.f2g_conv32_s2_fwd, y), (False, lib.f2g_conv32_s2_dgrad, gx)):
        d = desc(fwd)
        d.w += 4                                            # a misaligned image
        assert fn(C.byref(d), st) == EINVAL
        d = desc(fwd)
        d.y_line += 2                                       # output rows that are no 16-byte segments
        assert fn(C.byref(d), st) == EINVAL
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), "a refused launch wrote its output"
        assert fn(C.byref(desc(fwd)), st) == 0              # (the descriptor itself is fine)
    d = desc(True)
    d.y, d.y_seq, d.y_line = gy.data_ptr(), H * Wout * 32, Wout * 32       # the weight gradient's roles: y = gradient
    gw = torch.zeros(32, 27 * 32, device=DEV)
    assert lib.f2g_conv32_s2_wgrad(C.byref(d), gw.data_ptr(), st) == EINVAL
    d.precision = 3
    assert lib.f2g_conv32_s2_wgrad(C.byref(d), gw.data_ptr(), st) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 8. ops: tunables, counters, the launch of today
def test_ops_route_and_the_launch_with_the_tunables_off(ops):
    S, H, Win = 3, 11, 13
    Wout = wout_of(Win)
    c = case(S, H, Win)
    wp, wT = (torch.nn.Parameter(g(t)) for t in packed(W))
    xg, gg = g(c["x"]).view(-1, 32), g(c["gy"]).view(-1, 32)

    def both():
        y = torch.full((S * H * Wout, 32), 7.0, device=DEV)
        gx = torch.full((S * H * Win, 32), 7.0, device=DEV)
        n = ops.FP16X3_CONV32_FWD_LAUNCHES, ops.FP16X3_CONV32_DGRAD_LAUNCHES
        ops.conv32_s2_fwd(xg, S, H, Win, Wout, wp, g(B), SLOPE, y)
        ops.conv32_s2_dgrad(gg, S, H, Win, Wout, wT, gx)
        torch.cuda.synchronize()
        return y, gx, ops.FP16X3_CONV32_FWD_LAUNCHES - n[0], ops.FP16X3_CONV32_DGRAD_LAUNCHES - n[1]

    def precision3():
        """today's launch, spelled out: precision 3 over the three-piece images"""
        lib, st = ops.L.lib, ops.L.stream_ptr()
        y = torch.full((S * H * Wout, 32), 7.0, device=DEV)
        gx = torch.full((S * H * Win, 32), 7.0, device=DEV)
        bias = g(B)
        i3f, i3d = ops.x3_image(wp.detach()), ops.x3_image(wT.detach().view(27 * 32, 32))
        d = ops.L.Conv32Desc()
        d.S, d.H, d.Win, d.Wout, d.precision = S, H, Win, Wout, 3
        d.x, d.x_seq, d.x_line = xg.data_ptr(), H * Win * 32, Win * 32
        d.w, d.bias, d.lrelu_slope = i3f.data_ptr(), bias.data_ptr(), SLOPE
        d.y, d.y_seq, d.y_line = y.data_ptr(), H * Wout * 32, Wout * 32
        assert lib.f2g_conv32_s2_fwd(C.byref(d), st) == 0
        d = ops.L.Conv32Desc()
        d.S, d.H, d.Win, d.Wout, d.precision = S, H, Win, Wout, 3
        d.x, d.x_seq, d.x_line = gg.data_ptr(), H * Wout * 32, Wout * 32
        d.w, d.y, d.y_seq, d.y_line = i3d.data_ptr(), gx.data_ptr(), H * Win * 32, Win * 32
        assert lib.f2g_conv32_s2_dgrad(C.byref(d), st) == 0
        torch.cuda.synchronize()
        return y, gx

    y, gx, nf, nd = both()
    assert (nf, nd) == (1, 1)
    close(y, c["y"], c["y_tol"], "ops forward")
    close(gx, c["gx"], c["gx_tol"], "ops data gradient")
    y3, gx3 = precision3()
    ops.FP16X3_CONV32_FWD = False                           # one tunable at a time
    y, gx, nf, nd = both()
    assert (nf, nd) == (0, 1) and torch.equal(y, y3)
    ops.FP16X3_CONV32_FWD, ops.FP16X3_CONV32_DGRAD = True, False
    y, gx, nf, nd = both()
    assert (nf, nd) == (1, 0) and torch.equal(gx, gx3)
    ops.FP16X3_CONV32_DGRAD = True
    ops.set_gemm_precision("bf16x6")                        # the tunables mean nothing outside the fp16x3 mode
    y, gx, nf, nd = both()
    assert (nf, nd) == (0, 0) and torch.equal(y, y3) and torch.equal(gx, gx3)


# ------------------------------------------------------------------ 9. the cached image follows its weight
def test_weight_image_follows_its_weight(ops):
    """the MRD's chains: the forward image hangs under the packed copy of the conv weight (pack -> f16x2seq), the data
    gradient's under the transposed tiles.  After a raw-pointer update (bump_weight_epoch + the batched
    rebuild_derived) and after an in-place update the image and its scale equal the emulation's and the output moves."""
    from flow2gan_amd import fused_disc as FD
    S, H, Win = 2, 9, 21
    Wout = wout_of(Win)
    c = case(S, H, Win)
    w = torch.nn.Parameter(g(W.clone()))

    def build_t(t):
        out = ops.empty(27, 32, 32, device=t.device)
        ops.permute4(out, t, (27, 32, 32, 1), (1, 27, 32 * 27, 0))
        return out

    def launch_and_check(what):
        wp, wT = ops.derived(w, "pack", FD.pack_conv_weight), ops.derived(w, "dgrad_taps", build_t)
        y = run_fwd(ops, c["x"], wp)
        gx = run_dgrad(ops, c["gy"], Win, wT)
        torch.cuda.synchronize()
        wc = w.detach().cpu()
        close(y, ref_fwd(c["x"], wc, B), tol_fwd(c["x"], wc, B), f"forward, {what}")
        close(gx, ref_dgrad(c["gy"], wc, Win), tol_dgrad(c["gy"], wc, Win), f"data gradient, {what}")
        for lay, host in zip((wp, wT), packed(wc)):
            assert torch.equal(lay.cpu().reshape(host.shape), host), f"{what}: the re-laid copy is stale"
            buf = ops.conv32_f16_image(lay).cpu()
            assert buf.numel() == 27648 + 1
            want_img, want_rs = emul.weight_image(host)
            assert torch.equal(buf[:27648].view(torch.int32), want_img), f"{what}: the cached image is stale"
            assert torch.equal(buf[27648:], want_rs), f"{what}: the cached scale is stale"
        return y.clone(), gx.clone()

    def update(w):
        w.data.copy_(w.detach() * 37.0 + 0.01)              # (the matrix's scale must move too)

    image_follows_weight(ops, w, launch_and_check, update=update, min_replays=2)


# ------------------------------------------------------------------ 10. one MRD window against the CPU oracle
def test_mrd_window_against_oracle(ops):
    """one resolution's sub-discriminator at the shapes of tests/test_hip_disc_autograd.py: scores, feature maps, the
    input gradient and every parameter gradient against the oracle at that file's tolerance; both counters move with
    the tunables on and stand still with them off"""
    counters = ("FP16X3_CONV32_FWD_LAUNCHES", "FP16X3_CONV32_DGRAD_LAUNCHES")
    r = subdisc_against_oracle(ops, "mrd", counters, "mrd window, fp16x3 band convolutions")
    nf, nd = (f + b for f, b in zip(r.fwd, r.bwd))
    print(f"[conv32 fp16x3] window {r.sub.window_length}: {nf} forward and {nd} data-gradient launches")
    assert nf > 0 and nd > 0
    ops.FP16X3_CONV32_FWD = ops.FP16X3_CONV32_DGRAD = False
    assert r.rerun() == ((0, 0), (0, 0))
