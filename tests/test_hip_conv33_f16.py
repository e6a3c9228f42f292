"""conv33h3.hip on the GPU: the fp16x3 (3, 3) fifth layer of an MRD band stack (f2g_conv33_fwd at
f2g_conv32_desc.precision 4), forward and data-gradient role, against float64 conv2d with padding (1, 1) and its
autograd.

What the structure can get wrong, at the smallest shapes that show it: a wrong two-piece fragment, patch offset or
piece order (one k step at a time), a scale from the wrong tile of a block's walk or from the previous launch
(sequences many binades apart), where the patch's maximum is looked for (halo rows, zeros, a NaN), blocks with few
tiles and degenerate widths, the reduction's order, strided / offset slices of wider maps with every epilogue, the
descriptors the entry points must refuse, the Python routing with its two tunables and counters, the cached weight
image following its weight, and one MRD resolution end to end against the CPU oracle.

Tolerance, per element: 1.8e-6 * sum |a||w| (the TOL of the fp16x3 GPU tests: the suite's 1e-6 for fp32 accumulation
plus the arithmetic's 3 * 2^-22 per product) + 2^-28 (amax_patch sum_k |w_k| + wmax sum_k |a_k|), the floor term of the
tile-wide scale (tests/fp16x3_conv33_emul.py), + 1.8e-6 |bias|.  Column sums: 1e-4 * max |want|.  Shapes are (S, H, W).
"""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import fp16x3_conv33_emul as emul
from fp16x3_gpu import EINVAL, TOL, fp16x3_mode, image_follows_weight, library, subdisc_against_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOPE = 0.1
BLOCKS = 256            # persistent blocks of a launch: grid = min(tiles, 256)


@pytest.fixture
def ops():
    """the fp16x3 mode with both (3, 3) tunables on; mode and tunables restored afterwards"""
    names = ("FP16X3_CONV33_FWD", "FP16X3_CONV33_DGRAD", "FP16X3_CONV32_FWD", "FP16X3_CONV32_DGRAD",
             "FP16X3_CONV32_WGRAD")
    with fp16x3_mode(library(), *names) as o:
        o.FP16X3_CONV33_FWD = o.FP16X3_CONV33_DGRAD = True
        yield o


def g(t):
    return t.to(DEV).contiguous()


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


W33 = rnd(32, 32, 3, 3, seed=2, scale=0.05)        # [co][ci][dh][dw]
B = rnd(32, seed=3)


def packed(w):
    """(forward matrix [co][tap][ci], data-gradient matrix [ci][8 - tap][co]), both (32, 9 * 32)"""
    return (w.permute(0, 2, 3, 1).reshape(32, 9 * 32).contiguous(),
            w.flip(2, 3).permute(1, 2, 3, 0).reshape(32, 9 * 32).contiguous())


def ref_fwd(x, w, b):
    """x (S, H, W, 32) -> float64 (S, H, W, 32)"""
    y = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=(1, 1))
    return F.leaky_relu(y, SLOPE).permute(0, 2, 3, 1)


def ref_dgrad(gy, w):
    """gy (S, H, W, 32) -> float64 (S, H, W, 32), by autograd"""
    S, H, W_ = gy.shape[:3]
    x = torch.zeros(S, 32, H, W_, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), None, padding=(1, 1)).backward(gy.permute(0, 3, 1, 2).double())
    return x.grad.permute(0, 2, 3, 1)


def tol_fwd(x, w, b):
    return emul.bound_fwd(x, w, rel=TOL)[0] + TOL * b.double().abs()


def tol_dgrad(gy, w):
    return emul.bound_dgrad(gy, w, rel=TOL)[0]


def seq_scales(S):
    """sequence s times 2^((7 s mod 41) - 20): neighbouring tiles of a block's walk lie many binades apart"""
    return torch.ldexp(torch.ones(S), (7 * torch.arange(S)) % 41 - 20)[:, None, None, None]


@functools.lru_cache(maxsize=None)
def case(S, H, W_, seed=0, spread=0):
    """Inputs, float64 references and per-element tolerances of one shape with the module's weights: computed once,
    shared, not modified.  spread = 1: x under seq_scales and gy under the flipped ones; 2: the other way round."""
    x, gy = rnd(S, H, W_, 32, seed=11 + seed), rnd(S, H, W_, 32, seed=14 + seed)
    if spread:
        sc = seq_scales(S) if spread == 1 else seq_scales(S).flip(0)
        x, gy = x * sc, gy * sc.flip(0)
    yact = rnd(S, H, W_, 32, seed=15 + seed)
    yact = torch.where(yact > 0, yact, SLOPE * yact)       # an activation map: leaky_relu(pre)
    factor = torch.where(yact > 0, 1.0, SLOPE).double()
    return dict(x=x, gy=gy, yact=yact, factor=factor, y=ref_fwd(x, W33, B), y_tol=tol_fwd(x, W33, B),
                gx=ref_dgrad(gy, W33), gx_tol=tol_dgrad(gy, W33))


def close(got, want, tol, name):
    got = got.detach().cpu().double().reshape(want.shape)
    err = (got - want).abs()
    bad = ~(err <= tol)                                     # (a NaN fails)
    worst = float((err / tol)[tol > 0].max()) if bool((tol > 0).any()) else 0.0
    print(f"[conv33 fp16x3] {name}: worst error {worst:.3f} of the tolerance")
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements beyond the tolerance, worst {worst:.3f} of it"


def close_sums(got, want, name):
    scale = want.abs().max().item() + 1e-30
    err = (got.detach().cpu().double() - want).abs().max().item()
    print(f"[conv33 fp16x3] {name}: max err {err:.3e} vs scale {scale:.3e}")
    assert err <= 1e-4 * scale, f"{name}: max err {err:.3e} vs scale {scale:.3e}"


def run_fwd(ops, x, wp, b=B, y=None, **kw):
    """x: the map (S, H, W, 32); y / kw: a wider output map and its y_off / y_line / y_seq"""
    S, H, W_ = x.shape[:3]
    if y is None:
        y = torch.full((S * H * W_, 32), 7.0, device=DEV)
    n0 = ops.FP16X3_CONV33_FWD_LAUNCHES, ops.FP16X3_CONV33_DGRAD_LAUNCHES
    ops.conv33(g(x).view(-1, 32), S, H, W_, wp, g(b), SLOPE, y, **kw)
    assert (ops.FP16X3_CONV33_FWD_LAUNCHES, ops.FP16X3_CONV33_DGRAD_LAUNCHES) == (n0[0] + 1, n0[1])
    return y


def run_dgrad(ops, gy, wf, W_=None, **kw):
    """gy: the gradient map (S, H, W, 32), or a wider map that holds it (W_ and x_off / x_line / x_seq in kw)"""
    S, H = gy.shape[:2]
    W_ = gy.shape[2] if W_ is None else W_
    gx = torch.full((S * H * W_, 32), 7.0, device=DEV)
    n0 = ops.FP16X3_CONV33_FWD_LAUNCHES, ops.FP16X3_CONV33_DGRAD_LAUNCHES
    ops.conv33(g(gy).view(-1, 32), S, H, W_, wf, None, 0.0, gx, form=1, **kw)
    assert (ops.FP16X3_CONV33_FWD_LAUNCHES, ops.FP16X3_CONV33_DGRAD_LAUNCHES) == (n0[0], n0[1] + 1)
    return gx


def all_three(ops, c, wp, wf, tag):
    """forward, plain data gradient, masked data gradient with column sums"""
    close(run_fwd(ops, c["x"], wp), c["y"], c["y_tol"], f"forward, {tag}")
    close(run_dgrad(ops, c["gy"], wf), c["gx"], c["gx_tol"], f"data gradient, {tag}")
    cs = torch.zeros(32, device=DEV)
    gm = run_dgrad(ops, c["gy"], wf, mask=(g(c["yact"]).view(-1, 32), 0, SLOPE), colsum=cs)
    want = c["gx"] * c["factor"]
    close(gm, want, c["gx_tol"] * c["factor"], f"masked data gradient, {tag}")
    close_sums(cs, want.reshape(-1, 32).sum(0), f"column sums, {tag}")


# ------------------------------------------------------------------ 1. one k step at a time
def test_one_k_step_at_a_time(ops):
    """All weights zero except one (tap, channel half) of the 18: the WHOLE result is compared, so a wrong hi / lo
    fragment, patch offset or piece order, or a contribution from a k step that should be silent, all fail.  The data
    gradient's k-step halves are halves of the OUTPUT channels.  (2, 9, 13): one tile per sequence."""
    S, H, W_ = 2, 9, 13
    c = case(S, H, W_)
    for tap in range(9):
        for half in range(2):
            sl = slice(16 * half, 16 * half + 16)
            w = torch.zeros_like(W33)
            w[:, sl, tap // 3, tap % 3] = W33[:, sl, tap // 3, tap % 3]
            wp, _ = packed(w)
            close(run_fwd(ops, c["x"], g(wp)), ref_fwd(c["x"], w, B), tol_fwd(c["x"], w, B),
                  f"forward, tap {tap} half {half}")
            w = torch.zeros_like(W33)
            w[sl, :, tap // 3, tap % 3] = W33[sl, :, tap // 3, tap % 3]
            _, wf = packed(w)
            close(run_dgrad(ops, c["gy"], g(wf)), ref_dgrad(c["gy"], w), tol_dgrad(c["gy"], w),
                  f"data gradient, tap {tap} output half {half}")


# ------------------------------------------------------------------ 2. scales from the wrong tile or launch
def walk_binades(x):
    """the smallest distance, in binades, between the patch maxima of consecutive tiles of any block's walk"""
    S, H, W_ = x.shape[:3]
    R = emul.pick_rows(H, W_)
    amax = emul.patch_amax(x)[:, ::R, 0, 0].reshape(-1)     # one per tile, in tile order (sequence, tile row)
    assert amax.numel() == S * -(-H // R) > BLOCKS and bool((amax > 0).all())
    ex = torch.frexp(amax)[1]
    return int((ex[BLOCKS:] - ex[:-BLOCKS]).abs().min())


@pytest.mark.parametrize("S,H,W_,R", [(70, 40, 33, 7), (300, 37, 7, 36)])
def test_scales_belong_to_their_tile_and_launch(ops, S, H, W_, R):
    """Persistent blocks walk several tiles: (70, 40, 33) has R = 7 and 420 tiles on 256 blocks, (300, 37, 7) R = 36
    and 600 tiles, the last tile of a sequence one row.  Sequence s is multiplied by 2^((7 s mod 41) - 20), so a scale
    carried over from the previous tile of a block's walk, or from the previous launch, is off by many binades and
    shows as inf or as lost bits.  The second launch has the scaling flipped."""
    assert emul.pick_rows(H, W_) == R
    wp, wf = (g(t) for t in packed(W33))
    for launch, spread in enumerate((1, 2)):
        c = case(S, H, W_, launch, spread)
        assert walk_binades(c["x"]) >= 4 and walk_binades(c["gy"]) >= 4
        all_three(ops, c, wp, wf, f"launch {launch}")


# ------------------------------------------------------------------ 3. few tiles, degenerate widths
@pytest.mark.parametrize("S,H,W_", [(1, 1, 1), (1, 3, 112), (2, 5, 2), (1, 16, 16)])
def test_few_tiles_and_degenerate_widths(ops, S, H, W_):
    """One pixel; the widest row the kernel stages (R = 1); two columns; a tile-exact 16 x 16 map."""
    wp, wf = (g(t) for t in packed(W33))
    all_three(ops, case(S, H, W_), wp, wf, "few tiles")


# ------------------------------------------------------------------ 4. where the maximum sits
def test_zero_image_gives_the_bias_exactly(ops):
    S, H, W_ = 2, 9, 13
    wp, wf = (g(t) for t in packed(W33))
    y = run_fwd(ops, torch.zeros(S, H, W_, 32), wp)
    assert torch.equal(y.cpu(), F.leaky_relu(B, SLOPE).expand(S * H * W_, 32))
    gx = run_dgrad(ops, torch.zeros(S, H, W_, 32), wf)
    assert torch.equal(gx.cpu(), torch.zeros(S * H * W_, 32))


def test_maximum_in_the_halo_of_a_tile(ops):
    """(2, 14, 33): R = 7, two tiles per sequence.  Sequence 0 is zero except for ONE pixel of 2^20 in row 7: it
    belongs to the second tile and lies in the first tile's halo row.  A maximum taken over the tile's own rows alone
    would stage it unscaled and overflow fp16."""
    S, H, W_ = 2, 14, 33
    assert emul.pick_rows(H, W_) == 7
    wp, wf = (g(t) for t in packed(W33))
    x, gy = rnd(S, H, W_, 32, seed=5), rnd(S, H, W_, 32, seed=6)
    x[0], gy[0] = 0.0, 0.0
    x[0, 7, 17, 7] = 2.0 ** 20
    gy[0, 7, 17, 7] = 2.0 ** 20
    y = run_fwd(ops, x, wp)
    assert bool(torch.isfinite(y).all())
    close(y, ref_fwd(x, W33, B), tol_fwd(x, W33, B), "forward, maximum in the halo")
    gx = run_dgrad(ops, gy, wf)
    assert bool(torch.isfinite(gx).all())
    close(gx, ref_dgrad(gy, W33), tol_dgrad(gy, W33), "data gradient, maximum in the halo")


def test_a_nan_pixel_stays_in_its_windows_and_tiles(ops):
    """One NaN pixel: every output whose window holds it is NaN, and the outputs of the tiles whose patch does not
    hold it stay within tolerance (the tile that stages it unscaled promises nothing else).  (2, 21, 33): three tiles
    of seven rows per sequence, the NaN in the middle of the second."""
    S, H, W_ = 2, 21, 33
    wp, wf = (g(t) for t in packed(W33))
    x, gy = rnd(S, H, W_, 32, seed=7), rnd(S, H, W_, 32, seed=8)
    x[1, 10, 15, 5] = float("nan")
    gy[1, 10, 15, 5] = float("nan")
    ones = torch.ones_like(W33)
    for what, src, got, want, tol in (
            ("forward", x, run_fwd(ops, x, wp), ref_fwd(x.nan_to_num(0.0), W33, B), tol_fwd(x.nan_to_num(0.0), W33, B)),
            ("data gradient", gy, run_dgrad(ops, gy, wf), ref_dgrad(gy.nan_to_num(0.0), W33),
             tol_dgrad(gy.nan_to_num(0.0), W33))):
        holds = emul.exact_fwd(torch.isnan(src).float(), ones) > 0
        tiles = torch.isnan(emul.patch_amax(src)).expand_as(holds)
        got = got.cpu().double().reshape(want.shape)
        assert bool(holds.any()) and bool((tiles | ~holds).all())
        assert bool(torch.isnan(got[holds]).all()), f"{what}: a window that holds the NaN is not NaN"
        other = ~tiles
        assert bool(other.any())
        err = (got - want).abs()
        assert bool((err[other] <= tol[other]).all()), f"{what}: the NaN reached another tile"


# ------------------------------------------------------------------ 5. bit-reproducible
def test_fixed_reduction_order_is_bit_reproducible(ops):
    S, H, W_ = 70, 40, 33
    wp, wf = (g(t) for t in packed(W33))
    c = case(S, H, W_, 0, 1)
    assert torch.equal(run_fwd(ops, c["x"], wp), run_fwd(ops, c["x"], wp))
    assert torch.equal(run_dgrad(ops, c["gy"], wf), run_dgrad(ops, c["gy"], wf))


# ------------------------------------------------------------------ 6. slices of wider maps, as fused_disc calls it
@pytest.mark.parametrize("S,H,W_", [(3, 11, 13), (5, 40, 33)])
def test_slices_of_wider_maps_with_every_epilogue(ops, S, H, W_):
    """The data gradient reads a band's slice of a wider concatenated map (x_off, x_line, x_seq), plain and with mask
    + colsum; the forward writes a band's slice of a wider map (y_off, y_line, y_seq).  The neighbouring bands' columns
    hold a sentinel 2^10 louder than the band: read as input it would move the patch's maximum and the windows at the
    band's edge, which the result shows; in the output it must still stand."""
    wp, wf = (g(t) for t in packed(W33))
    c = case(S, H, W_)
    lo, Wtot = 5, W_ + 9                                    # the band's first column / the map's width
    wide = rnd(S, H, Wtot, 32, seed=21) * 1024.0
    wide[:, :, lo:lo + W_] = c["gy"]
    kw = dict(x_off=lo * 32, x_line=Wtot * 32, x_seq=H * Wtot * 32)
    close(run_dgrad(ops, wide, wf, W_, **kw), c["gx"], c["gx_tol"], "data gradient of a slice")
    cs = torch.zeros(32, device=DEV)
    gm = run_dgrad(ops, wide, wf, W_, mask=(g(c["yact"]).view(-1, 32), 0, SLOPE), colsum=cs, **kw)
    want = c["gx"] * c["factor"]
    close(gm, want, c["gx_tol"] * c["factor"], "masked data gradient of a slice")
    close_sums(cs, want.reshape(-1, 32).sum(0), "column sums of a slice")
    out = torch.full((S, H, Wtot, 32), 7.0, device=DEV)
    run_fwd(ops, c["x"], wp, y=out, y_off=lo * 32, y_line=Wtot * 32, y_seq=H * Wtot * 32)
    close(out[:, :, lo:lo + W_], c["y"], c["y_tol"], "forward into a slice")
    assert bool((out[:, :, :lo] == 7.0).all()) and bool((out[:, :, lo + W_:] == 7.0).all()), "a neighbour was written"


# ------------------------------------------------------------------ 7. refusals
def test_refusals(ops):
    S, H, W_ = 2, 9, 13
    lib, st = ops.L.lib, ops.L.stream_ptr()
    wp, wf = (g(t) for t in packed(W33))
    n = S * H * 113 * 32 + 64                               # (room for the W = 113 descriptor, were it taken)
    x, y = g(rnd(n, seed=1)), torch.full((n,), 7.0, device=DEV)
    other, bias = g(rnd(n, seed=2)), g(B)
    img = ops.conv32_f16_image(wp)
    assert img.numel() == 9216 + 1

    def desc(width=W_):
        d = ops.L.Conv32Desc()
        d.S, d.H, d.Win, d.Wout, d.precision = S, H, width, width, 4
        d.x, d.x_seq, d.x_line = x.data_ptr(), H * width * 32, width * 32
        d.w, d.y, d.y_seq, d.y_line = img.data_ptr(), y.data_ptr(), H * width * 32, width * 32
        return d

    def refused(d):
        assert lib.f2g_conv33_fwd(C.byref(d), st) == EINVAL
        torch.cuda.synchronize()
        assert bool((y == 7.0).all()), "a refused launch wrote its output"

    d = desc()
    d.w += 4                                                # a misaligned image
    refused(d)
    d = desc()
    d.y_line += 2                                           # output rows that are no 16-byte segments
    refused(d)
    refused(desc(113))                                      # one row and its border do not fit the staged patch
    d = desc()
    d.fm_ref = other.data_ptr()                             # the feature-matching term is the (3, 9) kernels'
    refused(d)
    d = desc()
    d.mask_src, d.mask_slope, d.bias = other.data_ptr(), SLOPE, bias.data_ptr()    # both roles at once
    refused(d)
    for p in (0, 1, 2, 5):                                  # every other precision
        d = desc()
        d.precision = p
        refused(d)
    assert lib.f2g_conv33_fwd(C.byref(desc()), st) == 0     # (the descriptor itself is fine)
    torch.cuda.synchronize()
    assert not bool((y[:S * H * W_ * 32] == 7.0).any())
    gw = torch.zeros(32, 9 * 32, device=DEV)
    d = desc()
    d.y = other.data_ptr()                                  # the weight gradient's roles: y = gradient
    assert lib.f2g_conv33_wgrad(C.byref(d), gw.data_ptr(), st) == EINVAL
    torch.cuda.synchronize()
    assert bool((gw == 0.0).all())
    d.precision = 3
    assert lib.f2g_conv33_wgrad(C.byref(d), gw.data_ptr(), st) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 8. ops: tunables, counters, the launch of today
def test_ops_route_and_the_launch_with_the_tunables_off(ops):
    S, H, W_ = 3, 11, 13
    c = case(S, H, W_)
    wp, wf = (torch.nn.Parameter(g(t)) for t in packed(W33))
    xg, gg, bias = g(c["x"]).view(-1, 32), g(c["gy"]).view(-1, 32), g(B)

    def both():
        y = torch.full((S * H * W_, 32), 7.0, device=DEV)
        gx = torch.full((S * H * W_, 32), 7.0, device=DEV)
        n = ops.FP16X3_CONV33_FWD_LAUNCHES, ops.FP16X3_CONV33_DGRAD_LAUNCHES
        ops.conv33(xg, S, H, W_, wp, bias, SLOPE, y)
        ops.conv33(gg, S, H, W_, wf, None, 0.0, gx, form=1)
        torch.cuda.synchronize()
        return y, gx, ops.FP16X3_CONV33_FWD_LAUNCHES - n[0], ops.FP16X3_CONV33_DGRAD_LAUNCHES - n[1]

    def precision3():
        """today's launch, spelled out: precision 3 over the three-piece images"""
        lib, st = ops.L.lib, ops.L.stream_ptr()
        outs = []
        for src, w, b, slope in ((xg, wp, bias, SLOPE), (gg, wf, None, 0.0)):
            out = torch.full((S * H * W_, 32), 7.0, device=DEV)
            i3 = ops.x3_image(w.detach())
            d = ops.L.Conv32Desc()
            d.S, d.H, d.Win, d.Wout, d.precision = S, H, W_, W_, 3
            d.x, d.x_seq, d.x_line = src.data_ptr(), H * W_ * 32, W_ * 32
            d.w, d.bias, d.lrelu_slope = i3.data_ptr(), (b.data_ptr() if b is not None else None), slope
            d.y, d.y_seq, d.y_line = out.data_ptr(), H * W_ * 32, W_ * 32
            assert lib.f2g_conv33_fwd(C.byref(d), st) == 0
            torch.cuda.synchronize()
            outs.append(out)
        return outs

    y, gx, nf, nd = both()
    assert (nf, nd) == (1, 1)
    close(y, c["y"], c["y_tol"], "ops forward")
    close(gx, c["gx"], c["gx_tol"], "ops data gradient")
    y3, gx3 = precision3()
    ops.FP16X3_CONV33_FWD = False                           # one tunable at a time
    y, gx, nf, nd = both()
    assert (nf, nd) == (0, 1) and torch.equal(y, y3)
    ops.FP16X3_CONV33_FWD, ops.FP16X3_CONV33_DGRAD = True, False
    y, gx, nf, nd = both()
    assert (nf, nd) == (1, 0) and torch.equal(gx, gx3)
    ops.FP16X3_CONV33_DGRAD = True
    ops.set_gemm_precision("bf16x6")                        # the tunables mean nothing outside the fp16x3 mode
    y, gx, nf, nd = both()
    assert (nf, nd) == (0, 0) and torch.equal(y, y3) and torch.equal(gx, gx3)


# ------------------------------------------------------------------ 9. the cached image follows its weight
def test_weight_image_follows_its_weight(ops):
    """the MRD's chains: the forward image hangs under the packed copy of the conv weight (pack -> f16x2seq), the data
    gradient's under the flipped / transposed matrix (dgrad33 -> f16x2seq).  After a raw-pointer update
    (bump_weight_epoch + the batched rebuild_derived) and after an in-place update the image and its scale equal the
    emulation's and the output moves."""
    from flow2gan_amd import fused_disc as FD
    S, H, W_ = 2, 9, 13
    c = case(S, H, W_)
    w = torch.nn.Parameter(g(W33.clone()))

    def build_f(t):                                         # (fused_disc._conv2d_dgrad's re-layout)
        out = ops.empty(32, 9 * 32, device=t.device)
        ops.permute4(out, t, (32, 9, 32, 1), (9, -1, 32 * 9, 0), in_offset=8)
        return out

    def launch_and_check(what):
        wp, wf = ops.derived(w, "pack", FD.pack_conv_weight), ops.derived(w, "dgrad33", build_f)
        y = run_fwd(ops, c["x"], wp)
        gx = run_dgrad(ops, c["gy"], wf)
        torch.cuda.synchronize()
        wc = w.detach().cpu()
        close(y, ref_fwd(c["x"], wc, B), tol_fwd(c["x"], wc, B), f"forward, {what}")
        close(gx, ref_dgrad(c["gy"], wc), tol_dgrad(c["gy"], wc), f"data gradient, {what}")
        for lay, host in zip((wp, wf), packed(wc)):
            assert torch.equal(lay.cpu().reshape(host.shape), host), f"{what}: the re-laid copy is stale"
            buf = ops.conv32_f16_image(lay).cpu()
            assert buf.numel() == 9216 + 1
            want_img, want_rs = emul.weight_image(host)
            assert torch.equal(buf[:9216].view(torch.int32), want_img), f"{what}: the cached image is stale"
            assert torch.equal(buf[9216:], want_rs), f"{what}: the cached scale is stale"
        return y.clone(), gx.clone()

    def update(w):
        w.data.copy_(w.detach() * 37.0 + 0.01)              # (the matrix's scale must move too)

    image_follows_weight(ops, w, launch_and_check, update=update, min_replays=2)


# ------------------------------------------------------------------ 10. one MRD resolution against the CPU oracle
def test_mrd_resolution_against_oracle(ops):
    """one resolution's sub-discriminator at the shapes of tests/test_hip_disc_autograd.py, the (3, 9) and the (3, 3)
    fp16x3 tunables all on: scores, feature maps, the input gradient and every parameter gradient against the oracle
    at that file's tolerance; both (3, 3) counters move with the tunables on and stand still with them off"""
    ops.FP16X3_CONV32_FWD = ops.FP16X3_CONV32_DGRAD = ops.FP16X3_CONV32_WGRAD = True
    counters = ("FP16X3_CONV33_FWD_LAUNCHES", "FP16X3_CONV33_DGRAD_LAUNCHES")
    r = subdisc_against_oracle(ops, "mrd", counters, "mrd resolution, fp16x3 band convolutions")
    nf, nd = (f + b for f, b in zip(r.fwd, r.bwd))
    print(f"[conv33 fp16x3] window {r.sub.window_length}: {nf} forward and {nd} data-gradient launches")
    assert nf > 0 and nd > 0
    ops.FP16X3_CONV33_FWD = ops.FP16X3_CONV33_DGRAD = False
    assert r.rerun() == ((0, 0), (0, 0))
