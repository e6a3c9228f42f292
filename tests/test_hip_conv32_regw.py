"""conv32x6.hip, fp32-class MRD band convolutions with the weight fragments held in registers for a
block's whole life: the reduction of a tile is split by k step (tap, input-channel half) over the block's
waves, and the waves' partial tiles meet through LDS in a fixed order.

What that structure can get wrong, at the smallest shapes that show it: the wrong fragment held by a wave
or a wrong patch offset (one k step at a time), weights or partial sums surviving from tile to tile or
from launch to launch (uneven tile walks, two launches), blocks with less than one tile per wave's worth
of work, the reduction's order (bit-reproducible), and the strided / offset gradient input with every
epilogue as fused_disc calls the data gradient.

Reference: float64 conv2d / its autograd.  Tolerances: max error <= rtol * max|want| with rtol = 2e-5 for
forward and data gradient (the exact-fp32 bar the fp32-class instances are held to) and 1e-4 for column
sums.  Shapes are (S, H, Win); Wout = (Win - 1) // 2 + 1.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from flow2gan_amd import ops as o
    was = o.GEMM_PRECISION, o.FP16X3
    o.set_gemm_precision("bf16x6")
    yield o
    o.GEMM_PRECISION, o.FP16X3 = was


def g(t):
    return t.to(DEV).contiguous()


def close(got, want, rtol=2e-5, name=""):
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = want.abs().max().item() + 1e-30
    err = (got - want).abs().max().item()
    assert err <= rtol * scale + 1e-30, f"{name}: max err {err:.3e} vs scale {scale:.3e}"


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


SLOPE = 0.1
W = rnd(32, 32, 3, 9, seed=2, scale=0.05)          # [co][ci][dh][j]
B = rnd(32, seed=3)


def packed(w):
    """(forward matrix [co][tap][ci], data-gradient tiles [tap][ci][co])"""
    return (w.permute(0, 2, 3, 1).reshape(32, 27 * 32).contiguous(),
            w.permute(2, 3, 1, 0).reshape(27, 32, 32).contiguous())


def ref_fwd(x, S, H, Win, w, b):
    y = F.conv2d(x.reshape(S, H, Win, 32).permute(0, 3, 1, 2).double(), w.double(), b.double(), stride=(1, 2),
                 padding=(1, 4))
    return F.leaky_relu(y, SLOPE).permute(0, 2, 3, 1).reshape(-1, 32)


def ref_dgrad(gy, S, H, Win, w):
    Wout = (Win - 1) // 2 + 1
    x = torch.zeros(S, 32, H, Win, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), None, stride=(1, 2), padding=(1, 4)).backward(
        gy.reshape(S, H, Wout, 32).permute(0, 3, 1, 2).double())
    return x.grad.permute(0, 2, 3, 1).reshape(-1, 32)


@functools.lru_cache(maxsize=None)
def case(S, H, Win, seed=0):
    """Inputs and float64 references of one shape with the module's weights: computed once, shared, not modified."""
    Wout = (Win - 1) // 2 + 1
    x = rnd(S * H * Win, 32, seed=11 + seed)
    gy = rnd(S * H * Wout, 32, seed=14 + seed)
    yact = rnd(S * H * Win, 32, seed=15 + seed)
    yact = torch.where(yact > 0, yact, SLOPE * yact)       # an activation map: leaky_relu(pre)
    gref = ref_dgrad(gy, S, H, Win, W)
    return dict(x=x, gy=gy, yact=yact, y=ref_fwd(x, S, H, Win, W, B), gx=gref,
                gm=gref * torch.where(yact > 0, 1.0, SLOPE).double())


def run_fwd(ops, x, S, H, Win, wp, b=B):
    Wout = (Win - 1) // 2 + 1
    y = torch.full((S * H * Wout, 32), 7.0, device=DEV)
    ops.conv32_s2_fwd(g(x), S, H, Win, Wout, wp, g(b), SLOPE, y)
    return y


def run_dgrad(ops, gy, S, H, Win, wT, **kw):
    Wout = (Win - 1) // 2 + 1
    gx = torch.full((S * H * Win, 32), 7.0, device=DEV)
    ops.conv32_s2_dgrad(g(gy), S, H, Win, Wout, wT, gx, **kw)
    return gx


def test_one_k_step_at_a_time(ops):
    """All weights zero except one (tap, input-channel half) of the 54: the WHOLE result is compared, so a wave
    holding another k step's fragment, a wrong patch offset, or a contribution from a k step that should be
    silent all fail.  (2, 9, 21): a partial tile on every edge."""
    S, H, Win = 2, 9, 21
    c = case(S, H, Win)
    for tap in range(27):
        for half in range(2):
            w = torch.zeros_like(W)
            w[:, 16 * half:16 * half + 16, tap // 9, tap % 9] = W[:, 16 * half:16 * half + 16, tap // 9, tap % 9]
            wp, wT = packed(w)
            close(run_fwd(ops, c["x"], S, H, Win, g(wp)), ref_fwd(c["x"], S, H, Win, w, B),
                  name=f"forward, tap {tap} half {half}")
            close(run_dgrad(ops, c["gy"], S, H, Win, g(wT)), ref_dgrad(c["gy"], S, H, Win, w),
                  name=f"data gradient, tap {tap} input half {half}")
            # (the data gradient reduces over co: ITS k-step halves are halves of the output channels)
            w = torch.zeros_like(W)
            w[16 * half:16 * half + 16, :, tap // 9, tap % 9] = W[16 * half:16 * half + 16, :, tap // 9, tap % 9]
            wp, wT = packed(w)
            close(run_dgrad(ops, c["gy"], S, H, Win, g(wT)), ref_dgrad(c["gy"], S, H, Win, w),
                  name=f"data gradient, tap {tap} output half {half}")


@pytest.mark.parametrize("S,H,Win", [(34, 47, 77), (70, 47, 39)])
def test_weights_held_across_tiles_and_launches(ops, S, H, Win):
    """(34, 47, 77): 612 tiles of 8 x 16 on 256 blocks -- 100 blocks walk three tiles, 156 two; (70, 47, 39):
    Wout = 20 picks the 16 x 8 tile, 630 tiles.  Forward, plain and masked data gradient with column sums; then
    the same weights with a second, different input in a second launch: nothing of launch one may survive."""
    wp, wT = (g(t) for t in packed(W))
    for seed in (0, 1):
        c = case(S, H, Win, seed)
        close(run_fwd(ops, c["x"], S, H, Win, wp), c["y"], name=f"forward, launch {seed}")
        close(run_dgrad(ops, c["gy"], S, H, Win, wT), c["gx"], name=f"data gradient, launch {seed}")
        cs = torch.zeros(32, device=DEV)
        gm = run_dgrad(ops, c["gy"], S, H, Win, wT, mask=(g(c["yact"]), 0, SLOPE), colsum=cs)
        close(gm, c["gm"], name=f"masked data gradient, launch {seed}")
        close(cs, c["gm"].sum(0), rtol=1e-4, name=f"column sums, launch {seed}")


@pytest.mark.parametrize("S,H,Win", [(1, 5, 2), (2, 9, 1), (2, 16, 16), (2, 8, 64)])
def test_few_tiles_and_degenerate_widths(ops, S, H, Win):
    """One partial tile with Wout = 1; Win = 1 (the odd column parity is empty); tile-exact 16 x 8 and 8 x 16."""
    wp, wT = (g(t) for t in packed(W))
    c = case(S, H, Win)
    close(run_fwd(ops, c["x"], S, H, Win, wp), c["y"], name="forward")
    close(run_dgrad(ops, c["gy"], S, H, Win, wT), c["gx"], name="data gradient")
    cs = torch.zeros(32, device=DEV)
    gm = run_dgrad(ops, c["gy"], S, H, Win, wT, mask=(g(c["yact"]), 0, SLOPE), colsum=cs)
    close(gm, c["gm"], name="masked data gradient")
    close(cs, c["gm"].sum(0), rtol=1e-4, name="column sums")


def test_fixed_reduction_order_is_bit_reproducible(ops):
    """The waves' partial tiles are summed in a fixed order without atomics: two runs agree bit for bit.  (The
    column sums use atomics and are not compared this way.)"""
    S, H, Win = 34, 47, 77
    wp, wT = (g(t) for t in packed(W))
    c = case(S, H, Win)
    assert torch.equal(run_fwd(ops, c["x"], S, H, Win, wp), run_fwd(ops, c["x"], S, H, Win, wp))
    assert torch.equal(run_dgrad(ops, c["gy"], S, H, Win, wT), run_dgrad(ops, c["gy"], S, H, Win, wT))


@pytest.mark.parametrize("S,H,Win", [(3, 11, 13), (24, 94, 77)])
def test_strided_offset_gradient_with_every_epilogue(ops, S, H, Win):
    """The data gradient reads a band's slice of a wider concatenated map (g_off, g_line, g_seq set), as
    fused_disc calls it: mask only, then mask plus the feature-matching term, both with column sums."""
    Wout = (Win - 1) // 2 + 1
    wp, wT = (g(t) for t in packed(W))
    c = case(S, H, Win)
    lo, Wtot = 5, Wout + 9                                  # the band's first column / the map's width
    wide = rnd(S, H, Wtot, 32, seed=21)
    wide[:, :, lo:lo + Wout] = c["gy"].reshape(S, H, Wout, 32)
    yreal = rnd(S * H * Win, 32, seed=16)
    wdev = torch.tensor([0.7])
    for use_fm in (False, True):
        want = c["gx"].clone()
        if use_fm:
            want = want + 0.25 * 0.7 * torch.sign(c["yact"].double() - yreal.double())
        want = want * torch.where(c["yact"] > 0, 1.0, SLOPE).double()
        cs = torch.zeros(32, device=DEV)
        gx = torch.full((S * H * Win, 32), 7.0, device=DEV)
        ops.conv32_s2_dgrad(g(wide), S, H, Win, Wout, wT, gx, g_seq=H * Wtot * 32, g_line=Wtot * 32, g_off=lo * 32,
                            mask=(g(c["yact"]), 0, SLOPE), fm=(g(yreal), 0, 0.25, g(wdev)) if use_fm else None,
                            colsum=cs)
        close(gx, want, name=f"strided data gradient (fm={use_fm})")
        close(cs, want.sum(0), rtol=1e-4, name=f"column sums (fm={use_fm})")
