"""Host-side checks of the fp16x3 weight gradient of the (3, 3) MRD band layer (csrc/conv33h3w.hip): the error bound of
the arithmetic with one monotone running scale per operand and block, over the emulation
(tests/fp16x3_conv33w_emul.py), the walk of the running scales, and the Python-side tunable and counter.

The bound, per output:  3 * 2^-22 sum |g||x| + 2^-28 sum_T (xrun_T sum_{px in T} |g| + grun_T sum_{px in T} |x|), the
bound of tests/fp16x3_conv32w_emul.py on the walk of conv33_wgrad6_kernel (block b takes the tiles b, b + grid, ...).
"""
import functools

import pytest
import torch

import fp16x3_conv33w_emul as emul
from test_fp16x3_conv32_host import FAMILIES, family as family32, rnd

# (S, H, W): R = 7, last tile of 5 rows; W = 7: R = 36, one partial tile; 300 tiles of 2 rows, blocks 0-43 walk two
SHAPES = [(3, 40, 33), (2, 37, 7), (150, 4, 86)]
SMALL = SHAPES[:2]
EXACT = [(3, 40, 33), (1, 3, 7), (1, 300, 1), (2, 5, 112), (300, 3, 112)]


def family(name, S, H, W, seed):
    """a map (S, H, W, 32) of the family (tests/test_fp16x3_conv32_host.py).  "decades" there sets sequence s 10^(3 s - 3)
    apart, which leaves float32 from s = 14 on: here the sequences' decades wrap at four (10^-3 .. 10^6; the same maps
    for S <= 4), so that the 150-sequence shape holds finite floats -- consecutive tiles of a block's walk (256 tiles
    apart) and the tiles of neighbouring blocks still lie decades apart."""
    if name != "decades":
        return family32(name, S, H, W, seed)
    x = rnd(S, H, W, 32, seed=seed)
    x = x * (10.0 ** (3 * (torch.arange(S) % 4) - 3))[:, None, None, None]
    x = x * (10.0 ** (torch.arange(H) % 4 - 2))[None, :, None, None]
    return x * (10.0 ** (torch.arange(W) % 5 - 2))[None, None, :, None]


@functools.lru_cache(maxsize=None)
def figures(name, S, H, W, quiet_windows=False):
    """(worst error / bound, worst error / relative term alone, worst error where sum |g||x| = 0).  quiet_windows: the
    gradient is a normal map that is zero wherever its 3-column window reaches a loud column of x, so that an output's
    sum holds nothing but quiet pixels of x."""
    x, g = family(name, S, H, W, 11), family(name, S, H, W, 14)
    if quiet_windows:
        g = family("normal", S, H, W, 14)
        g[:, :, (torch.arange(W) + 1) >= max(1, (2 * W) // 3)] = 0.0
    got, want = emul.wgrad(x, g, name.endswith("flushed")), emul.exact_wgrad(x, g)
    bnd, mag = emul.bound_wgrad(x, g)
    assert got.shape == want.shape == bnd.shape == (32, 9 * 32)
    err = (got - want).abs()
    ok = mag > 0
    return (float((err[ok] / bnd[ok]).max()), float((err[ok] / (emul.BOUND * mag[ok])).max()),
            float(err[~ok].max()) if bool((~ok).any()) else 0.0)


@pytest.mark.parametrize("S,H,W", SHAPES)
@pytest.mark.parametrize("name", FAMILIES)
def test_bound_holds(name, S, H, W):
    of_bound, of_rel, err_silent = figures(name, S, H, W)
    print(f"[conv33 fp16x3 wgrad] {name} {(S, H, W)}: {of_bound:.3f} of the bound, {of_rel:.3f} of 3 * 2^-22 alone")
    assert of_bound <= 1.0, (name, of_bound)
    assert err_silent == 0.0, name


@pytest.mark.parametrize("S,H,W", SMALL)
def test_quiet_windows_need_the_floor_term(S, H, W):
    """Pixels that are quiet against the rest of their patch exceed the relative term: the floor is not slack.  A weight
    gradient sums over EVERY pixel of the map, so the quiet columns of x show only where the gradient is silent over the
    loud ones (tests/test_fp16x3_conv32w_host.py).  There the bound still holds, through its floor term alone."""
    for name in ("quiet", "quiet_flushed"):
        of_bound, of_rel, err_silent = figures(name, S, H, W, True)
        print(f"[conv33 fp16x3 wgrad] {name} {(S, H, W)}, quiet windows: {of_bound:.3f} of the bound, {of_rel:.3g} of "
              f"3 * 2^-22 alone")
        assert of_rel > 1.0, (name, of_rel)
        assert of_bound <= 1.0 and err_silent == 0.0, (name, of_bound)


def test_quiet_windows_hold_the_bound_where_blocks_walk_two_tiles():
    S, H, W = SHAPES[2]
    for name in ("quiet", "quiet_flushed"):
        of_bound, of_rel, err_silent = figures(name, S, H, W, True)
        print(f"[conv33 fp16x3 wgrad] {name} {(S, H, W)}, quiet windows: {of_bound:.3f} of the bound, {of_rel:.3g} of "
              f"3 * 2^-22 alone")
        assert of_bound <= 1.0 and err_silent == 0.0, (name, of_bound)


@pytest.mark.parametrize("S,H,W", EXACT)
def test_emulation_agrees_with_float64_on_exact_inputs(S, H, W):
    """small integers split exactly under any power-of-two scale: row pick, patch extents, the walk and the layout of
    the result have no room to hide behind a tolerance (a partial last tile, H < R, W = 1, W = 112, walks of four
    tiles)"""
    gen = torch.Generator().manual_seed(H)
    x = torch.randint(-8, 9, (S, H, W, 32), generator=gen).float()
    g = torch.randint(-8, 9, (S, H, W, 32), generator=gen).float()
    assert torch.equal(emul.wgrad(x, g), emul.exact_wgrad(x, g)), (S, H, W)


def test_exact_wgrad_is_autograds():
    S, H, W = 2, 9, 13
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(S, H, W, 32, generator=gen, dtype=torch.float64)
    g = torch.randn(S, H, W, 32, generator=gen, dtype=torch.float64)
    conv = torch.nn.Conv2d(32, 32, (3, 3), padding=(1, 1)).double()
    conv(x.permute(0, 3, 1, 2)).backward(g.permute(0, 3, 1, 2))
    want = conv.weight.grad                                            # (co, ci, 3, 3)
    got = emul.exact_wgrad(x, g).view(32, 3, 3, 32).permute(0, 3, 1, 2)  # [co][tap][ci] -> (co, ci, kh, kw)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)


def test_the_running_scale_follows_the_walk():
    """(300, 2, 86): R = 2, one tile per sequence, 300 tiles on 256 blocks: block b < 44 walks the tiles b and b + 256.
    A later louder tile lowers the scale, a later quieter one keeps it, a zero tile and a NaN tile leave the scale in
    force; every block starts at scale 1."""
    S, H, W = 300, 2, 86
    x, g = torch.ones(S, H, W, 32), torch.ones(S, H, W, 32)
    quiet, loud = 2.0 ** -10, 2.0 ** 5
    x[:256], x[256:] = quiet, loud
    x[1], x[257] = loud, quiet
    g[2], g[259] = 0.0, float("nan")
    w = emul.walk(x, g)
    assert (w["R"], w["nh"], w["grid"], w["steps"]) == (2, 1, 256, 2)
    sx, sg = w["sx"], w["sg"]
    assert (int(sx[0]), int(sx[256])) == (24, 9)             # quiet, then loud: 2^(14 + 10), then 2^(14 - 5)
    assert (int(sx[1]), int(sx[257])) == (9, 9)              # loud, then quiet: the scale does not rise
    assert (int(sg[2]), int(sg[258])) == (0, 14)             # the zero tile: scale 1
    assert (int(sg[3]), int(sg[259])) == (14, 14)            # the NaN tile: the scale in force
    assert int(sx[100]) == 24 and float(w["xrun"][256]) == loud and float(w["xrun"][257]) == loud


def test_partition():
    assert emul.partition(1) == (1, 1) and emul.partition(256) == (256, 1)
    assert emul.partition(257) == (256, 2) and emul.partition(520) == (256, 3)
    assert emul.block_tiles(1, 0) == [0] and emul.block_tiles(256, 255) == [255]
    assert emul.block_tiles(257, 0) == [0, 256] and emul.block_tiles(257, 1) == [1]
    assert emul.block_tiles(520, 7) == [7, 263, 519] and emul.block_tiles(520, 8) == [8, 264]
    assert emul.pick_rows(40, 33) == 7 and emul.pick_rows(4, 86) == 2 and emul.pick_rows(300, 1) == 115


def test_tunable_and_counter():
    import os
    from flow2gan_amd import _lib, _opts, ops
    assert "fp16x3_conv33_wgrad" in _opts._ASKED and "fp16x3_conv33_wgrad" in _opts.__doc__
    if "fp16x3_conv33_wgrad" not in os.environ.get("F2G_OPTS", "").lower():
        assert ops.FP16X3_CONV33_WGRAD is False
    assert isinstance(ops.FP16X3_CONV33_WGRAD_LAUNCHES, int)
    assert "f2g_conv33_wgrad_h3" in _lib.EXPORTS
