"""Host-side checks of the fp16x3 weight gradient of the MRD band convolutions (csrc/conv32h3w.hip): the error bound
of the arithmetic with one monotone running scale per operand and block, over the emulation
(tests/fp16x3_conv32w_emul.py), the walk of the running scales, and the Python-side tunable and counter.

The bound, per output:  3 * 2^-22 sum |g||x| + 2^-28 sum_T (xrun_T sum_{px in T} |g| + grun_T sum_{px in T} |x|).  The
second term is the floor of tests/fp16x3_conv32_emul.py with the block's running maximum in place of the tile's own.
"""
import functools

import pytest
import torch

import fp16x3_conv32w_emul as emul
from test_fp16x3_conv32_host import FAMILIES, SHAPES, family


@functools.lru_cache(maxsize=None)
def figures(name, S, H, Win, quiet_windows=False):
    """(worst error / bound, worst error / relative term alone, worst error where sum |g||x| = 0).  quiet_windows: the
    gradient is a normal map that is zero outside the output columns whose whole window lies in the quiet columns of
    x, so that an output's sum holds nothing but quiet pixels of x."""
    Wout = emul.wout_of(Win)
    x, g = family(name, S, H, Win, 11), family(name, S, H, Wout, 14)
    if quiet_windows:
        g = family("normal", S, H, Wout, 14)
        g[:, :, (2 * torch.arange(Wout) + 4) >= max(1, (2 * Win) // 3)] = 0.0
    got, want = emul.wgrad(x, g, name.endswith("flushed")), emul.exact_wgrad(x, g)
    bnd, mag = emul.bound_wgrad(x, g)
    assert got.shape == want.shape == bnd.shape == (32, 27 * 32)
    err = (got - want).abs()
    ok = mag > 0
    return (float((err[ok] / bnd[ok]).max()), float((err[ok] / (emul.BOUND * mag[ok])).max()),
            float(err[~ok].max()) if bool((~ok).any()) else 0.0)


@pytest.mark.parametrize("S,H,Win", SHAPES)
@pytest.mark.parametrize("name", FAMILIES)
def test_bound_holds(name, S, H, Win):
    of_bound, of_rel, err_silent = figures(name, S, H, Win)
    print(f"[conv32 fp16x3 wgrad] {name} {(S, H, Win)}: {of_bound:.3f} of the bound, {of_rel:.3f} of 3 * 2^-22 alone")
    assert of_bound <= 1.0, (name, of_bound)
    assert err_silent == 0.0, name


@pytest.mark.parametrize("S,H,Win", SHAPES)
def test_quiet_windows_need_the_floor_term(S, H, Win):
    """Pixels that are quiet against the rest of their patch exceed the relative term: the floor is not slack.  A
    weight gradient sums over EVERY pixel of the map, so with both operands of a quiet family the loud columns carry
    every output (0.149 and 0.048 of the relative term at the two shapes); the quiet columns of x show only where the
    gradient is silent over the loud ones.  There the bound still holds, through its floor term alone."""
    for name in ("quiet", "quiet_flushed"):
        of_bound, of_rel, err_silent = figures(name, S, H, Win, True)
        print(f"[conv32 fp16x3 wgrad] {name} {(S, H, Win)}, quiet windows: {of_bound:.3f} of the bound, {of_rel:.3g} of "
              f"3 * 2^-22 alone")
        assert of_rel > 1.0, (name, of_rel)
        assert of_bound <= 1.0 and err_silent == 0.0, (name, of_bound)


def test_bound_holds_where_blocks_walk_several_tiles():
    """(300, 8, 15): one 8 x 16 tile per sequence, 300 tiles on 150 blocks of two; sequences many binades apart, so
    the second tile of a block runs under its block's running maximum as often as under its own"""
    S, H, Win = 300, 8, 15
    Wout = emul.wout_of(Win)
    gen = torch.Generator().manual_seed(5)
    sc = torch.ldexp(torch.ones(S), (7 * torch.arange(S)) % 41 - 20)[:, None, None, None]
    x = torch.randn(S, H, Win, 32, generator=gen) * sc
    g = torch.randn(S, H, Wout, 32, generator=gen) * sc.flip(0)
    assert emul.walk(x, g)["per"] == 2
    bnd, mag = emul.bound_wgrad(x, g)
    err = (emul.wgrad(x, g) - emul.exact_wgrad(x, g)).abs()
    print(f"[conv32 fp16x3 wgrad] walks of two tiles: {float((err / bnd).max()):.3f} of the bound")
    assert bool((err <= bnd).all())


def test_emulation_agrees_with_float64_on_exact_inputs():
    """small integers split exactly under any power-of-two scale: tile pick, patch extents, the walk and the layout
    of the result have no room to hide behind a tolerance (both tile shapes, partial tiles, degenerate widths)"""
    for S, H, Win in SHAPES + [(1, 5, 2), (2, 9, 1), (1, 17, 35)]:
        gen = torch.Generator().manual_seed(H)
        Wout = emul.wout_of(Win)
        x = torch.randint(-8, 9, (S, H, Win, 32), generator=gen).float()
        g = torch.randint(-8, 9, (S, H, Wout, 32), generator=gen).float()
        assert torch.equal(emul.wgrad(x, g), emul.exact_wgrad(x, g)), (S, H, Win)
    assert emul.pick_tiles(9, 11)[:2] == (8, 16) and emul.pick_tiles(16, 20)[:2] == (16, 8)


def test_the_running_scale_only_falls():
    """(300, 8, 31): 300 tiles of 8 x 16 on 150 blocks of two consecutive sequences.  Even blocks walk a quiet tile,
    then a loud one: the loud tile lowers the scale.  Odd blocks walk loud, then quiet: the quiet tile keeps the loud
    tile's scale.  A zero tile and a NaN tile leave the scale in force; every block starts at scale 1."""
    S, H, Win = 300, 8, 31
    x = torch.ones(S, H, Win, 32)
    g = torch.ones(S, H, emul.wout_of(Win), 32)
    quiet, loud = 2.0 ** -10, 2.0 ** 5
    x[0::4], x[1::4], x[2::4], x[3::4] = quiet, loud, loud, quiet
    g[8], g[11] = 0.0, float("nan")            # the first tile of block 4; the second tile of block 5
    w = emul.walk(x, g)
    assert (w["per"], w["blocks"], w["th"], w["tw"]) == (2, 150, 8, 16)
    sx = w["sx"].view(150, 2)
    assert sx[0::2].tolist() == [[24, 9]] * 75           # quiet, then loud: 2^(14 + 10), then 2^(14 - 5)
    assert sx[1::2].tolist() == [[9, 9]] * 75            # loud, then quiet: the scale does not rise
    assert bool((sx[:, 1] <= sx[:, 0]).all())
    sg = w["sg"].view(150, 2)
    assert sg[4].tolist() == [0, 14] and sg[5].tolist() == [14, 14]    # the zero tile: scale 1; the NaN tile: in force
    assert sg[0].tolist() == [14, 14]
    assert w["xrun"].view(150, 2)[1].tolist() == [loud, loud] and w["xrun"].view(150, 2)[0].tolist() == [quiet, loud]


def test_partition():
    assert emul.partition(12) == (1, 12) and emul.partition(256) == (1, 256) and emul.partition(257) == (2, 129)
    assert emul.partition(510) == (2, 255) and emul.partition(630) == (3, 210)


def test_tunable_and_counter():
    import os
    from flow2gan_amd import _lib, _opts, ops
    assert "fp16x3_conv32_wgrad" in _opts._ASKED and "fp16x3_conv32_wgrad" in _opts.__doc__
    if "fp16x3_conv32_wgrad" not in os.environ.get("F2G_OPTS", "").lower():
        assert ops.FP16X3_CONV32_WGRAD is False
    assert isinstance(ops.FP16X3_CONV32_WGRAD_LAUNCHES, int)
    assert "f2g_conv32_s2_wgrad_h3" in _lib.EXPORTS
