"""Host-side checks of the fp16x3 MRD band convolutions (csrc/conv32h3.hip): the error bound of the arithmetic with
one scale per tile patch and one for the whole weight matrix, over the emulation (tests/fp16x3_conv32_emul.py), and
the Python-side tunables and counters.

The bound, per output:  3 * 2^-22 sum |a||w| + 2^-28 (amax_patch sum_k |w_k| + wmax sum_k |a_k|).  The second term
is the floor of tests/fp16x3_seq_emul.py with the tile's patch in place of the sequence, and its mirror image for the
weight: an element 2^-28 below its patch's (matrix's) largest is subnormal in hi.
"""
import functools

import pytest
import torch

import fp16x3_conv32_emul as emul

SHAPES = [(2, 9, 21), (3, 16, 40)]      # (S, H, Win): one partial 8 x 16 tile per map; 16 x 8 tiles, three per row
FAMILIES = ["normal", "binades", "decades", "quiet", "quiet_flushed"]


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def family(name, S, H, W, seed):
    """a map (S, H, W, 32) of the family"""
    x = rnd(S, H, W, 32, seed=seed)
    gen = torch.Generator().manual_seed(seed + 1)
    if name == "binades":            # element exponents over 40 binades
        x = x * torch.ldexp(torch.ones_like(x), torch.randint(-20, 21, x.shape, generator=gen))
    elif name == "decades":          # rows, columns and sequences decades apart
        x = x * (10.0 ** (3 * torch.arange(S) - 3))[:, None, None, None]
        x = x * (10.0 ** (torch.arange(H) % 4 - 2))[None, :, None, None]
        x = x * (10.0 ** (torch.arange(W) % 5 - 2))[None, None, :, None]
    elif name.startswith("quiet"):   # columns 2^-34 below the rest of their patch: whole windows lie inside them
        q = torch.ones(W)
        q[:max(1, (2 * W) // 3)] = 2.0 ** -34
        x = x * q[None, None, :, None]
    return x


@functools.lru_cache(maxsize=None)
def weight(name):
    w = rnd(32, 32, 3, 9, seed=2) * 0.05
    if name == "binades":
        gen = torch.Generator().manual_seed(4)
        w = w * torch.ldexp(torch.ones_like(w), torch.randint(-20, 21, w.shape, generator=gen))
    return w


@functools.lru_cache(maxsize=None)
def figures(name, S, H, Win):
    """(worst error / bound, worst error / relative term alone) of the forward and of the data gradient"""
    w, flush = weight(name), name.endswith("flushed")
    Wout = emul.wout_of(Win)
    x, g = family(name, S, H, Win, 11), family(name, S, H, Wout, 14)
    out = {}
    for what, got, want, (bnd, mag) in (
            ("forward", emul.fwd(x, w, flush), emul.exact_fwd(x, w), emul.bound_fwd(x, w)),
            ("data gradient", emul.dgrad(g, w, Win, flush), emul.exact_dgrad(g, w, Win), emul.bound_dgrad(g, w, Win))):
        assert got.shape == want.shape == bnd.shape
        err = (got - want).abs()
        ok = mag > 0
        out[what] = (float((err[ok] / bnd[ok]).max()), float((err[ok] / (emul.BOUND * mag[ok])).max()),
                     float(err[~ok].max()) if bool((~ok).any()) else 0.0)
    return out


@pytest.mark.parametrize("S,H,Win", SHAPES)
@pytest.mark.parametrize("name", FAMILIES)
def test_bound_holds(name, S, H, Win):
    for what, (of_bound, of_rel, err_silent) in figures(name, S, H, Win).items():
        print(f"[conv32 fp16x3] {name} {(S, H, Win)} {what}: {of_bound:.3f} of the bound, {of_rel:.3f} of 3 * 2^-22 alone")
        assert of_bound <= 1.0, (name, what, of_bound)
        assert err_silent == 0.0, (name, what)


@pytest.mark.parametrize("S,H,Win", SHAPES)
def test_quiet_windows_need_the_floor_term(S, H, Win):
    """windows that are quiet against the rest of their patch exceed the relative term: the floor is not slack"""
    for name in ("quiet", "quiet_flushed"):
        for what, (of_bound, of_rel, _) in figures(name, S, H, Win).items():
            assert of_rel > 1.0, (name, what, of_rel)


def test_emulation_agrees_with_float64_on_exact_inputs():
    """small integers in patch and weights split exactly: tile pick, patch extents and the untiling have no room to
    hide behind a tolerance (both tile shapes, partial tiles on every edge, both column parities)"""
    for S, H, Win in SHAPES + [(1, 5, 2), (2, 9, 1), (1, 17, 35)]:
        gen = torch.Generator().manual_seed(H)
        Wout = emul.wout_of(Win)
        x = torch.randint(-8, 9, (S, H, Win, 32), generator=gen).float()
        g = torch.randint(-8, 9, (S, H, Wout, 32), generator=gen).float()
        w = torch.randint(-8, 9, (32, 32, 3, 9), generator=gen).float()
        assert torch.equal(emul.fwd(x, w), emul.exact_fwd(x, w))
        assert torch.equal(emul.dgrad(g, w, Win), emul.exact_dgrad(g, w, Win))


def test_tile_pick():
    assert emul.pick_tiles(24, 32) == (8, 16, 3, 2) and emul.pick_tiles(47, 20) == (16, 8, 3, 3)
    assert emul.pick_tiles(47, 39) == (16, 8, 3, 5)          # (48 x 40 pixels against 48 x 48)
    assert emul.pick_tiles(9, 11) == (8, 16, 2, 1) and emul.pick_tiles(16, 8) == (16, 8, 1, 1)


def test_tunables_and_counters():
    from flow2gan_amd import _opts, ops
    for name in ("fp16x3_conv32_fwd", "fp16x3_conv32_dgrad"):
        assert name in _opts._ASKED and name in _opts.__doc__
    import os
    if "fp16x3_conv32" not in os.environ.get("F2G_OPTS", "").lower():
        assert ops.FP16X3_CONV32_FWD is False and ops.FP16X3_CONV32_DGRAD is False
    assert isinstance(ops.FP16X3_CONV32_FWD_LAUNCHES, int) and isinstance(ops.FP16X3_CONV32_DGRAD_LAUNCHES, int)
