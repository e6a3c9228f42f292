"""Host-side checks of the fp16x3 (3, 3) fifth layer of an MRD band stack (csrc/conv33h3.hip): the error bound of the
arithmetic with one scale per whole-row tile patch and one for the whole weight matrix, over the emulation
(tests/fp16x3_conv33_emul.py), the row pick, and the Python-side tunables and counters.

The bound, per output:  3 * 2^-22 sum |a||w| + 2^-28 (amax_patch sum_k |w_k| + wmax sum_k |a_k|).  The second term
is the floor of tests/fp16x3_seq_emul.py with the tile's patch in place of the sequence, and its mirror image for the
weight: an element 2^-28 below its patch's (matrix's) largest is subnormal in hi.
"""
import functools

import pytest
import torch

import fp16x3_conv33_emul as emul

SHAPES = [(2, 40, 33), (2, 37, 7)]      # (S, H, W): R = 7, last tile five rows; R = 36, last tile one row
FAMILIES = ["normal", "binades", "decades", "quiet", "quiet_flushed"]


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def family(name, S, H, W, seed):
    """a map (S, H, W, 32) of the family (the families of tests/test_fp16x3_conv32_host.py)"""
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
    w = rnd(32, 32, 3, 3, seed=2) * 0.05
    if name == "binades":
        gen = torch.Generator().manual_seed(4)
        w = w * torch.ldexp(torch.ones_like(w), torch.randint(-20, 21, w.shape, generator=gen))
    return w


@functools.lru_cache(maxsize=None)
def figures(name, S, H, W):
    """(worst error / bound, worst error / relative term alone, worst error where the bound is zero) of the forward
    and of the data gradient"""
    w, flush = weight(name), name.endswith("flushed")
    x, g = family(name, S, H, W, 11), family(name, S, H, W, 14)
    out = {}
    for what, got, want, (bnd, mag) in (
            ("forward", emul.fwd(x, w, flush), emul.exact_fwd(x, w), emul.bound_fwd(x, w)),
            ("data gradient", emul.dgrad(g, w, flush), emul.exact_dgrad(g, w), emul.bound_dgrad(g, w))):
        assert got.shape == want.shape == bnd.shape
        err = (got - want).abs()
        ok = mag > 0
        out[what] = (float((err[ok] / bnd[ok]).max()), float((err[ok] / (emul.BOUND * mag[ok])).max()),
                     float(err[~ok].max()) if bool((~ok).any()) else 0.0)
    return out


@pytest.mark.parametrize("S,H,W", SHAPES)
@pytest.mark.parametrize("name", FAMILIES)
def test_bound_holds(name, S, H, W):
    for what, (of_bound, of_rel, err_silent) in figures(name, S, H, W).items():
        print(f"[conv33 fp16x3] {name} {(S, H, W)} {what}: {of_bound:.3f} of the bound, {of_rel:.3f} of 3 * 2^-22 alone")
        assert of_bound <= 1.0, (name, what, of_bound)
        assert err_silent == 0.0, (name, what)


@pytest.mark.parametrize("S,H,W", SHAPES)
def test_quiet_windows_need_the_floor_term(S, H, W):
    """windows that are quiet against the rest of their patch exceed the relative term: the floor is not slack"""
    for name in ("quiet", "quiet_flushed"):
        for what, (of_bound, of_rel, _) in figures(name, S, H, W).items():
            assert of_rel > 1.0, (name, what, of_rel)


def test_emulation_agrees_with_float64_on_exact_inputs():
    """small integers in patch and weights split exactly: row pick, patch extents and the untiling have no room to
    hide behind a tolerance (partial last tiles, one tile, W = 1, W = 112)"""
    for S, H, W in SHAPES + [(1, 3, 7), (1, 300, 1), (2, 5, 112), (1, 16, 16)]:
        gen = torch.Generator().manual_seed(H)
        x = torch.randint(-8, 9, (S, H, W, 32), generator=gen).float()
        g = torch.randint(-8, 9, (S, H, W, 32), generator=gen).float()
        w = torch.randint(-8, 9, (32, 32, 3, 3), generator=gen).float()
        assert torch.equal(emul.fwd(x, w), emul.exact_fwd(x, w))
        assert torch.equal(emul.dgrad(g, w), emul.exact_dgrad(g, w))


def test_data_gradient_is_the_autograd_gradient():
    """exact_dgrad (the reference of the bound) is conv2d's own input gradient"""
    g, w = rnd(2, 9, 5, 32, seed=1), rnd(32, 32, 3, 3, seed=2)
    x = torch.zeros(2, 32, 9, 5, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x, w.double(), padding=(1, 1)).backward(g.permute(0, 3, 1, 2).double())
    assert torch.allclose(emul.exact_dgrad(g, w), x.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)


def test_row_pick():
    for (H, W), R in {(40, 33): 7, (37, 7): 36, (5, 112): 1, (3, 7): 3, (300, 1): 115, (300, 2): 86}.items():
        assert emul.pick_rows(H, W) == R, (H, W)


def test_tunables_and_counters():
    from flow2gan_amd import _opts, ops
    for name in ("fp16x3_conv33_fwd", "fp16x3_conv33_dgrad"):
        assert name in _opts._ASKED and name in _opts.__doc__
    import os
    if "fp16x3_conv33" not in os.environ.get("F2G_OPTS", "").lower():
        assert ops.FP16X3_CONV33_FWD is False and ops.FP16X3_CONV33_DGRAD is False
        # (with the tunables off nothing has moved the counters: they still stand where they start)
        assert ops.FP16X3_CONV33_FWD_LAUNCHES == 0 and ops.FP16X3_CONV33_DGRAD_LAUNCHES == 0
    assert isinstance(ops.FP16X3_CONV33_FWD_LAUNCHES, int) and isinstance(ops.FP16X3_CONV33_DGRAD_LAUNCHES, int)
