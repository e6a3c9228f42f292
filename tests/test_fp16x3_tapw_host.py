"""CPU: the arithmetic of the fp16x3 tap-walking weight gradient (tests/fp16x3_colswin_emul.py) against float64 at the
bound of tests/fp16x3_emul.py -- the taps shift rows of the halo map, so one power-of-two scale per column of the whole
map leaves every tap's sum over rows exactly and the per-product bound 3 * 2^-22 of |g| |x| is the column image's --
and the route's tunable."""
import pytest
import torch

import fp16x3_colswin_emul as win
import fp16x3_emul as emul

S, HIN, HALO, CIN, COUT = 3, 37, 2, 32, 24


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def spread(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.ldexp(torch.ones(*shape), torch.randint(-20, 1, shape, generator=g))


def halo(v):
    """(S, HIN, C) -> the flat halo layout (S * (HIN + 2 HALO), C) with zero halo rows"""
    out = torch.zeros(S, HIN + 2 * HALO, v.shape[2], dtype=v.dtype)
    out[:, HALO:HALO + HIN] = v
    return out.reshape(-1, v.shape[2])


CASES = {
    "randn": lambda: (rnd(S, HIN, COUT, seed=1), rnd(S, HIN, CIN, seed=2)),
    "elements_over_2^-20..1": lambda: (rnd(S, HIN, COUT, seed=3) * spread(S, HIN, COUT, seed=4),
                                       rnd(S, HIN, CIN, seed=5) * spread(S, HIN, CIN, seed=6)),
    "channels_over_decades": lambda: (rnd(S, HIN, COUT, seed=7) * torch.logspace(-30, 30, COUT)[None, None, :],
                                      rnd(S, HIN, CIN, seed=8) * torch.logspace(-30, 30, CIN)[None, None, :]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_emulated_tap_weight_gradient_is_within_the_bound(case):
    g, x = (halo(v) for v in CASES[case]())
    got = win.tap_wgrad(g, x, HALO)
    xw = win.windows(x, HALO).double()
    want = g.double().t() @ xw
    mag = g.double().abs().t() @ xw.abs()
    ratio = float(((got - want).abs() / mag).max())
    print(f"{case}: worst |err| / (|g|^T |x_win|) = {ratio:.2e} (bound {emul.BOUND:.2e})")
    assert torch.isfinite(got).all()
    assert ratio <= emul.BOUND


def test_windows_are_the_conv_weight_gradient():
    """the row shift is the layer's arithmetic: g^T x_win equals autograd's weight gradient of conv1d(k = 5, pad 2)"""
    gv, xv = rnd(S, HIN, COUT, seed=11).double(), rnd(S, HIN, CIN, seed=12).double()
    w = torch.zeros(COUT, CIN, 5, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv1d(xv.permute(0, 2, 1), w, None, padding=2).backward(gv.permute(0, 2, 1))
    want = w.grad.permute(0, 2, 1).reshape(COUT, 5 * CIN)
    got = halo(gv).t() @ win.windows(halo(xv), HALO)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_the_route_is_a_tunable_and_off_by_default():
    from flow2gan_amd import _opts, ops
    assert "fp16x3_tapw_min_rows" in _opts._ASKED
    assert "fp16x3_tapw_min_rows" in _opts.__doc__
    assert ops.FP16X3_TAPW_MIN_ROWS == ops.FP16X3_TAP_OFF
