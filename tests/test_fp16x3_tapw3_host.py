"""CPU: the arithmetic of the fp16x3 tap-walking weight gradient of a stride-3 layer (tests/fp16x3_colswin3_emul.py)
against float64 at the bound of tests/fp16x3_emul.py -- tap and stride only select rows of the halo map, so one
power-of-two scale per column of the whole map leaves the sum over rows exactly and the per-product bound 3 * 2^-22 of
|g| |x| is the column image's --, the windows against autograd's conv1d(k = 5, stride = 3, padding = 2) weight gradient
at all three residues of Hin modulo 3, and the route's tunable."""
import pytest
import torch

import fp16x3_colswin3_emul as win3
import fp16x3_emul as emul

S, HIN, HALO, CIN, COUT = 3, 37, 2, 32, 24
STEP, PAD = 3, 3 * HALO


def hout_of(hin):
    return (hin - 1) // STEP + 1


HOUT = hout_of(HIN)


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def spread(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.ldexp(torch.ones(*shape), torch.randint(-20, 1, shape, generator=g))


def halo(v):
    """(S, H, C) -> the flat halo layout (S * (H + 2 HALO), C) with zero halo rows"""
    out = torch.zeros(v.shape[0], v.shape[1] + 2 * HALO, v.shape[2], dtype=v.dtype)
    out[:, HALO:HALO + v.shape[1]] = v
    return out.reshape(-1, v.shape[2])


def geometry(hin):
    """nseq, hp_in, hp, pad of the layer's window operand"""
    return S, hin + 2 * HALO, hout_of(hin) + 2 * HALO, PAD


CASES = {
    "randn": lambda: (rnd(S, HOUT, COUT, seed=1), rnd(S, HIN, CIN, seed=2)),
    "elements_over_2^-20..1": lambda: (rnd(S, HOUT, COUT, seed=3) * spread(S, HOUT, COUT, seed=4),
                                       rnd(S, HIN, CIN, seed=5) * spread(S, HIN, CIN, seed=6)),
    "channels_over_decades": lambda: (rnd(S, HOUT, COUT, seed=7) * torch.logspace(-30, 30, COUT)[None, None, :],
                                      rnd(S, HIN, CIN, seed=8) * torch.logspace(-30, 30, CIN)[None, None, :]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_emulated_stride3_tap_weight_gradient_is_within_the_bound(case):
    g, x = (halo(v) for v in CASES[case]())
    got = win3.tap3_wgrad(g, x, *geometry(HIN))
    xw = win3.windows3(x, *geometry(HIN)).double()
    want = g.double().t() @ xw
    mag = g.double().abs().t() @ xw.abs()
    ratio = float(((got - want).abs() / mag).max())
    print(f"{case}: worst |err| / (|g|^T |x_win|) = {ratio:.2e} (bound {emul.BOUND:.2e})")
    assert torch.isfinite(got).all()
    assert ratio <= emul.BOUND


@pytest.mark.parametrize("hin", [36, 37, 38])
def test_windows_are_the_strided_conv_weight_gradient(hin):
    """row selection is the layer's arithmetic: g^T windows3(x) equals autograd's weight gradient of conv1d(k = 5,
    stride = 3, padding = 2), at every residue of Hin modulo 3"""
    gv, xv = rnd(S, hout_of(hin), COUT, seed=11).double(), rnd(S, hin, CIN, seed=12).double()
    w = torch.zeros(COUT, CIN, 5, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv1d(xv.permute(0, 2, 1), w, None, stride=STEP, padding=2)
    assert y.shape[2] == hout_of(hin)
    y.backward(gv.permute(0, 2, 1))
    want = w.grad.permute(0, 2, 1).reshape(COUT, 5 * CIN)
    got = halo(gv).t() @ win3.windows3(halo(xv), *geometry(hin))
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_the_route_is_a_tunable_and_off_by_default():
    from flow2gan_amd import _opts, ops
    assert "fp16x3_tapw3_min_rows" in _opts._ASKED
    assert "fp16x3_tapw3_min_rows" in _opts.__doc__
    assert ops.FP16X3_TAPW3_MIN_ROWS == ops.FP16X3_TAP_OFF
    assert ops.FP16X3_TAPW3_LAUNCHES >= 0
