"""fp16x3 over stride-3 windows of five positions of a halo map, the part that needs no GPU: the error bound of the
per-sequence scale on its emulation (tests/fp16x3_seq3_emul.py) at the production period-11 geometry (P0 = 27 windows
three positions apart, Hp = 85) -- 3 * 2^-22 (|A| |B|^T) + 2^-28 amax_seq sum|w| per output, for the input families of
tests/test_fp16x3_seq_host.py -- and the tunable of the route."""
import pytest
import torch

import fp16x3_seq3_emul as emul
import fp16x3_seq_emul as seq

S, P0, C, N, STEP, TAPS = 5, 27, 64, 128, 3, 5
HP = STEP * (P0 - 1) + TAPS + 2


def _inputs(family, seed):
    g = torch.Generator().manual_seed(seed)
    x, w = torch.randn(S, HP, C, generator=g), torch.randn(N, TAPS * C, generator=g)
    if family == "exponents":       # every element times 2^randint(-40, 0)
        x = x * torch.ldexp(torch.ones(S, HP, C), torch.randint(-40, 1, (S, HP, C), generator=g))
        w = w * torch.ldexp(torch.ones(N, TAPS * C), torch.randint(-40, 1, (N, TAPS * C), generator=g))
    if family == "sequences":       # sequences over 60 decades
        x = x * torch.logspace(-30, 30, S)[:, None, None]
    if family.startswith("quiet"):  # windows that are quiet against their own sequence: positions 0..39 x 2^-32
        x[:, :40] *= 2.0 ** -32
    return x, w


@pytest.mark.parametrize("family", ["randn", "exponents", "sequences", "quiet", "quiet_flushed"])
def test_emulated_arithmetic_keeps_the_bound_with_the_floor_term(family):
    x, w = _inputs(family, 3000)
    got = emul.gemm(x, w, P0, TAPS, STEP, flush=family == "quiet_flushed")
    want = emul.windows(x.double(), P0, TAPS, STEP) @ w.double().t()
    tol, mag = emul.bound(x, w, P0, TAPS, STEP)
    err = (got - want).abs()
    worst_rel = float((err / mag).max())
    worst = float((err / tol).max())
    print(f"{family}: worst error / (|A||B|^T) {worst_rel:.3e} (3 * 2^-22 = {emul.BOUND:.3e}), "
          f"worst error / full bound {worst:.3f}")
    assert torch.isfinite(got).all()
    assert worst <= 1.0, (family, worst)
    if not family.startswith("quiet"):      # these stay under the relative bound alone
        assert worst_rel <= emul.BOUND, (family, worst_rel)


def test_strided_windows_are_the_conv():
    """the stride is the layer's arithmetic: windows(x) w^T equals conv1d(k = 5, stride 3) of the map"""
    g = torch.Generator().manual_seed(5)
    x, w = torch.randn(S, HP, 8, generator=g).double(), torch.randn(6, 8, TAPS, generator=g).double()
    want = torch.nn.functional.conv1d(x.permute(0, 2, 1), w, None, stride=STEP)[:, :, :P0].permute(0, 2, 1)
    got = emul.windows(x, P0, TAPS, STEP) @ w.permute(0, 2, 1).reshape(6, TAPS * 8).t()
    assert float((got - want.reshape(S * P0, 6)).abs().max()) <= 1e-12 * float(want.abs().max())


def test_stride_one_is_the_stride_one_emulation():
    x, w = _inputs("sequences", 3001)
    assert torch.equal(emul.windows(x, P0, TAPS, 1), seq.windows(x, P0, TAPS))
    assert torch.equal(emul.gemm(x, w, P0, TAPS, 1), seq.gemm(x, w, P0, TAPS))
    assert emul.BOUND == seq.BOUND and emul.FLOOR == seq.FLOOR == 2.0 ** -28


def test_the_route_is_a_tunable_and_off_by_default():
    from flow2gan_amd import _opts, ops
    assert "fp16x3_tap3_min_rows" in _opts._ASKED
    assert "fp16x3_tap3_min_rows" in _opts.__doc__
    assert ops.FP16X3_TAP3_MIN_ROWS == ops.FP16X3_TAP_OFF
    assert ops.FP16X3_TAP3_LAUNCHES >= 0
