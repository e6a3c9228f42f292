"""fp16x3 over stride-1 windows of a halo map, the part that needs no GPU: the error bound of the per-sequence scale
on its emulation (tests/fp16x3_seq_emul.py) -- 3 * 2^-22 (|A| |B|^T) + 2^-28 amax_seq sum|w| per output -- and the
tunable of the route."""
import pytest
import torch

import fp16x3_seq_emul as emul

S, P0, C, N = 5, 64, 64, 128


def _inputs(family, taps, seed):
    g = torch.Generator().manual_seed(seed)
    Hp = P0 + taps - 1
    x, w = torch.randn(S, Hp, C, generator=g), torch.randn(N, taps * C, generator=g)
    if family == "exponents":       # every element times 2^randint(-40, 0)
        x = x * torch.ldexp(torch.ones(S, Hp, C), torch.randint(-40, 1, (S, Hp, C), generator=g))
        w = w * torch.ldexp(torch.ones(N, taps * C), torch.randint(-40, 1, (N, taps * C), generator=g))
    if family == "sequences":       # sequences over 60 decades
        x = x * torch.logspace(-30, 30, S)[:, None, None]
    if family.startswith("quiet"):  # a window that is quiet against its own sequence: positions 0..39 x 2^-32
        x[:, :40] *= 2.0 ** -32
    return x, w


@pytest.mark.parametrize("taps", [5, 2])
@pytest.mark.parametrize("family", ["randn", "exponents", "sequences", "quiet", "quiet_flushed"])
def test_emulated_arithmetic_keeps_the_bound_with_the_floor_term(family, taps):
    x, w = _inputs(family, taps, 2000 + taps)
    got = emul.gemm(x, w, P0, taps, flush=family == "quiet_flushed")
    want = emul.windows(x.double(), P0, taps) @ w.double().t()
    tol, mag = emul.bound(x, w, P0, taps)
    err = (got - want).abs()
    worst_rel = float((err / mag).max())
    worst = float((err / tol).max())
    print(f"{family} taps={taps}: worst error / (|A||B|^T) {worst_rel:.3e} (3 * 2^-22 = {emul.BOUND:.3e}), "
          f"worst error / full bound {worst:.3f}")
    assert torch.isfinite(got).all()
    assert worst <= 1.0, (family, taps, worst)
    if not family.startswith("quiet"):      # these stay under the relative bound alone
        assert worst_rel <= emul.BOUND, (family, taps, worst_rel)


def test_quiet_windows_need_the_floor_term():
    """the quiet rows of the quiet-window case miss the relative bound: the floor term is what the coarser scale
    costs, not slack"""
    x, w = _inputs("quiet", 5, 2005)
    got = emul.gemm(x, w, P0, 5)
    want = emul.windows(x.double(), P0, 5) @ w.double().t()
    _, mag = emul.bound(x, w, P0, 5)
    rel = ((got - want).abs() / mag).view(S, P0, N)
    assert float(rel[:, :36].max()) > emul.BOUND        # windows of positions 0..39 only
    assert float(rel[:, 40:].max()) <= emul.BOUND       # windows of loud positions only


def test_image_layout_is_hi_slab_then_lo_slab():
    x = torch.randn(3, 96, generator=torch.Generator().manual_seed(1))
    img, rs = emul.image(x)
    hi, lo, rs2 = emul.split(x)
    halves = img.view(torch.int16).view(3, 3, 2, 32)
    assert torch.equal(halves[:, :, 0].reshape(3, 96), hi.view(torch.int16))
    assert torch.equal(halves[:, :, 1].reshape(3, 96), lo.view(torch.int16))
    assert torch.equal(rs, rs2)


def test_route_tunable_is_declared_with_its_off_sentinel():
    from flow2gan_amd import _opts, ops
    assert "fp16x3_tap_min_rows" in _opts._ASKED and "fp16x3_tap_min_rows" in _opts.__doc__
    assert ops.FP16X3_TAP_OFF == ops.FP16X3_WGRAD_OFF and ops.FP16X3_TAP_MIN_ROWS >= 1
    assert ops.FP16X3_TAP_LAUNCHES >= 0
