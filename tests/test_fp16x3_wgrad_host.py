"""CPU: the arithmetic of the fp16x3 weight gradient (tests/fp16x3_cols_emul.py) against float64 at the bound of
tests/fp16x3_emul.py -- a power-of-two scale per column of both K-major operands leaves the sum over rows exactly,
so the per-product bound 3 * 2^-22 of |a| |b| is the forward kernel's -- and the layout of the column image."""
import pytest
import torch

import fp16x3_cols_emul as cols
import fp16x3_emul as emul


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def spread(R, M, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.ldexp(torch.ones(R, M), torch.randint(-20, 1, (R, M), generator=g))


CASES = {
    "one_row": lambda: (rnd(1, 32, seed=1), rnd(1, 32, seed=2)),
    "elements_over_2^-20..1": lambda: (rnd(777, 384, seed=3) * spread(777, 384, 4),
                                       rnd(777, 128, seed=5) * spread(777, 128, 6)),
    "columns_over_decades": lambda: (rnd(777, 384, seed=7) * torch.logspace(-30, 30, 384)[None, :],
                                     rnd(777, 128, seed=8) * torch.logspace(-15, 15, 128)[None, :]),
    "long_reduction": lambda: (rnd(4100, 128, seed=9), rnd(4100, 160, seed=10)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_emulated_weight_gradient_is_within_the_bound(case):
    A, B = CASES[case]()
    got = cols.wgrad(A, B)
    want = A.double().t() @ B.double()
    mag = A.double().abs().t() @ B.double().abs()
    ratio = float(((got - want).abs() / mag).max())
    print(f"{case}: worst |err| / (|A|^T |B|) = {ratio:.2e} (bound {emul.BOUND:.2e})")
    assert torch.isfinite(got).all()
    assert ratio <= emul.BOUND


def test_column_image_layout_and_scales():
    """a chunk = four consecutive columns of a row: four hi halves, then four lo halves; the pieces and scales are
    those of the row split of the transpose, and undoing the scale gives the values back to 2^-22"""
    x = rnd(9, 12, seed=11) * torch.logspace(-8, 8, 12)[None, :]
    x[:, 3] = 0.0                                   # an all-zero column: scale 1
    x[4, 5] = float("inf")                          # a non-finite column: scale 1, values stay non-finite
    img, rs = cols.image(x)
    hi, lo, rs_t = emul.split(x.t())
    assert torch.equal(rs, rs_t) and float(rs[3]) == 1.0 and float(rs[5]) == 1.0
    halves = img.view(torch.int16).view(9, 3, 8)
    assert torch.equal(halves[:, :, :4].reshape(9, 12), hi.t().contiguous().view(torch.int16))
    assert torch.equal(halves[:, :, 4:].reshape(9, 12), lo.t().contiguous().view(torch.int16))
    amax = x.abs().amax(0)
    ok = torch.isfinite(amax) & (amax > 0)
    scaled = (amax / rs)[ok]
    assert bool((scaled >= 2.0 ** 14).all()) and bool((scaled < 2.0 ** 15).all())
    back = (hi.double() + lo.double() * 2.0 ** -11).t() * rs.double()[None, :]
    assert bool(((back - x.double()).abs()[:, ok] <= 2.0 ** -22 * x.double().abs()[:, ok]).all())
    assert not bool(torch.isfinite(back[4, 5]))      # (hi = inf, lo = fp16(inf - inf) = NaN)
