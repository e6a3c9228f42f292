"""fp16x3 (F2G_GEMM=fp16x3), the parts that need no GPU: the error bound of the arithmetic on its emulation
(tests/fp16x3_emul.py), the mode switch of ops.set_gemm_precision, and the kernel's name staying outside the route
ledger of tests/test_hip_gemm_routes.py."""
import pytest
import torch

import fp16x3_emul as emul

M, N = 300, 160


def _inputs(family, K, seed):
    g = torch.Generator().manual_seed(seed)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    if family == "exponents":       # every element times 2^randint(-20, 0)
        A = A * torch.ldexp(torch.ones(M, K), torch.randint(-20, 1, (M, K), generator=g))
        B = B * torch.ldexp(torch.ones(N, K), torch.randint(-20, 1, (N, K), generator=g))
    if family == "rows":            # rows of A over 60 decades
        A = A * torch.logspace(-30, 30, M)[:, None]
    return A, B


@pytest.mark.parametrize("K", [32, 768, 2304])
@pytest.mark.parametrize("family", ["randn", "exponents", "rows"])
def test_emulated_arithmetic_keeps_the_per_product_bound(family, K):
    """worst |C - C64| / (|A| |B|^T) <= 3 * 2^-22: 2^-22 from each operand's residual, 2^-22 for the dropped term"""
    A, B = _inputs(family, K, 1000 + K)
    got = emul.gemm(A, B)
    want = A.double() @ B.double().t()
    mag = A.double().abs() @ B.double().abs().t()
    worst = float(((got - want).abs() / mag).max())
    print(f"{family} K={K}: worst {worst:.3e} (bound {emul.BOUND:.3e})")
    assert torch.isfinite(got).all()
    assert worst <= emul.BOUND, (family, K, worst)


def test_emulated_split_special_rows():
    """zero row, non-finite row (scale 1, values stay non-finite), power-of-two amax at the top of the range"""
    x = torch.zeros(4, 32)
    x[1, 3] = float("inf")
    x[1, 4] = 2.0
    x[2] = torch.linspace(-1, 1, 32)
    x[2, 0] = 4.0
    x[3, 5] = 1e-45                 # (a subnormal amax: the clamped scale)
    hi, lo, rs = emul.split(x)
    assert rs[0] == 1 and rs[1] == 1 and bool((hi[0] == 0).all()) and bool(torch.isinf(hi[1, 3]))
    assert float(hi[2, 0]) == 2.0 ** 14 and float(rs[2]) == 2.0 ** -12
    assert float(rs[3]) == 2.0 ** -126 and bool(torch.isfinite(rs).all()) and bool((rs > 0).all())
    back = (hi.double() + lo.double() * 2.0 ** -11) * rs.double()[:, None]
    assert torch.equal(back[2], x[2].double()) or float((back[2] - x[2].double()).abs().max()) <= 4.0 * 2.0 ** -22


def test_set_gemm_precision_knows_fp16x3():
    from flow2gan_amd import ops
    was = "fp16x3" if getattr(ops, "FP16X3", False) else {0: "fp32", 1: "bf16x3", 2: "bf16", 3: "bf16x6"}[ops.GEMM_PRECISION]
    try:
        ops.set_gemm_precision("fp16x3")
        assert ops.FP16X3 is True and ops.GEMM_PRECISION == 3
        ops.set_gemm_precision("bf16x6")
        assert ops.FP16X3 is False and ops.GEMM_PRECISION == 3
        for name, p in (("fp32", 0), ("bf16x3", 1), ("bf16", 2)):
            ops.set_gemm_precision("fp16x3")
            ops.set_gemm_precision(name)
            assert ops.FP16X3 is False and ops.GEMM_PRECISION == p
        with pytest.raises(ValueError):
            ops.set_gemm_precision("fp16x4")
        assert ops.FP16X3_LAUNCHES >= 0 and ops.FP16X3_MIN_K >= 32 and ops.FP16X3_MIN_N >= 1
    finally:
        ops.set_gemm_precision(was)


def test_environment_switch_selects_the_mode_at_import():
    """F2G_GEMM=fp16x3 in the environment: the flag is set and the mode is bf16x6's (a fresh interpreter, since the
    variable is read when flow2gan_amd.ops is imported); F2G_GEMM=bf16x6 leaves the flag clear"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in (("fp16x3", "True 3"), ("bf16x6", "False 3"), ("FP16X3", "True 3")):
        env = dict(os.environ, F2G_GEMM=value, PYTHONPATH=root)
        out = subprocess.run([sys.executable, "-c", "from flow2gan_amd import ops; print(ops.FP16X3, ops.GEMM_PRECISION)"],
                             env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.split("\n")[-2].strip() == want, (value, out.stdout)


def test_new_kernel_name_stays_outside_the_route_ledger():
    """the ledger of test_hip_gemm_routes.py collects the literals of the lean / x6 / narrow / generic families from
    csrc/: the fp16x3 kernel's own translation unit adds none (61 = the set before gemm_f16.hip existed)"""
    from test_hip_gemm_routes import ROUTES, kernel_literals
    lits = kernel_literals()
    assert len(lits) == 61, sorted(lits)
    assert lits == ROUTES
    assert not any(n.startswith("h3") for n in lits)
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flow2gan_amd", "csrc",
                            "gemm_f16.hip")).read()
    assert '"h3<ep=all>"' in src
