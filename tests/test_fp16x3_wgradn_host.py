"""Host-side checks of the fp16x3 weight gradient over two plain fp32 matrices, both scaled inside the kernel
(csrc/gemm_f16wn.hip): the error bound of the arithmetic with one monotone running scale per operand and block over
the emulation (tests/fp16x3_runk_emul.py) on every case the GPU file launches, that bound against the GPU tolerance, the
walk of the running scales, the built library's answers for the descriptor (host code: nothing is launched), ops.gemm's
chooser and the Python-side tunable and counter.

The bound, per output:  3 * 2^-22 sum |a||b| + 2^-28 sum_T (brun_T sum_{r in T} |a| + arun_T sum_{r in T} |b|).
The GPU tolerance, per output:  TOL * sum |a||b| + 2^-28 (bmax sum_r |a| + amax sum_r |b|), TOL = 1.8e-6 and the
maxima over the whole operands: a running maximum never exceeds them and 3 * 2^-22 < TOL, so the tolerance holds the
bound whatever the grid -- which test_bound_is_inside_the_gpu_tolerance checks case by case."""
import ctypes as C
import os

import pytest
import torch

import fp16x3_route_cases as route_cases
import fp16x3_runk_emul as emul
from fp16x3_gpu import TOL              # (the GPU file's own)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = emul.gpu_cases()
IDS = [f"{p}-{'x'.join(map(str, s))}-k{k}" for p, s, k in CASES]


def gpu_tolerance(a, b):
    """the per-element tolerance of tests/test_hip_gemm_f16_wgradn.py (a store onto nothing: no |c0| term)"""
    aa, ba = a.double().abs(), b.double().abs()
    floor = emul.FLOOR * (ba.max() * aa.sum(0)[:, None] + aa.max() * ba.sum(0)[None, :])
    return TOL * (aa.t() @ ba) + floor


# ------------------------------------------------------------------ the arithmetic
@pytest.mark.parametrize("pattern,shape,split_k", CASES, ids=IDS)
def test_emulation_stays_inside_the_bound(pattern, shape, split_k):
    a, b = emul.inputs(pattern, *shape)
    got, want = emul.wgrad(a, b, split_k), emul.exact_wgrad(a, b)
    bnd, mag = emul.bound(a, b, split_k)
    err = (got - want).abs()
    assert torch.isfinite(got).all()
    assert bool((err <= bnd).all()), float((err / (bnd + 1e-300)).max())
    if pattern in ("zero_a", "zero_b"):
        assert not bool(got.any())


@pytest.mark.parametrize("pattern,shape,split_k", CASES, ids=IDS)
def test_bound_is_inside_the_gpu_tolerance(pattern, shape, split_k):
    """the inputs are fair: what the arithmetic is allowed, the GPU test allows"""
    a, b = emul.inputs(pattern, *shape)
    bnd, _ = emul.bound(a, b, split_k)
    assert bool((bnd <= gpu_tolerance(a, b)).all())


def test_emulation_agrees_with_float64_on_exact_inputs():
    """small integers split exactly under any power-of-two scale: tiles, chunks and slabs have no room to hide behind a
    tolerance"""
    for (R, M, N), split_k in [((1, 4, 32), 1), ((97, 260, 132), 1), ((777, 132, 160), 3)]:
        gen = torch.Generator().manual_seed(R)
        a = torch.randint(-8, 9, (R, M), generator=gen).float()
        b = torch.randint(-8, 9, (R, N), generator=gen).float()
        assert torch.equal(emul.wgrad(a, b, split_k), emul.exact_wgrad(a, b)), (R, M, N)


def test_k_chunks():
    """f2g_launch_h3w's rule: whole slabs per block, every row once; R = 777 in three: 288 / 288 / 201"""
    assert emul.kchunk_of(777, 3) == (288, 3) and emul.kchunk_of(777, 1) == (800, 1)
    assert emul.kchunk_of(64, 3) == (32, 2) and emul.kchunk_of(1, 4) == (32, 1)
    for R in range(1, 400):
        for split_k in (1, 2, 3, 5):
            kchunk, chunks = emul.kchunk_of(R, split_k)
            assert kchunk % emul.SLAB == 0 and (chunks - 1) * kchunk < R <= chunks * kchunk and chunks <= split_k


@pytest.mark.parametrize("pattern,shape,split_k", CASES, ids=IDS)
def test_scale_exponents_never_rise_within_a_block(pattern, shape, split_k):
    a, b = emul.inputs(pattern, *shape)
    w = emul.walk(a, b, split_k)
    per = w["kchunk"] // emul.SLAB
    for s in (w["sa"], w["sb"]):
        for z in range(0, s.shape[1], per):
            blk = s[:, z:z + per]
            # (scale 1 = exponent 0 at a block's leading zero slabs is "no scale yet": the first live slab sets it)
            live = w["arun" if s is w["sa"] else "brun"][:, z:z + per] > 0
            assert bool(((blk[:, 1:] <= blk[:, :-1]) | ~live[:, :-1]).all())


def test_a_zero_slab_and_a_non_finite_slab_leave_the_scale_alone():
    """R = 224: seven slabs, two chunks of four and three under split_k = 2.  Slab 0 zero: scale 1; slab 2 holds a NaN,
    slab 5 an inf (in column tile 1: tile 0 does not see it), slab 6 is zero: the scale in force; chunk 1 (slabs 4..6)
    starts over.  (The finite floats of a non-finite slab are split at the scale in force like the rest: here they are
    no larger than the running maximum, as the rule assumes -- a larger one may leave fp16's range.)"""
    R, M, N = 224, 132, 32
    a, b = torch.ones(R, M), torch.ones(R, N)
    a[:32] = 0.0
    a[32:96] = 2.0 ** -3
    a[70, 5] = float("nan")
    a[96:128] = 2.0 ** 4
    a[128:192] = 2.0 ** -6
    a[160:192, :128] = 2.0 ** -2
    a[170, 130] = float("inf")
    a[192:] = 0.0
    w = emul.walk(a, b, 2)
    assert emul.kchunk_of(R, 2) == (128, 2)
    assert not torch.isfinite(w["ma"][0, 2]) and not torch.isfinite(w["ma"][1, 5]) and torch.isfinite(w["ma"][0, 5])
    assert w["sa"][0].tolist() == [0, 17, 17, 10, 20, 16, 16]
    assert w["sa"][1].tolist() == [0, 17, 17, 10, 20, 20, 20]
    assert w["sb"][0].tolist() == [14] * 7
    # the columns beside the NaN's and the inf's stay finite and inside the bound
    keep = torch.ones(M, dtype=torch.bool)
    keep[5] = keep[130] = False
    got, want = emul.wgrad(a, b, 2)[keep], emul.exact_wgrad(a[:, keep], b)
    assert bool(((got - want).abs() <= emul.bound(torch.nan_to_num(a, nan=0.0, posinf=0.0), b, 2)[0][keep]).all())


# ------------------------------------------------------------------ the library's answers
def descriptor(ops, keep, R=160, M=132, N=160, ld_pad=4):
    """ops.wgrad's descriptor over two plain matrices with both operands marked, over host memory: the host checks
    never read through the pointers"""
    lda, ldb = M + ld_pad, N + ld_pad
    a, b, out = torch.zeros(R * lda), torch.zeros(R * ldb), torch.zeros(M * N)
    keep += [a, b, out]
    d = ops.GemmDesc()
    for S, t, cols, ld in ((d.A, a, M, lda), (d.B, b, N, ldb)):
        S.base, S.rows, S.cols, S.P1, S.P0, S.seglen, S.L1 = t.data_ptr(), R, cols, 1, 1, cols, 1
        S.unit, S.L0u, S.seq_stride, S.split = 1, cols, ld, 10
    d.E.C, d.E.ldc, d.E.atomic = out.data_ptr(), N, 1
    d.form, d.split_k, d.precision = 2, 1, 4
    return d


@pytest.fixture(scope="module")
def lib():
    from flow2gan_amd import _lib
    return _lib.lib


def test_the_library_answers_for_the_descriptor(lib):
    """f2g_gemm_f16_ok: 1 for the base descriptor -- never 2, there is nothing to make first -- and for what the kernel
    shares with gemm_h3w_kernel's epilogue; 0 for every refusal; f2g_gemm_colsum_part_rows: 0"""
    from flow2gan_amd import ops
    keep = []
    spare = torch.zeros(256)
    keep.append(spare)
    ok = lambda d: lib.f2g_gemm_f16_ok(C.byref(d))
    assert ok(descriptor(ops, keep)) == 1
    assert lib.f2g_gemm_colsum_part_rows(C.byref(descriptor(ops, keep))) == 0
    for R, M, N in emul.SHAPES + emul.MAGNITUDE_SHAPES:
        assert ok(descriptor(ops, keep, R, M, N)) == 1, (R, M, N)
    p = spare.data_ptr()
    accepted = {"store": [("E", "atomic", 0)], "accumulate": [("E", "atomic", 0), ("E", "accumulate", 1)],
                "split_k": [("d", "split_k", 3)], "bias": [("E", "bias", p)], "scale": [("E", "scale", 0.75)],
                "aux+alpha_n": [("E", "aux", p), ("E", "ldaux", 256), ("E", "alpha_n", p)]}
    for name, sets in accepted.items():
        assert ok(emul.apply(descriptor(ops, keep), sets)) == 1, name
    for name, sets in emul.refusals(p).items():
        d = emul.apply(descriptor(ops, keep), sets)
        assert ok(d) == 0, name
        assert lib.f2g_gemm_colsum_part_rows(C.byref(d)) == 0, name
    for prec in (0, 1, 2, 3):
        assert ok(emul.apply(descriptor(ops, keep), [("d", "precision", prec)])) == 0
    for form in (0, 1):
        assert ok(emul.apply(descriptor(ops, keep), [("d", "form", form)])) == 0
    # the mark of gemm_h3n_kernel's operand A (split = 9) means nothing at form 2, on one operand or on both, as before
    for marks in ((9, 9), (9, 10), (10, 9), (9, 0), (0, 9)):
        assert ok(emul.apply(descriptor(ops, keep), [("A", "split", marks[0]), ("B", "split", marks[1])])) == 0, marks
    # unmarked, the descriptor is the image route's as before: 2 = once both column images are made
    assert ok(emul.apply(descriptor(ops, keep), [("A", "split", 0), ("B", "split", 0)])) == 2


# ------------------------------------------------------------------ ops.gemm's chooser
def choose(ops, wgrad_rows, wgradn_rows, builder_args=None, sets=()):
    """(route or None, d, A, Bm, out) of ops._fp16x3_route for the plain weight-gradient case of tests/fp16x3_route_cases.py with the
    two thresholds as given; an image builder that runs raises"""
    def boom(operand):
        raise AssertionError("an image builder ran")
    ops._FP16X3_ROUTES = {key: tuple(r._replace(images=tuple(f and boom for f in r.images)) for r in rs)
                          for key, rs in ops._FP16X3_ROUTES.items()}
    ops.FP16X3_WGRAD_MIN_ROWS, ops.FP16X3_WGRADN_MIN_ROWS = wgrad_rows, wgradn_rows
    d, A, Bm, out = route_cases.build(ops, "WGRAD", builder_args or {}, list(sets), False)
    return ops._fp16x3_route(d, A, Bm, out, 2, bool(d.E.atomic), d.split_k, 0, False, None), d, A, Bm, out


def test_the_chooser_picks_the_route_behind_the_image_route():
    from flow2gan_amd import ops
    with route_cases.host_setup(ops):
        off = ops.FP16X3_TAP_OFF
        assert ops.FP16X3_WGRADN_MIN_ROWS == off and ops.FP16X3_WGRAD_MIN_ROWS == ops.FP16X3_WGRAD_OFF
        # the defaults: nothing
        r, d, A, Bm, out = choose(ops, ops.FP16X3_WGRAD_OFF, off)
        assert r is None and (d.A.split, d.B.split) == (0, 0)
        # its threshold at 1, the image route off: WGRADN, the marks left on the descriptor, the caller's operands
        # untouched, no builder run (_fp16x3_gemm: the counter moves, d.A / d.B stay the marked fp32 operands)
        r, d, A, Bm, out = choose(ops, ops.FP16X3_WGRAD_OFF, 1)
        assert r.counter == "FP16X3_WGRADN_LAUNCHES" and r.images == (None, None) and r.needs == 1
        assert (d.A.split, d.B.split, d.precision) == (10, 10, 4) and (A.split, Bm.split) == (0, 0)
        assert (d.A.base, d.B.base) == (A.base, Bm.base) and not d.A.rscale and not d.B.rscale
        n0 = ops.FP16X3_WGRADN_LAUNCHES
        d.A.split = d.B.split = 0
        d.precision = 3
        assert ops._fp16x3_gemm(d, A, Bm, out, 2, True, 1, 0, False, None)
        assert ops.FP16X3_WGRADN_LAUNCHES == n0 + 1 and (d.A.split, d.B.split) == (10, 10)
        assert (d.A.base, d.B.base) == (A.base, Bm.base)
        # a threshold above the rows: not yet
        assert choose(ops, ops.FP16X3_WGRAD_OFF, 513)[0] is None and choose(ops, ops.FP16X3_WGRAD_OFF, 512)[0] is not None
        # both at 1: the image route wins
        r, d, A, Bm, out = choose(ops, 1, 1)
        assert r.counter == "FP16X3_WGRAD_LAUNCHES" and (d.A.split, d.B.split) == (0, 0)
        # what the library declines is declined here, with the marks cleared: 130 columns, a non-atomic call
        r, d, A, Bm, out = choose(ops, ops.FP16X3_WGRAD_OFF, 1, dict(M=130))
        assert r is None and (d.A.split, d.B.split) == (0, 0)
        r, d, A, Bm, out = choose(ops, ops.FP16X3_WGRAD_OFF, 1, sets=[("E", "atomic", 0)])
        assert r is None and (d.A.split, d.B.split) == (0, 0)
        # the bf16x6 mode: no fp16x3 route at all
        ops.set_gemm_precision("bf16x6")
        assert choose(ops, 1, 1)[0] is None


def test_the_route_takes_nothing_the_recorded_table_gives_elsewhere():
    """the subset claim of ops._FP16X3_ROUTES' comment, against the recorded decisions: with the image route off and
    this one at 1, every WGRAD case of tests/golden/fp16x3_route_answers.json that the image route took goes to WGRADN
    or to nobody, and every case nobody took still goes to nobody"""
    import json
    from flow2gan_amd import _lib, ops
    with open(route_cases.GOLDEN) as f:
        golden = json.load(f)["answers"]
    taken = declined = 0
    with route_cases.host_setup(ops):
        for label, args, sets, x6p, x3_out in route_cases.changes("WGRAD"):
            old = _lib.set_option("x6p", x6p)
            for k in route_cases.thresholds(ops):
                setattr(ops, k, 1)
            ops.FP16X3_WGRAD_MIN_ROWS = ops.FP16X3_WGRAD_OFF
            got = route_cases.python_choice(ops, *route_cases.build(ops, "WGRAD", args, sets, False), x3_out)
            _lib.set_option("x6p", old)
            was = golden[f"WGRAD: {label}"][2]
            assert got in (("WGRADN", "") if was == "WGRAD" else (was,)), (label, was, got)
            taken += got == "WGRADN"
            declined += was == "WGRAD" and got == ""
    assert taken >= 20
    print(f"[h3wn] WGRAD cases of the recorded table: {taken} to WGRADN, {declined} the image route took and this declines")


def test_tunable_and_counter():
    from flow2gan_amd import _opts, ops
    assert "fp16x3_wgradn_min_rows" in _opts._ASKED and "fp16x3_wgradn_min_rows" in _opts.__doc__
    assert ops.FP16X3_WGRADN_MIN_ROWS == ops.FP16X3_TAP_OFF
    assert isinstance(ops.FP16X3_WGRADN_LAUNCHES, int)
    assert "`fp16x3_wgradn_min_rows`" in open(os.path.join(ROOT, "README.md")).read()
