"""conv33h3w.hip on the GPU: the fp16x3 weight gradient of the (3, 3) MRD band layer (f2g_conv33_wgrad_h3) with one
monotone running scale per operand and block, against float64 autograd of F.conv2d.

What the structure can get wrong, at the smallest shapes that show it: a wrong two-piece fragment, tap offset, piece
order, accumulator tile or flush address (one image row and one channel half at a time; one pixel pair per tap, which
covers the tap the two wave groups share), a scale that does not follow the block's walk b, b + grid, ... or
accumulators that do not follow the scale (sequences many binades apart, blocks of two and three tiles), the
accumulation into a prefilled matrix with few tiles and degenerate widths, where the maximum is looked for (zeros, a
halo row, floats beside and below the map, a NaN), the strided gradient input, the descriptors the entry point must
refuse, the Python routing with its tunable and counter, and one MRD resolution end to end against the CPU oracle.

Tolerance, per element: 1.8e-6 * sum |g||x| (the TOL of the fp16x3 GPU tests) + 2^-28 sum_T (xrun_T sum_{px in T} |g|
+ grun_T sum_{px in T} |x|), the floor term of the running scales (tests/fp16x3_conv33w_emul.py: bound_wgrad).
Shapes are (S, H, W); gw is (32, 9 * 32) [co][tap][ci].
"""
import ctypes as C
import functools

import pytest
import torch

import fp16x3_conv33w_emul as emul
from fp16x3_gpu import EINVAL, TOL, fp16x3_mode, library, subdisc_against_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
TUNABLES = ("FP16X3_CONV32_FWD", "FP16X3_CONV32_DGRAD", "FP16X3_CONV32_WGRAD", "FP16X3_CONV33_FWD",
            "FP16X3_CONV33_DGRAD", "FP16X3_CONV33_WGRAD")


@pytest.fixture
def ops():
    """the fp16x3 mode with the (3, 3) weight-gradient tunable on; mode and band-conv tunables restored afterwards"""
    with fp16x3_mode(library(), *TUNABLES) as o:
        o.FP16X3_CONV33_WGRAD = True
        yield o


def g(t):
    return t.to(DEV).contiguous()


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def pow2(e):
    return torch.ldexp(torch.ones(e.shape), e)


def reference(x, gy):
    """(float64 gradient, per-element tolerance)"""
    return emul.exact_wgrad(x, gy), emul.bound_wgrad(x, gy, rel=TOL)[0]


@functools.lru_cache(maxsize=None)
def case(S, H, W, spread=0):
    """Inputs, float64 reference and per-element tolerance of one shape: computed once, shared, not modified.
    spread 1: sequence s of x times 2^((7 s mod 41) - 20), the flipped sequence for the gradient; 2: the other way
    round."""
    x, gy = rnd(S, H, W, 32, seed=11), rnd(S, H, W, 32, seed=14)
    if spread:
        seq = pow2((7 * torch.arange(S)) % 41 - 20)[:, None, None, None]
        x, gy = (x * seq, gy * seq.flip(0)) if spread == 1 else (x * seq.flip(0), gy * seq)
    want, tol = reference(x, gy)
    return dict(x=x, gy=gy, want=want, tol=tol)


def close(got, want, tol, name):
    got = got.detach().cpu().double().reshape(want.shape)
    err = (got - want).abs()
    bad = ~(err <= tol)                                     # (a NaN fails)
    worst = float((err / tol)[tol > 0].max()) if bool((tol > 0).any()) else 0.0
    print(f"[conv33 fp16x3 wgrad] {name}: worst error {worst:.3f} of the tolerance")
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements beyond the tolerance, worst {worst:.3f} of it"


def run(ops, x, gy, prefill=None):
    """one launch through ops: gw (32, 288) = prefill (zeros) + the gradient"""
    S, H, W = x.shape[:3]
    gw = torch.zeros(32, 9 * 32, device=DEV) if prefill is None else g(prefill.clone())
    n0 = ops.FP16X3_CONV33_WGRAD_LAUNCHES
    ops.conv33_wgrad(g(x).view(-1, 32), g(gy).view(-1, 32), S, H, W, gw)
    assert ops.FP16X3_CONV33_WGRAD_LAUNCHES == n0 + 1
    return gw


def desc_of(ops, x, gy, S, H, W, precision=4):
    d = ops.L.Conv32Desc()
    d.S, d.H, d.Win, d.Wout, d.precision = S, H, W, W, precision
    d.x, d.x_seq, d.x_line = x.data_ptr(), H * W * 32, W * 32
    d.y, d.y_seq, d.y_line = gy.data_ptr(), H * W * 32, W * 32
    return d


# ------------------------------------------------------------------ 1. one piece at a time
@pytest.mark.parametrize("S,H,W", [(2, 9, 13), (1, 7, 33)])
def test_one_piece_at_a_time(ops, S, H, W):
    """One tile per sequence.  The gradient zero except for ONE image row, for every row of the tile; then the input
    zero except for one 16-channel half, then the same for the gradient's channels: the WHOLE gw is compared each time,
    so a wrong hi / lo fragment, tap offset, piece order, accumulator tile or flush address all fail, and so does a
    contribution from a k step that should be silent."""
    assert emul.pick_rows(H, W) == H
    c = case(S, H, W)
    for row in range(H):
        gy = torch.zeros_like(c["gy"])
        gy[S - 1, row] = c["gy"][S - 1, row]
        close(run(ops, c["x"], gy), *reference(c["x"], gy), f"{(S, H, W)}, image row {row}")
    for half in range(2):
        sl = slice(16 * half, 16 * half + 16)
        x = torch.zeros_like(c["x"])
        x[..., sl] = c["x"][..., sl]
        close(run(ops, x, c["gy"]), *reference(x, c["gy"]), f"{(S, H, W)}, input channel half {half}")
        gy = torch.zeros_like(c["gy"])
        gy[..., sl] = c["gy"][..., sl]
        close(run(ops, c["x"], gy), *reference(c["x"], gy), f"{(S, H, W)}, output channel half {half}")


# ------------------------------------------------------------------ 2. tap identity
def test_tap_identity(ops):
    """(1, 5, 6): one nonzero gradient pixel and one nonzero input pixel at the offset of tap t, both powers of two:
    gw is nonzero in tap t's 32 x 32 block only, and exact there -- for each of the nine taps, the centre tap that the
    two wave groups share included."""
    S, H, W = 1, 5, 6
    for t in range(9):
        dh, dw = t // 3, t % 3
        x, gy = torch.zeros(S, H, W, 32), torch.zeros(S, H, W, 32)
        gy[0, 2, 3, 3 + t] = 8.0
        x[0, 2 + dh - 1, 3 + dw - 1, 20 - t] = 2.0 ** -5
        got = run(ops, x, gy).cpu().double().view(32, 9, 32)
        want = emul.exact_wgrad(x, gy).view(32, 9, 32)
        assert float(want[3 + t, t, 20 - t]) == 0.25 and int((want != 0).sum()) == 1
        others = [u for u in range(9) if u != t]
        assert not bool(got[:, others].any()), f"tap {t} reached another tap's block"
        assert torch.equal(got, want), f"tap {t}"


# ------------------------------------------------------------------ 3. the scales move with the walk
@pytest.mark.parametrize("S,H,W,steps", [(150, 4, 86, 2), (260, 4, 86, 3)])
def test_scales_move_with_the_walk(ops, S, H, W, steps):
    """Tiles of two rows, 300 tiles (blocks 0-43 walk two) and 520 tiles (blocks 0-7 walk three) on 256 blocks.  The
    sequences lie up to 40 binades apart, in opposite directions for the two operands, then the other way round: a later
    louder tile (the rescale is taken) and a later quieter one (the scale stands) occur in the same launch.  A scale
    taken from the wrong tile, accumulators that are not rescaled when a scale drops, or only one of the two sets
    rescaled, all leave the tolerance."""
    for spread in (1, 2):
        c = case(S, H, W, spread)
        w = emul.walk(c["x"], c["gy"])
        assert (w["R"], w["grid"], w["steps"]) == (2, 256, steps)
        later = w["sx"][256:512]                            # the blocks' second tiles against their first
        first = w["sx"][:later.numel()]
        assert bool((later < first).any()) and bool((later == first).any())
        close(run(ops, c["x"], c["gy"]), c["want"], c["tol"], f"{(S, H, W)}, spread {spread}")


# ------------------------------------------------------------------ 4. accumulate; few tiles, degenerate widths
@pytest.mark.parametrize("S,H,W", [(1, 3, 7), (1, 1, 1), (1, 300, 1), (2, 40, 2), (2, 5, 112), (3, 40, 33)])
def test_accumulates_into_a_prefilled_matrix(ops, S, H, W):
    """gw comes back as prefill + gradient (the fp32 additions: TOL of the prefill on top).  H < R; one k step; W = 1
    (R = 115: three tiles, the last partial), W = 2, W = 112 (R = 1); a partial last tile (40 = 5 * 7 + 5)."""
    c = case(S, H, W)
    prefill = rnd(32, 9 * 32, seed=31, scale=3.0)
    close(run(ops, c["x"], c["gy"], prefill), c["want"] + prefill.double(), c["tol"] + TOL * prefill.double().abs(),
          f"{(S, H, W)}, prefilled")


# ------------------------------------------------------------------ 5. where the maximum is looked for
def test_zero_inputs_leave_the_prefill(ops):
    S, H, W = 2, 9, 13
    prefill = rnd(32, 9 * 32, seed=32)
    c = case(S, H, W)
    for x, gy in ((torch.zeros_like(c["x"]), c["gy"]), (c["x"], torch.zeros_like(c["gy"])),
                  (torch.zeros_like(c["x"]), torch.zeros_like(c["gy"]))):
        assert torch.equal(run(ops, x, gy, prefill).cpu(), prefill)


def test_maximum_in_a_halo_row(ops):
    """(2, 14, 33): R = 7, two tiles per sequence.  Sequence 0 is zero except for ONE input float of 2^20 in row 7, the
    halo row below the first tile: a maximum taken over a tile's own rows alone would leave that tile at scale 1 and
    2^20 outside fp16."""
    S, H, W = 2, 14, 33
    assert emul.pick_rows(H, W) == 7
    x, gy = rnd(S, H, W, 32, seed=5), rnd(S, H, W, 32, seed=6)
    x[0] = 0.0
    x[0, 7, 5, 7] = 2.0 ** 20
    gw = run(ops, x, gy)
    assert bool(torch.isfinite(gw).all())
    close(gw, *reference(x, gy), "maximum in a halo row")


def test_floats_beside_and_below_the_map_do_not_exist(ops):
    """(3, 40, 33), the gradient a slice of a wider and taller map whose other floats are 1e30: the zero border columns
    of the staged rows and the rows below the map in the partial last tile (40 = 5 * 7 + 5) hold nothing -- neither for
    the running maximum nor for the sums."""
    S, H, W = 3, 40, 33
    c = case(S, H, W)
    lo, Wtot, Htot = 3, W + 7, H + 3
    wide = torch.full((S, Htot, Wtot, 32), 1e30)
    wide[:, :H, lo:lo + W] = c["gy"]
    wide, x = g(wide), g(c["x"])
    gw = torch.zeros(32, 9 * 32, device=DEV)
    ops.conv33_wgrad(x.view(-1, 32), wide.view(-1, 32), S, H, W, gw, g_off=lo * 32, g_line=Wtot * 32,
                     g_seq=Htot * Wtot * 32)
    close(gw, c["want"], c["tol"], f"{(S, H, W)}, 1e30 around the gradient")


def test_a_nan_float_stays_in_its_sums(ops):
    """One NaN in x[1, 4, 6, 5]: the (tap, ci = 5) sums that reach it are NaN, for every co; every other output stays
    within the tolerance computed with that float zeroed, and the next launch knows nothing of it."""
    S, H, W = 2, 9, 13
    c = case(S, H, W)
    x = c["x"].clone()
    x[1, 4, 6, 5] = float("nan")
    holds = emul.exact_wgrad(torch.isnan(x).float(), torch.ones_like(c["gy"])) > 0
    assert int(holds.sum()) == 32 * 9                       # all nine taps, ci = 5
    got = run(ops, x, c["gy"]).cpu().double()
    assert bool(torch.isnan(got[holds]).all()), "a sum that holds the NaN is not NaN"
    want, tol = reference(x.nan_to_num(0.0), c["gy"])
    err = (got - want).abs()
    assert bool((err[~holds] <= tol[~holds]).all()), "the NaN reached another sum"
    close(run(ops, c["x"], c["gy"]), c["want"], c["tol"], "the launch after the NaN")


# ------------------------------------------------------------------ 6. the gradient as a band's slice
@pytest.mark.parametrize("S,H,W", [(3, 11, 13), (5, 40, 33)])
def test_gradient_slice_of_a_wider_map(ops, S, H, W):
    """The gradient is a band's slice of the concatenated map (g_off, g_line, g_seq, as fused_disc passes them); the
    neighbouring bands' columns are 2^10 louder.  Against the reference, and bit for bit against the contiguous case
    where one tile per block fixes the order of the sums (small-integer inputs make the sums exact)."""
    c = case(S, H, W)
    lo, Wtot = 5, W + 9
    wide = rnd(S, H, Wtot, 32, seed=21) * 1024.0
    wide[:, :, lo:lo + W] = c["gy"]
    gw = torch.zeros(32, 9 * 32, device=DEV)
    ops.conv33_wgrad(g(c["x"]).view(-1, 32), g(wide).view(-1, 32), S, H, W, gw, g_off=lo * 32, g_line=Wtot * 32,
                     g_seq=H * Wtot * 32)
    close(gw, c["want"], c["tol"], f"{(S, H, W)}, strided gradient")
    gen = torch.Generator().manual_seed(9)
    xi = torch.randint(-8, 9, (S, H, W, 32), generator=gen).float()
    gi = torch.randint(-8, 9, (S, H, W, 32), generator=gen).float()
    wide[:, :, lo:lo + W] = gi
    gws = torch.zeros(32, 9 * 32, device=DEV)
    ops.conv33_wgrad(g(xi).view(-1, 32), g(wide).view(-1, 32), S, H, W, gws, g_off=lo * 32, g_line=Wtot * 32,
                     g_seq=H * Wtot * 32)
    assert torch.equal(gws, run(ops, xi, gi)) and torch.equal(gws.cpu().double(), emul.exact_wgrad(xi, gi))


# ------------------------------------------------------------------ 7. refusals
def test_refusals(ops):
    S, H, W = 2, 9, 13
    c = case(S, H, W)
    lib, st = ops.L.lib, ops.L.stream_ptr()
    x, gy = g(c["x"]), g(c["gy"])
    gw = torch.full((32, 9 * 32), 7.0, device=DEV)
    bad = [("precision", p) for p in (0, 1, 2, 3, 5)]
    bad += [("x", None), ("y", None), ("x", x.data_ptr() + 4), ("y", gy.data_ptr() + 8)]
    bad += [("x_line", W * 32 + 2), ("x_seq", H * W * 32 + 1), ("y_line", W * 32 + 2), ("y_seq", H * W * 32 + 3)]
    bad += [("Wout", W + 1), ("Win", W - 1), ("y_line", W * 32 - 4), ("x_line", W * 32 - 4)]
    for field, value in bad:
        d = desc_of(ops, x, gy, S, H, W)
        setattr(d, field, value)
        assert lib.f2g_conv33_wgrad_h3(C.byref(d), gw.data_ptr(), st) == EINVAL, (field, value)
    assert lib.f2g_conv33_wgrad_h3(C.byref(desc_of(ops, x, gy, S, H, W)), None, st) == EINVAL
    wide_x, wide_g = torch.zeros(1, 2, 113, 32, device=DEV), torch.zeros(1, 2, 113, 32, device=DEV)
    assert lib.f2g_conv33_wgrad_h3(C.byref(desc_of(ops, wide_x, wide_g, 1, 2, 113)), gw.data_ptr(), st) == EINVAL
    d = desc_of(ops, x, gy, S, H, W)
    d.S = 0
    assert lib.f2g_conv33_wgrad_h3(C.byref(d), gw.data_ptr(), st) == 0               # nothing to do: F2G_OK
    torch.cuda.synchronize()
    assert bool((gw == 7.0).all()), "a refused or empty launch wrote gw"
    assert lib.f2g_conv33_wgrad_h3(C.byref(desc_of(ops, x, gy, S, H, W)), gw.data_ptr(), st) == 0
    torch.cuda.synchronize()
    close(gw, c["want"] + 7.0, c["tol"] + TOL * 7.0, "the intact descriptor")


# ------------------------------------------------------------------ 8. routing
def test_ops_route(ops, monkeypatch):
    """The tunable on: the new entry point, the counter moves by one per call.  Off: the counter stands still and the
    result is bit for bit the precision-3 launch spelled out through ctypes ((3, 11, 13): one tile per block; small-
    integer inputs, whose sums are exact in any order of the three blocks' atomics).  In bf16x6 the tunable means
    nothing."""
    S, H, W = 3, 11, 13
    c = case(S, H, W)
    names, real_call = [], ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])

    def once(x, gy):
        gw = torch.zeros(32, 9 * 32, device=DEV)
        del names[:]
        n0 = ops.FP16X3_CONV33_WGRAD_LAUNCHES
        ops.conv33_wgrad(g(x).view(-1, 32), g(gy).view(-1, 32), S, H, W, gw)
        torch.cuda.synchronize()
        return gw, ops.FP16X3_CONV33_WGRAD_LAUNCHES - n0, [n for n in names if "wgrad" in n]

    for _ in range(2):
        gw, n, took = once(c["x"], c["gy"])
        assert (n, took) == (1, ["f2g_conv33_wgrad_h3"])
        close(gw, c["want"], c["tol"], "ops weight gradient")
    gen = torch.Generator().manual_seed(4)
    xi = torch.randint(-8, 9, (S, H, W, 32), generator=gen).float()
    gi = torch.randint(-8, 9, (S, H, W, 32), generator=gen).float()
    xg, gg = g(xi), g(gi)
    p3 = torch.zeros(32, 9 * 32, device=DEV)
    assert ops.L.lib.f2g_conv33_wgrad(C.byref(desc_of(ops, xg, gg, S, H, W, 3)), p3.data_ptr(), ops.L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(p3.cpu().double(), emul.exact_wgrad(xi, gi))
    ops.FP16X3_CONV33_WGRAD = False
    gw, n, took = once(xi, gi)
    assert (n, took) == (0, ["f2g_conv33_wgrad"]) and torch.equal(gw, p3)
    gw, n, took = once(c["x"], c["gy"])
    assert (n, took) == (0, ["f2g_conv33_wgrad"])
    close(gw, c["want"], c["tol"], "ops weight gradient, tunable off")
    ops.FP16X3_CONV33_WGRAD = True
    ops.set_gemm_precision("bf16x6")                        # the tunable means nothing outside the fp16x3 mode
    gw, n, took = once(xi, gi)
    assert (n, took) == (0, ["f2g_conv33_wgrad"]) and torch.equal(gw, p3)


# ------------------------------------------------------------------ 9. one MRD resolution against the CPU oracle
def test_mrd_resolution_against_oracle(ops):
    """one resolution's sub-discriminator at the shapes of tests/test_hip_disc_autograd.py with all six band-conv
    tunables on: scores, feature maps, the input gradient and every parameter gradient against the oracle at that
    file's tolerance; the (3, 3) weight-gradient counter moves with the tunable on and stands still with it off"""
    for n in TUNABLES:
        setattr(ops, n, True)
    r = subdisc_against_oracle(ops, "mrd", ("FP16X3_CONV33_WGRAD_LAUNCHES",),
                               "mrd resolution, fp16x3 band convolutions with the (3, 3) weight gradient")
    nw = r.fwd[0] + r.bwd[0]
    print(f"[conv33 fp16x3 wgrad] window {r.sub.window_length}: {nw} (3, 3) weight-gradient launches")
    assert nw > 0
    ops.FP16X3_CONV33_WGRAD = False
    assert r.rerun() == ((0,), (0,))
