"""conv32h3w.hip on the GPU: the fp16x3 weight gradient of the MRD band convolutions (f2g_conv32_s2_wgrad_h3) with
one monotone running scale per operand and block, against float64 autograd of F.conv2d.

What the structure can get wrong, at the smallest shapes that show it: a wrong two-piece fragment, patch offset per
tap, piece order, accumulator tile or flush address (one k step at a time), a scale that does not follow the block's
walk or accumulators that do not follow the scale (sequences and tile bands many binades apart, blocks of two and
three tiles), the accumulation into a prefilled matrix with few tiles and degenerate widths, where the maximum is
looked for (zeros, a halo pixel, a NaN), the strided gradient input, the descriptors the entry point must refuse, the
Python routing with its tunable and counter, and one MRD window end to end against the CPU oracle.

Tolerance, per element: 1.8e-6 * sum |g||x| (the TOL of the fp16x3 GPU tests) + 2^-28 sum_T (xrun_T sum_{px in T} |g|
+ grun_T sum_{px in T} |x|), the floor term of the running scales (tests/fp16x3_conv32w_emul.py: bound_wgrad).
Shapes are (S, H, Win); gw is (32, 27 * 32) [co][tap][ci].
"""
import ctypes as C
import functools

import pytest
import torch

import fp16x3_conv32w_emul as emul
from fp16x3_gpu import EINVAL, TOL, fp16x3_mode, library, subdisc_against_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture
def ops():
    """the fp16x3 mode with the weight-gradient tunable on; mode and band-conv tunables restored afterwards"""
    with fp16x3_mode(library(), "FP16X3_CONV32_FWD", "FP16X3_CONV32_DGRAD", "FP16X3_CONV32_WGRAD") as o:
        o.FP16X3_CONV32_WGRAD = True
        yield o


def g(t):
    return t.to(DEV).contiguous()


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def wout_of(Win):
    return (Win - 1) // 2 + 1


def pow2(e):
    return torch.ldexp(torch.ones(e.shape), e)


def spread(t, flip):
    """sequence s times 2^((7 s mod 41) - 20), tile-to-tile bands inside each sequence: rows times
    2^((5 (h // 8) mod 13) - 6), columns times 2^((3 (w // 16) mod 7) - 3); flip (the gradient): over s and over h"""
    S, H, W = t.shape[:3]
    seq = pow2((7 * torch.arange(S)) % 41 - 20)
    rows = pow2((5 * (torch.arange(H) // 8)) % 13 - 6)
    cols = pow2((3 * (torch.arange(W) // 16)) % 7 - 3)
    if flip:
        seq, rows = seq.flip(0), rows.flip(0)
    return t * seq[:, None, None, None] * rows[None, :, None, None] * cols[None, None, :, None]


def reference(x, gy):
    """(float64 gradient, per-element tolerance)"""
    return emul.exact_wgrad(x, gy), emul.bound_wgrad(x, gy, rel=TOL)[0]


@functools.lru_cache(maxsize=None)
def case(S, H, Win, seed=0, spread_out=False):
    """Inputs, float64 reference and per-element tolerance of one shape: computed once, shared, not modified."""
    x, gy = rnd(S, H, Win, 32, seed=11 + seed), rnd(S, H, wout_of(Win), 32, seed=14 + seed)
    if spread_out:
        x, gy = spread(x, False), spread(gy, True)
    want, tol = reference(x, gy)
    return dict(x=x, gy=gy, want=want, tol=tol)


def close(got, want, tol, name):
    got = got.detach().cpu().double().reshape(want.shape)
    err = (got - want).abs()
    bad = ~(err <= tol)                                     # (a NaN fails)
    worst = float((err / tol)[tol > 0].max()) if bool((tol > 0).any()) else 0.0
    print(f"[conv32 fp16x3 wgrad] {name}: worst error {worst:.3f} of the tolerance")
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements beyond the tolerance, worst {worst:.3f} of it"


def run(ops, x, gy, prefill=None):
    """one launch through ops: gw (32, 864) = prefill (zeros) + the gradient"""
    S, H, Win = x.shape[:3]
    gw = torch.zeros(32, 27 * 32, device=DEV) if prefill is None else g(prefill.clone())
    n0 = ops.FP16X3_CONV32_WGRAD_LAUNCHES
    ops.conv32_s2_wgrad(g(x).view(-1, 32), g(gy).view(-1, 32), S, H, Win, wout_of(Win), gw)
    assert ops.FP16X3_CONV32_WGRAD_LAUNCHES == n0 + 1
    return gw


# ------------------------------------------------------------------ 1. one k step at a time
@pytest.mark.parametrize("S,H,Win,th,tw", [(2, 9, 21, 8, 16), (2, 16, 8, 16, 8)])
def test_one_k_step_at_a_time(ops, S, H, Win, th, tw):
    """The gradient zero except for ONE tile row of one tile (a k step on 8 x 16 tiles, half of one on 16 x 8), then
    the input zero except for one 16-channel half, then the same for the gradient's channels: the WHOLE gw is compared
    each time, so a wrong hi / lo fragment, patch offset per tap, piece order, accumulator tile or flush address all
    fail, and so does a contribution from a k step that should be silent."""
    assert emul.pick_tiles(H, wout_of(Win))[:2] == (th, tw)
    c = case(S, H, Win)
    for row in range(th):
        gy = torch.zeros_like(c["gy"])
        gy[1, row] = c["gy"][1, row]                         # sequence 1: the tile row of its first tile
        close(run(ops, c["x"], gy), *reference(c["x"], gy), f"{(S, H, Win)}, tile row {row}")
    for half in range(2):
        sl = slice(16 * half, 16 * half + 16)
        x = torch.zeros_like(c["x"])
        x[..., sl] = c["x"][..., sl]
        close(run(ops, x, c["gy"]), *reference(x, c["gy"]), f"{(S, H, Win)}, input channel half {half}")
        gy = torch.zeros_like(c["gy"])
        gy[..., sl] = c["gy"][..., sl]
        close(run(ops, c["x"], gy), *reference(c["x"], gy), f"{(S, H, Win)}, output channel half {half}")


# ------------------------------------------------------------------ 2. the scales move with the walk
@pytest.mark.parametrize("S,H,Win,tiles,per", [(34, 47, 77, (16, 8), 2), (70, 47, 39, (16, 8), 3),
                                               (70, 24, 63, (8, 16), 2)])
def test_scales_move_with_the_walk(ops, S, H, Win, tiles, per):
    """Blocks walk two or three consecutive tiles.  Sequences lie up to 40 binades apart and the tiles inside a
    sequence up to 18, in opposite directions for the two operands: a scale taken from the wrong tile, accumulators
    that are not rescaled when a scale drops, or only one of the two sets rescaled, all leave the tolerance.  Two
    launches with different inputs into separate gw."""
    w = emul.walk(*(case(S, H, Win, 0, True)[k] for k in ("x", "gy")))
    assert (w["th"], w["tw"]) == tiles and w["per"] == per
    for seed in (0, 1):
        c = case(S, H, Win, seed, True)
        close(run(ops, c["x"], c["gy"]), c["want"], c["tol"], f"{(S, H, Win)}, launch {seed}")


# ------------------------------------------------------------------ 3. accumulate; few tiles, degenerate widths
@pytest.mark.parametrize("S,H,Win", [(1, 5, 2), (2, 9, 1), (2, 16, 16), (2, 8, 64)])
def test_accumulates_into_a_prefilled_matrix(ops, S, H, Win):
    """gw comes back as prefill + gradient (the fp32 additions: TOL of the prefill on top).  One partial tile with
    Wout = 1; Win = 1; tile-exact 16 x 8 and 8 x 16."""
    c = case(S, H, Win)
    prefill = rnd(32, 27 * 32, seed=31, scale=3.0)
    close(run(ops, c["x"], c["gy"], prefill), c["want"] + prefill.double(), c["tol"] + TOL * prefill.double().abs(),
          f"{(S, H, Win)}, prefilled")


# ------------------------------------------------------------------ 4. zeros, a halo maximum, a NaN
def test_zero_inputs_leave_the_prefill(ops):
    S, H, Win = 2, 9, 21
    prefill = rnd(32, 27 * 32, seed=32)
    c = case(S, H, Win)
    for x, gy in ((torch.zeros_like(c["x"]), torch.zeros_like(c["gy"])), (c["x"], torch.zeros_like(c["gy"])),
                  (torch.zeros_like(c["x"]), c["gy"])):
        assert torch.equal(run(ops, x, gy, prefill).cpu(), prefill)


def test_maximum_in_the_halo_of_a_tile(ops):
    """(2, 9, 63): 8 x 16 tiles, two per row.  Sequence 0 is zero except for ONE input pixel of 2^20 that belongs to the
    second tile's columns and lies in the first tile's halo (tests/test_hip_conv32_f16.py places it the same way): a
    maximum taken over a tile's own columns alone would leave the first tile at scale 1 and 2^20 outside fp16."""
    S, H, Win = 2, 9, 63
    x, gy = rnd(S, H, Win, 32, seed=5), rnd(S, H, wout_of(Win), 32, seed=6)
    x[0] = 0.0
    x[0, 3, 34, 7] = 2.0 ** 20        # input column 34: the centre of output column 17, in the window of column 15
    gw = run(ops, x, gy)
    assert bool(torch.isfinite(gw).all())
    close(gw, *reference(x, gy), "maximum in the halo")


def test_a_nan_pixel_stays_in_its_sums(ops):
    """One NaN in x[1, 9, 30, 5]: exactly the (tap, ci) pairs whose own sums hold it are NaN, for every co; the other
    outputs stay within the tolerance computed with the NaN zeroed."""
    S, H, Win = 2, 20, 63
    x, gy = rnd(S, H, Win, 32, seed=7), rnd(S, H, wout_of(Win), 32, seed=8)
    x[1, 9, 30, 5] = float("nan")
    holds = emul.exact_wgrad(torch.isnan(x).float(), torch.ones_like(gy)) > 0
    assert int(holds.sum()) == 32 * 15                      # three tap rows x the five even tap columns, ci = 5
    got = run(ops, x, gy).cpu().double()
    assert bool(torch.isnan(got[holds]).all()), "a sum that holds the NaN is not NaN"
    want, tol = reference(x.nan_to_num(0.0), gy)
    err = (got - want).abs()
    assert bool((err[~holds] <= tol[~holds]).all()), "the NaN reached another sum"


# ------------------------------------------------------------------ 5. strided gradient
@pytest.mark.parametrize("S,H,Win", [(3, 11, 13), (24, 94, 77)])
def test_strided_offset_gradient(ops, S, H, Win):
    """The gradient is a band's slice of a wider map (y_line, y_seq and a pointer offset at the C level), as fused_disc
    holds it.  The neighbouring bands' columns are 2^10 louder: they are outside the map and must reach neither the
    running maximum nor the sums."""
    Wout = wout_of(Win)
    c = case(S, H, Win)
    lo, Wtot = 5, Wout + 9
    wide = rnd(S, H, Wtot, 32, seed=21) * 1024.0
    wide[:, :, lo:lo + Wout] = c["gy"]
    wide, x = g(wide), g(c["x"])
    gw = torch.zeros(32, 27 * 32, device=DEV)
    d = ops.L.Conv32Desc()
    d.S, d.H, d.Win, d.Wout, d.precision = S, H, Win, Wout, 4
    d.x, d.x_seq, d.x_line = x.data_ptr(), H * Win * 32, Win * 32
    d.y, d.y_seq, d.y_line = wide.data_ptr() + 4 * lo * 32, H * Wtot * 32, Wtot * 32
    assert ops.L.lib.f2g_conv32_s2_wgrad_h3(C.byref(d), gw.data_ptr(), ops.L.stream_ptr()) == 0
    torch.cuda.synchronize()
    close(gw, c["want"], c["tol"], f"{(S, H, Win)}, strided gradient")


# ------------------------------------------------------------------ 6. refusals
def test_refusals(ops):
    S, H, Win = 2, 9, 21
    Wout = wout_of(Win)
    c = case(S, H, Win)
    lib, st = ops.L.lib, ops.L.stream_ptr()
    x, gy = g(c["x"]), g(c["gy"])
    gw = torch.full((32, 27 * 32), 7.0, device=DEV)

    def desc():
        d = ops.L.Conv32Desc()
        d.S, d.H, d.Win, d.Wout, d.precision = S, H, Win, Wout, 4
        d.x, d.x_seq, d.x_line = x.data_ptr(), H * Win * 32, Win * 32
        d.y, d.y_seq, d.y_line = gy.data_ptr(), H * Wout * 32, Wout * 32
        return d

    for field, value in (("precision", 3), ("precision", 0), ("x", x.data_ptr() + 4), ("y_line", Wout * 32 + 2)):
        d = desc()
        setattr(d, field, value)
        assert lib.f2g_conv32_s2_wgrad_h3(C.byref(d), gw.data_ptr(), st) == EINVAL, field
    torch.cuda.synchronize()
    assert bool((gw == 7.0).all()), "a refused launch wrote gw"
    assert lib.f2g_conv32_s2_wgrad_h3(C.byref(desc()), gw.data_ptr(), st) == 0      # (the descriptor itself is fine)
    torch.cuda.synchronize()
    close(gw, c["want"] + 7.0, c["tol"] + TOL * 7.0, "the intact descriptor")


# ------------------------------------------------------------------ 7. routing
def test_ops_route(ops, monkeypatch):
    """The tunable on: the new entry point, the counter moves by one per call.  Off, or in bf16x6: the counter stands
    still and the call goes to f2g_conv32_s2_wgrad as before."""
    S, H, Win = 3, 11, 13
    c = case(S, H, Win)
    names, real_call = [], ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
    xg, gg = g(c["x"]).view(-1, 32), g(c["gy"]).view(-1, 32)

    def once():
        gw = torch.zeros(32, 27 * 32, device=DEV)
        del names[:]
        n0 = ops.FP16X3_CONV32_WGRAD_LAUNCHES
        ops.conv32_s2_wgrad(xg, gg, S, H, Win, wout_of(Win), gw)
        torch.cuda.synchronize()
        return gw, ops.FP16X3_CONV32_WGRAD_LAUNCHES - n0, [n for n in names if "wgrad" in n]

    for _ in range(2):
        gw, n, took = once()
        assert (n, took) == (1, ["f2g_conv32_s2_wgrad_h3"])
        close(gw, c["want"], c["tol"], "ops weight gradient")
    ops.FP16X3_CONV32_WGRAD = False
    _, n, took = once()
    assert (n, took) == (0, ["f2g_conv32_s2_wgrad"])
    ops.FP16X3_CONV32_WGRAD = True
    ops.set_gemm_precision("bf16x6")                        # the tunable means nothing outside the fp16x3 mode
    _, n, took = once()
    assert (n, took) == (0, ["f2g_conv32_s2_wgrad"])


# ------------------------------------------------------------------ 8. one MRD window against the CPU oracle
def test_mrd_window_against_oracle(ops):
    """one resolution's sub-discriminator at the shapes of tests/test_hip_disc_autograd.py with all three band-conv
    tunables on: scores, feature maps, the input gradient and every parameter gradient against the oracle at that
    file's tolerance; the weight-gradient counter moves with the tunable on and stands still with it off"""
    ops.FP16X3_CONV32_FWD = ops.FP16X3_CONV32_DGRAD = True
    r = subdisc_against_oracle(ops, "mrd", ("FP16X3_CONV32_WGRAD_LAUNCHES",),
                               "mrd window, fp16x3 band convolutions with the weight gradient")
    nw = r.fwd[0] + r.bwd[0]
    print(f"[conv32 fp16x3 wgrad] window {r.sub.window_length}: {nw} weight-gradient launches")
    assert nw > 0
    ops.FP16X3_CONV32_WGRAD = False
    assert r.rerun() == ((0,), (0,))
