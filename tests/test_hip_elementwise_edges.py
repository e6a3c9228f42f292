"""The thin kernels of csrc/elementwise.hip that every discriminator step runs between the MFMA kernels --
gradient landing (lrelu_bwd*), losses (l1, hinge, masked mse), column sums and copies -- at the sizes and
layouts flow2gan_amd/fused_disc.py calls them with, against float64 on the CPU, ELEMENT BY ELEMENT.

What these kernels can get wrong and the older tests cannot see: a grid-stride loop that wraps (every grid here
is capped, the workload's maps are far above the caps), the partly filled last group of the four-in-flight
float4 kernels, the host's choice between the float4 and the scalar kernel (alignment, n % 4, ld != cols), row
tails of the fused column-sum kernel, and the two edge values of the landing expression
(g + w * sign(y - f)) * (y > 0 ? 1 : slope): y == f (sign 0) and y == 0 / -0.0 (the slope side).

Bounds are derived, not tuned (u = 2^-24, the unit roundoff of fp32); every reference is built from the
fp32-rounded scalars the C ABI receives (ctypes c_float: w, slope, clip, and wg = w * wdev rounded once).
  * landing maps: three roundings (wg, the add, the multiply; wg * sign is exact)  ->  4 u (|g| + |wg|);
  * hinge / unclipped l1 gradients, copies, halos, masks: exact;  clipped l1 gradient: 4 u |want|;
  * sums (loss cells, column sums): (t + 8 + nb) u sum|term|, t = terms one thread adds serially, 8 = the block
    tree (6 wave steps + 2), nb = blocks / row slices that add to the same cell atomically; t and nb are worked
    out from the launch rule next to each check.  Loose by design -- the float64 sum of the fp32 terms must sit
    inside a quarter of it on the CPU before the GPU is asked -- the per-element checks are the sharp ones.
Every buffer a kernel writes a slice of carries the sentinel 7.0 around the slice and is compared WHOLE (bound 0
outside the slice); inputs are compared bit for bit afterwards; loss cells and column sums start non-zero.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
FILL = 7.0
# float4 groups of the wrapping vector cases: the grid of l1_loss4 / lrelu_bwd4 is f2g_grid_for(n4, 1024, 2048) =
# 2048 blocks of 256 threads, stride = 524288 float4, one outer trip = 4 * stride = 2048 * 1024.  This n4 gives a
# second trip whose u = 0 group is full (2048 * 256) and whose u = 1 group holds 77 float4
N4_WRAP = 2048 * 1024 + 2048 * 256 + 77
LAST_GROUP = 4 * (2048 * 1024 + 2048 * 256)       # first float of that partial group
LOSS_INIT = (0.75, -1.25, 0.5)                    # the cell under test is [1] (loss_offset = 1)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from flow2gan_amd import ops as o
    return o


@pytest.fixture(scope="module")
def pool():
    """Random fp32 data of the largest size, drawn once and only ever sliced and copied: three Gaussian vectors
    and two positive ones (lo in [0.25, 0.9], hi in [1.1, 4]: their logarithms have opposite signs)."""
    gen = torch.Generator().manual_seed(20240607)
    n = 4 * N4_WRAP
    p = {k: torch.randn(n, generator=gen) for k in ("g", "y", "f")}
    p["lo"] = 0.25 + 0.65 * torch.rand(n, generator=gen)
    p["hi"] = 1.1 + 2.9 * torch.rand(n, generator=gen)
    p["swap"] = torch.rand(n, generator=gen) < 0.5
    return p


def f32(x):
    """the value a C float parameter receives"""
    return ctypes.c_float(x).value


def f32mul(a, b):
    """one fp32 multiplication (wg = w * wdev[0] in the kernels)"""
    return float(np.float32(a) * np.float32(b))


def close_each(got, want64, bound, name=""):
    """|got - want| <= bound for EVERY element (bound: tensor of want's shape); reports the worst index."""
    got = got.detach().cpu().double().reshape(-1)
    want = want64.detach().cpu().double().reshape(-1)
    bound = torch.as_tensor(bound, dtype=torch.float64).reshape(-1)
    assert got.shape == want.shape == bound.shape, (name, got.shape, want.shape, bound.shape)
    err = (got - want).abs()
    bad = ~(err <= bound)                         # (a NaN is bad)
    if bool(bad.any()):
        over = torch.where(bad, torch.nan_to_num(err - bound, nan=math.inf), torch.full_like(err, -math.inf))
        i = int(over.argmax())
        raise AssertionError(f"{name}: {int(bad.sum())} of {got.numel()} elements outside their bound; worst at flat "
                             f"index {i}: got {got[i].item()!r}, want {want[i].item()!r}, bound {bound[i].item():.3e}")


def view2d(buf, rows, cols, ld, off):
    return buf.as_strided((rows, cols), (ld, 1), off)


def embed(data, rows, cols, ld, off, post=9, fill=FILL):
    """A flat buffer with the (rows, cols) data at row stride ld, `off` floats in, and `fill` everywhere else
    (in front, in the ld - cols gaps, behind)."""
    buf = torch.full((off + (rows - 1) * ld + cols + post,), fill, dtype=data.dtype)
    view2d(buf, rows, cols, ld, off).copy_(data.reshape(rows, cols))
    return buf


def grid_for(n, block, cap=2048 * 4):
    """common.h: f2g_grid_for"""
    return max(1, min((n + block - 1) // block, cap))


def flat_sum_rule(n, vec):
    """(t, nb) of the loss kernels: vec -> l1_loss4_kernel on f2g_grid_for(n / 4, 256 * 4, 2048) blocks, a thread
    takes the float4 groups i0 + k * gridDim * 256; else a grid-stride loop on f2g_grid_for(n, 256, 1024) blocks."""
    if vec:
        nb = grid_for(n // 4, 1024, 2048)
        return 4 * -(-(n // 4) // (nb * 256)), nb
    nb = grid_for(n, 256, 1024)
    return -(-n // (nb * 256)), nb


def colsum_rule(rows, ncol_lanes, rows_per_thread):
    """(t, nb, RS) of colsum_kernel (ncol_lanes = cols, 64 rows per thread) and lrelu_bwd_cs_kernel (ncol_lanes =
    C / 4, 32 rows per thread): CS = the power of two >= min(ncol_lanes, 256), RS = 256 / CS row lanes, rows_per =
    min(rows_per_thread * RS, rows) rows per blockIdx.y slice.  The thread that issues the atomic adds its own
    rows and then the RS - 1 other lanes' partials serially; one atomic per slice and column."""
    cs_log2 = 0
    while (1 << cs_log2) < ncol_lanes and cs_log2 < 8:
        cs_log2 += 1
    RS = 256 >> cs_log2
    rows_per = min(rows_per_thread * RS, rows)
    return -(-rows_per // RS) + RS - 1, -(-rows // rows_per), RS


def plant(y, f, idx):
    """The edge values of the landing expression at the flat indices idx of y (in turn): y == f, y == 0, y == -0.0
    (without f: zeros only)."""
    for k, i in enumerate(idx):
        kind = k % 3 if f is not None else 1 + k % 2
        y[i] = f[i] if kind == 0 else (0.0 if kind == 1 else -0.0)


def edge_indices(n):
    """first, last and a few inner elements (the last ones sit in the last, partly filled group)"""
    return sorted({i for i in (0, 1, 2, 3, 4, 5, n // 2, n // 2 + 1, n // 2 + 2, n - 6, n - 5, n - 4, n - 3, n - 2,
                               n - 1) if 0 <= i < n})


# ====================================================================== l1 loss
def check_l1(ops, Ab, a_off, Bb, b_off, rows, cols, ld, w, vec, clip=0.0, wdev=None, loss=True, grad=True, name=""):
    """f2g_l1_loss over the (rows, cols) views of the flat CPU buffers Ab / Bb (Bb may BE Ab: halves of one tensor)
    `a_off` / `b_off` floats in; gb follows b's layout.  vec = the kernel the case is meant for; the host rule is
    restated here so that a case cannot silently sit on the other side."""
    n = rows * cols
    assert vec == ((rows == 1 or ld == cols) and n % 4 == 0 and a_off % 4 == 0 and b_off % 4 == 0), name
    a32, b32 = view2d(Ab, rows, cols, ld, a_off), view2d(Bb, rows, cols, ld, b_off)
    a64, b64 = a32.double(), b32.double()
    w32, c32 = f32(w), f32(clip)
    wg = f32mul(w32, 1.0 if wdev is None else f32(wdev))
    if c32 > 0:
        d = torch.log(a64.clamp(min=c32)) - torch.log(b64.clamp(min=c32))
        t32 = (torch.log(a32.clamp(min=c32)) - torch.log(b32.clamp(min=c32))).abs().double()
        gwant = torch.where(b64 > c32, -wg * torch.sign(d) / b64, torch.zeros_like(d))
        gbound = 4 * U * gwant.abs()              # 1 / b, the product with it (+ wg)
    else:
        d = a64 - b64
        t32 = (a32 - b32).abs().double()
        gwant = -wg * torch.sign(d)               # exact: wg * sign * 1.0
        gbound = torch.zeros_like(d)
    tsum = w32 * float(d.abs().sum())
    t, nb = flat_sum_rule(n, vec)
    lbound = (t + 8 + nb) * U * (tsum + abs(LOSS_INIT[1])) + (2.0 ** -22 * tsum if c32 > 0 else 0.0)
    lwant = LOSS_INIT[1] + tsum
    assert abs(LOSS_INIT[1] + w32 * float(t32.sum()) - lwant) <= lbound / 4, (name, "fp32 terms leave no margin")

    A = Ab.to(DEV)
    B = A if Bb is Ab else Bb.to(DEV)
    GB = torch.full_like(B, FILL) if grad else None
    losses = torch.tensor(LOSS_INIT, device=DEV)
    wd = None if wdev is None else torch.tensor([wdev], device=DEV)
    if a_off == b_off:
        ops.l1_loss(losses if loss else None, GB, A, B, rows, cols, ld, w, clip=clip, wdev=wd, loss_offset=1, off=a_off)
    else:
        ops.l1_loss_ab(losses if loss else None, GB, A, a_off, B, b_off, rows, cols, ld, w, clip=clip, wdev=wd,
                       loss_offset=1)
    assert torch.equal(A.cpu(), Ab) and torch.equal(B.cpu(), Bb), f"{name}: an input changed"
    if grad:
        want = torch.full(Bb.shape, FILL, dtype=torch.float64)
        view2d(want, rows, cols, ld, b_off).copy_(gwant)
        bound = torch.zeros(Bb.shape, dtype=torch.float64)
        view2d(bound, rows, cols, ld, b_off).copy_(gbound)
        close_each(GB, want, bound, name=f"{name}: gradient buffer")
    got = losses.cpu()
    assert got[0].item() == LOSS_INIT[0] and got[2].item() == LOSS_INIT[2], f"{name}: a neighbouring loss cell changed"
    if loss:
        close_each(got[1:2], torch.tensor([lwant], dtype=torch.float64), torch.tensor([lbound]), name=f"{name}: loss")
    else:
        assert got[1].item() == LOSS_INIT[1]


def l1_inputs(pool, n, clip):
    """(a, b, clip) of n elements.  Unclipped: Gaussian with ties a == b planted (sign 0).  Clipped (1e-7): a and b
    from [0.25, 0.9] / [1.1, 4] on random halves, so |log a - log b| >= 0.2 (fp32 logf cannot flip the sign) and
    |log a| + |log b| = |term|; values at and below the clip planted on both sides, front and back."""
    if not clip:
        a, b = pool["g"][:n].clone(), pool["y"][:n].clone()
        for i in edge_indices(n)[::2]:
            a[i] = b[i]
        return a, b
    sw = pool["swap"][:n]
    a = torch.where(sw, pool["hi"][:n], pool["lo"][:n])
    b = torch.where(sw, pool["lo"][:n], pool["hi"][:n])
    c32 = f32(clip)
    for base in (0, max(0, n - 12)):
        for k, (av, bv) in enumerate([(1e-9, None), (1e-9, 1e-9), (None, 1e-9), (c32, None), (c32, c32), (None, c32),
                                      (1e-9, c32), (c32, 1e-9)]):
            if base + k < n:
                if av is not None:
                    a[base + k] = av
                if bv is not None:
                    b[base + k] = bv
    return a, b


@pytest.mark.parametrize("clip", [0.0, 1e-7])
@pytest.mark.parametrize("n4", [N4_WRAP, 1250, 3])
def test_l1_loss_vector_kernel(ops, pool, n4, clip):
    """l1_loss4_kernel: `(rows == 1 || ld == cols) && !(n & 3)` and a, b, gb 16-byte aligned.  N4_WRAP: the capped
    grid (2048 blocks) makes a second outer trip (`i0 += 4 * stride`) whose u = 1 group is partly filled; 1250 and
    3 float4: uncapped grids (2 blocks / 1 block) whose groups u = 1..3 are empty or ragged.  Loss and gradient,
    with a device weight; ties (unclipped) and clipped values also sit in the last group."""
    n = 4 * n4
    a, b = l1_inputs(pool, n, clip)
    check_l1(ops, embed(a, 1, n, n, 8), 8, embed(b, 1, n, n, 8), 8, 1, n, n, 3.0 / n, True, clip=clip, wdev=0.7,
             name=f"l1 vector n4={n4} clip={clip}")


@pytest.mark.parametrize("clip", [0.0, 1e-7])
@pytest.mark.parametrize("case", ["n%4==1", "b_off odd", "ld!=cols wrap", "ld!=cols small"])
def test_l1_loss_scalar_kernel(ops, pool, case, clip):
    """l1_loss_kernel, by each cause that fails the host test `(rows == 1 || ld == cols) && !(n & 3) && aligned`
    alone: n % 4 == 1; an odd b_off (n % 4 == 0, through l1_loss_ab, gb follows b); ld != cols with rows * cols =
    2 * 262144 + 77 (the grid is f2g_grid_for(n, 256, 1024): it wraps above 262144 elements; here every thread
    makes three trips, the last one ragged) and the small (5, 7, 12)."""
    rows, cols, ld, a_off, b_off = {"n%4==1": (1, 5001, 5001, 4, 4), "b_off odd": (1, 5000, 5000, 0, 1),
                                    "ld!=cols wrap": (155, 3383, 3388, 4, 4),
                                    "ld!=cols small": (5, 7, 12, 4, 4)}[case]
    assert case != "ld!=cols wrap" or rows * cols == 2 * 262144 + 77
    a, b = l1_inputs(pool, rows * cols, clip)
    check_l1(ops, embed(a, rows, cols, ld, a_off), a_off, embed(b, rows, cols, ld, b_off), b_off, rows, cols, ld,
             2.0 / (rows * cols), False, clip=clip, wdev=1.3, name=f"l1 scalar {case} clip={clip}")


@pytest.mark.parametrize("clip", [0.0, 1e-7])
@pytest.mark.parametrize("layout", ["halves vec", "halves scalar", "layer4 real-vs-fake", "layer4 same half"])
def test_l1_loss_layouts_of_fused_disc(ops, pool, layout, clip):
    """The two layouts of the fused walk.  Halves of one tensor [real; fake]: l1_loss_ab(losses, None, y, 0, y, n,
    1, n, n, 1 / n, loss_offset=1) -- n % 4 == 0 takes l1_loss4_kernel, an odd n (b_off = n unaligned) takes
    l1_loss_kernel.  Layer 4 of the MRD lives in the concatenated map: cols = W * 32, ld = Wcat * 32, offsets
    foff * 32 -- once with b `half` = rows * ld further on in the same map (l1_loss_ab, the fake half against the
    real one), once with the same offset into a second map (l1_loss, off=): `ld != cols` -> l1_loss_kernel.  Here
    with the gradient too (gb follows b)."""
    if layout.startswith("halves"):
        n = 1000 if layout == "halves vec" else 1001
        a, b = l1_inputs(pool, n, clip)
        buf = torch.cat([a, b, torch.full((9,), FILL)])
        check_l1(ops, buf, 0, buf, n, 1, n, n, 1.0 / n, n % 4 == 0, clip=clip, name=f"l1 {layout} clip={clip}")
        return
    rows, W, Wcat, foff = 6, 5, 9, 2
    cols, ld = W * 32, Wcat * 32
    half = rows * ld if layout == "layer4 real-vs-fake" else 0
    a, b = l1_inputs(pool, 2 * rows * cols, clip)
    cat = torch.full((2 * rows * ld + 9,), FILL)
    view2d(cat, rows, cols, ld, foff * 32).copy_(a[:rows * cols].reshape(rows, cols))
    other = cat
    if half:
        view2d(cat, rows, cols, ld, half + foff * 32).copy_(b[:rows * cols].reshape(rows, cols))
    else:       # the same slice of a second map (ops.l1_loss: one offset for both)
        other = embed(b[:rows * cols], rows, cols, ld, foff * 32)
    check_l1(ops, cat, foff * 32, other, half + foff * 32, rows, cols, ld, 1.0 / (rows * cols), False, clip=clip,
             wdev=0.7, name=f"l1 {layout} clip={clip}")


def test_l1_loss_one_output_at_a_time(ops, pool):
    """`if (!a || !b || (!loss && !gb)) return F2G_EINVAL`: loss alone and gradient alone work on both kernels
    (l1_loss4_kernel: n = 5000; l1_loss_kernel: n = 5001), neither is refused."""
    from flow2gan_amd._lib import F2GError
    for n in (5000, 5001):
        a, b = l1_inputs(pool, n, 0.0)
        Ab, Bb = embed(a, 1, n, n, 4), embed(b, 1, n, n, 4)
        check_l1(ops, Ab, 4, Bb, 4, 1, n, n, 1.0 / n, n % 4 == 0, wdev=0.7, grad=False, name=f"l1 loss only n={n}")
        check_l1(ops, Ab, 4, Bb, 4, 1, n, n, 1.0 / n, n % 4 == 0, wdev=0.7, loss=False, name=f"l1 grad only n={n}")
    A, B = a.to(DEV), b.to(DEV)
    with pytest.raises(F2GError):
        ops.l1_loss(None, None, A, B, 1, n, n, 1.0 / n)
    with pytest.raises(F2GError):
        ops.l1_loss_ab(None, None, A, 0, B, 0, 1, n, n, 1.0 / n)


# ====================================================================== hinge loss
@pytest.mark.parametrize("sgn", [-1.0, 1.0])
@pytest.mark.parametrize("n,s_off,outputs", [(2 * 262144 + 77, 3, "both"), (2 * 262144 + 77, 262145, "loss"),
                                             (5, 1, "both"), (5, 5, "grad"), (77, 77, "loss"), (4096, 4096, "grad")])
def test_hinge_loss(ops, pool, n, s_off, outputs, sgn):
    """hinge_loss_kernel: one grid-stride loop on f2g_grid_for(n, 256, 1024) blocks, so n = 2 * 262144 + 77 makes
    every thread wrap twice with a ragged last trip; n = 5 is one partly filled block.  `if (!s || (!loss && !gs))
    return F2G_EINVAL`: loss alone, gradient alone and both.  s_off (gs follows it) odd and non-zero, also the
    second-half call of fused_disc (s_off = n); loss_offset = 1; a device weight.  Scores with 1 + sgn * s == 0
    exactly are planted: `live = v > 0.f` makes them dead (no loss, gradient 0)."""
    s = pool["g"][:n].clone()
    for i in edge_indices(n)[::2]:
        s[i] = -sgn                               # 1 + sgn * s == 0
    for i in edge_indices(n)[1::4]:
        s[i] = -3.0 * sgn                         # clearly dead
    Sb = embed(s, 1, n, n, s_off)
    w, wdev = 1.0 / n, 0.7
    w32 = f32(w)
    wg = f32mul(w32, f32(wdev))
    v64 = 1.0 + sgn * s.double()
    live = v64 > 0
    gwant = torch.where(live, torch.full_like(v64, wg * sgn), torch.zeros_like(v64))
    tsum = w32 * float(v64[live].sum())
    t, nb = flat_sum_rule(n, False)               # the same launch rule as the scalar l1 kernel
    lbound = (t + 8 + nb) * U * (tsum + abs(LOSS_INIT[1]))
    lwant = LOSS_INIT[1] + tsum
    v32 = (1.0 + sgn * s).clamp(min=0).double()   # fp32 terms
    assert abs(LOSS_INIT[1] + w32 * float(v32.sum()) - lwant) <= lbound / 4

    S = Sb.to(DEV)
    GS = torch.full_like(S, FILL) if outputs != "loss" else None
    losses = torch.tensor(LOSS_INIT, device=DEV)
    ops.hinge_loss(losses if outputs != "grad" else None, GS, S, n, sgn, w, wdev=torch.tensor([wdev], device=DEV),
                   loss_offset=1, s_off=s_off)
    assert torch.equal(S.cpu(), Sb), "the scores changed"
    if GS is not None:
        want = embed(gwant, 1, n, n, s_off)
        close_each(GS, want, torch.zeros_like(want), name="hinge gradient buffer (exact)")
    got = losses.cpu()
    assert got[0].item() == LOSS_INIT[0] and got[2].item() == LOSS_INIT[2]
    if outputs != "grad":
        close_each(got[1:2], torch.tensor([lwant], dtype=torch.float64), torch.tensor([lbound]), name="hinge loss")
    else:
        assert got[1].item() == LOSS_INIT[1]


def test_hinge_loss_refuses_no_output(ops):
    """`if (!s || (!loss && !gs)) return F2G_EINVAL`"""
    from flow2gan_amd._lib import F2GError
    with pytest.raises(F2GError):
        ops.hinge_loss(None, None, torch.zeros(8, device=DEV), 8, 1.0, 1.0)


# ====================================================================== leaky-ReLU backward (landing)
def landing_ref(g32, y32, f32_, wg, slope32):
    """(want, bound) of (g + wg * sign(y - f)) * (y > 0 ? 1 : slope) in float64"""
    g64, y64 = g32.double(), y32.double()
    v = g64 if f32_ is None else g64 + wg * torch.sign(y64 - f32_.double())
    want = v * torch.where(y64 > 0, 1.0, slope32)
    return want, 4 * U * (g64.abs() + (abs(wg) if f32_ is not None else 0.0))


def check_lrelu(ops, Gb, g_off, Yb, y_off, Rb, r_off, rows, cols, ld, w, slope, vec, wdev=None, name=""):
    """f2g_lrelu_bwd in place over the (rows, cols) view of Gb; y_act / f_real are views of Yb / Rb (Rb may BE Yb
    or be None).  vec restates the host rule as in check_l1."""
    n = rows * cols
    assert vec == ((rows == 1 or ld == cols) and n % 4 == 0 and g_off % 4 == 0 and y_off % 4 == 0
                   and (Rb is None or r_off % 4 == 0)), name
    wg = f32mul(f32(w), 1.0 if wdev is None else f32(wdev))
    want, bound = landing_ref(view2d(Gb, rows, cols, ld, g_off), view2d(Yb, rows, cols, ld, y_off),
                              None if Rb is None else view2d(Rb, rows, cols, ld, r_off), wg, f32(slope))
    G, Y = Gb.to(DEV), Yb.to(DEV)
    R = Y if Rb is Yb else (None if Rb is None else Rb.to(DEV))
    ops.lrelu_bwd(G, Y, R, w, slope, rows, cols, ld, wdev=None if wdev is None else torch.tensor([wdev], device=DEV),
                  g_off=g_off, y_off=y_off, r_off=r_off)
    assert torch.equal(Y.cpu(), Yb) and (Rb is None or torch.equal(R.cpu(), Rb)), f"{name}: an input changed"
    wbuf, bbuf = Gb.double(), torch.zeros(Gb.shape, dtype=torch.float64)
    view2d(wbuf, rows, cols, ld, g_off).copy_(want)
    view2d(bbuf, rows, cols, ld, g_off).copy_(bound)
    close_each(G, wbuf, bbuf, name=name)


def landing_inputs(pool, n, with_f, extra=()):
    """Gaussian g, y, f of n elements with y == f, y == 0 and y == -0.0 planted at the edges and at `extra`."""
    g, y = pool["g"][:n].clone(), pool["y"][:n].clone()
    f = pool["f"][:n].clone() if with_f else None
    idx = edge_indices(n) + [i for i in extra if 0 <= i < n]
    plant(y, f, idx)
    if with_f:                                     # the double edge: y == f == 0
        y[idx[len(idx) // 2]] = 0.0
        f[idx[len(idx) // 2]] = 0.0
    return g, y, f


@pytest.mark.parametrize("with_f", [False, True])
@pytest.mark.parametrize("shape", [(1, 4 * N4_WRAP), (1, 4 * 1250), (1, 12), (5, 8)])
def test_lrelu_bwd_vector_kernel(ops, pool, shape, with_f):
    """lrelu_bwd4_kernel: `(rows == 1 || ld == cols) && !(n & 3)` and g, y_act, f_real 16-byte aligned.  N4_WRAP:
    2048 blocks, a second outer trip with a partly filled u = 1 group; 1250 and 3 float4 and (rows 5, ld == cols
    == 8): ragged groups on uncapped grids.  Ties y == f_real and zeros y == 0 / -0.0 are planted at both ends
    and inside the last partial group."""
    rows, cols = shape
    n = rows * cols
    g, y, f = landing_inputs(pool, n, with_f, extra=(LAST_GROUP, LAST_GROUP + 1, LAST_GROUP + 2, LAST_GROUP + 5,
                                                     4 * 2048 * 1024, 4 * 2048 * 1024 + 1, 4 * 2048 * 1024 + 2))
    check_lrelu(ops, embed(g, rows, cols, cols, 4), 4, embed(y, rows, cols, cols, 8), 8,
                embed(f, rows, cols, cols, 12) if with_f else None, 12, rows, cols, cols, 0.3, 0.1, True,
                wdev=0.7 if with_f else None, name=f"lrelu_bwd vector {shape} f={with_f}")


@pytest.mark.parametrize("case,with_f", [(c, f) for c in ("n%4==1", "n%4==2", "g_off odd", "y_off odd", "r_off odd",
                                                          "ld!=cols wrap", "ld!=cols small")
                                         for f in (False, True) if f or c != "r_off odd"])
def test_lrelu_bwd_scalar_kernel(ops, pool, case, with_f):
    """lrelu_bwd_kernel, by each cause that fails `(rows == 1 || ld == cols) && !(n & 3) && aligned` alone: n % 4
    != 0; an odd g_off, y_off or r_off; ld != cols with rows * cols = 2097152 + 4099 (the grid is f2g_grid_for(n,
    256) with the default cap of 8192 blocks: it wraps above 2097152 elements) and the small (5, 7, 12).  Ties and
    zeros planted at both ends; the gaps between rows keep their fill."""
    rows, cols, ld, offs = {"n%4==1": (1, 5001, 5001, (4, 8, 12)), "n%4==2": (1, 4998, 4998, (4, 8, 12)),
                            "g_off odd": (1, 5000, 5000, (1, 8, 12)), "y_off odd": (1, 5000, 5000, (4, 3, 12)),
                            "r_off odd": (1, 5000, 5000, (4, 8, 5)), "ld!=cols wrap": (51, 41201, 41204, (4, 8, 12)),
                            "ld!=cols small": (5, 7, 12, (4, 8, 12))}[case]
    assert case != "ld!=cols wrap" or rows * cols == 2097152 + 4099
    n = rows * cols
    g, y, f = landing_inputs(pool, n, with_f)
    check_lrelu(ops, embed(g, rows, cols, ld, offs[0]), offs[0], embed(y, rows, cols, ld, offs[1]), offs[1],
                embed(f, rows, cols, ld, offs[2]) if with_f else None, offs[2], rows, cols, ld, 0.3, 0.1, False,
                wdev=0.7 if with_f else None, name=f"lrelu_bwd scalar {case} f={with_f}")


@pytest.mark.parametrize("call", ["half map", "half map odd", "layer4 slice", "layer4 slice no fm", "scores",
                                  "scores odd"])
def test_lrelu_bwd_call_shapes_of_fused_disc(ops, pool, call):
    """The call shapes of fused_disc.py.  half map: lrelu_bwd(gm, y, y, w, SLOPE, 1, n, n, wdev=g1, y_off=n,
    r_off=0) -- g a fake-half-sized buffer, y the [real; fake] map, the fake half against the real one:
    lrelu_bwd4_kernel when n % 4 == 0, else (y_off = n unaligned) lrelu_bwd_kernel.  layer4 slice: lrelu_bwd(gcat,
    cat, cat, w, SLOPE, Sx * Ft, Wl * C, ldc, g_off=foff * C, y_off=half + foff * C, r_off=foff * C) and the same
    without the feature-matching term: `ld != cols` -> lrelu_bwd_kernel.  scores: lrelu_bwd(gs, sc, sc, 1 / nh,
    1.0, 1, nh, nh, wdev=g1, g_off=nh, y_off=nh, r_off=0) with slope 1.0 -- only the sign term acts; the first
    half of gs keeps its contents."""
    if call.startswith("half map"):
        n = 2048 if call == "half map" else 2049
        g, y, f = landing_inputs(pool, n, True)
        Yb = torch.cat([f, y, torch.full((9,), FILL)])          # [real; fake]
        check_lrelu(ops, embed(g, 1, n, n, 0), 0, Yb, n, Yb, 0, 1, n, n, 0.3, 0.1, n % 4 == 0, wdev=0.7, name=call)
    elif call.startswith("layer4"):
        rows, Wl, Wcat, foff, C = 6, 5, 9, 2, 32
        cols, ldc = Wl * C, Wcat * C
        half = rows * ldc
        with_f = call == "layer4 slice"
        g, y, f = landing_inputs(pool, rows * cols, True)
        cat = torch.full((2 * rows * ldc + 9,), FILL)
        view2d(cat, rows, cols, ldc, foff * C).copy_(f.reshape(rows, cols))
        view2d(cat, rows, cols, ldc, half + foff * C).copy_(y.reshape(rows, cols))
        check_lrelu(ops, embed(g, rows, cols, ldc, foff * C), foff * C, cat, half + foff * C, cat if with_f else None,
                    foff * C, rows, cols, ldc, 0.3 if with_f else 0.0, 0.1, False,
                    wdev=0.7 if with_f else None, name=call)
    else:
        nh = 80 if call == "scores" else 77
        g, y, f = landing_inputs(pool, nh, True)
        sc = torch.cat([f, y, torch.full((9,), FILL)])
        gs = torch.cat([pool["f"][100:100 + nh], g, torch.full((9,), FILL)])
        check_lrelu(ops, gs, nh, sc, nh, sc, 0, 1, nh, nh, 0.3, 1.0, nh % 4 == 0, wdev=0.7, name=call)


# ====================================================================== landing + column sums
def check_lrelu_colsum(ops, pool, rows, C, ld, with_f, with_cs, g_off=0, y_off=0, r_off=0, name=""):
    """f2g_lrelu_bwd_colsum over (rows, C) at row stride ld: the map as in check_lrelu, the column sums (onto a
    non-zero start, inside a sentinel frame) by the sum bound with (t, nb) of colsum_rule(rows, C / 4, 32)."""
    n = rows * C
    g, y, f = landing_inputs(pool, n, with_f, extra=(n - C, n - C + 1, n - C + 2, n - 2 * C, n - 2 * C + 1, C - 1, C))
    w, slope, wdev = 0.3, 0.1, 0.7
    wg = f32mul(f32(w), f32(wdev))
    Gb, Yb = embed(g, rows, C, ld, g_off), embed(y, rows, C, ld, y_off)
    Rb = embed(f, rows, C, ld, r_off) if with_f else None
    want, bound = landing_ref(g.reshape(rows, C), y.reshape(rows, C), f.reshape(rows, C) if with_f else None, wg,
                              f32(slope))
    init = pool["f"][500:500 + C].double()
    t, nb, _ = colsum_rule(rows, C // 4, 32)
    csbound = (t + 8 + nb) * U * (want.abs().sum(0) + init.abs())
    cswant = init + want.sum(0)
    assert bool(((init + want.float().double().sum(0) - cswant).abs() <= csbound / 4).all()), name

    G, Y = Gb.to(DEV), Yb.to(DEV)
    R = None if Rb is None else Rb.to(DEV)
    csb = torch.full((C + 8,), FILL)
    csb[4:4 + C] = init.float()
    CS = csb.to(DEV)
    ops.lrelu_bwd_colsum(G, Y, R, w, slope, rows, C, ld, CS[4:4 + C] if with_cs else None,
                         wdev=torch.tensor([wdev], device=DEV), g_off=g_off, y_off=y_off, r_off=r_off)
    assert torch.equal(Y.cpu(), Yb) and (Rb is None or torch.equal(R.cpu(), Rb)), f"{name}: an input changed"
    wbuf, bbuf = Gb.double(), torch.zeros(Gb.shape, dtype=torch.float64)
    view2d(wbuf, rows, C, ld, g_off).copy_(want)
    view2d(bbuf, rows, C, ld, g_off).copy_(bound)
    close_each(G, wbuf, bbuf, name=f"{name}: map")
    cwant, cb = csb.double(), torch.zeros(C + 8, dtype=torch.float64)
    if with_cs:
        cwant[4:4 + C] = cswant
        cb[4:4 + C] = csbound
    close_each(CS, cwant, cb, name=f"{name}: column sums")


@pytest.mark.parametrize("with_f,with_cs", [(False, True), (True, True), (True, False)])
@pytest.mark.parametrize("C,rows", [(32, 1), (32, 31), (32, 1024), (32, 2 * 1024 + 3 * 32 + 5), (1024, 3),
                                    (1024, 32 * 3 + 7), (24, 77), (1028, 37)])
def test_lrelu_bwd_colsum(ops, pool, C, rows, with_f, with_cs):
    """lrelu_bwd_cs_kernel (f2g_lrelu_bwd_colsum: `CS = 2^cs_log2 >= C / 4` capped at 256, `RS = 256 >> cs_log2`,
    `rows_per = min(32 * RS, rows)`, grid (ceil(C4 / CS), ceil(rows / rows_per))).  C = 32: RS = 32, 1024 rows per
    slice -- 1 row and 31 rows (idle row lanes, remainder loop only), 1024 (the unrolled loop exactly), 2149 = two
    full slices and a third with three unrolled trips for some lanes and the remainder loop for others.  C = 1024:
    RS = 1, 32 rows per slice -- 3 rows (remainder only), 103 (slices + a 7-row one: one unrolled trip + 3).  C =
    24: six column groups on CS = 8 (`c < C4` idles two lanes).  C = 1028: 257 groups -> two column blocks, the
    second with one live lane.  Ties and zeros sit in the first and the last rows."""
    check_lrelu_colsum(ops, pool, rows, C, C, with_f, with_cs, name=f"lrelu_bwd_colsum C={C} rows={rows}")


def test_lrelu_bwd_colsum_strided_with_offsets(ops, pool):
    """lrelu_bwd_cs_kernel with ld > C (`ld4 = ld / 4` row stride) and g_off / y_off / r_off into wider buffers;
    the ld - C gap keeps its fill."""
    check_lrelu_colsum(ops, pool, 70, 32, 48, True, True, g_off=16, y_off=32, r_off=4, name="lrelu_bwd_colsum ld=48")
    check_lrelu_colsum(ops, pool, 2 * 1024 + 9, 32, 40, False, True, g_off=8, y_off=4, name="lrelu_bwd_colsum ld=40")


def test_lrelu_bwd_colsum_refuses_unvectorisable_shapes(ops):
    """`if (!g || !y_act || (C & 3) || (ld & 3)) return F2G_EINVAL`: nothing is launched."""
    from flow2gan_amd._lib import F2GError
    G, Y = torch.full((8 * 40,), FILL, device=DEV), torch.ones(8 * 40, device=DEV)
    cs = torch.ones(32, device=DEV)
    with pytest.raises(F2GError):
        ops.lrelu_bwd_colsum(G, Y, None, 0.0, 0.1, 8, 30, 32, cs)
    with pytest.raises(F2GError):
        ops.lrelu_bwd_colsum(G, Y, None, 0.0, 0.1, 8, 32, 34, cs)
    torch.cuda.synchronize()
    assert bool((G == FILL).all()) and bool((cs == 1.0).all())


# ====================================================================== column sums
@pytest.mark.parametrize("cols,rows,prod,out_offset", [(1, 1000, False, 0), (1, 64 * 256 + 37, True, 3),
                                                       (32, 300, True, 0), (32, 2 * 512 + 37, False, 5),
                                                       (100, 77, False, 2), (100, 3 * 128 + 5, True, 0),
                                                       (300, 50, True, 0), (300, 2 * 64 + 9, False, 7)])
def test_colsum(ops, pool, cols, rows, prod, out_offset):
    """colsum_kernel (f2g_colsum: `CS = 2^cs_log2 >= cols` capped at 256, `RS = 256 >> cs_log2`, `rows_per =
    min(64 * RS, rows)`): cols 1 / 32 / 100 / 300 give RS 256 / 8 / 2 / 1 (300: two column blocks, `c < cols`),
    rows below one slice of 64 * RS rows and above it with a remainder; the product form b= and out_offset; a and
    b are the first columns of wider matrices (lda, ldb > cols), out is accumulated onto."""
    lda, ldb = cols + 3, cols + 5
    A = pool["g"][:rows * lda].reshape(rows, lda)
    B = pool["y"][:rows * ldb].reshape(rows, ldb)
    term = A[:, :cols].double() * (B[:, :cols].double() if prod else 1.0)
    init = pool["f"][:cols].double()
    t, nb, _ = colsum_rule(rows, cols, 64)
    bound = (t + 8 + nb) * U * (term.abs().sum(0) + init.abs())
    want = init + term.sum(0)
    t32 = (A[:, :cols] * B[:, :cols]).double() if prod else term
    assert bool(((init + t32.sum(0) - want).abs() <= bound / 4).all())
    ob = torch.full((out_offset + cols + 8,), FILL)
    ob[out_offset:out_offset + cols] = init.float()
    out, Ad, Bd = ob.to(DEV), A.to(DEV), B.to(DEV)
    ops.colsum(out, Ad[:, :cols], rows, cols, b=Bd[:, :cols] if prod else None, out_offset=out_offset)
    assert torch.equal(Ad.cpu(), A) and torch.equal(Bd.cpu(), B)
    wbuf, bbuf = ob.double(), torch.zeros(ob.shape, dtype=torch.float64)
    wbuf[out_offset:out_offset + cols] = want
    bbuf[out_offset:out_offset + cols] = bound
    close_each(out, wbuf, bbuf, name=f"colsum cols={cols} rows={rows}")


@pytest.mark.parametrize("nrows,W,Cc,ld,off", [(33, 5, 32, 9 * 32, 2 * 32), (70, 12, 32, 20 * 32, 3 * 32)])
def test_colsum_strided(ops, pool, nrows, W, Cc, ld, off):
    """ops.colsum_strided: two launches of colsum_kernel -- the (nrows, W * Cc) slice at row stride ld, `off`
    floats in, into a zeroed table, then the (W, Cc) table into out (accumulated).  W * Cc = 160 is one column
    block; 384 > 256 takes two.  The bound is the sum of the two launches' bounds over sum |a|."""
    a = pool["g"][:nrows * W * Cc].reshape(nrows, W * Cc)
    Ab = embed(a, nrows, W * Cc, ld, off)
    init = pool["f"][:Cc].double()
    a64 = a.double().reshape(nrows, W, Cc)
    want = init + a64.sum((0, 1))
    t1, nb1, _ = colsum_rule(nrows, W * Cc, 64)
    t2, nb2, _ = colsum_rule(W, Cc, 64)
    bound = (t1 + 8 + nb1 + t2 + 8 + nb2) * U * (a64.abs().sum((0, 1)) + init.abs())
    ob = torch.full((Cc + 8,), FILL)
    ob[:Cc] = init.float()
    out, A = ob.to(DEV), Ab.to(DEV)
    ops.colsum_strided(out, A, nrows, W, Cc, ld, off)
    assert torch.equal(A.cpu(), Ab)
    wbuf, bbuf = ob.double(), torch.zeros(ob.shape, dtype=torch.float64)
    wbuf[:Cc], bbuf[:Cc] = want, bound
    close_each(out, wbuf, bbuf, name="colsum_strided")


# ====================================================================== copies, halos, masks
@pytest.mark.parametrize("B,T", [(2, 1001), (3, 700417)])
def test_copy3_stacks_real_and_fake(ops, pool, B, T):
    """copy3_kernel as fused_disc stacks [real; fake]: copy3(x2, 0, T, real, 0, T, 1, B, T) and the same with
    out_offset = B * T.  The grid is f2g_grid_for(total, 256) (cap 8192 blocks): 3 * 700417 = 2097152 + 4099
    elements wrap it.  Exact; the eager path (ops.BATCH is None)."""
    assert ops.BATCH is None
    real, fake = pool["g"][:B * T], pool["y"][:B * T]
    x2 = torch.full((2 * B * T + 9,), FILL, device=DEV)
    ops.copy3(x2, 0, T, real.to(DEV), 0, T, 1, B, T)
    ops.copy3(x2, 0, T, fake.to(DEV), 0, T, 1, B, T, out_offset=B * T)
    assert torch.equal(x2.cpu(), torch.cat([real, fake, torch.full((9,), FILL)]))


@pytest.mark.parametrize("accumulate", [False, True])
def test_copy3_strided(ops, pool, accumulate):
    """copy3_kernel over three dimensions with different strides on the two sides (so1 != si1, n2 odd), offsets on
    both, plain (exact) and accumulate=True (`*o + v`: one rounding, u (|out| + |in|)); what lies between the rows
    keeps its fill.  A zero-stride source (the broadcast of leaf.py: si0 = 0) is copied too."""
    n0, n1, n2, so0, so1, si0, si1, oo, io = 3, 5, 7, 61, 11, 47, 9, 5, 2
    xin = pool["g"][:io + n0 * si0 + 9].clone()
    ob = torch.full((oo + n0 * so0 + 9,), FILL)
    src = xin.as_strided((n0, n1, n2), (si0, si1, 1), io)
    dst0 = pool["y"][:n0 * n1 * n2].reshape(n0, n1, n2)
    ob.as_strided((n0, n1, n2), (so0, so1, 1), oo).copy_(dst0)
    want, bound = ob.double(), torch.zeros(ob.shape, dtype=torch.float64)
    want.as_strided((n0, n1, n2), (so0, so1, 1), oo).copy_(src.double() + (dst0.double() if accumulate else 0.0))
    if accumulate:
        bound.as_strided((n0, n1, n2), (so0, so1, 1), oo).copy_(U * (src.double().abs() + dst0.double().abs()))
    out, X = ob.to(DEV), xin.to(DEV)
    ops.copy3(out, so0, so1, X, si0, si1, n0, n1, n2, accumulate=accumulate, out_offset=oo, in_offset=io)
    assert torch.equal(X.cpu(), xin)
    close_each(out, want, bound, name=f"copy3 strided accumulate={accumulate}")
    Cc, Bn = 13, 4
    tiled = torch.full((Bn * Cc + 3,), FILL, device=DEV)
    ops.copy3(tiled, Cc, 0, X, 0, 0, Bn, 1, Cc)
    assert torch.equal(tiled.cpu(), torch.cat([xin[:Cc].repeat(Bn), torch.full((3,), FILL)]))


@pytest.mark.parametrize("S,rows,C,lo,hi", [(3, 11, 32, 2, 2), (2, 9, 1024, 2, 2), (5, 7, 32, 0, 3)])
def test_zero_halo(ops, S, rows, C, lo, hi):
    """zero_halo_kernel: rows [0, lo) and [rows - hi, rows) of every sequence := 0 in float4 lanes; interior rows
    and what surrounds the buffer keep their fill.  (2, 9, 1024): (lo + hi) * C / 4 = 1024 lanes per sequence, 8
    blocks; lo = 0: one-sided."""
    buf = torch.full((4 + S * rows * C + 8,), FILL, device=DEV)
    ops.zero_halo(buf[4:4 + S * rows * C], S, rows, C, lo, hi)
    want = torch.full((S, rows, C), FILL)
    want[:, :lo] = 0.0
    want[:, rows - hi:] = 0.0
    assert torch.equal(buf.cpu(), torch.cat([torch.full((4,), FILL), want.reshape(-1), torch.full((8,), FILL)]))


def test_mask_rows(ops, pool):
    """mask_rows_kernel: rows f >= lens[b] of a (B * F, ld) matrix := 0 in its first C columns; lengths 0 and F
    (nothing / everything kept) and two in between; columns C.. and the kept rows are unchanged bit for bit."""
    B, Fr, C, ld = 4, 37, 10, 13
    lens = [0, Fr, 1, 20]
    x = pool["g"][:B * Fr * ld].reshape(B * Fr, ld)
    X = x.to(DEV)
    ops.mask_rows(X, B, Fr, C, torch.tensor(lens, dtype=torch.int32, device=DEV))
    want = x.clone().reshape(B, Fr, ld)
    for b, L in enumerate(lens):
        want[b, L:, :C] = 0.0
    assert torch.equal(X.cpu(), want.reshape(B * Fr, ld))


@pytest.mark.parametrize("B,T,lens", [(3, 87407, [0, 87407, 40000]), (3, 87407, None), (2, 5, [5, 2])])
def test_masked_mse(ops, pool, B, T, lens):
    """masked_mse_kernel: loss += inv_denom * sum e^2, g_err = 2 * inv_denom * e with e = pred - ref where t <
    lens[b], else 0; lens = None keeps everything.  The grid is f2g_grid_for(B * T, 256, 1024): B * T = 262144 + 77
    wraps it.  Gradient: two roundings (the difference, the product; 2 * inv_denom is exact) -> 3 u |want|; the
    loss by the sum bound."""
    n = B * T
    assert T < 1000 or n == 262144 + 77
    pred, ref = pool["g"][:n].reshape(B, T).clone(), pool["y"][:n].reshape(B, T)
    pred[-1, -1] = ref[-1, -1]                    # e == 0
    inv = 1.0 / max(1, sum(lens) if lens else n)
    inv32 = f32(inv)
    live = torch.ones(B, T, dtype=torch.bool)
    if lens is not None:
        live = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    e64 = torch.where(live, pred.double() - ref.double(), torch.zeros(B, T, dtype=torch.float64))
    gwant = 2.0 * inv32 * e64
    init = 0.625
    tsum = inv32 * float((e64 * e64).sum())
    nb = grid_for(n, 256, 1024)
    t = -(-n // (nb * 256))
    lbound = (t + 8 + nb) * U * (tsum + init)
    e32 = torch.where(live, pred - ref, torch.zeros(B, T))
    assert abs(init + inv32 * float((e32 * e32).double().sum()) - (init + tsum)) <= lbound / 4
    P, R = pred.to(DEV), ref.to(DEV)
    loss = torch.tensor([FILL, init, FILL], device=DEV)
    gerr = torch.full((n + 9,), FILL, device=DEV)
    ops.masked_mse(loss[1:2], gerr, P, R, B, T, None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV),
                   inv)
    assert torch.equal(P.cpu(), pred) and torch.equal(R.cpu(), ref)
    want = torch.cat([gwant.reshape(-1), torch.full((9,), FILL, dtype=torch.float64)])
    close_each(gerr, want, torch.cat([3 * U * gwant.abs().reshape(-1), torch.zeros(9, dtype=torch.float64)]),
               name="masked_mse gradient")
    close_each(loss, torch.tensor([FILL, init + tsum, FILL], dtype=torch.float64), torch.tensor([0.0, lbound, 0.0]),
               name="masked_mse loss")


def test_log_clip(ops, pool):
    """log_clip_kernel: x := logf(fmaxf(x, clip)) in place, values at, below (zero and negative too) and above the
    clip, over more than one block.  Bound 2^-22 |want|: two units in the last place for logf."""
    n, clip = 5003, 1e-7
    c32 = f32(clip)
    x = torch.exp(pool["g"][:n] * 6.0)            # e^-24 .. e^24, most of it above the clip
    x[:8] = torch.tensor([c32, 1e-9, 0.0, -1.0, float(np.nextafter(np.float32(c32), np.float32(1.0))), 1.0, 1e-30,
                          float(np.nextafter(np.float32(c32), np.float32(0.0)))])
    x[-3:] = torch.tensor([c32, 1e-12, 2.5])
    buf = torch.full((4 + n + 9,), FILL, device=DEV)
    buf[4:4 + n] = x.to(DEV)
    ops.log_clip_(buf[4:4 + n], clip)
    want = torch.log(x.double().clamp(min=c32))
    wbuf = torch.cat([torch.full((4,), FILL, dtype=torch.float64), want, torch.full((9,), FILL, dtype=torch.float64)])
    bbuf = torch.cat([torch.zeros(4, dtype=torch.float64), 2.0 ** -22 * want.abs(), torch.zeros(9, dtype=torch.float64)])
    close_each(buf, wbuf, bbuf, name="log_clip_")


# ====================================================================== ties and zeros in the fused store expressions
def close(got, want, rtol=2e-5, name=""):
    """the normwise comparison of the files these three cases come from (their own tolerances)"""
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = want.abs().max().item() + 1e-30
    err = (got - want).abs().max().item()
    assert err <= rtol * scale + 1e-30, f"{name}: max err {err:.3e} vs scale {scale:.3e}"


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def plant_pixels(yact, yreal, pixels):
    """yact, yreal: (positions, channels).  At the given positions in turn: the whole pixel tied (yact == yreal),
    the whole pixel zero (+0.0 in the first half of the channels, -0.0 in the second), and both (yact == yreal ==
    0)."""
    h = yact.shape[1] // 2
    for k, p in enumerate(pixels):
        if k % 3 == 0:
            yact[p] = yreal[p]
        elif k % 3 == 1:
            yact[p, :h] = 0.0
            yact[p, h:] = -0.0
        else:
            yact[p] = 0.0
            yreal[p] = 0.0


@pytest.mark.parametrize("mode", ["default", "bf16x6"])
def test_conv32_dgrad_landing_ties_and_zeros(ops, mode):
    """c32_mask_fm (conv32_common.h), the store expression of the MRD data gradients: `v += fmw * (dl > 0.f ? 1.f :
    (dl < 0.f ? -1.f : 0.f))` then `v * (y > 0.f ? 1.f : mask_slope)`, through conv32_s2_dgrad with mask + fm +
    colsum at (S, H, Win) = (3, 11, 13) -- conv32.hip in the default mode, conv32x6.hip in bf16x6.  Pixels with yact
    == yreal, yact == +-0 and both are planted in the corners, the last ones on the partial edge tiles (H = 11 and
    Win = 13 fill neither an 8 x 16 nor a 16 x 8 tile).  Reference and tolerances of
    test_direct_conv32_dgrad_fused_lrelu_backward."""
    S, H, Win = 3, 11, 13
    Wout = (Win - 1) // 2 + 1
    w = rnd(32, 32, 3, 9, seed=2, scale=0.05)
    gy = rnd(S * H * Wout, 32, seed=4)
    yact = rnd(S * H * Win, 32, seed=5)
    yact = torch.where(yact > 0, yact, 0.1 * yact)
    yreal = rnd(S * H * Win, 32, seed=6)
    pix = lambda s, h, x: (s * H + h) * Win + x
    plant_pixels(yact, yreal, [pix(0, 0, 0), pix(0, 0, 1), pix(0, 1, 0), pix(1, 5, 6), pix(1, 5, 7), pix(1, 6, 6),
                               pix(2, 10, 12), pix(2, 10, 11), pix(2, 9, 12), pix(0, 10, 12), pix(1, 8, 12),
                               pix(2, 10, 0)])
    wdev = torch.tensor([0.7])
    wT = w.permute(2, 3, 1, 0).reshape(27, 32, 32).contiguous()
    x = torch.zeros(S, 32, H, Win, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), None, stride=(1, 2), padding=(1, 4)).backward(
        gy.reshape(S, H, Wout, 32).permute(0, 3, 1, 2).double())
    base = x.grad.permute(0, 2, 3, 1).reshape(S * H * Win, 32)
    wg = f32mul(f32(0.25), f32(0.7))
    want = (base + wg * torch.sign(yact.double() - yreal.double())) * torch.where(yact > 0, 1.0, f32(0.1)).double()
    was = ops.GEMM_PRECISION, ops.FP16X3
    try:
        if mode != "default":
            ops.set_gemm_precision(mode)
        gx = torch.full((S * H * Win, 32), FILL, device=DEV)
        cs = torch.zeros(32, device=DEV)
        Y, R = yact.to(DEV), yreal.to(DEV)
        ops.conv32_s2_dgrad(gy.to(DEV), S, H, Win, Wout, wT.to(DEV), gx, mask=(Y, 0, 0.1),
                            fm=(R, 0, 0.25, wdev.to(DEV)), colsum=cs)
    finally:
        ops.GEMM_PRECISION, ops.FP16X3 = was
    assert torch.equal(Y.cpu(), yact) and torch.equal(R.cpu(), yreal)
    close(gx, want, name=f"conv32 dgrad + landing, ties and zeros ({mode})")
    close(cs, want.sum(0), rtol=1e-4, name="column sums")


def test_mpdpost_dgrad_landing_ties_and_zeros(ops):
    """mpdpost data gradient (mpd0.hip) with mask + fm at (S, H) = (5, 27): its store adds `fmw * sign(y - ref)` and
    multiplies by `y > 0 ? 1 : slope` per float4.  Positions with y == ref, y == +-0 and both are planted in the
    first and last rows of the sequences.  Reference and tolerance of test_mpd_last_layer_direct_kernels."""
    S, H, HALO, Cc = 5, 27, 2, 1024
    y = torch.zeros(S, H + 2 * HALO, Cc)
    y[:, HALO:HALO + H] = rnd(S, H, Cc, seed=1)
    ref_map = torch.zeros(S, H + 2 * HALO, Cc)
    ref_map[:, HALO:HALO + H] = rnd(S, H, Cc, seed=6)
    pos = lambda s, h: s * (H + 2 * HALO) + HALO + h
    yv, rv = y.view(-1, Cc), ref_map.view(-1, Cc)
    plant_pixels(yv, rv, [pos(0, 0), pos(0, 1), pos(0, 2), pos(2, 13), pos(2, 14), pos(2, 15), pos(4, 26), pos(4, 25),
                          pos(4, 24)])
    w = rnd(1, Cc, 3, seed=2) * 0.05
    w3 = w[0].t().contiguous()
    gs = rnd(S, H, seed=4)
    yd = y[:, HALO:HALO + H].permute(0, 2, 1).double().requires_grad_(True)
    F.conv1d(yd, w.double(), None, padding=1).backward(gs[:, None, :].double())
    plain = yd.grad.permute(0, 2, 1)
    y64, r64 = y[:, HALO:HALO + H].double(), ref_map[:, HALO:HALO + H].double()
    wg = f32mul(f32(0.3), f32(0.7))
    want = (plain + wg * torch.sign(y64 - r64)) * torch.where(y64 > 0, 1.0, f32(0.1))
    gm = torch.zeros(S * (H + 2 * HALO), Cc, device=DEV)
    cs = torch.zeros(Cc, device=DEV)
    ops.mpdpost_dgrad(gs.to(DEV), S, H, HALO, w3.to(DEV), gm, mask=(y.to(DEV), 0, 0.1),
                      fm=(ref_map.to(DEV), 0, 0.3, torch.tensor([0.7], device=DEV)), colsum=cs)
    gmv = gm.view(S, H + 2 * HALO, Cc)
    close(gmv[:, HALO:HALO + H], want, name="mpdpost dgrad + landing, ties and zeros")
    assert float(gmv[:, :HALO].abs().max()) == 0.0 and float(gmv[:, HALO + H:].abs().max()) == 0.0
    close(cs, want.sum((0, 1)), rtol=1e-4, name="mpdpost column sums")


def test_gemm_mask_epilogue_ties_and_zeros(ops, monkeypatch):
    """The GEMM epilogue's mask= (+ fm=) store (x6_epilogue.h: `v[e] += fmw * sign(y[e] - f[e])`, `v[e] *= y[e] >
    0.f ? 1.f : E.mask_slope`) at the smallest shape of test_fp32_class_gemm_with_32_output_columns, (S, Hp, Cout,
    nt) = (5, 300, 64, 2): rows of the mask map with y == +-0 (mask only), then also y == ref and both (mask + fm)
    are planted at stored rows of the first tile and of the last, partly filled 128-row tile (5 * 299 = 11 * 128 +
    87 rows).  Reference and tolerances of that test."""
    S, Hp, Cout, nt = 5, 300, 64, 2
    monkeypatch.setattr(ops, "X6F_TALL_ROWS", 1000)
    monkeypatch.setattr(ops, "X6_MIN_ROWS", 1)
    gen = torch.Generator().manual_seed(S + Hp)
    Lq = Hp - nt + 1
    gmap = torch.randn(S, Hp, Cout, generator=gen)
    w = torch.randn(32, nt * Cout, generator=gen) * 0.05
    cols = torch.stack([gmap[:, i:i + Lq] for i in range(nt)], 2).reshape(S * Lq, nt * Cout)
    ref = (cols.double() @ w.double().t()).reshape(S, Lq, 32)
    Hin = 3 * Lq + 4
    ymask = torch.randn(S * Hin, 32, generator=gen)
    yreal = torch.randn(S * Hin, 32, generator=gen)
    rows = 2 + 3 * torch.arange(Lq)
    row = lambda s, q: s * Hin + 2 + 3 * q
    plant_pixels(ymask, yreal, [row(0, 0), row(0, 1), row(0, 2), row(2, 150), row(2, 151), row(2, 152),
                                row(4, Lq - 1), row(4, Lq - 2), row(4, Lq - 3), row(4, Lq - 80), row(4, Lq - 50)])
    wd = torch.nn.Parameter(w.to(DEV))
    wg = f32mul(f32(0.25), f32(0.7))
    m = ymask.reshape(S, Hin, 32)[:, rows].double()
    r = yreal.reshape(S, Hin, 32)[:, rows].double()
    untouched = torch.ones(Hin, dtype=torch.bool)
    untouched[rows] = False
    was = ops.GEMM_PRECISION, ops.FP16X3
    try:
        ops.set_gemm_precision("bf16x6")
        for use_fm in (False, True):
            out = torch.full((S * Hin, 32), FILL, device=DEV)
            cs = torch.zeros(32, device=DEV)
            A = ops.win1d(gmap.reshape(S * Hp, Cout).to(DEV), S, Hp, Cout, Lq, 1, 0, nt)
            ops.gemm(A, ops.mat(wd), out, rowmap=(Lq, Hin * 32, 3 * 32, 2 * 32), mask=(ymask.to(DEV), 0, 0.1),
                     fm=(yreal.to(DEV), 0, 0.25, torch.tensor([0.7], device=DEV)) if use_fm else None, colsum=cs)
            if not use_fm:
                assert ops.L.lib.f2g_gemm_last_path() == 5, "the 32-column launch did not take gemm_x6n_kernel"
            want = (ref + (wg * torch.sign(m - r) if use_fm else 0.0)) * torch.where(m > 0, 1.0, f32(0.1))
            o = out.cpu().reshape(S, Hin, 32)
            close(o[:, rows].double(), want, rtol=2e-5, name=f"masked rowmapped output (fm={use_fm})")
            assert bool((o[:, untouched] == FILL).all())
            close(cs.cpu().double(), want.sum((0, 1)), rtol=1e-4, name=f"column sums (fm={use_fm})")
    finally:
        ops.GEMM_PRECISION, ops.FP16X3 = was
