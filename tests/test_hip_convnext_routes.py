"""Route matrix of csrc/convnext.hip: every instance of the dwnorm, dwconv and BiasNorm kernels the dispatch
can pick, reached on purpose, named (f2g_convnext_last_launch) and compared with ONE float64 restatement of the
block (autograd for every gradient), plus the z prologue of f2g_fused_block against float64.

Each GPU case asserts the kernel instance that ran against a Python restatement of the dispatch rule
(`dw_route`, `dwconv_route`) BEFORE it compares numbers; a CPU ledger test sweeps the rule and holds its set of
names, the names in csrc/convnext.hip and the names claimed by the parametrised cases to one explicit set.

Tolerances (the project's bars, relative to the largest expected magnitude of the compared tensor): forward
and du 2e-5; gx, g_cproj, g_te 1e-4; parameter-gradient sums 2e-4.  On the frames from three before each item's
length to the end of the item the same bars hold per element against the ROW's own largest expected
magnitude, and where the reference is exactly zero the kernel's value must be exactly zero.

Fused block: the float64 chain is the block reference -> z rounded to bf16 -> the MLP restatement of
test_hip_gemm_routes._mlp_operands.  A z element computed in fp32 may round to the neighbouring bf16 value; the
reference's own spread (z rounded from float64 against z rounded from an fp32 evaluation of the same formula, on
the CPU, over the 18 reference cases of this module) measures 8.0e-4 of the output scale in the maximum and
3.2e-5 in the rms (the same formula summed in three other orders stayed within 8.7e-4 / 4.7e-5) -- under half of _fused_close's 2e-3 / 1e-4, which is therefore the GPU bound
(test_fused_block_reference_spread asserts the halves).  One z element that lands on the neighbouring bf16
value re-rounds about a tenth of its row's hidden activations, which is where the maximum comes from.
"""
import functools
import os
import re
import struct

import pytest
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
NAN = float("nan")
SENT = 7.25                                                   # guard sentinel
SENT_BITS = struct.unpack("<i", struct.pack("<f", SENT))[0]
TOL_FWD, TOL_GX, TOL_SUM = 2e-5, 1e-4, 2e-4

# every name f2g_convnext_last_launch can report
REACHABLE = {
    "dwnorm4<bwd=0,fw=4,nch=1>", "dwnorm4<bwd=0,fw=4,nch=2>", "dwnorm4<bwd=0,fw=4,nch=3>",
    "dwnorm4<bwd=1,fw=4,nch=1>", "dwnorm4<bwd=1,fw=4,nch=2>", "dwnorm4<bwd=1,fw=4,nch=3>",
    "dwnorm4<bwd=1,fw=2,nch=3>",
    "dwnorm<bwd=0,fw=2>", "dwnorm<bwd=0,fw=4>", "dwnorm<bwd=1,fw=2>", "dwnorm<bwd=1,fw=4>",
    "dwconv4_bwd", "dwconv_bwd", "biasnorm_fwd", "biasnorm_bwd",
}
COVERED = set()         # the names the parametrised GPU cases below claim (filled while the module is imported)


# ------------------------------------------------------------------ the dispatch rule, restated
def dw_route(bwd, C, K, up, cond, aligned, w_aligned=None):
    """convnext.hip: launch_dwnorm / vec4_ok.  aligned: every tensor the launch touches starts on 16 bytes and
    has a row stride in whole float4s; w_aligned: the taps do (asked for with 7 taps only)."""
    w_aligned = aligned if w_aligned is None else w_aligned
    if bwd:
        four = (cond and up == 4) or (C <= 512 and C % 4 == 0)
    else:
        four = C % 4 == 0
    fw = 4 if four else 2
    if C % 4 == 0 and aligned and (K != 7 or w_aligned):
        return f"dwnorm4<bwd={int(bwd)},fw={fw},nch={(C + 255) // 256}>"
    return f"dwnorm<bwd={int(bwd)},fw={fw}>"


def dwconv_route(C, K, aligned, w_aligned=None):
    """convnext.hip: the vec4 predicate of f2g_dwconv_bwd"""
    w_aligned = aligned if w_aligned is None else w_aligned
    return "dwconv4_bwd" if (K == 7 and C % 4 == 0 and aligned and w_aligned) else "dwconv_bwd"


def block_routes(C, K, up, cond, aligned, w_aligned=None):
    return (dw_route(False, C, K, up, cond, aligned, w_aligned), dw_route(True, C, K, up, cond, aligned, w_aligned),
            dwconv_route(C, K, aligned, w_aligned))


def claim(*names):
    COVERED.update(names)
    return names


def test_convnext_route_ledger():
    """CPU: the rule's names over every (C, K, up, cond, alignment, direction), the names in csrc/convnext.hip,
    the names the GPU cases of this module claim and REACHABLE are one set -- an instance added to the
    dispatcher without a case, or a case naming a dead instance, turns the suite red."""
    swept = {"biasnorm_fwd", "biasnorm_bwd"}
    for C in range(1, 769):
        for K in (1, 3, 5, 7):
            for aligned in (False, True):
                swept.add(dwconv_route(C, K, aligned))
                for up in (1, 2, 4):
                    for cond in (False, True):
                        for bwd in (False, True):
                            swept.add(dw_route(bwd, C, K, up, cond, aligned))
    assert swept == REACHABLE, sorted(swept ^ REACHABLE)
    src = open(os.path.join(ROOT, "flow2gan_amd", "csrc", "convnext.hip")).read()
    lits = set(re.findall(r'"((?:dwnorm4?<[^"<>]*>)|dwconv4?_bwd|biasnorm_(?:fwd|bwd))"', src))
    assert lits == REACHABLE, sorted(lits ^ REACHABLE)
    assert COVERED == REACHABLE, sorted(COVERED ^ REACHABLE)


# ------------------------------------------------------------------ the float64 reference
def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def lens_for(Fr, B):
    """[F, F - 2, 1] and a fourth item that ends 1..3 frames past a frame-group boundary"""
    past = min(Fr, 4 * ((Fr - 1) // 8) + 1 + Fr % 3)
    return [Fr, max(1, Fr - 2), 1, past][:B]


def rows_of(t):
    """(B, C, F) -> (B * F, C), the kernels' layout"""
    return t.detach().permute(0, 2, 1).reshape(-1, t.shape[1]).contiguous()


def block_formula(x, mask, w_dw, b_dw, beta, ls, cproj, up, te):
    """dwconv(x * mask) -> BiasNorm -> + condition (zero beyond Fc * up) -> * (1 + te), in the dtype of its
    arguments; returns (u, rstd, z)"""
    B, C, Fr = x.shape
    u = Fn.conv1d(x * mask, w_dw, b_dw, padding=w_dw.shape[-1] // 2, groups=C)
    s = ((u - beta[None, :, None]) ** 2).mean(1, keepdim=True) ** -0.5 * ls.exp()
    v = u * s
    if cproj is not None:
        n = min(Fr, cproj.shape[2] * up)
        v = v + Fn.pad(torch.repeat_interleave(cproj, up, dim=2)[:, :, :n], (0, Fr - n))
    if te is not None:
        v = v * (1 + te[:, :, None])
    return u, s, v


@functools.lru_cache(maxsize=None)
def block_ref(C, Fr, up, K, cond=True, te=True, bdw=True, use_lens=True, fc_short=False, B=4, grads=True):
    """Inputs (fp32, CPU) and the float64 results of one case; computed once, shared, never modified."""
    seed = 1000 * C + 10 * Fr + up + K
    Fc = (Fr + up - 1) // up - (1 if fc_short else 0)
    R = dict(C=C, F=Fr, up=up, K=K, B=B, Fc=Fc)
    R["x"] = rnd(B, C, Fr, seed=seed + 1)
    R["lens"] = torch.tensor(lens_for(Fr, B)) if use_lens else None
    R["w_dw"] = rnd(C, 1, K, seed=seed + 2, scale=0.3)
    R["b_dw"] = rnd(C, seed=seed + 3, scale=0.1) if bdw else None
    R["beta"] = rnd(C, seed=seed + 4, scale=0.1)
    R["ls"] = torch.tensor([0.7])
    R["cproj"] = rnd(B, C, max(Fc, 1), seed=seed + 5)[:, :, :Fc] if cond else None
    R["te"] = rnd(B, C, seed=seed + 6, scale=0.3) if te else None
    R["gz"] = rnd(B, C, Fr, seed=seed + 7)
    R["gres"] = rnd(B * Fr, C, seed=seed + 8)
    R["gam"] = rnd(C, seed=seed + 9)
    ln = R["lens"] if use_lens else torch.full((B,), Fr)
    R["len_list"] = ln.tolist()
    mask = (torch.arange(Fr)[None] < ln[:, None]).double()[:, None]
    leaf = {k: (R[k].double().requires_grad_(grads) if R[k] is not None else None)
            for k in ("x", "w_dw", "b_dw", "beta", "ls", "cproj", "te")}
    u, s, z = block_formula(leaf["x"], mask, leaf["w_dw"], leaf["b_dw"], leaf["beta"], leaf["ls"][0], leaf["cproj"], up,
                            leaf["te"])
    R["z"] = rows_of(z)
    R["rstd"] = s.detach()[:, 0, :].reshape(-1)
    if grads:
        u.retain_grad()
        z.backward(R["gz"].double())
        R["du"] = rows_of(u.grad)
        R["gx_conv"] = rows_of(leaf["x"].grad)
        R["g_w"], R["g_beta"], R["g_ls"] = leaf["w_dw"].grad, leaf["beta"].grad, leaf["ls"].grad
        R["g_b"] = leaf["b_dw"].grad if bdw else u.grad.sum((0, 2))
        R["g_cproj"] = rows_of(leaf["cproj"].grad) if cond else None
        R["g_te"] = leaf["te"].grad if te else None
        R["g_gamma"] = (R["gres"].double() * rows_of(R["x"]).double()).sum(0)
    return R


# ------------------------------------------------------------------ device plumbing and checks
@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from flow2gan_amd import ops as o
    return o


def last(ops):
    return ops.L.lib.f2g_convnext_last_launch().decode()


def dev(t):
    return None if t is None else t.detach().float().to(DEV).contiguous()


def put(t, pad):
    """an input matrix inside a sentinel buffer `pad` columns wider (pad 0: contiguous)"""
    rows, C = t.shape
    buf = torch.full((rows, C + pad), SENT, device=DEV)
    buf[:, :C] = t.float().to(DEV)
    return buf[:, :C], buf


def out(rows, C, pad, dtype=torch.float32):
    """an output matrix, NaN where it must be written, inside a sentinel buffer `pad` columns wider"""
    buf = torch.full((rows, C + pad), SENT, device=DEV, dtype=dtype)
    buf[:, :C] = NAN
    return buf[:, :C], buf


def guards_intact(buf, C):
    return bool((buf[:, C:].contiguous().view(torch.int32) == SENT_BITS).all())


def stack(t, C, rows, fill):
    """(rows, C) placed at columns [C // 2, C // 2 + C) of a (rows, 2 C) buffer: the stacked condition / time
    buffers of the model, read and written at an offset"""
    buf = fill.clone().to(DEV) if torch.is_tensor(fill) else torch.full((rows, 2 * C), fill, device=DEV)
    if t is not None:
        buf[:, C // 2: C // 2 + C] = t.float().to(DEV)
    return buf


def close(got, want, tol, name):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert torch.isfinite(got).all(), name
    scale = want.abs().max().item() + 1e-30
    err = (got - want).abs().max().item()
    assert err <= tol * scale, f"{name}: max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.2e} > {tol:.0e})"


def close_rows(got, want, rows, tol, name):
    """per element against the scale of its own row; exact zero where the reference is exactly zero"""
    g, w = got.detach().cpu().double()[rows], want.detach().cpu().double()[rows]
    scale = w.abs().amax(1, keepdim=True)
    bad = (g - w).abs() > tol * scale
    assert not bad.any(), f"{name}: {int(bad.sum())} elements of the edge rows off by more than {tol:.0e} of their row"
    assert bool((g[w == 0] == 0).all()), f"{name}: non-zero where the reference is exactly zero"


def edge_rows(R):
    """the frames from 3 before each item's length (the taps reach the mask) to the item's end"""
    idx = [b * R["F"] + f for b, n in enumerate(R["len_list"]) for f in range(max(0, n - 3), R["F"])]
    return torch.tensor(idx, dtype=torch.long)


def run_block(ops, R, *, layout="plain", w_off=False, partials=True, drop=(), check_rstd=False):
    """forward, dwnorm_bwd and dwconv_bwd of one reference case on the same tensors.
    layout: plain (contiguous), wide (every matrix inside a wider sentinel buffer: + 8 columns where C % 4 == 0,
    + 3 otherwise), x_off1 (x a view one float into its buffer), x_ld50 (x with row stride C + 2).
    w_off: the taps one float into their buffer.  drop: optional outputs / inputs left out (g_cproj, g_te,
    g_beta, g_ls, gres).  Accumulated outputs start from non-zero contents and must come back as old + gradient."""
    C, Fr, up, K, B, Fc = (R[k] for k in ("C", "F", "up", "K", "B", "Fc"))
    rows, cond, has_te = B * Fr, R["cproj"] is not None, R["te"] is not None
    pad = 0 if layout != "wide" else (8 if C % 4 == 0 else 3)
    aligned = layout in ("plain", "wide") and pad % 4 == 0
    want_fwd, want_bwd, want_conv = block_routes(C, K, up, cond, aligned, aligned and not w_off)
    edges = edge_rows(R)

    if layout == "x_off1":
        xbuf = torch.full((rows * C + 1,), SENT, device=DEV)
        x = xbuf[1:].view(rows, C)
        x.copy_(rows_of(R["x"]))
    elif layout == "x_ld50":
        x, xbuf = put(rows_of(R["x"]), 2)
    else:
        x, xbuf = put(rows_of(R["x"]), pad)
    if w_off:
        wbuf = torch.full((C * K + 1,), SENT, device=DEV)
        w_dw = wbuf[1:].view(C, 1, K)
        w_dw.copy_(R["w_dw"])
    else:
        w_dw = dev(R["w_dw"])
    lens = None if R["lens"] is None else R["lens"].int().to(DEV)
    args = (B, Fr, C, K, lens, w_dw, dev(R["b_dw"]), dev(R["beta"]), dev(R["ls"]))
    cp_all = stack(rows_of(R["cproj"]), C, B * Fc, SENT) if cond else None
    te_all = stack(R["te"], C, B, SENT) if has_te else None
    cpa = (cp_all, 2 * C if cond else 0, Fc if cond else 0, up, C // 2 if cond else 0, te_all, 2 * C if has_te else 0,
           C // 2 if has_te else 0)

    # ---- forward
    z, zbuf = out(rows, C, pad)
    rstd = torch.full((rows + 8,), SENT, device=DEV) if check_rstd else None
    ops.dwnorm_fwd(x, z, *args, *cpa, rstd=rstd)
    assert last(ops) == want_fwd, (last(ops), want_fwd)
    close(z, R["z"], TOL_FWD, "z")
    close_rows(z, R["z"], edges, TOL_FWD, "z")
    assert guards_intact(zbuf, C)
    if check_rstd:
        got, want = rstd[:rows].cpu().double(), R["rstd"]
        assert bool(((got - want).abs() <= TOL_FWD * want.abs()).all()), "rstd"
        assert bool((rstd[rows:] == SENT).all())

    # ---- dwnorm backward
    gz, gzbuf = put(rows_of(R["gz"]), pad)
    du, dubuf = out(rows, C, pad)
    old = {"g_cp": rnd(max(B * Fc, 1), 2 * C, seed=31, scale=0.25)[:B * Fc], "g_te": rnd(B, 2 * C, seed=32, scale=0.25),
           "g_beta": rnd(C, seed=33, scale=0.25), "g_ls": rnd(1, seed=34, scale=0.25)}
    g_cp = old["g_cp"].to(DEV) if cond and "g_cproj" not in drop else None
    g_te = old["g_te"].to(DEV) if has_te and "g_te" not in drop else None
    g_beta = old["g_beta"].to(DEV) if "g_beta" not in drop else None
    g_ls = old["g_ls"].to(DEV) if "g_ls" not in drop else None
    ops.dwnorm_bwd(x, gz, du, *args, *cpa, g_cproj=g_cp, g_te=g_te, g_beta=g_beta, g_log_scale=g_ls,
                   partials=partials)
    assert last(ops) == want_bwd, (last(ops), want_bwd)
    close(du, R["du"], TOL_FWD, "du")
    close_rows(du, R["du"], edges, TOL_FWD, "du")
    assert guards_intact(dubuf, C) and guards_intact(gzbuf, C)
    sl = slice(C // 2, C // 2 + C)
    if g_cp is not None:
        close(g_cp[:, sl], old["g_cp"][:, sl].double() + R["g_cproj"], TOL_GX, "g_cproj (accumulated)")
        keep = torch.ones(2 * C, dtype=torch.bool)
        keep[sl] = False
        assert torch.equal(g_cp.cpu()[:, keep], old["g_cp"][:, keep]), "g_cproj: columns of other blocks changed"
        # store mode against accumulate mode, both onto zeros: the same sums; a second store-mode call does
        # not double them
        acc0 = torch.zeros(B * Fc, 2 * C, device=DEV)
        ops.dwnorm_bwd(x, gz, torch.empty_like(du), *args, *cpa, g_cproj=acc0, partials=partials)
        st = torch.zeros(B * Fc, 2 * C, device=DEV)
        for _ in range(2):
            ops.dwnorm_bwd(x, gz, torch.empty_like(du), *args, *cpa, g_cproj=st, g_cproj_store=True, partials=partials)
        assert last(ops) == want_bwd
        close(st[:, sl], R["g_cproj"], TOL_GX, "g_cproj (stored)")
        close(st, acc0, 1e-6, "g_cproj store mode against accumulate mode")
    if g_te is not None:
        close(g_te[:, sl], old["g_te"][:, sl].double() + R["g_te"], TOL_GX, "g_te")
        keep = torch.ones(2 * C, dtype=torch.bool)
        keep[sl] = False
        assert torch.equal(g_te.cpu()[:, keep], old["g_te"][:, keep]), "g_te: columns of other blocks changed"
    if g_beta is not None:
        close(g_beta, old["g_beta"].double() + R["g_beta"], TOL_SUM, "g_beta")
    if g_ls is not None:
        close(g_ls, old["g_ls"].double() + R["g_ls"], TOL_SUM, "g_log_scale")

    # ---- depthwise conv backward (on the kernel's own du)
    with_res = "gres" not in drop
    gx, gxbuf = out(rows, C, pad)
    gres, gresbuf = put(R["gres"], pad) if with_res else (None, None)
    oldc = {"g_w": rnd(C, 1, K, seed=35, scale=0.25), "g_b": rnd(C, seed=36, scale=0.25), "g_gam": rnd(C, seed=37, scale=0.25)}
    g_w, g_b = oldc["g_w"].to(DEV), oldc["g_b"].to(DEV)
    g_gam = oldc["g_gam"].to(DEV) if with_res else None
    ops.dwconv_bwd(du, x, gx, B, Fr, C, K, lens, w_dw, gres=gres, gamma=dev(R["gam"]) if with_res else None,
                   g_w=g_w, g_b=g_b, g_gamma=g_gam, partials=partials)
    assert last(ops) == want_conv, (last(ops), want_conv)
    want_gx = R["gx_conv"] + (R["gam"].double()[None] * R["gres"].double() if with_res else 0.0)
    close(gx, want_gx, TOL_GX, "gx")
    close_rows(gx, want_gx, edges, TOL_GX, "gx")
    assert guards_intact(gxbuf, C) and (gresbuf is None or guards_intact(gresbuf, C))
    assert bool((xbuf[:1] == SENT).all()) if layout == "x_off1" else guards_intact(xbuf, C)
    close(g_w, oldc["g_w"].double() + R["g_w"], TOL_SUM, "g_w_dw")
    close(g_b, oldc["g_b"].double() + R["g_b"], TOL_SUM, "g_b_dw")
    if with_res:
        close(g_gam, oldc["g_gam"].double() + R["g_gamma"], TOL_SUM, "g_gamma")


# ------------------------------------------------------------------ dwnorm forward + backward, dwconv backward
def block_case(C, Fr, up, K, layout="plain", w_off=False, fc_short=False, **kw):
    """a pytest.param whose id names the case; claims the three routes it must take"""
    pad_ok = layout in ("plain", "wide") and (layout == "plain" or C % 4 == 0)
    names = claim(*block_routes(C, K, up, True, pad_ok, pad_ok and not w_off))
    tag = f"C{C}-F{Fr}-up{up}-K{K}-{layout}" + ("-woff" if w_off else "") + ("-fcshort" if fc_short else "")
    return pytest.param(C, Fr, up, K, layout, w_off, fc_short, names, id=tag)


BLOCK_CASES = [
    block_case(48, 21, 2, 7),                     # nch 1; F no multiple of FW or up; idle waves in the last block
    block_case(384, 23, 4, 7, fc_short=True),     # nch 2; Fc one row short of ceil(F / up)
    block_case(512, 9, 1, 7),                     # nch 2; the largest C on the backward FW = 4
    block_case(768, 11, 1, 7),                    # backward FW = 2, nch 3
    block_case(768, 11, 2, 7),
    block_case(768, 11, 4, 7),                    # backward FW = 4, nch 3
    block_case(520, 7, 1, 7),                     # third chunk partly filled; dwconv4: 3 channel blocks, the last partial
    block_case(50, 21, 1, 7),                     # scalar FW = 2 both ways
    block_case(50, 21, 2, 7),
    block_case(50, 21, 4, 7),                     # scalar FW = 4 backward
    block_case(766, 5, 1, 7),                     # scalar, 12 chunks per lane, the last partial
    block_case(48, 21, 2, 7, layout="x_off1"),    # scalar because of alignment alone
    block_case(48, 21, 2, 7, layout="x_ld50"),
    block_case(48, 21, 1, 1, w_off=True), block_case(48, 21, 1, 3, w_off=True), block_case(48, 21, 1, 5, w_off=True),
    block_case(48, 21, 1, 1, layout="x_off1"), block_case(48, 21, 1, 3, layout="x_off1"),
    block_case(48, 21, 1, 5, layout="x_off1"),
    block_case(48, 1, 1, 7), block_case(48, 3, 1, 7),   # F below one frame group
    block_case(48, 21, 2, 7, layout="wide"),      # every operand inside a wider sentinel buffer: vector route ...
    block_case(50, 21, 2, 7, layout="wide"),      # ... and scalar route
    # dwconv_bwd frame edges: 16-frame strips, 4 per block (vector); 32-frame strips (scalar, K = 5)
    *[block_case(48, f, 1, 7) for f in (15, 16, 17, 63, 64, 65)],
    *[block_case(48, f, 1, 5) for f in (31, 32, 33)],
]


@pytest.mark.gpu
@pytest.mark.parametrize("C,Fr,up,K,layout,w_off,fc_short,names", BLOCK_CASES)
def test_dwnorm_dwconv_routes(ops, C, Fr, up, K, layout, w_off, fc_short, names):
    run_block(ops, block_ref(C, Fr, up, K, fc_short=fc_short), layout=layout, w_off=w_off)


OPTIONAL = [   # reference variant, what the launch leaves out
    (dict(cond=False), ()), (dict(te=False), ()), (dict(bdw=False), ()), (dict(use_lens=False), ()),
    (dict(), ("g_cproj",)), (dict(), ("g_te",)), (dict(), ("gres",)), (dict(), ("g_beta", "g_ls")),
    (dict(cond=False, te=False, bdw=False), ("gres",)),
]
OPTIONAL_IDS = ["no-cproj", "no-te", "no-b_dw", "no-lens", "no-g_cproj", "no-g_te", "no-gres-gamma-g_gamma",
                "no-g_beta-g_log_scale", "bare"]


@pytest.mark.gpu
@pytest.mark.parametrize("C", [claim(*block_routes(48, 7, 2, True, True), *block_routes(48, 7, 2, False, True)) and 48,
                               claim(*block_routes(50, 7, 2, True, True), *block_routes(50, 7, 2, False, True)) and 50])
@pytest.mark.parametrize("variant,drop", OPTIONAL, ids=OPTIONAL_IDS)
def test_dwnorm_dwconv_optional_inputs(ops, C, variant, drop):
    """absent optional inputs and outputs against float64 (without b_dw, cond and gres the masked frames of z
    and gx are exactly zero); every accumulated output starts from non-zero contents"""
    run_block(ops, block_ref(C, 21, 2, 7, **variant), drop=drop)


@pytest.mark.gpu
@pytest.mark.parametrize("C,Fr,up", [
    claim(*block_routes(48, 7, 2, True, True)) and (48, 21, 2), claim(*block_routes(768, 7, 1, True, True)) and (768, 11, 1),
    claim(*block_routes(50, 7, 2, True, True)) and (50, 21, 2), claim(*block_routes(50, 7, 4, True, True)) and (50, 21, 4)])
def test_atomic_epilogues(ops, C, Fr, up):
    """partials = NULL: the four backward kernels add their parameter gradients atomically -- the same
    expectations as with the workspace"""
    run_block(ops, block_ref(C, Fr, up, 7), partials=False)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [48, 384, 50])
def test_rstd_output(ops, C):
    """the forward kernels' per-row normaliser exp(log_scale) / sqrt(mean_c((u - beta)^2)), with lens"""
    run_block(ops, block_ref(C, 21, 2, 7), check_rstd=True)


# ------------------------------------------------------------------ operand formats of z
@pytest.mark.gpu
@pytest.mark.parametrize("C,Fr,up", [(48, 21, 2), (384, 23, 4), (768, 11, 1)])
@pytest.mark.parametrize("fmt", [1, 2])
def test_z_operand_formats(ops, C, Fr, up, fmt):
    """z_format 1 / 2 with lens, cond and te: bitwise the split-bf16 image / the bf16 rounding of the fp32
    kernel's own z; format 2 also against float64 to half a bf16 step plus the fp32 forward bound"""
    R = block_ref(C, Fr, up, 7, fc_short=(C == 384))
    B, Fc, rows = R["B"], R["Fc"], R["B"] * Fr
    x = dev(rows_of(R["x"]))
    args = (B, Fr, C, 7, R["lens"].int().to(DEV), dev(R["w_dw"]), dev(R["b_dw"]), dev(R["beta"]), dev(R["ls"]))
    cpa = (stack(rows_of(R["cproj"]), C, B * Fc, SENT), 2 * C, Fc, up, C // 2, stack(R["te"], C, B, SENT), 2 * C, C // 2)
    z = torch.full((rows, C), NAN, device=DEV)
    ops.dwnorm_fwd(x, z, *args, *cpa)
    name = dw_route(False, C, 7, up, True, True)
    assert last(ops) == name
    close(z, R["z"], TOL_FWD, "z")
    if fmt == 1:
        zi = torch.full((rows, C), NAN, device=DEV)
        ops.dwnorm_fwd(x, zi, *args, *cpa, z_format=1)
        assert last(ops) == name
        assert torch.equal(zi.view(torch.int32), ops.split_bf16(z).view(torch.int32))
    else:
        zb, zbuf = out(rows, C, 8, dtype=torch.bfloat16)
        ops.dwnorm_fwd(x, zb, *args, *cpa, z_format=2)
        assert last(ops) == name
        assert torch.equal(zb, z.bfloat16())
        assert bool((zbuf[:, C:].float() == SENT).all())
        want = R["z"]
        err = (zb.cpu().double() - want).abs()
        assert bool((err <= 2.0 ** -8 * want.abs() + TOL_FWD * want.abs().max()).all()), float(err.max())


@pytest.mark.gpu
@pytest.mark.parametrize("C,fmt,ldz", [(50, 1, 50), (50, 2, 56), (48, 2, 52)])
def test_z_operand_formats_refused(ops, C, fmt, ldz):
    """formats 1 / 2 exist on the vector kernel only: C % 4 != 0, or a bf16 row stride that is no multiple of 8
    elements, is refused with F2G_EINVAL before anything is launched"""
    R = block_ref(C, 21, 2, 7)
    B, rows = R["B"], R["B"] * 21
    zbuf = torch.full((rows, ldz), SENT, device=DEV, dtype=torch.bfloat16 if fmt == 2 else torch.float32)
    with pytest.raises(ops.L.F2GError, match="code -1"):
        ops.dwnorm_fwd(dev(rows_of(R["x"])), zbuf[:, :C], B, 21, C, 7, R["lens"].int().to(DEV), dev(R["w_dw"]),
                       dev(R["b_dw"]), dev(R["beta"]), dev(R["ls"]), z_format=fmt)
    torch.cuda.synchronize()
    assert bool((zbuf.float() == SENT).all())


# ------------------------------------------------------------------ BiasNorm
BN_C = [1, 24, 50, 64, 65, 766, 768]
BN_ROWS = [1, 3, 4, 5, 31, 32, 33]     # forward: 4 rows per block; backward: 4 waves x 8 rows per block
BN_CASES = [(BN_C[i], BN_ROWS[i], 0) for i in range(7)] + [(BN_C[i], BN_ROWS[(i + 3) % 7], 0) for i in range(7)] + \
           [(50, 33, 5), (768, 5, 8)]
claim("biasnorm_fwd", "biasnorm_bwd")


@functools.lru_cache(maxsize=None)
def biasnorm_ref(C, rows):
    x = rnd(rows, C, seed=7 * C + rows)
    beta, ls, gy = rnd(C, seed=C + 1, scale=0.1), torch.tensor([1.2]), rnd(rows, C, seed=C + rows + 2)
    xd, bd, ld = x.double().requires_grad_(), beta.double().requires_grad_(), ls.double().requires_grad_()
    s = ((xd - bd) ** 2).mean(1, keepdim=True) ** -0.5 * ld[0].exp()
    y = xd * s
    y.backward(gy.double())
    return dict(x=x, beta=beta, ls=ls, gy=gy, y=y.detach(), gx=xd.grad, g_beta=bd.grad, g_ls=ld.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("C,rows,pad", BN_CASES)
def test_biasnorm_routes(ops, C, rows, pad):
    """both BiasNorm kernels at the edges of their row split and channel loop; pad > 0: all three matrices of
    each kernel inside wider sentinel buffers; g_beta / g_log_scale accumulate from non-zero contents and
    either may be absent"""
    R = biasnorm_ref(C, rows)
    x, xbuf = put(R["x"], pad)
    y, ybuf = out(rows, C, pad)
    beta, ls = dev(R["beta"]), dev(R["ls"])
    ops.biasnorm_fwd(x, y, rows, C, beta, ls)
    assert last(ops) == "biasnorm_fwd"
    close(y, R["y"], TOL_FWD, "biasnorm y")
    assert guards_intact(ybuf, C)
    gy, gybuf = put(R["gy"], pad)
    gx, gxbuf = out(rows, C, pad)
    old_b, old_l = rnd(C, seed=41, scale=0.25), rnd(1, seed=42, scale=0.25)
    gb, gl = old_b.to(DEV), old_l.to(DEV)
    ops.biasnorm_bwd(x, gy, gx, rows, C, beta, ls, gb, gl)
    assert last(ops) == "biasnorm_bwd"
    close(gx, R["gx"], TOL_GX, "biasnorm gx")
    close(gb, old_b.double() + R["g_beta"], TOL_SUM, "biasnorm g_beta")
    close(gl, old_l.double() + R["g_ls"], TOL_SUM, "biasnorm g_log_scale")
    assert guards_intact(gxbuf, C) and guards_intact(xbuf, C) and guards_intact(gybuf, C)
    for drop in ("beta", "ls"):
        gx2 = torch.full((rows, C), NAN, device=DEV)
        gb2 = None if drop == "beta" else old_b.to(DEV)
        gl2 = None if drop == "ls" else old_l.to(DEV)
        ops.biasnorm_bwd(x, gy, gx2, rows, C, beta, ls, gb2, gl2)
        close(gx2, R["gx"], TOL_GX, f"biasnorm gx without g_{drop}")
        if gb2 is not None:
            close(gb2, old_b.double() + R["g_beta"], TOL_SUM, "biasnorm g_beta without g_log_scale")
        if gl2 is not None:
            close(gl2, old_l.double() + R["g_ls"], TOL_SUM, "biasnorm g_log_scale without g_beta")


@pytest.mark.gpu
def test_biasnorm_forward_above_768_channels(ops):
    """biasnorm_fwd_kernel loops over the channels (no per-lane register array), so the forward has no channel
    limit; the backward keeps C / 64 values per lane and refuses C > 768"""
    C, rows = 800, 5
    R = biasnorm_ref(C, rows)
    y, ybuf = out(rows, C, 4)
    ops.biasnorm_fwd(dev(R["x"]), y, rows, C, dev(R["beta"]), dev(R["ls"]))
    assert last(ops) == "biasnorm_fwd"
    close(y, R["y"], TOL_FWD, "biasnorm y")
    assert guards_intact(ybuf, C)
    gx = torch.full((rows, C), SENT, device=DEV)
    with pytest.raises(ops.L.F2GError, match="code -1"):
        ops.biasnorm_bwd(dev(R["x"]), dev(R["gy"]), gx, rows, C, dev(R["beta"]), dev(R["ls"]), None, None)
    torch.cuda.synchronize()
    assert bool((gx == SENT).all())


# ------------------------------------------------------------------ the fused block against float64
FUSED_RT = {384: (1, 2, 4), 512: (1, 2, 3), 768: (1, 2)}
FUSED_F, FUSED_B = 23, 3


@functools.lru_cache(maxsize=None)
def fused_weights(C):
    H = 3 * C
    gen = torch.Generator().manual_seed(C)
    return dict(H=H, w1=torch.randn(H, C, generator=gen) * 0.05, w2=torch.randn(C, H, generator=gen) * 0.03,
                b1=torch.randn(H, generator=gen) * 0.1, al=0.25 + 0.2 * torch.randn(H, generator=gen),
                b2=torch.randn(C, generator=gen) * 0.1, gam=0.5 + torch.rand(C, generator=gen))


def mlp_ref(z_bf16, x_rows, W):
    """test_hip_gemm_routes._mlp_operands: bf16 operands, float64 sums, the hidden activation rounded to bf16"""
    a = z_bf16.double() @ W["w1"].to(torch.bfloat16).double().t() + W["b1"].double()
    p = (a.clamp(min=0) + W["al"].double() * a.clamp(max=0)).float().to(torch.bfloat16)
    return p.double() @ W["w2"].to(torch.bfloat16).double().t() + W["b2"].double() + W["gam"].double() * x_rows.double()


@functools.lru_cache(maxsize=None)
def fused_ref(C, up, cond):
    """(case, float64 output with z rounded from float64, the same with z rounded from an fp32 evaluation)"""
    R = block_ref(C, FUSED_F, up, 7, cond=cond, te=cond, fc_short=True, B=FUSED_B, grads=False)
    W = fused_weights(C)
    x_rows = rows_of(R["x"])
    want = mlp_ref(R["z"].to(torch.bfloat16), x_rows, W)
    mask = (torch.arange(FUSED_F)[None] < R["lens"][:, None]).float()[:, None]
    z32 = block_formula(R["x"], mask, R["w_dw"], R["b_dw"], R["beta"], R["ls"][0], R["cproj"], up, R["te"])[2]
    return R, want, mlp_ref(rows_of(z32).to(torch.bfloat16), x_rows, W)


FUSED_CASES = [(C, up, cond) for C in (384, 512, 768) for up in (4, 2, 1) for cond in (True, False)]


def test_fused_block_reference_spread():
    """CPU: how far the float64 chain moves when z is rounded to bf16 from an fp32 evaluation instead of from
    float64 -- the reference's own spread must stay under half of the GPU bound (2e-3 max, 1e-4 rms)"""
    worst_max = worst_rms = 0.0
    for C, up, cond in FUSED_CASES:
        _, want, want32 = fused_ref(C, up, cond)
        scale = float(want.abs().max())
        worst_max = max(worst_max, float((want32 - want).abs().max()) / scale)
        worst_rms = max(worst_rms, float((want32 - want).pow(2).mean().sqrt()) / scale)
    print(f"fused block reference spread: max {worst_max:.3e}, rms {worst_rms:.3e} of the output scale")
    assert worst_max <= 1e-3 and worst_rms <= 5e-5, (worst_max, worst_rms)


@pytest.mark.gpu
@pytest.mark.parametrize("C,up,cond", FUSED_CASES)
def test_fused_block_against_float64(ops, C, up, cond, lib_option):
    """f2g_fused_block directly against float64 (not against dwnorm_fwd + fused_mlp): 3 items of 23 frames = 69
    rows (tiles straddle item boundaries), ragged lengths, the condition one row short, every tile height the
    channel count allows (option mlp_rt, asserted through f2g_fused_last_launch)"""
    R, want, _ = fused_ref(C, up, cond)
    W = fused_weights(C)
    B, Fr, Fc, rows, H = R["B"], R["F"], R["Fc"], R["B"] * R["F"], W["H"]
    x = dev(rows_of(R["x"]))
    wp = ops.mlp_pack(W["w1"].to(DEV), W["w2"].to(DEV))
    args = (B, Fr, C, 7, R["lens"].int().to(DEV), dev(R["w_dw"]), dev(R["b_dw"]), dev(R["beta"]), dev(R["ls"]))
    cpa = ((stack(rows_of(R["cproj"]), C, B * Fc, SENT), 2 * C, Fc, up, C // 2, stack(R["te"], C, B, SENT), 2 * C, C // 2)
           if cond else (None, 0, 0, 1, 0, None, 0, 0))
    scale = float(want.abs().max())
    for rt in FUSED_RT[C]:
        lib_option("mlp_rt", rt)
        got, gbuf = out(rows, C, 4)
        ops.fused_block(x, *args, wp, dev(W["b1"]), dev(W["al"]), dev(W["b2"]), dev(W["gam"]), got, H, *cpa)
        torch.cuda.synchronize()
        assert ops.L.lib.f2g_fused_last_launch().decode() == f"fused_block<rt={rt},parts=1>"
        assert torch.isfinite(got).all(), rt
        err = got.cpu().double() - want
        print(f"C={C} up={up} cond={cond} rt={rt}: max {float(err.abs().max()) / scale:.3e} "
              f"rms {float(err.pow(2).mean().sqrt()) / scale:.3e}")
        assert float(err.abs().max()) < 2e-3 * scale, (rt, float(err.abs().max()), scale)
        assert float(err.pow(2).mean().sqrt()) < 1e-4 * scale, (rt, float(err.pow(2).mean().sqrt()), scale)
        assert guards_intact(gbuf, C)
