"""f2g_dwblock_bwd on the GPU: the BiasNorm backward and the depthwise-conv backward of a ConvNeXt block in one
launch (csrc/convnext.hip: blockbwd_kernel) against the float64 restatement of the block in
tests/test_hip_convnext_routes.py (block_ref: autograd for every gradient), with that module's bars: gx, g_cproj and
g_te within 1e-4 of the tensor's largest expected magnitude, the parameter-gradient sums within 2e-4, the per-row
bars from three frames before each item's length to its end, and exact zeros where float64 is exactly zero.

T = 16 frames is the kernel's tile; a block walks several tiles only when the launch has more than 768 of them, so one
case per chunk count uses a long item (F = 6150 at B = 4: two tiles per block, the last block one tile short)."""
import functools
import random

import numpy as np
import pytest
import torch

from test_hip_convnext_routes import (DEV, NAN, SENT, TOL_GX, TOL_SUM, block_formula, block_ref, close, close_rows,
                                      dev, edge_rows, guards_intact, lens_for, out, put, rnd, rows_of)

T = 16
SUMS = ("g_w", "g_b", "g_gamma", "g_beta", "g_ls")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from flow2gan_amd import ops as o
    assert o.DWBLOCK_T == T
    return o


def last(ops):
    return ops.L.lib.f2g_convnext_last_launch().decode()


def off_of(C):
    """column offset of a block inside the stacked condition / time buffers: about C / 2, in whole float4s"""
    return (C // 2) // 4 * 4


def stack(t, C, rows, fill):
    """(rows, C) at columns [off_of(C), off_of(C) + C) of a (rows, 2 C) buffer: the stacked condition / time tensors
    of the model, read and written at an offset"""
    buf = torch.full((rows, 2 * C), fill, device=DEV)
    buf[:, off_of(C): off_of(C) + C] = t.float().to(DEV)
    return buf


def guarded(values, fill):
    """a flat parameter-gradient buffer with 8 sentinel floats behind it"""
    n = values.numel()
    buf = torch.full((n + 8,), SENT, device=DEV)
    buf[:n] = values.flatten().to(DEV) if fill is None else fill
    return buf[:n].view(values.shape), buf


def launch(ops, R, *, pad=8, store=False, with_res=True, fill=None, x=None, gz=None, gres=None, own_ws=False):
    """one f2g_dwblock_bwd launch on the tensors of a reference case: every matrix inside a sentinel buffer `pad`
    columns wider, outputs NaN where they must be written, the condition / time tensors at a column offset inside
    buffers twice as wide (as the model stacks them), every parameter gradient followed by sentinels.  Accumulated
    outputs start from random contents (fill None) or from `fill`.  Asserts the instance that ran, that no NaN is
    left and that no sentinel moved; returns the outputs and what they started from."""
    C, Fr, up, B, Fc = (R[k] for k in ("C", "F", "up", "B", "Fc"))
    rows, cond, has_te = B * Fr, R["cproj"] is not None, R["te"] is not None
    xv, xbuf = put(rows_of(R["x"]) if x is None else x, pad)
    gzv, gzbuf = put(rows_of(R["gz"]) if gz is None else gz, pad)
    grv, grbuf = put(R["gres"] if gres is None else gres, pad) if with_res else (None, None)
    gx, gxbuf = out(rows, C, pad)
    lens = None if R["lens"] is None else R["lens"].int().to(DEV)
    cp_all = stack(rows_of(R["cproj"]), C, B * Fc, SENT) if cond else None
    te_all = stack(R["te"], C, B, SENT) if has_te else None
    sl = slice(off_of(C), off_of(C) + C)
    old = {"g_cproj": rnd(max(B * Fc, 1), 2 * C, seed=31, scale=0.25)[:B * Fc], "g_te": rnd(B, 2 * C, seed=32, scale=0.25),
           "g_beta": rnd(C, seed=33, scale=0.25), "g_ls": rnd(1, seed=34, scale=0.25),
           "g_w": rnd(C, 1, 7, seed=35, scale=0.25), "g_b": rnd(C, seed=36, scale=0.25), "g_gamma": rnd(C, seed=37, scale=0.25)}
    if fill is not None:
        old = {k: torch.full_like(v, fill) for k, v in old.items()}
    g_cp = old["g_cproj"].clone().to(DEV) if cond else None
    if cond and store:
        g_cp[:, sl] = NAN                     # stored, not accumulated: every element must be written
    g_te = old["g_te"].clone().to(DEV) if has_te else None
    G, bufs = {}, {}
    for k in SUMS:
        G[k], bufs[k] = guarded(old[k], None)
    if not with_res:
        G["g_gamma"] = None
    ws = wsn = None
    if own_ws:
        wsn = ops.L.lib.f2g_dwblock_bwd_workspace(B, Fr, C)
        ws = torch.full((wsn + 64,), SENT, device=DEV)
        ws[:wsn] = NAN
    ops.dwblock_bwd(xv, gzv, gx, B, Fr, C, 7, lens, dev(R["w_dw"]), dev(R["b_dw"]), dev(R["beta"]), dev(R["ls"]),
                    cp_all, 2 * C if cond else 0, Fc if cond else 0, up, off_of(C) if cond else 0, te_all,
                    2 * C if has_te else 0, off_of(C) if has_te else 0, g_cproj=g_cp, g_te=g_te, g_beta=G["g_beta"],
                    g_log_scale=G["g_ls"], g_cproj_store=store, gres=grv, gamma=dev(R["gam"]) if with_res else None,
                    g_w=G["g_w"], g_b=G["g_b"], g_gamma=G["g_gamma"], workspace=ws)
    torch.cuda.synchronize()
    assert last(ops) == f"blockbwd<nch={(C + 255) // 256}>", last(ops)
    assert guards_intact(gxbuf, C) and guards_intact(xbuf, C) and guards_intact(gzbuf, C)
    assert grbuf is None or guards_intact(grbuf, C)
    assert not bool(torch.isnan(gx).any()), "gx: NaN left"
    keep = torch.ones(2 * C, dtype=torch.bool)
    keep[sl] = False
    if cond:
        assert not bool(torch.isnan(g_cp).any()), "g_cproj: NaN left"
        assert torch.equal(g_cp.cpu()[:, keep], old["g_cproj"][:, keep]), "g_cproj: columns of other blocks changed"
        assert bool((cp_all.cpu()[:, keep] == SENT).all())
    if has_te:
        assert torch.equal(g_te.cpu()[:, keep], old["g_te"][:, keep]), "g_te: columns of other blocks changed"
    for k in SUMS:
        assert bool((bufs[k][-8:] == SENT).all()), f"{k}: sentinel changed"
    if own_ws:
        assert not bool(torch.isnan(ws[:wsn]).any()), "workspace: a partial row was not written"
        assert bool((ws[wsn:] == SENT).all()), "workspace tail changed"
    G.update(gx=gx, g_cproj=None if g_cp is None else g_cp[:, sl], g_te=None if g_te is None else g_te[:, sl])
    G["old"] = {k: (v[:, sl] if k in ("g_cproj", "g_te") else v) for k, v in old.items()}
    return G


def check(G, R, *, store=False, with_res=True):
    """the bars of tests/test_hip_convnext_routes.py"""
    old = G["old"]
    want_gx = R["gx_conv"] + (R["gam"].double()[None] * R["gres"].double() if with_res else 0.0)
    close(G["gx"], want_gx, TOL_GX, "gx")
    close_rows(G["gx"], want_gx, edge_rows(R), TOL_GX, "gx")
    if R["cproj"] is not None and R["Fc"] > 0:
        close(G["g_cproj"], R["g_cproj"] + (0.0 if store else old["g_cproj"].double()), TOL_GX, "g_cproj")
    if R["te"] is not None:
        close(G["g_te"], old["g_te"].double() + R["g_te"], TOL_GX, "g_te")
    close(G["g_w"], old["g_w"].double() + R["g_w"], TOL_SUM, "g_w_dw")
    close(G["g_b"], old["g_b"].double() + R["g_b"], TOL_SUM, "g_b_dw")
    close(G["g_beta"], old["g_beta"].double() + R["g_beta"], TOL_SUM, "g_beta")
    close(G["g_ls"], old["g_ls"].double() + R["g_ls"], TOL_SUM, "g_log_scale")
    if with_res:
        close(G["g_gamma"], old["g_gamma"].double() + R["g_gamma"], TOL_SUM, "g_gamma")


# ------------------------------------------------------------------ against float64
def case(C, Fr, up, cond=True, fc_short=False, te=True, bdw=True, res=True, store=False, pad=8):
    tag = f"C{C}-F{Fr}-up{up}" + ("" if cond else "-nocond") + ("-fcshort" if fc_short else "") + ("" if te else "-note") + \
          ("" if bdw else "-nobdw") + ("" if res else "-nores") + ("-store" if store else "") + f"-pad{pad}"
    return pytest.param(C, Fr, up, cond, fc_short, te, bdw, res, store, pad, id=tag)


LONG = 6150      # B = 4: 385 tiles of 16 frames -> two tiles per block, 193 blocks per item
CASES = [
    # one chunk per lane
    case(8, 1, 1), case(8, 5, 2, store=True), case(8, T - 1, 4), case(8, T, 1, cond=False, pad=0),
    case(8, T + 1, 2, fc_short=True), case(8, 2 * T + 3, 4, store=True), case(8, 2 * T + 3, 4, fc_short=True, te=False),
    case(8, LONG, 2, store=True),
    # two chunks, the second partly filled (260) or full (384, 512)
    case(260, 1, 2, pad=0), case(260, 5, 4, fc_short=True, store=True), case(260, T - 1, 1, bdw=False),
    case(260, T, 2, store=True), case(260, T + 1, 4, cond=False), case(260, 2 * T + 3, 1, fc_short=True, res=False),
    case(260, LONG, 4, store=True),
    case(384, 1, 4), case(384, 5, 1, store=True), case(384, T - 1, 2, te=False), case(384, T, 4, store=True, pad=0),
    case(384, T + 1, 1, res=False), case(384, 2 * T + 3, 2, fc_short=True, store=True), case(384, 2 * T + 3, 4),
    case(512, 5, 2, cond=False), case(512, T - 1, 4, bdw=False, store=True), case(512, T, 1),
    case(512, T + 1, 4, fc_short=True), case(512, 2 * T + 3, 2, store=True),
    # three chunks
    case(768, 1, 1, store=True), case(768, 5, 4), case(768, T - 1, 2, store=True), case(768, T, 4, pad=0),
    case(768, T + 1, 2, fc_short=True), case(768, 2 * T + 3, 1, store=True), case(768, 2 * T + 3, 4, fc_short=True, store=True),
    case(768, 2 * T + 3, 2, te=False, res=False), case(768, T + 1, 1, cond=False, te=False, bdw=False, res=False),
    case(520, 2 * T + 3, 2, store=True),      # the third chunk partly filled
    case(768, 401, 4, store=True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("C,Fr,up,cond,fc_short,te,bdw,res,store,pad", CASES)
def test_against_float64(ops, C, Fr, up, cond, fc_short, te, bdw, res, store, pad):
    R = block_ref(C, Fr, up, 7, cond=cond, te=te, bdw=bdw, fc_short=fc_short)
    assert R["len_list"] == lens_for(Fr, 4)
    check(launch(ops, R, pad=pad, store=store, with_res=res), R, store=store, with_res=res)


def test_cases_cover_every_axis():
    """CPU: every value of every axis of the issue's list, and every pair (chunk count, up)"""
    v = [p.values for p in CASES]
    assert {c[0] for c in v} >= {8, 260, 384, 512, 768}
    assert {c[1] for c in v} >= {1, 5, T - 1, T, T + 1, 2 * T + 3}
    assert {((c[0] + 255) // 256, c[2]) for c in v if c[3]} == {(n, u) for n in (1, 2, 3) for u in (1, 2, 4)}
    for axis in range(3, 9):
        assert {c[axis] for c in v} == {False, True}, axis
    assert {(c[2], c[4]) for c in v if c[3]} >= {(u, s) for u in (1, 2, 4) for s in (False, True)}


# ------------------------------------------------------------------ bounds, accumulation, reproducibility
@pytest.mark.gpu
@pytest.mark.parametrize("C,Fr,up", [(8, 2 * T + 3, 2), (384, T + 1, 4), (768, 2 * T + 3, 1)])
def test_bounds(ops, C, Fr, up):
    """wide sentinel buffers round every matrix (launch asserts them) and a caller's workspace: NaN-filled where
    the partial rows go, sentinels behind -- every partial row is written, nothing behind them"""
    R = block_ref(C, Fr, up, 7)
    check(launch(ops, R, pad=12, own_ws=True), R)
    check(launch(ops, R, pad=12, own_ws=True, store=True), R, store=True)


@pytest.mark.gpu
@pytest.mark.parametrize("C,Fr,up", [(8, T + 1, 1), (512, 2 * T + 3, 2), (768, T - 1, 4)])
def test_accumulation(ops, C, Fr, up):
    """parameter gradients (and g_te, g_cproj without the store mode) pre-filled with 1.0 come back as 1.0 plus
    the sum"""
    R = block_ref(C, Fr, up, 7)
    G = launch(ops, R, fill=1.0)
    assert all(bool((v == 1.0).all()) for v in G["old"].values())
    check(G, R)


@pytest.mark.gpu
@pytest.mark.parametrize("C,Fr,up", [(8, LONG, 2), (384, 2 * T + 3, 4), (768, 2 * T + 3, 2)])
def test_reproducible(ops, C, Fr, up):
    """two launches on the same inputs: bit-identical outputs, every gradient sum included (no atomics)"""
    R = block_ref(C, Fr, up, 7)
    a, b = launch(ops, R), launch(ops, R)
    for k in ("gx", "g_cproj", "g_te") + SUMS:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


# ------------------------------------------------------------------ batch isolation
@functools.lru_cache(maxsize=None)
def scaled_ref(C, Fr, up):
    """block_ref's case with the rows of item b (x, gz, gres) scaled by 10^(b - 2), and its float64 results"""
    R = dict(block_ref(C, Fr, up, 7))
    B = R["B"]
    sc = torch.tensor([10.0 ** (b - 2) for b in range(B)])
    R["x"], R["gz"] = R["x"] * sc[:, None, None], R["gz"] * sc[:, None, None]
    R["gres"] = (R["gres"].view(B, Fr, C) * sc[:, None, None]).reshape(B * Fr, C)
    mask = (torch.arange(Fr)[None] < R["lens"][:, None]).double()[:, None]
    leaf = {k: R[k].double().requires_grad_() for k in ("x", "w_dw", "b_dw", "beta", "ls", "cproj", "te")}
    u, _, z = block_formula(leaf["x"], mask, leaf["w_dw"], leaf["b_dw"], leaf["beta"], leaf["ls"][0], leaf["cproj"], up,
                            leaf["te"])
    z.backward(R["gz"].double())
    R["gx_conv"], R["g_cproj"] = rows_of(leaf["x"].grad), rows_of(leaf["cproj"].grad)
    R["g_w"], R["g_b"], R["g_beta"], R["g_ls"], R["g_te"] = (leaf[k].grad for k in ("w_dw", "b_dw", "beta", "ls", "te"))
    R["g_gamma"] = (R["gres"].double() * rows_of(R["x"]).double()).sum(0)
    return R


@pytest.mark.gpu
@pytest.mark.parametrize("C,Fr,up", [(8, 2 * T + 3, 4), (384, T + 1, 2), (768, T, 1)])
def test_batch_isolation(ops, C, Fr, up):
    """item b's rows scaled by 10^(b - 2): every ITEM meets the bars against its own largest magnitude -- a halo
    frame read from the neighbouring item would be wrong by orders of magnitude"""
    R = scaled_ref(C, Fr, up)
    G = launch(ops, R, fill=0.0)
    check(G, R)
    B, Fc = R["B"], R["Fc"]
    want_gx = R["gx_conv"] + R["gam"].double()[None] * R["gres"].double()
    for b in range(B):
        rows = slice(b * Fr, (b + 1) * Fr)
        close(G["gx"][rows], want_gx[rows], TOL_GX, f"gx of item {b}")
        close(G["g_cproj"][b * Fc:(b + 1) * Fc], R["g_cproj"][b * Fc:(b + 1) * Fc], TOL_GX, f"g_cproj of item {b}")
        close(G["g_te"][b], R["g_te"][b], TOL_GX, f"g_te of item {b}")


# ------------------------------------------------------------------ the route in fused.block_bwd
RC, RH, RF, RB = 48, 144, 21, 4


@functools.lru_cache(maxsize=None)
def full_block_ref(K, up):
    """one whole ConvNeXt block in float64: block_formula, then pwconv1 -> PReLU -> pwconv2 + gamma * x; autograd"""
    R = dict(block_ref(RC, RF, up, K, B=RB))
    gen = torch.Generator().manual_seed(77 + K)
    W = dict(w1=torch.randn(RH, RC, generator=gen) * 0.1, b1=torch.randn(RH, generator=gen) * 0.1,
             al=0.25 + 0.1 * torch.randn(RH, generator=gen), w2=torch.randn(RC, RH, generator=gen) * 0.1,
             b2=torch.randn(RC, generator=gen) * 0.1, gam=R["gam"], gout=R["gres"])
    mask = (torch.arange(RF)[None] < R["lens"][:, None]).double()[:, None]
    leaf = {k: R[k].double().requires_grad_() for k in ("x", "w_dw", "b_dw", "beta", "ls", "cproj", "te")}
    _, _, z = block_formula(leaf["x"], mask, leaf["w_dw"], leaf["b_dw"], leaf["beta"], leaf["ls"][0], leaf["cproj"], up,
                            leaf["te"])
    zr = z.permute(0, 2, 1).reshape(-1, RC)
    gam = W["gam"].double().requires_grad_()
    a = zr @ W["w1"].double().t() + W["b1"].double()
    p = a.clamp(min=0) + W["al"].double() * a.clamp(max=0)
    y = p @ W["w2"].double().t() + W["b2"].double() + gam * leaf["x"].permute(0, 2, 1).reshape(-1, RC)
    y.backward(W["gout"].double())
    R.update(W, gx=rows_of(leaf["x"].grad), g_cproj=rows_of(leaf["cproj"].grad), g_gamma=gam.grad,
             **{"g_" + k: leaf[n].grad for k, n in (("w", "w_dw"), ("b", "b_dw"), ("beta", "beta"), ("ls", "ls"), ("te", "te"))})
    return R


def run_block_bwd(ops, R, counts=None, monkeypatch=None):
    """fused.block_fwd + fused.block_bwd of full_block_ref's block; returns what block_bwd returns plus the
    condition / time gradients and dz (block_bwd leaves it in the z buffer)"""
    from flow2gan_amd import fused
    K, up, Fc = R["K"], R["up"], R["Fc"]
    bp = fused._Blk([dev(R["w_dw"]), dev(R["b_dw"]), dev(R["ls"]).reshape(()), dev(R["beta"]), dev(R["w1"]).reshape(RH, RC, 1),
                     dev(R["b1"]), dev(R["al"]), dev(R["w2"]).reshape(RC, RH, 1), dev(R["b2"]), dev(R["gam"]).reshape(RC, 1)])
    x, lens = dev(rows_of(R["x"])), R["lens"].int().to(DEV)
    cp, te = dev(rows_of(R["cproj"])), dev(R["te"])
    cpa = (cp, RC, Fc, up, 0, te, RC, 0)
    _, z, a = fused.block_fwd(bp, x, RB, RF, lens, *cpa, keep=True)
    g_cp, g_te = torch.zeros(RB * Fc, RC, device=DEV), torch.zeros(RB, RC, device=DEV)
    if counts is not None:
        real = ops.call

        def counting(name, *args):
            counts[name] = counts.get(name, 0) + 1
            if name in ("f2g_dwnorm_bwd", "f2g_dwconv_bwd", "f2g_dwblock_bwd"):
                real(name, *args)
                counts.setdefault("kernels", []).append(last(ops))
                return
            real(name, *args)

        monkeypatch.setattr(ops, "call", counting)
    gx, grads = fused.block_bwd(bp, x, z, a, dev(R["gout"]), RB, RF, lens, False, False, *cpa, g_cproj=g_cp, g_te=g_te,
                                g_cproj_store=True)
    if counts is not None:
        monkeypatch.setattr(ops, "call", real)
    torch.cuda.synchronize()
    return dict(gx=gx, g_w=grads[0], g_b=grads[1], g_ls=grads[2].reshape(1), g_beta=grads[3], g_gamma=grads[9].reshape(RC),
                g_cproj=g_cp, g_te=g_te, dz=z, x=x, lens=lens, cpa=cpa, bp=bp)


def check_block(G, R):
    close(G["gx"], R["gx"], TOL_GX, "gx")
    close_rows(G["gx"], R["gx"], edge_rows(R), TOL_GX, "gx")
    close(G["g_cproj"], R["g_cproj"], TOL_GX, "g_cproj")
    close(G["g_te"], R["g_te"], TOL_GX, "g_te")
    for k in SUMS:
        close(G[k], R[k], TOL_SUM, k)


@pytest.mark.gpu
def test_route_fused_runs_one_launch(ops, monkeypatch):
    """tunable on: block_bwd ends in ONE f2g_dwblock_bwd call and allocates no du; float64 bars on the whole block"""
    R = full_block_ref(7, 2)
    monkeypatch.setattr(ops, "DW_BWD_FUSED", True)
    counts = {}
    G = run_block_bwd(ops, R, counts, monkeypatch)
    assert counts.get("f2g_dwblock_bwd") == 1 and "f2g_dwnorm_bwd" not in counts and "f2g_dwconv_bwd" not in counts, counts
    assert counts["kernels"] == ["blockbwd<nch=1>"]
    check_block(G, R)


@pytest.mark.gpu
def test_route_five_taps_keeps_the_pair(ops, monkeypatch):
    """tunable on, K = 5: f2g_dwblock_bwd_ok declines, block_bwd takes the two launches"""
    R = full_block_ref(5, 2)
    monkeypatch.setattr(ops, "DW_BWD_FUSED", True)
    counts = {}
    G = run_block_bwd(ops, R, counts, monkeypatch)
    assert counts.get("f2g_dwnorm_bwd") == 1 and counts.get("f2g_dwconv_bwd") == 1 and "f2g_dwblock_bwd" not in counts
    assert counts["kernels"] == ["dwnorm4<bwd=1,fw=4,nch=1>", "dwconv_bwd"]
    check_block(G, R)


@pytest.mark.gpu
def test_route_off_is_the_pair_bit_for_bit(ops, monkeypatch):
    """tunable off: block_bwd's outputs are those of ops.dwnorm_bwd + ops.dwconv_bwd called directly on the same
    dz, bit for bit -- gx, g_cproj, g_te.  The pair's second stages add the parameter-gradient sums by atomics
    (across items in dwnorm_reduce_kernel, across row blocks in f2g_colsum), so two runs of the very same launches
    differ in the last bit there: those are held to 1e-6 of the tensor's largest magnitude instead"""
    R = full_block_ref(7, 2)
    monkeypatch.setattr(ops, "DW_BWD_FUSED", False)
    counts = {}
    G = run_block_bwd(ops, R, counts, monkeypatch)
    assert counts["kernels"] == ["dwnorm4<bwd=1,fw=4,nch=1>", "dwconv4_bwd"], counts
    bp, x, lens, cpa = G["bp"], G["x"], G["lens"], G["cpa"]
    Fc = R["Fc"]
    g_cp, g_te = torch.zeros(RB * Fc, RC, device=DEV), torch.zeros(RB, RC, device=DEV)
    g_beta, g_ls, g_w, g_b, g_gam = ops.zeros_many([(RC,), (1,), (RC, 1, 7), (RC,), (RC, 1)], DEV)
    du, gx = torch.empty(RB * RF, RC, device=DEV), torch.empty(RB * RF, RC, device=DEV)
    ops.dwnorm_bwd(x, G["dz"], du, RB, RF, RC, 7, lens, bp.w_dw, bp.b_dw, bp.beta, bp.log_scale.reshape(1), *cpa,
                   g_cproj=g_cp, g_te=g_te, g_beta=g_beta, g_log_scale=g_ls, g_cproj_store=True)
    ops.dwconv_bwd(du, x, gx, RB, RF, RC, 7, lens, bp.w_dw, gres=dev(R["gout"]), gamma=bp.gamma.reshape(RC), g_w=g_w,
                   g_b=g_b, g_gamma=g_gam)
    torch.cuda.synchronize()
    for k, t in (("gx", gx), ("g_cproj", g_cp), ("g_te", g_te)):
        assert torch.equal(G[k].view(torch.int32), t.view(torch.int32)), k
    for k, t in (("g_w", g_w), ("g_b", g_b), ("g_gamma", g_gam.reshape(RC)), ("g_beta", g_beta), ("g_ls", g_ls)):
        close(G[k], t.double(), 1e-6, k)


# ------------------------------------------------------------------ end to end
TINY = dict(sampling_rate=24000, n_mels=100, mel_n_fft=1024, mel_hop_length=256,
            n_ffts=(512, 256, 128), hop_lengths=(256, 128, 64), channels=(48, 32, 24),
            time_embed_channels=32, hidden_factor=3, num_layers=(2, 2, 2),
            cond_enc_channels=32, cond_enc_num_layers=1)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["nodrop", "drop"])
def test_tiny_stage1_loss_and_all_grads_fused(ops, golden, tag, monkeypatch):
    """tests/test_hip_generator.py::test_tiny_stage1_loss_and_all_grads (its case, its tolerances, exact-fp32
    GEMMs) with the tunable on: every ConvNeXt block of the generator and of the condition encoder ends its
    backward in the one launch"""
    import flow2gan_amd as f2g
    g = golden("tiny_stage1")
    tt = lambda a: torch.from_numpy(np.asarray(a))
    m = f2g.MelAudioGenerator(**TINY)
    m.load_state_dict({k[2:]: tt(v) for k, v in g.items() if k.startswith("w/")})
    m = m.to(DEV).train()
    monkeypatch.setattr(random, "random", lambda: 0.0)  # limiter always on, as in the fixture
    bw = None
    if tag == "drop":
        u, idx = tt(g["drop_u"]), tt(g["drop_idx"])
        mask = torch.ones(2, 3)
        mask[torch.arange(2), idx] = 0.0
        mask = mask * 1.5
        bw = torch.where(u < 0.05, mask, torch.ones_like(mask)).t().contiguous().to(DEV)
    else:
        m.branch_dropout = 0.0
    counts = {}
    real = ops.call

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        real(name, *args)

    was = ops.DW_BWD_FUSED
    ops.DW_BWD_FUSED = True
    ops.call = counting
    try:
        loss = m(tt(g["mel"]).to(DEV), tt(g["audio"]).to(DEV), tt(g["lens"]), noise=tt(g["noise"]).to(DEV),
                 t=tt(g["t"]).to(DEV), branch_weights=bw)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.DW_BWD_FUSED = was
        ops.call = real
    print({k: v for k, v in counts.items() if "dw" in k})
    assert counts.get("f2g_dwblock_bwd", 0) >= 1 and "f2g_dwnorm_bwd" not in counts and "f2g_dwconv_bwd" not in counts, \
        {k: v for k, v in counts.items() if "dw" in k}
    want = float(g[f"{tag}/loss"])
    got = float(loss.detach())
    assert abs(got - want) < 2e-5 * abs(want), (got, want)
    worst = []
    for name, p in m.named_parameters():
        ref = tt(g[f"{tag}/g/{name}"])
        assert p.grad is not None, name
        err = float((p.grad.cpu().double() - ref.double()).abs().max())
        scale = float(ref.abs().max()) + 1e-12
        worst.append((err / scale, name))
    worst.sort(reverse=True)
    assert worst[0][0] < 2e-3, worst[:8]
