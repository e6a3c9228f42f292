"""f2g_dwblock_bwd (BiasNorm backward + depthwise-conv backward of a ConvNeXt block in one launch,
csrc/convnext.hip) -- the part that needs no GPU: the shape rule and the workspace query of the built library, every
refusal of the entry point (host checks: nothing is read through the fake addresses and nothing is launched), a
Python restatement of the block decomposition (tiles, halo frames, condition groups) and the tunable."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
BASE = 0x10000000          # fake, 16-byte aligned "device" addresses, 1 MiB apart
T, MAX_TILES, BLOCKS = 16, 8, 768        # csrc/convnext.hip: BB_T, BB_MAX_TILES, BB_BLOCKS


@pytest.fixture(scope="module")
def L():
    from flow2gan_amd import _lib
    return _lib


# ------------------------------------------------------------------ the rules, restated
def ok_rule(Cc, K, up, cond):
    return K == 7 and Cc % 4 == 0 and 4 <= Cc <= 768 and (not cond or up in (1, 2, 4))


def tiles_per_block(B, F):
    return min(MAX_TILES, max(1, B * ((F + T - 1) // T) // BLOCKS))


def blocks_per_item(B, F):
    tiles, tpb = (F + T - 1) // T, tiles_per_block(B, F)
    return (tiles + tpb - 1) // tpb


def decomposition(B, F):
    """[(block, tile start, owned frames, halo frames as (frame index, clamped row that is loaded))] of one item:
    block j walks tiles j * tpb .. j * tpb + tpb - 1; a tile owns [t0, min(t0 + T, F)); wave w of the block takes
    the owned frames t0 + 4 w .. t0 + 4 w + 3 and the halo frames t0 - 3, t0 - 2 | t0 - 1 | t0 + T, t0 + T + 1 |
    t0 + T + 2; frames outside [0, F) are skipped (du = 0 there), loads clamp their row index"""
    tpb = tiles_per_block(B, F)
    out = []
    for j in range(blocks_per_item(B, F)):
        for t in range(tpb):
            t0 = (j * tpb + t) * T
            if t0 >= F:
                break
            owned = [[f for f in range(t0 + 4 * w, t0 + 4 * w + 4) if f < F] for w in range(4)]
            halo = [f for f in (t0 - 3, t0 - 2, t0 - 1, t0 + T, t0 + T + 1, t0 + T + 2)]
            loads = [(f, min(max(f, 0), F - 1)) for f in halo]
            out.append((j, t0, owned, [f for f in halo if 0 <= f < F], loads))
    return out


# ------------------------------------------------------------------ shape rule and workspace
def test_ok_rule(L):
    lib = L.lib
    for Cc in range(1, 773):
        for K in (1, 3, 5, 7):
            for up in (1, 2, 3, 4, 8):
                for cond in (0, 1):
                    assert bool(lib.f2g_dwblock_bwd_ok(Cc, K, up, cond)) == ok_rule(Cc, K, up, bool(cond)), (Cc, K, up, cond)


def test_workspace_covers_one_partial_row_per_block(L):
    ws = L.lib.f2g_dwblock_bwd_workspace
    for B in (1, 4, 64, 1000):
        for F in range(1, 3 * T + 2):
            for Cc in (4, 260, 768):
                got = ws(B, F, Cc)
                assert got > 0
                assert got == B * blocks_per_item(B, F) * (11 * Cc + 1), (B, F, Cc)
    # one tile per block while there are few tiles: a block per started tile
    assert ws(1, T, 4) == 45 and ws(1, T + 1, 4) == 90 and ws(1, 3 * T + 1, 4) == 180
    # long items: several tiles per block, never more than MAX_TILES, still every tile covered
    for B, F in ((64, 752), (64, 188), (16, 752), (4096, 752)):
        tpb, nb = tiles_per_block(B, F), blocks_per_item(B, F)
        assert 1 <= tpb <= MAX_TILES and nb * tpb * T >= F and (nb - 1) * tpb * T < F
        assert ws(B, F, 384) == B * nb * (11 * 384 + 1)
    from flow2gan_amd import ops
    assert ops.DWBLOCK_T == T


# ------------------------------------------------------------------ refusals
POINTERS_N_F = ["x", "lens", "w_dw", "b_dw", "beta", "log_scale", "cproj", "te"]
POINTERS_N = ["gz", "g_cproj", "g_te", "g_beta", "g_log_scale"]
POINTERS_D = ["gx", "gres", "gamma", "g_w", "g_b", "g_gamma", "partials"]


def descriptor(L, Cc=64, K=7, up=2, B=2, F=20, cond=True):
    d = L.DwblockBwd()
    f, n = d.n.f, d.n
    addr = iter(range(BASE, BASE + (1 << 26), 1 << 20))
    for name in POINTERS_N_F:
        setattr(f, name, next(addr))
    for name in POINTERS_N:
        setattr(n, name, next(addr))
    for name in POINTERS_D:
        setattr(d, name, next(addr))
    if not cond:
        f.cproj = n.g_cproj = None
    f.B, f.F, f.C, f.K, f.Fc, f.up = B, F, Cc, K, (F + up - 1) // up, up
    f.ldx = n.ldgz = d.ldgx = d.ldgres = Cc + 4
    f.ldcp = f.ldte = 2 * Cc
    return d


def run(L, d):
    return L.lib.f2g_dwblock_bwd(C.byref(d), None)


def where(d, name):
    return d.n.f if name in POINTERS_N_F else (d.n if name in POINTERS_N else d)


@pytest.mark.parametrize("name", ["x", "gz", "gx", "w_dw", "beta", "log_scale", "partials"])
def test_null_pointer_is_refused(L, name):
    d = descriptor(L)
    setattr(where(d, name), name, None)
    assert run(L, d) == EINVAL


def test_du_is_refused(L):
    d = descriptor(L)
    d.n.du = BASE + (1 << 27)
    assert run(L, d) == EINVAL


@pytest.mark.parametrize("kw", [dict(K=5), dict(Cc=6), dict(Cc=772), dict(up=3)], ids=["K5", "C6", "C772", "up3-cond"])
def test_shape_is_refused(L, kw):
    assert run(L, descriptor(L, **kw)) == EINVAL


@pytest.mark.parametrize("name", POINTERS_N_F + POINTERS_N + POINTERS_D)
def test_misaligned_pointer_is_refused(L, name):
    d = descriptor(L)
    setattr(where(d, name), name, getattr(where(d, name), name) + 4)
    assert run(L, d) == EINVAL


@pytest.mark.parametrize("name", ["ldx", "ldgz", "ldgx", "ldgres", "ldcp", "ldte"])
def test_stride_not_in_float4s_is_refused(L, name):
    d = descriptor(L)
    setattr(where(d, {"ldx": "x", "ldcp": "x", "ldte": "x", "ldgz": "gz"}.get(name, "gx")), name, 70)
    assert run(L, d) == EINVAL


@pytest.mark.parametrize("name", ["x", "gz", "gres"])
def test_gx_aliasing_an_input_is_refused(L, name):
    d = descriptor(L)
    d.gx = getattr(where(d, name), name)
    assert run(L, d) == EINVAL


def test_empty_batch_is_ok_without_a_gpu(L):
    """every check passes and nothing is launched: the same descriptor with B = 0 or F = 0 returns F2G_OK on a host
    without a GPU; up = 3 without a condition input is no refusal either"""
    for kw in (dict(B=0), dict(F=0), dict(B=0, up=3, cond=False)):
        assert run(L, descriptor(L, **kw)) == 0, kw


# ------------------------------------------------------------------ the decomposition
def test_decomposition_owns_every_frame_once():
    for B in (1, 64, 1024):
        for F in range(1, 201):
            tiles = decomposition(B, F)
            owned = [f for _, _, ow, _, _ in tiles for wv in ow for f in wv]
            assert sorted(owned) == list(range(F)), (B, F)
            for up in (1, 2, 4):
                owner = {}
                for j, t0, ow, _, _ in tiles:
                    for w, frames in enumerate(ow):
                        for f in frames:
                            # one wave of one tile of one block sums a condition row's frames
                            assert owner.setdefault(f // up, (j, t0, w)) == (j, t0, w), (B, F, up, f)
            for j, t0, ow, halo, loads in tiles:
                assert all(0 <= row < F for _, row in loads), (B, F, t0)
                assert all(0 <= f < F for f in halo)
                # the du rows phase 2 reads for the owned frames are exactly the owned and halo frames inside [0, F)
                need = {g for wv in ow for f in wv for g in range(f - 3, f + 4) if 0 <= g < F}
                have = {f for wv in ow for f in wv} | set(halo)
                assert need <= have, (B, F, t0)
                assert all(0 <= g - (t0 - 3) < T + 6 for g in have)


# ------------------------------------------------------------------ the tunable
def test_tunable_is_off_by_default_and_follows_f2g_opts(monkeypatch):
    from flow2gan_amd import _opts, ops
    assert ops.DW_BWD_FUSED is False
    assert "dw_bwd_fused" in _opts._ASKED and "dw_bwd_fused" in _opts.__doc__
    assert "`dw_bwd_fused`" in open(os.path.join(ROOT, "README.md")).read()
    monkeypatch.setattr(_opts, "_OPTS", _opts._parse("dw_bwd_fused=1"))
    assert _opts.opt("dw_bwd_fused", False) is True
    monkeypatch.setattr(_opts, "_OPTS", _opts._parse("DW_BWD_FUSED=0"))
    assert _opts.opt("dw_bwd_fused", False) is False
