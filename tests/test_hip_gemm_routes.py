"""Route matrix of f2g_gemm: every kernel instance the dispatch can pick, reached on purpose and named
(f2g_gemm_last_kernel), at the edges where kernels go wrong, against float64.

Operands are POISONED: each logical operand sits inside a larger NaN buffer -- padding columns (ld > cols), a
prefix before `base`, at least a tile of rows after the last one; windowed operands have NaN everywhere outside
the positions their windows cover.  The contract (include/flow2gan_hip.h: "invalid elements read as 0") means
none of it may reach a result: an element read past the operand and multiplied by a zero weight still turns
the result into NaN.  Outputs are surrounded by sentinel guards (unchanged bit for bit), stored outputs are
pre-filled with NaN (every logical element must be written), accumulated ones with finite values the result
must include.  Each element is checked against the scale of its own products,
|got - want| <= tol * (|A| |B|^T + |epilogue terms|)[i, j].
"""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
NAN = float("nan")
SENT = 7.25            # guard sentinel
# per-element tolerance relative to the row scale: exact fp32 (and the fp32-class six-product mode); split-bf16
# (the dropped lo*lo term is <= 2^-16 per product); plain bf16 over the bf16-ROUNDED operands
TOL = {"fp32": 1e-6, "bf16x3": 3e-5, "bf16hi": 1e-5, "bf16": 1e-5, "bf16x6": 1e-6}
# operand modes of the lean kernel: (f2g_gemm_desc.precision, f2g_operand.split, pm of its name)
MODES = {"fp32": (0, 0, 0), "bf16x3": (1, 1, 1), "bf16hi": (2, 1, 2), "bf16": (2, 2, 3)}

# every kernel name f2g_gemm_last_kernel can report, and where this module reaches it (the ledger test below
# compares the set with the literals in csrc/)
ROUTES = set()


def route(*names):
    ROUTES.update(names)
    return names[0] if len(names) == 1 else names


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from flow2gan_amd import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def last_kernel(ops):
    return ops.L.lib.f2g_gemm_last_kernel().decode()


# ------------------------------------------------------------------ poisoned operands
class Op:
    """An operand inside a NaN buffer: `flat` (fp32, what the reference reads), `img` (what the kernel reads:
    the fp32 buffer, its split-bf16 image or its bf16 copy), `o` (the descriptor), `off` (elements before base)."""

    def __init__(self, ops, flat, split, off, **fields):
        self.flat, self.split, self.off = flat, split, off
        self.img = flat if split == 0 else (ops.split_bf16(flat) if split == 1 else ops.to_bf16(flat))
        o = ops.L.Operand()
        o.base = self.img.data_ptr() + (2 if split == 2 else 4) * off
        o.split = split
        f = dict(P1=1, P0=1, step1=0, pad1=0, L1=1, step0=0, pad0=0, unit=1, line_stride=0, reflect=0,
                 unbounded=0)
        f.update(fields)
        f.setdefault("seglen", f["cols"])
        f.setdefault("L0u", f["cols"])
        for k, v in f.items():
            setattr(o, k, v)
        self.o = o

    def dense(self, bf16=False, r0=0, r1=None):
        """float64 rows [r0, r1) of what the descriptor addresses, by the header's formula (invalid = 0)."""
        o = self.o
        r1 = o.rows if r1 is None else r1
        src = self.flat.bfloat16().float() if bf16 else self.flat
        if o.P0 == 1 and o.P1 == 1 and o.L1 == 1 and o.seglen >= o.cols and o.L0u >= o.cols and not o.reflect \
                and not o.unbounded:                    # plain matrix: a view, no index tensors
            assert self.off + r1 * o.seq_stride <= self.flat.numel()
            v = src[self.off + r0 * o.seq_stride:self.off + r1 * o.seq_stride].view(r1 - r0, o.seq_stride)[:, :o.cols]
            v = v.double()
            assert torch.isfinite(v).all(), "test bug: a valid element of the operand is poison"
            return v
        r = torch.arange(r0, r1, device=DEV)
        c = torch.arange(o.cols, device=DEV)
        p0, q = r % o.P0, r // o.P0
        p1, s = q % o.P1, q // o.P1
        seglen = min(o.seglen, o.cols)
        l1 = (p1 * o.step1 - o.pad1)[:, None] + (c // seglen)[None, :]
        e = ((p0 * o.step0 - o.pad0) * o.unit)[:, None] + (c % seglen)[None, :]
        if o.reflect:
            e = e.abs()
            e = torch.where(e >= o.L0u, 2 * (o.L0u - 1) - e, e)
        ok = (l1 >= 0) & (l1 < o.L1) & (e >= 0) & (e < o.L0u)
        addr = self.off + (s * o.seq_stride)[:, None] + l1 * o.line_stride + e
        inside = (addr >= 0) & (addr < self.flat.numel())
        if o.unbounded:         # (reads past the sequence ends inside the buffer, zeros outside it: the caller pairs
            ok = inside         # them with zeros)
        assert bool((inside | ~ok).all()), "test bug: a valid element lies outside the buffer"
        ok = ok & inside
        v = src.double()[torch.where(ok, addr, 0)]
        v = torch.where(ok, v, torch.zeros_like(v))
        assert torch.isfinite(v).all(), "test bug: a valid element of the operand is poison"
        return v


def plain(ops, x, split=0, pre=None, tail=256, pad=None):
    """x (rows, cols) at `pre` elements into a NaN buffer, row stride = cols rounded up + `pad` columns."""
    rows, cols = x.shape
    q = 8 if split == 2 else 4                          # (16-byte rows / offsets: lean_b_ok, lean_bf16_ok)
    pre = q if pre is None else pre
    ld = -(-cols // q) * q + (q if pad is None else pad)
    flat = torch.full((pre + (rows + tail) * ld,), NAN, device=DEV)
    flat[pre:pre + rows * ld].view(rows, ld)[:, :cols] = x
    return Op(ops, flat, split, pre, rows=rows, cols=cols, seq_stride=ld)


def win1(ops, x, L_out, step, pad, taps, split=0, gap=8, pre=8, reflect=False, covered_only=True):
    """1-D windows over a (nseq, L, C) map, sequences `gap` elements apart, NaN between them and (covered_only)
    at every position no window of the descriptor reads."""
    nseq, L, Cc = x.shape
    stride = L * Cc + gap
    flat = torch.full((pre + nseq * stride + 256 * Cc,), NAN, device=DEV)
    view = flat[pre:pre + nseq * stride].view(nseq, stride)[:, :L * Cc].view(nseq, L, Cc)
    view.copy_(x)
    if covered_only and not reflect:
        used = torch.zeros(L, dtype=torch.bool)
        for p in range(L_out):
            lo = p * step - pad
            used[max(lo, 0):max(min(lo + taps, L), 0)] = True
        view[:, ~used.to(DEV)] = NAN
    return Op(ops, flat, split, pre, rows=nseq * L_out, cols=taps * Cc, P0=L_out, step0=step, pad0=pad, unit=Cc,
              L0u=L * Cc, seq_stride=stride, reflect=int(reflect))


def win2(ops, x, kh, kw, split=0, pre=8):
    """(kh, kw) windows, stride 1, no padding, over (nseq, H, W, C) maps: kh segments of kw * C columns; NaN
    between lines, between sequences and in the columns no window reaches."""
    nseq, H, W, Cc = x.shape
    line = W * Cc + 8
    seq = H * line + 16
    flat = torch.full((pre + nseq * seq + 64 * line,), NAN, device=DEV)
    v = flat[pre:pre + nseq * seq].view(nseq, seq)[:, :H * line].view(nseq, H, line)[:, :, :W * Cc]
    v.copy_(x.reshape(nseq, H, W * Cc))
    Ho, Wo = H - kh + 1, W - kw + 1
    return Op(ops, flat, split, pre, rows=nseq * Ho * Wo, cols=kh * kw * Cc, P1=Ho, P0=Wo, seglen=kw * Cc,
              step1=1, L1=H, step0=1, unit=Cc, L0u=W * Cc, seq_stride=seq, line_stride=line)


# ------------------------------------------------------------------ guarded outputs
class Out:
    """M x N output inside a sentinel buffer; `fill` = NaN (stores) or a finite (M, N) tensor (accumulation).
    rowmap = (P0o, seq_stride_o, row_stride_o, off_o) as in f2g_epilogue."""

    def __init__(self, M, N, fill=NAN, rowmap=None, guard=64):
        self.M, self.N = M, N
        self.ldc = -(-N // 4) * 4 + 4
        self.rowmap, self.base = rowmap, guard
        if rowmap:
            r = torch.arange(M, device=DEV)
            P0o, sso, rso, offo = rowmap
            roff = (r // P0o) * sso + (r % P0o) * rso + offo
            self.offs = guard + roff[:, None] + torch.arange(N, device=DEV)[None, :]
            size = (int(self.offs.max()) + 1 if M else guard) + guard + 2 * self.ldc
        else:
            size = guard + (M + 2) * self.ldc + guard
        self.flat = torch.full((size,), SENT, device=DEV)
        if rowmap:
            self.flat[self.offs] = fill if isinstance(fill, torch.Tensor) else torch.full((M, N), fill, device=DEV)
        else:
            self.view()[:, :N] = fill

    def view(self):
        """the plain output as an (M, ldc) view"""
        return self.flat[self.base:self.base + self.M * self.ldc].view(self.M, self.ldc)

    def got(self, r0=0, r1=None):
        """float64 rows [r0, r1) of the output"""
        r1 = self.M if r1 is None else r1
        if self.rowmap:
            return self.flat[self.offs[r0:r1]].double()
        return self.view()[r0:r1, :self.N].double()

    def guards_ok(self):
        if self.rowmap:
            mask = torch.ones(self.flat.numel(), dtype=torch.bool, device=DEV)
            mask[self.offs] = False
            ok = bool((self.flat[mask] == SENT).all())
        else:
            end = self.base + self.M * self.ldc
            ok = bool((self.flat[:self.base] == SENT).all()) and bool((self.flat[end:] == SENT).all()) and \
                bool((self.view()[:, self.N:] == SENT).all())
        assert ok, "a guard element of the output was written"


class Vec:
    """column-sum vector (accumulated onto finite values) between sentinel guards"""

    def __init__(self, N, seed):
        self.init = rnd(N, seed=seed)
        self.flat = torch.full((N + 8,), SENT, device=DEV)
        self.flat[4:4 + N] = self.init
        self.N = N

    def ptr(self):
        return self.flat.data_ptr() + 16

    def got(self):
        assert bool((self.flat[:4] == SENT).all()) and bool((self.flat[4 + self.N:] == SENT).all())
        return self.flat[4:4 + self.N].double()


def make_desc(ops, A, B, out, *, form=0, precision=0, split_k=1, bias=None, res=None, gamma=None, aux=None,
              alpha_n=None, colsum=None, colsum_alpha=None, lrelu=0.0, scale=0.0, accumulate=False, atomic=False):
    """the f2g_gemm_desc of a launch (A / B: Op or f2g_operand; out: Out)"""
    L = ops.L
    d = L.GemmDesc()
    d.A, d.B = getattr(A, "o", A), getattr(B, "o", B)
    e = L.Epilogue()
    e.C = out.flat.data_ptr() + 4 * out.base
    e.ldc = out.ldc
    if out.rowmap:
        e.P0o, e.seq_stride_o, e.row_stride_o, e.off_o = out.rowmap
    e.bias = None if bias is None else bias.data_ptr()
    if res is not None:
        e.res, e.ldres = res.data_ptr(), res.stride(0)
    e.gamma = None if gamma is None else gamma.data_ptr()
    if aux is not None:
        e.aux, e.ldaux, e.alpha_n = aux.data_ptr(), aux.stride(0), alpha_n.data_ptr()
    e.colsum = None if colsum is None else colsum.ptr()
    e.colsum_alpha = None if colsum_alpha is None else colsum_alpha.ptr()
    e.lrelu_slope, e.scale = lrelu, scale
    e.accumulate, e.atomic = int(accumulate), int(atomic)
    d.E = e
    d.form, d.split_k, d.precision = form, split_k, precision
    return d


def launch(ops, A, B, out, **kw):
    d = make_desc(ops, A, B, out, **kw)
    ops.call("f2g_gemm", C.byref(d))
    torch.cuda.synchronize()
    return d


def lean_ok(ops, d):
    return ops.L.lib.f2g_gemm_lean_ok(C.byref(d))


def x6_ok(ops, d):
    return ops.L.lib.f2g_gemm_x6_ok(C.byref(d))


def expect(acc, mag, *, bias=None, res=None, gamma=None, aux=None, alpha_n=None, lrelu=0.0, scale=0.0, c0=None):
    """the generic epilogue's arithmetic (gemm_common.h: gemm_epilogue) in float64: (out, its scale, colsum, its
    scale, colsum_alpha)"""
    s = scale if scale else 1.0
    v, m = acc * s, mag * abs(s)
    if bias is not None:
        v, m = v + bias.double()[None], m + bias.double().abs()[None]
    if res is not None:
        gm = gamma.double()[None] if gamma is not None else 1.0
        v, m = v + gm * res.double(), m + (gm * res.double()).abs()
    csa = None
    if aux is not None:
        a = aux.double()
        csa = (v * a.clamp(max=0)).sum(0), (m * a.clamp(max=0).abs()).sum(0)
        mult = torch.where(a > 0, torch.ones_like(a), alpha_n.double()[None].expand_as(a))
        v, m = v * mult, m * mult.abs()
    if lrelu:
        v = torch.where(v > 0, v, lrelu * v)
    cs = v.sum(0), m.sum(0)
    if c0 is not None:
        v, m = v + c0.double(), m + c0.double().abs()
    return v, m, cs, csa


def check(got, want, mag, tol, what):
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    err = (got - want).abs()
    bad = err > tol * mag + 1e-30
    assert not bool(bad.any()), \
        f"{what}: {int(bad.sum())} elements off, worst {float((err / (mag + 1e-30)).max()):.3e} (tol {tol:.0e})"


CHUNK = 1024      # output rows per piece of the float64 reference (keeps its device footprint small)


def products(A, B, form, bf16, b=None, r0=0, r1=None):
    """float64 A.B (by the form's convention) and |A|.|B| -- output rows [r0, r1) for forms 0 / 1"""
    b = B.dense(bf16) if b is None else b
    if form == 2:
        a = A.dense(bf16)
        return a.t() @ b, a.abs().t() @ b.abs()
    a = A.dense(bf16, r0, r1)
    bt = b.t() if form == 0 else b
    return a @ bt, a.abs() @ bt.abs()


EPI = {   # epilogue instances of the lean kernel (selection: gemm_lean.hip f2g_launch_lean, "epilogue instance")
    0: dict(bias=True, res=True, lrelu=0.1),
    1: dict(bias=True, aux=True, colsum=True),
    2: dict(bias=True, colsum=True, lrelu=0.2, rowmap=True),
    3: dict(bias=True, res=True, colsum=True, scale=0.75, accumulate=True),
}


def run(ops, A, B, M, N, *, form=0, mode="fp32", epi=None, seed=0, split_k=1, tol=None, precision=None):
    """one launch with the epilogue `epi` (dict of EPI's keys) against float64; returns the descriptor and C"""
    epi = epi or {}
    prec = MODES[mode][0] if precision is None else precision
    bf16 = mode in ("bf16hi", "bf16")
    kw, ref = {}, {}
    if epi.get("bias"):
        kw["bias"] = ref["bias"] = rnd(N, seed=seed + 1)
    if epi.get("res"):
        kw["res"] = ref["res"] = rnd(M, N, seed=seed + 2)
        kw["gamma"] = ref["gamma"] = rnd(N, seed=seed + 3)
    if epi.get("aux"):
        kw["aux"] = ref["aux"] = rnd(M, N, seed=seed + 4)
        kw["alpha_n"] = ref["alpha_n"] = 0.25 + 0.1 * rnd(N, seed=seed + 5)
        kw["colsum_alpha"] = Vec(N, seed + 6)
    if epi.get("colsum"):
        kw["colsum"] = Vec(N, seed + 7)
    for k in ("lrelu", "scale"):
        if epi.get(k):
            kw[k] = ref[k] = epi[k]
    c0 = None
    if epi.get("accumulate") or epi.get("atomic"):
        c0 = ref["c0"] = rnd(M, N, seed=seed + 8)
        kw["accumulate" if epi.get("accumulate") else "atomic"] = True
    rowmap = None
    if epi.get("rowmap"):      # rows of 40-row sequences interleaved two apart, 3 spare lines per sequence
        ldo = -(-N // 4) * 4 + 4
        rowmap = (40, (2 * 40 + 3) * ldo, 2 * ldo, ldo + 4)
    out = Out(M, N, NAN if c0 is None else c0, rowmap=rowmap)
    d = launch(ops, A, B, out, form=form, precision=prec, split_k=split_k, **kw)
    out.guards_ok()
    tol = TOL[mode] if tol is None else tol
    name = last_kernel(ops)
    b = B.dense(bf16)
    cs = csa = None
    step = M if form == 2 else CHUNK
    for r0 in range(0, max(M, 1), step):
        r1 = min(M, r0 + step)
        acc, mag = products(A, B, form, bf16, b, r0, r1)
        rows = {k: (v[r0:r1] if k in ("res", "aux", "c0") else v) for k, v in ref.items()}
        want, wmag, cs_c, csa_c = expect(acc, mag, **rows)
        check(out.got(r0, r1), want, wmag, tol, f"C rows {r0}..{r1} ({mode}, {name})")
        cs = cs_c if cs is None else (cs[0] + cs_c[0], cs[1] + cs_c[1])
        if csa_c is not None:
            csa = csa_c if csa is None else (csa[0] + csa_c[0], csa[1] + csa_c[1])
    if "colsum" in kw:
        check(kw["colsum"].got(), kw["colsum"].init.double() + cs[0], cs[1] + kw["colsum"].init.double().abs(),
              tol, "colsum")
    if "colsum_alpha" in kw:
        ca = kw["colsum_alpha"]
        check(ca.got(), ca.init.double() + csa[0], csa[1] + ca.init.double().abs(), tol, "colsum_alpha")
    return d, out


def mode_ops(ops, mode, A_x, B_x, win=None):
    """A (poisoned, plain or from a windowed-operand builder) and B (plain, poisoned) in `mode`'s format"""
    sp = MODES[mode][1]
    A = win(sp) if win else plain(ops, A_x, sp)
    return A, plain(ops, B_x, sp)


# ------------------------------------------------------------------ lean kernel, 128-row tiles
LEAN_CASES = []
for _mode in MODES:
    for _ep in range(4):
        LEAN_CASES.append((_mode, _ep))
        route(f"lean<sk=0,ep={_ep},pm={MODES[_mode][2]}>")


@pytest.mark.gpu
@pytest.mark.parametrize("mode,ep", LEAN_CASES)
def test_lean_operand_modes_and_epilogues(ops, mode, ep):
    """4 operand modes x 4 epilogue instances: one slab, ragged rows / columns, long K, multi-segment windows"""
    seed = 17 * ep + len(mode)
    bf = mode == "bf16"
    N = (65, 130, 257, 130)[ep]
    Bx = None
    if ep == 3:                 # (5, 12, 22, 32) maps, (3, 2) windows: 3 segments of 64 columns, M = 1050
        x = rnd(5, 12, 22, 32, seed=seed)
        K = 192
        Bx = rnd(N, K, seed=seed + 9, scale=0.1)
        A, B = mode_ops(ops, mode, None, Bx, win=lambda sp: win2(ops, x, 3, 2, split=sp))
        M = A.o.rows
    else:
        M = (1, 127, 129)[ep]
        K = ((64 if bf else 32), (128 if bf else 96), 640)[ep]
        A, B = mode_ops(ops, mode, rnd(M, K, seed=seed), rnd(N, K, seed=seed + 9, scale=0.1))
    d, _ = run(ops, A, B, M, N, mode=mode, epi=EPI[ep], seed=seed)
    assert last_kernel(ops) == f"lean<sk=0,ep={ep},pm={MODES[mode][2]}>"
    assert ops.L.lib.f2g_gemm_last_path() == 1
    assert lean_ok(ops, d) & 1, "f2g_gemm_lean_ok disagrees with the launch"
    if bf:
        assert lean_ok(ops, d) == 3, "true bf16 operands ran, but f2g_gemm_lean_ok does not report them"


# ------------------------------------------------------------------ lean kernel, 256-row tiles
TALL = [(pm_mode, ep) for pm_mode in ("bf16x3", "bf16") for ep in range(4)]
for _m, _ep in TALL:
    route(f"lean_tall<ep={_ep},pm={MODES[_m][2]}>")


@pytest.mark.gpu
@pytest.mark.parametrize("mode,ep", TALL)
def test_lean_tall_instances(ops, mode, ep, lib_option):
    lib_option("lean_tall", 2)
    lib_option("streamk", 0)
    M = (257, 511, 1000, 1000)[ep]
    N, K = (130, 257, 130, 200)[ep], 128
    A, B = mode_ops(ops, mode, rnd(M, K, seed=ep), rnd(N, K, seed=ep + 1, scale=0.1))
    d, _ = run(ops, A, B, M, N, mode=mode, epi=EPI[ep], seed=ep, split_k=0 if ep == 3 else 1)
    assert last_kernel(ops) == f"lean_tall<ep={ep},pm={MODES[mode][2]}>"
    assert lean_ok(ops, d) & 1
    if mode == "bf16":
        assert lean_ok(ops, d) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("ep", [route("lean_tap<ep=2>") and 2, route("lean_tap<ep=3>") and 3])
def test_lean_tap_instances(ops, ep, lib_option):
    """stride-1 five-tap windows over maps of 69 positions (64 outputs: 4 sequences per 256-row tile; the last
    position is covered by no window and holds NaN), 64 channels"""
    lib_option("lean_tall", 2)
    lib_option("streamk", 0)
    x = rnd(9, 69, 64, seed=ep)
    A = win1(ops, x, 64, 1, 0, 5, split=1, gap=0)
    B = plain(ops, rnd(130, 320, seed=ep + 1, scale=0.1), 1)
    d, _ = run(ops, A, B, A.o.rows, 130, mode="bf16x3", epi=EPI[ep], seed=ep)
    assert last_kernel(ops) == f"lean_tap<ep={ep}>"
    assert lean_ok(ops, d) & 1


@pytest.mark.gpu
def test_lean_tall_rule(ops, lib_option):
    """the default rule (lean_tall = 1): >= 400 tall tiles and K >= 640; 0 never, 2 always"""
    M, N, K = 25600, 512, 640
    A, B = mode_ops(ops, "bf16x3", rnd(M, K, seed=3), rnd(N, K, seed=4, scale=0.1))
    for v, name in ((1, "lean_tall<ep=0,pm=1>"), (0, "lean<sk=0,ep=0,pm=1>"), (2, "lean_tall<ep=0,pm=1>")):
        lib_option("lean_tall", v)
        d, out = run(ops, A, B, M, N, mode="bf16x3", epi=dict(bias=True), seed=3)
        del out
        assert last_kernel(ops) == name, v
        assert lean_ok(ops, d) & 1
    # one row tile fewer than 400 tall tiles: the 128-row instance
    lib_option("lean_tall", 1)
    A = None
    A2 = plain(ops, rnd(M - 256, K, seed=5), 1)
    run(ops, A2, B, M - 256, N, mode="bf16x3", seed=5)
    assert last_kernel(ops) == "lean<sk=0,ep=0,pm=1>"


# ------------------------------------------------------------------ stream-K
def stream_k_rule(M, N, K, mode, streamk, streamk_min):
    """units per block, or 0 (gemm_lean.hip: f2g_lean_stream_k; true bf16 operands count 64-element slabs)"""
    if streamk == 0:
        return 0
    tiles = -(-M // 128) * -(-N // 128)
    nt = (K // 2 if mode == "bf16" else K) // 32
    if nt < 16:
        return 0
    if tiles * 2 > 256:
        if streamk < 2:
            return 0
        if (tiles / 512) / -(-tiles // 512) > 0.9:
            return 0
    return max(-(-tiles * nt // 512), streamk_min)


SK_CASES = [   # M, N, K, mode, streamk, streamk_min, accumulate
    (100, 100, 512, "fp32", 1, 4, False),              # 1 tile, 16 slabs
    (300, 100, 544, "bf16x3", 1, 1, True),             # 3 tiles, 17 slabs
    (896, 65, 1056, "fp32", 1, 3, False),              # 7 tiles, 33 slabs
    (384, 300, 3200, "bf16hi", 1, 16, True),           # 9 tiles, 100 slabs
    (16507, 100, 544, "fp32", 1, 4, False),            # 129 tiles: not the latency regime
    (16507, 100, 544, "bf16x3", 2, 4, True),           # ... but under-filled rounds
    (12797, 300, 1024, "bf16", 2, 4, False),           # 300 tiles, 16 bf16 slabs
    (300, 200, 960, "bf16", 1, 4, False),              # 30 fp32 slabs = 15 bf16 slabs: no stream-K
    (260, 130, 1056, "fp32", 0, 4, True),              # option off
    (130, 700, 3232, "bf16x3", 2, 16, False),          # 6 tiles, 101 slabs
]
for _c in SK_CASES:          # (the name each case asserts)
    route(f"lean<sk={1 if stream_k_rule(*_c[:6]) else 0},ep=3,pm={MODES[_c[3]][2]}>")


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,mode,streamk,smin,acc", SK_CASES)
def test_stream_k(ops, M, N, K, mode, streamk, smin, acc, lib_option):
    """library-chosen split (split_k = 0) on the lean kernel: bias / residual once, colsum and scale under the
    atomic seams, the zero fill of a NaN C or accumulation onto a finite one"""
    lib_option("streamk", streamk)
    lib_option("streamk_min", smin)
    A, B = mode_ops(ops, mode, rnd(M, K, seed=M), rnd(N, K, seed=N, scale=0.1))
    epi = dict(bias=True, res=True, colsum=True, scale=1.5, accumulate=acc)
    d, _ = run(ops, A, B, M, N, mode=mode, epi=epi, seed=K, split_k=0)
    upb = stream_k_rule(M, N, K, mode, streamk, smin)
    assert lean_ok(ops, d) & 1
    assert ops.L.lib.f2g_gemm_last_path() == (2 if upb else 1)
    assert last_kernel(ops) == f"lean<sk={1 if upb else 0},ep=3,pm={MODES[mode][2]}>"


# ------------------------------------------------------------------ generic MFMA tiles, split-K
def auto_split(M, N, K):
    """gemm.hip: auto_split -- the library's own K split of a generic launch"""
    if N <= 64:
        return 1
    tiles = -(-M // 128) * -(-N // 128)
    nk = -(-K // 32)
    if tiles * 2 <= 256 and nk >= 16:
        s = min(nk // 8, 8)
        if s * tiles > 256:
            s = 256 // tiles
        return s if s >= 2 else 1
    if nk < 64:
        return 1

    def eff(s):
        return (tiles * s / 512.0) / ((tiles * s + 511) // 512)
    best, best_s = eff(1) + 0.15, 1
    for s in range(2, 9):
        if nk // s < 20:
            break
        if eff(s) > best:
            best, best_s = eff(s), s
    return best_s


def _generic_ops(ops, kind, M, N, K, seed):
    """A, B, form of a generic route: kind = (form, loader modes of A / B)"""
    if kind == "F0,PF,PF":
        return plain(ops, rnd(M, K, seed=seed)), plain(ops, rnd(N, K, seed=seed + 1, scale=0.1)), 0
    if kind in ("F0,GF,PF", "F1,GF,PF"):         # padded three-tap windows: not the lean kernel's
        A = win1(ops, rnd(M // 10, 12, K // 3, seed=seed), 10, 1, 1, 3)
        Bx = rnd(N, K, seed=seed + 1, scale=0.1)
        return A, plain(ops, Bx if kind[1] == "0" else Bx.t().contiguous()), int(kind[1])
    if kind == "F0,GR,PF":                       # STFT framing: reflect-padded frames of 64 samples, hop 16
        A = win1(ops, rnd(M // 25, 400, 1, seed=seed), 25, 16, 32, 64, reflect=True)
        return A, plain(ops, rnd(N, 64, seed=seed + 1, scale=0.1)), 0
    if kind in ("F0,SL,SL", "F1,SL,SL"):         # K % 4 != 0
        f = int(kind[1])
        Bx = rnd(N, K, seed=seed + 1, scale=0.1)
        return plain(ops, rnd(M, K, seed=seed)), plain(ops, Bx if f == 0 else Bx.t().contiguous()), f
    if kind == "F1,PF,PF":
        return plain(ops, rnd(M, K, seed=seed)), plain(ops, rnd(K, N, seed=seed + 1, scale=0.1)), 1
    raise AssertionError(kind)


GENERIC_CASES = [   # kind, M, N, K, split_k, expected split in the name, operand mode (fp32 operands; bf16x3 /
    ("F0,PF,PF", 300, 40, 64, 1, 1, "fp32"),         # bf16hi: the generic split-bf16 core, which splits them itself)
    ("F0,GF,PF", 300, 96, 96, 2, 2, "fp32"),
    ("F0,GF,PF", 300, 96, 96, 3, 3, "bf16x3"),
    ("F0,GR,PF", 250, 66, 64, 1, 1, "fp32"),
    ("F0,SL,SL", 129, 96, 50, 3, 3, "fp32"),
    ("F1,PF,PF", 200, 96, 128, 3, 3, "fp32"),
    ("F1,PF,PF", 200, 96, 128, 1, 1, "bf16hi"),
    ("F1,GF,PF", 400, 100, 96, 2, 2, "fp32"),
    ("F1,SL,SL", 77, 80, 50, 7, 7, "fp32"),
    ("F1,PF,PF", 200, 130, 1024, 0, auto_split(200, 130, 1024), "fp32"),      # latency branch
    ("F1,PF,PF", 6016, 768, 2304, 0, auto_split(6016, 768, 2304), "fp32"),    # deep reduction, last-wave fill
    ("F1,PF,PF", 1000, 200, 480, 0, auto_split(1000, 200, 480), "fp32"),      # neither: no split
]
for _c in GENERIC_CASES:
    route(f"generic<{_c[0]}>")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,M,N,K,split,named,mode", GENERIC_CASES)
def test_generic_routes_and_split_k(ops, kind, M, N, K, split, named, mode):
    """descriptors the lean kernel does not take; explicit and automatic K splits (bias / residual enter once,
    the zero fill of a NaN output)"""
    A, B, form = _generic_ops(ops, kind, M, N, K, seed=M + K)
    M = A.o.rows
    d, _ = run(ops, A, B, M, N, form=form, mode=mode, epi=dict(bias=True, res=True, colsum=True), seed=K,
               split_k=split)
    assert last_kernel(ops) == f"generic<{kind}>" + (f" split={named}" if named > 1 else "")
    assert ops.L.lib.f2g_gemm_last_path() == 0
    assert lean_ok(ops, d) == 0, "f2g_gemm_lean_ok accepts a descriptor the generic kernels ran"
    if form == 1 or K % 32:
        assert x6_ok(ops, d) == 0
    if split == 0:
        assert named > 1 or K == 480, "the automatic cases must reach both branches"


# ------------------------------------------------------------------ weight gradients (form 2)
WG_CASES = [   # kind, R, M, N, lean_wgrad, expected
    ("plain", 256, 96, 80, 0, "generic<F2,PF,PF>"),
    ("winB", 256, 64, 96, 0, "generic<F2,PF,GF>"),
    ("plain", 100, 96, 80, 0, "generic<F2,GF,GF>"),
    ("plain", 90, 6, 80, 0, "generic<F2,SL,SL>"),
    ("plain", 3008, 128, 256, 0, "generic<F2,PF,PF>"),
    ("plain", 3008, 128, 256, 1, "generic<F2,PF,PF>"),
    ("plain", 3008, 128, 256, 2, "leanw<bwin=0>"),
    ("plain", 24064, 128, 128, 1, "leanw<bwin=0>"),
    ("plain", 24064, 128, 128, 0, "generic<F2,PF,PF>"),
]
route(*sorted({c[-1] for c in WG_CASES}))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,R,M,N,lw,name", WG_CASES)
def test_weight_gradient_routes(ops, kind, R, M, N, lw, name, lib_option):
    """g[m, n] += sum_r A[r, m] B[r, n], atomic onto a finite output; option lean_wgrad 0 / 1 / 2"""
    lib_option("lean_wgrad", lw)
    A = plain(ops, rnd(R, M, seed=R))
    if kind == "winB":          # padded three-tap windows of 32 channels
        B = win1(ops, rnd(R // 16, 18, N // 3, seed=R + 1), 16, 1, 1, 3)
    else:
        B = plain(ops, rnd(R, N, seed=R + 1))
    d, _ = run(ops, A, B, M, N, form=2, epi=dict(atomic=True), seed=R, split_k=1)
    assert last_kernel(ops) == name
    assert ops.L.lib.f2g_gemm_wgrad_lean(C.byref(d)) == int(name.startswith("leanw"))
    assert x6_ok(ops, d) == 0


def _halo_x(S, Hin, Cin, halo, seed):
    x = torch.zeros(S, Hin + 2 * halo, Cin, device=DEV)
    x[:, halo:halo + Hin] = rnd(S, Hin, Cin, seed=seed)
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("mode,stv,taps,name", [
    ("fp32", 1, 5, route("leanw<bwin=1>")),
    ("bf16x3", 3, 5, route("leanw3<bwin=1>")),
    ("bf16x6", 1, 5, route("leanw6t<step=1>")),
    ("bf16x6", 3, 5, route("leanw6s<step=3>")),
    ("bf16x6", 1, 3, route("leanw6<bwin=1>")),
])
def test_weight_gradient_over_unbounded_windows(ops, mode, stv, taps, name, lib_option):
    """MPD-style weight gradients: windows read past their sequence ends where the gradient map's halo rows are
    zero (f2g_operand.unbounded: exempt from poisoning, the contract allows those reads)"""
    lib_option("lean_wgrad", 2)
    S, Hin, Cin, Cout, HALO = 7, 131, 128, 256, 2
    Hout = (Hin + 4 - taps) // stv + 1
    Hp = Hout + 2 * HALO
    x = _halo_x(S, Hin, Cin, HALO, 1)
    gy = torch.zeros(S, Hp, Cout, device=DEV)
    gy[:, HALO:HALO + Hout] = rnd(S, Hout, Cout, seed=2)
    sp = 1 if mode == "bf16x3" else 0
    L = Hin + 2 * HALO
    B = Op(ops, x.reshape(-1).contiguous(), sp, 0, rows=S * Hp, cols=taps * Cin, P0=Hp, step0=stv,
           pad0=HALO * stv, unit=Cin, L0u=L * Cin, seq_stride=L * Cin, unbounded=1)
    A = Op(ops, gy.reshape(-1).contiguous(), sp, 0, rows=S * Hp, cols=Cout, seq_stride=Cout)
    prec = {"fp32": 0, "bf16x3": 1, "bf16x6": 3}[mode]
    d, _ = run(ops, A, B, Cout, taps * Cin, form=2, mode=mode, epi=dict(atomic=True), seed=5, split_k=1,
               precision=prec)
    assert last_kernel(ops) == name
    if mode == "fp32":
        assert ops.L.lib.f2g_gemm_wgrad_lean(C.byref(d)) == 1
    else:
        assert lean_ok(ops, d) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("mode,name", [("bf16x3", route("leanw3<bwin=0>")), ("bf16x6", route("leanw6<bwin=0>"))])
def test_weight_gradient_split_kernels_plain(ops, mode, name):
    R, M, N = 777, 384, 128
    sp = 1 if mode == "bf16x3" else 0
    A, B = plain(ops, rnd(R, M, seed=1), sp), plain(ops, rnd(R, N, seed=2), sp)
    d, _ = run(ops, A, B, M, N, form=2, mode=mode, epi=dict(atomic=True), seed=3, split_k=1,
               precision=1 if mode == "bf16x3" else 3)
    assert last_kernel(ops) == name
    assert lean_ok(ops, d) == 1


# ------------------------------------------------------------------ deterministic mode
@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in SK_CASES if stream_k_rule(*c[:6])] +
                         [c for c in GENERIC_CASES if c[4] == 0 and c[5] > 1], ids=str)
def test_deterministic_takes_no_split(ops, case, lib_option):
    """deterministic = 1: neither stream-K nor an automatic split; three launches give the same bits (C only:
    column sums stay atomic)"""
    lib_option("deterministic", 1)
    if not isinstance(case[0], str):           # a stream-K case
        M, N, K, mode, streamk, smin, acc = case
        lib_option("streamk", streamk)
        lib_option("streamk_min", smin)
        A, B = mode_ops(ops, mode, rnd(M, K, seed=M), rnd(N, K, seed=N, scale=0.1))
        form, name = 0, f"lean<sk=0,ep=3,pm={MODES[mode][2]}>"
    else:
        kind, M, N, K = case[:4]
        mode = case[6]
        A, B, form = _generic_ops(ops, kind, M, N, K, seed=M + K)
        name = f"generic<{kind}>"
    outs = []
    for _ in range(3):
        _, out = run(ops, A, B, M, N, form=form, mode=mode, epi=dict(bias=True, res=True, colsum=True, scale=1.5),
                     seed=K, split_k=0)
        assert last_kernel(ops) == name
        outs.append(out.flat.clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.gpu
def test_deterministic_from_the_environment():
    env = dict(os.environ, F2G_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, "-c", "from flow2gan_amd import _lib; print(_lib.get_option('deterministic'))"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "1"


# ------------------------------------------------------------------ narrow VALU kernels
NARROW_CASES = [   # form, N, K, M, A kind, epilogue
    (0, 1, 1, 1, "plain", dict(bias=True, lrelu=0.1, scale=2.0, colsum=True)),
    (1, 2, 3, 63, "plain", dict(accumulate=True)),
    (0, 3, 5, 64, "plain", dict(atomic=True, colsum=True)),
    (1, 4, 127, 65, "plain", dict(bias=True, rowmap=True)),
    (0, 4, 96, 1000, "win", dict(bias=True, lrelu=0.2, colsum=True)),
    (1, 3, 96, 1000, "win", dict(scale=0.5, accumulate=True)),
    (0, 2, 127, 1000, "plain", dict(bias=True)),
    (0, 4, 3748, 65, "plain", dict(bias=True)),     # 59 968 bytes of weight panel: still narrow
]
route("narrow_rows<form=0>", "narrow_rows<form=1>")


@pytest.mark.gpu
@pytest.mark.parametrize("form,N,K,M,kind,epi", NARROW_CASES)
def test_narrow_rows(ops, form, N, K, M, kind, epi):
    if kind == "win":           # padded three-tap windows (100 sequences of 10 outputs)
        A = win1(ops, rnd(M // 10, 12, K // 3, seed=K), 10, 1, 1, 3)
    else:
        A = plain(ops, rnd(M, K, seed=K))
    Bx = rnd(N, K, seed=N, scale=0.1)
    B = plain(ops, Bx if form == 0 else Bx.t().contiguous())
    d, _ = run(ops, A, B, A.o.rows, N, form=form, epi=epi, seed=M + N)
    assert last_kernel(ops) == f"narrow_rows<form={form}>"
    assert ops.L.lib.f2g_gemm_last_path() == 3
    assert lean_ok(ops, d) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,epi,name", [
    (4, 3749, dict(bias=True), "generic<F0,SL,SL>"),            # one float past the LDS rule: MFMA tiles
    (5, 96, dict(bias=True), "generic<F0,PF,PF>"),              # five columns
    (3, 96, dict(bias=True, res=True), "generic<F0,PF,PF>"),    # residual: not a narrow epilogue
])
def test_narrow_boundaries_leave_the_narrow_path(ops, N, K, epi, name):
    M = 130
    A, B = plain(ops, rnd(M, K, seed=K)), plain(ops, rnd(N, K, seed=N, scale=0.1))
    d, _ = run(ops, A, B, M, N, epi=epi, seed=K)
    assert last_kernel(ops) == name
    assert lean_ok(ops, d) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,R,name", [
    (1, 256, 65, route("narrow_wgrad4<1>")),
    (1, 4, 1_100_000, "narrow_wgrad4<1>"),          # rows_per clamped at 512
    (3, 64, 1, route("narrow_wgrad4<4>")),
    (4, 4096, 65, "narrow_wgrad4<4>"),
    (2, 6, 1, route("narrow_wgrad")),
    (4, 4097, 300, "narrow_wgrad"),
    (4, 6, 1_100_000, "narrow_wgrad"),
])
def test_narrow_weight_gradients(ops, M, N, R, name):
    A, B = plain(ops, rnd(R, M, seed=R), tail=64), plain(ops, rnd(R, N, seed=N), tail=64)
    run(ops, A, B, M, N, form=2, epi=dict(atomic=True), seed=M + N)
    assert last_kernel(ops) == name
    assert ops.L.lib.f2g_gemm_last_path() == 3


# ------------------------------------------------------------------ the data gradient through the cached transpose
@pytest.mark.gpu
def test_cached_transpose_route(ops, monkeypatch):
    """form 1 against a whole weight Parameter: ops.gemm runs it as a forward GEMM over the cached transpose"""
    monkeypatch.setattr(ops, "GEMM_PRECISION", 0)
    M, K, N = 1000, 128, 130
    a = plain(ops, rnd(M, K, seed=1))
    w = torch.nn.Parameter(rnd(K, N, seed=2, scale=0.1))
    out = torch.full((M, N), NAN, device=DEV)
    ops.gemm(a.o, ops.mat(w), out, form=1, split_k=1)
    torch.cuda.synchronize()
    assert last_kernel(ops) == "lean<sk=0,ep=0,pm=0>"
    acc = a.dense() @ w.detach().double()
    check(out.double(), acc, a.dense().abs() @ w.detach().double().abs(), TOL["fp32"], "dgrad")


# ------------------------------------------------------------------ precision 3 (fp32-class six-product kernels)
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [route("x6f<wimg=0>"), route("x6f<wimg=1>"), route("x6g"), route("x6n"),
                                    route("x6")])
def test_fp32_class_kernels_over_poisoned_operands(ops, kernel, monkeypatch):
    """the precision-3 kernels that read fp32 operands directly: an over-read shows up as NaN"""
    monkeypatch.setattr(ops, "X6_MIN_ROWS", 1)
    monkeypatch.setattr(ops, "X6_MIN_K", 32 if kernel == "x6" else 1 << 20)
    monkeypatch.setattr(ops, "X6F", 0 if kernel == "x6" else 1)
    monkeypatch.setattr(ops, "X6G", kernel == "x6g")
    monkeypatch.setattr(ops, "GEMM_PRECISION", 3)
    M, K = 1001, 96
    N = 32 if kernel == "x6n" else 160
    A = plain(ops, rnd(M, K, seed=1))
    wx = rnd(N, K, seed=2, scale=0.1)
    if kernel == "x6f<wimg=0>":
        B = plain(ops, wx)
        Bop = B.o
        Bop._keep = (B.flat, None, None)
        bd = B.dense()
    else:                           # the weight as a cached image: a whole Parameter
        w = torch.nn.Parameter(wx.clone())
        Bop = ops.mat(w)
        bd = wx.double()
    A.o._keep = (A.flat, None, None)
    bias, res = rnd(N, seed=3), rnd(M, N, seed=4)
    out, cs = Out(M, N), Vec(N, 5)
    # what the precision-3 dispatch reports for the fp32 operands: both operands as images (bit 0) and the fp32
    # tensors as handed over (bit 2), no tap-walking instance (bit 1) for plain matrices
    d = make_desc(ops, A, plain(ops, wx), out, precision=3, bias=bias, res=res, colsum=cs)
    assert x6_ok(ops, d) == 5
    ops.gemm(A.o, Bop, out.view(), bias=bias, res=res, colsum=cs.flat[4:4 + N])
    torch.cuda.synchronize()
    assert last_kernel(ops) == kernel
    assert ops.L.lib.f2g_gemm_last_path() == (5 if kernel == "x6n" else 4)
    out.guards_ok()
    a = A.dense()
    want, m, (cs_want, cs_mag), _ = expect(a @ bd.t(), a.abs() @ bd.abs().t(), bias=bias, res=res)
    check(out.got(), want, m, TOL["bf16x6"], kernel)
    check(cs.got(), cs.init.double() + cs_want, cs_mag + cs.init.double().abs(), TOL["bf16x6"], "colsum")


@pytest.mark.gpu
@pytest.mark.parametrize("taps", [route("x6p<taps=5>") and 5, route("x6p<taps=2>") and 2])
def test_fp32_class_tap_walking_kernel(ops, taps, monkeypatch, lib_option):
    """gemm_x6p_kernel over the three-piece image of a map (stride-1 windows), option x6p = 2"""
    lib_option("x6p", 2)
    monkeypatch.setattr(ops, "X6_MIN_ROWS", 1)
    monkeypatch.setattr(ops, "X6_MIN_K", 32)
    monkeypatch.setattr(ops, "X6F", 0)
    monkeypatch.setattr(ops, "GEMM_PRECISION", 3)
    S, P0, Cc, N = 5, 64, 64, 128
    Hp = P0 + taps - 1
    x = rnd(S, Hp, Cc, seed=taps)
    flat = torch.full((S * Hp * Cc + 256 * Cc,), NAN, device=DEV)
    flat[:S * Hp * Cc] = x.reshape(-1)
    A = ops.win1d(flat, S, Hp, Cc, P0, 1, 0, taps)
    w = torch.nn.Parameter(rnd(N, taps * Cc, seed=7, scale=0.1))
    bias = rnd(N, seed=8)
    out = torch.full((S * P0, N), NAN, device=DEV)
    d = make_desc(ops, A, ops.mat(w), Out(S * P0, N), precision=3, bias=bias, lrelu=0.1)
    assert x6_ok(ops, d) & 3 == 3, "f2g_gemm_x6_ok does not report the tap-walking instance"
    ops.gemm(A, ops.mat(w), out, bias=bias, lrelu=0.1)
    torch.cuda.synchronize()
    assert last_kernel(ops) == f"x6p<taps={taps}>"
    a = torch.stack([x[:, i:i + P0] for i in range(taps)], 2).reshape(S * P0, taps * Cc).double()
    want, m, _, _ = expect(a @ w.detach().double().t(), a.abs() @ w.detach().double().abs().t(), bias=bias,
                           lrelu=0.1)
    check(out.double(), want, m, TOL["bf16x6"], "x6p")


# ------------------------------------------------------------------ fused inference kernels: library options
def fused_last(ops):
    return ops.L.lib.f2g_fused_last_launch().decode()


def _mlp_operands(ops, C, rows, seed):
    """bf16 z, packed weights, biases, PReLU slopes, residual; the float64 result of the same arithmetic (bf16
    operands, the hidden activation rounded to bf16)"""
    H = 3 * C
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, C, generator=gen).to(torch.bfloat16).to(DEV)
    w1 = (torch.randn(H, C, generator=gen) * 0.05).to(DEV)
    w2 = (torch.randn(C, H, generator=gen) * 0.03).to(DEV)
    b1 = (torch.randn(H, generator=gen) * 0.1).to(DEV)
    al = (0.25 + 0.2 * torch.randn(H, generator=gen)).to(DEV)
    b2 = (torch.randn(C, generator=gen) * 0.1).to(DEV)
    x = torch.randn(rows, C, generator=gen).to(DEV)
    gam = (0.5 + torch.rand(C, generator=gen)).to(DEV)
    a = z.double() @ w1.to(torch.bfloat16).double().t() + b1.double()
    pz = (a.clamp(min=0) + al.double() * a.clamp(max=0)).float().to(torch.bfloat16)
    want = pz.double() @ w2.to(torch.bfloat16).double().t() + b2.double() + gam.double() * x.double()
    return (z, ops.mlp_pack(w1, w2), b1, al, b2, x, gam), want, H


def _fused_close(got, want, what):
    assert torch.isfinite(got).all(), what
    scale = float(want.abs().max())
    assert float((got.double() - want).abs().max()) < 2e-3 * scale, what
    assert float((got.double() - want).pow(2).mean().sqrt()) < 1e-4 * scale, what


def mlp_rt_rule(C, v):
    """fusedmlp.hip: pick_rt with option mlp_rt = v > 0 -- capped at what the accumulators hold, 3 -> 2 at C = 384"""
    r = min(v, {768: 2, 512: 3, 384: 4}[C])
    return 2 if (C == 384 and r == 3) else r


@pytest.mark.gpu
@pytest.mark.parametrize("C", [384, 512, 768])
@pytest.mark.parametrize("v", [1, 2, 3, 4])
def test_fused_mlp_tile_option(ops, C, v, lib_option):
    """option mlp_rt forces the rows per tile of f2g_fused_mlp / f2g_fused_block, with its clamps"""
    lib_option("mlp_rt", v)
    rows = 300
    args, want, H = _mlp_operands(ops, C, rows, seed=C + v)
    out = torch.full((rows, C), NAN, device=DEV)
    ops.fused_mlp(args[0], args[1], *args[2:6], args[6], out, rows, C, H)
    torch.cuda.synchronize()
    assert fused_last(ops) == f"fused_mlp<rt={mlp_rt_rule(C, v)},parts=1>"
    _fused_close(out, want, f"mlp_rt={v}")


def mlp_parts_rule(S, option, parts):
    """fusedmlp.hip: launch_fused -- blocks per row tile along the S hidden slabs (the call's `parts` first)"""
    forced = parts if parts > 0 else option
    J = min(max(forced if forced > 0 else 1, 1), S)
    spb = -(-S // J)
    return -(-S // spb)


@pytest.mark.gpu
@pytest.mark.parametrize("option,parts", [(0, 0), (1, 0), (2, 0), (5, 0), (5, 3), (0, 2), (1, 5), (2, 1)])
def test_fused_mlp_split_option(ops, option, parts, lib_option):
    """option mlp_split against the per-call `parts`: partial tiles added atomically onto the zeroed output"""
    lib_option("mlp_split", option)
    C, rows = 512, 200
    args, want, H = _mlp_operands(ops, C, rows, seed=option * 10 + parts)
    out = torch.full((rows, C), NAN, device=DEV)
    ops.fused_mlp(args[0], args[1], *args[2:6], args[6], out, rows, C, H, parts=parts)
    torch.cuda.synchronize()
    assert fused_last(ops).endswith(f",parts={mlp_parts_rule(H // 128, option, parts)}>"), fused_last(ops)
    _fused_close(out, want, f"mlp_split={option}, parts={parts}")


def _block_entries(ops):
    """the entries of test_fused_block_multi_equals_separate_launches (tests/test_hip_ops.py): not in cost order,
    ragged row counts, one entry without condition / time inputs"""
    B, K = 3, 7
    gen = torch.Generator().manual_seed(11)
    entries = []
    for C, Fr, up, cond in ((384, 94, 4, True), (768, 23, 1, True), (512, 47, 2, False), (768, 5, 1, True)):
        H = 3 * C
        Fc = (Fr + up - 1) // up
        NC = 2 * C
        e = dict(x=torch.randn(B * Fr, C, generator=gen).to(DEV), B=B, F=Fr, Cc=C, K=K,
                 lens=torch.tensor([Fr, max(1, Fr - 4), max(1, Fr // 2)]).int().to(DEV),
                 w_dw=(torch.randn(C, 1, K, generator=gen) * 0.3).to(DEV),
                 b_dw=(torch.randn(C, generator=gen) * 0.1).to(DEV), beta=(torch.randn(C, generator=gen) * 0.1).to(DEV),
                 log_scale=torch.tensor([0.6]).to(DEV),
                 wp=ops.mlp_pack((torch.randn(H, C, generator=gen) * 0.05).to(DEV),
                                 (torch.randn(C, H, generator=gen) * 0.03).to(DEV)),
                 b1=(torch.randn(H, generator=gen) * 0.1).to(DEV), alpha=(0.25 + 0.2 * torch.randn(H, generator=gen)).to(DEV),
                 b2=(torch.randn(C, generator=gen) * 0.1).to(DEV), gamma=(0.5 + torch.rand(C, generator=gen)).to(DEV),
                 out=torch.full((B * Fr, C), NAN, device=DEV), Hh=H)
        if cond:
            e.update(cproj=torch.randn(B * Fc, NC, generator=gen).to(DEV), ldcp=NC, Fc=Fc, up=up, cp_off=C // 2,
                     te=(torch.randn(B, NC, generator=gen) * 0.3).to(DEV), ldte=NC, te_off=C // 2)
        entries.append(e)
    return entries


@pytest.mark.gpu
@pytest.mark.parametrize("rt384", [2, 4])
@pytest.mark.parametrize("rt512", [2, 3])
def test_fused_block_multi_tile_options(ops, rt384, rt512, lib_option):
    """options multi_rt384 / multi_rt512: 64-row tiles for the cheaper entries of f2g_fused_block_multi (the
    768-channel entries keep theirs), each entry against its own f2g_fused_block launch"""
    entries = _block_entries(ops)
    wants = []
    for e in entries:
        want = torch.empty_like(e["out"])
        ops.fused_block(e["x"], e["B"], e["F"], e["Cc"], e["K"], e["lens"], e["w_dw"], e["b_dw"], e["beta"],
                        e["log_scale"], e["wp"], e["b1"], e["alpha"], e["b2"], e["gamma"], want, e["Hh"],
                        e.get("cproj"), e.get("ldcp", 0), e.get("Fc", 0), e.get("up", 1), e.get("cp_off", 0),
                        e.get("te"), e.get("ldte", 0), e.get("te_off", 0))
        wants.append(want)
    lib_option("multi_rt384", rt384)
    lib_option("multi_rt512", rt512)
    outs = ops.fused_block_multi(entries)
    torch.cuda.synchronize()
    rts = [{384: 2 if rt384 == 2 else 4, 512: 2 if rt512 == 2 else 3, 768: 2}[e["Cc"]] for e in entries]
    assert fused_last(ops) == "fused_block_multi<rt=" + ",".join(map(str, rts)) + ">"
    for e, got, want in zip(entries, outs, wants):
        # (the same arithmetic row by row; another tile height is another kernel instance, whose z prologue may
        # round differently: the bounds of test_fused_block_multi_equals_separate_launches)
        assert torch.isfinite(got).all(), e["Cc"]
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) < 2e-3 * scale, (e["Cc"], e["F"])
        assert float((got - want).pow(2).mean().sqrt()) < 2e-5 * scale, (e["Cc"], e["F"])


# ------------------------------------------------------------------ ledger
def kernel_literals():
    """every kernel name f2g_gemm_last_kernel can report: the string literals handed to f2g_note_kernel (directly
    or through the name tables of f2g_launch_lean / generic_name)"""
    names = set()
    for fn in os.listdir(os.path.join(ROOT, "flow2gan_amd", "csrc")):
        if not fn.endswith((".hip", ".h")) or fn == "capi.hip":      # (capi.hip: the option table's names)
            continue
        src = open(os.path.join(ROOT, "flow2gan_amd", "csrc", fn)).read()
        names |= set(re.findall(r'"((?:lean|lean_tall|lean_tap|leanw\d?|leanw6[ts]|x6[fgnp]?|narrow_\w+|generic)'
                                r'(?:<[^"<>]*>)?)"', src))
    return names


def test_route_ledger_names_every_kernel_instance():
    """CPU: a kernel instance added to the dispatch without a case in this module turns the suite red"""
    lits = kernel_literals()
    assert len(lits) >= 50, sorted(lits)
    assert "lean<sk=1,ep=3,pm=0>" in lits and "generic<F1,GF,PF>" in lits and "narrow_wgrad" in lits
    missing = sorted(lits - ROUTES)
    assert not missing, f"kernel instances without a route case: {missing}"
    stale = sorted(ROUTES - lits)
    assert not stale, f"route cases naming no kernel of csrc/: {stale}"

