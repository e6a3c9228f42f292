"""What two or more of the fp16x3 GPU test files (tests/test_hip_gemm_f16*.py, tests/test_hip_conv3*_f16*.py) share:
the library fixture, the mode fixture's body, the refusal check, the watch over launched descriptors, the "cached
image follows its weight" sequence, one sub-discriminator and a generator's stage-1 step against the CPU oracle, and
the operand builders that more than one file launches.  What belongs to one kernel stays in that kernel's file.

A plain module: pytest rewrites `assert` in test modules and conftests only, so every assert here says what it
compared and the values it found."""
import contextlib
import ctypes as C
import math
import random
import types

import pytest
import torch

from fp16x3_emul import FLOOR
from test_hip_gemm_routes import DEV, NAN, SENT, Op, _halo_x, last_kernel, plain, products, rnd

TOL = 1.8e-6        # per element, of |A| |B|^T + |epilogue terms|: the suite's 1e-6 for exact-class fp32 accumulation
                    # plus the arithmetic's 3 * 2^-22 = 7.2e-7 per product
EINVAL = -1
HALO = 2            # zero halo rows either side of a sequence of an MPD map
TINY = dict(sampling_rate=24000, n_mels=100, mel_n_fft=1024, mel_hop_length=256,
            n_ffts=(512, 256, 128), hop_lengths=(256, 128, 64), channels=(64, 32, 32),
            time_embed_channels=32, hidden_factor=3, num_layers=(2, 1, 1),
            cond_enc_channels=32, cond_enc_num_layers=1)


def library():
    """flow2gan_amd.ops; skips without a GPU"""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from flow2gan_amd import ops as o
    return o


@pytest.fixture(scope="module")
def ops():
    return library()


@pytest.fixture
def any_grid(lib_option):
    """library option x6p = 2: the tap-walking kernels take grids that do not fill the chip"""
    lib_option("x6p", 2)


def mode_name(ops):
    return "fp16x3" if ops.FP16X3 else {0: "fp32", 1: "bf16x3", 2: "bf16", 3: "bf16x6"}[ops.GEMM_PRECISION]


@contextlib.contextmanager
def fp16x3_mode(ops, *names):
    """the fp16x3 mode; the tunables `names` (which the caller assigns) and the mode are restored afterwards"""
    was, vals = mode_name(ops), [getattr(ops, n) for n in names]
    ops.set_gemm_precision("fp16x3")
    try:
        yield ops
    finally:
        for n, v in zip(names, vals):
            setattr(ops, n, v)
        ops.set_gemm_precision(was)


def f16_ok(ops, d):
    return ops.L.lib.f2g_gemm_f16_ok(C.byref(d))


def ran(ops, kernel_name):
    """the last launch was `kernel_name`, through the fp16x3 table"""
    return last_kernel(ops) == kernel_name and ops.L.lib.f2g_gemm_last_path() == 6


def assert_declined(ops, d, out, ok=0):
    """f2g_gemm_f16_ok == ok (0: never; 2: "would run once the operands are replaced by their images") and F2G_EINVAL
    from f2g_gemm -- never another kernel; the output `out` (test_hip_gemm_routes.Out) stays untouched"""
    answer = f16_ok(ops, d)
    assert answer == ok, f"f2g_gemm_f16_ok answered {answer} for a descriptor it must answer {ok} for"
    rc = ops.L.lib.f2g_gemm(C.byref(d), ops.L.stream_ptr())
    assert rc == EINVAL, f"f2g_gemm returned {rc} for a descriptor it must refuse with F2G_EINVAL ({EINVAL})"
    torch.cuda.synchronize()
    kernel = last_kernel(ops)
    assert kernel == "", f"a refused launch ran {kernel!r}"
    written = out.flat[~torch.isnan(out.flat)] != SENT
    assert not bool(written.any()), f"a refused launch wrote {int(written.sum())} floats of its output"


@contextlib.contextmanager
def watching_gemm_calls(ops, monkeypatch, *image_builders):
    """(seen, images): of every f2g_gemm launched inside the block (A.base, A.split, bool(A.rscale), B.split,
    bool(B.rscale)) as the descriptor is launched, and the arguments of every call of ops.<image_builders>"""
    seen, images = [], []
    real_call = ops.call

    def watch_call(name, *args):
        if name == "f2g_gemm":
            d = args[0]._obj                # (C.byref's object: the descriptor as it is launched)
            seen.append((d.A.base, d.A.split, bool(d.A.rscale), d.B.split, bool(d.B.rscale)))
        return real_call(name, *args)

    def watching(real):
        def watch_image(*args, **kw):
            images.append(args)
            return real(*args, **kw)
        return watch_image

    with monkeypatch.context() as mp:
        mp.setattr(ops, "call", watch_call)
        for name in image_builders:
            mp.setattr(ops, name, watching(getattr(ops, name)))
        yield seen, images


def same_bits(launch, n=3):
    """launch() -- which returns the int32 words it wrote -- gives the same bits n times"""
    bits = [launch() for _ in range(n)]
    for i, b in enumerate(bits[1:], 1):
        assert torch.equal(bits[0], b), f"launch {i} differs from launch 0 in {int((bits[0] != b).sum())} words"


def scale_rows(w):
    """the raw-pointer rewrite of a weight: every output row by its own factor over six decades (the row scales of
    its image must move too)"""
    factors = torch.logspace(-3, 3, w.shape[0], device=w.device)
    w.data.copy_(w.detach() * factors.view(-1, *([1] * (w.dim() - 1))))


def image_follows_weight(ops, w, launch_and_check, *, update=scale_rows, min_replays=1):
    """after a raw-pointer update (the optimizer's way: `update(w)`, invisible to autograd, then bump_weight_epoch + the
    batched rebuild_derived) and after an autograd-visible in-place update, the next launch reads a rebuilt image and
    rebuilt scales.  launch_and_check(what) launches, holds the result and the cached image to their references and
    returns the tensor (or tuple of tensors) the launch wrote, every one of which must move with the weight."""
    def moved(before, after, what):
        before, after = (t if isinstance(t, tuple) else (t,) for t in (before, after))
        for i, (b, a) in enumerate(zip(before, after)):
            assert not torch.equal(b, a), f"output {i} is bit for bit what it was before {what}"

    first = launch_and_check("first launch")
    version = w._version
    update(w)
    assert w._version == version, \
        f"the raw-pointer update moved _version from {version} to {w._version}: autograd saw it, not the epoch alone"
    ops.bump_weight_epoch([w])
    replayed = ops.rebuild_derived([w])
    assert replayed >= min_replays or not ops.EAGER_REBUILD, \
        f"rebuild_derived replayed {replayed} derived tensors, expected at least {min_replays}"
    second = launch_and_check("after the raw-pointer update")
    moved(first, second, "the raw-pointer update")
    with torch.no_grad():
        w.mul_(-0.37)
    third = launch_and_check("after the in-place update")
    moved(second, third, "the in-place update")


def subdisc_against_oracle(ops, kind, counters, label):
    """The first sub-discriminator of the "mpd" or "mrd" at the shapes of tests/test_hip_disc_autograd.py: score,
    feature maps, input gradient and every parameter gradient against the oracle at that file's tolerance
    (T._compare under `label`).  Returns sub (the HIP sub-discriminator), fwd and bwd (by how much each of the ops
    counters named in `counters` moved in the forward and in the backward pass) and rerun(), which runs the HIP side
    again -- after the caller switched its route off, say -- and returns fresh (fwd, bwd)."""
    import test_hip_disc_autograd as T
    do, dh = T._models(kind)
    sub_o, sub_h = do.discriminators[0], dh.discriminators[0]
    _, y_hat = T._inputs()

    def loss_of(score, fmap):
        gen = torch.Generator().manual_seed(77)
        loss = torch.relu(1 + score).mean()
        for m in fmap:
            loss = loss + (m * torch.randn(m.shape, generator=gen).to(m.device)).sum() / math.sqrt(m.numel())
        return loss

    def count():
        return [getattr(ops, n) for n in counters]

    def hip_run():
        for p in sub_h.parameters():
            p.grad = None
        yh = y_hat.to(DEV).requires_grad_(True)
        n0 = count()
        score, fmap = sub_h(yh)
        n1 = count()
        loss_of(score, fmap).backward()
        torch.cuda.synchronize()
        n2 = count()
        return score, fmap, yh.grad, tuple(b - a for a, b in zip(n0, n1)), tuple(b - a for a, b in zip(n1, n2))

    score, fmap, gx, fwd, bwd = hip_run()
    sides = T._hip_sides(types.SimpleNamespace(discriminators=[sub_h]), kind, y_hat.to(DEV))[0]
    yo = y_hat.clone().requires_grad_(True)
    do.zero_grad(set_to_none=True)
    so, fo = T._with_sides(sides, lambda: sub_o(yo))
    loss_of(so, fo).backward()
    pairs = [("score", score, so.detach())] + [(f"fmap.{i}", m, fo[i].detach()) for i, m in enumerate(fmap)]
    pairs += [("y_hat", gx, yo.grad)]
    pairs += [(k, p.grad, dict(sub_o.named_parameters())[k].grad) for k, p in sub_h.named_parameters()]
    do.zero_grad(set_to_none=True)
    T._compare(pairs, label)
    return types.SimpleNamespace(sub=sub_h, fwd=fwd, bwd=bwd, rerun=lambda: hip_run()[3:])


def stage1_against_oracle(ops, counters, infer=False):
    """A generator's stage-1 step -- the construction of test_hip_generator.py::test_stage1_against_oracle_other_shape
    (B = 3, odd T) with the TINY widths, whose pointwise reductions are all multiples of 32 -- against the CPU oracle at
    that test's tolerances: the loss to 2e-5, every parameter gradient to 2e-3 of the oracle's largest; with `infer`,
    4-step inference to 1e-4 RMS.  Returns fwd, bwd (and inf): by how much each of the ops counters named in `counters`
    moved in the forward pass, the backward pass (and the inference)."""
    import flow2gan_amd as f2g
    import flow2gan_oracle as O
    torch.manual_seed(3)
    mo = O.MelAudioGenerator(**TINY).train()
    mh = f2g.MelAudioGenerator(**TINY)
    mh.load_state_dict(mo.state_dict())
    mh = mh.to(DEV).train()
    mo.branch_dropout = mh.branch_dropout = 0.0
    gen = torch.Generator().manual_seed(4)
    B, Tn = 3, 5120
    audio = 0.1 * torch.randn(B, Tn, generator=gen)
    lens = torch.tensor([5120, 3000, 4097])
    mel = O.LogMelSpectrogram()(audio)
    noise = 0.1 * torch.randn(B, Tn, generator=gen)
    t = torch.tensor([[0.1], [0.5], [0.9]])

    def count():
        return [getattr(ops, n) for n in counters]

    def moved(a, b):
        return tuple(y - x for x, y in zip(a, b))

    st = random.getstate()
    random.seed(5)
    lo = mo(mel, audio, lens, noise=noise, t=t)
    lo.backward()
    random.setstate(st)
    random.seed(5)
    n0 = count()
    lh = mh(mel.to(DEV), audio.to(DEV), lens, noise=noise.to(DEV), t=t.to(DEV))
    n1 = count()
    lh.backward()
    n2 = count()
    random.setstate(st)
    res = types.SimpleNamespace(fwd=moved(n0, n1), bwd=moved(n1, n2))
    print(f"launches per counter {counters}: forward {res.fwd}, backward {res.bwd}; "
          f"loss {float(lh):.7f} oracle {float(lo):.7f}")
    assert abs(float(lh) - float(lo)) < 2e-5 * abs(float(lo)), f"loss {float(lh)!r} against the oracle's {float(lo)!r}"
    po = dict(mo.named_parameters())
    missing = [n for n, p in mh.named_parameters() if p.grad is None]
    assert not missing, f"parameters without a gradient: {missing}"
    errs = sorted(((float((p.grad.cpu() - po[n].grad).abs().max()) / (float(po[n].grad.abs().max()) + 1e-12), n)
                   for n, p in mh.named_parameters()), reverse=True)
    print("worst gradients:", errs[:3])
    assert errs[0][0] < 2e-3, f"parameter gradients off by more than 2e-3 of the oracle's largest: {errs[:8]}"
    if infer:
        mo.eval(), mh.eval()
        with torch.no_grad():
            nz = 0.1 * torch.randn(B, mel.shape[2] * 256, generator=gen)
            yo = mo.infer(mel, None, 4, True, noise=nz)
            n3 = count()
            yh = mh.infer(mel.to(DEV), None, 4, True, noise=nz.to(DEV))
        res.inf = moved(n3, count())
        err = float((yh.cpu().double() - yo.double()).pow(2).mean().sqrt())
        print(f"infer: launches per counter {res.inf}, rms {err:.3e}")
        assert err <= 1e-4, f"4-step inference: rms {err:.3e} against the oracle, more than 1e-4"
    return res


# ------------------------------------------------------------------ operands of the pointwise kernels
def as_image(ops, op):
    """replace the fp32 operand `op` (test_hip_gemm_routes.Op over a NaN-poisoned buffer) by its f2g_split_f16x2
    image: a copy of the buffer -- poison included -- whose rows' K columns the split kernel rewrote"""
    o = op.o
    op.img = op.flat.clone()
    op.rs = torch.full((o.rows + 8,), NAN, device=DEV)
    ops.call("f2g_split_f16x2", op.img.data_ptr() + 4 * op.off, op.rs.data_ptr() + 16,
             op.flat.data_ptr() + 4 * op.off, o.seq_stride, o.rows, o.cols)
    o.base, o.split, o.rscale = op.img.data_ptr() + 4 * op.off, 5, op.rs.data_ptr() + 16
    return op


def cached_image(ops, w):
    """(int32 words (rows, K), reciprocal scales (rows,)) of the f2g_split_f16x2 image the derived-weight cache holds
    of the weight w, on the CPU"""
    o = ops._f16_operand(ops.mat(w))
    rows, K = w.shape
    buf = o._keep[0]
    torch.cuda.synchronize()
    return buf[:rows * K].cpu().view(torch.int32).view(rows, K), buf[rows * K:rows * K + rows].cpu()


# ------------------------------------------------------------------ operands of the tap-walking forward kernels
def seq_image(ops, op, nseq, run, ld):
    """replace the fp32 operand `op` (test_hip_gemm_routes.Op over a NaN-poisoned buffer) by its f2g_split_f16x2_seq
    image: a copy of the buffer -- poison included -- whose runs the image routine rewrote"""
    op.img = op.flat.clone()
    op.rs = torch.full((nseq + 8,), NAN, device=DEV)
    ops.call("f2g_split_f16x2_seq", op.img.data_ptr() + 4 * op.off, op.rs.data_ptr() + 16,
             op.flat.data_ptr() + 4 * op.off, ld, nseq, run)
    op.o.base, op.o.split, op.o.rscale = op.img.data_ptr() + 4 * op.off, 7, op.rs.data_ptr() + 16
    return op


def halo_windows(ops, x, P0, taps, step=1):
    """stride-`step` windows of `taps` positions over the contiguous map x (S, Hp, C), NaN behind the last sequence"""
    S, Hp, Cc = x.shape
    flat = torch.full((S * Hp * Cc + 256 * Cc,), NAN, device=DEV)
    flat[:S * Hp * Cc] = x.reshape(-1)
    return Op(ops, flat, 0, 0, rows=S * P0, cols=taps * Cc, P0=P0, step0=step, pad0=0, unit=Cc, L0u=Hp * Cc,
              seq_stride=Hp * Cc)


def case(ops, S, P0, Cc, N, taps, seed=0, step=1, extra=0, images=True):
    """A (windows over a map whose sequences span 60 decades: a scale taken from the wrong sequence is wrong by
    orders of magnitude), B (the weights), the floor term of every output -- the per-sequence scale's 2^-28
    amax_seq(row) sum_k |w[n,k]|, carried like a product's scale -- float64 products and their scale"""
    Hp = step * (P0 - 1) + taps + extra
    x = rnd(S, Hp, Cc, seed=seed + taps) * torch.logspace(-30, 30, S, device=DEV)[:, None, None]
    w = rnd(N, taps * Cc, seed=seed + 50, scale=(taps * Cc) ** -0.5)
    A = halo_windows(ops, x, P0, taps, step)
    B = plain(ops, w, pad=0)
    if images:
        seq_image(ops, A, S, Hp * Cc, Hp * Cc)
        seq_image(ops, B, N, taps * Cc, B.o.seq_stride)
    amax = x.double().abs().reshape(S, -1).amax(1).repeat_interleave(P0)
    floor = FLOOR * amax[:, None] * w.double().abs().sum(1)[None, :]
    acc, mag = products(A, B, 0, False)
    return types.SimpleNamespace(A=A, B=B, x=x, w=w, acc=acc, mag=mag + floor / TOL, M=S * P0, N=N, Hp=Hp)


# ------------------------------------------------------------------ operands of the weight-gradient kernels
def as_cols_image(ops, op):
    """replace the fp32 operand `op` (test_hip_gemm_routes.Op over a NaN-poisoned buffer) by its column image: a copy
    of the buffer -- poison included -- whose rows' columns f2g_split_f16x2_cols rewrote"""
    o = op.o
    op.img = op.flat.clone()
    op.rs = torch.full((o.cols + 8,), NAN, device=DEV)
    op.work = torch.empty(o.cols, device=DEV, dtype=torch.int32)
    ops.call("f2g_split_f16x2_cols", op.img.data_ptr() + 4 * op.off, op.rs.data_ptr() + 16, op.work.data_ptr(),
             op.flat.data_ptr() + 4 * op.off, o.seq_stride, o.rows, o.cols)
    o.base, o.split, o.rscale = op.img.data_ptr() + 4 * op.off, 6, op.rs.data_ptr() + 16
    return op


def as_cols_window_image(ops, op):
    """replace the fp32 window operand `op` by the f2g_split_f16x2_cols image of its WHOLE map (xrows x unit floats,
    halo rows included); the window fields stay as they are"""
    o = op.o
    xrows = (o.rows // o.P0) * (o.seq_stride // o.unit)
    op.img = op.flat.clone()
    op.rs = torch.full((o.unit + 8,), NAN, device=DEV)
    op.work = torch.empty(o.unit, device=DEV, dtype=torch.int32)
    ops.call("f2g_split_f16x2_cols", op.img.data_ptr() + 4 * op.off, op.rs.data_ptr() + 16, op.work.data_ptr(),
             op.flat.data_ptr() + 4 * op.off, o.unit, xrows, o.unit)
    o.base, o.split, o.rscale = op.img.data_ptr() + 4 * op.off, 6, op.rs.data_ptr() + 16
    return op


def hout_of(Hin):
    """rows out of conv(k = 5, stride = 3, padding = 2)"""
    return (Hin - 1) // 3 + 1


def maps(Cin, Cout, S, Hin, seed, extra=0):
    """a stride-3 layer's input halo map x (S, Hin + 4 + extra, Cin) and gradient map (S, Hout + 4, Cout), zero halo
    rows"""
    Hout = hout_of(Hin)
    x = torch.zeros(S, Hin + 2 * HALO + extra, Cin, device=DEV)
    x[:, HALO:HALO + Hin] = rnd(S, Hin, Cin, seed=seed)
    gy = torch.zeros(S, Hout + 2 * HALO, Cout, device=DEV)
    gy[:, HALO:HALO + Hout] = rnd(S, Hout, Cout, seed=seed + 1)
    return x, gy


def maps_s1(Cin, Cout, S, Hin, seed):
    """a stride-1 layer's halo map x (S, Hp, Cin) and gradient map (S, Hp, Cout), both with zero halo rows"""
    Hp = Hin + 2 * HALO
    x = _halo_x(S, Hin, Cin, HALO, seed)
    gy = torch.zeros(S, Hp, Cout, device=DEV)
    gy[:, HALO:HALO + Hin] = rnd(S, Hin, Cout, seed=seed + 1)
    return x, gy


def operands(ops, x, gy, images=True, step=3, taps=5, pad0=3 * HALO):
    """A: the gradient as a plain matrix inside a NaN buffer; B: unbounded windows of `taps` positions, `step` apart,
    over the map; images: both replaced by their column images"""
    S, HpIn, Cin = x.shape
    Hp, Cout = gy.shape[1], gy.shape[2]
    A = plain(ops, gy.reshape(S * Hp, Cout))
    B = Op(ops, x.reshape(-1).contiguous(), 0, 0, rows=S * Hp, cols=taps * Cin, P0=Hp, step0=step, pad0=pad0,
           unit=Cin, L0u=HpIn * Cin, seq_stride=HpIn * Cin, unbounded=1)
    if images:
        as_cols_image(ops, A)
        as_cols_window_image(ops, B)
    return A, B


def operands_s1(ops, x, gy, images=True, step=1, taps=5):
    """operands() over a stride-1 layer's maps (maps_s1: Hp rows in both): pad0 = 2 `step`"""
    return operands(ops, x, gy, images, step, taps, pad0=HALO * step)
