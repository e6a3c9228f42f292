"""Differentiable discriminator modules (leaf.DiscPFn / DiscRFn): the f2g_lrelu_bwd_add kernel against float64
torch, gradients of a caller-built loss against the CPU oracle run with the HIP path's leaky-ReLU sides,
selective work, consistency with the fused D-step, and the no-grad behaviour."""
import collections
import ctypes
import math
import types

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gemm_mode_exact")]
DEV = "cuda"
SLOPE = 0.1
GRAD_TOL = 5e-3       # of each tensor's max |want|, no absolute floor (tests/test_hip_gan.py's kink-resolved bound)

TINY = dict(sampling_rate=24000, n_mels=100, mel_n_fft=1024, mel_hop_length=256,
            n_ffts=(512, 256, 128), hop_lengths=(256, 128, 64), channels=(48, 32, 24),
            time_embed_channels=32, hidden_factor=3, num_layers=(2, 2, 2),
            cond_enc_channels=32, cond_enc_num_layers=1)


@pytest.fixture(scope="module")
def f2g():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import flow2gan_amd
    return flow2gan_amd


# ====================================================================================== the kernel
HALO = 2


def _kernel_case(layout, C):
    """-> (buffer shape, view of the valid region as (n0, n1, n2, C), dims, g strides, g_off, upstream shape,
    permutation taking the (B, C, h, w) upstream to (n0, n1, n2, C))."""
    if layout == "mpd":                     # halo layout: (B*p sequences) x (H + 2*HALO rows) x C
        B, p, H = 2, 3, 5
        Hp = H + 2 * HALO
        shape = (B, p, Hp, C)
        region = (slice(None), slice(None), slice(HALO, HALO + H))
        return shape, region, (B, p, H), (p * Hp * C, Hp * C, C), HALO * C, (B, C, H, p), (0, 3, 2, 1)
    B, Ft, W = 2, 3, 7
    if layout == "mrd":                     # contiguous (B, Ft, W, C)
        return (B, Ft, W, C), (slice(None),) * 3, (B, Ft, W), (Ft * W * C, W * C, C), 0, (B, C, Ft, W), (0, 2, 3, 1)
    Wcat, foff = 11, 3                      # a band's slice of the concatenated map
    return ((B, Ft, Wcat, C), (slice(None), slice(None), slice(foff, foff + W)), (B, Ft, W),
            (Ft * Wcat * C, Wcat * C, C), foff * C, (B, C, Ft, W), (0, 2, 3, 1))


def _upstream(kind, ushape, gen):
    B, C, h, w = ushape
    if kind == "contiguous":
        return torch.randn(ushape, generator=gen).to(DEV)
    if kind == "channels_last":             # non-contiguous view: channel stride 1, no unit position stride
        return torch.randn(B, h, w, C, generator=gen).to(DEV).permute(0, 3, 1, 2)
    if kind == "batch_swapped":             # non-contiguous view that keeps the unit position stride
        return torch.randn(C, B, h, w, generator=gen).to(DEV).permute(1, 0, 2, 3)
    assert kind == "expanded"               # what .sum().backward() hands over: every stride 0
    return torch.tensor(0.37, device=DEV).expand(ushape)


@pytest.mark.parametrize("kind", ["contiguous", "channels_last", "batch_swapped", "expanded"])
@pytest.mark.parametrize("layout", ["mpd", "mrd", "slice"])
@pytest.mark.parametrize("C", [32, 128])
def test_lrelu_bwd_add_kernel(f2g, C, layout, kind):
    from flow2gan_amd import ops
    gen = torch.Generator().manual_seed(1000 + C + len(layout) + len(kind))
    shape, region, dims, gstr, g_off, ushape, perm = _kernel_case(layout, C)
    g0 = torch.randn(shape, generator=gen).to(DEV)          # (halo rows / foreign columns hold values too)
    y = torch.randn(shape, generator=gen).to(DEV)
    u = _upstream(kind, ushape, gen)
    if kind != "contiguous":
        assert not u.is_contiguous()
    ub, uc, uh, uw = u.stride()
    ustr = (ub, uw, uh, uc) if layout == "mpd" else (ub, uh, uw, uc)
    want = (g0[region].double() + u.permute(perm).double()) * torch.where(y[region] > 0, 1.0, SLOPE).double()
    inside = torch.zeros(shape, dtype=torch.bool, device=DEV)
    inside[region] = True
    for with_colsum in (True, False):
        g = g0.clone()
        cs = ops.zeros(C, device=DEV) if with_colsum else None
        ops.lrelu_bwd_add(g, y, dims, gstr, C, u, ustr, SLOPE, colsum=cs, g_off=g_off)
        torch.cuda.synchronize()
        got = g[region].double()
        err = (got - want).abs()
        assert bool((err <= 1e-6 * want.abs()).all()), (with_colsum, float((err / want.abs().clamp_min(1e-30)).max()))
        assert torch.equal(g[~inside], g0[~inside]), "wrote outside the map"
        if with_colsum:
            npos = want.numel() // C
            assert npos <= 160
            wsum = want.reshape(-1, C).sum(0)
            bound = 1e-5 * want.reshape(-1, C).abs().sum(0)
            cerr = (cs.double() - wsum).abs()
            assert bool((cerr <= bound).all()), float((cerr / bound).max())


def test_lrelu_bwd_add_return_codes(f2g):
    from flow2gan_amd import _lib, ops
    g = ops.zeros(4 * 8 + 4, device=DEV)
    y = ops.zeros(4 * 8 + 4, device=DEV)
    u = ops.zeros(4 * 8, device=DEV)

    def rc(gp, yp, up, C=8, n=(1, 2, 2), gs=(32, 16, 8), off=0):
        return _lib.lib.f2g_lrelu_bwd_add(gp, yp, off, n[0], n[1], n[2], C, gs[0], gs[1], gs[2], up, 32, 2, 1, 4,
                                          SLOPE, None, ctypes.c_void_p(_lib.stream_ptr()))
    gp, yp, up = g.data_ptr(), y.data_ptr(), u.data_ptr()
    EINVAL = rc(None, yp, up)
    assert EINVAL != 0
    assert rc(gp, None, up) == EINVAL and rc(gp, yp, None) == EINVAL
    assert rc(gp, yp, up, C=6) == EINVAL
    assert rc(gp + 4, yp, up) == EINVAL                      # misaligned g
    for n in ((0, 2, 2), (1, 0, 2), (1, 2, 0)):
        assert rc(gp, yp, up, n=n) == 0                      # empty extents
    assert rc(gp, yp, up, C=0) == 0
    assert rc(gp, yp, up) == 0
    torch.cuda.synchronize()


# ====================================================================================== gradients vs the oracle
B, T = 2, 6001
_MODELS, _REF = {}, {}


def _models(family):
    """(oracle module, HIP module) with the oracle's weights under a fixed seed; built once per family."""
    if family not in _MODELS:
        import flow2gan_oracle as O
        from flow2gan_amd.models import discriminators as D
        Oc, Hc = {"mpd": (O.MultiPeriodDiscriminator, D.MultiPeriodDiscriminator),
                  "mrd": (O.MultiResolutionDiscriminator, D.MultiResolutionDiscriminator)}[family]
        torch.manual_seed(9)
        do, dh = Oc(), Hc()
        dh.load_state_dict(do.state_dict(), strict=False)
        _MODELS[family] = (do, dh.to(DEV))
    return _MODELS[family]


def _inputs():
    gen = torch.Generator().manual_seed(5)
    return 0.1 * torch.randn(B, T, generator=gen), 0.3 * torch.randn(B, T, generator=gen)


def _hip_sides(dh, family, x):
    """Per sub-discriminator, the sign pattern of every leaky-ReLU of the HIP forward of x (a device batch), as
    bool masks in the oracle's (B, C, H, W) convention and call order."""
    from flow2gan_amd import fused_disc as FD
    n = x.shape[0]
    out = []
    with torch.no_grad():
        for d in dh.discriminators:
            ms = []
            if family == "mpd":
                p = d.period
                st = FD._mpd_forward_one(x.contiguous(), p, d._params())
                for l in range(1, 6):
                    a = FD.unhalo(st["acts"][l], n * p, st["hs"][l])
                    ms.append((a.reshape(n, p, st["hs"][l], a.shape[-1]).permute(0, 3, 2, 1) > 0).cpu())
            else:
                st = FD._mrd_forward_one(x.contiguous(), d.window_length, d._params())
                Ft, Wcat, C = st["Ft"], st["Wcat"], FD.MRD_CH
                cat = st["cat"].view(n, Ft, Wcat, C)
                foff = 0
                for bi in range(5):
                    ws = st["widths"][bi]
                    for l in range(4):
                        ms.append((st["acts"][bi][l].view(n, Ft, ws[l + 1], C).permute(0, 3, 1, 2) > 0).cpu())
                    ms.append((cat[:, :, foff:foff + ws[5]].permute(0, 3, 1, 2) > 0).cpu())
                    foff += ws[5]
            out.append(ms)
    return out


def _with_sides(masks, fn):
    """Run fn() with `leaky_relu` inside flow2gan_oracle taking the side of every element from `masks` (consumed
    in call order): leaky-ReLU has no derivative at 0, and the handful of pre-activations that land on different
    sides in the two implementations would otherwise change the gradient through them by the factor 10."""
    import flow2gan_oracle as O
    queue = collections.deque(masks)

    def leaky(x, slope):
        m = queue.popleft()
        assert m.shape == x.shape, (m.shape, x.shape)
        return torch.where(m, x, slope * x)

    proxy = types.SimpleNamespace(**{k: getattr(O.F, k) for k in dir(O.F) if not k.startswith("__")})
    proxy.leaky_relu = leaky
    real_F, O.F = O.F, proxy
    try:
        out = fn()
    finally:
        O.F = real_F
    assert not queue, len(queue)
    return out


def _custom_loss(sr, sg, fr, fg):
    """Hinge terms on the scores + a dense, fixed random weighting of EVERY feature map of both halves."""
    gen = torch.Generator().manual_seed(77)
    loss = 0.0
    for s_r, s_g in zip(sr, sg):
        loss = loss + torch.relu(1 - s_r).mean() + torch.relu(1 + s_g).mean()
    for maps in (fr, fg):
        for sub in maps:
            for m in sub:
                r = torch.randn(m.shape, generator=gen).to(m.device)
                loss = loss + (m * r).sum() / math.sqrt(m.numel())
    return loss


def _reference(family):
    """Oracle gradients of _custom_loss with the HIP path's leaky-ReLU sides, once per (family, GEMM mode)."""
    from flow2gan_amd import ops
    key = (family, ops.GEMM_PRECISION)
    if key not in _REF:
        do, dh = _models(family)
        y, y_hat = _inputs()
        sides_r, sides_f = _hip_sides(dh, family, y.to(DEV)), _hip_sides(dh, family, y_hat.to(DEV))
        masks = []
        for i in range(len(sides_r)):           # _MultiD.forward: sub-discriminator i on y, then on y_hat
            masks += sides_r[i] + sides_f[i]
        yo = y_hat.clone().requires_grad_(True)
        do.zero_grad(set_to_none=True)

        def fn():
            loss = _custom_loss(*do(y, yo))
            loss.backward()
            return float(loss.detach())
        loss = _with_sides(masks, fn)
        _REF[key] = dict(loss=loss, gx=yo.grad.clone(), sides_f=sides_f,
                         grads={k: p.grad.clone() for k, p in do.named_parameters()})
        do.zero_grad(set_to_none=True)
    return _REF[key]


def _compare(pairs, tag):
    """pairs: (name, got, want).  Prints the worst figure, then holds every tensor to GRAD_TOL of its max."""
    rows = []
    for name, got, want in pairs:
        assert got is not None, name
        wmax = float(want.abs().max())
        err = float((got.detach().cpu().double() - want.double()).abs().max())
        rows.append((err / wmax if wmax > 0 else float("inf"), name, wmax))
    rows.sort(reverse=True)
    print(f"[disc-autograd] {tag}: worst relative error {rows[0][0]:.3e} ({rows[0][1]}) over {len(rows)} tensors")
    for rel, name, wmax in rows[1:4]:
        print(f"[disc-autograd]     then {rel:.3e} ({name}, max |want| {wmax:.3e})")
    for rel, name, wmax in rows:
        assert wmax > 0, name
        assert rel <= GRAD_TOL, (tag, name, rel)
    return rows[0][0]


def _hip_run(dh, y, y_hat, params_grad=True, input_grad=True):
    for p in dh.parameters():
        p.grad = None
        p.requires_grad_(params_grad)
    try:
        yd = y.to(DEV)
        yh = y_hat.to(DEV).requires_grad_(input_grad)
        loss = _custom_loss(*dh(yd, yh))
        loss.backward()
        torch.cuda.synchronize()
        assert yd.grad is None
        return float(loss.detach()), yh.grad, {k: p.grad for k, p in dh.named_parameters()}
    finally:
        for p in dh.parameters():
            p.requires_grad_(True)


@pytest.mark.parametrize("family", ["mpd", "mrd"])
def test_custom_loss_gradients_vs_oracle(f2g, family, gemm_mode_exact):
    ref = _reference(family)
    _, dh = _models(family)
    loss, gx, grads = _hip_run(dh, *_inputs())
    print(f"[disc-autograd] {family} {gemm_mode_exact} loss {loss:.7f} (oracle {ref['loss']:.7f})")
    pairs = [(k, grads[k], ref["grads"][k]) for k in ref["grads"]] + [("y_hat", gx, ref["gx"])]
    _compare(pairs, f"{family} {gemm_mode_exact} all gradients")


@pytest.mark.parametrize("family", ["mpd", "mrd"])
def test_input_gradient_only(f2g, family, gemm_mode_exact):
    ref = _reference(family)
    _, dh = _models(family)
    _, gx, grads = _hip_run(dh, *_inputs(), params_grad=False)
    assert all(v is None for v in grads.values())
    _compare([("y_hat", gx, ref["gx"])], f"{family} {gemm_mode_exact} input only")


@pytest.mark.parametrize("family", ["mpd", "mrd"])
def test_parameter_gradients_only(f2g, family, gemm_mode_exact):
    ref = _reference(family)
    _, dh = _models(family)
    _, gx, grads = _hip_run(dh, *_inputs(), input_grad=False)
    assert gx is None
    _compare([(k, grads[k], ref["grads"][k]) for k in ref["grads"]], f"{family} {gemm_mode_exact} parameters only")


@pytest.mark.parametrize("family", ["mpd", "mrd"])
def test_loss_on_one_feature_map(f2g, family, gemm_mode_exact):
    """Only fmap[1] of sub-discriminator 0 is used: every other upstream gradient is None.  The layers above the
    map get no (or an all-zero) gradient, the layers below it and the input the oracle's."""
    ref = _reference(family)
    do, dh = _models(family)
    _, y_hat = _inputs()
    below = {"mpd": ("convs.0.", "convs.1.", "convs.2."),
             "mrd": ("band_convs.0.0.", "band_convs.0.1.", "band_convs.0.2.")}[family]

    def one_map_loss(d, x):
        _, fmap = d(x)
        m = fmap[1]
        r = torch.randn(m.shape, generator=torch.Generator().manual_seed(3)).to(m.device)
        return (m * r).sum() / math.sqrt(m.numel())

    yo = y_hat.clone().requires_grad_(True)
    do.zero_grad(set_to_none=True)
    _with_sides(ref["sides_f"][0], lambda: one_map_loss(do.discriminators[0], yo).backward())
    want = {k: p.grad.clone() for k, p in do.discriminators[0].named_parameters() if p.grad is not None}
    do.zero_grad(set_to_none=True)
    assert sorted(k for k in want if float(want[k].abs().max()) > 0) == \
        sorted(k for k in want if k.startswith(below)), "the oracle's own gradients do not stop at the map"

    for p in dh.parameters():
        p.grad = None
    yh = y_hat.to(DEV).requires_grad_(True)
    one_map_loss(dh.discriminators[0], yh).backward()
    torch.cuda.synchronize()
    pairs = [("y_hat", yh.grad, yo.grad)]
    for k, p in dh.discriminators[0].named_parameters():
        if k.startswith(below):
            pairs.append((k, p.grad, want[k]))
        else:
            assert p.grad is None or not bool(p.grad.any()), k
    for d in dh.discriminators[1:]:
        assert all(p.grad is None for p in d.parameters())
    _compare(pairs, f"{family} {gemm_mode_exact} one feature map")


# ====================================================================================== the fused D-step
def test_composed_d_step_matches_fused(f2g, golden, gemm_mode_exact, monkeypatch):
    """A D-step loss composed from the modules + GAN.discriminator_loss against GAN.forward(train_disc=True):
    a structural check (normalisation, halves, ordering), not a precision claim."""
    import random

    from flow2gan_amd.models.gan import GAN
    g = golden("tiny_stage2")
    gen = f2g.MelAudioGenerator(**TINY)
    gen.load_state_dict({k[2:]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith("w/")})
    gen.branch_dropout = 0.0
    torch.manual_seed(int(g["d_seed"]))
    gan = GAN(gen).to(DEV)
    monkeypatch.setattr(random, "random", lambda: 0.0)
    mel, audio, noise = (torch.from_numpy(np.asarray(g[k])).to(DEV) for k in ("mel", "audio", "noise"))
    lens = torch.from_numpy(np.asarray(g["n1/lens"]))
    # A freshly initialised discriminator scores everything near 0: every hinge term is active, the real half's
    # score gradients sum to -1 and the generated half's to +1, and conv_post's bias gradient is an exact
    # cancellation whose computed value is rounding residue on both sides (nothing to compare).  So each
    # sub-discriminator's bias is shifted until the median real score sits on the hinge's threshold: about half
    # of the real terms go inactive and every gradient of the step is a real quantity.
    with torch.no_grad():
        pred = gan.generator.eval().infer(cond=mel, audio_lens=lens, n_timesteps=1, clamp_pred=False, noise=noise)
        for d in gan.discriminator:
            for sub, s_real in zip(d.discriminators, d(audio, pred)[0]):
                sub.conv_post.bias += 1.0 - s_real.median()

    gan.zero_grad(set_to_none=True)
    fused = gan(mel, audio, lens, 1, True, noise=noise)
    (fused[0] + fused[1]).backward()
    want = {k: p.grad.clone() for k, p in gan.discriminator.named_parameters()}

    gan.zero_grad(set_to_none=True)
    composed = []
    for d in gan.discriminator:
        sr, sg, _, _ = d(audio, pred)
        composed.append(gan.discriminator_loss(sr, sg))
    (composed[0] + composed[1]).backward()
    torch.cuda.synchronize()
    for a, b in zip(composed, fused):
        a, b = float(a.detach()), float(b.detach())
        assert abs(a - b) <= 2e-5 * abs(b), (a, b)
    for p in gan.generator.parameters():
        assert p.grad is None
    _compare([(k, p.grad, want[k].cpu()) for k, p in gan.discriminator.named_parameters()],
             f"{gemm_mode_exact} composed D-step against the fused one")


# ====================================================================================== no-grad behaviour
@pytest.mark.parametrize("family", ["mpd", "mrd"])
def test_no_grad_outputs_identical_and_graph_free(f2g, family):
    _, dh = _models(family)
    y, y_hat = (t.to(DEV) for t in _inputs())
    with torch.no_grad():
        quiet = dh(y, y_hat)
    loud = dh(y, y_hat.clone().requires_grad_(True))

    def flat(out):
        sr, sg, fr, fg = out
        return list(sr) + list(sg) + [m for sub in fr for m in sub] + [m for sub in fg for m in sub]
    a, b = flat(quiet), flat(loud)
    assert len(a) == len(b)
    for q, l in zip(a, b):
        assert torch.equal(q, l)
        assert not q.requires_grad and q.grad_fn is None
        assert l.requires_grad


def test_conditional_variant_still_refused(f2g):
    from flow2gan_amd.models import discriminators as D
    for make in (lambda: D.MultiPeriodDiscriminator(num_embeddings=4), lambda: D.DiscriminatorP(2, num_embeddings=4),
                 lambda: D.MultiResolutionDiscriminator(num_embeddings=4),
                 lambda: D.DiscriminatorR(512, num_embeddings=4)):
        with pytest.raises(NotImplementedError):
            make()
    _, dh = _models("mpd")
    x = torch.zeros(1, 600, device=DEV)
    with pytest.raises(NotImplementedError):
        dh(x, x, bandwidth_id=torch.zeros(1, dtype=torch.long, device=DEV))
    with pytest.raises(NotImplementedError):
        dh.discriminators[0](x, cond_embedding_id=torch.zeros(1, dtype=torch.long, device=DEV))
