"""Direct 32->32 (3,9)/(1,2) conv forward at the band shapes of one GAN stage-2 step (B = 64: 128
sequences; frames 47 / 94 / 188; band widths of the three stride-2 layers): TFLOP/s of the kernel
the library picks (F2G_CONV32_V2=0: the round-2 kernel).

AB=1: the precision-4 leg.  The same library's precision-3 launch (conv32x6.hip) against its precision-4 launch
(conv32h3.hip: fp16x3, the patch scaled per tile inside the kernel) in F2G_GEMM=fp16x3, one process on one box, legs
alternating (p3 1, p4 1, p3 2, ...), three runs each, weight images cached in both legs as in the step: the 45
forward shapes, the plain data gradient (S = 64), the masked data gradient + column sums (S = 128); then the stage-2
step, tunables off against on, in three alternating pairs.  ONLY=wgrad: the weight gradient instead (S = 128), the
precision-3 f2g_conv32_s2_wgrad launch against f2g_conv32_s2_wgrad_h3 (conv32h3w.hip), then the stage-2 step with
fp16x3_conv32_wgrad alone differing between the legs and the other two band-conv tunables as shipped.  ONLY=conv33:
the (3, 3) fifth layer instead -- every band width of the three resolutions after the three stride-2 layers, 15
shapes: forward (S = 128), plain data gradient (S = 64), masked data gradient + column sums (S = 128) --, the
precision-3 f2g_conv33_fwd launch (conv32x6.hip: conv33_x6_kernel) against its precision-4 launch (conv33h3.hip:
conv33_h3_kernel), then the stage-2 step with fp16x3_conv33_fwd / fp16x3_conv33_dgrad alone differing.  ONLY=wgrad33:
that layer's weight gradient at the same 15 shapes (S = 128), the precision-3 f2g_conv33_wgrad launch (conv32x6.hip:
conv33_wgrad6_kernel) against f2g_conv33_wgrad_h3 (conv33h3w.hip: conv33_wgrad3h_kernel), then the stage-2 step with
fp16x3_conv33_wgrad alone differing.  OUT=path: the report is written there as well."""
import os, sys, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from flow2gan_amd import ops, _lib as L
dev = "cuda"
# MODE=bf16x6: the fp32-class instances on the bf16 pipe (conv32x6.hip); MODE=bf16x3: the split-bf16 ones
ops.set_gemm_precision(os.environ.get("MODE", "fp32"))
ONLY = os.environ.get("ONLY", "")          # "fwd" / "dgrad" / "wgrad": that part alone
def timeit(fn, n=10):
    for _ in range(3): fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e-3


def band_shapes():
    for H, nb in ((47, 1025), (94, 513), (188, 257)):
        edges = [int(f * nb) for f in (0.0, 0.1, 0.25, 0.5, 0.75, 1.0)]
        for b in range(5):
            Win = edges[b + 1] - edges[b]
            for layer in range(3):
                yield H, Win, (Win - 1) // 2 + 1
                Win = (Win - 1) // 2 + 1


def band33_shapes():
    """(H, W, W) of the (3, 3) fifth layer: every third shape's output width"""
    for i, (H, Win, Wout) in enumerate(band_shapes()):
        if i % 3 == 2:
            yield H, Wout, Wout


def ab_main():
    import statistics, time
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    ops.set_gemm_precision("fp16x3")
    w = torch.nn.Parameter(torch.randn(32, 27 * 32, device=dev) * 0.05)       # (parameters: the images are cached)
    wT = torch.nn.Parameter(torch.randn(27, 32, 32, device=dev) * 0.05)
    w33 = torch.nn.Parameter(torch.randn(32, 9 * 32, device=dev) * 0.05)     # [co][tap][ci] / [ci][8 - tap][co]
    bb = torch.randn(32, device=dev)

    WG = ONLY == "wgrad"                       # the weight-gradient tunable alone differs between the legs
    C33 = ONLY == "conv33"                     # the (3, 3) layer's two tunables alone differ between the legs
    WG33 = ONLY == "wgrad33"                   # the (3, 3) layer's weight-gradient tunable alone differs
    only = "" if C33 or WG33 else ONLY
    shapes = list(band33_shapes() if C33 or WG33 else band_shapes())

    def leg(on):
        if WG:
            ops.FP16X3_CONV32_WGRAD = on
        elif WG33:
            ops.FP16X3_CONV33_WGRAD = on
        elif C33:
            ops.FP16X3_CONV33_FWD = ops.FP16X3_CONV33_DGRAD = on
        else:
            ops.FP16X3_CONV32_FWD = ops.FP16X3_CONV32_DGRAD = on

    say(f"# tools/conv32_probe.py AB=1  {L.version()}  {torch.cuda.get_device_name(0)}")
    say("# p3 = f2g_conv32_desc.precision 3 (conv32x6.hip), p4 = precision 4 (conv32h3.hip; weight gradient: "
        "conv32h3w.hip; ONLY=conv33: conv33h3.hip; ONLY=wgrad33: conv33h3w.hip), the same library, F2G_GEMM=fp16x3,")
    say("# one process, legs alternating p3 1, p4 1, p3 2, p4 2, p3 3, p4 3; us per launch (10 launches after 3)")
    for title, S, kind in (("forward", 128, "fwd"), ("plain data gradient (S = 64)", 64, "dgrad"),
                           ("masked data gradient + column sums (S = 128)", 128, "mask"),
                           ("weight gradient (S = 128)", 128, "wgrad"),
                           ("(3, 3) weight gradient (S = 128)", 128, "wgrad33")):
        if (kind == "wgrad33") != WG33:
            continue
        if not WG33 and ((kind == "wgrad") != WG or (only and not kind.startswith(only) and not (only == "dgrad" and kind == "mask"))):
            continue
        runs = {False: [], True: []}
        for rep in range(3):
            for on in (False, True):
                leg(on)
                ts = []
                for H, Win, Wout in shapes:
                    if WG33:
                        x = torch.randn(S * H * Win, 32, device=dev)
                        gy = torch.randn(S * H * Win, 32, device=dev)
                        gw = torch.zeros(32, 9 * 32, device=dev)
                        ts.append(timeit(lambda: ops.conv33_wgrad(x, gy, S, H, Win, gw)))
                    elif C33:
                        x = torch.randn(S * H * Win, 32, device=dev)
                        y = torch.empty(S * H * Win, 32, device=dev)
                        if kind == "fwd":
                            ts.append(timeit(lambda: ops.conv33(x, S, H, Win, w33, bb, 0.1, y)))
                        elif kind == "mask":
                            ym = torch.randn(S * H * Win, 32, device=dev)
                            csum = torch.zeros(32, device=dev)
                            ts.append(timeit(lambda: ops.conv33(x, S, H, Win, w33, None, 0.0, y, form=1,
                                                                mask=(ym, 0, 0.1), colsum=csum)))
                        else:
                            ts.append(timeit(lambda: ops.conv33(x, S, H, Win, w33, None, 0.0, y, form=1)))
                    elif kind == "fwd":
                        x = torch.randn(S * H * Win, 32, device=dev)
                        y = torch.empty(S * H * Wout, 32, device=dev)
                        ts.append(timeit(lambda: ops.conv32_s2_fwd(x, S, H, Win, Wout, w, bb, 0.1, y)))
                    elif kind == "wgrad":
                        x = torch.randn(S * H * Win, 32, device=dev)
                        gy = torch.randn(S * H * Wout, 32, device=dev)
                        gw = torch.zeros(32, 27 * 32, device=dev)
                        ts.append(timeit(lambda: ops.conv32_s2_wgrad(x, gy, S, H, Win, Wout, gw)))
                    else:
                        gy = torch.randn(S * H * Wout, 32, device=dev)
                        gx = torch.empty(S * H * Win, 32, device=dev)
                        if kind == "mask":
                            ym = torch.randn(S * H * Win, 32, device=dev)
                            csum = torch.zeros(32, device=dev)
                            ts.append(timeit(lambda: ops.conv32_s2_dgrad(gy, S, H, Win, Wout, wT, gx, mask=(ym, 0, 0.1),
                                                                         colsum=csum)))
                        else:
                            ts.append(timeit(lambda: ops.conv32_s2_dgrad(gy, S, H, Win, Wout, wT, gx)))
                runs[on].append(ts)
        say(f"\n== {title}: us per launch, three runs per leg; range = max - min of a leg's three runs")
        say("   H  Win |           p3            |           p4            |     medians     | ratio | verdict")
        for i, (H, Win, Wout) in enumerate(shapes):
            a = [r[i] * 1e6 for r in runs[False]]
            b = [r[i] * 1e6 for r in runs[True]]
            ma, mb = statistics.median(a), statistics.median(b)
            rng = max(max(a) - min(a), max(b) - min(b))
            verdict = "wins" if ma - mb > rng else ("LOSES" if mb - ma > rng else "within range")
            say(f"{H:4d} {Win:4d} | {a[0]:7.1f} {a[1]:7.1f} {a[2]:7.1f} | {b[0]:7.1f} {b[1]:7.1f} {b[2]:7.1f} | "
                f"{ma:7.1f} {mb:7.1f} | {mb / ma:.3f} | {verdict}")
        ta, tb = [sum(r) * 1e3 for r in runs[False]], [sum(r) * 1e3 for r in runs[True]]
        say(f"total of the {len(shapes)} launches (ms): p3 " + " ".join(f"{t:.2f}" for t in ta) + "   p4 "
            + " ".join(f"{t:.2f}" for t in tb) + f"   ranges {max(ta) - min(ta):.2f} / {max(tb) - min(tb):.2f}"
            + f"   medians {statistics.median(ta):.2f} -> {statistics.median(tb):.2f}")
    if not ONLY or WG or C33 or WG33:
        import flow2gan_amd
        from flow2gan_amd import harness
        from flow2gan_amd.models.config import get_gan_config, get_generator_config
        from flow2gan_amd.models.gan import GAN
        Bn = 64
        gcfg = get_generator_config("mel_24k_base")
        sr = gcfg["sampling_rate"]
        torch.manual_seed(1234)
        gen = flow2gan_amd.MelAudioGenerator(**gcfg)
        gen.branch_dropout = 0.0
        gan = GAN(gen, **get_gan_config("gan_multi_scale_mel_recon")).to(dev)
        logmel = flow2gan_amd.LogMelSpectrogram(sr, gcfg["mel_n_fft"], gcfg["mel_hop_length"], gcfg["n_mels"]).to(dev)
        gg = torch.Generator().manual_seed(99)
        audio = (0.1 * torch.randn(Bn, sr, generator=gg)).clamp_(-1, 1).to(dev)
        lens = torch.full((Bn,), sr, dtype=torch.int64)
        g_params, d_params = list(gan.generator.parameters()), list(gan.discriminator.parameters())

        def stage2():
            for disc, params in ((True, d_params), (False, g_params)):
                for p_ in params:
                    p_.grad = None
                loss, _ = harness.compute_loss_stage2(audio, lens, gan, logmel, 1, train_disc=disc)
                loss.backward()
                ops.bump_weight_epoch(params)
                ops.rebuild_derived(params)

        nsteps = 4
        for on in (False, True):
            leg(on)
            stage2(), stage2()
        torch.cuda.synchronize()
        per, counts = {False: [], True: []}, {False: (0, 0), True: (0, 0)}
        for rep in range(3):
            for on in (False, True):
                leg(on)
                def launches():
                    if WG33:
                        return 0, 0, ops.FP16X3_CONV33_WGRAD_LAUNCHES
                    if C33:
                        return ops.FP16X3_CONV33_FWD_LAUNCHES, ops.FP16X3_CONV33_DGRAD_LAUNCHES, 0
                    return ops.FP16X3_CONV32_FWD_LAUNCHES, ops.FP16X3_CONV32_DGRAD_LAUNCHES, ops.FP16X3_CONV32_WGRAD_LAUNCHES
                n0 = launches()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(nsteps):
                    stage2()
                torch.cuda.synchronize()
                per[on].append((time.perf_counter() - t0) * 1e3 / nsteps)
                counts[on] = tuple((a - b) // nsteps for a, b in zip(launches(), n0))
        what = "fp16x3_conv32_wgrad alone off against on, the other band-conv tunables as shipped" if WG \
            else "fp16x3_conv33_wgrad alone off against on, the other band-conv tunables as shipped" if WG33 \
            else ("fp16x3_conv33_fwd / fp16x3_conv33_dgrad alone off against on, the other band-conv tunables as "
                  "shipped" if C33 else "tunables off against on")
        say(f"\n== the stage-2 step (B = {Bn}, F2G_GEMM=fp16x3), {what}: ms per step, blocks of "
            f"{nsteps} steps, three alternating pairs")
        for rep in range(3):
            say(f"pair {rep + 1}: off {per[False][rep]:.2f}   on {per[True][rep]:.2f}")
        mo, mn = statistics.median(per[False]), statistics.median(per[True])
        say(f"medians {mo:.2f} -> {mn:.2f} (ratio {mn / mo:.3f}); within-leg ranges "
            f"{max(per[False]) - min(per[False]):.2f} / {max(per[True]) - min(per[True]):.2f}; precision-4 launches per "
            f"step: off {counts[False]}, on {counts[True]} (forward, data gradient, weight gradient)")
    leg(False)
    if os.environ.get("OUT"):
        os.makedirs(os.path.dirname(os.path.abspath(os.environ["OUT"])), exist_ok=True)
        with open(os.environ["OUT"], "w") as f:
            f.write("\n".join(lines) + "\n")


if os.environ.get("AB", "0") == "1":
    ab_main()
    sys.exit(0)

tot_t = tot_f = 0.0
for H, nb in ((47, 1025), (94, 513), (188, 257)) if ONLY in ("", "fwd") else ():
    edges = [int(f * nb) for f in (0.0, 0.1, 0.25, 0.5, 0.75, 1.0)]
    for b in range(5):
        Win = edges[b + 1] - edges[b]
        for layer in range(3):
            Wout = (Win - 1) // 2 + 1
            S = 128
            x = torch.randn(S * H * Win, 32, device=dev)
            w = torch.randn(32, 27 * 32, device=dev) * 0.05
            bb = torch.randn(32, device=dev)
            y = torch.empty(S * H * Wout, 32, device=dev)
            f = lambda: ops.conv32_s2_fwd(x, S, H, Win, Wout, w, bb, 0.1, y)
            t = timeit(f)
            fl = 2.0 * S * H * Wout * 32 * 864
            tot_t += t; tot_f += fl
            print(f"H={H:3d} Win={Win:3d} Wout={Wout:3d}: {t*1e6:7.1f} us {fl/t/1e12:6.1f} TF", flush=True)
            Win = Wout
if tot_t:
    print(f"all 45 forward launches of a pass: {tot_t*1e3:.2f} ms, {tot_f/tot_t/1e12:.1f} TFLOP/s")

# ---- data gradient at the same shapes
tot_t = tot_f = 0.0
for H, nb in ((47, 1025), (94, 513), (188, 257)) if ONLY in ("", "dgrad") else ():
    edges = [int(f * nb) for f in (0.0, 0.1, 0.25, 0.5, 0.75, 1.0)]
    for b in range(5):
        Win = edges[b + 1] - edges[b]
        for layer in range(3):
            Wout = (Win - 1) // 2 + 1
            # MASK=1: the D-step's form (both halves, leaky-ReLU mask + bias sums fused); default: the G-step's
            # (generated half only, plain)
            MASK = os.environ.get("MASK", "0") == "1"
            S = 128 if MASK else 64
            gy = torch.randn(S * H * Wout, 32, device=dev)
            wT = torch.randn(27, 32, 32, device=dev) * 0.05
            gx = torch.empty(S * H * Win, 32, device=dev)
            if MASK:
                ym = torch.randn(S * H * Win, 32, device=dev)
                csum = torch.zeros(32, device=dev)
                t = timeit(lambda: ops.conv32_s2_dgrad(gy, S, H, Win, Wout, wT, gx, mask=(ym, 0, 0.1), colsum=csum))
            else:
                t = timeit(lambda: ops.conv32_s2_dgrad(gy, S, H, Win, Wout, wT, gx))
            fl = 2.0 * S * H * Wout * 32 * 864
            tot_t += t; tot_f += fl
            print(f"dgrad H={H:3d} Win={Win:3d}: {t*1e6:7.1f} us {fl/t/1e12:6.1f} TF", flush=True)
            Win = Wout
if tot_t:
    print(f"all 45 data-gradient launches of a pass (S = {128 if os.environ.get('MASK', '0') == '1' else 64}): {tot_t*1e3:.2f} ms, {tot_f/tot_t/1e12:.1f} TFLOP/s")

# ---- weight gradient at the same shapes (D-step: both halves, S = 128)
tot_t = tot_f = 0.0
for H, nb in ((47, 1025), (94, 513), (188, 257)) if ONLY in ("", "wgrad") else ():
    edges = [int(f * nb) for f in (0.0, 0.1, 0.25, 0.5, 0.75, 1.0)]
    for b in range(5):
        Win = edges[b + 1] - edges[b]
        for layer in range(3):
            Wout = (Win - 1) // 2 + 1
            S = 128
            x = torch.randn(S * H * Win, 32, device=dev)
            gy = torch.randn(S * H * Wout, 32, device=dev)
            gw = torch.zeros(32, 27 * 32, device=dev)
            t = timeit(lambda: ops.conv32_s2_wgrad(x, gy, S, H, Win, Wout, gw))
            fl = 2.0 * S * H * Wout * 32 * 864
            tot_t += t; tot_f += fl
            print(f"wgrad H={H:3d} Win={Win:3d}: {t*1e6:7.1f} us {fl/t/1e12:6.1f} TF", flush=True)
            Win = Wout
if tot_t:
    print(f"all 45 weight-gradient launches of a pass (S = 128): {tot_t*1e3:.2f} ms, {tot_f/tot_t/1e12:.1f} TFLOP/s")
