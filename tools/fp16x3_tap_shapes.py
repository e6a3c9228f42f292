#!/usr/bin/env python
"""fp16x3 against bf16x6 on the MPD's tap-walking GEMMs and on the stage-2 step -- one box, one process.

Per period (2, 3, 5, 7, 11) at B = 64 x 1 s of 24 kHz audio, real and generated halves together (S = 128 p sequences):
  fwd5    the forward of the 1024 -> 1024 stride-1 layer (five taps, K = 5120; bias + leaky ReLU, halo row map)
  dgrad5  that layer's data gradient (five taps; row map, leaky-ReLU mask, column sums, the result's bf16x3 image)
  dgrad4  the two two-tap residue data gradients of the 512 -> 1024 stride-3 layer below (K = 2048; row map, mask,
          column sums), timed together
and the same at B = 32, 16 and 8 for periods 2 and 11 (where the route's row threshold lies),
each timed in both modes, the modes ALTERNATING block by block (time_blocks / med_spread of tools/fp16x3_shapes.py),
with everything a launch costs in its mode inside the timed region: fp16x3 = the map's f2g_split_f16x2_seq image pass
plus gemm_h3p_kernel (the weight's image is cached, as in the step); bf16x6 = the launch as that mode routes it
(gemm_x6p_kernel over the map's three-piece image: written by the producer's epilogue in the step, made once outside
the timed region here -- the baseline pays no image pass).

Then the stage-2 step as tools/fp16x3_shapes.py runs it, in three legs that alternate block by block: bf16x6, fp16x3
with the route off, fp16x3 with the route on.

The tool, whose purpose is to measure the route, sets the threshold itself: --min-rows, default 1 = every launch the
library accepts goes to the new kernel.  The header of the output states the command it was made with.

--tap3 measures the STRIDE-3 route instead (gemm_h3p3_kernel, ops.FP16X3_TAP3_MIN_ROWS; default output
profiles/fp16x3_tap3_shapes.txt), the stride-1 route staying as shipped:
  fwd3    the forward of the 128 -> 512 stride-3 layer (five taps, K = 640; bias + leaky ReLU, halo row map, the
          result's bf16x3 image -- as _mpd_forward_one launches it)
  fwd4    the forward of the 512 -> 1024 stride-3 layer (K = 2560; the same epilogue)
per period at B = 64 and for periods 2 and 11 at B = 32 and 16, under the same timing conditions (fp16x3 = the map's
f2g_split_f16x2_seq pass plus the kernel; bf16x6 = gemm_x6_kernel over a three-piece image made once outside the timed
region), then the stage-2 step in the fp16x3 mode with that tunable alone differing, in three alternating pairs.

--tap3n measures the route of the 32-CHANNEL stride-3 layer (gemm_h3p3n_kernel, ops.FP16X3_TAP3N_MIN_ROWS; default
output profiles/fp16x3_tap3n_shapes.txt), every other route staying as shipped:
  fwd2    the forward of the 32 -> 128 stride-3 layer (five taps, K = 160; bias + leaky ReLU, halo row map, the
          result's bf16x3 image -- as _mpd_forward_one launches it)
  fwd2-   the same launch without the result's image (E.x3_out unset)
per period at B = 64 and B = 16.  fp16x3 = the kernel alone: it reads the fp32 map and scales it per sequence segment
itself, there is no image pass to include; bf16x6 = the launch as that mode routes it (gemm_x6g_kernel, which splits
the fp32 map inside the kernel: K = 160 < x6_min_k, no image pass either).  Then the stage-2 step in the fp16x3 mode with that
tunable alone differing, in three alternating pairs.

--tapn measures the route of that layer's DATA GRADIENT (gemm_h3pn_kernel, ops.FP16X3_TAPN_MIN_ROWS; default output
profiles/fp16x3_tapn_shapes.txt), every other route staying as shipped:
  dgrad2  the three stride-residue data gradients of the 32 -> 128 layer (two, two and one taps over the 128-channel
          gradient map, K = 256 / 256 / 128, N = 32; stride-3 row map into the 32-channel halo map, no mask -- as
          fused_disc._conv1d_dgrad launches them), timed together
per period at B = 64 and B = 16.  fp16x3 = the kernel alone (no image pass); bf16x6 = the launches as that mode routes
them (gemm_x6n_kernel, which splits the fp32 map inside the kernel and pays no image pass either; its device code is
the parent commit's).  Then the stage-2 step in the fp16x3 mode with that tunable alone differing, in three alternating
pairs.

--tapn3 measures that data gradient as ONE launch (gemm_h3pn3_kernel, ops.FP16X3_TAPN3_MIN_ROWS; default output
profiles/fp16x3_tapn3_shapes.txt), every other route staying as shipped.  The shapes are the ten data gradients of the
32 -> 128 layer that a stage-2 step issues at B = 64 and at B = 16, taken from the calls fused_disc._conv1d_dgrad
receives while one step runs.  Per shape three legs alternate in one process, three blocks of 12 each: the three
launches both modes run as shipped (gemm_x6n_kernel; below ops.X6F_TALL_ROWS rows the exact-fp32 kernel -- the row
names the kernel), the three gemm_h3pn_kernel launches, the one
gemm_h3pn3_kernel launch; per leg the median, the range of its blocks and the bytes of the gradient map read per
second.  "wins" / "loses": beyond BOTH legs' ranges.  Then the stage-2 step in the fp16x3 mode with that tunable alone
differing, in three alternating pairs.

    python tools/fp16x3_tap_shapes.py [--out profiles/fp16x3_tap_shapes.txt] [--append] [--no-shapes] [--no-steps]
                                      [--min-rows R] [--tap3 | --tap3n | --tapn | --tapn3]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fp16x3_shapes import med_spread, time_blocks  # noqa: E402

PERIODS = (2, 3, 5, 7, 11)
B, T = 64, 24000


def heights(p):
    hs = [(T + p - 1) // p]
    for st in (3, 3, 3, 3, 1):
        hs.append((hs[-1] + 4 - 5) // st + 1)
    return hs


def cases(ops, FD, p, dev, batch=B):
    """(name, rows, K, N, fn) of period p at `batch` clips; the operands are allocated here, outside the timed region"""
    S, hs = 2 * batch * p, heights(p)
    H3, H4 = hs[3], hs[4]
    g = torch.Generator().manual_seed(p)

    def halo_map(H, Cc, scale=1.0, x3=False):
        buf = FD._halo_rows(S, H, Cc, dev, x3=x3)
        FD.unhalo(buf, S, H).copy_((torch.randn(S, H, Cc, generator=g) * scale).to(dev))
        if x3 and getattr(buf, "_f2g_x3_buf", None) is not None:      # the producer's image, made once
            buf._f2g_x3 = ops.x3_flat_image(buf)
        return buf

    w5 = torch.nn.Parameter((torch.randn(1024, 1024, 5, 1, generator=g) * 5120 ** -0.5).to(dev))
    w4 = torch.nn.Parameter((torch.randn(1024, 512, 5, 1, generator=g) * 2560 ** -0.5).to(dev))
    b5 = torch.randn(1024, generator=g).to(dev)
    out = []
    # forward of layer 5
    x4 = halo_map(H4, 1024, x3=True)
    y5 = FD._halo_rows(S, H4, 1024, dev)
    wp = ops.derived(w5, "pack", FD.pack_conv_weight)
    out.append(("fwd5", S * H4, 5120, 1024, lambda: ops.gemm(
        ops.win1d(x4, S, H4 + 2 * FD.HALO, 1024, H4, 1, 0, 5), ops.mat(wp), y5, bias=b5, lrelu=FD.SLOPE,
        rowmap=FD._halo_map(H4, 1024))))
    # data gradients: of layer 5 (one five-tap residue), of layer 4 (its two two-tap residues)
    for name, w, stride, Hin, Cin in (("dgrad5", w5, 1, H4, 1024), ("dgrad4", w4, 3, H3, 512)):
        gpre = halo_map(H4, 1024, 1e-3, x3=True)
        act = halo_map(Hin, Cin)
        want_img = 2 * Cin >= ops.X6_MIN_K
        gx = FD._halo_rows(S, Hin, Cin, dev, x3=want_img)
        cs = torch.zeros(Cin, device=dev)
        launches = []
        for rho, j0, nt, e0, Lq in FD._residues(5, stride, 2, Hin):
            if Lq == 0 or nt not in (5, 2):
                continue
            wq = FD._dgrad_weight(w, stride, j0, nt)
            launches.append((wq, (nt - 1) - e0 - FD.HALO, nt, Lq,
                             (Lq, (Hin + 2 * FD.HALO) * Cin, stride * Cin, (FD.HALO + rho) * Cin)))

        def fn(gpre=gpre, act=act, gx=gx, cs=cs, launches=launches, want_img=want_img):
            for wq, pad, nt, Lq, rm in launches:
                ops.gemm(ops.win1d(gpre, S, H4 + 2 * FD.HALO, 1024, Lq, 1, pad, nt), ops.mat(wq), gx, rowmap=rm,
                         mask=(act, 0, FD.SLOPE), colsum=cs, x3_out=want_img)
        rows = sum(S * l[3] for l in launches)
        out.append((name, rows, launches[0][2] * 1024, Cin, fn))
    return out


def cases3(ops, FD, p, dev, batch=B):
    """(name, rows, K, N, fn) of the two stride-3 forwards of period p at `batch` clips"""
    S, hs = 2 * batch * p, heights(p)
    g = torch.Generator().manual_seed(100 + p)
    out = []
    for name, l in (("fwd3", 2), ("fwd4", 3)):
        Cin, Cout, H, Hout = FD.MPD_CH[l], FD.MPD_CH[l + 1], hs[l], hs[l + 1]
        x = FD._halo_rows(S, H, Cin, dev, x3=True)
        FD.unhalo(x, S, H).copy_(torch.randn(S, H, Cin, generator=g).to(dev))
        if getattr(x, "_f2g_x3_buf", None) is not None:      # the producer's image, made once
            x._f2g_x3 = ops.x3_flat_image(x)
        y = FD._halo_rows(S, Hout, Cout, dev, x3=True)
        w = torch.nn.Parameter((torch.randn(Cout, Cin, 5, 1, generator=g) * (5 * Cin) ** -0.5).to(dev))
        b = torch.randn(Cout, generator=g).to(dev)
        wp = ops.derived(w, "pack", FD.pack_conv_weight)

        def fn(x=x, y=y, wp=wp, b=b, H=H, Hout=Hout, Cin=Cin, Cout=Cout):
            ops.gemm(ops.win1d(x, S, H + 2 * FD.HALO, Cin, Hout, 3, 0, 5), ops.mat(wp), y, bias=b, lrelu=FD.SLOPE,
                     rowmap=FD._halo_map(Hout, Cout), x3_out=True)
        out.append((name, S * Hout, 5 * Cin, Cout, fn))
    return out


def cases3n(ops, FD, p, dev, batch=B):
    """(name, rows, K, N, fn) of the 32 -> 128 stride-3 forward of period p at `batch` clips, with and without the
    result's three-piece image"""
    S, hs = 2 * batch * p, heights(p)
    g = torch.Generator().manual_seed(200 + p)
    Cin, Cout, H, Hout = FD.MPD_CH[1], FD.MPD_CH[2], hs[1], hs[2]
    x = FD._halo_rows(S, H, Cin, dev, x3=True)
    FD.unhalo(x, S, H).copy_(torch.randn(S, H, Cin, generator=g).to(dev))
    if getattr(x, "_f2g_x3_buf", None) is not None:      # the producer's image, made once
        x._f2g_x3 = ops.x3_flat_image(x)
    y = FD._halo_rows(S, Hout, Cout, dev, x3=True)
    w = torch.nn.Parameter((torch.randn(Cout, Cin, 5, 1, generator=g) * (5 * Cin) ** -0.5).to(dev))
    b = torch.randn(Cout, generator=g).to(dev)
    wp = ops.derived(w, "pack", FD.pack_conv_weight)

    def fn(x3):
        ops.gemm(ops.win1d(x, S, H + 2 * FD.HALO, Cin, Hout, 3, 0, 5), ops.mat(wp), y, bias=b, lrelu=FD.SLOPE,
                 rowmap=FD._halo_map(Hout, Cout), x3_out=x3)
    return [("fwd2", S * Hout, 5 * Cin, Cout, lambda: fn(True)), ("fwd2-", S * Hout, 5 * Cin, Cout, lambda: fn(False))]


def casesn(ops, FD, p, dev, batch=B):
    """(name, rows, K, N, fn) of the three residue data gradients of the 32 -> 128 stride-3 layer of period p at
    `batch` clips, launched one after the other as fused_disc._conv1d_dgrad does"""
    S, hs = 2 * batch * p, heights(p)
    g = torch.Generator().manual_seed(300 + p)
    Cin, Cout, Hin, Hout = FD.MPD_CH[1], FD.MPD_CH[2], hs[1], hs[2]
    gpre = FD._halo_rows(S, Hout, Cout, dev)
    FD.unhalo(gpre, S, Hout).copy_((torch.randn(S, Hout, Cout, generator=g) * 1e-3).to(dev))
    gx = FD._halo_rows(S, Hin, Cin, dev)
    w = torch.nn.Parameter((torch.randn(Cout, Cin, 5, 1, generator=g) * (5 * Cin) ** -0.5).to(dev))
    launches = []
    for rho, j0, nt, e0, Lq in FD._residues(5, 3, 2, Hin):
        if Lq:
            launches.append((FD._dgrad_weight(w, 3, j0, nt), (nt - 1) - e0 - FD.HALO, nt, Lq,
                             (Lq, (Hin + 2 * FD.HALO) * Cin, 3 * Cin, (FD.HALO + rho) * Cin)))

    def fn():
        for wq, pad, nt, Lq, rm in launches:
            ops.gemm(ops.win1d(gpre, S, Hout + 2 * FD.HALO, Cout, Lq, 1, pad, nt), ops.mat(wq), gx, rowmap=rm)
    # (FLOPs of the table: rows x the longest reduction, as for dgrad4; the one-tap residue has half of it)
    return [("dgrad2", sum(S * l[3] for l in launches), 2 * Cout, Cin, fn)]


def shapes3_table(ops, dev, say, counter="FP16X3_TAP3_LAUNCHES", cases_of=cases3,
                  batches=((B, PERIODS), (32, (2, 11)), (16, (2, 11)))):
    from flow2gan_amd import fused_disc as FD
    ops.set_gemm_precision("bf16x6")        # (the maps' three-piece images are reserved in this mode only)
    say("batch period  launch     rows      K      N  bf16x6_us  spread  fp16x3_us  spread  ratio  beyond spread  "
        "TFLOP/s(fp16x3)  kernels")
    seen = []
    for batch, periods in batches:
        for p in periods:
            for name, rows, K, N, fn in cases_of(ops, FD, p, dev, batch):
                n0 = getattr(ops, counter)
                per, kern = time_blocks(ops, fn)
                taken = getattr(ops, counter) > n0
                if name == "dgrad2":      # (FLOPs: the residues have 2, 2 and 1 taps -- 5 / 6 of rows x 256)
                    K = K * 5 // 6
                (a, sa), (b, sb) = med_spread(per["bf16x6"]), med_spread(per["fp16x3"])
                verdict = "-" if not taken else ("wins" if b / a < 1.0 - max(sa, sb) else
                                                 ("loses" if b / a > 1.0 + max(sa, sb) else "inside"))
                say(f"{batch:5d} {p:6d}  {name:7s} {rows:7d} {K:6d} {N:6d} {a:10.1f} {sa:7.3f} {b:10.1f} {sb:7.3f} "
                    f"{b / a:6.3f}  {verdict:13s} {2.0 * rows * K * N / b * 1e-6:12.1f}      "
                    f"{kern['bf16x6']} | {kern['fp16x3']}" + ("" if taken else "   (not taken by the library)"))
                seen.append(verdict)
            torch.cuda.empty_cache()
    say(f"# launches: {len(seen)}; fp16x3 wins by more than the spread: {seen.count('wins')}, loses by more than the "
        f"spread: {seen.count('loses')}, inside the spread: {seen.count('inside')}, not taken: {seen.count('-')}")


def shapes_table(ops, dev, say):
    from flow2gan_amd import fused_disc as FD
    ops.set_gemm_precision("bf16x6")        # (the maps' three-piece images are reserved in this mode only)
    say("batch period  launch     rows      K      N  bf16x6_us  spread  fp16x3_us  spread  ratio  TFLOP/s(fp16x3)  kernels")
    worst = []
    # the step's own shapes (B = 64, every period), then smaller batches at the two outer periods: where the rule's
    # row threshold lies (a launch the library keeps off the kernel -- a grid that does not fill the chip, library
    # option x6p = 1 -- runs the bf16x6 kernel in both legs and is marked so)
    for batch, periods in ((B, PERIODS), (32, (2, 11)), (16, (2, 11)), (8, (2, 11))):
        for p in periods:
            for name, rows, K, N, fn in cases(ops, FD, p, dev, batch):
                n0 = ops.FP16X3_TAP_LAUNCHES
                per, kern = time_blocks(ops, fn)
                taken = ops.FP16X3_TAP_LAUNCHES > n0
                assert taken or batch < B, f"period {p} {name}: the fp16x3 leg never took the route"
                (a, sa), (b, sb) = med_spread(per["bf16x6"]), med_spread(per["fp16x3"])
                say(f"{batch:5d} {p:6d}  {name:7s} {rows:7d} {K:6d} {N:6d} {a:10.1f} {sa:7.3f} {b:10.1f} {sb:7.3f} "
                    f"{b / a:6.3f} {2.0 * rows * K * N / b * 1e-6:12.1f}      {kern['bf16x6']} | {kern['fp16x3']}"
                    + ("" if taken else "   (not taken: the grid does not fill the chip)"))
                if taken:
                    worst.append((b / a, max(sa, sb), p, f"B {batch} {name}", rows // (2 if name == "dgrad4" else 1)))
            torch.cuda.empty_cache()
    won = [w for w in worst if w[0] < 1.0 - w[1]]
    lost = [w for w in worst if w[0] > 1.0 + w[1]]
    say(f"# launches where fp16x3 wins by more than the spread: {len(won)} of {len(worst)}"
        + "".join(f"\n#   period {p} {n} rows {r}: ratio {q:.3f}, spread {s:.3f}" for q, s, p, n, r in won))
    say(f"# launches where fp16x3 loses by more than the spread: {len(lost)} of {len(worst)}"
        + "".join(f"\n#   period {p} {n} rows {r}: ratio {q:.3f}, spread {s:.3f}" for q, s, p, n, r in lost))
    if won:
        say(f"# fewest output rows of a winning launch (dgrad4: of one of its two launches): {min(w[4] for w in won)}")
        say(f"# rule: ops.FP16X3_TAP_MIN_ROWS = {min(w[4] for w in won)} -- on, from the smallest row count that wins by "
            "more than its spread" + ("" if lost else "; no launch the library accepts loses"))


_MODEL = []     # (gan, logmel, sampling rate): built once per run


def stage2_of(ops, dev, batch=B):
    """the stage-2 step (D-step, then G-step; the weight images rebuilt as after an optimizer step) of mel_24k_base at
    `batch` clips of 1 s, as a function"""
    import flow2gan_amd
    from flow2gan_amd import harness
    from flow2gan_amd.models.config import get_gan_config, get_generator_config
    from flow2gan_amd.models.gan import GAN
    if not _MODEL:
        gcfg = get_generator_config("mel_24k_base")
        torch.manual_seed(1234)
        gen = flow2gan_amd.MelAudioGenerator(**gcfg)
        gen.branch_dropout = 0.0
        gan = GAN(gen, **get_gan_config("gan_multi_scale_mel_recon")).to(dev)
        logmel = flow2gan_amd.LogMelSpectrogram(gcfg["sampling_rate"], gcfg["mel_n_fft"], gcfg["mel_hop_length"],
                                                gcfg["n_mels"]).to(dev)
        _MODEL.extend((gan, logmel, gcfg["sampling_rate"]))
    gan, logmel, sr = _MODEL
    g = torch.Generator().manual_seed(99)
    audio = (0.1 * torch.randn(batch, sr, generator=g)).clamp_(-1, 1).to(dev)
    lens = torch.full((batch,), sr, dtype=torch.int64)
    g_params, d_params = list(gan.generator.parameters()), list(gan.discriminator.parameters())

    def stage2():
        for disc, params in ((True, d_params), (False, g_params)):
            for p in params:
                p.grad = None
            loss, _ = harness.compute_loss_stage2(audio, lens, gan, logmel, 1, train_disc=disc)
            loss.backward()
            ops.bump_weight_epoch(params)
            ops.rebuild_derived(params)
    return stage2


def traced_dgrads(ops, dev, batch):
    """[(S, Hout, Hin)] of every data gradient of the 32 -> 128 layer that one stage-2 step at `batch` clips issues, in
    order -- taken from the calls fused_disc._conv1d_dgrad receives, not restated here"""
    from flow2gan_amd import fused_disc as FD
    seen, real = [], FD._conv1d_dgrad

    def watch(g_pre, S, Hout, Cout, w, stride, pad, Hin, **kw):
        if (w.shape[2] * w.shape[3], stride, pad, w.shape[1], Cout) == (5, 3, 2, 32, 128):
            seen.append((S, Hout, Hin))
        return real(g_pre, S, Hout, Cout, w, stride, pad, Hin, **kw)
    FD._conv1d_dgrad = watch
    try:
        stage2_of(ops, dev, batch)()
        torch.cuda.synchronize()
    finally:
        FD._conv1d_dgrad = real
    return seen


def time_legs(legs, blocks=3, reps=12):
    """{leg: [per-call microseconds, one entry per block]}, the legs alternating block by block; legs = [(name, enter,
    fn)], enter() sets the leg's mode and tunables"""
    per = {name: [] for name, _, _ in legs}
    for name, enter, fn in legs:            # warm-up: code objects, weight images
        enter()
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for name, enter, fn in legs:
            enter()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            per[name].append(s.elapsed_time(e) * 1e3 / reps)
    return per


def tapn3_table(ops, dev, say, min_rows):
    """the data gradient of the 32 -> 128 layer at the shapes a stage-2 step issues it, three legs alternating in one
    process, three blocks of 12 each: the three launches both modes run as shipped (leg "x6n": gemm_x6n_kernel from
    ops.X6F_TALL_ROWS rows on, the exact-fp32 kernel below; the row names it), the three gemm_h3pn_kernel launches, the one gemm_h3pn3_kernel launch.  No mask, no column sums (as --tapn); the output map
    is allocated and its halo zeroed outside the timed region"""
    from flow2gan_amd import fused_disc as FD
    Cin, Cout = FD.MPD_CH[1], FD.MPD_CH[2]
    say("# per data gradient: median us of 3 alternating blocks of 12, min..max of the leg's blocks, and the bytes of the "
        "gradient map the leg's launches read per second (TB/s; the README's streaming figure is 5.5-5.8) -- x6n and "
        "h3pn read the map three times, h3pn3 once")
    say("batch     S  Hout   Hin    rows   x6n_us  min..max         TB/s   h3pn_us  min..max         TB/s  h3pn3_us  "
        "min..max         TB/s  h3pn3/x6n  verdict kernel of the x6n leg")
    verdicts = []
    for batch in (B, 16):
        for S, Hout, Hin in traced_dgrads(ops, dev, batch):
            g = torch.Generator().manual_seed(S + Hin)
            gpre = FD._halo_rows(S, Hout, Cout, dev)
            FD.unhalo(gpre, S, Hout).copy_((torch.randn(S, Hout, Cout, generator=g) * 1e-3).to(dev))
            gx = FD._halo_rows(S, Hin, Cin, dev)
            w = torch.nn.Parameter((torch.randn(Cout, Cin, 5, 1, generator=g) * (5 * Cin) ** -0.5).to(dev))
            launches = [(FD._dgrad_weight(w, 3, j0, nt), (nt - 1) - e0 - FD.HALO, nt, Lq,
                         (Lq, (Hin + 2 * FD.HALO) * Cin, 3 * Cin, (FD.HALO + rho) * Cin))
                        for rho, j0, nt, e0, Lq in FD._residues(5, 3, 2, Hin) if Lq]

            def three(S=S, Hout=Hout, gpre=gpre, gx=gx, launches=launches):
                for wq, pad, nt, Lq, rm in launches:
                    ops.gemm(ops.win1d(gpre, S, Hout + 2 * FD.HALO, Cout, Lq, 1, pad, nt), ops.mat(wq), gx, rowmap=rm)

            def one(S=S, Hout=Hout, Hin=Hin, gpre=gpre, gx=gx, w=w):
                assert FD._conv1d_dgrad3(gpre, S, Hout, Cout, w, Hin, gx, None, None, None)

            def enter(mode, tapn, tapn3):
                def go():
                    ops.set_gemm_precision(mode)
                    ops.FP16X3_TAPN_MIN_ROWS, ops.FP16X3_TAPN3_MIN_ROWS = tapn, tapn3
                return go
            legs = [("x6n", enter("bf16x6", ops.FP16X3_TAP_OFF, ops.FP16X3_TAP_OFF), three),
                    ("h3pn", enter("fp16x3", min_rows, ops.FP16X3_TAP_OFF), three),
                    ("h3pn3", enter("fp16x3", ops.FP16X3_TAP_OFF, min_rows), one)]
            kern = {}
            for name, go, fn in legs:           # (which kernel each leg really runs)
                go(), fn()
                kern[name] = ops.L.lib.f2g_gemm_last_kernel().decode()
            # (the first leg is whatever the bf16x6 mode launches: gemm_x6n_kernel from ops.X6F_TALL_ROWS rows on, the
            # exact-fp32 kernels below -- the row names it)
            assert kern["h3pn"].startswith("h3pn<") and kern["h3pn3"] == "h3pn3", kern
            per = time_legs(legs)
            read3 = sum(S * (l[3] + l[2] - 1) for l in launches) * Cout * 4
            read1 = S * (Hout + 1) * Cout * 4
            cols, med = "", {}
            for name, nbytes in (("x6n", read3), ("h3pn", read3), ("h3pn3", read1)):
                m = med[name] = med_spread(per[name])[0]
                cols += f" {m:8.1f}  {min(per[name]):6.1f}..{max(per[name]):6.1f}  {nbytes / m * 1e-6:7.2f} "
            lo, hi = (min(per["h3pn3"]), max(per["h3pn3"])), (min(per["x6n"]), max(per["x6n"]))
            verdict = "wins" if lo[1] < hi[0] else ("loses" if lo[0] > hi[1] else "inside")
            verdicts.append(verdict)
            say(f"{batch:5d} {S:5d} {Hout:5d} {Hin:5d} {S * Hout:7d} {cols} {med['h3pn3'] / med['x6n']:8.3f}  {verdict:7s} {kern['x6n']}")
            del gpre, gx
            torch.cuda.empty_cache()
    say(f"# data gradients: {len(verdicts)}; h3pn3 against the three x6n launches, beyond both legs' ranges: wins "
        f"{verdicts.count('wins')}, loses {verdicts.count('loses')}, inside {verdicts.count('inside')}")


def steps_table(ops, dev, say, min_rows, steps=4, tap3=False, route="TAP3"):
    stage2 = stage2_of(ops, dev)

    legs = (("bf16x6", "bf16x6", ops.FP16X3_TAP_OFF), ("fp16x3 route off", "fp16x3", ops.FP16X3_TAP_OFF),
            ("fp16x3 route on", "fp16x3", min_rows))
    if tap3:        # the fp16x3 mode as shipped, the stride-3 tunable alone differing: three alternating pairs
        legs, counter, blocks = legs[1:], f"FP16X3_{route}_LAUNCHES", 3
    else:
        counter, blocks = "FP16X3_TAP_LAUNCHES", 7

    def enter(leg):
        ops.set_gemm_precision(leg[1])
        if tap3:
            setattr(ops, f"FP16X3_{route}_MIN_ROWS", leg[2])
        else:
            ops.FP16X3_TAP_MIN_ROWS = leg[2]

    per = {leg[0]: [] for leg in legs}
    launches = {leg[0]: 0 for leg in legs}
    for leg in legs:
        enter(leg)
        stage2(), stage2()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for leg in legs:
            enter(leg)
            n0 = getattr(ops, counter)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                stage2()
            torch.cuda.synchronize()
            per[leg[0]].append((time.perf_counter() - t0) * 1e3 / steps)
            launches[leg[0]] = max(launches[leg[0]], (getattr(ops, counter) - n0) // steps)
    say(f"# stage-2 step: medians of {blocks} alternating blocks of 4 steps per leg; spread = (max - min) / median")
    if tap3:
        say("stage-2 step        ms   min..max of the leg's blocks   stride-3 route launches per step")
        for leg in legs:
            say(f"{leg[0]:17s} {med_spread(per[leg[0]])[0]:7.2f}   {min(per[leg[0]]):7.2f}..{max(per[leg[0]]):7.2f}"
                f"                  {launches[leg[0]]}")
    else:
        say("stage-2 step        ms  spread  ratio to bf16x6  tap-route launches per step")
        base = med_spread(per["bf16x6"])[0]
        for leg in legs:
            m, s = med_spread(per[leg[0]])
            say(f"{leg[0]:17s} {m:7.2f} {s:7.3f} {m / base:8.3f}          {launches[leg[0]]}")
    off, on = med_spread(per["fp16x3 route off"]), med_spread(per["fp16x3 route on"])
    say(f"# route on / route off (the same mode, the route alone differing): {on[0] / off[0]:.3f} "
        f"(spreads {on[1]:.3f} / {off[1]:.3f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/fp16x3_tap_shapes.txt (--tap3: fp16x3_tap3_shapes.txt)")
    ap.add_argument("--tap3", action="store_true", help="measure the stride-3 route (legs fwd3 / fwd4) instead")
    ap.add_argument("--tap3n", action="store_true", help="measure the 32-channel stride-3 route (legs fwd2 / fwd2-) instead")
    ap.add_argument("--tapn", action="store_true", help="measure the route of the 32 -> 128 layer's residue data gradients (leg dgrad2) instead")
    ap.add_argument("--tapn3", action="store_true", help="measure that data gradient as ONE launch over its three residues instead")
    ap.add_argument("--append", action="store_true", help="add this run's table to --out instead of replacing it")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--no-shapes", action="store_true")
    ap.add_argument("--min-rows", type=int, default=1, help="ops.FP16X3_TAP_MIN_ROWS for this run (1: every launch "
                    "of the table on the new kernel)")
    args = ap.parse_args()
    if args.tap3 + args.tap3n + args.tapn + args.tapn3 > 1:
        ap.error("--tap3, --tap3n, --tapn and --tapn3 are separate runs")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "fp16x3_tapn3_shapes.txt" if args.tapn3 else "fp16x3_tapn_shapes.txt" if args.tapn else "fp16x3_tap3n_shapes.txt" if args.tap3n else (
            "fp16x3_tap3_shapes.txt" if args.tap3 else "fp16x3_tap_shapes.txt"))
    assert torch.cuda.is_available(), "needs an MI355X"
    from flow2gan_amd import ops
    if args.min_rows < 1 or args.min_rows >= ops.FP16X3_TAP_OFF:
        ap.error("--min-rows must enable the route: both modes would time the same bf16x6 launch otherwise")
    was_rows, was_rows3, was_rows3n = ops.FP16X3_TAP_MIN_ROWS, ops.FP16X3_TAP3_MIN_ROWS, ops.FP16X3_TAP3N_MIN_ROWS
    was_rowsn, was_rowsn3 = ops.FP16X3_TAPN_MIN_ROWS, ops.FP16X3_TAPN3_MIN_ROWS
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    given = [a for i, a in enumerate(sys.argv[1:], 1) if a != "--out" and sys.argv[i - 1] != "--out"]
    say("# command (the output path aside): python tools/fp16x3_tap_shapes.py " + " ".join(given))
    say(f"# tools/fp16x3_tap_shapes.py  {ops.L.version()}  "
        + (f"FP16X3_TAPN3_MIN_ROWS={args.min_rows} FP16X3_TAPN_MIN_ROWS={was_rowsn} FP16X3_TAP3N_MIN_ROWS={was_rows3n} "
           f"FP16X3_TAP3_MIN_ROWS={was_rows3} FP16X3_TAP_MIN_ROWS={was_rows} " if args.tapn3 else
           f"FP16X3_TAPN_MIN_ROWS={args.min_rows} FP16X3_TAP3N_MIN_ROWS={was_rows3n} FP16X3_TAP3_MIN_ROWS={was_rows3} "
           f"FP16X3_TAP_MIN_ROWS={was_rows} " if args.tapn else
           f"FP16X3_TAP3N_MIN_ROWS={args.min_rows} FP16X3_TAP3_MIN_ROWS={was_rows3} FP16X3_TAP_MIN_ROWS={was_rows} "
           if args.tap3n else
           f"FP16X3_TAP3_MIN_ROWS={args.min_rows} FP16X3_TAP_MIN_ROWS={was_rows} " if args.tap3 else
           f"FP16X3_TAP_MIN_ROWS={args.min_rows} ") + f"X6_MIN_K={ops.X6_MIN_K}  {torch.cuda.get_device_name(0)}")
    if not args.tapn3:      # (--tapn3 has three legs and states its own method above its table)
        say("# per-launch medians of 5 alternating blocks of 12 launches (us), "
            + ("the fp16x3 leg has no image pass (the kernel scales the fp32 map itself)" if args.tap3n or args.tapn else
               "the map's image pass included in the fp16x3 leg") + "; spread = (max - min) / median of a mode's blocks; ratio = fp16x3 / bf16x6 (< 1: fp16x3 faster)")
    from test_hip_gemm_f16 import mode_name       # (the one place that names the mode in force)
    was = mode_name(ops)
    try:
        if not args.no_shapes and args.tapn3:
            tapn3_table(ops, dev, say, args.min_rows)
        elif not args.no_shapes and args.tapn:
            ops.FP16X3_TAPN_MIN_ROWS = args.min_rows
            shapes3_table(ops, dev, say, "FP16X3_TAPN_LAUNCHES", casesn, ((B, PERIODS), (16, PERIODS)))
        elif not args.no_shapes and args.tap3n:
            ops.FP16X3_TAP3N_MIN_ROWS = args.min_rows
            shapes3_table(ops, dev, say, "FP16X3_TAP3N_LAUNCHES", cases3n, ((B, PERIODS), (16, PERIODS)))
        elif not args.no_shapes and args.tap3:
            ops.FP16X3_TAP3_MIN_ROWS = args.min_rows
            shapes3_table(ops, dev, say)
        elif not args.no_shapes:
            ops.FP16X3_TAP_MIN_ROWS = args.min_rows
            shapes_table(ops, dev, say)
        if not args.no_steps:
            steps_table(ops, dev, say, args.min_rows, tap3=args.tap3 or args.tap3n or args.tapn or args.tapn3,
                        route="TAPN3" if args.tapn3 else "TAPN" if args.tapn else ("TAP3N" if args.tap3n else "TAP3"))
    finally:
        ops.FP16X3_TAP_MIN_ROWS, ops.FP16X3_TAP3_MIN_ROWS, ops.FP16X3_TAP3N_MIN_ROWS = was_rows, was_rows3, was_rows3n
        ops.FP16X3_TAPN_MIN_ROWS, ops.FP16X3_TAPN3_MIN_ROWS = was_rowsn, was_rowsn3
        ops.set_gemm_precision(was)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(("#\n# ---- another run of the same tool\n" if args.append else "") + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
