#!/usr/bin/env python
"""fp16x3 against bf16x6 on the weight gradient of the MPD's stride-1 layer and on the stage-2 step -- one box, one
process.

Per period (2, 3, 5, 7, 11) at B = 64 and B = 16 x 1 s of 24 kHz audio, real and generated halves together (S = 2 B p
sequences): the weight gradient of the 1024 -> 1024 five-tap stride-1 layer, ops.wgrad over unbounded windows of the
halo map (1024 x 5120 outputs, reduction over all S (H + 4) rows of the padded gradient map), timed in both modes, the
modes ALTERNATING block by block (time_blocks / med_spread of tools/fp16x3_shapes.py), with everything a launch costs
in its mode inside the timed region: fp16x3 = the two f2g_split_f16x2_cols image calls (gradient and map: two kernels
each) plus gemm_h3wt_kernel; bf16x6 = gemm_leanw6t_kernel, which splits the fp32 operands itself.

Then the stage-2 step as tools/fp16x3_shapes.py runs it, in the fp16x3 mode, in two legs that alternate block by
block: the route off and on (the tap route of the forward and data gradient stays at its default in both).

The tool, whose purpose is to measure the route, sets the threshold itself: --min-rows, default 1 = every launch the
library accepts goes to the new kernel.  The header of the output states the command it was made with.

--step3 measures the weight gradient of the two STRIDE-3 layers instead (gemm_h3ws_kernel against gemm_leanw6s_kernel,
ops.FP16X3_TAPW3_MIN_ROWS; default output profiles/fp16x3_tapw3_shapes.txt), the stride-1 route staying as shipped:
  wgrad3  the 128 -> 512 layer (512 x 640 outputs; the map has heights(p)[2] rows per sequence, the gradient
          heights(p)[3])
  wgrad4  the 512 -> 1024 layer (1024 x 2560 outputs; heights(p)[3] -> heights(p)[4])
per period at B = 64 and B = 16 under the same timing conditions (both image calls inside the fp16x3 leg), then the
stage-2 step in the fp16x3 mode with that tunable alone differing, in three alternating pairs of blocks, reported as
medians and within-leg ranges.

--step3n measures the weight gradient of the 32 -> 128 STRIDE-3 layer on the kernel that scales both fp32 operands
inside itself (gemm_h3wsn_kernel, ops.FP16X3_TAPW3N_MIN_ROWS; default output profiles/fp16x3_tapw3n_shapes.txt): leg
wgrad2 (128 x 160 outputs; the map has heights(p)[1] rows per sequence, the gradient heights(p)[2]) per period at B = 64
and B = 16.  Both legs run in the fp16x3 mode with that tunable alone differing -- off, the library launches what it
launched before the kernel existed, and the table names it --, in three alternating blocks of 12 launches per leg,
reported as medians and within-leg ranges, with the bytes per second of reading both operands once.  Then the stage-2
step as for --step3.

    python tools/fp16x3_tapw_shapes.py [--out profiles/fp16x3_tapw_shapes.txt] [--append] [--no-shapes] [--no-steps]
                                       [--min-rows R] [--step3 | --step3n]
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
from fp16x3_tap_shapes import PERIODS, T, heights  # noqa: E402

BATCHES = (64, 16)
CH = 1024


def case(ops, FD, p, dev, batch):
    """(reduction rows, fn) of period p at `batch` clips; the operands are allocated here, outside the timed region"""
    S, H = 2 * batch * p, heights(p)[4]
    Hp = H + 2 * FD.HALO
    g = torch.Generator().manual_seed(p)
    x = FD._halo_rows(S, H, CH, dev)
    FD.unhalo(x, S, H).copy_(torch.randn(S, H, CH, generator=g).to(dev))
    gy = FD._halo_rows(S, H, CH, dev)
    FD.unhalo(gy, S, H).copy_((torch.randn(S, H, CH, generator=g) * 1e-3).to(dev))
    gw = torch.zeros(CH, 5 * CH, device=dev)

    def fn():
        ops.wgrad(gy, CH, CH, ops.win1d(x, S, Hp, CH, Hp, 1, FD.HALO, 5, unbounded=True), gw)
    return S * Hp, fn


def case3(ops, FD, p, dev, batch, l):
    """(reduction rows, Cin, Cout, fn) of the stride-3 layer l (2: 128 -> 512, 3: 512 -> 1024) of period p at `batch`
    clips; the operands are allocated here, outside the timed region"""
    S, hs = 2 * batch * p, heights(p)
    Cin, Cout, H, Hout = FD.MPD_CH[l], FD.MPD_CH[l + 1], hs[l], hs[l + 1]
    Hp = Hout + 2 * FD.HALO
    g = torch.Generator().manual_seed(10 * p + l)
    x = FD._halo_rows(S, H, Cin, dev)
    FD.unhalo(x, S, H).copy_(torch.randn(S, H, Cin, generator=g).to(dev))
    gy = FD._halo_rows(S, Hout, Cout, dev)
    FD.unhalo(gy, S, Hout).copy_((torch.randn(S, Hout, Cout, generator=g) * 1e-3).to(dev))
    gw = torch.zeros(Cout, 5 * Cin, device=dev)

    def fn():
        ops.wgrad(gy, Cout, Cout, ops.win1d(x, S, H + 2 * FD.HALO, Cin, Hp, 3, 3 * FD.HALO, 5, unbounded=True), gw)
    return S * Hp, Cin, Cout, fn


def shapes3_table(ops, dev, say):
    from flow2gan_amd import fused_disc as FD
    say("batch period  launch     rows  bf16x6_us  spread  fp16x3_us  spread  ratio  beyond spread  TFLOP/s(fp16x3)  "
        "kernels")
    seen = []
    for batch in BATCHES:
        for p in PERIODS:
            for name, l in (("wgrad3", 2), ("wgrad4", 3)):
                rows, Cin, Cout, fn = case3(ops, FD, p, dev, batch, l)
                n0 = ops.FP16X3_TAPW3_LAUNCHES
                per, kern = time_blocks(ops, fn)
                assert ops.FP16X3_TAPW3_LAUNCHES > n0 and kern["fp16x3"].startswith("h3ws"), \
                    f"B {batch} period {p} {name}: the fp16x3 leg never took the route"
                (a, sa), (b, sb) = med_spread(per["bf16x6"]), med_spread(per["fp16x3"])
                verdict = "wins" if b / a < 1.0 - max(sa, sb) else ("loses" if b / a > 1.0 + max(sa, sb) else "inside")
                say(f"{batch:5d} {p:6d}  {name:7s} {rows:7d} {a:10.1f} {sa:7.3f} {b:10.1f} {sb:7.3f} {b / a:6.3f}  "
                    f"{verdict:13s} {2.0 * rows * Cout * 5 * Cin / b * 1e-6:12.1f}      "
                    f"{kern['bf16x6']} | {kern['fp16x3']}")
                seen.append(verdict)
                del fn
                torch.cuda.empty_cache()
    say(f"# launches: {len(seen)}; fp16x3 wins by more than the spread: {seen.count('wins')}, loses by more than the "
        f"spread: {seen.count('loses')}, inside the spread: {seen.count('inside')}")


def shapes3n_table(ops, dev, say, min_rows, blocks=3, reps=12):
    """the 32 -> 128 layer: the route off and on in the fp16x3 mode, the legs alternating block by block"""
    import statistics
    from flow2gan_amd import fused_disc as FD
    ops.set_gemm_precision("fp16x3")
    legs = (("off", ops.FP16X3_TAP_OFF), ("on", min_rows))
    say("batch period  launch     rows     MB   off_us   min..max     on_us   min..max  ratio  beyond ranges  "
        "GB/s(on)  kernels off | on")
    seen = []
    for batch in BATCHES:
        for p in PERIODS:
            rows, Cin, Cout, fn = case3(ops, FD, p, dev, batch, 1)
            S, H = 2 * batch * p, heights(p)[1]
            mb = (rows * Cout + S * (H + 2 * FD.HALO) * Cin) * 4e-6
            per, kern = {k: [] for k, _ in legs}, {}
            for k, r in legs:               # warm-up: code objects
                ops.FP16X3_TAPW3N_MIN_ROWS = r
                n0 = ops.FP16X3_TAPW3N_LAUNCHES
                for _ in range(3):
                    fn()
                kern[k] = ops.L.lib.f2g_gemm_last_kernel().decode()
                assert (ops.FP16X3_TAPW3N_LAUNCHES > n0) == (k == "on"), f"B {batch} period {p}: leg {k}"
            assert kern["on"].startswith("h3wsn") and not kern["off"].startswith("h3")
            torch.cuda.synchronize()
            for _ in range(blocks):
                for k, r in legs:
                    ops.FP16X3_TAPW3N_MIN_ROWS = r
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for _ in range(reps):
                        fn()
                    e.record()
                    torch.cuda.synchronize()
                    per[k].append(s.elapsed_time(e) * 1e3 / reps)
            a, b = statistics.median(per["off"]), statistics.median(per["on"])
            verdict = "wins" if max(per["on"]) < min(per["off"]) else \
                ("loses" if min(per["on"]) > max(per["off"]) else "inside")
            say(f"{batch:5d} {p:6d}  wgrad2  {rows:7d} {mb:6.1f} {a:8.1f} {min(per['off']):6.1f}..{max(per['off']):<6.1f}"
                f" {b:8.1f} {min(per['on']):6.1f}..{max(per['on']):<6.1f} {b / a:6.3f}  {verdict:13s} {mb / b * 1e3:8.0f}  "
                f"{kern['off']} | {kern['on']}")
            seen.append(verdict)
            del fn
            torch.cuda.empty_cache()
    say(f"# launches: {len(seen)}; the route wins beyond the legs' ranges: {seen.count('wins')}, loses beyond them: "
        f"{seen.count('loses')}, ranges overlap: {seen.count('inside')}")


def shapes_table(ops, dev, say):
    from flow2gan_amd import fused_disc as FD
    say("batch period     rows  bf16x6_us  spread  fp16x3_us  spread  ratio  TFLOP/s(fp16x3)  kernels")
    seen = []
    for batch in BATCHES:
        for p in PERIODS:
            rows, fn = case(ops, FD, p, dev, batch)
            n0 = ops.FP16X3_TAPW_LAUNCHES
            per, kern = time_blocks(ops, fn)
            assert ops.FP16X3_TAPW_LAUNCHES > n0, f"B {batch} period {p}: the fp16x3 leg never took the route"
            (a, sa), (b, sb) = med_spread(per["bf16x6"]), med_spread(per["fp16x3"])
            say(f"{batch:5d} {p:6d} {rows:8d} {a:10.1f} {sa:7.3f} {b:10.1f} {sb:7.3f} {b / a:6.3f} "
                f"{2.0 * rows * CH * 5 * CH / b * 1e-6:12.1f}      {kern['bf16x6']} | {kern['fp16x3']}")
            seen.append((b / a, max(sa, sb), batch, p, rows))
            del fn
            torch.cuda.empty_cache()
    won = [w for w in seen if w[0] < 1.0 - w[1]]
    lost = [w for w in seen if w[0] > 1.0 + w[1]]
    for name, some in (("wins", won), ("loses", lost)):
        say(f"# launches where fp16x3 {name} by more than the spread: {len(some)} of {len(seen)}"
            + "".join(f"\n#   B {bb} period {p} rows {r}: ratio {q:.3f}, spread {s:.3f}" for q, s, bb, p, r in some))
    if len(won) == len(seen):
        say(f"# every accepted launch wins by more than its spread; fewest reduction rows measured: "
            f"{min(w[4] for w in seen)} (the rule used for fp16x3_tap_min_rows would turn the route on from there)")
    else:
        say("# not every accepted launch wins by more than its spread: the default stays off")


def steps_table(ops, dev, say, min_rows, steps=4, step3=False, step3n=False):
    import flow2gan_amd
    from flow2gan_amd import harness
    from flow2gan_amd.models.config import get_gan_config, get_generator_config
    from flow2gan_amd.models.gan import GAN
    gcfg = get_generator_config("mel_24k_base")
    sr, B = gcfg["sampling_rate"], 64
    torch.manual_seed(1234)
    gen = flow2gan_amd.MelAudioGenerator(**gcfg)
    gen.branch_dropout = 0.0
    gan = GAN(gen, **get_gan_config("gan_multi_scale_mel_recon")).to(dev)
    logmel = flow2gan_amd.LogMelSpectrogram(sr, gcfg["mel_n_fft"], gcfg["mel_hop_length"], gcfg["n_mels"]).to(dev)
    g = torch.Generator().manual_seed(99)
    audio = (0.1 * torch.randn(B, sr, generator=g)).clamp_(-1, 1).to(dev)
    lens = torch.full((B,), sr, dtype=torch.int64)
    g_params, d_params = list(gan.generator.parameters()), list(gan.discriminator.parameters())

    def stage2():
        for disc, params in ((True, d_params), (False, g_params)):
            for p in params:
                p.grad = None
            loss, _ = harness.compute_loss_stage2(audio, lens, gan, logmel, 1, train_disc=disc)
            loss.backward()
            ops.bump_weight_epoch(params)
            ops.rebuild_derived(params)

    legs = (("fp16x3 route off", ops.FP16X3_TAP_OFF), ("fp16x3 route on", min_rows))
    ops.set_gemm_precision("fp16x3")
    # (--step3: the stride-3 tunable alone differing, three alternating pairs)
    tunable, counter, blocks = ("FP16X3_TAPW3_MIN_ROWS", "FP16X3_TAPW3_LAUNCHES", 3) if step3 else \
        ("FP16X3_TAPW_MIN_ROWS", "FP16X3_TAPW_LAUNCHES", 7)
    if step3n:
        tunable, counter, blocks, step3 = "FP16X3_TAPW3N_MIN_ROWS", "FP16X3_TAPW3N_LAUNCHES", 3, True
    per = {leg[0]: [] for leg in legs}
    launches = {leg[0]: 0 for leg in legs}
    for name, rows in legs:
        setattr(ops, tunable, rows)
        stage2(), stage2()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for name, rows in legs:
            setattr(ops, tunable, rows)
            n0 = getattr(ops, counter)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                stage2()
            torch.cuda.synchronize()
            per[name].append((time.perf_counter() - t0) * 1e3 / steps)
            launches[name] = max(launches[name], (getattr(ops, counter) - n0) // steps)
    say(f"# stage-2 step (B = 64, fp16x3 mode): medians of {blocks} alternating blocks of 4 steps per leg; spread = "
        "(max - min) / median")
    if step3:
        say("stage-2 step        ms   min..max of the leg's blocks   stride-3 weight-gradient launches per step")
        for name, _ in legs:
            say(f"{name:17s} {med_spread(per[name])[0]:7.2f}   {min(per[name]):7.2f}..{max(per[name]):7.2f}"
                f"                  {launches[name]}")
    else:
        say("stage-2 step        ms  spread  tap-walking weight-gradient launches per step")
        for name, _ in legs:
            m, s = med_spread(per[name])
            say(f"{name:17s} {m:7.2f} {s:7.3f}      {launches[name]}")
    off, on = med_spread(per["fp16x3 route off"]), med_spread(per["fp16x3 route on"])
    say(f"# route on / route off: {on[0] / off[0]:.3f} (spreads {on[1]:.3f} / {off[1]:.3f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/fp16x3_tapw_shapes.txt (--step3: "
                    "fp16x3_tapw3_shapes.txt)")
    ap.add_argument("--step3", action="store_true", help="measure the stride-3 layers' weight gradient (legs wgrad3 / "
                    "wgrad4) instead")
    ap.add_argument("--step3n", action="store_true", help="measure the 32 -> 128 stride-3 layer's weight gradient on "
                    "the kernel that scales the fp32 operands itself (leg wgrad2) instead")
    ap.add_argument("--append", action="store_true", help="add this run's table to --out instead of replacing it")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--no-shapes", action="store_true")
    ap.add_argument("--min-rows", type=int, default=1, help="ops.FP16X3_TAPW_MIN_ROWS for this run (1: every launch "
                    "of the table on the new kernel)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "fp16x3_tapw3n_shapes.txt" if args.step3n else
                                "fp16x3_tapw3_shapes.txt" if args.step3 else "fp16x3_tapw_shapes.txt")
    assert torch.cuda.is_available(), "needs an MI355X"
    from flow2gan_amd import ops
    if args.min_rows < 1 or args.min_rows >= ops.FP16X3_TAP_OFF:
        ap.error("--min-rows must enable the route: both modes would time the same bf16x6 launch otherwise")
    was_rows, was_rows3, was_rows3n = ops.FP16X3_TAPW_MIN_ROWS, ops.FP16X3_TAPW3_MIN_ROWS, ops.FP16X3_TAPW3N_MIN_ROWS
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    given = [a for i, a in enumerate(sys.argv[1:], 1) if a != "--out" and sys.argv[i - 1] != "--out"]
    say("# command (the output path aside): python tools/fp16x3_tapw_shapes.py " + " ".join(given))
    say(f"# tools/fp16x3_tapw_shapes.py  {ops.L.version()}  "
        + (f"FP16X3_TAPW3N_MIN_ROWS={args.min_rows} FP16X3_TAPW3_MIN_ROWS={was_rows3} FP16X3_TAPW_MIN_ROWS={was_rows}"
           if args.step3n else
           f"FP16X3_TAPW3_MIN_ROWS={args.min_rows} FP16X3_TAPW_MIN_ROWS={was_rows}" if args.step3 else
           f"FP16X3_TAPW_MIN_ROWS={args.min_rows}") + f"  {torch.cuda.get_device_name(0)}")
    if args.step3n:
        say("# per-launch medians and ranges of 3 alternating blocks of 12 launches (us) per leg, both legs in the fp16x3 "
            "mode: off = the tunable at its default, on = at --min-rows; ratio = on / off (< 1: the route faster); MB = "
            "both fp32 operands read once")
    else:
        say("# per-launch medians of 5 alternating blocks of 12 launches (us), both column-image calls included in the "
            "fp16x3 leg; spread = (max - min) / median of a mode's blocks; ratio = fp16x3 / bf16x6 (< 1: fp16x3 faster)")
    from test_hip_gemm_f16 import mode_name       # (the one place that names the mode in force)
    was = mode_name(ops)
    try:
        if not args.no_shapes and args.step3n:
            shapes3n_table(ops, dev, say, args.min_rows)
        elif not args.no_shapes and args.step3:
            ops.FP16X3_TAPW3_MIN_ROWS = args.min_rows
            shapes3_table(ops, dev, say)
        elif not args.no_shapes:
            ops.FP16X3_TAPW_MIN_ROWS = args.min_rows
            shapes_table(ops, dev, say)
        if not args.no_steps:
            steps_table(ops, dev, say, args.min_rows, step3=args.step3, step3n=args.step3n)
    finally:
        ops.FP16X3_TAPW_MIN_ROWS, ops.FP16X3_TAPW3_MIN_ROWS, ops.FP16X3_TAPW3N_MIN_ROWS = was_rows, was_rows3, was_rows3n
        ops.set_gemm_precision(was)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(("#\n# ---- another run of the same tool\n" if args.append else "") + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
