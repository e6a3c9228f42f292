#!/usr/bin/env python
"""The fused ConvNeXt-block backward (f2g_dwblock_bwd, F2G_OPTS=dw_bwd_fused=1) against the two launches it replaces
(f2g_dwnorm_bwd + f2g_dwconv_bwd), per launch and per step -- one box, one process, one library.

Shapes: the tool TRACES them.  One stage-1 step of mel_24k_base (B = 2 x 1 s of 24 kHz audio) runs with a recorder
round fused.block_bwd; every distinct (C, F, up, Fc, condition, time embedding, row strides of the stacked condition /
time tensors) it sees is a row of the table, at B = 64 and B = 16 (the frame counts do not depend on B).

Per shape, two legs on the same tensors, ALTERNATING, three runs of --reps launches each, timed with events:
  pair   ops.empty(du) + ops.dwnorm_bwd + ops.empty(gx) + ops.dwconv_bwd   (as fused.block_bwd issues them: each with
         its workspace allocation and its second-stage reduction launch)
  fused  ops.empty(gx) + ops.dwblock_bwd                                   (workspace allocation and reduction launch
         included)
The table gives each leg's median and range in us, fused / pair, the verdict (a win or a loss is one beyond BOTH legs'
ranges) and the fused leg's bytes per second over x, gz, gres read and gx written once.

Then the stage-1 step and the stage-2 step (D-step + G-step) at B = 64 in the bf16x6 mode, the tunable alone
differing: three alternating pairs of blocks of four steps, medians and ranges per leg.

    python tools/dwblock_bwd_shapes.py [--out profiles/dwblock_bwd.txt] [--append] [--no-shapes] [--no-steps]
                                       [--batches 64,16] [--reps 20]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def trace_shapes(dev):
    """distinct block_bwd shapes of one stage-1 step, in the order they first run"""
    import flow2gan_amd
    from flow2gan_amd import fused, harness
    from flow2gan_amd.models.config import get_generator_config
    gcfg = get_generator_config("mel_24k_base")
    sr, B = gcfg["sampling_rate"], 2
    torch.manual_seed(1234)
    gen = flow2gan_amd.MelAudioGenerator(**gcfg).to(dev).train()
    logmel = flow2gan_amd.LogMelSpectrogram(sr, gcfg["mel_n_fft"], gcfg["mel_hop_length"], gcfg["n_mels"]).to(dev)
    audio = (0.1 * torch.randn(B, sr, generator=torch.Generator().manual_seed(99))).clamp_(-1, 1).to(dev)
    lens = torch.full((B,), sr, dtype=torch.int64)
    seen, real = {}, fused.block_bwd

    def recorder(bp, x, z, a, gout, B_, F, lens_, ln, lsc, cproj=None, ldcp=0, Fc=0, up=1, cp_off=0, te=None, ldte=0,
                 te_off=0, g_cproj=None, g_te=None, g_cproj_store=False):
        key = (bp.C, bp.K, F, up if cproj is not None else 1, Fc, cproj is not None, te is not None, ldcp, ldte,
               lens_ is not None, bool(g_cproj_store))
        seen[key] = seen.get(key, 0) + 1
        return real(bp, x, z, a, gout, B_, F, lens_, ln, lsc, cproj, ldcp, Fc, up, cp_off, te, ldte, te_off, g_cproj,
                    g_te, g_cproj_store)

    fused.block_bwd = recorder
    try:
        loss, _ = harness.compute_loss_stage1(audio, lens, logmel, gen)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        fused.block_bwd = real
    del gen, logmel
    torch.cuda.empty_cache()
    return seen


def case(ops, key, B, dev):
    """the two legs of one traced shape at batch B on the same tensors (allocated here, outside the timed region)"""
    C, K, F, up, Fc, cond, has_te, ldcp, ldte, has_lens, store = key
    g = torch.Generator().manual_seed(C + F)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dev)
    rows = B * F
    x, gz, gres = rn(rows, C), rn(rows, C), rn(rows, C)
    w_dw, b_dw, beta, ls, gam = rn(C, 1, K, scale=0.3), rn(C, scale=0.1), rn(C, scale=0.1), torch.tensor([0.7], device=dev), rn(C)
    lens = torch.full((B,), F, dtype=torch.int32, device=dev) if has_lens else None
    cproj = rn(B * Fc, ldcp) if cond else None
    te = rn(B, ldte, scale=0.3) if has_te else None
    g_cp = torch.zeros(B * Fc, ldcp, device=dev) if cond else None
    g_te = torch.zeros(B, ldte, device=dev) if has_te else None
    g_beta, g_ls, g_w, g_b, g_gam = ops.zeros_many([(C,), (1,), (C, 1, K), (C,), (C,)], dev)
    cpa = (cproj, ldcp, Fc, up, 0, te, ldte, 0)
    kw = dict(g_cproj=g_cp, g_te=g_te, g_beta=g_beta, g_log_scale=g_ls, g_cproj_store=store and cond)

    def pair():
        du = ops.empty(rows, C, device=dev)
        ops.dwnorm_bwd(x, gz, du, B, F, C, K, lens, w_dw, b_dw, beta, ls, *cpa, **kw)
        gx = ops.empty(rows, C, device=dev)
        ops.dwconv_bwd(du, x, gx, B, F, C, K, lens, w_dw, gres=gres, gamma=gam, g_w=g_w, g_b=g_b, g_gamma=g_gam)

    def fused_leg():
        gx = ops.empty(rows, C, device=dev)
        ops.dwblock_bwd(x, gz, gx, B, F, C, K, lens, w_dw, b_dw, beta, ls, *cpa, **kw, gres=gres, gamma=gam, g_w=g_w,
                        g_b=g_b, g_gamma=g_gam)

    return pair, fused_leg


def shapes_table(ops, dev, say, shapes, batches, reps, runs=3):
    last = lambda: ops.L.lib.f2g_convnext_last_launch().decode()
    say("batch    C     F  up   Fc cond te launches/step  pair_us   min..max    fused_us   min..max   ratio  verdict  "
        "GB/s(fused)  kernels pair | fused")
    verdicts = []
    for B in batches:
        for key, count in shapes.items():
            C, K, F, up, Fc, cond, has_te = key[:7]
            if not ops.dwblock_bwd_ok(C, K, up, cond):
                say(f"{B:5d} {C:4d} {F:5d} {up:3d}: f2g_dwblock_bwd_ok declines (K = {K}); the pair stays")
                continue
            legs = dict(zip(("pair", "fused"), case(ops, key, B, dev)))
            kern, per = {}, {k: [] for k in legs}
            for k, fn in legs.items():        # warm-up: code objects, allocator
                for _ in range(3):
                    fn()
                kern[k] = last()
            torch.cuda.synchronize()
            for _ in range(runs):
                for k, fn in legs.items():
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for _ in range(reps):
                        fn()
                    e.record()
                    torch.cuda.synchronize()
                    per[k].append(s.elapsed_time(e) * 1e3 / reps)
            a, b = statistics.median(per["pair"]), statistics.median(per["fused"])
            verdict = "wins" if max(per["fused"]) < min(per["pair"]) else \
                ("loses" if min(per["fused"]) > max(per["pair"]) else "inside")
            verdicts.append(verdict)
            say(f"{B:5d} {C:4d} {F:5d} {up:3d} {Fc:4d} {int(cond):4d} {int(has_te):2d} {count:8d}     {a:9.1f} "
                f"{min(per['pair']):6.1f}..{max(per['pair']):<6.1f} {b:9.1f} {min(per['fused']):6.1f}..{max(per['fused']):<6.1f}"
                f" {b / a:6.3f}  {verdict:7s} {16.0 * B * F * C / b * 1e-3:9.0f}    {kern['pair']} | {kern['fused']}")
            del legs
            torch.cuda.empty_cache()
    say(f"# launches: {len(verdicts)}; fused wins beyond both legs' ranges: {verdicts.count('wins')}, loses beyond them: "
        f"{verdicts.count('loses')}, ranges overlap: {verdicts.count('inside')}")


def steps_table(ops, dev, say, steps=4, blocks=3):
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
    audio = (0.1 * torch.randn(B, sr, generator=torch.Generator().manual_seed(99))).clamp_(-1, 1).to(dev)
    lens = torch.full((B,), sr, dtype=torch.int64)
    g_params, d_params = list(gan.generator.parameters()), list(gan.discriminator.parameters())

    def stage1():
        for p in g_params:
            p.grad = None
        loss, _ = harness.compute_loss_stage1(audio, lens, logmel, gan.generator)
        loss.backward()
        ops.bump_weight_epoch(g_params)
        ops.rebuild_derived(g_params)

    def stage2():
        for disc, params in ((True, d_params), (False, g_params)):
            for p in params:
                p.grad = None
            loss, _ = harness.compute_loss_stage2(audio, lens, gan, logmel, 1, train_disc=disc)
            loss.backward()
            ops.bump_weight_epoch(params)
            ops.rebuild_derived(params)

    ops.set_gemm_precision("bf16x6")
    counts = {}
    real = ops.call

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        real(name, *args)

    say(f"# steps (B = {B}, bf16x6 mode): medians and ranges of {blocks} alternating blocks of {steps} steps per leg, "
        "ops.DW_BWD_FUSED alone differing")
    say("step     leg      ms     min..max      f2g_dwblock_bwd / f2g_dwnorm_bwd / f2g_dwconv_bwd calls per step")
    for sname, step in (("stage-1", stage1), ("stage-2", stage2)):
        legs = (("off", False), ("on", True))
        per, calls = {k: [] for k, _ in legs}, {}
        for k, v in legs:
            ops.DW_BWD_FUSED = v
            step()
            counts.clear()
            ops.call = counting
            try:
                step()
            finally:
                ops.call = real
            calls[k] = tuple(counts.get(n, 0) for n in ("f2g_dwblock_bwd", "f2g_dwnorm_bwd", "f2g_dwconv_bwd"))
        torch.cuda.synchronize()
        for _ in range(blocks):
            for k, v in legs:
                ops.DW_BWD_FUSED = v
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    step()
                torch.cuda.synchronize()
                per[k].append((time.perf_counter() - t0) * 1e3 / steps)
        for k, _ in legs:
            say(f"{sname:8s} {k:4s} {statistics.median(per[k]):8.2f}  {min(per[k]):7.2f}..{max(per[k]):<7.2f}     "
                f"{calls[k][0]} / {calls[k][1]} / {calls[k][2]}")
        a, b = statistics.median(per["off"]), statistics.median(per["on"])
        verdict = "wins" if max(per["on"]) < min(per["off"]) else ("loses" if min(per["on"]) > max(per["off"]) else "inside")
        say(f"# {sname}: on - off = {b - a:+.2f} ms ({b / a:.4f}); beyond both legs' ranges: {verdict}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dwblock_bwd.txt"))
    ap.add_argument("--append", action="store_true", help="add this run's table to --out instead of replacing it")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--no-shapes", action="store_true")
    ap.add_argument("--batches", default="64,16")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from flow2gan_amd import ops
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    given = [a for i, a in enumerate(sys.argv[1:], 1) if a != "--out" and sys.argv[i - 1] != "--out"]
    say("# command (the output path aside): python tools/dwblock_bwd_shapes.py " + " ".join(given))
    say(f"# tools/dwblock_bwd_shapes.py  {ops.L.version()}  {torch.cuda.get_device_name(0)}")
    was, was_mode = ops.DW_BWD_FUSED, ops.GEMM_PRECISION
    try:
        if not args.no_shapes:
            shapes = trace_shapes(dev)
            say("# traced block_bwd shapes of one stage-1 step (C, K, F, up, Fc, cond, te, ldcp, ldte, lens, store): calls")
            for key, n in shapes.items():
                say(f"#   {key}: {n}")
            say(f"# per launch: medians and ranges of 3 alternating runs of {args.reps} launches (us) per leg; ratio = "
                "fused / pair (< 1: the one launch faster)")
            shapes_table(ops, dev, say, shapes, [int(b) for b in args.batches.split(",")], args.reps)
        if not args.no_steps:
            steps_table(ops, dev, say)
    finally:
        ops.DW_BWD_FUSED, ops.GEMM_PRECISION = was, was_mode
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(("#\n# ---- another run of the same tool\n" if args.append else "") + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
