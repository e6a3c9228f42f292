#!/usr/bin/env python
"""fp16x3 against bf16x6 on the generator's pointwise GEMM shapes and on the train steps -- one box, one process.

Per shape (rows 6016 / 12032 / 24064 = B 64 x 1 s at the three branch rates; (K, N) of pwconv1 / pwconv2 of the
three branches) and epilogue (forward: bias + fused PReLU with both outputs for K < N, bias + residual * gamma for
K > N; data gradient: PReLU backward with both column sums for K > N, plain for K < N) the launch is timed through
ops.gemm in both modes, the modes ALTERNATING block by block, with everything a launch costs in its mode inside
the timed region: the activation's image pass (f2g_split_f16x2) in fp16x3, the in-kernel split or the image pass
of bf16x6, the partial-column-sum reduction.  The weight images come from the derived-weight cache in both modes
(built once before the timing, as in a step between two optimizer updates).  `spread` is the relative range of a
mode's own per-block medians: a difference smaller than it is not a difference.

Then the stage-1 step and the stage-2 step (D step + G step) of mel_24k_base at B = 64 through
flow2gan_amd.harness, weights invalidated and rebuilt after every sub-step as an optimizer would, the two modes
alternating.

    python tools/fp16x3_shapes.py [--out profiles/fp16x3_gemm_shapes.txt] [--append] [--no-steps] [--min-k K] [--min-n N]

--noimage: the route that reads the fp32 activation as it is (gemm_h3n_kernel, csrc/gemm_f16n.hip; the tunable
fp16x3_plainn_min_n).  THREE legs alternate on the same 36 launches -- bf16x6, fp16x3 through the image route
(FP16X3_MIN_N = 1: every shape on gemm_h3_kernel, image pass included), fp16x3 through the new route
(FP16X3_PLAINN_MIN_N = 1) --, then the stage-1 and the stage-2 step in F2G_GEMM=fp16x3 with the tunable alone differing
(off, the shipped rule, against 1), three alternating pairs of four-step blocks.

    python tools/fp16x3_shapes.py --noimage [--append] [--no-steps]      (-> profiles/fp16x3_gemm_noimage_shapes.txt)
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = (6016, 12032, 24064)
KN = ((768, 2304), (2304, 768), (512, 1536), (1536, 512), (384, 1152), (1152, 384))
MODES = ("bf16x6", "fp16x3")


def shape_case(ops, rows, K, N, kind, dev):
    """a closure that launches one GEMM of the shape the way the generator does"""
    g = torch.Generator().manual_seed(rows + K + 7 * N)
    x = torch.randn(rows, K, generator=g).to(dev)
    w = torch.nn.Parameter((torch.randn(N, K, generator=g) * K ** -0.5).to(dev))
    out = torch.empty(rows, N, device=dev)
    bias = torch.randn(N, generator=g).to(dev)
    if kind == "fwd" and K < N:         # pwconv1: bias, PReLU, pre-activation kept for the backward
        slope, act = torch.full((N,), 0.25, device=dev), torch.empty(rows, N, device=dev)
        return lambda: ops.gemm(ops.mat(x), ops.mat(w), out, bias=bias, prelu=slope, prelu_out=act)
    if kind == "fwd":                   # pwconv2: bias, residual * gamma
        res, gamma = torch.randn(rows, N, generator=g).to(dev), torch.full((N,), 0.1, device=dev)
        return lambda: ops.gemm(ops.mat(x), ops.mat(w), out, bias=bias, res=res, gamma=gamma)
    # data gradients: form 1 against the weight of the forward GEMM with the SAME (K, N) = a weight of shape (K, N)
    wt = torch.nn.Parameter((torch.randn(K, N, generator=g) * K ** -0.5).to(dev))
    if K > N:                           # through pwconv2 into the PReLU: its backward with both column sums
        aux, alpha = torch.randn(rows, N, generator=g).to(dev), torch.full((N,), 0.25, device=dev)
        sums = torch.zeros(2 * N, device=dev)
        return lambda: ops.gemm(ops.mat(x), ops.mat(wt), out, form=1, aux=aux, alpha_n=alpha,
                                colsum_alpha=sums[:N], colsum=sums[N:])
    return lambda: ops.gemm(ops.mat(x), ops.mat(wt), out, form=1)


def time_blocks(ops, fn, blocks=5, reps=12):
    """per-mode list of per-launch microseconds, one entry per block, the modes alternating"""
    per = {m: [] for m in MODES}
    kern = {}
    for m in MODES:                     # warm-up: code objects, weight images
        ops.set_gemm_precision(m)
        for _ in range(3):
            fn()
        kern[m] = ops.L.lib.f2g_gemm_last_kernel().decode()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for m in MODES:
            ops.set_gemm_precision(m)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            per[m].append(s.elapsed_time(e) * 1e3 / reps)
    return per, kern


def med_spread(v):
    m = statistics.median(v)
    return m, (max(v) - min(v)) / m


def shapes_table(ops, dev, say):
    say("form  rows      K      N  epilogue   bf16x6_us  spread  fp16x3_us  spread  ratio  TFLOP/s(fp16x3)  kernels")
    worst = []
    for rows in ROWS:
        for K, N in KN:
            for kind in ("fwd", "dgrad"):
                fn = shape_case(ops, rows, K, N, kind, dev)
                per, kern = time_blocks(ops, fn)
                (a, sa), (b, sb) = med_spread(per["bf16x6"]), med_spread(per["fp16x3"])
                epi = {("fwd", True): "prelu2", ("fwd", False): "res", ("dgrad", True): "plain",
                       ("dgrad", False): "dprelu"}[(kind, K < N)]
                say(f"{kind:5s} {rows:5d} {K:6d} {N:6d}  {epi:8s} {a:10.1f} {sa:7.3f} {b:10.1f} {sb:7.3f} "
                    f"{b / a:6.3f} {2.0 * rows * K * N / b * 1e-6:12.1f}      {kern['bf16x6']} | {kern['fp16x3']}")
                worst.append((b / a, max(sa, sb), rows, K, N, kind))
    lost = [w for w in worst if w[0] > 1.0 + w[1]]
    say(f"# shapes where fp16x3 loses by more than the spread: {len(lost)} of {len(worst)}"
        + "".join(f"\n#   {k} rows {r} K {kk} N {n}: ratio {q:.3f}, spread {s:.3f}" for q, s, r, kk, n, k in lost))


def steps_table(ops, dev, say, steps=4, legs=None, counter="FP16X3_LAUNCHES"):
    """legs: (name, function that sets the leg up) twice -- the two modes unless given; counter: the ops counter whose
    launches per step of the second leg are reported"""
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

    def stepped(params):
        ops.bump_weight_epoch(params)
        ops.rebuild_derived(params)

    def zero(params):
        for p in params:
            p.grad = None

    def stage1():
        gen.train()
        zero(g_params)
        loss, _ = harness.compute_loss_stage1(audio, lens, logmel, gen)
        loss.backward()
        stepped(g_params)

    def stage2():
        for disc, params in ((True, d_params), (False, g_params)):
            zero(params)
            loss, _ = harness.compute_loss_stage2(audio, lens, gan, logmel, 1, train_disc=disc)
            loss.backward()
            stepped(params)

    legs = legs or tuple((m, lambda m=m: ops.set_gemm_precision(m)) for m in MODES)
    (na, _), (nb, _) = legs
    say(f"step     {na}_ms  spread  {nb}_ms  spread  ratio  {nb} launches per step ({counter})")
    for name, fn in (("stage1", stage1), ("stage2", stage2)):
        per = {m: [] for m, _ in legs}
        launches = 0
        for m, setup in legs:
            setup()
            fn(), fn()
        torch.cuda.synchronize()
        for _ in range(3):
            for m, setup in legs:
                setup()
                n0 = getattr(ops, counter)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    fn()
                torch.cuda.synchronize()
                per[m].append((time.perf_counter() - t0) * 1e3 / steps)
                if m == nb:
                    launches = max(launches, (getattr(ops, counter) - n0) // steps)
        (a, sa), (b, sb) = med_spread(per[na]), med_spread(per[nb])
        say(f"{name:8s} {a:9.2f} {sa:7.3f} {b:10.2f} {sb:7.3f} {b / a:6.3f}  {launches}"
            f"      # within-leg ranges {sa * a:.2f} / {sb * b:.2f} ms")


# ---- --noimage: three legs on the shapes, the tunable alone on the steps
LEGS = ("bf16x6", "image", "noimage")


def set_leg(ops, leg, off):
    """bf16x6; fp16x3 with every shape on the image route; fp16x3 with every shape on the route without an image"""
    ops.set_gemm_precision("bf16x6" if leg == "bf16x6" else "fp16x3")
    ops.FP16X3_MIN_N = 1
    ops.FP16X3_PLAINN_MIN_N = 1 if leg == "noimage" else off


def noimage_shapes_table(ops, dev, say, blocks=5, reps=12):
    say("form  rows      K      N  epilogue   bf16x6_us  spread   image_us  spread  noimage_us  spread  img/x6  noi/x6  "
        "noi/img  TFLOP/s(noimage)  kernels")
    off = ops.FP16X3_TAP_OFF
    rows_out = []
    for rows in ROWS:
        for K, N in KN:
            for kind in ("fwd", "dgrad"):
                fn = shape_case(ops, rows, K, N, kind, dev)
                per, kern = {m: [] for m in LEGS}, {}
                for m in LEGS:                      # warm-up: code objects, weight images
                    set_leg(ops, m, off)
                    for _ in range(3):
                        fn()
                    kern[m] = ops.L.lib.f2g_gemm_last_kernel().decode()
                torch.cuda.synchronize()
                for _ in range(blocks):
                    for m in LEGS:
                        set_leg(ops, m, off)
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        for _ in range(reps):
                            fn()
                        e.record()
                        torch.cuda.synchronize()
                        per[m].append(s.elapsed_time(e) * 1e3 / reps)
                (a, sa), (b, sb), (c, sc) = (med_spread(per[m]) for m in LEGS)
                epi = {("fwd", True): "prelu2", ("fwd", False): "res", ("dgrad", True): "plain",
                       ("dgrad", False): "dprelu"}[(kind, K < N)]
                say(f"{kind:5s} {rows:5d} {K:6d} {N:6d}  {epi:8s} {a:10.1f} {sa:7.3f} {b:10.1f} {sb:7.3f} {c:11.1f} "
                    f"{sc:7.3f} {b / a:7.3f} {c / a:7.3f} {c / b:8.3f} {2.0 * rows * K * N / c * 1e-6:13.1f}      "
                    + " | ".join(kern[m] for m in LEGS))
                rows_out.append((kind, rows, K, N, a, sa, b, sb, c, sc))
    for what, i, j in (("noimage against bf16x6", 8, 4), ("noimage against image", 8, 6)):
        win = [r for r in rows_out if r[i] / r[j] < 1.0 - max(r[i + 1], r[j + 1])]
        lose = [r for r in rows_out if r[i] / r[j] > 1.0 + max(r[i + 1], r[j + 1])]
        say(f"# {what}: wins by more than the spread in {len(win)} of {len(rows_out)} launches, loses in {len(lose)}"
            + "".join(f"\n#   loses: {r[0]} rows {r[1]} K {r[2]} N {r[3]}: ratio {r[i] / r[j]:.3f}" for r in lose))


def noimage_legs(ops):
    """the step legs of --noimage: F2G_GEMM=fp16x3 both times, fp16x3_plainn_min_n off (as shipped) and 1"""
    def leg(value):
        def go():
            ops.set_gemm_precision("fp16x3")
            ops.FP16X3_PLAINN_MIN_N = value
        return go
    return (("off", leg(ops.FP16X3_TAP_OFF)), ("on", leg(1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/fp16x3_gemm_shapes.txt, with --noimage "
                    "profiles/fp16x3_gemm_noimage_shapes.txt")
    ap.add_argument("--noimage", action="store_true", help="three legs: bf16x6, fp16x3 through the image route, "
                    "fp16x3 through the route that reads the fp32 activation as it is (fp16x3_plainn_min_n)")
    ap.add_argument("--append", action="store_true", help="add this run's table to --out instead of replacing it")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--no-shapes", action="store_true")
    ap.add_argument("--min-k", type=int, default=0, help="ops.FP16X3_MIN_K for this run (0: the default)")
    ap.add_argument("--min-n", type=int, default=0, help="ops.FP16X3_MIN_N for this run (0: the default; 1: every "
                    "shape of the table on the new kernel)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from flow2gan_amd import ops
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "fp16x3_gemm_noimage_shapes.txt" if args.noimage
                                else "fp16x3_gemm_shapes.txt")
    if args.min_k:
        ops.FP16X3_MIN_K = args.min_k
    if args.min_n:
        ops.FP16X3_MIN_N = args.min_n
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/fp16x3_shapes.py  {ops.L.version()}  FP16X3_MIN_K={ops.FP16X3_MIN_K} FP16X3_MIN_N={ops.FP16X3_MIN_N}  {torch.cuda.get_device_name(0)}")
    say("# per-launch medians of 5 alternating blocks of 12 launches (us), activation image pass included; "
        "spread = (max - min) / median of a mode's blocks; ratio = fp16x3 / bf16x6 (< 1: fp16x3 faster)")
    was = ops.GEMM_PRECISION, ops.FP16X3
    keep = ops.FP16X3_MIN_N, ops.FP16X3_PLAINN_MIN_N
    try:
        if args.noimage:
            say("# --noimage: legs bf16x6 | image (fp16x3, FP16X3_MIN_N = 1: gemm_h3_kernel + f2g_split_f16x2 per call) | "
                "noimage (fp16x3, FP16X3_PLAINN_MIN_N = 1: gemm_h3n_kernel reads the fp32 activation)")
            if not args.no_shapes:
                noimage_shapes_table(ops, dev, say)
            ops.FP16X3_MIN_N = keep[0]
            if not args.no_steps:
                say(f"# steps in F2G_GEMM=fp16x3, FP16X3_MIN_N={ops.FP16X3_MIN_N}: fp16x3_plainn_min_n off | 1, three "
                    "alternating pairs of four-step blocks")
                steps_table(ops, dev, say, legs=noimage_legs(ops), counter="FP16X3_PLAINN_LAUNCHES")
        else:
            if not args.no_shapes:
                shapes_table(ops, dev, say)
            if not args.no_steps:
                steps_table(ops, dev, say)
    finally:
        ops.FP16X3_MIN_N, ops.FP16X3_PLAINN_MIN_N = keep
        ops.set_gemm_precision("fp16x3" if was[1] else {0: "fp32", 1: "bf16x3", 2: "bf16", 3: "bf16x6"}[was[0]])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(("#\n# ---- another run of the same tool\n" if args.append else "") + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
