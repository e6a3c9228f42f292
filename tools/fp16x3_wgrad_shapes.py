#!/usr/bin/env python
"""fp16x3 against bf16x6 on the generator's weight-gradient launches and on the train steps -- one box, one process.

Per shape -- (M, N) = (3C, C) and (C, 3C), the weight gradients of pwconv1 / pwconv2, for C = 768, 512, 384, each at
R = 6016, 12032 and 24064 reduction rows (B 64 x 1 s at the three branch rates) -- ops.wgrad is timed in both modes,
the modes ALTERNATING block by block (time_blocks / med_spread of tools/fp16x3_shapes.py), with everything a launch
costs in its mode inside the timed region: fp16x3 = the two f2g_split_f16x2_cols calls (both operands are
activations) plus gemm_h3w_kernel; bf16x6 = the launch as that mode routes it (gemm_leanw6_kernel splits the fp32
operands itself).  Both accumulate atomically onto the same gradient buffer with the split-K factor of ops.split_for.
At each branch's own shape both results are checked against float64 (tests/test_hip_gemm_routes.py: check).

Then the stage-1 and the stage-2 step as tools/fp16x3_shapes.py runs them (steps_table), the two modes alternating.

The route is off by default in the package (ops.FP16X3_WGRAD_MIN_ROWS = FP16X3_WGRAD_OFF), so this tool, whose
purpose is to measure it, sets the threshold itself: --min-rows, default 1 = every launch on the new kernel.  The
header of the output states the command it was made with.

--noimage measures the route that reads both fp32 operands as they are and scales them inside the kernel
(gemm_h3wn_kernel, csrc/gemm_f16wn.hip; ops.FP16X3_WGRADN_MIN_ROWS, off by default; default output
profiles/fp16x3_wgrad_noimage_shapes.txt).  THREE legs alternate on the same 18 shapes -- bf16x6, fp16x3 through the
image route (FP16X3_WGRAD_MIN_ROWS = 1, both image calls inside the timed launch), fp16x3 through the new route
(FP16X3_WGRADN_MIN_ROWS = 1, the image route off) -- with win / lose counts "by more than the spread" against both other
legs, and all three against float64 at each branch's own shape (the new route's tolerance: the suite's 1.8e-6 of
|dy|^T |x| plus the floor 2^-28 (xmax sum |dy| + dymax sum |x|) of tests/test_hip_gemm_f16_wgradn.py).  Then the steps in
F2G_GEMM=fp16x3 with the tunable alone differing (off | 1), three alternating pairs of four-step blocks, with the
launches per step on the kernel.

    python tools/fp16x3_wgrad_shapes.py [--out profiles/fp16x3_wgrad_shapes.txt] [--append] [--no-shapes] [--no-steps]
                                        [--min-rows R] [--noimage]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fp16x3_shapes import MODES, med_spread, steps_table, time_blocks  # noqa: E402

ROWS = (6016, 12032, 24064)
CHANNELS = (768, 512, 384)          # the branch with C channels runs at ROWS[i] rows
TOL = {"bf16x6": 1e-6, "fp16x3": 1.8e-6}     # the suite's tolerances of the two arithmetics


def shapes_table(ops, dev, say):
    from test_hip_gemm_routes import check
    say("    R      M      N  bf16x6_us  spread  fp16x3_us  spread  ratio  TFLOP/s(fp16x3)  kernels")
    worst = []
    for i, Cc in enumerate(CHANNELS):
        for R in ROWS:
            for M, N in ((3 * Cc, Cc), (Cc, 3 * Cc)):
                g = torch.Generator().manual_seed(R + M + 7 * N)
                dy = (torch.randn(R, M, generator=g) * R ** -0.5).to(dev)
                x = torch.randn(R, N, generator=g).to(dev)
                grad = torch.zeros(M, N, device=dev)
                fn = lambda: ops.wgrad(dy, M, M, ops.mat(x), grad)     # noqa: E731
                if R == ROWS[i]:        # the branch's own shape: both modes against float64
                    want = dy.double().t() @ x.double()
                    mag = dy.double().abs().t() @ x.double().abs()
                    for m in MODES:
                        ops.set_gemm_precision(m)
                        grad.zero_()
                        fn()
                        torch.cuda.synchronize()
                        check(grad.double(), want, mag, TOL[m], f"{m} R {R} M {M} N {N}")
                    del want, mag
                per, kern = time_blocks(ops, fn)
                (a, sa), (b, sb) = med_spread(per["bf16x6"]), med_spread(per["fp16x3"])
                say(f"{R:5d} {M:6d} {N:6d} {a:10.1f} {sa:7.3f} {b:10.1f} {sb:7.3f} {b / a:6.3f} "
                    f"{2.0 * R * M * N / b * 1e-6:12.1f}      {kern['bf16x6']} | {kern['fp16x3']}")
                worst.append((b / a, max(sa, sb), R, M, N))
    lost = [w for w in worst if w[0] > 1.0 + w[1]]
    won = [w for w in worst if w[0] < 1.0 - w[1]]
    say(f"# shapes where fp16x3 wins by more than the spread: {len(won)} of {len(worst)}"
        + "".join(f"\n#   R {r} M {m} N {n}: ratio {q:.3f}, spread {s:.3f}" for q, s, r, m, n in won))
    say(f"# shapes where fp16x3 loses by more than the spread: {len(lost)} of {len(worst)}"
        + "".join(f"\n#   R {r} M {m} N {n}: ratio {q:.3f}, spread {s:.3f}" for q, s, r, m, n in lost))


# ---- --noimage: three legs on the shapes, the tunable alone on the steps
LEGS = ("bf16x6", "image", "noimage")


def set_leg(ops, leg):
    """bf16x6; fp16x3 with every shape on the image route; fp16x3 with every shape on the route without an image"""
    ops.set_gemm_precision("bf16x6" if leg == "bf16x6" else "fp16x3")
    ops.FP16X3_WGRAD_MIN_ROWS = 1 if leg == "image" else ops.FP16X3_WGRAD_OFF
    ops.FP16X3_WGRADN_MIN_ROWS = 1 if leg == "noimage" else ops.FP16X3_TAP_OFF


def noimage_shapes_table(ops, dev, say, blocks=5, reps=12):
    from test_hip_gemm_routes import check
    say("    R      M      N  bf16x6_us  spread   image_us  spread  noimage_us  spread  img/x6  noi/x6  noi/img  "
        "TFLOP/s(noimage)  kernels")
    tol = {"bf16x6": TOL["bf16x6"], "image": TOL["fp16x3"], "noimage": TOL["fp16x3"]}
    rows_out = []
    for i, Cc in enumerate(CHANNELS):
        for R in ROWS:
            for M, N in ((3 * Cc, Cc), (Cc, 3 * Cc)):
                g = torch.Generator().manual_seed(R + M + 7 * N)
                dy = (torch.randn(R, M, generator=g) * R ** -0.5).to(dev)
                x = torch.randn(R, N, generator=g).to(dev)
                grad = torch.zeros(M, N, device=dev)
                fn = lambda: ops.wgrad(dy, M, M, ops.mat(x), grad)     # noqa: E731
                if R == ROWS[i]:        # the branch's own shape: all legs against float64
                    da, xa = dy.double().abs(), x.double().abs()
                    want, mag = dy.double().t() @ x.double(), da.t() @ xa
                    floor = 2.0 ** -28 * (xa.max() * da.sum(0)[:, None] + da.max() * xa.sum(0)[None, :])
                    for m in LEGS:
                        set_leg(ops, m)
                        grad.zero_()
                        fn()
                        torch.cuda.synchronize()
                        check(grad.double(), want, mag + (floor / tol[m] if m == "noimage" else 0.0), tol[m],
                              f"{m} R {R} M {M} N {N}")
                    del want, mag, floor, da, xa
                per, kern = {m: [] for m in LEGS}, {}
                for m in LEGS:                      # warm-up: code objects
                    set_leg(ops, m)
                    for _ in range(3):
                        fn()
                    kern[m] = ops.L.lib.f2g_gemm_last_kernel().decode()
                torch.cuda.synchronize()
                for _ in range(blocks):
                    for m in LEGS:
                        set_leg(ops, m)
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        for _ in range(reps):
                            fn()
                        e.record()
                        torch.cuda.synchronize()
                        per[m].append(s.elapsed_time(e) * 1e3 / reps)
                (a, sa), (b, sb), (c, sc) = (med_spread(per[m]) for m in LEGS)
                say(f"{R:5d} {M:6d} {N:6d} {a:10.1f} {sa:7.3f} {b:10.1f} {sb:7.3f} {c:11.1f} {sc:7.3f} {b / a:7.3f} "
                    f"{c / a:7.3f} {c / b:8.3f} {2.0 * R * M * N / c * 1e-6:13.1f}      "
                    + " | ".join(kern[m] for m in LEGS))
                rows_out.append((R, M, N, a, sa, b, sb, c, sc))
    for what, i, j in (("noimage against bf16x6", 7, 3), ("noimage against image", 7, 5)):
        win = [r for r in rows_out if r[i] / r[j] < 1.0 - max(r[i + 1], r[j + 1])]
        lose = [r for r in rows_out if r[i] / r[j] > 1.0 + max(r[i + 1], r[j + 1])]
        say(f"# {what}: wins by more than the spread in {len(win)} of {len(rows_out)} launches, loses in {len(lose)}"
            + "".join(f"\n#   wins: R {r[0]} M {r[1]} N {r[2]}: ratio {r[i] / r[j]:.3f}" for r in win)
            + "".join(f"\n#   loses: R {r[0]} M {r[1]} N {r[2]}: ratio {r[i] / r[j]:.3f}" for r in lose))


def noimage_legs(ops):
    """the step legs of --noimage: F2G_GEMM=fp16x3 both times, the image route off (as shipped),
    fp16x3_wgradn_min_rows off (as shipped) and 1"""
    def leg(value):
        def go():
            ops.set_gemm_precision("fp16x3")
            ops.FP16X3_WGRAD_MIN_ROWS = ops.FP16X3_WGRAD_OFF
            ops.FP16X3_WGRADN_MIN_ROWS = value
        return go
    return (("off", leg(ops.FP16X3_TAP_OFF)), ("on", leg(1)))


def noimage_main(args, ops):
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    given = [a for i, a in enumerate(sys.argv[1:], 1) if a != "--out" and sys.argv[i - 1] != "--out"]
    say("# command (the output path aside): python tools/fp16x3_wgrad_shapes.py " + " ".join(given))
    say(f"# tools/fp16x3_wgrad_shapes.py  {ops.L.version()}  FP16X3_MIN_K={ops.FP16X3_MIN_K} "
        f"FP16X3_MIN_N={ops.FP16X3_MIN_N}  {torch.cuda.get_device_name(0)}")
    say("# per-launch medians of 5 alternating blocks of 12 launches (us); spread = (max - min) / median of a leg's "
        "blocks; ratios < 1: the numerator's leg is faster")
    say("# --noimage: legs bf16x6 (the launch as that mode routes it) | image (fp16x3, FP16X3_WGRAD_MIN_ROWS = 1: two "
        "f2g_split_f16x2_cols calls + gemm_h3w_kernel) | noimage (fp16x3, FP16X3_WGRADN_MIN_ROWS = 1: gemm_h3wn_kernel "
        "reads both fp32 operands)")
    from test_hip_gemm_f16 import mode_name
    was, keep = mode_name(ops), (ops.FP16X3_WGRAD_MIN_ROWS, ops.FP16X3_WGRADN_MIN_ROWS)
    try:
        if not args.no_shapes:
            noimage_shapes_table(ops, dev, say)
        if not args.no_steps:
            say("# steps in F2G_GEMM=fp16x3, the image route off: fp16x3_wgradn_min_rows off | 1, three alternating pairs "
                "of four-step blocks")
            steps_table(ops, dev, say, legs=noimage_legs(ops), counter="FP16X3_WGRADN_LAUNCHES")
    finally:
        ops.FP16X3_WGRAD_MIN_ROWS, ops.FP16X3_WGRADN_MIN_ROWS = keep
        ops.set_gemm_precision(was)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(("#\n# ---- another run of the same tool\n" if args.append else "") + "\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/fp16x3_wgrad_shapes.txt, with --noimage "
                    "profiles/fp16x3_wgrad_noimage_shapes.txt")
    ap.add_argument("--noimage", action="store_true", help="three legs: bf16x6, fp16x3 through the image route, fp16x3 "
                    "through the route that reads both fp32 operands as they are (fp16x3_wgradn_min_rows)")
    ap.add_argument("--append", action="store_true", help="add this run's table to --out instead of replacing it")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--no-shapes", action="store_true")
    ap.add_argument("--min-rows", type=int, default=1, help="ops.FP16X3_WGRAD_MIN_ROWS for this run (1: every shape "
                    "of the table on the new kernel)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from flow2gan_amd import ops
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "fp16x3_wgrad_noimage_shapes.txt" if args.noimage
                                else "fp16x3_wgrad_shapes.txt")
    if args.noimage:
        return noimage_main(args, ops)
    if args.min_rows < 1 or args.min_rows >= ops.FP16X3_WGRAD_OFF:
        ap.error("--min-rows must enable the route: both modes would time the same bf16x6 launch otherwise")
    ops.FP16X3_WGRAD_MIN_ROWS = args.min_rows
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    given = [a for i, a in enumerate(sys.argv[1:], 1) if a != "--out" and sys.argv[i - 1] != "--out"]
    say("# command (the output path aside): python tools/fp16x3_wgrad_shapes.py " + " ".join(given))
    say(f"# tools/fp16x3_wgrad_shapes.py  {ops.L.version()}  FP16X3_WGRAD_MIN_ROWS={ops.FP16X3_WGRAD_MIN_ROWS} "
        f"FP16X3_MIN_K={ops.FP16X3_MIN_K} FP16X3_MIN_N={ops.FP16X3_MIN_N}  {torch.cuda.get_device_name(0)}")
    say("# per-launch medians of 5 alternating blocks of 12 launches (us), both column-image calls included; "
        "spread = (max - min) / median of a mode's blocks; ratio = fp16x3 / bf16x6 (< 1: fp16x3 faster)")
    from test_hip_gemm_f16 import mode_name       # (the one place that names the mode in force)
    was = mode_name(ops)
    try:
        if not args.no_shapes:
            shapes_table(ops, dev, say)
        if not args.no_steps:
            n0 = ops.FP16X3_WGRAD_LAUNCHES
            steps_table(ops, dev, say)
            say(f"# weight-gradient launches on gemm_h3w_kernel during the step runs: {ops.FP16X3_WGRAD_LAUNCHES - n0}")
    finally:
        ops.set_gemm_precision(was)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(("#\n# ---- another run of the same tool\n" if args.append else "") + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
