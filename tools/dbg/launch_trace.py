"""Which launches does one step issue, in which order and with which arguments?  Writes one line per f2g_* call of
ONE step after warm-up: entry point, stream (ordinal of the stream's first appearance) and every argument --
descriptors field by field, floats with repr, device addresses as `@n` = ordinal of that exact address's first
appearance in the trace.  Two builds of the package that issue the same launches write the same file, whatever the
weight gradients' atomics do to the values: record in fresh processes and compare with diff.

    python tools/dbg/launch_trace.py STEP [--gemm fp32|bf16x6|bf16x3] [--serial] [--out FILE]

STEP: D / G (fused GAN.forward + backward on the tiny_stage2 golden configuration), mpd / mrd (the custom-loss
backward of tests/test_hip_disc_autograd.py through the discriminator modules, B = 2, T = 6001, gradients to the
input and the parameters), mpd1 / mrd1 (a loss on one middle feature map of sub-discriminator 0).  --serial: launch
lanes off (ops.CONCURRENT = False).  The last line on stdout is the step's torch.cuda.max_memory_allocated()."""
import argparse
import ctypes as C
import math
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
import flow2gan_amd
from flow2gan_amd import ops, _lib

ap = argparse.ArgumentParser()
ap.add_argument("step", choices=["D", "G", "mpd", "mrd", "mpd1", "mrd1"])
ap.add_argument("--gemm", default="fp32")
ap.add_argument("--serial", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
ops.set_gemm_precision(args.gemm)
ops.CONCURRENT = not args.serial
random.random = lambda: 0.0       # (the tests' setting: LimitParamValue always draws)

if args.step in ("D", "G"):
    import test_hip_gan as TG
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "tiny_stage2.npz")))
    gan = TG.build_gan(flow2gan_amd, g)
    mel, audio, noise = (TG.T(g[k]).to("cuda") for k in ("mel", "audio", "noise"))
    lens = TG.T(g["n2/lens"])

    def step():
        gan.zero_grad()
        if args.step == "D":
            d = gan(mel, audio, lens, 2, True, noise=noise)
            (d[0] + 0.1 * d[1]).backward()
        else:
            ls = gan(mel, audio, lens, 2, False, noise=noise)
            sum(w * l for w, l in zip((1.0, 0.1, 1.0, 0.1, 45.0), ls)).backward()
else:
    import test_hip_disc_autograd as TA
    _, dh = TA._models(args.step[:3])
    y, y_hat = (t.to("cuda") for t in TA._inputs())

    def step():
        for p in dh.parameters():
            p.grad = None
        yh = y_hat.clone().requires_grad_(True)
        if args.step.endswith("1"):
            m = dh.discriminators[0](yh)[1][1]
            r = torch.randn(m.shape, generator=torch.Generator().manual_seed(3)).to(m.device)
            loss = (m * r).sum() / math.sqrt(m.numel())
        else:
            loss = TA._custom_loss(*dh(y, yh))
        loss.backward()

step(); step()
torch.cuda.synchronize()

lines, addrs, streams = [], {}, {}


def addr(v):
    v = v.value if isinstance(v, C.c_void_p) else v
    return "null" if not v else "@%d" % addrs.setdefault(int(v), len(addrs))


def show(v, ctype=None):
    """One argument: by its declared ctypes type where the value itself is a plain Python number."""
    if hasattr(v, "_obj"):              # byref(descriptor)
        v = v._obj
    if isinstance(v, C.Structure):
        return "{" + " ".join(f"{n}={show(getattr(v, n), t)}" for n, t in v._fields_ if not n.startswith("_pad")) + "}"
    if isinstance(v, C.Array):
        items = [show(e, v._type_) for e in v]
        empty = show(v._type_(), v._type_)
        while items and items[-1] == empty:      # (unused table rows)
            items.pop()
        return "[" + " ".join(items) + "]"
    if ctype is C.c_void_p or isinstance(v, C.c_void_p):
        return addr(v)
    if isinstance(v, C._SimpleCData):
        v = v.value
    return repr(float(v)) if ctype is C.c_float or isinstance(v, float) else repr(v)


orig = _lib.call


def spy(name, *a):
    orig(name, *a)      # (first: the re-layout batch it may flush launches before it)
    s = streams.setdefault(torch.cuda.current_stream().cuda_stream, len(streams))
    sig = _lib._SIGS[name]
    lines.append(f"{name} s{s} " + " ".join(show(v, t) for v, t in zip(a, sig)))


for mod in list(sys.modules.values()):
    if getattr(mod, "__name__", "").startswith("flow2gan_amd") and getattr(mod, "call", None) is orig:
        mod.call = spy
torch.cuda.reset_peak_memory_stats()
step()
torch.cuda.synchronize()
peak = torch.cuda.max_memory_allocated()
out = open(args.out, "w") if args.out else sys.stdout
out.write("\n".join(lines) + "\n")
print(f"{args.step} {args.gemm} {'serial' if args.serial else 'lanes'}: {len(lines)} calls, max_memory_allocated {peak}")
