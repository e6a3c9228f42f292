"""Descriptors around every fp16x3 GEMM route, enumerated deterministically, and what the host code decides for them:
f2g_gemm_f16_ok, f2g_gemm_colsum_part_rows and the route ops.gemm's chooser picks.  Host code only -- the operands lie
over host memory that nothing reads, no kernel is launched, no image is built.

tests/test_fp16x3_routes_host.py compares the decisions of the tree under test with tests/golden/
fp16x3_route_answers.json, which holds those of the commit BEFORE a change of the routing code:

    python tests/fp16x3_route_cases.py --record --repo <checkout and build of the parent commit> --commit <its id>

--record refuses the checkout this file lies in: the table is never recorded from the tree it is to judge.
--time [--repo <checkout>] times the Python side of all cases (timeit, minimum and spread of the repeats)."""
import argparse
import contextlib
import ctypes as C
import json
import os
import re
import sys
import timeit

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fp16x3_route_answers.json")
IMAGE_BUILDERS = ("_f16_operand", "_f16_seq_operand", "_f16_cols_operand", "_f16_cols_window_operand")
_BUFS = {}


def buf(n):
    """n floats of host memory (shared by every case that asks for as many; never read)"""
    if n not in _BUFS:
        _BUFS[n] = torch.empty(n)
    return _BUFS[n]


def fwd_plain(ops, M=384, N=256, K=192, **_):
    return ops.mat(buf(M * K).view(M, K)), ops.mat(buf(N * K).view(N, K)), buf(M * N).view(M, N), 0, False


def wgrad_plain(ops, R=512, M=256, N=128, **_):
    return ops.mat(buf(R * M).view(R, M)), ops.mat(buf(R * N).view(R, N)), buf(M * N).view(M, N), 2, True


def fwd_win(ops, S=3, P0=16, unit=128, taps=5, step=1, n=128, **_):
    """forward form over windows of a halo map of S sequences (two spare map rows per sequence) against (n, K)"""
    L_in = (P0 - 1) * step + taps + 2
    A = ops.win1d(buf(S * L_in * unit), S, L_in, unit, P0, step, 0, taps)
    return A, ops.mat(buf(n * taps * unit).view(n, taps * unit)), buf(S * P0 * n).view(S * P0, n), 0, False


def wgrad_win(ops, S=3, P0=16, unit=128, taps=5, step=1, n=128, **_):
    """weight gradient: the (S * P0, n) gradient map against unbounded windows of the whole input map"""
    hp_in, pad = (P0, 2) if step == 1 else (3 * P0, 6)
    B = ops.win1d(buf(S * hp_in * unit), S, hp_in, unit, P0, step, pad, taps, unbounded=True)
    return ops.mat(buf(S * P0 * n).view(S * P0, n)), B, buf(n * taps * unit).view(n, taps * unit), 2, True


# name (ops.FP16X3_<name>_LAUNCHES; PLAIN: ops.FP16X3_LAUNCHES) -> builder, its arguments, the operand under windows,
# the marks of (A, B) while the library is asked, the split of the images the kernel reads (0: the fp32 operand itself)
BASES = {
    "PLAINN": (fwd_plain, {}, "A", (9, 0), (0, 5)),
    "PLAIN": (fwd_plain, {}, "A", (0, 0), (5, 5)),
    "WGRAD": (wgrad_plain, {}, "B", (0, 0), (6, 6)),
    "TAPW3N": (wgrad_win, dict(unit=32, step=3), "B", (8, 8), (0, 0)),
    "TAPW": (wgrad_win, dict(), "B", (0, 0), (6, 6)),
    "TAPW3": (wgrad_win, dict(step=3), "B", (0, 0), (6, 6)),
    "TAPN": (fwd_win, dict(taps=2, n=32), "A", (8, 0), (0, 7)),
    "TAP": (fwd_win, dict(unit=512, P0=100), "A", (0, 0), (7, 7)),
    "TAP3N": (fwd_win, dict(unit=32, step=3), "A", (8, 0), (0, 7)),
    "TAP3": (fwd_win, dict(step=3), "A", (0, 0), (7, 7)),
}
# shapes that fill the chip under the library's grid rule (option x6p = 1: 256 tiles) for the forward window bases
CHIP_FILLING = {"TAPN": dict(S=2048), "TAP": dict(S=96, n=1024), "TAP3N": dict(S=2048), "TAP3": dict(S=512, n=1024)}


def changes(name):
    """(label, builder arguments, [(object, field, value)], x6p, x3_out) of every case of base `name`: the base itself
    and every single change of the fixed list"""
    _, args, win, marks, images = BASES[name]
    spare = buf(256).data_ptr()
    out = [("base", {}, [], 2, False)]
    raw = lambda label, *sets: out.append((label, {}, list(sets), 2, False))
    # both operands as the images the kernel reads, with their reciprocal scales: the answer 1
    raw("images", *[s for o, sp in zip("AB", images) if sp for s in ((o, "split", sp), (o, "rscale", spare))])
    for v in (0, 1, 2):
        raw(f"form={v}", ("d", "form", v))
    for v in (3, 4):
        raw(f"precision={v}", ("d", "precision", v))
    for o in "AB":
        for v in (0, 5, 6, 7, 8, 9):
            raw(f"{o}.split={v}", (o, "split", v))
            raw(f"{o}.split={v}+rscale", (o, "split", v), (o, "rscale", spare))
    windows = BASES[name][0] in (fwd_win, wgrad_win)
    for field, values in (("step", (1, 2, 3)), ("unit", (32, 64, 128, 256)), ("taps", (1, 2, 3, 4, 5)),
                          ("P0", (4, 8, 100))):
        for v in values:
            if windows:       # (a consistent geometry: the builder makes it)
                out.append((f"{field}={v}", {field: v}, [], 2, False))
            elif field != "taps":
                raw(f"{win}.{field}={v}", (win, {"step": "step0"}.get(field, field), v))
    for v in (-2, 0, 1, 9):
        raw(f"{win}.pad0={v}", (win, "pad0", v))
    for o in "AB":
        raw(f"{o}.base+4", (o, "base+", 4))
        raw(f"{o}.alpha", (o, "alpha", spare))
        raw(f"{o}.lrelu_src", (o, "lrelu_src", spare))
        raw(f"{o}.reflect", (o, "reflect", 1))
    raw(f"{win}.unbounded", (win, "unbounded", 0 if BASES[name][0] is wgrad_win else 1))
    for v in (1, 2):
        raw(f"split_k={v}", ("d", "split_k", v))
    raw("E.atomic", ("E", "atomic", 0 if BASES[name][0] in (wgrad_plain, wgrad_win) else 1))
    for field, v in (("accumulate", 1), ("c_bf16", 1), ("bias", spare), ("res", spare), ("gamma", spare),
                     ("colsum", spare), ("colsum_alpha", spare), ("colsum_part_ld", 4), ("lrelu_slope", 0.1),
                     ("scale", 0.5), ("scale", 1.0), ("mask_src", spare), ("prelu_slope", spare), ("prelu_out", spare),
                     ("alpha_n", spare), ("ldc", 8), ("ldc", 1 << 20), ("C+", 4), ("x3_out", spare)):
        raw(f"E.{field}={'set' if v == spare else v}", ("E", field, v))
    raw("E.res+ldres", ("E", "res", spare), ("E", "ldres", 256))
    raw("E.res misaligned", ("E", "res", spare + 4), ("E", "ldres", 256))
    raw("E.aux", ("E", "aux", spare), ("E", "ldaux", 256))
    raw("E.aux+alpha_n", ("E", "aux", spare), ("E", "ldaux", 256), ("E", "alpha_n", spare))
    raw("E.mask_src+fm_ref", ("E", "mask_src", spare), ("E", "fm_ref", spare))
    raw("E.fm_ref", ("E", "fm_ref", spare))
    raw("E.mask_src+accumulate", ("E", "mask_src", spare), ("E", "accumulate", 1))
    raw("E.prelu_slope+accumulate", ("E", "prelu_slope", spare), ("E", "accumulate", 1))
    raw("E.x3_out+prelu_out", ("E", "x3_out", spare), ("E", "prelu_out", spare))
    raw("E.colsums as parts", ("E", "colsum", spare), ("E", "colsum_alpha", spare), ("E", "colsum_part_ld", 256))
    raw("E.P0o", ("E", "P0o", 4), ("E", "seq_stride_o", 4096), ("E", "row_stride_o", 256))
    raw("E.P0o odd strides", ("E", "P0o", 4), ("E", "seq_stride_o", 4097), ("E", "row_stride_o", 256))
    # the caller asks for the output's three-piece image (ops.gemm(x3_out=True) over an x3_reserve'd output)
    out.append(("x3_out asked", {}, [], 2, True))
    for mode in (0, 1, 2):
        out.append((f"x6p={mode} small", {}, [], mode, False))
        out.append((f"x6p={mode} chip-filling", CHIP_FILLING.get(name, {}), [], mode, False))
    for other in sorted({b[3] for b in BASES.values()} - {marks}):
        raw(f"marks={other}", ("A", "split", other[0]), ("B", "split", other[1]))
    return out


def case_ids():
    return [f"{name}: {c[0]}" for name in BASES for c in changes(name)]


@contextlib.contextmanager
def host_setup(ops):
    """ops as the cases need it: fp16x3 mode, operands over host tensors (ops.ptr refuses them), a launch is an error"""
    saved = {k: getattr(ops, k) for k in dir(ops)
             if k.startswith("FP16X3") or k in ("GEMM_PRECISION", "ptr", "call", "_FP16X3_ROUTES") + IMAGE_BUILDERS}

    def no_launch(name, *a):
        raise AssertionError(f"the route decision launched {name}")
    ops.ptr = lambda t: None if t is None else t.data_ptr()
    ops.call = no_launch
    ops.set_gemm_precision("fp16x3")
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


def thresholds(ops):
    return [k for k in dir(ops) if re.fullmatch(r"FP16X3_(\w+_)?MIN_(K|N|ROWS)", k)]


def _apply(objs, sets):
    for o, field, v in sets:
        if o in objs:
            if field.endswith("+"):
                v, field = getattr(objs[o], field[:-1]) + v, field[:-1]
            setattr(objs[o], field, v)


def build(ops, name, args, sets, marked):
    """the descriptor of a case (marked: under the base's marks, as the library is asked; else as ops.gemm has it when
    it comes to the chooser) and the arguments of the chooser"""
    builder, base_args, _, marks, _ = BASES[name]
    A, Bm, out, form, atomic = builder(ops, **{**base_args, **args})
    if marked:
        A.split, Bm.split = marks
    _apply({"A": A, "B": Bm}, sets)
    d = ops.GemmDesc()
    d.A, d.B = A, Bm
    d.E.C, d.E.ldc, d.E.atomic = out.data_ptr(), out.stride(0), int(atomic)
    d.form, d.split_k, d.precision = form, 1, 4 if marked else 3
    _apply({"E": d.E, "d": d}, sets)
    return d, A, Bm, out


def python_choice(ops, d, A, Bm, out, x3_out):
    """the counter name of the route the chooser picks ('' = none; '+x3': it has the output's image written)"""
    if x3_out:
        out._f2g_x3_buf = buf(256)
    args = (d, A, Bm, out, d.form, bool(d.E.atomic), d.split_k, 0, x3_out, None)
    if hasattr(ops, "_fp16x3_route"):                    # the choice alone: no image builder is reached
        r = ops._fp16x3_route(*args)
        took = [r.counter] if r is not None else []
    else:                                                # before the chooser was split off: which counter moved
        counters = [k for k in dir(ops) if re.fullmatch(r"FP16X3_(\w+_)?LAUNCHES", k)]
        before = {k: getattr(ops, k) for k in counters}
        ops._fp16x3_gemm(*args)
        took = [k for k in counters if getattr(ops, k) != before[k]]
    if x3_out:
        del out._f2g_x3_buf
    assert len(took) <= 1, took
    name = took[0][len("FP16X3_"):-len("LAUNCHES")].rstrip("_") or "PLAIN" if took else ""
    return name + ("+x3" if took and d.E.x3_out else "")


COLUMNS = ("f2g_gemm_f16_ok, f2g_gemm_colsum_part_rows, the chooser's route with every threshold at 1, the same with "
           "the no-image plain route off (so that the image route is reached)")


def answers(ops, lib_mod):
    """{case id: [COLUMNS]}"""
    lib = lib_mod.lib
    out = {}
    with host_setup(ops):
        for k in IMAGE_BUILDERS:                         # (only a tree from before the split reaches them)
            setattr(ops, k, lambda o: o)
        for k in thresholds(ops):
            setattr(ops, k, 1)
        for name in BASES:
            for label, args, sets, x6p, x3_out in changes(name):
                old = lib_mod.set_option("x6p", x6p)
                d = build(ops, name, args, sets, True)[0]
                row = [lib.f2g_gemm_f16_ok(C.byref(d)), lib.f2g_gemm_colsum_part_rows(C.byref(d))]
                for ops.FP16X3_PLAINN_MIN_N in (1, ops.FP16X3_TAP_OFF):
                    row.append(python_choice(ops, *build(ops, name, args, sets, False), x3_out))
                lib_mod.set_option("x6p", old)
                out[f"{name}: {label}"] = row
    return out


def time_python_side(ops, lib_mod, repeats=7):
    """seconds for ops._fp16x3_gemm over every case, image builders stubbed: (minimum, spread) of `repeats` runs with
    every threshold at 1, and with the thresholds the tree ships"""
    stub = lambda o: o
    res = {}
    with host_setup(ops):
        for k in IMAGE_BUILDERS:
            setattr(ops, k, stub)
        if hasattr(ops, "_FP16X3_ROUTES"):
            ops._FP16X3_ROUTES = {key: tuple(r._replace(images=tuple(f and stub for f in r.images)) for r in rs)
                                  for key, rs in ops._FP16X3_ROUTES.items()}
        old = lib_mod.set_option("x6p", 2)
        cases = [build(ops, name, args, sets, False) for name in BASES for _, args, sets, _, _ in changes(name)]

        def run():
            for d, A, Bm, o in cases:
                d.A, d.B, d.precision = A, Bm, 3
                ops._fp16x3_gemm(d, A, Bm, o, d.form, bool(d.E.atomic), d.split_k, 0, False, None)
        shipped = {k: getattr(ops, k) for k in thresholds(ops)}
        for label in ("shipped thresholds", "thresholds at 1"):
            t = timeit.repeat(run, number=20, repeat=repeats)
            res[label] = (min(t) / 20, (max(t) - min(t)) / 20, len(cases))
            for k in shipped:
                setattr(ops, k, 1)
        lib_mod.set_option("x6p", old)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--repo", default=os.path.dirname(HERE))
    ap.add_argument("--commit", default="")
    a = ap.parse_args()
    repo = os.path.realpath(a.repo)
    sys.path.insert(0, repo)
    from flow2gan_amd import _lib, ops
    assert os.path.realpath(ops.__file__).startswith(repo + os.sep), ops.__file__
    if a.time:
        for label, (best, spread, n) in time_python_side(ops, _lib).items():
            print(f"{label}: {n} cases in {best * 1e3:.3f} ms (minimum of 7 repeats, spread {spread * 1e3:.3f} ms)")
    if a.record:
        if repo == os.path.realpath(os.path.dirname(HERE)) or not a.commit:
            sys.exit("--record wants --repo <a checkout of the parent commit, not this tree> and --commit <its id>")
        table = {"recorded_from": a.commit, "columns": COLUMNS, "answers": answers(ops, _lib)}
        with open(GOLDEN, "w") as f:
            f.write(json.dumps(table, separators=(",", ":")).replace('],"', '],\n"') + "\n")
        print("recorded", len(table["answers"]), "cases from", a.commit)


if __name__ == "__main__":
    main()
