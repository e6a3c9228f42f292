"""Tunables of the host side, in ONE place: module constants with built-in defaults that
`F2G_OPTS="name=value,..."` may override at import (the same variable carries the library's own dispatch
options, csrc/common.h; names match in any letter case).  A name that neither side knows -- a retired or
misspelt switch -- draws one warning when the package is imported (warn_unknown).  Tests and tools change a
tunable by assigning the module attribute (`ops.X6F_MIN_K = 32`) or, for the library's,
`flow2gan_amd._lib.set_option("x6p", 2)`.

Only switches that something still needs are tunables: a test that flips them or takes one path as its
reference, bench.py, a debug cross-check, a cap, or a threshold that tests lower to reach a kernel on small
shapes.  The comment at each declaration says which.

The names (each declared in flow2gan_amd/ops.py unless noted): conv32_x6, fft, fft_reflect, fft_min, fused_multi,
eager_rebuild, time_ahead (models/generator.py), colsum_parts, x6f, x6g, x3_check, multi_cap, lane_cap_<pool>,
x6_min_k, x6_min_rows, x6_nopass_k, x6f_min_k, x6f_min_n, x6f_min_tiles, x6f_tall_rows, fp16x3_min_k, fp16x3_min_n
(F2G_GEMM=fp16x3: the shortest reduction and the fewest output columns the fp16x3 GEMM kernel takes),
fp16x3_plainn_min_n (the fewest output columns at which such a GEMM takes the fp16x3 kernel that reads the fp32
activation matrix itself and scales it per 128-row tile inside the kernel, without an image pass; off by default),
fp16x3_wgrad_min_rows (the fewest reduction rows at which a weight gradient takes the fp16x3 weight-gradient kernel),
fp16x3_wgradn_min_rows (the fewest reduction rows at which such a weight gradient takes the fp16x3 kernel that reads
both fp32 activation matrices themselves and scales each under one running scale per block inside the kernel, without
an image pass; tried behind fp16x3_wgrad_min_rows' image route; off by default),
fp16x3_tap_min_rows (the fewest output rows at which a GEMM over stride-1 windows of a halo map takes the fp16x3
tap-walking kernel; the route also asks for a reduction of at least x6_min_k, i.e. the launches the bf16x6 mode gives
to its image kernels), fp16x3_tapw_min_rows (the fewest reduction rows at which the weight gradient of a stride-1
five-tap layer over a halo map takes the fp16x3 tap-walking weight-gradient kernel; off by default),
fp16x3_tap3_min_rows (the fewest output rows at which a GEMM over stride-3 windows of five positions of a halo map with
a multiple of 128 channels -- the MPD's strided forward layers -- takes the fp16x3 stride-3 tap-walking kernel; off by
default), fp16x3_tapw3_min_rows (the fewest reduction rows at which the weight gradient of a stride-3 five-tap layer
over a halo map with a multiple of 128 channels -- the MPD's strided layers -- takes the fp16x3 stride-3 tap-walking
weight-gradient kernel; off by default), fp16x3_tapw3n_min_rows (the fewest reduction rows at which the weight gradient
of the stride-3 five-tap layer over a 32-channel halo map onto 128 channels -- the MPD's 32 -> 128 layer -- takes the
fp16x3 kernel that reads both fp32 operands once and scales them under one running scale per operand and block inside
the kernel, without an image pass; off by default), fp16x3_tap3n_min_rows (the fewest output rows at which the GEMM over stride-3
windows of five positions of a 32-channel halo map -- the MPD's 32 -> 128 forward layer -- takes the fp16x3 kernel that
scales the fp32 map per sequence segment inside the kernel, without an image pass; off by default),
fp16x3_tapn_min_rows (the fewest output rows at which a GEMM over stride-1 windows of two or one positions of a
128-channel halo map onto at most 32 columns -- the stride-residue data gradients of that layer -- takes the fp16x3
kernel that scales the fp32 map per sequence segment inside the kernel; off by default), fp16x3_tapn3_min_rows (the
fewest output rows, S * ceil(Hin / 3), at which that layer's data gradient is ONE launch over 96 columns for its three
stride residues, which reads the gradient map once instead of three times; off by default), fp16x3_conv32_fwd, fp16x3_conv32_dgrad (F2G_GEMM=fp16x3: the MRD (3, 9) band layers' forward / data gradient on the
fp16x3 kernels that scale each tile's patch inside the kernel; both off by default), fp16x3_conv32_wgrad (the same
layers' weight gradient on the fp16x3 kernel that keeps one running scale per operand and block; off by default),
fp16x3_conv33_fwd, fp16x3_conv33_dgrad (F2G_GEMM=fp16x3: the MRD (3, 3) fifth layer's forward / data gradient on the
fp16x3 kernel that scales each whole-row tile's patch inside the kernel, csrc/conv33h3.hip; both off by default),
fp16x3_conv33_wgrad (that layer's weight gradient on the fp16x3 kernel that keeps one running scale per operand and
block over its walk of whole-row tiles, csrc/conv33h3w.hip; off by default), dw_bwd_fused (fused.block_bwd runs the
BiasNorm and depthwise-conv backward passes of a ConvNeXt block as one launch that keeps du on chip, f2g_dwblock_bwd,
where the library takes the shape; off by default).

Environment switches that remain on their own (user-facing, or needed before anything is imported):
F2G_GEMM (arithmetic of the GEMMs), F2G_STREAMS (launch lanes), F2G_DETERMINISTIC (no splits on the library's
own initiative), F2G_WEIGHT_CACHE, F2G_LIB_PATH, F2G_DRYRUN, F2G_DIST_TIMEOUT_S."""
from __future__ import annotations

import os
import warnings


def _parse(text: str) -> dict:
    out = {}
    for item in text.split(","):
        if "=" in item:
            k, v = item.split("=", 1)
            out[k.strip().lower()] = v.strip()
    return out


_OPTS = _parse(os.environ.get("F2G_OPTS", ""))
_ASKED: set = set()     # every name opt() was asked for


def opt(name: str, default):
    """Value of tunable `name` (lower case): F2G_OPTS's, else `default`; typed like the default."""
    _ASKED.add(name)
    v = _OPTS.get(name)
    if v is None:
        return default
    if isinstance(default, bool):
        return v not in ("0", "false", "off", "")
    return type(default)(v)


def warn_unknown(lib_knows) -> list:
    """Warn once about the F2G_OPTS names that no tunable declared so far asked for and that `lib_knows(name)`
    denies (the library's options); returns them."""
    unknown = sorted(n for n in _OPTS if n not in _ASKED and not lib_knows(n))
    if unknown:
        warnings.warn("F2G_OPTS: unknown option name(s) ignored: " + ", ".join(unknown), stacklevel=2)
    return unknown
