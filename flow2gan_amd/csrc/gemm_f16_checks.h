// Host-side conditions that more than one fp16x3 kernel states about a descriptor, written once: the forward
// tap-walking family (gemm_f16p.hip, gemm_f16p3.hip, gemm_f16p3n.hip, gemm_f16pn.hip) and the tap-walking weight
// gradients (gemm_f16wt.hip, gemm_f16ws.hip, gemm_f16wsn.hip).  A kernel's own f2g_h3*_ok adds what really is its own:
// channel counts, tile geometry, the output's leading dimension.  No device code; internal linkage throughout.
#pragma once
#include "gemm_common.h"
#include "x6_epilogue.h"

namespace {

// 32-bit byte offsets with the sign bit to spare for "past the end", a slab of slack below it: 2^31 - 2^20 bytes
inline bool h3_fits31(long long floats) { return floats * 4 < 0x7ff00000ll; }

// f16_images_status (gemm_common.h) for the kernels that scale A themselves -- A stays fp32 under its mark (the
// caller's test), so the answer follows B alone: 1 = B is the image with its reciprocal scales, 2 = B is fp32, 0 =
// anything else
inline int f16_b_image_status(const f2g_operand& B, int split) {
  if (B.split == split) return B.rscale ? 1 : 0;
  return B.split == 0 ? 2 : 0;
}

// form 2 (weight gradient) over two plain K-major matrices (gemm_h3w_kernel, gemm_f16.hip, and gemm_h3wn_kernel,
// gemm_f16wn.hip): what gemm_leanw6_kernel<false> takes for two plain operands, with partial tiles (any M, N that are
// multiples of 4) and without a bf16 output
inline bool h3w_operand_ok(const f2g_operand& S) {
  return host_plain(S) && !S.alpha && S.rows > 0 && S.cols >= 4 && S.cols % 4 == 0 && al16(S.base) &&
         (S.seq_stride & 3) == 0 && S.seq_stride >= S.cols &&
         // (the kernel's 32-bit byte offsets reach one slab of 32 rows past the last row: they must not wrap)
         h3_fits31(((long long)S.rows + 32) * S.seq_stride);
}

// ---- form 0 over windows of a halo map (A) against a plain matrix (B) ------------------------------------------
// Everything but the window geometry: gemm_x6p_kernel's switch and grid rule on the kernel's tiles (tile_rows x
// tile_cols; tile_cols == 0: the blocks walk row tiles of every column), 32-bit byte extents, whole slabs and 16-byte
// loads, no on-load transforms, and the epilogue -- wide: x6_epilogue.h's, less the combinations f2g_gemm refuses for
// every kernel; thin: thin_epilogue.h's bias, leaky ReLU, mask + feature-matching term, column sums by atomics and row
// map, everything else refused here, not run on a slower path
inline bool h3_tap_fwd_ok(const f2g_gemm_desc& d, int tile_rows, int tile_cols, bool wide) {
  const f2g_operand& A = d.A;
  const f2g_operand& B = d.B;
  const f2g_epilogue& E = d.E;
  if (d.precision != 4 || d.form != 0 || !A.base || !B.base || !E.C || !host_plain(B) || A.cols != B.cols) return false;
  const int mode = f2g_opt(F2G_OPT_X6P);    // 0 off, 1 chip-filling grids, 2 whatever the grid
  const long long M = A.rows, N = B.rows, ext = x6_a_extent(A);
  if (mode == 0 || M < 1 || N < 1 || ext <= 0 || A.L0u > A.seq_stride) return false;    // (a window stays in its run)
  const long long tiles = ((M + tile_rows - 1) / tile_rows) * (tile_cols ? (N + tile_cols - 1) / tile_cols : 1);
  if (mode < 2 && tiles < 256) return false;
  if (ext * 4 >= 0xe0000000ll || N * B.seq_stride * 4 >= 0xe0000000ll) return false;
  if (!al16(A.base) || !al16(B.base) || (B.seq_stride % 32) || B.seq_stride < B.cols) return false;
  if (A.alpha || A.lrelu_src || B.alpha || B.lrelu_src || d.split_k > 1) return false;
  if (!wide) {
    if (E.aux || E.res || E.colsum_alpha || E.prelu_slope || E.prelu_out || E.scale != 0.f) return false;
    return !(E.atomic || E.accumulate || E.c_bf16 || E.x3_out || E.colsum_part_ld > 0);
  }
  if (!x6e::wide_ok(E, B.rows) || (E.x3_out && E.prelu_out)) return false;
  if (E.prelu_slope && (E.accumulate || E.P0o > 0)) return false;
  return !(E.mask_src && E.accumulate);
}

// ---- form 2: a plain K-major matrix (A) against unbounded five-tap windows of one contiguous map (B) -----------
// Everything but the channel counts (A.cols, B.unit) and the map's rows: a bare atomic add as the epilogue, no on-load
// transforms, A plain and aligned, B unbounded windows of five positions with stride `step`, whole sequences
inline bool h3_tapw_ok(const f2g_gemm_desc& d, int step) {
  const f2g_operand& A = d.A;
  const f2g_operand& B = d.B;
  const f2g_epilogue& E = d.E;
  if (d.form != 2 || d.precision != 4 || !A.base || !B.base || !E.C) return false;
  if (!E.atomic || E.P0o > 0 || E.bias || E.res) return false;
  if ((E.scale != 0.f && E.scale != 1.f) || E.colsum || E.colsum_alpha || E.colsum_part_ld > 0 ||
      E.lrelu_slope != 0.f || E.mask_src || E.aux || E.prelu_slope || E.c_bf16 || E.x3_out || E.accumulate ||
      A.lrelu_src || A.alpha || B.lrelu_src || B.alpha)
    return false;
  if (!host_plain(A) || A.rows < 1 || A.rows != B.rows || !al16(A.base) || (A.seq_stride & 3) ||
      A.seq_stride < A.cols)
    return false;
  if (B.P1 != 1 || B.L1 != 1 || B.P0 < 1 || B.step0 != step || !B.unbounded || B.reflect || !al16(B.base))
    return false;
  return B.cols == 5 * B.unit && B.seglen >= B.cols && (B.rows % B.P0) == 0 && B.pad0 >= 0 && B.pad0 <= 8;
}

// Map rows per sequence under stride-3 windows (B.unit > 0): whole rows (a sequence has seq_stride / unit of them, not
// P0), and windows that overhang a sequence by at most pad0 rows at either end -- 3 (P0 - 1) + 5 - pad0 <= rows + pad0,
// what every layer with Hp = Hout + 4, pad0 = 6, 3 Hout <= Hin + 2 meets; a stride-1 geometry with step0 flipped to 3
// does not.  0 = declined
inline long long h3_tapw3_map_rows(const f2g_operand& B) {
  if (B.seq_stride < B.unit || (B.seq_stride % B.unit)) return 0;
  const long long HpIn = B.seq_stride / B.unit;
  return 3ll * (B.P0 - 1) + 5 - B.pad0 > HpIn + B.pad0 ? 0 : HpIn;
}

// Both operands within h3_fits31: the whole map of `map_rows` rows per sequence, and A
inline bool h3_tapw_extents_ok(const f2g_operand& A, const f2g_operand& B, long long map_rows) {
  return h3_fits31((long long)(B.rows / B.P0) * map_rows * B.unit) && h3_fits31((long long)A.rows * A.seq_stride);
}

}  // namespace
