// Thin epilogue of the kernels whose tile is 128 output rows x all N <= 32 columns, four waves of 32 x 32 -- the data
// gradients that land on a 32-channel map through the row map of a stride residue.  gemm_h3pn_kernel
// (gemm_f16pn.hip) calls it; gemm_h3pn3_kernel (gemm_f16pn3.hip: three such column groups side by side) calls
// row_values_cut and column_sums.  gemm_x6n_kernel (gemm_x6.hip) has the same steps inline, where they were written first:
// calling these functions there moved it from 102 to 104 registers, so it keeps its copy and its device code stays
// what it was.  A change to one belongs in the other.
//
// The generic epilogue (gemm_epilogue) pays one 64-bit division per ELEMENT for that row map (16 per lane and tile,
// ~35 VALU instructions each).  Here the tile's 128 output-row offsets are computed once, one division per ROW, into
// an LDS table, and the elements look them up: bias, leaky ReLU, the leaky-ReLU backward mask with the
// feature-matching term, column sums (atomics after a cross-half shuffle), row-mapped or plain stores.  Nothing else:
// the callers send aux / res / prelu / scale / atomic / accumulate elsewhere or refuse them on the host.
#pragma once
#include "common.h"

namespace thin {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Offsets of the output rows m0 .. m0 + 127 into rowoff[128] (-1 behind row M - 1), by threads 0 .. 127.  The caller
// puts a barrier between this and row_values.
__device__ __forceinline__ void row_offsets(const f2g_epilogue& E, int M, int m0, int tid, long long* rowoff) {
  if (tid >= 128) return;
  const int row = m0 + tid;
  long long off = -1;
  if (row < M) {
    if (E.P0o > 0) {
      const int sq = row / E.P0o;
      off = (long long)sq * E.seq_stride_o + (long long)(row - sq * E.P0o) * E.row_stride_o + E.off_o;
    } else {
      off = (long long)row * E.ldc;
    }
  }
  rowoff[tid] = off;
}

// The wave's 32 x 32 accumulator tile (tile rows wave * 32 .., column li) -> memory.  Returns the lane's part of
// the column sum of what it stored.
__device__ __forceinline__ float row_values(const f2g_epilogue& E, const f32x16& acc, int N, int wave, int li, int h,
                                            const long long* rowoff) {
  const int col = li;
  float cs = 0.f;
  if (col >= N) return cs;
  const float bias = E.bias ? E.bias[col] : 0.f;
  const float fmw = E.fm_ref ? E.fm_w * (E.fm_wdev ? E.fm_wdev[0] : 1.f) : 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const long long ro = rowoff[wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * h];
    if (ro < 0) continue;
    const long long off = ro + col;
    float v = acc[e] + bias;
    if (E.lrelu_slope != 0.f) v = v > 0.f ? v : E.lrelu_slope * v;
    if (E.mask_src) {   // leaky-ReLU backward of the layer below (+ feature-matching term)
      const float y = E.mask_src[off];
      if (E.fm_ref) {
        const float dl = y - E.fm_ref[off];
        v += fmw * (dl > 0.f ? 1.f : (dl < 0.f ? -1.f : 0.f));
      }
      v *= y > 0.f ? 1.f : E.mask_slope;
    }
    cs += v;
    E.C[off] = v;
  }
  return cs;
}

// row_values for a tile of three 32-column groups side by side (gemm_h3pn3_kernel, gemm_f16pn3.hip: f2g_epilogue's
// col_fold / seq_live): the 32 x 32 accumulator tile of tile rows rg * 32 .., columns col0 + li, less the elements
// behind their row's live columns -- rowlive[row] = the columns of that row in front of E.seq_live (<= 0: none) --,
// which are neither stored nor summed.  A function of its own: row_values above stays the code it was for its callers.
// No bias, no leaky ReLU (the caller's host check refuses them).
__device__ __forceinline__ float row_values_cut(const f2g_epilogue& E, const f32x16& acc, int rg, int col0, int li,
                                                int h, const long long* rowoff, const int* rowlive) {
  const int col = col0 + li;
  float cs = 0.f;
  const float fmw = E.fm_ref ? E.fm_w * (E.fm_wdev ? E.fm_wdev[0] : 1.f) : 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int tr = rg * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
    const long long ro = rowoff[tr];
    if (ro < 0 || col >= rowlive[tr]) continue;
    const long long off = ro + col;
    float v = acc[e];
    if (E.mask_src) {   // leaky-ReLU backward of the layer below (+ feature-matching term)
      const float y = E.mask_src[off];
      if (E.fm_ref) {
        const float dl = y - E.fm_ref[off];
        v += fmw * (dl > 0.f ? 1.f : (dl < 0.f ? -1.f : 0.f));
      }
      v *= y > 0.f ? 1.f : E.mask_slope;
    }
    cs += v;
    E.C[off] = v;
  }
  return cs;
}

// Column sums: the two half-waves hold the same column, one atomic per column and wave
__device__ __forceinline__ void column_sums(const f2g_epilogue& E, int N, int li, int h, float cs) {
  if (!E.colsum) return;
  cs += __shfl_xor(cs, 32);
  if (h == 0 && li < N) atomicAdd(E.colsum + li, cs);
}

}  // namespace thin
