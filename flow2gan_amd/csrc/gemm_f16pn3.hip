// fp16x3 data gradient of the MPD's Conv2d(32 -> 128, (5, 1), stride (3, 1)) onto its 32-channel map in ONE launch for
// the three stride residues (gemm_f16pn.hip runs them as three: K = 128 / 256 / 256, 32 columns each through a stride-3
// row map, the 128-channel fp32 gradient map read three times).  With pad 2 and Hout = ceil(Hin / 3), input row
// h = 3 q + rho receives
//     rho = 0: g[q] through tap 2          rho = 1: g[q] through tap 3, g[q + 1] through tap 0
//     rho = 2: g[q] through tap 4, g[q + 1] through tap 1
// so all three read the window [g[q], g[q + 1]], and rows 3 q, 3 q + 1, 3 q + 2 of the result are 96 consecutive floats
// of the halo map: ONE forward-form GEMM, M = S * Hout rows, K = 256 over stride-1 windows of two positions, N = 96
// contiguous columns, against Wc[rho * 32 + ci][j * 128 + co] = w[co][ci][t(rho, j)], whose block (rho = 0, j = 1) is
// zero and is not multiplied.  gemm_h3pn3_kernel is that GEMM; tests/fp16x3_res3_emul.py restates the identity and the
// arithmetic in float64.
//
// OPERAND A is the fp32 map itself (f2g_operand.split = 8, no rscale), staged exactly as gemm_h3pn_kernel<2> stages it
// -- the code below is that kernel's, line for line, and stays a copy because that kernel sits at 256 registers with
// nothing to spare: SEGMENTS of a 128-row tile (the positions the rows of one sequence read, n + 1 entries for n rows,
// at most 17 segments and 145 entries), every position a window of a valid row reads loaded, scaled and split ONCE into
// the 528-byte slab layout for all three residues, nothing else loaded; one power-of-two scale per segment from the
// integer maximum of sign-less bit patterns (thread, the 32 lanes of a position, one LDS word): C is reproducible bit
// for bit run to run, E.colsum (atomics) the one exception.  gemm_f16pn.hip has the layout, gemm_f16p.hip the error
// bound: 3 * 2^-22 sum |g||w| + 2^-28 amax_segment sum |w| per output; the one-tap residue lives under the scale of a
// segment that also holds g[q + 1], which the bound allows for (amax_segment <= amax_seq).
//
// FOUR WAVES, ONE RESIDUE EACH.  The fragments of all 96 rows of Wc are 320 registers, which no wave has.  Each wave
// keeps ONE residue's fragments (row rho * 32 + li of B's f2g_split_f16x2_seq image, split = 7, one scale per row) in
// registers for the block's life and walks the rows of the tile it owns, 32 at a time:
//     wave 0: rho = 1, 128 registers, rows 0 .. 127        wave 2: rho = 0 (g[q] only), 64 registers, rows 0 .. 63
//     wave 1: rho = 2, 128 registers, rows 0 .. 127        wave 3: rho = 0,             64 registers, rows 64 .. 127
// Waves 0 and 1 issue 64 groups of three MFMAs per tile, waves 2 and 3 sixteen: the SIMDs of waves 0 and 1 carry the
// tile (the three launches it replaces put 40 groups on every SIMD), which a launch at the HBM floor of one pass over
// the map can afford on paper -- profiles/fp16x3_tapn3_shapes.txt has what it does.  The LDS reads per tile are those
// of the three launches together (320 KB).  The alternative -- the 80 KB image resident in LDS beside a 64-row stage,
// one block per CU -- reads the weights again for every row group and leaves no second block to hide a tile's loads.
// Per 32-row group: v = (acc0 + 2^-11 acc1) * rscale_seg[row] * rscale_b[col], then thin::row_values_cut with column
// offset 32 rho: mask_src, fm_ref / fm_w / fm_wdev, mask_slope at the output's own address, and
//     E.seq_live: column c of row q is real only while 96 q + c < 32 Hin -- for Hin % 3 != 0 the last row of a sequence
//     computes non-zero values behind its end, which would land in the zero halo rows; they are neither stored nor
//     summed (one word per row in LDS: the row's live columns);
//     E.col_fold = 32: column n stands for channel n % 32; every wave keeps its lane's sum of channel li across the
//     block's tiles and issues one atomic per channel and wave at the end, as gemm_h3pn_kernel does.
// BARRIERS: the two of gemm_h3pn_kernel per tile, outside everything that depends on a wave's residue; every wave
// walks the same tiles (blockIdx.x, + gridDim.x, ... below R.ntiles, known on entry), so all four reach every barrier.
// PREFETCH: not explicit.  With the weights (128), a group's two accumulator sets (32) and its fragments in flight, the
// 76 registers of the next tile's positions do not fit 256.  What there is comes from the roles: waves 2 and 3 finish
// their 16 groups early and request their half of the next tile's positions while waves 0 and 1 still multiply, and
// the CU's second block stages under this one's MFMAs.
//
// RESOURCES (gfx950, tools/kernel_resources.py; DESIGN.md section 3 has the table): 256 threads,
// __launch_bounds__(256, 2); LDS 79,376 bytes = 145 entries x 528 (76,560) + 128 row scales + 128 row entries + 128 row
// offsets (8 bytes) + 128 live-column counts + 2 x 32 segment maxima: two blocks per CU (160 KB).
// Registers: 256 VGPRs (128 of them the weights, 76 the positions in flight), no AGPRs, no scratch, no vector or scalar
// spills; occupancy 2 waves per SIMD = the two blocks.  The row map's division is the one the row tables make anyway
// (E.P0o == A.P0) and the lane indices of the final column sums are taken afresh: either, left alone, cost a spill.
// MEASURED: profiles/fp16x3_tapn3_shapes.txt (tools/fp16x3_tap_shapes.py --tapn3); DESIGN.md section 0 reads it: 138-143
// us for the 175 MB map at B = 64 against 173-185 for the three gemm_x6n_kernel launches (0.79-0.81, 20 of 20 shapes
// beyond both legs' ranges), 1.25 TB/s of map bytes -- twice the launch's HBM floor: the MFMAs of waves 0 and 1 and a
// tile's loads with nothing else in flight are what is left.
#include <stddef.h>
#include <stdint.h>

#include "gemm_f16_checks.h"
#include "gemm_f16_common.h"
#include "split_f16.h"
#include "thin_epilogue.h"

namespace {

constexpr int PITCH = 528;                 // bytes of a staged position: 4 slabs x (64 hi + 64 lo) + 16 (132 dwords)
constexpr int NSEG = 17;                   // segments of a tile at most: 2 + 126 / P0, P0 >= 8 (host check)
constexpr int NTHR = 256;
constexpr int KS = 16;                     // 16-k steps of the whole reduction (two positions x 128 channels)
static_assert(NSEG <= 32, "a tile's segments");

struct h3pn3_lds {
  static constexpr int LPOS = 128 + NSEG;                   // staged entries of a tile
  static constexpr int OPERA = LPOS * PITCH;
  static constexpr int RSTAB = OPERA;                       // the tile's 128 row scales
  static constexpr int RENT = RSTAB + 128 * 4;              // ... first entries
  static constexpr int ROWOFF = RENT + 128 * 4;             // ... output offsets (thin_epilogue.h)
  static constexpr int ROWLIVE = ROWOFF + 128 * 8;          // ... columns in front of E.seq_live
  static constexpr int SEGMAX = ROWLIVE + 128 * 4;          // segment maxima, two sets of 32 words (tile parity)
  static constexpr size_t SMEM = (size_t)SEGMAX + 2 * 32 * 4;
  static constexpr int NJ = (LPOS + 7) / 8;                 // positions per thread: 8 per pass, 32 lanes each
  static_assert(SMEM <= 80 * 1024, "two blocks per CU");
  static_assert(ROWOFF % 8 == 0, "64-bit offsets");
};

struct h3pn3_tap {
  int P0, seqfl, offfl, ntiles;            // rows per sequence; floats per sequence; -pad0 * 128; row tiles
  unsigned rEP;                            // ceil(2^16 / (P0 + 1)): e / EP = e * rEP >> 16 for e < 145 (below)
  unsigned bytes;
};

// `ngroups` 32-row groups of the tile from group rg0 on against this wave's residue: TAPS positions of the window
// (1: the residue that g[q] alone reaches), columns col0 .. col0 + 31.  Returns the lane's part of channel li's sum.
template <int TAPS>
__device__ __forceinline__ float h3pn3_groups(const f2g_epilogue& E, const unsigned char* smemn, const u32x4 (&wq)[KS][2],
                                              int rg0, int ngroups, int col0, float sb, int li, int h) {
  const float* rstab = reinterpret_cast<const float*>(smemn + h3pn3_lds::RSTAB);
  const int* rent = reinterpret_cast<const int*>(smemn + h3pn3_lds::RENT);
  const long long* rowoff = reinterpret_cast<const long long*>(smemn + h3pn3_lds::ROWOFF);
  const int* rowlive = reinterpret_cast<const int*>(smemn + h3pn3_lds::ROWLIVE);
  float cs = 0.f;
#pragma unroll 1
  for (int rg = rg0; rg < rg0 + ngroups; ++rg) {
    const unsigned char* rA = smemn + rent[rg * 32 + li] * PITCH + h * 16;
    f32x16 acc[1], acx[1];
    h3_zero<1>(acc, acx);
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
      for (int sl = 0; sl < 4; ++sl)
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          const int ks = (t * 4 + sl) * 2 + k2;
          const f16x8 ah = *reinterpret_cast<const f16x8*>(rA + t * PITCH + sl * 128 + k2 * 32);
          const f16x8 al = *reinterpret_cast<const f16x8*>(rA + t * PITCH + sl * 128 + 64 + k2 * 32);
          h3_product(acc[0], acx[0], ah, al, __builtin_bit_cast(f16x8, wq[ks][0]), __builtin_bit_cast(f16x8, wq[ks][1]));
        }
    // v = (acc0 + 2^-11 acc1) / s_a[segment of the row] / s_b[col] (gemm_f16_common.h: h3_value)
#pragma unroll
    for (int e = 0; e < 16; ++e)
      acc[0][e] = h3_value(acc[0][e], acx[0][e], rstab[rg * 32 + (e & 3) + 8 * (e >> 2) + 4 * h], sb);
    cs += thin::row_values_cut(E, acc[0], rg, col0, li, h, rowoff, rowlive);
  }
  return cs;
}

__global__ __launch_bounds__(NTHR, 2) void gemm_h3pn3_kernel(const f2g_gemm_desc d, int M, const h3pn3_tap R) {
  using lds = h3pn3_lds;
  constexpr int NJ = lds::NJ;
  extern __shared__ __attribute__((aligned(16))) unsigned char smemn[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, h = lane >> 5;
  const int pe = tid >> 5, pc = tid & 31;  // staging: entry pe + 8 j, 16-byte chunk pc (channels 4 pc .. 4 pc + 3)
  float* rstab = reinterpret_cast<float*>(smemn + lds::RSTAB);
  int* rent = reinterpret_cast<int*>(smemn + lds::RENT);
  long long* rowoff = reinterpret_cast<long long*>(smemn + lds::ROWOFF);
  int* rowlive = reinterpret_cast<int*>(smemn + lds::ROWLIVE);
  unsigned* segmax = reinterpret_cast<unsigned*>(smemn + lds::SEGMAX);
  const int EP = R.P0 + 1;                 // entries of a whole sequence's segment
  __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)d.A.base, 0, R.bytes, 0x00020000);

  // ---- this wave's residue and this lane's weight fragments, for the block's life: wq[k-step][0 hi / 1 lo] = the
  // halves of reduction elements 16 ks + 8 h .. + 7 of row rho * 32 + li (the image: slabs of 32 elements, 64 bytes hi
  // + 64 bytes lo).  The one-tap residue stops at the first position's 8 steps: the zero block is never read.
  const int rho = wave < 2 ? wave + 1 : 0;
  const int nks = wave < 2 ? KS : KS / 2;
  u32x4 wq[KS][2];
  {
    const unsigned rowbytesW = (unsigned)(d.B.seq_stride * 4);
    __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)d.B.base, 0, 96u * rowbytesW, 0x00020000);
    const unsigned vo = (unsigned)(rho * 32 + li) * rowbytesW + h * 16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int p = 0; p < 2; ++p)
        wq[ks][p] = __builtin_amdgcn_raw_buffer_load_b128(rsW, ks < nks ? vo : 0xf0000000u,      // (outside = zeros)
                                                          (ks >> 1) * 128 + p * 64 + (ks & 1) * 32, 0);
  }
  const float sb = d.B.rscale[rho * 32 + li];
  if (tid < 64) segmax[tid] = 0u;
  __syncthreads();

  float cs = 0.f;                          // this lane's part of channel li's sum over the block's tiles
  int par = 0;
  for (int tile = blockIdx.x; tile < R.ntiles; tile += gridDim.x, par ^= 1) {
    // ---- geometry of the tile: its first sequence and window, the entries of its first segment and of all of them
    // (rows past M own none)
    const int m0 = tile * 128;
    const int sq0 = m0 / R.P0, rl0 = m0 - sq0 * R.P0;
    const int nval = M - m0 < 128 ? M - m0 : 128;
    const int n0 = R.P0 - rl0 < nval ? R.P0 - rl0 : nval;
    const int rest = nval - n0, nfull = rest / R.P0, part = rest - nfull * R.P0;
    const int E0 = n0 + 1;
    const int L = E0 + nfull * EP + (part ? part + 1 : 0);
    // entry e -> its segment k and its position q behind the sequence's first window start
    // (e - E0 < 145 and, where the quotient is not 0, EP <= 145: (e - E0) * EP * (rEP - 2^16 / EP) < 2^16 -- exact)
    auto place = [&](int e, int& k, int& q) {
      k = 0, q = e + rl0;
      if (e >= E0) {
        const int e2 = e - E0;
        k = 1 + (int)(((unsigned)e2 * R.rEP) >> 16);
        q = e2 - (k - 1) * EP;
      }
    };
    // (the three loops below each place their entries AGAIN: left to itself the compiler keeps the 19 segment indices
    // and 19 lane masks of the first loop alive beside the positions)
    auto again = [](int e) {
      asm volatile("" : "+v"(e));
      return e;
    };
    unsigned* smx = segmax + 32 * par;
    // ---- request the positions; segment maxima: thread, the 32 lanes of a position, one LDS word per segment
    u32x4 xa[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int e = pe + 8 * j;
      int k, q;
      place(e, k, q);
      // (the byte offset stays under the resource limit: host check; the others lie outside the resource = zeros)
      const unsigned vo = e < L ? ((unsigned)(sq0 + k) * (unsigned)R.seqfl + (unsigned)(R.offfl + q * 128)) * 4u + pc * 16
                                : 0xf0000000u;
      xa[j] = __builtin_amdgcn_raw_buffer_load_b128(rsA, vo, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int e = again(pe + 8 * j);
      const float4 v = make_float4(__uint_as_float(xa[j].x), __uint_as_float(xa[j].y), __uint_as_float(xa[j].z),
                                   __uint_as_float(xa[j].w));
      unsigned m = f2g_f16_amax4(v, 0u);
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) {
        const unsigned t = (unsigned)__shfl_xor((int)m, o);
        m = m > t ? m : t;
      }
      if (pc == 0 && e < L) {
        int k, q;
        place(e, k, q);
        atomicMax(smx + k, m);
      }
    }
    lds_barrier();       // A: the maxima are complete; every wave has left the previous tile's MFMAs and epilogue
    // ---- scale and split the positions into LDS; per row: reciprocal scale, first entry, output offset, live columns;
    // the other parity's maxima to zero (last read before the previous tile's barrier B, next written behind this
    // tile's)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int e = again(pe + 8 * j);
      if (e >= L) continue;
      int k, q;
      place(e, k, q);
      float s, rs;
      f2g_f16_scales(smx[k], s, rs);
      const float4 v = make_float4(__uint_as_float(xa[j].x), __uint_as_float(xa[j].y), __uint_as_float(xa[j].z),
                                   __uint_as_float(xa[j].w));
      const uint4 p = f2g_f16_split4(v, s);                // (h01, h23, l01, l23)
      unsigned char* dst = smemn + e * PITCH + (pc >> 3) * 128 + (pc & 7) * 8;
      *reinterpret_cast<u32x2*>(dst) = u32x2{p.x, p.y};
      *reinterpret_cast<u32x2*>(dst + 64) = u32x2{p.z, p.w};
    }
    if (tid < 128) {
      // (rows past the end read entry 0: staged data, never used, and have no live column)
      const int r = m0 + tid;
      // (E.P0o == A.P0, host check: the row map's division is the one made here -- thin::row_offsets' formula)
      float s, rs = 0.f;
      int entry = 0, live = 0;
      long long off = -1;
      if (r < M) {
        const int sq = r / R.P0, k = sq - sq0, rl = r - sq * R.P0;
        entry = k == 0 ? rl - rl0 : E0 + (k - 1) * EP + rl;
        f2g_f16_scales(smx[k], s, rs);
        off = (long long)sq * d.E.seq_stride_o + (long long)rl * d.E.row_stride_o + d.E.off_o;
        const long long lv = d.E.seq_live - (long long)rl * d.E.row_stride_o;
        live = lv > 96 ? 96 : (int)lv;
      }
      rstab[tid] = rs;
      rent[tid] = entry;
      rowoff[tid] = off;
      rowlive[tid] = live;
    }
    if (tid < 32) segmax[32 * (par ^ 1) + tid] = 0u;
    lds_barrier();       // B: the tile is staged
    // ---- the wave's residue over the rows it owns (wave-uniform: no barrier inside)
    if (wave < 2) cs += h3pn3_groups<2>(d.E, smemn, wq, 0, 4, 32 * rho, sb, li, h);
    else cs += h3pn3_groups<1>(d.E, smemn, wq, (wave - 2) * 2, 2, 0, sb, li, h);
  }
  // (lane indices taken afresh: kept alive across the tile loop they cost the one register the loop does not have)
  int t2 = threadIdx.x;
  asm volatile("" : "+v"(t2));
  thin::column_sums(d.E, 32, t2 & 31, (t2 >> 5) & 1, cs);
}

}  // namespace

// A the fp32 map marked split = 8 under stride-1 windows of 2 positions over 128 channels, 96 columns = three rows of the
// 32-channel halo map side by side (E.col_fold = 32) cut at E.seq_live floats per sequence, row tiles of 128, the thin
// epilogue less bias and leaky ReLU
int f2g_h3pn3_ok(const f2g_gemm_desc& d) {
  const f2g_operand& A = d.A;
  const f2g_epilogue& E = d.E;
  if (A.split != 8 || d.B.rows != 96 || !h3_tap_fwd_ok(d, 128, 0, false)) return 0;
  if (E.bias || E.lrelu_slope != 0.f) return 0;
  if (host_plain(A) || A.P1 != 1 || A.step0 != 1 || A.unit != 128 || A.seglen < A.cols || A.cols != 256) return 0;
  if ((A.seq_stride % A.unit) || A.pad0 > 0 || A.P0 < 8) return 0;      // (P0: NSEG segments)
  if (E.col_fold != 32 || E.P0o != A.P0 || E.row_stride_o != 96) return 0;
  // (the cut lies in the last row of a sequence: every other row is whole, and no row is all cut)
  if ((E.seq_live % 32) || E.seq_live <= 96ll * (A.P0 - 1) || E.seq_live > 96ll * A.P0) return 0;
  return f16_b_image_status(d.B, 7);
}

int f2g_launch_h3pn3(const f2g_gemm_desc& d, hipStream_t st) {
  using lds = h3pn3_lds;
  const int M = d.A.rows;
  dyn_lds_once<gemm_h3pn3_kernel>((int)lds::SMEM);
  h3pn3_tap R;
  R.P0 = d.A.P0, R.seqfl = (int)d.A.seq_stride, R.offfl = -d.A.pad0 * 128, R.ntiles = (M + 127) / 128;
  R.rEP = (65536u + (unsigned)(R.P0 + 1) - 1u) / (unsigned)(R.P0 + 1);
  R.bytes = (unsigned)(x6_a_extent(d.A) * 4);
  const int grid = R.ntiles < 512 ? R.ntiles : 512;      // two resident blocks per CU
  f2g_note_kernel("h3pn3", 1, 6);
  hipLaunchKernelGGL(gemm_h3pn3_kernel, dim3(grid), dim3(NTHR), lds::SMEM, st, d, M, R);
  return f2g_check_launch();
}
