// fp16x3 tap-walking weight gradient of a stride-1 conv layer over halo maps (the 1024-channel MPD layer; what
// gemm_leanw6t_kernel, gemm_x6p.hip, runs in the bf16x6 mode):
//   gw[co][t * Cin + ci] += sum_r g[r][co] * x[r + t - pad][ci],  t = 0..TAPS-1
// over f2g_split_f16x2_cols images of the gradient (r x Cout) and of the WHOLE contiguous map (xrows x Cin, halo rows
// included).  The taps shift ROWS of the map, so a power-of-two scale per COLUMN (channel) of the map is the same for
// every tap and leaves the sum over rows exactly: the error bound is the column image's (split_f16.h).
#include <stddef.h>
#include <stdint.h>

#include "gemm_f16_checks.h"
#include "gemm_f16_common.h"

namespace {

// gemm_leanw6t_kernel's structure: a block owns a (co tile x ci tile x ALL taps) output, a slab stages 32 gradient
// rows and the 32 + TAPS - 1 map rows they touch once (double-buffered, one barrier per slab), the taps walk by
// shifting the transposing fragment reads one row down, map rows before or behind the buffer and slabs past kend
// read as zeros (offset 0x80000000: outside the buffer resource), the K range is cut into blockIdx.z chunks that add
// their results atomically.  From gemm_h3w_kernel: no split arithmetic in the K loop -- a staged 16-byte chunk goes to
// LDS as it lies in memory, its first 8 bytes to the hi plane, the other 8 to the lo plane --, v_mfma_f32_32x32x16_f16
// into TWO accumulator sets (hi hi, and hi lo' + lo hi' with the factor 2^-11), and the rescale by both operands'
// reciprocal column scales BEFORE the atomic add (it is linear: the K chunks are added after it).
//
// REGISTERS.  Two accumulator sets of leanw6t's 2 x TAPS tiles would be 320 registers per wave at two waves per
// SIMD (256 each).  Hence the tile: 128 co x 64 ci, 8 waves = (co quarter wm) x (ci half wq), each wave 32 co x 32 ci
// x TAPS x 2 sets = 160 accumulator registers, two waves per SIMD (one block per CU).  The alternative -- 4 waves of
// 64 co x 32 ci on 320 accumulator registers, one per SIMD -- reads 14 fragments per 30 MFMAs instead of 12 per 15
// but leaves nobody to issue while a wave waits for its fragments; the LDS has the room (below), so the two waves
// per SIMD were kept.
//
// PER SLAB (32 k): a wave issues 2 x (2 + 2 TAPS) = 24 fragments = 48 ds_read_b64_tr_b16 (2 LDS clocks each: 96, 768
// for the block's eight waves) for 2 x 3 TAPS = 30 MFMAs (32 clocks each on its SIMD: 960, 1920 for the SIMD's two
// waves) -- the LDS is busy 0.4 of the matrix pipe's time.  gemm_leanw6t_kernel: 120 MFMAs per wave and slab for
// twice the tile, i.e. 60 against 30 here.  Staging: 1024 + 576 chunks of 16 bytes per slab, 3 or 4 loads and twice
// as many 8-byte LDS stores per thread, no vector ALU work on the data.
//
// LDS: stage = [g hi | g lo | x hi | x lo]; a gradient row is 128 halves = 256 bytes with leanw6t's swizzle (the row's
// four 64-byte column blocks rotated by row & 3), a map row 64 halves = 128 bytes with its two blocks swapped by
// (row >> 1) & 1: four consecutive rows of one column block -- what one half of a transposing read touches, from any
// tap's first row -- lie in four different 64-byte bank groups.
template <int TAPS>
__global__ __launch_bounds__(512, 1) void gemm_h3wt_kernel(const f2g_gemm_desc d, int K, int kchunk,
                                                           long long xrows) {
  constexpr int XR = 32 + TAPS - 1;              // staged map rows: the slab's 32 + the taps' overhang
  constexpr int GP = 256, XP = 128;              // row pitches
  constexpr int GPL = 32 * GP, XPL = XR * XP;    // bytes of one plane
  constexpr int XOFF = 2 * GPL;
  constexpr int BUFB = 2 * GPL + 2 * XPL;        // one stage
  constexpr int NXQ = (XR * 16 + 511) / 512;     // map chunks per thread
  extern __shared__ __attribute__((aligned(16))) unsigned char smt[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 3, wq = wave >> 2, li = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.x * 128, c0 = blockIdx.y * 64;      // co tile, ci tile
  const int kbeg = blockIdx.z * kchunk;
  int kend = kbeg + kchunk;
  if (kend > K) kend = K;
  const int nt = (kend - kbeg + 31) / 32;
  if (nt <= 0) return;
  const int Cin = d.B.unit, pad = d.B.pad0;
  __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
      (void*)d.A.base, 0, (unsigned)((long long)K * d.A.seq_stride * 4), 0x00020000);
  __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
      (void*)d.B.base, 0, (unsigned)(xrows * Cin * 4), 0x00020000);
  // staging: gradient chunk cc of rows r0 + 16 q, map chunk cx of rows rx + 32 q
  const int cc = tid & 31, r0 = tid >> 5, cx = tid & 15, rx = tid >> 4;
  unsigned offG[2];
  int wofG[2], wofX[NXQ];
  const unsigned rowG = (unsigned)(d.A.seq_stride * 4);
  const unsigned rowX = (unsigned)Cin * 4u, colX = (unsigned)(c0 + 4 * cx) * 4u;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int r = r0 + 16 * q;
    offG[q] = (unsigned)r * rowG + (unsigned)(m0 + 4 * cc) * 4u;
    wofG[q] = r * GP + ((((cc >> 3) ^ (r & 3))) << 6) + (cc & 7) * 8;
  }
#pragma unroll
  for (int q = 0; q < NXQ; ++q) {
    const int r = rx + 32 * q;
    wofX[q] = r < XR ? XOFF + r * XP + ((((cx >> 3) ^ ((r >> 1) & 1))) << 6) + (cx & 7) * 8 : -1;
  }
  // transposed-read roles (gemm_leanw6_kernel): 16-lane group g4, lane i16 -> row (g4 >> 1) * 8 + (i16 >> 2)
  // (+4 for the second half), 8 bytes at (g4 & 1) * 32 + (i16 & 3) * 8 of the tile's 64-byte column block
  const int g4 = lane >> 4, i16 = lane & 15;
  const int rrow = (g4 >> 1) * 8 + (i16 >> 2), within = (g4 & 1) * 32 + (i16 & 3) * 8;
  const int rofA = rrow * GP + (((wm ^ (rrow & 3))) << 6) + within;
  int rofB[TAPS];
#pragma unroll
  for (int t = 0; t < TAPS; ++t) rofB[t] = XOFF + (rrow + t) * XP + (((wq ^ (((rrow + t) >> 1) & 1))) << 6) + within;
  f32x16 acc[TAPS], acx[TAPS];
  h3_zero<TAPS>(acc, acx);
  u32x4 xg[2], xx[NXQ];
  auto gload = [&](int s) {       // slab s of this block's chunk (rows kbeg + 32 s ..); past the end: zeros
    const int kr = kbeg + 32 * s;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int r = kr + r0 + 16 * q;
      // (the whole offset in the vector register, as for the map: a row past kend must not be read, and its
      // offset -- which may have wrapped -- is replaced, not used)
      xg[q] = __builtin_amdgcn_raw_buffer_load_b128(
          ra, (s < nt && r < kend) ? (unsigned)kr * rowG + offG[q] : 0x80000000u, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < NXQ; ++q) {
      const long long xr = (long long)kr - pad + rx + 32 * q;        // flat map row of staged row rx + 32 q
      const bool ok = s < nt && wofX[q] >= 0 && xr >= 0 && xr < xrows;
      xx[q] = __builtin_amdgcn_raw_buffer_load_b128(rb, ok ? (unsigned)(xr * rowX) + colX : 0x80000000u, 0, 0);
    }
  };
  auto store = [&](unsigned char* buf) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      *reinterpret_cast<u32x2*>(buf + wofG[q]) = u32x2{xg[q].x, xg[q].y};
      *reinterpret_cast<u32x2*>(buf + GPL + wofG[q]) = u32x2{xg[q].z, xg[q].w};
    }
#pragma unroll
    for (int q = 0; q < NXQ; ++q)
      if (wofX[q] >= 0) {
        *reinterpret_cast<u32x2*>(buf + wofX[q]) = u32x2{xx[q].x, xx[q].y};
        *reinterpret_cast<u32x2*>(buf + XPL + wofX[q]) = u32x2{xx[q].z, xx[q].w};
      }
  };
  gload(0);
  store(smt);
  gload(1);
  lds_barrier();
  for (int s = 0; s < nt; ++s) {
    const unsigned char* cur = smt + (s & 1) * BUFB;
    // the next slab goes into the other stage (its readers left through the barrier that closed slab s - 1)
    store(smt + ((s + 1) & 1) * BUFB);
    gload(s + 2);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const f16x8 ah = tr_frag_f16<GP>(cur + ks * 16 * GP + rofA);
      const f16x8 al = tr_frag_f16<GP>(cur + ks * 16 * GP + GPL + rofA);
#pragma unroll
      for (int t = 0; t < TAPS; ++t) {
        const f16x8 bh = tr_frag_f16<XP>(cur + ks * 16 * XP + rofB[t]);
        const f16x8 bl = tr_frag_f16<XP>(cur + ks * 16 * XP + XPL + rofB[t]);
        h3_product(acc[t], acx[t], ah, al, bh, bl);
      }
    }
    lds_barrier();
  }
  // gw[co][t * Cin + ci] += (acc + 2^-11 acx) / s_g[co] / s_x[ci] (gemm_f16_common.h: h3_value): rows m0 + wm * 32 +
  // (MFMA row), columns t * Cin + c0 + wq * 32 + li
  float* C0 = d.E.C;
  const int ci = c0 + wq * 32 + li;
  const float sb = d.B.rscale[ci];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int row = m0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
    const float sa = d.A.rscale[row];
    float* crow = C0 + (long long)row * d.E.ldc + ci;
#pragma unroll
    for (int t = 0; t < TAPS; ++t) atomicAdd(crow + t * Cin, h3_value(acc[t][e], acx[t][e], sa, sb));
  }
}

}  // namespace

// Form 2 at precision 4 with a WINDOW operand B: f2g_leanw6t_ok's conditions for a stride-1 layer (gemm_x6p.hip) --
// A a plain matrix of whole 128-column tiles, B unbounded stride-1 windows of 5 positions x unit channels (unit a
// multiple of 128) over one contiguous map (h3_tapw_ok, gemm_f16_checks.h) -- over f2g_split_f16x2_cols images of the
// gradient and of the whole map.
int f2g_h3wt_ok(const f2g_gemm_desc& d) {
  const f2g_operand& A = d.A;
  const f2g_operand& B = d.B;
  if (!h3_tapw_ok(d, 1) || A.cols < 128 || (A.cols % 128) || B.unit < 128 || (B.unit % 128)) return 0;
  if (B.seq_stride != (long long)B.P0 * B.unit) return 0;     // (one flat row index for the whole buffer)
  return h3_tapw_extents_ok(A, B, B.P0) ? f16_images_status(A, B, 6) : 0;
}


int f2g_launch_h3wt(const f2g_gemm_desc& d, hipStream_t st) {
  const int M = d.A.cols, K = d.A.rows, Cin = d.B.unit;
  constexpr int TAPS = 5;
  constexpr size_t smem = (size_t)2 * (2 * 32 * 256 + 2 * (32 + TAPS - 1) * 128);
  dyn_lds_once<gemm_h3wt_kernel<5>>((int)smem);
  // f2g_launch_leanw6t's rule on this kernel's 128 x 64 tiles: one block per CU, the rows split so that tiles x
  // chunks fill rounds of 256 blocks, at least 1024 rows per chunk
  const int tiles = (M / 128) * (Cin / 64);
  int best = 1;
  double beste = 0.0;
  for (int z = 1; z <= 64; ++z) {
    const long long blocks = (long long)tiles * z;
    if ((long long)K / z < 1024) break;
    const double eff = (double)blocks / (double)(((blocks + 255) / 256) * 256);
    if (eff > beste + 0.02) beste = eff, best = z;
  }
  const int kchunk = ((K + best - 1) / best + 31) / 32 * 32;
  const int zs = (K + kchunk - 1) / kchunk;
  const long long xrows = (long long)(d.B.rows / d.B.P0) * d.B.P0;
  dim3 grid(M / 128, Cin / 64, zs);
  f2g_note_kernel("h3wt<taps=5>", d.split_k > 1 ? d.split_k : 1, 6);
  hipLaunchKernelGGL(gemm_h3wt_kernel<5>, grid, dim3(512), smem, st, d, K, kchunk, xrows);
  return f2g_check_launch();
}
