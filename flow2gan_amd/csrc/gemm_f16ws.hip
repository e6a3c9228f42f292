// fp16x3 tap-walking weight gradient of a STRIDED conv layer over halo maps (the MPD's stride-3 layers 128 -> 512 and
// 512 -> 1024; what gemm_leanw6s_kernel, gemm_x6p.hip, runs in the bf16x6 mode):
//   gw[co][t * Cin + ci] += sum over (s, p) of g[s * Hp + p][co] * x[s * HpIn + STRIDE * p + t - pad][ci],  t = 0..TAPS-1
// over f2g_split_f16x2_cols images of the gradient (nseq * Hp x Cout) and of the WHOLE contiguous map (nseq * HpIn x
// Cin, halo rows included).  Tap and stride only select ROWS of the map, so a power-of-two scale per COLUMN (channel)
// of the map is the same for every tap, position and sequence and leaves the sum over rows exactly: the error bound is
// the column image's (split_f16.h), exactly as for gemm_h3wt_kernel (gemm_f16wt.hip).
#include <stddef.h>
#include <stdint.h>

#include "gemm_f16_checks.h"
#include "gemm_f16_common.h"

namespace {

// THE WALK is gemm_leanw6s_kernel's: a block owns a (co tile x ci tile x ALL taps) output and a chunk of whole
// sequences (blockIdx.z); a sequence has Hp gradient rows but HpIn != STRIDE * Hp map rows, so there is no one flat row
// index and the block walks its sequences one by one in slabs of R = 16 gradient rows (one MFMA k step).  Per slab it
// stages the STRIDE * 15 + TAPS map rows they touch -- every row once for all taps --, double-buffered, one barrier
// per slab.  Fragment row of reduction index i and tap t = staged row STRIDE * i + t.  Map rows before or behind the
// buffer, rows of a slab beyond Hp and slabs past the block's last one read as zeros (offset 0x80000000: outside the
// buffer resource; the offset of such a row is replaced, never used).
// THE ARITHMETIC is gemm_h3wt_kernel's: no split and no VALU work on data in the K loop -- a staged 16-byte chunk goes
// to LDS as it lies in the image, its first 8 bytes to the hi plane, the other 8 to the lo plane --,
// v_mfma_f32_32x32x16_f16 into TWO accumulator sets (hi hi, and hi lo' + lo hi' with the factor 2^-11), and the
// rescale by both operands' reciprocal column scales BEFORE the atomic add (it is linear: the sequence chunks are
// added after it).
//
// TILE.  Two accumulator sets of leanw6s's 128 x 128 tile would be 320 registers per wave; gemm_h3wt_kernel's 128 co x
// 64 ci is the known fit: 8 waves = (co quarter wm) x (ci half wq), each 32 co x 32 ci x TAPS x 2 sets = 160
// accumulator registers, two waves per SIMD (one block per CU).
//
// R = 16, not 32.  A sequence's last slab is padded with zero rows, and the Hp of the two layers at the five periods
// (tools/fp16x3_tap_shapes.py: heights) are small: 512 -> 1024 has Hp = 153, 103, 64, 47, 31 -- rows walked with R =
// 16: 160, 112, 64, 48, 32 (waste 4.6, 8.7, 0, 2.1, 3.2 %), with R = 32: 160, 128, 64, 64, 32 (4.6, 24, 0, 36, 3.2 %);
// 128 -> 512 has Hp = 449, 301, 182, 131, 85 -- R = 16: 464, 304, 192, 144, 96 (3.3, 1.0, 5.5, 9.9, 12.9 %), R = 32: 480,
// 320, 192, 160, 96 (6.9, 6.3, 5.5, 22, 12.9 %).  R = 32 would halve the barriers per MFMA, but a slab of 16 already
// carries 15 MFMAs per wave (480 matrix clocks, 960 for the SIMD's two waves) against 24 ds_read_b64_tr_b16 (48 LDS
// clocks, 384 for the block) and 1 + 2 staged chunks per thread: the barrier is not what bounds it, the wasted rows
// would be.  LDS is no constraint either way (below: 41 KB for both stages).
//
// LDS: stage = [g hi | g lo | x hi | x lo].  A gradient row is 128 halves = 256 bytes with leanw6t's swizzle (the row's
// four 64-byte column blocks rotated by row & 3).  A map row is 64 halves = 128 bytes (pitch 128: two rows per 256-byte
// bank line) with its two 64-byte blocks swapped by (row >> 1) & 1.  One half of a transposing read touches four
// reduction rows of one column block, i.e. staged rows r, r + 3, r + 6, r + 9 (any r: any tap's first row).  The
// 64-byte bank group of staged row q is 2 (q & 1) + (block ^ (q >> 1) & 1): rows 3 apart differ in q & 1 (the group's
// high bit), rows 6 apart agree in q & 1 but differ in (q >> 1) & 1 (6 >> 1 is odd: the low bit), so r, r + 3, r + 6,
// r + 9 lie in four different bank groups (unswizzled they would fall onto two).  The second half of a read lies 4
// reduction rows = 4 * STRIDE = 12 staged rows further: (q + 12) >> 1 = (q >> 1) + 6 keeps the swap bit, so the swizzle
// term does not depend on the half (static_assert below; with R = 16 there is one k step per slab).
//
// RESOURCES (tools/kernel_resources.py, gfx950), <5, 3>: 210 VGPRs, 0 AGPRs, 0 scratch, 0 vector or scalar spills, 2
// waves per SIMD; 41984 bytes of LDS (two stages of 2 x 4096 gradient and 2 x 6400 map bytes).
template <int TAPS, int STRIDE>
__global__ __launch_bounds__(512, 1) void gemm_h3ws_kernel(const f2g_gemm_desc d, int nseq, int spb,
                                                           long long xrows) {
  constexpr int R = 16;                          // gradient rows of a slab
  constexpr int XR = (R - 1) * STRIDE + TAPS;    // staged map rows of a slab
  constexpr int GP = 256, XP = 128;              // row pitches
  constexpr int GPL = R * GP, XPL = XR * XP;     // bytes of one plane
  constexpr int XOFF = 2 * GPL;
  constexpr int BUFB = 2 * GPL + 2 * XPL;        // one stage
  constexpr int NXQ = (XR * 16 + 511) / 512;     // map chunks per thread
  static_assert(((4 * STRIDE) >> 1) % 2 == 0, "the map's swizzle term must not depend on the half of a fragment read");
  extern __shared__ __attribute__((aligned(16))) unsigned char sms[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 3, wq = wave >> 2, li = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.x * 128, c0 = blockIdx.y * 64;      // co tile, ci tile
  const int Cin = d.B.unit, pad = d.B.pad0, Hp = d.B.P0;
  const int HpIn = (int)(d.B.seq_stride / Cin);
  const int sq0 = blockIdx.z * spb;
  int sq1 = sq0 + spb;
  if (sq1 > nseq) sq1 = nseq;
  const int nslab = (Hp + R - 1) / R;
  const int nt = (sq1 - sq0) * nslab;
  if (nt <= 0) return;
  __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
      (void*)d.A.base, 0, (unsigned)((long long)nseq * Hp * d.A.seq_stride * 4), 0x00020000);
  __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
      (void*)d.B.base, 0, (unsigned)(xrows * Cin * 4), 0x00020000);
  // staging: gradient chunk cc of slab row r0, map chunk cx of staged rows rx + 32 q
  const int cc = tid & 31, r0 = tid >> 5, cx = tid & 15, rx = tid >> 4;
  const unsigned rowG = (unsigned)(d.A.seq_stride * 4), colG = (unsigned)(m0 + 4 * cc) * 4u;
  const unsigned rowX = (unsigned)Cin * 4u, colX = (unsigned)(c0 + 4 * cx) * 4u;
  const int wofG = r0 * GP + ((((cc >> 3) ^ (r0 & 3))) << 6) + (cc & 7) * 8;
  int wofX[NXQ];
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
  for (int t = 0; t < TAPS; ++t) {
    const int xr = STRIDE * rrow + t;
    rofB[t] = XOFF + xr * XP + (((wq ^ ((xr >> 1) & 1))) << 6) + within;
  }
  f32x16 acc[TAPS], acx[TAPS];
  h3_zero<TAPS>(acc, acx);
  u32x4 xg, xx[NXQ];
  auto gload = [&](int j) {       // slab j of this block: sequence sq0 + j / nslab, gradient rows R (j % nslab) ..
    const int sj = j / nslab, p0 = (j - sj * nslab) * R, sq = sq0 + sj;
    const bool on = j < nt;
    const int p = p0 + r0;
    // (the whole offset in the vector register; a row that is not read has its offset replaced, not used)
    xg = __builtin_amdgcn_raw_buffer_load_b128(
        ra, (on && p < Hp) ? (unsigned)((long long)sq * Hp + p) * rowG + colG : 0x80000000u, 0, 0);
    const long long xb = (long long)sq * HpIn + (long long)STRIDE * p0 - pad;     // map row of staged row 0
#pragma unroll
    for (int q = 0; q < NXQ; ++q) {
      const long long xr = xb + rx + 32 * q;
      const bool ok = on && wofX[q] >= 0 && xr >= 0 && xr < xrows;
      xx[q] = __builtin_amdgcn_raw_buffer_load_b128(rb, ok ? (unsigned)(xr * rowX) + colX : 0x80000000u, 0, 0);
    }
  };
  auto store = [&](unsigned char* buf) {
    *reinterpret_cast<u32x2*>(buf + wofG) = u32x2{xg.x, xg.y};
    *reinterpret_cast<u32x2*>(buf + GPL + wofG) = u32x2{xg.z, xg.w};
#pragma unroll
    for (int q = 0; q < NXQ; ++q)
      if (wofX[q] >= 0) {
        *reinterpret_cast<u32x2*>(buf + wofX[q]) = u32x2{xx[q].x, xx[q].y};
        *reinterpret_cast<u32x2*>(buf + XPL + wofX[q]) = u32x2{xx[q].z, xx[q].w};
      }
  };
  gload(0);
  store(sms);
  gload(1);
  lds_barrier();
  for (int j = 0; j < nt; ++j) {
    const unsigned char* cur = sms + (j & 1) * BUFB;
    // the next slab goes into the other stage (its readers left through the barrier that closed slab j - 1)
    store(sms + ((j + 1) & 1) * BUFB);
    gload(j + 2);
    const f16x8 ah = tr_frag_f16<GP>(cur + rofA);
    const f16x8 al = tr_frag_f16<GP>(cur + GPL + rofA);
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      // (the second half of a read: 4 reduction rows = 4 * STRIDE staged rows further)
      const f16x8 bh = tr_frag_f16<XP, 4 * STRIDE>(cur + rofB[t]);
      const f16x8 bl = tr_frag_f16<XP, 4 * STRIDE>(cur + XPL + rofB[t]);
      h3_product(acc[t], acx[t], ah, al, bh, bl);
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

// Form 2 at precision 4 with a WINDOW operand B of stride 3: f2g_h3wt_ok's conditions (gemm_f16wt.hip) with step0 == 3
// and the map rows of h3_tapw3_map_rows (gemm_f16_checks.h).  The images: the gradient's, and ONE of the whole map.
int f2g_h3ws_ok(const f2g_gemm_desc& d) {
  const f2g_operand& A = d.A;
  const f2g_operand& B = d.B;
  if (!h3_tapw_ok(d, 3) || A.cols < 128 || (A.cols % 128) || B.unit < 128 || (B.unit % 128)) return 0;
  const long long HpIn = h3_tapw3_map_rows(B);
  return HpIn && h3_tapw_extents_ok(A, B, HpIn) ? f16_images_status(A, B, 6) : 0;
}


int f2g_launch_h3ws(const f2g_gemm_desc& d, hipStream_t st) {
  const int M = d.A.cols, K = d.A.rows, Cin = d.B.unit;
  constexpr int TAPS = 5, STRIDE = 3, R = 16;
  constexpr size_t smem = (size_t)2 * (2 * R * 256 + 2 * ((R - 1) * STRIDE + TAPS) * 128);
  dyn_lds_once<gemm_h3ws_kernel<5, 3>>((int)smem);
  // f2g_launch_leanw6t's stride-3 rule on this kernel's 128 x 64 tiles: blocks = tiles x sequence chunks, the chunk
  // count whose block total fills rounds of 256 best, at least 256 reduction rows and whole sequences per block
  const int nseq = K / d.B.P0, tiles = (M / 128) * (Cin / 64);
  int best = 1;
  double beste = 0.0;
  for (int z = 1; z <= nseq && z <= 256; ++z) {
    const int per = (nseq + z - 1) / z;
    if (per * d.B.P0 < 256 && z > 1) break;
    const long long blocks = (long long)tiles * ((nseq + per - 1) / per);
    const double eff = (double)blocks / (double)(((blocks + 255) / 256) * 256);
    if (eff > beste + 0.02) beste = eff, best = z;
  }
  const int spb = (nseq + best - 1) / best, zs = (nseq + spb - 1) / spb;
  const long long xrows = (long long)nseq * (d.B.seq_stride / Cin);
  dim3 grid(M / 128, Cin / 64, zs);
  f2g_note_kernel("h3ws<taps=5,step=3>", d.split_k > 1 ? d.split_k : 1, 6);
  hipLaunchKernelGGL((gemm_h3ws_kernel<5, 3>), grid, dim3(512), smem, st, d, nseq, spb, xrows);
  return f2g_check_launch();
}
