// K-major weight-gradient kernels of the implicit-GEMM family (form 2: C[m,n] (+)= sum_r A[r,m] * B[r,n]);
// gemm.hip has the family, gemm_common.h what they share.
#include <stddef.h>
#include <stdint.h>

#include "gemm_common.h"

namespace {

// ---- lean weight-gradient kernel, split-bf16 --------------------------------------------------
// C[m,n] (+)= sum_r A[r,m] * B[r,n]: both operands are K-MAJOR (the reduction walks rows, memory is
// contiguous along m / n), while a bf16 MFMA wants 8 consecutive k per lane.  The transposition is
// done by the LDS itself: slabs of 32 rows are staged exactly as they lie in memory (pre-split
// images: a 16-byte chunk = four m as hi | lo, stored as two 8-byte halves into a hi and a lo plane
// of 32 x 128 bf16) and read back with ds_read_b64_tr_b16, which hands lane c of a 16-lane group
// column c of a 4 (k) x 16 (m) block whose 8-byte pieces the group's lanes point at -- two such reads
// = the 8 k of one operand.  Rows are 256 bytes; the 64-byte column blocks are XOR-swizzled with
// (row & 3) so that the four rows of a transposed block fall on different banks (a padded pitch
// would push the tile past two blocks per CU).  Everything else is the lean kernel's recipe:
// buffer loads with the K advance in a scalar register, rows past the end out of range = zeros, two
// register stages, LDS stores behind the MFMAs, fragments prefetched across the barrier.
// A: plain (R x M).  B: plain, or a 1-D window operand (rows = (sequence, position), P1 = 1, one
// segment) flagged `unbounded`: windows may reach past the ends of their sequence because the caller
// guarantees that those rows of A are zero (halo layout of the MPD maps) -- the per-row offsets are
// recomputed every slab (one magic-number division per staged row).

template <bool BWIN>
__global__ __launch_bounds__(256, 2)
void gemm_leanw3_kernel(const f2g_gemm_desc d, int M, int N, int K, int kchunk) {
  constexpr int PL = 32 * 256;            // bytes of one plane (32 rows x 128 bf16)
  constexpr int BUF = 4 * PL;             // [A hi | A lo | B hi | B lo]
  extern __shared__ __attribute__((aligned(16))) float smem[];
  unsigned char* sm = reinterpret_cast<unsigned char*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, h = lane >> 5;
  int m0, n0;
  tile_of_block(128, 128, m0, n0);
  const int kbeg = blockIdx.z * kchunk;
  int kend = kbeg + kchunk;
  if (kend > K) kend = K;
  const int nt = (kend - kbeg + BK - 1) / BK;
  if (nt <= 0) return;

  // staging: thread = (row rid + 8q of the slab, 16-byte chunk c of the 128-wide tile row)
  const int rid = tid >> 5, c = tid & 31;
  __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
      (void*)d.A.base, 0, (unsigned)((long long)K * d.A.seq_stride * 4), 0x00020000);
  const long long b_bytes = BWIN ? (long long)(d.B.rows / d.B.P0) * d.B.seq_stride * 4
                                 : (long long)K * d.B.seq_stride * 4;
  __amdgpu_buffer_rsrc_t rb =
      __builtin_amdgcn_make_buffer_rsrc((void*)d.B.base, 0, (unsigned)b_bytes, 0x00020000);
  unsigned offA[4], offB[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    offA[q] = (unsigned)(((long long)(rid + 8 * q) * d.A.seq_stride + m0 + 4 * c) * 4);
    offB[q] = (unsigned)(((long long)(rid + 8 * q) * d.B.seq_stride + n0 + 4 * c) * 4);
  }
  const int stepA = (int)(BK * d.A.seq_stride * 4), stepB = (int)(BK * d.B.seq_stride * 4);
  const unsigned mgP0 = BWIN ? magic_of(d.B.P0) : 0u;
  const int colB = (n0 + 4 * c) * 4;
  // LDS store offsets (row r, chunk c): r*256 + (((c >> 3) ^ (r & 3)) << 6) + (c & 7)*8
  int wofs[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = rid + 8 * q;
    wofs[q] = r * 256 + ((((c >> 3) ^ (r & 3))) << 6) + (c & 7) * 8;
  }
  // transposed-fragment addresses: 16-lane group g = (m half, k half), lane i = (row i>>2, quad i&3)
  const int g = lane >> 4, i16 = lane & 15;
  const int rrow = (g >> 1) * 8 + (i16 >> 2), sw = i16 >> 2, within = (g & 1) * 32 + (i16 & 3) * 8;
  int rofA[2], rofB[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    rofA[t] = rrow * 256 + ((((wm * 2 + t) ^ sw)) << 6) + within;
    rofB[t] = rrow * 256 + ((((wn * 2 + t) ^ sw)) << 6) + within;
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

  int ka = (int)((long long)kbeg * d.A.seq_stride * 4), kb = (int)((long long)kbeg * d.B.seq_stride * 4);
  const int ka0 = ka, kb0 = kb;
  int srow = kbeg;   // first row of the slab being loaded (window operands)
  auto gload = [&](bool valid, u32x4 (&la)[4], u32x4 (&lb)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      la[q] = __builtin_amdgcn_raw_buffer_load_b128(ra, offA[q], valid ? ka : ka0, 0);
      if constexpr (BWIN) {
        const int r = (valid ? srow : kbeg) + rid + 8 * q;
        const int sq = fast_div(r, d.B.P0, mgP0), p = r - sq * d.B.P0;
        const long long off = ((long long)sq * d.B.seq_stride + (long long)(p * d.B.step0 - d.B.pad0) * d.B.unit) * 4 + colB;
        const unsigned vo = (r < K && off >= 0 && off < b_bytes) ? (unsigned)off : 0x80000000u;
        lb[q] = __builtin_amdgcn_raw_buffer_load_b128(rb, vo, 0, 0);
      } else {
        lb[q] = __builtin_amdgcn_raw_buffer_load_b128(rb, offB[q], valid ? kb : kb0, 0);
      }
    }
  };
  auto advance = [&]() {
    ka += stepA;
    kb += stepB;
    srow += BK;
  };
  auto lstore = [&](int bufoff, const u32x4 (&la)[4], const u32x4 (&lb)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned char* pa = sm + bufoff + wofs[q];
      *reinterpret_cast<u32x2*>(pa) = u32x2{la[q].x, la[q].y};
      *reinterpret_cast<u32x2*>(pa + PL) = u32x2{la[q].z, la[q].w};
      *reinterpret_cast<u32x2*>(pa + 2 * PL) = u32x2{lb[q].x, lb[q].y};
      *reinterpret_cast<u32x2*>(pa + 3 * PL) = u32x2{lb[q].z, lb[q].w};
    }
  };
  bf16x8 fa0[4], fb0[4], fa1[4], fb1[4];   // [0..1] hi of the two sub-tiles, [2..3] lo
  auto frags = [&](int bufoff, int ks, bf16x8 (&fa)[4], bf16x8 (&fb)[4]) {
    const unsigned char* base = sm + bufoff + ks * 16 * 256;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      fa[t] = tr_frag(base + rofA[t]);
      fa[2 + t] = tr_frag(base + PL + rofA[t]);
      fb[t] = tr_frag(base + 2 * PL + rofB[t]);
      fb[2 + t] = tr_frag(base + 3 * PL + rofB[t]);
    }
  };
  auto mfma12 = [&](const bf16x8 (&fa)[4], const bf16x8 (&fb)[4]) {
#pragma unroll
    for (int term = 0; term < 3; ++term)
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          const bf16x8 av = term == 0 ? fa[2 + mi] : fa[mi];
          const bf16x8 bv = term == 1 ? fb[2 + ni] : fb[ni];
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[mi][ni], 0, 0, 0);
        }
  };
  u32x4 xa[4], xb[4], ya[4], yb[4];
  gload(true, xa, xb);
  lstore(0, xa, xb);
  advance();
  gload(nt > 1, xa, xb);
  __syncthreads();
  frags(0, 0, fa0, fb0);
  auto step3 = [&](int t, int curoff, int nxtoff, const u32x4 (&wa)[4], const u32x4 (&wb)[4],
                   u32x4 (&la)[4], u32x4 (&lb)[4]) {
    frags(curoff, 1, fa1, fb1);
    advance();
    gload(t + 2 < nt, la, lb);    // past the end: re-read the first slab (never used)
    mfma12(fa0, fb0);
    lstore(nxtoff, wa, wb);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    frags(nxtoff, 0, fa0, fb0);
    mfma12(fa1, fb1);
    __builtin_amdgcn_sched_barrier(0);
  };
  int t = 0;
  for (; t + 1 < nt; t += 2) {
    step3(t, 0, BUF, xa, xb, ya, yb);
    step3(t + 1, BUF, 0, ya, yb, xa, xb);
  }
  if (t < nt) step3(t, 0, BUF, xa, xb, ya, yb);
  gemm_epilogue<2, 2>(d.E, acc, M, N, m0, n0, wm, wn, li, h, blockIdx.z == 0);
}

// ---- weight gradient with fp32-class products on the bf16 pipe (precision 3, form 2) -----------------
// The operands of gemm_leanw3_kernel (A plain R x M, B plain or an unbounded 1-D window), read as the
// fp32 tensors they are: a weight gradient reduces over ROWS, so the row-major three-piece images of
// the forward kernel are of no use here -- instead every thread splits the 4-float chunks it loads
// into three bf16 pieces on their way into LDS (5.5 VALU instructions per element next to 48 MFMAs
// per slab and wave: the other block of the CU runs its MFMAs meanwhile), K-major planes
// [A p0 | A p1 | A p2 | B p0 | B p1 | B p2] of 32 rows x 128 bf16 with gemm_leanw3_kernel's swizzle, the
// transposing ds_read_b64_tr_b16 fragments, and the six products with i + j <= 2 (smallest first).
// One 48 KB LDS buffer, two blocks per CU:  split + store slab t -> request slab t + 1 -> barrier ->
// read its 24 fragments -> barrier -> 48 MFMAs.
template <bool BWIN>
__global__ __launch_bounds__(256, 2)
void gemm_leanw6_kernel(const f2g_gemm_desc d, int M, int N, int K, int kchunk) {
  constexpr int PL = 32 * 256;            // bytes of one plane (32 rows x 128 bf16)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  unsigned char* sm = reinterpret_cast<unsigned char*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, h = lane >> 5;
  int m0, n0;
  tile_of_block(128, 128, m0, n0);
  const int kbeg = blockIdx.z * kchunk;
  int kend = kbeg + kchunk;
  if (kend > K) kend = K;
  const int nt = (kend - kbeg + BK - 1) / BK;
  if (nt <= 0) return;
  const int rid = tid >> 5, c = tid & 31;
  __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
      (void*)d.A.base, 0, (unsigned)((long long)K * d.A.seq_stride * 4), 0x00020000);
  const long long b_bytes = BWIN ? (long long)(d.B.rows / d.B.P0) * d.B.seq_stride * 4
                                 : (long long)K * d.B.seq_stride * 4;
  __amdgpu_buffer_rsrc_t rb =
      __builtin_amdgcn_make_buffer_rsrc((void*)d.B.base, 0, (unsigned)b_bytes, 0x00020000);
  unsigned offA[4], offB[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    offA[q] = (unsigned)(((long long)(rid + 8 * q) * d.A.seq_stride + m0 + 4 * c) * 4);
    offB[q] = (unsigned)(((long long)(rid + 8 * q) * d.B.seq_stride + n0 + 4 * c) * 4);
  }
  const int stepA = (int)(BK * d.A.seq_stride * 4), stepB = (int)(BK * d.B.seq_stride * 4);
  const unsigned mgP0 = BWIN ? magic_of(d.B.P0) : 0u;
  const int p0one = BWIN && d.B.P0 == 1 ? -1 : 0;
  const int colB = (n0 + 4 * c) * 4;
  int wofs[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = rid + 8 * q;
    wofs[q] = r * 256 + ((((c >> 3) ^ (r & 3))) << 6) + (c & 7) * 8;
  }
  const int g = lane >> 4, i16 = lane & 15;
  const int rrow = (g >> 1) * 8 + (i16 >> 2), sw = i16 >> 2, within = (g & 1) * 32 + (i16 & 3) * 8;
  int rofA[2], rofB[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    rofA[t] = rrow * 256 + ((((wm * 2 + t) ^ sw)) << 6) + within;
    rofB[t] = rrow * 256 + ((((wn * 2 + t) ^ sw)) << 6) + within;
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

  const int ka0 = (int)((long long)kbeg * d.A.seq_stride * 4), kb0 = (int)((long long)kbeg * d.B.seq_stride * 4);
  u32x4 xa[4], xb[4];
  // chunk q (rows rid + 8 q) of slab s of this block's K range; s >= nt: the first slab again (never used)
  auto gload1 = [&](int q, int s) {
    const bool valid = s < nt;
    const int s_ = valid ? s : 0;
    // rows past K pair with nothing: zeros (the resource ends at K rows for A; B is tested)
    const int r = kbeg + s_ * BK + rid + 8 * q;
    // (an offset with bit 31 set lies behind every resource: the load returns zeros.  Written as arithmetic: as a
    // select the compiler turned it into two loads under complementary exec masks -- a branch inside the chain)
    const unsigned past = (unsigned)(r >= K) << 31;
    xa[q] = __builtin_amdgcn_raw_buffer_load_b128(ra, offA[q] | past, ka0 + s_ * stepA, 0);
    if constexpr (BWIN) {
      // (fast_div without its d == 1 branch: control flow would cut the MFMA chain's scheduling region)
      int sq = (int)__umulhi((unsigned)r, mgP0);
      sq -= (sq * d.B.P0 > r) ? 1 : 0;
      sq += (r - sq) & p0one;
      const int pp = r - sq * d.B.P0;
      const long long off = ((long long)sq * d.B.seq_stride + (long long)(pp * d.B.step0 - d.B.pad0) * d.B.unit) * 4 + colB;
      const unsigned vo = (unsigned)off | ((unsigned)!(r < K && off >= 0 && off < b_bytes) << 31);
      xb[q] = __builtin_amdgcn_raw_buffer_load_b128(rb, vo, 0, 0);
    } else {
      xb[q] = __builtin_amdgcn_raw_buffer_load_b128(rb, offB[q] | past, kb0 + s_ * stepB, 0);
    }
  };
  auto stage = [&](int q) {      // split chunk q of both operands into the K-major planes
    u32x2 p0, p1, p2;
    unsigned char* pa = sm + wofs[q];
    split3x4(xa[q], p0, p1, p2);
    *reinterpret_cast<u32x2*>(pa) = p0;
    *reinterpret_cast<u32x2*>(pa + PL) = p1;
    *reinterpret_cast<u32x2*>(pa + 2 * PL) = p2;
    split3x4(xb[q], p0, p1, p2);
    *reinterpret_cast<u32x2*>(pa + 3 * PL) = p0;
    *reinterpret_cast<u32x2*>(pa + 4 * PL) = p1;
    *reinterpret_cast<u32x2*>(pa + 5 * PL) = p2;
  };
  bf16x8 fa[2][3][2], fb[2][3][2];
  auto frags = [&]() {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int pc = 0; pc < 3; ++pc)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          fa[ks][pc][tt] = tr_frag(sm + ks * 16 * 256 + pc * PL + rofA[tt]);
          fb[ks][pc][tt] = tr_frag(sm + ks * 16 * 256 + (3 + pc) * PL + rofB[tt]);
        }
  };
  // the 48 MFMAs of a slab as 12 groups of four (one product term of one k step), smallest terms first
  auto mf4 = [&](int g) {
    const int ks = g / 6, r = g % 6;
    const int i = r == 0 ? 0 : r == 1 ? 1 : r == 2 ? 2 : r == 3 ? 0 : r == 4 ? 1 : 0;
    const int j = r < 3 ? 2 - i : r < 5 ? 1 - i : 0;
    if ((F2G_X6LAB & 32) && g != 0) return;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][i][mi], fb[ks][j][ni], acc[mi][ni], 0, 0, 0);
  };
  // Schedule (round 6; gemm_x6f_kernel has the measurements): the single operand buffer is dead once every wave
  // holds its fragments, so slab t + 1 is split and stored BETWEEN the MFMAs of slab t, in the same wave's
  // instruction stream -- one chunk of either operand per quarter of the chain, its registers requested again for
  // slab t + 2 at once --, and only barrier, fragment reads, barrier stand between two MFMA chains.
#pragma unroll
  for (int q = 0; q < 4; ++q) gload1(q, 0);
#pragma unroll
  for (int q = 0; q < 4; ++q) stage(q);
#pragma unroll
  for (int q = 0; q < 4; ++q) gload1(q, 1);
  lds_barrier();
  frags();
  lds_barrier();
  for (int t = 0; t + 1 < nt; ++t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      mf4(3 * q);
      stage(q);
      mf4(3 * q + 1);
      gload1(q, t + 2);
      mf4(3 * q + 2);
#if !(F2G_X6LAB & 128)
#pragma unroll
      for (int m = 0; m < 12; ++m) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, BWIN ? 5 : 4, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x200, 6, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
#endif
      __builtin_amdgcn_sched_barrier(0);
    }
    lds_barrier();
    frags();
    lds_barrier();
  }
#pragma unroll
  for (int g = 0; g < 12; ++g) mf4(g);
  gemm_epilogue<2, 2>(d.E, acc, M, N, m0, n0, wm, wn, li, h, blockIdx.z == 0);
}

// ---- lean weight-gradient kernel, exact fp32 ---------------------------------------------------
// Same operands as gemm_leanw3_kernel (A plain R x M, B plain or an unbounded 1-D window), fp32 MFMA.
// v_mfma_f32_32x32x2_f32 takes ONE k per lane half, so K-major tiles are its natural layout: the
// slab [32 k][128 m] is stored as it arrives (ds_write_b128) and lane (m = li, k = 2s + hh) reads
// single floats, 32 consecutive ones per lane half: conflict-free ds_read_b32 at per-lane base +
// immediate offsets.  As in the forward lean kernel nothing in the K loop touches the vector ALU:
// the K advance of both operands is scalar.  For a window operand the slab's first row (sequence,
// position) is walked by SALU and the rows of a slab add a per-thread constant; only a slab that
// straddles a sequence end (or starts before the buffer) pays a few VALU instructions to redirect
// the rows behind the boundary.
template <bool BWIN>
__global__ __launch_bounds__(256, 2)
void gemm_leanw_kernel(const f2g_gemm_desc d, int M, int N, int K, int kchunk) {
  constexpr int TP = 32 * 128;            // floats of one operand tile
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [buf][A tile | B tile]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, h = lane >> 5;
  int m0, n0;
  tile_of_block(128, 128, m0, n0);
  const int kbeg = blockIdx.z * kchunk;
  int kend = kbeg + kchunk;
  if (kend > K) kend = K;
  const int nt = (kend - kbeg + BK - 1) / BK;
  if (nt <= 0) return;
  const int rid = tid >> 5, c = tid & 31;
  __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
      (void*)d.A.base, 0, (unsigned)((long long)K * d.A.seq_stride * 4), 0x00020000);
  const long long b_bytes = BWIN ? (long long)(d.B.rows / d.B.P0) * d.B.seq_stride * 4
                                 : (long long)K * d.B.seq_stride * 4;
  __amdgpu_buffer_rsrc_t rb =
      __builtin_amdgcn_make_buffer_rsrc((void*)d.B.base, 0, (unsigned)b_bytes, 0x00020000);
  const long long rowB = BWIN ? (long long)d.B.step0 * d.B.unit * 4 : d.B.seq_stride * 4;   // bytes per row
  unsigned offA[4], offB[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    offA[q] = (unsigned)(((long long)(rid + 8 * q) * d.A.seq_stride + m0 + 4 * c) * 4);
    offB[q] = (unsigned)((long long)(rid + 8 * q) * rowB + (n0 + 4 * c) * 4);
  }
  const int stepA = (int)(BK * d.A.seq_stride * 4);
  int ka = (int)((long long)kbeg * d.A.seq_stride * 4);
  const int ka0 = ka;
  // B: scalar byte offset of the slab's first row.  Window operand: (sequence sq, position p0)
  int sq = 0, p0 = 0;
  long long kb = (long long)kbeg * d.B.seq_stride * 4;
  const int wrapjump = BWIN ? (int)((d.B.seq_stride - (long long)d.B.P0 * d.B.step0 * d.B.unit) * 4) : 0;
  if (BWIN) {
    sq = kbeg / d.B.P0;
    p0 = kbeg - sq * d.B.P0;
    kb = ((long long)sq * d.B.seq_stride + (long long)(p0 * d.B.step0 - d.B.pad0) * d.B.unit) * 4;
  }
  const long long kb_first = kb;
  const int p_first = p0;
  float* wA = smem + rid * 128 + c * 4;
  float* wB = smem + TP + rid * 128 + c * 4;
  const float* rA = smem + h * 128 + wm * 64 + li;
  const float* rB = smem + TP + h * 128 + wn * 64 + li;

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

  auto gload = [&](int soa, long long sob, int pp, u32x4 (&la)[4], u32x4 (&lb)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) la[q] = __builtin_amdgcn_raw_buffer_load_b128(ra, offA[q], soa, 0);
    if (BWIN && (pp + BK > d.B.P0 || sob < 0 || sob + 32 * rowB + 512 > 0x7fffffffll)) {
      // (rare, uniform) the slab straddles a sequence end or touches the buffer's ends: per-row offsets
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = rid + 8 * q;
        // (P0 >= 16 is required: a slab's 32 rows cross at most two sequence ends)
        const int wraps = (pp + r >= d.B.P0 ? 1 : 0) + (pp + r >= 2 * d.B.P0 ? 1 : 0);
        long long off = sob + (long long)offB[q] + (long long)wraps * wrapjump;
        if (pp + r >= 3 * d.B.P0) off = -1;   // (defensive)
        const unsigned vo = (off >= 0 && off < b_bytes) ? (unsigned)off : 0x80000000u;
        lb[q] = __builtin_amdgcn_raw_buffer_load_b128(rb, vo, 0, 0);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) lb[q] = __builtin_amdgcn_raw_buffer_load_b128(rb, offB[q], (int)sob, 0);
    }
  };
  auto advance = [&]() {
    ka += stepA;
    if (BWIN) {
      p0 += BK;
      kb += BK * rowB;
      while (p0 >= d.B.P0) {      // (twice for sequences shorter than a slab)
        p0 -= d.B.P0;
        kb += wrapjump;
      }
    } else {
      kb += BK * rowB;
    }
  };
  auto lstore = [&](int bufoff, const u32x4 (&la)[4], const u32x4 (&lb)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      *reinterpret_cast<u32x4*>(wA + bufoff + q * 8 * 128) = la[q];
      *reinterpret_cast<u32x4*>(wB + bufoff + q * 8 * 128) = lb[q];
    }
  };
  // Fragments: single floats at (k pair s2, sub-tile i) = base + (s2 * 256 + i * 32) floats.  Written
  // as plain loads the compiler pairs them into ds_read2_b32, whose 8-bit offsets cannot span the
  // 1 KB row pitch: it then spends one address VALU per read inside the K loop -- next to fp32 MFMAs
  // that is the expensive kind of instruction.  ds_read_b32 takes a 16-bit immediate: one base VGPR
  // per operand and immediates for everything else (asm), waits by hand, one k pair ahead.
  unsigned aA = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const float*)(rA);
  unsigned aB = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const float*)(rB);
  auto mfma_slab = [&](auto bufc, unsigned pa, unsigned pb) {
    constexpr int bufoff = decltype(bufc)::value;
    float a[2][2], b[2][2];
    auto rd = [](auto s2c, float (&av)[2], float (&bv)[2], unsigned qa, unsigned qb) {
      constexpr int o = (bufoff + decltype(s2c)::value * 256) * 4;
      asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(av[0]) : "v"(qa), "n"(o));
      asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(av[1]) : "v"(qa), "n"(o + 128));
      asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(bv[0]) : "v"(qb), "n"(o));
      asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(bv[1]) : "v"(qb), "n"(o + 128));
    };
    auto mm = [&](const float (&av)[2], const float (&bv)[2]) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
    };
    rd(std::integral_constant<int, 0>{}, a[0], b[0], pa, pb);
    auto pair = [&](auto s2c) {
      constexpr int s2 = decltype(s2c)::value;
      constexpr int cu = s2 & 1, nx = cu ^ 1;
      if constexpr (s2 + 1 < 16) {
        rd(std::integral_constant<int, s2 + 1>{}, a[nx], b[nx], pa, pb);
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(a[cu][0]), "+v"(a[cu][1]), "+v"(b[cu][0]), "+v"(b[cu][1]));
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[cu][0]), "+v"(a[cu][1]), "+v"(b[cu][0]), "+v"(b[cu][1]));
      }
      mm(a[cu], b[cu]);
    };
    pair(std::integral_constant<int, 0>{});
    pair(std::integral_constant<int, 1>{});
    pair(std::integral_constant<int, 2>{});
    pair(std::integral_constant<int, 3>{});
    pair(std::integral_constant<int, 4>{});
    pair(std::integral_constant<int, 5>{});
    pair(std::integral_constant<int, 6>{});
    pair(std::integral_constant<int, 7>{});
    pair(std::integral_constant<int, 8>{});
    pair(std::integral_constant<int, 9>{});
    pair(std::integral_constant<int, 10>{});
    pair(std::integral_constant<int, 11>{});
    pair(std::integral_constant<int, 12>{});
    pair(std::integral_constant<int, 13>{});
    pair(std::integral_constant<int, 14>{});
    pair(std::integral_constant<int, 15>{});
  };
  constexpr int BUFF = 2 * TP;
  {
    u32x4 la[4], lb[4];
    gload(ka, kb, p0, la, lb);
    lstore(0, la, lb);
  }
  __syncthreads();
  auto step = [&](int t, auto curc, int nxtoff) {
    u32x4 la[4], lb[4];
    advance();
    const bool again = t + 1 < nt;   // the last iteration re-reads the first slab (never used)
    gload(again ? ka : ka0, again ? kb : kb_first, again ? p0 : p_first, la, lb);
    __builtin_amdgcn_sched_barrier(0);
    mfma_slab(curc, aA, aB);
    __builtin_amdgcn_sched_barrier(0);
    lstore(nxtoff, la, lb);
    __syncthreads();
  };
  int t = 0;
  for (; t + 1 < nt; t += 2) {
    step(t, std::integral_constant<int, 0>{}, BUFF);
    step(t + 1, std::integral_constant<int, BUFF>{}, 0);
  }
  if (t < nt) step(t, std::integral_constant<int, 0>{}, BUFF);
  gemm_epilogue<2, 2>(d.E, acc, M, N, m0, n0, wm, wn, li, h, blockIdx.z == 0);
}

}  // namespace

// form 2 on the kernels above: split-bf16 with both operands pre-split, whole 128 x 128 tiles,
// A a plain matrix, B plain or an `unbounded` single-segment 1-D window
bool f2g_leanw_ok(const f2g_gemm_desc& d) {
  const f2g_operand& A = d.A;
  const f2g_operand& B = d.B;
  if (d.form != 2 || A.rows != B.rows || A.rows <= 0) return false;
  if (!host_plain(A) || A.alpha || B.alpha || B.reflect || B.lrelu_src) return false;
  if (A.cols % 128 || B.cols % 128 || !al16(A.base) || !al16(B.base)) return false;
  if ((A.seq_stride & 3) || (B.seq_stride & 3)) return false;
  if ((long long)A.rows * A.seq_stride * 4 >= 0x7ff00000ll) return false;
  if (host_plain(B)) return (long long)B.rows * B.seq_stride * 4 < 0x7ff00000ll;
  if (!B.unbounded || B.P1 != 1 || B.P0 < 1 || B.rows % B.P0 || B.seglen < B.cols) return false;
  if ((((long long)B.step0 * B.unit) & 3) || (((long long)B.pad0 * B.unit) & 3)) return false;
  return (long long)(B.rows / B.P0) * B.seq_stride * 4 < 0x7ff00000ll;
}

// exact fp32 weight gradient (form 2, both operands fp32): the K-major lean kernel where its shape conditions
// hold and every block walks a long reduction (>= 4096 rows: the MPD weight gradients, 115 -> 125-131
// TFLOP/s, step 254.5 -> 252.6 ms; on the generator's 6016-row weight gradients the generic kernel's 8 waves
// hide the short K loops better: 92 vs 83).  option lean_wgrad: 0 off, 1 auto (default), 2 always.  ONE rule for
// f2g_gemm's dispatch and for the host's query (f2g_gemm_wgrad_lean).
bool f2g_leanw_fp32_takes(const f2g_gemm_desc& d, int split) {
  const int leanw_mode = f2g_opt(F2G_OPT_LEAN_WGRAD);
  if (d.form != 2 || d.A.split || d.B.split || split < 1) return false;
  // (its scalar row walk assumes that a slab crosses at most two sequence ends)
  return leanw_mode > 0 && d.precision == 0 && d.E.atomic && f2g_leanw_ok(d) &&
         (host_plain(d.B) || d.B.P0 >= 16) && (leanw_mode > 1 || d.A.rows / split >= 4096);
}

// The launcher of all three kernels: KPLAIN / KWIN are a kernel's BWIN = false / true instances (B a plain matrix /
// a window operand), `plain_name` / `win_name` what f2g_gemm_last_kernel reports for them.
template <auto KPLAIN, auto KWIN, int SMEM, int PATH>
static int launch_leanw(const f2g_gemm_desc& d, const char* plain_name, const char* win_name, int split,
                        hipStream_t st) {
  const int M = d.A.cols, N = d.B.cols, K = d.A.rows;
  int kchunk = ((K + split - 1) / split + BK - 1) / BK * BK;
  const int zs = (K + kchunk - 1) / kchunk;
  dim3 grid(M / 128, N / 128, zs);
  dyn_lds_once<KPLAIN, KWIN>(SMEM);
  const bool plain = host_plain(d.B);
  f2g_note_kernel(plain ? plain_name : win_name, split, PATH);
  hipLaunchKernelGGL(plain ? KPLAIN : KWIN, grid, dim3(256), SMEM, st, d, M, N, K, kchunk);
  return f2g_check_launch();
}

int f2g_launch_leanw(const f2g_gemm_desc& d, int pieces, int split, hipStream_t st) {
  if (pieces == 1)     // [buf][A tile | B tile] of 32 x 128 floats
    return launch_leanw<gemm_leanw_kernel<false>, gemm_leanw_kernel<true>, 2 * 2 * 32 * 128 * 4, 1>(
        d, "leanw<bwin=0>", "leanw<bwin=1>", split, st);
  if (pieces == 3)     // [buf][A hi | A lo | B hi | B lo] planes of 32 rows x 128 bf16
    return launch_leanw<gemm_leanw3_kernel<false>, gemm_leanw3_kernel<true>, 2 * 4 * 32 * 256, 1>(
        d, "leanw3<bwin=0>", "leanw3<bwin=1>", split, st);
  if (f2g_leanw6t_ok(d, split))       // all taps of a stride-1 layer from one staged window (gemm_x6p.hip)
    return f2g_launch_leanw6t(d, split, st);
  return launch_leanw<gemm_leanw6_kernel<false>, gemm_leanw6_kernel<true>, 6 * 32 * 256, 4>(
      d, "leanw6<bwin=0>", "leanw6<bwin=1>", split, st);
}

// 1 if f2g_gemm would run this form-2 descriptor (exact fp32, E.atomic, split_k as set) on the K-major lean
// weight-gradient kernel -- two blocks per CU, so the host deals its blocks in rounds of 512 (ops.split_for)
extern "C" int f2g_gemm_wgrad_lean(const f2g_gemm_desc* dp) {
  if (!dp || !dp->A.base || !dp->B.base) return 0;
  return f2g_leanw_fp32_takes(*dp, dp->split_k < 1 ? 1 : dp->split_k) ? 1 : 0;
}
