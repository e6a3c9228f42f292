// fp16x3: fp32-class products from TWO scaled fp16 pieces per operand, three MFMAs per product (gemm.hip has the
// family, gemm_common.h what the GEMM files share).  f2g_split_f16x2 writes the operand images, gemm_h3_kernel reads them;
// f2g_split_f16x2_cols writes the images of K-major operands (one scale per column), gemm_h3w_kernel reads those.
// The other fp16x3 kernels have a file each (gemm_f16*.hip); all share gemm_f16_common.h, the image writers
// split_f16.h, the ok functions gemm_f16_checks.h.  h3_table below lists every kernel of the family and says which one
// a descriptor belongs to.
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "gemm_f16_checks.h"
#include "gemm_f16_common.h"
#include "split_f16.h"

namespace {

// One wave per row, four rows per block and pass (split_f16.h has the routine and the arithmetic)
__global__ __launch_bounds__(256) void split_f16x2_kernel(float* dst, float* rscale, const float* src, long long ld,
                                                          int rows, int K) {
  f2g_split_f16x2_rows<true>(dst, rscale, src, ld, rows, K, (long long)blockIdx.x * 4 + (threadIdx.x >> 6),
                       (long long)gridDim.x * 4);
}

// ---- the column image (K-major operands: the reduction of a weight gradient walks ROWS, so a scale that leaves
// the sum is one per column) --------------------------------------------------------------------------------------
// Both kernels: thread = (16-byte chunk blockIdx.x * 32 + (tid & 31) of a row, row blockIdx.y * 8 + (tid >> 5) and
// every gridDim.y * 8 rows from there): 32 threads read 512 contiguous bytes of a row.
// First pass: the columns' largest sign-less bit patterns -- per thread over its rows, per block through LDS, across
// blocks by atomicMax into `work` (zeroed before; a maximum does not depend on the order: the image is reproducible).
__global__ __launch_bounds__(256) void cols_amax_kernel(unsigned* work, const float* src, long long ld, int rows,
                                                        int cols) {
  __shared__ uint4 part[8][32];
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5, c0 = (blockIdx.x * 32 + cl) * 4;
  const long long step = (long long)gridDim.y * 8;
  unsigned m[4] = {0u, 0u, 0u, 0u};
  if (c0 < cols) {
    const float* p = src + c0;
#pragma unroll 4
    for (long long r = (long long)blockIdx.y * 8 + rl; r < rows; r += step) {
      const float4 v = *reinterpret_cast<const float4*>(p + r * ld);
      const unsigned a[4] = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
#pragma unroll
      for (int j = 0; j < 4; ++j) m[j] = m[j] > (a[j] & 0x7fffffffu) ? m[j] : (a[j] & 0x7fffffffu);
    }
  }
  part[rl][cl] = make_uint4(m[0], m[1], m[2], m[3]);
  __syncthreads();
  if (rl != 0 || c0 >= cols) return;
#pragma unroll
  for (int q = 1; q < 8; ++q) {
    const uint4 t = part[q][cl];
    m[0] = m[0] > t.x ? m[0] : t.x;
    m[1] = m[1] > t.y ? m[1] : t.y;
    m[2] = m[2] > t.z ? m[2] : t.z;
    m[3] = m[3] > t.w ? m[3] : t.w;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (m[j]) atomicMax(work + c0 + j, m[j]);
}

// Second pass: every thread scales and splits its chunks (split_f16.h: the row image's arithmetic with the scale of
// each element's column) -- the same 16 bytes at the same offset, so dst may be src; rscale[c] = 1 / s.
__global__ __launch_bounds__(256) void cols_split_kernel(float* dst, float* rscale, const unsigned* work,
                                                         const float* src, long long ld, int rows, int cols) {
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5, c0 = (blockIdx.x * 32 + cl) * 4;
  if (c0 >= cols) return;
  const long long step = (long long)gridDim.y * 8;
  float s[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float rs;
    f2g_f16_scales(work[c0 + j], s[j], rs);
    if (blockIdx.y == 0 && rl == 0) rscale[c0 + j] = rs;
  }
  const float4 s4 = make_float4(s[0], s[1], s[2], s[3]);
  // four rows at a time: all loads before the first store (dst may be src, which the compiler must assume anyway)
  for (long long r = (long long)blockIdx.y * 8 + rl; r < rows; r += 4 * step) {
    float4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (r + q * step < rows) v[q] = *reinterpret_cast<const float4*>(src + (r + q * step) * ld + c0);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (r + q * step < rows) *reinterpret_cast<uint4*>(dst + (r + q * step) * ld + c0) = f2g_f16_split4(v[q], s4);
  }
}

// ---- the GEMM -----------------------------------------------------------------------------------------------------
// The structure of the lean kernel's split-bf16 instance (gemm_lean.hip, PM == 1) on 128 x 128 tiles with four waves:
// raw buffer loads (rows past the end carry an out-of-range offset and read as zeros), no vector ALU instruction in
// the K loop, a staged 16-byte chunk goes to LDS as two 8-byte halves (row = [hi k0..31 | lo k0..31 | pad], 144-byte
// pitch), fragments are ds_read_b128 of eight consecutive k, the slab after next is requested before the MFMA phase
// and the next one is written to LDS behind the first MFMAs.  What differs: the f16 MFMA, TWO accumulator sets (hi hi
// apart from the cross terms, which carry the factor 2^-11), one fragment set per 16-k step instead of two (the
// second accumulator set takes the registers), and the epilogue: the bias cannot ride in the accumulators, so the
// rescaled value goes through the generic epilogue (gemm_common.h) whatever the descriptor asks for.
__global__ __launch_bounds__(256, 2) void gemm_h3_kernel(const f2g_gemm_desc d, int M, int N, int K) {
  constexpr int BM = 128, BN = 128, TSZ = 128 * LDR;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, h = lane >> 5;
  // staged row of this thread (of 32, repeated four times 32 rows apart): rows r and r + 4 share no LDS bank
  const int ch = tid & 7;
  const int rr = ((tid >> 4) & 3) + 8 * (tid >> 6) + 4 * ((tid >> 3) & 1);
  int m0, n0;
  tile_of_block(BM, BN, m0, n0);
  __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)d.A.base, 0, 0x80000000u, 0x00020000);
  // B's resource ends with its last row: the rows of a partial last tile are out of range = zeros
  __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
      (void*)d.B.base, 0, (unsigned)((long long)N * d.B.seq_stride * 4), 0x00020000);
  const int qstepB = (int)(32 * d.B.seq_stride * 4);
  unsigned offA[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = m0 + rr + 32 * q;
    offA[q] = r < M ? (unsigned)((long long)r * d.A.seq_stride * 4) + ch * 16 : 0x80000000u;
  }
  const unsigned offB = (unsigned)((long long)(n0 + rr) * d.B.seq_stride * 4) + ch * 16;
  float* wA = smem + rr * LDR + ch * 2;
  float* wB = smem + 2 * TSZ + rr * LDR + ch * 2;
  const float* rA = smem + (wm * 64 + li) * LDR + h * 4;
  const float* rB = smem + 2 * TSZ + (wn * 64 + li) * LDR + h * 4;
  const int nt = K / BK;

  f32x16 acc[2][2], acx[2][2];
  h3_zero<4>(acc[0], acx[0]);

  auto gload = [&](int so, u32x4 (&la)[4], u32x4 (&lb)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      la[q] = __builtin_amdgcn_raw_buffer_load_b128(ra, offA[q], so, 0);
      lb[q] = __builtin_amdgcn_raw_buffer_load_b128(rb, offB, so + q * qstepB, 0);
    }
  };
  auto lstore = [&](int bufoff, const u32x4 (&la)[4], const u32x4 (&lb)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      *reinterpret_cast<u32x2*>(wA + bufoff + q * 32 * LDR) = u32x2{la[q].x, la[q].y};
      *reinterpret_cast<u32x2*>(wA + bufoff + q * 32 * LDR + 16) = u32x2{la[q].z, la[q].w};
      *reinterpret_cast<u32x2*>(wB + bufoff + q * 32 * LDR) = u32x2{lb[q].x, lb[q].y};
      *reinterpret_cast<u32x2*>(wB + bufoff + q * 32 * LDR + 16) = u32x2{lb[q].z, lb[q].w};
    }
  };
  // fragments of 16-k step ks: [0..1] = hi of the two sub-tiles, [2..3] = lo
  auto frags = [&](int off, int ks, f16x8 (&fa)[4], f16x8 (&fb)[4]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      fa[i] = *reinterpret_cast<const f16x8*>(rA + off + i * 32 * LDR + ks * 8);
      fb[i] = *reinterpret_cast<const f16x8*>(rB + off + i * 32 * LDR + ks * 8);
      fa[2 + i] = *reinterpret_cast<const f16x8*>(rA + off + i * 32 * LDR + ks * 8 + 16);
      fb[2 + i] = *reinterpret_cast<const f16x8*>(rB + off + i * 32 * LDR + ks * 8 + 16);
    }
  };
  // two register stages: slab t's MFMAs run while slab t + 1 (in registers since the previous step) goes to LDS and
  // the loads of slab t + 2 fly
  u32x4 xa[4], xb[4], ya[4], yb[4];
  gload(0, xa, xb);
  lstore(0, xa, xb);
  gload(nt > 1 ? BK * 4 : 0, xa, xb);
  __syncthreads();
  auto step = [&](int t, int curoff, int nxtoff, const u32x4 (&wa)[4], const u32x4 (&wb)[4], u32x4 (&la)[4],
                  u32x4 (&lb)[4]) {
    f16x8 fa[4], fb[4];
    gload(t + 2 < nt ? (t + 2) * BK * 4 : 0, la, lb);      // past the end: the first slab again (never used)
    frags(curoff, 0, fa, fb);
    h3_mfma12(acc, acx, fa, fa + 2, fb, fb + 2);
    lstore(nxtoff, wa, wb);
    frags(curoff, 1, fa, fb);
    h3_mfma12(acc, acx, fa, fa + 2, fb, fb + 2);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
  };
  int t = 0;
  for (; t + 1 < nt; t += 2) {
    step(t, 0, TSZ, xa, xb, ya, yb);
    step(t + 1, TSZ, 0, ya, yb, xa, xb);
  }
  if (t < nt) step(t, 0, TSZ, xa, xb, ya, yb);

  // v = (acc0 + 2^-11 acc1) / s_a[row] / s_b[col] (gemm_f16_common.h: h3_value), then the generic epilogue on v
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int col = n0 + (wn * 2 + ni) * 32 + li;
    const float sb = col < N ? d.B.rscale[col] : 0.f;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + (wm * 2 + mi) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        const float sa = row < M ? d.A.rscale[row] : 0.f;
        acc[mi][ni][e] = h3_value(acc[mi][ni][e], acx[mi][ni][e], sa, sb);
      }
  }
  gemm_epilogue<2, 2>(d.E, acc, M, N, m0, n0, wm, wn, li, h, true);
}

// ---- the weight gradient: C[m,n] (+)= sum_r A[r,m] B[r,n] over f2g_split_f16x2_cols images ----------------------
// gemm_leanw3_kernel<false>'s structure (gemm_wgrad.hip has the layout): buffer loads with the K advance in a scalar
// register (rows past the last one lie behind the resource = zeros; so do the chunks of a partial tile's columns
// past M / N, whose offsets carry bit 31), the 16-byte chunks stored as they lie in memory into hi and lo planes of
// 32 rows x 128 halves with the (row & 3) swizzle, fragments through the transposing ds_read_b64_tr_b16, no vector
// ALU instruction in the K loop.  What differs is what differs between gemm_h3_kernel and the lean kernel: the f16
// MFMA, two accumulator sets, ONE fragment set per 16-k step (the second accumulator set takes the registers of
// leanw3's prefetched one), and the rescale by the reciprocal COLUMN scales of both operands before the generic
// epilogue.  The rescale is linear, so the partial tiles of a K split are rescaled and then added atomically.
__global__ __launch_bounds__(256, 2) void gemm_h3w_kernel(const f2g_gemm_desc d, int M, int N, int K, int kchunk) {
  constexpr int PL = 32 * 256;            // bytes of one plane (32 rows x 128 halves)
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
  __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
      (void*)d.B.base, 0, (unsigned)((long long)K * d.B.seq_stride * 4), 0x00020000);
  // (M % 4 == 0 and N % 4 == 0: a chunk lies inside the matrix or outside it)
  const unsigned pastA = m0 + 4 * c < M ? 0u : 0x80000000u, pastB = n0 + 4 * c < N ? 0u : 0x80000000u;
  unsigned offA[4], offB[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    offA[q] = (unsigned)(((long long)(rid + 8 * q) * d.A.seq_stride + m0 + 4 * c) * 4) | pastA;
    offB[q] = (unsigned)(((long long)(rid + 8 * q) * d.B.seq_stride + n0 + 4 * c) * 4) | pastB;
  }
  const int stepA = (int)(BK * d.A.seq_stride * 4), stepB = (int)(BK * d.B.seq_stride * 4);
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

  f32x16 acc[2][2], acx[2][2];
  h3_zero<4>(acc[0], acx[0]);

  int ka = (int)((long long)kbeg * d.A.seq_stride * 4), kb = (int)((long long)kbeg * d.B.seq_stride * 4);
  const int ka0 = ka, kb0 = kb;
  auto gload = [&](bool valid, u32x4 (&la)[4], u32x4 (&lb)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      la[q] = __builtin_amdgcn_raw_buffer_load_b128(ra, offA[q], valid ? ka : ka0, 0);
      lb[q] = __builtin_amdgcn_raw_buffer_load_b128(rb, offB[q], valid ? kb : kb0, 0);
    }
  };
  auto advance = [&]() {
    ka += stepA;
    kb += stepB;
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
  // fragments of 16-k step ks: [0..1] = hi of the two sub-tiles, [2..3] = lo
  auto frags = [&](int bufoff, int ks, f16x8 (&fa)[4], f16x8 (&fb)[4]) {
    const unsigned char* base = sm + bufoff + ks * 16 * 256;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      fa[t] = tr_frag_f16<256>(base + rofA[t]);
      fa[2 + t] = tr_frag_f16<256>(base + PL + rofA[t]);
      fb[t] = tr_frag_f16<256>(base + 2 * PL + rofB[t]);
      fb[2 + t] = tr_frag_f16<256>(base + 3 * PL + rofB[t]);
    }
  };
  // two register stages: slab t's MFMAs run while slab t + 1 (in registers since the previous step) goes to LDS and
  // the loads of slab t + 2 fly
  u32x4 xa[4], xb[4], ya[4], yb[4];
  gload(true, xa, xb);
  lstore(0, xa, xb);
  advance();
  gload(nt > 1, xa, xb);
  __syncthreads();
  auto step = [&](int t, int curoff, int nxtoff, const u32x4 (&wa)[4], const u32x4 (&wb)[4], u32x4 (&la)[4],
                  u32x4 (&lb)[4]) {
    f16x8 fa[4], fb[4];
    advance();
    gload(t + 2 < nt, la, lb);      // past the end: the first slab again (never used)
    frags(curoff, 0, fa, fb);
    // (the loads stay in front: left to itself the scheduler sinks them behind the LDS stores, to the barrier, and
    // the next step waits for them at once)
    __builtin_amdgcn_sched_barrier(0);
    h3_mfma12(acc, acx, fa, fa + 2, fb, fb + 2);
    lstore(nxtoff, wa, wb);
    __builtin_amdgcn_sched_barrier(0);
    frags(curoff, 1, fa, fb);
    h3_mfma12(acc, acx, fa, fa + 2, fb, fb + 2);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
  };
  int t = 0;
  for (; t + 1 < nt; t += 2) {
    step(t, 0, BUF, xa, xb, ya, yb);
    step(t + 1, BUF, 0, ya, yb, xa, xb);
  }
  if (t < nt) step(t, 0, BUF, xa, xb, ya, yb);

  // v = (acc0 + 2^-11 acc1) / s_a[m] / s_b[n] (gemm_f16_common.h: h3_value), then the generic epilogue (a row's
  // scale is loaded once for both column sub-tiles)
  float sb[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int col = n0 + (wn * 2 + ni) * 32 + li;
    sb[ni] = col < N ? d.B.rscale[col] : 0.f;
  }
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = m0 + (wm * 2 + mi) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      const float sa = row < M ? d.A.rscale[row] : 0.f;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) acc[mi][ni][e] = h3_value(acc[mi][ni][e], acx[mi][ni][e], sa, sb[ni]);
    }
  gemm_epilogue<2, 2>(d.E, acc, M, N, m0, n0, wm, wn, li, h, blockIdx.z == 0);
}

inline bool h3_operand_ok(const f2g_operand& S) {
  return host_plain(S) && !S.alpha && S.rows > 0 && S.cols >= BK && S.cols % BK == 0 && S.cols <= F2G_F16_MAX_K &&
         al16(S.base) && (S.seq_stride & 3) == 0 && S.seq_stride >= S.cols &&
         h3_fits31((long long)S.rows * S.seq_stride);
}

// gemm_h3_kernel, and gemm_h3n_kernel (gemm_f16n.hip) where A is marked split = 9 -- the fp32 matrix itself, scaled
// per row tile inside the kernel: the same conditions, A without rscale, and the answer follows B alone
int h3_plain_ok(const f2g_gemm_desc& d) {
  if (d.A.cols != d.B.cols || !h3_operand_ok(d.A) || !h3_operand_ok(d.B)) return 0;
  if (d.A.split == 9 && d.A.rscale) return 0;
  const f2g_epilogue& E = d.E;
  if (d.split_k > 1 || E.x3_out || E.colsum_part_ld > 0 || E.c_bf16) return 0;
  // (the combinations f2g_gemm refuses for every kernel)
  if (E.prelu_slope && (E.atomic || E.accumulate || E.P0o > 0)) return 0;
  if (E.mask_src && (E.atomic || E.accumulate)) return 0;
  if (E.aux && !E.alpha_n) return 0;
  return d.A.split == 9 ? f16_b_image_status(d.B, 5) : f16_images_status(d.A, d.B, 5);
}

int h3w_ok(const f2g_gemm_desc& d) {
  if (d.precision != 4 || d.A.rows != d.B.rows || !h3w_operand_ok(d.A) || !h3w_operand_ok(d.B)) return 0;
  const f2g_epilogue& E = d.E;
  if (E.x3_out || E.colsum_part_ld > 0 || E.c_bf16 || (d.split_k > 1 && !E.atomic)) return 0;
  // (the combinations f2g_gemm refuses for every form-2 kernel)
  if (E.prelu_slope || E.mask_src || (E.aux && !E.alpha_n)) return 0;
  return f16_images_status(d.A, d.B, 6);
}

int f2g_launch_h3(const f2g_gemm_desc& d, hipStream_t st) {
  const int M = d.A.rows, N = d.B.rows, K = d.A.cols;
  constexpr int smem = 4 * 128 * LDR * 4;
  dyn_lds_once<gemm_h3_kernel>(smem);
  f2g_note_kernel("h3<ep=all>", 1, 6);
  hipLaunchKernelGGL(gemm_h3_kernel, dim3((M + 127) / 128, (N + 127) / 128), dim3(256), smem, st, d, M, N, K);
  return f2g_check_launch();
}

int f2g_launch_h3w(const f2g_gemm_desc& d, hipStream_t st) {
  const int M = d.A.cols, N = d.B.cols, K = d.A.rows, split = d.split_k > 1 ? d.split_k : 1;
  const int kchunk = ((K + split - 1) / split + BK - 1) / BK * BK;
  constexpr int smem = 2 * 4 * 32 * 256;      // [buf][A hi | A lo | B hi | B lo] planes of 32 rows x 128 halves
  dyn_lds_once<gemm_h3w_kernel>(smem);
  f2g_note_kernel("h3w", split, 6);
  hipLaunchKernelGGL(gemm_h3w_kernel, dim3((M + 127) / 128, (N + 127) / 128, (K + kchunk - 1) / kchunk),
                     dim3(256), smem, st, d, M, N, K, kchunk);
  return f2g_check_launch();
}

// ---- the ONE route decision of precision 4 -------------------------------------------------------------------------
// The fp16x3 kernels, one entry each.  h3_route_of walks the table in order: the FIRST entry whose `claims` holds -- a
// test of the descriptor's form, marks and operand shapes alone -- is the descriptor's candidate, and that kernel's own
// conditions (`ok`) decide.  Nothing else is asked: a descriptor one kernel declines is never offered to another.  So
// the order is part of the rule -- the epilogue fields only one kernel knows (E.col_fold / E.seq_live) in front of
// everything, the marked operands (split = 8 / 9 / 10: fp32, scaled inside the kernel) in front of the shapes, a windows' stride 3 in front of "any stride", the plain kernels of each form last.
// `ok` answers f2g_gemm_f16_ok: 0 = not for this kernel, 1 = runs as handed over (the operands the kernel's images
// with their reciprocal scales, or marked fp32), 2 = once the fp32 operands are replaced by those images.
// `part_tile`: the tile height the kernel's wide epilogue counts partial column sums in, one row per 64 output rows of
// whole tiles (f2g_gemm_colsum_part_rows); 0 = no wide epilogue.  `what`: the descriptors it takes, for F2G_EINVAL.
struct h3_entry {
  bool (*claims)(const f2g_gemm_desc& d);
  int (*ok)(const f2g_gemm_desc& d);
  int (*launch)(const f2g_gemm_desc& d, hipStream_t st);
  int part_tile;
  const char* what;
};

inline bool h3_form2_p4(const f2g_gemm_desc& d) { return d.form == 2 && d.precision == 4; }
inline bool h3_tapw_shape(const f2g_gemm_desc& d) { return h3_form2_p4(d) && host_plain(d.A) && !host_plain(d.B); }

const h3_entry h3_table[] = {
    // H3_TAPN3, gemm_h3pn3_kernel (gemm_f16pn3.hip).  It stands first and claims every descriptor that sets E.col_fold
    // or E.seq_live, whatever its form and marks: no other kernel knows the two fields, so what this one declines is
    // F2G_EINVAL and never reaches H3_TAPN or any entry below with the fields ignored
    {[](const f2g_gemm_desc& d) { return d.E.col_fold != 0 || d.E.seq_live != 0; }, f2g_h3pn3_ok, f2g_launch_h3pn3, 0,
     "form 0 over the fp32 map (A.split = 8) under stride-1 windows of 2 positions over 128 channels onto 96 columns, "
     "three rows of a 32-channel map side by side (E.col_fold = 32, E.seq_live), against a f2g_split_f16x2_seq image"},
    // H3_TAPW3N, gemm_h3wsn_kernel (gemm_f16wsn.hip)
    {[](const f2g_gemm_desc& d) { return h3_form2_p4(d) && (d.A.split == 8 || d.B.split == 8); }, f2g_h3wsn_ok,
     f2g_launch_h3wsn, 0,
     "form 2 + atomic over a plain fp32 matrix of 128 columns and the fp32 map under unbounded stride-3 windows of 5 "
     "positions over 32 channels, both marked split = 8 without rscale"},
    // H3_WGRADN, gemm_h3wn_kernel (gemm_f16wn.hip): BOTH marks (split = 10; 9 is H3_PLAINN's mark on A at form 0 and
    // keeps answering 0 at form 2); a descriptor with one operand marked stays with H3_WGRAD below, which declines it
    {[](const f2g_gemm_desc& d) { return h3_form2_p4(d) && d.A.split == 10 && d.B.split == 10; }, f2g_h3wn_ok,
     f2g_launch_h3wn, 0,
     "form 2 over two plain fp32 matrices themselves, both marked split = 10 without rscale"},
    // H3_TAPW3, gemm_h3ws_kernel (gemm_f16ws.hip)
    {[](const f2g_gemm_desc& d) { return h3_tapw_shape(d) && d.B.step0 == 3; }, f2g_h3ws_ok, f2g_launch_h3ws, 0,
     "form 2 + atomic over f2g_split_f16x2_cols images of a plain matrix and of the map under unbounded stride-3 "
     "windows of 5 positions that overhang a sequence of seq_stride / unit map rows by at most pad0 rows"},
    // H3_TAPW, gemm_h3wt_kernel (gemm_f16wt.hip)
    {h3_tapw_shape, f2g_h3wt_ok, f2g_launch_h3wt, 0,
     "form 2 + atomic over such images under unbounded stride-1 windows of 5 positions"},
    // H3_WGRAD, gemm_h3w_kernel
    {[](const f2g_gemm_desc& d) { return d.form == 2; }, h3w_ok, f2g_launch_h3w, 0,
     "form 2 over f2g_split_f16x2_cols images of two plain matrices"},
    // H3_PLAINN, gemm_h3n_kernel (gemm_f16n.hip); h3_plain_ok declines a window operand so marked
    {[](const f2g_gemm_desc& d) { return d.form == 0 && d.A.split == 9; }, h3_plain_ok, f2g_launch_h3n, 0,
     "form 0 over the plain fp32 matrix A itself (A.split = 9 without rscale) against B's f2g_split_f16x2 image"},
    // H3_TAP3N, gemm_h3p3n_kernel (gemm_f16p3n.hip)
    {[](const f2g_gemm_desc& d) { return d.form == 0 && d.A.split == 8 && d.A.step0 == 3; }, f2g_h3p3n_ok,
     f2g_launch_h3p3n, 128,
     "form 0 over the fp32 map (A.split = 8) under stride-3 windows of 5 positions over 32 channels against a "
     "f2g_split_f16x2_seq image"},
    // H3_TAPN, gemm_h3pn_kernel (gemm_f16pn.hip): the thin epilogue
    {[](const f2g_gemm_desc& d) { return d.form == 0 && d.A.split == 8; }, f2g_h3pn_ok, f2g_launch_h3pn, 0,
     "form 0 over the fp32 map (A.split = 8) under stride-1 windows of 2 or 1 positions over 128 channels onto at "
     "most 32 columns against a f2g_split_f16x2_seq image"},
    // H3_TAP3, gemm_h3p3_kernel (gemm_f16p3.hip)
    {[](const f2g_gemm_desc& d) { return d.form == 0 && !host_plain(d.A) && d.A.step0 == 3; }, f2g_h3p3_ok,
     f2g_launch_h3p3, 256,
     "form 0 over f2g_split_f16x2_seq images of stride-3 windows of 5 positions over a multiple of 128 channels"},
    // H3_TAP, gemm_h3p_kernel (gemm_f16p.hip): windows of a halo map, or f2g_split_f16x2_seq images
    {[](const f2g_gemm_desc& d) { return d.form == 0 && (!host_plain(d.A) || d.A.split == 7 || d.B.split == 7); },
     f2g_h3p_ok, f2g_launch_h3p, 256,
     "form 0 over f2g_split_f16x2_seq images of stride-1 windows of 5 or 2 positions"},
    // H3_PLAIN, gemm_h3_kernel
    {[](const f2g_gemm_desc& d) { return d.form == 0; }, h3_plain_ok, f2g_launch_h3, 0,
     "form 0 over f2g_split_f16x2 images of two plain matrices"},
};

struct h3_route {
  const h3_entry* entry = nullptr;      // set where status != 0
  int status = 0;
};

h3_route h3_route_of(const f2g_gemm_desc& d) {
  h3_route r;
  if (!d.A.base || !d.B.base || !d.E.C) return r;
  for (const h3_entry& e : h3_table)
    if (e.claims(d)) {
      r.status = e.ok(d);
      if (r.status) r.entry = &e;
      break;
    }
  return r;
}

}  // namespace

extern "C" int f2g_gemm_f16_ok(const f2g_gemm_desc* dp) { return dp ? h3_route_of(*dp).status : 0; }

int f2g_gemm_h3_part_tile(const f2g_gemm_desc& d) {
  const h3_route r = h3_route_of(d);
  return r.entry ? r.entry->part_tile : 0;
}

int f2g_gemm_h3(const f2g_gemm_desc& d, hipStream_t st) {
  const h3_route r = h3_route_of(d);
  if (r.status == 1) return r.entry->launch(d, st);
  std::string msg = "f2g_gemm precision 4: f2g_gemm_f16_ok(d) != 1 for this descriptor.  The kernels take";
  for (const h3_entry& e : h3_table) msg += std::string(&e == h3_table ? " " : "; or ") + e.what;
  f2g_set_error(msg.c_str());
  return F2G_EINVAL;
}

extern "C" int f2g_split_f16x2_cols(float* dst, float* rscale, uint32_t* work, const float* src, int64_t ld,
                                    int32_t rows, int32_t cols, f2g_stream_t stream) {
  if (!dst || !rscale || !work || !src || rows < 1 || cols < 4 || (cols & 3) || ld < cols || (ld & 3) || !al16(dst) ||
      !al16(src))
    return F2G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const hipError_t zeroed = hipMemsetAsync(work, 0, (size_t)cols * 4, st);
  if (zeroed != hipSuccess) {
    f2g_set_error(hipGetErrorString(zeroed));
    return F2G_ELAUNCH;
  }
  const int bands = (cols + 127) / 128;
  int gy = (rows + 31) / 32, cap = 4096 / bands;
  if (cap < 1) cap = 1;
  if (gy > cap) gy = cap;
  hipLaunchKernelGGL(cols_amax_kernel, dim3(bands, gy), dim3(256), 0, st, work, src, (long long)ld, rows, cols);
  hipLaunchKernelGGL(cols_split_kernel, dim3(bands, gy), dim3(256), 0, st, dst, rscale, work, src, (long long)ld, rows,
                     cols);
  return f2g_check_launch();
}

extern "C" int f2g_split_f16x2(float* dst, float* rscale, const float* src, int64_t ld, int32_t rows, int32_t K,
                               f2g_stream_t stream) {
  if (!dst || !rscale || !src || rows < 0 || K < BK || K % BK || K > F2G_F16_MAX_K || ld < K || (ld & 3) ||
      !al16(dst) || !al16(src))
    return F2G_EINVAL;
  if (rows == 0) return F2G_OK;
  int blocks = (rows + 3) / 4;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(split_f16x2_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dst, rscale, src,
                     (long long)ld, rows, K);
  return f2g_check_launch();
}
