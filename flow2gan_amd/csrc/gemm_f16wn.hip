// fp16x3 weight gradient over the two fp32 activation matrices THEMSELVES, both scaled inside the kernel:
//   C[m, n] (+)= sum_r A[r, m] B[r, n]
// gemm_h3w_kernel (gemm_f16.hip) with both operands marked f2g_operand.split = 10 -- `base` is the caller's plain fp32
// K-major matrix, there is no f2g_split_f16x2_cols image of it and no rscale.  The two two-pass image calls of the
// image route (12 bytes of HBM traffic per element, one allocation each) are gone: the kernel reads 4 bytes per
// element, as gemm_leanw6_kernel<false> (gemm_wgrad.hip) does, and splits into two fp16 pieces where that kernel
// splits into three bf16 pieces: 24 MFMAs per wave and slab instead of 48, four LDS planes instead of six, 16
// transposing fragment reads instead of 24.
//
// THE WALK is gemm_h3w_kernel's: 128 x 128 tile, four waves (2 x 2 sub-tiles of 32 x 32 each), slabs of 32 reduction
// rows; raw buffer loads with the K advance in a scalar register -- rows past K lie behind the resource and read as
// zeros, so do the chunks of a partial tile's columns past M / N, whose offsets carry bit 31 (M % 4 == 0 and N % 4 == 0:
// a chunk lies inside the matrix or outside it) --, fragments through the transposing ds_read_b64_tr_b16, h3_mfma12 on
// two accumulator sets, a K split over blockIdx.z with f2g_launch_h3w's kchunk rule, gemm_epilogue<2, 2> with
// blockIdx.z == 0 as "first".  An image chunk and an fp32 chunk are both 16 bytes per four elements: the loads, the LDS
// layout and the fragment reads carry over unchanged, only the split moves from the image pass to the place where a
// staged chunk goes to LDS (f2g_f16_split4(v, s)).
//
// ONE MONOTONE RUNNING SCALE PER OPERAND AND BLOCK, the rule of gemm_f16wsn.hip: m_run_a and m_run_b start at 0 = scale
// 1; before slab T is split m_run = max(m_run, m_T) over the slab's floats of the tile's 128 columns that lie inside the
// matrix (the zeros substituted past K, M and N do not count), a slab whose maximum is zero or not finite leaves m_run
// alone and is split at the scale in force; (s, rs) = f2g_f16_scales(m_run).  When either scale moves, both
// accumulator sets are multiplied by the exact powers of two s_new / s_old of the two operands (a wave-uniform branch,
// not taken while the scales stand).  v = h3_value(acc, acx, rs_a, rs_b) goes through the generic epilogue; the
// rescale is linear, so the partial tiles of a K split are rescaled and then added atomically.  The maxima are integer
// maxima of sign-less bit patterns (thread, wave through h3n_wave_max, one LDS word per wave and operand,
// double-buffered by slab parity): a block's contribution is reproducible.  Per output
//   |err| <= 3 * 2^-22 sum_r |a||b| + 2^-28 sum_T (brun_T sum_{r in T} |a| + arun_T sum_{r in T} |b|)
// with the running maxima in force at slab T of the block's tile and K chunk (DESIGN section 4;
// tests/fp16x3_runk_emul.py).  Columns share their tile's scale: a column quiet against its tile sees the floor term,
// which the image route's per-column scale spares it.
//
// THE SCHEDULE, gemm_h3w_kernel's two LDS buffers and one barrier per slab.  Slab t + 1 is in registers since step
// t - 1; its maxima are reduced at the end of step t - 1 (the loads have had the step's MFMAs to land) into the eight
// LDS words of the slab's parity, and the barrier that ends step t - 1 publishes them.  Step t requests slab t + 2,
// combines the words into the scales of slab t + 1, runs slab t's first twelve MFMAs, splits slab t + 1 into the other
// buffer where lstore stands in gemm_h3w_kernel, runs the second twelve, multiplies the accumulators if a scale moved
// (slab t's products are in), and posts the maxima of slab t + 2.  A wave may post slab t + 2's words while another
// still reads slab t + 1's: hence the parity.  The prologue does the same for slabs 0 and 1 with one barrier more.  A
// slab past the block's last one posts zeros for its maxima: it moves no scale, and its split is never read -- under a K
// split it would be the next block's data.
//
// LDS: [buf 0 | buf 1 | maxima], buf = [A hi | A lo | B hi | B lo] planes of 32 rows x 128 halves = 8192 bytes each,
// the row's four 64-byte column blocks rotated by (row & 3) (gemm_wgrad.hip has the layout and why the transposing
// reads and the 8-byte stores are conflict-free); maxima = [slab parity][A, B][4 waves] words.  65600 bytes.
//
// RESOURCES (tools/kernel_resources.py, gfx950): 253 VGPRs (gemm_h3w_kernel: 246), 0 AGPRs, 0 scratch, 0 vector spills, 2
// waves per SIMD (two blocks per CU); 30 scalar registers are parked in VGPR lanes, as in gemm_h3w_kernel, behind the K
// loop in the generic epilogue.  65600 bytes of LDS (two buffers of four 8192-byte planes, 16 maxima words): two blocks
// per CU.  The per-load "is the slab past the end" selects of an earlier draft cost eight registers and one spill:
// hence a slab past the end is loaded like gemm_h3w_kernel's and its maxima are posted as zeros.
// PER WAVE AND SLAB, counted from the ISA of the loop body: 24 v_mfma_f32_32x32x16_f16, 32 ds_read_b64_tr_b16, 8
// buffer_load_dwordx4, 16 eight-byte LDS stores (8 ds_write2st64_b64) and 224 vector ALU instructions -- 147 beside the
// MFMAs (the split of 32 floats per lane: 32 v_cvt_pk_f16_f32, 32 v_cvt_f32_f16, 49 packed or scalar multiplies, 24
// fused multiply-adds; the rest addresses and the two scales) and 77 between the last MFMA and the barrier (the maxima:
// 32 v_and, 22 integer maxima, 8 DPP maxima, 8 v_readlane) -- 7 per element; the rescale branch, when a scale moves,
// adds 128 v_pk_mul_f32.  (gemm_leanw6_kernel: 48 MFMAs and 5.5 per element.)  The split is written on pairs of floats
// (h3wn_pair below) so that the packed instructions are used: with split_f16.h's scalar routine the loop has 255.
// MEASURED: tools/fp16x3_wgrad_shapes.py --noimage -> profiles/fp16x3_wgrad_noimage_shapes.txt; DESIGN.md section 0
// has the numbers and what they say.
#include <stddef.h>
#include <stdint.h>

#include "gemm_f16_checks.h"
#include "gemm_f16_common.h"
#include "split_f16.h"

namespace {

__device__ __forceinline__ float4 h3wn_f4(const u32x4 v) {
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

typedef float h3wn_f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h3wn_f16x2 __attribute__((ext_vector_type(2)));

// split_f16.h's f2g_f16_pair / f2g_f16_split4 on PAIRS of floats, so that the compiler may use the packed fp32
// instructions and the packed conversion: the same values bit for bit -- y = x s, y - hi and 2^11 (y - hi) are exact,
// the two conversions round to nearest even
__device__ __forceinline__ unsigned h3wn_pair(float x0, float x1, float s, unsigned& lo) {
  const h3wn_f32x2 y = h3wn_f32x2{x0, x1} * s;
  const h3wn_f16x2 hi = __builtin_convertvector(y, h3wn_f16x2);
  const h3wn_f32x2 r = (y - __builtin_convertvector(hi, h3wn_f32x2)) * 2048.f;
  lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r, h3wn_f16x2));
  return __builtin_bit_cast(unsigned, hi);
}

__device__ __forceinline__ uint4 h3wn_split4(const u32x4 v, float s) {
  const unsigned u0 = v.x, u1 = v.y, u2 = v.z, u3 = v.w;
  unsigned l01, l23;
  const unsigned h01 = h3wn_pair(__uint_as_float(u0), __uint_as_float(u1), s, l01);
  const unsigned h23 = h3wn_pair(__uint_as_float(u2), __uint_as_float(u3), s, l23);
  return make_uint4(h01, h23, l01, l23);
}

__global__ __launch_bounds__(256, 2) void gemm_h3wn_kernel(const f2g_gemm_desc d, int M, int N, int K, int kchunk) {
  constexpr int PL = 32 * 256;            // bytes of one plane (32 rows x 128 halves)
  constexpr int BUF = 4 * PL;             // [A hi | A lo | B hi | B lo]
  extern __shared__ __attribute__((aligned(16))) float smem[];
  unsigned char* sm = reinterpret_cast<unsigned char*>(smem);
  unsigned* smx = reinterpret_cast<unsigned*>(sm + 2 * BUF);      // [slab parity][A, B][4 waves]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
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

  // slab j of this block's K chunk (consecutive slabs are requested in order: the scalars advance with each call);
  // past the chunk's last slab: the chunk's first one again, whose maxima are posted as zeros (post_amax) and whose
  // split is never read
  int ka = (int)((long long)kbeg * d.A.seq_stride * 4), kb = (int)((long long)kbeg * d.B.seq_stride * 4);
  const int ka0 = ka, kb0 = kb;
  auto gload = [&](int j, u32x4 (&la)[4], u32x4 (&lb)[4]) {
    const bool on = j < nt;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      la[q] = __builtin_amdgcn_raw_buffer_load_b128(ra, offA[q], on ? ka : ka0, 0);
      lb[q] = __builtin_amdgcn_raw_buffer_load_b128(rb, offB[q], on ? kb : kb0, 0);
    }
    ka += stepA;
    kb += stepB;
  };
  // both operands' chunks are split at their scales on their way to LDS
  auto lstore = [&](int bufoff, const u32x4 (&la)[4], const u32x4 (&lb)[4], float sa, float sb) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned char* pa = sm + bufoff + wofs[q];
      const uint4 a = h3wn_split4(la[q], sa);
      *reinterpret_cast<u32x2*>(pa) = u32x2{a.x, a.y};
      *reinterpret_cast<u32x2*>(pa + PL) = u32x2{a.z, a.w};
      const uint4 b = h3wn_split4(lb[q], sb);
      *reinterpret_cast<u32x2*>(pa + 2 * PL) = u32x2{b.x, b.y};
      *reinterpret_cast<u32x2*>(pa + 3 * PL) = u32x2{b.z, b.w};
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
  // the maxima of the slab in the registers, per wave, into the words of its parity (read behind the next barrier)
  // -- zeros for a slab past the chunk's last one (under a K split it would be the next block's data): no scale moves
  auto post_amax = [&](int j, const u32x4 (&la)[4], const u32x4 (&lb)[4]) {
    const int par = j & 1;
    unsigned ma = 0, mb = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      ma = f2g_f16_amax4(h3wn_f4(la[q]), ma);
      mb = f2g_f16_amax4(h3wn_f4(lb[q]), mb);
    }
    ma = h3n_wave_max(ma);
    mb = h3n_wave_max(mb);
    if (lane == 0) smx[par * 8 + wave] = j < nt ? ma : 0u, smx[par * 8 + 4 + wave] = j < nt ? mb : 0u;
  };
  // the running scale of one operand moves on to the slab whose maxima are in m4; f = s_new / s_old
  auto next_scale = [&](const unsigned* m4, unsigned& mrun, float& s, float& rs, float& f) {
    unsigned m = m4[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) m = m > m4[w] ? m : m4[w];
    m = (unsigned)__builtin_amdgcn_readfirstlane((int)m);
    if (m != 0u && m < 0x7f800000u && m > mrun) mrun = m;   // (a zero or non-finite slab: the scale in force)
    float sn, rsn;
    f2g_f16_scales(mrun, sn, rsn);
    f = sn * rs;
    s = sn;
    rs = rsn;
  };

  unsigned mra = 0u, mrb = 0u;             // the running maxima; 0 = scale 1
  float sa = 1.f, rsa = 1.f, sb = 1.f, rsb = 1.f;
  // two register stages: slab t's MFMAs run while slab t + 1 (in registers since the previous step) is split into LDS
  // and the loads of slab t + 2 fly
  u32x4 xa[4], xb[4], ya[4], yb[4];
  gload(0, xa, xb);
  post_amax(0, xa, xb);
  __syncthreads();
  {
    float f;
    next_scale(smx, mra, sa, rsa, f);      // (the accumulators are zero: no rescale)
    next_scale(smx + 4, mrb, sb, rsb, f);
  }
  lstore(0, xa, xb, sa, sb);
  gload(1, xa, xb);
  post_amax(1, xa, xb);
  __syncthreads();
  auto step = [&](int t, int curoff, int nxtoff, const u32x4 (&wa)[4], const u32x4 (&wb)[4], u32x4 (&la)[4],
                  u32x4 (&lb)[4]) {
    f16x8 fa[4], fb[4];
    float fA, fB;
    gload(t + 2, la, lb);
    next_scale(smx + ((t + 1) & 1) * 8, mra, sa, rsa, fA);
    next_scale(smx + ((t + 1) & 1) * 8 + 4, mrb, sb, rsb, fB);
    frags(curoff, 0, fa, fb);
    // (the loads stay in front: left to itself the scheduler sinks them behind the LDS stores, to the barrier, and
    // the next step waits for them at once)
    __builtin_amdgcn_sched_barrier(0);
    h3_mfma12(acc, acx, fa, fa + 2, fb, fb + 2);
    lstore(nxtoff, wa, wb, sa, sb);
    __builtin_amdgcn_sched_barrier(0);
    frags(curoff, 1, fa, fb);
    h3_mfma12(acc, acx, fa, fa + 2, fb, fb + 2);
    if (fA != 1.f || fB != 1.f) {          // a scale moved: the stored sums go over to slab t + 1's
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            acc[mi][ni][e] = acc[mi][ni][e] * fA * fB;
            acx[mi][ni][e] = acx[mi][ni][e] * fA * fB;
          }
    }
    post_amax(t + 2, la, lb);             // slab t + 2 has landed under the MFMAs
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

  // v = (acc0 + 2^-11 acc1) / s_a / s_b with the block's final scales (gemm_f16_common.h: h3_value), then the generic
  // epilogue
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][ni][e] = h3_value(acc[mi][ni][e], acx[mi][ni][e], rsa, rsb);
  gemm_epilogue<2, 2>(d.E, acc, M, N, m0, n0, wm, wn, li, h, blockIdx.z == 0);
}

}  // namespace

// Form 2 at precision 4 with BOTH operands marked split = 10: neither carries an rscale (there are no images), and
// gemm_h3w_kernel's conditions (gemm_f16.hip: h3w_ok) hold -- the operands (gemm_f16_checks.h: h3w_operand_ok) and
// every epilogue condition.  1 = runs as handed over, 0 = not for this kernel (there is no 2: nothing has to be made
// first).
int f2g_h3wn_ok(const f2g_gemm_desc& d) {
  const f2g_operand& A = d.A;
  const f2g_operand& B = d.B;
  if (d.form != 2 || d.precision != 4 || A.split != 10 || B.split != 10 || A.rscale || B.rscale) return 0;
  if (A.rows != B.rows || !h3w_operand_ok(A) || !h3w_operand_ok(B)) return 0;
  const f2g_epilogue& E = d.E;
  if (E.x3_out || E.colsum_part_ld > 0 || E.c_bf16 || (d.split_k > 1 && !E.atomic)) return 0;
  // (the combinations f2g_gemm refuses for every form-2 kernel)
  if (E.prelu_slope || E.mask_src || (E.aux && !E.alpha_n)) return 0;
  return 1;
}

int f2g_launch_h3wn(const f2g_gemm_desc& d, hipStream_t st) {
  const int M = d.A.cols, N = d.B.cols, K = d.A.rows, split = d.split_k > 1 ? d.split_k : 1;
  const int kchunk = ((K + split - 1) / split + BK - 1) / BK * BK;      // (f2g_launch_h3w's rule)
  constexpr int smem = 2 * 4 * 32 * 256 + 2 * 2 * 4 * (int)sizeof(unsigned);
  dyn_lds_once<gemm_h3wn_kernel>(smem);
  f2g_note_kernel("h3wn", split, 6);
  hipLaunchKernelGGL(gemm_h3wn_kernel, dim3((M + 127) / 128, (N + 127) / 128, (K + kchunk - 1) / kchunk),
                     dim3(256), smem, st, d, M, N, K, kchunk);
  return f2g_check_launch();
}
