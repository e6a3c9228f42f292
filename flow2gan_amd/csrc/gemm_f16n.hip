// fp16x3 pointwise GEMM over the fp32 activation matrix ITSELF, scaled inside the kernel: gemm_h3_kernel (gemm_f16.hip)
// with operand A marked f2g_operand.split = 9 -- `base` is the caller's fp32 (M, K) matrix, there is no image of it and
// no rscale; operand B is still the weight's f2g_split_f16x2 image with its reciprocal row scales.  The image pass of
// the activation (f2g_split_f16x2: 10 bytes of HBM traffic per element, one allocation per call) is gone: the kernel
// reads 4 bytes per element, as gemm_x6g_kernel does.
//
// WHAT STAYS gemm_h3_kernel's: the 128 x 128 tile and four waves, the raw buffer loads (rows past M carry offset bit
// 31 and read as zeros), the 144-byte LDS pitch and the two LDS buffers, one fragment set per 16-k step, h3_mfma12 on
// two accumulator sets, the rescale and gemm_epilogue<2, 2> with every epilogue kind.  An image chunk and an fp32
// chunk are both 16 bytes per four elements: the loads, the LDS layout and the fragment reads carry over unchanged, only
// the split moves from the image pass to the place where a staged chunk goes to LDS.
//
// ONE MONOTONE RUNNING SCALE PER BLOCK for its 128-row tile of A, the rule of gemm_f16wsn.hip and conv32h3w.hip: m_run
// starts at 0 = scale 1; before slab T (32 reduction columns) is split m_run = max(m_run, m_T) over every staged float
// of the slab that lies inside the matrix (the zeros substituted for rows past M do not count), a slab whose maximum is
// zero or not finite leaves m_run alone and is split at the scale in force; (s, rs) = f2g_f16_scales(m_run).  When the
// scale moves, both accumulator sets are multiplied by the exact power of two s_new / s_old before the slab's MFMAs (a
// wave-uniform branch, not taken while the scale stands).  v = h3_value(acc, acx, rs_run, B.rscale[col]) goes through
// the generic epilogue.  The maxima are integer maxima of sign-less bit patterns (thread, wave, one LDS word
// per wave): the result is reproducible.  Per output
//   |err| <= 3 * 2^-22 sum_k |a||w| + 2^-28 sum_T arun_T sum_{k in T} |w_k|
// with arun_T the running maximum in force at slab T of the row's tile (tests/fp16x3_runtile_emul.py).
// Rows share their tile's scale: a row quiet against its tile sees the floor term, which the image route's per-row
// scale spares it.
//
// THE SCHEDULE, one barrier per slab as in gemm_h3_kernel.  Slab t + 1 is in registers since step t - 1; its maxima are
// reduced at the end of step t - 1 (the loads have had the step's MFMAs to land) into four LDS words of the slab's
// parity, and the barrier that ends step t - 1 publishes them.  Step t requests slab t + 2, combines the four words
// into the scale of slab t + 1, runs slab t's MFMAs with the split and the LDS stores of slab t + 1 where lstore stands
// in gemm_h3_kernel, multiplies the accumulators if the scale moved (slab t's products are in), and posts the maxima of
// slab t + 2.  The words are double-buffered by slab parity: a wave may post slab t + 2's while another still reads slab
// t + 1's.  The prologue does the same for slabs 0 and 1 with one barrier more.  A slab past the last one is loaded as
// zeros: it moves no scale and is never multiplied.
//
// RESOURCES (tools/kernel_resources.py, gfx950): 218 VGPRs (gemm_h3_kernel: 213), 0 AGPRs, 0 scratch, 0 vector spills,
// 2 waves per SIMD (two blocks per CU); 28 scalar registers are parked in VGPR lanes, all of them in the generic
// epilogue behind the K loop (gemm_h3_kernel: 50 in the same place), none inside the loop.  73760 bytes of LDS (two
// buffers of 2 x 128 rows x 144 bytes, 8 maxima words): two blocks per CU.
// MEASURED: tools/fp16x3_shapes.py --noimage -> profiles/fp16x3_gemm_noimage_shapes.txt; DESIGN.md section 0 has the
// numbers and what they say.
#include <stddef.h>
#include <stdint.h>

#include "gemm_f16_common.h"
#include "split_f16.h"

namespace {

__device__ __forceinline__ float4 h3n_f4(const u32x4 v) {
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

__global__ __launch_bounds__(256, 2) void gemm_h3n_kernel(const f2g_gemm_desc d, int M, int N, int K) {
  constexpr int BM = 128, BN = 128, TSZ = 128 * LDR;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  unsigned* smx = reinterpret_cast<unsigned*>(smem + 4 * TSZ);      // [slab parity][4 waves]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
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

  // slab j: A's fp32 chunks (past the last slab: zeros, which move no scale), B's image chunks (past the last slab:
  // the first one again, never used)
  auto gload = [&](int j, u32x4 (&la)[4], u32x4 (&lb)[4]) {
    const bool on = j < nt;
    const int so = on ? j * BK * 4 : 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      la[q] = __builtin_amdgcn_raw_buffer_load_b128(ra, on ? offA[q] : 0x80000000u, so, 0);
      lb[q] = __builtin_amdgcn_raw_buffer_load_b128(rb, offB, so + q * qstepB, 0);
    }
  };
  // A's chunks are split at the scale s on their way to LDS, B's are stored as they are
  auto lstore = [&](int bufoff, const u32x4 (&la)[4], const u32x4 (&lb)[4], float s) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint4 p = f2g_f16_split4(h3n_f4(la[q]), s);
      *reinterpret_cast<u32x2*>(wA + bufoff + q * 32 * LDR) = u32x2{p.x, p.y};
      *reinterpret_cast<u32x2*>(wA + bufoff + q * 32 * LDR + 16) = u32x2{p.z, p.w};
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
  // the maximum of the A slab in the registers, per wave, into the word of its parity (read behind the next barrier)
  auto post_amax = [&](const u32x4 (&la)[4], int par) {
    unsigned m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) m = f2g_f16_amax4(h3n_f4(la[q]), m);
    m = h3n_wave_max(m);
    if (lane == 0) smx[par * 4 + wave] = m;
  };
  // the running scale moves on to the slab whose maxima are in m4; f = s_new / s_old
  unsigned mrun = 0u;                      // 0 = scale 1
  float s = 1.f, rs = 1.f;
  auto next_scale = [&](const unsigned* m4, float& f) {
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

  // two register stages: slab t's MFMAs run while slab t + 1 (in registers since the previous step) is split into LDS
  // and the loads of slab t + 2 fly
  u32x4 xa[4], xb[4], ya[4], yb[4];
  gload(0, xa, xb);
  post_amax(xa, 0);
  __syncthreads();
  {
    float f;
    next_scale(smx, f);                    // (the accumulators are zero: no rescale)
  }
  lstore(0, xa, xb, s);
  gload(1, xa, xb);
  post_amax(xa, 1);
  __syncthreads();
  auto step = [&](int t, int curoff, int nxtoff, const u32x4 (&wa)[4], const u32x4 (&wb)[4], u32x4 (&la)[4],
                  u32x4 (&lb)[4]) {
    f16x8 fa[4], fb[4];
    float f;
    gload(t + 2, la, lb);
    next_scale(smx + ((t + 1) & 1) * 4, f);
    frags(curoff, 0, fa, fb);
    h3_mfma12(acc, acx, fa, fa + 2, fb, fb + 2);
    lstore(nxtoff, wa, wb, s);
    frags(curoff, 1, fa, fb);
    h3_mfma12(acc, acx, fa, fa + 2, fb, fb + 2);
    if (f != 1.f) {                        // the scale moved: the stored sums go over to slab t + 1's
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            acc[mi][ni][e] *= f;
            acx[mi][ni][e] *= f;
          }
    }
    post_amax(la, t & 1);                  // slab t + 2 has landed under the MFMAs
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

  // v = (acc0 + 2^-11 acc1) / s_run / s_b[col] (gemm_f16_common.h: h3_value), then the generic epilogue on v
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int col = n0 + (wn * 2 + ni) * 32 + li;
    const float sb = col < N ? d.B.rscale[col] : 0.f;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][ni][e] = h3_value(acc[mi][ni][e], acx[mi][ni][e], rs, sb);
  }
  gemm_epilogue<2, 2>(d.E, acc, M, N, m0, n0, wm, wn, li, h, true);
}

}  // namespace

int f2g_launch_h3n(const f2g_gemm_desc& d, hipStream_t st) {
  const int M = d.A.rows, N = d.B.rows, K = d.A.cols;
  constexpr int smem = 4 * 128 * LDR * 4 + 2 * 4 * (int)sizeof(unsigned);
  dyn_lds_once<gemm_h3n_kernel>(smem);
  f2g_note_kernel("h3n<ep=all>", 1, 6);
  hipLaunchKernelGGL(gemm_h3n_kernel, dim3((M + 127) / 128, (N + 127) / 128), dim3(256), smem, st, d, M, N, K);
  return f2g_check_launch();
}
