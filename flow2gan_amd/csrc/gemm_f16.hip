// fp16x3: fp32-class products from TWO scaled fp16 pieces per operand, three MFMAs per product (gemm.hip has the
// family, gemm_common.h what the GEMM files share).  f2g_split_f16x2 writes the operand images, gemm_h3_kernel reads them.
#include <stddef.h>
#include <stdint.h>

#include "gemm_common.h"
#include "split_f16.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// One wave per row, four rows per block and pass (split_f16.h has the routine and the arithmetic)
__global__ __launch_bounds__(256) void split_f16x2_kernel(float* dst, float* rscale, const float* src, long long ld,
                                                          int rows, int K) {
  f2g_split_f16x2_rows<true>(dst, rscale, src, ld, rows, K, (long long)blockIdx.x * 4 + (threadIdx.x >> 6),
                       (long long)gridDim.x * 4);
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
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][ni][e] = acx[mi][ni][e] = 0.f;

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
  auto mfma12 = [&](const f16x8 (&fa)[4], const f16x8 (&fb)[4]) {
#pragma unroll
    for (int term = 0; term < 3; ++term)
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          if (term == 0)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[mi], fb[ni], acc[mi][ni], 0, 0, 0);
          else
            acx[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(term == 1 ? fa[mi] : fa[2 + mi],
                                                                 term == 1 ? fb[2 + ni] : fb[ni], acx[mi][ni], 0, 0, 0);
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
    mfma12(fa, fb);
    lstore(nxtoff, wa, wb);
    frags(curoff, 1, fa, fb);
    mfma12(fa, fb);
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

  // v = (acc0 + 2^-11 acc1) / s_a[row] / s_b[col]: the reciprocals one after the other (their product may leave the
  // float range), then the generic epilogue on v
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
        acc[mi][ni][e] = (acc[mi][ni][e] + acx[mi][ni][e] * 0x1p-11f) * sa * sb;
      }
  }
  gemm_epilogue<2, 2>(d.E, acc, M, N, m0, n0, wm, wn, li, h, true);
}

inline bool h3_operand_ok(const f2g_operand& S) {
  return host_plain(S) && !S.alpha && S.rows > 0 && S.cols >= BK && S.cols % BK == 0 && S.cols <= F2G_F16_MAX_K &&
         al16(S.base) && (S.seq_stride & 3) == 0 && S.seq_stride >= S.cols &&
         (long long)S.rows * S.seq_stride * 4 < 0x7ff00000ll;
}

// 0: not for this kernel; 1: as handed over (both operands f2g_split_f16x2 images with their reciprocal scales);
// 2: once both fp32 operands are replaced by their images
int h3_ok(const f2g_gemm_desc& d) {
  if (d.form != 0 || !d.A.base || !d.B.base || !d.E.C || d.A.cols != d.B.cols) return 0;
  if (!h3_operand_ok(d.A) || !h3_operand_ok(d.B)) return 0;
  const f2g_epilogue& E = d.E;
  if (d.split_k > 1 || E.x3_out || E.colsum_part_ld > 0 || E.c_bf16) return 0;
  // (the combinations f2g_gemm refuses for every kernel)
  if (E.prelu_slope && (E.atomic || E.accumulate || E.P0o > 0)) return 0;
  if (E.mask_src && (E.atomic || E.accumulate)) return 0;
  if (E.aux && !E.alpha_n) return 0;
  if (d.A.split == 5 && d.B.split == 5) return d.A.rscale && d.B.rscale ? 1 : 0;
  return d.A.split == 0 && d.B.split == 0 ? 2 : 0;
}

}  // namespace

extern "C" int f2g_gemm_f16_ok(const f2g_gemm_desc* dp) { return dp ? h3_ok(*dp) : 0; }

int f2g_gemm_h3(const f2g_gemm_desc& d, hipStream_t st) {
  if (h3_ok(d) != 1) {
    f2g_set_error("f2g_gemm precision 4: form 0 over f2g_split_f16x2 images of two plain matrices "
                  "(f2g_gemm_f16_ok(d) != 1 for this descriptor)");
    return F2G_EINVAL;
  }
  const int M = d.A.rows, N = d.B.rows, K = d.A.cols;
  constexpr int smem = 4 * 128 * LDR * 4;
  dyn_lds_once<gemm_h3_kernel>(smem);
  f2g_note_kernel("h3<ep=all>", 1, 6);
  hipLaunchKernelGGL(gemm_h3_kernel, dim3((M + 127) / 128, (N + 127) / 128), dim3(256), smem, st, d, M, N, K);
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
