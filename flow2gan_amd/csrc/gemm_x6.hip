// ---- fp32-class GEMM on the bf16 matrix pipe (precision 3; round 3) -------------------------------
// Every fp32 operand is split into THREE bf16 pieces x = p0 + p1 + p2 (24 mantissa bits) and a product
// is the six MFMAs with i + j <= 2 (a0b0, a0b1, a1b0, a0b2, a1b1, a2b0; fp32 accumulation, smallest
// terms first): what is dropped is <= 2^-24 relative -- the error class of fp32 rounding itself
// (measured 8e-8 ... 1e-7 of sum |a w| where the fp32 fmaf chain has 7e-8 ... 2e-7, tools/micro/x6_lab.hip),
// not the 2^-16 of the two-piece mode.  The fp32 MFMA needs 8 x 64 cycles for the block of products
// these six 32-cycle MFMAs cover, so the matrix pipe is 2.7x less busy per FLOP.
// Operand image (f2g_split_bf16x3): row-major, per 32-element slab of a row its three pieces side by
// side, [row][K / 32][piece][32] bf16 = 192 contiguous bytes per row and slab (whole cache lines).
// Kernel: the simplest structure that works -- 128 x 128 x 32 tiles, 4 waves of 64 x 64, single LDS
// buffer (rows 208 bytes apart: 52 dwords, conflict-free for ds_read_b128), the next slab's operands
// requested one pass ahead by buffer loads with per-thread constant offsets, the whole slab's fragments
// in registers, TWO blocks per CU hide each other's store / barrier / read phases:
//   store slab t -> barrier -> read its 24 fragments -> barrier -> 48 MFMAs.
// Plain (rows x K) operands only (the generator's 1x1 convolutions and linears); epilogue = the generic
// kernel's (bias, residual, PReLU with both outputs, PReLU backward with column sums, ...).
#include <stddef.h>
#include <stdint.h>

#include "gemm_common.h"
#include "x6_epilogue.h"

// (gemm_x6_kernel raises its waves' priority for the MFMA phase: +2 ... 14 % in the step; the kernels that
// split operands on the VALU lose with it -- the other block's split is what feeds their next slab)
#define X6_MFMA_PRIO 1

#if F2G_X6LAB & 256      // (gemm_common.h lists the lab bits)
// gemm_x6f_kernel's interval sums: [0] MFMA chain with the staging between, [1] wait for the block at the "stores
// visible" barrier, [2] fragment reads + "fragments read" barrier, [3] iterations, [4] kernel entry -> first chain
// (prologue), [5] the last slab's chain (12 x 4 MFMAs issued), [6] epilogue, [7] blocks
__device__ unsigned long long g_x6prof[8];
extern "C" int f2g_lab_x6prof(unsigned long long* out8) {
  unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_x6prof), sizeof(z)) != hipSuccess) return 1;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_x6prof), z, sizeof(z)) != hipSuccess;
}
#endif

__global__ __launch_bounds__(256) void split3_img_kernel(__bf16* __restrict__ dst, const float* __restrict__ src,
                                                         long long ld, long long rows, int K) {
  const long long total = rows * (K / 4);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / (K / 4);
    const int k4 = (int)(i - r * (K / 4)) * 4;
    const float4 v = *reinterpret_cast<const float4*>(src + r * ld + k4);
    const float x[4] = {v.x, v.y, v.z, v.w};
    unsigned short p[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const __bf16 a = (__bf16)x[e];
      const float r1 = x[e] - (float)a;
      const __bf16 b = (__bf16)r1;
      const __bf16 c = (__bf16)(r1 - (float)b);
      p[0][e] = __builtin_bit_cast(unsigned short, a);
      p[1][e] = __builtin_bit_cast(unsigned short, b);
      p[2][e] = __builtin_bit_cast(unsigned short, c);
    }
    __bf16* o = dst + (r * (K / 32) + k4 / 32) * 96 + (k4 & 31);
#pragma unroll
    for (int q = 0; q < 3; ++q)
      *reinterpret_cast<uint2*>(o + 32 * q) =
          make_uint2(p[q][0] | ((unsigned)p[q][1] << 16), p[q][2] | ((unsigned)p[q][3] << 16));
  }
}

// The tile's three-piece image for the next GEMM (f2g_epilogue.x3_out): read back what the block has just
// stored (L2; the barrier orders the block's own stores before these loads) and write whole 16-byte pieces.
template <int ROWS = 128, int NTHR = 256>
__device__ __forceinline__ void x3_tile_readback(const f2g_epilogue& E, int M, int N, int m0, int n0, int tid) {
  __syncthreads();
  for (int u = tid; u < ROWS * 16; u += NTHR) {
    const int row = m0 + (u >> 4), col = n0 + (u & 15) * 8;
    if (row >= M || col >= N) continue;
    long long off;
    if (E.P0o > 0) {
      const int sq = row / E.P0o;
      off = (long long)sq * E.seq_stride_o + (long long)(row - sq * E.P0o) * E.row_stride_o + E.off_o + col;
    } else {
      off = (long long)row * E.ldc + col;
    }
    const float4 v0 = *reinterpret_cast<const float4*>(E.C + off);
    const float4 v1 = *reinterpret_cast<const float4*>(E.C + off + 4);
    const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    unsigned pk[3][4];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const __bf16 a = (__bf16)x[e];
      const float r1 = x[e] - (float)a;
      const __bf16 b = (__bf16)r1;
      const __bf16 c = (__bf16)(r1 - (float)b);
      const unsigned sa = __builtin_bit_cast(unsigned short, a), sb = __builtin_bit_cast(unsigned short, b),
                     sc = __builtin_bit_cast(unsigned short, c);
      if (e & 1) pk[0][e >> 1] |= sa << 16, pk[1][e >> 1] |= sb << 16, pk[2][e >> 1] |= sc << 16;
      else pk[0][e >> 1] = sa, pk[1][e >> 1] = sb, pk[2][e >> 1] = sc;
    }
    __bf16* q = reinterpret_cast<__bf16*>(E.x3_out) + (off >> 5) * 96 + (off & 31);
#pragma unroll
    for (int pc = 0; pc < 3; ++pc)
      *reinterpret_cast<uint4*>(q + 32 * pc) = make_uint4(pk[pc][0], pk[pc][1], pk[pc][2], pk[pc][3]);
  }
}

// A rows: plain (row r at r * K * 6 bytes of a dense image) or single-segment windows over the flat image
// of a contiguous buffer (MPD halo maps: row (s, p) at s * seq6 + p * step6 + off6 bytes, K contiguous --
// element e of a contiguous buffer lives at (e / 32) * 192 + piece * 64 + (e % 32) * 2 whatever its row
// length, so a window that starts on a 32-element boundary addresses the image like the tensor)
struct x6_rows {
  int P0;
  unsigned seq6, step6, off6, bytes;
};

__global__ __launch_bounds__(256, 2) void gemm_x6_kernel(const f2g_gemm_desc d, int M, int N, int K,
                                                         const x6_rows R, const int wide) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem6[];
  constexpr int PITCH = 208, OPER = 128 * PITCH, NJ = 6;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, h = lane >> 5;
  int m0, n0;
  tile_of_block(128, 128, m0, n0);
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  const unsigned rowbytes = (unsigned)(K / 32) * 192u;
  __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)d.A.base, 0, R.bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)d.B.base, 0, (unsigned)N * rowbytes, 0x00020000);
  // chunk id = tid + 256 j -> (row of the tile, 16-byte chunk of the row's 192 bytes); rows past the
  // end lie outside the resource: zeros
  unsigned voA[NJ], voW[NJ];
  int lo[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int id = tid + 256 * j, row = id / 12, c = id - row * 12;
    const int r = m0 + row, sq = r / R.P0;
    voA[j] = r < M ? (unsigned)sq * R.seq6 + (unsigned)(r - sq * R.P0) * R.step6 + R.off6 + c * 16
                   : 0xf0000000u;                 // (outside the resource: zeros)
    voW[j] = (unsigned)(n0 + row) * rowbytes + c * 16;
    lo[j] = row * PITCH + c * 16;
  }
  u32x4 xa[NJ], xw[NJ];
  auto gload = [&](int t) {
    const int so = t * 192;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      xa[j] = __builtin_amdgcn_raw_buffer_load_b128(rsA, voA[j], so, 0);
      xw[j] = __builtin_amdgcn_raw_buffer_load_b128(rsW, voW[j], so, 0);
    }
  };
  const unsigned char* rA = smem6 + (wm * 64 + li) * PITCH + h * 16;
  const unsigned char* rB = smem6 + OPER + (wn * 64 + li) * PITCH + h * 16;
  const int nt = K / 32;
  gload(0);
  for (int t = 0; t < nt; ++t) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      *reinterpret_cast<u32x4*>(smem6 + lo[j]) = xa[j];
      *reinterpret_cast<u32x4*>(smem6 + OPER + lo[j]) = xw[j];
    }
    gload(t + 1 < nt ? t + 1 : 0);       // (past the end: re-read, never used)
    lds_barrier();
    bf16x8 fa[2][3][2], fb[2][3][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          fa[ks][p][i] = *reinterpret_cast<const bf16x8*>(rA + p * 64 + i * 32 * PITCH + ks * 32);
          fb[ks][p][i] = *reinterpret_cast<const bf16x8*>(rB + p * 64 + i * 32 * PITCH + ks * 32);
        }
    lds_barrier();
    __builtin_amdgcn_s_setprio(X6_MFMA_PRIO);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int sdeg = 2; sdeg >= 0; --sdeg)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const int j = sdeg - i;
          if (j < 0 || j > 2) continue;
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][i][mi], fb[ks][j][ni], acc[mi][ni], 0, 0, 0);
        }
    __builtin_amdgcn_s_setprio(0);
  }
  if (wide) {
    // (every fragment read of the main loop lies before its last barrier: a wave that is through its MFMAs
    // may overlay the operand buffers with its private patch)
    X6LAB_EPI x6e::wide_epilogue(d.E, acc, M, N, m0 + wm * 64, n0 + wn * 64, lane, smem6 + wave * x6e::ESZ);
    return;
  }
  X6LAB_EPI gemm_epilogue<2, 2>(d.E, acc, M, N, m0, n0, wm, wn, li, h, true);
  if (X6LAB_X3 d.E.x3_out) x3_tile_readback(d.E, M, N, m0, n0, tid);
}

// (Stride-1 conv windows -- the (5, 1) MPD layers and the two-tap residues of their stride-3 data gradients --
// run on the tap-walking ping-pong kernel of gemm_x6p.hip; its 128-row and single-group 256-row predecessors
// gemm_x6t_kernel / gemm_x6t8_kernel were removed in round 6.  Windows gemm_x6p_kernel does not take -- fewer
// than 64 channels per position, grids that do not fill the chip -- read their rows through the kernel above.)

// The same tile and schedule over the fp32 operands themselves (f2g_operand.split = 0): every thread
// splits the 4-float chunks it loads into the three pieces on their way into LDS, as gemm_leanw6_kernel
// does -- 4 bytes per element from L2 instead of 6, no image pass, no producer, 5.5 VALU instructions per
// element beside the 48 MFMAs per slab and wave.
template <bool WIMG>
__global__ __launch_bounds__(256, 2) void gemm_x6f_kernel(const f2g_gemm_desc d, int M, int N, int K,
                                                          const x6_rows R, const int wide) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem6[];
#if F2G_X6LAB & 256
  unsigned long long pe0, pe1, pe2, pe3;
  X6PROF_STAMP(pe0);
#endif
  // WIMG (round 5): the WEIGHT operand is its cached f2g_split_bf16x3 image (192 bytes per row and slab, stored
  // to LDS as it comes) -- every one of the M / 128 row tiles used to split the same weight slab again; only
  // the activation rows (read once per column tile) are still split here
  constexpr int PITCH = 208, OPER = 128 * PITCH, NJ = 4, NJW = WIMG ? 6 : 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, h = lane >> 5;
  int m0, n0;
  tile_of_block(128, 128, m0, n0);
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  // (here R.seq6 / step6 / off6 / bytes are in units of 4 bytes per element: x6_rows_of(d, 4))
  __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)d.A.base, 0, R.bytes, 0x00020000);
  const unsigned rowbytesW = (unsigned)(K / 32) * 192u;
  __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc(
      (void*)d.B.base, 0, WIMG ? (unsigned)N * rowbytesW : (unsigned)((long long)N * d.B.seq_stride * 4), 0x00020000);
  // chunk id = tid + 256 j -> (row of the tile, 16-byte chunk = 4 of the slab's 32 floats)
  unsigned voA[NJ], voW[NJW];
  int lo[NJ], loW[NJW];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int id = tid + 256 * j, row = id >> 3, c = id & 7;
    const int r = m0 + row, sq = r / R.P0;
    voA[j] = r < M ? (unsigned)sq * R.seq6 + (unsigned)(r - sq * R.P0) * R.step6 + R.off6 + c * 16 : 0xf0000000u;
    lo[j] = row * PITCH + c * 8;
  }
#pragma unroll
  for (int j = 0; j < NJW; ++j) {
    const int id = tid + 256 * j;
    if (WIMG) {
      const int row = id / 12, c = id - row * 12;
      voW[j] = n0 + row < N ? (unsigned)(n0 + row) * rowbytesW + c * 16 : 0xf0000000u;
      loW[j] = row * PITCH + c * 16;
    } else {
      const int row = id >> 3, c = id & 7;
      voW[j] = n0 + row < N ? (unsigned)((long long)(n0 + row) * d.B.seq_stride * 4) + c * 16 : 0xf0000000u;
      loW[j] = row * PITCH + c * 8;
    }
  }
  u32x4 xa[NJ], xw[NJW];
  auto gload = [&](int t) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) xa[j] = __builtin_amdgcn_raw_buffer_load_b128(rsA, voA[j], t * 128, 0);
#pragma unroll
    for (int j = 0; j < NJW; ++j) xw[j] = __builtin_amdgcn_raw_buffer_load_b128(rsW, voW[j], t * (WIMG ? 192 : 128), 0);
  };
  const unsigned char* rA = smem6 + (wm * 64 + li) * PITCH + h * 16;
  const unsigned char* rB = smem6 + OPER + (wn * 64 + li) * PITCH + h * 16;
  const int nt = K / 32;
  bf16x8 fa[2][3][2], fb[2][3][2];
  // Schedule (round 6).  The slab loop used to be phases -- split + store, barrier, fragments, barrier, 48 MFMAs --
  // and relied on the CU's other block to fill the matrix pipe meanwhile; measured, the phases simply ADD
  // (lab builds, tools/micro/x6lab_run.sh: without the split -32 us, without 44 of the 48 MFMAs -71 us of a 143 us
  // launch), and tools/micro/mfma_valu_overlap.hip shows why: VALU work of ANOTHER wave hides only partly behind a
  // wave's MFMAs, VALU work of the SAME wave's stream, issued between its MFMAs, hides completely.  The operand
  // buffer is dead once every wave holds its fragments, so the staging of slab t + 1 -- the split of the
  // activation chunks, the LDS stores of both operands, the requests for slab t + 2 -- now sits between the MFMAs
  // of slab t, one chunk per quarter of the chain, and only the fragment reads stand between two MFMA chains.
  auto stage_a = [&](int j) {
    u32x2 p0, p1, p2;
    split3x4(xa[j], p0, p1, p2);
#if F2G_X6LAB & 512      // (lab: the split without its LDS stores)
    asm volatile("" : : "v"(p0.x), "v"(p0.y), "v"(p1.x), "v"(p1.y), "v"(p2.x), "v"(p2.y));
    return;
#endif
    *reinterpret_cast<u32x2*>(smem6 + lo[j]) = p0;
    *reinterpret_cast<u32x2*>(smem6 + lo[j] + 64) = p1;
    *reinterpret_cast<u32x2*>(smem6 + lo[j] + 128) = p2;
  };
  auto stage_w = [&](int j) {
#if F2G_X6LAB & 512
    asm volatile("" : : "v"(xw[j].x), "v"(xw[j].y), "v"(xw[j].z), "v"(xw[j].w));
    return;
#endif
    if (WIMG) {
      *reinterpret_cast<u32x4*>(smem6 + OPER + loW[j]) = xw[j];
    } else {
      u32x2 p0, p1, p2;
      split3x4(xw[j], p0, p1, p2);
      *reinterpret_cast<u32x2*>(smem6 + OPER + loW[j]) = p0;
      *reinterpret_cast<u32x2*>(smem6 + OPER + loW[j] + 64) = p1;
      *reinterpret_cast<u32x2*>(smem6 + OPER + loW[j] + 128) = p2;
    }
  };
  auto frags = [&]() {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          fa[ks][p][i] = *reinterpret_cast<const bf16x8*>(rA + p * 64 + i * 32 * PITCH + ks * 32);
          fb[ks][p][i] = *reinterpret_cast<const bf16x8*>(rB + p * 64 + i * 32 * PITCH + ks * 32);
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
  gload(0);
#pragma unroll
  for (int j = 0; j < NJ; ++j) stage_a(j);
#pragma unroll
  for (int j = 0; j < NJW; ++j) stage_w(j);
  gload(nt > 1 ? 1 : 0);
  lds_barrier();
  frags();
  lds_barrier();
#if F2G_X6LAB & 256
  unsigned long long pt0, pt1, pt2;
  unsigned long long ps0 = 0, ps1 = 0, ps2 = 0;
  X6PROF_STAMP(pt0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  pt2 = pt0;
  pe1 = pt0;
#endif
  for (int t = 0; t + 1 < nt; ++t) {
    const int t2 = t + 2 < nt ? t + 2 : 0;       // (past the end: re-read, never used)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // quarter q: MFMA groups 3 q ... 3 q + 2 with the staging of activation chunk q (and its share of the
      // weight chunks) between them; the chunk's registers are requested again for slab t + 2 right away
      mf4(3 * q);
      if (WIMG) {
        if (q < 3) {
          stage_w(2 * q);
          stage_w(2 * q + 1);
          xw[2 * q] = __builtin_amdgcn_raw_buffer_load_b128(rsW, voW[2 * q], t2 * 192, 0);
          xw[2 * q + 1] = __builtin_amdgcn_raw_buffer_load_b128(rsW, voW[2 * q + 1], t2 * 192, 0);
        }
      } else {
        stage_w(q);
        xw[q] = __builtin_amdgcn_raw_buffer_load_b128(rsW, voW[q], t2 * 128, 0);
      }
      mf4(3 * q + 1);
      stage_a(q);
      xa[q] = __builtin_amdgcn_raw_buffer_load_b128(rsA, voA[q], t2 * 128, 0);
      mf4(3 * q + 2);
#if !(F2G_X6LAB & 128)
      // one MFMA, then its share of the quarter's VALU work; the LDS stores and the requests close the quarter
#pragma unroll
      for (int m = 0; m < 12; ++m) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, WIMG ? 3 : 5, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x200, 8, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 3, 0);
#endif
      __builtin_amdgcn_sched_barrier(0);
    }
    X6PROF_STAMP(pt1);
    lds_barrier();
    X6PROF_ACC(ps0, pt1, pt0);
    X6PROF_ACC(ps2, pt0, pt2);      // (the previous iteration's fragment interval)
    X6PROF_STAMP(pt2);
    frags();
    lds_barrier();
    X6PROF_ACC(ps1, pt2, pt1);
    X6PROF_STAMP(pt0);
  }
#if F2G_X6LAB & 256
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  X6PROF_ACC(ps2, pt0, pt2);
  if (tid == 0 && nt > 1) {
    atomicAdd(&g_x6prof[0], ps0);
    atomicAdd(&g_x6prof[1], ps1);
    atomicAdd(&g_x6prof[2], ps2);
    atomicAdd(&g_x6prof[3], (unsigned long long)(nt - 1));
  }
#endif
  X6PROF_STAMP(pe2);
#pragma unroll
  for (int g = 0; g < 12; ++g) mf4(g);
  X6PROF_STAMP(pe3);
  if (wide) {
    // (every fragment read of the main loop lies before its last barrier: a wave that is through its MFMAs
    // may overlay the operand buffers with its private patch)
    X6LAB_EPI x6e::wide_epilogue(d.E, acc, M, N, m0 + wm * 64, n0 + wn * 64, lane, smem6 + wave * x6e::ESZ);
#if F2G_X6LAB & 256
    unsigned long long pe4;
    X6PROF_STAMP(pe4);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    if (tid == 0) {
      atomicAdd(&g_x6prof[4], pe1 - pe0);
      atomicAdd(&g_x6prof[5], pe3 - pe2);
      atomicAdd(&g_x6prof[6], pe4 - pe3);
      atomicAdd(&g_x6prof[7], 1ull);
    }
#endif
    return;
  }
  X6LAB_EPI gemm_epilogue<2, 2>(d.E, acc, M, N, m0, n0, wm, wn, li, h, true);
  if (X6LAB_X3 d.E.x3_out) x3_tile_readback(d.E, M, N, m0, n0, tid);
}

// gemm_x6f_kernel<true> with the WEIGHT fragments straight from memory (round 6).  Measured on the kernel above
// (tools/micro/x6prof.py: s_memtime stamps inside the slab loop): with the staging between the MFMAs a chain of 48
// MFMAs (1536 clocks) takes 2420 clocks alone on its CU, 1800 without the LDS stores -- a store moves its address
// and data registers to the LDS at 2 clocks per source dword (MI355X_MICROARCH.md, LDS), ~600 clocks per slab
// and block, and the wave's MFMAs wait behind it.  Half of those stores put the weight image into LDS only to read
// it back in MFMA fragment order.  Here the cached weight image is FRAGMENT-MAJOR (B.split = 4: [N / 32][K / 32]
// [piece][k step][lane][16 bytes] -- the pieces of f2g_split_bf16x3 in another order: F2G_MULTI_SPLIT3G), so a
// wave's B fragment is one coalesced 1 KB load into the registers the MFMAs read: no LDS store, no LDS read, no
// staging registers for the weights; the two k-step halves of the fragment set are requested again for slab
// t + 1 as soon as the MFMAs of slab t have consumed them.  LDS carries the activation tile only (half the
// stores, half the fragment reads of gemm_x6f_kernel).
__global__ __launch_bounds__(256, 2) void gemm_x6g_kernel(const f2g_gemm_desc d, int M, int N, int K,
                                                          const x6_rows R, const int wide) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem6[];
  constexpr int PITCH = 208, NJ = 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, h = lane >> 5;
  int m0, n0;
  tile_of_block(128, 128, m0, n0);
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  const int nt = K / 32;
  __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)d.A.base, 0, R.bytes, 0x00020000);
  // (the image ends with the last whole 32-row group: groups of a ragged last tile read zeros)
  __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)d.B.base, 0, (unsigned)((long long)N * K * 6), 0x00020000);
  unsigned voA[NJ];
  int lo[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int id = tid + 256 * j, row = id >> 3, c = id & 7;
    const int r = m0 + row, sq = r / R.P0;
    voA[j] = r < M ? (unsigned)sq * R.seq6 + (unsigned)(r - sq * R.P0) * R.step6 + R.off6 + c * 16 : 0xf0000000u;
    lo[j] = row * PITCH + c * 8;
  }
  // fragment (i, piece p, k step ks) of slab t: 1 KB at (((n0 / 32 + 2 wn + i) nt + t) 12 + 4 p + 2 ks) * 512 bytes
  unsigned voB[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) voB[i] = (unsigned)((n0 >> 5) + 2 * wn + i) * (unsigned)nt * 6144u + lane * 16;
  u32x4 xa[NJ];
  u32x2 pa[NJ][3];      // the pieces of slab t + 1, split during the chain of slab t, stored behind it
  bf16x8 fa[2][3][2], fb[2][3][2];
  auto load_b = [&](int ks, int t) {        // the six fragments of k step ks
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int i = 0; i < 2; ++i)
        fb[ks][p][i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsW, voB[i] + (4 * p + 2 * ks) * 512, t * 6144, 0));
  };
  auto stage_a = [&](int j) {
    u32x2 p0, p1, p2;
    split3x4(xa[j], p0, p1, p2);
    *reinterpret_cast<u32x2*>(smem6 + lo[j]) = p0;
    *reinterpret_cast<u32x2*>(smem6 + lo[j] + 64) = p1;
    *reinterpret_cast<u32x2*>(smem6 + lo[j] + 128) = p2;
  };
  const unsigned char* rA = smem6 + (wm * 64 + li) * PITCH + h * 16;
  auto frags_a = [&]() {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int i = 0; i < 2; ++i)
          fa[ks][p][i] = *reinterpret_cast<const bf16x8*>(rA + p * 64 + i * 32 * PITCH + ks * 32);
  };
  // the 48 MFMAs of a slab as 12 groups of four (one product term of one k step), smallest terms first
  auto mf4 = [&](int g) {
    const int ks = g / 6, r = g % 6;
    const int i = r == 0 ? 0 : r == 1 ? 1 : r == 2 ? 2 : r == 3 ? 0 : r == 4 ? 1 : 0;
    const int j = r < 3 ? 2 - i : r < 5 ? 1 - i : 0;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][i][mi], fb[ks][j][ni], acc[mi][ni], 0, 0, 0);
  };
#pragma unroll
  for (int j = 0; j < NJ; ++j) xa[j] = __builtin_amdgcn_raw_buffer_load_b128(rsA, voA[j], 0, 0);
  load_b(0, 0);
  load_b(1, 0);
#pragma unroll
  for (int j = 0; j < NJ; ++j) stage_a(j);
#pragma unroll
  for (int j = 0; j < NJ; ++j) xa[j] = __builtin_amdgcn_raw_buffer_load_b128(rsA, voA[j], nt > 1 ? 128 : 0, 0);
  lds_barrier();
  frags_a();
  lds_barrier();
  for (int t = 0; t + 1 < nt; ++t) {
    const int t2 = t + 2 < nt ? t + 2 : 0;       // (past the end: re-read, never used)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // quarter q: MFMA groups 3 q ... 3 q + 2 with the staging of activation chunk q of slab t + 1 between them;
      // the chunk's registers are requested again for slab t + 2 right away.  Groups 0-5 are k step 0, 6-11 k step
      // 1: quarter 2 opens with the requests for k step 0 of slab t + 1, quarter 3 closes with those for k step 1.
      if (q == 2) load_b(0, t + 1);
      mf4(3 * q);
      mf4(3 * q + 1);
#if F2G_X6LAB & 1024      // (lab: the stores inside the chain, quarter by quarter)
      stage_a(q);
#else
      split3x4(xa[q], pa[q][0], pa[q][1], pa[q][2]);
#endif
      xa[q] = __builtin_amdgcn_raw_buffer_load_b128(rsA, voA[q], t2 * 128, 0);
      mf4(3 * q + 2);
      if (q == 3) load_b(1, t + 1);
      if (q == 2) __builtin_amdgcn_sched_group_barrier(0x020, 6, 0);
#pragma unroll
      for (int m = 0; m < 12; ++m) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x200, 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 7, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
#if !(F2G_X6LAB & 1024)
    // the twelve LDS stores of the slab BEHIND the chain: a store moves its address and data registers to the LDS
    // over the path the MFMAs read their operands through -- between the MFMAs they cost the chain ~50 clocks each
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      *reinterpret_cast<u32x2*>(smem6 + lo[q]) = pa[q][0];
      *reinterpret_cast<u32x2*>(smem6 + lo[q] + 64) = pa[q][1];
      *reinterpret_cast<u32x2*>(smem6 + lo[q] + 128) = pa[q][2];
    }
#endif
    lds_barrier();
    frags_a();
    lds_barrier();
  }
#pragma unroll
  for (int g = 0; g < 12; ++g) mf4(g);
  if (wide) {
    x6e::wide_epilogue(d.E, acc, M, N, m0 + wm * 64, n0 + wn * 64, lane, smem6 + wave * x6e::ESZ);
    return;
  }
  gemm_epilogue<2, 2>(d.E, acc, M, N, m0, n0, wm, wn, li, h, true);
  if (d.E.x3_out) x3_tile_readback(d.E, M, N, m0, n0, tid);
}

// The in-kernel-split kernel for N <= 32 output columns (round 6): the data gradients that land on a 32-channel
// map -- the second MPD layer's stride residues, 341376 x 32 x 256 -- ran on the generic fp32 kernel's 128 x 32
// tiles at 50 TFLOP/s (matrix pipe 0.29 busy behind bounds-tested window loads).  Same schedule as
// gemm_x6f_kernel<true> on a 128 x 32 tile: four waves of 32 x 32, the weight slab (32 rows of the cached image)
// stored as it comes, six fragment reads each way per 12 MFMAs, generic epilogue (row maps, masks, column sums).
__global__ __launch_bounds__(256, 2) void gemm_x6n_kernel(const f2g_gemm_desc d, int M, int N, int K,
                                                          const x6_rows R) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem6[];
  constexpr int PITCH = 208, OPER = 128 * PITCH, NJ = 4, NJW = 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.x * 128, n0 = 0;
  f32x16 acc[1][1];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[0][0][e] = 0.f;
  __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)d.A.base, 0, R.bytes, 0x00020000);
  const unsigned rowbytesW = (unsigned)(K / 32) * 192u;
  __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)d.B.base, 0, (unsigned)N * rowbytesW, 0x00020000);
  unsigned voA[NJ], voW[NJW];
  int lo[NJ], loW[NJW];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int id = tid + 256 * j, row = id >> 3, c = id & 7;
    const int r = m0 + row, sq = r / R.P0;
    voA[j] = r < M ? (unsigned)sq * R.seq6 + (unsigned)(r - sq * R.P0) * R.step6 + R.off6 + c * 16 : 0xf0000000u;
    lo[j] = row * PITCH + c * 8;
  }
#pragma unroll
  for (int j = 0; j < NJW; ++j) {
    const int id = tid + 256 * j, row = id / 12, c = id - row * 12;      // 32 rows x 12 chunks = 384 chunks
    voW[j] = (id < 384 && row < N) ? (unsigned)row * rowbytesW + c * 16 : 0xf0000000u;
    loW[j] = id < 384 ? row * PITCH + c * 16 : -1;
  }
  u32x4 xa[NJ], xw[NJW];
  auto gload = [&](int t) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) xa[j] = __builtin_amdgcn_raw_buffer_load_b128(rsA, voA[j], t * 128, 0);
#pragma unroll
    for (int j = 0; j < NJW; ++j) xw[j] = __builtin_amdgcn_raw_buffer_load_b128(rsW, voW[j], t * 192, 0);
  };
  const unsigned char* rA = smem6 + (wave * 32 + li) * PITCH + h * 16;
  const unsigned char* rB = smem6 + OPER + li * PITCH + h * 16;
  const int nt = K / 32;
  gload(0);
  for (int t = 0; t < nt; ++t) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      u32x2 p0, p1, p2;
      split3x4(xa[j], p0, p1, p2);
      *reinterpret_cast<u32x2*>(smem6 + lo[j]) = p0;
      *reinterpret_cast<u32x2*>(smem6 + lo[j] + 64) = p1;
      *reinterpret_cast<u32x2*>(smem6 + lo[j] + 128) = p2;
    }
#pragma unroll
    for (int j = 0; j < NJW; ++j)
      if (loW[j] >= 0) *reinterpret_cast<u32x4*>(smem6 + OPER + loW[j]) = xw[j];
    gload(t + 1 < nt ? t + 1 : 0);       // (past the end: re-read, never used)
    lds_barrier();
    bf16x8 fa[2][3], fb[2][3];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        fa[ks][p] = *reinterpret_cast<const bf16x8*>(rA + p * 64 + ks * 32);
        fb[ks][p] = *reinterpret_cast<const bf16x8*>(rB + p * 64 + ks * 32);
      }
    lds_barrier();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int sdeg = 2; sdeg >= 0; --sdeg)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const int j = sdeg - i;
          if (j < 0 || j > 2) continue;
          acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][i], fb[ks][j], acc[0][0], 0, 0, 0);
        }
  }
  // Epilogue.  The row map of a stride residue costs the generic epilogue one 64-bit division per ELEMENT (16 per
  // lane and tile, ~35 VALU instructions each beside 96 MFMAs); here the 128 output-row offsets of the tile are
  // computed once, one division per ROW, into the (now free) operand buffer, and the elements look them up.
  // (thin_epilogue.h has the same steps as functions, for gemm_h3pn_kernel; calling them here moved this kernel from
  // 102 to 104 registers, so it keeps its own copy -- a change to one belongs in the other)
  const f2g_epilogue& E = d.E;
  if (E.aux || E.res || E.prelu_slope || E.atomic || E.accumulate || E.scale != 0.f) {
    gemm_epilogue<1, 1>(E, acc, M, N, m0, n0, wave, 0, li, h, true);
    return;
  }
  __syncthreads();                                   // every wave is through its last fragment reads
  long long* rowoff = reinterpret_cast<long long*>(smem6);
  if (tid < 128) {
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
  __syncthreads();
  const int col = li;
  if (col >= N) return;
  const float bias = E.bias ? E.bias[col] : 0.f;
  const float fmw = E.fm_ref ? E.fm_w * (E.fm_wdev ? E.fm_wdev[0] : 1.f) : 0.f;
  float cs = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const long long ro = rowoff[wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * h];
    if (ro < 0) continue;
    const long long off = ro + col;
    float v = acc[0][0][e] + bias;
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
  if (E.colsum) {
    cs += __shfl_xor(cs, 32);
    if (h == 0) atomicAdd(E.colsum + col, cs);
  }
}

// (x6_a_extent -- the extent of what the A operand's rows may touch -- and x6_tap_ok -- stride-1 conv windows of
// TAPS positions over a halo map image -- live in gemm_common.h: gemm_f16p.hip applies them too)

static bool x6_shape_ok(const f2g_gemm_desc& d) {
  if (d.form != 0 || !host_plain(d.B) || d.A.cols != d.B.cols) return false;
  const long long M = d.A.rows, N = d.B.rows, K = d.A.cols, ext = x6_a_extent(d.A);
  if (K < 32 || (K % 32) || M < 1 || N < 1 || ext <= 0) return false;
  if (ext * 6 >= 0xe0000000ll || N * K * 6 >= 0xe0000000ll) return false;        // 32-bit buffer offsets
  if (d.A.alpha || d.A.lrelu_src || d.B.alpha || d.B.lrelu_src) return false;    // (no on-load transforms)
  if (d.E.c_bf16 || d.E.atomic || d.split_k > 1) return false;
  if (d.E.x3_out) {     // whole 8-element groups of the output on 8-element boundaries of its buffer
    const f2g_epilogue& E = d.E;
    if (E.prelu_out || (((uintptr_t)E.x3_out) & 15) || (((uintptr_t)E.C) & 15) || (N % 8)) return false;
    if (E.P0o > 0 ? ((E.seq_stride_o | E.row_stride_o | E.off_o) & 7) != 0 : (E.ldc & 7) != 0) return false;
  }
  return true;
}

// 1: the launch takes the wide epilogue (x6_epilogue.h; else the generic one + image read-back)
static int x6_wide(const f2g_gemm_desc& d) {
  return x6e::wide_ok(d.E, d.B.rows) ? 1 : 0;
}

// the same descriptor over the fp32 tensors themselves (split = 0): gemm_x6f_kernel
// (B.split = 3: the weight operand as its cached image -- gemm_x6f_kernel<true>; the activation stays fp32)
static bool x6f_ok(const f2g_gemm_desc& d) {
  if (d.A.split || (d.B.split != 0 && d.B.split != 3 && d.B.split != 4) || !x6_shape_ok(d)) return false;
  // (the fragment-major weight image: whole 32-row groups, plain matrix)
  if (d.B.split == 4 && ((d.B.rows & 31) || d.B.rows <= 32 || d.B.P0 != 1 || d.B.P1 != 1)) return false;
  if (!al16(d.A.base) || !al16(d.B.base) || (d.A.seq_stride & 3) || (d.B.split == 0 && (d.B.seq_stride & 3))) return false;
  const long long ext = host_plain(d.A) ? (long long)d.A.rows * d.A.seq_stride : x6_a_extent(d.A);
  return ext * 4 < 0xe0000000ll && (long long)d.B.rows * (d.B.split ? d.B.cols * 6ll : d.B.seq_stride * 4) < 0xe0000000ll;
}

// Which six-product kernel a form-0 descriptor gets: ONE rule for the dispatch below and for the host's query
// (f2g_gemm_colsum_part_rows).  `arg`: the taps of X6_P, WIMG of X6_F.
enum x6_kind {
  X6_NONE,   // precision 3 cannot run the descriptor
  X6_P,      // gemm_x6p_kernel<taps> (gemm_x6p.hip): stride-1 conv windows over images, ping-pong wave groups
  X6_IMG,    // gemm_x6_kernel: three-piece images of both operands
  X6_F,      // gemm_x6f_kernel<wimg>: fp32 activations split inside the kernel, weights fp32 or their cached image
  X6_G,      // gemm_x6g_kernel: ... weights as the fragment-major image (split = 4)
  X6_N       // gemm_x6n_kernel: thin outputs on 128 x 32 tiles (generic epilogue)
};
struct x6_pick {
  x6_kind kind;
  int arg;
};

static x6_pick x6_choose(const f2g_gemm_desc& d) {
  if (x6f_ok(d)) {     // fp32 operands, split inside the kernel
    if (d.B.rows <= 32 && d.B.split == 3 && !d.E.x3_out) return {X6_N, 0};
    if (d.B.split == 4) return {X6_G, 0};
    return {X6_F, d.B.split == 3 ? 1 : 0};
  }
  // fp32-class products from three-piece images (both operands f2g_split_bf16x3 images: split = 3)
  if (d.A.split != 3 || d.B.split != 3 || !x6_shape_ok(d)) return {X6_NONE, 0};
  for (int taps = 5; taps >= 2; taps -= 3)
    if (x6_tap_ok(d, taps) && f2g_x6p_ok(d, taps)) return {X6_P, taps};
  return {X6_IMG, 0};
}

// x6_rows of the A operand; `es` = bytes per element of what the kernel reads: 6 a three-piece image (dense: a plain
// matrix has the row pitch K there), 4 the fp32 tensor itself (its own pitch)
static x6_rows x6_rows_of(const f2g_operand& A, int es) {
  x6_rows R;
  if (host_plain(A)) {
    const long long pitch = es == 6 ? A.cols : A.seq_stride;
    R.P0 = 1, R.seq6 = (unsigned)(pitch * es), R.step6 = 0, R.off6 = 0;
    R.bytes = (unsigned)((long long)A.rows * pitch * es);
  } else {
    R.P0 = A.P0, R.seq6 = (unsigned)(A.seq_stride * es);
    R.step6 = (unsigned)((long long)A.step0 * A.unit * es), R.off6 = (unsigned)(-(long long)A.pad0 * A.unit * es);
    R.bytes = (unsigned)(x6_a_extent(A) * es);
  }
  return R;
}

int f2g_gemm_x6(const f2g_gemm_desc& d, hipStream_t st) {
  const int M = d.A.rows, N = d.B.rows, K = d.A.cols;
  constexpr size_t smem = 2 * 128 * 208;
  const dim3 grid((M + 127) / 128, (N + 127) / 128);
  const x6_pick pick = x6_choose(d);
  switch (pick.kind) {
    case X6_NONE:
      f2g_set_error("f2g_gemm precision 3: form 0 over plain f2g_split_bf16x3 images (split = 3), K % 32 == 0");
      return F2G_EINVAL;
    case X6_P:
      return f2g_launch_x6p(d, pick.arg, x6_a_extent(d.A), st);
    case X6_IMG:
      dyn_lds_once<gemm_x6_kernel>((int)smem);
      f2g_note_kernel("x6", 1, 4);
      hipLaunchKernelGGL(gemm_x6_kernel, grid, dim3(256), smem, st, d, M, N, K, x6_rows_of(d.A, 6), x6_wide(d));
      break;
    case X6_N: {
      constexpr size_t smem_n = (128 + 32) * 208;
      f2g_note_kernel("x6n", 1, 5);      // (its own family in the benchmark's tables: a different kernel on 128 x 32 tiles)
      hipLaunchKernelGGL(gemm_x6n_kernel, dim3((M + 127) / 128), dim3(256), smem_n, st, d, M, N, K, x6_rows_of(d.A, 4));
      break;
    }
    case X6_G: {
      constexpr size_t smem_g = 4 * x6e::ESZ > 128 * 208 ? 4 * x6e::ESZ : 128 * 208;
      f2g_note_kernel("x6g", 1, 4);
      hipLaunchKernelGGL(gemm_x6g_kernel, grid, dim3(256), smem_g, st, d, M, N, K, x6_rows_of(d.A, 4), x6_wide(d));
      break;
    }
    case X6_F:
      dyn_lds_once<gemm_x6f_kernel<false>, gemm_x6f_kernel<true>>((int)smem);
      f2g_note_kernel(pick.arg ? "x6f<wimg=1>" : "x6f<wimg=0>", 1, 4);
      hipLaunchKernelGGL(pick.arg ? gemm_x6f_kernel<true> : gemm_x6f_kernel<false>, grid, dim3(256), smem, st, d, M, N,
                         K, x6_rows_of(d.A, 4), x6_wide(d));
      break;
  }
  return f2g_check_launch();
}

// How f2g_gemm would run this form-0 descriptor at precision 3 -- the SAME tests as its dispatch, E.x3_out
// included (set it before asking).  Bits: 1 = over three-piece images of both operands (split = 3; also
// reported for the fp32 tensors the images would be made of), 2 = and then on a tap-walking instance
// (stride-1 conv windows of 5 or 2 positions), 4 = over the fp32 operands as they are handed over
// (gemm_x6f_kernel: alignment and stride conditions of the in-kernel split).  0 = not at precision 3.
extern "C" int f2g_gemm_x6_ok(const f2g_gemm_desc* d) {
  if (!d || !x6_shape_ok(*d)) return 0;
  return 1 | ((x6_tap_ok(*d, 5) || x6_tap_ok(*d, 2)) ? 2 : 0) | (x6f_ok(*d) ? 4 : 0);
}

// Rows of the partial column-sum matrices (E.colsum_part_ld > 0) the launch of `d` writes: one per 64 output
// rows of whole tiles -- or 0 when the kernel that takes it (x6_choose; at precision 4 the fp16x3 route) has no wide
// epilogue.
extern "C" int32_t f2g_gemm_colsum_part_rows(const f2g_gemm_desc* dp) {
  if (!dp || (dp->precision != 3 && dp->precision != 4) || dp->form != 0) return 0;
  f2g_gemm_desc d = *dp;
  if (d.E.colsum_part_ld <= 0) d.E.colsum_part_ld = 4;          // (alignment of the pointers is the caller's)
  if (d.precision == 4) {      // the fp16x3 kernel the descriptor belongs to says how tall its tiles are (gemm_f16.hip)
    const int tile = f2g_gemm_h3_part_tile(d);
    return tile ? tile / 64 * ((d.A.rows + tile - 1) / tile) : 0;
  }
  if (!x6_wide(d)) return 0;
  const int M = d.A.rows;
  switch (x6_choose(d).kind) {
    case X6_NONE:
    case X6_N:     // (generic epilogue)
      return 0;
    case X6_P:     // 256-row tiles
      return 4 * ((M + 255) / 256);
    default:
      return 2 * ((M + 127) / 128);
  }
}

extern "C" int64_t f2g_split_bf16x3_bytes(int32_t rows, int32_t K) { return (int64_t)rows * K * 6; }

extern "C" int f2g_split_bf16x3(void* dst, const float* src, int64_t ld, int32_t rows, int32_t K,
                                f2g_stream_t stream) {
  if (!dst || !src || rows < 0 || K < 32 || (K % 32) || ld < K || (ld & 3) || (((uintptr_t)src) & 15) ||
      (((uintptr_t)dst) & 15))
    return F2G_EINVAL;
  if (rows == 0) return F2G_OK;
  const long long total = (long long)rows * (K / 4);
  hipLaunchKernelGGL(split3_img_kernel, dim3(f2g_grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<__bf16*>(dst), src, (long long)ld, (long long)rows, K);
  return f2g_check_launch();
}
