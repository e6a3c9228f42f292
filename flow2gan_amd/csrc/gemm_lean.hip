// Lean forward kernel of the implicit-GEMM family (gemm.hip has the family, gemm_common.h what they share).
#include <stddef.h>
#include <stdint.h>

#include "gemm_common.h"

namespace {

// ---- lean forward kernel --------------------------------------------------------------------
// Measured on this part (tools/micro/gemm_lab.hip + PMC): v_mfma_f32_32x32x2_f32 occupies the
// vector ALU for 64 cycles, and with two waves per SIMD keeping that pipe full every OTHER VALU
// instruction issued on the SIMD costs ~37 cycles of it.  The generic loaders (gemm.hip) spend 50-100
// VALU instructions per K slab on addresses, masks and on-load transforms (108 TFLOP/s on the
// 1024-channel MPD layers against 143 for the bare MFMA stream).  This kernel has NO vector
// ALU instruction inside the K loop:
//   * operands are read with buffer_load_dwordx4: resource (base, 2 GiB window) in SGPRs, a
//     per-thread CONSTANT byte offset per staged row (decoded once: sequence / line / position of
//     the im2col row), the K advance in a scalar register (SALU walks the window's segments);
//     rows past the end carry the offset 0x80000000 = out of range = the hardware returns zeros;
//   * LDS addresses are per-thread constants + immediates (K loop unrolled by two);
//   * the next slab is requested before the MFMA phase and written to LDS after it;
//   * the bias enters through the accumulator initialisation.
// It serves form 0 with a row-major B ([n][k] weights) and an A operand whose windows never leave
// their source (plain matrices, and conv windows over buffers that carry their zero padding as
// halo rows): every 1x1 conv, the MPD convs and their data gradients (transposed weights).

__device__ __forceinline__ unsigned lean_row_offset(const f2g_operand& S, int r, int es = 4) {
  if (r >= S.rows) return 0x80000000u;
  long long off;
  if (S.P0 == 1 && S.P1 == 1) {
    off = (long long)r * S.seq_stride;
  } else {
    const int q = r / S.P0, p0 = r - q * S.P0;
    const int sq = q / S.P1, p1 = q - sq * S.P1;
    off = (long long)sq * S.seq_stride + (long long)(p1 * S.step1 - S.pad1) * S.line_stride +
          (long long)(p0 * S.step0 - S.pad0) * S.unit;
  }
  return (unsigned)(off * es);
}

// EP selects the epilogue compiled into an instance (the host picks it from the descriptor): one
// kernel holding all of them needs 256 VGPRs + scratch; each on its own stays near 130-160.
//   0 plain store (+ residual*gamma, leaky ReLU, fused PReLU)   1 PReLU backward (+ column sums)
//   2 row-mapped store (halo layout; + leaky ReLU, or leaky-ReLU backward of the layer below)
//   3 everything else (generic epilogue; the only one stream-K instances use)
// P3 (split-bf16, precision 1): both operands arrive PRE-SPLIT (f2g_split_bf16: every aligned group
// of four floats replaced by its four bf16 high parts and four bf16 remainders, same 16 bytes, same
// addressing), so the K loop stays free of VALU work: a staged 16-byte chunk goes to LDS as two
// 8-byte halves (row = [hi k0..31 | lo k0..31 | pad], the fp32 tile's 144-byte pitch), fragments are
// ds_read_b128 of eight consecutive k, and every product is lo*hi + hi*lo + hi*hi on
// v_mfma_f32_32x32x16_bf16 (24 MFMAs of 32 cycles per wave and slab instead of 64 of 64).
// PM: 0 exact fp32, 1 split-bf16 (three MFMAs per product), 2 plain bf16 = the high parts of the
// same images only (precision 2: one MFMA per product, the lo halves are neither staged nor read),
// 3 plain bf16 over TRUE bf16 tensors (f2g_to_bf16 images / bf16 producers: 2 bytes per element,
// operand strides in elements): the same 128-byte staged row now holds 64 k, so a slab carries
// twice the reduction for the same load, LDS and barrier work (16 MFMAs per wave and slab).
// WM: wave rows of the block = 2 (128 x 128 tile, 4 waves, two blocks per CU) or 4 (256 x 128, 8
// waves, one block per CU).  The bf16 instances are bound by L2 -> CU operand delivery (PMC: 13 TB/s
// of L2 reads on the 1024-channel MPD layer at 128 x 128 = 32 FLOP per byte): the taller tile
// moves a quarter less per FLOP with the same waves per SIMD.
// TAP (split-bf16, 256 x 128 only): A is a stride-1 (taps, 1) conv window over a halo layout
// (win1d, step 1, pad 0).  Tap-major K order makes the plain kernel fetch every activation row once
// per tap; here the rows a tile needs -- its output rows' padded positions plus taps - 1, including
// the halo rows of the sequence ends inside the tile -- are staged ONCE per 32-channel slab and
// the taps walk over them in LDS (a lane's fragment row = its output row's staged row + tap):
// 260-320 staged rows instead of 5 x 256 per channel slab, about half the L2 -> CU traffic of
// the kernel that is bound by exactly that.
// SK: 0 one tile per block, 1 stream-K with atomic seams (linear epilogues, zeroed output).  (A third mode,
// stream-K with a seam FIX-UP through a per-stream workspace, was measured flat under the launch lanes in
// round 4 and removed in round 6: DESIGN.md section 8, "measured and dropped".)
template <int SK, int EP, int PM, int WM = 2, bool TAP = false>
__global__ __launch_bounds__(WM * 128, 4 / WM)
void gemm_lean_kernel(const f2g_gemm_desc d, int M, int N, int K, int kchunk, int upb) {
  constexpr bool P3 = PM == 1 || PM == 2, HI = PM == 2, BF = PM == 3;
  constexpr int BKE = BF ? 64 : BK;   // elements per slab
  constexpr int ES = BF ? 2 : 4;      // bytes per element
  constexpr int BM = 64 * WM, BN = 128, TSZ = BM * LDR, TSB = BN * LDR;
  constexpr int RS = 16 * WM;         // rows staged per pass of the block (32 or 64)
  constexpr int QB = BN / RS;         // passes over the B tile (4 or 2)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, h = lane >> 5;
  // staged row of this thread (of 32, repeated four times 32 rows apart).  The split-bf16 tile is
  // filled with 8-byte stores, served 16 lanes = two rows at a time over 32 banks: rows r and r + 4
  // (4 x 36 dwords = 16 mod 32) share no bank, rows r and r + 1 would share 12 of 16.
  const int ch = tid & 7;
  const int t8 = tid & 255;
  const int rr = (P3 ? (((t8 >> 4) & 3) + 8 * (t8 >> 6) + 4 * ((t8 >> 3) & 1)) : (t8 >> 3)) + 32 * (tid >> 8);
  __amdgpu_buffer_rsrc_t ra =
      __builtin_amdgcn_make_buffer_rsrc((void*)d.A.base, 0, 0x80000000u, 0x00020000);
  // B is a plain [n][k] matrix: the resource ends with its last row, so the rows of a partial
  // last tile (n >= N) are out of range = zeros, and ONE per-thread offset serves all four staged
  // rows (their distance, 32 rows, is uniform and rides in the scalar offset)
  __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
      (void*)d.B.base, 0, (unsigned)((long long)N * d.B.seq_stride * ES), 0x00020000);
  const int qstepB = (int)(RS * d.B.seq_stride * ES);
  // scalar K walk of A: segments of `seglen` columns, `line_stride` floats apart
  const int seglen = d.A.seglen < d.A.cols ? d.A.seglen : d.A.cols;
  const int spseg = seglen / BKE;                                 // slabs per segment
  const int segjump = (int)((d.A.line_stride - seglen) * ES);     // bytes skipped at a segment end
  // LDS: [A buffer 0 | A buffer 1 | B buffer 0 | B buffer 1]; a slab offset `bo` (0 / TSZ) selects the
  // A buffer, the B buffer of the same index lies bo / TSZ * TSB further on
  float* wA = smem + rr * LDR + ch * (P3 ? 2 : 4);
  float* wB = smem + 2 * TSZ + rr * LDR + ch * (P3 ? 2 : 4);
  const float* rA = smem + (wm * 64 + li) * LDR + h * ((P3 || BF) ? 4 : 16);
  const float* rB = smem + 2 * TSZ + (wn * 64 + li) * LDR + h * ((P3 || BF) ? 4 : 16);
  auto bofB = [](int bo) { return WM == 2 ? bo : (bo ? TSB : 0); };

  // ---- work of this block.  Classic: one tile (blockIdx.x/y), K chunk blockIdx.z.  Stream-K
  // (upb > 0): the (tile, slab) units of the whole problem are numbered tile-major and every
  // block takes `upb` consecutive ones -- a tile count just above a multiple of the 512 resident
  // blocks no longer costs a nearly empty extra round; tiles cut between blocks are accumulated
  // atomically onto a zeroed output, bias / residual entering with the part that holds slab 0.
  const int nt_all = K / BKE;
  const int tiles_n = (N + BN - 1) / BN;
  int u = 0, u_end = 0;
  if (SK == 1) {
    const int G = gridDim.x;
    const int q8 = G >> 3, r8 = G & 7, xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int b = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;  // XCD-contiguous
    const int total = ((M + BM - 1) / BM) * tiles_n * nt_all;
    u = b * upb;
    u_end = u + upb < total ? u + upb : total;
    if (u >= u_end) return;
  }
  bool more = true;
  while (more) {
    int m0, n0, s0, nt;
    bool first, partial;
    if (!SK) {
      tile_of_block(BM, BN, m0, n0);
      const int kbeg = blockIdx.z * kchunk;
      int kend = kbeg + kchunk;
      if (kend > K) kend = K;
      s0 = kbeg / BKE;
      nt = (kend - kbeg) / BKE;
      first = blockIdx.z == 0;
      partial = false;
      more = false;
    } else {
      const int tl = u / nt_all;
      s0 = u - tl * nt_all;
      nt = nt_all - s0 < u_end - u ? nt_all - s0 : u_end - u;
      first = s0 == 0;
      partial = nt != nt_all;
      const int tm = tl / tiles_n;
      m0 = tm * BM;
      n0 = (tl - tm * tiles_n) * BN;
      u += nt;
      more = u < u_end;
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int col = n0 + (wn * 2 + ni) * 32 + li;
      // (a scaled result takes its bias in the epilogue: v = acc * scale + bias, as the generic kernels)
      const float b = (d.E.bias && first && col < N && (EP != 3 || d.E.scale == 0.f)) ? d.E.bias[col] : 0.f;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[mi][ni][e] = b;
    }
    if constexpr (TAP) {
      constexpr int RAMAX = 320;                 // staged activation rows per channel slab (host-checked)
      constexpr int TSA = RAMAX * LDR;
      float* sA = smem;                          // [2][RAMAX][LDR]
      float* sB = smem + 2 * TSA;                // [2][128][LDR]
      const int Cin = d.A.unit, taps = d.A.cols / Cin, P0 = d.A.P0;
      const int Hp = (int)(d.A.seq_stride / Cin);
      auto qof = [&](int m) { const int sq = m / P0; return sq * Hp + (m - sq * P0); };
      const int mlast = (m0 + BM < M ? m0 + BM : M) - 1;
      const int qb = qof(m0);
      int rowA[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        int r = m0 + wm * 64 + mi * 32 + li;
        r = r > mlast ? mlast : r;
        rowA[mi] = (qof(r) - qb) * LDR + h * 4;
      }
      const long long a_bytes = (long long)(d.A.rows / P0) * d.A.seq_stride * 4;
      __amdgpu_buffer_rsrc_t rat =
          __builtin_amdgcn_make_buffer_rsrc((void*)d.A.base, 0, (unsigned)a_bytes, 0x00020000);
      unsigned voA[5];
      int wofA[5];
#pragma unroll
      for (int u = 0; u < 5; ++u) {
        const int ci = tid + 512 * u, j = ci >> 3, c8 = ci & 7;
        voA[u] = j < RAMAX ? (unsigned)((long long)j * Cin * 4 + c8 * 16) : 0x80000000u;
        wofA[u] = (j < RAMAX ? j : 0) * LDR + c8 * 2;
      }
      const long long sa0 = (long long)qb * Cin * 4;
      const unsigned offBt = (unsigned)((long long)(n0 + rr) * d.B.seq_stride * 4) + ch * 16;
      float* wBt = sB + rr * LDR + ch * 2;
      const float* rBt = sB + (wn * 64 + li) * LDR + h * 4;
      const int ncs = Cin / BK, nit = ncs * taps;
      auto gloadA = [&](int cs, u32x4 (&ax)[5]) {
        const int so = (int)(sa0 + (long long)cs * BK * 4);
#pragma unroll
        for (int u = 0; u < 5; ++u) ax[u] = __builtin_amdgcn_raw_buffer_load_b128(rat, voA[u], so, 0);
      };
      auto lstoreA = [&](int buf, const u32x4 (&ax)[5]) {
#pragma unroll
        for (int u = 0; u < 5; ++u) {
          if (u < 4 || tid + 512 * 4 < RAMAX * 8) {
            float* p = sA + buf * TSA + wofA[u];
            *reinterpret_cast<u32x2*>(p) = u32x2{ax[u].x, ax[u].y};
            *reinterpret_cast<u32x2*>(p + 16) = u32x2{ax[u].z, ax[u].w};
          }
        }
      };
      auto gloadB = [&](int cs, int tap, u32x4 (&lb)[2]) {
        const int so = (tap * Cin + cs * BK) * 4;
#pragma unroll
        for (int q = 0; q < 2; ++q) lb[q] = __builtin_amdgcn_raw_buffer_load_b128(rb, offBt, so + q * qstepB, 0);
      };
      auto lstoreB = [&](int buf, const u32x4 (&lb)[2]) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          float* p = wBt + buf * TSB + q * RS * LDR;
          *reinterpret_cast<u32x2*>(p) = u32x2{lb[q].x, lb[q].y};
          *reinterpret_cast<u32x2*>(p + 16) = u32x2{lb[q].z, lb[q].w};
        }
      };
      bf16x8 fa0[4], fb0[4], fa1[4], fb1[4];
      auto fragsT = [&](int cs, int tap, int bbuf, int ks, bf16x8 (&fa)[4], bf16x8 (&fb)[4]) {
        const float* pa = sA + (cs & 1) * TSA + tap * LDR + ks * 8;
        const float* pb = rBt + bbuf * TSB + ks * 8;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          fa[i] = *reinterpret_cast<const bf16x8*>(pa + rowA[i]);
          fa[2 + i] = *reinterpret_cast<const bf16x8*>(pa + rowA[i] + 16);
          fb[i] = *reinterpret_cast<const bf16x8*>(pb + i * 32 * LDR);
          fb[2 + i] = *reinterpret_cast<const bf16x8*>(pb + i * 32 * LDR + 16);
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
      // (cs, tap) of iteration it, it + 1 and it + 2, walked with scalar counters
      int cs0 = 0, tp0 = 0, cs1 = 0, tp1 = 1, cs2 = 0, tp2 = 2;
      auto wrap = [&](int& c, int& t) { if (t >= taps) { t -= taps; ++c; } };
      wrap(cs1, tp1);
      wrap(cs2, tp2);
      wrap(cs2, tp2);
      u32x4 xb[2], yb[2], ax[5];
      gloadA(0, ax);
      gloadB(0, 0, xb);
      lstoreA(0, ax);
      lstoreB(0, xb);
      gloadB(cs1, tp1, xb);     // (nit >= 2: taps >= 2)
      if (ncs > 1) gloadA(1, ax);
      __syncthreads();
      fragsT(0, 0, 0, 0, fa0, fb0);
      auto stepT = [&](int it, int cur, int nxt, const u32x4 (&wb)[2], u32x4 (&lb)[2]) {
        fragsT(cs0, tp0, cur, 1, fa1, fb1);
        const bool more2 = it + 2 < nit;
        gloadB(more2 ? cs2 : 0, more2 ? tp2 : 0, lb);
        // the next channel slab's rows: requested at tap 0 (the prologue did it for slab 1), stored
        // at tap 2 into the buffer slab cs - 1 has left two barriers ago
        if (tp0 == 0 && cs0 > 0 && cs0 + 1 < ncs) gloadA(cs0 + 1, ax);
        mfma12(fa0, fb0);
        lstoreB(nxt, wb);
        if (tp0 == (taps > 2 ? 2 : taps - 1) && cs0 + 1 < ncs) lstoreA((cs0 + 1) & 1, ax);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        fragsT(cs1, tp1, nxt, 0, fa0, fb0);
        mfma12(fa1, fb1);
        __builtin_amdgcn_sched_barrier(0);
        cs0 = cs1; tp0 = tp1; cs1 = cs2; tp1 = tp2;
        ++tp2;
        wrap(cs2, tp2);
      };
      int it = 0;
      for (; it + 1 < nit; it += 2) {
        stepT(it, 0, 1, xb, yb);
        stepT(it + 1, 1, 0, yb, xb);
      }
      if (it < nit) stepT(it, 0, 1, xb, yb);
    } else {
    unsigned offA[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      offA[q] = lean_row_offset(d.A, m0 + rr + RS * q, ES);
      if (offA[q] != 0x80000000u) offA[q] += ch * 16;
    }
    const unsigned offB = (unsigned)((long long)(n0 + rr) * d.B.seq_stride * ES) + ch * 16;
    int left = spseg - (s0 % spseg);
    const int ka0 = (int)(((long long)(s0 / spseg) * d.A.line_stride + (long long)(s0 % spseg) * BKE) * ES);
    const int kb0 = s0 * BKE * ES;
    int ka = ka0, kb = kb0;

    auto gload = [&](int soa, int sob, u32x4 (&la)[4], u32x4 (&lb)[4]) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        la[q] = __builtin_amdgcn_raw_buffer_load_b128(ra, offA[q], soa, 0);
        if (q < QB) lb[q] = __builtin_amdgcn_raw_buffer_load_b128(rb, offB, sob + q * qstepB, 0);
      }
    };
    auto lstore = [&](int bufoff, const u32x4 (&la)[4], const u32x4 (&lb)[4]) {
      const int bb = bofB(bufoff);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if constexpr (P3) {
          *reinterpret_cast<u32x2*>(wA + bufoff + q * RS * LDR) = u32x2{la[q].x, la[q].y};
          if constexpr (!HI)
            *reinterpret_cast<u32x2*>(wA + bufoff + q * RS * LDR + 16) = u32x2{la[q].z, la[q].w};
          if (q < QB) {
            *reinterpret_cast<u32x2*>(wB + bb + q * RS * LDR) = u32x2{lb[q].x, lb[q].y};
            if constexpr (!HI)
              *reinterpret_cast<u32x2*>(wB + bb + q * RS * LDR + 16) = u32x2{lb[q].z, lb[q].w};
          }
        } else {
          *reinterpret_cast<u32x4*>(wA + bufoff + q * RS * LDR) = la[q];
          if (q < QB) *reinterpret_cast<u32x4*>(wB + bb + q * RS * LDR) = lb[q];
        }
      }
    };
    auto mfma_slab = [&](int bufoff) {
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        float4 a[2], b[2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
          a[mi] = *reinterpret_cast<const float4*>(rA + bufoff + mi * 32 * LDR + s4 * 4);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          b[ni] = *reinterpret_cast<const float4*>(rB + bofB(bufoff) + ni * 32 * LDR + s4 * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
              const float av = q == 0 ? a[mi].x : q == 1 ? a[mi].y : q == 2 ? a[mi].z : a[mi].w;
              const float bv = q == 0 ? b[ni].x : q == 1 ? b[ni].y : q == 2 ? b[ni].z : b[ni].w;
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[mi][ni], 0, 0, 0);
            }
      }
    };
    // (SALU) K offsets of the slab after the current one
    auto advance = [&]() {
      ka += BK * 4;
      kb += BK * 4;
      if (--left == 0) {
        left = spseg;
        ka += segjump;
      }
    };
    if constexpr (P3 || BF) {
      // The bf16 MFMA phase of a slab is 5x shorter than the fp32 one (24 x 32 cycles), too short to
      // hide a load, an LDS fill and a barrier behind it one after the other.  So the phases overlap
      // inside a wave: slab t's MFMAs are interleaved with the LDS stores of slab t+1 (in registers
      // since the previous iteration) while the loads of slab t+2 fly -- two register stages.
      u32x4 xa[4], xb[4], ya[4], yb[4];
      if (nt > 0) {
        gload(ka, kb, xa, xb);
        lstore(0, xa, xb);
      }
      advance();
      gload(nt > 1 ? ka : ka0, nt > 1 ? kb : kb0, xa, xb);
      __syncthreads();
      // fragments: f0 = first k step (8 consecutive k per lane half), f1 = second; [0..1] = hi of
      // the two sub-tiles, [2..3] = lo.  f0 of the NEXT slab is read right after the barrier, under
      // the MFMAs of f1; f1 is read at the top of an iteration, under the MFMAs of f0.
      bf16x8 fa0[4], fb0[4], fa1[4], fb1[4];
      auto frags = [&](int off, int ks, bf16x8 (&fa)[4], bf16x8 (&fb)[4]) {
        if constexpr (BF) {   // half `ks` of the slab = k steps 2ks, 2ks+1: [0..1] and [2..3]
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
              fa[2 * j + i] = *reinterpret_cast<const bf16x8*>(rA + off + i * 32 * LDR + (2 * ks + j) * 8);
              fb[2 * j + i] = *reinterpret_cast<const bf16x8*>(rB + bofB(off) + i * 32 * LDR + (2 * ks + j) * 8);
            }
          return;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          fa[i] = *reinterpret_cast<const bf16x8*>(rA + off + i * 32 * LDR + ks * 8);
          fb[i] = *reinterpret_cast<const bf16x8*>(rB + bofB(off) + i * 32 * LDR + ks * 8);
          if constexpr (!HI) {
            fa[2 + i] = *reinterpret_cast<const bf16x8*>(rA + off + i * 32 * LDR + ks * 8 + 16);
            fb[2 + i] = *reinterpret_cast<const bf16x8*>(rB + bofB(off) + i * 32 * LDR + ks * 8 + 16);
          }
        }
      };
      f32x16 shadow[2][2];   // (lab, F2G_LABVAR & 16: second accumulator set -> twice the dependent distance)
      if (F2G_LABVAR & 16) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) shadow[mi][ni][e] = 0.f;
      }
      auto mfma12 = [&](const bf16x8 (&fa)[4], const bf16x8 (&fb)[4]) {
        if constexpr (BF) {
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
              for (int ni = 0; ni < 2; ++ni)
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[2 * j + mi], fb[2 * j + ni],
                                                                     acc[mi][ni], 0, 0, 0);
          return;
        }
#pragma unroll
        for (int term = HI ? 2 : 0; term < 3; ++term)
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
              const bf16x8 av = term == 0 ? fa[2 + mi] : fa[mi];
              const bf16x8 bv = term == 1 ? fb[2 + ni] : fb[ni];
              if ((F2G_LABVAR & 16) && term == 1)
                shadow[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, shadow[mi][ni], 0, 0, 0);
              else
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[mi][ni], 0, 0, 0);
            }
      };
      frags(0, 0, fa0, fb0);
      auto step3 = [&](int t, int curoff, int nxtoff, const u32x4 (&wa)[4], const u32x4 (&wb)[4],
                       u32x4 (&la)[4], u32x4 (&lb)[4]) {
        if (!(F2G_LABVAR & 8)) frags(curoff, 1, fa1, fb1);
        advance();
        const bool again = t + 2 < nt;   // past the end: re-read the first slab (never used)
        if (!(F2G_LABVAR & 1)) gload(again ? ka : ka0, again ? kb : kb0, la, lb);
        mfma12(fa0, fb0);
        if (!(F2G_LABVAR & 2)) lstore(nxtoff, wa, wb);
        // issue order: fragments, the loads of the slab after next, one LDS store behind each of
        // the first MFMAs
        constexpr int NM = HI ? 4 : (BF ? 8 : 12);        // MFMAs per half slab
        constexpr int NW = 4 + QB;                        // LDS store instructions per slab
        constexpr int WPM = (NW + NM - 1) / NM;
        __builtin_amdgcn_sched_group_barrier(0x100, HI ? 4 : 8, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 4 + QB, 0);
#pragma unroll
        for (int i = 0; i < NM; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          if (i * WPM < NW) __builtin_amdgcn_sched_group_barrier(0x200, WPM, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (!(F2G_LABVAR & 4)) __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        if (!(F2G_LABVAR & 8)) frags(nxtoff, 0, fa0, fb0);
        mfma12(fa1, fb1);
        __builtin_amdgcn_sched_group_barrier(0x100, HI ? 4 : 8, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, HI ? 4 : (BF ? 8 : 12), 0);
        __builtin_amdgcn_sched_barrier(0);
      };
      int t = 0;
      for (; t + 1 < nt; t += 2) {
        step3(t, 0, TSZ, xa, xb, ya, yb);
        step3(t + 1, TSZ, 0, ya, yb, xa, xb);
      }
      if (t < nt) step3(t, 0, TSZ, xa, xb, ya, yb);
      if (F2G_LABVAR & 16) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][ni][e] += shadow[mi][ni][e];
      }
    } else {
    if (nt > 0) {
      u32x4 la[4], lb[4];
      gload(ka, kb, la, lb);
      lstore(0, la, lb);
    }
    __syncthreads();
    auto step = [&](int t, int curoff, int nxtoff) {
      u32x4 la[4], lb[4];
      advance();
      const bool again = t + 1 < nt;   // the last iteration re-reads the first slab (never used)
      gload(again ? ka : ka0, again ? kb : kb0, la, lb);
      __builtin_amdgcn_sched_barrier(0);
      mfma_slab(curoff);
      __builtin_amdgcn_sched_barrier(0);
      lstore(nxtoff, la, lb);
      __syncthreads();
    };
    int t = 0;
    for (; t + 1 < nt; t += 2) {
      step(t, 0, TSZ);
      step(t + 1, TSZ, 0);
    }
    if (t < nt) {
      step(t, 0, TSZ);
      // an odd slab count leaves the (unused) restaged slab in buffer 1; the next segment starts in
      // buffer 0, which every wave has finished reading (barrier above)
    }

    }

    }
    const int li_e = li, h_e = h;
    const f2g_epilogue& E = d.E;
    const bool simple = !partial && !E.aux && !E.colsum && !E.colsum_alpha && E.P0o == 0 &&
                        !E.atomic && !E.accumulate && E.scale == 0.f && !E.mask_src;
    (void)simple;
    if constexpr (EP == 0) {
      // plain store (+ leaky ReLU / PReLU): uniform row bases, per-lane constant offset
      const float sl = E.lrelu_slope;
      const bool pre = E.prelu_slope != nullptr, two = pre && E.prelu_out != nullptr;
      const bool cbf = E.c_bf16 != 0;
      const unsigned coff = (unsigned)(((long long)(4 * h_e) * E.ldc + li_e) * 4);
      const unsigned poff = (unsigned)(((long long)(4 * h_e) * E.ld_prelu_out + li_e) * 4);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          const int col0 = n0 + (wn * 2 + ni) * 32;
          const int row0 = m0 + (wm * 2 + mi) * 32;
          const float ps = (pre && col0 + li_e < N) ? E.prelu_slope[col0 + li_e] : 0.f;
          const bool hasres = E.res != nullptr;
          const float gam = (hasres && col0 + li_e < N) ? (E.gamma ? E.gamma[col0 + li_e] : 1.f) : 0.f;
          if (row0 + 32 <= M && col0 + 32 <= N) {
            char* cb = reinterpret_cast<char*>(E.C + (long long)row0 * E.ldc + col0);
            __bf16* cb16 = reinterpret_cast<__bf16*>(E.C) + (long long)row0 * E.ldc + col0;
            char* pb = reinterpret_cast<char*>(E.prelu_out + (long long)row0 * E.ld_prelu_out + col0);
            const char* rb = reinterpret_cast<const char*>(E.res + (long long)row0 * E.ldres + col0);
            const unsigned roff = (unsigned)(((long long)(4 * h_e) * E.ldres + li_e) * 4);
            float rv[16];
            if (hasres) {   // all 16 residual values requested before any is consumed
#pragma unroll
              for (int e = 0; e < 16; ++e)
                rv[e] = *reinterpret_cast<const float*>(rb + (long long)((e & 3) + 8 * (e >> 2)) * E.ldres * 4 + roff);
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              float v = acc[mi][ni][e];
              if (hasres) v += gam * rv[e];
              if (sl != 0.f) v = fmaxf(v, 0.f) + sl * fminf(v, 0.f);
              const long long ro = (e & 3) + 8 * (e >> 2);
              if (pre) {
                const float pv = fmaxf(v, 0.f) + ps * fminf(v, 0.f);
                if (two) *reinterpret_cast<float*>(pb + ro * E.ld_prelu_out * 4 + poff) = pv;
                else v = pv;
              }
              if (cbf)   // C is a bf16 tensor (ldc in elements): the next GEMM's operand as it is
                cb16[(ro + 4 * h_e) * E.ldc + li_e] = (__bf16)v;
              else
                *reinterpret_cast<float*>(cb + ro * E.ldc * 4 + coff) = v;
            }
            __builtin_amdgcn_sched_barrier(0);   // one sub-tile's loads / stores at a time (registers)
          } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int row = row0 + (e & 3) + 8 * (e >> 2) + 4 * h_e;
              float v = acc[mi][ni][e];
              if (hasres && row < M && col0 + li_e < N) v += gam * E.res[(long long)row * E.ldres + col0 + li_e];
              if (sl != 0.f) v = fmaxf(v, 0.f) + sl * fminf(v, 0.f);
              if (row < M && col0 + li_e < N) {
                if (pre) {
                  const float pv = fmaxf(v, 0.f) + ps * fminf(v, 0.f);
                  if (two) E.prelu_out[(long long)row * E.ld_prelu_out + col0 + li_e] = pv;
                  else v = pv;
                }
                if (cbf) reinterpret_cast<__bf16*>(E.C)[(long long)row * E.ldc + col0 + li_e] = (__bf16)v;
                else E.C[(long long)row * E.ldc + col0 + li_e] = v;
              }
            }
          }
        }
    } else if constexpr (EP == 1) {
      // PReLU backward fused into the data gradient (modules.py:444,488 backward):
      //   v = acc * (a > 0 ? 1 : alpha[n]);  d alpha[n] += sum_r acc * min(a, 0);  d bias[n] += sum_r v
      // plain store (C may alias aux: each element is read before it is written by the same lane)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int col = n0 + (wn * 2 + ni) * 32 + li_e;
        const bool cok = col < N;
        const float aln = cok ? E.alpha_n[col] : 0.f;
        float cs = 0.f, csa = 0.f;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
          const int row0 = m0 + (wm * 2 + mi) * 32 + 4 * h_e;
          const bool full = cok && row0 - 4 * h_e + 32 <= M;
          const float* ab = E.aux + (long long)row0 * E.ldaux + col;
          float* cb = E.C + (long long)row0 * E.ldc + col;
#pragma unroll
          for (int e4 = 0; e4 < 4; ++e4) {           // four rows (r, r+1, r+2, r+3) at a time
            float av[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int r = 8 * e4 + k;
              av[k] = (full || (cok && row0 + r < M)) ? ab[(long long)r * E.ldaux] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int r = 8 * e4 + k;
              const float a0 = acc[mi][ni][e4 * 4 + k];
              csa += a0 * fminf(av[k], 0.f);
              const float v = a0 * (av[k] > 0.f ? 1.f : aln);
              if (full || (cok && row0 + r < M)) {
                cs += v;
                cb[(long long)r * E.ldc] = v;
              }
            }
          }
        }
        if (E.colsum || E.colsum_alpha) {
          cs += __shfl_xor(cs, 32);
          csa += __shfl_xor(csa, 32);
          if (cok && h_e == 0) {
            if (E.colsum) atomicAdd(E.colsum + col, cs);
            if (E.colsum_alpha) atomicAdd(E.colsum_alpha + col, csa);
          }
        }
      }
    } else if constexpr (EP == 2) {
      // row-mapped store: the halo layout of the MPD maps and the stride residues of their data
      // gradients.  One division per 32-row sub-tile instead of one per element (the 32 rows of a
      // sub-tile wrap the sequence length (>= 32) at most once).  Options: leaky ReLU (forward), or
      // the leaky-ReLU backward of the layer below (+ feature-matching term) with the column sums
      // of the result = that layer's bias gradient.
      const float sl = E.lrelu_slope;
      const bool msk = E.mask_src != nullptr, fm = E.fm_ref != nullptr;
      const float fmw = fm ? E.fm_w * (E.fm_wdev ? E.fm_wdev[0] : 1.f) : 0.f;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int col = n0 + (wn * 2 + ni) * 32 + li_e;
        const bool cok = col < N;
        float cs = 0.f;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
          const int row0 = m0 + (wm * 2 + mi) * 32;
          const int q0 = row0 / E.P0o;                         // uniform
          const int p0 = row0 - q0 * E.P0o + 4 * h_e;            // position of this lane's first row
          const long long cbase = E.off_o + col;
#pragma unroll
          for (int e4 = 0; e4 < 4; ++e4) {
            long long off[4];
            bool ok[4];
            float yv[4], rv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int re = 8 * e4 + k;
              int p = p0 + re, q = q0;
              if (p >= E.P0o) { p -= E.P0o; ++q; }
              ok[k] = cok && row0 + re + 4 * h_e < M;
              off[k] = cbase + (long long)q * E.seq_stride_o + (long long)p * E.row_stride_o;
              if (msk) yv[k] = ok[k] ? E.mask_src[off[k]] : 0.f;
              if (fm) rv[k] = ok[k] ? E.fm_ref[off[k]] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              float v = acc[mi][ni][e4 * 4 + k];
              if (sl != 0.f) v = fmaxf(v, 0.f) + sl * fminf(v, 0.f);
              if (msk) {
                if (fm) {
                  const float dl = yv[k] - rv[k];
                  v += fmw * (dl > 0.f ? 1.f : (dl < 0.f ? -1.f : 0.f));
                }
                v *= yv[k] > 0.f ? 1.f : E.mask_slope;
              }
              if (ok[k]) {
                cs += v;
                E.C[off[k]] = v;
              }
            }
            asm volatile("" ::: "memory");   // four rows at a time: keeps the next group's loads
            __builtin_amdgcn_sched_barrier(0);   // from being hoisted (register pressure)
          }
        }
        if (E.colsum) {
          cs += __shfl_xor(cs, 32);
          if (cok && h_e == 0) atomicAdd(E.colsum + col, cs);
        }
      }
    } else {
      f2g_epilogue E2 = E;
      if (E.scale == 0.f) E2.bias = nullptr;   // already in the accumulators
      if (partial) { E2.atomic = 1; E2.accumulate = 0; }
      gemm_epilogue<2, 2>(E2, acc, M, N, m0, n0, wm, wn, li_e, h_e, first);
    }
  }
}

// Can `S` (the A operand of a form-0 GEMM) be read by the lean kernel: aligned, no on-load
// transform, reduction in whole 32-column slabs per segment, and every window inside its source?
inline bool lean_a_ok(const f2g_operand& S) {
  if (S.reflect || S.alpha || S.lrelu_src || S.rows <= 0 || S.cols < BK) return false;
  if (!al16(S.base) || (S.seq_stride & 3) || (S.line_stride & 3)) return false;
  const long long eu0 = (long long)S.step0 * S.unit, ep0 = (long long)S.pad0 * S.unit;
  if ((eu0 & 3) || (ep0 & 3)) return false;
  const int seglen = S.seglen < S.cols ? S.seglen : S.cols;
  if (seglen % BK || S.cols % seglen) return false;
  const int nseg = S.cols / seglen;
  if (S.P0 < 1 || S.P1 < 1) return false;
  if (S.rows % (S.P0 * S.P1)) return false;
  // line range
  if (S.pad1 > 0 || (long long)(S.P1 - 1) * S.step1 - S.pad1 + nseg - 1 >= S.L1) return false;
  // element range inside a line
  if (S.pad0 > 0 || ((long long)(S.P0 - 1) * S.step0 - S.pad0) * S.unit + seglen > S.L0u) return false;
  if (nseg > 1 && S.line_stride < seglen) return false;
  // byte offsets must stay below 2 GiB
  const long long nseq = S.rows / (S.P0 * S.P1);
  const long long last = (nseq - 1) * S.seq_stride + (long long)(S.L1 - 1) * S.line_stride + S.L0u;
  return last * 4 < 0x7ff00000ll;
}

// A as a stride-1 conv window whose rows a 256-row tile can stage once per channel slab (TAP mode)
inline bool lean_tap_ok(const f2g_operand& A) {
  if (A.P1 != 1 || A.step0 != 1 || A.pad0 != 0 || A.unit < BK || A.unit % BK) return false;
  if (A.cols % A.unit || A.cols / A.unit < 2 || A.seglen < A.cols || A.seq_stride % A.unit) return false;
  const int taps = A.cols / A.unit, Hp = (int)(A.seq_stride / A.unit);
  if (A.P0 < 8 || Hp < A.P0 + taps - 1) return false;
  return 256 + taps - 1 + (Hp - A.P0) * (256 / A.P0 + 1) <= 320;
}

// the same operand as a TRUE bf16 tensor (split = 2): 16-byte chunks hold 8 elements, slabs 64
inline bool lean_bf16_ok(const f2g_operand& A, const f2g_operand& B) {
  const long long eu0 = (long long)A.step0 * A.unit, ep0 = (long long)A.pad0 * A.unit;
  if ((A.seq_stride & 7) || (A.line_stride & 7) || (eu0 & 7) || (ep0 & 7) || (B.seq_stride & 7)) return false;
  const int seglen = A.seglen < A.cols ? A.seglen : A.cols;
  return seglen % 64 == 0 && B.cols % 64 == 0;
}

inline bool lean_b_ok(const f2g_operand& S) {
  return host_plain(S) && !S.alpha && al16(S.base) && (S.seq_stride & 3) == 0 && S.cols % BK == 0 &&
         (long long)S.rows * S.seq_stride * 4 < 0x7ff00000ll;
}

}  // namespace

bool f2g_lean_operands_ok(const f2g_gemm_desc& d) { return lean_a_ok(d.A) && lean_b_ok(d.B); }

bool f2g_lean_bf16_ok(const f2g_gemm_desc& d) { return lean_bf16_ok(d.A, d.B); }

int f2g_launch_lean(const f2g_gemm_desc& d, int M, int N, int K, int split, int upb, hipStream_t st) {
  // operand images: split = 1 -> split-bf16 pairs (precision 1: all three products, 2: high parts),
  // split = 2 -> true bf16 tensors (precision 2 only)
  const int pm = d.A.split == 2 ? 3 : (d.precision == 1 ? 1 : (d.precision == 2 ? 2 : 0));
  const int bk = pm == 3 ? 64 : BK;
  int kchunk = ((K + split - 1) / split + bk - 1) / bk * bk;
  int zs = (K + kchunk - 1) / kchunk;
  // 256 x 128 tiles (8 waves) for the bf16 instances when the taller grid still fills the chip
  // and the reduction is long enough to amortise the larger prologue / epilogue (measured: +11 % on
  // the 1024-channel MPD layers, -7 % at K = 384 / 512)
  // (option lean_tall: 0 never, 1 when K >= 640 and there are >= 400 tall tiles, 2 whenever possible)
  const int tall_mode = f2g_opt(F2G_OPT_LEAN_TALL);
  const long long tall_tiles = (long long)((M + 255) / 256) * ((N + 127) / 128);
  const bool tall = (pm == 1 || pm == 3) && upb == 0 && zs == 1 && tall_mode > 0 &&
                    (tall_mode > 1 || (tall_tiles >= 400 && K >= 640));
  const int bm = tall ? 256 : 128;
  // tap-reusing variant for stride-1 conv windows
  const bool tap = tall && pm == 1 && lean_tap_ok(d.A);
  const size_t smem = tap ? (size_t)(2 * 320 + 2 * 128) * LDR * sizeof(float)
                          : (size_t)(2 * bm + 2 * 128) * LDR * sizeof(float);
  dim3 grid((M + bm - 1) / bm, (N + 127) / 128, zs);
  if (grid.x == 0 || grid.y == 0) return F2G_OK;
  if (upb > 0) {
    const long long total = (long long)grid.x * grid.y * (K / bk);
    grid = dim3((unsigned)((total + upb - 1) / upb), 1, 1);
  }
  // epilogue instance (see gemm_lean_kernel)
  const f2g_epilogue& E = d.E;
  int ep = 3;
  if (upb == 0) {
    const bool plainish = !E.aux && !E.colsum_alpha && !E.atomic && !E.accumulate && E.scale == 0.f;
    if (plainish && !E.colsum && E.P0o == 0 && !E.mask_src) ep = 0;
    else if (E.aux && !E.res && E.P0o == 0 && !E.atomic && !E.accumulate && E.scale == 0.f &&
             !E.prelu_slope && E.lrelu_slope == 0.f && !E.mask_src) ep = 1;
    else if (plainish && !E.res && !E.prelu_slope && E.P0o >= 32) ep = 2;
  }
  if (E.c_bf16 && ep != 0) {
    f2g_set_error("f2g_gemm: a bf16 output needs the plain-store epilogue of the lean kernel");
    return F2G_EINVAL;
  }
  dyn_lds_once<gemm_lean_kernel<2, 0, 0>, gemm_lean_kernel<2, 1, 0>, gemm_lean_kernel<2, 2, 0>,
               gemm_lean_kernel<2, 3, 0>, gemm_lean_kernel<false, 0, 0>, gemm_lean_kernel<false, 1, 0>,
               gemm_lean_kernel<false, 2, 0>, gemm_lean_kernel<false, 3, 0>, gemm_lean_kernel<true, 3, 0>,
               gemm_lean_kernel<false, 0, 1>, gemm_lean_kernel<false, 1, 1>, gemm_lean_kernel<false, 2, 1>,
               gemm_lean_kernel<false, 3, 1>, gemm_lean_kernel<true, 3, 1>, gemm_lean_kernel<false, 0, 2>,
               gemm_lean_kernel<false, 1, 2>, gemm_lean_kernel<false, 2, 2>, gemm_lean_kernel<false, 3, 2>,
               gemm_lean_kernel<true, 3, 2>, gemm_lean_kernel<false, 0, 3>, gemm_lean_kernel<false, 1, 3>,
               gemm_lean_kernel<false, 2, 3>, gemm_lean_kernel<false, 3, 3>,
               gemm_lean_kernel<true, 3, 3>>(4 * 128 * LDR * 4);
  dyn_lds_once<gemm_lean_kernel<false, 0, 1, 4>, gemm_lean_kernel<false, 1, 1, 4>,
               gemm_lean_kernel<false, 2, 1, 4>, gemm_lean_kernel<false, 3, 1, 4>,
               gemm_lean_kernel<false, 0, 3, 4>, gemm_lean_kernel<false, 1, 3, 4>,
               gemm_lean_kernel<false, 2, 3, 4>,
               gemm_lean_kernel<false, 3, 3, 4>>((2 * 256 + 2 * 128) * LDR * 4);
  dyn_lds_once<gemm_lean_kernel<false, 2, 1, 4, true>,
               gemm_lean_kernel<false, 3, 1, 4, true>>((2 * 320 + 2 * 128) * LDR * 4);
  {
    static const char* const flat[4][4] = {
        {"lean<sk=0,ep=0,pm=0>", "lean<sk=0,ep=0,pm=1>", "lean<sk=0,ep=0,pm=2>", "lean<sk=0,ep=0,pm=3>"},
        {"lean<sk=0,ep=1,pm=0>", "lean<sk=0,ep=1,pm=1>", "lean<sk=0,ep=1,pm=2>", "lean<sk=0,ep=1,pm=3>"},
        {"lean<sk=0,ep=2,pm=0>", "lean<sk=0,ep=2,pm=1>", "lean<sk=0,ep=2,pm=2>", "lean<sk=0,ep=2,pm=3>"},
        {"lean<sk=0,ep=3,pm=0>", "lean<sk=0,ep=3,pm=1>", "lean<sk=0,ep=3,pm=2>", "lean<sk=0,ep=3,pm=3>"}};
    static const char* const sk[4] = {"lean<sk=1,ep=3,pm=0>", "lean<sk=1,ep=3,pm=1>", "lean<sk=1,ep=3,pm=2>",
                                      "lean<sk=1,ep=3,pm=3>"};
    static const char* const tl[4][2] = {{"lean_tall<ep=0,pm=1>", "lean_tall<ep=0,pm=3>"},
                                         {"lean_tall<ep=1,pm=1>", "lean_tall<ep=1,pm=3>"},
                                         {"lean_tall<ep=2,pm=1>", "lean_tall<ep=2,pm=3>"},
                                         {"lean_tall<ep=3,pm=1>", "lean_tall<ep=3,pm=3>"}};
    static const char* const tp[2] = {"lean_tap<ep=2>", "lean_tap<ep=3>"};
    // (the same selection as the launches below)
    const char* name = tap && (ep == 2 || ep == 3) ? tp[ep - 2]
                       : tall                      ? tl[ep][pm == 1 ? 0 : 1]
                       : upb > 0                   ? sk[pm]
                                                   : flat[ep][pm];
    f2g_note_kernel(name, split, upb > 0 ? 2 : 1);
  }
#define F2G_LEAN(SKV, EPV)                                                                        \
  do {                                                                                            \
    if (pm == 1)                                                                                  \
      hipLaunchKernelGGL((gemm_lean_kernel<SKV, EPV, 1>), grid, dim3(256), smem, st, d, M, N, K,  \
                         kchunk, upb);                                                         \
    else if (pm == 2)                                                                             \
      hipLaunchKernelGGL((gemm_lean_kernel<SKV, EPV, 2>), grid, dim3(256), smem, st, d, M, N, K,  \
                         kchunk, upb);                                                         \
    else if (pm == 3)                                                                             \
      hipLaunchKernelGGL((gemm_lean_kernel<SKV, EPV, 3>), grid, dim3(256), smem, st, d, M, N, K,  \
                         kchunk, upb);                                                         \
    else                                                                                          \
      hipLaunchKernelGGL((gemm_lean_kernel<SKV, EPV, 0>), grid, dim3(256), smem, st, d, M, N, K,  \
                         kchunk, upb);                                                         \
  } while (0)
#define F2G_LEAN_T(EPV)                                                                           \
  do {                                                                                            \
    if (pm == 1)                                                                                  \
      hipLaunchKernelGGL((gemm_lean_kernel<false, EPV, 1, 4>), grid, dim3(512), smem, st, d, M,   \
                         N, K, kchunk, upb);                                                   \
    else                                                                                          \
      hipLaunchKernelGGL((gemm_lean_kernel<false, EPV, 3, 4>), grid, dim3(512), smem, st, d, M,   \
                         N, K, kchunk, upb);                                                   \
  } while (0)
  if (tap && (ep == 2 || ep == 3)) {
    if (ep == 2)
      hipLaunchKernelGGL((gemm_lean_kernel<false, 2, 1, 4, true>), grid, dim3(512), smem, st, d, M, N, K,
                         kchunk, upb);
    else
      hipLaunchKernelGGL((gemm_lean_kernel<false, 3, 1, 4, true>), grid, dim3(512), smem, st, d, M, N, K,
                         kchunk, upb);
  } else if (tall) {
    if (ep == 0) F2G_LEAN_T(0);
    else if (ep == 1) F2G_LEAN_T(1);
    else if (ep == 2) F2G_LEAN_T(2);
    else F2G_LEAN_T(3);
  } else
  if (upb > 0) F2G_LEAN(true, 3);
  else if (ep == 0) F2G_LEAN(false, 0);
  else if (ep == 1) F2G_LEAN(false, 1);
  else if (ep == 2) F2G_LEAN(false, 2);
  else F2G_LEAN(false, 3);
#undef F2G_LEAN
#undef F2G_LEAN_T
  return f2g_check_launch();
}

// Stream-K decision for the lean kernel: units per block, or 0 to keep the classic tile grid.
// Measured on the stage-2 step (B = 64): evening out the rounds lifts the kernels alone on the chip
// (GEMM class 283.8 -> 275.4 ms serialised) but not the step itself, whose launch lanes already
// fill one kernel's idle CUs with another lane's work (266.5 -> 269.0 ms: the zero fill and the
// atomic epilogues remain).  Default: only the latency regime (fewer tiles than half the CUs:
// batch-1 chunked synthesis, the per-item MLPs), where nothing else runs beside the kernel;
// option streamk = 2 applies it to every ragged tile grid.
int f2g_lean_stream_k(int M, int N, int K, bool all_grids) {
  const long long tiles = (long long)((M + 127) / 128) * ((N + 127) / 128);
  const int nt = K / BK;
  if (nt < 16) return 0;
  const long long total = tiles * nt;
  if (tiles * 2 > 256) {
    if (!all_grids) return 0;
    const double rounds = (double)tiles / 512.0;
    const double eff = rounds / (double)((tiles + 511) / 512);
    if (eff > 0.9) return 0;                     // the tile grid already fills its rounds
  }
  long long upb = (total + 511) / 512;
  const int min_slabs = f2g_opt(F2G_OPT_STREAMK_MIN);      // (default 4; 8 until round 6: 64-row time-path GEMMs 54 -> 44 us)
  if (upb < min_slabs) upb = min_slabs;
  return (int)upb;
}

// Would f2g_gemm run this form-0 descriptor on the lean kernel (whatever its precision)?  The host
// asks before it pre-splits the operands of a split-bf16 GEMM.
extern "C" int f2g_gemm_lean_ok(const f2g_gemm_desc* dp) {
  if (!dp || !dp->A.base || !dp->B.base) return 0;
  const f2g_gemm_desc& d = *dp;
  if (d.form == 2) return f2g_leanw_ok(d) ? 1 : 0;   // split-bf16 weight-gradient kernel
  if (d.form != 0) return 0;
  if (d.A.cols != d.B.cols || !host_plain(d.B)) return 0;
  if (!(d.B.rows > 64 && lean_a_ok(d.A) && lean_b_ok(d.B))) return 0;
  return lean_bf16_ok(d.A, d.B) ? 3 : 1;   // bit 1: also as true bf16 tensors (split = 2)
}
