// fp16x3 over STRIDE-1 conv windows of two or one positions of a halo map with 128 CHANNELS onto N <= 32 output
// columns (the three stride-residue data gradients of the MPD's 32 -> 128 layer, K = 256 / 256 / 128 -- what
// gemm_x6n_kernel runs in the bf16x6 mode), SCALED INSIDE THE KERNEL: the A operand is the fp32 map itself
// (f2g_operand.split = 8), there is no image pass and no rscale.  gemm_f16p.hip has the arithmetic and the error bound
// of the tap-walking family, gemm_f16p3n.hip the segment scale; gemm_h3pn_kernel<TAPS = 2, 1> are the instances.
//
// SEGMENTS.  A tile is 128 output rows x all N columns, four waves of 32 x 32 as gemm_x6n_kernel.  Its rows belong to
// 1 .. 17 sequences (P0 >= 8); the positions the rows of ONE sequence read are a contiguous run of the map -- rows
// rl_a .. rl_b of the sequence read positions rl_a .. rl_b + TAPS - 1 behind the sequence's first window start, every
// one of them by some window -- and that run is a SEGMENT: n + TAPS - 1 staged entries for n rows, 128 + 17 (TAPS - 1)
// <= 145 entries per tile at most.  Every position is loaded, split and staged ONCE, whatever the taps.
//     entry(row r) = first entry of its segment + (rl - first rl of the segment);  fragment of (r, t) = entry(r) + t
// A segment gets ONE power-of-two scale, s = 2^(14 - floor(log2 max|x|)) over its entries (split_f16.h:
// f2g_f16_scales -- exponent clamp, all-zero and non-finite rules exactly those of f2g_split_f16x2_seq for a run).
// A window never leaves its sequence, so every output row has exactly one scale and its sum is exact; a segment's
// maximum is at most its sequence's, so the error bound of gemm_f16p.hip holds with amax_seq read as amax_segment.
// Only positions a window of a valid row (r < M) reads are loaded, enter a maximum or are staged.
//
// THE MAXIMUM is an integer maximum of sign-less bit patterns (the same order as the values'; a NaN ranks above inf):
// a thread's four floats, the 32 lanes that share a 512-byte position (a butterfly), then ds_max_u32 on one LDS word
// per segment.  An integer maximum does not depend on the order of its operands: the launch is reproducible bit for
// bit -- but for E.colsum, which is added by atomics.
//
// WEIGHTS IN REGISTERS, PERSISTENT TILES.  B is the weight's f2g_split_f16x2_seq image (split = 7, one scale per
// row).  A lane's fragments of it -- row li, the 8 reduction elements of its half of every 16-k step: 16 bytes of
// the image's hi halves and 16 of its lo halves, as they lie there -- are loaded ONCE per block, straight from the
// image into registers (K / 16 steps x 8 registers: 128 for K = 256), and stay; block b walks the row tiles b,
// b + grid, ...  Nothing of B ever enters the LDS.  Per tile, 2 barriers that wait for the LDS only:
//     request the tile's fp32 positions (<= 19 x 16 bytes per thread), segment maxima (LDS atomics)     barrier A
//     scales, split into the 4 slabs of 64 B hi + 64 B lo per position the h3p kernels read (pitch 528 bytes:
//     ds_read_b128 of 32 consecutive rows stay off each other's banks); per row: scale, entry, output offset
//                                                                                                        barrier B
//     TAPS x 8 k-steps x 3 v_mfma_f32_32x32x16_f16 (no slab loop: the whole reduction of the tile is staged)
//     v = (acc0 + 2^-11 acc1) * rscale_seg[row] * rscale_b[col] -> thin_epilogue.h (the one gemm_x6n_kernel has)
// The phases of ONE block run one after the other, as gemm_h3p3n_kernel's do; the overlap comes from the SECOND block
// of the CU, whose loads, split and stores run under this block's MFMAs and the other way round.  The positions'
// registers are dead during the MFMAs and the accumulators during staging, which is what lets both fit beside the
// weights.  Column sums are kept per lane across the block's tiles: one atomic per column and wave at the end.
//
// RESOURCES (gfx950, tools/kernel_resources.py; DESIGN.md section 3 has the table): 256 threads,
// __launch_bounds__(256, 2); LDS <TAPS = 2> 78,864 bytes = 145 entries x 528 (76,560) + 128 row scales + 128 row
// entries + 128 row offsets (8 bytes) + 2 x 32 segment maxima, <TAPS = 1> 69,888 bytes (128 entries): two blocks per
// CU (160 KB).  Registers <2> 256 VGPRs (128 of them the weights, 76 the positions in flight), <1> 178; no AGPRs, no
// scratch, no vector or scalar spills; occupancy 2 waves per SIMD = the two blocks.  Of the two ways to two blocks per
// CU -- this one, or a 64-row tile with the weight image resident in LDS -- this one reads 128 KB of fragments per
// 128 rows from the LDS and the other 256 KB (the weights again for every row group), on a kernel whose LDS traffic is
// as long as its MFMAs.
// MEASURED: profiles/fp16x3_tapn_shapes.txt (tools/fp16x3_tap_shapes.py --tapn); DESIGN.md section 0 reads it.
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
static_assert(NSEG <= 32, "a tile's segments");

template <int TAPS>
struct h3pn_lds {
  static constexpr int LPOS = 128 + NSEG * (TAPS - 1);      // staged entries of a tile
  static constexpr int OPERA = LPOS * PITCH;
  static constexpr int RSTAB = OPERA;                       // the tile's 128 row scales
  static constexpr int RENT = RSTAB + 128 * 4;              // ... first entries
  static constexpr int ROWOFF = RENT + 128 * 4;             // ... output offsets (thin_epilogue.h)
  static constexpr int SEGMAX = ROWOFF + 128 * 8;           // segment maxima, two sets of 32 words (tile parity)
  static constexpr size_t SMEM = (size_t)SEGMAX + 2 * 32 * 4;
  static constexpr int NJ = (LPOS + 7) / 8;                 // positions per thread: 8 per pass, 32 lanes each
  static_assert(SMEM <= 80 * 1024, "two blocks per CU");
  static_assert(ROWOFF % 8 == 0, "64-bit offsets");
};

struct h3pn_tap {
  int P0, seqfl, offfl, ntiles;            // rows per sequence; floats per sequence; -pad0 * 128; row tiles
  unsigned rEP;                            // ceil(2^16 / (P0 + TAPS - 1)): e / EP = e * rEP >> 16 for e < 145 (below)
  unsigned bytes;
};

template <int TAPS>
__global__ __launch_bounds__(NTHR, 2) void gemm_h3pn_kernel(const f2g_gemm_desc d, int M, int N, const h3pn_tap R) {
  static_assert(TAPS == 1 || TAPS == 2, "K = TAPS * 128: the weight fragments are kept in registers");
  using lds = h3pn_lds<TAPS>;
  constexpr int NJ = lds::NJ, KS = TAPS * 8;   // 16-k steps of the reduction
  extern __shared__ __attribute__((aligned(16))) unsigned char smemn[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, h = lane >> 5;
  const int pe = tid >> 5, pc = tid & 31;  // staging: entry pe + 8 j, 16-byte chunk pc (channels 4 pc .. 4 pc + 3)
  float* rstab = reinterpret_cast<float*>(smemn + lds::RSTAB);
  int* rent = reinterpret_cast<int*>(smemn + lds::RENT);
  long long* rowoff = reinterpret_cast<long long*>(smemn + lds::ROWOFF);
  unsigned* segmax = reinterpret_cast<unsigned*>(smemn + lds::SEGMAX);
  const int EP = R.P0 + TAPS - 1;          // entries of a whole sequence's segment
  __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)d.A.base, 0, R.bytes, 0x00020000);

  // ---- this lane's weight fragments, for the block's life: wq[k-step][0 hi / 1 lo] = the halves of reduction
  // elements 16 ks + 8 h .. + 7 of row li (the image: slabs of 32 elements, 64 bytes hi + 64 bytes lo); rows past N:
  // zeros
  u32x4 wq[KS][2];
  {
    const unsigned rowbytesW = (unsigned)(d.B.seq_stride * 4);
    __amdgpu_buffer_rsrc_t rsW =
        __builtin_amdgcn_make_buffer_rsrc((void*)d.B.base, 0, (unsigned)N * rowbytesW, 0x00020000);
    const unsigned vo = li < N ? (unsigned)li * rowbytesW + h * 16 : 0xf0000000u;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int p = 0; p < 2; ++p)
        wq[ks][p] = __builtin_amdgcn_raw_buffer_load_b128(rsW, vo, (ks >> 1) * 128 + p * 64 + (ks & 1) * 32, 0);
  }
  const float sb = li < N ? d.B.rscale[li] : 0.f;
  if (tid < 64) segmax[tid] = 0u;
  __syncthreads();

  float cs = 0.f;                          // this lane's part of column li's sum over the block's tiles
  int par = 0;
  for (int tile = blockIdx.x; tile < R.ntiles; tile += gridDim.x, par ^= 1) {
    // ---- geometry of the tile: its first sequence and window, the entries of its first segment and of all of them
    // (rows past M own none)
    const int m0 = tile * 128;
    const int sq0 = m0 / R.P0, rl0 = m0 - sq0 * R.P0;
    const int nval = M - m0 < 128 ? M - m0 : 128;
    const int n0 = R.P0 - rl0 < nval ? R.P0 - rl0 : nval;
    const int rest = nval - n0, nfull = rest / R.P0, part = rest - nfull * R.P0;
    const int E0 = n0 + TAPS - 1;
    const int L = E0 + nfull * EP + (part ? part + TAPS - 1 : 0);
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
    // and 19 lane masks of the first loop alive beside the positions -- 6 vector spills, 48 scalar ones)
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
    // ---- scale and split the positions into LDS; per row: reciprocal scale, first entry, output offset; the other
    // parity's maxima to zero (last read before the previous tile's barrier B, next written behind this tile's)
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
      // (rows past the end read entry 0: staged data, never used)
      const int r = m0 + tid;
      float s, rs = 0.f;
      int entry = 0;
      if (r < M) {
        const int sq = r / R.P0, k = sq - sq0, rl = r - sq * R.P0;
        entry = k == 0 ? rl - rl0 : E0 + (k - 1) * EP + rl;
        f2g_f16_scales(smx[k], s, rs);
      }
      rstab[tid] = rs;
      rent[tid] = entry;
    }
    thin::row_offsets(d.E, M, m0, tid, rowoff);
    if (tid < 32) segmax[32 * (par ^ 1) + tid] = 0u;
    lds_barrier();       // B: the tile is staged
    const unsigned char* rA = smemn + rent[wave * 32 + li] * PITCH + h * 16;
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
      acc[0][e] = h3_value(acc[0][e], acx[0][e], rstab[wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * h], sb);
    cs += thin::row_values(d.E, acc[0], N, wave, li, h, rowoff);
  }
  thin::column_sums(d.E, N, li, h, cs);
}

}  // namespace

// A the fp32 map marked split = 8 under stride-1 windows of 2 or 1 positions over 128 channels, at most 32 columns,
// row tiles of 128, the thin epilogue
int f2g_h3pn_ok(const f2g_gemm_desc& d) {
  const f2g_operand& A = d.A;
  if (A.split != 8 || d.B.rows > 32 || !h3_tap_fwd_ok(d, 128, 0, false)) return 0;
  if (host_plain(A) || A.P1 != 1 || A.step0 != 1 || A.unit != 128 || A.seglen < A.cols) return 0;
  if (A.cols != A.unit && A.cols != 2 * A.unit) return 0;
  if ((A.seq_stride % A.unit) || A.pad0 > 0 || A.P0 < 8) return 0;      // (P0: NSEG segments)
  return f16_b_image_status(d.B, 7);
}


template <int TAPS>
static void h3pn_launch(const f2g_gemm_desc& d, hipStream_t st) {
  using lds = h3pn_lds<TAPS>;
  const int M = d.A.rows, N = d.B.rows;
  dyn_lds_once<gemm_h3pn_kernel<TAPS>>((int)lds::SMEM);
  h3pn_tap R;
  R.P0 = d.A.P0, R.seqfl = (int)d.A.seq_stride, R.offfl = -d.A.pad0 * 128, R.ntiles = (M + 127) / 128;
  R.rEP = (65536u + (unsigned)(R.P0 + TAPS - 1) - 1u) / (unsigned)(R.P0 + TAPS - 1);
  R.bytes = (unsigned)(x6_a_extent(d.A) * 4);
  const int grid = R.ntiles < 512 ? R.ntiles : 512;      // two resident blocks per CU
  hipLaunchKernelGGL((gemm_h3pn_kernel<TAPS>), dim3(grid), dim3(NTHR), lds::SMEM, st, d, M, N, R);
}

int f2g_launch_h3pn(const f2g_gemm_desc& d, hipStream_t st) {
  if (d.A.cols == 2 * d.A.unit) {
    f2g_note_kernel("h3pn<taps=2>", 1, 6);
    h3pn_launch<2>(d, st);
  } else {
    f2g_note_kernel("h3pn<taps=1>", 1, 6);
    h3pn_launch<1>(d, st);
  }
  return f2g_check_launch();
}
