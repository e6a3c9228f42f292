// fp16x3 over STRIDE-3 conv windows of five positions of a halo map with 32 CHANNELS (the MPD's 32 -> 128 forward
// layer, K = 160 -- what gemm_x6g_kernel runs in the bf16x6 mode), SCALED INSIDE THE KERNEL: the A operand is
// the fp32 map itself (f2g_operand.split = 8), there is no image pass and no rscale.  gemm_f16p.hip has the arithmetic
// and the error bound of the tap-walking family; gemm_h3p3n_kernel<TAPS = 5, STRIDE = 3> is the one instance.
//
// SEGMENTS.  A tile is 128 output rows x all N <= 128 columns.  Its rows belong to 1 .. 17 sequences (P0 >= 8); the
// positions the rows of ONE sequence read are a contiguous run of the map -- rows rl_a .. rl_b of the sequence read
// positions 3 rl_a .. 3 rl_b + 4 behind the sequence's first window start, every one of them by some window -- and
// that run is a SEGMENT: 3 n + 2 staged entries for n rows, 3 * 128 + 2 * 17 = 418 <= LPOS entries per tile at most.
//     entry(row r) = first entry of its segment + 3 (rl - first rl of the segment);  fragment of (r, t) = entry(r) + t
// A segment gets ONE power-of-two scale, s = 2^(14 - floor(log2 max|x|)) over its entries (split_f16.h:
// f2g_f16_scales -- exponent clamp, all-zero and non-finite rules exactly those of f2g_split_f16x2_seq for a run).
// A window never leaves its sequence, so every output row has exactly one scale and its sum is exact; a segment's
// maximum is at most its sequence's, so the error bound of gemm_f16p.hip holds with amax_seq read as amax_segment.
// Only positions a window of a valid row (r < M) reads are loaded, enter a maximum or are staged.
//
// THE MAXIMUM is an integer maximum of sign-less bit patterns (the same order as the values'; a NaN ranks above inf):
// a thread's four floats, the 8 lanes that share a position (a butterfly), then ds_max_u32 on one LDS word per
// segment.  An integer maximum does not depend on the order of its operands: the launch is reproducible bit for bit.
//
// RESIDENT WEIGHTS, PERSISTENT TILES.  B is the weight's f2g_split_f16x2_seq image (split = 7, one scale per row):
// all N rows x 5 slabs of it are loaded into LDS once per block and stay; block b walks the row tiles b, b + grid,
// ...  The next tile's fp32 positions are requested into registers (14 x 16 bytes per thread) before the current
// tile's MFMAs and arrive under them and the epilogue; maximum, split and LDS stores follow when the epilogue's
// patches (which overlay the staged positions) are free.  Per tile: 3 barriers that wait for the LDS only.
//     top      the prefetched registers -> segment maxima (LDS atomics)                     barrier A
//              scales, split into the 64 B hi + 64 B lo slabs the h3p kernels read, row scale table   barrier B
//              request the next tile; 5 taps x 2 k-steps x 12 v_mfma_f32_32x32x16_f16       barrier C
//              v = (acc0 + 2^-11 acc1) * rscale_seg[row] * rscale_b[col] -> x6e::wide_epilogue (64 x 64 wave tiles)
//
// RESOURCES (gfx950, tools/kernel_resources.py): 256 threads, one block per CU; LDS 145,216 bytes = 420 entries x
// 144 (60,480) + 128 weight rows x 656 (83,968) + 128 row scales + 2 x 32 segment maxima; 256 VGPRs + 255 AGPRs (one
// wave per SIMD: two accumulator sets, the loop-invariant weight fragments the compiler keeps across tiles, the
// 56-register prefetch), no scratch, no vector spills; 52 scalar registers are spilled to vector LANES, not to
// memory (the block keeps the whole f2g_epilogue live across its tile loop).
// MEASURED (profiles/fp16x3_tap3n_shapes.txt): this first version LOSES to gemm_x6g_kernel, 1.21-1.38 of its time --
// the four phases of a tile run one after the other; DESIGN.md section 0 has the numbers and the next step.
#include <stddef.h>
#include <stdint.h>

#include "gemm_f16_checks.h"
#include "gemm_f16_common.h"
#include "split_f16.h"
#include "x6_epilogue.h"

namespace {

constexpr int PITCH = 144;                 // bytes of a staged position: 2 x 64 + 16 (36 dwords)
constexpr int LPOS = 420;                  // staged entries of a tile (>= 3 * 128 + 2 * NSEG)
constexpr int NSEG = 17;                   // segments of a tile at most: 2 + 126 / P0, P0 >= 8 (host check)
constexpr int WPITCH = 5 * 128 + 16;       // bytes of a resident weight row: five slabs + 16 (164 dwords)
constexpr int OPERA = LPOS * PITCH;
constexpr int OPERW = 128 * WPITCH;
constexpr int RSTAB = OPERA + OPERW;       // the tile's 128 row scales
constexpr int SEGMAX = RSTAB + 128 * 4;    // segment maxima, two sets of 32 words (tile parity)
constexpr size_t SMEM = (size_t)SEGMAX + 2 * 32 * 4;
constexpr int NTHR = 256;
constexpr int NJ = (LPOS * 8 + NTHR - 1) / NTHR;   // 16-byte chunks of the staged fp32 positions per thread
using x6e::ESZ;
static_assert(3 * 128 + 2 * NSEG <= LPOS && NSEG <= 32, "a tile's segments");
static_assert(SMEM <= 160 * 1024, "a block's LDS");
static_assert(4 * ESZ <= OPERA, "epilogue patches overlay the staged positions only");

struct h3p3n_tap {
  int P0, seqfl, offfl, ntiles;            // rows per sequence; floats per sequence; -pad0 * 32; row tiles
  unsigned bytes;
};

template <int TAPS, int STRIDE>
__global__ __launch_bounds__(NTHR, 1) void gemm_h3p3n_kernel(const f2g_gemm_desc d, int M, int N,
                                                             const h3p3n_tap R) {
  static_assert(TAPS == 5 && STRIDE == 3, "the segment arithmetic below is that of (5, 3)");
  extern __shared__ __attribute__((aligned(16))) unsigned char smemp[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, h = lane >> 5;
  const int pe = tid >> 3, pc = tid & 7;   // staging: entry pe + 32 j, 16-byte chunk pc (floats 4 pc .. 4 pc + 3)
  float* rstab = reinterpret_cast<float*>(smemp + RSTAB);
  unsigned* segmax = reinterpret_cast<unsigned*>(smemp + SEGMAX);
  const int EP = STRIDE * R.P0 + 2;        // entries of a whole sequence's segment
  __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)d.A.base, 0, R.bytes, 0x00020000);

  // ---- geometry of the tile whose first row is m0: its first sequence and window, the entries of its first segment
  // and of all of them (rows past M own none)
  struct geom {
    int sq0, rl0, E0, L;
  };
  auto geom_of = [&](int m0) {
    geom g;
    g.sq0 = m0 / R.P0, g.rl0 = m0 - g.sq0 * R.P0;
    const int nval = M - m0 < 128 ? M - m0 : 128;
    const int n0 = R.P0 - g.rl0 < nval ? R.P0 - g.rl0 : nval;
    const int rest = nval - n0, nfull = rest / R.P0, part = rest - nfull * R.P0;
    g.E0 = STRIDE * n0 + 2;
    g.L = g.E0 + nfull * EP + (part ? STRIDE * part + 2 : 0);
    return g;
  };
  u32x4 xa[NJ];
  int kseg[NJ];                            // segment of entry pe + 32 j, -1 = not an entry of this tile
  auto request = [&](int m0) {
    const geom g = geom_of(m0);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int e = pe + 32 * j;
      int k = 0, q = e + STRIDE * g.rl0;
      if (e >= g.E0) {
        const int e2 = e - g.E0;
        k = 1 + e2 / EP;
        q = e2 - (k - 1) * EP;
      }
      const bool ok = e < g.L;
      kseg[j] = ok ? k : -1;
      // (the byte offset stays under the resource limit: host check; the others lie outside the resource = zeros)
      const unsigned vo = ok ? ((unsigned)(g.sq0 + k) * (unsigned)R.seqfl + (unsigned)(R.offfl + q * 32)) * 4u + pc * 16
                             : 0xf0000000u;
      xa[j] = __builtin_amdgcn_raw_buffer_load_b128(rsA, vo, 0, 0);
    }
  };

  int tile = blockIdx.x;
  request(tile * 128);
  if (tid < 64) segmax[tid] = 0u;
  {
    // the whole weight image -> LDS, once (rows past N: zeros)
    const unsigned rowbytesW = (unsigned)(d.B.seq_stride * 4);
    __amdgpu_buffer_rsrc_t rsW =
        __builtin_amdgcn_make_buffer_rsrc((void*)d.B.base, 0, (unsigned)N * rowbytesW, 0x00020000);
#pragma unroll 4
    for (int id = tid; id < 128 * 40; id += NTHR) {
      const int row = id / 40, c = id - row * 40;
      const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(
          rsW, row < N ? (unsigned)row * rowbytesW + c * 16 : 0xf0000000u, 0, 0);
      *reinterpret_cast<u32x4*>(smemp + OPERA + row * WPITCH + c * 16) = w;
    }
  }
  float sb[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int col = wn * 64 + ni * 32 + li;
    sb[ni] = col < N ? d.B.rscale[col] : 0.f;
  }
  const unsigned char* rB = smemp + OPERA + (wn * 64 + li) * WPITCH + h * 16;
  __syncthreads();

  for (int par = 0; tile < R.ntiles; tile += gridDim.x, par ^= 1) {
    const int m0 = tile * 128;
    const geom g = geom_of(m0);
    unsigned* smx = segmax + 32 * par;
    // ---- segment maxima: thread, the 8 lanes of a position, one LDS word per segment
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const float4 v = make_float4(__uint_as_float(xa[j].x), __uint_as_float(xa[j].y), __uint_as_float(xa[j].z),
                                   __uint_as_float(xa[j].w));
      unsigned m = f2g_f16_amax4(v, 0u);
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) {
        const unsigned t = (unsigned)__shfl_xor((int)m, o);
        m = m > t ? m : t;
      }
      if (pc == 0 && kseg[j] >= 0) atomicMax(smx + kseg[j], m);
    }
    lds_barrier();       // A: the maxima are complete; every wave has left the previous tile's epilogue patches
    // ---- scale and split the positions into LDS; the rows' reciprocal scales; the other parity's maxima to zero
    // (last read before the previous tile's barrier B, next written behind this tile's)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (kseg[j] < 0) continue;
      float s, rs;
      f2g_f16_scales(smx[kseg[j]], s, rs);
      const float4 v = make_float4(__uint_as_float(xa[j].x), __uint_as_float(xa[j].y), __uint_as_float(xa[j].z),
                                   __uint_as_float(xa[j].w));
      const uint4 p = f2g_f16_split4(v, s);              // (h01, h23, l01, l23)
      unsigned char* q = smemp + (pe + 32 * j) * PITCH + pc * 8;
      *reinterpret_cast<u32x2*>(q) = u32x2{p.x, p.y};
      *reinterpret_cast<u32x2*>(q + 64) = u32x2{p.z, p.w};
    }
    if (tid < 128) {
      float s, rs = 0.f;
      if (m0 + tid < M) f2g_f16_scales(smx[(m0 + tid) / R.P0 - g.sq0], s, rs);
      rstab[tid] = rs;
    }
    if (tid < 32) segmax[32 * (par ^ 1) + tid] = 0u;
    // fragment rows of this lane: output rows m0 + wm * 64 + i * 32 + li -> entry (rows past the end read entry 0:
    // staged data, never used)
    const unsigned char* rA[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = m0 + wm * 64 + i * 32 + li, sq = r / R.P0, k = sq - g.sq0, rl = r - sq * R.P0;
      const int entry = r < M ? (k == 0 ? STRIDE * (rl - g.rl0) : g.E0 + (k - 1) * EP + STRIDE * rl) : 0;
      rA[i] = smemp + entry * PITCH + h * 16;
    }
    lds_barrier();       // B: the tile is staged
    if (tile + (int)gridDim.x < R.ntiles) request((tile + (int)gridDim.x) * 128);
    f32x16 acc[2][2], acx[2][2];
    h3_zero<4>(acc[0], acx[0]);
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      // this tap's fragments ([ks][piece: 0 hi, 1 lo][sub-tile])
      f16x8 fa[2][2][2], fb[2][2][2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            fa[ks][p][s] = *reinterpret_cast<const f16x8*>(rA[s] + t * PITCH + p * 64 + ks * 32);
            fb[ks][p][s] = *reinterpret_cast<const f16x8*>(rB + s * 32 * WPITCH + t * 128 + p * 64 + ks * 32);
          }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) h3_mfma12(acc, acx, fa[ks][0], fa[ks][1], fb[ks][0], fb[ks][1]);
    }
    // v = (acc0 + 2^-11 acc1) / s_a[segment of the row] / s_b[col] (gemm_f16_common.h: h3_value)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float sa = rstab[wm * 64 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * h];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni][e] = h3_value(acc[mi][ni][e], acx[mi][ni][e], sa, sb[ni]);
      }
    lds_barrier();       // C: every wave's fragment reads are complete -- the patches overlay the staged positions
    x6e::wide_epilogue(d.E, acc, M, N, m0 + wm * 64, wn * 64, lane, smemp + wave * ESZ);
  }
}

}  // namespace

// A the fp32 map marked split = 8 under stride-3 windows of 5 positions over 32 channels, at most 128 columns, row
// tiles of 128
int f2g_h3p3n_ok(const f2g_gemm_desc& d) {
  const f2g_operand& A = d.A;
  if (A.split != 8 || d.B.rows > 128 || !h3_tap_fwd_ok(d, 128, 0, true)) return 0;
  if (host_plain(A) || A.P1 != 1 || A.step0 != 3 || A.unit != 32 || A.cols != 5 * A.unit || A.seglen < A.cols) return 0;
  if ((A.seq_stride % A.unit) || A.pad0 > 0 || A.P0 < 8) return 0;      // (P0: NSEG segments)
  return f16_b_image_status(d.B, 7);
}

int f2g_launch_h3p3n(const f2g_gemm_desc& d, hipStream_t st) {
  const int M = d.A.rows, N = d.B.rows;
  dyn_lds_once<gemm_h3p3n_kernel<5, 3>>((int)SMEM);
  h3p3n_tap R;
  R.P0 = d.A.P0, R.seqfl = (int)d.A.seq_stride, R.offfl = -d.A.pad0 * 32, R.ntiles = (M + 127) / 128;
  R.bytes = (unsigned)(x6_a_extent(d.A) * 4);
  const int grid = R.ntiles < 256 ? R.ntiles : 256;      // one resident block per CU
  f2g_note_kernel("h3p3n<taps=5,step=3>", 1, 6);
  hipLaunchKernelGGL((gemm_h3p3n_kernel<5, 3>), dim3(grid), dim3(NTHR), SMEM, st, d, M, N, R);
  return f2g_check_launch();
}
