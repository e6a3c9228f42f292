// fp16x3 over stride-1 conv windows of a halo map (the 1024-channel MPD layer, its data gradient and the residue
// data gradients of the stride-3 layers -- what gemm_x6p_kernel runs in the bf16x6 mode): f2g_split_f16x2_seq writes
// the operand images, gemm_h3p_kernel<TAPS> reads them.
//
// ONE SCALE PER SEQUENCE.  The per-row scale of f2g_split_f16x2 does not factor out of overlapping windows: a map
// position belongs to up to TAPS output rows.  A window never leaves its sequence (the seq_stride contiguous floats
// of one (batch, period column)), so one power-of-two scale per sequence leaves every output row's sum exactly, and
// the epilogue undoes it with rscale[row / P0].  split_f16.h has the arithmetic (the same with "row" read as
// "sequence"); what the coarser scale costs is a floor term: an element 2^-28 below its SEQUENCE's largest is
// subnormal in hi, so a window that is quiet against its own sequence keeps an absolute error of at most
// 2^-28 amax_seq sum_k |w[n,k]| per output beside the relative 3 * 2^-22 |a| |b| per product.
//
// IMAGE LAYOUT (not f2g_split_f16x2's groups of four): every aligned slab of 32 floats becomes 64 bytes of hi (32
// halves, in order) and then 64 bytes of lo -- the fp32 buffer's own addressing, element e in the 128 bytes at
// (e / 32) * 128, the image as large as the buffer -- so that a fragment read of the kernel is 16 bytes = eight
// consecutive-k halves of ONE piece.
#include <stddef.h>
#include <stdint.h>

#include "gemm_f16_checks.h"
#include "gemm_f16_common.h"
#include "split_f16.h"
#include "x6_epilogue.h"

namespace {

// ---- the image ----------------------------------------------------------------------------------------------------
// One block per run (a run is far longer than a register file -- 148 x 1024 floats for the fifth layer at period 2
// -- so it is read twice: the largest magnitude, then the split; the second read finds the cache).  No atomics: the
// waves' maxima meet in LDS and every thread takes the largest of the sixteen, so the image is reproducible bit for
// bit.  A thread takes eight floats at a time: two 16-byte loads, one 16-byte store per piece.
constexpr int SEQ_THREADS = 1024;

__global__ __launch_bounds__(SEQ_THREADS) void split_f16x2_seq_kernel(uint4* dst, float* __restrict__ rscale,
                                                                     const float* src, long long ld, int n8) {
  __shared__ unsigned part[SEQ_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const float4* s4 = reinterpret_cast<const float4*>(src + (long long)blockIdx.x * ld);
  unsigned m = 0;
  for (int c = tid; c < n8; c += SEQ_THREADS) {
    m = f2g_f16_amax4(s4[2 * c], m);
    m = f2g_f16_amax4(s4[2 * c + 1], m);
  }
  m = f2g_wave_max(m);
  if (lane == 0) part[tid >> 6] = m;
  __syncthreads();
  m = part[0];
#pragma unroll
  for (int w = 1; w < SEQ_THREADS / 64; ++w) m = m > part[w] ? m : part[w];
  float s, rs;
  f2g_f16_scales(m, s, rs);
  if (tid == 0) rscale[blockIdx.x] = rs;
  uint4* d4 = dst + (long long)blockIdx.x * (ld >> 2);
  for (int c = tid; c < n8; c += SEQ_THREADS) {
    const uint4 a = f2g_f16_split4(s4[2 * c], s), b = f2g_f16_split4(s4[2 * c + 1], s);     // (h01, h23, l01, l23)
    uint4* slab = d4 + (c >> 2) * 8 + (c & 3);
    slab[0] = make_uint4(a.x, a.y, b.x, b.y);
    slab[4] = make_uint4(a.z, a.w, b.z, b.w);
  }
}

// ---- the GEMM -----------------------------------------------------------------------------------------------------
// gemm_x6p_kernel's structure (gemm_x6p.hip has the schedule): a 256 x 128 tile, two ping-pong wave groups half a
// step apart, a group stages the map positions of its own 128 rows, weight slabs double-buffered, barriers wait for
// the LDS only, K order = channel slab outer, tap inner.  What differs: two pieces per operand (a staged position /
// weight row is 128 bytes + 16 of pitch instead of 192 + 16), v_mfma_f32_32x32x16_f16, two accumulator sets (hi hi',
// and hi lo' + lo hi', which carries the factor 2^-11) -- 24 MFMAs and 16 ds_read_b128 per wave and slab step
// instead of 48 and 24 --, and before the epilogue v = (acc0 + 2^-11 acc1) * rscale_a[row / P0] * rscale_b[col] with
// the tile's 256 row scales from a table in LDS (filled once: no division per element).  Then x6e::wide_epilogue.
constexpr int PITCH = 144;                 // bytes of a staged position / weight row: 2 x 64 + 16 (36 dwords)
constexpr int LH = 160;                    // staged positions of a group's 128 rows (host check)
constexpr int OPERA = 2 * LH * PITCH;      // both groups' positions
constexpr int OPERB = 128 * PITCH;         // one weight slab
constexpr int RSTAB = OPERA + 2 * OPERB;   // the tile's row scales (256 floats) behind the operands
using x6e::ESZ;

struct h3p_tap {
  int P0, HpIn, offpos, C32;
  unsigned bytes;
};

template <int TAPS>
__global__ __launch_bounds__(512, 1) void gemm_h3p_kernel(const f2g_gemm_desc d, int M, int N, int K,
                                                          const h3p_tap R) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smemp[];
  constexpr int NJA = (LH * 8 + 255) / 256, NJB = 128 * 8 / 512;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = wave >> 2, gt = tid & 255;
  const int wm = (wave >> 1) & 1, wn = wave & 1, li = lane & 31, h = lane >> 5;
  int m0, n0;
  tile_of_block(256, 128, m0, n0);
  const int mg = m0 + 128 * grp;                  // first row of this group's half of the tile
  f32x16 acc[2][2], acx[2][2];
  h3_zero<4>(acc[0], acx[0]);
  auto posrow = [&](int r) {
    const int sq = r / R.P0;
    return sq * R.HpIn + (r - sq * R.P0) + R.offpos;
  };
  // reciprocal scale of every row of the tile (its sequence's; rows past the end: 0), read after the main loop
  float* rstab = reinterpret_cast<float*>(smemp + RSTAB);
  if (tid < 256) rstab[tid] = m0 + tid < M ? d.A.rscale[(m0 + tid) / R.P0] : 0.f;
  const int pbase = posrow(mg);
  const int rlast = mg + 127 < M ? mg + 127 : M - 1;
  const int L = mg < M ? posrow(rlast) - pbase + TAPS : 0;     // staged positions (<= LH: host check)
  const unsigned rowbytesA = (unsigned)R.C32 * 128u;           // one position of the map image
  const unsigned rowbytesW = (unsigned)(d.B.seq_stride * 4);   // one weight row of the image (the matrix's pitch)
  __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)d.A.base, 0, R.bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)d.B.base, 0, (unsigned)N * rowbytesW, 0x00020000);
  unsigned char* myA = smemp + grp * (LH * PITCH);
  unsigned voA[NJA], voW[NJB];
  int loA[NJA], loW[NJB];
#pragma unroll
  for (int j = 0; j < NJA; ++j) {
    const int id = gt + 256 * j, q = id >> 3, c = id & 7;
    voA[j] = q < L ? (unsigned)(pbase + q) * rowbytesA + c * 16 : 0xf0000000u;   // (outside the resource: zeros)
    loA[j] = q < LH ? q * PITCH + c * 16 : -1;
  }
#pragma unroll
  for (int j = 0; j < NJB; ++j) {
    const int id = tid + 512 * j, row = id >> 3, c = id & 7;
    // (rows past N lie behind the resource = zeros; the offset itself must not wrap below it)
    voW[j] = n0 + row < N ? (unsigned)(n0 + row) * rowbytesW + c * 16 : 0xf0000000u;
    loW[j] = OPERA + row * PITCH + c * 16;
  }
  u32x4 xa[NJA], xw[NJB];
  auto gloadA = [&](int cs) {
#pragma unroll
    for (int j = 0; j < NJA; ++j) xa[j] = __builtin_amdgcn_raw_buffer_load_b128(rsA, voA[j], cs * 128, 0);
  };
  auto gloadB = [&](int slab) {
#pragma unroll
    for (int j = 0; j < NJB; ++j) xw[j] = __builtin_amdgcn_raw_buffer_load_b128(rsW, voW[j], slab * 128, 0);
  };
  auto storeA = [&]() {
#pragma unroll
    for (int j = 0; j < NJA; ++j)
      if (loA[j] >= 0) *reinterpret_cast<u32x4*>(myA + loA[j]) = xa[j];
  };
  auto storeB = [&](int buf) {
#pragma unroll
    for (int j = 0; j < NJB; ++j) *reinterpret_cast<u32x4*>(smemp + buf * OPERB + loW[j]) = xw[j];
  };
  // fragment rows of this lane: output rows mg + wm * 64 + i * 32 + li -> staged position of the group
  const unsigned char* rA[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = mg + wm * 64 + i * 32 + li;
    rA[i] = myA + (r < M ? posrow(r) - pbase : 0) * PITCH + h * 16;
  }
  const unsigned char* rB = smemp + OPERA + (wn * 64 + li) * PITCH + h * 16;
  // weight slab of step s = (cs, t): K order = channel slab outer, tap inner -> image slab t * C32 + cs
  const int nsteps = R.C32 * TAPS;
  auto slab_of = [&](int s) {
    if (s >= nsteps) s = 0;                      // (past the end: re-read, never used)
    const int c2 = s / TAPS, t2 = s - c2 * TAPS;
    return t2 * R.C32 + c2;
  };
  gloadA(0);
  gloadB(slab_of(0));
  storeA();
  storeB(0);
  gloadA(1 < R.C32 ? 1 : 0);
  gloadB(slab_of(1));
  lds_barrier();
  if (grp == 1) lds_barrier();                   // group 1 runs one slot behind
  int step = 0;
  for (int cs = 0; cs < R.C32; ++cs) {
#pragma unroll
    for (int t = 0; t < TAPS; ++t, ++step) {
      const int buf = step & 1;
      // ---- read slot: this step's fragments ([ks][piece: 0 hi, 1 lo][sub-tile]); my share of the next weight
      // slab; request the one after
      f16x8 fa[2][2][2], fb[2][2][2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            fa[ks][p][i] = *reinterpret_cast<const f16x8*>(rA[i] + t * PITCH + p * 64 + ks * 32);
            fb[ks][p][i] = *reinterpret_cast<const f16x8*>(rB + buf * OPERB + p * 64 + i * 32 * PITCH + ks * 32);
          }
      storeB(buf ^ 1);
      gloadB(slab_of(step + 2));
      lds_barrier();
      // ---- MFMA slot (the other group reads meanwhile)
      if (t == TAPS - 1 && cs + 1 < R.C32) {
        // last tap of this channel slab: the group's staged positions are replaced (their only readers are
        // this group's waves, whose reads were complete before the barrier above)
        storeA();
        gloadA(cs + 2 < R.C32 ? cs + 2 : 0);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) h3_mfma12(acc, acx, fa[ks][0], fa[ks][1], fb[ks][0], fb[ks][1]);
      __builtin_amdgcn_s_setprio(0);
      // (group 1's last MFMA slot needs no barrier behind it: group 0 is in its epilogue by then, and that
      // slot touches no LDS -- both groups pass 1 + 2 * nsteps barriers)
      if (!(grp == 1 && step == nsteps - 1)) lds_barrier();
    }
  }
  // v = (acc0 + 2^-11 acc1) / s_a[sequence of the row] / s_b[col] (gemm_f16_common.h: h3_value).  The table lies behind
  // everything the epilogue's patches overlay.
  float sb[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int col = n0 + wn * 64 + ni * 32 + li;
    sb[ni] = col < N ? d.B.rscale[col] : 0.f;
  }
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float sa = rstab[grp * 128 + wm * 64 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * h];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) acc[mi][ni][e] = h3_value(acc[mi][ni][e], acx[mi][ni][e], sa, sb[ni]);
    }
  // every fragment read of the main loop is complete (the last ones were group 1's, before the barrier group 0
  // has just passed): the waves turn their tiles through private patches at the bottom of the LDS
  x6e::wide_epilogue(d.E, acc, M, N, mg + wm * 64, n0 + wn * 64, lane, smemp + wave * ESZ);
}

}  // namespace

// stride-1 windows of 5 or 2 positions (x6_tap_ok) over two 32-channel groups at least, on 256 x 128 tiles
int f2g_h3p_ok(const f2g_gemm_desc& d) {
  if (!h3_tap_fwd_ok(d, 256, 128, true) || !(x6_tap_ok(d, 5) || x6_tap_ok(d, 2)) || d.A.unit / 32 < 2) return 0;
  return f16_images_status(d.A, d.B, 7);
}

int f2g_launch_h3p(const f2g_gemm_desc& d, hipStream_t st) {
  const int M = d.A.rows, N = d.B.rows, K = d.A.cols, taps = d.A.cols / d.A.unit;      // (f2g_h3p_ok: 5 or 2)
  constexpr size_t smem = (size_t)RSTAB + 256 * 4;
  static_assert(8 * ESZ <= RSTAB, "epilogue patches fit under the main loop's buffers, below the row scales");
  dyn_lds_once<gemm_h3p_kernel<5>, gemm_h3p_kernel<2>>((int)smem);
  h3p_tap R;
  R.P0 = d.A.P0, R.HpIn = (int)(d.A.seq_stride / d.A.unit), R.offpos = -d.A.pad0, R.C32 = d.A.unit / 32;
  R.bytes = (unsigned)(x6_a_extent(d.A) * 4);
  dim3 grid((M + 255) / 256, (N + 127) / 128);
  f2g_note_kernel(taps == 5 ? "h3p<taps=5>" : "h3p<taps=2>", 1, 6);
  if (taps == 5) hipLaunchKernelGGL(gemm_h3p_kernel<5>, grid, dim3(512), smem, st, d, M, N, K, R);
  else hipLaunchKernelGGL(gemm_h3p_kernel<2>, grid, dim3(512), smem, st, d, M, N, K, R);
  return f2g_check_launch();
}

extern "C" int f2g_split_f16x2_seq(float* dst, float* rscale, const float* src, int64_t ld, int32_t nseq,
                                   int32_t seq_floats, f2g_stream_t stream) {
  if (!dst || !rscale || !src || dst == src || nseq < 0 || seq_floats < 32 || (seq_floats % 32) || ld < seq_floats ||
      (ld % 32) || !al16(dst) || !al16(src))
    return F2G_EINVAL;
  if (nseq == 0) return F2G_OK;
  hipLaunchKernelGGL(split_f16x2_seq_kernel, dim3(nseq), dim3(SEQ_THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<uint4*>(dst), rscale, src, (long long)ld, seq_floats / 8);
  return f2g_check_launch();
}
