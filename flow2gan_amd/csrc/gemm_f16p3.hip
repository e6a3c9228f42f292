// fp16x3 over STRIDE-3 conv windows of five positions of a halo map (the MPD's 128 -> 512 and 512 -> 1024 forward
// layers -- what gemm_x6_kernel / X6_IMG runs in the bf16x6 mode): gemm_h3p_kernel's arithmetic (gemm_f16p.hip has the
// images, the per-sequence scale and the error bound; a window never leaves its sequence whatever its stride, so all
// of that holds unchanged) with another staging layout.  gemm_h3p3_kernel<TAPS = 5, STRIDE = 3> is the one instance.
//
// RESIDUE PLANES.  Tap t of window rl (counted inside its sequence) reads position q = 3 rl + t behind the
// sequence's first window start: class c = t % 3, index u = rl + t / 3.  A group's LDS area is three planes of LP
// entries, one per class; the 128 rows of a group own consecutive entries of every plane, and every sequence the
// group touches gets ONE entry more (u = its last row + 1, read by taps 3 and 4):
//     entry(row r) = (sq - sq0) * (P0 + 1) + rl - rl0        sq0, rl0: sequence and window of the group's first row
//     fragment of (r, t) = plane t % 3, entry(r) + t / 3
// so consecutive lanes read consecutive entries -- the bank pattern of gemm_h3p_kernel at the same 144-byte pitch --,
// only positions some window reads are staged (each once per channel slab; it serves the 5 / 3 windows that touch
// it), and the positions between a sequence's last window and the next sequence (HpIn - 3 P0 of them) cost nothing:
// the host bound is 130 + 126 / P0 <= LP, whatever HpIn.
//
// REPLACING A SLAB IN PORTIONS.  The taps run in the order 0, 3, 1, 4, 2.  Class 0 is dead once tap 3 has been read,
// class 1 after tap 4, class 2 after tap 2: a dead plane is overwritten with the next channel slab's at once, while
// the other taps still run, through ONE register stage of five 16-byte loads per thread (a straight twin of
// gemm_h3p_kernel needs thirteen):
//     step 1 (tap 3): store class 0 of slab cs + 1, request class 1      (two steps in flight)
//     step 3 (tap 4): store class 1, request class 2                     (one step)
//     step 4 (tap 2): store class 2, request class 0 of slab cs + 2      (two steps)
// Everything else -- 256 x 128 tile, two ping-pong wave groups, double-buffered weight slabs, barriers that wait for
// the LDS only, K order channel slab outer / tap inner, the row-scale table, x6e::wide_epilogue -- is gemm_h3p_kernel's.
#include <stddef.h>
#include <stdint.h>

#include "gemm_f16_checks.h"
#include "gemm_f16_common.h"
#include "x6_epilogue.h"

namespace {

constexpr int PITCH = 144;                 // bytes of a staged position / weight row: 2 x 64 + 16 (36 dwords)
constexpr int LP = 144;                    // entries of a plane (host check)
constexpr int PLANE = LP * PITCH;
constexpr int GROUPA = 3 * PLANE;          // one group's three planes
constexpr int OPERA = 2 * GROUPA;
constexpr int OPERB = 128 * PITCH;         // one weight slab
constexpr int RSTAB = OPERA + 2 * OPERB;   // the tile's row scales (256 floats) behind the operands
constexpr size_t SMEM = (size_t)RSTAB + 256 * 4;
using x6e::ESZ;
static_assert(SMEM <= 160 * 1024, "a block's LDS");
static_assert(8 * ESZ <= RSTAB, "epilogue patches fit under the main loop's buffers, below the row scales");

struct h3p3_tap {
  int P0, HpIn, offpos, C32, nseq;
  unsigned bytes;
};

template <int TAPS, int STRIDE>
__global__ __launch_bounds__(512, 1) void gemm_h3p3_kernel(const f2g_gemm_desc d, int M, int N, int K,
                                                           const h3p3_tap R) {
  static_assert(TAPS == 5 && STRIDE == 3, "the tap order and the class schedule below are those of (5, 3)");
  extern __shared__ __attribute__((aligned(16))) unsigned char smemp[];
  constexpr int NJA = (LP * 8 + 255) / 256, NJB = 128 * 8 / 512;
  constexpr int ORDER[TAPS] = {0, 3, 1, 4, 2};
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = wave >> 2, gt = tid & 255;
  const int wm = (wave >> 1) & 1, wn = wave & 1, li = lane & 31, h = lane >> 5;
  int m0, n0;
  tile_of_block(256, 128, m0, n0);
  const int mg = m0 + 128 * grp;                  // first row of this group's half of the tile
  f32x16 acc[2][2], acx[2][2];
  h3_zero<4>(acc[0], acx[0]);
  // reciprocal scale of every row of the tile (its sequence's; rows past the end: 0), read after the main loop
  float* rstab = reinterpret_cast<float*>(smemp + RSTAB);
  if (tid < 256) rstab[tid] = m0 + tid < M ? d.A.rscale[(m0 + tid) / R.P0] : 0.f;
  const int sq0 = mg / R.P0, rl0 = mg - sq0 * R.P0;
  const unsigned rowbytesA = (unsigned)R.C32 * 128u;           // one position of the map image
  const unsigned rowbytesW = (unsigned)(d.B.seq_stride * 4);   // one weight row of the image (the matrix's pitch)
  __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)d.A.base, 0, R.bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)d.B.base, 0, (unsigned)N * rowbytesW, 0x00020000);
  unsigned char* myA = smemp + grp * GROUPA;
  // staging: thread = (entry (gt >> 3) + 32 j, 16-byte chunk gt & 7) of whichever plane is being replaced.  voA: the
  // entry's position in the image, of the class requested last (the class lives in the VECTOR offset: the range
  // check of a buffer load does not see the scalar one); entries behind the last sequence lie outside the resource
  // = zeros, wherever the walk moves them.
  // The one entry a sequence owns past its last window is read for class 2 as well, where no window uses it: that
  // position lies inside the operand's extent or outside the resource.
  unsigned voA[NJA], voW[NJB];
  const int loA = (gt >> 3) * PITCH + (gt & 7) * 16, loW = OPERA + (tid >> 3) * PITCH + (tid & 7) * 16;
#pragma unroll
  for (int j = 0; j < NJA; ++j) {
    const int y = (gt >> 3) + 32 * j + rl0, k = y / (R.P0 + 1), u = y - k * (R.P0 + 1);
    voA[j] = sq0 + k < R.nseq ? (unsigned)((sq0 + k) * R.HpIn + R.offpos + STRIDE * u + 2) * rowbytesA + (gt & 7) * 16
                              : 0xf0000000u;      // (class 2's: the first request moves it to class 0)
  }
  const bool lastA = (gt >> 3) + 32 * (NJA - 1) < LP;          // (the last j covers half of its 32 entries)
#pragma unroll
  for (int j = 0; j < NJB; ++j) {
    const int id = tid + 512 * j, row = id >> 3, c = id & 7;
    // (rows past N lie behind the resource = zeros; the offset itself must not wrap below it)
    voW[j] = n0 + row < N ? (unsigned)(n0 + row) * rowbytesW + c * 16 : 0xf0000000u;
  }
  u32x4 xa[NJA], xw[NJB];
  // (the requests walk the classes 0, 1, 2, 0, ...: voA moves with them, one position up or two down)
  auto gloadA = [&](u32x4 (&x)[NJA], int cls, int cs) {
    const unsigned move = cls == 0 ? 0u - 2u * rowbytesA : rowbytesA;
#pragma unroll
    for (int j = 0; j < NJA; ++j) {
      voA[j] += move;
      x[j] = __builtin_amdgcn_raw_buffer_load_b128(rsA, voA[j], cs * 128, 0);
    }
  };
  auto storeA = [&](const u32x4 (&x)[NJA], int cls) {
#pragma unroll
    for (int j = 0; j < NJA; ++j)
      if (j + 1 < NJA || lastA) *reinterpret_cast<u32x4*>(myA + cls * PLANE + loA + j * 32 * PITCH) = x[j];
  };
  auto gloadB = [&](int slab) {
#pragma unroll
    for (int j = 0; j < NJB; ++j) xw[j] = __builtin_amdgcn_raw_buffer_load_b128(rsW, voW[j], slab * 128, 0);
  };
  auto storeB = [&](int buf) {
#pragma unroll
    for (int j = 0; j < NJB; ++j) *reinterpret_cast<u32x4*>(smemp + buf * OPERB + loW + j * 64 * PITCH) = xw[j];
  };
  // fragment rows of this lane: output rows mg + wm * 64 + i * 32 + li -> entry of the group's planes (rows past
  // the end read the group's first entry: staged data or zeros, never used)
  const unsigned char* rA[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = mg + wm * 64 + i * 32 + li, sq = r / R.P0;
    const int entry = r < M ? (sq - sq0) * (R.P0 + 1) + (r - sq * R.P0) - rl0 : 0;
    rA[i] = myA + entry * PITCH + h * 16;
  }
  const unsigned char* rB = smemp + OPERA + (wn * 64 + li) * PITCH + h * 16;
  // weight slab of step s = (cs, i): K order = channel slab outer, tap inner -> image slab ORDER[i] * C32 + cs
  const int nsteps = R.C32 * TAPS;
  auto slab_of = [&](int s) {
    if (s >= nsteps) s = 0;                      // (past the end: re-read, never used)
    const int c2 = s / TAPS, i2 = s - c2 * TAPS;
    const int t2 = i2 == 0 ? 0 : (i2 == 1 ? 3 : (i2 == 2 ? 1 : (i2 == 3 ? 4 : 2)));
    return t2 * R.C32 + c2;
  };
  {
    // channel slab 0, all three planes at once (the fragment registers are still free)
    u32x4 x1[NJA], x2[NJA];
    gloadA(xa, 0, 0);
    gloadA(x1, 1, 0);
    gloadA(x2, 2, 0);
    gloadB(slab_of(0));
    storeA(xa, 0);
    storeA(x1, 1);
    storeA(x2, 2);
    storeB(0);
  }
  gloadA(xa, 0, 1 < R.C32 ? 1 : 0);
  gloadB(slab_of(1));
  lds_barrier();
  if (grp == 1) lds_barrier();                   // group 1 runs one slot behind
  int step = 0;
  for (int cs = 0; cs < R.C32; ++cs) {
#pragma unroll
    for (int i = 0; i < TAPS; ++i, ++step) {
      const int t = ORDER[i], cls = t % STRIDE, buf = step & 1;
      // ---- read slot: this step's fragments ([ks][piece: 0 hi, 1 lo][sub-tile]); my share of the next weight
      // slab; request the one after
      f16x8 fa[2][2][2], fb[2][2][2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            fa[ks][p][s] = *reinterpret_cast<const f16x8*>(rA[s] + cls * PLANE + (t / STRIDE) * PITCH + p * 64 + ks * 32);
            fb[ks][p][s] = *reinterpret_cast<const f16x8*>(rB + buf * OPERB + p * 64 + s * 32 * PITCH + ks * 32);
          }
      storeB(buf ^ 1);
      gloadB(slab_of(step + 2));
      lds_barrier();
      // ---- MFMA slot (the other group reads meanwhile).  A plane whose last tap this was is replaced (its only
      // readers are this group's waves, whose reads were complete before the barrier above), and the stage
      // requests the plane that dies next
      if (i == 1 || i == 3 || i == 4) {
        const int dead = i == 1 ? 0 : (i == 3 ? 1 : 2), next = i == 4 ? 0 : dead + 1;
        if (cs + 1 < R.C32) storeA(xa, dead);
        const int ncs = i == 4 ? cs + 2 : cs + 1;
        gloadA(xa, next, ncs < R.C32 ? ncs : 0);   // (past the end: re-read, never stored)
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

// stride-3 windows of 5 positions over a multiple of 128 channels (x6_tap3_ok), on 256 x 128 tiles
int f2g_h3p3_ok(const f2g_gemm_desc& d) {
  if (!h3_tap_fwd_ok(d, 256, 128, true) || !x6_tap3_ok(d, LP)) return 0;
  return f16_images_status(d.A, d.B, 7);
}

int f2g_launch_h3p3(const f2g_gemm_desc& d, hipStream_t st) {
  const int M = d.A.rows, N = d.B.rows, K = d.A.cols;
  dyn_lds_once<gemm_h3p3_kernel<5, 3>>((int)SMEM);
  h3p3_tap R;
  R.P0 = d.A.P0, R.HpIn = (int)(d.A.seq_stride / d.A.unit), R.offpos = -d.A.pad0, R.C32 = d.A.unit / 32;
  R.nseq = M / R.P0;
  R.bytes = (unsigned)(x6_a_extent(d.A) * 4);
  dim3 grid((M + 255) / 256, (N + 127) / 128);
  f2g_note_kernel("h3p<taps=5,step=3>", 1, 6);
  hipLaunchKernelGGL((gemm_h3p3_kernel<5, 3>), grid, dim3(512), SMEM, st, d, M, N, K, R);
  return f2g_check_launch();
}
