// fp16x3 tap-walking weight gradient of the MPD's 32 -> 128 layer (five taps, stride 3; in the bf16x6 mode the launch
// runs on the generic exact-fp32 kernel with a K split: gemm_leanw6s_kernel, gemm_x6p.hip, wants a multiple of 128
// channels), SCALED INSIDE THE KERNEL:
//   gw[co][t * 32 + ci] += sum over (s, p) of g[s * Hp + p][co] * x[s * HpIn + STRIDE * p + t - pad0][ci],  t = 0..TAPS-1
// g is the plain fp32 gradient matrix (nseq * Hp x 128), x the fp32 halo map under unbounded stride-3 windows of five
// positions, unit = 32 (both operands marked f2g_operand.split = 8).  Both are read AS FP32, EVERY ELEMENT ONCE: there
// are no images and no rscale.  The launch is an HBM stream -- 306 MB at B = 64, period 2, against 14 GFLOP -- and the
// column-image route of gemm_h3ws_kernel (gemm_f16ws.hip) would pay 12 + 4 bytes per element for it.
//
// THE WALK.  The whole output (128 x 160) is ONE tile: a block owns all of it.  The walk unit is gemm_h3ws_kernel's
// slab -- R = 16 gradient rows of one sequence (one MFMA k step) and the XR = STRIDE * 15 + TAPS = 50 map rows they
// touch, every map row staged once for all taps; fragment row of reduction index i and tap t = staged row STRIDE * i +
// t.  Units are numbered sequence-major, nseq * ceil(Hp / 16) in all; block b of `blocks` takes the contiguous range
// [b * units / blocks, (b + 1) * units / blocks), which may cut a sequence between slabs (h3wsn_blocks has the grid
// rule).  Addressing is gemm_h3ws_kernel's: map rows in front of or behind the buffer and slab rows beyond Hp read as
// zeros (offset 0x80000000: outside the buffer resource, never fetched).
//
// ONE MONOTONE RUNNING SCALE PER OPERAND AND BLOCK, conv32h3w.hip's rule: m_run starts at 0 = scale 1; before slab T is
// split m_run = max(m_run, m_T) over every staged float of the slab (halo and overhang rows included; the zeros
// substituted outside the buffer do not count), a slab whose maximum is zero or not finite leaves m_run alone and is
// split at the scale in force; (s, rs) = f2g_f16_scales(m_run).  When a scale moves, both accumulator sets are
// multiplied by s_new / s_old before the slab's first MFMA (a wave-uniform branch, not taken while the scales stand).
// v = h3_value(acc, acx, rs_x, rs_g) leaves through atomic adds, the reciprocals one after the other.  The maxima are
// integer maxima of sign-less bit patterns (thread, wave butterfly, one LDS word per wave and operand): a block's
// contribution is reproducible, only the atomic adds between blocks reorder.  Per output
//   |err| <= 3 * 2^-22 sum |g||x| + 2^-28 sum_T (xrun_T sum_{rows in T} |g| + grun_T sum_{rows in T} |x_win|)
// with the running maxima in force at slab T (tests/fp16x3_runwin3_emul.py).
//
// THE PIPELINE.  256 threads; wave w owns output rows 32 w .. 32 w + 31 x 32 ci x TAPS x 2 sets = 160 accumulator
// registers.  A slab is 2 + 2 chunks of 16 bytes per thread.  While slab j's MFMAs run, slab j + 1 goes from registers
// -- its maxima met in LDS behind the barrier that closed slab j - 1 -- through the split at the new scales straight
// into the other LDS stage, and TWO slabs of loads are in flight: j + 2 (requested a slab earlier, waited for at the end
// of this one, where its maxima are posted) and j + 3 (requested into the registers the split has just freed).  One
// barrier per slab; the maxima words are double-buffered by slab parity (a wave may post slab j + 2's while another
// still reads slab j + 1's).  Two blocks per CU: 2 x 2 x 14.4 KB of loads in flight per CU.
//
// LDS: stage = [g hi | g lo | x hi | x lo].  A gradient row is 128 halves = 256 bytes with gemm_h3ws_kernel's swizzle
// (the row's four 64-byte column blocks rotated by row & 3).  A map row is 32 halves = ONE 64-byte block per plane
// here, pitch 64, so that kernel's swap of a row's two blocks has nothing to swap -- and nothing to repair: the
// 64-byte bank group of staged row q is q & 3 (four rows per 256-byte bank line), and the four reduction rows of one
// half of a transposing read are the staged rows r, r + 3, r + 6, r + 9, whose residues modulo 4 are r, r + 3, r + 2,
// r + 1: four different bank groups for every r (any tap's first row), because the stride is odd (static_assert
// below).  The second half of a read lies 4 * STRIDE = 12 rows = 768 bytes further: the same residues.  The split
// stores are ds_write_b64: 16 lanes write two whole map rows (128 contiguous bytes) or two 64-byte blocks of one
// gradient row whose swizzled indices differ in bit 0 -- 32 different banks either way.
//
// RESOURCES (tools/kernel_resources.py, gfx950), <5, 3>: 246 VGPRs, 0 AGPRs, 0 scratch, 0 vector or scalar spills, 2
// waves per SIMD (two blocks per CU); 29248 bytes of LDS (two stages of 2 x 4096 gradient and 2 x 3200 map bytes, 16
// maxima words).  The fragments of ONE tap beyond the running one are read ahead and no more (a scheduling barrier per
// tap): with all five taps' reads hoisted above the MFMAs the kernel needs 40 registers more and spills.
// MEASURED: tools/fp16x3_tapw_shapes.py --step3n -> profiles/fp16x3_tapw3n_shapes.txt; DESIGN.md section 0 has the
// numbers and what they say.
#include <stddef.h>
#include <stdint.h>

#include "gemm_f16_checks.h"
#include "gemm_f16_common.h"
#include "split_f16.h"

namespace {

constexpr int R = 16;                      // gradient rows of a slab
constexpr int NTHR = 256;
constexpr int GP = 256, XP = 64;           // row pitches of a plane
constexpr int GPL = R * GP;                // bytes of one gradient plane
constexpr int XROWB = 32 * 4;               // bytes of a map row in memory

struct h3wsn_args {
  const float* g;
  const float* x;
  float* C;
  long long ldc;
  unsigned gbytes, xbytes, rowG;           // buffer extents; bytes of a gradient row
  int nseq, Hp, HpIn, pad, nslab, units, xrows;
};

__device__ __forceinline__ float4 f4u(const u32x4 v) {
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// a chunk's two pieces into the hi plane (p) and the lo plane (p + plane_bytes)
__device__ __forceinline__ void h3wsn_put(unsigned char* p, int plane_bytes, const u32x4 v, float s) {
  const uint4 q = f2g_f16_split4(f4u(v), s);
  *reinterpret_cast<u32x2*>(p) = u32x2{q.x, q.y};
  *reinterpret_cast<u32x2*>(p + plane_bytes) = u32x2{q.z, q.w};
}

template <int TAPS, int STRIDE>
__global__ __launch_bounds__(NTHR, 2) void gemm_h3wsn_kernel(const h3wsn_args a) {
  constexpr int XR = (R - 1) * STRIDE + TAPS;    // staged map rows of a slab
  constexpr int XPL = XR * XP;                   // bytes of one map plane
  constexpr int XOFF = 2 * GPL;
  constexpr int BUFB = 2 * GPL + 2 * XPL;        // one stage
  constexpr int NGQ = R * 32 / NTHR;             // gradient chunks per thread: 2
  constexpr int NXQ = (XR * 8 + NTHR - 1) / NTHR;   // map chunks per thread: 2
  static_assert(STRIDE % 2 == 1, "staged rows STRIDE apart must walk all four 64-byte bank groups");
  static_assert(NGQ * NTHR == R * 32 && NXQ == 2 && XR > 32, "a gradient slab in whole chunks per thread");
  extern __shared__ __attribute__((aligned(16))) unsigned char sms[];
  unsigned* smx = reinterpret_cast<unsigned*>(sms + 2 * BUFB);   // [slab parity][x, g][4 waves]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, h = lane >> 5;
  // this block's units (h3wsn_blocks: never an empty range)
  const int u0 = (int)((long long)blockIdx.x * a.units / gridDim.x);
  const int nt = (int)((long long)(blockIdx.x + 1) * a.units / gridDim.x) - u0;
  if (nt <= 0) return;
  __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)a.g, 0, a.gbytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.xbytes, 0x00020000);
  // staging: gradient chunk cc of slab rows rg + 8 q, map chunk cx of staged rows rx + 32 q
  const int cc = tid & 31, rg = tid >> 5, cx = tid & 7, rx = tid >> 3;
  const unsigned colG = (unsigned)cc * 16u, colX = (unsigned)cx * 16u;
  // (row rg + 8 q keeps row & 3, so its chunk lies 8 rows further; map row rx + 32 exists for tid < 8 (XR - 32))
  const int wofG = rg * GP + ((((cc >> 3) ^ (rg & 3))) << 6) + (cc & 7) * 8;
  const int wofX = XOFF + rx * XP + cx * 8;
  const bool xrow2 = tid < 8 * (XR - 32);
  // transposed-read roles (gemm_h3ws_kernel): 16-lane group g4, lane i16 -> row (g4 >> 1) * 8 + (i16 >> 2) (+4 for the
  // second half), 8 bytes at (g4 & 1) * 32 + (i16 & 3) * 8 of the 64-byte column block
  const int g4 = lane >> 4, i16 = lane & 15;
  const int rrow = (g4 >> 1) * 8 + (i16 >> 2), within = (g4 & 1) * 32 + (i16 & 3) * 8;
  const int rofA = rrow * GP + (((wave ^ (rrow & 3))) << 6) + within;
  const int rofB = XOFF + STRIDE * rrow * XP + within;       // tap t: + t * XP
  f32x16 acc[TAPS], acx[TAPS];
  h3_zero<TAPS>(acc, acx);

  struct slab {
    u32x4 g[NGQ], x[NXQ];
  };
  // slab j of this block: unit u0 + j = (sequence, gradient rows p0 .. p0 + 15); past the block's last one: zeros
  auto gload = [&](int j, slab& s) {
    const bool on = j < nt;
    const int u = u0 + j, sq = u / a.nslab, p0 = (u - sq * a.nslab) * R;
    // (the whole offset in the vector register; a row that is not read has its offset replaced, not used.  Row indices
    // fit an int: both byte extents are below 2^31)
#pragma unroll
    for (int q = 0; q < NGQ; ++q) {
      const int p = p0 + rg + 8 * q;
      s.g[q] = __builtin_amdgcn_raw_buffer_load_b128(
          ra, (on && p < a.Hp) ? (unsigned)(sq * a.Hp + p) * a.rowG + colG : 0x80000000u, 0, 0);
    }
    const int xb = sq * a.HpIn + STRIDE * p0 - a.pad;     // map row of staged row 0
#pragma unroll
    for (int q = 0; q < NXQ; ++q) {
      const int xr = xb + rx + 32 * q;
      const bool ok = on && (q == 0 || xrow2) && xr >= 0 && xr < a.xrows;
      s.x[q] = __builtin_amdgcn_raw_buffer_load_b128(rb, ok ? (unsigned)xr * XROWB + colX : 0x80000000u, 0, 0);
    }
  };
  // the maxima of the slab in the registers, per wave, into the words of its parity (read behind the next barrier)
  auto post_amax = [&](const slab& s, int par) {
    unsigned mx = 0, mg = 0;
#pragma unroll
    for (int q = 0; q < NXQ; ++q) mx = f2g_f16_amax4(f4u(s.x[q]), mx);
#pragma unroll
    for (int q = 0; q < NGQ; ++q) mg = f2g_f16_amax4(f4u(s.g[q]), mg);
    mx = f2g_wave_max(mx);
    mg = f2g_wave_max(mg);
    if (lane == 0) smx[par * 8 + wave] = mx, smx[par * 8 + 4 + wave] = mg;
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
  auto put = [&](unsigned char* buf, const slab& s, float sg, float sx) {
#pragma unroll
    for (int q = 0; q < NGQ; ++q) h3wsn_put(buf + wofG + q * 8 * GP, GPL, s.g[q], sg);
#pragma unroll
    for (int q = 0; q < NXQ; ++q)
      if (q == 0 || xrow2) h3wsn_put(buf + wofX + q * 32 * XP, XPL, s.x[q], sx);
  };

  unsigned mrx = 0u, mrg = 0u;             // the running maxima; 0 = scale 1
  float sx = 1.f, rsx = 1.f, sg = 1.f, rsg = 1.f;
  slab sa, sb;
  gload(0, sa);
  gload(1, sb);
  post_amax(sa, 0);
  lds_barrier();
  {
    float f;
    next_scale(smx, mrx, sx, rsx, f);      // (the accumulators are zero: no rescale)
    next_scale(smx + 4, mrg, sg, rsg, f);
  }
  put(sms, sa, sg, sx);
  gload(2, sa);
  post_amax(sb, 1);
  lds_barrier();
  // slab j: `nxt` holds slab j + 1 (landed, its maxima posted), `aft` slab j + 2 (in flight)
  auto step = [&](int j, slab& nxt, slab& aft) {
    const unsigned char* cur = sms + (j & 1) * BUFB;
    const int pn = (j + 1) & 1;
    float fx, fg;
    next_scale(smx + pn * 8, mrx, sx, rsx, fx);
    next_scale(smx + pn * 8 + 4, mrg, sg, rsg, fg);
    const f16x8 ah = tr_frag_f16<GP>(cur + rofA);
    const f16x8 al = tr_frag_f16<GP>(cur + GPL + rofA);
    // slab j + 1 goes into the other stage (its readers left through the barrier that closed slab j - 1), slab j + 3
    // is requested into its registers
    put(sms + pn * BUFB, nxt, sg, sx);
    gload(j + 3, nxt);
    // (the loads stay in front: left to itself the scheduler sinks them to the barrier)
    __builtin_amdgcn_sched_barrier(0);
    // (the second half of a read: 4 reduction rows = 4 * STRIDE staged rows further.)  The next tap's fragments are
    // read under this tap's MFMAs and no further ahead: hoisted above the MFMAs, all five taps' cost 40 registers
    // and spill
    f16x8 bh[2], bl[2];
    bh[0] = tr_frag_f16<XP, 4 * STRIDE>(cur + rofB);
    bl[0] = tr_frag_f16<XP, 4 * STRIDE>(cur + XPL + rofB);
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      if (t + 1 < TAPS) {
        bh[(t + 1) & 1] = tr_frag_f16<XP, 4 * STRIDE>(cur + rofB + (t + 1) * XP);
        bl[(t + 1) & 1] = tr_frag_f16<XP, 4 * STRIDE>(cur + XPL + rofB + (t + 1) * XP);
      }
      h3_product(acc[t], acx[t], ah, al, bh[t & 1], bl[t & 1]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (fx != 1.f || fg != 1.f) {          // a scale moved: the stored sums go over to slab j + 1's
#pragma unroll
      for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          acc[t][e] = acc[t][e] * fx * fg;
          acx[t][e] = acx[t][e] * fx * fg;
        }
    }
    post_amax(aft, j & 1);                 // slab j + 2 has landed under the MFMAs
    lds_barrier();
  };
  int j = 0;
  for (; j + 1 < nt; j += 2) {
    step(j, sb, sa);
    step(j + 1, sa, sb);
  }
  if (j < nt) step(j, sb, sa);
  // gw[co][t * 32 + ci] += (acc + 2^-11 acx) / s_x / s_g (gemm_f16_common.h: h3_value): rows wave * 32 + (MFMA row),
  // columns t * 32 + li -- a wave instruction adds two 128-byte segments in two rows
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int row = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
    float* crow = a.C + (long long)row * a.ldc + li;
#pragma unroll
    for (int t = 0; t < TAPS; ++t) atomicAdd(crow + t * 32, h3_value(acc[t][e], acx[t][e], rsx, rsg));
  }
}

// THE GRID RULE: blocks of a walk of `units` slabs -- at most two per CU (256 CUs), and at least 256 reduction rows =
// 16 slabs for every block unless the grid is one block; block b takes the units [b * units / blocks, (b + 1) * units /
// blocks) (tests/fp16x3_runwin3_emul.py: partition restates it)
int h3wsn_blocks(long long units) {
  long long blocks = units / (256 / R);
  if (blocks > 2 * 256) blocks = 2 * 256;
  return blocks < 1 ? 1 : (int)blocks;
}

}  // namespace

// Form 2 at precision 4 with an operand marked split = 8: BOTH operands are so marked and carry no rscale (there are no
// images); f2g_h3ws_ok's conditions (gemm_f16ws.hip) with A of 128 columns and B over 32 channels.  1 = runs as handed
// over, 0 = not for this kernel (there is no 2: nothing has to be made first).
int f2g_h3wsn_ok(const f2g_gemm_desc& d) {
  const f2g_operand& A = d.A;
  const f2g_operand& B = d.B;
  if (A.split != 8 || B.split != 8 || A.rscale || B.rscale) return 0;
  if (!h3_tapw_ok(d, 3) || A.cols != 128 || B.unit != 32 || d.E.ldc < B.cols) return 0;
  const long long HpIn = h3_tapw3_map_rows(B);
  return HpIn && h3_tapw_extents_ok(A, B, HpIn) ? 1 : 0;
}


int f2g_launch_h3wsn(const f2g_gemm_desc& d, hipStream_t st) {
  constexpr int TAPS = 5, STRIDE = 3;
  constexpr size_t smem = (size_t)2 * (2 * GPL + 2 * ((R - 1) * STRIDE + TAPS) * XP) + 2 * 2 * 4 * sizeof(unsigned);
  h3wsn_args a;
  a.g = d.A.base, a.x = d.B.base, a.C = d.E.C;
  a.ldc = d.E.ldc;
  a.nseq = d.A.rows / d.B.P0, a.Hp = d.B.P0, a.HpIn = (int)(d.B.seq_stride / d.B.unit), a.pad = d.B.pad0;
  a.nslab = (a.Hp + R - 1) / R;
  a.xrows = a.nseq * a.HpIn;      // (f2g_h3wsn_ok: below 2^24)
  a.rowG = (unsigned)(d.A.seq_stride * 4);
  a.gbytes = (unsigned)((long long)d.A.rows * d.A.seq_stride * 4);
  a.xbytes = (unsigned)a.xrows * XROWB;
  const long long units = (long long)a.nseq * a.nslab;
  a.units = (int)units;
  f2g_note_kernel("h3wsn<taps=5,step=3>", 1, 6);
  hipLaunchKernelGGL((gemm_h3wsn_kernel<5, 3>), dim3(h3wsn_blocks(units)), dim3(NTHR), smem, st, a);
  return f2g_check_launch();
}
