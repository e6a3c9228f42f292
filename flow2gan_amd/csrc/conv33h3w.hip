// fp16x3 weight gradient of the (3, 3) fifth layer of an MRD band stack (conv33h3.hip has the forward and the data
// gradient, conv32x6.hip the bf16x6 kernel this one is built after: conv33_wgrad6_kernel; conv32h3w.hip the (3, 9)
// layers' kernel whose arithmetic it shares):
//   gw[co][tap][ci] += sum_px g[px][co] * x[px + tap][ci],
// MFMA rows = co, columns = ci, reduction = the pixels of a block's tiles.  Geometry and walk are
// conv33_wgrad6_kernel's: a tile is R whole rows (c33_pick_rows), the patch (R + 2) x (W + 2) with a zero border and
// the gradient rows staged in that same padded flat order, so the nine taps are nine constant flat offsets and a k
// step is 16 consecutive flat positions; min(ntiles, 256) persistent blocks walk the tiles b, b + grid, ... and keep
// their accumulators over all of them.  Both operands are staged as TWO planes (hi, lo: split_f16.h) of 64-byte
// pixels and read through ds_read_b64_tr_b16; a product is three v_mfma_f32_32x32x16_f16 into two accumulator sets
// (gemm_f16_common.h): 27 MFMAs per k step instead of 54, 92 KB of LDS instead of 138.
//
// ONE MONOTONE RUNNING SCALE PER OPERAND AND BLOCK (conv32h3w.hip's rule on this walk).  m_run, the largest sign-less
// bit pattern seen so far in the operand (x: every float of the patch rows h0 - 1 .. h0 + R, halo rows included; g:
// the tile's R x W gradient rows; the zero border and rows outside the map are staged from zeros and so count for
// nothing), starts at 0 = scale 1.  Before tile T is split m_run = max(m_run, m_T) (a tile whose maximum is zero or not
// finite leaves it alone), (s, rs) = f2g_f16_scales(m_run).  The maxima come from the registers that hold the tile's
// loads: thread maximum, f2g_wave_max, eight LDS words per operand behind a barrier -- the barrier that also ends the
// previous tile's reads of the planes, so a tile costs two barriers as in conv33_wgrad6_kernel.  When a scale moves,
// both accumulator sets are multiplied by s_new / s_old (a power of two, at most 1 once the block has met a finite
// nonzero tile) in a wave-uniform branch before the tile's first MFMA.  At the end v = (acc0 + 2^-11 acc1) * rs_x *
// rs_g.  Per output
//   |err| <= 3 * 2^-22 sum |g||x| + 2^-28 sum_T (xrun_T sum_{px in T} |g| + grun_T sum_{px in T} |x|).
//
// ACCUMULATORS.  Nine taps x two sets x 16 registers = 288 do not fit a wave's 256, so the taps are split over two
// groups of four waves (group = wave >> 2: a SIMD holds one wave of each).  A group's four waves take the k steps
// round-robin.  Group 0 owns the taps 0..3, group 1 the taps 5..8; the centre tap 4 is taken by group 0 on a wave's
// even turns and by group 1 on its odd ones (13.5 MFMA triples per k step and wave on either side): five tap tiles =
// 160 accumulator registers per wave.  Every tap is therefore partial in the four (tap 4: eight) waves that hold it:
// the flush folds and unscales first, so ONE float per element goes through LDS, sums over the holders and emits one
// atomic per output and block.  The next tile's loads are not requested ahead: 48 more live registers under the
// MFMAs do not fit beside 160 accumulators without spills.
#include <stdlib.h>

#include "conv32_common.h"
#include "gemm_f16_common.h"
#include "split_f16.h"

namespace {

constexpr int W33H_PLANES = 2 * (W33_XPL + W33_GPL);                 // hi and lo plane of either operand: 94208 bytes
constexpr size_t W33H_SMEM = (size_t)W33H_PLANES + 2 * 8 * sizeof(unsigned);   // + the waves' maxima of the two operands
constexpr int W33H_SLOTS = 5;                                        // tap tiles per wave
static_assert(W33H_PLANES >= 8 * 16 * 64 * 4, "the flush reuses the planes as its reduction buffer");
static_assert(W33H_SMEM <= 160 * 1024, "LDS of a CU");

__device__ __forceinline__ float4 f4(const f32x4 v) { return make_float4(v.x, v.y, v.z, v.w); }

// a chunk's two pieces into the hi plane (p) and the lo plane (p + plane_bytes)
__device__ __forceinline__ void store_planes2(unsigned char* p, int plane_bytes, const f32x4 v, float s) {
  const uint4 q = f2g_f16_split4(f4(v), s);
  *reinterpret_cast<u32x2*>(p) = u32x2{q.x, q.y};
  *reinterpret_cast<u32x2*>(p + plane_bytes) = u32x2{q.z, q.w};
}

// tap of slot a of wave group grp: 0..3 / 5..8 owned, slot 4 = the shared centre tap
__device__ __forceinline__ int w33h_tap(int grp, int a) { return a < 4 ? 5 * grp + a : 4; }

// flush: slot by slot the waves' folded, unscaled partial tiles meet in LDS (red: [8 waves][16][64 lanes] floats, the
// planes, dead by now); slots 0..3 hold one tap per group, summed over the group's four waves by its wave a; slot 4
// holds the centre tap, summed over all eight by wave 0.  One atomic per output and block.
__device__ __forceinline__ void c33_wgrad_flush_h3(float* gw, float* red_, const f32x16 (&acc)[W33H_SLOTS],
                                                   const f32x16 (&acx)[W33H_SLOTS], int wave, int lane, int li, int hh,
                                                   float rsx, float rsg) {
  typedef float __attribute__((address_space(3))) * lds_f;
  const lds_f red = (lds_f)red_;
  const int grp = wave >> 2;
#pragma unroll
  for (int a = 0; a < W33H_SLOTS; ++a) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 16; ++e) red[(wave * 16 + e) * 64 + lane] = h3_value(acc[a][e], acx[a][e], rsx, rsg);
    __syncthreads();
    const int first = a < 4 ? 4 * grp : 0, holders = a < 4 ? 4 : 8;
    if (wave == (a < 4 ? 4 * grp + a : 0)) {
      const int t = w33h_tap(grp, a);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float v = 0.f;
#pragma unroll
        for (int w8 = 0; w8 < 8; ++w8)
          if (w8 < holders) v += red[((first + w8) * 16 + e) * 64 + lane];
        atomicAdd(gw + (acc_row(e) + 4 * hh) * (T33 * C) + t * C + li, v);
      }
    }
  }
}

__global__ __launch_bounds__(512, 1) void conv33_wgrad3h_kernel(const f2g_conv32_desc d, float* gw, int R, int tiles_h,
                                                                int ntiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smb[];
  unsigned char* Xp = smb;                      // [2 pieces][W33_XP] pixels x 32 halves; position 0 = slack
  unsigned char* Gp = smb + 2 * W33_XPL;        // [2 pieces][W33_GP]
  unsigned* smx = reinterpret_cast<unsigned*>(smb + W33H_PLANES);   // [x, g][8 waves] maxima of the tile being staged
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2, turn0 = wave & 3;
  const int li = lane & 31, hh = lane >> 5;
  const int W = d.Win, PW = W + 2, npx = (R + 2) * PW, ngp = R * PW, nks = (ngp + 15) >> 4;
  const unsigned mgPW = magic_of(PW);
  // everything a fragment may touch and a tile does not rewrite (slack position, k-step overhang) is zero
  for (int o = tid * 16; o < W33H_PLANES; o += 512 * 16) *reinterpret_cast<u32x4*>(smb + o) = u32x4{0u, 0u, 0u, 0u};
  // chunk id = tid + 512 q -> (flat position, 4 channels)
  constexpr int NQ = (W33_GP * 8 + 511) / 512;          // 6: covers the patch (<= 352 positions) and the gradient rows
  const int c4 = tid & 7;
  // chunk q's place in the patch / the gradient rows: row relative to h0 (< -2^20: border = zeros; < -2^21: not
  // staged) and source offset.  Recomputed per tile: 24 registers held across the MFMAs would not fit beside the
  // accumulators (the empty asm keeps the arithmetic inside the tile loop: conv32_s2_fwd3h_kernel)
  auto x_place = [&](int q, int& row, int& off) {   // input patch position px = (pr + 1) * PW + (pc + 1)
    int tb = tid;
    asm volatile("" : "+v"(tb));
    const int px = (tb + 512 * q) >> 3;
    const int pr = fast_div(px, PW, mgPW), pc = px - pr * PW;
    const bool ok = px < npx && pc >= 1 && pc <= W;
    row = px < npx ? (ok ? pr - 1 : -(1 << 20)) : -(1 << 21);
    off = (pr - 1) * (int)d.x_line + (pc - 1) * C + c4 * 4;
  };
  auto g_place = [&](int q, int& row, int& off) {   // gradient position px = r * PW + (c + 1)
    int tb = tid;
    asm volatile("" : "+v"(tb));
    const int px = (tb + 512 * q) >> 3;
    const int r = fast_div(px, PW, mgPW), pc = px - r * PW;
    const bool ok = px < ngp && pc >= 1 && pc <= W;
    row = px < ngp ? (ok ? r : -(1 << 20)) : -(1 << 21);
    off = r * (int)d.y_line + (pc - 1) * C + c4 * 4;
  };
  // transposed-read lane roles (conv32_s2_wgrad6_kernel): 16-lane group g4 = (channel half, k half)
  const int g4 = lane >> 4, i16 = lane & 15;
  const int kpix = (g4 >> 1) * 8 + (i16 >> 2);
  const int chb = (g4 & 1) * 32 + (i16 & 3) * 8;
  const int go = kpix * 64 + chb;
  int xo[W33H_SLOTS];
#pragma unroll
  for (int a = 0; a < W33H_SLOTS; ++a) {
    const int t = w33h_tap(grp, a);
    xo[a] = (1 + PW + (t / 3 - 1) * PW + (t % 3 - 1) + kpix) * 64 + chb;
  }
  f32x16 acc[W33H_SLOTS], acx[W33H_SLOTS];
  h3_zero<W33H_SLOTS>(acc, acx);
  unsigned mrx = 0u, mrg = 0u;             // the running maxima; 0 = scale 1
  float sx = 1.f, rsx = 1.f, sg = 1.f, rsg = 1.f;
  // the running scale of one operand moves on to the tile whose maxima are in m8; f = s_new / s_old
  auto next_scale = [&](const unsigned* m8, unsigned& mrun, float& s, float& rs, float& f) {
    unsigned m = m8[0];
#pragma unroll
    for (int w8 = 1; w8 < 8; ++w8) m = m > m8[w8] ? m : m8[w8];
    m = (unsigned)__builtin_amdgcn_readfirstlane((int)m);
    if (m != 0u && m < 0x7f800000u && m > mrun) mrun = m;   // (a zero or non-finite tile: the scale in force)
    float sn, rsn;
    f2g_f16_scales(mrun, sn, rsn);
    f = sn * rs;
    s = sn;
    rs = rsn;
  };
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int sq = tile / tiles_h, h0 = (tile - sq * tiles_h) * R;
    const float* xs = d.x + (long long)sq * d.x_seq + (long long)h0 * d.x_line;
    const float* gs = d.y + (long long)sq * d.y_seq + (long long)h0 * d.y_line;
    f32x4 px_[NQ], pg_[NQ];
    unsigned mx = 0u, mg = 0u;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      int xrow, xoff, grow, goff;
      x_place(q, xrow, xoff);
      g_place(q, grow, goff);
      const int hx = h0 + xrow, hg = h0 + grow;
      px_[q] = *reinterpret_cast<const f32x4*>((xrow > -(1 << 20) && hx >= 0 && hx < d.H) ? xs + xoff : c32_zero);
      pg_[q] = *reinterpret_cast<const f32x4*>((grow > -(1 << 20) && hg < d.H) ? gs + goff : c32_zero);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      mx = f2g_f16_amax4(f4(px_[q]), mx);
      mg = f2g_f16_amax4(f4(pg_[q]), mg);
    }
    mx = f2g_wave_max(mx);
    mg = f2g_wave_max(mg);
    if (lane == 0) smx[wave] = mx, smx[8 + wave] = mg;
    __syncthreads();   // the maxima are posted; every wave is done with the previous tile's planes
    float fx, fg;
    next_scale(smx, mrx, sx, rsx, fx);
    next_scale(smx + 8, mrg, sg, rsg, fg);
    if (fx != 1.f || fg != 1.f) {          // a scale moved: the stored sums go over to the new one
#pragma unroll
      for (int a = 0; a < W33H_SLOTS; ++a)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          acc[a][e] = acc[a][e] * fx * fg;
          acx[a][e] = acx[a][e] * fx * fg;
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int px = (tid + 512 * q) >> 3;             // (staged: px < npx / px < ngp, x_place / g_place)
      if (px < npx) store_planes2(Xp + (px + 1) * 64 + c4 * 8, W33_XPL, px_[q], sx);
      if (px < ngp) store_planes2(Gp + px * 64 + c4 * 8, W33_GPL, pg_[q], sg);
    }
    __syncthreads();   // the tile is staged (and smx may be rewritten)
    int turn = 0;
    for (int ks = turn0; ks < nks; ks += 4, turn ^= 1) {
      f16x8 a[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) a[q] = tr_frag_f16<64>(Gp + q * W33_GPL + ks * (16 * 64) + go);
#pragma unroll
      for (int t = 0; t < W33H_SLOTS; ++t) {
        if (t == 4 && turn != grp) break;  // the centre tap: group 0 on even turns, group 1 on odd ones (wave-uniform)
        f16x8 b[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) b[q] = tr_frag_f16<64>(Xp + q * W33_XPL + ks * (16 * 64) + xo[t]);
        h3_term(1, acc[t], acx[t], a[0], a[1], b[0], b[1]);
        h3_term(0, acc[t], acx[t], a[0], a[1], b[0], b[1]);
        h3_term(2, acc[t], acx[t], a[0], a[1], b[0], b[1]);
      }
    }
  }
  c33_wgrad_flush_h3(gw, reinterpret_cast<float*>(smb), acc, acx, wave, lane, li, hh, rsx, rsg);
}

}  // namespace

// gw (32, 9 * 32) += the fp16x3 weight gradient of the (3, 3) band layer (include/flow2gan_hip.h)
extern "C" int f2g_conv33_wgrad_h3(const f2g_conv32_desc* d, float* gw, f2g_stream_t stream) {
  if (!d || !d->x || !d->y || !gw || d->precision != 4 || d->Win != d->Wout) return F2G_EINVAL;
  if ((((uintptr_t)d->x) & 15) || (((uintptr_t)d->y) & 15) || (d->x_line & 3) || (d->x_seq & 3) || (d->y_line & 3) ||
      (d->y_seq & 3))
    return F2G_EINVAL;
  if (d->S <= 0 || d->H <= 0 || d->Win <= 0) return F2G_OK;
  const int W = d->Win;
  if (W > 112 || d->x_line >= (1ll << 24) || d->y_line >= (1ll << 24) || d->x_line < (long long)W * C ||
      d->y_line < (long long)W * C)
    return F2G_EINVAL;
  const int R = c33_pick_rows(d->H, W);              // whole rows per tile (conv33_wgrad6_kernel's rule)
  if (R < 1) return F2G_EINVAL;
  const int tiles_h = (d->H + R - 1) / R;
  const long long nt = (long long)tiles_h * d->S;
  if (nt >= (1ll << 30)) return F2G_EINVAL;
  c32_lds_once<conv33_wgrad3h_kernel>(W33H_SMEM);
  const int grid = (int)(nt < 256 ? nt : 256);          // one resident block per CU: 256 x 9216 atomics at most
  hipLaunchKernelGGL(conv33_wgrad3h_kernel, dim3(grid), dim3(512), W33H_SMEM, (hipStream_t)stream, *d, gw, R, tiles_h,
                     (int)nt);
  return f2g_check_launch();
}
