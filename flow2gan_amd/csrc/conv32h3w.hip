// fp16x3 weight gradient of the direct MRD band convolutions (conv32h3.hip has the forward and the data gradient,
// conv32x6.hip the bf16x6 kernel this one is built after: conv32_s2_wgrad6_kernel):
//   gw[co][tap][ci] += sum_px g[px][co] * x[px -> tap][ci],
// MFMA rows = co, columns = ci, reduction = the pixels of a block's tiles.  Both operands are activations, staged
// as TWO planes (hi, lo: split_f16.h) of 64-byte pixels and read through ds_read_b64_tr_b16; a product is three
// v_mfma_f32_32x32x16_f16 into two accumulator sets (gemm_f16_common.h), 81 per wave and tile instead of 162.
//
// ONE MONOTONE RUNNING SCALE PER OPERAND AND BLOCK.  A block walks `per` consecutive tiles and keeps its 27
// accumulator tiles across them, so a tile's scale does not factor out of the tile alone.  The block keeps m_run, the
// largest sign-less bit pattern seen so far in the operand (x: every float of the staged patch, halo included, zeros
// outside the map; g: the TH x TW gradient tile), starting at 0 = scale 1.  Before tile T is split m_run = max(m_run,
// m_T) (a tile whose maximum is zero or not finite leaves it alone and is split at the scale in force), (s, rs) =
// f2g_f16_scales(m_run).  When a scale moves, both accumulator sets are multiplied by s_new / s_old -- a power of two,
// at most 1 once the block has met a finite nonzero tile, so a stored accumulator only shrinks -- before the new
// tile's first MFMA, the two operands' factors one after the other.  The branch is wave-uniform and not taken while
// the scales stand.  At the end v = (acc0 + 2^-11 acc1) * rs_x * rs_g leaves through the atomic adds.  Per output
//   |err| <= 3 * 2^-22 sum |g||x| + 2^-28 sum_T (xrun_T sum_{px in T} |g| + grun_T sum_{px in T} |x|)
// with the running maxima in force at tile T.
//
// Structure: persistent blocks of 8 waves, one per CU.  EVERY wave owns whole taps over all pixels -- wave w the taps
// w, w + 8, w + 16 and, waves 0..2, tap 24 + w: 4 x 2 x 16 = 128 accumulator registers, SIMD pairs (w, w + 4) carry 7,
// 7, 7 and 6 taps --, so the flush has no cross-wave reduction.  The staged image is DOUBLE-BUFFERED: the next tile's
// rows are requested into registers a tile ahead; after half of the current tile's k steps their maxima meet in LDS
// behind one barrier, and the chunks are split at the new scales straight into the other buffer under the MFMAs of
// the second half -- no registers hold split pieces.  2 x 71.9 KB for the 16 x 8 shape.
#include <stdlib.h>

#include "conv32_common.h"
#include "gemm_f16_common.h"
#include "split_f16.h"

namespace {

constexpr int NTAP = KH * KW;
constexpr int GPL = 128 * 64;            // bytes of one plane of the gradient tile
constexpr int GCH = 128 * (C / 4) / 512; // gradient chunks per thread: 2

template <int TH, int TW>
constexpr int wgrad3h_buf() {   // one staged tile: two planes of the patch's two column parities and of the gradient tile
  return 2 * 2 * ((TH + KH - 1) * (TW + (KW - 1) / 2) * 64 + 64) + 2 * GPL;
}
template <int TH, int TW>
constexpr size_t wgrad3h_smem() {   // two staged tiles and the waves' maxima of the two operands
  return (size_t)2 * wgrad3h_buf<TH, TW>() + 2 * 8 * sizeof(unsigned);
}

__device__ __forceinline__ float4 f4(const f32x4 v) { return make_float4(v.x, v.y, v.z, v.w); }

// a chunk's two pieces into the hi plane (p) and the lo plane (p + plane_bytes)
__device__ __forceinline__ void store_planes2(unsigned char* p, int plane_bytes, const f32x4 v, float s) {
  const uint4 q = f2g_f16_split4(f4(v), s);
  *reinterpret_cast<u32x2*>(p) = u32x2{q.x, q.y};
  *reinterpret_cast<u32x2*>(p + plane_bytes) = u32x2{q.z, q.w};
}

// tap a of wave w's four (the fourth exists for waves 0..2 only)
__device__ __forceinline__ int wgrad3h_tap(int wave, int a) { return a < 3 ? wave + 8 * a : 24 + (wave < 3 ? wave : 0); }

// flush: every tap is owned by one wave over all pixels, so its tile goes straight out as atomics, folded and
// unscaled on the way (the reciprocals one after the other: their product may leave the float range)
__device__ __forceinline__ void c32_wgrad_flush_h3(float* gw, const f32x16 (&acc)[4], const f32x16 (&acx)[4], int wave,
                                                   int li, int hh, float rsx, float rsg) {
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    if (a == 3 && wave >= 3) break;
    const int t = wgrad3h_tap(wave, a);
#pragma unroll
    for (int e = 0; e < 16; ++e)
      atomicAdd(gw + (acc_row(e) + 4 * hh) * (NTAP * C) + t * C + li, h3_value(acc[a][e], acx[a][e], rsx, rsg));
  }
}

template <int TH, int TW>
__global__ __launch_bounds__(512, 1) void conv32_s2_wgrad3h_kernel(const f2g_conv32_desc d, float* gw, int tiles_h,
                                                                   int tiles_w, int tiles_per_block) {
  // tiles of 8 x 16 or 16 x 8 output pixels; a k step = 16 pixels = one tile row or two
  constexpr int IH = TH + KH - 1, IW = TW + (KW - 1) / 2, XW = 2 * IW - 1;
  constexpr int XPAR = IH * IW * 64 + 64;  // bytes of one column parity of a plane (+64: conv32_s2_wgrad6_kernel)
  constexpr int XPL = 2 * XPAR;            // bytes of one plane of the input patch
  constexpr int XCH = (IH * XW * (C / 4) + 511) / 512;   // patch chunks per thread: 7
  constexpr int KR = 16 / TW;              // tile rows per k step
  constexpr int NK = TH / KR;              // k steps per tile: 8
  constexpr int BUFB = wgrad3h_buf<TH, TW>();
  static_assert(TH * TW == 128 && NK == 8 && XCH <= NK - 1 && GCH == 2, "tile shapes");
  static_assert(BUFB == 2 * XPL + 2 * GPL, "a staged tile");
  extern __shared__ __attribute__((aligned(16))) unsigned char smb[];
  // buffer b at smb + b * BUFB: [2 pieces][2 parities][IH][IW] pixels x 32 halves, then [2 pieces][128 px] x 32 halves
  unsigned* smx = reinterpret_cast<unsigned*>(smb + 2 * BUFB);   // [x, g][8 waves] maxima of the next tile
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, hh = lane >> 5;
  const int ntiles = d.S * tiles_h * tiles_w;
  f32x16 acc[4], acx[4];
  h3_zero<4>(acc, acx);
  // transposed-read lane roles: 16-lane group g4 = (channel half, k half); lane i = (pixel i>>2, quad i&3)
  const int g4 = lane >> 4, i16 = lane & 15;
  // pixel of the first read inside a k step: lane halves take pixels 0-7 / 8-15 of it (the next tile row when
  // rows are 8 pixels wide); kpix = offset in the dense gradient tile, kpat = in the staged patch
  const int kpix = (g4 >> 1) * 8 + (i16 >> 2);
  const int kpat = TW == 16 ? kpix : (g4 >> 1) * IW + (i16 >> 2);
  const int chb = (g4 & 1) * 32 + (i16 & 3) * 8;           // byte offset of this lane's 4 channels
  int xo[4];                                               // patch offsets of this wave's taps
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int t = wgrad3h_tap(wave, a);
    const int dh = t / KW, j = t - dh * KW;
    xo[a] = (j & 1) * XPAR + (dh * IW + (j >> 1) + kpat) * 64 + chb;
  }
  const int go = kpix * 64 + chb;
  // chunk q of this thread = 4 channels of patch pixel px0 + 64 q = (row r, column xr); plane offset and source
  // offset are recomputed per tile
  const int c4 = tid & 7, px0 = tid >> 3;
  // (the empty asm keeps the chunk arithmetic inside the tile loop instead of in registers across it:
  // conv32_s2_fwd3h_kernel)
  auto xoff = [&](int q) {                 // byte offset inside a plane, or -1
    int pxb = px0;
    asm volatile("" : "+v"(pxb));
    const int px = pxb + 64 * q;
    const int r = div_small<XW>(px), xr = px - r * XW;
    return px < IH * XW ? (xr & 1) * XPAR + (r * IW + (xr >> 1)) * 64 + c4 * 8 : -1;
  };
  auto tile_pos = [&](int ti, int& s, int& h0, int& w0) {
    s = ti / (tiles_h * tiles_w);
    const int rem = ti - s * (tiles_h * tiles_w);
    const int th = rem / tiles_w;
    h0 = th * TH;
    w0 = (rem - th * tiles_w) * TW;
  };
  auto load_tile = [&](int ti, f32x4 (&px_)[XCH], f32x4 (&pg_)[GCH]) {
    int s, h0, w0;
    tile_pos(ti, s, h0, w0);
    const int x0 = 2 * w0 - (KW - 1) / 2;
    const float* org = d.x + (long long)s * d.x_seq + (long long)(h0 - 1) * d.x_line + (long long)x0 * C + c4 * 4;
    int pxb = px0;
    asm volatile("" : "+v"(pxb));
#pragma unroll
    for (int q = 0; q < XCH; ++q) {
      const int px = pxb + 64 * q;
      const int r = div_small<XW>(px), xr = px - r * XW;
      const int h = h0 - 1 + r, x = x0 + xr;
      const bool ok = px < IH * XW && h >= 0 && h < d.H && x >= 0 && x < d.Win;
      px_[q] = *reinterpret_cast<const f32x4*>(ok ? org + (long long)r * d.x_line + xr * C : c32_zero);
    }
    const float* gs = d.y + (long long)s * d.y_seq;
#pragma unroll
    for (int q = 0; q < GCH; ++q) {
      const int px = (tid >> 3) + 64 * q;
      const int h = h0 + px / TW, w = w0 + px % TW;
      const bool ok = h < d.H && w < d.Wout;
      pg_[q] = *reinterpret_cast<const f32x4*>(ok ? gs + (long long)h * d.y_line + (long long)w * C + c4 * 4 : c32_zero);
    }
  };
  // the maxima of the tile in the registers, per wave, into smx (read behind the next barrier)
  auto post_amax = [&](const f32x4 (&px_)[XCH], const f32x4 (&pg_)[GCH]) {
    unsigned mx = 0, mg = 0;
#pragma unroll
    for (int q = 0; q < XCH; ++q) mx = f2g_f16_amax4(f4(px_[q]), mx);
#pragma unroll
    for (int q = 0; q < GCH; ++q) mg = f2g_f16_amax4(f4(pg_[q]), mg);
    mx = f2g_wave_max(mx);
    mg = f2g_wave_max(mg);
    if (lane == 0) smx[wave] = mx, smx[8 + wave] = mg;
  };
  // the running scale of one operand moves on to the tile whose maxima are in smx; f = s_new / s_old
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
  auto put_x = [&](unsigned char* X, int q, const f32x4 v, float s) {
    const int off = xoff(q);
    if (off >= 0) store_planes2(X + off, XPL, v, s);
  };
  auto put_g = [&](unsigned char* G, int q, const f32x4 v, float s) {
    store_planes2(G + ((tid >> 3) + 64 * q) * 64 + c4 * 8, GPL, v, s);
  };
  // k step `row` of the staged tile: this wave's three or four taps, three MFMAs each (hi lo' first so that the
  // two MFMAs into acx are not back to back, as conv32h3.hip's unit3)
  auto k_step = [&](const unsigned char* X, const unsigned char* G, int row) {
    f16x8 a[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) a[q] = tr_frag_f16<64>(G + q * GPL + go + row * 16 * 64);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t == 3 && wave >= 3) break;
      f16x8 b[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) b[q] = tr_frag_f16<64>(X + q * XPL + xo[t] + row * KR * IW * 64);
      h3_term(1, acc[t], acx[t], a[0], a[1], b[0], b[1]);
      h3_term(0, acc[t], acx[t], a[0], a[1], b[0], b[1]);
      h3_term(2, acc[t], acx[t], a[0], a[1], b[0], b[1]);
    }
  };
  const int t0 = blockIdx.x * tiles_per_block;
  int tend = t0 + tiles_per_block;
  if (tend > ntiles) tend = ntiles;
  if (t0 >= tend) return;
  if (tid < IH * 8) {   // the odd parity has one column less: keep its last column defined (never rewritten)
    const int r = tid >> 3;
    const int off = XPAR + (r * IW + IW - 1) * 64 + c4 * 8;
#pragma unroll
    for (int q = 0; q < 4; ++q)   // both buffers, both planes
      *reinterpret_cast<u32x2*>(smb + (q >> 1) * BUFB + (q & 1) * XPL + off) = u32x2{0u, 0u};
  }
  unsigned mrx = 0u, mrg = 0u;             // the running maxima; 0 = scale 1
  float sx = 1.f, rsx = 1.f, sg = 1.f, rsg = 1.f;
  {
    f32x4 px_[XCH], pg_[GCH];
    load_tile(t0, px_, pg_);
    post_amax(px_, pg_);
    __syncthreads();
    float f;
    next_scale(smx, mrx, sx, rsx, f);      // (the accumulators are zero: no rescale)
    next_scale(smx + 8, mrg, sg, rsg, f);
#pragma unroll
    for (int q = 0; q < XCH; ++q) put_x(smb, q, px_[q], sx);
#pragma unroll
    for (int q = 0; q < GCH; ++q) put_g(smb + 2 * XPL, q, pg_[q], sg);
  }
  __syncthreads();
  int cur = 0;
  for (int ti = t0; ti < tend; ++ti, cur ^= 1) {
    const bool more = ti + 1 < tend;       // (block-uniform: the barriers below are met by all or by none)
    const unsigned char* Xc = smb + cur * BUFB;
    const unsigned char* Gc = Xc + 2 * XPL;
    unsigned char* Xn = smb + (cur ^ 1) * BUFB;
    unsigned char* Gn = Xn + 2 * XPL;
    f32x4 px_[XCH], pg_[GCH];
    if (more) load_tile(ti + 1, px_, pg_);
#pragma unroll
    for (int row = 0; row < NK / 2; ++row) k_step(Xc, Gc, row);
    float fx = 1.f, fg = 1.f;
    if (more) {
      post_amax(px_, pg_);                 // the next tile's loads have landed under the first half's MFMAs
      __syncthreads();
      next_scale(smx, mrx, sx, rsx, fx);
      next_scale(smx + 8, mrg, sg, rsg, fg);
    }
    // the second half; the next tile is split at its scales into the other buffer, two chunks per k step
#pragma unroll
    for (int row = NK / 2; row < NK; ++row) {
      k_step(Xc, Gc, row);
      if (more) {
        const int j = row - NK / 2;
        if (2 * j < XCH) put_x(Xn, 2 * j < XCH ? 2 * j : 0, px_[2 * j < XCH ? 2 * j : 0], sx);
        if (2 * j + 1 < XCH) put_x(Xn, 2 * j + 1 < XCH ? 2 * j + 1 : 0, px_[2 * j + 1 < XCH ? 2 * j + 1 : 0], sx);
        if (row == NK - 1) {
          put_g(Gn, 0, pg_[0], sg);
          put_g(Gn, 1, pg_[1], sg);
        }
      }
    }
    if (more) {
      if (fx != 1.f || fg != 1.f) {        // a scale moved: the stored sums go over to the new one
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            acc[t][e] = acc[t][e] * fx * fg;
            acx[t][e] = acx[t][e] * fx * fg;
          }
      }
      __syncthreads();                     // the next tile is staged; every wave is done with this one's planes
    }
  }
  c32_wgrad_flush_h3(gw, acc, acx, wave, li, hh, rsx, rsg);
}

}  // namespace

// gw (32, 27 * 32) += the fp16x3 weight gradient of the (3, 9) band layer (include/flow2gan_hip.h)
extern "C" int f2g_conv32_s2_wgrad_h3(const f2g_conv32_desc* d, float* gw, f2g_stream_t stream) {
  if (!d || !d->x || !d->y || !gw) return F2G_EINVAL;
  if (d->precision != 4) return F2G_EINVAL;
  if (d->S <= 0 || d->H <= 0 || d->Wout <= 0) return F2G_OK;
  if (d->Wout != (d->Win + 8 - 9) / 2 + 1) return F2G_EINVAL;
  auto al = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
  if (!al(d->x) || !al(d->y) || (d->x_line & 3) || (d->x_seq & 3) || (d->y_line & 3) || (d->y_seq & 3))
    return F2G_EINVAL;
  const c32_tiling t = c32_pick_tiles(d->H, d->Wout);
  const long long nt = (long long)d->S * t.tiles_h * t.tiles_w;
  if (nt >= (1ll << 30) || d->x_line >= (1ll << 24)) return F2G_EINVAL;
  int per = (int)((nt + 255) / 256);        // <= 256 blocks (one per CU): bounds the atomics
  if (per < 1) per = 1;
  const unsigned grid = (unsigned)((nt + per - 1) / per);
  return c32_launch_shape<conv32_s2_wgrad3h_kernel<8, 16>, conv32_s2_wgrad3h_kernel<16, 8>>(
      t.tall, wgrad3h_smem<8, 16>(), wgrad3h_smem<16, 8>(), dim3(grid), dim3(512), (hipStream_t)stream, *d, gw,
      t.tiles_h, t.tiles_w, per);
}
