// fp32-CLASS instances of the direct MRD band convolutions (conv32.hip; reference
// discriminators.py:171-181: Conv2d(32, 32, (3, 9), stride (1, 2), padding (1, 4))) on the bf16 matrix
// pipe: f2g_conv32_desc.precision = 3.  Every fp32 value is three bf16 pieces x = p0 + p1 + p2 and a
// product the six v_mfma_f32_32x32x16_bf16 with i + j <= 2, fp32 accumulation, smallest terms first
// (error <= ~2^-23 per product: the class of fp32 rounding -- gemm_x6.hip, gemm_x6_kernel).  The matrix
// pipe is 2.7x less busy per product than with v_mfma_f32_32x32x2_f32 (12 MFMAs of 32 cycles per tap and
// wave instead of 16 of 64).
//
// The patch of a tile is split ONCE while it is staged (each element then feeds 27 taps x 32 outputs):
// a staged pixel is [32 p0 | 32 p1 | 32 p2 | pad] bf16 = 208 bytes (52 dwords: conflict-free
// ds_read_b128); the weights arrive as the f2g_split_bf16x3 image of the packed matrix (192 contiguous
// bytes per output channel and tap).  208-byte pixels need 83 KB for the forward patch, so ONE block of
// 8 waves per CU: the blocks are persistent (a block walks tiles b, b + G, ...) and request the next
// tile's patch into registers before they compute the current one.  Forward and data gradient split a
// tile's reduction over the waves, which hold the weight fragments of their k steps in registers for the
// block's life (no weight ever passes through LDS); the (3, 3) layer keeps its nine weight tiles in LDS.
#include <stdlib.h>

#include "conv32_common.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int NTAP = KH * KW;
constexpr int PB = 208;            // bytes of a staged pixel / weight row

// three bf16 pieces of four floats (common.h: f2g_split3_pair, round to nearest even at every step)
__device__ __forceinline__ void split3(const f32x4 v, u32x2& p0, u32x2& p1, u32x2& p2) {
  unsigned a0, a1, a2, b0, b1, b2;
  f2g_split3_pair(v.x, v.y, a0, a1, a2);
  f2g_split3_pair(v.z, v.w, b0, b1, b2);
  p0 = u32x2{a0, b0};
  p1 = u32x2{a1, b1};
  p2 = u32x2{a2, b2};
}

__device__ __forceinline__ void store_px3(unsigned char* p, const f32x4 v) {   // p = piece 0 of the chunk
  u32x2 p0, p1, p2;
  split3(v, p0, p1, p2);
  *reinterpret_cast<u32x2*>(p) = p0;
  *reinterpret_cast<u32x2*>(p + 64) = p1;
  *reinterpret_cast<u32x2*>(p + 128) = p2;
}

// one tap: A = this lane's staged pixel, B = this lane's weight row (both: piece q at + 64 q bytes, the
// lane half hh takes channels [16 ks + 8 hh, + 8) of k step ks).  Twelve MFMAs, smallest terms first.
// (Measured and dropped: the fragments of a tap requested one tap AHEAD of its MFMAs through a second
// register stage -- 96 fragment registers beside accumulators, patch and weight staging spill, 6.6 -> 7.5 ms
// over the 45 forward launches of a pass; weights two groups ahead and the patch split interleaved with the
// tap groups: no change.  Lab builds, profiles/r04_conv32x6.txt: no weight loads -12 %, no patch -11 %, no
// barriers -4 %, no MFMAs -8 %; none of them alone is the bound.)
struct frag6 {
  bf16x8 v[2][3];
};
__device__ __forceinline__ void ld6(frag6& f, const unsigned char* p) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int q = 0; q < 3; ++q) f.v[ks][q] = *reinterpret_cast<const bf16x8*>(p + q * 64 + ks * 32);
}
__device__ __forceinline__ void mm6(const frag6& a, const frag6& b, f32x16& acc0, f32x16& acc1) {
#define F2G_X6_PAIR(I, J)                                                               \
  acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v[0][I], b.v[0][J], acc0, 0, 0, 0);   \
  acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v[1][I], b.v[1][J], acc1, 0, 0, 0);
  F2G_X6_PAIR(2, 0) F2G_X6_PAIR(1, 1) F2G_X6_PAIR(0, 2) F2G_X6_PAIR(1, 0) F2G_X6_PAIR(0, 1) F2G_X6_PAIR(0, 0)
#undef F2G_X6_PAIR
}
__device__ __forceinline__ void tap6(const unsigned char* Ab, const unsigned char* Bb, f32x16& acc0, f32x16& acc1) {
  frag6 a, b;
  ld6(a, Ab);
  ld6(b, Bb);
  mm6(a, b, acc0, acc1);
}

// one product in the fp32 class: the six MFMAs with i + j <= 2 of the pieces a[i], b[j], smallest terms first
__device__ __forceinline__ void mfma6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16& c) {
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], c, 0, 0, 0);
}

// ---- forward ----------------------------------------------------------------------------------------
// The reduction of a tile is 54 k steps of 16 (27 taps x the two halves of the input channels), split over
// the block's 8 waves: waves 0..5 take seven consecutive k steps, waves 6 and 7 six.  A wave loads the B
// fragments of ITS k steps once, straight from the f2g_split_bf16x3 image (lane li = output channel, 16 bytes
// at q * 64 + ks * 32 + hh * 16 of the (co, tap) row), and keeps them in 84 registers until it exits: no
// weight passes through LDS, and a tile costs no weight traffic at all.  Per tile a wave computes all four
// 32-pixel groups over its own k steps -- three ds_read_b128 of the staged pixel's pieces per six MFMAs --
// and the eight partial 128 x 32 tiles meet through 64 KB of LDS in two phases of two pixel groups: every
// wave writes its partials [wave][group][pixel][channel], and wave w then owns 8 pixels of each group pair,
// which it sums over the waves in the fixed order 0..7 (no atomics: the result is bit-reproducible) and
// stores as 16-byte [pixel][channel] row segments after bias and leaky ReLU.  Four barriers per tile.
template <int TH_, int TW_>
__global__ __launch_bounds__(512, 1) void conv32_s2_fwd6_kernel(const f2g_conv32_desc d, int tiles_w,
                                                               int tiles_h, int ntiles) {
  constexpr int IHv = TH_ + KH - 1, IWv = TW_ + (KW - 1) / 2, XW = 2 * IWv - 1;
  constexpr int SUBB = IHv * IWv * PB + 64;             // bytes of one column parity of the patch
  constexpr int NCHK = (IHv * XW * (C / 4) + 511) / 512;
  constexpr int PGB = (TW_ == 16 ? 2 : 4) * IWv * PB;    // bytes from a pixel group's staged pixels to the next's
  constexpr int NKS = 2 * NTAP, KPW = 7;                // k steps of a tile / of a wave (waves 6, 7: one less)
  static_assert(TH_ * TW_ == 128, "a block owns 128 output pixels");
  static_assert(6 * KPW + 2 * (KPW - 1) == NKS, "the k split covers the reduction exactly");
  extern __shared__ __attribute__((aligned(16))) unsigned char smb[];
  unsigned char* At = smb;                               // [2 parities][IHv][IWv] pixels
  float* red = reinterpret_cast<float*>(smb + 2 * SUBB); // [8 waves][2 pixel groups][32 pixels][32 channels]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, hh = lane >> 5;
  const int c4 = tid & 7;
  const int px0 = tid >> 3;
  auto tile_pos = [&](int tile, int& sq, int& h0, int& w0) {
    const int tw = tile % tiles_w, rest = tile / tiles_w;
    const int th = rest % tiles_h;
    sq = rest / tiles_h;
    h0 = th * TH_;
    w0 = tw * TW_;
  };
  // chunk q of this thread = 4 channels of patch pixel px0 + 64 q = (row r, column xr); recomputed per
  // tile (a multiplication) instead of kept in 21 registers beside the weights: the empty asm makes px0 opaque,
  // or the compiler hoists every chunk's offsets out of the tile loop and spills them
  auto load_patch = [&](int tile, f32x4 (&pf)[NCHK]) {
    int sq, h0, w0;
    tile_pos(tile, sq, h0, w0);
    const int x0 = 2 * w0 - (KW - 1) / 2;
    const float* org = d.x + (long long)sq * d.x_seq + (long long)(h0 - 1) * d.x_line + (long long)x0 * C + c4 * 4;
    const int xl = (int)d.x_line;                // (< 2^24, checked by the launcher: row offsets fit 32 bits)
    int pxb = px0;
    asm volatile("" : "+v"(pxb));                // (keeps the chunk arithmetic inside the tile loop, see above)
#pragma unroll
    for (int q = 0; q < NCHK; ++q) {
      const int px = pxb + 64 * q;
      const int r = div_small<XW>(px), xr = px - r * XW;
      const int h = h0 - 1 + r, x = x0 + xr;
      const bool ok = px < IHv * XW && h >= 0 && h < d.H && x >= 0 && x < d.Win;
      pf[q] = *reinterpret_cast<const f32x4*>(ok ? org + (r * xl + xr * C) : c32_zero);
    }
  };
  auto store_patch = [&](const f32x4 (&pf)[NCHK]) {
    int pxb = px0;
    asm volatile("" : "+v"(pxb));
#pragma unroll
    for (int q = 0; q < NCHK; ++q) {
      const int px = pxb + 64 * q;
      const int r = div_small<XW>(px), xr = px - r * XW;
      if (px < IHv * XW) store_px3(At + (xr & 1) * SUBB + (r * IWv + (xr >> 1)) * PB + c4 * 8, pf[q]);
    }
  };
  int tile = blockIdx.x;
  if (tile >= ntiles) return;
  f32x4 pf[NCHK];
  load_patch(tile, pf);
  // this wave's k steps k0 .. k0 + nk - 1 (k = 2 tap + channel half): weight fragments for the block's life
  // and the wave-uniform patch offsets (the image is [co][27 taps][3 pieces][32] bf16 = 192 bytes per (co, tap))
  const int k0 = wave * KPW - (wave == 7 ? 1 : 0);
  const bool seven = wave < 6;
  bf16x8 wf[KPW][3];
  int koff[KPW];
  {
    const unsigned char* wrow = reinterpret_cast<const unsigned char*>(d.w) + li * (NTAP * 192) + hh * 16;
#pragma unroll
    for (int j = 0; j < KPW; ++j) {
      int k = k0 + j;
      k = k < NKS ? k : NKS - 1;                      // (the unused seventh step of waves 6, 7: any valid one)
      const int t = k >> 1, ks = k & 1;
      const int dh = t / KW, jw = t - dh * KW;
      koff[j] = (jw & 1) * SUBB + (dh * IWv + (jw >> 1)) * PB + ks * 32;
#pragma unroll
      for (int q = 0; q < 3; ++q) wf[j][q] = *reinterpret_cast<const bf16x8*>(wrow + t * 192 + q * 64 + ks * 32);
    }
  }
  int ph, pw;                                   // this lane's output pixel inside pixel group 0
  px_of_row<TW_>(0, li, ph, pw);
  const unsigned char* Ap = At + (ph * IWv + pw) * PB + hh * 16;
  // owner role: pixel (wave & 3) * 8 + (lane >> 3) of pixel group 2 * phase + (wave >> 2), channels 4 (lane & 7) ..
  const int orow = (wave & 3) * 8 + (lane >> 3), och = 4 * (lane & 7);
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (d.bias) bias4 = f32x4{d.bias[och], d.bias[och + 1], d.bias[och + 2], d.bias[och + 3]};
  store_patch(pf);
  __syncthreads();
  for (; tile < ntiles; tile += gridDim.x) {
    const int nxt = tile + gridDim.x;
    const bool more = nxt < ntiles;
    load_patch(more ? nxt : tile, pf);          // (the last tile re-requests its own: never stored)
    f32x16 acc[4];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[g4][e] = 0.f;
    // unit u = (k step u >> 2, pixel group u & 3): the three fragments of unit u + 1 are requested in front of
    // unit u's six MFMAs (i + j <= 2, smallest terms first), and the scheduler may not move anything across a
    // unit's end -- left alone it sinks the reads to their first use and waits lgkmcnt(0) in front of most MFMAs
    bf16x8 a[2][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) a[0][q] = *reinterpret_cast<const bf16x8*>(Ap + koff[0] + q * 64);
#pragma unroll
    for (int u = 0; u < 4 * KPW; ++u) {
      const int j = u >> 2, g4 = u & 3;
      if (u + 1 < 4 * KPW) {                       // (waves 6, 7 read their clamped seventh step and drop it)
        const unsigned char* an = Ap + koff[(u + 1) >> 2] + ((u + 1) & 3) * PGB;
#pragma unroll
        for (int q = 0; q < 3; ++q) a[(u + 1) & 1][q] = *reinterpret_cast<const bf16x8*>(an + q * 64);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (j < KPW - 1 || seven) {
        mfma6(a[u & 1], wf[j], acc[g4]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    int sq, h0, w0;
    tile_pos(tile, sq, h0, w0);
    float* ys = d.y + (long long)sq * d.y_seq;
    __syncthreads();                              // the owners of the previous tile are done with `red`
#pragma unroll
    for (int p2 = 0; p2 < 2; ++p2) {
      if (p2) __syncthreads();                    // the owners have read phase 0
#pragma unroll
      for (int g2 = 0; g2 < 2; ++g2)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          red[((wave * 2 + g2) * 32 + acc_row(e) + 4 * hh) * 32 + li] = acc[2 * p2 + g2][e];
      __syncthreads();                            // (phase 0: every wave is also done with this tile's patch)
      f32x4 s = *reinterpret_cast<const f32x4*>(red + (((wave >> 2)) * 32 + orow) * 32 + och);
#pragma unroll
      for (int w8 = 1; w8 < 8; ++w8) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(red + ((w8 * 2 + (wave >> 2)) * 32 + orow) * 32 + och);
        s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
      }
      s.x += bias4.x, s.y += bias4.y, s.z += bias4.z, s.w += bias4.w;
      if (d.lrelu_slope != 0.f) {
        s.x = s.x > 0.f ? s.x : d.lrelu_slope * s.x;
        s.y = s.y > 0.f ? s.y : d.lrelu_slope * s.y;
        s.z = s.z > 0.f ? s.z : d.lrelu_slope * s.z;
        s.w = s.w > 0.f ? s.w : d.lrelu_slope * s.w;
      }
      int qh, qw;
      px_of_row<TW_>(2 * p2 + (wave >> 2), orow, qh, qw);
      const int oh = h0 + qh, ow = w0 + qw;
      if (oh < d.H && ow < d.Wout)
        *reinterpret_cast<f32x4*>(ys + (long long)oh * d.y_line + (long long)ow * C + och) = s;
      if (p2 == 0 && more) store_patch(pf);       // the next tile's patch, behind the first phase's sums
    }
  }
}

// ---- data gradient -----------------------------------------------------------------------------------
// gx[h, x, ci] = sum_{dh, j, co} g[h + 1 - dh, (x + 4 - j) / 2, co] * w[co, ci, dh, j] over the taps with
// x + 4 - j even (conv32.hip): input columns of parity E = x & 1 use the taps j = E + 2u (5 / 4 of them per
// row) and read CONSECUTIVE gradient columns m + 2 - u (x = 2 m + E) -- both parities read the SAME
// gradient patch.  Here a tile is 128 positions m x BOTH parities: waves 0..3 compute the even input columns
// (15 taps = 30 k steps of 16 output channels, split 8 / 8 / 7 / 7), waves 4..7 the odd ones (12 taps = 24 k
// steps, 6 each), from one staged patch.  As in the forward kernel a wave holds the B fragments of its k steps
// in registers for the block's life (<= 96), computes all four position groups of its parity over them, and the
// four partial tiles of a parity meet through LDS in two phases of two position groups, summed in the fixed
// order of the waves; wave wq of a parity then owns 16 positions of each phase as four 16-byte
// [position][channel] items per tile, which is also the epilogue's store form.
// d.x = g (S, H, Wout, 32), d.y = gx (S, H, Win, 32),
// d.w = the f2g_split_bf16x3 image of wT [27 taps][ci][co] as an (864, 32) matrix: 192 bytes per (tap, ci).
template <int TH_, int TW_>
__global__ __launch_bounds__(512, 1) void conv32_s2_dgrad6_kernel(const f2g_conv32_desc d, int tiles_w,
                                                                 int tiles_h, int ntiles) {
  constexpr int IHv = TH_ + KH - 1, GWv = TW_ + 4;
  constexpr int NCHK = (IHv * GWv * (C / 4) + 511) / 512;
  constexpr int PGB = (TW_ == 16 ? 2 : 4) * GWv * PB;    // bytes from a position group's staged pixels to the next's
  constexpr int KPW = 8;                                 // k steps of a wave at most
  static_assert(TH_ * TW_ == 128, "a block owns 128 positions of each column parity");
  extern __shared__ __attribute__((aligned(16))) unsigned char smb[];
  unsigned char* At = smb;                               // [IHv][GWv] pixels
  float* red = reinterpret_cast<float*>(smb + IHv * GWv * PB);   // [8 waves][2 groups][32 positions][32 channels]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, hh = lane >> 5;
  const int wq = wave & 3, E = wave >> 2;                // E = column parity of this wave half
  const int c4 = tid & 7;
  const int NU = E ? 4 : 5;
  const int Wp = (d.Win + 1 - E) / 2;                    // input columns of this parity
  const int px0 = tid >> 3;
  auto tile_pos = [&](int tile, int& sq, int& h0, int& m0) {
    const int tw = tile % tiles_w, rest = tile / tiles_w;
    const int th = rest % tiles_h;
    sq = rest / tiles_h;
    h0 = th * TH_;
    m0 = tw * TW_;
  };
  // (the empty asm keeps the chunk arithmetic inside the tile loop: see the forward kernel)
  auto load_patch = [&](int tile, f32x4 (&pf)[NCHK]) {
    int sq, h0, m0;
    tile_pos(tile, sq, h0, m0);
    const float* org = d.x + (long long)sq * d.x_seq + (long long)(h0 - 1) * d.x_line + (long long)(m0 - 2) * C + c4 * 4;
    const int xl = (int)d.x_line;
    int pxb = px0;
    asm volatile("" : "+v"(pxb));
#pragma unroll
    for (int q = 0; q < NCHK; ++q) {
      const int px = pxb + 64 * q;
      const int r = div_small<GWv>(px), xc = px - r * GWv;
      const int h = h0 - 1 + r, c = m0 - 2 + xc;
      const bool ok = px < IHv * GWv && h >= 0 && h < d.H && c >= 0 && c < d.Wout;
      pf[q] = *reinterpret_cast<const f32x4*>(ok ? org + (r * xl + xc * C) : c32_zero);
    }
  };
  auto store_patch = [&](const f32x4 (&pf)[NCHK]) {
#pragma unroll
    for (int q = 0; q < NCHK; ++q) {
      const int px = px0 + 64 * q;
      if (px < IHv * GWv) store_px3(At + px * PB + c4 * 8, pf[q]);
    }
  };
  int tile = blockIdx.x;
  if (tile >= ntiles) return;
  f32x4 pf[NCHK];
  load_patch(tile, pf);
  // this wave's k steps k0 .. k0 + nk - 1 of its parity (k = 2 ti + half of the output channels; tap index ti of
  // parity E -> weight tile (ti / NU) * 9 + E + 2 * (ti % NU), gradient pixel (ti / NU) rows up and ti % NU
  // columns left of the position's): fragments for the block's life, wave-uniform patch offsets
  const int nk = E ? 6 : (wq < 2 ? 8 : 7);
  const int k0 = E ? 6 * wq : (wq < 2 ? 8 * wq : 16 + 7 * (wq - 2));
  bf16x8 wf[KPW][3];
  int koff[KPW];
  {
    const unsigned char* wrow = reinterpret_cast<const unsigned char*>(d.w) + li * 192 + hh * 16;
    const int nks = 2 * KH * NU;
#pragma unroll
    for (int j = 0; j < KPW; ++j) {
      int k = k0 + j;
      k = k < nks ? k : nks - 1;                      // (steps past nk: any valid one, never multiplied)
      const int ti = k >> 1, ks = k & 1;
      const int dh = E ? ti >> 2 : (ti * 13) >> 6;    // ti / NU for ti < 15 without a division
      const int u = ti - dh * NU;
      koff[j] = ks * 32 - (dh * GWv + u) * PB;
      const int tile_w = dh * KW + E + 2 * u;
#pragma unroll
      for (int q = 0; q < 3; ++q)
        wf[j][q] = *reinterpret_cast<const bf16x8*>(wrow + tile_w * (C * 192) + q * 64 + ks * 32);
    }
  }
  int ph, pw;
  px_of_row<TW_>(0, li, ph, pw);
  const unsigned char* Ap = At + ((ph + 2) * GWv + pw + 4) * PB + hh * 16;
  // owner role: item jj = position (wq & 1) * 16 + (lane >> 3) + 8 (jj & 1) of position group 2 (jj >> 1) + (wq >> 1),
  // channels 4 (lane & 7) ..
  const int och = 4 * (lane & 7);
  const bool msk = d.mask_src != nullptr, fm = d.fm_ref != nullptr;
  const float fmw = fm ? d.fm_w * (d.fm_wdev ? d.fm_wdev[0] : 1.f) : 0.f;
  float cs[4] = {0.f, 0.f, 0.f, 0.f};            // column sums of what this lane stores (channels och ..)
  store_patch(pf);
  __syncthreads();
  for (; tile < ntiles; tile += gridDim.x) {
    const int nxt = tile + gridDim.x;
    const bool more = nxt < ntiles;
    load_patch(more ? nxt : tile, pf);
    int sq, h0, m0;
    tile_pos(tile, sq, h0, m0);
    // the mask of this tile's outputs is requested HERE, one 16-byte segment per item: read in the epilogue it
    // put a memory round trip behind every tile's MFMAs with nothing else resident on the CU -- which is why the
    // fused leaky-ReLU backward used to lose against a separate pass over the map.  An item's offset is the
    // tile's (wave-uniform, 64 bits) + the lane's inside the tile (32 bits: y_line < 2^24), recomputed where it
    // is used instead of kept beside the weights; -1 = outside the map.
    const long long tbase = (long long)sq * d.y_seq + (long long)h0 * d.y_line + (long long)(2 * m0 + E) * C;
    auto item_off = [&](int jj) {
      int qh, qw, l8 = lane >> 3;
      asm volatile("" : "+v"(l8));               // (opaque: or every item's terms are hoisted and spilled)
      px_of_row<TW_>(2 * (jj >> 1) + (wq >> 1), (wq & 1) * 16 + l8 + 8 * (jj & 1), qh, qw);
      return (h0 + qh < d.H && m0 + qw < Wp) ? qh * (int)d.y_line + 2 * qw * C + och : -1;
    };
    f32x4 my[4];
    if (msk && !fm) {
      // (a clamped offset, not a pointer select against a zero block: that costs a GOT load + wait per request)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int o = item_off(jj);
        my[jj] = *reinterpret_cast<const f32x4*>(d.mask_src + (o >= 0 ? tbase + o : 0));
      }
    }
    f32x16 acc[4];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[g4][e] = 0.f;
    // units (k step, position group) with the next unit's fragments requested first: see the forward kernel
    bf16x8 a[2][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) a[0][q] = *reinterpret_cast<const bf16x8*>(Ap + koff[0] + q * 64);
#pragma unroll
    for (int u = 0; u < 4 * KPW; ++u) {
      const int j = u >> 2, g4 = u & 3;
      if (u + 1 < 4 * KPW) {
        const unsigned char* an = Ap + koff[(u + 1) >> 2] + ((u + 1) & 3) * PGB;
#pragma unroll
        for (int q = 0; q < 3; ++q) a[(u + 1) & 1][q] = *reinterpret_cast<const bf16x8*>(an + q * 64);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (j < 6 || j < nk) {
        mfma6(a[u & 1], wf[j], acc[g4]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();                              // the owners of the previous tile are done with `red`
#pragma unroll
    for (int p2 = 0; p2 < 2; ++p2) {
      if (p2) __syncthreads();                    // the owners have read phase 0
      // the mask + feature-matching instance requests this phase's two items of both maps here, in front of the
      // partial tiles' way through LDS (16 registers that the MFMA loop has no room for)
      f32x4 fv[2];
      if (msk && fm) {
#pragma unroll
        for (int i2 = 0; i2 < 2; ++i2) {
          const int o = item_off(2 * p2 + i2);
          const long long oo = o >= 0 ? tbase + o : 0;
          my[2 * p2 + i2] = *reinterpret_cast<const f32x4*>(d.mask_src + oo);
          fv[i2] = *reinterpret_cast<const f32x4*>(d.fm_ref + oo);
        }
      }
#pragma unroll
      for (int g2 = 0; g2 < 2; ++g2)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          red[((wave * 2 + g2) * 32 + acc_row(e) + 4 * hh) * 32 + li] = acc[2 * p2 + g2][e];
      __syncthreads();                            // (phase 0: every wave is also done with this tile's patch)
      // ---- epilogue: optional leaky-ReLU backward of the layer below (+ feature-matching term), column sums.
      // Three separate paths, so that the plain and the mask path carry no wait of the path with two maps.
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2) {
        const int jj = 2 * p2 + i2;
        const float* rp = red + (((E * 4) * 2 + (wq >> 1)) * 32 + (wq & 1) * 16 + (lane >> 3) + 8 * i2) * 32 + och;
        f32x4 s = *reinterpret_cast<const f32x4*>(rp);
#pragma unroll
        for (int w4 = 1; w4 < 4; ++w4) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(rp + w4 * (2 * 32 * 32));
          s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
        }
        const int o = item_off(jj);
        if (o < 0) continue;
        float v[4] = {s.x, s.y, s.z, s.w};
        if (msk && !fm) {
          const float y[4] = {my[jj].x, my[jj].y, my[jj].z, my[jj].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = c32_mask_fm(v[e], y[e], false, [] { return 0.f; }, 0.f, d.mask_slope);
        } else if (msk) {
          const float y[4] = {my[jj].x, my[jj].y, my[jj].z, my[jj].w}, f[4] = {fv[i2].x, fv[i2].y, fv[i2].z, fv[i2].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = c32_mask_fm(v[e], y[e], true, [&] { return f[e]; }, fmw, d.mask_slope);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) cs[e] += v[e];
        *reinterpret_cast<f32x4*>(d.y + tbase + o) = f32x4{v[0], v[1], v[2], v[3]};
      }
      if (p2 == 0 && more) store_patch(pf);       // the next tile's patch, behind the first phase's items
    }
  }
  // column sums: the waves' sums meet in LDS (the patch: nobody reads it after the last tile's MFMAs) and leave
  // as ONE 32-lane atomic per block.  Four 8-lane atomics per wave were 8192 atomic instructions per launch on
  // one 128-byte line: serialised in L2 they took longer than the masked launch's extra map read.
  if (d.colsum) {
    float* csl = reinterpret_cast<float*>(At);     // [8 waves][32 channels]
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = cs[e];
      v += __shfl_xor(v, 8);
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (lane < 8) csl[wave * 32 + 4 * lane + e] = v;
    }
    __syncthreads();
    if (tid < 32) {
      float v = csl[tid];
#pragma unroll
      for (int w8 = 1; w8 < 8; ++w8) v += csl[w8 * 32 + tid];
      atomicAdd(d.colsum + tid, v);
    }
  }
}

// ---- weight gradient -----------------------------------------------------------------------------------
// gw[co][tap][ci] += sum_px g[px][co] * x[px -> tap][ci]: MFMA rows = co, columns = ci, reduction = the
// pixels of an 8 x 16 output tile (conv32.hip, conv32_s2_wgrad3_kernel: a bf16 MFMA wants 8 consecutive k
// per lane and k = pixels is the slow axis of both staged operands, so the tile is staged as bf16 planes
// with 64-byte pixels and the fragments come from ds_read_b64_tr_b16).  Here THREE planes per operand
// (the pieces p0, p1, p2, split once while the tile is staged) and six MFMAs per product; wave w owns taps
// w, w + 8, w + 16 over the whole tile and tile row w of taps 24..26.  77 + 25 KB of planes = one block per
// CU, so the block requests the next tile's rows into registers before it computes the current one and
// splits them chunk by chunk under the MFMAs of the tile's rows.
constexpr int GPL = 128 * 64;            // bytes of one plane of the gradient tile
constexpr int GCH = 128 * (C / 4) / 512; // gradient chunks per thread: 2

template <int TH, int TW>
constexpr size_t wgrad6_smem() {   // three planes of the patch's two column parities and of the gradient tile
  return (size_t)3 * 2 * ((TH + KH - 1) * (TW + (KW - 1) / 2) * 64 + 64) + 3 * GPL;
}

template <int TH, int TW>
__global__ __launch_bounds__(512, 1) void conv32_s2_wgrad6_kernel(const f2g_conv32_desc d, float* gw,
                                                                  int tiles_h, int tiles_w,
                                                                  int tiles_per_block) {
  // tiles of 8 x 16 or 16 x 8 output pixels; a k step = 16 pixels = one tile row or two
  constexpr int IH = TH + KH - 1, IW = TW + (KW - 1) / 2, XW = 2 * IW - 1;
  constexpr int XPAR = IH * IW * 64 + 64;  // bytes of one column parity of a plane (+64: pixels x and x + 1 of the
                                           // 8-byte staging stores would otherwise share every bank)
  constexpr int XPL = 2 * XPAR;            // bytes of one plane of the input patch
  constexpr int XCH = (IH * XW * (C / 4) + 511) / 512;   // patch chunks per thread: 7
  constexpr int KR = 16 / TW;              // tile rows per k step
  constexpr int NK = TH / KR;              // k steps per tile: 8
  static_assert(TH * TW == 128 && NK == 8 && XCH <= NK && GCH <= NK, "tile shapes");
  extern __shared__ __attribute__((aligned(16))) unsigned char smb[];
  unsigned char* Xp = smb;                 // [3 pieces][2 parities][IH][IW] pixels x 32 bf16
  unsigned char* Gp = smb + 3 * XPL;       // [3 pieces][128 px] x 32 bf16
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, hh = lane >> 5;
  const int ntiles = d.S * tiles_h * tiles_w;
  f32x16 acc[6];
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[a][e] = 0.f;
  // transposed-read lane roles: 16-lane group g4 = (channel half, k half); lane i = (pixel i>>2, quad i&3)
  const int g4 = lane >> 4, i16 = lane & 15;
  // pixel of the first read inside a k step: lane halves take pixels 0-7 / 8-15 of it (the next tile row when
  // rows are 8 pixels wide); kpix = offset in the dense gradient tile, kpat = in the staged patch
  const int kpix = (g4 >> 1) * 8 + (i16 >> 2);
  const int kpat = TW == 16 ? kpix : (g4 >> 1) * IW + (i16 >> 2);
  const int chb = (g4 & 1) * 32 + (i16 & 3) * 8;           // byte offset of this lane's 4 channels
  int xo[3], xs[3];                                        // patch offsets of the owned / shared taps
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    int t = wave + 8 * a;
    int dh = t / KW, j = t - dh * KW;
    xo[a] = (j & 1) * XPAR + (dh * IW + (j >> 1) + kpat) * 64 + chb;
    t = 24 + a;
    dh = t / KW;
    j = t - dh * KW;
    xs[a] = (j & 1) * XPAR + (dh * IW + (j >> 1) + kpat) * 64 + chb;
  }
  const int go = kpix * 64 + chb;
  // chunk q of this thread = 4 channels of patch pixel px0 + 64 q = (row r, column xr); plane offset and
  // source offset are recomputed per tile (a multiplication) instead of kept in 21 registers
  const int c4 = tid & 7, px0 = tid >> 3;
  auto xoff = [&](int q) {                 // byte offset inside a plane, or -1
    const int px = px0 + 64 * q;
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
#pragma unroll
    for (int q = 0; q < XCH; ++q) {
      const int px = px0 + 64 * q;
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
  auto put3 = [&](unsigned char* base, int plane_bytes, int off, const u32x2 (&pk)[3]) {
#pragma unroll
    for (int q = 0; q < 3; ++q) *reinterpret_cast<u32x2*>(base + q * plane_bytes + off) = pk[q];
  };
  const int t0 = blockIdx.x * tiles_per_block;
  int tend = t0 + tiles_per_block;
  if (tend > ntiles) tend = ntiles;
  if (t0 >= tend) return;
  if (tid < IH * 8) {   // the odd parity has one column less: keep its last column defined (never rewritten)
    const int r = tid >> 3;
    const int off = XPAR + (r * IW + IW - 1) * 64 + c4 * 8;
#pragma unroll
    for (int q = 0; q < 3; ++q) *reinterpret_cast<u32x2*>(Xp + q * XPL + off) = u32x2{0u, 0u};
  }
  {
    f32x4 px_[XCH], pg_[GCH];
    load_tile(t0, px_, pg_);
#pragma unroll
    for (int q = 0; q < XCH; ++q)
      if (xoff(q) >= 0) {
        u32x2 pk[3];
        split3(px_[q], pk[0], pk[1], pk[2]);
        put3(Xp, XPL, xoff(q), pk);
      }
#pragma unroll
    for (int q = 0; q < GCH; ++q) {
      u32x2 pk[3];
      split3(pg_[q], pk[0], pk[1], pk[2]);
      put3(Gp, GPL, ((tid >> 3) + 64 * q) * 64 + c4 * 8, pk);
    }
  }
  __syncthreads();
  for (int ti = t0; ti < tend; ++ti) {
    const bool more = ti + 1 < tend;
    f32x4 px_[XCH], pg_[GCH];
    u32x2 kx[XCH][3], kg[GCH][3];
    load_tile(more ? ti + 1 : ti, px_, pg_);
    // owned taps: the 8 tile rows = 8 k steps of 16 pixels; one staged chunk of the next tile is split per row
#pragma unroll
    for (int row = 0; row < NK; ++row) {
      bf16x8 a[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) a[q] = tr_pix8(Gp + q * GPL + go + row * 16 * 64);
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        bf16x8 b[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) b[q] = tr_pix8(Xp + q * XPL + xo[t] + row * KR * IW * 64);
        mfma6(a, b, acc[t]);
      }
      if (row < XCH) split3(px_[row < XCH ? row : 0], kx[row < XCH ? row : 0][0], kx[row < XCH ? row : 0][1], kx[row < XCH ? row : 0][2]);
      if (row >= NK - GCH)
        split3(pg_[row >= NK - GCH ? row - (NK - GCH) : 0], kg[row >= NK - GCH ? row - (NK - GCH) : 0][0],
               kg[row >= NK - GCH ? row - (NK - GCH) : 0][1], kg[row >= NK - GCH ? row - (NK - GCH) : 0][2]);
    }
    // taps 24..26: this wave's k step (tile row `wave`, or rows 2 wave and 2 wave + 1)
    {
      const int row = wave;
      bf16x8 a[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) a[q] = tr_pix8(Gp + q * GPL + go + row * 16 * 64);
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        bf16x8 b[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) b[q] = tr_pix8(Xp + q * XPL + xs[t] + row * KR * IW * 64);
        mfma6(a, b, acc[3 + t]);
      }
    }
    __syncthreads();   // every wave is done with this tile's planes
    if (more) {
#pragma unroll
      for (int q = 0; q < XCH; ++q)
        if (xoff(q) >= 0) put3(Xp, XPL, xoff(q), kx[q]);
#pragma unroll
      for (int q = 0; q < GCH; ++q) put3(Gp, GPL, ((tid >> 3) + 64 * q) * 64 + c4 * 8, kg[q]);
    }
    __syncthreads();
  }
  static_assert(wgrad6_smem<TH, TW>() >= (size_t)8 * 16 * 64 * 4, "the flush reuses the planes as its reduction buffer");
  c32_wgrad_flush<NTAP, 3>(gw, reinterpret_cast<float*>(smb), acc, wave, lane, li, hh);
}

// ---- the fifth layer of a band stack: Conv2d(32, 32, (3, 3), padding (1, 1)), stride 1 (round 5) -------
// (discriminators.py:171-181, last entry of the band stack.)  As an implicit GEMM this is M = 10^5 pixels x
// N = 32 x K = 288 on the generic kernel's 128 x 32 tiles with bounds-tested windows: 51 TFLOP/s forward, 29
// in the weight gradient (profiles/r05_*).  Direct, fp32 class: the images are narrow (7 ... 33 columns after
// three stride-2 layers), so a tile is R WHOLE rows (R * W <= 256 pixels, >= 90 % of the MFMA rows used at
// every band width) staged with one zero column on either side and one row above / below -- the nine taps are
// then nine constant offsets into the staged patch, with no per-tap masks.  One persistent block of 8 waves per
// CU: all nine weight tiles (55 KB image, 208-byte rows) stay in LDS for the block's life, the next tile's
// patch is requested before the current tile's 108 MFMAs per wave and split into its three pieces behind them.
// The data gradient of a stride-1 conv is the same kernel over the gradient map with the taps flipped and the
// channel matrix transposed (the host re-lays the weights once per version).  (P33, T33 and the pick of R:
// conv32_common.h, shared with the fp16x3 instance in conv33h3.hip.)
__global__ __launch_bounds__(512, 1) void conv33_x6_kernel(const f2g_conv32_desc d, int R, int tiles_h, int ntiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smb[];
  unsigned char* At = smb;                       // [P33] staged pixels
  unsigned char* Bt = smb + P33 * PB;            // [9 taps][32 co] weight rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, hh = lane >> 5;
  const int W = d.Win, PW = W + 2, npx = (R + 2) * PW, tpx = R * W;
  const unsigned mgW = magic_of(W), mgPW = magic_of(PW);
  // weights: image [co][9 taps][192 bytes] -> LDS rows (tap, co) of 208 bytes
  {
    const unsigned char* wimg = reinterpret_cast<const unsigned char*>(d.w);
    for (int c = tid; c < T33 * C * 12; c += 512) {
      const int row = c / 12, part = c - row * 12;           // row = co * 9 + tap in the image
      const int co = row / T33, tap = row - co * T33;
      *reinterpret_cast<u32x4*>(Bt + (tap * C + co) * PB + part * 16) =
          *reinterpret_cast<const u32x4*>(wimg + row * 192 + part * 16);
    }
  }
  // this thread's chunks of a patch: chunk id = tid + 512 q -> (staged pixel, 4 channels)
  constexpr int NQ = (P33 * 8 + 511) / 512;
  int prow[NQ], poff[NQ], pdst[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int id = tid + 512 * q, px = id >> 3, c4 = id & 7;
    const int pr = fast_div(px, PW, mgPW), pc = px - pr * PW;
    const bool ok = px < npx && pc >= 1 && pc <= W;
    prow[q] = ok ? pr : -(1 << 20);                          // (columns of the zero border: never valid)
    poff[q] = (pr - 1) * (int)d.x_line + (pc - 1) * C + c4 * 4;
    pdst[q] = px < npx ? px * PB + c4 * 8 : -1;
  }
  auto load_patch = [&](int tile, f32x4 (&pf)[NQ]) {
    const int sq = tile / tiles_h, h0 = (tile - sq * tiles_h) * R;
    const float* org = d.x + (long long)sq * d.x_seq + (long long)h0 * d.x_line;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int h = h0 - 1 + prow[q];
      pf[q] = *reinterpret_cast<const f32x4*>((h >= 0 && h < d.H) ? org + poff[q] : c32_zero);
    }
  };
  auto store_patch = [&](const f32x4 (&pf)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (pdst[q] >= 0) store_px3(At + pdst[q], pf[q]);
  };
  // this lane's output pixel: tile pixel 32 wave + li -> (row, column) -> staged position
  const int mypx = wave * 32 + li;
  const int myr = fast_div(mypx, W, mgW), myc = mypx - myr * W;
  const unsigned char* Ap = At + (mypx < tpx ? ((myr + 1) * PW + myc + 1) * PB : (PW + 1) * PB) + hh * 16;
  const unsigned char* Bp = Bt + li * PB + hh * 16;
  const float bias = d.bias ? d.bias[li] : 0.f;
  float cs = 0.f;                                // column sums of what this lane stores (channel li)
  int tile = blockIdx.x;
  if (tile >= ntiles) return;
  {
    f32x4 pf[NQ];
    load_patch(tile, pf);
    store_patch(pf);
  }
  __syncthreads();
  for (; tile < ntiles; tile += gridDim.x) {
    const int nxt = tile + gridDim.x;
    const bool more = nxt < ntiles;
    f32x4 pf[NQ];
    load_patch(more ? nxt : tile, pf);            // (the last tile re-requests its own: never stored)
    const int sq = tile / tiles_h, h0 = (tile - sq * tiles_h) * R;
    const long long ybase = (long long)sq * d.y_seq + (long long)h0 * d.y_line;
    // data-gradient role: the leaky-ReLU backward mask of the layer below, requested before the MFMAs
    float my[16];
    if (d.mask_src) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int p = wave * 32 + acc_row(e) + 4 * hh;
        const int r = fast_div(p, W, mgW), c = p - r * W;
        my[e] = (p < tpx && h0 + r < d.H) ? d.mask_src[ybase + (long long)r * d.y_line + c * C + li] : 1.f;
      }
    }
    f32x16 acc0, acc1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
#pragma unroll
    for (int t = 0; t < T33; ++t)
      tap6(Ap + ((t / 3 - 1) * PW + (t % 3 - 1)) * PB, Bp + t * (C * PB), acc0, acc1);
    {
      float* ys = d.y + ybase;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int p = wave * 32 + acc_row(e) + 4 * hh;
        const int r = fast_div(p, W, mgW), c = p - r * W;
        if (p < tpx && h0 + r < d.H) {
          float v = acc0[e] + acc1[e] + bias;
          if (d.lrelu_slope != 0.f) v = v > 0.f ? v : d.lrelu_slope * v;
          if (d.mask_src) v *= my[e] > 0.f ? 1.f : d.mask_slope;
          cs += v;
          ys[(long long)r * d.y_line + c * C + li] = v;
        }
      }
    }
    __syncthreads();                               // every wave is done with this patch
    if (more) store_patch(pf);
    __syncthreads();
  }
  if (d.colsum) {
    cs += __shfl_xor(cs, 32);
    if (hh == 0) atomicAdd(d.colsum + li, cs);
  }
}


// ---- weight gradient of the (3, 3) fifth layer (round 6) -------------------------------------------------
// gw[co][tap][ci] += sum_px g[px][co] * x[px + tap][ci]   (discriminators.py:171-181 backward; as an implicit
// GEMM on the generic fp32 kernel -- 32 x 288 outputs over 10^5 pixels through bounds-tested windows -- it ran at
// 31 TFLOP/s).  Same tile as conv33_x6_kernel: R whole rows of a 7-112 column band image, staged with a zero
// column on either side and a row above / below, so that in the FLAT order of the staged patch the nine taps are
// nine constant offsets.  The gradient rows are staged in that same padded flat order (zeros in the border
// columns), which makes the reduction a plain walk over flat positions p: gw[tap] += G[p] * X[p + off(tap)], the
// border positions contributing G = 0.  k = pixels is the slow axis of both operands, so they are staged as
// three bf16 planes with 64-byte pixels (split once while staging) and the fragments come from
// ds_read_b64_tr_b16 (conv32_s2_wgrad6_kernel's scheme).  A k step = 16 consecutive flat positions; the block's
// 8 waves take the k steps round-robin and keep all nine 32 x 32 tap tiles (144 accumulator registers) over ALL
// tiles of their persistent block -- 3 gradient + 27 input fragments per 54 MFMAs -- and meet once at the end:
// tap by tap through LDS, one atomic per output and block.  (W33_GP, W33_XP: conv32_common.h.)
__global__ __launch_bounds__(512, 1) void conv33_wgrad6_kernel(const f2g_conv32_desc d, float* gw, int R,
                                                               int tiles_h, int ntiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smb[];
  unsigned char* Xp = smb;                      // [3 pieces][W33_XP] pixels x 32 bf16; position 0 = slack
  unsigned char* Gp = smb + 3 * W33_XPL;        // [3 pieces][W33_GP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, hh = lane >> 5;
  const int W = d.Win, PW = W + 2, npx = (R + 2) * PW, ngp = R * PW, nks = (ngp + 15) >> 4;
  const unsigned mgPW = magic_of(PW);
  // everything a fragment may touch and a tile does not rewrite (slack position, k-step overhang) is zero
  for (int o = tid * 16; o < 3 * (W33_XPL + W33_GPL); o += 512 * 16) *reinterpret_cast<u32x4*>(smb + o) = u32x4{0u, 0u, 0u, 0u};
  // chunk id = tid + 512 q -> (flat position, 4 channels)
  constexpr int NQ = (W33_GP * 8 + 511) / 512;          // 6: covers the patch (<= 352 positions) and the gradient rows
  const int c4 = tid & 7;
  int xrow[NQ], xoff[NQ], grow[NQ], goff[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int px = (tid + 512 * q) >> 3;
    {   // input patch position px = (pr + 1) * PW + (pc + 1)
      const int pr = fast_div(px, PW, mgPW), pc = px - pr * PW;
      const bool ok = px < npx && pc >= 1 && pc <= W;
      xrow[q] = px < npx ? (ok ? pr - 1 : -(1 << 20)) : -(1 << 21);     // (< -2^20: border = zeros; < -2^21: not staged)
      xoff[q] = (pr - 1) * (int)d.x_line + (pc - 1) * C + c4 * 4;
    }
    {   // gradient position px = r * PW + (c + 1)
      const int r = fast_div(px, PW, mgPW), pc = px - r * PW;
      const bool ok = px < ngp && pc >= 1 && pc <= W;
      grow[q] = px < ngp ? (ok ? r : -(1 << 20)) : -(1 << 21);
      goff[q] = r * (int)d.y_line + (pc - 1) * C + c4 * 4;
    }
  }
  // transposed-read lane roles (conv32_s2_wgrad6_kernel): 16-lane group g4 = (channel half, k half)
  const int g4 = lane >> 4, i16 = lane & 15;
  const int kpix = (g4 >> 1) * 8 + (i16 >> 2);
  const int chb = (g4 & 1) * 32 + (i16 & 3) * 8;
  const int go = kpix * 64 + chb;
  int xo[T33];
#pragma unroll
  for (int t = 0; t < T33; ++t) xo[t] = (1 + PW + (t / 3 - 1) * PW + (t % 3 - 1) + kpix) * 64 + chb;
  f32x16 acc[T33];
#pragma unroll
  for (int t = 0; t < T33; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
  __syncthreads();
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int sq = tile / tiles_h, h0 = (tile - sq * tiles_h) * R;
    const float* xs = d.x + (long long)sq * d.x_seq + (long long)h0 * d.x_line;
    const float* gs = d.y + (long long)sq * d.y_seq + (long long)h0 * d.y_line;
    f32x4 px_[NQ], pg_[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int hx = h0 + xrow[q], hg = h0 + grow[q];
      px_[q] = *reinterpret_cast<const f32x4*>((xrow[q] > -(1 << 20) && hx >= 0 && hx < d.H) ? xs + xoff[q] : c32_zero);
      pg_[q] = *reinterpret_cast<const f32x4*>((grow[q] > -(1 << 20) && hg < d.H) ? gs + goff[q] : c32_zero);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int px = (tid + 512 * q) >> 3;
      u32x2 pk[3];
      if (xrow[q] > -(1 << 21)) {
        split3(px_[q], pk[0], pk[1], pk[2]);
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<u32x2*>(Xp + pc * W33_XPL + (px + 1) * 64 + c4 * 8) = pk[pc];
      }
      if (grow[q] > -(1 << 21)) {
        split3(pg_[q], pk[0], pk[1], pk[2]);
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<u32x2*>(Gp + pc * W33_GPL + px * 64 + c4 * 8) = pk[pc];
      }
    }
    __syncthreads();
    for (int ks = wave; ks < nks; ks += 8) {
      bf16x8 a[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) a[q] = tr_pix8(Gp + q * W33_GPL + ks * (16 * 64) + go);
#pragma unroll
      for (int t = 0; t < T33; ++t) {
        bf16x8 b[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) b[q] = tr_pix8(Xp + q * W33_XPL + ks * (16 * 64) + xo[t]);
        mfma6(a, b, acc[t]);
      }
    }
    __syncthreads();   // every wave is done with this tile's planes
  }
  // every wave holds a partial tile of all nine taps: none is owned
  c32_wgrad_flush<T33, 0>(gw, reinterpret_cast<float*>(smb), acc, wave, lane, li, hh);
}

template <int TH_, int TW_>
constexpr size_t fwd6_smem() {
  return (size_t)2 * ((TH_ + 2) * (TW_ + 4) * PB + 64) + 8 * 2 * 32 * 32 * sizeof(float);
}
template <int TH_, int TW_>
constexpr size_t dgrad6_smem() {
  return (size_t)(TH_ + 2) * (TW_ + 4) * PB + 8 * 2 * 32 * 32 * sizeof(float);
}

}  // namespace

// precision-3 launchers, called from conv32.hip's entry points (arguments already checked there)
int f2g_conv32_fwd6_launch(const f2g_conv32_desc* d, hipStream_t st) {
  const c32_tiling t = c32_pick_tiles(d->H, d->Wout);
  const long long nt = (long long)t.tiles_h * t.tiles_w * d->S;
  if (nt >= (1ll << 30) || d->x_line >= (1ll << 24)) return F2G_EINVAL;
  const int grid = (int)(nt < 256 ? nt : 256);          // one resident block per CU
  return c32_launch_shape<conv32_s2_fwd6_kernel<8, 16>, conv32_s2_fwd6_kernel<16, 8>>(
      t.tall, fwd6_smem<8, 16>(), fwd6_smem<16, 8>(), dim3(grid), dim3(512), st, *d, t.tiles_w, t.tiles_h, (int)nt);
}

int f2g_conv32_dgrad6_launch(const f2g_conv32_desc* d, hipStream_t st) {
  const c32_tiling t = c32_pick_tiles(d->H, (d->Win + 1) / 2);   // positions m: the even parity has the most
  const long long nt = (long long)t.tiles_h * t.tiles_w * d->S;
  if (nt >= (1ll << 30) || d->x_line >= (1ll << 24) || d->y_line >= (1ll << 24)) return F2G_EINVAL;
  const int grid = (int)(nt < 256 ? nt : 256);
  return c32_launch_shape<conv32_s2_dgrad6_kernel<8, 16>, conv32_s2_dgrad6_kernel<16, 8>>(
      t.tall, dgrad6_smem<8, 16>(), dgrad6_smem<16, 8>(), dim3(grid), dim3(512), st, *d, t.tiles_w, t.tiles_h,
      (int)nt);
}

int f2g_conv32_wgrad6_launch(const f2g_conv32_desc* d, float* gw, hipStream_t st) {
  const c32_tiling t = c32_pick_tiles(d->H, d->Wout);
  const long long nt = (long long)d->S * t.tiles_h * t.tiles_w;
  if (nt >= (1ll << 30) || d->x_line >= (1ll << 24)) return F2G_EINVAL;
  int per = (int)((nt + 255) / 256);        // <= 256 blocks (one per CU): bounds the atomics
  if (per < 1) per = 1;
  const unsigned grid = (unsigned)((nt + per - 1) / per);
  return c32_launch_shape<conv32_s2_wgrad6_kernel<8, 16>, conv32_s2_wgrad6_kernel<16, 8>>(
      t.tall, wgrad6_smem<8, 16>(), wgrad6_smem<16, 8>(), dim3(grid), dim3(512), st, *d, gw, t.tiles_h, t.tiles_w,
      per);
}

// precision 4 (fp16x3 products, the patch scaled per tile inside the kernel): conv33h3.hip
int f2g_conv33_h3_launch(const f2g_conv32_desc* d, int R, int tiles_h, int ntiles, hipStream_t st);

// Conv2d(32, 32, (3, 3), padding (1, 1)) + bias + leaky ReLU, fp32 class (3) or fp16x3 (4) (include/flow2gan_hip.h)
extern "C" int f2g_conv33_fwd(const f2g_conv32_desc* d, f2g_stream_t stream) {
  if (!d || !d->x || !d->w || !d->y || (d->precision != 3 && d->precision != 4) || d->Win != d->Wout || d->fm_ref)
    return F2G_EINVAL;
  if ((((uintptr_t)d->x) & 15) || (((uintptr_t)d->w) & 15) || (d->x_line & 3) || (d->x_seq & 3)) return F2G_EINVAL;
  if (d->S <= 0 || d->H <= 0 || d->Win <= 0) return F2G_OK;
  const int W = d->Win;
  if (W > 112 || d->x_line >= (1ll << 24)) return F2G_EINVAL;     // 3 * (W + 2) staged pixels <= P33
  // geometry of the output map and of the two roles (forward: bias / slope; data gradient: mask_src + colsum,
  // whose source shares y's geometry by construction -- it is addressed with y's strides)
  if (d->y_line < (long long)W * C || (d->y != d->x && d->y_seq < (long long)d->H * d->y_line)) return F2G_EINVAL;
  if ((d->y_line & 3) || (d->y_seq & 3) || (((uintptr_t)d->y) & 15)) return F2G_EINVAL;
  if (d->mask_src && (d->lrelu_slope != 0.f || d->bias || (((uintptr_t)d->mask_src) & 15))) {
    f2g_set_error("f2g_conv33_fwd: mask_src (data-gradient role) excludes bias / lrelu_slope (forward role)");
    return F2G_EINVAL;
  }
  const int R = c33_pick_rows(d->H, W);              // whole rows per tile
  if (R < 1) return F2G_EINVAL;
  const int tiles_h = (d->H + R - 1) / R;
  const long long nt = (long long)tiles_h * d->S;
  if (nt >= (1ll << 30)) return F2G_EINVAL;
  if (d->precision == 4) return f2g_conv33_h3_launch(d, R, tiles_h, (int)nt, (hipStream_t)stream);
  constexpr size_t smem = (size_t)P33 * PB + (size_t)T33 * C * PB;
  c32_lds_once<conv33_x6_kernel>(smem);
  const int grid = (int)(nt < 256 ? nt : 256);          // one resident block per CU
  hipLaunchKernelGGL(conv33_x6_kernel, dim3(grid), dim3(512), smem, (hipStream_t)stream, *d, R, tiles_h, (int)nt);
  return f2g_check_launch();
}

// Weight gradient of that layer, fp32 class (precision 4 is refused here: the fp16x3 twin of conv33_wgrad6_kernel
// has an entry point of its own, f2g_conv33_wgrad_h3 in conv33h3w.hip): x =
// the layer's input (S, H, W, 32), y = the gradient of its pre-activation (S, H, W, 32; both optionally strided
// slices of wider maps), gw (32, 9 * 32) [co][tap][ci] +=.
extern "C" int f2g_conv33_wgrad(const f2g_conv32_desc* d, float* gw, f2g_stream_t stream) {
  if (!d || !d->x || !d->y || !gw || d->precision != 3 || d->Win != d->Wout) return F2G_EINVAL;
  if ((((uintptr_t)d->x) & 15) || (((uintptr_t)d->y) & 15) || (d->x_line & 3) || (d->x_seq & 3) || (d->y_line & 3) ||
      (d->y_seq & 3))
    return F2G_EINVAL;
  if (d->S <= 0 || d->H <= 0 || d->Win <= 0) return F2G_OK;
  const int W = d->Win;
  if (W > 112 || d->x_line >= (1ll << 24) || d->y_line >= (1ll << 24) || d->x_line < (long long)W * C ||
      d->y_line < (long long)W * C)
    return F2G_EINVAL;
  const int R = c33_pick_rows(d->H, W);              // whole rows per tile (conv33_x6_kernel's rule)
  if (R < 1) return F2G_EINVAL;
  const int tiles_h = (d->H + R - 1) / R;
  const long long nt = (long long)tiles_h * d->S;
  if (nt >= (1ll << 30)) return F2G_EINVAL;
  constexpr size_t smem = (size_t)3 * (W33_XPL + W33_GPL);
  static_assert(smem >= (size_t)8 * 16 * 64 * 4, "the flush reuses the planes as its reduction buffer");
  c32_lds_once<conv33_wgrad6_kernel>(smem);
  const int grid = (int)(nt < 256 ? nt : 256);          // one resident block per CU: 256 x 9216 atomics at most
  hipLaunchKernelGGL(conv33_wgrad6_kernel, dim3(grid), dim3(512), smem, (hipStream_t)stream, *d, gw, R, tiles_h,
                     (int)nt);
  return f2g_check_launch();
}
