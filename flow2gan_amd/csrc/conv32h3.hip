// fp16x3 instances of the direct MRD band convolutions (conv32x6.hip has the bf16x6 ones; reference
// discriminators.py:171-181: Conv2d(32, 32, (3, 9), stride (1, 2), padding (1, 4))): f2g_conv32_desc.precision = 4.
// Every fp32 value is two SCALED fp16 pieces and a product three v_mfma_f32_32x32x16_f16 into two accumulator sets
// (split_f16.h has the arithmetic, gemm_f16_common.h the MFMA side) -- half the MFMAs of the six-product kernels.
//
// ONE SCALE PER TILE, TAKEN INSIDE THE KERNEL.  The patch of a tile is split once while it is staged, as in
// conv32x6.hip, and every window of the tile lies inside that patch: one power-of-two scale over every float of
// the patch (halo pixels included; chunks outside the map read as zeros and do not count) factors out of every
// output of the tile exactly.  The next tile's patch sits in registers a tile ahead, so its largest magnitude costs
// a register pass, a wave butterfly and eight LDS words -- no image pass through HBM, no producer cooperation.  What
// the tile-wide scale costs is the floor term of the sequence-scaled images (gemm_f16p.hip) with the patch in place
// of the sequence: an element 2^-28 below its patch's largest is subnormal in hi, so per output
//   |err| <= 3 * 2^-22 sum |a||w| + 2^-28 (amax_patch sum_k |w_k| + wmax sum_k |a_k|).
// A patch that holds an inf or a NaN takes scale 1 (its non-finite values stay non-finite; large finite ones of the
// same patch may then leave fp16's range: that tile's outputs are not defined beyond "the windows that hold the NaN
// are NaN"); other tiles are untouched.
//
// A staged pixel is [32 hi | 32 lo | pad] halves = 144 bytes (36 dwords: conflict-free ds_read_b128, see px_of_row in
// conv32_common.h) instead of 208.  The weights arrive as ONE f2g_split_f16x2_seq run over the whole matrix (27648
// floats; 128 bytes per 32-float row segment: 32 hi halves, then 32 lo halves; the reciprocal scale is the float
// behind the image): one scale for the whole matrix, because the data gradient reduces over (tap, co) for an output
// column ci and no per-row scale of that layout factors out.
//
// Structure of the six-product kernels: persistent blocks of 8 waves, the next patch requested into registers a tile
// ahead, the reduction split by k step over the waves, which hold the weight fragments of their k steps in registers
// for the block's life (56 in the forward, 64 in the data gradient), partial tiles summed through LDS in the fixed
// wave order (no atomics: bit-reproducible).  Two accumulator sets for four pixel groups do not fit beside that, so a
// wave walks its k steps ONCE PER PHASE of two pixel groups (the weights stay put, the patch reads are the same) and
// folds acc0 + 2^-11 acc1 in registers before it writes its partials: the LDS reduction moves what it moves in the
// six-product kernels, and the second phase's MFMAs run under the first phase's sums.  The two reciprocal scales are
// applied to the summed tile, one after the other (powers of two: the same value as scaling every partial).
#include <stdlib.h>

#include "conv32_common.h"
#include "gemm_f16_common.h"
#include "split_f16.h"

namespace {

constexpr int NTAP = KH * KW;
constexpr int PB = 144;                    // bytes of a staged pixel
constexpr int WSEG = 128;                  // bytes of a 32-float row segment of the weight image
constexpr int WFLOATS = C * NTAP * C;      // floats of the weight matrix: the reciprocal scale lies behind them
constexpr int REDB = 8 * 2 * 32 * 32 * 4;  // bytes of the partial tiles: [8 waves][2 pixel groups][32][32] floats

__device__ __forceinline__ float4 f4(const f32x4 v) { return make_float4(v.x, v.y, v.z, v.w); }

__device__ __forceinline__ void store_px2(unsigned char* p, const f32x4 v, float s) {   // p = the chunk's hi halves
  const uint4 q = f2g_f16_split4(f4(v), s);
  *reinterpret_cast<u32x2*>(p) = u32x2{q.x, q.y};
  *reinterpret_cast<u32x2*>(p + 64) = u32x2{q.z, q.w};
}

// largest sign-less bit pattern of a thread's chunks of a patch, over its wave
template <int N>
__device__ __forceinline__ unsigned patch_amax(const f32x4 (&pf)[N]) {
  unsigned m = 0;
#pragma unroll
  for (int q = 0; q < N; ++q) m = f2g_f16_amax4(f4(pf[q]), m);
  return f2g_wave_max(m);
}

// the patch's scale and its reciprocal from the eight waves' maxima (smx: written before the last barrier)
__device__ __forceinline__ void patch_scales(const unsigned* smx, float& s, float& rs) {
  unsigned m = smx[0];
#pragma unroll
  for (int w8 = 1; w8 < 8; ++w8) m = m > smx[w8] ? m : smx[w8];
  f2g_f16_scales(m, s, rs);
}

// one unit = (k step, pixel group): the three MFMAs of a product tile.  hi lo' goes first so that the two MFMAs into
// acx are not back to back; the order inside each accumulator set is split_f16.h's.
__device__ __forceinline__ void unit3(f32x16& acc, f32x16& acx, const f16x8 (&a)[2], const f16x8 (&w)[2]) {
  h3_term(1, acc, acx, a[0], a[1], w[0], w[1]);
  h3_term(0, acc, acx, a[0], a[1], w[0], w[1]);
  h3_term(2, acc, acx, a[0], a[1], w[0], w[1]);
}

// ---- forward ----------------------------------------------------------------------------------------
// conv32_s2_fwd6_kernel's roles: 54 k steps of 16 (27 taps x the two halves of the input channels), waves 0..5 take
// seven consecutive ones, waves 6 and 7 six; lane li = output channel holds its 16 bytes of hi and of lo of each of
// them.  Per phase a wave runs its k steps over two 32-pixel groups -- two ds_read_b128 per three MFMAs --, the eight
// partial 64 x 32 tiles meet in LDS and wave w owns 8 pixels of each group of the pair.  Four barriers per tile.
template <int TH_, int TW_>
__global__ __launch_bounds__(512, 1) void conv32_s2_fwd3h_kernel(const f2g_conv32_desc d, int tiles_w,
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
  unsigned* smx = reinterpret_cast<unsigned*>(smb + 2 * SUBB + REDB);   // [8 waves] patch maxima
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
  // chunk q of this thread = 4 channels of patch pixel px0 + 64 q = (row r, column xr), recomputed per tile (the
  // empty asm keeps the chunk arithmetic inside the tile loop: conv32_s2_fwd6_kernel)
  auto load_patch = [&](int tile, f32x4 (&pf)[NCHK]) {
    int sq, h0, w0;
    tile_pos(tile, sq, h0, w0);
    const int x0 = 2 * w0 - (KW - 1) / 2;
    const float* org = d.x + (long long)sq * d.x_seq + (long long)(h0 - 1) * d.x_line + (long long)x0 * C + c4 * 4;
    const int xl = (int)d.x_line;                // (< 2^24, checked by the launcher: row offsets fit 32 bits)
    int pxb = px0;
    asm volatile("" : "+v"(pxb));
#pragma unroll
    for (int q = 0; q < NCHK; ++q) {
      const int px = pxb + 64 * q;
      const int r = div_small<XW>(px), xr = px - r * XW;
      const int h = h0 - 1 + r, x = x0 + xr;
      const bool ok = px < IHv * XW && h >= 0 && h < d.H && x >= 0 && x < d.Win;
      pf[q] = *reinterpret_cast<const f32x4*>(ok ? org + (r * xl + xr * C) : c32_zero);
    }
  };
  auto store_patch = [&](const f32x4 (&pf)[NCHK], float s) {
    int pxb = px0;
    asm volatile("" : "+v"(pxb));
#pragma unroll
    for (int q = 0; q < NCHK; ++q) {
      const int px = pxb + 64 * q;
      const int r = div_small<XW>(px), xr = px - r * XW;
      if (px < IHv * XW) store_px2(At + (xr & 1) * SUBB + (r * IWv + (xr >> 1)) * PB + c4 * 8, pf[q], s);
    }
  };
  int tile = blockIdx.x;
  if (tile >= ntiles) return;
  f32x4 pf[NCHK];
  load_patch(tile, pf);
  // this wave's k steps k0 .. k0 + nk - 1 (k = 2 tap + channel half): weight fragments for the block's life and the
  // wave-uniform patch offsets (the image is [co][27 taps][hi, lo][32] halves = 128 bytes per (co, tap))
  const int k0 = wave * KPW - (wave == 7 ? 1 : 0);
  const bool seven = wave < 6;
  f16x8 wf[KPW][2];
  int koff[KPW];
  {
    const unsigned char* wrow = reinterpret_cast<const unsigned char*>(d.w) + li * (NTAP * WSEG) + hh * 16;
#pragma unroll
    for (int j = 0; j < KPW; ++j) {
      int k = k0 + j;
      k = k < NKS ? k : NKS - 1;                      // (the unused seventh step of waves 6, 7: any valid one)
      const int t = k >> 1, ks = k & 1;
      const int dh = t / KW, jw = t - dh * KW;
      koff[j] = (jw & 1) * SUBB + (dh * IWv + (jw >> 1)) * PB + ks * 32;
#pragma unroll
      for (int q = 0; q < 2; ++q) wf[j][q] = *reinterpret_cast<const f16x8*>(wrow + t * WSEG + q * 64 + ks * 32);
    }
  }
  const float rsw = d.w[WFLOATS];
  int ph, pw;                                   // this lane's output pixel inside pixel group 0
  px_of_row<TW_>(0, li, ph, pw);
  const unsigned char* Ap = At + (ph * IWv + pw) * PB + hh * 16;
  // owner role: pixel (wave & 3) * 8 + (lane >> 3) of pixel group 2 * phase + (wave >> 2), channels 4 (lane & 7) ..
  const int orow = (wave & 3) * 8 + (lane >> 3), och = 4 * (lane & 7);
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (d.bias) bias4 = f32x4{d.bias[och], d.bias[och + 1], d.bias[och + 2], d.bias[och + 3]};
  // the first patch's scale: the waves' maxima meet in LDS
  {
    const unsigned m = patch_amax(pf);
    if (lane == 0) smx[wave] = m;
  }
  __syncthreads();
  float s_cur, rs_cur;
  patch_scales(smx, s_cur, rs_cur);
  store_patch(pf, s_cur);
  __syncthreads();
  for (; tile < ntiles; tile += gridDim.x) {
    const int nxt = tile + gridDim.x;
    const bool more = nxt < ntiles;
    load_patch(more ? nxt : tile, pf);          // (the last tile re-requests its own: never stored)
    int sq, h0, w0;
    tile_pos(tile, sq, h0, w0);
    float* ys = d.y + (long long)sq * d.y_seq;
#pragma unroll
    for (int p2 = 0; p2 < 2; ++p2) {
      f32x16 acc[2], acx[2];
      h3_zero<2>(acc, acx);
      // unit u = (k step u >> 1, pixel group 2 p2 + (u & 1)): the two fragments of unit u + 1 are requested in front
      // of unit u's three MFMAs, and the scheduler may not move anything across a unit's end (conv32_s2_fwd6_kernel)
      f16x8 a[2][2];
#pragma unroll
      for (int q = 0; q < 2; ++q) a[0][q] = *reinterpret_cast<const f16x8*>(Ap + koff[0] + 2 * p2 * PGB + q * 64);
#pragma unroll
      for (int u = 0; u < 2 * KPW; ++u) {
        const int j = u >> 1, g2 = u & 1;
        if (u + 1 < 2 * KPW) {                     // (waves 6, 7 read their clamped seventh step and drop it)
          const unsigned char* an = Ap + koff[(u + 1) >> 1] + (2 * p2 + ((u + 1) & 1)) * PGB;
#pragma unroll
          for (int q = 0; q < 2; ++q) a[(u + 1) & 1][q] = *reinterpret_cast<const f16x8*>(an + q * 64);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (j < KPW - 1 || seven) {
          unit3(acc[g2], acx[g2], a[u & 1], wf[j]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (p2) {
        // the next patch's largest magnitude, a tile's MFMAs after its loads were requested
        const unsigned m = patch_amax(pf);
        if (lane == 0) smx[wave] = m;
        __syncthreads();                          // the owners have read phase 0
      }
#pragma unroll
      for (int g2 = 0; g2 < 2; ++g2)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          red[((wave * 2 + g2) * 32 + acc_row(e) + 4 * hh) * 32 + li] = acc[g2][e] + acx[g2][e] * 0x1p-11f;
      __syncthreads();                            // (phase 1: every wave is also done with this tile's patch)
      f32x4 s = *reinterpret_cast<const f32x4*>(red + (((wave >> 2)) * 32 + orow) * 32 + och);
#pragma unroll
      for (int w8 = 1; w8 < 8; ++w8) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(red + ((w8 * 2 + (wave >> 2)) * 32 + orow) * 32 + och);
        s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
      }
      s.x = s.x * rs_cur * rsw + bias4.x, s.y = s.y * rs_cur * rsw + bias4.y;
      s.z = s.z * rs_cur * rsw + bias4.z, s.w = s.w * rs_cur * rsw + bias4.w;
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
      if (p2 && more) {                           // the next tile's patch under its own scale
        patch_scales(smx, s_cur, rs_cur);
        store_patch(pf, s_cur);
      }
      if (p2) __syncthreads();                    // the patch is staged; the owners are done with `red` and `smx`
    }
  }
}

// ---- data gradient -----------------------------------------------------------------------------------
// conv32_s2_dgrad6_kernel's roles: a tile is 128 positions m x BOTH column parities of the input, from ONE staged
// gradient patch under ONE scale; waves 0..3 compute the even input columns (30 k steps of 16 output channels, split
// 8 / 8 / 7 / 7), waves 4..7 the odd ones (24 k steps, 6 each); a wave holds the hi and lo fragments of its k steps
// (<= 64 registers), and per phase the four partial tiles of a parity meet through LDS in the fixed order of the
// waves; wave wq of a parity owns 16 positions of each phase as two 16-byte [position][channel] items.
// d.x = g (S, H, Wout, 32), d.y = gx (S, H, Win, 32),
// d.w = the one-run f2g_split_f16x2_seq image of wT [27 taps][ci][co] as an (864, 32) matrix: 128 bytes per (tap, ci).
template <int TH_, int TW_>
__global__ __launch_bounds__(512, 1) void conv32_s2_dgrad3h_kernel(const f2g_conv32_desc d, int tiles_w,
                                                                  int tiles_h, int ntiles) {
  constexpr int IHv = TH_ + KH - 1, GWv = TW_ + 4;
  constexpr int NCHK = (IHv * GWv * (C / 4) + 511) / 512;
  constexpr int PGB = (TW_ == 16 ? 2 : 4) * GWv * PB;    // bytes from a position group's staged pixels to the next's
  constexpr int KPW = 8;                                 // k steps of a wave at most
  static_assert(TH_ * TW_ == 128, "a block owns 128 positions of each column parity");
  extern __shared__ __attribute__((aligned(16))) unsigned char smb[];
  unsigned char* At = smb;                               // [IHv][GWv] pixels
  float* red = reinterpret_cast<float*>(smb + IHv * GWv * PB);   // [8 waves][2 groups][32 positions][32 channels]
  unsigned* smx = reinterpret_cast<unsigned*>(smb + IHv * GWv * PB + REDB);   // [8 waves] patch maxima
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
  auto store_patch = [&](const f32x4 (&pf)[NCHK], float s) {
#pragma unroll
    for (int q = 0; q < NCHK; ++q) {
      const int px = px0 + 64 * q;
      if (px < IHv * GWv) store_px2(At + px * PB + c4 * 8, pf[q], s);
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
  f16x8 wf[KPW][2];
  int koff[KPW];
  {
    const unsigned char* wrow = reinterpret_cast<const unsigned char*>(d.w) + li * WSEG + hh * 16;
    const int nks = 2 * KH * NU;
#pragma unroll
    for (int j = 0; j < KPW; ++j) {
      int k = k0 + j;
      k = k < nks ? k : nks - 1;                      // (steps past nk: any valid one, never multiplied)
      const int ti = k >> 1, ks = k & 1;
      const int dh = E ? ti >> 2 : (ti * 13) >> 6;    // ti / NU for ti < 15 without a division
      const int u = ti - dh * NU;
      koff[j] = ks * 32 - (dh * GWv + u) * PB;
      asm volatile("" : "+v"(koff[j]));               // (kept in vector registers: as scalars two of them spill)
      const int tile_w = dh * KW + E + 2 * u;
#pragma unroll
      for (int q = 0; q < 2; ++q)
        wf[j][q] = *reinterpret_cast<const f16x8*>(wrow + tile_w * (C * WSEG) + q * 64 + ks * 32);
    }
  }
  const float rsw = d.w[WFLOATS];
  int ph, pw;
  px_of_row<TW_>(0, li, ph, pw);
  const unsigned char* Ap = At + ((ph + 2) * GWv + pw + 4) * PB + hh * 16;
  // owner role: item jj = position (wq & 1) * 16 + (lane >> 3) + 8 (jj & 1) of position group 2 (jj >> 1) + (wq >> 1),
  // channels 4 (lane & 7) ..
  const int och = 4 * (lane & 7);
  const bool msk = d.mask_src != nullptr, fm = d.fm_ref != nullptr;
  const float fmw = fm ? d.fm_w * (d.fm_wdev ? d.fm_wdev[0] : 1.f) : 0.f;
  float fmv = fmw, mslope = d.mask_slope;        // (in vector registers: the scalar file is full, see koff)
  asm volatile("" : "+v"(fmv), "+v"(mslope));
  float cs[4] = {0.f, 0.f, 0.f, 0.f};            // column sums of what this lane stores (channels och ..)
  {
    const unsigned m = patch_amax(pf);
    if (lane == 0) smx[wave] = m;
  }
  __syncthreads();
  float s_cur, rs_cur;
  patch_scales(smx, s_cur, rs_cur);
  store_patch(pf, s_cur);
  __syncthreads();
  for (; tile < ntiles; tile += gridDim.x) {
    const int nxt = tile + gridDim.x;
    const bool more = nxt < ntiles;
    load_patch(more ? nxt : tile, pf);
    int sq, h0, m0;
    tile_pos(tile, sq, h0, m0);
    // the mask of this tile's outputs is requested HERE, one 16-byte segment per item (conv32_s2_dgrad6_kernel); an
    // item's offset is the tile's (wave-uniform, 64 bits) + the lane's inside the tile (32 bits: y_line < 2^24),
    // recomputed where it is used; -1 = outside the map.
    const long long tbase = (long long)sq * d.y_seq + (long long)h0 * d.y_line + (long long)(2 * m0 + E) * C;
    auto item_off = [&](int jj) {
      int qh, qw, l8 = lane >> 3;
      asm volatile("" : "+v"(l8));               // (opaque: or every item's terms are hoisted and spilled)
      px_of_row<TW_>(2 * (jj >> 1) + (wq >> 1), (wq & 1) * 16 + l8 + 8 * (jj & 1), qh, qw);
      return (h0 + qh < d.H && m0 + qw < Wp) ? qh * (int)d.y_line + 2 * qw * C + och : -1;
    };
    f32x4 my[4];
    if (msk && !fm) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int o = item_off(jj);
        my[jj] = *reinterpret_cast<const f32x4*>(d.mask_src + (o >= 0 ? tbase + o : 0));
      }
    }
#pragma unroll
    for (int p2 = 0; p2 < 2; ++p2) {
      f32x16 acc[2], acx[2];
      h3_zero<2>(acc, acx);
      // units (k step, position group of this phase) with the next unit's fragments requested first
      f16x8 a[2][2];
#pragma unroll
      for (int q = 0; q < 2; ++q) a[0][q] = *reinterpret_cast<const f16x8*>(Ap + koff[0] + 2 * p2 * PGB + q * 64);
#pragma unroll
      for (int u = 0; u < 2 * KPW; ++u) {
        const int j = u >> 1, g2 = u & 1;
        if (u + 1 < 2 * KPW) {
          const unsigned char* an = Ap + koff[(u + 1) >> 1] + (2 * p2 + ((u + 1) & 1)) * PGB;
#pragma unroll
          for (int q = 0; q < 2; ++q) a[(u + 1) & 1][q] = *reinterpret_cast<const f16x8*>(an + q * 64);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (j < 6 || j < nk) {
          unit3(acc[g2], acx[g2], a[u & 1], wf[j]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (p2) {
        const unsigned m = patch_amax(pf);        // the next patch's largest magnitude
        if (lane == 0) smx[wave] = m;
        __syncthreads();                          // the owners have read phase 0
      }
      // the mask + feature-matching instance requests this phase's two items of both maps here, in front of the
      // partial tiles' way through LDS
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
          red[((wave * 2 + g2) * 32 + acc_row(e) + 4 * hh) * 32 + li] = acc[g2][e] + acx[g2][e] * 0x1p-11f;
      __syncthreads();                            // (phase 1: every wave is also done with this tile's patch)
      // ---- epilogue: the two scales, optional leaky-ReLU backward of the layer below (+ feature-matching term),
      // column sums.  Three separate paths, so that the plain and the mask path carry no wait of the path with two maps.
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
        float v[4] = {s.x * rs_cur * rsw, s.y * rs_cur * rsw, s.z * rs_cur * rsw, s.w * rs_cur * rsw};
        if (msk && !fm) {
          const float y[4] = {my[jj].x, my[jj].y, my[jj].z, my[jj].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = c32_mask_fm(v[e], y[e], false, [] { return 0.f; }, 0.f, mslope);
        } else if (msk) {
          const float y[4] = {my[jj].x, my[jj].y, my[jj].z, my[jj].w}, f[4] = {fv[i2].x, fv[i2].y, fv[i2].z, fv[i2].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = c32_mask_fm(v[e], y[e], true, [&] { return f[e]; }, fmv, mslope);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) cs[e] += v[e];
        *reinterpret_cast<f32x4*>(d.y + tbase + o) = f32x4{v[0], v[1], v[2], v[3]};
      }
      if (p2 && more) {                           // the next tile's patch under its own scale
        patch_scales(smx, s_cur, rs_cur);
        store_patch(pf, s_cur);
      }
      if (p2) __syncthreads();                    // the patch is staged; the owners are done with `red` and `smx`
    }
  }
  // column sums: the waves' sums meet in LDS (the patch: the last barrier is behind every read of it) and leave as
  // ONE 32-lane atomic per block (conv32_s2_dgrad6_kernel)
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

template <int TH_, int TW_>
constexpr size_t fwd3h_smem() {
  return (size_t)2 * ((TH_ + 2) * (TW_ + 4) * PB + 64) + REDB + 64;
}
template <int TH_, int TW_>
constexpr size_t dgrad3h_smem() {
  return (size_t)(TH_ + 2) * (TW_ + 4) * PB + REDB + 64;
}

}  // namespace

// precision-4 launchers, called from conv32.hip's entry points (arguments already checked there)
int f2g_conv32_fwd3h_launch(const f2g_conv32_desc* d, hipStream_t st) {
  const c32_tiling t = c32_pick_tiles(d->H, d->Wout);
  const long long nt = (long long)t.tiles_h * t.tiles_w * d->S;
  if (nt >= (1ll << 30) || d->x_line >= (1ll << 24)) return F2G_EINVAL;
  const int grid = (int)(nt < 256 ? nt : 256);          // one resident block per CU
  return c32_launch_shape<conv32_s2_fwd3h_kernel<8, 16>, conv32_s2_fwd3h_kernel<16, 8>>(
      t.tall, fwd3h_smem<8, 16>(), fwd3h_smem<16, 8>(), dim3(grid), dim3(512), st, *d, t.tiles_w, t.tiles_h, (int)nt);
}

int f2g_conv32_dgrad3h_launch(const f2g_conv32_desc* d, hipStream_t st) {
  const c32_tiling t = c32_pick_tiles(d->H, (d->Win + 1) / 2);   // positions m: the even parity has the most
  const long long nt = (long long)t.tiles_h * t.tiles_w * d->S;
  if (nt >= (1ll << 30) || d->x_line >= (1ll << 24) || d->y_line >= (1ll << 24)) return F2G_EINVAL;
  const int grid = (int)(nt < 256 ? nt : 256);
  return c32_launch_shape<conv32_s2_dgrad3h_kernel<8, 16>, conv32_s2_dgrad3h_kernel<16, 8>>(
      t.tall, dgrad3h_smem<8, 16>(), dgrad3h_smem<16, 8>(), dim3(grid), dim3(512), st, *d, t.tiles_w, t.tiles_h,
      (int)nt);
}
