// fp16x3 instance of the fifth layer of an MRD band stack (conv32x6.hip has the bf16x6 one, conv33_x6_kernel; reference
// discriminators.py:171-181, last entry: Conv2d(32, 32, (3, 3), padding (1, 1)), stride 1): f2g_conv33_fwd at
// f2g_conv32_desc.precision = 4.  Every fp32 value is two SCALED fp16 pieces and a product three
// v_mfma_f32_32x32x16_f16 into two accumulator sets (split_f16.h has the arithmetic, gemm_f16_common.h the MFMA side):
// 54 MFMAs per wave and tile where the six-product kernel issues 108, two pieces to split per staged float instead of
// three, 144-byte staged pixels instead of 208-byte ones.
//
// Roles and tiling are conv33_x6_kernel's: one persistent block of 8 waves per CU walks tiles b, b + grid, ...; a
// tile is R WHOLE rows (c33_pick_rows) staged with a zero column on either side and one row above / below, so the nine
// taps are nine constant offsets into the staged patch; wave w owns tile pixels 32 w .. 32 w + 31 over the whole
// reduction (no partial tiles meet anywhere: apart from the colsum atomics the result is bit-reproducible); the next
// tile's patch is requested into registers before the current tile's MFMAs.  The data gradient is the same kernel over
// the gradient map with the host's [ci][8 - tap][co] re-layout of the weights.
//
// ONE SCALE PER PATCH, TAKEN INSIDE THE KERNEL (conv32h3.hip's mechanism): every window of the tile lies inside the
// staged (R + 2) x (W + 2) patch, so one power of two over every float of it -- the halo rows included; the border
// columns and the rows outside the map read as zeros and do not count -- factors out of every output of the tile
// exactly.  It is taken from the registers that hold the next patch: a register pass, a wave butterfly, eight LDS
// words.  Per output
//   |err| <= 3 * 2^-22 sum |a||w| + 2^-28 (amax_patch sum_k |w_k| + wmax sum_k |a_k|).
// A patch whose largest magnitude is zero, inf or NaN takes scale 1 (conv32h3.hip's policy: non-finite values stay
// non-finite, the tile's other outputs are then not defined beyond "the windows that hold the NaN are NaN"; other
// tiles are untouched).
//
// The weights arrive as ONE f2g_split_f16x2_seq run over the whole contiguous (32, 9 * 32) matrix (9216 floats; 128
// bytes per 32-float row segment: 32 hi halves, then 32 lo halves; the reciprocal scale is the float behind the
// image).  A wave multiplies every tap, so holding the weights in registers as the (3, 9) kernels do would take all
// eighteen k steps' hi and lo fragments = 144 registers per lane: built that way the kernel spilled 120 registers
// beside two accumulator pairs, the next patch and the mask, so the nine weight tiles stay in LDS for the block's life
// as in conv33_x6_kernel (rows (tap, co) of 144 bytes, 41 KB beside the 50 KB patch): a tap costs eight ds_read_b128
// per six MFMAs where the six-product kernel reads twelve per twelve.
#include <stdlib.h>

#include "conv32_common.h"
#include "gemm_f16_common.h"
#include "split_f16.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int PB = 144;                    // bytes of a staged pixel / weight row: [32 hi | 32 lo | pad] halves
constexpr int WSEG = 128;                  // bytes of a 32-float row segment of the weight image
constexpr int WFLOATS = C * T33 * C;       // floats of the weight matrix: the reciprocal scale lies behind them

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

__global__ __launch_bounds__(512, 1) void conv33_h3_kernel(const f2g_conv32_desc d, int R, int tiles_h, int ntiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smb[];
  unsigned char* At = smb;                                           // [P33] staged pixels
  unsigned char* Bt = smb + P33 * PB;                                // [9 taps][32 co] weight rows
  unsigned* smx = reinterpret_cast<unsigned*>(smb + (P33 + T33 * C) * PB);   // [8 waves] patch maxima
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, hh = lane >> 5;
  const int W = d.Win, PW = W + 2, npx = (R + 2) * PW, tpx = R * W;
  const unsigned mgW = magic_of(W), mgPW = magic_of(PW);
  int tile = blockIdx.x;
  if (tile >= ntiles) return;
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
  auto load_patch = [&](int t, f32x4 (&pf)[NQ]) {
    const int sq = t / tiles_h, h0 = (t - sq * tiles_h) * R;
    const float* org = d.x + (long long)sq * d.x_seq + (long long)h0 * d.x_line;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int h = h0 - 1 + prow[q];
      pf[q] = *reinterpret_cast<const f32x4*>((h >= 0 && h < d.H) ? org + poff[q] : c32_zero);
    }
  };
  auto store_patch = [&](const f32x4 (&pf)[NQ], float s) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (pdst[q] >= 0) store_px2(At + pdst[q], pf[q], s);
  };
  f32x4 pf[NQ];
  load_patch(tile, pf);
  // weights: image [co][9 taps][128 bytes: 32 hi | 32 lo] -> LDS rows (tap, co) of 144 bytes, for the block's life
  {
    const unsigned char* wimg = reinterpret_cast<const unsigned char*>(d.w);
    for (int c = tid; c < T33 * C * 8; c += 512) {
      const int row = c >> 3, part = c & 7;                  // row = co * 9 + tap in the image
      const int co = row / T33, tap = row - co * T33;
      *reinterpret_cast<u32x4*>(Bt + (tap * C + co) * PB + part * 16) =
          *reinterpret_cast<const u32x4*>(wimg + row * WSEG + part * 16);
    }
  }
  const unsigned char* Bp = Bt + li * PB + hh * 16;
  const float rsw = d.w[WFLOATS];
  // this lane's output pixel: tile pixel 32 wave + li -> (row, column) -> staged position
  const int mypx = wave * 32 + li;
  const int myr = fast_div(mypx, W, mgW), myc = mypx - myr * W;
  const unsigned char* Ap = At + (mypx < tpx ? ((myr + 1) * PW + myc + 1) * PB : (PW + 1) * PB) + hh * 16;
  const float bias = d.bias ? d.bias[li] : 0.f;
  float slope = d.lrelu_slope, mslope = d.mask_slope;   // (in vector registers: as scalars two values spill)
  asm volatile("" : "+v"(slope), "+v"(mslope));
  float cs = 0.f;                                // column sums of what this lane stores (channel li)
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
    // hi hi' of both channel halves into ONE accumulator, the cross terms into one per half (a fourth accumulator
    // spills): per tap the four fragments of the staged pixel and of the weight row, then six MFMAs ordered so that no
    // two in a row share an accumulator
    f32x16 acc, acx[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = acx[0][e] = acx[1][e] = 0.f;
#pragma unroll
    for (int t = 0; t < T33; ++t) {
      const unsigned char* ap = Ap + ((t / 3 - 1) * PW + (t % 3 - 1)) * PB;
      const unsigned char* bp = Bp + t * (C * PB);
      f16x8 a[2][2], b[2][2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          a[ks][q] = *reinterpret_cast<const f16x8*>(ap + q * 64 + ks * 32);
          b[ks][q] = *reinterpret_cast<const f16x8*>(bp + q * 64 + ks * 32);
        }
      h3_term(1, acc, acx[0], a[0][0], a[0][1], b[0][0], b[0][1]);
      h3_term(1, acc, acx[1], a[1][0], a[1][1], b[1][0], b[1][1]);
      h3_term(0, acc, acx[0], a[0][0], a[0][1], b[0][0], b[0][1]);
      h3_term(2, acc, acx[0], a[0][0], a[0][1], b[0][0], b[0][1]);
      h3_term(0, acc, acx[1], a[1][0], a[1][1], b[1][0], b[1][1]);
      h3_term(2, acc, acx[1], a[1][0], a[1][1], b[1][0], b[1][1]);
    }
    // the next patch's largest magnitude, a tile's MFMAs after its loads were requested
    {
      const unsigned m = patch_amax(pf);
      if (lane == 0) smx[wave] = m;
    }
    {
      float* ys = d.y + ybase;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int p = wave * 32 + acc_row(e) + 4 * hh;
        const int r = fast_div(p, W, mgW), c = p - r * W;
        if (p < tpx && h0 + r < d.H) {
          float v = h3_value(acc[e], acx[0][e] + acx[1][e], rs_cur, rsw) + bias;
          if (slope != 0.f) v = v > 0.f ? v : slope * v;
          if (d.mask_src) v *= my[e] > 0.f ? 1.f : mslope;
          cs += v;
          ys[(long long)r * d.y_line + c * C + li] = v;
        }
      }
    }
    __syncthreads();                               // every wave is done with this patch; the maxima are written
    if (more) {                                    // the next tile's patch under its own scale
      patch_scales(smx, s_cur, rs_cur);
      store_patch(pf, s_cur);
    }
    __syncthreads();                               // the patch is staged; every wave has read `smx`
  }
  if (d.colsum) {
    cs += __shfl_xor(cs, 32);
    if (hh == 0) atomicAdd(d.colsum + li, cs);
  }
}

}  // namespace

// precision-4 launcher of f2g_conv33_fwd (conv32x6.hip: arguments already checked there, R rows per tile picked)
int f2g_conv33_h3_launch(const f2g_conv32_desc* d, int R, int tiles_h, int ntiles, hipStream_t st) {
  constexpr size_t smem = (size_t)(P33 + T33 * C) * PB + 64;   // patch, weight rows, the waves' maxima
  c32_lds_once<conv33_h3_kernel>(smem);
  const int grid = ntiles < 256 ? ntiles : 256;          // one resident block per CU
  hipLaunchKernelGGL(conv33_h3_kernel, dim3(grid), dim3(512), smem, st, *d, R, tiles_h, ntiles);
  return f2g_check_launch();
}
