// What the direct MRD band convolutions share (conv32.hip: exact fp32 and split-bf16; conv32x6.hip: fp32 class;
// conv32h3.hip, conv32h3w.hip, conv33h3.hip: fp16x3): the vector types and layer constants, the accumulator-row map, the map from MFMA rows to
// tile pixels and the small divisions of the kernels that stage split pixels, the transposed fragment read of the
// weight gradients, the pick between the two tile shapes and their launch, the store expression of the data
// gradients and the flush of the weight gradients.  What a kernel stages and how it walks its taps stay with the kernel.
// Internal linkage throughout.
#pragma once
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int C = 32;                   // channels in = out
constexpr int KH = 3, KW = 9;           // the (3, 9) layer's taps

// source of every staged chunk that lies outside the map
__device__ __attribute__((aligned(16))) float c32_zero[4] = {0.f, 0.f, 0.f, 0.f};

// element e of a 32 x 32 MFMA accumulator sits on tile row (e & 3) + 8 (e >> 2) + 4 hh of lane half hh
__device__ __forceinline__ constexpr int acc_row(int e) { return (e & 3) + 8 * (e >> 2); }

// K-major fragment out of bf16 planes with 64-byte pixels (ds_read_b64_tr_b16): pixels +0..3 and +4..7
__device__ __forceinline__ bf16x8 tr_pix8(const unsigned char* p) {
  typedef s16x4 __attribute__((address_space(3))) * lds_p;
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(p));
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(p + 4 * 64));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

// x / D for 0 <= x < 512 and the staged widths that occur (39, 23: forward patch columns; 20, 12: gradient patch)
template <int D>
__device__ __forceinline__ int div_small(int x) {
  static_assert(D == 39 || D == 23 || D == 20 || D == 12, "magic constants below");
  return (x * (D == 39 ? 1681 : D == 23 ? 2850 : D == 20 ? 3277 : 5462)) >> 16;
}

// MFMA row r (0..31) of pixel group pg -> pixel (row, column) of a TH x TW tile of the kernels that stage split
// pixels (conv32x6.hip: 208-byte pixels, 52 dwords; conv32h3.hip: 144-byte pixels, 36 dwords).  16-wide tiles: the
// wave's rows 16..31 are the next tile row, whose staged pixels sit (IW - 16) * 52 = 16 (mod 64) dwords further than
// "16 lanes on" -- in ds_read_b128's lane groups {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} that puts four
// lanes of the second row on the banks of the first (measured: 31 % of the LDS cycles were conflicts).
// Rotating the second row's columns by 12 makes every group's sixteen 16-byte reads hit distinct banks.
// (36-dword pixels: (IW - 16) * 36 = 16 (mod 64) as well, and 36 / 4 = 9 is odd like 52 / 4 = 13, so sixteen
// consecutive columns cover the sixteen 16-byte bank groups once: the same rotation serves both pitches.
// Enumerated over those lane groups, 8-wide tiles keep a two-way overlap at either pitch: their rows are 12 pixels
// apart, so lanes 12-15 land on the banks of lanes 0-3; no rotation is applied there.)
template <int TW_>
__device__ __forceinline__ void px_of_row(int pg, int r, int& ph, int& pw) {
  if (TW_ == 16) {
    ph = 2 * pg + (r >> 4);
    pw = (r + 12 * (r >> 4)) & 15;
  } else {
    const int p = pg * 32 + r;
    ph = p / TW_;
    pw = p % TW_;
  }
}

// ---- tile shape: 8 x 16 or 16 x 8 output pixels, whichever wastes fewer pixels of the map, 8 x 16 on a tie.
// W = the columns to tile (Wout; per-parity column counts in the data gradients).  W_also > 0: a second column
// count tiled beside W whose waste counts too -- the exact-fp32 data gradient walks both column parities on the
// picked shape and weighs both, the fp32-class one (one tile = both parities) weighs the even parity alone.
struct c32_tiling {
  bool tall;                            // 16 x 8
  int tiles_h, tiles_w, tiles_w_also;
};
inline c32_tiling c32_pick_tiles(int H, int W, int W_also = 0) {
  auto waste = [&](int th, int tw) {
    return (long long)((H + th - 1) / th * th) * ((W + tw - 1) / tw * tw + (W_also + tw - 1) / tw * tw);
  };
  const bool tall = waste(16, 8) < waste(8, 16);
  const int th = tall ? 16 : 8, tw = tall ? 8 : 16;
  return {tall, (H + th - 1) / th, (W + tw - 1) / tw, (W_also + tw - 1) / tw};
}

// ---- the (3, 3) fifth layer (conv32x6.hip: conv33_x6_kernel, conv33_wgrad6_kernel; conv33h3.hip: conv33_h3_kernel):
// a tile is R WHOLE rows of a W-column band image, staged with a zero column on either side and a row above / below
constexpr int P33 = 352;                 // staged pixels of a tile: (R + 2) * (W + 2) <= P33
constexpr int T33 = 9;                   // taps
// its weight gradients (conv33_wgrad6_kernel, conv33h3w.hip: conv33_wgrad3h_kernel) stage patch and gradient rows in
// one padded flat order, a k step = 16 consecutive flat positions
constexpr int W33_GP = 352;      // gradient positions of a tile: R * (W + 2) rounded up to a k step
constexpr int W33_XP = 384;      // input positions: 1 + (R + 2) * (W + 2) + the last k step's overhang
constexpr int W33_GPL = W33_GP * 64, W33_XPL = W33_XP * 64;   // bytes of one plane of 64-byte pixels
// (largest input position a fragment touches: (R + 2) * (W + 2) + 17; gradient positions: R * (W + 2) + 15)
static_assert(P33 + 18 <= W33_XP && P33 <= W33_GP, "plane sizes");

// rows per tile: R * W <= 256 pixels where the staged patch allows it; 0 = not even one row fits (W > 112)
inline int c33_pick_rows(int H, int W) {
  int R = 256 / W;
  if (R > H) R = H;
  while (R > 1 && (R + 2) * (W + 2) > P33) --R;
  return (R < 1 || (R + 2) * (W + 2) > P33) ? 0 : R;
}

// a kernel instance's dynamic LDS limit, raised once per process (thread-safe: a function-local static)
template <auto KERNEL>
inline void c32_lds_once(size_t smem) {
  static const hipError_t done = [&] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)smem);
  }();
  (void)done;
}

// launch of the shape c32_pick_tiles chose out of a kernel's <8, 16> and <16, 8> instances
template <auto K8x16, auto K16x8, typename... Args>
inline int c32_launch_shape(bool tall, size_t smem8x16, size_t smem16x8, dim3 grid, dim3 block, hipStream_t st,
                            Args... args) {
  c32_lds_once<K8x16>(smem8x16);
  c32_lds_once<K16x8>(smem16x8);
  if (tall) hipLaunchKernelGGL(K16x8, grid, block, smem16x8, st, args...);
  else hipLaunchKernelGGL(K8x16, grid, block, smem8x16, st, args...);
  return f2g_check_launch();
}

// ---- store expression of the data gradients: the feature-matching sign term against the reference map (fm; ref()
// reads its value and is called only then), then the leaky-ReLU backward of the layer below, whose output was y
template <typename REF>
__device__ __forceinline__ float c32_mask_fm(float v, float y, bool fm, REF ref, float fmw, float mask_slope) {
  if (fm) {
    const float dl = y - ref();
    v += fmw * (dl > 0.f ? 1.f : (dl < 0.f ? -1.f : 0.f));
  }
  return v * (y > 0.f ? 1.f : mask_slope);
}

// ---- flush of a weight gradient: gw (32, NT * 32) [co][tap][ci] += the block's NT accumulator tiles (rows = co,
// columns = ci).  Wave w of 8 owns the taps w + 8 q, q < OWN, over all pixels (acc[q]): they go straight out as
// atomics.  Of the other NT - 8 * OWN taps every wave holds a partial tile (acc[OWN + q]): they are summed over
// the waves through LDS (red: [8 waves][16][64 lanes] floats, anything of the block's that is dead by now), one
// tap at a time, and leave as one atomic per output and block.  wave, lane = the thread's; li = lane & 31, hh =
// lane >> 5.  (The kernel's own values and the LDS address space spelled out: with the roles recomputed here, or
// red left a generic pointer until it is inlined, the compiler pairs fewer of the reduction's LDS reads and
// conv32_s2_wgrad_p_kernel changes a register count -- profiles/conv32_shared_isa.txt.)
template <int NT, int OWN>
__device__ __forceinline__ void c32_wgrad_flush(float* gw, float* red_, const f32x16 (&acc)[OWN + NT - 8 * OWN],
                                                int wave, int lane, int li, int hh) {
  typedef float __attribute__((address_space(3))) * lds_f;
  const lds_f red = (lds_f)red_;
#pragma unroll
  for (int q = 0; q < OWN; ++q) {
    const int t = wave + 8 * q;
#pragma unroll
    for (int e = 0; e < 16; ++e) atomicAdd(gw + (acc_row(e) + 4 * hh) * (NT * C) + t * C + li, acc[q][e]);
  }
#pragma unroll
  for (int q = 0; q < NT - 8 * OWN; ++q) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 16; ++e) red[(wave * 16 + e) * 64 + lane] = acc[OWN + q][e];
    __syncthreads();
    if (wave == (q & 7)) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float v = 0.f;
#pragma unroll
        for (int w8 = 0; w8 < 8; ++w8) v += red[(w8 * 16 + e) * 64 + lane];
        atomicAdd(gw + (acc_row(e) + 4 * hh) * (NT * C) + (8 * OWN + q) * C + li, v);
      }
    }
  }
}

}  // namespace
