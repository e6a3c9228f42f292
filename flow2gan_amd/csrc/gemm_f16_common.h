// The GEMM side of fp16x3 (split_f16.h has the image side), shared by the kernels of gemm_f16*.hip (gemm_f16.hip:
// h3_table lists them): the fragment type, the K-major fragment read, the three MFMAs of a product tile, zeroing and
// rescaling the two accumulator sets.  What a
// kernel stages and where its fragments and scales lie stay with the kernel.  Internal linkage throughout.
#pragma once
#include <type_traits>

#include "gemm_common.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// K-major fragment read (gemm_common.h: tr_frag, the bf16 kernels') out of planes whose rows lie PITCH bytes apart;
// the second half of the read -- four reduction rows further -- lies HALF plane rows further (4, or 4 * stride where
// consecutive reduction rows are `stride` plane rows apart: gemm_h3ws_kernel)
template <int PITCH, int HALF = 4>
__device__ __forceinline__ f16x8 tr_frag_f16(const unsigned char* p) {
  typedef s16x4 __attribute__((address_space(3))) * lds_p;
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(p));
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(p + HALF * PITCH));
  const s16x8 v = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(f16x8, v);
}

// A product tile (split_f16.h has the arithmetic): acc += hi hi', acx += hi lo' + lo hi' -- term 0, 1, 2 = the three
// v_mfma_f32_32x32x16_f16 in that order (a constant once the callers' loops are unrolled)
__device__ __forceinline__ void h3_term(int term, f32x16& acc, f32x16& acx, const f16x8& ah, const f16x8& al,
                                        const f16x8& bh, const f16x8& bl) {
  if (term == 0) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
  else acx = __builtin_amdgcn_mfma_f32_32x32x16_f16(term == 1 ? ah : al, term == 1 ? bl : bh, acx, 0, 0, 0);
}

__device__ __forceinline__ void h3_product(f32x16& acc, f32x16& acx, const f16x8& ah, const f16x8& al,
                                           const f16x8& bh, const f16x8& bl) {
#pragma unroll
  for (int term = 0; term < 3; ++term) h3_term(term, acc, acx, ah, al, bh, bl);
}

// The twelve MFMAs of a 16-k step of a 2 x 2 tile (ah, al: the hi and lo fragments of the two row sub-tiles; bh, bl:
// of the two column sub-tiles), term by term: four acc, four acx, four acx
__device__ __forceinline__ void h3_mfma12(f32x16 (&acc)[2][2], f32x16 (&acx)[2][2], const f16x8* ah, const f16x8* al,
                                          const f16x8* bh, const f16x8* bl) {
#pragma unroll
  for (int term = 0; term < 3; ++term)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) h3_term(term, acc[mi][ni], acx[mi][ni], ah[mi], al[mi], bh[ni], bl[ni]);
}

// Largest m of a wave's 64 lanes as a wave-uniform value, WITHOUT an LDS round trip (split_f16.h's f2g_wave_max is six
// dependent ds_bpermute: several hundred cycles that would sit between a slab's last MFMA and its barrier): four DPP
// steps inside every row of 16 lanes (the two quad permutations, the half-row and the row mirror: after them every
// lane holds its row's maximum), then the four rows through v_readlane and scalar maxima.  Every lane is active where
// this is called.  The same order-free integer maximum: reproducible.  (gemm_h3n_kernel, gemm_h3wn_kernel: the slab
// maxima of the operands they scale themselves)
__device__ __forceinline__ unsigned h3n_wave_max(unsigned m) {
  auto step = [&](auto ctrl) {
    const unsigned t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, decltype(ctrl)::value, 0xf, 0xf, false);
    m = m > t ? m : t;
  };
  step(std::integral_constant<int, 0xB1>{});      // quad_perm [1, 0, 3, 2]
  step(std::integral_constant<int, 0x4E>{});      // quad_perm [2, 3, 0, 1]
  step(std::integral_constant<int, 0x141>{});     // row_half_mirror
  step(std::integral_constant<int, 0x140>{});     // row_mirror
  const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)m, 0), b = (unsigned)__builtin_amdgcn_readlane((int)m, 16);
  const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)m, 32), e = (unsigned)__builtin_amdgcn_readlane((int)m, 48);
  const unsigned ab = a > b ? a : b, ce = c > e ? c : e;
  return ab > ce ? ab : ce;
}

// Both accumulator sets of N tiles to zero
template <int N>
__device__ __forceinline__ void h3_zero(f32x16* acc, f32x16* acx) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = acx[i][e] = 0.f;
}

// v = (acc0 + 2^-11 acc1) / s_a / s_b with the RECIPROCAL scales sa, sb, one after the other (their product may leave
// the float range)
__device__ __forceinline__ float h3_value(float acc, float acx, float sa, float sb) {
  return (acc + acx * 0x1p-11f) * sa * sb;
}

}  // namespace
