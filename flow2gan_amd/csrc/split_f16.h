// The image side of fp16x3 (gemm_f16_common.h: the GEMM side).  Row routine of f2g_split_f16x2 (gemm_f16.hip) and of
// its f2g_multi entry (multi.hip: weight images rebuilt in one batched launch): the two-piece fp16 image of fp32 rows
// and their reciprocal scales.  f2g_split_f16x2_cols (gemm_f16.hip: K-major operands, one scale per COLUMN) and
// f2g_split_f16x2_seq (gemm_f16p.hip: one scale per sequence of a halo map) share the arithmetic below.
#pragma once
#include "common.h"

// ---- the arithmetic -----------------------------------------------------------------------------------------------
// A row x of K floats, amax = max |x|, e = floor(log2 amax): the row is scaled by the power of two s = 2^(14 - e)
// (largest element in [2^14, 2^15): inside fp16's range whatever the row's magnitude; the exponent is clamped to
// +-126 so that s and 1 / s are both normal floats; s = 1 for an all-zero row and for a row that holds an inf or a
// NaN, whose values then stay non-finite).  y = x s (exact), hi = fp16(y) (nearest even), r = y - hi (exact in
// fp32), lo = fp16(2^11 r): the factor puts lo into hi's exponent range (|r| <= ulp(hi) / 2 = 2^-11 |hi|), so lo is
// a NORMAL fp16 wherever hi is one, and both are subnormal only for elements 2^-28 below their row's largest.
// y = hi + 2^-11 lo to 2^-22 |y|.  A product is then
//   acc0 += hi_a hi_b      acc1 += hi_a lo_b + lo_a hi_b       (lo lo dropped: <= 2^-22 |a b|)
//   v = (acc0 + 2^-11 acc1) / s_a[row] / s_b[col]
// three v_mfma_f32_32x32x16_f16 per product, fp32 accumulation: <= 3 * 2^-22 |a| |b| per product.
constexpr int F2G_F16_MAX_K = 4096;      // f2g_split_f16x2 keeps a row in registers: 16 chunks of 16 bytes per lane
constexpr int F2G_F16_CHUNKS = F2G_F16_MAX_K / 4 / 64;

__device__ __forceinline__ unsigned f2g_f16_pair(float y0, float y1, unsigned& lo) {
  const _Float16 h0 = (_Float16)y0, h1 = (_Float16)y1;      // v_cvt_f16_f32: round to nearest even, inf / NaN kept
  const _Float16 l0 = (_Float16)__fmul_rn(__fsub_rn(y0, (float)h0), 2048.f);
  const _Float16 l1 = (_Float16)__fmul_rn(__fsub_rn(y1, (float)h1), 2048.f);
  lo = __builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
  return __builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
}

__device__ __forceinline__ unsigned f2g_f16_amax4(const float4& v, unsigned m) {
  const unsigned a = __float_as_uint(v.x) & 0x7fffffffu, b = __float_as_uint(v.y) & 0x7fffffffu;
  const unsigned c = __float_as_uint(v.z) & 0x7fffffffu, d = __float_as_uint(v.w) & 0x7fffffffu;
  const unsigned ab = a > b ? a : b, cd = c > d ? c : d;
  const unsigned q = ab > cd ? ab : cd;
  return m > q ? m : q;
}

__device__ __forceinline__ uint4 f2g_f16_split4(const float4& v, float s) {
  unsigned l01, l23;
  const unsigned h01 = f2g_f16_pair(__fmul_rn(v.x, s), __fmul_rn(v.y, s), l01);
  const unsigned h23 = f2g_f16_pair(__fmul_rn(v.z, s), __fmul_rn(v.w, s), l23);
  return make_uint4(h01, h23, l01, l23);
}

// ... with one scale per element (four columns of a K-major operand)
__device__ __forceinline__ uint4 f2g_f16_split4(const float4& v, const float4& s) {
  unsigned l01, l23;
  const unsigned h01 = f2g_f16_pair(__fmul_rn(v.x, s.x), __fmul_rn(v.y, s.y), l01);
  const unsigned h23 = f2g_f16_pair(__fmul_rn(v.z, s.z), __fmul_rn(v.w, s.w), l23);
  return make_uint4(h01, h23, l01, l23);
}

// The scale s = 2^sexp of a row (column, sequence) whose largest sign-less bit pattern is m, and its reciprocal rs
__device__ __forceinline__ void f2g_f16_scales(unsigned m, float& s, float& rs) {
  int sexp = 14 - ((int)(m >> 23) - 127);          // (a subnormal amax: beyond the clamp either way)
  sexp = sexp > 126 ? 126 : (sexp < -126 ? -126 : sexp);
  sexp = (m == 0u || m >= 0x7f800000u) ? 0 : sexp;
  s = __uint_as_float((unsigned)(127 + sexp) << 23);
  rs = __uint_as_float((unsigned)(127 - sexp) << 23);
}

// Largest m of a wave's 64 lanes, in every lane (a fixed butterfly, no atomics)
__device__ __forceinline__ unsigned f2g_wave_max(unsigned m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = (unsigned)__shfl_xor((int)m, o);
    m = m > t ? m : t;
  }
  return m;
}

// One wave per row: its largest magnitude is the integer maximum of the sign-less bit patterns (the same order as
// the values'; a NaN ranks above inf; a fixed butterfly, no atomics), then every aligned group of four floats is
// stored as four hi and four lo halves -- the 16 bytes of f2g_split_bf16 at the same offset.  dst may be src.
// KEEP: the row is read ONCE with 16-byte loads and kept in registers between the two steps (f2g_split_f16x2: 64
// registers for the row, 94 in all; activations are read from HBM once); !KEEP: it is read a second time (the f2g_multi entry: weight rows,
// which the second read finds in the cache -- the table kernel stays at 38 registers instead of 94 and keeps its occupancy for the
// other kinds).  The arithmetic, and so the image, is the same.
// Rows w0, w0 + nw, ... are this wave's (w0 = its index among the nw waves that share the matrix).
template <bool KEEP>
__device__ __forceinline__ void f2g_split_f16x2_rows(float* dst, float* __restrict__ rscale, const float* src,
                                                     long long ld, int rows, int K, long long w0, long long nw) {
  const int lane = threadIdx.x & 63, K4 = K >> 2;
  for (long long r = w0; r < rows; r += nw) {
    const float4* s4 = reinterpret_cast<const float4*>(src + r * ld);
    float4 v[KEEP ? F2G_F16_CHUNKS : 1];
    unsigned m = 0;
    if constexpr (KEEP) {
#pragma unroll
      for (int j = 0; j < F2G_F16_CHUNKS; ++j) {
        const int c = lane + 64 * j;
        v[j] = c < K4 ? s4[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        m = f2g_f16_amax4(v[j], m);
      }
    } else {
      for (int c = lane; c < K4; c += 64) m = f2g_f16_amax4(s4[c], m);
    }
    float s, rs;
    f2g_f16_scales(f2g_wave_max(m), s, rs);
    if (lane == 0) rscale[r] = rs;
    uint4* d4 = reinterpret_cast<uint4*>(dst + r * ld);
    if constexpr (KEEP) {
#pragma unroll
      for (int j = 0; j < F2G_F16_CHUNKS; ++j) {
        const int c = lane + 64 * j;
        if (c < K4) d4[c] = f2g_f16_split4(v[j], s);
      }
    } else {
      for (int c = lane; c < K4; c += 64) d4[c] = f2g_f16_split4(s4[c], s);
    }
  }
}
