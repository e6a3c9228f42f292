// What more than one of the GEMM translation units needs (gemm.hip, gemm_lean.hip, gemm_wgrad.hip, gemm_x6.hip,
// gemm_x6p.hip, gemm_f16*.hip): vector types, tile constants, the tile order, the generic epilogue, the K-major
// fragment read, the three-piece split, the LDS barrier, the lab switches, and the host functions that cross those
// files.  Everything defined here has internal linkage; no GEMM file includes another.  (gemm_f16_common.h: what only
// fp16x3 shares; gemm_f16_checks.h: its host-side checks.)
#pragma once
#include "common.h"

// ---- host functions that cross the GEMM files (f2g_gemm in gemm.hip dispatches to all of them) ---------------
// gemm_lean.hip: form 0 over operands the lean kernel reads (A: lean_a_ok, B: a plain [n][k] matrix)
bool f2g_lean_operands_ok(const f2g_gemm_desc& d);
bool f2g_lean_bf16_ok(const f2g_gemm_desc& d);      // ... also as TRUE bf16 tensors (split = 2)
int f2g_lean_stream_k(int M, int N, int K, bool all_grids);
int f2g_launch_lean(const f2g_gemm_desc& d, int M, int N, int K, int split, int upb, hipStream_t st);
// gemm_wgrad.hip: form 2 on the K-major kernels.  `pieces`: 1 exact fp32 (gemm_leanw_kernel), 3 pre-split
// split-bf16 images (gemm_leanw3_kernel), 6 fp32-class products on the bf16 pipe (gemm_leanw6_kernel)
bool f2g_leanw_ok(const f2g_gemm_desc& d);
bool f2g_leanw_fp32_takes(const f2g_gemm_desc& d, int split);
int f2g_launch_leanw(const f2g_gemm_desc& d, int pieces, int split, hipStream_t st);
// gemm_x6.hip: form 0 at precision 3 (checks the descriptor, picks the kernel, launches)
int f2g_gemm_x6(const f2g_gemm_desc& d, hipStream_t st);
// gemm_f16.hip: precision 4 -- decides which of the fp16x3 kernels a descriptor belongs to (h3_table there lists them:
// one entry per kernel, with what it takes), checks it, launches that one
int f2g_gemm_h3(const f2g_gemm_desc& d, hipStream_t st);
// ... and the tile height that kernel counts partial column sums in (one row per 64 output rows of whole tiles), 0
// where it has no wide epilogue or declines the descriptor (f2g_gemm_colsum_part_rows)
int f2g_gemm_h3_part_tile(const f2g_gemm_desc& d);
// gemm_f16<x>.hip, one fp16x3 kernel each: f2g_h3<x>_ok answers f2g_gemm_f16_ok for the kernel's candidates -- 1 = runs
// as handed over (the operands the kernel's images with their reciprocal scales, or fp32 under its mark), 2 = once the
// fp32 operands are replaced by those images, 0 = not for this kernel -- and f2g_launch_h3<x> launches what it accepted
int f2g_h3p_ok(const f2g_gemm_desc& d);        // form 0, stride-1 windows of 5 or 2 positions over seq images
int f2g_launch_h3p(const f2g_gemm_desc& d, hipStream_t st);
int f2g_h3p3_ok(const f2g_gemm_desc& d);       // ... stride-3 windows of 5 positions over a multiple of 128 channels
int f2g_launch_h3p3(const f2g_gemm_desc& d, hipStream_t st);
int f2g_h3p3n_ok(const f2g_gemm_desc& d);      // ... over 32 channels of the fp32 map itself (A.split = 8), N <= 128
int f2g_launch_h3p3n(const f2g_gemm_desc& d, hipStream_t st);
int f2g_h3pn_ok(const f2g_gemm_desc& d);       // ... stride-1 windows of 2 or 1 positions of the fp32 map, N <= 32
int f2g_launch_h3pn(const f2g_gemm_desc& d, hipStream_t st);
int f2g_h3pn3_ok(const f2g_gemm_desc& d);      // ... the three residues' windows of 2 positions at once, N == 96, cut and folded
int f2g_launch_h3pn3(const f2g_gemm_desc& d, hipStream_t st);
int f2g_h3wt_ok(const f2g_gemm_desc& d);       // form 2, unbounded stride-1 windows of 5 positions over column images
int f2g_launch_h3wt(const f2g_gemm_desc& d, hipStream_t st);
int f2g_h3ws_ok(const f2g_gemm_desc& d);       // ... stride-3 windows over a multiple of 128 channels
int f2g_launch_h3ws(const f2g_gemm_desc& d, hipStream_t st);
int f2g_h3wsn_ok(const f2g_gemm_desc& d);      // ... over 32 channels, both fp32 operands marked split = 8 (1 or 0)
int f2g_launch_h3wsn(const f2g_gemm_desc& d, hipStream_t st);
int f2g_launch_h3n(const f2g_gemm_desc& d, hipStream_t st);      // form 0, plain fp32 A marked split = 9 (h3_plain_ok)
int f2g_h3wn_ok(const f2g_gemm_desc& d);       // form 2, two plain fp32 matrices both marked split = 10 (1 or 0)
int f2g_launch_h3wn(const f2g_gemm_desc& d, hipStream_t st);

// ---- lab switches (product builds: both 0) ---------------------------------------------------------------------
// F2G_LABVAR (tools/micro/build_variants.sh; timing only): ablations of the bf16 lean K loop (gemm_lean.hip) --
// 1 no global loads, 2 no LDS stores, 4 no barrier, 8 no fragment reads, 16 a second accumulator set.
#ifndef F2G_LABVAR
#define F2G_LABVAR 0
#endif
// F2G_X6LAB (tools/micro/x6lab.sh; timing only): ablations of the six-product kernels --
//   1 skip the epilogue, 2 skip the read-back that writes the result's three-piece image (gemm_x6.hip),
//   4 the main-loop barrier is __syncthreads() again (every lds_barrier() below),
//   16 no split arithmetic: the pieces are raw bit fields (split3x4 below),
//   32 gemm_x6f_kernel / gemm_leanw6_kernel issue 4 of a slab's 48 MFMAs, 128 the same two without their
//   sched_group_barrier pattern,
//   256 gemm_x6f_kernel times the three intervals of its slab loop with s_memtime (wave 0 of every block; the
//   stamps' results are collected by the loop's own lgkmcnt(0) waits, nothing is added to the critical path) and adds
//   them to g_x6prof (gemm_x6.hip; f2g_lab_x6prof reads and clears them),
//   512 gemm_x6f_kernel stages without LDS stores, 1024 gemm_x6g_kernel stores inside the chain, quarter by quarter.
#ifndef F2G_X6LAB
#define F2G_X6LAB 0
#endif
#if F2G_X6LAB & 1
#define X6LAB_EPI if (acc[0][0][0] == 1.2345e30f)
#else
#define X6LAB_EPI
#endif
#if F2G_X6LAB & 2
#define X6LAB_X3 acc[0][0][1] == 1.2345e30f &&
#else
#define X6LAB_X3
#endif
#if F2G_X6LAB & 256
#define X6PROF_STAMP(t) asm volatile("s_memtime %0" : "=s"(t) : : "memory")
#define X6PROF_ACC(sum, t1, t0)                                                                              \
  {                                                                                                          \
    unsigned dt_;                                                                                            \
    asm volatile("s_sub_u32 %0, %1, %2" : "=s"(dt_) : "s"((unsigned)(t1)), "s"((unsigned)(t0)) : "memory"); \
    sum += dt_;                                                                                              \
  }
#else
#define X6PROF_STAMP(t)
#define X6PROF_ACC(sum, t1, t0)
#endif

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

constexpr int BK = 32;
constexpr int LDR = BK + 4;  // row-major LDS tile leading dim (conflict-free ds_read_b128)

inline bool host_plain(const f2g_operand& S) {
  return S.P0 == 1 && S.P1 == 1 && S.seglen >= S.cols && S.L1 == 1 && S.pad0 == 0 &&
         S.pad1 == 0 && S.L0u >= S.cols && !S.reflect && !S.lrelu_src;
}

inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// A precision-4 kernel's answer for an operand pair it otherwise accepts, given the kind of fp16 image it reads
// (f2g_operand.split): 1 = both are such images with their reciprocal scales, 2 = both are fp32, 0 = anything else
inline int f16_images_status(const f2g_operand& A, const f2g_operand& B, int split) {
  if (A.split == split && B.split == split) return A.rscale && B.rscale ? 1 : 0;
  return A.split == 0 && B.split == 0 ? 2 : 0;
}

// extent in elements of what the A operand's rows may touch, or 0 if precision 3 cannot read it
inline long long x6_a_extent(const f2g_operand& A) {
  if (host_plain(A)) return (long long)A.rows * A.cols;
  // single-segment windows that never leave their sequence (halo layouts), everything on slab boundaries
  if (A.P1 != 1 || A.L1 != 1 || A.P0 < 1 || A.seglen < A.cols || A.reflect || A.pad0 > 0 || A.rows % A.P0)
    return 0;
  const long long step = (long long)A.step0 * A.unit, off = -(long long)A.pad0 * A.unit;
  if ((step % 32) || (off % 32) || (A.seq_stride % 32) || step < 0) return 0;
  if ((long long)(A.P0 - 1) * step + off + A.cols > A.L0u) return 0;
  return (long long)(A.rows / A.P0 - 1) * A.seq_stride + A.L0u;
}

// stride-1 conv windows of TAPS positions x C channels over a halo map image (gemm_x6p_kernel, gemm_h3p_kernel)
inline bool x6_tap_ok(const f2g_gemm_desc& d, int taps) {
  const f2g_operand& A = d.A;
  if (host_plain(A) || A.P1 != 1 || A.step0 != 1 || A.unit < 32 || (A.unit % 32)) return false;
  if (A.cols != taps * A.unit || A.seglen < A.cols || (A.seq_stride % A.unit) || (A.pad0 > 0)) return false;
  const int HpIn = (int)(A.seq_stride / A.unit);
  if (A.P0 < 8 || HpIn < A.P0) return false;
  // staged positions of a tile: its rows, the taps' overhang, the extra positions of every sequence end inside
  return 128 + taps - 1 + (HpIn - A.P0) * (128 / A.P0 + 1) <= 160;
}

// stride-3 conv windows of 5 positions x C channels over a halo map image (gemm_h3p3_kernel, whose planes hold
// `plane` entries: a group's 128 rows, one entry more per sequence they touch, one for the taps' overhang).
// unit % 128 == 0: the kernel is for the MPD's 128- and 512-channel strided layers, as gemm_h3wt_kernel is for the
// 1024-channel one, and a stride-3 descriptor with fewer channels is declined, never handed to another fp16x3 kernel
inline bool x6_tap3_ok(const f2g_gemm_desc& d, int plane) {
  const f2g_operand& A = d.A;
  if (host_plain(A) || A.P1 != 1 || A.step0 != 3 || A.unit < 128 || (A.unit % 128)) return false;
  if (A.cols != 5 * A.unit || A.seglen < A.cols || (A.seq_stride % A.unit) || (A.pad0 > 0)) return false;
  if (A.P0 < 8 || A.L0u > A.seq_stride) return false;
  return 130 + 126 / A.P0 <= plane;
}

// Raises the dynamic-LDS limit of the kernels KERNS to `bytes`, the first time a launcher comes by.
template <auto... KERNS>
void dyn_lds_once(int bytes) {
  static const bool done = [bytes] {
    for (const void* k : {reinterpret_cast<const void*>(KERNS)...})
      (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    return true;
  }();
  (void)done;
}

// XCD-aware tile order: block b runs on XCD b%8; give each XCD a contiguous run of tiles with the
// n index fastest so that the tiles sharing an A panel hit the same private L2.
__device__ __forceinline__ void tile_of_block(int BM, int BN, int& m0, int& n0) {
  const int tiles_n = gridDim.y, tiles_m = gridDim.x;
  const int nblk = tiles_m * tiles_n;
  int bid = blockIdx.y * tiles_m + blockIdx.x;
  const int q = nblk >> 3, rem = nblk & 7, xcd = bid & 7, idx = bid >> 3;
  bid = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + idx;
  const int tm = bid / tiles_n, tn = bid - tm * tiles_n;
  m0 = tm * BM;
  n0 = tn * BN;
}

template <int TM, int TN>
__device__ __forceinline__ void gemm_epilogue(const f2g_epilogue& E, f32x16 (&acc)[TM][TN], int M,
                                              int N, int m0, int n0, int wm, int wn, int li,
                                              int h, bool first) {
  const float scale = E.scale != 0.f ? E.scale : 1.f;
  const float fmw = E.fm_ref ? E.fm_w * (E.fm_wdev ? E.fm_wdev[0] : 1.f) : 0.f;
  // first: split-K / stream-K -- bias and residual enter once
#pragma unroll
  for (int ni = 0; ni < TN; ++ni) {
    const int col = n0 + (wn * TN + ni) * 32 + li;
    const bool cok = col < N;
    float bias = 0.f, gam = 0.f, aln = 0.f, pslope = 0.f;
    if (cok) {
      if (E.prelu_slope) pslope = E.prelu_slope[col];
      if (E.bias && first) bias = E.bias[col];
      if (E.res && first) gam = E.gamma ? E.gamma[col] : 1.f;
      if (E.aux) aln = E.alpha_n[col];
    }
    float cs = 0.f, csa = 0.f;
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + (wm * TM + mi) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (!cok || row >= M) continue;
        float v = acc[mi][ni][e] * scale + bias;
        if (E.res && first) v += gam * E.res[(long long)row * E.ldres + col];
        if (E.aux) {
          float av = E.aux[(long long)row * E.ldaux + col];
          csa += v * fminf(av, 0.f);
          v *= (av > 0.f ? 1.f : aln);
        }
        if (E.lrelu_slope != 0.f) v = v > 0.f ? v : E.lrelu_slope * v;
        if (E.prelu_slope) {
          const float pv = v > 0.f ? v : pslope * v;
          if (E.prelu_out) E.prelu_out[(long long)row * E.ld_prelu_out + col] = pv;
          else v = pv;
        }
        long long off;
        if (E.P0o > 0) {
          int sq = row / E.P0o;
          off = (long long)sq * E.seq_stride_o + (long long)(row - sq * E.P0o) * E.row_stride_o +
                E.off_o + col;
        } else {
          off = (long long)row * E.ldc + col;
        }
        if (E.mask_src) {   // leaky-ReLU backward of the layer below (+ feature-matching term)
          const float y = E.mask_src[off];
          if (E.fm_ref) {
            const float dl = y - E.fm_ref[off];
            v += fmw * (dl > 0.f ? 1.f : (dl < 0.f ? -1.f : 0.f));
          }
          v *= y > 0.f ? 1.f : E.mask_slope;
        }
        cs += v;
        if (E.atomic) atomicAdd(E.C + off, v);
        else if (E.accumulate) E.C[off] += v;
        else E.C[off] = v;
      }
    }
    if (E.colsum || E.colsum_alpha) {
      cs += __shfl_xor(cs, 32);
      csa += __shfl_xor(csa, 32);
      if (cok && h == 0) {
        if (E.colsum) atomicAdd(E.colsum + col, cs);
        if (E.colsum_alpha) atomicAdd(E.colsum_alpha + col, csa);
      }
    }
  }
}

// Main-loop barrier of the six-product kernels: the LDS traffic of this wave is done, then the block barrier.
// __syncthreads() also waits for vmcnt(0), i.e. for the NEXT slab's global loads the wave has just issued --
// the prefetch would be drained at every slab.
__device__ __forceinline__ void lds_barrier() {
#if F2G_X6LAB & 4      // (lab build: the old barrier, for A/B runs)
  __syncthreads();
#else
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
}

// One operand of a K-major bf16 MFMA (8 consecutive k of one m / n per lane) out of planes that hold the slab as
// it lies in memory, rows 256 bytes apart: two ds_read_b64_tr_b16, each handing lane c of a 16-lane group column c
// of a 4 (k) x 16 (m) block (gemm_wgrad.hip has the layout)
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* p) {
  typedef s16x4 __attribute__((address_space(3))) * lds_p;
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(p));
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(p + 4 * 256));
  const s16x8 v = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

// three bf16 pieces of four floats (common.h: f2g_split3_pair -- 18 VALU instructions per chunk)
__device__ __forceinline__ void split3x4(const u32x4& v, u32x2& p0, u32x2& p1, u32x2& p2) {
#if F2G_X6LAB & 16
  p0 = u32x2{v.x, v.y}; p1 = u32x2{v.z, v.w}; p2 = u32x2{v.x, v.w};
  return;
#endif
  // (by value first: __builtin_bit_cast applied to a vector-element expression reads element 0)
  const unsigned u0 = v.x, u1 = v.y, u2 = v.z, u3 = v.w;
  unsigned a0, a1, a2, b0, b1, b2;
  f2g_split3_pair(__uint_as_float(u0), __uint_as_float(u1), a0, a1, a2);
  f2g_split3_pair(__uint_as_float(u2), __uint_as_float(u3), b0, b1, b2);
  p0 = u32x2{a0, b0};
  p1 = u32x2{a1, b1};
  p2 = u32x2{a2, b2};
}

}  // namespace
