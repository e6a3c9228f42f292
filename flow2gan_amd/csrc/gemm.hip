// Implicit-GEMM family on the exact-fp32 matrix cores of gfx950 (v_mfma_f32_32x32x2_f32).
//
// One kernel template serves every GEMM-shaped op of the hot path (pointwise 1x1 convs, the
// k=3 cond-encoder conv, MPD (5,1)/(3,1) convs, MRD (3,9)/(3,3) convs, DFT / inverse-DFT
// matrices for STFT/iSTFT, mel / linear filterbanks) in three forms: forward, data gradient,
// weight gradient.  Operands are described by f2g_operand (include/flow2gan_hip.h): a
// channels-last tensor viewed as rows = pixels, cols = contiguous window (never materialised).
//
// Tiling (wave64): block = WAVES_M x WAVES_N waves (2, 4 or 8, chosen per operand kind in
// dispatch_tile); each wave owns TM x TN tiles of 32x32, accumulated in f32x16 registers by
// mfma_f32_32x32x2f32.  The 2 k-slots of that instruction are fed from the
// two lane halves: lanes 0-31 walk k in [0,16) of the BK=32 slab, lanes 32-63 walk [16,32), so a
// lane's operands for 4 consecutive MFMAs are one ds_read_b128 (row-major LDS tile) or four
// conflict-free ds_read_b32 (k-major tile).  Global->register->LDS double buffering, one
// barrier per K slab.
//
// Loaders are specialised at compile time: PLAIN operands (a row-major matrix: every pointwise
// GEMM, i.e. ~95 % of the FLOPs) keep one pointer per staged chunk and add a constant per K slab;
// GENERIC operands (windowed im2col views) decode rows once before the K loop and columns once
// per slab.
//
// This file: the generic kernels (exact fp32 and split-bf16), their tile choice and split-K, and f2g_gemm's
// dispatch over the whole family.  The specialised kernels it dispatches to live beside it: gemm_lean.hip (forward
// kernel without VALU work in the K loop), gemm_wgrad.hip (K-major weight gradients), gemm_x6.hip / gemm_x6p.hip
// (fp32-class products on the bf16 pipe), narrow.hip (<= 4 output columns); gemm_common.h holds what they share.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "gemm_common.h"

namespace {

// what f2g_note_kernel recorded last
int g_last_path = 0;   // kernel family of the last dispatch (f2g_gemm_last_path)
const char* g_last_kernel = "";   // instance of the last dispatch (f2g_gemm_last_kernel): a literal of a launcher's file
int g_last_split = 1;             // with the K split of a generic launch

// ------------------------------------------------------------------------------------------
// generic (windowed) element access
// ------------------------------------------------------------------------------------------
struct RowCtx {
  long long base;
  int l1b, e0;
};

__device__ __forceinline__ RowCtx decode_row(const f2g_operand& S, int r) {
  RowCtx rc;
  int s, p1, p0;
  if (S.P0 == 1 && S.P1 == 1) {
    s = r; p1 = 0; p0 = 0;
  } else {
    int q = r / S.P0;
    p0 = r - q * S.P0;
    s = q / S.P1;
    p1 = q - s * S.P1;
  }
  rc.base = (long long)s * S.seq_stride;
  rc.l1b = p1 * S.step1 - S.pad1;
  rc.e0 = (p0 * S.step0 - S.pad0) * S.unit;
  return rc;
}

__device__ __forceinline__ float prelu1(float v, float a) { return v > 0.f ? v : a * v; }

// ------------------------------------------------------------------------------------------
// Tile loaders.  A tile is TROWS x TCOLS floats in memory orientation, staged by 256 threads as
// float4 chunks: chunk idx = tid + 256*q -> (row = idx / CH, ch = idx % CH).  CH divides 256,
// so `ch` is the same for all of a thread's chunks and rows advance by 256/CH.
//   KM = false: rows are the tile's m/n index (fixed), cols walk K   -> advance along columns
//   KM = true : rows walk K (the reduction), cols are m/n (fixed)    -> advance along rows
// MODE (chosen on the host from the operand descriptor):
//   PF  plain matrix, 16-byte aligned rows, reduction extent % BK == 0: every chunk is ONE
//       unconditional global_load_dwordx4 through a clamped pointer; masks + PReLU in store().
//   GF  windowed operand whose offsets are all multiples of 4 floats: one clamped vector load
//       per chunk + a validity bit; leaky-ReLU derivative / PReLU applied in store().
//   SL  anything else (misaligned, reflect padding, odd extents): element-wise predicated.
// store() runs after the slab's MFMAs, so the transforms never wait on the load latency.
// ------------------------------------------------------------------------------------------
enum { PF = 0, GF = 1, SL = 2, GR = 3 };  // GR = GF + reflect padding (STFT framing)

// what an out-of-window chunk of a GF operand reads (16 aligned bytes of zeros)
// (not const: the compiler must keep the address select instead of folding a select of values)
__device__ __attribute__((aligned(16))) float g_zero16[4] = {0.f, 0.f, 0.f, 0.f};


// v = hi + lo + O(2^-17 |v|): hi = round-to-nearest bf16 of v, lo = bf16 of the remainder
__device__ __forceinline__ void split_bf16(float v, unsigned short& hi, unsigned short& lo) {
  const __bf16 h = (__bf16)v;
  const __bf16 l = (__bf16)(v - (float)h);
  hi = __builtin_bit_cast(unsigned short, h);
  lo = __builtin_bit_cast(unsigned short, l);
}

template <int MODE, bool KM, int TROWS, int TCOLS, int NT = 256>
struct Loader {
  static constexpr int CH = TCOLS / 4;
  static constexpr int NCHUNK = TROWS * CH;
  static constexpr bool PARTIAL = NCHUNK < NT;  // fewer chunks than threads: the rest idle
  static constexpr int NLD = PARTIAL ? 1 : NCHUNK / NT;
  static constexpr int RSTEP = NT / CH;
  static_assert((PARTIAL || NCHUNK % NT == 0) && NT % CH == 0, "tile must divide among the threads");
  bool active;

  // Staging registers of ONE slab.  Kept out of the loader object and declared per loop iteration
  // in the kernels, so that nothing is loop-carried and the compiler can leave the loads in flight
  // across the MFMA phase.
  struct Stg {
    float4 r[NLD];
    float4 r2[MODE != PF ? NLD : 1];  // lrelu_src values of the chunk
    float4 a4;                        // PReLU slopes of the chunk's 4 columns
    unsigned vmask;                   // bit q: chunk q holds valid data
  };
  float4 a4fix;                       // KM: PReLU slopes of the thread's fixed columns
  unsigned cmask;                       // PF/KM: valid columns of the thread's fixed chunk
  unsigned rokm;                        // RM: bit q: row in range
  const float* p[MODE == PF ? NLD : 1];  // PF: chunk pointers, advanced per slab
  long long pstep;                      // PF: floats per unit of k (1 or ld)
  int kbase;                            // PF: k of the pointers p[]
  int c0;                               // first window column (RM: + k0 per slab; KM: fixed)
  int row0;                             // KM: first reduction row of this thread
  RowCtx rc[(MODE != PF && !KM) ? NLD : 1];  // generic RM: decoded rows
  long long rb[(MODE != PF && !KM) ? NLD : 1];  // generic RM: offset of the row's window origin
  int seg, o;                           // generic KM: decoded fixed column
  unsigned mg_seg, mg_p0, mg_p1;        // generic: magic numbers of seglen / P0 / P1

  __device__ __forceinline__ void init(const f2g_operand& S, int tr0, int tc0, int kbeg, int tid) {
    active = !PARTIAL || tid < NCHUNK;
    if (MODE != PF) {
      mg_seg = magic_of(S.seglen);
      mg_p0 = magic_of(S.P0);
      mg_p1 = magic_of(S.P1);
    }
    const int ch = tid % CH, rr = active ? tid / CH : 0;
    rokm = 0; cmask = 0;
    float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (MODE == PF) {
      const long long ld = S.seq_stride;
      if (!KM) {
        c0 = ch * 4;
        pstep = 1;
        kbase = kbeg;
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
          const int row = tr0 + rr + RSTEP * q;
          const bool ok = row < S.rows;
          rokm |= (ok ? 1u : 0u) << q;
          p[q] = S.base + (long long)(ok ? row : 0) * ld + ch * 4 + kbeg;
        }
      } else {
        c0 = tc0 + ch * 4;
        row0 = rr;
        pstep = ld;
        kbase = kbeg;
#pragma unroll
        for (int j = 0; j < 4; ++j) cmask |= (c0 + j < S.cols ? 1u : 0u) << j;
#pragma unroll
        for (int q = 0; q < NLD; ++q)
          p[q] = S.base + (long long)(kbeg + rr * NLD + q) * ld + (cmask ? c0 : 0);
        if (S.alpha) {
          if (cmask & 1) a4.x = S.alpha[c0];
          if (cmask & 2) a4.y = S.alpha[c0 + 1];
          if (cmask & 4) a4.z = S.alpha[c0 + 2];
          if (cmask & 8) a4.w = S.alpha[c0 + 3];
        }
      }
    } else {
      if (!KM) {
        c0 = ch * 4;
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
          const int row = tr0 + rr + RSTEP * q;
          const bool ok = row < S.rows;
          rokm |= (ok ? 1u : 0u) << q;
          rc[q] = decode_row(S, ok ? row : 0);
          rb[q] = rc[q].base + (long long)rc[q].l1b * S.line_stride + rc[q].e0;
        }
      } else {
        c0 = tc0 + ch * 4;
        row0 = rr;
        seg = 0; o = c0;
        if (S.seglen < S.cols) { seg = c0 / S.seglen; o = c0 - seg * S.seglen; }
        if (MODE != PF && S.alpha) {
          if (c0 < S.cols) a4.x = S.alpha[c0];
          if (c0 + 1 < S.cols) a4.y = S.alpha[c0 + 1];
          if (c0 + 2 < S.cols) a4.z = S.alpha[c0 + 2];
          if (c0 + 3 < S.cols) a4.w = S.alpha[c0 + 3];
        }
      }
    }
    a4fix = a4;
  }

  __device__ __forceinline__ void gchunk(const f2g_operand& S, Stg& g, int q, bool rowok,
                                         const RowCtx& rcx, int c, int sg, int oo) {
    if (MODE == GF || MODE == GR) {
      // out-of-window chunks are read from a 16-byte block of zeros: nothing to mask afterwards
      // (off = offset of the chunk relative to S.base, precombined by the caller)
      const int l1 = rcx.l1b + sg, e = rcx.e0 + oo;
      const bool v = rowok && c < S.cols && (unsigned)l1 < (unsigned)S.L1 && e >= 0 &&
                     e + 3 < S.L0u;
      const long long off = rcx.base;
      g.r[q] = *reinterpret_cast<const float4*>(v ? S.base + off : g_zero16);
      if (S.lrelu_src)
        g.r2[q] = *reinterpret_cast<const float4*>(v ? S.lrelu_src + off : g_zero16);
      if (MODE == GR) {
        // STFT framing (center=True, reflect): only the chunks that straddle an end of the
        // sequence -- the first / last two frames -- take this element-wise mirrored path
        const bool inwin = rowok && c < S.cols && (unsigned)l1 < (unsigned)S.L1;
        if (inwin && !v) {
          const long long rowb = off - e;
          float t[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            int ee = e + k;
            ee = ee < 0 ? -ee : ee;
            ee = ee >= S.L0u ? 2 * (S.L0u - 1) - ee : ee;
            const bool ok = (unsigned)ee < (unsigned)S.L0u;
            t[k] = ok ? S.base[rowb + (ok ? ee : 0)] : 0.f;
          }
          g.r[q] = make_float4(t[0], t[1], t[2], t[3]);
        }
      }
    } else {
      // SL: the same clamped-address scheme element by element (4 unconditional scalar loads, no
      // divergent branches); handles reflect padding, odd segment lengths and misaligned rows.
      const int seglen = S.seglen < S.cols ? S.seglen : S.cols;
      float vv[4], lv[4];
      int sg_e = sg, oo_e = oo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int l1 = rcx.l1b + sg_e;
        int off_e = rcx.e0 + oo_e;
        bool ok = rowok && (c + e) < S.cols && (unsigned)l1 < (unsigned)S.L1;
        if (S.reflect) {
          off_e = off_e < 0 ? -off_e : off_e;
          off_e = off_e >= S.L0u ? 2 * (S.L0u - 1) - off_e : off_e;
        }
        ok = ok && (unsigned)off_e < (unsigned)S.L0u;
        const long long a = ok ? rcx.base + (long long)l1 * S.line_stride + off_e : 0;
        const float x = S.base[a];
        lv[e] = S.lrelu_src ? S.lrelu_src[a] : 1.f;
        vv[e] = ok ? x : 0.f;
        ++oo_e;
        const bool wrap = oo_e >= seglen;
        oo_e = wrap ? 0 : oo_e;
        sg_e += wrap ? 1 : 0;
      }
      g.r[q] = make_float4(vv[0], vv[1], vv[2], vv[3]);
      g.r2[q] = make_float4(lv[0], lv[1], lv[2], lv[3]);
      g.vmask |= 1u << q;
    }
  }

  __device__ __forceinline__ void load(const f2g_operand& S, int k0, Stg& g) {
    g.a4 = a4fix;
    if (MODE == PF) {
      if (!KM) {
        // PReLU slopes of this slab's columns (full slabs only: c+3 < cols); unconditional load
        // through a valid dummy address keeps it off the control-flow / waitcnt path
        const float* ap = S.alpha ? S.alpha + (c0 + k0) : S.base;
        g.a4 = *reinterpret_cast<const float4*>(ap);
      }
      // explicit slab offset (no running pointers): the kernels issue the load unconditionally
      // with a clamped slab index, which keeps the loaded registers out of any control flow
      const long long adv = (long long)(k0 - kbase) * pstep;
#pragma unroll
      for (int q = 0; q < NLD; ++q) g.r[q] = *reinterpret_cast<const float4*>(p[q] + adv);
      g.vmask = KM ? (cmask ? ~0u : 0u) : rokm;
    } else {
      g.vmask = 0;
      if (!KM) {
        const int c = c0 + k0;
        int sg = 0, oo = c;
        if (S.seglen < S.cols) { sg = fast_div(c, S.seglen, mg_seg); oo = c - sg * S.seglen; }
        if (MODE != PF && S.alpha) {
          g.a4.x = c < S.cols ? S.alpha[c] : 0.f;
          g.a4.y = c + 1 < S.cols ? S.alpha[c + 1] : 0.f;
          g.a4.z = c + 2 < S.cols ? S.alpha[c + 2] : 0.f;
          g.a4.w = c + 3 < S.cols ? S.alpha[c + 3] : 0.f;
        }
        const int so = sg * (int)S.line_stride + oo;  // the slab's offset inside a row's window
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
          RowCtx rx = rc[q];
          if (MODE == GF || MODE == GR) rx.base = rb[q] + so;
          gchunk(S, g, q, (rokm >> q) & 1, rx, c, sg, oo);
        }
      } else {
        // the thread's NLD rows are consecutive pixels: decode the first (two divisions), then
        // step (p0, p1, s) with carries
        const int rfirst = k0 + row0 * NLD;
        int s_, p1_, p0_;
        {
          const int r = rfirst < S.rows ? rfirst : 0;
          if (S.P0 == 1 && S.P1 == 1) { s_ = r; p1_ = 0; p0_ = 0; }
          else {
            const int qq = fast_div(r, S.P0, mg_p0);
            p0_ = r - qq * S.P0;
            s_ = fast_div(qq, S.P1, mg_p1);
            p1_ = qq - s_ * S.P1;
          }
        }
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
          const bool ok = rfirst + q < S.rows;
          RowCtx rcx;
          rcx.base = (long long)s_ * S.seq_stride;
          rcx.l1b = p1_ * S.step1 - S.pad1;
          rcx.e0 = (p0_ * S.step0 - S.pad0) * S.unit;
          if (MODE == GF || MODE == GR)
            rcx.base += (long long)(rcx.l1b + seg) * S.line_stride + (rcx.e0 + o);
          gchunk(S, g, q, ok, rcx, c0, seg, o);
          ++p0_;
          const bool c0w = p0_ >= S.P0;
          p0_ = c0w ? 0 : p0_;
          p1_ += c0w ? 1 : 0;
          const bool c1w = p1_ >= S.P1;
          p1_ = c1w ? 0 : p1_;
          s_ += c1w ? 1 : 0;
        }
      }
    }
  }

  // masks + on-load transforms of chunk q (runs after the slab's MFMAs)
  __device__ __forceinline__ float4 finalize(const f2g_operand& S, const Stg& g, int q) const {
    float4 v = g.r[q];
    const float4 a4 = g.a4;
    if (MODE != GF && MODE != GR && !((g.vmask >> q) & 1)) v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (MODE == PF && KM) {  // column tail of the fixed chunk
      if (!(cmask & 1)) v.x = 0.f;
      if (!(cmask & 2)) v.y = 0.f;
      if (!(cmask & 4)) v.z = 0.f;
      if (!(cmask & 8)) v.w = 0.f;
    }
    if (MODE != PF && S.lrelu_src) {
      const float sl = S.lrelu_slope;
      v.x *= g.r2[q].x > 0.f ? 1.f : sl; v.y *= g.r2[q].y > 0.f ? 1.f : sl;
      v.z *= g.r2[q].z > 0.f ? 1.f : sl; v.w *= g.r2[q].w > 0.f ? 1.f : sl;
    }
    if (S.alpha) {
      v.x = prelu1(v.x, a4.x); v.y = prelu1(v.y, a4.y);
      v.z = prelu1(v.z, a4.z); v.w = prelu1(v.w, a4.w);
    }
    return v;
  }

  // fp32 LDS image in memory orientation: [tile row][tile col]
  __device__ __forceinline__ void store(const f2g_operand& S, const Stg& g, float* lds, int ld,
                                        int tid) const {
    if (PARTIAL && !active) return;
    const int ch = tid % CH, rr = tid / CH;
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
      const int row = KM ? rr * NLD + q : rr + RSTEP * q;
      *reinterpret_cast<float4*>(lds + row * ld + ch * 4) = finalize(S, g, q);
    }
  }

  // split-bf16 LDS image, always [m-or-n index][k] (64-byte rows of 32 bf16, 16-byte chunks
  // XOR-swizzled by (row>>2)&3): hi = bf16(v), lo = bf16(v - hi).  k-major tiles are transposed
  // here: a thread owns NLD consecutive k of 4 columns and packs them per column.
  __device__ __forceinline__ void store_split(const f2g_operand& S, const Stg& g, unsigned char* hi,
                                              unsigned char* lo, int tid, bool with_lo) const {
    if (PARTIAL && !active) return;
    const int ch = tid % CH, rr = tid / CH;
    if (!KM) {
#pragma unroll
      for (int q = 0; q < NLD; ++q) {
        const float4 v = finalize(S, g, q);
        const int row = rr + RSTEP * q;
        const int k4 = ch * 4;
        const int off = row * 64 + ((((k4 >> 3) ^ ((row >> 2) & 3))) << 4) + ((k4 >> 2) & 1) * 8;
        unsigned short h0, h1, h2, h3, l0, l1, l2, l3;
        split_bf16(v.x, h0, l0); split_bf16(v.y, h1, l1);
        split_bf16(v.z, h2, l2); split_bf16(v.w, h3, l3);
        *reinterpret_cast<uint2*>(hi + off) = make_uint2(h0 | (h1 << 16), h2 | (h3 << 16));
        if (with_lo)
          *reinterpret_cast<uint2*>(lo + off) = make_uint2(l0 | (l1 << 16), l2 | (l3 << 16));
      }
    } else {
      unsigned short hs[4][NLD], ls[4][NLD];
#pragma unroll
      for (int q = 0; q < NLD; ++q) {
        const float4 v = finalize(S, g, q);
        split_bf16(v.x, hs[0][q], ls[0][q]); split_bf16(v.y, hs[1][q], ls[1][q]);
        split_bf16(v.z, hs[2][q], ls[2][q]); split_bf16(v.w, hs[3][q], ls[3][q]);
      }
      const int k0 = rr * NLD;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int row = ch * 4 + c;
        const int off = row * 64 + ((((k0 >> 3) ^ ((row >> 2) & 3))) << 4) + (k0 & 7) * 2;
        if (NLD == 1) {
          *reinterpret_cast<unsigned short*>(hi + off) = hs[c][0];
          if (with_lo) *reinterpret_cast<unsigned short*>(lo + off) = ls[c][0];
        } else {
#pragma unroll
          for (int q = 0; q < NLD; q += 2) {
            *reinterpret_cast<unsigned*>(hi + off + q * 2) = hs[c][q] | (hs[c][q + 1 < NLD ? q + 1 : q] << 16);
            if (with_lo)
              *reinterpret_cast<unsigned*>(lo + off + q * 2) = ls[c][q] | (ls[c][q + 1 < NLD ? q + 1 : q] << 16);
          }
        }
      }
    }
  }
};

// ---- exact fp32: v_mfma_f32_32x32x2_f32 --------------------------------------------------
template <int WAVES_M, int WAVES_N, int TM, int TN, bool AKM, bool BKM, int AMODE, int BMODE>
__global__ __launch_bounds__(WAVES_M * WAVES_N * 64, 2)
void gemm_kernel(const f2g_gemm_desc d, int M, int N, int K, int kchunk) {
  constexpr int NT = WAVES_M * WAVES_N * 64;
  constexpr int BM = WAVES_M * TM * 32;
  constexpr int BN = WAVES_N * TN * 32;
  constexpr int LDA = AKM ? BM : LDR;
  constexpr int LDB = BKM ? BN : LDR;
  constexpr int ASZ = AKM ? BK * BM : BM * LDR;
  constexpr int BSZ = BKM ? BK * BN : BN * LDR;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;            // 2 buffers
  float* Bs = smem + 2 * ASZ;  // 2 buffers

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave - wm * WAVES_N;
  const int li = lane & 31, h = lane >> 5;
  int m0, n0;
  tile_of_block(BM, BN, m0, n0);
  const int kbeg = blockIdx.z * kchunk;
  int kend = kbeg + kchunk;
  if (kend > K) kend = K;
  const int nt = (kend - kbeg + BK - 1) / BK;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  using SA = typename std::conditional<AKM, Loader<AMODE, true, BK, BM, NT>,
                                       Loader<AMODE, false, BM, BK, NT>>::type;
  using SB = typename std::conditional<BKM, Loader<BMODE, true, BK, BN, NT>,
                                       Loader<BMODE, false, BN, BK, NT>>::type;
  SA sa;
  SB sb;
  if (AKM) sa.init(d.A, 0, m0, kbeg, tid); else sa.init(d.A, m0, 0, kbeg, tid);
  if (BKM) sb.init(d.B, 0, n0, kbeg, tid); else sb.init(d.B, n0, 0, kbeg, tid);

  if (nt > 0) {
    typename SA::Stg ga;
    typename SB::Stg gb;
    sa.load(d.A, kbeg, ga);
    sb.load(d.B, kbeg, gb);
    sa.store(d.A, ga, As, LDA, tid);
    sb.store(d.B, gb, Bs, LDB, tid);
  }
  __syncthreads();

  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    typename SA::Stg ga;
    typename SB::Stg gb;
    {  // unconditional prefetch of the next slab (the last iteration re-reads slab 0, unused)
      const int kn = (t + 1 < nt) ? kbeg + (t + 1) * BK : kbeg;
      sa.load(d.A, kn, ga);
      sb.load(d.B, kn, gb);
    }
    __builtin_amdgcn_sched_barrier(0);
    const float* Ab = As + cur * ASZ;
    const float* Bb = Bs + cur * BSZ;
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      float a[TM][4], b[TN][4];
      const int kk = h * 16 + s4 * 4;
#pragma unroll
      for (int mi = 0; mi < TM; ++mi) {
        const int row = (wm * TM + mi) * 32 + li;
        if (AKM) {
#pragma unroll
          for (int q = 0; q < 4; ++q) a[mi][q] = Ab[(kk + q) * LDA + row];
        } else {
          float4 tv = *reinterpret_cast<const float4*>(Ab + row * LDA + kk);
          a[mi][0] = tv.x; a[mi][1] = tv.y; a[mi][2] = tv.z; a[mi][3] = tv.w;
        }
      }
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) {
        const int col = (wn * TN + ni) * 32 + li;
        if (BKM) {
#pragma unroll
          for (int q = 0; q < 4; ++q) b[ni][q] = Bb[(kk + q) * LDB + col];
        } else {
          float4 tv = *reinterpret_cast<const float4*>(Bb + col * LDB + kk);
          b[ni][0] = tv.x; b[ni][1] = tv.y; b[ni][2] = tv.z; b[ni][3] = tv.w;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
          for (int ni = 0; ni < TN; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi][q], b[ni][q], acc[mi][ni],
                                                                0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nt) {
      sa.store(d.A, ga, As + (cur ^ 1) * ASZ, LDA, tid);
      sb.store(d.B, gb, Bs + (cur ^ 1) * BSZ, LDB, tid);
    }
    __syncthreads();
  }
  gemm_epilogue<TM, TN>(d.E, acc, M, N, m0, n0, wm, wn, li, h, blockIdx.z == 0);
}

// ---- split-bf16 ("bf16x3"): each fp32 operand is staged as hi + lo bf16 and every product is
// hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation: relative error per
// product <= ~2^-16 (vs 2^-24 exact fp32, 2^-9 plain bf16) at 3/16 of the fp32-MFMA cycle cost.
// The MFMA phase of a slab is ~5x shorter than in the fp32 kernel, so latency is hidden with
// thread-level parallelism instead: 8 waves per block (wave tile 64x32 / 32x32, <=128 VGPRs),
// two blocks per CU = 4 waves per SIMD.
template <int WAVES_M, int WAVES_N, int TM, int TN, bool AKM, bool BKM, int AMODE, int BMODE>
__global__ __launch_bounds__(WAVES_M * WAVES_N * 64, WAVES_M * WAVES_N / 2)
void gemm_kernel_b3(const f2g_gemm_desc d, int M, int N, int K, int kchunk) {
  constexpr int NT = WAVES_M * WAVES_N * 64;
  constexpr int BM = WAVES_M * TM * 32;
  constexpr int BN = WAVES_N * TN * 32;
  constexpr int ASZ = BM * 64;  // bytes of one bf16 image (hi or lo)
  constexpr int BSZ = BN * 64;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  unsigned char* base = reinterpret_cast<unsigned char*>(smem);
  constexpr int BUF = 2 * ASZ + 2 * BSZ;  // per buffer: [A_hi | A_lo | B_hi | B_lo]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave - wm * WAVES_N;
  const int li = lane & 31, h = lane >> 5;
  int m0, n0;
  tile_of_block(BM, BN, m0, n0);
  const int kbeg = blockIdx.z * kchunk;
  int kend = kbeg + kchunk;
  if (kend > K) kend = K;
  const int nt = (kend - kbeg + BK - 1) / BK;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  using SA = typename std::conditional<AKM, Loader<AMODE, true, BK, BM, NT>,
                                       Loader<AMODE, false, BM, BK, NT>>::type;
  using SB = typename std::conditional<BKM, Loader<BMODE, true, BK, BN, NT>,
                                       Loader<BMODE, false, BN, BK, NT>>::type;
  SA sa;
  SB sb;
  if (AKM) sa.init(d.A, 0, m0, kbeg, tid); else sa.init(d.A, m0, 0, kbeg, tid);
  if (BKM) sb.init(d.B, 0, n0, kbeg, tid); else sb.init(d.B, n0, 0, kbeg, tid);

  // precision 1: hi/lo split, three MFMAs per product (fp32-class accuracy);
  // precision 2: hi only, one MFMA per product = plain bf16 inputs with fp32 accumulation
  const bool hl = d.precision == 1;
  auto compute = [&](const unsigned char* Ah) {
    const unsigned char* Al = Ah + ASZ;
    const unsigned char* Bh = Ah + 2 * ASZ;
    const unsigned char* Bl = Bh + BSZ;
    // per 16-k step: its fragments (one lgkmcnt wait), then the MFMAs back to back with the
    // accumulators interleaved so that consecutive MFMAs never depend on each other
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
      const int c = ks * 2 + h;
#pragma unroll
      for (int mi = 0; mi < TM; ++mi) {
        const int row = (wm * TM + mi) * 32 + li;
        const int off = row * 64 + ((c ^ ((row >> 2) & 3)) << 4);
        ah[mi] = *reinterpret_cast<const bf16x8*>(Ah + off);
        if (hl) al[mi] = *reinterpret_cast<const bf16x8*>(Al + off);
      }
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) {
        const int row = (wn * TN + ni) * 32 + li;
        const int off = row * 64 + ((c ^ ((row >> 2) & 3)) << 4);
        bh[ni] = *reinterpret_cast<const bf16x8*>(Bh + off);
        if (hl) bl[ni] = *reinterpret_cast<const bf16x8*>(Bl + off);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int term = 0; term < 3; ++term) {
        if (term < 2 && !hl) continue;
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
          for (int ni = 0; ni < TN; ++ni) {
            const bf16x8 av = term == 0 ? al[mi] : ah[mi];
            const bf16x8 bv = term == 1 ? bl[ni] : bh[ni];
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[mi][ni], 0, 0, 0);
          }
      }
      __builtin_amdgcn_s_setprio(0);
    }
  };
  // clamped slab origin: loads are always issued (never inside control flow); out-of-range slabs
  // re-read slab 0 and are discarded
  auto kof = [&](int t) { return t < nt ? kbeg + t * BK : kbeg; };

  // Software pipeline, prefetch distance 1 (global -> registers during the MFMA phase, converted
  // into the other LDS buffer afterwards); latency is covered by 4 waves per SIMD.
  unsigned char* bufs[2] = {base, base + BUF};
  {
    typename SA::Stg ga;
    typename SB::Stg gb;
    sa.load(d.A, kof(0), ga);
    sb.load(d.B, kof(0), gb);
    if (nt > 0) {
      sa.store_split(d.A, ga, bufs[0], bufs[0] + ASZ, tid, hl);
      sb.store_split(d.B, gb, bufs[0] + 2 * ASZ, bufs[0] + 2 * ASZ + BSZ, tid, hl);
    }
  }
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    typename SA::Stg ga;
    typename SB::Stg gb;
    sa.load(d.A, kof(t + 1), ga);
    sb.load(d.B, kof(t + 1), gb);
    __builtin_amdgcn_sched_barrier(0);
    compute(bufs[cur]);
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nt) {
      unsigned char* nb = bufs[cur ^ 1];
      sa.store_split(d.A, ga, nb, nb + ASZ, tid, hl);
      sb.store_split(d.B, gb, nb + 2 * ASZ, nb + 2 * ASZ + BSZ, tid, hl);
    }
    __syncthreads();
  }
  gemm_epilogue<TM, TN>(d.E, acc, M, N, m0, n0, wm, wn, li, h, blockIdx.z == 0);
}

template <int WAVES_M, int WAVES_N, int TM, int TN, bool AKM, bool BKM, int AMODE, int BMODE,
          bool B3 = false>
int launch(const f2g_gemm_desc& d, int M, int N, int K, int split, hipStream_t st) {
  constexpr int BM = WAVES_M * TM * 32;
  constexpr int BN = WAVES_N * TN * 32;
  constexpr int ASZ = AKM ? BK * BM : BM * LDR;
  constexpr int BSZ = BKM ? BK * BN : BN * LDR;
  constexpr size_t smem = B3 ? (size_t)2 * (2 * BM * 64 + 2 * BN * 64)
                             : (size_t)2 * (ASZ + BSZ) * sizeof(float);
  int kchunk = ((K + split - 1) / split + BK - 1) / BK * BK;
  if (kchunk < BK) kchunk = BK;
  int zs = (K + kchunk - 1) / kchunk;
  if (zs < 1) zs = 1;
  dim3 grid((M + BM - 1) / BM, (N + BN - 1) / BN, zs);
  if (grid.x == 0 || grid.y == 0) return F2G_OK;
  if constexpr (B3) {
    constexpr auto kern = gemm_kernel_b3<WAVES_M, WAVES_N, TM, TN, AKM, BKM, AMODE, BMODE>;
    dyn_lds_once<kern>((int)smem);
    hipLaunchKernelGGL(kern, grid, dim3(WAVES_M * WAVES_N * 64), smem, st, d, M, N, K, kchunk);
  } else {
    constexpr auto kern = gemm_kernel<WAVES_M, WAVES_N, TM, TN, AKM, BKM, AMODE, BMODE>;
    dyn_lds_once<kern>((int)smem);
    hipLaunchKernelGGL(kern, grid, dim3(WAVES_M * WAVES_N * 64), smem, st, d, M, N, K, kchunk);
  }
  return f2g_check_launch();
}

// name of a generic route (f2g_gemm_last_kernel): form (F0 forward, F1 data gradient, F2 weight gradient) and
// the loader modes of A and B
template <bool AKM, bool BKM, int AMODE, int BMODE>
const char* generic_name() {
  if (AKM) {
    if (AMODE == PF && BMODE == PF) return "generic<F2,PF,PF>";
    if (AMODE == PF && BMODE == GF) return "generic<F2,PF,GF>";
    if (AMODE == GF && BMODE == GF) return "generic<F2,GF,GF>";
    return "generic<F2,SL,SL>";
  }
  if (BKM) {
    if (AMODE == PF) return "generic<F1,PF,PF>";
    if (AMODE == GF) return "generic<F1,GF,PF>";
    return "generic<F1,SL,SL>";
  }
  if (AMODE == PF) return "generic<F0,PF,PF>";
  if (AMODE == GF) return "generic<F0,GF,PF>";
  if (AMODE == GR) return "generic<F0,GR,PF>";
  return "generic<F0,SL,SL>";
}

template <bool AKM, bool BKM, int AMODE, int BMODE>
int dispatch_tile(const f2g_gemm_desc& d, int M, int N, int K, int split, hipStream_t st) {
  f2g_note_kernel(generic_name<AKM, BKM, AMODE, BMODE>(), split, 0);
  // split-bf16 core: fast loader modes only; SL operands (small GEMMs) stay on exact fp32
  // (the reflect-padded STFT framing stays exact: small spectral bins are differences of large
  // terms, and the log-mel / spectral losses take their logarithm)
  if ((d.precision == 1 || d.precision == 2) && !d.A.reflect && !d.B.reflect) {
    if (AKM && M <= 32)
      return launch<1, 8, 1, 1, AKM, BKM, AMODE, BMODE, true>(d, M, N, K, split, st);  // 32 x 256
    if (N <= 32) return launch<8, 1, 1, 1, AKM, BKM, AMODE, BMODE, true>(d, M, N, K, split, st);
    if (N <= 64) return launch<4, 2, 1, 1, AKM, BKM, AMODE, BMODE, true>(d, M, N, K, split, st);
    // deep-K, wide-N problems (the 1024-channel MPD layers): 4 waves with 64x64 wave tiles read
    // less LDS per FLOP; everything else hides latency better with 8 waves of 64x32
    if (K >= 2048 && N >= 512)
      return launch<2, 2, 2, 2, AKM, BKM, AMODE, BMODE, true>(d, M, N, K, split, st);
    return launch<2, 4, 2, 1, AKM, BKM, AMODE, BMODE, true>(d, M, N, K, split, st);  // 128 x 128
  }
  // 32 x 256 for the weight gradients of 32-channel convs: 8 waves of one 32x32 tile each
  // (51 -> 57 TFLOP/s on the MRD band layers vs 4 waves of 32x64)
  if (AKM && M <= 32 && N <= 64)  // first MRD layer (2 -> 32 channels, 54 taps): 32 x 64, 2 waves
    return launch<1, 2, 1, 1, AKM, BKM, AMODE, BMODE>(d, M, N, K, split, st);
  if (AKM && M <= 32) return launch<1, 8, 1, 1, AKM, BKM, AMODE, BMODE>(d, M, N, K, split, st);
  // 128 x 32 (46 KB of LDS -> 3 blocks per CU); a 256 x 32 tile needs 83 KB and leaves ONE block
  // = one wave per SIMD on the CU, which cannot hide anything (measured 50 TFLOP/s on the
  // 32-channel MRD convs)
  if (N <= 32) return launch<4, 1, 1, 1, AKM, BKM, AMODE, BMODE>(d, M, N, K, split, st);
  if (N <= 64) return launch<4, 1, 1, 2, AKM, BKM, AMODE, BMODE>(d, M, N, K, split, st);
  // 128 x 128.  k-major LDS tiles (data / weight gradients) are read with four ds_read_b32 per
  // fragment instead of one ds_read_b128: 8 waves of 32x64 (4 waves per SIMD) hide that latency
  // (measured +5..20 % on every dgrad / wgrad shape); row-major forward tiles are best with 4
  // waves of 64x64 (least LDS traffic per MFMA).
  // (windowed forward operands -- the MPD convs -- spend VALU on im2col addressing: 8 waves too)
  if (AKM || BKM || AMODE == GF || AMODE == GR)
    return launch<4, 2, 1, 2, AKM, BKM, AMODE, BMODE>(d, M, N, K, split, st);
  return launch<2, 2, 2, 2, AKM, BKM, AMODE, BMODE>(d, M, N, K, split, st);
}

// ---- split-K for forward / data-gradient GEMMs ------------------------------------------------
// A 128x128 tiling of e.g. pwconv2 (M=6016, N=768) yields 282 blocks for 256 CUs: 26 CUs carry two
// tiles, the other 230 idle for half the kernel.  With a linear epilogue the reduction can be cut
// into s chunks whose partial tiles are added atomically onto a zeroed output (bias / residual
// enter through chunk 0): s*tiles blocks fill the last wave of resident blocks.
__global__ __launch_bounds__(256) void zero_out_kernel(const f2g_epilogue E, int M, int N) {
  const long long total = (long long)M * N;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total;
       i += (long long)gridDim.x * 256) {
    const int row = (int)(i / N), col = (int)(i - (long long)row * N);
    long long off;
    if (E.P0o > 0) {
      const int sq = row / E.P0o;
      off = (long long)sq * E.seq_stride_o + (long long)(row - sq * E.P0o) * E.row_stride_o +
            E.off_o + col;
    } else {
      off = (long long)row * E.ldc + col;
    }
    E.C[off] = 0.f;
  }
}

inline int auto_split(int M, int N, int K) {
  if (N <= 64) return 1;  // narrow tiles: thousands of blocks already
  // Measured (tools/splitk_sweep.py): splitting pays only for deep reductions (>= 64 slabs, each
  // chunk >= 20 slabs) and only through the fill of the last wave of 512 resident blocks:
  // 282 tiles x K 2304: s=3 +31 %; 1192 x 5120: s=3 +19 %; 188 x 6144: s=8 +22 %; every
  // shallower shape loses to the atomic epilogue.
  const long long tiles = (long long)((M + 127) / 128) * ((N + 127) / 128);
  const int nk = (K + BK - 1) / BK;
  // latency regime (batch-1 streaming synthesis, the per-item time MLPs): fewer tiles than half
  // the CUs -- every block is alone on its CU and the kernel lasts one block's K loop; cutting
  // that loop into <= 8 chunks of >= 8 slabs shortens it proportionally (chunked synthesis at
  // batch 1: 17.2 -> 12.1 ms per 1 s chunk, 9.1 ms replayed from a HIP graph)
  if (tiles * 2 <= 256 && nk >= 16) {
    int s = nk / 8;
    if (s > 8) s = 8;
    if ((long long)s * tiles > 256) s = (int)(256 / tiles);
    return s >= 2 ? s : 1;
  }
  if (nk < 64) return 1;
  auto eff = [&](int s) {
    const double w = (double)(tiles * s) / 512.0;
    return w / (double)((tiles * s + 511) / 512);
  };
  const double e1 = eff(1);
  double best = e1 + 0.15;
  int best_s = 1;
  for (int s = 2; s <= 8; ++s) {
    if (nk / s < 20) break;
    const double e = eff(s);
    if (e > best + 0.02) {
      best = e;
      best_s = s;
    }
  }
  return best_s;
}

// Loader mode of an operand; `red_is_cols`: the reduction runs along the operand's columns.
inline int op_mode(const f2g_operand& S, bool red_is_cols) {
  if (host_plain(S)) {
    const int red = red_is_cols ? S.cols : S.rows;
    const bool ok = al16(S.base) && (S.seq_stride & 3) == 0 && S.cols >= 4 && red % BK == 0 &&
                    (!S.alpha || !red_is_cols || al16(S.alpha));
    if (ok) return PF;
  }
  const long long eu0 = (long long)S.step0 * S.unit, ep0 = (long long)S.pad0 * S.unit;
  const bool vec = al16(S.base) && (S.seq_stride & 3) == 0 && (S.line_stride & 3) == 0 &&
                   (S.seglen & 3) == 0 && (eu0 & 3) == 0 && (ep0 & 3) == 0 && (S.L0u & 3) == 0 &&
                   (S.cols & 3) == 0 && (!S.reflect || !S.lrelu_src) &&
                   (!S.lrelu_src || al16(S.lrelu_src)) && S.L0u >= 4;
  if (vec && S.reflect) return red_is_cols ? GR : SL;  // instantiated for forward A operands only
  return vec ? GF : SL;
}

}  // namespace

// Which kernel family the last f2g_gemm call of this process dispatched to (diagnostics for the
// benchmark's per-kernel roofline; not thread safe): 0 generic MFMA kernels, 1 lean kernel,
// 2 lean kernel in stream-K mode, 3 narrow (VALU) kernels, 4 the precision-3 kernels, 5 their 32-column instance.
extern "C" int f2g_gemm_last_path(void) { return g_last_path; }

void f2g_note_kernel(const char* name, int split, int path) {
  g_last_kernel = name;
  g_last_split = split;
  g_last_path = path;
}

extern "C" const char* f2g_gemm_last_kernel(void) {
  static char buf[64];
  if (g_last_split > 1 && strncmp(g_last_kernel, "generic<", 8) == 0)
    snprintf(buf, sizeof(buf), "%s split=%d", g_last_kernel, g_last_split);
  else
    snprintf(buf, sizeof(buf), "%s", g_last_kernel);
  return buf;
}

// dst = split-bf16 image of src (n4 groups of four floats, both 16-byte aligned): group g becomes
// [hi(x0) hi(x1) hi(x2) hi(x3) | lo(x0) lo(x1) lo(x2) lo(x3)], hi = bf16(x) (round to nearest even),
// lo = bf16(x - hi): the same 16 bytes at the same address, so every operand descriptor (windows,
// halo rows, strides -- all multiples of four floats on the lean path) addresses it unchanged.
__global__ __launch_bounds__(256) void split_bf16_kernel(uint4* __restrict__ dst,
                                                         const float4* __restrict__ src, long long n4) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const float4 v = src[i];
    unsigned short h0, h1, h2, h3, l0, l1, l2, l3;
    split_bf16(v.x, h0, l0);
    split_bf16(v.y, h1, l1);
    split_bf16(v.z, h2, l2);
    split_bf16(v.w, h3, l3);
    dst[i] = make_uint4(h0 | ((unsigned)h1 << 16), h2 | ((unsigned)h3 << 16), l0 | ((unsigned)l1 << 16),
                        l2 | ((unsigned)l3 << 16));
  }
}

// dst (bf16, n elements) = round-to-nearest-even of src: the TRUE bf16 image of a tensor (same shape,
// strides in elements) for the plain-bf16 lean instances
__global__ __launch_bounds__(256) void to_bf16_kernel(uint2* __restrict__ dst, const float4* __restrict__ src,
                                                      long long n4) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const float4 v = src[i];
    unsigned short h0, h1, h2, h3, l;
    split_bf16(v.x, h0, l);
    split_bf16(v.y, h1, l);
    split_bf16(v.z, h2, l);
    split_bf16(v.w, h3, l);
    dst[i] = make_uint2(h0 | ((unsigned)h1 << 16), h2 | ((unsigned)h3 << 16));
  }
}

extern "C" int f2g_to_bf16(void* dst, const float* src, int64_t n, f2g_stream_t stream) {
  if (!dst || !src || (n & 3) || (((uintptr_t)dst) & 7) || !al16(src)) return F2G_EINVAL;
  if (n == 0) return F2G_OK;
  const long long n4 = n / 4;
  long long blocks = (n4 + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(to_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<uint2*>(dst), reinterpret_cast<const float4*>(src), n4);
  return f2g_check_launch();
}

extern "C" int f2g_split_bf16(float* dst, const float* src, int64_t n, f2g_stream_t stream) {
  if (!dst || !src || (n & 3) || !al16(dst) || !al16(src)) return F2G_EINVAL;
  if (n == 0) return F2G_OK;
  const long long n4 = n / 4;
  long long blocks = (n4 + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(split_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<uint4*>(dst), reinterpret_cast<const float4*>(src), n4);
  return f2g_check_launch();
}

extern "C" int f2g_gemm(const f2g_gemm_desc* dp, f2g_stream_t stream) {
  if (!dp || !dp->A.base || !dp->B.base || !dp->E.C) return F2G_EINVAL;
  f2g_note_kernel("", 1, g_last_path);   // (no kernel yet; the family stays until a launcher records its own)
  const f2g_gemm_desc& d = *dp;
  hipStream_t st = (hipStream_t)stream;
  int split = d.split_k > 0 ? d.split_k : 1;
  if (d.E.colsum_part_ld > 0 && f2g_gemm_colsum_part_rows(dp) == 0) {
    f2g_set_error("f2g_gemm: E.colsum_part_ld needs a launch with the wide epilogue "
                  "(f2g_gemm_colsum_part_rows(d) == 0 for this descriptor)");
    return F2G_EINVAL;
  }
  if (d.precision == 4) return f2g_gemm_h3(d, st);   // fp16x3: its own kernels or F2G_EINVAL
  if (d.E.col_fold || d.E.seq_live) {
    f2g_set_error("f2g_gemm: E.col_fold / E.seq_live belong to gemm_h3pn3_kernel (precision 4), never run elsewhere");
    return F2G_EINVAL;
  }
  if ((d.A.split >= 5 && d.A.split <= 10) || (d.B.split >= 5 && d.B.split <= 10)) {
    f2g_set_error("f2g_gemm: f2g_split_f16x2 / _cols / _seq images (split = 5 / 6 / 7) and maps or matrices scaled "
                  "inside the kernel (split = 8 / 9 / 10) belong to precision 4");
    return F2G_EINVAL;
  }
  if (d.precision == 3 && d.form == 2) {
    // fp32-class weight gradient: fp32 operands, split into three pieces inside the kernel
    if (d.A.split || d.B.split || d.A.rows != d.B.rows || !f2g_leanw_ok(d) || d.E.x3_out ||
        (split > 1 && !d.E.atomic)) {
      f2g_set_error("f2g_gemm precision 3, form 2: fp32 operands the K-major weight-gradient kernel reads");
      return F2G_EINVAL;
    }
    return f2g_launch_leanw(d, 6, split, st);
  }
  if (d.precision == 3) return f2g_gemm_x6(d, st);
  if (d.E.x3_out) {
    f2g_set_error("f2g_gemm: E.x3_out belongs to precision 3");
    return F2G_EINVAL;
  }
  {
    const int nr = f2g_gemm_narrow(d, st);  // <= 4 output columns / gradient rows: VALU kernels
    if (nr != 0) return nr < 0 ? nr : F2G_OK;
    f2g_note_kernel("", 1, 0);   // (from here on: the MFMA families)
  }
  if (d.E.prelu_slope && (d.E.atomic || d.E.accumulate || d.E.P0o > 0 || d.form == 2)) return F2G_EINVAL;
  if (d.E.mask_src && (d.E.atomic || d.E.accumulate || d.form == 2)) return F2G_EINVAL;
  if (d.form == 0 || d.form == 1) {
    const bool f1 = d.form == 1;
    if (f1 ? d.A.cols != d.B.rows : d.A.cols != d.B.cols) return F2G_EINVAL;
    if (!host_plain(d.B)) return F2G_EINVAL;
    const int M = d.A.rows, N = f1 ? d.B.cols : d.B.rows, K = d.A.cols;
    const int am = op_mode(d.A, true), bm = op_mode(d.B, !f1);
    // split_k: 1 = off, > 1 = as asked, 0 = decide here (linear epilogues only)
    // (an epilogue input that aliases the output -- in-place residual or PReLU-derivative mask --
    // would be destroyed by the zero fill)
    const bool linear = d.E.lrelu_slope == 0.f && d.E.res != d.E.C && d.E.aux != d.E.C && !d.E.prelu_slope &&
                        !d.E.mask_src;
    int s = d.split_k;
    // (STFT framing GEMMs are never split: atomics would make the spectra -- the input of every
    // discriminator and loss -- differ in the last bit from run to run)
    // option deterministic = 1 (F2G_DETERMINISTIC=1): never split on the library's own initiative (bit-reproducible forward)
    const bool no_auto = f2g_opt(F2G_OPT_DETERMINISTIC) != 0;
    // pre-split operands (f2g_split_bf16) are understood by the lean kernel's split-bf16 instances only
    const bool presplit = d.A.split != 0 && d.B.split == d.A.split;
    const bool bf16img = d.A.split == 2;
    const bool lean = !f1 && N > 64 && f2g_lean_operands_ok(d) &&
                      (d.precision == 0 || ((d.precision == 1 || d.precision == 2) && presplit)) &&
                      (!bf16img || (d.precision == 2 && f2g_lean_bf16_ok(d)));
    if ((d.A.split || d.B.split) && !(lean && d.precision != 0)) return F2G_EINVAL;
    if (d.E.c_bf16 && !lean) return F2G_EINVAL;
    if (lean && d.split_k == 0) {
      // library-chosen work split on the lean kernel: stream-K (same linear-epilogue condition as
      // split-K; option deterministic = 1 (F2G_DETERMINISTIC=1) keeps the plain tile grid)
      const int sk_mode = f2g_opt(F2G_OPT_STREAMK);
      int upb = 0;
      if (sk_mode > 0 && linear && !no_auto && !d.E.atomic && !d.E.c_bf16)
        upb = f2g_lean_stream_k(M, N, bf16img ? K / 2 : K, sk_mode > 1);   // (64-element slabs)
      if (upb > 0 && !d.E.accumulate)
        hipLaunchKernelGGL(zero_out_kernel, dim3(f2g_grid_for((int64_t)M * N, 256)), dim3(256), 0,
                           st, d.E, M, N);
      return f2g_launch_lean(d, M, N, K, 1, upb, st);
    }
    if (s == 0)
      s = (linear && am != SL && bm != SL && M > 0 && !d.A.reflect && !no_auto) ? auto_split(M, N, K)
                                                                                 : 1;
    if (s > 1 && !linear) return F2G_EINVAL;
    f2g_gemm_desc dd = d;
    if (s > 1 && !d.E.atomic) {
      if (!d.E.accumulate) {
        hipLaunchKernelGGL(zero_out_kernel, dim3(f2g_grid_for((int64_t)M * N, 256)), dim3(256), 0,
                           st, d.E, M, N);
      }
      dd.E.atomic = 1;
      dd.E.accumulate = 0;
    }
    if (!f1) {
      if (lean) return f2g_launch_lean(dd, M, N, K, s, 0, st);
      if (am == PF && bm == PF) return dispatch_tile<false, false, PF, PF>(dd, M, N, K, s, st);
      if (am == GF && bm == PF) return dispatch_tile<false, false, GF, PF>(dd, M, N, K, s, st);
      if (am == GR && bm == PF) return dispatch_tile<false, false, GR, PF>(dd, M, N, K, s, st);
      return dispatch_tile<false, false, SL, SL>(dd, M, N, K, s, st);
    }
    if (am == PF && bm == PF) return dispatch_tile<false, true, PF, PF>(dd, M, N, K, s, st);
    if (am == GF && bm == PF) return dispatch_tile<false, true, GF, PF>(dd, M, N, K, s, st);
    return dispatch_tile<false, true, SL, SL>(dd, M, N, K, s, st);
  } else if (d.form == 2) {
    if (d.A.rows != d.B.rows) return F2G_EINVAL;
    if (split > 1 && !d.E.atomic) return F2G_EINVAL;
    const int M = d.A.cols, N = d.B.cols, K = d.A.rows;
    if (d.A.split || d.B.split) {   // pre-split images: the lean weight-gradient kernel only
      if (!(d.precision == 1 && d.A.split && d.B.split && f2g_leanw_ok(d))) return F2G_EINVAL;
      return f2g_launch_leanw(d, 3, split, st);
    }
    if (f2g_leanw_fp32_takes(d, split)) return f2g_launch_leanw(d, 1, split, st);
    int am = op_mode(d.A, false), bm = op_mode(d.B, false);
    // split-K chunks are multiples of BK, so PF only needs the total extent % BK == 0
    if (am == PF && bm == PF) return dispatch_tile<true, true, PF, PF>(d, M, N, K, split, st);
    if (am == PF && bm == GF) return dispatch_tile<true, true, PF, GF>(d, M, N, K, split, st);
    if (am != SL && bm != SL) return dispatch_tile<true, true, GF, GF>(d, M, N, K, split, st);
    return dispatch_tile<true, true, SL, SL>(d, M, N, K, split, st);
  }
  return F2G_EINVAL;
}
