// cnslmat/cnsl-conv-frame.hip -- the frame-resident convolution forward for
// layers with a small kernel volume (K = kh*kw*C <= 32, e.g. the fbank input
// layer of BASELINE c2: 8x1x3 = 24), where the contraction is too thin to
// feed MFMA from an im2col tile and the layer is HBM-bound.
//
// One workgroup walks frames (grid-stride over rows); per frame
//   Y[g][p] = sum_k W[k][g] X[c][p + off_k]
// the frame's X map (5.3 KB) is staged in LDS; MFMA 32x32 with g on the
// accumulator rows and p on the lanes, bias fused.  conv_fwd_frame_kernel
// keeps W in LDS too and stores two 128-B runs of Y per accumulator;
// conv_fwd_slab_kernel stages each 32-map slab of Y in LDS and streams it
// out in 16-B stores; conv_fwd_regs_kernel holds every MFMA operand in
// registers and can run the max pool that follows on the slab.
// The frame backward is in cnsl-conv-frame-bwd.hip, the reduction of
// workgroup partials in cnsl-conv-reduce.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <stdint.h>
#include <stdlib.h>

#include "conv-frame-dev.h"
#include "conv-geom.h"
#include "f16-split.h"
#include "pool-stats-dev.h"
#include "x6-util.h"

using namespace kcnn;

namespace {

__host__ __device__ inline int align16(int bytes) { return (bytes + 15) & ~15; }

// ---------------------------------------------------------------------------
template <int NGB>
__global__ __launch_bounds__(256) void conv_fwd_frame_kernel(
    ConvGeom g, const float *__restrict__ X, int xs,
    const float *__restrict__ K, int ks, const float *__restrict__ bias,
    float *__restrict__ out, int os, int Kpad, int Gp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int2 *koff = reinterpret_cast<int2 *>(smem);
  float *Ws = reinterpret_cast<float *>(smem + align16(Kpad * 8));
  float *Xs = Ws + Kpad * Gp;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  for (int e = tid; e < Kpad * Gp; e += 256) {
    const int k = e / Gp, gg = e - k * Gp;
    Ws[e] = (k < g.Kdim && gg < g.G) ? K[(int64_t)k * ks + gg] : 0.0f;
  }
  for (int k = tid; k < Kpad; k += 256) {
    int2 v = make_int2(0, 0x7fff << 16);  // padded tap: never in bounds
    if (k < g.Kdim) {
      uint32_t c, r, kx, ky;
      g.div_khkw.divmod((uint32_t)k, c, r);
      g.div_kh.divmod(r, kx, ky);
      v = make_int2((int)c * g.HW, (int)((kx << 16) | ky));
    }
    koff[k] = v;
  }
  const int CHW = g.C * g.HW;
  const int ntile = (g.P + 31) >> 5;
  const int ksteps = Kpad >> 1;

  for (int n = blockIdx.x; n < g.R; n += gridDim.x) {
    __syncthreads();
    const float *xr = X + (int64_t)n * xs;
    for (int e = tid; e < CHW; e += 256) Xs[e] = xr[e];
    __syncthreads();
    for (int pt = wave; pt < ntile; pt += 4) {
      const int p = pt * 32 + (lane & 31);
      const bool pv = p < g.P;
      uint32_t px = 0, py = 0;
      if (pv) g.div_oh.divmod((uint32_t)p, px, py);
      for (int gs = 0; gs < Gp; gs += 32 * NGB) {  // Gp: multiple of 32*NGB
        floatx16 acc[NGB];
#pragma unroll
        for (int b = 0; b < NGB; b++) acc[b] = zero16();
        for (int s = 0; s < ksteps; s++) {
          const int k = 2 * s + (lane >> 5);
          // branch-free gather: padded taps (k >= Kdim) carry zero weights,
          // invalid positions / padding read a clamped address and are
          // zeroed by a select (no exec-masked regions around the MFMAs).
          const int2 ko = koff[k];
          const int xx = (int)px + (ko.y >> 16) - g.pad_w;
          const int yy = (int)py + (ko.y & 0xffff) - g.pad_h;
          const bool ok = pv && (unsigned)xx < (unsigned)g.W &&
                          (unsigned)yy < (unsigned)g.H;
          const float xv = Xs[ok ? ko.x + xx * g.H + yy : 0];
          const float bv = ok ? xv : 0.0f;
          const float *wrow = Ws + k * Gp + gs + (lane & 31);
#pragma unroll
          for (int b = 0; b < NGB; b++)
            acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(wrow[b * 32], bv, acc[b], 0, 0, 0);
        }
        if (pv) {
          float *orow = out + (int64_t)n * os + p;
#pragma unroll
          for (int b = 0; b < NGB; b++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
              const int gg = gs + b * 32 + mfma32_row(r, lane);
              if (gg < g.G) {
                float v = acc[b][r];
                if (bias) v = v + bias[gg];
                orow[(int64_t)gg * g.P] = v;
              }
            }
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Forward, slab-streamed: the workgroup computes one 32-map slab of a frame's
// output (32 x P, a contiguous run of Y) into LDS, then streams it to HBM as
// linear 16-byte-per-lane stores of whole lines.
__global__ __launch_bounds__(256) void conv_fwd_slab_kernel(
    ConvGeom g, const float *__restrict__ X, int xs,
    const float *__restrict__ K, int ks, const float *__restrict__ bias,
    float *__restrict__ out, int os, int Kpad, int Gp, int vec_ok) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int2 *koff = reinterpret_cast<int2 *>(smem);
  float *T = reinterpret_cast<float *>(smem + align16(Kpad * 8));   // [32][P]
  float *Ws = T + ((32 * g.P + 3) & ~3);                             // [Kpad][Gp]
  float *Xs = Ws + Kpad * Gp;                                        // [C*HW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < Kpad * Gp; e += 256) {
    const int k = e / Gp, gg = e - k * Gp;
    Ws[e] = (k < g.Kdim && gg < g.G) ? K[(int64_t)k * ks + gg] : 0.0f;
  }
  for (int k = tid; k < Kpad; k += 256) {
    int2 v = make_int2(0, 0x7fff << 16);
    if (k < g.Kdim) {
      uint32_t c, r, kx, ky;
      g.div_khkw.divmod((uint32_t)k, c, r);
      g.div_kh.divmod(r, kx, ky);
      v = make_int2((int)c * g.HW, (int)((kx << 16) | ky));
    }
    koff[k] = v;
  }
  const int CHW = g.C * g.HW;
  const int ntile = (g.P + 31) >> 5;
  const int ksteps = Kpad >> 1;
  for (int n = blockIdx.x; n < g.R; n += gridDim.x) {
    __syncthreads();
    const float *xr = X + (int64_t)n * xs;
    for (int e = tid; e < CHW; e += 256) Xs[e] = xr[e];
    __syncthreads();
    for (int gb = 0; gb < Gp; gb += 32) {
      for (int pt = wave; pt < ntile; pt += 4) {
        const int p = pt * 32 + (lane & 31);
        const bool pv = p < g.P;
        uint32_t px = 0, py = 0;
        if (pv) g.div_oh.divmod((uint32_t)p, px, py);
        floatx16 acc = zero16();
        const float *wcol = Ws + gb + (lane & 31);
        for (int s = 0; s < ksteps; s++) {
          const int k = 2 * s + (lane >> 5);
          const int2 ko = koff[k];
          const int xx = (int)px + (ko.y >> 16) - g.pad_w;
          const int yy = (int)py + (ko.y & 0xffff) - g.pad_h;
          const bool ok = pv && (unsigned)xx < (unsigned)g.W &&
                          (unsigned)yy < (unsigned)g.H;
          const float xv = Xs[ok ? ko.x + xx * g.H + yy : 0];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wcol[k * Gp], ok ? xv : 0.0f,
                                                     acc, 0, 0, 0);
        }
        if (pv) {
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int gl = mfma32_row(r, lane);
            const int gg = gb + gl;
            T[gl * g.P + p] = acc[r] + (bias && gg < g.G ? bias[gg] : 0.0f);
          }
        }
      }
      __syncthreads();
      const int rows = g.G - gb < 32 ? g.G - gb : 32;
      const int cnt = rows * g.P;
      float *dst = out + (int64_t)n * os + (int64_t)gb * g.P;
      if (vec_ok) {
        const float4 *src4 = reinterpret_cast<const float4 *>(T);
        float4 *dst4 = reinterpret_cast<float4 *>(dst);
        for (int e = tid; e < (cnt >> 2); e += 256) dst4[e] = src4[e];
        for (int e = (cnt & ~3) + tid; e < cnt; e += 256) dst[e] = T[e];
      } else {
        for (int e = tid; e < cnt; e += 256) dst[e] = T[e];
      }
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------
// Forward with every MFMA operand in registers.  Per wave: the kernel
// W[k][g] for all (up to 4) 32-filter groups is loaded once (KS*4 VGPRs); per
// frame the im2col values of the wave's position tiles are gathered once
// from the LDS-resident map (FT*KS VGPRs) and reused by every filter group,
// so the MFMA chains run with no LDS traffic.  Each 32-filter output slab
// (a contiguous 32 x P run of Y) is staged in LDS and streamed out with
// 16-B stores; bias fused.  KS = k-steps (Kdim <= 2*KS, padded taps carry
// zero weights), FT = position tiles per wave (P <= 4*32*FT).
// PC > 0 also runs the channel-only max pool that follows the convolution
// (MaxpoolComponent with pool 1 x 1 x PC, nnet-component-nnet0.cc:869-880)
// on the LDS-resident slab: pool[n][j*P + q] = max over maps PC*j .. PC*j+PC-1
// (same start value and comparison as A.8), plus the routing mask
// mask[n][j*P + q] bit c = (Y[PC*j + c][q] == pool value) that the pool's
// Backprop (A.9) would recompute from Y.
// PC == -1: a 3-D window (ph x pw x pc, runtime; pc divides 32) pooled from
// the same slab, with a 16-bit mask (bit c*pw*ph + w*ph + h); PC == -3 the
// same for the 3 x 1 x 4 window (c5's P1) fixed at compile time, so the
// window's 12 values are read once into registers.
// X6: the products on the bf16 matrix cores (x6-util.h).  KS is then the
// number of k16 steps; A = W^T split into its three bf16 planes once per
// kernel (4 groups x KS x 3 fragments in VGPRs), with the bias as row k =
// Kdim against a constant-1 row of B, so the accumulators hold conv + bias
// and no epilogue add remains; B = the gathered im2col values, split in
// registers once per frame and tile.  Unpadded maps only (host check).
// F16 (AR = 2): the products on the f16 matrix cores (f16-split.h), three
// per k16 step.  A = W^T scaled by 2^sa (one exponent for the whole kernel,
// from the wave's max |W|: every wave holds all of W), split once per kernel
// into hi / lo planes; B = the gathered im2col values of one position scaled
// by 2^sb(p) (the position's own max |x| over its taps: lanes l and l + 32
// hold the two halves of a column), split per frame and tile.  The bias is
// not a row of the product: y = fma(acc, 2^-(sa + sb(p)), b) exactly unscales
// and adds it in one rounding.  A tile whose column max is Inf, or whose
// unscale factor would leave fp32's range, sends the wave's whole frame to
// fwd_item_fp32 (plain fp32 sums, the reference's IEEE Inf / NaN pattern);
// a kernel with Inf in W sends every frame.  The decision is per (frame,
// wave) in every epilogue, so fused and unfused runs compute the same y.
struct PoolWin {
  int ph, pw, pc, oh2, OP;
  FastDiv div_OP, div_oh2;
};

// The F16 fallback for one item (32 filters gb*32.. x the 32 positions of
// p's tile) in fp32: y = sum_k W[k][g] x_k(p), then + b[g] (the reference's
// GEMM then bias add, conv2D.cc:138-145), the accumulator layout of the MFMA.
__device__ __forceinline__ floatx16 fwd_item_fp32(
    const ConvGeom &g, const float *__restrict__ K, int ks, const float *__restrict__ bias,
    const float *Xs, const int2 *koff, int gb, int tile, int lane) {
  const int h = lane >> 5;
  const int p = min(tile * 32 + (lane & 31), g.P - 1);
  uint32_t px, py;
  g.div_oh.divmod((uint32_t)p, px, py);
  const int pb = (int)px * g.H + (int)py;
  floatx16 y;
#pragma unroll
  for (int r = 0; r < 16; r++) y[r] = 0.0f;
  for (int k = 0; k < g.Kdim; k++) {
    const float x = Xs[koff[k].x + pb];
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int gg = gb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      y[r] = fmaf(gg < g.G ? K[(int64_t)k * ks + gg] : 0.0f, x, y[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int gg = gb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    y[r] = y[r] + (bias && gg < g.G ? bias[gg] : 0.0f);
  }
  return y;
}

// The F16 forward's check of an item touching a spread group (f16-split.h):
// with |W'|, |x'| <= 2^15 the elements the split holds only to 2^-25
// (scaled) add at most 2^-9 Kdim to a scaled sum, fct times that to y; an
// output with |y| >= 2^10 Kdim fct therefore carries at most 2^-19 |y| <=
// 2^-19 S of it.  True when some output of the item is below that bound:
// the caller then recomputes the whole item by fwd_item_fp32 (every lane: a
// wave-uniform decision, the same in the fused and the unfused epilogue).
__device__ __forceinline__ bool spread_reject(const floatx16 &y, float fct, const ConvGeom &g) {
  const float thr = fct * (1024.0f * (float)g.Kdim * (1.0f + 1.0f / 1024.0f));
  float mn = fabsf(y[0]);
#pragma unroll
  for (int r = 1; r < 16; r++) mn = fminf(mn, fabsf(y[r]));
  return __builtin_amdgcn_ballot_w64(!(mn >= thr)) != 0;
}

// The routing mask of a 4-way pool group, bit c = (v_c == mx): the four
// compares first, then the four selects, so each select reads a compare
// result three VALU later and needs no wait states (hipcc's order, compare /
// select pairs, pads every pair with s_nop 1).
__device__ __forceinline__ unsigned tie_mask4(float v0, float v1, float v2, float v3, float mx) {
  unsigned m, t0, t1, t2, t3;
  uint64_t c0, c1, c2, c3;
  asm("v_cmp_eq_f32_e64 %5, %9, %13\n\t"
      "v_cmp_eq_f32_e64 %6, %10, %13\n\t"
      "v_cmp_eq_f32_e64 %7, %11, %13\n\t"
      "v_cmp_eq_f32_e64 %8, %12, %13\n\t"
      "v_cndmask_b32_e64 %1, 0, 1, %5\n\t"
      "v_cndmask_b32_e64 %2, 0, 2, %6\n\t"
      "v_cndmask_b32_e64 %3, 0, 4, %7\n\t"
      "v_cndmask_b32_e64 %4, 0, 8, %8\n\t"
      "v_or3_b32 %0, %1, %2, %3\n\t"
      "v_or_b32_e32 %0, %0, %4"
      : "=v"(m), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&s"(c0), "=&s"(c1),
        "=&s"(c2), "=&s"(c3)
      : "v"(v0), "v"(v1), "v"(v2), "v"(v3), "v"(mx));
  return m;
}

// The register-pooled forward's statistics outputs (pool-stats.h): the
// per-frame block rowmax [max[R], min[R], cnt[R]], the per-workgroup column
// partials (the maxima's exponent bytes, [nblk][npool]) and the column block
// colmax [max[npool], min[npool], cnt[npool]], which this kernel initialises
// for pool_colmax_kernel (the maxima) and pool_count_kernel (the minima and
// counts)
struct RpStats {
  uint32_t *rowmax = nullptr, *partials = nullptr, *colmax = nullptr;
};

// The wave's max |pooled| bits of the frame and its min (|pooled| - 1,
// wrapping: a zero never wins; f16-split.h's spread groups) into its slots of
// rslot (LDS: [2][4] maxima, then [2][4] minima; the frame's four slots are
// combined after the next barrier)
__device__ __forceinline__ void frame_row_max(uint32_t *rslot, uint32_t v, uint32_t u, int lane) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    v = max(v, (uint32_t)__shfl_xor((int)v, o));
    u = min(u, (uint32_t)__shfl_xor((int)u, o));
  }
  if (lane == 0) {
    rslot[0] = v;
    rslot[8] = u;
  }
}

// The pooled output's column statistics (pool-stats-dev.h), as kernels of
// their own: the forward launches them unless its caller leaves them to the
// consumer (PoolColDeferred)
__global__ __launch_bounds__(256) void pool_colmax_kernel(const uint8_t *__restrict__ pcol,
                                                           int nblk, int npool,
                                                           uint32_t *__restrict__ colmax) {
  pool_colmax_block(pcol, nblk, npool, colmax, blockIdx.x, blockIdx.y);
}
__global__ __launch_bounds__(256) void pool_count_kernel(const float *__restrict__ P, int ps,
                                                         int R, int npool, int vec,
                                                         uint32_t *__restrict__ rowblk,
                                                         uint32_t *colblk) {
  __shared__ PoolCountSmem sm;
  pool_count_block(P, ps, R, npool, vec, rowblk, colblk, blockIdx.x, gridDim.x, sm);
}

// RP: the register-pooled form only (out == nullptr, PC 2 or 4, G = 128 and
// every wave with FT position tiles: c2), without the generic item loop and
// the LDS epilogue, whose uniform conditions otherwise overflow the SGPRs.
template <int KS, int FT, int PC, int AR, bool RP = false>
__global__ __launch_bounds__(256, 2) void conv_fwd_regs_kernel(
    ConvGeom g, const float *__restrict__ X, int xs,
    const float *__restrict__ K, int ks, const float *__restrict__ bias,
    float *__restrict__ out, int os, int vec_ok, int clk,
    float *__restrict__ pool, int ps, unsigned char *__restrict__ mask, int ms,
    PoolWin pw3, RpStats rps) {
  constexpr bool X6 = AR == 1, F16 = AR == 2, SPL = AR != 0;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *T = reinterpret_cast<float *>(smem);                 // [32][P]
  float *Bs = T + ((32 * g.P + 3) & ~3);                      // [128] bias
  float *Bz = Bs + 128;                                       // [32] -0 (F16 fp32 items)
  int2 *koff = reinterpret_cast<int2 *>(Bs + 160);             // [2*KS] taps
  constexpr int NKT = SPL ? 16 * KS : 2 * KS;                   // tap entries (<= 32)
  float *Xs = reinterpret_cast<float *>(koff + NKT);            // [C*HW]
  uint32_t *rslot = reinterpret_cast<uint32_t *>(Xs + g.C * g.HW);  // [2][2][4] RP row max / min
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = lane & 31, h = lane >> 5;
  const int NG = (g.G + 31) >> 5;  // <= 4 (host check)
  if (tid < 128) Bs[tid] = (bias && tid < g.G) ? bias[tid] : 0.0f;
  if (tid < 32) Bz[tid] = -0.0f;
  // A operand: W[k = 2s + h][gb*32 + l]
  float wreg[X6 ? 1 : 4][X6 ? 1 : KS];
  // X6: W^T[gb*32 + l][k = 16s + 8h + e] (e < 8), the bias at k = Kdim
  x6::bf16x8 w6[X6 ? 4 : 1][X6 ? KS : 1][3];
  // F16: W^T[gb*32 + l][k = 16s + 8h + e] * 2^sa, hi and lo planes
  f16x3::f16x8 wh[F16 ? 4 : 1][F16 ? KS : 1], wl[F16 ? 4 : 1][F16 ? KS : 1];
  int sa = 0;
  bool wslow = false;  // Inf in W: every item in fp32
  bool wspread = false;  // W is a spread group (f16-split.h): every item checked
  const float m1 = F16 ? f16x3::opaque_m1() : 0.0f;  // the split's -1 (f16-split.h)
  if constexpr (F16) {
    float wv[4][KS][8];
    float m = 0.0f;
    uint32_t mn = 0xffffffffu;  // min 2|w| - 2 (wrapping: a zero never wins)
#pragma unroll
    for (int gb = 0; gb < 4; gb++)
#pragma unroll
      for (int s = 0; s < KS; s++)
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const int k = 16 * s + 8 * h + e, gg = gb * 32 + l;
          wv[gb][s][e] = gg < g.G && k < g.Kdim ? K[(int64_t)k * ks + gg] : 0.0f;
          m = fmaxf(m, fabsf(wv[gb][s][e]));  // NaN ignored: it propagates by itself
          mn = min(mn, (__float_as_uint(wv[gb][s][e]) << 1) - 2u);
        }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      m = fmaxf(m, __shfl_xor(m, o));
      mn = min(mn, (uint32_t)__shfl_xor((int)mn, o));
    }
    const uint32_t mwb = __builtin_amdgcn_readfirstlane(__float_as_uint(m));
    wspread = f16x3::spread(mwb, (__builtin_amdgcn_readfirstlane(mn) >> 1) + 1u);
    const int s0 = f16x3::scale_exp(mwb);
    wslow = s0 == f16x3::SKIP;
    sa = wslow ? 0 : s0;
#pragma unroll
    for (int gb = 0; gb < 4; gb++)
#pragma unroll
      for (int s = 0; s < KS; s++) f16x3::split8h(wv[gb][s], sa, wh[gb][s], wl[gb][s], m1);
  }
  if constexpr (X6) {
#pragma unroll
    for (int gb = 0; gb < 4; gb++)
#pragma unroll
      for (int s = 0; s < KS; s++) {
        const int gg = gb * 32 + l;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const int k = 16 * s + 8 * h + e;
          v[e] = gg >= g.G ? 0.0f
                 : k < g.Kdim ? K[(int64_t)k * ks + gg]
                 : (k == g.Kdim && bias) ? bias[gg] : 0.0f;
        }
        x6::split8(v, w6[gb][s][0], w6[gb][s][1], w6[gb][s][2]);
      }
  } else {
#pragma unroll
    for (int gb = 0; gb < 4; gb++)
#pragma unroll
      for (int s = 0; s < KS; s++) {
        const int k = 2 * s + h, gg = gb * 32 + l;
        wreg[gb][s] = (k < g.Kdim && gg < g.G) ? K[(int64_t)k * ks + gg] : 0.0f;
      }
  }
  // tap k -> (channel offset, kx << 16 | ky); padded taps never in bounds.
  // X6 (unpadded maps): tap k -> its map offset c*HW + kx*H + ky in .x
  if (tid < NKT) {
    int2 v = make_int2(0, 0x3fff << 16);
    if (tid < g.Kdim) {
      uint32_t c, r, qx, qy;
      g.div_khkw.divmod((uint32_t)tid, c, r);
      g.div_kh.divmod(r, qx, qy);
      v = SPL ? make_int2((int)c * g.HW + (int)qx * g.H + (int)qy, 0)
             : make_int2((int)c * g.HW, (int)((qx << 16) | qy));
    }
    koff[tid] = v;
  }
  const int CHW = g.C * g.HW;
  const int ntile = (g.P + 31) >> 5;
  // X6: every aligned group of 8 taps one run of consecutive map offsets
  // (c2's 8 x 1 kernel: taps c*8 + ky at c*HW + ky)?  Then a group's 8 values
  // are read at one offset + e, without the per-tap table reads
  bool run8 = false;
  if constexpr (SPL) {
    run8 = true;
    for (int k = 0; k + 1 < g.Kdim && run8; k++) {
      if ((k + 1) % 8 == 0) continue;
      uint32_t c0, r0, x0, y0, c1, r1, x1, y1;
      g.div_khkw.divmod((uint32_t)k, c0, r0);
      g.div_kh.divmod(r0, x0, y0);
      g.div_khkw.divmod((uint32_t)(k + 1), c1, r1);
      g.div_kh.divmod(r1, x1, y1);
      const int o0 = (int)c0 * g.HW + (int)x0 * g.H + (int)y0;
      const int o1 = (int)c1 * g.HW + (int)x1 * g.H + (int)y1;
      run8 = o1 == o0 + 1;
    }
  }
  KCNN_TMARKS(6)  // per-phase totals of block 0 (clk != 0)
  // RP: the pooled output's statistics for the FC GEMM that reads it
  // (cu-gemm-f16x3.hip's operand scales): max |value| bits per frame (prow,
  // atomic max) and per pooled column over this workgroup's frames, kept in
  // the LDS slab T (unused by this form; npool = 32 * P words) by ds_max and
  // stored to the workgroup's row of the partials pcol at the end
  uint32_t *Tcol = reinterpret_cast<uint32_t *>(T);
  uint32_t *const prow = rps.rowmax, *const pcol = rps.partials;
  if constexpr (RP) {
    for (int e = tid; e < g.G / PC * g.P; e += 256) Tcol[e] = 0;
    // the column block for the kernels after this grid: pool_colmax_kernel's
    // atomic maxima start from 0, pool_count_kernel's minima from 0xffffffff
    // and its counts from 0
    const int c = blockIdx.x * 256 + tid;
    if (rps.colmax && c < g.G / PC * g.P) {
      rps.colmax[c] = 0;
      rps.colmax[g.G / PC * g.P + c] = 0xffffffffu;
      rps.colmax[2 * g.G / PC * g.P + c] = 0;
    }
  }
  // the next frame's map is prefetched into registers while this one runs
  constexpr int XV = 8;  // CHW <= 2048 (host check)
  float xv[XV];
#pragma unroll
  for (int i = 0; i < XV; i++)
    if (blockIdx.x < (unsigned)g.R && tid + 256 * i < CHW)
      xv[i] = X[(int64_t)blockIdx.x * xs + tid + 256 * i];
  int it = 0;  // this workgroup's frame count
  for (int n = blockIdx.x; n < g.R; n += gridDim.x, ++it) {
    // lane ids made opaque per frame: the frame-invariant LDS / global
    // addresses are recomputed instead of hoisted out of the loop (hoisted,
    // they overflow the register file)
    int tid_f = tid;
    asm volatile("" : "+v"(tid_f));
    int wave_q = wave;  // likewise the wave id (held, the wave-derived item
    asm volatile("" : "+s"(wave_q));  // constants overflow the SGPRs)
    const int lane_f = tid_f & 63, l_f = lane_f & 31, h_f = lane_f >> 5;
    __syncthreads();  // previous frame's Xs / T reads done
    if constexpr (RP) {  // the previous frame's row maximum from its four wave slots
      if (it > 0 && tid_f == 0 && prow) {
        const uint32_t *q = rslot + ((it - 1) & 1) * 4;
        prow[n - (int)gridDim.x] = max(max(q[0], q[1]), max(q[2], q[3]));
        prow[g.R + n - (int)gridDim.x] = min(min(q[8], q[9]), min(q[10], q[11])) + 1u;
      }
    }
    KCNN_TMARK(5)
#pragma unroll
    for (int i = 0; i < XV; i++)
      if (tid_f + 256 * i < CHW) Xs[tid_f + 256 * i] = xv[i];
    if (n + (int)gridDim.x < g.R) {
#pragma unroll
      for (int i = 0; i < XV; i++)
        if (tid_f + 256 * i < CHW)
          xv[i] = X[(int64_t)(n + gridDim.x) * xs + tid_f + 256 * i];
    }
    __syncthreads();
    KCNN_TMARK(0)
    float bx[SPL ? 1 : FT][SPL ? 1 : KS];
    x6::bf16x8 bx6[X6 ? FT : 1][X6 ? KS : 1][3];
    f16x3::f16x8 bxh[F16 ? FT : 1][F16 ? KS : 1], bxl[F16 ? FT : 1][F16 ? KS : 1];
    float ft[F16 ? FT : 1];  // F16: the unscale factor 2^-(sa + sb(p)) of tile t
    bool slow = false;       // F16: this wave_q's items of the frame in fp32
    int tsp = 0;             // F16: bit t, tile t has a spread position column
#pragma unroll
    for (int t = 0; t < FT; t++) {
      if constexpr (F16) {
        // B[k = 16s + 8h + e][p] = x_k(p) for k < Kdim, 0 past it
        if ((wave_q + 4 * t) * 32 >= g.P) continue;  // wave_q-uniform: no tile
        const int p = min((wave_q + 4 * t) * 32 + l_f, g.P - 1);
        uint32_t px, py;
        g.div_oh.divmod((uint32_t)p, px, py);
        const int pb = (int)px * g.H + (int)py;
        float v[KS][8];
        float m = 0.0f;
        uint32_t mn = 0xffffffffu;  // min 2|x| - 2 (wrapping: a zero never wins)
#pragma unroll
        for (int s = 0; s < KS; s++) {
          const int k0 = 16 * s + 8 * h_f;
          if (run8) {  // uniform
            const float *xr = Xs + koff[k0].x + pb;
#pragma unroll
            for (int e = 0; e < 8; e++) v[s][e] = xr[e];
          } else {
#pragma unroll
            for (int e = 0; e < 8; e++) v[s][e] = Xs[koff[k0 + e].x + pb];
          }
#pragma unroll
          for (int e = 0; e < 8; e++) {
            v[s][e] = k0 + e < g.Kdim ? v[s][e] : 0.0f;
            m = fmaxf(m, fabsf(v[s][e]));
            mn = min(mn, (__float_as_uint(v[s][e]) << 1) - 2u);
          }
        }
        // the column's other half: lane l ^ 32, through ds_bpermute.  (With
        // v_permlane32_swap here, one accumulator register of 16 lanes of a
        // wave's last item came out wrong in about one call in four of a
        // 601-frame forward, G = 96, Kdim 12; experiments/diag_det2.py.)
        m = fmaxf(m, __shfl_xor(m, 32));
        mn = min(mn, (uint32_t)__shfl_xor((int)mn, 32));
        const uint32_t mb = __float_as_uint(m);
        // a spread position column (f16-split.h): the tile's items are checked
        if (__builtin_amdgcn_ballot_w64(f16x3::spread(mb, (mn >> 1) + 1u)) != 0) tsp |= 1 << t;
        int sb = mb == 0 ? -sa : f16x3::scale_exp(mb);
        const int E = -(sa + sb);
        const bool bad = sb == f16x3::SKIP || E < -149 || E > 127;
        if (bad) sb = 0;
        ft[t] = __builtin_amdgcn_ldexpf(1.0f, bad ? 0 : E);
        if (__builtin_amdgcn_ballot_w64(bad) != 0) slow = true;
#pragma unroll
        for (int s = 0; s < KS; s++) f16x3::split8h(v[s], sb, bxh[t][s], bxl[t][s], m1);
        continue;
      }
      if constexpr (X6) {
        // B[k = 16s + 8h + e][p]: the map value of tap k at p (one add: the
        // maps are unpadded, so every tap of a valid position is inside),
        // 1 at k = Kdim (the bias row), 0 past it; positions past P read a
        // clamped position and are never stored
        if ((wave_q + 4 * t) * 32 >= g.P) continue;  // wave_q-uniform: no tile
        const int p = min((wave_q + 4 * t) * 32 + l_f, g.P - 1);
        uint32_t px, py;
        g.div_oh.divmod((uint32_t)p, px, py);
        const int pb = (int)px * g.H + (int)py;
#pragma unroll
        for (int s = 0; s < KS; s++) {
          float v[8];
          const int k0 = 16 * s + 8 * h_f;
          if (run8) {  // uniform
            const float *xr = Xs + koff[k0].x + pb;
#pragma unroll
            for (int e = 0; e < 8; e++) {
              const float xval = xr[e];
              v[e] = k0 + e < g.Kdim ? xval : (k0 + e == g.Kdim ? 1.0f : 0.0f);
            }
          } else {
#pragma unroll
            for (int e = 0; e < 8; e++) {
              const int k = k0 + e;
              const float xval = Xs[koff[k].x + pb];
              v[e] = k < g.Kdim ? xval : (k == g.Kdim ? 1.0f : 0.0f);
            }
          }
          x6::split8(v, bx6[t][s][0], bx6[t][s][1], bx6[t][s][2]);
        }
        continue;
      }
      const int p = (wave_q + 4 * t) * 32 + l_f;
      const bool pv = p < g.P;
      uint32_t px = 0, py = 0;
      g.div_oh.divmod((uint32_t)(pv ? p : 0), px, py);
#pragma unroll
      for (int s = 0; s < KS; s++) {
        const int2 ko = koff[2 * s + h_f];
        const int xx = (int)px + (ko.y >> 16) - g.pad_w;
        const int yy = (int)py + (ko.y & 0xffff) - g.pad_h;
        const bool ok = pv && (unsigned)xx < (unsigned)g.W && (unsigned)yy < (unsigned)g.H;
        const float v = Xs[ok ? ko.x + xx * g.H + yy : 0];
        bx[t][s] = ok ? v : 0.0f;
      }
    }
    if constexpr (F16) slow = slow || wslow;
    KCNN_TMARK(1)
    if constexpr (SPL && (PC == 2 || PC == 4)) {
      if (out == nullptr) {  // uniform: pooled straight from the registers
        // items (gb, t) in order; the MFMA chain of item i is issued before
        // the pooling of item i - 1, so that VALU work runs under the chain
        constexpr int NI = 4 * FT;
        const int npool = g.G / PC * g.P;  // pooled values of one frame row
        const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(pool + (int64_t)n * ps), (short)0, npool * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t mrs = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(mask + (int64_t)n * ms), (short)0, npool, 0x00020000);
        auto valid = [&](int i) { return i / FT < NG && wave_q + 4 * (i % FT) < ntile; };
        // the pooling of one item's accumulators (F16: y = acc * 2^-(sa +
        // sb(p)) + b first, in one rounding; fp32 items: acc * 1 + -0, i.e.
        // acc itself)
        uint32_t redo = 0;    // F16: items (bit gb * FT + t) recomputed in fp32
        uint32_t rowrun = 0;  // RP: max |pooled| bits of this lane in the frame
        uint32_t rowmn = 0xffffffffu;  // RP: min (|pooled| - 1) of this lane in the frame
        // (chk: std::true_type in the frames that touch a spread group, which
        // run their own copy of the item sequence, so the common one stays
        // free of the check's branches)
        auto pool_item = [&](floatx16 &acc, int gb, int t, bool sl, auto chk) {
          const int p = (wave_q + 4 * t) * 32 + l_f;
          // accumulator r = 4k + i of lane (l, h) is filter 8k + 4h + i at
          // position p: a pool group is PC consecutive registers (the
          // compares and order of the LDS epilogue, so the same bits).  Its
          // pooled row is U + h * 4 / PC with U uniform: buffer stores take
          // the lane part as voffset and U as soffset (no vector address
          // arithmetic).  Positions past P, and rows past G (G not a
          // multiple of 32), get a voffset past the descriptors' ranges and
          // are dropped (the range check covers voffset, not soffset).
          const unsigned vo = p < g.P ? (unsigned)(h_f * (4 / PC) * g.P + p) : 0x3ffffff0u;
          // the rows' soffsets U * P recomputed per item (SALU) instead of
          // hoisted out of the frame loop (held, they spill SGPRs)
          int Pq = g.P;
          asm volatile("" : "+s"(Pq));
          const float fct = F16 && !sl ? ft[F16 ? t : 0] : 1.0f;
          // the bias rows' offset made opaque per item: the loads are not
          // hoisted or shared across items (held for all four filter groups
          // they would take 64 VGPRs and spill)
          int boff = (sl ? 128 : gb * 32) + 4 * h_f;  // Bz = Bs + 128
          asm volatile("" : "+v"(boff));
          const float *bb = Bs + boff;
          if constexpr (F16) {
            // y = acc * 2^-(sa + sb(p)) + b in one rounding (fp32 items:
            // acc * 1 + -0, i.e. acc itself)
#pragma unroll
            for (int k = 0; k < 4; k++) {
              const float4 b4 = *reinterpret_cast<const float4 *>(bb + 8 * k);
              acc[4 * k + 0] = fmaf(acc[4 * k + 0], fct, b4.x);
              acc[4 * k + 1] = fmaf(acc[4 * k + 1], fct, b4.y);
              acc[4 * k + 2] = fmaf(acc[4 * k + 2], fct, b4.z);
              acc[4 * k + 3] = fmaf(acc[4 * k + 3], fct, b4.w);
            }
            if constexpr (decltype(chk)::value) {
              if (!sl && (wspread || (tsp >> t) & 1) && spread_reject(acc, fct, g)) {
                redo |= 1u << (gb * FT + t);  // uniform, rare: pooled after the sequence
                return;
              }
            }
          }
          // The pool value by IEEE max (v_max3: NaN skipped like the
          // reference's `val < x` test, ties between equal nonzero values
          // are the same bits).  The one case max and the reference's
          // first-wins scan differ is a +0 / -0 tie: any group whose max is
          // zero is rescanned the reference's way (uniform branch, rare).
          constexpr int NGP = 16 / PC;
          float mx[NGP];
          unsigned msk[NGP];
          bool anyz = false;
#pragma unroll
          for (int j = 0; j < NGP; j++) {
            float m = fmaxf(-1e20f, acc[j * PC]);
#pragma unroll
            for (int c = 1; c < PC; c++) m = fmaxf(m, acc[j * PC + c]);
            mx[j] = m;
            anyz |= m == 0.0f;
          }
          if (__builtin_expect(anyz, 0)) {
#pragma unroll
            for (int j = 0; j < NGP; j++) {
              if (mx[j] == 0.0f) {
                float m = -1e20f;
#pragma unroll
                for (int c = 0; c < PC; c++)
                  if (m < acc[j * PC + c]) m = acc[j * PC + c];
                mx[j] = m;
              }
            }
          }
          if constexpr (RP) {
            // lanes past P hold position P - 1's values: their max lands there
            const int pc = min(p, g.P - 1) + h_f * (4 / PC) * Pq;
#pragma unroll
            for (int j = 0; j < NGP; j++) {
              const uint32_t a = __float_as_uint(mx[j]) & 0x7fffffffu;  // never NaN
              const int r0 = j * PC;
              const int U = (gb * 32 + (r0 & 3) + 8 * (r0 >> 2)) / PC;
              __hip_atomic_fetch_max(Tcol + U * Pq + pc, a, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_WORKGROUP);
              rowrun = max(rowrun, a);
              const uint32_t u = a - 1u;  // wraps for 0: never the min
              rowmn = min(rowmn, u);
            }
            // (pinned per item: left free, the scheduler spreads the items'
            // statistics and holds 34 more VGPRs)
            asm volatile("" : "+v"(rowrun), "+v"(rowmn));
          }
#pragma unroll
          for (int j = 0; j < NGP; j++) {
            if constexpr (PC == 4) {
              msk[j] = tie_mask4(acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3], mx[j]);
            } else {
              unsigned m = 0;
#pragma unroll
              for (int c = 0; c < PC; c++) m |= (acc[j * PC + c] == mx[j] ? 1u : 0u) << c;
              msk[j] = m;
            }
          }
#pragma unroll
          for (int j = 0; j < NGP; j++) {
            const int r0 = j * PC;
            const int U = (gb * 32 + (r0 & 3) + 8 * (r0 >> 2)) / PC;
            const unsigned vv =
                g.G % 32 == 0 || U + h_f * (4 / PC) < g.G / PC ? vo : 0x3ffffff0u;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(mx[j]), prs, vv * 4u,
                                                  (unsigned)(U * Pq) * 4u, 0);
            __builtin_amdgcn_raw_buffer_store_b8((unsigned char)msk[j], mrs, vv,
                                                 (unsigned)(U * Pq), 0);
          }
        };
        // the items in fp32 (fwd_item_fp32, then pooled like any other):
        // every valid item of a slow frame (Inf, range), or the items a
        // spread check rejected; one code copy for both
        auto fp32_items = [&]() {
#pragma unroll 1
          while (redo) {  // uniform
            const int i = __builtin_ctz(redo);
            redo &= redo - 1;
            const int gb = i / FT, t = i % FT;
            floatx16 a = fwd_item_fp32(g, K, ks, bias, Xs, koff, gb, wave_q + 4 * t, lane_f);
            pool_item(a, gb, t, true, std::false_type{});
          }
        };
        if constexpr (F16) {
          if (slow) {  // uniform: the frame's items in fp32 (rare: Inf, range)
#pragma unroll 1
            for (int i = 0; i < NI; i++)
              if (RP || valid(i)) redo |= 1u << i;
            fp32_items();
            if constexpr (RP) frame_row_max(rslot + (it & 1) * 4 + wave_q, rowrun, rowmn, lane_f);
            KCNN_TMARK(2)
            continue;  // next frame
          }
        }
        auto chain = [&](int gb, int t) {
          floatx16 a = zero16();
#pragma unroll
          for (int s = 0; s < KS; s++) {
            if constexpr (F16)
              a = f16x3::mfma3(wh[gb][s], wl[gb][s], bxh[t][s], bxl[t][s], a);
            else
              a = x6::mfma6(w6[gb][s], bx6[t][s], a);
          }
          return a;
        };
        auto sequence = [&](auto chk) {
          if (RP || (NG == 4 && wave_q + 4 * (FT - 1) < ntile)) {
            // every item valid (c2: G = 128, P = 363): one straight-line
            // sequence, the MFMA chain of item i beside the pooling of i - 1
            floatx16 prev = chain(0, 0);
#pragma unroll
            for (int i = 1; i <= NI; i++) {
              floatx16 cur;
              if (i < NI) cur = chain(i / FT, i % FT);
              pool_item(prev, (i - 1) / FT, (i - 1) % FT, false, chk);
              if (i < NI) prev = cur;
            }
          } else if constexpr (!RP) {
#pragma unroll
            for (int i = 0; i < NI; i++) {
              if (!valid(i)) continue;  // uniform
              floatx16 a = chain(i / FT, i % FT);
              pool_item(a, i / FT, i % FT, false, chk);
            }
          }
        };
        if (F16 && (wspread || tsp != 0)) sequence(std::true_type{});  // uniform, rare
        else sequence(std::false_type{});
        if constexpr (F16) fp32_items();  // the items a spread check rejected (rare)
        if constexpr (RP) frame_row_max(rslot + (it & 1) * 4 + wave_q, rowrun, rowmn, lane_f);
        KCNN_TMARK(2)
        continue;  // next frame
      }
    }
    if constexpr (RP) continue;  // (never reached: host check)
#pragma unroll
    for (int gb = 0; gb < 4; gb++) {
      if (gb >= NG) break;
      float bsv[16];  // this lane_f's 16 accumulator rows' bias, read ahead (X6: 0, in acc)
#pragma unroll
      for (int r = 0; r < 16; r++) bsv[r] = X6 ? 0.0f : Bs[gb * 32 + mfma32_row(r, lane_f)];
#pragma unroll
      for (int t = 0; t < FT; t++) {
        const int pt = wave_q + 4 * t;
        if (pt >= ntile) continue;  // wave_q-uniform
        floatx16 acc = zero16();
        if constexpr (F16) {
          bool fp = slow;  // uniform
          if (!fp) {
#pragma unroll
            for (int s = 0; s < KS; s++)
              acc = f16x3::mfma3(wh[gb][s], wl[gb][s], bxh[t][s], bxl[t][s], acc);
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = fmaf(acc[r], ft[t], bsv[r]);
            fp = (wspread || (tsp >> t) & 1) && spread_reject(acc, ft[t], g);  // rare
          }
          if (fp) acc = fwd_item_fp32(g, K, ks, bias, Xs, koff, gb, pt, lane_f);
        } else if constexpr (X6) {
#pragma unroll
          for (int s = 0; s < KS; s++) acc = x6::mfma6(w6[gb][s], bx6[t][s], acc);
        } else {
#pragma unroll
          for (int s = 0; s < KS; s++)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wreg[gb][s], bx[t][s], acc, 0, 0, 0);
        }
        const int p = pt * 32 + l_f;
        if constexpr (PC == 2 || PC == 4) {
          if (out == nullptr) {  // uniform: pooled straight from the registers
            // accumulator r = 4k + i of lane (l, h) is filter 8k + 4h + i of
            // the slab at position p: a pool group of PC filters is PC
            // consecutive registers of one lane.  Same adds, compares and
            // order as the LDS epilogue below, so the same bits.
            if (p < g.P) {
              float *pd = pool + (int64_t)n * ps + p;
              unsigned char *md = mask + (int64_t)n * ms + p;
#pragma unroll
              for (int r0 = 0; r0 < 16; r0 += PC) {
                const int row = gb * 32 + mfma32_row(r0, lane_f);
                if (row >= g.G) continue;
                float mx = -1e20f, v[PC];
#pragma unroll
                for (int c = 0; c < PC; c++) {
                  v[c] = SPL ? acc[r0 + c] : acc[r0 + c] + bsv[r0 + c];
                  if (mx < v[c]) mx = v[c];
                }
                unsigned m = 0;
#pragma unroll
                for (int c = 0; c < PC; c++) m |= (v[c] == mx ? 1u : 0u) << c;
                const int64_t off = (int64_t)(row / PC) * g.P;
                pd[off] = mx;
                md[off] = (unsigned char)m;
              }
            }
            continue;
          }
        }
        if (p < g.P) {
#pragma unroll
          for (int r = 0; r < 16; r++)
            T[mfma32_row(r, lane_f) * g.P + p] = SPL ? acc[r] : acc[r] + bsv[r];
        }
      }
      KCNN_TMARK(2)
      if constexpr (PC == 2 || PC == 4) {
        if (out == nullptr) continue;  // nothing staged in T
      }
      __syncthreads();
      KCNN_TMARK(3)
      const int rows = g.G - gb * 32 < 32 ? g.G - gb * 32 : 32;
      const int cnt = rows * g.P;
      // out == nullptr (pooled variants): the caller needs only the pooled
      // output and the routing mask, Y itself is never stored
      float *dst = out ? out + (int64_t)n * os + (int64_t)gb * 32 * g.P : nullptr;
      if (dst == nullptr) {
      } else if (vec_ok & 2) {  // streaming stores: Y is not re-read here
        typedef float f4 __attribute__((ext_vector_type(4)));
        const f4 *src4 = reinterpret_cast<const f4 *>(T);
        f4 *dst4 = reinterpret_cast<f4 *>(dst);
        for (int e = tid_f; e < (cnt >> 2); e += 256)
          __builtin_nontemporal_store(src4[e], dst4 + e);
        for (int e = (cnt & ~3) + tid_f; e < cnt; e += 256) dst[e] = T[e];
      } else if (vec_ok) {
        const float4 *src4 = reinterpret_cast<const float4 *>(T);
        float4 *dst4 = reinterpret_cast<float4 *>(dst);
        for (int e = tid_f; e < (cnt >> 2); e += 256) dst4[e] = src4[e];
        for (int e = (cnt & ~3) + tid_f; e < cnt; e += 256) dst[e] = T[e];
      } else {
        for (int e = tid_f; e < cnt; e += 256) dst[e] = T[e];
      }
      if constexpr (PC < 0) {  // 3-D window; rows % pc == 0 (host check)
        constexpr int CPH = PC == -3 ? 3 : 0, CPW = PC == -3 ? 1 : 0, CPC = PC == -3 ? 4 : 0;
        const int wph = CPH ? CPH : pw3.ph, wpw = CPW ? CPW : pw3.pw, wpc = CPC ? CPC : pw3.pc;
        const int cnt_p = rows / wpc * pw3.OP;
        const int64_t pb = (int64_t)(gb * 32 / wpc) * pw3.OP;
        float *pd = pool + (int64_t)n * ps + pb;
        unsigned short *md = reinterpret_cast<unsigned short *>(mask) + (int64_t)n * ms + pb;
        for (int e = tid_f; e < cnt_p; e += 256) {
          uint32_t j, q, wi, hi;
          pw3.div_OP.divmod((uint32_t)e, j, q);
          pw3.div_oh2.divmod(q, wi, hi);
          const float *t = T + (int)j * wpc * g.P + (int)wi * wpw * g.oh + (int)hi * wph;
          float val = -1e20f;  // A.8: c, then w, then h
          unsigned m = 0;
          if constexpr (CPH > 0) {
            float v[CPC * CPW * CPH];
#pragma unroll
            for (int c = 0; c < CPC; c++)
#pragma unroll
              for (int w = 0; w < CPW; w++)
#pragma unroll
                for (int h = 0; h < CPH; h++)
                  v[(c * CPW + w) * CPH + h] = t[c * g.P + w * g.oh + h];
#pragma unroll
            for (int b = 0; b < CPC * CPW * CPH; b++)
              if (val < v[b]) val = v[b];
#pragma unroll
            for (int b = 0; b < CPC * CPW * CPH; b++) m |= (v[b] == val ? 1u : 0u) << b;
          } else {
            for (int c = 0; c < wpc; c++)
              for (int w = 0; w < wpw; w++)
                for (int h = 0; h < wph; h++) {
                  const float v = t[c * g.P + w * g.oh + h];
                  if (val < v) val = v;
                }
            int bit = 0;
            for (int c = 0; c < wpc; c++)
              for (int w = 0; w < wpw; w++)
                for (int h = 0; h < wph; h++, bit++)
                  m |= (t[c * g.P + w * g.oh + h] == val ? 1u : 0u) << bit;
          }
          pd[e] = val;
          md[e] = (unsigned short)m;
        }
      }
      if constexpr (PC > 0) {  // rows % PC == 0 (host check)
        const int cnt_p = rows / PC * g.P;
        const int64_t pb = (int64_t)(gb * 32 / PC) * g.P;
        float *pd = pool + (int64_t)n * ps + pb;
        unsigned char *md = mask + (int64_t)n * ms + pb;
        for (int e = tid_f; e < cnt_p; e += 256) {
          uint32_t j, q;
          g.div_P.divmod((uint32_t)e, j, q);
          const float *t = T + (int)j * PC * g.P + (int)q;
          float v[PC];
#pragma unroll
          for (int c = 0; c < PC; c++) v[c] = t[c * g.P];
          float val = -1e20f;
#pragma unroll
          for (int c = 0; c < PC; c++)
            if (val < v[c]) val = v[c];
          unsigned m = 0;
#pragma unroll
          for (int c = 0; c < PC; c++) m |= (v[c] == val ? 1u : 0u) << c;
          pd[e] = val;
          md[e] = (unsigned char)m;
        }
      }
      KCNN_TMARK(4)
      __syncthreads();
      KCNN_TMARK(5)
    }
  }
  if constexpr (RP) {
    // this workgroup's row of the column partials, and its last frame's row
    // maximum
    __syncthreads();
    if (it > 0 && tid == 0 && prow) {
      const uint32_t *q = rslot + ((it - 1) & 1) * 4;
      const int fr = blockIdx.x + (it - 1) * (int)gridDim.x;
      prow[fr] = max(max(q[0], q[1]), max(q[2], q[3]));
      prow[g.R + fr] = min(min(q[8], q[9]), min(q[10], q[11])) + 1u;
    }
    if (pcol) {  // exponent bytes (pool_colmax_kernel), four per dword store
      const int npool = g.G / PC * g.P;
      uint8_t *dst = reinterpret_cast<uint8_t *>(pcol) + (int64_t)blockIdx.x * npool;
      if (npool % 4 == 0) {
        for (int e = 4 * tid; e < npool; e += 1024)
          *reinterpret_cast<uint32_t *>(dst + e) =
              (Tcol[e] >> 23) | (Tcol[e + 1] >> 23) << 8 | (Tcol[e + 2] >> 23) << 16 |
              (Tcol[e + 3] >> 23) << 24;
      } else {
        for (int e = tid; e < npool; e += 256) dst[e] = (uint8_t)(Tcol[e] >> 23);
      }
    }
  }
#ifdef KCNN_PHASE_TIMING
  if (clk && blockIdx.x == 0 && lane == 0)
    printf("fwd wave %d: xload %lld gather %lld mfma %lld bar1 %lld store %lld bar2 %lld\n",
           wave, tm[0], tm[1], tm[2], tm[3], tm[4], tm[5]);
#endif
}

size_t fwd_lds(const ConvGeom &g, int Kpad, int Gp) {
  return (size_t)align16(Kpad * 8) + (size_t)Kpad * Gp * 4 + (size_t)g.C * g.HW * 4;
}

// conv_fwd_regs_kernel: 3 resident blocks per CU when their LDS fits (c2:
// 52 KB each; VGPRs allow 3).  The third block overlaps the others' store
// and barrier phases: c2 forward+pool 224 -> 200 us, although 4096 frames
// then split 5/6 per block instead of 8.
int fwd_regs_blocks_per_cu(size_t lds) {
  return lds * 3 <= 160 * 1024 ? 3 : 2;
}

// The register forward on the bf16 matrix cores (X6): unpadded maps with
// Kdim <= 31 (the bias takes row Kdim of at most two k16 steps) and one
// filter chunk (G <= 128).  Its ~200 VGPRs hold two workgroups per CU where
// the fp32 kernel holds three, and the kernel is bound by its gather and
// pool/store epilogue more than by its MFMAs: c2 fused forward + pool 137 ->
// 132 us, but c5 C1 (G = 256 in two chunks, 3-D pool from LDS) 0.52 ->
// 0.62 ms with the runtime window, and the same speed (c5 447.0 k vs 446.5 k
// frames/s) once the 3 x 1 x 4 window is compiled in, so chunked layers keep
// the fp32 MFMA.  The rule depends on the
// layer's shape only, so a fused and an unfused run of a layer use the same
// arithmetic (bitwise-equal outputs).  KCNN_FWD_X6=0 keeps the fp32 MFMA.
// The f16x3 form (family value 2, the default) has the same limits except
// Kdim <= 32 (no bias row) and half the MFMAs per item.
// Returns the kernel's AR: 0 fp32 MFMA, 1 bf16x6, 2 f16x3.
int fwd_arith(const ConvGeom &g, int use) {
  if (!use || g.pad_h != 0 || g.pad_w != 0 || g.Gtot > 128) return 0;
  if (use == 2) return g.Kdim <= 32 ? 2 : 0;
  return g.Kdim <= 31 ? 1 : 0;
}

// conv_fwd_regs_kernel's shape limits and dynamic LDS bytes (0: the shape is
// outside them or the plan does not fit).
size_t fwd_regs_lds(const ConvGeom &g) {
  if (g.Kdim > 32 || g.G > 128 || g.P < 16 || g.P > 4 * 32 * 3 || g.C * g.HW > 256 * 8)
    return 0;
  const size_t lds = (size_t)((32 * g.P + 3) & ~3) * 4 + 160 * 4 + 32 * 8 +
                     (size_t)g.C * g.HW * 4 + 8 * 4;
  return lds <= (size_t)kFrameLdsMax ? lds : 0;
}

}  // namespace

// The fused conv + pool forward's Y stores (fusion mode 2, Y kept for later)
// as streaming stores (vec_ok bit 1): c2 213 -> 206 us.  Not for the unfused
// conv, whose Y the pool reads right after (155 -> 181 us there).
static constexpr int kYNt = 2;

// conv_fwd_regs_kernel on one filter chunk.  The callers name the operands
// (pc == 0, pool and mask NULL: the convolution alone; else a ph x pw x pc
// max pool whose window the caller has checked); fwd_regs adds the launch
// values below them.
struct FwdRegs {
  const float *X = nullptr, *K = nullptr, *bias = nullptr;
  int xs = 0, ks = 0;
  float *out = nullptr, *pool = nullptr;
  int os = 0, ps = 0;
  unsigned char *mask = nullptr;
  int ms = 0, pc = 0, ph = 1, pw = 1;
  // set by fwd_regs
  int vec_ok = 0, clk = 0;
  PoolWin pw3{};
  bool rp = false;  // the register-pooled-only form (PC 4, f16x3): 8 more words of row slots
  RpStats rps;
  unsigned grid = 0;
  size_t lds = 0;
};

template <int KS, int PC, int AR>
static void fwd_regs_launch(const ConvGeom &g, const FwdRegs &a, hipStream_t st) {
  if constexpr (PC == 4 && AR == 2) {
    if (a.rp) {
      hipLaunchKernelGGL((conv_fwd_regs_kernel<KS, 3, PC, AR, true>), dim3(a.grid), dim3(256),
                         a.lds + 8 * 4, st, g, a.X, a.xs, a.K, a.ks, a.bias, a.out, a.os,
                         a.vec_ok, a.clk, a.pool, a.ps, a.mask, a.ms, a.pw3, a.rps);
      return;
    }
  }
  hipLaunchKernelGGL((conv_fwd_regs_kernel<KS, 3, PC, AR>), dim3(a.grid), dim3(256), a.lds, st,
                     g, a.X, a.xs, a.K, a.ks, a.bias, a.out, a.os, a.vec_ok, a.clk, a.pool,
                     a.ps, a.mask, a.ms, a.pw3, RpStats{});
}

// The kernel's k-steps and arithmetic for one pool form PC (0: no pool).
template <int PC>
static void fwd_regs_ks(const ConvGeom &g, const FwdRegs &a, int ar, hipStream_t st) {
  const int ksn = (g.Kdim + 1) / 2;
  if (ar == 2 && g.Kdim <= 16) fwd_regs_launch<1, PC, 2>(g, a, st);
  else if (ar == 2) fwd_regs_launch<2, PC, 2>(g, a, st);
  else if (ar == 1 && g.Kdim < 16) fwd_regs_launch<1, PC, 1>(g, a, st);
  else if (ar == 1) fwd_regs_launch<2, PC, 1>(g, a, st);
  else if (ksn <= 4) fwd_regs_launch<4, PC, 0>(g, a, st);
  else if (ksn <= 8) fwd_regs_launch<8, PC, 0>(g, a, st);
  else if (ksn <= 12) fwd_regs_launch<12, PC, 0>(g, a, st);
  else fwd_regs_launch<16, PC, 0>(g, a, st);
}

// -1 outside the kernel's limits (fwd_regs_lds), nothing launched.
static int fwd_regs(const ConvGeom &g, FwdRegs a, PoolStatsOut *stats, hipStream_t st) {
  a.lds = fwd_regs_lds(g);
  if (a.lds == 0) return -1;
  const int pc = a.pc;
  const bool win3 = a.ph > 1 || a.pw > 1;
  if (win3) {
    a.pw3.ph = a.ph; a.pw3.pw = a.pw; a.pw3.pc = pc;
    a.pw3.oh2 = g.oh / a.ph;
    a.pw3.OP = (g.oh / a.ph) * (g.ow / a.pw);
    a.pw3.div_OP = FastDiv((uint32_t)a.pw3.OP);
    a.pw3.div_oh2 = FastDiv((uint32_t)a.pw3.oh2);
  }
  // 16-B Y stores; streaming ones (kYNt) beside a pool only
  const bool aligned = ((uintptr_t)a.out % 16 == 0) && (a.os % 4 == 0);
  a.vec_ok = aligned ? (pc ? 1 | kYNt : 1) : 0;
  a.clk = phase_timing();
  const int ar = fwd_arith(g, family(kFamFwdX6));
  a.grid = frame_grid(g, ar ? 2 : fwd_regs_blocks_per_cu(a.lds));
  // the register-pooled-only form: pooled output only, pc 4, G = 128 and
  // exactly 12 position tiles, so each of the 4 waves has all 3 (the form
  // runs every item unfiltered: with 9-11 tiles a wave's third tile would
  // pool and take statistics from registers no gather wrote)
  const int ntile = (g.P + 31) / 32;
  a.rp = a.out == nullptr && pc == 4 && !win3 && g.G == 128 && ntile == 4 * 3 && ar == 2 &&
         a.lds + 8 * 4 <= (size_t)kFrameLdsMax;
  // the register-pooled kernel also gives the pooled output's max |value|
  // bits per frame and per column (stats, when the caller passes room)
  if (a.rp && stats && stats->partials &&
      stats->partial_words >= ((size_t)a.grid * (g.G / pc) * g.P + 3) / 4 &&
      (size_t)a.grid * 256 >= (size_t)(g.G / pc) * g.P) {
    a.rps.rowmax = stats->rowmax;
    a.rps.partials = stats->partials;
    a.rps.colmax = stats->colmax;
  }
  uint32_t *pcol = a.rps.partials;
  if (pc == 0) fwd_regs_ks<0>(g, a, ar, st);
  else if (win3 && a.ph == 3 && a.pw == 1 && pc == 4) fwd_regs_ks<-3>(g, a, ar, st);
  else if (win3) fwd_regs_ks<-1>(g, a, ar, st);
  else if (pc == 2) fwd_regs_ks<2>(g, a, ar, st);
  else if (pc == 4) fwd_regs_ks<4>(g, a, ar, st);
  else fwd_regs_ks<8>(g, a, ar, st);
  if (pcol) {
    PoolColDeferred d;
    d.pcol = reinterpret_cast<const uint8_t *>(pcol);
    d.nblk = (int)a.grid;
    d.npool = g.G / pc * g.P;
    d.P = a.pool;
    d.ps = a.ps;
    d.R = g.R;
    d.vec = a.ps % 4 == 0 && (uintptr_t)a.pool % 16 == 0;
    d.rowblk = stats->rowmax;
    d.colblk = stats->colmax;
    d.pending = 1;
    stats->produced = 1;
    if (PoolColDeferred *req = kcnn_pool_defer_current())
      *req = d;  // the consumer's statistics launches take it
    else return kcnn_pool_cols_complete(&d, reinterpret_cast<kcnn_stream_t>(st));
  }
  return (int)hipGetLastError();
}

// One filter chunk of kcnn_conv_fwd_frame: the register kernel, else the
// slab kernel, else conv_fwd_frame_kernel, each where its LDS plan fits.
static int fwd_frame_chunk(const ConvGeom &g, const float *X, int xs, const float *K, int ks,
                           const float *bias, float *out, int os, hipStream_t st) {
  FwdRegs a;
  a.X = X; a.xs = xs; a.K = K; a.ks = ks; a.bias = bias; a.out = out; a.os = os;
  const int rc = fwd_regs(g, a, nullptr, st);
  if (rc >= 0) return rc;
  const int Kpad = (g.Kdim + 1) & ~1;
  {
    // slab-streamed: T [32][P] staged in LDS, written as whole 16-B lines
    const int Gp = (g.G + 31) & ~31;
    const size_t lds = (size_t)align16(Kpad * 8) + (size_t)((32 * g.P + 3) & ~3) * 4 +
                       (size_t)Kpad * Gp * 4 + (size_t)g.C * g.HW * 4;
    if (lds <= (size_t)kFrameLdsMax) {
      const int vec_ok = ((uintptr_t)out % 16 == 0) && (os % 4 == 0);
      hipLaunchKernelGGL(conv_fwd_slab_kernel, dim3(frame_grid(g, 2)), dim3(256),
                         lds, st, g, X, xs, K, ks, bias, out, os, Kpad, Gp, vec_ok);
      return (int)hipGetLastError();
    }
  }
  const int ngb = g.G > 64 ? 4 : (g.G > 32 ? 2 : 1);
  const int Gp = (g.G + 32 * ngb - 1) / (32 * ngb) * (32 * ngb);
  const size_t lds = fwd_lds(g, Kpad, Gp);
  if (lds > (size_t)kFrameLdsMax) return -1;
  const unsigned grid = frame_grid(g, 4);
  if (ngb == 4) {
    hipLaunchKernelGGL(conv_fwd_frame_kernel<4>, dim3(grid), dim3(256), lds, st,
                       g, X, xs, K, ks, bias, out, os, Kpad, Gp);
  } else if (ngb == 2) {
    hipLaunchKernelGGL(conv_fwd_frame_kernel<2>, dim3(grid), dim3(256), lds, st,
                       g, X, xs, K, ks, bias, out, os, Kpad, Gp);
  } else {
    hipLaunchKernelGGL(conv_fwd_frame_kernel<1>, dim3(grid), dim3(256), lds, st,
                       g, X, xs, K, ks, bias, out, os, Kpad, Gp);
  }
  return (int)hipGetLastError();
}

int kcnn_conv_fwd_frame(const ConvGeom &g, const float *X, int xs,
                        const float *K, int ks, const float *bias, float *out,
                        int os, hipStream_t st) {
  if (!kcnn::in_frame_range(g)) return -1;
  const auto chunk = [&](const ConvGeom &gc, int g0) {
    return fwd_frame_chunk(gc, X, xs, K + g0, ks, bias ? bias + g0 : nullptr,
                           out + (int64_t)g0 * g.P, os, st);
  };
  if (g.G > 128 && g.G % 32 == 0 && g.Kdim <= 32) return for_filter_chunks(g, chunk);
  return chunk(g, 0);
}

// Forward + max pool (ph x pw x pc; 1 x 1 x pc: channel-only, 8-bit mask,
// else a 16-bit mask with ms in mask elements) in one pass; -1 when the
// geometry is outside the register-resident kernel's limits.
int kcnn_conv_fwd_frame_pool(const ConvGeom &g, const float *X, int xs,
                             const float *K, int ks, const float *bias,
                             float *out, int os, float *pool, int ps,
                             unsigned char *mask, int ms, int pc,
                             hipStream_t st, int ph, int pw, PoolStatsOut *stats) {
  if (stats) stats->produced = 0;
  const bool win3 = ph > 1 || pw > 1;
  if (win3) {
    if (pc < 1 || 32 % pc != 0 || ph * pw * pc > 16 || g.oh % ph != 0 || g.ow % pw != 0)
      return -1;
  } else if (!(pc == 2 || pc == 4 || pc == 8)) {
    return -1;
  }
  if (g.G % pc != 0) return -1;
  const int OP = win3 ? (g.oh / ph) * (g.ow / pw) : g.P;  // pooled positions per map
  // filter chunks (pool groups never straddle them) give no statistics
  const bool chunked = g.G > 128 && g.G % 32 == 0;
  const auto chunk = [&](const ConvGeom &gc, int g0) {
    const int64_t pofs = (int64_t)(g0 / pc) * OP;
    FwdRegs a;
    a.X = X; a.xs = xs; a.K = K + g0; a.ks = ks;
    a.bias = bias ? bias + g0 : nullptr;
    a.out = out ? out + (int64_t)g0 * g.P : nullptr; a.os = os;
    a.pool = pool + pofs; a.ps = ps;
    a.mask = win3 ? reinterpret_cast<unsigned char *>(
                        reinterpret_cast<unsigned short *>(mask) + pofs)
                  : mask + pofs;
    a.ms = ms; a.pc = pc; a.ph = ph; a.pw = pw;
    return fwd_regs(gc, a, chunked ? nullptr : stats, st);
  };
  return chunked ? for_filter_chunks(g, chunk) : chunk(g, 0);
}

int kcnn_pool_cols_complete(PoolColDeferred *d, kcnn_stream_t stream) {
  if (!d || !d->pending) return 0;
  d->pending = 0;
  hipStream_t st = kcnn::as_stream(stream);
  const int ncq = d->npool % 4 == 0 ? d->npool / 4 : d->npool;  // pool_colmax_kernel's threads
  hipLaunchKernelGGL(pool_colmax_kernel,
                     dim3((ncq + 255) / 256, (d->nblk + COLMAX_ROWS - 1) / COLMAX_ROWS),
                     dim3(256), 0, st, d->pcol, d->nblk, d->npool, d->colblk);
  // 256 blocks (c2: 41 suspect frames of 4096, at most one each); a pass
  // of 4096 frames gives a block at most 4096 / 256 = CNT_LIST of them
  const int cgrid = std::min(d->R, 256);
  hipLaunchKernelGGL(pool_count_kernel, dim3(cgrid), dim3(256), 0, st, d->P, d->ps, d->R,
                     d->npool, d->vec, d->rowblk, d->colblk);
  return (int)hipGetLastError();
}

size_t kcnn_pool_stats_partial_words(const ConvGeom &g, int pc) {
  // frame_grid(g, 2) workgroups (the f16x3 register kernel) x pooled columns
  // exponent bytes of the maxima
  return pc > 0 ? ((size_t)frame_grid(g, 2) * (g.G / pc) * g.P + 3) / 4 : 0;
}
