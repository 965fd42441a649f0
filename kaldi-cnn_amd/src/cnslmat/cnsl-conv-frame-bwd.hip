// cnslmat/cnsl-conv-frame-bwd.hip -- the frame-resident convolution backward
// in fp32: the fused backward (data and weight gradient from one pass over
// dY) and the separate frame dgrad / wgrad, for the layers of
// cnsl-conv-frame.hip's forward (K = kh*kw*C <= 32, HBM-bound).
//
// One workgroup walks frames (grid-stride over rows); per frame:
//   dgrad    Z[p][k] = sum_g dY[g][p] W[k][g]   (a plain GEMM: K = G, N = K)
//            with dY read straight from HBM as the MFMA A operand (lanes along
//            p: coalesced, no LDS), Z kept in LDS, then the col2im
//            dX[c][q] = sum_taps Z[q - tap][tap, c] from LDS.  No padded dY,
//            no flipped kernel, no im2col matrix (the reference's flip branch
//            moves ~30x the bytes).
//   wgrad    gW[k][g] = sum_{n,p} X[c][p + off_k] dY[g][p]; each wave owns a
//            32-wide g block, stages its dY tile through LDS (transpose), and
//            gathers the im2col operand from the LDS-resident X map.  Row
//            K of the A operand is all ones, so the bias gradient sum_p dY
//            falls out of the same MFMAs.  Per-workgroup partials are reduced
//            in a fixed order (cnsl-conv-reduce.hip: deterministic).
#include <hip/hip_runtime.h>

#include <type_traits>
#include <stdint.h>

#include "conv-frame-dev.h"
#include "conv-geom.h"
#include "conv-update.h"
#include "x6-util.h"

using namespace kcnn;

namespace {

constexpr int kBwdLdsMax = 160 * 1024;  // the fused backward: one workgroup per CU
constexpr int ZS = 33;  // padded row stride (floats) of the LDS Z / dY tiles

// ---------------------------------------------------------------------------
// Fused backward: data AND weight gradient from a single pass over dY.
// dY of one frame is streamed in 32-map slabs (32 x P floats, contiguous and
// 16-B aligned in HBM): linear dwordx4 loads, prefetched into registers one
// slab ahead, committed to LDS.  From the LDS slab
//   dgrad: Z[p][k] += sum_{g in slab} dY[g][p] W[k][g]   (lanes along p)
//   wgrad: gW[k][g] += sum_p X[k-tap](p) dY[g][p]         (lanes along g;
//          row K of the A operand = 1 gives the bias gradient)
// Each wave owns position tiles {wave, wave+4, wave+8} for both products, so
// no cross-wave reduction is needed; Z is col2im'ed from LDS per frame and
// the weight-gradient partials are reduced across workgroups in fixed order.
constexpr int BWD_THREADS = 512;  // 8 waves, one workgroup per CU
constexpr int BWD_WAVES = BWD_THREADS / 64;
constexpr int BWD_MAXT = 2;   // position tiles per wave (P <= 512)
constexpr int BWD_MAXV = 8;   // float4 prefetch registers per thread
constexpr int BWD_MAXX = 4;   // X prefetch registers per thread (C*H*W <= 2048)

// slab buffer: a 32 x SP slab, later Z [P][ZZ] and the wave-partial sums
__host__ __device__ inline int bwd_sd_floats(int SP) {
  const int slab = (32 * SP + 3) & ~3;
  return slab > BWD_WAVES * 1024 ? slab : BWD_WAVES * 1024;
}

template <int NCH, bool DX>
__global__ __launch_bounds__(BWD_THREADS, 1) void conv_bwd_frame_kernel(
    ConvGeom g, const float *__restrict__ X, int xs,
    const float *__restrict__ dY, int dys, const float *__restrict__ K, int ks,
    float *__restrict__ dX, int dxs, float *__restrict__ ws_part, int ZZ,
    int SP, FastDiv div_hp, FastDiv div_hpwp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *Wt = reinterpret_cast<float *>(smem);         // [NCH*32][32]
  float *Sd = Wt + NCH * 32 * 32;                      // [32][SP]  (16-B aligned)
  float *Xs = Sd + bwd_sd_floats(SP) + 32;             // [C][Wp][Hp] + {1}
  int *qtab = reinterpret_cast<int *>(Xs + ((g.C * (g.H + 2 * g.pad_h) *
                                              (g.W + 2 * g.pad_w) + 4) & ~3));
  float *Zs = Sd;                                       // [P][ZZ] after the slabs
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = lane & 31, h = lane >> 5;
  if (DX)  // K is only read by the data gradient (the gradient-only pass has K == NULL)
    for (int e = tid; e < NCH * 32 * 32; e += BWD_THREADS) {
      const int gg = e >> 5, k = e & 31;
      Wt[e] = (gg < g.G && k < g.Kdim) ? K[(int64_t)k * ks + gg] : 0.0f;
    }
  // wgrad A operand of this lane = row l of the [Kdim+1 x P] im2col tile,
  // read as Xs[min(abase + qmul * qtab[p], CHWp)] (byte offsets):
  //   conv row l < Kdim: abase = its tap offset in the zero-padded frame
  //     map, qtab[p] = px*Hp + py (no bounds tests);
  //   row Kdim and above: the constant slot Xs[CHWp] = 1 (row Kdim is the
  //     bias gradient, rows above are never stored);
  //   p >= P: qtab = huge, clamps to the constant slot, and B is masked to
  //     +0, so padded positions add exact zeros (finite * +0).
  const int Hp = g.H + 2 * g.pad_h, Wp = g.W + 2 * g.pad_w;
  const int CHWp = g.C * Hp * Wp;
  int abase = CHWp * 4, qmul = 0;
  if (l < g.Kdim) {
    uint32_t c, r, qx, qy;
    g.div_khkw.divmod((uint32_t)l, c, r);
    g.div_kh.divmod(r, qx, qy);
    abase = ((int)c * Hp * Wp + (int)qx * Hp + (int)qy) * 4;
    qmul = 1;
  }
  if (tid == 0) Xs[CHWp] = 1.0f;
  for (int p = tid; p < ((g.P + 31) & ~31); p += BWD_THREADS) {
    uint32_t px, py;
    g.div_oh.divmod((uint32_t)p, px, py);
    qtab[p] = p < g.P ? ((int)px * Hp + (int)py) * 4 : 0x3fffffff;
  }
  const uint32_t amax = (uint32_t)CHWp * 4;
  const char *Xb = reinterpret_cast<const char *>(Xs);
  const bool unpadded = g.pad_h == 0 && g.pad_w == 0;
  const int CHW = g.C * g.HW;
  const int ntile = (g.P + 31) >> 5;
  const int nv4 = 8 * g.P;  // float4 per slab (32 * P / 4)

  floatx16 wacc[NCH];
#pragma unroll
  for (int c = 0; c < NCH; c++) wacc[c] = zero16();
  // one slab in flight per thread: BWD_MAXV float4 registers (scalars, so
  // they stay in VGPRs), 16-B aligned linear loads of the 32 x P slab
  float4 p0, p1, p2, p3, p4, p5, p6, p7;
#define KCNN_SLAB_REGS(X) X(0, p0) X(1, p1) X(2, p2) X(3, p3) X(4, p4) X(5, p5) \
  X(6, p6) X(7, p7)
#define KCNN_SLAB_LOAD(i, r) \
  if (tid + BWD_THREADS * (i) < nv4) r = src4[tid + BWD_THREADS * (i)];
#define KCNN_SLAB_STORE(i, r) \
  if (tid + BWD_THREADS * (i) < nv4) dst4[tid + BWD_THREADS * (i)] = r;
  float4 *dst4 = reinterpret_cast<float4 *>(Sd);
  if (blockIdx.x < (unsigned)g.R) {
    const float4 *src4 = reinterpret_cast<const float4 *>(dY + (int64_t)blockIdx.x * dys);
    KCNN_SLAB_REGS(KCNN_SLAB_LOAD)
  }
  for (int n = blockIdx.x; n < g.R; n += gridDim.x) {
    __syncthreads();  // previous frame's Zs / Xs reads are done
    const float *xr = X + (int64_t)n * xs;
    if (unpadded) {
      for (int e = tid; e < CHW; e += BWD_THREADS) Xs[e] = xr[e];
    } else {
      for (int e = tid; e < CHWp; e += BWD_THREADS) {
        uint32_t c, r, wp, hp;
        div_hpwp.divmod((uint32_t)e, c, r);
        div_hp.divmod(r, wp, hp);
        const int wi = (int)wp - g.pad_w, hi = (int)hp - g.pad_h;
        Xs[e] = ((unsigned)wi < (unsigned)g.W && (unsigned)hi < (unsigned)g.H)
                    ? xr[(int)c * g.HW + wi * g.H + hi] : 0.0f;
      }
    }
    floatx16 zacc[BWD_MAXT];
#pragma unroll
    for (int t = 0; t < BWD_MAXT; t++) zacc[t] = zero16();
    // wgrad A operands of this frame (im2col values of the wave's tiles):
    // identical for every slab, so gathered once per frame into registers
    float ain[BWD_MAXT][16];
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
      KCNN_SLAB_REGS(KCNN_SLAB_STORE)
      __syncthreads();
      {
        const int nn = ch + 1 < NCH ? n : n + (int)gridDim.x;
        const int cc = ch + 1 < NCH ? ch + 1 : 0;
        if (nn < g.R) {
          const float4 *src4 = reinterpret_cast<const float4 *>(
              dY + (int64_t)nn * dys + (int64_t)cc * 32 * g.P);
          KCNN_SLAB_REGS(KCNN_SLAB_LOAD)
        }
      }
      const float *wrow = Wt + (ch * 32 + h) * 32 + l;
#pragma unroll
      for (int t = 0; t < BWD_MAXT; t++) {
        // tiles wave, wave + 8: with waves w and w + 4 sharing a SIMD, every
        // SIMD gets the same tile count (wave-uniform skip of surplus tiles)
        __builtin_amdgcn_sched_barrier(0);
        const int pt = wave + BWD_WAVES * t;
        if (pt >= ntile) continue;
        int pb = pt * 32;
        // opaque per iteration: keeps the frame-invariant operand addresses
        // of all tiles from being hoisted out of the frame loop (that would
        // pin ~150 VGPRs)
        asm volatile("" : "+s"(pb));
        const int ph = pb + h;
        if (ch == 0) {
          const int *qrow = qtab + ph;
#pragma unroll
          for (int s = 0; s < 16; s++) {
            const uint32_t off = min((uint32_t)(abase + qmul * qrow[2 * s]), amax);
            ain[t][s] = *reinterpret_cast<const float *>(Xb + off);
          }
        }
        if (DX) {
          const int pa = pb + l < g.P ? pb + l : g.P - 1;
          const float *srow = Sd + h * SP + pa;
#pragma unroll
          for (int s = 0; s < 16; s++)
            zacc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                srow[2 * s * SP], wrow[2 * s * 32], zacc[t], 0, 0, 0);
        }
        const float *scol = Sd + l * SP + ph;
        if (pb + 32 <= g.P) {  // wave-uniform: a full tile
#pragma unroll
          for (int s = 0; s < 16; s++)
            wacc[ch] = __builtin_amdgcn_mfma_f32_32x32x2f32(ain[t][s], scol[2 * s],
                                                           wacc[ch], 0, 0, 0);
        } else {
          // B bit-masked to +0 past P (the row tail reads the next map's
          // data); A is finite there (the clamped constant slot)
#pragma unroll
          for (int s = 0; s < 16; s++) {
            const bool pin = ph + 2 * s < g.P;
            const float bv = __uint_as_float(__float_as_uint(scol[2 * s]) &
                                             (pin ? 0xffffffffu : 0u));
            wacc[ch] = __builtin_amdgcn_mfma_f32_32x32x2f32(ain[t][s], bv, wacc[ch], 0, 0, 0);
          }
        }
      }
      __syncthreads();  // slab consumed
    }
    if (DX) {
#pragma unroll
      for (int t = 0; t < BWD_MAXT; t++) {
        const int pt = wave + BWD_WAVES * t;
        if (pt >= ntile) continue;
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int pl = pt * 32 + mfma32_row(r, lane);
          if (pl < g.P && l < g.Kdim) Zs[pl * ZZ + l] = zacc[t][r];
        }
      }
      __syncthreads();
      float *dxr = dX + (int64_t)n * dxs;
      const int khkw = g.kh * g.kw;
      for (int e = tid; e < CHW; e += BWD_THREADS) {
        uint32_t c, q, wi, hi;
        g.div_HW.divmod((uint32_t)e, c, q);
        g.div_H.divmod(q, wi, hi);
        float sum = 0.0f;
        for (int kxx = 0; kxx < g.kw; kxx++) {
          const int px = (int)wi + g.pad_w - kxx;
          if ((unsigned)px >= (unsigned)g.ow) continue;
          const float *zr = Zs + (int64_t)(px * g.oh) * ZZ + (int)c * khkw + kxx * g.kh;
          for (int kyy = 0; kyy < g.kh; kyy++) {
            const int py = (int)hi + g.pad_h - kyy;
            if ((unsigned)py < (unsigned)g.oh) sum += zr[py * ZZ + kyy];
          }
        }
        dxr[e] = sum;
      }
    }
  }
  // sum the waves' partials (each covers its own position tiles) through
  // LDS in a fixed wave order, then one [Kdim+1][G] partial per workgroup
  const int E = (g.Kdim + 1) * g.G;
  float *dst = ws_part + (int64_t)blockIdx.x * E;
  float *red = Sd;  // [BWD_WAVES][32 * 32]; 32 KB <= the slab buffer
#pragma unroll
  for (int ch = 0; ch < NCH; ch++) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; r++)
      red[wave * 1024 + mfma32_row(r, lane) * 32 + l] = wacc[ch][r];
    __syncthreads();
    for (int e = tid; e < 1024; e += BWD_THREADS) {
      const int i = e >> 5, j = e & 31;
      if (i > g.Kdim) continue;
      float sum = 0.0f;
#pragma unroll
      for (int w = 0; w < BWD_WAVES; w++) sum += red[w * 1024 + e];
      dst[i * g.G + ch * 32 + j] = sum;
    }
  }
}
#undef KCNN_SLAB_LOAD
#undef KCNN_SLAB_STORE
#undef KCNN_SLAB_REGS

// ---------------------------------------------------------------------------
// Fused backward, variant 3: dY slabs reach LDS by LDS-DMA
// (global_load_lds_dwordx4, 1 KiB per wave-instruction, no VGPRs), double
// buffered, one slab ahead; one barrier per slab.  From the slab in LDS the
// waves run the data gradient (owner waves of each position tile: Z lives
// in their registers for the whole frame) and the weight gradient (tiles
// handed out by the host so every wave carries the same number of 16-MFMA
// chunks; A operands = the frame's im2col values, gathered once per frame
// into the registers of the wave that uses them).
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) void glob_void_t;

__host__ __device__ inline int bwd_dma_buf_floats(int P) {
  return ((32 * P * 4 + 1023) & ~1023) / 4;  // whole 1-KiB DMA chunks
}
// both slab buffers; also holds Z [P][Kdim|1] (< 32 P) and the final
// [8 waves][32 x 32] reduction
__host__ __device__ inline int bwd_dma_sd_floats(int P) {
  const int two = 2 * bwd_dma_buf_floats(P);
  return two > BWD_WAVES * 1024 ? two : BWD_WAVES * 1024;
}

//
// PCM > 0: dY is not in HBM.  It is the Backprop of a channel-only Maxpool
// (1 x 1 x PCM) from its routing mask: dY[g][p] = bit g % PCM of
// mask[g / PCM][p] ? dP[g / PCM][p] : 0 (hipF_maxpool_backprop_mask).  dY /
// dys then point at dP, pmask / pms at the mask, and each slab is built in
// LDS from its 32 / PCM rows of dP and mask, loaded into registers at the
// start of the phase before it and expanded after that phase's MFMA chains.
template <int NCH, bool DX, bool WG, int PCM>
__global__ __launch_bounds__(BWD_THREADS, 1) void conv_bwd_dma_kernel(
    ConvGeom g, const float *__restrict__ X, int xs,
    const float *__restrict__ dY, int dys, const float *__restrict__ K, int ks,
    float *__restrict__ dX, int dxs, float *__restrict__ ws_part, int ZZ,
    unsigned long long wg0, unsigned long long wg1, int zsep, int dx_acc, int clk,
    const unsigned char *__restrict__ pmask, int pms) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int P = g.P;
  const int BUF = bwd_dma_buf_floats(P);
  float *Wt = reinterpret_cast<float *>(smem);         // [NCH*32][32]
  float *Sd0 = Wt + NCH * 32 * 32;                     // [32][P] x 2 buffers
  float *Xs = Sd0 + bwd_dma_sd_floats(P);              // [C][Wp][Hp] + {1}
  int *qtab = reinterpret_cast<int *>(Xs + ((g.C * (g.H + 2 * g.pad_h) *
                                              (g.W + 2 * g.pad_w) + 4) & ~3));
  // zsep: Z [P][ZZ] has its own buffer, so frame n's col2im runs inside frame
  // n+1's slab phases (next to the other waves' MFMAs) instead of in a
  // barrier-bounded tail; else Z reuses the last slab's buffer
  float *Zsep = reinterpret_cast<float *>(qtab + ((P + 31) & ~31));
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = lane & 31;
  if (DX)  // K and X are only read by the pass that needs them
    for (int e = tid; e < NCH * 32 * 32; e += BWD_THREADS) {
      const int gg = e >> 5, k = e & 31;
      Wt[e] = (gg < g.G && k < g.Kdim) ? K[(int64_t)k * ks + gg] : 0.0f;
    }
  const int Hp = g.H + 2 * g.pad_h, Wp = g.W + 2 * g.pad_w;
  const int CHWp = g.C * Hp * Wp;
  int abase = CHWp * 4, qmul = 0;
  if (l < g.Kdim) {
    uint32_t c, r, qx, qy;
    g.div_khkw.divmod((uint32_t)l, c, r);
    g.div_kh.divmod(r, qx, qy);
    abase = ((int)c * Hp * Wp + (int)qx * Hp + (int)qy) * 4;
    qmul = 1;
  }
  for (int e = tid; e < CHWp; e += BWD_THREADS) Xs[e] = 0.0f;  // padded border
  if (tid == 0) Xs[CHWp] = 1.0f;
  for (int p = tid; p < ((P + 31) & ~31); p += BWD_THREADS) {
    uint32_t px, py;
    g.div_oh.divmod((uint32_t)p, px, py);
    qtab[p] = p < P ? ((int)px * Hp + (int)py) * 4 : 0x3fffffff;
  }
  const uint32_t amax = (uint32_t)CHWp * 4;
  const char *Xb = reinterpret_cast<const char *>(Xs);
  const bool unpadded = g.pad_h == 0 && g.pad_w == 0;
  const int CHW = g.C * g.HW;
  const int ntile = (P + 31) >> 5;
  const int nchunk = BUF / 256;  // 1-KiB chunks per slab
  const int slab = 32 * P;

  // LDS-DMA of slab (n, c) into buffer b: wave w moves chunks w, w+8, ...
  // by buffer_load ... lds -- the chunk offset is a scalar (soffset), the
  // lane's 16 B a constant voffset, so the issue loop costs no VALU work.
  // The descriptor spans the frame's row: a last chunk running past the
  // row reads zeros (hardware range check); past the slab it reads the
  // next slab's first values into an LDS tail that is never read.
  const uint32_t row_bytes = (uint32_t)g.G * (uint32_t)P * 4u;
  auto dma_slab = [&](int n, int c, int b, int ln) {
    const float *base = dY + (int64_t)n * dys;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void *)base, (short)0, (int)row_bytes, 0x00020000);
    float *dst = Sd0 + b * BUF;
    for (int q = wave; q < nchunk; q += BWD_WAVES)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t *)(dst + q * 256), 16,
                                               (uint32_t)ln * 16u,
                                               (uint32_t)(c * slab + q * 256) * 4u, 0, 0);
  };

  // PCM: a slab's 32 / PCM rows of dP and mask (contiguous in the pooled
  // row).  Thread t < P stages position t of every row (P <= 512), so its
  // slab offsets are j * PCM * P + t: no per-element index arithmetic.
  constexpr int NJ = PCM > 0 ? 32 / PCM : 1;
  float pv[NJ];
  unsigned pm[(NJ + 3) / 4];  // mask bytes, 4 to a register
  auto stage_load = [&](int n, int c, int tt) {
    if (tt >= P) return;
    const int64_t off = (int64_t)c * NJ * P + tt;
    const float *src = dY + (int64_t)n * dys + off;
    const unsigned char *msrc = pmask + (int64_t)n * pms + off;
#pragma unroll
    for (int i = 0; i < (NJ + 3) / 4; i++) pm[i] = 0;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      pv[j] = src[j * P];
      pm[j / 4] |= (unsigned)msrc[j * P] << (8 * (j % 4));
    }
  };
  auto stage_commit = [&](int b, int tt) {
    if (tt >= P) return;
    float *d = Sd0 + b * BUF + tt;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      const unsigned v = __float_as_uint(pv[j]);
#pragma unroll
      for (int c = 0; c < PCM; c++) {
        // bit c of the element's mask byte, sign-extended to 0 / ~0
        const int sel = __builtin_amdgcn_sbfe((int)pm[j / 4], 8 * (j % 4) + c, 1);
        d[(j * PCM + c) * P] = __uint_as_float(v & (unsigned)sel);
      }
    }
  };
  floatx16 wacc[NCH];
#pragma unroll
  for (int c = 0; c < NCH; c++) wacc[c] = zero16();
  float xv[BWD_MAXX];
#define KCNN_XLOAD(nn)                                                               \
  _Pragma("unroll") for (int i = 0; i < BWD_MAXX; i++)                              \
    if (WG && tid + BWD_THREADS * i < CHW)                                         \
      xv[i] = X[(int64_t)(nn) * xs + tid + BWD_THREADS * i];
  // X values (in xv) into the padded frame buffer
#define KCNN_XCOMMIT()                                                               \
  _Pragma("unroll") for (int i = 0; i < BWD_MAXX; i++) {                            \
    const int e = tid + BWD_THREADS * i;                                             \
    if (WG && e < CHW) {                                                             \
      int slot = e;                                                                  \
      if (!unpadded) {                                                               \
        uint32_t c, q, wi, hi;                                                       \
        g.div_HW.divmod((uint32_t)e, c, q);                                          \
        g.div_H.divmod(q, wi, hi);                                                   \
        slot = (int)c * Hp * Wp + ((int)wi + g.pad_w) * Hp + (int)hi + g.pad_h;      \
      }                                                                              \
      Xs[slot] = xv[i];                                                              \
    }                                                                                \
  }
  // col2im: dX[nn][e] = sum over the valid taps (kx, ky) of
  // Z[(px*oh + py)*ZZ + c*kh*kw + kx*kh + ky], px = wi + pad_w - kx,
  // py = hi + pad_h - ky.  The output elements of a thread are the same in
  // every frame (e = tid + 512 i), so their Z base offset and valid tap
  // ranges are computed once; per tap that leaves an address subtract, a
  // range test, the read and the add (VALU work is not hidden behind the
  // MFMAs of this kernel: it executes on the same SIMDs, serially).
  const int khkw = g.kh * g.kw;
  const int zax = g.oh * ZZ - g.kh, zby = ZZ - 1;  // Z offset per kx / ky step
  int c2b[BWD_MAXX], c2r[BWD_MAXX];
#pragma unroll
  for (int i = 0; i < BWD_MAXX; i++) {
    const int e = tid + BWD_THREADS * i;
    c2b[i] = 0;
    c2r[i] = (int)0xff000000u;  // no taps (nx = -1)
    if (DX && e < CHW) {
      uint32_t c, q, wi, hi;
      g.div_HW.divmod((uint32_t)e, c, q);
      g.div_H.divmod(q, wi, hi);
      const int ty = (int)hi + g.pad_h, tx = (int)wi + g.pad_w;
      c2b[i] = (tx * g.oh + ty) * ZZ + (int)c * khkw;
      const int ylo = max(0, ty - g.oh + 1), yhi = min(g.kh - 1, ty);
      const int xlo = max(0, tx - g.ow + 1), xhi = min(g.kw - 1, tx);
      if (ylo <= yhi && xlo <= xhi)
        c2r[i] = ylo | (yhi - ylo) << 8 | xlo << 16 | (xhi - xlo) << 24;
    }
  }
  auto col2im = [&](const float *Zs, int nn, int i, int tt) {
    const int e = tt + BWD_THREADS * i;
    if (e >= CHW) return;
    const int rg = c2r[i];
    const int ylo = rg & 255, ny = (rg >> 8) & 255, xlo = (rg >> 16) & 255, nx = rg >> 24;
    float sum = 0.0f;
    for (int kx = xlo; kx <= xlo + nx; kx++) {  // kw = 1: one pass
      const int zk = c2b[i] - kx * zax;
      for (int k0 = 0; k0 < g.kh; k0 += 8) {
        // the 8 taps' reads first (one wait), then the masked sum.  A tap
        // outside the map reads another position's Z (or, off the LDS
        // allocation, 0) and is dropped by the mask: no address select
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = Zs[zk - (k0 + u) * zby];
#pragma unroll
        for (int u = 0; u < 8; u++)
          sum += (unsigned)(k0 + u - ylo) <= (unsigned)ny ? v[u] : 0.0f;
        __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);  // the reads
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    float *d = dX + (int64_t)nn * dxs + e;
    *d = dx_acc ? *d + sum : sum;  // dx_acc: a later filter chunk (G > 128)
  };
  // deferred col2im: pieces in phases 0 .. npiece-1 of the next frame, all
  // before that frame's last slab barrier (Z is rewritten after it)
  const int npiece = NCH > 1 ? NCH - 1 : 1;
  int cur = 0, nprev = -1;
  KCNN_TMARKS(7)  // per-phase totals of block 0 (clk != 0)
  if (blockIdx.x < (unsigned)g.R) {
    if constexpr (PCM > 0) {
      stage_load(blockIdx.x, 0, tid);
      stage_commit(0, tid);
    } else {
      dma_slab(blockIdx.x, 0, 0, lane);
    }
    KCNN_XLOAD(blockIdx.x)
  }
  __syncthreads();  // zeroed border before the first commit
  if (blockIdx.x < (unsigned)g.R) { KCNN_XCOMMIT() }
  for (int n = blockIdx.x; n < g.R; n += gridDim.x) {
    // lane ids made opaque per frame (see conv_fwd_regs_kernel, cnsl-conv-frame.hip)
    int tid_f = tid;
    asm volatile("" : "+v"(tid_f));
    const int lane_f = tid_f & 63, l_f = lane_f & 31, h_f = lane_f >> 5;
    floatx16 zacc[BWD_MAXT];
#pragma unroll
    for (int t = 0; t < BWD_MAXT; t++) zacc[t] = zero16();
    float ain[2][16];
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
      // slab (n, ch) landed; the other buffer's readers are done.  The
      // explicit vmcnt(0): an LDS-DMA writes LDS, not VGPRs, so no wait of
      // the compiler's covers another wave's reads of it
      KCNN_TMARK(6)
      x6::publish_dma();
      KCNN_TMARK(0)
      {
        const int nn = ch + 1 < NCH ? n : n + (int)gridDim.x;
        const int cc = ch + 1 < NCH ? ch + 1 : 0;
        if (nn < g.R) {
          if constexpr (PCM > 0) stage_load(nn, cc, tid_f);
          else dma_slab(nn, cc, cur ^ 1, lane_f);
          if (ch + 1 == NCH) { KCNN_XLOAD(nn) }
        }
      }
      if (DX && zsep && nprev >= 0) {
#pragma unroll
        for (int i = 0; i < BWD_MAXX; i++)
          if (i % npiece == ch) col2im(Zsep, nprev, i, tid_f);
      }
      KCNN_TMARK(1)
      const float *Sd = Sd0 + cur * BUF;
      const float *wrow = Wt + (ch * 32 + h_f) * 32 + l_f;
      if (DX && wave < ntile) {
        // Z[p][k] += dY[g][p] W[k][g] on the wave's own tiles (wave, wave +
        // 8): the W operand of this slab is read once and shared by both
        // tiles' chains; operand reads are all issued before the chains
        float db[16], da0[16];
#pragma unroll
        for (int s = 0; s < 16; s++) db[s] = wrow[2 * s * 32];
        int pb0 = wave * 32;
        asm volatile("" : "+s"(pb0));
        const float *srow0 = Sd + h_f * P + (pb0 + l_f < P ? pb0 + l_f : P - 1);
#pragma unroll
        for (int s = 0; s < 16; s++) da0[s] = srow0[2 * s * P];
#pragma unroll
        for (int s = 0; s < 16; s++)
          zacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(da0[s], db[s], zacc[0], 0, 0, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 24, 0);  // operand reads
        __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);  // MFMAs
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 1; t < BWD_MAXT; t++) {
          const int pt = wave + BWD_WAVES * t;
          if (pt >= ntile) break;  // wave-uniform; the chain below is in place
          int pb = pt * 32;
          asm volatile("" : "+s"(pb));
          const float *srow = Sd + h_f * P + (pb + l_f < P ? pb + l_f : P - 1);
          float da[16];
#pragma unroll
          for (int s = 0; s < 16; s++) da[s] = srow[2 * s * P];
#pragma unroll
          for (int s = 0; s < 16; s++)
            zacc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(da[s], db[s], zacc[t], 0, 0, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 16, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      KCNN_TMARK(2)
#pragma unroll
      for (int j = 0; j < 2; j++) {
        if (!WG) break;
        const int pt = (int)(((j ? wg1 : wg0) >> (8 * wave)) & 0xff);
        if (pt == 0xff) continue;
        int pb = pt * 32;
        asm volatile("" : "+s"(pb));
        const int ph = pb + h_f;
        if (ch == 0) {  // the frame's im2col values of this tile
          const int *qrow = qtab + ph;
#pragma unroll
          for (int s = 0; s < 16; s++) {
            const uint32_t off = min((uint32_t)(abase + qmul * qrow[2 * s]), amax);
            ain[j][s] = *reinterpret_cast<const float *>(Xb + off);
          }
        }
        const float *scol = Sd + l_f * P + ph;
        // one MFMA chain for full and partial tiles (a branch around the
        // chain makes the compiler copy the accumulator between register
        // sets, draining the MFMA pipeline at every tile); only the B
        // operand masking of the partial tile sits in a branch.  Past P a
        // row's tail reads the next map's values: bit-masked to +0.
        float wb[16];
#pragma unroll
        for (int s = 0; s < 16; s++) wb[s] = scol[2 * s];
        if (pb + 32 > P) {  // wave-uniform
          // k-step s covers positions ph + 2s, ph = pb + h: with lim =
          // P - pb - 2s (uniform) both halves are in for lim >= 2, only
          // h = 0 for lim == 1, neither below
#pragma unroll
          for (int s = 0; s < 16; s++) {
            const int lim = P - pb - 2 * s;
            if (lim <= 0 || (lim == 1 && h_f)) wb[s] = 0.0f;
          }
        }
#pragma unroll
        for (int s = 0; s < 16; s++)
          wacc[ch] = __builtin_amdgcn_mfma_f32_32x32x2f32(ain[j][s], wb[s], wacc[ch], 0, 0, 0);
      }
      if constexpr (PCM > 0) {  // the next slab, expanded into the other buffer
        const int nn = ch + 1 < NCH ? n : n + (int)gridDim.x;
        if (nn < g.R) stage_commit(cur ^ 1, tid_f);
      }
      KCNN_TMARK(3)
      if (ch + 1 < NCH) cur ^= 1;
    }
    // with one slab per frame, this frame's gather / col2im readers are
    // only fenced by a barrier here
    if (NCH == 1) __syncthreads();
    if (DX) {
      // zsep: Z's readers (the previous col2im) finished before the last slab
      // barrier; else every wave must be done with the last slab's buffer
      if (!zsep) __syncthreads();
      float *Zs = zsep ? Zsep : Sd0 + cur * BUF;
#pragma unroll
      for (int t = 0; t < BWD_MAXT; t++) {
        const int pt = wave + BWD_WAVES * t;
        if (pt >= ntile) continue;
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int pl = pt * 32 + mfma32_row(r, lane_f);
          if (pl < P && l_f < g.Kdim) Zs[pl * ZZ + l_f] = zacc[t][r];
        }
      }
      if (zsep) {
        nprev = n;
      } else {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < BWD_MAXX; i++) col2im(Zs, n, i, tid_f);
        __syncthreads();  // Zs (slab buffer) readers done before its next DMA
      }
    }
    // the next frame's X: this frame's gather (phase 0) is behind a barrier
    if (WG && n + (int)gridDim.x < g.R) { KCNN_XCOMMIT() }
    KCNN_TMARK(4)
    cur ^= 1;  // the next frame's first slab is in the other buffer
  }
  if (DX && zsep && nprev >= 0) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < BWD_MAXX; i++) col2im(Zsep, nprev, i, tid);
  }
  KCNN_TMARK(5)
#ifdef KCNN_PHASE_TIMING
  if (clk && blockIdx.x == 0 && lane == 0)
    printf("bwd3 wave %d: barrier %lld dma %lld dgrad %lld wgrad %lld tail %lld end %lld other %lld\n",
           wave, tm[0], tm[1], tm[2], tm[3], tm[4], tm[5], tm[6]);
#endif
#undef KCNN_XLOAD
#undef KCNN_XCOMMIT
  if (!WG) return;
  const int E = (g.Kdim + 1) * g.G;
  float *dst = ws_part + (int64_t)blockIdx.x * E;
  float *red = Sd0;  // [BWD_WAVES][32 * 32]; no DMA in flight any more
#pragma unroll
  for (int ch = 0; ch < NCH; ch++) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; r++)
      red[wave * 1024 + mfma32_row(r, lane) * 32 + l] = wacc[ch][r];
    __syncthreads();
    for (int e = tid; e < 1024; e += BWD_THREADS) {
      const int i = e >> 5, j = e & 31;
      if (i > g.Kdim) continue;
      float sum = 0.0f;
#pragma unroll
      for (int w = 0; w < BWD_WAVES; w++) sum += red[w * 1024 + e];
      dst[i * g.G + ch * 32 + j] = sum;
    }
  }
}

// ---------------------------------------------------------------------------
// NK = G/2 k-steps, fully unrolled: every A load of a 32-position tile is
// issued before the MFMA chain consumes it (64 x 256 B in flight per wave at
// G = 128), which is what hides HBM latency here.  Lanes past the last
// position read a clamped address; their Z rows are never stored.
template <int NK>
__global__ __launch_bounds__(256) void conv_dgrad_frame_kernel(
    ConvGeom g, const float *__restrict__ dY, int dys,
    const float *__restrict__ K, int ks, float *__restrict__ dX, int dxs,
    int ZZ) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *Wt = reinterpret_cast<float *>(smem);   // [2*NK][32]: Wt[g][k] = W[k][g]
  float *Zs = Wt + 2 * NK * 32;                  // [P][ZZ]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < 2 * NK * 32; e += 256) {
    const int gg = e >> 5, k = e & 31;
    Wt[e] = (gg < g.G && k < g.Kdim) ? K[(int64_t)k * ks + gg] : 0.0f;
  }
  const int ntile = (g.P + 31) >> 5;
  const int CHW = g.C * g.HW;
  const int khkw = g.kh * g.kw;
  const float *wcol = Wt + (lane >> 5) * 32 + (lane & 31);

  for (int n = blockIdx.x; n < g.R; n += gridDim.x) {
    __syncthreads();  // Wt ready / previous col2im done with Zs
    const float *dyr = dY + (int64_t)n * dys;
    for (int pt = wave; pt < ntile; pt += 4) {
      const int p = pt * 32 + (lane & 31);
      const int pc = p < g.P ? p : g.P - 1;
      const float *col = dyr + pc + (int64_t)(lane >> 5) * g.P;
      float a[NK];
#pragma unroll
      for (int s = 0; s < NK; s++) a[s] = col[(int64_t)(2 * s) * g.P];
      floatx16 acc = zero16();
#pragma unroll
      for (int s = 0; s < NK; s++)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], wcol[s * 64], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int pl = pt * 32 + mfma32_row(r, lane);
        if (pl < g.P && (lane & 31) < g.Kdim) Zs[pl * ZZ + (lane & 31)] = acc[r];
      }
    }
    __syncthreads();
    float *dxr = dX + (int64_t)n * dxs;
    for (int e = tid; e < CHW; e += 256) {
      uint32_t c, q, wi, hi;
      g.div_HW.divmod((uint32_t)e, c, q);
      g.div_H.divmod(q, wi, hi);
      float sum = 0.0f;
      for (int kx = 0; kx < g.kw; kx++) {
        const int px = (int)wi + g.pad_w - kx;
        if ((unsigned)px >= (unsigned)g.ow) continue;
        const float *zr = Zs + (int64_t)(px * g.oh) * ZZ + (int)c * khkw + kx * g.kh;
        for (int ky = 0; ky < g.kh; ky++) {
          const int py = (int)hi + g.pad_h - ky;
          if ((unsigned)py < (unsigned)g.oh) sum += zr[py * ZZ + ky];
        }
      }
      dxr[e] = sum;
    }
  }
}

// ---------------------------------------------------------------------------
template <int NSUP>
__global__ __launch_bounds__(256) void conv_wgrad_frame_kernel(
    ConvGeom g, const float *__restrict__ X, int xs,
    const float *__restrict__ dY, int dys, float *__restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *Ds = reinterpret_cast<float *>(smem);   // [4 waves][32][ZS]
  float *Xs = Ds + 4 * 32 * ZS;                   // [C*HW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float *myD = Ds + wave * 32 * ZS;

  // A-row of this lane: conv row j (< Kdim), the ones row (== Kdim), or pad.
  const int j = lane & 31;
  int koff = 0, kx = 0, ky = 0;
  if (j < g.Kdim) {
    uint32_t c, r, qx, qy;
    g.div_khkw.divmod((uint32_t)j, c, r);
    g.div_kh.divmod(r, qx, qy);
    koff = (int)c * g.HW;
    kx = (int)qx;
    ky = (int)qy;
  }
  const bool is_ones = (j == g.Kdim);
  const int CHW = g.C * g.HW;

  floatx16 acc[NSUP];
#pragma unroll
  for (int su = 0; su < NSUP; su++) acc[su] = zero16();

  for (int n = blockIdx.x; n < g.R; n += gridDim.x) {
    __syncthreads();
    const float *xr = X + (int64_t)n * xs;
    for (int e = tid; e < CHW; e += 256) Xs[e] = xr[e];
    __syncthreads();
    const float *dyr = dY + (int64_t)n * dys;
#pragma unroll
    for (int su = 0; su < NSUP; su++) {
      const int g0 = (su * 4 + wave) * 32;
      if (g0 >= g.G) continue;  // wave-uniform
      // dY tile rows g0 + 2i + (lane >> 5), column pc + (lane & 31); rows past
      // G or columns past P read a clamped address and are zeroed.
      const int gl0 = lane >> 5, pl0 = lane & 31;
      float nxt[16];
      auto load_tile = [&](int pc) {
        const bool pv = pc + pl0 < g.P;
        const int pcl = pv ? pc + pl0 : g.P - 1;
#pragma unroll
        for (int i = 0; i < 16; i++) {
          const int gg = g0 + 2 * i + gl0;
          const bool v = pv && gg < g.G;
          const float x = dyr[(int64_t)(v ? gg : 0) * g.P + pcl];
          nxt[i] = v ? x : 0.0f;
        }
      };
      load_tile(0);
      for (int pc = 0; pc < g.P; pc += 32) {
#pragma unroll
        for (int i = 0; i < 16; i++) myD[(2 * i + gl0) * ZS + pl0] = nxt[i];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (pc + 32 < g.P) load_tile(pc + 32);  // in flight during the MFMAs
        // im2col operand for p = pc + 2s + (lane >> 5), walked incrementally
        uint32_t px, py;
        g.div_oh.divmod((uint32_t)(pc + gl0), px, py);
        int ipx = (int)px, ipy = (int)py;
#pragma unroll 4
        for (int s = 0; s < 16; s++) {
          const int p = pc + 2 * s + gl0;
          const int xx = ipx + kx - g.pad_w, yy = ipy + ky - g.pad_h;
          const bool ok = j < g.Kdim && p < g.P && (unsigned)xx < (unsigned)g.W &&
                          (unsigned)yy < (unsigned)g.H;
          const float xv = Xs[ok ? koff + xx * g.H + yy : 0];
          const float av = ok ? xv : ((is_ones && p < g.P) ? 1.0f : 0.0f);
          const float bv = myD[(lane & 31) * ZS + 2 * s + gl0];
          acc[su] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[su], 0, 0, 0);
          ipy += 2;
          while (ipy >= g.oh) { ipy -= g.oh; ipx++; }
        }
      }
    }
  }
  // partial [Kdim + 1][G] of this workgroup
  const int E = (g.Kdim + 1) * g.G;
  float *dst = ws + (int64_t)blockIdx.x * E;
#pragma unroll
  for (int su = 0; su < NSUP; su++) {
    const int gl = (su * 4 + wave) * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int i = mfma32_row(r, lane);
      if (i <= g.Kdim && gl < g.G) dst[i * g.G + gl] = acc[su][r];
    }
  }
}

// The fp32 fused backward kernels' position limits (conv_bwd_dma_kernel and
// conv_bwd_frame_kernel: BWD_MAXT tiles per wave, BWD_MAXV slab registers).
bool bwd_fp32_positions_ok(const ConvGeom &g) {
  return g.P >= 16 && g.P <= 32 * BWD_WAVES * BWD_MAXT && 8 * g.P <= BWD_THREADS * BWD_MAXV;
}

}  // namespace

int kcnn_conv_dgrad_frame(const ConvGeom &g, const float *dY, int dys,
                          const float *K, int ks, float *dX, int dxs,
                          hipStream_t st) {
  if (g.Kdim > 32) return -1;
  if (g.G != 64 && g.G != 128) return -1;  // NK = G/2, fully unrolled
  const int ZZ = g.Kdim | 1;               // odd row stride: conflict-free col2im
  const size_t lds = ((size_t)g.G * 32 + (size_t)g.P * ZZ) * 4;
  if (lds > (size_t)kFrameLdsMax) return -1;
  if (g.G == 128)
    hipLaunchKernelGGL(conv_dgrad_frame_kernel<64>, dim3(frame_grid(g, 3)),
                       dim3(256), lds, st, g, dY, dys, K, ks, dX, dxs, ZZ);
  else
    hipLaunchKernelGGL(conv_dgrad_frame_kernel<32>, dim3(frame_grid(g, 3)),
                       dim3(256), lds, st, g, dY, dys, K, ks, dX, dxs, ZZ);
  return (int)hipGetLastError();
}

static int wgrad_frame_blocks(const ConvGeom &g) { return (int)frame_grid(g, 2); }

size_t kcnn_conv_wgrad_frame_ws(const ConvGeom &g) {
  if (g.Kdim > 31 || g.G > 256) return 0;
  const size_t lds = (size_t)(4 * 32 * ZS + g.C * g.HW) * 4;
  if (lds > (size_t)kFrameLdsMax) return 0;
  const int S = wgrad_frame_blocks(g);
  const int E = (g.Kdim + 1) * g.G;
  return (size_t)S * E * 4 + kcnn_reduce_splits_ws(S, E);
}

int kcnn_conv_wgrad_frame(const ConvGeom &g, const float *X, int xs,
                          const float *dY, int dys, float *gW, int gws,
                          float *gb, void *ws, size_t ws_bytes, hipStream_t st) {
  const size_t need = kcnn_conv_wgrad_frame_ws(g);
  if (need == 0 || ws == nullptr || ws_bytes < need) return -1;
  const int S = wgrad_frame_blocks(g);
  const int E = (g.Kdim + 1) * g.G;
  float *part = static_cast<float *>(ws);
  const size_t lds = (size_t)(4 * 32 * ZS + g.C * g.HW) * 4;
  if (g.G <= 128)
    hipLaunchKernelGGL(conv_wgrad_frame_kernel<1>, dim3(S), dim3(256), lds, st,
                       g, X, xs, dY, dys, part);
  else
    hipLaunchKernelGGL(conv_wgrad_frame_kernel<2>, dim3(S), dim3(256), lds, st,
                       g, X, xs, dY, dys, part);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  return kcnn_reduce_splits_epi(part, S, E, g.Kdim * g.G, g.G, 0, gW, gws, gb, ConvUpdateEpi{},
                                st);
}

static size_t bwd_lds(const ConvGeom &g, int SP) {
  const int NCH = g.G / 32;
  const size_t chwp = (size_t)g.C * (g.H + 2 * g.pad_h) * (g.W + 2 * g.pad_w);
  return ((size_t)NCH * 32 * 32 + (size_t)bwd_sd_floats(SP) + 32 +
          ((chwp + 4) & ~(size_t)3) + (size_t)((g.P + 31) & ~31)) * 4;
}

static int bwd_sp(const ConvGeom &g) { return g.P; }  // P odd: conflict-free slab reads

size_t kcnn_conv_bwd_frame_ws(const ConvGeom &g) {
  if (g.G > 128 && g.G % 32 == 0) {  // chunks of 128 filters share the workspace
    ConvGeom gc = g;
    gc.G = 128;
    return kcnn_conv_bwd_frame_ws(gc);
  }
  if (!kcnn::bwd_chunk_shape_ok(g)) return 0;
  if (!bwd_fp32_positions_ok(g) && !kcnn_conv_bwd_x6_eligible(g, true, 0)) return 0;
  const int S = (int)frame_grid(g, 1);
  const int E = (g.Kdim + 1) * g.G;
  return (size_t)S * E * 4 + kcnn_reduce_splits_ws(S, E);
}

static size_t bwd_dma_lds(const ConvGeom &g) {
  return ((size_t)(g.G / 32) * 32 * 32 + (size_t)bwd_dma_sd_floats(g.P) +
          (((size_t)g.C * (g.H + 2 * g.pad_h) * (g.W + 2 * g.pad_w) + 4) & ~(size_t)3) +
          (size_t)((g.P + 31) & ~31)) * 4;
}

// fn(NCH as an integral_constant) for the chunk's NCH = G / 32 slabs
template <class F>
static auto with_nch(const ConvGeom &g, F fn) {
  switch (g.G / 32) {
    case 1: return fn(std::integral_constant<int, 1>{});
    case 2: return fn(std::integral_constant<int, 2>{});
    case 3: return fn(std::integral_constant<int, 3>{});
    default: return fn(std::integral_constant<int, 4>{});
  }
}

// The conv_bwd_dma_kernel instance for the gradients wanted (both, the weight
// gradient alone, the data gradient alone) and the pool form pc (0: none) ...
using BwdDmaKernel = decltype(&conv_bwd_dma_kernel<1, true, true, 0>);
template <int NCH, bool DX, bool WG>
static BwdDmaKernel bwd_dma_pcm(int pc) {
  if (pc == 4) return conv_bwd_dma_kernel<NCH, DX, WG, 4>;
  if (pc == 8) return conv_bwd_dma_kernel<NCH, DX, WG, 8>;
  return conv_bwd_dma_kernel<NCH, DX, WG, 0>;
}
template <int NCH>
static BwdDmaKernel bwd_dma_grads(bool dx, bool wg, int pc) {
  if (dx && wg) return bwd_dma_pcm<NCH, true, true>(pc);
  if (wg) return bwd_dma_pcm<NCH, false, true>(pc);
  return bwd_dma_pcm<NCH, true, false>(pc);
}

// ... and the conv_bwd_frame_kernel instance with or without the data gradient
using BwdStagedKernel = decltype(&conv_bwd_frame_kernel<1, true>);
template <int NCH>
static BwdStagedKernel bwd_staged_dx(bool dx) {
  if (dx) return conv_bwd_frame_kernel<NCH, true>;
  return conv_bwd_frame_kernel<NCH, false>;
}

// One filter chunk (G <= 128) of kcnn_conv_bwd_frame; dx_acc adds to dX,
// chunked: the layer has more chunks than this one.
// pc > 0: dY / dys are the pooled derivative dP of a 1 x 1 x pc Maxpool and
// pmask / pms its routing mask (see conv_bwd_dma_kernel).
static int bwd_frame_chunk(const ConvGeom &g, const float *X, int xs,
                           const float *dY, int dys, const float *K, int ks,
                           float *dX, int dxs, float *gW, int gws, float *gb,
                           void *ws, size_t ws_bytes, int dx_acc, bool chunked,
                           hipStream_t st, const unsigned char *pmask, int pms, int pc, int ph,
                           const ConvUpdateEpi *ue) {
  if (dX == nullptr && gW == nullptr) return -1;
  if (!kcnn::bwd_chunk_shape_ok(g)) return -1;
  // the workgroups' gradient partials [S][E] and their reduction
  const int S = (int)frame_grid(g, 1);
  const int E = (g.Kdim + 1) * g.G;
  float *part = static_cast<float *>(ws);
  if (gW != nullptr) {
    const size_t need = kcnn_conv_bwd_frame_ws(g);
    if (need == 0 || ws == nullptr || ws_bytes < need) return -1;
  }
  const auto reduce = [&]() {
    return kcnn_reduce_splits_epi(part, S, E, g.Kdim * g.G, g.G, 0, gW, gws, gb,
                                  ue ? *ue : ConvUpdateEpi{}, st);
  };
  // the bf16x6 kernel (cnsl-conv-x6.hip) where the shape allows; KCNN_BWD_X6=0
  // keeps the fp32-MFMA kernels below
  if (family(kFamBwdX6) && kcnn_conv_bwd_x6_eligible(g, dX != nullptr, pc, ph)) {
    // The gradient's bf16-MFMA accumulation chains are kept to 16 frames per
    // workgroup: a longer chain grows its error linearly with the frames
    // (c2 stack, prev' normwise against fp64: 2.6e-6 at 4096 frames, 9.2e-6
    // at 16384, 3.8e-5 at 65536; an fp32 contraction 1.5e-6 at each;
    // experiments/diag_wgrad_acc.py).  Larger batches run as launches over
    // frame ranges of at most BWD_X6_FRAMES, each workgroup adding its range's
    // partial to its slot in fp32 (fixed order: deterministic).
    constexpr int BWD_X6_FRAMES = 4096;
    const int nch = gW != nullptr ? (g.R + BWD_X6_FRAMES - 1) / BWD_X6_FRAMES : 1;
    int rc = 0;
    for (int c = 0; c < nch && !rc; ++c) {
      const int r0 = (int)((int64_t)g.R * c / nch), r1 = (int)((int64_t)g.R * (c + 1) / nch);
      ConvGeom gc = g;
      gc.R = r1 - r0;
      gc.M = (int64_t)gc.R * g.P;
      // every range holds at least 2048 frames (nch > 1), so the same S slots
      rc = kcnn_conv_bwd_x6(gc, X ? X + (int64_t)r0 * xs : X, xs, dY + (int64_t)r0 * dys, dys,
                            K, ks, dX ? dX + (int64_t)r0 * dxs : dX, dxs, gW ? part : nullptr,
                            nch > 1 ? (int)frame_grid(gc, 1) : S, dx_acc, st,
                            pmask ? pmask + (int64_t)r0 * pms : pmask, pms, pc, ph, c > 0);
    }
    return rc || gW == nullptr ? rc : reduce();
  }
  if (ph != 1) return -1;  // 3-D windows: the bf16x6 kernel only
  if (!bwd_fp32_positions_ok(g)) return -1;
  if (pc == 0 && ((uintptr_t)dY % 16 != 0 || dys % 4 != 0)) return -1;  // 16-B slab loads
  // pc = 2 would stage 16 rows per slab: past the register budget
  if (pc != 0 && !(pc == 4 || pc == 8)) return -1;
  const int ZZ = g.Kdim | 1;
  // weight-gradient tiles per wave: dgrad tile T belongs to wave T % 8; the
  // wgrad tiles go to the least-loaded waves, so all waves carry the same
  // number of 16-MFMA chunks (deterministic: the same table with or without dX)
  unsigned long long wg[2] = {~0ull, ~0ull};
  {
    const int ntile = (g.P + 31) / 32;
    int load[BWD_WAVES] = {0}, nw[BWD_WAVES] = {0};
    for (int T = 0; T < ntile; T++) load[T % BWD_WAVES]++;
    for (int T = 0; T < ntile; T++) {
      int best = -1;
      for (int w = 0; w < BWD_WAVES; w++)
        if (nw[w] < 2 && (best < 0 || load[w] < load[best])) best = w;
      load[best]++;
      wg[nw[best]] &= ~(0xffull << (8 * best));
      wg[nw[best]] |= (unsigned long long)T << (8 * best);
      nw[best]++;
    }
  }
  size_t lds3 = bwd_dma_lds(g);
  // a separate Z buffer when it fits (deferred col2im, see the kernel)
  const size_t zbytes = (size_t)g.P * ZZ * 4;
  const int zsep = dX != nullptr && lds3 + zbytes <= (size_t)kBwdLdsMax;
  if (zsep) lds3 += zbytes;
  if (g.C * g.HW <= BWD_THREADS * BWD_MAXX && lds3 <= (size_t)kBwdLdsMax) {
    const BwdDmaKernel kernel = with_nch(g, [&](auto nch) {
      return bwd_dma_grads<decltype(nch)::value>(dX != nullptr, gW != nullptr, pc);
    });
    hipLaunchKernelGGL(kernel, dim3(S), dim3(BWD_THREADS), lds3, st, g, X, xs, dY, dys, K, ks,
                       dX, dxs, part, ZZ, wg[0], wg[1], zsep, dx_acc, phase_timing(), pmask, pms);
  } else {
    // register-staged kernel (the DMA kernel's limits fail): needs the
    // gradient outputs and writes dX (it cannot add to it), so it takes a
    // layer of one chunk only.  A chunked layer declines here at its first
    // chunk, before anything is launched (the DMA kernel's LDS need does not
    // grow with fewer filters, so a later chunk does not fail where the first
    // passed).
    if (gW == nullptr || chunked || pc) return -1;
    const int SP = bwd_sp(g);
    const size_t lds = bwd_lds(g, SP);
    if (lds > (size_t)kFrameLdsMax) return -1;
    const int Hp = g.H + 2 * g.pad_h, Wp = g.W + 2 * g.pad_w;
    const FastDiv dhp((uint32_t)Hp), dhpwp((uint32_t)(Hp * Wp));
    const BwdStagedKernel kernel = with_nch(
        g, [&](auto nch) { return bwd_staged_dx<decltype(nch)::value>(dX != nullptr); });
    hipLaunchKernelGGL(kernel, dim3(S), dim3(BWD_THREADS), lds, st, g, X, xs, dY, dys, K, ks, dX,
                       dxs, part, ZZ, SP, dhp, dhpwp);
  }
  int rc = (int)hipGetLastError();
  return rc || gW == nullptr ? rc : reduce();
}

// dX (nullable) and/or gW, gb (nullable) from one pass over dY.  gW == NULL
// runs the data gradient only and needs no workspace.  G > 128 (c5's
// 256-filter layers) runs in chunks of 128 filters: dY columns, W columns
// and gW/gb columns of a chunk are plain offsets into the same matrices, and
// the chunks after the first add their data gradient into dX (fixed order).
int kcnn_conv_bwd_frame(const ConvGeom &g, const float *X, int xs,
                        const float *dY, int dys, const float *K, int ks,
                        float *dX, int dxs, float *gW, int gws, float *gb,
                        void *ws, size_t ws_bytes, hipStream_t st,
                        const unsigned char *pmask, int pms, int pc, int ph) {
  // the caller's update request (conv-update.h), for this layer's W
  ConvUpdateEpi *u = kcnn_conv_update_current();
  if (u && !(gW && gb && u->Kdim == g.Kdim && u->G == g.G)) u = nullptr;
  if (g.G > 128 && (g.G % 32 != 0 || (int64_t)g.G * g.P * 4 % 16 != 0)) return -1;
  const int rc = for_filter_chunks(g, [&](const ConvGeom &gc, int g0) {
    // pooled rows of P / ph values when pc, masks of 1 (ph == 1) or 2 bytes
    const int64_t dofs = pc ? (int64_t)(g0 / pc) * (g.P / ph) : (int64_t)g0 * g.P;
    const int64_t mofs = dofs * (ph > 1 ? 2 : 1);
    ConvUpdateEpi uc{};
    if (u) {  // the chunk's filter columns of W, prev and b
      uc = *u;
      uc.W += g0;
      uc.prev += g0;
      uc.b += g0;
      uc.G = gc.G;
    }
    return bwd_frame_chunk(gc, X, xs, dY + dofs, dys, K + g0, ks, dX, dxs,
                           gW ? gW + g0 : nullptr, gws, gb ? gb + g0 : nullptr, ws, ws_bytes,
                           g0 > 0, g.G > 128, st, pmask ? pmask + mofs : nullptr, pms, pc, ph,
                           u ? &uc : nullptr);
  });
  if (rc == 0 && u) u->applied = 1;
  return rc;
}
