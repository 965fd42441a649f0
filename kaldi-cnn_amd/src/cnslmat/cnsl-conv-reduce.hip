// cnslmat/cnsl-conv-reduce.hip -- the deterministic reduction of the weight
// gradient's workgroup partials [S][E], out[e] = sum_s in[s][e] in a fixed
// order, for every convolution family: the frame backward
// (cnsl-conv-frame-bwd.hip, and cnsl-conv-x6.hip's kernel through it), the
// implicit-GEMM weight gradients (cnsl-conv-mfma.hip, cnsl-conv-igemm-x6.hip)
// and conv-dispatch.cc.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "conv-geom.h"
#include "conv-update.h"
#include "momentum-step.h"

namespace {

// Pass 1 of the implicit-GEMM v1 split-K reduction: sums groups of 32
// partial rows (conv_splitk_reduce_kernel adds the groups in order).
__global__ __launch_bounds__(256) void reduce_pass1(const float *__restrict__ in,
                                                    int S, int E,
                                                    float *__restrict__ tmp) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const int s0 = blockIdx.y * 32, s1 = min(S, s0 + 32);
  float acc = 0.0f;
  for (int s = s0; s < s1; s++) acc += in[(int64_t)s * E + e];
  tmp[(int64_t)blockIdx.y * E + e] = acc;
}

// One-pass deterministic reduction of S partial rows [S][E]: a block takes 64
// columns; its 4 waves sum interleaved rows (s = w, w + 4, ...) with the loads
// of 16 rows in flight, then add the 4 wave sums in order through LDS.  Same
// output mapping: e < nw -> gW[row][col] with (row, col) = gk_layout ?
// (e % inner, e / inner) : (e / inner, e % inner); e >= nw -> gb[e - nw].
// (Two passes of 32-row groups spent ~14 us of latency at c2, for 3.3 MB.)
// u.W != NULL (conv-update.h): the sums step W / prev (momentum_step) and b
// instead of being stored in gW / gb (W and prev with gW's (row, col)).
__global__ __launch_bounds__(256) void reduce_splits_kernel(
    const float *__restrict__ in, int S, int E, int nw, int inner, int gk_layout,
    float *__restrict__ gW, int gws, float *__restrict__ gb, ConvUpdateEpi u) {
  __shared__ float red[4][64];
  const int c = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + c;
  float acc = 0.0f;
  if (e < E) {
    int s = w;
    for (; s + 4 * 15 < S; s += 64) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; u++) v[u] = in[(int64_t)(s + 4 * u) * E + e];
#pragma unroll
      for (int u = 0; u < 16; u++) acc += v[u];
    }
    for (; s < S; s += 4) acc += in[(int64_t)s * E + e];
  }
  red[w][c] = acc;
  __syncthreads();
  if (w != 0 || e >= E) return;
  const float sum = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
  if (e < nw) {
    const int a = e / inner, b = e - a * inner;
    const int row = gk_layout ? b : a, col = gk_layout ? a : b;
    if (u.W) {  // ApplyGradient's MomentumUpdate on this element
      float *pw = u.W + (int64_t)row * u.ldw + col, *pp = u.prev + (int64_t)row * u.ldp + col;
      float p = *pp, w = *pw;
      kcnn::momentum_step(sum, p, w, u.momentum, u.a_wd, u.a_g);
      *pp = p;
      *pw = w;
    } else {
      gW[(int64_t)row * gws + col] = sum;
    }
  } else if (u.W) {  // its BiasUpdate
    u.b[e - nw] = __builtin_fmaf(u.a_g, sum, u.b[e - nw]);
  } else if (gb) {
    gb[e - nw] = sum;
  }
}

}  // namespace

size_t kcnn_reduce_splits_ws(int S, int E) {
  return (size_t)((S + 31) / 32) * (size_t)E * 4;
}

int kcnn_reduce_splits_epi(const float *in, int S, int E, int nw, int inner, int gk_layout,
                           float *gW, int gws, float *gb, const ConvUpdateEpi &u,
                           hipStream_t st) {
  hipLaunchKernelGGL(reduce_splits_kernel, dim3((E + 63) / 64), dim3(256), 0, st, in, S, E,
                     nw, inner, gk_layout, gW, gws, gb, u);
  return (int)hipGetLastError();
}

// The implicit-GEMM weight gradients' layout (gk_layout 1: e = g*Kdim + k
// for e < G*Kdim).  The caller's update request for this layer's W (conv-update.h: Kdim = inner,
// G = nw / inner) is applied here instead of storing gW / gb, as the frame
// kernels' reduction does (the long-kernel weight gradients run after the
// data gradient, so W is stepped after its last read).
int kcnn_reduce_splits_wgrad(const float *in, int S, int E, int nw, int inner, float *gW,
                             int gws, float *gb, hipStream_t st) {
  ConvUpdateEpi *u = kcnn_conv_update_current();
  if (u && !(gW && gb && inner > 0 && u->Kdim == inner && (int64_t)u->G * inner == nw &&
             E == nw + u->G))
    u = nullptr;
  const int rc = kcnn_reduce_splits_epi(in, S, E, nw, inner, 1, gW, gws, gb,
                                        u ? *u : ConvUpdateEpi{}, st);
  if (rc == 0 && u) u->applied = 1;
  return rc;
}

int kcnn_reduce_splits_pass1(const float *in, int S, int E, float *tmp,
                             hipStream_t st) {
  const int Q = (S + 31) / 32;
  hipLaunchKernelGGL(reduce_pass1, dim3((E + 255) / 256, Q), dim3(256), 0, st,
                     in, S, E, tmp);
  return (int)hipGetLastError();
}
