// nnet2/nnet-timemap-conv.hip -- a Convolution level of the time maps in ONE
// launch (kn_timemap_conv, nnet-kernels.h): the 1-D convolution along time
//   out[s][g] = act(b[g] + sum_{d < kw} sum_{c < C} in[s + delta d][c] W[c wc + d wd][g])
// with fp32 products on the bf16 matrix cores (bf16x6, cnslmat/x6-util.h), for
// the streaming computer's steps (capi/online-computer.h): a few hundred to a
// few thousand rows, where the kw GEMMs of the matrix layer and their
// statistics passes would each cost a launch.  bf16x6 needs no statistics.
//
// The sizes are small and the work is bound by launches and load latency, not
// by the matrix cores (1152 rows x 512 x 1536 is ~4 us of MFMA), so the tile
// is small and the grid wide: a block owns a 32 x 32 output tile and its four
// waves split the reduction -- the (tap, 16-channel chunk) steps, wave w
// taking steps w, w + 4, ... -- each wave loading its MFMA fragments straight
// from global memory (rows of `in` along c, 16 bytes a lane where the base and
// the stride allow; rows of W along g, coalesced over the lanes) one step
// ahead of the products.  At 1152 x 512 that is 576 blocks on 256 CUs.  Waves
// 1 .. 3 leave their accumulators in LDS and wave 0 adds them in that order,
// then the bias, applies the ReLU and stores: the same bits on every call.
// Both operands are split in registers from fp32 on every call; nothing is
// cached between calls.  The channel tail of a chunk is zero-filled and never
// read; rows and columns past the edge are loaded from the last valid one and
// not stored.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "nnet-kernels.h"
#include "../cnslmat/hip-util.h"
#include "../cnslmat/x6-util.h"

namespace {

using kcnn::x6::bf16x8;

struct ConvArgs {
  const float *in, *w, *bias;
  float *out;
  int64_t is, ws, os;
  int rows, channels, group, kw, delta, wc, wd;
  int nchunk;  // 16-channel chunks a tap
};

// The fragments of step s for this lane: a[j] = in[row + delta d][c + j], b[j]
// = W[(c + j) wc + d wd][col], c = 16 chunk + 8 (lane >> 5), zero past C.
template <bool VEC>
__device__ __forceinline__ void load_step(const ConvArgs &p, int s, int64_t row, int col,
                                          int half, float (&a)[8], float (&b)[8]) {
  const int d = s / p.nchunk;
  const int c = (s - d * p.nchunk) * 16 + half * 8;
  const float *ap = p.in + (row + (int64_t)p.delta * d) * p.is + c;
  if constexpr (VEC) {  // C % 4 == 0: a quad is inside the row or outside it
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
    if (c < p.channels) x = *reinterpret_cast<const float4 *>(ap);
    if (c + 4 < p.channels) y = *reinterpret_cast<const float4 *>(ap + 4);
    a[0] = x.x; a[1] = x.y; a[2] = x.z; a[3] = x.w;
    a[4] = y.x; a[5] = y.y; a[6] = y.z; a[7] = y.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = c + j < p.channels ? ap[j] : 0.0f;
  }
  const float *wp = p.w + ((int64_t)c * p.wc + (int64_t)d * p.wd) * p.ws + col;
  const int64_t step = (int64_t)p.wc * p.ws;
#pragma unroll
  for (int j = 0; j < 8; j++) b[j] = c + j < p.channels ? wp[j * step] : 0.0f;
}

template <bool VEC, bool RELU>
__global__ __launch_bounds__(256) void timemap_conv_kernel(ConvArgs p) {
  __shared__ float part[3][16][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int half = lane >> 5;
  const int row0 = blockIdx.y * 32, col = blockIdx.x * 32 + (lane & 31);
  // loads past the edge read the last valid row / column; never stored
  const int64_t lrow = min(row0 + (lane & 31), p.rows - 1);
  const int lcol = min(col, p.group - 1);
  const int steps = p.kw * p.nchunk;

  kcnn::floatx16 acc = kcnn::x6::zero16();
  float a[8], b[8], an[8], bn[8];
  int s = wave;
  if (s < steps) load_step<VEC>(p, s, lrow, lcol, half, a, b);
  for (; s < steps; s += 4) {
    const bool more = s + 4 < steps;  // (wave-uniform)
    if (more) load_step<VEC>(p, s + 4, lrow, lcol, half, an, bn);
    bf16x8 fa[3], fb[3];
    kcnn::x6::split8(a, fa[0], fa[1], fa[2]);
    kcnn::x6::split8(b, fb[0], fb[1], fb[2]);
    acc = kcnn::x6::mfma6(fa, fb, acc);
    if (more) {
#pragma unroll
      for (int j = 0; j < 8; j++) { a[j] = an[j]; b[j] = bn[j]; }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int g = 0; g < 16; g++) part[wave - 1][g][lane] = acc[g];
  }
  __syncthreads();
  if (wave > 0 || col >= p.group) return;
  const float bias = p.bias[col];
  // C/D map of 32x32x16: register g of lane l holds row (g & 3) + 8 (g >> 2) +
  // 4 (l >> 5), column l & 31
#pragma unroll
  for (int g = 0; g < 16; g++) {
    const int r = row0 + (g & 3) + 8 * (g >> 2) + 4 * half;
    if (r >= p.rows) continue;
    float v = ((acc[g] + part[0][g][lane]) + part[1][g][lane]) + part[2][g][lane];
    v = bias + v;
    if constexpr (RELU)
      if (v < 0.0f) v = 0.0f;  // ApplyFloor(0): NaN and -0 stay
    p.out[(int64_t)r * p.os + col] = v;
  }
}

}  // namespace

extern "C" int kn_timemap_conv(const float *in, MatrixDim in_dim, const float *w, MatrixDim w_dim,
                               const float *bias, float *out, MatrixDim out_dim, int rows,
                               int kernel_width, int delta, int wc, int wd, int relu,
                               kcnn_stream_t st) {
  const int C = in_dim.cols, group = w_dim.cols;
  if (in == nullptr || w == nullptr || bias == nullptr || out == nullptr || rows < 1 ||
      kernel_width < 1 || delta < 1 || wc < 1 || wd < 1 || C < 1 || group < 1 ||
      out_dim.cols != group || out_dim.rows < rows || !kcnn::contiguous_enough(in_dim) ||
      !kcnn::contiguous_enough(w_dim) || !kcnn::contiguous_enough(out_dim))
    return (int)hipErrorInvalidValue;
  // the last row's highest tap is a row of `in`, the last weight row one of W
  if ((int64_t)rows - 1 + (int64_t)delta * (kernel_width - 1) > (int64_t)in_dim.rows - 1 ||
      (int64_t)(C - 1) * wc + (int64_t)(kernel_width - 1) * wd > (int64_t)w_dim.rows - 1)
    return (int)hipErrorInvalidValue;
  const int64_t row_blocks = ((int64_t)rows + 31) / 32;
  if (row_blocks > 65535) return (int)hipErrorInvalidValue;
  ConvArgs p;
  p.in = in; p.w = w; p.bias = bias; p.out = out;
  p.is = in_dim.stride; p.ws = w_dim.stride; p.os = out_dim.stride;
  p.rows = rows; p.channels = C; p.group = group;
  p.kw = kernel_width; p.delta = delta; p.wc = wc; p.wd = wd;
  p.nchunk = (C + 15) / 16;
  const bool vec = C % 4 == 0 && in_dim.stride % 4 == 0 && (uintptr_t)in % 16 == 0;
  const dim3 grid((unsigned)((group + 31) / 32), (unsigned)row_blocks);
  const hipStream_t s = kcnn::as_stream(st);
  auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, p); };
  if (vec) {
    if (relu) launch(timemap_conv_kernel<true, true>);
    else launch(timemap_conv_kernel<true, false>);
  } else {
    if (relu) launch(timemap_conv_kernel<false, true>);
    else launch(timemap_conv_kernel<false, false>);
  }
  return kcnn::launch_status();
}
