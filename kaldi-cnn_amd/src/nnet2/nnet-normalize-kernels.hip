// nnet2/nnet-normalize-kernels.hip -- NormalizeComponent (reference
// nnet-component.cc:576-639) on gfx950: every row scaled to root-mean-square 1.
// HBM-bound, every byte touched once:
//   * rows of up to 4096 columns live in one wave's registers (the Softmax
//     form, row-regs.h; 4, 16, 32 or 64 values a lane): sum x^2 and sum dy x
//     are cross-lane reductions, no LDS and no barrier;
//   * rows of 4097 to 16384 columns live in the registers of one block's four
//     waves (32 or 64 values a thread); the waves' sums meet in LDS, in wave
//     order;
//   * wider rows run a block per row that reads the row twice;
//   * lanes take 4, 2 or 1 consecutive columns as the pointers and strides
//     allow; pad columns are never written;
//   * a row's sums are added in an order fixed by its length and the access
//     width alone: a thread's values in four interleaved chains, the lanes by
//     the xor butterfly, the waves in order.  No atomics.
// Backprop loads a whole row of out_deriv before it stores any of in_deriv
// (the re-read form finishes the dot product first), so the two may be the
// same matrix.
#include <hip/hip_runtime.h>
#include <math.h>

#include "nnet-kernels.h"
#include "row-regs.h"
#include "../cnslmat/hip-util.h"

using kcnn::contiguous_enough;
using kcnn::same_shape;
using namespace kcnn::rowregs;

namespace {

constexpr int kBlockRowMaxCols = 16384;  // 256 threads x 64 values

// kNormFloor = 2^-66 (nnet-component.cc:576).
constexpr float kNormFloor = 0x1.0p-66f;

// f = max(p, kNormFloor)^-0.5 with p = inv_d * sum x^2 (AddDiagMat2(1 / D),
// ApplyFloor, ApplyPow(-0.5)): a NaN p stays NaN, p = inf gives 0, and the
// floor gives exactly 2^33 (a correctly rounded square root and divide).
__device__ __forceinline__ float norm_scale(float ss, float inv_d, bool *floored) {
  float p = ss * inv_d;
  *floored = p <= kNormFloor;
  if (p < kNormFloor) p = kNormFloor;
  return __fdiv_rn(1.0f, __fsqrt_rn(p));
}

// The second term's coefficient (:632-638): -(1 / D) * (dot * g), g = f^3, or 0
// where f is the floor's 2^33 (ReplaceValue).  Products, as in the reference:
// a non-finite dot stays non-finite on the floor branch too.
__device__ __forceinline__ float norm_coef(float f, bool floored, float dot, float inv_d) {
  const float g = floored ? 0.0f : f * f * f;
  return -inv_d * (dot * g);
}

// A thread's TOT values added in four interleaved chains, then the chains.
template <int TOT>
__device__ __forceinline__ float sum_squares(const float (&x)[TOT]) {
  float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int j = 0; j < TOT; j++) a[j & 3] = fmaf(x[j], x[j], a[j & 3]);
  return (a[0] + a[1]) + (a[2] + a[3]);
}
template <int TOT>
__device__ __forceinline__ float sum_products(const float (&x)[TOT], const float (&y)[TOT]) {
  float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int j = 0; j < TOT; j++) a[j & 3] = fmaf(x[j], y[j], a[j & 3]);
  return (a[0] + a[1]) + (a[2] + a[3]);
}

// ---- Propagate --------------------------------------------------------------------
// One wave per row, four rows to a block.
template <int V, int TOT>
__global__ __launch_bounds__(256) void normalize_prop_wave_kernel(const float *__restrict__ in,
                                                                  int64_t is,
                                                                  float *__restrict__ out,
                                                                  int64_t os, int rows, int cols,
                                                                  float inv_d) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float x[TOT];
  load_row<V, TOT>(in + (int64_t)r * is, cols, lane, 0.0f, x);
  bool floored;
  const float f = norm_scale(wave_sum(sum_squares<TOT>(x)), inv_d, &floored);
#pragma unroll
  for (int j = 0; j < TOT; j++) x[j] *= f;
  store_row<V, TOT>(out + (int64_t)r * os, cols, lane, x);
}

// One block per row, the row in the registers of its four waves.
template <int V, int TOT>
__global__ __launch_bounds__(kBlock) void normalize_prop_block_kernel(
    const float *__restrict__ in, int64_t is, float *__restrict__ out, int64_t os, int rows,
    int cols, float inv_d) {
  __shared__ float red[4];
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    float x[TOT];
    load_row<V, TOT, kBlock>(in + (int64_t)r * is, cols, threadIdx.x, 0.0f, x);
    bool floored;
    const float f = norm_scale(block_sum(sum_squares<TOT>(x), red), inv_d, &floored);
#pragma unroll
    for (int j = 0; j < TOT; j++) x[j] *= f;
    store_row<V, TOT, kBlock>(out + (int64_t)r * os, cols, threadIdx.x, x);
  }
}

// Rows wider than a block holds: a block per row, the row read twice.
__global__ __launch_bounds__(kBlock) void normalize_prop_reread_kernel(
    const float *__restrict__ in, int64_t is, float *__restrict__ out, int64_t os, int rows,
    int cols, float inv_d) {
  __shared__ float red[4];
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const float *x = in + (int64_t)r * is;
    float *y = out + (int64_t)r * os;
    float ss = 0.0f;
    for (int c = threadIdx.x; c < cols; c += kBlock) ss = fmaf(x[c], x[c], ss);
    bool floored;
    const float f = norm_scale(block_sum(ss, red), inv_d, &floored);
    for (int c = threadIdx.x; c < cols; c += kBlock) y[c] = x[c] * f;
  }
}

// ---- Backprop ------------------------------------------------------------------------
// in_deriv = f dy + coef x from one read of x and dy.  E and D may be the
// same matrix (no __restrict__ on them).
template <int V, int TOT>
__global__ __launch_bounds__(256) void normalize_backprop_wave_kernel(
    const float *__restrict__ X, int64_t xs, const float *E, int64_t es, float *D, int64_t ds,
    int rows, int cols, float inv_d) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float x[TOT], e[TOT];
  load_row<V, TOT>(X + (int64_t)r * xs, cols, lane, 0.0f, x);
  load_row<V, TOT>(E + (int64_t)r * es, cols, lane, 0.0f, e);
  const float ss = wave_sum(sum_squares<TOT>(x));
  const float dot = wave_sum(sum_products<TOT>(e, x));
  bool floored;
  const float f = norm_scale(ss, inv_d, &floored);
  const float coef = norm_coef(f, floored, dot, inv_d);
#pragma unroll
  for (int j = 0; j < TOT; j++) e[j] = fmaf(coef, x[j], f * e[j]);
  store_row<V, TOT>(D + (int64_t)r * ds, cols, lane, e);
}

template <int V, int TOT>
__global__ __launch_bounds__(kBlock) void normalize_backprop_block_kernel(
    const float *__restrict__ X, int64_t xs, const float *E, int64_t es, float *D, int64_t ds,
    int rows, int cols, float inv_d) {
  __shared__ float red_ss[4], red_dot[4];
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    float x[TOT], e[TOT];
    load_row<V, TOT, kBlock>(X + (int64_t)r * xs, cols, threadIdx.x, 0.0f, x);
    load_row<V, TOT, kBlock>(E + (int64_t)r * es, cols, threadIdx.x, 0.0f, e);
    const float ss = block_sum(sum_squares<TOT>(x), red_ss);
    const float dot = block_sum(sum_products<TOT>(e, x), red_dot);
    bool floored;
    const float f = norm_scale(ss, inv_d, &floored);
    const float coef = norm_coef(f, floored, dot, inv_d);
#pragma unroll
    for (int j = 0; j < TOT; j++) e[j] = fmaf(coef, x[j], f * e[j]);
    store_row<V, TOT, kBlock>(D + (int64_t)r * ds, cols, threadIdx.x, e);
  }
}

// The re-read form: both sums, a barrier (block_sum's), then the element-wise
// pass, in which a thread reads E[c] before it writes D[c].
__global__ __launch_bounds__(kBlock) void normalize_backprop_reread_kernel(
    const float *__restrict__ X, int64_t xs, const float *E, int64_t es, float *D, int64_t ds,
    int rows, int cols, float inv_d) {
  __shared__ float red_ss[4], red_dot[4];
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const float *x = X + (int64_t)r * xs, *e = E + (int64_t)r * es;
    float *d = D + (int64_t)r * ds;
    float ss = 0.0f, dot = 0.0f;
    for (int c = threadIdx.x; c < cols; c += kBlock) {
      const float xv = x[c];
      ss = fmaf(xv, xv, ss);
      dot = fmaf(e[c], xv, dot);
    }
    ss = block_sum(ss, red_ss);
    dot = block_sum(dot, red_dot);
    bool floored;
    const float f = norm_scale(ss, inv_d, &floored);
    const float coef = norm_coef(f, floored, dot, inv_d);
    for (int c = threadIdx.x; c < cols; c += kBlock) d[c] = fmaf(coef, x[c], f * e[c]);
  }
}

// Values a thread holds: the wave kernels are built for 4, 16, 32 and 64 (a
// lane of 64), the block kernels for 32 and 64 (a thread of 256).  32 for the
// wave form, which Softmax does without: a 1152-column row in 64 registers a
// lane leaves room for two waves a SIMD in Backprop, in 32 for three.
int wave_values(int cols) { return cols <= 256 ? 4 : cols <= 1024 ? 16 : cols <= 2048 ? 32 : 64; }
int block_values(int cols) { return cols <= kBlock * 32 ? 32 : 64; }

}  // namespace

extern "C" {

int kn_normalize_prop(const float *in, MatrixDim in_dim, float *out, MatrixDim out_dim,
                      kcnn_stream_t st) {
  if (!same_shape(in_dim, out_dim) || !contiguous_enough(in_dim) ||
      !contiguous_enough(out_dim))
    return (int)hipErrorInvalidValue;
  const int rows = in_dim.rows, cols = in_dim.cols;
  if (rows == 0 || cols == 0) return 0;
  hipStream_t s = kcnn::as_stream(st);
  const float inv_d = (float)(1.0 / cols);
  const int64_t is = in_dim.stride, os = out_dim.stride;
  const Operand ops[] = {{in, in_dim.stride}, {out, out_dim.stride}};
  if (cols > kBlockRowMaxCols) {
    hipLaunchKernelGGL(normalize_prop_reread_kernel, dim3(row_blocks(rows)), dim3(kBlock), 0, s,
                       in, is, out, os, rows, cols, inv_d);
  } else if (cols > kWaveRowMaxCols) {
    dispatch_kernel<32, 64>(lane_width(ops), block_values(cols), [&](auto V, auto TOT) {
      hipLaunchKernelGGL((normalize_prop_block_kernel<decltype(V)::value, decltype(TOT)::value>),
                         dim3(row_blocks(rows)), dim3(kBlock), 0, s, in, is, out, os, rows, cols,
                         inv_d);
    });
  } else {
    dispatch_kernel<4, 16, 32, 64>(lane_width(ops), wave_values(cols), [&](auto V, auto TOT) {
      hipLaunchKernelGGL((normalize_prop_wave_kernel<decltype(V)::value, decltype(TOT)::value>),
                         dim3((rows + 3) / 4), dim3(256), 0, s, in, is, out, os, rows, cols,
                         inv_d);
    });
  }
  return kcnn::launch_status();
}

int kn_normalize_backprop(const float *in_value, MatrixDim iv_dim, const float *out_deriv,
                          MatrixDim od_dim, float *in_deriv, MatrixDim id_dim,
                          kcnn_stream_t st) {
  if (!same_shape(iv_dim, od_dim) || !same_shape(id_dim, od_dim) ||
      !contiguous_enough(iv_dim) || !contiguous_enough(od_dim) || !contiguous_enough(id_dim))
    return (int)hipErrorInvalidValue;
  const int rows = od_dim.rows, cols = od_dim.cols;
  if (rows == 0 || cols == 0) return 0;
  hipStream_t s = kcnn::as_stream(st);
  const float inv_d = (float)(1.0 / cols);
  const int64_t xs = iv_dim.stride, es = od_dim.stride, ds = id_dim.stride;
  const Operand ops[] = {
      {in_value, iv_dim.stride}, {out_deriv, od_dim.stride}, {in_deriv, id_dim.stride}};
  if (cols > kBlockRowMaxCols) {
    hipLaunchKernelGGL(normalize_backprop_reread_kernel, dim3(row_blocks(rows)), dim3(kBlock), 0,
                       s, in_value, xs, out_deriv, es, in_deriv, ds, rows, cols, inv_d);
  } else if (cols > kWaveRowMaxCols) {
    dispatch_kernel<32, 64>(lane_width(ops), block_values(cols), [&](auto V, auto TOT) {
      hipLaunchKernelGGL(
          (normalize_backprop_block_kernel<decltype(V)::value, decltype(TOT)::value>),
          dim3(row_blocks(rows)), dim3(kBlock), 0, s, in_value, xs, out_deriv, es, in_deriv, ds,
          rows, cols, inv_d);
    });
  } else {
    dispatch_kernel<4, 16, 32, 64>(lane_width(ops), wave_values(cols), [&](auto V, auto TOT) {
      hipLaunchKernelGGL(
          (normalize_backprop_wave_kernel<decltype(V)::value, decltype(TOT)::value>),
          dim3((rows + 3) / 4), dim3(256), 0, s, in_value, xs, out_deriv, es, in_deriv, ds, rows,
          cols, inv_d);
    });
  }
  return kcnn::launch_status();
}

}  // extern "C"
