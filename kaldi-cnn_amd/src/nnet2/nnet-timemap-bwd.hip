// nnet2/nnet-timemap-bwd.hip -- the HBM-bound passes of a TRAINING step over
// time maps (capi/time-plan.h, time_backward_schedule) on gfx950: the level-0
// layout of a step's runs, the scatter (the gather's adjoint) and the backward
// of the level epilogue (Maxpool along time and channels, ReLU, or both).
// Lanes along channels (coalesced rows), 16-byte accesses where the strides and
// bases allow, 64-bit row offsets.  Every output element has one writer, which
// sums its terms in a fixed order: no atomics.  The convolution gradients are
// GEMMs of the matrix layer on row-shifted views (NnetStack::BackpropTimeMaps).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "nnet-kernels.h"
#include "../cnslmat/hip-util.h"

namespace {

template <int V>
__device__ __forceinline__ void load(const float *p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 x = *reinterpret_cast<const float4 *>(p);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
  } else {
    v[0] = *p;
  }
}

template <int V>
__device__ __forceinline__ void store(float *p, const float (&v)[V]) {
  if constexpr (V == 4)
    *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else
    *p = v[0];
}

// The segment of map row r: the last u with starts[u] + u ext <= r.
__device__ __forceinline__ int segment_of(const int *__restrict__ starts, int num, int ext,
                                          int r) {
  int lo = 0, hi = num;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)starts[mid] + (int64_t)mid * ext <= r) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- level-0 layout ------------------------------------------------------------
// map[base_j + i] = feats[clamp(r0_j - left + i, lo_j, hi_j)], base_j =
// starts[j] + j ext.  Block: 256 * V consecutive columns; rows grid-strided
// over blockIdx.y (the search is uniform over a block).
template <int V>
__global__ __launch_bounds__(256) void timemap_layout_kernel(
    const float *__restrict__ feats, int64_t fs, int feat_rows, float *__restrict__ map,
    int64_t ms, int map_rows, int cols, const int *__restrict__ starts,
    const int *__restrict__ runs, int num_runs, int left, int ext) {
  const int c = (blockIdx.x * 256 + threadIdx.x) * V;
  if (c >= cols) return;
  for (int r = blockIdx.y; r < map_rows; r += gridDim.y) {
    const int j = segment_of(starts, num_runs, ext, r);
    const int64_t i = (int64_t)r - ((int64_t)starts[j] + (int64_t)j * ext);
    int64_t src = (int64_t)runs[3 * j] - left + i;
    src = max((int64_t)runs[3 * j + 1], min(src, (int64_t)runs[3 * j + 2]));
    // (a table that disagrees with the matrix still reads inside it)
    src = max((int64_t)0, min(src, (int64_t)feat_rows - 1));
    float v[V];
    load<V>(feats + src * fs + c, v);
    store<V>(map + (int64_t)r * ms + c, v);
  }
}

// ---- scatter ---------------------------------------------------------------------
// dmap[s][c] = sum over k ascending of dy[start_u + t][k + c n], t = s - base_u -
// delta k, for the k with 0 <= t < F_u; u the segment of map row s.  A row that
// no window reads gets 0.  Block: 256 * V consecutive channels (V lanes' worth
// stored at once; the reads are at a stride of n floats); rows over blockIdx.y.
template <int V>
__global__ __launch_bounds__(256) void timemap_scatter_kernel(
    const float *__restrict__ dy, int64_t ys, int dy_rows, float *__restrict__ dmap, int64_t ms,
    int rows, int channels, const int *__restrict__ starts, int num_utts, int ext, int n,
    int delta) {
  const int c = (blockIdx.x * 256 + threadIdx.x) * V;
  if (c >= channels) return;
  for (int s = blockIdx.y; s < rows; s += gridDim.y) {
    const int u = segment_of(starts, num_utts, ext, s);
    const int start = starts[u], frames = starts[u + 1] - start;
    const int64_t first = (int64_t)s - ((int64_t)start + (int64_t)u * ext);
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; j++) acc[j] = 0.0f;
    for (int k = 0; k < n; k++) {
      const int64_t t = first - (int64_t)delta * k;
      if (t < 0) break;
      if (t >= frames) continue;
      // (a table that disagrees with the matrix still reads inside it)
      const int64_t row = max((int64_t)0, min((int64_t)start + t, (int64_t)dy_rows - 1));
      const float *p = dy + row * ys + k + (int64_t)c * n;
#pragma unroll
      for (int j = 0; j < V; j++) acc[j] += p[(int64_t)j * n];
    }
    store<V>(dmap + (int64_t)s * ms + c, acc);
  }
}

// ---- level epilogue, backward --------------------------------------------------
// g[s][oc] = dout[s][oc], or with RELU act[s][oc] > 0 ? dout[s][oc] : 0
// (RectifiedLinearComponent::Backprop on the output value).  POOL: din[r][ch] =
// sum over w ascending of g[r - delta w][ch / pc] for the w with 0 <= r - delta
// w < rows and in[r][ch] == pooled[r - delta w][ch / pc]: every tied maximum
// receives the gradient, a NaN none.  Else din = g.  Block: 256 * V consecutive
// columns of din; all in_rows rows grid-strided over blockIdx.y.  V = 4 needs
// pc = 1.
template <int V, bool POOL, bool RELU>
__global__ __launch_bounds__(256) void timemap_epilogue_bwd_kernel(
    const float *__restrict__ in, int64_t is, const float *__restrict__ pooled, int64_t ps,
    const float *__restrict__ act, int64_t as, const float *__restrict__ dout, int64_t os,
    float *__restrict__ din, int64_t ds, int rows, int in_rows, int in_cols, int pw, int pc,
    int delta) {
  const int ch = (blockIdx.x * 256 + threadIdx.x) * V;
  if (ch >= in_cols) return;
  const int oc = POOL ? ch / pc : ch;
  for (int r = blockIdx.y; r < in_rows; r += gridDim.y) {
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; j++) acc[j] = 0.0f;
    if constexpr (POOL) {
      float x[V];
      load<V>(in + (int64_t)r * is + ch, x);
      for (int w = 0; w < pw; w++) {
        const int64_t s = (int64_t)r - (int64_t)delta * w;
        if (s < 0) break;
        if (s >= rows) continue;
        float g[V], m[V];
        load<V>(dout + s * os + oc, g);
        load<V>(pooled + s * ps + oc, m);
        if constexpr (RELU) {
          float a[V];
          load<V>(act + s * as + oc, a);
#pragma unroll
          for (int j = 0; j < V; j++) g[j] = a[j] > 0.0f ? g[j] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < V; j++)
          if (x[j] == m[j]) acc[j] += g[j];
      }
    } else {
      float a[V];
      load<V>(dout + (int64_t)r * os + ch, acc);
      load<V>(act + (int64_t)r * as + ch, a);
#pragma unroll
      for (int j = 0; j < V; j++) acc[j] = a[j] > 0.0f ? acc[j] : 0.0f;
    }
    store<V>(din + (int64_t)r * ds + ch, acc);
  }
}

bool aligned16(const void *p) { return (uintptr_t)p % 16 == 0; }
bool vec_ok(const void *p, MatrixDim d) { return d.stride % 4 == 0 && aligned16(p); }

}  // namespace

extern "C" {

int kn_timemap_layout(const float *feats, MatrixDim dim, float *map, MatrixDim map_dim,
                      const int *run_start, const int *runs, int num_runs, int left, int ext,
                      kcnn_stream_t st) {
  if (feats == nullptr || map == nullptr || run_start == nullptr || runs == nullptr ||
      num_runs < 1 || left < 0 || ext < left || dim.rows < 1 || dim.cols < 1 ||
      map_dim.rows < 1 || map_dim.cols != dim.cols || !kcnn::contiguous_enough(dim) ||
      !kcnn::contiguous_enough(map_dim))
    return (int)hipErrorInvalidValue;
  const bool vec4 = dim.cols % 4 == 0 && vec_ok(feats, dim) && vec_ok(map, map_dim);
  const dim3 grid = kcnn::elementwise_grid(map_dim.rows, dim.cols, vec4 ? 1024 : 256);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, kcnn::as_stream(st), feats,
                       (int64_t)dim.stride, dim.rows, map, (int64_t)map_dim.stride, map_dim.rows,
                       dim.cols, run_start, runs, num_runs, left, ext);
  };
  if (vec4) launch(timemap_layout_kernel<4>);
  else launch(timemap_layout_kernel<1>);
  return kcnn::launch_status();
}

int kn_timemap_scatter(const float *dy, MatrixDim dy_dim, float *dmap, MatrixDim dmap_dim,
                       const int *utt_start, int num_utts, int ext, int positions, int dilation,
                       int rows, kcnn_stream_t st) {
  if (dy == nullptr || dmap == nullptr || utt_start == nullptr || num_utts < 1 || ext < 0 ||
      positions < 1 || dilation < 1 || rows < 1 || dmap_dim.cols < 1 || dy_dim.rows < num_utts ||
      dmap_dim.rows < rows || (int64_t)dy_dim.cols != (int64_t)dmap_dim.cols * positions ||
      !kcnn::contiguous_enough(dy_dim) || !kcnn::contiguous_enough(dmap_dim))
    return (int)hipErrorInvalidValue;
  // the last result row's last position is a computed row, as for the gather
  if ((int64_t)dy_dim.rows - 1 + (int64_t)(num_utts - 1) * ext +
          (int64_t)dilation * ((int64_t)positions - 1) > (int64_t)rows - 1)
    return (int)hipErrorInvalidValue;
  const bool vec4 = dmap_dim.cols % 4 == 0 && vec_ok(dmap, dmap_dim);
  const dim3 grid = kcnn::elementwise_grid(rows, dmap_dim.cols, vec4 ? 1024 : 256);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, kcnn::as_stream(st), dy,
                       (int64_t)dy_dim.stride, dy_dim.rows, dmap, (int64_t)dmap_dim.stride, rows,
                       dmap_dim.cols, utt_start, num_utts, ext, positions, dilation);
  };
  if (vec4) launch(timemap_scatter_kernel<4>);
  else launch(timemap_scatter_kernel<1>);
  return kcnn::launch_status();
}

int kn_timemap_epilogue_bwd(const float *in, MatrixDim in_dim, const float *pooled,
                            MatrixDim p_dim, const float *relu, MatrixDim r_dim,
                            const float *dout, MatrixDim do_dim, float *din, MatrixDim di_dim,
                            int rows, int pool_width, int pool_channel, int delta,
                            kcnn_stream_t st) {
  const bool pool = pooled != nullptr, act = relu != nullptr;
  if (dout == nullptr || din == nullptr || (!pool && !act) || (pool && in == nullptr) ||
      rows < 1 || delta < 1 || pool_width < 1 || pool_channel < 1 ||
      (!pool && (pool_width != 1 || pool_channel != 1)) || di_dim.cols < 1 ||
      di_dim.cols % pool_channel != 0 || !kcnn::contiguous_enough(di_dim) ||
      !kcnn::contiguous_enough(do_dim))
    return (int)hipErrorInvalidValue;
  const int cols = di_dim.cols / pool_channel;
  // din's rows: those the forward read, the last row's highest tap the last
  const int64_t in_rows = (int64_t)rows + (int64_t)delta * (pool_width - 1);
  if (in_rows > di_dim.rows || do_dim.rows < rows || do_dim.cols != cols)
    return (int)hipErrorInvalidValue;
  if (pool && (in_dim.rows < in_rows || in_dim.cols != di_dim.cols ||
               !kcnn::contiguous_enough(in_dim) || p_dim.rows < rows || p_dim.cols != cols ||
               !kcnn::contiguous_enough(p_dim)))
    return (int)hipErrorInvalidValue;
  if (act && (r_dim.rows < rows || r_dim.cols != cols || !kcnn::contiguous_enough(r_dim)))
    return (int)hipErrorInvalidValue;
  bool vec4 = pool_channel == 1 && cols % 4 == 0 && vec_ok(dout, do_dim) && vec_ok(din, di_dim);
  if (pool) vec4 = vec4 && vec_ok(in, in_dim) && vec_ok(pooled, p_dim);
  if (act) vec4 = vec4 && vec_ok(relu, r_dim);
  const dim3 grid = kcnn::elementwise_grid((int)in_rows, di_dim.cols, vec4 ? 1024 : 256);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, kcnn::as_stream(st), in,
                       (int64_t)in_dim.stride, pooled, (int64_t)p_dim.stride, relu,
                       (int64_t)r_dim.stride, dout, (int64_t)do_dim.stride, din,
                       (int64_t)di_dim.stride, rows, (int)in_rows, di_dim.cols, pool_width,
                       pool_channel, delta);
  };
  if (vec4) {
    if (pool && act) launch(timemap_epilogue_bwd_kernel<4, true, true>);
    else if (pool) launch(timemap_epilogue_bwd_kernel<4, true, false>);
    else launch(timemap_epilogue_bwd_kernel<4, false, true>);
  } else {
    if (pool && act) launch(timemap_epilogue_bwd_kernel<1, true, true>);
    else if (pool) launch(timemap_epilogue_bwd_kernel<1, true, false>);
    else launch(timemap_epilogue_bwd_kernel<1, false, true>);
  }
  return kcnn::launch_status();
}

}  // extern "C"
