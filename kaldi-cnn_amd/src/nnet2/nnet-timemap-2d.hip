// nnet2/nnet-timemap-2d.hip -- the time maps that keep a height (frequency)
// axis (capi/time-plan.h, levels (C, H, n, delta)) on gfx950: a map row holds
// H C floats, element (h, c) at column h + c H.  Three launchers
// (nnet-kernels.h): kn_timemap_conv2d, a Convolution level whose filter is
// shorter than its input is high, as an implicit GEMM on the bf16 matrix cores
// (bf16x6, cnslmat/x6-util.h); kn_timemap_pool2d, a Maxpool level that may
// fold over height, with the ReLU level on it from the same read; and
// kn_timemap_gather2d, the window layout of the last map in runs of H floats.
//
// The convolution: M = (s, oh), m = s OH + oh; N = g; K = (d, c, i), k = (d C
// + c) kh + i.  As kn_timemap_conv, a block owns a 32 x 32 output tile and its
// four waves split the 16-wide K steps, wave w taking steps w, w + 4, ...,
// each loading its MFMA fragments straight from global memory one step ahead
// of the products.  An M tile runs across time steps whenever OH does not
// divide 32: every lane works out its own (s, oh).  The K tail of the last
// step is zero-filled and never read; rows and columns past the edge are
// loaded from the last valid one and never stored.  All four waves leave
// their accumulators in LDS and the 256 threads add them in wave order, then
// the bias, apply the ReLU and store with the lanes ALONG m: the output's
// column stride across g is OH, so a wave storing its own MFMA rows would
// write 4 bytes at a stride of OH floats, whereas 32 consecutive m are runs of
// consecutive floats inside each time step.  The order of the partial sums is
// fixed: the same bits on every call.  The row tiles are on grid x, so a
// corpus of 2^31 - 1 (row, height) pairs fits one launch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "nnet-kernels.h"
#include "../cnslmat/hip-util.h"
#include "../cnslmat/x6-util.h"

namespace {

using kcnn::x6::bf16x8;

struct Conv2dArgs {
  const float *in, *w, *bias;
  float *out;
  int64_t is, ws, os;
  int mtot;  // rows OH
  int height, channels, group, kh, kw, delta, oh;
  int ktot;  // kw C kh
};

// The fragments of step s for this lane: for k = 16 s + 8 half + j = (d C + c)
// kh + i, a[j] = in[row + delta d][col0 + i + c H] (col0 = the lane's oh) and
// b[j] = W[i + d kh + c kh kw][col]; zero past ktot.
__device__ __forceinline__ void load_step2d(const Conv2dArgs &p, int s, const float *arow,
                                            const float *wcol, int half, float (&a)[8],
                                            float (&b)[8]) {
  const int k0 = s * 16 + half * 8;
  const int ck = p.channels * p.kh;
  int d = k0 / ck;
  int c = (k0 - d * ck) / p.kh;
  int i = k0 - d * ck - c * p.kh;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    if (k0 + j < p.ktot) {
      a[j] = arow[(int64_t)p.delta * d * p.is + i + c * p.height];
      b[j] = wcol[(int64_t)(i + d * p.kh + c * p.kh * p.kw) * p.ws];
    } else {
      a[j] = 0.0f;
      b[j] = 0.0f;
    }
    if (++i == p.kh) {
      i = 0;
      if (++c == p.channels) { c = 0; d++; }
    }
  }
}

// part[w][g][lane], the rows padded to 65 floats: the readers below run along
// the MFMA rows, which are 64 floats apart
constexpr int kPartStride = 65;

template <bool RELU>
__global__ __launch_bounds__(256) void timemap_conv2d_kernel(Conv2dArgs p) {
  __shared__ float part[4][16][kPartStride];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int half = lane >> 5;
  const int m0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
  // loads past the edge read the last valid row / column; never stored
  const int lm = min(m0 + (lane & 31), p.mtot - 1);
  const int ls = lm / p.oh;
  const float *arow = p.in + (int64_t)ls * p.is + (lm - ls * p.oh);
  const float *wcol = p.w + min(n0 + (lane & 31), p.group - 1);
  const int steps = (p.ktot + 15) / 16;

  kcnn::floatx16 acc = kcnn::x6::zero16();
  float a[8], b[8], an[8], bn[8];
  int s = wave;
  if (s < steps) load_step2d(p, s, arow, wcol, half, a, b);
  for (; s < steps; s += 4) {
    const bool more = s + 4 < steps;  // (wave-uniform)
    if (more) load_step2d(p, s + 4, arow, wcol, half, an, bn);
    bf16x8 fa[3], fb[3];
    kcnn::x6::split8(a, fa[0], fa[1], fa[2]);
    kcnn::x6::split8(b, fb[0], fb[1], fb[2]);
    acc = kcnn::x6::mfma6(fa, fb, acc);
    if (more) {
#pragma unroll
      for (int j = 0; j < 8; j++) { a[j] = an[j]; b[j] = bn[j]; }
    }
  }
  // (a wave without a step leaves its zeros: x + 0 is x for every x the sum holds)
#pragma unroll
  for (int g = 0; g < 16; g++) part[wave][g][lane] = acc[g];
  __syncthreads();
  // C/D map of 32x32x16: register g of lane l holds row (g & 3) + 8 (g >> 2) +
  // 4 (l >> 5), column l & 31.  Thread t takes row t & 31 of columns (t >> 5) +
  // 8 q: the lanes of a store run along m.
  const int r = threadIdx.x & 31;
  const int m = m0 + r;
  if (m >= p.mtot) return;
  const int sr = m / p.oh;
  const int g = (r & 3) + 4 * (r >> 3), rl = 32 * ((r >> 2) & 1);
  float *orow = p.out + (int64_t)sr * p.os + (m - sr * p.oh);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int cl = (threadIdx.x >> 5) + 8 * q;
    const int col = n0 + cl;
    if (col >= p.group) continue;
    float v = ((part[0][g][rl + cl] + part[1][g][rl + cl]) + part[2][g][rl + cl]) +
              part[3][g][rl + cl];
    v = p.bias[col] + v;
    if constexpr (RELU)
      if (v < 0.0f) v = 0.0f;  // ApplyFloor(0): NaN and -0 stay
    orow[(int64_t)col * p.oh] = v;
  }
}

// ---- pool --------------------------------------------------------------------
// Thread: one output column oh' + oc H'; rows grid-strided over blockIdx.y.  v
// = the reference's fold (start -1e20f, replace when v < x) over c < pc
// (outer), w < pw, h < ph (inner) of in[r + delta w][oh' ph + h + (oc pc + c)
// H], stored to `pooled`; RELU: then x < 0 -> 0 (NaN and -0 stay) to `relu`.
struct Pool2dArgs {
  int rows, cols, height, out_height, ph, pw, pc, delta;
};

template <bool RELU>
__global__ __launch_bounds__(256) void timemap_pool2d_kernel(const float *__restrict__ in,
                                                             int64_t is,
                                                             float *__restrict__ pooled,
                                                             int64_t ps, float *__restrict__ relu,
                                                             int64_t rs, Pool2dArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.cols) return;
  const int oc = j / a.out_height, oh = j - oc * a.out_height;
  const int64_t col0 = (int64_t)oh * a.ph + (int64_t)oc * a.pc * a.height;
  for (int r = blockIdx.y; r < a.rows; r += gridDim.y) {
    float v = -1e20f;
    for (int c = 0; c < a.pc; c++)
      for (int w = 0; w < a.pw; w++) {
        const float *src = in + ((int64_t)r + (int64_t)a.delta * w) * is + col0 +
                           (int64_t)c * a.height;
        for (int h = 0; h < a.ph; h++) {
          const float x = src[h];
          if (v < x) v = x;
        }
      }
    pooled[(int64_t)r * ps + j] = v;
    if constexpr (RELU) {
      if (v < 0.0f) v = 0.0f;  // ApplyFloor(0)
      relu[(int64_t)r * rs + j] = v;
    }
  }
}

// ---- gather --------------------------------------------------------------------
// out[r][h + k H + c H n] = map[src(r) + delta k][h + c H], src(r) as in
// kn_timemap_gather (the utterance by a search over the starts, clamped into
// the map).  Block: one output row at a time (grid-strided over blockIdx.x),
// the columns strided over the threads and blockIdx.y: the stores are
// contiguous, the loads runs of H floats.  A thread's first column and its
// stride are split into (c, k, h) once, outside the rows, and stepped with
// carries: no division per element.
struct Gather2dArgs {
  int num_utts, ext, out_rows, map_rows;
  int channels, height, n, delta;
};

__global__ __launch_bounds__(256) void timemap_gather2d_kernel(const float *__restrict__ map,
                                                               int64_t ms,
                                                               float *__restrict__ out,
                                                               int64_t os,
                                                               const int *__restrict__ utt_start,
                                                               Gather2dArgs a) {
  __shared__ int s_src;
  const int hn = a.height * a.n;
  const int cols = a.channels * hn;
  const int e0 = blockIdx.y * 256 + threadIdx.x, stride = gridDim.y * 256;
  const int c0 = e0 / hn, k0 = (e0 - c0 * hn) / a.height, h0 = e0 - c0 * hn - k0 * a.height;
  const int dc = stride / hn, dk = (stride - dc * hn) / a.height,
            dh = stride - dc * hn - dk * a.height;
  for (int r = blockIdx.x; r < a.out_rows; r += gridDim.x) {
    __syncthreads();  // the last row's readers are done
    if (threadIdx.x == 0) {
      int lo = 0, hi = a.num_utts;  // start(lo) <= r < start(hi)
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (utt_start[mid] <= r) lo = mid; else hi = mid;
      }
      // (a table that disagrees with the matrices still reads inside `map`)
      s_src = max(0, min(r + lo * a.ext, a.map_rows - 1 - a.delta * (a.n - 1)));
    }
    __syncthreads();
    const float *src = map + (int64_t)s_src * ms;
    float *dst = out + (int64_t)r * os;
    const int64_t kstep = (int64_t)a.delta * ms;
    int c = c0, k = k0, h = h0;
    for (int e = e0; e < cols; e += stride) {
      dst[e] = src[k * kstep + h + c * a.height];
      // (h < H and dh < H, k < n and dk < n: one carry each)
      h += dh; k += dk; c += dc;
      if (h >= a.height) { h -= a.height; k++; }
      if (k >= a.n) { k -= a.n; c++; }
    }
  }
}

}  // namespace

extern "C" {

int kn_timemap_conv2d(const float *in, MatrixDim in_dim, const float *w, MatrixDim w_dim,
                      const float *bias, float *out, MatrixDim out_dim, int rows, int height,
                      int channels, int kernel_height, int kernel_width, int delta, int relu,
                      kcnn_stream_t st) {
  const int group = w_dim.cols;
  if (in == nullptr || w == nullptr || bias == nullptr || out == nullptr || rows < 1 ||
      height < 1 || channels < 1 || kernel_height < 1 || kernel_height > height ||
      kernel_width < 1 || delta < 1 || group < 1 || !kcnn::contiguous_enough(in_dim) ||
      !kcnn::contiguous_enough(w_dim) || !kcnn::contiguous_enough(out_dim))
    return (int)hipErrorInvalidValue;
  const int oh = height - kernel_height + 1;
  const int64_t ktot = (int64_t)kernel_width * channels * kernel_height;
  if ((int64_t)in_dim.cols < (int64_t)height * channels ||
      (int64_t)out_dim.cols != (int64_t)oh * group || out_dim.rows < rows)
    return (int)hipErrorInvalidValue;
  // the last row's highest tap is a row of `in`, the last weight row one of W
  if ((int64_t)rows - 1 + (int64_t)delta * (kernel_width - 1) > (int64_t)in_dim.rows - 1 ||
      ktot - 1 > (int64_t)w_dim.rows - 1)
    return (int)hipErrorInvalidValue;
  const int64_t mtot = (int64_t)rows * oh;
  const int64_t col_blocks = ((int64_t)group + 31) / 32;
  if (mtot > KN_TIMEMAP_MAX_ROW_HEIGHTS || col_blocks > 65535) return (int)hipErrorInvalidValue;
  Conv2dArgs p;
  p.in = in; p.w = w; p.bias = bias; p.out = out;
  p.is = in_dim.stride; p.ws = w_dim.stride; p.os = out_dim.stride;
  p.mtot = (int)mtot;
  p.height = height; p.channels = channels; p.group = group;
  p.kh = kernel_height; p.kw = kernel_width; p.delta = delta; p.oh = oh;
  p.ktot = (int)ktot;
  const dim3 grid((unsigned)((mtot + 31) / 32), (unsigned)col_blocks);
  const hipStream_t s = kcnn::as_stream(st);
  if (relu)
    hipLaunchKernelGGL(timemap_conv2d_kernel<true>, grid, dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(timemap_conv2d_kernel<false>, grid, dim3(256), 0, s, p);
  return kcnn::launch_status();
}

int kn_timemap_pool2d(const float *in, MatrixDim in_dim, float *pooled, MatrixDim p_dim,
                      float *relu, MatrixDim r_dim, int rows, int height, int pool_height,
                      int pool_width, int pool_channel, int delta, kcnn_stream_t st) {
  const bool act = relu != nullptr;
  if (in == nullptr || pooled == nullptr || rows < 1 || delta < 1 || height < 1 ||
      pool_height < 1 || pool_width < 1 || pool_channel < 1 || height % pool_height != 0 ||
      in_dim.cols < 1 || in_dim.cols % height != 0 ||
      (in_dim.cols / height) % pool_channel != 0 || !kcnn::contiguous_enough(in_dim))
    return (int)hipErrorInvalidValue;
  const int out_height = height / pool_height;
  const int cols = in_dim.cols / height / pool_channel * out_height;
  // the last row's highest tap is a row of `in`
  if ((int64_t)rows - 1 + (int64_t)delta * (pool_width - 1) > (int64_t)in_dim.rows - 1)
    return (int)hipErrorInvalidValue;
  if (p_dim.rows < rows || p_dim.cols != cols || !kcnn::contiguous_enough(p_dim))
    return (int)hipErrorInvalidValue;
  if (act && (r_dim.rows < rows || r_dim.cols != cols || !kcnn::contiguous_enough(r_dim)))
    return (int)hipErrorInvalidValue;
  Pool2dArgs a;
  a.rows = rows; a.cols = cols; a.height = height; a.out_height = out_height;
  a.ph = pool_height; a.pw = pool_width; a.pc = pool_channel; a.delta = delta;
  const dim3 grid = kcnn::elementwise_grid(rows, cols, 256);
  const hipStream_t s = kcnn::as_stream(st);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, in, (int64_t)in_dim.stride, pooled,
                       (int64_t)p_dim.stride, relu, (int64_t)r_dim.stride, a);
  };
  if (act) launch(timemap_pool2d_kernel<true>);
  else launch(timemap_pool2d_kernel<false>);
  return kcnn::launch_status();
}

int kn_timemap_gather2d(const float *map, MatrixDim map_dim, float *out, MatrixDim out_dim,
                        const int *utt_start, int num_utts, int ext, int height, int positions,
                        int dilation, kcnn_stream_t st) {
  const int64_t span = (int64_t)dilation * ((int64_t)positions - 1);
  if (map == nullptr || out == nullptr || utt_start == nullptr || num_utts < 1 || ext < 0 ||
      height < 1 || positions < 1 || dilation < 1 || map_dim.cols < 1 ||
      map_dim.cols % height != 0 || out_dim.rows < num_utts ||
      (int64_t)out_dim.cols != (int64_t)map_dim.cols * positions ||
      !kcnn::contiguous_enough(map_dim) || !kcnn::contiguous_enough(out_dim))
    return (int)hipErrorInvalidValue;
  // the last result row's last position is a row of `map`
  if ((int64_t)out_dim.rows - 1 + (int64_t)(num_utts - 1) * ext + span >
      (int64_t)map_dim.rows - 1)
    return (int)hipErrorInvalidValue;
  Gather2dArgs a;
  a.num_utts = num_utts;
  a.ext = ext;
  a.out_rows = out_dim.rows;
  a.map_rows = map_dim.rows;
  a.channels = map_dim.cols / height;
  a.height = height;
  a.n = positions;
  a.delta = dilation;
  // column blocks while the rows alone do not fill the device
  const int col_blocks = std::max(1, std::min((out_dim.cols + 1023) / 1024,
                                              out_dim.rows < 2048 ? 16 : 1));
  const dim3 grid((unsigned)std::min(out_dim.rows, 32768), (unsigned)col_blocks);
  hipLaunchKernelGGL(timemap_gather2d_kernel, grid, dim3(256), 0, kcnn::as_stream(st), map,
                     (int64_t)map_dim.stride, out, (int64_t)out_dim.stride, utt_start, a);
  return kcnn::launch_status();
}

}  // extern "C"
