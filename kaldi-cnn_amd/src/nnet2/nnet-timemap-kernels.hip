// nnet2/nnet-timemap-kernels.hip -- the two HBM-bound passes of the
// time-shared whole-utterance forward (capi/time-plan.h) on gfx950: the level
// epilogue (Maxpool along time and channels, ReLU, or the pool then the ReLU,
// one pass over a map) and the gather that rebuilds the window layout the
// first component above the time maps reads.  Lanes along channels (coalesced
// rows), 16-byte accesses where the strides and bases allow, 64-bit row
// offsets.  The convolutions themselves are GEMMs of the matrix layer.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "nnet-kernels.h"
#include "../cnslmat/hip-util.h"

namespace {

// ---- level epilogue ----------------------------------------------------------
// Block: 256 * V consecutive output channels; rows grid-strided over
// blockIdx.y.  POOL: v = the reference's fold (start -1e20f, replace when v <
// x) over c < pc (outer), w < pw (inner) of in[r + delta w][oc pc + c], stored
// to `mid` when a ReLU follows, else to `out`.  RELU: x < 0 -> 0 (NaN and -0
// stay), stored to `out`.  V = 4 needs pc = 1.
template <int V, bool POOL, bool RELU>
__global__ __launch_bounds__(256) void timemap_epilogue_kernel(
    const float *__restrict__ in, int64_t is, float *__restrict__ mid, int64_t ms,
    float *__restrict__ out, int64_t os, int rows, int cols, int pw, int pc, int delta) {
  const int c = (blockIdx.x * 256 + threadIdx.x) * V;
  if (c >= cols) return;
  for (int r = blockIdx.y; r < rows; r += gridDim.y) {
    float v[V];
    if constexpr (POOL) {
#pragma unroll
      for (int j = 0; j < V; j++) v[j] = -1e20f;
      if constexpr (V == 4) {
        for (int w = 0; w < pw; w++) {
          const float4 x =
              *reinterpret_cast<const float4 *>(in + (int64_t)(r + delta * w) * is + c);
          if (v[0] < x.x) v[0] = x.x;
          if (v[1] < x.y) v[1] = x.y;
          if (v[2] < x.z) v[2] = x.z;
          if (v[3] < x.w) v[3] = x.w;
        }
      } else {
        for (int cc = 0; cc < pc; cc++)
          for (int w = 0; w < pw; w++) {
            const float x = in[(int64_t)(r + delta * w) * is + (int64_t)c * pc + cc];
            if (v[0] < x) v[0] = x;
          }
      }
      float *dst = (RELU ? mid + (int64_t)r * ms : out + (int64_t)r * os) + c;
      if constexpr (V == 4)
        *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
      else
        *dst = v[0];
    } else if constexpr (V == 4) {
      const float4 x = *reinterpret_cast<const float4 *>(in + (int64_t)r * is + c);
      v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
      v[0] = in[(int64_t)r * is + c];
    }
    if constexpr (RELU) {
#pragma unroll
      for (int j = 0; j < V; j++)
        if (v[j] < 0.0f) v[j] = 0.0f;  // ApplyFloor(0)
      float *dst = out + (int64_t)r * os + c;
      if constexpr (V == 4)
        *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
      else
        *dst = v[0];
    }
  }
}

// ---- gather --------------------------------------------------------------------
// out[r][k + c n] = map[src(r) + delta k][c], src(r) = r + u ext for the
// utterance u of result row r (a search over the starts, one thread a row).
// Block: one output row at a time (grid-strided over blockIdx.x) x the tc
// channels from blockIdx.y * tc.  The n map rows are read along c (VL: 16
// bytes a lane) into an LDS tile laid out as the output row, tile[c n + k],
// which is then written out contiguously (VS: 16 bytes a lane): no lane stores
// 4 bytes at a stride of n.  The tile is the whole dynamic LDS (base 16-byte
// aligned); the row's source follows it.
struct GatherArgs {
  int num_utts, ext, out_rows, map_rows;
  int channels, n, delta, tc;
};

template <bool VL, bool VS>
__global__ __launch_bounds__(256) void timemap_gather_kernel(const float *__restrict__ map,
                                                             int64_t ms, float *__restrict__ out,
                                                             int64_t os,
                                                             const int *__restrict__ utt_start,
                                                             GatherArgs a) {
  extern __shared__ float tile[];
  int *s_src = reinterpret_cast<int *>(tile + (size_t)a.tc * a.n);
  const int c0 = blockIdx.y * a.tc;
  const int nc = min(a.tc, a.channels - c0);
  const int seg = nc * a.n;
  constexpr int V = VL ? 4 : 1;
  const int ncv = nc / V;
  for (int r = blockIdx.x; r < a.out_rows; r += gridDim.x) {
    __syncthreads();  // the last row's readers are done
    if (threadIdx.x == 0) {
      int lo = 0, hi = a.num_utts;  // start(lo) <= r < start(hi)
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (utt_start[mid] <= r) lo = mid; else hi = mid;
      }
      // (a table that disagrees with the matrices still reads inside `map`)
      *s_src = max(0, min(r + lo * a.ext, a.map_rows - 1 - a.delta * (a.n - 1)));
    }
    __syncthreads();
    const int64_t src = *s_src;
    for (int e = threadIdx.x; e < a.n * ncv; e += 256) {
      const int k = e / ncv, c = (e - k * ncv) * V;
      const float *p = map + (src + (int64_t)a.delta * k) * ms + c0 + c;
      if constexpr (VL) {
        const float4 x = *reinterpret_cast<const float4 *>(p);
        tile[(c + 0) * a.n + k] = x.x;
        tile[(c + 1) * a.n + k] = x.y;
        tile[(c + 2) * a.n + k] = x.z;
        tile[(c + 3) * a.n + k] = x.w;
      } else {
        tile[c * a.n + k] = *p;
      }
    }
    __syncthreads();
    float *dst = out + (int64_t)r * os + (int64_t)c0 * a.n;
    if constexpr (VS) {
      const int seg4 = seg >> 2;
      for (int e = threadIdx.x; e < seg4; e += 256)
        reinterpret_cast<float4 *>(dst)[e] = reinterpret_cast<const float4 *>(tile)[e];
      for (int e = (seg4 << 2) + threadIdx.x; e < seg; e += 256) dst[e] = tile[e];
    } else {
      for (int e = threadIdx.x; e < seg; e += 256) dst[e] = tile[e];
    }
  }
}

bool aligned16(const void *p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

extern "C" {

int kn_timemap_epilogue(const float *in, MatrixDim in_dim, float *pooled, MatrixDim p_dim,
                        float *relu, MatrixDim r_dim, int rows, int pool_width, int pool_channel,
                        int delta, kcnn_stream_t st) {
  const bool pool = pooled != nullptr, act = relu != nullptr;
  if (in == nullptr || (!pool && !act) || rows < 1 || delta < 1 || pool_width < 1 ||
      pool_channel < 1 || (!pool && (pool_width != 1 || pool_channel != 1)) ||
      in_dim.cols < 1 || in_dim.cols % pool_channel != 0 || !kcnn::contiguous_enough(in_dim))
    return (int)hipErrorInvalidValue;
  const int cols = in_dim.cols / pool_channel;
  // the last row's highest tap is a row of `in`
  if ((int64_t)rows - 1 + (int64_t)delta * (pool_width - 1) > (int64_t)in_dim.rows - 1)
    return (int)hipErrorInvalidValue;
  if (pool && (p_dim.rows < rows || p_dim.cols != cols || !kcnn::contiguous_enough(p_dim)))
    return (int)hipErrorInvalidValue;
  if (act && (r_dim.rows < rows || r_dim.cols != cols || !kcnn::contiguous_enough(r_dim)))
    return (int)hipErrorInvalidValue;
  bool vec4 = pool_channel == 1 && cols % 4 == 0 && in_dim.stride % 4 == 0 && aligned16(in);
  if (pool) vec4 = vec4 && p_dim.stride % 4 == 0 && aligned16(pooled);
  if (act) vec4 = vec4 && r_dim.stride % 4 == 0 && aligned16(relu);
  const dim3 grid = kcnn::elementwise_grid(rows, cols, vec4 ? 1024 : 256);
  const hipStream_t s = kcnn::as_stream(st);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, in, (int64_t)in_dim.stride, pooled,
                       (int64_t)p_dim.stride, act ? relu : pooled,
                       (int64_t)(act ? r_dim.stride : p_dim.stride), rows, cols, pool_width,
                       pool_channel, delta);
  };
  if (vec4) {
    if (pool && act) launch(timemap_epilogue_kernel<4, true, true>);
    else if (pool) launch(timemap_epilogue_kernel<4, true, false>);
    else launch(timemap_epilogue_kernel<4, false, true>);
  } else {
    if (pool && act) launch(timemap_epilogue_kernel<1, true, true>);
    else if (pool) launch(timemap_epilogue_kernel<1, true, false>);
    else launch(timemap_epilogue_kernel<1, false, true>);
  }
  return kcnn::launch_status();
}

int kn_timemap_gather(const float *map, MatrixDim map_dim, float *out, MatrixDim out_dim,
                      const int *utt_start, int num_utts, int ext, int positions, int dilation,
                      kcnn_stream_t st) {
  const int64_t span = (int64_t)dilation * ((int64_t)positions - 1);
  if (map == nullptr || out == nullptr || utt_start == nullptr || num_utts < 1 || ext < 0 ||
      positions < 1 || positions > KN_TIMEMAP_MAX_POSITIONS || dilation < 1 ||
      map_dim.cols < 1 || out_dim.rows < num_utts ||
      (int64_t)out_dim.cols != (int64_t)map_dim.cols * positions ||
      !kcnn::contiguous_enough(map_dim) || !kcnn::contiguous_enough(out_dim))
    return (int)hipErrorInvalidValue;
  // the last result row's last position is a row of `map`
  if ((int64_t)out_dim.rows - 1 + (int64_t)(num_utts - 1) * ext + span >
      (int64_t)map_dim.rows - 1)
    return (int)hipErrorInvalidValue;
  GatherArgs a;
  a.num_utts = num_utts;
  a.ext = ext;
  a.out_rows = out_dim.rows;
  a.map_rows = map_dim.rows;
  a.channels = map_dim.cols;
  a.n = positions;
  a.delta = dilation;
  // the channels of a tile: up to 256, fewer while the tile would pass 32 KiB
  a.tc = 256;
  while (a.tc > 1 && (int64_t)a.tc * positions > KN_TIMEMAP_MAX_POSITIONS) a.tc >>= 1;
  const bool vl = map_dim.cols % 4 == 0 && a.tc % 4 == 0 && map_dim.stride % 4 == 0 &&
                  aligned16(map);
  const bool vs = a.tc % 4 == 0 && out_dim.stride % 4 == 0 && aligned16(out);
  const dim3 grid((unsigned)std::min(out_dim.rows, 32768),
                  (unsigned)((map_dim.cols + a.tc - 1) / a.tc));
  const size_t lds = sizeof(float) * ((size_t)a.tc * positions + 4);
  const hipStream_t s = kcnn::as_stream(st);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, map, (int64_t)map_dim.stride, out,
                       (int64_t)out_dim.stride, utt_start, a);
  };
  if (vl && vs) launch(timemap_gather_kernel<true, true>);
  else if (vl) launch(timemap_gather_kernel<true, false>);
  else if (vs) launch(timemap_gather_kernel<false, true>);
  else launch(timemap_gather_kernel<false, false>);
  return kcnn::launch_status();
}

}  // extern "C"
