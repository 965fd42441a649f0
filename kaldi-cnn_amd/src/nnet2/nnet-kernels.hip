// nnet2/nnet-kernels.hip -- RectifiedLinearComponent and SpliceComponent on
// gfx950.  Both are HBM-bound copies/element-wise maps: one pass over the
// data, lanes along columns (coalesced rows), 64-bit row offsets, and the
// ReLU statistics reduced in a fixed order (deterministic).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "nnet-kernels.h"
#include "../cnslmat/hip-util.h"

using kcnn::FastDiv;

namespace {

// ---- ReLU ------------------------------------------------------------------
// Block: 256 consecutive columns; rows grid-strided over blockIdx.y.
__global__ __launch_bounds__(256) void relu_prop_kernel(const float *__restrict__ in,
                                                        int64_t is, float *__restrict__ out,
                                                        int64_t os, int rows, int cols) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  for (int r = blockIdx.y; r < rows; r += gridDim.y) {
    float v = in[(int64_t)r * is + c];
    if (v < 0.0f) v = 0.0f;  // ApplyFloor(0): `if (x < floor) x = floor`
    out[(int64_t)r * os + c] = v;
  }
}

// The same four columns to a lane (16-B accesses; see kn_relu_prop)
__global__ __launch_bounds__(256) void relu_prop4_kernel(const float *__restrict__ in,
                                                         int64_t is, float *__restrict__ out,
                                                         int64_t os, int rows, int cols) {
  const int c = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (c >= cols) return;
  for (int r = blockIdx.y; r < rows; r += gridDim.y) {
    float4 v = *reinterpret_cast<const float4 *>(in + (int64_t)r * is + c);
    if (v.x < 0.0f) v.x = 0.0f;
    if (v.y < 0.0f) v.y = 0.0f;
    if (v.z < 0.0f) v.z = 0.0f;
    if (v.w < 0.0f) v.w = 0.0f;
    *reinterpret_cast<float4 *>(out + (int64_t)r * os + c) = v;
  }
}

constexpr int kReluRowsPerPart = 64;

// Block: 256 consecutive columns x one chunk of kReluRowsPerPart rows.
__global__ __launch_bounds__(256) void relu_backprop_kernel(
    const float *__restrict__ ov, int64_t ovs, const float *__restrict__ od, int64_t ods,
    float *__restrict__ id, int64_t ids, int rows, int cols, float *__restrict__ part_v,
    float *__restrict__ part_h) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int r0 = blockIdx.y * kReluRowsPerPart;
  if (c >= cols) return;
  const int r1 = min(rows, r0 + kReluRowsPerPart);
  float sv = 0.0f, sh = 0.0f;
  for (int r = r0; r < r1; r++) {
    const float o = ov[(int64_t)r * ovs + c];
    const float h = o > 0.0f ? 1.0f : 0.0f;  // ApplyHeaviside
    id[(int64_t)r * ids + c] = h * od[(int64_t)r * ods + c];  // MulElements
    sv += o;
    sh += h;
  }
  if (part_v) {
    part_v[(int64_t)blockIdx.y * cols + c] = sv;
    part_h[(int64_t)blockIdx.y * cols + c] = sh;
  }
}

// The same map four columns to a lane (16-B accesses; cols, strides and
// pointers multiples of 4 floats): a block is 256 columns x one 64-row part,
// wave w taking rows w, w + 4, ...; the part's column sums are the four
// waves' sums added in wave order.
__global__ __launch_bounds__(256) void relu_backprop4_kernel(
    const float *__restrict__ ov, int64_t ovs, const float *__restrict__ od, int64_t ods,
    float *__restrict__ id, int64_t ids, int rows, int cols, float *__restrict__ part_v,
    float *__restrict__ part_h) {
  __shared__ float4 red[2][3][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = (blockIdx.x * 64 + lane) * 4;
  const int r0 = blockIdx.y * kReluRowsPerPart;
  const int r1 = min(rows, r0 + kReluRowsPerPart);
  float4 sv = make_float4(0.0f, 0.0f, 0.0f, 0.0f), sh = sv;
  if (c < cols) {
#pragma unroll 4
    for (int r = r0 + w; r < r1; r += 4) {
      const float4 o = *reinterpret_cast<const float4 *>(ov + (int64_t)r * ovs + c);
      const float4 d = *reinterpret_cast<const float4 *>(od + (int64_t)r * ods + c);
      const float4 h = make_float4(o.x > 0.0f ? 1.0f : 0.0f, o.y > 0.0f ? 1.0f : 0.0f,
                                   o.z > 0.0f ? 1.0f : 0.0f, o.w > 0.0f ? 1.0f : 0.0f);
      *reinterpret_cast<float4 *>(id + (int64_t)r * ids + c) =
          make_float4(h.x * d.x, h.y * d.y, h.z * d.z, h.w * d.w);
      sv.x += o.x; sv.y += o.y; sv.z += o.z; sv.w += o.w;
      sh.x += h.x; sh.y += h.y; sh.z += h.z; sh.w += h.w;
    }
  }
  if (part_v == nullptr) return;
  if (w > 0) {
    red[0][w - 1][lane] = sv;
    red[1][w - 1][lane] = sh;
  }
  __syncthreads();
  if (w > 0 || c >= cols) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float4 a = red[0][k][lane], b = red[1][k][lane];
    sv.x += a.x; sv.y += a.y; sv.z += a.z; sv.w += a.w;
    sh.x += b.x; sh.y += b.y; sh.z += b.z; sh.w += b.w;
  }
  *reinterpret_cast<float4 *>(part_v + (int64_t)blockIdx.y * cols + c) = sv;
  *reinterpret_cast<float4 *>(part_h + (int64_t)blockIdx.y * cols + c) = sh;
}

__global__ __launch_bounds__(256) void relu_stats_final_kernel(
    const float *__restrict__ part_v, const float *__restrict__ part_h, int nparts,
    int cols, double *__restrict__ value_sum, double *__restrict__ deriv_sum) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  float sv = 0.0f, sh = 0.0f;  // CuVector<BaseFloat> temp (:355-361)
#pragma unroll 16
  for (int p = 0; p < nparts; p++) {
    sv += part_v[(int64_t)p * cols + c];
    sh += part_h[(int64_t)p * cols + c];
  }
  value_sum[c] += (double)sv;
  deriv_sum[c] += (double)sh;
}

// ---- Splice ----------------------------------------------------------------
struct SpliceArgs {
  kn_splice_geom g;
  FastDiv div_cols, div_dim, div_ocs, div_ics;
};

__global__ __launch_bounds__(256) void splice_prop_kernel(const float *__restrict__ in,
                                                          int64_t is, float *__restrict__ out,
                                                          int64_t os, SpliceArgs a,
                                                          int64_t total) {
  const kn_splice_geom &g = a.g;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * 256) {
    uint32_t orow, col, chunk, oi;
    a.div_cols.divmod((uint32_t)e, orow, col);
    a.div_ocs.divmod(orow, chunk, oi);
    int irow, icol;
    if ((int)col < g.num_splice * g.dim) {
      uint32_t c, d;
      a.div_dim.divmod(col, c, d);
      irow = (int)chunk * g.in_cs + (g.table ? (int)g.in_index[c * g.out_cs + oi]
                                             : g.out_first + (int)oi + g.context[c] - g.in_first);
      icol = (int)d;
    } else {
      irow = (int)chunk * g.in_cs + (int)oi;
      icol = g.dim + ((int)col - g.num_splice * g.dim);
    }
    out[(int64_t)orow * os + col] = in[(int64_t)irow * is + icol];
  }
}

// The whole-utterance form (kn_splice_ragged_prop): a block takes groups of
// `rpb` consecutive output rows.  One thread per row finds the row's
// utterance (a binary search over the num_utts + 1 starts, which stay in the
// caches) and leaves the utterance's first input row, its last in-utterance
// index and the row's own index in LDS; then all 256 threads copy the group's
// V-float units, so narrow rows fill the lanes as wide ones do.  V = 4: 16-byte
// accesses (dim, const_dim and both strides multiples of 4, bases aligned).
constexpr int kRaggedMaxRows = 64;  // rows of a group
struct RaggedArgs {
  kn_ragged_splice_geom g;
  int in_rows, out_rows, rpb;
  FastDiv div_units, div_dim;
};

template <int V>
__global__ __launch_bounds__(256) void splice_ragged_kernel(const float *__restrict__ in,
                                                            int64_t is, float *__restrict__ out,
                                                            int64_t os,
                                                            const int *__restrict__ utt_start,
                                                            RaggedArgs a) {
  __shared__ int s_first[kRaggedMaxRows], s_last[kRaggedMaxRows], s_t[kRaggedMaxRows];
  const kn_ragged_splice_geom &g = a.g;
  const int units = (g.num_splice * g.dim + g.const_dim) / V;
  const int ngroups = (a.out_rows + a.rpb - 1) / a.rpb;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int r0 = grp * a.rpb;
    const int nr = min(a.rpb, a.out_rows - r0);
    __syncthreads();  // the last group's readers are done
    if ((int)threadIdx.x < nr) {
      const int r = r0 + (int)threadIdx.x;
      int lo = 0, hi = g.num_utts;  // start(lo) <= r < start(hi)
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (utt_start[mid] + mid * g.out_ext <= r) lo = mid; else hi = mid;
      }
      const int s0 = utt_start[lo], frames = utt_start[lo + 1] - s0;
      s_first[threadIdx.x] = s0 + lo * g.in_ext;
      s_last[threadIdx.x] = frames + g.in_ext - 1;
      s_t[threadIdx.x] = r - (s0 + lo * g.out_ext);
    }
    __syncthreads();
    const int n = nr * units;
    for (int e = threadIdx.x; e < n; e += 256) {
      uint32_t lr, cu;
      a.div_units.divmod((uint32_t)e, lr, cu);
      const int col = (int)cu * V;
      int idx, icol;
      if (col < g.num_splice * g.dim) {
        uint32_t c, d;
        a.div_dim.divmod((uint32_t)col, c, d);
        idx = s_t[lr] + g.context[c] + g.shift;
        icol = (int)d;
      } else {
        idx = s_t[lr] + g.const_shift;
        icol = g.dim + (col - g.num_splice * g.dim);
      }
      idx = max(0, min(idx, s_last[lr]));
      // (a table that disagrees with the matrices still reads inside `in`)
      const int irow = max(0, min(s_first[lr] + idx, a.in_rows - 1));
      const float *src = in + (int64_t)irow * is + icol;
      float *dst = out + (int64_t)(r0 + (int)lr) * os + col;
      if constexpr (V == 4)
        *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(src);
      else
        *dst = *src;
    }
  }
}

// The frame-index form (kn_splice_frames_prop), shaped as the ragged kernel:
// groups of `rpb` consecutive output rows to a block; one thread per row loads
// the {row, first, last} triple of the row's example, staged by the host, so
// nothing is searched here, and leaves the corpus row before the context
// offset, the utterance's bounds and the const tail's row in LDS; then all 256
// threads copy the group's V-float units.
struct FramesArgs {
  kn_frames_splice_geom g;
  int in_rows, out_rows, rpb;
  FastDiv div_units, div_dim, div_ocs;
};

template <int V>
__global__ __launch_bounds__(256) void splice_frames_kernel(const float *__restrict__ in,
                                                            int64_t is, float *__restrict__ out,
                                                            int64_t os,
                                                            const int *__restrict__ examples,
                                                            FramesArgs a) {
  __shared__ int s_row[kRaggedMaxRows], s_lo[kRaggedMaxRows], s_hi[kRaggedMaxRows],
      s_const[kRaggedMaxRows];
  const kn_frames_splice_geom &g = a.g;
  const int units = (g.num_splice * g.dim + g.const_dim) / V;
  const int ngroups = (a.out_rows + a.rpb - 1) / a.rpb;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int r0 = grp * a.rpb;
    const int nr = min(a.rpb, a.out_rows - r0);
    __syncthreads();  // the last group's readers are done
    if ((int)threadIdx.x < nr) {
      uint32_t n, oi;
      a.div_ocs.divmod((uint32_t)(r0 + (int)threadIdx.x), n, oi);
      const int *ex = examples + 3 * (int64_t)n;
      const int r = ex[0];
      s_lo[threadIdx.x] = ex[1];
      s_hi[threadIdx.x] = ex[2];
      s_row[threadIdx.x] = r + (g.table ? (int)g.out_offset[oi] : g.out_first + (int)oi);
      s_const[threadIdx.x] = r + g.const_first + (int)oi;
    }
    __syncthreads();
    const int n = nr * units;
    for (int e = threadIdx.x; e < n; e += 256) {
      uint32_t lr, cu;
      a.div_units.divmod((uint32_t)e, lr, cu);
      const int col = (int)cu * V;
      int row, icol;
      if (col < g.num_splice * g.dim) {
        uint32_t c, d;
        a.div_dim.divmod((uint32_t)col, c, d);
        row = s_row[lr] + g.context[c];
        icol = (int)d;
      } else {
        row = s_const[lr];
        icol = g.dim + (col - g.num_splice * g.dim);
      }
      row = max(s_lo[lr], min(row, s_hi[lr]));
      // (triples that disagree with the matrix still read inside `in`)
      row = max(0, min(row, a.in_rows - 1));
      const float *src = in + (int64_t)row * is + icol;
      float *dst = out + (int64_t)(r0 + (int)lr) * os + col;
      if constexpr (V == 4)
        *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(src);
      else
        *dst = *src;
    }
  }
}

// The streaming arena's step (kn_stream_assemble), shaped as the ragged
// kernel: groups of `rpb` consecutive written rows to a block; one thread per
// row finds the row's slot (a binary search over the num_slots + 1 staged
// prefix entries; a slot that writes nothing is never found) and leaves where
// the row comes from -- an arena row of the slot's current buffer, or a row of
// the caller's chunk -- and the arena row it goes to in LDS; then all 256
// threads copy the group's V-float units.  The arena is read and written
// through one pointer: sources and destinations are different buffers.
constexpr int kAssembleMaxBlocks = 1024;  // a step writes a few rows a stream
struct AssembleArgs {
  int num_slots, total_rows, arena_rows, chunk_rows, rpb;
  FastDiv div_units;
};

template <int V>
__global__ __launch_bounds__(256) void stream_assemble_kernel(
    float *arena, int64_t as, const float *__restrict__ chunk, int64_t cs,
    const int *__restrict__ row_start, const int *__restrict__ desc, AssembleArgs a, int units) {
  // s_src: the source row, in the chunk when s_chunk; s_dst < 0: nothing to copy
  __shared__ int s_src[kRaggedMaxRows], s_dst[kRaggedMaxRows], s_chunk[kRaggedMaxRows];
  const int ngroups = (a.total_rows + a.rpb - 1) / a.rpb;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int r0 = grp * a.rpb;
    const int nr = min(a.rpb, a.total_rows - r0);
    __syncthreads();  // the last group's readers are done
    if ((int)threadIdx.x < nr) {
      const int r = r0 + (int)threadIdx.x;
      int lo = 0, hi = a.num_slots;  // row_start[lo] <= r < row_start[hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (row_start[mid] <= r) lo = mid; else hi = mid;
      }
      const int *d = desc + 5 * (int64_t)lo;
      const int k = r - row_start[lo], tail = d[1];
      const bool from_chunk = k >= tail;
      const int src = from_chunk ? d[3] + (k - tail) : d[0] + k;
      const int dst = d[2] + k;
      const bool ok = k >= 0 && k < tail + d[4] && src >= 0 &&
                      src < (from_chunk ? a.chunk_rows : a.arena_rows) && dst >= 0 &&
                      dst < a.arena_rows;
      s_src[threadIdx.x] = src;
      s_chunk[threadIdx.x] = from_chunk;
      s_dst[threadIdx.x] = ok ? dst : -1;
    }
    __syncthreads();
    const int n = nr * units;
    for (int e = threadIdx.x; e < n; e += 256) {
      uint32_t lr, cu;
      a.div_units.divmod((uint32_t)e, lr, cu);
      if (s_dst[lr] < 0) continue;
      const int col = (int)cu * V;
      const float *src = s_chunk[lr] ? chunk + (int64_t)s_src[lr] * cs + col
                                     : arena + (int64_t)s_src[lr] * as + col;
      float *dst = arena + (int64_t)s_dst[lr] * as + col;
      if constexpr (V == 4)
        *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(src);
      else
        *dst = *src;
    }
  }
}

// A time-shared streaming step's level-0 map (kn_stream_segments), shaped as
// the kernel above: groups of `rpb` consecutive map rows to a block; one
// thread per row finds the row's segment (a binary search over the segments'
// first destination rows, ascending) and leaves the arena row it copies --
// clamped to the segment's [lo, hi], then into the arena -- in LDS; then all
// 256 threads copy the group's V-float units.  A map row no segment covers is
// not written.
struct SegmentArgs {
  int num_segs, map_rows, arena_rows, rpb;
  FastDiv div_units;
};

template <int V>
__global__ __launch_bounds__(256) void stream_segments_kernel(
    const float *__restrict__ arena, int64_t as, float *__restrict__ map, int64_t ms,
    const int *__restrict__ desc, SegmentArgs a, int units) {
  __shared__ int s_src[kRaggedMaxRows];  // < 0: nothing to copy
  const int ngroups = (a.map_rows + a.rpb - 1) / a.rpb;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int r0 = grp * a.rpb;
    const int nr = min(a.rpb, a.map_rows - r0);
    __syncthreads();  // the last group's readers are done
    if ((int)threadIdx.x < nr) {
      const int r = r0 + (int)threadIdx.x;
      int lo = 0, hi = a.num_segs;  // dst(lo) <= r < dst(hi)
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (desc[5 * (int64_t)mid + 3] <= r) lo = mid; else hi = mid;
      }
      const int *d = desc + 5 * (int64_t)lo;
      const int k = r - d[3];
      // (k < 2^31 - src0 by k < rows; the host keeps src0 + rows inside an int)
      const bool ok = k >= 0 && k < d[4] && d[1] <= d[2];
      const int src = ok ? max(0, min(max(d[1], min(d[0] + k, d[2])), a.arena_rows - 1)) : -1;
      s_src[threadIdx.x] = src;
    }
    __syncthreads();
    const int n = nr * units;
    for (int e = threadIdx.x; e < n; e += 256) {
      uint32_t lr, cu;
      a.div_units.divmod((uint32_t)e, lr, cu);
      if (s_src[lr] < 0) continue;
      const int col = (int)cu * V;
      const float *src = arena + (int64_t)s_src[lr] * as + col;
      float *dst = map + (int64_t)(r0 + (int)lr) * ms + col;
      if constexpr (V == 4)
        *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(src);
      else
        *dst = *src;
    }
  }
}

__global__ __launch_bounds__(256) void splice_backprop_kernel(
    const float *__restrict__ od, int64_t ods, float *__restrict__ id, int64_t ids,
    SpliceArgs a, int64_t total) {
  const kn_splice_geom &g = a.g;
  const int in_cols = g.dim + g.const_dim;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * 256) {
    const int irow = (int)(e / in_cols), icol = (int)(e - (int64_t)irow * in_cols);
    uint32_t chunk, ii;
    a.div_ics.divmod((uint32_t)irow, chunk, ii);
    float v = 0.0f;
    if (icol < g.dim) {
      for (int c = 0; c < g.num_splice; c++) {
        int oi = -1;
        if (g.table) {  // the output row of block c that read row ii (at most one)
          for (int o = 0; o < g.out_cs; o++)
            if (g.in_index[c * g.out_cs + o] == (int)ii) { oi = o; break; }
        } else {
          oi = g.in_first + (int)ii - g.context[c] - g.out_first;
        }
        if (oi >= 0 && oi < g.out_cs)
          v += od[((int64_t)chunk * g.out_cs + oi) * ods + c * g.dim + icol];
      }
    } else if ((int)ii < g.out_cs) {  // const part: copied from row (chunk, ii)
      v = od[((int64_t)chunk * g.out_cs + ii) * ods + g.num_splice * g.dim + (icol - g.dim)];
    }
    id[(int64_t)irow * ids + icol] = v;
  }
}

__global__ __launch_bounds__(256) void dvec_update_kernel(double *__restrict__ y,
                                                          const double *__restrict__ x,
                                                          double alpha, double beta, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  y[i] = beta * y[i] + (x ? alpha * x[i] : 0.0);
}

SpliceArgs splice_args(const kn_splice_geom &g, int out_cols) {
  SpliceArgs a;
  a.g = g;
  a.div_cols = FastDiv((uint32_t)(out_cols > 0 ? out_cols : 1));
  a.div_dim = FastDiv((uint32_t)(g.dim > 0 ? g.dim : 1));
  a.div_ocs = FastDiv((uint32_t)(g.out_cs > 0 ? g.out_cs : 1));
  a.div_ics = FastDiv((uint32_t)(g.in_cs > 0 ? g.in_cs : 1));
  return a;
}

}  // namespace

extern "C" {

int kn_relu_prop(const float *in, MatrixDim in_dim, float *out, MatrixDim out_dim,
                 kcnn_stream_t st) {
  if (in_dim.rows != out_dim.rows || in_dim.cols != out_dim.cols)
    return (int)hipErrorInvalidValue;
  if (in_dim.rows == 0 || in_dim.cols == 0) return 0;
  const bool vec4 = in_dim.cols % 4 == 0 && in_dim.stride % 4 == 0 && out_dim.stride % 4 == 0 &&
                    (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0;
  const int cpb = vec4 ? 1024 : 256;  // columns per block
  const dim3 grid = kcnn::elementwise_grid(in_dim.rows, in_dim.cols, cpb);
  if (vec4)
    hipLaunchKernelGGL(relu_prop4_kernel, grid, dim3(256), 0, kcnn::as_stream(st), in,
                       (int64_t)in_dim.stride, out, (int64_t)out_dim.stride, in_dim.rows,
                       in_dim.cols);
  else
    hipLaunchKernelGGL(relu_prop_kernel, grid, dim3(256), 0, kcnn::as_stream(st), in,
                       (int64_t)in_dim.stride, out, (int64_t)out_dim.stride, in_dim.rows,
                       in_dim.cols);
  return kcnn::launch_status();
}

size_t kn_relu_stats_ws(MatrixDim dim) {
  const int nparts = (dim.rows + kReluRowsPerPart - 1) / kReluRowsPerPart;
  return (size_t)2 * nparts * (dim.cols > 0 ? dim.cols : 1) * sizeof(float);
}

int kn_relu_backprop(const float *out_value, MatrixDim ov_dim, const float *out_deriv,
                     MatrixDim od_dim, float *in_deriv, MatrixDim id_dim,
                     double *value_sum, double *deriv_sum, void *ws, kcnn_stream_t st) {
  if (ov_dim.rows != od_dim.rows || ov_dim.cols != od_dim.cols ||
      id_dim.rows != od_dim.rows || id_dim.cols != od_dim.cols)
    return (int)hipErrorInvalidValue;
  if (od_dim.rows == 0 || od_dim.cols == 0) return 0;
  const bool stats = value_sum != nullptr;
  if (stats && ws == nullptr) return (int)hipErrorInvalidValue;
  const int nparts = (od_dim.rows + kReluRowsPerPart - 1) / kReluRowsPerPart;
  float *pv = stats ? static_cast<float *>(ws) : nullptr;
  float *ph = stats ? pv + (size_t)nparts * od_dim.cols : nullptr;
  hipStream_t s = kcnn::as_stream(st);
  const bool vec4 = od_dim.cols % 4 == 0 && ov_dim.stride % 4 == 0 &&
                    od_dim.stride % 4 == 0 && id_dim.stride % 4 == 0 &&
                    (uintptr_t)out_value % 16 == 0 && (uintptr_t)out_deriv % 16 == 0 &&
                    (uintptr_t)in_deriv % 16 == 0 && (uintptr_t)pv % 16 == 0;
  if (vec4)
    hipLaunchKernelGGL(relu_backprop4_kernel, dim3((od_dim.cols + 255) / 256, nparts),
                       dim3(256), 0, s, out_value, (int64_t)ov_dim.stride, out_deriv,
                       (int64_t)od_dim.stride, in_deriv, (int64_t)id_dim.stride, od_dim.rows,
                       od_dim.cols, pv, ph);
  else
    hipLaunchKernelGGL(relu_backprop_kernel, dim3((od_dim.cols + 255) / 256, nparts),
                       dim3(256), 0, s, out_value, (int64_t)ov_dim.stride, out_deriv,
                       (int64_t)od_dim.stride, in_deriv, (int64_t)id_dim.stride, od_dim.rows,
                       od_dim.cols, pv, ph);
  int rc = kcnn::launch_status();
  if (rc || !stats) return rc;
  hipLaunchKernelGGL(relu_stats_final_kernel, dim3((od_dim.cols + 255) / 256), dim3(256),
                     0, s, pv, ph, nparts, od_dim.cols, value_sum, deriv_sum);
  return kcnn::launch_status();
}

}  // extern "C"

namespace {
// The geometry checks both splice directions share: shapes against the
// chunk layout, and every input row a table (or a contiguous range) names
// inside the input chunk, the table within its kernel-argument array.
bool splice_geom_ok(MatrixDim in_dim, MatrixDim out_dim, const kn_splice_geom &g) {
  if (g.num_splice <= 0 || g.num_splice > KN_SPLICE_MAX_CONTEXT ||
      in_dim.rows != g.num_chunks * g.in_cs || out_dim.rows != g.num_chunks * g.out_cs ||
      in_dim.cols != g.dim + g.const_dim ||
      out_dim.cols != g.num_splice * g.dim + g.const_dim)
    return false;
  if (g.table) {
    if ((int64_t)g.num_splice * g.out_cs > KN_SPLICE_MAX_TAB) return false;
    for (int e = 0; e < g.num_splice * g.out_cs; e++)
      if (g.in_index[e] < 0 || g.in_index[e] >= g.in_cs) return false;
  } else {
    for (int c = 0; c < g.num_splice; c++) {
      const int lo = g.out_first + g.context[c] - g.in_first;
      if (lo < 0 || lo + g.out_cs > g.in_cs) return false;
    }
  }
  return true;
}
}  // namespace

extern "C" {

int kn_splice_prop(const float *in, MatrixDim in_dim, float *out, MatrixDim out_dim,
                   kn_splice_geom g, kcnn_stream_t st) {
  if (!splice_geom_ok(in_dim, out_dim, g)) return (int)hipErrorInvalidValue;
  const int64_t total = (int64_t)out_dim.rows * out_dim.cols;
  if (total == 0) return 0;
  if (total >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(splice_prop_kernel, dim3(kcnn::grid_for(total)), dim3(256), 0,
                     kcnn::as_stream(st), in, (int64_t)in_dim.stride, out,
                     (int64_t)out_dim.stride, splice_args(g, out_dim.cols), total);
  return kcnn::launch_status();
}

int kn_splice_ragged_prop(const float *in, MatrixDim in_dim, float *out, MatrixDim out_dim,
                          const int *utt_start, kn_ragged_splice_geom g, kcnn_stream_t st) {
  const int64_t in_rows = (int64_t)g.total + (int64_t)g.num_utts * g.in_ext;
  const int64_t out_rows = (int64_t)g.total + (int64_t)g.num_utts * g.out_ext;
  if (utt_start == nullptr || g.num_utts <= 0 || g.total < g.num_utts || g.in_ext < 0 ||
      g.out_ext < 0 || g.dim <= 0 || g.const_dim < 0 || g.num_splice <= 0 ||
      g.num_splice > KN_SPLICE_MAX_CONTEXT || in_rows != in_dim.rows ||
      out_rows != out_dim.rows || in_dim.cols != g.dim + g.const_dim ||
      out_dim.cols != g.num_splice * g.dim + g.const_dim || in_dim.stride < in_dim.cols ||
      out_dim.stride < out_dim.cols)
    return (int)hipErrorInvalidValue;
  if ((int64_t)out_dim.rows * out_dim.cols >= ((int64_t)1 << 31) ||
      (int64_t)in_dim.rows * in_dim.cols >= ((int64_t)1 << 31))
    return (int)hipErrorInvalidValue;
  const bool vec4 = g.dim % 4 == 0 && g.const_dim % 4 == 0 && in_dim.stride % 4 == 0 &&
                    out_dim.stride % 4 == 0 && (uintptr_t)in % 16 == 0 &&
                    (uintptr_t)out % 16 == 0;
  const int v = vec4 ? 4 : 1;
  const int units = out_dim.cols / v;
  RaggedArgs a;
  a.g = g;
  a.in_rows = in_dim.rows;
  a.out_rows = out_dim.rows;
  // about four units a thread and group
  a.rpb = std::max(1, std::min(kRaggedMaxRows, 1024 / units));
  a.div_units = FastDiv((uint32_t)units);
  a.div_dim = FastDiv((uint32_t)g.dim);
  const int ngroups = (out_dim.rows + a.rpb - 1) / a.rpb;
  const dim3 grid((unsigned)std::min(ngroups, 256 * 32));
  if (vec4)
    hipLaunchKernelGGL(splice_ragged_kernel<4>, grid, dim3(256), 0, kcnn::as_stream(st), in,
                       (int64_t)in_dim.stride, out, (int64_t)out_dim.stride, utt_start, a);
  else
    hipLaunchKernelGGL(splice_ragged_kernel<1>, grid, dim3(256), 0, kcnn::as_stream(st), in,
                       (int64_t)in_dim.stride, out, (int64_t)out_dim.stride, utt_start, a);
  return kcnn::launch_status();
}

int kn_splice_frames_prop(const float *feats, MatrixDim dim, float *out, MatrixDim out_dim,
                          const int *examples, kn_frames_splice_geom g, kcnn_stream_t st) {
  if (feats == nullptr || out == nullptr || examples == nullptr || g.num_examples <= 0 ||
      g.out_cs <= 0 || g.dim <= 0 || g.const_dim < 0 || g.num_splice <= 0 ||
      g.num_splice > KN_SPLICE_MAX_CONTEXT || dim.rows <= 0 ||
      (int64_t)g.num_examples * g.out_cs != out_dim.rows || dim.cols != g.dim + g.const_dim ||
      out_dim.cols != g.num_splice * g.dim + g.const_dim || dim.stride < dim.cols ||
      out_dim.stride < out_dim.cols || (g.table && g.out_cs > KN_SPLICE_MAX_TAB))
    return (int)hipErrorInvalidValue;
  if ((int64_t)out_dim.rows * out_dim.cols >= ((int64_t)1 << 31) ||
      (int64_t)dim.rows * dim.cols >= ((int64_t)1 << 31))
    return (int)hipErrorInvalidValue;
  // a corpus row plus the largest offset stays an int
  int64_t reach = std::llabs((long long)g.const_first) + g.out_cs;
  if (g.table)
    for (int oi = 0; oi < g.out_cs; oi++)
      reach = std::max<int64_t>(reach, std::abs((int)g.out_offset[oi]));
  else
    reach = std::max<int64_t>(reach, std::llabs((long long)g.out_first) + g.out_cs);
  int64_t ctx = 0;
  for (int c = 0; c < g.num_splice; c++)
    ctx = std::max<int64_t>(ctx, std::llabs((long long)g.context[c]));
  if ((int64_t)dim.rows + reach + ctx >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
  const bool vec4 = g.dim % 4 == 0 && g.const_dim % 4 == 0 && dim.stride % 4 == 0 &&
                    out_dim.stride % 4 == 0 && (uintptr_t)feats % 16 == 0 &&
                    (uintptr_t)out % 16 == 0;
  const int v = vec4 ? 4 : 1;
  const int units = out_dim.cols / v;
  FramesArgs a;
  a.g = g;
  a.in_rows = dim.rows;
  a.out_rows = out_dim.rows;
  // about four units a thread and group, as the ragged form
  a.rpb = std::max(1, std::min(kRaggedMaxRows, 1024 / units));
  a.div_units = FastDiv((uint32_t)units);
  a.div_dim = FastDiv((uint32_t)g.dim);
  a.div_ocs = FastDiv((uint32_t)g.out_cs);
  const int ngroups = (out_dim.rows + a.rpb - 1) / a.rpb;
  const dim3 grid((unsigned)std::min(ngroups, 256 * 32));
  if (vec4)
    hipLaunchKernelGGL(splice_frames_kernel<4>, grid, dim3(256), 0, kcnn::as_stream(st), feats,
                       (int64_t)dim.stride, out, (int64_t)out_dim.stride, examples, a);
  else
    hipLaunchKernelGGL(splice_frames_kernel<1>, grid, dim3(256), 0, kcnn::as_stream(st), feats,
                       (int64_t)dim.stride, out, (int64_t)out_dim.stride, examples, a);
  return kcnn::launch_status();
}

int kn_stream_assemble(float *arena, MatrixDim arena_dim, const float *chunk, MatrixDim chunk_dim,
                       const int *row_start, const int *desc, int num_slots, int total_rows,
                       kcnn_stream_t st) {
  const int cols = arena_dim.cols;
  if (arena == nullptr || row_start == nullptr || desc == nullptr || num_slots <= 0 ||
      total_rows < 0 || arena_dim.rows <= 0 || cols <= 0 || arena_dim.stride < cols ||
      chunk_dim.rows < 0 || (chunk_dim.rows > 0 && (chunk == nullptr || chunk_dim.cols != cols ||
                                                    chunk_dim.stride < cols)))
    return (int)hipErrorInvalidValue;
  if ((int64_t)arena_dim.rows * cols >= ((int64_t)1 << 31) ||
      (int64_t)chunk_dim.rows * cols >= ((int64_t)1 << 31))
    return (int)hipErrorInvalidValue;
  if (total_rows == 0) return 0;
  const bool with_chunk = chunk_dim.rows > 0;
  const bool vec4 = cols % 4 == 0 && arena_dim.stride % 4 == 0 && (uintptr_t)arena % 16 == 0 &&
                    (!with_chunk || (chunk_dim.stride % 4 == 0 && (uintptr_t)chunk % 16 == 0));
  const int units = cols / (vec4 ? 4 : 1);
  AssembleArgs a;
  a.num_slots = num_slots;
  a.total_rows = total_rows;
  a.arena_rows = arena_dim.rows;
  a.chunk_rows = chunk_dim.rows;
  // about four units a thread and group, as the ragged form
  a.rpb = std::max(1, std::min(kRaggedMaxRows, 1024 / units));
  a.div_units = FastDiv((uint32_t)units);
  const int ngroups = (total_rows + a.rpb - 1) / a.rpb;
  const dim3 grid((unsigned)std::min(ngroups, kAssembleMaxBlocks));
  if (vec4)
    hipLaunchKernelGGL(stream_assemble_kernel<4>, grid, dim3(256), 0, kcnn::as_stream(st), arena,
                       (int64_t)arena_dim.stride, chunk, (int64_t)chunk_dim.stride, row_start,
                       desc, a, units);
  else
    hipLaunchKernelGGL(stream_assemble_kernel<1>, grid, dim3(256), 0, kcnn::as_stream(st), arena,
                       (int64_t)arena_dim.stride, chunk, (int64_t)chunk_dim.stride, row_start,
                       desc, a, units);
  return kcnn::launch_status();
}

int kn_stream_segments(const float *arena, MatrixDim arena_dim, float *map, MatrixDim map_dim,
                       const int *desc, int num_segs, kcnn_stream_t st) {
  const int cols = arena_dim.cols;
  if (arena == nullptr || map == nullptr || desc == nullptr || num_segs <= 0 ||
      arena_dim.rows <= 0 || map_dim.rows <= 0 || cols <= 0 || map_dim.cols != cols ||
      arena_dim.stride < cols || map_dim.stride < cols)
    return (int)hipErrorInvalidValue;
  if ((int64_t)arena_dim.rows * cols >= ((int64_t)1 << 31) ||
      (int64_t)map_dim.rows * cols >= ((int64_t)1 << 31))
    return (int)hipErrorInvalidValue;
  const bool vec4 = cols % 4 == 0 && arena_dim.stride % 4 == 0 && map_dim.stride % 4 == 0 &&
                    (uintptr_t)arena % 16 == 0 && (uintptr_t)map % 16 == 0;
  const int units = cols / (vec4 ? 4 : 1);
  SegmentArgs a;
  a.num_segs = num_segs;
  a.map_rows = map_dim.rows;
  a.arena_rows = arena_dim.rows;
  a.rpb = std::max(1, std::min(kRaggedMaxRows, 1024 / units));
  a.div_units = FastDiv((uint32_t)units);
  const int ngroups = (map_dim.rows + a.rpb - 1) / a.rpb;
  const dim3 grid((unsigned)std::min(ngroups, kAssembleMaxBlocks));
  if (vec4)
    hipLaunchKernelGGL(stream_segments_kernel<4>, grid, dim3(256), 0, kcnn::as_stream(st), arena,
                       (int64_t)arena_dim.stride, map, (int64_t)map_dim.stride, desc, a, units);
  else
    hipLaunchKernelGGL(stream_segments_kernel<1>, grid, dim3(256), 0, kcnn::as_stream(st), arena,
                       (int64_t)arena_dim.stride, map, (int64_t)map_dim.stride, desc, a, units);
  return kcnn::launch_status();
}

int kn_splice_backprop(const float *out_deriv, MatrixDim od_dim, float *in_deriv,
                       MatrixDim id_dim, kn_splice_geom g, kcnn_stream_t st) {
  if (!splice_geom_ok(id_dim, od_dim, g)) return (int)hipErrorInvalidValue;
  const int64_t total = (int64_t)id_dim.rows * id_dim.cols;
  if (total == 0) return 0;
  if (total >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(splice_backprop_kernel, dim3(kcnn::grid_for(total)), dim3(256), 0,
                     kcnn::as_stream(st), out_deriv, (int64_t)od_dim.stride, in_deriv,
                     (int64_t)id_dim.stride, splice_args(g, od_dim.cols), total);
  return kcnn::launch_status();
}

int kn_dvec_update(double *y, const double *x, double alpha, double beta, int n,
                   kcnn_stream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(dvec_update_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     kcnn::as_stream(st), y, x, alpha, beta, n);
  return kcnn::launch_status();
}

}  // extern "C"
