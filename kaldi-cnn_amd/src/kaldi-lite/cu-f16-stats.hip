// kaldi-lite/cu-f16-stats.hip -- the group statistics pass behind the f16x3
// scheme's scales and checks (cnslmat/f16-split.h): the f16x3 GEMM
// (cu-gemm-f16x3.hip, through f16-stats.h), the f16x3 implicit-GEMM
// convolution (kl_absmax_rows_cols) and the FC backward (kl_gemm_stats3, which
// also carries a fused pool's deferred column blocks) call it.
//
// Max |x| and min nonzero |x| per row or per column of a pitched fp32 matrix,
// as the bit patterns of |x| (unsigned order = magnitude order, Inf / NaN
// above every finite value; max and min are order-independent, so the
// results are deterministic), and for a spread group (f16-split.h: an
// element far enough below the max to lose low bits, which the GEMM's store
// then checks, tile_epilogue) the count of its elements held only to 2^-25
// (an integer: deterministic).  A group set's statistics block is
// [max[n], min[n], cnt[n]] (n groups): max[i] sets the group's f16x3 scale,
// min[i] (0: no nonzero element) says whether the group is spread, cnt[i]
// (0 unless spread here) sizes its check.  The check is sound for any count
// that covers the group's small elements (each is held to 2^-25, spread or
// not), so a producer may also count them in a group that is not spread
// (the pooled output's columns, pool-stats.h): that only adds checks.  The
// min is taken as min(|x| - 1) in wrapping unsigned arithmetic, so a zero
// (0 - 1 = 0xffffffff) never wins, then + 1.
// A GEMM needs op(A)'s rows and op(B)'s columns; both operands' statistics
// go in one launch (stats_kernel: blocks [0, a.blocks) for A, then B's) and
// one more (stats_finalize_kernel) when either is per column:
//  rows, cols >= 2048: a block per row (thread t reads float4 t + 256 i,
//    four in flight), a wave reduction and an LDS step;
//  rows, shorter rows: a wave per row;
//  columns: block (cb, rc) covers 1024 columns (4 per thread) of a chunk of
//    rows (8 in flight) and stores its column maxima and minima as partial
//    rc; the finalize takes the maxima / minima over the chunks (64 columns
//    x 4 chunk groups per block, combined through LDS).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cnslmat/f16-split.h"
#include "cnslmat/hip-util.h"
#include "cnslmat/pool-stats-dev.h"
#include "cnslmat/pool-stats.h"
#include "kaldi-lite/cu-kernels-lite.h"
#include "kaldi-lite/f16-stats.h"

using namespace kcnn::f16x3;

namespace {

using kcnn::COLMAX_ROWS;
using kcnn::PoolCountSmem;
using kcnn::pool_colmax_block;
using kcnn::pool_count_block;

__device__ __forceinline__ const float *X_row(const StatOp &o, int r) {
  return o.X + (int64_t)r * o.ld;
}

// running max |x| (m) and min (|x| - 1) (n) over a float4
__device__ __forceinline__ void mm4(uint32_t &m, uint32_t &n, float4 q) {
  const uint32_t a = __float_as_uint(q.x) & 0x7fffffffu, b = __float_as_uint(q.y) & 0x7fffffffu,
                 c = __float_as_uint(q.z) & 0x7fffffffu, d = __float_as_uint(q.w) & 0x7fffffffu;
  m = max(max(m, a), max(max(b, c), d));
  n = min(min(n, a - 1u), min(min(b - 1u, c - 1u), d - 1u));
}
__device__ __forceinline__ void mm1(uint32_t &m, uint32_t &n, float x) {
  const uint32_t a = __float_as_uint(x) & 0x7fffffffu;
  m = max(m, a);
  n = min(n, a - 1u);
}

// the nonzero |x| of row r below bound (a spread row's count; sweep of
// stats_rows' shape)
__device__ __forceinline__ uint32_t count_small_row(const StatOp &o, const float *x, float bound,
                                                    int c, int step) {
  uint32_t n = 0;
  for (; c < o.cols; c += step)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (c + i < o.cols) {
        const float a = fabsf(x[c + i]);
        n += (a < bound && a != 0.0f) ? 1u : 0u;
      }
  return n;
}

// A row held in registers by the sweep (RV float4 per thread: up to 18432
// floats per block row, 4608 per wave row), so that a spread row counts its
// small elements without a second read (c5's C3 input and output derivative
// rows are 18432 floats, and the derivative's frames are all spread: a
// second read doubled that pass, 83 us per call)
constexpr int RV = 18;
__device__ __forceinline__ void stats_rows(const StatOp &o, int blk, uint32_t *red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool wide = o.rpb == 1;
  const int r = wide ? blk : blk * 4 + wave;
  if (r >= o.rows) return;  // (wide: uniform over the block)
  const float *x = X_row(o, r);
  const int step = wide ? 1024 : 256;  // floats per sweep of the row
  const int c0 = (wide ? threadIdx.x : lane) * 4;
  const bool held = o.vec && o.cols <= RV * step;  // uniform
  float4 q[RV];
  uint32_t m = 0, n = 0xffffffffu;
  if (held) {  // every load in flight at once; past the row: zeros (never max, min or small)
#pragma unroll
    for (int j = 0; j < RV; ++j) {
      const int c = c0 + j * step;
      if (c + 4 <= o.cols) {
        q[j] = *reinterpret_cast<const float4 *>(x + c);
      } else {
        q[j].x = c < o.cols ? x[c] : 0.0f;
        q[j].y = c + 1 < o.cols ? x[c + 1] : 0.0f;
        q[j].z = c + 2 < o.cols ? x[c + 2] : 0.0f;
        q[j].w = 0.0f;
      }
    }
#pragma unroll
    for (int j = 0; j < RV; ++j) mm4(m, n, q[j]);
  } else {
    int c = c0;
    if (o.vec) {
      for (; c + 3 * step + 4 <= o.cols; c += 4 * step) {
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const float4 *>(x + c + j * step);
#pragma unroll
        for (int j = 0; j < 4; ++j) mm4(m, n, v[j]);
      }
      for (; c + 4 <= o.cols; c += step) mm4(m, n, *reinterpret_cast<const float4 *>(x + c));
    }
    for (; c < o.cols; c += step)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (c + i < o.cols) mm1(m, n, x[c + i]);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    m = max(m, (uint32_t)__shfl_xor((int)m, d));
    n = min(n, (uint32_t)__shfl_xor((int)n, d));
  }
  if (wide) {  // the block's maxima / minima through LDS, to every thread
    if (lane == 0) {
      red[wave] = m;
      red[4 + wave] = n;
    }
    __syncthreads();
    m = max(max(red[0], red[1]), max(red[2], red[3]));
    n = min(min(red[4], red[5]), min(red[6], red[7]));
  }
  // a spread row (f16-split.h) counts its small elements (from the registers,
  // or a second sweep of the row from L2); every other row's count is 0
  uint32_t cnt = 0;
  if (kcnn::f16x3::spread(m, n + 1u)) {  // uniform over the wave (the block)
    const float bound = kcnn::f16x3::small_bound(m);
    if (held) {
      auto small = [&](float v) { return (fabsf(v) < bound && v != 0.0f) ? 1u : 0u; };
#pragma unroll
      for (int j = 0; j < RV; ++j)
        cnt += small(q[j].x) + small(q[j].y) + small(q[j].z) + small(q[j].w);
    } else {
      cnt = count_small_row(o, x, bound, c0, step);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, d);
    if (wide) {
      __syncthreads();  // (red's maxima read above)
      if (lane == 0) red[8 + wave] = cnt;
      __syncthreads();
      cnt = red[8] + red[9] + red[10] + red[11];
    }
  }
  if (wide ? threadIdx.x == 0 : lane == 0) {
    o.out[r] = m;
    o.out[o.rows + r] = n + 1u;
    o.out[2 * (size_t)o.rows + r] = cnt;
  }
}

__device__ __forceinline__ void stats_cols(const StatOp &o, int blk) {
  const int cbi = blk % o.cb, rci = blk / o.cb;
  const int c0 = cbi * 1024 + threadIdx.x * 4;
  const int r0 = rci * o.rb, rend = min(o.rows, r0 + o.rb);
  if (c0 >= o.cols) return;
  const bool v4 = o.vec && c0 + 4 <= o.cols;
  uint32_t cm[4] = {0u, 0u, 0u, 0u};
  uint32_t cn[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  auto load = [&](int r) {
    const float *x = X_row(o, r) + c0;
    if (v4) return *reinterpret_cast<const float4 *>(x);
    float4 q;
    q.x = x[0];
    q.y = c0 + 1 < o.cols ? x[1] : 0.0f;
    q.z = c0 + 2 < o.cols ? x[2] : 0.0f;
    q.w = c0 + 3 < o.cols ? x[3] : 0.0f;
    return q;
  };
  auto take = [&](float4 q) {
    mm1(cm[0], cn[0], q.x);
    mm1(cm[1], cn[1], q.y);
    mm1(cm[2], cn[2], q.z);
    mm1(cm[3], cn[3], q.w);
  };
  int r = r0;
  for (; r + 8 <= rend; r += 8) {
    float4 q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = load(r + j);
#pragma unroll
    for (int j = 0; j < 8; ++j) take(q[j]);
  }
  for (; r < rend; ++r) take(load(r));
  uint32_t *dst = o.part + (size_t)rci * o.cols + c0;
  uint32_t *dsn = dst + (size_t)o.rbk * o.cols;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (c0 + i < o.cols) {
      dst[i] = cm[i];
      dsn[i] = cn[i];
    }
}

// Up to three statistics passes in one launch (their blocks in order): a
// GEMM's two operands, or the FC backward's output derivative (rows and
// columns) and weight columns (kl_gemm_stats3)
struct StatOps {
  StatOp o[3];
  // a fused pool's pending column statistics (pool-stats-dev.h): pcx x pcy
  // colmax blocks after the ops' blocks in stats_kernel, pcn count blocks
  // after the finalize blocks in stats_finalize_kernel (0: none)
  PoolColDeferred pc;
  int pcx, pcy, pcn;
};
// the op of block `blk` among the ops' `count(o)` blocks, and its block index there
template <typename Count>
__device__ __forceinline__ int pick_op(const StatOps &s, int blk, Count count, int &local) {
  const int n0 = count(s.o[0]), n1 = count(s.o[1]);
  if (blk < n0) { local = blk; return 0; }
  if (blk < n0 + n1) { local = blk - n0; return 1; }
  local = blk - n0 - n1;
  return 2;
}
__host__ __device__ inline int ncount_blocks(const StatOp &o);
__host__ __device__ inline int nfinal_blocks(const StatOp &o) {
  return o.mode == 1 && o.blocks ? o.fblocks : 0;
}

__global__ __launch_bounds__(256) void stats_kernel(StatOps s) {
  __shared__ uint32_t red[12];
  if (s.o[0].clear && blockIdx.x == 0 && threadIdx.x < 2) s.o[0].clear[threadIdx.x] = 0u;
  const int nb3 = s.o[0].blocks + s.o[1].blocks + s.o[2].blocks;
  if ((int)blockIdx.x >= nb3) {  // (uniform) a pool's column maxima
    const int k = blockIdx.x - nb3;
    pool_colmax_block(s.pc.pcol, s.pc.nblk, s.pc.npool, s.pc.colblk, k % s.pcx, k / s.pcx);
    return;
  }
  int blk;
  const int w = pick_op(s, blockIdx.x, [](const StatOp &o) { return o.blocks; }, blk);
  const StatOp &o = s.o[w];  // (uniform)
  if (o.mode == 0) stats_rows(o, blk, red);
  else stats_cols(o, blk);
}

// The column maxima / minima over the partials (64 columns per block, 4
// groups of partials through LDS); the counts zeroed for stats_count_kernel.
__global__ __launch_bounds__(256) void stats_finalize_kernel(StatOps s) {
  __shared__ uint32_t red[2][4][64];
  __shared__ PoolCountSmem psm;
  const int nf3 = nfinal_blocks(s.o[0]) + nfinal_blocks(s.o[1]) + nfinal_blocks(s.o[2]);
  if ((int)blockIdx.x >= nf3) {  // (uniform) a pool's small elements, after its maxima
    pool_count_block(s.pc.P, s.pc.ps, s.pc.R, s.pc.npool, s.pc.vec, s.pc.rowblk, s.pc.colblk,
                     blockIdx.x - nf3, s.pcn, psm);
    return;
  }
  int blk;
  const StatOp &o = s.o[pick_op(s, blockIdx.x, [](const StatOp &q) { return nfinal_blocks(q); }, blk)];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int c = blk * 64 + lane;
  uint32_t m = 0, n = 0xffffffffu;
  if (c < o.cols) {
    const uint32_t *pm = o.part + c, *pn = o.part + (size_t)o.rbk * o.cols + c;
    int q = grp;
    for (; q + 28 < o.rbk; q += 32) {  // eight maxima and eight minima in flight
      uint32_t a[8], b[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a[j] = pm[(size_t)(q + 4 * j) * o.cols];
        b[j] = pn[(size_t)(q + 4 * j) * o.cols];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        m = max(m, a[j]);
        n = min(n, b[j]);
      }
    }
    for (; q < o.rbk; q += 4) {
      m = max(m, pm[(size_t)q * o.cols]);
      n = min(n, pn[(size_t)q * o.cols]);
    }
  }
  red[0][grp][lane] = m;
  red[1][grp][lane] = n;
  __syncthreads();
  m = max(max(red[0][0][lane], red[0][1][lane]), max(red[0][2][lane], red[0][3][lane]));
  n = min(min(red[1][0][lane], red[1][1][lane]), min(red[1][2][lane], red[1][3][lane]));
  if (grp == 0 && c < o.cols) {
    o.out[c] = m;
    o.out[o.cols + c] = n + 1u;
    o.out[2 * (size_t)o.cols + c] = 0;
  }
}

// The spread columns' counts (f16-split.h) after the finalize: block (cb,
// rc) takes 64 columns x a chunk of 64 rows, leaves at once unless one of
// its columns is spread (rare), and otherwise reads its rows' 64-column
// segments (one coalesced 256-B row piece per wave and row) and adds each
// spread column's count of small elements by an integer atomic (exact and
// order-independent).
constexpr int CNT_ROWS = 64;
__host__ __device__ inline int ncount_blocks(const StatOp &o) {
  return o.mode == 1 && o.blocks ? ((o.cols + 63) / 64) * ((o.rows + CNT_ROWS - 1) / CNT_ROWS) : 0;
}
__global__ __launch_bounds__(256) void stats_count_kernel(StatOps s) {
  int blk;
  const StatOp &o = s.o[pick_op(s, blockIdx.x, [](const StatOp &q) { return ncount_blocks(q); }, blk)];
  const int ncb = (o.cols + 63) / 64;
  const int cb = blk % ncb, rc = blk / ncb;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = cb * 64 + lane;
  bool spr = false;
  float bound = 0.0f;
  if (c < o.cols) {
    const uint32_t mx = o.out[c];
    spr = kcnn::f16x3::spread(mx, o.out[o.cols + c]);
    if (spr) bound = kcnn::f16x3::small_bound(mx);
  }
  if (__ballot(spr) == 0) return;  // block-uniform (the same columns in every wave)
  const int r0 = rc * CNT_ROWS, r1 = min(o.rows, r0 + CNT_ROWS);
  uint32_t cnt = 0;
  if (spr) {  // the wave's CNT_ROWS / 4 rows loaded together
    float v[CNT_ROWS / 4];
#pragma unroll
    for (int i = 0; i < CNT_ROWS / 4; ++i) {
      const int r = r0 + wave + 4 * i;
      v[i] = r < r1 ? fabsf(X_row(o, r)[c]) : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < CNT_ROWS / 4; ++i) cnt += (v[i] < bound && v[i] != 0.0f) ? 1u : 0u;
  }
  if (cnt) atomicAdd(o.out + 2 * (size_t)o.cols + c, cnt);
}

int stats_launch3(const StatOps &ops, hipStream_t st) {
  // empty operands: maxima 0 (no scale), minima 0 (no nonzero element)
  for (const StatOp &o : ops.o)
    if (o.blocks == 0 && o.out) {
      const size_t n = o.mode == 0 ? (size_t)std::max(o.rows, 0) : (size_t)std::max(o.cols, 0);
      if (n && hipMemsetAsync(o.out, 0, 3 * n * 4, st) != hipSuccess) return (int)hipGetLastError();
    }
  int nb = 0, nf = 0, nc = 0;
  for (const StatOp &o : ops.o) {
    nb += o.blocks;
    nf += nfinal_blocks(o);
    nc += ncount_blocks(o);
  }
  nb += ops.pcx * ops.pcy;
  nf += ops.pcn;
  if (nb == 0) return 0;
  hipLaunchKernelGGL(stats_kernel, dim3(nb), dim3(256), 0, st, ops);
  int rc = kcnn::launch_status();
  if (rc || nf == 0) return rc;
  hipLaunchKernelGGL(stats_finalize_kernel, dim3(nf), dim3(256), 0, st, ops);
  rc = kcnn::launch_status();
  if (rc || nc == 0) return rc;
  hipLaunchKernelGGL(stats_count_kernel, dim3(nc), dim3(256), 0, st, ops);
  return kcnn::launch_status();
}

}  // namespace

namespace kcnn::f16x3 {

// a statistics pass over X (rows x cols, pitch ld): mode 0 per row, 1 per
// column (partials at part, stat_part_words of them)
StatOp stat_op(const float *X, int rows, int cols, int ld, int mode, uint32_t *out,
               uint32_t *part) {
  StatOp o{};
  o.X = X; o.out = out; o.part = part;
  o.rows = rows; o.cols = cols; o.ld = ld; o.mode = mode;
  o.vec = ld % 4 == 0 && (uintptr_t)X % 16 == 0;
  if (rows <= 0 || cols <= 0) return o;  // blocks 0
  if (mode == 0) {
    o.rpb = cols >= 2048 ? 1 : 4;
    o.blocks = (rows + o.rpb - 1) / o.rpb;
  } else {
    o.cb = (cols + 1023) / 1024;
    // about 1024 blocks of at least 16 rows, at most 256 row chunks
    o.rbk = std::max(1, std::min(256, std::min((rows + 15) / 16, (1024 + o.cb - 1) / o.cb)));
    o.rb = (rows + o.rbk - 1) / o.rbk;
    o.rbk = (rows + o.rb - 1) / o.rb;
    o.blocks = o.cb * o.rbk;
    o.fblocks = (cols + 63) / 64;
  }
  return o;
}
size_t stat_part_words(int rows, int cols, int mode) {
  if (mode == 0) return 0;
  const StatOp o = stat_op(nullptr, rows, cols, cols, 1, nullptr, nullptr);
  return 2 * (size_t)o.rbk * cols;
}
int stats_launch(const StatOp &a, const StatOp &b, hipStream_t st) {
  StatOps ops{};
  ops.o[0] = a;
  ops.o[1] = b;
  ops.o[2] = StatOp{};
  return stats_launch3(ops, st);
}

}  // namespace kcnn::f16x3

extern "C" int kl_absmax_rows(const float *X, int rows, int cols, int ld, uint32_t *rmax,
                              kcnn_stream_t stream) {
  if (rows < 0 || cols < 0 || ld < cols || !rmax) return (int)hipErrorInvalidValue;
  return stats_launch(stat_op(X, rows, cols, ld, 0, rmax, nullptr), StatOp{},
                      kcnn::as_stream(stream));
}
extern "C" size_t kl_absmax_cols_words(int rows, int cols) {
  if (rows <= 0 || cols <= 0) return 0;
  return stat_part_words(rows, cols, 1);
}
extern "C" int kl_absmax_cols(const float *X, int rows, int cols, int ld, uint32_t *cmax,
                              uint32_t *part, kcnn_stream_t stream) {
  if (rows < 0 || cols < 0 || ld < cols || !cmax) return (int)hipErrorInvalidValue;
  if (rows > 0 && cols > 0 && !part) return (int)hipErrorInvalidValue;
  return stats_launch(stat_op(X, rows, cols, ld, 1, cmax, part), StatOp{},
                      kcnn::as_stream(stream));
}

// kl_absmax_rows of R (rows x cols, pitch ld) and kl_absmax_cols of Q
// (qrows x qcols, pitch ldq; part: kl_absmax_cols_words) in one statistics
// launch (and Q's finalize / count passes): the f16x3 implicit GEMM's frame
// and filter statistics (cnsl-conv-igemm-x6.hip); clear (nullable): two
// words set to 0 by the same launch (that kernel's list counters)
extern "C" int kl_absmax_rows_cols(const float *R, int rows, int cols, int ld, uint32_t *rmax,
                                   const float *Q, int qrows, int qcols, int ldq, uint32_t *cmax,
                                   uint32_t *part, uint32_t *clear, kcnn_stream_t stream) {
  if (rows < 0 || cols < 0 || ld < cols || !rmax || qrows < 0 || qcols < 0 || ldq < qcols ||
      !cmax)
    return (int)hipErrorInvalidValue;
  if (qrows > 0 && qcols > 0 && !part) return (int)hipErrorInvalidValue;
  StatOp q = stat_op(Q, qrows, qcols, ldq, 1, cmax, part);
  q.clear = clear;
  const StatOp r = stat_op(R, rows, cols, ld, 0, rmax, nullptr);
  if (clear && q.blocks + r.blocks == 0) {  // no statistics launch to clear it
    const hipError_t e = hipMemsetAsync(clear, 0, 8, kcnn::as_stream(stream));
    if (e != hipSuccess) return (int)e;
  }
  return stats_launch(q, r, kcnn::as_stream(stream));
}

// Up to three statistics passes in one set of launches (stats, finalize,
// count): op i over X_i (rows_i x cols_i, pitch ld_i), per row (mode_i 0)
// or per column (1, part_i: kl_absmax_cols_words of scratch) into the block
// out_i; X_i NULL skips op i.  The FC backward's output derivative (rows for
// the data gradient, columns for the weight gradient) and weight columns in
// one pass set instead of two (AffineComponent::Backprop).
extern "C" int kl_gemm_stats3(const float *X0, int rows0, int cols0, int ld0, int mode0,
                              uint32_t *out0, uint32_t *part0, const float *X1, int rows1,
                              int cols1, int ld1, int mode1, uint32_t *out1, uint32_t *part1,
                              const float *X2, int rows2, int cols2, int ld2, int mode2,
                              uint32_t *out2, uint32_t *part2, void *pool_cols,
                              kcnn_stream_t stream) {
  StatOps ops{};
  if (pool_cols) {  // the pool's column kernels' grids (cnsl-conv-frame.hip kcnn_pool_cols_complete)
    ops.pc = *static_cast<const PoolColDeferred *>(pool_cols);
    const int ncq = ops.pc.npool % 4 == 0 ? ops.pc.npool / 4 : ops.pc.npool;
    ops.pcx = (ncq + 255) / 256;
    ops.pcy = (ops.pc.nblk + COLMAX_ROWS - 1) / COLMAX_ROWS;
    ops.pcn = std::min(ops.pc.R, 256);
  }
  const float *X[3] = {X0, X1, X2};
  const int rows[3] = {rows0, rows1, rows2}, cols[3] = {cols0, cols1, cols2};
  const int ld[3] = {ld0, ld1, ld2}, mode[3] = {mode0, mode1, mode2};
  uint32_t *out[3] = {out0, out1, out2}, *part[3] = {part0, part1, part2};
  for (int i = 0; i < 3; ++i) {
    ops.o[i] = StatOp{};
    if (!X[i]) continue;
    if (rows[i] < 0 || cols[i] < 0 || ld[i] < cols[i] || !out[i] || (mode[i] != 0 && mode[i] != 1) ||
        (mode[i] == 1 && rows[i] > 0 && cols[i] > 0 && !part[i]))
      return (int)hipErrorInvalidValue;
    ops.o[i] = stat_op(X[i], rows[i], cols[i], ld[i], mode[i], out[i], mode[i] ? part[i] : nullptr);
  }
  return stats_launch3(ops, kcnn::as_stream(stream));
}
