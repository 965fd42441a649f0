// nnet2/nnet-loss-kernels.hip -- SoftmaxComponent, DropoutComponent and the
// cross-entropy objective (CuMatrix::CompObjfAndDeriv) on gfx950.  All are
// HBM-bound and built to touch every byte once:
//   * softmax rows of up to 4096 columns live in one wave's registers (64
//     values a lane): max, sum and the row dot product are cross-lane
//     reductions, no LDS and no barrier; wider rows run a block-per-row form
//     that re-reads the row;
//   * lanes take 4, 2 or 1 consecutive columns (16-, 8- or 4-byte accesses)
//     as the pointers and strides allow;
//   * column sums of P (NonlinearComponent::UpdateStats) and the objective
//     are reduced in a fixed order (per-part partials, then one ordered final
//     pass), never with float atomics, so results repeat bit for bit;
//   * the dropout mask is Philox4x32-10 of (seed, call, row, column / 4): a
//     pure function of the element's position, not of the launch geometry;
//     the row is the minibatch's (the matrix's row plus the caller's offset),
//     so a data-parallel shard draws its rows of the whole minibatch's mask.
#include <hip/hip_runtime.h>
#include <math.h>

#include "nnet-kernels.h"
#include "row-regs.h"
#include "../cnslmat/hip-util.h"

using kcnn::FastDiv;
using kcnn::contiguous_enough;
using kcnn::same_shape;
using namespace kcnn::rowregs;

namespace {

// ---- Softmax Propagate ---------------------------------------------------------
// One wave per row, four rows to a block.  Every kernel below that forms P
// from logits forms it with the same softmax_row, or softmax_max_sum and
// softmax_value (row-regs.h): the same bits as the P stored here.
template <int V, int TOT>
__global__ __launch_bounds__(256) void softmax_prop_wave_kernel(const float *__restrict__ in,
                                                                int64_t is,
                                                                float *__restrict__ out,
                                                                int64_t os, int rows, int cols) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float v[TOT];
  load_row<V, TOT>(in + (int64_t)r * is, cols, lane, -INFINITY, v);
  softmax_row<TOT>(v);
  store_row<V, TOT>(out + (int64_t)r * os, cols, lane, v);
}

// Rows wider than a wave holds: a block per row, the row read three times.
__global__ __launch_bounds__(256) void softmax_prop_block_kernel(const float *__restrict__ in,
                                                                 int64_t is,
                                                                 float *__restrict__ out,
                                                                 int64_t os, int rows, int cols) {
  __shared__ float red[4];
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const float *x = in + (int64_t)r * is;
    float *y = out + (int64_t)r * os;
    const RowMaxSum ms = softmax_max_sum(x, cols, red);
    for (int c = threadIdx.x; c < cols; c += 256) y[c] = softmax_value(x[c], ms);
  }
}

// ---- column sums of P in a fixed order -------------------------------------------
// A block of the wave-per-row kernels is one part of kSmRowsPerPart rows,
// wave w taking rows w, w + 4, ...; a part's column sums are the four
// waves' sums added in wave order, and the final pass adds the parts in
// order (fp64).  16 rows, not the 64 of the element-wise ReLU kernel: a block
// here spans whole rows, so 64-row parts would leave a 4096-row minibatch
// with 64 blocks for 256 compute units.
constexpr int kSmRowsPerPart = 16;
constexpr int kColRowsPerPart = 64;  // parts of colsum_part_kernel

template <int V, int TOT>
__device__ __forceinline__ void part_colsum_store(float (&cs)[TOT], float *red, int lane, int w,
                                                  float *__restrict__ part_row, int cols) {
  if (w > 0) {
#pragma unroll
    for (int j = 0; j < TOT; j++) red[((w - 1) * TOT + j) * 64 + lane] = cs[j];
  }
  __syncthreads();
  if (w > 0) return;
#pragma unroll
  for (int k = 0; k < 3; k++) {
#pragma unroll
    for (int j = 0; j < TOT; j++) cs[j] += red[(k * TOT + j) * 64 + lane];
  }
#pragma unroll
  for (int j = 0; j < TOT; j++) {
    const int c = row_col<V, TOT>(lane, j);
    if (c < cols) part_row[c] = cs[j];
  }
}

// Column sums of one 64-row part, a thread per column (the wide-row path).
__global__ __launch_bounds__(256) void colsum_part_kernel(const float *__restrict__ p, int64_t ps,
                                                          int rows, int cols,
                                                          float *__restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  const int r0 = blockIdx.y * kColRowsPerPart;
  const int r1 = min(rows, r0 + kColRowsPerPart);
  float s = 0.0f;
  for (int r = r0; r < r1; r++) s += p[(int64_t)r * ps + c];
  part[(int64_t)blockIdx.y * cols + c] = s;
}

// A block takes 64 columns: wave w of 16 adds its sixteenth of the parts in
// order (fp64), then the first wave adds the 16 sums in wave order.  (A
// thread per column alone leaves 54 waves walking 256 parts one load at a
// time: 64 us at 4096 x 3454, twice the kernel that made the parts.)
constexpr int kFinalWaves = 16;
__global__ __launch_bounds__(1024) void colsum_final_kernel(const float *__restrict__ part,
                                                            int nparts, int cols,
                                                            double *__restrict__ value_sum) {
  __shared__ double red[kFinalWaves][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int per = (nparts + kFinalWaves - 1) / kFinalWaves;
  const int p0 = w * per, p1 = min(nparts, p0 + per);
  double s = 0.0;
  if (c < cols)
    for (int p = p0; p < p1; p++) s += (double)part[(int64_t)p * cols + c];
  red[w][lane] = s;
  __syncthreads();
  if (w != 0 || c >= cols) return;
  double t = 0.0;
#pragma unroll
  for (int k = 0; k < kFinalWaves; k++) t += red[k][lane];
  value_sum[c] += t;
}

// ---- Softmax Backprop, general E ---------------------------------------------------
// D = P o E - diag(rowdot(P, E)) P from one read of P and E.
template <int V, int TOT, bool STATS>
__global__ __launch_bounds__(256) void softmax_backprop_wave_kernel(
    const float *__restrict__ P, int64_t ps, const float *__restrict__ E, int64_t es,
    float *__restrict__ D, int64_t ds, int rows, int cols, float *__restrict__ part) {
  __shared__ float red[STATS ? 3 * TOT * 64 : 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r0 = blockIdx.x * kSmRowsPerPart;
  const int r1 = min(rows, r0 + kSmRowsPerPart);
  float cs[STATS ? TOT : 1];
  if constexpr (STATS) {
#pragma unroll
    for (int j = 0; j < TOT; j++) cs[j] = 0.0f;
  }
  for (int r = r0 + w; r < r1; r += 4) {
    float p[TOT], e[TOT];
    load_row<V, TOT>(P + (int64_t)r * ps, cols, lane, 0.0f, p);
    load_row<V, TOT>(E + (int64_t)r * es, cols, lane, 0.0f, e);
    float dot = 0.0f;
#pragma unroll
    for (int j = 0; j < TOT; j++) {
      e[j] = p[j] * e[j];
      dot += e[j];
    }
    dot = wave_sum(dot);
#pragma unroll
    for (int j = 0; j < TOT; j++) {
      e[j] = e[j] - dot * p[j];
      if constexpr (STATS) cs[j] += p[j];
    }
    store_row<V, TOT>(D + (int64_t)r * ds, cols, lane, e);
  }
  if constexpr (STATS)
    part_colsum_store<V, TOT>(cs, red, lane, w, part + (int64_t)blockIdx.x * cols, cols);
}

__global__ __launch_bounds__(256) void softmax_backprop_block_kernel(
    const float *__restrict__ P, int64_t ps, const float *__restrict__ E, int64_t es,
    float *__restrict__ D, int64_t ds, int rows, int cols) {
  __shared__ float red[4];
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const float *p = P + (int64_t)r * ps, *e = E + (int64_t)r * es;
    float *d = D + (int64_t)r * ds;
    float dot = 0.0f;
    for (int c = threadIdx.x; c < cols; c += 256) dot += p[c] * e[c];
    dot = block_sum(dot, red);
    for (int c = threadIdx.x; c < cols; c += 256) d[c] = p[c] * e[c] - dot * p[c];
  }
}

// ---- N totals in a fixed order ---------------------------------------------------------
// {objective, weight} (N = 2) and {objective, weight, accuracy weight}
// (N = 3).  Each wave's terms (lane 0's: the caller has summed over the lanes
// where they differ) added in wave order into the block's partial.
template <int N>
__device__ __forceinline__ void block_terms_store(const double (&t)[N], double (*dred)[N],
                                                  double *__restrict__ part) {
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; k++) dred[threadIdx.x >> 6][k] = t[k];
  }
  __syncthreads();
  if (threadIdx.x < N)
    part[N * (size_t)blockIdx.x + threadIdx.x] =
        ((dred[0][threadIdx.x] + dred[1][threadIdx.x]) + dred[2][threadIdx.x]) +
        dred[3][threadIdx.x];
}

// tot[k] += the partials' term k: one wave, each lane its partials in order,
// then the cross-lane sum.
template <int N>
__device__ __forceinline__ void terms_final(const double *__restrict__ part, int nparts,
                                            double *__restrict__ tot) {
  double t[N] = {};
  for (int p = threadIdx.x; p < nparts; p += 64) {
#pragma unroll
    for (int k = 0; k < N; k++) t[k] += part[N * (size_t)p + k];
  }
#pragma unroll
  for (int k = 0; k < N; k++) t[k] = wave_sum(t[k]);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < N; k++) tot[k] += t[k];
  }
}
__global__ __launch_bounds__(64) void objf_final_kernel(const double *__restrict__ objf_part,
                                                        int nparts, double *__restrict__ tot) {
  terms_final<2>(objf_part, nparts, tot);
}
__global__ __launch_bounds__(64) void prob_final_kernel(const double *__restrict__ prob_part,
                                                        int nparts, double *__restrict__ tot) {
  terms_final<3>(prob_part, nparts, tot);
}

// ---- CompObjfAndDeriv ----------------------------------------------------------------
// deriv(row, col) += weight / A(row, col); elements outside the matrix are
// skipped (the hosts validate before they launch).
__global__ __launch_bounds__(256) void comp_objf_kernel(
    const int *__restrict__ el_row, const int *__restrict__ el_col,
    const float *__restrict__ el_w, int num, const float *__restrict__ A, int64_t as,
    float *__restrict__ deriv, int64_t ds, int rows, int cols, double *__restrict__ objf_part) {
  __shared__ double dred[4][2];
  const int e = blockIdx.x * 256 + threadIdx.x;
  double objf = 0.0, wsum = 0.0;
  if (e < num) {
    const int r = el_row[e], c = el_col[e];
    if (r >= 0 && r < rows && c >= 0 && c < cols) {
      const float w = el_w[e];
      const float a = A[(int64_t)r * as + c];
      deriv[(int64_t)r * ds + c] += __fdiv_rn(w, a);
      objf = (double)w * log((double)a);
      wsum = (double)w;
    }
  }
  block_terms_store<2>({wave_sum(objf), wave_sum(wsum)}, dred, objf_part);
}

// ---- Softmax + cross-entropy backward, fused -------------------------------------------
// Labels sorted by row, row r's at [row_start[r], row_start[r + 1]).  S_r =
// sum of the row's weights; D = -P S_r, + w at a label; the objective terms
// w log P at the labels; the column sums of P.  P read once, D written once.
template <int V, int TOT, bool STATS>
__global__ __launch_bounds__(256) void softmax_xent_wave_kernel(
    const float *__restrict__ P, int64_t ps, float *__restrict__ D, int64_t ds, int rows,
    int cols, const int *__restrict__ row_start, const int *__restrict__ lab_col,
    const float *__restrict__ lab_w, float *__restrict__ part, double *__restrict__ objf_part) {
  __shared__ float red[STATS ? 3 * TOT * 64 : 1];
  __shared__ double dred[4][2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r0 = blockIdx.x * kSmRowsPerPart;
  const int r1 = min(rows, r0 + kSmRowsPerPart);
  float cs[STATS ? TOT : 1];
  if constexpr (STATS) {
#pragma unroll
    for (int j = 0; j < TOT; j++) cs[j] = 0.0f;
  }
  double objf = 0.0, wsum = 0.0;
  for (int r = r0 + w; r < r1; r += 4) {
    const float *prow = P + (int64_t)r * ps;
    float p[TOT];
    load_row<V, TOT>(prow, cols, lane, 0.0f, p);
    const int lb = row_start[r], le = row_start[r + 1];
    float S = 0.0f;
    for (int l = lb; l < le; l++) S += lab_w[l];
#pragma unroll
    for (int j = 0; j < TOT; j++) {
      if constexpr (STATS) cs[j] += p[j];
      p[j] = -p[j] * S;
    }
    for (int l = lb; l < le; l++) {
      // the label's column is value t.j of lane t.lane: t.j is wave-uniform,
      // so the search over the register file is scalar compares
      const RowSlot t = row_slot<V>(__builtin_amdgcn_readfirstlane(lab_col[l]));
      const float lw = lab_w[l];  // every lane's load: not behind the one of lab_col
      const float add = lane == t.lane ? lw : 0.0f;
#pragma unroll
      for (int j = 0; j < TOT; j++)
        if (j == t.j) p[j] += add;
    }
    for (int l = lb + lane; l < le; l += 64) {
      const int c = lab_col[l];
      if (c >= 0 && c < cols) {
        const float lw = lab_w[l];
        objf += (double)lw * log((double)prow[c]);
        wsum += (double)lw;
      }
    }
    store_row<V, TOT>(D + (int64_t)r * ds, cols, lane, p);
  }
  if constexpr (STATS)
    part_colsum_store<V, TOT>(cs, red, lane, w, part + (int64_t)blockIdx.x * cols, cols);
  block_terms_store<2>({wave_sum(objf), wave_sum(wsum)}, dred, objf_part);
}

// The wide-row form: a block per row; partial r is the row's objective.
__global__ __launch_bounds__(256) void softmax_xent_block_kernel(
    const float *__restrict__ P, int64_t ps, float *__restrict__ D, int64_t ds, int rows,
    int cols, const int *__restrict__ row_start, const int *__restrict__ lab_col,
    const float *__restrict__ lab_w, double *__restrict__ objf_part) {
  __shared__ double dred[4][2];
  const int r = blockIdx.x;
  const float *p = P + (int64_t)r * ps;
  float *d = D + (int64_t)r * ds;
  const int lb = row_start[r], le = row_start[r + 1];
  float S = 0.0f;
  for (int l = lb; l < le; l++) S += lab_w[l];
  for (int c = threadIdx.x; c < cols; c += 256) d[c] = -p[c] * S;
  __syncthreads();  // the label elements are rewritten below by other threads
  double objf = 0.0, wsum = 0.0;
  for (int l = lb + (int)threadIdx.x; l < le; l += 256) {
    const int c = lab_col[l];
    if (c >= 0 && c < cols) {
      const float lw = lab_w[l];
      d[c] = -p[c] * S + lw;
      objf += (double)lw * log((double)p[c]);
      wsum += (double)lw;
    }
  }
  block_terms_store<2>({wave_sum(objf), wave_sum(wsum)}, dred, objf_part);
}

// ---- objective and frame accuracy, forward only (nnet-compute-prob) ----------------------
// CuMatrixBase::FindRowMaxId: a row's best column is the lowest column whose
// value is greater than every earlier column's, the comparison starting from
// -1e21; a NaN is never greater, and a row with no such column has none
// (kNoBest).  That is the first column holding the largest value above -1e21.
constexpr float kRowMaxStart = -1.0e21f;
constexpr int kNoBest = 0x7fffffff;

struct RowBest {
  float v;
  int c;
};
// a's columns all come before b's, or the two are merged by (value, column)
__device__ __forceinline__ RowBest better(RowBest a, RowBest b) {
  return (b.v > a.v || (b.v == a.v && b.c < a.c)) ? b : a;
}
__device__ __forceinline__ RowBest wave_best(RowBest a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    RowBest b;
    b.v = __shfl_xor(a.v, o);
    b.c = __shfl_xor(a.c, o);
    a = better(a, b);
  }
  return a;
}

// One wave per row, four rows to a block, the row in registers.  SOFTMAX: the
// row holds logits and P is formed by softmax_row and never stored; else the
// row holds P.  Then the row's best column, and per label w log P, w, and w
// where the label is the best column.  A row without labels is not read.
// Every lane carries the same totals.
template <int V, int TOT, bool SOFTMAX>
__global__ __launch_bounds__(256) void objf_accuracy_wave_kernel(
    const float *__restrict__ X, int64_t xs, int rows, int cols,
    const int *__restrict__ row_start, const int *__restrict__ lab_col,
    const float *__restrict__ lab_w, double *__restrict__ prob_part) {
  __shared__ double dred[4][3];
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  double objf = 0.0, wsum = 0.0, acc = 0.0;
  const int lb = r < rows ? row_start[r] : 0, le = r < rows ? row_start[r + 1] : 0;
  if (lb < le) {
    float v[TOT];
    load_row<V, TOT>(X + (int64_t)r * xs, cols, lane, -INFINITY, v);
    if constexpr (SOFTMAX) softmax_row<TOT>(v);
    RowBest best{kRowMaxStart, kNoBest};
#pragma unroll
    for (int j = 0; j < TOT; j++) {  // a lane's columns ascend with j
      const int c = row_col<V, TOT>(lane, j);
      if (c < cols && v[j] > best.v) best = RowBest{v[j], c};
    }
    best = wave_best(best);
    for (int l = lb; l < le; l++) {
      const int c = __builtin_amdgcn_readfirstlane(lab_col[l]);
      if (c < 0 || c >= cols) continue;  // (the hosts validate before they launch)
      const float lw = lab_w[l];
      objf += (double)lw * log((double)row_value_at<V, TOT>(v, c));
      wsum += (double)lw;
      if (c == best.c) acc += (double)lw;
    }
  }
  block_terms_store<3>({objf, wsum, acc}, dred, prob_part);
}

// The four waves' best columns of a block, merged in wave order.
__device__ __forceinline__ RowBest block_best(RowBest b, RowBest *bred) {
  b = wave_best(b);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) bred[threadIdx.x >> 6] = b;
  __syncthreads();
  return better(better(bred[0], bred[1]), better(bred[2], bred[3]));
}

// The wide-row form: a block per row.  SOFTMAX forms each P value as
// softmax_prop_block_kernel does, from logits read three times.
template <bool SOFTMAX>
__global__ __launch_bounds__(256) void objf_accuracy_block_kernel(
    const float *__restrict__ X, int64_t xs, int rows, int cols,
    const int *__restrict__ row_start, const int *__restrict__ lab_col,
    const float *__restrict__ lab_w, double *__restrict__ prob_part) {
  __shared__ float red[4];
  __shared__ RowBest bred[4];
  __shared__ double dred[4][3];
  const int r = blockIdx.x;
  const float *x = X + (int64_t)r * xs;
  const int lb = row_start[r], le = row_start[r + 1];
  double objf = 0.0, wsum = 0.0, acc = 0.0;
  if (lb < le) {  // block-uniform
    RowMaxSum ms{0.0f, 1.0f};
    if constexpr (SOFTMAX) ms = softmax_max_sum(x, cols, red);
    auto prob = [&](int c) {
      if constexpr (SOFTMAX) return softmax_value(x[c], ms);
      else return x[c];
    };
    RowBest best{kRowMaxStart, kNoBest};
    for (int c = threadIdx.x; c < cols; c += 256) {
      const float y = prob(c);
      if (y > best.v) best = RowBest{y, c};
    }
    best = block_best(best, bred);
    for (int l = lb + (int)threadIdx.x; l < le; l += 256) {
      const int c = lab_col[l];
      if (c < 0 || c >= cols) continue;
      const float lw = lab_w[l];
      objf += (double)lw * log((double)prob(c));
      wsum += (double)lw;
      if (c == best.c) acc += (double)lw;
    }
    objf = wave_sum(objf);
    wsum = wave_sum(wsum);
    acc = wave_sum(acc);
  }
  block_terms_store<3>({objf, wsum, acc}, dred, prob_part);
}

// ---- log-likelihoods (nnet-am-compute --apply-log --divide-by-priors) ----------------------
// ApplyFloor(1e-20) (NaN stays), the fp64 log of the fp32 probability, one
// fp64 subtraction of the column's offset (prior_scale * log prior, formed
// on the host; 0 without priors) and one rounding to fp32.
__device__ __forceinline__ float loglike(float p, double offset) {
  if (p < kSoftmaxFloor) p = kSoftmaxFloor;
  return (float)(log((double)p) - offset);
}

// A stored P, element-wise: 256 consecutive columns x rows grid-strided.
__global__ __launch_bounds__(256) void loglikes_kernel(const float *__restrict__ P, int64_t ps,
                                                       float *__restrict__ out, int64_t os,
                                                       int rows, int cols,
                                                       const double *__restrict__ offset) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  const double off = offset ? offset[c] : 0.0;
  for (int r = blockIdx.y; r < rows; r += gridDim.y)
    out[(int64_t)r * os + c] = loglike(P[(int64_t)r * ps + c], off);
}

// From the logits of a last SoftmaxComponent: P formed in registers by
// softmax_row's two steps and never stored.  (loglike floors the floored P
// again, which changes nothing.)
template <int V, int TOT>
__global__ __launch_bounds__(256) void softmax_loglikes_wave_kernel(
    const float *__restrict__ in, int64_t is, float *__restrict__ out, int64_t os, int rows,
    int cols, const double *__restrict__ offset) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float v[TOT];
  load_row<V, TOT>(in + (int64_t)r * is, cols, lane, -INFINITY, v);
  const float s = softmax_row_exp<TOT>(v);
#pragma unroll
  for (int j = 0; j < TOT; j++) {
    const int c = row_col<V, TOT>(lane, j);
    if (c < cols) v[j] = loglike(softmax_quotient(v[j], s), offset ? offset[c] : 0.0);
  }
  store_row<V, TOT>(out + (int64_t)r * os, cols, lane, v);
}

// The wide-row form, as softmax_prop_block_kernel.
__global__ __launch_bounds__(256) void softmax_loglikes_block_kernel(
    const float *__restrict__ in, int64_t is, float *__restrict__ out, int64_t os, int rows,
    int cols, const double *__restrict__ offset) {
  __shared__ float red[4];
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const float *x = in + (int64_t)r * is;
    float *y = out + (int64_t)r * os;
    const RowMaxSum ms = softmax_max_sum(x, cols, red);
    for (int c = threadIdx.x; c < cols; c += 256)
      y[c] = loglike(softmax_value(x[c], ms), offset ? offset[c] : 0.0);
  }
}

// ---- Dropout -----------------------------------------------------------------------------
struct Philox4 { uint32_t x, y, z, w; };

// Philox4x32-10 (Salmon et al., SC'11).
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2,
                                                 uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{c0, c1, c2, c3};
}

struct DropoutArgs {
  float dp, hl, low;   // proportion, high - low, low
  int scale_hl, add_low;
  uint32_t k0, k1, call_lo, call_hi;
  uint32_t row0;  // the matrix's first row in the minibatch the mask is drawn for
};

// The reference's sequence on one uniform draw (nnet-component.cc:3613-3622):
// Add(-dp), ApplyHeaviside, Scale(high - low) unless 1, Add(low) unless 0.
__device__ __forceinline__ float dropout_mask(uint32_t x, const DropoutArgs &a) {
  const float u = (float)(x >> 8) * 5.9604644775390625e-8f;  // 2^-24, exact
  float h = (u - a.dp) > 0.0f ? 1.0f : 0.0f;
  if (a.scale_hl) h *= a.hl;
  if (a.add_low) h += a.low;
  return h;
}

// A thread per (row, block of four columns): one Philox call, one 16-byte
// (VEC4) or four 4-byte accesses each way.
template <bool VEC4>
__global__ __launch_bounds__(256) void dropout_prop_kernel(const float *__restrict__ in,
                                                           int64_t is, float *__restrict__ out,
                                                           int64_t os, int cols, FastDiv div_ncb,
                                                           int64_t total, DropoutArgs a) {
  // high == low: every mask value is the same and no draw is needed
  const bool flat = a.scale_hl && a.hl == 0.0f;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * 256) {
    uint32_t row, cb;
    div_ncb.divmod((uint32_t)e, row, cb);
    float m[4];
    if (flat) {
      float h = 0.0f * a.hl;
      if (a.add_low) h += a.low;
      m[0] = m[1] = m[2] = m[3] = h;
    } else {
      const Philox4 x = philox4x32_10(cb, a.row0 + row, a.call_lo, a.call_hi, a.k0, a.k1);
      m[0] = dropout_mask(x.x, a);
      m[1] = dropout_mask(x.y, a);
      m[2] = dropout_mask(x.z, a);
      m[3] = dropout_mask(x.w, a);
    }
    const int c = (int)cb * 4;
    const float *x = in + (int64_t)row * is + c;
    float *y = out + (int64_t)row * os + c;
    if (VEC4 && c + 4 <= cols) {
      const float4 v = *reinterpret_cast<const float4 *>(x);
      *reinterpret_cast<float4 *>(y) = make_float4(m[0] * v.x, m[1] * v.y, m[2] * v.z, m[3] * v.w);
    } else {
#pragma unroll
      for (int s = 0; s < 4; s++)
        if (c + s < cols) y[s] = m[s] * x[s];
    }
  }
}

// AddMatMatDivMat: in_value == 0 ? out_deriv : out_deriv * out_value / in_value
// (the product first, then an IEEE divide).
__device__ __forceinline__ float dropout_dx(float od, float ov, float iv) {
  return iv == 0.0f ? od : __fdiv_rn(__fmul_rn(od, ov), iv);
}

__global__ __launch_bounds__(256) void dropout_backprop_kernel(
    const float *__restrict__ iv, int64_t ivs, const float *__restrict__ ov, int64_t ovs,
    const float *__restrict__ od, int64_t ods, float *__restrict__ id, int64_t ids, int rows,
    int cols) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  for (int r = blockIdx.y; r < rows; r += gridDim.y)
    id[(int64_t)r * ids + c] =
        dropout_dx(od[(int64_t)r * ods + c], ov[(int64_t)r * ovs + c], iv[(int64_t)r * ivs + c]);
}

__global__ __launch_bounds__(256) void dropout_backprop4_kernel(
    const float *__restrict__ iv, int64_t ivs, const float *__restrict__ ov, int64_t ovs,
    const float *__restrict__ od, int64_t ods, float *__restrict__ id, int64_t ids, int rows,
    int cols) {
  const int c = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (c >= cols) return;
  for (int r = blockIdx.y; r < rows; r += gridDim.y) {
    const float4 i = *reinterpret_cast<const float4 *>(iv + (int64_t)r * ivs + c);
    const float4 o = *reinterpret_cast<const float4 *>(ov + (int64_t)r * ovs + c);
    const float4 d = *reinterpret_cast<const float4 *>(od + (int64_t)r * ods + c);
    *reinterpret_cast<float4 *>(id + (int64_t)r * ids + c) =
        make_float4(dropout_dx(d.x, o.x, i.x), dropout_dx(d.y, o.y, i.y),
                    dropout_dx(d.z, o.z, i.z), dropout_dx(d.w, o.w, i.w));
  }
}

// ---- host side -------------------------------------------------------------------------------
// Values a lane holds (the kernels are built for 4, 16 and 64).
int lane_values(int cols) { return cols <= 256 ? 4 : cols <= 1024 ? 16 : 64; }

int wave_parts(int rows) { return (rows + kSmRowsPerPart - 1) / kSmRowsPerPart; }

}  // namespace

extern "C" {

int kn_softmax_prop(const float *in, MatrixDim in_dim, float *out, MatrixDim out_dim,
                    kcnn_stream_t st) {
  if (!same_shape(in_dim, out_dim) || !contiguous_enough(in_dim) ||
      !contiguous_enough(out_dim))
    return (int)hipErrorInvalidValue;
  const int rows = in_dim.rows, cols = in_dim.cols;
  if (rows == 0 || cols == 0) return 0;
  hipStream_t s = kcnn::as_stream(st);
  if (cols > kWaveRowMaxCols) {
    hipLaunchKernelGGL(softmax_prop_block_kernel, dim3(row_blocks(rows)), dim3(256), 0, s, in,
                       (int64_t)in_dim.stride, out, (int64_t)out_dim.stride, rows, cols);
    return kcnn::launch_status();
  }
  const Operand ops[] = {{in, in_dim.stride}, {out, out_dim.stride}};
  dispatch_kernel<4, 16, 64>(lane_width(ops), lane_values(cols), [&](auto V, auto TOT) {
    hipLaunchKernelGGL((softmax_prop_wave_kernel<decltype(V)::value, decltype(TOT)::value>),
                       dim3((rows + 3) / 4), dim3(256), 0, s, in, (int64_t)in_dim.stride, out,
                       (int64_t)out_dim.stride, rows, cols);
  });
  return kcnn::launch_status();
}

size_t kn_softmax_stats_ws(MatrixDim dim) {
  return (size_t)(wave_parts(dim.rows) > 0 ? wave_parts(dim.rows) : 1) *
         (dim.cols > 0 ? dim.cols : 1) * sizeof(float);
}

}  // extern "C"

namespace {
// The column sums of P for the wide-row path (the wave kernels make their
// parts themselves), then the ordered final pass either way.
int finish_colsum(const float *P, MatrixDim p_dim, bool wide, double *value_sum, float *part,
                  hipStream_t s) {
  int nparts = wave_parts(p_dim.rows);
  if (wide) {
    nparts = (p_dim.rows + kColRowsPerPart - 1) / kColRowsPerPart;
    hipLaunchKernelGGL(colsum_part_kernel, dim3((p_dim.cols + 255) / 256, nparts), dim3(256), 0,
                       s, P, (int64_t)p_dim.stride, p_dim.rows, p_dim.cols, part);
    const int rc = kcnn::launch_status();
    if (rc) return rc;
  }
  hipLaunchKernelGGL(colsum_final_kernel, dim3((p_dim.cols + 63) / 64), dim3(64 * kFinalWaves),
                     0, s, part, nparts, p_dim.cols, value_sum);
  return kcnn::launch_status();
}
}  // namespace

extern "C" {

int kn_softmax_backprop(const float *out_value, MatrixDim ov_dim, const float *out_deriv,
                        MatrixDim od_dim, float *in_deriv, MatrixDim id_dim, double *value_sum,
                        void *ws, kcnn_stream_t st) {
  if (!same_shape(ov_dim, od_dim) || !same_shape(id_dim, od_dim) ||
      !contiguous_enough(ov_dim) || !contiguous_enough(od_dim) || !contiguous_enough(id_dim))
    return (int)hipErrorInvalidValue;
  const int rows = od_dim.rows, cols = od_dim.cols;
  if (rows == 0 || cols == 0) return 0;
  const bool stats = value_sum != nullptr;
  if (stats && ws == nullptr) return (int)hipErrorInvalidValue;
  float *part = static_cast<float *>(ws);
  hipStream_t s = kcnn::as_stream(st);
  const bool wide = cols > kWaveRowMaxCols;
  if (wide) {
    hipLaunchKernelGGL(softmax_backprop_block_kernel, dim3(row_blocks(rows)), dim3(256), 0, s,
                       out_value, (int64_t)ov_dim.stride, out_deriv, (int64_t)od_dim.stride,
                       in_deriv, (int64_t)id_dim.stride, rows, cols);
  } else {
    const Operand ops[] = {
        {out_value, ov_dim.stride}, {out_deriv, od_dim.stride}, {in_deriv, id_dim.stride}};
    dispatch_kernel<4, 16, 64>(lane_width(ops), lane_values(cols), [&](auto V, auto TOT) {
      kcnn::with_bool(stats, [&](auto STATS) {
        hipLaunchKernelGGL((softmax_backprop_wave_kernel<decltype(V)::value, decltype(TOT)::value,
                                                         decltype(STATS)::value>),
                           dim3(wave_parts(rows)), dim3(256), 0, s, out_value,
                           (int64_t)ov_dim.stride, out_deriv, (int64_t)od_dim.stride, in_deriv,
                           (int64_t)id_dim.stride, rows, cols, part);
      });
    });
  }
  const int rc = kcnn::launch_status();
  if (rc || !stats) return rc;
  return finish_colsum(out_value, ov_dim, wide, value_sum, part, s);
}

size_t kn_objf_ws(int num_blocks) {
  return (size_t)2 * (num_blocks > 0 ? num_blocks : 1) * sizeof(double);
}

int kn_comp_objf_blocks(int num) { return (num + 255) / 256; }

int kn_comp_objf_and_deriv(const int *el_row, const int *el_col, const float *el_w, int num,
                           const float *probs, MatrixDim p_dim, float *deriv, MatrixDim d_dim,
                           double *tot, void *ws, kcnn_stream_t st) {
  if (!same_shape(p_dim, d_dim) || num < 0 || tot == nullptr)
    return (int)hipErrorInvalidValue;
  if (num == 0) return 0;
  if (ws == nullptr) return (int)hipErrorInvalidValue;
  hipStream_t s = kcnn::as_stream(st);
  const int nb = kn_comp_objf_blocks(num);
  double *objf_part = static_cast<double *>(ws);
  hipLaunchKernelGGL(comp_objf_kernel, dim3(nb), dim3(256), 0, s, el_row, el_col, el_w, num,
                     probs, (int64_t)p_dim.stride, deriv, (int64_t)d_dim.stride, p_dim.rows,
                     p_dim.cols, objf_part);
  const int rc = kcnn::launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(objf_final_kernel, dim3(1), dim3(64), 0, s, objf_part, nb, tot);
  return kcnn::launch_status();
}

int kn_softmax_xent_blocks(MatrixDim dim) {
  return dim.cols > kWaveRowMaxCols ? dim.rows : wave_parts(dim.rows);
}

int kn_softmax_xent_backprop(const float *out_value, MatrixDim ov_dim, float *in_deriv,
                             MatrixDim id_dim, const int *row_start, const int *lab_col,
                             const float *lab_w, double *value_sum, void *stats_ws, double *tot,
                             void *objf_ws, kcnn_stream_t st) {
  if (!same_shape(ov_dim, id_dim) || !contiguous_enough(ov_dim) ||
      !contiguous_enough(id_dim) || tot == nullptr || objf_ws == nullptr ||
      row_start == nullptr)
    return (int)hipErrorInvalidValue;
  const int rows = ov_dim.rows, cols = ov_dim.cols;
  if (rows == 0 || cols == 0) return 0;
  const bool stats = value_sum != nullptr;
  if (stats && stats_ws == nullptr) return (int)hipErrorInvalidValue;
  float *part = static_cast<float *>(stats_ws);
  double *objf_part = static_cast<double *>(objf_ws);
  hipStream_t s = kcnn::as_stream(st);
  const bool wide = cols > kWaveRowMaxCols;
  const int nb = kn_softmax_xent_blocks(ov_dim);
  if (wide) {
    hipLaunchKernelGGL(softmax_xent_block_kernel, dim3(nb), dim3(256), 0, s, out_value,
                       (int64_t)ov_dim.stride, in_deriv, (int64_t)id_dim.stride, rows, cols,
                       row_start, lab_col, lab_w, objf_part);
  } else {
    const Operand ops[] = {{out_value, ov_dim.stride}, {in_deriv, id_dim.stride}};
    dispatch_kernel<4, 16, 64>(lane_width(ops), lane_values(cols), [&](auto V, auto TOT) {
      kcnn::with_bool(stats, [&](auto STATS) {
        hipLaunchKernelGGL((softmax_xent_wave_kernel<decltype(V)::value, decltype(TOT)::value,
                                                     decltype(STATS)::value>),
                           dim3(nb), dim3(256), 0, s, out_value, (int64_t)ov_dim.stride, in_deriv,
                           (int64_t)id_dim.stride, rows, cols, row_start, lab_col, lab_w, part,
                           objf_part);
      });
    });
  }
  int rc = kcnn::launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(objf_final_kernel, dim3(1), dim3(64), 0, s, objf_part, nb, tot);
  rc = kcnn::launch_status();
  if (rc || !stats) return rc;
  return finish_colsum(out_value, ov_dim, wide, value_sum, part, s);
}

}  // extern "C"

namespace {
template <bool SOFTMAX>
int launch_objf_accuracy(const float *x, MatrixDim dim, const int *row_start, const int *lab_col,
                         const float *lab_w, double *tot, void *ws, kcnn_stream_t st) {
  if (!contiguous_enough(dim) || tot == nullptr || ws == nullptr || row_start == nullptr)
    return (int)hipErrorInvalidValue;
  const int rows = dim.rows, cols = dim.cols;
  if (rows == 0 || cols == 0) return 0;
  double *prob_part = static_cast<double *>(ws);
  hipStream_t s = kcnn::as_stream(st);
  const int nb = kn_prob_blocks(dim);
  if (cols > kWaveRowMaxCols) {
    hipLaunchKernelGGL(objf_accuracy_block_kernel<SOFTMAX>, dim3(nb), dim3(256), 0, s, x,
                       (int64_t)dim.stride, rows, cols, row_start, lab_col, lab_w, prob_part);
  } else {
    const Operand ops[] = {{x, dim.stride}};
    dispatch_kernel<4, 16, 64>(lane_width(ops), lane_values(cols), [&](auto V, auto TOT) {
      hipLaunchKernelGGL(
          (objf_accuracy_wave_kernel<decltype(V)::value, decltype(TOT)::value, SOFTMAX>),
          dim3(nb), dim3(256), 0, s, x, (int64_t)dim.stride, rows, cols, row_start, lab_col,
          lab_w, prob_part);
    });
  }
  const int rc = kcnn::launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(prob_final_kernel, dim3(1), dim3(64), 0, s, prob_part, nb, tot);
  return kcnn::launch_status();
}
}  // namespace

extern "C" {

int kn_prob_blocks(MatrixDim dim) {
  return dim.cols > kWaveRowMaxCols ? dim.rows : (dim.rows + 3) / 4;
}

size_t kn_prob_ws(int num_blocks) {
  return (size_t)3 * (num_blocks > 0 ? num_blocks : 1) * sizeof(double);
}

int kn_objf_accuracy(const float *probs, MatrixDim p_dim, const int *row_start,
                     const int *lab_col, const float *lab_w, double *tot, void *ws,
                     kcnn_stream_t st) {
  return launch_objf_accuracy<false>(probs, p_dim, row_start, lab_col, lab_w, tot, ws, st);
}

int kn_softmax_objf_accuracy(const float *logits, MatrixDim l_dim, const int *row_start,
                             const int *lab_col, const float *lab_w, double *tot, void *ws,
                             kcnn_stream_t st) {
  return launch_objf_accuracy<true>(logits, l_dim, row_start, lab_col, lab_w, tot, ws, st);
}

int kn_loglikes(const float *probs, MatrixDim p_dim, float *out, MatrixDim out_dim,
                const double *offset, kcnn_stream_t st) {
  if (!same_shape(p_dim, out_dim) || !contiguous_enough(p_dim) || !contiguous_enough(out_dim))
    return (int)hipErrorInvalidValue;
  const int rows = p_dim.rows, cols = p_dim.cols;
  if (rows == 0 || cols == 0) return 0;
  hipLaunchKernelGGL(loglikes_kernel, kcnn::elementwise_grid(rows, cols, 256), dim3(256), 0,
                     kcnn::as_stream(st), probs, (int64_t)p_dim.stride, out,
                     (int64_t)out_dim.stride, rows, cols, offset);
  return kcnn::launch_status();
}

int kn_softmax_loglikes(const float *logits, MatrixDim l_dim, float *out, MatrixDim out_dim,
                        const double *offset, kcnn_stream_t st) {
  if (!same_shape(l_dim, out_dim) || !contiguous_enough(l_dim) || !contiguous_enough(out_dim))
    return (int)hipErrorInvalidValue;
  const int rows = l_dim.rows, cols = l_dim.cols;
  if (rows == 0 || cols == 0) return 0;
  hipStream_t s = kcnn::as_stream(st);
  if (cols > kWaveRowMaxCols) {
    hipLaunchKernelGGL(softmax_loglikes_block_kernel, dim3(row_blocks(rows)), dim3(256), 0, s,
                       logits, (int64_t)l_dim.stride, out, (int64_t)out_dim.stride, rows, cols,
                       offset);
    return kcnn::launch_status();
  }
  const Operand ops[] = {{logits, l_dim.stride}, {out, out_dim.stride}};
  dispatch_kernel<4, 16, 64>(lane_width(ops), lane_values(cols), [&](auto V, auto TOT) {
    hipLaunchKernelGGL((softmax_loglikes_wave_kernel<decltype(V)::value, decltype(TOT)::value>),
                       dim3((rows + 3) / 4), dim3(256), 0, s, logits, (int64_t)l_dim.stride, out,
                       (int64_t)out_dim.stride, rows, cols, offset);
  });
  return kcnn::launch_status();
}

int kn_dropout_prop(const float *in, MatrixDim in_dim, float *out, MatrixDim out_dim,
                    float dropout_proportion, float high_minus_low, float low, uint64_t seed,
                    uint64_t call, int64_t row_offset, kcnn_stream_t st) {
  if (!same_shape(in_dim, out_dim) || !contiguous_enough(in_dim) ||
      !contiguous_enough(out_dim))
    return (int)hipErrorInvalidValue;
  const int rows = in_dim.rows, cols = in_dim.cols;
  // the counter word row_offset + row must not wrap: two rows would share a mask
  if (rows < 0 || row_offset < 0 || row_offset > ((int64_t)1 << 32) - rows)
    return (int)hipErrorInvalidValue;
  if (rows == 0 || cols == 0) return 0;
  const int ncb = (cols + 3) / 4;
  const int64_t total = (int64_t)rows * ncb;
  if (total >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
  DropoutArgs a;
  a.dp = dropout_proportion;
  a.hl = high_minus_low;
  a.low = low;
  a.scale_hl = high_minus_low != 1.0f;
  a.add_low = low != 0.0f;
  a.k0 = (uint32_t)seed;
  a.k1 = (uint32_t)(seed >> 32);
  a.call_lo = (uint32_t)call;
  a.call_hi = (uint32_t)(call >> 32);
  a.row0 = (uint32_t)row_offset;
  const bool vec4 = in_dim.stride % 4 == 0 && out_dim.stride % 4 == 0 &&
                    (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0;
  hipStream_t s = kcnn::as_stream(st);
  if (vec4)
    hipLaunchKernelGGL(dropout_prop_kernel<true>, dim3(kcnn::grid_for(total)), dim3(256), 0, s,
                       in, (int64_t)in_dim.stride, out, (int64_t)out_dim.stride, cols,
                       FastDiv((uint32_t)ncb), total, a);
  else
    hipLaunchKernelGGL(dropout_prop_kernel<false>, dim3(kcnn::grid_for(total)), dim3(256), 0, s,
                       in, (int64_t)in_dim.stride, out, (int64_t)out_dim.stride, cols,
                       FastDiv((uint32_t)ncb), total, a);
  return kcnn::launch_status();
}

int kn_dropout_backprop(const float *in_value, MatrixDim iv_dim, const float *out_value,
                        MatrixDim ov_dim, const float *out_deriv, MatrixDim od_dim,
                        float *in_deriv, MatrixDim id_dim, kcnn_stream_t st) {
  if (!same_shape(iv_dim, od_dim) || !same_shape(ov_dim, od_dim) || !same_shape(id_dim, od_dim))
    return (int)hipErrorInvalidValue;
  const int rows = od_dim.rows, cols = od_dim.cols;
  if (rows == 0 || cols == 0) return 0;
  const bool vec4 = cols % 4 == 0 && iv_dim.stride % 4 == 0 && ov_dim.stride % 4 == 0 &&
                    od_dim.stride % 4 == 0 && id_dim.stride % 4 == 0 &&
                    (uintptr_t)in_value % 16 == 0 && (uintptr_t)out_value % 16 == 0 &&
                    (uintptr_t)out_deriv % 16 == 0 && (uintptr_t)in_deriv % 16 == 0;
  const int cpb = vec4 ? 1024 : 256;
  const dim3 grid = kcnn::elementwise_grid(rows, cols, cpb);
  hipStream_t s = kcnn::as_stream(st);
  if (vec4)
    hipLaunchKernelGGL(dropout_backprop4_kernel, grid, dim3(256), 0, s, in_value,
                       (int64_t)iv_dim.stride, out_value, (int64_t)ov_dim.stride, out_deriv,
                       (int64_t)od_dim.stride, in_deriv, (int64_t)id_dim.stride, rows, cols);
  else
    hipLaunchKernelGGL(dropout_backprop_kernel, grid, dim3(256), 0, s, in_value,
                       (int64_t)iv_dim.stride, out_value, (int64_t)ov_dim.stride, out_deriv,
                       (int64_t)od_dim.stride, in_deriv, (int64_t)id_dim.stride, rows, cols);
  return kcnn::launch_status();
}

}  // extern "C"
