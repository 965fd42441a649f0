// nnet2/row-regs.h -- a matrix row held in registers, shared by the row
// kernels of nnet-loss-kernels.hip (Softmax) and nnet-normalize-kernels.hip
// (NormalizeComponent):
//   * the cross-lane and four-wave block reductions;
//   * the row <-> register mapping both ways (row_col, row_slot), load_row and
//     store_row, and the access to one wave-uniform column of a held row;
//   * the softmax of a row, once for a row in a wave's registers and once for
//     a block that re-reads its row: every kernel that forms P calls these;
//   * host side: the choice of the access width and the runtime-to-template
//     kernel dispatcher.
#ifndef KCNN_NNET2_ROW_REGS_H_
#define KCNN_NNET2_ROW_REGS_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

namespace kcnn {
namespace rowregs {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// The four waves' values of a 256-thread block, combined in wave order.
constexpr int kBlock = 256;
__device__ __forceinline__ float block_max(float v, float *red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float block_sum(float v, float *red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- a row in the registers of LANES threads ----------------------------------
// TOT values a thread, as TOT / V vectors of V consecutive columns: value
// k * V + s of thread `lane` is column (k * LANES + lane) * V + s.  LANES is
// 64 for a row in one wave, the block size for a row across a block's waves.
// A vector that crosses the row's end is accessed element by element.
template <int V, int TOT, int LANES = 64>
__device__ __forceinline__ int row_col(int lane, int j) {
  return ((j / V) * LANES + lane) * V + (j % V);
}

template <int V, int TOT, int LANES = 64>
__device__ __forceinline__ void load_row(const float *__restrict__ row, int cols, int lane,
                                         float fill, float (&v)[TOT]) {
#pragma unroll
  for (int k = 0; k < TOT / V; k++) {
    const int c = (k * LANES + lane) * V;
    if (c + V <= cols) {
      if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(row + c);
        v[k * 4] = t.x; v[k * 4 + 1] = t.y; v[k * 4 + 2] = t.z; v[k * 4 + 3] = t.w;
      } else if constexpr (V == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(row + c);
        v[k * 2] = t.x; v[k * 2 + 1] = t.y;
      } else {
        v[k] = row[c];
      }
    } else {
#pragma unroll
      for (int s = 0; s < V; s++) v[k * V + s] = c + s < cols ? row[c + s] : fill;
    }
  }
}

template <int V, int TOT, int LANES = 64>
__device__ __forceinline__ void store_row(float *__restrict__ row, int cols, int lane,
                                          const float (&v)[TOT]) {
#pragma unroll
  for (int k = 0; k < TOT / V; k++) {
    const int c = (k * LANES + lane) * V;
    if (c + V <= cols) {
      if constexpr (V == 4) {
        *reinterpret_cast<float4 *>(row + c) =
            make_float4(v[k * 4], v[k * 4 + 1], v[k * 4 + 2], v[k * 4 + 3]);
      } else if constexpr (V == 2) {
        *reinterpret_cast<float2 *>(row + c) = make_float2(v[k * 2], v[k * 2 + 1]);
      } else {
        row[c] = v[k];
      }
    } else {
#pragma unroll
      for (int s = 0; s < V; s++)
        if (c + s < cols) row[c + s] = v[k * V + s];
    }
  }
}

constexpr int kWaveRowMaxCols = 4096;  // 64 lanes x 64 values

// The inverse of row_col for a row in one wave: column c is value j of `lane`.
struct RowSlot {
  int lane, j;
};
template <int V>
__device__ __forceinline__ RowSlot row_slot(int c) {
  const int q = c / V;
  const int j = (q >> 6) * V + c % V;
  return RowSlot{q & 63, j};
}

// The value at wave-uniform column c of a held row, in every lane: c's j is
// wave-uniform too, so the search over the register file is scalar compares.
// (A kernel that writes at a slot keeps that loop in its own body: through a
// reference parameter the compiler merges the stores into one indexed store
// and the row leaves the registers for scratch.)
template <int V, int TOT>
__device__ __forceinline__ float row_value_at(const float (&v)[TOT], int c) {
  const RowSlot t = row_slot<V>(c);
  float x = 0.0f;
#pragma unroll
  for (int j = 0; j < TOT; j++)
    if (j == t.j) x = v[j];
  return __shfl(x, t.lane);
}

// ---- the softmax of a row ----------------------------------------------------------
constexpr float kSoftmaxFloor = 1.0e-20f;

// A row that load_row filled with -INFINITY becomes exp(v - max); the sum of
// those is returned.
template <int TOT>
__device__ __forceinline__ float softmax_row_exp(float (&v)[TOT]) {
  float m = v[0];
#pragma unroll
  for (int j = 1; j < TOT; j++) m = fmaxf(m, v[j]);
  m = wave_max(m);
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < TOT; j++) {
    v[j] = expf(v[j] - m);  // the accurate exp: the 1e-5 bar holds down to x - m = -46
    s += v[j];
  }
  return wave_sum(s);
}
// The probability from an exp(x - max) and the row's sum.
__device__ __forceinline__ float softmax_quotient(float e, float s) {
  float y = e / s;
  if (y < kSoftmaxFloor) y = kSoftmaxFloor;  // ApplyFloor(1e-20); NaN stays
  return y;
}
// The same row becomes its probabilities.
template <int TOT>
__device__ __forceinline__ void softmax_row(float (&v)[TOT]) {
  const float s = softmax_row_exp<TOT>(v);
#pragma unroll
  for (int j = 0; j < TOT; j++) v[j] = softmax_quotient(v[j], s);
}

// The block-per-row form for rows wider than a wave holds: the row's max and
// sum from two reads by a block of kBlock threads, then each probability from
// a third.
struct RowMaxSum {
  float m, s;
};
__device__ __forceinline__ RowMaxSum softmax_max_sum(const float *__restrict__ x, int cols,
                                                     float *red) {
  float m = -INFINITY;
  for (int c = threadIdx.x; c < cols; c += kBlock) m = fmaxf(m, x[c]);
  m = block_max(m, red);
  float s = 0.0f;
  for (int c = threadIdx.x; c < cols; c += kBlock) s += expf(x[c] - m);
  s = block_sum(s, red);
  return RowMaxSum{m, s};
}
__device__ __forceinline__ float softmax_value(float x, RowMaxSum ms) {
  return softmax_quotient(expf(x - ms.m), ms.s);
}

// ---- host side -----------------------------------------------------------------
struct Operand {
  const void *p;
  int stride;
};

// Columns a lane takes at once: 4 (16-byte accesses) when every operand's
// base and row stride allow, else 2, else 1.
template <size_t N>
int lane_width(const Operand (&ops)[N]) {
  int v = 4;
  for (const Operand &o : ops) {
    while (v > 1 && ((uintptr_t)o.p % (4 * v) != 0 || o.stride % v != 0)) v >>= 1;
  }
  return v;
}

inline unsigned row_blocks(int rows) { return (unsigned)(rows < 65535 ? rows : 65535); }

// f(V, TOT) as integral constants, for the one of TOTS that tot is.
template <int... TOTS, typename F>
void dispatch_kernel(int v, int tot, F f) {
  auto with_v = [&](auto vc) {
    (void)((tot == TOTS && (f(vc, std::integral_constant<int, TOTS>{}), true)) || ...);
  };
  if (v == 4) with_v(std::integral_constant<int, 4>{});
  else if (v == 2) with_v(std::integral_constant<int, 2>{});
  else with_v(std::integral_constant<int, 1>{});
}

}  // namespace rowregs
}  // namespace kcnn

#endif  // KCNN_NNET2_ROW_REGS_H_
