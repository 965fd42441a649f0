// nnet2/row-regs.h -- a matrix row held in registers: the cross-lane
// reductions, the row <-> register mapping and the host-side choice of the
// access width, shared by the row kernels of nnet-loss-kernels.hip (Softmax)
// and nnet-normalize-kernels.hip (NormalizeComponent).
#ifndef KCNN_NNET2_ROW_REGS_H_
#define KCNN_NNET2_ROW_REGS_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

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

}  // namespace rowregs
}  // namespace kcnn

#endif  // KCNN_NNET2_ROW_REGS_H_
