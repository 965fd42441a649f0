// kaldi-lite/f16-stats.h -- the group statistics pass (cu-f16-stats.hip) as
// the f16x3 GEMM uses it: one pass over an operand, and the launch of one or
// two of them.  Host only; the extern "C" entry points are in
// cu-kernels-lite.h.
#ifndef KCNN_KALDI_LITE_F16_STATS_H_
#define KCNN_KALDI_LITE_F16_STATS_H_

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace kcnn::f16x3 {

struct StatOp {
  const float *X;
  uint32_t *out;   // the statistics block [max, min, cnt], per row (mode 0) or column (1)
  uint32_t *part;  // mode 1: [2][rbk][cols] partials (maxima, then minima - 1)
  int rows, cols, ld, mode, vec;
  int blocks;      // of stats_kernel
  int rpb;         // mode 0: rows per block (4: a wave each; 1: a block)
  int cb, rbk, rb; // mode 1: column blocks, row chunks, rows per chunk
  int fblocks;     // mode 1: blocks of stats_finalize_kernel
  uint32_t *clear; // nullable: two words stats_kernel sets to 0 (a consumer's counters)
};

// a statistics pass over X (rows x cols, pitch ld): mode 0 per row, 1 per
// column (partials at part, stat_part_words of them)
StatOp stat_op(const float *X, int rows, int cols, int ld, int mode, uint32_t *out,
               uint32_t *part);
size_t stat_part_words(int rows, int cols, int mode);
// the passes a and b (StatOp{}: none) in one set of launches
int stats_launch(const StatOp &a, const StatOp &b, hipStream_t st);

}  // namespace kcnn::f16x3

#endif  // KCNN_KALDI_LITE_F16_STATS_H_
