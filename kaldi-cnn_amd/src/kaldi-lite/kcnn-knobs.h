// kaldi-lite/kcnn-knobs.h -- run-time switches of libkcnn.so.
//
// Kernel-family selectors are product settings: each picks between
// implementations of the same math (f16x3 / bf16x6 on the f16 / bf16 matrix
// cores, or the fp32-input MFMA kernels), is documented in DESIGN.md §3 and is covered by
// tests/test_gpu_families.py.  They are set through the C-ABI
// (kcnn_set_kernel_family) or, once when the library loads, by the
// environment variable named in the table below.
//
//   family     env              values
//   fwd_x6     KCNN_FWD_X6      2 f16x3 frame-resident forward, 1 bf16x6, 0 fp32 MFMA
//   bwd_x6     KCNN_BWD_X6      1 bf16x6 fused backward, 0 fp32 MFMA
//   igemm_x6   KCNN_IGEMM_X6    2 f16x3 implicit GEMM for convolutions of >= 2^34 flop (bf16x6
//                               below), 3 f16x3 for all, 1 bf16x6, 0 fp32 MFMA
//   wgrad_x6   KCNN_WGRAD_X6    2 wide bf16x6, 3 wide f16x3 (slower on c5), 1 128-wide bf16x6,
//                               0 fp32 MFMA
//   gemm       KCNN_GEMM        2 f16x3 GEMM (AddMatMat), its tile (256 x 128 or 256 x 256)
//                               chosen per call by the cost model (cu-gemm-f16x3.hip
//                               choose_plan); 3 f16x3 with the 256 x 256 tile for every
//                               call that can take it; 4 f16x3 with the 256 x 128 tile for
//                               every call; 1 bf16x6 GEMM; 0 rocBLAS sgemm
//
// (KCNN_FUSE, KCNN_LITERAL and KCNN_PROFILE are kcnn_set_fusion,
// kcnn_set_literal_path and kcnn_set_profiling.)
//
// One observation-only facility remains beside them: the per-phase clock
// marks of the convolution kernels (KCNN_TMARK and the printf of block 0's
// totals).  They are compiled only into the `make timing` library
// (-DKCNN_PHASE_TIMING), which switches them on when KCNN_PHASE_TIMING=1 is in
// the environment; they change no result.  phase_timing() is constant 0 in
// the product library.
#ifndef KCNN_KALDI_LITE_KNOBS_H_
#define KCNN_KALDI_LITE_KNOBS_H_

namespace kcnn {

enum Family { kFamFwdX6 = 0, kFamBwdX6, kFamIgemmX6, kFamWgradX6, kFamGemm, kNumFamilies };

int family(Family f);                 // current value of a selector
int set_family(Family f, int value);  // 0 on success, -1 for an invalid value
int family_by_name(const char *name);  // Family index, -1 when unknown

#ifdef KCNN_PHASE_TIMING
int phase_timing();  // 1 when the clock marks are switched on
#else
constexpr int phase_timing() { return 0; }
#endif

}  // namespace kcnn

#endif  // KCNN_KALDI_LITE_KNOBS_H_
