// kaldi-lite/launch-lds.h -- the launch of a kernel whose dynamic LDS is past
// the 64 KB a kernel gets without asking (the GEMM kernels of cu-gemm-x6.hip
// and cu-gemm-f16x3.hip).
#ifndef KCNN_KALDI_LITE_LAUNCH_LDS_H_
#define KCNN_KALDI_LITE_LAUNCH_LDS_H_

#include <hip/hip_runtime.h>

namespace kcnn {

// KERNEL on `blocks` workgroups of `threads` with LDS_BYTES of dynamic LDS;
// the kernel's limit is raised once, at its first launch
template <auto KERNEL, int LDS_BYTES, typename Args>
void launch_lds(const Args &a, unsigned blocks, unsigned threads, hipStream_t st) {
  static bool attr = [] {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               LDS_BYTES) == hipSuccess;
  }();
  (void)attr;
  hipLaunchKernelGGL(KERNEL, dim3(blocks), dim3(threads), LDS_BYTES, st, a);
}

}  // namespace kcnn

#endif  // KCNN_KALDI_LITE_LAUNCH_LDS_H_
