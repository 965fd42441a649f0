// scripts/launch_log.h -- the part the launch loggers share
// (conv_launch_log.cc, nnet2_launch_log.cc): hipLaunchKernel, the
// call-configuration pair and the few device calls libkcnn.so's host code
// makes, defined in the program so that they take precedence over the
// runtime's (link with -rdynamic).  No kernel runs; every launch is printed as
//   "  K <kernel handle offset in its library> grid x,y,z block x,y,z lds n"
// and scripts/conv_launch_names.py replaces the offsets by symbol names.
// Include it in exactly one translation unit of a program.
#ifndef KCNN_SCRIPTS_LAUNCH_LOG_H_
#define KCNN_SCRIPTS_LAUNCH_LOG_H_

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

static void *g_lib = nullptr;

static void log_launch(const void *f, dim3 g, dim3 b, size_t shmem) {
  Dl_info di;
  uintptr_t off = (uintptr_t)f;
  if (dladdr(f, &di) && di.dli_fbase) off -= (uintptr_t)di.dli_fbase;
  printf("  K %lx grid %u,%u,%u block %u,%u,%u lds %zu\n", (unsigned long)off, g.x, g.y, g.z,
         b.x, b.y, b.z, shmem);
}

static dim3 c_grid, c_block;
static size_t c_shmem;
static hipStream_t c_stream;
extern "C" {
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t s, hipStream_t st) {
  c_grid = g; c_block = b; c_shmem = s; c_stream = st;
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3 *g, dim3 *b, size_t *s, hipStream_t *st) {
  *g = c_grid; *b = c_block; *s = c_shmem; *st = c_stream;
  return hipSuccess;
}
hipError_t hipLaunchKernel(const void *f, dim3 g, dim3 b, void **, size_t shmem, hipStream_t) {
  log_launch(f, g, b, shmem);
  return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipMalloc(void **p, size_t n) {
  static uintptr_t next = 0xb00000000ull;
  *p = (void *)next;
  next += (n + 4095) & ~(size_t)4095;
  printf("  malloc %zu\n", n);
  return hipSuccess;
}
hipError_t hipFree(void *) { return hipSuccess; }
int rocblas_create_handle(void **h) { *h = (void *)0x1; return 0; }
int rocblas_destroy_handle(void *) { return 0; }
int rocblas_set_atomics_mode(void *, int) { return 0; }
int rocblas_set_pointer_mode(void *, int) { return 0; }
int rocblas_set_stream(void *, void *) { return 0; }
hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) {
  printf("  memset %d %zu\n", v, n);
  return hipSuccess;
}
}

// the library given on the command line, or exit(2)
static void open_lib(const char *path) {
  g_lib = dlopen(path, RTLD_NOW | RTLD_GLOBAL);
  if (!g_lib) { fprintf(stderr, "%s\n", dlerror()); exit(2); }
}

template <class F>
static F sym(const char *n) {
  void *p = dlsym(g_lib, n);
  if (!p) { fprintf(stderr, "missing %s\n", n); exit(2); }
  return reinterpret_cast<F>(p);
}

#endif  // KCNN_SCRIPTS_LAUNCH_LOG_H_
