// cnslmat/conv-frame-dev.h -- what the frame-resident forward
// (cnsl-conv-frame.hip) and the frame backward (cnsl-conv-frame-bwd.hip)
// both use: the LDS budget of a co-resident workgroup, the frame grid, the
// filter-chunk loop and the phase-timing marks.
#ifndef KCNN_CNSLMAT_CONV_FRAME_DEV_H_
#define KCNN_CNSLMAT_CONV_FRAME_DEV_H_

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "conv-geom.h"

namespace kcnn {

constexpr int kFrameLdsMax = 96 * 1024;

__device__ __forceinline__ floatx16 zero16() {
  floatx16 z;
#pragma unroll
  for (int i = 0; i < 16; i++) z[i] = 0.0f;
  return z;
}

inline unsigned frame_grid(const ConvGeom &g, int blocks_per_cu) {
  int64_t b = 256LL * blocks_per_cu;
  if (b > g.R) b = g.R;
  return (unsigned)(b > 0 ? b : 1);
}

// Runs fn(chunk geometry, first filter) over g's filters in chunks of 128
// (each a column range of W, b and Y).  Only the first chunk may decline
// (-1: nothing is written yet); a later one that does has left the layer
// half done and is hipErrorLaunchFailure, which every caller returns as an
// error (none falls through to another route on it).  So fn must decide at
// g0 == 0 whatever would make a later chunk decline.  G <= 128 is one
// chunk, g itself.
template <class F>
int for_filter_chunks(const ConvGeom &g, F fn) {
  int g0 = 0;
  do {
    ConvGeom gc = g;
    gc.G = g.G - g0 < 128 ? g.G - g0 : 128;
    const int rc = fn(gc, g0);
    if (rc) return g0 == 0 ? rc : (rc < 0 ? (int)hipErrorLaunchFailure : rc);
    g0 += 128;
  } while (g0 < g.G);
  return 0;
}

}  // namespace kcnn

// A kernel's per-phase s_memtime totals in the phase-timing build
// (KCNN_PHASE_TIMING; the kernel's argument clk = phase_timing()):
// KCNN_TMARKS(n) declares the totals tm[n], KCNN_TMARK(i) adds the clocks
// since the previous mark to phase i, and the kernel prints tm[] of block 0
// at its end.  Both expand to nothing in every other build.  (An empty
// struct with an empty mark() in their place moved instructions in eight
// conv_fwd_regs_kernel instances: profiles/conv_frame_split.md.)
#ifdef KCNN_PHASE_TIMING
#define KCNN_TMARKS(n) long long tm[n] = {}, tprev = clock64();
#define KCNN_TMARK(i) if (clk) { const long long tn = clock64(); tm[i] += tn - tprev; tprev = tn; }
#else
#define KCNN_TMARKS(n)
#define KCNN_TMARK(i)
#endif

#endif  // KCNN_CNSLMAT_CONV_FRAME_DEV_H_
