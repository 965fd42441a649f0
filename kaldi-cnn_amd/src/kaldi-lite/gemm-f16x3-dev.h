// kaldi-lite/gemm-f16x3-dev.h -- what the f16x3 GEMM's main-loop kernels
// (cu-gemm-f16x3.hip) and its split-K finish (cu-gemm-f16x3-reduce.hip) both
// use: the call's arguments, the tile order's index, the fp32 recomputation
// of a checked element, the store, and the split-K workspace's layout.
// Included by those two files only.
#ifndef KCNN_KALDI_LITE_GEMM_F16X3_DEV_H_
#define KCNN_KALDI_LITE_GEMM_F16X3_DEV_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cnslmat/momentum-step.h"

namespace kcnn::f16x3 {

struct GemmArgs {
  const float *A, *B;
  float *C;                      // the output
  float *part;                   // ksplit > 1: the partial slabs [ksplit][M][N]
  uint32_t *rflag;               // ksplit > 1: per 64 quads of C, 1 when the reduce left
                                 // its rejections to gemm_f16x3_fixup_kernel; after
                                 // them one word, gen when any group was flagged
  uint32_t gen;                  // this call's number (host counter, never 0)
  const uint32_t *amax, *bmax;   // max |x| bits per row of op(A), per column of op(B)
  const uint32_t *amin, *bmin;   // min nonzero |x| bits (0: none), the same groups
  const uint32_t *acnt, *bcnt;   // spread groups: their elements below 2^-3 after the scale
  const float *bias;             // nullable: C += bias[col] on every row (after alpha, beta)
  int M, N, K, lda, ldb, ldc;
  int bvec;                      // bmax, bcnt 16-B aligned and N % 4 == 0 (the reduce's loads)
  MomentumEpi mom;               // mom.W: C is a weight gradient applied in the store (emit)
  int kps, ksplit, tiles_m, tiles_n;
  int bn;                        // the tile's columns (BN_NARROW or BN_WIDE)
  int nwhole;                    // ksplit > 1: the first nwhole tiles (a multiple of 256) whole
  int fix_local;                 // ksplit > 1: no fix-up launch; the reduce recomputes every rejection
  uint32_t *fix_report;          // nullable (host memory): set to 1 when a group would be deferred
  float alpha, beta;
};

// The split-K finish of a call whose main kernel is launched, in two steps
// (cu-gemm-f16x3-reduce.hip).  split_k_site, before anything of the call is
// enqueued: the call site's fix-up word read and cleared on the host.
// split_k_finish, after the main launch: the reduce and, where the site says
// so, the fix-up, on a copy of `a` with fix_local and fix_report set (the
// main kernels read neither).
struct FixupSite {
  uint32_t *report = nullptr;  // fix_report: the site's word (device address), or none
  bool launch = true;          // the fix-up kernel runs (else fix_local)
};
FixupSite split_k_site(const GemmArgs &a, bool a_kc, bool b_kc);
int split_k_finish(const GemmArgs &a, bool a_kc, bool b_kc, const FixupSite &site,
                   hipStream_t st);

}  // namespace kcnn::f16x3

// Each including file's own copies, as its kernels are: the kernels' names
// carry (anonymous namespace)::GemmF16Args.
namespace {

struct GemmF16Args : kcnn::f16x3::GemmArgs {};

constexpr int BM = 256, BK = 32;
// The tile of C per workgroup is BM x BN: the narrow tile (BN 128, 8 waves
// of 64 x 64, 2 x 2 accumulators each) or the wide one (BN 256, 8 waves of
// 128 x 64, 4 x 2 accumulators: per MFMA two thirds of the narrow tile's
// operand loads, split and LDS writes, three quarters of its fragment reads,
// half its barriers and tiles).  Both hold the same 32 x 32 accumulator
// blocks of C, each summed in the same order: the same bits.
constexpr int BN_NARROW = 128, BN_WIDE = 256;

// The tiles go in groups of GM tile rows, column-major inside a group
// (tile_rc, cu-gemm-f16x3.hip); the order's index of tile (tm, tn)
constexpr int GM = 4;
__device__ __forceinline__ int tile_index(const GemmF16Args &p, int tm, int tn) {
  const int g = tm / GM, m0 = g * GM;
  const int gm = min(p.tiles_m - m0, GM);
  return g * GM * p.tiles_n + tn * gm + (tm - m0);
}
// C element (r, c) is a split tile's (its value from the partial slabs)
__device__ __forceinline__ bool in_split_tile(const GemmF16Args &p, int r, int c) {
  return p.nwhole == 0 || tile_index(p, r / BM, c / p.bn) >= p.nwhole;
}

// One C element by a whole wave, for the store's check (called with the same
// row and column in every lane): fp32 products of op(A) row i and op(B)
// column j in a fixed order per lane, then a butterfly over the lanes (every
// lane ends with the same bits: deterministic)
__device__ __forceinline__ float wave_dot(const GemmF16Args &p, bool a_kc, bool b_kc, int row,
                                          int col, int lane) {
  // element k of the row of op(A) / column of op(B): qa[k * sa], qb[k * sb]
  // (wave-uniform strides; the pointers step, no per-load index products)
  const int64_t sa = a_kc ? 1 : p.lda, sb = b_kc ? 1 : p.ldb;
  const float *qa = (a_kc ? p.A + (int64_t)row * p.lda : p.A + row) + lane * sa;
  const float *qb = (b_kc ? p.B + (int64_t)col * p.ldb : p.B + col) + lane * sb;
  const int64_t da = 64 * sa, db = 64 * sb;
  // four partial sums (k = lane + 64 (4 i + j) into sum j): eight loads in
  // flight per lane instead of one
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int k = lane;
#pragma unroll 1
  for (; k + 192 < p.K; k += 256) {
    float x[4], y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j] = qa[j * da];
      y[j] = qb[j * db];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = fmaf(x[j], y[j], s[j]);
    qa += 4 * da;
    qb += 4 * db;
  }
#pragma unroll 1
  for (; k < p.K; k += 64) {
    s[0] = fmaf(*qa, *qb, s[0]);
    qa += da;
    qb += db;
  }
  float t = (s[0] + s[1]) + (s[2] + s[3]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d);
  return t;
}
__device__ __forceinline__ float store_value(const GemmF16Args &p, float v, float *o, int col) {
  float r = p.beta == 0.0f ? p.alpha * v : p.alpha * v + p.beta * *o;
  if (p.bias) r += p.bias[col];
  return r;
}
// C[row][col] from the product's value v; with p.mom.W the element is instead
// the gradient of the momentum update (momentum-step.h: alpha * v, beta 0, no
// bias), applied to W and prev in place of storing C
__device__ __forceinline__ void emit(const GemmF16Args &p, int row, int col, float v) {
  if (p.mom.W) {
    float *w = p.mom.W + (int64_t)row * p.mom.ldw + col;
    float *q = p.mom.prev + (int64_t)row * p.mom.ldp + col;
    float wv = *w, pv = *q;
    kcnn::momentum_step(p.alpha * v, pv, wv, p.mom.momentum, p.mom.a_wd, p.mom.a_g);
    *q = pv;
    *w = wv;
    return;
  }
  float *o = p.C + (int64_t)row * p.ldc + col;
  *o = store_value(p, v, o, col);
}
// The elements a lane's check rejected (bit n of `mine` its n-th candidate,
// decode(lane, n) -> (row, col)), each recomputed by the whole wave
// (wave_dot) and handed to put(l, n, row, col, v) on lane 0: a wave-uniform
// loop over the wave's rejections
template <typename Decode, typename Put>
__device__ __forceinline__ void fix_rejected(const GemmF16Args &p, bool a_kc, bool b_kc,
                                             uint64_t mine, int lane, Decode decode, Put put) {
  for (;;) {
    const uint64_t who = __ballot(mine != 0);
    if (who == 0) break;
    const int l = __builtin_ctzll(who);
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)mine, l);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(mine >> 32), l);
    const uint64_t bits = ((uint64_t)hi << 32) | lo;
    const int n = __builtin_ctzll(bits);
    int row, col;
    decode(l, n, row, col);
    const float v = wave_dot(p, a_kc, b_kc, row, col, lane);
    if (lane == 0) put(l, n, row, col, v);
    if (lane == l) mine &= mine - 1;
  }
}
template <typename Decode>
__device__ __forceinline__ void fix_rejected(const GemmF16Args &p, bool a_kc, bool b_kc,
                                             uint64_t mine, int lane, Decode decode) {
  fix_rejected(p, a_kc, b_kc, mine, lane, decode,
               [&](int, int, int row, int col, float v) { emit(p, row, col, v); });
}

// emit's momentum step on four consecutive elements of a row, 16 B per
// access: the products' values v and the W and prev quads the caller loaded
// from wq and pq (the update's rows are 16-B aligned: host check)
__device__ __forceinline__ void momentum_quad(const GemmF16Args &p, const float4 &v, float4 &w4,
                                              float4 &q4, float4 *wq, float4 *pq) {
  const MomentumEpi &m = p.mom;
  kcnn::momentum_step(p.alpha * v.x, q4.x, w4.x, m.momentum, m.a_wd, m.a_g);
  kcnn::momentum_step(p.alpha * v.y, q4.y, w4.y, m.momentum, m.a_wd, m.a_g);
  kcnn::momentum_step(p.alpha * v.z, q4.z, w4.z, m.momentum, m.a_wd, m.a_g);
  kcnn::momentum_step(p.alpha * v.w, q4.w, w4.w, m.momentum, m.a_wd, m.a_g);
  *pq = q4;
  *wq = w4;
}

inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
// the split-K workspace: the slabs, then the reduce's flags (one word per
// 64 quads of C)
inline size_t slab_bytes(int s, int M, int N) {
  return align16(sizeof(float) * (size_t)s * M * ((N + 3) & ~3));
}
inline size_t flag_bytes(int M, int N) {
  return align16(sizeof(uint32_t) * (((size_t)M * ((N + 3) / 4) + 63) / 64 + 1));
}

}  // namespace

#endif
