// kaldi-lite/cu-gemm-f16x3-reduce.hip -- the split-K finish of the f16x3 GEMM
// (cu-gemm-f16x3.hip): the reduce of the partial slabs with the spread check
// on the summed value, the fix-up of the groups the reduce defers, and the
// host's table of call sites that says whether a call launches the fix-up.
#include <atomic>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>

#include "cnslmat/f16-split.h"
#include "cnslmat/hip-util.h"
#include "kaldi-lite/cu-kernels-lite.h"
#include "kaldi-lite/gemm-f16x3-dev.h"

namespace {

using namespace kcnn::f16x3;

// C = alpha * sum_s part[s] + beta * C, the splits added in increasing s
// (slab rows padded to np4 = N rounded up to 4: 16-B reads; a quad's columns
// past N are not stored); elements of an Inf / NaN row or column are the
// epilogue's (split 0).  The spread check of tile_epilogue on the summed
// value (unscaled: the threshold times 2^-(s_row + s_col)); a rejected
// element is not stored.  A wave with at most REJ_LOCAL of them recomputes
// them itself (wave_dot); one with more flags its 64 quads (rflag) for
// gemm_f16x3_fixup_kernel, which spreads such groups over the whole GPU: a
// spread row rejects hundreds of elements of one row, and one wave's
// wave_dots in series took milliseconds (nnet.config's weight gradients).
// A call launched without the fix-up (fix_local) recomputes such a group
// itself, in the order the fix-up would have used: the quarter order
// (quarter_sums) when the call's `rows` holds, wave_dot when not.  So a
// rejected element's bits depend on the operands and on whether its group of
// 64 quads exceeds REJ_LOCAL, never on which kernel recomputed it.  Every pass of a wave keeps all 64 lanes (a quad past the end rejects
// nothing): wave_dot spreads K over the whole wave.
constexpr int REJ_LOCAL = 4;
__device__ __forceinline__ uint32_t reduce_quad(const GemmF16Args &p, int64_t e, int nq, int np4,
                                                int64_t plane, int &r, int &c, bool store) {
  const int N = p.N;
  r = (int)(e / nq);
  c = (int)(e - (int64_t)r * nq) * 4;
  // every load of the quad issued before the first test: the slabs, the
  // row's statistics and the four columns' (one 16-B load each when the
  // blocks allow; a column past N reads as non-finite, i.e. not stored)
  const float *q = p.part + (int64_t)r * np4 + c;
  float4 v = *reinterpret_cast<const float4 *>(q);
  float4 w = p.ksplit > 1 ? *reinterpret_cast<const float4 *>(q + plane) : v;
  const uint32_t ar = p.amax[r], cr = p.acnt[r];
  uint32_t bm[4], cc[4];
  if (p.bvec) {
    const uint4 x = *reinterpret_cast<const uint4 *>(p.bmax + c);
    const uint4 y = *reinterpret_cast<const uint4 *>(p.bcnt + c);
    bm[0] = x.x; bm[1] = x.y; bm[2] = x.z; bm[3] = x.w;
    cc[0] = y.x; cc[1] = y.y; cc[2] = y.z; cc[3] = y.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bm[i] = c + i < N ? p.bmax[c + i] : NONFINITE;
      cc[i] = c + i < N ? p.bcnt[c + i] : 0u;
    }
  }
  // the bias quad too, and the momentum update's W and prev quads (the 16-B
  // paths' operands, loaded here, not after the tests: one memory round trip
  // per quad instead of two; host: the update's rows 16-B aligned)
  float4 w4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q4 = w4;
  float4 *wp = nullptr, *qp = nullptr;
  if (p.mom.W && store) {
    wp = reinterpret_cast<float4 *>(p.mom.W + (int64_t)r * p.mom.ldw + c);
    qp = reinterpret_cast<float4 *>(p.mom.prev + (int64_t)r * p.mom.ldp + c);
    if (c + 4 <= N) {
      w4 = *wp;
      q4 = *qp;
    }
  }
  float bv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (p.bias && store) {
    if (c + 4 <= N && ((uintptr_t)p.bias & 15) == 0) {
      const float4 b4 = *reinterpret_cast<const float4 *>(p.bias + c);
      bv[0] = b4.x; bv[1] = b4.y; bv[2] = b4.z; bv[3] = b4.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) bv[i] = c + i < N ? p.bias[c + i] : 0.0f;
    }
  }
  if (p.ksplit > 1) {
    v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
    for (int k = 2; k < p.ksplit; ++k) {
      w = *reinterpret_cast<const float4 *>(q + k * plane);
      v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
    }
  }
  if (ar >= NONFINITE) return 0;
  const float sv[4] = {v.x, v.y, v.z, v.w};
  // the counts are 0 unless a group is spread, so one test skips the check
  // (an all-zero row: its products are exactly 0, no check)
  const bool any = (cr | cc[0] | cc[1] | cc[2] | cc[3]) != 0 && ar != 0;
  float *o = p.C + (int64_t)r * p.ldc + c;
  const bool fin = max(max(bm[0], bm[1]), max(bm[2], bm[3])) < NONFINITE;
  if (p.mom.W && !any && fin) {  // the fused momentum update, 16-B (host: aligned)
    if (store) momentum_quad(p, v, w4, q4, wp, qp);
    return 0;
  }
  if (!p.mom.W && !any && fin && ((p.ldc & 3) | ((uintptr_t)p.C & 15)) == 0) {
    if (store) {  // one 16-B store (the same values)
      float4 ov = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (p.beta != 0.0f) ov = *reinterpret_cast<const float4 *>(o);
      const float oi[4] = {ov.x, ov.y, ov.z, ov.w};
      float wv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        wv[i] = p.beta == 0.0f ? p.alpha * sv[i] : p.alpha * sv[i] + p.beta * oi[i];
        if (p.bias) wv[i] += bv[i];
      }
      *reinterpret_cast<float4 *>(o) = make_float4(wv[0], wv[1], wv[2], wv[3]);
    }
    return 0;
  }
  // the check's thresholds (0: no check) of the four columns
  float thr[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (any) {
    const int er = scale_exp(ar);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // (an all-zero column: exact, no check)
      if (bm[i] >= NONFINITE || bm[i] == 0 || (cr | cc[i]) == 0) continue;
      thr[i] = __builtin_amdgcn_ldexpf(
          kcnn::f16x3::spread_weight(cr) + kcnn::f16x3::spread_weight(cc[i]),
          -(er + scale_exp(bm[i])));
    }
  }
  uint32_t rej = 0;  // bit i: column c + i is rejected
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (bm[i] >= NONFINITE) continue;  // (and columns past N)
    if (thr[i] != 0.0f && !(fabsf(sv[i]) >= thr[i])) {
      rej |= 1u << i;
      continue;
    }
    if (store) emit(p, r, c + i, sv[i]);
  }
  return rej;
}

// A quarter of K (quarter q of 4: k in [q kq, min(K, (q + 1) kq)), kq = K / 4
// rounded up) of the W sums of C[r][c .. c + W - 1], op(B) row-contiguous
// (W = 4: a quad by 16-B loads of op(B)'s rows; W = 1: one element): for
// each column, products k0 + 4 i + j go to accumulator j in increasing k
// over the quarter's whole multiples of FIX_DEPTH, the rest to accumulator 0,
// and the accumulators are added as (0 + 1) + (2 + 3).  A column's sum does
// not depend on W, nor on DEPTH, which is only how many k steps are loaded at
// once (the same products added in the same order).
constexpr int FIX_DEPTH = 16;
template <int W>
__device__ __forceinline__ void load_cols(const float *q, float (&y)[W]) {
  if constexpr (W == 4) {
    const float4 t = *reinterpret_cast<const float4 *>(q);
    y[0] = t.x; y[1] = t.y; y[2] = t.z; y[3] = t.w;
  } else {
    static_assert(W == 1, "a quad or one element");
    y[0] = *q;
  }
}
template <int DEPTH, int W>
__device__ __forceinline__ void quarter_sums(const float *A, int lda, const float *B, int ldb,
                                             int K, bool a_kc, int r, int c, int quarter,
                                             float (&q)[W]) {
  static_assert(DEPTH % 4 == 0 && FIX_DEPTH % DEPTH == 0, "accumulator j takes k = k0 + 4 i + j");
  const int kq = (K + 3) >> 2;
  const int k0 = quarter * kq, k1 = min(K, k0 + kq);
  const int km = k0 + max(k1 - k0, 0) / FIX_DEPTH * FIX_DEPTH;
  const int64_t sa = a_kc ? 1 : lda;
  const float *qa = a_kc ? A + (int64_t)r * lda + k0 : A + (int64_t)k0 * lda + r;
  const float *qb = B + (int64_t)k0 * ldb + c;
  float acc[4][W];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < W; ++j) acc[i][j] = 0.0f;
  int k = k0;
#pragma unroll 1
  for (; k < km; k += DEPTH) {
    float x[DEPTH];
    float y[DEPTH][W];
#pragma unroll
    for (int i = 0; i < DEPTH; ++i) {
      x[i] = qa[i * sa];
      load_cols<W>(qb + (int64_t)i * ldb, y[i]);
    }
#pragma unroll
    for (int i = 0; i < DEPTH; ++i)
#pragma unroll
      for (int j = 0; j < W; ++j) acc[i & 3][j] = fmaf(x[i], y[i][j], acc[i & 3][j]);
    qa += DEPTH * sa;
    qb += (int64_t)DEPTH * ldb;
  }
#pragma unroll 1
  for (; k < k1; ++k) {
    const float x = *qa;
    float y[W];
    load_cols<W>(qb, y);
#pragma unroll
    for (int j = 0; j < W; ++j) acc[0][j] = fmaf(x, y[j], acc[0][j]);
    qa += sa;
    qb += ldb;
  }
#pragma unroll
  for (int j = 0; j < W; ++j) q[j] = (acc[0][j] + acc[1][j]) + (acc[2][j] + acc[3][j]);
}
// loads in flight per lane in the reduce's own quarter sums (fix_local), which
// take one element at a time: the kernel runs in every split-K call and is
// bound by its slab reads, so the rarely taken path must not raise its
// register count
constexpr int LOCAL_DEPTH = 4;

__global__ __launch_bounds__(256) void gemm_f16x3_reduce_kernel(GemmF16Args p, int a_kc,
                                                                int b_kc, int rows) {
  const int np4 = (p.N + 3) & ~3, nq = np4 >> 2;
  const int64_t total = (int64_t)p.M * nq;
  const int64_t plane = (int64_t)p.M * np4;
  const int lane = threadIdx.x & 63;
  // the bound is total rounded up to the wave's 64 quads, so a pass keeps or
  // drops a whole wave (the last group's lanes past total stay, on quad 0
  // with no rejection: wave_dot below needs all 64), and every group of 64
  // quads gets its flag written
  const int64_t padded = (total + 63) & ~(int64_t)63;
  for (int64_t el = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; el < padded;
       el += (int64_t)gridDim.x * blockDim.x) {
    // (a whole tile's quads were stored by its workgroup: no slabs, no
    // rejections.  One index for both uses below: the 64-bit division is
    // then computed once)
    const bool inside = el < total;
    const int64_t e = inside ? el : 0;
    int r = (int)(e / nq), c = (int)(e - (int64_t)r * nq) * 4;
    const bool valid = inside && in_split_tile(p, r, c);
    uint32_t rej = valid ? reduce_quad(p, e, nq, np4, plane, r, c, true) : 0u;
    // the wave's rejections
    const int n = __builtin_popcountll(__ballot(rej & 1)) + __builtin_popcountll(__ballot(rej & 2)) +
                  __builtin_popcountll(__ballot(rej & 4)) + __builtin_popcountll(__ballot(rej & 8));
    const bool over = n > REJ_LOCAL;
    const bool defer = over && !p.fix_local;
    if (lane == 0) {
      p.rflag[el >> 6] = defer ? 1u : 0u;
      if (defer) p.rflag[(total + 63) >> 6] = p.gen;
      if (over && p.fix_report) *p.fix_report = 1u;
    }
    // (expected: what follows is rare, and the register allocator should
    // not spill the pass's own values for it)
    if (__builtin_expect(n == 0 || defer, 1)) continue;
    if (over && rows) {
      // the fix-up's sums of this group, each lane its own quad's rejected
      // elements in turn: the four quarters, added in quarter order (the
      // fix-up's wave order, a left fold).  The shape enters through a
      // barrier, so that this rare path's invariants are formed here and do
      // not take scalar registers from every pass of every call.
      int K = p.K, lda = p.lda, ldb = p.ldb, akc = a_kc;
      asm volatile("" : "+s"(K), "+s"(lda), "+s"(ldb), "+s"(akc));
#pragma unroll 1
      for (; rej; rej &= rej - 1) {
        const int col = c + __builtin_ctz(rej);
        float s[1], t[1];
        quarter_sums<LOCAL_DEPTH, 1>(p.A, lda, p.B, ldb, K, akc != 0, r, col, 0, s);
#pragma unroll 1
        for (int w = 1; w < 4; ++w) {
          quarter_sums<LOCAL_DEPTH, 1>(p.A, lda, p.B, ldb, K, akc != 0, r, col, w, t);
          s[0] += t[0];
        }
        emit(p, r, col, s[0]);
      }
      continue;
    }
    fix_rejected(p, a_kc != 0, b_kc != 0, rej, lane, [&](int l, int bit, int &row, int &col) {
      row = __builtin_amdgcn_readlane(r, l);
      col = __builtin_amdgcn_readlane(c, l) + bit;
    });
  }
}

// The flagged groups of 64 quads (gemm_f16x3_reduce_kernel), one per block
// at a time: slot s = t G + b for thread t of block b (G blocks), so the
// consecutive groups of one spread row go to different blocks.  A group's
// rejections are found again (reduce_quad, not stored) and recomputed in fp32:
//  - op(B) row-contiguous with 16-B rows (`rows`): every lane its quad's four sums, the
//    block's four waves each over a quarter of K (quarter_sums: 16-B loads of
//    op(B)'s rows, coalesced over the lanes; the lanes of one C row share
//    op(A)'s element), the quarters added in wave order, the rejected
//    elements stored;
//  - otherwise: wave_dot per rejected element, the quads dealt to
//    the waves by lane & 3.
// Deterministic: the group's results do not depend on the block or order,
// and they are the bits the reduce gives the group when the call runs
// without this kernel (fix_local).
// the fixup's grid: a flagged call's groups take the workgroups in turn
// (c2's weight-gradient shape with 32 spread rows, 1452 groups: +925 us at
// 128 workgroups, measured r05 by a one-off driver); an unflagged call exits at the
// first load, and the launch costs the same 4.4 us at 128 or 1024
constexpr int FIX_GRID = 1024;
__global__ __launch_bounds__(256) void gemm_f16x3_fixup_kernel(GemmF16Args p, int a_kc,
                                                               int b_kc, int rows) {
  __shared__ int list[256];
  __shared__ int nlist;
  __shared__ float4 quarter[4][64];
  const int np4 = (p.N + 3) & ~3, nq = np4 >> 2;
  const int64_t total = (int64_t)p.M * nq;
  const int64_t plane = (int64_t)p.M * np4;
  const int64_t nslots = (total + 63) >> 6;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // nothing flagged in this call (the word is another call's number, or
  // anything the workspace held: a stale match only costs the scan below)
  if (p.rflag[nslots] != p.gen) return;
  for (int64_t base = 0; base < nslots; base += (int64_t)gridDim.x * blockDim.x) {
    if (threadIdx.x == 0) nlist = 0;
    __syncthreads();
    const int64_t slot = base + (int64_t)threadIdx.x * gridDim.x + blockIdx.x;
    if (slot < nslots && p.rflag[slot] != 0) list[atomicAdd(&nlist, 1)] = (int)threadIdx.x;
    __syncthreads();
    const int n = nlist;
    for (int j = 0; j < n; ++j) {
      const int64_t e0 = (base + (int64_t)list[j] * gridDim.x + blockIdx.x) << 6;
      const int64_t e = e0 + lane;
      // (past C: row and column 0, whose loads below stay in bounds)
      int r = e < total ? (int)(e / nq) : 0;
      int c = e < total ? (int)(e - (int64_t)r * nq) * 4 : 0;
      const bool valid = e < total && in_split_tile(p, r, c);
      const uint32_t rej = valid ? reduce_quad(p, e, nq, np4, plane, r, c, false) : 0u;
      if (!rows) {
        const uint64_t mine = (lane & 3) == wave ? rej : 0u;
        fix_rejected(p, a_kc != 0, b_kc != 0, mine, lane, [&](int l, int bit, int &row, int &col) {
          row = __builtin_amdgcn_readlane(r, l);
          col = __builtin_amdgcn_readlane(c, l) + bit;
        });
        __syncthreads();
        continue;
      }
      // this wave's quarter of K for the lane's quad (r, c .. c + 3)
      float q[4];
      quarter_sums<FIX_DEPTH, 4>(p.A, p.lda, p.B, p.ldb, p.K, a_kc != 0, r, c, wave, q);
      quarter[wave][lane] = make_float4(q[0], q[1], q[2], q[3]);
      __syncthreads();
      if (wave == 0 && rej) {
        const float4 q0 = quarter[0][lane], q1 = quarter[1][lane], q2 = quarter[2][lane],
                     q3 = quarter[3][lane];
        const float v[4] = {((q0.x + q1.x) + q2.x) + q3.x, ((q0.y + q1.y) + q2.y) + q3.y,
                            ((q0.z + q1.z) + q2.z) + q3.z, ((q0.w + q1.w) + q2.w) + q3.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (rej >> i & 1) emit(p, r, c + i, v[i]);
      }
      __syncthreads();
    }
    __syncthreads();
  }
}

}  // namespace

// The fix-up launch of a split-K call (an exit-at-once kernel of 4.4 us in
// all but the rare calls with a spread group, FIX_GRID) is skipped for a call
// site (shape, transposes, momentum or not) whose previous call deferred no
// group: the site's word in host memory, cleared by the host at each launch
// and set by the reduce when a group would have been deferred, is read at
// the next launch.  A skipped call's reduce recomputes every rejection itself
// (fix_local), a group over REJ_LOCAL in the order the fix-up would have used
// (gemm_f16x3_reduce_kernel), so the word, read without a synchronise, never
// reaches a result: a stale or wrong guess costs time, not a bit of C
// (tests/test_gpu_gemm_fixup.py runs every route in both states).  Up to
// FIX_SITES sites; the others always launch the fix-up.
// kl_gemm_f16x3_fixup_counts counts the calls either way and
// kl_gemm_f16x3_fixup_sites_reset forgets the sites, for those tests.
constexpr int FIX_SITES = 256;
struct FixSites {
  std::mutex mu;
  uint32_t *flags = nullptr;  // pinned host words (1: the fix-up was needed or is unknown)
  uint32_t *dflags = nullptr; // the same words' device address
  int64_t key[FIX_SITES][6];
  int n = 0;
  bool failed = false;
};
static FixSites &fix_sites() {
  static FixSites fs;
  return fs;
}
// split-K calls that launched the fix-up, that skipped it
static std::atomic<unsigned long long> g_fix_calls[2];
extern "C" void kl_gemm_f16x3_fixup_counts(unsigned long long *out, int reset) {
  for (int i = 0; i < 2; ++i) {
    out[i] = g_fix_calls[i].load(std::memory_order_relaxed);
    if (reset) g_fix_calls[i].store(0, std::memory_order_relaxed);
  }
}
// every site forgotten: the next call at any key registers again, word 1 (the
// pinned words stay allocated; no device call)
extern "C" void kl_gemm_f16x3_fixup_sites_reset(void) {
  FixSites &fs = fix_sites();
  std::lock_guard<std::mutex> lk(fs.mu);
  fs.n = 0;
}

namespace kcnn::f16x3 {

// this call site's word, read and cleared (none: table full, no host memory)
FixupSite split_k_site(const GemmArgs &a, bool a_kc, bool b_kc) {
  FixupSite site;
  FixSites &fs = fix_sites();
  std::lock_guard<std::mutex> lk(fs.mu);
  if (!fs.flags && !fs.failed) {
    void *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, FIX_SITES * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent) ==
            hipSuccess &&
        hipHostGetDevicePointer(&d, h, 0) == hipSuccess) {
      fs.flags = static_cast<uint32_t *>(h);
      fs.dflags = static_cast<uint32_t *>(d);
    } else {
      (void)hipGetLastError();
      fs.failed = true;
    }
  }
  if (!fs.flags) return site;
  const int64_t k[6] = {a.M, a.N, a.K, !a_kc, b_kc, a.mom.W != nullptr};
  int i = 0;
  for (; i < fs.n; ++i)
    if (std::equal(k, k + 6, fs.key[i])) break;
  if (i == fs.n) {
    if (fs.n == FIX_SITES) return site;
    std::copy(k, k + 6, fs.key[fs.n++]);
    __atomic_store_n(fs.flags + i, 1u, __ATOMIC_RELAXED);
  }
  site.report = fs.dflags + i;
  site.launch = __atomic_load_n(fs.flags + i, __ATOMIC_RELAXED) != 0;
  __atomic_store_n(fs.flags + i, 0u, __ATOMIC_RELAXED);
  return site;
}

int split_k_finish(const GemmArgs &call, bool a_kc, bool b_kc, const FixupSite &site,
                   hipStream_t st) {
  GemmF16Args a{call};
  a.fix_report = site.report;
  a.fix_local = site.launch ? 0 : 1;
  const int M = a.M, N = a.N;
  // op(B) row-contiguous: 16-B loads along its rows in the recomputation of
  // a group over REJ_LOCAL, by the fix-up or (fix_local) by the reduce
  const int rows = !b_kc && a.ldb % 4 == 0 && (uintptr_t)a.B % 16 == 0 && N % 4 == 0;
  hipLaunchKernelGGL(gemm_f16x3_reduce_kernel, dim3(kcnn::grid_for((int64_t)M * ((N + 3) / 4))),
                     dim3(256), 0, st, a, a_kc ? 1 : 0, b_kc ? 1 : 0, rows);
  int rc = kcnn::launch_status();
  if (!rc) g_fix_calls[site.launch ? 0 : 1].fetch_add(1, std::memory_order_relaxed);
  if (rc || !site.launch) return rc;
  const int64_t slots = ((int64_t)M * ((N + 3) / 4) + 63) / 64;
  hipLaunchKernelGGL(gemm_f16x3_fixup_kernel,
                     dim3((unsigned)std::min<int64_t>(FIX_GRID, (slots + 15) / 16)), dim3(256), 0, st,
                     a, a_kc ? 1 : 0, b_kc ? 1 : 0, rows);
  return kcnn::launch_status();
}

}  // namespace kcnn::f16x3
