// kaldi-lite/cu-gemm-x6.hip -- fp32 GEMM on the bf16 matrix cores by an exact
// three-way split of each operand (the "bf16x6" scheme).
//
// Upstream Kaldi's CuMatrixBase::AddMatMat is cuBLAS sgemm; the reference
// calls it for the FullyConnectedComponent forward, data gradient and update
// (nnet-component.cc:1225-1227, :1247; nnet-component-nnet0.cc:1137-1142).
// On gfx950 the fp32-input MFMA runs at 1/16 of the bf16 rate (157 TF), and
// rocBLAS sgemm already reaches ~86 % of that on these shapes.  This kernel
// computes the same fp32 product on the bf16 MFMAs instead:
//
//   x = h + m + l exactly, h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)
//
// (each residual subtraction is exact in fp32 and leaves at most 16, then 8,
// significant bits).  Every product of two bf16 values is exact in fp32, so
//
//   a*b = hh + (hm + mh) + (mm + hl + lh) + (ml + lm + ll)
//
// with the terms of relative size 1, 2^-8, 2^-16 and < 2^-24.  The kernel
// keeps the first six, one v_mfma_f32_32x32x16_bf16 each, all accumulated in
// fp32.  The three it drops are below fp32's own rounding of the product
// (measured: max |c - c64| / (|A||B|) = 1.7e-7 against rocBLAS sgemm's 2.9e-7
// at K = 11616, scripts/fc_split_probe.py), so the result meets the same
// dot-product error bound as sgemm (tests/test_gpu_gemm.py).  Six bf16 MFMAs
// cost 6/16 of one fp32 MFMA.
//
// Structure: 512 threads, a 256 x 128 tile of C per workgroup (8 waves, each
// 64 x 64 = 2 x 2 accumulators of 32 x 32), K steps of 32.  Operands are read
// from HBM as fp32 once per K step into registers (one step ahead), split in
// registers, and written to LDS as three bf16 planes in the MFMA fragment
// layout ([row][k], 64-B rows, 16-B chunks XOR-swizzled by row), double
// buffered (2 x 72 KB).  The VALU split runs beside the bf16 MFMAs, which,
// unlike the fp32-input MFMA, do not hold the SIMD's vector pipe.  Either
// operand may be stored K-contiguous or M/N-contiguous (row-major Kaldi
// matrices, both transpose flags); the transpose happens in the split pass.
// Thin outputs split K over workgroups; partial tiles are summed in a fixed
// order (deterministic, no atomics).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "cnslmat/bf16-split.h"
#include "cnslmat/lds-dma.h"
#include "cnslmat/hip-util.h"
#include "kaldi-lite/cu-kernels-lite.h"
#include "kaldi-lite/launch-lds.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 256, BN = 128, BK = 32, NT = 512;
constexpr int ROWB = BK * 2;                 // bytes per LDS row of one plane
constexpr int A_PLANE = BM * ROWB;           // 16 KB
constexpr int B_PLANE = BN * ROWB;           // 8 KB
constexpr int BUF = 3 * (A_PLANE + B_PLANE); // 72 KB
constexpr int LDS_BYTES = 2 * BUF;

struct GemmX6Args {
  const float *A, *B;
  float *C;          // direct output, or the partial slabs [ksplit][M][N]
  int M, N, K, lda, ldb, ldc;
  int kps;           // K per split (multiple of BK)
  int ksplit, tiles_m, tiles_n;
  float alpha, beta;
  int partial;       // 1: write raw sums to C + split * M * N (ld N)
};

// byte offset of (row r, 16-B chunk c) inside a plane
__device__ __forceinline__ int swz(int r, int c) {
  return r * ROWB + ((c ^ ((r >> 2) & 3)) << 4);
}

using kcnn::x6::split2;  // x = h + m + l exactly (cnslmat/bf16-split.h)

// 8 fp32 -> three bf16x8 planes, x = h + m + l exactly for finite x
__device__ __forceinline__ void split8(const float *x, uint4 &h, uint4 &m, uint4 &l) {
  uint32_t hv[4], mv[4], lv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) split2(x[2 * i], x[2 * i + 1], hv[i], mv[i], lv[i]);
  h = make_uint4(hv[0], hv[1], hv[2], hv[3]);
  m = make_uint4(mv[0], mv[1], mv[2], mv[3]);
  l = make_uint4(lv[0], lv[1], lv[2], lv[3]);
}

// One operand tile (R rows of C's side x BK) per K step.
//   KC (K-contiguous source, element (row, k) at src[row * ld + k]):
//     unit = (row, 8-k chunk), R * 4 units, two float4 loads each.
//   !KC (source stored [k][row], element at src[k * ld + row]):
//     unit = (row, KPT consecutive k), lanes along the row so each load
//     instruction reads a contiguous run; KPT = R * BK / NT.
template <int R, bool KC>
struct TileLoader {
  static constexpr int KPT = KC ? 8 : R * BK / NT;
  static constexpr int UNITS = KC ? R * 4 : R * BK / KPT;
  static constexpr int UPT = (UNITS + NT - 1) / NT;  // units per thread
  static_assert(KC ? (UNITS % NT == 0) : (KPT % 8 == 0), "tile shape");
  float v[UPT][KPT];

  __device__ __forceinline__ void load(const float *__restrict__ src, int ld,
                                       int row0, int rows, int k0, int kend,
                                       int tid) {
#pragma unroll
    for (int u = 0; u < UPT; ++u) {
      const int unit = tid + u * NT;
      if (unit >= UNITS) break;
      if constexpr (KC) {
        const int r = unit >> 2, k = k0 + (unit & 3) * 8;
        const int gr = row0 + r;
        const float *p = src + (int64_t)gr * ld + k;
        if (gr < rows && k + 8 <= kend) {
          const float4 a = *reinterpret_cast<const float4 *>(p);
          const float4 b = *reinterpret_cast<const float4 *>(p + 4);
          v[u][0] = a.x; v[u][1] = a.y; v[u][2] = a.z; v[u][3] = a.w;
          v[u][4] = b.x; v[u][5] = b.y; v[u][6] = b.z; v[u][7] = b.w;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            v[u][j] = (gr < rows && k + j < kend) ? p[j] : 0.0f;
        }
      } else {
        const int r = unit % R, kq = unit / R;
        const int gr = row0 + r, k = k0 + kq * KPT;
        const float *p = src + (int64_t)k * ld + gr;
        if (gr < rows && k + KPT <= kend) {
#pragma unroll
          for (int j = 0; j < KPT; ++j) v[u][j] = p[(int64_t)j * ld];
        } else {
#pragma unroll
          for (int j = 0; j < KPT; ++j)
            v[u][j] = (gr < rows && k + j < kend) ? p[(int64_t)j * ld] : 0.0f;
        }
      }
    }
  }

  // split and write the three planes (plane stride PL bytes)
  template <int PL>
  __device__ __forceinline__ void store(char *lds, int tid) const {
#pragma unroll
    for (int u = 0; u < UPT; ++u) {
      const int unit = tid + u * NT;
      if (unit >= UNITS) break;
      int r, c0;
      if constexpr (KC) {
        r = unit >> 2;
        c0 = unit & 3;
      } else {
        r = unit % R;
        c0 = (unit / R) * (KPT / 8);
      }
#pragma unroll
      for (int cc = 0; cc < KPT / 8; ++cc) {
        uint4 h, m, l;
        split8(&v[u][cc * 8], h, m, l);
        const int off = swz(r, c0 + cc);
        *reinterpret_cast<uint4 *>(lds + off) = h;
        *reinterpret_cast<uint4 *>(lds + PL + off) = m;
        *reinterpret_cast<uint4 *>(lds + 2 * PL + off) = l;
      }
    }
  }
};

__device__ __forceinline__ f32x16 mfma(const bf16x8 &a, const bf16x8 &b, const f32x16 &c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(NT, 1) void gemm_x6_kernel(GemmX6Args p) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  // XCD-aware order: consecutive logical ids run on one XCD (blocks are
  // dealt round-robin over the 8 XCDs) and share the A rows of one tile_m.
  const int nb = gridDim.x, b = blockIdx.x;
  const int xcd = b & 7, q = nb >> 3, rr = nb & 7;
  const int lid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (b >> 3);
  const int split = lid % p.ksplit;
  const int rest = lid / p.ksplit;
  const int tn = rest % p.tiles_n, tm = rest / p.tiles_n;
  const int row0 = tm * BM, col0 = tn * BN;
  const int kbeg = split * p.kps;
  const int kend = min(p.K, kbeg + p.kps);
  const int T = kend > kbeg ? (kend - kbeg + BK - 1) / BK : 0;

  TileLoader<BM, A_KC> la;
  TileLoader<BN, B_KC> lb;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.0f;

  if (T > 0) {
    la.load(p.A, p.lda, row0, p.M, kbeg, kend, tid);
    lb.load(p.B, p.ldb, col0, p.N, kbeg, kend, tid);
    la.template store<A_PLANE>(lds, tid);
    lb.template store<B_PLANE>(lds + 3 * A_PLANE, tid);
    __syncthreads();
    if (T > 1) {
      la.load(p.A, p.lda, row0, p.M, kbeg + BK, kend, tid);
      lb.load(p.B, p.ldb, col0, p.N, kbeg + BK, kend, tid);
    }
  }

  const int ar = wm * 64 + (lane & 31), br = wn * 64 + (lane & 31);
  const int half = lane >> 5;
  // one k16 half of a step: 12 fragment reads, 24 MFMAs
  auto half_step = [&](const char *bufA, int s) {
    const char *bufB = bufA + 3 * A_PLANE;
    bf16x8 a[2][3], bb[2][3];
    const int c = 2 * s + half;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
        a[i][pl] = *reinterpret_cast<const bf16x8 *>(bufA + pl * A_PLANE + swz(ar + 32 * i, c));
        bb[i][pl] = *reinterpret_cast<const bf16x8 *>(bufB + pl * B_PLANE + swz(br + 32 * i, c));
      }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        f32x16 x = acc[i][j];
        x = mfma(a[i][2], bb[j][0], x);  // lh
        x = mfma(a[i][0], bb[j][2], x);  // hl
        x = mfma(a[i][1], bb[j][1], x);  // mm
        x = mfma(a[i][1], bb[j][0], x);  // mh
        x = mfma(a[i][0], bb[j][1], x);  // hm
        x = mfma(a[i][0], bb[j][0], x);  // hh
        acc[i][j] = x;
      }
  };
  auto split_next = [&](int t) {
    char *nA = lds + ((t + 1) & 1) * BUF;
    la.template store<A_PLANE>(nA, tid);
    lb.template store<B_PLANE>(nA + 3 * A_PLANE, tid);
  };
  // waves 4-7 split the next step's operands between their two MFMA halves,
  // waves 0-3 after both, so the two waves of a SIMD (w, w + 4) alternate
  // their vector and matrix phases (c2 FC GEMMs 1.655 -> 1.636 ms)
  const bool late = wave < 4;
  for (int t = 0; t < T; ++t) {
    const char *buf = lds + (t & 1) * BUF;
    half_step(buf, 0);
    if (!late && t + 1 < T) split_next(t);
    half_step(buf, 1);
    if (late && t + 1 < T) split_next(t);
    if (t + 2 < T) {
      la.load(p.A, p.lda, row0, p.M, kbeg + (t + 2) * BK, kend, tid);
      lb.load(p.B, p.ldb, col0, p.N, kbeg + (t + 2) * BK, kend, tid);
    }
    __syncthreads();
  }

  // C/D map of 32x32x16: register g of lane l holds
  // row (g & 3) + 8 (g >> 2) + 4 (l >> 5), column l & 31.
  float *out = p.partial ? p.C + (int64_t)split * p.M * p.N : p.C;
  const int ldo = p.partial ? p.N : p.ldc;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = col0 + wn * 64 + j * 32 + (lane & 31);
      if (col >= p.N) continue;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int row = row0 + wm * 64 + i * 32 + (g & 3) + 8 * (g >> 2) + 4 * half;
        if (row >= p.M) continue;
        float *o = out + (int64_t)row * ldo + col;
        if (p.partial) *o = acc[i][j][g];
        else *o = p.beta == 0.0f ? p.alpha * acc[i][j][g]
                                 : p.alpha * acc[i][j][g] + p.beta * *o;
      }
    }
}

// ---------------------------------------------------------------------------
// gemm_x6d_kernel: gemm_x6_kernel (same tiles, images, MFMA order: bitwise the
// same C) with its operand prefetch two K steps deep instead of one.  In
// gemm_x6_kernel the loads of tile t+2 go out at the end of step t and are
// split during step t+1, about 1.3 us later: an HBM miss under full load can
// take longer (rocprofv3: 40-54 % MFMA busy at 2.0-2.2 GHz on the c2 FC
// shapes).  Here tile t+3 is loaded at the end of step t into the register
// set that the split of step t just freed, so each load has two steps.  The
// loads are buffer loads with no branch (a row past the matrix, or a step
// past the split, reads past the buffer or re-reads the last tile), so every
// path issues the same loads and the compiler's vmcnt wait before a split
// counts exactly the later tile's loads instead of waiting for all of them.
// Needs whole BK steps (K % BK == 0) and the workgroup's offsets below 2^31
// (the host checks).
template <int R, bool KC>
struct TileLoaderD {
  static constexpr int KPT = KC ? 8 : R * BK / NT;
  static constexpr int UNITS = KC ? R * 4 : R * BK / KPT;
  static constexpr int UPT = (UNITS + NT - 1) / NT;
  static_assert(UNITS % NT == 0 && KPT % 8 == 0, "tile shape");
  float v[UPT][KPT];

  // base: KC, the tile's first row (src + row0 * ld); !KC, the split's first
  // k and the tile's first column (src + kbeg * ld + row0)
  __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rs, int ld, int vrows, int kk,
                                       int tid) {
    constexpr unsigned OOB = 0x80000000u;
#pragma unroll
    for (int u = 0; u < UPT; ++u) {
      const int unit = tid + u * NT;
      if constexpr (KC) {
        const int r = unit >> 2, k = kk + (unit & 3) * 8;
        const unsigned off = r < vrows ? (unsigned)(r * ld + k) * 4u : OOB;
        const auto a = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
        const auto b = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16u, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[u][j] = __uint_as_float(a[j]);
          v[u][4 + j] = __uint_as_float(b[j]);
        }
      } else {
        const int r = unit % R, k = kk + (unit / R) * KPT;
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
          const unsigned off = r < vrows ? (unsigned)((k + j) * ld + r) * 4u : OOB;
          v[u][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
        }
      }
    }
  }

  template <int PL>
  __device__ __forceinline__ void store(char *lds, int tid) const {
#pragma unroll
    for (int u = 0; u < UPT; ++u) {
      const int unit = tid + u * NT;
      int r, c0;
      if constexpr (KC) {
        r = unit >> 2;
        c0 = unit & 3;
      } else {
        r = unit % R;
        c0 = (unit / R) * (KPT / 8);
      }
#pragma unroll
      for (int cc = 0; cc < KPT / 8; ++cc) {
        uint4 h, m, l;
        split8(&v[u][cc * 8], h, m, l);
        const int off = swz(r, c0 + cc);
        *reinterpret_cast<uint4 *>(lds + off) = h;
        *reinterpret_cast<uint4 *>(lds + PL + off) = m;
        *reinterpret_cast<uint4 *>(lds + 2 * PL + off) = l;
      }
    }
  }
};

template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(NT, 1) void gemm_x6d_kernel(GemmX6Args p) {
  constexpr int DEPTH = 2;  // prefetch depth, in K steps
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int nb = gridDim.x, b = blockIdx.x;
  const int xcd = b & 7, q = nb >> 3, rr = nb & 7;
  const int lid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (b >> 3);
  const int split = lid % p.ksplit;
  const int rest = lid / p.ksplit;
  const int tn = rest % p.tiles_n, tm = rest / p.tiles_n;
  const int row0 = tm * BM, col0 = tn * BN;
  const int kbeg = split * p.kps;
  const int kend = min(p.K, kbeg + p.kps);
  const int T = kend > kbeg ? (kend - kbeg) / BK : 0;

  const float *baseA = A_KC ? p.A + (int64_t)row0 * p.lda : p.A + (int64_t)kbeg * p.lda + row0;
  const float *baseB = B_KC ? p.B + (int64_t)col0 * p.ldb : p.B + (int64_t)kbeg * p.ldb + col0;
  const __amdgpu_buffer_rsrc_t rsA =
      __builtin_amdgcn_make_buffer_rsrc((void *)baseA, (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB =
      __builtin_amdgcn_make_buffer_rsrc((void *)baseB, (short)0, 0x7fffffff, 0x00020000);
  const int vra = p.M - row0, vrb = p.N - col0;
  // k of tile t relative to the base (clamped to the last tile: a re-read)
  auto kk = [&](int t, bool kc) { return (kc ? kbeg : 0) + min(t, T - 1) * BK; };

  TileLoaderD<BM, A_KC> la[DEPTH];
  TileLoaderD<BN, B_KC> lb[DEPTH];
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.0f;
  if (T == 0) goto epilogue;

  la[0].load(rsA, p.lda, vra, kk(0, A_KC), tid);
  lb[0].load(rsB, p.ldb, vrb, kk(0, B_KC), tid);
  la[0].template store<A_PLANE>(lds, tid);
  lb[0].template store<B_PLANE>(lds + 3 * A_PLANE, tid);
  // tiles 1..DEPTH into sets 1, .., 0 in order, as at every later loop entry
  // (the vmcnt wait before tile 1's split then leaves the later tiles' loads
  // in flight)
#pragma unroll
  for (int j = 1; j <= DEPTH; ++j) {
    __builtin_amdgcn_sched_barrier(0);
    la[j % DEPTH].load(rsA, p.lda, vra, kk(j, A_KC), tid);
    lb[j % DEPTH].load(rsB, p.ldb, vrb, kk(j, B_KC), tid);
  }
  __syncthreads();
  {
    const int ar = wm * 64 + (lane & 31), br = wn * 64 + (lane & 31);
    const int half = lane >> 5;
    auto half_step = [&](const char *bufA, int s) {
      const char *bufB = bufA + 3 * A_PLANE;
      bf16x8 a[2][3], bb[2][3];
      const int c = 2 * s + half;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
          a[i][pl] = *reinterpret_cast<const bf16x8 *>(bufA + pl * A_PLANE + swz(ar + 32 * i, c));
          bb[i][pl] = *reinterpret_cast<const bf16x8 *>(bufB + pl * B_PLANE + swz(br + 32 * i, c));
        }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          f32x16 x = acc[i][j];
          x = mfma(a[i][2], bb[j][0], x);  // lh
          x = mfma(a[i][0], bb[j][2], x);  // hl
          x = mfma(a[i][1], bb[j][1], x);  // mm
          x = mfma(a[i][1], bb[j][0], x);  // mh
          x = mfma(a[i][0], bb[j][1], x);  // hm
          x = mfma(a[i][0], bb[j][0], x);  // hh
          acc[i][j] = x;
        }
    };
    // waves 4-7 split the next tile between their two MFMA halves, waves
    // 0-3 after both (gemm_x6_kernel's stagger)
    const bool late = wave < 4;
    // step t: tile t+1 is in set (t+1) % DEPTH, which then takes tile
    // t+1+DEPTH (a step past T, in the last group of DEPTH steps, does no
    // MFMAs but still issues its (clamped) loads: every path then issues the
    // same loads, so the loop header's vmcnt state is known and each split
    // waits only for its own tile)
    auto step = [&](int t, auto &lan, auto &lbn) {
      if (t < T) {
        const char *buf = lds + (t & 1) * BUF;
        char *nA = lds + ((t + 1) & 1) * BUF;
        half_step(buf, 0);
        if (!late && t + 1 < T) {
          lan.template store<A_PLANE>(nA, tid);
          lbn.template store<B_PLANE>(nA + 3 * A_PLANE, tid);
        }
        half_step(buf, 1);
        if (late && t + 1 < T) {
          lan.template store<A_PLANE>(nA, tid);
          lbn.template store<B_PLANE>(nA + 3 * A_PLANE, tid);
        }
      }
      lan.load(rsA, p.lda, vra, kk(t + 1 + DEPTH, A_KC), tid);
      lbn.load(rsB, p.ldb, vrb, kk(t + 1 + DEPTH, B_KC), tid);
      __syncthreads();
    };
    for (int t = 0; t < T; t += DEPTH) {
#pragma unroll
      for (int i = 0; i < DEPTH; ++i) step(t + i, la[(i + 1) % DEPTH], lb[(i + 1) % DEPTH]);
    }
  }
epilogue:
  float *out = p.partial ? p.C + (int64_t)split * p.M * p.N : p.C;
  const int ldo = p.partial ? p.N : p.ldc;
  const int half2 = lane >> 5;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = col0 + wn * 64 + j * 32 + (lane & 31);
      if (col >= p.N) continue;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int row = row0 + wm * 64 + i * 32 + (g & 3) + 8 * (g >> 2) + 4 * half2;
        if (row >= p.M) continue;
        float *o = out + (int64_t)row * ldo + col;
        if (p.partial) *o = acc[i][j][g];
        else *o = p.beta == 0.0f ? p.alpha * acc[i][j][g]
                                 : p.alpha * acc[i][j][g] + p.beta * *o;
      }
    }
}

// C = alpha * sum_s part[s] + beta * C, the splits added in increasing s
__global__ void gemm_x6_reduce_kernel(const float *__restrict__ part, int S, int M,
                                      int N, float alpha, float beta, float *C,
                                      int ldc) {
  const int64_t n4 = N / 4;
  const int64_t total = (int64_t)M * n4;
  const int64_t plane = (int64_t)M * N;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / n4, c = (e - r * n4) * 4;
    float4 s = *reinterpret_cast<const float4 *>(part + r * N + c);
    for (int k = 1; k < S; ++k) {
      const float4 v = *reinterpret_cast<const float4 *>(part + k * plane + r * N + c);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    float *o = C + r * ldc + c;
    if (beta == 0.0f) {
      o[0] = alpha * s.x; o[1] = alpha * s.y; o[2] = alpha * s.z; o[3] = alpha * s.w;
    } else {
      o[0] = alpha * s.x + beta * o[0]; o[1] = alpha * s.y + beta * o[1];
      o[2] = alpha * s.z + beta * o[2]; o[3] = alpha * s.w + beta * o[3];
    }
  }
}

__global__ void gemm_x6_reduce_scalar_kernel(const float *__restrict__ part, int S,
                                             int M, int N, float alpha, float beta,
                                             float *C, int ldc) {
  const int64_t total = (int64_t)M * N;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    float s = part[e];
    for (int k = 1; k < S; ++k) s += part[k * total + e];
    const int64_t r = e / N, c = e - r * N;
    float *o = C + r * ldc + c;
    *o = beta == 0.0f ? alpha * s : alpha * s + beta * *o;
  }
}

// ---------------------------------------------------------------------------
// LDS images of the plane GEMM below.  A K-contiguous operand keeps the
// [row][k] image (64-B rows, swz) read by ds_read_b128.  A row-contiguous one
// ([k][row] in memory: op(A) = A^T or B not transposed) has a [k][row] image;
// the MFMA fragment comes from it by ds_read_b64_tr_b16 (lane 4q + p of each
// 16-lane group addresses k-row q, columns 4p..4p+3; lane i gets column i of
// the 4 rows).  16-B chunks are XOR-swizzled by (k & 3) << 2, so the four
// k-rows of one transposed read hit four disjoint 16-bank groups.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// offset of (k, col) in a [k][R] transposed image, 16-B chunks swizzled
template <int R>
__device__ __forceinline__ int tswz(int k, int col) {
  return k * (R * 2) + ((((col >> 3) ^ ((k & 3) << 2))) << 4) + ((col & 7) << 1);
}

// MFMA fragment (32 rows from rb, k16 half s) of one plane
template <int R, bool KC>
__device__ __forceinline__ bf16x8 frag(const char *plane, int rb, int s, int lane) {
  if constexpr (KC) {
    return *reinterpret_cast<const bf16x8 *>(plane + swz(rb + (lane & 31), 2 * s + (lane >> 5)));
  } else {
    const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
    const int k = 16 * s + 8 * (g >> 1) + q;
    const int col = rb + 16 * (g & 1) + 4 * pp;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (lds_s16x4 *)(plane + tswz<R>(k, col)));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (lds_s16x4 *)(plane + tswz<R>(k + 4, col)));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 c = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, c);
  }
}

// ---------------------------------------------------------------------------
// Plane GEMM: both operands already split into their three bf16 planes in
// HBM (kl_split_planes), so the K step is pure data movement and MFMAs.
// Tiles reach LDS by LDS-DMA (buffer_load ... lds: 1 KiB per wave
// instruction, no VGPRs, no VALU): the lane of each 16-B LDS slot reads the
// global chunk that the swizzled image wants there (a permutation of 16-B
// chunks, so `frag` reads the images described above).  A K step is phase A
// (the MFMAs of k16 half 0, the fragment reads of half 1) | barrier | phase B
// (the MFMAs of half 1, the next tile's fragment reads of half 0);
// the DMA of tile t+2 is issued in phase B of step t into the buffer whose
// last reads finished before that step's barrier, and the next barrier
// (s_waitcnt vmcnt(0) + s_barrier) publishes it.
typedef __attribute__((address_space(3))) void lds_void_t;

struct GemmPlanesArgs {
  const uint16_t *A, *B;     // plane 0; plane p at + p * ps (elements)
  int64_t aps, bps;
  float *C;
  int M, N, K, lda, ldb, ldc;  // lda / ldb in bf16 elements
  int kps, ksplit, tiles_m, tiles_n;
  float alpha, beta;
  int partial;
};

// 1-KiB DMA segments per K step: A 3 x 16, B 3 x 8; wave w issues w + 8 i
constexpr int SEG_A = A_PLANE / 1024, SEG_B = B_PLANE / 1024;
constexpr int NSEG = 3 * (SEG_A + SEG_B), SEG_PER_WAVE = NSEG / 8;
static_assert(NSEG % 8 == 0, "segments per wave");

// byte offset (relative to the tile's k = kbeg origin of plane 0) that lane j
// of segment s of plane p reads, or an out-of-range marker for rows >= rows
template <int R, bool KC>
__device__ __forceinline__ int seg_src(int p, int s, int j, int ld, int64_t ps, int row0,
                                       int rows) {
  const int slot = s * 64 + j;
  if constexpr (KC) {
    const int r = slot >> 2, cs = slot & 3;
    const int c = cs ^ ((r >> 2) & 3);
    return row0 + r < rows ? (int)(p * ps * 2) + r * ld * 2 + c * 16 : (int)0x80000000;
  } else {
    constexpr int CPR = R / 8;  // 16-B chunks per k-row
    const int k = slot / CPR, cs = slot % CPR;
    const int c = cs ^ ((k & 3) << 2);
    return row0 + 8 * c < rows ? (int)(p * ps * 2) + k * ld * 2 + c * 16 : (int)0x80000000;
  }
}

template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(NT, 1) void gemm_planes_kernel(GemmPlanesArgs p) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  const int nb = gridDim.x, b = blockIdx.x;
  const int xcd = b & 7, q = nb >> 3, rr = nb & 7;
  const int lid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (b >> 3);
  const int split = lid % p.ksplit;
  const int rest = lid / p.ksplit;
  const int tn = rest % p.tiles_n, tm = rest / p.tiles_n;
  const int row0 = tm * BM, col0 = tn * BN;
  const int kbeg = split * p.kps;
  const int T = min(p.kps, p.K - kbeg) / BK;

  const uint16_t *abase = A_KC ? p.A + (int64_t)row0 * p.lda + kbeg
                               : p.A + (int64_t)kbeg * p.lda + row0;
  const uint16_t *bbase = B_KC ? p.B + (int64_t)col0 * p.ldb + kbeg
                               : p.B + (int64_t)kbeg * p.ldb + col0;
  const __amdgpu_buffer_rsrc_t ra =
      __builtin_amdgcn_make_buffer_rsrc((void *)abase, (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb =
      __builtin_amdgcn_make_buffer_rsrc((void *)bbase, (short)0, 0x7fffffff, 0x00020000);
  // this wave's segments: LDS offset within a buffer, source offset, operand
  int soff[SEG_PER_WAVE];
#pragma unroll
  for (int i = 0; i < SEG_PER_WAVE; ++i) {
    const int g = wave + 8 * i;
    if (g < 3 * SEG_A)
      soff[i] = seg_src<BM, A_KC>(g / SEG_A, g % SEG_A, lane, p.lda, p.aps, row0, p.M);
    else
      soff[i] = seg_src<BN, B_KC>((g - 3 * SEG_A) / SEG_B, (g - 3 * SEG_A) % SEG_B, lane,
                                  p.ldb, p.bps, col0, p.N);
  }
  const int akstep = A_KC ? BK * 2 : BK * p.lda * 2;  // bytes per K step
  const int bkstep = B_KC ? BK * 2 : BK * p.ldb * 2;
  auto dma = [&](int tile, int bufi) {
    char *dst = lds + bufi * BUF;
#pragma unroll
    for (int i = 0; i < SEG_PER_WAVE; ++i) {
      const int g = wave + 8 * i;  // wave-uniform
      const bool isa = g < 3 * SEG_A;
      const int ldso = isa ? (g / SEG_A) * A_PLANE + (g % SEG_A) * 1024
                           : 3 * A_PLANE + ((g - 3 * SEG_A) / SEG_B) * B_PLANE +
                                 ((g - 3 * SEG_A) % SEG_B) * 1024;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(isa ? ra : rb, (lds_void_t *)(dst + ldso), 16,
                                               soff[i], tile * (isa ? akstep : bkstep), 0, 0);
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.0f;

  const int ar = wm * 64, br = wn * 64;
  bf16x8 fa0[2][3], fb0[2][3], fa1[2][3], fb1[2][3];
  constexpr int NRA = A_KC ? 1 : 2, NRB = B_KC ? 1 : 2;
  constexpr int NREAD = 6 * NRA + 6 * NRB;
  (void)NRA; (void)NRB;
  auto read_frag = [&](const char *buf, int s, int r, bf16x8 (&fa)[2][3],
                       bf16x8 (&fb)[2][3]) {
    if (r < 6) {
      const int i = r / 3, pl = r % 3;
      fa[i][pl] = frag<BM, A_KC>(buf + pl * A_PLANE, ar + 32 * i, s, lane);
    } else {
      const int i = (r - 6) / 3, pl = (r - 6) % 3;
      fb[i][pl] = frag<BN, B_KC>(buf + 3 * A_PLANE + pl * B_PLANE, br + 32 * i, s, lane);
    }
  };
  auto mfma_n = [&](int n, const bf16x8 (&fa)[2][3], const bf16x8 (&fb)[2][3]) {
    const int i = n / 12, j = (n / 6) & 1, pr = n % 6;
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
    acc[i][j] = mfma(fa[i][PA[pr]], fb[j][PB[pr]], acc[i][j]);
  };

  if (T > 0) {
    dma(0, 0);
    dma(min(1, T - 1), 1);
    kcnn::x6::publish_dma();  // the DMA of both tiles landed, for every wave
#pragma unroll
    for (int r = 0; r < 12; ++r) read_frag(lds, 0, r, fa0, fb0);
  }
  for (int t = 0; t < T; ++t) {
    const char *buf = lds + (t & 1) * BUF;
    const char *nbuf = lds + ((t + 1) & 1) * BUF;
#pragma unroll
    for (int n = 0; n < 24; ++n) {
      mfma_n(n, fa0, fb0);
      if (n >= 2 && n - 2 < NREAD / 2) {
        read_frag(buf, 1, 2 * (n - 2), fa1, fb1);
        read_frag(buf, 1, 2 * (n - 2) + 1, fa1, fb1);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    kcnn::x6::publish_dma();  // the DMA of tile t+1 landed; buffer t & 1 fully read
#pragma unroll
    for (int n = 0; n < 24; ++n) {
      mfma_n(n, fa1, fb1);
      if (n == 0) dma(min(t + 2, T - 1), t & 1);  // past T: the last tile again
      if (n >= 2 && n - 2 < NREAD / 2) {
        read_frag(nbuf, 0, 2 * (n - 2), fa0, fb0);
        read_frag(nbuf, 0, 2 * (n - 2) + 1, fa0, fb0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // a DMA past T may still be in flight: drain it before the LDS is released
  __builtin_amdgcn_s_waitcnt(0);

  float *out = p.partial ? p.C + (int64_t)split * p.M * p.N : p.C;
  const int ldo = p.partial ? p.N : p.ldc;
  const int half = lane >> 5;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = col0 + wn * 64 + j * 32 + (lane & 31);
      if (col >= p.N) continue;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int row = row0 + wm * 64 + i * 32 + (g & 3) + 8 * (g >> 2) + 4 * half;
        if (row >= p.M) continue;
        float *o = out + (int64_t)row * ldo + col;
        if (p.partial) *o = acc[i][j][g];
        else *o = p.beta == 0.0f ? p.alpha * acc[i][j][g]
                                 : p.alpha * acc[i][j][g] + p.beta * *o;
      }
    }
}

// fp32 [rows x cols] (pitch ld) -> planes h, m, l [rows x cols] (pitch ldp,
// plane stride ps elements); 4 columns per thread when aligned
// vec: 16-B loads of 4 fp32 and 8-B stores of 4 bf16 per plane are aligned
// (src 16-B, dst 8-B aligned, ld, ldp and ps multiples of 4; set by the host)
__global__ void split_planes_kernel(const float *__restrict__ src, int rows, int cols, int ld,
                                    uint16_t *__restrict__ dst, int ldp, int64_t ps, int vec) {
  const int c4 = (cols + 3) >> 2;
  const int64_t total = (int64_t)rows * c4;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / c4;
    const int c = (int)(e - r * c4) * 4;
    const float *sp = src + r * ld + c;
    uint16_t *dp = dst + r * ldp + c;
    if (vec && c + 4 <= cols) {
      const float4 v = *reinterpret_cast<const float4 *>(sp);
      uint32_t h0, m0, l0, h1, m1, l1;
      split2(v.x, v.y, h0, m0, l0);
      split2(v.z, v.w, h1, m1, l1);
      *reinterpret_cast<uint2 *>(dp) = make_uint2(h0, h1);
      *reinterpret_cast<uint2 *>(dp + ps) = make_uint2(m0, m1);
      *reinterpret_cast<uint2 *>(dp + 2 * ps) = make_uint2(l0, l1);
    } else {
      for (int i = c; i < cols && i < c + 4; ++i) {
        uint32_t h, m, l;
        split2(src[r * ld + i], 0.0f, h, m, l);
        dst[r * ldp + i] = (uint16_t)h;
        dst[r * ldp + i + ps] = (uint16_t)m;
        dst[r * ldp + i + 2 * ps] = (uint16_t)l;
      }
    }
  }
}

// f(A_KC, B_KC) with the two layouts as std::true_type / std::false_type: a
// kernel's template parameters from the call's transposes
template <typename F>
void with_layouts(bool a_kc, bool b_kc, F f) {
  kcnn::with_bool(a_kc, [&](auto A) { kcnn::with_bool(b_kc, [&](auto B) { f(A, B); }); });
}

// K splits for a tile count: the fraction of the last wave of workgroups
// that is busy, less a small charge per extra split (partials + reduction)
int choose_ksplit(int64_t tiles, int K) {
  int best = 1;
  double best_score = -1.0;
  for (int s = 1; s <= 4; ++s) {
    if (s > 1 && K / s < 1024) break;
    const int64_t nb = tiles * s;
    const int64_t waves = (nb + 255) / 256;
    const double score = (double)nb / (double)(waves * 256) - 0.02 * (s - 1);
    if (score > best_score + 1e-9) { best_score = score; best = s; }
  }
  return best;
}

// The tiles and the split-K set-up of a call (a: GemmX6Args or GemmPlanesArgs
// with M, N and K set): the split count, cut to 1 without the workspace for
// it, the K span per split, and the kernel's output, the partial slabs in the
// workspace when split and the caller's C otherwise.  Returns the grid's
// workgroups.
template <typename Args>
int64_t split_k_setup(Args &a, float *C, void *ws, size_t ws_bytes) {
  a.tiles_m = (a.M + BM - 1) / BM;
  a.tiles_n = (a.N + BN - 1) / BN;
  const int64_t tiles = (int64_t)a.tiles_m * a.tiles_n;
  int s = choose_ksplit(tiles, a.K);
  const size_t need = s > 1 ? sizeof(float) * (size_t)s * a.M * a.N : 0;
  if (need > ws_bytes || !ws) s = 1;
  a.ksplit = s;
  a.kps = ((a.K + s - 1) / s + BK - 1) / BK * BK;
  a.partial = s > 1;
  a.C = s > 1 ? static_cast<float *>(ws) : C;
  return tiles * s;
}
// C = alpha * (the sum of the s slabs at ws) + beta * C, by quads where C allows
int reduce_launch(const void *ws, int s, int M, int N, float alpha, float beta, float *C, int ldc,
                  hipStream_t st) {
  if (N % 4 == 0 && ldc % 4 == 0 && (uintptr_t)C % 16 == 0)
    hipLaunchKernelGGL(gemm_x6_reduce_kernel, dim3(kcnn::grid_for((int64_t)M * (N / 4))),
                       dim3(256), 0, st, (const float *)ws, s, M, N, alpha, beta, C, ldc);
  else
    hipLaunchKernelGGL(gemm_x6_reduce_scalar_kernel, dim3(kcnn::grid_for((int64_t)M * N)),
                       dim3(256), 0, st, (const float *)ws, s, M, N, alpha, beta, C, ldc);
  return kcnn::launch_status();
}

}  // namespace

extern "C" size_t kl_gemm_x6_workspace_bytes(int M, int N, int K) {
  const int64_t tiles = (int64_t)((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  const int s = choose_ksplit(tiles, K);
  return s > 1 ? sizeof(float) * (size_t)s * M * N : 0;
}

// C[M x N] = alpha * op(A) op(B) + beta * C, row-major; op(A) is A^T when
// transA (A stored K x M), op(B) is B^T when transB (B stored N x K).
extern "C" int kl_gemm_x6(int transA, int transB, int M, int N, int K, float alpha,
                          const float *A, int lda, const float *B, int ldb, float beta,
                          float *C, int ldc, void *ws, size_t ws_bytes,
                          kcnn_stream_t stream) {
  if (M < 0 || N < 0 || K < 0) return (int)hipErrorInvalidValue;
  if (M == 0 || N == 0) return 0;
  // 16-B operand loads on the K-contiguous side
  const bool a_kc = !transA, b_kc = transB != 0;
  if ((a_kc && (lda % 4 || (uintptr_t)A % 16)) || (b_kc && (ldb % 4 || (uintptr_t)B % 16)))
    return (int)hipErrorInvalidValue;
  hipStream_t st = kcnn::as_stream(stream);
  GemmX6Args a;
  a.A = A; a.B = B; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb;
  a.alpha = alpha; a.beta = beta; a.ldc = ldc;
  const int64_t nb = split_k_setup(a, C, ws, ws_bytes);
  if (nb >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
  // two-deep prefetch kernel: whole BK steps, the workgroup's offsets below 2^31
  auto deep_fits = [&](bool kc, int ld, int R) {
    if (kc) return (int64_t)R * ld * 4 + (int64_t)K * 4 < ((int64_t)1 << 31);
    return (int64_t)(a.kps + 1) * ld * 4 + (int64_t)R * 4 < ((int64_t)1 << 31);
  };
  const bool deep = K % BK == 0 && deep_fits(a_kc, lda, BM) && deep_fits(b_kc, ldb, BN);
  with_layouts(a_kc, b_kc, [&](auto A, auto B) {
    constexpr bool AKC = decltype(A)::value, BKC = decltype(B)::value;
    if (deep) kcnn::launch_lds<&gemm_x6d_kernel<AKC, BKC>, LDS_BYTES>(a, (unsigned)nb, NT, st);
    else kcnn::launch_lds<&gemm_x6_kernel<AKC, BKC>, LDS_BYTES>(a, (unsigned)nb, NT, st);
  });
  const int rc = kcnn::launch_status();
  if (rc || a.ksplit == 1) return rc;
  return reduce_launch(ws, a.ksplit, M, N, alpha, beta, C, ldc, st);
}

extern "C" int kl_split_planes(const float *src, int rows, int cols, int ld, uint16_t *dst,
                               int ldp, int64_t ps, kcnn_stream_t stream) {
  if (rows < 0 || cols < 0 || ld < cols || ldp < cols) return (int)hipErrorInvalidValue;
  if (rows == 0 || cols == 0) return 0;
  const int vec = ((ld | ldp) & 3) == 0 && (ps & 3) == 0 && (uintptr_t)src % 16 == 0 &&
                  (uintptr_t)dst % 8 == 0;
  hipLaunchKernelGGL(split_planes_kernel,
                     dim3(kcnn::grid_for((int64_t)rows * ((cols + 3) / 4))), dim3(256), 0,
                     kcnn::as_stream(stream), src, rows, cols, ld, dst, ldp, ps, vec);
  return kcnn::launch_status();
}

// C = alpha op(A) op(B) + beta C from plane-split operands (kl_split_planes
// layout: op(A) = A^T when transA, A stored K x M; op(B) = B^T when transB).
// Needs K % 32 == 0, lda / ldb % 8 == 0, 16-B aligned planes, and on a
// row-contiguous operand (A^T or B) its row count % 8 == 0; returns
// hipErrorNotSupported otherwise (the caller uses kl_gemm_x6).
extern "C" size_t kl_gemm_planes_workspace_bytes(int M, int N, int K) {
  return kl_gemm_x6_workspace_bytes(M, N, K);
}
extern "C" int kl_gemm_planes(int transA, int transB, int M, int N, int K, float alpha,
                              const uint16_t *A, int lda, int64_t aps, const uint16_t *B,
                              int ldb, int64_t bps, float beta, float *C, int ldc, void *ws,
                              size_t ws_bytes, kcnn_stream_t stream) {
  if (M < 0 || N < 0 || K < 0) return (int)hipErrorInvalidValue;
  if (M == 0 || N == 0) return 0;
  const bool a_kc = !transA, b_kc = transB != 0;
  auto ok = [&](bool kc, const uint16_t *ptr, int ld, int64_t ps, int rows, int R) {
    if (ld % 8 || ps % 8 || (uintptr_t)ptr % 16) return false;
    if (!kc && rows % 8) return false;
    const int64_t span = kc ? (int64_t)R * ld * 2 + (int64_t)K * 2 : (int64_t)(K + BK) * ld * 2;
    return 2 * ps * 2 + span < ((int64_t)1 << 31);
  };
  if (K % BK || !ok(a_kc, A, lda, aps, M, BM) || !ok(b_kc, B, ldb, bps, N, BN))
    return (int)hipErrorNotSupported;
  hipStream_t st = kcnn::as_stream(stream);
  GemmPlanesArgs a;
  a.A = A; a.B = B; a.aps = aps; a.bps = bps; a.M = M; a.N = N; a.K = K;
  a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.alpha = alpha; a.beta = beta;
  const int64_t nb = split_k_setup(a, C, ws, ws_bytes);
  if (nb >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
  with_layouts(a_kc, b_kc, [&](auto A, auto B) {
    kcnn::launch_lds<&gemm_planes_kernel<decltype(A)::value, decltype(B)::value>, LDS_BYTES>(
        a, (unsigned)nb, NT, st);
  });
  const int rc = kcnn::launch_status();
  if (rc || a.ksplit == 1) return rc;
  return reduce_launch(ws, a.ksplit, M, N, alpha, beta, C, ldc, st);
}
