// kaldi-lite/cu-gemm-f16x3.hip -- fp32 GEMM on the f16 matrix cores from a
// two-part f16 split of each operand under a power-of-two scale per output
// row and column (the "f16x3" scheme, AddMatMat's default engine).
//
// Upstream Kaldi's CuMatrixBase::AddMatMat is cuBLAS sgemm; the reference
// calls it for the FullyConnectedComponent forward, data gradient and update
// (nnet-component.cc:1225-1227, :1247; nnet-component-nnet0.cc:1137-1142).
// The bf16x6 kernel (cu-gemm-x6.hip) reaches fp32 accuracy with six bf16
// products per fp32 product.  f16 carries 11 significant bits to bf16's 8,
// so two parts suffice once the operands are scaled into f16's range:
//
//   x' = x * 2^s   (s per row of op(A) / column of op(B): the row's largest
//                   |x'| lies in [2^14, 2^15))
//   hi = f16(x'),  lo = f16(x' - hi)        (x' - hi is exact in fp32)
//
// x' = hi + lo to within 2^-22 |x'| while |x'| >= 2^-3; below that lo is an
// f16 subnormal and the error is under 2^-25 absolute, 2^-39 of the row's
// largest element.  With every f16 product exact in fp32,
//
//   a'b' = hi.hi + (hi.lo + lo.hi) + lo.lo
//
// and the kernel keeps the first three (one v_mfma_f32_32x32x16_f16 each,
// smallest first, accumulated in fp32), then C = acc * 2^-(s_a + s_b) by an
// exact ldexp.  The bound is therefore per group, not per product: for two
// groups that are not "spread" (no element more than 20 binades under the
// group's max, f16-split.h) every element is held to 2^-19, and a product is
// within (2 * 2^-19 + 2^-22) S of exact; a product touching a spread group
// is checked at its store against the count of the group's small elements
// and recomputed in fp32 when the check cannot clear it (tile_epilogue;
// gemm_f16x3_reduce_kernel, cu-gemm-f16x3-reduce.hip).  So every finite C
// element meets the 1e-5 * S parity bar whatever the operands' range; the scale puts a
// whole row near FLT_MAX or of fp32 subnormals into f16's range like any
// other (the bf16x6 split loses bits there).  The f16 MFMA runs at the bf16
// rate: half the matrix-core work of bf16x6 for the same split VALU.
//
// The scales come from per-row / per-column max |x| (cu-f16-stats.hip,
// kl_absmax_rows / kl_absmax_cols: the bit patterns of |x|, whose unsigned
// order is the magnitude order).  A row of
// op(A) or a column of op(B) holding Inf or NaN has no scale; every C
// element in it is Inf or NaN in IEEE arithmetic.  The main loop leaves
// those elements alone and the tile's split-0 workgroup computes them as
// plain fp32 dot products (tile_epilogue), which gives sgemm's IEEE pattern
// (+Inf, -Inf or NaN).
//
// Structure: gemm_x6d_kernel's (cu-gemm-x6.hip): 512 threads, a 256 x 128
// tile of C per workgroup (8 waves of 2 x 2 accumulators of 32 x 32), K steps
// of 32, operands loaded as fp32 by branch-free buffer loads two steps ahead,
// split in registers into two f16 planes of swizzled [row][k] LDS images
// (double-buffered, 2 x 48 KB), one barrier per step; or, where the call's
// plan says so (choose_plan), a 256 x 256 tile (8 waves of 4 x 2 accumulators,
// 2 x 64 KB; gemm_f16x3_fast_kernel with BN_WIDE).  Thin outputs split K
// over workgroups into partial slabs, which gemm_f16x3_reduce_kernel
// (cu-gemm-f16x3-reduce.hip) sums in a fixed order.  What both files' kernels
// use is in gemm-f16x3-dev.h.
#include <atomic>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "cnslmat/f16-split.h"
#include "cnslmat/hip-util.h"
#include "kaldi-lite/cu-kernels-lite.h"
#include "kaldi-lite/f16-stats.h"
#include "kaldi-lite/gemm-f16x3-dev.h"
#include "kaldi-lite/kcnn-knobs.h"
#include "kaldi-lite/launch-lds.h"

namespace {

using namespace kcnn::f16x3;
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

constexpr int NT = 512;
constexpr int ROWB = BK * 2;                  // bytes per LDS row of one plane
constexpr int A_PLANE = BM * ROWB;            // 16 KB
template <int BN>
struct Tile {
  static constexpr int WN = BN / 64;             // waves along the columns
  static constexpr int WR = BM / (8 / WN);       // rows per wave
  static constexpr int MI = WR / 32;             // accumulator rows per wave
  static constexpr int B_PLANE = BN * ROWB;      // 8 / 16 KB
  static constexpr int BUF = 2 * (A_PLANE + B_PLANE);   // 48 / 64 KB
  static constexpr int LDS_BYTES = 2 * BUF + (BM + BN) * 8;  // + sexp, sw
};

// Tile t of the order -> (tile row, tile column).  The tiles go in groups of
// GM tile rows, column-major inside a group, so the 32 workgroups an XCD runs
// at once (consecutive logical ids, block_tile) cover about 32 / GM tile
// columns of GM tile rows, sharing GM row panels of op(A) and a few column
// panels of op(B) in that XCD's L2, instead of one row panel and 32 column
// panels (c2's data gradient: an XCD wave then reads 8 MB of operand panels
// instead of 17).  (Back: tile_index, gemm-f16x3-dev.h.)
__device__ __forceinline__ void tile_rc(const GemmF16Args &p, int t, int &tm, int &tn) {
  const int gsz = GM * p.tiles_n;
  const int g = t / gsz, r = t - g * gsz;
  const int m0 = g * GM;
  const int gm = min(p.tiles_m - m0, GM);
  tm = m0 + r % gm;
  tn = r / gm;
}
// This workgroup's (split, tile row, tile column); true for a whole tile.
// Blocks [0, nwhole) take tiles [0, nwhole) over all of K, the others the
// ksplit splits of the remaining tiles (consecutive logical ids: the splits
// of one tile).  Each part in the XCD-aware order (gemm_x6_kernel): block b
// runs on XCD b & 7, and consecutive logical ids go to one XCD (nwhole is a
// multiple of 256, so both parts keep that phase and every XCD gets an
// eighth of each).  nwhole 0: the plain split grid.
__device__ __forceinline__ bool block_tile(const GemmF16Args &p, int &split, int &tm, int &tn) {
  const bool whole = (int)blockIdx.x < p.nwhole;
  const int b = whole ? (int)blockIdx.x : (int)blockIdx.x - p.nwhole;
  const int nb = whole ? p.nwhole : (int)gridDim.x - p.nwhole;
  const int ks = whole ? 1 : p.ksplit;
  const int xcd = b & 7, q = nb >> 3, rr = nb & 7;
  const int lid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (b >> 3);
  split = lid % ks;
  tile_rc(p, (whole ? 0 : p.nwhole) + lid / ks, tm, tn);
  return whole;
}

// A workgroup's work: its tile (block_tile), its span of K in steps of BK,
// and, once bound, the operands' buffer descriptors from the tile's first row
// (K-contiguous) or the span's first k (row-contiguous)
template <bool A_KC, bool B_KC, int BN>
struct TileWork {
  int split;
  bool whole;           // the tile over all of K (block_tile)
  int row0, col0;
  int kbeg, T, klast;   // first k, K steps, valid k of the last step
  int vra, vrb;         // the rows of op(A) and columns of op(B) from the tile's first on
  __amdgpu_buffer_rsrc_t rsA, rsB;

  __device__ __forceinline__ explicit TileWork(const GemmF16Args &p) {
    int tm, tn;
    whole = block_tile(p, split, tm, tn);
    row0 = tm * BM; col0 = tn * BN;
    vra = p.M - row0; vrb = p.N - col0;
    kbeg = whole ? 0 : split * p.kps;
    const int kend = whole ? p.K : min(p.K, kbeg + p.kps);
    T = kend > kbeg ? (kend - kbeg + BK - 1) / BK : 0;
    klast = kend - kbeg - (T - 1) * BK;
  }
  // descriptors whose range ends at the operand's last element: a partial
  // last tile reads 0 past it (and the split zeroes the pitch's padding)
  __device__ __forceinline__ void bind(const GemmF16Args &p) {
    const float *baseA = A_KC ? p.A + (int64_t)row0 * p.lda : p.A + (int64_t)kbeg * p.lda + row0;
    const float *baseB = B_KC ? p.B + (int64_t)col0 * p.ldb : p.B + (int64_t)kbeg * p.ldb + col0;
    const int64_t endA = A_KC ? ((int64_t)(vra - 1) * p.lda + p.K) * 4
                              : ((int64_t)(p.K - 1 - kbeg) * p.lda + vra) * 4;
    const int64_t endB = B_KC ? ((int64_t)(vrb - 1) * p.ldb + p.K) * 4
                              : ((int64_t)(p.K - 1 - kbeg) * p.ldb + vrb) * 4;
    rsA = __builtin_amdgcn_make_buffer_rsrc(
        (void *)baseA, (short)0, (int)(endA < 0x7fffffff ? endA : 0x7fffffff), 0x00020000);
    rsB = __builtin_amdgcn_make_buffer_rsrc(
        (void *)baseB, (short)0, (int)(endB < 0x7fffffff ? endB : 0x7fffffff), 0x00020000);
  }
  // k of tile t relative to the base (clamped to the last tile: a re-read)
  __device__ __forceinline__ int kk(int t, bool kc) const {
    return (kc ? kbeg : 0) + min(t, T - 1) * BK;
  }
};

__device__ __forceinline__ int swz(int r, int c) {
  return r * ROWB + ((c ^ ((r >> 2) & 3)) << 4);
}
// offset of (k, col) in a [k][R] image of 16-bit values, 16-B chunks XOR-
// swizzled by (k & 3) << 2 so the four k-rows of one transposed read hit
// four disjoint 16-bank groups (as cu-gemm-x6.hip's tswz)
template <int R>
__device__ __forceinline__ int tswz(int k, int col) {
  return k * (R * 2) + ((((col >> 3) ^ ((k & 3) << 2))) << 4) + ((col & 7) << 1);
}

// Operand tile loaders (R rows of C's side x BK per K step), loads two steps
// ahead by branch-free buffer loads (gemm_x6d_kernel's TileLoaderD), split in
// registers into the hi / lo planes.  Three source layouts:
//   LK  K-contiguous (element (row, k) at src[row * ld + k]): unit = (row,
//       8-k chunk), two 16-B loads; [row][k] image (swz), fragments by
//       ds_read_b128;
//   LR  row-contiguous ([k][row]) with one dword per lane: unit = (row, KPT
//       consecutive k), lanes along the row; [row][k] image;
//   LT  row-contiguous with 16-B loads along the rows (ld % 4 == 0, 16-B
//       base, the row count a multiple of 4): unit = (4 rows, KQ k); [k][row]
//       image (tswz), fragments by ds_read_b64_tr_b16.
// Every row of a unit has its own scale exponent (e[]).
enum { LK = 0, LR = 1, LT = 2 };

template <int R, int MODE>
struct Loader {
  static constexpr int KPT = MODE == LK ? 8 : MODE == LR ? R * BK / NT : R * BK / (NT * 4);
  static constexpr int UNITS = MODE == LK ? R * 4 : MODE == LR ? R * BK / KPT : NT;
  static constexpr int UPT = (UNITS + NT - 1) / NT;
  static constexpr int NE = MODE == LT ? 4 : UPT;  // exponents per thread
  static_assert(UNITS % NT == 0, "tile shape");
  static_assert(MODE != LR || KPT % 8 == 0, "tile shape");
  static_assert(MODE != LT || (R / 4) * (BK / KPT) == NT, "tile shape");
  static constexpr int NV = MODE == LT ? 4 * KPT : KPT;  // values per unit
  float v[UPT][NV];
  int e[NE];

  // first row of exponent i
  __device__ static __forceinline__ int row_of(int i, int tid) {
    if constexpr (MODE == LT) return 4 * (tid % (R / 4)) + i;
    const int unit = tid + i * NT;
    return MODE == LK ? unit >> 2 : unit % R;
  }
  __device__ __forceinline__ void init_exp(const int *sexp, int tid) {
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int s = sexp[row_of(i, tid)];
      e[i] = s == SKIP ? 0 : s;
    }
  }

  // base: LK, the tile's first row (src + row0 * ld); LR / LT, the split's
  // first k and the tile's first column (src + kbeg * ld + row0).  Rows past
  // the matrix read past the buffer's range (0).
  __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rs, int ld, int vrows, int kk,
                                       int tid) {
    constexpr unsigned OOB = 0x80000000u;
#pragma unroll
    for (int u = 0; u < UPT; ++u) {
      const int unit = tid + u * NT;
      if constexpr (MODE == LK) {
        const int r = unit >> 2, k = kk + (unit & 3) * 8;
        const unsigned off = r < vrows ? (unsigned)(r * ld + k) * 4u : OOB;
        const auto a = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
        const auto b = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16u, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[u][j] = __uint_as_float(a[j]);
          v[u][4 + j] = __uint_as_float(b[j]);
        }
      } else if constexpr (MODE == LR) {
        const int r = unit % R, k = kk + (unit / R) * KPT;
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
          const unsigned off = r < vrows ? (unsigned)((k + j) * ld + r) * 4u : OOB;
          v[u][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
        }
      } else {
        const int rq = unit % (R / 4), k = kk + (unit / (R / 4)) * KPT;
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
          const unsigned off = 4 * rq < vrows ? (unsigned)((k + j) * ld + 4 * rq) * 4u : OOB;
          const auto a = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
#pragma unroll
          for (int i = 0; i < 4; ++i) v[u][4 * j + i] = __uint_as_float(a[i]);
        }
      }
    }
  }

  // a unit's row, first 16-B chunk and first k of the step (LK, LR)
  __device__ static __forceinline__ void unit_pos(int unit, int &r, int &c0, int &kb) {
    r = MODE == LK ? unit >> 2 : unit % R;
    c0 = MODE == LK ? unit & 3 : (unit / R) * (KPT / 8);
    kb = MODE == LK ? c0 * 8 : (unit / R) * KPT;
  }

  // split and write the two planes (plane stride PL bytes); kv < BK: the
  // tile is the last, partial one and its k >= kv are zeroed (they are the
  // next row's values or a pitch's padding)
  // (RAG: K is not a whole number of BK steps, so the last tile can be
  // partial; without it no masking code is emitted -- the compiler turns
  // the uniform kv test into per-element selects)
  template <int PL, bool RAG>
  __device__ __forceinline__ void store(char *lds, int tid, int kv, float m1) const {
#pragma unroll
    for (int u = 0; u < UPT; ++u) {
      const int unit = tid + u * NT;
      float x[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) x[j] = v[u][j];
      if constexpr (MODE == LT) {
        const int rq = unit % (R / 4), kq = unit / (R / 4);
        if (RAG && kv < BK) {
#pragma unroll
          for (int j = 0; j < KPT; ++j)
            if (kq * KPT + j >= kv)
#pragma unroll
              for (int i = 0; i < 4; ++i) x[4 * j + i] = 0.0f;
        }
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
          uint32_t h0, l0, h1, l1;
          split2h(x[4 * j], x[4 * j + 1], e[0], e[1], h0, l0, m1);
          split2h(x[4 * j + 2], x[4 * j + 3], e[2], e[3], h1, l1, m1);
          const int o = tswz<R>(kq * KPT + j, 4 * rq);
          *reinterpret_cast<uint2 *>(lds + o) = make_uint2(h0, h1);
          *reinterpret_cast<uint2 *>(lds + PL + o) = make_uint2(l0, l1);
        }
      } else {
        int r, c0, kb;
        unit_pos(unit, r, c0, kb);
        if (RAG && kv < BK) {
#pragma unroll
          for (int j = 0; j < KPT; ++j)
            if (kb + j >= kv) x[j] = 0.0f;
        }
#pragma unroll
        for (int cc = 0; cc < KPT / 8; ++cc) {
          uint32_t h[4], l[4];
#pragma unroll
          for (int i = 0; i < 4; ++i)
            split2h(x[cc * 8 + 2 * i], x[cc * 8 + 2 * i + 1], e[u], e[u], h[i], l[i], m1);
          const int off = swz(r, c0 + cc);
          *reinterpret_cast<uint4 *>(lds + off) = make_uint4(h[0], h[1], h[2], h[3]);
          *reinterpret_cast<uint4 *>(lds + PL + off) = make_uint4(l[0], l[1], l[2], l[3]);
        }
      }
    }
  }

  // The split of store() in NPIECE pieces of one pair each, for the fast
  // kernel's interleaving with MFMAs: piece pc splits one pair into the
  // caller's temporaries; a unit's (LK, LR) or a k-row's (LT) plane writes go
  // with its last piece
  static constexpr int NPIECE = MODE == LT ? 2 * KPT : UPT * (KPT / 2);
  template <int PL, bool RAG>
  __device__ __forceinline__ void piece(char *lds, int tid, int pc, int kv, uint32_t (&ph)[4],
                                        uint32_t (&pl)[4], float m1) const {
    if constexpr (MODE == LT) {
      const int j = pc >> 1, hf = pc & 1;
      const int unit = tid;
      const int rq = unit % (R / 4), kq = unit / (R / 4);
      float x0 = v[0][4 * j + 2 * hf], x1 = v[0][4 * j + 2 * hf + 1];
      if (RAG && kv < BK) {
        asm volatile("");  // a branch: not per-element selects in every K step
        if (kq * KPT + j >= kv) x0 = x1 = 0.0f;
      }
      split2h(x0, x1, e[2 * hf], e[2 * hf + 1], ph[hf], pl[hf], m1);
      if (hf == 1) {
        const int o = tswz<R>(kq * KPT + j, 4 * rq);
        *reinterpret_cast<uint2 *>(lds + o) = make_uint2(ph[0], ph[1]);
        *reinterpret_cast<uint2 *>(lds + PL + o) = make_uint2(pl[0], pl[1]);
      }
    } else {
      constexpr int PPU = KPT / 2;  // pieces per unit
      const int u = pc / PPU, q = pc % PPU;
      const int unit = tid + u * NT;
      int r, c0, kb;
      unit_pos(unit, r, c0, kb);
      float x0 = v[u][2 * q], x1 = v[u][2 * q + 1];
      if (RAG && kv < BK) {
        asm volatile("");  // a branch: not per-element selects in every K step
        if (kb + 2 * q >= kv) x0 = 0.0f;
        if (kb + 2 * q + 1 >= kv) x1 = 0.0f;
      }
      split2h(x0, x1, e[u], e[u], ph[q & 3], pl[q & 3], m1);
      if ((q & 3) == 3) {
        const int off = swz(r, c0 + (q >> 2));
        *reinterpret_cast<uint4 *>(lds + off) = make_uint4(ph[0], ph[1], ph[2], ph[3]);
        *reinterpret_cast<uint4 *>(lds + PL + off) = make_uint4(pl[0], pl[1], pl[2], pl[3]);
      }
    }
  }
  // The loads of load() in NPART parts, each the values of PPP consecutive
  // pieces: the wide tile's loop holds one loader set per operand and issues
  // part q of the next tile as soon as piece() has consumed part q of this one
  static constexpr int NPART = MODE == LT ? KPT : UPT;
  static constexpr int PPP = NPIECE / NPART;
  __device__ __forceinline__ void load_part(__amdgpu_buffer_rsrc_t rs, int ld, int vrows, int kk,
                                            int tid, int q) {
    static_assert(MODE != LR, "the wide tile has no LR loader");
    constexpr unsigned OOB = 0x80000000u;
    if constexpr (MODE == LK) {
      const int unit = tid + q * NT;
      const int r = unit >> 2, k = kk + (unit & 3) * 8;
      const unsigned off = r < vrows ? (unsigned)(r * ld + k) * 4u : OOB;
      const auto a = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
      const auto b = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16u, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[q][j] = __uint_as_float(a[j]);
        v[q][4 + j] = __uint_as_float(b[j]);
      }
    } else {
      const int rq = tid % (R / 4), k = kk + (tid / (R / 4)) * KPT;
      const unsigned off = 4 * rq < vrows ? (unsigned)((k + q) * ld + 4 * rq) * 4u : OOB;
      const auto a = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[0][4 * q + i] = __uint_as_float(a[i]);
    }
  }
  // fragment reads per MFMA fragment (LT: two transposed 8-B reads)
  static constexpr int NRD = MODE == LT ? 2 : 1;

  // MFMA fragment: 32 rows from rb, k16 half s (lane l: row l & 31, k 8 (l >> 5) + 0..7)
  __device__ static __forceinline__ f16x8 frag(const char *plane, int rb, int s, int lane) {
    if constexpr (MODE != LT) {
      return *reinterpret_cast<const f16x8 *>(plane + swz(rb + (lane & 31), 2 * s + (lane >> 5)));
    } else {
      const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
      const int k = 16 * s + 8 * (g >> 1) + q;
      const int col = rb + 16 * (g & 1) + 4 * pp;
      const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_s16x4 *)(plane + tswz<R>(k, col)));
      const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_s16x4 *)(plane + tswz<R>(k + 4, col)));
      const s16x8 c = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      return __builtin_bit_cast(f16x8, c);
    }
  }
};


// The scale exponents of the tile's rows and columns into sexp, and each
// one's spread weight into sw (f16-split.h spread_weight: 0 unless the group
// is spread; -inf for an all-zero group, whose products are exactly 0: the
// threshold sum is then -inf, i.e. no check).  Returns bit 0: one of them is
// an Inf / NaN row or column; bit 1: one of them is spread (both for the
// whole block).
template <int BN>
__device__ __forceinline__ int tile_scales(const GemmF16Args &p, int *sexp, float *sw, int row0,
                                           int col0, int tid) {
  int skip = 0, spr = 0;
  for (int i = tid; i < BM + BN; i += NT) {
    int s = 0;
    float w = 0.0f;
    if (i < BM) {
      if (row0 + i < p.M) {
        const uint32_t m = p.amax[row0 + i];
        s = scale_exp(m);
        w = m == 0 ? -__builtin_inff() : kcnn::f16x3::spread_weight(p.acnt[row0 + i]);
      }
    } else if (col0 + i - BM < p.N) {
      const uint32_t m = p.bmax[col0 + i - BM];
      s = scale_exp(m);
      w = m == 0 ? -__builtin_inff() : kcnn::f16x3::spread_weight(p.bcnt[col0 + i - BM]);
    }
    sexp[i] = s;
    sw[i] = w;
    skip |= s == SKIP;
    spr |= w > 0.0f;
  }
  const int any_skip = __syncthreads_or(skip) != 0;
  return any_skip | (__syncthreads_or(spr) != 0 ? 2 : 0);
}

// C/D map of 32x32x16: register g of lane l holds row (g & 3) + 8 (g >> 2) +
// 4 (l >> 5), column l & 31 of its 32 x 32 block.  cd_row: that row from
// `base` on (half: l >> 5); cd_col: that column of the wave's block j from
// `base` on.  (The base is inside, so that the sums keep one association.)
__device__ __forceinline__ int cd_row(int base, int g, int half) {
  return base + (g & 3) + 8 * (g >> 2) + 4 * half;
}
__device__ __forceinline__ int cd_col(int base, int j, int l) { return base + j * 32 + (l & 31); }

// The tile's results.  Each value is unscaled by 2^-(s_row + s_col) (exact).
//  - One split (or a whole tile of a split grid, block_tile): C = alpha * v
//    + beta * C.
//  - ksplit > 1: the split's values go to its partial slab, which
//    gemm_f16x3_reduce_kernel adds in increasing split order.  (Adding them
//    in the tile's last-arriving workgroup instead needs a device-scope
//    release fence per workgroup, which on gfx950 writes back the XCD's L2:
//    the c2 FC forward went 330 -> 436 us and the weight gradient 368 ->
//    654 us with it.)
//  - Elements of an Inf / NaN row or column are skipped above; split 0's
//    workgroup computes them here as fp32 dot products in increasing k
//    (IEEE Inf / NaN, the reference sgemm's pattern).
template <bool A_KC, bool B_KC, int BN>
__device__ __forceinline__ void tile_epilogue(const GemmF16Args &p, const int *sexp,
                                              const float *sw,
                                              const f32x16 (&acc)[Tile<BN>::MI][2], int split,
                                              bool whole, int row0, int col0, int flags, int tid,
                                              char *lds) {
  constexpr int MI = Tile<BN>::MI, WR = Tile<BN>::WR, WN = Tile<BN>::WN;
  const int lane = tid & 63, wave = tid >> 6, wm = wave / WN, wn = wave % WN;
  const int half2 = lane >> 5;
  const bool partial = p.ksplit > 1 && !whole;
  const bool skip = flags & 1;
  // the spread check (f16-split.h): with a spread row or column in the tile
  // and one split, an element whose |acc| is below its threshold is
  // recomputed in fp32 (fix_rejected) instead of stored; split K checks the
  // summed value in gemm_f16x3_reduce_kernel
  const bool check = (flags & 2) && !partial;
  const int np4 = (p.N + 3) & ~3;  // partial slab pitch (16-B rows)
  float *slab = partial ? p.part + (int64_t)split * p.M * np4 : p.C;
  const int ldo = partial ? np4 : p.ldc;
  // bit (2 (i & 1) + j) * 16 + g of word i >> 1: that element is rejected
  uint64_t rej[MI / 2];
#pragma unroll
  for (int h = 0; h < MI / 2; ++h) rej[h] = 0;
  auto fix = [&]() {
#pragma unroll
    for (int h = 0; h < MI / 2; ++h)
      fix_rejected(p, A_KC, B_KC, rej[h], lane, [&](int l, int n, int &row, int &col) {
        const int i = 2 * h + (n >> 5), j = (n >> 4) & 1, g = n & 15;
        row = cd_row(row0 + wm * WR + i * 32, g, l >> 5);
        col = cd_col(col0 + wn * 64, j, l);
      });
  };
  // A whole tile without Inf / NaN rows or columns (block-uniform): each
  // wave's WR x 64 block through LDS in 32-row passes (the main loop's
  // plane buffers, free after a barrier), then 16-B stores of whole rows:
  // a quarter of the store instructions of the per-register stores below
  // (c2's data gradient: 400 -> 388 us at K 1024).  An element the check
  // rejects is recomputed by its wave (fix_rejected) into its staging slot
  // before the pass is stored, so alpha, beta * C and the bias are applied
  // to it once, by the same 16-B store as its neighbours (a
  // second store_value after the staged store read back the new C).
  // (the momentum update's W and prev have 16-B aligned rows: host check)
  const bool staged = row0 + BM <= p.M && col0 + BN <= p.N && !skip &&
                      (partial || p.mom.W || ((ldo & 3) | ((uintptr_t)slab & 15)) == 0);
  if (staged) {
    __syncthreads();  // every wave past its last read of the plane buffers
    constexpr int SR = 68;  // staging row pitch (floats): 16-B rows, rows 4 apart on other banks
    float *st = reinterpret_cast<float *>(lds) + wave * 32 * SR;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int cl = cd_col(wn * 64, j, lane);
        const int ec = sexp[BM + cl];
        const float wc = check ? sw[BM + cl] : 0.0f;
        const bool bcheck =
            check && (__ballot(wc > 0.0f || sw[wm * WR + i * 32 + (lane & 31)] > 0.0f) != 0);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const int rr = cd_row(0, g, half2);
          const int rl = wm * WR + i * 32 + rr;
          if (bcheck) {
            const float thr = wc + sw[rl];
            if (thr != 0.0f && !(fabsf(acc[i][j][g]) >= thr))
              rej[i >> 1] |= (uint64_t)1 << ((2 * (i & 1) + j) * 16 + g);
          }
          st[cd_col(rr * SR, j, lane)] =
              __builtin_amdgcn_ldexpf(acc[i][j][g], -(sexp[rl] + ec));
        }
      }
      if (check) {
        // this pass's rejections (bits 32 (i & 1) .. + 31 of its word) into their slots
        // (lane 0 writes after every lane's staging write: one wave, LDS in order)
        const uint64_t mine = (rej[i >> 1] >> (32 * (i & 1))) & 0xffffffffull;
        fix_rejected(
            p, A_KC, B_KC, mine, lane,
            [&](int l, int n, int &row, int &col) {
              const int j = (n >> 4) & 1, g = n & 15;
              row = cd_row(row0 + wm * WR + i * 32, g, l >> 5);
              col = cd_col(col0 + wn * 64, j, l);
            },
            [&](int l, int n, int, int, float v) {
              const int j = (n >> 4) & 1, g = n & 15;
              st[cd_col(cd_row(0, g, l >> 5) * SR, j, l)] = v;
            });
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int f = lane + 64 * k, rr = f >> 4, c4 = f & 15;
        const float4 v = *reinterpret_cast<const float4 *>(st + rr * SR + 4 * c4);
        const int row = row0 + wm * WR + i * 32 + rr, col = col0 + wn * 64 + 4 * c4;
        if (!partial && p.mom.W) {  // emit's momentum step, four elements per access
          float4 *wq = reinterpret_cast<float4 *>(p.mom.W + (int64_t)row * p.mom.ldw + col);
          float4 *pq = reinterpret_cast<float4 *>(p.mom.prev + (int64_t)row * p.mom.ldp + col);
          float4 w4 = *wq, q4 = *pq;
          momentum_quad(p, v, w4, q4, wq, pq);
          continue;
        }
        float4 *o = reinterpret_cast<float4 *>(slab + (int64_t)row * ldo + col);
        if (partial) {
          *o = v;
          continue;
        }
        float4 w = make_float4(p.alpha * v.x, p.alpha * v.y, p.alpha * v.z, p.alpha * v.w);
        if (p.beta != 0.0f) {
          const float4 c = *o;
          w = make_float4(p.alpha * v.x + p.beta * c.x, p.alpha * v.y + p.beta * c.y,
                          p.alpha * v.z + p.beta * c.z, p.alpha * v.w + p.beta * c.w);
        }
        if (p.bias) {
          w.x += p.bias[col];
          w.y += p.bias[col + 1];
          w.z += p.bias[col + 2];
          w.w += p.bias[col + 3];
        }
        *o = w;
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int cl = cd_col(wn * 64, j, lane);
      const int col = col0 + cl;
      const int ec = sexp[BM + cl];
      if (col >= p.N || ec == SKIP) continue;
      const float wc = check ? sw[BM + cl] : 0.0f;
      // this 32 x 32 block's check: one of its columns or rows is spread
      // (wave-uniform; most blocks skip it)
      const bool bcheck =
          check && (__ballot(wc > 0.0f || sw[wm * WR + i * 32 + (lane & 31)] > 0.0f) != 0);
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int rl = cd_row(wm * WR + i * 32, g, half2);
        const int row = row0 + rl;
        const int er = sexp[rl];
        if (row >= p.M || er == SKIP) continue;
        if (bcheck) {
          const float thr = wc + sw[rl];
          if (thr != 0.0f && !(fabsf(acc[i][j][g]) >= thr)) {
            rej[i >> 1] |= (uint64_t)1 << ((2 * (i & 1) + j) * 16 + g);
            continue;
          }
        }
        const float v = __builtin_amdgcn_ldexpf(acc[i][j][g], -(er + ec));
        if (partial) slab[(int64_t)row * ldo + col] = v;
        else emit(p, row, col, v);
      }
    }
  if (check) fix();
  if (skip && split == 0) {
    for (int e = tid; e < BM * BN; e += NT) {
      const int rl = e / BN, cl = e - rl * BN;
      const int row = row0 + rl, col = col0 + cl;
      if (row >= p.M || col >= p.N) continue;
      if (sexp[rl] != SKIP && sexp[BM + cl] != SKIP) continue;
      float sum = 0.0f;
      for (int k = 0; k < p.K; ++k) {
        const float a = A_KC ? p.A[(int64_t)row * p.lda + k] : p.A[(int64_t)k * p.lda + row];
        const float b = B_KC ? p.B[(int64_t)col * p.ldb + k] : p.B[(int64_t)k * p.ldb + col];
        sum = fmaf(a, b, sum);
      }
      emit(p, row, col, sum);
    }
  }
}

template <int AM, int BMODE, bool RAG>
__global__ __launch_bounds__(NT, 1) void gemm_f16x3_kernel(GemmF16Args p) {
  constexpr bool A_KC = AM == LK, B_KC = BMODE == LK;
  constexpr int BN = BN_NARROW, B_PLANE = Tile<BN>::B_PLANE, BUF = Tile<BN>::BUF;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  int *sexp = reinterpret_cast<int *>(lds + 2 * BUF);  // [BM] rows, then [BN] columns
  float *sw = reinterpret_cast<float *>(sexp + BM + BN);  // spread weights, the same order
  const int tid = threadIdx.x;
  const float m1 = kcnn::f16x3::opaque_m1();
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  TileWork<A_KC, B_KC, BN> tw(p);
  const int flags = tile_scales<BN>(p, sexp, sw, tw.row0, tw.col0, tid);
  tw.bind(p);

  using LA = Loader<BM, AM>;
  using LB = Loader<BN, BMODE>;
  LA la[2];
  LB lb[2];
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.0f;
  la[0].init_exp(sexp, tid);
  la[1].init_exp(sexp, tid);
  lb[0].init_exp(sexp + BM, tid);
  lb[1].init_exp(sexp + BM, tid);

  if (tw.T > 0) {
    la[0].load(tw.rsA, p.lda, tw.vra, tw.kk(0, A_KC), tid);
    lb[0].load(tw.rsB, p.ldb, tw.vrb, tw.kk(0, B_KC), tid);
    la[0].template store<A_PLANE, RAG>(lds, tid, tw.T == 1 ? tw.klast : BK, m1);
    lb[0].template store<B_PLANE, RAG>(lds + 2 * A_PLANE, tid, tw.T == 1 ? tw.klast : BK, m1);
    // tiles 1, 2 into sets 1, 0 (as at every later loop entry)
    __builtin_amdgcn_sched_barrier(0);
    la[1].load(tw.rsA, p.lda, tw.vra, tw.kk(1, A_KC), tid);
    lb[1].load(tw.rsB, p.ldb, tw.vrb, tw.kk(1, B_KC), tid);
    __builtin_amdgcn_sched_barrier(0);
    la[0].load(tw.rsA, p.lda, tw.vra, tw.kk(2, A_KC), tid);
    lb[0].load(tw.rsB, p.ldb, tw.vrb, tw.kk(2, B_KC), tid);
    __syncthreads();

    const int ar = wm * 64, br = wn * 64;
    // one k16 half of a step: 8 fragments, 12 MFMAs
    auto half_step = [&](const char *bufA, int s) {
      const char *bufB = bufA + 2 * A_PLANE;
      f16x8 a[2][2], bb[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
          a[i][pl] = LA::frag(bufA + pl * A_PLANE, ar + 32 * i, s, lane);
          bb[i][pl] = LB::frag(bufB + pl * B_PLANE, br + 32 * i, s, lane);
        }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          f32x16 x = acc[i][j];
          x = mfma(a[i][1], bb[j][0], x);  // lo hi
          x = mfma(a[i][0], bb[j][1], x);  // hi lo
          x = mfma(a[i][0], bb[j][0], x);  // hi hi
          acc[i][j] = x;
        }
    };
    // waves 4-7 split the next tile between their two MFMA halves, waves
    // 0-3 after both (gemm_x6_kernel's stagger)
    const bool late = wave < 4;
    // step t: tile t+1 is in set (t+1) & 1, which then takes tile t+3 (a
    // step past T issues its clamped loads too, so every path issues the
    // same loads and each split waits only for its own tile)
    auto step = [&](int t, LA &lan, LB &lbn) {
      if (t < tw.T) {
        const char *buf = lds + (t & 1) * BUF;
        char *nA = lds + ((t + 1) & 1) * BUF;
        const int kv = t + 2 == tw.T ? tw.klast : BK;
        half_step(buf, 0);
        if (!late && t + 1 < tw.T) {
          lan.template store<A_PLANE, RAG>(nA, tid, kv, m1);
          lbn.template store<B_PLANE, RAG>(nA + 2 * A_PLANE, tid, kv, m1);
        }
        half_step(buf, 1);
        if (late && t + 1 < tw.T) {
          lan.template store<A_PLANE, RAG>(nA, tid, kv, m1);
          lbn.template store<B_PLANE, RAG>(nA + 2 * A_PLANE, tid, kv, m1);
        }
      }
      lan.load(tw.rsA, p.lda, tw.vra, tw.kk(t + 3, A_KC), tid);
      lbn.load(tw.rsB, p.ldb, tw.vrb, tw.kk(t + 3, B_KC), tid);
      __syncthreads();
    };
    for (int t = 0; t < tw.T; t += 2) {
      step(t, la[1], lb[1]);
      step(t + 1, la[0], lb[0]);
    }
  }

  tile_epilogue<A_KC, B_KC, BN>(p, sexp, sw, acc, tw.split, tw.whole, tw.row0, tw.col0, flags, tid,
                                lds);
}

// ---------------------------------------------------------------------------
// gemm_f16x3_fast_kernel: gemm_f16x3_kernel's arithmetic (the same images,
// fragments and MFMA order into every accumulator: bitwise the same C) with
// one barrier per K step in its middle and the LDS traffic moved under the
// MFMAs.  K step t:
//   phase A: the 12 k16-half-0 MFMAs (fragments F0, read in the previous
//            phase B); beside them the split of tile t+1 into the other
//            buffer (one pair per MFMA) and the reads of the half-1
//            fragments F1;
//   barrier: tile t+1 written, buffer t & 1 read by every wave;
//   phase B: the 12 half-1 MFMAs; beside them the F0 reads of step t+1 (from
//            the other buffer) and the HBM loads of tile t+3.
// Each MFMA and the work placed after it are fenced (sched_barrier), so this
// is the issue order.  The bf16x6 kernel of this shape (cu-gemm-x6.hip
// gemm_x6_fast_kernel) measured no faster: its six products held the chip at
// its power limit.  f16x3's three leave the clock up, and the MFMA pipe idles
// on LDS latency instead (35-44 % busy at 2.1-2.3 GHz with the two-phase
// loop).
//
// The wide tile (BN_WIDE) has 24 MFMAs in a phase and 128 accumulator
// registers per lane, so it cannot hold two fragment sets and two loader
// sets.  A half's MFMAs go accumulator row by accumulator row, and only two
// rows' A fragments are held: row i + 1's are read beside row i's MFMAs, a
// phase's last row reads the next phase's first, and the four B fragments
// are re-read during the last row as each dies.  Reading a buffer in both of
// a step's phases needs a second barrier, at the step's end (one barrier per
// 24 MFMAs of a wave, the narrow tile's rate).  One loader set per operand:
// phase A splits tile t+1 out of it piece by piece, and each part
// (Loader::load_part) is loaded again with tile t+2 as soon as its last piece
// is split, a whole K step (48 MFMAs, the narrow tile's two) before that
// tile's split.
template <int AM, int BMODE, bool RAG, int BN = BN_NARROW>
__global__ __launch_bounds__(NT, 1) void gemm_f16x3_fast_kernel(GemmF16Args p) {
  constexpr bool A_KC = AM == LK, B_KC = BMODE == LK;
  constexpr int B_PLANE = Tile<BN>::B_PLANE, BUF = Tile<BN>::BUF, MI = Tile<BN>::MI;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  int *sexp = reinterpret_cast<int *>(lds + 2 * BUF);
  float *sw = reinterpret_cast<float *>(sexp + BM + BN);
  const int tid = threadIdx.x;
  const float m1 = kcnn::f16x3::opaque_m1();
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / Tile<BN>::WN, wn = wave % Tile<BN>::WN;
  TileWork<A_KC, B_KC, BN> tw(p);
  tw.bind(p);

  using LA = Loader<BM, AM>;
  using LB = Loader<BN, BMODE>;
  f32x16 acc[MI][2];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.0f;

  const int ar = wm * Tile<BN>::WR, br = wn * 64;
  // waves 4-7 (each SIMD's second wave) at priority 1 for the whole kernel
  // (MI355X_MICROARCH.md, two waves per SIMD, item 4: the younger half loses
  // every VALU arbitration otherwise)
  constexpr int PRIO = 1;
  if (PRIO && wave >= 4) __builtin_amdgcn_s_setprio(1);
  int flags = 0;
  if constexpr (BN == BN_WIDE) {
    LA la;
    LB lb;
    // two A rows and the four B fragments: row i's MFMAs run beside the reads
    // of row i + 1 into the other slot
    f16x8 fa[2][2], fb[2][2];
    // n-th MFMA of a half: accumulator (n / 6, (n / 3) % 2), lo.hi, hi.lo, hi.hi
    auto mfma_n = [&](int n) {
      const int i = n / 6, j = (n / 3) & 1, pr = n % 3;
      constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};
      acc[i][j] = mfma(fa[i & 1][PA[pr]], fb[j][PB[pr]], acc[i][j]);
    };
    // the fragment reads placed after MFMA n of the phase on half s of buf;
    // (nb, ns) is the next phase's buffer and half.  Row i's first two MFMAs
    // are followed by the reads of the next row (the next phase's row 0 after
    // the last) into the slot row i - 1 left; B's four are re-read for the
    // next phase during the last row, each after its last use (column block
    // 0's lo, hi, then block 1's), three MFMAs or more before its first
    auto reads_after = [&](int n, const char *buf, int s, const char *nb, int ns) {
      constexpr int L = 6 * MI;
      const int i = n / 6, r = (i + 1) % MI;
      const char *src = i + 1 < MI ? buf : nb;
      const int hs = i + 1 < MI ? s : ns;
      if (n % 6 == 0) fa[r & 1][1] = LA::frag(src + A_PLANE, ar + 32 * r, hs, lane);
      if (n % 6 == 1) fa[r & 1][0] = LA::frag(src, ar + 32 * r, hs, lane);
      if (n == L - 5) fb[0][1] = LB::frag(nb + 2 * A_PLANE + B_PLANE, br, ns, lane);
      if (n == L - 4) fb[0][0] = LB::frag(nb + 2 * A_PLANE, br, ns, lane);
      if (n == L - 2) fb[1][1] = LB::frag(nb + 2 * A_PLANE + B_PLANE, br + 32, ns, lane);
      if (n == L - 1) fb[1][0] = LB::frag(nb + 2 * A_PLANE, br + 32, ns, lane);
    };
    if (tw.T > 0) {
      la.load(tw.rsA, p.lda, tw.vra, tw.kk(0, A_KC), tid);
      lb.load(tw.rsB, p.ldb, tw.vrb, tw.kk(0, B_KC), tid);
    }
    __builtin_amdgcn_sched_barrier(0);
    flags = tile_scales<BN>(p, sexp, sw, tw.row0, tw.col0, tid);
    la.init_exp(sexp, tid);
    lb.init_exp(sexp + BM, tid);
    if (tw.T > 0) {
      la.template store<A_PLANE, RAG>(lds, tid, tw.T == 1 ? tw.klast : BK, m1);
      lb.template store<B_PLANE, RAG>(lds + 2 * A_PLANE, tid, tw.T == 1 ? tw.klast : BK, m1);
      __builtin_amdgcn_sched_barrier(0);
      la.load(tw.rsA, p.lda, tw.vra, tw.kk(1, A_KC), tid);
      lb.load(tw.rsB, p.ldb, tw.vrb, tw.kk(1, B_KC), tid);
      __syncthreads();
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) fa[0][pl] = LA::frag(lds + pl * A_PLANE, ar, 0, lane);
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
          fb[j][pl] = LB::frag(lds + 2 * A_PLANE + pl * B_PLANE, br + 32 * j, 0, lane);

      // step t: the loader set holds tile t+1 (split in phase A) and takes
      // tile t+2 part by part behind the split.  The last step does the same
      // with the clamped tile (a re-read of tile T-1, split into the buffer
      // no one reads again): one loop body, no peeled copy whose fragments
      // would have to live beside the loop's at the join
      auto step = [&](int t) {
        const char *buf = lds + (t & 1) * BUF;
        char *nbuf = lds + ((t + 1) & 1) * BUF;
        const int kv = t + 2 == tw.T ? tw.klast : BK;
        uint32_t ph[4], pl[4];
        // phase A
#pragma unroll
        for (int n = 0; n < 6 * MI; ++n) {
          mfma_n(n);
          if (n < LA::NPIECE) {
            la.template piece<A_PLANE, RAG>(nbuf, tid, n, kv, ph, pl, m1);
            if ((n + 1) % LA::PPP == 0)
              la.load_part(tw.rsA, p.lda, tw.vra, tw.kk(t + 2, A_KC), tid, n / LA::PPP);
          } else if (n - LA::NPIECE < LB::NPIECE) {
            const int m = n - LA::NPIECE;
            lb.template piece<B_PLANE, RAG>(nbuf + 2 * A_PLANE, tid, m, kv, ph, pl, m1);
            if ((m + 1) % LB::PPP == 0)
              lb.load_part(tw.rsB, p.ldb, tw.vrb, tw.kk(t + 2, B_KC), tid, m / LB::PPP);
          }
          reads_after(n, buf, 0, buf, 1);
          __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();  // tile t+1 written
        // phase B
#pragma unroll
        for (int n = 0; n < 6 * MI; ++n) {
          mfma_n(n);
          reads_after(n, buf, 1, nbuf, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();  // buffer t & 1 read by every wave: step t+1 writes it
      };
      static_assert(LA::NPIECE + LB::NPIECE <= 6 * MI, "a piece per MFMA of phase A");
#pragma unroll 1
      for (int t = 0; t < tw.T; ++t) step(t);
    }
  } else {
    LA la[2];
    LB lb[2];
    f16x8 fa0[2][2], fb0[2][2], fa1[2][2], fb1[2][2];
    // r-th fragment of half s: A fragments (i, plane) first, then B
    auto read_frag = [&](const char *buf, int s, int r, f16x8 (&fa)[2][2], f16x8 (&fb)[2][2]) {
      if (r < 4) {
        const int i = r >> 1, pl = r & 1;
        fa[i][pl] = LA::frag(buf + pl * A_PLANE, ar + 32 * i, s, lane);
      } else {
        const int i = (r - 4) >> 1, pl = (r - 4) & 1;
        fb[i][pl] = LB::frag(buf + 2 * A_PLANE + pl * B_PLANE, br + 32 * i, s, lane);
      }
    };
    // n-th MFMA of a half: accumulator (n / 6, (n / 3) % 2), lo.hi, hi.lo, hi.hi
    auto mfma_n = [&](int n, const f16x8 (&fa)[2][2], const f16x8 (&fb)[2][2]) {
      const int i = n / 6, j = (n / 3) & 1, pr = n % 3;
      constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};
      acc[i][j] = mfma(fa[i][PA[pr]], fb[j][PB[pr]], acc[i][j]);
    };

    // the first two K tiles' loads go out before the tile's scales are read
    // (the split needs both; the scales' loads and barriers then pass under
    // the tiles' latency: c2's data gradient 400 -> 381 us at K 1024 without
    // the scales at all)
    if (tw.T > 0) {
      la[0].load(tw.rsA, p.lda, tw.vra, tw.kk(0, A_KC), tid);
      lb[0].load(tw.rsB, p.ldb, tw.vrb, tw.kk(0, B_KC), tid);
      la[1].load(tw.rsA, p.lda, tw.vra, tw.kk(1, A_KC), tid);
      lb[1].load(tw.rsB, p.ldb, tw.vrb, tw.kk(1, B_KC), tid);
    }
    __builtin_amdgcn_sched_barrier(0);
    flags = tile_scales<BN>(p, sexp, sw, tw.row0, tw.col0, tid);
    la[0].init_exp(sexp, tid);
    la[1].init_exp(sexp, tid);
    lb[0].init_exp(sexp + BM, tid);
    lb[1].init_exp(sexp + BM, tid);
    if (tw.T > 0) {
      la[0].template store<A_PLANE, RAG>(lds, tid, tw.T == 1 ? tw.klast : BK, m1);
      lb[0].template store<B_PLANE, RAG>(lds + 2 * A_PLANE, tid, tw.T == 1 ? tw.klast : BK, m1);
      __builtin_amdgcn_sched_barrier(0);
      la[0].load(tw.rsA, p.lda, tw.vra, tw.kk(2, A_KC), tid);
      lb[0].load(tw.rsB, p.ldb, tw.vrb, tw.kk(2, B_KC), tid);
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 8; ++r) read_frag(lds, 0, r, fa0, fb0);

      // step t: tile t+1 is in set (t+1) & 1 (split in phase A), which then
      // takes tile t+3 (phase B; a step past T issues its clamped loads too)
      // (more_c: std::true_type where the step is known not to be the last,
      // so its split and next-fragment reads carry no branch; std::false_type
      // for the last step, which has neither)
      auto step = [&](int t, LA &lan, LB &lbn, auto more_c) {
        const char *buf = lds + (t & 1) * BUF;
        char *nbuf = lds + ((t + 1) & 1) * BUF;
        constexpr bool more = decltype(more_c)::value;
        const int kv = t + 2 == tw.T ? tw.klast : BK;
        uint32_t ph[4], pl[4];
        // phase A
#pragma unroll
        for (int n = 0; n < 12; ++n) {
          mfma_n(n, fa0, fb0);
          if (more) {
            if (n < LA::NPIECE)
              lan.template piece<A_PLANE, RAG>(nbuf, tid, n, kv, ph, pl, m1);
            else if (n - LA::NPIECE < LB::NPIECE)
              lbn.template piece<B_PLANE, RAG>(nbuf + 2 * A_PLANE, tid, n - LA::NPIECE, kv, ph, pl, m1);
          }
          if (n >= 2 && n < 10) read_frag(buf, 1, n - 2, fa1, fb1);
          __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        // phase B
#pragma unroll
        for (int n = 0; n < 12; ++n) {
          mfma_n(n, fa1, fb1);
          if (n == 1) lan.load(tw.rsA, p.lda, tw.vra, tw.kk(t + 3, A_KC), tid);
          if (n == 3) lbn.load(tw.rsB, p.ldb, tw.vrb, tw.kk(t + 3, B_KC), tid);
          if (more && n >= 2 && n < 10) read_frag(nbuf, 0, n - 2, fa0, fb0);
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      int t = 0;
      // every step of the loop has a successor; the last one or two after it
      for (; t + 2 < tw.T; t += 2) {
        step(t, la[1], lb[1], std::true_type{});
        step(t + 1, la[0], lb[0], std::true_type{});
      }
      if (t + 1 < tw.T) {
        step(t, la[1], lb[1], std::true_type{});
        step(t + 1, la[0], lb[0], std::false_type{});
      } else {
        step(t, la[1], lb[1], std::false_type{});
      }
    }
  }

  tile_epilogue<A_KC, B_KC, BN>(p, sexp, sw, acc, tw.split, tw.whole, tw.row0, tw.col0, flags, tid,
                                lds);
}

// The plan of a call: the tile, the split-K count and the whole tiles in
// front of the split ones (block_tile), of least modelled time.  Per tile:
// the whole tiles in nwhole / 256 rounds of one workgroup per CU, the split
// ones in ceil((tiles - nwhole) s / 256) rounds, a round of k steps
// a k + b us (b: the tile prologue and epilogue), and for s > 1 the
// reduce's (s + 1) fp32 reads and writes of the split tiles' share of M N
// at 4 TB/s.  Narrow tile: 0.0458 k + 11.1, fitted to c2's three FC GEMMs on
// MI355X.  (The reduce was unpriced before r06: nnet.config's 4096 x 3454
// x 4096 layers took 4 splits and an 86-92 us reduce, one split being 2.4 %
// faster per step; c2's 364-tile weight gradient split all its tiles in 2.84
// rounds, where 256 whole tiles and 108 split ones take 1 + 0.84.)
// Wide tile: 0.0793 k + 21.4, fitted on MI355X to 4096 x 4096 x K calls (256
// wide tiles, one round; 512 narrow ones, two) at K = 1024, 2016 and 4096
// with each tile forced: 120.9 / 209.0 / 412.6 us wide against 134.3 / 235.1 /
// 463.7 narrow, the narrow times less the narrow model being the statistics
// launches both share (profiles/gemm_tiles.md, which also has c2's three
// GEMMs: forward 353 -> 329 us, data gradient 377 -> 344, both as the model
// picks; the weight gradient's 184 wide tiles measured 380 against the narrow
// hybrid's 411, which the model, 346 against 314, does not see: it prices a
// round of 184 workgroups as one of 256).
// A pure function of the call's shape: no timing or history enters it.
struct GemmPlan {
  int bn, ksplit, nwhole;
  double us;
};
constexpr double NARROW_A = 0.0458, NARROW_B = 11.1;
constexpr double WIDE_A = 0.0793, WIDE_B = 21.4;
GemmPlan plan_tile(int bn, int M, int N, int K) {
  const int64_t tiles = (int64_t)((M + BM - 1) / BM) * ((N + bn - 1) / bn);
  const double ca = bn == BN_WIDE ? WIDE_A : NARROW_A, cb = bn == BN_WIDE ? WIDE_B : NARROW_B;
  auto round = [&](int k) { return ca * k + cb; };
  GemmPlan best{bn, 1, 0, (double)((tiles + 255) / 256) * round(K)};
  for (int s = 2; s <= 4 && K / s >= 1024; ++s) {
    const int ks = (K + s - 1) / s;
    for (int64_t w = 0; w < tiles; w += 256) {
      const int64_t rest = tiles - w;
      const double t = (double)(w / 256) * round(K) + (double)((rest * s + 255) / 256) * round(ks) +
                       (double)(s + 1) * M * N * 4.0 / 4.0e6 * (double)rest / (double)tiles;
      if (t < best.us) best = GemmPlan{bn, s, (int)w, t};
    }
  }
  return best;
}
// family: the "gemm" selector (kcnn-knobs.h): 3 the wide tile wherever the
// call can take it (wide_ok: no LR operand), 4 the narrow tile, else the model
GemmPlan choose_plan(int M, int N, int K, bool wide_ok, int family) {
  const GemmPlan narrow = plan_tile(BN_NARROW, M, N, K);
  if (!wide_ok || family == 4) return narrow;
  const GemmPlan wide = plan_tile(BN_WIDE, M, N, K);
  if (family == 3) return wide;
  return wide.us < narrow.us ? wide : narrow;
}
// an operand's loader: K-contiguous, or row-contiguous with 16-B loads along
// its rows when they are aligned (pitch % 4 == 0: a quad that starts inside
// the row count M or N ends inside the pitch; its values past the count feed
// only C rows or columns that are not stored, and the kernel's descriptors
// end at the last row's padded quad), else one dword per lane
int loader_mode(bool kc, const void *ptr, int ld) {
  if (kc) return (int)LK;
  return ld % 4 == 0 && (uintptr_t)ptr % 16 == 0 ? (int)LT : (int)LR;
}
std::atomic<unsigned long long> g_tile_calls[2];  // launches on the narrow, the wide tile

// the one-barrier fast kernel where no operand is LR (an LR operand's 16
// loaded values per thread and K step spill there), on the plan's tile, else
// the two-phase kernel on the narrow tile (bitwise the same C)
template <int AM, int BMODE, bool RAG>
void launch_t(const GemmF16Args &a, unsigned blocks, hipStream_t st) {
  using kcnn::launch_lds;
  constexpr int NARROW_LDS = Tile<BN_NARROW>::LDS_BYTES, WIDE_LDS = Tile<BN_WIDE>::LDS_BYTES;
  if constexpr (AM != LR && BMODE != LR) {
    if (a.bn == BN_WIDE)
      launch_lds<&gemm_f16x3_fast_kernel<AM, BMODE, RAG, BN_WIDE>, WIDE_LDS>(a, blocks, NT, st);
    else
      launch_lds<&gemm_f16x3_fast_kernel<AM, BMODE, RAG, BN_NARROW>, NARROW_LDS>(a, blocks, NT, st);
  } else {
    launch_lds<&gemm_f16x3_kernel<AM, BMODE, RAG>, NARROW_LDS>(a, blocks, NT, st);
  }
}
template <bool RAG>
void launch_r(int am, int bm, const GemmF16Args &a, unsigned blocks, hipStream_t st) {
  // am: LK or a row-contiguous mode; bm likewise
  if (am == LK && bm == LK) launch_t<LK, LK, RAG>(a, blocks, st);
  else if (am == LK && bm == LT) launch_t<LK, LT, RAG>(a, blocks, st);
  else if (am == LK) launch_t<LK, LR, RAG>(a, blocks, st);
  else if (am == LT && bm == LK) launch_t<LT, LK, RAG>(a, blocks, st);
  else if (am == LT && bm == LT) launch_t<LT, LT, RAG>(a, blocks, st);
  else if (am == LT) launch_t<LT, LR, RAG>(a, blocks, st);
  else if (bm == LK) launch_t<LR, LK, RAG>(a, blocks, st);
  else if (bm == LT) launch_t<LR, LT, RAG>(a, blocks, st);
  else launch_t<LR, LR, RAG>(a, blocks, st);
}
void launch(int am, int bm, const GemmF16Args &a, unsigned blocks, hipStream_t st) {
  if (a.K % BK) launch_r<true>(am, bm, a, blocks, st);
  else launch_r<false>(am, bm, a, blocks, st);
}

// (of the larger split count of the two tiles' plans: the workspace is sized
// before the operands' alignment and the selector's value at the call are known)
size_t partial_bytes(int M, int N, int K) {
  const int s = std::max(plan_tile(BN_NARROW, M, N, K).ksplit, plan_tile(BN_WIDE, M, N, K).ksplit);
  return s > 1 ? slab_bytes(s, M, N) + flag_bytes(M, N) : 0;
}

}  // namespace

extern "C" size_t kl_gemm_f16x3_workspace_bytes(int M, int N, int K) {
  return partial_bytes(M, N, K);
}
// f16x3 launches on the narrow tile (out[0]) and on the wide tile (out[1])
// since the last reset
extern "C" void kl_gemm_f16x3_tile_counts(unsigned long long *out, int reset) {
  for (int i = 0; i < 2; ++i) {
    out[i] = g_tile_calls[i].load(std::memory_order_relaxed);
    if (reset) g_tile_calls[i].store(0, std::memory_order_relaxed);
  }
}
// The plan of a call under the current "gemm" selector, without a GPU:
// out = {the tile's columns, ksplit, nwhole}; operand bases taken as 16-B
// aligned, a workspace of kl_gemm_f16x3_workspace_bytes given.  Returns the
// plan's workspace need (0 for one split).
extern "C" size_t kl_gemm_f16x3_plan(int transA, int transB, int M, int N, int K, int lda,
                                     int ldb, int *out) {
  out[0] = out[1] = out[2] = 0;
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  const int am = loader_mode(!transA, nullptr, lda), bm = loader_mode(transB != 0, nullptr, ldb);
  const GemmPlan plan = choose_plan(M, N, K, am != LR && bm != LR, kcnn::family(kcnn::kFamGemm));
  out[0] = plan.bn;
  out[1] = plan.ksplit;
  out[2] = plan.ksplit > 1 ? plan.nwhole : 0;
  return plan.ksplit > 1 ? slab_bytes(plan.ksplit, M, N) + flag_bytes(M, N) : 0;
}
namespace {

// One call, as its extern "C" entry fills it:
// C[M x N] = alpha * op(A) op(B) + beta * C (+ bias[col] on every row), or
// with mom.W the product applied as the momentum update instead of stored.
struct GemmCall {
  int transA, transB, M, N, K;
  float alpha, beta;
  const float *A, *B;
  float *C;
  int lda, ldb, ldc;
  // the statistics blocks [max[n], min[n], cnt[n]] of op(A)'s rows and op(B)'s
  // columns (kl_absmax_rows / kl_absmax_cols); nullable where the entry takes
  // them from the caller: gemm_stats computes the missing ones
  const uint32_t *amax, *bmax;
  const float *bias;  // nullable
  void *ws;           // kl_gemm_f16x3_full_workspace_bytes; after gemm_stats the split-K part
  size_t ws_bytes;
  kcnn_stream_t stream;
  MomentumEpi mom;
};

size_t stats_ws_words(int M, int N, int K, int transA, int transB) {
  const size_t pa = transA ? stat_part_words(K, M, 1) : 0;
  const size_t pb = transB ? 0 : stat_part_words(K, N, 1);
  return 3 * ((size_t)M + N) + 4 + pa + pb;
}

// The shape and workspace checks, then the operand statistics the caller did
// not supply (op(A)'s rows: A's rows, or its columns when transposed; op(B)'s
// columns: B's columns, or its rows when transposed; one read of that
// operand), one launch for both (two with a per-column one), into the
// workspace after the partial slabs.
int gemm_stats(GemmCall &c) {
  const int M = c.M, N = c.N, K = c.K;
  if (M < 0 || N < 0 || K < 0) return (int)hipErrorInvalidValue;
  if (M == 0 || N == 0 || K == 0) return (int)hipErrorNotSupported;
  const size_t pb = partial_bytes(M, N, K);
  if (!c.ws || c.ws_bytes < kl_gemm_f16x3_full_workspace_bytes(M, N, K))
    return (int)hipErrorInvalidValue;
  uint32_t *amax = reinterpret_cast<uint32_t *>(static_cast<char *>(c.ws) + pb);
  uint32_t *bmax = amax + 3 * (size_t)M;  // statistics blocks: [max, min, cnt] per group
  uint32_t *parta = bmax + 3 * (size_t)N + 4;
  uint32_t *partb = parta + (c.transA ? stat_part_words(K, M, 1) : 0);
  const StatOp sa = c.amax     ? StatOp{}
                    : c.transA ? stat_op(c.A, K, M, c.lda, 1, amax, parta)
                               : stat_op(c.A, M, K, c.lda, 0, amax, nullptr);
  const StatOp sb = c.bmax     ? StatOp{}
                    : c.transB ? stat_op(c.B, N, K, c.ldb, 0, bmax, nullptr)
                               : stat_op(c.B, K, N, c.ldb, 1, bmax, partb);
  if (!c.amax || !c.bmax) {
    const int rc = c.amax ? stats_launch(sb, StatOp{}, kcnn::as_stream(c.stream))
                          : stats_launch(sa, sb, kcnn::as_stream(c.stream));
    if (rc) return rc;
  }
  if (!c.amax) c.amax = amax;
  if (!c.bmax) c.bmax = bmax;
  c.ws = pb ? c.ws : nullptr;
  c.ws_bytes = pb;
  return 0;
}

// The call's plan and its launches, the statistics given.  Needs 16-B
// aligned K-contiguous operands (A untransposed, B transposed) with pitches
// % 4 == 0 and every workgroup's buffer offsets below 2^31; returns
// hipErrorNotSupported otherwise (the caller uses kl_gemm_x6).
int gemm_launch(const GemmCall &c) {
  const int M = c.M, N = c.N, K = c.K;
  const bool a_kc = !c.transA, b_kc = c.transB != 0;
  if ((a_kc && (c.lda % 4 || (uintptr_t)c.A % 16)) || (b_kc && (c.ldb % 4 || (uintptr_t)c.B % 16)))
    return (int)hipErrorNotSupported;
  hipStream_t st = kcnn::as_stream(c.stream);
  GemmF16Args a{};
  a.A = c.A; a.B = c.B; a.C = c.C; a.amax = c.amax; a.bmax = c.bmax; a.bias = c.bias;
  a.mom = c.mom;
  // statistics blocks [max[n], min[n], cnt[n]] (stats_rows, stats_finalize_kernel)
  a.amin = a.amax + M;
  a.acnt = a.amax + 2 * (size_t)M;
  a.bmin = a.bmax + N;
  a.bcnt = a.bmax + 2 * (size_t)N;
  a.bvec = N % 4 == 0 && (uintptr_t)a.bmax % 16 == 0 && (uintptr_t)a.bcnt % 16 == 0;
  a.M = M; a.N = N; a.K = K; a.lda = c.lda; a.ldb = c.ldb; a.ldc = c.ldc;
  a.alpha = c.alpha; a.beta = c.beta;
  const int am = loader_mode(a_kc, c.A, c.lda), bm = loader_mode(b_kc, c.B, c.ldb);
  const GemmPlan plan =
      choose_plan(M, N, K, am != LR && bm != LR, kcnn::family(kcnn::kFamGemm));
  const int BN = plan.bn;
  a.bn = BN;
  a.tiles_m = (M + BM - 1) / BM;
  a.tiles_n = (N + BN - 1) / BN;
  const int64_t tiles = (int64_t)a.tiles_m * a.tiles_n;
  int nwhole = plan.nwhole;
  int s = plan.ksplit;
  const size_t need = s > 1 ? slab_bytes(s, M, N) + flag_bytes(M, N) : 0;
  if (need > c.ws_bytes || !c.ws) s = 1;
  if (s > 1) {
    a.part = static_cast<float *>(c.ws);
    a.rflag = reinterpret_cast<uint32_t *>(static_cast<char *>(c.ws) + slab_bytes(s, M, N));
    static std::atomic<uint32_t> calls{0};
    a.gen = ++calls;
    if (a.gen == 0) a.gen = ++calls;
  }
  a.ksplit = s;
  a.kps = ((K + s - 1) / s + BK - 1) / BK * BK;
  // every offset a workgroup forms (rows of its tile, k up to its K span +
  // 2 BK) < 2^31
  auto fits = [&](bool kc, int ld, int R, int span) {
    if (kc) return (int64_t)R * ld * 4 + (int64_t)(K + 2 * BK) * 4 < ((int64_t)1 << 31);
    return (int64_t)(span + 2 * BK) * ld * 4 + (int64_t)R * 4 < ((int64_t)1 << 31);
  };
  if (!fits(a_kc, c.lda, BM, a.kps) || !fits(b_kc, c.ldb, BN, a.kps))
    return (int)hipErrorNotSupported;
  if (s == 1 || !fits(a_kc, c.lda, BM, K) || !fits(b_kc, c.ldb, BN, K)) nwhole = 0;
  a.nwhole = nwhole;
  const int64_t nb = nwhole + (tiles - nwhole) * s;
  if (nb >= ((int64_t)1 << 31)) return (int)hipErrorNotSupported;
  // (the site's word is read and cleared before anything of the call is enqueued)
  const FixupSite site = s > 1 ? split_k_site(a, a_kc, b_kc) : FixupSite{};
  launch(am, bm, a, (unsigned)nb, st);
  const int rc = kcnn::launch_status();
  if (!rc) g_tile_calls[BN == BN_WIDE ? 1 : 0].fetch_add(1, std::memory_order_relaxed);
  if (rc || s == 1) return rc;
  return split_k_finish(a, a_kc, b_kc, site, st);
}

int gemm_run(GemmCall c) {
  const int rc = gemm_stats(c);
  return rc ? rc : gemm_launch(c);
}

}  // namespace

extern "C" size_t kl_gemm_f16x3_full_workspace_bytes(int M, int N, int K) {
  size_t w = 0;
  for (int ta = 0; ta < 2; ++ta)
    for (int tb = 0; tb < 2; ++tb) w = std::max(w, stats_ws_words(M, N, K, ta, tb));
  return partial_bytes(M, N, K) + align16(sizeof(uint32_t) * w);
}
// The operand statistics computed here, in the workspace
extern "C" int kl_gemm_f16x3(int transA, int transB, int M, int N, int K, float alpha,
                             const float *A, int lda, const float *B, int ldb, float beta,
                             float *C, int ldc, void *ws, size_t ws_bytes,
                             kcnn_stream_t stream) {
  return gemm_run({transA, transB, M, N, K, alpha, beta, A, B, C, lda, ldb, ldc, nullptr, nullptr,
                   nullptr, ws, ws_bytes, stream, {}});
}
// ... with either operand's statistics supplied by its producer (nullable:
// only the missing ones are computed), and C += bias[col] on every row (bias
// nullable), in the same store: the FC forward's out = bias; out += in W^T
// without the bias copy or C's re-read
extern "C" int kl_gemm_f16x3_bias(int transA, int transB, int M, int N, int K, float alpha,
                                  const float *A, int lda, const float *B, int ldb, float beta,
                                  float *C, int ldc, const uint32_t *amax_given,
                                  const uint32_t *bmax_given, const float *bias, void *ws,
                                  size_t ws_bytes, kcnn_stream_t stream) {
  return gemm_run({transA, transB, M, N, K, alpha, beta, A, B, C, lda, ldb, ldc, amax_given,
                   bmax_given, bias, ws, ws_bytes, stream, {}});
}
// The weight-gradient product applied as the momentum update in its own
// store (momentum-step.h): for every element g = (op(A) op(B))[i][j],
// prev = momentum prev + a_wd W + a_g g, W += prev, the bits of
// kl_gemm_f16x3_bias(alpha 1, beta 0, a null bias) into a gradient buffer
// followed by hipF_momentum_update, without the buffer's write and read.  W
// and prev are M x N with 16-B aligned rows (hipErrorNotSupported otherwise).
extern "C" int kl_gemm_f16x3_momentum(int transA, int transB, int M, int N, int K,
                                      const float *A, int lda, const float *B, int ldb,
                                      const uint32_t *amax_given, const uint32_t *bmax_given,
                                      float *W, int ldw, float *prev, int ldp, float momentum,
                                      float a_wd, float a_g, void *ws, size_t ws_bytes,
                                      kcnn_stream_t stream) {
  if (!W || !prev || ldw % 4 || ldp % 4 || (uintptr_t)W % 16 || (uintptr_t)prev % 16)
    return (int)hipErrorNotSupported;
  return gemm_run({transA, transB, M, N, K, 1.0f, 0.0f, A, B, nullptr, lda, ldb, ldw, amax_given,
                   bmax_given, nullptr, ws, ws_bytes, stream,
                   {W, prev, ldw, ldp, momentum, a_wd, a_g}});
}
