// cnslmat/conv-geom.h -- geometry shared by the convolution kernels.
#ifndef KCNN_CNSLMAT_CONV_GEOM_H_
#define KCNN_CNSLMAT_CONV_GEOM_H_

#include "hip-util.h"
#include "pool-stats.h"

namespace kcnn {

typedef float floatx16 __attribute__((ext_vector_type(16)));

// One convolution instance: R rows (frames) of H x W x C maps (column
// h + w*H + c*H*W), virtual zero padding (pad_h, pad_w), kernel kh x kw,
// G output maps of oh x ow (p = px*oh + py).
struct ConvGeom {
  int R, H, W, C, pad_h, pad_w, kh, kw, G, oh, ow, P, Kdim, HW;
  int Gtot;   // the layer's filter count (G is one chunk's when a launch splits G)
  int64_t M;  // R * P
  FastDiv div_P, div_oh, div_khkw, div_kh, div_H, div_HW;
};

inline ConvGeom make_geom(int R, int H, int W, int C, int pad_h, int pad_w,
                          int kh, int kw, int G) {
  ConvGeom g;
  g.R = R; g.H = H; g.W = W; g.C = C; g.pad_h = pad_h; g.pad_w = pad_w;
  g.kh = kh; g.kw = kw; g.G = G; g.Gtot = G;
  g.oh = H + 2 * pad_h - kh + 1;
  g.ow = W + 2 * pad_w - kw + 1;
  g.P = g.oh * g.ow;
  g.Kdim = kh * kw * C;
  g.HW = H * W;
  g.M = (int64_t)R * g.P;
  g.div_P = FastDiv((uint32_t)(g.P > 0 ? g.P : 1));
  g.div_oh = FastDiv((uint32_t)(g.oh > 0 ? g.oh : 1));
  g.div_khkw = FastDiv((uint32_t)(kh * kw > 0 ? kh * kw : 1));
  g.div_kh = FastDiv((uint32_t)(kh > 0 ? kh : 1));
  g.div_H = FastDiv((uint32_t)(H > 0 ? H : 1));
  g.div_HW = FastDiv((uint32_t)(g.HW > 0 ? g.HW : 1));
  return g;
}

// ---- Route predicates.  Each limit is written once, here or beside its
// kernel, and read by the workspace sizers, the launchers and the routes of
// conv-dispatch.cc alike.

// The frame forward kernels' range (kcnn_conv_fwd_frame; cnsl-conv-frame.hip).
inline bool in_frame_range(const ConvGeom &g) { return g.Kdim <= 64 && g.P >= 16; }

// The small-filter direct kernel's shapes (kcnn_conv_direct): an MFMA tile
// would be >= 80 % padding there.
inline bool use_direct(const ConvGeom &g, int concat) { return concat && g.G <= 8; }

// A fused forward (conv + ReLU, conv + 3-D pool in the implicit GEMM's
// epilogue) must give the bits of the unfused convolution, so it runs only
// where the unfused route is that same implicit GEMM: not in the frame
// kernels' range (even where those then decline) and not on the direct
// kernel's shapes.  Elsewhere the fused entry point declines and the caller
// runs the components unfused.
inline bool unfused_is_igemm(const ConvGeom &g, int concat) {
  return !in_frame_range(g) && !use_direct(g, concat);
}

// One filter chunk of the fused backward (fp32 DMA, register-staged and
// bf16x6 kernels): Kdim <= 31 (row Kdim is the bias gradient) and whole
// 32-filter slabs, at most four.
inline bool bwd_chunk_shape_ok(const ConvGeom &g) {
  return g.Kdim <= 31 && g.G % 32 == 0 && g.G <= 128 && g.G != 0;
}

// MFMA 32x32 accumulator register r of lane l holds row
// (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31.
__device__ __forceinline__ int mfma32_row(int r, int lane) {
  return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}

}  // namespace kcnn

struct ConvUpdateEpi;  // conv-update.h

// Frame-resident kernels.  Each returns -1 when the shape is not eligible
// (caller falls back to the implicit-GEMM path).
// The forward, alone or with the max pool behind it (cnsl-conv-frame.hip).
int kcnn_conv_fwd_frame(const kcnn::ConvGeom &g, const float *X, int xs,
                        const float *K, int ks, const float *bias, float *out,
                        int os, hipStream_t st);
// the pooled output's statistics: pool-stats.h
size_t kcnn_pool_stats_partial_words(const kcnn::ConvGeom &g, int pc);
int kcnn_conv_fwd_frame_pool(const kcnn::ConvGeom &g, const float *X, int xs,
                             const float *K, int ks, const float *bias,
                             float *out, int os, float *pool, int ps,
                             unsigned char *mask, int ms, int pc,
                             hipStream_t st, int ph = 1, int pw = 1,
                             PoolStatsOut *stats = nullptr);
// The fp32 backward (cnsl-conv-frame-bwd.hip): the data gradient, the weight
// gradient (ws of kcnn_conv_wgrad_frame_ws(g) bytes, 0 = not eligible) ...
int kcnn_conv_dgrad_frame(const kcnn::ConvGeom &g, const float *dY, int dys,
                          const float *K, int ks, float *dX, int dxs,
                          hipStream_t st);
size_t kcnn_conv_wgrad_frame_ws(const kcnn::ConvGeom &g);
int kcnn_conv_wgrad_frame(const kcnn::ConvGeom &g, const float *X, int xs,
                          const float *dY, int dys, float *gW, int gws,
                          float *gb, void *ws, size_t ws_bytes, hipStream_t st);
// ... and the fused backward (one pass over dY): dX (nullable) and gW/gb.
// ws must hold kcnn_conv_bwd_frame_ws(g) bytes (0 = shape not eligible).
size_t kcnn_conv_bwd_frame_ws(const kcnn::ConvGeom &g);
// pc > 0: dY / dys are instead the derivative of a ph x 1 x pc Maxpool over
// Y and pmask / pms its routing mask (hipF_conv2d_maxpool[3d]: 1 byte per
// pooled value when ph == 1, else 2; pms in bytes); dY is built per slab in
// LDS and never stored.  ph > 1 runs on the bf16x6 kernel only.
int kcnn_conv_bwd_frame(const kcnn::ConvGeom &g, const float *X, int xs,
                        const float *dY, int dys, const float *K, int ks,
                        float *dX, int dxs, float *gW, int gws, float *gb,
                        void *ws, size_t ws_bytes, hipStream_t st,
                        const unsigned char *pmask = nullptr, int pms = 0,
                        int pc = 0, int ph = 1);
// The same fused backward on the bf16 MFMAs with exact three-way operand
// splits (cnsl-conv-x6.hip); ws_part == NULL runs the data gradient only,
// part_acc adds to ws_part what an earlier frame range left there.
bool kcnn_conv_bwd_x6_eligible(const kcnn::ConvGeom &g, bool dx, int pc, int ph = 1);
int kcnn_conv_bwd_x6(const kcnn::ConvGeom &g, const float *X, int xs, const float *dY,
                     int dys, const float *K, int ks, float *dX, int dxs, float *ws_part,
                     int S, int dx_acc, hipStream_t st, const unsigned char *pmask,
                     int pms, int pc, int ph, bool part_acc = false);
// Conv2D(concat) + bias (+ ReLU when relu) as an implicit GEMM on the f16
// (f16x3, igemm_x6 family 2 / 3) or bf16 (bf16x6) MFMAs
// (cnsl-conv-igemm-x6.hip); -1 when the shape is outside its limits.
int kcnn_conv_igemm_x6(const kcnn::ConvGeom &g, const float *X, int xs, const float *K,
                       int ks, const float *bias, float *out, int os, int relu,
                       hipStream_t st);
// kcnn_conv_igemm_x6 with a ph x pw x pc Maxpool of two-position windows in
// its epilogue (pooled output and 16-bit routing mask); -1 when not covered.
int kcnn_conv_igemm_x6_pool(const kcnn::ConvGeom &g, const float *X, int xs, const float *K,
                            int ks, const float *bias, float *out, int os, float *pool,
                            int ps, unsigned short *mask, int ms, int ph, int pw, int pc,
                            hipStream_t st);
// Weight gradient on the bf16 MFMAs (cnsl-conv-igemm-x6.hip): the split
// plan (false = not eligible), then partials [S][G*Kdim + G] into ws for
// kcnn_reduce_splits_wgrad.
bool kcnn_conv_wgrad_x6_plan(const kcnn::ConvGeom &g, int xs, int dys, int &S, int &fps,
                             size_t &ws_bytes);
int kcnn_conv_wgrad_x6(const kcnn::ConvGeom &g, const float *X, int xs, const float *dY,
                       int dys, float *ws, int S, int fps, hipStream_t st);

// The split reduction (cnsl-conv-reduce.hip): deterministic column sums of a
// [S x E] fp32 slab of workgroup partials, sum[e] = sum_s in[s][e], in one
// pass (reduce_splits_kernel): a block takes 64 columns, its four waves sum
// interleaved rows and their sums are added in a fixed order.  e < nw goes
// to gW[row][col], (row, col) = gk_layout ? (e % inner, e / inner) :
// (e / inner, e % inner), and e >= nw to gb[e - nw]; with u.W set
// (conv-update.h) the sums step W / prev / b instead.
int kcnn_reduce_splits_epi(const float *in, int S, int E, int nw, int inner, int gk_layout,
                           float *gW, int gws, float *gb, const ConvUpdateEpi &u,
                           hipStream_t st);
// the implicit-GEMM wgrad layout (gk_layout 1: e = g*inner + k -> gW[k][g])
// under the current thread's update request, marked applied when taken
int kcnn_reduce_splits_wgrad(const float *in, int S, int E, int nw, int inner, float *gW,
                             int gws, float *gb, hipStream_t st);
// The bytes callers reserve behind their partials, and the first pass of the
// implicit-GEMM v1 split-K reduction (groups of 32 rows into tmp
// [ceil(S/32) x E]; conv_splitk_reduce_kernel adds the groups).
size_t kcnn_reduce_splits_ws(int S, int E);
int kcnn_reduce_splits_pass1(const float *in, int S, int E, float *tmp,
                             hipStream_t st);

// The fp32-MFMA family (cnsl-conv-mfma.hip), same contract as the launchers
// above: 0 launched, -1 declined with nothing launched, > 0 a HIP error.
// Small filter counts (use_direct), one thread per output position.
int kcnn_conv_direct(const kcnn::ConvGeom &g, int concat, const float *X, int xs,
                     const float *K, int ks, const float *bias, float *out, int os,
                     hipStream_t st);
// conv_igemm2_kernel: Conv2D(concat) + bias (+ ReLU); declines operands past
// 32-bit byte offsets, unaligned K and padded maps of more than 32 taps.
int kcnn_conv_igemm2(const kcnn::ConvGeom &g, const float *X, int xs, const float *K, int ks,
                     const float *bias, float *out, int os, int relu, hipStream_t st);
// conv_igemm_kernel, either output layout, split over K with a fixed-order
// reduction when ws holds kcnn_conv_igemm_ws(g) bytes; never declines.
size_t kcnn_conv_igemm_ws(const kcnn::ConvGeom &g);
int kcnn_conv_igemm(const kcnn::ConvGeom &g, const float *X, int xs, const float *K, int ks,
                    const float *bias, float *out, int os, int concat, void *ws,
                    size_t ws_bytes, hipStream_t st);
// conv_wgrad2_kernel (G >= 32, Kdim >= 32, P <= 96) and its reduction;
// kcnn_conv_wgrad2_ws is 0 outside its plan.
size_t kcnn_conv_wgrad2_ws(const kcnn::ConvGeom &g, int xs, int dys);
int kcnn_conv_wgrad2(const kcnn::ConvGeom &g, const float *X, int xs, const float *dY,
                     int dys, float *gW, int gws, float *gb, void *ws, size_t ws_bytes,
                     hipStream_t st);
// conv_wgrad_kernel and its reduction: every geometry; a workspace under
// kcnn_conv_wgrad_ws(g) is hipErrorInvalidValue, never -1.
size_t kcnn_conv_wgrad_ws(const kcnn::ConvGeom &g);
int kcnn_conv_wgrad(const kcnn::ConvGeom &g, const float *X, int xs, const float *dY,
                    int dys, float *gW, int gws, float *gb, void *ws, size_t ws_bytes,
                    hipStream_t st);
// The scatter data gradient (Kdim >= 32, G >= 16, HW >= 1.25 P): 0 bytes and
// -1 outside its shapes, -1 too when ws is short.
size_t kcnn_conv_dgrad_scatter_ws(const kcnn::ConvGeom &g);
int kcnn_conv_dgrad_scatter(const kcnn::ConvGeom &g, const float *dY, int dys,
                            const float *W, int ks, float *dX, int dxs, void *ws,
                            size_t ws_bytes, hipStream_t st);

#endif  // KCNN_CNSLMAT_CONV_GEOM_H_
