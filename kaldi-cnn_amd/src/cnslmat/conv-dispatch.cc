// cnslmat/conv-dispatch.cc -- which kernels serve a convolution.
//
// Every hipF_conv2d* entry point of the C shim (include/cnsl-hip-kernels.h)
// and its workspace sizer: the arguments are checked once (conv_args), then
// the geometry walks a ladder of routes.  A route is one call into a kernel
// family's launcher (conv-geom.h): 0 launched, -1 declined with nothing
// launched, > 0 a HIP error.  The limits a route depends on are predicates of
// conv-geom.h or of the family's own file, each written once.  Host code
// only; the kernels are in cnsl-conv-frame.hip (frame-resident forward),
// cnsl-conv-frame-bwd.hip (frame-resident fp32 backward), cnsl-conv-x6.hip
// (bf16x6 fused backward), cnsl-conv-igemm-x6.hip (bf16x6 / f16x3 implicit
// GEMM and weight gradient), cnsl-conv-mfma.hip (fp32 MFMA, direct) and
// cnsl-conv-reduce.hip (the weight gradients' split reduction).
// profiles/conv_dispatch.md has the ladders as tables.
#include <stdint.h>

#include <algorithm>

#include "conv-geom.h"

using kcnn::ConvGeom;
using kcnn::as_stream;
using kcnn::make_geom;
using kcnn::use_direct;

namespace {

constexpr int kInvalid = (int)hipErrorInvalidValue;

// The map and kernel sizes every entry point takes.
struct ConvShape {
  int H, W, C, pad_h, pad_w, kh, kw, G;
};

// The matrices an entry point was given (NULL: none of that kind), in this
// order; conv_args checks each present one against the geometry.
struct ConvMats {
  const MatrixDim *in;         // X [R x H*W*C]: its columns
  const MatrixDim *kernel;     // W [Kdim x G]
  const MatrixDim *grad_W;     // gW [Kdim x G]
  const MatrixDim *out;        // Y or dY, concat layout [R x P*G]
  const MatrixDim *out_plain;  // Y, plain layout [R*P x G]
  const MatrixDim *in_deriv;   // dX [R x H*W*C], and pad <= kernel - 1
};

// The geometry of `rows` frames of shape s into g; hipErrorInvalidValue when
// the output map is empty or a present matrix does not fit it, else 0.
int conv_args(int rows, const ConvShape &s, const ConvMats &m, ConvGeom &g) {
  g = make_geom(rows, s.H, s.W, s.C, s.pad_h, s.pad_w, s.kh, s.kw, s.G);
  const bool ok =
      g.oh > 0 && g.ow > 0 && (!m.in || m.in->cols == g.HW * s.C) &&
      (!m.kernel || (m.kernel->rows == g.Kdim && m.kernel->cols == s.G)) &&
      (!m.grad_W || (m.grad_W->rows == g.Kdim && m.grad_W->cols == s.G)) &&
      (!m.out || (m.out->rows == g.R && m.out->cols == g.P * s.G)) &&
      (!m.out_plain || (m.out_plain->rows == g.M && m.out_plain->cols == s.G)) &&
      (!m.in_deriv || (m.in_deriv->rows == g.R && m.in_deriv->cols == g.HW * s.C &&
                       s.pad_h <= s.kh - 1 && s.pad_w <= s.kw - 1));
  return ok ? 0 : kInvalid;
}

// R * P past the kernels' 32-bit position index
bool too_long(const ConvGeom &g) { return g.M >= ((int64_t)1 << 31); }

// A ph x pw x pc pool over Y [R x P*G] into pool_dim, mask rows of mask_stride
bool pool_fits(const ConvGeom &g, MatrixDim out_dim, MatrixDim pool_dim, int mask_stride,
               int ph, int pw, int pc) {
  return ph > 0 && pw > 0 && pc > 0 && pool_dim.rows == g.R &&
         (int64_t)pool_dim.cols * ph * pw * pc == out_dim.cols && mask_stride >= pool_dim.cols;
}

// The flipped kernel's bytes in the data gradient's workspace (256-B padded)
size_t flip_bytes(const ConvShape &s) {
  return ((size_t)s.kh * s.kw * s.G * s.C * sizeof(float) + 255) & ~(size_t)255;
}

// ---- forward: Conv2D + bias (+ ReLU when relu; then -1 means "run unfused")
int conv2d_forward(const float *in, MatrixDim in_dim, const ConvShape &s, const float *kernel,
                   MatrixDim kernel_dim, const float *bias, float *out, MatrixDim out_dim,
                   int concat, void *ws, size_t ws_bytes, kcnn_stream_t stream, int relu) {
  ConvGeom g;
  if (conv_args(in_dim.rows, s, {&in_dim, &kernel_dim, nullptr, concat ? &out_dim : nullptr,
                                 concat ? nullptr : &out_dim, nullptr}, g))
    return kInvalid;
  if (g.M == 0) return 0;
  if (too_long(g)) return kInvalid;
  if (!concat) bias = nullptr;
  hipStream_t st = as_stream(stream);
  const int xs = in_dim.stride, ks = kernel_dim.stride, os = out_dim.stride;
  int rc;
  // the fused ReLU runs in the implicit GEMMs' epilogue only (conv-geom.h:
  // the same kernel as the unfused convolution)
  if (relu && !kcnn::unfused_is_igemm(g, concat)) return -1;
  // frame: short kernels (Kdim <= 64) on maps of 16 positions and more, one
  // frame per workgroup pass with the map and the filters in LDS
  if (!relu && concat && kcnn_conv_fwd_frame(g, in, xs, kernel, ks, bias, out, os, st) == 0)
    return 0;
  // direct: at most 8 filters (the data gradient of a 1- or 3-channel layer)
  if (!relu && (rc = kcnn_conv_direct(g, concat, in, xs, kernel, ks, bias, out, os, st)) >= 0)
    return rc;
  // igemm_x6: long kernels on the f16 / bf16 MFMAs with exact operand splits
  if (concat && kcnn_conv_igemm_x6(g, in, xs, kernel, ks, bias, out, os, relu, st) == 0)
    return 0;
  // igemm2: the same contraction on the fp32 MFMAs (family igemm_x6 = 0, or
  // shapes past the bf16 kernel's limits)
  if (concat && (rc = kcnn_conv_igemm2(g, in, xs, kernel, ks, bias, out, os, relu, st)) >= 0)
    return rc;
  if (relu) return -1;
  // igemm: everything else (plain layout, unaligned or > 2 GB operands),
  // split over K when the workspace allows
  return kcnn_conv_igemm(g, in, xs, kernel, ks, bias, out, os, concat, ws, ws_bytes, st);
}

// ---- weight gradient on the bf16 MFMAs: partials, then their reduction
int wgrad_x6(const ConvGeom &g, const float *X, int xs, const float *dY, int dys, float *gW,
             int gws, float *gb, void *ws, size_t ws_bytes, hipStream_t st) {
  int S, fps;
  size_t need;
  if (!kcnn_conv_wgrad_x6_plan(g, xs, dys, S, fps, need) || ws == nullptr || ws_bytes < need)
    return -1;
  float *part = static_cast<float *>(ws);
  const int rc = kcnn_conv_wgrad_x6(g, X, xs, dY, dys, part, S, fps, st);
  if (rc) return rc;
  return kcnn_reduce_splits_wgrad(part, S, g.G * g.Kdim + g.G, g.G * g.Kdim, g.Kdim, gW, gws,
                                  gb, st);
}

// ---- the pooled backward of a ph x 1 x pc window (ph == 1: channel-only,
// 1-byte mask; else a 2-byte mask), mask_pitch = the mask's row pitch in
// bytes.  One route, the fused backward: -1 declined, > 0 a HIP error.
int conv2d_backward_pooled(const float *in, MatrixDim in_dim, const ConvShape &s,
                           const unsigned char *mask, int64_t mask_pitch, int64_t mask_cols,
                           const float *pool_deriv, MatrixDim pool_deriv_dim, int ph, int pc,
                           const float *kernel, MatrixDim kernel_dim, float *in_deriv,
                           MatrixDim in_deriv_dim, float *grad_W, MatrixDim grad_W_dim,
                           float *grad_b, void *ws, size_t ws_bytes, hipStream_t st) {
  ConvGeom g;
  if (conv_args(in_dim.rows, s, {&in_dim, &kernel_dim, grad_W ? &grad_W_dim : nullptr, nullptr,
                                 nullptr, in_deriv ? &in_deriv_dim : nullptr}, g))
    return kInvalid;
  if (!(pc == 2 || pc == 4 || pc == 8) || s.G % pc != 0 ||  // pc = 2: declined below
      ph < 1 || g.oh % ph != 0 || pool_deriv_dim.rows != g.R ||
      (int64_t)pool_deriv_dim.cols * pc * ph != (int64_t)g.P * s.G || mask == nullptr ||
      mask_cols < pool_deriv_dim.cols || (grad_W == nullptr && in_deriv == nullptr))
    return kInvalid;
  if (too_long(g) || mask_pitch >= ((int64_t)1 << 31)) return kInvalid;
  if (g.R == 0) return 0;
  return kcnn_conv_bwd_frame(g, in, in_dim.stride, pool_deriv, pool_deriv_dim.stride, kernel,
                             kernel_dim.stride, in_deriv, in_deriv ? in_deriv_dim.stride : 0,
                             grad_W, grad_W ? grad_W_dim.stride : 0, grad_b, ws, ws_bytes, st,
                             mask, (int)mask_pitch, pc, ph);
}

}  // namespace

extern "C" {

size_t hipF_conv2d_workspace_bytes(MatrixDim in_dim, int in_height, int in_width,
                                   int in_channel, int pad_h, int pad_w, int kernel_height,
                                   int kernel_width, int group) {
  const ConvShape s{in_height, in_width, in_channel, pad_h, pad_w, kernel_height,
                    kernel_width, group};
  ConvGeom g;
  if (conv_args(in_dim.rows, s, {}, g)) return 0;
  if (use_direct(g, 1)) return 0;  // caller decides concat; direct needs none
  return kcnn_conv_igemm_ws(g);
}

int hipF_conv2d(const float *in, MatrixDim in_dim, int in_height, int in_width,
                int in_channel, int pad_h, int pad_w, const float *kernel,
                MatrixDim kernel_dim, int kernel_height, int kernel_width, int group,
                const float *bias, float *out, MatrixDim out_dim, int concat, void *workspace,
                size_t workspace_bytes, kcnn_stream_t stream) {
  const ConvShape s{in_height, in_width, in_channel, pad_h, pad_w, kernel_height,
                    kernel_width, group};
  return conv2d_forward(in, in_dim, s, kernel, kernel_dim, bias, out, out_dim, concat,
                        workspace, workspace_bytes, stream, 0);
}

int hipF_conv2d_relu(const float *in, MatrixDim in_dim, int in_height, int in_width,
                     int in_channel, int pad_h, int pad_w, const float *kernel,
                     MatrixDim kernel_dim, int kernel_height, int kernel_width, int group,
                     const float *bias, float *out, MatrixDim out_dim, kcnn_stream_t stream) {
  const ConvShape s{in_height, in_width, in_channel, pad_h, pad_w, kernel_height,
                    kernel_width, group};
  return conv2d_forward(in, in_dim, s, kernel, kernel_dim, bias, out, out_dim, 1,
                        nullptr, 0, stream, 1);
}

// Conv2D(concat) + bias + channel-only Maxpool_prop in one pass (see
// include/cnsl-hip-kernels.h).  Returns -1 (nothing launched) when the
// geometry is not covered, so the caller runs the two components unfused.
int hipF_conv2d_maxpool(const float *in, MatrixDim in_dim, int in_height, int in_width,
                        int in_channel, int pad_h, int pad_w, const float *kernel,
                        MatrixDim kernel_dim, int kernel_height, int kernel_width, int group,
                        const float *bias, float *out, MatrixDim out_dim, float *pool,
                        MatrixDim pool_dim, unsigned char *mask, int mask_stride,
                        int pool_channel_dim, kcnn_stream_t stream) {
  return kcnn_conv2d_maxpool_stats(in, in_dim, in_height, in_width, in_channel, pad_h, pad_w,
                                   kernel, kernel_dim, kernel_height, kernel_width, group,
                                   bias, out, out_dim, pool, pool_dim, mask, mask_stride,
                                   pool_channel_dim, stream, nullptr);
}

// The scratch words for the pooled output's statistics (pool-stats.h) of
// hipF_conv2d_maxpool's geometry; 0 when the layer takes no frame kernel.
size_t kcnn_conv2d_maxpool_stats_words(int rows, int in_height, int in_width, int in_channel,
                                       int kernel_height, int kernel_width, int group,
                                       int pool_channel_dim) {
  const ConvShape s{in_height,     in_width,     in_channel, /*pad_h=*/0, /*pad_w=*/0,
                    kernel_height, kernel_width, group};
  ConvGeom g;
  if (conv_args(rows, s, {}, g) || pool_channel_dim <= 0) return 0;
  return kcnn_pool_stats_partial_words(g, pool_channel_dim);
}

// hipF_conv2d_maxpool plus the pooled output's statistics when its kernel
// gives them (stats nullable; stats->produced tells).  One route: the
// register forward with the pool in its epilogue.
int kcnn_conv2d_maxpool_stats(const float *in, MatrixDim in_dim, int in_height, int in_width,
                              int in_channel, int pad_h, int pad_w, const float *kernel,
                              MatrixDim kernel_dim, int kernel_height, int kernel_width,
                              int group, const float *bias, float *out, MatrixDim out_dim,
                              float *pool, MatrixDim pool_dim, unsigned char *mask,
                              int mask_stride, int pool_channel_dim, kcnn_stream_t stream,
                              PoolStatsOut *stats) {
  const ConvShape s{in_height, in_width, in_channel, pad_h, pad_w, kernel_height,
                    kernel_width, group};
  if (stats) stats->produced = 0;
  ConvGeom g;
  if (conv_args(in_dim.rows, s, {&in_dim, &kernel_dim, nullptr, &out_dim}, g) ||
      !pool_fits(g, out_dim, pool_dim, mask_stride, 1, 1, pool_channel_dim))
    return kInvalid;
  if (g.R == 0) return 0;
  if (too_long(g)) return -1;
  return kcnn_conv_fwd_frame_pool(g, in, in_dim.stride, kernel, kernel_dim.stride, bias, out,
                                  out_dim.stride, pool, pool_dim.stride, mask, mask_stride,
                                  pool_channel_dim, as_stream(stream), 1, 1, stats) == 0
             ? 0
             : -1;
}

int hipF_conv2d_maxpool3d(const float *in, MatrixDim in_dim, int in_height, int in_width,
                          int in_channel, int pad_h, int pad_w, const float *kernel,
                          MatrixDim kernel_dim, int kernel_height, int kernel_width, int group,
                          const float *bias, float *out, MatrixDim out_dim, float *pool,
                          MatrixDim pool_dim, unsigned short *mask, int mask_stride,
                          int pool_height_dim, int pool_width_dim, int pool_channel_dim,
                          kcnn_stream_t stream) {
  const ConvShape s{in_height, in_width, in_channel, pad_h, pad_w, kernel_height,
                    kernel_width, group};
  const int ph = pool_height_dim, pw = pool_width_dim, pc = pool_channel_dim;
  ConvGeom g;
  if (conv_args(in_dim.rows, s, {&in_dim, &kernel_dim, nullptr, &out_dim}, g) ||
      !pool_fits(g, out_dim, pool_dim, mask_stride, ph, pw, pc))
    return kInvalid;
  if (g.R == 0) return 0;
  if (too_long(g)) return -1;
  hipStream_t st = as_stream(stream);
  const int xs = in_dim.stride, ks = kernel_dim.stride, os = out_dim.stride;
  // frame: the register forward with the window in its epilogue
  if (kcnn_conv_fwd_frame_pool(g, in, xs, kernel, ks, bias, out, os, pool, pool_dim.stride,
                               reinterpret_cast<unsigned char *>(mask), mask_stride, pc, st,
                               ph, pw) == 0)
    return 0;
  // igemm_x6: long kernels, the pool in the implicit GEMM's epilogue, where
  // the unfused convolution is that same kernel (conv-geom.h)
  if (!kcnn::unfused_is_igemm(g, 1)) return -1;
  return kcnn_conv_igemm_x6_pool(g, in, xs, kernel, ks, bias, out, os, pool, pool_dim.stride,
                                 mask, mask_stride, ph, pw, pc, st) == 0
             ? 0
             : -1;
}

size_t hipF_conv2d_wgrad_workspace_bytes(MatrixDim in_dim, int in_height, int in_width,
                                         int in_channel, int pad_h, int pad_w,
                                         int kernel_height, int kernel_width, int group) {
  const ConvShape s{in_height, in_width, in_channel, pad_h, pad_w, kernel_height,
                    kernel_width, group};
  ConvGeom g;
  if (conv_args(in_dim.rows, s, {}, g)) return 0;
  // the largest of the routes' needs (hipF_conv2d_wgrad)
  const int xs = in_dim.stride > 0 ? in_dim.stride : g.HW * in_channel, dys = g.P * group;
  int xS, xfps;
  size_t x6 = 0;
  if (!kcnn_conv_wgrad_x6_plan(g, xs, dys, xS, xfps, x6)) x6 = 0;
  return std::max({kcnn_conv_bwd_frame_ws(g), kcnn_conv_wgrad_frame_ws(g), x6,
                   kcnn_conv_wgrad2_ws(g, xs, dys), kcnn_conv_wgrad_ws(g)});
}

int hipF_conv2d_wgrad(const float *in, MatrixDim in_dim, int in_height, int in_width,
                      int in_channel, int pad_h, int pad_w, const float *out_deriv,
                      MatrixDim out_deriv_dim, int kernel_height, int kernel_width, int group,
                      float *grad_W, MatrixDim grad_W_dim, float *grad_b, void *workspace,
                      size_t workspace_bytes, kcnn_stream_t stream) {
  const ConvShape s{in_height, in_width, in_channel, pad_h, pad_w, kernel_height,
                    kernel_width, group};
  ConvGeom g;
  if (conv_args(in_dim.rows, s, {&in_dim, nullptr, &grad_W_dim, &out_deriv_dim}, g) ||
      too_long(g))
    return kInvalid;
  hipStream_t st = as_stream(stream);
  const int xs = in_dim.stride, dys = out_deriv_dim.stride, gws = grad_W_dim.stride;
  int rc;
  if (g.M > 0) {
    // fused backward: its gradient-only pass (Kdim <= 31; one stream of dY)
    if ((rc = kcnn_conv_bwd_frame(g, in, xs, out_deriv, dys, nullptr, 0, nullptr, 0, grad_W,
                                  gws, grad_b, workspace, workspace_bytes, st)) >= 0)
      return rc;
    // frame: short kernels the fused backward declined (G up to 256)
    if ((rc = kcnn_conv_wgrad_frame(g, in, xs, out_deriv, dys, grad_W, gws, grad_b, workspace,
                                    workspace_bytes, st)) >= 0)
      return rc;
    // wgrad_x6: long kernels on the bf16 MFMAs
    if ((rc = wgrad_x6(g, in, xs, out_deriv, dys, grad_W, gws, grad_b, workspace,
                       workspace_bytes, st)) >= 0)
      return rc;
    // wgrad2: long kernels on the fp32 MFMAs (family wgrad_x6 = 0), P <= 96
    if ((rc = kcnn_conv_wgrad2(g, in, xs, out_deriv, dys, grad_W, gws, grad_b, workspace,
                               workspace_bytes, st)) >= 0)
      return rc;
  }
  // wgrad: everything else, and the zero gradient of an empty batch
  return kcnn_conv_wgrad(g, in, xs, out_deriv, dys, grad_W, gws, grad_b, workspace,
                         workspace_bytes, st);
}

size_t hipF_conv2d_dgrad_workspace_bytes(MatrixDim out_deriv_dim, int in_height, int in_width,
                                         int in_channel, int pad_h, int pad_w,
                                         int kernel_height, int kernel_width, int group) {
  const ConvShape s{in_height, in_width, in_channel, pad_h, pad_w, kernel_height,
                    kernel_width, group};
  ConvGeom g;
  if (conv_args(out_deriv_dim.rows, s, {}, g)) return 0;
  // flip: flipped kernel + the forward routes over the virtually padded dY
  ConvGeom gt = make_geom(out_deriv_dim.rows, g.oh, g.ow, group, kernel_height - 1 - pad_h,
                          kernel_width - 1 - pad_w, kernel_height, kernel_width, in_channel);
  return std::max(flip_bytes(s) + (use_direct(gt, 1) ? 0 : kcnn_conv_igemm_ws(gt)),
                  kcnn_conv_dgrad_scatter_ws(g));
}

int hipF_conv2d_dgrad(const float *out_deriv, MatrixDim out_deriv_dim, int in_height,
                      int in_width, int in_channel, int pad_h, int pad_w, const float *kernel,
                      MatrixDim kernel_dim, int kernel_height, int kernel_width, int group,
                      float *in_deriv, MatrixDim in_deriv_dim, void *workspace,
                      size_t workspace_bytes, kcnn_stream_t stream) {
  const ConvShape s{in_height, in_width, in_channel, pad_h, pad_w, kernel_height,
                    kernel_width, group};
  ConvGeom g;
  if (conv_args(out_deriv_dim.rows, s,
                {nullptr, &kernel_dim, nullptr, &out_deriv_dim, nullptr, &in_deriv_dim}, g))
    return kInvalid;
  if (g.R == 0) return 0;
  if (too_long(g)) return kInvalid;
  hipStream_t st = as_stream(stream);
  const int dys = out_deriv_dim.stride, ks = kernel_dim.stride, dxs = in_deriv_dim.stride;
  int rc;
  // fused backward: its data-gradient-only pass (Kdim <= 31)
  if ((rc = kcnn_conv_bwd_frame(g, nullptr, 0, out_deriv, dys, kernel, ks, in_deriv, dxs,
                                nullptr, 0, nullptr, nullptr, 0, st)) >= 0)
    return rc;
  // frame: Kdim <= 32 with 64 or 128 filters
  if ((rc = kcnn_conv_dgrad_frame(g, out_deriv, dys, kernel, ks, in_deriv, dxs, st)) >= 0)
    return rc;
  // scatter: long kernels on maps with more positions than the output
  if ((rc = kcnn_conv_dgrad_scatter(g, out_deriv, dys, kernel, ks, in_deriv, dxs, workspace,
                                    workspace_bytes, st)) >= 0)
    return rc;
  // flip: dX = Conv2D(virtually padded dY, FlipMat(W)) -- the reference's
  // flip branch (nnet-component-nnet0.cc:529-540) in gather form, through
  // the forward routes
  if (workspace == nullptr ||
      workspace_bytes < hipF_conv2d_dgrad_workspace_bytes(out_deriv_dim, in_height, in_width,
                                                          in_channel, pad_h, pad_w,
                                                          kernel_height, kernel_width, group))
    return kInvalid;
  float *flip = static_cast<float *>(workspace);
  const MatrixDim fd{kernel_height * kernel_width * group, in_channel, in_channel};
  rc = hipF_flip_mat(kernel, kernel_dim, kernel_height, kernel_width, group, flip, fd, stream);
  if (rc) return rc;
  const size_t fb = flip_bytes(s);
  return hipF_conv2d(out_deriv, out_deriv_dim, g.oh, g.ow, group, kernel_height - 1 - pad_h,
                     kernel_width - 1 - pad_w, flip, fd, kernel_height, kernel_width,
                     in_channel, nullptr, in_deriv, in_deriv_dim, 1,
                     static_cast<char *>(workspace) + fb, workspace_bytes - fb, stream);
}

size_t hipF_conv2d_backward_workspace_bytes(MatrixDim in_dim, int in_height, int in_width,
                                            int in_channel, int pad_h, int pad_w,
                                            int kernel_height, int kernel_width, int group) {
  const ConvShape s{in_height, in_width, in_channel, pad_h, pad_w, kernel_height,
                    kernel_width, group};
  ConvGeom g;
  if (conv_args(in_dim.rows, s, {}, g)) return 0;
  const MatrixDim od{in_dim.rows, g.P * group, g.P * group};
  return std::max({kcnn_conv_bwd_frame_ws(g),
                   hipF_conv2d_dgrad_workspace_bytes(od, in_height, in_width, in_channel, pad_h,
                                                     pad_w, kernel_height, kernel_width, group),
                   hipF_conv2d_wgrad_workspace_bytes(in_dim, in_height, in_width, in_channel,
                                                     pad_h, pad_w, kernel_height, kernel_width,
                                                     group)});
}

int hipF_conv2d_backward_pooled(const float *in, MatrixDim in_dim, int in_height, int in_width,
                                int in_channel, int pad_h, int pad_w,
                                const unsigned char *mask, int mask_stride,
                                const float *pool_deriv, MatrixDim pool_deriv_dim,
                                int pool_channel_dim, const float *kernel,
                                MatrixDim kernel_dim, int kernel_height, int kernel_width,
                                int group, float *in_deriv, MatrixDim in_deriv_dim,
                                float *grad_W, MatrixDim grad_W_dim, float *grad_b,
                                void *workspace, size_t workspace_bytes,
                                kcnn_stream_t stream) {
  const ConvShape s{in_height, in_width, in_channel, pad_h, pad_w, kernel_height,
                    kernel_width, group};
  return conv2d_backward_pooled(in, in_dim, s, mask, mask_stride, mask_stride,
                                pool_deriv, pool_deriv_dim, 1, pool_channel_dim, kernel,
                                kernel_dim, in_deriv, in_deriv_dim, grad_W, grad_W_dim, grad_b,
                                workspace, workspace_bytes, as_stream(stream));
}

int hipF_conv2d_backward_pooled3d(const float *in, MatrixDim in_dim, int in_height,
                                  int in_width, int in_channel, int pad_h, int pad_w,
                                  const unsigned short *mask, int mask_stride,
                                  const float *pool_deriv, MatrixDim pool_deriv_dim,
                                  int pool_height_dim, int pool_width_dim,
                                  int pool_channel_dim, const float *kernel,
                                  MatrixDim kernel_dim, int kernel_height, int kernel_width,
                                  int group, float *in_deriv, MatrixDim in_deriv_dim,
                                  float *grad_W, MatrixDim grad_W_dim, float *grad_b,
                                  void *workspace, size_t workspace_bytes,
                                  kcnn_stream_t stream) {
  const ConvShape s{in_height, in_width, in_channel, pad_h, pad_w, kernel_height,
                    kernel_width, group};
  if (pool_width_dim != 1 || pool_height_dim < 2) return -1;  // not covered
  return conv2d_backward_pooled(in, in_dim, s,
                                reinterpret_cast<const unsigned char *>(mask),
                                (int64_t)mask_stride * 2, mask_stride, pool_deriv,
                                pool_deriv_dim, pool_height_dim, pool_channel_dim, kernel,
                                kernel_dim, in_deriv, in_deriv_dim, grad_W, grad_W_dim, grad_b,
                                workspace, workspace_bytes, as_stream(stream));
}

int hipF_conv2d_backward(const float *in, MatrixDim in_dim, int in_height, int in_width,
                         int in_channel, int pad_h, int pad_w, const float *out_deriv,
                         MatrixDim out_deriv_dim, const float *kernel, MatrixDim kernel_dim,
                         int kernel_height, int kernel_width, int group, float *in_deriv,
                         MatrixDim in_deriv_dim, float *grad_W, MatrixDim grad_W_dim,
                         float *grad_b, void *workspace, size_t workspace_bytes,
                         kcnn_stream_t stream) {
  const ConvShape s{in_height, in_width, in_channel, pad_h, pad_w, kernel_height,
                    kernel_width, group};
  ConvGeom g;
  if (conv_args(in_dim.rows, s,
                {&in_dim, &kernel_dim, &grad_W_dim, &out_deriv_dim, nullptr,
                 in_deriv ? &in_deriv_dim : nullptr}, g) ||
      grad_W == nullptr || too_long(g))
    return kInvalid;
  // fused backward: dX and gW / gb from one pass over dY (Kdim <= 31); a
  // route that declines (-1) has launched nothing, an error is returned
  if (g.R > 0) {
    const int rc = kcnn_conv_bwd_frame(
        g, in, in_dim.stride, out_deriv, out_deriv_dim.stride, kernel, kernel_dim.stride,
        in_deriv, in_deriv ? in_deriv_dim.stride : 0, grad_W, grad_W_dim.stride, grad_b,
        workspace, workspace_bytes, as_stream(stream));
    if (rc >= 0) return rc;
  }
  // else the data gradient's routes, then the weight gradient's
  if (in_deriv != nullptr) {
    const int rc = hipF_conv2d_dgrad(out_deriv, out_deriv_dim, in_height, in_width, in_channel,
                                     pad_h, pad_w, kernel, kernel_dim, kernel_height,
                                     kernel_width, group, in_deriv, in_deriv_dim, workspace,
                                     workspace_bytes, stream);
    if (rc) return rc;
  }
  return hipF_conv2d_wgrad(in, in_dim, in_height, in_width, in_channel, pad_h, pad_w,
                           out_deriv, out_deriv_dim, kernel_height, kernel_width, group, grad_W,
                           grad_W_dim, grad_b, workspace, workspace_bytes, stream);
}

}  // extern "C"
