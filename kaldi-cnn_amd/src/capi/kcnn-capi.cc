// capi/kcnn-capi.cc -- extern "C" layer of libkcnn.so (include/kcnn.h).
// Converts C++ exceptions (KALDI_ASSERT / KALDI_ERR / HIP errors) into error
// codes + kcnn_last_error(), and wraps caller device buffers as CuSubMatrix /
// borrowed CuMatrix views.  The component stack behind kcnn_nnet_* is
// kcnn::NnetStack (nnet-stack.h).
#include "kcnn.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "../cnslmat/hip-util.h"
#include "../kaldi-lite/cu-device.h"
#include "../kaldi-lite/cu-kernels-lite.h"
#include "../kaldi-lite/cu-matrix.h"
#include "../kaldi-lite/kaldi-io.h"
#include "../nnet0/nnet-component-nnet0.h"
#include "../nnet2/nnet-component.h"
#include "../nnet2/nnet-kernels.h"
#include "nnet-stack.h"
#include "online-computer.h"
#include "xent-labels.h"

using namespace kaldi;
using namespace kaldi::nnet2;

struct kcnn_nnet {
  kcnn::NnetStack stack;
  template <typename... Args>
  explicit kcnn_nnet(Args &&...args) : stack(std::forward<Args>(args)...) {}
};

// A corpus that stays on the device: the caller's feature matrix (borrowed)
// and its utterances' starts (frame-index.h).
struct kcnn_corpus {
  const float *feats = nullptr;
  MatrixDim dim = {0, 0, 0};
  kcnn::CorpusIndex index;
};

struct kcnn_online {
  kcnn::OnlineComputer computer;
  template <typename... Args>
  explicit kcnn_online(Args &&...args) : computer(std::forward<Args>(args)...) {}
};

namespace {
thread_local std::string g_err;

int fail(const char *what) {
  g_err = what;
  return -1;
}

template <typename F>
int guard(F f) {
  try {
    f();
    return 0;
  } catch (const std::exception &e) {
    return fail(e.what());
  } catch (...) {
    return fail("unknown C++ exception");
  }
}

CuSubMatrix<BaseFloat> view(const float *p, MatrixDim d) {
  return CuSubMatrix<BaseFloat>(const_cast<float *>(p), d.rows, d.cols, d.stride);
}

void borrow(CuMatrix<BaseFloat> *m, const float *p, MatrixDim d) {
  m->Borrow(const_cast<float *>(p), d.rows, d.cols, d.stride);
}

ChunkInfo chunk_info(int cols, int rows, int num_chunks) {
  if (num_chunks <= 0) num_chunks = rows;
  KALDI_ASSERT(rows > 0 && rows % num_chunks == 0);
  return ChunkInfo(cols, num_chunks, 0, rows / num_chunks - 1);
}

// In/out ChunkInfos of one component call: the output chunk holds frames
// [0, out_rows/num_chunks - 1]; the input chunk is widened by the component's
// Context() (SpliceComponent; {0} for every other component).
void component_chunks(const Component *c, MatrixDim in_dim, MatrixDim out_dim,
                      int num_chunks, ChunkInfo *ii, ChunkInfo *oi) {
  const std::vector<int32> ctx = c->Context();
  if (num_chunks <= 0) num_chunks = out_dim.rows;
  KALDI_ASSERT(out_dim.rows > 0 && out_dim.rows % num_chunks == 0 &&
               in_dim.rows % num_chunks == 0);
  const int ocs = out_dim.rows / num_chunks;
  KALDI_ASSERT(in_dim.rows / num_chunks == ocs + ctx.back() - ctx.front());
  *oi = ChunkInfo(out_dim.cols, num_chunks, 0, ocs - 1);
  if (ctx.front() == 0 && ctx.back() == 0) {
    *ii = ChunkInfo(in_dim.cols, num_chunks, 0, ocs - 1);
  } else {
    // ChunkInfo offsets are >= 0 (Check): shift both by -ctx.front()
    *oi = ChunkInfo(out_dim.cols, num_chunks, -ctx.front(), ocs - 1 - ctx.front());
    *ii = ChunkInfo(in_dim.cols, num_chunks, 0, ocs - 1 + ctx.back() - ctx.front());
  }
}

void copy_out(std::string s, char *buf, size_t len) {
  if (!buf || !len) return;
  strncpy(buf, s.c_str(), len - 1);
  buf[len - 1] = '\0';
}

UpdatableComponent *updatable(const kcnn_component *c) {
  KALDI_ASSERT(c && c->c);
  UpdatableComponent *u = dynamic_cast<UpdatableComponent *>(c->c);
  if (!u) KALDI_ERR << c->c->Type() << " has no parameters";
  return u;
}

// Parameter storage of a component: linear (0), bias (1), prev_grad (2).
void param_ref(const kcnn_component *c, int which, float **data, MatrixDim *dim) {
  using cnsl::nnet0::ConvolutionComponent;
  using cnsl::nnet0::FullyConnectedComponent;
  CuMatrixBase<BaseFloat> *m = nullptr;
  CuVectorBase<BaseFloat> *v = nullptr;
  if (auto *cc = dynamic_cast<ConvolutionComponent *>(c->c)) {
    if (which == 0) m = &cc->LinearParamsMutable();
    else if (which == 1) v = &cc->BiasParamsMutable();
    else if (which == 2) m = &cc->PrevGradMutable();
  } else if (auto *fc = dynamic_cast<FullyConnectedComponent *>(c->c)) {
    if (which == 0) m = &fc->LinearParamsMutable();
    else if (which == 1) v = &fc->BiasParamsMutable();
    else if (which == 2) m = &fc->PrevGradMutable();
  } else if (auto *af = dynamic_cast<AffineComponent *>(c->c)) {
    if (which == 0) m = &af->LinearParamsMutable();
    else if (which == 1) v = &af->BiasParamsMutable();
  }
  if (m) {
    *data = m->Data();
    *dim = m->Dim();
  } else if (v) {
    *data = v->Data();
    dim->rows = 1; dim->cols = v->Dim(); dim->stride = v->Dim();
  } else {
    KALDI_ERR << c->c->Type() << " has no parameter #" << which;
  }
}

void copy2d(float *dst, MatrixDim dd, const float *src, MatrixDim sd) {
  KALDI_ASSERT(dd.rows == sd.rows && dd.cols == sd.cols);
  if (dd.rows == 0 || dd.cols == 0) return;
  CU_SAFE_CALL(hipMemcpy2DAsync(dst, sizeof(float) * dd.stride, src,
                                sizeof(float) * sd.stride,
                                sizeof(float) * dd.cols, dd.rows,
                                hipMemcpyDeviceToDevice,
                                CuDevice::Instantiate().Stream()));
}

// Output and InputDeriv may run deferred work, so they are not const; the C
// signatures of kcnn_nnet_output / kcnn_nnet_input_deriv are.
kcnn::NnetStack &stack(const kcnn_nnet *n) { return const_cast<kcnn_nnet *>(n)->stack; }

void matrix_out(const CuMatrix<BaseFloat> &m, const float **data, MatrixDim *dim) {
  *data = m.Data();
  *dim = m.Dim();
}
}  // namespace

extern "C" {

const char *kcnn_last_error(void) { return g_err.c_str(); }
const char *kcnn_version(void) { return "kcnn-mi355x 0.1 (gfx950)"; }
unsigned long long kcnn_device_malloc_calls(void) {
  return (unsigned long long)CuDevice::Instantiate().MallocCalls();
}

int kcnn_init(int device) {
  return guard([&] { CuDevice::Instantiate().SelectGpuId("yes", device); });
}
int kcnn_set_stream(kcnn_stream_t stream) {
  return guard([&] {
    CuDevice::Instantiate().SetStream(reinterpret_cast<hipStream_t>(stream));
  });
}
int kcnn_synchronize(void) {
  return guard([&] { CuDevice::Instantiate().Synchronize(); });
}
int kcnn_set_literal_path(int literal) {
  cnsl::nnet0::SetLiteralPath(literal != 0);
  return 0;
}
int kcnn_set_fusion(int on) {
  if (on < 0 || on > 2) return fail("kcnn_set_fusion: mode is 0, 1 or 2");
  kcnn::set_fusion_mode(on);
  return 0;
}
int kcnn_set_gemm_mode(int mode) {
  if (mode < 0 || mode > 4) return fail("kcnn_set_gemm_mode: mode is 0 to 4");
  CuDevice::Instantiate().SetGemmMode(mode);
  return 0;
}
int kcnn_gemm_tile_counts(unsigned long long *out, int reset) {
  if (!out) return fail("kcnn_gemm_tile_counts: out is NULL");
  kl_gemm_f16x3_tile_counts(out, reset);
  return 0;
}
int kcnn_gemm_plan(int trans_a, int trans_b, int m, int n, int k, int lda, int ldb, int *out) {
  if (!out) return fail("kcnn_gemm_plan: out is NULL");
  if (m <= 0 || n <= 0 || k <= 0) return fail("kcnn_gemm_plan: dimensions must be positive");
  kl_gemm_f16x3_plan(trans_a, trans_b, m, n, k, lda, ldb, out);
  return 0;
}
int kcnn_gemm_fixup_counts(unsigned long long *out, int reset) {
  if (!out) return fail("kcnn_gemm_fixup_counts: out is NULL");
  kl_gemm_f16x3_fixup_counts(out, reset);
  return 0;
}
int kcnn_gemm_fixup_sites_reset(void) {
  kl_gemm_f16x3_fixup_sites_reset();
  return 0;
}
int kcnn_set_kernel_family(const char *name, int value) {
  const int f = kcnn::family_by_name(name);
  if (f < 0) return fail("kcnn_set_kernel_family: unknown family");
  if (kcnn::set_family(static_cast<kcnn::Family>(f), value) != 0)
    return fail("kcnn_set_kernel_family: value out of range");
  return 0;
}
int kcnn_get_kernel_family(const char *name) {
  const int f = kcnn::family_by_name(name);
  return f < 0 ? -1 : kcnn::family(static_cast<kcnn::Family>(f));
}
int kcnn_gemm(int trans_a, int trans_b, int m, int n, int k, float alpha,
              const float *a, int lda, const float *b, int ldb, float beta,
              float *c, int ldc) {
  return guard([&] {
    if (m < 0 || n < 0 || k < 0) KALDI_ERR << "kcnn_gemm: negative dimension";
    const int ar = trans_a ? k : m, ac = trans_a ? m : k;
    const int br = trans_b ? n : k, bc = trans_b ? k : n;
    if (lda < ac || ldb < bc || ldc < n) KALDI_ERR << "kcnn_gemm: leading dimension too small";
    CuSubMatrix<BaseFloat> A(const_cast<float *>(a), ar, ac, lda);
    CuSubMatrix<BaseFloat> B(const_cast<float *>(b), br, bc, ldb);
    CuSubMatrix<BaseFloat> C(c, m, n, ldc);
    C.AddMatMat(alpha, A, trans_a ? kTrans : kNoTrans, B, trans_b ? kTrans : kNoTrans, beta);
  });
}
int kcnn_split_planes(const float *src, int rows, int cols, int ld, uint16_t *dst, int ldp,
                      int64_t ps) {
  return guard([&] {
    CuDevice &d = CuDevice::Instantiate();
    const int rc = kl_split_planes(src, rows, cols, ld, dst, ldp, ps,
                                   reinterpret_cast<kcnn_stream_t>(d.Stream()));
    if (rc) KALDI_ERR << "kcnn_split_planes: " << hipGetErrorString((hipError_t)rc);
  });
}
int kcnn_gemm_planes(int trans_a, int trans_b, int m, int n, int k, float alpha,
                     const uint16_t *a, int lda, int64_t aps, const uint16_t *b, int ldb,
                     int64_t bps, float beta, float *c, int ldc) {
  return guard([&] {
    CuDevice &d = CuDevice::Instantiate();
    const size_t wsb = kl_gemm_planes_workspace_bytes(m, n, k);
    CuScratch ws_s(wsb);
    void *ws = ws_s.p;
    const int rc = kl_gemm_planes(trans_a, trans_b, m, n, k, alpha, a, lda, aps, b, ldb, bps,
                                  beta, c, ldc, ws, wsb,
                                  reinterpret_cast<kcnn_stream_t>(d.Stream()));
    if (rc) KALDI_ERR << "kcnn_gemm_planes: " << hipGetErrorString((hipError_t)rc);
  });
}
int kcnn_set_profiling(int on) {
  CuDevice::Instantiate().SetProfiling(on != 0);
  return 0;
}
int kcnn_profile_string(char *buf, size_t len) {
  return guard([&] { copy_out(CuDevice::Instantiate().ProfileString(), buf, len); });
}
int kcnn_reset_profile(void) {
  return guard([&] {
    CuDevice &d = CuDevice::Instantiate();
    (void)d.ProfileString();  // resolves and recycles the pending events
    d.ResetProfile();
  });
}
void kcnn_set_randn_seed(uint64_t seed) { SetRandnSeed(seed); }

int kcnn_selftest_fastdiv(void) {
  const uint32_t divs[] = {1, 2, 3, 5, 7, 8, 11, 24, 33, 40, 128, 363, 440,
                           1320, 11616, 46464, 65535, 1000003, 0x7fffffffu};
  uint64_t state = 12345;
  for (uint32_t d : divs) {
    kcnn::FastDiv f(d);
    for (int t = 0; t < 20000; t++) {
      state = state * 6364136223846793005ull + 1442695040888963407ull;
      uint32_t n = (uint32_t)(state >> 33);  // < 2^31
      if (t < 64) n = (uint32_t)t;
      if (t >= 64 && t < 128) n = 0x7fffffffu - (uint32_t)(t - 64);
      uint32_t q, r;
      f.divmod(n, q, r);
      if (q != n / d || r != n % d) {
        std::ostringstream ss;
        ss << "FastDiv(" << d << ") failed at n=" << n << ": " << q << "," << r;
        return fail(ss.str().c_str());
      }
    }
  }
  return 0;
}

// ---- CuMatrixBase methods -----------------------------------------------------
int kcnn_mat_conv2d(const float *in, MatrixDim in_dim, const float *kernel,
                    MatrixDim kernel_dim, int in_height, int in_width,
                    int in_channel, int kernel_height, int kernel_width,
                    int group, float *out, MatrixDim out_dim, int concat) {
  return guard([&] {
    auto x = view(in, in_dim), k = view(kernel, kernel_dim), o = view(out, out_dim);
    x.Conv2D(k, in_height, in_width, in_channel, kernel_height, kernel_width,
             group, &o, concat != 0);
  });
}
int kcnn_mat_add_mat_rep_vec(float *m, MatrixDim dim, const float *vec,
                             int vec_dim, int rep) {
  return guard([&] {
    auto x = view(m, dim);
    CuSubVector<BaseFloat> v(const_cast<float *>(vec), vec_dim);
    x.AddMatRepVec(v, rep);
  });
}
int kcnn_mat_flip_mat(const float *m, MatrixDim dim, int kernel_height,
                      int kernel_width, int in_channel, int group, float *flip,
                      MatrixDim flip_dim) {
  return guard([&] {
    auto x = view(m, dim);
    CuMatrix<BaseFloat> f;
    borrow(&f, flip, flip_dim);
    x.FlipMat(kernel_height, kernel_width, in_channel, group, &f);
  });
}
int kcnn_mat_padding_zero(const float *m, MatrixDim dim, int orig_height,
                          int orig_width, int orig_channel, int kernel_height,
                          int kernel_width, float *padmat, MatrixDim pad_dim) {
  return guard([&] {
    auto x = view(m, dim);
    CuMatrix<BaseFloat> p;
    borrow(&p, padmat, pad_dim);
    x.PaddingZero(orig_height, orig_width, orig_channel, kernel_height,
                  kernel_width, &p);
  });
}
int kcnn_mat_tp_block(const float *m, MatrixDim dim, int in_channel,
                      int block_size, float *out, MatrixDim out_dim) {
  return guard([&] {
    auto x = view(m, dim);
    CuMatrix<BaseFloat> o;
    borrow(&o, out, out_dim);
    x.TpBlock(in_channel, block_size, &o);
  });
}
int kcnn_mat_tp_inside_block(const float *m, MatrixDim dim, int group,
                             int block_size, float *out, MatrixDim out_dim) {
  return guard([&] {
    auto x = view(m, dim);
    CuMatrix<BaseFloat> o;
    borrow(&o, out, out_dim);
    x.TpInsideBlock(group, block_size, &o);
  });
}
int kcnn_mat_mod_permute_channel(float *comp, MatrixDim dim, int comp_idx,
                                 int num_component, int in_height, int in_width,
                                 float *container, MatrixDim container_dim,
                                 int from_comp_to_container) {
  return guard([&] {
    auto c = view(comp, dim);
    auto k = view(container, container_dim);
    c.ModPermuteChannel(comp_idx, num_component, in_height, in_width, &k,
                        from_comp_to_container != 0);
  });
}
int kcnn_mat_mod_permute_row(const float *m, MatrixDim dim, int in_channel,
                             int block_size, float *out, MatrixDim out_dim) {
  return guard([&] {
    auto x = view(m, dim);
    CuMatrix<BaseFloat> o;
    borrow(&o, out, out_dim);
    x.ModPermuteRow(in_channel, block_size, &o);
  });
}
int kcnn_mat_maxpool_prop(const float *in, MatrixDim in_dim, int in_height,
                          int in_width, int pool_height_dim, int pool_width_dim,
                          int pool_channel_dim, int overlap, int overlap2D,
                          float *out, MatrixDim out_dim) {
  return guard([&] {
    auto x = view(in, in_dim), o = view(out, out_dim);
    x.Maxpool_prop(in_height, in_width, pool_height_dim, pool_width_dim,
                   pool_channel_dim, overlap != 0, overlap2D != 0, &o);
  });
}
int kcnn_mat_maxpool_backprop(const float *in_value, MatrixDim in_dim,
                              const float *out_value, MatrixDim ov_dim,
                              const float *out_deriv, MatrixDim od_dim,
                              float *in_deriv, MatrixDim id_dim, int in_height,
                              int in_width, int pool_height_dim,
                              int pool_width_dim, int pool_channel_dim,
                              int overlap, int overlap2D) {
  return guard([&] {
    auto x = view(in_value, in_dim), y = view(out_value, ov_dim),
         dy = view(out_deriv, od_dim);
    CuMatrix<BaseFloat> dx;
    borrow(&dx, in_deriv, id_dim);
    x.Maxpool_backprop(y, dy, &dx, in_height, in_width, pool_height_dim,
                       pool_width_dim, pool_channel_dim, overlap != 0,
                       overlap2D != 0);
  });
}

// ---- components ------------------------------------------------------------------
kcnn_component *kcnn_component_new_from_string(const char *line) {
  kcnn_component *h = nullptr;
  guard([&] { h = new kcnn_component{Component::NewFromString(line)}; });
  return h;
}
kcnn_component *kcnn_component_read(const char *path) {
  kcnn_component *h = nullptr;
  guard([&] {
    std::ifstream is(path, std::ios::binary);
    if (!is) KALDI_ERR << "cannot open " << path;
    bool binary = false;
    if (!InitKaldiInputStream(is, &binary)) KALDI_ERR << "bad Kaldi header in " << path;
    h = new kcnn_component{Component::ReadNew(is, binary)};
  });
  return h;
}
int kcnn_component_write(const kcnn_component *c, const char *path, int binary) {
  return guard([&] {
    std::ofstream os(path, std::ios::binary);
    if (!os) KALDI_ERR << "cannot open " << path << " for writing";
    InitKaldiOutputStream(os, binary != 0);
    c->c->Write(os, binary != 0);
    if (!os) KALDI_ERR << "write failed: " << path;
  });
}
kcnn_component *kcnn_component_copy(const kcnn_component *c) {
  kcnn_component *h = nullptr;
  guard([&] { h = new kcnn_component{c->c->Copy()}; });
  return h;
}
void kcnn_component_free(kcnn_component *c) {
  if (!c) return;
  delete c->c;
  delete c;
}
int kcnn_component_type(const kcnn_component *c, char *buf, size_t len) {
  return guard([&] { copy_out(c->c->Type(), buf, len); });
}
int kcnn_component_info(const kcnn_component *c, char *buf, size_t len) {
  return guard([&] { copy_out(c->c->Info(), buf, len); });
}
int kcnn_component_input_dim(const kcnn_component *c) { return c->c->InputDim(); }
int kcnn_component_output_dim(const kcnn_component *c) { return c->c->OutputDim(); }
int kcnn_component_context(const kcnn_component *c, int *offsets, int max_len) {
  int n = -1;
  guard([&] {
    const std::vector<int32> ctx = c->c->Context();
    n = (int)ctx.size();
    for (int k = 0; k < n && k < max_len; k++) offsets[k] = ctx[k];
  });
  return n;
}
int kcnn_component_nonlinear_stats(const kcnn_component *c, double *value_sum,
                                   double *deriv_sum, int max_len, int *len,
                                   double *count) {
  return guard([&] {
    auto *nl = dynamic_cast<const kaldi::nnet2::NonlinearComponent *>(c->c);
    if (!nl) KALDI_ERR << c->c->Type() << " is not a NonlinearComponent";
    Vector<double> v, d;
    nl->GetValueSum(&v);
    nl->GetDerivSum(&d);
    *len = v.Dim();
    for (int k = 0; k < v.Dim() && k < max_len; k++) {
      value_sum[k] = v(k);
      deriv_sum[k] = d(k);
    }
    *count = nl->Count();
  });
}
int kcnn_component_backprop_needs_input(const kcnn_component *c) {
  return c->c->BackpropNeedsInput();
}
int kcnn_component_backprop_needs_output(const kcnn_component *c) {
  return c->c->BackpropNeedsOutput();
}

int kcnn_component_propagate(const kcnn_component *c, const float *in,
                             MatrixDim in_dim, float *out, MatrixDim out_dim,
                             int num_chunks) {
  return guard([&] {
    auto x = view(in, in_dim), y = view(out, out_dim);
    ChunkInfo ii, oi;
    component_chunks(c->c, in_dim, out_dim, num_chunks, &ii, &oi);
    c->c->Propagate(ii, oi, x, &y);
  });
}

int kcnn_component_backprop(kcnn_component *c, const float *in_value,
                            MatrixDim in_dim, const float *out_value,
                            MatrixDim ov_dim, const float *out_deriv,
                            MatrixDim od_dim, float *in_deriv,
                            MatrixDim id_dim, int num_chunks, int update) {
  return guard([&] {
    auto x = view(in_value, in_dim), y = view(out_value, ov_dim),
         dy = view(out_deriv, od_dim);
    ChunkInfo ii, oi;
    component_chunks(c->c, in_dim, od_dim, num_chunks, &ii, &oi);
    CuMatrix<BaseFloat> dx;
    if (in_deriv) borrow(&dx, in_deriv, id_dim);
    // the component itself, as NnetUpdater passes it: parameters for
    // updatable components, diagnostic stats for NonlinearComponents
    Component *to_update = update ? c->c : nullptr;
    c->c->Backprop(ii, oi, x, y, dy, to_update, in_deriv ? &dx : nullptr);
  });
}

int kcnn_component_param_dim(const kcnn_component *c, int which, int *rows,
                             int *cols) {
  return guard([&] {
    float *p;
    MatrixDim d;
    param_ref(c, which, &p, &d);
    *rows = d.rows;
    *cols = d.cols;
  });
}
int kcnn_component_get_param(const kcnn_component *c, int which, float *dst,
                             MatrixDim dst_dim) {
  return guard([&] {
    float *p;
    MatrixDim d;
    param_ref(c, which, &p, &d);
    copy2d(dst, dst_dim, p, d);
  });
}
int kcnn_component_set_param(kcnn_component *c, int which, const float *src,
                             MatrixDim src_dim) {
  return guard([&] {
    float *p;
    MatrixDim d;
    param_ref(c, which, &p, &d);
    copy2d(p, d, src, src_dim);
  });
}
float kcnn_component_learning_rate(const kcnn_component *c) {
  float lr = -1.0f;
  guard([&] { lr = updatable(c)->LearningRate(); });
  return lr;
}
int kcnn_component_set_learning_rate(kcnn_component *c, float lr) {
  return guard([&] { updatable(c)->SetLearningRate(lr); });
}
int kcnn_component_dot_product(const kcnn_component *a, const kcnn_component *b,
                               float *out) {
  return guard([&] { *out = updatable(a)->DotProduct(*updatable(b)); });
}
int kcnn_component_set_zero(kcnn_component *c, int treat_as_gradient) {
  return guard([&] { updatable(c)->SetZero(treat_as_gradient != 0); });
}
int kcnn_component_scale(kcnn_component *c, float scale) {
  return guard([&] { updatable(c)->Scale(scale); });
}
int kcnn_component_add(kcnn_component *c, float alpha, const kcnn_component *other) {
  return guard([&] { updatable(c)->Add(alpha, *updatable(other)); });
}
int kcnn_component_perturb_params(kcnn_component *c, float stddev) {
  return guard([&] { updatable(c)->PerturbParams(stddev); });
}
int kcnn_component_num_gradient_params(const kcnn_component *c) {
  auto *u = dynamic_cast<UpdatableComponent *>(c->c);
  return u ? u->NumGradientParams() : 0;
}
int kcnn_component_compute_gradient(const kcnn_component *c,
                                    const float *in_value, MatrixDim in_dim,
                                    const float *out_deriv, MatrixDim od_dim,
                                    float *grad) {
  return guard([&] {
    updatable(c)->ComputeGradient(view(in_value, in_dim), view(out_deriv, od_dim),
                                  grad);
  });
}
int kcnn_component_apply_gradient(kcnn_component *c, const float *grad,
                                  int num_sample) {
  return guard([&] { updatable(c)->ApplyGradient(grad, num_sample); });
}
int kcnn_component_backprop_gradient(const kcnn_component *c,
                                     const float *in_value, MatrixDim in_dim,
                                     const float *out_deriv, MatrixDim od_dim,
                                     float *in_deriv, MatrixDim id_dim,
                                     float *grad) {
  return guard([&] {
    const UpdatableComponent *u = updatable(c);
    ChunkInfo ii = chunk_info(in_dim.cols, in_dim.rows, 0);
    ChunkInfo oi = chunk_info(od_dim.cols, od_dim.rows, 0);
    auto x = view(in_value, in_dim);
    CuMatrix<BaseFloat> dx;
    if (in_deriv) borrow(&dx, in_deriv, id_dim);
    u->BackpropGradient(ii, oi, x, x, view(out_deriv, od_dim),
                        in_deriv ? &dx : nullptr, grad);
  });
}
int kcnn_component_conv_flip_branch(const kcnn_component *c) {
  auto *cc = dynamic_cast<cnsl::nnet0::ConvolutionComponent *>(c->c);
  if (!cc) return fail("not a ConvolutionComponent");
  return cc->FlipKernelBranch() ? 1 : 0;
}

namespace {
DropoutComponent *dropout(const kcnn_component *c) {
  KALDI_ASSERT(c && c->c);
  DropoutComponent *d = dynamic_cast<DropoutComponent *>(c->c);
  if (!d) KALDI_ERR << c->c->Type() << " is not a DropoutComponent";
  return d;
}
}  // namespace

int kcnn_component_set_dropout_scale(kcnn_component *c, float scale) {
  return guard([&] { dropout(c)->SetDropoutScale(scale); });
}
int kcnn_component_dropout_seed(const kcnn_component *c, uint64_t *seed) {
  return guard([&] { *seed = dropout(c)->Seed(); });
}
int kcnn_component_set_dropout_seed(kcnn_component *c, uint64_t seed) {
  return guard([&] { dropout(c)->SetSeed(seed); });
}
int kcnn_component_set_dropout_row_offset(kcnn_component *c, uint64_t offset) {
  return guard([&] { dropout(c)->SetRowOffset(offset); });
}

int kcnn_comp_objf_and_deriv(const int32_t *rows, const int32_t *cols, const float *weights,
                             int num, const float *probs, MatrixDim p_dim, float *deriv,
                             MatrixDim d_dim, double *tot_objf, double *tot_weight) {
  return guard([&] {
    KALDI_ASSERT(p_dim.rows == d_dim.rows && p_dim.cols == d_dim.cols);
    const std::string bad = kcnn::check_labels(rows, cols, num, p_dim.rows, p_dim.cols, false);
    if (!bad.empty()) KALDI_ERR << "kcnn_comp_objf_and_deriv: " << bad;
    CuDevice &d = CuDevice::Instantiate();
    hipStream_t st = d.Stream();
    double tot[2] = {0.0, 0.0};
    if (num > 0) {
      const size_t n = (size_t)num;
      CuScratch el(n * 12), dtot(sizeof(tot));
      int32_t *dr = static_cast<int32_t *>(el.p), *dc = dr + n;
      float *dw = reinterpret_cast<float *>(dc + n);
      CU_SAFE_CALL(hipMemcpyAsync(dr, rows, n * 4, hipMemcpyHostToDevice, st));
      CU_SAFE_CALL(hipMemcpyAsync(dc, cols, n * 4, hipMemcpyHostToDevice, st));
      CU_SAFE_CALL(hipMemcpyAsync(dw, weights, n * 4, hipMemcpyHostToDevice, st));
      CU_SAFE_CALL(hipMemsetAsync(dtot.p, 0, sizeof(tot), st));
      kcnn::comp_objf_and_deriv(dr, dc, dw, num, probs, p_dim, deriv, d_dim,
                                static_cast<double *>(dtot.p));
      CU_SAFE_CALL(hipMemcpyAsync(tot, dtot.p, sizeof(tot), hipMemcpyDeviceToHost, st));
      CU_SAFE_CALL(hipStreamSynchronize(st));
    }
    if (tot_objf) *tot_objf = tot[0];
    if (tot_weight) *tot_weight = tot[1];
  });
}

int kcnn_comp_objf_accuracy(const int32_t *rows, const int32_t *cols, const float *weights,
                            int num, const float *probs, MatrixDim p_dim, double *out) {
  return guard([&] {
    const std::string bad = kcnn::check_labels(rows, cols, num, p_dim.rows, p_dim.cols, false);
    if (!bad.empty()) KALDI_ERR << "kcnn_comp_objf_accuracy: " << bad;
    if (num > 0 && weights == nullptr) KALDI_ERR << "kcnn_comp_objf_accuracy: bad label arrays";
    out[0] = out[1] = out[2] = 0.0;
    if (num == 0 || p_dim.rows == 0) return;
    // the kernel takes the labels by row: a stable sort keeps a row's order
    std::vector<int> order(num);
    for (int i = 0; i < num; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return rows[a] < rows[b]; });
    std::vector<int32_t> r(num), c(num);
    std::vector<float> w(num);
    for (int i = 0; i < num; i++) {
      r[i] = rows[order[i]];
      c[i] = cols[order[i]];
      w[i] = weights[order[i]];
    }
    const kcnn::LabelLayout lay = kcnn::label_layout(num, p_dim.rows);
    std::vector<char> image(lay.bytes);
    kcnn::stage_labels(r.data(), c.data(), w.data(), num, p_dim.rows, image.data());
    hipStream_t st = CuDevice::Instantiate().Stream();
    CuScratch dev(lay.bytes), dtot(3 * sizeof(double));
    CuScratch ws(kn_prob_ws(kn_prob_blocks(p_dim)));
    CU_SAFE_CALL(hipMemcpyAsync(dev.p, image.data(), lay.bytes, hipMemcpyHostToDevice, st));
    CU_SAFE_CALL(hipMemsetAsync(dtot.p, 0, 3 * sizeof(double), st));
    const char *base = static_cast<const char *>(dev.p);
    {
      CuProfileScope prof("kn_objf_accuracy");
      CNSL_SAFE_CALL(kn_objf_accuracy(
          probs, p_dim, reinterpret_cast<const int32_t *>(base + lay.row_start),
          reinterpret_cast<const int32_t *>(base + lay.col),
          reinterpret_cast<const float *>(base + lay.weight), static_cast<double *>(dtot.p),
          ws.p, reinterpret_cast<kcnn_stream_t>(st)));
    }
    CU_SAFE_CALL(hipMemcpyAsync(out, dtot.p, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    CU_SAFE_CALL(hipStreamSynchronize(st));
  });
}

// ---- component stack (kcnn::NnetStack) ---------------------------------------------
kcnn_nnet *kcnn_nnet_new(const char *config) {
  kcnn_nnet *n = nullptr;
  guard([&] { n = new kcnn_nnet(config); });
  return n;
}
kcnn_nnet *kcnn_nnet_read(const char *path) {
  kcnn_nnet *n = nullptr;
  guard([&] {
    std::ifstream is(path, std::ios::binary);
    if (!is) KALDI_ERR << "cannot open " << path;
    bool binary = false;
    if (!InitKaldiInputStream(is, &binary)) KALDI_ERR << "bad Kaldi header in " << path;
    n = new kcnn_nnet(is, binary);
  });
  return n;
}
int kcnn_nnet_write(const kcnn_nnet *n, const char *path, int binary) {
  return guard([&] {
    std::ofstream os(path, std::ios::binary);
    if (!os) KALDI_ERR << "cannot open " << path << " for writing";
    InitKaldiOutputStream(os, binary != 0);
    n->stack.Write(os, binary != 0);
    os.flush();
    if (!os) KALDI_ERR << "write failed: " << path;
  });
}
kcnn_nnet *kcnn_nnet_copy(const kcnn_nnet *n, const float *scales, int num_scales,
                          int remove_dropout) {
  kcnn_nnet *copy = nullptr;
  guard([&] { copy = new kcnn_nnet(n->stack, scales, num_scales, remove_dropout != 0); });
  return copy;
}
void kcnn_nnet_free(kcnn_nnet *n) { delete n; }
int kcnn_nnet_num_components(const kcnn_nnet *n) { return n->stack.NumComponents(); }
kcnn_component *kcnn_nnet_component(kcnn_nnet *n, int i) { return n->stack.ComponentAt(i); }

int kcnn_nnet_propagate(kcnn_nnet *n, const float *in, MatrixDim in_dim) {
  return guard([&] { n->stack.Propagate(in, in_dim); });
}
int kcnn_nnet_output(const kcnn_nnet *n, int i, const float **data, MatrixDim *dim) {
  return guard([&] { matrix_out(stack(n).Output(i), data, dim); });
}
int kcnn_nnet_input_deriv(const kcnn_nnet *n, int i, const float **data, MatrixDim *dim) {
  return guard([&] { matrix_out(stack(n).InputDeriv(i), data, dim); });
}
int kcnn_nnet_backprop_component(kcnn_nnet *n, int i, const float *out_deriv,
                                 MatrixDim od_dim, int mode, float *grad,
                                 int skip_first_dx) {
  return guard([&] {
    n->stack.BackpropComponent(i, out_deriv, od_dim,
                               static_cast<kcnn::NnetStack::BackpropMode>(mode), grad,
                               skip_first_dx != 0);
  });
}
int kcnn_nnet_backprop_split(kcnn_nnet *n, int i, const float *out_deriv, MatrixDim od_dim,
                             float *grad, int skip_first_dx, void (*between)(void *),
                             void *ctx) {
  return guard([&] {
    n->stack.BackpropSplit(i, out_deriv, od_dim, grad, skip_first_dx != 0, between, ctx);
  });
}
int kcnn_nnet_backprop(kcnn_nnet *n, const float *out_deriv, MatrixDim od_dim) {
  return guard([&] { n->stack.Backprop(out_deriv, od_dim); });
}
int kcnn_nnet_backprop_xent(kcnn_nnet *n, const int32_t *rows, const int32_t *cols,
                            const float *weights, int num, int skip_first_dx) {
  return guard([&] { n->stack.BackpropXent(rows, cols, weights, num, skip_first_dx != 0); });
}
int kcnn_nnet_xent_deriv(kcnn_nnet *n, const int32_t *rows, const int32_t *cols,
                         const float *weights, int num, int *first, const float **out_deriv,
                         MatrixDim *od_dim) {
  return guard([&] {
    if (first == nullptr || out_deriv == nullptr || od_dim == nullptr)
      KALDI_ERR << "kcnn_nnet_xent_deriv: no result pointers";
    *first = n->stack.XentDeriv(rows, cols, weights, num, out_deriv, od_dim);
  });
}
int kcnn_nnet_set_row_offset(kcnn_nnet *n, uint64_t offset) {
  return guard([&] { n->stack.SetRowOffset(offset); });
}
int kcnn_nnet_skip_dropout_call(kcnn_nnet *n) {
  return guard([&] { n->stack.SkipDropoutCall(); });
}
int kcnn_nnet_objf_total(kcnn_nnet *n, double *out, int reset) {
  return guard([&] { n->stack.ObjfTotal(out, reset != 0); });
}
int kcnn_nnet_compute_prob(kcnn_nnet *n, const float *in, MatrixDim in_dim,
                           const int32_t *rows, const int32_t *cols, const float *weights,
                           int num) {
  return guard([&] { n->stack.ComputeProb(in, in_dim, rows, cols, weights, num); });
}
int kcnn_nnet_prob_total(kcnn_nnet *n, double out[3], int reset) {
  return guard([&] { n->stack.ProbTotal(out, reset != 0); });
}
int kcnn_nnet_left_context(const kcnn_nnet *n) { return n->stack.LeftContext(); }
int kcnn_nnet_right_context(const kcnn_nnet *n) { return n->stack.RightContext(); }
int kcnn_nnet_compute(kcnn_nnet *n, const float *in, MatrixDim in_dim, const int32_t *lengths,
                      int num_utts, int pad_input, const float *priors, int num_priors,
                      float prior_scale, int apply_log, const float **data, MatrixDim *dim) {
  return guard([&] {
    if (data == nullptr || dim == nullptr) KALDI_ERR << "kcnn_nnet_compute: no result pointers";
    matrix_out(n->stack.Compute(in, in_dim, lengths, num_utts, pad_input != 0, priors,
                                num_priors, prior_scale, apply_log != 0),
               data, dim);
  });
}
int kcnn_nnet_compute_shared(kcnn_nnet *n, const float *in, MatrixDim in_dim,
                             const int32_t *lengths, int num_utts, int pad_input,
                             const float *priors, int num_priors, float prior_scale,
                             int apply_log, const float **data, MatrixDim *dim) {
  return guard([&] {
    if (data == nullptr || dim == nullptr)
      KALDI_ERR << "kcnn_nnet_compute_shared: no result pointers";
    matrix_out(n->stack.ComputeShared(in, in_dim, lengths, num_utts, pad_input != 0, priors,
                                      num_priors, prior_scale, apply_log != 0),
               data, dim);
  });
}
int kcnn_nnet_time_shared_prefix(const kcnn_nnet *n) {
  int prefix = 0;
  guard([&] { prefix = n->stack.TimeSharedPlan().prefix(); });
  return prefix;
}
int kcnn_nnet_time_map(const kcnn_nnet *n, int level, const float **data, MatrixDim *dim,
                       int *channels, int *positions, int *dilation) {
  return guard([&] {
    if (data == nullptr || dim == nullptr || channels == nullptr || positions == nullptr ||
        dilation == nullptr)
      KALDI_ERR << "kcnn_nnet_time_map: no result pointers";
    const kcnn::NnetStack::TimeMapInfo m = n->stack.TimeMap(level);
    *data = m.data;
    *dim = m.dim;
    *channels = m.channels;
    *positions = m.positions;
    *dilation = m.dilation;
  });
}
int kcnn_nnet_time_map_height(const kcnn_nnet *n, int level, int *height) {
  return guard([&] {
    if (height == nullptr) KALDI_ERR << "kcnn_nnet_time_map_height: no result pointer";
    *height = n->stack.TimeMap(level).height;
  });
}

// ---- training from a device-resident corpus ----------------------------------------
kcnn_corpus *kcnn_corpus_new(const float *feats, MatrixDim dim, const int32_t *lengths,
                             int num_utts) {
  kcnn_corpus *c = nullptr;
  guard([&] {
    std::unique_ptr<kcnn_corpus> made(new kcnn_corpus);
    const std::string bad =
        kcnn::build_corpus_index(lengths, num_utts, dim.rows, dim.cols, &made->index);
    if (!bad.empty()) KALDI_ERR << "kcnn_corpus_new: " << bad;
    if (feats == nullptr) KALDI_ERR << "kcnn_corpus_new: no feature matrix";
    if (dim.stride < dim.cols)
      KALDI_ERR << "kcnn_corpus_new: a row stride of " << dim.stride << " for " << dim.cols
                << " columns";
    made->feats = feats;
    made->dim = dim;
    c = made.release();
  });
  return c;
}
void kcnn_corpus_free(kcnn_corpus *c) { delete c; }

int kcnn_nnet_propagate_frames(kcnn_nnet *n, const kcnn_corpus *corpus, const int32_t *frames,
                               int num_frames) {
  return guard([&] {
    if (corpus == nullptr) KALDI_ERR << "kcnn_nnet_propagate_frames: no corpus";
    n->stack.PropagateFrames(corpus->feats, corpus->dim, corpus->index, frames, num_frames);
  });
}
int kcnn_nnet_compute_prob_frames(kcnn_nnet *n, const kcnn_corpus *corpus,
                                  const int32_t *frames, int num_frames, const int32_t *rows,
                                  const int32_t *cols, const float *weights, int num) {
  return guard([&] {
    if (corpus == nullptr) KALDI_ERR << "kcnn_nnet_compute_prob_frames: no corpus";
    n->stack.ComputeProbFrames(corpus->feats, corpus->dim, corpus->index, frames, num_frames,
                               rows, cols, weights, num);
  });
}

int kcnn_nnet_propagate_frames_shared(kcnn_nnet *n, const kcnn_corpus *corpus,
                                      const int32_t *frames, int num_frames) {
  return guard([&] {
    if (corpus == nullptr) KALDI_ERR << "kcnn_nnet_propagate_frames_shared: no corpus";
    n->stack.PropagateFramesShared(corpus->feats, corpus->dim, corpus->index, frames,
                                   num_frames);
  });
}
int kcnn_nnet_time_train_prefix(const kcnn_nnet *n) {
  int prefix = 0;
  guard([&] { prefix = n->stack.TimeSharedTrainPlan().prefix(); });
  return prefix;
}
int kcnn_nnet_time_map_deriv(const kcnn_nnet *n, int level, const float **data, MatrixDim *dim,
                             int *channels, int *positions, int *dilation) {
  return guard([&] {
    if (data == nullptr || dim == nullptr || channels == nullptr || positions == nullptr ||
        dilation == nullptr)
      KALDI_ERR << "kcnn_nnet_time_map_deriv: no result pointers";
    const kcnn::NnetStack::TimeMapInfo m = n->stack.TimeMapDeriv(level);
    *data = m.data;
    *dim = m.dim;
    *channels = m.channels;
    *positions = m.positions;
    *dilation = m.dilation;
  });
}
int kcnn_nnet_time_gradient(const kcnn_nnet *n, int i, const float **data, int *num) {
  return guard([&] {
    if (data == nullptr || num == nullptr)
      KALDI_ERR << "kcnn_nnet_time_gradient: no result pointers";
    *data = n->stack.TimeGradient(i, num);
  });
}

// ---- streaming forward pass (kcnn::OnlineComputer) ---------------------------------
kcnn_online *kcnn_online_new(kcnn_nnet *n, int num_streams, int max_chunk, const float *priors,
                             int num_priors, float prior_scale, int apply_log) {
  kcnn_online *o = nullptr;
  guard([&] {
    o = new kcnn_online(n ? &n->stack : nullptr, num_streams, max_chunk, priors, num_priors,
                        prior_scale, apply_log != 0);
  });
  return o;
}
kcnn_online *kcnn_online_new_shared(kcnn_nnet *n, int num_streams, int max_chunk,
                                    const float *priors, int num_priors, float prior_scale,
                                    int apply_log, int share_time) {
  kcnn_online *o = nullptr;
  guard([&] {
    o = new kcnn_online(n ? &n->stack : nullptr, num_streams, max_chunk, priors, num_priors,
                        prior_scale, apply_log != 0, share_time != 0);
  });
  return o;
}
int kcnn_online_shared_prefix(const kcnn_online *o) {
  int prefix = -1;
  guard([&] {
    if (o == nullptr) KALDI_ERR << "kcnn_online_shared_prefix: no computer";
    prefix = o->computer.TimeSharedPrefix();
  });
  return prefix;
}
void kcnn_online_free(kcnn_online *o) { delete o; }

int kcnn_online_accept(kcnn_online *o, const float *chunk, MatrixDim dim, const int32_t *streams,
                       const int32_t *num_new, const int32_t *final, int num, int32_t *num_out,
                       const float **data, MatrixDim *out_dim) {
  return guard([&] {
    if (o == nullptr) KALDI_ERR << "kcnn_online_accept: no computer";
    if (data == nullptr || out_dim == nullptr)
      KALDI_ERR << "kcnn_online_accept: no result pointers";
    matrix_out(o->computer.Accept(chunk, dim, streams, num_new, final, num, num_out), data,
               out_dim);
  });
}
int kcnn_online_reset(kcnn_online *o, int stream) {
  return guard([&] {
    if (o == nullptr) KALDI_ERR << "kcnn_online_reset: no computer";
    o->computer.Reset(stream);
  });
}
int kcnn_online_frames(const kcnn_online *o, int stream, int64_t out[2]) {
  return guard([&] {
    if (o == nullptr || out == nullptr) KALDI_ERR << "kcnn_online_frames: no computer";
    o->computer.Frames(stream, out);
  });
}

}  // extern "C"
