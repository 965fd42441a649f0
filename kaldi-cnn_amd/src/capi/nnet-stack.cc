// capi/nnet-stack.cc -- kcnn::NnetStack (nnet-stack.h).
#include "nnet-stack.h"

#include <stdlib.h>

#include <cmath>
#include <set>
#include <sstream>
#include <string>

#include "../kaldi-lite/kaldi-io.h"
#include "../nnet2/nnet-kernels.h"
#include "xent-labels.h"

using namespace kaldi;
using namespace kaldi::nnet2;

namespace kcnn {

namespace {
int g_fusion = [] {
  const char *e = getenv("KCNN_FUSE");
  return e && *e ? atoi(e) : 1;
}();

// The non-virtual Component::Propagate's sizing (nnet-component.h:203-215):
// resize (zero-filled) only when the size differs.
void size_output(CuMatrix<BaseFloat> *m, int rows, int cols) {
  if (m->NumRows() != rows || m->NumCols() != cols) m->Resize(rows, cols);
}
}  // namespace

int fusion_mode() { return g_fusion; }
void set_fusion_mode(int mode) { g_fusion = mode; }

void comp_objf_and_deriv(const int32_t *rows, const int32_t *cols, const float *weights,
                         int num, const float *probs, MatrixDim p_dim, float *deriv,
                         MatrixDim d_dim, double *tot) {
  CuScratch ws(kn_objf_ws(kn_comp_objf_blocks(num)));
  CuProfileScope prof("kn_comp_objf_and_deriv");
  CNSL_SAFE_CALL(kn_comp_objf_and_deriv(
      rows, cols, weights, num, probs, p_dim, deriv, d_dim, tot, ws.p,
      reinterpret_cast<kcnn_stream_t>(CuDevice::Instantiate().Stream())));
}

NnetStack::NnetStack(const char *config) {
  std::vector<std::unique_ptr<Component>> parsed;
  std::istringstream is(config);
  std::string line;
  while (std::getline(is, line)) {
    const size_t b = line.find_first_not_of(" \t\r");
    if (b == std::string::npos || line[b] == '#') continue;
    parsed.emplace_back(Component::NewFromString(line.substr(b)));
  }
  Init(std::move(parsed));
}

NnetStack::NnetStack(std::istream &is, bool binary) {
  ExpectToken(is, binary, "<Nnet>");
  ExpectToken(is, binary, "<NumComponents>");
  int32 num = 0;
  ReadBasicType(is, binary, &num);
  if (num < 0) KALDI_ERR << "<NumComponents> " << num;
  ExpectToken(is, binary, "<Components>");
  std::vector<std::unique_ptr<Component>> parsed;
  // one at a time: a count the content does not back fails at its first
  // missing component, whatever it claims
  for (int32 i = 0; i < num; i++) parsed.emplace_back(Component::ReadNew(is, binary));
  ExpectToken(is, binary, "</Components>");
  ExpectToken(is, binary, "</Nnet>");
  Init(std::move(parsed));
}

NnetStack::NnetStack(const NnetStack &src, const float *scales, int num_scales,
                     bool remove_dropout) {
  int num_updatable = 0;
  for (const Comp &c : src.comps_) num_updatable += c.updatable != nullptr;
  if (scales != nullptr && num_scales != num_updatable)
    KALDI_ERR << num_scales << " scales for " << num_updatable << " updatable components";
  std::vector<std::unique_ptr<Component>> copies;
  int k = 0;
  for (const Comp &c : src.comps_) {
    const float scale = (c.updatable && scales) ? scales[k] : 1.0f;
    k += c.updatable != nullptr;
    if (remove_dropout && dynamic_cast<const DropoutComponent *>(c.c.get())) continue;
    copies.emplace_back(c.c->Copy());
    if (c.updatable && scales)
      dynamic_cast<UpdatableComponent &>(*copies.back()).Scale(scale);
  }
  Init(std::move(copies));
}

void NnetStack::Write(std::ostream &os, bool binary) const {
  WriteToken(os, binary, "<Nnet>");
  WriteToken(os, binary, "<NumComponents>");
  WriteBasicType(os, binary, (int32)comps_.size());
  WriteToken(os, binary, "<Components>");
  for (const Comp &c : comps_) {
    c.c->Write(os, binary);
    if (!binary) os << std::endl;
  }
  WriteToken(os, binary, "</Components>");
  WriteToken(os, binary, "</Nnet>");
}

void NnetStack::Init(std::vector<std::unique_ptr<Component>> parsed) {
  if (parsed.empty()) KALDI_ERR << "a network needs at least one component";
  const size_t nc = parsed.size();
  for (size_t i = 0; i + 1 < nc; i++)
    if (parsed[i]->OutputDim() != parsed[i + 1]->InputDim())
      KALDI_ERR << "dimension mismatch between component " << i << " ("
                << parsed[i]->OutputDim() << ") and " << i + 1 << " ("
                << parsed[i + 1]->InputDim() << ")";
  // sized once: handles, PoolColDeferreds and matrices are pointed at
  comps_.resize(nc);
  acts_.resize(nc + 1);
  time_maps_.resize(nc);
  time_derivs_.resize(nc);
  time_grads_.resize(nc);
  for (size_t i = 0; i < nc; i++) {
    Comp &c = comps_[i];
    c.c = std::move(parsed[i]);
    Component *p = c.c.get();
    c.handle.c = p;
    c.conv = dynamic_cast<cnsl::nnet0::ConvolutionComponent *>(p);
    c.pool = dynamic_cast<cnsl::nnet0::MaxpoolComponent *>(p);
    c.relu = dynamic_cast<RectifiedLinearComponent *>(p);
    c.affine = dynamic_cast<AffineComponent *>(p);
    c.softmax = dynamic_cast<SoftmaxComponent *>(p);
    c.splice = dynamic_cast<SpliceComponent *>(p);
    c.updatable = dynamic_cast<UpdatableComponent *>(p);
  }
  // The last output is one frame per chunk; walking back, a component's input
  // offsets are the set of output offset + Context().
  acts_[nc].offsets.assign(1, 0);
  for (size_t k = nc; k-- > 0;) {
    const std::vector<int32> ctx = comps_[k].c->Context();
    std::set<int32> in;
    for (int32 o : acts_[k + 1].offsets)
      for (int32 c : ctx) in.insert(o + c);
    acts_[k].offsets.assign(in.begin(), in.end());
  }
  {  // MakeOffsetsContiguous on the network input
    std::vector<int32> &first = acts_[0].offsets;
    const int32 lo = first.front(), hi = first.back();
    first.clear();
    for (int32 o = lo; o <= hi; o++) first.push_back(o);
  }
  // ChunkInfo offsets must be >= 0: shift everything by -first input offset
  const int32 shift = -acts_[0].offsets.front();
  for (Activation &a : acts_)
    for (int32 &o : a.offsets) o += shift;
}

NnetStack::LabelStaging::~LabelStaging() {
  if (copied) {
    (void)hipEventSynchronize(copied);
    (void)hipEventDestroy(copied);
  }
  if (host) (void)hipHostFree(host);
}

kcnn_component *NnetStack::ComponentAt(int i) {
  if (i < 0 || i >= NumComponents()) return nullptr;
  return &comps_[i].handle;
}

ChunkInfo NnetStack::in_info(int i) {
  if (whole_utts_) return ChunkInfo(comps_[i].c->InputDim(), 1, 0, in(i).utt_rows - 1);
  return ChunkInfo(comps_[i].c->InputDim(), num_chunks_, in(i).offsets);
}
ChunkInfo NnetStack::out_info(int i) {
  if (whole_utts_) return ChunkInfo(comps_[i].c->OutputDim(), 1, 0, out(i).utt_rows - 1);
  return ChunkInfo(comps_[i].c->OutputDim(), num_chunks_, out(i).offsets);
}

// Everything that held for the last minibatch only.
void NnetStack::ForgetMinibatch() {
  for (Comp &c : comps_) c.mask_valid = c.deriv_deferred = false;
  xent_fused_ = false;
  for (Activation &a : acts_) {
    a.stale = kStored;
    a.stats_valid = false;
    a.col_deferred.pending = 0;
  }
}

// The statistics of component i's input while its Propagate / Backprop runs,
// when the fused forward that wrote it gave them.
std::unique_ptr<CuGemmStatsHint> NnetStack::input_stats(int i) {
  Activation &a = in(i);
  if (!a.stats_valid) return nullptr;
  const CuMatrix<BaseFloat> &x = a.value;
  uint32_t *stats = static_cast<uint32_t *>(a.stats.p);
  std::unique_ptr<CuGemmStatsHint> h(new CuGemmStatsHint(
      x.Data(), x.NumRows(), x.NumCols(), x.Stride(), stats, stats + 3 * (size_t)x.NumRows()));
  if (a.col_deferred.pending) h->pending = &a.col_deferred;
  return h;
}

// d(output of component i): the caller's for the last component, else the
// input derivative of the component above.
CuSubMatrix<BaseFloat> NnetStack::out_deriv_of(int i, const float *caller_ptr,
                                               MatrixDim caller_dim) {
  if (i == NumComponents() - 1)
    return CuSubMatrix<BaseFloat>(const_cast<float *>(caller_ptr), caller_dim.rows,
                                  caller_dim.cols, caller_dim.stride);
  CuMatrix<BaseFloat> &d = comps_[i + 1].deriv;
  return CuSubMatrix<BaseFloat>(d.Data(), d.NumRows(), d.NumCols(), d.Stride());
}

// NnetUpdater passes every component as to_update: updatable ones only update
// in kUpdate; NonlinearComponent stats (per replica) always accumulate.
Component *NnetStack::to_update(const Comp &c, BackpropMode mode) const {
  return (mode == kUpdate || !c.updatable) ? c.c.get() : nullptr;
}

// Component i (Conv) and i + 1 (Maxpool with a fusable window) in one fused
// pass; false, having launched nothing, when the pair does not qualify.
bool NnetStack::PropagateMaxpoolPair(int i) {
  if (!g_fusion || i + 1 >= NumComponents()) return false;
  const cnsl::nnet0::ConvolutionComponent *conv = comps_[i].conv;
  const cnsl::nnet0::MaxpoolComponent *pool = comps_[i + 1].pool;
  if (!conv || !pool) return false;
  const int mask_bytes = pool->FusedMaskBytes();  // 1: channel-only, 2: 3-D window
  if (mask_bytes == 0) return false;
  Activation &x = in(i), &y = out(i), &pooled = out(i + 1);
  const int rows = x.value.NumRows();
  unsigned char *mask = static_cast<unsigned char *>(
      comps_[i + 1].mask.reserve((size_t)rows * pool->OutputDim() * mask_bytes));
  size_output(&y.value, rows, conv->OutputDim());
  size_output(&pooled.value, rows, pool->OutputDim());
  const bool store = g_fusion == 2;
  // room for the pooled output's statistics (the row block [max, min, cnt]
  // and the column block [max, min, cnt], kept) and the kernel's column
  // partials (kept too: the column work may run in the backward)
  PoolStatsOut ps;
  const size_t pw = mask_bytes == 1 && conv->In_pad_height() == 0 && conv->In_pad_width() == 0
                        ? kcnn_conv2d_maxpool_stats_words(
                              rows, conv->In_height(), conv->In_width(), conv->In_channels(),
                              conv->Kernel_height(), conv->Kernel_width(), conv->Group(),
                              pool->FusableChannelPool())
                        : 0;
  pooled.col_deferred.pending = 0;
  if (pw) {
    ps.partials = static_cast<uint32_t *>(pooled.col_partials.reserve(pw * 4));
    ps.partial_words = pw;
    ps.rowmax = static_cast<uint32_t *>(
        pooled.stats.reserve(4 * 3 * ((size_t)rows + pool->OutputDim())));
    ps.colmax = ps.rowmax + 3 * (size_t)rows;
  }
  {
    PoolColDeferScope defer(pw ? &pooled.col_deferred : nullptr);
    if (!conv->PropagateMaxpool(x.value, &y.value, *pool, &pooled.value, mask,
                                pool->OutputDim(), store, pw ? &ps : nullptr))
      return false;
  }
  pooled.stats_valid = ps.produced;
  comps_[i + 1].mask_valid = true;
  y.stale = store ? kStored : kRecomputable;
  return true;
}

// Component i (Conv) and i + 1 (RectifiedLinearComponent) in one pass, fusion
// mode 1 only: the conv output (the ReLU's in_value, which its Backprop does
// not read) is left unstored; false when the pair does not qualify.
bool NnetStack::PropagateReluPair(int i) {
  if (g_fusion != 1 || i + 1 >= NumComponents()) return false;
  const cnsl::nnet0::ConvolutionComponent *conv = comps_[i].conv;
  const RectifiedLinearComponent *relu = comps_[i + 1].relu;
  if (!conv || !relu || relu->InputDim() != conv->OutputDim()) return false;
  const int rows = in(i).value.NumRows();
  size_output(&out(i).value, rows, conv->OutputDim());
  size_output(&out(i + 1).value, rows, relu->OutputDim());
  if (!conv->PropagateRelu(in(i).value, &out(i + 1).value)) return false;
  out(i).stale = kRecomputable;
  return true;
}

// The rows of the last output for an input of in_dim (one per chunk); throws
// on an input the network cannot take.
static int checked_num_chunks(MatrixDim in_dim, int input_dim, int in_cs) {
  KALDI_ASSERT(in_dim.cols == input_dim);
  if (in_dim.rows % in_cs != 0)
    KALDI_ERR << "input rows " << in_dim.rows << " are not a multiple of the "
              << in_cs << "-frame input chunk";
  return in_dim.rows / in_cs;
}

void NnetStack::PropagateFirst(const float *input, MatrixDim in_dim, int count,
                               const FrameList *fl) {
  const int in_cs = (int)acts_[0].offsets.size();
  num_chunks_ = fl ? fl->num : checked_num_chunks(in_dim, comps_[0].c->InputDim(), in_cs);
  acts_[0].value.Borrow(const_cast<float *>(input), in_dim.rows, in_dim.cols, in_dim.stride);
  ForgetMinibatch();
  prob_forward_ = whole_utts_ = frames_fused_ = time_shared_ = time_train_ = false;
  examples_first_ = 0;
  int first = 0;  // the component the loop starts at
  if (fl != nullptr) {
    // the offset of the input chunk's first frame from an example's own
    const int in_first = -LeftContext();
    if (const SpliceComponent *splice = comps_[0].splice) {
      // the Splice reads the corpus itself: its output rows' offsets from the
      // example's frame are the chunk offsets less the shift Init gave them
      std::vector<int32> out_offsets(out(0).offsets);
      for (int32 &o : out_offsets) o += in_first;
      size_output(&out(0).value, num_chunks_ * (int)out_offsets.size(), splice->OutputDim());
      CuProfileScope prof("kn_splice_frames_prop");
      splice->PropagateFrames(acts_[0].value, &out(0).value, fl->examples, num_chunks_,
                              out_offsets, in_first);
      frames_fused_ = true;
      first = 1;
    } else {
      // the window matrix, laid out as a caller's contiguous one would be
      const int rows = num_chunks_ * in_cs, cols = in_dim.cols;
      float *win = static_cast<float *>(
          frames_input_.reserve(sizeof(float) * (size_t)rows * cols));
      CuSubMatrix<BaseFloat> laid(win, rows, cols, cols);
      {
        CuProfileScope prof("kn_splice_frames_prop");
        SpliceComponent::LayOutFrames(acts_[0].value, &laid, fl->examples, num_chunks_, in_cs,
                                      in_first);
      }
      acts_[0].value.Borrow(win, rows, cols, cols);
    }
  }
  for (int i = first; i < count; i++) {
    if (PropagateMaxpoolPair(i) || PropagateReluPair(i)) { i++; continue; }
    ChunkInfo ii = in_info(i), oi = out_info(i);
    auto hint = input_stats(i);
    comps_[i].c->Propagate(ii, oi, in(i).value, &out(i).value);
  }
}

void NnetStack::Propagate(const float *input, MatrixDim in_dim) {
  PropagateFirst(input, in_dim, NumComponents());
}

int NnetStack::CheckFrames(const FrameList &fl, const char *who) const {
  if (fl.corpus == nullptr || fl.feats == nullptr) KALDI_ERR << who << ": no corpus";
  if (fl.dim.cols != comps_[0].c->InputDim())
    KALDI_ERR << who << ": a corpus of " << fl.dim.cols << " columns for a network of "
              << comps_[0].c->InputDim();
  if (fl.dim.rows != fl.corpus->rows())
    KALDI_ERR << who << ": the corpus index covers " << fl.corpus->rows() << " rows, the matrix "
              << "has " << fl.dim.rows;
  const std::string bad =
      check_frames(*fl.corpus, fl.frames, fl.num, (int)acts_[0].offsets.size());
  if (!bad.empty()) KALDI_ERR << who << ": " << bad;
  CheckExamples(fl.num, who);
  return fl.num;
}

void NnetStack::CheckExamples(int num, const char *who) const {
  std::string bad;
  // every activation of the pass, the window matrix among them
  for (size_t k = 0; bad.empty() && k < acts_.size(); k++)
    bad = check_frames_matrix(k == 0 ? "the input" : "an activation",
                              (int64_t)num * (int64_t)acts_[k].offsets.size(),
                              k == 0 ? comps_[0].c->InputDim() : comps_[k - 1].c->OutputDim());
  if (!bad.empty()) KALDI_ERR << who << ": " << bad;
  if (comps_[0].splice != nullptr) {
    // gapped output offsets travel in the kernel's table of shorts
    const std::vector<int32> &o = acts_[1].offsets;
    if (o.back() - o.front() + 1 != (int32)o.size() &&
        (o.size() > KN_SPLICE_MAX_TAB || acts_[0].offsets.back() > 32767))
      KALDI_ERR << who << ": " << o.size() << " gapped output rows per example in a context of "
                << acts_[0].offsets.back() << " frames exceed the first Splice's offset table";
  }
}

// The examples' triples -> pinned staging buffer -> device, on the library's
// stream (before the labels and the forward, as ComputeProb stages its labels).
void NnetStack::StageFrames(FrameList *fl) {
  const size_t bytes = frame_triples_bytes(fl->num);
  stage_frames(*fl->corpus, fl->frames, fl->num, frames_.Begin(bytes));
  fl->examples = reinterpret_cast<const int32_t *>(
      frames_.Commit(bytes, CuDevice::Instantiate().Stream()));
}

void NnetStack::PropagateFrames(const float *feats, MatrixDim dim, const CorpusIndex &corpus,
                                const int32_t *frames, int num) {
  FrameList fl = {feats, dim, &corpus, frames, num, nullptr};
  CheckFrames(fl, "kcnn_nnet_propagate_frames");  // every check before any launch
  StageFrames(&fl);
  PropagateFirst(feats, dim, NumComponents(), &fl);
}

TimePlan NnetStack::TimeSharedTrainPlan() const {
  TimePlan plan = time_train_plan(TimeSharedPlan());
  if (plan.prefix() == NumComponents()) {
    // the backward over the maps starts from the input derivative of the
    // component above them
    plan.levels.clear();
    plan.declined = "no component follows the prefix";
  }
  return plan;
}

void NnetStack::PropagateFramesShared(const float *feats, MatrixDim dim,
                                      const CorpusIndex &corpus, const int32_t *frames, int num) {
  const char *who = "kcnn_nnet_propagate_frames_shared";
  FrameList fl = {feats, dim, &corpus, frames, num, nullptr};
  CheckFrames(fl, who);  // every check before any launch
  const TimePlan plan = TimeSharedTrainPlan();
  const int p = plan.prefix(), nc = NumComponents();
  if (p == 0) {  // PropagateFrames itself
    StageFrames(&fl);
    PropagateFirst(feats, dim, nc, &fl);
    return;
  }
  const std::vector<FrameRun> runs = frame_runs(corpus, frames, num);
  const int num_runs = (int)runs.size();
  std::vector<int32_t> lengths(runs.size());
  for (size_t j = 0; j < runs.size(); j++) lengths[j] = runs[j].length;
  TimeRows rows;
  const std::string bad = plan_train_rows(plan, lengths.data(), num_runs, &rows);
  if (!bad.empty()) KALDI_ERR << who << ": " << bad;
  KALDI_ASSERT(rows.result_rows == num && p < nc);
  // the runs' starts and triples, staged as PropagateFrames stages its examples
  const size_t bytes = run_image_bytes(runs.size());
  stage_runs(runs, frames_.Begin(bytes));
  const int32_t *d_starts = reinterpret_cast<const int32_t *>(
      frames_.Commit(bytes, CuDevice::Instantiate().Stream()));
  const int32_t *d_runs = d_starts + runs.size() + 1;

  num_chunks_ = num;
  acts_[0].value.Borrow(const_cast<float *>(feats), dim.rows, dim.cols, dim.stride);
  ForgetMinibatch();
  prob_forward_ = whole_utts_ = false;
  examples_first_ = 0;
  // component 0 reads the corpus and has no Backprop, as after PropagateFrames
  frames_fused_ = time_shared_ = time_train_ = true;
  time_backward_done_ = false;
  train_plan_ = plan;
  train_rows_ = rows;
  train_starts_ = d_starts;
  train_runs_ = num_runs;
  time_dviews_.assign((size_t)p, TimeMapInfo());

  // level 0: each run's k + L + R rows, clamped into its utterance
  const int context = plan.levels[0].positions - 1;
  CuMatrix<BaseFloat> &m0 = time_maps_[0];
  if (m0.NumRows() != rows.input_rows || m0.NumCols() != dim.cols)
    m0.Resize((int)rows.input_rows, dim.cols, kUndefined);  // written whole
  {
    CuProfileScope prof("kn_timemap_layout");
    CNSL_SAFE_CALL(kn_timemap_layout(
        feats, dim, m0.Data(), m0.Dim(), d_starts, d_runs, num_runs, LeftContext(), context,
        reinterpret_cast<kcnn_stream_t>(CuDevice::Instantiate().Stream())));
  }
  time_views_.assign((size_t)p, TimeMapInfo());
  const TimeLevel &l0 = plan.levels[0];
  time_views_[0] = TimeMapInfo{m0.Data(), m0.Dim(), l0.channels, l0.positions, l0.dilation,
                               l0.height};
  FormTimeLevels(plan, rows, d_starts, num_runs, num);
  for (int i = p; i < nc; i++) {  // PropagateFirst's loop
    if (PropagateMaxpoolPair(i) || PropagateReluPair(i)) { i++; continue; }
    ChunkInfo ii = in_info(i), oi = out_info(i);
    auto hint = input_stats(i);
    comps_[i].c->Propagate(ii, oi, in(i).value, &out(i).value);
  }
}

NnetStack::TimeMapInfo NnetStack::TimeMapDeriv(int level) const {
  const char *who = "kcnn_nnet_time_map_deriv";
  if (!time_train_ || !time_backward_done_)
    KALDI_ERR << who << ": no backward pass has run over the time maps of a "
              << "kcnn_nnet_propagate_frames_shared";
  if (level < 0 || level >= (int)time_dviews_.size())
    KALDI_ERR << who << ": level " << level << " outside [0, " << time_dviews_.size() << ")";
  if (time_dviews_[level].data == nullptr)
    KALDI_ERR << who << ": level " << level << " has no derivative map (level 0, and a pool's "
              << "own level under a ReLU, are never formed)";
  return time_dviews_[level];
}

const float *NnetStack::TimeGradient(int i, int *num) const {
  const char *who = "kcnn_nnet_time_gradient";
  if (!time_train_ || !time_backward_done_)
    KALDI_ERR << who << ": no backward pass has run over the time maps of a "
              << "kcnn_nnet_propagate_frames_shared";
  if (i < 0 || i >= train_plan_.prefix() || comps_[i].conv == nullptr)
    KALDI_ERR << who << ": component " << i << " is not a Convolution of the "
              << train_plan_.prefix() << " components run as time maps";
  *num = comps_[i].conv->NumGradientParams();
  return time_grads_[i].Data();
}

// The launches of time_backward_schedule in order.  A derivative map has its
// level's geometry and the rows its launch writes; rows no window reads come
// out 0 at every level, since the scatter zeroes them at the top.
void NnetStack::BackpropTimeMaps() {
  const TimePlan &plan = train_plan_;
  const int p = plan.prefix();
  const kcnn_stream_t st = reinterpret_cast<kcnn_stream_t>(CuDevice::Instantiate().Stream());
  const CuMatrix<BaseFloat> &dy = InputDeriv(p);
  KALDI_ASSERT(dy.NumRows() == num_chunks_ && dy.NumCols() == comps_[p - 1].c->OutputDim());
  time_dviews_.assign((size_t)p, TimeMapInfo());
  auto deriv_of = [&](int l, int rows) -> CuMatrix<BaseFloat> & {
    CuMatrix<BaseFloat> &m = time_derivs_[l];
    const TimeLevel &lev = plan.levels[l];
    if (m.NumRows() != rows || m.NumCols() != lev.width) m.Resize(rows, lev.width, kUndefined);
    time_dviews_[l] = TimeMapInfo{m.Data(), m.Dim(), lev.channels, lev.positions, lev.dilation,
                                  lev.height};
    return m;
  };
  auto map_at = [&](int l, int rows) {  // the first `rows` rows of a forward map
    const TimeMapInfo &v = time_views_[l];
    KALDI_ASSERT(v.data != nullptr && v.dim.rows >= rows);
    return CuSubMatrix<BaseFloat>(const_cast<float *>(v.data), rows, v.dim.cols, v.dim.stride);
  };
  for (const TimeBackLaunch &t : time_backward_schedule(plan, train_rows_)) {
    if (t.op == TimeBackLaunch::kScatter) {
      CuMatrix<BaseFloat> &dm = deriv_of(t.din_level, t.in_rows);
      CuProfileScope prof("kn_timemap_scatter");
      CNSL_SAFE_CALL(kn_timemap_scatter(dy.Data(), dy.Dim(), dm.Data(), dm.Dim(), train_starts_,
                                        train_runs_, t.context, t.positions, t.dilation,
                                        t.in_rows, st));
      continue;
    }
    const CuMatrix<BaseFloat> &dout = time_derivs_[t.dout_level];
    KALDI_ASSERT(time_dviews_[t.dout_level].data != nullptr && dout.NumRows() == t.rows);
    if (t.op == TimeBackLaunch::kEpilogueBwd) {
      CuMatrix<BaseFloat> &din = deriv_of(t.din_level, t.in_rows);
      KALDI_ASSERT(t.in_rows == t.rows + t.dilation * (t.taps - 1));
      const CuSubMatrix<BaseFloat> x = map_at(t.in_level, t.in_rows);
      const bool pool = t.pooled_level >= 0, act = t.act_level >= 0;
      const CuSubMatrix<BaseFloat> pm = map_at(pool ? t.pooled_level : t.in_level, t.rows),
                                   am = map_at(act ? t.act_level : t.in_level, t.rows);
      CuProfileScope prof("kn_timemap_epilogue_bwd");
      CNSL_SAFE_CALL(kn_timemap_epilogue_bwd(
          x.Data(), x.Dim(), pool ? pm.Data() : nullptr, pm.Dim(), act ? am.Data() : nullptr,
          am.Dim(), dout.Data(), dout.Dim(), din.Data(), din.Dim(), t.rows, t.taps,
          pool ? t.pool_channel : 1, t.dilation, st));
      continue;
    }
    // a Convolution: per tap d, the gradient block map_in[delta d ..)^T dout
    // into rows c wc + d wd of the flat gradient, and din[delta d ..) += dout
    // W_d^T with the weights as they stand; then the step
    cnsl::nnet0::ConvolutionComponent *conv = comps_[t.comp].conv;
    KALDI_ASSERT(conv != nullptr);
    const int G = conv->Group(), K = conv->KernelDim();
    CuMatrix<BaseFloat> &grad = time_grads_[t.comp];
    if (grad.NumRows() != 1 || grad.NumCols() != conv->NumGradientParams())
      grad.Resize(1, conv->NumGradientParams(), kUndefined);  // written whole
    const CuSubMatrix<BaseFloat> x = map_at(t.in_level, t.in_rows);
    KALDI_ASSERT(dout.NumCols() == G && x.NumCols() * t.taps == K &&
                 t.in_rows == t.rows + t.dilation * (t.taps - 1));
    for (int d = 0; d < t.taps; d++) {
      const CuSubMatrix<BaseFloat> xd = x.RowRange(t.dilation * d, t.rows);
      CuSubMatrix<BaseFloat> gd(grad.Data() + (int64_t)d * t.wd * G, x.NumCols(), G, t.wc * G);
      gd.AddMatMat(1.0f, xd, kTrans, dout, kNoTrans, 0.0f);
    }
    CuSubVector<BaseFloat> gb(grad.Data() + (size_t)K * G, G);
    gb.AddRowSumMat(1.0f, dout, 0.0f);
    if (t.din_level >= 0) {
      CuMatrix<BaseFloat> &din = deriv_of(t.din_level, t.in_rows);
      din.SetZero();
      const CuMatrix<BaseFloat> &W = conv->LinearParams();
      for (int d = 0; d < t.taps; d++) {
        CuSubMatrix<BaseFloat> dd = din.RowRange(t.dilation * d, t.rows);
        const CuSubMatrix<BaseFloat> wd(const_cast<float *>(W.Data()) + (int64_t)d * t.wd * W.Stride(),
                                        x.NumCols(), G, t.wc * W.Stride());
        dd.AddMatMat(1.0f, dout, kNoTrans, wd, kTrans, 1.0f);
      }
    }
    conv->ApplyGradient(grad.Data(), num_chunks_);
  }
  time_backward_done_ = true;
}

void NnetStack::ComputeProbFrames(const float *feats, MatrixDim dim, const CorpusIndex &corpus,
                                  const int32_t *frames, int num, const int32_t *rows,
                                  const int32_t *cols, const float *weights, int num_labels) {
  FrameList fl = {feats, dim, &corpus, frames, num, nullptr};
  ComputeProbOn(feats, dim, &fl, rows, cols, weights, num_labels,
                "kcnn_nnet_compute_prob_frames");
}

const CuMatrix<BaseFloat> &NnetStack::ComputeExamples(const float *feats, MatrixDim dim,
                                                      const int32_t *examples, int num,
                                                      bool apply_log,
                                                      const double *prior_offsets) {
  const int nc = NumComponents();
  const int count = FusedLoglikes(apply_log) ? nc - 1 : nc;
  // every step emits another row count and every forward kernel writes its
  // whole output: sized as PropagateUtterances sizes them
  if (!cnsl::nnet0::LiteralPath())
    for (int i = 0; i < count; i++) {
      CuMatrix<BaseFloat> &y = out(i).value;
      const int rows = num * (int)out(i).offsets.size(), cols = comps_[i].c->OutputDim();
      if (y.NumRows() != rows || y.NumCols() != cols) y.Resize(rows, cols, kUndefined);
    }
  const FrameList fl = {feats, dim, nullptr, nullptr, num, examples};
  PropagateFirst(feats, dim, count, &fl);
  prob_forward_ = true;
  return Loglikes(apply_log, prior_offsets, num);
}

CuMatrix<BaseFloat> &NnetStack::ExamplesInput(int first, int num) {
  KALDI_ASSERT(first > 0 && first < NumComponents() && num > 0);
  CuMatrix<BaseFloat> &y = out(first - 1).value;
  const int rows = num * (int)out(first - 1).offsets.size(),
            cols = comps_[first - 1].c->OutputDim();
  if (y.NumRows() != rows || y.NumCols() != cols) y.Resize(rows, cols, kUndefined);
  return y;
}

const CuMatrix<BaseFloat> &NnetStack::ComputeExamplesFrom(int first, const float *feats,
                                                          MatrixDim dim, int num,
                                                          bool apply_log,
                                                          const double *prior_offsets) {
  const int nc = NumComponents();
  KALDI_ASSERT(first > 0 && first < nc && comps_[0].splice != nullptr &&
               !cnsl::nnet0::LiteralPath());
  const int count = FusedLoglikes(apply_log) ? nc - 1 : nc;
  for (int i = first; i < count; i++) {  // sized as ComputeExamples sizes them
    CuMatrix<BaseFloat> &y = out(i).value;
    const int rows = num * (int)out(i).offsets.size(), cols = comps_[i].c->OutputDim();
    if (y.NumRows() != rows || y.NumCols() != cols) y.Resize(rows, cols, kUndefined);
  }
  num_chunks_ = num;
  acts_[0].value.Borrow(const_cast<float *>(feats), dim.rows, dim.cols, dim.stride);
  ForgetMinibatch();
  whole_utts_ = time_shared_ = time_train_ = false;
  frames_fused_ = true;  // as after ComputeExamples through a first Splice
  examples_first_ = first;
  for (int i = first; i < count; i++) {
    if (PropagateMaxpoolPair(i) || PropagateReluPair(i)) { i++; continue; }
    ChunkInfo ii = in_info(i), oi = out_info(i);
    auto hint = input_stats(i);
    comps_[i].c->Propagate(ii, oi, in(i).value, &out(i).value);
  }
  prob_forward_ = true;
  return Loglikes(apply_log, prior_offsets, num);
}

const CuMatrix<BaseFloat> &NnetStack::Output(int i) {
  KALDI_ASSERT(i >= -1 && i < NumComponents());
  Activation &a = out(i);
  if (examples_first_ > 0 && i >= 0 && i + 1 < examples_first_)
    KALDI_ERR << "output of component " << i << " was not formed: the streaming step ran "
              << "components 0 to " << examples_first_ - 1 << " as time maps";
  if (time_shared_ && i >= 0 && i + 1 < (int)time_views_.size())
    KALDI_ERR << "output of component " << i << " was not formed: "
              << (time_train_ ? "kcnn_nnet_propagate_frames_shared" : "kcnn_nnet_compute_shared")
              << " ran components 0 to " << time_views_.size() - 1 << " as time maps; see "
              << "kcnn_nnet_time_map";
  if (a.stale == kGone)
    KALDI_ERR << "output of component " << i << " was not stored (fused with the "
              << "next Maxpool, kcnn_set_fusion(1)) and its backprop has run; "
              << "use kcnn_set_fusion(2) to keep it";
  if (a.stale == kRecomputable) {
    // a fused conv's output, or the last Softmax's after ComputeProb: run its
    // Propagate (which sizes the matrix) now
    comps_[i].c->Propagate(in_info(i), out_info(i), in(i).value, &a.value);
    a.stale = kStored;
  }
  return a.value;
}

// A deferred pool Backprop (Comp::deriv_deferred), run now.
void NnetStack::MaterialisePoolDeriv(int i) {
  Comp &c = comps_[i];
  KALDI_ASSERT(c.pool != NULL && c.mask_valid && i + 1 < NumComponents());
  c.pool->BackpropFromMask(static_cast<unsigned char *>(c.mask.p), c.pool->OutputDim(),
                           out_deriv_of(i, nullptr, MatrixDim()), &c.deriv);
  c.deriv_deferred = false;
}

const CuMatrix<BaseFloat> &NnetStack::InputDeriv(int i) {
  KALDI_ASSERT(i >= 0 && i < NumComponents());
  RequireAbovePrefix(i, "kcnn_nnet_input_deriv");
  if (i == 0 && frames_fused_)
    KALDI_ERR << "input derivative of component 0: after kcnn_nnet_propagate_frames a first "
              << "SpliceComponent reads the corpus itself and its Backprop is not run (it has "
              << "no parameters, and examples share corpus rows)";
  if (comps_[i].deriv_deferred) MaterialisePoolDeriv(i);
  return comps_[i].deriv;
}

void NnetStack::BackpropComponent(int i, const float *out_deriv, MatrixDim od_dim,
                                  BackpropMode mode, float *grad, bool skip_first_dx) {
  const int nc = NumComponents();
  KALDI_ASSERT(i >= 0 && i < nc);
  RequireTrainingForward("kcnn_nnet_backprop_component");
  RequireLastNotFused(i, "kcnn_nnet_backprop_component");
  RequireAbovePrefix(i, "kcnn_nnet_backprop_component");
  // a first Splice that gathered from the corpus: nothing to update, and its
  // input derivative would be a window matrix of rows that examples share
  if (i == 0 && frames_fused_) return;
  Comp &c = comps_[i];
  auto hint = input_stats(i);
  if (out(i).stale == kRecomputable) out(i).stale = kGone;
  const CuMatrix<BaseFloat> &x = in(i).value, &y = out(i).value;
  const bool pool_above_deferred = i + 1 < nc && comps_[i + 1].deriv_deferred;
  CuMatrix<BaseFloat> *dx = &c.deriv;
  if (i == 0 && skip_first_dx && c.updatable) dx = nullptr;
  if (mode == kGradientOnly) {
    KALDI_ASSERT(c.updatable != NULL && grad != NULL && !pool_above_deferred && !c.mask_valid);
    c.updatable->BackpropGradient(in_info(i), out_info(i), x, y,
                                  out_deriv_of(i, out_deriv, od_dim), nullptr, grad);
    return;
  }
  if (pool_above_deferred) {  // the pool above left its Backprop here
    const Comp &p = comps_[i + 1];
    if (c.conv && p.pool &&
        c.conv->BackpropPooled(x, *p.pool, static_cast<unsigned char *>(p.mask.p),
                               p.pool->OutputDim(), out_deriv_of(i + 1, out_deriv, od_dim),
                               to_update(c, mode), dx, mode == kGradient ? grad : nullptr))
      return;
    MaterialisePoolDeriv(i + 1);
  }
  CuSubMatrix<BaseFloat> od = out_deriv_of(i, out_deriv, od_dim);
  ChunkInfo ii = in_info(i), oi = out_info(i);
  if (mode == kGradient && c.updatable) {
    c.updatable->BackpropGradient(ii, oi, x, y, od, dx, grad);
    return;
  }
  if (c.mask_valid) {  // pool of a fused pair: route through its mask
    KALDI_ASSERT(c.pool != NULL);
    // fusion mode 1, not the last component: left to the conv below, which
    // builds its out_deriv from od and the mask slab by slab
    if (g_fusion == 1 && i < nc - 1 && c.pool->FoldsIntoConvBackprop()) {
      c.deriv_deferred = true;
      return;
    }
    c.pool->BackpropFromMask(static_cast<unsigned char *>(c.mask.p), c.pool->OutputDim(), od,
                             dx);
    return;
  }
  c.c->Backprop(ii, oi, x, y, od, to_update(c, mode), dx);
}

void NnetStack::BackpropSplit(int i, const float *out_deriv, MatrixDim od_dim, float *grad,
                              bool skip_first_dx, void (*between)(void *), void *ctx) {
  const int nc = NumComponents();
  KALDI_ASSERT(i >= 0 && i < nc && grad != NULL);
  RequireTrainingForward("kcnn_nnet_backprop_split");
  RequireLastNotFused(i, "kcnn_nnet_backprop_split");
  RequireAbovePrefix(i, "kcnn_nnet_backprop_split");
  Comp &c = comps_[i];
  if (c.affine == NULL) KALDI_ERR << "kcnn_nnet_backprop_split: component " << i << " is not affine";
  KALDI_ASSERT(!(i + 1 < nc && comps_[i + 1].deriv_deferred) && !c.mask_valid);
  auto hint = input_stats(i);
  if (out(i).stale == kRecomputable) out(i).stale = kGone;
  const CuMatrix<BaseFloat> &x = in(i).value, &y = out(i).value;
  CuSubMatrix<BaseFloat> od = out_deriv_of(i, out_deriv, od_dim);
  CuMatrix<BaseFloat> *dx = (i == 0 && skip_first_dx) ? nullptr : &c.deriv;
  ChunkInfo ii = in_info(i), oi = out_info(i);
  CuGemmBackpropStats stats(od, c.affine->LinearParams(), true, &x);
  c.affine->BackpropGradient(ii, oi, x, y, od, nullptr, grad);
  if (between) between(ctx);
  if (dx) c.c->Backprop(ii, oi, x, y, od, to_update(c, kDataOnly), dx);
}

void NnetStack::Backprop(const float *out_deriv, MatrixDim od_dim) {
  // after PropagateFramesShared the prefix runs once, over its time maps
  const int stop = time_train_ ? train_plan_.prefix() : 0;
  for (int i = NumComponents() - 1; i >= stop; i--)
    BackpropComponent(i, out_deriv, od_dim, kUpdate, nullptr, false);
  if (time_train_) BackpropTimeMaps();
}

double *NnetStack::objf_totals() {
  kaldi::CuBuffer &t = labels_.totals;
  if (!t.p)
    CU_SAFE_CALL(hipMemsetAsync(t.reserve(2 * sizeof(double)), 0, 2 * sizeof(double),
                                CuDevice::Instantiate().Stream()));
  return static_cast<double *>(t.p);
}

const char *NnetStack::LabelStaging::Stage(const int32_t *rows, const int32_t *cols,
                                           const float *weights, int num, int num_rows,
                                           hipStream_t st) {
  const size_t bytes = label_layout(num, num_rows).bytes;
  stage_labels(rows, cols, weights, num, num_rows, Begin(bytes));
  return Commit(bytes, st);
}

char *NnetStack::LabelStaging::Begin(size_t bytes) {
  if (copied == nullptr)
    CU_SAFE_CALL(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
  else
    CU_SAFE_CALL(hipEventSynchronize(copied));  // the last copy has left the buffer
  if (host_bytes < bytes) {
    if (host) CU_SAFE_CALL(hipHostFree(host));
    host = nullptr;
    host_bytes = 0;
    CU_SAFE_CALL(hipHostMalloc(&host, bytes, hipHostMallocDefault));
    host_bytes = bytes;
  }
  return static_cast<char *>(host);
}

const char *NnetStack::LabelStaging::Commit(size_t bytes, hipStream_t st) {
  dev.reserve(bytes);
  CU_SAFE_CALL(hipMemcpyAsync(dev.p, host, bytes, hipMemcpyHostToDevice, st));
  CU_SAFE_CALL(hipEventRecord(copied, st));
  return static_cast<const char *>(dev.p);
}

int NnetStack::XentDeriv(const int32_t *rows, const int32_t *cols, const float *weights,
                         int num, const float **out_deriv, MatrixDim *od_dim,
                         const char *who) {
  const int nc = NumComponents();
  RequireTrainingForward(who);
  const Comp &last = comps_[nc - 1];
  const CuMatrix<BaseFloat> &y = out(nc - 1).value;
  const int N = y.NumRows(), dim = last.c->OutputDim();
  if (N == 0 || y.NumCols() != dim) KALDI_ERR << who << ": no Propagate ran";
  if (num > 0 && weights == nullptr) KALDI_ERR << who << ": bad label arrays";
  // every check before any launch
  const std::string bad = check_labels(rows, cols, num, N, dim, true);
  if (!bad.empty()) KALDI_ERR << who << ": " << bad;
  const DeviceLabels lab = StageLabels(rows, cols, weights, num, N);
  const int32_t *d_start = lab.row_start, *d_row = lab.row, *d_col = lab.col;
  const float *d_w = lab.weight;
  double *tot = objf_totals();
  if (last.softmax != nullptr && !cnsl::nnet0::LiteralPath()) {
    // zeroed derivative + CompObjfAndDeriv + the Softmax's Backprop, fused
    last.softmax->BackpropXent(y, d_start, d_col, d_w, tot, last.softmax,
                               &comps_[nc - 1].deriv);
    xent_fused_ = true;
    *out_deriv = nullptr;
    *od_dim = MatrixDim{0, 0, 0};
    return nc - 2;
  }
  // NnetUpdater::ComputeObjfAndDeriv: a zeroed [rows x OutputDim] matrix,
  // CompObjfAndDeriv against the last output; Backprop follows
  xent_deriv_.Resize(N, dim, kSetZero);
  if (num > 0)
    comp_objf_and_deriv(d_row, d_col, d_w, num, y.Data(), y.Dim(), xent_deriv_.Data(),
                        xent_deriv_.Dim(), tot);
  *out_deriv = xent_deriv_.Data();
  *od_dim = xent_deriv_.Dim();
  return nc - 1;
}

void NnetStack::BackpropXent(const int32_t *rows, const int32_t *cols, const float *weights,
                             int num, bool skip_first_dx) {
  const float *od = nullptr;
  MatrixDim od_dim = {0, 0, 0};
  const int first =
      XentDeriv(rows, cols, weights, num, &od, &od_dim, "kcnn_nnet_backprop_xent");
  const int stop = time_train_ ? train_plan_.prefix() : 0;
  for (int i = first; i >= stop; i--)
    BackpropComponent(i, od, od_dim, kUpdate, nullptr, skip_first_dx);
  if (time_train_) BackpropTimeMaps();
  // the whole backward has run: the last component is the caller's again
  xent_fused_ = false;
}

void NnetStack::SkipDropoutCall() {
  for (Comp &c : comps_)
    if (DropoutComponent *d = dynamic_cast<DropoutComponent *>(c.c.get())) d->SkipCall();
}

void NnetStack::SetRowOffset(uint64_t offset) {
  for (Comp &c : comps_)
    if (DropoutComponent *d = dynamic_cast<DropoutComponent *>(c.c.get()))
      d->SetRowOffset(offset);
}

// The list -> pinned staging buffer -> device, on the library's stream.
NnetStack::DeviceLabels NnetStack::StageLabels(const int32_t *rows, const int32_t *cols,
                                               const float *weights, int num, int num_rows) {
  const LabelLayout lay = label_layout(num, num_rows);
  const char *base =
      labels_.Stage(rows, cols, weights, num, num_rows, CuDevice::Instantiate().Stream());
  DeviceLabels d;
  d.row_start = reinterpret_cast<const int32_t *>(base + lay.row_start);
  d.row = reinterpret_cast<const int32_t *>(base + lay.row);
  d.col = reinterpret_cast<const int32_t *>(base + lay.col);
  d.weight = reinterpret_cast<const float *>(base + lay.weight);
  return d;
}

void NnetStack::RequireTrainingForward(const char *who) const {
  if (prob_forward_)
    KALDI_ERR << who << ": the last forward pass was kcnn_nnet_compute_prob's or "
              << "kcnn_nnet_compute's, which keep nothing for a backprop; run "
              << "kcnn_nnet_propagate first";
}

void NnetStack::RequireAbovePrefix(int i, const char *who) const {
  if (time_train_ && i < train_plan_.prefix())
    KALDI_ERR << who << ": component " << i << " is one of the " << train_plan_.prefix()
              << " that kcnn_nnet_propagate_frames_shared ran as time maps; their backward runs "
              << "once, over the maps, in kcnn_nnet_backprop / kcnn_nnet_backprop_xent";
}

void NnetStack::RequireLastNotFused(int i, const char *who) const {
  if (xent_fused_ && i == NumComponents() - 1)
    KALDI_ERR << who << ": kcnn_nnet_xent_deriv has already written the last "
              << "SoftmaxComponent's input derivative from the labels; start the backward at "
              << "the component it returned (" << i - 1 << ")";
}

double *NnetStack::prob_totals() {
  if (!prob_totals_.p)
    CU_SAFE_CALL(hipMemsetAsync(prob_totals_.reserve(3 * sizeof(double)), 0, 3 * sizeof(double),
                                CuDevice::Instantiate().Stream()));
  return static_cast<double *>(prob_totals_.p);
}

void NnetStack::ComputeProb(const float *input, MatrixDim in_dim, const int32_t *rows,
                            const int32_t *cols, const float *weights, int num) {
  ComputeProbOn(input, in_dim, nullptr, rows, cols, weights, num, "kcnn_nnet_compute_prob");
}

void NnetStack::ComputeProbOn(const float *input, MatrixDim in_dim, FrameList *fl,
                              const int32_t *rows, const int32_t *cols, const float *weights,
                              int num, const char *who) {
  const int nc = NumComponents();
  const Comp &last = comps_[nc - 1];
  // every check before any launch
  const int N = fl ? CheckFrames(*fl, who)
                   : checked_num_chunks(in_dim, comps_[0].c->InputDim(),
                                        (int)acts_[0].offsets.size());
  const int dim = last.c->OutputDim();
  if (num > 0 && weights == nullptr) KALDI_ERR << who << ": bad label arrays";
  const std::string bad = check_labels(rows, cols, num, N, dim, true);
  if (!bad.empty()) KALDI_ERR << who << ": " << bad;
  const bool fused = last.softmax != nullptr && !cnsl::nnet0::LiteralPath();
  // The labels go first: staging waits for the last call's copy to have left
  // the pinned buffer, and behind the forward pass that wait would be for the
  // whole of the last call, every call.  (The examples before them.)
  if (fl) StageFrames(fl);
  const DeviceLabels lab = StageLabels(rows, cols, weights, num, N);
  PropagateFirst(input, in_dim, fused ? nc - 1 : nc, fl);
  prob_forward_ = true;
  if (fused) out(nc - 1).stale = kRecomputable;  // the Softmax did not run
  // the matrix the sums are taken from: the Softmax's input, or the last output
  const CuMatrix<BaseFloat> &x = fused ? in(nc - 1).value : out(nc - 1).value;
  KALDI_ASSERT(x.NumRows() == N && x.NumCols() == dim);
  double *tot = prob_totals();
  CuScratch ws(kn_prob_ws(kn_prob_blocks(x.Dim())));
  const kcnn_stream_t st = reinterpret_cast<kcnn_stream_t>(CuDevice::Instantiate().Stream());
  if (fused) {
    CuProfileScope prof("kn_softmax_objf_accuracy");
    CNSL_SAFE_CALL(kn_softmax_objf_accuracy(x.Data(), x.Dim(), lab.row_start, lab.col,
                                            lab.weight, tot, ws.p, st));
  } else {
    CuProfileScope prof("kn_objf_accuracy");
    CNSL_SAFE_CALL(
        kn_objf_accuracy(x.Data(), x.Dim(), lab.row_start, lab.col, lab.weight, tot, ws.p, st));
  }
}

int NnetStack::LeftContext() const {
  int left = 0;
  for (const Comp &c : comps_) left -= c.c->Context().front();
  return left;
}

int NnetStack::RightContext() const {
  int right = 0;
  for (const Comp &c : comps_) right += c.c->Context().back();
  return right;
}

// The clamped frames of a padded pass laid out by a one-slot Splice: an
// utterance of T frames gets T + ext rows of padded_input_, `left` copies of
// its first frame in front.
void NnetStack::LayOutClamped(const float *input, MatrixDim in_dim, const int32_t *utt_start,
                              int num_utts, int total, int ext, int left) {
  size_output(&padded_input_, total + num_utts * ext, in_dim.cols);
  kn_ragged_splice_geom g;
  g.num_utts = num_utts;
  g.total = total;
  g.in_ext = 0;
  g.out_ext = ext;
  g.shift = g.const_shift = -left;
  g.dim = in_dim.cols;
  g.const_dim = 0;
  g.num_splice = 1;
  g.context[0] = 0;
  CuProfileScope prof("kn_splice_ragged_prop");
  CNSL_SAFE_CALL(kn_splice_ragged_prop(
      input, in_dim, padded_input_.Data(), padded_input_.Dim(), utt_start, g,
      reinterpret_cast<kcnn_stream_t>(CuDevice::Instantiate().Stream())));
}

void NnetStack::PropagateUtterances(const float *input, MatrixDim in_dim,
                                    const int32_t *utt_start, int num_utts, int total,
                                    bool pad_input, int count, int first) {
  const int nc = NumComponents();
  // an activation's extra rows per utterance: the contexts still to come
  int ext = 0;
  acts_[nc].utt_ext = 0;
  for (int k = nc; k-- > 0;) {
    const std::vector<int32> ctx = comps_[k].c->Context();
    ext += ctx.back() - ctx.front();
    acts_[k].utt_ext = ext;
  }
  for (Activation &a : acts_) a.utt_rows = total + num_utts * a.utt_ext;
  const int left = LeftContext();
  // the caller's frames alone feed a first Splice, which clamps its reads
  const bool clamp_in_splice = pad_input && ext > 0 && comps_[0].splice != nullptr;
  if (clamp_in_splice) acts_[0].utt_rows = in_dim.rows;
  ForgetMinibatch();
  prob_forward_ = whole_utts_ = true;
  frames_fused_ = false;
  examples_first_ = 0;
  time_shared_ = first > 0;
  time_train_ = false;
  if (first > 0) {
    // the time maps have run and the gather has written component first's input
    acts_[0].value.Borrow(const_cast<float *>(input), in_dim.rows, in_dim.cols, in_dim.stride);
  } else if (pad_input && ext > 0 && !clamp_in_splice) {
    // component 0 is row-wise: the clamped frames laid out by a one-slot Splice
    LayOutClamped(input, in_dim, utt_start, num_utts, total, ext, left);
    acts_[0].value.Borrow(padded_input_.Data(), padded_input_.NumRows(),
                          padded_input_.NumCols(), padded_input_.Stride());
  } else {
    acts_[0].value.Borrow(const_cast<float *>(input), in_dim.rows, in_dim.cols, in_dim.stride);
  }
  KALDI_ASSERT(first > 0 || acts_[0].value.NumRows() == acts_[0].utt_rows);
  // Every batch of utterances has another row count, and every forward kernel
  // writes its whole output: the outputs are sized here without the zero fill
  // of Component::Propagate's Resize (at 26438 rows of nnet.config that fill
  // is 1.7 ms of an 11.2 ms call, profiles/compute.md).  The literal path
  // keeps the reference's zeroing Resize.
  if (!cnsl::nnet0::LiteralPath())
    for (int i = first; i < count; i++) {
      CuMatrix<BaseFloat> &y = out(i).value;
      if (y.NumRows() != out(i).utt_rows || y.NumCols() != comps_[i].c->OutputDim())
        y.Resize(out(i).utt_rows, comps_[i].c->OutputDim(), kUndefined);
    }
  for (int i = first; i < count; i++) {
    if (const SpliceComponent *splice = comps_[i].splice) {
      const bool clamp = i == 0 && clamp_in_splice;
      size_output(&out(i).value, out(i).utt_rows, splice->OutputDim());
      splice->PropagateRagged(in(i).value, &out(i).value, utt_start, num_utts, total,
                              clamp ? 0 : in(i).utt_ext, out(i).utt_ext, clamp ? left : 0);
      continue;
    }
    if (PropagateMaxpoolPair(i) || PropagateReluPair(i)) { i++; continue; }
    ChunkInfo ii = in_info(i), oi = out_info(i);
    auto hint = input_stats(i);
    comps_[i].c->Propagate(ii, oi, in(i).value, &out(i).value);
  }
}

const CuMatrix<BaseFloat> &NnetStack::Compute(const float *input, MatrixDim in_dim,
                                              const int32_t *lengths, int num_utts,
                                              bool pad_input, const float *priors,
                                              int num_priors, float prior_scale,
                                              bool apply_log) {
  return ComputeOn(input, in_dim, lengths, num_utts, pad_input, priors, num_priors, prior_scale,
                   apply_log, false, "kcnn_nnet_compute");
}

const CuMatrix<BaseFloat> &NnetStack::ComputeShared(const float *input, MatrixDim in_dim,
                                                    const int32_t *lengths, int num_utts,
                                                    bool pad_input, const float *priors,
                                                    int num_priors, float prior_scale,
                                                    bool apply_log) {
  return ComputeOn(input, in_dim, lengths, num_utts, pad_input, priors, num_priors, prior_scale,
                   apply_log, true, "kcnn_nnet_compute_shared");
}

const CuMatrix<BaseFloat> &NnetStack::ComputeOn(const float *input, MatrixDim in_dim,
                                                const int32_t *lengths, int num_utts,
                                                bool pad_input, const float *priors,
                                                int num_priors, float prior_scale,
                                                bool apply_log, bool share_time,
                                                const char *who) {
  const int nc = NumComponents();
  const Comp &last = comps_[nc - 1];
  const int dim = last.c->OutputDim();
  const int context = LeftContext() + RightContext();
  // every check before any launch
  if (lengths == nullptr || num_utts < 1) KALDI_ERR << who << ": no utterances";
  if (in_dim.cols != comps_[0].c->InputDim())
    KALDI_ERR << who << ": input of " << in_dim.cols << " columns for a network of "
              << comps_[0].c->InputDim();
  const int min_len = pad_input ? 1 : context + 1;
  int64_t sum = 0, total = 0;  // input rows, result rows
  for (int u = 0; u < num_utts; u++) {
    if (lengths[u] < min_len)
      KALDI_ERR << who << ": utterance " << u << " has " << lengths[u]
                << " frames; at least " << min_len << " are needed"
                << (pad_input ? "" : " without pad_input");
    sum += lengths[u];
    total += pad_input ? lengths[u] : lengths[u] - context;
  }
  if (sum != in_dim.rows)
    KALDI_ERR << who << ": the lengths sum to " << sum << ", the input has "
              << in_dim.rows << " rows";
  if (total + (int64_t)num_utts * context >= ((int64_t)1 << 31))
    KALDI_ERR << who << ": too many rows";
  CheckPriors(priors, num_priors, apply_log, who);
  // the time maps' rows, when the leading components run as time maps (a
  // stack the plan declines takes Compute's own pass)
  TimePlan plan;
  TimeRows rows;
  if (share_time) plan = TimeSharedPlan();
  if (plan.prefix() > 0) {
    const std::string bad = plan_time_rows(plan, lengths, num_utts, pad_input, &rows);
    if (!bad.empty()) KALDI_ERR << who << ": " << bad;
    KALDI_ASSERT(rows.result_rows == total && rows.input_rows == total + (int64_t)num_utts * context);
  }
  // The starts of the utterances' result rows and the fp64 prior offsets, in
  // one staged image (first, as ComputeProb stages its labels first).
  const size_t off_at = ((size_t)(num_utts + 1) * sizeof(int32_t) + 7) / 8 * 8;
  const size_t bytes = off_at + (priors ? (size_t)dim * sizeof(double) : 0);
  char *image = utts_.Begin(bytes);
  int32_t *starts = reinterpret_cast<int32_t *>(image);
  starts[0] = 0;
  for (int u = 0; u < num_utts; u++)
    starts[u + 1] = starts[u] + (pad_input ? lengths[u] : lengths[u] - context);
  if (priors) {
    double *off = reinterpret_cast<double *>(image + off_at);
    for (int c = 0; c < dim; c++) off[c] = (double)prior_scale * log((double)priors[c]);
  }
  const char *base = utts_.Commit(bytes, CuDevice::Instantiate().Stream());
  const int32_t *d_starts = reinterpret_cast<const int32_t *>(base);
  const double *d_off = priors ? reinterpret_cast<const double *>(base + off_at) : nullptr;

  if (plan.prefix() > 0)
    PropagateTimeShared(input, in_dim, d_starts, num_utts, (int)total, pad_input, plan, rows);
  PropagateUtterances(input, in_dim, d_starts, num_utts, (int)total, pad_input,
                      FusedLoglikes(apply_log) ? nc - 1 : nc, plan.prefix());
  return Loglikes(apply_log, d_off, (int)total);
}

TimePlan NnetStack::TimeSharedPlan() const {
  std::vector<TimeComp> desc(comps_.size());
  for (size_t i = 0; i < comps_.size(); i++) {
    const Comp &c = comps_[i];
    TimeComp &t = desc[i];
    const std::vector<int32> ctx = c.c->Context();
    t.input_dim = c.c->InputDim();
    t.output_dim = c.c->OutputDim();
    t.left = -ctx.front();
    t.right = ctx.back();
    if (c.splice) {
      t.kind = TimeComp::kSplice;
      t.contiguous = ctx.back() - ctx.front() + 1 == (int32)ctx.size();
      t.const_dim = c.splice->ConstComponentDim();
    } else if (c.conv) {
      t.kind = TimeComp::kConv;
      t.in_height = c.conv->In_height();
      t.in_width = c.conv->In_width();
      t.in_channel = c.conv->In_channels();
      t.kernel_height = c.conv->Kernel_height();
      t.kernel_width = c.conv->Kernel_width();
      t.stride = c.conv->Stride();
      t.pad_height = c.conv->In_pad_height();
      t.pad_width = c.conv->In_pad_width();
      t.group = c.conv->Group();
      t.out_height = c.conv->Out_height();
      t.out_width = c.conv->Out_width();
    } else if (c.pool) {
      t.kind = TimeComp::kPool;
      t.in_height = c.pool->In_height();
      t.in_width = c.pool->In_width();
      t.in_channel = c.pool->In_channels();
      t.pool_height = c.pool->Pool_height_dim();
      t.pool_width = c.pool->Pool_width_dim();
      t.pool_channel = c.pool->Pool_channel_dim();
      t.overlap = c.pool->Overlapping();
    } else if (c.relu) {
      t.kind = TimeComp::kRelu;
    }
  }
  return make_time_plan(desc, cnsl::nnet0::LiteralPath(), true);
}

NnetStack::TimeMapInfo NnetStack::TimeMap(int level) const {
  if (!time_shared_)
    KALDI_ERR << "kcnn_nnet_time_map: the last forward pass was not kcnn_nnet_compute_shared's "
              << "over time maps";
  if (level < 0 || level >= (int)time_views_.size())
    KALDI_ERR << "kcnn_nnet_time_map: level " << level << " outside [0, " << time_views_.size()
              << ")";
  return time_views_[level];
}

// The components the plan covers as time maps (time-plan.h), then the gather
// into component plan.prefix()'s input; `rows` has been checked.
void NnetStack::PropagateTimeShared(const float *input, MatrixDim in_dim,
                                    const int32_t *utt_start, int num_utts, int total,
                                    bool pad_input, const TimePlan &plan, const TimeRows &rows) {
  const int p = plan.prefix();
  const int context = plan.levels[0].positions - 1;
  time_views_.assign((size_t)p, TimeMapInfo());
  auto view_of = [&](int l, const float *data, MatrixDim dim) {
    const TimeLevel &lev = plan.levels[l];
    time_views_[l] = TimeMapInfo{data, dim, lev.channels, lev.positions, lev.dilation, lev.height};
  };
  // level 0: the frames themselves, clamped when padded
  if (pad_input && context > 0) {
    LayOutClamped(input, in_dim, utt_start, num_utts, total, context, LeftContext());
    view_of(0, padded_input_.Data(), padded_input_.Dim());
  } else {
    view_of(0, input, in_dim);
  }
  KALDI_ASSERT(time_views_[0].dim.rows == rows.input_rows);
  FormTimeLevels(plan, rows, utt_start, num_utts, total);
}

void NnetStack::FormTimeLevels(const TimePlan &plan, const TimeRows &rows, const int32_t *starts,
                               int num_starts, int total) {
  const int p = plan.prefix();
  auto view_of = [&](int l, const float *data, MatrixDim dim) {
    const TimeLevel &lev = plan.levels[l];
    time_views_[l] = TimeMapInfo{data, dim, lev.channels, lev.positions, lev.dilation, lev.height};
  };
  const TimeLevel &top = plan.levels[p - 1];
  CuMatrix<BaseFloat> &y = out(p - 1).value;
  const int top_dim = top.width * top.positions;
  KALDI_ASSERT(comps_[p - 1].c->OutputDim() == top_dim);
  if (y.NumRows() != total || y.NumCols() != top_dim)
    y.Resize(total, top_dim, kUndefined);  // written whole
  // a level's own map, sized as Compute sizes its outputs: without the fill
  auto map_of = [&](int l, int r, MatrixDim *dim) {
    CuMatrix<BaseFloat> &m = time_maps_[l];
    const int c = plan.levels[l].width;
    if (m.NumRows() != r || m.NumCols() != c) m.Resize(r, c, kUndefined);
    view_of(l, m.Data(), *dim = m.Dim());
    return m.Data();
  };
  RunTimeSchedule(time_schedule(plan, rows, kUtteranceRoute), time_views_[0].data,
                  time_views_[0].dim, map_of, &y, starts, num_starts);
}

void NnetStack::RunTimeSchedule(const std::vector<TimeLaunch> &sched, const float *in0,
                                MatrixDim in0_dim, const TimeMapFn &map_of,
                                CuMatrix<BaseFloat> *y, const int32_t *d_starts, int num_starts) {
  const kcnn_stream_t st = reinterpret_cast<kcnn_stream_t>(CuDevice::Instantiate().Stream());
  struct View { float *data; MatrixDim dim; };
  std::vector<View> views((size_t)sched.back().in_level + 1, View{nullptr, {0, 0, 0}});
  views[0] = View{const_cast<float *>(in0), in0_dim};
  auto form = [&](int l, int rows) {  // level l's map from the caller; -1: no map
    if (l >= 0) views[(size_t)l].data = map_of(l, rows, &views[(size_t)l].dim);
    return l >= 0 ? views[(size_t)l] : View{nullptr, {0, 0, 0}};
  };
  for (const TimeLaunch &t : sched) {
    View in = views[(size_t)t.in_level];
    KALDI_ASSERT(in.data != nullptr);
    in.dim.rows = t.in_rows;
    const View m = form(t.out_level, t.rows), act = form(t.act_level, t.rows);
    const View &o = m.data ? m : act;  // where a convolution stores
    cnsl::nnet0::ConvolutionComponent *conv = comps_[t.comp].conv;
    KALDI_ASSERT(conv != nullptr || t.op > TimeLaunch::kConv2d);
    const CuMatrix<BaseFloat> *W = conv ? &conv->LinearParams() : nullptr;
    if (t.op == TimeLaunch::kConvTaps) {
      // tap d: map'[rows] (+)= map[rows + delta d] W_d, GEMMs of the matrix layer
      CuSubMatrix<BaseFloat> out(o.data, t.rows, o.dim.cols, o.dim.stride);
      for (int d = 0; d < t.taps; d++) {
        CuSubMatrix<BaseFloat> a(in.data + (int64_t)t.dilation * d * in.dim.stride, t.rows,
                                 in.dim.cols, in.dim.stride);
        CuSubMatrix<BaseFloat> wd(const_cast<float *>(W->Data()) + (int64_t)d * t.wd * W->Stride(),
                                  in.dim.cols, o.dim.cols, t.wc * W->Stride());
        if (d == 0)
          out.AddMatMatBias(1.0f, a, kNoTrans, wd, kNoTrans, conv->BiasParams());
        else
          out.AddMatMat(1.0f, a, kNoTrans, wd, kNoTrans, 1.0f);
      }
    } else if (t.op == TimeLaunch::kConv) {
      CuProfileScope prof("kn_timemap_conv");
      CNSL_SAFE_CALL(kn_timemap_conv(in.data, in.dim, W->Data(), W->Dim(),
                                     conv->BiasParams().Data(), o.data, o.dim, t.rows, t.taps,
                                     t.dilation, t.wc, t.wd, t.relu, st));
    } else if (t.op == TimeLaunch::kConv2d) {
      CuProfileScope prof("kn_timemap_conv2d");
      CNSL_SAFE_CALL(kn_timemap_conv2d(in.data, in.dim, W->Data(), W->Dim(),
                                       conv->BiasParams().Data(), o.data, o.dim, t.rows, t.height,
                                       t.channels, t.kernel_height, t.taps, t.dilation, t.relu,
                                       st));
    } else if (t.op == TimeLaunch::kPool2d) {
      CuProfileScope prof("kn_timemap_pool2d");
      CNSL_SAFE_CALL(kn_timemap_pool2d(in.data, in.dim, m.data, m.dim, act.data, act.dim, t.rows,
                                       t.height, t.pool_height, t.taps, t.pool_channel,
                                       t.dilation, st));
    } else if (t.op == TimeLaunch::kEpilogue) {
      CuProfileScope prof("kn_timemap_epilogue");
      CNSL_SAFE_CALL(kn_timemap_epilogue(in.data, in.dim, m.data, m.dim, act.data, act.dim,
                                         t.rows, t.taps, t.pool_channel, t.dilation, st));
    } else if (t.op == TimeLaunch::kGather) {
      CuProfileScope prof("kn_timemap_gather");
      CNSL_SAFE_CALL(kn_timemap_gather(in.data, in.dim, y->Data(), y->Dim(), d_starts,
                                       num_starts, t.context, t.positions, t.dilation, st));
    } else {
      CuProfileScope prof("kn_timemap_gather2d");
      CNSL_SAFE_CALL(kn_timemap_gather2d(in.data, in.dim, y->Data(), y->Dim(), d_starts,
                                         num_starts, t.context, t.height, t.positions,
                                         t.dilation, st));
    }
  }
}

void NnetStack::CheckPriors(const float *priors, int num_priors, bool apply_log,
                            const char *who) const {
  if (priors == nullptr) return;
  const int dim = OutputDim();
  if (!apply_log) KALDI_ERR << who << ": priors without apply_log are not supported";
  if (num_priors != dim)
    KALDI_ERR << who << ": " << num_priors << " priors for " << dim << " outputs";
  for (int c = 0; c < dim; c++)
    if (!(priors[c] > 0.0f) || !std::isfinite(priors[c]))
      KALDI_ERR << who << ": prior " << c << " is " << priors[c]
                << "; priors must be finite and > 0";
}

bool NnetStack::FusedLoglikes(bool apply_log) const {
  return apply_log && comps_.back().softmax != nullptr && !cnsl::nnet0::LiteralPath();
}

const CuMatrix<BaseFloat> &NnetStack::Loglikes(bool apply_log, const double *d_off, int total) {
  const int nc = NumComponents(), dim = OutputDim();
  if (!apply_log) return out(nc - 1).value;
  const kcnn_stream_t st = reinterpret_cast<kcnn_stream_t>(CuDevice::Instantiate().Stream());
  if (loglikes_.NumRows() != total || loglikes_.NumCols() != dim)
    loglikes_.Resize(total, dim, kUndefined);  // written whole
  if (FusedLoglikes(apply_log)) {
    out(nc - 1).stale = kRecomputable;  // the Softmax did not run
    const CuMatrix<BaseFloat> &x = in(nc - 1).value;
    KALDI_ASSERT(x.NumRows() == total && x.NumCols() == dim);
    CuProfileScope prof("kn_softmax_loglikes");
    CNSL_SAFE_CALL(
        kn_softmax_loglikes(x.Data(), x.Dim(), loglikes_.Data(), loglikes_.Dim(), d_off, st));
  } else {
    const CuMatrix<BaseFloat> &p = out(nc - 1).value;
    KALDI_ASSERT(p.NumRows() == total && p.NumCols() == dim);
    CuProfileScope prof("kn_loglikes");
    CNSL_SAFE_CALL(
        kn_loglikes(p.Data(), p.Dim(), loglikes_.Data(), loglikes_.Dim(), d_off, st));
  }
  return loglikes_;
}

void NnetStack::ProbTotal(double out[3], bool reset) {
  hipStream_t st = CuDevice::Instantiate().Stream();
  double *tot = prob_totals();
  CU_SAFE_CALL(hipMemcpyAsync(out, tot, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (reset) CU_SAFE_CALL(hipMemsetAsync(tot, 0, 3 * sizeof(double), st));
  CU_SAFE_CALL(hipStreamSynchronize(st));
}

void NnetStack::ObjfTotal(double out[2], bool reset) {
  hipStream_t st = CuDevice::Instantiate().Stream();
  double *tot = objf_totals();
  CU_SAFE_CALL(hipMemcpyAsync(out, tot, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (reset) CU_SAFE_CALL(hipMemsetAsync(tot, 0, 2 * sizeof(double), st));
  CU_SAFE_CALL(hipStreamSynchronize(st));
}

}  // namespace kcnn
