// capi/online-computer.cc -- kcnn::OnlineComputer (online-computer.h).
#include "online-computer.h"

#include <cmath>
#include <string>

#include "../nnet2/nnet-kernels.h"

using namespace kaldi;

namespace kcnn {

namespace {
// the constructor's checks of its numbers, and the state they make
StreamState checked_state(const NnetStack *net, int num_streams, int max_chunk) {
  if (net == nullptr) KALDI_ERR << "kcnn_online_new: no network";
  const int left = net->LeftContext(), right = net->RightContext();
  const std::string bad =
      check_stream_geometry(left, right, max_chunk, num_streams, net->InputDim());
  if (!bad.empty()) KALDI_ERR << "kcnn_online_new: " << bad;
  return StreamState(left, right, max_chunk, num_streams);
}
}  // namespace

OnlineComputer::OnlineComputer(NnetStack *net, int num_streams, int max_chunk,
                               const float *priors, int num_priors, float prior_scale,
                               bool apply_log, bool share_time)
    : share_time_(share_time),
      net_(net),
      state_(checked_state(net, num_streams, max_chunk)),
      apply_log_(apply_log) {
  net_->CheckPriors(priors, num_priors, apply_log, "kcnn_online_new");
  if (priors != nullptr) {  // as Compute forms them
    prior_offsets_.resize((size_t)num_priors);
    for (int c = 0; c < num_priors; c++)
      prior_offsets_[c] = (double)prior_scale * log((double)priors[c]);
  }
  empty_.Borrow(nullptr, 0, net_->OutputDim(), net_->OutputDim());
}

const CuMatrix<BaseFloat> &OnlineComputer::Accept(const float *chunk, MatrixDim dim,
                                                  const int32_t *streams, const int32_t *num_new,
                                                  const int32_t *final, int num,
                                                  int32_t *num_out) {
  const char *who = "kcnn_online_accept";
  const int cols = net_->InputDim();
  // every check before any launch and any change of a slot
  if (num > 0 && num_out == nullptr) KALDI_ERR << who << ": no num_out";
  if (dim.rows < 0) KALDI_ERR << who << ": a chunk of " << dim.rows << " rows";
  if (dim.rows > 0) {
    if (chunk == nullptr) KALDI_ERR << who << ": no chunk";
    if (dim.cols != cols)
      KALDI_ERR << who << ": a chunk of " << dim.cols << " columns for a network of " << cols;
    if (dim.stride < dim.cols)
      KALDI_ERR << who << ": a row stride of " << dim.stride << " for " << dim.cols << " columns";
  }
  const StreamStep step = {streams, num_new, final, num, dim.rows};
  StepTotals totals;
  const std::string bad = state_.Check(step, &totals);
  if (!bad.empty()) KALDI_ERR << who << ": " << bad;
  if (totals.out_rows > 0) net_->CheckExamples(totals.out_rows, who);
  if (num == 0) return empty_;
  // the time maps' rows, when the step runs the leading components as such
  TimePlan plan;
  TimeRows rows;
  if (share_time_ && totals.out_rows > 0) plan = net_->TimeSharedPlan();
  if (plan.prefix() > 0) {
    state_.Segments(step, &segs_);
    const std::string no = plan_time_rows(plan, segs_.lengths.data(), segs_.num, false, &rows);
    if (!no.empty()) KALDI_ERR << who << ": " << no;
    KALDI_ASSERT(rows.result_rows == totals.out_rows && rows.input_rows == segs_.map_rows &&
                 rows.input_rows <= state_.max_map_rows());
    for (const TimeLevel &lev : plan.levels)
      if (state_.max_map_rows() * lev.width >= kStreamLimit)
        KALDI_ERR << who << ": a time map of " << state_.max_map_rows() << " rows of "
                  << lev.width << " columns reaches 2^31 elements";
  }

  hipStream_t st = CuDevice::Instantiate().Stream();
  const MatrixDim arena_dim = {state_.arena_rows(), cols, cols};
  if (arena_.p == nullptr) {
    arena_.reserve(sizeof(float) * (size_t)arena_dim.rows * (size_t)cols);
    if (!prior_offsets_.empty()) {
      const size_t bytes = sizeof(double) * prior_offsets_.size();
      CU_SAFE_CALL(hipMemcpyAsync(d_offsets_.reserve(bytes), prior_offsets_.data(), bytes,
                                  hipMemcpyHostToDevice, st));
    }
  }
  // the step's image -> the device, before the launches; the slots advance
  // (a time-shared step's segment descriptors and result starts behind it)
  const StepLayout lay = step_layout(num, totals);
  const size_t seg_ints =
      plan.prefix() > 0 ? segs_.desc.size() + segs_.out_start.size() : (size_t)0;
  const size_t bytes = lay.bytes + sizeof(int32_t) * seg_ints;
  char *image = staging_.Begin(bytes);
  state_.Plan(step, totals, image, num_out);
  if (seg_ints > 0) {
    int32_t *seg = reinterpret_cast<int32_t *>(image + lay.bytes);
    std::copy(segs_.desc.begin(), segs_.desc.end(), seg);
    std::copy(segs_.out_start.begin(), segs_.out_start.end(), seg + segs_.desc.size());
  }
  const int32_t *d_image = reinterpret_cast<const int32_t *>(staging_.Commit(bytes, st));
  float *arena = static_cast<float *>(arena_.p);
  if (totals.copy_rows > 0) {
    CuProfileScope prof("kn_stream_assemble");
    CNSL_SAFE_CALL(kn_stream_assemble(arena, arena_dim, dim.rows > 0 ? chunk : nullptr,
                                      dim.rows > 0 ? dim : MatrixDim{0, cols, cols},
                                      d_image + lay.row_start, d_image + lay.desc, num,
                                      totals.copy_rows, reinterpret_cast<kcnn_stream_t>(st)));
  }
  if (totals.out_rows == 0) return empty_;
  if (plan.prefix() > 0) {
    const int32_t *d_seg = d_image + lay.bytes / sizeof(int32_t);
    return AcceptShared(plan, rows, segs_, arena, arena_dim, d_seg, d_seg + segs_.desc.size());
  }
  return net_->ComputeExamples(arena, arena_dim, d_image + lay.triples, totals.out_rows,
                               apply_log_,
                               static_cast<const double *>(d_offsets_.p));
}

// The step's time maps, the gather into component prefix's input, and the
// net's pass from there; `rows` has been checked against `plan`.
const CuMatrix<BaseFloat> &OnlineComputer::AcceptShared(const TimePlan &plan,
                                                        const TimeRows &rows,
                                                        const StepSegments &segs,
                                                        const float *arena, MatrixDim arena_dim,
                                                        const int32_t *d_desc,
                                                        const int32_t *d_out_start) {
  const int p = plan.prefix();
  const kcnn_stream_t st = reinterpret_cast<kcnn_stream_t>(CuDevice::Instantiate().Stream());
  if (maps_.size() < (size_t)p) maps_.resize((size_t)p);
  // the first `r` rows of level l's buffer
  auto map_of = [&](int l, int r, MatrixDim *dim) {
    const int width = plan.levels[l].width;
    *dim = MatrixDim{r, width, width};
    return static_cast<float *>(
        maps_[l].reserve(sizeof(float) * (size_t)state_.max_map_rows() * (size_t)width));
  };
  MatrixDim in_dim;
  float *m0 = map_of(0, (int)rows.input_rows, &in_dim);
  {
    CuProfileScope prof("kn_stream_segments");
    CNSL_SAFE_CALL(kn_stream_segments(arena, arena_dim, m0, in_dim, d_desc, segs.num, st));
  }
  const TimeLevel &top = plan.levels[p - 1];
  CuMatrix<BaseFloat> &y = net_->ExamplesInput(p, segs.out_rows);
  KALDI_ASSERT(y.NumCols() == top.width * top.positions && y.NumRows() == segs.out_rows);
  net_->RunTimeSchedule(time_schedule(plan, rows, kStreamRoute), m0, in_dim, map_of, &y,
                        d_out_start, segs.num);
  return net_->ComputeExamplesFrom(p, arena, arena_dim, segs.out_rows, apply_log_,
                                   static_cast<const double *>(d_offsets_.p));
}

int OnlineComputer::TimeSharedPrefix() const {
  return share_time_ ? net_->TimeSharedPlan().prefix() : 0;
}

void OnlineComputer::Reset(int stream) {
  if (!state_.Reset(stream))
    KALDI_ERR << "kcnn_online_reset: stream " << stream << " outside [0, "
              << state_.num_streams() << ")";
}

void OnlineComputer::Frames(int stream, int64_t out[2]) const {
  if (!state_.Frames(stream, out))
    KALDI_ERR << "kcnn_online_frames: stream " << stream << " outside [0, "
              << state_.num_streams() << ")";
}

}  // namespace kcnn
