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
                               bool apply_log)
    : net_(net),
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
  const StepLayout lay = step_layout(num, totals);
  char *image = staging_.Begin(lay.bytes);
  state_.Plan(step, totals, image, num_out);
  const int32_t *d_image =
      reinterpret_cast<const int32_t *>(staging_.Commit(lay.bytes, st));
  float *arena = static_cast<float *>(arena_.p);
  if (totals.copy_rows > 0) {
    CuProfileScope prof("kn_stream_assemble");
    CNSL_SAFE_CALL(kn_stream_assemble(arena, arena_dim, dim.rows > 0 ? chunk : nullptr,
                                      dim.rows > 0 ? dim : MatrixDim{0, cols, cols},
                                      d_image + lay.row_start, d_image + lay.desc, num,
                                      totals.copy_rows, reinterpret_cast<kcnn_stream_t>(st)));
  }
  if (totals.out_rows == 0) return empty_;
  return net_->ComputeExamples(arena, arena_dim, d_image + lay.triples, totals.out_rows,
                               apply_log_,
                               static_cast<const double *>(d_offsets_.p));
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
