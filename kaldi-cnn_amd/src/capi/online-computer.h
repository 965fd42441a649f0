// capi/online-computer.h -- the streaming forward pass behind kcnn_online_*
// (include/kcnn.h): upstream NnetOnlineComputer(nnet, pad_input = true), the
// decodable of online2-wav-nnet2-latgen-faster --online=true, for num_streams
// concurrent utterances batched into one pass per step.  A step gives some
// slots their next frames; every frame whose right context is then in -- all
// of them once the utterance has ended -- is computed, frame t from the input
// frames clamp(t + o, 0, T - 1), o = -L .. R, of the eventual utterance of T
// frames.  The bookkeeping is stream-state.h's; the frames a slot still needs
// live in a device arena of the computer's own (two buffers a slot, written
// by kn_stream_assemble, never in place), which is the `feats` of the net's
// frames pass, the step's staged triples being its examples
// (NnetStack::ComputeExamples).  So the net's activations hold nothing of a
// stream, and its other forward calls between steps disturb none.  A network
// with a Splice above component 0 is recomputed per example, as
// PropagateFrames does: nothing deeper than the input is cached.
//
// With share_time, a step of a network the time plan accepts (time-plan.h) is
// a small whole-utterance pass over time maps instead: each emitting slot's
// frames [e0 - L, e0 + k + R), clamped, are one segment of the level-0 map
// (kn_stream_segments from the arena; stream-state.h StepSegments), the packed
// segments an unpadded ComputeShared input.  The launches are ComputeShared's
// (time_schedule, run by NnetStack::RunTimeSchedule) under kStreamRoute
// (time-plan.h, which says why the routes differ): every Convolution level is
// one kn_timemap_conv (kn_timemap_conv2d where the level or its input keeps a
// height), the ReLU on it fused; the components above the prefix run as in any
// other step (NnetStack::ComputeExamplesFrom).  The maps are the computer's own, one
// buffer a level allocated once for the most rows a step can have, so a step
// of another size allocates nothing below the first FC and the net's other
// forward calls, ComputeShared included, disturb nothing.  Nothing is carried
// between steps: Reset, final and slot reuse are what they were, and a step
// takes either route whatever the last one took.
// Errors are thrown; kcnn-capi.cc turns them into error codes.
#ifndef KCNN_CAPI_ONLINE_COMPUTER_H_
#define KCNN_CAPI_ONLINE_COMPUTER_H_

#include <vector>

#include "nnet-stack.h"
#include "stream-state.h"

#pragma GCC visibility push(hidden)
namespace kcnn {

class OnlineComputer {
 public:
  // Borrows `net`, which must outlive the computer.  priors: as Compute's
  // (OutputDim host floats, finite and > 0, only with apply_log; or NULL).
  // Allocates nothing on the device; throws on numbers no arena can have.
  OnlineComputer(NnetStack *net, int num_streams, int max_chunk, const float *priors,
                 int num_priors, float prior_scale, bool apply_log, bool share_time = false);

  // One step: slot streams[i] gets num_new[i] frames (0 .. max_chunk; 0 only
  // with final[i]), rows of `chunk` ([sum of num_new x InputDim], device) in
  // order, and ends its utterance where final[i] != 0, which frees the slot.
  // num_out[i] (host) is the number of rows slot streams[i] contributes to
  // the result, slots in the step's order, frames ascending; the result
  // (valid until the net's next forward call) is the net's last output P or
  // its log-likelihoods, [0 x OutputDim] with no network kernel run when the
  // step emits nothing.  Every check precedes every launch and every change
  // of a slot.  Does not synchronise and reads nothing back.
  const CuMatrix<BaseFloat> &Accept(const float *chunk, MatrixDim dim, const int32_t *streams,
                                    const int32_t *num_new, const int32_t *final, int num,
                                    int32_t *num_out);
  void Reset(int stream);                          // abandons the slot's utterance
  void Frames(int stream, int64_t out[2]) const;  // {seen, emitted}
  // The components the next step would run as time maps: the net's plan as
  // the literal path now stands, 0 without share_time or when it declines.
  int TimeSharedPrefix() const;

 private:
  // the time-shared route of a step whose image is staged and arena assembled
  const CuMatrix<BaseFloat> &AcceptShared(const TimePlan &plan, const TimeRows &rows,
                                          const StepSegments &segs, const float *arena,
                                          MatrixDim arena_dim, const int32_t *d_desc,
                                          const int32_t *d_out_start);
  bool share_time_;
  StepSegments segs_;
  // level l's map, [state_.max_map_rows() x its width], allocated once by the
  // first time-shared step (a level a fused ReLU skips is never allocated)
  std::vector<kaldi::CuBuffer> maps_;
  NnetStack *net_;
  StreamState state_;
  bool apply_log_;
  std::vector<double> prior_offsets_;   // prior_scale * log(prior), or empty
  // allocated by the first accepted step, once
  kaldi::CuBuffer arena_, d_offsets_;
  NnetStack::LabelStaging staging_;     // a step's prefix, descriptors and triples
  CuMatrix<BaseFloat> empty_;           // the result of a step that emits nothing
};

}  // namespace kcnn
#pragma GCC visibility pop

#endif  // KCNN_CAPI_ONLINE_COMPUTER_H_
