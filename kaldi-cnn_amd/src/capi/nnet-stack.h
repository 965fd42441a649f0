// capi/nnet-stack.h -- the NnetUpdater-style component stack behind
// kcnn_nnet_* (include/kcnn.h): the chunk offsets (Nnet::ComputeChunkInfo),
// the Conv -> Maxpool and Conv -> ReLU fused passes and what they leave
// unstored or deferred, the statistics hand-off to the FC GEMMs, the
// data-parallel gradient / data-gradient split and the cross-entropy backward;
// and what follows a training iteration: the <Nnet> file (Nnet::Read / Write),
// the scaled, Dropout-free copy (nnet-am-copy), ComputeProb
// (nnet-compute-prob) and Compute, the whole-utterance forward pass of
// upstream NnetComputer (nnet-am-compute, the decodable), with ComputeShared,
// the same pass with the convolutional prefix run once per time step
// (time-plan.h); and what comes
// before one: PropagateFrames, a minibatch as rows of a corpus that stays on
// the device (nnet-get-egs and nnet-shuffle-egs without the window matrices),
// with PropagateFramesShared, such a step with the convolutional prefix run
// once per time step of each run of consecutive rows, forward and backward.
// Errors are thrown (KALDI_ASSERT / KALDI_ERR); kcnn-capi.cc turns them into
// error codes.
#ifndef KCNN_CAPI_NNET_STACK_H_
#define KCNN_CAPI_NNET_STACK_H_

#include <functional>
#include <iosfwd>
#include <memory>
#include <vector>

#include "kcnn.h"

#include "../cnslmat/pool-stats.h"
#include "../kaldi-lite/cu-device.h"
#include "../kaldi-lite/cu-matrix.h"
#include "../nnet0/nnet-component-nnet0.h"
#include "../nnet2/nnet-component.h"
#include "frame-index.h"
#include "time-plan.h"

struct kcnn_component {
  kaldi::nnet2::Component *c;
};

// Internal to libkcnn.so, as the file-static functions this replaces were: the
// library's exported surface stays include/kcnn.h.
#pragma GCC visibility push(hidden)
namespace kcnn {

using kaldi::BaseFloat;
using kaldi::CuMatrix;
using kaldi::CuSubMatrix;

// Runtime fusion of Conv -> Maxpool (kcnn_set_fusion; env KCNN_FUSE): 0 off,
// 1 on without storing the conv output, 2 on and the conv output stored.
int fusion_mode();
void set_fusion_mode(int mode);

// kn_comp_objf_and_deriv (nnet2/nnet-kernels.h) on the library's stream with
// its workspace and profile scope: labels and totals are device pointers.
void comp_objf_and_deriv(const int32_t *rows, const int32_t *cols, const float *weights,
                         int num, const float *probs, MatrixDim p_dim, float *deriv,
                         MatrixDim d_dim, double *tot);

class NnetStack {
 public:
  // kcnn_nnet_backprop_component's `mode` (include/kcnn.h)
  enum BackpropMode : int {
    kUpdate = 0,        // Backprop, updatable components update
    kGradient = 1,      // the parameter gradient to `grad` and dX, no update
    kDataOnly = 2,      // dX alone
    kGradientOnly = 3,  // the parameter gradient alone (a later kDataOnly adds dX)
  };

  // One component per config line ('#' comments and blank lines skipped);
  // throws on a bad line, an empty config or mismatched dimensions.
  explicit NnetStack(const char *config);
  // Upstream Nnet::Read: <Nnet> <NumComponents> n <Components> n x
  // Component::ReadNew </Components> </Nnet>, then the checks of the config
  // constructor.  Throws on anything else.
  NnetStack(std::istream &is, bool binary);
  // A new stack of src's components' Copy()s (upstream nnet-am-copy): with
  // scales, the k-th updatable component Scale(scales[k]) (Nnet::
  // ScaleComponents; num_scales must be their number); with remove_dropout,
  // without the DropoutComponents (Nnet::RemoveDropout).  Checked as above.
  NnetStack(const NnetStack &src, const float *scales, int num_scales, bool remove_dropout);

  // Upstream Nnet::Write; in text mode a newline follows each component.
  void Write(std::ostream &os, bool binary) const;

  int NumComponents() const { return (int)comps_.size(); }
  kcnn_component *ComponentAt(int i);  // NULL out of range

  void Propagate(const float *in, MatrixDim in_dim);
  // Output of component i (-1: the network input) and d(input of component
  // i) of the last minibatch.  Not const: an unstored output is recomputed
  // and a deferred pool derivative computed on request.
  const CuMatrix<BaseFloat> &Output(int i);
  const CuMatrix<BaseFloat> &InputDeriv(int i);

  // out_deriv is read for the last component only; lower ones read the input
  // derivative of the component above.
  void BackpropComponent(int i, const float *out_deriv, MatrixDim od_dim, BackpropMode mode,
                         float *grad, bool skip_first_dx);
  // An affine layer's parameter gradient, then between(ctx) (the caller starts
  // its all-reduce there), then the layer's data gradient: kGradientOnly and
  // kDataOnly in one call, so both GEMMs' operand statistics come from one
  // launch set that lives across the callback (the pair of calls computed
  // them twice).
  void BackpropSplit(int i, const float *out_deriv, MatrixDim od_dim, float *grad,
                     bool skip_first_dx, void (*between)(void *), void *ctx);
  void Backprop(const float *out_deriv, MatrixDim od_dim);  // kUpdate, top down
  // Cross-entropy against the last output for (row, col, weight) labels
  // sorted by row, accumulated into the objective totals, then Backprop.
  // Does not synchronise.
  void BackpropXent(const int32_t *rows, const int32_t *cols, const float *weights, int num,
                    bool skip_first_dx);
  // The first half of BackpropXent, for a caller that runs the backward
  // itself (kcnn_dp.py: per component, gradients all-reduced): the labels
  // checked and staged, the objective and weight added to the totals, and
  // d(last output) left where the generic backward reads it.  Returns the
  // component that backward starts at.  With a last SoftmaxComponent (not on
  // the literal path) the fused kernel has written that Softmax's input
  // derivative too: nc - 2 is returned, *out_deriv is NULL with a zero dim
  // (nothing below the last component reads it), and BackpropComponent /
  // BackpropSplit of the last component throw until the next forward pass,
  // since its out_deriv was never formed.  Otherwise nc - 1, and *out_deriv /
  // *od_dim are the stack's own matrix, to be passed to those calls; valid
  // until the next XentDeriv.  `who` names the C entry point in errors.
  // Does not synchronise.
  int XentDeriv(const int32_t *rows, const int32_t *cols, const float *weights, int num,
                const float **out_deriv, MatrixDim *od_dim,
                const char *who = "kcnn_nnet_xent_deriv");
  // {objective, weight} summed since the last reset; synchronises.
  void ObjfTotal(double out[2], bool reset);
  // DropoutComponent::SetRowOffset on every DropoutComponent of the stack
  // (none: nothing happens); holds until set again.
  void SetRowOffset(uint64_t offset);
  // Every DropoutComponent counts one Propagate call without running: a
  // data-parallel rank with an empty shard stays on the others' call number.
  void SkipDropoutCall();
  // nnet-compute-prob on one minibatch: the forward pass, then the objective,
  // the weight and the accuracy weight of the labels (as for BackpropXent)
  // added to totals of their own.  No component changes.  A last Softmax is
  // not run: one kernel takes the three sums from its input (the literal path
  // runs it and reads its output).  Backprop* throw until the next Propagate;
  // Output recomputes the unstored last output on request.  Does not
  // synchronise.
  void ComputeProb(const float *in, MatrixDim in_dim, const int32_t *rows, const int32_t *cols,
                   const float *weights, int num);
  // {objective, weight, accuracy weight} of ComputeProb since the last reset;
  // synchronises.
  void ProbTotal(double out[3], bool reset);

  // The frames the network reads before / after the frame it computes: the
  // sums over the components of -Context().front() / Context().back()
  // (upstream Nnet::LeftContext / RightContext).
  int LeftContext() const;
  int RightContext() const;
  // Upstream NnetComputer on num_utts whole utterances stacked row-wise in
  // `in` ([sum of lengths x InputDim], device; lengths on the host), each
  // propagated as ONE chunk of many rows.  pad_input: an utterance of T
  // frames is seen as frames -L .. T-1+R, frame f being frame clamp(f, 0,
  // T-1), and gives T rows; else it gives T - L - R rows and T <= L + R is an
  // error.  The padded frames are never stored: the first SpliceComponent
  // clamps its reads (when component 0 is not one, a one-slot pass of its
  // kernel lays the clamped frames out first, and Output(-1) is that
  // matrix).  Every activation keeps the frames the contexts still to come
  // need, so rows shrink Splice by Splice, per utterance; all other
  // components see one chunk of all rows, the fused Conv -> Maxpool and Conv
  // -> ReLU passes and the statistics hand-off included.  A DropoutComponent
  // draws its mask: use the test model.
  // The result (returned; valid until the next forward call), from the last
  // output P: with apply_log, log(max(P, 1e-20)) - prior_scale * log(prior
  // [col]) (nnet-am-compute --apply-log --divide-by-priors; kn_loglikes),
  // without priors (NULL) the log alone; without apply_log, P itself, and
  // priors are then refused.  priors: OutputDim host floats, all finite and
  // > 0.  A last Softmax is then not run: one kernel forms each probability
  // from its input and writes the log-likelihood (the literal path runs it
  // and reads its output; the same bits).  Every check precedes every launch.
  // Outputs are sized without Resize's zero fill (every forward kernel writes
  // its whole output); the literal path keeps the fill.
  // Leaves the state ComputeProb leaves; does not synchronise.
  const CuMatrix<BaseFloat> &Compute(const float *in, MatrixDim in_dim, const int32_t *lengths,
                                     int num_utts, bool pad_input, const float *priors,
                                     int num_priors, float prior_scale, bool apply_log);
  // Compute with the leading Splice -> {Convolution | Maxpool | ReLU}...
  // components (the prefix, time-plan.h) run once per time step instead of
  // once per window: each is a TIME MAP, one row per row of the (clamped)
  // input and one column per channel -- a convolution tap a GEMM of the matrix
  // layer on a row-shifted view (AddMatMatBias, then AddMatMat with beta = 1),
  // pools and ReLUs one pass each (kn_timemap_epilogue) -- and a gather
  // (kn_timemap_gather) then writes Output(prefix - 1) in the window layout
  // Compute gives it; from component `prefix` upwards the pass is Compute's
  // own.  A level may keep a height (frequency) axis H, its map row H C
  // floats (time-plan.h): a Convolution with kernel-height < in-height, or on
  // such a level, is one kn_timemap_conv2d, a Maxpool on one kn_timemap_pool2d
  // and the gather kn_timemap_gather2d (nnet2/nnet-timemap-2d.hip).  The
  // launches are time_schedule's under kUtteranceRoute (time-plan.h), run by
  // RunTimeSchedule; the maps are a CuMatrix a level, sized per call.
  // Same arguments, checks, result and state as Compute; to the error
  // bar of the GEMMs, not the bits, the same values.  Output(i) below prefix -
  // 1 throws afterwards (those activations are never formed); TimeMap gives
  // the maps.  A stack the plan declines runs Compute itself.
  const CuMatrix<BaseFloat> &ComputeShared(const float *in, MatrixDim in_dim,
                                           const int32_t *lengths, int num_utts, bool pad_input,
                                           const float *priors, int num_priors,
                                           float prior_scale, bool apply_log);
  // The plan of ComputeShared for this stack as the literal path now stands
  // (no levels: declined); host only.
  TimePlan TimeSharedPlan() const;
  // Level `level` (the output of component `level`) of the last ComputeShared:
  // its first dim.rows rows are computed, row s being row s of the level-0
  // map, the (clamped) input.  Valid until the next forward call; throws when
  // the last forward was not ComputeShared's over time maps.
  struct TimeMapInfo {
    const float *data = nullptr;
    MatrixDim dim = {0, 0, 0};
    int channels = 0, positions = 0, dilation = 0;
    int height = 1;  // dim.cols = height channels, element (h, c) at column h + c height
  };
  TimeMapInfo TimeMap(int level) const;

  // Propagate on a minibatch given as `num` rows (HOST indices, any order,
  // repeats allowed) of a corpus that stays on the device: `feats` holds whole
  // utterances stacked row-wise, `corpus` their starts (frame-index.h).
  // Example n, corpus row r in utterance rows [s, e), has the input chunk
  // clamp(r + o, s, e - 1) for the input chunk's offsets o = -L .. R: the
  // window matrix Propagate would be given.  From component 0's output upwards
  // the pass is Propagate's, num chunks.  A first SpliceComponent gathers its
  // output straight from the corpus (the window matrix is never stored;
  // Output(-1) is the borrowed corpus) and its Backprop is then skipped: it has
  // no parameters, and InputDeriv(0) throws.  Any other component 0 gets the
  // window matrix laid out by the same kernel into a matrix of the stack's
  // (Output(-1)) and runs as after Propagate.  Every check (frames, indices,
  // columns, sizes) precedes every launch; the examples are staged first.
  void PropagateFrames(const float *feats, MatrixDim dim, const CorpusIndex &corpus,
                       const int32_t *frames, int num);
  // PropagateFrames with the prefix of the training plan (TimeSharedTrainPlan)
  // run once per time step of each RUN of the list (frame-index.h, frame_runs:
  // a maximal stretch of consecutive rows of one utterance; any list is legal,
  // and example n stays frames[n]).  A run of k frames is a segment of k + L +
  // R rows of the level-0 map, laid out clamped from the corpus by
  // kn_timemap_layout; the levels are time_schedule's under kUtteranceRoute, so
  // every level is formed, and the gather writes Output(prefix - 1) as
  // PropagateFrames would, to the error bar of the GEMMs.  Components prefix ..
  // run as PropagateFrames runs them (Dropout, row offsets, fused pairs, the
  // statistics hand-off).  PropagateFrames' checks, then the segments' (the
  // rows of every map below 2^31, plan_train_rows), precede every launch.
  // Leaves PropagateFrames' state, but Output(i) below prefix - 1 throws and
  // TimeMap gives the maps.  Backprop / BackpropXent then run components prefix
  // .. as always and the prefix ONCE over the maps (time_backward_schedule: the
  // scatter, kn_timemap_epilogue_bwd, and per Convolution the weight, bias and
  // data gradients as per-tap GEMMs on row-shifted views), every Convolution of
  // the prefix stepping by ApplyGradient(gradient, num).  The prefix's
  // RectifiedLinearComponents accumulate no NonlinearStats in such a step:
  // their window columns are never formed.  BackpropComponent, BackpropSplit
  // and InputDeriv of a prefix component throw, changing nothing.  With a
  // training prefix of 0 (or the literal path on) the call is PropagateFrames.
  void PropagateFramesShared(const float *feats, MatrixDim dim, const CorpusIndex &corpus,
                             const int32_t *frames, int num);
  // The plan of PropagateFramesShared: TimeSharedPlan, declined when a level
  // keeps a height (time-plan.h, time_train_plan) or when it covers the whole
  // stack (the backward starts from the component above the prefix).
  TimePlan TimeSharedTrainPlan() const;
  // After PropagateFramesShared and a Backprop / BackpropXent, until the next
  // forward call: the derivative map of `level` (rows and geometry as
  // TimeMap's; level 0 and a pool's own level under a ReLU have none and
  // throw), and the flat gradient ([KernelDim x Group | Group], as
  // ComputeGradient lays it out) that the backward applied to prefix
  // Convolution i.
  TimeMapInfo TimeMapDeriv(int level) const;
  const float *TimeGradient(int i, int *num) const;
  // ComputeProb on such a minibatch; leaves the state ComputeProb leaves.
  void ComputeProbFrames(const float *feats, MatrixDim dim, const CorpusIndex &corpus,
                         const int32_t *frames, int num, const int32_t *rows,
                         const int32_t *cols, const float *weights, int num_labels);

  // What kcnn::OnlineComputer (online-computer.h) needs: Compute's checks of
  // its priors under another caller's name; the checks PropagateFrames makes
  // of its pass once the frame list itself is checked (`num` examples: the
  // window matrix and every activation below 2^31 rows and elements, a gapped
  // first Splice within its offset table); and the pass itself from triples
  // the caller has made and put on the device, `examples` ({row, lo, hi} per
  // example, rows of `feats`), instead of a CorpusIndex and a frame list.
  // ComputeExamples is PropagateFrames' forward (a first Splice gathering
  // straight from `feats`, any other component 0 getting its window matrix
  // laid out, the fused pairs, the statistics hand-off) with the outputs sized
  // as Compute sizes them, without the zero fill, then Compute's result: the
  // last output, or with apply_log its log less prior_offsets (DEVICE fp64,
  // OutputDim entries, or NULL), by the fused kernel from a last Softmax's
  // input unless the literal path is on.  Checks nothing: CheckExamples first.
  // Leaves the state ComputeProbFrames leaves; does not synchronise.
  void CheckPriors(const float *priors, int num_priors, bool apply_log, const char *who) const;
  void CheckExamples(int num, const char *who) const;
  const CuMatrix<BaseFloat> &ComputeExamples(const float *feats, MatrixDim dim,
                                             const int32_t *examples, int num, bool apply_log,
                                             const double *prior_offsets);
  // The upper part of ComputeExamples, for a caller that has formed component
  // `first`'s input itself (an OnlineComputer with share_time: its time maps,
  // gathered into ExamplesInput): components first .. of a pass of `num`
  // examples, then ComputeExamples' result.  0 < first < NumComponents(), and
  // component 0 is a Splice (the plan's condition).  ExamplesInput sizes
  // Output(first - 1) to its `num` rows, without the fill, and returns it to
  // be written whole.  (feats, dim) is what Output(-1) then names, as after
  // ComputeExamples; Output(i) below first - 1 throws afterwards: those
  // activations were never formed.  Same state otherwise.
  CuMatrix<BaseFloat> &ExamplesInput(int first, int num);
  const CuMatrix<BaseFloat> &ComputeExamplesFrom(int first, const float *feats, MatrixDim dim,
                                                 int num, bool apply_log,
                                                 const double *prior_offsets);
  // Runs one pass over time maps, the launches of time_schedule (time-plan.h)
  // in order: the one place that names the kn_timemap_* kernels, for
  // ComputeShared and for an OnlineComputer's time-shared step.  Storage is
  // the caller's: (in0, in0_dim) is the level-0 map, map_of(level, rows, &dim)
  // gives the map a launch writes, of `rows` rows at least (the launches that
  // follow read it where it was given), `y` is the gather's destination,
  // sized, and d_starts (device) the num_starts + 1 starts of its results.
  using TimeMapFn = std::function<float *(int level, int rows, MatrixDim *dim)>;
  void RunTimeSchedule(const std::vector<TimeLaunch> &sched, const float *in0,
                       MatrixDim in0_dim, const TimeMapFn &map_of, CuMatrix<BaseFloat> *y,
                       const int32_t *d_starts, int num_starts);
  int InputDim() const { return comps_.front().c->InputDim(); }
  int OutputDim() const { return comps_.back().c->OutputDim(); }

  // BackpropXent: the label list's pinned staging buffer and its device image
  // (xent-labels.h), the event after which the staging buffer may be
  // rewritten, and the fp64 {objective, weight} totals on the device.
  // Compute stages its utterance starts and prior offsets through another,
  // PropagateFrames its example triples (frame-index.h) through a third, and
  // an OnlineComputer its steps through one of its own.
  struct LabelStaging {
    void *host = nullptr;
    size_t host_bytes = 0;
    hipEvent_t copied = nullptr;
    kaldi::CuBuffer totals, dev;
    LabelStaging() {}
    ~LabelStaging();  // waits for the last copy to leave `host`
    LabelStaging(const LabelStaging &) = delete;
    LabelStaging &operator=(const LabelStaging &) = delete;
    // the staging buffer, of `bytes` at least and free to be written
    char *Begin(size_t bytes);
    // its first `bytes` -> dev on `st`; returns dev
    const char *Commit(size_t bytes, hipStream_t st);
    // the checked labels -> host -> dev on `st`; returns dev
    const char *Stage(const int32_t *rows, const int32_t *cols, const float *weights, int num,
                      int num_rows, hipStream_t st);
  };

 private:
  struct Comp {
    std::unique_ptr<kaldi::nnet2::Component> c;
    kcnn_component handle{nullptr};
    // what the component is, found once (the stack never changes); NULL
    // where it is not of that kind
    cnsl::nnet0::ConvolutionComponent *conv = nullptr;
    cnsl::nnet0::MaxpoolComponent *pool = nullptr;
    kaldi::nnet2::RectifiedLinearComponent *relu = nullptr;
    kaldi::nnet2::AffineComponent *affine = nullptr;
    kaldi::nnet2::SoftmaxComponent *softmax = nullptr;
    kaldi::nnet2::SpliceComponent *splice = nullptr;
    kaldi::nnet2::UpdatableComponent *updatable = nullptr;
    CuMatrix<BaseFloat> deriv;  // d(input of this component)
    // a pool run fused with the conv below: its routing mask ([rows x
    // OutputDim] x FusedMaskBytes), valid for the last Propagate's minibatch
    kaldi::CuBuffer mask;
    bool mask_valid = false;
    // deriv of a mask-fused pool not computed (fusion mode 1): the conv
    // below consumes the pool's out_deriv and mask directly; materialised by
    // InputDeriv on request, or when that conv's pass declines
    bool deriv_deferred = false;
  };
  // Whether an activation's matrix holds its values: a fused pass leaves the
  // conv output unstored (fusion mode 1; nothing in training reads it).
  // Output recomputes it on request until the producing component's backprop
  // has run, which may have changed its parameters.
  enum Stale { kStored, kRecomputable, kGone };
  // acts_[i] is component i's input, acts_[i + 1] its output; acts_[0]
  // borrows the caller's network input.
  struct Activation {
    CuMatrix<BaseFloat> value;
    // frame offsets of this activation's chunk, ascending (upstream
    // Nnet::ComputeChunkInfo).  Gapped contexts (SpliceComponent
    // context=-3:0:3) make a middle layer's offsets non-contiguous.
    std::vector<kaldi::int32> offsets;
    // Compute: the rows more than its final output frames that an utterance
    // has here (the contexts still to come), and all the utterances' rows
    int utt_ext = 0, utt_rows = 0;
    Stale stale = kStored;
    // max |value| per row and per column from the fused forward that wrote
    // it (pool-stats.h), offered to the next component's GEMMs
    // (CuGemmStatsHint) for the minibatch of the last Propagate
    kaldi::CuBuffer stats;
    bool stats_valid = false;
    // the column statistics left pending by the fused forward (the next
    // component's FC backward runs them, pool-stats.h PoolColDeferred) and
    // the forward's per-workgroup column partials they read, kept until then
    PoolColDeferred col_deferred;
    kaldi::CuBuffer col_partials;
  };
  // the constructors' shared tail: the checks, the kinds, the chunk offsets
  void Init(std::vector<std::unique_ptr<kaldi::nnet2::Component>> parsed);
  // A minibatch of corpus rows (PropagateFrames): the caller's arguments, and
  // `examples`, their staged triples on the device once StageFrames has run
  // (ComputeExamples: the caller's own, with no corpus and no frames).
  struct FrameList {
    const float *feats;
    MatrixDim dim;
    const CorpusIndex *corpus;
    const int32_t *frames;
    int num;
    const int32_t *examples;
  };
  // Propagate's checks and its first `count` components; with `fl` (checked
  // and staged) the input is its minibatch and (in, in_dim) the corpus matrix
  void PropagateFirst(const float *in, MatrixDim in_dim, int count,
                      const FrameList *fl = nullptr);
  // PropagateFrames' checks; returns the number of examples
  int CheckFrames(const FrameList &fl, const char *who) const;
  void StageFrames(FrameList *fl);
  // ComputeProb and ComputeProbFrames (fl != NULL)
  void ComputeProbOn(const float *in, MatrixDim in_dim, FrameList *fl, const int32_t *rows,
                     const int32_t *cols, const float *weights, int num, const char *who);
  void RequireTrainingForward(const char *who) const;
  // throws for the last component after a fused XentDeriv
  void RequireLastNotFused(int i, const char *who) const;
  // the checked labels staged on the device (xent-labels.h)
  struct DeviceLabels {
    const int32_t *row_start, *row, *col;
    const float *weight;
  };
  DeviceLabels StageLabels(const int32_t *rows, const int32_t *cols, const float *weights,
                           int num, int num_rows);
  double *prob_totals();
  // whether a result with apply_log is formed from a last Softmax's input
  bool FusedLoglikes(bool apply_log) const;
  // Compute's result once the forward has run (all components, or all but
  // the last with FusedLoglikes): the last output, or its `total` rows of
  // log-likelihoods less d_off (device, or NULL)
  const CuMatrix<BaseFloat> &Loglikes(bool apply_log, const double *d_off, int total);
  // Compute's forward pass over components first .. count - 1; first > 0:
  // ComputeShared's time maps have written component first's input
  void PropagateUtterances(const float *in, MatrixDim in_dim, const int32_t *utt_start,
                           int num_utts, int total, bool pad_input, int count, int first = 0);
  void LayOutClamped(const float *in, MatrixDim in_dim, const int32_t *utt_start, int num_utts,
                     int total, int ext, int left);
  // Compute and ComputeShared (share_time) under the caller's name
  const CuMatrix<BaseFloat> &ComputeOn(const float *in, MatrixDim in_dim, const int32_t *lengths,
                                       int num_utts, bool pad_input, const float *priors,
                                       int num_priors, float prior_scale, bool apply_log,
                                       bool share_time, const char *who);
  void PropagateTimeShared(const float *in, MatrixDim in_dim, const int32_t *utt_start,
                           int num_utts, int total, bool pad_input, const TimePlan &plan,
                           const TimeRows &rows);
  // the levels above level 0 (time_views_[0] is set) and the gather into
  // Output(prefix - 1), of `total` rows
  void FormTimeLevels(const TimePlan &plan, const TimeRows &rows, const int32_t *starts,
                      int num_starts, int total);
  // the backward over the maps of the last PropagateFramesShared, from
  // InputDeriv(prefix), and the prefix Convolutions' steps
  void BackpropTimeMaps();
  // throws when component i is of the prefix the last forward ran as time maps
  void RequireAbovePrefix(int i, const char *who) const;

  Activation &in(int i) { return acts_[i]; }
  Activation &out(int i) { return acts_[i + 1]; }
  kaldi::nnet2::ChunkInfo in_info(int i);
  kaldi::nnet2::ChunkInfo out_info(int i);
  void ForgetMinibatch();
  std::unique_ptr<kaldi::CuGemmStatsHint> input_stats(int i);
  bool PropagateMaxpoolPair(int i);
  bool PropagateReluPair(int i);
  void MaterialisePoolDeriv(int i);
  CuSubMatrix<BaseFloat> out_deriv_of(int i, const float *caller_ptr, MatrixDim caller_dim);
  kaldi::nnet2::Component *to_update(const Comp &c, BackpropMode mode) const;
  double *objf_totals();

  std::vector<Comp> comps_;
  std::vector<Activation> acts_;  // comps_.size() + 1
  int num_chunks_ = 0;
  LabelStaging labels_;
  CuMatrix<BaseFloat> xent_deriv_;  // the literal path's d(last output)
  kaldi::CuBuffer prob_totals_;     // ComputeProb's fp64 {objective, weight, accuracy}
  // the last forward was ComputeProb's or Compute's: there is nothing to
  // backpropagate
  bool prob_forward_ = false;
  // XentDeriv took the fused route: the last Softmax's input derivative is
  // written and its Backprop must not run; until the next forward pass, or
  // the end of BackpropXent
  bool xent_fused_ = false;
  // the last forward was Compute's: an activation is one chunk of utt_rows
  bool whole_utts_ = false;
  LabelStaging utts_;                   // Compute's utterance starts and prior offsets
  CuMatrix<BaseFloat> padded_input_;    // Compute's clamped input frames, when laid out
  CuMatrix<BaseFloat> loglikes_;        // Compute's result with apply_log
  // the last forward was ComputeShared's over time maps: time_views_ holds
  // its levels, level 0 a view of the input or of padded_input_, the others
  // of time_maps_ (one a component, sized once)
  bool time_shared_ = false;
  std::vector<CuMatrix<BaseFloat>> time_maps_;
  std::vector<TimeMapInfo> time_views_;
  // the last forward was PropagateFramesShared's over time maps (time_shared_
  // holds too): its plan and rows, the runs' starts on the device (in
  // frames_), and what its backward leaves -- the derivative maps (views of
  // time_derivs_, data NULL where none is formed) and the gradients applied
  bool time_train_ = false, time_backward_done_ = false;
  TimePlan train_plan_;
  TimeRows train_rows_;
  const int32_t *train_starts_ = nullptr;
  int train_runs_ = 0;
  std::vector<CuMatrix<BaseFloat>> time_derivs_, time_grads_;
  std::vector<TimeMapInfo> time_dviews_;
  // the last forward was PropagateFrames' through a first Splice: component
  // 0's input is the corpus, not a window matrix, and it has no Backprop
  bool frames_fused_ = false;
  // the last forward was ComputeExamplesFrom's: the outputs of components
  // below examples_first_ - 1 were not formed (0: all were)
  int examples_first_ = 0;
  LabelStaging frames_;                // PropagateFrames' example triples
  // its window matrix when laid out, contiguous as a caller's would be
  kaldi::CuBuffer frames_input_;
};

}  // namespace kcnn
#pragma GCC visibility pop

#endif  // KCNN_CAPI_NNET_STACK_H_
