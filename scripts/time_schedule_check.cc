// scripts/time_schedule_check.cc -- the launches of a pass over time maps
// (kaldi-cnn_amd/src/capi/time-plan.h, time_schedule) as a stand-alone host
// program, for a run under a host sanitizer.  No GPU call.
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Ikaldi-cnn_amd/src scripts/time_schedule_check.cc -o time_schedule_check
//   ./time_schedule_check tests/golden/nnet.config tests/golden/freq_conv.config
//
// For nnet.config, freq_conv.config, nets F and M of time_plan_height_check.cc
// and the shrunken 1-D net of time_plan_check.cc (pool-channel-dim 1 and 4), on
// utterances of (1, 7, 23, 2) result frames padded and unpadded, under the
// whole-utterance route and the streaming step's:
// 1. the schedule, printed, against a table written out below by hand from
//    the two loops this function replaced (NnetStack::PropagateTimeShared and
//    OnlineComputer::AcceptShared before it): per launch the op, the levels,
//    the rows and every integer argument.  A table gives rows as the input's
//    rows less a number, the reaches of the levels up to that one added up by
//    hand; the input has 33 + 4 context rows either way.
// 2. what holds of every schedule: a launch reads a level that level 0 or an
//    earlier launch wrote, with rows enough for its highest tap; the
//    whole-utterance route writes every level once, with no kn_timemap_conv
//    and no fused ReLU; the streaming route has no per-tap GEMMs and leaves
//    unwritten exactly the Convolution levels directly below a ReLU; the one
//    gather is last and reads the top level's computed rows.
// 3. an empty plan gives an empty schedule.
#include <fstream>
#include <set>

#include "time_plan_config.h"

using kcnn::TimeComp;
using kcnn::TimeLaunch;
using kcnn::TimeLevel;
using kcnn::TimePlan;
using kcnn::TimeRoute;
using kcnn::TimeRows;

namespace {

const char *kOpNames[] = {"conv_taps", "conv", "conv2d", "pool2d", "epilogue", "gather",
                          "gather2d"};

// One launch as a table states it: in_less and out_less are what the level
// read and the level(s) written have fewer rows than the input.
struct Want {
  TimeLaunch::Op op;
  int comp, in_level, in_less, out_level, act_level, out_less;
  int height, channels, kernel_height, taps, dilation, wc, wd, relu, pool_height, pool_channel;
  int positions, context;
};

Want conv(TimeLaunch::Op op, int comp, int in_level, int in_less, int out_level, int act_level,
          int out_less, int taps, int dilation, int wc, int wd, int relu) {
  return {op, comp, in_level, in_less, out_level, act_level, out_less, 0, 0, 0, taps, dilation,
          wc, wd, relu, 0, 0, 0, 0};
}
Want conv2d(int comp, int in_level, int in_less, int out_level, int act_level, int out_less,
            int height, int channels, int kernel_height, int taps, int dilation, int relu) {
  return {TimeLaunch::kConv2d, comp, in_level, in_less, out_level, act_level, out_less, height,
          channels, kernel_height, taps, dilation, 0, 0, relu, 0, 0, 0, 0};
}
Want pool2d(int comp, int in_level, int in_less, int out_level, int act_level, int out_less,
            int height, int pool_height, int taps, int pool_channel, int dilation) {
  return {TimeLaunch::kPool2d, comp, in_level, in_less, out_level, act_level, out_less, height,
          0, 0, taps, dilation, 0, 0, 0, pool_height, pool_channel, 0, 0};
}
Want epilogue(int comp, int in_level, int in_less, int out_level, int act_level, int out_less,
              int taps, int pool_channel, int dilation) {
  return {TimeLaunch::kEpilogue, comp, in_level, in_less, out_level, act_level, out_less, 0, 0,
          0, taps, dilation, 0, 0, 0, 0, pool_channel, 0, 0};
}
// (out_less is not read: a gather's rows are the result rows)
Want gather(int level, int in_less, int height, int positions, int dilation, int context) {
  return {height > 0 ? TimeLaunch::kGather2d : TimeLaunch::kGather, level, level, in_less, -1,
          -1, 0, height, 0, 0, 0, dilation, 0, 0, 0, 0, 0, positions, context};
}

const TimeLaunch::Op kTaps = TimeLaunch::kConvTaps, kConv = TimeLaunch::kConv;

// ---- the tables: {whole utterances, a streaming step} ---------------------------
struct Tables {
  std::vector<Want> utterance, stream;
};

// Splice 40 x 21; conv kw 4 -> 128, ReLU; conv kw 3 -> 128, ReLU; conv kw 3 ->
// 256, ReLU; conv kw 3 -> 256; pool 1 x 2 x 1, ReLU; conv kw 3 -> 512 (dilation
// 2), ReLU; conv kw 3 -> 512, ReLU.  Reaches 3 0 2 0 2 0 2 1 0 4 0 4 0.
Tables nnet_config_tables() {
  return {{conv(kTaps, 1, 0, 0, 1, -1, 3, 4, 1, 1, 40, 0),
           epilogue(2, 1, 3, -1, 2, 3, 1, 1, 1),
           conv(kTaps, 3, 2, 3, 3, -1, 5, 3, 1, 3, 1, 0),
           epilogue(4, 3, 5, -1, 4, 5, 1, 1, 1),
           conv(kTaps, 5, 4, 5, 5, -1, 7, 3, 1, 3, 1, 0),
           epilogue(6, 5, 7, -1, 6, 7, 1, 1, 1),
           conv(kTaps, 7, 6, 7, 7, -1, 9, 3, 1, 3, 1, 0),
           epilogue(8, 7, 9, 8, 9, 10, 2, 1, 1),
           conv(kTaps, 10, 9, 10, 10, -1, 14, 3, 2, 3, 1, 0),
           epilogue(11, 10, 14, -1, 11, 14, 1, 1, 2),
           conv(kTaps, 12, 11, 14, 12, -1, 18, 3, 2, 3, 1, 0),
           epilogue(13, 12, 18, -1, 13, 18, 1, 1, 2),
           gather(13, 18, 0, 2, 2, 20)},
          {conv(kConv, 1, 0, 0, -1, 2, 3, 4, 1, 1, 40, 1),
           conv(kConv, 3, 2, 3, -1, 4, 5, 3, 1, 3, 1, 1),
           conv(kConv, 5, 4, 5, -1, 6, 7, 3, 1, 3, 1, 1),
           conv(kConv, 7, 6, 7, 7, -1, 9, 3, 1, 3, 1, 0),
           epilogue(8, 7, 9, 8, 9, 10, 2, 1, 1),
           conv(kConv, 10, 9, 10, -1, 11, 14, 3, 2, 3, 1, 1),
           conv(kConv, 12, 11, 14, -1, 13, 18, 3, 2, 3, 1, 1),
           gather(13, 18, 0, 2, 2, 20)}};
}

// Splice 40 x 11; conv 8 x 1 -> 128 (H 33); pool 1 x 1 x 4; ReLU.  No reach.
Tables freq_conv_tables() {
  const std::vector<Want> both = {conv2d(1, 0, 0, 1, -1, 0, 40, 1, 8, 1, 1, 0),
                                  pool2d(2, 1, 0, 2, 3, 0, 33, 1, 1, 4, 1),
                                  gather(3, 0, 33, 11, 1, 10)};
  return {both, both};
}

// F: Splice 7 x 6; conv 3 x 1 -> 6 (H 5); pool 1 x 1 x 3; ReLU.  No reach.
const char *kNetF =
    "SpliceComponent input-dim=7 left-context=2 right-context=3 const-component-dim=0\n"
    "ConvolutionComponent in-height=7 in-width=6 in-channel=1 kernel-height=3 kernel-width=1 "
    "stride=1 group=6 out-height=5 out-width=6\n"
    "MaxpoolComponent in-height=5 in-width=6 in-channel=6 pool-height-dim=1 pool-width-dim=1 "
    "pool-channel-dim=3\n"
    "RectifiedLinearComponent dim=60\n"
    "FullyConnectedComponent input-dim=60 output-dim=9\n"
    "SoftmaxComponent dim=9\n";
Tables net_f_tables() {
  const std::vector<Want> both = {conv2d(1, 0, 0, 1, -1, 0, 7, 1, 3, 1, 1, 0),
                                  pool2d(2, 1, 0, 2, 3, 0, 5, 1, 1, 3, 1),
                                  gather(3, 0, 5, 6, 1, 5)};
  return {both, both};
}

// M: Splice 8 x 7; conv 3 x 2 -> 8 (H 6, n 6); ReLU; pool 2 x 2 x 1 (H 3, n 3,
// dilation 2); ReLU; conv 2 x 2 -> 12 (H 2, n 2); ReLU; conv 2 x 2 -> 16 (H 1, n
// 1); ReLU.  Reaches 1 0 1 0 2 0 2 0.
const char *kNetM =
    "SpliceComponent input-dim=8 left-context=3 right-context=3 const-component-dim=0\n"
    "ConvolutionComponent in-height=8 in-width=7 in-channel=1 kernel-height=3 kernel-width=2 "
    "stride=1 group=8 out-height=6 out-width=6\n"
    "RectifiedLinearComponent dim=288\n"
    "MaxpoolComponent in-height=6 in-width=6 in-channel=8 pool-height-dim=2 pool-width-dim=2 "
    "pool-channel-dim=1\n"
    "RectifiedLinearComponent dim=72\n"
    "ConvolutionComponent in-height=3 in-width=3 in-channel=8 kernel-height=2 kernel-width=2 "
    "stride=1 group=12 out-height=2 out-width=2\n"
    "RectifiedLinearComponent dim=48\n"
    "ConvolutionComponent in-height=2 in-width=2 in-channel=12 kernel-height=2 kernel-width=2 "
    "stride=1 group=16 out-height=1 out-width=1\n"
    "RectifiedLinearComponent dim=16\n"
    "FullyConnectedComponent input-dim=16 output-dim=10\n"
    "SoftmaxComponent dim=10\n";
Tables net_m_tables() {
  return {{conv2d(1, 0, 0, 1, -1, 1, 8, 1, 3, 2, 1, 0),
           epilogue(2, 1, 1, -1, 2, 1, 1, 1, 1),
           pool2d(3, 2, 1, 3, 4, 2, 6, 2, 2, 1, 1),
           conv2d(5, 4, 2, 5, -1, 4, 3, 8, 2, 2, 2, 0),
           epilogue(6, 5, 4, -1, 6, 4, 1, 1, 2),
           conv2d(7, 6, 4, 7, -1, 6, 2, 12, 2, 2, 2, 0),
           epilogue(8, 7, 6, -1, 8, 6, 1, 1, 2),
           gather(8, 6, 0, 1, 2, 6)},
          {conv2d(1, 0, 0, -1, 2, 1, 8, 1, 3, 2, 1, 1),
           pool2d(3, 2, 1, 3, 4, 2, 6, 2, 2, 1, 1),
           conv2d(5, 4, 2, -1, 6, 4, 3, 8, 2, 2, 2, 1),
           conv2d(7, 6, 4, -1, 8, 6, 2, 12, 2, 2, 2, 1),
           gather(8, 6, 0, 1, 2, 6)}};
}

// Splice 8 x 11; conv kw 4 -> 32, ReLU; conv kw 3 -> 32; pool 1 x 2 x pc; ReLU;
// conv kw 2 -> 64 (dilation 2); ReLU.  Reaches 3 0 2 1 0 2 0.
std::string shrunken(int pc) {
  const std::string c2 = std::to_string(32 / pc);
  return "SpliceComponent input-dim=8 left-context=5 right-context=5 const-component-dim=0\n"
         "ConvolutionComponent in-height=8 in-width=11 in-channel=1 kernel-height=8 "
         "kernel-width=4 stride=1 group=32 out-height=1 out-width=8\n"
         "RectifiedLinearComponent dim=256\n"
         "ConvolutionComponent in-height=1 in-width=8 in-channel=32 kernel-height=1 "
         "kernel-width=3 stride=1 group=32 out-height=1 out-width=6\n"
         "MaxpoolComponent in-height=1 in-width=6 in-channel=32 pool-height-dim=1 "
         "pool-width-dim=2 pool-channel-dim=" + std::to_string(pc) + "\n"
         "RectifiedLinearComponent dim=" + std::to_string(3 * (32 / pc)) + "\n"
         "ConvolutionComponent in-height=1 in-width=3 in-channel=" + c2 + " kernel-height=1 "
         "kernel-width=2 stride=1 group=64 out-height=1 out-width=2\n"
         "RectifiedLinearComponent dim=128\n"
         "FullyConnectedComponent input-dim=128 output-dim=10\n";
}
Tables shrunken_tables(int pc) {
  return {{conv(kTaps, 1, 0, 0, 1, -1, 3, 4, 1, 1, 8, 0),
           epilogue(2, 1, 3, -1, 2, 3, 1, 1, 1),
           conv(kTaps, 3, 2, 3, 3, -1, 5, 3, 1, 3, 1, 0),
           epilogue(4, 3, 5, 4, 5, 6, 2, pc, 1),
           conv(kTaps, 6, 5, 6, 6, -1, 8, 2, 2, 2, 1, 0),
           epilogue(7, 6, 8, -1, 7, 8, 1, 1, 2),
           gather(7, 8, 0, 2, 2, 10)},
          {conv(kConv, 1, 0, 0, -1, 2, 3, 4, 1, 1, 8, 1),
           conv(kConv, 3, 2, 3, 3, -1, 5, 3, 1, 3, 1, 0),
           epilogue(4, 3, 5, 4, 5, 6, 2, pc, 1),
           conv(kConv, 6, 5, 6, -1, 7, 8, 2, 2, 2, 1, 1),
           gather(7, 8, 0, 2, 2, 10)}};
}

// ---- the checks -------------------------------------------------------------------
void print_launch(const TimeLaunch &t) {
  printf("  %-9s comp %2d  in %2d x %-3d  out %2d act %2d  rows %-3d  H %d C %d kh %d taps %d "
         "delta %d wc %d wd %d relu %d ph %d pc %d n %d context %d\n",
         kOpNames[t.op], t.comp, t.in_level, t.in_rows, t.out_level, t.act_level, t.rows,
         t.height, t.channels, t.kernel_height, t.taps, t.dilation, t.wc, t.wd, t.relu,
         t.pool_height, t.pool_channel, t.positions, t.context);
}

void check_table(const std::vector<TimeLaunch> &got, const std::vector<Want> &want,
                 int input_rows, int result_rows) {
  expect(got.size() == want.size(), "the number of launches", (long)got.size(),
         (long)want.size());
  for (size_t i = 0; i < got.size() && i < want.size(); i++) {
    const TimeLaunch &t = got[i];
    const Want &w = want[i];
    const bool last = w.out_level < 0 && w.act_level < 0;
    expect(t.op == w.op && t.comp == w.comp, "a launch's op and component", (long)i, t.op);
    expect(t.in_level == w.in_level && t.out_level == w.out_level && t.act_level == w.act_level,
           "a launch's levels", (long)i, t.in_level);
    expect(t.in_rows == input_rows - w.in_less &&
               t.rows == (last ? result_rows : input_rows - w.out_less),
           "a launch's rows", (long)i, t.rows);
    expect(t.height == w.height && t.channels == w.channels &&
               t.kernel_height == w.kernel_height && t.taps == w.taps &&
               t.dilation == w.dilation && t.wc == w.wc && t.wd == w.wd && t.relu == w.relu &&
               t.pool_height == w.pool_height && t.pool_channel == w.pool_channel &&
               t.positions == w.positions && t.context == w.context,
           "a launch's integer arguments", (long)i);
  }
}

bool is_gather(const TimeLaunch &t) {
  return t.op == TimeLaunch::kGather || t.op == TimeLaunch::kGather2d;
}

void check_invariants(const TimePlan &plan, const TimeRows &rows,
                      const std::vector<TimeLaunch> &got, bool stream) {
  const int p = plan.prefix();
  std::vector<int> written((size_t)p, 0);
  written[0] = 1;
  expect(!got.empty() && is_gather(got.back()), "the last launch is a gather");
  for (size_t i = 0; i < got.size(); i++) {
    const TimeLaunch &t = got[i];
    expect(t.in_level >= 0 && t.in_level < p && written[(size_t)t.in_level] == 1,
           "a launch reads a level written before it", (long)i, t.in_level);
    expect(t.comp >= 1 && t.comp < p, "a launch's component", (long)i, t.comp);
    if (t.in_level < 0 || t.in_level >= p || t.comp < 1 || t.comp >= p) continue;
    expect(t.in_rows == rows.computed[(size_t)t.in_level], "a launch reads the computed rows",
           (long)i);
    if (is_gather(t)) {
      const TimeLevel &top = plan.levels[(size_t)p - 1];
      expect(i + 1 == got.size() && t.in_level == p - 1 && t.rows == rows.result_rows,
             "the one gather is last and reads the top level", (long)i);
      // the last window's highest row is one of the rows read
      expect(rows.base.back() + rows.frames.back() - 1 +
                     (int64_t)top.dilation * (top.positions - 1) < t.in_rows,
             "the gather's windows lie in the rows read", (long)i);
      continue;
    }
    expect(t.in_level == t.comp - 1, "a level launch reads the level below", (long)i);
    expect(t.in_rows >= t.rows + plan.levels[(size_t)t.comp].reach,
           "the rows read hold the last row's highest tap", (long)i, t.in_rows);
    for (int l : {t.out_level, t.act_level}) {
      if (l < 0) continue;
      expect(l < p && (l == t.comp || l == t.comp + 1), "a launch writes its own levels",
             (long)i, l);
      if (l < p) written[(size_t)l]++;
      if (l < p) expect(t.rows == rows.computed[(size_t)l], "a level's rows", (long)i, l);
    }
    expect(t.out_level >= 0 || t.act_level >= 0, "a level launch writes a level", (long)i);
    if (stream) {
      expect(t.op != TimeLaunch::kConvTaps, "a streaming step has no per-tap GEMMs", (long)i);
    } else {
      expect(t.op != TimeLaunch::kConv && t.relu == 0,
             "whole utterances: no kn_timemap_conv and no fused ReLU", (long)i);
    }
  }
  for (int l = 1; l < p; l++) {
    const bool skipped = stream && plan.levels[(size_t)l].kind == TimeComp::kConv && l + 1 < p &&
                         plan.levels[(size_t)l + 1].kind == TimeComp::kRelu;
    expect(written[(size_t)l] == (skipped ? 0 : 1), "the levels written, each once", l,
           written[(size_t)l]);
  }
}

void check_net(const char *name, const std::string &config, int prefix, const Tables &tables) {
  const std::vector<TimeComp> comps = parse_config(config);
  const TimePlan plan = kcnn::make_time_plan(comps, false, true);
  expect(plan.prefix() == prefix, "a net's prefix", plan.prefix(), prefix);
  if (plan.prefix() != prefix) {
    printf("  %s declined: %s\n", name, plan.declined.c_str());
    return;
  }
  const int context = comps[0].left + comps[0].right;
  const std::vector<int32_t> frames = {1, 7, 23, 2};
  for (int pad = 1; pad >= 0; pad--) {
    std::vector<int32_t> lengths = frames;
    if (!pad)
      for (int32_t &t : lengths) t += context;
    TimeRows rows;
    const std::string bad = kcnn::plan_time_rows(plan, lengths.data(), 4, pad != 0, &rows);
    expect(bad.empty(), "plan_time_rows", (long)bad.size());
    if (!bad.empty()) continue;
    for (int stream = 0; stream < 2; stream++) {
      const TimeRoute route = stream ? kcnn::kStreamRoute : kcnn::kUtteranceRoute;
      const std::vector<TimeLaunch> got = kcnn::time_schedule(plan, rows, route);
      printf("%s %s, %s: %d launches\n", name, pad ? "padded" : "unpadded",
             stream ? "a streaming step" : "whole utterances", (int)got.size());
      for (const TimeLaunch &t : got) print_launch(t);
      check_table(got, stream ? tables.stream : tables.utterance, 33 + 4 * context, 33);
      check_invariants(plan, rows, got, stream != 0);
    }
  }
}

std::string slurp(const char *path) {
  std::ifstream f(path);
  std::ostringstream s;
  s << f.rdbuf();
  return s.str();
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    printf("usage: %s nnet.config freq_conv.config\n", argv[0]);
    return 2;
  }
  check_net("nnet.config", slurp(argv[1]), 14, nnet_config_tables());
  check_net("freq_conv.config", slurp(argv[2]), 4, freq_conv_tables());
  check_net("net F", kNetF, 4, net_f_tables());
  check_net("net M", kNetM, 9, net_m_tables());
  check_net("shrunken", shrunken(1), 8, shrunken_tables(1));
  check_net("shrunken pc 4", shrunken(4), 8, shrunken_tables(4));
  {  // a declined plan has no launches
    const TimePlan none = kcnn::make_time_plan(parse_config(kNetM), true, true);
    expect(none.prefix() == 0, "the literal path declines");
    expect(kcnn::time_schedule(none, TimeRows(), kcnn::kUtteranceRoute).empty() &&
               kcnn::time_schedule(none, TimeRows(), kcnn::kStreamRoute).empty(),
           "an empty plan gives an empty schedule");
  }
  if (failures) {
    printf("REFUSED: %d of %ld time schedule checks failed\n", failures, checks);
    return 1;
  }
  printf("all time schedule checks passed (%ld)\n", checks);
  return 0;
}
