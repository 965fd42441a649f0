// scripts/time_plan_height_check.cc -- the host plan of the time-shared forward
// with HEIGHT MAPS (kaldi-cnn_amd/src/capi/time-plan.h, make_time_plan's third
// parameter: levels (C, H, n, delta) that keep a frequency axis) as a
// stand-alone host program, for a run under a host sanitizer.  No GPU call.
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Ikaldi-cnn_amd/src scripts/time_plan_height_check.cc -o time_plan_height_check
//   ./time_plan_height_check tests/golden/freq_conv.config
//
// 1. The (C, H, n, delta) chains of nets F and M (below) and of
//    freq_conv.config, the values written out; which levels run on the
//    height-map kernels.
// 2. Every decline height maps add, and the two-argument call on net F.
// 3. plan_time_rows on utterances of (1, 7, 23, 2) frames, padded and not
//    (unpadded: that many RESULT frames).
// 4. A host model of the whole pass on integer data -- the maps by the
//    formulas of nnet-kernels.h (kn_timemap_conv2d, kn_timemap_pool2d, the
//    ReLU), every access checked against the rows computed, then the gather
//    (kn_timemap_gather2d) -- against the window pass: each frame's own window
//    through the same layers in the window layout of the reference (h + w H +
//    c H W).  Every sum is exact, so the two are compared with ==.
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <random>

#include "time_plan_config.h"

using kcnn::TimeComp;
using kcnn::TimeLevel;
using kcnn::TimePlan;
using kcnn::TimeRows;

namespace {

// ---- config lines ---------------------------------------------------------------
std::string conv_line(int h, int w, int c, int kh, int kw, int g, const char *extra = "",
                      int oh = -1) {
  std::ostringstream s;
  s << "ConvolutionComponent in-height=" << h << " in-width=" << w << " in-channel=" << c
    << " kernel-height=" << kh << " kernel-width=" << kw << " stride=1 group=" << g
    << " out-height=" << (oh < 0 ? h - kh + 1 : oh) << " out-width=" << w - kw + 1 << " "
    << extra << "\n";
  return s.str();
}
std::string pool_line(int h, int w, int c, int ph, int pw, int pc) {
  std::ostringstream s;
  s << "MaxpoolComponent in-height=" << h << " in-width=" << w << " in-channel=" << c
    << " pool-height-dim=" << ph << " pool-width-dim=" << pw << " pool-channel-dim=" << pc << "\n";
  return s.str();
}
std::string splice_line(int d, int l, int r) {
  std::ostringstream s;
  s << "SpliceComponent input-dim=" << d << " left-context=" << l << " right-context=" << r
    << " const-component-dim=0\n";
  return s.str();
}
std::string relu_line(int dim) {
  return "RectifiedLinearComponent dim=" + std::to_string(dim) + "\n";
}
std::string fc_line(int i, int o) {
  return "FullyConnectedComponent input-dim=" + std::to_string(i) + " output-dim=" +
         std::to_string(o) + "\n";
}

// F, c2 shrunken: Splice d 7, L 2, R 3; conv 3 x 1 -> 6 (H 5, n 6); pool 1 x 1 x
// 3; ReLU 60; FC; Softmax
std::string net_f() {
  return splice_line(7, 2, 3) + conv_line(7, 6, 1, 3, 1, 6) + pool_line(5, 6, 6, 1, 1, 3) +
         relu_line(60) + fc_line(60, 9) + "SoftmaxComponent dim=9\n";
}
// M, every kind of level: Splice d 8, L 3, R 3; conv 3 x 2 -> 8 (H 6, n 6); ReLU;
// pool 2 x 2 x 1 (H 3, n 3, delta 2); ReLU; conv 2 x 2 -> 12 (H 2, n 2); ReLU;
// conv 2 x 2 -> 16, the full height (H 1, n 1); ReLU; FC; Softmax
std::string net_m() {
  return splice_line(8, 3, 3) + conv_line(8, 7, 1, 3, 2, 8) + relu_line(288) +
         pool_line(6, 6, 8, 2, 2, 1) + relu_line(72) + conv_line(3, 3, 8, 2, 2, 12) +
         relu_line(48) + conv_line(2, 2, 12, 2, 2, 16) + relu_line(16) + fc_line(16, 10) +
         "SoftmaxComponent dim=10\n";
}

struct Chnd {
  int c, h, n, d;
  bool two_d;  // runs on the height-map kernels
};

void check_chain(const char *name, const std::vector<TimeComp> &comps,
                 const std::vector<Chnd> &want) {
  const TimePlan plan = kcnn::make_time_plan(comps, false, true);
  expect(plan.prefix() == (int)want.size(), name, plan.prefix(), (long)want.size());
  if (plan.prefix() != (int)want.size()) {
    printf("  declined: %s\n", plan.declined.c_str());
    return;
  }
  for (size_t l = 0; l < want.size(); l++) {
    const TimeLevel &lev = plan.levels[l];
    expect(lev.channels == want[l].c && lev.height == want[l].h &&
               lev.positions == want[l].n && lev.dilation == want[l].d,
           "a level's (C, H, n, delta)", (long)l, lev.channels * 1000 + lev.height);
    expect(lev.width == lev.channels * lev.height, "a level's width", (long)l, lev.width);
    if (l > 0)
      expect(kcnn::time_level_2d(plan, (int)l) == want[l].two_d, "a level's kernels", (long)l);
  }
  const TimeLevel &top = plan.levels.back();
  printf("%s: prefix %d, ending at (%d, %d, %d, %d)\n", name, plan.prefix(), top.channels,
         top.height, top.positions, top.dilation);
}

void check_declines() {
  struct Case {
    const char *what, *word;  // a word of the reason
    std::string config;
  };
  const std::string sp = splice_line(8, 3, 3), tail = fc_line(10, 10);
  const std::vector<Case> cases = {
      {"in-pad-height", "in-pad-height", sp + conv_line(8, 7, 1, 3, 2, 8, "in-pad-height=1") + tail},
      {"in-pad-width", "in-pad-width", sp + conv_line(8, 7, 1, 3, 2, 8, "in-pad-width=1") + tail},
      {"kernel-height > in-height", "Convolution 1", sp + conv_line(8, 7, 1, 9, 2, 8, "", 1) + tail},
      {"a wrong out-height", "Convolution 1", sp + conv_line(8, 7, 1, 3, 2, 8, "", 5) + tail},
      {"a stride", "Convolution 1",
       sp + "ConvolutionComponent in-height=8 in-width=7 in-channel=1 kernel-height=2 "
            "kernel-width=1 stride=2 group=8 out-height=4 out-width=4\n" + tail},
      {"in-channel 2 on the Splice", "Convolution 1", sp + conv_line(4, 7, 2, 3, 2, 8) + tail},
      {"in-height that is not the level's", "Convolution 1",
       sp + conv_line(7, 7, 1, 3, 2, 8) + tail},
      {"a second Convolution of another height", "Convolution 2",
       sp + conv_line(8, 7, 1, 3, 2, 8) + conv_line(5, 6, 8, 2, 2, 4) + tail},
      {"pool-height-dim that does not divide H", "Maxpool 2",
       sp + conv_line(8, 7, 1, 3, 2, 8) + pool_line(6, 6, 8, 4, 2, 1) + tail},
      {"a pool of another height", "Maxpool 2",
       sp + conv_line(8, 7, 1, 3, 2, 8) + pool_line(3, 6, 8, 1, 2, 1) + tail},
      {"a pool on the Splice", "no Convolution", sp + pool_line(8, 7, 1, 2, 1, 1) + tail},
      {"a ReLU on the Splice", "no Convolution",
       sp + relu_line(56) + conv_line(8, 7, 1, 3, 2, 8) + tail},
  };
  for (const Case &c : cases) {
    const TimePlan plan = kcnn::make_time_plan(parse_config(c.config), false, true);
    expect(plan.prefix() == 0 && plan.declined.find(c.word) != std::string::npos, c.what,
           plan.prefix());
    printf("declined (%s): %s\n", c.what, plan.declined.c_str());
  }
  // an overlapping pool, and the literal path
  std::vector<TimeComp> over =
      parse_config(sp + conv_line(8, 7, 1, 3, 2, 8) + pool_line(6, 6, 8, 2, 2, 1));
  over.back().overlap = true;
  expect(kcnn::make_time_plan(over, false, true).prefix() == 0, "an overlapping pool");
  expect(kcnn::make_time_plan(parse_config(net_m()), true, true).prefix() == 0,
         "the literal path");
  // too many filters for one launch
  std::vector<TimeComp> wide = parse_config(net_f());
  wide[1].group = kcnn::kTimeMaxGroup2d + 1;
  expect(kcnn::make_time_plan(wide, false, true).prefix() == 0, "filters past the limit");
  // without height maps F is declined as it always was, with the same words
  const TimePlan two = kcnn::make_time_plan(parse_config(net_f()), false);
  expect(two.prefix() == 0 &&
             two.declined == "Convolution 1 is not a 1-D convolution along time of its input (1 "
                             "channels, height 7, 6 positions)",
         "the two-argument call on net F");
  printf("declined (two arguments, net F): %s\n", two.declined.c_str());
  const TimePlan two_m = kcnn::make_time_plan(parse_config(net_m()), false, false);
  expect(two_m.prefix() == 0, "the two-argument plan of net M");
  // a 1-D net gives the same plan either way
  const std::string one_d = splice_line(8, 5, 5) + conv_line(8, 11, 1, 8, 4, 32) +
                            relu_line(256) + conv_line(1, 8, 32, 1, 3, 32) +
                            pool_line(1, 6, 32, 1, 2, 4) + relu_line(24) + fc_line(24, 10);
  const TimePlan a = kcnn::make_time_plan(parse_config(one_d), false),
                 b = kcnn::make_time_plan(parse_config(one_d), false, true);
  expect(a.prefix() == 6 && b.prefix() == 6, "the 1-D net's prefix", a.prefix(), b.prefix());
  for (int l = 0; l < a.prefix() && l < b.prefix(); l++) {
    const TimeLevel &x = a.levels[(size_t)l], &y = b.levels[(size_t)l];
    expect(x.channels == y.channels && x.positions == y.positions && x.dilation == y.dilation &&
               x.width == y.width && x.taps == y.taps && x.pool_channel == y.pool_channel &&
               x.reach == y.reach && x.sum_reach == y.sum_reach && x.height == y.height &&
               y.pool_height == 1 && (l == 0 || (y.height == 1 && !kcnn::time_level_2d(b, l))),
           "a 1-D level with and without height maps", l);
  }
}

// ---- the host model of one pass ---------------------------------------------------
struct Weights {
  std::vector<std::vector<int>> w;  // [kernel row i + d kh + c kh kw][g]
  std::vector<int> b;
};

// the window pass: one frame's window row (h + w H + c H W) through component c
std::vector<long> window_layer(const TimeComp &c, const Weights &wt, const std::vector<long> &x) {
  std::vector<long> y((size_t)c.output_dim);
  if (c.kind == TimeComp::kConv) {
    const int H = c.in_height, W = c.in_width, kh = c.kernel_height, kw = c.kernel_width;
    const int OH = c.out_height, OW = c.out_width;
    for (int g = 0; g < c.group; g++)
      for (int ow = 0; ow < OW; ow++)
        for (int oh = 0; oh < OH; oh++) {
          long s = wt.b[(size_t)g];
          for (int ch = 0; ch < c.in_channel; ch++)
            for (int d = 0; d < kw; d++)
              for (int i = 0; i < kh; i++)
                s += x[(size_t)(oh + i + (ow + d) * H + ch * H * W)] *
                     wt.w[(size_t)(i + d * kh + ch * kh * kw)][(size_t)g];
          y[(size_t)(oh + ow * OH + g * OH * OW)] = s;
        }
  } else if (c.kind == TimeComp::kPool) {
    const int H = c.in_height, W = c.in_width;
    const int OH = H / c.pool_height, OW = W / c.pool_width;
    for (int oc = 0; oc < c.in_channel / c.pool_channel; oc++)
      for (int ow = 0; ow < OW; ow++)
        for (int oh = 0; oh < OH; oh++) {
          long v = -(1L << 40);
          for (int ch = 0; ch < c.pool_channel; ch++)
            for (int w = 0; w < c.pool_width; w++)
              for (int h = 0; h < c.pool_height; h++) {
                const long xv = x[(size_t)(oh * c.pool_height + h + (ow * c.pool_width + w) * H +
                                           (oc * c.pool_channel + ch) * H * W)];
                if (v < xv) v = xv;
              }
          y[(size_t)(oh + ow * OH + oc * OH * OW)] = v;
        }
  } else {
    for (size_t i = 0; i < x.size(); i++) y[i] = x[i] < 0 ? 0 : x[i];
  }
  return y;
}

struct Map {
  int64_t rows = 0;  // computed
  int width = 0;
  std::vector<long> v;
  long at(int64_t r, int c) const {
    if (r < 0 || r >= rows || c < 0 || c >= width) {
      printf("WRONG: map access (%ld, %d) outside %ld x %d\n", (long)r, c, (long)rows, width);
      exit(1);
    }
    return v[(size_t)(r * width + c)];
  }
};

void run_model(const char *name, const std::string &config, const std::vector<int32_t> &frames,
               bool pad, unsigned seed) {
  const std::vector<TimeComp> comps = parse_config(config);
  const TimePlan plan = kcnn::make_time_plan(comps, false, true);
  expect(plan.prefix() > 1, "the model's plan", plan.prefix());
  if (plan.prefix() < 2) return;
  const int p = plan.prefix(), L = comps[0].left, R = comps[0].right, context = L + R;
  const int dim = comps[0].input_dim;
  std::vector<int32_t> lengths = frames;
  if (!pad)
    for (int32_t &t : lengths) t += context;
  TimeRows rows;
  const std::string bad =
      kcnn::plan_time_rows(plan, lengths.data(), (int)lengths.size(), pad, &rows);
  expect(bad.empty(), "plan_time_rows", (long)bad.size());
  if (!bad.empty()) {
    printf("REFUSED: %s\n", bad.c_str());
    return;
  }
  int64_t base = 0, total = 0;
  for (size_t u = 0; u < frames.size(); u++) {
    expect(rows.base[u] == base && rows.frames[u] == frames[u], "an utterance's base and frames",
           (long)u);
    base += frames[u] + context;
    total += frames[u];
  }
  expect(rows.input_rows == base && rows.result_rows == total, "the rows of the pass");
  for (int l = 0; l < p; l++)
    expect(rows.computed[(size_t)l] == base - plan.levels[(size_t)l].sum_reach,
           "a level's computed rows", l);

  std::mt19937 gen(seed);
  auto draw = [&](int lo, int hi) { return (int)(gen() % (unsigned)(hi - lo + 1)) + lo; };
  std::vector<Weights> wts((size_t)p);
  for (int l = 1; l < p; l++)
    if (comps[(size_t)l].kind == TimeComp::kConv) {
      const TimeComp &c = comps[(size_t)l];
      wts[(size_t)l].w.assign((size_t)(c.kernel_height * c.kernel_width * c.in_channel),
                              std::vector<int>((size_t)c.group));
      for (auto &row : wts[(size_t)l].w)
        for (int &x : row) x = draw(-1, 1);
      wts[(size_t)l].b.resize((size_t)c.group);
      for (int &x : wts[(size_t)l].b) x = draw(-2, 2);
    }
  // the utterances, and level 0: the frames, clamped when padded
  std::vector<std::vector<long>> utts;
  for (int32_t t : lengths) {
    utts.emplace_back((size_t)t * dim);
    for (long &x : utts.back()) x = draw(-2, 2);
  }
  std::vector<Map> maps((size_t)p);
  maps[0].rows = rows.input_rows;
  maps[0].width = dim;
  for (size_t u = 0; u < utts.size(); u++) {
    const int T = lengths[u];
    for (int64_t r = 0; r < frames[u] + context; r++) {
      int64_t src = pad ? r - L : r;
      src = src < 0 ? 0 : (src > T - 1 ? T - 1 : src);
      for (int c = 0; c < dim; c++) maps[0].v.push_back(utts[u][(size_t)(src * dim + c)]);
    }
  }
  expect((int64_t)maps[0].v.size() == rows.input_rows * dim, "level 0's size");
  // the maps
  for (int l = 1; l < p; l++) {
    const TimeLevel &lev = plan.levels[(size_t)l], &below = plan.levels[(size_t)l - 1];
    const Map &in = maps[(size_t)l - 1];
    Map &out = maps[(size_t)l];
    out.rows = rows.computed[(size_t)l];
    out.width = lev.width;
    out.v.assign((size_t)(out.rows * out.width), 0);
    const int H = below.height, C = below.channels, OH = lev.height, delta = below.dilation;
    for (int64_t s = 0; s < out.rows; s++) {
      if (lev.kind == TimeComp::kConv) {
        const int kh = H - OH + 1, kw = lev.taps;
        for (int g = 0; g < lev.channels; g++)
          for (int oh = 0; oh < OH; oh++) {
            long sum = wts[(size_t)l].b[(size_t)g];
            for (int d = 0; d < kw; d++)
              for (int c = 0; c < C; c++)
                for (int i = 0; i < kh; i++)
                  sum += in.at(s + (int64_t)delta * d, oh + i + c * H) *
                         wts[(size_t)l].w[(size_t)(i + d * kh + c * kh * kw)][(size_t)g];
            out.v[(size_t)(s * out.width + oh + g * OH)] = sum;
          }
      } else if (lev.kind == TimeComp::kPool) {
        const int ph = lev.pool_height, pw = lev.taps, pc = lev.pool_channel;
        for (int oc = 0; oc < lev.channels; oc++)
          for (int oh = 0; oh < OH; oh++) {
            long v = -(1L << 40);
            for (int c = 0; c < pc; c++)
              for (int w = 0; w < pw; w++)
                for (int h = 0; h < ph; h++) {
                  const long x = in.at(s + (int64_t)delta * w, oh * ph + h + (oc * pc + c) * H);
                  if (v < x) v = x;
                }
            out.v[(size_t)(s * out.width + oh + oc * OH)] = v;
          }
      } else {
        for (int c = 0; c < out.width; c++) {
          const long x = in.at(s, c);
          out.v[(size_t)(s * out.width + c)] = x < 0 ? 0 : x;
        }
      }
    }
  }
  // the gather against the window pass
  const TimeLevel &top = plan.levels[(size_t)p - 1];
  const int H = top.height, n = top.positions;
  long compared = 0;
  for (size_t u = 0; u < utts.size(); u++)
    for (int64_t t = 0; t < frames[u]; t++) {
      // the frame's window: element (h, k) is level 0's row base + t + k
      std::vector<long> x((size_t)(dim * (context + 1)));
      for (int k = 0; k <= context; k++)
        for (int h = 0; h < dim; h++)
          x[(size_t)(h + k * dim)] = maps[0].at(rows.base[u] + t + k, h);
      for (int l = 1; l < p; l++) x = window_layer(comps[(size_t)l], wts[(size_t)l], x);
      expect((int)x.size() == top.width * n, "the window row's size", (long)x.size());
      for (int c = 0; c < top.channels; c++)
        for (int k = 0; k < n; k++)
          for (int h = 0; h < H; h++) {
            const long got =
                maps[(size_t)p - 1].at(rows.base[u] + t + (int64_t)top.dilation * k, h + c * H);
            const long want = x[(size_t)(h + k * H + c * H * n)];
            if (got != want) expect(false, "the gathered map against the window pass", got, want);
            compared++;
          }
    }
  checks += compared;
  printf("%s %s: %ld elements equal the window pass\n", name, pad ? "padded" : "unpadded",
         compared);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    printf("usage: %s freq_conv.config\n", argv[0]);
    return 2;
  }
  std::ifstream f(argv[1]);
  const std::string golden((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  if (golden.empty()) {
    printf("cannot read %s\n", argv[1]);
    return 2;
  }
  check_chain("net F", parse_config(net_f()),
              {{1, 7, 6, 1, false}, {6, 5, 6, 1, true}, {2, 5, 6, 1, true}, {2, 5, 6, 1, false}});
  check_chain("net M", parse_config(net_m()),
              {{1, 8, 7, 1, false}, {8, 6, 6, 1, true}, {8, 6, 6, 1, false}, {8, 3, 3, 2, true},
               {8, 3, 3, 2, false}, {12, 2, 2, 2, true}, {12, 2, 2, 2, false},
               {16, 1, 1, 2, true}, {16, 1, 1, 2, false}});
  check_chain("freq_conv.config", parse_config(golden),
              {{1, 40, 11, 1, false}, {128, 33, 11, 1, true}, {32, 33, 11, 1, true},
               {32, 33, 11, 1, false}});
  check_declines();
  const std::vector<int32_t> frames = {1, 7, 23, 2};
  for (int pad = 0; pad < 2; pad++) {
    run_model("net F", net_f(), frames, pad != 0, 11);
    run_model("net M", net_m(), frames, pad != 0, 12);
  }
  // a height level whose rows x height pass 2^31 - 1 is refused by the rows' plan
  {
    const TimePlan plan = kcnn::make_time_plan(parse_config(golden), false, true);
    const int32_t big[1] = {70000000};  // x 33 > 2^31
    TimeRows rows;
    const std::string bad = kcnn::plan_time_rows(plan, big, 1, true, &rows);
    expect(bad.find("too many") != std::string::npos, "rows x height past 32 bits",
           (long)bad.size());
    printf("refused (70000000 frames of freq_conv.config): %s\n", bad.c_str());
  }
  if (failures) {
    printf("%d of %ld time plan height checks FAILED\n", failures, checks);
    return 1;
  }
  printf("all time plan height checks passed (%ld)\n", checks);
  return 0;
}
