// scripts/time_backward_check.cc -- the host plan of a training step over time
// maps (kaldi-cnn_amd/src/capi/frame-index.h: frame_runs, stage_runs;
// time-plan.h: time_train_plan, plan_train_rows, time_backward_schedule) as a
// stand-alone host program, for a run under a host sanitizer.  No GPU call.
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Ikaldi-cnn_amd/src scripts/time_backward_check.cc -o time_backward_check
//   ./time_backward_check tests/golden/nnet.config tests/golden/freq_conv.config
//
// On a corpus of 3 utterances (7, 23, 40 frames; the first shorter than L + R
// of the shrunken nets), on one list written out by hand and on random lists,
// for the shrunken 1-D nets (pool-channel-dim 1 and 4) and nnet.config:
// 1. the runs against a naive restatement (entry by entry: the same run as the
//    entry before when the row follows it in the same utterance), their
//    lengths summing to the list's, and the staged image;
// 2. result row n's window at level 0: map row base_j + t + k, k < L + R + 1,
//    is corpus row clamp(frames[n] - L + k, s, e - 1);
// 3. every launch of the forward and of the backward schedule reads and writes
//    inside the rows of its maps; the backward writes every derivative map it
//    reads before reading it, top level first, the scatter first, one launch
//    per forward launch, no data gradient for the convolution on level 0;
// 4. a plan with a height level (freq_conv.config) gives training prefix 0,
//    nnet.config 14, the shrunken nets 8;
// 5. oversize passes are refused by arithmetic alone.
#include <fstream>
#include <random>

#include "time_plan_config.h"

using kcnn::CorpusIndex;
using kcnn::FrameRun;
using kcnn::TimeBackLaunch;
using kcnn::TimeComp;
using kcnn::TimeLaunch;
using kcnn::TimePlan;
using kcnn::TimeRows;

namespace {

const char *kConv =
    "ConvolutionComponent in-height=%d in-width=%d in-channel=%d kernel-height=%d "
    "kernel-width=%d stride=1 group=%d out-height=1 out-width=%d\n";

// tests/test_gpu_compute_shared.py's shrunken(channel_pool)
std::string shrunken(bool channel_pool) {
  const int pw = channel_pool ? 1 : 2, pc = channel_pool ? 4 : 1;
  const int w = 6 / pw, c = 32 / pc;
  char buf[4096];
  std::string s =
      "SpliceComponent input-dim=8 left-context=5 right-context=5 const-component-dim=0\n";
  snprintf(buf, sizeof buf, kConv, 8, 11, 1, 8, 4, 32, 8);
  s += buf;
  s += "RectifiedLinearComponent dim=256\n";
  snprintf(buf, sizeof buf, kConv, 1, 8, 32, 1, 3, 32, 6);
  s += buf;
  snprintf(buf, sizeof buf,
           "MaxpoolComponent in-height=1 in-width=6 in-channel=32 pool-height-dim=1 "
           "pool-width-dim=%d pool-channel-dim=%d\n", pw, pc);
  s += buf;
  snprintf(buf, sizeof buf, "RectifiedLinearComponent dim=%d\n", w * c);
  s += buf;
  snprintf(buf, sizeof buf, kConv, 1, w, c, 1, 2, 64, w - 1);
  s += buf;
  snprintf(buf, sizeof buf, "RectifiedLinearComponent dim=%d\n", (w - 1) * 64);
  s += buf;
  snprintf(buf, sizeof buf, "FullyConnectedComponent input-dim=%d output-dim=10\n", (w - 1) * 64);
  s += buf;
  s += "SoftmaxComponent dim=10\n";
  return s;
}

std::string read_file(const char *path) {
  std::ifstream f(path);
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

// The list of tests/test_gpu_train_shared.py on utterances [0, 7), [7, 30), [30, 70).
std::vector<int32_t> hand_list() {
  std::vector<int32_t> f;
  auto run = [&](int a, int n) { for (int i = 0; i < n; i++) f.push_back(a + i); };
  run(0, 7);    // the whole first utterance: clamps at both ends
  run(7, 5);    // list-adjacent and consecutive across the boundary: must split
  run(41, 1);   // a run of 1
  run(25, 5);   // ends at an utterance's last row ...
  run(30, 6);   // ... and the next starts at the first row of the next: must split
  run(50, 8);   // the same run twice
  run(50, 8);
  f.push_back(20); f.push_back(19); f.push_back(18);  // descending: three runs
  run(62, 8);   // ends at the corpus's last row
  return f;
}

void check_runs(const CorpusIndex &corpus, const std::vector<int32_t> &f,
                std::vector<FrameRun> *out) {
  const std::vector<FrameRun> runs = kcnn::frame_runs(corpus, f.data(), (int)f.size());
  // naive: the utterance of a row by a scan; entry i continues entry i - 1's run or not
  auto utt = [&](int32_t r) {
    int u = 0;
    while (corpus.starts[(size_t)u + 1] <= r) u++;
    return u;
  };
  size_t j = 0;
  int32_t at = 0;
  long total = 0;
  for (size_t i = 0; i < f.size(); i++) {
    const bool cont = i > 0 && f[i] == f[i - 1] + 1 && utt(f[i]) == utt(f[i - 1]);
    if (i > 0 && !cont) { j++; at = 0; }
    expect(j < runs.size(), "a run for every entry", (long)i, (long)j);
    if (j >= runs.size()) return;
    const int u = utt(f[i]);
    expect(runs[j].first + at == f[i], "entry i is row `at` of its run", (long)i, f[i]);
    expect(runs[j].lo == corpus.starts[(size_t)u] && runs[j].hi == corpus.starts[(size_t)u + 1] - 1,
           "a run's utterance", (long)i, u);
    expect(at < runs[j].length, "a run's length covers its entries", (long)i, runs[j].length);
    at++;
  }
  expect(j + 1 == runs.size(), "no run without entries", (long)j, (long)runs.size());
  for (const FrameRun &r : runs) total += r.length;
  expect(total == (long)f.size(), "the runs' lengths sum to the list's", total, (long)f.size());
  // the staged image
  std::vector<int32_t> image(kcnn::run_image_bytes(runs.size()) / sizeof(int32_t), -7);
  kcnn::stage_runs(runs, image.data());
  expect(image[0] == 0 && image[runs.size()] == (int32_t)f.size(), "the staged starts", image[0],
         image[runs.size()]);
  for (size_t r = 0; r < runs.size(); r++) {
    const int32_t *tri = image.data() + runs.size() + 1 + 3 * r;
    expect(image[r + 1] - image[r] == runs[r].length && tri[0] == runs[r].first &&
               tri[1] == runs[r].lo && tri[2] == runs[r].hi, "a staged run", (long)r);
  }
  *out = runs;
}

// Checks 2 and 3 for one plan and one list.
void check_pass(const char *name, const TimePlan &plan, const CorpusIndex &corpus,
                const std::vector<int32_t> &f, int left) {
  std::vector<FrameRun> runs;
  check_runs(corpus, f, &runs);
  std::vector<int32_t> lengths;
  for (const FrameRun &r : runs) lengths.push_back(r.length);
  TimeRows rows;
  const std::string bad = kcnn::plan_train_rows(plan, lengths.data(), (int)lengths.size(), &rows);
  if (!bad.empty()) {
    printf("REFUSED: %s: %s\n", name, bad.c_str());
    failures++;
    return;
  }
  const int p = plan.prefix();
  const int context = plan.levels[0].positions - 1;
  expect(rows.result_rows == (int64_t)f.size(), "result rows", (long)rows.result_rows);
  // 2. the level-0 map as kn_timemap_layout fills it, and every example's window
  std::vector<int32_t> map0((size_t)rows.input_rows, -1);
  int64_t start = 0;  // the sum of the earlier runs' lengths
  for (size_t j = 0; j < runs.size(); start += runs[j].length, j++) {
    expect(rows.base[j] == start + (int64_t)j * context && rows.frames[j] == runs[j].length,
           "base_j = start_j + j (L + R)", (long)j);
    for (int64_t i = 0; i < runs[j].length + context; i++) {
      int64_t src = (int64_t)runs[j].first - left + i;
      src = std::max<int64_t>(runs[j].lo, std::min<int64_t>(src, runs[j].hi));
      expect(rows.base[j] + i < rows.input_rows, "a level-0 row inside the map", (long)j, (long)i);
      map0[(size_t)(rows.base[j] + i)] = (int32_t)src;
    }
  }
  for (int32_t v : map0) expect(v >= 0, "every level-0 row is written");
  {
    size_t n = 0;
    for (size_t j = 0; j < runs.size(); j++)
      for (int t = 0; t < runs[j].length; t++, n++) {
        const int u = (int)(std::upper_bound(corpus.starts.begin(), corpus.starts.end() - 1, f[n]) -
                            corpus.starts.begin()) - 1;
        const int64_t s = corpus.starts[(size_t)u], e = corpus.starts[(size_t)u + 1];
        for (int k = 0; k <= context; k++) {
          const int64_t want = std::max<int64_t>(s, std::min<int64_t>((int64_t)f[n] - left + k, e - 1));
          expect(map0[(size_t)(rows.base[j] + t + k)] == want, "example n's clamped context",
                 (long)n, k);
        }
      }
  }
  // 3. the forward: reads and writes inside the rows of its maps
  std::vector<int64_t> have((size_t)p, -1);  // rows a level's map holds
  have[0] = rows.input_rows;
  const std::vector<TimeLaunch> fwd = kcnn::time_schedule(plan, rows, kcnn::kUtteranceRoute);
  for (const TimeLaunch &t : fwd) {
    expect(have[(size_t)t.in_level] >= t.in_rows, "a forward launch reads rows that exist",
           t.in_level, t.in_rows);
    if (t.op == TimeLaunch::kGather) {
      const int64_t span = (int64_t)t.dilation * (t.positions - 1);
      expect(rows.base.back() + rows.frames.back() - 1 + span <= t.in_rows - 1,
             "the gather's last window inside the top map");
      continue;
    }
    expect(t.op == TimeLaunch::kConvTaps || t.op == TimeLaunch::kEpilogue,
           "a training plan has 1-D launches only", (long)t.op);
    expect((int64_t)t.rows - 1 + (int64_t)t.dilation * (t.taps - 1) <= (int64_t)t.in_rows - 1,
           "a forward launch's highest tap", t.rows, t.in_rows);
    for (int l : {t.out_level, t.act_level})
      if (l >= 0) have[(size_t)l] = t.rows;
  }
  // the backward
  const std::vector<TimeBackLaunch> bwd = kcnn::time_backward_schedule(plan, rows);
  expect(bwd.size() == fwd.size(), "one backward launch per forward launch", (long)bwd.size());
  std::vector<int64_t> dhave((size_t)p, -1);  // rows a derivative map holds
  for (size_t i = 0; i < bwd.size(); i++) {
    const TimeBackLaunch &b = bwd[i];
    if (i == 0) {
      expect(b.op == TimeBackLaunch::kScatter && b.din_level == p - 1, "the scatter is first");
      expect(b.rows == (int)f.size() && b.in_rows == rows.computed[(size_t)p - 1],
             "the scatter writes the top level's computed rows", b.rows, b.in_rows);
      expect(b.positions == plan.levels[(size_t)p - 1].positions &&
                 b.dilation == plan.levels[(size_t)p - 1].dilation && b.context == context,
             "the scatter's geometry");
      dhave[(size_t)b.din_level] = b.in_rows;
      continue;
    }
    expect(b.op != TimeBackLaunch::kScatter, "one scatter");
    expect(b.dout_level >= 1 && dhave[(size_t)b.dout_level] == b.rows,
           "a backward launch reads a derivative map written before it, whole", b.dout_level,
           b.rows);
    expect((int64_t)b.in_rows == (int64_t)b.rows + (int64_t)b.dilation * (b.taps - 1),
           "din's rows are those the forward read", b.in_rows, b.rows);
    expect(b.in_level >= 0 && have[(size_t)b.in_level] >= b.in_rows,
           "the forward map below holds in_rows rows", b.in_level, b.in_rows);
    if (b.op == TimeBackLaunch::kEpilogueBwd) {
      expect(b.pooled_level >= 0 || b.act_level >= 0, "a pool and/or a ReLU");
      for (int l : {b.pooled_level, b.act_level})
        if (l >= 0) expect(have[(size_t)l] >= b.rows, "the epilogue's forward maps hold `rows`", l);
      expect(b.din_level == b.in_level && b.din_level >= 1, "an epilogue's din is its input's");
      if (b.pooled_level < 0) expect(b.taps == 1 && b.pool_channel == 1, "a lone ReLU");
    } else {
      expect(plan.levels[(size_t)b.comp].kind == TimeComp::kConv, "a convolution's component");
      expect((b.in_level == 0) == (b.din_level < 0),
             "no data gradient exactly for the convolution on level 0", b.in_level, b.din_level);
      // gradient rows c wc + d wd cover [0, C taps) once
      const int C = plan.levels[(size_t)b.in_level].width;
      std::vector<int> seen((size_t)C * b.taps, 0);
      for (int c = 0; c < C; c++)
        for (int d = 0; d < b.taps; d++) {
          const int64_t r = (int64_t)c * b.wc + (int64_t)d * b.wd;
          expect(r >= 0 && r < (int64_t)seen.size(), "a gradient row inside the gradient", c, d);
          if (r >= 0 && r < (int64_t)seen.size()) seen[(size_t)r]++;
        }
      for (int v : seen) expect(v == 1, "every gradient row written once");
    }
    if (b.din_level >= 0) {
      expect(dhave[(size_t)b.din_level] < 0, "a derivative map has one writer", b.din_level);
      expect(b.in_rows == rows.computed[(size_t)b.din_level], "din: the level's computed rows");
      dhave[(size_t)b.din_level] = b.in_rows;
    }
  }
  // windows stay inside: rows no window reads are not the last written ones
  printf("%s: %zu frames in %zu runs: %ld level-0 rows, %zu forward and %zu backward launches\n",
         name, f.size(), runs.size(), (long)rows.input_rows, fwd.size(), bwd.size());
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 3) {
    printf("usage: %s nnet.config freq_conv.config\n", argv[0]);
    return 2;
  }
  CorpusIndex corpus;
  const int32_t utt_lengths[3] = {7, 23, 40};
  expect(kcnn::build_corpus_index(utt_lengths, 3, 70, 8, &corpus).empty(), "the corpus index");

  // 4. the training plans
  const TimePlan s = kcnn::time_train_plan(kcnn::make_time_plan(parse_config(shrunken(false)), false, true));
  const TimePlan pc4 = kcnn::time_train_plan(kcnn::make_time_plan(parse_config(shrunken(true)), false, true));
  const TimePlan nnet = kcnn::time_train_plan(kcnn::make_time_plan(parse_config(read_file(argv[1])), false, true));
  const TimePlan with_height = kcnn::make_time_plan(parse_config(read_file(argv[2])), false, true);
  const TimePlan freq = kcnn::time_train_plan(with_height);
  expect(s.prefix() == 8 && pc4.prefix() == 8, "the shrunken nets train with prefix 8", s.prefix());
  expect(nnet.prefix() == 14, "nnet.config trains with prefix 14", nnet.prefix());
  expect(with_height.prefix() > 0 && freq.prefix() == 0 && !freq.declined.empty(),
         "a plan with a height level gives training prefix 0", with_height.prefix(), freq.prefix());
  expect(kcnn::time_train_plan(kcnn::make_time_plan(parse_config(shrunken(false)), true, true)).prefix() == 0,
         "the literal path gives training prefix 0");
  expect(kcnn::time_backward_schedule(freq, TimeRows()).empty(), "no plan, no backward launches");
  printf("training prefixes: shrunken %d, shrunken pc 4 %d, nnet.config %d, freq_conv.config %d\n",
         s.prefix(), pc4.prefix(), nnet.prefix(), freq.prefix());

  // 1 - 3 on the hand-written list and on random ones
  const std::vector<int32_t> hand = hand_list();
  {
    std::vector<FrameRun> runs;
    check_runs(corpus, hand, &runs);
    const int want[][2] = {{0, 7}, {7, 5}, {41, 1}, {25, 5}, {30, 6}, {50, 8}, {50, 8},
                           {20, 1}, {19, 1}, {18, 1}, {62, 8}};
    expect(runs.size() == 11, "the hand-written list has 11 runs", (long)runs.size());
    for (size_t j = 0; j < runs.size() && j < 11; j++)
      expect(runs[j].first == want[j][0] && runs[j].length == want[j][1], "a run of the list",
             (long)j, runs[j].first);
  }
  check_pass("shrunken", s, corpus, hand, 5);
  check_pass("shrunken pc 4", pc4, corpus, hand, 5);
  {
    // nnet.config reads 40 columns; the index is of rows alone
    check_pass("nnet.config", nnet, corpus, hand, (nnet.levels[0].positions - 1) / 2);
  }
  std::mt19937 gen(20);
  for (int trial = 0; trial < 200; trial++) {
    std::vector<int32_t> f;
    const int pieces = 1 + (int)(gen() % 12);
    for (int q = 0; q < pieces; q++) {
      const int a = (int)(gen() % 70), n = 1 + (int)(gen() % 12);
      const bool down = gen() % 5 == 0;
      for (int i = 0; i < n; i++) f.push_back(std::max(0, std::min(69, down ? a - i : a + i)));
    }
    char name[64];
    snprintf(name, sizeof name, "random list %d", trial);
    check_pass(name, trial % 2 ? pc4 : s, corpus, f, 5);
  }

  // 5. oversize passes, by arithmetic alone
  {
    TimeRows rows;
    const int32_t big[2] = {1 << 30, 1 << 30};
    expect(!kcnn::plan_train_rows(s, big, 2, &rows).empty(), "2^31 rows are refused");
    const int32_t wide[1] = {(1 << 26)};  // 2^26 rows x 32 columns = 2^31 elements of a map
    expect(!kcnn::plan_train_rows(s, wide, 1, &rows).empty(), "2^31 elements of a map are refused");
    const int32_t fits[1] = {(1 << 23)};
    expect(kcnn::plan_train_rows(s, fits, 1, &rows).empty(), "2^23 rows fit");
    const int32_t none[1] = {0};
    expect(!kcnn::plan_train_rows(s, none, 1, &rows).empty(), "an empty run is refused");
    expect(!kcnn::plan_train_rows(s, fits, 0, &rows).empty(), "no runs are refused");
    expect(!kcnn::plan_train_rows(freq, fits, 1, &rows).empty(), "no plan is refused");
  }

  if (failures) {
    printf("%d of %ld checks FAILED\n", failures, checks);
    return 1;
  }
  printf("all time backward checks passed (%ld)\n", checks);
  return 0;
}
