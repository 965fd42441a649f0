// scripts/stream_segments_check.cc -- the host plan of a time-shared streaming
// step (StreamState::Segments, kaldi-cnn_amd/src/capi/stream-state.h, with the
// row plan of capi/time-plan.h) as a stand-alone host program, for a run under
// a host sanitizer.  No GPU call.
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ikaldi-cnn_amd/src scripts/stream_segments_check.cc -o stream_segments_check
//   ./stream_segments_check
//
// Random schedules (every L, R in 0..3, max_chunk in 1..4, three slots reused
// as their utterances of 0..9 frames end, by `final` with the last frames or
// by a `final` of none, a Reset now and then) against a brute-force model whose
// "frames" are integers (utterance id x 1000 + frame number).  Per step the
// segments are taken BEFORE Plan, then Plan's descriptors are executed as
// kn_stream_assemble would and the segments as kn_stream_segments would, every
// index checked: map row j of a slot's segment must be the slot's frame
// clamp(e0 - L + j, 0, newest); the segments must be packed, in the step's
// order, k_i + L + R long with k_i = Plan's num_out; Segments must move no
// slot; the row plan must accept them as an unpadded input and its windows
// must be the windows of Plan's triples; and no step may pass max_map_rows(),
// which a step built for it must reach.  Then what the plan refuses.
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "capi/stream-state.h"
#include "capi/time-plan.h"

namespace {

int failures = 0;
long steps_run = 0, segments_seen = 0, rows_checked = 0, most_rows = 0;

void fail(const char *what, long a = 0, long b = 0) {
  if (failures < 20) printf("WRONG: %s (%ld, %ld)\n", what, a, b);
  failures++;
}

// the plan of Splice(-L .. R) -> Convolution over the whole window: context L + R
kcnn::TimePlan plan_for(int L, int R) {
  std::vector<kcnn::TimeComp> comps(2);
  comps[0].kind = kcnn::TimeComp::kSplice;
  comps[0].input_dim = 3;
  comps[0].left = L;
  comps[0].right = R;
  kcnn::TimeComp &c = comps[1];
  c.kind = kcnn::TimeComp::kConv;
  c.in_height = c.kernel_height = 3;
  c.in_width = L + R + 1;
  c.in_channel = 1;
  c.kernel_width = 1;
  c.group = 2;
  c.out_height = 1;
  c.out_width = L + R + 1;
  return kcnn::make_time_plan(comps, false);
}

struct Utt {
  bool busy = false;
  int id = 0, length = 0, fed = 0, got = 0;
};

struct Model {
  int L, R, mc, ns;
  kcnn::StreamState st;
  kcnn::TimePlan plan;
  std::vector<int> arena;
  std::vector<Utt> utt;
  Model(int l, int r, int m, int n)
      : L(l), R(r), mc(m), ns(n), st(l, r, m, n), plan(plan_for(l, r)),
        arena((size_t)st.arena_rows(), -7), utt((size_t)n) {}

  // One step: slot who[i] gets n[i] frames, final fin[i].
  void Step(const std::vector<int32_t> &who, const std::vector<int32_t> &n,
            const std::vector<int32_t> &fin) {
    std::vector<int> chunk;
    for (size_t i = 0; i < who.size(); i++)
      for (int k = 0; k < n[i]; k++) chunk.push_back(utt[who[i]].id * 1000 + utt[who[i]].fed + k);
    const kcnn::StreamStep step = {who.data(), n.data(), fin.data(), (int)who.size(),
                                   (int64_t)chunk.size()};
    kcnn::StepTotals tot;
    const std::string err = st.Check(step, &tot);
    if (!err.empty()) {
      printf("REFUSED a valid step: %s\n", err.c_str());
      failures++;
      return;
    }
    std::vector<int64_t> before((size_t)2 * ns), now(2);
    for (int s = 0; s < ns; s++) st.Frames(s, &before[2 * s]);
    kcnn::StepSegments segs;
    segs.desc.assign(3, 99);  // stale contents must go
    st.Segments(step, &segs);
    for (int s = 0; s < ns; s++) {
      st.Frames(s, now.data());
      if (now[0] != before[2 * s] || now[1] != before[2 * s + 1]) fail("Segments moved a slot", s);
    }
    const kcnn::StepLayout lay = kcnn::step_layout(step.num, tot);
    int32_t *img = static_cast<int32_t *>(malloc(lay.bytes ? lay.bytes : 1));  // exact size
    int32_t *num_out = static_cast<int32_t *>(malloc(sizeof(int32_t) * (who.size() + 1)));
    st.Plan(step, tot, img, num_out);
    steps_run++;
    const int rows = st.arena_rows();
    const int32_t *desc = img + lay.desc;
    for (int i = 0; i < step.num; i++) {  // the assembly
      const int32_t *d = desc + kcnn::kStreamDescInts * i;
      std::vector<int> tail;
      for (int k = 0; k < d[1]; k++) tail.push_back(arena[d[0] + k]);
      for (int k = 0; k < d[1] + d[4]; k++)
        arena[d[2] + k] = k < d[1] ? tail[k] : chunk[d[3] + k - d[1]];
    }
    // the segments against the model
    if ((int)segs.desc.size() != kcnn::kStreamSegmentInts * segs.num ||
        (int)segs.lengths.size() != segs.num || (int)segs.out_start.size() != segs.num + 1 ||
        segs.out_start[0] != 0)
      fail("segment arrays");
    if (segs.out_rows != tot.out_rows) fail("out_rows", segs.out_rows, tot.out_rows);
    if (segs.map_rows > st.max_map_rows()) fail("more rows than the worst case", segs.map_rows);
    most_rows = std::max<long>(most_rows, segs.map_rows);
    std::vector<int> map((size_t)segs.map_rows, -9);
    int u = 0, at = 0;
    for (int i = 0; i < step.num; i++) {
      Utt &r = utt[who[i]];
      r.fed += n[i];
      const int k = num_out[i];
      if (k > 0) {
        if (u >= segs.num) { fail("a segment is missing", i); break; }
        const int32_t *d = &segs.desc[(size_t)kcnn::kStreamSegmentInts * u];
        if (d[3] != at || d[4] != k + L + R || segs.lengths[u] != d[4] ||
            segs.out_start[u + 1] - segs.out_start[u] != k)
          fail("segment shape", i, d[4]);
        if (d[1] < 0 || d[2] >= rows || d[1] > d[2]) fail("clamp bounds out of the arena", d[1], d[2]);
        for (int j = 0; j < d[4]; j++, rows_checked++) {
          const int src = std::max(d[1], std::min(d[0] + j, d[2]));
          if (src < 0 || src >= rows) { fail("source row out of the arena", src); continue; }
          const int expect = r.id * 1000 + std::max(0, std::min(r.got - L + j, r.fed - 1));
          if (arena[src] != expect) fail("segment row", arena[src], expect);
          if (d[3] + j < 0 || d[3] + j >= segs.map_rows) { fail("map row", d[3] + j); continue; }
          map[d[3] + j] = arena[src];
        }
        at += d[4];
        u++;
        segments_seen++;
      }
      r.got += k;
      if (fin[i]) {
        if (r.got != r.length || r.fed != r.length) fail("an utterance ended short", r.got);
        r.busy = false;
      }
    }
    if (u != segs.num || at != segs.map_rows) fail("segments not packed", at, segs.map_rows);
    // the row plan takes them as an unpadded input; its windows are the triples'
    if (segs.num > 0) {
      kcnn::TimeRows tr;
      const std::string no =
          kcnn::plan_time_rows(plan, segs.lengths.data(), segs.num, false, &tr);
      if (!no.empty()) {
        printf("the row plan REFUSED a step: %s\n", no.c_str());
        failures++;
      } else {
        if (tr.input_rows != segs.map_rows || tr.result_rows != segs.out_rows) fail("plan rows");
        const int32_t *tri = img + lay.triples;
        for (int v = 0; v < segs.num; v++)
          for (int r = segs.out_start[v]; r < segs.out_start[v + 1]; r++, tri += 3)
            for (int o = 0; o <= L + R; o++) {
              const int row = std::max(tri[1], std::min(tri[0] - L + o, tri[2]));
              const int64_t m = r + (int64_t)v * (L + R) + o;  // the gather's source
              if (m < 0 || m >= segs.map_rows) { fail("window row", m); continue; }
              if (map[m] != arena[row]) fail("window", map[m], arena[row]);
            }
      }
    } else if (tot.out_rows != 0) {
      fail("no segment for a step that emits");
    }
    free(img);
    free(num_out);
  }
};

void walk(int L, int R, int mc, std::mt19937 *rng) {
  const int ns = 3;
  Model m(L, R, mc, ns);
  int next_id = 1;
  for (int step = 0; step < 400; step++) {
    std::vector<int> order = {0, 1, 2};
    std::shuffle(order.begin(), order.end(), *rng);
    order.resize(1 + (*rng)() % ns);
    std::vector<int32_t> who, n, fin;
    for (int s : order) {
      Utt &r = m.utt[s];
      if (r.busy && (*rng)() % 23 == 0) {  // abandoned: the slot starts afresh
        m.st.Reset(s);
        r.busy = false;
      }
      if (!r.busy) {
        r = Utt();
        r.busy = true;
        r.id = next_id++ % 2000 + 1;
        r.length = (int)((*rng)() % 10);
      }
      const int left = r.length - r.fed;
      int k = left == 0 ? 0 : 1 + (int)((*rng)() % std::min(left, mc));
      if (left > 0 && (*rng)() % 5 == 0) k = std::min(left, mc);
      // the last frames carry `final`, or a later step of none does
      const bool last = k == left && (left == 0 || (*rng)() % 2 == 0);
      if (k == 0 && !last) continue;
      who.push_back(s);
      n.push_back(k);
      fin.push_back(last ? 1 : 0);
    }
    if (!who.empty()) m.Step(who, n, fin);
  }
}

// The step max_map_rows() is for: every slot holds R frames not yet emitted,
// then gets max_chunk frames and ends.
void worst_case(int L, int R, int mc, int ns) {
  Model m(L, R, mc, ns);
  const int T = (R + mc - 1) / mc * mc + mc;  // whole chunks, the last one final
  std::vector<int32_t> who, n, fin;
  for (int s = 0; s < ns; s++) {
    m.utt[s].busy = true;
    m.utt[s].id = s + 1;
    m.utt[s].length = T;
    who.push_back(s);
    n.push_back(mc);
    fin.push_back(0);
  }
  most_rows = 0;
  for (int fed = 0; fed < T; fed += mc) {
    if (fed + mc == T) fin.assign((size_t)ns, 1);
    m.Step(who, n, fin);
  }
  if (most_rows != m.st.max_map_rows()) fail("the worst case is not reached", most_rows,
                                             (long)m.st.max_map_rows());
  if (m.st.max_map_rows() != (int64_t)ns * (mc + L + 2 * R)) fail("max_map_rows");
}

void refusals() {
  // a plan of another context than the state's: segments one row short
  kcnn::StreamState st(2, 1, 4, 2);
  const int32_t who[] = {1}, n[] = {3}, fin[] = {0};
  const kcnn::StreamStep step = {who, n, fin, 1, 3};
  kcnn::StepTotals tot;
  if (!st.Check(step, &tot).empty()) fail("a valid step");
  kcnn::StepSegments segs;
  st.Segments(step, &segs);
  if (segs.num != 1 || segs.lengths[0] != 2 + 3 || segs.out_rows != 2) fail("one segment");
  kcnn::TimeRows tr;
  auto refused = [&](const kcnn::TimePlan &p, const int32_t *len, int num, const char *word) {
    const std::string err = kcnn::plan_time_rows(p, len, num, false, &tr);
    const bool ok = err.find(word) != std::string::npos;
    printf("%-28s %s  (%s)\n", word, ok ? "refused" : "WRONG", err.c_str());
    if (!ok) failures++;
  };
  if (!kcnn::plan_time_rows(plan_for(2, 1), segs.lengths.data(), 1, false, &tr).empty())
    fail("the state's own plan");
  const int32_t shorter[] = {5};
  refused(plan_for(3, 2), shorter, 1, "at least 6 are needed");
  refused(plan_for(2, 1), segs.lengths.data(), 0, "no utterances");
  refused(kcnn::TimePlan(), segs.lengths.data(), 1, "no plan");
  // a step that emits nothing has no segment
  kcnn::StreamState quiet(2, 3, 4, 2);
  const int32_t two[] = {2};
  const kcnn::StreamStep small = {who, two, fin, 1, 2};
  if (!quiet.Check(small, &tot).empty() || tot.out_rows != 0) fail("a step that emits nothing");
  quiet.Segments(small, &segs);
  if (segs.num != 0 || segs.map_rows != 0 || segs.out_rows != 0 || !segs.desc.empty() ||
      segs.out_start.size() != 1)
    fail("segments of a step that emits nothing");
}

}  // namespace

int main() {
  std::mt19937 rng(20261021);
  for (int L = 0; L <= 3; L++)
    for (int R = 0; R <= 3; R++)
      for (int mc = 1; mc <= 4; mc++) walk(L, R, mc, &rng);
  printf("%ld steps, %ld segments, %ld map rows checked\n", steps_run, segments_seen,
         rows_checked);
  for (int L = 0; L <= 3; L++)
    for (int R = 0; R <= 3; R++)
      for (int mc = 1; mc <= 4; mc++) worst_case(L, R, mc, 3);
  refusals();
  printf(failures ? "FAILED: %d\n" : "all stream segment checks passed\n", failures);
  return failures ? 1 : 0;
}
