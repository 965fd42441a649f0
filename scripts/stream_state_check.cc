// scripts/stream_state_check.cc -- the host bookkeeping of kcnn::OnlineComputer
// (kaldi-cnn_amd/src/capi/stream-state.h) as a stand-alone host program, for a
// run under a host sanitizer.  No GPU call.
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ikaldi-cnn_amd/src scripts/stream_state_check.cc -o stream_state_check
//   ./stream_state_check
//
// Drives StreamState against a host model of the arena whose "frames" are
// integers (utterance id x 1000 + frame number), for every L, R in 0..3,
// max_chunk in 1..4 and utterance length 0..9: EVERY chunking of the length
// into chunks of 1..max_chunk frames, ended both by `final` with the last
// frames and by a `final` of no frames.  Three slots run the utterances
// interleaved (a seeded draw picks the slots and the order of each step) and
// are reused as they end.  The model executes each step's descriptors as
// kn_stream_assemble would, with every arena and chunk index checked, poisons
// the buffers the slots left, and reads every emitted triple as
// kn_splice_frames_prop would: each window must be the clamped window of the
// whole utterance, each frame emitted once and in order, slots not named
// untouched.  Refused steps are then shown to change nothing.
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "capi/stream-state.h"

namespace {

int failures = 0;
long steps_run = 0, frames_emitted = 0, scripts_run = 0;

void fail(const char *what, long a = 0, long b = 0) {
  if (failures < 20) printf("WRONG: %s (%ld, %ld)\n", what, a, b);
  failures++;
}

// One utterance fed in chunks: chunks[k] frames in step k; flush: a last step
// of no frames carries `final`, else the last chunk does.
struct Script {
  int length;
  std::vector<int> chunks;
  bool flush;
};

void compositions(int left, int max_chunk, std::vector<int> *cur, std::vector<Script> *out,
                  int length) {
  if (left == 0) {
    if (!cur->empty()) out->push_back({length, *cur, false});
    out->push_back({length, *cur, true});
    return;
  }
  for (int n = 1; n <= std::min(left, max_chunk); n++) {
    cur->push_back(n);
    compositions(left - n, max_chunk, cur, out, length);
    cur->pop_back();
  }
}

struct Running {
  bool busy = false;
  Script s;
  size_t next = 0;   // the next chunk
  int id = 0;        // utterance id
  int fed = 0, got = 0;
};

constexpr int kPoison = -7;

struct Model {
  int L, R, mc, ns;
  kcnn::StreamState st;
  std::vector<int> arena;
  Model(int l, int r, int m, int n)
      : L(l), R(r), mc(m), ns(n), st(l, r, m, n), arena((size_t)st.arena_rows(), kPoison) {}

  // Runs one step naming `who` (slot indices); returns false on a refusal.
  bool Step(const std::vector<int> &who, std::vector<Running> *run) {
    std::vector<int32_t> streams, num_new, final;
    std::vector<int> chunk;
    for (int s : who) {
      Running &r = (*run)[s];
      int n = r.next < r.s.chunks.size() ? r.s.chunks[r.next] : 0;
      const bool last = r.s.flush ? r.next == r.s.chunks.size() : r.next + 1 == r.s.chunks.size();
      streams.push_back(s);
      num_new.push_back(n);
      final.push_back(last ? 1 : 0);
      for (int k = 0; k < n; k++) chunk.push_back(r.id * 1000 + r.fed + k);
    }
    std::vector<int64_t> before((size_t)2 * ns);
    for (int s = 0; s < ns; s++) st.Frames(s, &before[2 * s]);
    const kcnn::StreamStep step = {streams.data(), num_new.data(), final.data(), (int)who.size(),
                                   (int64_t)chunk.size()};
    kcnn::StepTotals tot;
    const std::string err = st.Check(step, &tot);
    if (!err.empty()) {
      printf("REFUSED a valid step: %s\n", err.c_str());
      failures++;
      return false;
    }
    const kcnn::StepLayout lay = kcnn::step_layout(step.num, tot);
    int32_t *img = static_cast<int32_t *>(malloc(lay.bytes ? lay.bytes : 1));  // exact size
    int32_t *num_out = static_cast<int32_t *>(malloc(sizeof(int32_t) * (who.size() + 1)));
    st.Plan(step, tot, img, num_out);
    steps_run++;
    // the assembly, as the kernel runs it: every source is read before any
    // row is written, which the kernel's lanes do not promise -- so a
    // destination that is also some slot's source is an error
    const int32_t *row_start = img + lay.row_start, *desc = img + lay.desc;
    const int rows = st.arena_rows(), cap = st.cap();
    if (row_start[0] != 0 || row_start[step.num] != tot.copy_rows) fail("prefix ends");
    std::vector<char> is_src((size_t)rows, 0);
    for (int i = 0; i < step.num; i++) {
      const int32_t *d = desc + kcnn::kStreamDescInts * i;
      if (row_start[i + 1] - row_start[i] != d[1] + d[4]) fail("prefix", i);
      for (int k = 0; k < d[1]; k++) {
        if (d[0] + k < 0 || d[0] + k >= rows) { fail("tail row out of the arena", d[0] + k); continue; }
        is_src[d[0] + k] = 1;
      }
    }
    for (int i = 0; i < step.num; i++) {
      const int32_t *d = desc + kcnn::kStreamDescInts * i;
      const int s = streams[i];
      if (d[1] < 0 || d[1] > L + R || d[4] != num_new[i] || d[1] + d[4] > cap) fail("descriptor", i);
      // the destination: one whole buffer of this slot's
      if (d[2] != 2 * s * cap && d[2] != (2 * s + 1) * cap) fail("destination", d[2]);
      for (int k = 0; k < d[1] + d[4]; k++) {
        const int dst = d[2] + k;
        if (dst < 0 || dst >= rows) { fail("write out of the arena", dst); continue; }
        if (is_src[dst]) fail("a row is read and written in one step", dst);
        if (k < d[1]) {
          const int src = d[0] + k;
          if (src < 0 || src >= rows || src / cap / 2 != s) { fail("tail source", src); continue; }
          arena[dst] = arena[src];
        } else {
          const int c = d[3] + k - d[1];
          if (c < 0 || c >= (int)chunk.size()) { fail("chunk row out of range", c); continue; }
          arena[dst] = chunk[c];
        }
      }
      // what the slot left must never be read again
      const int old = d[2] == 2 * s * cap ? (2 * s + 1) * cap : 2 * s * cap;
      for (int k = 0; k < cap; k++) arena[old + k] = kPoison;
    }
    // the emitted frames
    const int32_t *tri = img + lay.triples;
    int out = 0;
    for (int i = 0; i < step.num; i++) {
      Running &r = (*run)[streams[i]];
      r.fed += num_new[i];
      const int T = r.s.length;
      const int want = final[i] ? r.fed - r.got : std::max(0, r.fed - R) - r.got;
      if (num_out[i] != want) fail("num_out", num_out[i], want);
      for (int k = 0; k < num_out[i]; k++, tri += 3, out++) {
        const int t = r.got + k;
        for (int o = -L; o <= R; o++) {
          const int row = std::max(tri[1], std::min(tri[0] + o, tri[2]));
          if (row < 0 || row >= rows) { fail("window row out of the arena", row); continue; }
          const int expect = r.id * 1000 + std::max(0, std::min(t + o, T - 1));
          if (arena[row] != expect) fail("window", arena[row], expect);
        }
        frames_emitted++;
      }
      r.got += num_out[i];
      if (final[i] && (r.got != T || r.fed != T)) fail("an utterance ended short", r.got, T);
      r.next++;
    }
    if (out != tot.out_rows) fail("out_rows", out, tot.out_rows);
    // Frames: the named slots advanced (a final one is free), the others untouched
    for (int s = 0; s < ns; s++) {
      int64_t now[2];
      st.Frames(s, now);
      int at = -1;
      for (int i = 0; i < step.num; i++)
        if (streams[i] == s) at = i;
      if (at < 0) {
        if (now[0] != before[2 * s] || now[1] != before[2 * s + 1]) fail("an unnamed slot moved", s);
      } else if (final[at]) {
        if (now[0] != 0 || now[1] != 0) fail("a final slot is not free", s);
      } else if (now[0] != (*run)[s].fed || now[1] != (*run)[s].got) {
        fail("Frames", s);
      }
    }
    free(img);
    free(num_out);
    return true;
  }
};

void walk(int L, int R, int mc, std::mt19937 *rng) {
  std::vector<Script> scripts;
  for (int T = 0; T <= 9; T++) {
    std::vector<int> cur;
    compositions(T, mc, &cur, &scripts, T);
  }
  std::shuffle(scripts.begin(), scripts.end(), *rng);
  const int ns = 3;
  Model m(L, R, mc, ns);
  std::vector<Running> run((size_t)ns);
  size_t next_script = 0;
  int next_id = 1;
  for (;;) {
    for (Running &r : run)
      if (!r.busy && next_script < scripts.size()) {
        r = Running();
        r.busy = true;
        r.s = scripts[next_script++];
        r.id = next_id++ % 2000 + 1;
        scripts_run++;
      }
    std::vector<int> busy;
    for (int s = 0; s < ns; s++)
      if (run[s].busy) busy.push_back(s);
    if (busy.empty()) break;
    // a non-empty subset of the busy slots, in a drawn order
    std::shuffle(busy.begin(), busy.end(), *rng);
    busy.resize(1 + (*rng)() % busy.size());
    if (!m.Step(busy, &run)) return;
    for (int s : busy) {
      const Running &r = run[s];
      if (r.next >= r.s.chunks.size() + (r.s.flush ? 1 : 0)) run[s].busy = false;
    }
  }
}

// Every refusal, after some accepted steps: the message, and no slot moved.
void refusals() {
  kcnn::StreamState st(2, 2, 4, 3);
  auto frames = [&] {
    std::vector<int64_t> f(6);
    for (int s = 0; s < 3; s++) st.Frames(s, &f[2 * s]);
    return f;
  };
  auto run = [&](std::vector<int32_t> streams, std::vector<int32_t> n, std::vector<int32_t> fin,
                 int64_t chunk_rows, const char *word) {
    const kcnn::StreamStep step = {streams.data(), n.data(), fin.data(), (int)streams.size(),
                                   chunk_rows};
    kcnn::StepTotals tot;
    const std::vector<int64_t> before = frames();
    const std::string err = st.Check(step, &tot);
    const bool ok = word ? err.find(word) != std::string::npos : err.empty();
    printf("%-28s %s  (%s)\n", word ? word : "a valid step", ok ? (word ? "refused" : "accepted") : "WRONG",
           err.c_str());
    if (!ok) failures++;
    if (word && frames() != before) fail("a refused step moved a slot");
    if (!word) {
      const kcnn::StepLayout lay = kcnn::step_layout(step.num, tot);
      std::vector<int32_t> img(lay.bytes / 4 + 1), num_out(streams.size() + 1);
      st.Plan(step, tot, img.data(), num_out.data());
    }
  };
  run({0, 2}, {4, 3}, {0, 0}, 7, nullptr);
  run({2}, {1}, {0}, 1, nullptr);
  run({0, 3}, {1, 1}, {0, 0}, 2, "stream 3 outside");
  run({-1}, {1}, {0}, 1, "stream -1 outside");
  run({0, 1, 0}, {1, 1, 1}, {0, 0, 0}, 3, "named twice");
  run({0, 1, 2, 1}, {1, 1, 1, 1}, {0, 0, 0, 0}, 4, "4 slots named");
  run({1}, {5}, {0}, 5, "5 new frames outside");
  run({1}, {-1}, {1}, -1, "-1 new frames outside");
  run({1}, {0}, {0}, 0, "no new frames");
  run({0, 1}, {2, 2}, {0, 1}, 5, "sum to 4");
  run({0, 1}, {2, 2}, {0, 1}, 3, "sum to 4");
  {
    kcnn::StepTotals tot;
    const kcnn::StreamStep step = {nullptr, nullptr, nullptr, 2, 2};
    if (st.Check(step, &tot).find("bad stream arrays") == std::string::npos) fail("null arrays");
    const kcnn::StreamStep neg = {nullptr, nullptr, nullptr, -1, 0};
    if (st.Check(neg, &tot).find("bad stream arrays") == std::string::npos) fail("num < 0");
  }
  run({0}, {0}, {1}, 0, nullptr);  // a flush: slot 0 ends
  if (frames() != std::vector<int64_t>({0, 0, 0, 0, 4, 2})) fail("the slots after the steps");
  int64_t f[2];
  if (st.Reset(3) || st.Reset(-1) || st.Frames(3, f) || !st.Reset(2)) fail("Reset / Frames range");
  if (frames() != std::vector<int64_t>(6, 0)) fail("Reset");

  auto geom = [](int64_t l, int64_t r, int64_t mc, int64_t ns, int64_t cols, const char *word) {
    const std::string err = kcnn::check_stream_geometry(l, r, mc, ns, cols);
    const bool ok = word ? err.find(word) != std::string::npos : err.empty();
    printf("%-28s %s  (%s)\n", word ? word : "a valid geometry", ok ? "ok" : "WRONG", err.c_str());
    if (!ok) failures++;
  };
  geom(2, 2, 16, 32, 40, nullptr);
  geom(0, 0, 1, 1, 1, nullptr);
  geom(2, 2, 16, 0, 40, "num_streams 0");
  geom(2, 2, 0, 32, 40, "max_chunk 0");
  geom(-1, 2, 16, 32, 40, "context");
  geom(2, 2, 16, 1 << 20, 64, "2^31");
  geom(1000000, 1000000, 2147483647, 1, 4, "2^31");
  geom(2, 2, 16, 2147483647, 1, "2^31");
  geom(1000000, 1000000, 4, 1, 4, nullptr);
}

}  // namespace

int main() {
  std::mt19937 rng(20261020);
  for (int L = 0; L <= 3; L++)
    for (int R = 0; R <= 3; R++)
      for (int mc = 1; mc <= 4; mc++) walk(L, R, mc, &rng);
  printf("%ld utterances in %ld steps, %ld frames emitted\n", scripts_run, steps_run,
         frames_emitted);
  refusals();
  printf(failures ? "FAILED: %d\n" : "all stream state checks passed\n", failures);
  return failures ? 1 : 0;
}
