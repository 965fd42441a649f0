// scripts/frame_index_check.cc -- the corpus index and the frame-list checking
// and staging routine of kcnn_nnet_propagate_frames
// (kaldi-cnn_amd/src/capi/frame-index.h) as a stand-alone host program, for a
// run under a host sanitizer.  No GPU call.
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ikaldi-cnn_amd/src scripts/frame_index_check.cc -o frame_index_check
//   ./frame_index_check
//
// Runs every refusal (no utterances, a length below 1, lengths that do not
// sum to the rows, a corpus of 2^31 elements, no frames, an index below 0 or
// past the corpus, a window matrix of 2^31 rows, an activation of 2^31
// elements) and valid lists -- every row, the first and the last row of every
// utterance, repeats, one frame, utterances of one frame -- staging the valid
// ones into an exactly-sized heap buffer so that a write past either end is
// caught, and checking each triple against a linear search.
#include <stdio.h>
#include <stdlib.h>

#include "capi/frame-index.h"

namespace {

int failures = 0;

void expect(const char *what, const std::string &err, const char *word) {
  const bool ok = word ? err.find(word) != std::string::npos : err.empty();
  printf("%-34s %s  (%s)\n", what, ok ? (word ? "refused" : "accepted") : "WRONG", err.c_str());
  if (!ok) failures++;
}

void expect_bad_corpus(const char *what, const std::vector<int32_t> &lengths, int64_t rows,
                       int64_t cols, const char *word) {
  kcnn::CorpusIndex idx;
  idx.starts.assign(1, 77);  // must stay as it is
  const std::string err = kcnn::build_corpus_index(lengths.empty() ? nullptr : lengths.data(),
                                                   (int)lengths.size(), rows, cols, &idx);
  expect(what, err, word);
  if (idx.starts.size() != 1 || idx.starts[0] != 77) {
    printf("%-34s THE INDEX CHANGED\n", what);
    failures++;
  }
}

void expect_staged(const char *what, const kcnn::CorpusIndex &idx,
                   const std::vector<int32_t> &lengths, const std::vector<int32_t> &frames,
                   int chunk_rows) {
  const int num = (int)frames.size();
  const std::string err = kcnn::check_frames(idx, frames.data(), num, chunk_rows);
  if (!err.empty()) {
    printf("%-34s REFUSED (%s)\n", what, err.c_str());
    failures++;
    return;
  }
  const size_t bytes = kcnn::frame_triples_bytes(num);
  int32_t *buf = static_cast<int32_t *>(malloc(bytes));  // exact size
  kcnn::stage_frames(idx, frames.data(), num, buf);
  bool ok = true;
  for (int i = 0; i < num && ok; i++) {
    int32_t s = 0;
    size_t u = 0;
    while (frames[i] >= s + lengths[u]) s += lengths[u++];  // linear search
    ok = buf[3 * i] == frames[i] && buf[3 * i + 1] == s && buf[3 * i + 2] == s + lengths[u] - 1;
  }
  printf("%-34s %s  (%d frames, %zu bytes staged)\n", what, ok ? "staged" : "WRONG IMAGE", num,
         bytes);
  if (!ok) failures++;
  free(buf);
}

}  // namespace

int main() {
  const std::vector<int32_t> lengths = {1, 7, 23, 2, 1, 1, 40};
  int32_t rows = 0;
  for (int32_t t : lengths) rows += t;

  expect_bad_corpus("no utterances", {}, rows, 40, "no utterances");
  expect_bad_corpus("a length of 0", {1, 0, 74}, rows, 40, "utterance 1 has 0");
  expect_bad_corpus("a negative length", {76, -1}, rows, 40, "utterance 1 has -1");
  expect_bad_corpus("lengths short of the rows", {1, 7, 23}, rows, 40, "sum to 31");
  expect_bad_corpus("lengths past the rows", {1, 7, 23, 2, 1, 1, 41}, rows, 40, "sum to 76");
  expect_bad_corpus("lengths far past the rows", {2147483647, 2147483647, 2147483647}, rows, 40,
                    "sum to 6442450941");
  expect_bad_corpus("more utterances than rows", {1, 1, 1}, 2, 40, "3 utterances");
  expect_bad_corpus("no rows", {1}, 0, 40, "empty");
  expect_bad_corpus("no columns", {75}, rows, 0, "empty");
  expect_bad_corpus("2^31 elements", {1 << 26}, 1 << 26, 32, "2^31");

  kcnn::CorpusIndex idx;
  expect("the corpus", kcnn::build_corpus_index(lengths.data(), (int)lengths.size(), rows, 40, &idx),
         nullptr);
  if (idx.num_utts() != (int)lengths.size() || idx.rows() != rows || idx.starts[0] != 0) {
    printf("WRONG INDEX\n");
    failures++;
  }
  {  // the largest corpus the element limit admits, one column
    kcnn::CorpusIndex big;
    const std::vector<int32_t> two = {2147483646, 1};
    expect("2^31 - 1 rows of one column",
           kcnn::build_corpus_index(two.data(), 2, 2147483647, 1, &big), nullptr);
    const std::vector<int32_t> ends = {0, 2147483645, 2147483646};
    expect_staged("its boundary rows", big, two, ends, 1);
    const int32_t past = 2147483647;
    expect("the row past it", kcnn::check_frames(big, &past, 1, 1), "outside");
  }

  std::vector<int32_t> frames;
  expect("no frames", kcnn::check_frames(idx, frames.data(), 0, 21), "no frames");
  frames = {0, 5, rows};
  expect("an index past the corpus", kcnn::check_frames(idx, frames.data(), 3, 21), "frame 2: row");
  frames = {0, -1, 5};
  expect("a negative index", kcnn::check_frames(idx, frames.data(), 3, 21), "frame 1: row -1");
  frames = {3};
  expect("null frames", kcnn::check_frames(idx, nullptr, 1, 21), "no frames");
  expect("an empty corpus", kcnn::check_frames(kcnn::CorpusIndex(), frames.data(), 1, 21),
         "empty corpus");
  frames.assign(1100, 3);
  expect("2^31 window rows", kcnn::check_frames(idx, frames.data(), 1100, 2000001), "2^31 rows");
  expect("just under 2^31 window rows", kcnn::check_frames(idx, frames.data(), 1073, 2000001),
         nullptr);
  expect("an activation of 2^31 elements",
         kcnn::check_frames_matrix("an activation", 1 << 20, 2048), "2^31");
  expect("an activation of 2^31 rows", kcnn::check_frames_matrix("the input", 1LL << 31, 0),
         "2^31");
  expect("an activation under the limit", kcnn::check_frames_matrix("x", (1 << 20) - 1, 2048),
         nullptr);

  frames.clear();
  for (int32_t r = 0; r < rows; r++) frames.push_back((r * 31) % rows);  // every row, shuffled
  expect_staged("every row", idx, lengths, frames, 21);
  frames.clear();
  int32_t s = 0;
  for (int32_t t : lengths) {  // the boundary indices
    frames.push_back(s);
    frames.push_back(s + t - 1);
    s += t;
  }
  expect_staged("first and last row of each", idx, lengths, frames, 21);
  frames = {34, 34, 0, 34, rows - 1, 0};
  expect_staged("repeats", idx, lengths, frames, 21);
  frames = {rows - 1};
  expect_staged("the last row alone", idx, lengths, frames, 1);
  frames = {0};
  expect_staged("the first row alone", idx, lengths, frames, 1);
  {
    kcnn::CorpusIndex one;
    const std::vector<int32_t> l1 = {1};
    expect("a corpus of one frame", kcnn::build_corpus_index(l1.data(), 1, 1, 40, &one), nullptr);
    expect_staged("its frame, three times", one, l1, {0, 0, 0}, 21);
  }

  printf(failures ? "FAILED: %d\n" : "all frame index checks passed\n", failures);
  return failures ? 1 : 0;
}
