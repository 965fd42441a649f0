// capi/frame-index.h -- host-side checking and staging of a minibatch given
// as corpus row indices (kcnn_nnet_propagate_frames / _compute_prob_frames):
// the corpus handle's utterance starts, the checks of a frame list against
// them, and the {row, first row, last row of its utterance} triple per example
// that kn_splice_frames_prop reads (nnet2/nnet-kernels.h); and the runs of
// consecutive rows of such a list, with their device image, for a training
// step over time maps (kcnn_nnet_propagate_frames_shared).  Pure host code
// with no GPU call: a bad index is refused here, before any launch, so it can
// never become an out-of-range device access.  Header-only so that a
// stand-alone program can run it under a host sanitizer
// (scripts/frame_index_check.cc).
#ifndef KCNN_CAPI_FRAME_INDEX_H_
#define KCNN_CAPI_FRAME_INDEX_H_

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <sstream>
#include <string>
#include <vector>

namespace kcnn {

// The utterances of a corpus [rows x cols] stacked row-wise: utterance u holds
// rows [starts[u], starts[u + 1]).  Built once per corpus, so a minibatch does
// no O(utterances) work.
struct CorpusIndex {
  std::vector<int32_t> starts;  // num_utts + 1 entries, ascending from 0 to the rows
  int32_t rows() const { return starts.empty() ? 0 : starts.back(); }
  int num_utts() const { return starts.empty() ? 0 : (int)starts.size() - 1; }
};

constexpr int64_t kFrameIndexLimit = (int64_t)1 << 31;  // rows and elements of a matrix

// The prefix array of `lengths` into *index: every length >= 1, their sum the
// corpus's rows, rows x cols below 2^31.  Returns "" or what is wrong, *index
// then being unchanged.
inline std::string build_corpus_index(const int32_t *lengths, int num_utts, int64_t rows,
                                      int64_t cols, CorpusIndex *index) {
  std::ostringstream err;
  if (lengths == nullptr || num_utts < 1) return "no utterances";
  if (rows < 1 || cols < 1 || rows * cols >= kFrameIndexLimit) {
    err << "a corpus of " << rows << " x " << cols << " is empty or reaches 2^31 elements";
    return err.str();
  }
  if (num_utts > rows) {  // (before the starts are sized by it)
    err << num_utts << " utterances of at least 1 frame in a corpus of " << rows << " rows";
    return err.str();
  }
  std::vector<int32_t> starts((size_t)num_utts + 1);
  int64_t sum = 0;
  for (int u = 0; u < num_utts; u++) {
    if (lengths[u] < 1) {
      err << "utterance " << u << " has " << lengths[u] << " frames; at least 1 is needed";
      return err.str();
    }
    starts[u] = sum <= rows ? (int32_t)sum : 0;  // (rows is below 2^31)
    sum += lengths[u];
  }
  if (sum != rows) {
    err << "the lengths sum to " << sum << ", the corpus has " << rows << " rows";
    return err.str();
  }
  starts[num_utts] = (int32_t)sum;
  index->starts.swap(starts);
  return "";
}

// A frame list against the corpus: at least one frame, every index a corpus
// row, and num x chunk_rows (the rows of the window matrix Propagate would be
// given: one per input chunk offset and example) below 2^31.
inline std::string check_frames(const CorpusIndex &corpus, const int32_t *frames, int num,
                                int chunk_rows) {
  std::ostringstream err;
  if (frames == nullptr || num < 1) return "no frames";
  if (corpus.num_utts() < 1) return "an empty corpus";
  if ((int64_t)num * chunk_rows >= kFrameIndexLimit) {
    err << num << " frames of " << chunk_rows << " input rows each reach 2^31 rows";
    return err.str();
  }
  const int32_t rows = corpus.rows();
  for (int i = 0; i < num; i++)
    if (frames[i] < 0 || frames[i] >= rows) {
      err << "frame " << i << ": row " << frames[i] << " outside [0, " << rows << ")";
      return err.str();
    }
  return "";
}

// "" when a matrix of rows x cols stays below 2^31 rows and elements.
inline std::string check_frames_matrix(const char *what, int64_t rows, int64_t cols) {
  if (rows < kFrameIndexLimit && rows * cols < kFrameIndexLimit) return "";
  std::ostringstream err;
  err << what << " of " << rows << " x " << cols << " reaches 2^31 rows or elements";
  return err.str();
}

inline size_t frame_triples_bytes(int num) { return sizeof(int32_t) * 3 * (size_t)num; }

// Fills `staging` (frame_triples_bytes(num) bytes) from a CHECKED list:
// example n's {frames[n], first row of its utterance, last row of it}.  The
// utterance is found by a binary search over the starts.
inline void stage_frames(const CorpusIndex &corpus, const int32_t *frames, int num,
                         void *staging) {
  int32_t *out = static_cast<int32_t *>(staging);
  const std::vector<int32_t> &s = corpus.starts;
  for (int i = 0; i < num; i++) {
    // the first start past the row; the one before it is the row's utterance
    const size_t u = (size_t)(std::upper_bound(s.begin(), s.end() - 1, frames[i]) - s.begin()) - 1;
    out[3 * (size_t)i] = frames[i];
    out[3 * (size_t)i + 1] = s[u];
    out[3 * (size_t)i + 2] = s[u + 1] - 1;
  }
}

// A run of a CHECKED frame list (kcnn_nnet_propagate_frames_shared): a maximal
// stretch of list entries with frames[i + 1] == frames[i] + 1 and both rows in
// one utterance.  Any list is legal -- any order, repeats, runs of one frame --
// and the runs are stretches of the list itself, so example n stays frames[n].
struct FrameRun {
  int32_t first, length;  // r0, the corpus row of its first example, and k
  int32_t lo, hi;         // the first and the last row of its utterance
};

inline std::vector<FrameRun> frame_runs(const CorpusIndex &corpus, const int32_t *frames,
                                        int num) {
  std::vector<FrameRun> runs;
  const std::vector<int32_t> &s = corpus.starts;
  for (int i = 0; i < num; i++) {
    if (!runs.empty()) {
      FrameRun &r = runs.back();
      if (frames[i] == r.first + r.length && frames[i] <= r.hi) {
        r.length++;
        continue;
      }
    }
    const size_t u = (size_t)(std::upper_bound(s.begin(), s.end() - 1, frames[i]) - s.begin()) - 1;
    runs.push_back(FrameRun{frames[i], 1, s[u], s[u + 1] - 1});
  }
  return runs;
}

// The device image of the runs, which kn_timemap_layout reads: the num_runs + 1
// starts of the runs' result rows (the prefix of their lengths), then {r0,
// first row, last row} per run, as stage_frames stages an example's triple.
inline size_t run_image_bytes(size_t num_runs) { return sizeof(int32_t) * (4 * num_runs + 1); }

inline void stage_runs(const std::vector<FrameRun> &runs, void *staging) {
  int32_t *starts = static_cast<int32_t *>(staging), *tri = starts + runs.size() + 1;
  starts[0] = 0;
  for (size_t j = 0; j < runs.size(); j++) {
    starts[j + 1] = starts[j] + runs[j].length;
    tri[3 * j] = runs[j].first;
    tri[3 * j + 1] = runs[j].lo;
    tri[3 * j + 2] = runs[j].hi;
  }
}

}  // namespace kcnn

#endif  // KCNN_CAPI_FRAME_INDEX_H_
