// scripts/xent_labels_check.cc -- the label checking and staging routine of
// kcnn_nnet_backprop_xent (kaldi-cnn_amd/src/capi/xent-labels.h) as a
// stand-alone host program, for a run under a host sanitizer.  No GPU call.
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ikaldi-cnn_amd/src scripts/xent_labels_check.cc -o xent_labels_check
//   ./xent_labels_check
//
// Runs the four kinds of bad list (row / column out of range, unsorted rows,
// a repeated pair) and valid lists (empty, one label a row, several a row,
// rows without labels), staging the valid ones into an exactly-sized heap
// buffer so that a write past either end is caught.
#include <stdio.h>
#include <stdlib.h>

#include "capi/xent-labels.h"

namespace {

struct Labels {
  std::vector<int32_t> rows, cols;
  std::vector<float> w;
  void add(int r, int c, float weight) {
    rows.push_back(r);
    cols.push_back(c);
    w.push_back(weight);
  }
};

int failures = 0;

void expect_bad(const char *what, const Labels &l, int num_rows, int num_cols, const char *word) {
  const std::string err = kcnn::check_labels(l.rows.data(), l.cols.data(), (int)l.rows.size(),
                                             num_rows, num_cols, true);
  const bool ok = err.find(word) != std::string::npos;
  printf("%-28s %s  (%s)\n", what, ok ? "refused" : "NOT REFUSED", err.c_str());
  if (!ok) failures++;
}

void expect_good(const char *what, const Labels &l, int num_rows, int num_cols) {
  const int num = (int)l.rows.size();
  const std::string err = kcnn::check_labels(l.rows.data(), l.cols.data(), num, num_rows,
                                             num_cols, true);
  if (!err.empty()) {
    printf("%-28s REFUSED (%s)\n", what, err.c_str());
    failures++;
    return;
  }
  const kcnn::LabelLayout lay = kcnn::label_layout(num, num_rows);
  char *buf = static_cast<char *>(malloc(lay.bytes));  // exact size
  kcnn::stage_labels(l.rows.data(), l.cols.data(), l.w.data(), num, num_rows, buf);
  const int32_t *start = reinterpret_cast<const int32_t *>(buf + lay.row_start);
  const int32_t *col = reinterpret_cast<const int32_t *>(buf + lay.col);
  const float *w = reinterpret_cast<const float *>(buf + lay.weight);
  bool ok = start[0] == 0 && start[num_rows] == num;
  for (int r = 0; r < num_rows && ok; r++) {
    ok = start[r] <= start[r + 1];
    for (int i = start[r]; i < start[r + 1] && ok; i++)
      ok = l.rows[i] == r && col[i] == l.cols[i] && w[i] == l.w[i];
  }
  printf("%-28s %s  (%d labels, %zu bytes staged)\n", what, ok ? "staged" : "WRONG IMAGE", num,
         lay.bytes);
  if (!ok) failures++;
  free(buf);
}

}  // namespace

int main() {
  const int N = 37, D = 10;
  Labels one;
  for (int r = 0; r < N; r++) one.add(r, (r * 7) % D, 1.0f);

  Labels bad = one;
  bad.add(N, 0, 1.0f);
  expect_bad("row past the end", bad, N, D, "outside");
  bad = one;
  bad.rows[0] = -1;
  expect_bad("negative row", bad, N, D, "outside");
  bad = one;
  bad.cols[5] = D;
  expect_bad("column past the end", bad, N, D, "outside");
  bad = one;
  bad.cols[5] = -3;
  expect_bad("negative column", bad, N, D, "outside");
  bad = one;
  std::swap(bad.rows[3], bad.rows[4]);
  expect_bad("unsorted rows", bad, N, D, "not sorted");
  bad = Labels();
  bad.add(3, 1, 0.5f);
  bad.add(3, 2, 0.25f);
  bad.add(3, 1, 0.25f);
  expect_bad("repeated pair", bad, N, D, "repeated");

  expect_good("empty list", Labels(), N, D);
  expect_good("one label a row", one, N, D);
  Labels soft;
  for (int r = 0; r < N; r++) {
    if (r % 5 == 2) continue;  // rows without a label
    for (int k = 0; k <= r % 3; k++) soft.add(r, (r + 3 * k) % D, 0.125f * (k + 1));
  }
  expect_good("several a row, gaps", soft, N, D);
  Labels last;
  last.add(N - 1, D - 1, 1.0f);
  expect_good("only the last element", last, N, D);

  printf(failures ? "FAILED: %d\n" : "all label checks passed\n", failures);
  return failures ? 1 : 0;
}
