// capi/xent-labels.h -- host-side checking and staging of the label list of
// kcnn_nnet_backprop_xent / kcnn_comp_objf_and_deriv (the reference's
// std::vector<MatrixElement<BaseFloat> >).  Pure host code with no GPU call:
// a bad label is refused here, before any launch, so it can never become an
// out-of-range device access.  Header-only so that a stand-alone program can
// run it under a host sanitizer (scripts/xent_labels_check.cc).
#ifndef KCNN_CAPI_XENT_LABELS_H_
#define KCNN_CAPI_XENT_LABELS_H_

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

namespace kcnn {

// 0 <= row < num_rows, 0 <= col < num_cols and no repeated (row, col); with
// `sorted`, rows non-decreasing as well.  Returns "" or what is wrong.
inline std::string check_labels(const int32_t *rows, const int32_t *cols, int num, int num_rows,
                                int num_cols, bool sorted) {
  std::ostringstream err;
  if (num < 0 || (num > 0 && (rows == nullptr || cols == nullptr))) return "bad label arrays";
  for (int i = 0; i < num; i++) {
    if (rows[i] < 0 || rows[i] >= num_rows) {
      err << "label " << i << ": row " << rows[i] << " outside [0, " << num_rows << ")";
      return err.str();
    }
    if (cols[i] < 0 || cols[i] >= num_cols) {
      err << "label " << i << ": column " << cols[i] << " outside [0, " << num_cols << ")";
      return err.str();
    }
    if (sorted && i > 0 && rows[i] < rows[i - 1]) {
      err << "label " << i << ": rows are not sorted (" << rows[i] << " after " << rows[i - 1]
          << ")";
      return err.str();
    }
  }
  std::vector<std::pair<int32_t, int32_t> > seen(num);
  for (int i = 0; i < num; i++) seen[i] = std::make_pair(rows[i], cols[i]);
  std::sort(seen.begin(), seen.end());
  for (int i = 1; i < num; i++)
    if (seen[i] == seen[i - 1]) {
      err << "element (" << seen[i].first << ", " << seen[i].second << ") is repeated";
      return err.str();
    }
  return "";
}

// The staged image, one block copied to the device in one transfer:
//   int32 row_start[num_rows + 1] | int32 row[num] | int32 col[num] | float weight[num]
struct LabelLayout {
  size_t row_start, row, col, weight, bytes;  // byte offsets, total
};
inline LabelLayout label_layout(int num, int num_rows) {
  LabelLayout l;
  l.row_start = 0;
  l.row = sizeof(int32_t) * ((size_t)num_rows + 1);
  l.col = l.row + sizeof(int32_t) * (size_t)num;
  l.weight = l.col + sizeof(int32_t) * (size_t)num;
  l.bytes = l.weight + sizeof(float) * (size_t)num;
  return l;
}

// Fills `staging` (label_layout(num, num_rows).bytes bytes) from CHECKED
// labels sorted by row.
inline void stage_labels(const int32_t *rows, const int32_t *cols, const float *weights, int num,
                         int num_rows, void *staging) {
  const LabelLayout l = label_layout(num, num_rows);
  char *base = static_cast<char *>(staging);
  int32_t *row_start = reinterpret_cast<int32_t *>(base + l.row_start);
  int i = 0;
  for (int r = 0; r <= num_rows; r++) {
    while (i < num && rows[i] < r) i++;
    row_start[r] = i;
  }
  if (num > 0) {
    memcpy(base + l.row, rows, sizeof(int32_t) * (size_t)num);
    memcpy(base + l.col, cols, sizeof(int32_t) * (size_t)num);
    memcpy(base + l.weight, weights, sizeof(float) * (size_t)num);
  }
}

}  // namespace kcnn

#endif  // KCNN_CAPI_XENT_LABELS_H_
