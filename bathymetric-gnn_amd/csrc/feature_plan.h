// The host plan of a feature-label call (include/bgnn_features.h): which features a bin of the grid has to look at, and in which
// order.  Host arithmetic only -- the C ABI's error codes and the standard library, nothing from HIP, no bgnn_ctx -- so that the
// planner can be compiled and checked on its own.  feature_labels.hip owns the device side.
//
// The features are walked from the last to the first, so every bin's list comes out in descending index.  A feature enters the
// list of every bin its disc meets that is still open; a bin closes when a disc holds its four corner cells (a disc is convex: it
// then holds every cell of the bin, and nothing with a lower index can show there).  A survey-sized disc therefore costs one entry
// per interior bin, and the plan stays near sum(bounding-box area) / bin area: it never becomes features x bins.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/bgnn_features.h"

namespace bgnn {

struct FeaturePlanShape {
  int error = BGNN_OK;                // else `message` says why
  std::string message;
  int64_t bins_r = 0, bins_c = 0, bins = 0;
  int64_t entries = 0;
  size_t bytes = 0;                   // 8 * (bins + 1) + 4 * entries
};

inline bool feature_grid_within_limit(int64_t rows, int64_t cols) {
  return rows >= 1 && cols >= 1 && rows <= (int64_t)BGNN_FL_MAX_CELLS / cols;
}

// The argument checks every entry point shares: the shape of the grid and of the table, not the table's contents.
inline void feature_plan_check_shape(FeaturePlanShape &s, const char *who, const int32_t *table, int64_t n_features, int64_t rows,
                                     int64_t cols) {
  char buf[256];
  auto fail = [&](int code) { s.error = code; s.message = buf; };
  if (rows < 1 || cols < 1) {
    snprintf(buf, sizeof(buf), "%s: a grid of %lld x %lld", who, (long long)rows, (long long)cols);
    return fail(BGNN_ERR_INVALID);
  }
  if (n_features < 0 || (n_features > 0 && !table)) {
    snprintf(buf, sizeof(buf), "%s: NULL table or a negative count (%lld features)", who, (long long)n_features);
    return fail(BGNN_ERR_INVALID);
  }
  if (!feature_grid_within_limit(rows, cols)) {
    snprintf(buf, sizeof(buf), "%s: %lld x %lld cells exceed the limit of %lld", who, (long long)rows, (long long)cols,
             (long long)BGNN_FL_MAX_CELLS);
    return fail(BGNN_ERR_UNSUPPORTED);
  }
  if (n_features > (int64_t)BGNN_FL_MAX_FEATURES) {
    snprintf(buf, sizeof(buf), "%s: %lld features exceed the limit of %lld", who, (long long)n_features, (long long)BGNN_FL_MAX_FEATURES);
    return fail(BGNN_ERR_UNSUPPORTED);
  }
  s.bins_r = (rows + BGNN_FL_BIN - 1) / BGNN_FL_BIN;
  s.bins_c = (cols + BGNN_FL_BIN - 1) / BGNN_FL_BIN;
  s.bins = s.bins_r * s.bins_c;
}

// One walk over the table.  count[b] receives the length of bin b's list; with `cursor` (the bins' first positions, advanced here)
// and `feat` the lists are written as well.  Returns false on a table entry outside the contract.
inline bool feature_plan_walk(FeaturePlanShape &s, const int32_t *table, int64_t n_features, int64_t rows, int64_t cols,
                              std::vector<uint8_t> &closed, int64_t *count, int64_t *cursor, int32_t *feat) {
  const int64_t B = BGNN_FL_BIN;
  const int64_t rmax = std::min<int64_t>(rows + cols, 2147483647);
  std::fill(closed.begin(), closed.end(), (uint8_t)0);
  for (int64_t k = n_features - 1; k >= 0; --k) {
    const int64_t row = table[4 * k], col = table[4 * k + 1], rad = table[4 * k + 2];
    if (row < 0 || row >= rows || col < 0 || col >= cols || rad > rmax) {
      char buf[256];
      snprintf(buf, sizeof(buf), "feature %lld: centre (%lld, %lld) with radius %lld outside a grid of %lld x %lld", (long long)k,
               (long long)row, (long long)col, (long long)rad, (long long)rows, (long long)cols);
      s.error = BGNN_ERR_INVALID; s.message = buf;
      return false;
    }
    if (rad < 0) continue;                                      // paints nothing
    const int64_t r2 = rad * rad;                               // < 2^62
    const int64_t b_r0 = std::max<int64_t>(row - rad, 0) / B, b_r1 = std::min(row + rad, rows - 1) / B;
    const int64_t b_c0 = std::max<int64_t>(col - rad, 0) / B, b_c1 = std::min(col + rad, cols - 1) / B;
    for (int64_t br = b_r0; br <= b_r1; ++br) {
      const int64_t lo_r = br * B, hi_r = std::min(lo_r + B, rows) - 1;
      const int64_t near_r = row < lo_r ? lo_r - row : (row > hi_r ? row - hi_r : 0);
      const int64_t far_r = std::max(row - lo_r, hi_r - row);   // the farther of the bin's two edge rows (>= 0 wherever the centre lies)
      for (int64_t bc = b_c0; bc <= b_c1; ++bc) {
        const int64_t b = br * s.bins_c + bc;
        if (closed[b]) continue;
        const int64_t lo_c = bc * B, hi_c = std::min(lo_c + B, cols) - 1;
        const int64_t near_c = col < lo_c ? lo_c - col : (col > hi_c ? col - hi_c : 0);
        if (near_r * near_r + near_c * near_c > r2) continue;   // the disc misses the bin
        const int64_t far_c = std::max(col - lo_c, hi_c - col);
        if (cursor) feat[cursor[b]++] = (int32_t)k;
        ++count[b];
        if (far_r * far_r + far_c * far_c <= r2) closed[b] = 1;   // the farthest corner cell, hence all four
      }
    }
  }
  return true;
}

// The size of the plan.  counts (optional) receives the bins' list lengths.
inline FeaturePlanShape feature_plan_shape(const char *who, const int32_t *table, int64_t n_features, int64_t rows, int64_t cols,
                                           std::vector<int64_t> *counts = nullptr) {
  FeaturePlanShape s;
  feature_plan_check_shape(s, who, table, n_features, rows, cols);
  if (s.error != BGNN_OK) return s;
  std::vector<uint8_t> closed((size_t)s.bins);
  std::vector<int64_t> local;
  std::vector<int64_t> &count = counts ? *counts : local;
  count.assign((size_t)s.bins, 0);
  if (!feature_plan_walk(s, table, n_features, rows, cols, closed, count.data(), nullptr, nullptr)) {
    s.message = std::string(who) + ": " + s.message;
    return s;
  }
  for (int64_t b = 0; b < s.bins; ++b) s.entries += count[b];
  s.bytes = (size_t)8 * (size_t)(s.bins + 1) + (size_t)4 * (size_t)s.entries;
  return s;
}

// Writes the plan (bin_ptr, then bin_feat) into `plan`, which holds at least the bytes of feature_plan_shape.
inline FeaturePlanShape feature_plan_fill(const char *who, const int32_t *table, int64_t n_features, int64_t rows, int64_t cols,
                                          void *plan, size_t plan_bytes) {
  std::vector<int64_t> count;
  FeaturePlanShape s = feature_plan_shape(who, table, n_features, rows, cols, &count);
  if (s.error != BGNN_OK) return s;
  if (plan_bytes < s.bytes) {
    char buf[160];
    snprintf(buf, sizeof(buf), "%s: plan of %zu bytes, %zu needed", who, plan_bytes, s.bytes);
    s.error = BGNN_ERR_INVALID; s.message = buf;
    return s;
  }
  int64_t *bin_ptr = static_cast<int64_t *>(plan);
  int32_t *feat = reinterpret_cast<int32_t *>(bin_ptr + s.bins + 1);
  std::vector<int64_t> cursor((size_t)s.bins);
  int64_t run = 0;
  for (int64_t b = 0; b < s.bins; ++b) { bin_ptr[b] = run; cursor[b] = run; run += count[b]; }
  bin_ptr[s.bins] = run;
  std::vector<uint8_t> closed((size_t)s.bins);
  std::fill(count.begin(), count.end(), (int64_t)0);
  (void)feature_plan_walk(s, table, n_features, rows, cols, closed, count.data(), cursor.data(), feat);
  return s;
}

// What bgnn_feature_labels asks of a plan it is handed before it uploads it: the kernel indexes the table with these entries.
inline bool feature_plan_consistent(const void *plan, size_t plan_bytes, int64_t bins, int64_t n_features, std::string &why) {
  if (plan_bytes < (size_t)8 * (size_t)(bins + 1)) { why = "shorter than its bin_ptr table"; return false; }
  const int64_t *bin_ptr = static_cast<const int64_t *>(plan);
  const int64_t room = (int64_t)((plan_bytes - (size_t)8 * (size_t)(bins + 1)) / 4);
  if (bin_ptr[0] != 0) { why = "bin_ptr[0] is not 0"; return false; }
  for (int64_t b = 0; b < bins; ++b)
    if (bin_ptr[b + 1] < bin_ptr[b]) { why = "bin_ptr decreases"; return false; }
  if (bin_ptr[bins] > room) { why = "bin_ptr ends beyond the plan"; return false; }
  const int32_t *feat = reinterpret_cast<const int32_t *>(bin_ptr + bins + 1);
  for (int64_t e = 0; e < bin_ptr[bins]; ++e)
    if (feat[e] < 0 || (int64_t)feat[e] >= n_features) { why = "an entry outside the table"; return false; }
  return true;
}

}  // namespace bgnn
