// The host side of include/bgnn_tilestore.h: the check every box passes before a scan or a cut is launched, and the two interval
// tests of the cut.  Host only, no HIP: tests/tile_boxes_check.cpp compiles this header alone.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

#include "../../include/bgnn_tilestore.h"

namespace bgnn {

static_assert(sizeof(bgnn_tile_box) == BGNN_TILE_BOX_BYTES, "a box is four 8-byte words");

struct TileBoxCheck {
  bool ok = true;
  std::string message;        // why not
  int64_t max_bands = 0;      // bands of BGNN_TILE_BAND_ROWS rows of the tallest box
};

// Every box inside [0, rows) x [0, cols), h, w > 0, dst >= 0 and, with dst_cells >= 0, dst + h * w <= dst_cells.  No sum here can
// overflow: row0 <= rows - h is compared, not row0 + h, and h * w < 2^62.
inline TileBoxCheck tile_boxes_check(const bgnn_tile_box *boxes, int64_t n_boxes, int64_t rows, int64_t cols, int64_t dst_cells) {
  TileBoxCheck c;
  auto fail = [&](int64_t k, const char *why) {
    char buf[256];
    const bgnn_tile_box &b = boxes[k];
    snprintf(buf, sizeof buf, "box %lld (row0 %lld, col0 %lld, %d x %d, dst %lld) %s", (long long)k, (long long)b.row0,
             (long long)b.col0, (int)b.h, (int)b.w, (long long)b.dst, why);
    c.ok = false;
    c.message = buf;
    return c;
  };
  for (int64_t k = 0; k < n_boxes; ++k) {
    const bgnn_tile_box &b = boxes[k];
    if (b.h <= 0 || b.w <= 0) return fail(k, "is empty");
    if (b.row0 < 0 || b.col0 < 0 || b.h > rows || b.w > cols || b.row0 > rows - b.h || b.col0 > cols - b.w)
      return fail(k, "leaves the plane");
    if (b.dst < 0) return fail(k, "has a negative destination");
    const int64_t cells = (int64_t)b.h * b.w;
    if (dst_cells >= 0 && (cells > dst_cells || b.dst > dst_cells - cells)) return fail(k, "ends past the store");
    const int64_t bands = ((int64_t)b.h + BGNN_TILE_BAND_ROWS - 1) / BGNN_TILE_BAND_ROWS;
    if (bands > c.max_bands) c.max_bands = bands;
  }
  return c;
}

// [a, a + a_bytes) and [b, b + b_bytes) share a byte
inline bool ranges_overlap(uintptr_t a, uint64_t a_bytes, uintptr_t b, uint64_t b_bytes) {
  if (a_bytes == 0 || b_bytes == 0) return false;
  return a < b ? (uint64_t)(b - a) < a_bytes : (uint64_t)(a - b) < b_bytes;
}

}  // namespace bgnn
