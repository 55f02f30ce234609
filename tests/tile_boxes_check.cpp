// Stand-alone host program around csrc/tile_boxes.h (the box check of bgnn_tile_scan / bgnn_tile_cut and the interval test of the
// cut) and the planning arithmetic of plan_tile_boxes restated in C++: no HIP, no library.  tests/test_host_tile_plan.py compiles
// and runs it; it is also what an address / undefined-behaviour sanitizer build of that host code runs.
// Prints one line per case, "name: ok" or "name: FAILED ..."; the exit status is the number of failures.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../bathymetric-gnn_amd/csrc/tile_boxes.h"

using bgnn::tile_boxes_check;

static int failures = 0;
static void report(const char *name, bool ok, const std::string &detail = "") {
  printf("%s: %s%s%s\n", name, ok ? "ok" : "FAILED", detail.empty() ? "" : " ", detail.c_str());
  if (!ok) ++failures;
}

// GroundTruthDataset._scan_ground_truth's candidates: the stride grid, then the far-corner tile
static std::vector<bgnn_tile_box> plan(int64_t height, int64_t width, int32_t tile, int32_t overlap) {
  std::vector<bgnn_tile_box> boxes;
  const int64_t stride = tile - overlap;
  if (stride <= 0) return boxes;
  int64_t dst = 0;
  auto add = [&](int64_t r0, int64_t c0) {
    boxes.push_back(bgnn_tile_box{r0, c0, tile, tile, dst});
    dst += (int64_t)tile * tile;
  };
  for (int64_t r0 = 0; r0 + tile <= height; r0 += stride)
    for (int64_t c0 = 0; c0 + tile <= width; c0 += stride) add(r0, c0);
  if (height > tile && width > tile && (height % stride != 0 || width % stride != 0)) add(height - tile, width - tile);
  return boxes;
}

static void planned(const char *name, int64_t height, int64_t width, int32_t tile, int32_t overlap, size_t want, int64_t want_bands) {
  const std::vector<bgnn_tile_box> boxes = plan(height, width, tile, overlap);
  const auto c = tile_boxes_check(boxes.data(), (int64_t)boxes.size(), height, width, (int64_t)boxes.size() * tile * tile);
  char buf[128];
  snprintf(buf, sizeof buf, "(%zu boxes, %lld bands) %s", boxes.size(), (long long)c.max_bands, c.message.c_str());
  report(name, c.ok && boxes.size() == want && c.max_bands == want_bands, buf);
}

static void refused(const char *name, bgnn_tile_box b, int64_t rows, int64_t cols, int64_t dst_cells, const char *why) {
  const bgnn_tile_box boxes[2] = {{0, 0, 1, 1, 0}, b};          // a good box in front: the check walks on to the bad one
  const auto c = tile_boxes_check(boxes, 2, rows, cols, dst_cells);
  report(name, !c.ok && c.message.find(why) != std::string::npos && c.message.find("box 1 ") == 0, c.message);
}

int main() {
  planned("plan_150x131", 150, 131, 32, 8, 5 * 5 + 1, 1);
  planned("plan_72x96", 72, 96, 32, 8, 2 * 3, 1);
  planned("plan_32x90", 32, 90, 32, 8, 3, 1);
  planned("plan_20x100", 20, 100, 32, 8, 0, 0);
  planned("plan_33x33", 33, 33, 32, 8, 2, 1);
  planned("plan_46400", 46400, 46400, 512, 64, 103 * 103 + 1, 16);
  planned("plan_stride_0", 100, 100, 32, 32, 0, 0);

  const int64_t big = INT64_MAX, i32 = 2147483647;
  refused("empty_h", {0, 0, 0, 4, 0}, 10, 10, -1, "is empty");
  refused("empty_w", {0, 0, 4, 0, 0}, 10, 10, -1, "is empty");
  refused("negative_h", {0, 0, -4, 4, 0}, 10, 10, -1, "is empty");
  refused("negative_row", {-1, 0, 4, 4, 0}, 10, 10, -1, "leaves the plane");
  refused("negative_col", {0, -1, 4, 4, 0}, 10, 10, -1, "leaves the plane");
  refused("past_rows", {7, 0, 4, 4, 0}, 10, 10, -1, "leaves the plane");
  refused("past_cols", {0, 7, 4, 4, 0}, 10, 10, -1, "leaves the plane");
  refused("taller_than_plane", {0, 0, 11, 4, 0}, 10, 10, -1, "leaves the plane");
  refused("row0_at_int64_max", {big, 0, 4, 4, 0}, 10, 10, -1, "leaves the plane");          // row0 + h would overflow
  refused("col0_at_int64_max", {0, big, 4, 4, 0}, 10, 10, -1, "leaves the plane");
  refused("negative_dst", {0, 0, 4, 4, -1}, 10, 10, -1, "negative destination");
  refused("past_store", {0, 0, 4, 4, 1}, 10, 10, 16, "ends past the store");
  refused("dst_at_int64_max", {0, 0, 4, 4, big}, 10, 10, 1 << 20, "ends past the store");   // dst + h * w would overflow
  refused("tile_larger_than_store", {0, 0, 4, 4, 0}, 10, 10, 15, "ends past the store");
  refused("huge_tile_small_store", {0, 0, (int32_t)i32, (int32_t)i32, 0}, big, big, 1 << 20, "ends past the store");

  {
    const bgnn_tile_box edge[3] = {{6, 6, 4, 4, 0}, {0, 0, 10, 10, 16}, {9, 9, 1, 1, 116}};   // flush with the far edges and the store's end
    const auto c = tile_boxes_check(edge, 3, 10, 10, 117);
    report("flush_boxes", c.ok && c.max_bands == 1, c.message);
    const bgnn_tile_box tall = {0, 0, (int32_t)i32, 1, 0};
    const auto t = tile_boxes_check(&tall, 1, big, big, -1);
    report("tallest_box", t.ok && t.max_bands == (i32 + 31) / 32, t.message);
    report("no_boxes", tile_boxes_check(nullptr, 0, 10, 10, 0).ok);
  }

  using bgnn::ranges_overlap;
  report("overlap_inside", ranges_overlap(100, 50, 120, 4));
  report("overlap_touching", !ranges_overlap(100, 20, 120, 4) && !ranges_overlap(120, 4, 100, 20));
  report("overlap_reversed", ranges_overlap(120, 4, 100, 21));
  report("overlap_empty", !ranges_overlap(100, 0, 100, 8) && !ranges_overlap(100, 8, 100, 0));
  report("overlap_top_of_memory", !ranges_overlap(UINTPTR_MAX - 7, 8, 0, 8) && ranges_overlap(UINTPTR_MAX - 7, 8, UINTPTR_MAX - 3, 4));
  return failures;
}
