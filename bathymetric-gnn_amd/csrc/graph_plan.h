// The layout of one tile batch: everything bgnn_graph_build works out on the host before it touches the device.  Host arithmetic
// only -- the C ABI's error codes and the standard library, nothing from HIP, no bgnn_ctx -- so that the planner can be compiled and
// checked on its own (tests/graph_plan_check.cpp).  One entry point, plan_graph: a pure function of the batch's shapes and
// resolutions, the stencil, the CU count and the ragged_atlas option.  graph_api.hip owns the device side: the handle, the
// table cache, the buffers, the uploads.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/bgnn.h"

// Per-tile metadata (device + host copy)
struct BgnnTileMeta {
  int32_t h, w;
  int32_t cell_off;   // first cell of the tile in the concatenated cell space
  int32_t pad;
  double rx, ry;      // resolution (x, y)
};

// Work item of the tile-structured kernels: a band of rows of one tile
struct BgnnWorkItem {
  int32_t tile, r0, nr, pad;
};

namespace bgnn {

struct GraphPlan {
  int error = BGNN_OK;                // BGNN_ERR_INVALID: `message` says why, nothing else is filled
  std::string message;
  std::vector<BgnnTileMeta> h_tiles;
  int64_t cells = 0;
  int32_t item_cells = 0;             // cells per row band of the feature kernel
  std::vector<BgnnWorkItem> items;    // row bands {tile, r0, nr}
  bool uniform = true;                // every tile has the shape of the first
  int32_t uni_h = 0, uni_w = 0;       // that shape (0: ragged)
  int32_t bh2 = 0, bw2 = 0, n_blocks2 = 0;   // 16x16 blocks: per tile (uniform), in all
  int32_t bh3 = 0, bw3 = 0, n_blocks3 = 0;   // 8x16 blocks
  int32_t max_h = 0, max_w = 0;
  // ragged batches: the per-grid block lists {tile, r0, c0} ...
  std::vector<BgnnWorkItem> items2, items3;
  // ... and the shelf-packed canvas; atlas_h == 0: none (uniform batch, one grid, ragged_atlas off, or rejected: no fewer blocks)
  int32_t atlas_w = 0, atlas_h = 0;
  std::vector<int32_t> atlas_pos;     // [n_tiles][2] = (row, column) of each grid's origin on the canvas
  BgnnTileMeta atlas_meta{};          // the canvas as ONE tile
  // uniform batches at one resolution share their two tables through the context's cache; the key is
  // (n_tiles, uni_h, uni_w, item_cells, rx, ry)
  bool cacheable = false;
  double rx = 0.0, ry = 0.0;
  // ragged batches: every host-built table travels in ONE block (one staging copy, one H2D) -- with 50 000-node VR batches the
  // per-batch host work is what bounds the stream.  Offsets are 256-byte aligned; o_items3 or (o_atile, o_apos) is used
  std::vector<char> block;
  size_t o_tiles = 0, o_items = 0, o_items2 = 0, o_items3 = 0, o_atile = 0, o_apos = 0;
};

inline GraphPlan plan_graph(int n_tiles, const int32_t *hw, const double *resolution, int K, int num_cus, int ragged_atlas) {
  GraphPlan p;
  auto fail = [&p](const char *fmt, int a = 0, int b = 0, int c = 0) {
    char buf[256];
    snprintf(buf, sizeof(buf), fmt, a, b, c);
    p.error = BGNN_ERR_INVALID; p.message = buf;
  };
  int64_t cells_est = 0;
  for (int t = 0; t < n_tiles; ++t) cells_est += (int64_t)hw[2 * t] * hw[2 * t + 1];
  p.item_cells = (int32_t)std::min<int64_t>(2048, std::max<int64_t>(256, cells_est / (4 * num_cus)));
  p.h_tiles.resize(n_tiles);
  for (int t = 0; t < n_tiles; ++t) {
    const int h = hw[2 * t], w = hw[2 * t + 1];
    if (h < 2 || w < 2) {
      // np.gradient needs >= 2 samples per axis: the reference raises ValueError here too
      fail("Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) elements are "
           "required. (tile %d is %dx%d)", t, h, w);
      return p;
    }
    BgnnTileMeta &m = p.h_tiles[t];
    m.h = h; m.w = w; m.cell_off = (int32_t)p.cells; m.pad = 0;
    m.rx = resolution[2 * t]; m.ry = resolution[2 * t + 1];
    p.cells += (int64_t)h * w;
    if (p.cells >= ((int64_t)1 << 30)) { fail("batch too large: 2^30 cells or more; split it"); return p; }
    // row bands of the feature kernel: ~2048 cells each for big batches, down to one 256-thread pass (256 cells) when the
    // batch is small, so that a single tile still spreads over the whole chip
    int rows_per = std::max(1, p.item_cells / w);
    for (int r0 = 0; r0 < h; r0 += rows_per) p.items.push_back({t, r0, std::min(rows_per, h - r0), 0});
    if (h != hw[0] || w != hw[1]) p.uniform = false;
    if (h > p.max_h) p.max_h = h;
    if (w > p.max_w) p.max_w = w;
  }
  if (p.uniform) {
    p.uni_h = hw[0]; p.uni_w = hw[1];
    p.bh2 = (p.uni_h + 15) / 16; p.bw2 = (p.uni_w + 15) / 16;
    p.n_blocks2 = n_tiles * p.bh2 * p.bw2;
    p.bh3 = (p.uni_h + 7) / 8; p.bw3 = p.bw2;
    p.n_blocks3 = n_tiles * p.bh3 * p.bw3;
    p.cacheable = true;
    p.rx = resolution[0]; p.ry = resolution[1];
    for (int t = 1; t < n_tiles && p.cacheable; ++t)
      p.cacheable = resolution[2 * t] == resolution[0] && resolution[2 * t + 1] == resolution[1];
    return p;
  }
  for (int t = 0; t < n_tiles; ++t)
    for (int r0 = 0; r0 < p.h_tiles[t].h; r0 += 16)
      for (int c0 = 0; c0 < p.h_tiles[t].w; c0 += 16) p.items2.push_back({t, r0, c0, 0});
  p.n_blocks2 = (int32_t)p.items2.size();
  for (int t = 0; t < n_tiles; ++t)
    for (int r0 = 0; r0 < p.h_tiles[t].h; r0 += 8)
      for (int c0 = 0; c0 < p.h_tiles[t].w; c0 += 16) p.items3.push_back({t, r0, c0, 0});
  p.n_blocks3 = (int32_t)p.items3.size();
  // shelf-pack the grids (tallest first) onto a canvas for the fused layer kernels
  if (n_tiles >= 2 && ragged_atlas) {
    const int G = K == 16 ? 2 : 1;                                      // gutter = reach of the stencil
    // First-fit shelves, grids by decreasing height (wider first among equals): a grid goes into the first shelf that is tall enough
    // and has room, else it opens a new shelf.  A few canvas widths around sqrt(cells) are tried and the one with the fewest 8 x 16
    // blocks wins -- a 50 000-node batch of refinement grids then needs ~480 blocks instead of ~525 (one width, next-fit), i.e. ONE
    // round of workgroups on 512 slots instead of one and a bit.  (~10 us of host work per batch.)
    std::vector<int> order(n_tiles);
    for (int t = 0; t < n_tiles; ++t) order[t] = t;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
      return p.h_tiles[a].h != p.h_tiles[b].h ? p.h_tiles[a].h > p.h_tiles[b].h : p.h_tiles[a].w > p.h_tiles[b].w;
    });
    struct Shelf { int y, h, x; };
    std::vector<Shelf> shelves;
    auto pack = [&](int aw, int32_t *pos) -> int {                      // -> canvas height (before rounding to whole blocks)
      shelves.clear();
      int y = 0;
      for (int t : order) {
        const int h = p.h_tiles[t].h, w = p.h_tiles[t].w;
        bool placed = false;
        for (auto &sh : shelves)
          if (sh.x + w <= aw && h <= sh.h) {
            if (pos) { pos[2 * t] = sh.y; pos[2 * t + 1] = sh.x; }
            sh.x += w + G; placed = true;
            break;
          }
        if (!placed) {
          if (pos) { pos[2 * t] = y; pos[2 * t + 1] = 0; }
          shelves.push_back({y, h, w + G});
          y += h + G;
        }
      }
      return y - G;
    };
    const int aw_min = ((p.max_w + G + 15) / 16) * 16;
    const int side = (int)std::sqrt((double)p.cells);
    int aw = 0, ah = 0;
    int64_t best = -1;
    // <= 9 candidates between 0.9 and 1.5 sqrt(cells) (<= 4 for batches of many hundred grids: there the host time counts and a round more or less does not)
    const int step = std::max(16, (side * 6 / 10 / (n_tiles > 400 ? 3 : 8) + 15) / 16 * 16);
    for (int cand = std::max(aw_min, (side * 9 / 10 + 15) / 16 * 16);; cand += step) {
      const int hc = ((pack(cand, nullptr) + 7) / 8) * 8;
      const int64_t blocks = (int64_t)(hc / 8) * (cand / 16);
      if (best < 0 || blocks < best) { best = blocks; aw = cand; ah = hc; }
      if (cand >= side * 3 / 2 || cand + step > 8192) break;            // (always at least one candidate)
    }
    p.atlas_pos.assign((size_t)n_tiles * 2, 0);
    (void)pack(aw, p.atlas_pos.data());
    // worth it only if the canvas has fewer blocks than the grids have on their own (refinement grids: yes; two big tiles of
    // different size: no -- they fill their own blocks already and would leave half a canvas empty)
    if ((int64_t)(ah / 8) * (aw / 16) < (int64_t)p.items3.size()) {
      p.atlas_w = aw; p.atlas_h = ah;
      p.atlas_meta.h = ah; p.atlas_meta.w = aw; p.atlas_meta.cell_off = 0; p.atlas_meta.rx = 1.0; p.atlas_meta.ry = 1.0;
    }
  }
  auto put = [&p](const void *src, size_t bytes) {
    const size_t at = (p.block.size() + 255) & ~(size_t)255;
    p.block.resize(at + bytes);
    memcpy(p.block.data() + at, src, bytes);
    return at;
  };
  p.o_tiles = put(p.h_tiles.data(), sizeof(BgnnTileMeta) * p.h_tiles.size());
  p.o_items = put(p.items.data(), sizeof(BgnnWorkItem) * p.items.size());
  p.o_items2 = put(p.items2.data(), sizeof(BgnnWorkItem) * p.items2.size());
  if (p.atlas_h) {
    p.o_atile = put(&p.atlas_meta, sizeof(p.atlas_meta));
    p.o_apos = put(p.atlas_pos.data(), sizeof(int32_t) * p.atlas_pos.size());
  } else {
    p.o_items3 = put(p.items3.data(), sizeof(BgnnWorkItem) * p.items3.size());
  }
  return p;
}

}  // namespace bgnn
