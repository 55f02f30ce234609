// Stand-alone check of csrc/graph_plan.h (no HIP, no GPU): for a list of tile batches, the plan's scalars and a hash of its tables
// as one JSON document on stdout, and the plan's invariants as properties ("props": "ok" or the first one broken): row bands and
// block lists cover every tile exactly once, the ragged block's offsets are aligned and tile it, the canvas holds every grid with the
// gutter between any two.  tests/test_host_graph_plan.py compiles it, runs it and compares the document with
// tests/golden/graph_plan.json.
#include <stdio.h>

#include <set>
#include <utility>

#include "../bathymetric-gnn_amd/csrc/graph_plan.h"

// ---- cases ----------------------------------------------------------------------------------------------------------------------
struct Case {
  std::string name;
  std::vector<int32_t> hw;
  std::vector<double> res;
  int K, cus, atlas;
};

static Case make_case(const char *name, std::vector<std::pair<int, int>> shapes, int K, int cus, int atlas, double rx = 0.5, double ry = 0.5) {
  Case c{name, {}, {}, K, cus, atlas};
  for (auto &s : shapes) { c.hw.push_back(s.first); c.hw.push_back(s.second); c.res.push_back(rx); c.res.push_back(ry); }
  return c;
}

// the shapes of test_ragged_batch_canvas_walk_equals_per_grid_blocks (tests/test_gpu_forward.py)
static const std::vector<std::pair<int, int>> kVrShapes = {
    {35, 41}, {4, 41}, {25, 27}, {33, 16}, {50, 5}, {16, 21}, {30, 22}, {9, 5}, {3, 5}, {10, 50}, {12, 34}, {39, 14}, {16, 23},
    {15, 49}, {11, 46}, {41, 43}, {8, 21}, {33, 26}, {34, 35}, {34, 5}, {49, 29}, {46, 16}, {20, 45}, {11, 6}, {20, 35}, {8, 44},
    {19, 13}, {29, 45}, {45, 44}, {17, 3}, {40, 36}, {40, 3}, {4, 27}, {19, 23}, {47, 12}, {28, 18}, {17, 41}, {10, 18}, {8, 10},
    {16, 36}, {30, 24}, {11, 41}, {41, 14}, {5, 18}, {10, 41}, {27, 27}, {16, 27}, {49, 14}, {39, 3}, {18, 47}, {44, 7}, {43, 43},
    {24, 20}, {50, 48}, {35, 22}, {13, 47}, {15, 29}, {35, 14}, {18, 38}, {12, 35}, {2, 2}, {2, 90}, {70, 3}, {3, 300}, {50, 50}};

// 420 grids of 2..8 cells a side: x <- (1103515245 x + 12345) mod 2^31 from 12345, side = 2 + (x >> 16) mod 7, height then width
static std::vector<std::pair<int, int>> many_small_grids() {
  std::vector<std::pair<int, int>> s(420);
  uint32_t x = 12345;
  auto side = [&x]() { x = (x * 1103515245u + 12345u) & 0x7fffffffu; return 2 + (int)((x >> 16) % 7); };
  for (auto &g : s) { g.first = side(); g.second = side(); }
  return s;
}

static std::vector<Case> cases() {
  std::vector<Case> c;
  c.push_back(make_case("one_256", {{256, 256}}, 8, 256, 1));
  c.push_back(make_case("headline_128x256", std::vector<std::pair<int, int>>(128, {256, 256}), 8, 256, 1));
  c.push_back(make_case("one_2x2", {{2, 2}}, 8, 256, 1));
  c.push_back(make_case("three_181x199", std::vector<std::pair<int, int>>(3, {181, 199}), 8, 256, 1));
  c.push_back(make_case("two_64_two_resolutions", {{64, 64}, {64, 64}}, 8, 256, 1));
  c.back().res = {0.5, 0.5, 1.0, 1.0};
  c.push_back(make_case("128x64_64cus", std::vector<std::pair<int, int>>(128, {64, 64}), 8, 64, 1));
  c.push_back(make_case("32x64_64cus", std::vector<std::pair<int, int>>(32, {64, 64}), 8, 64, 1));
  c.push_back(make_case("vr65_k8", kVrShapes, 8, 256, 1, 0.7, 0.9));
  c.push_back(make_case("vr65_k16", kVrShapes, 16, 256, 1, 0.7, 0.9));
  c.push_back(make_case("vr65_k8_no_atlas", kVrShapes, 8, 256, 0, 0.7, 0.9));
  c.push_back(make_case("vr65_k16_no_atlas", kVrShapes, 16, 256, 0, 0.7, 0.9));
  c.push_back(make_case("many420_k8", many_small_grids(), 8, 256, 1));
  c.push_back(make_case("many420_k16", many_small_grids(), 16, 256, 1));
  c.push_back(make_case("rejected_canvas", {{40, 48}, {33, 64}}, 8, 256, 1));
  c.push_back(make_case("single_candidate", {{3, 300}, {2, 2}}, 8, 256, 1));
  c.push_back(make_case("error_1x5", {{1, 5}}, 8, 256, 1));
  c.push_back(make_case("error_2pow30", std::vector<std::pair<int, int>>(4, {16384, 16384}), 8, 256, 1));
  return c;
}
// ---- end of cases ---------------------------------------------------------------------------------------------------------------

static uint64_t fnv1a(const void *p, size_t bytes) {
  uint64_t h = 0xcbf29ce484222325ull;
  const unsigned char *b = (const unsigned char *)p;
  for (size_t i = 0; i < bytes; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
  return h;
}

// {tile, r0, c0} blocks of bh x 16 cells: aligned, inside their tile, distinct, and their cells add up to the tile's
static bool blocks_cover(const bgnn::GraphPlan &p, const std::vector<BgnnWorkItem> &items, int bh) {
  std::vector<int64_t> area(p.h_tiles.size(), 0);
  std::set<std::pair<int, std::pair<int, int>>> seen;
  for (const auto &it : items) {
    if (it.tile < 0 || it.tile >= (int)p.h_tiles.size()) return false;
    const BgnnTileMeta &m = p.h_tiles[it.tile];
    const int r0 = it.r0, c0 = it.nr;
    if (r0 < 0 || c0 < 0 || r0 % bh || c0 % 16 || r0 >= m.h || c0 >= m.w) return false;
    if (!seen.insert({it.tile, {r0, c0}}).second) return false;
    area[it.tile] += (int64_t)std::min(bh, m.h - r0) * std::min(16, m.w - c0);
  }
  for (size_t t = 0; t < area.size(); ++t)
    if (area[t] != (int64_t)p.h_tiles[t].h * p.h_tiles[t].w) return false;
  return true;
}

static std::string properties(const Case &c, const bgnn::GraphPlan &p) {
  const int n = (int)p.h_tiles.size();
  // row bands: in order per tile, each starting where the last one ended, ending at the tile's height
  std::vector<int> next(n, 0);
  int64_t cells = 0;
  for (const auto &it : p.items) {
    if (it.tile < 0 || it.tile >= n || it.r0 != next[it.tile] || it.nr < 1) return "row bands";
    next[it.tile] += it.nr;
  }
  for (int t = 0; t < n; ++t) {
    if (next[t] != p.h_tiles[t].h) return "row bands";
    if (p.h_tiles[t].cell_off != cells) return "cell offsets";
    cells += (int64_t)p.h_tiles[t].h * p.h_tiles[t].w;
  }
  if (cells != p.cells) return "cell count";
  if (p.uniform) {
    if (p.bh2 != (p.uni_h + 15) / 16 || p.bw2 != (p.uni_w + 15) / 16 || p.bh3 != (p.uni_h + 7) / 8 || p.bw3 != p.bw2) return "uniform blocks";
    if (p.n_blocks2 != n * p.bh2 * p.bw2 || p.n_blocks3 != n * p.bh3 * p.bw3) return "uniform block counts";
    if (!p.items2.empty() || !p.items3.empty() || !p.block.empty() || p.atlas_h) return "uniform batch with ragged tables";
    return "ok";
  }
  if (!blocks_cover(p, p.items2, 16) || p.n_blocks2 != (int)p.items2.size()) return "items2";
  if (!blocks_cover(p, p.items3, 8) || p.n_blocks3 != (int)p.items3.size()) return "items3";
  // the block: 256-byte aligned tables in ascending order, no overlap, the last one ends the block
  std::vector<std::pair<size_t, size_t>> seg = {{p.o_tiles, sizeof(BgnnTileMeta) * n}, {p.o_items, sizeof(BgnnWorkItem) * p.items.size()},
                                                {p.o_items2, sizeof(BgnnWorkItem) * p.items2.size()}};
  if (p.atlas_h) { seg.push_back({p.o_atile, sizeof(BgnnTileMeta)}); seg.push_back({p.o_apos, sizeof(int32_t) * 2 * n}); }
  else seg.push_back({p.o_items3, sizeof(BgnnWorkItem) * p.items3.size()});
  size_t end = 0;
  for (auto &s : seg) {
    if (s.first % 256 || s.first < end) return "block offsets";
    end = s.first + s.second;
  }
  if (end != p.block.size()) return "block size";
  if (!p.atlas_h) return "ok";
  // the canvas: whole blocks, every grid inside, any two grids at least the gutter apart along one axis
  const int G = c.K == 16 ? 2 : 1;
  if (p.atlas_w % 16 || p.atlas_h % 8 || p.atlas_meta.h != p.atlas_h || p.atlas_meta.w != p.atlas_w) return "canvas size";
  if ((int)p.atlas_pos.size() != 2 * n) return "canvas positions";
  for (int a = 0; a < n; ++a) {
    const int ya = p.atlas_pos[2 * a], xa = p.atlas_pos[2 * a + 1], ha = p.h_tiles[a].h, wa = p.h_tiles[a].w;
    if (ya < 0 || xa < 0 || ya + ha > p.atlas_h || xa + wa > p.atlas_w) return "grid outside the canvas";
    for (int b = a + 1; b < n; ++b) {
      const int yb = p.atlas_pos[2 * b], xb = p.atlas_pos[2 * b + 1], hb = p.h_tiles[b].h, wb = p.h_tiles[b].w;
      const bool apart = ya + ha + G <= yb || yb + hb + G <= ya || xa + wa + G <= xb || xb + wb + G <= xa;
      if (!apart) return "grids closer than the gutter";
    }
  }
  return "ok";
}

int main() {
  const std::vector<Case> cs = cases();
  printf("{\n");
  for (size_t i = 0; i < cs.size(); ++i) {
    const Case &c = cs[i];
    const int n = (int)c.hw.size() / 2;
    const bgnn::GraphPlan p = bgnn::plan_graph(n, c.hw.data(), c.res.data(), c.K, c.cus, c.atlas);
    printf("\"%s\": {\"error\": %d, \"message\": \"%s\"", c.name.c_str(), p.error, p.message.c_str());
    if (p.error == BGNN_OK) {
      printf(", \"cells\": %lld, \"n_items\": %zu, \"uniform\": %d, \"uni\": [%d, %d], \"blocks2\": [%d, %d, %d], "
             "\"blocks3\": [%d, %d, %d], \"max\": [%d, %d], \"atlas\": [%d, %d], \"cacheable\": %d",
             (long long)p.cells, p.items.size(), p.uniform ? 1 : 0, p.uni_h, p.uni_w, p.bh2, p.bw2, p.n_blocks2, p.bh3,
             p.bw3, p.n_blocks3, p.max_h, p.max_w, p.atlas_w, p.atlas_h, p.cacheable ? 1 : 0);
      if (p.cacheable) printf(", \"key\": [%d, %d, %d, %d, %.17g, %.17g]", n, p.uni_h, p.uni_w, p.item_cells, p.rx, p.ry);
      if (p.uniform)
        printf(", \"tiles_hash\": \"%016llx\", \"items_hash\": \"%016llx\"",
               (unsigned long long)fnv1a(p.h_tiles.data(), sizeof(BgnnTileMeta) * n),
               (unsigned long long)fnv1a(p.items.data(), sizeof(BgnnWorkItem) * p.items.size()));
      else
        printf(", \"offsets\": [%zu, %zu, %zu, %zu, %zu, %zu], \"block_bytes\": %zu, \"block_alloc\": %zu, \"block_hash\": \"%016llx\"",
               p.o_tiles, p.o_items, p.o_items2, p.o_items3, p.o_atile, p.o_apos, p.block.size(), (p.block.size() + 255) & ~(size_t)255,
               (unsigned long long)fnv1a(p.block.data(), p.block.size()));
      printf(", \"props\": \"%s\"", properties(c, p).c_str());
    }
    printf("}%s\n", i + 1 < cs.size() ? "," : "");
  }
  printf("}\n");
  return 0;
}
