// Slope-based feature labels (include/bgnn_slope.h): create_feature_mask_from_slope and the slope half of add_feature_labels of the
// reference's scripts/prepare_feature_labels.py, on a depth plane that stays in HBM.  Four launches on the context's stream; every
// grid is a function of rows and cols.  The scheme is that of review_regions.hip with the size as the only aggregate.
//
//   sl_local     a 16 x 64 tile of depths in LDS with a one-cell halo: numpy.gradient's differences (one-sided in the plane's first
//                and last row / column, central inside), s = gx * gx + gy * gy and steep = s >= cut.  Every steep cell unites with
//                its left and upper neighbour inside the tile.  Writes every cell's parent (the global index of its tile-local root,
//                -1 off the mask) and size (0 but at tile-local roots)
//   sl_merge     every steep cell in the first row / column of a tile unites with its neighbour across the border
//   sl_flatten   every tile-local root that is not a global root points at its root and adds its size to the root's: one integer
//                atomicAdd per tile-local component; the components of up to 64 tiles that hang under one root are summed in a wave
//   sl_emit      per cell: the labels and the filtered mask from the size at the cell's root (at most two hops after sl_flatten);
//                the six counts per workgroup, then one 64-bit integer atomicAdd per count and workgroup
//
// Union-find, the invariant parent[i] <= i and the termination argument: union_find.h.  No thread waits for another: no spin-wait,
// no grid-wide barrier, no persistent kernel, no float atomics.
//
// Compiled with -ffp-contract=off: s = gx * gx + gy * gy has to be numpy's three float32 operations, two products and a sum, bit
// for bit; a fused multiply-add would round once less.  (x * 0.5f is x / 2.0f in every case, subnormal results included.)
#include "bgnn_internal.h"
#include "plane_util.h"
#include "union_find.h"
#include "../../include/bgnn_slope.h"

namespace bgnn {
namespace {

constexpr int SL_THREADS = BLOCK_THREADS;
constexpr int SL_ITEMS = 4;                           // cells per thread and step of sl_emit (each load coalesced)
constexpr int SL_CHUNK = SL_THREADS * SL_ITEMS;
constexpr int SL_MAX_GRID = 2048;                     // 256 CUs x 8 workgroups
constexpr int TILE_R = 16, TILE_C = 64;               // tile of sl_local: 1024 cells
constexpr int HALO_R = TILE_R + 2, HALO_C = TILE_C + 2;

struct TileGrid {
  int32_t rows, cols, tiles_r, tiles_c;
};

__global__ __launch_bounds__(SL_THREADS) void sl_local(const float *__restrict__ depth, float cut, TileGrid tg,
                                                       int32_t *__restrict__ parent, int32_t *__restrict__ size) {
  constexpr int CELLS = TILE_R * TILE_C, PER = CELLS / SL_THREADS;
  __shared__ float ld[HALO_R * HALO_C];
  __shared__ int32_t lp[CELLS], lsize[CELLS];
  const int t = threadIdx.x;
  const int64_t tiles = (int64_t)tg.tiles_r * tg.tiles_c;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int r0 = (int)(tile / tg.tiles_c) * TILE_R, c0 = (int)(tile % tg.tiles_c) * TILE_C;
    __syncthreads();                                            // (the previous tile is written out)
    // the tile and its halo; a cell outside the plane is never read back: at the plane's border the difference is one-sided
    for (int h = t; h < HALO_R * HALO_C; h += SL_THREADS) {
      const int gr = r0 - 1 + h / HALO_C, gc = c0 - 1 + h % HALO_C;
      const bool in = gr >= 0 && gr < tg.rows && gc >= 0 && gc < tg.cols;
      ld[h] = in ? depth[(int64_t)gr * tg.cols + gc] : 0.0f;
    }
    __syncthreads();
    bool steep[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int l = k * SL_THREADS + t, lr = l / TILE_C, lc = l % TILE_C, gr = r0 + lr, gc = c0 + lc;
      steep[k] = false;
      if (gr < tg.rows && gc < tg.cols) {
        const int at = (lr + 1) * HALO_C + lc + 1;
        const float here = ld[at];
        float gy, gx;
        if (gr == 0) gy = ld[at + HALO_C] - here;
        else if (gr == tg.rows - 1) gy = here - ld[at - HALO_C];
        else gy = (ld[at + HALO_C] - ld[at - HALO_C]) * 0.5f;
        if (gc == 0) gx = ld[at + 1] - here;
        else if (gc == tg.cols - 1) gx = here - ld[at - 1];
        else gx = (ld[at + 1] - ld[at - 1]) * 0.5f;
        const float s = gx * gx + gy * gy;
        steep[k] = s >= cut;                                    // (false for a NaN on either side)
      }
      lp[l] = steep[k] ? l : -1;
      lsize[l] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int l = k * SL_THREADS + t;
      if (!steep[k]) continue;
      if (l % TILE_C > 0 && load_parent<false>(lp, l - 1) >= 0) unite<false>(lp, l, l - 1);
      if (l >= TILE_C && load_parent<false>(lp, l - TILE_C) >= 0) unite<false>(lp, l, l - TILE_C);
    }
    __syncthreads();
    // A thread's cells lie in one column, SL_THREADS / TILE_C rows apart: those that share the first one's root go to LDS as one
    // add, the others cell by cell.
    int32_t root[PER];
    int32_t r_first = -1, n_first = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int l = k * SL_THREADS + t;
      root[k] = steep[k] ? find_root<false>(lp, l) : -1;
      if (!steep[k]) continue;
      if (r_first < 0) r_first = root[k];
      if (root[k] == r_first) n_first += 1;
      else atomicAdd(&lsize[root[k]], 1);
    }
    if (r_first >= 0) atomicAdd(&lsize[r_first], n_first);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int l = k * SL_THREADS + t, gr = r0 + l / TILE_C, gc = c0 + l % TILE_C;
      if (gr >= tg.rows || gc >= tg.cols) continue;
      const int64_t i = (int64_t)gr * tg.cols + gc;
      const int rl = root[k];
      parent[i] = steep[k] ? (int32_t)((int64_t)(r0 + rl / TILE_C) * tg.cols + c0 + rl % TILE_C) : -1;
      size[i] = steep[k] && rl == l ? lsize[l] : 0;
    }
  }
}

// The cells that have a neighbour across a tile border: (tiles_r - 1) * cols in the first rows of the lower tiles (upper
// neighbour), then (tiles_c - 1) * rows in the first columns of the right-hand tiles (left neighbour).
__global__ __launch_bounds__(SL_THREADS) void sl_merge(TileGrid tg, int32_t *parent) {
  const int64_t nh = (int64_t)(tg.tiles_r - 1) * tg.cols, total = nh + (int64_t)(tg.tiles_c - 1) * tg.rows;
  for (int64_t j = (int64_t)blockIdx.x * SL_THREADS + threadIdx.x; j < total; j += (int64_t)gridDim.x * SL_THREADS) {
    int64_t i, other;
    if (j < nh) {
      const int64_t r = (j / tg.cols + 1) * TILE_R, c = j % tg.cols;
      i = r * tg.cols + c;
      other = i - tg.cols;
    } else {
      const int64_t k = j - nh, c = (k / tg.rows + 1) * TILE_C, r = k % tg.rows;
      i = r * tg.cols + c;
      other = i - 1;
    }
    if (load_parent<true>(parent, (int32_t)i) >= 0 && load_parent<true>(parent, (int32_t)other) >= 0) unite<true>(parent, (int32_t)i, (int32_t)other);
  }
}

// Roots are stable here: the merges ended with the previous kernel.  Only global roots' sizes change, only others' are read.  A
// workgroup takes 4096 consecutive cells at a time -- in a tile's first row that is the first cells of 64 tiles -- and lists the
// tile-local roots among them in LDS (in any order: every later step is an integer add).  Then a wave takes 64 of the list: the
// pieces that hang under one root are summed in the wave (shuffles) and one lane adds them to that root.  Where a cluster covers many
// tiles this is one global atomic per 64 tiles, not 64 on one address.  After FL_GROUPS roots the lanes still left add their own.
constexpr int FL_ITEMS = 16, FL_CHUNK = SL_THREADS * FL_ITEMS, FL_GROUPS = 4;

__global__ __launch_bounds__(SL_THREADS) void sl_flatten(int64_t cells, int32_t *parent, int32_t *size) {
  __shared__ int32_t cand[FL_CHUNK];
  __shared__ int32_t n_cand;
  const int t = threadIdx.x, lane = t & 63;
  const int64_t chunks = (cells + FL_CHUNK - 1) / FL_CHUNK;
  for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    __syncthreads();                                            // (the previous list is consumed)
    if (t == 0) n_cand = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FL_ITEMS; ++k) {
      const int64_t i = chunk * FL_CHUNK + k * SL_THREADS + t;
      // a tile-local root: its own parent (still: nothing has re-pointed it) with a size; global roots are skipped below
      if (i < cells && __hip_atomic_load(size + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0) cand[atomicAdd(&n_cand, 1)] = (int32_t)i;
    }
    __syncthreads();
    const int n = n_cand;
    for (int j0 = 0; j0 < n; j0 += SL_THREADS) {                // (the same trips for every thread of the workgroup)
      const int j = j0 + t;
      int32_t root = -1, piece = 0;
      bool todo = false;
      if (j < n) {
        const int32_t i = cand[j];
        root = find_root<true>(parent, i);
        todo = root != i;
        if (todo) {
          __hip_atomic_store(parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          piece = size[i];                                      // (not a global root: nobody adds to it)
        }
      }
      for (int group = 0;; ++group) {                           // (the same trips for every lane of the wave)
        const unsigned long long left = __ballot(todo);
        if (left == 0ull) break;
        const bool own = group == FL_GROUPS;                    // every lane for itself
        const int leader = __ffsll((long long)left) - 1;
        const int32_t r = own ? root : __shfl(root, leader);
        const bool mine = todo && root == r;
        int32_t g_size = mine ? piece : 0;
        if (!own) {
#pragma unroll
          for (int w = 32; w > 0; w >>= 1) g_size += __shfl_xor(g_size, w);
        }
        if (own ? todo : lane == leader) atomicAdd(size + r, g_size);
        if (own) break;
        todo = todo && !mine;
      }
    }
  }
}

struct EmitArgs {
  const float *depth;
  const int32_t *base;           // overlay mode (else nullptr)
  const int32_t *parent, *size;
  int32_t *labels;
  uint8_t *mask;                 // or nullptr
  unsigned long long *stats;
  int64_t cells, min_size;
  float nodata;
};

__global__ __launch_bounds__(SL_THREADS) void sl_emit(EmitArgs a) {
  __shared__ int64_t red[SL_THREADS];
  const int t = threadIdx.x;
  const bool overlay = a.base != nullptr;                       // (uniform)
  int64_t n[BGNN_SL_STATS] = {0, 0, 0, 0, 0, 0};
  for (int64_t base = (int64_t)blockIdx.x * SL_CHUNK; base < a.cells; base += (int64_t)gridDim.x * SL_CHUNK) {
#pragma unroll
    for (int k = 0; k < SL_ITEMS; ++k) {
      const int64_t i = base + k * SL_THREADS + t;
      if (i >= a.cells) continue;
      const int32_t p = a.parent[i];
      bool keep = false;
      if (p >= 0) {
        const int32_t root = find_root<true>(a.parent, p);      // (stable: at most two hops)
        const int64_t s = a.size[root];
        keep = s >= a.min_size;
        n[1] += 1;
        if ((int64_t)p == i) { n[2] += 1; if (keep) n[3] += 1; }
        if (keep) n[4] += 1;
      }
      int32_t label;
      bool valid, paint;
      if (overlay) {
        const int32_t b = a.base[i];
        valid = b >= 0;
        paint = keep && b == 0;
        label = paint ? 1 : b;
      } else {
        const float d = a.depth[i];
        valid = d != a.nodata && finite_bits(d);
        paint = keep && valid;
        label = valid ? (paint ? 1 : 0) : -1;
      }
      n[0] += valid;
      n[5] += paint;
      a.labels[i] = label;
      if (a.mask != nullptr) a.mask[i] = keep ? 1 : 0;
    }
  }
#pragma unroll
  for (int k = 0; k < BGNN_SL_STATS; ++k) {
    const int64_t v = block_reduce(n[k], red, SumOp());
    if (t == 0 && v != 0) atomicAdd(a.stats + k, (unsigned long long)v);
  }
}

inline bool within_limit(int64_t rows, int64_t cols) { return rows >= 2 && cols >= 2 && rows <= (int64_t)BGNN_SL_MAX_CELLS / cols; }

}  // namespace
}  // namespace bgnn

using namespace bgnn;

static_assert(BGNN_SL_STATS * 8 == BGNN_SL_STATS_BYTES, "the statistics block as the header states it");

extern "C" size_t bgnn_slope_features_workspace_bytes(int64_t rows, int64_t cols) {
  if (!within_limit(rows, cols)) return 0;
  return 2 * align256((size_t)rows * (size_t)cols * 4);
}

extern "C" int bgnn_slope_features(bgnn_ctx *ctx, const float *depth, const int32_t *base_labels, int64_t rows, int64_t cols,
                                   double nodata, float cut, int64_t min_cluster_size, void *workspace, size_t workspace_bytes,
                                   int32_t *labels, uint8_t *slope_mask, void *stats) {
  BGNN_REQUIRE(ctx && depth && workspace && labels && stats, "bgnn_slope_features: NULL argument");
  BGNN_REQUIRE(rows >= 2 && cols >= 2, "bgnn_slope_features: a grid of %lld x %lld (the gradient needs at least 2 cells along every axis)",
               (long long)rows, (long long)cols);
  if (!within_limit(rows, cols)) {
    set_error("bgnn_slope_features: %lld x %lld cells exceed the limit of %lld (int32 cluster labels)", (long long)rows, (long long)cols,
              (long long)BGNN_SL_MAX_CELLS);
    return BGNN_ERR_UNSUPPORTED;
  }
  const size_t need = bgnn_slope_features_workspace_bytes(rows, cols);
  BGNN_REQUIRE(workspace_bytes >= need, "bgnn_slope_features: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  BGNN_REQUIRE(((uintptr_t)workspace & 3) == 0, "bgnn_slope_features: the workspace is not 4-byte aligned");
  BGNN_REQUIRE(((uintptr_t)stats & 7) == 0, "bgnn_slope_features: the statistics block is not 8-byte aligned");
  BGNN_REQUIRE(((uintptr_t)depth & 3) == 0 && ((uintptr_t)base_labels & 3) == 0 && ((uintptr_t)labels & 3) == 0,
               "bgnn_slope_features: a plane is not 4-byte aligned");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const int64_t cells = rows * cols;
  char *w = static_cast<char *>(workspace);
  int32_t *parent = reinterpret_cast<int32_t *>(w);
  int32_t *size = reinterpret_cast<int32_t *>(w + align256((size_t)cells * 4));
  TileGrid tg;
  tg.rows = (int32_t)rows; tg.cols = (int32_t)cols;
  tg.tiles_r = (int32_t)((rows + TILE_R - 1) / TILE_R); tg.tiles_c = (int32_t)((cols + TILE_C - 1) / TILE_C);
  const int64_t tiles = (int64_t)tg.tiles_r * tg.tiles_c;
  const int64_t borders = (int64_t)(tg.tiles_r - 1) * cols + (int64_t)(tg.tiles_c - 1) * rows;
  const auto grid_of = [](int64_t work_items) { return capped_grid(work_items, SL_MAX_GRID); };
  const int g_tiles = grid_of(tiles), g_flatten = grid_of((cells + FL_CHUNK - 1) / FL_CHUNK);
  const int g_borders = grid_of((borders + SL_THREADS - 1) / SL_THREADS), g_emit = grid_of((cells + SL_CHUNK - 1) / SL_CHUNK);
  EmitArgs a;
  a.depth = depth; a.base = base_labels; a.parent = parent; a.size = size; a.labels = labels; a.mask = slope_mask;
  a.stats = static_cast<unsigned long long *>(stats);
  a.cells = cells; a.min_size = min_cluster_size; a.nodata = (float)nodata;
  const dim3 b(SL_THREADS);
  hipStream_t s = ctx->stream;

  BGNN_HIP_CHECK(hipMemsetAsync(stats, 0, BGNN_SL_STATS_BYTES, s));
  hipLaunchKernelGGL(sl_local, dim3(g_tiles), b, 0, s, depth, cut, tg, parent, size);
  hipLaunchKernelGGL(sl_merge, dim3(g_borders), b, 0, s, tg, parent);
  hipLaunchKernelGGL(sl_flatten, dim3(g_flatten), b, 0, s, cells, parent, size);
  hipLaunchKernelGGL(sl_emit, dim3(g_emit), b, 0, s, a);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
