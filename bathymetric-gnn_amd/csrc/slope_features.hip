// Slope-based feature labels (include/bgnn_slope.h): create_feature_mask_from_slope and the slope half of add_feature_labels of the
// reference's scripts/prepare_feature_labels.py, on a depth plane that stays in HBM.  Four launches on the context's stream; every
// grid is a function of rows and cols.
//
//   sl_local      a 16 x 64 tile of depths in LDS with a one-cell halo: numpy.gradient's differences (one-sided in the plane's
//                 first and last row / column, central inside), s = gx * gx + gy * gy and steep = s >= cut; then the tile-local
//                 labelling of the steep cells
//   label_merge, label_flatten<SizeOnly>   component_label.h: the unions across the tile borders; the sizes summed at the roots
//   sl_emit       per cell: the labels and the filtered mask from the size at the cell's root (at most two hops after the flatten);
//                 the six counts per workgroup, then one 64-bit integer atomicAdd per count and workgroup
//
// The labelling, its invariant parent[i] <= i and the termination argument: component_label.h.  No thread waits for another: no
// spin-wait, no grid-wide barrier, no persistent kernel, no float atomics.
//
// Compiled with -ffp-contract=off: s = gx * gx + gy * gy has to be numpy's three float32 operations, two products and a sum, bit
// for bit; a fused multiply-add would round once less.  (x * 0.5f is x / 2.0f in every case, subnormal results included.)
#include "bgnn_internal.h"
#include "component_label.h"
#include "../../include/bgnn_slope.h"

namespace bgnn {
namespace {

constexpr int SL_THREADS = BLOCK_THREADS;
constexpr int SL_ITEMS = 4;                           // cells per thread and step of sl_emit (each load coalesced)
constexpr int SL_CHUNK = SL_THREADS * SL_ITEMS;
constexpr int HALO_R = TILE_R + 2, HALO_C = TILE_C + 2;

__global__ __launch_bounds__(SL_THREADS) void sl_local(const float *__restrict__ depth, float cut, TileGrid tg,
                                                       int32_t *__restrict__ parent, int32_t *__restrict__ size) {
  __shared__ float ld[HALO_R * HALO_C];
  __shared__ int32_t lp[TILE_CELLS], lsize[TILE_CELLS];
  const int t = threadIdx.x;
  const int64_t tiles = tg.tiles();
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
    bool steep[TILE_PER];
#pragma unroll
    for (int k = 0; k < TILE_PER; ++k) {
      const int l = tile_cell(k), lr = l / TILE_C, lc = l % TILE_C, gr = r0 + lr, gc = c0 + lc;
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
    }
    int32_t root[TILE_PER];
    tile_label(steep, lp, lsize, root);
    tile_write(tg, r0, c0, steep, root, lsize, parent, size);
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
  const TileGrid tg(rows, cols);
  const int g_emit = capped_grid((cells + SL_CHUNK - 1) / SL_CHUNK, PLANE_MAX_GRID);
  EmitArgs a;
  a.depth = depth; a.base = base_labels; a.parent = parent; a.size = size; a.labels = labels; a.mask = slope_mask;
  a.stats = static_cast<unsigned long long *>(stats);
  a.cells = cells; a.min_size = min_cluster_size; a.nodata = (float)nodata;
  const dim3 b(SL_THREADS);
  hipStream_t s = ctx->stream;

  BGNN_HIP_CHECK(hipMemsetAsync(stats, 0, BGNN_SL_STATS_BYTES, s));
  hipLaunchKernelGGL(sl_local, dim3(tg.local_grid()), b, 0, s, depth, cut, tg, parent, size);
  launch_merge_flatten(s, tg, parent, SizeOnly{size});
  hipLaunchKernelGGL(sl_emit, dim3(g_emit), b, 0, s, a);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
