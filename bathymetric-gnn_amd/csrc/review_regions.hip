// Low-confidence regions for review (include/bgnn_review.h): scripts/export_for_review.py of the reference's training plan, on a
// confidence plane that stays in HBM.  Six launches on the context's stream; every grid is a function of rows and cols.
//
//   rv_local     a 16 x 64 tile in LDS: every uncertain cell unites with its left and upper neighbour inside the tile; per
//                tile-local root the cells, the fixed-point confidence sum and the rows / columns the component touches in the tile
//                (a 16-bit and a 64-bit set: integer LDS atomics).  Writes every cell's parent (the global index of its tile-local
//                root, -1 off the mask) and size (0 but at tile-local roots); sum and bounds only at tile-local roots
//   rv_merge     every uncertain cell in the first row / column of a tile unites with its neighbour across the border
//   rv_flatten   every tile-local root that is not a global root points at its root and adds its aggregate to the root's: integer
//                atomicAdd / atomicMin / atomicMax, at most one set per tile-local component, not per cell; the components of up to
//                64 tiles that hang under one root are combined in a wave first
//   rv_count     every workgroup owns a contiguous range of cells: uncertain cells, components, kept components and their cells
//   rv_scan      one workgroup: the exclusive scan of the kept counts in workgroup order (each workgroup's first record) and counts[]
//   rv_emit      the same ranges again, in order: a kept root's record goes to base + rank in the range; the mask of every cell from
//                the size at its root (at most two hops after rv_flatten)
//
// Union-find, the invariant parent[i] <= i and the termination argument: union_find.h.  A component's root is its smallest cell
// index, so "ascending by root" is the order scipy.ndimage.label numbers the components.  No thread waits for another: no spin-wait,
// no grid-wide barrier, no persistent kernel, no float atomics.
//
// Compiled with -ffp-contract=off: (double)c * 2^32 is exact either way, the flag keeps the file under the rule of its neighbours.
#include "bgnn_internal.h"
#include "plane_util.h"
#include "union_find.h"
#include "../../include/bgnn_review.h"

namespace bgnn {
namespace {

constexpr int RV_THREADS = BLOCK_THREADS;
constexpr int RV_ITEMS = 4;                           // cells per thread and step of a streaming pass (each load coalesced)
constexpr int RV_CHUNK = RV_THREADS * RV_ITEMS;
constexpr int RV_MAX_GRID = 2048;                     // 256 CUs x 8 workgroups
constexpr int RV_WAVES = RV_THREADS / 64;
constexpr int TILE_R = 16, TILE_C = 64;               // tile of rv_local: 1024 cells
constexpr int ROW_WORDS = 4;                          // a partial row of rv_count: int64 [BGNN_RV_COUNTS]

// workspace: the partial rows, the record bases, then the seven planes
constexpr size_t WS_ROWS = 0;
constexpr size_t WS_BASES = WS_ROWS + (size_t)RV_MAX_GRID * ROW_WORDS * 8;
constexpr size_t WS_PLANES = WS_BASES + (size_t)RV_MAX_GRID * 8;
static_assert(WS_PLANES == BGNN_RV_FIXED_BYTES && WS_PLANES % 256 == 0, "the fixed part as the header states it");
static_assert(sizeof(bgnn_review_record) == BGNN_RV_RECORD_BYTES, "record layout");
static_assert(ROW_WORDS == BGNN_RV_COUNTS, "one partial per count");

struct TileGrid {
  int32_t rows, cols, tiles_r, tiles_c;
};

// The aggregates of the components, indexed by cell; valid at tile-local roots after rv_local, complete at global roots after rv_flatten
struct Aggregates {
  int32_t *size;
  unsigned long long *sum;
  int32_t *min_row, *max_row, *min_col, *max_col;
};

__device__ __forceinline__ unsigned long long fixed_point(float c) {              // c in [0, 1]: at most 2^32
  return (unsigned long long)__double2ll_rn((double)c * 4294967296.0);
}

__global__ __launch_bounds__(RV_THREADS) void rv_local(const float *__restrict__ conf, float low, float high, TileGrid tg,
                                                       int32_t *__restrict__ parent, Aggregates ag) {
  constexpr int CELLS = TILE_R * TILE_C, PER = CELLS / RV_THREADS;
  __shared__ int32_t lp[CELLS], lsize[CELLS];
  __shared__ uint32_t lrows[CELLS];
  __shared__ unsigned long long lsum[CELLS], lcols[CELLS];
  const int t = threadIdx.x;
  const int64_t tiles = (int64_t)tg.tiles_r * tg.tiles_c;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int r0 = (int)(tile / tg.tiles_c) * TILE_R, c0 = (int)(tile % tg.tiles_c) * TILE_C;
    __syncthreads();                                            // (the previous tile is written out)
    bool unc[PER];
    unsigned long long fx[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int l = k * RV_THREADS + t, gr = r0 + l / TILE_C, gc = c0 + l % TILE_C;
      const bool in = gr < tg.rows && gc < tg.cols;
      const float c = in ? conf[(int64_t)gr * tg.cols + gc] : __uint_as_float(0x7FC00000u);
      unc[k] = c >= low && c <= high && finite_bits(c);
      fx[k] = unc[k] ? fixed_point(c) : 0ull;
      lp[l] = unc[k] ? l : -1;
      lsize[l] = 0; lrows[l] = 0u; lsum[l] = 0ull; lcols[l] = 0ull;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int l = k * RV_THREADS + t;
      if (!unc[k]) continue;
      if (l % TILE_C > 0 && load_parent<false>(lp, l - 1) >= 0) unite<false>(lp, l, l - 1);
      if (l >= TILE_C && load_parent<false>(lp, l - TILE_C) >= 0) unite<false>(lp, l, l - TILE_C);
    }
    __syncthreads();
    // A thread's cells lie in one column, RV_THREADS / TILE_C rows apart: those that share the first one's root go to LDS as one
    // set of atomics, the others cell by cell.
    int32_t root[PER];
    int32_t r_first = -1, n_first = 0;
    uint32_t rows_first = 0u;
    unsigned long long sum_first = 0ull;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int l = k * RV_THREADS + t;
      root[k] = unc[k] ? find_root<false>(lp, l) : -1;
      if (!unc[k]) continue;
      if (r_first < 0) r_first = root[k];
      if (root[k] == r_first) {
        n_first += 1; rows_first |= 1u << (l / TILE_C); sum_first += fx[k];
      } else {
        atomicAdd(&lsize[root[k]], 1);
        atomicOr(&lrows[root[k]], 1u << (l / TILE_C));
        atomicAdd(&lsum[root[k]], fx[k]);
        atomicOr(&lcols[root[k]], 1ull << (l % TILE_C));
      }
    }
    if (r_first >= 0) {
      atomicAdd(&lsize[r_first], n_first);
      atomicOr(&lrows[r_first], rows_first);
      atomicAdd(&lsum[r_first], sum_first);
      atomicOr(&lcols[r_first], 1ull << (t % TILE_C));
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int l = k * RV_THREADS + t, gr = r0 + l / TILE_C, gc = c0 + l % TILE_C;
      if (gr >= tg.rows || gc >= tg.cols) continue;
      const int64_t i = (int64_t)gr * tg.cols + gc;
      const int rl = root[k];
      parent[i] = unc[k] ? (int32_t)((int64_t)(r0 + rl / TILE_C) * tg.cols + c0 + rl % TILE_C) : -1;
      const bool is_root = unc[k] && rl == l;
      ag.size[i] = is_root ? lsize[l] : 0;
      if (is_root) {
        const uint32_t rs = lrows[l];
        const unsigned long long cs = lcols[l];
        ag.sum[i] = lsum[l];
        ag.min_row[i] = r0 + (__ffs((int)rs) - 1);
        ag.max_row[i] = r0 + 31 - __clz((int)rs);
        ag.min_col[i] = c0 + (__ffsll((long long)cs) - 1);
        ag.max_col[i] = c0 + 63 - __clzll((long long)cs);
      }
    }
  }
}

// The cells that have a neighbour across a tile border: (tiles_r - 1) * cols in the first rows of the lower tiles (upper
// neighbour), then (tiles_c - 1) * rows in the first columns of the right-hand tiles (left neighbour).
__global__ __launch_bounds__(RV_THREADS) void rv_merge(TileGrid tg, int32_t *parent) {
  const int64_t nh = (int64_t)(tg.tiles_r - 1) * tg.cols, total = nh + (int64_t)(tg.tiles_c - 1) * tg.rows;
  for (int64_t j = (int64_t)blockIdx.x * RV_THREADS + threadIdx.x; j < total; j += (int64_t)gridDim.x * RV_THREADS) {
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

// Roots are stable here: the merges ended with the previous kernel.  Only global roots' aggregates change, only others' are read.
// A workgroup takes 4096 consecutive cells at a time -- in a tile's first row that is the first cells of 64 tiles -- and lists the
// tile-local roots among them in LDS (in any order: every later step is an integer add, minimum or maximum).  Then a wave takes 64
// of the list: the pieces that hang under one root are combined in the wave (shuffles) and one lane adds them to that root.  Where a
// region covers many tiles this is one set of global atomics per 64 tiles, not 64 on one address.  After FL_GROUPS roots the lanes
// still left add their own piece.
constexpr int FL_ITEMS = 16, FL_CHUNK = RV_THREADS * FL_ITEMS, FL_GROUPS = 4;

__global__ __launch_bounds__(RV_THREADS) void rv_flatten(int64_t cells, int32_t *parent, Aggregates ag) {
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
      const int64_t i = chunk * FL_CHUNK + k * RV_THREADS + t;
      if (i < cells && ag.size[i] > 0) cand[atomicAdd(&n_cand, 1)] = (int32_t)i;      // (> 0: a tile-local root)
    }
    __syncthreads();
    const int n = n_cand;
    for (int j0 = 0; j0 < n; j0 += RV_THREADS) {                // (the same trips for every thread of the workgroup)
      const int j = j0 + t;
      int32_t root = -1, size = 0, r_lo = INT32_MAX, r_hi = INT32_MIN, c_lo = INT32_MAX, c_hi = INT32_MIN;
      unsigned long long sum = 0ull;
      bool todo = false;
      if (j < n) {
        const int32_t i = cand[j];
        root = find_root<true>(parent, i);
        todo = root != i;
        if (todo) {
          __hip_atomic_store(parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          size = ag.size[i]; sum = ag.sum[i];
          r_lo = ag.min_row[i]; r_hi = ag.max_row[i]; c_lo = ag.min_col[i]; c_hi = ag.max_col[i];
        }
      }
      for (int group = 0;; ++group) {                           // (the same trips for every lane of the wave)
        const unsigned long long left = __ballot(todo);
        if (left == 0ull) break;
        const bool own = group == FL_GROUPS;                    // every lane for itself
        const int leader = __ffsll((long long)left) - 1;
        const int32_t r = own ? root : __shfl(root, leader);
        const bool mine = todo && root == r;
        int32_t g_size = mine ? size : 0, g_r_lo = mine ? r_lo : INT32_MAX, g_r_hi = mine ? r_hi : INT32_MIN;
        int32_t g_c_lo = mine ? c_lo : INT32_MAX, g_c_hi = mine ? c_hi : INT32_MIN;
        unsigned long long g_sum = mine ? sum : 0ull;
        if (!own) {
#pragma unroll
          for (int w = 32; w > 0; w >>= 1) {
            g_size += __shfl_xor(g_size, w);
            g_sum += __shfl_xor(g_sum, w);
            g_r_lo = min(g_r_lo, __shfl_xor(g_r_lo, w)); g_r_hi = max(g_r_hi, __shfl_xor(g_r_hi, w));
            g_c_lo = min(g_c_lo, __shfl_xor(g_c_lo, w)); g_c_hi = max(g_c_hi, __shfl_xor(g_c_hi, w));
          }
        }
        if (own ? todo : lane == leader) {
          atomicAdd(ag.size + r, g_size);
          atomicAdd(ag.sum + r, g_sum);
          atomicMin(ag.min_row + r, g_r_lo);
          atomicMax(ag.max_row + r, g_r_hi);
          atomicMin(ag.min_col + r, g_c_lo);
          atomicMax(ag.max_col + r, g_c_hi);
        }
        if (own) break;
        todo = todo && !mine;
      }
    }
  }
}

// Workgroup b owns the cells [b * chunk, min((b + 1) * chunk, cells)); chunk is a multiple of RV_CHUNK.
__global__ __launch_bounds__(RV_THREADS) void rv_count(int64_t cells, int64_t chunk, int64_t min_size, const int32_t *__restrict__ parent,
                                                       const int32_t *__restrict__ size, int64_t *__restrict__ rows) {
  __shared__ int64_t red[RV_THREADS];
  const int64_t begin = (int64_t)blockIdx.x * chunk, end = begin + chunk < cells ? begin + chunk : cells;
  int64_t n[ROW_WORDS] = {0, 0, 0, 0};
  for (int64_t base = begin; base < end; base += RV_CHUNK) {
#pragma unroll
    for (int k = 0; k < RV_ITEMS; ++k) {
      const int64_t i = base + k * RV_THREADS + threadIdx.x;
      const int32_t p = i < end ? parent[i] : -1;
      n[0] += p >= 0;
      if (p >= 0 && (int64_t)p == i) {
        const int64_t s = size[i];
        n[1] += 1;
        if (s >= min_size) { n[2] += 1; n[3] += s; }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < ROW_WORDS; ++k) {
    const int64_t v = block_reduce(n[k], red, SumOp());
    if (threadIdx.x == 0) rows[(int64_t)blockIdx.x * ROW_WORDS + k] = v;
  }
}

// One workgroup: bases[b] = kept components of the workgroups before b; counts[] = the column sums of the n partial rows.
__global__ __launch_bounds__(RV_THREADS) void rv_scan(const int64_t *__restrict__ rows, int n, int64_t *__restrict__ bases,
                                                      int64_t *__restrict__ counts) {
  constexpr int PER = RV_MAX_GRID / RV_THREADS;
  __shared__ int64_t red[RV_THREADS], before[RV_THREADS];
  const int t = threadIdx.x;
  int64_t tot[ROW_WORDS] = {0, 0, 0, 0};
  for (int j = 0; j < PER; ++j) {
    const int b = t * PER + j;
    if (b >= n) break;
#pragma unroll
    for (int k = 0; k < ROW_WORDS; ++k) tot[k] += rows[(int64_t)b * ROW_WORDS + k];
  }
  before[t] = tot[2];
  __syncthreads();
  if (t == 0) {
    int64_t run = 0;
    for (int j = 0; j < RV_THREADS; ++j) { const int64_t v = before[j]; before[j] = run; run += v; }
  }
  __syncthreads();
  int64_t run = before[t];
  for (int j = 0; j < PER; ++j) {
    const int b = t * PER + j;
    if (b >= n) break;
    bases[b] = run;
    run += rows[(int64_t)b * ROW_WORDS + 2];
  }
#pragma unroll
  for (int k = 0; k < ROW_WORDS; ++k) {
    const int64_t v = block_reduce(tot[k], red, SumOp());
    if (t == 0) counts[k] = v;
  }
}

__global__ __launch_bounds__(RV_THREADS) void rv_emit(int64_t cells, int64_t chunk, int64_t min_size, const int32_t *__restrict__ parent,
                                                      Aggregates ag, const int64_t *__restrict__ bases,
                                                      bgnn_review_record *__restrict__ records, int64_t capacity,
                                                      float *__restrict__ mask) {
  __shared__ int32_t wave_kept[RV_ITEMS][RV_WAVES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t begin = (int64_t)blockIdx.x * chunk, end = begin + chunk < cells ? begin + chunk : cells;
  int64_t out = bases[blockIdx.x];                              // the next record of this range
  for (int64_t base = begin; base < end; base += RV_CHUNK) {
    bool flag[RV_ITEMS];
    int any = 0;
#pragma unroll
    for (int k = 0; k < RV_ITEMS; ++k) {
      const int64_t i = base + k * RV_THREADS + t;
      const int32_t p = i < end ? parent[i] : -1;
      bool keep = false;
      flag[k] = false;
      if (p >= 0) {
        const int32_t root = find_root<true>(parent, p);        // (stable: at most two hops)
        keep = (int64_t)ag.size[root] >= min_size;
        flag[k] = keep && (int64_t)root == i;
      }
      if (mask != nullptr && i < end) mask[i] = keep ? 1.0f : 0.0f;
      any |= flag[k];
    }
    if (__syncthreads_count(any) == 0) continue;                // (the same for every thread; the usual case: roots are few)
    // cell order within the step: item k, then wave, then lane
    int rank[RV_ITEMS];
#pragma unroll
    for (int k = 0; k < RV_ITEMS; ++k) {
      const unsigned long long b = __ballot(flag[k]);
      rank[k] = __popcll(b & ((1ull << lane) - 1ull));
      if (lane == 0) wave_kept[k][wave] = __popcll(b);
    }
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int k = 0; k < RV_ITEMS; ++k) {
#pragma unroll
      for (int w = 0; w < RV_WAVES; ++w) {
        if (w == wave && flag[k]) {
          const int64_t i = base + k * RV_THREADS + t, slot = out + before + rank[k];
          if (slot < capacity) {
            bgnn_review_record r;
            r.first = i; r.size = ag.size[i];
            r.min_row = ag.min_row[i]; r.max_row = ag.max_row[i]; r.min_col = ag.min_col[i]; r.max_col = ag.max_col[i];
            r.conf_sum = ag.sum[i];
            records[slot] = r;
          }
        }
        before += wave_kept[k][w];
      }
    }
    out += before;
    __syncthreads();                                            // (wave_kept is read; the next step may write it)
  }
}

inline bool within_limit(int64_t rows, int64_t cols) { return rows >= 1 && cols >= 1 && rows <= (int64_t)BGNN_RV_MAX_CELLS / cols; }

}  // namespace
}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_review_workspace_bytes(int64_t rows, int64_t cols) {
  if (!within_limit(rows, cols)) return 0;
  const size_t cells = (size_t)rows * (size_t)cols;
  return WS_PLANES + 6 * align256(cells * 4) + align256(cells * 8);
}

extern "C" int bgnn_review_regions(bgnn_ctx *ctx, const float *confidence, int64_t rows, int64_t cols, float low, float high,
                                   int64_t min_region_size, void *workspace, size_t workspace_bytes, void *records, int64_t capacity,
                                   int64_t *counts, float *review_mask) {
  BGNN_REQUIRE(ctx && confidence && workspace && counts, "bgnn_review_regions: NULL argument");
  BGNN_REQUIRE(capacity >= 0, "bgnn_review_regions: a capacity of %lld records", (long long)capacity);
  BGNN_REQUIRE(records || capacity == 0, "bgnn_review_regions: NULL record table with a capacity of %lld", (long long)capacity);
  BGNN_REQUIRE(rows >= 1 && cols >= 1, "bgnn_review_regions: a grid of %lld x %lld", (long long)rows, (long long)cols);
  BGNN_REQUIRE(min_region_size >= 1, "bgnn_review_regions: min_region_size %lld", (long long)min_region_size);
  BGNN_REQUIRE(low == low && high == high && low >= 0.0f && high <= 1.0f && low <= high,
               "bgnn_review_regions: the bounds [%g, %g] are not finite, not ordered or outside [0, 1] (the fixed-point range)", (double)low,
               (double)high);
  if (!within_limit(rows, cols)) {
    set_error("bgnn_review_regions: %lld x %lld cells exceed the limit of %lld (int32 region labels)", (long long)rows, (long long)cols,
              (long long)BGNN_RV_MAX_CELLS);
    return BGNN_ERR_UNSUPPORTED;
  }
  const size_t need = bgnn_review_workspace_bytes(rows, cols);
  BGNN_REQUIRE(workspace_bytes >= need, "bgnn_review_regions: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  BGNN_REQUIRE(((uintptr_t)workspace & 7) == 0, "bgnn_review_regions: the workspace is not 8-byte aligned");
  BGNN_REQUIRE(((uintptr_t)records & 7) == 0 && ((uintptr_t)counts & 7) == 0, "bgnn_review_regions: records / counts are not 8-byte aligned");
  BGNN_REQUIRE(((uintptr_t)confidence & 3) == 0 && ((uintptr_t)review_mask & 3) == 0, "bgnn_review_regions: a plane is not 4-byte aligned");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const int64_t cells = rows * cols;
  char *w = static_cast<char *>(workspace);
  int64_t *part = reinterpret_cast<int64_t *>(w + WS_ROWS), *bases = reinterpret_cast<int64_t *>(w + WS_BASES);
  const size_t p4 = align256((size_t)cells * 4), p8 = align256((size_t)cells * 8);
  int32_t *parent = reinterpret_cast<int32_t *>(w + WS_PLANES);
  Aggregates ag;
  ag.sum = reinterpret_cast<unsigned long long *>(w + WS_PLANES + p4);
  ag.size = reinterpret_cast<int32_t *>(w + WS_PLANES + p4 + p8);
  ag.min_row = reinterpret_cast<int32_t *>(w + WS_PLANES + 2 * p4 + p8);
  ag.max_row = reinterpret_cast<int32_t *>(w + WS_PLANES + 3 * p4 + p8);
  ag.min_col = reinterpret_cast<int32_t *>(w + WS_PLANES + 4 * p4 + p8);
  ag.max_col = reinterpret_cast<int32_t *>(w + WS_PLANES + 5 * p4 + p8);
  TileGrid tg;
  tg.rows = (int32_t)rows; tg.cols = (int32_t)cols;
  tg.tiles_r = (int32_t)((rows + TILE_R - 1) / TILE_R); tg.tiles_c = (int32_t)((cols + TILE_C - 1) / TILE_C);
  const int64_t tiles = (int64_t)tg.tiles_r * tg.tiles_c;
  const int64_t borders = (int64_t)(tg.tiles_r - 1) * cols + (int64_t)(tg.tiles_c - 1) * rows;
  const auto grid_of = [](int64_t work_items) { return capped_grid(work_items, RV_MAX_GRID); };
  const int64_t steps = (cells + RV_CHUNK - 1) / RV_CHUNK;
  const int g_tiles = grid_of(tiles), g_flatten = grid_of((cells + FL_CHUNK - 1) / FL_CHUNK);
  const int g_borders = grid_of((borders + RV_THREADS - 1) / RV_THREADS);
  // the ordered passes: every workgroup a contiguous range of whole steps, none of them empty
  const int64_t chunk = (steps + RV_MAX_GRID - 1) / RV_MAX_GRID * RV_CHUNK;
  const int g_ranges = (int)((cells + chunk - 1) / chunk);
  const dim3 b(RV_THREADS), one(1);
  hipStream_t s = ctx->stream;

  hipLaunchKernelGGL(rv_local, dim3(g_tiles), b, 0, s, confidence, low, high, tg, parent, ag);
  hipLaunchKernelGGL(rv_merge, dim3(g_borders), b, 0, s, tg, parent);
  hipLaunchKernelGGL(rv_flatten, dim3(g_flatten), b, 0, s, cells, parent, ag);
  hipLaunchKernelGGL(rv_count, dim3(g_ranges), b, 0, s, cells, chunk, min_region_size, parent, ag.size, part);
  hipLaunchKernelGGL(rv_scan, one, b, 0, s, part, g_ranges, bases, counts);
  hipLaunchKernelGGL(rv_emit, dim3(g_ranges), b, 0, s, cells, chunk, min_region_size, parent, ag, bases,
                     static_cast<bgnn_review_record *>(records), capacity, review_mask);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
