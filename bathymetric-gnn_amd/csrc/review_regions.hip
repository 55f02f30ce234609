// Low-confidence regions for review (include/bgnn_review.h): scripts/export_for_review.py of the reference's training plan, on a
// confidence plane that stays in HBM.  Six launches on the context's stream; every grid is a function of rows and cols.
//
//   rv_local     a 16 x 64 tile in LDS: the tile-local labelling of the uncertain cells; beside the size, per tile-local root the
//                fixed-point confidence sum and the rows / columns the component touches in the tile (a 16-bit and a 64-bit set:
//                integer LDS atomics), written as sum and bounds at tile-local roots
//   label_merge, label_flatten<Aggregates>   component_label.h: the unions across the tile borders; size, sum and bounds combined
//                at the roots (integer atomicAdd / atomicMin / atomicMax)
//   rv_count     every workgroup owns a contiguous range of cells: uncertain cells, components, kept components and their cells
//   rv_scan      one workgroup: the exclusive scan of the kept counts in workgroup order (each workgroup's first record) and counts[]
//   rv_emit      the same ranges again, in order: a kept root's record goes to base + rank in the range; the mask of every cell from
//                the size at its root (at most two hops after the flatten)
//
// The labelling, its invariant parent[i] <= i and the termination argument: component_label.h.  A component's root is its smallest
// cell index, so "ascending by root" is the order scipy.ndimage.label numbers the components.  No thread waits for another: no
// spin-wait, no grid-wide barrier, no persistent kernel, no float atomics.
//
// Compiled with -ffp-contract=off: (double)c * 2^32 is exact either way, the flag keeps the file under the rule of its neighbours.
#include "bgnn_internal.h"
#include "component_label.h"
#include "../../include/bgnn_review.h"

namespace bgnn {
namespace {

constexpr int RV_THREADS = BLOCK_THREADS;
constexpr int RV_ITEMS = 4;                           // cells per thread and step of a streaming pass (each load coalesced)
constexpr int RV_CHUNK = RV_THREADS * RV_ITEMS;
constexpr int RV_WAVES = RV_THREADS / 64;
constexpr int ROW_WORDS = 4;                          // a partial row of rv_count: int64 [BGNN_RV_COUNTS]

// workspace: the partial rows, the record bases, then the seven planes
constexpr size_t WS_ROWS = 0;
constexpr size_t WS_BASES = WS_ROWS + (size_t)PLANE_MAX_GRID * ROW_WORDS * 8;
constexpr size_t WS_PLANES = WS_BASES + (size_t)PLANE_MAX_GRID * 8;
static_assert(WS_PLANES == BGNN_RV_FIXED_BYTES && WS_PLANES % 256 == 0, "the fixed part as the header states it");
static_assert(sizeof(bgnn_review_record) == BGNN_RV_RECORD_BYTES, "record layout");
static_assert(ROW_WORDS == BGNN_RV_COUNTS, "one partial per count");

// The aggregates of the components, indexed by cell; valid at tile-local roots after rv_local, complete at global roots after
// label_flatten, whose aggregate this is (component_label.h)
struct Aggregates {
  int32_t *size;
  unsigned long long *sum;
  int32_t *min_row, *max_row, *min_col, *max_col;

  struct Piece {
    int32_t size, r_lo, r_hi, c_lo, c_hi;
    unsigned long long sum;
  };
  __device__ static Piece identity() { return {0, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, 0ull}; }
  __device__ Piece load(int32_t i) const { return {size[i], min_row[i], max_row[i], min_col[i], max_col[i], sum[i]}; }
  __device__ static void combine(Piece &g, int w) {
    g.size += __shfl_xor(g.size, w);
    g.sum += __shfl_xor(g.sum, w);
    g.r_lo = min(g.r_lo, __shfl_xor(g.r_lo, w)); g.r_hi = max(g.r_hi, __shfl_xor(g.r_hi, w));
    g.c_lo = min(g.c_lo, __shfl_xor(g.c_lo, w)); g.c_hi = max(g.c_hi, __shfl_xor(g.c_hi, w));
  }
  __device__ void add_to_root(int32_t r, const Piece &g) const {
    atomicAdd(size + r, g.size);
    atomicAdd(sum + r, g.sum);
    atomicMin(min_row + r, g.r_lo);
    atomicMax(max_row + r, g.r_hi);
    atomicMin(min_col + r, g.c_lo);
    atomicMax(max_col + r, g.c_hi);
  }
};

__device__ __forceinline__ unsigned long long fixed_point(float c) {              // c in [0, 1]: at most 2^32
  return (unsigned long long)__double2ll_rn((double)c * 4294967296.0);
}

__global__ __launch_bounds__(RV_THREADS) void rv_local(const float *__restrict__ conf, float low, float high, TileGrid tg,
                                                       int32_t *__restrict__ parent, Aggregates ag) {
  __shared__ int32_t lp[TILE_CELLS], lsize[TILE_CELLS];
  __shared__ uint32_t lrows[TILE_CELLS];
  __shared__ unsigned long long lsum[TILE_CELLS], lcols[TILE_CELLS];
  const int t = threadIdx.x;
  const int64_t tiles = tg.tiles();
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int r0 = (int)(tile / tg.tiles_c) * TILE_R, c0 = (int)(tile % tg.tiles_c) * TILE_C;
    __syncthreads();                                            // (the previous tile is written out)
    bool unc[TILE_PER];
    unsigned long long fx[TILE_PER];
#pragma unroll
    for (int k = 0; k < TILE_PER; ++k) {
      const int l = tile_cell(k), gr = r0 + l / TILE_C, gc = c0 + l % TILE_C;
      const bool in = gr < tg.rows && gc < tg.cols;
      const float c = in ? conf[(int64_t)gr * tg.cols + gc] : __uint_as_float(0x7FC00000u);
      unc[k] = c >= low && c <= high && finite_bits(c);
      fx[k] = unc[k] ? fixed_point(c) : 0ull;
      lrows[l] = 0u; lsum[l] = 0ull; lcols[l] = 0ull;
    }
    int32_t root[TILE_PER];
    tile_label(unc, lp, lsize, root);
    // As tile_label counts: the cells that share the first one's root go to LDS as one set of atomics, the others cell by cell.
    int32_t r_first = -1;
    uint32_t rows_first = 0u;
    unsigned long long sum_first = 0ull;
#pragma unroll
    for (int k = 0; k < TILE_PER; ++k) {
      const int l = tile_cell(k);
      if (!unc[k]) continue;
      if (r_first < 0) r_first = root[k];
      if (root[k] == r_first) {
        rows_first |= 1u << (l / TILE_C); sum_first += fx[k];
      } else {
        atomicOr(&lrows[root[k]], 1u << (l / TILE_C));
        atomicAdd(&lsum[root[k]], fx[k]);
        atomicOr(&lcols[root[k]], 1ull << (l % TILE_C));
      }
    }
    if (r_first >= 0) {
      atomicOr(&lrows[r_first], rows_first);
      atomicAdd(&lsum[r_first], sum_first);
      atomicOr(&lcols[r_first], 1ull << (t % TILE_C));
    }
    tile_write(tg, r0, c0, unc, root, lsize, parent, ag.size);
#pragma unroll
    for (int k = 0; k < TILE_PER; ++k) {
      const int l = tile_cell(k);
      if (!unc[k] || root[k] != l) continue;                    // (a tile-local root: on the mask, so inside the plane)
      const int64_t i = tile_to_global(tg, r0, c0, l);
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
  constexpr int PER = PLANE_MAX_GRID / RV_THREADS;
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
  const TileGrid tg(rows, cols);
  const int64_t steps = (cells + RV_CHUNK - 1) / RV_CHUNK;
  // the ordered passes: every workgroup a contiguous range of whole steps, none of them empty
  const int64_t chunk = (steps + PLANE_MAX_GRID - 1) / PLANE_MAX_GRID * RV_CHUNK;
  const int g_ranges = (int)((cells + chunk - 1) / chunk);
  const dim3 b(RV_THREADS), one(1);
  hipStream_t s = ctx->stream;

  hipLaunchKernelGGL(rv_local, dim3(tg.local_grid()), b, 0, s, confidence, low, high, tg, parent, ag);
  launch_merge_flatten(s, tg, parent, ag);
  hipLaunchKernelGGL(rv_count, dim3(g_ranges), b, 0, s, cells, chunk, min_region_size, parent, ag.size, part);
  hipLaunchKernelGGL(rv_scan, one, b, 0, s, part, g_ranges, bases, counts);
  hipLaunchKernelGGL(rv_emit, dim3(g_ranges), b, 0, s, cells, chunk, min_region_size, parent, ag, bases,
                     static_cast<bgnn_review_record *>(records), capacity, review_mask);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
