// Depth hypotheses per cell (include/bgnn_hypotheses.h): the sorted segments that the robust finalize leaves (sounding_robust.hip)
// are cut into runs without a gap, one run is chosen per cell and the planes are read off it.  The segment logic is that of
// sounding_hypothesis.h; the two size classes are those of the finalize.
//
//   hyp_count_short     one thread per cell: the runs of a segment of up to ROBUST_WAVE_MAX soundings (0 for an empty cell); a
//                       longer one is appended to the list of long segments (the finalize's list went with its workspace).
//   hyp_count_long      a fixed grid walks the list, one workgroup per cell: thread t asks positions 1 + t, 257 + t, ..; one
//                       block_reduce.
//   hyp_tile_sums       where records are wanted, the exclusive scan of n_hyp over the cells into hyp_start, in three launches as
//   scan_tile_sums      in the finalize: the sum of every tile of HY_SCAN_TILE cells, the scan of those sums by one workgroup
//   hyp_scan_cells      (plane_util.h), the scan inside every tile.
//   hyp_choose_short    one thread per short cell walks its segment again: the best key so far and its run, the records on the
//                       way, then the sums over the chosen run and the planes.
//   hyp_choose_long     one workgroup per listed cell: every thread summarises a contiguous share of the segment, thread 0 stitches
//                       the 256 summaries in order, all threads sum the chosen run (block_reduce), and every thread writes the
//                       records of the runs that end inside its share.
//
// No atomics but the list's counter; the only order that shows anywhere is that of the list, and nothing depends on it.  Compiled
// with -ffp-contract=off.
#include "bgnn_internal.h"
#include "plane_util.h"
#include "sounding_args.h"
#include "sounding_hypothesis.h"
#include "sounding_moments.h"
#include "sounding_rank.h"
#include "../../include/bgnn_hypotheses.h"

namespace bgnn {

constexpr int HY_THREADS = BLOCK_THREADS;
constexpr int HY_WAVES = HY_THREADS / 64;
constexpr int HY_SCAN_ITEMS = 16;                     // consecutive cells per thread of the scan
constexpr int HY_SCAN_TILE = HY_THREADS * HY_SCAN_ITEMS;
constexpr int HY_LONG_GRID = 1024;                    // workgroups that walk the list of long segments
constexpr int HY_WAVE_MAX = BGNN_ROBUST_WAVE_MAX;
constexpr int64_t HY_MAX_GAP_Q = BGNN_HYP_MAX_GAP_Q;

__global__ __launch_bounds__(HY_THREADS) void hyp_count_short(const uint32_t *__restrict__ start, const int32_t *__restrict__ q,
                                                              int64_t n_cells, int64_t gap_q, int32_t *__restrict__ n_hyp,
                                                              uint32_t *__restrict__ list_count, int32_t *__restrict__ list) {
  for (int64_t cell = (int64_t)blockIdx.x * HY_THREADS + threadIdx.x; cell < n_cells; cell += (int64_t)gridDim.x * HY_THREADS) {
    const uint32_t b = start[cell], n = start[cell + 1] - b;
    if (n > (uint32_t)HY_WAVE_MAX) {
      list[atomicAdd(list_count, 1u)] = (int32_t)cell;                                  // hyp_count_long's
      continue;
    }
    n_hyp[cell] = n == 0 ? 0 : (int32_t)(1 + hyp_count_breaks(q + b, 1, n, 1, gap_q));
  }
}

__global__ __launch_bounds__(HY_THREADS) void hyp_count_long(const uint32_t *__restrict__ start, const int32_t *__restrict__ q,
                                                             const uint32_t *__restrict__ list_count, const int32_t *__restrict__ list,
                                                             int64_t gap_q, int32_t *__restrict__ n_hyp) {
  __shared__ uint32_t scratch[HY_THREADS];
  const uint32_t listed = *list_count;
  for (uint32_t e = blockIdx.x; e < listed; e += gridDim.x) {
    const int32_t cell = list[e];
    const uint32_t b = start[cell], n = start[cell + 1] - b;
    const uint32_t mine = (uint32_t)hyp_count_breaks(q + b, 1 + (int64_t)threadIdx.x, n, HY_THREADS, gap_q);
    const uint32_t breaks = block_reduce(mine, scratch, SumOp());
    if (threadIdx.x == 0) n_hyp[cell] = (int32_t)(1 + breaks);
  }
}

__global__ __launch_bounds__(HY_THREADS) void hyp_tile_sums(const int32_t *__restrict__ n_hyp, int64_t n_cells, int64_t n_tiles,
                                                            uint32_t *__restrict__ sums) {
  __shared__ uint32_t scratch[HY_THREADS];
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t base = tile * HY_SCAN_TILE;
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < HY_SCAN_ITEMS; ++j) {
      const int64_t i = base + j * HY_THREADS + threadIdx.x;
      v += i < n_cells ? (uint32_t)n_hyp[i] : 0u;
    }
    const uint32_t total = block_reduce(v, scratch, SumOp());
    if (threadIdx.x == 0) sums[tile] = total;
  }
}

__global__ __launch_bounds__(HY_THREADS) void hyp_scan_cells(const int32_t *__restrict__ n_hyp, int64_t n_cells, int64_t n_tiles,
                                                             const uint32_t *__restrict__ sums, uint32_t *__restrict__ hyp_start) {
  __shared__ uint32_t scratch[HY_WAVES];
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t first = tile * HY_SCAN_TILE + (int64_t)threadIdx.x * HY_SCAN_ITEMS;
    uint32_t c[HY_SCAN_ITEMS], mine = 0;
#pragma unroll
    for (int j = 0; j < HY_SCAN_ITEMS; ++j) {
      c[j] = first + j < n_cells ? (uint32_t)n_hyp[first + j] : 0u;
      mine += c[j];
    }
    uint32_t total;
    uint32_t at = sums[tile] + block_exclusive_scan(mine, scratch, &total);
#pragma unroll
    for (int j = 0; j < HY_SCAN_ITEMS; ++j) {
      if (first + j < n_cells) hyp_start[first + j] = at;
      at += c[j];
    }
  }
}

// ---- the planes ----------------------------------------------------------------------------------------------------------------------

struct HypPlanes {
  int32_t *chosen, *kept;
  float *depth, *sd, *lo, *hi, *share;
  uint8_t *valid;
  int64_t *center2, *limit;
};

// s: the cell's segment of n soundings; sums: over the chosen run p (p.h = -1: none, and s is not read)
__device__ __forceinline__ void write_hyp_cell(const HypPlanes &o, int64_t cell, const int32_t *s, uint32_t n, const HypPick &p,
                                               const SegSums &sums, float nodata) {
  const bool ok = p.h >= 0;
  float mean = nodata, sd = nodata, lo = nodata, hi = nodata, share = nodata;
  int64_t c2 = 0, lim = -1;
  uint32_t nh = 0;
  if (ok) {
    nh = (uint32_t)(p.b - p.a);
    const int32_t q_first = s[p.a], q_last = s[p.b - 1];
    mean = sounding_mean(nh, sums.s1);
    sd = sounding_std(nh, sums.s1, sums.s2_lo, sums.s2_hi);
    lo = (float)((double)q_first * (1.0 / 65536.0));
    hi = (float)((double)q_last * (1.0 / 65536.0));
    share = (float)((double)nh / (double)n);
    c2 = (int64_t)q_first + (int64_t)q_last;
    lim = (int64_t)q_last - (int64_t)q_first;
  }
  o.chosen[cell] = (int32_t)p.h;
  o.kept[cell] = (int32_t)nh;
  o.depth[cell] = mean;
  o.sd[cell] = sd;
  o.lo[cell] = lo;
  o.hi[cell] = hi;
  o.share[cell] = share;
  o.valid[cell] = ok ? 1 : 0;
  o.center2[cell] = c2;
  o.limit[cell] = lim;
}

// guide: nullptr under the count rule.  hyp_start: nullptr where no records are wanted
__global__ __launch_bounds__(HY_THREADS) void hyp_choose_short(const uint32_t *__restrict__ start, const int32_t *__restrict__ q,
                                                               int64_t n_cells, int64_t gap_q, const float *__restrict__ guide,
                                                               int32_t min_count, float nodata, HypPlanes o,
                                                               const uint32_t *__restrict__ hyp_start, uint32_t *__restrict__ hyp_first,
                                                               int32_t *__restrict__ hyp_count) {
  for (int64_t cell = (int64_t)blockIdx.x * HY_THREADS + threadIdx.x; cell < n_cells; cell += (int64_t)gridDim.x * HY_THREADS) {
    const uint32_t b = start[cell], n = start[cell + 1] - b;
    if (n > (uint32_t)HY_WAVE_MAX) continue;           // hyp_choose_long's
    SegSums sums = {0, 0, 0};
    HypPick p = {-1, 0, 0, {0, 0}};
    const int32_t *s = q + b;
    if (n > 0) {
      const HypRule r = hyp_rule_of(s, n, gap_q, min_count, guide != nullptr, guide ? guide[cell] : 0.0f);
      const uint32_t at = hyp_start ? hyp_start[cell] : 0u;
      hyp_walk(s, n, r, &p, hyp_start ? hyp_first + at : nullptr, hyp_start ? hyp_count + at : nullptr, b);
      for (int64_t i = p.a; i < p.b; ++i) seg_sums_add(&sums, s[i]);
    }
    write_hyp_cell(o, cell, s, n, p, sums, nodata);
  }
}

__global__ __launch_bounds__(HY_THREADS) void hyp_choose_long(const uint32_t *__restrict__ start, const int32_t *__restrict__ q,
                                                              const uint32_t *__restrict__ list_count, const int32_t *__restrict__ list,
                                                              int64_t gap_q, const float *__restrict__ guide, int32_t min_count,
                                                              float nodata, HypPlanes o, const uint32_t *__restrict__ hyp_start,
                                                              uint32_t *__restrict__ hyp_first, int32_t *__restrict__ hyp_count) {
  __shared__ HypChunk chunks[HY_THREADS];
  __shared__ unsigned long long scratch[HY_THREADS];
  __shared__ HypPick pick;
  const int t = threadIdx.x;
  const uint32_t listed = *list_count;
  for (uint32_t e = blockIdx.x; e < listed; e += gridDim.x) {
    const int32_t cell = list[e];
    const uint32_t b = start[cell], n = start[cell + 1] - b;
    const int32_t *s = q + b;
    const HypRule r = hyp_rule_of(s, n, gap_q, min_count, guide != nullptr, guide ? guide[cell] : 0.0f);
    const int64_t len = ((int64_t)n + HY_THREADS - 1) / HY_THREADS, lo = t * len, hi = lo + len < (int64_t)n ? lo + len : (int64_t)n;
    uint32_t *rec_first = nullptr;
    int32_t *rec_count = nullptr;
    if (hyp_start) {
      const uint32_t at = hyp_start[cell];
      rec_first = hyp_first + at;
      rec_count = hyp_count + at;
    }
    chunks[t] = hyp_chunk_scan(s, lo, hi, r);           // (its last readers passed the barriers of block_reduce below)
    __syncthreads();
    if (t == 0) hyp_stitch(s, n, chunks, HY_THREADS, r, &pick, rec_first, rec_count, b);
    __syncthreads();
    const HypPick p = pick;
    SegSums mine = {0, 0, 0};
    for (int64_t i = p.a + t; i < p.b; i += HY_THREADS) seg_sums_add(&mine, s[i]);      // (a == b where none is chosen)
    SegSums sums;
    sums.s1 = (int64_t)block_reduce((unsigned long long)mine.s1, scratch, SumOp());
    sums.s2_lo = block_reduce((unsigned long long)mine.s2_lo, scratch, SumOp());
    sums.s2_hi = block_reduce((unsigned long long)mine.s2_hi, scratch, SumOp());
    if (t == 0) write_hyp_cell(o, cell, s, n, p, sums, nodata);
    if (rec_first) hyp_chunk_records(s, gap_q, chunks[t], rec_first, rec_count, b);
  }
}

// ---- the host side --------------------------------------------------------------------------------------------------------------------

// the workspace of build: every part a multiple of 256 bytes
struct HypWorkspace {
  size_t sums, list_count, list, bytes;               // offsets, and the size of it all
  int64_t n_tiles;
};
static HypWorkspace hyp_workspace(int64_t n_cells, int64_t capacity) {
  HypWorkspace w;
  w.n_tiles = (n_cells + HY_SCAN_TILE - 1) / HY_SCAN_TILE;
  w.sums = 0;
  w.list_count = w.sums + align256(4 * (size_t)w.n_tiles);
  w.list = w.list_count + 256;
  w.bytes = w.list + align256(4 * ((size_t)capacity / (HY_WAVE_MAX + 1) + 1));          // a listed cell holds HY_WAVE_MAX + 1 at least
  return w;
}

static bool hyp_cells_ok(int64_t v) { return v >= 1 && v <= (int64_t)BGNN_HYP_MAX_CELLS; }
static bool hyp_capacity_ok(int64_t v) { return v >= 1 && v <= (int64_t)BGNN_HYP_MAX_CAPACITY; }

}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_hypotheses_workspace_bytes(int64_t cells, int64_t capacity) {
  if (!hyp_cells_ok(cells) || !hyp_capacity_ok(capacity)) return 0;
  return hyp_workspace(cells, capacity).bytes;
}

extern "C" int bgnn_hypotheses_build(bgnn_ctx *ctx, const uint32_t *start, const int32_t *sorted_q, int64_t cells, int64_t capacity,
                                     int64_t gap_q, int32_t rule, const float *guide, int32_t min_count, float nodata_value,
                                     void *workspace, size_t workspace_bytes, int32_t *n_hyp, int32_t *chosen, int32_t *kept, float *depth,
                                     float *stddev, float *zmin, float *zmax, float *share, uint8_t *valid, int64_t *center2,
                                     int64_t *limit, uint32_t *hyp_start, uint32_t *hyp_first, int32_t *hyp_count) {
  const char *fn = "bgnn_hypotheses_build";
  BGNN_REQUIRE(start && sorted_q && workspace && n_hyp && chosen && kept && depth && stddev && zmin && zmax && share && valid && center2 &&
                   limit,
               "%s: NULL argument", fn);
  BGNN_REQUIRE(hyp_cells_ok(cells), "%s: %lld cells, 1 .. %lld expected", fn, (long long)cells, (long long)BGNN_HYP_MAX_CELLS);
  BGNN_REQUIRE(hyp_capacity_ok(capacity), "%s: a capacity of %lld soundings, 1 .. %lld expected", fn, (long long)capacity,
               (long long)BGNN_HYP_MAX_CAPACITY);
  BGNN_REQUIRE(gap_q >= 0 && gap_q <= HY_MAX_GAP_Q, "%s: a gap_q of %lld, 0 .. %lld expected", fn, (long long)gap_q, (long long)HY_MAX_GAP_Q);
  BGNN_REQUIRE(rule == BGNN_HYP_RULE_COUNT || rule == BGNN_HYP_RULE_GUIDE, "%s: unknown rule %d", fn, (int)rule);
  BGNN_REQUIRE(rule != BGNN_HYP_RULE_COUNT || !guide, "%s: a guide with the count rule", fn);
  BGNN_REQUIRE(rule != BGNN_HYP_RULE_GUIDE || guide, "%s: no guide with the guide rule", fn);
  BGNN_REQUIRE(min_count >= 1, "%s: a min_count of %d, at least 1 expected", fn, (int)min_count);
  const HypWorkspace w = hyp_workspace(cells, capacity);
  BGNN_REQUIRE(workspace_bytes >= w.bytes, "%s: a workspace of %zu bytes, %zu expected", fn, workspace_bytes, w.bytes);
  BGNN_REQUIRE(aligned8(workspace), "%s: the workspace is not 8-byte aligned", fn);
  BGNN_REQUIRE(aligned8(center2) && aligned8(limit), "%s: center2 or limit is not 8-byte aligned", fn);
  const bool records = hyp_start != nullptr;
  BGNN_REQUIRE((hyp_first != nullptr) == records && (hyp_count != nullptr) == records,
               "%s: records given in part: hyp_start, hyp_first and hyp_count go together", fn);
  BGNN_REQUIRE(ctx, "%s: NULL context", fn);
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  char *ws = static_cast<char *>(workspace);
  uint32_t *sums = reinterpret_cast<uint32_t *>(ws + w.sums), *list_count = reinterpret_cast<uint32_t *>(ws + w.list_count);
  int32_t *list = reinterpret_cast<int32_t *>(ws + w.list);
  const HypPlanes planes = {chosen, kept, depth, stddev, zmin, zmax, share, valid, center2, limit};
  const dim3 b(HY_THREADS);
  const dim3 g_cells(capped_grid((cells + HY_THREADS - 1) / HY_THREADS, PLANE_MAX_GRID));         // a thread per cell
  const dim3 g_tiles(capped_grid(w.n_tiles, PLANE_MAX_GRID));
  BGNN_HIP_CHECK(hipMemsetAsync(list_count, 0, 256, ctx->stream));
  hipLaunchKernelGGL(hyp_count_short, g_cells, b, 0, ctx->stream, start, sorted_q, cells, gap_q, n_hyp, list_count, list);
  hipLaunchKernelGGL(hyp_count_long, dim3(HY_LONG_GRID), b, 0, ctx->stream, start, sorted_q, list_count, list, gap_q, n_hyp);
  if (records) {
    hipLaunchKernelGGL(hyp_tile_sums, g_tiles, b, 0, ctx->stream, n_hyp, cells, w.n_tiles, sums);
    hipLaunchKernelGGL((scan_tile_sums<uint32_t, uint32_t>), dim3(1), b, 0, ctx->stream, sums, w.n_tiles, hyp_start + cells);      // (the total)
    hipLaunchKernelGGL(hyp_scan_cells, g_tiles, b, 0, ctx->stream, n_hyp, cells, w.n_tiles, sums, hyp_start);
  }
  hipLaunchKernelGGL(hyp_choose_short, g_cells, b, 0, ctx->stream, start, sorted_q, cells, gap_q, guide, min_count, nodata_value, planes,
                     hyp_start, hyp_first, hyp_count);
  hipLaunchKernelGGL(hyp_choose_long, dim3(HY_LONG_GRID), b, 0, ctx->stream, start, sorted_q, list_count, list, gap_q, guide, min_count,
                     nodata_value, planes, hyp_start, hyp_first, hyp_count);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
