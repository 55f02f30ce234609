// Robust gridding of a point cloud of soundings (include/bgnn_soundings_robust.h): the accepted soundings are staged, filed by
// cell, sorted per cell, and the median, the MAD and the kept / rejected rule of every cell are read off the sorted segments.
//
//   sounding_pass<UniformAddress, StageSink>
//                       the cloud pass of sounding_pass.h under the address rule of sounding_grid.hip, but a sounding goes into its
//                       own slot of the stage as (cell, q), cell = -1 where it is not accepted: one 8-byte store, no atomics but
//                       the four counters.
//   robust_count        one integer atomic per accepted slot into the count of its cell.
//   robust_tile_sums    the exclusive scan of the counts over the cells in three launches: the sum of every tile of RB_SCAN_TILE
//   scan_tile_sums      cells, the scan of those sums by one workgroup (plane_util.h), and the scan inside every tile, which writes
//   robust_scan_cells   start[] and appends every cell with more than ROBUST_WAVE_MAX soundings to the list of long segments.
//   robust_scatter      q into sorted_q[start[cell] + cursor], the cursor taken by counting the cell's count back down to zero.
//   robust_sort_short   a wave takes 64 cells at a time and ranks every segment of 2 .. ROBUST_WAVE_MAX soundings by counting:
//                       lane i holds s_i and counts the s_j below it (ties by lane), n shuffles for a segment of n.
//   robust_sort_long    a fixed grid walks the list: a segment of up to ROBUST_LDS_MAX soundings is sorted by one workgroup in LDS
//                       (bitonic, padded to a power of two); a longer one by a least-significant-digit radix sort of four 8-bit
//                       passes between the segment and the workspace, one workgroup, tiles of 256 keys ranked in order (a wave
//                       ranks its equal digits by eight ballots, the four waves are chained through LDS).  Slow by design: one
//                       workgroup's bandwidth, three barriers per tile.
//   robust_stats_short  one thread per cell with up to ROBUST_WAVE_MAX soundings (the empty ones included): the MAD by the merge
//                       walk of sounding_rank.h, the kept range by two binary searches, the sums over it in a loop.
//   robust_stats_long   one workgroup per listed cell: thread 0 finds the MAD by bisection and the kept range, all threads sum.
//   sounding_pass<UniformAddress, FlagSink>
//                       one streaming pass: the sounding's cell, its q, |2q - center2| against limit.
//
// The only arrival order that shows anywhere is that of the cursors and of the list; the sort removes the first, and nothing
// depends on the second.  Compiled with -ffp-contract=off.
#include "bgnn_internal.h"
#include "sounding_args.h"
#include "sounding_moments.h"
#include "sounding_pass.h"
#include "sounding_rank.h"

namespace bgnn {

constexpr int RB_THREADS = BLOCK_THREADS;
constexpr int RB_WAVES = RB_THREADS / 64;
constexpr int RB_SCAN_ITEMS = 16;                     // consecutive cells per thread of the scan
constexpr int RB_SCAN_TILE = RB_THREADS * RB_SCAN_ITEMS;
constexpr int RB_LONG_GRID = 1024;                    // workgroups that walk the list of long segments
constexpr int RB_CELL_MAX_GRID = 1 << 16;
constexpr int ROBUST_WAVE_MAX = BGNN_ROBUST_WAVE_MAX;
constexpr int ROBUST_LDS_MAX = BGNN_ROBUST_LDS_MAX;
static_assert(ROBUST_WAVE_MAX == 64, "robust_sort_short ranks one sounding per lane");
static_assert((ROBUST_LDS_MAX & (ROBUST_LDS_MAX - 1)) == 0 && ROBUST_LDS_MAX >= 2 * RB_THREADS, "the bitonic network pads to a power of two");

__global__ __launch_bounds__(RB_THREADS) void robust_count(const int2 *__restrict__ slots, int64_t offered, uint32_t n_cells,
                                                           uint32_t *__restrict__ cnt) {
  for (int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x; i < offered; i += (int64_t)gridDim.x * RB_THREADS) {
    const uint32_t cell = (uint32_t)slots[i].x;        // (-1, and a cell of some other grid, fail the one comparison)
    if (cell < n_cells) atomicAdd(cnt + cell, 1u);
  }
}

__global__ __launch_bounds__(RB_THREADS) void robust_scatter(const int2 *__restrict__ slots, int64_t offered, uint32_t n_cells,
                                                             const uint32_t *__restrict__ start, uint32_t *__restrict__ cnt,
                                                             int32_t *__restrict__ binned) {
  for (int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x; i < offered; i += (int64_t)gridDim.x * RB_THREADS) {
    const int2 s = slots[i];
    if ((uint32_t)s.x < n_cells) binned[start[s.x] + (atomicSub(cnt + s.x, 1u) - 1u)] = s.y;      // (the counts are back at zero afterwards)
  }
}

__global__ __launch_bounds__(RB_THREADS) void robust_tile_sums(const uint32_t *__restrict__ cnt, int64_t n_cells, int64_t n_tiles,
                                                               uint32_t *__restrict__ sums) {
  __shared__ uint32_t scratch[RB_THREADS];
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t base = tile * RB_SCAN_TILE;
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < RB_SCAN_ITEMS; ++j) {
      const int64_t i = base + j * RB_THREADS + threadIdx.x;
      v += i < n_cells ? cnt[i] : 0u;
    }
    const uint32_t total = block_reduce(v, scratch, SumOp());
    if (threadIdx.x == 0) sums[tile] = total;
  }
}

__global__ __launch_bounds__(RB_THREADS) void robust_scan_cells(const uint32_t *__restrict__ cnt, int64_t n_cells, int64_t n_tiles,
                                                                const uint32_t *__restrict__ sums, uint32_t *__restrict__ start,
                                                                uint32_t *__restrict__ list_count, int32_t *__restrict__ list) {
  __shared__ uint32_t scratch[RB_WAVES];
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t first = tile * RB_SCAN_TILE + (int64_t)threadIdx.x * RB_SCAN_ITEMS;
    uint32_t c[RB_SCAN_ITEMS], mine = 0;
#pragma unroll
    for (int j = 0; j < RB_SCAN_ITEMS; ++j) {
      c[j] = first + j < n_cells ? cnt[first + j] : 0u;
      mine += c[j];
    }
    uint32_t total;
    uint32_t at = sums[tile] + block_exclusive_scan(mine, scratch, &total);
#pragma unroll
    for (int j = 0; j < RB_SCAN_ITEMS; ++j) {
      if (first + j < n_cells) {
        start[first + j] = at;
        if (c[j] > (uint32_t)ROBUST_WAVE_MAX) list[atomicAdd(list_count, 1u)] = (int32_t)(first + j);
      }
      at += c[j];
    }
  }
}

__global__ __launch_bounds__(RB_THREADS) void robust_sort_short(const uint32_t *__restrict__ start, int64_t n_cells,
                                                                int32_t *__restrict__ binned) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * RB_THREADS + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * RB_WAVES;
  for (int64_t base = wave * 64; base < n_cells; base += n_waves * 64) {                 // (wave-uniform)
    const int64_t cell = base + lane;
    uint32_t b = 0, cnt = 0;
    if (cell < n_cells) {
      b = start[cell];
      cnt = start[cell + 1] - b;
    }
    unsigned long long todo = __ballot(cnt >= 2 && cnt <= (uint32_t)ROBUST_WAVE_MAX);
    while (todo) {
      const int j = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const uint32_t sb = __shfl(b, j), sn = __shfl(cnt, j);
      const bool have = (uint32_t)lane < sn;
      const int32_t v = have ? binned[sb + lane] : INT32_MAX;
      uint32_t rank = 0;
      for (uint32_t i = 0; i < sn; ++i) {
        const int32_t o = __shfl(v, (int)i);
        rank += (o < v) || (o == v && i < (uint32_t)lane);
      }
      if (have) binned[sb + rank] = v;                 // (every lane has read its sounding before any is written: one wave)
    }
  }
}

// ---- segments longer than a wave ---------------------------------------------------------------------------------------------------

__device__ __forceinline__ void sort_in_lds(int32_t *seg, uint32_t n, int32_t *s) {
  const int t = threadIdx.x;
  uint32_t padded = 2 * RB_THREADS;
  while (padded < n) padded <<= 1;                     // <= ROBUST_LDS_MAX
  __syncthreads();
  for (uint32_t i = t; i < padded; i += RB_THREADS) s[i] = i < n ? seg[i] : INT32_MAX;
  __syncthreads();
  for (uint32_t k = 2; k <= padded; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = t; i < padded; i += RB_THREADS) {
        const uint32_t p = i ^ j;
        if (p > i) {
          const int32_t a = s[i], b = s[p];
          if ((a > b) == ((i & k) == 0)) { s[i] = b; s[p] = a; }
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = t; i < n; i += RB_THREADS) seg[i] = s[i];
}

// lds: 4 x 256 words of digit offsets and RB_WAVES x 256 words of per-wave digit counts
__device__ __forceinline__ void sort_by_radix(int32_t *seg, int32_t *tmp, uint32_t n, uint32_t *lds) {
  uint32_t *offset = lds, *wave_cnt = lds + 4 * 256;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  __syncthreads();
  for (int i = t; i < (4 + RB_WAVES) * 256; i += RB_THREADS) lds[i] = 0;
  __syncthreads();
  for (uint32_t i = t; i < n; i += RB_THREADS) {
    const uint32_t key = (uint32_t)seg[i] ^ 0x80000000u;                                  // unsigned order = signed order
#pragma unroll
    for (int p = 0; p < 4; ++p) atomicAdd(&offset[p * 256 + ((key >> (8 * p)) & 255u)], 1u);
  }
  __syncthreads();
  if (t < 4) {                                         // the four histograms into their exclusive scans
    uint32_t run = 0;
    for (int d = 0; d < 256; ++d) {
      const uint32_t c = offset[t * 256 + d];
      offset[t * 256 + d] = run;
      run += c;
    }
  }
  __syncthreads();
  int32_t *src = seg, *dst = tmp;
  for (int p = 0; p < 4; ++p) {
    uint32_t *off = offset + p * 256;
    for (uint32_t base = 0; base < n; base += RB_THREADS) {                               // (uniform over the workgroup)
      const uint32_t i = base + t;
      const bool have = i < n;
      const uint32_t key = have ? (uint32_t)src[i] ^ 0x80000000u : 0xFFFFFFFFu;
      const uint32_t digit = (key >> (8 * p)) & 255u;
      unsigned long long peers = __ballot(have);       // the lanes of this wave with this lane's digit
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long m = __ballot(bit);
        peers &= bit ? m : ~m;
      }
      const uint32_t rank = __popcll(peers & ((1ull << lane) - 1ull));
      const bool leader = have && rank == 0;
      if (leader) wave_cnt[wave * 256 + digit] = __popcll(peers);
      __syncthreads();
      uint32_t before = 0, all = 0;
      if (have) {
#pragma unroll
        for (int w = 0; w < RB_WAVES; ++w) {
          const uint32_t c = wave_cnt[w * 256 + digit];
          before += w < wave ? c : 0;
          all += c;
        }
        dst[off[digit] + before + rank] = (int32_t)(key ^ 0x80000000u);
      }
      __syncthreads();
      if (leader) {
        if (before == 0) off[digit] += all;            // the first wave that holds the digit moves its offset on
        wave_cnt[wave * 256 + digit] = 0;
      }
      __syncthreads();
    }
    int32_t *swap = src; src = dst; dst = swap;        // (the barrier above orders the pass's stores before the next pass's loads)
  }
}

__global__ __launch_bounds__(RB_THREADS) void robust_sort_long(const uint32_t *__restrict__ start, const uint32_t *__restrict__ list_count,
                                                               const int32_t *__restrict__ list, int32_t *__restrict__ binned,
                                                               int32_t *__restrict__ tmp) {
  __shared__ int32_t lds[ROBUST_LDS_MAX];
  static_assert(ROBUST_LDS_MAX >= (4 + RB_WAVES) * 256, "the radix sort's tables fit the bitonic sort's LDS");
  const uint32_t listed = *list_count;
  for (uint32_t e = blockIdx.x; e < listed; e += gridDim.x) {
    const int32_t cell = list[e];
    const uint32_t b = start[cell], n = start[cell + 1] - b;
    if (n <= (uint32_t)ROBUST_LDS_MAX) sort_in_lds(binned + b, n, lds);
    else sort_by_radix(binned + b, tmp + b, n, reinterpret_cast<uint32_t *>(lds));
  }
}

// ---- the planes ----------------------------------------------------------------------------------------------------------------------

struct RobustPlanes {
  int32_t *count, *kept;
  float *median, *mad, *kept_mean, *kept_std, *kept_min, *kept_max;
  uint8_t *valid;
  int64_t *center2, *limit;
};

__device__ __forceinline__ void write_cell(const RobustPlanes &o, int64_t cell, uint32_t n, uint32_t kept, int64_t m2, int64_t D,
                                           int64_t L, const SegSums &sums, int32_t q_first, int32_t q_last, int32_t min_count,
                                           float nodata) {
  const bool ok = kept >= (uint32_t)min_count;         // (min_count >= 1: an empty cell is never valid)
  float med = nodata, mad = nodata, mean = nodata, sd = nodata, lo = nodata, hi = nodata;
  if (ok) {
    med = (float)((double)m2 * (1.0 / 131072.0));
    mad = (float)((double)D * (1.0 / 262144.0));
    mean = sounding_mean(kept, sums.s1);
    sd = sounding_std(kept, sums.s1, sums.s2_lo, sums.s2_hi);
    lo = (float)((double)q_first * (1.0 / 65536.0));
    hi = (float)((double)q_last * (1.0 / 65536.0));
  }
  o.count[cell] = (int32_t)n;
  o.kept[cell] = (int32_t)kept;
  o.median[cell] = med;
  o.mad[cell] = mad;
  o.kept_mean[cell] = mean;
  o.kept_std[cell] = sd;
  o.kept_min[cell] = lo;
  o.kept_max[cell] = hi;
  o.valid[cell] = ok ? 1 : 0;
  o.center2[cell] = m2;
  o.limit[cell] = L;
}

__global__ __launch_bounds__(RB_THREADS) void robust_stats_short(const uint32_t *__restrict__ start, const int32_t *__restrict__ binned,
                                                                 int64_t n_cells, double k, double floor_m, int32_t min_count,
                                                                 float nodata, RobustPlanes o) {
  for (int64_t cell = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x; cell < n_cells; cell += (int64_t)gridDim.x * RB_THREADS) {
    const uint32_t b = start[cell], n = start[cell + 1] - b;
    if (n > (uint32_t)ROBUST_WAVE_MAX) continue;       // robust_stats_long's
    SegSums sums = {0, 0, 0};
    if (n == 0) {
      write_cell(o, cell, 0, 0, 0, 0, -1, sums, 0, 0, min_count, nodata);
      continue;
    }
    const int32_t *s = binned + b;
    const int64_t m2 = seg_center2(s, n), D = seg_mad2_walk(s, n, m2), L = robust_limit(D, k, floor_m);
    int64_t lo, hi;
    seg_within(s, n, m2, L, &lo, &hi);
    for (int64_t i = lo; i < hi; ++i) seg_sums_add(&sums, s[i]);
    write_cell(o, cell, n, (uint32_t)(hi - lo), m2, D, L, sums, s[lo], s[hi - 1], min_count, nodata);      // (hi > lo: the median is kept)
  }
}

__global__ __launch_bounds__(RB_THREADS) void robust_stats_long(const uint32_t *__restrict__ start, const int32_t *__restrict__ binned,
                                                                const uint32_t *__restrict__ list_count, const int32_t *__restrict__ list,
                                                                double k, double floor_m, int32_t min_count, float nodata,
                                                                RobustPlanes o) {
  __shared__ unsigned long long scratch[RB_THREADS];
  __shared__ int64_t rule[5];                          // m2, D, L, lo, hi
  const uint32_t listed = *list_count;
  for (uint32_t e = blockIdx.x; e < listed; e += gridDim.x) {
    const int32_t cell = list[e];
    const uint32_t b = start[cell], n = start[cell + 1] - b;
    const int32_t *s = binned + b;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int64_t m2 = seg_center2(s, n), D = seg_mad2_bisect(s, n, m2), L = robust_limit(D, k, floor_m);
      int64_t lo, hi;
      seg_within(s, n, m2, L, &lo, &hi);
      rule[0] = m2; rule[1] = D; rule[2] = L; rule[3] = lo; rule[4] = hi;
    }
    __syncthreads();
    const int64_t lo = rule[3], hi = rule[4];
    SegSums mine = {0, 0, 0};
    for (int64_t i = lo + threadIdx.x; i < hi; i += RB_THREADS) seg_sums_add(&mine, s[i]);
    SegSums sums;
    sums.s1 = (int64_t)block_reduce((unsigned long long)mine.s1, scratch, SumOp());
    sums.s2_lo = block_reduce((unsigned long long)mine.s2_lo, scratch, SumOp());
    sums.s2_hi = block_reduce((unsigned long long)mine.s2_hi, scratch, SumOp());
    if (threadIdx.x == 0)
      write_cell(o, cell, n, (uint32_t)(hi - lo), rule[0], rule[1], rule[2], sums, s[lo], s[hi - 1], min_count, nodata);
  }
}

// ---- the host side --------------------------------------------------------------------------------------------------------------------

// the workspace of finalize: every part a multiple of 256 bytes
struct RobustWorkspace {
  size_t cnt, sums, list_count, list, tmp, bytes;     // offsets, and the size of it all
  int64_t n_tiles;
};
static RobustWorkspace rb_workspace(int64_t n_cells, int64_t capacity) {
  RobustWorkspace w;
  w.n_tiles = (n_cells + RB_SCAN_TILE - 1) / RB_SCAN_TILE;
  w.cnt = 0;
  w.sums = w.cnt + align256(4 * (size_t)n_cells);
  w.list_count = w.sums + align256(4 * (size_t)w.n_tiles);
  w.list = w.list_count + 256;
  w.tmp = w.list + align256(4 * ((size_t)capacity / (ROBUST_WAVE_MAX + 1) + 1));       // a listed cell holds ROBUST_WAVE_MAX + 1 at least
  w.bytes = w.tmp + align256(4 * (size_t)capacity);
  return w;
}

}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_soundings_robust_stage_bytes(int64_t capacity) {
  if (!stage_capacity_ok(capacity)) return 0;
  const unsigned __int128 bytes = (unsigned __int128)capacity * BGNN_ROBUST_SLOT_BYTES + BGNN_ROBUST_STAGE_HEADER_BYTES;
  return bytes > (unsigned __int128)SIZE_MAX ? 0 : (size_t)bytes;
}

extern "C" size_t bgnn_soundings_robust_workspace_bytes(int64_t height, int64_t width, int64_t capacity) {
  if (!dim_ok(height) || !dim_ok(width) || !cells_ok(height, width, BGNN_ROBUST_MAX_CELLS) || !stage_capacity_ok(capacity)) return 0;
  if (sizeof(size_t) < 8) return 0;                    // (fewer than 2^31 cells and soundings of 4 bytes each: 64 bits hold it all)
  return rb_workspace(height * width, capacity).bytes;
}

extern "C" int bgnn_soundings_robust_reset(bgnn_ctx *ctx, void *stage) {
  BGNN_REQUIRE(stage, "bgnn_soundings_robust_reset: NULL argument");
  BGNN_REQUIRE(aligned8(stage), "bgnn_soundings_robust_reset: the stage is not 8-byte aligned");
  BGNN_REQUIRE(ctx, "bgnn_soundings_robust_reset: NULL context");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  BGNN_HIP_CHECK(hipMemsetAsync(stage, 0, BGNN_ROBUST_STAGE_HEADER_BYTES, ctx->stream));
  return BGNN_OK;
}

extern "C" int bgnn_soundings_robust_add(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0, double y0,
                                         double res, int64_t height, int64_t width, int64_t offered, int64_t capacity, void *stage) {
  // (the context last: what is wrong with the other arguments is reported whatever the context)
  const char *fn = "bgnn_soundings_robust_add";
  BGNN_TRY(require_cloud(fn, x, y, z, n, res, x0, y0, "resolution", stage != nullptr));
  BGNN_TRY(require_robust_grid(fn, height, width));
  BGNN_TRY(require_capacity(fn, capacity));
  BGNN_TRY(require_offered_capacity(fn, n, offered, capacity));
  BGNN_REQUIRE(aligned8(stage), "%s: the stage is not 8-byte aligned", fn);
  return launch_sounding_pass(fn, ctx, x, y, z, n, UniformAddress{x0, y0, res, height, width},
                              StageSink{static_cast<char *>(stage), offered});
}

extern "C" int bgnn_soundings_robust_finalize(bgnn_ctx *ctx, const void *stage, int64_t offered, int64_t capacity, int64_t height,
                                              int64_t width, double k, double floor_m, int32_t min_count, float nodata_value,
                                              void *workspace, size_t workspace_bytes, uint32_t *start, int32_t *sorted_q, int32_t *count,
                                              int32_t *kept, float *median, float *mad, float *kept_mean, float *kept_std, float *kept_min,
                                              float *kept_max, uint8_t *valid, int64_t *center2, int64_t *limit) {
  BGNN_REQUIRE(stage && workspace && start && sorted_q && count && kept && median && mad && kept_mean && kept_std && kept_min &&
                   kept_max && valid && center2 && limit,
               "bgnn_soundings_robust_finalize: NULL argument");
  BGNN_TRY(require_robust_grid("bgnn_soundings_robust_finalize", height, width));
  BGNN_TRY(require_capacity("bgnn_soundings_robust_finalize", capacity));
  BGNN_REQUIRE(offered >= 0 && offered <= capacity, "bgnn_soundings_robust_finalize: %lld soundings offered, 0 .. the capacity of %lld expected",
               (long long)offered, (long long)capacity);
  BGNN_REQUIRE(finite_arg(k) && k >= 1.0, "bgnn_soundings_robust_finalize: a multiplier k of %g, a finite number of at least 1 expected", k);
  BGNN_REQUIRE(finite_arg(floor_m) && floor_m >= 0.0, "bgnn_soundings_robust_finalize: a floor of %g m, a finite number of at least 0 expected",
               floor_m);
  BGNN_REQUIRE(min_count >= 1, "bgnn_soundings_robust_finalize: a min_count of %d, at least 1 expected", (int)min_count);
  const int64_t n_cells = height * width;
  const RobustWorkspace w = rb_workspace(n_cells, capacity);
  BGNN_REQUIRE(workspace_bytes >= w.bytes, "bgnn_soundings_robust_finalize: a workspace of %zu bytes, %zu expected", workspace_bytes, w.bytes);
  BGNN_REQUIRE(aligned8(stage), "bgnn_soundings_robust_finalize: the stage is not 8-byte aligned");
  BGNN_REQUIRE(aligned8(workspace), "bgnn_soundings_robust_finalize: the workspace is not 8-byte aligned");
  BGNN_REQUIRE(aligned8(center2) && aligned8(limit), "bgnn_soundings_robust_finalize: center2 or limit is not 8-byte aligned");
  BGNN_REQUIRE(ctx, "bgnn_soundings_robust_finalize: NULL context");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  char *ws = static_cast<char *>(workspace);
  uint32_t *cnt = reinterpret_cast<uint32_t *>(ws + w.cnt), *sums = reinterpret_cast<uint32_t *>(ws + w.sums);
  uint32_t *list_count = reinterpret_cast<uint32_t *>(ws + w.list_count);
  int32_t *list = reinterpret_cast<int32_t *>(ws + w.list), *tmp = reinterpret_cast<int32_t *>(ws + w.tmp);
  const int2 *slots = reinterpret_cast<const int2 *>(static_cast<const char *>(stage) + BGNN_ROBUST_STAGE_HEADER_BYTES);
  const RobustPlanes planes = {count, kept, median, mad, kept_mean, kept_std, kept_min, kept_max, valid, center2, limit};
  const dim3 b(RB_THREADS);
  const dim3 g_slots(capped_grid((offered + RB_THREADS - 1) / RB_THREADS, PLANE_MAX_GRID));
  const dim3 g_tiles(capped_grid(w.n_tiles, PLANE_MAX_GRID));
  const dim3 g_waves(capped_grid((n_cells + RB_THREADS - 1) / RB_THREADS, RB_CELL_MAX_GRID));      // a wave per 64 cells, a thread per cell
  BGNN_HIP_CHECK(hipMemsetAsync(ws, 0, w.list, ctx->stream));                                     // the counts, the sums, the list's length
  if (offered > 0) hipLaunchKernelGGL(robust_count, g_slots, b, 0, ctx->stream, slots, offered, (uint32_t)n_cells, cnt);
  hipLaunchKernelGGL(robust_tile_sums, g_tiles, b, 0, ctx->stream, cnt, n_cells, w.n_tiles, sums);
  hipLaunchKernelGGL((scan_tile_sums<uint32_t, uint32_t>), dim3(1), b, 0, ctx->stream, sums, w.n_tiles, start + n_cells);      // (the accepted)
  hipLaunchKernelGGL(robust_scan_cells, g_tiles, b, 0, ctx->stream, cnt, n_cells, w.n_tiles, sums, start, list_count, list);
  if (offered > 0) {
    hipLaunchKernelGGL(robust_scatter, g_slots, b, 0, ctx->stream, slots, offered, (uint32_t)n_cells, start, cnt, sorted_q);
    hipLaunchKernelGGL(robust_sort_short, g_waves, b, 0, ctx->stream, start, n_cells, sorted_q);
    hipLaunchKernelGGL(robust_sort_long, dim3(RB_LONG_GRID), b, 0, ctx->stream, start, list_count, list, sorted_q, tmp);
  }
  hipLaunchKernelGGL(robust_stats_short, g_waves, b, 0, ctx->stream, start, sorted_q, n_cells, k, floor_m, min_count, nodata_value, planes);
  if (offered > 0)
    hipLaunchKernelGGL(robust_stats_long, dim3(RB_LONG_GRID), b, 0, ctx->stream, start, sorted_q, list_count, list, k, floor_m, min_count,
                       nodata_value, planes);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

extern "C" int bgnn_soundings_robust_flag(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0, double y0,
                                          double res, int64_t height, int64_t width, const int64_t *center2, const int64_t *limit,
                                          uint8_t *flags) {
  const char *fn = "bgnn_soundings_robust_flag";
  BGNN_TRY(require_cloud(fn, x, y, z, n, res, x0, y0, "resolution", center2 && limit && (n == 0 || flags)));
  BGNN_TRY(require_robust_grid(fn, height, width));
  BGNN_REQUIRE(aligned8(center2) && aligned8(limit), "%s: center2 or limit is not 8-byte aligned", fn);
  return launch_sounding_pass(fn, ctx, x, y, z, n, UniformAddress{x0, y0, res, height, width}, FlagSink{center2, limit, flags});
}
