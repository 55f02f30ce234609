// Gridding soundings at variable resolution (include/bgnn_soundings_vr.h): the address side.  A sounding goes to a record of the
// refinement grid of its base cell; the states, the stage and both finalize passes are those of sounding_grid.hip and
// sounding_robust.hip, which see a layout of `total` records as a 1 x total grid.
//
//   vr_density     the soundings that are finite, on the base grid and in range, counted per base cell: one integer atomic per run
//                  of neighbouring lanes in one base cell.
//   vr_plan_sums   the planner in three launches over tiles of VR_PLAN_TILE base cells: the dimension of every cell from its
//   vr_plan_scan   count and the ladder and the sum of d * d over the tile; the exclusive scan of the tile sums by one workgroup
//   vr_plan_cells  (64-bit: an integer sum, its order is free), which leaves the total; the scan inside every tile, which writes
//                  the table.
//   vr_add         the load shape of soundings_add: four soundings per thread, loaded before any is filed; then per sounding one
//                  16-byte load of its base cell's entry and file_sounding (sounding_file.h) under the record.  The five counters
//                  are reduced per workgroup and added with one atomic per workgroup and counter.
//   vr_stage       the same address into the positional (record, q) slots of a robust stage: one 8-byte store per sounding.
//   vr_flag        one streaming pass: the sounding's record, its q, |2q - center2| against limit.
//
// Writes are vector stores and integer atomics only.  Compiled with -ffp-contract=off: the address rounds operation by operation
// as the header states it.
#include "bgnn_internal.h"
#include "plane_util.h"
#include "sounding_file.h"
#include "sounding_vr_cell.h"
#include "../../include/bgnn_soundings.h"
#include "../../include/bgnn_soundings_robust.h"
#include "../../include/bgnn_soundings_vr.h"

namespace bgnn {

constexpr int VR_THREADS = BLOCK_THREADS;
constexpr int VR_WAVES = VR_THREADS / 64;
constexpr int VR_ITEMS = 4;                           // soundings per thread and step, a workgroup's width apart: coalesced loads
constexpr int VR_TILE = VR_THREADS * VR_ITEMS;
constexpr int VR_PLAN_TILE = BGNN_VR_PLAN_TILE;       // one base cell per thread
constexpr int64_t VR_MAX_DIM = 2147483647;
static_assert(VR_PLAN_TILE == VR_THREADS, "the planner's scan holds one base cell per thread");
static_assert(sizeof(VRLayoutEntry) == BGNN_VR_ENTRY_BYTES, "the entry the header documents");

struct VRGeometry {
  double x0, y0, B;
  int64_t BH, BW, total;
};

struct VRLadder {
  int32_t d[BGNN_VR_MAX_RUNGS];
  int32_t n;
  int64_t target, min_base;
};

// The kind of a sounding (sounding_file.h) and, where it is accepted, its record.  The entry is loaded only for a sounding that
// lies on the base grid: b is then inside the table.
__device__ __forceinline__ int vr_classify(double x, double y, float z, const VRGeometry &g, const VRLayoutEntry *__restrict__ table,
                                           int64_t *record) {
  double fu = 0.0, fv = 0.0;
  const int64_t b = vr_base_cell(x, y, g.x0, g.y0, g.B, g.BH, g.BW, &fu, &fv);
  bool refined = false;
  *record = -1;
  if (b >= 0) {
    const VRLayoutEntry e = table[b];                  // (16 bytes, one load)
    refined = vr_entry_refined(e, g.total);
    if (refined) *record = vr_record(e, fu, fv);
  }
  return sounding_kind(x, y, z, b >= 0, refined);
}

// the five counters of a workgroup: four into the header in front of the state or stage, unrefined beside it
__device__ __forceinline__ void vr_add_counters(const uint32_t (&tally)[SOUNDING_KINDS], uint32_t *scratch, char *header,
                                                int64_t *unrefined) {
  unsigned long long *counters = reinterpret_cast<unsigned long long *>(header);
#pragma unroll
  for (int j = 0; j < SOUNDING_KINDS; ++j) {
    const uint32_t total = block_reduce(tally[j], scratch, SumOp());
    if (threadIdx.x == 0 && total)
      atomicAdd(j == SOUNDING_UNREFINED ? reinterpret_cast<unsigned long long *>(unrefined) : counters + j, (unsigned long long)total);
  }
}

__global__ __launch_bounds__(VR_THREADS) void vr_density(const double *__restrict__ xs, const double *__restrict__ ys,
                                                         const float *__restrict__ zs, int64_t n, VRGeometry g,
                                                         uint32_t *__restrict__ counts) {
  for (int64_t base = (int64_t)blockIdx.x * VR_TILE; base < n; base += (int64_t)gridDim.x * VR_TILE) {
#pragma unroll
    for (int k = 0; k < VR_ITEMS; ++k) {
      const int64_t i = base + k * VR_THREADS + threadIdx.x;
      const bool in = i < n;
      const double x = in ? xs[i] : 0.0, y = in ? ys[i] : 0.0;
      const float z = in ? zs[i] : 0.0f;
      double fu, fv;
      const int64_t b = vr_base_cell(x, y, g.x0, g.y0, g.B, g.BH, g.BW, &fu, &fv);
      const bool ok = in && sounding_kind(x, y, z, b >= 0, true) == SOUNDING_ACCEPTED;
      // a run of neighbouring lanes in one base cell (a swath) is counted by its first lane (every lane of the wave gets here)
      const int lane = threadIdx.x & 63;
      const int64_t mine = ok ? b : (int64_t)-1 - lane;                                // (a rejected lane merges with nobody)
      const int64_t prev = __shfl_up(mine, 1);
      const bool start = lane == 0 || prev != mine;
      const unsigned long long starts = __ballot(start);
      if (ok && start) {
        const unsigned long long after = lane == 63 ? 0ull : starts >> (lane + 1);
        atomicAdd(counts + b, (uint32_t)(after ? __ffsll((long long)after) : 64 - lane));      // the lanes to the end of the run
      }
    }
  }
}

// the dimension the ladder gives a base cell of n soundings (0: not refined)
__device__ __forceinline__ int32_t vr_plan_dim(uint32_t n, const VRLadder &l) {
  int32_t d = 0;
  if ((int64_t)n >= l.min_base) {
#pragma unroll
    for (int r = 0; r < BGNN_VR_MAX_RUNGS; ++r)
      if (r < l.n && (int64_t)n >= l.target * (int64_t)l.d[r] * (int64_t)l.d[r]) d = l.d[r];      // (ascending: the last that fits)
  }
  return d;
}

// The exclusive scan of one value per thread over the workgroup; *total: the sum.  scratch: VR_WAVES words of LDS, free on return.
__device__ __forceinline__ unsigned long long vr_block_exclusive_scan(unsigned long long v, unsigned long long *scratch,
                                                                       unsigned long long *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  __syncthreads();
  if (lane == 63) scratch[wave] = incl;
  __syncthreads();
  unsigned long long before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < VR_WAVES; ++w) {
    const unsigned long long c = scratch[w];
    before += w < wave ? c : 0;
    all += c;
  }
  *total = all;
  return before + incl - v;
}

__global__ __launch_bounds__(VR_THREADS) void vr_plan_sums(const uint32_t *__restrict__ counts, int64_t n_cells, int64_t n_tiles,
                                                           VRLadder ladder, unsigned long long *__restrict__ sums) {
  __shared__ unsigned long long scratch[VR_THREADS];
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t b = tile * VR_PLAN_TILE + threadIdx.x;
    const int64_t d = b < n_cells ? vr_plan_dim(counts[b], ladder) : 0;
    const unsigned long long total = block_reduce((unsigned long long)(d * d), scratch, SumOp());
    if (threadIdx.x == 0) sums[tile] = total;
  }
}

// one workgroup: sums[] becomes its own exclusive scan; the sum of it all goes to *total
__global__ __launch_bounds__(VR_THREADS) void vr_plan_scan(unsigned long long *__restrict__ sums, int64_t n_tiles,
                                                           int64_t *__restrict__ total) {
  __shared__ unsigned long long scratch[VR_WAVES];
  unsigned long long running = 0;
  for (int64_t base = 0; base < n_tiles; base += VR_THREADS) {
    const int64_t i = base + threadIdx.x;
    const unsigned long long v = i < n_tiles ? sums[i] : 0ull;
    unsigned long long all;
    const unsigned long long before = vr_block_exclusive_scan(v, scratch, &all);
    if (i < n_tiles) sums[i] = running + before;
    running += all;
  }
  if (threadIdx.x == 0) *total = (int64_t)running;      // (below 2^31 cells of at most 2^30 records each)
}

__global__ __launch_bounds__(VR_THREADS) void vr_plan_cells(const uint32_t *__restrict__ counts, int64_t n_cells, int64_t n_tiles,
                                                            VRLadder ladder, const unsigned long long *__restrict__ sums,
                                                            VRLayoutEntry *__restrict__ table) {
  __shared__ unsigned long long scratch[VR_WAVES];
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t b = tile * VR_PLAN_TILE + threadIdx.x;
    const int32_t d = b < n_cells ? vr_plan_dim(counts[b], ladder) : 0;
    unsigned long long all;
    const unsigned long long before = vr_block_exclusive_scan((unsigned long long)((int64_t)d * d), scratch, &all);
    if (b < n_cells) {
      VRLayoutEntry e;
      e.index = (int64_t)(sums[tile] + before);
      e.dx = d;
      e.dy = d;
      table[b] = e;
    }
  }
}

__global__ __launch_bounds__(VR_THREADS) void vr_add(const double *__restrict__ xs, const double *__restrict__ ys,
                                                     const float *__restrict__ zs, int64_t n, VRGeometry g,
                                                     const VRLayoutEntry *__restrict__ table, char *__restrict__ state,
                                                     int64_t *__restrict__ unrefined) {
  __shared__ uint32_t scratch[VR_THREADS];
  SoundingCell *cells = reinterpret_cast<SoundingCell *>(state + BGNN_SOUNDINGS_HEADER_BYTES);
  const int t = threadIdx.x;
  uint32_t tally[SOUNDING_KINDS] = {0, 0, 0, 0, 0};    // (a workgroup sees fewer than 2^31 soundings)
  for (int64_t base = (int64_t)blockIdx.x * VR_TILE; base < n; base += (int64_t)gridDim.x * VR_TILE) {
    double x[VR_ITEMS], y[VR_ITEMS];
    float z[VR_ITEMS];
#pragma unroll
    for (int k = 0; k < VR_ITEMS; ++k) {
      const int64_t i = base + k * VR_THREADS + t;
      const bool in = i < n;
      x[k] = in ? xs[i] : 0.0;
      y[k] = in ? ys[i] : 0.0;
      z[k] = in ? zs[i] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < VR_ITEMS; ++k) {
      const bool in = base + k * VR_THREADS + t < n;
      int64_t record = -1;
      const int kind = in ? vr_classify(x[k], y[k], z[k], g, table, &record) : -1;
#pragma unroll
      for (int j = 0; j < SOUNDING_KINDS; ++j) tally[j] += kind == j;
      file_sounding(cells, kind == SOUNDING_ACCEPTED, record, z[k]);      // (every lane of the wave: the runs are merged inside it)
    }
  }
  vr_add_counters(tally, scratch, state, unrefined);
}

__global__ __launch_bounds__(VR_THREADS) void vr_stage(const double *__restrict__ xs, const double *__restrict__ ys,
                                                       const float *__restrict__ zs, int64_t n, VRGeometry g,
                                                       const VRLayoutEntry *__restrict__ table, char *__restrict__ stage,
                                                       int64_t offered, int64_t *__restrict__ unrefined) {
  __shared__ uint32_t scratch[VR_THREADS];
  int2 *slots = reinterpret_cast<int2 *>(stage + BGNN_ROBUST_STAGE_HEADER_BYTES) + offered;
  const int t = threadIdx.x;
  uint32_t tally[SOUNDING_KINDS] = {0, 0, 0, 0, 0};
  for (int64_t base = (int64_t)blockIdx.x * VR_TILE; base < n; base += (int64_t)gridDim.x * VR_TILE) {
    double x[VR_ITEMS], y[VR_ITEMS];
    float z[VR_ITEMS];
#pragma unroll
    for (int k = 0; k < VR_ITEMS; ++k) {
      const int64_t i = base + k * VR_THREADS + t;
      const bool in = i < n;
      x[k] = in ? xs[i] : 0.0;
      y[k] = in ? ys[i] : 0.0;
      z[k] = in ? zs[i] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < VR_ITEMS; ++k) {
      const int64_t i = base + k * VR_THREADS + t;
      if (i >= n) continue;
      int64_t record;
      const int kind = vr_classify(x[k], y[k], z[k], g, table, &record);
#pragma unroll
      for (int j = 0; j < SOUNDING_KINDS; ++j) tally[j] += kind == j;
      const bool ok = kind == SOUNDING_ACCEPTED;
      slots[i] = make_int2(ok ? (int)record : -1, ok ? (int)sounding_q(z[k]) : 0);      // (total <= 2^31 - 1: a record fits)
    }
  }
  vr_add_counters(tally, scratch, stage, unrefined);
}

__global__ __launch_bounds__(VR_THREADS) void vr_flag(const double *__restrict__ xs, const double *__restrict__ ys,
                                                      const float *__restrict__ zs, int64_t n, VRGeometry g,
                                                      const VRLayoutEntry *__restrict__ table, const int64_t *__restrict__ center2,
                                                      const int64_t *__restrict__ limit, uint8_t *__restrict__ flags) {
  for (int64_t base = (int64_t)blockIdx.x * VR_TILE; base < n; base += (int64_t)gridDim.x * VR_TILE) {
#pragma unroll
    for (int k = 0; k < VR_ITEMS; ++k) {
      const int64_t i = base + k * VR_THREADS + threadIdx.x;
      if (i >= n) continue;
      const float z = zs[i];
      int64_t record;
      uint8_t f = BGNN_ROBUST_FLAG_NOT_ACCEPTED;
      if (vr_classify(xs[i], ys[i], z, g, table, &record) == SOUNDING_ACCEPTED) {
        const int64_t d = 2 * (int64_t)sounding_q(z) - center2[record];
        f = (d < 0 ? -d : d) > limit[record] ? BGNN_ROBUST_FLAG_REJECTED : BGNN_ROBUST_FLAG_KEPT;      // (limit -1: an empty record)
      }
      flags[i] = f;
    }
  }
}

static inline bool vr_dim_ok(int64_t v) { return v >= 1 && v <= VR_MAX_DIM; }
static inline bool vr_cells_ok(int64_t height, int64_t width) { return height <= (int64_t)BGNN_VR_MAX_BASE_CELLS / width; }
static inline bool vr_aligned8(const void *p) { return ((uintptr_t)p & 7) == 0; }
static inline bool vr_finite(double v) { return v - v == 0.0; }
static inline int64_t vr_plan_tiles(int64_t n_cells) { return (n_cells + VR_PLAN_TILE - 1) / VR_PLAN_TILE; }

}  // namespace bgnn

using namespace bgnn;

#define VR_REQUIRE_BASE(fn)                                                                                                       \
  BGNN_REQUIRE(vr_dim_ok(base_height) && vr_dim_ok(base_width),                                                                   \
               fn ": a base grid of %lld x %lld cells, 1 .. 2147483647 each way expected", (long long)base_height,                \
               (long long)base_width);                                                                                            \
  if (!vr_cells_ok(base_height, base_width)) {                                                                                    \
    set_error(fn ": a base grid of %lld x %lld cells: more than %lld in all", (long long)base_height, (long long)base_width,      \
              (long long)BGNN_VR_MAX_BASE_CELLS);                                                                                 \
    return BGNN_ERR_UNSUPPORTED;                                                                                                  \
  }

// what every pass over soundings checks of its cloud and of the base grid
#define VR_REQUIRE_CLOUD(fn)                                                                                                      \
  BGNN_REQUIRE(n >= 0, fn ": %lld soundings", (long long)n);                                                                      \
  BGNN_REQUIRE(n == 0 || (x && y && z), fn ": NULL argument");                                                                    \
  BGNN_REQUIRE(vr_finite(base_res) && base_res > 0.0, fn ": a base resolution of %g, a finite number above 0 expected", base_res); \
  BGNN_REQUIRE(vr_finite(x0) && vr_finite(y0), fn ": the origin (%g, %g) is not finite", x0, y0);                                 \
  VR_REQUIRE_BASE(fn)

#define VR_REQUIRE_TABLE(fn)                                                                                           \
  BGNN_REQUIRE(table, fn ": NULL argument");                                                                           \
  BGNN_REQUIRE(total >= 1 && total <= (int64_t)BGNN_VR_MAX_RECORDS, fn ": a layout of %lld records, 1 .. %lld expected", \
               (long long)total, (long long)BGNN_VR_MAX_RECORDS);                                                      \
  BGNN_REQUIRE(vr_aligned8(table), fn ": the table is not 8-byte aligned")

extern "C" size_t bgnn_vr_soundings_plan_workspace_bytes(int64_t base_height, int64_t base_width) {
  if (!vr_dim_ok(base_height) || !vr_dim_ok(base_width) || !vr_cells_ok(base_height, base_width)) return 0;
  return align256(8 * (size_t)vr_plan_tiles(base_height * base_width));
}

extern "C" int bgnn_vr_soundings_density(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0,
                                         double y0, double base_res, int64_t base_height, int64_t base_width, uint32_t *counts) {
  // (the context last: what is wrong with the other arguments is reported whatever the context)
  VR_REQUIRE_CLOUD("bgnn_vr_soundings_density");
  BGNN_REQUIRE(counts, "bgnn_vr_soundings_density: NULL argument");
  BGNN_REQUIRE(((uintptr_t)counts & 3) == 0, "bgnn_vr_soundings_density: the counts are not 4-byte aligned");
  BGNN_REQUIRE(ctx, "bgnn_vr_soundings_density: NULL context");
  if (n == 0) return BGNN_OK;
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const VRGeometry geo = {x0, y0, base_res, base_height, base_width, 0};
  const dim3 g(capped_grid((n + VR_TILE - 1) / VR_TILE, PLANE_MAX_GRID)), b(VR_THREADS);
  hipLaunchKernelGGL(vr_density, g, b, 0, ctx->stream, x, y, z, n, geo, counts);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

extern "C" int bgnn_vr_soundings_plan(bgnn_ctx *ctx, const uint32_t *counts, int64_t base_height, int64_t base_width,
                                      const int32_t *ladder, int32_t n_rungs, int64_t target_count, int64_t min_base_count,
                                      void *workspace, size_t workspace_bytes, void *table, int64_t *total) {
  BGNN_REQUIRE(counts && ladder && workspace && table && total, "bgnn_vr_soundings_plan: NULL argument");
  VR_REQUIRE_BASE("bgnn_vr_soundings_plan");
  BGNN_REQUIRE(n_rungs >= 1 && n_rungs <= BGNN_VR_MAX_RUNGS, "bgnn_vr_soundings_plan: a ladder of %d rungs, 1 .. %d expected", (int)n_rungs,
               BGNN_VR_MAX_RUNGS);
  VRLadder l;
  for (int r = 0; r < BGNN_VR_MAX_RUNGS; ++r) l.d[r] = 0;
  for (int r = 0; r < n_rungs; ++r) {
    BGNN_REQUIRE(ladder[r] >= 1 && ladder[r] <= BGNN_VR_MAX_DIM, "bgnn_vr_soundings_plan: rung %d of the ladder is %d, 1 .. %d expected", r,
                 (int)ladder[r], BGNN_VR_MAX_DIM);
    BGNN_REQUIRE(r == 0 || ladder[r] > ladder[r - 1], "bgnn_vr_soundings_plan: the ladder is not strictly ascending at rung %d (%d after %d)",
                 r, (int)ladder[r], (int)(r ? ladder[r - 1] : 0));
    l.d[r] = ladder[r];
  }
  l.n = n_rungs;
  BGNN_REQUIRE(target_count >= 1 && target_count <= (int64_t)BGNN_VR_MAX_TARGET, "bgnn_vr_soundings_plan: a target_count of %lld, 1 .. %lld expected",
               (long long)target_count, (long long)BGNN_VR_MAX_TARGET);
  BGNN_REQUIRE(min_base_count >= 1 && min_base_count <= (int64_t)BGNN_VR_MAX_TARGET,
               "bgnn_vr_soundings_plan: a min_base_count of %lld, 1 .. %lld expected", (long long)min_base_count, (long long)BGNN_VR_MAX_TARGET);
  l.target = target_count;
  l.min_base = min_base_count;
  const int64_t n_cells = base_height * base_width, n_tiles = vr_plan_tiles(n_cells);
  const size_t need = align256(8 * (size_t)n_tiles);
  BGNN_REQUIRE(workspace_bytes >= need, "bgnn_vr_soundings_plan: a workspace of %zu bytes, %zu expected", workspace_bytes, need);
  BGNN_REQUIRE(((uintptr_t)counts & 3) == 0, "bgnn_vr_soundings_plan: the counts are not 4-byte aligned");
  BGNN_REQUIRE(vr_aligned8(workspace), "bgnn_vr_soundings_plan: the workspace is not 8-byte aligned");
  BGNN_REQUIRE(vr_aligned8(table), "bgnn_vr_soundings_plan: the table is not 8-byte aligned");
  BGNN_REQUIRE(vr_aligned8(total), "bgnn_vr_soundings_plan: total is not 8-byte aligned");
  BGNN_REQUIRE(ctx, "bgnn_vr_soundings_plan: NULL context");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  unsigned long long *sums = static_cast<unsigned long long *>(workspace);
  const dim3 g(capped_grid(n_tiles, PLANE_MAX_GRID)), b(VR_THREADS);
  hipLaunchKernelGGL(vr_plan_sums, g, b, 0, ctx->stream, counts, n_cells, n_tiles, l, sums);
  hipLaunchKernelGGL(vr_plan_scan, dim3(1), b, 0, ctx->stream, sums, n_tiles, total);
  hipLaunchKernelGGL(vr_plan_cells, g, b, 0, ctx->stream, counts, n_cells, n_tiles, l, sums, static_cast<VRLayoutEntry *>(table));
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

extern "C" int bgnn_vr_soundings_add(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0, double y0,
                                     double base_res, int64_t base_height, int64_t base_width, const void *table, int64_t total,
                                     int64_t offered, void *state, int64_t *unrefined) {
  VR_REQUIRE_CLOUD("bgnn_vr_soundings_add");
  BGNN_REQUIRE(state && unrefined, "bgnn_vr_soundings_add: NULL argument");
  VR_REQUIRE_TABLE("bgnn_vr_soundings_add");
  BGNN_REQUIRE(offered >= 0, "bgnn_vr_soundings_add: %lld soundings offered before", (long long)offered);
  BGNN_REQUIRE(n <= (int64_t)BGNN_SOUNDINGS_MAX_TOTAL && offered <= (int64_t)BGNN_SOUNDINGS_MAX_TOTAL - n,
               "bgnn_vr_soundings_add: %lld soundings after %lld offered before: a total above %lld", (long long)n, (long long)offered,
               (long long)BGNN_SOUNDINGS_MAX_TOTAL);
  BGNN_REQUIRE(vr_aligned8(state), "bgnn_vr_soundings_add: the state is not 8-byte aligned");
  BGNN_REQUIRE(vr_aligned8(unrefined), "bgnn_vr_soundings_add: the unrefined counter is not 8-byte aligned");
  BGNN_REQUIRE(ctx, "bgnn_vr_soundings_add: NULL context");
  if (n == 0) return BGNN_OK;
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const VRGeometry geo = {x0, y0, base_res, base_height, base_width, total};
  const dim3 g(capped_grid((n + VR_TILE - 1) / VR_TILE, PLANE_MAX_GRID)), b(VR_THREADS);
  hipLaunchKernelGGL(vr_add, g, b, 0, ctx->stream, x, y, z, n, geo, static_cast<const VRLayoutEntry *>(table), static_cast<char *>(state),
                     unrefined);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

extern "C" int bgnn_vr_soundings_stage(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0, double y0,
                                       double base_res, int64_t base_height, int64_t base_width, const void *table, int64_t total,
                                       int64_t offered, int64_t capacity, void *stage, int64_t *unrefined) {
  VR_REQUIRE_CLOUD("bgnn_vr_soundings_stage");
  BGNN_REQUIRE(stage && unrefined, "bgnn_vr_soundings_stage: NULL argument");
  VR_REQUIRE_TABLE("bgnn_vr_soundings_stage");
  BGNN_REQUIRE(capacity >= 1 && capacity <= (int64_t)BGNN_ROBUST_MAX_CAPACITY, "bgnn_vr_soundings_stage: a capacity of %lld soundings, 1 .. %lld expected",
               (long long)capacity, (long long)BGNN_ROBUST_MAX_CAPACITY);
  BGNN_REQUIRE(offered >= 0, "bgnn_vr_soundings_stage: %lld soundings offered before", (long long)offered);
  BGNN_REQUIRE(n <= capacity && offered <= capacity - n,
               "bgnn_vr_soundings_stage: %lld soundings after %lld offered before: more than the capacity of %lld", (long long)n,
               (long long)offered, (long long)capacity);
  BGNN_REQUIRE(vr_aligned8(stage), "bgnn_vr_soundings_stage: the stage is not 8-byte aligned");
  BGNN_REQUIRE(vr_aligned8(unrefined), "bgnn_vr_soundings_stage: the unrefined counter is not 8-byte aligned");
  BGNN_REQUIRE(ctx, "bgnn_vr_soundings_stage: NULL context");
  if (n == 0) return BGNN_OK;
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const VRGeometry geo = {x0, y0, base_res, base_height, base_width, total};
  const dim3 g(capped_grid((n + VR_TILE - 1) / VR_TILE, PLANE_MAX_GRID)), b(VR_THREADS);
  hipLaunchKernelGGL(vr_stage, g, b, 0, ctx->stream, x, y, z, n, geo, static_cast<const VRLayoutEntry *>(table), static_cast<char *>(stage),
                     offered, unrefined);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

extern "C" int bgnn_vr_soundings_flag(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0, double y0,
                                      double base_res, int64_t base_height, int64_t base_width, const void *table, int64_t total,
                                      const int64_t *center2, const int64_t *limit, uint8_t *flags) {
  VR_REQUIRE_CLOUD("bgnn_vr_soundings_flag");
  BGNN_REQUIRE(center2 && limit && (n == 0 || flags), "bgnn_vr_soundings_flag: NULL argument");
  VR_REQUIRE_TABLE("bgnn_vr_soundings_flag");
  BGNN_REQUIRE(vr_aligned8(center2) && vr_aligned8(limit), "bgnn_vr_soundings_flag: center2 or limit is not 8-byte aligned");
  BGNN_REQUIRE(ctx, "bgnn_vr_soundings_flag: NULL context");
  if (n == 0) return BGNN_OK;
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const VRGeometry geo = {x0, y0, base_res, base_height, base_width, total};
  const dim3 g(capped_grid((n + VR_TILE - 1) / VR_TILE, PLANE_MAX_GRID)), b(VR_THREADS);
  hipLaunchKernelGGL(vr_flag, g, b, 0, ctx->stream, x, y, z, n, geo, static_cast<const VRLayoutEntry *>(table), center2, limit, flags);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
