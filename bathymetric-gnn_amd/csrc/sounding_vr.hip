// Gridding soundings at variable resolution (include/bgnn_soundings_vr.h): the address side.  A sounding goes to a record of the
// refinement grid of its base cell; the states, the stage and both finalize passes are those of sounding_grid.hip and
// sounding_robust.hip, which see a layout of `total` records as a 1 x total grid.
//
// Three of the four cloud passes are instantiations of sounding_pass (sounding_pass.h: four soundings per thread, loaded before any is handled):
//
//   <VRBaseAddress, DensitySink>  the soundings that are finite, on the base grid and in range, counted per base cell: one integer
//                                 atomic per run of neighbouring lanes in one base cell.  No table, no counters.
//   <VRAddress, FileSink>         per sounding one 16-byte load of its base cell's entry and file_sounding (sounding_file.h) under
//                                 the record.  The five counters are reduced per workgroup and added with one atomic per workgroup
//                                 and counter, unrefined beside the header.
//   <VRAddress, FlagSink>         the sounding's record, its q, |2q - center2| against limit.  No counters.
//
//   vr_stage        the address of <VRAddress, ...> into the positional (record, q) slots of a robust stage, one 8-byte store per
//                   sounding: the same loop as a kernel of its own (see there why).
//   vr_plan_sums    the planner in three launches over tiles of VR_PLAN_TILE base cells: the dimension of every cell from its
//   scan_tile_sums  count and the ladder and the sum of d * d over the tile; the exclusive scan of the tile sums by one workgroup
//   vr_plan_cells   (plane_util.h; 64-bit: an integer sum, its order is free), which leaves the total; the scan inside every tile,
//                   which writes the table.
//
// Writes are vector stores and integer atomics only.  Compiled with -ffp-contract=off: the address rounds operation by operation
// as the header states it.
#include "bgnn_internal.h"
#include "sounding_args.h"
#include "sounding_pass.h"
#include "../../include/bgnn_soundings_vr.h"

namespace bgnn {

constexpr int VR_THREADS = BLOCK_THREADS;
constexpr int VR_WAVES = VR_THREADS / 64;
constexpr int VR_PLAN_TILE = BGNN_VR_PLAN_TILE;       // one base cell per thread
static_assert(VR_PLAN_TILE == VR_THREADS, "the planner's scan holds one base cell per thread");
static_assert(sizeof(VRLayoutEntry) == BGNN_VR_ENTRY_BYTES, "the entry the header documents");

struct VRLadder {
  int32_t d[BGNN_VR_MAX_RUNGS];
  int32_t n;
  int64_t target, min_base;
};

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

__global__ __launch_bounds__(VR_THREADS) void vr_plan_cells(const uint32_t *__restrict__ counts, int64_t n_cells, int64_t n_tiles,
                                                            VRLadder ladder, const unsigned long long *__restrict__ sums,
                                                            VRLayoutEntry *__restrict__ table) {
  __shared__ unsigned long long scratch[VR_WAVES];
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t b = tile * VR_PLAN_TILE + threadIdx.x;
    const int32_t d = b < n_cells ? vr_plan_dim(counts[b], ladder) : 0;
    unsigned long long all;
    const unsigned long long before = block_exclusive_scan((unsigned long long)((int64_t)d * d), scratch, &all);
    if (b < n_cells) {
      VRLayoutEntry e;
      e.index = (int64_t)(sums[tile] + before);
      e.dx = d;
      e.dy = d;
      table[b] = e;
    }
  }
}

// ---- the stage pass, kept as a kernel of its own ------------------------------------------------------------------------------------
// As sounding_pass<VRAddress, StageSink> this pass measured 1.46 ms against 1.26 ms on 2 x 10^8 soundings in swath order (the same
// on scattered ones); __restrict__ on the members of the address and the sink, and classifying before or between the stores, did
// not change that, and this kernel inside the same translation unit is back at 1.26 ms.  The cause is not known, so the kernel
// stays as it was, with its own copy of the address rule and of the counters, until it is.

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

__global__ __launch_bounds__(VR_THREADS) void vr_stage(const double *__restrict__ xs, const double *__restrict__ ys,
                                                       const float *__restrict__ zs, int64_t n, VRGeometry g,
                                                       const VRLayoutEntry *__restrict__ table, char *__restrict__ stage,
                                                       int64_t offered, int64_t *__restrict__ unrefined) {
  __shared__ uint32_t scratch[VR_THREADS];
  int2 *slots = reinterpret_cast<int2 *>(stage + BGNN_ROBUST_STAGE_HEADER_BYTES) + offered;
  const int t = threadIdx.x;
  uint32_t tally[SOUNDING_KINDS] = {0, 0, 0, 0, 0};
  for (int64_t base = (int64_t)blockIdx.x * PASS_TILE; base < n; base += (int64_t)gridDim.x * PASS_TILE) {
    double x[PASS_ITEMS], y[PASS_ITEMS];
    float z[PASS_ITEMS];
#pragma unroll
    for (int k = 0; k < PASS_ITEMS; ++k) {
      const int64_t i = base + k * VR_THREADS + t;
      const bool in = i < n;
      x[k] = in ? xs[i] : 0.0;
      y[k] = in ? ys[i] : 0.0;
      z[k] = in ? zs[i] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < PASS_ITEMS; ++k) {
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

static inline int64_t vr_plan_tiles(int64_t n_cells) { return (n_cells + VR_PLAN_TILE - 1) / VR_PLAN_TILE; }

static int require_base(const char *fn, int64_t base_height, int64_t base_width) {
  return require_grid(fn, base_height, base_width, "base grid", BGNN_VR_MAX_BASE_CELLS, "");
}

// what every pass over soundings checks of its cloud and of the base grid
static int require_vr_cloud(const char *fn, const double *x, const double *y, const float *z, int64_t n, double x0, double y0,
                            double base_res, int64_t base_height, int64_t base_width) {
  BGNN_TRY(require_cloud(fn, x, y, z, n, base_res, x0, y0, "base resolution"));
  return require_base(fn, base_height, base_width);
}

static int require_table(const char *fn, const void *table, int64_t total) {
  BGNN_REQUIRE(table, "%s: NULL argument", fn);
  BGNN_REQUIRE(total >= 1 && total <= (int64_t)BGNN_VR_MAX_RECORDS, "%s: a layout of %lld records, 1 .. %lld expected", fn, (long long)total,
               (long long)BGNN_VR_MAX_RECORDS);
  BGNN_REQUIRE(aligned8(table), "%s: the table is not 8-byte aligned", fn);
  return BGNN_OK;
}

}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_vr_soundings_plan_workspace_bytes(int64_t base_height, int64_t base_width) {
  if (!dim_ok(base_height) || !dim_ok(base_width) || !cells_ok(base_height, base_width, BGNN_VR_MAX_BASE_CELLS)) return 0;
  return align256(8 * (size_t)vr_plan_tiles(base_height * base_width));
}

extern "C" int bgnn_vr_soundings_density(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0,
                                         double y0, double base_res, int64_t base_height, int64_t base_width, uint32_t *counts) {
  // (the context last: what is wrong with the other arguments is reported whatever the context)
  const char *fn = "bgnn_vr_soundings_density";
  BGNN_TRY(require_vr_cloud(fn, x, y, z, n, x0, y0, base_res, base_height, base_width));
  BGNN_REQUIRE(counts, "%s: NULL argument", fn);
  BGNN_REQUIRE(((uintptr_t)counts & 3) == 0, "%s: the counts are not 4-byte aligned", fn);
  const VRGeometry geo = {x0, y0, base_res, base_height, base_width, 0};
  return launch_sounding_pass(fn, ctx, x, y, z, n, VRBaseAddress{geo}, DensitySink{counts});
}

extern "C" int bgnn_vr_soundings_plan(bgnn_ctx *ctx, const uint32_t *counts, int64_t base_height, int64_t base_width,
                                      const int32_t *ladder, int32_t n_rungs, int64_t target_count, int64_t min_base_count,
                                      void *workspace, size_t workspace_bytes, void *table, int64_t *total) {
  BGNN_REQUIRE(counts && ladder && workspace && table && total, "bgnn_vr_soundings_plan: NULL argument");
  BGNN_TRY(require_base("bgnn_vr_soundings_plan", base_height, base_width));
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
  BGNN_REQUIRE(aligned8(workspace), "bgnn_vr_soundings_plan: the workspace is not 8-byte aligned");
  BGNN_REQUIRE(aligned8(table), "bgnn_vr_soundings_plan: the table is not 8-byte aligned");
  BGNN_REQUIRE(aligned8(total), "bgnn_vr_soundings_plan: total is not 8-byte aligned");
  BGNN_REQUIRE(ctx, "bgnn_vr_soundings_plan: NULL context");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  unsigned long long *sums = static_cast<unsigned long long *>(workspace);
  const dim3 g(capped_grid(n_tiles, PLANE_MAX_GRID)), b(VR_THREADS);
  hipLaunchKernelGGL(vr_plan_sums, g, b, 0, ctx->stream, counts, n_cells, n_tiles, l, sums);
  hipLaunchKernelGGL((scan_tile_sums<unsigned long long, int64_t>), dim3(1), b, 0, ctx->stream, sums, n_tiles, total);      // (total < 2^61)
  hipLaunchKernelGGL(vr_plan_cells, g, b, 0, ctx->stream, counts, n_cells, n_tiles, l, sums, static_cast<VRLayoutEntry *>(table));
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

extern "C" int bgnn_vr_soundings_add(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0, double y0,
                                     double base_res, int64_t base_height, int64_t base_width, const void *table, int64_t total,
                                     int64_t offered, void *state, int64_t *unrefined) {
  const char *fn = "bgnn_vr_soundings_add";
  BGNN_TRY(require_vr_cloud(fn, x, y, z, n, x0, y0, base_res, base_height, base_width));
  BGNN_REQUIRE(state && unrefined, "%s: NULL argument", fn);
  BGNN_TRY(require_table(fn, table, total));
  BGNN_TRY(require_offered_total(fn, n, offered));
  BGNN_REQUIRE(aligned8(state), "%s: the state is not 8-byte aligned", fn);
  BGNN_REQUIRE(aligned8(unrefined), "%s: the unrefined counter is not 8-byte aligned", fn);
  const VRGeometry geo = {x0, y0, base_res, base_height, base_width, total};
  return launch_sounding_pass(fn, ctx, x, y, z, n, VRAddress{geo, static_cast<const VRLayoutEntry *>(table), unrefined},
                              FileSink{static_cast<char *>(state)});
}

extern "C" int bgnn_vr_soundings_stage(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0, double y0,
                                       double base_res, int64_t base_height, int64_t base_width, const void *table, int64_t total,
                                       int64_t offered, int64_t capacity, void *stage, int64_t *unrefined) {
  const char *fn = "bgnn_vr_soundings_stage";
  BGNN_TRY(require_vr_cloud(fn, x, y, z, n, x0, y0, base_res, base_height, base_width));
  BGNN_REQUIRE(stage && unrefined, "%s: NULL argument", fn);
  BGNN_TRY(require_table(fn, table, total));
  BGNN_TRY(require_capacity(fn, capacity));
  BGNN_TRY(require_offered_capacity(fn, n, offered, capacity));
  BGNN_REQUIRE(aligned8(stage), "%s: the stage is not 8-byte aligned", fn);
  BGNN_REQUIRE(aligned8(unrefined), "%s: the unrefined counter is not 8-byte aligned", fn);
  const VRGeometry geo = {x0, y0, base_res, base_height, base_width, total};
  BGNN_REQUIRE(ctx, "%s: NULL context", fn);
  if (n == 0) return BGNN_OK;
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const dim3 g(capped_grid((n + PASS_TILE - 1) / PASS_TILE, PLANE_MAX_GRID)), b(VR_THREADS);
  hipLaunchKernelGGL(vr_stage, g, b, 0, ctx->stream, x, y, z, n, geo, static_cast<const VRLayoutEntry *>(table), static_cast<char *>(stage),
                     offered, unrefined);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

extern "C" int bgnn_vr_soundings_flag(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0, double y0,
                                      double base_res, int64_t base_height, int64_t base_width, const void *table, int64_t total,
                                      const int64_t *center2, const int64_t *limit, uint8_t *flags) {
  const char *fn = "bgnn_vr_soundings_flag";
  BGNN_TRY(require_vr_cloud(fn, x, y, z, n, x0, y0, base_res, base_height, base_width));
  BGNN_REQUIRE(center2 && limit && (n == 0 || flags), "%s: NULL argument", fn);
  BGNN_TRY(require_table(fn, table, total));
  BGNN_REQUIRE(aligned8(center2) && aligned8(limit), "%s: center2 or limit is not 8-byte aligned", fn);
  const VRGeometry geo = {x0, y0, base_res, base_height, base_width, total};
  return launch_sounding_pass(fn, ctx, x, y, z, n, VRAddress{geo, static_cast<const VRLayoutEntry *>(table), nullptr},      // (no counters)
                              FlagSink{center2, limit, flags});
}
