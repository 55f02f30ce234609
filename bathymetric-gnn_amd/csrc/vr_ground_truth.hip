// Ground truth at native resolution from a clean / noisy VR BAG pair (include/bgnn_vrtruth.h): both files' refinement records in
// HBM, a host pair table staged into the workspace, flat per-cell outputs in the noisy file's iteration order.
//
//   vt_label_pass    a workgroup owns a contiguous run of output cells, in tiles of 1024.  It finds the grid of its first cell once
//                    (binary search of the table's offsets) and walks: per tile the offsets of the grids that meet the tile are
//                    staged in LDS relative to the tile, 256 per round until they cover it; a thread places the first of its four
//                    consecutive cells among them by binary search in LDS and steps on for the other three.  Reads 8 B (noisy
//                    record) + 4-8 B (clean depth: half of a record, a whole 8-byte sector share) per cell, writes 17 B: memory-bound.
//                    Counts the top digit of the noise magnitudes for the selection, the per-grid counts in LDS (one 64-bit integer
//                    atomic per count, grid and tile), and leaves the workgroup's partial of the statistics.  18 KiB of LDS: the
//                    eight workgroups per CU of a full grid run together (at 28 KiB five did, and the other three behind them)
//   vt_refine_pass   re-reads labels and difference (8 B / cell) and counts the next digit of the magnitudes under the current
//                    prefixes (radix_select.h); returns at once when there is no noise cell
//   vt_select        one workgroup per level: select_digit; the last level forms the float64 median
//   vt_finish        adds the partials in workgroup order
//
// Compiled with -ffp-contract=off: nd - cd and the float64 mean of two ranks round as written.
#include "bgnn_internal.h"
#include "radix_select.h"
#include "../../include/bgnn_vrtruth.h"

namespace bgnn {
namespace {

constexpr int VT_THREADS = BLOCK_THREADS;
constexpr int VT_ITEMS = 4;                          // consecutive cells per thread: one 16-byte store per plane
constexpr int VT_TILE = BGNN_VT_TILE_CELLS;
constexpr int VT_MAX_GRID = 2048;                    // 256 CUs x 8 workgroups
constexpr int VT_RUN = VT_MAX_GRID / 64;             // partials per lane of the finishing wave
// offsets staged per tile: a grid has at least one cell, so entry VT_TILE + 1 past the tile's first grid lies beyond the tile
constexpr int VT_STAGE = VT_TILE + 2 * VT_THREADS;
static_assert(VT_TILE == VT_THREADS * VT_ITEMS && BGNN_VT_PAIR_BYTES == sizeof(bgnn_vr_pair) && BGNN_VT_COUNTS == 4, "tile and table");

using VtDigits = Digits<11, 11, 10>;
static_assert(VtDigits::covers<uint32_t>(), "the three levels cover the key");
using VtState = SelectState<2, uint32_t>;            // the lower and the upper middle rank
constexpr int vt_hist_word(int level) {
  int w = 0;
  for (int l = 0; l < level; ++l) w += (l == 0 ? 1 : 2) << VtDigits::width(l);
  return w;
}
constexpr int VT_HIST_WORDS = vt_hist_word(VtDigits::N);

struct VtPartial {           // one per workgroup of vt_label_pass
  double noise_abs_sum;
  int64_t noise, seafloor;
  float noise_abs_max;
  int32_t pad;
};
static_assert(sizeof(VtPartial) == 32, "partial row");

constexpr size_t VT_STATE_OFFSET = (size_t)VT_HIST_WORDS * 8;
constexpr size_t VT_PARTIAL_OFFSET = VT_STATE_OFFSET + sizeof(VtState);
static_assert(VT_PARTIAL_OFFSET % 8 == 0, "the partials are 8-byte aligned");

inline int vt_grid(int64_t total) { return capped_grid((total + VT_TILE - 1) / VT_TILE, VT_MAX_GRID); }
inline size_t vt_table_bytes(int64_t n_grids) { return align256((size_t)n_grids * BGNN_VT_PAIR_BYTES); }

__device__ __forceinline__ bool depth_ok(float d, float nodata) { return finite_bits(d) && d != nodata; }

template <bool UNC>
__global__ __launch_bounds__(VT_THREADS) void vt_label_pass(const float2 *__restrict__ noisy, const float2 *__restrict__ clean,
                                                            const bgnn_vr_pair *__restrict__ pairs, int64_t n_grids, int64_t total,
                                                            int64_t tiles_per_wg, float nodata, float threshold,
                                                            int32_t *__restrict__ labels, float *__restrict__ difference,
                                                            float *__restrict__ depth_out, float *__restrict__ unc_out,
                                                            uint8_t *__restrict__ mask, unsigned long long *grid_counts,
                                                            int64_t *__restrict__ hist, VtPartial *__restrict__ partials) {
  // 18 KiB of LDS, so that the eight workgroups a CU gets of a full grid are resident together
  constexpr int BINS = (1 << VtDigits::width(0)) / 2;            // a magnitude's key has its top bit set: the upper half of the digit
  __shared__ int32_t lds_hist[BINS];
  __shared__ int32_t rel[VT_STAGE];                  // staged offsets minus the tile's first cell, clamped to [-1, VT_TILE + 1]
  __shared__ uint32_t cnt[VT_STAGE];                 // per staged grid: cells labelled 0 | cells labelled 2 << 16 (at most 1024 each)
  __shared__ int64_t red[VT_THREADS];
  const int t = threadIdx.x;
  for (int b = t; b < BINS; b += VT_THREADS) lds_hist[b] = 0;
  const float nan = __uint_as_float(0x7FC00000u);
  const int64_t lo = (int64_t)blockIdx.x * tiles_per_wg * VT_TILE;
  const int64_t hi = lo + tiles_per_wg * VT_TILE < total ? lo + tiles_per_wg * VT_TILE : total;
  double noise_sum = 0.0;
  float noise_max = 0.0f;
  uint32_t n_noise = 0, n_sea = 0;                   // (per thread: at most its share of a run, far below 2^32)

  int64_t g0 = 0;                                    // the grid of the tile's first cell (uniform)
  if (lo < hi) {
    int64_t a = 0, b = n_grids;                      // pairs[a].out_offset <= lo < pairs[b].out_offset (b == n_grids: total)
    while (b - a > 1) {
      const int64_t mid = (a + b) >> 1;
      if (pairs[mid].out_offset <= lo) a = mid; else b = mid;
    }
    g0 = a;
  }
  for (int64_t base = lo; base < hi; base += VT_TILE) {
    const int len = (int)(hi - base < VT_TILE ? hi - base : VT_TILE);
    __syncthreads();                                 // (the previous tile's readers of rel / cnt are done; lds_hist is cleared)
    int staged = 0, last = 0;
    for (;;) {                                       // (uniform) 256 offsets per round until they reach the tile's end
      const int k = staged + t;
      const int64_t gi = g0 + k;
      if (gi <= n_grids) {
        const int64_t d = (gi < n_grids ? pairs[gi].out_offset : total) - base;
        rel[k] = d < -1 ? -1 : (d > VT_TILE + 1 ? VT_TILE + 1 : (int32_t)d);
        cnt[k] = 0;
      }
      staged += VT_THREADS;
      __syncthreads();
      last = n_grids - g0 < staged - 1 ? (int)(n_grids - g0) : staged - 1;
      if (rel[last] >= len || staged + VT_THREADS > VT_STAGE) break;
    }
    // entries 0 .. last; grid j of the stage is [rel[j], rel[j + 1]); rel[0] <= 0 and rel[last] >= len
    const int c0 = t * VT_ITEMS;
    const int cs = c0 < len ? c0 : len - 1;
    int j = 0;
    {
      int a = 0, b = last;                           // rel[a] <= cs < rel[b]
      while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (rel[mid] <= cs) a = mid; else b = mid;
      }
      j = a;
    }
    bool in[VT_ITEMS], paired[VT_ITEMS];
    int gj[VT_ITEMS];
    float2 nrec[VT_ITEMS];
    float cd[VT_ITEMS];
#pragma unroll
    for (int k = 0; k < VT_ITEMS; ++k) {
      const int c = c0 + k;
      in[k] = c < len && rel[last] > c;              // (the second test holds by construction: a guard for the loads below)
      nrec[k] = make_float2(nan, nan);
      cd[k] = nan;
      paired[k] = false;
      if (in[k]) {
        while (j + 1 < last && rel[j + 1] <= c) ++j;
        const bgnn_vr_pair p = pairs[g0 + j];
        const int64_t within = base + c - p.out_offset;         // 0 <= within < p.cells: the host checked the table
        nrec[k] = noisy[p.noisy_start + within];
        paired[k] = p.clean_start >= 0;
        if (paired[k]) cd[k] = clean[p.clean_start + within].x;
      }
      gj[k] = j;
    }
    float d[VT_ITEMS], nd[VT_ITEMS], nu[VT_ITEMS];
    int32_t lab[VT_ITEMS];
    uint32_t mask_word = 0;
#pragma unroll
    for (int k = 0; k < VT_ITEMS; ++k) {
      nd[k] = nrec[k].x; nu[k] = nrec[k].y;
      const bool ok = in[k] && paired[k] && depth_ok(nd[k], nodata) && depth_ok(cd[k], nodata);
      d[k] = paired[k] ? nd[k] - cd[k] : nan;
      const float mag = fabsf(d[k]);
      const bool noise = ok && mag > threshold;
      lab[k] = ok ? (noise ? 2 : 0) : -1;
      mask_word |= ok ? 1u << (8 * k) : 0u;
      if (ok) {
        atomicAdd(&cnt[gj[k]], noise ? 0x10000u : 1u);
        if (noise) { noise_sum += (double)mag; noise_max = mag > noise_max ? mag : noise_max; ++n_noise; }
        else ++n_sea;
      }
      hist_add(lds_hist, noise, (order_key(mag) >> VtDigits::shift(0)) & (BINS - 1));      // (whole waves: no lane has left)
    }
    const int64_t i = base + c0;
    if (c0 + VT_ITEMS <= len) {                      // (base is a multiple of the tile: i is a multiple of four)
      *reinterpret_cast<int4 *>(labels + i) = make_int4(lab[0], lab[1], lab[2], lab[3]);
      *reinterpret_cast<float4 *>(difference + i) = make_float4(d[0], d[1], d[2], d[3]);
      *reinterpret_cast<float4 *>(depth_out + i) = make_float4(nd[0], nd[1], nd[2], nd[3]);
      if (UNC) *reinterpret_cast<float4 *>(unc_out + i) = make_float4(nu[0], nu[1], nu[2], nu[3]);
      *reinterpret_cast<uint32_t *>(mask + i) = mask_word;
    } else {
#pragma unroll
      for (int k = 0; k < VT_ITEMS; ++k) {
        if (c0 + k < len) {
          labels[i + k] = lab[k]; difference[i + k] = d[k]; depth_out[i + k] = nd[k];
          if (UNC) unc_out[i + k] = nu[k];
          mask[i + k] = (uint8_t)((mask_word >> (8 * k)) & 1u);
        }
      }
    }
    __syncthreads();
    for (int k = t; k < last; k += VT_THREADS) {     // the staged grids' counts: valid, class 0, (class 1,) class 2
      const int32_t n0 = (int32_t)(cnt[k] & 0xFFFFu), n2 = (int32_t)(cnt[k] >> 16);
      if ((n0 | n2) != 0) {
        unsigned long long *row = grid_counts + (g0 + k) * BGNN_VT_COUNTS;
        atomicAdd(row, (unsigned long long)(n0 + n2));
        if (n0 != 0) atomicAdd(row + 1, (unsigned long long)n0);
        if (n2 != 0) atomicAdd(row + 3, (unsigned long long)n2);
      }
    }
    if (base + VT_TILE < hi) {                       // the grid of the next tile's first cell: rel[a] <= VT_TILE < rel[b]
      int a = 0, b = last;
      if (rel[last] <= VT_TILE) a = last;            // (the stage ends with the tile: the next grid starts the next tile)
      while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (rel[mid] <= VT_TILE) a = mid; else b = mid;
      }
      g0 += a;
    }
  }
  __syncthreads();
  hist_flush(lds_hist, BINS, hist + BINS);
  VtPartial p{};
  p.noise_abs_sum = block_reduce(noise_sum, red, SumOp());
  p.noise_abs_max = block_reduce(noise_max, red, [](float a, float b) { return b > a ? b : a; });
  p.noise = block_reduce((int64_t)n_noise, red, SumOp());
  p.seafloor = block_reduce((int64_t)n_sea, red, SumOp());
  if (t == 0) partials[blockIdx.x] = p;
}

template <int LEVEL>
__global__ __launch_bounds__(VT_THREADS) void vt_refine_pass(const int32_t *__restrict__ labels, const float *__restrict__ difference,
                                                             int64_t total, const VtState *__restrict__ sel,
                                                             int64_t *__restrict__ hist) {
  using Counter = DigitCounter<2, uint32_t, VtDigits::shift(LEVEL), VtDigits::width(LEVEL)>;
  __shared__ int32_t lds[2 * Counter::BINS];
  if (sel->ngroups == 0) return;                     // (uniform, before any barrier) no noise cell: nothing to select
  Counter counter;
  counter.init(sel, lds);
  for (int64_t base = (int64_t)blockIdx.x * VT_TILE; base < total; base += (int64_t)gridDim.x * VT_TILE) {
    const int64_t i = base + (int64_t)threadIdx.x * VT_ITEMS;
    int32_t lab[VT_ITEMS] = {-1, -1, -1, -1};
    float d[VT_ITEMS] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i + VT_ITEMS <= total) {
      const int4 l = *reinterpret_cast<const int4 *>(labels + i);
      const float4 v = *reinterpret_cast<const float4 *>(difference + i);
      lab[0] = l.x; lab[1] = l.y; lab[2] = l.z; lab[3] = l.w;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else {
#pragma unroll
      for (int k = 0; k < VT_ITEMS; ++k)
        if (i + k < total) { lab[k] = labels[i + k]; d[k] = difference[i + k]; }
    }
#pragma unroll
    for (int k = 0; k < VT_ITEMS; ++k) counter.add(lab[k] == 2, order_key(fabsf(d[k])));
  }
  counter.flush(hist);
}

// One workgroup per level.  Level 0: the ranks from the total.  The last level: the prefixes are the keys and the median is formed.
template <int LEVEL>
__global__ __launch_bounds__(VT_THREADS) void vt_select(const int64_t *__restrict__ hist, VtState *sel, char *stats) {
  __shared__ SelectScratch<2, uint32_t> sh;
  select_digit<LEVEL == 0, VtDigits::width(LEVEL)>(hist, sel, sh, 2, [](const int64_t *part, int64_t *rank) {
    const int64_t n = part[VT_THREADS];
    if (n > 0) { rank[0] = (n - 1) / 2; rank[1] = n / 2; }
  });
  if (LEVEL == VtDigits::N - 1 && threadIdx.x == 0) {
    const VtState &o = sh.out;
    const int64_t n = o.rank0[0] < 0 ? 0 : o.rank0[0] + o.rank0[1] + 1;      // (n - 1) / 2 + n / 2 = n - 1
    double median = __longlong_as_double(0x7FF8000000000000ll);
    if (n > 0) {
      const double a = (double)key_value(o.prefix[0]), b = (double)key_value(o.prefix[1]);
      median = (n & 1) ? a : (a + b) / 2.0;                                  // numpy.median of a float64 array
    }
    *reinterpret_cast<double *>(stats + BGNN_VT_STATS_NOISE_ABS_MEDIAN) = median;
  }
}

// The partials in workgroup order: lane l of wave 0 adds the run [32 l, 32 l + 32), lane 0 adds the runs.  A fixed association
// for a given n.
__global__ __launch_bounds__(VT_THREADS) void vt_finish(const VtPartial *__restrict__ partials, int n, char *stats) {
  __shared__ double lane_sums[64];
  __shared__ int64_t red[VT_THREADS];
  const int t = threadIdx.x;
  int64_t nn = 0, ns = 0;
  float mx = 0.0f;                                             // (magnitudes: no NaN, so the maximum is the same in any order)
  for (int k = t; k < n; k += VT_THREADS) {
    nn += partials[k].noise; ns += partials[k].seafloor;
    mx = partials[k].noise_abs_max > mx ? partials[k].noise_abs_max : mx;
  }
  nn = block_reduce(nn, red, SumOp());
  ns = block_reduce(ns, red, SumOp());
  mx = block_reduce(mx, red, [](float a, float b) { return b > a ? b : a; });
  if (t < 64) {
    double run = 0.0;
    for (int k = t * VT_RUN; k < (t + 1) * VT_RUN && k < n; ++k) run += partials[k].noise_abs_sum;
    lane_sums[t] = run;
  }
  __syncthreads();
  if (t == 0) {
    double sum = 0.0;
    for (int l = 0; l * VT_RUN < n; ++l) sum += lane_sums[l];
    *reinterpret_cast<int64_t *>(stats + BGNN_VT_STATS_VALID) = nn + ns;
    *reinterpret_cast<int64_t *>(stats + BGNN_VT_STATS_NOISE) = nn;
    *reinterpret_cast<int64_t *>(stats + BGNN_VT_STATS_SEAFLOOR) = ns;
    *reinterpret_cast<double *>(stats + BGNN_VT_STATS_NOISE_ABS_SUM) = sum;
    *reinterpret_cast<float *>(stats + BGNN_VT_STATS_NOISE_ABS_MAX) = mx;
    *reinterpret_cast<int32_t *>(stats + BGNN_VT_STATS_NOISE_ABS_MAX + 4) = 0;
  }
}

// Every row of the pair table against the contract of the header.  On failure `row` names the first bad row.
const char *check_pairs(const bgnn_vr_pair *pairs, int64_t n_grids, int64_t total, int64_t n_noisy, int64_t n_clean, int64_t *row) {
  int64_t next = 0;
  for (int64_t g = 0; g < n_grids; ++g) {
    const bgnn_vr_pair &p = pairs[g];
    *row = g;
    if (p.cells < 1) return "has no cell";
    if (p.out_offset != next || p.cells > total - next) return "does not continue the outputs where the row before it ends";
    if (p.noisy_start < 0 || p.noisy_start > n_noisy || p.cells > n_noisy - p.noisy_start) return "leaves the noisy records";
    if (p.clean_start < -1) return "has a clean_start below -1";
    if (p.clean_start >= 0 && (p.clean_start > n_clean || p.cells > n_clean - p.clean_start)) return "leaves the clean records";
    next += p.cells;
  }
  *row = n_grids;
  return next == total ? nullptr : "rows do not cover total_cells";
}

}  // namespace
}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_vr_ground_truth_workspace_bytes(int64_t total_cells, int64_t n_grids) {
  if (total_cells < 0 || n_grids < 0) return 0;
  return vt_table_bytes(n_grids) + align256(VT_PARTIAL_OFFSET + (size_t)vt_grid(total_cells) * sizeof(VtPartial));
}

extern "C" int bgnn_vr_ground_truth(bgnn_ctx *ctx, const float *noisy, int64_t n_noisy, const float *clean, int64_t n_clean,
                                    const bgnn_vr_pair *pairs, int64_t n_grids, int64_t total_cells, double nodata,
                                    double noise_threshold, void *ws, size_t ws_bytes, int32_t *labels, float *difference,
                                    float *noisy_depth, float *uncertainty, uint8_t *mask, int64_t *grid_counts, void *stats) {
  const char *who = "bgnn_vr_ground_truth";
  BGNN_REQUIRE(ctx, "%s: NULL argument", who);
  BGNN_REQUIRE(n_noisy >= 0 && n_clean >= 0 && n_grids >= 0 && total_cells >= 0, "%s: %lld noisy and %lld clean records, %lld grids, %lld cells",
               who, (long long)n_noisy, (long long)n_clean, (long long)n_grids, (long long)total_cells);
  if (total_cells == 0) {
    BGNN_REQUIRE(n_grids == 0, "%s: %lld grids without a cell", who, (long long)n_grids);
    return BGNN_OK;
  }
  BGNN_REQUIRE(noisy && (clean || n_clean == 0) && pairs && ws && labels && difference && noisy_depth && mask && grid_counts && stats,
               "%s: NULL argument", who);
  BGNN_REQUIRE(n_grids >= 1, "%s: %lld cells in no grid", who, (long long)total_cells);
  BGNN_REQUIRE(((uintptr_t)noisy & 7) == 0 && ((uintptr_t)clean & 7) == 0, "%s: the records are not 8-byte aligned", who);
  BGNN_REQUIRE((((uintptr_t)labels | (uintptr_t)difference | (uintptr_t)noisy_depth | (uintptr_t)uncertainty) & 15) == 0,
               "%s: an output plane is not 16-byte aligned", who);
  BGNN_REQUIRE(((uintptr_t)mask & 3) == 0, "%s: the mask is not 4-byte aligned", who);
  BGNN_REQUIRE(((uintptr_t)grid_counts & 7) == 0 && ((uintptr_t)stats & 7) == 0, "%s: the count table or the statistics block is not 8-byte aligned", who);
  const void *outs[] = {labels, difference, noisy_depth, uncertainty, mask, grid_counts, stats, ws};
  for (const void *o : outs)
    BGNN_REQUIRE(!o || (o != (const void *)noisy && o != (const void *)clean), "%s: an output aliases a record array", who);
  int64_t bad = 0;
  const char *why = check_pairs(pairs, n_grids, total_cells, n_noisy, n_clean, &bad);
  BGNN_REQUIRE(!why, "%s: pair table, row %lld of %lld: %s", who, (long long)bad, (long long)n_grids, why);
  const size_t need = bgnn_vr_ground_truth_workspace_bytes(total_cells, n_grids);
  BGNN_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
  BGNN_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: the workspace is not 16-byte aligned", who);

  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  char *w = static_cast<char *>(ws);
  BGNN_TRY(ctx_upload(ctx, pairs, (size_t)n_grids * BGNN_VT_PAIR_BYTES, w));
  const bgnn_vr_pair *d_pairs = reinterpret_cast<const bgnn_vr_pair *>(w);
  char *sel_base = w + vt_table_bytes(n_grids);
  int64_t *hist = reinterpret_cast<int64_t *>(sel_base);
  VtState *sel = reinterpret_cast<VtState *>(sel_base + VT_STATE_OFFSET);
  VtPartial *partials = reinterpret_cast<VtPartial *>(sel_base + VT_PARTIAL_OFFSET);
  char *st = static_cast<char *>(stats);
  BGNN_HIP_CHECK(hipMemsetAsync(sel_base, 0, VT_PARTIAL_OFFSET, s));
  BGNN_HIP_CHECK(hipMemsetAsync(grid_counts, 0, (size_t)n_grids * BGNN_VT_COUNTS * sizeof(int64_t), s));
  const int64_t n_tiles = (total_cells + VT_TILE - 1) / VT_TILE;
  const int grid = vt_grid(total_cells);
  const int64_t tiles_per_wg = (n_tiles + grid - 1) / grid;
  const dim3 g(grid), b(VT_THREADS), one(1);
  const float2 *nz = reinterpret_cast<const float2 *>(noisy), *cl = reinterpret_cast<const float2 *>(clean);
  unsigned long long *gc = reinterpret_cast<unsigned long long *>(grid_counts);
  const float nd = (float)nodata, thr = (float)noise_threshold;
  if (uncertainty)
    hipLaunchKernelGGL(vt_label_pass<true>, g, b, 0, s, nz, cl, d_pairs, n_grids, total_cells, tiles_per_wg, nd, thr, labels,
                       difference, noisy_depth, uncertainty, mask, gc, hist + vt_hist_word(0), partials);
  else
    hipLaunchKernelGGL(vt_label_pass<false>, g, b, 0, s, nz, cl, d_pairs, n_grids, total_cells, tiles_per_wg, nd, thr, labels,
                       difference, noisy_depth, uncertainty, mask, gc, hist + vt_hist_word(0), partials);
  hipLaunchKernelGGL(vt_select<0>, one, b, 0, s, hist + vt_hist_word(0), sel, st);
  hipLaunchKernelGGL(vt_refine_pass<1>, g, b, 0, s, labels, difference, total_cells, sel, hist + vt_hist_word(1));
  hipLaunchKernelGGL(vt_select<1>, one, b, 0, s, hist + vt_hist_word(1), sel, st);
  hipLaunchKernelGGL(vt_refine_pass<2>, g, b, 0, s, labels, difference, total_cells, sel, hist + vt_hist_word(2));
  hipLaunchKernelGGL(vt_select<2>, one, b, 0, s, hist + vt_hist_word(2), sel, st);
  hipLaunchKernelGGL(vt_finish, one, b, 0, s, partials, grid, st);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
