// Ground truth from a survey pair and model evaluation (include/bgnn_eval.h): the two steps of the reference's workflow around
// training and inference, on planes that stay in HBM.
//
// Ground truth: the median of (noisy - clean) over the valid cells is an exact radix selection (radix_select.h, the implementation
// the noise analysis selects its order statistics with: here two ranks, int64 counts) over the order-preserving uint32 image of the
// float32 difference, in digits of 11, 11 and 10 bits.
//   gt_first_pass     reads both depth planes (8 B / cell), writes the raw difference into the `difference` plane (NaN = invalid,
//                     4 B / cell) and counts the top digit
//   gt_refine_pass    re-reads the raw difference (4 B / cell) and counts the next digit of the keys under the current prefixes:
//                     one histogram while both middle ranks share a prefix, two once they have parted (at any level)
//   gt_select         one workgroup: select_digit narrows prefix and rank of both ranks; the first level sets the ranks
//                     (n - 1) / 2 and n / 2 from the total; after the last level the prefixes are the two keys, and the offset is
//                     formed as numpy's mean of two float32 does
//   gt_label_pass     difference = raw - offset, labels, masked uncertainty (4-8 B in, 8-12 B out per cell) and the per-workgroup
//                     partials of the statistics (block_reduce); gt_finish adds them in workgroup order
// All passes are HBM-bound streams.
//
// Evaluation: eval_pass counts every integer of compute_metrics as wave ballots (28 per 64 cells, scalar adds), sums the three
// float64 confidence terms per thread in a fixed order, and leaves one partial row per workgroup; eval_finish adds the rows in
// workgroup order into the accumulator block.
//
// Compiled with -ffp-contract=off: the subtraction, the offset's add-then-halve and the float64 squares round as written.
#include <type_traits>

#include "bgnn_internal.h"
#include "radix_select.h"
#include "../../include/bgnn_eval.h"

namespace bgnn {

constexpr int EV_THREADS = BLOCK_THREADS;
constexpr int EV_ITEMS = 4;                          // consecutive cells per thread and step: one 16-byte load per plane
constexpr int EV_TILE = EV_THREADS * EV_ITEMS;
constexpr int EV_MAX_GRID = 2048;                    // 256 CUs x 8 workgroups
constexpr int EV_WAVES = EV_THREADS / 64;

// the grid of every streaming pass: a function of `cells` alone
static inline int stream_grid(int64_t cells) { return capped_grid((cells + EV_TILE - 1) / EV_TILE, EV_MAX_GRID); }

// ---- ground truth ----------------------------------------------------------------------------------------------------
using GtDigits = Digits<11, 11, 10>;
static_assert(GtDigits::covers<uint32_t>(), "the three levels cover the key");
using GtState = SelectState<2, uint32_t>;            // the lower and the upper middle rank
// workspace: int64 histograms (a pair may exceed 2^32 cells) [level 0 | level 1 x 2 groups | level 2 x 2 groups], the selection
// state, the partials
constexpr int gt_hist_word(int level) {
  int w = 0;
  for (int l = 0; l < level; ++l) w += (l == 0 ? 1 : 2) << GtDigits::width(l);
  return w;
}
constexpr int GT_HIST_WORDS = gt_hist_word(GtDigits::N);

struct GtPartial {           // one per workgroup of gt_label_pass
  double noise_abs_sum, seafloor_sum;
  int64_t noise, seafloor;
  float noise_abs_max;
  int32_t pad;
};
static_assert(sizeof(GtPartial) == 40, "partial row");

constexpr size_t GT_STATE_OFFSET = (size_t)GT_HIST_WORDS * 8;
constexpr size_t GT_PARTIAL_OFFSET = GT_STATE_OFFSET + sizeof(GtState);

template <bool VEC, typename T>
__device__ __forceinline__ void load_items(const T *p, int64_t i, int64_t n, T (&v)[EV_ITEMS], T fill) {
  static_assert(sizeof(T) == 4 && EV_ITEMS == 4, "one 16-byte access");
  if (VEC && i + EV_ITEMS <= n) {
    const uint4 t = *reinterpret_cast<const uint4 *>(p + i);
    const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int k = 0; k < EV_ITEMS; ++k) __builtin_memcpy(&v[k], &w[k], 4);
  } else {
#pragma unroll
    for (int k = 0; k < EV_ITEMS; ++k) v[k] = i + k < n ? p[i + k] : fill;
  }
}

template <bool VEC, typename T>
__device__ __forceinline__ void store_items(T *p, int64_t i, int64_t n, const T (&v)[EV_ITEMS]) {
  if (VEC && i + EV_ITEMS <= n) {
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < EV_ITEMS; ++k) __builtin_memcpy(&w[k], &v[k], 4);
    *reinterpret_cast<uint4 *>(p + i) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int k = 0; k < EV_ITEMS; ++k)
      if (i + k < n) p[i + k] = v[k];
  }
}

template <bool VEC>
__global__ __launch_bounds__(EV_THREADS) void gt_first_pass(const float *__restrict__ clean, const float *__restrict__ noisy,
                                                            int64_t cells, float nodata, float *__restrict__ raw_out,
                                                            int64_t *__restrict__ hist) {
  constexpr int BINS = 1 << GtDigits::width(0);
  __shared__ int32_t lds[BINS];
  for (int b = threadIdx.x; b < BINS; b += EV_THREADS) lds[b] = 0;
  __syncthreads();
  const float nan = __uint_as_float(0x7FC00000u);
  for (int64_t base = (int64_t)blockIdx.x * EV_TILE; base < cells; base += (int64_t)gridDim.x * EV_TILE) {
    const int64_t i = base + (int64_t)threadIdx.x * EV_ITEMS;
    float c[EV_ITEMS], z[EV_ITEMS], raw[EV_ITEMS];
    load_items<VEC>(clean, i, cells, c, nan);
    load_items<VEC>(noisy, i, cells, z, nan);
    bool ok[EV_ITEMS];
#pragma unroll
    for (int k = 0; k < EV_ITEMS; ++k) {
      ok[k] = finite_bits(c[k]) && finite_bits(z[k]) && c[k] != nodata && z[k] != nodata;
      raw[k] = ok[k] ? z[k] - c[k] : nan;      // finite operands never give NaN: NaN marks the invalid cell from here on
    }
    store_items<VEC>(raw_out, i, cells, raw);
#pragma unroll
    for (int k = 0; k < EV_ITEMS; ++k) hist_add(lds, ok[k], order_key(raw[k]) >> GtDigits::shift(0));
  }
  __syncthreads();
  hist_flush(lds, BINS, hist);
}

template <bool VEC, int LEVEL>
__global__ __launch_bounds__(EV_THREADS) void gt_refine_pass(const float *__restrict__ raw_in, int64_t cells,
                                                             const GtState *__restrict__ sel, int64_t *__restrict__ hist) {
  using Counter = DigitCounter<2, uint32_t, GtDigits::shift(LEVEL), GtDigits::width(LEVEL)>;
  __shared__ int32_t lds[2 * Counter::BINS];
  Counter counter;
  counter.init(sel, lds);
  const float nan = __uint_as_float(0x7FC00000u);
  for (int64_t base = (int64_t)blockIdx.x * EV_TILE; base < cells; base += (int64_t)gridDim.x * EV_TILE) {
    const int64_t i = base + (int64_t)threadIdx.x * EV_ITEMS;
    float raw[EV_ITEMS];
    load_items<VEC>(raw_in, i, cells, raw, nan);
#pragma unroll
    for (int k = 0; k < EV_ITEMS; ++k) counter.add(raw[k] == raw[k], order_key(raw[k]));
  }
  counter.flush(hist);
}

// One workgroup per level.  Level 0: the ranks from the total.  The last level: the prefixes are the keys and the offset is formed.
template <int LEVEL>
__global__ __launch_bounds__(EV_THREADS) void gt_select(const int64_t *__restrict__ hist, GtState *sel, char *stats) {
  __shared__ SelectScratch<2, uint32_t> sh;
  select_digit<LEVEL == 0, GtDigits::width(LEVEL)>(hist, sel, sh, 2, [](const int64_t *part, int64_t *rank) {
    const int64_t n = part[EV_THREADS];
    if (n > 0) { rank[0] = (n - 1) / 2; rank[1] = n / 2; }
  });
  if (LEVEL == GtDigits::N - 1 && threadIdx.x == 0) {
    const GtState &o = sh.out;
    const int64_t n = o.rank0[0] < 0 ? 0 : o.rank0[0] + o.rank0[1] + 1;      // (n - 1) / 2 + n / 2 = n - 1
    float offset = __uint_as_float(0x7FC00000u);
    if (n > 0) {
      const float a = key_value(o.prefix[0]), b = key_value(o.prefix[1]);
      offset = (n & 1) ? a : (a + b) / 2.0f;                   // numpy: add.reduce in float32, then the division by the count
    }
    *reinterpret_cast<float *>(stats + BGNN_GT_STATS_OFFSET) = offset;
    *reinterpret_cast<int64_t *>(stats + BGNN_GT_STATS_VALID) = n;
  }
}

template <bool VEC>
__global__ __launch_bounds__(EV_THREADS) void gt_label_pass(float *__restrict__ difference, const float *__restrict__ unc_in,
                                                            float *__restrict__ unc_out, int32_t *__restrict__ labels, int64_t cells,
                                                            float threshold, const char *__restrict__ stats,
                                                            GtPartial *__restrict__ partials) {
  const float offset = *reinterpret_cast<const float *>(stats + BGNN_GT_STATS_OFFSET);      // (gt_select of the last level)
  const float nan = __uint_as_float(0x7FC00000u);
  double noise_sum = 0.0, sea_sum = 0.0;
  float noise_max = 0.0f;
  uint32_t n_noise = 0, n_sea = 0;                             // (per thread: cells / threads of the grid, far below 2^32)
  for (int64_t base = (int64_t)blockIdx.x * EV_TILE; base < cells; base += (int64_t)gridDim.x * EV_TILE) {
    const int64_t i = base + (int64_t)threadIdx.x * EV_ITEMS;
    float raw[EV_ITEMS], d[EV_ITEMS];
    int32_t lab[EV_ITEMS];
    load_items<VEC>(difference, i, cells, raw, nan);
#pragma unroll
    for (int k = 0; k < EV_ITEMS; ++k) {
      const bool ok = raw[k] == raw[k];
      d[k] = ok ? raw[k] - offset : nan;
      const float mag = fabsf(d[k]);
      const bool noise = ok && mag > threshold;
      lab[k] = ok ? (noise ? 2 : 0) : -1;
      if (i + k < cells && ok) {
        if (noise) {
          noise_sum += (double)mag; noise_max = mag > noise_max ? mag : noise_max; ++n_noise;
        } else {
          sea_sum += (double)d[k]; ++n_sea;
        }
      }
    }
    store_items<VEC>(difference, i, cells, d);
    store_items<VEC>(labels, i, cells, lab);
    if (unc_out) {
      float u[EV_ITEMS];
      load_items<VEC>(unc_in, i, cells, u, nan);
#pragma unroll
      for (int k = 0; k < EV_ITEMS; ++k) u[k] = lab[k] >= 0 ? u[k] : nan;
      store_items<VEC>(unc_out, i, cells, u);
    }
  }
  // the workgroup's partial: a fixed tree over the threads
  __shared__ int64_t red[EV_THREADS];
  const auto later = [](float a, float b) { return b > a ? b : a; };
  GtPartial p{};
  p.noise_abs_sum = block_reduce(noise_sum, red, SumOp());
  p.seafloor_sum = block_reduce(sea_sum, red, SumOp());
  p.noise_abs_max = block_reduce(noise_max, red, later);
  p.noise = block_reduce((int64_t)n_noise, red, SumOp());
  p.seafloor = block_reduce((int64_t)n_sea, red, SumOp());
  if (threadIdx.x == 0) partials[blockIdx.x] = p;
}

// The sum of src[0], src[stride], ... (n terms) in ascending order, formed by one wave: lane l adds the run [32 l, 32 l + 32),
// lane 0 adds the runs.  A fixed association for a given n.  Called by every thread of the workgroup (one barrier inside); a
// wave that sums nothing passes src = nullptr.  lane_sums: 64 doubles of LDS per summing wave.  Lane 0 of the wave holds the result.
constexpr int EV_RUN = EV_MAX_GRID / 64;
__device__ __forceinline__ double ordered_sum(const double *src, int stride, int n, double *lane_sums) {
  const int lane = threadIdx.x & 63;
  if (src) {
    double run = 0.0;
    for (int k = lane * EV_RUN; k < (lane + 1) * EV_RUN && k < n; ++k) run += src[(int64_t)k * stride];
    lane_sums[lane] = run;
  }
  __syncthreads();
  double total = 0.0;
  if (src && lane == 0)
    for (int l = 0; l * EV_RUN < n; ++l) total += lane_sums[l];
  return total;
}

__global__ __launch_bounds__(EV_THREADS) void gt_finish(const GtPartial *__restrict__ partials, int n, char *stats) {
  __shared__ double lane_sums[2][64];
  __shared__ int64_t red[EV_THREADS];
  static_assert(sizeof(GtPartial) % 8 == 0 && offsetof(GtPartial, seafloor_sum) == 8, "the float64 sums lead the partial row");
  const int t = threadIdx.x;
  int64_t nn = 0, ns = 0;
  float mx = 0.0f;                                             // (magnitudes: no NaN, so the maximum is the same in any order)
  for (int k = t; k < n; k += EV_THREADS) {
    nn += partials[k].noise; ns += partials[k].seafloor;
    mx = partials[k].noise_abs_max > mx ? partials[k].noise_abs_max : mx;
  }
  nn = block_reduce(nn, red, SumOp());
  ns = block_reduce(ns, red, SumOp());
  mx = block_reduce(mx, red, [](float a, float b) { return b > a ? b : a; });
  if (t == 128) {
    *reinterpret_cast<int64_t *>(stats + BGNN_GT_STATS_NOISE) = nn;
    *reinterpret_cast<int64_t *>(stats + BGNN_GT_STATS_SEAFLOOR) = ns;
    *reinterpret_cast<float *>(stats + BGNN_GT_STATS_NOISE_ABS_MAX) = mx;
  }
  const int j = t >> 6;                                        // the two float64 sums, a wave each
  const double *src = j < 2 ? reinterpret_cast<const double *>(partials) + j : nullptr;
  const double total = ordered_sum(src, (int)(sizeof(GtPartial) / 8), n, lane_sums[j & 1]);
  if (j < 2 && (t & 63) == 0)
    *reinterpret_cast<double *>(stats + (j == 0 ? BGNN_GT_STATS_NOISE_ABS_SUM : BGNN_GT_STATS_SEAFLOOR_SUM)) = total;
}

// ---- evaluation ------------------------------------------------------------------------------------------------------
constexpr int EVAL_INTS = 2 + 16 + 2 * BGNN_EVAL_THRESHOLDS;      // total, correct, confusion, covered, covered_correct
constexpr int EVAL_SUMS = 4;                                      // conf_sum, conf_sq, conf_correct_sum, conf_incorrect_sum
constexpr int EVAL_ROW_WORDS = 32;                                // one partial row: EVAL_INTS int64, then the float64 sums
static_assert(EVAL_INTS + EVAL_SUMS == EVAL_ROW_WORDS, "partial row");
static_assert(BGNN_EVAL_ACC_CONFUSION == 16 && BGNN_EVAL_ACC_COVERED == 16 + 16 * 8 && BGNN_EVAL_ACC_COVERED_CORRECT == BGNN_EVAL_ACC_COVERED + 40 &&
                  BGNN_EVAL_ACC_CONF_SUM == 8 * EVAL_INTS && BGNN_EVAL_ACC_CONF_INCORRECT_SUM == BGNN_EVAL_ACC_CONF_SUM + 24 &&
                  BGNN_EVAL_ACC_CONF_CELLS == 8 * EVAL_ROW_WORDS && BGNN_EVAL_ACC_BYTES == BGNN_EVAL_ACC_CONF_CELLS + 8,
              "block layout: a partial row is in the block's order");

struct EvalThresholds { float t[BGNN_EVAL_THRESHOLDS]; };

__device__ __forceinline__ uint32_t wave_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

template <bool VEC, bool CONF>
__global__ __launch_bounds__(EV_THREADS) void eval_pass(const int32_t *__restrict__ labels, const float *__restrict__ pred,
                                                        const float *__restrict__ conf, int64_t cells, EvalThresholds thr,
                                                        int64_t *__restrict__ rows) {
  uint32_t cnt[EVAL_INTS];                                     // wave-uniform: every add is a ballot's population count
#pragma unroll
  for (int k = 0; k < EVAL_INTS; ++k) cnt[k] = 0;
  double sum = 0.0, sq = 0.0, csum = 0.0, isum = 0.0;
  const float nan = __uint_as_float(0x7FC00000u);
  for (int64_t base = (int64_t)blockIdx.x * EV_TILE; base < cells; base += (int64_t)gridDim.x * EV_TILE) {
    const int64_t i = base + (int64_t)threadIdx.x * EV_ITEMS;
    int32_t lab[EV_ITEMS];
    float p[EV_ITEMS], c[EV_ITEMS];
    load_items<VEC>(labels, i, cells, lab, (int32_t)-1);
    load_items<VEC>(pred, i, cells, p, nan);
    if (CONF) load_items<VEC>(conf, i, cells, c, nan);
#pragma unroll
    for (int k = 0; k < EV_ITEMS; ++k) {
      const bool counted = lab[k] >= 0 && p[k] >= 0.0f && finite_bits(p[k]);
      const double pt = trunc((double)p[k]);
      const bool correct = counted && pt == (double)lab[k];
      const int row = lab[k] < 3 ? lab[k] : 3;
      const int col = p[k] < 3.0f ? (int)p[k] : 3;             // (only read where counted: 0 <= p < 3 there)
      cnt[0] += wave_count(counted);
      cnt[1] += wave_count(correct);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) cnt[2 + r * 4 + q] += wave_count(counted && row == r && col == q);
      if (CONF) {
#pragma unroll
        for (int j = 0; j < BGNN_EVAL_THRESHOLDS; ++j) {
          const bool cov = counted && c[k] >= thr.t[j];
          cnt[18 + j] += wave_count(cov);
          cnt[18 + BGNN_EVAL_THRESHOLDS + j] += wave_count(cov && correct);
        }
        if (counted) {
          const double e = (double)c[k] - 0.5;
          sum += e; sq += e * e;
          if (correct) csum += e; else isum += e;
        }
      }
    }
  }
  __shared__ uint32_t w_cnt[EV_WAVES][EVAL_INTS];
  __shared__ double r_sum[EV_THREADS], r_sq[EV_THREADS], r_csum[EV_THREADS], r_isum[EV_THREADS];
  const int t = threadIdx.x;
  if ((t & 63) == 0) {
#pragma unroll
    for (int k = 0; k < EVAL_INTS; ++k) w_cnt[t >> 6][k] = cnt[k];
  }
  r_sum[t] = sum; r_sq[t] = sq; r_csum[t] = csum; r_isum[t] = isum;
  __syncthreads();
  for (int w = EV_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) { r_sum[t] += r_sum[t + w]; r_sq[t] += r_sq[t + w]; r_csum[t] += r_csum[t + w]; r_isum[t] += r_isum[t + w]; }
    __syncthreads();
  }
  int64_t *row = rows + (int64_t)blockIdx.x * EVAL_ROW_WORDS;
  if (t < EVAL_INTS) {
    int64_t v = 0;
#pragma unroll
    for (int w = 0; w < EV_WAVES; ++w) v += (int64_t)w_cnt[w][t];
    row[t] = v;
  }
  if (t == 64) {
    double *f = reinterpret_cast<double *>(row + EVAL_INTS);
    f[0] = r_sum[0]; f[1] = r_sq[0]; f[2] = r_csum[0]; f[3] = r_isum[0];
  }
}

// 1024 threads: thread t adds integer word (t & 31) of the rows (t >> 5), (t >> 5) + 32, ...: a row is one coalesced 256-byte read
constexpr int EF_THREADS = 1024, EF_GROUPS = EF_THREADS / EVAL_ROW_WORDS;

template <bool CONF>
__global__ __launch_bounds__(EF_THREADS) void eval_finish(const int64_t *__restrict__ rows, int n, char *acc) {
  __shared__ double lane_sums[EVAL_SUMS][64];
  __shared__ int64_t part[EF_GROUPS][EVAL_ROW_WORDS];
  const int t = threadIdx.x, c = t & (EVAL_ROW_WORDS - 1), g = t / EVAL_ROW_WORDS;
  int64_t v = 0;
  if (c < EVAL_INTS)
    for (int k = g; k < n; k += EF_GROUPS) v += rows[(int64_t)k * EVAL_ROW_WORDS + c];
  part[g][c] = v;
  // the float64 sums, a wave each (waves 1 .. EVAL_SUMS; the barrier inside covers part[])
  const int j = (t >> 6) - 1;
  const bool sums = CONF && j >= 0 && j < EVAL_SUMS;
  const double *src = sums ? reinterpret_cast<const double *>(rows + EVAL_INTS + j) : nullptr;
  const double total = ordered_sum(src, EVAL_ROW_WORDS, n, lane_sums[sums ? j : 0]);
  if (sums && (t & 63) == 0) *reinterpret_cast<double *>(acc + BGNN_EVAL_ACC_CONF_SUM + 8 * j) += total;
  if (t < EVAL_INTS && (CONF || t < 18)) {                      // (18 ..: covered, covered_correct)
    int64_t sum = 0;
    for (int k = 0; k < EF_GROUPS; ++k) sum += part[k][t];
    *reinterpret_cast<int64_t *>(acc + 8 * t) += sum;
    if (CONF && t == 0) *reinterpret_cast<int64_t *>(acc + BGNN_EVAL_ACC_CONF_CELLS) += sum;
  }
}

static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_ground_truth_workspace_bytes(int64_t cells) {
  if (cells < 0) return 0;
  const size_t bytes = GT_PARTIAL_OFFSET + (size_t)stream_grid(cells) * sizeof(GtPartial);
  return align256(bytes);
}

extern "C" int bgnn_ground_truth_build(bgnn_ctx *ctx, const float *clean, const float *noisy, const float *noisy_unc, int64_t cells,
                                       double nodata, double noise_threshold, void *ws, size_t ws_bytes, int32_t *labels,
                                       float *difference, float *unc_out, void *stats) {
  BGNN_REQUIRE(ctx && clean && noisy && ws && labels && difference && stats, "bgnn_ground_truth_build: NULL argument");
  BGNN_REQUIRE(!unc_out || noisy_unc, "bgnn_ground_truth_build: unc_out without noisy_unc");
  BGNN_REQUIRE(cells >= 0, "bgnn_ground_truth_build: %lld cells", (long long)cells);
  BGNN_REQUIRE(ws_bytes >= bgnn_ground_truth_workspace_bytes(cells), "bgnn_ground_truth_build: workspace of %zu bytes, %zu needed",
               ws_bytes, bgnn_ground_truth_workspace_bytes(cells));
  BGNN_REQUIRE(((uintptr_t)ws & 7) == 0, "bgnn_ground_truth_build: the workspace is not 8-byte aligned");
  BGNN_REQUIRE(((uintptr_t)stats & 7) == 0, "bgnn_ground_truth_build: the statistics block is not 8-byte aligned");
  BGNN_REQUIRE(difference != clean && difference != noisy && difference != noisy_unc,
               "bgnn_ground_truth_build: the difference plane aliases an input");
  if (cells == 0) return BGNN_OK;
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  char *w = static_cast<char *>(ws);
  int64_t *hist = reinterpret_cast<int64_t *>(w);
  GtState *sel = reinterpret_cast<GtState *>(w + GT_STATE_OFFSET);
  GtPartial *partials = reinterpret_cast<GtPartial *>(w + GT_PARTIAL_OFFSET);
  char *st = static_cast<char *>(stats);
  const int grid = stream_grid(cells);
  const dim3 g(grid), b(EV_THREADS), one(1);
  const float nd = (float)nodata, thr = (float)noise_threshold;
  const float *unc_in = unc_out ? noisy_unc : nullptr;
  const bool vec = aligned16(clean) && aligned16(noisy) && aligned16(difference) && aligned16(labels) &&
                   (!unc_out || (aligned16(unc_in) && aligned16(unc_out)));
  hipStream_t s = ctx->stream;
  BGNN_HIP_CHECK(hipMemsetAsync(w, 0, GT_PARTIAL_OFFSET, s));
  const auto passes = [&](auto vec_flag) {                     // the seven launches, for aligned (VEC) or unaligned planes
    constexpr bool VEC = decltype(vec_flag)::value;
    hipLaunchKernelGGL(gt_first_pass<VEC>, g, b, 0, s, clean, noisy, cells, nd, difference, hist + gt_hist_word(0));
    hipLaunchKernelGGL(gt_select<0>, one, b, 0, s, hist + gt_hist_word(0), sel, st);
    hipLaunchKernelGGL((gt_refine_pass<VEC, 1>), g, b, 0, s, difference, cells, sel, hist + gt_hist_word(1));
    hipLaunchKernelGGL(gt_select<1>, one, b, 0, s, hist + gt_hist_word(1), sel, st);
    hipLaunchKernelGGL((gt_refine_pass<VEC, 2>), g, b, 0, s, difference, cells, sel, hist + gt_hist_word(2));
    hipLaunchKernelGGL(gt_select<2>, one, b, 0, s, hist + gt_hist_word(2), sel, st);
    hipLaunchKernelGGL(gt_label_pass<VEC>, g, b, 0, s, difference, unc_in, unc_out, labels, cells, thr, st, partials);
  };
  if (vec) passes(std::true_type{});
  else passes(std::false_type{});
  hipLaunchKernelGGL(gt_finish, one, b, 0, s, partials, grid, st);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

extern "C" size_t bgnn_eval_workspace_bytes(int64_t cells) {
  if (cells < 0) return 0;
  return (size_t)stream_grid(cells) * EVAL_ROW_WORDS * 8;
}

extern "C" int bgnn_eval_reset(bgnn_ctx *ctx, void *acc) {
  BGNN_REQUIRE(ctx && acc, "bgnn_eval_reset: NULL argument");
  BGNN_REQUIRE(((uintptr_t)acc & 7) == 0, "bgnn_eval_reset: the accumulator block is not 8-byte aligned");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  BGNN_HIP_CHECK(hipMemsetAsync(acc, 0, BGNN_EVAL_ACC_BYTES, ctx->stream));
  return BGNN_OK;
}

extern "C" int bgnn_eval_accumulate(bgnn_ctx *ctx, const int32_t *labels, const float *pred, const float *confidence, int64_t cells,
                                    void *ws, size_t ws_bytes, void *acc) {
  BGNN_REQUIRE(ctx && labels && pred && ws && acc, "bgnn_eval_accumulate: NULL argument");
  BGNN_REQUIRE(cells >= 0, "bgnn_eval_accumulate: %lld cells", (long long)cells);
  BGNN_REQUIRE(ws_bytes >= bgnn_eval_workspace_bytes(cells), "bgnn_eval_accumulate: workspace of %zu bytes, %zu needed", ws_bytes,
               bgnn_eval_workspace_bytes(cells));
  BGNN_REQUIRE(((uintptr_t)ws & 7) == 0, "bgnn_eval_accumulate: the workspace is not 8-byte aligned");
  BGNN_REQUIRE(((uintptr_t)acc & 7) == 0, "bgnn_eval_accumulate: the accumulator block is not 8-byte aligned");
  if (cells == 0) return BGNN_OK;
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  EvalThresholds thr;
  const double t[BGNN_EVAL_THRESHOLDS] = {0.5, 0.6, 0.7, 0.8, 0.9};
  for (int j = 0; j < BGNN_EVAL_THRESHOLDS; ++j) thr.t[j] = (float)t[j];
  const int grid = stream_grid(cells);
  const dim3 g(grid), b(EV_THREADS), one(1);
  int64_t *rows = static_cast<int64_t *>(ws);
  char *a = static_cast<char *>(acc);
  const bool vec = aligned16(labels) && aligned16(pred) && (!confidence || aligned16(confidence));
  hipStream_t s = ctx->stream;
  if (confidence) {
    if (vec) hipLaunchKernelGGL((eval_pass<true, true>), g, b, 0, s, labels, pred, confidence, cells, thr, rows);
    else hipLaunchKernelGGL((eval_pass<false, true>), g, b, 0, s, labels, pred, confidence, cells, thr, rows);
    hipLaunchKernelGGL(eval_finish<true>, one, dim3(EF_THREADS), 0, s, rows, grid, a);
  } else {
    if (vec) hipLaunchKernelGGL((eval_pass<true, false>), g, b, 0, s, labels, pred, confidence, cells, thr, rows);
    else hipLaunchKernelGGL((eval_pass<false, false>), g, b, 0, s, labels, pred, confidence, cells, thr, rows);
    hipLaunchKernelGGL(eval_finish<false>, one, dim3(EF_THREADS), 0, s, rows, grid, a);
  }
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
