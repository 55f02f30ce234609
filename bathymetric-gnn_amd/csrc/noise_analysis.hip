// Noise pattern analysis of a ground truth (include/bgnn_analysis.h): scripts/analyze_noise_patterns.py, analyze_ground_truth, on
// planes that stay in HBM.  A fixed sequence of launches on the context's stream; every grid is a function of rows and cols.
//
//   na_stream        labels, difference, noisy depth (12 B / cell): the counts, the depth bins, the float64 sums as per-workgroup
//                    partials, and the top 11 key bits of |difference| over the noise cells
//   na_refine<MAG>   two more histogram passes over labels and difference for the six ranks of median / p90 / p99 at once; the
//                    first of them also sums (|d| - mean)^2, the stable form of the variance
//   na_rough         clean depth through a 20 x 68 LDS halo: numpy's nanstd of the 5 x 5 window in float64 (two-pass), stored as
//                    one float64 per cell whose sign bit is the class (set: noise, clear: seafloor; NaN: neither, or no value),
//                    the class sums, and the top 11 bits of that key.  na_refine<ROUGH> x 5 narrows both classes' two middle ranks
//                    in one 64-bit key space: every noise key lies above every seafloor key
//   ccl_local .. ccl_stats   connected components of the noise mask, below; na_refine<SIZE> x 2 selects the median cluster size
//   na_select        one workgroup after every histogram pass: narrows prefix and rank of every rank (radix_select.h, select_digit)
//   na_finish        one workgroup: adds the partial rows in workgroup order into the result block
//
// Multi-rank radix selection: radix_select.h, the implementation the ground truth selects its median with; here up to six ranks
// and uint32 counts (cells are below 2^31).  This file keeps the streaming loops, the rule that sets each selection's ranks from the
// first level's totals, and what is written to the block after the last level.
//
// Connected components of the noise mask (4-connectivity, scipy.ndimage.label's default structure): component_label.h, with its
// invariant parent[i] <= i and the termination argument; no thread waits for another.
//   ccl_local    a 16 x 64 tile in LDS: the tile-local labelling of the noise cells.  Also the per-column noise / valid counts of
//                the tile (64 x 2 global integer adds)
//   label_merge, label_flatten<SizeOnly>   the unions across the tile borders; the sizes summed at the roots
//   ccl_stats    over the global roots (parent[i] == i): count, size sum, maximum, size bins, the top size bits
//
// Compiled with -ffp-contract=off: the float32 rank arithmetic of numpy's percentile and the float64 squares round as written.
#include "bgnn_internal.h"
#include "component_label.h"
#include "radix_select.h"
#include "../../include/bgnn_analysis.h"

namespace bgnn {
namespace {

constexpr int NA_THREADS = BLOCK_THREADS;
constexpr int NA_ITEMS = 4;                           // cells per thread and step of a streaming pass (each load coalesced)
constexpr int NA_CHUNK = NA_THREADS * NA_ITEMS;
constexpr int NA_RANKS = 6;
constexpr int HALO_R = TILE_R + 4, HALO_C = TILE_C + 4;
constexpr int ROW_WORDS = 40;                         // a partial row: 8-byte words

enum { SEL_MAG = 0, SEL_ROUGH = 1, SEL_SIZE = 2, SEL_COUNT = 3 };

// What each selection selects: its key, the key's digits (most significant first), its ranks
template <int SEL> struct Selection {                 // SEL_MAG: the bits of |difference|; SEL_SIZE: a cluster's cell count
  using Key = uint32_t;
  using D = Digits<11, 11, 10>;
  static constexpr int nranks = SEL == SEL_MAG ? 6 : 2;
};
template <> struct Selection<SEL_ROUGH> {             // the roughness plane's float64 words, the class in the sign bit
  using Key = uint64_t;
  using D = Digits<11, 11, 11, 11, 11, 9>;
  static constexpr int nranks = 4;
};
template <int SEL> using SelState = SelectState<NA_RANKS, typename Selection<SEL>::Key>;
constexpr int NA_BINS = 1 << 11;                      // of every selection's top digit, and the widest
constexpr int NA_LEVELS = Selection<SEL_ROUGH>::D::N;
static_assert(Selection<SEL_MAG>::D::covers<uint32_t>() && Selection<SEL_ROUGH>::D::covers<uint64_t>(), "the digits cover the key");
static_assert(sizeof(SelState<SEL_ROUGH>) <= 256 && Selection<SEL_MAG>::D::N <= NA_LEVELS, "workspace slots");

// workspace: [histograms | selection states] (cleared by one memset), the partial rows, then the three planes
constexpr size_t WS_LEVEL_WORDS = (size_t)NA_RANKS * NA_BINS;
constexpr size_t WS_SEL_WORDS = (size_t)NA_LEVELS * WS_LEVEL_WORDS;
constexpr size_t WS_STATE = (size_t)SEL_COUNT * WS_SEL_WORDS * 4;
constexpr size_t WS_CLEAR_BYTES = WS_STATE + (size_t)SEL_COUNT * 256;
constexpr size_t WS_ROWS = WS_CLEAR_BYTES;
constexpr size_t WS_PLANES = WS_ROWS + (size_t)PLANE_MAX_GRID * ROW_WORDS * 8;
static_assert(WS_PLANES % 256 == 0, "planes are 256-byte aligned");

__device__ __forceinline__ int64_t block_sum_i(uint32_t v, void *s) { return block_reduce((int64_t)v, s, SumOp()); }
__device__ __forceinline__ double block_sum_d(double v, void *s) { return block_reduce(v, s, SumOp()); }
__device__ __forceinline__ void put_i(int64_t *row, int k, int64_t v) { if (threadIdx.x == 0) row[k] = v; }
__device__ __forceinline__ void put_d(int64_t *row, int k, double v) { if (threadIdx.x == 0) row[k] = __double_as_longlong(v); }

// ---- 1. magnitude, sign, depth bins --------------------------------------------------------------------------------------
// partial row: int64 [0, 22) in the block's order from `valid`; float64 [22, 34): abs, sq, pos, neg, bin_abs[8]; [34]: the maximum
constexpr int ST_INTS = 6 + 2 * BGNN_NA_DEPTH_BINS, ST_SUMS = 4 + BGNN_NA_DEPTH_BINS;

__global__ __launch_bounds__(NA_THREADS) void na_stream(const int32_t *__restrict__ labels, const float *__restrict__ diff,
                                                        const float *__restrict__ noisy, int64_t cells, uint32_t *__restrict__ hist,
                                                        int64_t *__restrict__ rows) {
  __shared__ int32_t lds[NA_BINS];
  __shared__ int64_t red[NA_THREADS];
  for (int b = threadIdx.x; b < NA_BINS; b += NA_THREADS) lds[b] = 0;
  __syncthreads();
  const float edge[BGNN_NA_DEPTH_BINS + 1] = {0.0f, 10.0f, 20.0f, 50.0f, 100.0f, 200.0f, 500.0f, 1000.0f, 10000.0f};
  uint32_t ci[ST_INTS];                                         // (per thread: cells / threads of the grid, far below 2^32)
  double cd[ST_SUMS];
#pragma unroll
  for (int k = 0; k < ST_INTS; ++k) ci[k] = 0;
#pragma unroll
  for (int k = 0; k < ST_SUMS; ++k) cd[k] = 0.0;
  float mx = 0.0f;
  for (int64_t base = (int64_t)blockIdx.x * NA_CHUNK; base < cells; base += (int64_t)gridDim.x * NA_CHUNK) {
#pragma unroll
    for (int k = 0; k < NA_ITEMS; ++k) {
      const int64_t i = base + k * NA_THREADS + threadIdx.x;
      const bool in = i < cells;
      const int32_t lab = in ? labels[i] : -1;
      const float d = in ? diff[i] : 0.0f;
      const float x = in ? -noisy[i] : __uint_as_float(0x7FC00000u);
      const bool valid = lab >= 0, noise = lab == 2, fin = finite_bits(d), nf = noise && fin;
      const float mag = fabsf(d);
      ci[0] += valid; ci[1] += noise; ci[2] += (lab == 0);
      ci[3] += (nf && d > 0.0f); ci[4] += (nf && d < 0.0f); ci[5] += (noise && !fin);
#pragma unroll
      for (int b = 0; b < BGNN_NA_DEPTH_BINS; ++b) {
        const bool inb = x >= edge[b] && x < edge[b + 1];       // (NaN: in no bin)
        ci[6 + b] += (noise && inb);
        ci[6 + BGNN_NA_DEPTH_BINS + b] += (valid && inb);
        if (nf && inb) cd[4 + b] += (double)mag;
      }
      if (nf) {
        cd[0] += (double)mag;
        cd[1] += (double)d * (double)d;
        if (d > 0.0f) cd[2] += (double)d;
        if (d < 0.0f) cd[3] += (double)d;
        mx = mag > mx ? mag : mx;
      }
      hist_add(lds, nf, __float_as_uint(mag) >> Selection<SEL_MAG>::D::shift(0));
    }
  }
  __syncthreads();
  hist_flush(lds, NA_BINS, hist);
  int64_t *row = rows + (int64_t)blockIdx.x * ROW_WORDS;
#pragma unroll
  for (int k = 0; k < ST_INTS; ++k) put_i(row, k, block_sum_i(ci[k], red));
#pragma unroll
  for (int k = 0; k < ST_SUMS; ++k) put_d(row, ST_INTS + k, block_sum_d(cd[k], red));
  const float m = block_reduce(mx, red, [](float a, float b) { return a > b ? a : b; });
  put_i(row, ST_INTS + ST_SUMS, (int64_t)__float_as_uint(m));
}

// Adds the first n partial rows in workgroup order.  Column t: kind 0 int64 sum, 1 float64 sum, 2 float32 maximum (low 4 bytes of
// the word, 4 bytes stored), 3 int64 maximum; stored at block + off[t].
struct FinishMap {
  int32_t width;
  int16_t off[ROW_WORDS];
  int8_t kind[ROW_WORDS];
};

__global__ __launch_bounds__(64) void na_finish(const int64_t *__restrict__ rows, int n, FinishMap m, char *block) {
  const int t = threadIdx.x;
  if (t >= m.width) return;
  const int kind = m.kind[t];
  int64_t si = 0;
  double sd = 0.0;
  float mf = 0.0f;
  for (int k = 0; k < n; ++k) {
    const int64_t w = rows[(int64_t)k * ROW_WORDS + t];
    if (kind == 0) si += w;
    else if (kind == 1) sd += __longlong_as_double(w);
    else if (kind == 2) { const float v = __uint_as_float((uint32_t)w); mf = v > mf ? v : mf; }
    else si = w > si ? w : si;
  }
  char *dst = block + m.off[t];
  if (kind == 1) *reinterpret_cast<double *>(dst) = sd;
  else if (kind == 2) *reinterpret_cast<float *>(dst) = mf;
  else *reinterpret_cast<int64_t *>(dst) = si;
}

// ---- radix selection ---------------------------------------------------------------------------------------------------------
// What a refine pass reads per cell
struct Source {
  const int32_t *labels;       // MAG
  const float *diff;           // MAG
  const int32_t *parent;       // SIZE
  const int32_t *size;         // SIZE
  const uint64_t *rough;       // ROUGH
};

template <int SEL>
__device__ __forceinline__ bool source_key(const Source &s, int64_t i, typename Selection<SEL>::Key &key) {
  if (SEL == SEL_MAG) {
    const float d = s.diff[i];
    key = __float_as_uint(fabsf(d));
    return s.labels[i] == 2 && finite_bits(d);
  } else if (SEL == SEL_SIZE) {
    key = (uint32_t)s.size[i];
    return (int64_t)s.parent[i] == i;
  } else {
    key = s.rough[i];
    return (key & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
  }
}

// The histogram pass of level LEVEL >= 1 of selection SEL.  Level 1 of SEL_MAG also leaves the partial of
// sum ((double)|d| - mean)^2 with mean = abs_sum / n from the block (DEV; word 0 of the row).
template <int SEL, int LEVEL>
__global__ __launch_bounds__(NA_THREADS) void na_refine(Source src, int64_t cells, const SelState<SEL> *__restrict__ sel,
                                                        uint32_t *__restrict__ hist, const char *__restrict__ block,
                                                        int64_t *__restrict__ rows) {
  using Key = typename Selection<SEL>::Key;
  using D = typename Selection<SEL>::D;
  using Counter = DigitCounter<NA_RANKS, Key, D::shift(LEVEL), D::width(LEVEL)>;
  constexpr bool DEV = SEL == SEL_MAG && LEVEL == 1;
  __shared__ int32_t lds[NA_RANKS * Counter::BINS];
  __shared__ int64_t red[NA_THREADS];
  Counter counter;
  counter.init(sel, lds);
  double mean = 0.0, dev = 0.0;
  if (DEV) {
    const int64_t n = *reinterpret_cast<const int64_t *>(block + BGNN_NA_NOISE) - *reinterpret_cast<const int64_t *>(block + BGNN_NA_NONFINITE);
    mean = n > 0 ? *reinterpret_cast<const double *>(block + BGNN_NA_ABS_SUM) / (double)n : 0.0;
  }
  for (int64_t base = (int64_t)blockIdx.x * NA_CHUNK; base < cells; base += (int64_t)gridDim.x * NA_CHUNK) {
#pragma unroll
    for (int k = 0; k < NA_ITEMS; ++k) {
      const int64_t i = base + k * NA_THREADS + threadIdx.x;
      Key key = 0;
      const bool ok = i < cells && source_key<SEL>(src, i, key);
      if (DEV && ok) {
        const double e = (double)__uint_as_float((uint32_t)key) - mean;
        dev += e * e;
      }
      counter.add(ok, key);
    }
  }
  counter.flush(hist);
  if (DEV) put_d(rows + (int64_t)blockIdx.x * ROW_WORDS, 0, block_sum_d(dev, red));
}

// numpy's percentile on a float32 array of n values (method "linear"): the virtual index in float32, (n - 1) * q with
// q = p / float32(100), its floor and floor + 1 (formed in float32), clipped.
__device__ __forceinline__ void percentile_ranks(int64_t n, float p, int64_t &lo, int64_t &hi) {
  const float q = p / 100.0f;
  const float v = (float)(n - 1) * q;
  const float f = floorf(v);
  lo = (int64_t)f;
  hi = (int64_t)(f + 1.0f);
  if (v >= (float)(n - 1)) lo = hi = n - 1;
  if (v < 0.0f) lo = hi = 0;
}

// One workgroup after the histogram pass of level LEVEL.  Level 0: the ranks from the totals.  The last level: the prefixes are
// the keys, written to the block.
template <int SEL, int LEVEL>
__global__ __launch_bounds__(NA_THREADS) void na_select(const uint32_t *__restrict__ hist, SelState<SEL> *sel, char *block) {
  using Key = typename Selection<SEL>::Key;
  using D = typename Selection<SEL>::D;
  __shared__ SelectScratch<NA_RANKS, Key> sh;
  select_digit<LEVEL == 0, D::width(LEVEL)>(hist, sel, sh, Selection<SEL>::nranks, [](const int64_t *part, int64_t *rank) {
    const int64_t n = part[NA_THREADS];
    if (SEL == SEL_ROUGH) {                // keys with the sign bit (noise) are the upper half of the top digit
      const int64_t ns = part[NA_THREADS / 2], nn = n - ns;
      if (ns > 0) { rank[0] = (ns - 1) / 2; rank[1] = ns / 2; }
      if (nn > 0) { rank[2] = ns + (nn - 1) / 2; rank[3] = ns + nn / 2; }
    } else if (n > 0) {
      rank[0] = (n - 1) / 2; rank[1] = n / 2;
      if (SEL == SEL_MAG) {
        percentile_ranks(n, 90.0f, rank[2], rank[3]);
        percentile_ranks(n, 99.0f, rank[4], rank[5]);
      }
    }
  });
  if (LEVEL == D::N - 1 && threadIdx.x == 0) {
    const SelState<SEL> &out = sh.out;
    if (SEL == SEL_MAG) {
      for (int r = 0; r < BGNN_NA_MAG_RANKS; ++r) {
        reinterpret_cast<int64_t *>(block + BGNN_NA_MAG_RANK)[r] = out.rank0[r];
        reinterpret_cast<uint32_t *>(block + BGNN_NA_MAG_VALUE)[r] = out.rank[r] >= 0 ? (uint32_t)out.prefix[r] : 0x7FC00000u;
      }
    } else if (SEL == SEL_SIZE) {
      for (int r = 0; r < 2; ++r) reinterpret_cast<int64_t *>(block + BGNN_NA_SIZE_MID)[r] = out.rank[r] >= 0 ? (int64_t)out.prefix[r] : 0;
    } else {                               // block order: noise lo, hi (ranks 2, 3), seafloor lo, hi (ranks 0, 1); the sign bit goes
      for (int r = 0; r < 4; ++r) {
        const int from = (r + 2) & 3;
        reinterpret_cast<uint64_t *>(block + BGNN_NA_ROUGH_MID)[r] =
            out.rank[from] >= 0 ? ((uint64_t)out.prefix[from] & 0x7FFFFFFFFFFFFFFFull) : 0x7FF8000000000000ull;
      }
    }
  }
}

// ---- 5. roughness ------------------------------------------------------------------------------------------------------------
// partial row: int64 noise cells, seafloor cells with a roughness; float64 their sums
__global__ __launch_bounds__(NA_THREADS) void na_rough(const float *__restrict__ clean, const int32_t *__restrict__ labels, TileGrid tg,
                                                       uint64_t *__restrict__ plane, uint32_t *__restrict__ hist,
                                                       int64_t *__restrict__ rows) {
  __shared__ float halo[HALO_R][HALO_C];
  __shared__ int32_t lds[NA_BINS];
  __shared__ int64_t red[NA_THREADS];
  const int t = threadIdx.x;
  for (int b = t; b < NA_BINS; b += NA_THREADS) lds[b] = 0;
  const float nan32 = __uint_as_float(0x7FC00000u);
  const uint64_t nan64 = 0x7FF8000000000000ull;
  uint32_t cnt[2] = {0, 0};
  double sum[2] = {0.0, 0.0};
  const int64_t tiles = tg.tiles();
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int r0 = (int)(tile / tg.tiles_c) * TILE_R, c0 = (int)(tile % tg.tiles_c) * TILE_C;
    __syncthreads();                                            // (the previous tile's readers of halo[] are done; lds[] is cleared)
    for (int idx = t; idx < HALO_R * HALO_C; idx += NA_THREADS) {
      const int hr = idx / HALO_C, hc = idx % HALO_C;
      const int gr = r0 + hr - 2, gc = c0 + hc - 2;
      const bool in = gr >= 0 && gr < tg.rows && gc >= 0 && gc < tg.cols;
      halo[hr][hc] = in ? clean[(int64_t)gr * tg.cols + gc] : nan32;
    }
    __syncthreads();
    const int lr = t >> 4, lc = (t & 15) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // numpy.nanstd of the 25 values: the mean of the non-NaN values, then the mean of their squared deviations, in float64
      double s = 0.0;
      int n = 0;
#pragma unroll
      for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int b = 0; b < 5; ++b) {
          const float v = halo[lr + a][lc + j + b];
          if (v == v) { s += (double)v; ++n; }
        }
      const double mean = s / (double)n;                        // (n == 0: NaN, as numpy)
      double q = 0.0;
#pragma unroll
      for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int b = 0; b < 5; ++b) {
          const float v = halo[lr + a][lc + j + b];
          if (v == v) { const double e = (double)v - mean; q += e * e; }
        }
      const double rough = sqrt(q / (double)n);                 // (+-inf in the window: inf - inf = NaN)
      const int gr = r0 + lr, gc = c0 + lc + j;
      const bool in = gr < tg.rows && gc < tg.cols;
      const int64_t i = (int64_t)gr * tg.cols + gc;
      const int32_t lab = in ? labels[i] : -1;
      const bool noise = lab == 2, sea = lab == 0, ok = (noise || sea) && rough == rough;
      const uint64_t bits = ok ? ((uint64_t)__double_as_longlong(rough) & 0x7FFFFFFFFFFFFFFFull) | (noise ? 0x8000000000000000ull : 0ull) : nan64;
      if (in) plane[i] = bits;
      if (ok && noise) { cnt[0] += 1; sum[0] += rough; }
      if (ok && sea) { cnt[1] += 1; sum[1] += rough; }
      hist_add(lds, ok, (uint32_t)(bits >> Selection<SEL_ROUGH>::D::shift(0)));
    }
  }
  __syncthreads();
  hist_flush(lds, NA_BINS, hist);
  int64_t *row = rows + (int64_t)blockIdx.x * ROW_WORDS;
  put_i(row, 0, block_sum_i(cnt[0], red));
  put_i(row, 1, block_sum_i(cnt[1], red));
  put_d(row, 2, block_sum_d(sum[0], red));
  put_d(row, 3, block_sum_d(sum[1], red));
}

// ---- 3. clusters -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NA_THREADS) void ccl_local(const int32_t *__restrict__ labels, TileGrid tg, int32_t *__restrict__ parent,
                                                        int32_t *__restrict__ size, int32_t *__restrict__ col_noise,
                                                        int32_t *__restrict__ col_valid) {
  __shared__ int32_t lp[TILE_CELLS], lsize[TILE_CELLS], cn[TILE_C], cv[TILE_C];
  const int t = threadIdx.x;
  const int64_t tiles = tg.tiles();
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int r0 = (int)(tile / tg.tiles_c) * TILE_R, c0 = (int)(tile % tg.tiles_c) * TILE_C;
    __syncthreads();                                            // (the previous tile is written out)
    if (t < TILE_C) { cn[t] = 0; cv[t] = 0; }
    __syncthreads();
    bool noise[TILE_PER];
#pragma unroll
    for (int k = 0; k < TILE_PER; ++k) {
      const int l = tile_cell(k), gr = r0 + l / TILE_C, gc = c0 + l % TILE_C;
      const bool in = gr < tg.rows && gc < tg.cols;
      const int32_t lab = in ? labels[(int64_t)gr * tg.cols + gc] : -1;
      noise[k] = lab == 2;
      if (lab >= 0) atomicAdd(&cv[l % TILE_C], 1);
      if (noise[k]) atomicAdd(&cn[l % TILE_C], 1);
    }
    int32_t root[TILE_PER];
    tile_label(noise, lp, lsize, root);
    tile_write(tg, r0, c0, noise, root, lsize, parent, size);
    if (t < TILE_C && c0 + t < tg.cols) {
      if (cn[t] != 0) atomicAdd(col_noise + c0 + t, cn[t]);
      if (cv[t] != 0) atomicAdd(col_valid + c0 + t, cv[t]);
    }
  }
}

// partial row: int64 clusters, cells, isolated, size_bins[7]; [10]: the maximum
__global__ __launch_bounds__(NA_THREADS) void ccl_stats(int64_t cells, const int32_t *__restrict__ parent, const int32_t *__restrict__ size,
                                                        uint32_t *__restrict__ hist, int64_t *__restrict__ rows) {
  __shared__ int32_t lds[NA_BINS];
  __shared__ int64_t red[NA_THREADS];
  for (int b = threadIdx.x; b < NA_BINS; b += NA_THREADS) lds[b] = 0;
  __syncthreads();
  const int32_t edge[BGNN_NA_SIZE_BINS + 1] = {1, 2, 5, 10, 50, 100, 1000, 10000};
  uint32_t ci[3 + BGNN_NA_SIZE_BINS];
#pragma unroll
  for (int k = 0; k < 3 + BGNN_NA_SIZE_BINS; ++k) ci[k] = 0;
  int64_t total = 0, mx = 0;
  for (int64_t base = (int64_t)blockIdx.x * NA_CHUNK; base < cells; base += (int64_t)gridDim.x * NA_CHUNK) {
#pragma unroll
    for (int k = 0; k < NA_ITEMS; ++k) {
      const int64_t i = base + k * NA_THREADS + threadIdx.x;
      const bool root = i < cells && (int64_t)parent[i] == i;
      const int32_t s = root ? size[i] : 0;
      if (root) {
        ci[0] += 1; total += s; ci[2] += (s == 1);
        mx = s > mx ? s : mx;
#pragma unroll
        for (int b = 0; b < BGNN_NA_SIZE_BINS; ++b) ci[3 + b] += (s >= edge[b] && s < edge[b + 1]);
      }
      hist_add(lds, root, (uint32_t)s >> Selection<SEL_SIZE>::D::shift(0));
    }
  }
  __syncthreads();
  hist_flush(lds, NA_BINS, hist);
  int64_t *row = rows + (int64_t)blockIdx.x * ROW_WORDS;
  put_i(row, 0, block_sum_i(ci[0], red));
  put_i(row, 1, block_reduce(total, red, SumOp()));
#pragma unroll
  for (int k = 2; k < 3 + BGNN_NA_SIZE_BINS; ++k) put_i(row, k, block_sum_i(ci[k], red));
  put_i(row, 3 + BGNN_NA_SIZE_BINS, block_reduce(mx, red, [](int64_t a, int64_t b) { return a > b ? a : b; }));
}

// The launches of selection SEL once its top digit is counted: na_select of level 0, then na_refine and na_select of every further
// level; after_first_refine() goes between the two of level 1.
struct SelLaunch {
  hipStream_t stream;
  int grid;
  Source src;
  int64_t cells;
  char *workspace, *block;
  int64_t *rows;
};
template <int SEL, int LEVEL = 0, typename F>
void launch_selection(const SelLaunch &a, F after_first_refine) {
  uint32_t *hist = reinterpret_cast<uint32_t *>(a.workspace) + (size_t)SEL * WS_SEL_WORDS + (size_t)LEVEL * WS_LEVEL_WORDS;
  SelState<SEL> *state = reinterpret_cast<SelState<SEL> *>(a.workspace + WS_STATE + (size_t)SEL * 256);
  if constexpr (LEVEL > 0) {
    hipLaunchKernelGGL((na_refine<SEL, LEVEL>), dim3(a.grid), dim3(NA_THREADS), 0, a.stream, a.src, a.cells, state, hist, a.block, a.rows);
    if (LEVEL == 1) after_first_refine();
  }
  hipLaunchKernelGGL((na_select<SEL, LEVEL>), dim3(1), dim3(NA_THREADS), 0, a.stream, hist, state, a.block);
  if constexpr (LEVEL + 1 < Selection<SEL>::D::N) launch_selection<SEL, LEVEL + 1>(a, after_first_refine);
}

inline bool within_limit(int64_t rows, int64_t cols) { return rows >= 1 && cols >= 1 && rows <= (int64_t)BGNN_NA_MAX_CELLS / cols; }

inline void map_run(FinishMap &m, int kind, int offset, int count, int stride = 8) {
  for (int k = 0; k < count; ++k) { m.off[m.width] = (int16_t)(offset + k * stride); m.kind[m.width] = (int8_t)kind; ++m.width; }
}

}  // namespace
}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_noise_analysis_workspace_bytes(int64_t rows, int64_t cols) {
  if (!within_limit(rows, cols)) return 0;
  const size_t cells = (size_t)rows * (size_t)cols;
  return WS_PLANES + 2 * align256(cells * 4) + align256(cells * 8);
}

extern "C" int bgnn_noise_analysis(bgnn_ctx *ctx, const int32_t *labels, const float *difference, const float *noisy, const float *clean,
                                   int64_t rows, int64_t cols, void *workspace, size_t workspace_bytes, void *block, int32_t *col_noise,
                                   int32_t *col_valid) {
  BGNN_REQUIRE(ctx && labels && difference && noisy && clean && workspace && block && col_noise && col_valid,
               "bgnn_noise_analysis: NULL argument");
  BGNN_REQUIRE(rows >= 1 && cols >= 1, "bgnn_noise_analysis: a grid of %lld x %lld", (long long)rows, (long long)cols);
  if (!within_limit(rows, cols)) {
    set_error("bgnn_noise_analysis: %lld x %lld cells exceed the limit of %lld (int32 cluster labels)", (long long)rows, (long long)cols,
              (long long)BGNN_NA_MAX_CELLS);
    return BGNN_ERR_UNSUPPORTED;
  }
  const size_t need = bgnn_noise_analysis_workspace_bytes(rows, cols);
  BGNN_REQUIRE(workspace_bytes >= need, "bgnn_noise_analysis: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  BGNN_REQUIRE(((uintptr_t)workspace & 7) == 0, "bgnn_noise_analysis: the workspace is not 8-byte aligned");
  BGNN_REQUIRE(((uintptr_t)block & 7) == 0, "bgnn_noise_analysis: the result block is not 8-byte aligned");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const int64_t cells = rows * cols;
  char *w = static_cast<char *>(workspace), *blk = static_cast<char *>(block);
  uint32_t *hists = reinterpret_cast<uint32_t *>(w);
  auto top_hist = [&](int sel) { return hists + (size_t)sel * WS_SEL_WORDS; };
  int64_t *part = reinterpret_cast<int64_t *>(w + WS_ROWS);
  int32_t *parent = reinterpret_cast<int32_t *>(w + WS_PLANES);
  int32_t *size = reinterpret_cast<int32_t *>(w + WS_PLANES + align256((size_t)cells * 4));
  uint64_t *rough = reinterpret_cast<uint64_t *>(w + WS_PLANES + 2 * align256((size_t)cells * 4));
  const TileGrid tg(rows, cols);
  const int g_stream = capped_grid((cells + NA_CHUNK - 1) / NA_CHUNK, PLANE_MAX_GRID), g_tiles = tg.local_grid();
  const dim3 b(NA_THREADS), one(1), fin(64);
  hipStream_t s = ctx->stream;
  const SelLaunch sel{s, g_stream, Source{labels, difference, parent, size, rough}, cells, w, blk, part};

  BGNN_HIP_CHECK(hipMemsetAsync(w, 0, WS_CLEAR_BYTES, s));
  BGNN_HIP_CHECK(hipMemsetAsync(blk, 0, BGNN_NA_BYTES, s));
  BGNN_HIP_CHECK(hipMemsetAsync(col_noise, 0, (size_t)cols * 4, s));
  BGNN_HIP_CHECK(hipMemsetAsync(col_valid, 0, (size_t)cols * 4, s));

  // 1, 2: magnitude, sign, depth bins; the six order statistics of |difference|
  hipLaunchKernelGGL(na_stream, dim3(g_stream), b, 0, s, labels, difference, noisy, cells, top_hist(SEL_MAG), part);
  {
    FinishMap m{};
    map_run(m, 0, BGNN_NA_VALID, ST_INTS);
    map_run(m, 1, BGNN_NA_ABS_SUM, 2);
    map_run(m, 1, BGNN_NA_POS_SUM, 2 + BGNN_NA_DEPTH_BINS);
    map_run(m, 2, BGNN_NA_ABS_MAX, 1);
    hipLaunchKernelGGL(na_finish, one, fin, 0, s, part, g_stream, m, blk);
  }
  launch_selection<SEL_MAG>(sel, [&] {
    FinishMap m{};
    map_run(m, 1, BGNN_NA_DEV_SQ_SUM, 1);
    hipLaunchKernelGGL(na_finish, one, fin, 0, s, part, g_stream, m, blk);
  });

  // 5: roughness and its class medians
  hipLaunchKernelGGL(na_rough, dim3(g_tiles), b, 0, s, clean, labels, tg, rough, top_hist(SEL_ROUGH), part);
  {
    FinishMap m{};
    map_run(m, 0, BGNN_NA_ROUGH_COUNT, 2);
    map_run(m, 1, BGNN_NA_ROUGH_SUM, 2);
    hipLaunchKernelGGL(na_finish, one, fin, 0, s, part, g_tiles, m, blk);
  }
  launch_selection<SEL_ROUGH>(sel, [] {});

  // 3, 4: clusters, the per-column counts, the median cluster size
  hipLaunchKernelGGL(ccl_local, dim3(g_tiles), b, 0, s, labels, tg, parent, size, col_noise, col_valid);
  launch_merge_flatten(s, tg, parent, SizeOnly{size});
  hipLaunchKernelGGL(ccl_stats, dim3(g_stream), b, 0, s, cells, parent, size, top_hist(SEL_SIZE), part);
  {
    FinishMap m{};
    map_run(m, 0, BGNN_NA_NUM_CLUSTERS, 2);
    map_run(m, 0, BGNN_NA_ISOLATED, 1 + BGNN_NA_SIZE_BINS);
    map_run(m, 3, BGNN_NA_MAX_CLUSTER, 1);
    hipLaunchKernelGGL(na_finish, one, fin, 0, s, part, g_stream, m, blk);
  }
  launch_selection<SEL_SIZE>(sel, [] {});
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
