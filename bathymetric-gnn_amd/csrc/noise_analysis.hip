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
//   na_select        one workgroup after every histogram pass: walks the histograms and narrows prefix and rank of every rank
//   na_finish        one workgroup: adds the partial rows in workgroup order into the result block
//
// Multi-rank radix selection.  Ranks whose keys share the prefix fixed so far share one histogram ("group"); a level's pass
// compares each key with the at most six group prefixes.  The histograms are integer LDS atomics merged with integer global
// atomics, hist_add peels a wave's two most frequent bins first (ground_truth.hip explains why).
//
// Connected components (4-connectivity, scipy.ndimage.label's default structure): label equivalence by union-find over int32
// cell indices, parent[i] = -1 off the noise mask.
//   ccl_local    a 16 x 64 tile in LDS: every noise cell unites with its left and upper neighbour inside the tile; then the cell's
//                parent becomes the global index of its tile-local root, and that root's size counter gets the cells of the
//                component inside the tile.  Also the per-column noise / valid counts of the tile (64 x 2 global integer adds)
//   ccl_merge    every noise cell in the first row / column of a tile unites with its neighbour across the border (global atomics)
//   ccl_flatten  every tile-local root that is not a global root finds its root, points at it, and adds its counter to the root's
//                (integer atomicAdd: order-independent).  Roots are stable here: the merges ended with the previous kernel
//   ccl_stats    over the global roots (parent[i] == i): count, size sum, maximum, size bins, the top size bits
//
// Termination, by construction.  Invariant: parent[i] <= i for every noise cell, at all times.  It holds after initialisation
// (parent[i] = i, or the tile-local root, the smallest index of the component in the tile, in row-major order both locally and
// globally), and the only later writes are atomicMin(&parent[a], b) with b < a and, in ccl_flatten, parent[i] = root <= i.
//   find(x)   follows parent while parent[x] != x: each step strictly lowers x, so it ends after at most x steps whatever other
//             threads write meanwhile (a stale read only makes it stop at an older ancestor; the atomicMin below detects that).
//   unite(a, b)   a = find(a), b = find(b); equal: done.  Otherwise, with a > b: old = atomicMin(&parent[a], b).  old == a: a was
//             still a root and now points at b: done.  Otherwise another thread lowered parent[a] to old < a first; whichever of
//             old and b stayed in parent[a], the pair (old, b) still has to be united: continue with a = old.  Every iteration
//             replaces the larger of two non-negative indices by a strictly smaller one, so a + b strictly decreases: the loop ends.
// No thread waits for another: there is no spin-wait on a flag or a workgroup, no grid-wide barrier and no persistent kernel; a
// workgroup's progress never depends on another workgroup being scheduled.
//
// Compiled with -ffp-contract=off: the float32 rank arithmetic of numpy's percentile and the float64 squares round as written.
#include "bgnn_internal.h"
#include "../../include/bgnn_analysis.h"

namespace bgnn {
namespace {

constexpr int NA_THREADS = 256;
constexpr int NA_ITEMS = 4;                           // cells per thread and step of a streaming pass (each load coalesced)
constexpr int NA_CHUNK = NA_THREADS * NA_ITEMS;
constexpr int NA_MAX_GRID = 2048;                     // 256 CUs x 8 workgroups
constexpr int NA_BINS = 2048;                         // 11-bit digits (the last digit of a key may be narrower)
constexpr int NA_RANKS = 6;
constexpr int NA_LEVELS = 6;                          // of a 64-bit key: 11 x 5 + 9; a 32-bit key has 11 + 11 + 10
constexpr int TILE_R = 16, TILE_C = 64;               // tile of ccl_local / na_rough: 1024 cells
constexpr int HALO_R = TILE_R + 4, HALO_C = TILE_C + 4;
constexpr int ROW_WORDS = 40;                         // a partial row: 8-byte words

enum { SEL_MAG = 0, SEL_ROUGH = 1, SEL_SIZE = 2, SEL_COUNT = 3 };

struct SelState {
  uint64_t prefix[NA_RANKS];       // the key bits fixed so far, per rank (NO_PREFIX: the rank does not exist)
  uint64_t gprefix[NA_RANKS];      // the same per group: the distinct prefixes
  int64_t rank[NA_RANKS];          // the rank among the keys under the prefix
  int64_t rank0[NA_RANKS];         // the rank among all keys
  int32_t group[NA_RANKS];         // the histogram the rank reads at the next level (-1: none)
  int32_t ngroups, nranks;
};
static_assert(sizeof(SelState) <= 256, "selection state");
constexpr uint64_t NO_PREFIX = ~0ull;                 // matches no key: a prefix below the last level has fewer than 64 bits

// workspace: [histograms | selection states] (cleared by one memset), the partial rows, then the three planes
constexpr size_t WS_LEVEL_WORDS = (size_t)NA_RANKS * NA_BINS;
constexpr size_t WS_SEL_WORDS = (size_t)NA_LEVELS * WS_LEVEL_WORDS;
constexpr size_t WS_STATE = (size_t)SEL_COUNT * WS_SEL_WORDS * 4;
constexpr size_t WS_CLEAR_BYTES = WS_STATE + (size_t)SEL_COUNT * 256;
constexpr size_t WS_ROWS = WS_CLEAR_BYTES;
constexpr size_t WS_PLANES = WS_ROWS + (size_t)NA_MAX_GRID * ROW_WORDS * 8;
static_assert(WS_PLANES % 256 == 0, "planes are 256-byte aligned");
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

inline int capped_grid(int64_t work_items) {
  return (int)(work_items < 1 ? 1 : (work_items > NA_MAX_GRID ? NA_MAX_GRID : work_items));
}

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// One count per active lane into an LDS histogram; called by whole waves (see ground_truth.hip: hist_add).
__device__ __forceinline__ void hist_add(int32_t *hist, bool active, uint32_t bin) {
  const int lane = threadIdx.x & 63;
  unsigned long long waiting = __ballot(active);
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    if (waiting == 0) break;                                    // (uniform)
    const int leader = __ffsll(waiting) - 1;
    const uint32_t lb = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
    const bool mine = active && bin == lb;
    const unsigned long long m = __ballot(mine);
    if (lane == leader) atomicAdd(&hist[lb], (int32_t)__popcll(m));
    if (mine) active = false;
    waiting &= ~m;
  }
  if (active) atomicAdd(&hist[bin], 1);
}

__device__ __forceinline__ void hist_flush(const int32_t *lds, int bins, uint32_t *global) {
  for (int b = threadIdx.x; b < bins; b += NA_THREADS) {
    const int32_t c = lds[b];
    if (c != 0) atomicAdd(global + b, (uint32_t)c);
  }
}

// A fixed tree over the workgroup's threads; every thread calls it, every thread gets the result.
template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, void *scratch, Op op) {
  static_assert(sizeof(T) <= 8, "scratch holds 8 bytes per thread");
  T *s = static_cast<T *>(scratch);
  const int t = threadIdx.x;
  __syncthreads();                                              // (the previous call's readers are done)
  s[t] = v;
  __syncthreads();
  for (int w = NA_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) s[t] = op(s[t], s[t + w]);
    __syncthreads();
  }
  return s[0];
}
__device__ __forceinline__ int64_t block_sum_i(uint32_t v, void *s) {
  return block_reduce<int64_t>((int64_t)v, s, [](int64_t a, int64_t b) { return a + b; });
}
__device__ __forceinline__ double block_sum_d(double v, void *s) {
  return block_reduce<double>(v, s, [](double a, double b) { return a + b; });
}
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
      hist_add(lds, nf, __float_as_uint(mag) >> 21);
    }
  }
  __syncthreads();
  hist_flush(lds, NA_BINS, hist);
  int64_t *row = rows + (int64_t)blockIdx.x * ROW_WORDS;
#pragma unroll
  for (int k = 0; k < ST_INTS; ++k) put_i(row, k, block_sum_i(ci[k], red));
#pragma unroll
  for (int k = 0; k < ST_SUMS; ++k) put_d(row, ST_INTS + k, block_sum_d(cd[k], red));
  const float m = block_reduce<float>(mx, red, [](float a, float b) { return a > b ? a : b; });
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
__device__ __forceinline__ bool source_key(const Source &s, int64_t i, uint64_t &key) {
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

// SHIFT: the bits below this level's digit; BITS: the digit's width; the bits above the digit are the prefix.
// DEV (SEL_MAG): also the partial of sum ((double)|d| - mean)^2 with mean = abs_sum / n from the block (word 0 of the row).
template <int SEL, int SHIFT, int BITS, bool DEV>
__global__ __launch_bounds__(NA_THREADS) void na_refine(Source src, int64_t cells, const SelState *__restrict__ sel,
                                                        uint32_t *__restrict__ hist, const char *__restrict__ block,
                                                        int64_t *__restrict__ rows) {
  constexpr int BINS = 1 << BITS;
  __shared__ int32_t lds[NA_RANKS * NA_BINS];
  __shared__ int64_t red[NA_THREADS];
  const int ng = sel->ngroups;                                  // (uniform; 0 without a key)
  uint64_t gp[NA_RANKS];
#pragma unroll
  for (int g = 0; g < NA_RANKS; ++g) gp[g] = sel->gprefix[g];
  for (int b = threadIdx.x; b < ng * NA_BINS; b += NA_THREADS) lds[b] = 0;
  __syncthreads();
  double mean = 0.0, dev = 0.0;
  if (DEV) {
    const int64_t n = *reinterpret_cast<const int64_t *>(block + BGNN_NA_NOISE) - *reinterpret_cast<const int64_t *>(block + BGNN_NA_NONFINITE);
    mean = n > 0 ? *reinterpret_cast<const double *>(block + BGNN_NA_ABS_SUM) / (double)n : 0.0;
  }
  for (int64_t base = (int64_t)blockIdx.x * NA_CHUNK; base < cells; base += (int64_t)gridDim.x * NA_CHUNK) {
#pragma unroll
    for (int k = 0; k < NA_ITEMS; ++k) {
      const int64_t i = base + k * NA_THREADS + threadIdx.x;
      uint64_t key = 0;
      const bool ok = i < cells && source_key<SEL>(src, i, key);
      if (DEV && ok) {
        const double e = (double)__uint_as_float((uint32_t)key) - mean;
        dev += e * e;
      }
      const uint64_t top = key >> (SHIFT + BITS);
      const uint32_t bin = (uint32_t)(key >> SHIFT) & (BINS - 1);
#pragma unroll
      for (int g = 0; g < NA_RANKS; ++g)
        if (g < ng) hist_add(lds + g * NA_BINS, ok && top == gp[g], bin);      // (uniform condition)
    }
  }
  __syncthreads();
  for (int g = 0; g < ng; ++g) hist_flush(lds + g * NA_BINS, BINS, hist + (size_t)g * NA_BINS);
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

// One workgroup.  FIRST: the single histogram of the top digit; the ranks come from its totals.  LAST: the prefixes are the keys.
template <int SEL, int BITS, bool FIRST, bool LAST>
__global__ __launch_bounds__(NA_THREADS) void na_select(const uint32_t *__restrict__ hist, SelState *sel, char *block) {
  constexpr int BINS = 1 << BITS, PER = BINS / NA_THREADS;
  static_assert(PER >= 1, "a digit has at least 8 bits");
  __shared__ int64_t part[NA_THREADS + 1];
  __shared__ SelState in, out;
  const int t = threadIdx.x;
  if (t == 0) {
    if (FIRST) {
      for (int r = 0; r < NA_RANKS; ++r) { in.prefix[r] = 0; in.gprefix[r] = 0; in.rank[r] = -1; in.rank0[r] = -1; in.group[r] = 0; }
      in.ngroups = 1;
      in.nranks = SEL == SEL_MAG ? 6 : (SEL == SEL_ROUGH ? 4 : 2);
    } else {
      in = *sel;
    }
    for (int r = 0; r < NA_RANKS; ++r) { out.prefix[r] = NO_PREFIX; out.gprefix[r] = NO_PREFIX; out.rank[r] = -1; out.group[r] = -1; }
  }
  __syncthreads();
  const int ng = in.ngroups;
  for (int g = 0; g < ng; ++g) {
    const uint32_t *h = hist + (size_t)g * NA_BINS;
    int64_t local[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) { local[k] = (int64_t)h[t * PER + k]; sum += local[k]; }
    __syncthreads();                       // (the previous round's readers of part[] are done)
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
      int64_t run = 0;
      for (int k = 0; k < NA_THREADS; ++k) { const int64_t v = part[k]; part[k] = run; run += v; }
      part[NA_THREADS] = run;
      if (FIRST) {                         // the ranks, from the totals
        const int64_t n = run;
        if (SEL == SEL_ROUGH) {            // keys with the sign bit (noise) are the upper half of the top digit
          const int64_t ns = part[NA_THREADS / 2], nn = n - ns;
          if (ns > 0) { in.rank[0] = (ns - 1) / 2; in.rank[1] = ns / 2; }
          if (nn > 0) { in.rank[2] = ns + (nn - 1) / 2; in.rank[3] = ns + nn / 2; }
        } else if (n > 0) {
          in.rank[0] = (n - 1) / 2; in.rank[1] = n / 2;
          if (SEL == SEL_MAG) {
            percentile_ranks(n, 90.0f, in.rank[2], in.rank[3]);
            percentile_ranks(n, 99.0f, in.rank[4], in.rank[5]);
          }
        }
        for (int r = 0; r < NA_RANKS; ++r) {
          in.rank0[r] = in.rank[r];
          if (in.rank[r] < 0) in.group[r] = -1;
        }
      }
    }
    __syncthreads();
    const int64_t start = part[t];
    for (int r = 0; r < in.nranks; ++r) {
      const int64_t rank = in.rank[r];
      if (in.group[r] != g || rank < 0) continue;
      if (rank >= start && rank < start + sum) {                // exactly one thread: rank < the count under the prefix
        int64_t below = start;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
          if (rank >= below && rank < below + local[k]) {
            out.prefix[r] = (in.prefix[r] << BITS) | (uint64_t)(t * PER + k);
            out.rank[r] = rank - below;
          }
          below += local[k];
        }
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    int groups = 0;
    for (int r = 0; r < in.nranks; ++r) {
      out.rank0[r] = in.rank0[r];
      if (out.rank[r] < 0) continue;
      int g = -1;
      for (int q = 0; q < r; ++q)
        if (out.rank[q] >= 0 && out.prefix[q] == out.prefix[r]) { g = out.group[q]; break; }
      if (g < 0) { g = groups++; out.gprefix[g] = out.prefix[r]; }
      out.group[r] = g;
    }
    for (int r = in.nranks; r < NA_RANKS; ++r) out.rank0[r] = -1;
    out.ngroups = groups;
    out.nranks = in.nranks;
    *sel = out;
    if (LAST) {
      if (SEL == SEL_MAG) {
        for (int r = 0; r < BGNN_NA_MAG_RANKS; ++r) {
          reinterpret_cast<int64_t *>(block + BGNN_NA_MAG_RANK)[r] = out.rank0[r];
          reinterpret_cast<uint32_t *>(block + BGNN_NA_MAG_VALUE)[r] = out.rank[r] >= 0 ? (uint32_t)out.prefix[r] : 0x7FC00000u;
        }
      } else if (SEL == SEL_SIZE) {
        for (int r = 0; r < 2; ++r) reinterpret_cast<int64_t *>(block + BGNN_NA_SIZE_MID)[r] = out.rank[r] >= 0 ? (int64_t)out.prefix[r] : 0;
      } else {                             // block order: noise lo, hi (ranks 2, 3), seafloor lo, hi (ranks 0, 1); the sign bit goes
        for (int r = 0; r < 4; ++r) {
          const int from = (r + 2) & 3;
          reinterpret_cast<uint64_t *>(block + BGNN_NA_ROUGH_MID)[r] =
              out.rank[from] >= 0 ? (out.prefix[from] & 0x7FFFFFFFFFFFFFFFull) : 0x7FF8000000000000ull;
        }
      }
    }
  }
}

// ---- 5. roughness ------------------------------------------------------------------------------------------------------------
struct TileGrid {
  int32_t rows, cols, tiles_r, tiles_c;
};

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
  const int64_t tiles = (int64_t)tg.tiles_r * tg.tiles_c;
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
      hist_add(lds, ok, (uint32_t)(bits >> 53));
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
// GLOBAL: the parent array is in global memory and other workgroups lower it meanwhile: device-scope loads.  Else: LDS.
template <bool GLOBAL>
__device__ __forceinline__ int32_t load_parent(const int32_t *p, int32_t x) {
  return GLOBAL ? __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                : __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool GLOBAL>
__device__ __forceinline__ int32_t find_root(const int32_t *p, int32_t x) {
  for (;;) {                                                    // parent[x] <= x: every step strictly lowers x
    const int32_t q = load_parent<GLOBAL>(p, x);
    if (q == x) return x;
    x = q;
  }
}
template <bool GLOBAL>
__device__ __forceinline__ void unite(int32_t *p, int32_t a, int32_t b) {
  for (;;) {                                                    // a + b strictly decreases: see the head of the file
    a = find_root<GLOBAL>(p, a);
    b = find_root<GLOBAL>(p, b);
    if (a == b) return;
    if (a < b) { const int32_t s = a; a = b; b = s; }
    const int32_t old = atomicMin(p + a, b);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(NA_THREADS) void ccl_local(const int32_t *__restrict__ labels, TileGrid tg, int32_t *__restrict__ parent,
                                                        int32_t *__restrict__ size, int32_t *__restrict__ col_noise,
                                                        int32_t *__restrict__ col_valid) {
  constexpr int CELLS = TILE_R * TILE_C, PER = CELLS / NA_THREADS;
  __shared__ int32_t lp[CELLS], lsize[CELLS], cn[TILE_C], cv[TILE_C];
  const int t = threadIdx.x;
  const int64_t tiles = (int64_t)tg.tiles_r * tg.tiles_c;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int r0 = (int)(tile / tg.tiles_c) * TILE_R, c0 = (int)(tile % tg.tiles_c) * TILE_C;
    __syncthreads();                                            // (the previous tile is written out)
    if (t < TILE_C) { cn[t] = 0; cv[t] = 0; }
    __syncthreads();
    bool noise[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int l = k * NA_THREADS + t, gr = r0 + l / TILE_C, gc = c0 + l % TILE_C;
      const bool in = gr < tg.rows && gc < tg.cols;
      const int32_t lab = in ? labels[(int64_t)gr * tg.cols + gc] : -1;
      noise[k] = lab == 2;
      lp[l] = noise[k] ? l : -1;
      lsize[l] = 0;
      if (lab >= 0) atomicAdd(&cv[l % TILE_C], 1);
      if (noise[k]) atomicAdd(&cn[l % TILE_C], 1);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int l = k * NA_THREADS + t;
      if (!noise[k]) continue;
      if (l % TILE_C > 0 && load_parent<false>(lp, l - 1) >= 0) unite<false>(lp, l, l - 1);
      if (l >= TILE_C && load_parent<false>(lp, l - TILE_C) >= 0) unite<false>(lp, l, l - TILE_C);
    }
    __syncthreads();
    int32_t root[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      root[k] = noise[k] ? find_root<false>(lp, k * NA_THREADS + t) : -1;
      if (noise[k]) atomicAdd(&lsize[root[k]], 1);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int l = k * NA_THREADS + t, gr = r0 + l / TILE_C, gc = c0 + l % TILE_C;
      if (gr >= tg.rows || gc >= tg.cols) continue;
      const int64_t i = (int64_t)gr * tg.cols + gc;
      const int rl = root[k];
      parent[i] = noise[k] ? (int32_t)((int64_t)(r0 + rl / TILE_C) * tg.cols + c0 + rl % TILE_C) : -1;
      size[i] = (noise[k] && rl == l) ? lsize[l] : 0;
    }
    if (t < TILE_C && c0 + t < tg.cols) {
      if (cn[t] != 0) atomicAdd(col_noise + c0 + t, cn[t]);
      if (cv[t] != 0) atomicAdd(col_valid + c0 + t, cv[t]);
    }
  }
}

// The cells that have a neighbour across a tile border: (tiles_r - 1) * cols in the first rows of the lower tiles (upper
// neighbour), then (tiles_c - 1) * rows in the first columns of the right-hand tiles (left neighbour).
__global__ __launch_bounds__(NA_THREADS) void ccl_merge(TileGrid tg, int32_t *parent) {
  const int64_t nh = (int64_t)(tg.tiles_r - 1) * tg.cols, total = nh + (int64_t)(tg.tiles_c - 1) * tg.rows;
  for (int64_t j = (int64_t)blockIdx.x * NA_THREADS + threadIdx.x; j < total; j += (int64_t)gridDim.x * NA_THREADS) {
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

__global__ __launch_bounds__(NA_THREADS) void ccl_flatten(int64_t cells, int32_t *parent, int32_t *size) {
  for (int64_t i = (int64_t)blockIdx.x * NA_THREADS + threadIdx.x; i < cells; i += (int64_t)gridDim.x * NA_THREADS) {
    const int32_t s = size[i];                                  // (> 0: a tile-local root; only global roots' counters change here)
    if (s <= 0) continue;
    const int32_t root = find_root<true>(parent, (int32_t)i);
    if (root == (int32_t)i) continue;
    __hip_atomic_store(parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(size + root, s);
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
      hist_add(lds, root, (uint32_t)s >> 21);
    }
  }
  __syncthreads();
  hist_flush(lds, NA_BINS, hist);
  int64_t *row = rows + (int64_t)blockIdx.x * ROW_WORDS;
  put_i(row, 0, block_sum_i(ci[0], red));
  put_i(row, 1, block_reduce<int64_t>(total, red, [](int64_t a, int64_t b) { return a + b; }));
#pragma unroll
  for (int k = 2; k < 3 + BGNN_NA_SIZE_BINS; ++k) put_i(row, k, block_sum_i(ci[k], red));
  put_i(row, 3 + BGNN_NA_SIZE_BINS, block_reduce<int64_t>(mx, red, [](int64_t a, int64_t b) { return a > b ? a : b; }));
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
  auto hist = [&](int sel, int level) { return hists + (size_t)sel * WS_SEL_WORDS + (size_t)level * WS_LEVEL_WORDS; };
  auto state = [&](int sel) { return reinterpret_cast<SelState *>(w + WS_STATE + (size_t)sel * 256); };
  int64_t *part = reinterpret_cast<int64_t *>(w + WS_ROWS);
  int32_t *parent = reinterpret_cast<int32_t *>(w + WS_PLANES);
  int32_t *size = reinterpret_cast<int32_t *>(w + WS_PLANES + align256((size_t)cells * 4));
  uint64_t *rough = reinterpret_cast<uint64_t *>(w + WS_PLANES + 2 * align256((size_t)cells * 4));
  TileGrid tg;
  tg.rows = (int32_t)rows; tg.cols = (int32_t)cols;
  tg.tiles_r = (int32_t)((rows + TILE_R - 1) / TILE_R); tg.tiles_c = (int32_t)((cols + TILE_C - 1) / TILE_C);
  const int64_t tiles = (int64_t)tg.tiles_r * tg.tiles_c;
  const int64_t borders = (int64_t)(tg.tiles_r - 1) * cols + (int64_t)(tg.tiles_c - 1) * rows;
  const int g_stream = capped_grid((cells + NA_CHUNK - 1) / NA_CHUNK), g_tiles = capped_grid(tiles);
  const int g_cells = capped_grid((cells + NA_THREADS - 1) / NA_THREADS), g_borders = capped_grid((borders + NA_THREADS - 1) / NA_THREADS);
  const dim3 b(NA_THREADS), one(1), fin(64);
  hipStream_t s = ctx->stream;
  Source src{labels, difference, parent, size, rough};

  BGNN_HIP_CHECK(hipMemsetAsync(w, 0, WS_CLEAR_BYTES, s));
  BGNN_HIP_CHECK(hipMemsetAsync(blk, 0, BGNN_NA_BYTES, s));
  BGNN_HIP_CHECK(hipMemsetAsync(col_noise, 0, (size_t)cols * 4, s));
  BGNN_HIP_CHECK(hipMemsetAsync(col_valid, 0, (size_t)cols * 4, s));

  // 1, 2: magnitude, sign, depth bins; the six order statistics of |difference|
  hipLaunchKernelGGL(na_stream, dim3(g_stream), b, 0, s, labels, difference, noisy, cells, hist(SEL_MAG, 0), part);
  {
    FinishMap m{};
    map_run(m, 0, BGNN_NA_VALID, ST_INTS);
    map_run(m, 1, BGNN_NA_ABS_SUM, 2);
    map_run(m, 1, BGNN_NA_POS_SUM, 2 + BGNN_NA_DEPTH_BINS);
    map_run(m, 2, BGNN_NA_ABS_MAX, 1);
    hipLaunchKernelGGL(na_finish, one, fin, 0, s, part, g_stream, m, blk);
  }
  hipLaunchKernelGGL((na_select<SEL_MAG, 11, true, false>), one, b, 0, s, hist(SEL_MAG, 0), state(SEL_MAG), blk);
  hipLaunchKernelGGL((na_refine<SEL_MAG, 10, 11, true>), dim3(g_stream), b, 0, s, src, cells, state(SEL_MAG), hist(SEL_MAG, 1), blk, part);
  {
    FinishMap m{};
    map_run(m, 1, BGNN_NA_DEV_SQ_SUM, 1);
    hipLaunchKernelGGL(na_finish, one, fin, 0, s, part, g_stream, m, blk);
  }
  hipLaunchKernelGGL((na_select<SEL_MAG, 11, false, false>), one, b, 0, s, hist(SEL_MAG, 1), state(SEL_MAG), blk);
  hipLaunchKernelGGL((na_refine<SEL_MAG, 0, 10, false>), dim3(g_stream), b, 0, s, src, cells, state(SEL_MAG), hist(SEL_MAG, 2), blk, part);
  hipLaunchKernelGGL((na_select<SEL_MAG, 10, false, true>), one, b, 0, s, hist(SEL_MAG, 2), state(SEL_MAG), blk);

  // 5: roughness and its class medians: six digits of 11, 11, 11, 11, 11 and 9 bits
  hipLaunchKernelGGL(na_rough, dim3(g_tiles), b, 0, s, clean, labels, tg, rough, hist(SEL_ROUGH, 0), part);
  {
    FinishMap m{};
    map_run(m, 0, BGNN_NA_ROUGH_COUNT, 2);
    map_run(m, 1, BGNN_NA_ROUGH_SUM, 2);
    hipLaunchKernelGGL(na_finish, one, fin, 0, s, part, g_tiles, m, blk);
  }
  hipLaunchKernelGGL((na_select<SEL_ROUGH, 11, true, false>), one, b, 0, s, hist(SEL_ROUGH, 0), state(SEL_ROUGH), blk);
  hipLaunchKernelGGL((na_refine<SEL_ROUGH, 42, 11, false>), dim3(g_stream), b, 0, s, src, cells, state(SEL_ROUGH), hist(SEL_ROUGH, 1), blk, part);
  hipLaunchKernelGGL((na_select<SEL_ROUGH, 11, false, false>), one, b, 0, s, hist(SEL_ROUGH, 1), state(SEL_ROUGH), blk);
  hipLaunchKernelGGL((na_refine<SEL_ROUGH, 31, 11, false>), dim3(g_stream), b, 0, s, src, cells, state(SEL_ROUGH), hist(SEL_ROUGH, 2), blk, part);
  hipLaunchKernelGGL((na_select<SEL_ROUGH, 11, false, false>), one, b, 0, s, hist(SEL_ROUGH, 2), state(SEL_ROUGH), blk);
  hipLaunchKernelGGL((na_refine<SEL_ROUGH, 20, 11, false>), dim3(g_stream), b, 0, s, src, cells, state(SEL_ROUGH), hist(SEL_ROUGH, 3), blk, part);
  hipLaunchKernelGGL((na_select<SEL_ROUGH, 11, false, false>), one, b, 0, s, hist(SEL_ROUGH, 3), state(SEL_ROUGH), blk);
  hipLaunchKernelGGL((na_refine<SEL_ROUGH, 9, 11, false>), dim3(g_stream), b, 0, s, src, cells, state(SEL_ROUGH), hist(SEL_ROUGH, 4), blk, part);
  hipLaunchKernelGGL((na_select<SEL_ROUGH, 11, false, false>), one, b, 0, s, hist(SEL_ROUGH, 4), state(SEL_ROUGH), blk);
  hipLaunchKernelGGL((na_refine<SEL_ROUGH, 0, 9, false>), dim3(g_stream), b, 0, s, src, cells, state(SEL_ROUGH), hist(SEL_ROUGH, 5), blk, part);
  hipLaunchKernelGGL((na_select<SEL_ROUGH, 9, false, true>), one, b, 0, s, hist(SEL_ROUGH, 5), state(SEL_ROUGH), blk);

  // 3, 4: clusters, the per-column counts, the median cluster size
  hipLaunchKernelGGL(ccl_local, dim3(g_tiles), b, 0, s, labels, tg, parent, size, col_noise, col_valid);
  hipLaunchKernelGGL(ccl_merge, dim3(g_borders), b, 0, s, tg, parent);
  hipLaunchKernelGGL(ccl_flatten, dim3(g_cells), b, 0, s, cells, parent, size);
  hipLaunchKernelGGL(ccl_stats, dim3(g_stream), b, 0, s, cells, parent, size, hist(SEL_SIZE, 0), part);
  {
    FinishMap m{};
    map_run(m, 0, BGNN_NA_NUM_CLUSTERS, 2);
    map_run(m, 0, BGNN_NA_ISOLATED, 1 + BGNN_NA_SIZE_BINS);
    map_run(m, 3, BGNN_NA_MAX_CLUSTER, 1);
    hipLaunchKernelGGL(na_finish, one, fin, 0, s, part, g_stream, m, blk);
  }
  hipLaunchKernelGGL((na_select<SEL_SIZE, 11, true, false>), one, b, 0, s, hist(SEL_SIZE, 0), state(SEL_SIZE), blk);
  hipLaunchKernelGGL((na_refine<SEL_SIZE, 10, 11, false>), dim3(g_stream), b, 0, s, src, cells, state(SEL_SIZE), hist(SEL_SIZE, 1), blk, part);
  hipLaunchKernelGGL((na_select<SEL_SIZE, 11, false, false>), one, b, 0, s, hist(SEL_SIZE, 1), state(SEL_SIZE), blk);
  hipLaunchKernelGGL((na_refine<SEL_SIZE, 0, 10, false>), dim3(g_stream), b, 0, s, src, cells, state(SEL_SIZE), hist(SEL_SIZE, 2), blk, part);
  hipLaunchKernelGGL((na_select<SEL_SIZE, 10, false, true>), one, b, 0, s, hist(SEL_SIZE, 2), state(SEL_SIZE), blk);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
