// Operating curves of a classified survey against its ground truth (include/bgnn_curve.h): one memory-bound pass over five
// planes (20 B / cell; 12 B without the residual planes) that files every counted cell under its confidence code, so that the host
// reads every threshold of the table off one histogram.
//
//   curve_pass   a workgroup keeps the whole block as an LDS histogram (uint32 counts, 64-bit fixed-point sums: 38 KB, four
//                workgroups per CU), strides over its shares of 1024 cells, and adds its non-zero entries into the block with
//                global integer atomics at the end.  The threshold table sits in LDS padded to 256 entries with +inf: the code of
//                a confidence is a branch-free lower bound of 8 steps.
//
// Real confidences cluster, so most lanes of a wave hit one LDS address: two rounds peel the key of the first lane still active
// (ballot, one add of the population count by that lane; the fixed-point sums of a large group by a butterfly); what is left adds
// for itself.  All entries are integers: the order of the adds does not show in the result.
//
// Compiled with -ffp-contract=off: difference - correction and the fixed-point product round as written.
#include "bgnn_internal.h"
#include "plane_util.h"
#include "../../include/bgnn_curve.h"

namespace bgnn {

constexpr int CV_THREADS = BLOCK_THREADS;
constexpr int CV_ITEMS = 4;                          // consecutive cells per thread and step: one 16-byte load per plane
constexpr int CV_TILE = CV_THREADS * CV_ITEMS;
constexpr int CV_MAX_T = BGNN_CURVE_MAX_THRESHOLDS;
constexpr int CV_MAX_CODES = BGNN_CURVE_CODES(CV_MAX_T);
constexpr int CV_TABLE = 2 * CV_MAX_T;               // the padded table: lower-bound steps 128, 64 .. 1 stay inside it
constexpr int CV_PEEL_ROUNDS = 2;
constexpr int CV_BUTTERFLY_MIN = 16;                 // lanes of one residual entry from which a wave sum beats their own adds
static_assert(CV_TILE == BGNN_CURVE_WG_CELLS, "the share the header documents");
static_assert(CV_THREADS == 256 && CV_TABLE == 256, "one table entry per thread");

struct CurveLds {
  unsigned long long before[CV_MAX_CODES * 4], after[CV_MAX_CODES * 4], base_abs[4];
  uint32_t counts[CV_MAX_CODES * 16], res_cells[CV_MAX_CODES * 4], base_cells[4], skipped;
  float thr[CV_TABLE];
};
static_assert(sizeof(CurveLds) <= 40 * 1024, "four workgroups per CU");

static inline int curve_grid(int64_t cells) { return capped_grid((cells + CV_TILE - 1) / CV_TILE, BGNN_CURVE_MAX_GRID); }

template <bool VEC, typename T>
__device__ __forceinline__ void curve_load(const T *p, int64_t i, int64_t n, T (&v)[CV_ITEMS], T fill) {
  static_assert(sizeof(T) == 4 && CV_ITEMS == 4, "one 16-byte access");
  if (VEC && i + CV_ITEMS <= n) {
    const uint4 t = *reinterpret_cast<const uint4 *>(p + i);
    const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int k = 0; k < CV_ITEMS; ++k) __builtin_memcpy(&v[k], &w[k], 4);
  } else {
#pragma unroll
    for (int k = 0; k < CV_ITEMS; ++k) v[k] = i + k < n ? p[i + k] : fill;
  }
}

// 2 * #{k : t_k < c} + [c == t_k], 2T + 1 for NaN: in 0 .. 2T + 1 for every bit pattern of c and of the table
__device__ __forceinline__ int confidence_code(const float *thr, int T, float c) {
  if (c != c) return 2 * T + 1;
  int lo = 0;
#pragma unroll
  for (int step = CV_TABLE / 2; step > 0; step >>= 1)
    if (thr[lo + step - 1] < c) lo += step;          // (lo + step - 1 <= 254)
  lo = lo < T ? lo : T;
  return 2 * lo + (lo < T && thr[lo] == c ? 1 : 0);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ uint32_t fixed_point(float magnitude) {      // magnitude in [0, 32768): below 2^31
  return (uint32_t)llrint((double)magnitude * (double)BGNN_CURVE_RES_SCALE);
}

// One cell per lane into the LDS histogram.  key = code * 16 + true class * 4 + predicted class; res: the cell enters the residual
// entry (code, true class).  Every lane of the wave calls this.
template <bool RES>
__device__ __forceinline__ void file_cell(CurveLds &s, bool counted, int key, bool res, uint32_t qb, uint32_t qa) {
  const int lane = threadIdx.x & 63;
  bool active = counted;
#pragma unroll
  for (int round = 0; round < CV_PEEL_ROUNDS; ++round) {
    const unsigned long long m = __ballot(active);
    if (m == 0) break;                                         // (wave-uniform)
    const int leader = __ffsll(m) - 1;
    const int k0 = __shfl(key, leader);
    const bool grp = active && key == k0;
    const uint32_t n = (uint32_t)__popcll(__ballot(grp));
    if (lane == leader) atomicAdd(&s.counts[k0], n);
    if (RES) {
      const bool r = grp && res;
      const uint32_t rn = (uint32_t)__popcll(__ballot(r));
      const int ri = (k0 >> 4) * 4 + ((k0 >> 2) & 3);
      if (rn >= CV_BUTTERFLY_MIN) {                            // (wave-uniform)
        const unsigned long long b = wave_sum(r ? qb : 0u), a = wave_sum(r ? qa : 0u);
        if (lane == leader) {
          atomicAdd(&s.res_cells[ri], rn);
          atomicAdd(&s.before[ri], b);
          atomicAdd(&s.after[ri], a);
        }
      } else if (r) {
        atomicAdd(&s.res_cells[ri], 1u);
        atomicAdd(&s.before[ri], (unsigned long long)qb);
        atomicAdd(&s.after[ri], (unsigned long long)qa);
      }
    }
    active = active && !grp;
  }
  if (active) {
    atomicAdd(&s.counts[key], 1u);
    if (RES && res) {
      const int ri = (key >> 4) * 4 + ((key >> 2) & 3);
      atomicAdd(&s.res_cells[ri], 1u);
      atomicAdd(&s.before[ri], (unsigned long long)qb);
      atomicAdd(&s.after[ri], (unsigned long long)qa);
    }
  }
}

__device__ __forceinline__ void flush(unsigned long long v, int64_t *dst) {
  if (v) atomicAdd(reinterpret_cast<unsigned long long *>(dst), v);
}

template <bool VEC, bool RES>
__global__ __launch_bounds__(CV_THREADS) void curve_pass(const float *__restrict__ thresholds, int T, const int32_t *__restrict__ labels,
                                                         const float *__restrict__ pred, const float *__restrict__ conf,
                                                         const float *__restrict__ diff, const float *__restrict__ corr, int64_t cells,
                                                         char *__restrict__ block) {
  __shared__ CurveLds s;
  const int t = threadIdx.x;
  const int codes = BGNN_CURVE_CODES(T);                       // T in 1 .. 128 (checked by the entry point): codes <= CV_MAX_CODES
  for (int i = t; i < codes * 16; i += CV_THREADS) s.counts[i] = 0;
  for (int i = t; i < codes * 4; i += CV_THREADS) { s.res_cells[i] = 0; s.before[i] = 0; s.after[i] = 0; }
  if (t < 4) { s.base_cells[t] = 0; s.base_abs[t] = 0; }
  if (t == 0) s.skipped = 0;
  s.thr[t] = t < T ? thresholds[t] : __uint_as_float(0x7F800000u);
  __syncthreads();

  uint32_t base_n[4] = {0, 0, 0, 0}, skipped = 0;
  unsigned long long base_q[4] = {0, 0, 0, 0};
  const float nan = __uint_as_float(0x7FC00000u), cap = (float)BGNN_CURVE_RES_CAP;
  for (int64_t base = (int64_t)blockIdx.x * CV_TILE; base < cells; base += (int64_t)gridDim.x * CV_TILE) {
    const int64_t i = base + (int64_t)t * CV_ITEMS;
    int32_t lab[CV_ITEMS];
    float p[CV_ITEMS], c[CV_ITEMS], d[CV_ITEMS], r[CV_ITEMS];
    curve_load<VEC>(labels, i, cells, lab, (int32_t)-1);
    curve_load<VEC>(pred, i, cells, p, nan);
    curve_load<VEC>(conf, i, cells, c, nan);
    if (RES) {
      curve_load<VEC>(diff, i, cells, d, nan);
      curve_load<VEC>(corr, i, cells, r, nan);
    }
#pragma unroll
    for (int k = 0; k < CV_ITEMS; ++k) {
      const bool counted = lab[k] >= 0 && p[k] >= 0.0f && finite_bits(p[k]);
      const int row = lab[k] < 0 ? 0 : (lab[k] < 3 ? lab[k] : 3);
      const int col = p[k] >= 0.0f && p[k] < 3.0f ? (int)p[k] : 3;
      const int key = confidence_code(s.thr, T, c[k]) * 16 + row * 4 + col;
      bool res = false;
      uint32_t qb = 0, qa = 0;
      if (RES) {
        const float mag = fabsf(d[k]), left = fabsf(d[k] - r[k]);
        const bool has_base = counted && mag < cap;            // (false for NaN and inf)
        res = has_base && col == 2 && left < cap;
        qb = has_base ? fixed_point(mag) : 0u;
        qa = res ? fixed_point(left) : 0u;
        skipped += counted && !has_base;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool mine = has_base && row == j;
          base_n[j] += mine;
          base_q[j] += mine ? qb : 0u;
        }
      }
      file_cell<RES>(s, counted, key, res, qb, qa);
    }
  }
  if (RES) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (base_n[j]) { atomicAdd(&s.base_cells[j], base_n[j]); atomicAdd(&s.base_abs[j], base_q[j]); }
    }
    if (skipped) atomicAdd(&s.skipped, skipped);
  }
  __syncthreads();

  int64_t *counts = reinterpret_cast<int64_t *>(block + BGNN_CURVE_COUNTS(T));
  for (int i = t; i < codes * 16; i += CV_THREADS) flush(s.counts[i], counts + i);
  if (RES) {
    int64_t *res_cells = reinterpret_cast<int64_t *>(block + BGNN_CURVE_RES_CELLS(T));
    int64_t *before = reinterpret_cast<int64_t *>(block + BGNN_CURVE_ABS_BEFORE(T));
    int64_t *after = reinterpret_cast<int64_t *>(block + BGNN_CURVE_ABS_AFTER(T));
    for (int i = t; i < codes * 4; i += CV_THREADS) {
      flush(s.res_cells[i], res_cells + i);
      flush(s.before[i], before + i);
      flush(s.after[i], after + i);
    }
    if (t < 4) {
      flush(s.base_cells[t], reinterpret_cast<int64_t *>(block + BGNN_CURVE_BASE_CELLS(T)) + t);
      flush(s.base_abs[t], reinterpret_cast<int64_t *>(block + BGNN_CURVE_BASE_ABS(T)) + t);
    }
    if (t == 0) flush(s.skipped, reinterpret_cast<int64_t *>(block + BGNN_CURVE_RES_SKIPPED(T)));
  }
}

static inline bool curve_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
static inline bool curve_table_ok(int n) { return n >= 1 && n <= CV_MAX_T; }

}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_curve_block_bytes(int n_thresholds) {
  return curve_table_ok(n_thresholds) ? (size_t)BGNN_CURVE_BLOCK_BYTES(n_thresholds) : 0;
}

extern "C" int bgnn_curve_reset(bgnn_ctx *ctx, void *block, int n_thresholds) {
  // (the context last: what is wrong with the other arguments is reported whatever the context)
  BGNN_REQUIRE(block, "bgnn_curve_reset: NULL argument");
  BGNN_REQUIRE(curve_table_ok(n_thresholds), "bgnn_curve_reset: %d thresholds, 1 .. %d expected", n_thresholds, CV_MAX_T);
  BGNN_REQUIRE(((uintptr_t)block & 7) == 0, "bgnn_curve_reset: the block is not 8-byte aligned");
  BGNN_REQUIRE(ctx, "bgnn_curve_reset: NULL context");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  BGNN_HIP_CHECK(hipMemsetAsync(block, 0, bgnn_curve_block_bytes(n_thresholds), ctx->stream));
  return BGNN_OK;
}

extern "C" int bgnn_curve_accumulate(bgnn_ctx *ctx, const float *thresholds, int n_thresholds, const int32_t *labels, const float *pred,
                                     const float *confidence, const float *difference, const float *correction, int64_t cells,
                                     void *block) {
  BGNN_REQUIRE(thresholds && labels && pred && confidence && block, "bgnn_curve_accumulate: NULL argument");
  BGNN_REQUIRE(curve_table_ok(n_thresholds), "bgnn_curve_accumulate: %d thresholds, 1 .. %d expected", n_thresholds, CV_MAX_T);
  BGNN_REQUIRE((difference == nullptr) == (correction == nullptr),
               "bgnn_curve_accumulate: difference and correction must both be given or both be NULL");
  BGNN_REQUIRE(cells >= 0 && cells <= ((int64_t)1 << 32), "bgnn_curve_accumulate: %lld cells", (long long)cells);
  BGNN_REQUIRE(((uintptr_t)block & 7) == 0, "bgnn_curve_accumulate: the block is not 8-byte aligned");
  BGNN_REQUIRE(ctx, "bgnn_curve_accumulate: NULL context");
  if (cells == 0) return BGNN_OK;
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const dim3 g(curve_grid(cells)), b(CV_THREADS);
  char *blk = static_cast<char *>(block);
  const bool vec = curve_aligned16(labels) && curve_aligned16(pred) && curve_aligned16(confidence) &&
                   (!difference || (curve_aligned16(difference) && curve_aligned16(correction)));
  hipStream_t s = ctx->stream;
  const int T = n_thresholds;
  if (difference) {
    if (vec) hipLaunchKernelGGL((curve_pass<true, true>), g, b, 0, s, thresholds, T, labels, pred, confidence, difference, correction, cells, blk);
    else hipLaunchKernelGGL((curve_pass<false, true>), g, b, 0, s, thresholds, T, labels, pred, confidence, difference, correction, cells, blk);
  } else {
    if (vec) hipLaunchKernelGGL((curve_pass<true, false>), g, b, 0, s, thresholds, T, labels, pred, confidence, difference, correction, cells, blk);
    else hipLaunchKernelGGL((curve_pass<false, false>), g, b, 0, s, thresholds, T, labels, pred, confidence, difference, correction, cells, blk);
  }
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
