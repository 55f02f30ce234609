// Exact percentiles of a stream of errors that stays in HBM (include/bgnn_quantile.h): the device half of the adaptive Huber delta.
//
//   qt_add      one memory-bound pass over correction, target and mask (9 B / row): |c - t| of every masked row as an
//               order-preserving uint32 key, appended to the caller's stage.  A workgroup takes shares of 4096 rows (16 per thread,
//               16-byte loads where the planes allow them) and reserves the slots of a share with ONE integer atomic on the cursor:
//               every wave ballots its 16 items, the four wave totals meet in LDS, thread 0 adds their sum to the cursor, and a
//               key's slot is that base + the waves before + the items before + the lanes before (prefix population counts).  A slot
//               at or beyond the capacity is counted as dropped and not written.  The same pass counts the top digit of every filed
//               key into an LDS histogram (hist_add) that is merged into the state with integer atomics (hist_flush): the first
//               level of the selection costs no pass of its own.
//   qt_refine   levels 1 and 2: a pass over the filed keys that counts the level's digit under the prefixes fixed so far
//               (radix_select.h, DigitCounter: up to six groups)
//   qt_select   one workgroup after every level: narrows prefix and rank of every rank (select_digit); level 0 sets the ranks
//               from the fractions and the total, level 2 writes the result block
//
// Everything that is added is an integer: counters, histogram and the selected keys do not depend on how the waves interleave;
// only the order of the stage does, and nothing reads it as an order.
//
// Compiled with -ffp-contract=off: c - t and (M - 1) * f round as written.
#include "bgnn_internal.h"
#include "radix_select.h"
#include "../../include/bgnn_quantile.h"

namespace bgnn {
namespace {

constexpr int QT_THREADS = BLOCK_THREADS;
constexpr int QT_WAVES = QT_THREADS / 64;
constexpr int QT_VEC = 4;                             // consecutive rows of one 16-byte load
constexpr int QT_GROUPS = 4;                          // such loads per thread and share
constexpr int QT_ITEMS = QT_VEC * QT_GROUPS;
constexpr int QT_GROUP_ROWS = QT_THREADS * QT_VEC;
constexpr int QT_SHARE = QT_THREADS * QT_ITEMS;
constexpr int QT_RANKS = 2 * BGNN_QUANTILE_MAX_FRACTIONS;
constexpr int QT_REFINE_ITEMS = 4;                    // keys per thread and step of a refine pass (each load coalesced)
constexpr int QT_REFINE_CHUNK = QT_THREADS * QT_REFINE_ITEMS;
using QtDigits = Digits<BGNN_QUANTILE_TOP_BITS, 11, 10>;
using QtState = SelectState<QT_RANKS, uint32_t>;
constexpr int QT_TOP_BINS = 1 << QtDigits::width(0);
static_assert(QtDigits::covers<uint32_t>(), "the digits cover the key");
static_assert(QT_SHARE == BGNN_QUANTILE_WG_ROWS, "the share the header documents");
static_assert(BGNN_QUANTILE_STATE_BYTES == BGNN_QUANTILE_ST_HIST + 4 * QT_TOP_BINS, "the state ends with the top digit's histogram");
static_assert(BGNN_QUANTILE_OUT_BYTES == BGNN_QUANTILE_OUT_RANKS + BGNN_QUANTILE_OUT_RANK_BYTES * BGNN_QUANTILE_MAX_FRACTIONS, "result block");

// workspace of a selection: the histograms of levels 1 and 2 (cleared by one memset), then the selection state
constexpr size_t QT_WS_LEVEL_WORDS = (size_t)QT_RANKS * (1 << 11);
constexpr size_t QT_WS_HIST_BYTES = (QtDigits::N - 1) * QT_WS_LEVEL_WORDS * 4;
constexpr size_t QT_WS_BYTES = QT_WS_HIST_BYTES + 256;
static_assert(sizeof(QtState) <= 256, "workspace slot of the selection state");

inline bool capacity_ok(int64_t capacity) { return capacity >= 1 && capacity < ((int64_t)1 << 32); }

template <bool VEC>
__device__ __forceinline__ void qt_load(const float *p, int64_t i, int64_t n, float (&v)[QT_VEC]) {
  if (VEC && i + QT_VEC <= n) {
    const float4 t = *reinterpret_cast<const float4 *>(p + i);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < QT_VEC; ++k) v[k] = i + k < n ? p[i + k] : 0.0f;
  }
}
template <bool VEC>
__device__ __forceinline__ void qt_load_mask(const uint8_t *p, int64_t i, int64_t n, bool (&m)[QT_VEC]) {
  if (VEC && i + QT_VEC <= n) {
    const uint32_t w = *reinterpret_cast<const uint32_t *>(p + i);
#pragma unroll
    for (int k = 0; k < QT_VEC; ++k) m[k] = ((w >> (8 * k)) & 0xFFu) != 0;
  } else {
#pragma unroll
    for (int k = 0; k < QT_VEC; ++k) m[k] = i + k < n && p[i + k] != 0;
  }
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct AddLds {
  int32_t hist[QT_TOP_BINS];
  unsigned long long counters[4];          // rows, filed, nonfinite, dropped of this workgroup
  unsigned long long base;                 // the share's first slot
  uint32_t wave_total[QT_WAVES];
};

// VEC: correction and target are 16-byte aligned, the mask 4-byte aligned.  TARGET / MASK: the plane is given.
template <bool VEC, bool TARGET, bool MASK>
__global__ __launch_bounds__(QT_THREADS) void qt_add(const float *__restrict__ correction, const float *__restrict__ target,
                                                     const uint8_t *__restrict__ mask, int64_t n, uint32_t *__restrict__ stage,
                                                     unsigned long long capacity, char *__restrict__ state) {
  __shared__ AddLds s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int b = t; b < QT_TOP_BINS; b += QT_THREADS) s.hist[b] = 0;
  if (t < 4) s.counters[t] = 0;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long *cursor = reinterpret_cast<unsigned long long *>(state + BGNN_QUANTILE_ST_CURSOR);
  uint32_t rows = 0, filed = 0, nonfinite = 0, dropped = 0;          // (per thread: at most n / threads of the grid + 16)
  for (int64_t share = (int64_t)blockIdx.x * QT_SHARE; share < n; share += (int64_t)gridDim.x * QT_SHARE) {
    uint32_t key[QT_ITEMS];
    uint32_t ok = 0;                                             // bit k: item k is filed or dropped (one register, not 16 lane masks)
#pragma unroll
    for (int g = 0; g < QT_GROUPS; ++g) {
      const int64_t i = share + (int64_t)g * QT_GROUP_ROWS + (int64_t)t * QT_VEC;       // (i may pass n: every load checks)
      float c[QT_VEC], d[QT_VEC];
      bool m[QT_VEC];
      qt_load<VEC>(correction, i, n, c);
      if (TARGET) qt_load<VEC>(target, i, n, d);
      if (MASK) qt_load_mask<VEC>(mask, i, n, m);
#pragma unroll
      for (int k = 0; k < QT_VEC; ++k) {
        const bool in = i + k < n && (!MASK || m[k]);
        const float e = TARGET ? fabsf(c[k] - d[k]) : c[k];
        const bool fin = finite_bits(e);
        key[g * QT_VEC + k] = order_key(e);
        ok |= (uint32_t)(in && fin) << (g * QT_VEC + k);
        rows += in;
        nonfinite += in && !fin;
      }
    }
    // the slots of this share: one atomic of the workgroup
    uint32_t wave_count = 0;
#pragma unroll
    for (int k = 0; k < QT_ITEMS; ++k) wave_count += (uint32_t)__popcll(__ballot((ok >> k) & 1u));
    __syncthreads();                                             // (the previous share's readers of base and wave_total are done)
    if (lane == 0) s.wave_total[wave] = wave_count;
    __syncthreads();
    if (t == 0) {
      uint32_t total = 0;
#pragma unroll
      for (int w = 0; w < QT_WAVES; ++w) total += s.wave_total[w];
      s.base = total ? atomicAdd(cursor, (unsigned long long)total) : 0ull;
    }
    __syncthreads();
    unsigned long long slot0 = s.base;
    for (int w = 0; w < wave; ++w) slot0 += s.wave_total[w];
#pragma unroll
    for (int k = 0; k < QT_ITEMS; ++k) {
      const bool mine = (ok >> k) & 1u;
      const unsigned long long votes = __ballot(mine);           // (the same ballot as above: nothing is kept across the barriers)
      const unsigned long long slot = slot0 + (unsigned long long)__popcll(votes & below);
      const bool keep = mine && slot < capacity;
      if (keep) stage[slot] = key[k];                            // slot < capacity: inside the stage
      filed += keep;
      dropped += mine && !keep;
      hist_add(s.hist, keep, key[k] >> QtDigits::shift(0));
      slot0 += (unsigned long long)__popcll(votes);
    }
  }
  const uint32_t sums[4] = {wave_sum_u32(rows), wave_sum_u32(filed), wave_sum_u32(nonfinite), wave_sum_u32(dropped)};
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (sums[k]) atomicAdd(&s.counters[k], (unsigned long long)sums[k]);
  }
  __syncthreads();
  hist_flush(s.hist, QT_TOP_BINS, reinterpret_cast<uint32_t *>(state + BGNN_QUANTILE_ST_HIST));
  if (t < 4 && s.counters[t]) atomicAdd(reinterpret_cast<unsigned long long *>(state) + t, s.counters[t]);
}
static_assert(BGNN_QUANTILE_ST_ROWS == 0 && BGNN_QUANTILE_ST_FILED == 8 && BGNN_QUANTILE_ST_NONFINITE == 16 && BGNN_QUANTILE_ST_DROPPED == 24,
              "the order of qt_add's counters");

// the filed keys: the state's count, never more than the stage holds
__device__ __forceinline__ int64_t filed_keys(const char *state, int64_t capacity) {
  const int64_t m = *reinterpret_cast<const int64_t *>(state + BGNN_QUANTILE_ST_FILED);
  return m < 0 ? 0 : (m > capacity ? capacity : m);
}

template <int LEVEL>
__global__ __launch_bounds__(QT_THREADS) void qt_refine(const uint32_t *__restrict__ stage, int64_t capacity, const char *__restrict__ state,
                                                        const QtState *__restrict__ sel, uint32_t *__restrict__ hist) {
  using Counter = DigitCounter<QT_RANKS, uint32_t, QtDigits::shift(LEVEL), QtDigits::width(LEVEL)>;
  __shared__ int32_t lds[QT_RANKS * Counter::BINS];
  Counter counter;
  counter.init(sel, lds);
  const int64_t m = filed_keys(state, capacity);
  for (int64_t base = (int64_t)blockIdx.x * QT_REFINE_CHUNK; base < m; base += (int64_t)gridDim.x * QT_REFINE_CHUNK) {
#pragma unroll
    for (int k = 0; k < QT_REFINE_ITEMS; ++k) {
      const int64_t i = base + k * QT_THREADS + threadIdx.x;
      const bool ok = i < m;
      counter.add(ok, ok ? stage[i] : 0u);
    }
  }
  counter.flush(hist);
}

struct Fractions {
  double f[BGNN_QUANTILE_MAX_FRACTIONS];
  int32_t n;
};

template <int LEVEL>
__global__ __launch_bounds__(QT_THREADS) void qt_select(const uint32_t *__restrict__ hist, QtState *sel, const char *__restrict__ state,
                                                        Fractions fr, char *__restrict__ out) {
  __shared__ SelectScratch<QT_RANKS, uint32_t> sh;
  select_digit<LEVEL == 0, QtDigits::width(LEVEL)>(hist, sel, sh, 2 * fr.n, [&fr](const int64_t *part, int64_t *rank) {
    const int64_t m = part[QT_THREADS];
    if (m <= 0) return;
    for (int k = 0; k < fr.n; ++k) {
      const double vi = (double)(m - 1) * fr.f[k];
      int64_t lo = (int64_t)floor(vi);
      lo = lo < 0 ? 0 : (lo > m - 1 ? m - 1 : lo);                // (f in [0, 1]: already inside)
      rank[2 * k] = lo;
      rank[2 * k + 1] = lo + 1 < m - 1 ? lo + 1 : m - 1;
    }
  });
  if (LEVEL == QtDigits::N - 1 && threadIdx.x == 0) {
    const QtState &o = sh.out;
    int64_t *head = reinterpret_cast<int64_t *>(out);
    head[0] = *reinterpret_cast<const int64_t *>(state + BGNN_QUANTILE_ST_FILED);
    head[1] = *reinterpret_cast<const int64_t *>(state + BGNN_QUANTILE_ST_NONFINITE);
    head[2] = *reinterpret_cast<const int64_t *>(state + BGNN_QUANTILE_ST_DROPPED);
    head[3] = *reinterpret_cast<const int64_t *>(state + BGNN_QUANTILE_ST_ROWS);
    for (int k = 0; k < BGNN_QUANTILE_MAX_FRACTIONS; ++k) {
      char *rec = out + BGNN_QUANTILE_OUT_RANKS + BGNN_QUANTILE_OUT_RANK_BYTES * k;
      for (int j = 0; j < 2; ++j) {
        const int r = 2 * k + j;
        const bool have = k < fr.n && o.rank[r] >= 0;
        reinterpret_cast<int64_t *>(rec)[j] = have ? o.rank0[r] : -1;
        reinterpret_cast<uint32_t *>(rec + 16)[j] = have ? __float_as_uint(key_value(o.prefix[r])) : 0x7FC00000u;
      }
    }
  }
}

template <bool VEC, bool TARGET>
void launch_add(bool mask, dim3 g, hipStream_t s, const float *c, const float *t, const uint8_t *m, int64_t n, uint32_t *stage,
                int64_t capacity, char *state) {
  const dim3 b(QT_THREADS);
  const unsigned long long cap = (unsigned long long)capacity;
  if (mask) hipLaunchKernelGGL((qt_add<VEC, TARGET, true>), g, b, 0, s, c, t, m, n, stage, cap, state);
  else hipLaunchKernelGGL((qt_add<VEC, TARGET, false>), g, b, 0, s, c, t, m, n, stage, cap, state);
}

}  // namespace
}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_quantile_workspace_bytes(int64_t capacity) { return capacity_ok(capacity) ? QT_WS_BYTES : 0; }

extern "C" int bgnn_quantile_reset(bgnn_ctx *ctx, void *state) {
  // (the context last: what is wrong with the other arguments is reported whatever the context)
  BGNN_REQUIRE(state, "bgnn_quantile_reset: NULL argument");
  BGNN_REQUIRE(((uintptr_t)state & 7) == 0, "bgnn_quantile_reset: the state block is not 8-byte aligned");
  BGNN_REQUIRE(ctx, "bgnn_quantile_reset: NULL context");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  BGNN_HIP_CHECK(hipMemsetAsync(state, 0, BGNN_QUANTILE_STATE_BYTES, ctx->stream));
  return BGNN_OK;
}

extern "C" int bgnn_quantile_add(bgnn_ctx *ctx, int64_t n, const float *correction, const float *target, const uint8_t *mask,
                                 uint32_t *stage, int64_t capacity, void *state) {
  BGNN_REQUIRE(correction && stage && state, "bgnn_quantile_add: NULL argument");
  BGNN_REQUIRE(n >= 0, "bgnn_quantile_add: %lld rows", (long long)n);
  BGNN_REQUIRE(capacity_ok(capacity), "bgnn_quantile_add: a capacity of %lld, 1 .. 2^32 - 1 expected", (long long)capacity);
  BGNN_REQUIRE(((uintptr_t)stage & 3) == 0, "bgnn_quantile_add: the stage is not 4-byte aligned");
  BGNN_REQUIRE(((uintptr_t)correction & 3) == 0 && ((uintptr_t)target & 3) == 0, "bgnn_quantile_add: a plane is not 4-byte aligned");
  BGNN_REQUIRE(((uintptr_t)state & 7) == 0, "bgnn_quantile_add: the state block is not 8-byte aligned");
  BGNN_REQUIRE(ctx, "bgnn_quantile_add: NULL context");
  if (n == 0) return BGNN_OK;
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const dim3 g(capped_grid((n + QT_SHARE - 1) / QT_SHARE, BGNN_QUANTILE_MAX_GRID));
  const bool vec = ((uintptr_t)correction & 15) == 0 && ((uintptr_t)target & 15) == 0 && ((uintptr_t)mask & 3) == 0;
  char *st = static_cast<char *>(state);
  if (target) {
    if (vec) launch_add<true, true>(mask != nullptr, g, ctx->stream, correction, target, mask, n, stage, capacity, st);
    else launch_add<false, true>(mask != nullptr, g, ctx->stream, correction, target, mask, n, stage, capacity, st);
  } else {
    if (vec) launch_add<true, false>(mask != nullptr, g, ctx->stream, correction, target, mask, n, stage, capacity, st);
    else launch_add<false, false>(mask != nullptr, g, ctx->stream, correction, target, mask, n, stage, capacity, st);
  }
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

extern "C" int bgnn_quantile_select(bgnn_ctx *ctx, const uint32_t *stage, int64_t capacity, const void *state, const double *fractions,
                                    int32_t n_fractions, void *workspace, size_t workspace_bytes, void *out) {
  BGNN_REQUIRE(stage && state && fractions && workspace && out, "bgnn_quantile_select: NULL argument");
  BGNN_REQUIRE(capacity_ok(capacity), "bgnn_quantile_select: a capacity of %lld, 1 .. 2^32 - 1 expected", (long long)capacity);
  BGNN_REQUIRE(n_fractions >= 1 && n_fractions <= BGNN_QUANTILE_MAX_FRACTIONS, "bgnn_quantile_select: %d fractions, 1 .. %d expected",
               (int)n_fractions, BGNN_QUANTILE_MAX_FRACTIONS);
  Fractions fr{};
  fr.n = n_fractions;
  for (int k = 0; k < n_fractions; ++k) {
    BGNN_REQUIRE(fractions[k] >= 0.0 && fractions[k] <= 1.0, "bgnn_quantile_select: fraction %d is %g, outside [0, 1]", k, fractions[k]);
    fr.f[k] = fractions[k];
  }
  BGNN_REQUIRE(((uintptr_t)stage & 3) == 0, "bgnn_quantile_select: the stage is not 4-byte aligned");
  BGNN_REQUIRE(((uintptr_t)state & 7) == 0, "bgnn_quantile_select: the state block is not 8-byte aligned");
  BGNN_REQUIRE(((uintptr_t)workspace & 7) == 0, "bgnn_quantile_select: the workspace is not 8-byte aligned");
  BGNN_REQUIRE(((uintptr_t)out & 7) == 0, "bgnn_quantile_select: the result block is not 8-byte aligned");
  BGNN_REQUIRE(workspace_bytes >= QT_WS_BYTES, "bgnn_quantile_select: workspace of %zu bytes, %zu needed", workspace_bytes, QT_WS_BYTES);
  BGNN_REQUIRE(ctx, "bgnn_quantile_select: NULL context");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  char *w = static_cast<char *>(workspace), *o = static_cast<char *>(out);
  const char *st = static_cast<const char *>(state);
  uint32_t *lower = reinterpret_cast<uint32_t *>(w);
  QtState *sel = reinterpret_cast<QtState *>(w + QT_WS_HIST_BYTES);
  const dim3 b(QT_THREADS), one(1), g(capped_grid((capacity + QT_REFINE_CHUNK - 1) / QT_REFINE_CHUNK, BGNN_QUANTILE_MAX_GRID));
  BGNN_HIP_CHECK(hipMemsetAsync(w, 0, QT_WS_BYTES, s));
  hipLaunchKernelGGL(qt_select<0>, one, b, 0, s, reinterpret_cast<const uint32_t *>(st + BGNN_QUANTILE_ST_HIST), sel, st, fr, o);
  hipLaunchKernelGGL(qt_refine<1>, g, b, 0, s, stage, capacity, st, sel, lower);
  hipLaunchKernelGGL(qt_select<1>, one, b, 0, s, lower, sel, st, fr, o);
  hipLaunchKernelGGL(qt_refine<2>, g, b, 0, s, stage, capacity, st, sel, lower + QT_WS_LEVEL_WORDS);
  hipLaunchKernelGGL(qt_select<2>, one, b, 0, s, lower + QT_WS_LEVEL_WORDS, sel, st, fr, o);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
