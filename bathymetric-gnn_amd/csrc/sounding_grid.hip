// Gridding a point cloud of soundings (include/bgnn_soundings.h): count, mean, standard deviation, minimum and maximum per cell
// from one pass over (x, y, z), 20 B per sounding, bound by the scattered atomics into the cells.
//
//   sounding_pass<UniformAddress, FileSink>
//                       the cloud pass of sounding_pass.h: grid-stride over shares of 1024 soundings, four per thread loaded before
//                       any is filed.  A sounding is classified (sounding_file.h: not finite / outside / out of range /
//                       accepted) and an accepted one goes into its cell with six global integer atomics: n, S1 = sum q, the low
//                       and the high words of q^2, and the two extremes under the order-preserving map of float32 onto uint32.
//                       The minimum is kept as the maximum of the inverted key, so an all-zero state is the empty one.  A swath
//                       puts runs of consecutive soundings into one cell: a run of neighbouring lanes on one cell is summed
//                       towards its first lane inside the wave (a segmented halving over shuffles, skipped where no two
//                       neighbours of the wave share a cell) and only that lane goes to memory -- measured on 2e8 soundings:
//                       9.2 ms against 60.7 ms in swath order, 49.6 ms either way when scattered.  The four counters are reduced
//                       per workgroup (block_reduce) and added with one atomic per workgroup and counter.
//   soundings_finalize  one thread per cell: the variance numerator n * S2 - S1^2 is formed exactly in 128 bits and rounded once
//                       to float64 (its low bits folded into a sticky bit of the top 64: there is no 128-bit conversion on the
//                       device).  Reads the state only.
//   extent_partial      float64 min / max of the finite x and y: per thread, then the fixed halving tree, one record per
//   extent_finish       workgroup; a second launch of one workgroup finishes the records.
//
// All sums are integers: the order of the atomics does not show in the result.  Compiled with -ffp-contract=off: the cell index
// and the finalisation round operation by operation as the header states them.
#include "bgnn_internal.h"
#include "sounding_args.h"
#include "sounding_moments.h"
#include "sounding_pass.h"

namespace bgnn {

constexpr int SG_THREADS = BLOCK_THREADS;
constexpr int SG_FINALIZE_MAX_GRID = 1 << 20;
constexpr int SG_EXTENT_SHARE = 4 * SG_THREADS;        // soundings per workgroup of extent_partial, up to its grid cap

struct ExtentRecord {
  double min_x, max_x, min_y, max_y;
  long long finite_x, finite_y;
};
static_assert(sizeof(ExtentRecord) == BGNN_SOUNDINGS_EXTENT_BYTES, "the record the header documents");

__global__ __launch_bounds__(SG_THREADS) void soundings_finalize(const char *__restrict__ state, int64_t n_cells, int32_t min_count,
                                                                 float nodata, int32_t *__restrict__ count, float *__restrict__ mean,
                                                                 float *__restrict__ stdev, float *__restrict__ zmin,
                                                                 float *__restrict__ zmax, uint8_t *__restrict__ valid) {
  const SoundingCell *cells = reinterpret_cast<const SoundingCell *>(state + BGNN_SOUNDINGS_HEADER_BYTES);
  for (int64_t i = (int64_t)blockIdx.x * SG_THREADS + threadIdx.x; i < n_cells; i += (int64_t)gridDim.x * SG_THREADS) {
    const SoundingCell c = cells[i];
    const bool ok = c.n >= (uint32_t)min_count;       // (min_count >= 1: an empty cell is never valid)
    float m = nodata, s = nodata, lo = nodata, hi = nodata;
    if (ok) {
      m = sounding_mean(c.n, c.s1);                    // (sounding_moments.h: the exact numerator rounded once to float64)
      s = sounding_std(c.n, c.s1, c.s2_lo, c.s2_hi);
      lo = order_value(~c.min_inv);
      hi = order_value(c.max_key);
    }
    count[i] = (int32_t)c.n;
    mean[i] = m;
    stdev[i] = s;
    zmin[i] = lo;
    zmax[i] = hi;
    valid[i] = ok ? 1 : 0;
  }
}

struct MinOp {
  __device__ __forceinline__ double operator()(double a, double b) const { return b < a ? b : a; }
};
struct MaxOp {
  __device__ __forceinline__ double operator()(double a, double b) const { return b > a ? b : a; }
};

// every thread holds a record; the workgroup's record lands in *out (thread 0 writes)
__device__ __forceinline__ void extent_reduce_store(const ExtentRecord &r, ExtentRecord *out) {
  __shared__ double scratch[SG_THREADS];
  ExtentRecord w;
  w.min_x = block_reduce(r.min_x, scratch, MinOp());
  w.max_x = block_reduce(r.max_x, scratch, MaxOp());
  w.min_y = block_reduce(r.min_y, scratch, MinOp());
  w.max_y = block_reduce(r.max_y, scratch, MaxOp());
  w.finite_x = block_reduce(r.finite_x, scratch, SumOp());
  w.finite_y = block_reduce(r.finite_y, scratch, SumOp());
  if (threadIdx.x == 0) *out = w;
}

__device__ __forceinline__ ExtentRecord extent_empty() {
  const double inf = __longlong_as_double(0x7FF0000000000000LL);
  return ExtentRecord{inf, -inf, inf, -inf, 0, 0};
}

__global__ __launch_bounds__(SG_THREADS) void extent_partial(const double *__restrict__ xs, const double *__restrict__ ys, int64_t n,
                                                             ExtentRecord *__restrict__ partials) {
  ExtentRecord r = extent_empty();
  for (int64_t i = (int64_t)blockIdx.x * SG_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SG_THREADS) {
    const double x = xs[i], y = ys[i];
    if (finite_bits64(x)) { r.min_x = MinOp()(r.min_x, x); r.max_x = MaxOp()(r.max_x, x); ++r.finite_x; }
    if (finite_bits64(y)) { r.min_y = MinOp()(r.min_y, y); r.max_y = MaxOp()(r.max_y, y); ++r.finite_y; }
  }
  extent_reduce_store(r, partials + blockIdx.x);
}

__global__ __launch_bounds__(SG_THREADS) void extent_finish(const ExtentRecord *__restrict__ partials, int n_partials,
                                                            ExtentRecord *__restrict__ out) {
  ExtentRecord r = extent_empty();
  for (int p = threadIdx.x; p < n_partials; p += SG_THREADS) {
    const ExtentRecord q = partials[p];
    r.min_x = MinOp()(r.min_x, q.min_x); r.max_x = MaxOp()(r.max_x, q.max_x);
    r.min_y = MinOp()(r.min_y, q.min_y); r.max_y = MaxOp()(r.max_y, q.max_y);
    r.finite_x += q.finite_x; r.finite_y += q.finite_y;
  }
  extent_reduce_store(r, out);
}

}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_soundings_state_bytes(int64_t height, int64_t width) {
  if (!dim_ok(height) || !dim_ok(width)) return 0;
  const unsigned __int128 bytes = (unsigned __int128)height * (unsigned __int128)width * BGNN_SOUNDINGS_CELL_BYTES + BGNN_SOUNDINGS_HEADER_BYTES;
  return bytes > (unsigned __int128)SIZE_MAX ? 0 : (size_t)bytes;
}

extern "C" int bgnn_soundings_reset(bgnn_ctx *ctx, void *state, int64_t height, int64_t width) {
  // (the context last: what is wrong with the other arguments is reported whatever the context)
  BGNN_REQUIRE(state, "bgnn_soundings_reset: NULL argument");
  BGNN_TRY(require_grid("bgnn_soundings_reset", height, width, "grid", 0, ""));
  BGNN_REQUIRE(bgnn_soundings_state_bytes(height, width) != 0, "bgnn_soundings_reset: the state of %lld x %lld cells exceeds size_t",
               (long long)height, (long long)width);
  BGNN_REQUIRE(aligned8(state), "bgnn_soundings_reset: the state is not 8-byte aligned");
  BGNN_REQUIRE(ctx, "bgnn_soundings_reset: NULL context");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  BGNN_HIP_CHECK(hipMemsetAsync(state, 0, bgnn_soundings_state_bytes(height, width), ctx->stream));
  return BGNN_OK;
}

extern "C" int bgnn_soundings_add(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0, double y0,
                                  double res, int64_t height, int64_t width, int64_t offered, void *state) {
  const char *fn = "bgnn_soundings_add";
  BGNN_TRY(require_cloud(fn, x, y, z, n, res, x0, y0, "resolution", state != nullptr));
  BGNN_TRY(require_grid(fn, height, width, "grid", 0, ""));
  BGNN_TRY(require_offered_total(fn, n, offered));
  BGNN_REQUIRE(aligned8(state), "%s: the state is not 8-byte aligned", fn);
  return launch_sounding_pass(fn, ctx, x, y, z, n, UniformAddress{x0, y0, res, height, width}, FileSink{static_cast<char *>(state)});
}

extern "C" int bgnn_soundings_finalize(bgnn_ctx *ctx, const void *state, int64_t height, int64_t width, int32_t min_count,
                                       float nodata_value, int32_t *count, float *mean, float *std, float *min, float *max,
                                       uint8_t *valid) {
  BGNN_REQUIRE(state && count && mean && std && min && max && valid, "bgnn_soundings_finalize: NULL argument");
  BGNN_TRY(require_grid("bgnn_soundings_finalize", height, width, "grid", 0, ""));
  BGNN_REQUIRE(min_count >= 1, "bgnn_soundings_finalize: a min_count of %d, at least 1 expected", (int)min_count);
  BGNN_REQUIRE(aligned8(state), "bgnn_soundings_finalize: the state is not 8-byte aligned");
  BGNN_REQUIRE(ctx, "bgnn_soundings_finalize: NULL context");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const int64_t n_cells = height * width;
  const dim3 g(capped_grid((n_cells + SG_THREADS - 1) / SG_THREADS, SG_FINALIZE_MAX_GRID)), b(SG_THREADS);
  hipLaunchKernelGGL(soundings_finalize, g, b, 0, ctx->stream, static_cast<const char *>(state), n_cells, min_count, nodata_value, count,
                     mean, std, min, max, valid);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

extern "C" int bgnn_soundings_extent(bgnn_ctx *ctx, const double *x, const double *y, int64_t n, void *extent) {
  BGNN_REQUIRE(n >= 0, "bgnn_soundings_extent: %lld soundings", (long long)n);
  BGNN_REQUIRE(extent && (n == 0 || (x && y)), "bgnn_soundings_extent: NULL argument");
  BGNN_REQUIRE(aligned8(extent), "bgnn_soundings_extent: the extent buffer is not 8-byte aligned");
  BGNN_REQUIRE(ctx, "bgnn_soundings_extent: NULL context");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  ExtentRecord *records = static_cast<ExtentRecord *>(extent);
  const int parts = capped_grid((n + SG_EXTENT_SHARE - 1) / SG_EXTENT_SHARE, BGNN_SOUNDINGS_EXTENT_MAX_GRID);
  hipLaunchKernelGGL(extent_partial, dim3(parts), dim3(SG_THREADS), 0, ctx->stream, x, y, n, records + 1);
  hipLaunchKernelGGL(extent_finish, dim3(1), dim3(SG_THREADS), 0, ctx->stream, records + 1, parts, records);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
