// The streaming pass over a point cloud of soundings (x, y, z), 20 B per sounding: one loop for every gridder.  A pass is an
// address rule, which says what kind a sounding is (sounding_file.h) and which cell or record it belongs to, and a sink, which
// says what happens to it there.
//
//   address rules   UniformAddress  the cell of sounding_cell.h on a height x width grid, upper-left origin; four kinds.
//                   VRBaseAddress   the base cell of sounding_vr_cell.h without a table: no entry is loaded, every base cell
//                                   counts as refined.
//                   VRAddress       the record of sounding_vr_cell.h under a layout table: one 16-byte load of the base cell's
//                                   entry, only for a sounding that lies on the base grid; five kinds, the fifth (unrefined)
//                                   counted beside the header.
//   sinks           FileSink        file_sounding into a SoundingCell state, six integer atomics per run of neighbouring lanes.
//                   StageSink       (where, q) into the sounding's own slot of a robust stage, where = -1 if not accepted: one
//                                   8-byte store, no atomics.
//                   FlagSink        |2q - center2| against limit: one byte per sounding.
//                   DensitySink     one integer atomic per run of neighbouring lanes in one base cell.
//
// FileSink and StageSink keep counters: the kinds are tallied per thread, reduced per workgroup (block_reduce) and added with
// one atomic per workgroup and counter into the header in front of the state or stage.  FlagSink and DensitySink keep none, and
// their instantiations have neither the tallies, nor the LDS, nor the reductions.
#pragma once
#include "bgnn_internal.h"
#include "plane_util.h"
#include "sounding_cell.h"
#include "sounding_file.h"
#include "sounding_vr_cell.h"
#include "../../include/bgnn_soundings.h"
#include "../../include/bgnn_soundings_robust.h"

namespace bgnn {

constexpr int PASS_ITEMS = 4;                         // soundings per thread and step, a workgroup's width apart: coalesced loads
constexpr int PASS_TILE = BLOCK_THREADS * PASS_ITEMS;

// ---- address rules: KINDS counters, and classify() -> the SoundingKind, *where the cell or record (negative: none) ------------------

struct UniformAddress {
  static constexpr int KINDS = 4;                     // no unrefined kind, and no counter for one
  double x0, y0, res;
  int64_t height, width;
  __device__ __forceinline__ int classify(double x, double y, float z, int64_t *where) const {
    *where = sounding_cell(x, y, x0, y0, res, height, width);
    return sounding_kind(x, y, z, *where >= 0, true);
  }
};

struct VRGeometry {
  double x0, y0, B;
  int64_t BH, BW, total;
};

struct VRBaseAddress {
  static constexpr int KINDS = 4;
  VRGeometry g;
  __device__ __forceinline__ int classify(double x, double y, float z, int64_t *where) const {
    double fu, fv;
    *where = vr_base_cell(x, y, g.x0, g.y0, g.B, g.BH, g.BW, &fu, &fv);
    return sounding_kind(x, y, z, *where >= 0, true);
  }
};

struct VRAddress {
  static constexpr int KINDS = SOUNDING_KINDS;
  VRGeometry g;
  const VRLayoutEntry *table;
  int64_t *unrefined;                                 // the fifth counter; read only by a pass whose sink keeps counters
  __device__ __forceinline__ int classify(double x, double y, float z, int64_t *where) const {
    double fu = 0.0, fv = 0.0;
    const int64_t b = vr_base_cell(x, y, g.x0, g.y0, g.B, g.BH, g.BW, &fu, &fv);
    bool refined = false;
    *where = -1;
    if (b >= 0) {                                     // on the base grid: b is inside the table
      const VRLayoutEntry e = table[b];               // (16 bytes, one load)
      refined = vr_entry_refined(e, g.total);
      if (refined) *where = vr_record(e, fu, fv);
    }
    return sounding_kind(x, y, z, b >= 0, refined);
  }
};

// ---- sinks: COUNTERS, header() where it has them, and put() for every item of every lane (in: the item lies below n) -----------------

struct FileSink {
  static constexpr bool COUNTERS = true;
  static constexpr bool PRELOAD = true;
  char *state;
  __device__ __forceinline__ char *header() const { return state; }
  __device__ __forceinline__ void put(bool, int64_t, int kind, int64_t where, float z) const {
    file_sounding(reinterpret_cast<SoundingCell *>(state + BGNN_SOUNDINGS_HEADER_BYTES), kind == SOUNDING_ACCEPTED, where, z);
  }
};

struct StageSink {
  static constexpr bool COUNTERS = true;
  static constexpr bool PRELOAD = true;
  char *stage;
  int64_t offered;                                    // item i goes to slot offered + i
  __device__ __forceinline__ char *header() const { return stage; }
  __device__ __forceinline__ void put(bool in, int64_t i, int kind, int64_t where, float z) const {
    int2 *slots = reinterpret_cast<int2 *>(stage + BGNN_ROBUST_STAGE_HEADER_BYTES) + offered;
    const bool ok = kind == SOUNDING_ACCEPTED;        // (the entry points cap cells and records: where fits an int; |q| < 2^31)
    if (in) slots[i] = make_int2(ok ? (int)where : -1, ok ? (int)sounding_q(z) : 0);
  }
};

struct FlagSink {
  static constexpr bool COUNTERS = false;
  static constexpr bool PRELOAD = false;
  const int64_t *center2, *limit;
  uint8_t *flags;
  __device__ __forceinline__ void put(bool in, int64_t i, int kind, int64_t where, float z) const {
    if (!in) return;
    uint8_t f = BGNN_ROBUST_FLAG_NOT_ACCEPTED;
    if (kind == SOUNDING_ACCEPTED) {
      const int64_t d = 2 * (int64_t)sounding_q(z) - center2[where];
      f = (d < 0 ? -d : d) > limit[where] ? BGNN_ROBUST_FLAG_REJECTED : BGNN_ROBUST_FLAG_KEPT;      // (limit -1: an empty cell)
    }
    flags[i] = f;
  }
};

struct DensitySink {
  static constexpr bool COUNTERS = false;
  static constexpr bool PRELOAD = true;
  uint32_t *counts;
  __device__ __forceinline__ void put(bool, int64_t, int kind, int64_t where, float) const {
    // a run of neighbouring lanes in one base cell (a swath) is counted by its first lane
    const bool ok = kind == SOUNDING_ACCEPTED;
    const int lane = threadIdx.x & 63;
    const int64_t mine = ok ? where : (int64_t)-1 - lane;                              // (a rejected lane merges with nobody)
    const int64_t prev = __shfl_up(mine, 1);
    const bool start = lane == 0 || prev != mine;
    const unsigned long long starts = __ballot(start);
    if (ok && start) {
      const unsigned long long after = lane == 63 ? 0ull : starts >> (lane + 1);
      atomicAdd(counts + where, (uint32_t)(after ? __ffsll((long long)after) : 64 - lane));      // the lanes to the end of the run
    }
  }
};

// ---- the pass -----------------------------------------------------------------------------------------------------------------------
//
// Grid-stride over tiles of PASS_TILE soundings.  Settled here, once, for every pass:
//   - the four soundings of a thread are loaded before any of them is handled (zeros past the tail), unless the sink says
//     PRELOAD = false: the flag passes load each sounding where it is classified, the one compile-time switch of the load shape;
//   - FileSink and DensitySink shuffle across the wave, so every lane of every wave reaches put() on every item, the lanes past n
//     included: the loop never skips an item.  An item past n has kind -1, which is no kind: it enters no tally and no sink
//     accepts it; the sinks that store per sounding look at `in` and store nothing there;
//     (for FileSink this is a convention, not something a test can hold: a shuffle from a lane that has left is not defined, and
//     on gfx950 it happens to read as zero, which the sums and maxima absorb; DensitySink miscounts at once);
//   - the tallies and their LDS exist only where the sink keeps counters, and only Address::KINDS of them: a uniform pass has no
//     fifth tally and no pointer for one.
template <class Address, class Sink>
__global__ __launch_bounds__(BLOCK_THREADS) void sounding_pass(const double *__restrict__ xs, const double *__restrict__ ys,
                                                               const float *__restrict__ zs, int64_t n, Address address, Sink sink) {
  const int t = threadIdx.x;
  uint32_t tally[Address::KINDS] = {};                // (a workgroup sees fewer than 2^31 soundings)
  for (int64_t base = (int64_t)blockIdx.x * PASS_TILE; base < n; base += (int64_t)gridDim.x * PASS_TILE) {
    double x[PASS_ITEMS], y[PASS_ITEMS];
    float z[PASS_ITEMS];
    auto load = [&](int k) {
      const int64_t i = base + k * BLOCK_THREADS + t;
      const bool in = i < n;
      x[k] = in ? xs[i] : 0.0;
      y[k] = in ? ys[i] : 0.0;
      z[k] = in ? zs[i] : 0.0f;
    };
    if constexpr (Sink::PRELOAD) {
#pragma unroll
      for (int k = 0; k < PASS_ITEMS; ++k) load(k);
    }
    int64_t where[PASS_ITEMS];
    int kind[PASS_ITEMS];
#pragma unroll
    for (int k = 0; k < PASS_ITEMS; ++k) {            // all four before any goes to the sink: the table loads of a VR pass are not
      if (!Sink::PRELOAD) load(k);
      where[k] = -1;                                  // held up behind the sink's stores, and x and y are dead before the sink runs
      kind[k] = base + k * BLOCK_THREADS + t < n ? address.classify(x[k], y[k], z[k], &where[k]) : -1;
    }
#pragma unroll
    for (int k = 0; k < PASS_ITEMS; ++k) {
      const int64_t i = base + k * BLOCK_THREADS + t;
      if constexpr (Sink::COUNTERS) {
#pragma unroll
        for (int j = 0; j < Address::KINDS; ++j) tally[j] += kind[k] == j;
      }
      sink.put(i < n, i, kind[k], where[k], z[k]);
    }
  }
  if constexpr (Sink::COUNTERS) {
    __shared__ uint32_t scratch[BLOCK_THREADS];
    unsigned long long *counters = reinterpret_cast<unsigned long long *>(sink.header());
#pragma unroll
    for (int j = 0; j < Address::KINDS; ++j) {
      const uint32_t total = block_reduce(tally[j], scratch, SumOp());
      unsigned long long *counter = counters + j;
      if constexpr (Address::KINDS > SOUNDING_UNREFINED)
        if (j == SOUNDING_UNREFINED) counter = reinterpret_cast<unsigned long long *>(address.unrefined);
      if (t == 0 && total) atomicAdd(counter, (unsigned long long)total);
    }
  }
}

// The launch of a pass whose other arguments are in order: the context is checked last, an empty cloud launches nothing.
template <class Address, class Sink>
int launch_sounding_pass(const char *fn, bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n,
                         const Address &address, const Sink &sink) {
  BGNN_REQUIRE(ctx, "%s: NULL context", fn);
  if (n == 0) return BGNN_OK;
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const dim3 g(capped_grid((n + PASS_TILE - 1) / PASS_TILE, PLANE_MAX_GRID)), b(BLOCK_THREADS);
  hipLaunchKernelGGL((sounding_pass<Address, Sink>), g, b, 0, ctx->stream, x, y, z, n, address, sink);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

}  // namespace bgnn
