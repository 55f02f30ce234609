// The trainer part of the C ABI (include/bgnn_trainer.h): the per-node training targets of a batch gathered from its per-cell
// planes, and the bookkeeping of a step added into an epoch's accumulator block on the device.
//   training_targets_kernel  one thread per cell, 256 per workgroup: node ids ascend with the cell index, so the reads of the
//                            planes are coalesced and the local_std reads / row writes of a wave fall into a few lines.  About 21 B
//                            in and 13 B out per valid cell, 4 B per invalid one: HBM-bound
//   epoch_accumulate_kernel  one workgroup, every entry of the block owned by one thread
// Compiled with -ffp-contract=off: the accumulator's multiply and add round separately, as a host replay in Python floats does.
#include "bgnn_internal.h"
#include "../../include/bgnn_loss.h"
#include "../../include/bgnn_trainer.h"

namespace bgnn {

constexpr int TT_THREADS = 256;
constexpr int EA_THREADS = 256;
static_assert(BGNN_EPOCH_MAX_CLASSES == BGNN_LOSS_MAX_CLASSES, "the accumulator holds the loss pass's confusion matrix");
static_assert(BGNN_EPOCH_MAX_CLASSES * BGNN_EPOCH_MAX_CLASSES <= EA_THREADS, "one thread per confusion entry");
static_assert(BGNN_EPOCH_ACC_NODES == 6 * sizeof(double) && BGNN_EPOCH_ACC_CONFUSION == BGNN_EPOCH_ACC_STEPS + 8, "block layout");

struct TargetArgs {
  const int32_t *node_id;    // [cells]: >= 0 the cell's node
  const float *local_std;    // [rows]
  const int64_t *counts;     // [0] = nodes
  int64_t cells;
  const float *a, *b;
  const void *labels;
  const uint8_t *noise_mask;
  int64_t *y;
  float *target;
  uint8_t *mask;
};

// torch.clamp's order of operations on float32: a NaN passes through both
__device__ __forceinline__ float normalised_correction(float raw, float local_std) {
  const float s = local_std < BGNN_CORRECTION_NORM_FLOOR ? BGNN_CORRECTION_NORM_FLOOR : local_std;   // clamp(min=): NaN stays
  const float q = (float)((double)raw / (double)s);          // the correctly rounded float32 quotient (53 >= 2 * 24 + 2 bits)
  if (q != q) return q;
  return q < -BGNN_CORRECTION_NORM_CAP ? -BGNN_CORRECTION_NORM_CAP : (q > BGNN_CORRECTION_NORM_CAP ? BGNN_CORRECTION_NORM_CAP : q);
}

template <int MODE>
__global__ __launch_bounds__(TT_THREADS) void training_targets_kernel(const TargetArgs t) {
  const int64_t cell = (int64_t)blockIdx.x * TT_THREADS + threadIdx.x;
  if (cell >= t.cells) return;
  const int64_t r = t.node_id[cell];
  if (r < 0 || r >= t.counts[0]) return;
  if (MODE == BGNN_TARGETS_SYNTHETIC) {
    const float raw = t.a[cell] - t.b[cell];
    t.y[r] = static_cast<const int64_t *>(t.labels)[cell];
    t.target[r] = normalised_correction(raw, t.local_std[r]);
    t.mask[r] = t.noise_mask[cell] ? 1 : 0;
  } else {
    const int32_t label = static_cast<const int32_t *>(t.labels)[cell];
    t.y[r] = (int64_t)label;
    t.target[r] = normalised_correction(t.a[cell], t.local_std[r]);
    t.mask[r] = label == 2 ? 1 : 0;
  }
}

__global__ __launch_bounds__(EA_THREADS) void epoch_accumulate_kernel(const int64_t *graph_counts, const float *terms,
                                                                      const int64_t *counts, int C, char *acc) {
  const int64_t n = graph_counts[0];
  if (n <= 0) return;
  double *sums = reinterpret_cast<double *>(acc + BGNN_EPOCH_ACC_SUMS);
  int64_t *scal = reinterpret_cast<int64_t *>(acc + BGNN_EPOCH_ACC_NODES);      // nodes, correct, steps
  int64_t *conf = reinterpret_cast<int64_t *>(acc + BGNN_EPOCH_ACC_CONFUSION);
  const int t = threadIdx.x;
  if (t < C * C) conf[t] += counts[t];
  if (t < 6) {
    const double p = (double)terms[t] * (double)n;
    sums[t] += p;
  }
  if (t >= 64 && t < 67) {       // (a wave of its own: the three scalars, one lane each)
    int64_t add = n;
    if (t == 65) {
      add = 0;
      for (int c = 0; c < C; ++c) add += counts[c * C + c];
    } else if (t == 66) {
      add = 1;
    }
    scal[t - 64] += add;
  }
}

}  // namespace bgnn

using namespace bgnn;

extern "C" int bgnn_training_targets(bgnn_ctx *ctx, const bgnn_graph *graph, int32_t mode, const float *a, const float *b,
                                     const void *labels, const uint8_t *noise_mask, int64_t *y, float *target, uint8_t *mask) {
  BGNN_REQUIRE(ctx && graph && a && labels && y && target && mask, "bgnn_training_targets: NULL argument");
  BGNN_REQUIRE(mode == BGNN_TARGETS_SYNTHETIC || mode == BGNN_TARGETS_GROUND_TRUTH, "bgnn_training_targets: mode %d (0 or 1)", mode);
  BGNN_REQUIRE(mode != BGNN_TARGETS_SYNTHETIC || (b && noise_mask), "bgnn_training_targets: mode 0 needs the clean plane and the noise mask");
  BGNN_REQUIRE(graph->kind == 0 && graph->d_node_id && graph->d_local_std && graph->d_counts,
               "bgnn_training_targets: the graph was not built from tiles (bgnn_graph_build)");
  BGNN_REQUIRE(graph->ctx == ctx, "bgnn_training_targets: the graph belongs to another context");
  const int64_t cells = graph->total_cells;
  if (cells <= 0) return BGNN_OK;
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  TargetArgs t{};
  t.node_id = graph->d_node_id;
  t.local_std = graph->d_local_std;
  t.counts = graph->d_counts;
  t.cells = cells;
  t.a = a; t.b = b; t.labels = labels; t.noise_mask = noise_mask;
  t.y = y; t.target = target; t.mask = mask;
  const dim3 grid((unsigned)((cells + TT_THREADS - 1) / TT_THREADS));
  if (mode == BGNN_TARGETS_SYNTHETIC)
    hipLaunchKernelGGL(training_targets_kernel<BGNN_TARGETS_SYNTHETIC>, grid, dim3(TT_THREADS), 0, ctx->stream, t);
  else
    hipLaunchKernelGGL(training_targets_kernel<BGNN_TARGETS_GROUND_TRUTH>, grid, dim3(TT_THREADS), 0, ctx->stream, t);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

extern "C" int bgnn_epoch_accumulate(bgnn_ctx *ctx, const bgnn_graph *graph, const float *terms, const int64_t *counts,
                                     int32_t num_classes, void *acc) {
  BGNN_REQUIRE(ctx && graph && terms && counts && acc, "bgnn_epoch_accumulate: NULL argument");
  BGNN_REQUIRE(num_classes >= 2 && num_classes <= BGNN_EPOCH_MAX_CLASSES, "bgnn_epoch_accumulate: %d classes (2 .. %d)", num_classes,
               BGNN_EPOCH_MAX_CLASSES);
  BGNN_REQUIRE(((uintptr_t)acc & 7) == 0, "bgnn_epoch_accumulate: the accumulator block is not 8-byte aligned");
  BGNN_REQUIRE(graph->d_counts, "bgnn_epoch_accumulate: the graph has no device counters");
  BGNN_REQUIRE(graph->ctx == ctx, "bgnn_epoch_accumulate: the graph belongs to another context");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(epoch_accumulate_kernel, dim3(1), dim3(EA_THREADS), 0, ctx->stream, graph->d_counts, terms, counts,
                     (int)num_classes, static_cast<char *>(acc));
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

extern "C" int bgnn_epoch_reset(bgnn_ctx *ctx, void *acc) {
  BGNN_REQUIRE(ctx && acc, "bgnn_epoch_reset: NULL argument");
  BGNN_REQUIRE(((uintptr_t)acc & 7) == 0, "bgnn_epoch_reset: the accumulator block is not 8-byte aligned");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  BGNN_HIP_CHECK(hipMemsetAsync(acc, 0, BGNN_EPOCH_ACC_BYTES, ctx->stream));
  return BGNN_OK;
}
