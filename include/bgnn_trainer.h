/*
 * bgnn_trainer.h -- C ABI of libbgnn_hip.so, trainer part: the two pieces of the reference's training step that sit around the
 * forward, the loss and the optimizer (training/trainer.py:400-424 / :258-284: the per-node labels of a sample; :764-767: the
 * step's bookkeeping), as device code (ABI 7, additive; no entry point of bgnn.h or of the other side headers changes).
 *
 * The conventions of bgnn.h hold (DEVICE / HOST pointers, return codes, bgnn_last_error(), the context's stream, asynchronous).
 * The Python mirror binds these in bathymetric_gnn_amd/runtime.py (_TRAINER_SIGNATURES); training/trainer.py (TileStore,
 * EpochMetrics) drives them.
 */
#ifndef BGNN_TRAINER_H
#define BGNN_TRAINER_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_TARGETS_SYNTHETIC 0    /* a = noisy depth, b = clean depth, labels int64, noise_mask uint8 */
#define BGNN_TARGETS_GROUND_TRUTH 1 /* a = the difference plane, b = NULL, labels int32 (-1 = nodata), noise_mask = NULL */
#define BGNN_CORRECTION_NORM_FLOOR 0.01f /* config/constants.py CORRECTION_NORM_FLOOR, as float32 */
#define BGNN_CORRECTION_NORM_CAP 50.0f   /* config/constants.py CORRECTION_NORM_CAP */

/* bgnn_training_targets: the labels a dataset of the reference attaches to a graph, per node, for a grid graph (bgnn_graph_build)
 *   and the planes of the batch it was built from: flat DEVICE arrays with one entry per CELL, in the layout of the bgnn_tiles the
 *   graph was built from.  One launch, one thread per cell; a cell that is node r writes row r of
 *     y      int64    labels[cell]
 *     target float32  clamp(raw / max(local_std[r], CORRECTION_NORM_FLOOR), -CORRECTION_NORM_CAP, +CORRECTION_NORM_CAP)
 *                     raw = a[cell] - b[cell] (float32 subtraction) in mode 0, a[cell] in mode 1; local_std is the graph's own
 *                     per-node table (no export); the quotient is the correctly rounded float32 one (divided in float64, rounded
 *                     once); a NaN local_std or quotient stays NaN, as torch.clamp leaves it
 *     mask   uint8    noise_mask[cell] != 0 in mode 0, labels[cell] == 2 in mode 1
 *   The two constants are config/constants.py's (below).  Every row below the graph's node count has exactly one owning cell: no
 *   atomics, and rows at or beyond the node count are not written.  A batch without cells launches nothing.
 *   BGNN_ERR_INVALID: NULL arguments, a mode other than the two, mode 0 without b or noise_mask, a graph that was not built from
 *   tiles (bgnn_graph_from_edges). */
int bgnn_training_targets(bgnn_ctx *ctx, const bgnn_graph *graph, int32_t mode, const float *a, const float *b, const void *labels,
                          const uint8_t *noise_mask, int64_t *y, float *target, uint8_t *mask);

/* The accumulator block of an epoch (DEVICE, caller-owned, 8-byte aligned, BGNN_EPOCH_ACC_BYTES):
 *   double  sums[6]        running sums of (double)term * (double)n, in bgnn_loss.h's order of terms
 *   int64   nodes          sum of n
 *   int64   correct        sum of the trace of the step's confusion matrix
 *   int64   steps          steps with n > 0
 *   int64   confusion[BGNN_EPOCH_MAX_CLASSES * BGNN_EPOCH_MAX_CLASSES]   the first C * C entries used, row-major at stride C */
#define BGNN_EPOCH_MAX_CLASSES 16
#define BGNN_EPOCH_ACC_SUMS 0    /* byte offsets */
#define BGNN_EPOCH_ACC_NODES 48
#define BGNN_EPOCH_ACC_CORRECT 56
#define BGNN_EPOCH_ACC_STEPS 64
#define BGNN_EPOCH_ACC_CONFUSION 72
#define BGNN_EPOCH_ACC_BYTES (72 + 8 * BGNN_EPOCH_MAX_CLASSES * BGNN_EPOCH_MAX_CLASSES)

/* bgnn_epoch_accumulate: the bookkeeping of one step, without a host round trip.  terms DEVICE float32 [6] and counts DEVICE int64
 *   [C * C + BGNN_LOSS_N_COUNTS] as bgnn_loss_forward left them; n is the graph's node count, read from its device counters.  One
 *   workgroup, each entry of the block owned by one thread: one float64 multiply and one add per term (unfused), integer adds
 *   for the rest -- equal inputs give equal bits, and the block equals a host replay in Python floats.  A label outside [0, C)
 *   never equals a prediction, so the trace is the reference's (predicted == y).sum().  n == 0: nothing is added, no step is
 *   counted, terms and counts are not read.
 * bgnn_epoch_reset: zeroes the block.
 *   BGNN_ERR_INVALID: NULL arguments, num_classes outside 2 .. BGNN_EPOCH_MAX_CLASSES, a block that is not 8-byte aligned. */
int bgnn_epoch_accumulate(bgnn_ctx *ctx, const bgnn_graph *graph, const float *terms, const int64_t *counts, int32_t num_classes,
                          void *acc);
int bgnn_epoch_reset(bgnn_ctx *ctx, void *acc);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_TRAINER_H */
