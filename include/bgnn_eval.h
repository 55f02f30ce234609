/*
 * bgnn_eval.h -- C ABI of libbgnn_hip.so, the two steps of the reference's workflow that surround training and inference, as
 * device code (ABI 7, additive; no entry point of bgnn.h or of the other side headers changes):
 *   ground truth  scripts/prepare_ground_truth.py, compute_ground_truth lines 159-185 and 235-255: a clean / noisy survey pair to
 *                 the label, difference and uncertainty planes, around an exact median of the difference over every valid cell
 *   evaluation    scripts/evaluate_model.py, compute_metrics: everything that function derives its dictionary from, counted over
 *                 a classified survey and its labels
 *
 * The conventions of bgnn.h hold (DEVICE / HOST pointers, return codes, bgnn_last_error(), the context's stream, asynchronous):
 * no entry point synchronises with the host, allocates, or copies to the host.  The Python mirror binds these in
 * bathymetric_gnn_amd/runtime.py (_EVAL_SIGNATURES); data/ground_truth.py and training/evaluation.py drive them.
 *
 * Determinism.  Every count is an integer sum (LDS and global integer atomics), every float64 sum is formed per thread in a fixed
 * order, reduced per workgroup in a fixed tree, stored as a per-workgroup partial and added in workgroup order (runs of 32
 * workgroups, then the runs) by one finishing workgroup; the grid is a function of `cells` alone.  Equal inputs give equal bits.
 * There are no float atomics.
 */
#ifndef BGNN_EVAL_H
#define BGNN_EVAL_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The statistics block of bgnn_ground_truth_build (DEVICE, caller-owned, 8-byte aligned, BGNN_GT_STATS_BYTES):
 *   int64   valid          cells where both depths are finite and != nodata
 *   int64   noise          cells labelled 2
 *   int64   seafloor       cells labelled 0
 *   double  noise_abs_sum  sum of (double)|difference| over the noise cells
 *   double  seafloor_sum   sum of (double)difference over the seafloor cells
 *   float   offset         the median that was removed (NaN without a valid cell)
 *   float   noise_abs_max  max of |difference| over the noise cells (0 without one) */
#define BGNN_GT_STATS_VALID 0     /* byte offsets */
#define BGNN_GT_STATS_NOISE 8
#define BGNN_GT_STATS_SEAFLOOR 16
#define BGNN_GT_STATS_NOISE_ABS_SUM 24
#define BGNN_GT_STATS_SEAFLOOR_SUM 32
#define BGNN_GT_STATS_OFFSET 40
#define BGNN_GT_STATS_NOISE_ABS_MAX 44
#define BGNN_GT_STATS_BYTES 48

/* bgnn_ground_truth_build: clean, noisy, noisy_unc (or NULL): flat DEVICE float32 planes of `cells` entries, already cut to one
 *   shape.  Per cell, in float32:
 *     raw        = noisy - clean
 *     valid      = both depths finite and != (float)nodata
 *     offset     = the median of raw over the valid cells as numpy forms it on a float32 array: the element of rank (n - 1) / 2 for
 *                  an odd count n; for an even one (a + b) rounded to float32, then halved, a and b of ranks n / 2 - 1 and n / 2;
 *                  NaN for n == 0.  -0.0 sorts below +0.0
 *     difference = raw - offset, NaN on invalid cells
 *     labels     = 2 where |difference| > (float)noise_threshold on valid cells, 0 on the other valid cells, -1 on invalid ones
 *                  (the threshold rounded to float32 first, as numpy compares a float32 array with a Python float: float32(0.15)
 *                  > 0.15, so |difference| == float32(0.15) is not noise)
 *     unc_out    = noisy_unc, NaN on invalid cells (written only when both pointers are given)
 *   and the statistics block above.  `difference` doubles as the selection's scratch: it must not alias an input.
 *   The median is an exact radix selection over the order-preserving uint32 image of raw: three histogram passes of 11 / 11 / 10
 *   bits, a one-workgroup kernel narrowing the prefix of both ranks after each; no sort.  ws: DEVICE scratch of at least
 *   bgnn_ground_truth_workspace_bytes(cells) bytes, 8-byte aligned (histograms, selection state, per-workgroup partials).
 *   cells == 0 launches nothing and writes nothing, `stats` included.
 *   BGNN_ERR_INVALID: NULL ctx / clean / noisy / ws / labels / difference / stats, unc_out without noisy_unc, cells < 0, a
 *   workspace that is too small or misaligned, a stats block that is not 8-byte aligned.
 * bgnn_ground_truth_workspace_bytes: 0 for cells < 0. */
size_t bgnn_ground_truth_workspace_bytes(int64_t cells);
int bgnn_ground_truth_build(bgnn_ctx *ctx, const float *clean, const float *noisy, const float *noisy_unc, int64_t cells,
                            double nodata, double noise_threshold, void *ws, size_t ws_bytes, int32_t *labels, float *difference,
                            float *unc_out, void *stats);

/* The accumulator block of an evaluation (DEVICE, caller-owned, 8-byte aligned, BGNN_EVAL_ACC_BYTES).  A cell counts when
 * label >= 0, pred >= 0 and pred is finite; its prediction is truncated toward zero (predictions at or above 2^31 are outside the
 * contract: numpy's cast to int32 is undefined there; here such a cell falls into class ">= 3" and is correct only if the label
 * equals the truncated value).
 *   int64   total
 *   int64   correct                 label == truncated prediction (also above class 2)
 *   int64   confusion[4][4]         [min(label, 3)][min(prediction, 3)]: classes 0, 1, 2 and ">= 3"
 *   int64   covered[5]              confidence >= (float)t for t = 0.5, 0.6, 0.7, 0.8, 0.9 (each threshold rounded to float32:
 *                                   float32(0.7) < 0.7, so a confidence of exactly float32(0.7) is covered)
 *   int64   covered_correct[5]      the same, on correct cells
 *   double  conf_sum                sum of (double)c - 0.5 over counted cells
 *   double  conf_sq                 sum of ((double)c - 0.5)^2 over counted cells
 *   double  conf_correct_sum        sum of (double)c - 0.5 over correct cells
 *   double  conf_incorrect_sum      sum of (double)c - 0.5 over counted cells that are not correct
 *   int64   conf_cells              counted cells of the calls that gave a confidence plane (== total when every call did)
 * A NaN confidence on a counted cell poisons the sums it enters and compares false, as in numpy. */
#define BGNN_EVAL_THRESHOLDS 5
#define BGNN_EVAL_ACC_TOTAL 0     /* byte offsets */
#define BGNN_EVAL_ACC_CORRECT 8
#define BGNN_EVAL_ACC_CONFUSION 16
#define BGNN_EVAL_ACC_COVERED 144
#define BGNN_EVAL_ACC_COVERED_CORRECT 184
#define BGNN_EVAL_ACC_CONF_SUM 224
#define BGNN_EVAL_ACC_CONF_SQ 232
#define BGNN_EVAL_ACC_CONF_CORRECT_SUM 240
#define BGNN_EVAL_ACC_CONF_INCORRECT_SUM 248
#define BGNN_EVAL_ACC_CONF_CELLS 256
#define BGNN_EVAL_ACC_BYTES 264

/* bgnn_eval_accumulate: adds the cells of labels (DEVICE int32), pred (DEVICE float32) and confidence (DEVICE float32 or NULL:
 *   the confidence entries of the block are left alone), `cells` entries each, into the block: row bands of one survey or several
 *   surveys accumulate across calls.  ws: DEVICE scratch of at least bgnn_eval_workspace_bytes(cells) bytes, 8-byte aligned.
 *   cells == 0 launches nothing.
 * bgnn_eval_reset: zeroes the block.
 *   BGNN_ERR_INVALID: NULL ctx / labels / pred / ws / acc, cells < 0, a workspace that is too small or misaligned, a block that is
 *   not 8-byte aligned. */
size_t bgnn_eval_workspace_bytes(int64_t cells);
int bgnn_eval_reset(bgnn_ctx *ctx, void *acc);
int bgnn_eval_accumulate(bgnn_ctx *ctx, const int32_t *labels, const float *pred, const float *confidence, int64_t cells, void *ws,
                         size_t ws_bytes, void *acc);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_EVAL_H */
