/*
 * bgnn_curve.h -- C ABI of libbgnn_hip.so, operating curves of a classified survey against its ground truth (ABI 7, additive; no
 * entry point of bgnn.h or of the other side headers changes): one pass over the planes counts, for every threshold of a caller's
 * table at once, what the reference's workflow asks after each training run (docs/LESSONS_LEARNED.md "Inference Threshold
 * Selection", "Visual Validation Checklist" step 5; docs/HOW_IT_WORKS.md "Operational Confidence Thresholds";
 * docs/TRAINING_PLAN.md "Metrics to Track"): which cells auto-correction (conf > t), coverage (conf >= t) and review (conf < t)
 * select, what they are and what they are predicted as, and what the predicted corrections do to the residual error.
 *
 * The conventions of bgnn_eval.h hold (DEVICE pointers owned by the caller, return codes, bgnn_last_error(), the context's stream,
 * asynchronous): no entry point synchronises with the host, allocates, or copies to the host; refusals happen before any launch.
 * The Python mirror binds these in bathymetric_gnn_amd/runtime.py (_CURVE_SIGNATURES); training/operating_curve.py drives them.
 *
 * Determinism.  Every entry of the block is an integer sum (LDS and global integer atomics); the grid is a function of `cells`
 * alone.  Equal inputs give equal bits however the workgroups interleave.  There are no float atomics and no float sums.
 */
#ifndef BGNN_CURVE_H
#define BGNN_CURVE_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_CURVE_MAX_THRESHOLDS 128
#define BGNN_CURVE_WG_CELLS 1024     /* cells of one workgroup's share: the grid is min(ceil(cells / 1024), BGNN_CURVE_MAX_GRID) */
#define BGNN_CURVE_MAX_GRID 1024     /* workgroups; beyond that each takes every 1024th share */
#define BGNN_CURVE_RES_CAP 32768     /* residuals at or above this many metres enter no sum */
#define BGNN_CURVE_RES_SCALE 65536   /* fixed point: q(v) = llrint((double)v * 65536.0), half to even */

/* Which cells count: the rule of bgnn_eval_accumulate -- label >= 0, pred finite and >= 0; pred is truncated toward zero; the
 * true class is min(label, 3), the predicted class min(trunc(pred), 3): classes 0, 1, 2 and ">= 3".
 *
 * The confidence code of a cell, against the table t_0 < t_1 < ... < t_(T-1):
 *     code(c) = 2 * #{k : t_k < c} + [c == t_k for some k]          0 .. 2T
 *     code(NaN) = 2T + 1
 * -inf, negative values, values above 1 and +inf fall into the end codes 0, 1, 2T - 1, 2T like any other number.  The reference's
 * three comparisons are exact functions of the code:
 *     c >  t_k  <=>  2k + 2 <= code <= 2T        (auto-correct)
 *     c >= t_k  <=>  2k + 1 <= code <= 2T        (evaluate_model.py's coverage)
 *     c <  t_k  <=>  code <= 2k                  (review)
 * and a NaN confidence satisfies none of them, as in numpy.
 *
 * The block (DEVICE, caller-owned, 8-byte aligned, BGNN_CURVE_BLOCK_BYTES(T) bytes), every entry int64, B = 2T + 2 codes:
 *   counts[B][4][4]    counted cells per (code, true class, predicted class)
 *   res_cells[B][4]    per (code, true class): predicted-noise cells (predicted class 2) whose difference and correction are
 *                      finite and where |difference| and |difference - correction| are both < 32768
 *   abs_before[B][4]   the sum of q(|difference|) over those cells
 *   abs_after[B][4]    the sum of q(|difference - correction|) over those cells
 *   base_cells[4]      per true class: counted cells, of any predicted class, with finite |difference| < 32768
 *   base_abs[4]        the sum of q(|difference|) over those cells
 *   res_skipped        counted cells whose residual entered no sum (difference not finite, or |difference| >= 32768)
 * difference - correction is formed in float32, as numpy forms it on float32 planes.  q(v) = llrint((double)v * 65536.0): the
 * product is exact in float64 and the rounding is half to even (np.rint); q < 2^31.  A block holds at most 2^32 counted cells in
 * total over all the calls accumulated into it: within that bound no sum reaches 2^63.  (A predicted-noise cell whose difference
 * qualifies and whose correction does not is in base_* only: the derived figures treat it as not corrected.) */
#define BGNN_CURVE_CODES(T) (2 * (T) + 2)
#define BGNN_CURVE_COUNTS(T) 0                                   /* byte offsets */
#define BGNN_CURVE_RES_CELLS(T) (128 * BGNN_CURVE_CODES(T))
#define BGNN_CURVE_ABS_BEFORE(T) (160 * BGNN_CURVE_CODES(T))
#define BGNN_CURVE_ABS_AFTER(T) (192 * BGNN_CURVE_CODES(T))
#define BGNN_CURVE_BASE_CELLS(T) (224 * BGNN_CURVE_CODES(T))
#define BGNN_CURVE_BASE_ABS(T) (224 * BGNN_CURVE_CODES(T) + 32)
#define BGNN_CURVE_RES_SKIPPED(T) (224 * BGNN_CURVE_CODES(T) + 64)
#define BGNN_CURVE_BLOCK_BYTES(T) (224 * BGNN_CURVE_CODES(T) + 72)

/* bgnn_curve_block_bytes: BGNN_CURVE_BLOCK_BYTES(n_thresholds); 0 for n_thresholds outside 1 .. BGNN_CURVE_MAX_THRESHOLDS.
 * bgnn_curve_reset: zeroes the block of a table of n_thresholds entries.
 * bgnn_curve_accumulate: adds the cells of labels (DEVICE int32), pred, confidence (DEVICE float32) and, when given, difference
 *   and correction (DEVICE float32), `cells` entries each, into the block: row bands of one survey or several surveys accumulate
 *   across calls, all with the same table.  thresholds: DEVICE float32, n_thresholds entries, every one finite, strictly
 *   increasing (the caller's contract: it is not checked here, and no bit pattern of the table or of the planes takes an index out
 *   of range).  difference == NULL and correction == NULL together: the residual entries (res_cells .. res_skipped) are left
 *   alone.  cells == 0 launches nothing.
 *   BGNN_ERR_INVALID: NULL ctx / thresholds / labels / pred / confidence / block, n_thresholds outside 1 .. 128, only one of
 *   difference and correction, cells < 0 or above 2^32, a block that is not 8-byte aligned. */
size_t bgnn_curve_block_bytes(int n_thresholds);
int bgnn_curve_reset(bgnn_ctx *ctx, void *block, int n_thresholds);
int bgnn_curve_accumulate(bgnn_ctx *ctx, const float *thresholds, int n_thresholds, const int32_t *labels, const float *pred,
                          const float *confidence, const float *difference, const float *correction, int64_t cells, void *block);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_CURVE_H */
