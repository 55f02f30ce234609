/*
 * bgnn_locale.h -- C ABI of libbgnn_hip.so, the locale rule for depth hypotheses (ABI 7, additive; no entry point of bgnn.h or of
 * the other side headers changes): a guide plane for BGNN_HYP_RULE_GUIDE (bgnn_hypotheses.h) from the neighbouring cells that
 * have exactly one hypothesis.  CUBE's third disambiguation rule after "number of samples" (BGNN_HYP_RULE_COUNT) and "predicted
 * surface" (BGNN_HYP_RULE_GUIDE with a guide of the caller's): where a fish school outnumbers the seabed in a cell, the cells
 * around it that hold the seabed alone say which of the two to take.
 *
 * The conventions of bgnn_hypotheses.h hold (DEVICE pointers owned by the caller, return codes, bgnn_last_error(), the context's
 * stream, asynchronous): the entry point does not synchronise with the host, allocate, copy to the host or take a workspace;
 * refusals happen before any launch, the context checked last; no launch geometry depends on a device value.  The Python mirror
 * binds it in bathymetric_gnn_amd/runtime.py (_LOCALE_SIGNATURES); data/locale_guide.py drives it.
 *
 * The inputs are [height][width] planes, row-major: n_hyp and chosen (int32) of a bgnn_hypotheses_build over the grid, under
 * either rule, and center2 (int64, 8-byte aligned) of the bgnn_soundings_robust_finalize the hypotheses were built from: m2,
 * twice the cell's median in units of 2^-17 m, |m2| < 2^32.
 *
 * Per cell (r, c), all in integers (csrc/locale_window.h):
 *     a cell (r', c') is a witness iff n_hyp == 1 && chosen == 0 there; its value is its center2
 *     the window is |r' - r| <= radius, |c' - c| <= radius, clipped to the grid, without (r, c) itself
 *     support = k, the number of witnesses in the window, written for every cell
 *     w[0 .. k) the witness values of the window in ascending order
 *     k >= min_support:  med2 = w[(k-1)/2] + w[k/2]  (exact, |med2| < 2^33),  guide = (float)((double)med2 * 2^-18), one rounding
 *     k <  min_support:  guide = the quiet NaN with bits 0x7FC00000
 * bgnn_hypotheses_build under BGNN_HYP_RULE_GUIDE takes the plane as it is: a NaN guide, and one that rounds to |g| >= 32768, fall
 * back to the count key.
 *
 * Both outputs are a function of the three planes alone: equal bits on every run, and so for every order of the cloud.
 */
#ifndef BGNN_LOCALE_H
#define BGNN_LOCALE_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_LOCALE_MAX_RADIUS 8

/* bgnn_locale_guide: guide (float32) and support (int32), [height][width] each, from n_hyp, chosen and center2, which it only reads.
 *   BGNN_ERR_INVALID: a NULL argument, height or width < 1, height * width > 2^31 - 1, radius outside 1 .. BGNN_LOCALE_MAX_RADIUS,
 *   min_support outside 1 .. (2 * radius + 1)^2 - 1, a center2 that is not 8-byte aligned. */
int bgnn_locale_guide(bgnn_ctx *ctx, const int32_t *n_hyp, const int32_t *chosen, const int64_t *center2, int64_t height,
                      int64_t width, int32_t radius, int32_t min_support, float *guide, int32_t *support);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_LOCALE_H */
