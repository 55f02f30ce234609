/*
 * bgnn_loss.h -- C ABI of libbgnn_hip.so, the multi-task training loss (ABI 7, additive).
 *
 * The conventions of bgnn.h hold (DEVICE / HOST pointers, return codes, bgnn_last_error(), the context's stream).  This header
 * adds the loss behind training/losses.py's BathymetricGNNLoss (reference training/losses.py, the five component losses and
 * their weighted sum) and its gradient with respect to the three differentiable model outputs.  The Python mirror binds the
 * entry points in bathymetric_gnn_amd/runtime.py (_LOSS_SIGNATURES).
 *
 * Per node everything is float64: the float32 inputs are widened on load, exp / log / log1p are the double ones.  With N rows,
 * C classes, y the labels, q the predicted classes, w the class weights (ones when has_class_weights == 0), e = label_smoothing:
 *   classification        lp = log-softmax(logits); K = {i : y_i != -100} (BGNN_LOSS_IGNORE_INDEX); W = sum_K w[y_i]
 *                         ((1 - e) * -sum_K w[y_i] lp[i, y_i] + (e / C) * -sum_K sum_c w[c] lp[i, c]) / W
 *                         d/dlogits[i, c] = ((1 - e) w[y_i] (p[i, c] - [c == y_i]) + (e / C) (p[i, c] sum_c' w[c'] - w[c])) / W for
 *                         i in K, 0 for an ignored row.  A label outside [0, C) other than -100 makes the term (and the total)
 *                         NaN, and the gradient of that row NaN: there is no device assert.
 *   correction            Huber over S = {i : noise_mask_i != 0} (every row when noise_mask is NULL), M = #S, d = correction - target:
 *                         sum_S (|d| < delta ? d d / 2 : delta (|d| - delta / 2)) / M;  gradient d / M or delta sign(d) / M on S,
 *                         0 elsewhere; 0 with a zero gradient when M == 0 or when correction or correction_targets is NULL.
 *   confidence            t = (q_i == y_i); -sum (t max(log x, -100) + (1 - t) max(log1p(-x), -100)) / N;
 *                         gradient (x - t) / max((1 - x) x, (double)1e-12f) / N
 *   feature_preservation  penalty_weight * #{y == feature_class and q == feature_noise_class} / N            (no gradient)
 *   shoal_safety          FP = {y == seafloor_class and q == shoal_noise_class}; 0 when FP is empty or correction_targets is NULL,
 *                         else (shoal_penalty #{FP, target < 0} + deep_penalty #{FP, not target < 0}) / #FP   (no gradient)
 *   total                 sum_k term_weights[k] * term_k, from the unrounded float64 terms
 * Every float sum is float64 in an order that is a function of n alone: BGNN_LOSS_ROWS_PER_THREAD rows per thread, a shuffle tree
 * within the wave, the waves of a workgroup in index order through LDS, one partial per workgroup of BGNN_LOSS_ROWS_PER_WG rows,
 * and one workgroup that adds the partials (thread t takes partials t, t + BGNN_LOSS_FINISH_WIDTH, ..., then the same tree).
 * There are no float atomics; the counts are integer sums through the same partials.  Each term and each gradient element is
 * rounded to float32 once, and two calls on equal inputs give equal bits.  Nothing is read back to the host.
 */
#ifndef BGNN_LOSS_H
#define BGNN_LOSS_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_LOSS_MAX_CLASSES 16
#define BGNN_LOSS_IGNORE_INDEX (-100)
#define BGNN_LOSS_ROWS_PER_THREAD 4
#define BGNN_LOSS_ROWS_PER_WG 1024  /* 256 threads x BGNN_LOSS_ROWS_PER_THREAD: one partial per this many rows */
#define BGNN_LOSS_FINISH_WIDTH 256  /* partials the finish workgroup reads per pass; it loops above this many */
#define BGNN_LOSS_MAX_ROWS (1ll << 30)

/* order of terms[6] and of term_weights[5] (the total has no weight) */
#define BGNN_LOSS_CLASSIFICATION 0
#define BGNN_LOSS_CORRECTION 1
#define BGNN_LOSS_CONFIDENCE 2
#define BGNN_LOSS_FEATURE_PRESERVATION 3
#define BGNN_LOSS_SHOAL_SAFETY 4
#define BGNN_LOSS_TOTAL 5

/* counts: int64 [C * C + BGNN_LOSS_N_COUNTS]: the confusion matrix (rows true, columns predicted; rows whose label and
 * prediction are both in [0, C)), then these */
#define BGNN_LOSS_COUNT_MASKED 0            /* M */
#define BGNN_LOSS_COUNT_FALSE_POSITIVES 1   /* #FP */
#define BGNN_LOSS_COUNT_SHOAL 2             /* #{FP, target < 0}; 0 without correction_targets */
#define BGNN_LOSS_COUNT_DEEP 3              /* #{FP, not target < 0}; 0 without correction_targets */
#define BGNN_LOSS_COUNT_IGNORED 4           /* labels equal to BGNN_LOSS_IGNORE_INDEX */
#define BGNN_LOSS_COUNT_INVALID 5           /* other labels outside [0, C) */
#define BGNN_LOSS_COUNT_FEATURE_AS_NOISE 6  /* the count of the feature_preservation term */
#define BGNN_LOSS_N_COUNTS 7

/* sums: double [BGNN_LOSS_N_SUMS] at the start of the workspace bgnn_loss_forward filled; what bgnn_loss_backward divides by */
#define BGNN_LOSS_SUM_W 0        /* sum over K of w[y_i] */
#define BGNN_LOSS_SUM_M 1        /* rows of the correction term */
#define BGNN_LOSS_SUM_N 2        /* n */
#define BGNN_LOSS_SUM_WEIGHTS 3  /* sum_c w[c] */
#define BGNN_LOSS_N_SUMS 4

/* What the loss object holds.  HOST. */
typedef struct bgnn_loss_params {
  int32_t num_classes;                    /* C, 2 .. BGNN_LOSS_MAX_CLASSES */
  int32_t has_class_weights;              /* 0: class_weights is not read, every weight is 1 */
  double class_weights[BGNN_LOSS_MAX_CLASSES];
  double label_smoothing;                 /* in [0, 1] */
  double delta;                           /* of the Huber term, > 0 */
  int32_t feature_class, feature_noise_class; /* feature_preservation */
  int32_t seafloor_class, shoal_noise_class;  /* shoal_safety */
  double penalty_weight, shoal_penalty, deep_penalty;
  double term_weights[5];
} bgnn_loss_params;

/* DEVICE pointers, [n] unless said otherwise. */
typedef struct bgnn_loss_inputs {
  const float *logits;             /* [n][C] */
  const float *confidence;
  const float *correction;         /* or NULL */
  const int64_t *predicted_class;
  const int64_t *labels;
  const float *correction_targets; /* or NULL */
  const uint8_t *noise_mask;       /* non-zero = the row is in the correction term; or NULL: every row */
} bgnn_loss_inputs;

/* bgnn_loss_workspace_bytes: bytes of DEVICE workspace bgnn_loss_forward needs for n rows; 0 for n < 1 or n > BGNN_LOSS_MAX_ROWS.
 *
 * bgnn_loss_forward: terms DEVICE float32 [6], counts DEVICE int64 [C * C + BGNN_LOSS_N_COUNTS]; neither needs clearing.  Two
 *   launches on the context's stream (the per-node pass, the finish); asynchronous.  The first BGNN_LOSS_N_SUMS doubles of the
 *   workspace are the `sums` of bgnn_loss_backward and must stay untouched until that call's work has completed.
 *
 * bgnn_loss_backward: upstream DEVICE float32 [3]: d(loss) / d(classification, confidence, correction).  grad_logits [n][C],
 *   grad_confidence [n], grad_correction [n]; each may be NULL (then it is not written); grad_correction is zero-filled when the
 *   correction term is absent.  One launch; the softmax is recomputed.
 *
 * BGNN_ERR_INVALID: NULL arguments, n < 1, C outside 2 .. BGNN_LOSS_MAX_CLASSES, delta not > 0, a workspace that is too small
 *   or not 16-byte aligned.  BGNN_ERR_UNSUPPORTED: n > BGNN_LOSS_MAX_ROWS. */
size_t bgnn_loss_workspace_bytes(int64_t n);
int bgnn_loss_forward(bgnn_ctx *ctx, const bgnn_loss_params *params, int64_t n, const bgnn_loss_inputs *inputs, void *workspace,
                      size_t workspace_bytes, float *terms, int64_t *counts);
int bgnn_loss_backward(bgnn_ctx *ctx, const bgnn_loss_params *params, int64_t n, const bgnn_loss_inputs *inputs,
                       const double *sums, const float *upstream, float *grad_logits, float *grad_confidence,
                       float *grad_correction);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_LOSS_H */
