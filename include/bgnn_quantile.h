/*
 * bgnn_quantile.h -- C ABI of libbgnn_hip.so, exact percentiles of a stream of errors that never leaves the device (ABI 7,
 * additive; no entry point of bgnn.h or of the other side headers changes): the device half of the adaptive Huber delta the
 * reference defers (training/losses.py compute_correction_delta, Options 2 and 3: the percentile of |predicted - target| over an
 * epoch).  Every training step files its masked errors into a caller-owned stage with one launch and no host wait; at the end of
 * the epoch one selection returns the exact order statistics that numpy's linear interpolation needs.
 *
 * The conventions of bgnn_trainer.h hold (DEVICE / HOST pointers, return codes, bgnn_last_error(), the context's stream,
 * asynchronous): no entry point synchronises with the host, allocates, or copies to the host; every check runs before the device
 * is touched.  The Python mirror binds these in bathymetric_gnn_amd/runtime.py (_QUANTILE_SIGNATURES); training/huber_delta.py
 * (CorrectionErrorTracker, device_percentile) drives them.
 *
 * Determinism.  The stage's ORDER depends on how the waves interleave and is not part of the contract; its MULTISET, every
 * counter, the histogram and therefore every selected value are integers added by integer atomics: equal inputs give equal bits.
 * There are no float atomics and no float sums.
 */
#ifndef BGNN_QUANTILE_H
#define BGNN_QUANTILE_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_QUANTILE_MAX_FRACTIONS 3
#define BGNN_QUANTILE_TOP_BITS 11        /* the key's top digit: the state's histogram has 2^11 bins, bin = key >> 21 */
#define BGNN_QUANTILE_MAX_GRID 2048      /* workgroups of a pass; each takes shares of BGNN_QUANTILE_WG_ROWS rows */
#define BGNN_QUANTILE_WG_ROWS 4096

/* The stage (DEVICE, caller-owned, 4-byte aligned): uint32 [capacity], 1 <= capacity < 2^32.  Slot s < filed holds the key of one
 * filed value: the order-preserving image of its float32 bits,
 *     key(v) = bits(v) | 0x80000000 for a clear sign bit, ~bits(v) for a set one,
 * so that unsigned key order is float order (-0.0 sorts directly below +0.0).  Slots at and beyond `filed` are never written.
 *
 * The state block (DEVICE, caller-owned, 8-byte aligned, BGNN_QUANTILE_STATE_BYTES), since the last reset:
 *   int64  rows        rows with mask != 0 (every row without a mask)            = filed + dropped + nonfinite
 *   int64  filed       values in the stage
 *   int64  nonfinite   masked rows whose value was NaN or +-inf: counted, not filed
 *   int64  dropped     finite masked rows that found the stage full: counted, not filed
 *   int64  cursor      the slot reservations made so far (filed + dropped); words 5 .. 7 are reserved, zero
 *   uint32 hist[2048]  the filed keys per top digit (key >> 21): the first level of the selection, counted by the pass that files */
#define BGNN_QUANTILE_ST_ROWS 0          /* byte offsets */
#define BGNN_QUANTILE_ST_FILED 8
#define BGNN_QUANTILE_ST_NONFINITE 16
#define BGNN_QUANTILE_ST_DROPPED 24
#define BGNN_QUANTILE_ST_CURSOR 32
#define BGNN_QUANTILE_ST_HIST 64
#define BGNN_QUANTILE_STATE_BYTES (64 + 4 * (1 << BGNN_QUANTILE_TOP_BITS))

/* The result block of a selection (DEVICE, caller-owned, 8-byte aligned, BGNN_QUANTILE_OUT_BYTES; the caller reads it back in one
 * copy):
 *   int64  count M, nonfinite, dropped, rows           the state's filed, nonfinite, dropped, rows
 *   per fraction k < BGNN_QUANTILE_MAX_FRACTIONS, 24 bytes at BGNN_QUANTILE_OUT_RANKS + 24 k:
 *     int64 lo, hi; float32 v_lo, v_hi                 the two ranks and the exact order statistics at them
 *       vi = (double)(M - 1) * f_k  (one float64 product), lo = (int64)floor(vi), hi = min(lo + 1, M - 1)
 *   M == 0, and every k >= n_fractions: lo = hi = -1, v_lo = v_hi = NaN.
 * The host interpolates as numpy's method "linear" does on float64 values:
 *     g = vi - lo; a = v_lo; b = v_hi; d = b - a; r = a + d * g; if g >= 0.5: r = b - d * (1 - g); if d == 0: r = a
 * which equals float(np.percentile(values.astype(np.float64), 100 f_k)) bit for bit.
 * dropped > 0: the stage holds whichever finite masked rows arrived first; the values describe those and the caller must
 * discard them.  Only the fact of overflow is deterministic: filed + dropped is the number of finite masked rows. */
#define BGNN_QUANTILE_OUT_COUNT 0        /* byte offsets */
#define BGNN_QUANTILE_OUT_NONFINITE 8
#define BGNN_QUANTILE_OUT_DROPPED 16
#define BGNN_QUANTILE_OUT_ROWS 24
#define BGNN_QUANTILE_OUT_RANKS 32
#define BGNN_QUANTILE_OUT_RANK_BYTES 24
#define BGNN_QUANTILE_OUT_BYTES (32 + 24 * BGNN_QUANTILE_MAX_FRACTIONS)

/* bgnn_quantile_reset: zeroes the state block (the stage needs no clearing).
 * bgnn_quantile_add: files the values of n rows, one launch.  correction, target: DEVICE float32 [n]; mask: DEVICE uint8 [n] or
 *   NULL (every row).  For every row with mask != 0 the value is e = fabsf(correction - target), a float32 subtraction (the bits of
 *   torch's (c - t).abs()); target == NULL: e = correction as it stands, sign included (a percentile of any float32 array).  A
 *   non-finite e is counted in nonfinite; a finite one reserves a slot (per workgroup and share of 4096 rows: ballots, prefix population counts,
 *   one integer atomic on the cursor), is written there when the slot is below capacity and counted in filed and in hist, and is counted in
 *   dropped otherwise.  Nothing is written at or beyond stage + capacity.  n == 0 launches nothing.
 * bgnn_quantile_workspace_bytes: the workspace of bgnn_quantile_select for a stage of `capacity` slots; 0 for a capacity outside
 *   1 .. 2^32 - 1.
 * bgnn_quantile_select: the order statistics of n_fractions fractions f_k = p_k / 100 (HOST float64 [n_fractions], read during
 *   the call) over the filed keys: up to six ranks in one run of the shared radix selection (csrc/radix_select.h), whose first
 *   level is the state's histogram; two passes over the stage count the lower digits.  Writes the result block; the state and the
 *   stage are only read, so further adds and selections may follow.  workspace: DEVICE, 8-byte aligned.
 *   BGNN_ERR_INVALID: NULL ctx / correction / stage / state / fractions / workspace / out, n < 0, capacity < 1 or >= 2^32,
 *   n_fractions outside 1 .. 3, a fraction outside [0, 1] or NaN, a stage that is not 4-byte aligned, a state, workspace or result
 *   block that is not 8-byte aligned, a workspace smaller than bgnn_quantile_workspace_bytes(capacity). */
int bgnn_quantile_reset(bgnn_ctx *ctx, void *state);
int bgnn_quantile_add(bgnn_ctx *ctx, int64_t n, const float *correction, const float *target, const uint8_t *mask, uint32_t *stage,
                      int64_t capacity, void *state);
size_t bgnn_quantile_workspace_bytes(int64_t capacity);
int bgnn_quantile_select(bgnn_ctx *ctx, const uint32_t *stage, int64_t capacity, const void *state, const double *fractions,
                         int32_t n_fractions, void *workspace, size_t workspace_bytes, void *out);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_QUANTILE_H */
