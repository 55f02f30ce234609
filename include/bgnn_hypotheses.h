/*
 * bgnn_hypotheses.h -- C ABI of libbgnn_hip.so, depth hypotheses per cell (ABI 7, additive; no entry point of bgnn.h or of the other
 * side headers changes): the sorted per-cell sounding lists that bgnn_soundings_robust_finalize leaves are cut into runs without a
 * gap, one run a depth hypothesis, and one of them is chosen per cell.  What the one depth per cell of both gridders cannot give:
 * a cell that straddles a step (a wreck, a pier face) or holds a dense false cluster (a fish school) keeps its surfaces apart
 * instead of averaging across them.  CUBE-style disambiguation without CUBE's sequential estimator, which depends on the order of
 * arrival.
 *
 * The conventions of bgnn_soundings_robust.h hold (DEVICE pointers owned by the caller, return codes, bgnn_last_error(), the
 * context's stream, asynchronous): no entry point synchronises with the host, allocates, or copies to the host; refusals happen
 * before any launch, the context checked last; no launch geometry depends on a device value.  The Python mirror binds these in
 * bathymetric_gnn_amd/runtime.py (_HYPOTHESES_SIGNATURES); data/sounding_hypotheses.py drives them.
 *
 * The inputs are `start` (uint32, cells + 1) and `sorted_q` (int32, capacity entries, ascending inside a cell) of a robust
 * finalize; x and y are never looked at, so a VR layout of `total` records is cells = total, as the finalize treats it.
 *
 * Per cell with segment s[0 .. n), all in integers (csrc/sounding_hypothesis.h):
 *     a break sits before i (1 <= i < n) iff (int64)s[i] - (int64)s[i-1] > gap_q        (the difference reaches 2^32 - 1)
 *     hypothesis h is the h-th run [a_h, b_h) between breaks, ascending in depth; n_h = b_h - a_h
 *     m2_h = s[a_h + (n_h-1)/2] + s[a_h + n_h/2]                                         twice its median
 *     n_hyp = 0 for an empty cell
 * gap_q: 0 .. 2^32 (at 2^32 every non-empty cell is one hypothesis, at 0 only equal values merge).  The candidates are the
 * hypotheses with n_h >= min_count; the chosen one has the smallest key, compared lexicographically, all int64:
 *     BGNN_HYP_RULE_COUNT   (-n_h, |m2_h - c2|, h), c2 = s[(n-1)/2] + s[n/2] twice the cell's median; guide must be NULL
 *     BGNN_HYP_RULE_GUIDE   (|m2_h - g2|, -n_h, h), g2 = 2 * llrint((double)g * 65536.0), g the cell's entry of `guide` (DEVICE
 *                           float32, cells entries); a cell whose g is not finite or has |g| >= 32768 takes the COUNT key
 * No candidate: chosen = -1.
 *
 * The planes, `cells` entries each; the float planes hold nodata_value where valid == 0:
 *     n_hyp      int32    the number of hypotheses, also where valid == 0
 *     chosen     int32    the index of the chosen hypothesis, or -1
 *     kept       int32    n_h of the chosen one, 0 where none
 *     depth, std float32  the mean and std formulas of bgnn_soundings.h over the chosen run (exact integer sums, one rounding)
 *     min, max   float32  (float)((double)q * 2^-16) of the run's first and last sounding
 *     share      float32  (float)((double)n_h / (double)n)
 *     valid      uint8    chosen >= 0
 *     center2    int64    s[a] + s[b-1] of the chosen run, 0 where none
 *     limit      int64    s[b-1] - s[a] of the chosen run, -1 where none
 * |2q - center2| <= limit iff s[a] <= q <= s[b-1]: bgnn_soundings_robust_flag and bgnn_vr_soundings_flag apply a hypothesis result
 * as they are.
 *
 * The records, optional (all three NULL or none): hyp_start (uint32, cells + 1: the hypotheses in front of cell c, hyp_start[cells]
 * the total), hyp_first (uint32, capacity: the index into sorted_q of each hypothesis's first sounding, in cell order and then
 * ascending) and hyp_count (int32, capacity).  The total never exceeds the accepted soundings.
 *
 * Every output is a function of the sorted segments alone: equal bits in any order, in any split over calls, on every run.
 */
#ifndef BGNN_HYPOTHESES_H
#define BGNN_HYPOTHESES_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_HYP_RULE_COUNT 0                 /* the most soundings, then the nearest to the cell's median */
#define BGNN_HYP_RULE_GUIDE 1                 /* the nearest to the guide surface, then the most soundings */
#define BGNN_HYP_MAX_CELLS 2147483647
#define BGNN_HYP_MAX_CAPACITY 2147483647      /* the entries of sorted_q, hyp_first and hyp_count */
#define BGNN_HYP_MAX_GAP_Q 4294967296         /* 2^32, in units of 2^-16 m */

/* bgnn_hypotheses_workspace_bytes: what build needs beside its outputs (the partials of the scan, the list of cells with more than
 *   BGNN_ROBUST_WAVE_MAX soundings); 0 for cells outside 1 .. BGNN_HYP_MAX_CELLS or capacity outside 1 .. BGNN_HYP_MAX_CAPACITY.
 * bgnn_hypotheses_build: the eleven planes, and the records where they are given, from start and sorted_q, which it only reads.
 *   workspace: DEVICE, 8-byte aligned, workspace_bytes of bgnn_hypotheses_workspace_bytes(cells, capacity) at least.
 *   BGNN_ERR_INVALID: a NULL argument, cells or capacity outside their ranges, gap_q outside 0 .. BGNN_HYP_MAX_GAP_Q, an unknown
 *   rule, a guide with BGNN_HYP_RULE_COUNT or none with BGNN_HYP_RULE_GUIDE, min_count < 1, a workspace that is too small, a
 *   workspace, center2 or limit that is not 8-byte aligned, records given in part. */
size_t bgnn_hypotheses_workspace_bytes(int64_t cells, int64_t capacity);
int bgnn_hypotheses_build(bgnn_ctx *ctx, const uint32_t *start, const int32_t *sorted_q, int64_t cells, int64_t capacity, int64_t gap_q,
                          int32_t rule, const float *guide, int32_t min_count, float nodata_value, void *workspace,
                          size_t workspace_bytes, int32_t *n_hyp, int32_t *chosen, int32_t *kept, float *depth, float *stddev,
                          float *zmin, float *zmax, float *share, uint8_t *valid, int64_t *center2, int64_t *limit,
                          uint32_t *hyp_start, uint32_t *hyp_first, int32_t *hyp_count);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_HYPOTHESES_H */
