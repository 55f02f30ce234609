/*
 * bgnn_soundings_robust.h -- C ABI of libbgnn_hip.so, robust gridding of a point cloud of soundings (ABI 7, additive; no entry
 * point of bgnn.h or of the other side headers changes): the accepted soundings are kept, filed by cell and sorted per cell, and
 * the median, the median absolute deviation and a kept / rejected rule per cell are read off the sorted segments.  What the
 * streaming sums of bgnn_soundings.h cannot give: a surface that a few bad soundings do not move, and which soundings those are
 * (the reference: docs/LESSONS_LEARNED.md section 6, docs/TRAINING_DASHBOARD.md "Next Steps" 5).
 *
 * The conventions of bgnn_eval.h hold (DEVICE pointers owned by the caller, return codes, bgnn_last_error(), the context's stream,
 * asynchronous): no entry point synchronises with the host, allocates, or copies to the host; refusals happen before any launch;
 * no launch geometry depends on a value read back.  The Python mirror binds these in bathymetric_gnn_amd/runtime.py
 * (_ROBUST_SIGNATURES); data/sounding_robust.py drives them.
 *
 * Grid, acceptance, counters and quantisation are those of bgnn_soundings.h: col = floor((x - x0) / res), row = floor((y0 - y) /
 * res) in float64 (csrc/sounding_cell.h); nonfinite, outside, out_of_range (|z| >= 32768), accepted, checked in that order;
 * q = llrint((double)z * 65536.0).  One more limit: height * width <= 2^31 - 1, so that a cell fits the int32 of the stage;
 * beyond, BGNN_ERR_UNSUPPORTED.
 *
 * The stage.  BGNN_ROBUST_STAGE_HEADER_BYTES of counters (int64 accepted, nonfinite, outside, out_of_range) and then `capacity`
 * slots of (int32 cell, int32 q): sounding offered + i of an add call goes into slot offered + i, with cell = -1 where it is not
 * accepted.  Slots are positional, so the stage itself is the same bits in any split over calls.  8 bytes per sounding.  An
 * all-zero header is the empty stage; slots at and past `offered` are never read.
 *
 * Finalize reads the first `offered` slots only (more may be added afterwards, and finalize run again): it counts the soundings
 * per cell with integer atomics, scans the counts into start[cells + 1] (uint32, start[cells] = accepted), scatters q into
 * sorted_q (capacity int32) through per-cell cursors and sorts every segment sorted_q[start[c] .. start[c + 1]) ascending, in
 * place: after the sort nothing depends on the order in which the cursors were taken.  Segments of up to BGNN_ROBUST_WAVE_MAX
 * soundings are ranked inside a wave, up to BGNN_ROBUST_LDS_MAX one workgroup sorts in LDS, anything longer is radix-sorted by one
 * workgroup through the workspace (correct for any length up to capacity, and slow: one workgroup's bandwidth).
 *
 * Per cell with n >= 1, s the sorted segment, all in integers (csrc/sounding_rank.h):
 *     m2 = s[(n-1)/2] + s[n/2]                    twice the median, in units of 2^-17 m
 *     d_i = |2 s_i - m2|                          int64, below 2^33
 *     D = d_((n-1)/2) + d_(n/2) of the sorted d   twice the MAD of the doubled distances
 *     Td = max(k * ((double)D * 0.5), floor_m * 131072.0)      float64, operation by operation
 *     L = (int64)floor(min(Td, 2^34))
 *     sounding i is kept iff d_i <= L
 * k is the caller's multiplier (1.4826 folded in where sigma units are wanted), finite and >= 1; floor_m (metres) finite and >= 0.
 * With k >= 1 at least (n-1)/2 + 1 soundings are kept; the kept ones are a contiguous range of s; floor_m >= 65536 keeps all.
 *
 * The planes, height * width entries each, valid = kept >= min_count; the float planes hold nodata_value where valid == 0:
 *     count      int32    n, also where valid == 0
 *     kept       int32    the number of kept soundings, also where valid == 0
 *     median     float32  (float)((double)m2 * 2^-17)
 *     mad        float32  (float)((double)D * 2^-18)      (not scaled by 1.4826)
 *     kept_mean  float32  the mean formula of bgnn_soundings.h over the kept soundings
 *     kept_std   float32  the std formula of bgnn_soundings.h over the kept soundings (the exact numerator n S2 - S1^2)
 *     kept_min, kept_max  float32  (float)((double)q * 2^-16) of the first and of the last kept sounding
 *     valid      uint8
 *     center2    int64    m2 (0 for n == 0)
 *     limit      int64    L (-1 for n == 0): with center2 the per-cell rule that bgnn_soundings_robust_flag applies
 * Every plane is a function of the multiset of soundings alone: equal bits in any order, in any split over calls, on every run.
 */
#ifndef BGNN_SOUNDINGS_ROBUST_H
#define BGNN_SOUNDINGS_ROBUST_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_ROBUST_STAGE_HEADER_BYTES 32     /* int64 accepted, nonfinite, outside, out_of_range: the front of the stage */
#define BGNN_ROBUST_SLOT_BYTES 8              /* int32 cell (-1: not accepted), int32 q */
#define BGNN_ROBUST_MAX_CAPACITY 2147483647   /* soundings of one stage */
#define BGNN_ROBUST_MAX_CELLS 2147483647      /* height * width */
#define BGNN_ROBUST_WAVE_MAX 64               /* the longest segment ranked inside a wave */
#define BGNN_ROBUST_LDS_MAX 4096              /* the longest segment one workgroup sorts in LDS */
#define BGNN_ROBUST_FLAG_KEPT 0
#define BGNN_ROBUST_FLAG_REJECTED 1           /* accepted, but |2q - center2| > limit (every accepted sounding of an empty cell) */
#define BGNN_ROBUST_FLAG_NOT_ACCEPTED 2       /* nonfinite, outside or out of range */

/* bgnn_soundings_robust_stage_bytes: BGNN_ROBUST_STAGE_HEADER_BYTES + BGNN_ROBUST_SLOT_BYTES * capacity; 0 for capacity outside
 *   1 .. BGNN_ROBUST_MAX_CAPACITY or where that does not fit size_t.  The stage is a DEVICE block, caller-owned, 8-byte aligned.
 * bgnn_soundings_robust_workspace_bytes: what finalize needs beside its outputs (the counts and cursors, 4 bytes per cell; the
 *   partials of the scan; the list of segments longer than BGNN_ROBUST_WAVE_MAX; capacity int32 for the radix sort); 0 for a grid
 *   or a capacity outside the limits or where it does not fit size_t.
 * bgnn_soundings_robust_reset: zeroes the counters in front of the stage.
 * bgnn_soundings_robust_add: x, y (DEVICE float64) and z (DEVICE float32), n entries each, into slots offered .. offered + n - 1.
 *   offered: the soundings offered to this stage by the calls before this one (the caller's count; nothing is read back).
 *   n == 0 launches nothing.  BGNN_ERR_INVALID: NULL ctx / x / y / z / stage (x, y, z may be NULL when n == 0), res not a finite
 *   number above 0, x0 or y0 not finite, height or width outside 1 .. 2^31 - 1, capacity outside 1 .. BGNN_ROBUST_MAX_CAPACITY,
 *   n < 0, offered < 0, offered + n above capacity, a stage that is not 8-byte aligned.  BGNN_ERR_UNSUPPORTED: height * width above
 *   BGNN_ROBUST_MAX_CELLS.
 * bgnn_soundings_robust_finalize: start (uint32, height * width + 1), sorted_q (int32, capacity) and the eleven planes from the
 *   first `offered` slots of the stage, which it only reads.  workspace: DEVICE, 8-byte aligned, workspace_bytes of
 *   bgnn_soundings_robust_workspace_bytes(height, width, capacity) at least.  BGNN_ERR_INVALID: a NULL argument, height or width
 *   outside 1 .. 2^31 - 1, capacity outside its range, offered outside 0 .. capacity, k not finite or below 1, floor_m not finite or
 *   below 0, min_count < 1, a workspace that is too small, a stage, workspace, center2 or limit that is not 8-byte aligned.
 *   BGNN_ERR_UNSUPPORTED: height * width above BGNN_ROBUST_MAX_CELLS.
 * bgnn_soundings_robust_flag: one streaming pass, stateless, over any n soundings: flags[i] (uint8) is BGNN_ROBUST_FLAG_KEPT,
 *   _REJECTED or _NOT_ACCEPTED under the rule (center2, limit) of the sounding's cell.  BGNN_ERR_INVALID / BGNN_ERR_UNSUPPORTED as
 *   for add, for NULL center2 / limit / flags (flags, x, y, z may be NULL when n == 0) and for misaligned center2 / limit. */
size_t bgnn_soundings_robust_stage_bytes(int64_t capacity);
size_t bgnn_soundings_robust_workspace_bytes(int64_t height, int64_t width, int64_t capacity);
int bgnn_soundings_robust_reset(bgnn_ctx *ctx, void *stage);
int bgnn_soundings_robust_add(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0, double y0,
                              double res, int64_t height, int64_t width, int64_t offered, int64_t capacity, void *stage);
int bgnn_soundings_robust_finalize(bgnn_ctx *ctx, const void *stage, int64_t offered, int64_t capacity, int64_t height, int64_t width,
                                   double k, double floor_m, int32_t min_count, float nodata_value, void *workspace,
                                   size_t workspace_bytes, uint32_t *start, int32_t *sorted_q, int32_t *count, int32_t *kept,
                                   float *median, float *mad, float *kept_mean, float *kept_std, float *kept_min, float *kept_max,
                                   uint8_t *valid, int64_t *center2, int64_t *limit);
int bgnn_soundings_robust_flag(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0, double y0,
                               double res, int64_t height, int64_t width, const int64_t *center2, const int64_t *limit, uint8_t *flags);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_SOUNDINGS_ROBUST_H */
