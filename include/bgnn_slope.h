/*
 * bgnn_slope.h -- C ABI of libbgnn_hip.so, slope-based feature labels (ABI 7, additive; no entry point of bgnn.h or of the other
 * side headers changes): scripts/prepare_feature_labels.py of the reference's training plan (phase 3), create_feature_mask_from_slope
 * and the slope half of add_feature_labels, as device code on a depth plane that stays in HBM.  The wreck discs of that script go
 * through bgnn_feature_labels (bgnn_features.h) in overlay mode afterwards.
 *
 * The conventions of bgnn.h hold (DEVICE / HOST pointers, return codes, bgnn_last_error(), the context's stream, asynchronous):
 * the entry point does not synchronise with the host, allocate, or copy to the host.  The number of launches is fixed (four
 * kernels) and every grid is a function of rows and cols alone.  The Python mirror binds these in bathymetric_gnn_amd/runtime.py
 * (_SLOPE_SIGNATURES); data/slope_features.py drives them.
 *
 * What is computed, on the raw float32 plane, nodata and NaN included (numpy.gradient's arithmetic, float32 throughout):
 *     gy = (d[r+1][c] - d[r-1][c]) * 0.5 inside, d[1][c] - d[0][c] in the first row, d[rows-1][c] - d[rows-2][c] in the last;
 *     gx likewise along a row;   s = gx * gx + gy * gy   (three float32 operations, no contraction);   steep = s >= cut.
 * `cut` is the caller's reduction of the slope threshold: the smallest float32 s whose degrees(arctan(sqrt(s))) exceeds the
 * threshold, found on the host (sqrt, arctan and degrees are monotone); a NaN cut gives an empty mask, a NaN s is never steep.  The
 * 4-connected components of the steep cells (scipy.ndimage.label's default structure) with fewer than min_cluster_size cells are
 * cleared; sizes count every steep cell, valid or not.  What is left is the filtered mask.
 *
 * Determinism.  Labels are a union-find over int32 cell indices (roots are the components' first cells whatever the order of the
 * unions); sizes and the statistics are integer adds.  There are no float atomics: equal inputs give equal bits.
 *
 * Limits.  rows >= 2, cols >= 2 (numpy.gradient refuses a shorter axis) and rows * cols <= BGNN_SL_MAX_CELLS (labels are int32 cell
 * indices).  A larger grid is refused with BGNN_ERR_UNSUPPORTED.
 */
#ifndef BGNN_SLOPE_H
#define BGNN_SLOPE_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_SL_MAX_CELLS 2147483647 /* rows * cols <= this */

/* The statistics block of bgnn_slope_features (DEVICE, caller-owned, 8-byte aligned, BGNN_SL_STATS_BYTES), cleared and written by
 * the call: int64 each, in this order
 *   valid           depth mode: cells that are finite and != nodata; overlay mode: cells whose base label is >= 0
 *   steep           cells with s >= cut
 *   clusters        4-connected components of the steep cells
 *   kept_clusters   components of at least min_cluster_size cells
 *   kept_cells      cells of the kept components (the ones of slope_mask)
 *   feature         cells this call labelled 1: kept and valid in depth mode (the reference's "Slope-based features"), kept with
 *                   a base label of 0 in overlay mode */
#define BGNN_SL_STATS 6
#define BGNN_SL_STATS_BYTES 48

/* bgnn_slope_features_workspace_bytes: 0 for rows < 2, cols < 2 or a grid beyond the limit.  Else, with up(b) = b rounded up to a
 *   multiple of 256: 2 * up(4 * rows * cols) (per cell an int32 parent and an int32 size).
 *
 * bgnn_slope_features: depth (DEVICE float32): a row-major plane of rows x cols cells, the source of the slope.
 *   base_labels (DEVICE int32 plane, or NULL): NULL is depth mode, the reference's function: labels = -1 where depth == (float)nodata
 *   or depth is not finite, else 1 where the filtered mask holds, else 0.  Given, it is overlay mode: labels = base_labels, but the
 *   cells of the filtered mask whose base label is 0 become 1; -1 (no data), 2 (noise) and every other value pass through unchanged
 *   (the rule of bgnn_feature_labels).  `nodata` is not read then.  labels may be base_labels itself (in place).
 *   cut: see above.  min_cluster_size: any value; below 2 every component is kept.
 *   workspace: DEVICE scratch of at least bgnn_slope_features_workspace_bytes(rows, cols) bytes, 4-byte aligned.  Nothing in it has
 *   to be cleared by the caller.
 *   labels: DEVICE int32 [rows][cols]; every cell is written.  slope_mask: DEVICE uint8 [rows][cols] or NULL: 1 on the cells of the
 *   filtered mask, invalid cells included (what create_feature_mask_from_slope returns), 0 elsewhere; every cell is written.
 *   stats: DEVICE, as above.
 *   BGNN_ERR_INVALID: a NULL or misaligned pointer, rows < 2 or cols < 2, a workspace that is too small.  BGNN_ERR_UNSUPPORTED:
 *   rows * cols > BGNN_SL_MAX_CELLS.  Every check runs before the context or the device is touched. */
size_t bgnn_slope_features_workspace_bytes(int64_t rows, int64_t cols);
int bgnn_slope_features(bgnn_ctx *ctx, const float *depth, const int32_t *base_labels, int64_t rows, int64_t cols, double nodata,
                        float cut, int64_t min_cluster_size, void *workspace, size_t workspace_bytes, int32_t *labels,
                        uint8_t *slope_mask, void *stats);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_SLOPE_H */
