/*
 * bgnn_features.h -- C ABI of libbgnn_hip.so, feature labels from charted objects (ABI 7, additive; no entry point of bgnn.h or of
 * the other side headers changes): scripts/extract_s57_features.py, create_feature_labels, as device code on a survey plane that
 * stays in HBM.  Every charted wreck, rock and obstruction paints a disc of its class's label onto the survey grid; later features
 * overwrite earlier ones.
 *
 * The float64 geo arithmetic (radius in pixels, centre, bounds check, label lookup) stays with the caller; what arrives here is
 * the int32 table of the applied features in list order, four entries each:
 *     (row, col, radius_px, label)      0 <= row < rows, 0 <= col < cols, radius_px <= min(rows + cols, 2^31 - 1)
 * A cell (r, c) is inside feature k when (c - col)^2 + (r - row)^2 <= radius_px^2 in int64 -- the reference's
 * sqrt(dx^2 + dy^2) <= radius_px on integer operands -- and radius_px >= 0.  A negative radius paints nothing.  Every paintable cell
 * takes the label of the HIGHEST-index feature it is inside: that is "painted in list order".  There are no atomics on the plane and
 * no per-feature pass.
 *
 * Host plan.  The grid is cut into bins of BGNN_FL_BIN x BGNN_FL_BIN cells, row-major, ceil(rows / BIN) x ceil(cols / BIN) of them.
 * For every bin the plan lists, in DESCENDING index, the features whose disc meets the bin (the nearest cell of the bin to the centre
 * is inside the disc; that is never more than the features whose clamped bounding box meets the bin), cut after the first feature
 * whose disc contains all four corner cells of the bin: nothing below it can show.  The plan is one HOST block:
 *     int64  bin_ptr[bins + 1]          bin_ptr[0] = 0; the list of bin b is bin_feat[bin_ptr[b] .. bin_ptr[b + 1])
 *     int32  bin_feat[bin_ptr[bins]]
 * bgnn_feature_labels_plan_bytes and bgnn_feature_labels_plan are pure host functions: no context, no device.
 *
 * The conventions of bgnn.h hold (DEVICE / HOST pointers, return codes, bgnn_last_error(), the context's stream, asynchronous):
 * bgnn_feature_labels does not synchronise with the host, allocate, or copy to the host.  Table and plan travel through the
 * context's pinned staging; the caller's copies may go away when the call returns.  One kernel launch, a workgroup per bin (a
 * bounded number of workgroups: on a large grid each takes several bins).
 *
 * Determinism.  A cell's label is a function of the table alone; the three counts are integer sums (one 64-bit integer add per
 * workgroup and count).  Equal inputs give equal bits.
 *
 * Limits.  rows >= 1, cols >= 1, rows * cols <= BGNN_FL_MAX_CELLS, 0 <= n_features <= BGNN_FL_MAX_FEATURES.  Beyond:
 * BGNN_ERR_UNSUPPORTED.
 */
#ifndef BGNN_FEATURES_H
#define BGNN_FEATURES_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_FL_BIN 64                    /* cells along either side of a bin */
#define BGNN_FL_MAX_CELLS 2147483647      /* rows * cols <= this */
#define BGNN_FL_MAX_FEATURES 2147483646   /* n_features <= this */

/* The statistics block of bgnn_feature_labels (DEVICE, caller-owned, 8-byte aligned, BGNN_FL_STATS_BYTES), cleared and written by
 * the call:
 *   int64   valid          depth mode: cells that are finite and != nodata; overlay mode: cells whose base label is >= 0
 *   int64   feature        cells of the output plane whose label is 1
 *   int64   painted        cells that took their label from a feature (whatever the label) */
#define BGNN_FL_STATS_VALID 0     /* byte offsets */
#define BGNN_FL_STATS_FEATURE 8
#define BGNN_FL_STATS_PAINTED 16
#define BGNN_FL_STATS_BYTES 24

/* bgnn_feature_labels_plan_bytes: the size of the plan of `table` (HOST int32 [n_features][4]; may be NULL when n_features is 0)
 *   on a grid of rows x cols cells: 8 * (bins + 1) + 4 * entries.  0 when the arguments are outside the contract (see
 *   bgnn_feature_labels_plan, which says why).
 * bgnn_feature_labels_plan: writes that plan into `plan` (HOST, 8-byte aligned, plan_bytes >= the size above).
 *   BGNN_ERR_INVALID: a NULL pointer, rows < 1 or cols < 1, n_features < 0, a table entry with its centre outside the grid or a
 *   radius above min(rows + cols, 2^31 - 1), a plan that is too small or misaligned.  BGNN_ERR_UNSUPPORTED: a grid or a feature
 *   count beyond the limits. */
size_t bgnn_feature_labels_plan_bytes(const int32_t *table, int64_t n_features, int64_t rows, int64_t cols);
int bgnn_feature_labels_plan(const int32_t *table, int64_t n_features, int64_t rows, int64_t cols, void *plan, size_t plan_bytes);

/* bgnn_feature_labels_workspace_bytes: plan_bytes and 16 * n_features, each rounded up to 256 bytes; 0 for n_features outside
 *   [0, BGNN_FL_MAX_FEATURES].
 * bgnn_feature_labels: exactly one of depth (DEVICE float32) and base_labels (DEVICE int32) is given; rows x cols cells, row-major.
 *   depth mode    the reference's function: valid = depth != (float)nodata and finite; labels = 0 on valid cells, -1 elsewhere;
 *                 then the valid cells inside a disc take the label of the highest-index feature that holds them
 *   overlay mode  labels = base_labels; only cells whose base label is 0 are painted: -1 (no data), 2 (noise) and every other
 *                 value pass through unchanged.  `nodata` is not read.  labels may be base_labels itself (in place)
 *   table, plan: HOST, as above; the plan is checked against the table and the grid before anything is launched (monotone bin_ptr
 *   that ends at the entry count plan_bytes holds, every index inside the table).  workspace: DEVICE scratch of at least
 *   bgnn_feature_labels_workspace_bytes(n_features, plan_bytes) bytes, 16-byte aligned.  labels: DEVICE int32 [rows][cols].
 *   BGNN_ERR_INVALID: a NULL pointer (table may be NULL when n_features is 0), both planes or neither, rows < 1 or cols < 1,
 *   n_features < 0, a plan that is too small, misaligned or inconsistent, a workspace that is too small or misaligned, a
 *   statistics block that is not 8-byte aligned.  BGNN_ERR_UNSUPPORTED: a grid or a feature count beyond the limits.  Every check
 *   runs before the context or the device is touched. */
size_t bgnn_feature_labels_workspace_bytes(int64_t n_features, size_t plan_bytes);
int bgnn_feature_labels(bgnn_ctx *ctx, const float *depth, const int32_t *base_labels, int64_t rows, int64_t cols, double nodata,
                        const int32_t *table, int64_t n_features, const void *plan, size_t plan_bytes, void *workspace,
                        size_t workspace_bytes, int32_t *labels, void *stats);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_FEATURES_H */
