/*
 * bgnn_review.h -- C ABI of libbgnn_hip.so, the export of low-confidence regions for review (ABI 7, additive; no entry point of
 * bgnn.h or of the other side headers changes): scripts/export_for_review.py of the reference's training plan (step 5.1), as device
 * code on the confidence plane of a finished inference that stays in HBM.
 *
 * The conventions of bgnn.h hold (DEVICE / HOST pointers, return codes, bgnn_last_error(), the context's stream, asynchronous):
 * no entry point synchronises with the host, allocates, or copies to the host.  The number of launches is fixed (six kernels) and
 * every grid is a function of rows and cols alone: nothing is data-dependent, there is no host loop "until converged".  The Python
 * mirror binds these in bathymetric_gnn_amd/runtime.py (_REVIEW_SIGNATURES); data/review_regions.py drives them and derives the
 * reference's list of regions from the record table.
 *
 * What is computed.  uncertain = conf >= low && conf <= high && finite(conf), compared in float32, both bounds inclusive.  The
 * 4-connected components of that mask (scipy.ndimage.label's default structure; diagonal contact does not join) are the regions; a
 * region is kept when it has at least min_region_size cells.  The kept regions are reported in ascending order of their first cell
 * in row-major order, which is the order ndimage.label numbers them.
 *
 * Determinism.  Labels are a union-find over int32 cell indices whose roots are the components' first cells whatever the order of
 * the unions.  Sizes, bounds and confidence sums are integer adds / minima / maxima (LDS and global integer atomics): the confidence
 * enters as the fixed-point integer llrint((double)c * 2^32), so its sum does not depend on the order of the adds.  The record table
 * is filled by an ordered compaction (every workgroup owns a contiguous range of cells; one workgroup scans the per-workgroup counts).
 * There are no float atomics: equal inputs give equal bits.
 *
 * Limit.  rows >= 1, cols >= 1 and rows * cols < 2^31 (BGNN_RV_MAX_CELLS, the limit of BGNN_NA_MAX_CELLS and for its reason: labels
 * are int32 cell indices).  A larger grid is refused with BGNN_ERR_UNSUPPORTED.
 *
 * Deviation from the reference's signature.  The bounds must lie in [0, 1]: that is the range of the fixed-point sum (a cell adds at
 * most 2^32, fewer than 2^31 cells: the uint64 sum cannot overflow), and the confidence is a sigmoid output.  The reference accepts
 * any pair of floats.
 */
#ifndef BGNN_REVIEW_H
#define BGNN_REVIEW_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_RV_MAX_CELLS 2147483647 /* rows * cols <= this */
#define BGNN_RV_COUNTS 4             /* int64 counts[4]: uncertain cells, components, kept components, cells in kept components */
#define BGNN_RV_RECORD_BYTES 40
#define BGNN_RV_FIXED_BYTES 81920    /* the fixed part of the workspace */

/* One kept region.  conf_sum / 2^32 / size is its mean confidence, exact to 2^-33 (half a unit of the fixed-point format per cell). */
typedef struct bgnn_review_record {
  int64_t first;      /* the region's first cell in row-major order: row * cols + col */
  int64_t size;       /* cells */
  int32_t min_row;    /* the bounding box, inclusive */
  int32_t max_row;
  int32_t min_col;
  int32_t max_col;
  uint64_t conf_sum;  /* sum over the cells of llrint((double)confidence * 2^32) */
} bgnn_review_record;

/* bgnn_review_workspace_bytes: 0 for rows < 1, cols < 1 or a grid beyond the limit.  Else, with cells = rows * cols and
 *   up(b) = b rounded up to a multiple of 256:
 *       BGNN_RV_FIXED_BYTES + 6 * up(4 * cells) + up(8 * cells)
 *   (per cell an int32 parent, an int32 size, four int32 bounds and the uint64 sum: 32 bytes; the fixed part holds the
 *   per-workgroup counts and record bases of the compaction).
 *
 * bgnn_review_regions: confidence (DEVICE float32): a row-major plane of rows x cols cells.
 *   low, high: the inclusive bounds, already rounded to float32 (numpy rounds a Python float so when it compares it with a float32
 *   array).  min_region_size >= 1.
 *   workspace: DEVICE scratch of at least bgnn_review_workspace_bytes(rows, cols) bytes, 8-byte aligned.  Nothing in it has to be
 *   cleared by the caller.
 *   records: DEVICE table of `capacity` bgnn_review_record, 8-byte aligned (may be NULL when capacity is 0).  The first
 *   min(counts[2], capacity) entries are written, in the order above; the others are left as they are.
 *   counts: DEVICE int64 [BGNN_RV_COUNTS], always the true numbers: counts[2] > capacity tells the caller that the table was too
 *   small; it calls again with a table of counts[2] entries.
 *   review_mask: DEVICE float32 plane of rows x cols, or NULL: 1.0 on every uncertain cell whose region is kept, 0.0 elsewhere;
 *   every cell is written.
 *   BGNN_ERR_INVALID: a NULL or misaligned pointer, rows < 1 or cols < 1, a workspace that is too small, min_region_size < 1,
 *   capacity < 0, bounds that are not finite, low > high, a bound outside [0, 1].  BGNN_ERR_UNSUPPORTED: rows * cols >
 *   BGNN_RV_MAX_CELLS. */
size_t bgnn_review_workspace_bytes(int64_t rows, int64_t cols);
int bgnn_review_regions(bgnn_ctx *ctx, const float *confidence, int64_t rows, int64_t cols, float low, float high,
                        int64_t min_region_size, void *workspace, size_t workspace_bytes, void *records, int64_t capacity,
                        int64_t *counts, float *review_mask);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_REVIEW_H */
