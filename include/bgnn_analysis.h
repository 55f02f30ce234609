/*
 * bgnn_analysis.h -- C ABI of libbgnn_hip.so, the noise pattern analysis of a ground truth (ABI 7, additive; no entry point of
 * bgnn.h or of the other side headers changes): scripts/analyze_noise_patterns.py, analyze_ground_truth, as device code on the
 * four planes of a ground truth (labels, difference, noisy depth, clean depth) that stay in HBM.
 *
 * The conventions of bgnn.h hold (DEVICE / HOST pointers, return codes, bgnn_last_error(), the context's stream, asynchronous):
 * no entry point synchronises with the host, allocates, or copies to the host.  The number of launches is fixed: nothing is
 * data-dependent, there is no host loop "until converged".  The Python mirror binds these in bathymetric_gnn_amd/runtime.py
 * (_ANALYSIS_SIGNATURES); data/noise_analysis.py drives them and derives the reference's dictionary from the result block.
 *
 * Determinism.  Every count is an integer sum (LDS and global integer atomics), every float64 sum is formed per thread in a fixed
 * order, reduced per workgroup in a fixed tree, stored as a per-workgroup partial and added in workgroup order by one finishing
 * workgroup; the grids are functions of rows and cols alone.  Cluster sizes are integer atomic adds on the root's counter.  There
 * are no float atomics: equal inputs give equal bits.
 *
 * Limit.  rows >= 1, cols >= 1 and rows * cols < 2^31 (BGNN_NA_MAX_CELLS): cluster labels are int32 cell indices.  A larger grid is
 * refused with BGNN_ERR_UNSUPPORTED.  (20000 x 20000 is 4.0e8 cells; a 60000 x 60000 survey is analysed in bands of rows by the
 * caller or waits for 64-bit labels.)
 */
#ifndef BGNN_ANALYSIS_H
#define BGNN_ANALYSIS_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_NA_MAX_CELLS 2147483647 /* rows * cols <= this */
#define BGNN_NA_DEPTH_BINS 8  /* on -noisy_depth, float32 comparisons: [0,10) [10,20) [20,50) [50,100) [100,200) [200,500) [500,1000) [1000,10000) */
#define BGNN_NA_SIZE_BINS 7   /* cluster sizes: [1,2) [2,5) [5,10) [10,50) [50,100) [100,1000) [1000,10000) */
#define BGNN_NA_MAG_RANKS 6   /* order statistics of |difference|: median lo / hi, p90 lo / hi, p99 lo / hi */

/* The result block of bgnn_noise_analysis (DEVICE, caller-owned, 8-byte aligned, BGNN_NA_BYTES).  valid = labels >= 0,
 * noise = labels == 2, seafloor = labels == 0.  "Noise cells" in the float entries are the noise cells whose difference is finite;
 * the others are counted in `nonfinite` and enter no float entry (the Python layer raises on nonfinite > 0).
 *   int64   valid, noise, seafloor
 *   int64   positive, negative       noise cells with difference > 0 / < 0
 *   int64   nonfinite                noise cells whose difference is NaN or +-inf
 *   int64   bin_noise[8]             noise cells per depth bin (all of them, finite or not)
 *   int64   bin_valid[8]             valid cells per depth bin
 *   double  abs_sum, sq_sum          sum of (double)|d| and of (double)d * (double)d over the noise cells
 *   double  dev_sq_sum               sum of ((double)|d| - abs_sum / n)^2 over the noise cells (second pass: the stable variance)
 *   double  pos_sum, neg_sum         sum of (double)d over the positive / negative noise cells
 *   double  bin_abs_sum[8]           sum of (double)|d| over the noise cells per depth bin
 *   float   abs_max                  max of |d| over the noise cells (0 without one); 4 bytes of padding follow
 *   int64   mag_rank[6]              the ranks numpy's median and percentile(90 / 99) read on a float32 array of n values: median
 *                                    (n - 1) / 2 and n / 2; percentile q: v = (float)(n - 1) * (q / 100f) in float32, floor(v)
 *                                    and floor(v) + 1, both n - 1 where v >= (float)(n - 1); -1 for n == 0
 *   float   mag_value[6]             |d| of those ranks among the noise cells in ascending order: exact selections
 *   int64   num_clusters             4-connected components of the noise mask (scipy.ndimage.label's default structure)
 *   int64   cluster_cells            the sum of their sizes
 *   int64   max_cluster, isolated    the largest size; the number of components of size 1
 *   int64   size_bins[7]             components per size bin (sizes of 10000 and more fall in none)
 *   int64   size_mid[2]              the sizes of ranks (k - 1) / 2 and k / 2 among the k components (0 without one)
 *   int64   rough_count[2]           noise / seafloor cells whose roughness is not NaN
 *   double  rough_sum[2]             the sum of the roughness over them
 *   double  rough_mid[4]             roughness of ranks (m - 1) / 2 and m / 2 among those m cells: noise lo, hi, seafloor lo, hi
 *                                    (NaN for m == 0): exact selections on the float64 values
 * Roughness of a cell: numpy's nanstd of the 5 x 5 window of (double)clean_depth around it, cells outside the grid and NaN cells
 * skipped, two-pass (mean, then mean of squared deviations), NaN when the window holds +-inf. */
#define BGNN_NA_VALID 0     /* byte offsets */
#define BGNN_NA_NOISE 8
#define BGNN_NA_SEAFLOOR 16
#define BGNN_NA_POSITIVE 24
#define BGNN_NA_NEGATIVE 32
#define BGNN_NA_NONFINITE 40
#define BGNN_NA_BIN_NOISE 48
#define BGNN_NA_BIN_VALID 112
#define BGNN_NA_ABS_SUM 176
#define BGNN_NA_SQ_SUM 184
#define BGNN_NA_DEV_SQ_SUM 192
#define BGNN_NA_POS_SUM 200
#define BGNN_NA_NEG_SUM 208
#define BGNN_NA_BIN_ABS_SUM 216
#define BGNN_NA_ABS_MAX 280
#define BGNN_NA_MAG_RANK 288
#define BGNN_NA_MAG_VALUE 336
#define BGNN_NA_NUM_CLUSTERS 360
#define BGNN_NA_CLUSTER_CELLS 368
#define BGNN_NA_MAX_CLUSTER 376
#define BGNN_NA_ISOLATED 384
#define BGNN_NA_SIZE_BINS_OFFSET 392
#define BGNN_NA_SIZE_MID 448
#define BGNN_NA_ROUGH_COUNT 464
#define BGNN_NA_ROUGH_SUM 480
#define BGNN_NA_ROUGH_MID 496
#define BGNN_NA_BYTES 528

/* bgnn_noise_analysis: labels (DEVICE int32), difference, noisy, clean (DEVICE float32): row-major planes of rows x cols cells.
 *   block: the result block above; col_noise, col_valid: DEVICE int32 [cols], the noise / valid cells of every column.  All three
 *   are cleared and written by the call.  workspace: DEVICE scratch of at least bgnn_noise_analysis_workspace_bytes(rows, cols)
 *   bytes, 8-byte aligned: histograms, selection states, per-workgroup partials, and per cell an int32 parent, an int32 size counter
 *   and the float64 roughness (16 bytes / cell).
 *   BGNN_ERR_INVALID: a NULL pointer, rows < 1 or cols < 1, a workspace that is too small or misaligned, a block that is not 8-byte
 *   aligned.  BGNN_ERR_UNSUPPORTED: rows * cols > BGNN_NA_MAX_CELLS.
 * bgnn_noise_analysis_workspace_bytes: 0 for rows < 1, cols < 1 or a grid beyond the limit. */
size_t bgnn_noise_analysis_workspace_bytes(int64_t rows, int64_t cols);
int bgnn_noise_analysis(bgnn_ctx *ctx, const int32_t *labels, const float *difference, const float *noisy, const float *clean,
                        int64_t rows, int64_t cols, void *workspace, size_t workspace_bytes, void *block, int32_t *col_noise,
                        int32_t *col_valid);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_ANALYSIS_H */
