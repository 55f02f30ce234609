/*
 * bgnn_vrtruth.h -- C ABI of libbgnn_hip.so, ground truth at native resolution from a clean / noisy VR BAG pair (ABI 7, additive; no
 * entry point of bgnn.h or of the other side headers changes): step 1.2 of the reference's docs/TRAINING_PLAN.md,
 * compute_ground_truth_native -- labels per refinement grid, not per cell of a resampled raster -- with both files' refinement
 * records resident in HBM.
 *
 * The records are BAG varres_refinements as they are: float32 [N][2] = (depth, depth_uncrt), 8 bytes per record.  Which grid of the
 * noisy file faces which record range of the clean file is decided on the host (data/vr_ground_truth.py: vr_pair_table) and comes
 * in as a HOST pair table of n_grids rows in the noisy file's iteration order (row-major over the base grid, cells of a zero
 * dimension skipped).  A row names the grid's place in the flat outputs (out_offset, back to back in table order), its number of
 * cells, where its records start in the noisy file and where its twin's start in the clean file (clean_start = -1: no twin).  Every
 * row is checked before anything is launched (cells >= 1; out_offset equal to the cells before it, the last row ending at
 * total_cells; noisy_start >= 0 and noisy_start + cells <= n_noisy; clean_start == -1, or clean_start >= 0 and clean_start + cells <=
 * n_clean); then the table travels through the context's pinned staging into the caller's workspace: the caller's copy may go away
 * when the call returns.  The kernels read records only through checked rows: they cannot leave either record array.
 *
 * Per cell, in float32 (nd, nu: the noisy record; cd: the clean depth of the same cell of the twin):
 *     noisy_depth = nd, uncertainty = nu                                          every grid, paired or not
 *   paired grid:
 *     difference  = nd - cd
 *     valid       = nd finite and != (float)nodata, cd finite and != (float)nodata
 *     labels      = 2 where |difference| > (float)noise_threshold on valid cells, 0 on the other valid cells, -1 on invalid ones
 *                   (the threshold rounded to float32 first, as numpy compares a float32 array with a Python float)
 *     mask        = valid
 *   unpaired grid:
 *     difference  = NaN (0x7fc00000), labels = -1, mask = 0
 * There is no removal of a systematic offset: the plan has none.
 *
 * grid_counts: per grid the cells that are valid | labelled 0 | labelled 1 (always 0 here) | labelled 2: the columns of
 * bgnn_tile_scan's table (BGNN_TILE_COUNTS), so that the keep rule of the tile stores reads either.
 *
 * The statistics block (DEVICE, caller-owned, 8-byte aligned, BGNN_VT_STATS_BYTES):
 *   int64   valid              cells labelled 0 or 2
 *   int64   noise              cells labelled 2
 *   int64   seafloor           cells labelled 0
 *   double  noise_abs_sum      sum of (double)|difference| over the noise cells
 *   double  noise_abs_median   numpy.median of the float64 copies of |difference| over the noise cells: the element of rank
 *                              (n - 1) / 2 for an odd count n, (a + b) / 2 in float64 of ranks n / 2 - 1 and n / 2 for an even one;
 *                              NaN without a noise cell.  An exact radix selection (three digits of 11 / 11 / 10 bits); no sort
 *   float   noise_abs_max      max of |difference| over the noise cells (0 without one)
 *
 * The conventions of bgnn.h hold (DEVICE / HOST pointers, return codes, bgnn_last_error(), the context's stream, asynchronous): the
 * entry point does not synchronise with the host, allocate, or copy to the host.  Every argument check runs before the context or
 * the device is touched.  The Python mirror binds these in bathymetric_gnn_amd/runtime.py (_VRTRUTH_SIGNATURES);
 * data/vr_ground_truth.py drives them.
 *
 * Geometry.  The grid is a function of total_cells alone.  A workgroup owns a contiguous run of output cells, in tiles of
 * BGNN_VT_TILE_CELLS; it finds the grid of its first cell once, by binary search of the offsets, and walks the table from there: per
 * tile the offsets of the grids that meet the tile are staged in LDS and a thread places its four consecutive cells among them.
 * Record loads are 8 bytes (a record is always 8-byte aligned), output stores 16 bytes.  Every cell address is 64-bit.
 *
 * Determinism.  Counts are integer sums (LDS and global integer atomics); the float64 sum is formed per thread in a fixed order,
 * reduced per workgroup in a fixed tree, stored as a per-workgroup partial and added in workgroup order by one finishing workgroup.
 * There are no float atomics.  Equal inputs give equal bits.
 */
#ifndef BGNN_VRTRUTH_H
#define BGNN_VRTRUTH_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_VT_PAIR_BYTES 32       /* sizeof(bgnn_vr_pair) */
#define BGNN_VT_TILE_CELLS 1024     /* output cells a workgroup takes per step */
#define BGNN_VT_COUNTS 4            /* int64 counts per grid: valid, class 0, class 1, class 2 (== BGNN_TILE_COUNTS) */

#define BGNN_VT_STATS_VALID 0       /* byte offsets */
#define BGNN_VT_STATS_NOISE 8
#define BGNN_VT_STATS_SEAFLOOR 16
#define BGNN_VT_STATS_NOISE_ABS_SUM 24
#define BGNN_VT_STATS_NOISE_ABS_MEDIAN 32
#define BGNN_VT_STATS_NOISE_ABS_MAX 40
#define BGNN_VT_STATS_BYTES 48

typedef struct bgnn_vr_pair {
  int64_t out_offset;    /* first cell of the grid in the flat outputs */
  int64_t cells;         /* rows * columns of the grid */
  int64_t noisy_start;   /* first record of the grid in the noisy file */
  int64_t clean_start;   /* first record of its twin in the clean file, or -1 */
} bgnn_vr_pair;

/* bgnn_vr_ground_truth_workspace_bytes: the staged table, the selection's histograms and state, the per-workgroup partials; rounded
 * up to 256.  0 for total_cells < 0 or n_grids < 0. */
size_t bgnn_vr_ground_truth_workspace_bytes(int64_t total_cells, int64_t n_grids);

/* bgnn_vr_ground_truth:
 *   noisy, clean: DEVICE float32 [n_noisy][2] / [n_clean][2], 8-byte aligned.  clean may be NULL when n_clean == 0 (no row can then
 *   name a twin).
 *   pairs: HOST, n_grids rows (see above).  ws: DEVICE scratch of at least bgnn_vr_ground_truth_workspace_bytes(total_cells, n_grids)
 *   bytes, 16-byte aligned.
 *   labels (int32), difference, noisy_depth, uncertainty (float32; uncertainty may be NULL): DEVICE, total_cells entries, 16-byte
 *   aligned.  mask: DEVICE uint8 [total_cells], 4-byte aligned.  grid_counts: DEVICE int64 [n_grids][BGNN_VT_COUNTS], 8-byte aligned,
 *   cleared and written by the call.  stats: the block above.  No output may overlap a record array (not checked beyond equality).
 *   total_cells == 0 (then n_grids == 0) launches nothing and writes nothing, `stats` included; every other pointer may be NULL.
 *   BGNN_ERR_INVALID: a NULL pointer, a negative count, a row outside the contract above, a workspace that is too small or
 *   misaligned, a misaligned array. */
int bgnn_vr_ground_truth(bgnn_ctx *ctx, const float *noisy, int64_t n_noisy, const float *clean, int64_t n_clean,
                         const bgnn_vr_pair *pairs, int64_t n_grids, int64_t total_cells, double nodata, double noise_threshold,
                         void *ws, size_t ws_bytes, int32_t *labels, float *difference, float *noisy_depth, float *uncertainty,
                         uint8_t *mask, int64_t *grid_counts, void *stats);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_VRTRUTH_H */
