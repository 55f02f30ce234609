/*
 * bgnn_tilestore.h -- C ABI of libbgnn_hip.so, training tiles cut from planes that lie in HBM (ABI 7, additive; no entry point of
 * bgnn.h or of the other side headers changes): the reference's GroundTruthDataset._scan_ground_truth (training/trainer.py:133-171)
 * and TileManager.iterate_tiles(skip_empty=True) (data/tiling.py), without the plane leaving the device.
 *   scan   for every candidate box of an [rows][cols] plane, how many of its cells are valid and how many carry class 0 / 1 / 2
 *   cut    the boxes that were kept, gathered from up to four planes of one shape into flat tile stores, with the validity mask
 * Which boxes are candidates, and which are kept, is decided by the caller between the two calls, from the counts: the only thing
 * that comes to the host is the count table, 32 bytes per box.
 *
 * A box is a rectangle of the plane and the place of its tile in a flat store:
 *     rows row0 .. row0 + h - 1, columns col0 .. col0 + w - 1;  the tile is written row-major, h x w cells, from cell `dst` on.
 * Boxes are a HOST array.  Every box is checked before anything is launched (h > 0, w > 0, row0 >= 0, col0 >= 0,
 * row0 + h <= rows, col0 + w <= cols, dst >= 0; for the cut also dst + h * w <= dst_cells); then the table travels through the
 * context's pinned staging into the caller's workspace: the caller's copy may go away when the call returns.  Boxes may overlap in
 * the plane (a cell is read once per box that holds it, never more); the tiles of a cut must not overlap in the store (not checked:
 * the caller lays them out back to back).
 *
 * Workspace.  Both calls take DEVICE scratch of at least bgnn_tile_workspace_bytes(n_boxes) bytes, 16-byte aligned, from the
 * caller: the box table.  The library keeps no slot for it.  A scan and a cut queued behind each other may share one workspace (the
 * stream orders them).
 *
 * Validity.  Two predicates, for the scan's first count and for the cut's mask:
 *   BGNN_TILE_VALID_LABEL   an int32 plane: cell >= 0 (the ground-truth label band: -1 is "no data")
 *   BGNN_TILE_VALID_DEPTH   a float32 plane: cell finite and != (float)nodata.  A NaN nodata compares unequal to everything: finite
 *                           only (BathymetricGrid.valid_mask with nodata_value None or NaN)
 *
 * The conventions of bgnn.h hold (DEVICE / HOST pointers, return codes, bgnn_last_error(), the context's stream, asynchronous): no
 * entry point synchronises with the host, allocates, or copies to the host.  Every argument check runs before the context or the
 * device is touched.  The Python mirror binds these in bathymetric_gnn_amd/runtime.py (_TILESTORE_SIGNATURES);
 * training/trainer.py (TileStore.from_ground_truths, TileStore.from_survey) drives them.
 *
 * Geometry.  The grid comes from the boxes, not from the plane: a workgroup takes a band of BGNN_TILE_BAND_ROWS rows of one box, so
 * a plane with a few large boxes still fills the machine.  Inside a band a wave walks a row with one 4-byte cell per lane: the
 * source rows start at arbitrary columns, and nothing assumes more than the 4-byte alignment of the planes.  Every cell address is
 * 64-bit: rows * cols may exceed 2^31.
 *
 * Determinism.  The counts are integer sums: per thread, then a fixed tree per workgroup, then one 64-bit integer atomic add per
 * count and workgroup.  There is no float arithmetic beyond the two comparisons of the depth predicate; the cut moves 32-bit words,
 * so NaNs keep their payload.  Equal inputs give equal bits.
 */
#ifndef BGNN_TILESTORE_H
#define BGNN_TILESTORE_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_TILE_VALID_LABEL 0
#define BGNN_TILE_VALID_DEPTH 1
#define BGNN_TILE_MAX_PLANES 4      /* planes of one cut */
#define BGNN_TILE_BAND_ROWS 32      /* rows of a box behind one workgroup */
#define BGNN_TILE_BOX_BYTES 32      /* sizeof(bgnn_tile_box) */
#define BGNN_TILE_COUNTS 4          /* int64 counts per box: valid, class 0, class 1, class 2 */

typedef struct bgnn_tile_box {
  int64_t row0, col0;   /* the rectangle's first row and column in the plane */
  int32_t h, w;         /* its extent */
  int64_t dst;          /* cell offset of the tile in the flat store (bgnn_tile_cut; bgnn_tile_scan only checks dst >= 0) */
} bgnn_tile_box;

/* bgnn_tile_workspace_bytes: BGNN_TILE_BOX_BYTES * n_boxes rounded up to 256; 0 for n_boxes outside [0, 2^31 - 1].  Either call
 * answers more than 2^31 - 1 boxes with BGNN_ERR_UNSUPPORTED: split the table. */
size_t bgnn_tile_workspace_bytes(int64_t n_boxes);

/* bgnn_tile_scan: plane: DEVICE, [rows][cols], int32 (BGNN_TILE_VALID_LABEL) or float32 (BGNN_TILE_VALID_DEPTH), 4-byte aligned.
 *   counts: DEVICE int64 [n_boxes][BGNN_TILE_COUNTS], 8-byte aligned, cleared and written by the call:
 *     label mode   cells >= 0 | cells == 0 | cells == 1 | cells == 2  (other non-negative values are valid and of no class)
 *     depth mode   cells finite and != (float)nodata | 0 | 0 | 0      (`nodata` is not read in label mode)
 *   n_boxes == 0 launches nothing and writes nothing (boxes, ws and counts may then be NULL).
 *   BGNN_ERR_INVALID: a NULL pointer, rows < 1 or cols < 1, n_boxes < 0, an unknown mode, a box outside the contract above, a
 *   workspace that is too small or not 16-byte aligned, a plane that is not 4-byte or a count table that is not 8-byte aligned. */
int bgnn_tile_scan(bgnn_ctx *ctx, const void *plane, int64_t rows, int64_t cols, int32_t mode, double nodata,
                   const bgnn_tile_box *boxes, int64_t n_boxes, void *ws, size_t ws_bytes, int64_t *counts);

/* bgnn_tile_cut: one launch.  planes, dst: HOST arrays of n_planes DEVICE pointers, 1 <= n_planes <= BGNN_TILE_MAX_PLANES.
 *   planes[i]: [rows][cols] of 4-byte elements (int32 or float32: the words are moved, not interpreted); dst[i]: a flat store of
 *   dst_cells such elements.  Entry i with planes[i] == NULL and dst[i] == NULL is skipped (an absent uncertainty plane); one of the
 *   two alone is refused, and so are more than BGNN_TILE_MAX_PLANES planes: cut those in a second call.
 *   mask: DEVICE uint8 [dst_cells] or NULL.  Given, it receives 1 where the cell of planes[mask_plane] is valid under `mode` and 0
 *   elsewhere, at the same offsets as the tiles (planes[mask_plane] must then be given; with mask == NULL, mask_plane, mode and
 *   nodata are not read).
 *   No destination (mask included) may overlap a source plane.
 *   n_boxes == 0 launches nothing and writes nothing (boxes and ws may then be NULL).
 *   BGNN_ERR_INVALID: a NULL ctx / planes / dst / boxes / ws, n_planes outside 1 .. BGNN_TILE_MAX_PLANES, no plane given at all, a
 *   half-given entry, rows < 1 or cols < 1, n_boxes < 0, dst_cells < 0, a mask with an unknown mode or a mask_plane that names no
 *   given plane, a box outside the contract or past dst_cells, a destination that overlaps a source, a workspace that is too small
 *   or not 16-byte aligned, a plane or store that is not 4-byte aligned. */
int bgnn_tile_cut(bgnn_ctx *ctx, const void *const *planes, void *const *dst, int32_t n_planes, int64_t rows, int64_t cols,
                  uint8_t *mask, int32_t mask_plane, int32_t mode, double nodata, const bgnn_tile_box *boxes, int64_t n_boxes,
                  int64_t dst_cells, void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_TILESTORE_H */
