/*
 * bgnn_soundings_vr.h -- C ABI of libbgnn_hip.so, gridding a point cloud of soundings at variable resolution (ABI 7, additive; no
 * entry point of bgnn.h or of the other side headers changes): soundings are filed straight into the refinement records of a VR
 * layout -- a base grid whose cells each carry a refinement grid of their own dimensions, the BAG's varres_metadata /
 * varres_refinements -- where bgnn_soundings.h and bgnn_soundings_robust.h file onto one uniform raster.  The layout is planned
 * from the cloud's own density (bgnn_vr_soundings_density, bgnn_vr_soundings_plan) or taken from an existing BAG.
 *
 * A layout of `total` records is a 1 x total grid to the two finalize entry points, which are per-cell functions of a flat state:
 *     bgnn_soundings_finalize(state, 1, total, ...)               the planes of a state filled by bgnn_vr_soundings_add
 *     bgnn_soundings_robust_finalize(stage, ..., 1, total, ...)   the planes of a stage filled by bgnn_vr_soundings_stage
 * bgnn_soundings_state_bytes(1, total), bgnn_soundings_reset, bgnn_soundings_robust_stage_bytes, _workspace_bytes and _reset
 * serve as they are.  Quantisation, sums, extremes and planes are those of the two headers; only the address differs.
 *
 * The conventions of bgnn_eval.h hold (DEVICE pointers owned by the caller, return codes, bgnn_last_error(), the context's stream,
 * asynchronous): no entry point synchronises with the host, allocates, or copies to the host; refusals happen before any launch.
 * The Python mirror binds these in bathymetric_gnn_amd/runtime.py (_VR_SOUNDINGS_SIGNATURES); data/sounding_vr.py drives them.
 *
 * The base grid.  base_height x base_width cells of `base_res` metres, (x0, y0) the SOUTH-WEST corner; base row 0 is the southmost
 * row and refinement row 0 the southmost row of its grid: the BAG's order, the opposite of bgnn_soundings.h's north-up origin.  In
 * float64, with true divisions, operation by operation (csrc/sounding_vr_cell.h):
 *     u = (x - x0) / base_res      v = (y - y0) / base_res      bc = floor(u)      br = floor(v)
 * The sounding is on the base grid iff 0 <= bc < base_width and 0 <= br < base_height (compared as float64); b = br * base_width + bc.
 *
 * The layout table.  One BGNN_VR_ENTRY_BYTES entry per base cell, row-major from the south-west: int64 index, int32 dx, int32 dy.
 * dx == 0 or dy == 0: the cell is not refined.  Dimensions run 1 .. BGNN_VR_MAX_DIM and may differ in x and y.
 *
 * The record of a sounding in a refined cell:
 *     fu = u - bc      fv = v - br                  (both exact)
 *     sc = floor(fu * dx)      sr = floor(fv * dy)
 *     record = index + sr * dx + sc
 * No clamp: fu <= 1 - 2^-53, and round-to-nearest gives fl(fu * d) < d for every d in range.
 *
 * Which counter a sounding enters, checked in this order, exactly one each:
 *     nonfinite      x, y or z is NaN or +-inf
 *     outside        off the base grid
 *     unrefined      on the base grid, in a cell without a refinement grid
 *     out_of_range   |z| >= 32768
 *     accepted       otherwise
 * accepted, nonfinite, outside, out_of_range go where bgnn_soundings.h puts them, the front of the state or stage; unrefined goes
 * into a caller-owned DEVICE int64 beside it.  An entry whose records do not lie inside 0 .. total - 1 (a table that belongs to
 * another state) is treated as not refined: nothing is ever written outside the state.
 *
 * The planner's rule, all in integers.  A ladder d_1 < d_2 < ... of dimensions, target_count >= 1, min_base_count >= 1.  n: the
 * soundings of the base cell that pass every check above but `unrefined`.  d = max{d_i : n >= target_count * d_i * d_i} (64-bit),
 * 0 when n < min_base_count or no rung fits; dx = dy = d.  index is the exclusive sum of d * d over the base cells in row-major
 * order (also in the cells that are not refined), so the grids tile the records back to back; total is the sum.
 */
#ifndef BGNN_SOUNDINGS_VR_H
#define BGNN_SOUNDINGS_VR_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_VR_ENTRY_BYTES 16                /* int64 index | int32 dx, dy */
#define BGNN_VR_MAX_DIM 32768                 /* the largest dimension of a refinement grid, each way */
#define BGNN_VR_MAX_RUNGS 16                  /* the longest ladder */
#define BGNN_VR_MAX_BASE_CELLS 2147483647     /* base_height * base_width */
#define BGNN_VR_MAX_RECORDS 2147483647        /* total: a record fits the int32 of the robust stage */
#define BGNN_VR_MAX_TARGET 2147483647         /* target_count and min_base_count */
#define BGNN_VR_PLAN_TILE 256                 /* base cells per workgroup of the planner's scan */

/* bgnn_vr_soundings_plan_workspace_bytes: what plan needs beside its outputs (8 bytes per BGNN_VR_PLAN_TILE base cells, rounded
 *   up to 256); 0 for a base grid outside the limits.
 * bgnn_vr_soundings_density: x, y (DEVICE float64), z (DEVICE float32), n entries each, into counts (DEVICE uint32, base_height *
 *   base_width, zeroed by the caller before the first call): one integer atomic per sounding that is finite, on the base grid and
 *   in range.  Accumulates over calls; at most 2^32 - 1 soundings per base cell.  n == 0 launches nothing.
 * bgnn_vr_soundings_plan: counts and the ladder (HOST int32, n_rungs entries, strictly ascending, 1 .. BGNN_VR_MAX_DIM) into the
 *   table (DEVICE, BGNN_VR_ENTRY_BYTES per base cell) and *total (DEVICE int64).  The scan runs on the device in three launches;
 *   nothing is read back.  total may exceed BGNN_VR_MAX_RECORDS: the caller reads it and refuses.
 * bgnn_vr_soundings_add: files the soundings into a state of bgnn_soundings_state_bytes(1, total) bytes under the record address.
 *   offered: as in bgnn_soundings_add.  unrefined: DEVICE int64, 8-byte aligned, added to.
 * bgnn_vr_soundings_stage: the same address into slots offered .. offered + n - 1 of a robust stage of `capacity` slots, (record,
 *   q), record = -1 where the sounding is not accepted: the positional slots of bgnn_soundings_robust_add.
 * bgnn_vr_soundings_flag: the stateless pass of bgnn_soundings_robust_flag under the record address: flags[i] is
 *   BGNN_ROBUST_FLAG_KEPT (0), _REJECTED (1) or _NOT_ACCEPTED (2: nonfinite, outside, unrefined or out of range) under the rule
 *   (center2, limit; DEVICE int64, total entries each) of the sounding's record.
 * BGNN_ERR_INVALID, before any launch: a NULL argument (x, y, z, flags may be NULL when n == 0), n < 0, base_res not a finite
 *   number above 0, x0 or y0 not finite, base_height or base_width outside 1 .. 2^31 - 1, total outside 1 .. BGNN_VR_MAX_RECORDS,
 *   offered < 0 or offered + n above BGNN_SOUNDINGS_MAX_TOTAL (add) or above capacity (stage), capacity outside 1 ..
 *   BGNN_ROBUST_MAX_CAPACITY, a ladder that is empty, longer than BGNN_VR_MAX_RUNGS, not strictly ascending or outside 1 ..
 *   BGNN_VR_MAX_DIM, target_count or min_base_count outside 1 .. BGNN_VR_MAX_TARGET, a workspace that is too small, a table,
 *   state, stage, workspace, total, unrefined, center2 or limit that is not 8-byte aligned, counts not 4-byte aligned.
 *   BGNN_ERR_UNSUPPORTED: base_height * base_width above BGNN_VR_MAX_BASE_CELLS. */
size_t bgnn_vr_soundings_plan_workspace_bytes(int64_t base_height, int64_t base_width);
int bgnn_vr_soundings_density(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0, double y0,
                              double base_res, int64_t base_height, int64_t base_width, uint32_t *counts);
int bgnn_vr_soundings_plan(bgnn_ctx *ctx, const uint32_t *counts, int64_t base_height, int64_t base_width, const int32_t *ladder,
                           int32_t n_rungs, int64_t target_count, int64_t min_base_count, void *workspace, size_t workspace_bytes,
                           void *table, int64_t *total);
int bgnn_vr_soundings_add(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0, double y0,
                          double base_res, int64_t base_height, int64_t base_width, const void *table, int64_t total, int64_t offered,
                          void *state, int64_t *unrefined);
int bgnn_vr_soundings_stage(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0, double y0,
                            double base_res, int64_t base_height, int64_t base_width, const void *table, int64_t total,
                            int64_t offered, int64_t capacity, void *stage, int64_t *unrefined);
int bgnn_vr_soundings_flag(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0, double y0,
                           double base_res, int64_t base_height, int64_t base_width, const void *table, int64_t total,
                           const int64_t *center2, const int64_t *limit, uint8_t *flags);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_SOUNDINGS_VR_H */
