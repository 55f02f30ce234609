/*
 * bgnn_soundings.h -- C ABI of libbgnn_hip.so, gridding a point cloud of soundings (ABI 7, additive; no entry point of bgnn.h or
 * of the other side headers changes): one pass over (x, y, z) files every sounding under the cell it falls into and keeps, per
 * cell, what the count, mean, standard deviation, minimum and maximum planes are formed from.  The reference stops in front of
 * this step (data/loaders.py, BathymetricLoader._load_xyz raises NotImplementedError) while its documents ask for what it gives
 * (docs/TRAINING_DASHBOARD.md "Next Steps" 5: the per-cell sounding count; docs/LESSONS_LEARNED.md section 6).
 *
 * The conventions of bgnn_eval.h hold (DEVICE pointers owned by the caller, return codes, bgnn_last_error(), the context's stream,
 * asynchronous): no entry point synchronises with the host, allocates, or copies to the host; refusals happen before any launch.
 * The Python mirror binds these in bathymetric_gnn_amd/runtime.py (_SOUNDINGS_SIGNATURES); data/sounding_grid.py drives them.
 *
 * The grid.  height x width cells of `res` metres, (x0, y0) the upper-left corner: the GDAL geotransform (x0, res, 0, y0, 0, -res).
 * In float64, with a true division (csrc/sounding_cell.h):
 *     col = floor((x - x0) / res)        row = floor((y0 - y) / res)        cell = row * width + col   (64-bit)
 * Cells are half-open: x == x0 + width * res is outside, y == y0 is row 0.
 *
 * Which counter a sounding enters, checked in this order, exactly one each:
 *     nonfinite      x, y or z is NaN or +-inf
 *     outside        col or row outside the grid
 *     out_of_range   |z| >= 32768
 *     accepted       otherwise
 *
 * What a cell keeps of its accepted soundings, q = llrint((double)z * 65536.0) (the product is exact, the rounding half to even,
 * |q| < 2^31):  n, S1 = sum q, S2 = sum q^2 (as the sums of the low and of the high 32 bits of q^2) and the extremes of the raw z
 * under the order-preserving map of float32 onto uint32 (so -0.0 sorts below +0.0).  Every one is an integer and is added, or
 * maximised, with integer atomics: equal soundings give equal bits in any order, in any split over calls, on every run.  There are
 * no float atomics and no float sums.  Within BGNN_SOUNDINGS_MAX_TOTAL soundings offered to one state no entry overflows.
 *
 * The planes of bgnn_soundings_finalize, with valid = n >= min_count:
 *     count   int32    n, also where valid == 0
 *     mean    float32  (float)((double)S1 / (double)n * 2^-16)
 *     std     float32  (float)(sqrt((double)(n * S2 - S1 * S1) / ((double)n * (double)n)) * 2^-16): the population standard
 *                      deviation, 0 for n == 1; the numerator is an exact integer rounded once to float64
 *     min,max float32  the raw extremes, not quantised
 *     valid   uint8
 * Where valid == 0 the four float planes hold nodata_value.  A one-sounding cell's mean is the sounding rounded to 2^-16 m (at
 * most 2^-17 m = 7.6 um off); its min and max return it exactly.
 */
#ifndef BGNN_SOUNDINGS_H
#define BGNN_SOUNDINGS_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_SOUNDINGS_HEADER_BYTES 32        /* int64 accepted, nonfinite, outside, out_of_range: the front of the state */
#define BGNN_SOUNDINGS_CELL_BYTES 40          /* int64 S1 | uint64 S2 low words, S2 high words | uint32 n, ~min key, max key, pad */
#define BGNN_SOUNDINGS_MAX_TOTAL 2147483647   /* soundings offered to one state over all calls */
#define BGNN_SOUNDINGS_Z_CAP 32768            /* metres: |z| at or above this is counted as out_of_range */
#define BGNN_SOUNDINGS_SCALE 65536            /* fixed point of the sums: 2^-16 m */
#define BGNN_SOUNDINGS_EXTENT_BYTES 48        /* float64 min_x, max_x, min_y, max_y | int64 finite_x, finite_y */
#define BGNN_SOUNDINGS_EXTENT_MAX_GRID 1024   /* workgroups of the extent pass */
/* the extent buffer: the result in front, one partial of the same record per workgroup behind it */
#define BGNN_SOUNDINGS_EXTENT_BUFFER_BYTES (BGNN_SOUNDINGS_EXTENT_BYTES * (1 + BGNN_SOUNDINGS_EXTENT_MAX_GRID))

/* bgnn_soundings_state_bytes: BGNN_SOUNDINGS_HEADER_BYTES + BGNN_SOUNDINGS_CELL_BYTES * height * width; 0 for height < 1 or
 *   width < 1 or where that does not fit size_t.  The state is a DEVICE block, caller-owned, 8-byte aligned, opaque but for the
 *   four counters in front.
 * bgnn_soundings_reset: zeroes the state: an all-zero state is the empty one.
 * bgnn_soundings_add: files x, y (DEVICE float64) and z (DEVICE float32), n entries each, into the state.  A survey is added
 *   line file by line file: the state persists across calls, all with the same grid.  offered: the soundings offered to this
 *   state by the calls before this one (the caller's count; nothing is read back).  n == 0 launches nothing.
 *   BGNN_ERR_INVALID: NULL ctx / x / y / z / state (x, y, z may be NULL when n == 0), res not a finite number above 0, x0 or y0
 *   not finite, height or width outside 1 .. 2^31 - 1, n < 0, offered < 0, offered + n above BGNN_SOUNDINGS_MAX_TOTAL, a state
 *   that is not 8-byte aligned.
 * bgnn_soundings_finalize: the six planes (DEVICE, height * width entries each) from the state, which it only reads: more can be
 *   added afterwards.  BGNN_ERR_INVALID: NULL ctx / state / plane, height or width outside 1 .. 2^31 - 1, min_count < 1, a state
 *   that is not 8-byte aligned.
 * bgnn_soundings_extent: the float64 minimum and maximum of the finite x and of the finite y, and how many of each are finite,
 *   into the first BGNN_SOUNDINGS_EXTENT_BYTES of `extent` (DEVICE, 8-byte aligned, BGNN_SOUNDINGS_EXTENT_BUFFER_BYTES: the rest
 *   is workspace).  No finite value: min = +inf, max = -inf, count 0.  A fixed halving tree per workgroup, the partials finished
 *   by a second launch of one workgroup.  BGNN_ERR_INVALID: NULL ctx / extent, NULL x or y with n > 0, n < 0, a misaligned
 *   extent. */
size_t bgnn_soundings_state_bytes(int64_t height, int64_t width);
int bgnn_soundings_reset(bgnn_ctx *ctx, void *state, int64_t height, int64_t width);
int bgnn_soundings_add(bgnn_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, double x0, double y0, double res,
                       int64_t height, int64_t width, int64_t offered, void *state);
int bgnn_soundings_finalize(bgnn_ctx *ctx, const void *state, int64_t height, int64_t width, int32_t min_count, float nodata_value,
                            int32_t *count, float *mean, float *std, float *min, float *max, uint8_t *valid);
int bgnn_soundings_extent(bgnn_ctx *ctx, const double *x, const double *y, int64_t n, void *extent);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_SOUNDINGS_H */
