/*
 * bgnn_sidecar.h -- C ABI of libbgnn_hip.so, VR BAG sidecar raster (ABI 7, additive).
 *
 * The conventions of bgnn.h hold (DEVICE / HOST pointers, return codes, bgnn_last_error(), the context's stream).  This header
 * adds the rasteriser behind data/vr_bag.py's SidecarBuilder (reference data/vr_bag.py:695-778, add_refinement_results): the
 * classification / confidence / correction planes and the valid mask of every refinement grid painted onto one georeferenced
 * raster [height, width], each refinement cell as a scale x scale block of pixels, refinement row 0 at the south.  The Python
 * mirror binds the entry points in bathymetric_gnn_amd/runtime.py (_SIDECAR_SIGNATURES).
 *
 * Semantics (those of the reference's loop over grids in iteration order):
 *   - where two grids cover a pixel the three value planes hold the LATER grid's values (later = higher index in the table),
 *     whatever the order, stream or context the bgnn_sidecar_add calls were issued in;
 *   - the valid mask is sticky: 1.0 where ANY covering cell of any applied grid was valid;
 *   - values are copied bit for bit (NaN payloads, -0.0); pixels never covered are NaN (0x7fc00000) / 0.0;
 *   - pixels outside the raster are dropped one by one; grids whose keep flag is 0 are not applied.
 * No float atomics: the result does not depend on arrival order, two runs give identical bits.
 *
 * Buffers, all DEVICE and caller-owned:
 *   images  uint64 [3, height, width], ZERO-FILLED by the caller before the first add (0 = never written).  A covering cell of
 *           table grid g leaves max(old, ((g + 1) << 32) | float bits) there (64-bit integer atomic max).  24 B per pixel.
 *   valid   float32 [height, width], zero-filled by the caller; add stores 1.0f (every writer stores the same value).
 *   planes  float32 [3, height, width], written by bgnn_sidecar_finish from the images' low words.
 * A raster may have at most BGNN_SIDECAR_MAX_PIXELS pixels (6 GiB of images); more -> BGNN_ERR_INVALID.
 */
#ifndef BGNN_SIDECAR_H
#define BGNN_SIDECAR_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_SIDECAR_MAX_PIXELS 268435456 /* 2^28 */

/* bgnn_sidecar_table_bytes: bytes of the DEVICE placement table for n_grids grids (0 when n_grids < 0).
 *
 * bgnn_sidecar_table: checks the per-grid placement and writes the table the kernels read.  HOST inputs: hw int32 [n_grids][2]
 *   (rows, cols of each grid, in iteration order), placement int64 [n_grids][3] = {out_row_start, out_col_start, scale}
 *   (SidecarBuilder.placement: the float64 arithmetic of the reference stays on the host; the device only sees integers).
 *   Each grid's footprint is clipped to the raster here, so that the kernels only ever visit pixels inside it.
 *   pixel_offsets (HOST int64 [n_grids + 1], may be NULL) receives the prefix sum of the clipped footprint sizes: a run of
 *   grids [first, first + n) has pixel_offsets[first + n] - pixel_offsets[first] pixels to paint.
 *   Refused with BGNN_ERR_INVALID: NULL tables, table_bytes != bgnn_sidecar_table_bytes(n_grids), a grid with rows or cols < 1,
 *   scale < 1, rows * scale or cols * scale >= 2^31, height * width outside 1 .. BGNN_SIDECAR_MAX_PIXELS.
 *   Synchronous (the table is complete on return and may be read from any stream).
 *
 * bgnn_sidecar_add: paints the run of grids [first_grid, first_grid + n_grids) of the table.  classification / confidence /
 *   correction (DEVICE float32 [n_cells]) and mask (DEVICE u8 [n_cells], as bgnn_vr_unpack left it) hold the run's cells back to
 *   back in table order (n_cells = their total); keep (DEVICE u8 [n_grids], may be NULL = all kept) are the run's keep flags
 *   from bgnn_vr_unpack; n_pixels the run's footprint (from pixel_offsets).  image_pixels is the pixel capacity of `images` and
 *   `valid` and must equal height * width.  One thread per footprint pixel, consecutive lanes on consecutive pixels of one
 *   raster row.  Asynchronous, on the context's stream; runs may be added in any order and concurrently from several contexts.
 *
 * bgnn_sidecar_finish: images -> planes (low word, NaN where the image is 0).  Call once every add has completed or is ordered
 *   before it on the context's stream.  Asynchronous. */
size_t bgnn_sidecar_table_bytes(int32_t n_grids);
int bgnn_sidecar_table(bgnn_ctx *ctx, int32_t height, int32_t width, int32_t n_grids, const int32_t *hw,
                       const int64_t *placement, void *table, size_t table_bytes, int64_t *pixel_offsets);
int bgnn_sidecar_add(bgnn_ctx *ctx, int32_t height, int32_t width, uint64_t *images, float *valid, int64_t image_pixels,
                     const void *table, int32_t table_grids, int32_t first_grid, int32_t n_grids, int64_t n_pixels,
                     const float *classification, const float *confidence, const float *correction, const uint8_t *mask,
                     int64_t n_cells, const uint8_t *keep);
int bgnn_sidecar_finish(bgnn_ctx *ctx, int32_t height, int32_t width, const uint64_t *images, int64_t image_pixels,
                        float *planes);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_SIDECAR_H */
