/*
 * bgnn_aux.h -- C ABI of libbgnn_hip.so, auxiliary node-feature planes (ABI 7, additive; no entry point of bgnn.h or of the other
 * side headers changes).  The graph build of bgnn.h computes its node features from depth (and takes uncertainty as one plane); a
 * model may want more per-cell inputs that are measured, not derived -- the sounding density of a gridded point cloud is the first.
 * These entry points take up to BGNN_AUX_MAX_PLANES such planes and append them, as they are, as node-feature columns.
 *
 * The column rule.  F0 is the column count of the plain build: the requested node features (uncertainty skipped when the batch has
 * none), then uncertainty appended when given and not listed.  Plane i becomes column F0 + i; the graph then has F = F0 + n_aux
 * columns (bgnn_graph_counts reports it, bgnn_graph_export writes x[N][F]).  Everything else the build fills -- the first F0 columns,
 * the stencil, the edge attributes, local_std -- is what bgnn_graph_build fills, bit for bit.
 *
 * The wide table.  With n_aux >= 1 the graph owns a second node table of BGNN_AUX_ROW_FLOATS columns (64-byte rows): the F0 words of
 * the 8-column table, the plane values of the node's cell, zeros.  One lane moves one 16-byte quarter of a row; words are moved as
 * uint32 and never interpreted, so a NaN payload survives.  A model with in_channels > 8 reads that table with a [16][hidden] first
 * extractor weight; its extractor keeps a launch of its own (the forms that fuse it into the next GEMM read 8-column rows).  A graph
 * of 8 columns or fewer built WITHOUT planes has no wide table and runs exactly the launches it ran before.
 *
 * The conventions of bgnn.h hold (DEVICE / HOST pointers, return codes, bgnn_last_error(), the context's stream, asynchronous).
 * Every check of n_aux, of the planes and of F0 + n_aux runs before the context or the device is touched.  The Python mirror binds
 * these in bathymetric_gnn_amd/runtime.py (_AUX_SIGNATURES); data/graph_construction.py (GraphBuilder.build_graph(density=...),
 * build_from_device(aux_t=...)) and models/pipeline.py (TileBatchEngine.infer_device(density_t=...)) drive them.
 */
#ifndef BGNN_AUX_H
#define BGNN_AUX_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_AUX_MAX_PLANES 8       /* planes of one build */
#define BGNN_AUX_ROW_FLOATS 16      /* columns of the wide node table: F0 + n_aux may not exceed it */

/* bgnn_graph_build_aux: bgnn_graph_build, then aux[0 .. n_aux - 1] appended as node-feature columns F0 .. F0 + n_aux - 1.
 *   aux: HOST array of n_aux DEVICE float planes, each laid out like tiles->depth (tiles concatenated, row-major); only the cells
 *   the mask marks valid are read.  0 <= n_aux <= BGNN_AUX_MAX_PLANES; with n_aux == 0 aux is not read and the call IS
 *   bgnn_graph_build.
 *   BGNN_ERR_INVALID: a NULL ctx / tiles / opts / out, n_aux out of range, aux NULL with n_aux >= 1, a NULL plane, and whatever
 *   bgnn_graph_build refuses.  BGNN_ERR_UNSUPPORTED: F0 + n_aux > BGNN_AUX_ROW_FLOATS. */
int bgnn_graph_build_aux(bgnn_ctx *ctx, const bgnn_tiles *tiles, const bgnn_graph_opts *opts, int32_t n_aux,
                         const float *const *aux, bgnn_graph **out);

/* bgnn_infer_tiles_aux: bgnn_infer_tiles with the planes handed to its graph build (same internal path, same result grids).  The
 *   model's in_channels must equal F0 + n_aux.  Refusals as above, then those of bgnn_infer_tiles. */
int bgnn_infer_tiles_aux(bgnn_ctx *ctx, bgnn_model *model, const bgnn_tiles *tiles, const bgnn_graph_opts *opts, int32_t n_aux,
                         const float *const *aux, float thr_auto, float thr_review, float norm_floor, float *classification,
                         float *confidence, float *correction, int64_t *n_nodes_out);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_AUX_H */
