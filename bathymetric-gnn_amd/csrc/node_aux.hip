// Auxiliary node-feature planes (include/bgnn_aux.h): the wide node table of a graph built with planes, and the argument checks of
// the two entry points.  x16[row][c] = the word of x8[row][c] for c < F0, planes[c - F0][cell_of_node[row]] for F0 <= c < F0 + n_aux,
// zero beyond.  Words are moved as uint32 and never interpreted.
#include "bgnn_internal.h"

namespace bgnn {

struct NodeAuxArgs {
  const uint4 *x8;              // [rows][2] quarters of the 8-column table
  const int32_t *cell_of_node;  // [rows]
  const int64_t *counts;        // [0] = rows in use
  uint4 *x16;                   // [rows][4] quarters of the wide table
  const uint32_t *planes[BGNN_AUX_MAX_PLANES];
  int32_t F0, F;                // columns of the plain build, columns in all
};

// One lane, one 16-byte quarter of a row: four consecutive lanes store one 64-byte row, a wave 16 consecutive rows.
__global__ __launch_bounds__(256) void node_aux_kernel(NodeAuxArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = i >> 2;
  if (row >= a.counts[0]) return;
  const int q = (int)(i & 3);
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (q * 4 < a.F0) v = a.x8[row * 2 + q];                 // (F0 <= 8: only quarters 0 and 1 hold words of x8)
  if (q * 4 + 4 > a.F0 && q * 4 < a.F) {                   // the quarter holds plane columns (and pad columns of either table)
    const int64_t cell = a.cell_of_node[row];
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = q * 4 + k;
      if (c < a.F0) continue;
      uint32_t word = 0u;
#pragma unroll
      for (int j = 0; j < BGNN_AUX_MAX_PLANES; ++j)          // (compile-time index: the pointers stay in the argument segment)
        if (c - a.F0 == j && c < a.F) word = a.planes[j][cell];
      w[k] = word;
    }
    v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  a.x16[i] = v;
}

int launch_node_aux(bgnn_ctx *ctx, bgnn_graph *g, int F0, int n_aux, const float *const *aux) {
  BGNN_REQUIRE(g->d_x8 && g->d_x16 && F0 >= 1 && F0 <= 8 && n_aux >= 1 && n_aux <= BGNN_AUX_MAX_PLANES && F0 + n_aux <= BGNN_AUX_ROW_FLOATS,
               "node_aux: F0=%d n_aux=%d (internal)", F0, n_aux);
  const int64_t rows = g->row_capacity;
  if (rows <= 0) return BGNN_OK;
  NodeAuxArgs a{};
  a.x8 = reinterpret_cast<const uint4 *>(g->d_x8); a.cell_of_node = g->d_cell_of_node; a.counts = g->d_counts;
  a.x16 = reinterpret_cast<uint4 *>(g->d_x16);
  for (int j = 0; j < n_aux; ++j) a.planes[j] = reinterpret_cast<const uint32_t *>(aux[j]);
  a.F0 = F0; a.F = F0 + n_aux;
  ProfScope ps(ctx, BGNN_K_FEATURES);
  hipLaunchKernelGGL(node_aux_kernel, dim3((unsigned)((rows * 4 + 255) / 256)), dim3(256), 0, ctx->stream, a);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

int aux_planes_check(const char *who, const bgnn_tiles *tiles, const bgnn_graph_opts *opts, int32_t n_aux, const float *const *aux) {
  BGNN_REQUIRE(n_aux >= 0 && n_aux <= BGNN_AUX_MAX_PLANES, "%s: n_aux=%d out of range (0..%d)", who, n_aux, BGNN_AUX_MAX_PLANES);
  if (n_aux == 0) return BGNN_OK;
  BGNN_REQUIRE(aux, "%s: aux is NULL with n_aux=%d", who, n_aux);
  for (int j = 0; j < n_aux; ++j) BGNN_REQUIRE(aux[j], "%s: plane %d is NULL", who, j);
  BGNN_REQUIRE(opts->n_node_features >= 0 && opts->n_node_features <= 8, "n_node_features=%d out of range", opts->n_node_features);
  const int F0 = node_feature_columns(tiles, opts, nullptr);
  if (F0 + n_aux > BGNN_AUX_ROW_FLOATS) {
    set_error("%s: %d node-feature columns and %d planes exceed the %d columns of the wide node table", who, F0, n_aux,
              BGNN_AUX_ROW_FLOATS);
    return BGNN_ERR_UNSUPPORTED;
  }
  return BGNN_OK;
}

}  // namespace bgnn

using namespace bgnn;

extern "C" {

int bgnn_graph_build_aux(bgnn_ctx *ctx, const bgnn_tiles *tiles, const bgnn_graph_opts *opts, int32_t n_aux,
                         const float *const *aux, bgnn_graph **out) {
  BGNN_REQUIRE(ctx && tiles && opts && out, "bgnn_graph_build_aux: NULL argument");
  BGNN_TRY(aux_planes_check("bgnn_graph_build_aux", tiles, opts, n_aux, aux));
  return graph_build(ctx, tiles, opts, out, nullptr, nullptr, n_aux, aux);
}

int bgnn_infer_tiles_aux(bgnn_ctx *ctx, bgnn_model *model, const bgnn_tiles *tiles, const bgnn_graph_opts *opts, int32_t n_aux,
                         const float *const *aux, float thr_auto, float thr_review, float norm_floor, float *classification,
                         float *confidence, float *correction, int64_t *n_nodes_out) {
  BGNN_REQUIRE(ctx && model && tiles && opts, "bgnn_infer_tiles_aux: NULL argument");
  BGNN_TRY(aux_planes_check("bgnn_infer_tiles_aux", tiles, opts, n_aux, aux));
  return infer_tiles(ctx, model, tiles, opts, n_aux, aux, thr_auto, thr_review, norm_floor, classification, confidence, correction,
                     n_nodes_out);
}

}  // extern "C"
