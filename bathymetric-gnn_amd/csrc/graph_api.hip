// C ABI of libbgnn_hip.so, graph handles (declared in include/bgnn.h): building a tile batch's graph from its plan (graph_plan.h),
// foreign graphs from an edge list, counts, export, scatter, and what a handle owns.  Host code only; the kernels are in graph_build.hip.
#include "bgnn_internal.h"

namespace bgnn {

// ---- the context's table cache (bgnn_ctx::TableCache): the two tables of uniform batches at one resolution --------------------
// A hit, or a new entry -- at 8 entries the least recently used one NO LIVE GRAPH points into makes room (nothing in flight reads it
// after a stream sync).  *fresh: the tables are new and have to be uploaded.  Every entry pinned, or no memory for a new one: g is
// left as it is and keeps private tables.
static void table_cache_acquire(bgnn_ctx *ctx, bgnn_graph *g, const GraphPlan &p, bool *fresh) {
  auto &cache = ctx->table_cache;
  *fresh = false;
  bgnn_ctx::TableCache *e = nullptr;
  for (auto &c : cache)
    if (c.n_tiles == g->n_tiles && c.h == p.uni_h && c.w == p.uni_w && c.item_cells == p.item_cells && c.rx == p.rx && c.ry == p.ry) { e = &c; break; }
  if (e) {
    ++e->refs;
  } else {
    if (cache.size() >= 8) {
      size_t lru = cache.size();
      for (size_t i = 0; i < cache.size(); ++i)
        if (cache[i].refs == 0 && (lru == cache.size() || cache[i].stamp < cache[lru].stamp)) lru = i;
      if (lru == cache.size()) return;
      (void)hipStreamSynchronize(ctx->stream);
      (void)hipFree(cache[lru].d_tiles); (void)hipFree(cache[lru].d_items);
      cache.erase(cache.begin() + lru);
    }
    bgnn_ctx::TableCache n{g->n_tiles, p.uni_h, p.uni_w, p.item_cells, p.rx, p.ry, nullptr, nullptr, g->n_items, 0, ctx->table_next_id++, 1};
    if (hipMalloc((void **)&n.d_tiles, sizeof(BgnnTileMeta) * g->n_tiles) != hipSuccess ||
        hipMalloc((void **)&n.d_items, sizeof(BgnnWorkItem) * g->n_items) != hipSuccess) {
      (void)hipGetLastError();
      if (n.d_tiles) (void)hipFree(n.d_tiles);
      return;
    }
    cache.push_back(n);
    e = &cache.back();
    *fresh = true;
  }
  e->stamp = ++ctx->table_stamp;
  g->d_tiles = e->d_tiles; g->d_items = e->d_items; g->tables_cached = true; g->table_cache_id = e->id;
}

// drops g's reference on its cache entry (evictable at 0)
static void table_cache_release(bgnn_graph *g) {
  if (!g->tables_cached) return;
  for (auto &e : g->ctx->table_cache)
    if (e.id == g->table_cache_id) { if (e.refs > 0) --e.refs; break; }
}

// A handle owns the pool blocks it recorded (graph_alloc) and one reference on a table-cache entry.
void graph_free(bgnn_graph *g) {
  g->ctx->live_graphs.erase(g);
  table_cache_release(g);
  for (void *p : g->blocks) g->ctx->pool.release(p);
  delete g;
}

static int validate_opts(const bgnn_graph_opts *o) {
  BGNN_REQUIRE(o->connectivity == 4 || o->connectivity == 8 || o->connectivity == 16,
               "Unknown connectivity: %d", o->connectivity);
  BGNN_REQUIRE(o->n_node_features >= 0 && o->n_node_features <= 8, "n_node_features=%d out of range", o->n_node_features);
  BGNN_REQUIRE(o->n_edge_features >= 1 && o->n_edge_features <= 4, "n_edge_features=%d out of range (1..4)", o->n_edge_features);
  for (int i = 0; i < o->n_node_features; ++i)
    BGNN_REQUIRE(o->node_features[i] >= 0 && o->node_features[i] <= 7, "bad node feature id %d", o->node_features[i]);
  for (int i = 0; i < o->n_edge_features; ++i)
    BGNN_REQUIRE(o->edge_features[i] >= 0 && o->edge_features[i] <= 3, "bad edge feature id %d", o->edge_features[i]);
  return BGNN_OK;
}

// the device side of a planned batch: tables, buffers, uploads, kernels (on failure the caller frees g with what it holds by then)
static int graph_fill(bgnn_ctx *ctx, bgnn_graph *g, const GraphPlan &p, const bgnn_tiles *tiles, const bgnn_graph_opts *opts,
                      int32_t n_aux, const float *const *aux) {
  const int64_t cells = p.cells;
  bool upload_tables = false;
  char *blk = nullptr;                                     // ragged batch: ONE block with every host-built table
  if (!p.uniform) {
    BGNN_TRY(graph_alloc(g, blk, p.block.size()));
    g->d_tiles = (BgnnTileMeta *)(blk + p.o_tiles); g->d_items = (BgnnWorkItem *)(blk + p.o_items);
    g->d_items2 = (BgnnWorkItem *)(blk + p.o_items2);
    if (p.atlas_h) { g->d_atlas_tile = (BgnnTileMeta *)(blk + p.o_atile); g->d_atlas_pos = (int32_t *)(blk + p.o_apos); }
    else g->d_items3 = (BgnnWorkItem *)(blk + p.o_items3);
  } else {
    if (p.cacheable) table_cache_acquire(ctx, g, p, &upload_tables);
    if (!g->tables_cached) {
      BGNN_TRY(graph_alloc(g, g->d_tiles, g->n_tiles));
      BGNN_TRY(graph_alloc(g, g->d_items, g->n_items));
      upload_tables = true;
    }
  }
  BGNN_TRY(graph_alloc(g, g->d_node_id, cells));
  BGNN_TRY(graph_alloc(g, g->d_cell_of_node, cells));
  BGNN_TRY(graph_alloc(g, g->d_counts, 4));
  BGNN_TRY(graph_alloc(g, g->d_x8, cells * 8));
  g->d_x = g->d_x8; g->ldx = 8;
  BGNN_TRY(graph_alloc(g, g->d_local_std, cells));
  BGNN_TRY(graph_alloc(g, g->d_nbr, cells * g->K));
  // every edge feature list is a selection / ordering of (distance, depth_difference, slope, zero): all of them are built compact
  // (graph_build.hip, FeatureArgs) on a stencil the fused kernels know
  g->compact_edges = g->K == 4 || g->K == 8 || g->K == 16;
  for (int i = 0; i < 4; ++i) g->edge_ids[i] = i < g->ED ? opts->edge_features[i] : BGNN_EF_ZERO;
  g->edge_default = g->ED == 3 && opts->edge_features[0] == BGNN_EF_DISTANCE && opts->edge_features[1] == BGNN_EF_DEPTH_DIFFERENCE &&
                    opts->edge_features[2] == BGNN_EF_SLOPE;
  if (g->compact_edges) {
    BGNN_TRY(graph_alloc(g, g->d_slope, cells * g->K));
    BGNN_TRY(graph_alloc(g, g->d_node_depth, cells));
    BGNN_TRY(graph_alloc(g, g->d_tile_dist, g->n_tiles));
  } else {
    BGNN_TRY(graph_alloc(g, g->d_eattr, cells * g->K * g->ED));
  }
  if (p.atlas_h) BGNN_TRY(graph_alloc(g, g->d_atlas, (size_t)p.atlas_h * p.atlas_w));
  if (p.atlas_h && g->compact_edges) BGNN_TRY(graph_alloc(g, g->d_atlas_tile_of, (size_t)p.atlas_h * p.atlas_w));
  if (!p.uniform) BGNN_TRY(ctx_upload(ctx, p.block.data(), p.block.size(), blk));
  if (upload_tables) {
    BGNN_TRY(ctx_upload(ctx, g->h_tiles.data(), sizeof(BgnnTileMeta) * g->n_tiles, g->d_tiles));
    BGNN_TRY(ctx_upload(ctx, p.items.data(), sizeof(BgnnWorkItem) * p.items.size(), g->d_items));
  }
  BGNN_TRY(launch_graph_build(ctx, g, tiles, opts));
  if (n_aux > 0) {                                         // bgnn_aux.h: the wide node table, the planes behind the plain build's columns
    const int F0 = g->F;
    BGNN_TRY(graph_alloc(g, g->d_x16, cells * BGNN_AUX_ROW_FLOATS));
    BGNN_TRY(launch_node_aux(ctx, g, F0, n_aux, aux));
    g->d_x = g->d_x16; g->ldx = BGNN_AUX_ROW_FLOATS; g->F = F0 + n_aux;
  }
  return BGNN_OK;
}

int graph_build(bgnn_ctx *ctx, const bgnn_tiles *tiles, const bgnn_graph_opts *opts, bgnn_graph **out, int64_t *n_nodes_copy,
                float *const *clear_grids, int32_t n_aux, const float *const *aux) {
  BGNN_REQUIRE(ctx && tiles && opts && out, "bgnn_graph_build: NULL argument");
  BGNN_REQUIRE(tiles->n_tiles >= 1, "bgnn_graph_build: n_tiles=%d", tiles->n_tiles);
  // (the per-grid kernels index grids by gridDim.y: 65 535 at most -- say so instead of failing the launch)
  BGNN_REQUIRE(tiles->n_tiles <= 60000, "bgnn_graph_build: %d grids in one batch, at most 60000 (split the batch)", tiles->n_tiles);
  BGNN_REQUIRE(tiles->hw && tiles->resolution && tiles->depth && tiles->mask, "bgnn_graph_build: NULL tile array");
  BGNN_TRY(validate_opts(opts));
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const int nf = node_feature_columns(tiles, opts, nullptr);
  BGNN_REQUIRE(nf >= 1 && nf <= 8, "node feature count %d out of range (1..8)", nf);
  GraphPlan p = plan_graph(tiles->n_tiles, tiles->hw, tiles->resolution, opts->connectivity, ctx->num_cus, ctx->opts.ragged_atlas);
  if (p.error != BGNN_OK) { set_error("%s", p.message.c_str()); return p.error; }
  bgnn_graph *g = new bgnn_graph();
  g->ctx = ctx; g->kind = 0; g->n_tiles = tiles->n_tiles; g->d_n_nodes_copy = n_nodes_copy;
  if (clear_grids) for (int i = 0; i < 3; ++i) g->clear_grids[i] = clear_grids[i];
  g->K = opts->connectivity; g->ED = opts->n_edge_features; g->include_self_loops = opts->include_self_loops ? 1 : 0;
  g->has_unc = tiles->uncertainty ? 1 : 0;
  g->F = nf;
  g->h_tiles = std::move(p.h_tiles);
  g->total_cells = (int32_t)p.cells; g->row_capacity = (int32_t)p.cells; g->n_items = (int32_t)p.items.size();
  g->uni_h = p.uni_h; g->uni_w = p.uni_w; g->max_h = p.max_h; g->max_w = p.max_w;
  g->bh2 = p.bh2; g->bw2 = p.bw2; g->n_blocks2 = p.n_blocks2;
  g->bh3 = p.bh3; g->bw3 = p.bw3; g->n_blocks3 = p.n_blocks3;
  g->atlas_w = p.atlas_w; g->atlas_h = p.atlas_h;
  const int rc = graph_fill(ctx, g, p, tiles, opts, n_aux, aux);
  if (rc != BGNN_OK) { graph_free(g); return rc; }
  ctx->live_graphs.insert(g);
  *out = g;
  return BGNN_OK;
}

}  // namespace bgnn

using namespace bgnn;

extern "C" {

int bgnn_graph_build(bgnn_ctx *ctx, const bgnn_tiles *tiles, const bgnn_graph_opts *opts, bgnn_graph **out) {
  return graph_build(ctx, tiles, opts, out, nullptr, nullptr);
}

int bgnn_graph_from_edges(bgnn_ctx *ctx, int64_t n_nodes, int32_t n_feat, const float *x, int64_t n_edges,
                          const int64_t *edge_index, int32_t edge_dim, const float *edge_attr, bgnn_graph **out) {
  BGNN_REQUIRE(ctx && out, "bgnn_graph_from_edges: NULL argument");
  BGNN_REQUIRE(n_nodes >= 0 && n_nodes < ((int64_t)1 << 31) && n_edges >= 0 && n_edges < ((int64_t)1 << 31),
               "graph too large");
  BGNN_REQUIRE(n_feat >= 1 && n_feat <= 8, "n_feat=%d unsupported (1..8)", n_feat);
  BGNN_REQUIRE(edge_dim >= 1 && edge_dim <= 4, "edge_dim=%d unsupported (1..4)", edge_dim);
  BGNN_REQUIRE((x || n_nodes == 0) && (edge_index || n_edges == 0) && (edge_attr || n_edges == 0), "NULL tensor");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  bgnn_graph *g = new bgnn_graph();
  g->ctx = ctx; g->kind = 1; g->F = n_feat; g->ED = edge_dim; g->K = 0;
  g->total_cells = (int32_t)n_nodes; g->row_capacity = (int32_t)n_nodes; g->generic_E = n_edges;
  int rc = launch_generic_build(ctx, g, n_nodes, n_feat, x, n_edges, edge_index, edge_dim, edge_attr);
  if (rc != BGNN_OK) { graph_free(g); return rc; }
  ctx->live_graphs.insert(g);
  *out = g;
  return BGNN_OK;
}

int bgnn_graph_destroy(bgnn_graph *g) {
  if (!g) return BGNN_OK;
  graph_free(g);
  return BGNN_OK;
}

int bgnn_graph_counts(bgnn_graph *g, int64_t *n_nodes, int64_t *n_edges, int32_t *n_feat, int32_t *edge_dim,
                      int64_t *node_off, int64_t *edge_off) {
  BGNN_REQUIRE(g, "graph is NULL");
  bgnn_ctx *ctx = g->ctx;
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  if (n_feat) *n_feat = g->F;
  if (edge_dim) *edge_dim = g->ED;
  if (g->kind == 1) {
    if (n_nodes) *n_nodes = g->total_cells;
    if (n_edges) *n_edges = g->generic_E;
    if (node_off) { node_off[0] = 0; node_off[1] = g->total_cells; }
    if (edge_off) { edge_off[0] = 0; edge_off[1] = g->generic_E; }
    return BGNN_OK;
  }
  BGNN_TRY(launch_graph_count_edges(g));
  std::vector<int64_t> tc((size_t)g->n_tiles * 2);
  BGNN_HIP_CHECK(hipMemcpyAsync(tc.data(), ctx->ws[5], tc.size() * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  BGNN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  int64_t nn = 0, ne = 0;
  for (int t = 0; t < g->n_tiles; ++t) {
    if (node_off) node_off[t] = nn;
    if (edge_off) edge_off[t] = ne;
    nn += tc[t]; ne += tc[g->n_tiles + t];
  }
  if (node_off) node_off[g->n_tiles] = nn;
  if (edge_off) edge_off[g->n_tiles] = ne;
  g->n_nodes_host = nn; g->n_edges_host = ne;
  if (n_nodes) *n_nodes = nn;
  if (n_edges) *n_edges = ne;
  return BGNN_OK;
}

int bgnn_graph_export(bgnn_graph *g, float *x, int64_t *edge_index, float *edge_attr, float *pos,
                      int64_t *valid_rows, int64_t *valid_cols, float *local_std, int64_t *batch) {
  BGNN_REQUIRE(g, "graph is NULL");
  BGNN_REQUIRE(g->kind == 0, "bgnn_graph_export: only graphs built by bgnn_graph_build can be exported");
  BGNN_HIP_CHECK(hipSetDevice(g->ctx->device));
  return launch_graph_export(g, x, edge_index, edge_attr, pos, valid_rows, valid_cols, local_std, batch);
}

int bgnn_graph_scatter(bgnn_graph *g, const float *node_values, float fill, float *grid) {
  BGNN_REQUIRE(g && node_values && grid, "bgnn_graph_scatter: NULL argument");
  BGNN_REQUIRE(g->kind == 0, "Data object missing grid_shape metadata");
  BGNN_HIP_CHECK(hipSetDevice(g->ctx->device));
  return launch_graph_scatter(g, node_values, fill, grid);
}

}  // extern "C"
