// The model half of the C ABI (include/bgnn.h), device side: bgnn_model_create / bgnn_model_destroy, the model's pointers into its
// blob, model_sync and the device tables of bgnn_model_refresh.  What the blob holds, where, and how it is made from the weights
// is model_images.h (host arithmetic only): image_map lays a model out once, at creation, and the map stays with the model;
// fill_images writes every image; refresh_plan derives the refresh tables.
#include "bgnn_internal.h"

namespace bgnn {

// The model's pointers, once, from its map: an image that does not exist for the model's shape is nullptr.
static void model_assign_pointers(bgnn_model *m) {
  const bgnn_model_desc &d = m->desc;
  const ImageMap &I = m->images;
  const int hid = d.hidden, L = d.num_layers;
  auto at = [&](const Image &im) { return im.floats ? m->blob + im.off : nullptr; };
  m->fe_W0t = at(I.fe_W0t); m->fe_b0 = at(I.fe_b0); m->fe_W1t = at(I.fe_W1t); m->fe_b1 = at(I.fe_b1);
  m->l0f_Wt = at(I.l0f_Wt); m->l0f_b = at(I.l0f_b); m->l0f_Wsp = at(I.l0f_Wsp); m->l0f_Wbf = at(I.l0f_Wbf); m->l0f_Wpm = at(I.l0f_Wpm);
  m->l0f_Wt_blk = at(I.l0f_Wt_blk); m->l0af_W = at(I.l0af_W); m->l0af_shift = at(I.l0af_shift);
  m->ones = at(I.ones); m->raw = at(I.raw);
  m->head_hidden_total = I.HT;
  m->hd_W0 = at(I.hd_W0); m->hd_W0t = at(I.hd_W0t); m->hd_b0 = at(I.hd_b0); m->hd_W1 = at(I.hd_W1); m->hd_b1 = at(I.hd_b1);
  m->hd_W0sp = at(I.hd_W0sp); m->hd_W0bf = at(I.hd_W0bf); m->hd_W0fp = at(I.hd_W0fp);
  m->hd_tab = I.htab_ok ? at(I.hd_tab) : nullptr;
  m->layers.assign(L, BgnnLayer{});
  for (int l = 0; l < L; ++l) {
    const ImageMap::Layer &M = I.layers[l];
    BgnnLayer &Ly = m->layers[l];
    const bool gat = d.gnn_type == BGNN_GNN_GAT, last = l == L - 1;
    Ly.heads = gat && !last ? d.heads : 1; Ly.d_in = gat && l > 0 ? hid * d.heads : hid; Ly.width = Ly.heads * hid; Ly.concat = !last;
    Ly.Wt = at(M.Wt); Ly.Wt_blk = at(M.Wt_blk); Ly.att_src = at(M.att_src); Ly.att_dst = at(M.att_dst); Ly.V = at(M.V);
    Ly.scale = at(M.scale); Ly.shift = at(M.shift); Ly.Wsp = at(M.Wsp); Ly.Wfp = at(M.Wfp); Ly.Wbf = at(M.Wbf);
    Ly.b1 = at(M.b1); Ly.Wt2 = at(M.Wt2); Ly.b2 = at(M.b2);
    Ly.tr_bias = at(M.tr_bias); Ly.bn_w = at(M.bn_w); Ly.bn_b = at(M.bn_b); Ly.tr_Wt = at(M.tr_Wt);
  }
}

// What follows the weight VALUES: the float16 images are there when every weight fits float16 (else BGNN_SPLIT_F16 falls back to
// the bf16 split), their scales, the host copy of the folded edge vectors (model_canonical_V).  After every fill.
static void model_assign_values(bgnn_model *m, PackValues &&pv) {
  const ImageMap &I = m->images;
  auto f16 = [&](const Image &im) { return im.floats && pv.f16_ok ? m->blob + im.off : nullptr; };
  m->l0f_Wsp16 = f16(I.l0f_Wsp16); m->hd_W0sp16 = f16(I.hd_W0sp16);
  m->l0f_Wsp16_inv = pv.inv16_l0f; m->hd_W0sp16_inv = pv.inv16_hd;
  for (size_t l = 0; l < m->layers.size(); ++l) { m->layers[l].Wsp16 = f16(I.layers[l].Wsp16); m->layers[l].Wsp16_inv = pv.inv16[l]; }
  m->h_V = std::move(pv.h_V);
}

static int model_create_native(bgnn_ctx *ctx, const bgnn_model_desc *d, WeightLayout &&wl, const float *w, bgnn_model **out) {
  // (the generic kernels take 32 / 64 / 128 as long as a layer stays within 256 columns -- the heads' hidden/2 has to be a multiple of
  //  16 and their three first layers side by side a multiple of 32; the fused kernels exist for hidden 64 only, the reference's
  //  default: config/config.py:41)
  BGNN_REQUIRE(d->hidden == 32 || d->hidden == 64 || d->hidden == 128, "hidden_channels=%d unsupported (32, 64 or 128)", d->hidden);
  BGNN_REQUIRE(d->in_channels >= 1 && d->in_channels <= 16, "in_channels=%d unsupported (1..16)", d->in_channels);
  BGNN_REQUIRE(d->num_layers >= 1 && d->num_layers <= 64, "num_gnn_layers=%d unsupported", d->num_layers);
  BGNN_REQUIRE(d->gnn_type >= BGNN_GNN_GAT && d->gnn_type <= BGNN_GNN_GIN, "gnn_type=%d unknown", d->gnn_type);
  const bool gat = d->gnn_type == BGNN_GNN_GAT;
  // (`heads` only shapes a GAT backbone: models/gnn.py:125-143)
  // (up to 256 columns a layer is one launch per kernel; 512 columns -- 8 heads of 64, 4 of 128 -- run the generic kernels in two
  //  256-column blocks: Wt_blk)
  BGNN_REQUIRE(!gat || (d->heads >= 1 && d->heads * d->hidden <= 512 && (d->heads & (d->heads - 1)) == 0),
               "heads=%d unsupported (power of two, heads*hidden <= 512)", d->heads);
  BGNN_REQUIRE(!gat || (d->edge_dim >= 1 && d->edge_dim <= 4), "edge_dim=%d unsupported (1..4)", d->edge_dim);
  BGNN_REQUIRE(d->num_classes >= 1 && d->num_classes <= 16, "num_classes=%d unsupported", d->num_classes);
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  bgnn_model *m = new bgnn_model();
  m->ctx = ctx; m->desc = *d; m->weights = std::move(wl); m->images = image_map(*d);
  std::vector<float> pk(m->images.total, 0.0f);
  PackValues pv;
  fill_images(m->desc, m->weights, m->images, w, pk.data(), &pv);
  hipError_t e = hipMalloc((void **)&m->blob, pk.size() * sizeof(float));
  if (e != hipSuccess) { delete m; set_error("hipMalloc(model) failed: %s", hipGetErrorString(e)); return BGNN_ERR_NOMEM; }
  e = hipMemcpy(m->blob, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(m->blob); delete m; set_error("hipMemcpy(model) failed: %s", hipGetErrorString(e)); return BGNN_ERR_HIP; }
  model_assign_pointers(m);
  model_assign_values(m, std::move(pv));
  *out = m;
  return BGNN_OK;
}

// The edge vectors of every GAT layer over the canonical attributes (distance, depth_difference, slope) for a graph built with
// another edge feature list: device table [layers][heads][3], V3[l][h][id] = sum over the list positions j with ids[j] == id of
// V_l[h][j] ("zero" columns drop out, a repeated attribute adds up).  Made once per (model, list) and kept with the model.
int model_canonical_V(bgnn_model *m, const bgnn_graph *g, const float **out) {
  const int ED = g->ED, heads = m->desc.heads;
  uint32_t key = (uint32_t)ED;
  for (int j = 0; j < 4; ++j) key = key * 8u + (uint32_t)(j < ED ? g->edge_ids[j] : 7);
  for (auto &kv : m->v3_tables)
    if (kv.first == key) { *out = kv.second; return BGNN_OK; }
  const size_t L = m->layers.size();
  std::vector<float> t(L * (size_t)heads * 3, 0.0f);
  size_t off = 0;
  for (size_t l = 0; l < L; ++l) {
    const int H = m->layers[l].heads;
    for (int h = 0; h < H; ++h)
      for (int j = 0; j < ED; ++j) {
        const int id = g->edge_ids[j];
        if (id >= 0 && id < 3) t[(l * heads + h) * 3 + id] += m->h_V[off + (size_t)h * ED + j];
      }
    off += (size_t)H * ED;
  }
  float *d = nullptr;
  BGNN_HIP_CHECK(hipMalloc((void **)&d, t.size() * sizeof(float)));
  if (hipMemcpy(d, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    set_error("hipMemcpy(canonical edge vectors) failed");
    return BGNN_ERR_HIP;
  }
  m->v3_tables.emplace_back(key, d);
  *out = d;
  return BGNN_OK;
}

// Stale eval images (bgnn_model_refresh rewrote only what training reads): the fill over the weights the model holds, into the
// allocation it has -- the map is the model's own, so nothing moves.  Waits for the stream twice (download, upload from pageable
// memory).
int model_sync_slow(bgnn_ctx *ctx, bgnn_model *m) {
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  std::vector<float> w(m->weights.total), pk(m->images.total, 0.0f);
  BGNN_HIP_CHECK(hipMemcpyAsync(w.data(), m->raw, w.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  BGNN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  PackValues pv;
  fill_images(m->desc, m->weights, m->images, w.data(), pk.data(), &pv);
  BGNN_HIP_CHECK(hipMemcpyAsync(m->blob, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  BGNN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  model_assign_values(m, std::move(pv));               // (the float16 images may have come or gone with the weights' range; h_V)
  for (auto &kv : m->v3_tables) (void)hipFree(kv.second);   // (the stream is idle: nothing reads them; remade on demand)
  m->v3_tables.clear();
  m->eval_stale = false;
  return BGNN_OK;
}

// The device tables of bgnn_model_refresh: refresh_plan's (model_images.h), uploaded as one allocation.
int model_refresh_tables(bgnn_ctx *ctx, bgnn_model *m) {
  if (m->refresh) return BGNN_OK;
  if (m->weights.total >= ((size_t)1 << 24) || m->images.total >= ((size_t)1 << 31)) {
    set_error("bgnn_model_refresh: a model of %zu weights is beyond the gather tables (2^24)", m->weights.total);
    return BGNN_ERR_UNSUPPORTED;
  }
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const RefreshPlan P = refresh_plan(m->desc, m->weights, m->images);
  BGNN_REQUIRE(P.error.empty(), "bgnn_model_refresh: %s (internal)", P.error.c_str());
  RefreshTables *T = new RefreshTables();
  T->fold_cols = P.fold_cols; T->fe_W1 = P.fe_W1; T->fe_b1 = P.fe_b1; T->W0 = P.W0; T->l0f_Wt = P.l0f_Wt; T->l0f_b = P.l0f_b;
  T->n_copy = (int32_t)(P.copy.size() / 2); T->n_relay = (int32_t)(P.relay.size() / 2); T->n_vjob = (int32_t)(P.vjob.size() / 4);
  std::vector<int32_t> all;
  all.insert(all.end(), P.copy.begin(), P.copy.end());
  all.insert(all.end(), P.relay.begin(), P.relay.end());
  all.insert(all.end(), P.vjob.begin(), P.vjob.end());
  all.push_back(0);                                    // (never an empty allocation)
  hipError_t e = hipMalloc((void **)&T->dev, all.size() * sizeof(int32_t));
  if (e != hipSuccess) { delete T; set_error("hipMalloc(refresh tables) failed: %s", hipGetErrorString(e)); return BGNN_ERR_NOMEM; }
  e = hipMemcpy(T->dev, all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(T->dev); delete T; set_error("hipMemcpy(refresh tables) failed: %s", hipGetErrorString(e)); return BGNN_ERR_HIP; }
  T->d_copy = T->dev; T->d_relay = T->d_copy + P.copy.size(); T->d_vjob = T->d_relay + P.relay.size();
  m->refresh = T;
  return BGNN_OK;
}

}  // namespace bgnn

using namespace bgnn;

extern "C" {

size_t bgnn_model_weight_count(const bgnn_model_desc *d) { return d ? weight_layout(*d).total : 0; }

int bgnn_model_create(bgnn_ctx *ctx, const bgnn_model_desc *d_in, const float *w, size_t n_weights, bgnn_model **out) {
  BGNN_REQUIRE(ctx && d_in && w && out, "bgnn_model_create: NULL argument");
  bgnn_model_desc dl = *d_in;                                  // the LOGICAL model
  BGNN_REQUIRE(dl.gnn_type >= BGNN_GNN_GAT && dl.gnn_type <= BGNN_GNN_GIN, "gnn_type=%d unknown", dl.gnn_type);
  const bool gat = dl.gnn_type == BGNN_GNN_GAT;
  if (!gat) dl.heads = 1;                                      // (`heads` only shapes a GAT backbone: models/gnn.py:125-143)
  BGNN_REQUIRE(dl.hidden >= 2 && dl.hidden <= 128, "hidden_channels=%d unsupported (2..128)", dl.hidden);
  BGNN_REQUIRE(dl.heads >= 1 && dl.heads <= 256 && pad_heads(dl.heads) * pad_hidden(dl.hidden) <= 512,
               "heads=%d x hidden_channels=%d unsupported: the layer is laid out as %d heads of %d channels (next power of two x next of "
               "32 / 64 / 128), which must stay within 512 columns", dl.heads, dl.hidden, pad_heads(dl.heads), pad_hidden(dl.hidden));
  BGNN_REQUIRE(dl.in_channels >= 1 && dl.in_channels <= 16, "in_channels=%d unsupported (1..16)", dl.in_channels);
  BGNN_REQUIRE(dl.num_layers >= 1 && dl.num_layers <= 64, "num_gnn_layers=%d unsupported", dl.num_layers);
  BGNN_REQUIRE(!gat || (dl.edge_dim >= 1 && dl.edge_dim <= 4), "edge_dim=%d unsupported (1..4)", dl.edge_dim);
  BGNN_REQUIRE(dl.num_classes >= 1 && dl.num_classes <= 16, "num_classes=%d unsupported", dl.num_classes);
  WeightLayout ll = weight_layout(dl);
  BGNN_REQUIRE(n_weights == ll.total, "weight blob has %zu floats, expected %zu", n_weights, ll.total);
  const bool padded = pad_hidden(dl.hidden) != dl.hidden || (gat && pad_heads(dl.heads) != dl.heads);
  int rc;
  if (!padded) {
    rc = model_create_native(ctx, &dl, std::move(ll), w, out);
  } else {
    bgnn_model_desc dp;
    WeightLayout lp;
    std::vector<float> wp;
    pad_model_weights(&dl, ll, w, &dp, &lp, wp);
    rc = model_create_native(ctx, &dp, std::move(lp), wp.data(), out);
  }
  if (rc != BGNN_OK) return rc;
  (*out)->logical_hidden = dl.hidden; (*out)->logical_heads = dl.heads; (*out)->padded = padded;
  return BGNN_OK;
}

int bgnn_model_destroy(bgnn_model *m) {
  if (!m) return BGNN_OK;
  (void)hipSetDevice(m->ctx->device);
  (void)hipStreamSynchronize(m->ctx->stream);
  (void)hipFree(m->blob);
  for (auto &kv : m->v3_tables) (void)hipFree(kv.second);
  if (m->refresh) { (void)hipFree(m->refresh->dev); delete m->refresh; }
  delete m;
  return BGNN_OK;
}

}  // extern "C"
