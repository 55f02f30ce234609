// The training half of the C ABI (include/bgnn_train.h): the tape of a training step, the training-mode forward and the backward
// pass.  Host code only; kernels live in the other TUs.
#include <algorithm>

#include "bgnn_internal.h"

using namespace bgnn;

// The tape of a taped training forward (bgnn_forward_train_tape): byte offsets of the saved activations.  Header (BgnnTapeHeader)
// at 0, then in this order, every table [row_capacity][width] float32 row-major and starting on a 256-byte boundary:
//   h0, h1: the extractor's ReLU(+dropout) output of its first Linear, the output of its second [hidden];
//   per layer: GAT the lin output xw [HC] and the attention dots asd [2H] | GraphSAGE the neighbour mean agg | GIN agg = s (sum of
//   the neighbours + self) and u (ReLU output of nn.0) [hidden]; then z (BatchNorm input) and hout (layer output) [W], the batch
//   statistics mean and rstd (float64 [W]);
//   hbd: the heads' hidden units after ReLU and dropout [head_hidden_total].
// Entries a backbone does not save stay 0.
struct TapeLayout {
  struct Layer { size_t xw, asd, agg, u, z, hout, mean, rstd; };
  size_t h0 = 0, h1 = 0;
  std::vector<Layer> layers;
  size_t hbd = 0;
  size_t total = 0;
};

static TapeLayout tape_layout(const bgnn_model *m, const bgnn_graph *g) {
  const size_t rows = (size_t)std::max<int32_t>(g->row_capacity, 0), hid = (size_t)m->desc.hidden;
  const bool gat = m->desc.gnn_type == BGNN_GNN_GAT, gin = m->desc.gnn_type == BGNN_GNN_GIN;
  TapeLayout t;
  size_t off = 256;
  auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  t.h0 = take(rows * hid * 4); t.h1 = take(rows * hid * 4);
  for (const BgnnLayer &L : m->layers) {             // (a plain layer: one head, hidden wide)
    const size_t HC = (size_t)L.heads * hid, W = (size_t)L.width;
    TapeLayout::Layer e{};
    if (gat) { e.xw = take(rows * HC * 4); e.asd = take(rows * 2 * L.heads * 4); }
    else { e.agg = take(rows * hid * 4); if (gin) e.u = take(rows * hid * 4); }
    e.z = take(rows * W * 4); e.hout = take(rows * W * 4);
    e.mean = take(W * 8); e.rstd = take(W * 8);
    t.layers.push_back(e);
  }
  t.hbd = take(rows * (size_t)m->head_hidden_total * 4);
  t.total = off;
  return t;
}

// what the backward pass covers (BGNN_ERR_UNSUPPORTED + message otherwise)
static int backward_supported(const bgnn_model *m) {
  const bgnn_model_desc &d = m->desc;
  if (d.gnn_type == BGNN_GNN_GCN) {
    set_error("backward pass: the GCN backbone has none (the GAT, GraphSAGE and GIN backbones have one)");
    return BGNN_ERR_UNSUPPORTED;
  }
  if (m->padded) {
    set_error("backward pass: hidden_channels=%d / heads=%d run zero-padded; the training path exists for hidden 32 / 64 / 128 and "
              "power-of-two head counts only", m->logical_hidden, m->logical_heads);
    return BGNN_ERR_UNSUPPORTED;
  }
  for (const BgnnLayer &L : m->layers)
    if (L.heads * d.hidden > 256) {
      set_error("backward pass: layers wider than 256 columns are not supported (heads=%d x hidden_channels=%d = %d)", L.heads, d.hidden,
                L.heads * d.hidden);
      return BGNN_ERR_UNSUPPORTED;
    }
  return BGNN_OK;
}

// training-mode forward: BatchNorm statistics of this batch, written layer by layer ([sum of layer widths] each)
struct TrainOut {
  float *mean, *var_unbiased;
  const bgnn_dropout *dp = nullptr;      // active dropout (bgnn_forward_train_dropout)
  char *tape = nullptr;                  // taped forward: saved activations (TapeLayout)
};

// Exact float32, unfused: BatchNorm takes its statistics from the batch (batch statistics amplify the error of the operand-split
// matrix paths, and the fused layers carry the folded eval statistics).
static int forward_train(bgnn_ctx *ctx, bgnn_model *m, bgnn_graph *g, const bgnn_outputs *o, const TrainOut &tr) {
  FwdTables t;
  BGNN_TRY(forward_begin(ctx, m, g, &t));
  if (t.rows <= 0) return BGNN_OK;
  const bgnn_model_desc &d = m->desc;
  const bool gat = d.gnn_type == BGNN_GNN_GAT;
  const int64_t rows = t.rows, *dm = t.dm;
  const int hid = d.hidden;
  const int maxw = std::max(2 * hid, d.heads * hid);
  float *X = t.X, *Y = t.Y, *asdX = t.asdX;
  // the node table: 8-column rows, or the wide table of a build with auxiliary planes (bgnn_aux.h); Kx: rows of fe_W0t
  const float *xt = g->d_x;
  const int ldx = g->ldx, Kx = extractor_rows(d.in_channels);
  void *bnws = nullptr;
  BGNN_TRY(ctx_workspace(ctx, 5, bn_train_workspace_bytes(maxw >= 256 ? 256 : maxw), &bnws));
  // taped forward: the saved activations are COPIES of the forward's own tables (outputs and statistics stay bit-identical)
  char *tape = tr.tape;
  const TapeLayout tl = tape_layout(m, g);
  auto save = [&](size_t off, const void *src, size_t bytes) -> int {
    if (tape) BGNN_HIP_CHECK(hipMemcpyAsync(tape + off, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return BGNN_OK;
  };
  const size_t tab = (size_t)rows * hid * sizeof(float);   // (bytes of one [rows][hid] table of the tape)
  // active dropout: x [rows][width] *= keep / (1 - p) in place (stream ids: bgnn.h, bgnn_dropout)
  const bgnn_dropout *dp = tr.dp;
  auto drop = [&](float *x, int width, float p, uint32_t stream) {
    return dp && p > 0.0f ? launch_dropout(ctx, x, width, width, dm, rows, make_drop_spec(p, dp->seed, stream)) : BGNN_OK;
  };
  size_t tr_off = 0, bn_layer = 0;
  auto batch_norm = [&](float *z, const BgnnLayer &L, int relu) {          // z [rows][L.width], in place (256 columns per launch)
    int rc = BGNN_OK;
    double *s_mean = nullptr, *s_rstd = nullptr;    // taped: the statistics go to the tape as well
    if (tape) { s_mean = (double *)(tape + tl.layers[bn_layer].mean); s_rstd = (double *)(tape + tl.layers[bn_layer].rstd); }
    for (int c0 = 0; c0 < L.width && rc == BGNN_OK; c0 += 256) {
      const int w = std::min(256, L.width - c0);
      rc = launch_bn_train(ctx, z + c0, L.width, w, rows, dm, L.bn_w + c0, L.bn_b + c0, d.bn_eps, relu, bnws,
                           tr.mean ? tr.mean + tr_off + c0 : nullptr, tr.var_unbiased ? tr.var_unbiased + tr_off + c0 : nullptr,
                           s_mean ? s_mean + c0 : nullptr, s_rstd ? s_rstd + c0 : nullptr);
    }
    tr_off += (size_t)L.width;
    ++bn_layer;
    return rc;
  };
  const size_t nl = m->layers.size();
  // feature extractor (gnn.py:386): Linear(in,hid) ReLU [Dropout] Linear(hid,hid); then the backbone
  if (!gat) {
    // GCN / GraphSAGE / GIN backbones (gnn.py:120-143; torch_geometric default arguments): plain gathers + GEMMs, the layer's
    // last map unfolded (tr_bias, tr_Wt), BatchNorm afterwards
    BGNN_TRY(launch_gemm_f32(ctx, xt, ldx, m->fe_W0t, m->fe_b0, Y, hid, dm, rows, Kx, hid, 1));
    if (dp) BGNN_TRY(drop(Y, hid, dp->p_extractor, 1));
    BGNN_TRY(launch_gemm_f32(ctx, Y, hid, m->fe_W1t, m->fe_b1, X, hid, dm, rows, hid, hid, 0));
    BGNN_TRY(save(tl.h0, Y, tab));
    BGNN_TRY(save(tl.h1, X, tab));
    float *dinv = asdX;
    if (d.gnn_type == BGNN_GNN_GCN) BGNN_TRY(launch_degree_inv_sqrt(ctx, g, dinv));
    for (size_t l = 0; l < nl; ++l) {                 // invariant: X = h_l [rows][hid]
      const BgnnLayer &L = m->layers[l];
      const TapeLayout::Layer &T = tl.layers[l];
      const int relu = l + 1 < nl ? 1 : 0;
      if (d.gnn_type == BGNN_GNN_GCN) {               // lin, normalised aggregate, + bias
        BGNN_TRY(launch_gemm_f32(ctx, X, hid, L.Wt, nullptr, Y, hid, dm, rows, hid, hid, 0));
        BGNN_TRY(launch_neighbor_reduce(ctx, g, 1, Y, hid, dinv, m->ones, L.tr_bias, 0, X, hid, nullptr));
      } else if (d.gnn_type == BGNN_GNN_SAGE) {       // [mean_j x_j | x_i] @ [lin_l ; lin_r]^T + bias
        BGNN_TRY(launch_neighbor_reduce(ctx, g, 2, X, hid, nullptr, nullptr, nullptr, 0, Y, 2 * hid, Y + hid));
        if (tape)   // the mean half of the [mean | x] rows
          BGNN_HIP_CHECK(hipMemcpy2DAsync(tape + T.agg, (size_t)hid * sizeof(float), Y, (size_t)2 * hid * sizeof(float),
                                          (size_t)hid * sizeof(float), (size_t)rows, hipMemcpyDeviceToDevice, ctx->stream));
        BGNN_TRY(launch_gemm_f32(ctx, Y, 2 * hid, L.tr_Wt, L.tr_bias, X, hid, dm, rows, 2 * hid, hid, 0));
      } else {                                        // GIN: nn(sum_j x_j + x_i), nn = Linear ReLU Linear
        BGNN_TRY(launch_neighbor_reduce(ctx, g, 3, X, hid, nullptr, nullptr, nullptr, 0, Y, hid, nullptr));
        BGNN_TRY(save(T.agg, Y, tab));
        BGNN_TRY(launch_gemm_f32(ctx, Y, hid, L.Wt, L.b1, X, hid, dm, rows, hid, hid, 1));
        BGNN_TRY(save(T.u, X, tab));
        BGNN_TRY(launch_gemm_f32(ctx, X, hid, L.tr_Wt, L.tr_bias, Y, hid, dm, rows, hid, hid, 0));
        std::swap(X, Y);
      }
      // X = z: BatchNorm, ReLU, feature dropout
      BGNN_TRY(save(T.z, X, tab));
      BGNN_TRY(batch_norm(X, L, relu));
      if (dp && relu) BGNN_TRY(drop(X, hid, dp->p_features, 64 + (uint32_t)l));
      BGNN_TRY(save(T.hout, X, tab));
    }
    std::swap(X, Y);                                  // the tail below expects the backbone output in Y
  } else {
    const BgnnLayer &L0 = m->layers[0];
    if (ctx->opts.fold_extractor) {       // second extractor layer folded into lin_0 (see bgnn_model_create)
      // extractor layer 1 runs inside the lin_0 GEMM (same instructions, h1 never leaves the registers) wherever that GEMM takes
      // its W-resident form; below 32 768 rows it keeps its own launch -- the results are bit-identical either way
      // (active extractor dropout sits between the two: the first layer then keeps its own launch)
      // (... and the front form reads 8-column node rows: a graph with auxiliary planes, bgnn_aux.h, keeps the own launch too)
      const bool front = ldx == 8 && hid == 64 && gemm_front_available(ctx, rows, L0.heads * hid, 0) && !(dp && dp->p_extractor > 0.0f);
      if (!front) BGNN_TRY(launch_gemm_f32(ctx, xt, ldx, m->fe_W0t, m->fe_b0, Y, hid, dm, rows, Kx, hid, 1));
      if (!front && dp) BGNN_TRY(drop(Y, hid, dp->p_extractor, 1));
      if (tape) {        // the folded chain never forms h0 (front form) or h1: the tape gets them from their own launches
        float *h0 = (float *)(tape + tl.h0);
        if (front) BGNN_TRY(launch_gemm_f32(ctx, g->d_x8, 8, m->fe_W0t, m->fe_b0, h0, hid, dm, rows, 8, hid, 1));
        else BGNN_TRY(save(tl.h0, Y, tab));
        BGNN_TRY(launch_gemm_f32(ctx, h0, hid, m->fe_W1t, m->fe_b1, (float *)(tape + tl.h1), hid, dm, rows, hid, hid, 0));
      }
      BGNN_TRY(launch_gemm_f32(ctx, front ? g->d_x8 : Y, front ? 8 : hid, m->l0f_Wt, m->l0f_b, X, L0.heads * hid, dm, rows, hid,
                               L0.heads * hid, 0, L0.att_src, L0.att_dst, asdX, L0.heads, hid, nullptr, 0,
                               front ? m->fe_W0t : nullptr, front ? m->fe_b0 : nullptr, front ? m->l0f_Wpm : nullptr,
                               m->l0f_Wt_blk, 1.0f));
    } else {
      BGNN_TRY(launch_gemm_f32(ctx, xt, ldx, m->fe_W0t, m->fe_b0, X, hid, dm, rows, Kx, hid, 1));
      if (dp) BGNN_TRY(drop(X, hid, dp->p_extractor, 1));
      BGNN_TRY(launch_gemm_f32(ctx, X, hid, m->fe_W1t, m->fe_b1, Y, hid, dm, rows, hid, hid, 0));
      BGNN_TRY(save(tl.h0, X, tab));
      BGNN_TRY(save(tl.h1, Y, tab));
      BGNN_TRY(launch_gemm_f32(ctx, Y, L0.d_in, L0.Wt, nullptr, X, L0.heads * hid, dm, rows, L0.d_in, L0.heads * hid, 0,
                               L0.att_src, L0.att_dst, asdX, L0.heads, hid, nullptr, 0, nullptr, nullptr, nullptr, L0.Wt_blk));
    }
    // GNN backbone (gnn.py:173-188).  Invariant at the top of each iteration: X = lin_l(h_l), asdX = its dots.
    for (size_t l = 0; l < nl; ++l) {
      BgnnLayer L = m->layers[l];                        // out = aggregate + bias, BatchNorm afterwards
      L.scale = m->ones; L.shift = L.tr_bias;
      const TapeLayout::Layer &T = tl.layers[l];
      const int relu = L.concat ? 1 : 0;
      const size_t out_bytes = (size_t)rows * L.width * sizeof(float);
      // GATConv(dropout = p): the coefficients are thinned inside the plain aggregate kernel
      const bool att_drop = dp && dp->p_attention > 0.0f;
      const DropSpec att_spec = att_drop ? make_drop_spec(dp->p_attention, dp->seed, 16 + (uint32_t)l) : DropSpec{};
      BGNN_TRY(save(T.xw, X, (size_t)rows * L.heads * hid * sizeof(float)));
      BGNN_TRY(save(T.asd, asdX, (size_t)rows * 2 * L.heads * sizeof(float)));
      BGNN_TRY(gat_aggregate_unfused(ctx, g, L, hid, d.edge_dim, X, asdX, Y, 0, att_drop ? &att_spec : nullptr));
      BGNN_TRY(save(T.z, Y, out_bytes));
      BGNN_TRY(batch_norm(Y, L, relu));
      if (dp && relu) BGNN_TRY(drop(Y, L.width, dp->p_features, 64 + (uint32_t)l));     // (a single-layer backbone has no ReLU: never)
      BGNN_TRY(save(T.hout, Y, out_bytes));
      if (l + 1 < nl) {
        const BgnnLayer &Ln = m->layers[l + 1];
        BGNN_TRY(launch_gemm_f32(ctx, Y, Ln.d_in, Ln.Wt, nullptr, X, Ln.heads * hid, dm, rows, Ln.d_in, Ln.heads * hid, 0,
                                 Ln.att_src, Ln.att_dst, asdX, Ln.heads, hid, nullptr, 0, nullptr, nullptr, nullptr, Ln.Wt_blk));
      }
    }
  }
  // heads (gnn.py:392-406)
  BGNN_TRY(forward_heads_hidden(ctx, m, Y, t, o));
  if (dp && dp->p_heads > 0.0f)      // (the draw is indexed over the heads' own units; the table may carry pad columns up to a multiple of 32)
    BGNN_TRY(launch_dropout(ctx, t.hidb, head_count(&d) * (hid / 2), m->head_hidden_total, dm, rows, make_drop_spec(dp->p_heads, dp->seed, 2)));
  BGNN_TRY(save(tl.hbd, t.hidb, (size_t)rows * m->head_hidden_total * sizeof(float)));
  BGNN_TRY(launch_heads_final(ctx, m, t.hidb, m->head_hidden_total, dm, rows, 0.85f, 0.6f, o));
  return BGNN_OK;
}

static int forward_train_impl(bgnn_ctx *ctx, bgnn_model *m, bgnn_graph *g, const bgnn_dropout *dropout, float *bn_batch_mean,
                              float *bn_batch_var, const bgnn_outputs *o, void *tape, size_t tape_bytes) {
  BGNN_REQUIRE(ctx && m && g && o, "bgnn_forward_train: NULL argument");
  if (dropout) {
    const float ps[4] = {dropout->p_extractor, dropout->p_attention, dropout->p_features, dropout->p_heads};
    for (float p : ps) BGNN_REQUIRE(p >= 0.0f && p < 1.0f, "bgnn_forward_train_dropout: dropout probability %g outside [0, 1)", (double)p);
    if (ps[0] == 0.0f && ps[1] == 0.0f && ps[2] == 0.0f && ps[3] == 0.0f) dropout = nullptr;
  }
  BGNN_REQUIRE(m->ctx == ctx && g->ctx == ctx, "bgnn_forward_train: model/graph belong to another context");
  if (m->padded) {      // (batch statistics and dropout draws are laid out over the layer widths the caller sees)
    set_error("bgnn_forward_train: hidden_channels=%d / heads=%d run zero-padded to %d / %d; the training-mode forward exists for "
              "hidden 32 / 64 / 128 and power-of-two head counts only", m->logical_hidden, m->logical_heads, m->desc.hidden, m->desc.heads);
    return BGNN_ERR_UNSUPPORTED;
  }
  BGNN_REQUIRE(!o->action && !o->needs_review && !o->auto_correct, "bgnn_forward_train: the deployment flags belong to predict()");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  int64_t c[4];
  BGNN_HIP_CHECK(hipMemcpyAsync(c, g->d_counts, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
  BGNN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  // torch.nn.functional.batch_norm in training mode refuses a single row the same way
  BGNN_REQUIRE(c[0] != 1, "Expected more than 1 value per channel when training, got input size [1, %d]", m->layers[0].width);
  TrainOut tr{bn_batch_mean, bn_batch_var, dropout};
  if (tape) {
    BGNN_TRY(backward_supported(m));
    const size_t need = tape_layout(m, g).total;
    BGNN_REQUIRE(tape_bytes >= need, "bgnn_forward_train_tape: the tape has %zu bytes, this model and graph need %zu (bgnn_tape_bytes)",
                 tape_bytes, need);
    BgnnTapeHeader h{};
    const bgnn_dropout *dp = dropout;
    h.s_ext = dp ? make_drop_spec(dp->p_extractor, dp->seed, 1).scale : 1.0f;
    h.s_feat = dp ? make_drop_spec(dp->p_features, dp->seed, 0).scale : 1.0f;
    h.s_heads = dp ? make_drop_spec(dp->p_heads, dp->seed, 2).scale : 1.0f;
    h.att = dp ? make_drop_spec(dp->p_attention, dp->seed, 16) : DropSpec{};
    BGNN_TRY(ctx_upload(ctx, &h, sizeof(h), tape));
    tr.tape = (char *)tape;
  }
  return forward_train(ctx, m, g, o, tr);
}

extern "C" {

int bgnn_forward_train(bgnn_ctx *ctx, bgnn_model *m, bgnn_graph *g, float *bn_batch_mean, float *bn_batch_var,
                       const bgnn_outputs *o) {
  return bgnn_forward_train_dropout(ctx, m, g, nullptr, bn_batch_mean, bn_batch_var, o);
}

int bgnn_forward_train_dropout(bgnn_ctx *ctx, bgnn_model *m, bgnn_graph *g, const bgnn_dropout *dropout, float *bn_batch_mean,
                               float *bn_batch_var, const bgnn_outputs *o) {
  return forward_train_impl(ctx, m, g, dropout, bn_batch_mean, bn_batch_var, o, nullptr, 0);
}

size_t bgnn_tape_bytes(const bgnn_model *m, const bgnn_graph *g) {
  if (!m || !g) { set_error("bgnn_tape_bytes: NULL argument"); return 0; }
  if (backward_supported(m) != BGNN_OK) return 0;
  return tape_layout(m, g).total;
}

int bgnn_forward_train_tape(bgnn_ctx *ctx, bgnn_model *m, bgnn_graph *g, const bgnn_dropout *dropout, float *bn_batch_mean,
                            float *bn_batch_var, const bgnn_outputs *o, void *tape, size_t tape_bytes) {
  BGNN_REQUIRE(tape, "bgnn_forward_train_tape: NULL tape");
  return forward_train_impl(ctx, m, g, dropout, bn_batch_mean, bn_batch_var, o, tape, tape_bytes);
}

// ---- backward --------------------------------------------------------------------------------------------------------------
int bgnn_backward(bgnn_ctx *ctx, bgnn_model *m, bgnn_graph *g, const void *tape, const bgnn_output_grads *gin, float *grad_weights) {
  BGNN_REQUIRE(ctx && m && g && tape && gin && grad_weights, "bgnn_backward: NULL argument");
  BGNN_REQUIRE(m->ctx == ctx && g->ctx == ctx, "bgnn_backward: model/graph belong to another context");
  BGNN_TRY(backward_supported(m));
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const bgnn_model_desc &d = m->desc;
  const WeightLayout &go = m->weights;                 // (the gradient blob is laid out as the weight blob)
  BGNN_HIP_CHECK(hipMemsetAsync(grad_weights, 0, go.total * sizeof(float), ctx->stream));   // (running statistics: 0)
  const int64_t rows = g->row_capacity;
  if (rows <= 0) return BGNN_OK;
  const bool gat = d.gnn_type == BGNN_GNN_GAT;
  BGNN_REQUIRE(g->F == d.in_channels && (!gat || g->ED == d.edge_dim), "bgnn_backward: graph does not fit the model");
  const TapeLayout tl = tape_layout(m, g);
  const char *tp = (const char *)tape;
  auto T = [&](size_t off) { return (float *)(tp + off); };
  const BgnnTapeHeader *hdr = (const BgnnTapeHeader *)tape;
  const float *s_ext = (const float *)tape, *s_feat = s_ext + 1;
  const int hid = d.hidden, hh = hid / 2, nc = d.num_classes, nh = head_count(&d), HT = m->head_hidden_total, ED = d.edge_dim;
  const int n2 = nc + nh - 1, L = (int)m->layers.size();
  const int64_t *dm = g->d_counts;
  int Hmax = 1;
  for (const BgnnLayer &Ly : m->layers) Hmax = std::max(Hmax, Ly.heads);
  const int64_t slots = gat ? gat_bwd_slot_count(g) : 0;
  // scratch (context slot 6): two row tables for the running gradient, dxw, d(attention dots), per-node dV shares, the per-slot
  // alpha~ / dlogit tables, the heads' gradients, dV, then the reduction workspaces; the plain backbones use the three row tables
  // (hidden wide) and a per-node 1 / in-degree in place of the attention tables
  const size_t RW = gat ? 256 : (size_t)hid;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  const size_t oG0 = take((size_t)rows * RW * 4), oG1 = take((size_t)rows * RW * 4), oDXW = take((size_t)rows * RW * 4);
  const size_t oDASD = take(gat ? (size_t)rows * 2 * Hmax * 4 : 0), oDVN = take(gat ? (size_t)rows * Hmax * ED * 4 : 0);
  const size_t oAL = take((size_t)slots * Hmax * 4), oDL = take((size_t)slots * Hmax * 4);
  const size_t oDY2 = take((size_t)rows * n2 * 4), oDHID = take((size_t)rows * HT * 4), oDV = take(64 * 4);
  const size_t oWG = take(wgrad_workspace_bytes()), oCS = take(colsum_workspace_bytes()), oBN = take(bn_backward_workspace_bytes(256));
  const size_t oCI = take(gat ? 0 : (size_t)rows * 4);
  void *ws;
  BGNN_TRY(ctx_workspace(ctx, 6, off, &ws));
  char *wb = (char *)ws;
  float *G0 = (float *)(wb + oG0), *G1 = (float *)(wb + oG1), *DXW = (float *)(wb + oDXW), *DASD = (float *)(wb + oDASD);
  float *DVN = (float *)(wb + oDVN), *AL = (float *)(wb + oAL), *DL = (float *)(wb + oDL), *DY2 = (float *)(wb + oDY2);
  float *DHID = (float *)(wb + oDHID), *DV = (float *)(wb + oDV), *CINV = (float *)(wb + oCI);
  void *WG = wb + oWG, *CS = wb + oCS, *BNW = wb + oBN;
  float *gw = grad_weights;
  const float *raw = m->raw;

  // heads (gnn.py:392-406): second layers, then the first layers, then dL/d(backbone output) = dhid . W0 (stacked)
  BGNN_TRY(launch_heads_backward(ctx, m, T(tl.hbd), gin->class_logits, gin->class_probs, gin->confidence,
                                 d.predict_correction ? gin->correction : nullptr, hdr, dm, rows, DY2, DHID));
  const float *hL = T(tl.layers[L - 1].hout);
  for (int k = 0; k < nh; ++k) {
    const int nout = k == 0 ? nc : 1, col = k == 0 ? 0 : nc + k - 1;
    BGNN_TRY(launch_wgrad(ctx, DY2 + col, n2, T(tl.hbd) + k * hh, HT, dm, rows, nout, hh, gw + go.hd_W1[k], hh, WG));
    BGNN_TRY(launch_colsum(ctx, DY2 + col, n2, nout, nullptr, 0, 0, 1, dm, rows, gw + go.hd_b1[k], CS));
    BGNN_TRY(launch_wgrad(ctx, DHID + k * hh, HT, hL, hid, dm, rows, hh, hid, gw + go.hd_W0[k], hid, WG));
    BGNN_TRY(launch_colsum(ctx, DHID + k * hh, HT, hh, nullptr, 0, 0, 1, dm, rows, gw + go.hd_b0[k], CS));
  }
  BGNN_TRY(launch_gemm_f32(ctx, DHID, HT, m->hd_W0, nullptr, G0, hid, dm, rows, HT, hid, 0));
  // GraphSAGE / GIN layers, last to first (every one hidden -> hidden).  Invariant: G0 = dL/d(output of layer l) [rows][hid]
  if (!gat && d.gnn_type == BGNN_GNN_SAGE) BGNN_TRY(launch_plain_inv_count(ctx, g, CINV));
  for (int l = L - 1; l >= 0 && !gat; --l) {
    const BgnnLayer &Ly = m->layers[l];
    const WeightLayout::Layer &O = go.layers[l];
    const TapeLayout::Layer &S = tl.layers[l];
    const int relu = l + 1 < L ? 1 : 0;
    const float *hin = l > 0 ? T(tl.layers[l - 1].hout) : T(tl.h1);
    // BatchNorm (+ ReLU + feature dropout) backward: G0 becomes dL/dz; then the bias of the layer's last map
    BGNN_TRY(launch_bn_backward(ctx, G0, relu ? T(S.hout) : nullptr, T(S.z), hid, (const double *)T(S.mean),
                                (const double *)T(S.rstd), Ly.bn_w, relu, s_feat, dm, rows, BNW, gw + O.bn_w, gw + O.bn_b));
    BGNN_TRY(launch_colsum(ctx, G0, hid, hid, nullptr, 0, 0, 1, dm, rows, gw + O.bias, CS));
    if (d.gnn_type == BGNN_GNN_SAGE) {
      // z = lin_l(mean) + lin_r(h): d lin_l.W = G^T mean, d lin_r.W = G^T h; dmean = G W_l (DXW), root = G W_r (G1)
      BGNN_TRY(launch_wgrad(ctx, G0, hid, T(S.agg), hid, dm, rows, hid, hid, gw + O.W, hid, WG));
      BGNN_TRY(launch_wgrad(ctx, G0, hid, hin, hid, dm, rows, hid, hid, gw + O.W2, hid, WG));
      BGNN_TRY(launch_gemm_f32(ctx, G0, hid, raw + O.W, nullptr, DXW, hid, dm, rows, hid, hid, 0));
      BGNN_TRY(launch_gemm_f32(ctx, G0, hid, raw + O.W2, nullptr, G1, hid, dm, rows, hid, hid, 0));
      // dh_j = root_j + sum over the out-edges j -> i of dmean_i / max(cnt_i, 1)
      BGNN_TRY(launch_plain_bwd_aggregate(ctx, g, 2, hid, G1, DXW, CINV, G0));
    } else {
      // z = nn.2(u), u = ReLU(nn.0(s)): d nn.2.W = G^T u; du = (G W_2) [u > 0] (DXW); d nn.0.b = sum du, d nn.0.W = du^T s;
      // ds = du W_1 (G1)
      BGNN_TRY(launch_wgrad(ctx, G0, hid, T(S.u), hid, dm, rows, hid, hid, gw + O.W2, hid, WG));
      BGNN_TRY(launch_gemm_f32(ctx, G0, hid, raw + O.W2, nullptr, DXW, hid, dm, rows, hid, hid, 0));
      BGNN_TRY(launch_relu_drop_bwd(ctx, DXW, hid, T(S.u), hid, hid, dm, rows, m->ones));
      BGNN_TRY(launch_colsum(ctx, DXW, hid, hid, nullptr, 0, 0, 1, dm, rows, gw + O.b1, CS));
      BGNN_TRY(launch_wgrad(ctx, DXW, hid, T(S.agg), hid, dm, rows, hid, hid, gw + O.W, hid, WG));
      BGNN_TRY(launch_gemm_f32(ctx, DXW, hid, raw + O.W, nullptr, G1, hid, dm, rows, hid, hid, 0));
      // s_i = sum_{j -> i} h_j + h_i: dh_j = ds_j + sum over the out-edges j -> i of ds_i
      BGNN_TRY(launch_plain_bwd_aggregate(ctx, g, 3, hid, G1, G1, nullptr, G0));
    }
  }
  // GAT layers, last to first.  Invariant: G0 = dL/d(output of layer l) [rows][width]
  for (int l = L - 1; l >= 0 && gat; --l) {
    const BgnnLayer &Ly = m->layers[l];
    const WeightLayout::Layer &O = go.layers[l];
    const TapeLayout::Layer &S = tl.layers[l];
    const int W = Ly.width, H = Ly.heads, HC = H * hid, D = Ly.d_in;
    const int relu = l + 1 < L ? 1 : 0;
    // BatchNorm (+ ReLU + feature dropout) backward: G0 becomes dL/dz; then the GAT bias
    BGNN_TRY(launch_bn_backward(ctx, G0, relu ? T(S.hout) : nullptr, T(S.z), W, (const double *)T(S.mean),
                                (const double *)T(S.rstd), Ly.bn_w, relu, s_feat, dm, rows, BNW, gw + O.bn_w, gw + O.bn_b));
    BGNN_TRY(launch_colsum(ctx, G0, W, W, nullptr, 0, 0, 1, dm, rows, gw + O.bias, CS));
    // attention (concat, or the last layer's single head: the aggregate's gradient is dL/dz itself)
    BGNN_TRY(launch_gat_backward(ctx, g, Ly, hid, ED, hdr, 16 + (uint32_t)l, T(S.xw), T(S.asd), G0, AL, DL, DASD, DVN, DXW));
    BGNN_TRY(launch_colsum(ctx, T(S.xw), HC, HC, DASD, 2 * H, 0, hid, dm, rows, gw + O.as, CS));
    BGNN_TRY(launch_colsum(ctx, T(S.xw), HC, HC, DASD, 2 * H, H, hid, dm, rows, gw + O.ad, CS));
    BGNN_TRY(launch_colsum(ctx, DVN, H * ED, H * ED, nullptr, 0, 0, 1, dm, rows, DV, CS));
    BGNN_TRY(launch_gat_edge_param_grads(ctx, DV, raw + O.ae, raw + O.We, H, hid, ED, gw + O.ae, gw + O.We));
    // lin: dW = dxw^T . h_in, dL/dh_in = dxw . W
    const float *hin = l > 0 ? T(tl.layers[l - 1].hout) : T(tl.h1);
    BGNN_TRY(launch_wgrad(ctx, DXW, HC, hin, D, dm, rows, HC, D, gw + O.W, D, WG));
    BGNN_TRY(launch_gemm_f32(ctx, DXW, HC, raw + O.W, nullptr, G1, D, dm, rows, HC, D, 0));
    std::swap(G0, G1);
  }
  // feature extractor (gnn.py:386): Linear, ReLU, Dropout, Linear
  BGNN_TRY(launch_wgrad(ctx, G0, hid, T(tl.h0), hid, dm, rows, hid, hid, gw + go.fe_W1, hid, WG));
  BGNN_TRY(launch_colsum(ctx, G0, hid, hid, nullptr, 0, 0, 1, dm, rows, gw + go.fe_b1, CS));
  BGNN_TRY(launch_gemm_f32(ctx, G0, hid, raw + go.fe_W1, nullptr, G1, hid, dm, rows, hid, hid, 0));
  BGNN_TRY(launch_relu_drop_bwd(ctx, G1, hid, T(tl.h0), hid, hid, dm, rows, s_ext));
  BGNN_TRY(launch_wgrad(ctx, G1, hid, g->d_x, g->ldx, dm, rows, hid, d.in_channels, gw + go.fe_W0, d.in_channels, WG));
  BGNN_TRY(launch_colsum(ctx, G1, hid, hid, nullptr, 0, 0, 1, dm, rows, gw + go.fe_b0, CS));
  return BGNN_OK;
}

}  // extern "C"
