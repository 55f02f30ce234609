// C ABI of libbgnn_hip.so (declared in include/bgnn.h): contexts, the pool and the forward / fused-inference orchestration
// (graph handles: graph_api.hip; models: model_pack.hip; training forward and backward: train_api.hip).  Host code only; kernels
// live in the other TUs.
#include <stdarg.h>
#include <string.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>

#include "bgnn_internal.h"

namespace bgnn {

static thread_local char g_err[1024] = "";

void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- pool -----------------------------------------------------------------------------------
int DevPool::alloc(size_t bytes, void **out) {
  if (bytes == 0) bytes = 256;
  bytes = (bytes + 255) & ~(size_t)255;
  auto it = free_blocks.lower_bound(bytes);
  if (it != free_blocks.end() && it->first <= bytes + bytes / 4 + 4096) {
    *out = it->second;
    live[*out] = it->first;
    free_blocks.erase(it);
    return BGNN_OK;
  }
  void *p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    trim();
    e = hipMalloc(&p, bytes);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error("device allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    return BGNN_ERR_NOMEM;
  }
  total_bytes += bytes;
  live[p] = bytes;
  *out = p;
  return BGNN_OK;
}

void DevPool::release(void *p) {
  if (!p) return;
  auto it = live.find(p);
  if (it == live.end()) return;
  free_blocks.emplace(it->second, p);
  live.erase(it);
}

void DevPool::trim() {
  for (auto &kv : free_blocks) {
    (void)hipFree(kv.second);
    total_bytes -= kv.first;
  }
  free_blocks.clear();
}

int ctx_workspace(bgnn_ctx *ctx, int slot, size_t bytes, void **out) {
  if (ctx->ws_bytes[slot] < bytes) {
    if (ctx->ws[slot]) {
      BGNN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
      BGNN_HIP_CHECK(hipFree(ctx->ws[slot]));
      ctx->ws[slot] = nullptr;
      ctx->ws_bytes[slot] = 0;
    }
    size_t want = bytes + bytes / 8;
    hipError_t e = hipMalloc(&ctx->ws[slot], want);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      ctx->pool.trim();
      want = bytes;
      e = hipMalloc(&ctx->ws[slot], want);
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      set_error("workspace allocation of %zu bytes failed: %s", want, hipGetErrorString(e));
      return BGNN_ERR_NOMEM;
    }
    ctx->ws_bytes[slot] = want;
  }
  *out = ctx->ws[slot];
  return BGNN_OK;
}

int ctx_upload(bgnn_ctx *ctx, const void *host, size_t bytes, void *dev) {
  if (bytes == 0) return BGNN_OK;
  bgnn_ctx::Staging *slot = nullptr;
  for (auto &st : ctx->staging) {
    if (st.cap < bytes) continue;
    if (st.in_flight && hipEventQuery(st.ev) != hipSuccess) continue;
    slot = &st;
    break;
  }
  (void)hipGetLastError();                            // hipEventQuery reports "not ready" as an error code
  if (!slot) {
    bgnn_ctx::Staging st{nullptr, std::max<size_t>(bytes, 64 * 1024), nullptr, false};
    BGNN_HIP_CHECK(hipHostMalloc(&st.p, st.cap, hipHostMallocDefault));
    BGNN_HIP_CHECK(hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
    ctx->staging.push_back(st);
    slot = &ctx->staging.back();
  }
  memcpy(slot->p, host, bytes);
  BGNN_HIP_CHECK(hipMemcpyAsync(dev, slot->p, bytes, hipMemcpyHostToDevice, ctx->stream));
  BGNN_HIP_CHECK(hipEventRecord(slot->ev, ctx->stream));
  slot->in_flight = true;
  return BGNN_OK;
}

ProfScope::ProfScope(bgnn_ctx *c, int kernel) : ctx(c), idx(-1) {
  if (!(c->prof_mask & (1u << kernel))) return;
  ProfRecord r;
  r.kernel = kernel;
  hipEvent_t ev[2];
  for (int i = 0; i < 2; ++i) {
    if (!c->event_pool.empty()) { ev[i] = c->event_pool.back(); c->event_pool.pop_back(); }
    else if (hipEventCreate(&ev[i]) != hipSuccess) return;
  }
  r.start = ev[0]; r.stop = ev[1];
  (void)hipEventRecord(r.start, c->stream);
  c->prof_records.push_back(r);
  idx = (int)c->prof_records.size() - 1;
}

ProfScope::~ProfScope() {
  if (idx >= 0) (void)hipEventRecord(ctx->prof_records[idx].stop, ctx->stream);
}

// x [n][in] -> x8 [n][8], zero padded (the node-feature layout of the graph build)
__global__ void pad_rows8_kernel(const float *x, int in, float *x8, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n * 8) x8[i] = (i & 7) < in ? x[(i >> 3) * in + (i & 7)] : 0.0f;
}
// ... -> x16 [n][16] for in > 8 (the wide node table of bgnn_aux.h)
__global__ void pad_rows16_kernel(const float *x, int in, float *x16, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n * 16) x16[i] = (i & 15) < in ? x[(i >> 4) * in + (i & 15)] : 0.0f;
}

__global__ void copy_cols_kernel(const float *src, int src_stride, float *dst, int dst_stride, int n_copy, const int64_t *d_m) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= *d_m * dst_stride) return;
  const int64_t r = i / dst_stride;
  const int c = (int)(i - r * dst_stride);
  dst[i] = c < n_copy ? src[r * src_stride + c] : 0.0f;
}

// rows [*d_m][src_stride] -> [*d_m][dst_stride]: the first n_copy columns, the rest of a destination row zero
static int launch_copy_cols(bgnn_ctx *ctx, const float *src, int src_stride, float *dst, int dst_stride, int n_copy, const int64_t *d_m,
                            int64_t rows_cap) {
  const int64_t n = rows_cap * dst_stride;
  if (n <= 0) return BGNN_OK;
  hipLaunchKernelGGL(copy_cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, src, src_stride, dst, dst_stride,
                     n_copy, d_m);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

// ---- what the inference forward and the training forward (train_api.hip) share ------------------------------------------------
int forward_begin(bgnn_ctx *ctx, const bgnn_model *m, const bgnn_graph *g, FwdTables *t) {
  const bgnn_model_desc &d = m->desc;
  BGNN_REQUIRE(g->F == d.in_channels, "mat1 and mat2 shapes cannot be multiplied (graph has %d node features, model expects %d)",
               g->F, d.in_channels);
  const bool gat = d.gnn_type == BGNN_GNN_GAT;
  BGNN_REQUIRE(!gat || g->ED == d.edge_dim, "edge_attr has %d columns, model edge_dim is %d", g->ED, d.edge_dim);
  const int64_t rows = g->row_capacity;
  if (rows <= 0) return BGNN_OK;
  const int maxw = std::max(2 * d.hidden, d.heads * d.hidden);
  void *pa, *pb, *pasd, *phid;
  BGNN_TRY(ctx_workspace(ctx, 0, (size_t)rows * maxw * sizeof(float), &pa));
  BGNN_TRY(ctx_workspace(ctx, 1, (size_t)rows * maxw * sizeof(float), &pb));
  BGNN_TRY(ctx_workspace(ctx, 2, (size_t)rows * 4 * d.heads * sizeof(float), &pasd));
  BGNN_TRY(ctx_workspace(ctx, 3, (size_t)rows * m->head_hidden_total * sizeof(float), &phid));
  t->X = (float *)pa; t->Y = (float *)pb; t->hidb = (float *)phid;
  t->asdX = (float *)pasd; t->asdY = t->asdX + rows * 2 * d.heads;
  t->dm = g->d_counts;
  if (!gat && g->kind != 0 && d.gnn_type != BGNN_GNN_GCN) {
    // foreign graphs: the CSR build dropped explicit self loops (GATConv and GCNConv replace them anyway); SAGEConv and
    // GINConv treat them as ordinary edges, which the CSR no longer holds
    int64_t c[4];
    BGNN_HIP_CHECK(hipMemcpyAsync(c, g->d_counts, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
    BGNN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (c[2] != c[1]) {
      set_error("GraphSAGE / GIN on a foreign graph with explicit self loops (or out-of-range edges: %lld of %lld edges kept) "
                "is not supported", (long long)c[2], (long long)c[1]);
      return BGNN_ERR_UNSUPPORTED;
    }
  }
  t->rows = rows;
  return BGNN_OK;
}

int gat_aggregate_unfused(bgnn_ctx *ctx, const bgnn_graph *g, const BgnnLayer &L, int C, int ED, const float *xw, const float *asd,
                          float *out, int relu, const DropSpec *attention_drop) {
  int rc = attention_drop ? BGNN_ERR_UNSUPPORTED : launch_gat_aggregate_tiled(ctx, g, L, C, ED, xw, asd, out, relu);
  if (rc == BGNN_ERR_UNSUPPORTED) rc = launch_gat_aggregate(ctx, g, L, C, ED, xw, asd, out, relu, attention_drop);
  return rc;
}

int forward_heads_hidden(bgnn_ctx *ctx, const bgnn_model *m, const float *h, const FwdTables &t, const bgnn_outputs *o) {
  const int hid = m->desc.hidden;
  if (o->hidden)                  // [N][logical hidden]: a padded model's pad columns (all zero) stay inside
    BGNN_TRY(launch_copy_cols(ctx, h, hid, o->hidden, m->logical_hidden, m->logical_hidden, t.dm, t.rows));
  return launch_gemm_f32(ctx, h, hid, m->hd_W0t, m->hd_b0, t.hidb, m->head_hidden_total, t.dm, t.rows, hid, m->head_hidden_total, 1);
}

}  // namespace bgnn

using namespace bgnn;

extern "C" {

int bgnn_abi_version(void) { return BGNN_ABI_VERSION; }
const char *bgnn_last_error(void) { return g_err; }

// ---- context ----------------------------------------------------------------------------------
int bgnn_ctx_create(int device, void *stream, bgnn_ctx **out) {
  BGNN_REQUIRE(out != nullptr, "bgnn_ctx_create: out is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    set_error("no HIP device available (%s)", e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    return BGNN_ERR_HIP;
  }
  BGNN_REQUIRE(device >= 0 && device < n, "bgnn_ctx_create: device %d out of range (have %d)", device, n);
  BGNN_HIP_CHECK(hipSetDevice(device));
  hipDeviceProp_t prop;
  BGNN_HIP_CHECK(hipGetDeviceProperties(&prop, device));
  bgnn_ctx *c = new bgnn_ctx();
  c->device = device;
  c->num_cus = prop.multiProcessorCount;
  if (stream) {
    c->stream = (hipStream_t)stream;
    c->owns_stream = false;
  } else {
    hipError_t se = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (se != hipSuccess) {
      delete c;
      set_error("hipStreamCreate failed: %s", hipGetErrorString(se));
      return BGNN_ERR_HIP;
    }
    c->owns_stream = true;
  }
  if (hipMalloc((void **)&c->zero_page, 16384) != hipSuccess || hipMemset(c->zero_page, 0, 16384) != hipSuccess) {
    set_error("zero page allocation failed");
    delete c;
    return BGNN_ERR_NOMEM;
  }
  c->stamps = reinterpret_cast<unsigned long long *>(c->zero_page + 1024);
  {   // defaults from the environment, read once per context
    auto env_int = [](const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; };
    BgnnOpts &o = c->opts;
    o.matrix_path = getenv("BGNN_BF16") ? 3 : getenv("BGNN_SPLIT_F16") ? 2 : getenv("BGNN_SPLIT_BF16") ? 1 : 0;
    o.fused = getenv("BGNN_NO_FUSED") ? 0 : 1;
    o.fold_extractor = getenv("BGNN_NO_FOLD") ? 0 : 1;
    o.ragged_atlas = getenv("BGNN_NO_ATLAS") ? 0 : 1;
    o.fused_front = getenv("BGNN_NO_FUSED_FRONT") ? 0 : 1;
    o.bf16_two_phase = getenv("BGNN_NO_TWO_PHASE") ? 0 : env_int("BGNN_TWO_PHASE", 1);
    o.bf16_layer0_af = getenv("BGNN_NO_LAYER0_AF") ? 0 : 1;
    o.stats_narrow = env_int("BGNN_STATS_NARROW", -1);
    o.diag_mask = env_int("BGNN_FUSED_DBG", 0);
    o.diag_stamps = getenv("BGNN_FUSED_STAMPS") ? 1 : 0;
    o.gemm_diag = env_int("BGNN_GEMM_DBG", 0);
    o.gemm_pair_major = getenv("BGNN_NO_PAIR_MAJOR") ? 0 : 1;
  }
  *out = c;
  return BGNN_OK;
}

static int *option_slot(bgnn_ctx *ctx, const char *name) {
  BgnnOpts &o = ctx->opts;
  struct { const char *n; int *p; } tab[] = {
      {"matrix_path", &o.matrix_path}, {"fused", &o.fused}, {"fold_extractor", &o.fold_extractor}, {"ragged_atlas", &o.ragged_atlas}, {"features_tiled", &o.features_tiled}, {"fused_front", &o.fused_front}, {"bf16_two_phase", &o.bf16_two_phase}, {"bf16_layer0_af", &o.bf16_layer0_af}, {"stats_narrow", &o.stats_narrow},
      {"diag_mask", &o.diag_mask}, {"diag_stamps", &o.diag_stamps}, {"gemm_diag", &o.gemm_diag}, {"gemm_pair_major", &o.gemm_pair_major}, {"fused_light_form", &o.fused_light_form}};
  for (auto &t : tab) if (strcmp(t.n, name) == 0) return t.p;
  return nullptr;
}

int bgnn_ctx_set_option(bgnn_ctx *ctx, const char *name, int value) {
  BGNN_REQUIRE(ctx && name, "bgnn_ctx_set_option: NULL argument");
  int *p = option_slot(ctx, name);
  BGNN_REQUIRE(p, "bgnn_ctx_set_option: unknown option '%s'", name);
  if (p == &ctx->opts.matrix_path) BGNN_REQUIRE(value >= 0 && value <= 3, "matrix_path=%d (0 exact f32, 1 bf16x3, 2 fp16x3, 3 bf16 storage)", value);
  if ((p == &ctx->opts.diag_mask || p == &ctx->opts.diag_stamps || p == &ctx->opts.gemm_diag) && value != 0)
    BGNN_REQUIRE(BGNN_DIAG, "option '%s' needs the diagnostic build of the library (python __graft_entry__.py --diag)", name);
  *p = value;
  return BGNN_OK;
}

int bgnn_ctx_get_option(bgnn_ctx *ctx, const char *name, int *value) {
  BGNN_REQUIRE(ctx && name && value, "bgnn_ctx_get_option: NULL argument");
  int *p = option_slot(ctx, name);
  BGNN_REQUIRE(p, "bgnn_ctx_get_option: unknown option '%s'", name);
  *value = *p;
  return BGNN_OK;
}

// diagnostic (not part of the documented ABI): read and clear the fused kernel's phase counters
// (out: 64 counters -- 0..15 the fused layer kernels together, 16..31 unused, 32..47 the 256 -> 64 instance, 48..63 the heads
//  instance)
int bgnn_debug_stamps(bgnn_ctx *ctx, unsigned long long *out32) {
  if (!ctx || !out32) return BGNN_ERR_INVALID;
  (void)hipStreamSynchronize(ctx->stream);
  if (hipMemcpy(out32, ctx->stamps, 512, hipMemcpyDeviceToHost) != hipSuccess) return BGNN_ERR_HIP;
  (void)hipMemset(ctx->stamps, 0, 512);
  return BGNN_OK;
}

int bgnn_ctx_destroy(bgnn_ctx *ctx) {
  if (!ctx) return BGNN_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  // graphs still alive on this context go with it: their handles are invalid from here on (bgnn.h: bgnn_ctx_destroy)
  while (!ctx->live_graphs.empty()) graph_free(*ctx->live_graphs.begin());
  for (auto &r : ctx->prof_records) { (void)hipEventDestroy(r.start); (void)hipEventDestroy(r.stop); }
  for (auto &e : ctx->event_pool) (void)hipEventDestroy(e);
  for (auto &st : ctx->staging) { (void)hipEventDestroy(st.ev); (void)hipHostFree(st.p); }
  for (int i = 0; i < 7; ++i) if (ctx->ws[i]) (void)hipFree(ctx->ws[i]);
  for (auto &e : ctx->table_cache) { (void)hipFree(e.d_tiles); (void)hipFree(e.d_items); }
  if (ctx->zero_page) (void)hipFree(ctx->zero_page);
  ctx->pool.trim();
  for (auto &kv : ctx->pool.live) (void)hipFree(kv.first);
  if (ctx->owns_stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return BGNN_OK;
}

int bgnn_ctx_synchronize(bgnn_ctx *ctx) {
  BGNN_REQUIRE(ctx, "ctx is NULL");
  BGNN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return BGNN_OK;
}

void *bgnn_ctx_stream(bgnn_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int bgnn_ctx_profile(bgnn_ctx *ctx, uint32_t kernel_mask) {
  BGNN_REQUIRE(ctx, "ctx is NULL");
  ctx->prof_mask = kernel_mask;
  return BGNN_OK;
}

int bgnn_ctx_profile_read(bgnn_ctx *ctx, double *ms, int64_t *launches) {
  BGNN_REQUIRE(ctx && ms && launches, "bgnn_ctx_profile_read: NULL argument");
  BGNN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  for (auto &r : ctx->prof_records) {
    float t = 0.f;
    BGNN_HIP_CHECK(hipEventElapsedTime(&t, r.start, r.stop));
    ms[r.kernel] += (double)t;
    launches[r.kernel] += 1;
    ctx->event_pool.push_back(r.start);
    ctx->event_pool.push_back(r.stop);
  }
  ctx->prof_records.clear();
  return BGNN_OK;
}

// ---- forward ----------------------------------------------------------------------------------
struct GridOut {             // optional fused node -> grid outputs (bgnn_infer_tiles)
  float *cls = nullptr, *conf = nullptr, *corr = nullptr;
  float norm_floor = 0.01f;
  bool done = false;         // set when the fused tail wrote the grids
};

// Eval-mode forward: folded BatchNorm statistics, the fused launches where they have an instance, the opt-in matrix paths.
static int forward_infer(bgnn_ctx *ctx, bgnn_model *m, bgnn_graph *g, float thr_auto, float thr_review, const bgnn_outputs *o,
                         GridOut *grids) {
  FwdTables t;
  BGNN_TRY(forward_begin(ctx, m, g, &t));
  if (t.rows <= 0) return BGNN_OK;
  const bgnn_model_desc &d = m->desc;
  const bool gat = d.gnn_type == BGNN_GNN_GAT;
  const int64_t rows = t.rows, *dm = t.dm;
  const int hid = d.hidden;
  float *X = t.X, *Y = t.Y, *asdX = t.asdX, *asdY = t.asdY;
  const bool use_fused = ctx->opts.fused;
  // the node table: 8-column rows, or the wide table of a build with auxiliary planes (bgnn_aux.h).  Kx: rows of fe_W0t.  The
  // forms that read the table inside another kernel (fused front, aggregate-first extractor) know 8-column rows only
  const float *xt = g->d_x;
  const int ldx = g->ldx, Kx = extractor_rows(d.in_channels);
  const bool x8rows = ldx == 8;
  // matrix_path 3 (BASELINE config 3): layer activations xw are stored as bf16 and multiplied on the bf16 MFMA; it exists
  // only on the fused stencil path of the default model shape
  const bool bf16 = ctx->opts.matrix_path == 3;
  if (bf16) {
    BGNN_REQUIRE(gat && use_fused && g->kind == 0 && hid == 64 && d.heads == 4 && d.num_layers >= 2 && g->compact_edges && !o->hidden,
                 "matrix_path = bf16 (bf16 activation storage) runs on the fused stencil path of the default model shape only "
                 "(GAT, hidden 64, heads 4, >= 2 layers, graphs built by bgnn_graph_build)");
  }
  // feature extractor (gnn.py:386): Linear(in,hid) ReLU [Dropout] Linear(hid,hid); then lin of layer 0
  bool layer0_done = false;                           // bf16 path: layer 0's aggregate already ran (aggregate-first launch): the loop starts at layer 1
  const size_t nl_gat = gat ? m->layers.size() : 0;
  if (!gat) {
    // GCN / GraphSAGE / GIN backbones (gnn.py:120-143; torch_geometric default arguments): plain gathers + GEMMs.
    // Not the hot path: no fusion beyond BatchNorm / bias / ReLU folded into the neighbouring kernel.
    BGNN_TRY(launch_gemm_f32(ctx, xt, ldx, m->fe_W0t, m->fe_b0, Y, hid, dm, rows, Kx, hid, 1));
    BGNN_TRY(launch_gemm_f32(ctx, Y, hid, m->fe_W1t, m->fe_b1, X, hid, dm, rows, hid, hid, 0));
    float *dinv = asdX;
    if (d.gnn_type == BGNN_GNN_GCN) BGNN_TRY(launch_degree_inv_sqrt(ctx, g, dinv));
    const size_t nl = m->layers.size();
    // On stencil graphs a layer is ONE launch of the fused layer kernel in its plain-backbone mode -- aggregate ->
    // GEMM -> per-column post-op -- instead of reduce + GEMM launches with h round-tripping through HBM (GIN: its second Linear
    // stays a GEMM launch).  Anything the fused form does not cover falls through to the plain kernels below.
    const bool plain_fused = use_fused && g->kind == 0 && hid == 64;
    for (size_t l = 0; l < nl; ++l) {                 // invariant: X = h_l [rows][hid]
      const BgnnLayer &L = m->layers[l];
      const int relu = l + 1 < nl ? 1 : 0;
      if (plain_fused) {
        int rc = BGNN_ERR_UNSUPPORTED;
        if (d.gnn_type == BGNN_GNN_GCN) rc = launch_fused_plain_layer(ctx, g, 1, hid, X, dinv, L.Wfp, m->ones, L.scale, L.shift, relu, Y);
        else if (d.gnn_type == BGNN_GNN_SAGE) rc = launch_fused_plain_layer(ctx, g, 2, hid, X, nullptr, L.Wfp, m->ones, m->ones, L.b2, relu, Y);
        else rc = launch_fused_plain_layer(ctx, g, 3, hid, X, nullptr, L.Wfp, m->ones, m->ones, L.b1, 1, Y);
        if (rc == BGNN_OK) {
          if (d.gnn_type == BGNN_GNN_GIN) BGNN_TRY(launch_gemm_f32(ctx, Y, hid, L.Wt2, L.b2, X, hid, dm, rows, hid, hid, relu));
          else std::swap(X, Y);
          continue;
        }
        if (rc != BGNN_ERR_UNSUPPORTED) return rc;
      }
      if (d.gnn_type == BGNN_GNN_GCN) {               // lin, normalised aggregate, + bias, BatchNorm, ReLU
        BGNN_TRY(launch_gemm_f32(ctx, X, hid, L.Wt, nullptr, Y, hid, dm, rows, hid, hid, 0));
        BGNN_TRY(launch_neighbor_reduce(ctx, g, 1, Y, hid, dinv, L.scale, L.shift, relu, X, hid, nullptr));
      } else if (d.gnn_type == BGNN_GNN_SAGE) {       // [mean_j x_j | x_i] @ [lin_l ; lin_r]^T (BatchNorm folded) + bias, ReLU
        BGNN_TRY(launch_neighbor_reduce(ctx, g, 2, X, hid, nullptr, nullptr, nullptr, 0, Y, 2 * hid, Y + hid));
        BGNN_TRY(launch_gemm_f32(ctx, Y, 2 * hid, L.Wt, L.b2, X, hid, dm, rows, 2 * hid, hid, relu));
      } else {                                        // GIN: nn(sum_j x_j + x_i), nn = Linear ReLU Linear; BatchNorm; ReLU
        BGNN_TRY(launch_neighbor_reduce(ctx, g, 3, X, hid, nullptr, nullptr, nullptr, 0, Y, hid, nullptr));
        BGNN_TRY(launch_gemm_f32(ctx, Y, hid, L.Wt, L.b1, X, hid, dm, rows, hid, hid, 1));
        BGNN_TRY(launch_gemm_f32(ctx, X, hid, L.Wt2, L.b2, Y, hid, dm, rows, hid, hid, relu));
        std::swap(X, Y);
      }
    }
    std::swap(X, Y);                                  // the tail below expects the backbone output in Y
  } else {
    const BgnnLayer &L0 = m->layers[0];
    if (ctx->opts.fold_extractor) {       // second extractor layer folded into lin_0 (see bgnn_model_create)
      const int sm = ctx->opts.matrix_path;
      const int smode = sm == 3 ? 3 : sm == 2 && m->l0f_Wsp16 ? 2 : sm ? 1 : 0;
      const float *wsplit = sm == 3 ? m->l0f_Wbf : sm == 2 && m->l0f_Wsp16 ? m->l0f_Wsp16 : sm ? m->l0f_Wsp : nullptr;
      // extractor layer 1 runs inside the lin_0 GEMM (same instructions, h1 never leaves the registers) wherever that GEMM takes
      // its W-resident form; below 32 768 rows (exact path) it keeps its own launch -- the results are bit-identical either way
      const bool front = x8rows && hid == 64 && gemm_front_available(ctx, rows, L0.heads * hid, smode);
      BGNN_REQUIRE(x8rows || sm != 3, "matrix_path = bf16 reads 8-column node rows: not for a graph built with auxiliary planes");
      BGNN_REQUIRE(front || sm != 3, "matrix_path = bf16 needs fused_front = 1");
      // bf16 path, default shape: layer 0 aggregates the extractor's h1 and applies lin_0 afterwards, inside the fused launch
      // (gat_layer_bf16_2p_kernel, AF) -- no lin_0 product in HBM, no front GEMM
      if (sm == 3 && front && ctx->opts.bf16_layer0_af && ctx->opts.bf16_two_phase && m->l0af_W && nl_gat >= 2 && use_fused && !o->hidden) {
        const BgnnLayer &L1 = m->layers[1];
        const float *V3a = nullptr;
        if (g->kind == 0 && g->compact_edges && !g->edge_default) { const float *v3; BGNN_TRY(model_canonical_V(m, g, &v3)); V3a = v3; }
        if (L1.heads == 4 && L1.Wbf && g->kind == 0) {
          BGNN_TRY(launch_extractor_af(ctx, g->d_x8, m->fe_W0t, m->fe_b0, m->l0f_Wbf + (size_t)hid * L0.heads * hid / 2, Y, asdX, dm, rows, L0.heads));
          int rc = launch_fused_layer0_af(ctx, g, L0, L1, hid, V3a, Y, asdX, m->l0af_W, m->l0af_shift, X, asdY);
          if (rc == BGNN_OK) { std::swap(asdX, asdY); layer0_done = true; }
          else if (rc != BGNN_ERR_UNSUPPORTED) return rc;
        }
      }
      if (!layer0_done) {
      if (!front) BGNN_TRY(launch_gemm_f32(ctx, xt, ldx, m->fe_W0t, m->fe_b0, Y, hid, dm, rows, Kx, hid, 1));
      BGNN_TRY(launch_gemm_f32(ctx, front ? g->d_x8 : Y, front ? 8 : hid, m->l0f_Wt, m->l0f_b, X, L0.heads * hid, dm, rows, hid,
                               L0.heads * hid, 0, L0.att_src, L0.att_dst, asdX, L0.heads, hid, wsplit, smode,
                               front ? m->fe_W0t : nullptr, front ? m->fe_b0 : nullptr, front && smode == 0 ? m->l0f_Wpm : nullptr,
                               m->l0f_Wt_blk, smode == 2 ? m->l0f_Wsp16_inv : 1.0f));
      }
    } else {
      BGNN_REQUIRE(!bf16, "matrix_path = bf16 needs fold_extractor = 1");
      BGNN_TRY(launch_gemm_f32(ctx, xt, ldx, m->fe_W0t, m->fe_b0, X, hid, dm, rows, Kx, hid, 1));
      BGNN_TRY(launch_gemm_f32(ctx, X, hid, m->fe_W1t, m->fe_b1, Y, hid, dm, rows, hid, hid, 0));
      BGNN_TRY(launch_gemm_f32(ctx, Y, L0.d_in, L0.Wt, nullptr, X, L0.heads * hid, dm, rows, L0.d_in, L0.heads * hid, 0,
                               L0.att_src, L0.att_dst, asdX, L0.heads, hid, nullptr, 0, nullptr, nullptr, nullptr, L0.Wt_blk));
    }
  }
  // GNN backbone (gnn.py:173-188).  Invariant at the top of each iteration: X = lin_l(h_l), asdX = its dots.
  const size_t nl = gat ? m->layers.size() : 0;
  // a graph built with another edge feature list than the default: the fused kernels take the edge vectors over the canonical three
  const float *v3_all = nullptr;
  if (gat && use_fused && g->kind == 0 && g->compact_edges && !g->edge_default) BGNN_TRY(model_canonical_V(m, g, &v3_all));
  for (size_t l = layer0_done ? 1 : 0; l < nl; ++l) {
    const float *V3 = v3_all ? v3_all + l * (size_t)d.heads * 3 : nullptr;
    const BgnnLayer &L = m->layers[l];
    const int relu = L.concat ? 1 : 0;
    if (l + 1 < nl) {
      const BgnnLayer &Ln = m->layers[l + 1];
      int rc = use_fused ? launch_fused_layer_next(ctx, g, L, Ln, hid, V3, X, asdX, Y, asdY) : BGNN_ERR_UNSUPPORTED;
      if (rc == BGNN_OK) { std::swap(X, Y); std::swap(asdX, asdY); continue; }
      if (rc != BGNN_ERR_UNSUPPORTED) return rc;
      BGNN_REQUIRE(!bf16, "matrix_path = bf16: no fused instance for layer %d of this model / graph", (int)l);
      BGNN_TRY(gat_aggregate_unfused(ctx, g, L, hid, d.edge_dim, X, asdX, Y, relu, nullptr));
      BGNN_TRY(launch_gemm_f32(ctx, Y, Ln.d_in, Ln.Wt, nullptr, X, Ln.heads * hid, dm, rows, Ln.d_in, Ln.heads * hid, 0,
                               Ln.att_src, Ln.att_dst, asdX, Ln.heads, hid, nullptr, 0, nullptr, nullptr, nullptr, Ln.Wt_blk));
    } else {
      int rc = use_fused ? launch_fused_layer_heads(ctx, g, m, L, hid, V3, X, asdX, thr_auto, thr_review,
                                                    grids ? grids->norm_floor : 0.01f, o, grids ? grids->cls : nullptr,
                                                    grids ? grids->conf : nullptr, grids ? grids->corr : nullptr)
                         : BGNN_ERR_UNSUPPORTED;
      if (rc == BGNN_OK) { if (grids) grids->done = true; return BGNN_OK; }
      if (rc != BGNN_ERR_UNSUPPORTED) return rc;
      BGNN_REQUIRE(!bf16, "matrix_path = bf16: no fused instance for the last layer of this model / graph");
      BGNN_TRY(gat_aggregate_unfused(ctx, g, L, hid, d.edge_dim, X, asdX, Y, relu, nullptr));
    }
  }
  // heads (gnn.py:392-406)
  BGNN_TRY(forward_heads_hidden(ctx, m, Y, t, o));
  BGNN_TRY(launch_heads_final(ctx, m, t.hidb, m->head_hidden_total, dm, rows, thr_auto, thr_review, o));
  return BGNN_OK;
}

int bgnn_forward(bgnn_ctx *ctx, bgnn_model *m, bgnn_graph *g, float thr_auto, float thr_review, const bgnn_outputs *o) {
  BGNN_REQUIRE(ctx && m && g && o, "bgnn_forward: NULL argument");
  BGNN_REQUIRE(m->ctx == ctx && g->ctx == ctx, "bgnn_forward: model/graph belong to another context");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  BGNN_TRY(model_sync(ctx, m));
  return forward_infer(ctx, m, g, thr_auto, thr_review, o, nullptr);
}

// ---- sub-modules of the model on their own (parity tests against reference-generated fixtures) ----------------
static int row_count_on_device(bgnn_ctx *ctx, int64_t n, int64_t **d_n) {
  void *p;
  BGNN_TRY(ctx_workspace(ctx, 5, 64, &p));
  BGNN_TRY(ctx_upload(ctx, &n, sizeof(n), p));
  *d_n = (int64_t *)p;
  return BGNN_OK;
}

int bgnn_feature_extractor(bgnn_ctx *ctx, bgnn_model *m, const float *x, int64_t n_nodes, float *out) {
  BGNN_REQUIRE(ctx && m && out && (x || n_nodes == 0), "bgnn_feature_extractor: NULL argument");
  BGNN_REQUIRE(m->ctx == ctx, "bgnn_feature_extractor: model belongs to another context");
  BGNN_REQUIRE(n_nodes >= 0 && n_nodes < ((int64_t)1 << 30), "bgnn_feature_extractor: n_nodes=%lld out of range", (long long)n_nodes);
  if (n_nodes == 0) return BGNN_OK;
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  BGNN_TRY(model_sync(ctx, m));
  const int hid = m->desc.hidden, in = m->desc.in_channels, Kx = extractor_rows(in);
  void *px8, *ph;
  BGNN_TRY(ctx_workspace(ctx, 0, (size_t)n_nodes * Kx * sizeof(float), &px8));
  BGNN_TRY(ctx_workspace(ctx, 1, (size_t)n_nodes * hid * sizeof(float), &ph));
  int64_t *dn;
  BGNN_TRY(row_count_on_device(ctx, n_nodes, &dn));
  if (Kx == 8)
    hipLaunchKernelGGL(pad_rows8_kernel, dim3((unsigned)((n_nodes * 8 + 255) / 256)), dim3(256), 0, ctx->stream, x, in,
                       (float *)px8, n_nodes);
  else
    hipLaunchKernelGGL(pad_rows16_kernel, dim3((unsigned)((n_nodes * 16 + 255) / 256)), dim3(256), 0, ctx->stream, x, in,
                       (float *)px8, n_nodes);
  BGNN_HIP_CHECK(hipGetLastError());
  BGNN_TRY(launch_gemm_f32(ctx, (const float *)px8, Kx, m->fe_W0t, m->fe_b0, (float *)ph, hid, dn, n_nodes, Kx, hid, 1));
  if (!m->padded) return launch_gemm_f32(ctx, (const float *)ph, hid, m->fe_W1t, m->fe_b1, out, hid, dn, n_nodes, hid, hid, 0);
  void *po;                                               // padded width: out is [n][logical hidden]
  BGNN_TRY(ctx_workspace(ctx, 2, (size_t)n_nodes * hid * sizeof(float), &po));
  BGNN_TRY(launch_gemm_f32(ctx, (const float *)ph, hid, m->fe_W1t, m->fe_b1, (float *)po, hid, dn, n_nodes, hid, hid, 0));
  BGNN_TRY(launch_copy_cols(ctx, (const float *)po, hid, out, m->logical_hidden, m->logical_hidden, dn, n_nodes));
  return BGNN_OK;
}

int bgnn_heads(bgnn_ctx *ctx, bgnn_model *m, const float *hidden, int64_t n_nodes, float thr_auto, float thr_review,
               const bgnn_outputs *o) {
  BGNN_REQUIRE(ctx && m && o && (hidden || n_nodes == 0), "bgnn_heads: NULL argument");
  BGNN_REQUIRE(m->ctx == ctx, "bgnn_heads: model belongs to another context");
  BGNN_REQUIRE(n_nodes >= 0 && n_nodes < ((int64_t)1 << 30), "bgnn_heads: n_nodes=%lld out of range", (long long)n_nodes);
  BGNN_REQUIRE(!o->hidden, "bgnn_heads: `hidden` is this call's input");
  if (n_nodes == 0) return BGNN_OK;
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  BGNN_TRY(model_sync(ctx, m));
  const int hid = m->desc.hidden;
  void *phid;
  BGNN_TRY(ctx_workspace(ctx, 3, (size_t)n_nodes * m->head_hidden_total * sizeof(float), &phid));
  int64_t *dn;
  BGNN_TRY(row_count_on_device(ctx, n_nodes, &dn));
  if (m->padded) {                                        // hidden is [n][logical hidden]: widen it with zero columns
    void *pw;
    BGNN_TRY(ctx_workspace(ctx, 1, (size_t)n_nodes * hid * sizeof(float), &pw));
    BGNN_TRY(launch_copy_cols(ctx, hidden, m->logical_hidden, (float *)pw, hid, m->logical_hidden, dn, n_nodes));
    hidden = (const float *)pw;
  }
  BGNN_TRY(launch_gemm_f32(ctx, hidden, hid, m->hd_W0t, m->hd_b0, (float *)phid, m->head_hidden_total, dn, n_nodes, hid,
                           m->head_hidden_total, 1));
  BGNN_TRY(launch_heads_final(ctx, m, (const float *)phid, m->head_hidden_total, dn, n_nodes, thr_auto, thr_review, o));
  return BGNN_OK;
}

int bgnn_infer_tiles(bgnn_ctx *ctx, bgnn_model *m, const bgnn_tiles *tiles, const bgnn_graph_opts *opts, float thr_auto,
                     float thr_review, float norm_floor, float *classification, float *confidence, float *correction,
                     int64_t *n_nodes_out) {
  return infer_tiles(ctx, m, tiles, opts, 0, nullptr, thr_auto, thr_review, norm_floor, classification, confidence, correction,
                     n_nodes_out);
}

}  // extern "C"

// bgnn_infer_tiles, and bgnn_infer_tiles_aux (node_aux.hip) with its planes
int bgnn::infer_tiles(bgnn_ctx *ctx, bgnn_model *m, const bgnn_tiles *tiles, const bgnn_graph_opts *opts, int32_t n_aux,
                      const float *const *aux, float thr_auto, float thr_review, float norm_floor, float *classification,
                      float *confidence, float *correction, int64_t *n_nodes_out) {
  BGNN_REQUIRE(ctx && m && tiles && opts, "bgnn_infer_tiles: NULL argument");
  BGNN_REQUIRE(m->ctx == ctx, "bgnn_infer_tiles: model belongs to another context");
  BGNN_TRY(model_sync(ctx, m));
  bgnn_graph *g = nullptr;
  float *const grids[3] = {classification, confidence, correction};
  // (the compaction scan writes the node count there itself; a ragged batch's canvas fill zero-fills the result grids on its way)
  BGNN_TRY(graph_build(ctx, tiles, opts, &g, n_nodes_out, grids, n_aux, aux));
  const int64_t rows = g->row_capacity;
  GridOut go;
  go.cls = classification; go.conf = confidence; go.corr = correction; go.norm_floor = norm_floor;
  // first try the fully fused tail (no per-node outputs at all); otherwise per-node outputs + K6
  void *p;
  int rc = ctx_workspace(ctx, 4, (size_t)rows * (sizeof(int64_t) + 2 * sizeof(float)), &p);
  if (rc == BGNN_OK) {
    bgnn_outputs none{};
    bgnn_outputs o{};
    o.predicted_class = (int64_t *)p;
    o.confidence = (float *)(o.predicted_class + rows);
    o.correction = m->desc.predict_correction ? o.confidence + rows : nullptr;
    const bool try_fused = fused_heads_available(ctx, g, m);
    if (try_fused && g->d_atlas && !g->grids_cleared) {   // the canvas walk writes valid cells only: clear the grids (fill 0.0) first
      const size_t nb = (size_t)g->total_cells * sizeof(float);
      if (classification && confidence == classification + g->total_cells && correction == confidence + g->total_cells) {
        BGNN_HIP_CHECK(hipMemsetAsync(classification, 0, 3 * nb, ctx->stream));      // one [3, cells] block: one fill
      } else {
        if (classification) BGNN_HIP_CHECK(hipMemsetAsync(classification, 0, nb, ctx->stream));
        if (confidence) BGNN_HIP_CHECK(hipMemsetAsync(confidence, 0, nb, ctx->stream));
        if (correction) BGNN_HIP_CHECK(hipMemsetAsync(correction, 0, nb, ctx->stream));
      }
    }
    rc = forward_infer(ctx, m, g, thr_auto, thr_review, try_fused ? &none : &o, &go);
    if (rc == BGNN_OK && !go.done) {
      if (try_fused) rc = forward_infer(ctx, m, g, thr_auto, thr_review, &o, nullptr);   // (not reached in practice)
      if (rc == BGNN_OK)
        rc = launch_results_to_grids(g, o.predicted_class, o.confidence, o.correction, norm_floor, classification,
                                     confidence, correction);
    }
  }
  graph_free(g);   // buffers return to the pool; stream order keeps them valid for the work already queued
  return rc;
}

