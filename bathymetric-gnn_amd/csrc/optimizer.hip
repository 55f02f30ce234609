// The optimizer part of the C ABI (include/bgnn_optim.h): gradient clipping + AdamW over the flat weight blob, and the refresh of a
// live packed model from that blob.  Latency-bound kernels over <= 1 M elements: plain, one element per thread.
// Compiled with -ffp-contract=off: the refresh's float64 dot products restate the host packer's (model_images.h fill_images)
// operation by operation, and the step's sums have one fixed order.
#include <algorithm>
#include <cmath>

#include "bgnn_internal.h"
#include "plane_util.h"

using namespace bgnn;

namespace {

constexpr int kBlock = BLOCK_THREADS;

struct AdamChunk { uint64_t offset; uint32_t count, slot; };        // <= BGNN_ADAMW_CHUNK elements of one slot
struct AdamSlot { double step_size, bc2_sqrt; };                    // lr / (1 - beta1^t), sqrt(1 - beta2^t)

// fixed tree over the block's 256 running sums (no leading barrier: each kernel calls it once, on scratch nobody has read)
__device__ inline double block_sum_fixed(double s, double *sh) { return block_reduce<false>(s, sh, SumOp()); }

// partial[c] = sum of g^2 over chunk c: thread t takes elements t, t + 256, ... in order, then the tree
__global__ void __launch_bounds__(kBlock) adamw_sumsq_kernel(const float *g, const AdamChunk *chunks, double *partial) {
  __shared__ double sh[kBlock];
  const AdamChunk c = chunks[blockIdx.x];
  double s = 0.0;
  for (uint32_t i = threadIdx.x; i < c.count; i += kBlock) { const double v = (double)g[c.offset + i]; s += v * v; }
  s = block_sum_fixed(s, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one workgroup: thread t sums partials t, t + 256, ... in order, then the tree.  scal[0] = the clip coefficient
__global__ void __launch_bounds__(kBlock) adamw_norm_kernel(const double *partial, int n, double max_norm, int clip, double *scal,
                                                            float *grad_norm) {
  __shared__ double sh[kBlock];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kBlock) s += partial[i];
  s = block_sum_fixed(s, sh);
  if (threadIdx.x == 0) {
    const double norm = sqrt(s);
    double coef = 1.0;
    if (clip) { coef = max_norm / (norm + 1e-6); coef = coef > 1.0 ? 1.0 : coef; }     // (NaN stays NaN, as torch.clamp keeps it)
    scal[0] = coef;
    if (grad_norm) *grad_norm = (float)norm;
  }
}

__global__ void __launch_bounds__(kBlock) adamw_update_kernel(float *w, const float *g, float *m1, float *m2, const AdamChunk *chunks,
                                                              const AdamSlot *slots, const double *scal, int clip, double lr_wd,
                                                              double beta1, double beta2, double eps) {
  const AdamChunk c = chunks[blockIdx.x];
  const AdamSlot sl = slots[c.slot];
  const double coef = scal[0];
  for (uint32_t i = threadIdx.x; i < c.count; i += kBlock) {
    const uint64_t k = c.offset + i;
    double gr = (double)g[k];
    if (clip) gr *= coef;
    double p = (double)w[k];
    p *= 1.0 - lr_wd;                                               // decoupled weight decay
    double m = (double)m1[k], v = (double)m2[k];
    m = m + (gr - m) * (1.0 - beta1);
    v = v * beta2 + (1.0 - beta2) * (gr * gr);
    const double denom = sqrt(v) / sl.bc2_sqrt + eps;
    p -= sl.step_size * (m / denom);
    w[k] = (float)p; m1[k] = (float)m; m2[k] = (float)v;
  }
}

// ---- refresh ---------------------------------------------------------------------------------------------------------------
__global__ void refresh_gather_kernel(const int32_t *pairs, int n, float *dst, const float *src) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[pairs[2 * i]] = src[pairs[2 * i + 1]];
}

// The float64 dot products of the host packer, k ascending: the folded layer-0 weight [hid][HC0] and bias [HC0], then the edge
// vectors V (one job each)
__global__ void refresh_fold_kernel(RefreshTables T, int hid, int ED, float *blob, const float *w) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int HC0 = T.fold_cols, n_w = hid * HC0, n_fold = n_w + HC0;
  if (idx < n_w) {
    const int i = idx / HC0, o = idx - i * HC0;
    double s = 0.0;
    for (int k = 0; k < hid; ++k) s += (double)w[T.fe_W1 + k * hid + i] * (double)w[T.W0 + o * hid + k];
    blob[T.l0f_Wt + idx] = (float)s;
  } else if (idx < n_fold) {
    const int o = idx - n_w;
    double s = 0.0;
    for (int k = 0; k < hid; ++k) s += (double)w[T.fe_b1 + k] * (double)w[T.W0 + o * hid + k];
    blob[T.l0f_b + o] = (float)s;
  } else if (idx - n_fold < T.n_vjob) {
    const int32_t *j = T.d_vjob + 4 * (idx - n_fold);
    double s = 0.0;
    for (int c = 0; c < hid; ++c) s += (double)w[j[1] + c] * (double)w[j[2] + c * ED];
    blob[j[0]] = (float)s;
  }
}

}  // namespace

extern "C" {

int bgnn_adamw_step(bgnn_ctx *ctx, float *weights, const float *grads, float *exp_avg, float *exp_avg_sq, size_t n_weights,
                    const bgnn_adamw_slot *slots, int32_t n_slots, const bgnn_adamw_params *p, float *grad_norm) {
  BGNN_REQUIRE(ctx && weights && grads && exp_avg && exp_avg_sq && p && (slots || n_slots == 0), "bgnn_adamw_step: NULL argument");
  BGNN_REQUIRE(n_slots >= 0 && n_slots <= (1 << 20), "bgnn_adamw_step: n_slots=%d out of range", n_slots);
  BGNN_REQUIRE(p->lr >= 0.0 && p->eps >= 0.0 && p->weight_decay >= 0.0 && p->beta1 >= 0.0 && p->beta1 < 1.0 && p->beta2 >= 0.0 &&
               p->beta2 < 1.0, "bgnn_adamw_step: lr=%g betas=(%g, %g) eps=%g weight_decay=%g: invalid (torch.optim.AdamW's ranges)",
               p->lr, p->beta1, p->beta2, p->eps, p->weight_decay);
  BGNN_REQUIRE(!std::isnan(p->max_norm), "bgnn_adamw_step: max_norm is NaN");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const int clip = p->max_norm > 0.0 && !std::isinf(p->max_norm) ? 1 : 0;
  std::vector<AdamChunk> chunks;
  std::vector<AdamSlot> sl((size_t)std::max(n_slots, 1));
  std::vector<std::pair<uint64_t, uint64_t>> spans;
  for (int32_t s = 0; s < n_slots; ++s) {
    const bgnn_adamw_slot &S = slots[s];
    BGNN_REQUIRE(S.offset <= n_weights && S.count <= n_weights - S.offset, "bgnn_adamw_step: slot %d (%llu floats at %llu) leaves the "
                 "blob of %zu", s, (unsigned long long)S.count, (unsigned long long)S.offset, n_weights);
    BGNN_REQUIRE(S.step >= 1, "bgnn_adamw_step: slot %d has step=%lld (the count including this step: >= 1)", s, (long long)S.step);
    const double bc1 = 1.0 - std::pow(p->beta1, (double)S.step), bc2 = 1.0 - std::pow(p->beta2, (double)S.step);
    sl[s].step_size = p->lr / bc1; sl[s].bc2_sqrt = std::sqrt(bc2);
    if (S.count) spans.emplace_back(S.offset, S.count);
    for (uint64_t o = 0; o < S.count; o += BGNN_ADAMW_CHUNK)
      chunks.push_back(AdamChunk{S.offset + o, (uint32_t)std::min<uint64_t>(BGNN_ADAMW_CHUNK, S.count - o), (uint32_t)s});
  }
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i)
    BGNN_REQUIRE(spans[i - 1].first + spans[i - 1].second <= spans[i].first, "bgnn_adamw_step: slots overlap at float %llu",
                 (unsigned long long)spans[i].first);
  if (chunks.empty()) {                                  // nothing has a gradient: torch's norm of no tensors is 0
    if (grad_norm) BGNN_HIP_CHECK(hipMemsetAsync(grad_norm, 0, sizeof(float), ctx->stream));
    return BGNN_OK;
  }
  const size_t nc = chunks.size();
  // one pool block: scal [2] | partial [nc] (float64) | slot table | chunk table
  const size_t o_part = 16, o_slot = o_part + nc * sizeof(double), o_chunk = o_slot + sl.size() * sizeof(AdamSlot);
  const size_t bytes = o_chunk + nc * sizeof(AdamChunk);
  void *ws = nullptr;
  BGNN_TRY(ctx->pool.alloc(bytes, &ws));
  char *wb = (char *)ws;
  double *scal = (double *)wb, *partial = (double *)(wb + o_part);
  AdamSlot *d_slot = (AdamSlot *)(wb + o_slot);
  AdamChunk *d_chunk = (AdamChunk *)(wb + o_chunk);
  int rc = ctx_upload(ctx, sl.data(), sl.size() * sizeof(AdamSlot), d_slot);
  if (rc == BGNN_OK) rc = ctx_upload(ctx, chunks.data(), nc * sizeof(AdamChunk), d_chunk);
  if (rc == BGNN_OK) {
    hipLaunchKernelGGL(adamw_sumsq_kernel, dim3((unsigned)nc), dim3(kBlock), 0, ctx->stream, grads, d_chunk, partial);
    hipLaunchKernelGGL(adamw_norm_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, partial, (int)nc, p->max_norm, clip, scal, grad_norm);
    hipLaunchKernelGGL(adamw_update_kernel, dim3((unsigned)nc), dim3(kBlock), 0, ctx->stream, weights, grads, exp_avg, exp_avg_sq, d_chunk,
                       d_slot, scal, clip, p->lr * p->weight_decay, p->beta1, p->beta2, p->eps);
    if (hipGetLastError() != hipSuccess) { set_error("bgnn_adamw_step: kernel launch failed"); rc = BGNN_ERR_HIP; }
  }
  ctx->pool.release(ws);      // (stream order keeps the block valid for the work already queued)
  return rc;
}

int bgnn_model_refresh_prepare(bgnn_ctx *ctx, bgnn_model *m) {
  BGNN_REQUIRE(ctx && m, "bgnn_model_refresh_prepare: NULL argument");
  BGNN_REQUIRE(m->ctx == ctx, "bgnn_model_refresh: model belongs to another context");
  if (m->padded) {
    set_error("bgnn_model_refresh: hidden_channels=%d / heads=%d run zero-padded to %d / %d; a model is refreshed in place (and trained) "
              "at hidden 32 / 64 / 128 and power-of-two head counts only", m->logical_hidden, m->logical_heads, m->desc.hidden, m->desc.heads);
    return BGNN_ERR_UNSUPPORTED;
  }
  return model_refresh_tables(ctx, m);
}

int bgnn_model_refresh(bgnn_ctx *ctx, bgnn_model *m, const float *weights, size_t n_weights, int32_t what) {
  BGNN_REQUIRE(ctx && m && weights, "bgnn_model_refresh: NULL argument");
  BGNN_REQUIRE(what == BGNN_REFRESH_ALL || what == BGNN_REFRESH_STATS, "bgnn_model_refresh: what=%d unknown", what);
  BGNN_TRY(bgnn_model_refresh_prepare(ctx, m));
  BGNN_REQUIRE(n_weights == m->weights.total, "bgnn_model_refresh: weight blob has %zu floats, expected %zu", n_weights, m->weights.total);
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const RefreshTables &T = *m->refresh;
  BGNN_HIP_CHECK(hipMemcpyAsync(m->raw, weights, n_weights * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  m->eval_stale = true;
  if (what == BGNN_REFRESH_STATS) return BGNN_OK;
  const int hid = m->desc.hidden, ED = m->desc.edge_dim;
  if (T.n_copy)
    hipLaunchKernelGGL(refresh_gather_kernel, dim3((unsigned)((T.n_copy + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, T.d_copy,
                       T.n_copy, m->blob, weights);
  const int n_fold = T.fold_cols * (hid + 1) + T.n_vjob;
  if (n_fold)
    hipLaunchKernelGGL(refresh_fold_kernel, dim3((unsigned)((n_fold + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, T, hid, ED,
                       m->blob, weights);
  if (T.n_relay)
    hipLaunchKernelGGL(refresh_gather_kernel, dim3((unsigned)((T.n_relay + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, T.d_relay,
                       T.n_relay, m->blob, (const float *)m->blob);
  BGNN_HIP_CHECK(hipGetLastError());
  // (h_V and the cached tables of V over the canonical edge attributes now lag behind; only the eval forward reads them, and
  //  model_sync drops and rebuilds them before it does)
  return BGNN_OK;
}

}  // extern "C"
