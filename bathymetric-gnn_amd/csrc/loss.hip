// The multi-task training loss on the device (include/bgnn_loss.h): BathymetricGNNLoss of the reference (training/losses.py) and
// its gradient with respect to class_logits, confidence and correction.  tests/_loss_cpu.py is the same in numpy.
//
// Three kernels, every float sum in float64 in an order that depends on n alone (no float atomics):
//   loss_nodes     LOSS_ROWS_PER_THREAD rows per thread, 256 threads: the five per-node sums (weighted NLL, smoothing sum, W, Huber,
//                  BCE) go through a shuffle tree, the four waves in order through LDS, one partial per workgroup; the counts
//                  (confusion matrix, M, false positives, ...) through an LDS histogram of integer atomics, one bin-major column per workgroup
//   loss_finish    one workgroup: thread t adds partials t, t + 256, ... then the same tree; one wave per count bin; forms the six
//                  terms and the sums
//   loss_backward  one thread per LOSS_ROWS_PER_THREAD rows: recomputes the softmax, writes the three gradients
// The pass reads about 41 B per node; the double exp / log per node stay far below the time those bytes take.
#include "bgnn_internal.h"
#include "../../include/bgnn_loss.h"

#include <math.h>

namespace bgnn {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_RPT = BGNN_LOSS_ROWS_PER_THREAD;
constexpr int LOSS_ROWS_WG = BGNN_LOSS_ROWS_PER_WG;
constexpr int LOSS_MAXC = BGNN_LOSS_MAX_CLASSES;
constexpr int LOSS_NF = 5;                                                   // float sums of the per-node pass
constexpr int LOSS_F_STRIDE = 8;                                             // doubles per workgroup partial
constexpr int LOSS_BINS_STRIDE = LOSS_MAXC * LOSS_MAXC + 8;                  // int32 per workgroup partial
constexpr size_t LOSS_HEAD = 64;                                             // the sums, at the start of the workspace
static_assert(LOSS_ROWS_WG == LOSS_THREADS * LOSS_RPT && BGNN_LOSS_FINISH_WIDTH == LOSS_THREADS, "launch geometry");
static_assert(BGNN_LOSS_N_COUNTS <= 8 && BGNN_LOSS_N_SUMS * sizeof(double) <= LOSS_HEAD, "partial layout");

enum { LF_NLL = 0, LF_SMOOTH = 1, LF_W = 2, LF_HUBER = 3, LF_BCE = 4 };

struct LossArgs {
  bgnn_loss_params prm;
  bgnn_loss_inputs in;
  int64_t n;
  int32_t nwg;
  double *sums;       // [BGNN_LOSS_N_SUMS]
  double *pf;         // [nwg][LOSS_F_STRIDE]
  int32_t *pi;        // [bins][nwg]: bin-major, so that the finish reads a bin's partials contiguously
  float *terms;
  int64_t *counts;
};

// sum of v[k] over the workgroup's 256 threads, k < LOSS_NF: shuffle tree in the wave, then the waves in index order.  The results
// are in sh[0 .. LOSS_NF) for every thread after the call.  sh: LOSS_NF * (waves + 1) doubles.
__device__ __forceinline__ void block_sum5(double (&v)[LOSS_NF], double *sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < LOSS_NF; ++k) {
    double x = v[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if (lane == 0) sh[LOSS_NF + wave * LOSS_NF + k] = x;
  }
  __syncthreads();
  if (threadIdx.x < LOSS_NF) {
    double s = 0.0;
    for (int w = 0; w < LOSS_THREADS / 64; ++w) s += sh[LOSS_NF + w * LOSS_NF + threadIdx.x];
    sh[threadIdx.x] = s;
  }
  __syncthreads();
}

// log-softmax of one row in double: x[c] becomes logits - logsumexp; returns nothing else
__device__ __forceinline__ void row_log_softmax(const float *row, int C, double (&lp)[LOSS_MAXC]) {
  double m = -INFINITY;
#pragma unroll
  for (int c = 0; c < LOSS_MAXC; ++c)
    if (c < C) {
      lp[c] = (double)row[c];
      m = lp[c] > m ? lp[c] : m;
    }
  double se = 0.0;
#pragma unroll
  for (int c = 0; c < LOSS_MAXC; ++c)
    if (c < C) se += exp(lp[c] - m);
  const double lse = m + log(se);
#pragma unroll
  for (int c = 0; c < LOSS_MAXC; ++c)
    if (c < C) lp[c] -= lse;
}

__device__ __forceinline__ double class_weight(const bgnn_loss_params &p, int c) { return p.has_class_weights ? p.class_weights[c] : 1.0; }

__global__ __launch_bounds__(LOSS_THREADS) void loss_nodes(const LossArgs a) {
  __shared__ int32_t hist[LOSS_BINS_STRIDE];
  __shared__ double sh[LOSS_NF * (LOSS_THREADS / 64 + 1)];
  const int C = a.prm.num_classes;
  const int bins = C * C + BGNN_LOSS_N_COUNTS;
  for (int b = threadIdx.x; b < bins; b += LOSS_THREADS) hist[b] = 0;
  __syncthreads();
  int32_t *cnt = hist + C * C;
  const bool has_corr = a.in.correction && a.in.correction_targets;
  double v[LOSS_NF] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const int64_t base = (int64_t)blockIdx.x * LOSS_ROWS_WG + threadIdx.x;
  for (int r = 0; r < LOSS_RPT; ++r) {
    const int64_t i = base + (int64_t)r * LOSS_THREADS;
    if (i >= a.n) break;
    const int64_t y = a.in.labels[i], q = a.in.predicted_class[i];
    const bool y_ok = y >= 0 && y < C;
    if (y == BGNN_LOSS_IGNORE_INDEX) atomicAdd(&cnt[BGNN_LOSS_COUNT_IGNORED], 1);
    else if (!y_ok) atomicAdd(&cnt[BGNN_LOSS_COUNT_INVALID], 1);
    if (y_ok) {
      double lp[LOSS_MAXC];
      row_log_softmax(a.in.logits + i * C, C, lp);
      double sm = 0.0, wy = 1.0, lpy = 0.0;
#pragma unroll
      for (int c = 0; c < LOSS_MAXC; ++c)
        if (c < C) {
          const double w = class_weight(a.prm, c);
          sm -= w * lp[c];
          if (c == (int)y) { wy = w; lpy = lp[c]; }
        }
      v[LF_NLL] -= wy * lpy;
      v[LF_SMOOTH] += sm;
      v[LF_W] += wy;
      if (q >= 0 && q < C) atomicAdd(&hist[(int)y * C + (int)q], 1);
    }
    // confidence: binary cross-entropy against (predicted == label), both logarithms clamped below at -100
    {
      const double x = (double)a.in.confidence[i];
      double l1 = log(x), l0 = log1p(-x);
      l1 = l1 < -100.0 ? -100.0 : l1;
      l0 = l0 < -100.0 ? -100.0 : l0;
      v[LF_BCE] -= (q == y) ? l1 : l0;
    }
    if (has_corr && (!a.in.noise_mask || a.in.noise_mask[i])) {
      const double d = (double)a.in.correction[i] - (double)a.in.correction_targets[i], ad = fabs(d);
      v[LF_HUBER] += ad < a.prm.delta ? 0.5 * d * d : a.prm.delta * (ad - 0.5 * a.prm.delta);
      atomicAdd(&cnt[BGNN_LOSS_COUNT_MASKED], 1);
    }
    if (y == a.prm.feature_class && q == a.prm.feature_noise_class) atomicAdd(&cnt[BGNN_LOSS_COUNT_FEATURE_AS_NOISE], 1);
    if (y == a.prm.seafloor_class && q == a.prm.shoal_noise_class) {
      atomicAdd(&cnt[BGNN_LOSS_COUNT_FALSE_POSITIVES], 1);
      if (a.in.correction_targets)
        atomicAdd(&cnt[a.in.correction_targets[i] < 0.0f ? BGNN_LOSS_COUNT_SHOAL : BGNN_LOSS_COUNT_DEEP], 1);
    }
  }
  block_sum5(v, sh);
  if (threadIdx.x < LOSS_NF) a.pf[(size_t)blockIdx.x * LOSS_F_STRIDE + threadIdx.x] = sh[threadIdx.x];
  for (int b = threadIdx.x; b < bins; b += LOSS_THREADS) a.pi[(size_t)b * a.nwg + blockIdx.x] = hist[b];
}

__global__ __launch_bounds__(LOSS_THREADS) void loss_finish(const LossArgs a) {
  __shared__ long long tot[LOSS_BINS_STRIDE];
  __shared__ double sh[LOSS_NF * (LOSS_THREADS / 64 + 1)];
  __shared__ double out_terms[6], out_sums[BGNN_LOSS_N_SUMS];
  const int C = a.prm.num_classes;
  const int bins = C * C + BGNN_LOSS_N_COUNTS;
  double v[LOSS_NF] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int j = threadIdx.x; j < a.nwg; j += LOSS_THREADS) {
#pragma unroll
    for (int k = 0; k < LOSS_NF; ++k) v[k] += a.pf[(size_t)j * LOSS_F_STRIDE + k];
  }
  // the counts: one wave per bin, the lanes over the workgroups' partials (contiguous per bin), a shuffle tree
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = wave; b < bins; b += LOSS_THREADS / 64) {
    long long c = 0;
#pragma unroll 8
    for (int j = lane; j < a.nwg; j += 64) c += a.pi[(size_t)b * a.nwg + j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if (lane == 0) tot[b] = c;
  }
  block_sum5(v, sh);          // its barriers also order the stores to tot before the reads below
  for (int b = threadIdx.x; b < bins; b += LOSS_THREADS) a.counts[b] = (int64_t)tot[b];
  if (threadIdx.x == 0) {
    const bgnn_loss_params &p = a.prm;
    const long long *cnt = tot + C * C;
    const double N = (double)a.n, M = (double)cnt[BGNN_LOSS_COUNT_MASKED], FP = (double)cnt[BGNN_LOSS_COUNT_FALSE_POSITIVES];
    const double W = sh[LF_W];
    double t[6];
    t[BGNN_LOSS_CLASSIFICATION] = cnt[BGNN_LOSS_COUNT_INVALID]
                                      ? (double)NAN
                                      : ((1.0 - p.label_smoothing) * sh[LF_NLL] + (p.label_smoothing / (double)C) * sh[LF_SMOOTH]) / W;
    t[BGNN_LOSS_CORRECTION] = cnt[BGNN_LOSS_COUNT_MASKED] ? sh[LF_HUBER] / M : 0.0;
    t[BGNN_LOSS_CONFIDENCE] = sh[LF_BCE] / N;
    t[BGNN_LOSS_FEATURE_PRESERVATION] = p.penalty_weight * (double)cnt[BGNN_LOSS_COUNT_FEATURE_AS_NOISE] / N;
    t[BGNN_LOSS_SHOAL_SAFETY] =
        (cnt[BGNN_LOSS_COUNT_FALSE_POSITIVES] && a.in.correction_targets)
            ? (p.shoal_penalty * (double)cnt[BGNN_LOSS_COUNT_SHOAL] + p.deep_penalty * (double)cnt[BGNN_LOSS_COUNT_DEEP]) / FP
            : 0.0;
    double total = 0.0;
    for (int k = 0; k < 5; ++k) total += p.term_weights[k] * t[k];
    t[BGNN_LOSS_TOTAL] = total;
    for (int k = 0; k < 6; ++k) out_terms[k] = t[k];
    double sw = 0.0;
    for (int c = 0; c < C; ++c) sw += class_weight(p, c);
    out_sums[BGNN_LOSS_SUM_W] = W;
    out_sums[BGNN_LOSS_SUM_M] = M;
    out_sums[BGNN_LOSS_SUM_N] = N;
    out_sums[BGNN_LOSS_SUM_WEIGHTS] = sw;
  }
  __syncthreads();
  // one lane per scalar: per-lane addresses, so these are ordinary vector stores
  if (threadIdx.x < 6) a.terms[threadIdx.x] = (float)out_terms[threadIdx.x];
  if (threadIdx.x < BGNN_LOSS_N_SUMS) a.sums[threadIdx.x] = out_sums[threadIdx.x];
}

struct LossBwdArgs {
  bgnn_loss_params prm;
  bgnn_loss_inputs in;
  int64_t n;
  const double *sums;
  const float *upstream;
  float *g_logits, *g_conf, *g_corr;
};

__global__ __launch_bounds__(LOSS_THREADS) void loss_backward(const LossBwdArgs a) {
  const int C = a.prm.num_classes;
  const double W = a.sums[BGNN_LOSS_SUM_W], M = a.sums[BGNN_LOSS_SUM_M], N = a.sums[BGNN_LOSS_SUM_N], SW = a.sums[BGNN_LOSS_SUM_WEIGHTS];
  const double u_cls = (double)a.upstream[0], u_conf = (double)a.upstream[1], u_corr = (double)a.upstream[2];
  const double eps = a.prm.label_smoothing, hard = 1.0 - eps, soft = eps / (double)C;
  const bool has_corr = a.in.correction && a.in.correction_targets;
  const double bce_floor = (double)1e-12f;          // torch's clamp constant, rounded to float32 as torch rounds it
  const int64_t base = (int64_t)blockIdx.x * LOSS_ROWS_WG + threadIdx.x;
  for (int r = 0; r < LOSS_RPT; ++r) {
    const int64_t i = base + (int64_t)r * LOSS_THREADS;
    if (i >= a.n) break;
    const int64_t y = a.in.labels[i];
    if (a.g_logits) {
      float *g = a.g_logits + i * C;
      if (y >= 0 && y < C) {
        double lp[LOSS_MAXC];
        row_log_softmax(a.in.logits + i * C, C, lp);
        const double wy = class_weight(a.prm, (int)y);
#pragma unroll
        for (int c = 0; c < LOSS_MAXC; ++c)
          if (c < C) {
            const double p = exp(lp[c]);
            const double d = hard * wy * (p - (c == (int)y ? 1.0 : 0.0)) + soft * (p * SW - class_weight(a.prm, c));
            g[c] = (float)(u_cls * (d / W));
          }
      } else {
        const float fill = y == BGNN_LOSS_IGNORE_INDEX ? 0.0f : NAN;
        for (int c = 0; c < C; ++c) g[c] = fill;
      }
    }
    if (a.g_conf) {
      const double x = (double)a.in.confidence[i], t = a.in.predicted_class[i] == y ? 1.0 : 0.0;
      double den = (1.0 - x) * x;
      den = den > bce_floor ? den : bce_floor;
      a.g_conf[i] = (float)(u_conf * ((x - t) / den / N));
    }
    if (a.g_corr) {
      double gc = 0.0;
      if (has_corr && (!a.in.noise_mask || a.in.noise_mask[i])) {
        const double d = (double)a.in.correction[i] - (double)a.in.correction_targets[i];
        const double h = fabs(d) < a.prm.delta ? d : (d > 0.0 ? a.prm.delta : (d < 0.0 ? -a.prm.delta : d));
        gc = u_corr * (h / M);
      }
      a.g_corr[i] = (float)gc;
    }
  }
}

static int loss_check(const char *fn, const bgnn_loss_params *p, int64_t n, const bgnn_loss_inputs *in) {
  BGNN_REQUIRE(p && in, "%s: NULL argument", fn);
  BGNN_REQUIRE(n >= 1, "%s: n = %lld", fn, (long long)n);
  if (n > BGNN_LOSS_MAX_ROWS) {
    set_error("%s: %lld rows, at most %lld are supported", fn, (long long)n, (long long)BGNN_LOSS_MAX_ROWS);
    return BGNN_ERR_UNSUPPORTED;
  }
  BGNN_REQUIRE(p->num_classes >= 2 && p->num_classes <= BGNN_LOSS_MAX_CLASSES, "%s: %d classes (2 .. %d)", fn, p->num_classes,
               BGNN_LOSS_MAX_CLASSES);
  BGNN_REQUIRE(p->delta > 0.0, "%s: delta must be positive", fn);
  BGNN_REQUIRE(in->logits && in->confidence && in->predicted_class && in->labels, "%s: NULL input", fn);
  return BGNN_OK;
}

static inline int32_t loss_workgroups(int64_t n) { return (int32_t)((n + LOSS_ROWS_WG - 1) / LOSS_ROWS_WG); }

}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_loss_workspace_bytes(int64_t n) {
  if (n < 1 || n > BGNN_LOSS_MAX_ROWS) return 0;
  const size_t nwg = (size_t)loss_workgroups(n);
  const size_t bytes = LOSS_HEAD + nwg * LOSS_F_STRIDE * sizeof(double) + nwg * LOSS_BINS_STRIDE * sizeof(int32_t);
  return (bytes + 255) / 256 * 256;
}

extern "C" int bgnn_loss_forward(bgnn_ctx *ctx, const bgnn_loss_params *params, int64_t n, const bgnn_loss_inputs *inputs,
                                 void *workspace, size_t workspace_bytes, float *terms, int64_t *counts) {
  BGNN_REQUIRE(ctx && workspace && terms && counts, "bgnn_loss_forward: NULL argument");
  BGNN_TRY(loss_check("bgnn_loss_forward", params, n, inputs));
  const size_t need = bgnn_loss_workspace_bytes(n);
  BGNN_REQUIRE(workspace_bytes >= need, "bgnn_loss_forward: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  BGNN_REQUIRE(((uintptr_t)workspace & 15) == 0, "bgnn_loss_forward: workspace not 16-byte aligned");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  LossArgs a{};
  a.prm = *params;
  a.in = *inputs;
  a.n = n;
  a.nwg = loss_workgroups(n);
  char *ws = static_cast<char *>(workspace);
  a.sums = reinterpret_cast<double *>(ws);
  a.pf = reinterpret_cast<double *>(ws + LOSS_HEAD);
  a.pi = reinterpret_cast<int32_t *>(ws + LOSS_HEAD + (size_t)a.nwg * LOSS_F_STRIDE * sizeof(double));
  a.terms = terms;
  a.counts = counts;
  hipLaunchKernelGGL(loss_nodes, dim3(a.nwg), dim3(LOSS_THREADS), 0, ctx->stream, a);
  hipLaunchKernelGGL(loss_finish, dim3(1), dim3(LOSS_THREADS), 0, ctx->stream, a);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

extern "C" int bgnn_loss_backward(bgnn_ctx *ctx, const bgnn_loss_params *params, int64_t n, const bgnn_loss_inputs *inputs,
                                  const double *sums, const float *upstream, float *grad_logits, float *grad_confidence,
                                  float *grad_correction) {
  BGNN_REQUIRE(ctx && sums && upstream, "bgnn_loss_backward: NULL argument");
  BGNN_TRY(loss_check("bgnn_loss_backward", params, n, inputs));
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  LossBwdArgs a{};
  a.prm = *params;
  a.in = *inputs;
  a.n = n;
  a.sums = sums;
  a.upstream = upstream;
  a.g_logits = grad_logits;
  a.g_conf = grad_confidence;
  a.g_corr = grad_correction;
  hipLaunchKernelGGL(loss_backward, dim3(loss_workgroups(n)), dim3(LOSS_THREADS), 0, ctx->stream, a);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
