// Reductions over the node rows of the backward pass (bgnn_backward), all deterministic -- no float atomics:
//
//   wgrad    dW[out][in] = sum_r dY[r][out] * X[r][in]    (the weight gradient of a Linear / of GATConv's lin)
//            exact float32 on the matrix cores (v_mfma_f32_32x32x2_f32, the op the forward GEMMs use).  The rows are cut into a
//            fixed number of chunks (<= 1024, set by the row capacity and the output size only); each wave multiplies one 32 x 32
//            output tile over one chunk into a partial, and the partials are added in chunk order (float64) afterwards.
//   colsum   out[c] = sum_r X[r][c] * (S ? S[r][s_off + c / s_div] : 1)   per-block float64 partials, added in block order.
//            Bias gradients (S = nullptr) and GATConv's attention vectors (X = xw, S = d a_src / d a_dst per head).
//   relu_drop_bwd   d *= (h > 0) * scale: the backward of ReLU followed by (inverted) dropout, from the stored output h
//            (a kept value is h = relu(y) / (1 - p) > 0 exactly when y > 0; a dropped one is 0).
#include <algorithm>
#include "bgnn_internal.h"

namespace bgnn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int WG_MAX_CHUNKS = 1024;
constexpr size_t WG_MAX_PARTIAL = (size_t)16 << 20;   // floats of partials per call (64 MiB)
constexpr int CS_MAX_BLOCKS = 1024;

struct WgradArgs {
  const float *dY, *X;
  float *partial;            // [chunks][n_out][n_in]
  const int64_t *d_m;
  int ldy, ldx, n_out, n_in, tiles_in, n_tiles, chunks;
};

// Lane l of a wave loads dY[row + (l >> 5)][o0 + (l & 31)] (the A operand: m = output, k = row) and X[row + (l >> 5)][i0 + (l & 31)]
// (the B operand: k = row, n = input); one MFMA consumes two rows.  Accumulator register i of lane l holds
// C[o0 + 8 (i >> 2) + 4 (l >> 5) + (i & 3)][i0 + (l & 31)].
__global__ __launch_bounds__(256) void wgrad_partial_kernel(WgradArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.y * 4 + wave;
  if (tile >= a.n_tiles) return;
  const int o0 = (tile / a.tiles_in) * 32, i0 = (tile % a.tiles_in) * 32;
  const int64_t M = *a.d_m;
  const int64_t per = (((M + a.chunks - 1) / a.chunks) + 15) & ~(int64_t)15;
  const int64_t r0 = (int64_t)blockIdx.x * per;
  const int64_t r1 = r0 + per < M ? r0 + per : M;
  const int c = lane & 31, k = lane >> 5;
  const bool oc = o0 + c < a.n_out, ic = i0 + c < a.n_in;
  const float *py = a.dY + o0 + c, *px = a.X + i0 + c;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  constexpr int U = 8;                               // MFMAs per step: 16 rows, loads issued before the products
  for (int64_t rb = r0; rb < r1; rb += 2 * U) {
    float av[U], bv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = rb + 2 * u + k;
      const bool ok = r < r1;
      av[u] = ok && oc ? py[r * a.ldy] : 0.0f;
      bv[u] = ok && ic ? px[r * a.ldx] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
  }
  float *dst = a.partial + (size_t)blockIdx.x * a.n_out * a.n_in;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int o = o0 + 8 * (i >> 2) + 4 * k + (i & 3);
    if (o < a.n_out && ic) dst[(size_t)o * a.n_in + i0 + c] = acc[i];
  }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *partial, int chunks, int n_out, int n_in, float *dW, int ldw) {
  const int64_t n = (int64_t)n_out * n_in;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int ch = 0; ch < chunks; ++ch) s += (double)partial[(size_t)ch * n + e];
    dW[(e / n_in) * ldw + e % n_in] = (float)s;
  }
}

size_t wgrad_workspace_bytes() { return WG_MAX_PARTIAL * sizeof(float); }

int launch_wgrad(bgnn_ctx *ctx, const float *dY, int ldy, const float *X, int ldx, const int64_t *d_m, int64_t max_rows, int n_out,
                 int n_in, float *dW, int ldw, void *workspace) {
  BGNN_REQUIRE(n_out >= 1 && n_in >= 1 && (size_t)n_out * n_in <= WG_MAX_PARTIAL, "wgrad: %d x %d output unsupported", n_out, n_in);
  if (max_rows <= 0) {
    BGNN_HIP_CHECK(hipMemset2DAsync(dW, (size_t)ldw * sizeof(float), 0, (size_t)n_in * sizeof(float), n_out, ctx->stream));
    return BGNN_OK;
  }
  int64_t chunks = std::min<int64_t>(WG_MAX_CHUNKS, (max_rows + 255) / 256);
  chunks = std::min<int64_t>(chunks, (int64_t)(WG_MAX_PARTIAL / ((size_t)n_out * n_in)));
  if (chunks < 1) chunks = 1;
  WgradArgs a{dY, X, (float *)workspace, d_m, ldy, ldx, n_out, n_in, (n_in + 31) / 32, 0, (int)chunks};
  a.n_tiles = ((n_out + 31) / 32) * a.tiles_in;
  ProfScope ps(ctx, BGNN_K_GEMM);
  hipLaunchKernelGGL(wgrad_partial_kernel, dim3((unsigned)chunks, (unsigned)((a.n_tiles + 3) / 4)), dim3(256), 0, ctx->stream, a);
  const int64_t n = (int64_t)n_out * n_in;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1024)), dim3(256), 0, ctx->stream,
                     (const float *)workspace, (int)chunks, n_out, n_in, dW, ldw);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

// ---- column sums -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float *X, int ld, int W, int Wp, const float *S, int lds, int s_off,
                                                             int s_div, const int64_t *d_m, double *partial) {
  const int64_t M = *d_m;
  const int lanes = 256 / Wp;
  const int col = threadIdx.x % Wp, rl = threadIdx.x / Wp;
  const int64_t per_block = (M + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * per_block, r1 = r0 + per_block < M ? r0 + per_block : M;
  double s = 0.0;
  if (col < W) {
    for (int64_t r = r0 + rl; r < r1; r += lanes) {
      double v = (double)X[r * ld + col];
      if (S) v *= (double)S[r * lds + s_off + col / s_div];
      s += v;
    }
  }
  __shared__ double sh[256];
  sh[threadIdx.x] = s;
  __syncthreads();
  if (rl == 0 && col < W) {
    for (int k = 1; k < lanes; ++k) s += sh[k * Wp + col];
    partial[(int64_t)blockIdx.x * W + col] = s;
  }
}

__global__ __launch_bounds__(256) void colsum_reduce_kernel(const double *partial, int nb, int W, float *out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= W) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += partial[(int64_t)b * W + c];
  out[c] = (float)s;
}

size_t colsum_workspace_bytes() { return (size_t)CS_MAX_BLOCKS * 256 * sizeof(double); }

int launch_colsum(bgnn_ctx *ctx, const float *X, int ld, int W, const float *S, int lds, int s_off, int s_div, const int64_t *d_m,
                  int64_t max_rows, float *out, void *workspace) {
  BGNN_REQUIRE(W >= 1 && W <= 256 && (!S || s_div >= 1), "colsum: width %d unsupported", W);
  if (max_rows <= 0) {
    BGNN_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)W * sizeof(float), ctx->stream));
    return BGNN_OK;
  }
  int Wp = 1;
  while (Wp < W) Wp <<= 1;
  const int nb = (int)std::min<int64_t>(CS_MAX_BLOCKS, (max_rows + 255) / 256);
  hipLaunchKernelGGL(colsum_partial_kernel, dim3(nb), dim3(256), 0, ctx->stream, X, ld, W, Wp, S, lds, s_off, s_div, d_m,
                     (double *)workspace);
  hipLaunchKernelGGL(colsum_reduce_kernel, dim3((W + 255) / 256), dim3(256), 0, ctx->stream, (const double *)workspace, nb, W, out);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

// ---- ReLU + dropout backward ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void relu_drop_bwd_kernel(float *d, int ldd, const float *h, int ldh, int W, const int64_t *d_m,
                                                            const float *scale) {
  const int64_t n = *d_m * (int64_t)W;
  const float s = *scale;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / W;
    const int c = (int)(e - r * W);
    float *p = d + r * ldd + c;
    *p = h[r * ldh + c] > 0.0f ? *p * s : 0.0f;
  }
}

int launch_relu_drop_bwd(bgnn_ctx *ctx, float *d, int ldd, const float *h, int ldh, int W, const int64_t *d_m, int64_t max_rows,
                         const float *scale) {
  if (max_rows <= 0) return BGNN_OK;
  const int64_t blocks = std::min<int64_t>((max_rows * W + 255) / 256, (int64_t)ctx->num_cus * 16);
  hipLaunchKernelGGL(relu_drop_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d, ldd, h, ldh, W, d_m, scale);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

}  // namespace bgnn
