// Backward of the neighbour aggregates of the GraphSAGE and GIN layers (bgnn_backward): the transpose of neighbor_reduce.hip's
// in-edge gather.  The forward sums over the IN-edges of a node; its backward sums over the OUT-edges of every source node j:
//   MEAN (SAGEConv):  out_j = root_j + sum_{i : j -> i} g_i / max(cnt_i, 1)     root = dL/dz . lin_r.weight, g = dL/dz . lin_l.weight
//   SUM  (GINConv) :  out_j = root_j + sum_{i : j -> i} g_i                     root = g = ds (the (1 + eps) x_i term, eps = 0)
// cnt_i counts node i's in-edges as the forward does: stencil holes (-1) do not count, repeated CSR edges count each time, a stencil
// graph's explicit self loop (GraphBuilder include_self_loops) counts once.  Foreign graphs reach here without self loops (the
// forward refuses SAGE / GIN on those that carry some).  The out-edges come from the graph's transposed index (gat_backward.hip,
// ensure_transposed_index: each node's list sorted by slot), a stencil graph's explicit self loop is added after them: a fixed
// order, one owner per output row, no atomics -- two calls give bit-identical results.  HBM / L2 bound gather; lanes own float4
// channel groups of one node, as in neighbor_reduce_kernel.
#include <algorithm>
#include "bgnn_internal.h"

namespace bgnn {

// 1 / max(cnt_i, 1) per node (the MEAN mode's coefficient), counted as neighbor_reduce_kernel counts
__global__ __launch_bounds__(256) void plain_inv_count_kernel(const int32_t *nbr, const int32_t *rowptr, int K, int self_loops,
                                                              const int64_t *d_m, float *cinv) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= *d_m) return;
  const int64_t beg = rowptr ? rowptr[i] : i * K, end = rowptr ? rowptr[i + 1] : beg + K;
  int cnt = self_loops;
  for (int64_t p = beg; p < end; ++p) cnt += nbr[p] >= 0 ? 1 : 0;
  cinv[i] = 1.0f / (float)(cnt > 0 ? cnt : 1);
}

struct PlainBwdArgs {
  const float *root;       // [N][D]
  const float *g;          // [N][D]: the gradient of the aggregate's output, read at the targets of the out-edges
  const float *cinv;       // MEAN: 1 / max(cnt, 1) per node; SUM: nullptr
  const int32_t *tr_ptr, *tr_dst;   // out-edges of every node: its targets
  float *out;              // [N][D] (not g)
  const int64_t *d_m;
  int self_loops;
};

template <int LPN>                                       // lanes per node = D / 4
__global__ __launch_bounds__(256) void plain_bwd_aggregate_kernel(PlainBwdArgs a) {
  constexpr int NPW = 64 / LPN;
  constexpr int D = LPN * 4;
  const int64_t M = *a.d_m;
  const int lane = threadIdx.x & 63;
  const int sub = lane / LPN, l = lane % LPN;
  const int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t j = wave_id * NPW + sub;
  if (j >= M) return;
  float4 acc = *reinterpret_cast<const float4 *>(a.root + j * D + l * 4);
  auto add = [&](int64_t i) {
    const float4 gi = *reinterpret_cast<const float4 *>(a.g + i * D + l * 4);
    if (a.cinv) {
      const float c = a.cinv[i];
      acc.x += c * gi.x; acc.y += c * gi.y; acc.z += c * gi.z; acc.w += c * gi.w;
    } else {
      acc.x += gi.x; acc.y += gi.y; acc.z += gi.z; acc.w += gi.w;
    }
  };
  const int32_t q0 = a.tr_ptr[j], q1 = a.tr_ptr[j + 1];
  for (int32_t q = q0; q < q1; ++q) add(a.tr_dst[q]);
  if (a.self_loops) add(j);
  *reinterpret_cast<float4 *>(a.out + j * D + l * 4) = acc;
}

int launch_plain_inv_count(bgnn_ctx *ctx, const bgnn_graph *g, float *cinv) {
  const int64_t rows = g->row_capacity;
  if (rows <= 0) return BGNN_OK;
  BGNN_TRY(ensure_stencil_table(g));
  ProfScope ps(ctx, BGNN_K_AGGREGATE);
  hipLaunchKernelGGL(plain_inv_count_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream, g->d_nbr,
                     g->kind == 0 ? nullptr : g->d_rowptr, g->K, g->kind == 0 ? g->include_self_loops : 0, g->d_counts, cinv);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

int launch_plain_bwd_aggregate(bgnn_ctx *ctx, const bgnn_graph *g, int mode, int D, const float *root, const float *grad,
                               const float *cinv, float *out) {
  const int64_t rows = g->row_capacity;
  if (rows <= 0) return BGNN_OK;
  BGNN_REQUIRE(D == 32 || D == 64 || D == 128, "plain aggregate backward: width %d unsupported (32, 64 or 128)", D);
  BGNN_REQUIRE(mode == 2 || mode == 3, "plain aggregate backward: mode %d (2 = mean, 3 = sum)", mode);
  BGNN_REQUIRE(mode != 2 || cinv, "plain aggregate backward: the mean mode needs 1 / count per node");
  BGNN_REQUIRE(out != grad, "plain aggregate backward: out must not alias the gradient it gathers");
  BGNN_TRY(ensure_stencil_table(g));
  BGNN_TRY(ensure_transposed_index(g));
  PlainBwdArgs a{root, grad, mode == 2 ? cinv : nullptr, g->d_tr_ptr, g->d_tr_dst, out, g->d_counts,
                 g->kind == 0 ? g->include_self_loops : 0};
  ProfScope ps(ctx, BGNN_K_AGGREGATE);
  const int lpn = D / 4, npw = 64 / lpn;
  const int64_t waves = (rows + npw - 1) / npw;
  dim3 grid((unsigned)((waves + 3) / 4)), block(256);
  if (lpn == 32) hipLaunchKernelGGL(plain_bwd_aggregate_kernel<32>, grid, block, 0, ctx->stream, a);
  else if (lpn == 16) hipLaunchKernelGGL(plain_bwd_aggregate_kernel<16>, grid, block, 0, ctx->stream, a);
  else hipLaunchKernelGGL(plain_bwd_aggregate_kernel<8>, grid, block, 0, ctx->stream, a);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

}  // namespace bgnn
