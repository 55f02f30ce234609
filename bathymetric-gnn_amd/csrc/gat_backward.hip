// Backward of the GAT layers and of the output heads (bgnn_backward).  Restates the derivative of torch_geometric GATConv.forward
// with edge_dim, as gat_aggregate.hip restates its forward (oracle/gat_cpu.py: gat_conv):
//   e_ij = leaky_relu(a_src[j] + a_dst[i] + ea_ij . V, 0.2),  alpha = softmax_i(e),  alpha~ = alpha * mask,  out_i = sum_j alpha~_ij xw_j
// With g = dL/d out:
//   target side (per node i, head h; lanes as gat_aggregate_kernel's):  dalpha~_ij = <g_i[h], xw_j[h]>, dalpha = dalpha~ * mask,
//     de_ij = alpha_ij (dalpha_ij - sum_k alpha_ik dalpha_ik),  dlogit = de * (e > 0 ? 1 : 0.2)
//     -> alpha~ and dlogit per slot, d a_dst[i,h] = sum_j dlogit_ij, and node i's share of dV[h][f] = sum dlogit_ij ea_ij[f]
//   source side (per node j, its out-edges in a fixed order, then its self loop):  dxw_j[h] = sum_i alpha~_ij g_i[h],
//     d a_src[j,h] = sum_i dlogit_ij;  dxw += d a_src (x) att_src + d a_dst (x) att_dst
// Slots: stencil graphs [N][K + 1] (slot K = the self loop), CSR graphs [E] then the N self loops.  The out-edges of a node come
// from a transposed index built once per graph on the device (counting sort, each node's list then sorted by slot: fixed order).
// No float atomics anywhere: every sum has one owner or goes through a block-ordered column reduction (wgrad_f32.hip).
#include <algorithm>
#include "bgnn_internal.h"

namespace bgnn {

struct AttBwdArgs {
  const float *xw;        // [N][HC]
  const float *asd;       // [N][2H]
  const int32_t *nbr;     // ELL [N][K] or CSR col[E]
  const float *eattr;     // [N][K][ED] or [E][ED]
  const int32_t *rowptr;  // CSR only
  const float *V;         // [H][ED]
  const float *g;         // [N][HC] dL/d(aggregate)
  float *alpha_t;         // [slots][H]
  float *dlogit;          // [slots][H]
  float *dasd;            // [N][2H]
  float *dVn;             // [N][H][ED]
  const BgnnTapeHeader *hdr;
  const int64_t *d_m;
  int64_t self_base;      // CSR: slot of node i's self loop = self_base + i
  int K, H, C, ED;
  uint32_t att_stream;
};

__device__ __forceinline__ int64_t bwd_slot(const AttBwdArgs &a, int64_t i, int64_t p) {
  return a.rowptr ? p : i * (a.K + 1) + (p - i * a.K);
}
__device__ __forceinline__ int64_t bwd_self_slot(const AttBwdArgs &a, int64_t i) {
  return a.rowptr ? a.self_base + i : i * (a.K + 1) + a.K;
}

template <int LPN>
__global__ __launch_bounds__(256) void gat_bwd_target_kernel(AttBwdArgs a) {
  constexpr int NPW = 64 / LPN;
  constexpr int HC = LPN * 4;
  const int64_t M = *a.d_m;
  const int lane = threadIdx.x & 63;
  const int sub = lane / LPN, l = lane % LPN;
  const int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t i = wave_id * NPW + sub;
  if (i >= M) return;                               // (the lanes of one node leave together: shuffles stay inside a node)
  const int H = a.H, ED = a.ED, G = a.C / 4;         // G lanes per head
  const int hh = l / G;
  const bool writer = (l % G) == 0;
  int64_t beg, end;
  if (a.rowptr) { beg = a.rowptr[i]; end = a.rowptr[i + 1]; }
  else { beg = i * a.K; end = beg + a.K; }
  float v[4];
  for (int f = 0; f < 4; ++f) v[f] = f < ED ? a.V[hh * ED + f] : 0.0f;
  const float ad = a.asd[i * 2 * H + H + hh];
  const DropSpec drop = a.hdr->att;
  auto mask = [&](int64_t j) -> float {
    if (drop.thr == 0) return 1.0f;
    const uint64_t idx = (((uint64_t)i << 32) | (uint64_t)(uint32_t)j) * (uint64_t)H + (uint64_t)hh;
    return bgnn_drop_hash(drop.seed, a.att_stream, idx) >= drop.thr ? drop.scale : 0.0f;
  };
  auto logit = [&](int64_t p, int j) -> float {
    float lg = a.asd[(int64_t)j * 2 * H + hh] + ad;
    float dot = 0.0f;
    for (int f = 0; f < ED; ++f) dot += a.eattr[p * ED + f] * v[f];
    lg += dot;
    return lg > 0.0f ? lg : 0.2f * lg;
  };
  // pass 1: running max, self-loop attribute (mean of the incoming attributes)
  float ea_sum[4] = {0.f, 0.f, 0.f, 0.f};
  int deg = 0;
  float mx = -__builtin_inff();
  for (int64_t p = beg; p < end; ++p) {
    const int j = a.nbr[p];
    if (j < 0) continue;
    for (int f = 0; f < ED; ++f) ea_sum[f] += a.eattr[p * ED + f];
    mx = fmaxf(mx, logit(p, j));
    ++deg;
  }
  float ea_self[4] = {0.f, 0.f, 0.f, 0.f};
  float self_lg;
  {
    const float cnt = (float)(deg > 0 ? deg : 1);
    float dot = 0.0f;
    for (int f = 0; f < ED; ++f) { ea_self[f] = ea_sum[f] / cnt; dot += ea_self[f] * v[f]; }
    self_lg = a.asd[i * 2 * H + hh] + ad + dot;
    self_lg = self_lg > 0.0f ? self_lg : 0.2f * self_lg;
    mx = fmaxf(mx, self_lg);
  }
  // pass 2: denominator
  float den = 0.0f;
  for (int64_t p = beg; p < end; ++p) {
    const int j = a.nbr[p];
    if (j >= 0) den += expf(logit(p, j) - mx);
  }
  const float pself = expf(self_lg - mx);
  den += pself;
  den += 1e-16f;
  // pass 3: dalpha per slot (dot over the head's channels: G lanes), sum_k alpha_ik dalpha_ik
  const float4 gi = *reinterpret_cast<const float4 *>(a.g + i * HC + l * 4);
  auto head_dot = [&](int64_t j) -> float {
    const float4 x = *reinterpret_cast<const float4 *>(a.xw + j * HC + l * 4);
    float d = gi.x * x.x + gi.y * x.y + gi.z * x.z + gi.w * x.w;
    for (int o = 1; o < G; o <<= 1) d += __shfl_xor(d, o, 64);
    return d;
  };
  float s_ad = 0.0f;
  for (int64_t p = beg; p < end; ++p) {
    const int j = a.nbr[p];
    if (j < 0) continue;
    const float al = expf(logit(p, j) - mx) / den;
    const float mk = mask(j);
    const float da = head_dot(j) * mk;
    s_ad += al * da;
    if (writer) {
      const int64_t s = bwd_slot(a, i, p);
      a.alpha_t[s * H + hh] = al * mk;
      a.dlogit[s * H + hh] = da;                    // (dalpha for now; pass 4 turns it into dlogit)
    }
  }
  const float al_self = pself / den, mk_self = mask(i);
  const float da_self = head_dot(i) * mk_self;
  s_ad += al_self * da_self;
  if (!writer) return;
  // pass 4 (one lane per head): dlogit, d a_dst, dV
  float dad = 0.0f, dv[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t p = beg; p < end; ++p) {
    const int j = a.nbr[p];
    if (j < 0) continue;
    const float lg = logit(p, j);
    const float al = expf(lg - mx) / den;
    const int64_t s = bwd_slot(a, i, p);
    const float de = al * (a.dlogit[s * H + hh] - s_ad);
    const float dl = lg > 0.0f ? de : 0.2f * de;
    a.dlogit[s * H + hh] = dl;
    dad += dl;
    for (int f = 0; f < ED; ++f) dv[f] += dl * a.eattr[p * ED + f];
  }
  {
    const float de = al_self * (da_self - s_ad);
    const float dl = self_lg > 0.0f ? de : 0.2f * de;
    const int64_t s = bwd_self_slot(a, i);
    a.alpha_t[s * H + hh] = al_self * mk_self;
    a.dlogit[s * H + hh] = dl;
    dad += dl;
    for (int f = 0; f < ED; ++f) dv[f] += dl * ea_self[f];
  }
  a.dasd[i * 2 * H + H + hh] = dad;
  for (int f = 0; f < ED; ++f) a.dVn[(i * H + hh) * ED + f] = dv[f];
}

struct AttSrcArgs {
  const float *g;          // [N][HC]
  const float *alpha_t, *dlogit;
  const int32_t *tr_ptr, *tr_slot, *tr_dst;   // out-edges of every node: slot and target
  float *dasd;             // [N][2H]: d a_dst read, d a_src written
  const float *att_src, *att_dst;
  float *dxw;              // [N][HC]
  const int64_t *d_m;
  int64_t self_base;       // CSR: self slot = self_base + j; stencil (self_base < 0): j * (K + 1) + K
  int K, H, C;
};

template <int LPN>
__global__ __launch_bounds__(256) void gat_bwd_source_kernel(AttSrcArgs a) {
  constexpr int NPW = 64 / LPN;
  constexpr int HC = LPN * 4;
  const int64_t M = *a.d_m;
  const int lane = threadIdx.x & 63;
  const int sub = lane / LPN, l = lane % LPN;
  const int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t j = wave_id * NPW + sub;
  if (j >= M) return;
  const int H = a.H, hh = (l * 4) / a.C;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float das = 0.0f;
  const int32_t q0 = a.tr_ptr[j], q1 = a.tr_ptr[j + 1];
  for (int32_t q = q0; q < q1; ++q) {
    const int64_t s = a.tr_slot[q], i = a.tr_dst[q];
    const float at = a.alpha_t[s * H + hh];
    const float4 gi = *reinterpret_cast<const float4 *>(a.g + i * HC + l * 4);
    acc.x += at * gi.x; acc.y += at * gi.y; acc.z += at * gi.z; acc.w += at * gi.w;
    das += a.dlogit[s * H + hh];
  }
  {
    const int64_t s = a.self_base >= 0 ? a.self_base + j : j * (a.K + 1) + a.K;
    const float at = a.alpha_t[s * H + hh];
    const float4 gj = *reinterpret_cast<const float4 *>(a.g + j * HC + l * 4);
    acc.x += at * gj.x; acc.y += at * gj.y; acc.z += at * gj.z; acc.w += at * gj.w;
    das += a.dlogit[s * H + hh];
  }
  const float dad = a.dasd[j * 2 * H + H + hh];
  const float4 as = *reinterpret_cast<const float4 *>(a.att_src + l * 4);
  const float4 at = *reinterpret_cast<const float4 *>(a.att_dst + l * 4);
  float4 o;
  o.x = acc.x + das * as.x + dad * at.x; o.y = acc.y + das * as.y + dad * at.y;
  o.z = acc.z + das * as.z + dad * at.z; o.w = acc.w + das * as.w + dad * at.w;
  *reinterpret_cast<float4 *>(a.dxw + j * HC + l * 4) = o;
  if ((l % (a.C / 4)) == 0) a.dasd[j * 2 * H + hh] = das;
}

// ---- transposed index of a graph (out-edges per source node) -------------------------------------------------------------------
__global__ void tr_count_kernel(const int32_t *nbr, const int32_t *rowptr, int K, const int64_t *d_m, int32_t *cnt) {
  const int64_t M = *d_m;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t beg = rowptr ? rowptr[i] : i * K, end = rowptr ? rowptr[i + 1] : beg + K;
    for (int64_t p = beg; p < end; ++p) {
      const int j = nbr[p];
      if (j >= 0) atomicAdd(&cnt[j], 1);            // (integer counts: exact in any order)
    }
  }
}

// exclusive prefix sum of cnt[0..M) into ptr[0..M], one workgroup (1024 contiguous segments)
__global__ __launch_bounds__(1024) void tr_scan_kernel(const int32_t *cnt, const int64_t *d_m, int32_t *ptr) {
  const int64_t M = *d_m;
  const int t = threadIdx.x;
  const int64_t seg = (M + 1023) / 1024;
  const int64_t b = t * seg, e = b + seg < M ? b + seg : M;
  int64_t s = 0;
  for (int64_t k = b; k < e; ++k) s += cnt[k];
  __shared__ int64_t part[1024];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int64_t run = 0;
    for (int k = 0; k < 1024; ++k) { const int64_t v = part[k]; part[k] = run; run += v; }
    ptr[M] = (int32_t)run;
  }
  __syncthreads();
  int64_t run = part[t];
  for (int64_t k = b; k < e; ++k) { ptr[k] = (int32_t)run; run += cnt[k]; }
}

__global__ void tr_fill_kernel(const int32_t *nbr, const int32_t *rowptr, int K, const int64_t *d_m, const int32_t *ptr,
                               int32_t *cursor, int32_t *tr_slot, int32_t *tr_dst) {
  const int64_t M = *d_m;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t beg = rowptr ? rowptr[i] : i * K, end = rowptr ? rowptr[i + 1] : beg + K;
    for (int64_t p = beg; p < end; ++p) {
      const int j = nbr[p];
      if (j < 0) continue;
      const int32_t q = ptr[j] + atomicAdd(&cursor[j], 1);
      tr_slot[q] = (int32_t)(rowptr ? p : i * (K + 1) + (p - beg));
      tr_dst[q] = (int32_t)i;
    }
  }
}

// the fill placed each node's out-edges in arrival order: sort every list by slot (insertion sort -- lists are short)
__global__ void tr_sort_kernel(const int64_t *d_m, const int32_t *ptr, int32_t *tr_slot, int32_t *tr_dst) {
  const int64_t M = *d_m;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += (int64_t)gridDim.x * blockDim.x) {
    const int32_t q0 = ptr[j], q1 = ptr[j + 1];
    for (int32_t q = q0 + 1; q < q1; ++q) {
      const int32_t s = tr_slot[q], d = tr_dst[q];
      int32_t k = q - 1;
      while (k >= q0 && tr_slot[k] > s) { tr_slot[k + 1] = tr_slot[k]; tr_dst[k + 1] = tr_dst[k]; --k; }
      tr_slot[k + 1] = s; tr_dst[k + 1] = d;
    }
  }
}

int ensure_transposed_index(const bgnn_graph *g) {
  if (g->tr_valid) return BGNN_OK;
  bgnn_ctx *ctx = g->ctx;
  BGNN_TRY(ensure_stencil_table(g));
  const int64_t rows = g->row_capacity;
  const int64_t cap = g->kind == 1 ? std::max<int64_t>(g->generic_E, 1) : std::max<int64_t>(rows * g->K, 1);
  void *p3 = nullptr;
  BGNN_TRY(graph_alloc(g, g->d_tr_ptr, rows + 1));
  BGNN_TRY(graph_alloc(g, g->d_tr_slot, cap));
  BGNN_TRY(graph_alloc(g, g->d_tr_dst, cap));
  BGNN_TRY(ctx->pool.alloc((size_t)std::max<int64_t>(rows, 1) * 2 * sizeof(int32_t), &p3));
  int32_t *cnt = (int32_t *)p3, *cursor = cnt + rows;
  const int32_t *rowptr = g->kind == 1 ? g->d_rowptr : nullptr;
  BGNN_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)rows * 2 * sizeof(int32_t), ctx->stream));
  const unsigned nb = (unsigned)std::min<int64_t>((rows + 255) / 256, (int64_t)ctx->num_cus * 16);
  hipLaunchKernelGGL(tr_count_kernel, dim3(nb), dim3(256), 0, ctx->stream, g->d_nbr, rowptr, g->K, g->d_counts, cnt);
  hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t *)cnt, g->d_counts, g->d_tr_ptr);
  hipLaunchKernelGGL(tr_fill_kernel, dim3(nb), dim3(256), 0, ctx->stream, g->d_nbr, rowptr, g->K, g->d_counts,
                     (const int32_t *)g->d_tr_ptr, cursor, g->d_tr_slot, g->d_tr_dst);
  hipLaunchKernelGGL(tr_sort_kernel, dim3(nb), dim3(256), 0, ctx->stream, g->d_counts, (const int32_t *)g->d_tr_ptr, g->d_tr_slot,
                     g->d_tr_dst);
  BGNN_HIP_CHECK(hipGetLastError());
  ctx->pool.release(p3);                             // (stream-ordered: the next user of the block queues behind these kernels)
  g->tr_valid = true;
  return BGNN_OK;
}

int64_t gat_bwd_slot_count(const bgnn_graph *g) {
  return g->kind == 1 ? g->generic_E + g->row_capacity : (int64_t)g->row_capacity * (g->K + 1);
}

int launch_gat_backward(bgnn_ctx *ctx, const bgnn_graph *g, const BgnnLayer &L, int C, int ED, const BgnnTapeHeader *hdr,
                        uint32_t att_stream, const float *xw, const float *asd, const float *grad_out, float *alpha_t, float *dlogit,
                        float *dasd, float *dVn, float *dxw) {
  const int64_t rows = g->row_capacity;
  if (rows <= 0) return BGNN_OK;
  const int HC = L.heads * C;
  BGNN_REQUIRE(HC <= 256 && HC % 32 == 0 && C % 32 == 0, "GAT backward: heads x hidden = %d unsupported (at most 256 columns)", HC);
  BGNN_TRY(ensure_stencil_table(g));
  BGNN_TRY(ensure_edge_attrs(g));
  BGNN_TRY(ensure_transposed_index(g));
  ProfScope ps(ctx, BGNN_K_AGGREGATE);
  AttBwdArgs a{};
  a.xw = xw; a.asd = asd; a.nbr = g->d_nbr; a.eattr = g->d_eattr; a.rowptr = g->kind == 1 ? g->d_rowptr : nullptr;
  a.V = L.V; a.g = grad_out; a.alpha_t = alpha_t; a.dlogit = dlogit; a.dasd = dasd; a.dVn = dVn; a.hdr = hdr; a.d_m = g->d_counts;
  a.self_base = g->kind == 1 ? g->generic_E : -1;
  a.K = g->K; a.H = L.heads; a.C = C; a.ED = ED; a.att_stream = att_stream;
  AttSrcArgs s{};
  s.g = grad_out; s.alpha_t = alpha_t; s.dlogit = dlogit; s.tr_ptr = g->d_tr_ptr; s.tr_slot = g->d_tr_slot; s.tr_dst = g->d_tr_dst;
  s.dasd = dasd; s.att_src = L.att_src; s.att_dst = L.att_dst; s.dxw = dxw; s.d_m = g->d_counts;
  s.self_base = a.self_base; s.K = g->K; s.H = L.heads; s.C = C;
  const int LPN = HC / 4;
  const int64_t waves = (rows + 64 / LPN - 1) / (64 / LPN);
  dim3 grid((unsigned)((waves + 3) / 4)), block(256);
#define BGNN_BWD_CASE(N)                                                                    \
  case N:                                                                                   \
    hipLaunchKernelGGL(gat_bwd_target_kernel<N>, grid, block, 0, ctx->stream, a);           \
    hipLaunchKernelGGL(gat_bwd_source_kernel<N>, grid, block, 0, ctx->stream, s);           \
    break;
  switch (LPN) {
    BGNN_BWD_CASE(8) BGNN_BWD_CASE(16) BGNN_BWD_CASE(32) BGNN_BWD_CASE(64)
    default:
      set_error("GAT backward: heads x hidden = %d unsupported", HC);
      return BGNN_ERR_UNSUPPORTED;
  }
#undef BGNN_BWD_CASE
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

// d att_edge[h][c] = sum_f dV[h][f] W_e[hC + c][f],  d lin_edge.weight[hC + c][f] = att_edge[h][c] dV[h][f]
__global__ void gat_edge_param_grads_kernel(const float *dV, const float *att_edge, const float *W_e, int H, int C, int ED,
                                            float *d_att_edge, float *d_W_e) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= H * C) return;
  const int h = t / C;
  float s = 0.0f;
  for (int f = 0; f < ED; ++f) {
    s += dV[h * ED + f] * W_e[(int64_t)t * ED + f];
    d_W_e[(int64_t)t * ED + f] = att_edge[t] * dV[h * ED + f];
  }
  d_att_edge[t] = s;
}

int launch_gat_edge_param_grads(bgnn_ctx *ctx, const float *dV, const float *att_edge, const float *W_e, int H, int C, int ED,
                                float *d_att_edge, float *d_W_e) {
  hipLaunchKernelGGL(gat_edge_param_grads_kernel, dim3((H * C + 255) / 256), dim3(256), 0, ctx->stream, dV, att_edge, W_e, H, C, ED,
                     d_att_edge, d_W_e);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

// ---- heads ---------------------------------------------------------------------------------------------------------------------
// Per node, from the stored hidden units hb (after ReLU and dropout) and the output gradients: the logits and the confidence
// pre-activation are recomputed from hb, then
//   dlogit = dL/dlogits + p * (dL/dp - <dL/dp, p>)      (softmax Jacobian),   ds = dL/dconfidence * sig * (1 - sig),   dcorr
// dY2 [N][n2] = (dlogit | ds | dcorr): the gradient of the heads' second layers' outputs; dhid [N][ldh] = dL/d(first-layer
// output) through the head dropout and the ReLU (zero in the pad columns).
struct HeadsBwdArgs {
  const float *hb;        // [N][ldh]
  const float *W1, *b1;   // the model's packed second layers (hd_W1 / hd_b1)
  const float *dlog, *dprob, *dconf, *dcorr;
  const BgnnTapeHeader *hdr;
  float *dY2, *dhid;
  const int64_t *d_m;
  int ldh, hh, nc, nh, n2;
};

__global__ __launch_bounds__(256) void heads_backward_kernel(HeadsBwdArgs a) {
  const int64_t M = *a.d_m;
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= M) return;
  const float *hb = a.hb + r * a.ldh;
  const int nc = a.nc, hh = a.hh;
  float lg[16], dl[16];
  float mx = -__builtin_inff();
  for (int k = 0; k < nc; ++k) {
    float s = a.b1[k];
    for (int u = 0; u < hh; ++u) s += a.W1[k * hh + u] * hb[u];
    lg[k] = s;
    mx = fmaxf(mx, s);
  }
  float den = 0.0f;
  for (int k = 0; k < nc; ++k) { lg[k] = expf(lg[k] - mx); den += lg[k]; }
  float sp = 0.0f;
  for (int k = 0; k < nc; ++k) {
    lg[k] /= den;                                    // probabilities
    if (a.dprob) sp += a.dprob[r * nc + k] * lg[k];
  }
  for (int k = 0; k < nc; ++k) {
    float d = a.dlog ? a.dlog[r * nc + k] : 0.0f;
    if (a.dprob) d += lg[k] * (a.dprob[r * nc + k] - sp);
    dl[k] = d;
    a.dY2[r * a.n2 + k] = d;
  }
  float ds = 0.0f;
  if (a.dconf) {
    float s = a.b1[nc];
    for (int u = 0; u < hh; ++u) s += a.W1[nc * hh + u] * hb[hh + u];
    const float sg = 1.0f / (1.0f + expf(-s));
    ds = a.dconf[r] * sg * (1.0f - sg);
  }
  a.dY2[r * a.n2 + nc] = ds;
  const float dc = a.nh > 2 && a.dcorr ? a.dcorr[r] : 0.0f;
  if (a.nh > 2) a.dY2[r * a.n2 + nc + 1] = dc;
  const float sc = a.hdr->s_heads;
  float *dh = a.dhid + r * a.ldh;
  for (int u = 0; u < a.ldh; ++u) {
    const int k = u / hh, uu = u - k * hh;
    float d = 0.0f;
    if (k == 0) {
      for (int c = 0; c < nc; ++c) d += dl[c] * a.W1[c * hh + uu];
    } else if (k == 1) {
      d = ds * a.W1[nc * hh + uu];
    } else if (k == 2 && a.nh > 2) {
      d = dc * a.W1[(nc + 1) * hh + uu];
    }
    dh[u] = k < a.nh && hb[u] > 0.0f ? d * sc : 0.0f;
  }
}

int launch_heads_backward(bgnn_ctx *ctx, const bgnn_model *m, const float *hb, const float *dlog, const float *dprob, const float *dconf,
                          const float *dcorr, const BgnnTapeHeader *hdr, const int64_t *d_m, int64_t max_rows, float *dY2, float *dhid) {
  if (max_rows <= 0) return BGNN_OK;
  const bgnn_model_desc &d = m->desc;
  BGNN_REQUIRE(d.num_classes <= 16, "heads backward: %d classes unsupported", d.num_classes);
  HeadsBwdArgs a{hb, m->hd_W1, m->hd_b1, dlog, dprob, dconf, dcorr, hdr, dY2, dhid, d_m, m->head_hidden_total, d.hidden / 2,
                 d.num_classes, d.predict_correction ? 3 : 2, d.num_classes + (d.predict_correction ? 2 : 1)};
  ProfScope ps(ctx, BGNN_K_HEADS);
  hipLaunchKernelGGL(heads_backward_kernel, dim3((unsigned)((max_rows + 255) / 256)), dim3(256), 0, ctx->stream, a);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

}  // namespace bgnn
