// The model half of the C ABI (include/bgnn.h): the layout of the weight blob, the host-side packers of every weight image the kernels
// read, zero padding to a supported width, bgnn_model_create / bgnn_model_destroy.  Host code only.
#include <string.h>

#include <algorithm>
#include <cmath>

#include "bgnn_internal.h"

namespace bgnn {

int head_count(const bgnn_model_desc *d) { return d->predict_correction ? 3 : 2; }

// The one place that knows which tensors the weight blob holds, in which order and with which shapes (include/bgnn.h,
// bgnn_model_weight_count; models/gnn.py _blob_slots is its Python twin).
static WeightLayout weight_layout(const bgnn_model_desc &d) {
  const bool gat = d.gnn_type == BGNN_GNN_GAT;
  const size_t hid = d.hidden, hh = hid / 2;
  WeightLayout t;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += n; return at; };
  t.fe_W0 = take(hid * d.in_channels); t.fe_b0 = take(hid); t.fe_W1 = take(hid * hid); t.fe_b1 = take(hid);
  for (int l = 0; l < d.num_layers; ++l) {
    // GAT: H heads of hid channels over D inputs (the last layer: one head); every other backbone maps hidden -> hidden
    const size_t H = gat && l + 1 < d.num_layers ? d.heads : 1, D = gat && l > 0 ? hid * d.heads : hid, HC = H * hid;
    WeightLayout::Layer L{};
    L.W = take(HC * D);
    if (gat) { L.as = take(HC); L.ad = take(HC); L.ae = take(HC); L.We = take(HC * d.edge_dim); L.bias = take(HC); }
    else if (d.gnn_type == BGNN_GNN_GCN) L.bias = take(hid);
    else if (d.gnn_type == BGNN_GNN_SAGE) { L.bias = take(hid); L.W2 = take(hid * hid); }
    else { L.b1 = take(hid); L.W2 = take(hid * hid); L.bias = take(hid); }                 // GIN
    L.bn_w = take(HC); L.bn_b = take(HC); L.bn_mean = take(HC); L.bn_var = take(HC);
    t.layers.push_back(L);
  }
  for (int k = 0; k < head_count(&d); ++k) {
    const size_t nout = k == 0 ? d.num_classes : 1;
    t.hd_W0[k] = take(hh * hid); t.hd_b0[k] = take(hh); t.hd_W1[k] = take(nout * hh); t.hd_b1[k] = take(nout);
  }
  t.total = o;
  return t;
}

// ---- bf16x3 operand split (opt-in matrix path) --------------------------------------------------------------
// w = hi + lo + O(2^-16 |w|) with hi = bf16(w), lo = bf16(w - hi), round to nearest even.  The image replaces Wt
// [D][NC] float32 byte for byte: per 16-row half-chunk, per 32-column tile t, per part p (hi, lo), one 1-KiB block in
// the lane order of v_mfma_f32_32x32x16_bf16's A operand: [k-group 2][column m 32][k 8] bf16.
static inline uint16_t bf16_rne(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline float bf16_to_f32(uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; }

static inline uint16_t f16_rne(float f) {               // float32 -> IEEE half, round to nearest even, overflow -> inf
  uint32_t u; memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  const int32_t e = (int32_t)((u >> 23) & 0xff) - 127 + 15;
  uint32_t m = u & 0x7fffffu;
  if (((u >> 23) & 0xff) == 0xff) return (uint16_t)(sign | 0x7c00u | (m ? 0x200u : 0));
  if (e >= 31) return (uint16_t)(sign | 0x7c00u);
  if (e <= 0) {                                            // subnormal half (or zero)
    if (e < -10) return (uint16_t)sign;
    m |= 0x800000u;
    const int shift = 14 - e;                              // 24-bit significand -> 10 bits at exponent 2^-14
    const uint32_t half = m >> shift, rem = m & ((1u << shift) - 1), mid = 1u << (shift - 1);
    return (uint16_t)(sign | (half + ((rem > mid || (rem == mid && (half & 1))) ? 1 : 0)));
  }
  const uint32_t half = ((uint32_t)e << 10) | (m >> 13), rem = m & 0x1fffu;
  return (uint16_t)(sign | (half + ((rem > 0x1000u || (rem == 0x1000u && (half & 1))) ? 1 : 0)));
}
static inline float f16_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1f, m = h & 0x3ffu;
  uint32_t u;
  if (e == 0) {
    if (m == 0) u = sign;
    else { int k = 0; uint32_t mm = m; while (!(mm & 0x400u)) { mm <<= 1; ++k; } u = sign | ((uint32_t)(113 - k) << 23) | ((mm & 0x3ffu) << 13); }
  } else if (e == 31) u = sign | 0x7f800000u | (m << 13);
  else u = sign | ((e + 112) << 23) | (m << 13);
  float f; memcpy(&f, &u, 4); return f;
}

// float16 images hold W * 2^S, S chosen so that the largest |w| lands in [2^12, 2^13): the lo part of an element is then ~2^-11 of it
// and NORMAL in float16 for everything within 2^14 of the largest weight -- unscaled, the lo parts of glorot-sized weights (|w| <=
// 0.14, lo <= 6.7e-5) sat at float16's smallest normal and were carried with an absolute step of 2^-24, i.e. ~21 bits of W: that,
// not the dropped lo x lo term, was what put fp16x3 2.4x farther from the float64 forward than the exact path (profiles/NOTES_r05.md).
// The kernels multiply their accumulators by 2^-S (*inv_scale; exact) before the epilogue.  Returns false when a weight is beyond float16's range.
static bool pack_split(const float *Wt, int D, int NC, float *dst_as_float, bool f16, float *inv_scale = nullptr) {
  float sc = 1.0f;
  if (f16) {
    float amax = 0.0f;
    for (size_t i = 0; i < (size_t)D * NC; ++i) {
      if (!(std::fabs(Wt[i]) < 65504.0f)) return false;   // (a weight that large also drives the ACTIVATIONS out of float16's range: bf16 split instead)
      amax = std::max(amax, std::fabs(Wt[i]));
    }
    if (amax > 0.0f) {
      int e;
      std::frexp(amax, &e);                              // amax = m 2^e, m in [0.5, 1)
      const int S = std::max(-100, std::min(100, 13 - e));
      sc = std::ldexp(1.0f, S);
    }
  }
  if (inv_scale) *inv_scale = 1.0f / sc;
  uint16_t *dst = reinterpret_cast<uint16_t *>(dst_as_float);
  const int NT = NC / 32;
  for (int hc = 0; hc < D / 16; ++hc)
    for (int t = 0; t < NT; ++t)
      for (int part = 0; part < 2; ++part)
        for (int kg = 0; kg < 2; ++kg)
          for (int m = 0; m < 32; ++m)
            for (int i = 0; i < 8; ++i) {
              const float w = Wt[(size_t)(hc * 16 + kg * 8 + i) * NC + t * 32 + m] * sc;
              const uint16_t hi = f16 ? f16_rne(w) : bf16_rne(w);
              const uint16_t v = part == 0 ? hi : f16 ? f16_rne(w - f16_to_f32(hi)) : bf16_rne(w - bf16_to_f32(hi));
              dst[((((size_t)hc * NT + t) * 2 + part) * 2 + kg) * 256 + m * 8 + i] = v;
            }
  return true;
}

// bf16 (hi only) image for the bf16 storage path: [D/16 half-chunks][NC/32 tiles][1 KiB = k-group 2 x column 32 x k 8] in MFMA
// A-fragment lane order.  Every GEMM of that path takes an MFMA RESULT tile as its B operand (the aggregation's in the fused layer
// kernel -- gat_layer_fused.hip AggWindow --, extractor layer 1's in the lin_0 GEMM), so element i of lane half kg is
// k = 8 (i >> 2) + 4 kg + (i & 3) of the 16-k step, not 8 kg + i
static void pack_bf16_image_accop(const float *Wt, int D, int NC, float *dst_as_float) {
  uint16_t *dst = reinterpret_cast<uint16_t *>(dst_as_float);
  const int NT = NC / 32;
  for (int hc = 0; hc < D / 16; ++hc)
    for (int t = 0; t < NT; ++t)
      for (int kg = 0; kg < 2; ++kg)
        for (int m = 0; m < 32; ++m)
          for (int i = 0; i < 8; ++i)
            dst[(((size_t)hc * NT + t) * 2 + kg) * 256 + m * 8 + i] =
                bf16_rne(Wt[(size_t)(hc * 16 + 8 * (i >> 2) + 4 * kg + (i & 3)) * NC + t * 32 + m]);
}

// Alpha tile of the bf16 front GEMM (gemm_f32.hip, AMF): the attention dots alpha_src[hd] = sum_c Y[hd C + c] att_src[hd C + c]
// with Y = x W + b are x (W att) + b att.  32 weight columns behind the W image, packed like one more tile: column hd = the hi
// bf16 part of sum_c W_bf16[k][hd C + c] att_src[hd C + c], 4 + hd the same for att_dst, 8 + hd / 12 + hd the lo parts (hi + lo:
// 16 mantissa bits; W_bf16 = the rounded weights the GEMM itself multiplies by), the rest zero; then 8 floats: b att per head.
static void pack_alpha_tile(const float *Wt, const float *bias, const float *att_src, const float *att_dst, int D, int H, int C,
                            float *dst) {
  std::vector<float> Wa((size_t)D * 32, 0.0f);
  for (int k = 0; k < D; ++k)
    for (int hd = 0; hd < H; ++hd) {
      double s = 0.0, d = 0.0;
      for (int c = 0; c < C; ++c) {
        const double w = (double)bf16_to_f32(bf16_rne(Wt[(size_t)k * H * C + hd * C + c]));
        s += w * (double)att_src[hd * C + c];
        d += w * (double)att_dst[hd * C + c];
      }
      const float fs = (float)s, fd = (float)d;
      const float hs = bf16_to_f32(bf16_rne(fs)), hd_ = bf16_to_f32(bf16_rne(fd));
      Wa[(size_t)k * 32 + hd] = hs;       Wa[(size_t)k * 32 + 8 + hd] = bf16_to_f32(bf16_rne(fs - hs));
      Wa[(size_t)k * 32 + 4 + hd] = hd_;  Wa[(size_t)k * 32 + 12 + hd] = bf16_to_f32(bf16_rne(fd - hd_));
    }
  pack_bf16_image_accop(Wa.data(), D, 32, dst);
  float *cb = dst + (size_t)D / 16 * 256;
  for (int hd = 0; hd < 8; ++hd) cb[hd] = 0.0f;
  for (int hd = 0; hd < H; ++hd) {
    double s = 0.0, d = 0.0;
    for (int c = 0; c < C; ++c) {
      s += (double)(bias ? bias[hd * C + c] : 0.0f) * (double)att_src[hd * C + c];
      d += (double)(bias ? bias[hd * C + c] : 0.0f) * (double)att_dst[hd * C + c];
    }
    cb[hd] = (float)s; cb[4 + hd] = (float)d;
  }
}

// column-permuted f32 image for the fused exact-f32 kernel: column 32 t + r of a row goes to (t / TG) * 32 TG + r * TG + t % TG,
// TG = 4 / 2 / 1 tiles per LDS read (gat_layer_fused.hip: WTileGroup)
// (tg > 0 forces the group width: the lin_0 GEMM's pair-major form reads TWO tiles per ds_read_b64, gemm_f32.hip PM)
// [D][NC] -> [NC / 256][D][256]: the 256-column blocks of a wide layer, each a contiguous image for the generic GEMM
static void pack_col_blocks(const float *Wt, int D, int NC, float *dst) {
  for (int b = 0; b < NC / 256; ++b)
    for (int k = 0; k < D; ++k)
      for (int c = 0; c < 256; ++c) dst[((size_t)b * D + k) * 256 + c] = Wt[(size_t)k * NC + b * 256 + c];
}

static void pack_tilegroup_image(const float *Wt, int D, int NC, float *dst, int tg = 0) {
  const int NT = NC / 32, TG = tg > 0 ? tg : NT % 4 == 0 ? 4 : NT % 2 == 0 ? 2 : 1;
  for (int k = 0; k < D; ++k)
    for (int t = 0; t < NT; ++t)
      for (int r = 0; r < 32; ++r)
        dst[(size_t)k * NC + (t / TG) * 32 * TG + r * TG + t % TG] = Wt[(size_t)k * NC + t * 32 + r];
}

// ---- model widths the kernels have no instance for: zero padding -------------------------------------------------------------
// The kernels exist for hidden 32 / 64 / 128 and power-of-two head counts.  Any other width the reference's config allows
// (config/config.py:43-45: any gnn_hidden_channels / gnn_heads) is embedded in the next supported one: channel c of head h goes to
// column h * Cp + c, everything else is zero weight, zero bias, BatchNorm (weight 1, bias 0, mean 0, var 1).  A padded channel is
// then exactly 0.0 at every stage (Linear: 0, ReLU: 0, GATConv: alpha * 0 summed, + bias 0, BatchNorm: (0 - 0) s + 0), a padded
// head's attention logits are all leaky_relu(0) (a uniform softmax over zeros), and a real channel only ever sees added +0.0 terms:
// the results of the logical model, in another summation grouping.  Input: the flat blob in bgnn_model_weight_count's order.
static inline int pad_hidden(int c) { return c <= 32 ? 32 : c <= 64 ? 64 : 128; }
static inline int pad_heads(int h) { int p = 1; while (p < h) p <<= 1; return p; }

// logical model d, blob w in layout a -> padded model *dp, blob `out` in layout *b
static void pad_model_weights(const bgnn_model_desc *d, const WeightLayout &a, const float *w, bgnn_model_desc *dp, WeightLayout *b,
                              std::vector<float> &out) {
  const bool gat = d->gnn_type == BGNN_GNN_GAT;
  *dp = *d;
  dp->hidden = pad_hidden(d->hidden);
  if (gat) dp->heads = pad_heads(d->heads);
  *b = weight_layout(*dp);
  const int C = d->hidden, Cp = dp->hidden, Hh = d->heads, in = d->in_channels, hh = C / 2, hhp = Cp / 2, L = d->num_layers, ED = d->edge_dim;
  out.assign(b->total, 0.0f);
  // index maps: a plain width-C vector, and the concatenation of H heads of C channels
  auto ident = [](int n) { std::vector<int> m(n); for (int i = 0; i < n; ++i) m[i] = i; return m; };
  auto headmap = [&](int H) { std::vector<int> m((size_t)H * C); for (int h = 0; h < H; ++h) for (int c = 0; c < C; ++c) m[(size_t)h * C + c] = h * Cp + c; return m; };
  // matrix [rows][cols] (torch Linear weight: [out][in]) at src -> [rows_p][cols_p] at dst, vector likewise; `fill` for the pad
  // entries of a vector of n_p
  auto mat = [&](size_t src, size_t dst, const std::vector<int> &rm, const std::vector<int> &cm, int cols_p) {
    for (size_t r = 0; r < rm.size(); ++r)
      for (size_t c = 0; c < cm.size(); ++c) out[dst + (size_t)rm[r] * cols_p + cm[c]] = w[src + r * cm.size() + c];
  };
  auto vec = [&](size_t src, size_t dst, const std::vector<int> &m, int n_p = 0, float fill = 0.0f) {
    for (int i = 0; i < n_p; ++i) out[dst + i] = fill;
    for (size_t i = 0; i < m.size(); ++i) out[dst + m[i]] = w[src + i];
  };
  const std::vector<int> mC = ident(C), mIn = ident(in), mHh = ident(hh), mED = ident(ED);
  mat(a.fe_W0, b->fe_W0, mC, mIn, in); vec(a.fe_b0, b->fe_b0, mC);
  mat(a.fe_W1, b->fe_W1, mC, mC, Cp); vec(a.fe_b1, b->fe_b1, mC);
  for (int l = 0; l < L; ++l) {
    const WeightLayout::Layer &A = a.layers[l], &B = b->layers[l];
    // rows: the layer's output columns (GAT: its heads side by side; the last layer has one); columns: its input
    const std::vector<int> mOut = gat && l + 1 < L ? headmap(Hh) : mC, mInL = gat && l > 0 ? headmap(Hh) : mC;
    const int outp = (gat && l + 1 < L ? dp->heads : 1) * Cp, inp = (gat && l > 0 ? dp->heads : 1) * Cp;
    mat(A.W, B.W, mOut, mInL, inp);
    if (gat) { vec(A.as, B.as, mOut); vec(A.ad, B.ad, mOut); vec(A.ae, B.ae, mOut); mat(A.We, B.We, mOut, mED, ED); }
    if (A.W2) mat(A.W2, B.W2, mC, mC, Cp);
    if (A.b1) vec(A.b1, B.b1, mC);
    vec(A.bias, B.bias, mOut);
    vec(A.bn_w, B.bn_w, mOut, outp, 1.0f); vec(A.bn_b, B.bn_b, mOut); vec(A.bn_mean, B.bn_mean, mOut); vec(A.bn_var, B.bn_var, mOut, outp, 1.0f);
  }
  for (int k = 0; k < head_count(d); ++k) {
    const std::vector<int> mN = ident(k == 0 ? d->num_classes : 1);
    mat(a.hd_W0[k], b->hd_W0[k], mHh, mC, Cp); vec(a.hd_b0[k], b->hd_b0[k], mHh);                // mlp.0
    mat(a.hd_W1[k], b->hd_W1[k], mN, mHh, hhp); vec(a.hd_b1[k], b->hd_b1[k], mN);                // mlp.3
  }
}

// Every image of a packed model as ONE host vector, and where each lies in it.  pack() is the host packer: bgnn_model_create
// uploads its result, model_sync runs it again over the weights a refreshed model holds (the same allocation takes the result),
// and bgnn_model_refresh's gather tables come from a run over an index-valued blob (model_refresh_tables).
struct Packed {
  struct LOff { size_t Wt, as, ad, V, sc, sh, b1, Wt2, b2, tr_bias, tr_bw, tr_bb, tr_Wt; };   // tr_*: unfolded, for bgnn_forward_train
  std::vector<float> pk;
  int HT = 0;
  bool htab_ok = false, f16_ok = true;                 // f16_ok: every weight fits float16: else BGNN_SPLIT_F16 falls back to the bf16 split
  size_t o_fe_W0t = 0, o_fe_b0 = 0, o_fe_W1t = 0, o_fe_b1 = 0, o_ones = 0, o_raw = 0;
  size_t o_hW0 = 0, o_hW0t = 0, o_hb0 = 0, o_hW1 = 0, o_hb1 = 0, o_htab = 0, o_l0f_Wt = 0, o_l0f_b = 0;
  size_t o_hW0sp = 0, o_l0fsp = 0, o_hW0sp16 = 0, o_l0fsp16 = 0, o_hW0bf = 0, o_l0fbf = 0, o_hW0fp = 0, o_l0fpm = 0;
  size_t o_l0af_W = 0, o_l0af_sh = 0, o_l0f_blk = 0;
  std::vector<LOff> lo;
  std::vector<size_t> o_wsp, o_wsp16, o_wbf, o_wfp, o_plainfp, o_wblk;
  std::vector<float> inv16;                            // 2^-S of each float16 image (pack_split)
  float inv16_hd = 1.0f, inv16_l0f = 1.0f;
  void pack(const bgnn_model_desc *d, const WeightLayout &wl, const float *w);
  void assign(bgnn_model *m) const;                    // the model's pointers into m->blob (which holds pk)
};

void Packed::pack(const bgnn_model_desc *d, const WeightLayout &wl, const float *w) {
  const bool gat = d->gnn_type == BGNN_GNN_GAT;
  const int hid = d->hidden, in = d->in_channels, hh = hid / 2, L = d->num_layers, ED = d->edge_dim;
  const int nh = head_count(d);
  HT = ((nh * hh + 31) / 32) * 32;
  pk.clear();
  auto reserve = [&](size_t n) { size_t o = pk.size(); pk.resize(o + ((n + 3) & ~(size_t)3), 0.0f); return o; };
  // feature extractor
  o_fe_W0t = reserve((size_t)8 * hid), o_fe_b0 = reserve(hid);
  for (int o = 0; o < hid; ++o) for (int i = 0; i < in; ++i) pk[o_fe_W0t + (size_t)i * hid + o] = w[wl.fe_W0 + (size_t)o * in + i];
  std::copy(w + wl.fe_b0, w + wl.fe_b0 + hid, pk.begin() + o_fe_b0);
  o_fe_W1t = reserve((size_t)hid * hid), o_fe_b1 = reserve(hid);
  for (int o = 0; o < hid; ++o) for (int i = 0; i < hid; ++i) pk[o_fe_W1t + (size_t)i * hid + o] = w[wl.fe_W1 + (size_t)o * hid + i];
  std::copy(w + wl.fe_b1, w + wl.fe_b1 + hid, pk.begin() + o_fe_b1);
  lo.assign(L, LOff{});
  // BatchNorm (eval) as y = x * s + t
  auto bn_fold = [&](const float *bw, const float *bb, const float *rm, const float *rv, int c, double &sc, double &sh) {
    sc = (double)bw[c] / std::sqrt((double)rv[c] + (double)d->bn_eps);
    sh = (double)bb[c] - (double)rm[c] * sc;
  };
  for (int l = 0; l < L && !gat; ++l) {
    // every layer hid -> hid.  W^T layouts [in][out]; BatchNorm folded into the last linear map of the layer
    // (GCN: into the reduce kernel's scale / shift, because the aggregate sits between lin and bias)
    // (b0 / W1 / b1: the first bias, the second matrix and the second bias of the layer -- GIN alone has all three)
    const WeightLayout::Layer &O = wl.layers[l];
    const bool gin = d->gnn_type == BGNN_GNN_GIN;
    const float *W0 = w + O.W, *b0 = w + (gin ? O.b1 : O.bias), *W1 = w + O.W2, *b1 = w + O.bias;
    const float *bw = w + O.bn_w, *bb = w + O.bn_b, *rm = w + O.bn_mean, *rv = w + O.bn_var;
    {   // the unfolded last map of the layer (training-mode forward: BatchNorm statistics come from the batch)
      const float *rb = w + O.bias;
      lo[l].tr_bias = reserve(hid); lo[l].tr_bw = reserve(hid); lo[l].tr_bb = reserve(hid);
      std::copy(rb, rb + hid, pk.begin() + lo[l].tr_bias);
      std::copy(bw, bw + hid, pk.begin() + lo[l].tr_bw); std::copy(bb, bb + hid, pk.begin() + lo[l].tr_bb);
      lo[l].tr_Wt = 0;
      if (d->gnn_type == BGNN_GNN_SAGE) {
        lo[l].tr_Wt = reserve((size_t)2 * hid * hid);
        for (int o = 0; o < hid; ++o) for (int i = 0; i < hid; ++i) {
          pk[lo[l].tr_Wt + (size_t)i * hid + o] = W0[(size_t)o * hid + i];
          pk[lo[l].tr_Wt + (size_t)(hid + i) * hid + o] = W1[(size_t)o * hid + i];
        }
      } else if (d->gnn_type == BGNN_GNN_GIN) {
        lo[l].tr_Wt = reserve((size_t)hid * hid);
        for (int o = 0; o < hid; ++o) for (int i = 0; i < hid; ++i) pk[lo[l].tr_Wt + (size_t)i * hid + o] = W1[(size_t)o * hid + i];
      }
    }
    if (d->gnn_type == BGNN_GNN_GCN) {
      lo[l].Wt = reserve((size_t)hid * hid); lo[l].sc = reserve(hid); lo[l].sh = reserve(hid);
      for (int o = 0; o < hid; ++o) {
        for (int i = 0; i < hid; ++i) pk[lo[l].Wt + (size_t)i * hid + o] = W0[(size_t)o * hid + i];
        double sc, sh; bn_fold(bw, bb, rm, rv, o, sc, sh);
        pk[lo[l].sc + o] = (float)sc; pk[lo[l].sh + o] = (float)((double)b0[o] * sc + sh);
      }
    } else if (d->gnn_type == BGNN_GNN_SAGE) {
      lo[l].Wt = reserve((size_t)2 * hid * hid); lo[l].b2 = reserve(hid);
      for (int o = 0; o < hid; ++o) {
        double sc, sh; bn_fold(bw, bb, rm, rv, o, sc, sh);
        for (int i = 0; i < hid; ++i) {
          pk[lo[l].Wt + (size_t)i * hid + o] = (float)((double)W0[(size_t)o * hid + i] * sc);           // lin_l: mean part
          pk[lo[l].Wt + (size_t)(hid + i) * hid + o] = (float)((double)W1[(size_t)o * hid + i] * sc);     // lin_r: root part
        }
        pk[lo[l].b2 + o] = (float)((double)b0[o] * sc + sh);
      }
    } else {
      lo[l].Wt = reserve((size_t)hid * hid); lo[l].b1 = reserve(hid); lo[l].Wt2 = reserve((size_t)hid * hid); lo[l].b2 = reserve(hid);
      for (int o = 0; o < hid; ++o) {
        double sc, sh; bn_fold(bw, bb, rm, rv, o, sc, sh);
        for (int i = 0; i < hid; ++i) {
          pk[lo[l].Wt + (size_t)i * hid + o] = W0[(size_t)o * hid + i];
          pk[lo[l].Wt2 + (size_t)i * hid + o] = (float)((double)W1[(size_t)o * hid + i] * sc);
        }
        pk[lo[l].b1 + o] = b0[o];
        pk[lo[l].b2 + o] = (float)((double)b1[o] * sc + sh);
      }
    }
  }
  for (int l = 0; l < L && gat; ++l) {
    const bool last = l == L - 1;
    const int H = last ? 1 : d->heads, D = l == 0 ? hid : hid * d->heads, HC = H * hid, W = last ? hid : HC;
    const WeightLayout::Layer &O = wl.layers[l];
    lo[l].Wt = reserve((size_t)D * HC);
    for (int o = 0; o < HC; ++o) for (int i = 0; i < D; ++i) pk[lo[l].Wt + (size_t)i * HC + o] = w[O.W + (size_t)o * D + i];
    lo[l].as = reserve(HC); std::copy(w + O.as, w + O.as + HC, pk.begin() + lo[l].as);
    lo[l].ad = reserve(HC); std::copy(w + O.ad, w + O.ad + HC, pk.begin() + lo[l].ad);
    const float *att_edge = w + O.ae, *W_e = w + O.We;
    lo[l].V = reserve((size_t)H * ED);
    for (int h = 0; h < H; ++h)
      for (int f = 0; f < ED; ++f) {
        double s = 0.0;
        for (int c = 0; c < hid; ++c) s += (double)att_edge[h * hid + c] * (double)W_e[(size_t)(h * hid + c) * ED + f];
        pk[lo[l].V + (size_t)h * ED + f] = (float)s;
      }
    const float *bias = w + O.bias, *bw = w + O.bn_w, *bb = w + O.bn_b, *rm = w + O.bn_mean, *rv = w + O.bn_var;
    lo[l].sc = reserve(W); lo[l].sh = reserve(W);
    for (int c = 0; c < W; ++c) {
      const double s = (double)bw[c] / std::sqrt((double)rv[c] + (double)d->bn_eps);
      pk[lo[l].sc + c] = (float)s;
      pk[lo[l].sh + c] = (float)(((double)bias[c] - (double)rm[c]) * s + (double)bb[c]);
    }
    lo[l].tr_bias = reserve(W); lo[l].tr_bw = reserve(W); lo[l].tr_bb = reserve(W); lo[l].tr_Wt = 0;
    std::copy(bias, bias + W, pk.begin() + lo[l].tr_bias);
    std::copy(bw, bw + W, pk.begin() + lo[l].tr_bw); std::copy(bb, bb + W, pk.begin() + lo[l].tr_bb);
  }
  o_ones = reserve(512);                     // (as wide as the widest layer: heads * hidden <= 512)
  std::fill(pk.begin() + o_ones, pk.begin() + o_ones + 512, 1.0f);
  // heads: first layers concatenated column-wise, second layers packed
  o_raw = reserve(wl.total);                // the blob as given: the backward's untransposed weights
  std::copy(w, w + wl.total, pk.begin() + o_raw);
  o_hW0 = reserve((size_t)HT * hid);
  o_hW0t = reserve((size_t)hid * HT), o_hb0 = reserve(HT);
  o_hW1 = reserve((size_t)d->num_classes * hh + 2 * hh), o_hb1 = reserve(d->num_classes + 2);
  for (int k = 0; k < nh; ++k) {
    const float *W0 = w + wl.hd_W0[k], *b0 = w + wl.hd_b0[k], *W1 = w + wl.hd_W1[k], *b1 = w + wl.hd_b1[k];
    for (int o = 0; o < hh; ++o) for (int i = 0; i < hid; ++i) pk[o_hW0t + (size_t)i * HT + k * hh + o] = W0[(size_t)o * hid + i];
    std::copy(W0, W0 + (size_t)hh * hid, pk.begin() + o_hW0 + (size_t)k * hh * hid);
    std::copy(b0, b0 + hh, pk.begin() + o_hb0 + k * hh);
    const int nout = k == 0 ? d->num_classes : 1;
    const size_t woff = k == 0 ? 0 : (size_t)d->num_classes * hh + (size_t)(k - 1) * hh;
    std::copy(W1, W1 + (size_t)nout * hh, pk.begin() + o_hW1 + woff);
    const size_t boff = k == 0 ? 0 : d->num_classes + (k - 1);
    std::copy(b1, b1 + nout, pk.begin() + o_hb1 + boff);
  }
  // the fused heads kernel takes all of the above as ONE LDS image (a single DMA piece per workgroup): first-layer biases at 0,
  // second-layer row j at 96 + 32 j, second-layer biases at 288 (gat_layer_fused.hip, FusedLds::HEADW)
  o_htab = reserve(296);
  const int n_rows1 = d->num_classes + nh - 1;
  htab_ok = HT <= 96 && hh == 32 && n_rows1 <= 6;
  if (htab_ok) {
    std::copy(pk.begin() + o_hb0, pk.begin() + o_hb0 + HT, pk.begin() + o_htab);
    std::copy(pk.begin() + o_hW1, pk.begin() + o_hW1 + (size_t)n_rows1 * hh, pk.begin() + o_htab + 96);
    std::copy(pk.begin() + o_hb1, pk.begin() + o_hb1 + n_rows1, pk.begin() + o_htab + 288);
  }

  // LocalFeatureExtractor ends in a Linear without activation (gnn.py:52-68) and GATConv's lin follows directly:
  // y = z W1^T + b1, xw = y W0^T  ==>  xw = z (W1^T W0^T) + b1 W0^T.  Folded in float64, one GEMM less per forward.
  const int HC0 = (L > 1 ? d->heads : 1) * hid;
  o_l0f_Wt = reserve((size_t)hid * HC0), o_l0f_b = reserve(HC0);
  for (int o = 0; o < HC0 && gat; ++o) {
    for (int i = 0; i < hid; ++i) {
      double s = 0.0;
      for (int k = 0; k < hid; ++k) s += (double)pk[o_fe_W1t + (size_t)i * hid + k] * (double)pk[lo[0].Wt + (size_t)k * HC0 + o];
      pk[o_l0f_Wt + (size_t)i * HC0 + o] = (float)s;
    }
    double s = 0.0;
    for (int k = 0; k < hid; ++k) s += (double)pk[o_fe_b1 + k] * (double)pk[lo[0].Wt + (size_t)k * HC0 + o];
    pk[o_l0f_b + o] = (float)s;
  }

  // bf16 and float16 hi / lo images of the fused kernels' next-stage weights (layers 1.., the heads' first layers) and
  // of the folded layer-0 weight
  o_wsp.assign(L, 0); o_wsp16.assign(L, 0); o_wbf.assign(L, 0); o_wfp.assign(L, 0);
  o_hW0sp = 0, o_l0fsp = 0, o_hW0sp16 = 0, o_l0fsp16 = 0, o_hW0bf = 0, o_l0fbf = 0, o_hW0fp = 0, o_l0fpm = 0;
  f16_ok = true;                  // every weight fits float16: else BGNN_SPLIT_F16 falls back to the bf16 split
  inv16.assign(L, 1.0f);          // 2^-S of each float16 image (pack_split)
  inv16_hd = 1.0f, inv16_l0f = 1.0f;
  if (gat) {
    for (int l = 1; l < L; ++l) {
      const int H = l == L - 1 ? 1 : d->heads, D = hid * d->heads, HC = H * hid;
      o_wsp[l] = reserve((size_t)D * HC); o_wsp16[l] = reserve((size_t)D * HC); o_wbf[l] = reserve((size_t)D * HC / 2);
      o_wfp[l] = reserve((size_t)D * HC);
    }
    o_hW0fp = reserve((size_t)hid * HT);
    o_hW0sp = reserve((size_t)hid * HT); o_hW0sp16 = reserve((size_t)hid * HT); o_hW0bf = reserve((size_t)hid * HT / 2);
    if (HC0 % 64 == 0) o_l0fpm = reserve((size_t)hid * HC0);
    o_l0fsp = reserve((size_t)hid * HC0); o_l0fsp16 = reserve((size_t)hid * HC0); o_l0fbf = reserve((size_t)hid * HC0 / 2 + (size_t)hid / 16 * 256 + 8);   // + the alpha tile and its constants
    for (int l = 1; l < L; ++l) {          // (reserve may reallocate pk: take the source pointers afterwards)
      const int H = l == L - 1 ? 1 : d->heads, D = hid * d->heads, HC = H * hid;
      std::vector<float> src(pk.begin() + lo[l].Wt, pk.begin() + lo[l].Wt + (size_t)D * HC);
      pack_split(src.data(), D, HC, pk.data() + o_wsp[l], false);
      if (!pack_split(src.data(), D, HC, pk.data() + o_wsp16[l], true, &inv16[l])) f16_ok = false;
      pack_bf16_image_accop(src.data(), D, HC, pk.data() + o_wbf[l]);
      pack_tilegroup_image(src.data(), D, HC, pk.data() + o_wfp[l]);
    }
    std::vector<float> src(pk.begin() + o_hW0t, pk.begin() + o_hW0t + (size_t)hid * HT);
    pack_split(src.data(), hid, HT, pk.data() + o_hW0sp, false);
    if (!pack_split(src.data(), hid, HT, pk.data() + o_hW0sp16, true, &inv16_hd)) f16_ok = false;
    pack_bf16_image_accop(src.data(), hid, HT, pk.data() + o_hW0bf);
    pack_tilegroup_image(src.data(), hid, HT, pk.data() + o_hW0fp);
    std::vector<float> src0(pk.begin() + o_l0f_Wt, pk.begin() + o_l0f_Wt + (size_t)hid * HC0);
    pack_split(src0.data(), hid, HC0, pk.data() + o_l0fsp, false);
    if (!pack_split(src0.data(), hid, HC0, pk.data() + o_l0fsp16, true, &inv16_l0f)) f16_ok = false;
    pack_bf16_image_accop(src0.data(), hid, HC0, pk.data() + o_l0fbf);
    if (o_l0fpm) pack_tilegroup_image(src0.data(), hid, HC0, pk.data() + o_l0fpm, 2);
    if (HC0 / hid <= 4) {
      const std::vector<float> b0(pk.begin() + o_l0f_b, pk.begin() + o_l0f_b + HC0);
      const std::vector<float> as0(pk.begin() + lo[0].as, pk.begin() + lo[0].as + HC0), ad0(pk.begin() + lo[0].ad, pk.begin() + lo[0].ad + HC0);
      pack_alpha_tile(src0.data(), b0.data(), as0.data(), ad0.data(), hid, HC0 / hid, hid, pk.data() + o_l0fbf + (size_t)hid * HC0 / 2);
    }
  }

  // layer 0 "aggregate first" (bf16 path, default shape): the folded lin_0 weight as four per-head [64 k][64 columns] bf16 images
  // ([head][k-step][tile] KiB, accumulator-operand k order), and layer 0's folded shift with the folded lin_0 bias carried through the
  // BatchNorm scale (the attention coefficients of a node sum to 1: sum_j alpha_ij (W h_j + b) = W sum_j alpha_ij h_j + b)
  o_l0af_W = 0, o_l0af_sh = 0;
  if (gat && hid == 64 && L > 1 && d->heads == 4) {
    o_l0af_W = reserve((size_t)4 * 2048); o_l0af_sh = reserve(HC0);
    for (int hd = 0; hd < 4; ++hd) {
      std::vector<float> wh((size_t)hid * 64);
      for (int k = 0; k < hid; ++k)
        for (int c = 0; c < 64; ++c) wh[(size_t)k * 64 + c] = pk[o_l0f_Wt + (size_t)k * HC0 + hd * 64 + c];
      pack_bf16_image_accop(wh.data(), hid, 64, pk.data() + o_l0af_W + (size_t)hd * 2048);
    }
    for (int o = 0; o < HC0; ++o)
      pk[o_l0af_sh + o] = (float)((double)pk[lo[0].sh + o] + (double)pk[lo[0].sc + o] * (double)pk[o_l0f_b + o]);
  }

  // plain backbones (hidden 64): the layer weight in the fused layer kernel's column-permuted image (launch_fused_plain_layer)
  o_plainfp.assign(L, 0);
  if (!gat && hid == 64) {
    for (int l = 0; l < L; ++l) o_plainfp[l] = reserve((size_t)(d->gnn_type == BGNN_GNN_SAGE ? 2 : 1) * hid * hid);
    for (int l = 0; l < L; ++l) {                          // (reserve may reallocate pk: sources taken afterwards)
      const int D = (d->gnn_type == BGNN_GNN_SAGE ? 2 : 1) * hid;
      std::vector<float> src(pk.begin() + lo[l].Wt, pk.begin() + lo[l].Wt + (size_t)D * hid);
      pack_tilegroup_image(src.data(), D, hid, pk.data() + o_plainfp[l]);
    }
  }

  // layers wider than 256 columns: blocked images for the generic GEMM (layer 0: the folded and the unfolded weight)
  o_wblk.assign(L, 0);
  o_l0f_blk = 0;
  if (gat && d->heads * hid > 256) {
    for (int l = 0; l + 1 < L; ++l) o_wblk[l] = reserve((size_t)(l == 0 ? hid : hid * d->heads) * d->heads * hid);
    if (L > 1) o_l0f_blk = reserve((size_t)hid * HC0);
    for (int l = 0; l + 1 < L; ++l) {                      // (reserve may reallocate pk: sources taken afterwards)
      const int D = l == 0 ? hid : hid * d->heads, HC = d->heads * hid;
      std::vector<float> src(pk.begin() + lo[l].Wt, pk.begin() + lo[l].Wt + (size_t)D * HC);
      pack_col_blocks(src.data(), D, HC, pk.data() + o_wblk[l]);
    }
    if (o_l0f_blk) {
      std::vector<float> src0(pk.begin() + o_l0f_Wt, pk.begin() + o_l0f_Wt + (size_t)hid * HC0);
      pack_col_blocks(src0.data(), hid, HC0, pk.data() + o_l0f_blk);
    }
  }

}

void Packed::assign(bgnn_model *m) const {
  const bgnn_model_desc *d = &m->desc;
  const bool gat = d->gnn_type == BGNN_GNN_GAT;
  const int hid = d->hidden, L = d->num_layers, ED = d->edge_dim;
  m->fe_W0t = m->blob + o_fe_W0t; m->fe_b0 = m->blob + o_fe_b0; m->fe_W1t = m->blob + o_fe_W1t; m->fe_b1 = m->blob + o_fe_b1;
  m->l0f_Wt = m->blob + o_l0f_Wt; m->l0f_b = m->blob + o_l0f_b;
  m->l0f_Wsp = gat ? m->blob + o_l0fsp : nullptr;
  m->l0f_Wsp16 = gat && f16_ok ? m->blob + o_l0fsp16 : nullptr;
  m->l0f_Wsp16_inv = inv16_l0f; m->hd_W0sp16_inv = inv16_hd;
  m->l0f_Wbf = gat ? m->blob + o_l0fbf : nullptr;
  m->l0f_Wpm = gat && o_l0fpm ? m->blob + o_l0fpm : nullptr;
  m->l0f_Wt_blk = o_l0f_blk ? m->blob + o_l0f_blk : nullptr;
  m->hd_W0bf = gat ? m->blob + o_hW0bf : nullptr;
  m->hd_W0fp = gat ? m->blob + o_hW0fp : nullptr;
  m->l0af_W = o_l0af_W ? m->blob + o_l0af_W : nullptr;
  m->l0af_shift = o_l0af_sh ? m->blob + o_l0af_sh : nullptr;
  m->layers.resize(L);
  m->h_V.clear();
  for (int l = 0; l < L && !gat; ++l) {
    BgnnLayer &Ly = m->layers[l];
    Ly = BgnnLayer{};
    Ly.heads = 1; Ly.d_in = hid; Ly.width = hid; Ly.concat = l != L - 1;
    Ly.Wt = m->blob + lo[l].Wt;
    if (d->gnn_type == BGNN_GNN_GCN) { Ly.scale = m->blob + lo[l].sc; Ly.shift = m->blob + lo[l].sh; }
    if (d->gnn_type == BGNN_GNN_SAGE) Ly.b2 = m->blob + lo[l].b2;
    if (d->gnn_type == BGNN_GNN_GIN) { Ly.b1 = m->blob + lo[l].b1; Ly.Wt2 = m->blob + lo[l].Wt2; Ly.b2 = m->blob + lo[l].b2; }
    Ly.tr_bias = m->blob + lo[l].tr_bias; Ly.bn_w = m->blob + lo[l].tr_bw; Ly.bn_b = m->blob + lo[l].tr_bb;
    Ly.tr_Wt = lo[l].tr_Wt ? m->blob + lo[l].tr_Wt : nullptr;
    Ly.Wfp = o_plainfp[l] ? m->blob + o_plainfp[l] : nullptr;
  }
  m->ones = m->blob + o_ones;
  for (int l = 0; l < L && gat; ++l) {
    const bool last = l == L - 1;
    BgnnLayer &Ly = m->layers[l];
    Ly.heads = last ? 1 : d->heads; Ly.d_in = l == 0 ? hid : hid * d->heads;
    Ly.width = last ? hid : Ly.heads * hid; Ly.concat = !last;
    Ly.Wt = m->blob + lo[l].Wt; Ly.att_src = m->blob + lo[l].as; Ly.att_dst = m->blob + lo[l].ad;
    Ly.Wt_blk = o_wblk[l] ? m->blob + o_wblk[l] : nullptr;
    Ly.V = m->blob + lo[l].V; Ly.scale = m->blob + lo[l].sc; Ly.shift = m->blob + lo[l].sh;
    Ly.Wsp = l > 0 ? m->blob + o_wsp[l] : nullptr;
    Ly.Wsp16 = l > 0 && f16_ok ? m->blob + o_wsp16[l] : nullptr;
    Ly.Wsp16_inv = inv16[l];
    Ly.Wbf = l > 0 ? m->blob + o_wbf[l] : nullptr;
    Ly.Wfp = l > 0 ? m->blob + o_wfp[l] : nullptr;
    Ly.tr_bias = m->blob + lo[l].tr_bias; Ly.bn_w = m->blob + lo[l].tr_bw; Ly.bn_b = m->blob + lo[l].tr_bb;
  }
  for (int l = 0; l < L && gat; ++l) {                 // host copy of the folded edge vectors (model_canonical_V)
    const int H = l == L - 1 ? 1 : d->heads;
    m->h_V.insert(m->h_V.end(), pk.begin() + lo[l].V, pk.begin() + lo[l].V + (size_t)H * ED);
  }
  m->head_hidden_total = HT;
  m->hd_W0sp = gat ? m->blob + o_hW0sp : nullptr;
  m->hd_W0sp16 = gat && f16_ok ? m->blob + o_hW0sp16 : nullptr;
  m->hd_W0t = m->blob + o_hW0t; m->hd_b0 = m->blob + o_hb0; m->hd_W1 = m->blob + o_hW1; m->hd_b1 = m->blob + o_hb1;
  m->hd_tab = htab_ok ? m->blob + o_htab : nullptr;
  m->raw = m->blob + o_raw; m->hd_W0 = m->blob + o_hW0;
}

static int model_create_native(bgnn_ctx *ctx, const bgnn_model_desc *d, WeightLayout &&wl, const float *w, bgnn_model **out) {
  // (the generic kernels take 32 / 64 / 128 as long as a layer stays within 256 columns -- the heads' hidden/2 has to be a multiple of
  //  16 and their three first layers side by side a multiple of 32; the fused kernels exist for hidden 64 only, the reference's
  //  default: config/config.py:41)
  BGNN_REQUIRE(d->hidden == 32 || d->hidden == 64 || d->hidden == 128, "hidden_channels=%d unsupported (32, 64 or 128)", d->hidden);
  BGNN_REQUIRE(d->in_channels >= 1 && d->in_channels <= 8, "in_channels=%d unsupported (1..8)", d->in_channels);
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
  Packed P;
  P.pack(d, wl, w);
  const std::vector<float> &pk = P.pk;
  bgnn_model *m = new bgnn_model();
  m->ctx = ctx; m->desc = *d; m->weights = std::move(wl); m->blob_floats = pk.size();
  hipError_t e = hipMalloc((void **)&m->blob, pk.size() * sizeof(float));
  if (e != hipSuccess) { delete m; set_error("hipMalloc(model) failed: %s", hipGetErrorString(e)); return BGNN_ERR_NOMEM; }
  e = hipMemcpy(m->blob, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(m->blob); delete m; set_error("hipMemcpy(model) failed: %s", hipGetErrorString(e)); return BGNN_ERR_HIP; }
  P.assign(m);
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

// Stale eval images (bgnn_model_refresh rewrote only what training reads): the host packer over the weights the model holds, into
// the allocation it has.  Waits for the stream twice (download, upload from pageable memory).
int model_sync_slow(bgnn_ctx *ctx, bgnn_model *m) {
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  std::vector<float> w(m->weights.total);
  BGNN_HIP_CHECK(hipMemcpyAsync(w.data(), m->raw, w.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  BGNN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  Packed P;
  P.pack(&m->desc, m->weights, w.data());
  BGNN_REQUIRE(P.pk.size() == m->blob_floats, "model_sync: the repacked model has %zu floats, the live one %zu", P.pk.size(), m->blob_floats);
  BGNN_HIP_CHECK(hipMemcpyAsync(m->blob, P.pk.data(), P.pk.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  BGNN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  P.assign(m);                                         // (the float16 images may have come or gone with the weights' range; h_V)
  for (auto &kv : m->v3_tables) (void)hipFree(kv.second);   // (the stream is idle: nothing reads them; remade on demand)
  m->v3_tables.clear();
  m->eval_stale = false;
  return BGNN_OK;
}

// The gather tables of bgnn_model_refresh.  The host packer runs over a blob whose element i holds i + 1 (exact in float32 below
// 2^24): wherever an image is a plain copy of a weight -- transposes, concatenations, stacked heads, column blocks -- the packed
// value names its source, and a 0 is padding that stays 0.  Only the images the training path reads are taken (the others hold
// products of indices); the re-layouts of the folded layer-0 weight come from the same packers over an index-valued l0f_Wt.
int model_refresh_tables(bgnn_ctx *ctx, bgnn_model *m) {
  if (m->refresh) return BGNN_OK;
  const bgnn_model_desc *d = &m->desc;
  const WeightLayout &wl = m->weights;
  const size_t total = wl.total;
  if (total >= ((size_t)1 << 24) || m->blob_floats >= ((size_t)1 << 31)) {
    set_error("bgnn_model_refresh: a model of %zu weights is beyond the gather tables (2^24)", total);
    return BGNN_ERR_UNSUPPORTED;
  }
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const bool gat = d->gnn_type == BGNN_GNN_GAT;
  const int hid = d->hidden, L = d->num_layers, ED = d->edge_dim, hh = hid / 2;
  std::vector<float> probe(total);
  for (size_t i = 0; i < total; ++i) probe[i] = (float)(i + 1);
  Packed P;
  P.pack(d, wl, probe.data());
  BGNN_REQUIRE(P.pk.size() == m->blob_floats, "bgnn_model_refresh: the probe pack has %zu floats, the live model %zu", P.pk.size(), m->blob_floats);
  std::vector<int32_t> copy, relay, vjob;
  bool ok = true;
  auto take = [&](size_t off, size_t n) {
    for (size_t i = off; i < off + n; ++i) {
      const float v = P.pk[i];
      if (v == 0.0f) continue;
      if (!(v >= 1.0f && v <= (float)total && v == std::floor(v))) { ok = false; continue; }
      copy.push_back((int32_t)i); copy.push_back((int32_t)v - 1);
    }
  };
  const size_t HT = (size_t)P.HT;
  take(P.o_fe_W0t, (size_t)8 * hid); take(P.o_fe_b0, hid); take(P.o_fe_W1t, (size_t)hid * hid); take(P.o_fe_b1, hid);
  for (int l = 0; l < L; ++l) {
    const Packed::LOff &O = P.lo[l];
    const BgnnLayer &Ly = m->layers[l];
    const size_t W = (size_t)Ly.width;
    take(O.tr_bias, W); take(O.tr_bw, W); take(O.tr_bb, W);
    if (gat) {
      const size_t HC = (size_t)Ly.heads * hid;
      take(O.Wt, (size_t)Ly.d_in * HC); take(O.as, HC); take(O.ad, HC);
      if (P.o_wblk[l]) take(P.o_wblk[l], (size_t)Ly.d_in * HC);
      for (int h = 0; h < Ly.heads; ++h)
        for (int f = 0; f < ED; ++f) {
          vjob.push_back((int32_t)(O.V + (size_t)h * ED + f));
          vjob.push_back((int32_t)(wl.layers[l].ae + (size_t)h * hid));
          vjob.push_back((int32_t)(wl.layers[l].We + (size_t)h * hid * ED + f));
          vjob.push_back(0);
        }
    } else if (d->gnn_type == BGNN_GNN_GCN) {
      take(O.Wt, (size_t)hid * hid);
    } else if (d->gnn_type == BGNN_GNN_SAGE) {
      take(O.tr_Wt, (size_t)2 * hid * hid);
    } else {
      take(O.Wt, (size_t)hid * hid); take(O.b1, hid); take(O.tr_Wt, (size_t)hid * hid);
    }
  }
  take(P.o_hW0, HT * hid); take(P.o_hW0t, (size_t)hid * HT); take(P.o_hb0, HT);
  take(P.o_hW1, (size_t)d->num_classes * hh + 2 * hh); take(P.o_hb1, (size_t)d->num_classes + 2);
  BGNN_REQUIRE(ok, "bgnn_model_refresh: an image taken for a plain copy of the weights is none (internal)");
  RefreshTables *T = new RefreshTables();
  if (gat) {
    const int HC0 = m->layers[0].heads * hid;
    const size_t n0 = (size_t)hid * HC0;
    T->fold_cols = HC0; T->fe_W1 = (int32_t)wl.fe_W1; T->fe_b1 = (int32_t)wl.fe_b1; T->W0 = (int32_t)wl.layers[0].W;
    T->l0f_Wt = (int32_t)P.o_l0f_Wt; T->l0f_b = (int32_t)P.o_l0f_b;
    std::vector<float> idx(n0), img(n0);
    for (size_t i = 0; i < n0; ++i) idx[i] = (float)(i + 1);
    auto relay_of = [&](size_t dst) {
      for (size_t i = 0; i < n0; ++i) { relay.push_back((int32_t)(dst + i)); relay.push_back((int32_t)(P.o_l0f_Wt + (size_t)img[i] - 1)); }
    };
    if (P.o_l0fpm) { pack_tilegroup_image(idx.data(), hid, HC0, img.data(), 2); relay_of(P.o_l0fpm); }
    if (P.o_l0f_blk) { pack_col_blocks(idx.data(), hid, HC0, img.data()); relay_of(P.o_l0f_blk); }
  }
  T->n_copy = (int32_t)(copy.size() / 2); T->n_relay = (int32_t)(relay.size() / 2); T->n_vjob = (int32_t)(vjob.size() / 4);
  std::vector<int32_t> all;
  all.insert(all.end(), copy.begin(), copy.end());
  all.insert(all.end(), relay.begin(), relay.end());
  all.insert(all.end(), vjob.begin(), vjob.end());
  all.push_back(0);                                    // (never an empty allocation)
  hipError_t e = hipMalloc((void **)&T->dev, all.size() * sizeof(int32_t));
  if (e != hipSuccess) { delete T; set_error("hipMalloc(refresh tables) failed: %s", hipGetErrorString(e)); return BGNN_ERR_NOMEM; }
  e = hipMemcpy(T->dev, all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(T->dev); delete T; set_error("hipMemcpy(refresh tables) failed: %s", hipGetErrorString(e)); return BGNN_ERR_HIP; }
  T->d_copy = T->dev; T->d_relay = T->d_copy + copy.size(); T->d_vjob = T->d_relay + relay.size();
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
  BGNN_REQUIRE(dl.in_channels >= 1 && dl.in_channels <= 8, "in_channels=%d unsupported (1..8)", dl.in_channels);
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
