// The images of a packed model: what the device blob of a bgnn_model holds, where, and how each image is made from the weight
// blob.  Host arithmetic only -- the C ABI's structures and the standard library, nothing from HIP -- so that the layout and the
// packers can be compiled and checked on their own (tests/pack_host_check.cpp).  Three passes over one table:
//   image_map     the layout: every image's {offset, floats, flags}, a pure function of the model description
//   fill_images   the values: every image written into a zeroed buffer of map.total floats, sources read in place
//   refresh_plan  the tables of bgnn_model_refresh: how the images the training path reads follow a new weight blob
// model_pack.hip owns the device side: allocation, upload, the model's pointers.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/bgnn.h"

namespace bgnn {

inline int head_count(const bgnn_model_desc *d) { return d->predict_correction ? 3 : 2; }

// Offsets (in floats) of every tensor of the weight blob (bgnn_model_weight_count order) -- of the gradient blob as well; filled by
// weight_layout.
// Layer slots: GAT  W = lin.weight, as / ad / ae = att_src / att_dst / att_edge, We = lin_edge.weight, bias;
//              GCN  W = lin.weight, bias;  GraphSAGE  W = lin_l.weight, bias = lin_l.bias, W2 = lin_r.weight;
//              GIN  W = nn.0.weight, b1 = nn.0.bias, W2 = nn.2.weight, bias = nn.2.bias;
// then every backbone's BatchNorm weight / bias / running_mean / running_var.  Slots a backbone does not have stay 0.
struct WeightLayout {
  size_t fe_W0, fe_b0, fe_W1, fe_b1;
  struct Layer { size_t W, as, ad, ae, We, bias, bn_w, bn_b, bn_mean, bn_var, W2, b1; };
  std::vector<Layer> layers;
  size_t hd_W0[3], hd_b0[3], hd_W1[3], hd_b1[3];   // per head: mlp.0 weight / bias, mlp.3 weight / bias
  size_t total;
};

// The one place that knows which tensors the weight blob holds, in which order and with which shapes (include/bgnn.h,
// bgnn_model_weight_count; models/gnn.py _blob_slots is its Python twin).
inline WeightLayout weight_layout(const bgnn_model_desc &d) {
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
inline bool pack_split(const float *Wt, int D, int NC, float *dst_as_float, bool f16, float *inv_scale = nullptr) {
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
inline void pack_bf16_image_accop(const float *Wt, int D, int NC, float *dst_as_float) {
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
inline void pack_alpha_tile(const float *Wt, const float *bias, const float *att_src, const float *att_dst, int D, int H, int C,
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


// [D][NC] -> [NC / 256][D][256]: the 256-column blocks of a wide layer, each a contiguous image for the generic GEMM
inline void pack_col_blocks(const float *Wt, int D, int NC, float *dst) {
  for (int b = 0; b < NC / 256; ++b)
    for (int k = 0; k < D; ++k)
      for (int c = 0; c < 256; ++c) dst[((size_t)b * D + k) * 256 + c] = Wt[(size_t)k * NC + b * 256 + c];
}

// column-permuted f32 image for the fused exact-f32 kernel: column 32 t + r of a row goes to (t / TG) * 32 TG + r * TG + t % TG,
// TG = 4 / 2 / 1 tiles per LDS read (gat_layer_fused.hip: WTileGroup)
// (tg > 0 forces the group width: the lin_0 GEMM's pair-major form reads TWO tiles per ds_read_b64, gemm_f32.hip PM)
inline void pack_tilegroup_image(const float *Wt, int D, int NC, float *dst, int tg = 0) {
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
inline void pad_model_weights(const bgnn_model_desc *d, const WeightLayout &a, const float *w, bgnn_model_desc *dp, WeightLayout *b,
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

// ---- the image table ---------------------------------------------------------------------------------------------------------
// Every image is declared ONCE: its name here (the name of the bgnn_model / BgnnLayer pointer that ends up on it), its extent and
// flags in image_map.  An image of 0 floats does not exist for the model's shape.
//   IMG_TRAIN  bgnn_forward_train* or bgnn_backward read it and it follows the weights: bgnn_model_refresh has to rewrite it
//              (`raw` is read there too, but bgnn_model_refresh copies the new blob onto it itself; `ones` never changes)
//   IMG_COPY   every element is one weight, or padding 0
//   IMG_RELAY  every element is one element of l0f_Wt (fill_relays)
//   neither:   derived arithmetically
constexpr unsigned IMG_TRAIN = 1, IMG_COPY = 2, IMG_RELAY = 4;
struct Image {
  size_t off = 0, floats = 0;
  unsigned flags = 0;
};
#define BGNN_MODEL_IMAGES(X)                                                                                                    \
  X(fe_W0t) X(fe_b0) X(fe_W1t) X(fe_b1) X(ones) X(raw) X(hd_W0) X(hd_W0t) X(hd_b0) X(hd_W1) X(hd_b1) X(hd_tab) X(l0f_Wt) X(l0f_b) \
  X(hd_W0fp) X(hd_W0sp) X(hd_W0sp16) X(hd_W0bf) X(l0f_Wpm) X(l0f_Wsp) X(l0f_Wsp16) X(l0f_Wbf) X(l0af_W) X(l0af_shift) X(l0f_Wt_blk)
#define BGNN_LAYER_IMAGES(X)                                                                                                    \
  X(Wt) X(att_src) X(att_dst) X(V) X(scale) X(shift) X(b1) X(Wt2) X(b2) X(tr_bias) X(bn_w) X(bn_b) X(tr_Wt) X(Wsp) X(Wsp16) X(Wbf) \
  X(Wfp) X(Wt_blk)
struct ImageMap {
#define X(name) Image name;
  struct Layer { BGNN_LAYER_IMAGES(X) };
  BGNN_MODEL_IMAGES(X)
#undef X
  std::vector<Layer> layers;
  size_t total = 0;          // floats of the whole blob
  int HT = 0;                // the heads' first layers side by side, padded to a multiple of 32
  bool htab_ok = false;      // hd_tab is filled (the fused heads epilogue's shape); else it exists and stays zero
  // f(name, layer or -1, image) for every image that exists
  template <class F> void for_each(F f) const {
#define X(name) if (name.floats) f(#name, -1, name);
    BGNN_MODEL_IMAGES(X)
#undef X
#define X(name) if (layers[l].name.floats) f(#name, (int)l, layers[l].name);
    for (size_t l = 0; l < layers.size(); ++l) { BGNN_LAYER_IMAGES(X) }
#undef X
  }
};

// Rows of the first extractor image fe_W0t = the K of its GEMM: the node table's 8 columns, or the wide table's 16
inline int extractor_rows(int in_channels) { return in_channels > 8 ? 16 : 8; }

// The layout pass.  Images lie in the order of the put() calls, each rounded up to 4 floats.
inline ImageMap image_map(const bgnn_model_desc &d) {
  const bool gat = d.gnn_type == BGNN_GNN_GAT, sage = d.gnn_type == BGNN_GNN_SAGE, gin = d.gnn_type == BGNN_GNN_GIN;
  const size_t hid = d.hidden, hh = hid / 2, heads = d.heads, ED = d.edge_dim, nc = d.num_classes;
  const int L = d.num_layers, nh = head_count(&d);
  const unsigned TC = IMG_TRAIN | IMG_COPY;
  ImageMap m;
  m.HT = (int)((nh * hh + 31) / 32) * 32;
  m.htab_ok = m.HT <= 96 && hh == 32 && nc + nh - 1 <= 6;
  const size_t HT = m.HT, HC0 = (L > 1 ? heads : 1) * hid;
  auto put = [&](Image &im, size_t n, unsigned flags = 0) { im.off = m.total; im.floats = n; im.flags = flags; m.total += (n + 3) & ~(size_t)3; };
  // feature extractor: W^T layouts [in, 8 rows][out] (in_channels > 8: 16 rows, the wide node table of bgnn_aux.h)
  put(m.fe_W0t, extractor_rows(d.in_channels) * hid, TC); put(m.fe_b0, hid, TC); put(m.fe_W1t, hid * hid, TC); put(m.fe_b1, hid, TC);
  m.layers.resize(L);
  for (int l = 0; l < L; ++l) {
    ImageMap::Layer &M = m.layers[l];
    if (gat) {
      const size_t H = l == L - 1 ? 1 : heads, D = l == 0 ? hid : hid * heads, HC = H * hid;
      put(M.Wt, D * HC, TC); put(M.att_src, HC, TC); put(M.att_dst, HC, TC);
      put(M.V, H * ED, IMG_TRAIN);                                   // att_edge . lin_edge
      put(M.scale, HC); put(M.shift, HC);                            // BatchNorm (eval) as y = x * s + t, the bias folded in
      put(M.tr_bias, HC, TC); put(M.bn_w, HC, TC); put(M.bn_b, HC, TC);
      continue;
    }
    // every layer hid -> hid.  tr_*: the unfolded last map of the layer (training-mode forward: BatchNorm statistics come from the batch)
    put(M.tr_bias, hid, TC); put(M.bn_w, hid, TC); put(M.bn_b, hid, TC);
    if (sage) put(M.tr_Wt, 2 * hid * hid, TC);
    if (gin) put(M.tr_Wt, hid * hid, TC);
    // W^T layouts [in][out]; BatchNorm folded into the last linear map of the layer (GCN: into the reduce kernel's scale / shift,
    // because the aggregate sits between lin and bias)
    if (sage) { put(M.Wt, 2 * hid * hid); put(M.b2, hid); }
    else if (gin) { put(M.Wt, hid * hid, TC); put(M.b1, hid, TC); put(M.Wt2, hid * hid); put(M.b2, hid); }
    else { put(M.Wt, hid * hid, TC); put(M.scale, hid); put(M.shift, hid); }
  }
  put(m.ones, 512);                                                  // (as wide as the widest layer: heads * hidden <= 512)
  put(m.raw, weight_layout(d).total, IMG_COPY);                      // the blob as given: the backward's untransposed weights
  // heads: first layers stacked (hd_W0) and concatenated column-wise (hd_W0t), second layers packed
  put(m.hd_W0, HT * hid, TC); put(m.hd_W0t, hid * HT, TC); put(m.hd_b0, HT, TC);
  put(m.hd_W1, nc * hh + 2 * hh, TC); put(m.hd_b1, nc + 2, TC);
  // the fused heads kernel takes all of the above as ONE LDS image (a single DMA piece per workgroup): first-layer biases at 0,
  // second-layer row j at 96 + 32 j, second-layer biases at 288 (gat_layer_fused.hip, FusedLds::HEADW)
  put(m.hd_tab, 296);
  // the extractor's second Linear folded into lin of layer 0 (fill_images); zero for the other backbones
  put(m.l0f_Wt, hid * HC0, gat ? IMG_TRAIN : 0); put(m.l0f_b, HC0, gat ? IMG_TRAIN : 0);
  if (gat) {
    // bf16 and float16 hi / lo images, the bf16 (hi only) image and the column-permuted f32 image of the fused kernels' next-stage
    // weights (layers 1.., the heads' first layers) and of the folded layer-0 weight
    for (int l = 1; l < L; ++l) {
      ImageMap::Layer &M = m.layers[l];
      const size_t n = M.Wt.floats;
      put(M.Wsp, n); put(M.Wsp16, n); put(M.Wbf, n / 2); put(M.Wfp, n, IMG_COPY);
    }
    put(m.hd_W0fp, hid * HT, IMG_COPY); put(m.hd_W0sp, hid * HT); put(m.hd_W0sp16, hid * HT); put(m.hd_W0bf, hid * HT / 2);
    if (HC0 % 64 == 0) put(m.l0f_Wpm, hid * HC0, IMG_TRAIN | IMG_RELAY);
    put(m.l0f_Wsp, hid * HC0); put(m.l0f_Wsp16, hid * HC0);
    put(m.l0f_Wbf, hid * HC0 / 2 + hid / 16 * 256 + 8);              // + the alpha tile and its constants
    // layer 0 "aggregate first" (bf16 path, default shape): four per-head bf16 images of l0f_Wt, and layer 0's shift with l0f_b in it
    if (hid == 64 && L > 1 && heads == 4) { put(m.l0af_W, 4 * 2048); put(m.l0af_shift, HC0); }
    // layers wider than 256 columns: blocked images for the generic GEMM (layer 0: the folded and the unfolded weight)
    if (heads * hid > 256) {
      for (int l = 0; l + 1 < L; ++l) put(m.layers[l].Wt_blk, m.layers[l].Wt.floats, TC);
      if (L > 1) put(m.l0f_Wt_blk, hid * HC0, IMG_TRAIN | IMG_RELAY);
    }
  } else if (hid == 64) {
    // plain backbones (hidden 64): the layer weight in the fused layer kernel's column-permuted image (launch_fused_plain_layer)
    for (int l = 0; l < L; ++l) put(m.layers[l].Wfp, m.layers[l].Wt.floats, sage ? 0 : IMG_COPY);
  }
  return m;
}

// What a fill finds out about the weight VALUES (everything else about a packed model follows from its description)
struct PackValues {
  bool f16_ok = true;                      // every weight fits float16: else BGNN_SPLIT_F16 falls back to the bf16 split
  std::vector<float> inv16;                // 2^-S of each layer's float16 image (pack_split) ...
  float inv16_hd = 1.0f, inv16_l0f = 1.0f; // ... of the heads' and of the folded layer-0 weight's
  std::vector<float> h_V;                  // every GAT layer's V: [layers][heads_l][edge_dim]
};

// Every RELAY image from the l0f_Wt that dst holds
inline void fill_relays(const bgnn_model_desc &d, const ImageMap &map, float *dst) {
  const int hid = d.hidden, HC0 = (int)map.l0f_b.floats;
  if (map.l0f_Wpm.floats) pack_tilegroup_image(dst + map.l0f_Wt.off, hid, HC0, dst + map.l0f_Wpm.off, 2);
  if (map.l0f_Wt_blk.floats) pack_col_blocks(dst + map.l0f_Wt.off, hid, HC0, dst + map.l0f_Wt_blk.off);
}

// The fill pass: weights w (layout wl) -> every image of `map`, in dst [map.total], which comes in zeroed.
inline void fill_images(const bgnn_model_desc &d, const WeightLayout &wl, const ImageMap &map, const float *w, float *dst, PackValues *pv) {
  const bool gat = d.gnn_type == BGNN_GNN_GAT, sage = d.gnn_type == BGNN_GNN_SAGE, gin = d.gnn_type == BGNN_GNN_GIN;
  const int hid = d.hidden, in = d.in_channels, hh = hid / 2, L = d.num_layers, ED = d.edge_dim, HT = map.HT, nh = head_count(&d);
  auto at = [&](const Image &im) { return dst + im.off; };
  // feature extractor
  for (int o = 0; o < hid; ++o) for (int i = 0; i < in; ++i) at(map.fe_W0t)[(size_t)i * hid + o] = w[wl.fe_W0 + (size_t)o * in + i];
  std::copy(w + wl.fe_b0, w + wl.fe_b0 + hid, at(map.fe_b0));
  for (int o = 0; o < hid; ++o) for (int i = 0; i < hid; ++i) at(map.fe_W1t)[(size_t)i * hid + o] = w[wl.fe_W1 + (size_t)o * hid + i];
  std::copy(w + wl.fe_b1, w + wl.fe_b1 + hid, at(map.fe_b1));
  *pv = PackValues();
  pv->inv16.assign(L, 1.0f);
  // BatchNorm (eval) as y = x * s + t
  auto bn_fold = [&](const float *bw, const float *bb, const float *rm, const float *rv, int c, double &sc, double &sh) {
    sc = (double)bw[c] / std::sqrt((double)rv[c] + (double)d.bn_eps);
    sh = (double)bb[c] - (double)rm[c] * sc;
  };
  for (int l = 0; l < L && !gat; ++l) {
    // (b0 / W1 / b1: the first bias, the second matrix and the second bias of the layer -- GIN alone has all three)
    const WeightLayout::Layer &O = wl.layers[l];
    const ImageMap::Layer &M = map.layers[l];
    const float *W0 = w + O.W, *b0 = w + (gin ? O.b1 : O.bias), *W1 = w + O.W2, *b1 = w + O.bias;
    const float *bw = w + O.bn_w, *bb = w + O.bn_b, *rm = w + O.bn_mean, *rv = w + O.bn_var;
    std::copy(b1, b1 + hid, at(M.tr_bias));
    std::copy(bw, bw + hid, at(M.bn_w)); std::copy(bb, bb + hid, at(M.bn_b));
    float *Wt = at(M.Wt);
    if (sage) {
      for (int o = 0; o < hid; ++o) for (int i = 0; i < hid; ++i) {
        at(M.tr_Wt)[(size_t)i * hid + o] = W0[(size_t)o * hid + i];
        at(M.tr_Wt)[(size_t)(hid + i) * hid + o] = W1[(size_t)o * hid + i];
      }
      for (int o = 0; o < hid; ++o) {
        double sc, sh; bn_fold(bw, bb, rm, rv, o, sc, sh);
        for (int i = 0; i < hid; ++i) {
          Wt[(size_t)i * hid + o] = (float)((double)W0[(size_t)o * hid + i] * sc);             // lin_l: mean part
          Wt[(size_t)(hid + i) * hid + o] = (float)((double)W1[(size_t)o * hid + i] * sc);     // lin_r: root part
        }
        at(M.b2)[o] = (float)((double)b0[o] * sc + sh);
      }
    } else if (gin) {
      for (int o = 0; o < hid; ++o) {
        double sc, sh; bn_fold(bw, bb, rm, rv, o, sc, sh);
        for (int i = 0; i < hid; ++i) {
          at(M.tr_Wt)[(size_t)i * hid + o] = W1[(size_t)o * hid + i];
          Wt[(size_t)i * hid + o] = W0[(size_t)o * hid + i];
          at(M.Wt2)[(size_t)i * hid + o] = (float)((double)W1[(size_t)o * hid + i] * sc);
        }
        at(M.b1)[o] = b0[o];
        at(M.b2)[o] = (float)((double)b1[o] * sc + sh);
      }
    } else {
      for (int o = 0; o < hid; ++o) {
        for (int i = 0; i < hid; ++i) Wt[(size_t)i * hid + o] = W0[(size_t)o * hid + i];
        double sc, sh; bn_fold(bw, bb, rm, rv, o, sc, sh);
        at(M.scale)[o] = (float)sc; at(M.shift)[o] = (float)((double)b0[o] * sc + sh);
      }
    }
    if (M.Wfp.floats) pack_tilegroup_image(Wt, (sage ? 2 : 1) * hid, hid, at(M.Wfp));
  }
  for (int l = 0; l < L && gat; ++l) {
    const int H = l == L - 1 ? 1 : d.heads, D = l == 0 ? hid : hid * d.heads, HC = H * hid;
    const WeightLayout::Layer &O = wl.layers[l];
    const ImageMap::Layer &M = map.layers[l];
    for (int o = 0; o < HC; ++o) for (int i = 0; i < D; ++i) at(M.Wt)[(size_t)i * HC + o] = w[O.W + (size_t)o * D + i];
    std::copy(w + O.as, w + O.as + HC, at(M.att_src));
    std::copy(w + O.ad, w + O.ad + HC, at(M.att_dst));
    const float *att_edge = w + O.ae, *W_e = w + O.We;
    for (int h = 0; h < H; ++h)
      for (int f = 0; f < ED; ++f) {
        double s = 0.0;
        for (int c = 0; c < hid; ++c) s += (double)att_edge[h * hid + c] * (double)W_e[(size_t)(h * hid + c) * ED + f];
        at(M.V)[(size_t)h * ED + f] = (float)s;
      }
    pv->h_V.insert(pv->h_V.end(), at(M.V), at(M.V) + (size_t)H * ED);
    // (this fold is NOT bn_fold's: ((bias - mean) * s) + bn_b rounds differently from bias * s + (bn_b - mean * s))
    const float *bias = w + O.bias, *bw = w + O.bn_w, *bb = w + O.bn_b, *rm = w + O.bn_mean, *rv = w + O.bn_var;
    for (int c = 0; c < HC; ++c) {
      const double s = (double)bw[c] / std::sqrt((double)rv[c] + (double)d.bn_eps);
      at(M.scale)[c] = (float)s;
      at(M.shift)[c] = (float)(((double)bias[c] - (double)rm[c]) * s + (double)bb[c]);
    }
    std::copy(bias, bias + HC, at(M.tr_bias));
    std::copy(bw, bw + HC, at(M.bn_w)); std::copy(bb, bb + HC, at(M.bn_b));
    if (M.Wt_blk.floats) pack_col_blocks(at(M.Wt), D, HC, at(M.Wt_blk));
    if (l == 0) continue;
    pack_split(at(M.Wt), D, HC, at(M.Wsp), false);
    if (!pack_split(at(M.Wt), D, HC, at(M.Wsp16), true, &pv->inv16[l])) pv->f16_ok = false;
    pack_bf16_image_accop(at(M.Wt), D, HC, at(M.Wbf));
    pack_tilegroup_image(at(M.Wt), D, HC, at(M.Wfp));
  }
  std::fill(at(map.ones), at(map.ones) + 512, 1.0f);
  std::copy(w, w + wl.total, at(map.raw));
  for (int k = 0; k < nh; ++k) {
    const float *W0 = w + wl.hd_W0[k], *b0 = w + wl.hd_b0[k], *W1 = w + wl.hd_W1[k], *b1 = w + wl.hd_b1[k];
    for (int o = 0; o < hh; ++o) for (int i = 0; i < hid; ++i) at(map.hd_W0t)[(size_t)i * HT + k * hh + o] = W0[(size_t)o * hid + i];
    std::copy(W0, W0 + (size_t)hh * hid, at(map.hd_W0) + (size_t)k * hh * hid);
    std::copy(b0, b0 + hh, at(map.hd_b0) + k * hh);
    const int nout = k == 0 ? d.num_classes : 1;
    std::copy(W1, W1 + (size_t)nout * hh, at(map.hd_W1) + (k == 0 ? 0 : (size_t)d.num_classes * hh + (size_t)(k - 1) * hh));
    std::copy(b1, b1 + nout, at(map.hd_b1) + (k == 0 ? 0 : d.num_classes + (k - 1)));
  }
  if (map.htab_ok) {
    const int n_rows1 = d.num_classes + nh - 1;
    std::copy(at(map.hd_b0), at(map.hd_b0) + HT, at(map.hd_tab));
    std::copy(at(map.hd_W1), at(map.hd_W1) + (size_t)n_rows1 * hh, at(map.hd_tab) + 96);
    std::copy(at(map.hd_b1), at(map.hd_b1) + n_rows1, at(map.hd_tab) + 288);
  }
  if (!gat) return;

  // LocalFeatureExtractor ends in a Linear without activation (gnn.py:52-68) and GATConv's lin follows directly:
  // y = z W1^T + b1, xw = y W0^T  ==>  xw = z (W1^T W0^T) + b1 W0^T.  Folded in float64, one GEMM less per forward.
  // (optimizer.hip refresh_fold_kernel restates these sums, k ascending)
  const int HC0 = (int)map.l0f_b.floats;
  const ImageMap::Layer &M0 = map.layers[0];
  const float *l0f_Wt = at(map.l0f_Wt);
  for (int o = 0; o < HC0; ++o) {
    for (int i = 0; i < hid; ++i) {
      double s = 0.0;
      for (int k = 0; k < hid; ++k) s += (double)at(map.fe_W1t)[(size_t)i * hid + k] * (double)at(M0.Wt)[(size_t)k * HC0 + o];
      at(map.l0f_Wt)[(size_t)i * HC0 + o] = (float)s;
    }
    double s = 0.0;
    for (int k = 0; k < hid; ++k) s += (double)at(map.fe_b1)[k] * (double)at(M0.Wt)[(size_t)k * HC0 + o];
    at(map.l0f_b)[o] = (float)s;
  }
  fill_relays(d, map, dst);
  pack_split(at(map.hd_W0t), hid, HT, at(map.hd_W0sp), false);
  if (!pack_split(at(map.hd_W0t), hid, HT, at(map.hd_W0sp16), true, &pv->inv16_hd)) pv->f16_ok = false;
  pack_bf16_image_accop(at(map.hd_W0t), hid, HT, at(map.hd_W0bf));
  pack_tilegroup_image(at(map.hd_W0t), hid, HT, at(map.hd_W0fp));
  pack_split(l0f_Wt, hid, HC0, at(map.l0f_Wsp), false);
  if (!pack_split(l0f_Wt, hid, HC0, at(map.l0f_Wsp16), true, &pv->inv16_l0f)) pv->f16_ok = false;
  pack_bf16_image_accop(l0f_Wt, hid, HC0, at(map.l0f_Wbf));
  if (HC0 / hid <= 4)
    pack_alpha_tile(l0f_Wt, at(map.l0f_b), at(M0.att_src), at(M0.att_dst), hid, HC0 / hid, hid, at(map.l0f_Wbf) + (size_t)hid * HC0 / 2);
  // layer 0 "aggregate first": the folded lin_0 weight as four per-head [64 k][64 columns] bf16 images ([head][k-step][tile] KiB,
  // accumulator-operand k order), and layer 0's folded shift with the folded lin_0 bias carried through the BatchNorm scale (the
  // attention coefficients of a node sum to 1: sum_j alpha_ij (W h_j + b) = W sum_j alpha_ij h_j + b)
  if (map.l0af_W.floats) {
    for (int hd = 0; hd < 4; ++hd) {
      std::vector<float> wh((size_t)hid * 64);
      for (int k = 0; k < hid; ++k)
        for (int c = 0; c < 64; ++c) wh[(size_t)k * 64 + c] = l0f_Wt[(size_t)k * HC0 + hd * 64 + c];
      pack_bf16_image_accop(wh.data(), hid, 64, at(map.l0af_W) + (size_t)hd * 2048);
    }
    for (int o = 0; o < HC0; ++o)
      at(map.l0af_shift)[o] = (float)((double)at(M0.shift)[o] + (double)at(M0.scale)[o] * (double)at(map.l0f_b)[o]);
  }
}

// The tables of bgnn_model_refresh (optimizer.hip), read off the map.  A TRAIN|COPY image: the fill runs over a blob whose
// element i holds i + 1 (exact in float32 below 2^24), so that every packed value names its source and a 0 is padding that stays
// 0.  A TRAIN|RELAY image: the same over an index-valued l0f_Wt.  The derived TRAIN images have their jobs: V one dot product per
// element, l0f_Wt / l0f_b the fold.  Any other TRAIN image is an error: it would go stale with the first optimizer step.
struct RefreshPlan {
  std::vector<int32_t> copy;     // [n][2]: blob[dst] = weights[src]
  std::vector<int32_t> relay;    // [n][2]: blob[dst] = blob[src] (after the fold)
  std::vector<int32_t> vjob;     // [n][4]: blob[dst] = sum_c weights[ae + c] * weights[we + c * edge_dim]  (dst, ae, we, 0)
  // the fold: blob[l0f_Wt + i HC0 + o] = sum_k fe_W1[k][i] * W0[o][k], blob[l0f_b + o] = sum_k fe_b1[k] * W0[o][k]
  int32_t fold_cols = 0;                  // HC0 (0: no fold, not a GAT model)
  int32_t fe_W1 = 0, fe_b1 = 0, W0 = 0;   // offsets in the weight blob
  int32_t l0f_Wt = 0, l0f_b = 0;          // offsets in the packed blob
  std::string error;                      // not empty: the plan is void
};

inline RefreshPlan refresh_plan(const bgnn_model_desc &d, const WeightLayout &wl, const ImageMap &map) {
  RefreshPlan P;
  const size_t hid = d.hidden, ED = d.edge_dim;
  std::vector<float> probe(wl.total), img(map.total, 0.0f);
  for (size_t i = 0; i < wl.total; ++i) probe[i] = (float)(i + 1);
  PackValues pv;
  fill_images(d, wl, map, probe.data(), img.data(), &pv);
  // sources of an index-valued image: (destination, base + value - 1) per element that is no padding
  auto pairs = [&](const char *name, const Image &im, size_t base, size_t limit, std::vector<int32_t> &out) {
    for (size_t i = im.off; i < im.off + im.floats; ++i) {
      const float v = img[i];
      if (v == 0.0f) continue;
      if (!(v >= 1.0f && v <= (float)limit && v == std::floor(v))) { P.error = std::string(name) + " is flagged a plain copy and is none"; return; }
      out.push_back((int32_t)i); out.push_back((int32_t)(base + (size_t)v - 1));
    }
  };
  map.for_each([&](const char *name, int l, const Image &im) {
    if (!(im.flags & IMG_TRAIN) || (im.flags & IMG_RELAY)) return;
    if (im.flags & IMG_COPY) pairs(name, im, 0, wl.total, P.copy);
    else if (l >= 0 && &im == &map.layers[l].V)
      for (size_t h = 0; h < im.floats / ED; ++h)
        for (size_t f = 0; f < ED; ++f) {
          P.vjob.push_back((int32_t)(im.off + h * ED + f));
          P.vjob.push_back((int32_t)(wl.layers[l].ae + h * hid));
          P.vjob.push_back((int32_t)(wl.layers[l].We + h * hid * ED + f));
          P.vjob.push_back(0);
        }
    else if (&im == &map.l0f_Wt || &im == &map.l0f_b) {
      P.fold_cols = (int32_t)map.l0f_b.floats; P.fe_W1 = (int32_t)wl.fe_W1; P.fe_b1 = (int32_t)wl.fe_b1; P.W0 = (int32_t)wl.layers[0].W;
      P.l0f_Wt = (int32_t)map.l0f_Wt.off; P.l0f_b = (int32_t)map.l0f_b.off;
    } else P.error = std::string(name) + " is read by the training path and bgnn_model_refresh has no rule for it";
  });
  for (size_t i = 0; i < map.l0f_Wt.floats; ++i) img[map.l0f_Wt.off + i] = (float)(i + 1);
  fill_relays(d, map, img.data());
  map.for_each([&](const char *name, int, const Image &im) {
    if ((im.flags & IMG_TRAIN) && (im.flags & IMG_RELAY)) pairs(name, im, map.l0f_Wt.off, map.l0f_Wt.floats, P.relay);
  });
  return P;
}

}  // namespace bgnn
