// Stand-alone check of csrc/model_images.h (no HIP, no GPU): for a list of model shapes, the layout, a hash of the filled blob, the
// value-dependent results and the refresh tables as one JSON document on stdout; and the refresh plan as a property (apply it on
// the CPU to a blob filled from weight set A, with weight set B: the images the training path reads must equal a fill from B byte
// for byte, every other image must still be A's).  tests/test_host_pack.py compiles it, runs it and compares the document with
// tests/golden/pack_images.json.  `--time`: the median fill time of two shapes instead.
#include <stdio.h>

#include <chrono>

#include "../bathymetric-gnn_amd/csrc/model_images.h"

using namespace bgnn;

// ---- cases and the weight generator -----------------------------------------------------------------------------------------
struct Case {
  const char *name;
  int type, hidden, layers, heads, classes, edge_dim, correction, in;
  bool big_weight;   // one lin weight of layer 1 set to 1e5: beyond float16
  bool property;     // also the refresh-plan property
};
static const Case kCases[] = {
    {"gat_default", BGNN_GNN_GAT, 64, 3, 4, 3, 3, 1, 8, false, true},
    {"gat_two_heads_in7", BGNN_GNN_GAT, 64, 3, 4, 3, 3, 0, 7, false, false},
    {"gat_128x4", BGNN_GNN_GAT, 128, 3, 4, 3, 3, 1, 8, false, true},
    {"gat_64x8", BGNN_GNN_GAT, 64, 3, 8, 3, 3, 1, 8, false, false},
    {"gat_one_layer", BGNN_GNN_GAT, 64, 1, 4, 3, 3, 1, 8, false, true},
    {"gat_32x2_edge1", BGNN_GNN_GAT, 32, 2, 2, 3, 1, 1, 8, false, false},
    {"gat_32x1_16cls", BGNN_GNN_GAT, 32, 4, 1, 16, 4, 1, 8, false, false},
    {"gcn_64", BGNN_GNN_GCN, 64, 3, 1, 3, 3, 1, 8, false, false},
    {"sage_64", BGNN_GNN_SAGE, 64, 3, 1, 3, 3, 1, 8, false, true},
    {"gin_64", BGNN_GNN_GIN, 64, 3, 1, 3, 3, 1, 8, false, true},
    {"gcn_32", BGNN_GNN_GCN, 32, 3, 1, 3, 3, 1, 8, false, false},
    {"sage_128", BGNN_GNN_SAGE, 128, 3, 1, 3, 3, 1, 8, false, false},
    {"gin_32", BGNN_GNN_GIN, 32, 3, 1, 3, 3, 1, 8, false, false},
    {"gat_default_beyond_f16", BGNN_GNN_GAT, 64, 3, 4, 3, 3, 1, 8, true, false},
    {"gat_48x3_padded", BGNN_GNN_GAT, 48, 3, 3, 3, 3, 1, 8, false, false},
};

static bgnn_model_desc desc_of(const Case &c) {
  bgnn_model_desc d{};
  d.in_channels = c.in; d.hidden = c.hidden; d.num_layers = c.layers; d.heads = c.heads; d.num_classes = c.classes;
  d.edge_dim = c.edge_dim; d.predict_correction = c.correction; d.bn_eps = 1e-5f; d.gnn_type = c.type;
  return d;
}

// xorshift64; 24 bits per draw.  Weights in [-0.15, 0.15), BatchNorm variances in [0.5, 1): integer arithmetic and one exact or
// singly rounded float operation each, so every compiler produces the same blob
static std::vector<float> make_weights(const bgnn::WeightLayout &wl, uint64_t seed, bool big_weight) {
  uint64_t x = 0x9E3779B97F4A7C15ull ^ (seed * 0xD1B54A32D192ED03ull);
  auto draw = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (uint32_t)(x >> 40); };
  std::vector<float> w(wl.total);
  for (size_t i = 0; i < wl.total; ++i) w[i] = ((float)draw() - 8388608.0f) * (0.15f / 8388608.0f);
  for (const auto &L : wl.layers) {
    const size_t n = L.bn_var - L.bn_mean;             // (the four BatchNorm vectors of a layer have one length)
    for (size_t i = 0; i < n; ++i) w[L.bn_var + i] = (float)((draw() >> 1) + 8388608u) * (1.0f / 16777216.0f);
  }
  if (big_weight) w[wl.layers[1].W + 5] = 1e5f;
  return w;
}

static uint64_t fnv1a(const void *p, size_t bytes, uint64_t h = 0xcbf29ce484222325ull) {
  const unsigned char *b = (const unsigned char *)p;
  for (size_t i = 0; i < bytes; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
  return h;
}

// hash of a table of `width`-int entries, entries sorted
static uint64_t table_hash(const int32_t *t, size_t n, int width) {
  std::vector<std::vector<int32_t>> e(n);
  for (size_t i = 0; i < n; ++i) e[i].assign(t + i * width, t + (i + 1) * width);
  std::sort(e.begin(), e.end());
  uint64_t h = 0xcbf29ce484222325ull;
  for (const auto &v : e) h = fnv1a(v.data(), v.size() * sizeof(int32_t), h);
  return h;
}

static std::vector<float> fill(const bgnn_model_desc &d, const WeightLayout &wl, const ImageMap &map, const std::vector<float> &w, PackValues *pv) {
  std::vector<float> pk(map.total, 0.0f);
  fill_images(d, wl, map, w.data(), pk.data(), pv);
  return pk;
}

// "ok", or the first image that breaks the property
static std::string plan_property(const bgnn_model_desc &d, const WeightLayout &wl, const ImageMap &map, const RefreshPlan &P,
                                 const std::vector<float> &pkA) {
  const std::vector<float> wB = make_weights(wl, 0x5eed, false);
  PackValues pv;
  const std::vector<float> pkB = fill(d, wl, map, wB, &pv);
  std::vector<float> pk = pkA;
  const float *w = wB.data();
  const int hid = d.hidden, ED = d.edge_dim, HC0 = P.fold_cols;
  for (size_t i = 0; i < P.copy.size(); i += 2) pk[P.copy[i]] = w[P.copy[i + 1]];
  for (int o = 0; o < HC0; ++o) {          // the fold and the V jobs as optimizer.hip refresh_fold_kernel states them, k ascending
    for (int i = 0; i < hid; ++i) {
      double s = 0.0;
      for (int k = 0; k < hid; ++k) s += (double)w[P.fe_W1 + k * hid + i] * (double)w[P.W0 + o * hid + k];
      pk[P.l0f_Wt + (size_t)i * HC0 + o] = (float)s;
    }
    double s = 0.0;
    for (int k = 0; k < hid; ++k) s += (double)w[P.fe_b1 + k] * (double)w[P.W0 + o * hid + k];
    pk[P.l0f_b + o] = (float)s;
  }
  for (size_t j = 0; j < P.vjob.size(); j += 4) {
    double s = 0.0;
    for (int c = 0; c < hid; ++c) s += (double)w[P.vjob[j + 1] + c] * (double)w[P.vjob[j + 2] + c * ED];
    pk[P.vjob[j]] = (float)s;
  }
  for (size_t i = 0; i < P.relay.size(); i += 2) pk[P.relay[i]] = pk[P.relay[i + 1]];
  std::string bad;
  map.for_each([&](const char *name, int l, const Image &im) {
    const std::vector<float> &want = im.flags & IMG_TRAIN ? pkB : pkA;
    if (bad.empty() && memcmp(&pk[im.off], &want[im.off], im.floats * sizeof(float)))
      bad = std::string(name) + (l >= 0 ? " of layer " + std::to_string(l) : "") + (im.flags & IMG_TRAIN ? " is not B's" : " is no longer A's");
  });
  if (bad.empty() && pkB == pkA) bad = "weight sets A and B pack alike";
  return bad.empty() ? "ok" : bad;
}

// every image flagged COPY holds nothing but weights and padding: an index-valued blob comes out as integers in range
static bool copy_flags_hold(const bgnn_model_desc &d, const WeightLayout &wl, const ImageMap &map) {
  std::vector<float> probe(wl.total);
  for (size_t i = 0; i < wl.total; ++i) probe[i] = (float)(i + 1);
  PackValues pv;
  const std::vector<float> pk = fill(d, wl, map, probe, &pv);
  bool ok = true;
  map.for_each([&](const char *, int, const Image &im) {
    if (!(im.flags & IMG_COPY)) return;
    for (size_t i = im.off; i < im.off + im.floats; ++i)
      if (pk[i] != 0.0f && !(pk[i] >= 1.0f && pk[i] <= (float)wl.total && pk[i] == std::floor(pk[i]))) ok = false;
  });
  return ok;
}

static int time_fill() {
  for (int ci : {0, 2}) {
    const bgnn_model_desc d = desc_of(kCases[ci]);
    const WeightLayout wl = weight_layout(d);
    const std::vector<float> w = make_weights(wl, 1, false);
    std::vector<double> ms;
    for (int r = 0; r < 20; ++r) {
      const auto t0 = std::chrono::steady_clock::now();
      const ImageMap map = image_map(d);
      PackValues pv;
      const std::vector<float> pk = fill(d, wl, map, w, &pv);
      ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    printf("%s: median %.3f ms (min %.3f max %.3f)\n", kCases[ci].name, 0.5 * (ms[9] + ms[10]), ms[0], ms[19]);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "--time")) return time_fill();
  const int n = sizeof(kCases) / sizeof(kCases[0]);
  printf("{\n");
  for (int ci = 0; ci < n; ++ci) {
    const Case &c = kCases[ci];
    bgnn_model_desc d = desc_of(c);
    WeightLayout wl = weight_layout(d);
    std::vector<float> w = make_weights(wl, 2 * ci + 1, c.big_weight);
    printf("\"%s\": {\"weights\": %zu, ", c.name, wl.total);
    if (pad_hidden(d.hidden) != d.hidden || pad_heads(d.heads) != d.heads) {
      bgnn_model_desc dp;
      WeightLayout lp;
      std::vector<float> wp;
      pad_model_weights(&d, wl, w.data(), &dp, &lp, wp);
      d = dp; wl = lp; w = wp;
      printf("\"padded_weights\": %zu, \"padded_hash\": \"%016llx\", ", wl.total, (unsigned long long)fnv1a(w.data(), w.size() * 4));
    }
    const ImageMap map = image_map(d);
    PackValues pv;
    const std::vector<float> pk = fill(d, wl, map, w, &pv);
    printf("\"total\": %zu, \"HT\": %d, \"htab_ok\": %s, \"f16_ok\": %s, \"inv16\": [", map.total, map.HT, map.htab_ok ? "true" : "false",
           pv.f16_ok ? "true" : "false");
    for (size_t l = 0; l < pv.inv16.size(); ++l) printf("%s%.9g", l ? ", " : "", (double)pv.inv16[l]);
    printf("], \"inv16_hd\": %.9g, \"inv16_l0f\": %.9g, \"hash\": \"%016llx\", \"h_V\": \"%016llx\",\n  \"images\": {", (double)pv.inv16_hd,
           (double)pv.inv16_l0f, (unsigned long long)fnv1a(pk.data(), pk.size() * 4), (unsigned long long)fnv1a(pv.h_V.data(), pv.h_V.size() * 4));
    bool first = true;
    map.for_each([&](const char *name, int l, const Image &im) {
      printf("%s\"%s%s\": [%zu, %zu, \"%s%s%s\"]", first ? "" : ", ", l >= 0 ? ("L" + std::to_string(l) + ".").c_str() : "", name, im.off, im.floats,
             im.flags & IMG_TRAIN ? "T" : "", im.flags & IMG_COPY ? "C" : "", im.flags & IMG_RELAY ? "R" : "");
      first = false;
    });
    const RefreshPlan P = refresh_plan(d, wl, map);
    printf("},\n  \"copy_flags_hold\": %s, \"plan\": {\"error\": \"%s\", \"n_copy\": %zu, \"n_relay\": %zu, \"n_vjob\": %zu, \"copy\": \"%016llx\", "
           "\"relay\": \"%016llx\", \"vjob\": \"%016llx\", \"fold\": [%d, %d, %d, %d, %d, %d]}",
           copy_flags_hold(d, wl, map) ? "true" : "false", P.error.c_str(), P.copy.size() / 2, P.relay.size() / 2, P.vjob.size() / 4,
           (unsigned long long)table_hash(P.copy.data(), P.copy.size() / 2, 2), (unsigned long long)table_hash(P.relay.data(), P.relay.size() / 2, 2),
           (unsigned long long)table_hash(P.vjob.data(), P.vjob.size() / 4, 4), P.fold_cols, P.fe_W1, P.fe_b1, P.W0, P.l0f_Wt, P.l0f_b);
    if (c.property) printf(",\n  \"plan_property\": \"%s\"", plan_property(d, wl, map, P, pk).c_str());
    printf("}%s\n", ci + 1 < n ? "," : "");
  }
  printf("}\n");
  return 0;
}
