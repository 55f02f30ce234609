// Stand-alone check of csrc/model_images.h at in_channels above 8 (no HIP, no GPU): for a few shapes, the first extractor image
// fe_W0t -- its row count, the weight transposed into rows 0 .. in - 1, zeros in the rows behind -- and the refresh plan's copy
// table applied to it, as one JSON document on stdout.  tests/test_host_density.py compiles and runs it.
#include <stdio.h>

#include "../bathymetric-gnn_amd/csrc/model_images.h"

using namespace bgnn;

int main() {
  const int types[] = {BGNN_GNN_GAT, BGNN_GNN_SAGE};
  const int ins[] = {7, 8, 9, 16};
  printf("{");
  bool first = true;
  for (int type : types)
    for (int in : ins) {
      bgnn_model_desc d{};
      d.in_channels = in; d.hidden = 64; d.num_layers = 3; d.heads = type == BGNN_GNN_GAT ? 4 : 1; d.num_classes = 3; d.edge_dim = 3;
      d.predict_correction = 1; d.bn_eps = 1e-5f; d.gnn_type = type;
      const WeightLayout wl = weight_layout(d);
      const ImageMap map = image_map(d);
      auto weights = [&](float base) {
        std::vector<float> w(wl.total);
        for (size_t i = 0; i < wl.total; ++i) w[i] = base + (float)(i % 977) * 0.001f;      // (never zero)
        for (const auto &L : wl.layers) for (size_t i = L.bn_var; i < L.bn_var + (L.bn_var - L.bn_mean); ++i) w[i] = 0.75f;
        return w;
      };
      const std::vector<float> wA = weights(0.25f), wB = weights(0.5f);
      std::vector<float> pkA(map.total, 0.0f), pkB(map.total, 0.0f);
      PackValues pv;
      fill_images(d, wl, map, wA.data(), pkA.data(), &pv);
      fill_images(d, wl, map, wB.data(), pkB.data(), &pv);
      const int hid = d.hidden, rows = (int)(map.fe_W0t.floats / hid);
      bool transposed = true, zero_behind = true;
      for (int i = 0; i < rows; ++i)
        for (int o = 0; o < hid; ++o) {
          const float v = pkA[map.fe_W0t.off + (size_t)i * hid + o];
          if (i < in) transposed = transposed && v == wA[wl.fe_W0 + (size_t)o * in + i];
          else zero_behind = zero_behind && v == 0.0f && pkB[map.fe_W0t.off + (size_t)i * hid + o] == 0.0f;
        }
      const RefreshPlan P = refresh_plan(d, wl, map);
      std::vector<float> pk = pkA;
      for (size_t i = 0; i < P.copy.size(); i += 2) pk[P.copy[i]] = wB[P.copy[i + 1]];
      const bool refreshed = !memcmp(&pk[map.fe_W0t.off], &pkB[map.fe_W0t.off], map.fe_W0t.floats * sizeof(float));
      printf("%s\"%s_in%d\": {\"rows\": %d, \"fe_W0t_off\": %zu, \"weights\": %zu, \"transposed\": %s, \"zero_behind\": %s, "
             "\"plan_error\": \"%s\", \"refreshed\": %s}", first ? "" : ", ", type == BGNN_GNN_GAT ? "gat" : "sage", in, rows, map.fe_W0t.off,
             wl.total, transposed ? "true" : "false", zero_behind ? "true" : "false", P.error.c_str(), refreshed ? "true" : "false");
      first = false;
    }
  printf("}\n");
  return 0;
}
