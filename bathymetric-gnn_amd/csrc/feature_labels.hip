// Feature labels from charted objects (include/bgnn_features.h): scripts/extract_s57_features.py, create_feature_labels, on a
// survey plane that stays in HBM.  A gather over host-planned bins (feature_plan.h): one launch, a workgroup per bin of 64 x 64
// cells (at most 16 workgroups per CU: on a larger grid a workgroup takes every gridDim.x-th bin), no atomics on the plane.
//
//   fl_paint   reads the bin's cells (depth, or the base labels in overlay mode): 16-byte loads where the row allows.  A thread owns
//              four cells along a row in each of four rows, 16 rows apart, so a wave's loads and stores are whole 256-byte row
//              segments.  The bin's feature list is staged through LDS in chunks of 256 entries (row, col, radius, label); every
//              thread walks a chunk from the top (the list is in descending index: the first hit decides a cell) and a wave leaves
//              the walk once none of its cells is open.  A workgroup stops staging once none of its waves has an open cell.  The
//              three counts are kept per thread over the workgroup's bins, then reduced per wave with shuffles, per workgroup
//              through LDS, and added with one 64-bit integer atomic per count and workgroup.
//
// The disc test is (c - col)^2 + (r - row)^2 <= radius^2 in int64: with a radius up to 2^31 - 1 and a grid side below 2^31 both
// sides stay below 2^63.  No float enters it.
//
// Compiled with -ffp-contract=off like its neighbours (the validity test is two float32 comparisons; nothing here contracts).
#include "bgnn_internal.h"
#include "feature_plan.h"
#include "plane_util.h"

namespace bgnn {
namespace {

constexpr int FL_THREADS = 256;
constexpr int FL_BIN = BGNN_FL_BIN;
constexpr int FL_CHUNK = 256;                         // list entries staged at once (4 KiB of LDS)
constexpr int FL_GRID_PER_CU = 16;                    // workgroups per CU at most: two rounds of the eight that fit
constexpr int FL_ROWS = 4, FL_COLS = 4;               // cells of a thread: 4 along a row, in rows 16 apart
static_assert(FL_BIN == 64 && FL_THREADS == (FL_BIN / FL_COLS) * (FL_BIN / FL_ROWS), "a thread owns 16 cells of a 64 x 64 bin");

struct FlArgs {
  const float *depth;            // depth mode (else nullptr)
  const int32_t *base;           // overlay mode (else nullptr)
  int32_t *out;
  const int64_t *bin_ptr;
  const int32_t *bin_feat;
  const int4 *table;
  unsigned long long *stats;     // valid, feature, painted
  int32_t rows, cols, bins_c, bins;
  float nodata;
};

// VEC: cols is a multiple of 4 and the planes are 16-byte aligned: every thread's four cells are one aligned 16-byte access, all
// inside the grid or all outside.
template <bool VEC>
__global__ __launch_bounds__(FL_THREADS) void fl_paint(FlArgs a) {
  __shared__ int4 feat[FL_CHUNK];
  __shared__ unsigned long long wave_sum[FL_THREADS / 64][3];
  const int t = threadIdx.x;
  const bool overlay = a.base != nullptr;               // (uniform)
  uint32_t n_valid = 0, n_feature = 0, n_painted = 0;   // over every bin of this workgroup: below 2^32 / 256 per thread
  for (int32_t bin = (int32_t)blockIdx.x; bin < a.bins; bin += (int32_t)gridDim.x) {
    const int br = bin / a.bins_c, bc = bin % a.bins_c;
    const int c0 = bc * FL_BIN + (t & 15) * FL_COLS;
    const int r0 = br * FL_BIN + (t >> 4);

    int32_t lab[FL_ROWS][FL_COLS];
    uint32_t in = 0, valid = 0, open = 0, painted = 0;    // one bit per cell: k * 4 + i
#pragma unroll
    for (int k = 0; k < FL_ROWS; ++k) {
      const int r = r0 + 16 * k;
      int32_t raw[FL_COLS] = {0, 0, 0, 0};
      uint32_t inrow = 0;
      if (r < a.rows && c0 < a.cols) {
        const int64_t at = (int64_t)r * a.cols + c0;
        if (VEC) {
          const int4 v = overlay ? *reinterpret_cast<const int4 *>(a.base + at) : *reinterpret_cast<const int4 *>(a.depth + at);
          raw[0] = v.x; raw[1] = v.y; raw[2] = v.z; raw[3] = v.w;
          inrow = 15u;
        } else {
#pragma unroll
          for (int i = 0; i < FL_COLS; ++i)
            if (c0 + i < a.cols) {
              raw[i] = overlay ? a.base[at + i] : __float_as_int(a.depth[at + i]);
              inrow |= 1u << i;
            }
        }
      }
#pragma unroll
      for (int i = 0; i < FL_COLS; ++i) {
        const uint32_t bit = 1u << (k * FL_COLS + i);
        const bool here = (inrow >> i) & 1u;
        bool ok, paintable;
        if (overlay) {
          lab[k][i] = raw[i];
          ok = here && raw[i] >= 0;
          paintable = here && raw[i] == 0;
        } else {
          const float d = __int_as_float(raw[i]);
          ok = here && d != a.nodata && finite_bits(d);
          lab[k][i] = ok ? 0 : -1;
          paintable = ok;
        }
        if (here) in |= bit;
        if (ok) valid |= bit;
        if (paintable) open |= bit;
      }
    }

    const int64_t begin = a.bin_ptr[bin], end = a.bin_ptr[bin + 1];
    for (int64_t base = begin; base < end; base += FL_CHUNK) {
      const int n = (int)(end - base < FL_CHUNK ? end - base : FL_CHUNK);
      __syncthreads();                                            // (the previous chunk's readers are done)
      if (t < n) feat[t] = a.table[a.bin_feat[base + t]];
      if (!__syncthreads_or(open != 0)) break;                    // (uniform: nothing left to decide in this bin)
      if (__ballot(open != 0) == 0) continue;                     // (wave-uniform: this wave is done, the others still read)
      for (int j = 0; j < n; ++j) {
        const int4 f = feat[j];                                   // row, col, radius, label: one address, a broadcast
        if (open != 0 && f.z >= 0) {
          const int64_t r2 = (int64_t)f.z * f.z;
#pragma unroll
          for (int k = 0; k < FL_ROWS; ++k) {
            const int64_t dy = (int64_t)(r0 + 16 * k) - f.x;
            const int64_t room = r2 - dy * dy;                    // dx^2 may be at most this
            if (room < 0) continue;
#pragma unroll
            for (int i = 0; i < FL_COLS; ++i) {
              const uint32_t bit = 1u << (k * FL_COLS + i);
              const int64_t dx = (int64_t)(c0 + i) - f.y;
              if ((open & bit) && dx * dx <= room) {
                lab[k][i] = f.w;
                open &= ~bit;
                painted |= bit;
              }
            }
          }
        }
        if (__ballot(open != 0) == 0) break;                      // every cell this wave owns is decided
      }
    }

#pragma unroll
    for (int k = 0; k < FL_ROWS; ++k) {
      const int r = r0 + 16 * k;
      const uint32_t inrow = (in >> (k * FL_COLS)) & 15u;
      if (inrow == 0) continue;
      const int64_t at = (int64_t)r * a.cols + c0;
      if (VEC) {
        *reinterpret_cast<int4 *>(a.out + at) = make_int4(lab[k][0], lab[k][1], lab[k][2], lab[k][3]);
      } else {
#pragma unroll
        for (int i = 0; i < FL_COLS; ++i)
          if ((inrow >> i) & 1u) a.out[at + i] = lab[k][i];
      }
#pragma unroll
      for (int i = 0; i < FL_COLS; ++i) n_feature += (((inrow >> i) & 1u) && lab[k][i] == 1) ? 1u : 0u;
    }
    n_valid += (uint32_t)__popc(valid);
    n_painted += (uint32_t)__popc(painted);
  }  // bins of this workgroup

  // one sum per wave (shuffles), one per workgroup (LDS), one 64-bit integer add per count and workgroup
  unsigned long long sum[3] = {n_valid, n_feature, n_painted};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) sum[q] += __shfl_xor(sum[q], w);
  }
  __syncthreads();
  if ((t & 63) == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) wave_sum[t >> 6][q] = sum[q];
  }
  __syncthreads();
  if (t < 3) {
    unsigned long long v = 0;
#pragma unroll
    for (int w = 0; w < FL_THREADS / 64; ++w) v += wave_sum[w][t];
    if (v) atomicAdd(a.stats + t, v);
  }
}

inline int plan_error(const FeaturePlanShape &s) {
  set_error("%s", s.message.c_str());
  return s.error;
}

}  // namespace
}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_feature_labels_plan_bytes(const int32_t *table, int64_t n_features, int64_t rows, int64_t cols) {
  const FeaturePlanShape s = feature_plan_shape("bgnn_feature_labels_plan_bytes", table, n_features, rows, cols);
  if (s.error != BGNN_OK) { (void)plan_error(s); return 0; }
  return s.bytes;
}

extern "C" int bgnn_feature_labels_plan(const int32_t *table, int64_t n_features, int64_t rows, int64_t cols, void *plan,
                                        size_t plan_bytes) {
  BGNN_REQUIRE(plan, "bgnn_feature_labels_plan: NULL plan");
  BGNN_REQUIRE(((uintptr_t)plan & 7) == 0, "bgnn_feature_labels_plan: the plan is not 8-byte aligned");
  const FeaturePlanShape s = feature_plan_fill("bgnn_feature_labels_plan", table, n_features, rows, cols, plan, plan_bytes);
  return s.error == BGNN_OK ? BGNN_OK : plan_error(s);
}

extern "C" size_t bgnn_feature_labels_workspace_bytes(int64_t n_features, size_t plan_bytes) {
  if (n_features < 0 || n_features > (int64_t)BGNN_FL_MAX_FEATURES) return 0;
  return align256(plan_bytes) + align256((size_t)n_features * 16);
}

extern "C" int bgnn_feature_labels(bgnn_ctx *ctx, const float *depth, const int32_t *base_labels, int64_t rows, int64_t cols,
                                   double nodata, const int32_t *table, int64_t n_features, const void *plan, size_t plan_bytes,
                                   void *workspace, size_t workspace_bytes, int32_t *labels, void *stats) {
  BGNN_REQUIRE(ctx && plan && workspace && labels && stats, "bgnn_feature_labels: NULL argument");
  BGNN_REQUIRE((depth != nullptr) != (base_labels != nullptr),
               "bgnn_feature_labels: exactly one of depth and base_labels is given (%s)", depth ? "both are" : "neither is");
  FeaturePlanShape s;
  feature_plan_check_shape(s, "bgnn_feature_labels", table, n_features, rows, cols);
  if (s.error != BGNN_OK) return plan_error(s);
  BGNN_REQUIRE(((uintptr_t)plan & 7) == 0, "bgnn_feature_labels: the plan is not 8-byte aligned");
  std::string why;
  BGNN_REQUIRE(feature_plan_consistent(plan, plan_bytes, s.bins, n_features, why), "bgnn_feature_labels: the plan of %zu bytes is %s",
               plan_bytes, why.c_str());
  const size_t need = bgnn_feature_labels_workspace_bytes(n_features, plan_bytes);
  BGNN_REQUIRE(workspace_bytes >= need, "bgnn_feature_labels: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  BGNN_REQUIRE(((uintptr_t)workspace & 15) == 0, "bgnn_feature_labels: the workspace is not 16-byte aligned");
  BGNN_REQUIRE(((uintptr_t)stats & 7) == 0, "bgnn_feature_labels: the statistics block is not 8-byte aligned");
  BGNN_REQUIRE(((uintptr_t)labels & 3) == 0 && ((uintptr_t)depth & 3) == 0 && ((uintptr_t)base_labels & 3) == 0,
               "bgnn_feature_labels: a plane is not 4-byte aligned");
  for (int64_t k = 0; k < n_features; ++k) {                    // (the plan function checked its own copy; this one is what is uploaded)
    const int64_t row = table[4 * k], col = table[4 * k + 1];
    BGNN_REQUIRE(row >= 0 && row < rows && col >= 0 && col < cols, "bgnn_feature_labels: feature %lld has its centre outside the grid",
                 (long long)k);
  }
  BGNN_REQUIRE(s.bins <= 2147483647, "bgnn_feature_labels: %lld bins", (long long)s.bins);   // (rows * cols <= 2^31 - 1: always)

  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  char *w = static_cast<char *>(workspace);
  const size_t used = (size_t)8 * (size_t)(s.bins + 1) + (size_t)4 * (size_t)static_cast<const int64_t *>(plan)[s.bins];
  BGNN_TRY(ctx_upload(ctx, plan, used, w));
  BGNN_TRY(ctx_upload(ctx, table, (size_t)n_features * 16, w + align256(plan_bytes)));
  BGNN_HIP_CHECK(hipMemsetAsync(stats, 0, BGNN_FL_STATS_BYTES, ctx->stream));
  FlArgs a;
  a.depth = depth; a.base = base_labels; a.out = labels;
  a.bin_ptr = reinterpret_cast<const int64_t *>(w);
  a.bin_feat = reinterpret_cast<const int32_t *>(w + (size_t)8 * (size_t)(s.bins + 1));
  a.table = reinterpret_cast<const int4 *>(w + align256(plan_bytes));
  a.stats = static_cast<unsigned long long *>(stats);
  a.rows = (int32_t)rows; a.cols = (int32_t)cols; a.bins_c = (int32_t)s.bins_c; a.bins = (int32_t)s.bins;
  a.nodata = (float)nodata;
  const void *in = depth ? (const void *)depth : (const void *)base_labels;
  const bool vec = (cols & 3) == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)labels & 15) == 0;
  // a workgroup walks the bins blockIdx.x, blockIdx.x + gridDim.x, ...: neighbouring bins (which tend to share long lists) go to
  // different workgroups, and the three counters see 3 x FL_GRID_PER_CU x CUs adds instead of 3 per bin -- every workgroup adding
  // to the same three words serialises in L2, and at 20000 x 20000 (97969 bins) that, not the 8 bytes per cell, set the time
  const int64_t max_grid = (int64_t)FL_GRID_PER_CU * (ctx->num_cus > 0 ? ctx->num_cus : 256);
  const dim3 grid((uint32_t)(s.bins < max_grid ? s.bins : max_grid)), block(FL_THREADS);
  if (vec) hipLaunchKernelGGL(fl_paint<true>, grid, block, 0, ctx->stream, a);
  else hipLaunchKernelGGL(fl_paint<false>, grid, block, 0, ctx->stream, a);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
