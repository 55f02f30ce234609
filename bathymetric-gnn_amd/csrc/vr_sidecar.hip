// VR BAG sidecar raster on the device (include/bgnn_sidecar.h): the rasterisation of SidecarBuilder.add_refinement_results
// (reference data/vr_bag.py:695-778) for the result planes bgnn_infer_tiles left in HBM.
//
// "The later grid wins" must hold for runs of grids added in any order from two contexts' streams at once, so it cannot rest on
// launch order: per value plane a uint64 image takes a 64-bit integer atomic max of ((grid index + 1) << 32) | float bits.  The
// highest grid index wins whatever the arrival order and the low word carries the value untouched; 0 = never written.  The valid
// mask is sticky and every writer stores the same 1.0f: plain stores.  bgnn_sidecar_finish turns the images into float planes.
//
// Work is spread over FOOTPRINT pixels (a cell at scale s is s x s pixels), clipped to the raster on the host when the table is
// made: consecutive lanes take consecutive pixels of one raster row, so a wave's atomics fall into contiguous 8-byte slots.
// Bytes per footprint pixel: 24 B of atomics + (valid cells) 4 B mask store; reads 13 B per cell, shared by s*s pixels.
// finish: 24 B in, 12 B out per raster pixel.
#include "bgnn_internal.h"
#include "../../include/bgnn_sidecar.h"

namespace bgnn {

struct SidecarEntry {      // one per grid, plus a closing entry that holds the totals; 48 B
  int64_t cell_off;        // cells of the grids before this one
  int64_t pix_off;         // clipped footprint pixels of the grids before this one
  int32_t h, w;            // rows, cols of the grid
  int32_t row0, col0;      // raster position of the grid's top-left pixel (may lie outside)
  int32_t scale;
  int32_t r_lo, c_lo, cw;  // clipped footprint: first raster row / col inside, columns inside (0: nothing inside)
};
static_assert(sizeof(SidecarEntry) == 48, "table layout");

struct SidecarAddArgs {
  const SidecarEntry *tab;
  int32_t first, n_grids, width;
  int64_t n_pixels, n_cells, plane;   // plane = height * width
  unsigned long long *img;
  float *valid;
  const float *cls, *conf, *corr;
  const uint8_t *mask, *keep;
};

// largest g in [lo, hi] with tab[g].pix_off <= q (grids with an empty footprint share their successor's offset and are passed over)
__device__ __forceinline__ int sidecar_find(const SidecarEntry *tab, int lo, int hi, int64_t q) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].pix_off <= q) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void sidecar_add_kernel(SidecarAddArgs a) {
  __shared__ int s_lo, s_hi;
  const int64_t base = a.tab[a.first].pix_off;
  const int64_t p0 = (int64_t)blockIdx.x * 256;
  if (threadIdx.x == 0) {      // the block's 256 pixels lie in a short run of grids: search the table once, the lanes inside that run
    const int64_t last = (p0 + 255 < a.n_pixels ? p0 + 255 : a.n_pixels - 1);
    s_lo = sidecar_find(a.tab, a.first, a.first + a.n_grids - 1, base + p0);
    s_hi = sidecar_find(a.tab, s_lo, a.first + a.n_grids - 1, base + last);
  }
  __syncthreads();
  const int64_t p = p0 + threadIdx.x;
  if (p >= a.n_pixels) return;
  const int64_t q = base + p;
  const int g = sidecar_find(a.tab, s_lo, s_hi, q);
  if (a.keep && !a.keep[g - a.first]) return;
  const SidecarEntry e = a.tab[g];
  const int64_t local = q - e.pix_off;
  if (e.cw <= 0) return;                                    // (cannot happen: an empty footprint owns no pixel index)
  const int32_t rr = (int32_t)(local / e.cw), cc = (int32_t)(local - (int64_t)rr * e.cw);
  const int32_t R = e.r_lo + rr, Cc = e.c_lo + cc;          // inside the raster by construction of the table
  const int32_t r = e.h - 1 - (R - e.row0) / e.scale;       // refinement row 0 is the south row
  const int32_t c = (Cc - e.col0) / e.scale;
  const int64_t cell = e.cell_off - a.tab[a.first].cell_off + (int64_t)r * e.w + c;
  if (r < 0 || r >= e.h || c < 0 || c >= e.w || cell < 0 || cell >= a.n_cells) return;
  const int64_t pix = (int64_t)R * a.width + Cc;
  if (pix < 0 || pix >= a.plane) return;
  const unsigned long long tag = (unsigned long long)(uint32_t)(g + 1) << 32;
  atomicMax(a.img + pix, tag | __float_as_uint(a.cls[cell]));
  atomicMax(a.img + a.plane + pix, tag | __float_as_uint(a.conf[cell]));
  atomicMax(a.img + 2 * a.plane + pix, tag | __float_as_uint(a.corr[cell]));
  if (a.mask[cell]) a.valid[pix] = 1.0f;
}

struct SidecarFinishArgs {
  const unsigned long long *img;
  float *planes;
  int64_t n;     // 3 * height * width
};

__global__ __launch_bounds__(256) void sidecar_finish_kernel(SidecarFinishArgs a) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    const unsigned long long v = a.img[i];
    a.planes[i] = __uint_as_float(v ? (uint32_t)v : 0x7fc00000u);      // numpy's float32 NaN where nothing was painted
  }
}

static bool sidecar_raster_ok(int32_t height, int32_t width) {
  return height > 0 && width > 0 && (int64_t)height * width <= (int64_t)BGNN_SIDECAR_MAX_PIXELS;
}

}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_sidecar_table_bytes(int32_t n_grids) {
  return n_grids < 0 ? 0 : ((size_t)n_grids + 1) * sizeof(SidecarEntry);
}

extern "C" int bgnn_sidecar_table(bgnn_ctx *ctx, int32_t height, int32_t width, int32_t n_grids, const int32_t *hw,
                                  const int64_t *placement, void *table, size_t table_bytes, int64_t *pixel_offsets) {
  BGNN_REQUIRE(ctx && table, "bgnn_sidecar_table: NULL argument");
  BGNN_REQUIRE(sidecar_raster_ok(height, width), "bgnn_sidecar_table: raster %d x %d outside 1 .. %lld pixels (BGNN_SIDECAR_MAX_PIXELS)",
               height, width, (long long)BGNN_SIDECAR_MAX_PIXELS);
  BGNN_REQUIRE(n_grids >= 0 && (n_grids == 0 || (hw && placement)), "bgnn_sidecar_table: NULL grid table");
  BGNN_REQUIRE(table_bytes == bgnn_sidecar_table_bytes(n_grids), "bgnn_sidecar_table: table_bytes %zu, %zu needed for %d grids",
               table_bytes, bgnn_sidecar_table_bytes(n_grids), n_grids);
  std::vector<SidecarEntry> tab((size_t)n_grids + 1);
  int64_t cells = 0, pixels = 0;
  for (int32_t g = 0; g < n_grids; ++g) {
    const int64_t h = hw[2 * g], w = hw[2 * g + 1];
    const int64_t row0 = placement[3 * g], col0 = placement[3 * g + 1], s = placement[3 * g + 2];
    BGNN_REQUIRE(h >= 1 && w >= 1, "bgnn_sidecar_table: grid %d has %lld x %lld cells", g, (long long)h, (long long)w);
    BGNN_REQUIRE(s >= 1, "bgnn_sidecar_table: grid %d has scale %lld < 1", g, (long long)s);
    BGNN_REQUIRE(s < (1ll << 31) && h * s < (1ll << 31) && w * s < (1ll << 31),
                 "bgnn_sidecar_table: grid %d: footprint %lld x %lld cells at scale %lld exceeds 2^31 pixels a side", g, (long long)h,
                 (long long)w, (long long)s);
    SidecarEntry &e = tab[g];
    e.cell_off = cells; e.pix_off = pixels;
    e.h = (int32_t)h; e.w = (int32_t)w; e.scale = (int32_t)s;
    e.row0 = e.col0 = e.r_lo = e.c_lo = e.cw = 0;
    // clip [row0, row0 + h s) x [col0, col0 + w s) to the raster (int64: a grid may lie anywhere)
    const int64_t r_lo = row0 > 0 ? row0 : 0, r_hi = row0 + h * s < height ? row0 + h * s : height;
    const int64_t c_lo = col0 > 0 ? col0 : 0, c_hi = col0 + w * s < width ? col0 + w * s : width;
    if (r_hi > r_lo && c_hi > c_lo) {       // (then row0 / col0 lie in (-2^31, raster size): they fit int32)
      e.row0 = (int32_t)row0; e.col0 = (int32_t)col0;
      e.r_lo = (int32_t)r_lo; e.c_lo = (int32_t)c_lo; e.cw = (int32_t)(c_hi - c_lo);
      pixels += (r_hi - r_lo) * (c_hi - c_lo);
    }
    cells += h * w;
  }
  SidecarEntry &end = tab[n_grids];
  end = SidecarEntry{};
  end.cell_off = cells; end.pix_off = pixels;
  if (pixel_offsets)
    for (int32_t g = 0; g <= n_grids; ++g) pixel_offsets[g] = tab[g].pix_off;
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  BGNN_HIP_CHECK(hipMemcpyAsync(table, tab.data(), table_bytes, hipMemcpyHostToDevice, ctx->stream));
  BGNN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return BGNN_OK;
}

extern "C" int bgnn_sidecar_add(bgnn_ctx *ctx, int32_t height, int32_t width, uint64_t *images, float *valid, int64_t image_pixels,
                                const void *table, int32_t table_grids, int32_t first_grid, int32_t n_grids, int64_t n_pixels,
                                const float *classification, const float *confidence, const float *correction, const uint8_t *mask,
                                int64_t n_cells, const uint8_t *keep) {
  BGNN_REQUIRE(ctx && images && valid && table, "bgnn_sidecar_add: NULL argument");
  BGNN_REQUIRE(sidecar_raster_ok(height, width), "bgnn_sidecar_add: raster %d x %d outside 1 .. %lld pixels (BGNN_SIDECAR_MAX_PIXELS)",
               height, width, (long long)BGNN_SIDECAR_MAX_PIXELS);
  BGNN_REQUIRE(image_pixels == (int64_t)height * width, "bgnn_sidecar_add: images hold %lld pixels, the raster %d x %d has %lld",
               (long long)image_pixels, height, width, (long long)height * width);
  BGNN_REQUIRE(table_grids >= 0 && first_grid >= 0 && n_grids >= 0 && (int64_t)first_grid + n_grids <= table_grids,
               "bgnn_sidecar_add: grids [%d, %d + %d) outside the table of %d", first_grid, first_grid, n_grids, table_grids);
  BGNN_REQUIRE(n_pixels >= 0 && n_cells >= 0, "bgnn_sidecar_add: bad sizes");
  BGNN_REQUIRE(n_pixels < (1ll << 39), "bgnn_sidecar_add: %lld footprint pixels in one call, at most 2^39", (long long)n_pixels);
  if (n_grids == 0 || n_pixels == 0 || n_cells == 0) return BGNN_OK;
  BGNN_REQUIRE(classification && confidence && correction && mask, "bgnn_sidecar_add: NULL result plane");
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  ProfScope ps(ctx, BGNN_K_SCATTER);
  SidecarAddArgs a{reinterpret_cast<const SidecarEntry *>(table), first_grid, n_grids, width, n_pixels, n_cells,
                   (int64_t)height * width, reinterpret_cast<unsigned long long *>(images), valid,
                   classification, confidence, correction, mask, keep};
  hipLaunchKernelGGL(sidecar_add_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, ctx->stream, a);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

extern "C" int bgnn_sidecar_finish(bgnn_ctx *ctx, int32_t height, int32_t width, const uint64_t *images, int64_t image_pixels,
                                   float *planes) {
  BGNN_REQUIRE(ctx && images && planes, "bgnn_sidecar_finish: NULL argument");
  BGNN_REQUIRE(sidecar_raster_ok(height, width), "bgnn_sidecar_finish: raster %d x %d outside 1 .. %lld pixels (BGNN_SIDECAR_MAX_PIXELS)",
               height, width, (long long)BGNN_SIDECAR_MAX_PIXELS);
  BGNN_REQUIRE(image_pixels == (int64_t)height * width, "bgnn_sidecar_finish: images hold %lld pixels, the raster %d x %d has %lld",
               (long long)image_pixels, height, width, (long long)height * width);
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  ProfScope ps(ctx, BGNN_K_SCATTER);
  const int64_t n = 3 * (int64_t)height * width;
  const int64_t b = (n + 255) / 256;
  SidecarFinishArgs a{reinterpret_cast<const unsigned long long *>(images), planes, n};
  hipLaunchKernelGGL(sidecar_finish_kernel, dim3((unsigned)(b > 16384 ? 16384 : b)), dim3(256), 0, ctx->stream, a);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
