// The locale guide (include/bgnn_locale.h): per cell the median of the witness values in a window of neighbouring cells, as a
// float32 guide plane for bgnn_hypotheses_build, and the number of witnesses.  The window logic is that of locale_window.h.
//
//   locale_guide_tiles  a 256-thread workgroup per tile of LC_TILE_H x LC_TILE_W cells, a fixed grid striding over the tiles.  The
//                       tile and a halo of `radius` cells go into LDS as int64 witness values (LOCALE_NO_WITNESS for a cell that
//                       is none or lies outside the grid); then one thread per cell finds its two order statistics by counting
//                       over its window of the image.  A tile row is one half of a wave: its 32 threads read 32 consecutive
//                       int64 of one image row at every step, all 64 banks once, whatever the row stride.
//
// No scratch, no atomics, no workspace, no float arithmetic before the conversion.  Compiled with -ffp-contract=off.
#include "bgnn_internal.h"
#include "plane_util.h"
#include "sounding_args.h"
#include "locale_window.h"
#include "../../include/bgnn_locale.h"

namespace bgnn {

constexpr int LC_THREADS = BLOCK_THREADS;
constexpr int LC_TILE_W = 32;
constexpr int LC_TILE_H = LC_THREADS / LC_TILE_W;
constexpr int LC_MAX_R = BGNN_LOCALE_MAX_RADIUS;
constexpr int LC_IMAGE = (LC_TILE_H + 2 * LC_MAX_R) * (LC_TILE_W + 2 * LC_MAX_R);      // 24 x 48 entries, 9216 bytes
constexpr int64_t LC_MAX_CELLS = 2147483647;

__global__ __launch_bounds__(LC_THREADS) void locale_guide_tiles(const int32_t *__restrict__ n_hyp, const int32_t *__restrict__ chosen,
                                                                 const int64_t *__restrict__ center2, int64_t height, int64_t width,
                                                                 int radius, int32_t min_support, int64_t tiles_x, int64_t n_tiles,
                                                                 uint32_t *__restrict__ guide, int32_t *__restrict__ support) {
  __shared__ int64_t image[LC_IMAGE];
  const int iw = LC_TILE_W + 2 * radius, ih = LC_TILE_H + 2 * radius;
  const int lr = threadIdx.x / LC_TILE_W, lc = threadIdx.x % LC_TILE_W;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row0 = tile / tiles_x * LC_TILE_H - radius, col0 = tile % tiles_x * LC_TILE_W - radius;      // of the image
    for (int i = threadIdx.x; i < ih * iw; i += LC_THREADS) {
      const int64_t r = row0 + i / iw, c = col0 + i % iw;
      int64_t v = LOCALE_NO_WITNESS;
      if (r >= 0 && r < height && c >= 0 && c < width) {
        const int64_t cell = r * width + c;
        v = locale_witness_value(n_hyp[cell], chosen[cell], center2[cell]);
      }
      image[i] = v;
    }
    __syncthreads();
    const int64_t r = row0 + radius + lr, c = col0 + radius + lc;
    if (r < height && c < width) {
      // the window in image coordinates, clipped to the grid: the image's row j is the grid's row0 + j
      const int r0 = (int)(r - radius < 0 ? -row0 : lr), r1 = (int)(r + radius > height - 1 ? height - 1 - row0 : lr + 2 * radius);
      const int c0 = (int)(c - radius < 0 ? -col0 : lc), c1 = (int)(c + radius > width - 1 ? width - 1 - col0 : lc + 2 * radius);
      int64_t med2 = 0;
      const int32_t k = locale_window(image, iw, r0, r1, c0, c1, (lr + radius) * iw + lc + radius, min_support, &med2);
      const int64_t cell = r * width + c;
      support[cell] = k;
      guide[cell] = locale_guide_bits(k, min_support, med2);
    }
    __syncthreads();                                   // (the next tile overwrites the image)
  }
}

}  // namespace bgnn

using namespace bgnn;

extern "C" int bgnn_locale_guide(bgnn_ctx *ctx, const int32_t *n_hyp, const int32_t *chosen, const int64_t *center2, int64_t height,
                                 int64_t width, int32_t radius, int32_t min_support, float *guide, int32_t *support) {
  const char *fn = "bgnn_locale_guide";
  BGNN_REQUIRE(n_hyp && chosen && center2 && guide && support, "%s: NULL argument", fn);
  BGNN_REQUIRE(height >= 1 && width >= 1, "%s: a grid of %lld x %lld cells, at least 1 x 1 expected", fn, (long long)height,
               (long long)width);
  BGNN_REQUIRE(height <= LC_MAX_CELLS / width, "%s: %lld x %lld cells, %lld at the most expected", fn, (long long)height,
               (long long)width, (long long)LC_MAX_CELLS);
  BGNN_REQUIRE(radius >= 1 && radius <= LC_MAX_R, "%s: a radius of %d, 1 .. %d expected", fn, (int)radius, LC_MAX_R);
  const int32_t window = (2 * radius + 1) * (2 * radius + 1) - 1;
  BGNN_REQUIRE(min_support >= 1 && min_support <= window, "%s: a min_support of %d, 1 .. %d expected at radius %d", fn, (int)min_support,
               (int)window, (int)radius);
  BGNN_REQUIRE(aligned8(center2), "%s: center2 is not 8-byte aligned", fn);
  BGNN_REQUIRE(ctx, "%s: NULL context", fn);
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  const int64_t tiles_x = (width + LC_TILE_W - 1) / LC_TILE_W, tiles_y = (height + LC_TILE_H - 1) / LC_TILE_H;
  const int64_t n_tiles = tiles_x * tiles_y;
  hipLaunchKernelGGL(locale_guide_tiles, dim3(capped_grid(n_tiles, PLANE_MAX_GRID)), dim3(LC_THREADS), 0, ctx->stream, n_hyp, chosen,
                     center2, height, width, (int)radius, min_support, tiles_x, n_tiles, reinterpret_cast<uint32_t *>(guide), support);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
