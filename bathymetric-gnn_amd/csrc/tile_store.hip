// Training tiles cut from planes in HBM (include/bgnn_tilestore.h): the candidate boxes of a plane scanned for their valid and class
// counts, and the kept boxes gathered from up to four planes into flat tile stores with their validity mask.  Both kernels are
// memory-bound copies / counts with the same geometry:
//
//   grid (box, band)   a workgroup takes a band of 32 rows of one box (blockIdx.y strides on when a box has more than 65535
//                      bands); a workgroup whose band lies below its box returns at once.  The grid is a function of the boxes alone
//   wave = row         the four waves of a workgroup take every fourth row of the band; a lane takes the cells lane, lane + 64, ...
//                      of the row, four of them per step, so a wave instruction touches 256 contiguous bytes and four (scan) or up
//                      to sixteen (cut) loads are in flight per lane.  Source rows start at arbitrary columns: 4-byte accesses only
//
//   tile_scan   counts per thread in 64-bit integers, one block_reduce over the four counts, one 64-bit integer atomic add per count
//               and workgroup into the box's row of the table (cleared by the entry point)
//   tile_cut    moves 32-bit words (NaN payloads pass), writes the mask byte of the cell beside them
//
// Every cell address is int64.  Compiled with -ffp-contract=off like its neighbours (the depth predicate is two float32
// comparisons; nothing here contracts).
#include "bgnn_internal.h"
#include "plane_util.h"
#include "tile_boxes.h"

namespace bgnn {
namespace {

constexpr int TS_THREADS = BLOCK_THREADS;
constexpr int TS_BAND = BGNN_TILE_BAND_ROWS;
constexpr int TS_WAVES = TS_THREADS / 64;
constexpr int TS_STEP = 4;                            // cells of a lane per step along a row, 64 apart
constexpr int TS_MAX_GRID_Y = 65535;
constexpr int MODE_NONE = 2;                          // tile_cut without a mask
static_assert(TS_THREADS == 256 && TS_BAND % TS_WAVES == 0, "four waves share the rows of a band evenly");

template <int MODE>
__device__ __forceinline__ bool cell_valid(uint32_t bits, float nodata) {
  if (MODE == BGNN_TILE_VALID_LABEL) return (int32_t)bits >= 0;
  const float d = __uint_as_float(bits);
  return finite_bits(d) && d != nodata;               // (a NaN nodata: unequal to everything)
}
// what a lane past the end of the row holds: invalid under either predicate, of no class
template <int MODE>
__device__ __forceinline__ uint32_t outside_bits() { return MODE == BGNN_TILE_VALID_LABEL ? 0xFFFFFFFFu : 0x7FC00000u; }

struct Count4 { unsigned long long v[BGNN_TILE_COUNTS]; };
struct Count4Sum {
  __device__ __forceinline__ Count4 operator()(const Count4 &a, const Count4 &b) const {
    Count4 r;
#pragma unroll
    for (int q = 0; q < BGNN_TILE_COUNTS; ++q) r.v[q] = a.v[q] + b.v[q];
    return r;
  }
};

template <int MODE>
__global__ __launch_bounds__(TS_THREADS) void tile_scan(const uint32_t *__restrict__ plane, int64_t cols,
                                                        const bgnn_tile_box *__restrict__ boxes, unsigned long long *counts,
                                                        float nodata) {
  __shared__ Count4 scratch[TS_THREADS];
  const bgnn_tile_box b = boxes[blockIdx.x];          // (uniform)
  const int bands = (b.h + TS_BAND - 1) / TS_BAND;
  if ((int)blockIdx.y >= bands) return;               // (uniform: before any barrier)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Count4 n = {{0, 0, 0, 0}};
  for (int band = (int)blockIdx.y; band < bands; band += (int)gridDim.y) {
    const int r_end = min(b.h, (band + 1) * TS_BAND);
    for (int r = band * TS_BAND + wave; r < r_end; r += TS_WAVES) {
      const uint32_t *row = plane + ((b.row0 + r) * cols + b.col0);
      for (int c0 = lane; c0 < b.w; c0 += 64 * TS_STEP) {
        uint32_t v[TS_STEP];
#pragma unroll
        for (int k = 0; k < TS_STEP; ++k) {
          const int c = c0 + 64 * k;
          v[k] = c < b.w ? row[c] : outside_bits<MODE>();
        }
#pragma unroll
        for (int k = 0; k < TS_STEP; ++k) {
          n.v[0] += cell_valid<MODE>(v[k], nodata) ? 1u : 0u;
          if (MODE == BGNN_TILE_VALID_LABEL) {
            n.v[1] += v[k] == 0u ? 1u : 0u;
            n.v[2] += v[k] == 1u ? 1u : 0u;
            n.v[3] += v[k] == 2u ? 1u : 0u;
          }
        }
      }
    }
  }
  const Count4 sum = block_reduce<false>(n, scratch, Count4Sum());
  if (threadIdx.x < BGNN_TILE_COUNTS && sum.v[threadIdx.x] != 0)
    atomicAdd(counts + (int64_t)blockIdx.x * BGNN_TILE_COUNTS + threadIdx.x, sum.v[threadIdx.x]);
}

struct CutArgs {
  const uint32_t *src[BGNN_TILE_MAX_PLANES];          // the given planes, packed to the front
  uint32_t *dst[BGNN_TILE_MAX_PLANES];
  uint8_t *mask;
  const bgnn_tile_box *boxes;
  int64_t cols;
  int32_t n_planes, mask_plane;                       // (mask_plane: an index into the packed list)
  float nodata;
};

template <int MODE>
__global__ __launch_bounds__(TS_THREADS) void tile_cut(CutArgs a) {
  const bgnn_tile_box b = a.boxes[blockIdx.x];        // (uniform)
  const int bands = (b.h + TS_BAND - 1) / TS_BAND;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int band = (int)blockIdx.y; band < bands; band += (int)gridDim.y) {
    const int r_end = min(b.h, (band + 1) * TS_BAND);
    for (int r = band * TS_BAND + wave; r < r_end; r += TS_WAVES) {
      const int64_t from = (b.row0 + r) * a.cols + b.col0;
      const int64_t to = b.dst + (int64_t)r * b.w;
      for (int c0 = lane; c0 < b.w; c0 += 64 * TS_STEP) {
        uint32_t v[BGNN_TILE_MAX_PLANES][TS_STEP];
#pragma unroll
        for (int p = 0; p < BGNN_TILE_MAX_PLANES; ++p) {
          if (p < a.n_planes) {
#pragma unroll
            for (int k = 0; k < TS_STEP; ++k) {
              const int c = c0 + 64 * k;
              v[p][k] = c < b.w ? a.src[p][from + c] : 0u;
            }
          }
        }
#pragma unroll
        for (int p = 0; p < BGNN_TILE_MAX_PLANES; ++p) {
          if (p < a.n_planes) {
#pragma unroll
            for (int k = 0; k < TS_STEP; ++k) {
              const int c = c0 + 64 * k;
              if (c < b.w) {
                a.dst[p][to + c] = v[p][k];
                if (MODE != MODE_NONE && p == a.mask_plane) a.mask[to + c] = cell_valid<MODE>(v[p][k], a.nodata) ? 1 : 0;
              }
            }
          }
        }
      }
    }
  }
}

inline dim3 box_grid(int64_t n_boxes, int64_t max_bands) {
  return dim3((uint32_t)n_boxes, (uint32_t)(max_bands < TS_MAX_GRID_Y ? max_bands : TS_MAX_GRID_Y));
}

// the checks both entry points share; on BGNN_OK `check` holds the band count
int check_call(const char *who, int64_t rows, int64_t cols, const bgnn_tile_box *boxes, int64_t n_boxes, int64_t dst_cells,
               const void *ws, size_t ws_bytes, TileBoxCheck &check) {
  BGNN_REQUIRE(rows >= 1 && cols >= 1, "%s: a plane of %lld x %lld cells", who, (long long)rows, (long long)cols);
  BGNN_REQUIRE(n_boxes >= 0, "%s: %lld boxes", who, (long long)n_boxes);
  if (n_boxes > 2147483647) {
    set_error("%s: %lld boxes, at most 2^31 - 1 per call", who, (long long)n_boxes);
    return BGNN_ERR_UNSUPPORTED;
  }
  if (n_boxes == 0) return BGNN_OK;
  BGNN_REQUIRE(boxes && ws, "%s: NULL argument", who);
  check = tile_boxes_check(boxes, n_boxes, rows, cols, dst_cells);
  BGNN_REQUIRE(check.ok, "%s: %s", who, check.message.c_str());
  const size_t need = bgnn_tile_workspace_bytes(n_boxes);
  BGNN_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
  BGNN_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: the workspace is not 16-byte aligned", who);
  return BGNN_OK;
}

}  // namespace
}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_tile_workspace_bytes(int64_t n_boxes) {
  if (n_boxes < 0 || n_boxes > 2147483647) return 0;
  return align256((size_t)n_boxes * BGNN_TILE_BOX_BYTES);
}

extern "C" int bgnn_tile_scan(bgnn_ctx *ctx, const void *plane, int64_t rows, int64_t cols, int32_t mode, double nodata,
                              const bgnn_tile_box *boxes, int64_t n_boxes, void *ws, size_t ws_bytes, int64_t *counts) {
  BGNN_REQUIRE(ctx && plane, "bgnn_tile_scan: NULL argument");
  BGNN_REQUIRE(mode == BGNN_TILE_VALID_LABEL || mode == BGNN_TILE_VALID_DEPTH, "bgnn_tile_scan: unknown mode %d", (int)mode);
  BGNN_REQUIRE(((uintptr_t)plane & 3) == 0, "bgnn_tile_scan: the plane is not 4-byte aligned");
  TileBoxCheck check;
  BGNN_TRY(check_call("bgnn_tile_scan", rows, cols, boxes, n_boxes, -1, ws, ws_bytes, check));
  if (n_boxes == 0) return BGNN_OK;
  BGNN_REQUIRE(counts, "bgnn_tile_scan: NULL argument");
  BGNN_REQUIRE(((uintptr_t)counts & 7) == 0, "bgnn_tile_scan: the count table is not 8-byte aligned");

  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  BGNN_TRY(ctx_upload(ctx, boxes, (size_t)n_boxes * BGNN_TILE_BOX_BYTES, ws));
  BGNN_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)n_boxes * BGNN_TILE_COUNTS * sizeof(int64_t), ctx->stream));
  const dim3 grid = box_grid(n_boxes, check.max_bands), block(TS_THREADS);
  const uint32_t *p = static_cast<const uint32_t *>(plane);
  const bgnn_tile_box *d_boxes = static_cast<const bgnn_tile_box *>(ws);
  unsigned long long *c = reinterpret_cast<unsigned long long *>(counts);
  if (mode == BGNN_TILE_VALID_LABEL)
    hipLaunchKernelGGL(tile_scan<BGNN_TILE_VALID_LABEL>, grid, block, 0, ctx->stream, p, cols, d_boxes, c, (float)nodata);
  else
    hipLaunchKernelGGL(tile_scan<BGNN_TILE_VALID_DEPTH>, grid, block, 0, ctx->stream, p, cols, d_boxes, c, (float)nodata);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

extern "C" int bgnn_tile_cut(bgnn_ctx *ctx, const void *const *planes, void *const *dst, int32_t n_planes, int64_t rows, int64_t cols,
                             uint8_t *mask, int32_t mask_plane, int32_t mode, double nodata, const bgnn_tile_box *boxes,
                             int64_t n_boxes, int64_t dst_cells, void *ws, size_t ws_bytes) {
  BGNN_REQUIRE(ctx && planes && dst, "bgnn_tile_cut: NULL argument");
  BGNN_REQUIRE(n_planes >= 1 && n_planes <= BGNN_TILE_MAX_PLANES, "bgnn_tile_cut: %d planes, 1 to %d per call", (int)n_planes,
               BGNN_TILE_MAX_PLANES);
  BGNN_REQUIRE(dst_cells >= 0, "bgnn_tile_cut: a store of %lld cells", (long long)dst_cells);
  CutArgs a = {};
  a.mask_plane = -1;
  for (int i = 0; i < n_planes; ++i) {
    BGNN_REQUIRE((planes[i] != nullptr) == (dst[i] != nullptr), "bgnn_tile_cut: plane %d has %s", i,
                 planes[i] ? "no destination" : "a destination and no source");
    if (!planes[i]) continue;
    BGNN_REQUIRE(((uintptr_t)planes[i] & 3) == 0 && ((uintptr_t)dst[i] & 3) == 0, "bgnn_tile_cut: plane %d or its store is not 4-byte aligned", i);
    if (mask && i == mask_plane) a.mask_plane = a.n_planes;
    a.src[a.n_planes] = static_cast<const uint32_t *>(planes[i]);
    a.dst[a.n_planes] = static_cast<uint32_t *>(dst[i]);
    ++a.n_planes;
  }
  BGNN_REQUIRE(a.n_planes >= 1, "bgnn_tile_cut: no plane is given");
  if (mask) {
    BGNN_REQUIRE(mode == BGNN_TILE_VALID_LABEL || mode == BGNN_TILE_VALID_DEPTH, "bgnn_tile_cut: unknown mode %d", (int)mode);
    BGNN_REQUIRE(a.mask_plane >= 0, "bgnn_tile_cut: mask_plane %d names no given plane", (int)mask_plane);
  }
  TileBoxCheck check;
  BGNN_TRY(check_call("bgnn_tile_cut", rows, cols, boxes, n_boxes, dst_cells, ws, ws_bytes, check));
  if (n_boxes == 0) return BGNN_OK;
  // (rows * cols * 4 stays below 2^64 for every plane that exists; the product is formed in 64-bit unsigned)
  const uint64_t plane_bytes = (uint64_t)rows * (uint64_t)cols * 4u, store_bytes = (uint64_t)dst_cells * 4u;
  for (int i = 0; i < a.n_planes; ++i) {
    for (int j = 0; j < a.n_planes; ++j)
      BGNN_REQUIRE(!ranges_overlap((uintptr_t)a.dst[i], store_bytes, (uintptr_t)a.src[j], plane_bytes),
                   "bgnn_tile_cut: a destination overlaps a source plane");
    BGNN_REQUIRE(!mask || !ranges_overlap((uintptr_t)mask, (uint64_t)dst_cells, (uintptr_t)a.src[i], plane_bytes),
                 "bgnn_tile_cut: the mask overlaps a source plane");
  }

  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  BGNN_TRY(ctx_upload(ctx, boxes, (size_t)n_boxes * BGNN_TILE_BOX_BYTES, ws));
  a.mask = mask;
  a.boxes = static_cast<const bgnn_tile_box *>(ws);
  a.cols = cols;
  a.nodata = (float)nodata;
  const dim3 grid = box_grid(n_boxes, check.max_bands), block(TS_THREADS);
  if (!mask) hipLaunchKernelGGL(tile_cut<MODE_NONE>, grid, block, 0, ctx->stream, a);
  else if (mode == BGNN_TILE_VALID_LABEL) hipLaunchKernelGGL(tile_cut<BGNN_TILE_VALID_LABEL>, grid, block, 0, ctx->stream, a);
  else hipLaunchKernelGGL(tile_cut<BGNN_TILE_VALID_DEPTH>, grid, block, 0, ctx->stream, a);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
