// Training tiles gathered from a flat tile store under the eight symmetries of the square (include/bgnn_augment.h): one launch
// copies the tiles of a batch out of the store, each under its own op, for up to four 4-byte planes and one 1-byte plane.  A
// memory-bound copy; the only question is which way the lanes run.
//
//   grid (entry, block)  a workgroup of 256 threads takes one 64 x 64 block of one entry's OUTPUT tile, for all planes (blockIdx.y
//                        strides on when a tile has more than 65535 blocks).  The grid is a function of the entries alone
//   even k (0 2 4 6)     identity, 180 degrees and the two mirrors keep rows as rows: a wave takes every fourth output row of the
//                        block, lane = output column.  The source cells of a wave instruction are one contiguous 256-byte segment,
//                        ascending or (mirrored columns) descending in the lane.  No LDS, no barrier
//   odd k (1 3 5 7)      rows become columns, so the block passes through LDS.  Load: a wave takes every fourth output COLUMN jj,
//                        lane = output row ii: the source cells are again one contiguous row segment (ascending or descending),
//                        written to img[jj][ii].  Barrier.  Store: a wave takes every fourth output row ii, lane = output column jj,
//                        reads img[jj][ii] and writes one contiguous output row segment.  No global access has its lanes a row apart
//   the image            uint32 [64][65].  The load phase writes a row of it (lanes on consecutive words); the store phase reads a
//                        column, lanes 65 words apart: ds_read_b32 banks are (word % 32) per 32-lane half, and 65 * l % 32 = l % 32,
//                        so neither phase has a conflict.  (At a row stride of 64 the column read would be 32-way.)
//   planes               the block's offsets are worked out once and every plane goes through them.  Two images alternate from
//                        plane to plane, so one barrier per plane is enough: an image is written again two planes later, and the
//                        barrier in between is passed only after every thread has read it
//   the byte plane       is widened to words on its way through the same image: one code path, and a byte image (row stride 65
//                        bytes) would put four lanes on every bank of the column read
//
// Values are never interpreted: 32-bit words and bytes are moved.  Every cell address is int64.  Compiled with -ffp-contract=off
// like its neighbours (there is no float arithmetic here at all).
//
// Resources (tools/kernel_resources.py tile_augment.hip, gfx950):  tile_gather  VGPR 47  AGPR 0  scratch 0  LDS 33280 bytes (two
// images of 64 * 65 words)  occupancy 4 waves per SIMD: four workgroups per CU, which is what the LDS allows (4 * 33280 of 160 KiB).
#include "bgnn_internal.h"
#include "plane_util.h"
#include "tile_boxes.h"
#include "../../include/bgnn_augment.h"

namespace bgnn {
namespace {

constexpr int AG_THREADS = BLOCK_THREADS;
constexpr int AG_B = BGNN_AUG_BLOCK;
constexpr int AG_WAVES = AG_THREADS / 64;
constexpr int AG_ROWS = AG_B / AG_WAVES;              // rows (or columns) of a block per wave
constexpr int AG_STEP = 4;                            // rows of the direct path in flight per plane
constexpr int AG_MAX_GRID_Y = 65535;
// which ops read the source rows / columns backwards (the table of bgnn_augment.h): bit `op`
constexpr unsigned AG_FLIP_ROWS = 0xCCu;              // ops 2 3 6 7
constexpr unsigned AG_FLIP_COLS = 0x96u;              // ops 1 2 4 7
static_assert(sizeof(bgnn_tile_entry) == BGNN_AUG_ENTRY_BYTES, "an entry is four 8-byte words");
static_assert(AG_THREADS == 256 && AG_B == 64 && AG_ROWS % AG_STEP == 0, "lane = one cell of a 64-cell segment, four waves share the block");
static_assert(BGNN_AUG_MAX_PLANES == 4, "GatherArgs holds four pairs");

struct GatherArgs {
  const uint32_t *src[BGNN_AUG_MAX_PLANES];           // the given planes, packed to the front
  uint32_t *dst[BGNN_AUG_MAX_PLANES];
  const uint8_t *src_mask;                            // the byte plane, or both NULL
  uint8_t *dst_mask;
  const bgnn_tile_entry *entries;
  int32_t n_planes;
};

// Where a block's cells lie.  Row r = wave + AG_WAVES * q (q = 0 .. AG_ROWS - 1) of a phase, lane l:
//   load   cell from + q * from_step   valid: q < n_load  and load_lane
//   store  cell to + q * to_step       valid: q < n_store and store_lane
struct BlockWalk {
  int64_t from, from_step, to, to_step;
  int n_load, n_store;
  bool load_lane, store_lane;
};

// rows r = first, first + AG_WAVES, ... below `end`: how many
__device__ __forceinline__ int rows_below(int first, int end) {
  const int n = (end - first + AG_WAVES - 1) / AG_WAVES;
  return n < 0 ? 0 : (n > AG_ROWS ? AG_ROWS : n);
}

// even k: output rows straight from source rows
template <class T>
__device__ __forceinline__ void copy_rows(const T *__restrict__ s, T *__restrict__ d, const BlockWalk &k) {
  if (!k.store_lane) return;
  for (int q0 = 0; q0 < k.n_store; q0 += AG_STEP) {
    T v[AG_STEP];
#pragma unroll
    for (int q = 0; q < AG_STEP; ++q)
      if (q0 + q < k.n_store) v[q] = s[k.from + (q0 + q) * k.from_step];
#pragma unroll
    for (int q = 0; q < AG_STEP; ++q)
      if (q0 + q < k.n_store) d[k.to + (q0 + q) * k.to_step] = v[q];
  }
}

// odd k: through one LDS image (the barrier is the caller's `turn` below: every thread of the workgroup comes here)
template <class T>
__device__ __forceinline__ void turn_block(const T *__restrict__ s, T *__restrict__ d, const BlockWalk &k,
                                           uint32_t (*img)[AG_B + 1], int lane, int wave) {
  if (k.load_lane) {
    T v[AG_ROWS];
#pragma unroll
    for (int q = 0; q < AG_ROWS; ++q)
      if (q < k.n_load) v[q] = s[k.from + q * k.from_step];
#pragma unroll
    for (int q = 0; q < AG_ROWS; ++q)
      if (q < k.n_load) img[wave + AG_WAVES * q][lane] = (uint32_t)v[q];
  }
  __syncthreads();
  if (k.store_lane) {
#pragma unroll
    for (int q = 0; q < AG_ROWS; ++q)
      if (q < k.n_store) d[k.to + q * k.to_step] = (T)img[lane][wave + AG_WAVES * q];
  }
}

__global__ __launch_bounds__(AG_THREADS) void tile_gather(GatherArgs a) {
  __shared__ uint32_t img[2][AG_B][AG_B + 1];
  const bgnn_tile_entry e = a.entries[blockIdx.x];    // (uniform)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool odd = (e.op & 1) != 0;
  const bool flip_rows = ((AG_FLIP_ROWS >> e.op) & 1u) != 0, flip_cols = ((AG_FLIP_COLS >> e.op) & 1u) != 0;
  const int oh = odd ? e.w : e.h, ow = odd ? e.h : e.w;                       // the output tile
  const int64_t blocks_x = ((int64_t)ow + AG_B - 1) / AG_B, blocks = (((int64_t)oh + AG_B - 1) / AG_B) * blocks_x;
  unsigned turn = 0;                                  // images used so far: the next plane takes img[turn & 1]
  for (int64_t b = blockIdx.y; b < blocks; b += gridDim.y) {                  // (uniform: every thread meets the same barriers)
    const int r0 = (int)(b / blocks_x) * AG_B, c0 = (int)(b % blocks_x) * AG_B;   // the block's first output row and column
    BlockWalk k;
    // store phase, both paths: output row r0 + wave + 4 q, output column c0 + lane
    k.n_store = rows_below(r0 + wave, oh);
    k.store_lane = c0 + lane < ow;
    k.to = e.dst + (int64_t)(r0 + wave) * ow + (c0 + lane);
    k.to_step = (int64_t)AG_WAVES * ow;
    if (!odd) {
      // out[i][j] = t[flip_rows ? h-1-i : i][flip_cols ? w-1-j : j]
      const int i = r0 + wave, j = c0 + lane;
      const int64_t sr = flip_rows ? (int64_t)e.h - 1 - i : i, sc = flip_cols ? (int64_t)e.w - 1 - j : j;
      k.from = e.src + sr * e.w + sc;
      k.from_step = (flip_rows ? -(int64_t)AG_WAVES : (int64_t)AG_WAVES) * e.w;
      k.n_load = k.n_store;
      k.load_lane = k.store_lane;
#pragma unroll
      for (int p = 0; p < BGNN_AUG_MAX_PLANES; ++p)
        if (p < a.n_planes) copy_rows(a.src[p], a.dst[p], k);
      if (a.src_mask) copy_rows(a.src_mask, a.dst_mask, k);
    } else {
      // out[i][j] = t[flip_rows ? h-1-j : j][flip_cols ? w-1-i : i]; load phase: output column j = c0 + wave + 4 q, output row
      // i = r0 + lane, so a wave instruction walks ONE source row, along it
      const int j = c0 + wave, i = r0 + lane;
      const int64_t sr = flip_rows ? (int64_t)e.h - 1 - j : j, sc = flip_cols ? (int64_t)e.w - 1 - i : i;
      k.from = e.src + sr * e.w + sc;
      k.from_step = (flip_rows ? -(int64_t)AG_WAVES : (int64_t)AG_WAVES) * e.w;
      k.n_load = rows_below(j, ow);
      k.load_lane = i < oh;
#pragma unroll
      for (int p = 0; p < BGNN_AUG_MAX_PLANES; ++p)
        if (p < a.n_planes) turn_block(a.src[p], a.dst[p], k, img[turn++ & 1], lane, wave);
      if (a.src_mask) turn_block(a.src_mask, a.dst_mask, k, img[turn++ & 1], lane, wave);
    }
  }
}

struct EntryCheck {
  bool ok = true;
  std::string message;
  int64_t max_blocks = 0;     // 64 x 64 blocks of the largest tile
};

// Every entry inside both stores.  No sum here can overflow: src <= src_cells - cells is compared, and h * w < 2^62.
EntryCheck entries_check(const bgnn_tile_entry *entries, int64_t n, int64_t src_cells, int64_t dst_cells) {
  EntryCheck c;
  auto fail = [&](int64_t k, const char *why) {
    char buf[256];
    const bgnn_tile_entry &e = entries[k];
    snprintf(buf, sizeof buf, "entry %lld (src %lld, dst %lld, %d x %d, op %d) %s", (long long)k, (long long)e.src, (long long)e.dst,
             (int)e.h, (int)e.w, (int)e.op, why);
    c.ok = false;
    c.message = buf;
    return c;
  };
  for (int64_t k = 0; k < n; ++k) {
    const bgnn_tile_entry &e = entries[k];
    if (e.op < 0 || e.op >= BGNN_AUG_OPS) return fail(k, "names no op (0 .. 7)");
    if (e.h < 1 || e.w < 1) return fail(k, "is empty");
    if (e.src < 0 || e.dst < 0) return fail(k, "has a negative offset");
    const int64_t cells = (int64_t)e.h * e.w;
    if (cells > src_cells || e.src > src_cells - cells) return fail(k, "starts past the source store's end");
    if (cells > dst_cells || e.dst > dst_cells - cells) return fail(k, "ends past the destination store");
    const int64_t blocks = (((int64_t)e.h + AG_B - 1) / AG_B) * (((int64_t)e.w + AG_B - 1) / AG_B);
    if (blocks > c.max_blocks) c.max_blocks = blocks;
  }
  return c;
}

}  // namespace
}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_tile_gather_workspace_bytes(int64_t n_entries) {
  if (n_entries < 0 || n_entries > 2147483647) return 0;
  return align256((size_t)n_entries * BGNN_AUG_ENTRY_BYTES);
}

extern "C" int bgnn_tile_gather(bgnn_ctx *ctx, const void *const *src, void *const *dst, int32_t n_planes, const uint8_t *src_mask,
                                uint8_t *dst_mask, int64_t src_cells, int64_t dst_cells, const bgnn_tile_entry *entries,
                                int64_t n_entries, void *ws, size_t ws_bytes) {
  BGNN_REQUIRE(ctx, "bgnn_tile_gather: NULL argument");
  BGNN_REQUIRE(n_planes >= 0 && n_planes <= BGNN_AUG_MAX_PLANES, "bgnn_tile_gather: %d planes, at most %d per call", (int)n_planes,
               BGNN_AUG_MAX_PLANES);
  BGNN_REQUIRE(n_planes == 0 || (src && dst), "bgnn_tile_gather: NULL argument");
  BGNN_REQUIRE(src_cells >= 0 && dst_cells >= 0, "bgnn_tile_gather: stores of %lld and %lld cells", (long long)src_cells,
               (long long)dst_cells);
  GatherArgs a = {};
  for (int i = 0; i < n_planes; ++i) {
    BGNN_REQUIRE((src[i] != nullptr) == (dst[i] != nullptr), "bgnn_tile_gather: plane %d has %s", i,
                 src[i] ? "no destination" : "a destination and no source");
    if (!src[i]) continue;
    BGNN_REQUIRE(((uintptr_t)src[i] & 3) == 0 && ((uintptr_t)dst[i] & 3) == 0, "bgnn_tile_gather: plane %d or its store is not 4-byte aligned", i);
    a.src[a.n_planes] = static_cast<const uint32_t *>(src[i]);
    a.dst[a.n_planes] = static_cast<uint32_t *>(dst[i]);
    ++a.n_planes;
  }
  BGNN_REQUIRE((src_mask != nullptr) == (dst_mask != nullptr), "bgnn_tile_gather: the byte plane has %s",
               src_mask ? "no destination" : "a destination and no source");
  BGNN_REQUIRE(a.n_planes >= 1 || src_mask, "bgnn_tile_gather: no plane is given");
  BGNN_REQUIRE(n_entries >= 0, "bgnn_tile_gather: %lld entries", (long long)n_entries);
  if (n_entries > 2147483647) {
    set_error("bgnn_tile_gather: %lld entries, at most 2^31 - 1 per call", (long long)n_entries);
    return BGNN_ERR_UNSUPPORTED;
  }
  if (n_entries == 0) return BGNN_OK;
  BGNN_REQUIRE(entries && ws, "bgnn_tile_gather: NULL argument");
  const EntryCheck check = entries_check(entries, n_entries, src_cells, dst_cells);
  BGNN_REQUIRE(check.ok, "bgnn_tile_gather: %s", check.message.c_str());
  const size_t need = bgnn_tile_gather_workspace_bytes(n_entries);
  BGNN_REQUIRE(ws_bytes >= need, "bgnn_tile_gather: workspace of %zu bytes, %zu needed", ws_bytes, need);
  BGNN_REQUIRE(((uintptr_t)ws & 15) == 0, "bgnn_tile_gather: the workspace is not 16-byte aligned");
  // every destination against every source, the byte plane included (a store of 2^61 cells does not exist: the products fit)
  const uint64_t src_bytes = (uint64_t)src_cells * 4u, dst_bytes = (uint64_t)dst_cells * 4u;
  for (int i = 0; i < a.n_planes; ++i) {
    for (int j = 0; j < a.n_planes; ++j)
      BGNN_REQUIRE(!ranges_overlap((uintptr_t)a.dst[i], dst_bytes, (uintptr_t)a.src[j], src_bytes),
                   "bgnn_tile_gather: a destination overlaps a source");
    BGNN_REQUIRE(!src_mask || (!ranges_overlap((uintptr_t)a.dst[i], dst_bytes, (uintptr_t)src_mask, (uint64_t)src_cells) &&
                               !ranges_overlap((uintptr_t)dst_mask, (uint64_t)dst_cells, (uintptr_t)a.src[i], src_bytes)),
                 "bgnn_tile_gather: a destination overlaps a source");
  }
  BGNN_REQUIRE(!src_mask || !ranges_overlap((uintptr_t)dst_mask, (uint64_t)dst_cells, (uintptr_t)src_mask, (uint64_t)src_cells),
               "bgnn_tile_gather: a destination overlaps a source");

  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  BGNN_TRY(ctx_upload(ctx, entries, (size_t)n_entries * BGNN_AUG_ENTRY_BYTES, ws));
  a.src_mask = src_mask;
  a.dst_mask = dst_mask;
  a.entries = static_cast<const bgnn_tile_entry *>(ws);
  const dim3 grid((uint32_t)n_entries, (uint32_t)(check.max_blocks < AG_MAX_GRID_Y ? check.max_blocks : AG_MAX_GRID_Y)), block(AG_THREADS);
  hipLaunchKernelGGL(tile_gather, grid, block, 0, ctx->stream, a);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
