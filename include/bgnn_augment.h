/*
 * bgnn_augment.h -- C ABI of libbgnn_hip.so, training tiles gathered from a flat tile store under the eight symmetries of the square
 * (ABI 7, additive; no entry point of bgnn.h or of the other side headers changes).  The reference's TrainingConfig carries
 * augment_rotations / augment_flips and never reads them; this is what they stand for: a batch's tiles copied out of the store,
 * each turned or mirrored on the way, all planes of the batch in one launch.
 *
 * The transform.  op = k + 4 * f, k in 0 .. 3, f in 0 .. 1.  For a source tile t of h x w cells
 *     out = rot90(fliplr(t) if f else t, k)            (numpy: rot90 turns counter-clockwise, fliplr mirrors the columns)
 * which is, cell by cell (out[i][j] on the left; odd k: the output has w rows of h cells),
 *     op 0  t[i][j]              identity                  op 4  t[i][w-1-j]          fliplr
 *     op 1  t[j][w-1-i]          90 degrees                op 5  t[j][i]              transpose
 *     op 2  t[h-1-i][w-1-j]      180 degrees               op 6  t[h-1-i][j]          flipud
 *     op 3  t[h-1-j][i]          270 degrees               op 7  t[h-1-j][w-1-i]      anti-transpose
 * These eight are the whole dihedral group of the square.  Inverses: op 0 is the identity; a rotation k (f = 0) is undone by
 * (4 - k) % 4, so 1 <-> 3 and 2 is its own inverse; every op with f = 1 (4, 5, 6, 7) is its own inverse.  A caller that turns a tile
 * with odd k swaps the tile's resolution pair (x, y) as well: the call knows nothing of resolutions.
 *
 * An entry names one source tile, its place in the output and its op:
 *     the source is read row-major, h x w cells, from cell `src` of the source stores on;
 *     the output tile is written row-major from cell `dst` of the destination stores on, with the transformed extent.
 * Entries are a HOST array.  Every entry is checked before anything is launched (op in 0 .. 7, h >= 1, w >= 1, src >= 0, dst >= 0,
 * src + h * w <= src_cells, dst + h * w <= dst_cells); then the table travels through the context's pinned staging into the
 * caller's workspace: the caller's copy may go away when the call returns.  Two entries may read the same source tile (with equal
 * or different ops).  The destination tiles must not overlap each other (not checked: the caller lays them out back to back).
 *
 * Workspace.  DEVICE scratch of at least bgnn_tile_gather_workspace_bytes(n_entries) bytes, 16-byte aligned, from the caller: the
 * entry table.  The library keeps no slot for it.
 *
 * The conventions of bgnn.h hold (DEVICE / HOST pointers, return codes, bgnn_last_error(), the context's stream, asynchronous): the
 * entry point does not synchronise with the host, allocate, or copy to the host.  Every argument check runs before the context or the
 * device is touched.  The Python mirror binds these in bathymetric_gnn_amd/runtime.py (_AUGMENT_SIGNATURES); training/trainer.py
 * (TileStore.gather, TileStore.batch(ops=...), Trainer(augment_geometry=True)) drives them.
 *
 * Geometry.  The grid comes from the entries alone: a workgroup of 256 threads takes one BGNN_AUG_BLOCK x BGNN_AUG_BLOCK block of one
 * entry's OUTPUT tile, for all planes.  Ops with even k move row segments directly (a mirrored row is still one contiguous segment
 * per wave instruction); ops with odd k pass the block through LDS, so that both the reads and the writes run along rows.  Every
 * cell address is 64-bit: the stores may hold more than 2^31 cells.
 *
 * Determinism.  The call moves 32-bit words and bytes and never interprets them: NaN payloads, infinities and -1 labels pass.  There
 * are no atomics and no arithmetic on the values.  Equal inputs give equal bits.
 */
#ifndef BGNN_AUGMENT_H
#define BGNN_AUGMENT_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_AUG_OPS 8              /* the dihedral group: op = k + 4 * f */
#define BGNN_AUG_MAX_PLANES 4       /* 4-byte planes of one gather */
#define BGNN_AUG_BLOCK 64           /* rows and columns of an output block behind one workgroup */
#define BGNN_AUG_ENTRY_BYTES 32     /* sizeof(bgnn_tile_entry) */

typedef struct bgnn_tile_entry {
  int64_t src;          /* cell offset of the source tile in the source stores */
  int64_t dst;          /* cell offset of the output tile in the destination stores */
  int32_t h, w;         /* extent of the SOURCE tile (the output is h x w for even k, w x h for odd k) */
  int32_t op;           /* k + 4 * f, 0 .. 7 */
  int32_t pad;          /* not read */
} bgnn_tile_entry;

/* bgnn_tile_gather_workspace_bytes: BGNN_AUG_ENTRY_BYTES * n_entries rounded up to 256; 0 for n_entries outside [0, 2^31 - 1].  The
 * gather answers more than 2^31 - 1 entries with BGNN_ERR_UNSUPPORTED: split the table. */
size_t bgnn_tile_gather_workspace_bytes(int64_t n_entries);

/* bgnn_tile_gather: one launch.  src, dst: HOST arrays of n_planes DEVICE pointers, 0 <= n_planes <= BGNN_AUG_MAX_PLANES.
 *   src[i]: a flat store of src_cells 4-byte elements (int32 or float32: the words are moved, not interpreted); dst[i]: a flat store
 *   of dst_cells such elements.  Pair i with src[i] == NULL and dst[i] == NULL is absent (a store without uncertainty); one of the
 *   two alone is refused, and so are more than BGNN_AUG_MAX_PLANES planes: gather those in a second call.  With n_planes == 0 src and
 *   dst are not read.
 *   src_mask, dst_mask: DEVICE uint8 [src_cells] / [dst_cells], both or neither: a 1-byte plane moved like the others.
 *   At least one plane, word or byte, must be given.  No destination may overlap a source.
 *   n_entries == 0 launches nothing and writes nothing (entries and ws may then be NULL).
 *   BGNN_ERR_INVALID: a NULL ctx / src / dst / entries / ws, n_planes outside 0 .. BGNN_AUG_MAX_PLANES, a half-given pair (mask
 *   included), no plane at all, src_cells < 0 or dst_cells < 0, n_entries < 0, an entry outside the contract above, a destination
 *   that overlaps a source, a workspace that is too small or not 16-byte aligned, a 4-byte plane that is not 4-byte aligned. */
int bgnn_tile_gather(bgnn_ctx *ctx, const void *const *src, void *const *dst, int32_t n_planes, const uint8_t *src_mask,
                     uint8_t *dst_mask, int64_t src_cells, int64_t dst_cells, const bgnn_tile_entry *entries, int64_t n_entries,
                     void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_AUGMENT_H */
