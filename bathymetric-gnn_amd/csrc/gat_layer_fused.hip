// Fused GAT layer for stencil graphs (gfx950):  aggregate_l  ->  BN/ReLU  ->  GEMM_{l+1}
//
// One workgroup (256 threads = 4 waves; two workgroups per CU) owns an 8x16 block of cells of one tile and
// produces, for those 128 nodes, what the NEXT stage needs:
//   EPI_NEXT : xw_{l+1} = h_{l+1} @ W_{l+1}^T  and its attention dots (alpha_src, alpha_dst)
//   EPI_HEADS: the three output heads, softmax / argmax / sigmoid, the predict() flags and
//              (optionally) the classification / confidence / correction GRIDS of
//              BathymetricPipeline._process_tile -- i.e. K4(last) + K5 + K6 in one launch.
// h_{l+1} (the aggregate output, 1 KiB/node) never goes to HBM and never even to LDS: per 32-channel slab
// each lane gathers -- from the LDS image of the halo rows -- exactly the 16 values it must supply as the
// MFMA B operand, applies bias + BatchNorm + ReLU in registers and issues a rank-32 update of its wave's
// [32 nodes x NC] accumulator.  HBM traffic per layer drops from read xw + write h + read h + write xw'
// (4.3 KiB/node at HC = 256) to read xw (x1.4 halo, mostly L2) + write xw' (2.3 KiB/node); the kernel is
// then bound by the exact-f32 matrix pipe.
//
// Per slab s:   wait slab | barrier | gather (bf16: 8 aggregation MFMAs) + BN/ReLU in registers | wait W rows 0-15 | barrier | DMA slab s+1 |
//               16 x NT MFMAs | barrier | DMA W rows 0-15 of slab s+1 | 16 x NT MFMAs | barrier | DMA W rows 16-31
// so every DMA has at least half a slab of matrix work (plus the next gather) to land.
//
// Stencils (template K): 4 / 8 (the reference's connectivities, halo of 1 cell: 10 x 18 rows per block) and 16
// ("16-dilated", BASELINE config 3: the 8 base offsets and the same x 2; halo of 2 cells: 12 x 20 rows).
//
// Matrix / storage modes (template SP):
//   0  exact f32: activations f32 in HBM, v_mfma_f32_32x32x2_f32 (default; the parity path)
//   1  bf16x3, 2 fp16x3: activations f32 in HBM, operands split hi + lo in registers, three 16-bit MFMAs (opt-in)
//   3  bf16: activations (xw) stored as bf16 in HBM; the neighbourhood sum (alpha rounded to bf16, AggWindow below) and the GEMM
//      (one v_mfma_f32_32x32x16_bf16 per 16 k) run on the bf16 matrix pipe; softmax, BatchNorm, attention dots and every
//      accumulator stay f32 (BASELINE config 3 "bf16 node features"; not a parity path)
//
// Reference semantics: models/gnn.py:173-188 (conv -> norm -> relu), :392-406 (heads),
// :427-449 (predict), models/pipeline.py:278-307 (grids); GATConv per SURVEY Appendix B.
#include <stdlib.h>
#include <algorithm>
#include <type_traits>
#include <utility>
#include "gat_tile_common.h"

namespace bgnn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

enum { EPI_NEXT = 0, EPI_HEADS = 1 };

// Diagnostics exist only in the -DBGNN_DIAG=1 build (libbgnn_hip_diag.so): phase ablation bits (a.dbg) and per-phase
// s_memtime sums (a.stamps).  In the production build DBG(bit) is the constant false and BGNN_STAMP expands to nothing,
// so neither the tests inside the slab loop nor the live t_prev register pair exist.
#if BGNN_DIAG
#define DBG(bit) (a.dbg & (bit))
// (summed in scalar registers, written out by ONE set of atomics at the very end of the workgroup: an atomic per phase would
//  sit in the VM queue in front of the kernel's counted waits and lengthen them -- the first version did, and measured itself)
#define BGNN_STAMP(slot)                                                                   \
  if (a.stamps) {                                                                          \
    const unsigned long long _t = __builtin_amdgcn_s_memtime();                            \
    t_sum[slot] += _t - t_prev;                                                            \
    t_prev = _t;                                                                           \
  }
#else
#define DBG(bit) false
#define BGNN_STAMP(slot)
#endif

struct FusedArgs {
  TileBlocks tb;
  const int32_t *node_id;
  const int32_t *cell_map; // ragged-batch canvas: original cell of each node (the grids are written through it); else nullptr
  const void *xw;         // [rows][HC]   this layer's lin(x): f32, or bf16 with SP = 3
  const float *asd;       // [rows][2H]
  // the kernels rebuild the edge attributes from the compact storage:
  const float *slope;     // [rows][K]      slope attribute of every stencil slot (graph_build.hip, FeatureArgs)
  const float *node_depth;   // [rows]      depth of every node: depth difference = nan_to_num(depth[target] - depth[source])
  const float4 *tile_dist;   // [n_tiles]   (|dx|, |dy|, diagonal) edge lengths of a tile's unit offsets
  const int32_t *tile_of_cell;   // canvas walk: grid index of every canvas cell (else nullptr: the block's tile)
  const float *V;         // [H][3]
  const float *scale;     // [HC] folded bias + BatchNorm
  const float *shift;
  const float *Wt;        // [HC][NC] next stage weight (transposed); split / bf16 image with SP != 0
  const float *zero_page; // >= 16 B of zeros (source of halo rows that have no node)
  float *dump;            // >= 1 KiB scratch row: stores of rows that have no node land here (keeps the epilogue branch-free)
  int relu, dbg;
  int self_loops, relu2;  // AGG != 0 (plain backbones): the graph carries explicit self loops; ReLU of the post-GEMM epilogue
  unsigned long long *stamps;   // diagnostic build only: per-phase cycle sums
  // EPI_NEXT
  const float *att_src;   // [NC]
  const float *att_dst;
  void *out;              // [rows][NC]  f32, or bf16 with SP = 3
  float *asd_out;         // [rows][2*H2]
  int H2, C2;
  float w_inv;            // SP = 2: the float16 weight image holds W * 2^S (model_pack.hip pack_split); accumulators *= 2^-S before the epilogue
  const float *W0af;      // layer 0 "aggregate first" (gat_layer_bf16_2p_kernel, AF): the folded lin_0 weight as per-head 64 x 64 bf16 images
  // EPI_HEADS
  const float *hd_tab;    // [HEADW] b0 [96] | second-layer rows (cls [classes], conf, corr) at 96 + 32 j | their biases at 288
  const float *local_std; // [rows]
  int classes, hh, has_corr;
  float thr_auto, thr_review, norm_floor;
  bgnn_outputs o;
  float *cls_grid, *conf_grid, *corr_grid;   // [cells] or nullptr
};

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// LDS reads issued from inline asm.  hipcc cannot tell an LDS-DMA's destination from the address of a
// later ds_read, so with a DMA in flight it puts s_waitcnt vmcnt(0) in front of every compiler-visible
// LDS read -- which would serialise the slab / W prefetch with the phase it is meant to hide under.
// These reads are invisible to that pass; the code below waits for them explicitly (lgkmcnt) and fences
// the scheduler (sched_barrier) as the HIP guide's rule 18 requires.
__device__ __forceinline__ uint32_t lds_addr(const void *p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}
template <int OFF>
__device__ __forceinline__ f32x4 lds_read4(uint32_t addr) {
  f32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
template <int OFF>
__device__ __forceinline__ u32x4 lds_read4u(uint32_t addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
template <int OFF>
__device__ __forceinline__ float lds_read1(uint32_t addr) {
  float v;
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
__device__ __forceinline__ void lds_reads_done() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
template <int N>
__device__ __forceinline__ void lds_reads_wait() {       // all but the N youngest LDS operations have returned (they return in order)
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}
template <int OFF>
__device__ __forceinline__ void lds_write1(uint32_t addr, float v) {     // (an LDS write hipcc does not see either: same reason)
  asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory");
}
template <int K, int... B>
__device__ __forceinline__ void lds_write_coefficients(uint32_t addr, const float (&part)[K + 1], std::integer_sequence<int, B...>) {
  (lds_write1<B * 4>(addr, part[B]), ...);
}
template <int OFF>
__device__ __forceinline__ int lds_read1i(uint32_t addr) {
  int v;
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}

// Phase A's operands out of the halo tables (node ids `hid [HR]`, alpha_src `has [HR][H]`) by asm reads: phase A runs while slab
// 0's LDS-DMA is still in flight, and a compiler-visible LDS read there would be given an s_waitcnt vmcnt(0) (see above), i.e.
// the whole phase would queue up behind the DMA instead of passing under it.  Every read's offset is an immediate relative to the
// stencil's lowest halo row (pack expansion over the slots), 2 K + 1 reads in flight, one wait.
template <int K, int HWID>
struct HaloSlot {
  using Off = StencilOffsets<K>;
  static constexpr int R = K == 16 ? 2 : 1;
  static constexpr int MAXOFF = R * HWID + R;                        // self_idx - MAXOFF = the lowest row a slot can address
  static constexpr int rel(int b) { return MAXOFF - (Off::dr[b] * HWID + Off::dc[b]); }   // >= 0: slot b's source row, relative to it
};
template <int K, int HWID, int... B>
__device__ __forceinline__ void halo_ids(uint32_t hid_lo, int (&nb)[K], std::integer_sequence<int, B...>) {
  using S = HaloSlot<K, HWID>;
  ((nb[B] = lds_read1i<S::rel(B) * 4>(hid_lo)), ...);
}
template <int K, int HWID, int... B>
__device__ __forceinline__ void halo_depths(uint32_t hdp_lo, float (&ds)[K + 1], std::integer_sequence<int, B...>) {
  using S = HaloSlot<K, HWID>;
  ((ds[B] = lds_read1<S::rel(B) * 4>(hdp_lo)), ...);
  ds[K] = lds_read1<S::MAXOFF * 4>(hdp_lo);                          // the cell's own depth
}
// (the table is [H][HR] -- head-major: the 32 cells of a read then sit in consecutive dwords; as [HR][H] they were H dwords apart,
//  i.e. on 32 / H banks: a 4-way conflict on every one of the (K + 1) x heads-per-lane reads of phase A)
template <int H, int K, int HWID, int... B>
__device__ __forceinline__ void halo_alpha_src(uint32_t has_lo, float (&hs)[K + 1], std::integer_sequence<int, B...>) {
  using S = HaloSlot<K, HWID>;
  ((hs[B] = lds_read1<S::rel(B) * 4>(has_lo)), ...);
  hs[K] = lds_read1<S::MAXOFF * 4>(has_lo);
}

// MFMA phase of one slab: 8 groups of (2 k rows x NT tiles).  Group M covers k rows 8*(M/2) + 2*(M&1) + {0,1}
// (+ 4*hl, folded into the base address).  The W fragments of group M+1 are requested before the MFMAs of
// group M are issued, so their LDS latency hides under the matrix pipe.
// On gfx950 the f32 MFMA shares the SIMD's issue with everything else (tools/mfma_overlap_probe.hip), so every instruction
// beside the MFMAs costs matrix time: the W image therefore has its columns permuted (WTileGroup) so that ONE ds_read_b128 (or
// b64) brings the fragments of TG = 4 (or 2) tiles of a k row -- 32 LDS reads per slab and wave instead of 128.
template <int NT>
struct WTileGroup {      // tiles per LDS read: column 32 t + r of W^T sits at (t / TG) * 32 TG + r * TG + t % TG of the image row
  static constexpr int TG = NT % 4 == 0 ? 4 : NT % 2 == 0 ? 2 : 1;
};
template <int TG, int OFF>
__device__ __forceinline__ void lds_read_frags(float *dst, uint32_t addr) {
  if constexpr (TG == 4) {
    const f32x4 v = lds_read4<OFF>(addr);
    dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
  } else if constexpr (TG == 2) {
    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    f32x2_ v;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    dst[0] = v.x; dst[1] = v.y;
  } else {
    dst[0] = lds_read1<OFF>(addr);
  }
}
template <int NT, int NC, int M, int END = 8, bool ZC = false>   // ZC: the first k row starts the accumulators from an inline 0
struct MfmaGroups {
  static constexpr int ROW = 8 * (M / 2) + 2 * (M & 1);
  static constexpr int TG = WTileGroup<NT>::TG;
  __device__ static __forceinline__ void load(float (&wa)[NT], float (&wb)[NT], uint32_t wbuf0) {
    lload<0>(wa, wb, wbuf0);
  }
  template <int TH>
  __device__ static __forceinline__ void lload(float (&wa)[NT], float (&wb)[NT], uint32_t wbuf0) {
    if constexpr (TH < NT / TG) {
      lds_read_frags<TG, (ROW * NC + TH * 32 * TG) * 4>(wa + TH * TG, wbuf0);
      lds_read_frags<TG, ((ROW + 1) * NC + TH * 32 * TG) * 4>(wb + TH * TG, wbuf0);
      lload<TH + 1>(wa, wb, wbuf0);
    }
  }
  __device__ static __forceinline__ void run(f32x16 (&acc)[NT], const f32x4 (&g)[4], uint32_t wbuf0) {
    float wa[NT], wb[NT];
    load(wa, wb, wbuf0);
    step(acc, g, wbuf0, wa, wb);
  }
  __device__ static __forceinline__ void step(f32x16 (&acc)[NT], const f32x4 (&g)[4], uint32_t wbuf0, float (&wa)[NT],
                                             float (&wb)[NT]) {
    lds_reads_done();
    float na[NT], nb[NT];
    if constexpr (M + 1 < END) MfmaGroups<NT, NC, M + 1, END>::load(na, nb, wbuf0);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if constexpr (ZC) {             // the block's very first MFMAs: C = 0 as an inline constant -- no 16 NT v_mov to clear the accumulators
        const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[t], g[M / 2][2 * (M & 1)], z, 0, 0, 0);
      } else {
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[t], g[M / 2][2 * (M & 1)], acc[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[t], g[M / 2][2 * (M & 1) + 1], acc[t], 0, 0, 0);
    if constexpr (M + 1 < END) MfmaGroups<NT, NC, M + 1, END>::step(acc, g, wbuf0, na, nb);
  }
};

// ---- bf16x3 matrix path (opt-in): x = xh + xl, W = Wh + Wl (bf16 each), x W ~= xh Wh + xl Wh + xh Wl with float32
// accumulation on v_mfma_f32_32x32x16_bf16 -- 3 instructions of 32 cycles per 16 k instead of 8 x 64 cycles of
// v_mfma_f32_32x32x2_f32, and on the matrix pipe proper: unlike the f32 MFMA (which runs at the VALU rate and blocks
// its SIMD neighbour) it co-executes with the other workgroup's vector work.  Class logits move by ~6e-6
// (tests/study_bf16_split_accuracy.py); the exact-f32 path stays the default.
// fp16x3 is the same scheme with float16 parts on v_mfma_f32_32x32x16_f16: 11-bit parts instead of 8,
// so hi + lo carries 22 bits and the logits land within ~5e-7 of the float64 forward (float32 itself: 2e-7) -- but only
// while |x| stays below 65 504 (float16 range); larger activations would saturate.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <typename V8, typename E>
__device__ __forceinline__ void split_lp(const f32x4 &ga, const f32x4 &gb, V8 &hi, V8 &lo) {
  const float v[8] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w};
#pragma unroll
  for (int i = 0; i < 8; ++i) hi[i] = (E)v[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) lo[i] = (E)(v[i] - (float)hi[i]);
}
__device__ __forceinline__ bf16x8 to_bf16x8(const f32x4 &ga, const f32x4 &gb) {
  const float v[8] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w};
  bf16x8 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = (__bf16)v[i];       // v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN
  return r;
}
__device__ __forceinline__ f32x16 mfma_lp(const bf16x8 &a, const bf16x8 &b, const f32x16 &c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_lp(const f16x8 &a, const f16x8 &b, const f32x16 &c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// one 16-k half-chunk: tile t's W fragments (hi, lo) sit at wh + (2t + part) KiB (+ lane * 16, folded into wh);
// the fragments of tile t + 1 are requested before tile t's three MFMAs are issued
template <int NT, int T, typename V8>
struct SplitTiles {
  __device__ static __forceinline__ void step(f32x16 (&acc)[NT], const V8 &xh, const V8 &xl, uint32_t wh, f32x4 ah, f32x4 al) {
    lds_reads_done();
    f32x4 nh = ah, nl = al;
    if constexpr (T + 1 < NT) { nh = lds_read4<(2 * (T + 1)) * 1024>(wh); nl = lds_read4<(2 * (T + 1) + 1) * 1024>(wh); }
    const V8 wh8 = __builtin_bit_cast(V8, ah), wl8 = __builtin_bit_cast(V8, al);
    acc[T] = mfma_lp(wl8, xh, acc[T]);
    acc[T] = mfma_lp(wh8, xl, acc[T]);
    acc[T] = mfma_lp(wh8, xh, acc[T]);
    if constexpr (T + 1 < NT) SplitTiles<NT, T + 1, V8>::step(acc, xh, xl, wh, nh, nl);
  }
  __device__ static __forceinline__ void run(f32x16 (&acc)[NT], const V8 &xh, const V8 &xl, uint32_t wh) {
    static_assert(T == 0, "entry point");
    step(acc, xh, xl, wh, lds_read4<0>(wh), lds_read4<1024>(wh));
  }
};

// plain bf16 (SP = 3): one MFMA per tile and 16 k; tile t's fragment sits at wh + t KiB (hi-only image).
// The fragments of up to FOUR tiles are requested together and waited for once: a bf16 MFMA is 8 passes, far shorter than an LDS
// round trip, so the one-ahead scheme the f32 path uses (fragment t + 1 under the MFMA of tile t) left every one of the 16 reads
// of a slab exposed -- ~20 % of the 256 -> 256 instance's lifetime.  With NT = 8 the second batch's reads pass under the first
// batch's MFMAs.  (16 more live registers in a phase that has them to spare: the aggregation's operands are dead by then.)
template <int OFF>
__device__ __forceinline__ f32x4 lds_read4_at(uint32_t addr) { return lds_read4<OFF>(addr); }
template <int NT, int T0>
struct Bf16Tiles {
  static constexpr int NB = NT - T0 < 4 ? NT - T0 : 4;
  __device__ static __forceinline__ void load(f32x4 (&w)[4], uint32_t wh) {
    if constexpr (NB > 0) w[0] = lds_read4_at<(T0 + 0) * 1024>(wh);
    if constexpr (NB > 1) w[1] = lds_read4_at<(T0 + 1) * 1024>(wh);
    if constexpr (NB > 2) w[2] = lds_read4_at<(T0 + 2) * 1024>(wh);
    if constexpr (NB > 3) w[3] = lds_read4_at<(T0 + 3) * 1024>(wh);
  }
  __device__ static __forceinline__ void step(f32x16 (&acc)[NT], const bf16x8 &x, uint32_t wh, f32x4 (&w)[4]) {
    lds_reads_done();
    f32x4 nw[4];
    if constexpr (T0 + NB < NT) Bf16Tiles<NT, T0 + NB>::load(nw, wh);
#pragma unroll
    for (int i = 0; i < NB; ++i) acc[T0 + i] = mfma_lp(__builtin_bit_cast(bf16x8, w[i]), x, acc[T0 + i]);
    if constexpr (T0 + NB < NT) Bf16Tiles<NT, T0 + NB>::step(acc, x, wh, nw);
  }
  __device__ static __forceinline__ void run(f32x16 (&acc)[NT], const bf16x8 &x, uint32_t wh) {
    static_assert(T0 == 0, "entry point");
    f32x4 w[4];
    load(w, wh);
    step(acc, x, wh, w);
  }
};

template <int N>
__device__ __forceinline__ void wait_vm_lgkm() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// One HALF of a slab's W chunk (16 k rows of every column) is BYTES contiguous bytes of the weight image: 16 x NC f32
// (exact and split images share that byte geometry) or 16 x NC bf16 (hi-only image, SP = 3) = NQ pieces of 1 KiB
// dealt over the 4 waves.
template <int NT, int SP>
struct WHalf {
  static constexpr int BYTES = SP == 3 ? NT * 1024 : 2 * NT * 1024;
  static constexpr int NQ = BYTES / 1024;
  static constexpr int PER_WAVE = NQ / 4;                 // floor: a wait that counts on this many is conservative
};
template <int NT, int SP>
__device__ __forceinline__ void stage_w_half(const float *Wt, float *wbuf, int half_index, int wave, int lane) {
  using G = WHalf<NT, SP>;
  const char *src = reinterpret_cast<const char *>(Wt) + (int64_t)half_index * G::BYTES;
  float *dst = wbuf + (half_index & 1) * (G::BYTES / 4);
#pragma unroll
  for (int j = 0; j < (G::NQ + 3) / 4; ++j) {
    const int q = j * 4 + wave;
    if (q < G::NQ)
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(src + q * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void *)(dst + q * 256), 16, 0, 0);
  }
}

constexpr int FT_H = 8;                                  // fused kernel: 8 x 16 cell blocks

template <int K>
struct FusedGeom {                                       // halo geometry of one block
  static constexpr int R = K == 16 ? 2 : 1;              // halo radius in cells
  static constexpr int HW = TILE_W + 2 * R;              // halo row width  (18 / 20)
  static constexpr int HR = (FT_H + 2 * R) * HW;         // halo rows       (180 / 240)
};

// ---- bf16 storage path: the neighbourhood sum itself runs on the matrix pipe.
// A wave's 32 cells (two block rows) only touch the halo rows of a WINDOW of 2 + 2R halo lines = 120 (k = 16) / 72 (k = 4, 8)
// consecutive rows of the slab image.  With alpha[cell][window row] as a dense bf16 matrix (zero outside the stencil),
//     agg[ch][cell] = sum_row X[row][ch] * alpha[cell][row]      is      NKB x v_mfma_f32_32x32x16_bf16
// per 32-channel slab: A = X^T read straight from the [row][32 ch] slab image by ds_read_b64_tr_b16 (the hardware transpose), B =
// the dense alpha rows (one ds_read_b128 per 16 window rows).  The result tile has the cell on the lane and the channels in the
// 16 registers -- exactly what the next-layer GEMM wants as ITS B operand (k order 8(j>>2) + 4h + (j&3): the W image is packed
// to match, model_pack.hip pack_bf16_image_accop).  Per slab and wave that replaces 17 x 3 LDS reads, 272 unpack and 144 FMA
// instructions by 16 + 8 LDS reads and 8 MFMAs; 87 % of those MFMAs' products are zeros, on a pipe with 16x the vector rate.
// alpha is rounded to bf16 for this (the activations it multiplies already are).  Rows without a node hold zeros and 0 x 0 = 0;
// non-finite activations (which valid, finite depths cannot produce) would spread over the window instead of the stencil.
template <int K>
struct AggWindow {
  using G = FusedGeom<K>;
  static constexpr int ROWS = (2 + 2 * G::R) * G::HW;     // 120 / 72
  static constexpr int NKB = (ROWS + 15) / 16;            // 8 / 5 MFMAs per slab
  static constexpr int PAD = NKB * 16;                    // 128 / 80
  // Dense alpha matrix of a wave: [32 cells][PITCH bytes] of bf16, window row wp of cell r at r * PITCH + 2 wp.  PITCH is an ODD
  // multiple of 16 bytes >= 2 ROWS: 16 consecutive cell rows then start in 16 different 16-byte bank groups, so the B-operand reads
  // (16 lanes x ds_read_b128 = one row chunk each) are conflict-free without an XOR swizzle, and the matrix is 240 / 176 bytes
  // wide instead of 256 (k = 16: 30 KB per workgroup instead of 32 -- what lets the narrow instances fit three per CU).
  // k = 16: the last MFMA's upper k-half (window rows 120..127 = bytes 240..255) lies beyond the pitch: those lanes feed zeros.
  static constexpr int PITCH = K == 16 ? 240 : 176;
  static constexpr bool TAIL_BEYOND_PITCH = PAD * 2 > PITCH;
  static constexpr int LAST = TAIL_BEYOND_PITCH ? ROWS : PAD;   // rows the last wave's window may use
  static_assert(PITCH % 32 == 16 && PITCH >= 2 * ROWS && (PAD - 8) * 2 <= PITCH, "odd multiple of 16 B that holds every window row");
  __device__ static __forceinline__ int base(int wave) {  // first halo row of the wave's window (the last wave's is pulled inside)
    // k <= 8: pulled back so that all PAD rows the MFMAs read are slab rows.  k = 16: the matrix is only ROWS wide (PITCH), so
    // the window starts at most at HR - ROWS; the last MFMA's A operand then reads 8 rows past the slab image -- the head of the W
    // buffer, always finite bf16 weights -- against B rows that are zero by construction (TAIL_BEYOND_PITCH).
    const int b = wave * 2 * G::HW;
    return b < G::HR - LAST ? b : G::HR - LAST;
  }
  static_assert((2 * G::HW) % 4 == 0 && (G::HR - LAST) % 4 == 0, "windows start on a 4-row boundary (uniform swizzle per read)");
};
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
template <int OFF>
__device__ __forceinline__ u32x2 lds_read_tr(uint32_t addr) {      // EXEC must be all ones
  u32x2 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  const bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, v);
}
// one batch of NB window blocks: reads first (A: two transposed reads, B: one row read per block), then the MFMAs.
// TAILZ: block 7's upper k-half lies beyond the dense matrix's pitch (AggWindow): lanes with hl = 1 feed zeros there.
template <int KB0, int NB, bool ZERO, bool TAILZ>
__device__ __forceinline__ void agg_blocks(f32x16 &d, uint32_t tr0, uint32_t tr1, uint32_t bq, int hl) {
  u32x2 a0[NB], a1[NB];
  u32x4 b[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    // (the immediate must be a literal: spell the blocks out)
    if (KB0 + i == 0) { a0[i] = lds_read_tr<0>(tr0); a1[i] = lds_read_tr<0>(tr1); b[i] = lds_read4u<0>(bq); }
    if (KB0 + i == 1) { a0[i] = lds_read_tr<1024>(tr0); a1[i] = lds_read_tr<1024>(tr1); b[i] = lds_read4u<32>(bq); }
    if (KB0 + i == 2) { a0[i] = lds_read_tr<2048>(tr0); a1[i] = lds_read_tr<2048>(tr1); b[i] = lds_read4u<64>(bq); }
    if (KB0 + i == 3) { a0[i] = lds_read_tr<3072>(tr0); a1[i] = lds_read_tr<3072>(tr1); b[i] = lds_read4u<96>(bq); }
    if (KB0 + i == 4) { a0[i] = lds_read_tr<4096>(tr0); a1[i] = lds_read_tr<4096>(tr1); b[i] = lds_read4u<128>(bq); }
    if (KB0 + i == 5) { a0[i] = lds_read_tr<5120>(tr0); a1[i] = lds_read_tr<5120>(tr1); b[i] = lds_read4u<160>(bq); }
    if (KB0 + i == 6) { a0[i] = lds_read_tr<6144>(tr0); a1[i] = lds_read_tr<6144>(tr1); b[i] = lds_read4u<192>(bq); }
    if (KB0 + i == 7) { a0[i] = lds_read_tr<7168>(tr0); a1[i] = lds_read_tr<7168>(tr1); b[i] = lds_read4u<224>(bq); }
  }
  lds_reads_done();
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    if (TAILZ && KB0 + i == 7) {
      const u32x4 z4 = {0u, 0u, 0u, 0u};
      if (hl) b[i] = z4;
    }
    const u32x4 av = {a0[i].x, a0[i].y, a1[i].x, a1[i].y};
    const bf16x8 A = __builtin_bit_cast(bf16x8, av), B = __builtin_bit_cast(bf16x8, b[i]);
    if (ZERO && i == 0) {
      const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B, z, 0, 0, 0);
    } else {
      d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B, d, 0, 0, 0);
    }
  }
}

template <int HC, int C, int K, int NT, int EPI, int SP, int LF = 0>
struct FusedLds {       // LDS budget of one workgroup, in floats (kernel and launcher agree through this)
  static constexpr int H = HC / C, NC = NT * 32, HR = FusedGeom<K>::HR;
  static constexpr int XB = SP == 3 ? 2 : 4;             // bytes per stored activation
  // LF ("light form", exact GAT instances with a narrow next stage; context option fused_light_form): the slab image holds HALF a
  // slab -- [HR][16 channels], 64-byte rows -- and the coefficient table the heads of one head PAIR, so that four workgroups fit a CU
  // (<= 40 KB of LDS and <= 128 VGPRs each).  See the half-step loop in the kernel.
  static constexpr bool HS = LF != 0;
  static_assert(!HS || (SP == 0 && K <= 8 && NT <= 3), "light form: exact f32, halo of one cell, narrow next stage");
  static constexpr int AW = HS && H > 2 ? 2 : H;         // heads whose coefficients the table holds at a time
  static_assert(H <= 2 * AW, "light form: two head pairs at the most");
  static constexpr int SLAB1 = HS ? HR * 16 : HR * 32 * XB / 4;   // one slab image: [HR][32 channels] (HS: [HR][16])
  // bf16 storage, 256 -> 256 instance (two workgroups per CU whatever the LDS, its 128 accumulator registers decide): the slab image is
  // DOUBLE-BUFFERED -- slab s + 1 is requested as soon as slab s is visible, a whole slab period ahead, instead of after slab s has
  // been gathered (half a period ahead: with no matrix work to hide under, ~17 % of that instance's lifetime was spent waiting
  // for it).  Paid for by aliasing (alpha_src table and halo ids inside the alpha region, att vectors parked in the free buffer).
  // RING selects how the bf16 256 -> 256 instance spends its spare LDS (it runs two workgroups per CU whatever the LDS: 128 accumulator
  // registers decide).  1: two slab images (above).  2: two FULL 32-row W chunks instead of two 16-row halves -- chunk s + 1 is
  // requested a whole slab ahead and nothing is restaged inside a slab, so a slab needs TWO barriers instead of five.  The per-phase
  // timers had put ~30 % of that instance's lifetime at barriers, and doubling the slab's lead (RING 1) did not shorten them: the
  // time is barrier skew between the four waves (each shares its SIMD with a wave of the other workgroup), not DMA latency.
  // Measured (configs[2], 128 tiles): RING 0 10.29 ms of fused time per step, RING 1 10.06-10.19, RING 2 10.03 (two spilled registers at
  // k = 16) -- within noise of each other: neither the slab's lead nor the number of barriers is what bounds this instance.
  // RING 1 ships (no spills).
  static constexpr int RING = SP == 3 && NT == 8 && EPI == EPI_NEXT ? 1 : 0;
  static constexpr bool DBUF = RING == 1, WDB = RING == 2;
  static constexpr int SLAB = DBUF ? 2 * SLAB1 : SLAB1;
  static constexpr int WBUF = (WDB ? 4 : 2) * WHalf<NT, SP>::BYTES / 4;
  // the epilogue's four wave-private 32 x 36 store patches reuse slab (+ wbuf)
  static constexpr int PATCH_PAD = EPI == EPI_NEXT && SLAB + WBUF < 4 * 32 * TILED_PITCH ? 4 * 32 * TILED_PITCH - SLAB - WBUF : 0;
  static constexpr int HEADW = 96 + 6 * 32 + 8;          // heads: first-layer biases | second-layer rows (<= 4 classes + 2) | their biases
  // bf16 storage path, two space savers (so that its narrow instances fit three workgroups per CU):
  //  * the halo's alpha_src table (phase A only) lives in the dense-alpha region, which is first written after phase A;
  //  * the heads' small weight table (final epilogue only) is parked in the slab region once the last slab has been gathered.
  //  * DBUF: the halo ids live there as well (the epilogue takes its row ids from the lanes' own registers), and the next layer's
  //    att vectors are DMA'd into the free slab buffer during the last slab.
  static constexpr bool HAS_IN_ALPHA = SP == 3, HEADW_LATE = SP == 3 && EPI == EPI_HEADS, HID_IN_ALPHA = DBUF || WDB, ATT_LATE = DBUF || WDB;
  // (floats) past the four store patches, which start at image A, and past the 8 rows (128 floats) image A's last MFMA over-reads
  // (WDB: at the same offset from the slab image, i.e. inside W chunk buffer 0, which the last -- odd -- slab does not use)
  static constexpr int ATT_OFF = SLAB1 + 128 > 4 * 32 * TILED_PITCH ? SLAB1 + 128 : 4 * 32 * TILED_PITCH;
  static constexpr int RA = HAS_IN_ALPHA ? 0 : HR * (H + 1), RB = 2 * HC + (EPI == EPI_NEXT ? (ATT_LATE ? 0 : 2 * NC) : HEADW_LATE ? 0 : HEADW);
  static constexpr int RSZ = RA > RB ? RA : RB;
  // ODD pitch (in dwords): the gather reads one coefficient per cell with ds_read_b32, whose 32-lane groups bank on (a / 4) mod 32 --
  // with the round-2 pitch of 36 dwords the 32 cells of a group fell on 8 banks (4-way conflict on every coefficient read)
  static constexpr int APITCH = (AW * (K + 1)) | 1;
  // attention coefficients: [128 cells][APITCH] f32 (sparse, every head); bf16 storage path: the CURRENT head's coefficients as
  // four wave-private dense [32 cells][window rows] bf16 matrices (the aggregation's MFMA B operand) -- see AggWindow
  static constexpr int ALPHA = SP == 3 ? 4 * 32 * AggWindow<K>::PITCH / 4 : 128 * APITCH;
  static_assert(!HAS_IN_ALPHA || HR * (H + 1) + (HID_IN_ALPHA ? HR : 0) <= ALPHA, "the alpha_src and depth tables (and the halo ids) fit the dense-alpha region");
  static_assert(!DBUF || (4 * 32 * TILED_PITCH <= ATT_OFF && ATT_OFF + 2 * NC <= SLAB), "patches | att vectors share the slab region");
  static_assert(!WDB || (4 * 32 * TILED_PITCH <= ATT_OFF && ATT_OFF + 2 * NC <= SLAB + WBUF / 2), "patches | att vectors fit slab + W chunk buffer 0");
  static_assert(!HEADW_LATE || HEADW <= SLAB, "the heads' weight table fits the slab region");
  static_assert(SP != 3 || !AggWindow<K>::TAIL_BEYOND_PITCH || WBUF * 4 >= 8 * 64, "the 8 rows read past the slab image stay inside the W buffer");
  // (HID_IN_ALPHA: the epilogue's row ids come from a compact [128 cells] table instead of the halo table)
  static constexpr int PRE = SLAB + WBUF + PATCH_PAD + RSZ + (HID_IN_ALPHA ? 128 : HR) + 4;
  static constexpr int ALIGN = (4 - PRE % 4) % 4;        // the dense matrices start on a 16-byte boundary
  static constexpr int FLOATS = PRE + ALIGN + ALPHA;
  // (exact-f32 k = 16 heads instance: phase A holds 48 edge terms + 17 alpha_src + 17 logits next to twelve 64-bit slab bases --
  //  more than the 170 registers a third workgroup leaves (46 spills, and a spill reload shares vmcnt with the slab DMAs): two
  //  workgroups per CU.  The bf16 instance has half the slab pieces and stays at three: measured 1.08 ms against 1.27 ms at two.)
  static constexpr bool WIDE_PHASE_A = K == 16 && EPI == EPI_HEADS && SP == 0;
  static constexpr int PER_CU = HS && FLOATS * 4 * 4 <= 160 * 1024 ? 4 : FLOATS * 4 * 3 <= 160 * 1024 && NT <= 3 && !WIDE_PHASE_A ? 3 : FLOATS * 4 * 2 <= 160 * 1024 ? 2 : 1;
};

// AGG (exact path, EPI_NEXT only): what phase A puts into the coefficient table, and what the epilogue does with the product --
//   0  GATConv: softmax attention; epilogue = next layer's attention dots (the kernel this file is about)
//   1  GCNConv: coefficient dinv[i] dinv[j] (self: dinv[i]^2), dinv = (in-degree + 1)^-1/2 read where GAT reads alpha_src
//   2  SAGEConv (mean): TWO virtual heads over the SAME C source channels -- head 0 = 1 / count on every in-edge, head 1 = the node
//      itself -- so the GEMM sees [mean_j x_j | x_i] against the stacked [lin_l ; lin_r] weight
//   3  GINConv (eps = 0): 1 on every in-edge, 1 on the node itself (2 with an explicit self loop)
// and for 1 .. 3 the layer is aggregate -> GEMM -> per-column scale / shift (+ ReLU) -> h_{l+1}: the post-op vectors ride where the
// attention vectors ride (a.att_src = scale, a.att_dst = shift), the pre-GEMM scale / shift are the identity.  (GCN: A (X W) = (A X) W.)
template <int HC, int C, int K, int NT, int EPI, int SP = 0, int AGG = 0, int LF = 0>     // SP: 0 exact f32, 1 bf16x3, 2 fp16x3, 3 bf16 storage + MFMA; LF: FusedLds
// (register budget: what the LDS footprint allows per CU -- except the plain backbones on the 16-slot stencil, whose aggregate
//  coefficients (GCN's degree products / GIN's ones over 17 sources, in full float32) do not fit three workgroups' 168 registers:
//  they spilled 140 bytes per lane there and run two per CU instead)
__global__ __launch_bounds__(256, (AGG != 0 && K == 16 ? 2 : FusedLds<HC, C, K, NT, EPI, SP, LF>::PER_CU)) void gat_layer_fused_kernel(FusedArgs a) {
  static_assert(LF == 0 || AGG == 0, "light form: GAT instances");
  static_assert(AGG == 0 || (SP == 0 && EPI == EPI_NEXT), "the plain backbones run on the exact path, layer form");
  static_assert(AGG != 2 || HC == 2 * C, "GraphSAGE: two virtual heads");
  constexpr int SRCW = AGG == 2 ? C : HC;                // channels of a SOURCE row (GraphSAGE: both virtual heads read the same C)
  // (narrow next stages leave registers and LDS for a third workgroup per CU)
  // 4 waves.  Wave w: cells 32w..32w+31 of the block (two tile rows).  Lane (r, hl): node r of the group, k-half hl.
  constexpr int NTH = 256;
  constexpr int H = HC / C;
  constexpr int NC = NT * 32;
  constexpr int NSLAB = HC / 32, SPH = C / 32;
  // the exact path's gather with the next source's LDS reads in flight under the current source's accumulation: where the second
  // register set fits the instance's occupancy (256 -> 256: 252 of 256 VGPRs at two waves per SIMD; 256 -> 64: 150 of 168 at three;
  // the heads instances, k = 16 and the plain backbones would lose a resident workgroup to it)
  constexpr bool GATHER_PIPE = SP == 0 && K <= 8 && EPI == EPI_NEXT && AGG == 0;
  using Geo = FusedGeom<K>;
  using Lds = FusedLds<HC, C, K, NT, EPI, SP, LF>;
  constexpr bool HS = Lds::HS;                           // light form: half-slab image, half-steps (below)
  constexpr int HR = Geo::HR, HW_ = Geo::HW, RAD = Geo::R;
  constexpr int XB = Lds::XB;                            // bytes per stored activation
  constexpr int ROWB = HS ? 64 : 32 * XB;                // bytes of one halo row's (half-)slab (128 / 64)
  constexpr int CPR = ROWB / 16;                         // 16-byte chunks per row slab (8 / 4)
  using Off = StencilOffsets<K>;
  extern __shared__ __attribute__((aligned(128))) float lds[];
  float *slab = lds;                                   // [HR][32]  halo rows of the current slab, 16-B chunks XOR-swizzled
  float *wbuf = slab + Lds::SLAB;                      // W_{l+1} rows of the current slab: two 16-row halves
  // DBUF: two slab images.  EVEN slabs use the upper one (B, next to the W buffer), odd slabs the lower one (A): the k = 16
  // window's last MFMA reads 8 rows past its image (AggWindow) -- past B that is the W buffer's head, past A it is B's head,
  // which by then holds rows of an even slab (landed, or being replaced by the next one's): finite bf16 either way.
  constexpr bool DBUF = Lds::DBUF, WDB = Lds::WDB;
  constexpr int SLAB1B = Lds::SLAB1 * 4;                 // bytes of one slab image
  // Region R is time-shared: alpha_src of the halo rows during phase A, then (from the first slab barrier on)
  // the folded scale / shift table and, behind it, the next layer's att_src | att_dst for the epilogue.
  constexpr int RSZ = Lds::RSZ, APITCH = Lds::APITCH;
  float *rreg = wbuf + Lds::WBUF + Lds::PATCH_PAD;
  float *scsh = rreg;                                  // [2][HC]   folded scale / shift (slab loop)
  float *attr = Lds::HEADW_LATE ? slab : Lds::ATT_LATE ? slab + Lds::ATT_OFF : rreg + 2 * HC;   // [2][NC] att_src | att_dst (epilogue, EPI_NEXT) / heads' weight table
  int *cid = reinterpret_cast<int *>(rreg + RSZ);      // [128] node id of each block cell (HID_IN_ALPHA only)
  int *minid = cid + (Lds::HID_IN_ALPHA ? 128 : HR);   // [4]
  float *alx = reinterpret_cast<float *>(minid + 4) + Lds::ALIGN;   // [128][APITCH]  alpha[cell][head][K+1]; bf16 path: dense (AggWindow)
  float *has = Lds::HAS_IN_ALPHA ? alx : rreg;         // [H][HR]   (phase A; bf16 path: inside the not yet written dense-alpha region)
  float *hdp = has + HR * H;                           // [HR]      depth of the halo rows' nodes (phase A: depth differences)
  int *hid = Lds::HID_IN_ALPHA ? reinterpret_cast<int *>(alx + HR * (H + 1)) : reinterpret_cast<int *>(rreg + RSZ);   // [HR]

#if BGNN_DIAG
  unsigned long long t_sum[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long t_prev = a.stamps ? __builtin_amdgcn_s_memtime() : 0;
  const unsigned long long t_clk0 = t_prev, t_real0 = a.stamps ? __builtin_amdgcn_s_memrealtime() : 0;   // in-kernel clock probe
#endif
  const BlockPos pos = decode_block<FT_H>(a.tb);
  // (static s_setprio by SIMD wave slot or by workgroup parity, so that co-resident waves differ: measured, 1-3 % slower)
  const int tid = threadIdx.x, lane = tid & 63;
  // the wave index as a SCALAR: LDS-DMA destinations (M0) and the "does this wave move piece q" tests then stay on the scalar
  // unit instead of costing a v_readfirstlane / exec-mask sequence per DMA in the slab loop
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hl = lane >> 5;
  const int cell = wave * 32 + r;                      // block-local cell of this lane
  const int tr = cell / TILE_W, tc = cell % TILE_W;
  const int self_idx = (tr + RAD) * HW_ + tc + RAD;

  // W rows of slab 0 depend on nothing: first in the VM queue.
  stage_w_half<NT, SP>(a.Wt, wbuf, 0, wave, lane);
  stage_w_half<NT, SP>(a.Wt, wbuf, 1, wave, lane);
  // WDB: W chunk c (both halves, 2 x BYTES contiguous bytes of the image) lives in chunk buffer c & 1; chunk 1 can go now as well
  auto stage_w_chunk = [&](int c) {
    using G = WHalf<NT, SP>;
    const char *src = reinterpret_cast<const char *>(a.Wt) + (int64_t)c * 2 * G::BYTES;
    float *dst = wbuf + (c & 1) * (2 * G::BYTES / 4);
#pragma unroll
    for (int j = 0; j < (2 * G::NQ + 3) / 4; ++j) {
      const int q = j * 4 + wave;
      if (q < 2 * G::NQ)
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(src + q * 1024 + lane * 16),
                                         (__attribute__((address_space(3))) void *)(dst + q * 256), 16, 0, 0);
    }
  };
  if constexpr (WDB) { if (NSLAB > 1) stage_w_chunk(1); }

  // Prologue loads, two dependent rounds with everything of a round in flight together:
  //   round 1: node id of this thread's halo row (HR <= NTH: one row per thread), of this lane's own cell, and of
  //            the <= NPIECE halo rows whose chunks this thread moves by DMA (CPR lanes share a row);
  //   -> slab 0's DMA is issued straight from those registers (no LDS round trip, no barrier);
  //   round 2: alpha_src and node depth of the halo row; the own node's K slopes, alpha_dst (heads hl, hl + 2, ...) and the tile's edge lengths
  //            -- consumed in phase A, so their latency hides behind the halo bookkeeping.
  static_assert(HR <= NTH, "one halo row per thread");
  constexpr int NHL = (H + 1) / 2;                      // heads per lane
  constexpr int NPIECE = (HR * CPR + NTH - 1) / NTH;
  static_assert((NPIECE - 2) * NTH + NTH - 64 < HR * CPR, "every wave moves NPIECE or NPIECE - 1 pieces");
  // Round 1 is ONE round: every load is unconditional (coordinates clamped into the tile, validity applied to the value
  // afterwards), so nothing is exec-masked, no branch separates the loads and the compiler keeps all of them in flight behind
  // a single wait.  (With `if (inside) id = node_id[..]` per load, hipcc waited for the halo row's id, then for the own cell's,
  // then for the DMA rows': three dependent trips to L2 before round 2 could start.)
  // (Integer work is kept short on purpose: on the exact path this wave's SIMD partners stream f32 MFMAs, and every VALU
  //  instruction of the prologue waits for a gap between two of them -- ~50-100 cycles each by the per-phase timers.  Cell indices
  //  are 32-bit (a batch has < 2^30 cells), the node-id table is addressed base + 32-bit offset, the DMA pieces' halo rows advance
  //  by a constant step instead of being divided out, and validity is one unsigned compare per coordinate.)
  const uint32_t cbase = (uint32_t)pos.cell_off, uw = (uint32_t)pos.w, uh = (uint32_t)pos.h;
  const int h1 = pos.h - 1, w1 = pos.w - 1;
  auto cell_index = [&](int gr, int gc) -> uint32_t {    // clamped into the tile: always a readable cell
    const int r_ = max(0, min(gr, h1)), c_ = max(0, min(gc, w1));
    return cbase + __umul24((uint32_t)r_, uw) + (uint32_t)c_;      // (r, w < 2^14)
  };
  // node id of a cell: table base (uniform) + 32-bit BYTE offset -> the load's saddr + voffset form, no 64-bit address arithmetic
  auto node_at = [&](uint32_t cell) -> int {
    return *reinterpret_cast<const int *>(reinterpret_cast<const char *>(a.node_id) + (cell << 2));
  };
  auto in_tile = [&](int gr, int gc) -> bool { return (uint32_t)gr < uh && (uint32_t)gc < uw; };
  const int hr_t = tid / HW_, hc_t = tid - hr_t * HW_;
  const int gr_h = pos.r0 + hr_t - RAD, gc_h = pos.c0 + hc_t - RAD;
  const int gr_m = pos.r0 + tr, gc_m = pos.c0 + tc;
  const int raw_h = node_at(cell_index(gr_h, gc_h));
  const uint32_t cell_m = cell_index(gr_m, gc_m);
  const int raw_m = node_at(cell_m);
  // whose edge lengths: the block's tile, or (canvas walk) the grid this cell belongs to -- a canvas array read beside the ids
  int tile_m = pos.tile;
  if (a.tile_of_cell) {                                 // (only cells that hold a node have an entry: the table is not cleared)
    const int t_ = *reinterpret_cast<const int *>(reinterpret_cast<const char *>(a.tile_of_cell) + (cell_m << 2));
    tile_m = raw_m >= 0 ? t_ : 0;
  }
  // DMA piece p moves chunk (p * NTH + tid) % CPR of halo row (p * NTH + tid) / CPR: the row advances by NTH / CPR per piece
  static_assert(NTH % CPR == 0, "pieces advance by whole halo rows");
  constexpr int RSTEP = NTH / CPR, RSTEP_R = RSTEP / HW_, RSTEP_C = RSTEP % HW_;
  int drow[NPIECE], prow_r[NPIECE], prow_c[NPIECE];
  {
    const int row0 = tid / CPR;
    int pr = row0 / HW_, pc = row0 - pr * HW_;
#pragma unroll
    for (int p = 0; p < NPIECE; ++p) {
      prow_r[p] = pr; prow_c[p] = pc;
      drow[p] = node_at(cell_index(pos.r0 + pr - RAD, pos.c0 + pc - RAD));
      pr += RSTEP_R; pc += RSTEP_C;
      if (pc >= HW_) { pc -= HW_; pr += 1; }
    }
  }
  constexpr int NSC = (HC + NTH - 1) / NTH;
  float scv[NSC], shv[NSC];                             // folded scale / shift: to LDS once phase A has released R
#pragma unroll
  for (int i = 0; i < NSC; ++i) {
    const int c = tid + i * NTH;
    scv[i] = c < HC ? a.scale[c] : 0.0f; shv[i] = c < HC ? a.shift[c] : 0.0f;
  }
  float vpre[NHL][3];
#pragma unroll
  for (int i = 0; i < NHL; ++i) {
    const int hh = hl + i * 2;
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      // (light form, one head: only the hl = 0 lanes run phase A's arithmetic -- the edge vector stays a uniform value in scalar
      //  registers instead of three vector registers held from here to phase A)
      if constexpr (HS && H == 1) vpre[i][f] = a.V[f];
      else vpre[i][f] = (AGG == 0 && hh < H) ? a.V[hh * 3 + f] : 0.0f;
    }
  }
  // (heads: the small second-stage weight table -- 296 floats, packed on the host in its LDS layout -- is one LDS-DMA piece
  //  issued where its LDS region falls free, see stage_head_table below.  Read straight from global memory in the final epilogue
  //  it was 28 dependent float4 loads per lane behind runtime class tests, 41 % of that instance's lifetime; held in registers
  //  from the prologue on -- round 2 -- it cost three exec-masked loads with a vmcnt(0) each and, at k = 16, spills whose
  //  reloads share vmcnt with the slab DMAs.)
  BGNN_STAMP(9)    // block decode, address arithmetic, round 1 requested
  // validity (ids < 0 in the table encode invalid cells)
  int hid_v = (tid < HR && in_tile(gr_h, gc_h) && raw_h >= 0) ? raw_h : -1;
  int my_pre = (!DBG(32) && in_tile(gr_m, gc_m)) ? raw_m : -1;
#pragma unroll
  for (int p = 0; p < NPIECE; ++p) {
    // (measured with ids COMPUTED instead of loaded, all-valid tiles: 0.3 % (exact) / 2 % (bf16) -- the id round is already hidden)
    const bool row_ok = (p + 1) * NTH <= HR * CPR || prow_r[p] < FT_H + 2 * RAD;       // rows past the halo: last piece only
    if (!(row_ok && in_tile(pos.r0 + prow_r[p] - RAD, pos.c0 + prow_c[p] - RAD))) drow[p] = -1;
  }
#if BGNN_DIAG
  if (a.stamps) asm volatile("" ::"v"(hid_v), "v"(my_pre), "v"(drow[0]));
#endif
  BGNN_STAMP(10)   // round 1 arrived
  if (a.cell_map) {                  // canvas walk (wave-uniform test): blocks that hold only gutter / free space leave here
    // (not __syncthreads_or: its library reduction brings 256 bytes of static LDS in front of the dynamic region)
    const bool wave_any = __builtin_amdgcn_ballot_w64(my_pre >= 0) != 0;
    if (lane == 0) minid[wave] = wave_any ? 1 : 0;
    __syncthreads();
    if ((minid[0] | minid[1] | minid[2] | minid[3]) == 0) {
      __builtin_amdgcn_s_waitcnt(0);   // the W DMAs land in this WG's LDS: drain them before the LDS can be handed on
      return;
    }
  }
  // Round 2, complete BEFORE slab 0's DMA is queued (hipcc only ever waits vmcnt(0) with an LDS-DMA in flight): alpha_src of
  // this thread's halo row (and its node's depth); the own node's slopes and alpha_dst (heads hl, hl + 2, ...).  Unconditional as well:
  // rows without a node read row 0 and are masked afterwards.
  // Edge attributes come COMPACT (graph_build.hip, FeatureArgs): the K slopes of the own node, the node depths of the halo rows
  // (depth difference = one float32 subtraction, as the feature kernel takes it) and the three edge lengths of the tile -- a third
  // of the bytes and registers of the [K][3] block this round used to load (k = 16: 64 + 4 + 16 instead of 192 bytes per node).
  float eraw[K], adv[NHL], hasv[H], hdep;
  float4 tdist;
  if constexpr (AGG != 0) {                              // plain backbones: no edge terms; GCN reads dinv of the halo row
    const uint64_t hrow = (uint32_t)(hid_v >= 0 ? hid_v : 0);
#pragma unroll
    for (int hh = 0; hh < H; ++hh) hasv[hh] = 0.0f;
    if constexpr (AGG == 1) hasv[0] = a.asd[hrow];
#pragma unroll
    for (int i = 0; i < K; ++i) eraw[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < NHL; ++i) adv[i] = 0.0f;
    hdep = 0.0f; tdist = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    const uint64_t hrow = (uint32_t)(hid_v >= 0 ? hid_v : 0), mrow = (uint32_t)(my_pre >= 0 ? my_pre : 0);   // (zero-extended: one v_mad_u64_u32 each)
    hdep = a.node_depth[hrow];
    tdist = a.tile_dist[tile_m];
    if constexpr (H % 4 == 0) {
#pragma unroll
      for (int q = 0; q < H / 4; ++q) {
        const float4 v4 = *reinterpret_cast<const float4 *>(a.asd + hrow * 2 * H + 4 * q);
        hasv[4 * q] = v4.x; hasv[4 * q + 1] = v4.y; hasv[4 * q + 2] = v4.z; hasv[4 * q + 3] = v4.w;
      }
    } else {
#pragma unroll
      for (int hh = 0; hh < H; ++hh) hasv[hh] = a.asd[hrow * 2 * H + hh];
    }
    const float4 *ep = reinterpret_cast<const float4 *>(a.slope + mrow * K);
#pragma unroll
    for (int i = 0; i < K / 4; ++i) {
      const float4 q = ep[i];
      eraw[4 * i] = q.x; eraw[4 * i + 1] = q.y; eraw[4 * i + 2] = q.z; eraw[4 * i + 3] = q.w;
    }
#pragma unroll
    for (int i = 0; i < NHL; ++i) {
      const int hh = hl + i * 2;
      adv[i] = hh < H ? a.asd[mrow * 2 * H + H + hh] : 0.0f;
    }
  }
  // Halo rows go global -> LDS by LDS-DMA.  A wave-instruction writes 64 x 16 B linearly = 64 / CPR rows x ROWB bytes;
  // bank spreading is an XOR swizzle on the SOURCE side: LDS chunk p of a row holds channel chunk p ^ swz(row), with
  // swz(row) = ((row % HW) >> 1) & 7 for 128-byte rows -- by the row's COLUMN in the halo, see below -- and (row >> 2) & 3 for
  // 64-byte rows.  Each thread always moves the same <= NPIECE (row, chunk) pairs, so their source
  // offsets (32 bits, relative to the smallest node id this WAVE touches) are computed once.
  // 128-byte rows: a ds_read_b128 is served in four groups of 16 lanes, and a group is NOT 16 consecutive lanes: {0-3, 12-15,
  // 20-27}, {4-11, 16-19, 28-31} (+32): eight cells of the wave's first block row and the COMPLEMENTARY eight columns of its second.
  // A slot (parity of the row, chunk ^ swz) is free of conflicts when the 16 rows of a group differ in (row & 1, swz): with the
  // swizzle taken from the halo column, hc >> 1, any 16 distinct columns do (HW is even, so the parity follows the column too).
  // Round 2's (row >> 1) & 7 shifted the second block row's slots by one against the first: two 2-way conflicts per group, i.e.
  // every gather read took twice its LDS cycles (SQ_LDS_BANK_CONFLICT: 37-47 % of the exact instances' LDS-active cycles).
  static_assert(HW_ % 2 == 0, "row parity follows the halo column");
  // Light form, 64-byte rows of f32 (four chunks; row * 64 mod 256 puts halo row `row` into quarter row & 3 of a 256-byte bank line):
  // swz = bit 2 of the halo column | parity of the halo line << 1.  The eight columns a group takes from one line are two runs of
  // four, twelve apart: a run covers the four quarters, the two runs differ in bit 2 of the column, and the group's other line
  // differs in parity -- 16 distinct (quarter, chunk) slots.
  auto swz = [](int row) {
    return HS ? (((row % HW_) >> 2) & 1) | (((row / HW_) & 1) << 1) : XB == 4 ? ((row % HW_) >> 1) & 7 : (row >> 2) & 3;
  };
  // Per piece ONE 64-bit source base for the whole block (a single 32 x 32 -> 64-bit multiply-add off the table's base; an earlier
  // version kept 32-bit offsets relative to the smallest id of the wave, which cost a six-step wave reduction per block): rows
  // without a node read the context's zero page, which holds more than NSLAB * ROWB zero bytes, so that they can advance by ROWB
  // per slab exactly like real rows (no per-slab select) and EVERY wave issues a fixed number of slab pieces (npc): the counted
  // waits below can leave exactly the next slab in flight.
  static_assert(NSLAB * ROWB <= 4096, "the zero page covers a whole block's worth of slab offsets");
  const char *xbase = reinterpret_cast<const char *>(a.xw);
  const char *zp = reinterpret_cast<const char *>(a.zero_page);
  const char *dbase[NPIECE];
  // light form, one-head sources (the heads launch): the bases as 32-bit offsets in 16-byte units (64-channel rows: 2^28 nodes), ~0 = the
  // zero page, widened at each request -- three registers less across the whole block, which is what keeps this instance free of
  // scratch at 128 registers; a few vector instructions per half-step, and it has four of them
  constexpr bool DB32 = HS && H == 1;
  uint32_t doff[NPIECE];
  {
    const int cc = tid % CPR;
#pragma unroll
    for (int p = 0; p < NPIECE; ++p) {
      const int row = prow_r[p] * HW_ + prow_c[p];
      const int c = cc ^ (HS ? ((prow_c[p] >> 2) & 1) | ((prow_r[p] & 1) << 1) : swz(row));   // (HS: swz(row) without the division)
      dbase[p] = drow[p] >= 0 ? xbase + ((uint64_t)(uint32_t)drow[p] * (uint32_t)(SRCW * XB) + (uint32_t)(c * 16)) : zp;
      doff[p] = drow[p] >= 0 ? (uint32_t)drow[p] * (uint32_t)(SRCW * XB / 16) + (uint32_t)c : ~0u;
    }
  }
  int npc = 0;
#pragma unroll
  for (int p = 0; p < NPIECE; ++p) npc += (p * NTH + wave * 64 < HR * CPR) ? 1 : 0;
  // heads: the weight table -> LDS, one DMA piece (waves 0 and 1: 64 + 10 lanes x 16 B)
  static_assert(Lds::HEADW % 4 == 0 && Lds::HEADW <= 128 * 4, "the heads' table is at most two wave pieces");
  auto stage_head_table = [&]() {
    if constexpr (EPI == EPI_HEADS) {
      if (wave < 2 && (wave * 64 + lane) * 4 < Lds::HEADW)
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a.hd_tab + (wave * 64 + lane) * 4),
                                         (__attribute__((address_space(3))) void *)(attr + wave * 256), 16, 0, 0);
    }
  };
  auto issue_slab = [&](int s) {
    const int sb = (AGG == 2 ? s % SPH : s) * ROWB;    // wave-uniform (GraphSAGE: the second virtual head re-reads the same channels; HS: s counts half-slabs)
#pragma unroll
    for (int p = 0; p < NPIECE; ++p) {
      if ((p + 1) * NTH <= HR * CPR || p * NTH + tid < HR * CPR) {        // (only the last piece is partial: compile-time true before)
        uint32_t dof = doff[p];
        if constexpr (DB32) asm volatile("" : "+v"(dof));    // (opaque: the widened base must not be hoisted back out of the loop)
        const char *src = DB32 ? (dof != ~0u ? xbase + ((uint64_t)dof << 4) : zp) : dbase[p];
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(src + sb),
                                         (__attribute__((address_space(3))) void *)(slab + (DBUF && !(s & 1) ? Lds::SLAB1 : 0) + (p * NTH + wave * 64) * 4), 16, 0, 0);
      }
    }
  };
  // Round 2's values go to the halo tables first -- hipcc waits vmcnt(0) for them, which must not include slab 0's DMA -- and
  // only then is slab 0 requested: it is in flight during the whole of phase A, whose LDS reads are asm (no compiler wait).
  if (tid < HR) {
    hid[tid] = hid_v;
#pragma unroll
    for (int hh = 0; hh < H; ++hh) has[hh * HR + tid] = hid_v >= 0 ? hasv[hh] : (AGG == 0 ? -__builtin_inff() : 0.0f);   // (-inf: an absent source drops out of the softmax)
    hdp[tid] = hid_v >= 0 ? hdep : 0.0f;
  }
  if (Lds::HID_IN_ALPHA && hl == 0) cid[cell] = my_pre < 0 ? -1 : my_pre;
  {   // (phase A's register operands are complete as well before the DMA is queued: no wait behind it later)
    // (the table writes above sit under `tid < HR`: a wave that skips them has not waited yet -- touch every round-2 register)
    float sink = 0.0f;
#pragma unroll
    for (int i = 0; i < NHL; ++i) sink += adv[i];
#pragma unroll
    for (int i = 0; i < K; ++i) sink += eraw[i];
#pragma unroll
    for (int hh = 0; hh < H; ++hh) sink += hasv[hh];
    sink += hdep + tdist.x + tdist.y + tdist.z;
    asm volatile("" ::"v"(sink));
  }
  BGNN_STAMP(11)   // round 2 arrived, halo tables written
  issue_slab(0);
  BGNN_STAMP(0)   // slab 0 issued
  // (raw barrier, not __syncthreads(): its fence would wait vmcnt(0), i.e. for slab 0's DMA, which phase A is meant to pass under)
  wait_lgkm0();
  __builtin_amdgcn_s_barrier();
  BGNN_STAMP(1)   // round 2, halo tables in LDS

  // ---- phase A: attention coefficients -> LDS.  The two lanes that share a cell take the heads round-robin.
  uint32_t apk[NHL][(K + 2) / 2];                       // bf16 storage path: this lane's heads, (K + 1) coefficients as bf16 pairs
#pragma unroll
  for (int i = 0; i < NHL; ++i)
#pragma unroll
    for (int b = 0; b < (K + 2) / 2; ++b) apk[i][b] = 0u;
  static_assert(!HS || NHL <= 2, "light form: a lane holds at most one head beside the one in the table");
  float keep[K + 1];                                    // light form, H > 2: the coefficients of this lane's second head
#pragma unroll
  for (int b = 0; b <= K; ++b) keep[b] = 0.0f;
  {
    const uint32_t hid0 = lds_addr(hid), has0 = lds_addr(has);
    // (k = 16 bf16 heads instance, which runs at its register limit: the cell's halo index is recomputed from the thread id here --
    //  kept, it is spilled across the id rounds, and its reload would wait vmcnt(0), i.e. for slab 0's DMA, in front of phase A)
    int self_a = self_idx;
    if constexpr (K == 16 && EPI == EPI_HEADS && SP == 3) {
      int t2 = threadIdx.x;
      asm volatile("" : "+v"(t2));
      const int c2 = (t2 & 31) | (t2 >> 6) << 5;                 // wave * 32 + (lane & 31)
      self_a = (c2 / TILE_W + RAD) * HW_ + c2 % TILE_W + RAD;
    }
    int my = lds_read1i<0>(hid0 + (uint32_t)self_a * 4u);
    lds_reads_done();
    if (DBG(32)) my = -1;
    // the cell's node ids of the stencil sources once, alpha_src per head; then the head-independent edge terms once and the
    // lane's heads -- both at once, as packed f32 halves, when it owns two (gat_tile_common.h)
    float part[NHL][K + 1];
    if (my < 0) {                                       // (zeros only where they are needed: no live range across the arithmetic)
#pragma unroll
      for (int i = 0; i < NHL; ++i)
#pragma unroll
        for (int b = 0; b <= K; ++b) part[i][b] = 0.0f;
    } else {
      using S = HaloSlot<K, HW_>;
      int nb[K];
      float hs[NHL][K + 1];
      halo_ids<K, HW_>(hid0 + (uint32_t)(self_a - S::MAXOFF) * 4u, nb, std::make_integer_sequence<int, K>{});
      if constexpr (AGG != 0) {
        // plain backbones: the coefficient of in-edge b (b = K: the node itself), in the order the gather sums them -- the order of
        // neighbor_reduce.hip (slots ascending, self last)
        static_assert(AGG == 0 || NHL == 1, "one (virtual) head per lane");
        if constexpr (AGG == 1) halo_alpha_src<1, K, HW_>(has0 + (uint32_t)(self_a - S::MAXOFF) * 4u, hs[0], std::make_integer_sequence<int, K>{});
        lds_reads_done();
        int cnt = a.self_loops ? 1 : 0;
#pragma unroll
        for (int b = 0; b < K; ++b) cnt += nb[b] >= 0 ? 1 : 0;
        const float inv = 1.0f / (float)(cnt > 0 ? cnt : 1);
#pragma unroll
        for (int b = 0; b <= K; ++b) {
          const bool self = b == K, on = self || nb[b < K ? b : 0] >= 0;
          float c;
          if constexpr (AGG == 1) c = self ? hs[0][K] * hs[0][K] : (on ? hs[0][b] * hs[0][K] : 0.0f);      // dinv[j] * dinv[i]
          else if constexpr (AGG == 2) c = hl == 0 ? ((self ? a.self_loops != 0 : on) ? inv : 0.0f) : (self ? 1.0f : 0.0f);
          else c = self ? (a.self_loops ? 2.0f : 1.0f) : (on ? 1.0f : 0.0f);
          part[0][b] = c;
        }
      } else {
#pragma unroll
      for (int i = 0; i < NHL; ++i) {
        const int hh = hl + i * 2 < H ? hl + i * 2 : 0;
        halo_alpha_src<H, K, HW_>(has0 + (uint32_t)(hh * HR + self_a - S::MAXOFF) * 4u, hs[i], std::make_integer_sequence<int, K>{});
      }
      float dsrc[K + 1];
      halo_depths<K, HW_>(lds_addr(hdp) + (uint32_t)(self_a - S::MAXOFF) * 4u, dsrc, std::make_integer_sequence<int, K>{});
      lds_reads_done();
      EdgeTerms<K> et;
      edge_terms_compact<K>(nb, eraw, dsrc, tdist.x, tdist.y, tdist.z, et);
      if constexpr (NHL == 2 && H % 2 == 0 && H >= 4) {
        attention_head_pair<K, false>(et, hs[0], hs[1], adv[0], adv[1], vpre[0], vpre[1], part[0], part[1]);
      } else {
#pragma unroll
        for (int i = 0; i < NHL; ++i)
          if (hl + i * 2 < H) attention_head<K, false>(et, hs[i], adv[i], vpre[i], part[i]);
      }
      }   // AGG == 0
    }
#pragma unroll
    for (int i = 0; i < NHL; ++i) {
      const int hh = hl + i * 2;
      if (hh < H) {
        if constexpr (SP == 3) {      // kept in registers as bf16 pairs until this head's slabs come up (densified there)
#pragma unroll
          for (int b = 0; b <= K; b += 2) apk[i][b / 2] = pack_bf16x2(part[i][b], b + 1 <= K ? part[i][b + 1] : 0.0f);
        } else if (HS && H > Lds::AW && i > 0) {
          // light form: the table holds one head pair; the lane's second head waits in registers until the first pair's last
          // slab has been gathered (the rows of a cell are written and read by the cell's own two lanes only)
#pragma unroll
          for (int b = 0; b <= K; ++b) keep[b] = part[i][b];
        } else {
          // (asm writes: with slab 0's DMA in flight hipcc would wait vmcnt(0) in front of a visible ds_write too)
          lds_write_coefficients<K>(lds_addr(alx + cell * APITCH + (HS && H > Lds::AW ? hl : hh) * (K + 1)), part[i], std::make_integer_sequence<int, K + 1>{});
        }
      }
    }
    // (consumers wait at the barrier at the top of the slab loop)
  }

  BGNN_STAMP(2)   // phase A
  f32x16 acc[NT];
  if constexpr (SP != 0 || BGNN_DIAG) {                  // (exact path: slab 0's first MFMAs start from an inline zero instead)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
  }

  const uint32_t slab0 = lds_addr(slab);
  const uint32_t wbuf0 = lds_addr(wbuf + 4 * hl * NC + r * WTileGroup<NT>::TG);   // (column-permuted image: WTileGroup)
  // chunk (16 B) ownership of lane (r, hl) inside a 32-channel slab: exact-f32 path channel chunks 2j + hl (k = 8j + 4hl + i
  // of f32 k-step j); 16-bit MFMA paths channels 8hl..8hl+7 for k-step 0 and 16+8hl.. for k-step 1 (k = 16 step + 8hl + i)
  // (bf16 storage: the aggregation MFMA's result tile hands lane (r, hl) the exact path's channels, 8j + 4hl + i)
  constexpr bool F32_CHUNKS = SP == 0 || SP == 3;
  constexpr uint32_t CX1 = F32_CHUNKS ? 32 : 16, CX2 = 64, CX3 = F32_CHUNKS ? 96 : 80;
  const uint32_t scsh0 = lds_addr(scsh) + (F32_CHUNKS ? hl * 16 : hl * 32);
  const uint32_t wsp0 = lds_addr(wbuf) + lane * 16;      // 16-bit MFMA paths: A fragments are stored in lane order
  const uint32_t alx0 = lds_addr(alx + cell * APITCH);
  constexpr uint32_t WHALF = WHalf<NT, SP>::BYTES;
  // bf16 storage: addresses of the aggregation's operands (AggWindow)
  using Win = AggWindow<K>;
  const int wbase = Win::base(wave);
  const uint32_t dn0 = lds_addr(alx) + wave * (32 * Win::PITCH);                // this wave's dense alpha [32 cells][PITCH bytes] bf16
  const uint32_t bq0 = dn0 + r * Win::PITCH + hl * 16;                         // window rows 16 kb + 8 hl ..: + 32 kb (immediate)
  uint32_t tr0 = 0, tr1 = 0;
  if constexpr (SP == 3) {
    // transposed read: lane 4q + p of a 16-lane group addresses row q, channels 4p..4p+3 of the group's 16 channels
    const int grp = lane >> 4, q = (lane >> 2) & 3, p4 = lane & 3, cb = grp & 1;
    const int row0 = wbase + 8 * hl + q;                  // + 4 part + 16 kb
    const int c = 2 * cb + (p4 >> 1);
    tr0 = slab0 + row0 * 64 + ((c ^ ((row0 >> 2) & 3)) << 4) + 8 * (p4 & 1);
    tr1 = slab0 + (row0 + 4) * 64 + ((c ^ (((row0 + 4) >> 2) & 3)) << 4) + 8 * (p4 & 1);
  }

  // ---- slabs.  Lane (r, hl) gathers exactly the 16 values it feeds to the MFMA as B operand -- no LDS round trip, no
  // lane exchange.
  if constexpr (HS) {
    // ---- light form: a slab is two HALF-STEPS over one [HR][16 channels] image.  Half-step hs = 2 s + h:
    //   wait for everything | barrier A | DMA W half hs + 1 | gather channels 16 h .. 16 h + 15 of slab s + BN/ReLU (g[2h], g[2h+1]) |
    //   barrier B | DMA half-slab hs + 1 | 16 x NT MFMAs out of W half h
    // Barrier A publishes half-slab hs and W half hs (requested a whole half-step ago) and says that every wave has left the MFMAs of
    // half-step hs - 1, whose W half the DMA behind it refills; barrier B says that every wave has gathered, so the image can be
    // refilled under the MFMAs.  The same four barriers per slab as the full-slab form, no counted wait (a wave never has more in
    // flight than what the next barrier A needs), and per accumulator the same k rows in the same order: bit-identical.
    // The image is single because two of them would not fit four workgroups per CU; what the shorter lead exposes, the fourth
    // workgroup is there to cover.
    constexpr int AW = Lds::AW;
    auto half_step = [&](auto hc_, int s, uint32_t ap, f32x4 (&g)[4]) {
      constexpr int h = decltype(hc_)::value;
      const int hs = 2 * s + h;
      wait_vm_lgkm<0>();
      __builtin_amdgcn_s_barrier();                     // A
      if (h == 0 && s == 0) {
        // phase A is over on every wave: R changes hands (as in the full-slab form below)
#pragma unroll
        for (int i = 0; i < NSC; ++i) {
          const int c = tid + i * NTH;
          if (c < HC) { scsh[c] = scv[i]; scsh[HC + c] = shv[i]; }
        }
        if constexpr (EPI == EPI_HEADS) stage_head_table();
        if (EPI == EPI_NEXT && wave < 2 && lane * 4 < NC)
          __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>((wave == 0 ? a.att_src : a.att_dst) + lane * 4),
                                           (__attribute__((address_space(3))) void *)(attr + wave * NC), 16, 0, 0);
        wait_lgkm0();
        __builtin_amdgcn_s_barrier();                   // scale / shift visible
      }
      if (hs >= 1 && hs + 1 < 2 * NSLAB) stage_w_half<NT, SP>(a.Wt, wbuf, hs + 1, wave, lane);   // (halves 0 and 1 went in the prologue)
      constexpr int jA = 2 * h, jB = 2 * h + 1;
      g[jA] = (f32x4){0.f, 0.f, 0.f, 0.f}; g[jB] = (f32x4){0.f, 0.f, 0.f, 0.f};
      auto row_addr = [&](int b) -> uint32_t {          // chunk hl of source b's row; chunk 2 + hl sits at (addr ^ 32)
        const int dr_ = b < K ? Off::dr[b < K ? b : 0] : 0, dc_ = b < K ? Off::dc[b < K ? b : 0] : 0;
        const int nidx = self_idx - dr_ * HW_ - dc_;
        const int hcol = tc + RAD - dc_, hline = tr + RAD - dr_;
        return slab0 + nidx * 64 + ((((((hcol >> 2) & 1) | ((hline & 1) << 1))) ^ hl) << 4);
      };
      if constexpr (GATHER_PIPE) {
        f32x4 xb[2][2];
        float al[2];
        auto issue = [&](int b, int q) {
          const uint32_t rb = row_addr(b);
          al[q] = lds_read1<0>(ap + 4 * b);
          xb[q][0] = lds_read4<0>(rb); xb[q][1] = lds_read4<0>(rb ^ 32);
        };
        issue(0, 0);
#pragma unroll
        for (int b = 0; b <= K; ++b) {
          const int q = b & 1;
          if (b + 1 <= K) { issue(b + 1, q ^ 1); lds_reads_wait<3>(); } else lds_reads_done();
          g[jA] += al[q] * xb[q][0]; g[jB] += al[q] * xb[q][1];
        }
      } else {
#pragma unroll
        for (int b = 0; b <= K; ++b) {
          const uint32_t rb = row_addr(b);
          const float alpha = lds_read1<0>(ap + 4 * b);
          const f32x4 x0 = lds_read4<0>(rb), x1 = lds_read4<0>(rb ^ 32);
          lds_reads_done();
          g[jA] += alpha * x0; g[jB] += alpha * x1;
        }
      }
      {
        const uint32_t cp = scsh0 + s * 128 + h * 64;
        const f32x4 sc0 = lds_read4<0>(cp), sc1 = lds_read4<32>(cp), sh0 = lds_read4<HC * 4>(cp), sh1 = lds_read4<HC * 4 + 32>(cp);
        lds_reads_done();
        g[jA] = g[jA] * sc0 + sh0;
        g[jB] = g[jB] * sc1 + sh1;
        if (a.relu) {
#pragma unroll
          for (int j = jA; j <= jB; ++j) {
            asm("v_max_f32 %0, 0, %0" : "+v"(g[j].x)); asm("v_max_f32 %0, 0, %0" : "+v"(g[j].y));
            asm("v_max_f32 %0, 0, %0" : "+v"(g[j].z)); asm("v_max_f32 %0, 0, %0" : "+v"(g[j].w));
          }
        }
      }
      wait_lgkm0();
      __builtin_amdgcn_s_barrier();                     // B
      if (hs + 1 < 2 * NSLAB) issue_slab(hs + 1);
      if constexpr (h == 0) {
        if (s == 0) MfmaGroups<NT, NC, 0, 4, true>::run(acc, g, wbuf0);
        else MfmaGroups<NT, NC, 0, 4>::run(acc, g, wbuf0);
      } else {
        MfmaGroups<NT, NC, 4, 8>::run(acc, g, wbuf0);
      }
    };
#pragma unroll 1
    for (int s = 0; s < NSLAB; ++s) {
      const int hd = s / SPH;
      if constexpr (H > AW) {
        // the second head pair's coefficients take the first pair's place: this wave's reads of them are complete (every gather ends
        // with lgkmcnt(0)) and nobody else reads a cell's rows
        if (s == AW * SPH && hl + AW < H)
          lds_write_coefficients<K>(alx0 + hl * ((K + 1) * 4), keep, std::make_integer_sequence<int, K + 1>{});
      }
      const uint32_t ap = alx0 + (H > AW ? (hd & (AW - 1)) : hd) * ((K + 1) * 4);
      f32x4 g[4];
      half_step(std::integral_constant<int, 0>{}, s, ap, g);
      half_step(std::integral_constant<int, 1>{}, s, ap, g);
    }
  } else {
#pragma unroll 1
    for (int s = 0; s < NSLAB; ++s) {
      const uint32_t slabs = slab0;
      // VM queue order per wave: [slab s] [W rows 0-15 of slab s: WA] [W rows 16-31: WB] [slab s+1] [WA s+1] ...
      // WA / WB are WH pieces per wave each (unconditional); slab pieces are exec-masked, so they are never
      // counted on: a wait that must cover a W half uses only the W pieces issued after it.
      constexpr int WH = WHalf<NT, SP>::PER_WAVE;
      // When the pieces of a half do not divide evenly over the 4 waves, waves below NQ % 4 issue one more: their counted
      // waits leave one more operation in flight per half (a wave-uniform branch between two immediates).  With the floor
      // alone a narrow next stage (NQ = 2 or 3) waited for EVERYTHING at each of these points, the next slab included.
      constexpr int WREM = WHalf<NT, SP>::NQ % 4;
      const bool wextra = wave < WREM;
      // bf16 storage: a new head's coefficients become the wave's dense [32 cells][window rows] matrix.  Wave-private, and LDS
      // operations of one wave complete in order: no barrier, the aggregation's reads simply follow the writes.  Head 0 is
      // written after slab 0's first barrier (until then the region holds the alpha_src table phase A reads on every wave).
      auto densify = [&](int hd) {
        // The matrix is cleared ONCE: a cell's K + 1 window positions depend on its place in the block only, so every later head
        // overwrites exactly the entries head 0 wrote (absent sources with a zero coefficient) -- 8 x ds_write_b128 per head less.
        if (hd == 0) {
          const u32x4 z4 = {0u, 0u, 0u, 0u};
          constexpr int DB = 32 * Win::PITCH;
#pragma unroll
          for (int i = 0; i < (DB + 1023) / 1024; ++i)
            if ((i + 1) * 1024 <= DB || lane * 16 + i * 1024 < DB)
              asm volatile("ds_write_b128 %0, %1" ::"v"(dn0 + lane * 16 + i * 1024), "v"(z4) : "memory");
        }
        if (hl == (hd & 1)) {
          const int wself = self_idx - wbase;
          const uint32_t rowb = dn0 + r * Win::PITCH;
#pragma unroll
          for (int b = 0; b <= K; ++b) {
            const int off = b < K ? Off::dr[b < K ? b : 0] * HW_ + Off::dc[b < K ? b : 0] : 0;
            const int wp = wself - off;
            const uint32_t ad = rowb + (uint32_t)wp * 2u;
            const uint32_t v = NHL > 1 && (hd >> 1) ? apk[NHL > 1 ? 1 : 0][b / 2] : apk[0][b / 2];
            if (b & 1) asm volatile("ds_write_b16_d16_hi %0, %1" ::"v"(ad), "v"(v) : "memory");
            else asm volatile("ds_write_b16 %0, %1" ::"v"(ad), "v"(v) : "memory");
          }
        }
      };
      if constexpr (SP == 3) {
        if (s % SPH == 0 && s > 0) densify(s / SPH);
      }
      if (s == 0 || WDB) wait_vm_lgkm<0>();             // (slab 0 was queued BEHIND its W rows: wait for everything; WDB: slab s and
                                                        //  W chunk s are all this wave has in flight)
      else if (WREM && wextra) wait_vm_lgkm<2 * (WH + 1)>();
      else wait_vm_lgkm<2 * WH>();
      __builtin_amdgcn_s_barrier();                     // slab s visible to every wave
      if (s == 0) {
        // phase A is over on every wave: R changes hands.  Scale / shift from the registers they waited in; the
        // next layer's att_src | att_dst by DMA (one more VM op behind WB(0) on waves 0/1: the counted waits below
        // only get more conservative).
#pragma unroll
        for (int i = 0; i < NSC; ++i) {
          const int c = tid + i * NTH;
          if (c < HC) { scsh[c] = scv[i]; scsh[HC + c] = shv[i]; }
        }
        if constexpr (SP == 3) densify(0);             // (every wave is past phase A: the alpha_src table is dead)
        if constexpr (EPI == EPI_HEADS && !Lds::HEADW_LATE) stage_head_table();   // (R is free; the last slab's full wait covers it)
        if (EPI == EPI_NEXT && !Lds::ATT_LATE && wave < 2 && lane * 4 < NC)
          __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>((wave == 0 ? a.att_src : a.att_dst) + lane * 4),
                                           (__attribute__((address_space(3))) void *)(attr + wave * NC), 16, 0, 0);
        wait_lgkm0();
        __builtin_amdgcn_s_barrier();                   // scale / shift visible
      }
      // DBUF: slab s is visible and the other image was released a slab ago -> request slab s + 1 NOW (VM queue: [WA s][WB s][slab s+1])
      if (DBUF && s + 1 < NSLAB && !DBG(4)) issue_slab(s + 1);
      // WDB: every wave is past the MFMAs of slab s - 1, so chunk buffer (s + 1) & 1 is free: request W chunk s + 1 (chunk 1 went in the prologue)
      if constexpr (WDB) { if (s >= 1 && s + 1 < NSLAB && !DBG(8)) stage_w_chunk(s + 1); }
      if constexpr (Lds::ATT_LATE && WDB) {
        // last slab (odd: it multiplies out of chunk buffer 1): chunk buffer 0 takes the next layer's att_src | att_dst, past the store
        // patches' reach; the __syncthreads in front of the final epilogue waits for it
        static_assert(!WDB || (NSLAB % 2 == 0 && NC * 4 == 1024), "the last slab uses chunk buffer 1; one 1-KiB piece per vector");
        if (s + 1 == NSLAB && wave < 2)
          __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>((wave == 0 ? a.att_src : a.att_dst) + lane * 4),
                                           (__attribute__((address_space(3))) void *)(attr + wave * NC), 16, 0, 0);
      }
      if constexpr (Lds::ATT_LATE && DBUF) {
        // last slab: the free image (B: the last slab is odd) takes the next layer's att_src | att_dst.  EVERY wave issues one
        // piece (waves 2, 3 repeat 0, 1's) so that the counted wait below is the same on all of them.
        static_assert(!Lds::ATT_LATE || (NSLAB % 2 == 0 && NC * 4 == 1024), "the last slab uses image A; one 1-KiB piece per vector");
        if (s + 1 == NSLAB)
          __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(((wave & 1) == 0 ? a.att_src : a.att_dst) + lane * 4),
                                           (__attribute__((address_space(3))) void *)(attr + (wave & 1) * NC), 16, 0, 0);
      }
      BGNN_STAMP(3)   // wait for slab + barrier
      const uint32_t ap = alx0 + (s / SPH) * ((K + 1) * 4);
      f32x4 g[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (!DBG(1)) {
        auto nb_index = [&](int b) { return b >= K ? self_idx : self_idx - Off::dr[b < K ? b : 0] * HW_ - Off::dc[b < K ? b : 0]; };
        if constexpr (SP == 3) {
          // the neighbourhood sum on the matrix pipe (AggWindow): result register i = channel 8 (i >> 2) + 4 hl + (i & 3)
          f32x16 d;
          const uint32_t sbo = DBUF && !(s & 1) ? SLAB1B : 0;     // which slab image (wave-uniform)
          const uint32_t ta = tr0 + sbo, tb = tr1 + sbo;
          if constexpr (Win::NKB == 8) {
            agg_blocks<0, 4, true, false>(d, ta, tb, bq0, hl);
            agg_blocks<4, 4, false, Win::TAIL_BEYOND_PITCH>(d, ta, tb, bq0, hl);
          } else {
            static_assert(Win::NKB == 5, "window blocks");
            agg_blocks<0, 3, true, false>(d, ta, tb, bq0, hl);
            agg_blocks<3, 2, false, false>(d, ta, tb, bq0, hl);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) g[j] = (f32x4){d[4 * j], d[4 * j + 1], d[4 * j + 2], d[4 * j + 3]};
        } else {
          // 128-byte rows of f32: slot of channel chunk hl of that row; chunk 2j + hl sits at (slot ^ (j << 5)).
          if constexpr (GATHER_PIPE) {
            // source b + 1's five reads are in flight while source b is accumulated (two register sets; LDS operations return in
            // order, so "all but the five youngest" is source b).  The nine LDS round trips of a slab -- ~300-500 cycles each with the
            // other workgroup's W-fragment reads on the same LDS -- were serial: 2.35 ms of the 24.8 ms fused step by the phase
            // ablation.  Same additions in the same order: bit-identical.  Fused step 24.63 -> 24.25 ms (A/B on one box).
            f32x4 xb[2][4];
            float al[2];
            auto issue = [&](int b, int q) {
              const int nidx = nb_index(b);
              const int hcol = tc + RAD - (b < K ? Off::dc[b < K ? b : 0] : 0);
              const uint32_t rb = slabs + nidx * 128 + (((((hcol >> 1) & 7)) ^ (SP ? 2 * hl : hl)) << 4);
              al[q] = lds_read1<0>(ap + 4 * b);
              xb[q][0] = lds_read4<0>(rb); xb[q][1] = lds_read4<0>(rb ^ CX1); xb[q][2] = lds_read4<0>(rb ^ CX2); xb[q][3] = lds_read4<0>(rb ^ CX3);
            };
            issue(0, 0);
#pragma unroll
            for (int b = 0; b <= K; ++b) {
              const int q = b & 1;
              if (b + 1 <= K) { issue(b + 1, q ^ 1); lds_reads_wait<5>(); } else lds_reads_done();
#pragma unroll
              for (int j = 0; j < 4; ++j) g[j] += al[q] * xb[q][j];
            }
          } else {
#pragma unroll
          for (int b = 0; b <= K; ++b) {
            const int nidx = nb_index(b);
            const int hcol = tc + RAD - (b < K ? Off::dc[b < K ? b : 0] : 0);          // the source row's column in the halo
            const uint32_t rb = slabs + nidx * 128 + (((((hcol >> 1) & 7)) ^ (SP ? 2 * hl : hl)) << 4);
            f32x4 x[4];
            const float alpha = lds_read1<0>(ap + 4 * b);
            x[0] = lds_read4<0>(rb); x[1] = lds_read4<0>(rb ^ CX1); x[2] = lds_read4<0>(rb ^ CX2); x[3] = lds_read4<0>(rb ^ CX3);
            lds_reads_done();
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] += alpha * x[j];
          }
          }
        }
      }
      // layer epilogue: (+bias, BatchNorm) folded, ReLU -> h_{l+1}, in registers
      {
        const uint32_t cp = scsh0 + s * 128;
#pragma unroll
        for (int jp = 0; jp < 2; ++jp) {                // two chunks at a time (register budget)
          f32x4 sc0, sc1, sh0, sh1;
          if (jp == 0) { sc0 = lds_read4<0>(cp); sc1 = lds_read4<CX1>(cp); sh0 = lds_read4<HC * 4>(cp); sh1 = lds_read4<HC * 4 + CX1>(cp); }
          else { sc0 = lds_read4<CX2>(cp); sc1 = lds_read4<CX3>(cp); sh0 = lds_read4<HC * 4 + CX2>(cp); sh1 = lds_read4<HC * 4 + CX3>(cp); }
          lds_reads_done();
          g[2 * jp] = g[2 * jp] * sc0 + sh0;
          g[2 * jp + 1] = g[2 * jp + 1] * sc1 + sh1;
        }
        if (a.relu) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {               // one v_max_f32 each (the C select / fmax forms add a canonicalising one)
            asm("v_max_f32 %0, 0, %0" : "+v"(g[j].x)); asm("v_max_f32 %0, 0, %0" : "+v"(g[j].y));
            asm("v_max_f32 %0, 0, %0" : "+v"(g[j].z)); asm("v_max_f32 %0, 0, %0" : "+v"(g[j].w));
          }
        }
      }
      BGNN_STAMP(4)   // gather + layer epilogue
      if constexpr (WDB) {
        wait_lgkm0();                                   // (W chunk s landed with the wait at the top of the slab)
      } else if constexpr (DBUF) {
        // WA(s) landed; behind it in the queue: WB(s) and the npc pieces of slab s + 1 (last slab: the att piece)
        static_assert(!DBUF || WREM == 0, "DBUF instances deal the W pieces evenly");
        if (DBG(4)) wait_vm_lgkm<0>();
        else if (s + 1 == NSLAB) wait_vm_lgkm<WH + 1>();
        else if (npc == NPIECE) wait_vm_lgkm<WH + NPIECE>();
        else wait_vm_lgkm<WH + NPIECE - 1>();
      } else {
        if (WREM && wextra) wait_vm_lgkm<WH + 1>(); else wait_vm_lgkm<WH>();   // WA(s) landed (WB(s) may still fly)
      }
      __builtin_amdgcn_s_barrier();                     // every wave has finished reading slab s
      BGNN_STAMP(5)   // wait for WA + barrier
      if (!DBUF && s + 1 < NSLAB && !DBG(4)) issue_slab(s + 1);     // (WDB too: single slab image)
      if constexpr (Lds::HEADW_LATE) {
        // last slab gathered by every wave: its region now takes the heads' weight table; the two barriers between here and the
        // final epilogue publish it
        if (s + 1 == NSLAB) stage_head_table();       // (the vmcnt(0) after this slab's first MFMA half covers it)
      }
      // rank-16 update with W rows 0-15, then hand that half of the buffer to the next slab's DMA
      using LP8 = typename std::conditional<SP == 2, f16x8, bf16x8>::type;
      using LPE = typename std::conditional<SP == 2, _Float16, __bf16>::type;
      LP8 xh0, xl0, xh1, xl1;
      if constexpr (SP == 1 || SP == 2) { split_lp<LP8, LPE>(g[0], g[1], xh0, xl0); split_lp<LP8, LPE>(g[2], g[3], xh1, xl1); }
      if constexpr (SP == 3) { xh0 = to_bf16x8(g[0], g[1]); xh1 = to_bf16x8(g[2], g[3]); }
      if constexpr (WDB) {
        // both halves out of chunk buffer s & 1, nothing restaged, no barrier until the next slab's top
        const uint32_t cb = wsp0 + (uint32_t)(s & 1) * (2 * WHALF);
        if (!DBG(2)) {
          Bf16Tiles<NT, 0>::run(acc, xh0, cb);
          Bf16Tiles<NT, 0>::run(acc, xh1, cb + WHALF);
        }
        BGNN_STAMP(6)   // MFMA
        continue;
      }
      if (!DBG(2)) {
        if constexpr (SP == 3) Bf16Tiles<NT, 0>::run(acc, xh0, wsp0);
        else if constexpr (SP != 0) SplitTiles<NT, 0, LP8>::run(acc, xh0, xl0, wsp0);
        else if (s == 0 && !BGNN_DIAG) MfmaGroups<NT, NC, 0, 4, true>::run(acc, g, wbuf0);
        else MfmaGroups<NT, NC, 0, 4>::run(acc, g, wbuf0);
      }
      // WB(s) landed; the npc pieces of slab s+1 issued above stay in flight
      if (s + 1 < NSLAB && !DBG(4)) { if (npc == NPIECE) wait_vm_lgkm<NPIECE>(); else wait_vm_lgkm<NPIECE - 1>(); }
      else wait_vm_lgkm<0>();
      __builtin_amdgcn_s_barrier();                     // every wave is done with W rows 0-15
      if (s + 1 < NSLAB && !DBG(8)) stage_w_half<NT, SP>(a.Wt, wbuf, 2 * (s + 1), wave, lane);
      if (!DBG(2)) {
        if constexpr (SP == 3) Bf16Tiles<NT, 0>::run(acc, xh1, wsp0 + WHALF);
        else if constexpr (SP != 0) SplitTiles<NT, 0, LP8>::run(acc, xh1, xl1, wsp0 + WHALF);
        else MfmaGroups<NT, NC, 4, 8>::run(acc, g, wbuf0);
      }
      // (s_setprio 1 around the MFMA groups: measured, no change on either path)
      BGNN_STAMP(6)   // MFMA
      if (s + 1 < NSLAB) {
        wait_lgkm0();
        __builtin_amdgcn_s_barrier();                   // every wave is done with W rows 16-31
        if (!DBG(8)) stage_w_half<NT, SP>(a.Wt, wbuf, 2 * (s + 1) + 1, wave, lane);
        BGNN_STAMP(7)   // barrier + WB DMA issue
      }
    }
  }

  if constexpr (SP == 2) {                              // the float16 image holds W * 2^S (model_pack.hip pack_split): exact power-of-two rescale
    const float wi = a.w_inv;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][i] *= wi;
  }
  const float *attl = attr;                             // att_src | att_dst (DMA'd there during slab 0)
  // exact / split paths: the store patches below stay inside the slab region, which every wave left at the last slab's
  // second barrier -- a wave goes straight from its last MFMA into its own epilogue.  bf16 storage: the slab region is
  // smaller than the four patches, which then reach into wbuf: wait until every wave has read its last W fragments.
  if (EPI == EPI_NEXT && Lds::SLAB < 4 * 32 * TILED_PITCH) __syncthreads();
  if (!DBG(64)) {
    // (the cell's block coordinates from an OPAQUE copy of the lane id: hipcc otherwise shares `pos.r0 + tr` / `pos.c0 + tc` with the
    //  prologue's bounds tests, keeps both alive across the whole slab loop and, where an instance sits at its register limit --
    //  k = 16 at three workgroups per CU --, spills them)
    int lane_e = lane;
    asm volatile("" : "+v"(lane_e));
    const int cell_e = wave * 32 + (lane_e & 31);
    const int mr = cell_e / TILE_W, mc = cell_e % TILE_W;
    // (HID_IN_ALPHA: the halo id table was overwritten by the dense alpha matrices; the compact per-cell table is still there)
    const int id = Lds::HID_IN_ALPHA ? cid[cell_e] : hid[(mr + RAD) * HW_ + mc + RAD];
    if (EPI == EPI_NEXT) {
      // next layer's attention dots (its width per head is C as well): tile t belongs to head t / (C/32).
      // att_src / att_dst were staged into LDS: no global-load latency chain here.
      constexpr int TPH = C / 32, H2 = NT / TPH;
      static_assert(EPI != EPI_NEXT || NT % TPH == 0, "a wave's columns hold whole heads");
      typedef float f32x2 __attribute__((ext_vector_type(2)));
      f32x2 ps[H2 > 0 ? H2 : 1], pd[H2 > 0 ? H2 : 1];    // two-lane partial sums: the products go out as v_pk_fma_f32
#pragma unroll
      for (int hd = 0; hd < H2; ++hd) { ps[hd] = (f32x2){0.f, 0.f}; pd[hd] = (f32x2){0.f, 0.f}; }
      const uint32_t asl = lds_addr(attl + 4 * hl);
      // Row-per-lane stores (32 rows x 32 B per instruction) are store-issue bound; instead each 32x32 tile
      // is transposed through a wave-private LDS patch and written out as whole row segments: f32 128 bytes per row,
      // 8 rows per instruction; bf16 64 bytes per row, 16 rows per instruction.
      float *patch = slab + wave * (32 * TILED_PITCH);
      // bf16 storage: the patch holds TWO tiles side by side, already as bf16 -- [32 rows][128 B], 16-byte chunk c of row r at chunk
      // c ^ (r & 7), the two 8-byte halves of a chunk swapped on rows with bit 3 set: conflict-free for the ds_write_b64 (16 consecutive
      // lanes over 32 banks) and for the ds_read_b128 lane groups (MI355X_MICROARCH.md), half the LDS write bytes and read-backs of
      // the float32 patch, and whole 128-byte lines per stored row instead of two 64-byte halves.
      constexpr int LPR = 8;                            // lanes per stored row (f32: 128 B of one tile; bf16: 128 B of a tile pair)
      constexpr int NSTORE = 32 * LPR / 64;             // store instructions per tile (f32) / tile pair (bf16)
      static_assert(SP != 3 || EPI != EPI_NEXT || NT % 2 == 0, "bf16 tiles are stored in pairs");
      char *prow[NSTORE];                               // output row of patch row (lane / LPR) + (64 / LPR) k, column chunk lane % LPR
#pragma unroll
      for (int k = 0; k < NSTORE; ++k) {
        const int c = wave * 32 + lane / LPR + (64 / LPR) * k;
        const int rid = Lds::HID_IN_ALPHA ? cid[c] : hid[(c / TILE_W + RAD) * HW_ + c % TILE_W + RAD];
        prow[k] = (rid >= 0 ? reinterpret_cast<char *>(a.out) + (int64_t)rid * (NC * XB) : reinterpret_cast<char *>(a.dump)) + (lane % LPR) * 16;
      }
      // The att reads go through the asm path with an explicit wait per tile: left to the scheduler, all 2*NT*4
      // of them are hoisted above the stores, which -- next to 128 live accumulators -- spills them to scratch, and
      // every scratch reload then waits (vmcnt) for the stores in flight.
      static_assert(NC * 4 + 96 + 7 * 128 < 65536, "att offsets fit the ds_read immediate");
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        f32x4 s4[4], d4[4];
        s4[0] = lds_read4<0>(asl + t * 128); s4[1] = lds_read4<32>(asl + t * 128);
        s4[2] = lds_read4<64>(asl + t * 128); s4[3] = lds_read4<96>(asl + t * 128);
        d4[0] = lds_read4<NC * 4>(asl + t * 128); d4[1] = lds_read4<NC * 4 + 32>(asl + t * 128);
        d4[2] = lds_read4<NC * 4 + 64>(asl + t * 128); d4[3] = lds_read4<NC * 4 + 96>(asl + t * 128);
        lds_reads_done();
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float4 v = make_float4(acc[t][4 * g], acc[t][4 * g + 1], acc[t][4 * g + 2], acc[t][4 * g + 3]);
          if constexpr (AGG != 0) {
            // plain backbones: the layer's post-op on the product -- per-column scale (s4) / shift (d4), ReLU -- instead of attention dots
            v.x = v.x * s4[g].x + d4[g].x; v.y = v.y * s4[g].y + d4[g].y; v.z = v.z * s4[g].z + d4[g].z; v.w = v.w * s4[g].w + d4[g].w;
            if (a.relu2) { v.x = v.x > 0.f ? v.x : 0.f; v.y = v.y > 0.f ? v.y : 0.f; v.z = v.z > 0.f ? v.z : 0.f; v.w = v.w > 0.f ? v.w : 0.f; }
          } else {
            const f32x2 vlo = {v.x, v.y}, vhi = {v.z, v.w};
            ps[t / TPH] += vlo * (f32x2){s4[g].x, s4[g].y}; ps[t / TPH] += vhi * (f32x2){s4[g].z, s4[g].w};
            pd[t / TPH] += vlo * (f32x2){d4[g].x, d4[g].y}; pd[t / TPH] += vhi * (f32x2){d4[g].z, d4[g].w};
          }
          if constexpr (SP == 3) {
            typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
            bf16x4 o;
            o[0] = (__bf16)v.x; o[1] = (__bf16)v.y; o[2] = (__bf16)v.z; o[3] = (__bf16)v.w;
            char *pb = reinterpret_cast<char *>(patch) + r * 128 + ((hl ^ ((r >> 3) & 1)) << 3);
            *reinterpret_cast<bf16x4 *>(pb + ((((t & 1) * 4 + g) ^ (r & 7)) << 4)) = o;
          } else {
            *reinterpret_cast<float4 *>(patch + r * TILED_PITCH + 8 * g + 4 * hl) = v;
          }
        }
        asm volatile("" : "+v"(ps[t / TPH]), "+v"(pd[t / TPH]));   // the dots are due HERE (not sunk below the stores)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (SP == 3) {
          if (t & 1) {
#pragma unroll
            for (int k = 0; k < NSTORE; ++k) {          // row (lane >> 3) + 8 k: (row >> 3) & 1 == k & 1, the half swap is compile-time
              const int row = (lane >> 3) + 8 * k;
              uint4 q = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(patch) + row * 128 + (((lane & 7) ^ (row & 7)) << 4));
              if (k & 1) q = make_uint4(q.z, q.w, q.x, q.y);
              *reinterpret_cast<uint4 *>(prow[k] + (t - 1) * 64) = q;
            }
          }
        } else {
#pragma unroll
          for (int k = 0; k < NSTORE; ++k)
            *reinterpret_cast<float4 *>(prow[k] + t * 128) =
                *reinterpret_cast<const float4 *>(patch + ((lane >> 3) + 8 * k) * TILED_PITCH + (lane & 7) * 4);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // the node's [alpha_src (H2) | alpha_dst (H2)] row leaves as 16-byte (H2 = 4) / 8-byte (H2 = 1, 2) pieces instead of 2 H2 scalar
      // stores that each touched 32 different lines
      float srow[H2 > 0 ? H2 : 1], drow_[H2 > 0 ? H2 : 1];
#pragma unroll
      for (int hd = 0; hd < H2; ++hd) {
        const float sl = ps[hd].x + ps[hd].y, dl = pd[hd].x + pd[hd].y;
        srow[hd] = sl + __shfl_xor(sl, 32);
        drow_[hd] = dl + __shfl_xor(dl, 32);
      }
      if (AGG == 0 && id >= 0 && hl == 0) {
        float *ao = a.asd_out + (int64_t)id * 2 * H2;
        if constexpr (H2 == 4) {
          *reinterpret_cast<float4 *>(ao) = make_float4(srow[0], srow[1], srow[2], srow[3]);
          *reinterpret_cast<float4 *>(ao + 4) = make_float4(drow_[0], drow_[1], drow_[2], drow_[3]);
        } else if constexpr (H2 == 2) {
          *reinterpret_cast<float4 *>(ao) = make_float4(srow[0], srow[1], drow_[0], drow_[1]);
        } else if constexpr (H2 == 1) {
          *reinterpret_cast<float2 *>(ao) = make_float2(srow[0], drow_[0]);
        } else {
#pragma unroll
          for (int hd = 0; hd < H2; ++hd) { ao[hd] = srow[hd]; ao[H2 + hd] = drow_[hd]; }
        }
      }
    } else {
      // heads: hidden = relu(acc + b0); with hidden/2 == 32 tile 0 = classification, 1 = confidence,
      // 2 = correction hidden units.  Second layers: in-lane partial dots + one cross-half add.
      static_assert(EPI == EPI_NEXT || C == 64, "heads epilogue assumes hidden/2 == 32 (one accumulator tile per head)");
      const int ncls = a.classes;
      float lg[4] = {0.f, 0.f, 0.f, 0.f};
      float sc = 0.0f, sr = 0.0f;
      const int hl_e = lane_e >> 5;                      // (from the opaque lane id, like cell_e: `4 * hl` is shared with the prologue's attention-dot address)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c0 = 8 * g + 4 * hl_e;               // unit index within the head
          const float4 b4 = *reinterpret_cast<const float4 *>(attl + t * 32 + c0);
          float v[4] = {acc[t][4 * g] + b4.x, acc[t][4 * g + 1] + b4.y, acc[t][4 * g + 2] + b4.z,
                        acc[t][4 * g + 3] + b4.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = v[j] > 0.0f ? v[j] : 0.0f;
          if (t == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              if (k < ncls) {
                const float4 w4 = *reinterpret_cast<const float4 *>(attl + 96 + k * 32 + c0);
                lg[k] += v[0] * w4.x + v[1] * w4.y + v[2] * w4.z + v[3] * w4.w;
              }
            }
          } else if (t == 1) {
            const float4 w4 = *reinterpret_cast<const float4 *>(attl + 96 + ncls * 32 + c0);
            sc += v[0] * w4.x + v[1] * w4.y + v[2] * w4.z + v[3] * w4.w;
          } else if (a.has_corr) {
            const float4 w4 = *reinterpret_cast<const float4 *>(attl + 96 + (ncls + 1) * 32 + c0);
            sr += v[0] * w4.x + v[1] * w4.y + v[2] * w4.z + v[3] * w4.w;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) lg[k] += __shfl_xor(lg[k], 32);
      sc += __shfl_xor(sc, 32);
      sr += __shfl_xor(sr, 32);
      const int gr = pos.r0 + mr, gc = pos.c0 + mc;
      const bool inside = gr < pos.h && gc < pos.w;
      // (loaded BEFORE the first output store: vmcnt is one in-order queue for loads and stores, so a load issued after the
      //  logits / probabilities have been stored waits for HBM to take them)
      float sd_pre = 0.0f;
      if (hl == 0 && id >= 0 && a.has_corr && a.corr_grid) sd_pre = a.local_std[id];
      if (hl == 0 && inside && (!a.cell_map || id >= 0)) {
        // (canvas walk: only valid cells have an original position; the caller cleared the grids)
        const int64_t cidx = a.cell_map ? (int64_t)a.cell_map[id] : pos.cell_off + (int64_t)gr * pos.w + gc;
        float fcls = 0.f, fconf = 0.f, fcorr = 0.f;
        if (id >= 0) {
          float mx = -__builtin_inff();
#pragma unroll
          for (int k = 0; k < 4; ++k) if (k < ncls) { lg[k] += attl[288 + k]; mx = fmaxf(mx, lg[k]); }
          float pr[4], den = 0.0f;
#pragma unroll
          for (int k = 0; k < 4; ++k) { pr[k] = k < ncls ? expf(lg[k] - mx) : 0.0f; den += pr[k]; }
          int arg = 0;
          float best = -1.0f;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            pr[k] = pr[k] / den;
            if (k < ncls && pr[k] > best) { best = pr[k]; arg = k; }
          }
          const float conf = 1.0f / (1.0f + expf(-(sc + attl[288 + ncls])));
          const float corr = sr + attl[288 + ncls + 1];
          const int64_t n = id;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (k < ncls) {
              if (a.o.class_logits) a.o.class_logits[n * ncls + k] = lg[k];
              if (a.o.class_probs) a.o.class_probs[n * ncls + k] = pr[k];
            }
          }
          if (a.o.predicted_class) a.o.predicted_class[n] = arg;
          if (a.o.confidence) a.o.confidence[n] = conf;
          if (a.o.correction && a.has_corr) a.o.correction[n] = corr;
          int action = 0;
          if (arg == 2 && conf > a.thr_auto) action = 1;
          if (conf < a.thr_review) action = 2;
          if (a.o.action) a.o.action[n] = action;
          if (a.o.needs_review) a.o.needs_review[n] = action == 2;
          if (a.o.auto_correct) a.o.auto_correct[n] = action == 1;
          fcls = (float)arg; fconf = conf;
          if (a.has_corr && a.corr_grid) {
            float sd = sd_pre;
            sd = sd > a.norm_floor ? sd : a.norm_floor;
            fcorr = corr * sd;
          }
        }
        if (a.cls_grid) a.cls_grid[cidx] = fcls;
        if (a.conf_grid) a.conf_grid[cidx] = fconf;
        if (a.corr_grid) a.corr_grid[cidx] = fcorr;
      }
    }
  }
  BGNN_STAMP(8)   // final epilogue
#if BGNN_DIAG
  if (a.stamps && threadIdx.x == 0) {
    // counters 0..15: every instance; 32..47: the 256 -> 64 instance; 48..63: the heads instance (16..31: unused)
    unsigned long long *own = a.stamps + (EPI == EPI_HEADS ? 48 : NT == 2 ? 32 : 0);
    for (int i = 0; i < 12; ++i) atomicAdd(a.stamps + i, t_sum[i]);
    if (own != a.stamps) {
      for (int i = 0; i < 12; ++i) atomicAdd(own + i, t_sum[i]);
      atomicAdd(own + 15, 1ull);
    }
    atomicAdd(a.stamps + 15, 1ull);
    // shader cycles and 100 MHz reference ticks of this workgroup's lifetime: clock = cycles / ticks x 100 MHz
    atomicAdd(a.stamps + 13, __builtin_amdgcn_s_memtime() - t_clk0);
    atomicAdd(a.stamps + 14, __builtin_amdgcn_s_memrealtime() - t_real0);
  }
#endif
}

// ---- two-phase form of the bf16 256 -> 256 instance (matrix_path = bf16, BASELINE configs[2]) ------------------------------------
// The one-phase kernel above holds the [32 nodes x 256] accumulator (128 registers) NEXT TO everything the aggregation needs
// (~230 VGPRs, 78 KB of LDS: two workgroups per CU), and on the bf16 path neither pipe is the bound -- a workgroup's life is a
// chain of latencies that only MORE resident workgroups hide (the narrow instances gained 19 % going from two to three per CU).
// This form never holds both at once:
//   phase 1  for all 8 slabs: slab DMA -> aggregation MFMAs -> BatchNorm / ReLU -> the wave's [32 nodes x 32 ch] h slab as TWO
//            bf16x8 operands, kept in registers (8 x 8 = 64 VGPRs for the whole 256-channel h row block); no weights, no accumulator;
//   phase 2  four column passes of 64 columns (= one head of the next layer): the pass's whole W^T slice (16 k-steps x 2 tiles x
//            1 KiB = 32 KB, LDS-DMA into the region the slab image and the alpha matrices no longer need) -> 32 MFMAs into 32
//            accumulator registers -> attention dots + bf16 store of those 64 columns, under the next pass's W DMA.
// ~160 VGPRs and 51 KB of LDS: THREE workgroups per CU.  Per accumulator the MFMAs run in the same k order as in the one-phase
// kernel, the aggregation / BatchNorm / conversion code is the same: bit-identical results (tests/test_gpu_forward.py).
template <int K>
struct TwoPhaseLds {
  using Geo = FusedGeom<K>;
  using Win = AggWindow<K>;
  static constexpr int HR = Geo::HR, H = 4, HC = 256, NC = 256;       // NC: the next layer's four heads of 64 columns
  static constexpr int SLAB_B = HR * 64;                 // bf16 slab image [HR][32 ch]
  static constexpr int PAD_B = 512;                      // zeros: the k = 16 window's last MFMA reads 8 rows past the image (AggWindow)
  static constexpr int ALPHA_B = 4 * 32 * Win::PITCH;    // four wave-private dense alpha matrices
  static constexpr int SCSH_B = 2 * HC * 4;
  static constexpr int P1_B = SLAB_B + PAD_B + ALPHA_B + SCSH_B;
  static constexpr int W_B = 16 * 2 * 1024;              // one column pass of W^T
  static constexpr int PATCH_B = 4 * 32 * 128;           // four wave-private two-tile bf16 store patches
  static constexpr int ATT_B = 2 * NC * 4;
  static constexpr int P2_B = W_B + PATCH_B + ATT_B;
  static constexpr int SHARED_B = P1_B > P2_B ? P1_B : P2_B;
  static constexpr int BYTES = SHARED_B + 128 * 4 + 16;  // + node id of each block cell + the canvas walk's "any node" flags
  static_assert((SLAB_B + PAD_B) % 16 == 0, "the dense matrices start on a 16-byte boundary");
  static_assert(HR * (H + 2) * 4 <= ALPHA_B, "alpha_src, depth and id tables of the halo fit the (not yet written) alpha region");
  static_assert(SLAB_B + PAD_B + ALPHA_B <= W_B + PATCH_B, "scale / shift sit clear of the att vectors' landing zone");
  static_assert(3 * BYTES <= 160 * 1024, "three workgroups per CU");
};

// AF ("aggregate first", layer 0 only): a.xw is the extractor's h1 [rows][64] bf16 (gemm_f32.hip, extractor_af_kernel) instead of the
// 256-channel lin_0 product.  The sum over the in-edges is linear, so head hd's 64 output channels are W0_hd (sum_j alpha^hd_ij h1_j) + b:
// phase 1 aggregates the TWO 32-channel slabs of h1 once per head (the same 8 x 8 aggregation MFMAs, two slab DMAs instead of eight, a
// quarter of the bytes), an inserted step applies each head's 64 x 64 block of the folded lin_0 weight (a.W0af: 32 KB through the pass
// buffer, 8 MFMAs per head), folded bias + BatchNorm + ReLU (a.shift carries W's bias: the coefficients of a node sum to 1), and hands
// phase 2 the same [32 nodes x 256] bf16 operands.  The front GEMM's launch, its 512-byte rows and six slab round trips per block go.
template <int K, bool AF = false>
__global__ __launch_bounds__(256, 3) void gat_layer_bf16_2p_kernel(FusedArgs a) {
  static_assert(!AF || TwoPhaseLds<K>::SLAB_B + TwoPhaseLds<K>::PAD_B + TwoPhaseLds<K>::ALPHA_B >= TwoPhaseLds<K>::W_B,
                "aggregate-first: the scale / shift table sits clear of the pass buffer the heads' weight blocks land in");
  constexpr int NTH = 256, HC = 256, C = 64, H = 4, H2 = 4, NC = 64 * H2, NT = 2 * H2, NSLAB = 8, SPH = 2, NHL = 2;   // H2: heads of the next layer = column passes
  constexpr int SRC_ROWB = AF ? 128 : HC * 2;             // bytes of a source row (AF: the 64-channel h1)
  using Geo = FusedGeom<K>;
  using Lds = TwoPhaseLds<K>;
  using Win = AggWindow<K>;
  using Off = StencilOffsets<K>;
  constexpr int HR = Geo::HR, HW_ = Geo::HW, RAD = Geo::R;
  constexpr int ROWB = 64, CPR = 4;
  extern __shared__ __attribute__((aligned(128))) float lds[];
  char *base = reinterpret_cast<char *>(lds);
  float *slab = lds;                                                             // phase 1
  float *alx = reinterpret_cast<float *>(base + Lds::SLAB_B + Lds::PAD_B);       // phase 1: dense alpha; before that the halo tables
  float *scsh = reinterpret_cast<float *>(base + Lds::SLAB_B + Lds::PAD_B + Lds::ALPHA_B);
  float *has = alx;                                                              // [H][HR]
  float *hdp = has + HR * H;                                                     // [HR]
  int *hid = reinterpret_cast<int *>(hdp + HR);                                  // [HR]
  char *wpass = base;                                                            // phase 2: [16 k-steps][2 tiles][1 KiB]
  char *patches = base + Lds::W_B;                                               // phase 2: [4 waves][32 rows][128 B]
  float *attl = reinterpret_cast<float *>(base + Lds::W_B + Lds::PATCH_B);       // phase 2: att_src | att_dst of the next layer
  int *cid = reinterpret_cast<int *>(base + Lds::SHARED_B);                      // [128] node id of each block cell
  int *minid = cid + 128;

  const BlockPos pos = decode_block<FT_H>(a.tb);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hl = lane >> 5;
  const int cell = wave * 32 + r;
  const int tr = cell / TILE_W, tc = cell % TILE_W;
  const int self_idx = (tr + RAD) * HW_ + tc + RAD;

  // ---- prologue: the one-phase kernel's two load rounds (see there), without any weight traffic
  static_assert(HR <= NTH, "one halo row per thread");
  constexpr int NPIECE = (HR * CPR + NTH - 1) / NTH;
  static_assert((NPIECE - 2) * NTH + NTH - 64 < HR * CPR, "every wave moves NPIECE or NPIECE - 1 pieces");
  const uint32_t cbase = (uint32_t)pos.cell_off, uw = (uint32_t)pos.w, uh = (uint32_t)pos.h;
  const int h1 = pos.h - 1, w1 = pos.w - 1;
  auto cell_index = [&](int gr, int gc) -> uint32_t {
    const int r_ = max(0, min(gr, h1)), c_ = max(0, min(gc, w1));
    return cbase + __umul24((uint32_t)r_, uw) + (uint32_t)c_;
  };
  auto node_at = [&](uint32_t cl) -> int {
    return *reinterpret_cast<const int *>(reinterpret_cast<const char *>(a.node_id) + (cl << 2));
  };
  auto in_tile = [&](int gr, int gc) -> bool { return (uint32_t)gr < uh && (uint32_t)gc < uw; };
  const int hr_t = tid / HW_, hc_t = tid - hr_t * HW_;
  const int gr_h = pos.r0 + hr_t - RAD, gc_h = pos.c0 + hc_t - RAD;
  const int gr_m = pos.r0 + tr, gc_m = pos.c0 + tc;
  const int raw_h = node_at(cell_index(gr_h, gc_h));
  const uint32_t cell_m = cell_index(gr_m, gc_m);
  const int raw_m = node_at(cell_m);
  int tile_m = pos.tile;
  if (a.tile_of_cell) {                                 // (only cells that hold a node have an entry: the table is not cleared)
    const int t_ = *reinterpret_cast<const int *>(reinterpret_cast<const char *>(a.tile_of_cell) + (cell_m << 2));
    tile_m = raw_m >= 0 ? t_ : 0;
  }
  static_assert(NTH % CPR == 0, "pieces advance by whole halo rows");
  constexpr int RSTEP = NTH / CPR, RSTEP_R = RSTEP / HW_, RSTEP_C = RSTEP % HW_;
  int drow[NPIECE], prow_r[NPIECE], prow_c[NPIECE];
  {
    const int row0 = tid / CPR;
    int pr = row0 / HW_, pc = row0 - pr * HW_;
#pragma unroll
    for (int p = 0; p < NPIECE; ++p) {
      prow_r[p] = pr; prow_c[p] = pc;
      drow[p] = node_at(cell_index(pos.r0 + pr - RAD, pos.c0 + pc - RAD));
      pr += RSTEP_R; pc += RSTEP_C;
      if (pc >= HW_) { pc -= HW_; pr += 1; }
    }
  }
  float scv = a.scale[tid], shv = a.shift[tid];          // HC == NTH: one channel per thread
  float vpre[NHL][3];
#pragma unroll
  for (int i = 0; i < NHL; ++i)
#pragma unroll
    for (int f = 0; f < 3; ++f) vpre[i][f] = a.V[(hl + i * 2) * 3 + f];
  int hid_v = (tid < HR && in_tile(gr_h, gc_h) && raw_h >= 0) ? raw_h : -1;
  int my_pre = in_tile(gr_m, gc_m) ? raw_m : -1;
#pragma unroll
  for (int p = 0; p < NPIECE; ++p) {
    const bool row_ok = (p + 1) * NTH <= HR * CPR || prow_r[p] < FT_H + 2 * RAD;
    if (!(row_ok && in_tile(pos.r0 + prow_r[p] - RAD, pos.c0 + prow_c[p] - RAD))) drow[p] = -1;
  }
  if (a.cell_map) {                  // canvas walk: blocks that hold only gutter / free space leave here (nothing is in flight yet)
    const bool wave_any = __builtin_amdgcn_ballot_w64(my_pre >= 0) != 0;
    if (lane == 0) minid[wave] = wave_any ? 1 : 0;
    __syncthreads();
    if ((minid[0] | minid[1] | minid[2] | minid[3]) == 0) return;
  }
  float eraw[K], adv[NHL], hasv[H], hdep;
  float4 tdist;
  {
    const uint64_t hrow = (uint32_t)(hid_v >= 0 ? hid_v : 0), mrow = (uint32_t)(my_pre >= 0 ? my_pre : 0);
    hdep = a.node_depth[hrow];
    tdist = a.tile_dist[tile_m];
    const float4 v4 = *reinterpret_cast<const float4 *>(a.asd + hrow * 2 * H);
    hasv[0] = v4.x; hasv[1] = v4.y; hasv[2] = v4.z; hasv[3] = v4.w;
    const float4 *ep = reinterpret_cast<const float4 *>(a.slope + mrow * K);
#pragma unroll
    for (int i = 0; i < K / 4; ++i) {
      const float4 q = ep[i];
      eraw[4 * i] = q.x; eraw[4 * i + 1] = q.y; eraw[4 * i + 2] = q.z; eraw[4 * i + 3] = q.w;
    }
#pragma unroll
    for (int i = 0; i < NHL; ++i) adv[i] = a.asd[mrow * 2 * H + H + hl + i * 2];
  }
  auto swz = [](int row) { return (row >> 2) & 3; };
  static_assert(NSLAB * ROWB <= 4096, "the zero page covers a whole block's worth of slab offsets");
  const char *xbase = reinterpret_cast<const char *>(a.xw);
  const char *zp = reinterpret_cast<const char *>(a.zero_page);
  const char *dbase[NPIECE];
  {
    const int cc = tid % CPR;
#pragma unroll
    for (int p = 0; p < NPIECE; ++p) {
      const int row = prow_r[p] * HW_ + prow_c[p];
      const int c = cc ^ swz(row);
      dbase[p] = drow[p] >= 0 ? xbase + ((uint64_t)(uint32_t)drow[p] * (uint32_t)SRC_ROWB + (uint32_t)(c * 16)) : zp;
    }
  }
  auto issue_slab = [&](int s) {
    const int sb = s * ROWB;
#pragma unroll
    for (int p = 0; p < NPIECE; ++p) {
      if ((p + 1) * NTH <= HR * CPR || p * NTH + tid < HR * CPR)
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(dbase[p] + sb),
                                         (__attribute__((address_space(3))) void *)(slab + (p * NTH + wave * 64) * 4), 16, 0, 0);
    }
  };
  if (tid < HR) {
    hid[tid] = hid_v;
#pragma unroll
    for (int hh = 0; hh < H; ++hh) has[hh * HR + tid] = hid_v >= 0 ? hasv[hh] : -__builtin_inff();
    hdp[tid] = hid_v >= 0 ? hdep : 0.0f;
  }
  if (hl == 0) cid[cell] = my_pre < 0 ? -1 : my_pre;
  if (tid < Lds::PAD_B / 4) reinterpret_cast<float *>(base + Lds::SLAB_B)[tid] = 0.0f;   // (the rows read past the image: zeros)
  {
    float sink = 0.0f;
#pragma unroll
    for (int i = 0; i < NHL; ++i) sink += adv[i];
#pragma unroll
    for (int i = 0; i < K; ++i) sink += eraw[i];
#pragma unroll
    for (int hh = 0; hh < H; ++hh) sink += hasv[hh];
    sink += hdep + tdist.x + tdist.y + tdist.z + scv + shv;
    asm volatile("" ::"v"(sink));
  }
  issue_slab(0);
  wait_lgkm0();
  __builtin_amdgcn_s_barrier();                          // halo tables in LDS (slab 0 stays in flight)

  // ---- phase A: attention coefficients, kept as bf16 pairs until their head's slabs come up
  uint32_t apk[NHL][(K + 2) / 2];
#pragma unroll
  for (int i = 0; i < NHL; ++i)
#pragma unroll
    for (int b = 0; b < (K + 2) / 2; ++b) apk[i][b] = 0u;
  {
    const uint32_t hid0 = lds_addr(hid), has0 = lds_addr(has);
    int my = lds_read1i<0>(hid0 + (uint32_t)self_idx * 4u);
    lds_reads_done();
    float part[NHL][K + 1];
    if (my < 0) {
#pragma unroll
      for (int i = 0; i < NHL; ++i)
#pragma unroll
        for (int b = 0; b <= K; ++b) part[i][b] = 0.0f;
    } else {
      using S = HaloSlot<K, HW_>;
      int nb[K];
      float hs[NHL][K + 1];
      halo_ids<K, HW_>(hid0 + (uint32_t)(self_idx - S::MAXOFF) * 4u, nb, std::make_integer_sequence<int, K>{});
#pragma unroll
      for (int i = 0; i < NHL; ++i)
        halo_alpha_src<H, K, HW_>(has0 + (uint32_t)((hl + i * 2) * HR + self_idx - S::MAXOFF) * 4u, hs[i], std::make_integer_sequence<int, K>{});
      float dsrc[K + 1];
      halo_depths<K, HW_>(lds_addr(hdp) + (uint32_t)(self_idx - S::MAXOFF) * 4u, dsrc, std::make_integer_sequence<int, K>{});
      lds_reads_done();
      EdgeTerms<K> et;
      edge_terms_compact<K>(nb, eraw, dsrc, tdist.x, tdist.y, tdist.z, et);
      attention_head_pair<K, false>(et, hs[0], hs[1], adv[0], adv[1], vpre[0], vpre[1], part[0], part[1]);
    }
#pragma unroll
    for (int i = 0; i < NHL; ++i)
#pragma unroll
      for (int b = 0; b <= K; b += 2) apk[i][b / 2] = pack_bf16x2(part[i][b], b + 1 <= K ? part[i][b + 1] : 0.0f);
  }

  // ---- phase 1: aggregate every slab; h stays in registers as bf16 MFMA operands
  const uint32_t slab0 = lds_addr(slab);
  const uint32_t scsh0 = lds_addr(scsh) + hl * 16;
  const int wbase = Win::base(wave);
  const uint32_t dn0 = lds_addr(alx) + wave * (32 * Win::PITCH);
  const uint32_t bq0 = dn0 + r * Win::PITCH + hl * 16;
  uint32_t tr0, tr1;
  {
    // (an opaque copy of hl for this one-off address: hipcc otherwise shares `hl << 3` with phase 2's patch offsets, keeps it alive
    //  across phase A and phase 1 and -- at k = 16 -- spills it; the reload then sat in pass 0's epilogue behind an s_waitcnt vmcnt(0),
    //  i.e. behind the W DMA of pass 1 the epilogue is meant to run under)
    int hl1 = hl;
    asm volatile("" : "+v"(hl1));
    const int grp = lane >> 4, q = (lane >> 2) & 3, p4 = lane & 3, cb = grp & 1;
    const int row0 = wbase + 8 * hl1 + q;
    const int c = 2 * cb + (p4 >> 1);
    tr0 = slab0 + row0 * 64 + ((c ^ ((row0 >> 2) & 3)) << 4) + 8 * (p4 & 1);
    tr1 = slab0 + (row0 + 4) * 64 + ((c ^ (((row0 + 4) >> 2) & 3)) << 4) + 8 * (p4 & 1);
  }
  auto densify = [&](int hd, bool clear = true) {
    if (hd == 0 && clear) {
      const u32x4 z4 = {0u, 0u, 0u, 0u};
      constexpr int DB = 32 * Win::PITCH;
#pragma unroll
      for (int i = 0; i < (DB + 1023) / 1024; ++i)
        if ((i + 1) * 1024 <= DB || lane * 16 + i * 1024 < DB)
          asm volatile("ds_write_b128 %0, %1" ::"v"(dn0 + lane * 16 + i * 1024), "v"(z4) : "memory");
    }
    if (hl == (hd & 1)) {
      const int wself = self_idx - wbase;
      const uint32_t rowb = dn0 + r * Win::PITCH;
#pragma unroll
      for (int b = 0; b <= K; ++b) {
        const int off = b < K ? Off::dr[b < K ? b : 0] * HW_ + Off::dc[b < K ? b : 0] : 0;
        const uint32_t ad = rowb + (uint32_t)(wself - off) * 2u;
        const uint32_t v = (hd >> 1) ? apk[1][b / 2] : apk[0][b / 2];
        if (b & 1) asm volatile("ds_write_b16_d16_hi %0, %1" ::"v"(ad), "v"(v) : "memory");
        else asm volatile("ds_write_b16 %0, %1" ::"v"(ad), "v"(v) : "memory");
      }
    }
  };
  // W^T image (hi-only bf16, MFMA A-fragment lane order): k-step st, tile t at (st * NT + t) KiB.  A pass moves tiles 2 cp, 2 cp + 1
  // of all 16 k-steps: 32 pieces of 1 KiB, 8 per wave, to wpass + (st * 2 + tt) KiB.
  auto issue_w = [&](int cp) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int q = j * 4 + wave;                        // piece: st = q >> 1, tt = q & 1
      __builtin_amdgcn_global_load_lds(
          reinterpret_cast<const void *>(reinterpret_cast<const char *>(a.Wt) + ((q >> 1) * NT + 2 * cp + (q & 1)) * 1024 + lane * 16),
          (__attribute__((address_space(3))) void *)(wpass + q * 1024), 16, 0, 0);
    }
  };
  bf16x8 xh[NSLAB][2];
  auto slab_step = [&](auto sc) {
    constexpr int s = decltype(sc)::value;
    if constexpr (s % SPH == 0 && s > 0) densify(s / SPH);
    wait_vm_lgkm<0>();                                   // slab s is all this wave has in flight
    __builtin_amdgcn_s_barrier();                        // slab s visible to every wave
    if constexpr (s == 0) {
      scsh[tid] = scv; scsh[HC + tid] = shv;             // (phase A is over on every wave: nothing is in flight, visible stores are fine)
      densify(0);
      wait_lgkm0();
      __builtin_amdgcn_s_barrier();
    }
    f32x16 d;
    if constexpr (Win::NKB == 8) {
      agg_blocks<0, 4, true, false>(d, tr0, tr1, bq0, hl);
      agg_blocks<4, 4, false, Win::TAIL_BEYOND_PITCH>(d, tr0, tr1, bq0, hl);
    } else {
      static_assert(Win::NKB == 5, "window blocks");
      agg_blocks<0, 3, true, false>(d, tr0, tr1, bq0, hl);
      agg_blocks<3, 2, false, false>(d, tr0, tr1, bq0, hl);
    }
    // (the reads of slab s are complete -- agg_blocks waits for them before its MFMAs -- so the image can be handed to slab s + 1
    //  as soon as every wave is here; BatchNorm / ReLU / conversion then run under that DMA's flight)
    __builtin_amdgcn_s_barrier();
    if constexpr (s + 1 < NSLAB) {
      issue_slab(s + 1);
    } else {
      // last slab: the image and the alpha matrices are dead on every wave -> phase 2's first W pass and the next layer's
      // att_src | att_dst can be requested NOW (they land in [0, 32 KB) and behind the patches: clear of the scale / shift table the
      // BatchNorm below still reads).  One att piece per wave (waves 2, 3 repeat 0, 1's) so that every wave's VM queue counts alike.
      if (lane * 4 < NC)
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(((wave & 1) == 0 ? a.att_src : a.att_dst) + lane * 4),
                                         (__attribute__((address_space(3))) void *)(attl + (wave & 1) * NC), 16, 0, 0);
      issue_w(0);
    }
    f32x4 g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = (f32x4){d[4 * j], d[4 * j + 1], d[4 * j + 2], d[4 * j + 3]};
    {
      const uint32_t cp = scsh0 + s * 128;
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        f32x4 sc0, sc1, sh0, sh1;
        if (jp == 0) { sc0 = lds_read4<0>(cp); sc1 = lds_read4<32>(cp); sh0 = lds_read4<HC * 4>(cp); sh1 = lds_read4<HC * 4 + 32>(cp); }
        else { sc0 = lds_read4<64>(cp); sc1 = lds_read4<96>(cp); sh0 = lds_read4<HC * 4 + 64>(cp); sh1 = lds_read4<HC * 4 + 96>(cp); }
        lds_reads_done();
        g[2 * jp] = g[2 * jp] * sc0 + sh0;
        g[2 * jp + 1] = g[2 * jp + 1] * sc1 + sh1;
      }
      if (a.relu) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          asm("v_max_f32 %0, 0, %0" : "+v"(g[j].x)); asm("v_max_f32 %0, 0, %0" : "+v"(g[j].y));
          asm("v_max_f32 %0, 0, %0" : "+v"(g[j].z)); asm("v_max_f32 %0, 0, %0" : "+v"(g[j].w));
        }
      }
    }
    xh[s][0] = to_bf16x8(g[0], g[1]);
    xh[s][1] = to_bf16x8(g[2], g[3]);
  };
  if constexpr (!AF) {
    slab_step(std::integral_constant<int, 0>{}); slab_step(std::integral_constant<int, 1>{});
    slab_step(std::integral_constant<int, 2>{}); slab_step(std::integral_constant<int, 3>{});
    slab_step(std::integral_constant<int, 4>{}); slab_step(std::integral_constant<int, 5>{});
    slab_step(std::integral_constant<int, 6>{}); slab_step(std::integral_constant<int, 7>{});
  } else {
    // ---- aggregate first: the two slabs of h1, each under all four heads' coefficients; then the heads' 64 x 64 weight blocks
    bf16x8 xa[H][2][2];                                  // [head][slab][k half]: sum_j alpha^hd_ij h1_j as bf16 MFMA operands (64 VGPRs)
    auto af_slab = [&](auto sc) {
      constexpr int s = decltype(sc)::value;
      wait_vm_lgkm<0>();                                 // slab s is all this wave has in flight
      __builtin_amdgcn_s_barrier();                      // slab s visible to every wave (s = 0: phase A is over on every wave)
      if constexpr (s == 0) { scsh[tid] = scv; scsh[HC + tid] = shv; }     // (nothing is in flight: visible stores are fine; read in the weight step)
      auto head = [&](auto hc) {
        constexpr int hd = decltype(hc)::value;
        // the wave's dense matrix is private to it and LDS operations of a wave are served in order: the MFMAs' reads of the head
        // before are complete (agg_blocks waits for them), these writes are served before the reads below
        densify(hd, s == 0);
        f32x16 d;
        if constexpr (Win::NKB == 8) {
          agg_blocks<0, 4, true, false>(d, tr0, tr1, bq0, hl);
          agg_blocks<4, 4, false, Win::TAIL_BEYOND_PITCH>(d, tr0, tr1, bq0, hl);
        } else {
          agg_blocks<0, 3, true, false>(d, tr0, tr1, bq0, hl);
          agg_blocks<3, 2, false, false>(d, tr0, tr1, bq0, hl);
        }
        f32x4 g[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = (f32x4){d[4 * j], d[4 * j + 1], d[4 * j + 2], d[4 * j + 3]};
        xa[hd][s][0] = to_bf16x8(g[0], g[1]);
        xa[hd][s][1] = to_bf16x8(g[2], g[3]);
      };
      head(std::integral_constant<int, 0>{}); head(std::integral_constant<int, 1>{});
      head(std::integral_constant<int, 2>{}); head(std::integral_constant<int, 3>{});
      __builtin_amdgcn_s_barrier();                      // every wave has read slab s
      if constexpr (s == 0) {
        issue_slab(1);
      } else {
        // the image and the alpha matrices are dead: the heads' weight blocks (32 pieces of 1 KiB, [head][k-step][tile], into the pass
        // buffer) and the next layer's att vectors can be requested
        if (lane * 4 < NC)
          __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(((wave & 1) == 0 ? a.att_src : a.att_dst) + lane * 4),
                                           (__attribute__((address_space(3))) void *)(attl + (wave & 1) * NC), 16, 0, 0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int q = j * 4 + wave;
          __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(reinterpret_cast<const char *>(a.W0af) + q * 1024 + lane * 16),
                                           (__attribute__((address_space(3))) void *)(wpass + q * 1024), 16, 0, 0);
        }
      }
    };
    af_slab(std::integral_constant<int, 0>{}); af_slab(std::integral_constant<int, 1>{});
    wait_vm_lgkm<0>();
    __builtin_amdgcn_s_barrier();                        // the weight blocks (and the att vectors) are visible
    const uint32_t w0frag = lds_addr(wpass) + lane * 16;
    auto head_gemm = [&](auto hc) {
      constexpr int hd = decltype(hc)::value;
      // one 32-column tile at a time (4 fragments, 16 accumulator registers): both tiles at once did not fit beside xa / xh
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 w[4];                                      // k-step kk, tile t of head hd: (hd * 8 + 2 kk + t) KiB
        if (t == 0) { w[0] = lds_read4<(hd * 8 + 0) * 1024>(w0frag); w[1] = lds_read4<(hd * 8 + 2) * 1024>(w0frag);
                      w[2] = lds_read4<(hd * 8 + 4) * 1024>(w0frag); w[3] = lds_read4<(hd * 8 + 6) * 1024>(w0frag); }
        else { w[0] = lds_read4<(hd * 8 + 1) * 1024>(w0frag); w[1] = lds_read4<(hd * 8 + 3) * 1024>(w0frag);
               w[2] = lds_read4<(hd * 8 + 5) * 1024>(w0frag); w[3] = lds_read4<(hd * 8 + 7) * 1024>(w0frag); }
        lds_reads_done();
        if (hd == H - 1 && t == 1) {
          // every wave has read the last fragments: the pass buffer can take the first column pass of phase 2, which then flies
          // under this tile's MFMAs and epilogue
          __builtin_amdgcn_s_barrier();
          issue_w(0);
        }
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)                   // k-step kk = channels 16 kk .. of h1 = slab kk / 2, half kk % 2
          acc = mfma_lp(__builtin_bit_cast(bf16x8, w[kk]), xa[hd][kk / 2][kk % 2], acc);
        // folded bias + BatchNorm + ReLU of layer 0's output channels 64 hd + 32 t ..: "slab" 2 hd + t of the 256-channel h
        const int sl = 2 * hd + t;
        f32x4 g[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = (f32x4){acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]};
        const uint32_t cp = scsh0 + sl * 128;
#pragma unroll
        for (int jp = 0; jp < 2; ++jp) {
          f32x4 sc0, sc1, sh0, sh1;
          if (jp == 0) { sc0 = lds_read4<0>(cp); sc1 = lds_read4<32>(cp); sh0 = lds_read4<HC * 4>(cp); sh1 = lds_read4<HC * 4 + 32>(cp); }
          else { sc0 = lds_read4<64>(cp); sc1 = lds_read4<96>(cp); sh0 = lds_read4<HC * 4 + 64>(cp); sh1 = lds_read4<HC * 4 + 96>(cp); }
          lds_reads_done();
          g[2 * jp] = g[2 * jp] * sc0 + sh0;
          g[2 * jp + 1] = g[2 * jp + 1] * sc1 + sh1;
        }
        if (a.relu) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            asm("v_max_f32 %0, 0, %0" : "+v"(g[j].x)); asm("v_max_f32 %0, 0, %0" : "+v"(g[j].y));
            asm("v_max_f32 %0, 0, %0" : "+v"(g[j].z)); asm("v_max_f32 %0, 0, %0" : "+v"(g[j].w));
          }
        }
        xh[2 * hd + t][0] = to_bf16x8(g[0], g[1]);
        xh[2 * hd + t][1] = to_bf16x8(g[2], g[3]);
      }
    };
    head_gemm(std::integral_constant<int, 0>{}); head_gemm(std::integral_constant<int, 1>{});
    head_gemm(std::integral_constant<int, 2>{}); head_gemm(std::integral_constant<int, 3>{});
  }

  // ---- phase 2: the GEMM, one head (64 columns) of the next layer per pass (W(0) and the att vectors are already in flight; the
  // first pass's barrier also orders every wave's last scale / shift read before the first patch write)
  const uint32_t wfrag = lds_addr(wpass) + lane * 16;
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  // (a pass's two-lane partial dots are folded to one float per head as soon as the pass is over -- the same `x + y` the end of the
  //  kernel used to do -- and the row stores keep the node id, not the 64-bit row pointer: 12 registers less across the passes,
  //  which is what the k = 16 instance lacked at three workgroups per CU)
  float sl_[H2], dl_[H2];
  const int id = cid[cell];
  constexpr int NSTORE = 4;
  int rid_[NSTORE];
#pragma unroll
  for (int k = 0; k < NSTORE; ++k) rid_[k] = cid[wave * 32 + (lane >> 3) + 8 * k];
  char *patch = patches + wave * (32 * 128);
  const uint32_t asl = lds_addr(attl + 4 * hl);
  auto col_pass = [&](auto cpc) {
    constexpr int cp = decltype(cpc)::value;
    // VM queue of this wave: [att piece][W(0) x 8] (cp = 0) / [W(cp) x 8][the 4 row stores of pass cp - 1] (cp > 0)
    if constexpr (cp == 0) wait_vm_lgkm<0>(); else wait_vm_lgkm<NSTORE>();
    __builtin_amdgcn_s_barrier();                        // W(cp) visible
    f32x16 acc0, acc1;
    f32x2 ps_ = {0.f, 0.f}, pd_ = {0.f, 0.f};
    {
      const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      acc0 = z; acc1 = z;
    }
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {                     // four k-steps (two slabs) per LDS wait
      f32x4 w[8];
      if (q4 == 0) { w[0] = lds_read4<0>(wfrag); w[1] = lds_read4<1024>(wfrag); w[2] = lds_read4<2048>(wfrag); w[3] = lds_read4<3072>(wfrag);
                     w[4] = lds_read4<4096>(wfrag); w[5] = lds_read4<5120>(wfrag); w[6] = lds_read4<6144>(wfrag); w[7] = lds_read4<7168>(wfrag); }
      if (q4 == 1) { w[0] = lds_read4<8192>(wfrag); w[1] = lds_read4<9216>(wfrag); w[2] = lds_read4<10240>(wfrag); w[3] = lds_read4<11264>(wfrag);
                     w[4] = lds_read4<12288>(wfrag); w[5] = lds_read4<13312>(wfrag); w[6] = lds_read4<14336>(wfrag); w[7] = lds_read4<15360>(wfrag); }
      if (q4 == 2) { w[0] = lds_read4<16384>(wfrag); w[1] = lds_read4<17408>(wfrag); w[2] = lds_read4<18432>(wfrag); w[3] = lds_read4<19456>(wfrag);
                     w[4] = lds_read4<20480>(wfrag); w[5] = lds_read4<21504>(wfrag); w[6] = lds_read4<22528>(wfrag); w[7] = lds_read4<23552>(wfrag); }
      if (q4 == 3) { w[0] = lds_read4<24576>(wfrag); w[1] = lds_read4<25600>(wfrag); w[2] = lds_read4<26624>(wfrag); w[3] = lds_read4<27648>(wfrag);
                     w[4] = lds_read4<28672>(wfrag); w[5] = lds_read4<29696>(wfrag); w[6] = lds_read4<30720>(wfrag); w[7] = lds_read4<31744>(wfrag); }
      lds_reads_done();
#pragma unroll
      for (int i = 0; i < 4; ++i) {                      // k-step st = 4 q4 + i = slab st / 2, half st % 2
        const int st = 4 * q4 + i;
        acc0 = mfma_lp(__builtin_bit_cast(bf16x8, w[2 * i]), xh[st / 2][st % 2], acc0);
        acc1 = mfma_lp(__builtin_bit_cast(bf16x8, w[2 * i + 1]), xh[st / 2][st % 2], acc1);
      }
    }
    __builtin_amdgcn_s_barrier();                        // every wave has read W(cp)
    if constexpr (cp + 1 < H2) issue_w(cp + 1);
    // epilogue of the pass: head cp of the next layer -- attention dots, bf16 conversion, two tiles side by side through the
    // wave's patch, whole 128-byte row segments out (the one-phase kernel's epilogue, tile pair (2 cp, 2 cp + 1))
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      constexpr int NC4 = NC * 4;
      const int t = 2 * cp + tt;
      const f32x16 &acc = tt ? acc1 : acc0;
      f32x4 s4[4], d4[4];
      s4[0] = lds_read4<0>(asl + t * 128); s4[1] = lds_read4<32>(asl + t * 128);
      s4[2] = lds_read4<64>(asl + t * 128); s4[3] = lds_read4<96>(asl + t * 128);
      d4[0] = lds_read4<NC4>(asl + t * 128); d4[1] = lds_read4<NC4 + 32>(asl + t * 128);
      d4[2] = lds_read4<NC4 + 64>(asl + t * 128); d4[3] = lds_read4<NC4 + 96>(asl + t * 128);
      lds_reads_done();
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 v = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
        const f32x2 vlo = {v.x, v.y}, vhi = {v.z, v.w};
        ps_ += vlo * (f32x2){s4[g].x, s4[g].y}; ps_ += vhi * (f32x2){s4[g].z, s4[g].w};
        pd_ += vlo * (f32x2){d4[g].x, d4[g].y}; pd_ += vhi * (f32x2){d4[g].z, d4[g].w};
        typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
        bf16x4 o;
        o[0] = (__bf16)v.x; o[1] = (__bf16)v.y; o[2] = (__bf16)v.z; o[3] = (__bf16)v.w;
        char *pb = patch + r * 128 + ((hl ^ ((r >> 3) & 1)) << 3);
        *reinterpret_cast<bf16x4 *>(pb + (((tt * 4 + g) ^ (r & 7)) << 4)) = o;
      }
      asm volatile("" : "+v"(ps_), "+v"(pd_));
      __builtin_amdgcn_sched_barrier(0);
    }
    sl_[cp] = ps_.x + ps_.y; dl_[cp] = pd_.x + pd_.y;
#pragma unroll
    for (int k = 0; k < NSTORE; ++k) {
      const int row = (lane >> 3) + 8 * k;
      uint4 q = *reinterpret_cast<const uint4 *>(patch + row * 128 + (((lane & 7) ^ (row & 7)) << 4));
      if (k & 1) q = make_uint4(q.z, q.w, q.x, q.y);
      char *prow = (rid_[k] >= 0 ? reinterpret_cast<char *>(a.out) + (int64_t)rid_[k] * (NC * 2) : reinterpret_cast<char *>(a.dump)) + (lane & 7) * 16;
      *reinterpret_cast<uint4 *>(prow + cp * 128) = q;
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  col_pass(std::integral_constant<int, 0>{}); col_pass(std::integral_constant<int, 1>{});
  col_pass(std::integral_constant<int, 2>{}); col_pass(std::integral_constant<int, 3>{});
  {
    float srow[H2], drow_[H2];
#pragma unroll
    for (int hd = 0; hd < H2; ++hd) {
      const float sl = sl_[hd], dl = dl_[hd];
      srow[hd] = sl + __shfl_xor(sl, 32);
      drow_[hd] = dl + __shfl_xor(dl, 32);
    }
    if (id >= 0 && hl == 0) {
      float *ao = a.asd_out + (int64_t)id * 2 * H2;
      *reinterpret_cast<float4 *>(ao) = make_float4(srow[0], srow[1], srow[2], srow[3]);
      *reinterpret_cast<float4 *>(ao + 4) = make_float4(drow_[0], drow_[1], drow_[2], drow_[3]);
    }
  }
}

template <int K, bool AF = false>
static int launch_two_phase(bgnn_ctx *ctx, const FusedArgs &a) {
  constexpr size_t lds_bytes = (size_t)TwoPhaseLds<K>::BYTES;
  static std::atomic<uint64_t> configured{0};
  auto kern = gat_layer_bf16_2p_kernel<K, AF>;
  if (!(configured.load(std::memory_order_relaxed) >> (ctx->device & 63) & 1)) {
    BGNN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    configured.fetch_or(1ull << (ctx->device & 63), std::memory_order_relaxed);
  }
  hipLaunchKernelGGL(kern, dim3(a.tb.n_blocks), dim3(256), lds_bytes, ctx->stream, a);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

template <int HC, int C, int K, int NT, int EPI, int SP = 0, int AGG = 0, int LF = 0>
static int launch_inst(bgnn_ctx *ctx, const FusedArgs &a) {
  constexpr size_t lds_bytes = (size_t)FusedLds<HC, C, K, NT, EPI, SP, LF>::FLOATS * 4;
  static_assert(lds_bytes <= 160 * 1024, "one workgroup fits the CU's LDS");
  static std::atomic<uint64_t> configured{0};   // per instantiation: one bit per device (the attribute is per device)
  auto kern = gat_layer_fused_kernel<HC, C, K, NT, EPI, SP, AGG, LF>;
  if (!(configured.load(std::memory_order_relaxed) >> (ctx->device & 63) & 1)) {
    BGNN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    configured.fetch_or(1ull << (ctx->device & 63), std::memory_order_relaxed);
  }
  hipLaunchKernelGGL(kern, dim3(a.tb.n_blocks), dim3(256), lds_bytes, ctx->stream, a);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

// exact-f32 GAT instance: the light form (FusedLds, four workgroups per CU) where it exists and the context asks for it
template <int HC, int K, int NT, int EPI>
static int launch_exact(bgnn_ctx *ctx, const FusedArgs &a) {
  if constexpr (K <= 8 && NT <= 3) {
    if (ctx->opts.fused_light_form) return launch_inst<HC, 64, K, NT, EPI, 0, 0, 1>(ctx, a);
  }
  return launch_inst<HC, 64, K, NT, EPI, 0>(ctx, a);
}

// stencil dispatch: K = 8 and 4 (reference connectivities) on every matrix path; K = 16 ("16-dilated") on the exact-f32
// path (the parity instance, one workgroup per CU) and on the bf16 path (BASELINE config 3)
template <int HC, int NT, int EPI>
static int launch_by_stencil(bgnn_ctx *ctx, const bgnn_graph *g, int sp, const FusedArgs &a) {
  switch (sp) {
    case 0:
      return g->K == 8 ? launch_exact<HC, 8, NT, EPI>(ctx, a) : g->K == 4 ? launch_exact<HC, 4, NT, EPI>(ctx, a)
                                                                           : launch_exact<HC, 16, NT, EPI>(ctx, a);
    case 3:
      return g->K == 8 ? launch_inst<HC, 64, 8, NT, EPI, 3>(ctx, a) : g->K == 4 ? launch_inst<HC, 64, 4, NT, EPI, 3>(ctx, a)
                                                                                 : launch_inst<HC, 64, 16, NT, EPI, 3>(ctx, a);
    default: break;
  }
  if (g->K == 16) return BGNN_ERR_UNSUPPORTED;
  if (sp == 1) return g->K == 8 ? launch_inst<HC, 64, 8, NT, EPI, 1>(ctx, a) : launch_inst<HC, 64, 4, NT, EPI, 1>(ctx, a);
  return g->K == 8 ? launch_inst<HC, 64, 8, NT, EPI, 2>(ctx, a) : launch_inst<HC, 64, 4, NT, EPI, 2>(ctx, a);
}

// Dynamic LDS (bytes per workgroup) of an exact-f32 GAT instance gat_layer_fused_kernel<hc, 64, k, nt, epi, 0, 0, lf>, or -1: for
// tools/kernel_resources.py -- the compiler's resource remarks only know static LDS, and these kernels have none.  Not part of the API.
template <int HC, int K, int NT, int EPI>
static int exact_lds_bytes(int lf) {
  if constexpr (K <= 8 && NT <= 3) {
    if (lf) return FusedLds<HC, 64, K, NT, EPI, 0, 1>::FLOATS * 4;
  }
  return lf ? -1 : FusedLds<HC, 64, K, NT, EPI, 0, 0>::FLOATS * 4;
}
extern "C" int bgnn_internal_fused_lds_bytes(int hc, int k, int nt, int epi, int lf) {
#define BGNN_LDS_CASE(HCV, KV, NTV, EPIV) if (hc == HCV && k == KV && nt == NTV && epi == EPIV) return exact_lds_bytes<HCV, KV, NTV, EPIV>(lf);
#define BGNN_LDS_STENCILS(HCV, NTV, EPIV) BGNN_LDS_CASE(HCV, 4, NTV, EPIV) BGNN_LDS_CASE(HCV, 8, NTV, EPIV) BGNN_LDS_CASE(HCV, 16, NTV, EPIV)
  BGNN_LDS_STENCILS(256, 8, EPI_NEXT) BGNN_LDS_STENCILS(256, 2, EPI_NEXT) BGNN_LDS_STENCILS(128, 4, EPI_NEXT)
  BGNN_LDS_STENCILS(128, 2, EPI_NEXT) BGNN_LDS_STENCILS(64, 2, EPI_NEXT) BGNN_LDS_STENCILS(64, 3, EPI_HEADS)
#undef BGNN_LDS_STENCILS
#undef BGNN_LDS_CASE
  return -1;
}

static bool fused_supported(const bgnn_graph *g, int C) {
  // (compact_edges: slopes + node depths + tile edge lengths, from which the kernels rebuild the canonical attributes; any edge
  //  feature list over distance / depth_difference / slope / zero is built that way -- the caller passes the layer's edge vector
  //  re-expressed over the canonical three, model_canonical_V)
  return g->kind == 0 && (g->K == 4 || g->K == 8 || g->K == 16) && g->n_blocks3 > 0 && C == 64 && g->max_w <= 8192 && g->compact_edges;
}

static void fill_common(FusedArgs &a, const bgnn_graph *g, const BgnnLayer &L, const float *V3, const void *xw, const float *asd, int relu) {
  a.tb.tiles = g->d_tiles; a.tb.items2 = g->uni_h ? nullptr : g->d_items3;
  a.tb.bh = g->bh3; a.tb.bw = g->bw3; a.tb.n_blocks = g->n_blocks3;
  a.node_id = g->d_node_id; a.cell_map = nullptr; a.tile_of_cell = nullptr;
  if (g->d_atlas) {                  // ragged batch: walk the shelf-packed canvas (one "tile") instead of per-grid blocks
    a.tb.tiles = g->d_atlas_tile; a.tb.items2 = nullptr;
    a.tb.bh = g->atlas_h / 8; a.tb.bw = g->atlas_w / 16; a.tb.n_blocks = a.tb.bh * a.tb.bw;
    a.node_id = g->d_atlas; a.cell_map = g->d_cell_of_node; a.tile_of_cell = g->d_atlas_tile_of;
  }
  a.xw = xw; a.asd = asd; a.V = V3 ? V3 : L.V; a.scale = L.scale; a.shift = L.shift;
  a.slope = g->d_slope; a.node_depth = g->d_node_depth; a.tile_dist = g->d_tile_dist;
  a.relu = relu; a.zero_page = g->ctx->zero_page; a.dump = g->ctx->zero_page + 2048;
  a.dbg = BGNN_DIAG ? g->ctx->opts.diag_mask : 0;
  a.stamps = BGNN_DIAG && g->ctx->opts.diag_stamps ? g->ctx->stamps : nullptr;
}

// aggregate of layer L (width HC = L.heads*C) fused with the GEMM of the next layer `Ln`
int launch_fused_layer_next(bgnn_ctx *ctx, const bgnn_graph *g, const BgnnLayer &L, const BgnnLayer &Ln, int C, const float *V3,
                            const void *xw, const float *asd, void *xw_next, float *asd_next) {
  if (!fused_supported(g, C) || (!g->edge_default && !V3)) return BGNN_ERR_UNSUPPORTED;
  const int HC = L.heads * C, NC = Ln.heads * C;
  if (Ln.d_in != HC) return BGNN_ERR_UNSUPPORTED;
  FusedArgs a{};
  fill_common(a, g, L, V3, xw, asd, L.concat ? 1 : 0);
  int split = ctx->opts.matrix_path;                                   // 0 exact, 1 bf16x3, 2 fp16x3 (opt-in), 3 bf16 storage
  if (split == 2 && !Ln.Wsp16) split = 1;                              // a weight beyond float16's range: bf16 split instead
  a.Wt = split == 3 ? Ln.Wbf : split == 2 ? Ln.Wsp16 : split == 1 ? Ln.Wsp : Ln.Wfp;
  a.w_inv = Ln.Wsp16_inv;
  a.att_src = Ln.att_src; a.att_dst = Ln.att_dst; a.out = xw_next; a.asd_out = asd_next;
  a.H2 = Ln.heads; a.C2 = C;
  ProfScope ps(ctx, BGNN_K_FUSED);
  const bool main_shape = (HC == 256 && NC == 256) || (HC == 256 && NC == 64);
  if (split == 3 && !main_shape) return BGNN_ERR_UNSUPPORTED;          // bf16 storage: the default model's shapes only
  if ((split == 1 || split == 2) && (!main_shape || g->K == 16)) { split = 0; a.Wt = Ln.Wfp; }   // other shapes: exact-f32 instances only
  // bf16 storage, 256 -> 256: the two-phase form (three workgroups per CU; bit-identical to the one-phase instance)
  if (split == 3 && HC == 256 && NC == 256 && C == 64 && ctx->opts.bf16_two_phase)
    return g->K == 8 ? launch_two_phase<8>(ctx, a) : g->K == 4 ? launch_two_phase<4>(ctx, a) : launch_two_phase<16>(ctx, a);
#define BGNN_FUSED_CASE(hc, nt) if (HC == hc && NC == nt * 32) return launch_by_stencil<hc, nt, EPI_NEXT>(ctx, g, split, a);
  BGNN_FUSED_CASE(256, 8) BGNN_FUSED_CASE(256, 2)
#undef BGNN_FUSED_CASE
  if (g->K == 16) return BGNN_ERR_UNSUPPORTED;
#define BGNN_FUSED_CASE(hc, nt)                                                                         \
  if (HC == hc && NC == nt * 32)                                                                        \
    return g->K == 8 ? launch_exact<hc, 8, nt, EPI_NEXT>(ctx, a) : launch_exact<hc, 4, nt, EPI_NEXT>(ctx, a);
  BGNN_FUSED_CASE(128, 4) BGNN_FUSED_CASE(128, 2) BGNN_FUSED_CASE(64, 2)
#undef BGNN_FUSED_CASE
  return BGNN_ERR_UNSUPPORTED;
}

// Layer 0 of the bf16 path, aggregate first: h1 [rows][64] bf16 + layer 0's attention dots (launch_extractor_af) -> lin_1's product and dots.
// W0af: per-head images of the folded lin_0 weight; shift_af: L.shift + L.scale * (folded lin_0 bias).  UNSUPPORTED: take the front GEMM.
int launch_fused_layer0_af(bgnn_ctx *ctx, const bgnn_graph *g, const BgnnLayer &L, const BgnnLayer &Ln, int C, const float *V3,
                           const void *h1, const float *asd, const float *W0af, const float *shift_af, void *xw_next, float *asd_next) {
  if (!fused_supported(g, C) || (!g->edge_default && !V3) || !W0af || !shift_af) return BGNN_ERR_UNSUPPORTED;
  if (C != 64 || L.heads != 4 || Ln.heads != 4 || Ln.d_in != 256 || !Ln.Wbf) return BGNN_ERR_UNSUPPORTED;
  FusedArgs a{};
  fill_common(a, g, L, V3, h1, asd, L.concat ? 1 : 0);
  a.shift = shift_af;
  a.Wt = Ln.Wbf; a.W0af = W0af;
  a.att_src = Ln.att_src; a.att_dst = Ln.att_dst; a.out = xw_next; a.asd_out = asd_next;
  a.H2 = Ln.heads; a.C2 = C;
  ProfScope ps(ctx, BGNN_K_FUSED);
  return g->K == 8 ? launch_two_phase<8, true>(ctx, a) : g->K == 4 ? launch_two_phase<4, true>(ctx, a) : launch_two_phase<16, true>(ctx, a);
}

// One layer of a plain backbone (GCN / GraphSAGE / GIN) as aggregate -> GEMM -> post-op in ONE launch (kernel template AGG = mode):
// x [rows][C] -> out [rows][C].  `Wfp` = the layer's W^T ([C][C]; GraphSAGE: the stacked [2 C][C]) in the column-permuted image;
// post_scale / post_shift [C] and post_relu: the per-column epilogue; dinv [rows] (GCN only).  BGNN_ERR_UNSUPPORTED: take the plain kernels.
int launch_fused_plain_layer(bgnn_ctx *ctx, const bgnn_graph *g, int mode, int C, const float *x, const float *dinv, const float *Wfp,
                             const float *ones, const float *post_scale, const float *post_shift, int post_relu, float *out) {
  if (!fused_supported(g, C) || !Wfp || mode < 1 || mode > 3) return BGNN_ERR_UNSUPPORTED;
  FusedArgs a{};
  BgnnLayer L{};
  L.V = nullptr; L.scale = const_cast<float *>(ones); L.shift = ctx->zero_page;   // pre-GEMM epilogue: the identity
  fill_common(a, g, L, nullptr, x, dinv, 0);
  a.Wt = Wfp; a.att_src = post_scale; a.att_dst = post_shift; a.out = out; a.asd_out = nullptr;
  a.H2 = 1; a.C2 = C; a.relu2 = post_relu; a.self_loops = g->include_self_loops;
  ProfScope ps(ctx, BGNN_K_FUSED);
#define BGNN_PLAIN_CASE(M, HCV)                                                                                   \
  if (mode == M)                                                                                                  \
    return g->K == 8 ? launch_inst<HCV, 64, 8, 2, EPI_NEXT, 0, M>(ctx, a) : g->K == 4 ? launch_inst<HCV, 64, 4, 2, EPI_NEXT, 0, M>(ctx, a) \
                                                                                       : launch_inst<HCV, 64, 16, 2, EPI_NEXT, 0, M>(ctx, a);
  BGNN_PLAIN_CASE(1, 64) BGNN_PLAIN_CASE(2, 128) BGNN_PLAIN_CASE(3, 64)
#undef BGNN_PLAIN_CASE
  return BGNN_ERR_UNSUPPORTED;
}

// Will launch_fused_layer_heads take this (model, graph)?  bgnn_infer_tiles asks BEFORE the forward: only then can the forward run
// without per-node outputs (the last launch writes the grids itself).  Asked after the fact -- round 3 -- every model the fused tail
// does not cover (GCN / GraphSAGE / GIN, other head counts) ran its whole forward twice.
bool fused_heads_available(const bgnn_ctx *ctx, const bgnn_graph *g, const bgnn_model *m) {
  if (!ctx->opts.fused || m->desc.gnn_type != BGNN_GNN_GAT || m->layers.empty()) return false;
  const BgnnLayer &L = m->layers.back();
  return fused_supported(g, m->desc.hidden) && L.heads == 1 && m->desc.num_classes <= 4 && m->head_hidden_total == 96 && m->hd_tab &&
         (m->desc.predict_correction ? 3 : 2) * (m->desc.hidden / 2) <= 96;
}

// aggregate of the LAST layer (HC = C, one head) fused with the heads (+ grids)
int launch_fused_layer_heads(bgnn_ctx *ctx, const bgnn_graph *g, const bgnn_model *m, const BgnnLayer &L, int C, const float *V3,
                             const void *xw, const float *asd, float thr_auto, float thr_review, float norm_floor,
                             const bgnn_outputs *o, float *cls_grid, float *conf_grid, float *corr_grid) {
  if (!fused_supported(g, C) || (!g->edge_default && !V3) || L.heads != 1 || m->desc.num_classes > 4 || m->head_hidden_total != 96 || !m->hd_tab ||
      (m->desc.predict_correction ? 3 : 2) * (C / 2) > 96 || o->hidden)
    return BGNN_ERR_UNSUPPORTED;
  FusedArgs a{};
  fill_common(a, g, L, V3, xw, asd, L.concat ? 1 : 0);
  int split = ctx->opts.matrix_path;
  if (split == 2 && !m->hd_W0sp16) split = 1;
  if ((split == 1 || split == 2) && g->K == 16) split = 0;
  a.Wt = split == 3 ? m->hd_W0bf : split == 2 ? m->hd_W0sp16 : split == 1 ? m->hd_W0sp : m->hd_W0fp;
  a.w_inv = m->hd_W0sp16_inv;
  a.hd_tab = m->hd_tab;
  a.local_std = g->d_local_std;
  a.classes = m->desc.num_classes; a.hh = C / 2; a.has_corr = m->desc.predict_correction;
  a.thr_auto = thr_auto; a.thr_review = thr_review; a.norm_floor = norm_floor; a.o = *o;
  a.cls_grid = cls_grid; a.conf_grid = conf_grid; a.corr_grid = corr_grid;
  ProfScope ps(ctx, BGNN_K_FUSED);
  return launch_by_stencil<64, 3, EPI_HEADS>(ctx, g, split, a);
}

}  // namespace bgnn
