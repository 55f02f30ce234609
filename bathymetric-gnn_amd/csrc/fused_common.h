// Shared device code of the fused GAT layer kernels (gat_layer_fused.hip: the one-phase kernel; gat_layer_bf16_2p.hip: the two-phase
// form of the bf16 256 -> 256 instance): the launch arguments, the asm LDS accessors and waits, the MFMA tile helpers, the halo
// geometry, and the pieces both kernels run -- the block prologue (HaloPrologue), phase A's attention coefficients, the bf16
// aggregation window, BatchNorm / ReLU on a slab's registers and the bf16 tile-pair store patch.  One piece of host code rides along:
// launch_with_lds, the launch both files' launchers go through.
#pragma once
#include <stdlib.h>
#include <algorithm>
#include <atomic>
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

// The two-phase form of the bf16 256 -> 256 instance (gat_layer_bf16_2p.hip): stencil K = 4 / 8 / 16; af: layer 0 "aggregate first"
int launch_two_phase(bgnn_ctx *ctx, int K, bool af, const FusedArgs &a);

// "Set the dynamic-LDS attribute once per device, then launch" of one kernel instance.  `configured` is that instance's own word:
// one bit per device (the attribute is per device).
template <typename Kern>
static inline int launch_with_lds(bgnn_ctx *ctx, Kern kern, std::atomic<uint64_t> &configured, size_t lds_bytes, const FusedArgs &a) {
  if (!(configured.load(std::memory_order_relaxed) >> (ctx->device & 63) & 1)) {
    BGNN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    configured.fetch_or(1ull << (ctx->device & 63), std::memory_order_relaxed);
  }
  hipLaunchKernelGGL(kern, dim3(a.tb.n_blocks), dim3(256), lds_bytes, ctx->stream, a);
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}

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
template <int NT, int T0>
struct Bf16Tiles {
  static constexpr int NB = NT - T0 < 4 ? NT - T0 : 4;
  __device__ static __forceinline__ void load(f32x4 (&w)[4], uint32_t wh) {
    if constexpr (NB > 0) w[0] = lds_read4<(T0 + 0) * 1024>(wh);
    if constexpr (NB > 1) w[1] = lds_read4<(T0 + 1) * 1024>(wh);
    if constexpr (NB > 2) w[2] = lds_read4<(T0 + 2) * 1024>(wh);
    if constexpr (NB > 3) w[3] = lds_read4<(T0 + 3) * 1024>(wh);
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
// the neighbourhood sum of one slab: every block of the wave's window (ta, tb: the transposed reads' addresses; bq: the dense rows')
template <int K>
__device__ __forceinline__ void aggregate_window(f32x16 &d, uint32_t ta, uint32_t tb, uint32_t bq, int hl) {
  using Win = AggWindow<K>;
  if constexpr (Win::NKB == 8) {
    agg_blocks<0, 4, true, false>(d, ta, tb, bq, hl);
    agg_blocks<4, 4, false, Win::TAIL_BEYOND_PITCH>(d, ta, tb, bq, hl);
  } else {
    static_assert(Win::NKB == 5, "window blocks");
    agg_blocks<0, 3, true, false>(d, ta, tb, bq, hl);
    agg_blocks<3, 2, false, false>(d, ta, tb, bq, hl);
  }
}

// ---- the pieces both kernels run ---------------------------------------------------------------------------------------------

// 4 waves.  Wave w: cells 32w..32w+31 of the block (two tile rows).  Lane (r, hl): node r of the group, k-half hl.
template <int K>
struct LaneCoords {
  int tid, lane, wave, r, hl, cell, tr, tc, self_idx;
  __device__ __forceinline__ LaneCoords() {
    using Geo = FusedGeom<K>;
    tid = threadIdx.x; lane = tid & 63;
    // the wave index as a SCALAR: LDS-DMA destinations (M0) and the "does this wave move piece q" tests then stay on the scalar
    // unit instead of costing a v_readfirstlane / exec-mask sequence per DMA in the slab loop
    wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    r = lane & 31; hl = lane >> 5;
    cell = wave * 32 + r;                                // block-local cell of this lane
    tr = cell / TILE_W; tc = cell % TILE_W;
    self_idx = (tr + Geo::R) * Geo::HW + tc + Geo::R;
  }
};

// Block prologue: two dependent rounds of loads with everything of a round in flight together --
//   round 1: node id of this thread's halo row (HR <= NTH: one row per thread), of this lane's own cell, and of
//            the <= NPIECE halo rows whose chunks this thread moves by DMA (CPR lanes share a row);
//   -> slab 0's DMA is issued straight from those registers (no LDS round trip, no barrier);
//   round 2: alpha_src and node depth of the halo row; the own node's K slopes, alpha_dst (heads hl, hl + 2, ...) and the tile's edge lengths
//            -- consumed in phase A, so their latency hides behind the halo bookkeeping.
// The kernel calls the steps in this order: round1 | (its own loads) | validity | gutter_only | round2 | dma_bases | write_halo_tables |
// touch_round2 | issue_slab(0) | wait_lgkm0 + raw barrier; the waits depend on that order.
// Round 2's values (eraw, adv, hasv, hdep, tdist) are the KERNEL's locals, handed to round2 / write_halo_tables / touch_round2 by
// reference: as members of this struct they cost the operand-split instances with a narrow next stage two VGPRs and 30-40
// instructions (register copies on the slab loop's back edge; bf16x3 fused time +0.4 %).  NSLAB: slab requests per block.
// (Pointers into LDS go to these functions BY REFERENCE, as a lambda's capture would take them: passed by value, hipcc no longer folded
//  lds_addr() of the same pointer to a constant afterwards -- a null test and a shared-base round trip per table address, ~30 scalar
//  instructions per block.)
// CPR: 16-byte chunks per row of the slab image (ROWB = 16 CPR bytes); SRC_ROWB: bytes of a source row in HBM; H: heads;
// AGG: FusedLds (0: GAT form of round 2); HS / DB32: the light form's swizzle / its 32-bit DMA bases (gat_layer_fused.hip).
template <int K, int CPR, int SRC_ROWB, int H, int AGG, bool HS, bool DB32, int NSLAB>
struct HaloPrologue {
  using Geo = FusedGeom<K>;
  static constexpr int NTH = 256, HR = Geo::HR, HW_ = Geo::HW, RAD = Geo::R;
  static constexpr int ROWB = CPR * 16;
  static_assert(NSLAB * ROWB <= 4096, "the zero page covers a whole block's worth of slab offsets");
  static constexpr int NHL = (H + 1) / 2;                // heads per lane
  static constexpr int NPIECE = (HR * CPR + NTH - 1) / NTH;
  static_assert(HR <= NTH, "one halo row per thread");
  static_assert((NPIECE - 2) * NTH + NTH - 64 < HR * CPR, "every wave moves NPIECE or NPIECE - 1 pieces");
  // DMA piece p moves chunk (p * NTH + tid) % CPR of halo row (p * NTH + tid) / CPR: the row advances by NTH / CPR per piece
  static_assert(NTH % CPR == 0, "pieces advance by whole halo rows");
  static constexpr int RSTEP = NTH / CPR, RSTEP_R = RSTEP / HW_, RSTEP_C = RSTEP % HW_;

  uint32_t uw, uh;
  int r0h, c0h;                                          // tile coordinates of the halo's first cell
  int gr_h, gc_h, gr_m, gc_m, raw_h, raw_m, tile_m;
  int drow[NPIECE], prow_r[NPIECE], prow_c[NPIECE];
  int hid_v, my_pre;
  const char *xbase, *zp;
  const char *dbase[NPIECE];
  uint32_t doff[NPIECE];

  __device__ __forceinline__ bool in_tile(int gr, int gc) const { return (uint32_t)gr < uh && (uint32_t)gc < uw; }

  // Round 1 is ONE round: every load is unconditional (coordinates clamped into the tile, validity applied to the value
  // afterwards), so nothing is exec-masked, no branch separates the loads and the compiler keeps all of them in flight behind
  // a single wait.  (With `if (inside) id = node_id[..]` per load, hipcc waited for the halo row's id, then for the own cell's,
  // then for the DMA rows': three dependent trips to L2 before round 2 could start.)
  // (Integer work is kept short on purpose: on the exact path this wave's SIMD partners stream f32 MFMAs, and every VALU
  //  instruction of the prologue waits for a gap between two of them -- ~50-100 cycles each by the per-phase timers.  Cell indices
  //  are 32-bit (a batch has < 2^30 cells), the node-id table is addressed base + 32-bit offset, the DMA pieces' halo rows advance
  //  by a constant step instead of being divided out, and validity is one unsigned compare per coordinate.)
  __device__ __forceinline__ void round1(const FusedArgs &a, const BlockPos &pos, const LaneCoords<K> &ln) {
    const uint32_t cbase = (uint32_t)pos.cell_off;
    uw = (uint32_t)pos.w; uh = (uint32_t)pos.h;
    const int h1 = pos.h - 1, w1 = pos.w - 1;
    auto cell_index = [&](int gr, int gc) -> uint32_t {    // clamped into the tile: always a readable cell
      const int r_ = max(0, min(gr, h1)), c_ = max(0, min(gc, w1));
      return cbase + __umul24((uint32_t)r_, uw) + (uint32_t)c_;      // (r, w < 2^14)
    };
    // node id of a cell: table base (uniform) + 32-bit BYTE offset -> the load's saddr + voffset form, no 64-bit address arithmetic
    auto node_at = [&](uint32_t cell) -> int {
      return *reinterpret_cast<const int *>(reinterpret_cast<const char *>(a.node_id) + (cell << 2));
    };
    const int hr_t = ln.tid / HW_, hc_t = ln.tid - hr_t * HW_;
    r0h = pos.r0 - RAD; c0h = pos.c0 - RAD;              // (uniform: once, on the scalar unit)
    gr_h = r0h + hr_t; gc_h = c0h + hc_t;
    gr_m = pos.r0 + ln.tr; gc_m = pos.c0 + ln.tc;
    raw_h = node_at(cell_index(gr_h, gc_h));
    const uint32_t cell_m = cell_index(gr_m, gc_m);
    raw_m = node_at(cell_m);
    // whose edge lengths: the block's tile, or (canvas walk) the grid this cell belongs to -- a canvas array read beside the ids
    tile_m = pos.tile;
    if (a.tile_of_cell) {                                 // (only cells that hold a node have an entry: the table is not cleared)
      const int t_ = *reinterpret_cast<const int *>(reinterpret_cast<const char *>(a.tile_of_cell) + (cell_m << 2));
      tile_m = raw_m >= 0 ? t_ : 0;
    }
    const int row0 = ln.tid / CPR;
    int pr = row0 / HW_, pc = row0 - pr * HW_;
#pragma unroll
    for (int p = 0; p < NPIECE; ++p) {
      prow_r[p] = pr; prow_c[p] = pc;
      drow[p] = node_at(cell_index(r0h + pr, c0h + pc));
      pr += RSTEP_R; pc += RSTEP_C;
      if (pc >= HW_) { pc -= HW_; pr += 1; }
    }
  }
  // validity (ids < 0 in the table encode invalid cells); `no_self`: the diagnostic build's "no node of my own" switch
  __device__ __forceinline__ void validity(const LaneCoords<K> &ln, bool no_self) {
    hid_v = (ln.tid < HR && in_tile(gr_h, gc_h) && raw_h >= 0) ? raw_h : -1;
    my_pre = (!no_self && in_tile(gr_m, gc_m)) ? raw_m : -1;
#pragma unroll
    for (int p = 0; p < NPIECE; ++p) {
      // (measured with ids COMPUTED instead of loaded, all-valid tiles: 0.3 % (exact) / 2 % (bf16) -- the id round is already hidden)
      const bool row_ok = (p + 1) * NTH <= HR * CPR || prow_r[p] < FT_H + 2 * RAD;       // rows past the halo: last piece only
      if (!(row_ok && in_tile(r0h + prow_r[p], c0h + prow_c[p]))) drow[p] = -1;
    }
  }
  // canvas walk (wave-uniform test): does the block hold only gutter / free space?  (Contains a __syncthreads.)
  __device__ __forceinline__ bool gutter_only(const LaneCoords<K> &ln, int *const &minid) const {
    // (not __syncthreads_or: its library reduction brings 256 bytes of static LDS in front of the dynamic region)
    const bool wave_any = __builtin_amdgcn_ballot_w64(my_pre >= 0) != 0;
    if (ln.lane == 0) minid[ln.wave] = wave_any ? 1 : 0;
    __syncthreads();
    return (minid[0] | minid[1] | minid[2] | minid[3]) == 0;
  }
  // Round 2, complete BEFORE slab 0's DMA is queued (hipcc only ever waits vmcnt(0) with an LDS-DMA in flight): alpha_src of
  // this thread's halo row (and its node's depth); the own node's slopes and alpha_dst (heads hl, hl + 2, ...).  Unconditional as well:
  // rows without a node read row 0 and are masked afterwards.
  // Edge attributes come COMPACT (graph_build.hip, FeatureArgs): the K slopes of the own node, the node depths of the halo rows
  // (depth difference = one float32 subtraction, as the feature kernel takes it) and the three edge lengths of the tile -- a third
  // of the bytes and registers of the [K][3] block this round used to load (k = 16: 64 + 4 + 16 instead of 192 bytes per node).
  __device__ __forceinline__ void round2(const FusedArgs &a, const LaneCoords<K> &ln, float (&eraw)[K], float (&adv)[NHL], float (&hasv)[H], float &hdep,
                                         float4 &tdist) const {
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
        const int hh = ln.hl + i * 2;
        adv[i] = hh < H ? a.asd[mrow * 2 * H + H + hh] : 0.0f;
      }
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
  __device__ static __forceinline__ int swz(int row) {
    return HS ? (((row % HW_) >> 2) & 1) | (((row / HW_) & 1) << 1) : CPR == 8 ? ((row % HW_) >> 1) & 7 : (row >> 2) & 3;
  }
  // Per piece ONE 64-bit source base for the whole block (a single 32 x 32 -> 64-bit multiply-add off the table's base; an earlier
  // version kept 32-bit offsets relative to the smallest id of the wave, which cost a six-step wave reduction per block): rows
  // without a node read the context's zero page, which holds more than NSLAB * ROWB zero bytes, so that they can advance by ROWB
  // per slab exactly like real rows (no per-slab select) and EVERY wave issues a fixed number of slab pieces: the counted
  // waits of the slab loop can leave exactly the next slab in flight.
  // DB32 (light form, one-head sources: the heads launch): the bases as 32-bit offsets in 16-byte units (64-channel rows: 2^28 nodes),
  // ~0 = the zero page, widened at each request -- three registers less across the whole block, which is what keeps this instance free of
  // scratch at 128 registers; a few vector instructions per half-step, and it has four of them
  __device__ __forceinline__ void dma_bases(const FusedArgs &a, const LaneCoords<K> &ln) {
    xbase = reinterpret_cast<const char *>(a.xw);
    zp = reinterpret_cast<const char *>(a.zero_page);
    const int cc = ln.tid % CPR;
#pragma unroll
    for (int p = 0; p < NPIECE; ++p) {
      const int row = prow_r[p] * HW_ + prow_c[p];
      const int c = cc ^ (HS ? ((prow_c[p] >> 2) & 1) | ((prow_r[p] & 1) << 1) : swz(row));   // (HS: swz(row) without the division)
      dbase[p] = drow[p] >= 0 ? xbase + ((uint64_t)(uint32_t)drow[p] * (uint32_t)SRC_ROWB + (uint32_t)(c * 16)) : zp;
      doff[p] = drow[p] >= 0 ? (uint32_t)drow[p] * (uint32_t)(SRC_ROWB / 16) + (uint32_t)c : ~0u;
    }
  }
  // the slab image `dst` <- bytes sb .. sb + ROWB of every halo row's source (sb wave-uniform)
  __device__ __forceinline__ void issue_slab(float *const &dst, int sb, const LaneCoords<K> &ln) const {
#pragma unroll
    for (int p = 0; p < NPIECE; ++p) {
      if ((p + 1) * NTH <= HR * CPR || p * NTH + ln.tid < HR * CPR) {        // (only the last piece is partial: compile-time true before)
        uint32_t dof = doff[p];
        if constexpr (DB32) asm volatile("" : "+v"(dof));    // (opaque: the widened base must not be hoisted back out of the loop)
        const char *src = DB32 ? (dof != ~0u ? xbase + ((uint64_t)dof << 4) : zp) : dbase[p];
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(src + sb),
                                         (__attribute__((address_space(3))) void *)(dst + (p * NTH + ln.wave * 64) * 4), 16, 0, 0);
      }
    }
  }
  // Round 2's values go to the halo tables first -- hipcc waits vmcnt(0) for them, which must not include slab 0's DMA -- and
  // only then is slab 0 requested: it is in flight during the whole of phase A, whose LDS reads are asm (no compiler wait).
  __device__ __forceinline__ void write_halo_tables(const LaneCoords<K> &ln, const float (&hasv)[H], const float &hdep, int *const &hid,
                                                    float *const &has, float *const &hdp) const {
    if (ln.tid < HR) {
      hid[ln.tid] = hid_v;
#pragma unroll
      for (int hh = 0; hh < H; ++hh) has[hh * HR + ln.tid] = hid_v >= 0 ? hasv[hh] : (AGG == 0 ? -__builtin_inff() : 0.0f);   // (-inf: an absent source drops out of the softmax)
      hdp[ln.tid] = hid_v >= 0 ? hdep : 0.0f;
    }
  }
  // (phase A's register operands are complete as well before the DMA is queued: no wait behind it later)
  // (the table writes sit under `tid < HR`: a wave that skips them has not waited yet -- touch every round-2 register, and whatever
  //  else the kernel loaded beside them: `more`)
  template <typename... F>
  __device__ __forceinline__ void touch_round2(const float (&eraw)[K], const float (&adv)[NHL], const float (&hasv)[H], const float &hdep,
                                               const float4 &tdist, F... more) const {
    float sink = 0.0f;
#pragma unroll
    for (int i = 0; i < NHL; ++i) sink += adv[i];
#pragma unroll
    for (int i = 0; i < K; ++i) sink += eraw[i];
#pragma unroll
    for (int hh = 0; hh < H; ++hh) sink += hasv[hh];
    sink += ((hdep + tdist.x + tdist.y + tdist.z) + ... + more);
    asm volatile("" ::"v"(sink));
  }
};

// ---- phase A, GAT: the attention coefficients of this lane's heads (hl, hl + 2, ...: the two lanes that share a cell take the heads
// round-robin) out of the halo tables -- the cell's node ids of the stencil sources once, alpha_src per head; then the
// head-independent edge terms once and the lane's heads -- both at once, as packed f32 halves, when it owns two (gat_tile_common.h).
// hid0 / has0: LDS addresses of the id and alpha_src tables; hdp: the depth table; self_a: the cell's halo row.
template <int K, int H>
__device__ __forceinline__ void gat_coefficients(uint32_t hid0, uint32_t has0, const float *const &hdp, int self_a, int hl, const float (&eraw)[K],
                                                 const float (&adv)[(H + 1) / 2], const float4 &tdist, const float (&vpre)[(H + 1) / 2][3],
                                                 float (&part)[(H + 1) / 2][K + 1]) {
  constexpr int NHL = (H + 1) / 2, HW_ = FusedGeom<K>::HW, HR = FusedGeom<K>::HR;
  using S = HaloSlot<K, HW_>;
  int nb[K];
  float hs[NHL][K + 1];
  halo_ids<K, HW_>(hid0 + (uint32_t)(self_a - S::MAXOFF) * 4u, nb, std::make_integer_sequence<int, K>{});
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
}
template <int NHL, int K1>
__device__ __forceinline__ void zero_coefficients(float (&part)[NHL][K1]) {        // a cell without a node
#pragma unroll
  for (int i = 0; i < NHL; ++i)
#pragma unroll
    for (int b = 0; b < K1; ++b) part[i][b] = 0.0f;
}
template <int K>                                           // bf16 storage: kept in registers as bf16 pairs until the head's slabs come up (densify)
__device__ __forceinline__ void pack_coefficients(const float (&part)[K + 1], uint32_t (&apk)[(K + 2) / 2]) {
#pragma unroll
  for (int b = 0; b <= K; b += 2) apk[b / 2] = pack_bf16x2(part[b], b + 1 <= K ? part[b + 1] : 0.0f);
}

// bf16 storage: head hd's coefficients become the wave's dense [32 cells][window rows] matrix at dn0 (AggWindow).  Wave-private, and
// LDS operations of one wave complete in order: no barrier, the aggregation's reads simply follow the writes.
// The matrix is cleared ONCE (hd == 0 && clear): a cell's K + 1 window positions depend on its place in the block only, so every
// later head overwrites exactly the entries head 0 wrote (absent sources with a zero coefficient) -- 8 x ds_write_b128 per head less.
template <int K, int NHL>
__device__ __forceinline__ void densify(int hd, bool clear, uint32_t dn0, int wbase, int lane, int r, int hl, int self_idx,
                                        const uint32_t (&apk)[NHL][(K + 2) / 2]) {
  using Win = AggWindow<K>;
  using Off = StencilOffsets<K>;
  constexpr int HW_ = FusedGeom<K>::HW;
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
      const int wp = wself - off;
      const uint32_t ad = rowb + (uint32_t)wp * 2u;
      const uint32_t v = NHL > 1 && (hd >> 1) ? apk[NHL > 1 ? 1 : 0][b / 2] : apk[0][b / 2];
      if (b & 1) asm volatile("ds_write_b16_d16_hi %0, %1" ::"v"(ad), "v"(v) : "memory");
      else asm volatile("ds_write_b16 %0, %1" ::"v"(ad), "v"(v) : "memory");
    }
  }
}

// layer epilogue on a slab's 16 values per lane: (+bias, BatchNorm) folded, ReLU -> h_{l+1}, in registers.  cp: LDS address of the
// lane's first scale chunk (the shifts HC floats behind; the lane's chunks are 32 bytes apart: the exact / bf16 channel ownership).
__device__ __forceinline__ void relu4(f32x4 &v) {         // one v_max_f32 each (the C select / fmax forms add a canonicalising one)
  asm("v_max_f32 %0, 0, %0" : "+v"(v.x)); asm("v_max_f32 %0, 0, %0" : "+v"(v.y));
  asm("v_max_f32 %0, 0, %0" : "+v"(v.z)); asm("v_max_f32 %0, 0, %0" : "+v"(v.w));
}
template <int HC>
__device__ __forceinline__ void bn_relu(f32x4 (&g)[4], uint32_t cp, int relu) {
#pragma unroll
  for (int jp = 0; jp < 2; ++jp) {                // two chunks at a time (register budget)
    f32x4 sc0, sc1, sh0, sh1;
    if (jp == 0) { sc0 = lds_read4<0>(cp); sc1 = lds_read4<32>(cp); sh0 = lds_read4<HC * 4>(cp); sh1 = lds_read4<HC * 4 + 32>(cp); }
    else { sc0 = lds_read4<64>(cp); sc1 = lds_read4<96>(cp); sh0 = lds_read4<HC * 4 + 64>(cp); sh1 = lds_read4<HC * 4 + 96>(cp); }
    lds_reads_done();
    g[2 * jp] = g[2 * jp] * sc0 + sh0;
    g[2 * jp + 1] = g[2 * jp + 1] * sc1 + sh1;
  }
  if (relu) {
#pragma unroll
    for (int j = 0; j < 4; ++j) relu4(g[j]);
  }
}
// the light form's half-step: chunks jA, jA + 1 only (cp: the half's first scale chunk)
template <int HC, int JA>
__device__ __forceinline__ void bn_relu_half(f32x4 (&g)[4], uint32_t cp, int relu) {
  const f32x4 sc0 = lds_read4<0>(cp), sc1 = lds_read4<32>(cp), sh0 = lds_read4<HC * 4>(cp), sh1 = lds_read4<HC * 4 + 32>(cp);
  lds_reads_done();
  g[JA] = g[JA] * sc0 + sh0;
  g[JA + 1] = g[JA + 1] * sc1 + sh1;
  if (relu) {
#pragma unroll
    for (int j = JA; j <= JA + 1; ++j) relu4(g[j]);
  }
}

// bf16 store patch of a wave: TWO 32 x 32 tiles side by side, already as bf16 -- [32 rows][128 B], 16-byte chunk c of row r at chunk
// c ^ (r & 7), the two 8-byte halves of a chunk swapped on rows with bit 3 set: conflict-free for the ds_write_b64 (16 consecutive
// lanes over 32 banks) and for the ds_read_b128 lane groups (MI355X_MICROARCH.md), half the LDS write bytes and read-backs of
// the float32 patch, and whole 128-byte lines per stored row instead of two 64-byte halves.
// write: lane (r, hl)'s four values of register group g (columns 8 g + 4 hl ..) of the pair's tile tt
__device__ __forceinline__ void tile_pair_write(char *const &patch, int r, int hl, int tt, int g, const float4 &v) {
  typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
  bf16x4 o;
  o[0] = (__bf16)v.x; o[1] = (__bf16)v.y; o[2] = (__bf16)v.z; o[3] = (__bf16)v.w;
  char *pb = patch + r * 128 + ((hl ^ ((r >> 3) & 1)) << 3);
  *reinterpret_cast<bf16x4 *>(pb + (((tt * 4 + g) ^ (r & 7)) << 4)) = o;
}
// read back: 16 bytes (lane & 7) of row (lane >> 3) + 8 k -- (row >> 3) & 1 == k & 1, the half swap is compile-time
__device__ __forceinline__ uint4 tile_pair_row_segment(const char *const &patch, int lane, int k) {
  const int row = (lane >> 3) + 8 * k;
  uint4 q = *reinterpret_cast<const uint4 *>(patch + row * 128 + (((lane & 7) ^ (row & 7)) << 4));
  if (k & 1) q = make_uint4(q.z, q.w, q.x, q.y);
  return q;
}

}  // namespace bgnn
