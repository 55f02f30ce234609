// Fused GAT layer for stencil graphs (gfx950):  aggregate_l  ->  BN/ReLU  ->  GEMM_{l+1}
//
// This file: the one-phase kernel gat_layer_fused_kernel, its LDS budget FusedLds, the launchers and the four host entry points.
// gat_layer_bf16_2p.hip: the two-phase form of the bf16 256 -> 256 instance (TwoPhaseLds, its kernel, launch_two_phase).
// fused_common.h: what both kernels use -- FusedArgs, the asm LDS accessors and waits, the MFMA tile helpers, the halo geometry, the
// block prologue (HaloPrologue), phase A's GAT coefficients, the bf16 aggregation window, BatchNorm / ReLU on a slab, the bf16 store patch.
//
// One workgroup (256 threads = 4 waves; one to four workgroups per CU, by the instance: FusedLds::PER_CU) owns an 8x16 block of cells of one tile and
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
#include "fused_common.h"

namespace bgnn {

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
  // (RING 1.  A RING 2 -- two full 32-row W chunks, two barriers per slab instead of five -- measured within noise of it and of the
  //  single image: DESIGN.md)
  static constexpr int RING = SP == 3 && NT == 8 && EPI == EPI_NEXT ? 1 : 0;
  static constexpr bool DBUF = RING == 1;
  static constexpr int SLAB = DBUF ? 2 * SLAB1 : SLAB1;
  static constexpr int WBUF = 2 * WHalf<NT, SP>::BYTES / 4;
  // the epilogue's four wave-private 32 x 36 store patches reuse slab (+ wbuf)
  static constexpr int PATCH_PAD = EPI == EPI_NEXT && SLAB + WBUF < 4 * 32 * TILED_PITCH ? 4 * 32 * TILED_PITCH - SLAB - WBUF : 0;
  static constexpr int HEADW = 96 + 6 * 32 + 8;          // heads: first-layer biases | second-layer rows (<= 4 classes + 2) | their biases
  // bf16 storage path, two space savers (so that its narrow instances fit three workgroups per CU):
  //  * the halo's alpha_src table (phase A only) lives in the dense-alpha region, which is first written after phase A;
  //  * the heads' small weight table (final epilogue only) is parked in the slab region once the last slab has been gathered.
  //  * DBUF: the halo ids live there as well (the epilogue takes its row ids from the lanes' own registers), and the next layer's
  //    att vectors are DMA'd into the free slab buffer during the last slab.
  static constexpr bool HAS_IN_ALPHA = SP == 3, HEADW_LATE = SP == 3 && EPI == EPI_HEADS, HID_IN_ALPHA = DBUF, ATT_LATE = DBUF;
  // (floats) past the four store patches, which start at image A, and past the 8 rows (128 floats) image A's last MFMA over-reads
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

// Phase A of the plain backbones (AGG 1 GCN, 2 GraphSAGE, 3 GIN; below): the coefficient of in-edge b (b = K: the node itself), in the
// order the gather sums them -- the order of neighbor_reduce.hip (slots ascending, self last).  One (virtual) head per lane; GCN reads
// dinv where GAT reads alpha_src.  The GAT sibling is gat_coefficients (fused_common.h).
template <int K, int AGG>
__device__ __forceinline__ void plain_coefficients(uint32_t hid0, uint32_t has0, int self_a, int hl, int self_loops, float (&part)[K + 1]) {
  constexpr int HW_ = FusedGeom<K>::HW;
  using S = HaloSlot<K, HW_>;
  int nb[K];
  float hs[K + 1];
  halo_ids<K, HW_>(hid0 + (uint32_t)(self_a - S::MAXOFF) * 4u, nb, std::make_integer_sequence<int, K>{});
  if constexpr (AGG == 1) halo_alpha_src<1, K, HW_>(has0 + (uint32_t)(self_a - S::MAXOFF) * 4u, hs, std::make_integer_sequence<int, K>{});
  lds_reads_done();
  int cnt = self_loops ? 1 : 0;
#pragma unroll
  for (int b = 0; b < K; ++b) cnt += nb[b] >= 0 ? 1 : 0;
  const float inv = 1.0f / (float)(cnt > 0 ? cnt : 1);
#pragma unroll
  for (int b = 0; b <= K; ++b) {
    const bool self = b == K, on = self || nb[b < K ? b : 0] >= 0;
    float c;
    if constexpr (AGG == 1) c = self ? hs[K] * hs[K] : (on ? hs[b] * hs[K] : 0.0f);      // dinv[j] * dinv[i]
    else if constexpr (AGG == 2) c = hl == 0 ? ((self ? self_loops != 0 : on) ? inv : 0.0f) : (self ? 1.0f : 0.0f);
    else c = self ? (self_loops ? 2.0f : 1.0f) : (on ? 1.0f : 0.0f);
    part[b] = c;
  }
}

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
  constexpr bool DBUF = Lds::DBUF;
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
  const LaneCoords<K> ln;
  const int tid = ln.tid, lane = ln.lane, wave = ln.wave, r = ln.r, hl = ln.hl, cell = ln.cell, tr = ln.tr, tc = ln.tc, self_idx = ln.self_idx;

  // W rows of slab 0 depend on nothing: first in the VM queue.
  stage_w_half<NT, SP>(a.Wt, wbuf, 0, wave, lane);
  stage_w_half<NT, SP>(a.Wt, wbuf, 1, wave, lane);

  // The block prologue (fused_common.h, HaloPrologue) with this kernel's extras between its steps: the W halves above, the scale /
  // shift and edge vectors beside round 1, the stamps, and the drain in front of the early exit.
  // (light form, one-head sources -- the heads launch: 32-bit DMA bases, see HaloPrologue::dma_bases)
  constexpr bool DB32 = HS && H == 1;
  using Pro = HaloPrologue<K, CPR, SRCW * XB, H, AGG, HS, DB32, HS ? 2 * NSLAB : NSLAB>;
  constexpr int NHL = Pro::NHL, NPIECE = Pro::NPIECE;
  static_assert(AGG == 0 || NHL == 1, "plain backbones: one (virtual) head per lane");
  Pro pro;
  pro.round1(a, pos, ln);
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
  pro.validity(ln, DBG(32));
#if BGNN_DIAG
  if (a.stamps) asm volatile("" ::"v"(pro.hid_v), "v"(pro.my_pre), "v"(pro.drow[0]));
#endif
  BGNN_STAMP(10)   // round 1 arrived
  if (a.cell_map) {                  // canvas walk (wave-uniform test): blocks that hold only gutter / free space leave here
    if (pro.gutter_only(ln, minid)) {
      __builtin_amdgcn_s_waitcnt(0);   // the W DMAs land in this WG's LDS: drain them before the LDS can be handed on
      return;
    }
  }
  float eraw[K], adv[NHL], hasv[H], hdep;                // round 2's values: this kernel's locals (see HaloPrologue)
  float4 tdist;
  pro.round2(a, ln, eraw, adv, hasv, hdep, tdist);
  pro.dma_bases(a, ln);
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
  auto issue_slab = [&](int s) {   // (GraphSAGE: the second virtual head re-reads the same channels; HS: s counts half-slabs)
    pro.issue_slab(slab + (DBUF && !(s & 1) ? Lds::SLAB1 : 0), (AGG == 2 ? s % SPH : s) * ROWB, ln);
  };
  pro.write_halo_tables(ln, hasv, hdep, hid, has, hdp);
  if (Lds::HID_IN_ALPHA && hl == 0) cid[cell] = pro.my_pre < 0 ? -1 : pro.my_pre;
  pro.touch_round2(eraw, adv, hasv, hdep, tdist);
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
    float part[NHL][K + 1];
    if (my < 0) zero_coefficients(part);                // (zeros only where they are needed: no live range across the arithmetic)
    else if constexpr (AGG != 0) plain_coefficients<K, AGG>(hid0, has0, self_a, hl, a.self_loops, part[0]);
    else gat_coefficients<K, H>(hid0, has0, hdp, self_a, hl, eraw, adv, tdist, vpre, part);
#pragma unroll
    for (int i = 0; i < NHL; ++i) {
      const int hh = hl + i * 2;
      if (hh < H) {
        if constexpr (SP == 3) {      // kept in registers as bf16 pairs until this head's slabs come up (densified there)
          pack_coefficients<K>(part[i], apk[i]);
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
      bn_relu_half<HC, jA>(g, scsh0 + s * 128 + h * 64, a.relu);
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
      if constexpr (SP == 3) {
        if (s % SPH == 0 && s > 0) densify<K, NHL>(s / SPH, true, dn0, wbase, lane, r, hl, self_idx, apk);
      }
      if (s == 0) wait_vm_lgkm<0>();                    // (slab 0 was queued BEHIND its W rows: wait for everything)
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
        if constexpr (SP == 3) densify<K, NHL>(0, true, dn0, wbase, lane, r, hl, self_idx, apk);   // (every wave is past phase A: the alpha_src table is dead)
        if constexpr (EPI == EPI_HEADS && !Lds::HEADW_LATE) stage_head_table();   // (R is free; the last slab's full wait covers it)
        if (EPI == EPI_NEXT && !Lds::ATT_LATE && wave < 2 && lane * 4 < NC)
          __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>((wave == 0 ? a.att_src : a.att_dst) + lane * 4),
                                           (__attribute__((address_space(3))) void *)(attr + wave * NC), 16, 0, 0);
        wait_lgkm0();
        __builtin_amdgcn_s_barrier();                   // scale / shift visible
      }
      // DBUF: slab s is visible and the other image was released a slab ago -> request slab s + 1 NOW (VM queue: [WA s][WB s][slab s+1])
      if (DBUF && s + 1 < NSLAB && !DBG(4)) issue_slab(s + 1);
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
          aggregate_window<K>(d, ta, tb, bq0, hl);
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
      // layer epilogue: (+bias, BatchNorm) folded, ReLU -> h_{l+1}, in registers.  (bn_relu of fused_common.h, spelled out: called as a
      //  function here, the exact heads instances <64, 64, 4 | 8, 3, EPI_HEADS, 0> came out two VGPRs larger -- 142 / 162 for 140 / 160)
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
      if constexpr (DBUF) {
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
      if (!DBUF && s + 1 < NSLAB && !DBG(4)) issue_slab(s + 1);
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
            tile_pair_write(reinterpret_cast<char *>(patch), r, hl, t & 1, g, v);
          } else {
            *reinterpret_cast<float4 *>(patch + r * TILED_PITCH + 8 * g + 4 * hl) = v;
          }
        }
        asm volatile("" : "+v"(ps[t / TPH]), "+v"(pd[t / TPH]));   // the dots are due HERE (not sunk below the stores)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (SP == 3) {
          if (t & 1) {
#pragma unroll
            for (int k = 0; k < NSTORE; ++k)
              *reinterpret_cast<uint4 *>(prow[k] + (t - 1) * 64) = tile_pair_row_segment(reinterpret_cast<const char *>(patch), lane, k);
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

template <int HC, int C, int K, int NT, int EPI, int SP = 0, int AGG = 0, int LF = 0>
static int launch_inst(bgnn_ctx *ctx, const FusedArgs &a) {
  constexpr size_t lds_bytes = (size_t)FusedLds<HC, C, K, NT, EPI, SP, LF>::FLOATS * 4;
  static_assert(lds_bytes <= 160 * 1024, "one workgroup fits the CU's LDS");
  static std::atomic<uint64_t> configured{0};   // per instantiation (launch_with_lds)
  return launch_with_lds(ctx, gat_layer_fused_kernel<HC, C, K, NT, EPI, SP, AGG, LF>, configured, lds_bytes, a);
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
    return launch_two_phase(ctx, g->K, false, a);
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
  return launch_two_phase(ctx, g->K, true, a);
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
