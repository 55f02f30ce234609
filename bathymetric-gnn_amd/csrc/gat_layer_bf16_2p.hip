// Two-phase form of the bf16 256 -> 256 fused GAT layer (matrix_path = bf16, BASELINE configs[2]); the one-phase kernel and the host
// entry points are in gat_layer_fused.hip, what the two share in fused_common.h.
// The one-phase kernel holds the [32 nodes x 256] accumulator (128 registers) NEXT TO everything the aggregation needs
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
#include "fused_common.h"

namespace bgnn {

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

// a slab's (or, aggregate first, a weight step's) 16 f32 values per lane as the two bf16 operands of phase 2; BN: folded bias +
// BatchNorm + ReLU first (cp: the slab's scale chunk, bn_relu)
template <int HC, bool BN>
__device__ __forceinline__ void to_operands(const f32x16 &d, uint32_t cp, int relu, bf16x8 (&x)[2]) {
  f32x4 g[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) g[j] = (f32x4){d[4 * j], d[4 * j + 1], d[4 * j + 2], d[4 * j + 3]};
  if constexpr (BN) bn_relu<HC>(g, cp, relu);
  x[0] = to_bf16x8(g[0], g[1]);
  x[1] = to_bf16x8(g[2], g[3]);
}

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
  constexpr int HC = 256, H = 4, H2 = 4, NC = 64 * H2, NT = 2 * H2, NSLAB = 8, SPH = 2, NHL = 2;   // H2: heads of the next layer = column passes
  constexpr int SRC_ROWB = AF ? 128 : HC * 2;             // bytes of a source row (AF: the 64-channel h1)
  using Geo = FusedGeom<K>;
  using Lds = TwoPhaseLds<K>;
  using Win = AggWindow<K>;
  constexpr int HR = Geo::HR;
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
  const LaneCoords<K> ln;
  const int tid = ln.tid, lane = ln.lane, wave = ln.wave, r = ln.r, hl = ln.hl, cell = ln.cell, self_idx = ln.self_idx;

  // ---- prologue: the shared two load rounds (HaloPrologue), without any weight traffic
  HaloPrologue<K, CPR, SRC_ROWB, H, 0, false, false, AF ? 2 : NSLAB> pro;
  pro.round1(a, pos, ln);
  float scv = a.scale[tid], shv = a.shift[tid];          // HC == NTH: one channel per thread
  float vpre[NHL][3];
#pragma unroll
  for (int i = 0; i < NHL; ++i)
#pragma unroll
    for (int f = 0; f < 3; ++f) vpre[i][f] = a.V[(hl + i * 2) * 3 + f];
  pro.validity(ln, false);
  if (a.cell_map) {                  // canvas walk: blocks that hold only gutter / free space leave here (nothing is in flight yet)
    if (pro.gutter_only(ln, minid)) return;
  }
  float eraw[K], adv[NHL], hasv[H], hdep;                // round 2's values: this kernel's locals (see HaloPrologue)
  float4 tdist;
  pro.round2(a, ln, eraw, adv, hasv, hdep, tdist);
  pro.dma_bases(a, ln);
  pro.write_halo_tables(ln, hasv, hdep, hid, has, hdp);
  if (hl == 0) cid[cell] = pro.my_pre < 0 ? -1 : pro.my_pre;
  if (tid < Lds::PAD_B / 4) reinterpret_cast<float *>(base + Lds::SLAB_B)[tid] = 0.0f;   // (the rows read past the image: zeros)
  pro.touch_round2(eraw, adv, hasv, hdep, tdist, scv, shv);
  pro.issue_slab(slab, 0, ln);
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
    if (my < 0) zero_coefficients(part);
    else gat_coefficients<K, H>(hid0, has0, hdp, self_idx, hl, eraw, adv, tdist, vpre, part);
#pragma unroll
    for (int i = 0; i < NHL; ++i) pack_coefficients<K>(part[i], apk[i]);
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
  // one att piece per wave (waves 2, 3 repeat 0, 1's) so that every wave's VM queue counts alike
  auto issue_att = [&]() {
    if (lane * 4 < NC)
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(((wave & 1) == 0 ? a.att_src : a.att_dst) + lane * 4),
                                       (__attribute__((address_space(3))) void *)(attl + (wave & 1) * NC), 16, 0, 0);
  };
  bf16x8 xh[NSLAB][2];
  auto slab_step = [&](auto sc) {
    constexpr int s = decltype(sc)::value;
    if constexpr (s % SPH == 0 && s > 0) densify<K, NHL>(s / SPH, true, dn0, wbase, lane, r, hl, self_idx, apk);
    wait_vm_lgkm<0>();                                   // slab s is all this wave has in flight
    __builtin_amdgcn_s_barrier();                        // slab s visible to every wave
    if constexpr (s == 0) {
      scsh[tid] = scv; scsh[HC + tid] = shv;             // (phase A is over on every wave: nothing is in flight, visible stores are fine)
      densify<K, NHL>(0, true, dn0, wbase, lane, r, hl, self_idx, apk);
      wait_lgkm0();
      __builtin_amdgcn_s_barrier();
    }
    f32x16 d;
    aggregate_window<K>(d, tr0, tr1, bq0, hl);
    // (the reads of slab s are complete -- agg_blocks waits for them before its MFMAs -- so the image can be handed to slab s + 1
    //  as soon as every wave is here; BatchNorm / ReLU / conversion then run under that DMA's flight)
    __builtin_amdgcn_s_barrier();
    if constexpr (s + 1 < NSLAB) {
      pro.issue_slab(slab, (s + 1) * ROWB, ln);
    } else {
      // last slab: the image and the alpha matrices are dead on every wave -> phase 2's first W pass and the next layer's
      // att_src | att_dst can be requested NOW (they land in [0, 32 KB) and behind the patches: clear of the scale / shift table the
      // BatchNorm below still reads)
      issue_att();
      issue_w(0);
    }
    to_operands<HC, true>(d, scsh0 + s * 128, a.relu, xh[s]);
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
        densify<K, NHL>(hd, s == 0, dn0, wbase, lane, r, hl, self_idx, apk);
        f32x16 d;
        aggregate_window<K>(d, tr0, tr1, bq0, hl);
        to_operands<HC, false>(d, 0, 0, xa[hd][s]);
      };
      head(std::integral_constant<int, 0>{}); head(std::integral_constant<int, 1>{});
      head(std::integral_constant<int, 2>{}); head(std::integral_constant<int, 3>{});
      __builtin_amdgcn_s_barrier();                      // every wave has read slab s
      if constexpr (s == 0) {
        pro.issue_slab(slab, ROWB, ln);
      } else {
        // the image and the alpha matrices are dead: the heads' weight blocks (32 pieces of 1 KiB, [head][k-step][tile], into the pass
        // buffer) and the next layer's att vectors can be requested
        issue_att();
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
        to_operands<HC, true>(acc, scsh0 + (2 * hd + t) * 128, a.relu, xh[2 * hd + t]);
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
        tile_pair_write(patch, r, hl, tt, g, v);
      }
      asm volatile("" : "+v"(ps_), "+v"(pd_));
      __builtin_amdgcn_sched_barrier(0);
    }
    sl_[cp] = ps_.x + ps_.y; dl_[cp] = pd_.x + pd_.y;
#pragma unroll
    for (int k = 0; k < NSTORE; ++k) {
      const uint4 q = tile_pair_row_segment(patch, lane, k);
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

template <int K, bool AF>
static int launch_inst_2p(bgnn_ctx *ctx, const FusedArgs &a) {
  static std::atomic<uint64_t> configured{0};
  return launch_with_lds(ctx, gat_layer_bf16_2p_kernel<K, AF>, configured, (size_t)TwoPhaseLds<K>::BYTES, a);
}

int launch_two_phase(bgnn_ctx *ctx, int K, bool af, const FusedArgs &a) {
  if (af) return K == 8 ? launch_inst_2p<8, true>(ctx, a) : K == 4 ? launch_inst_2p<4, true>(ctx, a) : launch_inst_2p<16, true>(ctx, a);
  return K == 8 ? launch_inst_2p<8, false>(ctx, a) : K == 4 ? launch_inst_2p<4, false>(ctx, a) : launch_inst_2p<16, false>(ctx, a);
}

}  // namespace bgnn
