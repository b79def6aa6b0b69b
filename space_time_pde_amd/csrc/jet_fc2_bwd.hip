// Second hidden layer of the reference width (fc2: 256 -> 128), exact fp32: weight gradient AND input gradient of one row tile
// in ONE eight-wave workgroup (the backward of src/implicit_net.py:48-54 through fc2 that loss.backward(),
// experiments/rb2d/train.py:77, runs).
//
// The two kernels this replaces repeat each other's work.  k_wgrad_quad<..., 8> (jet_wgrad_impl.h) reads the adjoint blocks of
// fc2's output rows (abar2) and the stash of fc1's output rows (pre[1]) and evaluates the activation jets of the stash for its
// operand; k_layer_coop<..., PRO_NONE, EPI_ADJ, ...> (jet_layer_impl.h) reads abar2 again, forms W2^T abar2 and reads pre[1]
// again in its epilogue, late, for the activation adjoint.  Both are partitioned by INPUT k-tile: wave w of the weight gradient
// owns k-tiles 2w and 2w + 1 of dW2, and output tile kt of W2^T abar2 -- with the adjoint that turns it into abar1 -- needs
// pre[1] of k-tile kt only.  So here wave w
//   * keeps the weight gradient's row-tile loop (the transposed adjoint blocks in `pshare`, the private patches, its accumulator
//     blocks, its tile order and its MFMA order into each of them, the raw-input tile on waves 0 .. 2, the tangent column sums
//     on waves 3 .. 7, the flush), and
//   * per k-tile k first forms output tile 2w + k of W2^T abar2 (B operand: the adjoint blocks of the row tile in their stored
//     column-major image, which every wave ALSO leaves in `pflat` next to the transposed copy; A operand: the WhT[2] pack
//     through a register ring one fragment ahead), then runs the weight gradient's jets and MFMAs on the pre[1] blocks of that
//     k-tile, then takes the activation adjoint against the same blocks and stores abar1 -- over the pre[1] blocks themselves
//     when the caller says so: every block is read and later written by the same wave.
// abar2 and pre[1] are read once, abar1 is written once; X once by waves 0 .. 2.
//
// Same bits as the two kernels: every dW2 accumulator keeps its tile order and its (stream, k-step) MFMA order; every abar1
// accumulator receives its products in the order of k_layer_coop's main loop for this layer -- contraction tile kt = 0 .. 7
// ascending, k-step r = 0 .. 3 ascending within it (streams and output tiles are independent accumulators there) -- and goes
// through the same layer_epilogue<S1, S2, EPI_ADJ, ACT, 0> with the same combination weights (-ffp-contract=off: the same
// instruction sequence wherever it is inlined).  The swish-beta adjoint is a sum of fp32 atomics in both forms.
//
// Registers decide the shape (one workgroup per CU, two waves per SIMD: 256 per lane; the weight gradient alone takes 252-256).
//   * Input blocks: ONE set in flight.  The blocks of a k-tile are requested behind the adjoint of the k-tile before it and land
//     during the 160 input-gradient MFMAs that open their own k-tile and need none of them (both k-tiles a whole row tile ahead,
//     the weight gradient's scheme, spilled 66-96 registers at S = 5).
//   * The 8 raw-input accumulator blocks of waves 0 .. 2 live in LDS between the row tiles, the tangent sums per owning wave.
//   * Block addresses are a scalar base + the unsigned lane offset (as signed per-lane pointers the sixteen weight-fragment
//     addresses alone were 32 loop-invariant registers, reloaded from scratch behind a vmcnt(0)).
// No instantiation uses scratch (profiles/fc2_bwd_fused_resource_usage.txt).  On one MI355X, 2^20 points, softplus: 47.6 ms
// against 29.6 + 25.5 ms for the two kernels (profiles/fc2_bwd_fused_kernel_trace.txt), 0.74 of the fp32 MFMA roof.
#include "jet_layer_impl.h"
#include "jet_wgrad_impl.h"

// workgroup barrier without the compiler's vector-memory drain in front of it (__syncthreads() carries a vmcnt(0): the blocks
// requested a tile ahead would be waited for at once).  The barriers of this kernel order LDS traffic only: a block of global
// memory is read and written by one wave alone.
#define FC2F_BARRIER()                                     \
  do {                                                     \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     \
    __builtin_amdgcn_s_barrier();                          \
    asm volatile("" ::: "memory");                         \
  } while (0)

template <int S1, int S2, int ACT>
__global__ __launch_bounds__(512, 2) void k_fc2_bwd_fused(WgradArgs a, LayerArgs la) {
  constexpr int S = 1 + S1 + S2, NWV = 8, KTT = 2 * NWV, MCW = NWV, KW = 2;
  constexpr int TP = 24, TBLK = 16 * TP;
  constexpr int PIN_MFMA_DSR = 0x2 | 0x4 | 0x10 | 0x20 | 0x40 | 0x200;   // VALU, SALU, VMEM, DS writes may cross; MFMA / DS reads not
  // the next row tile's adjoint blocks are requested in front of the last activation adjoint of this one (its ~3,000 cycles and
  // the raw-input phase cover the round trip); swish, whose adjoint also carries the beta sums, has no 20 registers left there
  // (48 bytes of scratch) and requests them behind it
  constexpr bool EARLYP = ACT != STPDE_ACT_SWISH;
  constexpr int NTW = (MCW + (NWV - XT) - 1) / (NWV - XT);                // output tiles whose tangent column sums one wave keeps
  static_assert(S1 == 3 && XT == 3, "tangent streams and three raw-input tiles expected");
  __shared__ __attribute__((aligned(16))) float pshare[S][MCW][TBLK];    // transposed adjoint blocks of the row tile
  __shared__ __attribute__((aligned(16))) float ppriv[NWV][2][TBLK];     // private patches (activated-input blocks)
  __shared__ __attribute__((aligned(16))) float pflat[S][MCW][256];      // the same adjoint blocks, column-major image
  __shared__ __attribute__((aligned(16))) float xacc[XT][MCW][256];      // raw-input accumulator blocks of waves 0 .. 2 (below)
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lo = lane * 4;
  const int g = lane >> 4, c = lane & 15;

  // The 8 accumulator blocks of a wave's raw-input tile are touched once per row tile (32 of its 672 MFMAs) and by three waves
  // only, but as registers they are 32 of every wave's 256 next to the input gradient's operands: they stay in LDS between the
  // row tiles (a block is read, takes its four MFMAs and is written back by its own wave: the same sums)
  f32x4 acc[MCW][KW];
#pragma unroll
  for (int mi = 0; mi < MCW; ++mi) {
#pragma unroll
    for (int k = 0; k < KW; ++k) acc[mi][k] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (wv < XT) st4(&xacc[wv][mi][lo], f32x4{0.f, 0.f, 0.f, 0.f});
  }
  float acct[3][NTW];
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int q = 0; q < NTW; ++q) acct[d][q] = 0.f;
  float pacc = 0.f;
  int flip = 0;
  auto transpose = [&](f32x4 v) -> f32x4 {
    float* patch = ppriv[wv][flip];
    flip ^= 1;
    lds_put_T<TP>(patch, lane, v);
    __builtin_amdgcn_wave_barrier();
    const f32x4 r = lds_get_R<TP>(patch, lane);
    __builtin_amdgcn_wave_barrier();
    return r;
  };

  // the blocks of a row tile are requested ahead, into the registers their predecessors have just released: the adjoint blocks
  // one tile ahead, right after they went into the patches; the input blocks of a k-tile one k-tile ahead, behind the adjoint of
  // the k-tile before it (they land during the 160 input-gradient MFMAs that open a k-tile and need none of them)
  f32x4 praw[S], qraw[S];
  // block (st, blk) of row tile t of a buffer of fp32 blocks [tile][S][NB][256] (common.h: ld_blk, mode 0), addressed as a
  // scalar base + the unsigned lane offset: as signed per-lane pointers the compiler keeps block addresses in register pairs
  auto ldb = [&](const float* buf, int t, int NB, int st, int blk) -> f32x4 {
    return ld4(buf + (((size_t)t * S + st) * NB + blk) * 256 + (unsigned)lo);
  };
  auto load_p = [&](int t) {
#pragma unroll
    for (int st = 0; st < S; ++st) praw[st] = ldb(a.P, t, MCW, st, wv);
  };
  auto load_qk = [&](int t, int k) {
#pragma unroll
    for (int st = 0; st < S; ++st) qraw[st] = ldb(a.Q, t, KTT, st, KW * wv + k);
  };
  // A operand of the input gradient: fragment f of the KTT-periodic sequence (k, kt) = (f / 8, f % 8) of the WhT pack, the same
  // for every row tile; slot f & 1 of a register ring, requested one fragment (20 MFMAs) ahead, across the k-tiles and the row tiles
  constexpr int MTD = KTT, KTD = MCW;                                     // the input gradient's GEMM: roles swapped
  f32x4 wr[2];
  auto load_w = [&](int f) {
    const int k = (f / KTD) % KW, kt = f % KTD;
    // (scalar base + unsigned lane offset: as signed per-lane pointers the sixteen fragment addresses were kept in 32 registers)
    wr[f & 1] = ld4(la.Wp + (size_t)((kt * MTD + KW * wv + k) * 256) + (unsigned)lo);
  };
  if ((int)blockIdx.x < a.ntiles) {
    load_p(blockIdx.x);
    load_qk(blockIdx.x, 0);
    load_w(0);
  }
#pragma unroll 1
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int tnext = tile + (int)gridDim.x < a.ntiles ? tile + (int)gridDim.x : tile;     // (last one: re-read, unused)
    float cq[6];
    load_cq<S2>(a.cw, tile * 2 + (c >> 3), cq);
#pragma unroll
    for (int st = 0; st < S; ++st) {
      lds_put_T<TP>(&pshare[st][wv][0], lane, praw[st]);
      st4(&pflat[st][wv][lo], praw[st]);
    }
    // raw-input tile of waves 0 .. 2 (column-major image: transposed at its use, behind the MFMAs of both k-tiles)
    f32x4 xcur = f32x4{0.f, 0.f, 0.f, 0.f};
    if (wv < XT) xcur = ld4(a.X + ((size_t)tile * XT + wv) * 256 + (unsigned)lo);
    FC2F_BARRIER();
#pragma unroll
    for (int k = 0; k < KW; ++k) {
      // ---- input gradient, output tile KW * wv + k: W2^T abar2 over the eight contraction tiles (k_layer_coop's order)
      f32x4 gacc[S];
#pragma unroll
      for (int st = 0; st < S; ++st) gacc[st] = f32x4{0.f, 0.f, 0.f, 0.f};
      {
        // block (kt, st) of the column-major image is requested before the four MFMAs of the block in front of it
        f32x4 Bc = ld4(&pflat[0][0][lo]);
#pragma unroll
        for (int kt = 0; kt < KTD; ++kt) {
          const int f = k * KTD + kt;
          const f32x4 w = wr[f & 1];
          load_w(f + 1);
#pragma unroll
          for (int st = 0; st < S; ++st) {
            f32x4 Bn = Bc;
            if (st + 1 < S) Bn = ld4(&pflat[st + 1][kt][lo]);
            else if (kt + 1 < KTD) Bn = ld4(&pflat[0][kt + 1][lo]);
            __builtin_amdgcn_sched_barrier(PIN_MFMA_DSR);
#pragma unroll
            for (int r = 0; r < 4; ++r) gacc[st] = mfma4(w[r], Bc[r], gacc[st]);
            __builtin_amdgcn_sched_barrier(PIN_MFMA_DSR);
            Bc = Bn;
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- weight gradient, k-tile KW * wv + k (k_wgrad_quad<..., 8>)
      {
        f32x4 H[S];
        act_jet_fwd<S1, S2, ACT>(a.cfg, qraw, H, cq);
#pragma unroll
        for (int st = 0; st < S; ++st) {
          const f32x4 hr = transpose(H[st]);
          f32x4 pc = lds_get_R<TP>(&pshare[st][0][0], lane);
#pragma unroll
          for (int mi = 0; mi < MCW; ++mi) {
            f32x4 pn = pc;
            if (mi + 1 < MCW) pn = lds_get_R<TP>(&pshare[st][mi + 1][0], lane);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[mi][k] = mfma4(pc[r], hr[r], acc[mi][k]);
            pc = pn;
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (EARLYP && k + 1 == KW) load_p(tnext);
      __builtin_amdgcn_sched_barrier(0);
      // ---- activation adjoint against the blocks still held, abar1 stored (over those blocks' own memory when Out == Q)
      layer_epilogue<S1, S2, EPI_ADJ, ACT, 0>(la, tile, KW * wv + k, MTD, lane, gacc, nullptr, cq, pacc, nullptr, qraw);
      __builtin_amdgcn_sched_barrier(0);
      if (k + 1 < KW) load_qk(tile, k + 1);
      else {
        load_qk(tnext, 0);
        if (!EARLYP) load_p(tnext);
      }
    }
    if (wv < XT) {
      const f32x4 xrr = transpose(xcur);
#pragma unroll
      for (int mi = 0; mi < MCW; ++mi) {
        const f32x4 p0 = lds_get_R<TP>(&pshare[0][mi][0], lane);
        f32x4 ax = ld4(&xacc[wv][mi][lo]);
#pragma unroll
        for (int r = 0; r < 4; ++r) ax = mfma4(p0[r], xrr[r], ax);
        st4(&xacc[wv][mi][lo], ax);
      }
    } else {
      // tangent stream d of a skip connection sees the unit vector e_d: column d of the raw-input block gets the sum over the
      // rows of the adjoint; the output tiles are dealt to the NWV - XT waves without a raw-input tile (k_wgrad_quad)
#pragma unroll
      for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int q = 0; q < NTW; ++q) {
          const int mi = q * (NWV - XT) + wv - XT;
          if (mi >= MCW) continue;                           // wave-uniform
          const f32x4 pd = lds_get_R<TP>(&pshare[1 + d][mi][0], lane);
          acct[d][q] += (pd[0] + pd[1]) + (pd[2] + pd[3]);
        }
    }
    FC2F_BARRIER();         // every wave is done with pshare / pflat before the next tile's blocks go in
  }
  const int ldw = 16 * (KTT + XT);
#pragma unroll
  for (int mi = 0; mi < MCW; ++mi) {
#pragma unroll
    for (int k = 0; k <= KW; ++k) {
      if (k == KW && wv >= XT) continue;
      const int col = k < KW ? 16 * (KW * wv + k) : 16 * (KTT + wv);
      const f32x4 v = k < KW ? acc[mi][k < KW ? k : 0] : ld4(&xacc[wv < XT ? wv : 0][mi][lo]);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc_add_f32(a.dW, (size_t)(16 * mi + 4 * g + r) * ldw + col + c, v[r], a.det);
    }
  }
  if (wv >= XT) {
    // lane (g, c): partial row sums (rows 4g..4g+3 of every tile) of output feature c; fold the four lane groups
#pragma unroll
    for (int q = 0; q < NTW; ++q)
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const int mi = q * (NWV - XT) + wv - XT;
        if (mi >= MCW) continue;
        float v = acct[d][q];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (g == 0 && d < a.ncoord) acc_add_f32(a.dW, (size_t)(16 * mi + c) * ldw + 16 * KTT + d, v, a.det);
      }
  }
  flush_pbar<EPI_ADJ, ACT>(la, pacc, lane);
}

template <int S1, int S2, int ACT>
static int launch_fc2_fused(const WgradArgs& a, const LayerArgs& la, hipStream_t stream) {
  int gx = 256;                            // one workgroup per CU, persistent: the tile assignment of k_wgrad_quad<..., 8>
  if (gx > a.ntiles) gx = a.ntiles;
  STPDE_LAUNCH((k_fc2_bwd_fused<S1, S2, ACT>), dim3(gx), dim3(512), 0, stream, a, la);
  return stpde_check_launch("k_fc2_bwd_fused");
}

template <int S1, int S2>
static int launch_fc2_fused_act(const WgradArgs& a, const LayerArgs& la, hipStream_t stream) {
  switch (a.cfg.act) {
    case STPDE_ACT_TANH: return launch_fc2_fused<S1, S2, STPDE_ACT_TANH>(a, la, stream);
    case STPDE_ACT_RELU: return launch_fc2_fused<S1, S2, STPDE_ACT_RELU>(a, la, stream);
    case STPDE_ACT_SOFTPLUS: return launch_fc2_fused<S1, S2, STPDE_ACT_SOFTPLUS>(a, la, stream);
    case STPDE_ACT_ELU: return launch_fc2_fused<S1, S2, STPDE_ACT_ELU>(a, la, stream);
    case STPDE_ACT_LEAKYRELU: return launch_fc2_fused<S1, S2, STPDE_ACT_LEAKYRELU>(a, la, stream);
    default: return launch_fc2_fused<S1, S2, STPDE_ACT_SWISH>(a, la, stream);
  }
}

// 1 when stpde_jet_fc2_bwd serves this layer description (callers keep stpde_jet_wgrad + stpde_jet_layer_bwd otherwise): a pure
// function of the descriptor -- the "fc2_bwd_fused" switch of stpde_tune is the caller's to read
extern "C" int stpde_jet_fc2_bwd_supported(const stpde_layer_desc* d) {
  if (!d) return 0;
  const bool combo = d->cfg.S2 == 1 && d->cfg.combo;
  return !d->first_hidden && d->mfma_bf16 == 0 && d->packed == 0 && d->KT == 16 && d->MT == 8 && XT == 3 && d->cfg.S1 == 3 &&
         (d->cfg.S2 == 0 || combo) && d->cfg.act >= 0 && d->cfg.act <= 5;
}

extern "C" int stpde_jet_fc2_bwd(const stpde_layer_desc* d, const float* abar2, const float* WhT_pack, const float* pre1,
                                 const float* X, const float* cw, float* abar1, float* dW_aug, float* act_param_bar,
                                 void* stream) {
  if (!stpde_jet_fc2_bwd_supported(d)) {
    stpde_set_error("jet_fc2_bwd: exact fp32, unpacked buffers only (second hidden layer of the reference width: KT = 16, MT = 8, "
                    "S1 = 3, S2 = 0 or the combined stream)");
    return STPDE_E_UNSUPPORTED;
  }
  if (d->ntiles <= 0 || !abar2 || !WhT_pack || !pre1 || !X || !abar1 || !dW_aug || (d->cfg.S2 && !cw) || abar1 == abar2) {
    stpde_set_error("jet_fc2_bwd: bad argument");
    return STPDE_E_BADARG;
  }
  const int S = 1 + d->cfg.S1 + d->cfg.S2;
  WgradArgs a{};
  a.P = abar2;
  a.Q = pre1;
  a.X = X;
  a.dW = dW_aug;
  a.cw = cw;
  a.SP = S;
  a.KT = d->KT;
  a.MT = d->MT;
  a.ntiles = d->ntiles;
  a.cfg = d->cfg;
  a.det = d->det;
  a.ncoord = 3;
  LayerArgs la{};         // the input gradient's view (jet_layer.hip, layer_bwd): contraction over MT, result over KT
  la.Bin = abar2;
  la.Wp = WhT_pack;
  la.Out = abar1;
  la.Pre = pre1;
  la.cw = cw;
  la.pbar = act_param_bar;
  la.nsplit = 1;
  la.KT = d->MT;
  la.MT = d->KT;
  la.ntiles = d->ntiles;
  la.cfg = d->cfg;
  if (d->cfg.S2 == 1) return launch_fc2_fused_act<3, 1>(a, la, (hipStream_t)stream);
  return launch_fc2_fused_act<3, 0>(a, la, (hipStream_t)stream);
}
