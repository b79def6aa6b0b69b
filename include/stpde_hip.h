/*
 * stpde_hip.h -- C ABI of libstpde_hip.so: the MI355X (gfx950) device path behind the MeshfreeFlowNet
 * operator API (PDELayer / query_local_implicit_grid / ImNet / regular_nd_grid_interpolation).
 *
 * The reference (maxjiang93/space_time_pde) is pure Python on PyTorch and has NO native interface; each
 * entry point below states which reference code (file:line under /root/reference) it replaces.  The
 * binding a maintainer adds is the ctypes stub shown in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into memory owned by the caller (PyTorch caching allocator);
 *     the library never allocates, frees or retains device memory;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued there, nothing synchronises;
 *   - return value: 0 = ok, otherwise one of STPDE_E_*; stpde_last_error() gives the text;
 *   - all arithmetic is IEEE fp32 (no fast-math, no FMA contraction outside MFMA), indices int32.
 *
 * Fragment ("stash") layout used by the jet kernels.  Query points are grouped in tiles of 2 points =
 * 16 corner rows (row j = 8*point_in_tile + corner, corner = 4*b0+2*b1+b2 as
 * src/regular_nd_grid_interpolation.py:55-56).  A block of 16 rows x 16 features is stored as 64 lanes x 4
 * floats (1 KiB): lane = 16*g + j holds features 4g..4g+3 of row j -- exactly the C/D register image of
 * v_mfma_f32_16x16x4_f32 for out^T = W * in^T, which is also the B-operand image of the next layer, so
 * layers chain without any re-layout.  A layer buffer is [tile][stream][feature_tile][64][4] floats.
 * Streams: 0 = value, 1..3 = d/dr_k (if S1 == 3), then S2 second-order pairs (pair0[k], pair1[k]).
 */
#ifndef STPDE_HIP_H
#define STPDE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define STPDE_OK 0
#define STPDE_E_BADARG 1      /* shape / size / enum out of the supported range -> ValueError */
#define STPDE_E_UNSUPPORTED 2 /* stream configuration not compiled in            -> NotImplementedError */
#define STPDE_E_LAUNCH 3      /* HIP launch failure                              -> RuntimeError */

#define STPDE_ACT_TANH 0
#define STPDE_ACT_RELU 1
#define STPDE_ACT_SOFTPLUS 2
#define STPDE_ACT_ELU 3
#define STPDE_ACT_SWISH 4
#define STPDE_ACT_LEAKYRELU 5

#define STPDE_XT 3 /* the augmented raw input [r(3) ; latent(c) ; 1 ; 0-pad] occupies 3 feature tiles, the third one sparse (4 live slots): 3 + c + 1 <= 36, i.e. c <= 32 */
#define STPDE_PBAR_SLOTS 64 /* accumulation slots of the swish-beta adjoint (stpde_jet_layer_bwd), summed by the caller */

/* Derivative-stream configuration shared by the jet kernels. */
typedef struct {
  int S1;        /* 0 (value only) or 3 (value + d/dr_0..2)                         */
  int S2;        /* number of second-order streams: 0, 1 (combined, see below), 2 or 6 compiled in.
                  * S1 == 0 with S2 == 3 is the forward-only VALUE-TILE mode of stpde_jet_layer_fwd: the 4 "streams" are
                  * the value streams of 4 consecutive row tiles (desc.ntiles counts groups of 4 tiles), which share one
                  * pass over the weights; buffers are laid out exactly as for S1 = S2 = 0 with 4 * ntiles tiles. */
  int pair0[6];  /* second-order stream k is d2/dr_pair0[k] dr_pair1[k]             */
  int pair1[6];
  int act;       /* STPDE_ACT_*  (src/nonlinearities.py:15-22)                       */
  float act_param; /* swish beta; leaky-relu slope is fixed at 0.01 (torch default) */
  /* Combined second-order stream (S2 == 1): when every equation uses the second derivatives only through ONE linear
   * combination  L y = sum_k alpha[k] d2y/dq_a dq_b  over the canonical pairs (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
   * (e.g. the anisotropic Laplacian of the Rayleigh-Benard equations), the MLP carries that single stream instead of
   * one per pair: F' = sigma''(a) * sum_k c_k adot_a adot_b + sigma'(a) * (W F), with per-point weights
   * c_k = alpha[k] * kappa_a * kappa_b written by stpde_lig_gather into cw[P][8]. */
  int combo;     /* 1: S2 must be 1 and the stream is the combination above          */
  float alpha[6];
} stpde_jet_cfg;

int stpde_version(void);
int stpde_last_error(char* buf, unsigned long n);
/* Launch-geometry overrides for TESTS (round 6; nothing in the reference corresponds to it, and the library reads no
 * environment variable): the persistent-grid convolution kernels pick their grid and their minimum volume themselves; a
 * test forces other values to reach their multi-block and ragged-tail paths on volumes it can afford.  value 0 = the library's
 * own choice (the default of every key).  Keys: "conv3_lds_off" (1: the 3x3x3 LDS-tile kernel is not used),
 * "conv3_lds_minblk" (minimum number of blocks for it), "conv3_lds_gx", "conv_wgrad_lds_gx", "conv1_wgrad_lds_gx" (grid sizes).
 * "wgrad_fp32_swap": loop body of the exact-fp32 first-hidden-layer weight-gradient kernel (k_wgrad_coop, MODE 1, at most five
 * streams, every stream in the adjoint buffer): 0 = the library's own choice (the phase-swapped loop), 1 = the phase-swapped
 * loop, 2 = the lock-step loop.  The two loops differ for EVERY wave, not only in the phase order of waves 4 .. 7: in the
 * phase-swapped loop all eight waves fetch their next adjoint operand set in the row-major image with dword loads spread over
 * the MFMAs (no transposes through the LDS patch), and waves 4 .. 7 build their ring slot before their MFMAs instead of behind
 * them; the lock-step loop restores the old load form for all waves.  The results are the same bits either way (A/B timing,
 * tests/test_gpu_wgrad_fp32_phase_swap.py).
 * "fc2_bwd_fused": exact fp32, second hidden layer of the reference width: 0 / 1 = a call of stpde_lig_imnet_jet_bwd that asks
 * for it (STPDE_F_FC2_FUSED) and for weight gradients runs the layer's weight gradient and input gradient as ONE kernel
 * (stpde_jet_fc2_bwd) where stpde_jet_fc2_bwd_supported says so; 2 = the two kernels whatever the call asks for.  Same bits
 * either way in deterministic mode (tests/test_gpu_fc2_bwd_fused.py).
 * Returns the previous value, -1 for an unknown key.  Process-wide, thread-safe. */
#define STPDE_TUNE_CONV3_LDS_OFF 0
#define STPDE_TUNE_CONV3_LDS_MINBLK 1
#define STPDE_TUNE_CONV3_LDS_GX 2
#define STPDE_TUNE_CONV_WGRAD_LDS_GX 3
#define STPDE_TUNE_CONV1_WGRAD_LDS_GX 4
#define STPDE_TUNE_WGRAD_FP32_SWAP 5
#define STPDE_TUNE_FC2_BWD_FUSED 6
#define STPDE_TUNE_COUNT 7
int stpde_tune(const char* name, int value);
/* Dispatch trace (test / debugging facility; nothing in the reference corresponds to it): while enabled, every kernel
 * launch records which template instantiation it dispatched ("<kernel expression> @ <launcher with template
 * arguments>", unique entries).  stpde_trace_enable clears the set; stpde_trace_read copies the newline-separated
 * entries (truncated to n - 1 bytes) and returns the number of bytes needed for all of them. */
int stpde_trace_enable(int on);
long stpde_trace_read(char* buf, unsigned long n);

/* ---- a1/a2: clip, cell index, corner gather, weights, relative coords ------------------------------
 * Replaces regular_nd_grid_interpolation_coefficients (src/regular_nd_grid_interpolation.py:14-78) +
 * the torch.cat of local_implicit_grid.py:49 for dim = 3.  Writes the augmented input X
 * [ntiles][3][64][4], per-point coefficients coef[P][16] = {omega[b][d] (6), domega[b][d] (6), kappa[d] (3), 0}
 * and cell[P] = linear index of corner 0 in the latent grid.  lo_c/hi_c = xmin+eps / xmax-eps and
 * cube = (xmax-xmin)/(size-1) are computed by the caller with the reference's own fp32 expressions
 * (:48-51) so that floor(q/cube) is bit-identical (:52).  xmin must be 0 (quirk: :52 ignores xmin).
 * P must be even; pts [P][3] (a chunk of the [B*N] point list starting at p_base); latent [B][n0][n1][n2][C]
 * contiguous. */
typedef struct {
  int P, N, B, n0, n1, n2, C;
  int p_base; /* global index of pts[0]: batch of point p is min((p_base + p) / N, B - 1) */
  float lo_c[3], hi_c[3], cube[3];
  float alpha[6]; /* combined second-order stream weights (only read when cw != NULL) */
} stpde_gather_desc;
/* XR (optional, normally NULL since round 5): the same augmented input in the row-major fragment image (lane 16g+c holds
 * rows 4g..4g+3 of feature c).  No kernel of the library reads it any more: the weight-gradient kernels take X and turn
 * the fragments they need into the row-major image inside LDS (1.5 KiB per point less written and re-read). */
int stpde_lig_gather(const stpde_gather_desc* d, const float* pts, const float* latent, float* X, float* XR,
                     float* coef, int* cell, float* cw /* [P][8] or NULL */, void* stream);

/* ---- a4/a5/a6/a7: one IM-NET layer on all derivative streams --------------------------------------
 * Replaces the addmm + activation + cat of src/implicit_net.py:48-54 evaluated on the
 * [b*p*2^d, d+c] matrix of src/local_implicit_grid.py:53, together with the torch.autograd.grad sweeps of
 * src/pde.py:8-9 (forward-mode streams instead of reverse sweeps).
 * out_pre[tile][S][MT] = W_h * act_jet(in_pre[tile][S][KT]) + W_s * X + tangent consts   (pre-activations)
 * first_hidden != 0: the input is layer 0's output, computed on the fly from X (in_pre ignored). */
typedef struct {
  int ntiles, KT, MT, first_hidden;
  stpde_jet_cfg cfg;
  /* BASELINE config 4 ("bf16 MFMA MLP path"): != 0 runs the hidden-to-hidden GEMMs of the wide layers (those served
   * by the workgroup-cooperative kernels: KT % 4 == 0, KT >= 8, MT % 8 == 0) on v_mfma_f32_16x16x32_bf16 -- operands
   * rounded to bf16 (round-to-nearest-even), fp32 accumulation; layer-0 regeneration, skip/bias GEMM, activation
   * jets, stash and epilogues stay fp32.  Narrow layers (HBM-bound) keep the fp32 kernels. */
  /* mfma_bf16 == 3 ("fp32x3", forward and input-gradient kernels only): fp32-ACCURATE products on the bf16 pipe -- every
   * fp32 operand is split exactly into three bf16 terms (hi + mid + lo = 8 + 8 + 8 mantissa bits; the weights on the
   * host: Wh_pack_bf16 is then [3][KT/2][MT][64] blocks, the activations in the kernel's produce stage) and the six
   * partial products of weight >= 2^-16 are accumulated in fp32; bf16 x bf16 is exact in fp32 and the dropped products are
   * below 2^-24 of the result, i.e. below fp32 rounding.  6 bf16 MFMAs (K = 32) replace 8 fp32 MFMAs at 1/16 of the
   * per-instruction time. */
  int mfma_bf16;
  /* PACKED layer buffers (round 3, bf16 mode only; every consumer of such a buffer is a bf16-operand kernel).  Two formats:
   *   packed STASH   (buffers of pre-activations): value stream fp32, derivative streams bf16 -- per row tile
   *                  [MT][64][4] fp32, then [S-1][MT][64][4] bf16: MT * (1024 + (S-1) * 512) bytes instead of MT * S * 1024;
   *   packed ADJOINT (buffers of adjoints): every stream bf16 -- per row tile [S][MT][64][4] bf16, MT * S * 512 bytes (all
   *                  consumers round every stream to a bf16 MFMA operand; the d-latent reduction reads stream 0).  An
   *                  adjoint buffer never aliases the stash it belongs to.
   * Bit mask: 1 = in_pre (hidden input of a forward call / the pre-activations a backward kernel takes its adjoint against)
   * is a packed stash, 2 = the buffer this call WRITES is packed (out_pre of a forward call: stash; the adjoint destination
   * of stpde_jet_layer_bwd / _bwd_to, including the layer-0 adjoint of a first-hidden-layer call: adjoint format),
   * 4 = abar_out (input of the backward / weight-gradient kernels) is a packed adjoint buffer. */
  int packed;
  /* Deterministic mode (round 6; stpde_jet_wgrad / stpde_jet_fc1_bwd only): != 0 -> dW_aug addresses long accumulators (six
   * zero-filled 64-bit integers per element instead of one float, see stpde_conv3d_desc.det), into which the workgroups'
   * partial sums are added with integer atomics -- order-independent, bit-identical from run to run; stpde_det_finalize turns
   * them into fp32.  (The adjoint of a learnable swish beta keeps its fp32 atomics.) */
  int det;
} stpde_layer_desc;
/* Wh_pack_bf16 (used when d->mfma_bf16 != 0, may be NULL otherwise): [KT/2][MT][64] blocks of 8 bf16 =
 * the two fp32 blocks (2q, mt) and (2q+1, mt) of Wh_pack, lane by lane, rounded to bf16.
 * z0 (first_hidden only, may be NULL = not kept; ignored in the value-tile mode): [tile][KT][256] receives the value
 * stream of the layer-0 pre-activations the kernel regenerates from X -- the stash stpde_jet_layer_bwd(first_hidden) reads. */
int stpde_jet_layer_fwd(const stpde_layer_desc* d, const float* in_pre, const float* X, const float* Wh_pack,
                        const float* Ws_pack, const float* tanc, const float* W0s_pack, const float* tanc0,
                        float* out_pre, const float* cw /* combined-stream weights or NULL */,
                        const void* Wh_pack_bf16, float* z0, void* stream);

/* Fused forward of the three narrowest layers fc3 -> fc4 -> fc5 (src/implicit_net.py:48-54) for nf = 16 * nf16, nf16 in
 * {1, 2}: equivalent to three stpde_jet_layer_fwd calls, but the inter-layer data stays in registers (the accumulator
 * tiles of one layer are the B operand of the next); the pre-activations of all three layers are written for the backward.
 * Wh_pack / Ws_pack / tanc / out_pre: HOST arrays of 3 device pointers (layers 3, 4, 5).  Stream sets (0,0) (3,0)
 * (3,1 combined) (3,2), and the forward-only value-tile set (0,3): ntiles = row tiles / 4, tanc may be NULL. */
int stpde_jet_tail_fwd(const stpde_jet_cfg* cfg, int ntiles, int nf16, const float* in_pre2, const float* X,
                       const float* const* Wh_pack, const float* const* Ws_pack, const float* const* tanc,
                       float* const* out_pre, const float* cw, void* stream);

/* bf16 mode (stpde_imnet_plan.mfma_bf16 == 1; nf = 32, S1 = 3): the same chain with the hidden-to-hidden products on the
 * bf16 MFMA and PACKED layer buffers (stpde_layer_desc.packed).  packed: 1 = in_pre2 is packed, 2 = out_pre[0] / [1] are
 * written packed (out_pre[2], the rows of the output layer, stays fp32 blocks); Wh16_pack: the bf16 A-operand packs of the
 * three layers in TWO terms, [2][KT/2][MT][64] x 8 bf16 (hi, then lo = bf16(w - hi); two k-tiles per block) -- these layers
 * are narrow, so both operands of a product are split into two bf16 terms and the product is three bf16 MFMAs (2^-16
 * relative).  Compiled for packed == 3 with all three packs; packed == 0 and Wh16_pack == NULL: stpde_jet_tail_fwd. */
int stpde_jet_tail_fwd_p(const stpde_jet_cfg* cfg, int ntiles, int nf16, const float* in_pre2, const float* X,
                         const float* const* Wh_pack, const float* const* Ws_pack, const float* const* tanc,
                         float* const* out_pre, const float* cw, int packed, const void* const* Wh16_pack, void* stream);

/* Fused input-gradient chain of the same three layers: abar5 (adjoint of fc5's output rows, from stpde_lig_reduce_bwd)
 * -> abar4 -> abar3 -> abar2; equivalent to stpde_jet_layer_bwd on layers 5, 4, 3, but the adjoints of layers 4 and 3 feed
 * the next GEMM from the registers.  pre[0..2]: stashed pre-activations of the outputs of fc2, fc3, fc4; abar_out[0..2]:
 * where their adjoints go -- abar_out[l] may be pre[l] (in place) when no later kernel needs those pre-activations: the
 * weight gradient of layer l+1 reads pre[l], so either it runs first or abar_out[l] is a separate buffer.
 * WhT_pack: HOST array of the 3 transposed packs of layers 3, 4, 5. */
int stpde_jet_tail_bwd(const stpde_jet_cfg* cfg, int ntiles, int nf16, const float* abar5, const float* const* WhT_pack,
                       const float* const* pre, float* const* abar_out, const float* cw, float* act_param_bar,
                       void* stream);

/* bf16 mode: the same chain on the bf16 MFMA with every pre[] a packed stash and every abar_out[] a packed ADJOINT buffer
 * (packed == 3; abar_out[l] must not alias pre[l]);
 * WhT16_pack: bf16 packs of the transposed weights of layers 3 and 4 ([MT/2][KT][64] x 8 bf16; entry [2] is not read,
 * the product through the output layer stays fp32).  packed == 0 and WhT16_pack == NULL: stpde_jet_tail_bwd. */
int stpde_jet_tail_bwd_p(const stpde_jet_cfg* cfg, int ntiles, int nf16, const float* abar5, const float* const* WhT_pack,
                         const float* const* pre, float* const* abar_out, const float* cw, float* act_param_bar, int packed,
                         const void* const* WhT16_pack, void* stream);

/* Backward of the same layer w.r.t. its hidden input (the autograd backward of the addmm/activation graph,
 * i.e. what loss.backward() at experiments/rb2d/train.py:77 does through src/implicit_net.py:48-54):
 *   hbar = W_h^T * abar_out ; abar_in = act_jet_adjoint(hbar, in_pre)   written over in_pre (in place) when
 * first_hidden == 0, or into abar0[tile][1+S1][KT] otherwise (layer 0; its pre-activations are read from z0
 * [tile][KT][256], the value-stream stash written by stpde_jet_layer_fwd(first_hidden) -- round 2: regenerating them from X
 * cost 3.5 % of this kernel's MFMAs; X and W0s_pack are no longer read and may be NULL).  z0 may be the same buffer as abar0
 * when abar0 holds the value stream only (abar0_tan given, or S1 == 0): every lane reads its element before it writes it.
 * abar0_tan (first_hidden, S1 == 3; may be NULL): layer 0's tangent streams are the constant columns W0[:, d], so their
 * adjoints are needed only summed over rows; when given, abar0 receives the VALUE stream only ([tile][KT][256]) and
 * abar0_tan [tile][KT][3][16] the per-tile row sums of the three tangent-stream adjoints (a quarter of the traffic);
 * stpde_jet_tan0_reduce adds them into d W0[:, d].
 * act_param_bar (swish only, may be NULL): STPDE_PBAR_SLOTS (64) floats that ACCUMULATE partial sums of the adjoint of
 * the learnable beta (src/nonlinearities.py:5-12); the caller zero-fills them and adds the slots up. */
int stpde_jet_layer_bwd(const stpde_layer_desc* d, const float* abar_out, const float* WhT_pack, float* in_pre,
                        const float* X, const float* W0s_pack, const float* tanc0, float* abar0, const float* cw,
                        float* act_param_bar, const void* WhT_pack_bf16 /* as Wh_pack_bf16, of WhT_pack */,
                        float* abar0_tan, const float* z0, void* stream);

/* The same input gradient of a hidden layer (first_hidden == 0) written to a SEPARATE buffer abar_in instead of over the
 * stashed pre-activations in_pre (which stay intact): lets the whole input-gradient chain run before the weight gradients
 * -- "dgrad-first" order, so that the partial d latent of a rank is complete, and its all-reduce in flight, while the weight
 * gradients are still being computed (the overlap DistributedDataParallel gets from bucketed all-reduces inside
 * loss.backward(), experiments/rb2d/train_ddp.py:401-406). */
int stpde_jet_layer_bwd_to(const stpde_layer_desc* d, const float* abar_out, const float* WhT_pack, const float* in_pre,
                           float* abar_in, const float* cw, float* act_param_bar, const void* WhT_pack_bf16, void* stream);

/* Weight gradient of one layer: dW_aug[16*MT][16*(KT+3)] += sum_rows abar_out (x) [act_jet(in_pre) ; X_aug]
 * (columns: hidden inputs, then r(3), latent(c), bias, pad).  abar_out [tile][SP][MT] (SP = S, or 1+S1 for layer 0)
 * and in_pre [tile][S][KT] are the ordinary (column-major) layer buffers -- call it BEFORE stpde_jet_layer_bwd of the
 * same layer overwrites in_pre.  first_hidden: in_pre is the z0 stash [tile][KT][256] written by
 * stpde_jet_layer_fwd(first_hidden) (value stream of layer 0's pre-activations; the tangent streams are the constant
 * columns tanc0 [3][KT][256] = W0[:, d] in the column-major image, the second-order streams are zero) -- call it before
 * stpde_jet_layer_bwd(first_hidden) writes the layer-0 adjoint over the stash.  X = the (column-major) augmented input from
 * stpde_lig_gather.  fp32 atomics; caller zero-fills dW_aug.  d->mfma_bf16: layers with MT >= 8 contract with
 * bf16-rounded operands (two derivative streams per v_mfma_f32_16x16x32_bf16), fp32 accumulation.  d->packed (bf16 mode,
 * bits 1 = in_pre is a packed stash, 4 = abar_out is a packed adjoint buffer): the narrow layers (MT < 8) and the raw-input
 * layer (KT = 0, mfma_bf16 = 1, packed = 4) then contract over the rows with bf16 MFMAs as well; the raw-input columns of
 * the hidden layers stay fp32. */
int stpde_jet_wgrad(const stpde_layer_desc* d, int SP, const float* abar_out, const float* in_pre, const float* X,
                    const float* tanc0, float* dW_aug, const float* cw, void* stream);

/* bf16 mode, first hidden layer of the reference width (round 5): stpde_jet_wgrad(first_hidden) + stpde_jet_layer_bwd(first_hidden)
 * in ONE call -- one kernel reads the packed adjoint tile of fc1's rows once (LDS) for both products, W1h^T abar1 and
 * abar1^T act_jet(z0), and evaluates the activation jet of every z0 element once for the layer-0 adjoint and for the weight
 * gradient's operand blocks (csrc/jet_fc1_bwd.hip; the backward of src/implicit_net.py:48-54 through fc1 that loss.backward(),
 * experiments/rb2d/train.py:77, performs).  d: the description stpde_jet_layer_bwd takes for this layer (first_hidden = 1,
 * KT = 32, MT = 16, mfma_bf16 = 1, packed bits 2 and 4, S1 = 3, S2 = 0 or the combined stream).  abar1: packed ADJOINT buffer
 * of fc1's rows; WhT_pack_bf16: bf16 pack of W1h^T; z0 / tanc0 / cw / X as for the two calls it replaces; abar0 (packed
 * ADJOINT blocks of the value stream, must not alias z0), abar0_tan ([tile][32][3][16] row sums) as stpde_jet_layer_bwd writes
 * them; dW_aug: fc1's block of the flat gradient buffer (accumulated with fp32 atomics).
 * stpde_jet_fc1_bwd_supported(d) != 0 iff this call serves d (a pure function of d). */
int stpde_jet_fc1_bwd_supported(const stpde_layer_desc* d);
int stpde_jet_fc1_bwd(const stpde_layer_desc* d, const float* abar1, const void* WhT_pack_bf16, const float* z0,
                      const float* tanc0, const float* cw, const float* X, float* abar0, float* abar0_tan, float* dW_aug,
                      float* act_param_bar, void* stream);

/* Exact fp32, second hidden layer of the reference width: stpde_jet_wgrad + stpde_jet_layer_bwd of that layer in ONE call
 * (csrc/jet_fc2_bwd.hip).  Both products are partitioned by the layer's INPUT k-tile, so one eight-wave workgroup per row tile
 * reads the adjoint blocks abar2 and the stashed pre-activations pre1 of fc1's rows once and evaluates their activation jets
 * once.  d: the description stpde_jet_wgrad takes for this layer (first_hidden = 0, KT = 16, MT = 8, mfma_bf16 = 0, packed = 0,
 * S1 = 3, S2 = 0 or the combined stream; d->det as there).  abar2 [tile][S][8][256], pre1 [tile][S][16][256], X, cw as for the two
 * calls it replaces; WhT_pack: the fp32 pack of W2h^T (stpde_jet_layer_bwd's); abar1 [tile][S][16][256] receives the adjoint of
 * fc1's rows and MAY be pre1 itself (every block is read and later written by the same wave); dW_aug: fc2's block of the flat
 * gradient buffer; act_param_bar as stpde_jet_layer_bwd.  In deterministic mode dW_aug and abar1 are the bits of the two calls.
 * stpde_jet_fc2_bwd_supported(d) != 0 iff this call serves d (a pure function of d). */
int stpde_jet_fc2_bwd_supported(const stpde_layer_desc* d);
int stpde_jet_fc2_bwd(const stpde_layer_desc* d, const float* abar2, const float* WhT_pack, const float* pre1, const float* X,
                      const float* cw, float* abar1, float* dW_aug, float* act_param_bar, void* stream);

/* ---- a4: corner-weighted reduction (src/local_implicit_grid.py:59) on all streams ------------------
 * jets[(s*n_out + ch)*ldp + p] (ldp >= P lets a chunk of points write into a larger [S][n_out][Ptotal] array)
 * from out_pre[tile][S][1][64][4] (fc5 output) and coef; and its adjoint. */
/* S_mlp = number of streams held by the layer buffers: 1 + S1 + S2, or 1 + S1 for piecewise-linear activations
 * (relu / leaky-relu: sigma'' = 0, so every second-order MLP stream is identically zero and is not carried; the
 * second derivatives of y then come from the weight-derivative cross terms alone). */
int stpde_lig_reduce_fwd(const stpde_jet_cfg* cfg, int S_mlp, int P, int n_out, const float* out_pre,
                         const float* coef, float* jets, long ldp, void* stream);
int stpde_lig_reduce_bwd(const stpde_jet_cfg* cfg, int S_mlp, int P, int n_out, const float* jets_bar, long ldp,
                         const float* coef, float* abar_out, void* stream);

/* dW_aug[16*MT][ldw] (layer 0: ldw = 16 * XT) column d  +=  sum over tiles of abar0_tan[tile][mt][d][:]. */
int stpde_jet_tan0_reduce(int ntiles, int MT, const float* abar0_tan, float* dW_aug, int ldw, int det /* as stpde_layer_desc.det */,
                          void* stream);

/* ---- backward of the gather: d latent (index_put accumulate, backward of :65-66) --------------------
 * xbar = sum_l W_s,l^T * abar_l(value stream); latent channels are scatter-added into dlatent
 * [B][n0][n1][n2][C] at the 8 corner nodes of each point.  nlayers <= 8. */
typedef struct {
  int ntiles, nlayers, C, n1, n2;
  int MT[8];
  int SP[8];
  int packed[8];   /* != 0: abar[l] is a packed ADJOINT buffer (stpde_layer_desc.packed) of S[l] streams */
  int S[8];        /* streams of a packed buffer (only read where packed[l] != 0) */
} stpde_xbar_desc;
/* abar / WsL_pack: HOST arrays of nlayers device pointers.  WsL_pack[l] = [MT_l][XL][64 lanes][4]: A operand of W_s,l^T
 * restricted to the latent channels, XL = ceil(C / 16) tiles of 16 channels (lane (g, j), register r holds
 * W_s,l[16 mt + 4 g + r][dim + 16 xl + j], zero beyond channel C - 1); the coordinate / bias columns get no adjoint. */
int stpde_lig_xbar_scatter(const stpde_xbar_desc* d, const float* const* abar, const float* const* WsL_pack,
                           const int* cell, float* dlatent, void* stream);
/* Deterministic variant (default of the Python host): the same xbar, but the latent channels of every corner row are
 * written to xrows [16 * ntiles][CP] (CP = C rounded up to a multiple of 4; row = 8 * point + corner) instead of being
 * scatter-added with fp32 atomics; stpde_lig_dlatent_reduce then sums them per NODE in a fixed order (corner 0..7, points
 * of the owning cell in ascending index), like the reference's deterministic CPU index_put_(accumulate=True) (:65-66).
 * perm [P] = point indices in stable cell order, start [n_nodes + 1] = first position of each cell id (cell id = linear
 * index of the cell's corner-0 node incl. batch, as written by stpde_lig_gather); dlatent is accumulated into (+=). */
int stpde_lig_xbar_rows(const stpde_xbar_desc* d, const float* const* abar, const float* const* WsL_pack,
                        float* xrows, void* stream);
int stpde_lig_dlatent_reduce(int B, int n0, int n1, int n2, int C, const float* xrows, const int* perm,
                             const int* start, float* dlatent, void* stream);

/* ---- a4/a5/a7 in ONE call per direction (lig_imnet_jet_fwd / lig_imnet_jet_bwd) ---------------------
 * The whole query path of src/local_implicit_grid.py:47-59 (gather -> IM-NET on all derivative streams -> corner-weighted
 * sum) for one chunk of query points, and its backward (what loss.backward(), experiments/rb2d/train.py:77, does through
 * it: weight gradients of fc0..fc5, latent-grid gradient).  Launch sequencing only: the kernels are the ones behind the
 * per-layer entry points above, issued in the same order; the per-layer entry points stay exported (profiling, tests).
 * All buffers are the caller's (stpde_lig_workspace); sizes in floats for a chunk of P points, nt = P / 2 row tiles,
 * S = 1 + S1 + S2 streams of cfg_mlp, block = 256 floats:
 *   X [nt][3][block] (XR: unused since round 5, may be NULL)   coef [P][16]   cw [P][8] (combined stream only, else NULL)   cell [P] int
 *   pre[0] = z0 stash [nt][MT_0][block] (training only)      pre[l], l >= 1: [nt][S][MT_l][block]
 *   backward scratch: abar2x / abar3x = sizes of pre[2] / pre[3] (fresh adjoint buffers of the fused tail), tan0
 *   [nt][MT_0][48], abar0 [nt][1 + S1][MT_0][block] (only when tan0 is NULL and S1 == 3), xrows [16 nt][CP], perm [P],
 *   start [n_nodes + 1], sort_tmp (stpde_lig_sort_tmp_bytes). */
typedef struct {
  int nlayers;                 /* 6: fc0 .. fc5 of src/implicit_net.py:31-36 */
  int cin, cout, nf16;         /* latent channels, outputs, nf / 16 */
  int KT[8], MT[8];            /* hidden k-tiles / output tiles of each layer */
  const float* Wh[8];          /* A-operand packs (see stpde_jet_layer_fwd); Wh[0] / WhT[0] unused */
  const float* WhT[8];
  const float* Ws[8];
  const float* WsL[8];
  const float* tanc[8];
  const void* Wh16[8];         /* bf16 packs of the wide layers or NULL */
  const void* WhT16[8];
  int mfma_bf16;               /* 0 / 1 / 3 as stpde_layer_desc.mfma_bf16 */
  int packed_mask;             /* bit l >= 1: pre[l] is a packed stash and the adjoint of layer l's rows a packed adjoint buffer
                                  (stpde_layer_desc.packed); bit 0: the value-stream adjoint of layer 0 (workspace.abar0x) is
                                  a packed adjoint buffer.  Only with mfma_bf16 == 1; the library serves 0, 30 and 31. */
  long dw_off[8];              /* offset (floats) of layer l's dW_aug block [16 MT][16 (KT + 3)] in dW_flat */
} stpde_imnet_plan;
typedef struct {
  float* X;
  float* XR;
  float* coef;
  float* cw;
  int* cell;
  float* pre[8];
  float* abar2x;
  float* abar3x;
  float* tan0;
  float* abar0;
  float* abar1x;   /* dgrad-first order / packed buffers: fresh adjoint buffer of fc1's output rows */
  float* abar0x;   /* dgrad-first order / packed_mask bit 0: fresh layer-0 adjoint [nt][MT_0][block] (the z0 stash stays intact) */
  float* xrows;
  int* perm;
  int* start;
  void* sort_tmp;
  unsigned long sort_tmp_bytes;
  float* abar4x;   /* packed buffers: adjoint buffer of fc4's output rows (abar2x / abar3x / abar4x / abar1x then hold packed
                      ADJOINT buffers: nt * S * MT_l * 512 bytes) */
} stpde_lig_workspace;
#define STPDE_F_STASH 1          /* forward: keep what the backward needs (z0) */
#define STPDE_F_VALUE_TILES 2    /* forward-only value queries: four row tiles per pass over the weights */
#define STPDE_F_FUSED_TAIL 4     /* fc3 -> fc4 -> fc5 in one kernel each way (nf = 16 / 32) */
#define STPDE_F_TAN0_ROWSUM 8    /* backward: layer-0 tangent adjoints as per-tile row sums (needs workspace.tan0) */
#define STPDE_F_DETERMINISTIC 16 /* backward: d latent by per-node sums in a fixed order instead of fp32 atomics */
#define STPDE_F_WGRAD 32         /* backward: compute the weight gradients */
#define STPDE_F_WGRAD_FP32 64    /* fp32x3 mode: keep the wide layers' weight gradients on the exact-fp32 MFMA */
/* Backward in two calls, "dgrad-first" (needs workspace.abar1x / abar0x, the fused tail and the tangent row sums):
 * PHASE_A = corner-reduction adjoint, fc5 weight gradient, the whole input-gradient chain into fresh buffers, d latent;
 * PHASE_B = the remaining weight gradients (fc4 .. fc0).  Between the two the caller may start the all-reduce of d latent. */
#define STPDE_F_PHASE_A 128
#define STPDE_F_PHASE_B 256
/* bf16 mode: do NOT use the fused backward of the first hidden layer (stpde_jet_fc1_bwd); the input gradient and the weight
 * gradient of that layer then run as two kernels.  A/B switch of the tests.  Both phases of a dgrad-first backward must carry
 * the same value of this bit and of STPDE_F_WGRAD: phase B skips fc1's weight gradient exactly when phase A's fused kernel
 * produced it. */
#define STPDE_F_NO_FC1_FUSED 512
/* backward: dW_flat addresses long accumulators (stpde_layer_desc.det): [sum of the layers' dW_aug elements][6] int64, layer l at
 * element offset dw_off[l]; bit-reproducible IM-NET weight gradients */
#define STPDE_F_DET 1024
/* exact fp32, one-call order with STPDE_F_WGRAD: run the second hidden layer's weight gradient and input gradient as ONE kernel
 * (stpde_jet_fc2_bwd) where stpde_jet_fc2_bwd_supported serves the layer and stpde_tune("fc2_bwd_fused") is not 2.  Opt-in: a
 * call without this bit keeps the two kernels.  Same bits either way with STPDE_F_DET. */
#define STPDE_F_FC2_FUSED 2048
/* cfg_mlp = streams the layer kernels carry, cfg_out = streams of `jets` (they differ for piecewise-linear activations,
 * see stpde_lig_reduce_fwd); jets points at the first point of the chunk inside [S_out][n_out][ldp]. */
int stpde_lig_imnet_jet_fwd(const stpde_imnet_plan* plan, const stpde_jet_cfg* cfg_mlp, const stpde_jet_cfg* cfg_out,
                            const stpde_gather_desc* gd, const float* pts, const float* latent,
                            const stpde_lig_workspace* ws, float* jets, long ldp, int flags, void* stream);
/* cfg_val = cfg_mlp with S1 = S2 = 0 (layer-0 weight gradient of the value stream).  dW_flat (zero-filled by the caller,
 * accumulated into; may be NULL), dlatent (accumulated into; may be NULL), act_param_bar as stpde_jet_layer_bwd. */
int stpde_lig_imnet_jet_bwd(const stpde_imnet_plan* plan, const stpde_jet_cfg* cfg_mlp, const stpde_jet_cfg* cfg_out,
                            const stpde_jet_cfg* cfg_val, const stpde_gather_desc* gd, const stpde_lig_workspace* ws,
                            const float* jets_bar, long ldp, float* dW_flat, float* dlatent, float* act_param_bar,
                            int flags, void* stream);
/* Cell sort of the deterministic d latent (replaces the torch.sort + index_add_ + cumsum of the round-2 host): perm [P] =
 * point indices in stable cell order, start [n_nodes + 1] = number of points in cells < c; tmp = device scratch of at
 * least stpde_lig_sort_tmp_bytes(P, n_nodes) bytes. */
unsigned long stpde_lig_sort_tmp_bytes(int P, long n_nodes);
int stpde_lig_cell_sort(int P, long n_nodes, const int* cell, int* perm, int* start, void* tmp, unsigned long tmp_bytes,
                        void* stream);

/* ---- a2/a3 for any dim 1..4: plain multilinear interpolation ---------------------------------------
 * Replaces regular_nd_grid_interpolation (src/regular_nd_grid_interpolation.py:81-104) and the three outputs
 * of ..._coefficients (:14-78).  grid [B][n_0..n_{dim-1}][C], pts [B*N][dim].  Any output pointer may be NULL. */
typedef struct {
  int P, N, B, dim, C;
  int n[4];
  float lo_c[4], hi_c[4], cube[4];
} stpde_interp_desc;
int stpde_interp_fwd(const stpde_interp_desc* d, const float* grid, const float* pts, float* out /*[P][C]*/,
                     float* corner_values /*[P][2^dim][C]*/, float* weights /*[P][2^dim]*/,
                     float* x_relative /*[P][2^dim][dim]*/, void* stream);
/* dgrid[node] += w_j * out_bar[p] (out_bar [P][C]) and/or corner_bar[p][j] ([P][2^dim][C]); either may be NULL. */
int stpde_interp_bwd_grid(const stpde_interp_desc* d, const float* pts, const float* out_bar,
                          const float* corner_bar, float* dgrid, void* stream);

/* ---- a1/a2/a4 for dim = 1, 2, 4: VALUE-ONLY local-implicit-grid queries -------------------------------
 * The reference states query_local_implicit_grid for [b, n1..nd, c] grids (src/local_implicit_grid.py:10-61; its unit test
 * runs a 4-d query).  These two calls put such a query on the layer kernels above in their one-stream (value) configuration:
 *   stpde_lig_gather_nd      clip, cell index, corner gather, relative coordinates -> X [ntiles][3][64][4], the SAME
 *                            augmented-input image stpde_lig_gather writes, features [r(D) ; latent(C) ; 1] in the same slots
 *                            (D + C + 1 <= 36), and the corner weights cw [ntiles][16] (one per row)
 *   stpde_jet_layer_fwd / stpde_jet_tail_fwd_p   unchanged, S1 = S2 = 0 or the value-tile mode, over ntiles row tiles
 *   stpde_lig_reduce_nd_fwd  y[ch * ldp + p] = sum_j cw[row(p, j)] * out_pre[row(p, j)][ch], fp32, in corner order
 * A row tile holds 16 >> D points: row j = corner j & (2^D - 1) (first axis most significant, as stpde_interp_fwd) of point
 * tile * (16 >> D) + (j >> D).  pts [P][D] is a chunk of the [B * N] point list starting at p_base; latent
 * [B][n_0..n_{D-1}][C] contiguous; lo_c / hi_c / cube as for stpde_lig_gather (xmin must be 0).  ntiles may exceed
 * ceil(P / (16 >> D)) by up to 3 (the value-tile mode wants a multiple of 4): rows of points >= P are written as zeros
 * with weight 0 and belong to no output point; nothing is read or written past P points or ntiles tiles.  The cell index
 * is clamped to [0, n_k - 2] after the float clip and the batch index to B - 1, so no coordinate value -- NaN, infinite,
 * outside the box -- forms an address outside the latent grid.  No derivative streams in these two calls (dim = 1, 2: the
 * block after the next; dim = 4 requests take the composed formulation, local_implicit_grid.py); the training backward of the value stream is the next block.  Refused with STPDE_E_BADARG: D other than 1, 2, 4; P < 1; ntiles
 * outside [ceil(P / (16 >> D)), that + 3]; an axis with fewer than 2 nodes; D + C + 1 > 36; B * prod(n) or p_base + P
 * beyond 31 bits; n_out outside 1..16; ldp < P; a null pointer. */
typedef struct {
  int D, P, N, B, C;
  int p_base; /* global index of pts[0]: batch of point p is min((p_base + p) / N, B - 1) */
  int ntiles;
  int n[4];
  float lo_c[4], hi_c[4], cube[4];
} stpde_gather_nd_desc;
int stpde_lig_gather_nd(const stpde_gather_nd_desc* d, const float* pts, const float* latent, float* X,
                        float* cw /* [ntiles][16] */, void* stream);
int stpde_lig_reduce_nd_fwd(int D, int P, int ntiles, int n_out, const float* out_pre /* fc5 rows [ntiles][64][4] */,
                            const float* cw, float* y, long ldp, void* stream);

/* ---- training backward on the same grids (dim = 1, 2, 4; value stream only) -----------------------------------------
 * Between these three calls run, unchanged and in their S1 = S2 = 0 configuration over ntiles row tiles, stpde_jet_layer_fwd
 * with the z0 stash / stpde_jet_tail_fwd_p (forward), stpde_jet_wgrad, stpde_jet_layer_bwd / _bwd_to, stpde_jet_tail_bwd_p,
 * stpde_lig_xbar_rows and stpde_lig_cell_sort (backward).  Row numbering is the gather's: tile * 16 + j = point * 2^D + corner.
 *   stpde_lig_reduce_nd_bwd      adjoint of stpde_lig_reduce_nd_fwd: lane (g, j), register r of tile t of abar_out receives
 *                                cw[16 t + j] * y_bar[(4 g + r) * ldp + p], p = t * (16 >> D) + (j >> D); zeros where p >= P
 *                                or 4 g + r >= n_out.  EVERY float of the ntiles blocks is written (the buffer held the
 *                                forward's fc5 rows); nothing is read for p >= P.  Checks of stpde_lig_reduce_nd_fwd.
 *   stpde_lig_cell_nd            cell[p] = linear index, batch included, of the corner-0 node of the cell of point p: the
 *                                same clip, cell index and batch clamp as stpde_lig_gather_nd (so < B * prod(n) for every
 *                                coordinate value); the counterpart of the `cell` output of stpde_lig_gather.  Checks of
 *                                stpde_lig_gather_nd.
 *   stpde_lig_dlatent_reduce_nd  stpde_lig_dlatent_reduce for 2^D corners: dlatent[node] += sum over corners 0 .. 2^D - 1
 *                                (first axis most significant; a corner whose owning cell lies outside [0, n_k - 2] on any
 *                                axis is skipped) and the points of the owning cell in ascending perm position of
 *                                xrows[perm[q] * 2^D + corner], fp32, fixed order: bit-reproducible.  n = HOST array of the D
 *                                axis lengths.  xrows is what stpde_lig_xbar_rows wrote for the chunk, [16 * ntiles][CP]
 *                                floats (padding rows of the last tiles included; CP = C rounded up to a multiple of 4); perm
 *                                [P] / start [n_nodes + 1] from stpde_lig_cell_sort on the output of stpde_lig_cell_nd.
 *                                Refused: D other than 1, 2, 4; an axis with fewer than 2 nodes; C outside 1..64; B < 1;
 *                                B * prod(n) beyond 31 bits; a null pointer.
 * stpde_lig_xbar_rows serves C <= 32, so training on these grids needs in_features <= 32.  There is no atomic variant of the
 * d-latent sum on these grids. */
int stpde_lig_reduce_nd_bwd(int D, int P, int ntiles, int n_out, const float* y_bar, long ldp, const float* cw,
                            float* abar_out /* [ntiles][64][4] */, void* stream);
int stpde_lig_cell_nd(const stpde_gather_nd_desc* d, const float* pts, int* cell /* [P] */, void* stream);
int stpde_lig_dlatent_reduce_nd(int D, int B, const int* n /* [D] on the host */, int C, const float* xrows, const int* perm,
                                const int* start, float* dlatent, void* stream);

/* ---- coordinate derivatives on the same grids for dim = 1, 2 (forward only) -------------------------------------------
 * y and its first and selected second derivatives w.r.t. the query coordinates (what the src/pde.py:8-9 sweeps compute) in
 * one forward pass: stpde_lig_gather_nd, stpde_lig_coef_nd, the layer kernels / stpde_jet_tail_fwd_p unchanged in a stream
 * set (3, 0), (3, 2), (3, 4) or (3, 6) over ntiles row tiles of 16 >> D points, stpde_lig_reduce_nd_jet_fwd.  The layer
 * kernels carry three tangent streams whatever D is: the caller's `tanc` packs must hold zeros for the columns d >= D, which
 * makes the streams of those axes identically zero.  Not served (the caller keeps the composed formulation): D = 4 (by
 * these two: it has entry points of its own, further below), the combined second-order stream (its per-row weights are
 * indexed two points per tile) and bf16 operands; the backward is below.
 *   stpde_lig_coef_nd            coef[p][16] of stpde_lig_gather for point p of the chunk, from the same clip and cell index
 *                                as stpde_lig_gather_nd: {om[0][k], om[1][k], dom[0][k], dom[1][k], kap[k]} at 0 / 3 / 6 / 9 /
 *                                12 + k for k < D; om = 1, dom = 0, kap = 0 for the axes k >= D; entry 15 = 0.  Checks of
 *                                stpde_lig_gather_nd, and D other than 1, 2 refused.
 *   stpde_lig_reduce_nd_jet_fwd  jets[(s * n_out + ch) * ldp + p] = sum over the 2^D corners, in corner order, of the terms of
 *                                stpde_lig_reduce_fwd (w, dw, the d2w cross terms, kappa factors) on row
 *                                ((p % (16 >> D)) << D) | corner of tile p / (16 >> D) of out_pre [ntiles][S_mlp][1][256].
 *                                Stream order of dim = 3: value, d/dq_0, d/dq_1, d/dq_2, then the pairs of cfg.  The streams
 *                                of the axes >= D are stored as +0.0 whatever the inputs hold (never computed as 0 * f).
 *                                S_mlp < 1 + S1 + S2: streams the layer buffers do not hold count as zero (piecewise-linear
 *                                activations).  Refused with STPDE_E_BADARG: D other than 1, 2; a null pointer; P < 1 or
 *                                P > ntiles * (16 >> D) or ntiles > ceil(P / (16 >> D)) + 3; n_out outside 1..16; ldp < P;
 *                                S1 other than 0, 3; S2 other than 0, 2, 4, 6 (or != 0 with S1 = 0); cfg.combo set; a pair
 *                                index outside 0 .. D - 1; S_mlp outside 1 .. 1 + S1 + S2.
 * Nothing is read or written for p >= P; every index is bounded for every coordinate value (NaN, infinite, huge). */
int stpde_lig_coef_nd(const stpde_gather_nd_desc* d, const float* pts, float* coef /* [P][16] */, void* stream);
int stpde_lig_reduce_nd_jet_fwd(const stpde_jet_cfg* cfg, int S_mlp, int D, int P, int ntiles, int n_out,
                                const float* out_pre /* [ntiles][S_mlp][1][256] */, const float* coef,
                                float* jets /* [S][n_out][ldp] */, long ldp, void* stream);

/* ---- coordinate derivatives on 4-d grids (3-d space + time), forward only ------------------------------------------------
 * The layer kernels carry three first-order streams; a 4-d grid has four axes.  A request runs as up to four PASSES over the one
 * image of stpde_lig_gather_nd (one point = one 16-row tile): each pass is the layer kernels / stpde_jet_tail_fwd_p unchanged in
 * a stream set (3, 0), (3, 2), (3, 4) or (3, 6) whose `tanc` packs hold the skip-block columns a0 < a1 < a2 of the pass's axis
 * triple (slot i of the pass = axis a_i), followed by stpde_lig_reduce_nd4_jet_fwd.  Every mixed second derivative needs the
 * first-order streams of its two axes only, and the four triples of {0, 1, 2, 3} hold all six mixed pairs.
 *   stpde_lig_coef_nd4            coef[p][24] = {om[0][k], om[1][k], dom[0][k], dom[1][k], kap[k]} at 0 / 4 / 8 / 12 / 16 + k for
 *                                 the four axes, entries 20 .. 23 = 0, from the same clip and cell index as stpde_lig_gather_nd.
 *                                 Checks of stpde_lig_gather_nd, and D other than 4 refused.
 *   stpde_lig_reduce_nd4_jet_fwd  the corner sum of one pass over the 16 corners, in corner order, with the terms of
 *                                 stpde_lig_reduce_nd_jet_fwd: the weight is the product over all four axes, dw / d2w are taken
 *                                 for the pass's axes.  Stream dst_value of jets receives the value, dst_first[i] the derivative
 *                                 along axis[i], dst_pair[k] the second derivative along (pair0[k], pair1[k]); -1 = not stored.
 *                                 A pass writes no other stream, so several passes fill one jets tensor.  S_mlp = 4 with
 *                                 npairs > 0: the layer buffers hold no second-order streams (piecewise-linear activations),
 *                                 they count as zero.  Refused with STPDE_E_BADARG: D other than 4; a null pointer; P < 1 or
 *                                 P > ntiles or ntiles > P + 3; n_out outside 1..16; ldp < P; an axis triple that is not
 *                                 strictly increasing inside 0..3; npairs other than 0, 2, 4, 6; S_mlp other than 4 and
 *                                 4 + npairs; S outside 1..15; a pair axis outside the triple; a destination stream outside
 *                                 [-1, S) or named twice.
 * Nothing is read or written for p >= P; every index is bounded for every coordinate value (NaN, infinite, huge). */
typedef struct {
  int axis[3];             /* the pass's axis triple, strictly increasing, each < 4 */
  int npairs;              /* S2 of the pass's stream set: 0, 2, 4 or 6 (padded by repeating a pair, destination -1) */
  int pair0[6], pair1[6];  /* axes of pair k, both inside the triple */
  int S_mlp;               /* streams of out_pre: 4 + npairs, or 4 */
  int S;                   /* streams of the jets tensor */
  int dst_value, dst_first[3], dst_pair[6]; /* stream of jets to write, or -1 */
} stpde_nd4_pass_desc;
int stpde_lig_coef_nd4(const stpde_gather_nd_desc* d, const float* pts, float* coef /* [P][24] */, void* stream);
int stpde_lig_reduce_nd4_jet_fwd(const stpde_nd4_pass_desc* d, int D, int P, int ntiles, int n_out,
                                 const float* out_pre /* [ntiles][S_mlp][1][256] */, const float* coef,
                                 float* jets /* [S][n_out][ldp] */, long ldp, void* stream);

/* ---- training through those derivatives (dim = 1, 2): the adjoint of stpde_lig_reduce_nd_jet_fwd ------------------------
 * Between stpde_lig_reduce_nd_jet_bwd and the d latent calls of the value path (stpde_lig_xbar_rows on the value-stream
 * adjoints, stpde_lig_cell_nd, stpde_lig_cell_sort, stpde_lig_dlatent_reduce_nd) runs the per-kernel backward of dim = 3 in
 * the call's stream set over ntiles row tiles: stpde_jet_layer_bwd / _bwd_to, stpde_jet_tail_bwd_p, and the weight
 * gradients through the two `_nd` entry points below.  What those kernels do with the tangent streams of the axes k >= D
 * (all of them carry three): the forward streams are identically zero (`tanc` columns), their adjoints are exact zeros
 * (stpde_lig_reduce_nd_jet_bwd writes +0.0, no pair names such an axis, so no activation-jet cross term feeds them), and
 * the one place that would ADD something of theirs to a latent channel's weight column -- the row sums of tangent adjoint k
 * into raw-input column k of a layer's weight-gradient block -- is told the number of coordinate axes.
 *   stpde_lig_reduce_nd_jet_bwd  abar_out [ntiles][S_mlp][1][256] (over the forward's out_pre): lane (g, j), register r of
 *                                tile t, stream s = the adjoint of output feature 4 g + r of row j, which belongs to point
 *                                p = t * (16 >> D) + (j >> D), corner j & (2^D - 1); the coefficient algebra of
 *                                stpde_lig_reduce_bwd.  EVERY float of the buffer is written: zeros for features >= n_out,
 *                                for padding rows (p >= P) and for the tangent streams of the axes k >= D.  The rows
 *                                jets_bar[1 + k], k >= D, are never read (the forward stored +0.0 there).  S_mlp < 1 + S1 +
 *                                S2: the second-order cotangents still reach streams 0 .. 3 through the weight cross terms.
 *                                Argument checks of stpde_lig_reduce_nd_jet_fwd; nothing is read for p >= P.
 *   stpde_jet_wgrad_nd           stpde_jet_wgrad with ncoord = D coordinate axes (1 .. 3; 3 = stpde_jet_wgrad): the row sums
 *                                of tangent-stream adjoint k are added to raw-input column k for k < ncoord only.  ncoord != 3
 *                                with plain bf16 operands or packed buffers: STPDE_E_UNSUPPORTED.
 *   stpde_jet_tan0_reduce_nd     stpde_jet_tan0_reduce likewise: columns k < ncoord only. */
int stpde_lig_reduce_nd_jet_bwd(const stpde_jet_cfg* cfg, int S_mlp, int D, int P, int ntiles, int n_out,
                                const float* jets_bar /* [S][n_out][ldp] */, long ldp, const float* coef,
                                float* abar_out /* [ntiles][S_mlp][1][256] */, void* stream);
int stpde_jet_wgrad_nd(const stpde_layer_desc* d, int SP, const float* abar_out, const float* in_pre, const float* X,
                       const float* tanc0, float* dW_aug, const float* cw, int ncoord, void* stream);
int stpde_jet_tan0_reduce_nd(int ntiles, int MT, const float* abar0_tan, float* dW_aug, int ldw, int det, int ncoord, void* stream);

/* ---- a10: 3-D convolution of the U-Net encoder (src/unet3d.py:39-56: nn.Conv3d 1x1x1 and 3x3x3/pad 1, stride 1)
 * Activations are channels-last: x [B][T][Z][X][Ci], y [B][T][Z][X][Co], Ci and Co multiples of 16.
 * Implicit GEMM on v_mfma_f32_16x16x4_f32: y^T[Co x 16 voxels] = sum_tap W_tap[Co x Ci] * x_tap^T[Ci x 16 voxels].
 * w_pack [taps][Ci/16][Co/16][64][4] (A-operand image of W[:, :, tap]); bias [Co] or NULL.
 * The input-gradient is the same kernel called with the transposed, tap-flipped pack (no bias). */
typedef struct {
  int B, T, Z, X, Ci, Co, ksize; /* ksize 1 or 3 */
  /* Deterministic mode (round 6; 0 = off).  != 0: every sum the kernels of this call accumulate with atomics -- dW / dbias of
   * the weight-gradient calls, out_sums / m_bsum of stpde_conv3d_fused -- goes to ORDER-INDEPENDENT long accumulators instead
   * of fp32 / fp64 atomics: the destination pointer then addresses STPDE_DET_K (6) zero-filled signed 64-bit integers per
   * element (48 bytes instead of 4; element e at windows [6 e, 6 e + 6)), the result is bit-identical from run to run, and
   * stpde_det_finalize turns an accumulator array into fp32 (statistics / backward sums are read by the BatchNorm kernels
   * directly: a single replica [2][C][6] in the same scratch).  The forward does not split its taps over workgroups. */
  int det;
  /* Operand mode of the 3x3x3 GEMM products (0 = fp32 operands on v_mfma_f32_16x16x4_f32, today's path).  1 = bf16 operands:
   * every product of the call takes both operands rounded to bf16 (round-to-nearest-even, v_cvt_pk_bf16_f32, NaN stays NaN)
   * and accumulates in fp32 on v_mfma_f32_16x16x16_bf16 (one instruction per four fp32 k-steps, same tiles, same order):
   *   forward         y  = bias + sum_tap bf16(W_tap) . bf16(x_tap)   (bias, statistics epilogue, tap-split atomics in fp32)
   *   input gradient  dx = sum bf16(W^T) . bf16(gy)                   (the EPI 2 mask / BatchNorm-backward sums from the fp32
   *                                                                    result)
   *   weight grad.    dW = sum_vox bf16(ybar) x bf16(x_shifted)       (fp32 or deterministic long accumulators);
   *                   dbias stays the fp32 sum of the UNROUNDED ybar
   * Activations, packs and outputs stay fp32; 1x1x1 convolutions (HBM-bound) have no bf16 mode: mfma_bf16 = 1 with ksize 1 is
   * refused (STPDE_E_BADARG), as is any value other than 0 / 1 (3 is reserved for an exact-split fp32x3 mode). */
  int mfma_bf16;
} stpde_conv3d_desc;
/* acc [n][STPDE_DET_K] long accumulators (a deterministic-mode destination, see stpde_conv3d_desc.det) -> out [n] fp32. */
#define STPDE_DET_K 6
int stpde_det_finalize(const void* acc, long n, float* out, void* stream);
int stpde_conv3d_fwd(const stpde_conv3d_desc* d, const float* x, const float* w_pack, const float* bias, float* y,
                     void* stream);
/* dW[tap][Co][Ci] += sum_voxels ybar[v][co] * x[v + offset(tap)][ci]  (fp32 atomics; caller zero-fills dW). */
int stpde_conv3d_wgrad(const stpde_conv3d_desc* d, const float* x, const float* ybar, float* dW, void* stream);
/* The same + the bias gradient: dbias[Co] += sum over the voxels of ybar (fp32 atomics; caller zero-fills), taken from the
 * ybar fragments the kernel loads anyway -- replaces a separate reduction pass over ybar (the reference computes it inside
 * its convolution backward, torch.nn.Conv3d). */
int stpde_conv3d_wgrad_bias(const stpde_conv3d_desc* d, const float* x, const float* ybar, float* dW, float* dbias,
                            void* stream);

/* ---- a10 (round 4): the convolutions of one ResBlock3D with its BatchNorm work folded in (src/unet3d.py:39-56:
 * conv1-bn1-relu-conv2-bn2-relu-conv3-bn3 + shortcut, relu).  One call = one convolution of the chain plus what the
 * BatchNorm next to it would otherwise do in passes of its own over the same tensor:
 *   out_sums  the per-channel sums of y and y^2 the following BatchNorm needs, from the accumulator tiles (doubles,
 *             [STPDE_BN_REP][2][Co], caller zero-fills; every wave sums around its own first voxel and converts in fp64)
 *   in_sums   ksize 1: x is the RAW output of the previous convolution; its training-mode BatchNorm + ReLU are applied to
 *             the operand as it is loaded: x' = max(0, (x - mean) * (rstd * gamma) + beta), mean / rstd from in_sums over
 *             the N = B*T*Z*X voxels; the call writes in_stat = [mean; rstd] and updates the running statistics
 *   y2        ksize 1: a second convolution of the same input (conv1 and the shortcut of a block: x is read once)
 *   x2        ksize 1: a second input, y = W x + W2 x2 (the input gradient of a block = conv1's + the shortcut's)
 *   m         input-gradient convolutions: y is the gradient of act = relu(bn(m)); the call stores dz = y * [act > 0] and adds
 *             sum(dz), sum(dz * xhat) to m_bsum ([STPDE_BN_REP][2][Co] floats, zero-filled) -- the reduction pass of
 *             stpde_bn_bwd.  Volumes small enough for the tap-split kernel cannot do this in their epilogue:
 *             *epilogue_done = 0 then (y holds the unmasked gradient) and the caller runs the full stpde_bn_bwd.
 * Unused features: NULL pointers / zero channel counts. */
typedef struct {
  stpde_conv3d_desc d;
  const float* x;
  const float* w_pack;
  const float* bias;
  float* y;
  const float* x2;       /* [voxels][Ci2] */
  const float* w2_pack;  /* [Ci2/16][Co/16][64][4] */
  float* y2;             /* [voxels][Co2] */
  const float* wo2_pack; /* [Ci/16][Co2/16][64][4] */
  const float* bias2;
  const double* in_sums;
  const float* in_gamma; /* NULL = 1 */
  const float* in_beta;  /* NULL = 0 */
  float* in_running_mean; /* NULL: no running statistics */
  float* in_running_var;
  float* in_stat;        /* [2][Ci] */
  double* out_sums;
  const float* m;        /* [voxels][Co] */
  const float* m_stat;   /* [2][Co]: mean, rstd of m */
  const float* m_gamma;
  const float* m_beta;
  float* m_bsum;
  int Ci2, Co2;
  float in_eps, in_momentum;
} stpde_conv3d_fused_args;
int stpde_conv3d_fused(const stpde_conv3d_fused_args* a, int* epilogue_done, void* stream);
/* Weight (+ bias) gradient of a 1x1x1 convolution whose input was x' = max(0, bn(x)) applied on load (in_stat = [mean; rstd]
 * of x as written by stpde_conv3d_fused, in_gamma / in_beta nullable): the same transform on the operand here. */
int stpde_conv3d_wgrad_onload(const stpde_conv3d_desc* d, const float* x, const float* ybar, float* dW, float* dbias,
                              const float* in_stat, const float* in_gamma, const float* in_beta, void* stream);

/* ---- a10: BatchNorm3d (+ residual add) (+ ReLU) of the ResBlock3D chain (src/unet3d.py:39-56) -------------
 * Channels-last x [N][C], N = B*T*Z*X, C a power of two in [16, 512].
 * forward:  y = act(bn(x) [+ residual]);  training != 0: batch statistics (biased variance for the normalisation,
 *           running_mean / running_var updated in place with torch's momentum rule and the unbiased variance);
 *           training == 0: running statistics.  sums: [STPDE_BN_REP][3][C] scratch (training), stat: [2][C] receives mean, rstd.
 * backward: dz = dy * [y > 0] (relu) ; dresidual = dz ; dx, dgamma, dbeta as torch's batch_norm backward
 *           (training: with the batch-statistics terms, evaluation: without).  bsum: [STPDE_BN_REP][2][C] scratch.
 * The reduction kernels spread their per-block atomics over STPDE_BN_REP replicas of the sums (one copy made ~1000 blocks
 * queue on 2 C addresses); the elementwise kernels add the replicas up in a fixed order.
 * Any of residual, gamma, beta, dx, dresidual, dgamma, dbeta may be NULL. */
#define STPDE_BN_REP 16
typedef struct {
  long N;
  int C, training, relu;
  float eps, momentum;
  int scratch_zeroed;   /* != 0: the caller hands over zero-filled sums / bsum scratch (e.g. slices of one buffer cleared once
                           per step), so no memset is queued in front of the reduction kernels */
  int stats_mode;       /* forward, training: 0 = sums is the float scratch above; 1 = sums is double [STPDE_BN_REP][2][C]
                           (sum of x, sum of x^2; the format stpde_conv3d_fused writes) and this call fills it; 2 = the same
                           format, already complete (no statistics pass) */
  int reduce_done;      /* backward: bsum is already complete and dy already carries the ReLU mask (stpde_conv3d_fused, m):
                           only the elementwise pass runs; pass relu = 0 */
  int det;              /* deterministic mode (stpde_conv3d_desc.det): sums / bsum hold long accumulators -- forward statistics
                           [2][C][6] int64 (sum x, sum x^2; stats_mode 1 / 2 only), backward sums [2][C][6] -- in the same
                           zero-filled scratch */
} stpde_bn_desc;
int stpde_bn_fwd(const stpde_bn_desc* d, const float* x, const float* residual, const float* gamma, const float* beta,
                 float* running_mean, float* running_var, float* sums, float* stat, float* y, void* stream);
int stpde_bn_bwd(const stpde_bn_desc* d, const float* x, const float* y, const float* dy, const float* gamma,
                 const float* stat, float* bsum, float* dx, float* dresidual, float* dgamma, float* dbeta, void* stream);

/* ---- a10: max pooling / nearest up-sampling between the U-Net levels (src/unet3d.py:163-176, 216-238) ----------
 * Channels-last [B][T][Z][X][C], C % 4 == 0.  The descriptor holds the dimensions of the SMALL tensor (pooled output /
 * up-sampling input) and the integer factors (1..4) per dimension; the big tensor is [B][T*ft][Z*fz][X*fx][C].
 * mode 0: max-pool forward (in = big, out = small)       mode 1: max-pool backward (in = d small, aux = forward
 * input, out = d big; ties go to the first maximum of the window like torch)
 * mode 2: nearest up-sampling forward (in = small, out = big)   mode 3: its backward (in = d big, out = d small). */
typedef struct {
  int B, T, Z, X, C, ft, fz, fx;
} stpde_resample_desc;
int stpde_resample3d(const stpde_resample_desc* d, int mode, const float* in, const float* aux, float* out,
                     void* stream);

/* ---- a7/a8/a9: PDE residuals from the jet streams ---------------------------------------------------
 * Replaces the elementwise algebra that src/pde.py:115-143 evaluates through the lambdified equation strings once the
 * derivatives are known (e.g. the four Rayleigh-Benard residuals of experiments/rb2d/physics.py:26-57), and its
 * autograd backward.  The host compiles every equation into ONE straight-line program in SSA form: instruction i
 * produces value i from earlier values a, b (indices < i):
 *   JET   value = jets[a * ld_stream + b * ld_channel + p]   (a = stream, b = output channel)
 *   X     value = x[p][a]            CONST value = c
 *   ADD SUB MUL DIV (a, b)   NEG (a)   POWI value = v[a]^b (integer b)   SIN COS EXP LOG SQRT TANH ABS (a)
 *   OUT   residual b of the point = v[a]
 * Appended after OUT (nothing above is renumbered; values and adjoints follow torch and its autograd):
 *   TAN SINH COSH ASIN ACOS ATAN (a)   ATAN2 value = atan2(v[a], v[b])
 *   POWC  value = v[a]^c (real constant c: its integer part by POWI's multiplications, the fraction through powf, so an
 *         integral c is exact); adjoint c * v[a]^(c-1), never divided by v[a]: v[a] = 0 is regular for c >= 1
 *   POW   value = v[a]^v[b]; adjoints as torch.pow (0 into the base where v[b] == 0, 0 into the exponent where
 *         v[a] == 0 and v[b] >= 0)
 *   MIN MAX (a, b)  NaN propagates; on a tie each operand receives half the cotangent (torch.minimum / maximum)
 *   SIGN (a)  sign(0) = 0, sign(NaN) = NaN     STEP (a)  Heaviside with H(0) = 1/2, H(NaN) = NaN; both have adjoint 0
 * MIN MAX SIGN STEP are fixed IEEE sequences like ABS; the others go through the device's math library.
 * Appended after STEP (Piecewise with relational conditions; comparisons and selects only, fixed IEEE sequences):
 *   LT LE EQ NE (a, b)  mask = 1.0 where v[a] < / <= / == / != v[b], else 0.0 (a NaN operand: 0.0, for NE 1.0); > and >= are
 *         LT and LE with a and b swapped
 *   AND OR (a, b)  NOT (a)  on masks (an operand counts as true where it is != 0); the result is 1.0 or 0.0, never NaN
 *   SEL   value = v[a] != 0 ? v[then] : v[else], the two value indices packed into b: then = b & 0xffff, else = b >> 16
 *         (STPDE_RES_SEL_THEN / _ELSE; indices are below STPDE_RES_MAX_INS).  Both operands are evaluated.  Adjoint as
 *         torch.where: the selected operand receives the cotangent, the other exactly +0 (a select, not a product with the
 *         mask: a NaN cotangent does not reach the operand not taken), nothing reaches the mask
 *   STEPC (a)  Heaviside with H(0) = c, H(NaN) = NaN (STEP's c is 0 and means 1/2)
 *   Masks, comparison operands and STEPC have adjoint 0.
 * res [n_eq][P]; the adjoint adds d loss / d jets into jets_bar (same layout as jets, zero-filled by the caller).
 * The coordinates x are not differentiated here (the jets already are the coordinate derivatives).
 * Coefficients in device memory (the _coef entry points only): a late-bound CONST -- op = CONST, b = 1, a = k, c = 0 -- is
 *   the value of coefficient k of the stpde_res_coefs record: value[k][0] for every point, or value[k][p / n_per_batch] (one per
 *   batch element) where per_batch[k] != 0.  No opcode is added: every other program holds CONST with a = b = 0, and
 *   stpde_residual_fwd / _bwd read a CONST's c whatever its b.  The value is loaded when the kernel runs, not when the program
 *   is compiled: an in-place update is seen by the next launch, and by the next replay of a captured one.  The adjoint adds
 *   sum over the points of d loss / d coefficient into bar[k][0] (or [p / n_per_batch]): one sum per 256-point block, then
 *   one atomic per block. */
#define STPDE_RES_MAX_INS 192
enum {
  STPDE_RES_JET = 0, STPDE_RES_X, STPDE_RES_CONST, STPDE_RES_ADD, STPDE_RES_SUB, STPDE_RES_MUL, STPDE_RES_DIV,
  STPDE_RES_NEG, STPDE_RES_POWI, STPDE_RES_SIN, STPDE_RES_COS, STPDE_RES_EXP, STPDE_RES_LOG, STPDE_RES_SQRT,
  STPDE_RES_TANH, STPDE_RES_ABS, STPDE_RES_OUT,
  STPDE_RES_TAN, STPDE_RES_SINH, STPDE_RES_COSH, STPDE_RES_ASIN, STPDE_RES_ACOS, STPDE_RES_ATAN, STPDE_RES_ATAN2,
  STPDE_RES_POWC, STPDE_RES_POW, STPDE_RES_MIN, STPDE_RES_MAX, STPDE_RES_SIGN, STPDE_RES_STEP,
  STPDE_RES_LT, STPDE_RES_LE, STPDE_RES_EQ, STPDE_RES_NE, STPDE_RES_AND, STPDE_RES_OR, STPDE_RES_NOT,
  STPDE_RES_SEL, STPDE_RES_STEPC
};
#define STPDE_RES_SEL_THEN(b) ((int)((unsigned)(b) & 0xffffu))
#define STPDE_RES_SEL_ELSE(b) ((int)((unsigned)(b) >> 16))
typedef struct {
  int op, a, b;
  float c;
} stpde_res_ins;
int stpde_residual_fwd(const stpde_res_ins* prog_dev, int nins, int n_eq, int n_out, int P, const float* jets,
                       long ld_stream, long ld_channel, const float* x /* [P][3] or NULL */, float* res, void* stream);
int stpde_residual_bwd(const stpde_res_ins* prog_dev, int nins, int n_eq, int n_out, int P, const float* jets,
                       long ld_stream, long ld_channel, const float* x, const float* res_bar, float* jets_bar,
                       void* stream);
/* The same for a program with late-bound CONSTs.  The record is caller-owned host memory, read during the call.  The points
 * are B batch elements of n_per_batch each, batch-major: P = B * n_per_batch (anything else, n outside 1 .. 8 or a null
 * value[k] is STPDE_E_BADARG). */
#define STPDE_RES_MAX_COEF 8
typedef struct {
  int n;                 /* coefficients read by the program, <= STPDE_RES_MAX_COEF */
  int n_per_batch;       /* N; P must equal B * N */
  int det;               /* bwd: bar[k] address long accumulators (as STPDE_LOSS_DET), not floats */
  int per_batch[STPDE_RES_MAX_COEF];      /* 0: value[k][0] for every point; 1: value[k][b] */
  const float* value[STPDE_RES_MAX_COEF]; /* device */
  float* bar[STPDE_RES_MAX_COEF];         /* bwd only; NULL = no gradient wanted; zero-filled by the caller */
} stpde_res_coefs;
int stpde_residual_coef_fwd(const stpde_res_ins* prog_dev, int nins, int n_eq, int n_out, int P, const float* jets,
                            long ld_stream, long ld_channel, const float* x, float* res, const stpde_res_coefs* coefs,
                            void* stream);
int stpde_residual_coef_bwd(const stpde_res_ins* prog_dev, int nins, int n_eq, int n_out, int P, const float* jets,
                            long ld_stream, long ld_channel, const float* x, const float* res_bar, float* jets_bar,
                            const stpde_res_coefs* coefs, void* stream);

/* ---- a11: loss reductions of the train step (experiments/rb2d/train.py:69-76) -------------------------------
 * out_sum += sum_i f(a[i] - b[i]) with f = |d| (L1), d^2 (L2) or smooth-l1 with beta 1 (b == NULL: against 0);
 * a SUM, not a mean: the caller divides by the GLOBAL element count (point-sharded multi-GPU step).  The caller
 * zero-fills out_sum.  stpde_loss_grad writes grad_a[i] = *grad_sum_dev * f'(a[i] - b[i]) (sign(0) = 0 like torch). */
#define STPDE_LOSS_L1 0
#define STPDE_LOSS_L2 1
#define STPDE_LOSS_HUBER 2
/* kind | STPDE_LOSS_DET (stpde_loss_sum only): out_sum addresses ONE long accumulator (six zero-filled 64-bit integers, see
 * stpde_conv3d_desc.det) instead of a float -- the block sums are added with integer atomics, bit-identical from run to run;
 * stpde_det_finalize(out_sum, 1, ...) gives the float. */
#define STPDE_LOSS_DET 16
int stpde_loss_sum(int kind, long n, const float* a, const float* b, float* out_sum, void* stream);
int stpde_loss_grad(int kind, long n, const float* a, const float* b, const float* grad_sum_dev, float* grad_a,
                    void* stream);

/* ---- N1: train-step tail -- gradient value clipping + Adam in one pass ---------------------------------
 * Replaces torch.nn.utils.clip_grad_value_ + optim.Adam.step of experiments/rb2d/train.py:79-83 for one
 * parameter tensor (fp32, 16-byte aligned).  g = clamp(grad, +-clip) (clip <= 0: off); m, v, p are updated in
 * place with torch.optim.Adam's formulas: step_size = lr / (1 - beta1^t), bias2_sqrt = sqrt(1 - beta2^t). */
typedef struct {
  long n;
  float clip, beta1, beta2, eps, weight_decay, step_size, bias2_sqrt;
} stpde_adam_desc;
int stpde_clip_adam(const stpde_adam_desc* d, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                    void* stream);
/* The same update for ALL parameter tensors in one launch (the reference's optimizer walks ~300 tensors).  Both
 * tables live in device memory and are built by the caller: one stpde_adam_tensor per parameter (16-byte aligned
 * pointers; step_size / bias2_sqrt per tensor, d->step_size / d->bias2_sqrt / d->n are ignored) and one
 * stpde_adam_chunk per block of work: elements [offset, offset + chunk_elems) of tensor `tensor`, offset % 4 == 0. */
typedef struct {
  float* p;
  const float* g;
  float* m;
  float* v;
  long n;
  float step_size, bias2_sqrt;
} stpde_adam_tensor;
typedef struct {
  int tensor, pad;
  long offset;
} stpde_adam_chunk;
int stpde_clip_adam_multi(const stpde_adam_desc* d, const stpde_adam_tensor* tensors_dev,
                          const stpde_adam_chunk* chunks_dev, int nchunks, int chunk_elems, void* stream);

/* ---- capturable optimizers: step count and learning rate in device memory ----------------------------------
 * A launch captured in a HIP graph freezes its by-value arguments, so an optimizer that is to be replayed keeps what
 * changes from step to step in a block of device memory the caller owns: 32 bytes, 16-byte aligned, zero-filled before
 * the first step.  The caller writes `lr` (and `step` when it resumes from a checkpoint); stpde_opt_advance writes
 * the rest.  The layout is part of the ABI (callers poke the fields through typed views of the block): `step` is a
 * 64-bit signed integer at byte 0 (`long` on the LP64 targets this library builds for), `lr` an fp64 at byte 8,
 * `step_size` / `bias2_sqrt` fp32 at bytes 16 / 20; stpde_version() changes with it. */
typedef struct {
  long step;                    /* optimizer steps taken (all tensors of a group share it) */
  double lr;                    /* learning rate (the SGD kernels round it to fp32, like a by-value float) */
  float step_size, bias2_sqrt;  /* Adam: lr / (1 - beta1^step), sqrt(1 - beta2^step), fp64 rounded to fp32 */
  float reserved[2];
} stpde_opt_state;
typedef struct {
  double beta1, beta2;          /* Adam's betas; 0, 0 for SGD (step_size = lr, bias2_sqrt = 1) */
} stpde_opt_desc;
/* One-workgroup kernel, launched in front of the update kernel of a step: ++step, then the two derived scalars. */
int stpde_opt_advance(const stpde_opt_desc* d, stpde_opt_state* state_dev, void* stream);
/* stpde_clip_adam / stpde_clip_adam_multi with step_size and bias2_sqrt read from the state block (d->step_size,
 * d->bias2_sqrt and the two fields of the table rows are ignored).  The tables hold nothing that changes from step to
 * step: build them once, reuse them while the pointers stay. */
int stpde_clip_adam_dev(const stpde_adam_desc* d, const stpde_opt_state* state_dev, float* param, const float* grad,
                        float* exp_avg, float* exp_avg_sq, void* stream);
int stpde_clip_adam_multi_dev(const stpde_adam_desc* d, const stpde_opt_state* state_dev,
                              const stpde_adam_tensor* tensors_dev, const stpde_adam_chunk* chunks_dev, int nchunks,
                              int chunk_elems, void* stream);

/* ---- gradient value clipping + SGD in one pass (the reference's --optim sgd, train.py:220, :330-333) -------
 * g = clamp(grad, +-clip) (clip <= 0: off), then torch.optim.SGD: g += weight_decay * p; with momentum != 0
 * buf = g on the first step, else momentum * buf + (1 - dampening) * g, and g = g + momentum * buf (nesterov) or buf;
 * p -= lr * g.  state_dev == NULL: lr and first_step of the descriptor (the table row in the multi variant) are used.
 * state_dev != NULL: lr is the block's, and the step is the first one when the block's count is 1, i.e. right behind
 * the first stpde_opt_advance.  momentum == 0: no buffer is read or written (momentum_buf / buf may be NULL). */
typedef struct {
  long n;
  float clip, lr, momentum, dampening, weight_decay;
  int nesterov, first_step;
} stpde_sgd_desc;
int stpde_clip_sgd(const stpde_sgd_desc* d, const stpde_opt_state* state_dev, float* param, const float* grad,
                   float* momentum_buf, void* stream);
typedef struct {
  float* p;
  const float* g;
  float* buf;
  long n;
  int first_step, pad;
} stpde_sgd_tensor;
/* All tensors in one launch; chunk table as for stpde_clip_adam_multi (d->n and d->first_step are ignored). */
int stpde_clip_sgd_multi(const stpde_sgd_desc* d, const stpde_opt_state* state_dev, const stpde_sgd_tensor* tensors_dev,
                         const stpde_adam_chunk* chunks_dev, int nchunks, int chunk_elems, void* stream);

/* ---- N3 on the device: training batches drawn and produced by capturable launches -------------------------------
 * Replaces, for lres_filter = 'none', what RB2DataLoader.__getitem__ + RandomSampler(replacement=True) + the collate do per
 * batch (experiments/rb2d/dataloader_spacetime.py:118-171, train.py:318-321): random crop positions, random query points,
 * the linearly (or nearest-) down-sampled low-resolution input grid and the interpolated point targets, normalised.
 * The dataset stays where it is -- data_cl [T][Z][X][4] fp32, channels-last, 16-byte aligned -- and is read in place: no
 * [B][nt][nz][nx][4] crop is materialised.  Nothing here allocates or synchronises, so both entries are legal inside a
 * stream capture; what changes from draw to draw lives in a state block of device memory, as for the optimizers.
 *
 * State block: 32 bytes of device memory the caller owns, 16-byte aligned.  The layout is part of the ABI (callers fill
 * and read the fields through a typed view): the Philox key `seed`, an unsigned 64-bit integer at byte 0; the draw
 * counter `offset`, an unsigned 64-bit integer at byte 8 (one draw = one batch = +1); `oob`, an unsigned 32-bit count at
 * byte 16 of the crop ids outside [0, len) that the produce entry has clamped so far; 12 reserved bytes.
 *
 * Generator: Philox4x32-10 (Salmon et al., SC'11; the Random123 constants).  key = (seed_lo, seed_hi); the 128-bit
 * counter of a call is (offset_lo, offset_hi, q, purpose): `purpose` selects the stream, q numbers the calls within it.
 *   purpose 0, crop ids:     word j of call q is crop 4q + j;  id = (word * len) >> 32  (64-bit product), len = rt*rz*rx.
 *                            Uniform with replacement; an id's probability differs from 1/len by at most 2^-32, i.e. a
 *                            relative bias of at most len / 2^32 (len < 2^31 is required).
 *   purpose 1, coordinates:  flat element e = (b*N + n)*3 + k of point_coord is word e % 4 of call e / 4;
 *                            value = (word >> 8) * 2^-24, exact in fp32, in [0, 1).
 * Two draws never share a counter as long as `offset` differs, whatever B and N are.
 *
 * Arithmetic of the produce entry: bit-identical to RB2DeviceLoader.get() of this package on the same ids and points.
 *   low-res voxel, linear:   the eight values at taps (i0, i0 + 1) per axis are reduced t first, then z, then x, each stage
 *                            lo + (hi - lo) * w with every intermediate rounded to fp32; then (v - mean) / std.
 *   targets, linear:         q = point_coord * (n - 1) per component, then the clip / cell index / corner weights / corner sum
 *                            of stpde_interp_fwd (csrc/interp_geom.h is shared by both) on the crop's window; then normalise.
 *   nearest:                 the low-res tap tables hold the node itself (w is ignored); a target takes node i + 1 when
 *                            q - i > 0.5 with i = min(max(floor(q), 0), n - 2), else node i (ties go down).
 * Crop origin of id: t0 = id / (rz*rx), z0 = (id / rx) % rz, x0 = id % rx (C-order meshgrid, reference :82-86).  An id
 * outside [0, len) is clamped into the range before any address is formed and counted in `oob`; tap indices and cell
 * indices are clamped to the crop as well, so no buffer content can make the kernel read outside data_cl. */
typedef struct {
  unsigned long seed;    /* Philox key                                  */
  unsigned long offset;  /* draws taken so far                          */
  unsigned int oob;      /* out-of-range explicit crop ids seen so far  */
  unsigned int reserved[3];
} stpde_sampler_state;
typedef struct {
  int i0;   /* linear: lower tap, in [0, n - 2]; nearest: the node, in [0, n - 1] */
  float w;  /* linear: weight of tap i0 + 1, fp32 of an fp64 host computation      */
} stpde_sampler_tap;
typedef struct {
  int T, Z, X;           /* dataset extents                                        */
  int nt, nz, nx;        /* crop extents (>= 2 each)                               */
  int ntl, nzl, nxl;     /* low-res extents; each divides its crop extent          */
  int rt, rz, rx;        /* crop ranges: T - nt + 1, Z - nz + 1, X - nx + 1        */
  int B, N;              /* crops per batch, points per crop                       */
  int interp;            /* 0 linear, 1 nearest                                    */
  int normalize;         /* 1: (v - mean[c]) / std[c] on both outputs              */
  float mean[4], std[4];
  float lo_c[3], hi_c[3], cube[3]; /* as stpde_interp_desc for the crop box [0, n - 1] */
} stpde_sampler_desc;
/* crop_idx_out [B] int32, point_coord_out [B][N][3] fp32; then offset += 1 by a one-thread kernel behind the draw kernel
 * in stream order (never a race with the reads of `offset`). */
int stpde_sampler_draw(const stpde_sampler_desc* d, stpde_sampler_state* state_dev, int* crop_idx_out,
                       float* point_coord_out, void* stream);
/* One launch: lres_out [B][4][ntl][nzl][nxl], point_value_out [B][N][4].  crop_idx / point_coord: what the draw entry
 * filled, or the caller's own (explicit mode). */
int stpde_sampler_produce(const stpde_sampler_desc* d, stpde_sampler_state* state_dev, const float* data_cl,
                          const stpde_sampler_tap* taps_t, const stpde_sampler_tap* taps_z,
                          const stpde_sampler_tap* taps_x, const int* crop_idx, const float* point_coord,
                          float* lres_out, float* point_value_out, void* stream);

/* ---- N3 on the device, with the low-res pre-filter (lres_filter = gaussian / uniform / maximum) --------------------
 * What RB2DeviceLoader.get() does with dataloader_spacetime.lres_filter before it interpolates (reference
 * experiments/rb2d/dataloader_spacetime.py:96-116, :136-155), bit for bit, in capturable launches: the high-res crops of the
 * batch are filtered into a scratch crop, and BOTH outputs are then interpolated from it by the produce entry below.
 * `median` is not separable and has an entry of its own, stpde_sampler_median below.
 *
 * The filter acts on the crop [nt][nz][nx] per channel with scipy's 'reflect' boundary at the CROP faces (the edge sample is
 * repeated, period 2n, any radius); dataset values outside the crop are never read.  Up to three 1-D passes run in the order
 * t, z, x, each on the fp32 result of the one before; an axis with r = 0 is skipped, not run with one tap.
 *   gaussian, uniform: out[i] = (((+0 + w[0] x[i-r]) + w[1] x[i-r+1]) + ...) + w[2r] x[i+r], a separate fp32 multiply and add
 *                      per tap.  The tables are the caller's: w_t, w_z, w_x of 2r + 1 fp32 each (nw = 2r + 1), in device memory.
 *   maximum:           the largest of the 2r + 1 taps; a NaN tap gives NaN.  No tables (nw = 0, the pointers may be null).
 * The first pass that runs reads data_cl at the crop origin of crop_idx[b] -- clamped into [0, len) before any address is
 * formed and counted in state->oob, exactly as the produce entry does; later passes read scratch.  scratch_a and scratch_b are
 * [B][nt][nz][nx][4] fp32, 16-byte aligned, caller-owned and distinct; the passes ping-pong between them and the result is
 * ALWAYS left in scratch_a (with no axis to filter, a plain copy of the crops).  Nothing allocates or synchronises. */
#define STPDE_FILTER_GAUSSIAN 1
#define STPDE_FILTER_UNIFORM 2
#define STPDE_FILTER_MAXIMUM 3
typedef struct {
  int T, Z, X;           /* dataset extents                                                  */
  int nt, nz, nx;        /* crop extents (>= 2 each)                                         */
  int rt, rz, rx;        /* crop ranges: T - nt + 1, Z - nz + 1, X - nx + 1                  */
  int B;                 /* crops per batch                                                  */
  int kind;              /* STPDE_FILTER_GAUSSIAN / _UNIFORM / _MAXIMUM                      */
  int r[3];              /* radius along t, z, x, in [0, 2^20]; 0: the axis is skipped       */
  int nw[3];             /* entries of w_t, w_z, w_x: 2 r + 1 on a weighted axis that runs, else 0 */
} stpde_sampler_filter_desc;
int stpde_sampler_filter(const stpde_sampler_filter_desc* d, stpde_sampler_state* state_dev, const float* data_cl,
                         const int* crop_idx, const float* w_t, const float* w_z, const float* w_x, float* scratch_a,
                         float* scratch_b, void* stream);
/* stpde_sampler_produce on filtered crops: `crops` [B][nt][nz][nx][4] (scratch_a of the entry above) is read with crop-local
 * addressing, origin 0 of crop b; the crop ids are not looked at again (nothing is counted twice).  Same arithmetic, same
 * outputs; d is the descriptor the unfiltered entry takes. */
int stpde_sampler_produce_filtered(const stpde_sampler_desc* d, const float* crops, const stpde_sampler_tap* taps_t,
                                   const stpde_sampler_tap* taps_z, const stpde_sampler_tap* taps_x, const float* point_coord,
                                   float* lres_out, float* point_value_out, void* stream);

/* ---- N3 on the device, the median pre-filter (lres_filter = median) --------------------------------------------
 * The fourth filter of the reference loader: per voxel and channel the element of rank (W - 1) / 2 (ascending, 0-based) of the
 * W = (2 r_t + 1)(2 r_z + 1)(2 r_x + 1) values of its window -- W is odd, so this is the exact median, what
 * RB2DeviceLoader.get() computes by unfolding every window and torch.median.  Not separable: ONE selection kernel (csrc/
 * sampler_median.hip: a tile and its halo staged into LDS as order-preserving keys, MSB-first radix selection per voxel).
 *   d          the filter descriptor above with kind = STPDE_FILTER_MEDIAN, nw[k] = 0 and r[k] in [0, 7] (downsamp - 1; a larger
 *              halo does not fit the LDS of one workgroup and is refused).  r[k] = 0 is a window of 1 along that axis, not a
 *              skipped pass; all radii 0 is a plain copy of the crops.
 *   window     scipy's 'reflect' rule at the CROP faces (period 2n, valid for r >= n), the index formula of the 1-D passes;
 *              dataset values outside the crop are never read.
 *   NaN        a window that holds a NaN gives a (quiet) NaN, as torch.median.  Of zeros of both signs either may be returned.
 *   crops_out  [B][nt][nz][nx][4] fp32, 16-byte aligned: the layout of scratch_a, consumed as it is by
 *              stpde_sampler_produce_filtered.
 * crop_idx is clamped into [0, len) before any address is formed and a clamped id is counted once in state->oob, as above.
 * Nothing allocates or synchronises; apart from that count there are no atomics, so the result is the same every run.
 * stpde_sampler_filter keeps refusing kind 4.
 * Cost (an ESTIMATE, not a measurement): at the reference's training shape (B = 10, crop 16 x 128 x 128, r = 3: W = 343)
 * 2.6 M voxels x 343 taps x up to 32 walks x 16 B are about 4.6e11 B of LDS reads, a few ms at the LDS rate of the part.  Follow-up,
 * not built: select only at the nodes the two interpolations read (about 41 k of 262 k voxels per crop), roughly 6 x less. */
#define STPDE_FILTER_MEDIAN 4     /* accepted by stpde_sampler_median only */
int stpde_sampler_median(const stpde_sampler_filter_desc* d, stpde_sampler_state* state_dev, const float* data_cl,
                         const int* crop_idx, float* crops_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
