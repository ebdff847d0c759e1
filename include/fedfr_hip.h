/* fedfr_hip.h — C ABI of libfedfr_hip.so: the MI355X (gfx950) implementation of FedFR's per-client
 * training hot path.  The reference (jackie840129/FedFR) is pure Python/PyTorch and has no FFI; the
 * entry points below are what its Python modules bind through ctypes.  Each
 * group cites the reference code it replaces.
 *
 * Conventions
 *   - every function returns 0 on success, a negative FEDFR_ERR_* otherwise; fedfr_last_error_string()
 *     describes the most recent failure on the calling thread.  Nothing throws, nothing exits.
 *   - all pointers are DEVICE pointers owned by the caller (e.g. torch tensors' data_ptr()); the library
 *     allocates no device memory and retains no pointer after return.
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on it.
 *   - activations are NHWC in the 16-bit storage type (IEEE fp16 in libfedfr_hip.so, bf16 in libfedfr_hip_bf16.so: fedfr_storage_dtype(); raw uint16 bits); conv weights are KRSC ([Cout][kh][kw][Cin]) which is
 *     exactly a torch channels_last OIHW tensor; parameters / grads / optimizer state are fp32.
 */
#ifndef FEDFR_HIP_H
#define FEDFR_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FEDFR_OK 0
#define FEDFR_ERR_ARG (-1)
#define FEDFR_ERR_HIP (-2)
#define FEDFR_ERR_WORKSPACE (-3)
#define FEDFR_ERR_UNSUPPORTED (-4)

int fedfr_version(void);
/* 16-bit storage type of activations / activation gradients / MFMA weight operands this build uses: 1 = IEEE fp16 (libfedfr_hip.so, the
 * product: the reference's own AMP type, backbones/iresnet.py:159; gradients carry the host's loss scale, FEDFR_LOSS_SCALE, which
 * fedfr_sgd_step_scaled / fedfr_net_backward2_sgd_scaled undo and guard), 0 = bf16 (libfedfr_hip_bf16.so, `make -C fedfr_amd/csrc bf16`:
 * the same kernels, no loss scale, whole-network outputs 1.5-2.5e-2 from the fp32 reference instead of 2-3e-3) */
int fedfr_storage_dtype(void);
const char* fedfr_last_error_string(void);
/* Kernel-choice switches for same-box A/B measurements and validation fallbacks (no reference counterpart; every setting stays inside the
 * tests' tolerances; FEDFR_OPTIONS="name=value,..." in the environment applies them when the library is loaded; fedfr_option_info lists
 * them with their defaults).  Round 4 removed the switches whose alternative lost twice (the register-staged halo conv kernels, the
 * BatchNorm-on-load conv, the two-blocks-per-CU weight-gradient pair, sphnet's activation epilogue, the fork / join placement and row-slab sweeps);
 * round 6 the numeric tuning parameters and the switches whose alternative lost every same-box sweep of rounds 2-5 and validates nothing (nt_nbuf,
 * tn_target_blocks, wgrad9_wgs, wgrad_depth, fc_wgrad_aux, bn_sliced_pre, bn_sliced_bwd_passes, event_nofence): what is left selects a kernel
 * family or a fusion that the tests compare against its alternative.  [default]:
 *   GEMM kernels        "nt_glds" [4] LDS-DMA operand ring of the NT GEMM (0 register-staged everywhere, +8 every shape it serves),
 *                       "tn_glds" [2] LDS-DMA weight-gradient GEMM (0 register-staged, 1 four waves), "tn_use_tr" [1] (0 scalar LDS fragments),
 *                       "dgrad_parity" [2] stride-2 dgrad by output-parity class (2: one launch), "conv_c64p" [1] persistent
 *                       64-channel conv, "conv28_tpw2" [2] two 28x28 tiles per workgroup (1 forward only), "eval_fuse" [1] eval-mode BatchNorm in the conv epilogues
 *   weight gradients    "wgrad9" [1] nine-tap kernel, "wgrad9p" [1] paired 64 x 64 nine-tap kernel, "wgrad9p_bg" [1] a paired launch sums the
 *                       PREVIOUS pair's split-K slabs beside its own work (0: stand-alone reductions), "wgrad_pair_reduce" [1]
 *   BatchNorm forward   "bn_sliced" [1] channel-sliced passes without finalize launches, "fwd_xmom" [1] bn3 + identity + the next block's bn1 as one
 *                       pass from conv2's raw moments
 *   BatchNorm backward  "fuse_bnbwd" [2] reduction in the dgrad epilogue (1 every fused kernel, 2 the 14x14 layers), "fuse_bnbwd28" [1], "c64p_bnbwd" [1],
 *                       "fuse_bnred_next" [1] an apply pass reduces its output for the next BatchNorm, "stem_bnred" [1],
 *                       "stem_fuse_wgrad" [1] the stem's BatchNorm + PReLU backward applied inside its weight-gradient kernel (no apply pass)
 *   sphnet              "sph_fin_multi" [1], "sph_pair_wgrad" [1], "sph_fuse_prelu_bwd" [1]
 * Unknown names are an error.  The switches are process-wide and NOT synchronised: set them before other host threads call into the library.  The library
 * itself never writes one (round 6: plan creation used to toggle two of them for a moment, which raced with other threads' launches). */
int fedfr_set_option(const char* name, int value);
/* the switch's current value (a caller that changes one temporarily restores what it found) */
int fedfr_get_option(const char* name, int* value);
/* enumeration of the switches, so that a measurement can state which of them were NOT at their defaults (bench.py `options_non_default`):
 * number of switches; switch `index` = (name, current value, the value the library starts with).  Switches that give wrong results
 * (timing experiments such as "dbg_skip") exist only in a -DFEDFR_DEBUG build and are then listed too. */
int fedfr_option_count(void);
int fedfr_option_info(int index, const char** name, int* value, int* default_value);
/* HIP-event timing of every MFMA GEMM launch on its own stream (bench.py roofline leg).  Slots 0..3: conv fwd/dgrad
 * kernel gemm_nt tiles <128,128> <128,64> <64,128> <64,64>; 4..7: wgrad kernel gemm_tn, same tile order; 8..11: retired (the
 * register-staged halo conv kernels of rounds 1-3); 12 conv3x3_glds<14,14>, 13 conv3x3_glds<28,7>, 14 gemm_tn_glds, 15 the 64-channel 3x3
 * layers, 16 the nine-tap weight-gradient kernels, 17 gemm_nt_glds; 20..26 the HBM-bound BatchNorm / reduction / SGD kernels (flops = bytes).
 * enable(1) resets the counters; read() requires the stream to be synchronised; flops = sum of 2*M*N*K. */
int fedfr_profile_enable(int on);
int fedfr_profile_read(int slot, double* total_ms, long long* launches, double* flops);
/* the ALGORITHMIC HBM bytes of the same launches (slots 0..17: every operand read once, the output written once; split-K slabs and halo re-reads are
 * not algorithmic): lets a measurement say which roofline bounds a kernel family (bench.py `all_gemm_kernels[].bound`) */
int fedfr_profile_read_bytes(int slot, double* bytes);

/* ------------------------------------------------------------------------------------------------
 * iresnet plan — replaces IResNet.__init__/_make_layer/forward (backbones/iresnet.py:60-172) and,
 * through the hand-written adjoint, autograd's backward of it.
 * ------------------------------------------------------------------------------------------------ */
typedef struct FedfrNet fedfr_net_t;
fedfr_net_t* fedfr_net_create(const int* layers4, int batch, int in_hw, int num_features);
/* A lone IBasicBlock(cin, cout, stride) on a hin x hin map (reference backbones/iresnet.py:28-57) as a plan of its own, driven by the
 * same query / tensor_info / prepare_weights / forward / backward entry points (tensors in the reference block's state_dict order:
 * bn1.*, conv1.weight, bn2.*, prelu.weight, conv2.weight, bn3.*, downsample.0.weight, downsample.1.*).  With such a plan
 * fedfr_net_forward takes x = fp32 NCHW [B][cin][hin][hin] (feats may be NULL; y = act selector 6) and fedfr_net_backward takes
 * dfeats = fp32 NCHW [B][cout][hout][hout] (dx = act selector 7).  stride 1 needs cin == cout; stride 2 adds the 1x1 downsample. */
fedfr_net_t* fedfr_block_create(int cin, int cout, int stride, int hin, int batch);
/* SphereFace backbone (reference backbones/sphnet.py:16-73 — the network run.sh trains): type 20 or 64, 112 x 112 input, 512 features, as a
 * plan with the SAME entry points and buffers as an iresnet plan (fedfr_net_query / _tensor_info / _prepare_weights / _forward /
 * _backward*).  No BatchNorm: buffer and counter regions are empty, `bufs` is ignored, training and eval forward coincide; conv weights are
 * KRSC like iresnet's; fedfr_net_backward2_sgd leaves the whole update to the caller (*done_from = trainable count). */
fedfr_net_t* fedfr_net_create_sphere(int type, int batch);
void fedfr_net_destroy(fedfr_net_t* net);
/* nn.Dropout(p, inplace=True) between bn2 and fc (backbones/iresnet.py:96,169; the reference uses p = 0.4 for its webface configuration,
 * client.py:142): training forwards then zero a counter-based random subset of the flattened bn2 output (element i of the k-th training
 * forward is kept iff hash16(seed, k, i) >= p * 65536) and scale the rest by 1 / (1 - p); the backward applies the same mask.  p = 0 turns it
 * off; the call resets the forward counter.  *mask_offset_bytes (optional): where the last mask ([batch * fc_in] bytes, 0/1) lives in `act`. */
int fedfr_net_set_dropout(fedfr_net_t* net, float p, unsigned long long seed, long long* mask_offset_bytes);
/* the index k of the NEXT training forward's mask.  The plan's own counter restarts whenever a plan is (re)created — after an eviction, a
 * workspace release, for every new model — so a host that wants masks that never repeat keeps the count itself (fedfr_amd.IResNet does:
 * one counter per model, handed over before every training forward). */
int fedfr_net_set_dropout_step(fedfr_net_t* net, unsigned long long step);
/* debug (tests): while buf != NULL, fedfr_net_backward* copies the gradient entering every block (16-bit storage type, NHWC, last block first) and then
 * the gradient wrt the first block's input back to back into buf (caller-owned, `elems` 16-bit elements); NULL turns it off.  The one
 * exception to "no pointer is retained": clear it before freeing the buffer.
 * On a sphnet plan the copies are the gradient each PReLU backward pass of a block's second unit (u2) and of a stage head differentiates — 16-bit
 * NHWC [B * H * H][C], AFTER the pending branch gradient of the block behind it has been folded in — back to back in backward order: per stage from
 * the last to the first, its blocks from the last to the first, then its head (sphere20: 12 tensors, sphere64: 33).  With buf == NULL the pass
 * enqueues exactly what it enqueues without the hook. */
int fedfr_net_debug_capture(uint16_t* buf, size_t elems);
/* debug (tests), iresnet plans: what fedfr_net_debug_capture copies.  Level 0 (the default): as above.  Level 1: directly behind every block's
 * entering gradient also the block's intermediate gradients, each copied right behind the kernel that produced it: dc2 [B*Ho*Ho][Cout] (wrt conv2's
 * output), da2 [B*Hi*Hi][Cout] (wrt prelu(bn2)), dc1 [B*Hi*Hi][Cout] (wrt conv1's output), for a downsample block dd [B*Ho*Ho][Cout] (wrt the
 * downsample conv's output) and dxd [B*Ho*Ho][Cin] (its dgrad: compact, the bn1 backward pass places it at the even pixels), then da1
 * [B*Hi*Hi][Cin] (wrt bn1's output); and in FRONT of everything the gradient wrt the network's bn2 output, NHWC [B*hw][final_C], final_C the last
 * stage's planes (what the fc's input gradient becomes before bn2's backward).  Process-global like the buffer; without a buffer no level enqueues anything. */
int fedfr_net_debug_capture_detail(int level);
/* host-only: the 16-bit elements a backward pass of `net` captures at `level` (the size fedfr_net_debug_capture's buffer needs) */
int fedfr_net_debug_capture_elems(const fedfr_net_t* net, int level, long long* elems);
/* host-only, iresnet plans: the i-th 2-D BatchNorm in state_dict order (FEDFR_Q_NUM_BN of them: the stem's, per block bn1, bn2, bn3 and the
 * downsample's, the network's bn2) — its state_dict prefix, channel count, and where a training forward leaves its four rows of C floats
 * (scale, shift, mean, rstd): a float offset from byte FEDFR_Q_ACT_FLOAT_OFF_BYTES of `act`.  Behind the last BatchNorm's rows a network plan keeps 4 * F
 * floats for the features' BatchNorm1d, then the fc output [batch][F] and that BatchNorm1d's (mean, rstd) [2][F].  A sphnet plan has none: an
 * argument error. */
int fedfr_net_bn_info(const fedfr_net_t* net, int i, char* name, int name_cap, int* C, long long* save_offset_floats);
enum {
  FEDFR_Q_PARAM_COUNT = 0,      /* fp32 elements: trainable region + frozen features.weight */
  FEDFR_Q_TRAINABLE_COUNT = 1,
  FEDFR_Q_BUFFER_COUNT = 2,     /* fp32 BN running stats */
  FEDFR_Q_NBT_COUNT = 3,        /* int64 num_batches_tracked scalars */
  FEDFR_Q_SHADOW_COUNT = 4,     /* 16-bit elements */
  FEDFR_Q_ACT_BYTES = 5,
  FEDFR_Q_WS_BYTES = 6,
  FEDFR_Q_NUM_TENSORS = 7,
  FEDFR_Q_FC_IN = 8,
  FEDFR_Q_NUM_BN = 9,                /* 2-D BatchNorms fedfr_net_bn_info answers for */
  FEDFR_Q_ACT_FLOAT_OFF_BYTES = 10   /* byte offset of the float region (BatchNorm save rows first) inside `act` */
};
int fedfr_net_query(const fedfr_net_t* net, int what, long long* out);
/* state_dict entry i (reference key order).  kind: 0 conv 1 bn.weight 2 bn.bias 3 prelu 4 fc.weight
 * 5 fc.bias 6 running_mean 7 running_var 8 num_batches_tracked; region: 0 params 1 bufs 2 nbt. */
int fedfr_net_tensor_info(const fedfr_net_t* net, int i, char* name, int name_cap, int* kind, int* region,
                          long long* offset, int* ndim, int* shape4);
/* debug/inspection: where a saved activation lives inside `act` (16-bit element offset, [rows][channels] NHWC view).
 * block < 0: which = 0 stem conv output, 1 stem activation, 2 flattened bn2 output [B][fc_in] (NCHW order);
 * block >= 0: which = 0 block input, 1 bn1 out, 2 conv1 out, 3 prelu(bn2) out, 4 conv2 out, 5 downsample conv out
 * (offset -1 if the block has none), 6 block output, 7 gradient wrt the block input (fedfr_block_create plans only, after a backward).  An eval-mode forward (training = 0) applies the BatchNorms in the conv epilogues
 * where the kernel has one and then does not store the raw conv outputs (2, 4); fedfr_set_option("eval_fuse", 0) restores them.
 * sphnet plan (fedfr_net_create_sphere): block = the UNIT index in forward order, 0 ... last (per stage: the stride-2 stage head, then u1, u2 of each
 * residual block; sphere20 has 20 units, sphere64 62); which = 0 the unit's input (rows = B * Hin * Hin; unit 0: the image padded to 64 channels),
 * 1 c, the raw conv output, 2 t = prelu(c + bias) (+ the block input for u2) — the LAST unit's t is stored NCHW-flat [B][512 * 49], the view the fc
 * reads, not NHWC — and 3 dz, the gradient wrt c a backward pass leaves in the WORKSPACE (offset in 16-bit elements of `ws`, not of `act`);
 * rows = B * Hout * Hout, channels = the stored width.  block < 0 and every other selector are argument errors on a sphnet plan. */
int fedfr_net_act_info(const fedfr_net_t* net, int block, int which, long long* offset, int* rows, int* channels);
/* refresh the 16-bit weight shadows (storage type: fp16 / bf16 per build) from fp32 params (after load_state_dict / an external optimizer step);
 * fwd_shadow_too = 0 when fedfr_sgd_step already wrote the mirror region. */
int fedfr_net_prepare_weights(const fedfr_net_t* net, const float* params, uint16_t* shadow, int fwd_shadow_too,
                              void* stream);
/* x: fp32 NCHW [B][3][hw][hw] in [-1,1]; feats: fp32 [B][num_features].
 * training: 0 = model.eval(), 1 = model.train(), 2 = model.train() followed by IResNet.freeze_BN(test_mode=True) (iresnet.py:140-147):
 * every BatchNorm normalises with its running statistics and tracks nothing while the net trains (dropout on, activations kept); the
 * next fedfr_net_backward* of the plan then runs the BatchNorm backward of eval-mode modules (dx = gamma rstd dz). */
int fedfr_net_forward(const fedfr_net_t* net, const float* x, const float* params, float* bufs,
                      const uint16_t* shadow, void* act, void* ws, float* feats, int training, void* stream);
/* grads (fp32 [trainable_count]) are assigned, not accumulated */
int fedfr_net_backward(const fedfr_net_t* net, const float* x, const float* dfeats, const float* params,
                       const uint16_t* shadow, void* act, void* ws, float* grads, void* stream);

/* same, with the weight-gradient GEMMs (off the dgrad->BatchNorm critical path) on a second caller-owned stream so
 * they fill the CUs the main chain leaves idle; fork/join uses HIP events; when the call returns, everything is ordered
 * before later work on `stream`.  aux_stream == NULL behaves like fedfr_net_backward. */
int fedfr_net_backward2(const fedfr_net_t* net, const float* x, const float* dfeats, const float* params,
                        const uint16_t* shadow, void* act, void* ws, float* grads, void* stream, void* aux_stream);
/* fedfr_net_backward2 with `torch.optim.SGD(...).step()` (client.py:396,550; fedfr_sgd_step semantics: coupled weight decay, momentum
 * buffer, 16-bit mirror refreshed) folded in: parameter ranges whose gradients are final — the bn2 / fc / features tail, then each stage
 * of residual blocks as the pass leaves it — are updated on aux_stream while `stream` walks the earlier stages.  When the call's work
 * completes, parameters [*done_from, trainable_count) are updated; the caller runs fedfr_sgd_step on [0, *done_from) (stem + stage 1).
 * params / shadow are the buffers the pass reads (now written too); results are bit-identical to backward + one flat fedfr_sgd_step. */
int fedfr_net_backward2_sgd(const fedfr_net_t* net, const float* x, const float* dfeats, float* params, uint16_t* shadow, void* act, void* ws,
                            float* grads, float* momentum, float lr, float mu, float wd, int first, long long* done_from, void* stream,
                            void* aux_stream);
/* the same with fedfr_sgd_step_scaled as the update (dfeats arrives multiplied by 1 / grad_scale).  On return grads[*done_from, n) hold
 * unscaled gradients and grads[0, *done_from) still scaled ones: the caller finishes with fedfr_sgd_step_scaled on [0, *done_from). */
int fedfr_net_backward2_sgd_scaled(const fedfr_net_t* net, const float* x, const float* dfeats, float* params, uint16_t* shadow, void* act,
                                   void* ws, float* grads, float* momentum, float lr, float mu, float wd, int first, float grad_scale,
                                   unsigned* overflow, long long* done_from, void* stream, void* aux_stream);
/* the same with fedfr_sgd_step_drift as the update (DRIFT TERMS below): anchor / corr are indexed like params, so the ranges the pass updates
 * itself read their own slices.  overflow == NULL with grad_scale == 1 is the unguarded update, anything else the guarded one.  The caller
 * finishes with fedfr_sgd_step_drift on [0, *done_from); bit-identical to fedfr_net_backward2 + one flat fedfr_sgd_step_drift. */
int fedfr_net_backward2_sgd_drift(const fedfr_net_t* net, const float* x, const float* dfeats, float* params, uint16_t* shadow, void* act,
                                  void* ws, float* grads, float* momentum, float lr, float mu, float wd, int first, float grad_scale,
                                  unsigned* overflow, const float* anchor, float prox, const float* corr, long long* done_from, void* stream,
                                  void* aux_stream);

/* fp32 VALIDATION path of the same plan (csrc/net_f32.hip): IResNet.forward / autograd backward (iresnet.py:46-57,158-172) with fp32
 * activations and exact-fp32 arithmetic (im2col + the fp32-MFMA GEMM, two-pass BatchNorm in fp64) — what the "1e-3 fp32" tolerance is
 * checked with, and the yardstick that separates the product path's 16-bit storage noise from kernel error.  Slow by design (one launch per
 * operation, ~40 TFLOP/s); whole-network plans, dropout 0, training 0 / 1.  arena (fedfr_net_f32_arena_floats floats) keeps the
 * activations between forward and backward, ws (fedfr_net_f32_ws_floats floats) is scratch; params / bufs / grads are the plan's
 * ordinary fp32 buffers (grads assigned; running statistics updated by a training forward).
 * iresnet plans only: for a sphnet plan the two size queries return 0 and forward / backward are argument errors, checked before anything is
 * laid out or launched. */
size_t fedfr_net_f32_arena_floats(const fedfr_net_t* net);
size_t fedfr_net_f32_ws_floats(const fedfr_net_t* net);
int fedfr_net_f32_forward(const fedfr_net_t* net, const float* x, const float* params, float* bufs, float* arena, float* ws, float* feats,
                          int training, void* stream);
int fedfr_net_f32_backward(const fedfr_net_t* net, const float* dfeats, const float* params, float* arena, float* ws, float* grads,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * single convolutions — replace nn.Conv2d fwd / dgrad / wgrad at the call sites iresnet.py:38,41,76,121
 * (implicit GEMM on v_mfma_f32_16x16x32_f16 / _bf16 per build).  w: 16-bit KRSC; wd: 16-bit dgrad shadow [Cin][kh'][kw'][Cout].
 * stats (optional): [fedfr_conv2d_stat_rows][2][Cout] fp32 partial (sum, sumsq) of the 16-bit output.
 * ------------------------------------------------------------------------------------------------ */
int fedfr_conv2d_stat_rows(int batch, int hout, int cout);
int fedfr_conv2d_fwd(const uint16_t* x, const uint16_t* w, uint16_t* y, float* stats, int batch, int hin, int cin,
                     int cout, int ksize, int stride, void* stream);
int fedfr_conv2d_dgrad(const uint16_t* dy, const uint16_t* wd, uint16_t* dx, int batch, int hin, int cin, int cout,
                       int ksize, int stride, void* stream);
/* dgrad whose epilogue may also reduce the BatchNorm backward sums of (dx, bn_x): partials [rows][3][cin] =
 * (sum dz, sum dz*xhat, sum dx*min(z,0)).  *fused_rows (host int) = rows written, or 0 if this geometry is not fused
 * (then call fedfr_bn_bwd, which reduces itself). */
int fedfr_conv2d_dgrad_bnbwd(const uint16_t* dy, const uint16_t* wd, uint16_t* dx, int batch, int hin, int cin, int cout,
                             int ksize, int stride, const uint16_t* bn_x, const float* mean, const float* rstd,
                             const float* gamma, const float* beta, const float* alpha, float* partials, int* fused_rows,
                             void* stream);
/* The two conv epilogues that only whole networks used to reach, one kernel launch each (tests/test_conv_branches_gpu.py).
 * fedfr_conv2d_fwd_epilogue: the eval-mode forward of a 3x3 / stride-1 conv (what fedfr_net_forward(training = 0) runs under option
 *   "eval_fuse"): y = acc * scale[n] + shift[n] on the fp32 accumulator, PReLU with alpha[n] (NULL: none), rounded to 16 bits; with add
 *   [M][cout] y = round16(y + add); with y2, y2 = round16(y * scale2[n] + shift2[n]) of the STORED y.  Served for the shapes the LDS-DMA
 *   kernels take (14x14 / 28x28 maps with cin, cout multiples of 128, 56x56 with 64 -> 64 / 64 -> 128 / 128 -> 64, 112x112 with 64 -> 64,
 *   each from the batch at which they run on 128-row tiles); any other shape is FEDFR_ERR_UNSUPPORTED, nothing is launched.
 * fedfr_conv2d_dgrad_papply: sphnet's dgrad with the backward of the PReLU(+bias) in FRONT of the conv in its epilogue: z = act_x + bias
 *   (bias NULL: 0), dz = dgrad * (z <= 0 ? alpha[n] : 1) is what is stored, partials [*rows][3][cin] = (sum dz, sum dgrad z over z <= 0, the
 *   same again); *rows = batch * hin * hin / 196 (28x28 maps on the two-tiles kernel: / 392).  14x14 / 28x28 maps with cin, cout multiples
 *   of 128 from the batch at which they run on 128-row tiles; any other shape is FEDFR_ERR_UNSUPPORTED, nothing is launched. */
int fedfr_conv2d_fwd_epilogue(const uint16_t* x, const uint16_t* w, uint16_t* y, const float* scale, const float* shift, const float* alpha,
                              const uint16_t* add, uint16_t* y2, const float* scale2, const float* shift2, int batch, int hin, int cin,
                              int cout, void* stream);
int fedfr_conv2d_dgrad_papply(const uint16_t* dy, const uint16_t* wd, uint16_t* dz, int batch, int hin, int cin, int cout,
                              const uint16_t* act_x, const float* bias, const float* alpha, float* partials, int* rows, void* stream);
/* Host-only query of the kernel selector (no device is touched, nothing is launched): which kernel the forward conv (dgrad = 0) or the
 * dgrad (dgrad = 1) of this geometry runs on under the current options when it is asked for the epilogues in `want` — a bit set of
 * 1 forward statistics, 2 BatchNorm-backward rows, 4 raw moments, 8 PReLU-apply, 16 output epilogue (1, 4, 16: forward; 2, 8: dgrad; 2, 4, 8:
 * 3x3 only) — and what a caller has to know before the launch.  *profile_slot: the fedfr_profile_read slot of that kernel (a stride-2 3x3
 * dgrad under option "dgrad_parity": of its per-class launches); *stat_rows = fedfr_conv2d_stat_rows of the launch, *stat_rows_live the
 * leading rows of those that carry data; *part_rows: rows the reduction epilogue leaves, 0 if the kernel has none; *out_epilogue: 1 if
 * the kernel implements the output epilogue.  Without a device the persistent 64-channel kernel is planned for 256 compute units. */
int fedfr_conv2d_plan(int batch, int hin, int cin, int cout, int ksize, int stride, int dgrad, int want, int* profile_slot, int* stat_rows,
                      int* stat_rows_live, int* part_rows, int* out_epilogue);
/* lowest-priority HIP stream for the aux_stream argument of fedfr_net_backward2 (no reference counterpart; the reference trains on
 * one stream).  Destroy with fedfr_stream_destroy. */
int fedfr_stream_create_low_priority(void** stream);
int fedfr_stream_destroy(void* stream);
size_t fedfr_conv2d_wgrad_ws_bytes(int batch, int hin, int cin, int cout, int ksize, int stride);
int fedfr_conv2d_wgrad(const uint16_t* x, const uint16_t* dy, float* dw, void* ws, size_t ws_bytes, int batch, int hin,
                       int cin, int cout, int ksize, int stride, void* stream);
/* the two same-shape weight gradients of a residual block (conv1 / conv2, reference backbones/iresnet.py:38,41 through autograd) in one
 * launch; ws holds 2 x fedfr_conv2d_wgrad_ws_bytes.  Shapes the paired kernel does not take run as two fedfr_conv2d_wgrad calls. */
int fedfr_conv2d_wgrad_pair(const uint16_t* xa, const uint16_t* dya, float* dwa, const uint16_t* xb, const uint16_t* dyb,
                            float* dwb, void* ws, size_t ws_bytes, int batch, int hin, int cin, int cout, int ksize,
                            int stride, void* stream);
int fedfr_weight_shadows(const float* w_krsc, uint16_t* w_h16, uint16_t* wd_h16, int cout, int ksize, int cin,
                         void* stream);
/* plain GEMMs on the same kernels: C[m][n] = sum_k A[m][k] B[n][k] (fp32 out) and C[i][j] = sum_p P[p][i] Q[p][j] */
int fedfr_gemm_nt(const uint16_t* A, const uint16_t* B, float* C, void* ws, size_t ws_bytes, int M, int N, int K,
                  void* stream);
int fedfr_gemm_tn(const uint16_t* P, const uint16_t* Q, float* C, int Kp, int NI, int NJ, void* stream);
/* The network tail (between the last residual block and the embedding) one kernel launch at a time (tests/test_tail_kernels_gpu.py); what
 * fedfr_net_forward / _backward run there.
 * fedfr_bn1d_fwd: BatchNorm1d on fp32 x [B][C] -> y.  training: batch statistics (fp64 sums), running_mean / running_var updated with
 *   `momentum` (running_var from the unbiased variance; B = 1: the biased one); else the running statistics normalise and nothing is
 *   updated.  gamma NULL: 1, beta NULL: 0; save_mean / save_rstd [C] (both or neither) receive what the backward pass reads.
 * fedfr_bn1d_bwd: its backward from the saved statistics: dx [B][C], dbeta [C] = column sums of dy, dx_colsum [C] = column sums of dx
 *   (the bias gradient of the Linear in front), dx_h16 [B][C] and dx_h16_t [C][ldt] (ldt >= B; columns >= B are not written) = dx rounded
 *   to the 16-bit storage type; each of the five may be NULL.  frozen: the statistics were constants, dx = gamma rstd dy.
 * fedfr_reduce_slabs: dst[i] = sum_s slabs[s * n + i] (+ bias[i % bias_n]) in a fixed order; n % 4 == 0, bias_n % 4 == 0.  A second pair
 *   (dst1, slabs1: both or neither, same nsplit and n, no bias) is reduced by the same launch.
 * fedfr_dropout_fwd: in place on 16-bit t [n] (n % 8 == 0), 0 < p < 1: element e is kept iff the 16-bit field e % 4 of
 *   splitmix64(key ^ (e / 4)) is >= (unsigned)(p * 65536), key = seed * 0x100000001B3 + step * 0x9E3779B1 (mod 2^64); kept values are
 *   scaled by 1 / (1 - p), mask [n] receives one byte (1 kept / 0 dropped) per element.  fedfr_dropout_bwd: dx [n] fp32 (n % 4 == 0) in
 *   place through the same bytes.
 * fedfr_nchw_to_nhwc16: fp32 [B][C][HW] -> 16-bit [B][HW][C], C even. */
int fedfr_bn1d_fwd(const float* x, float* y, int B, int C, const float* gamma, const float* beta, float* running_mean, float* running_var,
                   float momentum, float eps, int training, float* save_mean, float* save_rstd, void* stream);
int fedfr_bn1d_bwd(const float* dy, const float* x, float* dx, int B, int C, const float* gamma, const float* save_mean, const float* save_rstd,
                   float* dbeta, float* dx_colsum, uint16_t* dx_h16, uint16_t* dx_h16_t, int ldt, int frozen, void* stream);
int fedfr_reduce_slabs(float* dst, const float* slabs, int nsplit, size_t n, const float* bias, int bias_n, float* dst1, const float* slabs1,
                       void* stream);
int fedfr_dropout_fwd(uint16_t* t, unsigned char* mask, size_t n, float p, unsigned long long seed, unsigned long long step, void* stream);
int fedfr_dropout_bwd(float* dx, const unsigned char* mask, size_t n, float p, void* stream);
int fedfr_nchw_to_nhwc16(const float* src, uint16_t* dst, int B, int C, int HW, void* stream);
/* stem conv 3->64 (iresnet.py:76) on fp32 NCHW input */
int fedfr_stem_stat_rows(int batch, int hw);
int fedfr_stem_fwd(const float* x, const float* w_krsc, uint16_t* y, float* stats, int batch, int hw, void* stream);
size_t fedfr_stem_wgrad_ws_bytes(int batch, int hw);
int fedfr_stem_wgrad(const float* x, const uint16_t* dy, float* dw, void* ws, int batch, int hw, void* stream);
/* the same weight gradient from the gradient wrt the stem's ACTIVATION: the BatchNorm + PReLU backward (coef [3][64] of fedfr_bn_bwd_rowslab
 * with coef_only, the forward's scale / shift, the slopes) is applied to dy_act and the conv output x0 on their way in (what
 * fedfr_net_backward runs under option "stem_fuse_wgrad") */
int fedfr_stem_wgrad_fused(const float* x, const uint16_t* dy_act, const uint16_t* x0, const float* coef, const float* sc, const float* sh,
                           const float* alpha, float* dw, void* ws, int batch, int hw, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm2d (train) + PReLU + residual — replace nn.BatchNorm2d / nn.PReLU / `out += identity`
 * (iresnet.py:37-56).  Tensors are [M][C] views (16-bit storage type) of NHWC activations.
 * ------------------------------------------------------------------------------------------------ */
/* partials: P rows [2][C] of (sum, sumsq); C % 8 == 0, as for every [M][C] entry point (any other C: FEDFR_ERR_ARG with a message);
 * tmp: 64 * 2 * C floats, needed when P > 1024 */
int fedfr_bn_finalize(const float* partials, int P, int C, double count, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, float momentum, float eps, float* scale, float* shift,
                      float* save_mean, float* save_rstd, float* tmp, void* stream);
int fedfr_bn_apply_stat_rows(int M, int C);
int fedfr_bn_apply(const uint16_t* x1, const float* sc1, const float* sh1, const float* alpha, const uint16_t* x2,
                   const float* sc2, const float* sh2, uint16_t* y, int M, int C, int nchw_hw, float* stats,
                   void* stream);
/* backward: partials [fedfr_bn_bwd_rows][3][C]; coef [3][C]; grads assigned */
int fedfr_bn_bwd_rows(int M, int C);
int fedfr_bn_bwd(const uint16_t* dy, const uint16_t* x, const float* mean, const float* rstd, const float* gamma,
                 const float* beta, const float* alpha, int M, int C, float* partials, float* coef, float* dgamma,
                 float* dbeta, float* dalpha, const uint16_t* add, const uint16_t* add_up, int H, uint16_t* dx,
                 void* stream);
/* The row-slab chain exactly as fedfr_net_backward drives it on the large maps (every argument of the apply pass is reachable):
 *   sc / sh: this BatchNorm's forward (scale, shift) — with alpha the PReLU mask is then sign(x sc + sh), the forward's own expression (NULL:
 *   derived from mean / rstd / gamma / beta, as fedfr_bn_bwd does);  count: elements per channel, HUGE_VAL for a frozen BatchNorm (dx = gamma
 *   rstd dz, the parameter-gradient sums unchanged);  rows_in > 0: `partials` already holds that many rows [3][C] left by a producing pass and
 *   the reduce pass is skipped;  coef_only: stop after the finalize (dgamma / dbeta / dalpha / coef written, dx untouched) — the consumer
 *   applies coef itself (fedfr_stem_wgrad_fused);  nx: dx is also reduced as the dy of the BatchNorm over nx (nmean / nrstd) into npart,
 *   fedfr_bn_bwd_apply_rows rows [3][C] = (sum dz, sum dz xhat, 0); with nalpha that BatchNorm has a PReLU behind it (nsc / nsh: its forward
 *   scale / shift) and the rows carry (sum dz, sum dz xhat, sum dx z over z <= 0) — served without alpha / add only.  npart may be `partials`
 *   (the finalize has read them before the apply pass writes). */
int fedfr_bn_bwd_apply_rows(int M, int C);
int fedfr_bn_bwd_rowslab(const uint16_t* dy, const uint16_t* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                         const float* alpha, const float* sc, const float* sh, int M, int C, double count, float* partials, int rows_in,
                         int coef_only, float* coef, float* dgamma, float* dbeta, float* dalpha, const uint16_t* add,
                         const uint16_t* add_up, int H, uint16_t* dx, const uint16_t* nx, const float* nmean, const float* nrstd,
                         float* npart, const float* nsc, const float* nsh, const float* nalpha, void* stream);

/* Channel-sliced train-mode BatchNorm passes that reduce the partial rows themselves (no finalize launch; csrc/bn_sliced.hip) — what
 * fedfr_net_forward / _backward run on the 28x28 and smaller maps.  Partial rows: [row][statistic][C] fp32, the layout fedfr_bn_apply /
 * fedfr_bn_bwd and the conv epilogues write.  Replaces nn.BatchNorm2d forward / backward (backbones/iresnet.py:46-57), one launch per
 * tensor pass.
 *   fedfr_bn_sliced_rows: rows such a pass writes for an [M][C] tensor (backward = 1: the backward passes, which use fewer, longer workgroups);  fedfr_bn_sliced_ok: whether the shape is served (else use the
 *   finalize + row-slab entry points above).
 *   fedfr_bn_apply_sliced: y = prelu?(bn(x1)) (+ x2); statistics of x1 = the P rows [2][C] at `partials`; writes scale / shift / mean / rstd
 *   [C], updates running_mean / running_var (NULL: skipped), and, with `stats`, the fedfr_bn_sliced_rows rows [2][C] of y (must not
 *   overlap `partials`).
 *   fedfr_bn_bwd_sliced: reduce pass into `partials` (fedfr_bn_sliced_rows rows [3][C]) unless rows_in > 0 says they are already there,
 *   then dx = BN(+PReLU) backward (+ add), dgamma / dbeta / dalpha assigned; with nx, dx is also reduced as the dy of the BatchNorm over
 *   nx (its mean / rstd given) into `npart` (rows [3][C], must not overlap `partials`).  sc / sh: the forward's scale / shift (PReLU mask). */
int fedfr_bn_sliced_rows(int M, int C, int backward);
int fedfr_bn_sliced_ok(int M, int C, int rows_in, int backward);
int fedfr_bn_apply_sliced(const float* partials, int P, double count, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, float momentum, float eps, float* scale, float* shift, float* save_mean,
                          float* save_rstd, const uint16_t* x1, const float* alpha, const uint16_t* x2, uint16_t* y, int M, int C,
                          float* stats, void* stream);
/* Round 3, the forward moment pass (option "fwd_xmom"; reference: the bn3 + identity of IBasicBlock.forward, backbones/iresnet.py:69-78, and the
 * bn1 of the NEXT block, :62).  fedfr_conv2d_fwd_moments: 3x3 / stride-1 conv whose epilogue leaves, per workgroup, rows [3][cout] of the raw
 * moments (sum y, sum y * other, sum y * y) of its 16-bit output against a same-shape tensor `other`; *rows = number of rows written (0: this
 * shape is not served by a kernel with that epilogue, nothing was written to `partials`, y is still computed).  `partials` must hold
 * batch * hin * hin / 196 rows.  fedfr_bn_apply2_sliced: y = bn(x1) + x2 and y2 = bn_next(y), both BatchNorms in training mode, from those
 * rows and the saved statistics (x2_mean, x2_rstd) of x2: the statistics of y are derived — mean = scale * mean(x1) + shift + mean(x2),
 * var = scale^2 var(x1) + var(x2) + 2 scale cov(x1, x2) — and written (with running statistics, scale / shift) for both BatchNorms. */
int fedfr_conv2d_fwd_moments(const uint16_t* x, const uint16_t* w, uint16_t* y, int batch, int hin, int cin, int cout, const uint16_t* other,
                             float* partials, int* rows, void* stream);
int fedfr_bn_apply2_sliced_ok(int M, int C, int rows);
int fedfr_bn_apply2_sliced(const float* partials, int P, double count, float momentum, float eps, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float* scale, float* shift, float* save_mean, float* save_rstd,
                           const float* x2_mean, const float* x2_rstd, const float* next_gamma, const float* next_beta,
                           float* next_running_mean, float* next_running_var, float* next_scale, float* next_shift, float* next_save_mean,
                           float* next_save_rstd, const uint16_t* x1, const uint16_t* x2, uint16_t* y, uint16_t* y2, int M, int C,
                           void* stream);
int fedfr_bn_bwd_sliced(const uint16_t* dy, const uint16_t* x, const float* mean, const float* rstd, const float* gamma,
                        const float* alpha, const float* sc, const float* sh, int M, int C, float* partials, int rows_in,
                        float* dgamma, float* dbeta, float* dalpha, const uint16_t* add, uint16_t* dx, const uint16_t* nx,
                        const float* nmean, const float* nrstd, float* npart, void* stream);

/* ------------------------------------------------------------------------------------------------
 * fp32 head — replaces FC_module.forward (client.py:69-74), CosFace/ArcFace (losses.py:17-45),
 * F.cross_entropy (client.py:545) and PartialFC's softmax/grad (partial_fc.py:138-166), BCE_module /
 * BCE_loss elementwise parts (client.py:45-58, losses.py:4-15).
 * ------------------------------------------------------------------------------------------------ */
int fedfr_normalize_rows(const float* x, float* xn, float* inv_norm, int R, int D, float eps, void* stream);
int fedfr_normalize_rows_bwd(const float* xn, const float* inv_norm, const float* dxn, float* dx, int R, int D,
                             float beta, void* stream);
/* C[m][n] = alpha * sum_k A[m*sam + k*sak] * B[k*sbk + n*sbn] (+bias[n]) (+beta*C); exact fp32 FMA chain */
int fedfr_sgemm(const float* A, const float* B, float* C, int M, int N, int K, long long sam, long long sak,
                long long sbk, long long sbn, int ldc, float alpha, float beta, const float* bias, void* stream);
/* Round 3, the dense head's latency chain (client.py:69-74 + losses.py:23-29 + client.py:545 at 128 x 1000 x 512): fedfr_sgemm as `splits`
 * split-K slabs C + z * slab_stride (k range z of ceil(K / splits) rounded up to 32; no bias / beta), whose consumers add the slabs in
 * order: fedfr_softmax_ce_fused = fedfr_margin_rowmax + fedfr_exp_rowsum + fedfr_softmax_grad in ONE launch for rows of <= 16384 classes
 * (bit-identical to the three; cosines summed over nslab slabs, gradient written over slab 0), fedfr_normalize_rows_bwd_slabs =
 * fedfr_normalize_rows_bwd on a dxn given as slabs.
 * The dense cross-entropy loss is taken in the log domain: nll_t[row] = (row_max - z_t) + log(row_sum) with z_t the target's logit
 * (fedfr_margin_rowmax writes it; -inf, hence nll_t = +inf, for a label outside [0, C)), finite where prob_t = exp(-nll_t) underflows
 * to 0 — F.cross_entropy's value; mean over rows = fedfr_sum_scale(nll_t, R, 1 / R).  z_t and nll_t (with row_max, z_t) may be NULL. */
int fedfr_sgemm_splitk(const float* A, const float* B, float* C, int M, int N, int K, long long sam, long long sak, long long sbk,
                       long long sbn, int ldc, float alpha, int splits, long long slab_stride, void* stream);
int fedfr_softmax_ce_fused(float* z, const long long* label, int R, int C, int ldz, float s, float m, int arcface, float inv_batch,
                           float* prob_t, int nslab, long long slab_stride, float* nll_t, void* stream);
int fedfr_normalize_rows_bwd_slabs(const float* xn, const float* inv_norm, const float* dxn, int nslab, long long slab_stride, float* dx,
                                   int R, int D, float beta, void* stream);
int fedfr_margin_rowmax(float* z, const long long* label, int R, int C, int ldz, float s, float m, int arcface,
                        float* row_max, float* dmul, float* z_t, void* stream);
int fedfr_exp_rowsum(float* z, int R, int C, int ldz, const float* row_max, float* row_sum, void* stream);
int fedfr_softmax_grad(float* z, const long long* label, int R, int C, int ldz, const float* row_sum,
                       const float* dmul, float s, float inv_batch, float* prob_t, const float* row_max, const float* z_t,
                       float* nll_t, void* stream);
int fedfr_margin_bwd(const float* dlogits, const long long* label, const float* dmul, float s, int R, int C, float* dcos,
                     void* stream);
int fedfr_nll_mean(const float* prob_t, int R, float floor_, float* loss, void* stream);
/* class-sharded softmax (PartialFC): fedfr_exp_rowsum that also emits the target's numerator — sums2 [2][R] = (sum_c e, e[label] or 0) —
 * so ONE sum all-reduce replaces partial_fc.py:147 and :161; fedfr_nll_mean_ratio: loss = -mean log(max(num/den, floor)) */
int fedfr_exp_rowsum_target(float* z, const long long* label, int R, int C, int ldz, const float* row_max, float* sums2,
                            void* stream);
int fedfr_nll_mean_ratio(const float* num, const float* den, int R, float floor_, float* loss, void* stream);
/* BCE personalised head: z = r*(g(cos) -/+ m) + bias, g(x) = 2((x+1)/2)^t - 1; gt[b][c] = (label[b] == c) */
int fedfr_bce_logits(const float* cosv, const long long* label, const float* bias, int B, int C, float m, float r, float t,
                     float* z, unsigned char* gt, float* dzdcos, void* stream);
/* row_loss[b] = sum_c bce(z, gt); dz = d(loss_scale * mean_b row_loss)/dz; dcos = dz * dzdcos (optional) */
int fedfr_bce_loss(const float* z, const unsigned char* gt, const float* dzdcos, int B, int C, float r, float lam,
                   float loss_scale, float* dz, float* dcos, float* row_loss, void* stream);
/* hard-negative mining (client.py:208-226, choose_hard_negative_2: `where(local @ public.T > thr)[1]`, union over rows):
 * flags[n] = 1 for every column n with alpha * sum_k A[m][k] B[k][n] > thr for some row m (flags are only ever set: zero them
 * first; exact fp32 MFMA, strided operands as fedfr_sgemm, the M x N similarity matrix is never materialised). */
int fedfr_sgemm_colflag(const float* A, const float* B, int M, int N, int K, long long sam, long long sak, long long sbk,
                        long long sbn, float alpha, float thr, unsigned char* flags, void* stream);
/* class-centre accumulation (client.py:171-178 data_update_fc, server.py:213-222 Initialize_pretrain_FC):
 * sums[c] += sum of the rows of feats whose label is c (batch order), counts[c] += their number. */
int fedfr_class_accumulate(const float* feats, const long long* label, int B, int D, int C, float* sums, float* counts,
                           void* stream);
/* sphnet building blocks (backbones/sphnet.py:4-13, :53-60: conv(+bias) -> PReLU, no normalisation).  Forward uses fedfr_bn_apply
 * with scale 1 / shift = bias.  Backward: z = x + bias (bias may be NULL), dz = dy * (z > 0 ? 1 : alpha), dbias = sum dz,
 * dalpha = sum dy * z over z <= 0, dx = dz (+ add).  partials: [fedfr_bn_bwd_rows][3][C], coef: [3][C] scratch. */
int fedfr_bias_prelu_bwd(const uint16_t* dy, const uint16_t* x, const float* bias, const float* alpha, int M, int C, float* partials,
                         float* coef, float* dbias, float* dalpha, const uint16_t* add, uint16_t* dx, void* stream);
/* The same backward as fedfr_net_backward runs it on sphnet, one pass at a time (thin wrappers for kernel-level tests; no reference counterpart):
 *   fedfr_prelu_bwd_pass: ONE streaming pass.  g = dy (+ add, the 16-bit rounded sum is written to gsum, required with add and is what the
 *   PReLU sees); z = x + bias (bias may be NULL); dz = g * (z > 0 ? 1 : alpha) -> dz; rows [fedfr_prelu_bwd_rows(M, C)][2][C] =
 *   (sum of the unrounded dz | sum g z over z <= 0) per workgroup.
 *   fedfr_prelu_bwd_finalize: P rows [2][C] -> dbias, dalpha (either may be NULL), summed in fp64.
 *   fedfr_prelu_bwd_finalize_multi: n = 1 ... 64 such finalizes in one launch.  Entry i: P[i] rows of nv_row[i] (2 or 3) statistics of C[i]
 *   channels (C % 8 == 0) at BYTE offset rows_off[i] of `base` (16-byte aligned), of which the first two are read; results at FLOAT offsets
 *   dbias_off[i] (< 0: none) and dalpha_off[i] of `grads`.  The offset arrays are host memory. */
int fedfr_prelu_bwd_rows(int M, int C);
int fedfr_prelu_bwd_pass(const uint16_t* dy, const uint16_t* add, const uint16_t* x, const float* bias, const float* alpha, int M, int C,
                         uint16_t* gsum, uint16_t* dz, float* rows, void* stream);
int fedfr_prelu_bwd_finalize(const float* rows, int P, int C, float* dbias, float* dalpha, void* stream);
int fedfr_prelu_bwd_finalize_multi(const void* base, float* grads, int n, const unsigned long long* rows_off, const long long* dbias_off,
                                   const long long* dalpha_off, const int* P, const int* C, const int* nv_row, void* stream);
/* eval-mode BatchNorm coefficients of n = 1 ... 160 BatchNorms in one launch (what fedfr_net_forward runs up front when not training, and
 * what freeze_BN training reads): entry i has C[i] channels, weight / bias at float offsets g_off[i] (< 0: weight = 1) / b_off[i] of `params`,
 * running mean / variance at rm_off[i] / rv_off[i] of `bufs`, and writes (scale, shift, mean, rstd), [4][C[i]], at save_off[i] of `save`:
 * rstd = 1 / sqrt(var + eps), scale = weight rstd, shift = bias - mean weight rstd, all in fp32.  The offset arrays are host memory. */
int fedfr_bn_eval_coeffs(const float* params, const float* bufs, float* save, int n, const int* C, const int* g_off, const int* b_off,
                         const int* rm_off, const int* rv_off, const int* save_off, float eps, void* stream);
/* fp32 NCHW [B][C][HW] -> 16-bit NHWC [B][HW][Cpad] with zero channels C..Cpad-1 (3-channel input of sphnet's first conv) */
int fedfr_pad_input_nhwc(const float* src_nchw, uint16_t* dst_nhwc, int B, int C, int HW, int Cpad, void* stream);
/* input pipeline (dataset.py:81-92): uint8 [B][H][W][3] + optional per-image flip flags -> fp32 [B][3][H][W] = (x/255 - 0.5)/0.5 */
int fedfr_preprocess_u8(const unsigned char* src_hwc, const unsigned char* flip, float* dst_nchw, int B, int H, int W, void* stream);
/* pairwise ROC histogram (roc_cuda.py:14-30 calc_ROC): over all pairs a < b with a < T (target rows first), b < N:
 * bin = int((<feats[a], feats[b]> + 1) * 1000) in fp64; hist[2*bin] += same label, hist[2*bin+1] += different label.
 * hist: 4002 uint64 counters, accumulated (zero them first). */
int fedfr_roc_histogram(const float* feats, const long long* label, int N, int D, int T, unsigned long long* hist, void* stream);
/* grouped pairwise ROC histogram (local_all.py:303-335: roc_cuda.py once per client on one feature matrix) in one pass: G disjoint
 * target sets.  row_index[n_tiles * 64] (device int32): feature rows in slot order, every group's rows starting at a multiple of 64,
 * -1 = padding, every row of feats at most once (rows that are nobody's target in tiles of group -1, or left out).  tile_group[n_tiles]
 * (HOST int32): group in [-1, G) of each 64-slot tile; it is copied to tile_group_dev[n_tiles] (device) on the stream.  For every
 * unordered pair of indexed rows {a, b} the bin of fedfr_roc_histogram is counted in hist[g(a)] if g(a) >= 0 and in hist[g(b)] if
 * g(b) >= 0 and g(b) != g(a): hist[c] equals fedfr_roc_histogram's result with group c's rows first.
 * hist: [G][4002] uint64 counters, accumulated (zero them first). */
int fedfr_roc_histogram_groups(const float* feats, const long long* label, int N, int D, const int* row_index, const int* tile_group,
                               int n_tiles, int G, int* tile_group_dev, unsigned long long* hist, void* stream);
/* 1:N identification (local_all.py:142-176 evaluation, one launch for all clients of :274-297): query [Q][D] fp32 with per-query id
 * qid[Q] (-1: not enrolled), gallery [G][D] fp32 with per-column id gid[G] (distinct among the ids >= 0), columns split into S client
 * segments by seg[S+1] (HOST memory, 0 = seg[0] < seg[1] < ... < seg[S] = G).  Scores are fp64 dot products of the fp32 features.
 * Pair (q, c) is positive iff qid[q] >= 0 && qid[q] == gid[c]; every other pair is a negative of the segment owning column c.
 * Outputs: pos[Q] fp64 (NaN where a query has no positive), neg_topk[S][K] fp64 (the K largest negatives of each segment, duplicates
 * counted, descending, -inf past neg_count), neg_count[S] int64.  1 <= K <= 1024.  The matrix is never materialised; results are exact
 * and run-to-run identical.  ws: fedfr_ident_workspace_bytes(Q, S, K) bytes of device memory. */
size_t fedfr_ident_workspace_bytes(int Q, int S, int K);
int fedfr_ident_topk(const float* query, const long long* qid, int Q, const float* gallery, const long long* gid, int G, int D,
                     const long long* seg, int S, int K, double* pos, double* neg_topk, long long* neg_count, void* ws, size_t ws_bytes,
                     void* stream);
/* IJB-C job 1:N (ijbc_all.py:367-427 evaluation): the fp64 form of the kernel above for one gallery, with ranks.  query [Q][D] and
 * gallery [G][D] fp64, mask[Q] int64 = the gallery row of the query's identity or -1 (all device memory).  Scores are
 * v_mfma_f64_16x16x4_f64 products accumulated over ascending k: for fp32-representable features the same fp64 numbers as
 * fedfr_ident_topk.  Outputs: pos[Q] fp64 = score of (q, mask[q]), NaN where mask[q] == -1; neg_topk[K] fp64 = the K largest scores of
 * the pairs (q, c != mask[q]), duplicates counted, descending, -inf past neg_count; neg_count int64; rank_gt[Q] / rank_eq[Q] int32 = the
 * number of columns c != mask[q] whose score is greater than / equal to pos[q] (-1 where mask[q] == -1), taken on the kernel's own
 * scores in a second sweep: query q is a top-k hit iff rank_gt[q] < k, and rank_eq[q] > 0 says that the answer depends on a tie.
 * 1 <= K <= 4096.  The matrix is never materialised; results are exact and run-to-run identical.  The device word *status (zero it
 * first) gets bit 1 when a score is not finite (a NaN / inf feature: the outputs are then unspecified; the reference drops NaN negatives
 * silently, callers here must refuse) and bit 2 when a mask entry lies outside [-1, G) (the entry is treated as -1).
 * ws: fedfr_ident_rank_workspace_bytes(Q, G, K) bytes of device memory. */
size_t fedfr_ident_rank_workspace_bytes(int Q, int G, int K);
int fedfr_ident_rank_topk(const double* query, int Q, const double* gallery, int G, int D, const long long* mask, int K, double* pos,
                          double* neg_topk, long long* neg_count, int* rank_gt, int* rank_eq, void* ws, size_t ws_bytes, int* status,
                          void* stream);
/* IJB-C template evaluation (ijbc_all.py image2template_feature_11/_1n, verification and the TPR@FPR table).
 * fedfr_template_pool: image features feats [N][D] fp32, or [N][2D] with flip = 1 (the two halves added, test mode F1); optional
 * faceness [N] (D1: an fp32 multiply); norm_images = 1 divides every image by its fp32 L2 norm first (use_norm_score=False; needs
 * fedfr_template_pool_workspace_bytes(N, 1) bytes of ws).  The CSR (device int32) lists template t's medias t_off[t] .. t_off[t+1]-1
 * (t_off [T+1] into [0, M]) and media m's images img[m_off[m]] .. (m_off [M+1] into [0, NI], every media non-empty, img[] < N).  Media
 * vector: the image itself, or the fp32 sum in list order divided once by the count; template vector: the fp32 sum of its medias in
 * order, written to raw [T][D] (optional).  out [T][D] fp64 = raw / ||raw||: mode 0 as sklearn normalize (a zero row stays zero),
 * mode 1 as the explicit divide.  A bad CSR entry sets bit 1 of the device word *status (the template is written as zeros).
 * D <= 128 or D in {256, 512, 1024}. */
size_t fedfr_template_pool_workspace_bytes(int N, int norm_images);
int fedfr_template_pool(const float* feats, int N, int D, int flip, const float* faceness, int norm_images, const int* t_off, int T,
                        const int* m_off, int M, const int* img, int NI, int mode, float* raw, double* out, void* ws, size_t ws_bytes,
                        int* status, void* stream);
/* fedfr_pair_scores_roc: for P pairs of template ids p1/p2 (int64, device), rows lut[id] (int32 [lut_n], -1 = no row) of feats [T][D]
 * fp64: score[p] = np.sum(f1 * f2, -1) bit for bit (numpy's pairwise order; optional).  With genuine != NULL also the ROC counts at the
 * G distinct genuine scores genuine[0] > genuine[1] > ... (label[p] == 1: genuine pair), accumulated into counts [3G+1] uint64 (zero
 * them first): [k] for k in [0, G] = impostors strictly between genuine[k-1] and genuine[k] (k = 0: above all, k = G: below all),
 * [G+1+k] = impostors equal to genuine[k], [2G+1+k] = genuine pairs equal to genuine[k].  ws: fedfr_roc_counts_workspace_bytes(P, G).
 * *status bit 2: a pair id without a row (its score is NaN); bit 4: a genuine score missing from the table; bit 8: a non-finite
 * score (not counted).  1 <= G <= 40000.
 * fedfr_roc_counts: the same counts for given scores. */
size_t fedfr_roc_counts_workspace_bytes(long long P, int G);
int fedfr_pair_scores_roc(const double* feats, int T, int D, const int* lut, long long lut_n, const long long* p1, const long long* p2,
                          long long P, double* score, const long long* label, const double* genuine, int G, unsigned long long* counts,
                          void* ws, size_t ws_bytes, int* status, void* stream);
int fedfr_roc_counts(const double* score, const long long* label, long long P, const double* genuine, int G, unsigned long long* counts,
                     void* ws, size_t ws_bytes, int* status, void* stream);
/* Spread-out regulariser of the class centres (server.py:48-63 SpreadOut_Module.forward and its autograd backward) on row-normalised
 * fn [N][D] fp32: S = fn fn^T, H_ij = max(S_ij - margin, 0) for i != j, H_ii = 0, c = 1 (mean = 0) or 1 / (N (N - 1)) (mean = 1):
 *   *loss = c * sum_ij H_ij^2 (summed in fp64),   dfn [N][D] = d(loss)/d(fn) = 4c * H fn   (H is symmetric: dS + dS^T = 2 dS),
 *   *active (optional) = the number of ordered pairs i != j with S_ij > margin.
 * d(loss)/d(FC) of the unnormalised centres is fedfr_normalize_rows_bwd of dfn.  S is an exact-fp32 MFMA product (k ascending) that is
 * never written to memory; every dfn row has one owner that adds the column tiles in ascending order and there are no floating-point
 * atomics, so two calls on the same input give the same bits.  N >= 2, D a multiple of 4 in [4, 1024]; fn and dfn must not overlap.
 * ws: fedfr_spreadout_workspace_bytes(N, D) bytes of device memory (O(N); 0 for unsupported sizes). */
size_t fedfr_spreadout_workspace_bytes(int N, int D);
int fedfr_spreadout_grad(const float* fn, int N, int D, float margin, int mean, float* dfn, float* loss, long long* active, void* ws,
                         size_t ws_bytes, void* stream);
/* BottleBlock converter of the personalised head (backbones/bottle.py; client.py:25-36 with converter_layer != 1), fp32, x [B][D], H = D / 4,
 * branch g = 0..3, LeakyReLU slope 0.01:
 *   h1_g = leaky(x W1_g^T + b1_g), h2_g = leaky(h1_g W2_g^T + b2_g), y = x + [h2_0|h2_1|h2_2|h2_3] W3^T + b3.
 * params / grads: HOST arrays of 18 DEVICE pointers in the order br1..br4 x (first weight [H][D], first bias [H], second weight [H][H],
 * second bias [H]), then concat_fc weight [D][D] and bias [D].  h1, h2 [B][D] (branch g in columns g H .. (g + 1) H) are written by the
 * forward and read by the backward; the pre-activations are never stored: leaky' is taken from the sign of the stored activation (0.01 at
 * exactly 0, as torch).  The backward writes all 18 gradients (overwriting) and dx = d y (residual) + the branch term; dx == NULL skips the
 * input gradient.  Exact-fp32 MFMA products, k ascending; every batch sum has one owner and a fixed order, no floating-point atomics: two
 * calls on the same input give the same bits.  Forward 2 launches, backward 2.  D a multiple of 64 in [64, 512], B >= 1 (bottle_rate 4).
 * ws: fedfr_bottle_workspace_bytes(B, D) bytes of device memory (0 for unsupported sizes). */
size_t fedfr_bottle_workspace_bytes(int B, int D);
int fedfr_bottle_forward(const float* x, const float* const* params, int B, int D, float* h1, float* h2, float* y, void* stream);
int fedfr_bottle_backward(const float* x, const float* const* params, const float* h1, const float* h2, const float* dy, int B, int D,
                          float* dx, float* const* grads, void* ws, size_t ws_bytes, void* stream);
/* Fused head of train_with_public_data (client.py:354-441; csrc/branch.hip), fp32, deterministic: no floating-point atomics anywhere.
 * fedfr_bce_fused: the personalised head's elementwise part in ONE pass over cos [B][C] (definitions: fedfr_bce_logits / fedfr_bce_loss above):
 *   row_loss[b] = sum_c bce(z[b][c], label[b] == c), dcos = d(loss_scale * mean_b row_loss)/dcos, dbias[c] = sum_b dz[b][c]; z, gt and dz/dcos are
 *   never stored.  A label outside [0, C) is an all-negative row.  dbias: one partial row per workgroup of 16 rows, added in ascending order by a
 *   second launch.  dcos must not alias cos.  ws: fedfr_bce_fused_workspace_bytes(B, C) bytes of device memory (0 for unsupported sizes). */
size_t fedfr_bce_fused_workspace_bytes(int B, int C);
int fedfr_bce_fused(const float* cosv, const long long* label, const float* bias, int B, int C, float m, float r, float t, float lam,
                    float loss_scale, float* row_loss, float* dcos, float* dbias, void* ws, size_t ws_bytes, void* stream);
/* dfeats = fedfr_normalize_rows_bwd_slabs(xn, inv_norm, dxn slabs) + dbce + mu * dcon in one pass over [B][D]; dbce (the BCE branch's gradient
 * wrt the converter input) and dcon (the contrastive gradient) may each be NULL. */
int fedfr_branch_dfeats(const float* xn, const float* inv_norm, const float* dxn, int nslab, long long slab_stride, const float* dbce,
                        const float* dcon, float mu, float* dfeats, int B, int D, void* stream);
/* The whole head as one call on the caller's stream:
 *   loss = CE(s * margin(cos(feats, fc)), labels) + bce_scale * BCE(cos(converter(feats), bce_weight); bce_bias) + mu * contrastive(feats, ...)
 * feats [B][D], labels [B] in [0, C), fc [C][D] (the first n_class rows are the local identities), arcface 0 = CosFace / 1 = ArcFace with s, m.
 * converter: 0 = no BCE branch (every bce / converter argument is ignored), 1 = Linear (converter_params = HOST array {weight [D][D], bias [D]}),
 * 2 = BottleBlock (HOST array of 18 device pointers as fedfr_bottle_forward takes them; D a multiple of 64 in [64, 512]); converter_grads: the
 * same layout, written.  bce_weight [n_class][D], bce_bias [n_class]; labels >= n_class (public identities) are all-negative BCE rows.
 * global_feats / last_feats [B][D]: both NULL = no contrastive term.  detach != 0: the BCE branch gives the embedding no gradient (BCE_detach).
 * Outputs (all overwritten): losses[4] = total, cos, contrastive, bce (an absent term is 0); dfeats [B][D]; dfc [C][D]; converter_grads;
 * dbce_weight [n_class][D]; dbce_bias [n_class].  The two identity-branch GEMMs run split-K when 256 <= C <= 4096 and D >= 256; beyond that the
 * d(f_hat) GEMM alone does once C >= 1024 (a long reduction over few tiles); the slabs are added in order by their consumers.  Every argument is checked before the first launch.
 * ws: fedfr_branch_workspace_bytes(...) bytes of device memory (0 for unsupported sizes); contrastive != 0 when global_feats is given. */
size_t fedfr_branch_workspace_bytes(int B, int D, int C, int n_class, int converter, int detach, int contrastive);
int fedfr_branch_head(const float* feats, const long long* labels, int B, int D, const float* fc, int C, int arcface, float s, float m,
                      int converter, const float* const* converter_params, const float* bce_weight, const float* bce_bias, int n_class,
                      float bce_m, float bce_r, float bce_t, float bce_lambda, float bce_scale, const float* global_feats,
                      const float* last_feats, float temperature, float mu, int detach, float* losses, float* dfeats, float* dfc,
                      float* const* converter_grads, float* dbce_weight, float* dbce_bias, void* ws, size_t ws_bytes, void* stream);
/* k-fold 1:1 verification (eval/verification.py test / evaluate / calculate_roc / calculate_val) in one pass over the embeddings of a
 * verification set: emb0 [2P][D], emb1 [2P][D] (the flipped images' embeddings; NULL = no flip test), both fp32 (fp64_input = 0) or
 * fp64 (1); rows 2p and 2p + 1 form pair p, issame [P] uint8.  Per row, in fp64: s = emb0 + emb1, with normalize = 1 divided by
 * sqrt(sum s^2) as sklearn.preprocessing.normalize does (a zero row stays zero), with normalize = 0 taken as it is; per pair
 * dist[p] = sum (a - b)^2 (optional output).  thr_a [Ta] and thr_b [Tb] (NULL = one table) are ascending fp64 threshold tables in
 * device memory; for each, k0 = #{k : thr[k] <= dist}, so np.less(dist, thr[k]) holds exactly for k >= k0, and
 *   counts_a [nfolds][2][Ta + 1], counts_b [nfolds][2][Tb + 1] uint64 (overwritten) count the pairs by fold, issame and k0;
 * folds are the contiguous ranges of KFold(n_splits = nfolds, shuffle = False) over the P pairs.  A NaN dist is counted in bin T (never
 * accepted) and sets *status bit 1 (zero *status first).  *norm_sum = the sum of the fp64 L2 norms of all raw rows of emb0 and emb1
 * (xnorm = norm_sum / number of rows), added in a fixed order: two calls give the same bits; the counts are integers.
 * D a multiple of 4 in [4, 1024]; 1 <= nfolds <= P; 2 (Ta + 1) + 2 (Tb + 1) <= 16000; embeddings 16-byte aligned.
 * ws: fedfr_verif_workspace_bytes(P, nfolds) bytes of device memory (0 for unsupported sizes). */
size_t fedfr_verif_workspace_bytes(int P, int nfolds);
int fedfr_verif_fold_counts(const void* emb0, const void* emb1, int fp64_input, int normalize, const unsigned char* issame, int P, int D,
                            int nfolds, const double* thr_a, int Ta, const double* thr_b, int Tb, unsigned long long* counts_a,
                            unsigned long long* counts_b, double* dist, double* norm_sum, int* status, void* ws, size_t ws_bytes,
                            void* stream);
/* model-contrastive term (client.py:372-375, :415-418): row_loss[b] = CE([cos(x,g)/T, cos(x,l)/T], 0) with
 * nn.CosineSimilarity(dim=1, eps=1e-8); dx = d(mean_b row_loss)/dx (optional).  g, l: frozen global / last-round embeddings. */
int fedfr_contrastive(const float* feats, const float* global_feats, const float* last_feats, int B, int D, float temperature,
                      float* row_loss, float* dfeats, void* stream);
int fedfr_colsum_f32(const float* x, int R, int C, float* out, void* stream);
int fedfr_sum_scale(const float* x, int n, float scale, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * optimiser / aggregation / PartialFC sampling — replace torch.optim.SGD.step (client.py:396,550),
 * FedPavg / FedAvg_on_FC (server.py:25-46), PartialFC.sample / update (partial_fc.py:89-116).
 * ------------------------------------------------------------------------------------------------ */
int fedfr_sgd_step(float* params, const float* grads, float* momentum_buf, uint16_t* h16_shadow, size_t n, float lr,
                   float momentum, float weight_decay, int first_step, void* stream);
/* fedfr_sgd_step on a gradient buffer that holds gradient / grad_scale (the GradScaler of client.py:394-396 with a static scale: the
 * fp16-storage build's backward pass runs on loss-scaled gradients): the kernel multiplies by grad_scale before the update and stores the
 * unscaled gradient back, so `grads` reads like p.grad afterwards.  grad_scale a power of two => bit-identical to unscale + fedfr_sgd_step.
 * Overflow guard (GradScaler.step's skip, without its host synchronisation): an element whose gradient is not finite keeps its parameter,
 * momentum and mirror value, and the device word *overflow (optional) is set to 1; the caller reads and clears it when it next synchronises. */
int fedfr_sgd_step_scaled(float* params, float* grads, float* momentum_buf, uint16_t* h16_shadow, size_t n, float lr, float momentum,
                          float weight_decay, int first_step, float grad_scale, unsigned* overflow, void* stream);
/* ------------------------------------------------------------------------------------------------
 * DRIFT TERMS — what a client optimises under FedProx (Li et al., MLSys 2020) and SCAFFOLD (Karimireddy et al., ICML 2020), inside the
 * same SGD kernel: one or two more read-only streams, no extra pass.  anchor = the round's global parameters x [n], a = prox = the proximal
 * coefficient, corr = the client's correction vector c - c_i [n].  Per element, every operation ONE fp32 rounding:
 *     d0 = fma(wd, p, g)                                   (as fedfr_sgd_step)
 *     d1 = anchor ? fma(a, fsub(p, anchor), d0) : d0
 *     d  = corr   ? fadd(d1, corr)              : d1
 *     buf = first ? d : fadd(fmul(buf, mu), d);   p = fma(-lr, buf, p)      (as fedfr_sgd_step)
 * g is the unscaled gradient: grad_scale and the overflow guard are fedfr_sgd_step_scaled's (an element whose gradient is not finite keeps p,
 * buf and its mirror value and sets *overflow, whatever anchor and corr hold there); overflow == NULL with grad_scale == 1 selects the
 * unguarded kernel, anything else the guarded one.  The 16-bit mirror is written as by fedfr_sgd_step.  The proximal term is part of the
 * update only: no loss value contains it.
 * FEDFR_ERR_ARG before any launch: anchor == NULL with prox != 0; anchor != NULL with prox == 0 or a prox that is not finite; anchor and
 * corr both NULL (fedfr_sgd_step / fedfr_sgd_step_scaled is the call to make); a buffer that is not 16-byte aligned; n == 0.
 * ------------------------------------------------------------------------------------------------ */
int fedfr_sgd_step_drift(float* params, float* grads, float* momentum_buf, uint16_t* h16_shadow, size_t n, float lr, float momentum,
                         float weight_decay, int first_step, float grad_scale, unsigned* overflow, const float* anchor, float prox,
                         const float* corr, void* stream);
/* SCAFFOLD's end-of-round pass of a client (option II of the paper, c_i+ = c_i - c + (x - y_i) / mass), one pass over six streams:
 *     t = fsub(x, y);  cn = fma(inv_mass, t, -corr);  dc = fsub(cn, c_i);  c_i = cn
 * x = the parameters the round started from, y = the trained ones, corr = the c - c_i the client trained with (NULL reads as +0.0),
 * inv_mass = fl32(1 / step_mass) with step_mass = sum_k lr_k (1 - mu^k) / (1 - mu) over the client's steps k = 1, 2, ... (the total weight
 * heavy-ball momentum gives the gradients of the run; mu = 0: sum_k lr_k).  c_i [n] is updated in place, dc [n] (another buffer) receives
 * the control update the client uploads.  FEDFR_ERR_ARG: a NULL or misaligned buffer, c_i == dc, n == 0, inv_mass not positive and finite. */
int fedfr_scaffold_control(float* c_i, float* dc, const float* x, const float* y, const float* corr, float inv_mass, size_t n, void* stream);
int fedfr_fedavg_axpy(float* dst, const float* src, float w, size_t n, int accumulate, void* stream);
/* dst = (accumulate ? dst : 0) + sum_i ws[i] * srcs[i] over k <= 8 client states (HOST arrays of k device pointers / k weights) in one pass,
 * ascending i, one fp32 multiply and one fp32 add per term: bit-identical to k fedfr_fedavg_axpy calls = the loop of server.py:27-33 */
int fedfr_fedavg_multi(float* dst, const float* const* srcs, const float* ws, int k, size_t n, int accumulate, void* stream);
int fedfr_fedavg_i64(float* acc, const long long* src, float w, int n, int accumulate, long long* out_trunc,
                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * server optimisers with update clipping — no reference counterpart (its --aggr_alg runs FedAvg only, server.py:328): the server-side
 * family of Reddi et al., "Adaptive Federated Optimization" (FedAvgM, FedAdagrad, FedAdam, FedYogi) on the flat fp32 parameter buffer,
 * as two one-pass streaming kernels beside fedfr_fedavg_multi.  Notation: x = the global parameters before the round [n], x_i = client
 * i's parameters after local training, k <= 8 clients per call, Delta = sum_i coef_i (x_i - x) the aggregated pseudo-gradient, m / v the
 * optimiser moments [n] (m starts at 0, v at tau^2 in every element; the caller owns and initialises them).
 *   1. fedfr_fedopt_sqnorm   sq_i = |x_i - x|^2 and coef_i = w_i min(1, clip / sqrt(sq_i)), on the device
 *   2. fedfr_fedopt_multi    Delta, the moment update and x' = x + step, reading x, m, v and every x_i once and writing x', m, v once
 * No call synchronises with the host; coef travels from 1 to 2 in device memory.  A caller that does not clip fills coef with w_i itself
 * and skips 1.  Every fp32 operation of 2 is a single correctly rounded + - * / sqrt in the order given below (nothing is contracted into
 * an fma), so a result can be reproduced bit for bit on a CPU (tests/fedopt_cases.py).
 * ------------------------------------------------------------------------------------------------ */
/* bytes of the workspace fedfr_fedopt_sqnorm needs for k clients of n elements: k x grid doubles, grid = min(ceil((n / 4 + 1) / 256), 2048)
 * (multi_state_grid in csrc/multi_state.h: the one launch rule of fedfr_fedavg_multi, fedfr_fedopt_* and fedfr_robust_*); 0 for k outside 1..8 or n = 0 */
size_t fedfr_fedopt_sqnorm_workspace_bytes(int k, size_t n);
/* Per-client squared update norms and clipped aggregation coefficients in one pass over x and the k client states (HOST arrays of k device
 * pointers xs / k weights ws, as fedfr_fedavg_multi):
 *   sq[i]   = sum_j (double) d_ij^2,  d_ij = x_i[j] - x[j] rounded to fp32 (the subtraction fedfr_fedopt_multi performs); square and sum in fp64
 *   coef[i] = (float) (ws[i] * min(1, clip / sqrt(sq[i])))   computed in fp64 and rounded once;  clip <= 0 or sq[i] == 0: coef[i] = ws[i]
 * sq (k doubles) and coef (k floats) are DEVICE arrays.  Deterministic, no atomics: every block writes one fp64 partial per client into
 * `workspace` ([k][grid], need not be initialised), lanes are reduced by a fixed shuffle tree, waves in ascending order through LDS, and a
 * second single-block launch adds the partials in ascending block order: two runs give identical bits.  x and xs[i] 16-byte aligned,
 * sq / workspace 8-byte aligned; FEDFR_ERR_WORKSPACE if workspace_bytes < fedfr_fedopt_sqnorm_workspace_bytes(k, n). */
int fedfr_fedopt_sqnorm(const float* x, const float* const* xs, const float* ws, int k, size_t n, float clip, double* sq, float* coef,
                        void* workspace, size_t workspace_bytes, void* stream);
/* One server-optimiser step.  kind: 0 FedAvgM, 1 FedAdagrad, 2 FedAdam, 3 FedYogi.  coef: DEVICE array of k floats (4-byte aligned).  Per element, every
 * operation rounded to fp32 once, in this order (b1 = beta1, c1 = one_minus_beta1, b2 = beta2, c2 = one_minus_beta2; the caller forms c1, c2 in fp32):
 *   D = first ? 0 : delta_scratch;  for i = 0 .. k-1:  D = D + coef[i] * (x_i - x)            (subtract, multiply, add)
 *   not last:  delta_scratch = D, nothing else is written
 *   last, kind 0:  m' = b1 * m + D                                        x' = x + lr * m'
 *         kind 1:  m' = b1 * m + c1 * D    v' = v + D * D
 *         kind 2:  m' = b1 * m + c1 * D    v' = b2 * v + c2 * (D * D)
 *         kind 3:  m' = b1 * m + c1 * D    v' = v - (c2 * (D * D)) * sign(v - D * D)   (sign(0) = 0)
 *         kinds 1-3:                                                      x' = x + (lr * m') / (sqrt(v') + tau)
 * No bias correction (as in the paper).  m, v are updated in place; x_out may be x.  More than 8 clients: chain calls over groups of <= 8 in
 * ascending client order with first = 1 on the first and last = 1 on the final group (delta_scratch [n] carries D between them; with one
 * call first = last = 1 and delta_scratch may be NULL); the result is bit-identical to one ascending loop over all clients.  v and beta2 /
 * one_minus_beta2 are ignored by kind 0 (v may be NULL); m, v, x_out may be NULL when last = 0.  delta_scratch may be one of the client
 * states when last = 0 (D overwrites it) and x_out when last = 1 (the all-reduce path of server.py forms w_i (x_i - x) and applies the summed D so).  All [n] buffers 16-byte aligned;
 * n % 4 trailing elements take a scalar path.  Bad arguments (NULL, k outside 1..8, misalignment, unknown kind) return FEDFR_ERR_ARG
 * before anything is launched. */
int fedfr_fedopt_multi(int kind, float* x_out, const float* x, const float* const* xs, const float* coef, int k, size_t n, float* m, float* v,
                       float* delta_scratch, int first, int last, float lr, float beta1, float one_minus_beta1, float beta2,
                       float one_minus_beta2, float tau, void* stream);

/* ------------------------------------------------------------------------------------------------
 * client-level differential privacy (DP-FedAvg, McMahan et al. 2018) — no reference counterpart.  fedfr_fedopt_sqnorm's clip bounds every
 * client's contribution to clip (the sensitivity); here are the Gaussian noise, generated on the device, and the server step that adds it
 * in the pass that already streams the client states.
 * THE NOISE STREAM.  Element e = offset + j of the logical stream (seed, round, stream_id) is lane e % 4 of the Philox4x32-10 block
 * (Salmon et al. 2011; multipliers 0xD2511F53 / 0xCD9E8D57, Weyl increments 0x9E3779B9 / 0xBB67AE85) with
 *   key = (seed low 32 bits, seed high 32 bits),   counter = (blk low 32, blk high 32, round low 32, stream_id),   blk = e / 4 (64 bits)
 * so a value depends on (seed, round, stream_id, e) only: not on the grid, on k, or on the number of passes of a chain.  Lanes (0, 1) and
 * (2, 3) of a block (words r_a, r_b) are Box-Muller pairs, in fp32:
 *   u1 = float((r_a >> 8) + 1) 2^-24 in (0, 1],  u2 = float(r_b >> 8) 2^-24 in [0, 1)   (both exact)
 *   rad = sqrt(-2 log(u1));   z_even = rad cospi(2 u2);   z_odd = rad sinpi(2 u2)         (|z| <= sqrt(48 ln 2) = 5.77)
 * offset must be a multiple of 4; with it a sharded or chunked buffer draws from one logical stream.  The n % 4 trailing elements take
 * the leading lanes of the block behind the last whole one (the same indexing).  tests/dp_cases.py restates the words bit for bit and
 * the Gaussian formula in fp64.
 * ------------------------------------------------------------------------------------------------ */
/* dst[j] = word (offset + j) of the stream, j < n.  dst 16-byte aligned; nothing is written behind n. */
int fedfr_philox_fill(unsigned* dst, size_t n, unsigned long long seed, unsigned long long round, unsigned stream_id,
                      unsigned long long offset, void* stream);
/* dst[j] = (accumulate ? dst[j] : 0) + std * z(offset + j): one fp32 multiply and one fp32 add, nothing contracted.  std finite. */
int fedfr_gaussian_fill(float* dst, size_t n, unsigned long long seed, unsigned long long round, unsigned stream_id,
                        unsigned long long offset, float std, int accumulate, void* stream);
/* fedfr_fedopt_multi with the Gaussian mechanism: on the LAST pass, after the sum over the clients and before the step,
 *   D = D + noise_std * z(offset + j)                                                       (multiply, add)
 * and one more kind, 4 = plain (DP-FedAvg proper):  x' = x + D, m and v neither read nor written (may be NULL).  Everything else —
 * arguments, chaining through delta_scratch, aliasing, alignment, the order of operations — is fedfr_fedopt_multi's.  noise_std must be
 * finite and >= 0; with noise_std = 0 nothing is drawn or added (no 0 * z), and kinds 0..3 ARE fedfr_fedopt_multi (the call is handed to
 * it: its bits, its messages).  Every pass of a chain must be given the chain's (noise_std, seed, round, stream_id, offset); only the
 * last pass uses them, so the noise is added exactly once (the entry point keeps no state: holding the earlier passes to it is the
 * caller's part).  z is the value fedfr_gaussian_fill writes for the same (seed, round, stream_id, offset + j), bit for bit.
 * FEDFR_ERR_ARG before anything is launched for what fedfr_fedopt_multi refuses, a noise_std that is negative or not finite, or an
 * offset that is not a multiple of 4. */
int fedfr_dp_multi(int kind, float* x_out, const float* x, const float* const* xs, const float* coef, int k, size_t n, float* m, float* v,
                   float* delta_scratch, int first, int last, float lr, float beta1, float one_minus_beta1, float beta2,
                   float one_minus_beta2, float tau, float noise_std, unsigned long long seed, unsigned long long round,
                   unsigned stream_id, unsigned long long offset, void* stream);

/* ------------------------------------------------------------------------------------------------
 * secure aggregation (Bonawitz et al., CCS 2017) — no reference counterpart.  A client uploads its update as fixed-point words under
 * pairwise and self masks; the server adds the uploads and the recovery streams and learns only the sum.  The masks come from a stream
 * cipher (a secure-aggregation mask must be indistinguishable from uniform without the key; Philox above is not a cipher).
 * THE MASK STREAM.  The generator is the ChaCha20 block function of RFC 8439 section 2.3: 20 rounds, then the input state is added.
 * State words 0-3 are the constants, 4-11 the key as 8 little-endian words, 12 the block counter, 13-15 three nonce words.  Element e of
 * the stream (key, counter0, nonce[3]) is word e % 16 of block counter0 + e / 16.  The counter is ONE 32-bit word: an entry returns
 * FEDFR_ERR_ARG for a call whose last block would pass 2^32 - 1.  A value depends on (key, nonce, counter0, e) only: not on the grid, on
 * the number of streams of a launch, or on how passes are chained.
 *   PROTOCOL NONCES (fedfr_amd/secagg.py).  nonce = (round low 32, round high 32, purpose), counter0 = 0; purpose 0 = pairwise mask,
 *   1 = self mask.  fedfr_secagg_mask and fedfr_secagg_aggregate always start their streams at counter0 = 0.
 *   ENCODING.  All arithmetic in Z / 2^32.  Client i with public weight w_i = n_i / sum n, c_i = fp32(fp32(w_i) 2^f) formed on the host
 *   (f = frac_bits, 8 ... 30), and K participants, L = (2^31 - 1) / K (integer division):
 *     d = x_i - x (one fp32 subtraction);  t = d c_i (one fp32 multiplication);  q = clamp(rint(t), -L, L) as int32, round half to even.
 *   A t that is NaN or infinite encodes as 0 and counts in `nonfinite`; a q equal to +L or -L counts in `saturated`.  The sum of K codes
 *   cannot leave the signed 32-bit range.
 *   MASKED UPLOAD.  y_i[e] = q_i[e] + sum_s sign_s m_s[e] mod 2^32 over the client's streams s (sign +1 for the pair mask with a peer
 *   j > i, -1 with a peer j < i, +1 for its own self mask).
 *   AGGREGATE.  S = sum_i y_i + sum_r sign_r m_r mod 2^32 over the received uploads and the recovery streams r;
 *     D = float(int32(S)) 2^-f rescale (one conversion, two fp32 multiplications);  out = x + D, or D when x is NULL.
 *   rescale = fp32(1 / sum of the survivors' w_i), exactly 1.0f when nobody dropped (the product is then the identity).  Addition mod
 *   2^32 is associative and commutative: S has ONE bit pattern whatever the order, the chaining or the grid.
 * keys ([k][8] words), nonces ([k][3] words) and signs (k values, each +1 or -1) are HOST arrays; they travel as one kernel argument.
 * tests/secagg_cases.py restates all of it in numpy, bit for bit.
 * ------------------------------------------------------------------------------------------------ */
/* dst[j] = word j of the stream (key[8], counter0, nonce[3]), j < n (key and nonce: HOST arrays).  dst 16-byte aligned; nothing is
 * written behind n; n = 0 is a no-op.  FEDFR_ERR_ARG for a NULL pointer, a misaligned dst, or a counter overflow. */
int fedfr_chacha20_fill(unsigned* dst, size_t n, const unsigned* key, unsigned counter0, const unsigned* nonce, void* stream);
/* y = encode(xi - x) + the k streams (0 <= k <= 32), as above, with coef = c_i and limit = L >= 1.  counters: DEVICE int32[2]
 * {saturated, nonfinite}, added to (atomically), may be NULL.  One pass: x and xi are read once (non-temporal), y is written once.
 * y, x, xi 16-byte aligned and distinct; n = 0 is a no-op.  Bad arguments return FEDFR_ERR_ARG before anything is launched. */
int fedfr_secagg_mask(unsigned* y, const float* x, const float* xi, float coef, int limit, const unsigned* keys, const unsigned* nonces,
                      const int* signs, int k, size_t n, int* counters, void* stream);
/* One pass of the aggregate over ku uploads (HOST array of 0 ... 8 device pointers) and k recovery streams (0 ... 32), ku + k > 0:
 *   S = (first ? 0 : acc) + sum ys + sum_r sign_r m_r;   last ? out = (x ? x + D : D) : acc = S.
 * More than 8 uploads or 32 streams: chain calls with first = 1 on the first and last = 1 on the final one, as fedfr_fedopt_multi (acc
 * [n] words carries S; with one call first = last = 1 and acc may be NULL).  x is read on the last pass only; out may be x.  With
 * <= 8 uploads and no dropout every upload word and x are read once and out is written once.  frac_bits 8 ... 30, rescale finite; all
 * [n] buffers 16-byte aligned; n = 0 is a no-op.  Bad arguments return FEDFR_ERR_ARG before anything is launched. */
int fedfr_secagg_aggregate(float* out, const float* x, unsigned* acc, const unsigned* const* ys, int ku, const unsigned* keys,
                           const unsigned* nonces, const int* signs, int k, int frac_bits, float rescale, size_t n, int first, int last,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * distributed differential privacy under secure aggregation (the distributed discrete Gaussian of Kairouz, Liu, Steinke, ICML 2021) — no
 * reference counterpart.  Every client clips its own update, encodes it as above, adds its own share of INTEGER Gaussian noise and masks
 * the result; the sum the server unmasks carries the noise of all surviving clients.
 * THE DISCRETE NOISE STREAM.  The target is N_Z(0, sigma^2), P(y) ~ exp(-y^2 / (2 sigma^2)) on the integers, 16 <= sigma <= 2^26 (fp64),
 * by the rejection scheme of Canonne, Kamath, Steinke (NeurIPS 2020): a discrete Laplace proposal of scale t = floor(sigma) + 1, thinned.
 * Attempt a = 0 ... 63 of element e = offset + j of the logical stream (seed, round, stream_id) takes the four words (w0, w1, w2, w3) of the
 * Philox4x32-10 block of THE NOISE STREAM with
 *   key = (seed low 32 bits, seed high 32 bits),   counter = (blk low 32, blk high 32, round low 32, stream_id),   blk = e * 64 + a (64 bits)
 * so a value depends on (seed, round, stream_id, e) only: not on the grid, on the lane, or on how many attempts a neighbour needed.
 * offset + n must not pass 2^58.  One attempt, in fp64, every operation rounded once, with s2 = sigma sigma, s2t = s2 / t,
 * c = -1 / (2 s2) formed on the host:
 *   U1 = double((w0 2^21 + (w1 >> 11)) + 1) 2^-53 in (0, 1],  U2 = double(w2 2^21 + (w3 >> 11)) 2^-53 in [0, 1)   (both exact),  B = w1 & 1
 *   G = floor(-t log(U1));   rejected if B == 1 and G == 0;   Y = B ? -G : G                          (|Y| <= 37 t)
 *   d = G - s2t;   p = exp((d d) c);   accepted iff U2 < p
 * The first accepted attempt is the value.  After 64 rejections (about 1e-40 per element) the value is 0 and the element is counted as
 * exhausted: a caller must treat a non-zero count as an error.  log and exp are the device library's; tests/ddp_cases.py restates the rest
 * operation by operation.
 *   THE CLIENTS' NOISE SHARES use stream_id 0x44444750 ("DDGP"; fedfr_secagg_mask_dp), beside stream_id 0 of the central mechanism's
 *   THE NOISE STREAM; the seed is the client's own secret of the round.
 * ------------------------------------------------------------------------------------------------ */
/* dst[j] = the value of element offset + j, j < n, as int32 (mod 2^32).  exhausted: DEVICE int32, added to.  dst 16-byte aligned; nothing
 * is written behind n; n = 0 is a no-op.  FEDFR_ERR_ARG for a NULL pointer, misalignment, sigma outside [16, 2^26] or offset + n > 2^58. */
int fedfr_dgauss_fill(int* dst, size_t n, unsigned long long seed, unsigned long long round, unsigned stream_id,
                      unsigned long long offset, double sigma, int* exhausted, void* stream);
/* fedfr_secagg_mask with the client's clip and noise share, one pass (x and xi read once, y written once):
 *   coef = clip_coef[0] 2^f (exact);   q = the ENCODING above of (xi - x) with this coef and limit = code_limit;
 *   y = q + noise(noise_offset + e) + sum_s sign_s m_s mod 2^32,   noise from the stream (noise_seed, noise_round, 0x44444750) at sigma.
 * clip_coef: DEVICE float, min(1, C / ||xi - x||) as fedfr_fedopt_sqnorm (k = 1, w = 1) leaves it: no host synchronisation between the
 * two passes.  sqnorm: DEVICE uint64, receives (is added) the exact sum of q^2 mod 2^64, taken BEFORE the noise: one reduction per
 * workgroup and one 64-bit atomic add (integer addition: one result whatever the order).  counters: DEVICE int32[3] {saturated,
 * nonfinite, exhausted}, added to.  counters and sqnorm may be NULL.  FEDFR_ERR_ARG before anything is launched for what fedfr_secagg_mask
 * refuses, frac_bits outside 8 ... 30, code_limit < 1, sigma outside [16, 2^26] or noise_offset + n > 2^58. */
int fedfr_secagg_mask_dp(unsigned* y, const float* x, const float* xi, const float* clip_coef, int frac_bits, int code_limit,
                         unsigned long long noise_seed, unsigned long long noise_round, unsigned long long noise_offset, double sigma,
                         const unsigned* keys, const unsigned* nonces, const int* signs, int k, size_t n, int* counters,
                         unsigned long long* sqnorm, void* stream);

/* ------------------------------------------------------------------------------------------------
 * narrow secure aggregation — no reference counterpart.  The masked upload above is one 32-bit word per parameter: as large as the fp32
 * state it hides.  Here a client uploads b = 8 or 16 bits per parameter and the server still learns only a sum, now in the small ring
 * Z / 2^b, by the recipe of Kairouz, Liu, Steinke (ICML 2021, sections 4 and 5): rotate the update so that no coordinate is large, round
 * stochastically so that the codes are unbiased, mask and sum modulo 2^b.  Block scales or indices (the compressed and top-k uploads)
 * cannot go under masks: they are per-client side information.  A fixed public scale can.
 * NARROW WORDS.  The constants of the format:
 *   ROTATION BLOCK.  B = 4096 elements; n_pad = ceil(n / B) B (fedfr_rht_padded_count); elements n ... n_pad - 1 of the update are 0.
 *   UPDATE.  u_e = x_i[e] - x[e], one fp32 subtraction, as above.
 *   ROTATION.  v = 2^-6 H_B (D u), block by block.  D is a PUBLIC Rademacher sign: element e is negated (its sign bit flipped) when bit
 *   e % 32 of word e / 32 of the Philox stream (rotation_seed, round, stream_id 0x52485444 "RHTD") of THE NOISE STREAM is 1 (word j =
 *   lane j % 4 of block j / 4).  H_B is the unnormalised Walsh-Hadamard butterfly, levels h = 1, 2, 4, ..., 2048 IN THAT ORDER; a level
 *   maps the pair (a, b) at distance h (a at an index whose bit h is clear) to (a + b, a - b), single fp32 operations.  The level order
 *   is part of the format: any parallel decomposition that keeps it gives the same bits.  The product with 2^-6 is exact.
 *   CODE.  t = v_e coef (one fp32 multiplication; coef = c_i of the ENCODING above);  fl = floor(t);  q = fl + [r 2^-24 < t - fl], with
 *   t - fl one fp32 subtraction and r the top 24 bits of word e of the client's PRIVATE Philox stream (private_seed, round, stream_id
 *   0x53525244 "SRRD"): a per-round seed the client draws and never sends.  q is clamped to +-L, L = (2^(b-1) - 1) / K (integer
 *   division, K participants); a t that is NaN or infinite gives 0.  Both cases count in {saturated, nonfinite} as above, over the n_pad
 *   rotated elements (one NaN in the update makes every element of its rotation block non-finite).  E[q] = t up to the
 *   rounding of t - fl (below 2^-24 of a code, and only for |t| < 2^-24 or so): the codes are unbiased.
 *   PACKING.  F = 32 / b codes per 32-bit word: element e is field e % F (little end first) of word e / F, as b-bit two's complement.
 *   An upload is n_pad / F words = n_pad b / 8 bytes.
 *   MASKS.  Packed word p takes word p of each ChaCha20 stream of THE MASK STREAM (counter0: the block of word 0; the counter check
 *   covers n_pad / F words).  Streams are added or subtracted FIELD-WISE mod 2^b: no carry or borrow crosses a field.  The server's sum
 *   of uploads and its recovery streams are field-wise too; the sum of K codes in +-L never wraps.
 *   DECODE.  Every field of the unmasked sum, sign-extended, is S;  s = float(S) 2^-f (exact);  u' = D (2^-6 H_B s): the same butterfly
 *   (the transform is its own inverse up to the scale);  out[e] = x[e] + rescale u'_e for e < n (one fp32 multiplication, one addition;
 *   u' alone when x is NULL); elements e >= n are dropped.
 * Field-wise addition is associative and commutative: the sum has ONE bit pattern whatever the order, the chaining or the grid.
 * tests/secagg_narrow_cases.py restates all of it in numpy, bit for bit.  How to choose f: INTEGRATION.md section 19.
 * ------------------------------------------------------------------------------------------------ */
size_t fedfr_rht_padded_count(size_t n);
/* The rotation alone: dst[0 .. n_pad) = 2^-6 H (D src) (inverse = 0) or D (2^-6 H src) (inverse != 0), src[e] = 0 for e >= n.  dst holds
 * n_pad floats, src n; both 16-byte aligned and distinct; n = 0 is a no-op. */
int fedfr_rht_fill(float* dst, const float* src, size_t n, unsigned long long rotation_seed, unsigned long long round, int inverse,
                   void* stream);
/* y[0 .. n_pad / F) = pack(code(rotate(xi - x))) (+) the k streams (0 <= k <= 32), as above, with L = (2^(bits-1) - 1) / participants.
 * counters: DEVICE int32[2] {saturated, nonfinite}, added to (atomically), may be NULL.  One pass: x and xi are read once, y is written
 * once, nothing else touches memory.  bits 8 or 16; 1 <= participants <= 2^(bits-1) - 1; y, x, xi 16-byte aligned and distinct; n = 0 is
 * a no-op.  Bad arguments, and a counter0 whose last block would pass 2^32 - 1, return FEDFR_ERR_ARG before anything is launched. */
int fedfr_secagg_mask_narrow(unsigned* y, const float* x, const float* xi, float coef, int participants, int bits,
                             unsigned long long rotation_seed, unsigned long long private_seed, unsigned long long round,
                             const unsigned* keys, const unsigned* nonces, const int* signs, int k, unsigned counter0, size_t n,
                             int* counters, void* stream);
/* One pass of the narrow aggregate over ku uploads (HOST array of 0 ... 8 device pointers, n_pad / F words each) and k recovery streams
 * (0 ... 32), ku + k > 0, all sums field-wise:
 *   S = (first ? 0 : acc) (+) sum ys (+) sum_r sign_r m_r;   last ? out = DECODE(S) : acc = S.
 * Chained as fedfr_secagg_aggregate (acc: n_pad / F words; with one call first = last = 1 and acc may be NULL).  x is read on the last
 * pass only; out may be x.  frac_bits 0 ... 30, rescale finite; all buffers 16-byte aligned; n = 0 is a no-op.  Bad arguments and a
 * counter overflow return FEDFR_ERR_ARG before anything is launched. */
int fedfr_secagg_aggregate_narrow(float* out, const float* x, unsigned* acc, const unsigned* const* ys, int ku, int bits,
                                  unsigned long long rotation_seed, unsigned long long round, const unsigned* keys, const unsigned* nonces,
                                  const int* signs, int k, unsigned counter0, int frac_bits, float rescale, size_t n, int first, int last,
                                  void* stream);

/* ------------------------------------------------------------------------------------------------
 * distributed differential privacy on narrow words — no reference counterpart: the two halves of Kairouz, Liu, Steinke (ICML 2021)
 * together.  A client clips, rotates, rounds stochastically, adds its share of discrete Gaussian noise mod 2^16, packs and masks.
 * NARROW WORDS UNDER DISTRIBUTED DP.  b = 16 only.  In this order:
 *   UPDATE, ROTATION.  As NARROW WORDS: v = 2^-6 H_B (D (x_i - x)) over the n_pad padded elements.
 *   CODE.  coef = fl(clip_coef[0] 2^f) (exact: a power-of-two scaling of the clip factor fedfr_fedopt_sqnorm left on the device);  the CODE
 *   of NARROW WORDS with this coef, the private draws of (private_seed, round, "SRRD") and the clamp +-code_limit, which the CALLER gives
 *   (privacy.DistributedDiscreteGaussian: (32767 - ceil(kappa sigma sqrt(K))) / K, the headroom the noise needs), not 32767 / K.
 *   SQUARED NORM.  sqnorm += sum of q_e^2 over ALL n_pad elements mod 2^64, taken before the noise.
 *   NOISE.  Element e = 4096 rb + 16 t + j, the POSITION IN THE PADDED ROTATED VECTOR, takes the value of element noise_offset + e of THE
 *   DISCRETE NOISE STREAM (noise_seed, noise_round, 0x44444750) at sigma: attempt a reads Philox block (noise_offset + e) 64 + a.  The
 *   n_pad - n PADDING COORDINATES CARRY NOISE like every other: after the rotation each of them holds a part of the update.
 *   noise_offset + n_pad must not pass 2^58.
 *   SUM, PACKING, MASKS.  field = q_e + noise_e mod 2^16; PACKING and MASKS of NARROW WORDS (counter0, field-wise streams).
 * The server's pass is fedfr_secagg_aggregate_narrow at bits = 16, unchanged: reduction mod 2^16 is a ring homomorphism, so a field of the
 * unmasked sum that wraps is post-processing of the noised integer sum (it costs accuracy, never privacy).  tests/ddp_narrow_cases.py
 * restates the pass from the restatements of its parts.
 * ------------------------------------------------------------------------------------------------ */
/* y[0 .. n_pad / 2) as above, one pass: x and xi read once, y written once.  counters: DEVICE int32[3] {saturated, nonfinite, exhausted},
 * added to; sqnorm: DEVICE uint64, added to; both may be NULL.  FEDFR_ERR_ARG before anything is launched for bits != 16, frac_bits outside
 * 8 ... 30, code_limit outside 1 ... 32767, sigma outside [16, 2^26], noise_offset + n_pad > 2^58, what fedfr_secagg_mask_narrow refuses of
 * the streams, NULL y / x / xi / clip_coef, y / x / xi not 16-byte, clip_coef / counters not 4-byte or sqnorm not 8-byte aligned, and a
 * counter0 whose last block would pass 2^32 - 1.  n = 0 is a no-op. */
int fedfr_secagg_mask_narrow_dp(unsigned* y, const float* x, const float* xi, const float* clip_coef, int frac_bits, int code_limit, int bits,
                                unsigned long long rotation_seed, unsigned long long private_seed, unsigned long long round,
                                unsigned long long noise_seed, unsigned long long noise_round, unsigned long long noise_offset, double sigma,
                                const unsigned* keys, const unsigned* nonces, const int* signs, int k, unsigned counter0, size_t n,
                                int* counters, unsigned long long* sqnorm, void* stream);

/* ------------------------------------------------------------------------------------------------
 * robust aggregation — no reference counterpart: every rule above is a weighted sum, so one client that returns a poisoned, diverged or NaN
 * state moves (or wipes out) the global model.  Coordinate-wise trimmed mean / median (Yin et al., 2018) and Krum / Multi-Krum (Blanchard
 * et al., 2017) over k <= 32 flat fp32 client states (HOST arrays of k device pointers, as fedfr_fedavg_multi), as streaming passes.
 * ------------------------------------------------------------------------------------------------ */
/* dst[j] = (s_trim + s_{trim+1} + ... + s_{k-1-trim}) / (float)(k - 2 trim), s_0 <= ... <= s_{k-1} the k values srcs[i][j] sorted, for every j.
 *   ORDER: a total order on bit patterns.  A value with bits u that is not a NaN compares by the unsigned key u ^ (sign ? 0xFFFFFFFF :
 *   0x80000000), so -inf < finite negatives < -0 < +0 < finite positives < +inf.  Every NaN has key 0xFFFFFFFF and sorts last: a NaN client
 *   is the first to be trimmed.  (A NaN that is kept makes the result NaN.)
 *   ARITHMETIC: acc = s_trim, then acc = acc + s_j in ascending sorted order, one fp32 rounding per addition; then one correctly rounded
 *   fp32 division by (float)(k - 2 trim).  Nothing is contracted, so the result can be reproduced bit for bit (tests/robust_cases.py).
 * trim = (k - 1) / 2 is the coordinate-wise median (the middle value, or the mean of the middle two); trim = 0 the unweighted mean in sorted
 * order.  Requires 1 <= k <= 32 (an order statistic cannot be chained over groups of clients the way a sum can), 0 <= 2 trim < k, all
 * buffers 16-byte aligned, dst overlapping no source.  Every source is read once (non-temporal loads); n % 4 trailing elements take a scalar path. */
int fedfr_robust_trimmed_mean(float* dst, const float* const* srcs, int k, int trim, size_t n, void* stream);
/* bytes of the workspace fedfr_robust_pairdist needs: k (k - 1) / 2 x grid doubles, grid as for fedfr_fedopt_sqnorm_workspace_bytes
 * (multi_state_grid); 0 for k outside 2..32 or n = 0 */
size_t fedfr_robust_pairdist_workspace_bytes(int k, size_t n);
/* dist[i][j] = sum_e (double) d_e^2, d_e = xs[i][e] - xs[j][e] rounded to fp32; square and sum in fp64 (exact product, one rounding per term).
 * dist: DEVICE array [k][k] of doubles, symmetric, zero diagonal.  Deterministic, no atomics: one fp64 partial per pair and block in
 * `workspace` (need not be initialised), reduced in a fixed order (lanes, waves, blocks): two runs give identical bits.  2 <= k <= 32; k <= 13
 * is one pass that reads every state once, more clients are tiled in groups of 8 (at most 16 distinct states per launch).  xs[i] 16-byte,
 * dist / workspace 8-byte aligned; FEDFR_ERR_WORKSPACE if workspace_bytes < fedfr_robust_pairdist_workspace_bytes(k, n). */
int fedfr_robust_pairdist(const float* const* xs, int k, size_t n, double* dist, void* workspace, size_t workspace_bytes, void* stream);
/* Krum / Multi-Krum on a distance matrix (DEVICE [k][k] doubles): score[i] = the k - f - 2 smallest dist[i][j], j != i, added in ascending
 * order in fp64 (an entry that is not finite counts as +inf); selected[i] = 1 for the m lowest scores (ties: the lower client index), else 0.
 * score (k doubles) and selected (k int32) are DEVICE arrays.  Requires 2 f + 3 <= k <= 32 and 1 <= m <= k - f (m = 1: Krum). */
int fedfr_robust_krum_select(const double* dist, int k, int f, int m, double* score, int* selected, void* stream);

/* ------------------------------------------------------------------------------------------------
 * reweighted aggregation — the two vector-wise robust rules that use every honest client: the geometric median (RFA, the smoothed
 * Weiszfeld iteration of Pillutla, Kakade and Harchaoui, 2019) and centred clipping (Karimireddy, He and Jaggi, 2021).  Both are "weights
 * from the distances to the current centre, one weighted step, repeat", so both run on ONE streaming pass and one single-block kernel:
 * R iterations are R + 1 passes and R + 1 small launches, back to back on one stream, no host round trip in between.
 * Notation: x_0 .. x_{k-1} the clients' flat fp32 states [n], k <= 32 (HOST array of k device pointers, as fedfr_fedavg_multi); z the centre
 * [n]; beta a DEVICE array of k fp32 weights.
 *
 * STEP PASS (fedfr_reweight_step), for every element; every operation is one correctly rounded fp32 operation, nothing is contracted:
 *   delta_i = x_i - z
 *   acc = z;  for i = 0 .. k-1 ascending:  if beta[i] != 0:  acc = acc + beta[i] * delta_i        (one multiply, one add)
 *   z' = acc                              a client with beta[i] == 0 is SKIPPED (a select, not a product with zero: its NaN or inf never reaches z')
 *   e_i = x_i - z'                        for every client, the skipped ones included
 *   D_i = D_i + (double) e_i * (double) e_i     in fp64 (the product is exact: one rounding per term)
 * dst == NULL is the distance-only mode: beta is not read, nothing but the workspace is written, z' = z and D_i = |x_i - z|^2.  dst may be z
 * (in place: a thread reads an element before it writes it); otherwise dst overlaps neither z nor a client state.  The D_i are NOT finished
 * by this call: every block writes one fp64 partial per client into `workspace` ([k][grid], need not be initialised; lanes by a fixed
 * shuffle tree, waves in ascending order); fedfr_reweight_weights adds the blocks in ascending order.  No atomics: two runs give the same bits.
 *
 * WEIGHTS (fedfr_reweight_weights), one block, fp64, each beta rounded to fp32 once.  D_i = the sum of client i's partials, d_i = sqrt(D_i);
 * a client whose D_i is not finite gets beta_i = 0; alpha_i >= 0 are the prior weights (HOST array of k doubles):
 *   rule 0, geometric median:  w_i = alpha_i / max(nu, d_i) (0 for a non-finite client);  S = w_0 + ... + w_{k-1} ascending;
 *                              beta_i = (float) (w_i / S)   (S == 0: every beta_i = 0).                  param = nu > 0
 *   rule 1, centred clipping:  beta_i = (float) (alpha_i * min(1, tau / d_i)), d_i == 0 gives alpha_i;  S = (double) beta_0 + ... ascending.
 *                              param = tau > 0, or 0 for AUTO: tau = the lower median of the finite d_i of slot 0 (the distance-only pass:
 *                              of m finite values sorted ascending, number (m - 1) / 2), computed at slot 0 and read back from info at
 *                              every later slot of the round.
 * `slot` 0 .. iters numbers the passes of a round.  The call writes D into hist_d[slot][0 .. k) (DEVICE, (iters + 1) x k doubles), and,
 * for slot < iters, beta into hist_beta[slot][0 .. k) (DEVICE, iters x k floats: the weights of step slot + 1).  info (DEVICE, 4 doubles):
 * [0] the tau in use (rule 1), [1] S of this slot, [2] 1.0 once a slot of the round had no finite client (slot 0 resets it to 0.0), [3] the
 * number of finite clients of this slot.
 * ------------------------------------------------------------------------------------------------ */
#define FEDFR_REWEIGHT_GEOMEDIAN 0
#define FEDFR_REWEIGHT_CCLIP 1
/* bytes of the workspace of fedfr_reweight_step / _weights: k x grid doubles, grid as for fedfr_fedopt_sqnorm_workspace_bytes
 * (multi_state_grid); 0 for k outside 1..32 or n = 0 */
size_t fedfr_reweight_workspace_bytes(int k, size_t n);
/* One step pass (above).  dst NULL (distance-only; beta may be NULL) or [n]; z [n]; xs HOST array of k device pointers; beta DEVICE [k].
 * 1 <= k <= 32, n > 0; dst, z, xs[i] 16-byte aligned, beta 4-byte, workspace 8-byte aligned; FEDFR_ERR_WORKSPACE if workspace_bytes <
 * fedfr_reweight_workspace_bytes(k, n).  Every state is read once (non-temporal loads); n % V trailing elements take a scalar path. */
int fedfr_reweight_step(float* dst, const float* z, const float* const* xs, const float* beta, int k, size_t n, void* workspace,
                        size_t workspace_bytes, void* stream);
/* The weights of the next step from the partials fedfr_reweight_step left in `workspace` for the same (k, n) (above).  rule 0 / 1; alpha HOST
 * array of k finite doubles >= 0; param: nu > 0 (rule 0), tau > 0 or 0 = auto (rule 1); 0 <= slot <= iters, iters >= 1.  hist_d, info,
 * workspace 8-byte aligned, hist_beta 4-byte aligned. */
int fedfr_reweight_weights(int rule, const double* alpha, double param, int slot, int iters, int k, size_t n, const void* workspace,
                           size_t workspace_bytes, double* hist_d, float* hist_beta, double* info, void* stream);

/* ------------------------------------------------------------------------------------------------
 * compressed client uploads with error feedback — no reference counterpart (its clients hand over full fp32 states).  A client sends
 * Q(x_i - x + e_i) and keeps the quantisation error e_i for the next round.  Codes of bits = 8 or 4 with ONE shared power-of-two scale
 * per 32 elements (the OCP microscaling layout): 8.25 or 4.25 bits per parameter instead of 32.  Every scale is a power of two, so
 * scaling and rescaling are exact and every output of both kernels can be reproduced bit for bit (tests/compress_cases.py).
 * THE FORMAT.  qmax = 2^(bits-1) - 1 (127 or 7); block b = elements 32 b .. min(32 b + 31, n - 1) (the last block may be short).
 *   1. value to send   v_j = (x_i[j] - x[j]) + e[j]: two fp32 operations in that order; without error feedback v_j = x_i[j] - x[j].
 *   2. non-finite      a block with any v_j NaN or +-inf: scale byte 255 (reserved for exactly this: step 3 never produces it), all codes
 *                      0, new residual +0 for the whole block (a diverged round must not poison the residual forever), and the block
 *                      adds 1 to the nonfinite_blocks counter.
 *   3. scale           otherwise amax = max |v_j| over the block, Ef = the biased exponent field of amax (0 for zero and subnormals);
 *                      scale byte eb = clamp(Ef - (bits - 2), 0, 254), scale = 2^(eb - 127).  amax / scale is in [2^(bits-2), 2^(bits-1))
 *                      unless eb is clamped at 0 (which only makes it smaller); Ef <= 254 gives eb <= 252.
 *   4. code            q_j = clamp(rint(v_j * 2^(127 - eb)), -qmax, qmax), rint = round half to even.  The product is exact wherever the
 *                      result can be non-zero; only |v_j| >= (qmax + 1/2) scale saturates.
 *   5. layout          8 bits: byte j = q_j as int8.  4 bits: byte j holds q_2j in the low and q_2j+1 in the high nibble (two's-complement
 *                      nibbles; a missing last element is 0).  Scale byte b belongs to block b.  ceil(n bits / 8) code bytes, ceil(n / 32)
 *                      scale bytes.
 *   6. dequantise      dq_j = float(q_j) * 2^(eb - 127): exact, subnormal scales included; eb = 255 gives NaN for the whole block, so the
 *                      server sees the poison as it would with fp32 uploads.
 *   7. residual        e'[j] = v_j - dq_j, one fp32 subtraction: dq + e' == v exactly for every finite block, |e'| < scale, and
 *                      |e'| <= scale / 2 where the element did not saturate.
 * ------------------------------------------------------------------------------------------------ */
/* ceil(n bits / 8): bytes of the code buffer of n elements; 0 for bits other than 4 or 8 */
size_t fedfr_delta_code_bytes(int bits, size_t n);
/* ceil(n / 32): bytes of the scale buffer of n elements */
size_t fedfr_delta_scale_bytes(size_t n);
/* One pass over x (global parameters), xi (client parameters) and resid (e, read and updated in place to e'): each is read once, codes, scale
 * bytes and e' are written once.  resid may be NULL: no error feedback, nothing read or written for it.  nonfinite_blocks may be NULL;
 * otherwise a DEVICE int the caller has zeroed, to which every non-finite block adds 1 (an integer atomic: order-free).  codes holds
 * fedfr_delta_code_bytes(bits, n), scales fedfr_delta_scale_bytes(n) bytes.  x, xi, resid, codes and scales 16-byte aligned (the scale
 * bytes of 512 elements leave as one 16-byte store).  FEDFR_ERR_ARG, before anything is launched, for bits other than 4 or 8, a NULL x, xi,
 * codes or scales, or a misaligned buffer; n = 0 with valid arguments is a no-op. */
int fedfr_delta_quantize(const float* x, const float* xi, float* resid, void* codes, unsigned char* scales, int bits, size_t n,
                         int* nonfinite_blocks, void* stream);
/* The weighted sum of k <= 8 uploads in one pass (HOST arrays of k device pointers codes / scales and k weights ws, as fedfr_fedavg_multi):
 *   s = accumulate ? dst[j] + ws[0] dq_0[j] : ws[0] dq_0[j];   s = s + ws[i] dq_i[j] for ascending i;   dst[j] = base ? base[j] + s : s
 * Each product is one fp32 multiply and each sum one fp32 add, nothing contracted: the roundings of k axpy launches on the dequantised
 * uploads.  More than 8 uploads chain calls with accumulate = 1 and pass base (the global parameters x) to the last one only.  dst may
 * equal base.  dst, base and every code buffer 16-byte aligned.  FEDFR_ERR_ARG, before anything is launched, for bits other than 4 or 8,
 * k outside 1..8, a NULL dst, codes, scales, ws or array entry, or a misaligned buffer; n = 0 with valid arguments is a no-op. */
int fedfr_delta_aggregate(float* dst, const float* base, const void* const* codes, const unsigned char* const* scales, const float* ws, int k,
                          int bits, size_t n, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * top-k sparsified client uploads with error feedback — no reference counterpart.  A client sends the `keep` largest-magnitude entries of
 * x_i - x + e_i as (index, value) pairs, 8 bytes per kept parameter, and keeps everything else as e_i for the next round.  The selection
 * is EXACT (a radix select on the device: no sampling, no approximate threshold) and nothing is rounded after step 1, so every output of
 * both kernels can be reproduced bit for bit (tests/sparse_cases.py).  1 <= keep <= n < 2^31.
 * THE FORMAT.
 *   1. value to send   v_j = (x_i[j] - x[j]) + e[j]: two fp32 operations in that order; without error feedback v_j = x_i[j] - x[j]
 *                      (step 1 of fedfr_delta_quantize).
 *   2. key             key_j = bits(v_j) & 0x7FFFFFFF, a 31-bit unsigned integer whose order is the order of |v_j|: +-0 have key 0,
 *                      subnormals order correctly, inf (0x7F800000) and every NaN (above it) order above every finite value, so what
 *                      a diverged client produces is always sent and the server sees it, as it would with fp32 uploads.
 *   3. selection       S = the keep elements that come first when sorted by (key descending, index ascending).  Equivalently: T = the
 *                      keep-th largest key, r = keep - #{key > T}, S = {key > T} and the r lowest-index elements with key == T.
 *   4. upload          idx: uint32 [keep], strictly ascending; val: fp32 [keep], val[t] = v[idx[t]] bit for bit (NaN payloads and the
 *                      sign of zero included).  Element j of S lands at t = #{key > T, index < j} + min(#{key == T, index < j}, r).
 *   5. residual        e'[j] = +0 if j is in S or v_j is not finite (a diverged round must not poison the residual), otherwise
 *                      e'[j] = v_j: scatter(idx, val) + e' == v exactly wherever v is finite and non-zero.
 *   6. counter         nonfinite adds the number of non-finite ELEMENTS of v (an integer atomic: order-free).
 * ------------------------------------------------------------------------------------------------ */
/* bytes of the workspace fedfr_topk_sparsify needs: the select state and three digit histograms, one pair of counts per tile of 2048
 * elements, and WITHOUT error feedback the n values v (with it they live in the residual buffer).  A multiple of 16, monotone in n. */
size_t fedfr_topk_workspace_bytes(size_t n, int feedback);
/* Stream-ordered, no host synchronisation and no device-to-host copy: T and r stay on the device.  A chain of launches on `stream`, none
 * of which waits for another workgroup of its own launch: v and the histogram of the top 11 key bits; two more histogram passes (10 bits
 * each) over the elements under the prefix chosen so far, each followed by a one-workgroup kernel that picks the bin; a pass that counts
 * (#key > T, #key == T) per tile; a one-workgroup scan of those counts; the emit pass.  Histograms are integer sums (LDS atomics, then
 * global atomics); there are no float atomics.  x (global parameters) and xi (client parameters) are read-only; resid (e) ends as e' and
 * may be NULL: no error feedback, nothing read or written for it; idx and val receive exactly keep entries; nothing is written behind any
 * buffer.  nonfinite may be NULL; otherwise a DEVICE int the caller has zeroed.  ws: fedfr_topk_workspace_bytes(n, resid != NULL) bytes,
 * need not be initialised.  x, xi, resid, idx, val and ws 16-byte aligned.  FEDFR_ERR_ARG, before anything is launched, for a NULL x, xi,
 * idx, val or ws, keep = 0 or keep > n, n >= 2^31, or a misaligned buffer; n = 0 with keep = 0 is a no-op. */
int fedfr_topk_sparsify(const float* x, const float* xi, float* resid, size_t n, size_t keep, unsigned* idx, float* val, int* nonfinite,
                        void* ws, void* stream);
/* The weighted sum of k <= 8 top-k uploads in one launch (HOST arrays of k device pointers idx / val, k entry counts keeps and k weights
 * ws, as fedfr_delta_aggregate).  Per element j:
 *   s = accumulate ? dst[j] : +0;   for ascending i with j in idx_i: s = s + ws[i] val_i[t];   dst[j] = base ? base[j] + s : s
 * One fp32 multiply and one fp32 add per entry, nothing contracted, no float atomics: a workgroup keeps a tile of s in LDS, adds the
 * uploads' entries of that tile upload by upload, and writes dst once.  More than 8 uploads chain calls with accumulate = 1 and pass base
 * (the global parameters x) to the last one only.  dst may equal base; the uploads may hold different numbers of entries.  Every idx_i
 * must be strictly ascending and below n; for ANY index content an entry is applied only if it lies inside the tile at hand, so a
 * malformed upload gives an unspecified sum but never an out-of-bounds access.  dst, base, idx_i and val_i 16-byte aligned.
 * FEDFR_ERR_ARG, before anything is launched, for k outside 1..8, a NULL dst, idx, val, keeps, ws or array entry, keeps[i] > n,
 * n >= 2^31, or a misaligned buffer; n = 0 with valid arguments is a no-op. */
int fedfr_sparse_aggregate(float* dst, const float* base, const unsigned* const* idx, const float* const* val, const size_t* keeps,
                           const float* ws, int k, size_t n, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * clip and Gaussian noise for compressed and top-k uploads — no reference counterpart.  The server bounds one client's influence on the
 * round by the norm of its upload AS THE SERVER WILL APPLY IT (the dequantised codes, the scattered entries), and may add the noise of
 * THE NOISE STREAM above.  Two steps, no host round trip between them: a norm pass that leaves the clipped weights on the device, and
 * the aggregates of the two sections above with their weights read from there.
 * THE NORMS.
 *   compressed   per block b of 32 elements S_b = sum q_j^2, an integer (<= 32 * 128^2: exact), T_b = double(S_b) 4^(eb_b - 127), exact
 *                in fp64 for every scale byte 0..254 (a 20-bit integer times a power of two between 2^-254 and 2^254); sq_i = sum_b T_b.
 *                A block with scale byte 255 contributes NaN.  Elements at index >= n of the last block (the pad nibble of an odd 4-bit
 *                n included) are not counted, whatever the upload holds there.  Code -128 (8 bits) and -8 (4 bits), which
 *                fedfr_delta_quantize never produces, count as 128^2 and 8^2: what fedfr_delta_aggregate would apply.
 *   top-k        sq_i = sum_e double(val_e)^2 (the square of an fp32 value is exact in fp64).  The scattered vector has this norm only if
 *                the indices are distinct and in range: violations_i counts the entries with idx_e >= n or idx_e <= idx_(e-1).
 *   order        the sums are fp64 in ONE fixed order, as fedfr_fedopt_sqnorm's: a thread's terms in its grid-stride order, the lanes of
 *                a wave by the xor-shuffle tree, the four waves ((w0 + w1) + w2) + w3, one partial per upload and block in `workspace`,
 *                the blocks ascending.  No float atomics; two runs give identical bits whatever the workspace held before.
 *   coefficient  coef_i = ws[i] min(1, clip / sqrt(sq_i)) in fp64, rounded to fp32 once (the final kernel of fedfr_fedopt_sqnorm itself);
 *                clip <= 0, sq_i = 0 or a NaN sq_i (the comparison fails) leave coef_i = ws[i].
 * ------------------------------------------------------------------------------------------------ */
/* bytes of the workspace of fedfr_delta_sqnorm (second argument: n) and fedfr_sparse_sqnorm (second argument: the largest keeps[i]):
 * k x grid doubles, grid = min(ceil((m / 8 + 1) / 256), 2048); 0 for k outside 1..8 */
size_t fedfr_upload_sqnorm_workspace_bytes(int k, size_t n_or_max_keep);
/* One pass over k <= 8 compressed uploads (HOST arrays of k device pointers codes / scales and k weights ws, as fedfr_delta_aggregate):
 * every code and scale byte is read once, no fp32 state is touched (8 bits: 1.03 bytes per parameter and upload).  sq: DEVICE double[k],
 * coef: DEVICE float[k], both written.  Code buffers 16-byte, sq and workspace 8-byte, coef 4-byte aligned.  FEDFR_ERR_ARG, before anything
 * is launched, for bits other than 4 or 8, k outside 1..8, a NULL codes, scales, ws, sq, coef, workspace or array entry, n = 0, a NaN clip
 * or a misaligned buffer; FEDFR_ERR_WORKSPACE if workspace_bytes < fedfr_upload_sqnorm_workspace_bytes(k, n). */
int fedfr_delta_sqnorm(const void* const* codes, const unsigned char* const* scales, const float* ws, int k, int bits, size_t n, float clip,
                       double* sq, float* coef, void* workspace, size_t workspace_bytes, void* stream);
/* The same over k <= 8 top-k uploads (idx / val / keeps / ws as fedfr_sparse_aggregate; keeps[i] = 0 is an upload of norm 0).
 * violations: DEVICE int[k], ADDED to (integer atomics: order-free); the caller zeroes it.  Index and value buffers 16-byte, sq and
 * workspace 8-byte, coef and violations 4-byte aligned.  FEDFR_ERR_ARG, before anything is launched, for k outside 1..8, a NULL idx, val,
 * keeps, ws, sq, coef, violations, workspace or array entry, keeps[i] > n, n = 0 or n >= 2^31, a NaN clip or a misaligned buffer;
 * FEDFR_ERR_WORKSPACE if workspace_bytes < fedfr_upload_sqnorm_workspace_bytes(k, max keeps[i]). */
int fedfr_sparse_sqnorm(const unsigned* const* idx, const float* const* val, const size_t* keeps, const float* ws, int k, size_t n, float clip,
                        double* sq, float* coef, int* violations, void* workspace, size_t workspace_bytes, void* stream);
/* fedfr_delta_aggregate, operation for operation, with coef[i] (DEVICE float[k], read once per thread) in the place of ws[i], and on the
 * LAST pass of a chain, if noise_std > 0, before base is added:
 *   s = s + noise_std * z(offset + j)                                                      (one fp32 multiply, one fp32 add)
 * z as fedfr_gaussian_fill writes it for the same (seed, round, stream_id, offset + j), bit for bit: the value depends on nothing else,
 * not on the grid, on k or on the number of passes.  Every pass of a chain must be given the chain's (noise_std, seed, round, stream_id,
 * offset); only the pass with last != 0 draws.  With noise_std = 0 nothing is drawn or added and the result is fedfr_delta_aggregate's
 * for ws = coef, bit for bit.  FEDFR_ERR_ARG, before anything is launched, for what fedfr_delta_aggregate refuses (coef for ws; coef
 * 4-byte aligned), a noise_std that is negative or not finite, or an offset that is not a multiple of 4. */
int fedfr_delta_aggregate_dp(float* dst, const float* base, const void* const* codes, const unsigned char* const* scales, const float* coef,
                             int k, int bits, size_t n, int accumulate, int last, float noise_std, unsigned long long seed,
                             unsigned long long round, unsigned stream_id, unsigned long long offset, void* stream);
/* fedfr_sparse_aggregate in the same way.  The noise is DENSE: every element of every tile receives it, not only the touched ones. */
int fedfr_sparse_aggregate_dp(float* dst, const float* base, const unsigned* const* idx, const float* const* val, const size_t* keeps,
                              const float* coef, int k, size_t n, int accumulate, int last, float noise_std, unsigned long long seed,
                              unsigned long long round, unsigned stream_id, unsigned long long offset, void* stream);

int fedfr_pfc_rand(float* perm, int n, unsigned long long seed, unsigned long long step, void* stream);
int fedfr_pfc_localize(long long* label, int n, long long class_start, int num_local, float* perm, void* stream);
int fedfr_pfc_topk(const float* perm, int n, int k, long long* index, int* npos_out, void* stream);
int fedfr_pfc_positive(const float* perm, int n, long long* index, int* count, void* stream);
int fedfr_pfc_remap(long long* label, int n, const long long* index, int k, void* stream);
/* dst[i] = table[index[i]] / table[index[i]] = src[i]; rows of D floats; indices outside [0, table_rows) are skipped */
int fedfr_rows_gather(float* dst, const float* table, const long long* index, int k, int D, int table_rows, void* stream);
int fedfr_rows_scatter(float* table, const float* src, const long long* index, int k, int D, int table_rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDFR_HIP_H */
