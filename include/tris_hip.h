/* tris_hip.h -- C ABI of libtris_hip.so: the MI355X (gfx950) kernels of the TRIS Stage-1 hot path.
 *
 * The reference (fawnliu/TRIS) has no native layer and no FFI: its hot path is PyTorch ops called from Python
 * (SURVEY.md 8b).  This header is therefore the boundary a maintainer binds *beneath* the reference's Python
 * call sites: each entry point below names the reference op (file:line under /root/reference) it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 (ids: int64) unless noted; no torch types, no hidden allocation:
 *     scratch is passed in (`workspace`, size from the matching *_workspace_bytes helper or documented inline);
 *   - activations are channels-last: an NHWC tensor is the row-major matrix [B*H*W, C];
 *   - conv weights are [Cout][kh][kw][Cin] (= torch.channels_last memory of the reference's [Cout,Cin,kh,kw]);
 *   - `stream` is a hipStream_t (0 = default stream); launches are asynchronous and re-entrant.  The ONLY state the
 *     library keeps is host-side configuration read at launch time: the arithmetic mode of the dense products (a
 *     process-wide default, tris_set_gemm_mode, plus a per-thread override, tris_set_gemm_mode_thread), the autotune
 *     switch with its per-process cache of tuned (tile, split-K) choices (tris_set_autotune), and the developer options of
 *     tris_set_option (read from the environment once, when the library is loaded).  No entry point keeps
 *     device state between calls (the SyncBN mailboxes of tris_mbox_* are caller-owned buffers);
 *   - return value: 0 on success, otherwise a hipError_t.
 */
#ifndef TRIS_HIP_H
#define TRIS_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dense products -------------------------------------------------------------------------------------------
 * C[b] = act(alpha * opA(A[b]) . opB(B[b]) + bias) + resid[b]        fp32 in / fp32 out; evaluated in the arithmetic mode
 *   in force for the launching thread (tris_set_gemm_mode below; default split-bf16 "x3", fp32-class accuracy)
 *   opA: transA=0 -> A[m*lda+k], 1 -> A[k*lda+m];  opB: transB=0 -> B[k*ldb+n], 1 -> B[n*ldb+k]
 *   bias_mode 1: bias[n], 2: bias[m];  act 0 none, 1 ReLU, 2 QuickGELU x*sigmoid(1.702x)
 *   workspace (optional, batch==1): enables split-K for small output grids; any size, used opportunistically.
 * Replaces nn.Linear / 1x1 nn.Conv2d / torch.bmm / matmul on the path: CLIP/clip/model.py:17,27,45 (1x1 convs),
 * :369-376 (MHA projections, MLP), :562 (text_projection); model/model_stage1.py:36-37,61-63,75; model/attn.py:73-109,
 * 118-128. */
int tris_gemm_f32(const float* A, const float* B, float* C, int M, int N, int K, long lda, long ldb, long ldc,
                  int transA, int transB, int batch, long strideA, long strideB, long strideC, const float* bias,
                  int bias_mode, const float* resid, long ldr, long strideR, int act, float alpha, float* workspace,
                  long workspace_bytes, void* stream);

/* One-shot: the NEXT tris_gemm_f32 launched from the calling thread (batch 1) also
 *   - stores the value BEFORE the activation to pre_out (layout of C) -- with act = 2 one launch yields QuickGELU(x W^T + b) and the
 *     pre-activation its backward needs (CLIP/clip/model.py:361-376, the transformer MLP);
 *   - multiplies what it stores by quickgelu'(dact_x[m, n]) (layout of C; applied last) -- the data gradient of the Linear behind a
 *     QuickGELU comes out as the gradient of the pre-activation.
 * Either pointer may be NULL.  The armed product runs without split-K and returns TRIS_DECLINED (nothing launched, arming consumed)
 * when the fast kernel does not serve its operands. */
int tris_gemm_epilogue_next(float* pre_out, const float* dact_x);

/* One-shot: the NEXT tris_gemm_f32 or tris_gemm_bnbwd_f32 launched from the calling thread (batch 1) takes its residual POOLED: the M
 * rows of C are the pixels of a [M / (H W), H, W] map and resid is [M / 4, ldr], the gradient of the 2x2 average pool of that map --
 * the epilogue adds 0.25f * resid[pooled pixel of m], the value tris_avgpool2_bwd_f32 would have written to a full-size tensor for it
 * to read back (the shortcut of a stride-2 Bottleneck, reference CLIP/clip/model.py:33-38; bit-identical to those two launches).
 * H and W even, M a multiple of H W, resid 16-byte aligned with ldr % 4 == 0: otherwise the armed product FAILS
 * (hipErrorInvalidValue).  It runs without split-K; where the fast kernel does not serve its operands tris_gemm_f32 returns
 * TRIS_DECLINED and tris_gemm_bnbwd_f32 reports *part_rows = 0 -- nothing launched, arming consumed. */
int tris_gemm_resid_pool_next(int H, int W);

/* One-shot: the NEXT tris_gemm_f32 launched from the calling thread may finish a split-K product INSIDE its own launch: each tile's
 * k slices take a ticket from tickets[tile], and the block that arrives last sums the tile's slabs in the order of the reduce launch it replaces (the result is
 * the separate reduce launch's, bit for bit, whichever block that is), applies bias / activation / residual and writes C.  Used for
 * up to 16 slices (developer option FUSE_SPLITK = n, 0 = never), one batch, the fast kernels.  `tickets`: `count` ints in device
 * memory, ZERO when handed over; every launch leaves them zero; private to the stream of the launch (two products in flight at
 * once must not share an array; a captured launch keeps reading the same array at every replay).  Without it, or with fewer ints
 * than the product has tiles, the slabs are summed by a second launch.  (The small products of the transformer towers and of the
 * late trunk stages -- reference CLIP/clip/model.py:366-397 -- are ~190 such pairs of launches per training step.) */
int tris_splitk_tickets_next(int* tickets, int count);
/* how many product launches of this process took the fused finish so far (tests, bench.py) */
long tris_splitk_fused_launches(void);

/* Arithmetic of the dense-product kernels.  tris_set_gemm_mode sets the process-wide DEFAULT; tris_set_gemm_mode_thread
 * sets an override for the calling thread only (-1 = none) -- e.g. the autograd thread running the weight-gradient
 * products in another mode -- so that concurrent launches from other threads are unaffected.  Both are host-side values
 * read when a product is launched; tris_get_gemm_mode returns the mode in force for the calling thread.  0 = v_mfma_f32_32x32x2_f32 (f32 in, bit-equal to an fmaf chain);
 * 1 = split-bf16 "x3": every fp32 operand is the exact sum of three bf16 pieces, the six significant piece products
 * run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation -> fp32-class accuracy (measured: error vs fp64 <= the f32-MFMA
 * path's) at up to 2.6x the f32-MFMA peak;  3 = "h2": two fp16 pieces per operand, three f16 MFMAs, power-of-two operand
 * scales (see tris_h2_next below; selected process-wide it runs with unit scales: tests).  Default: 1. */
int tris_set_gemm_mode(int mode);
int tris_set_gemm_mode_thread(int mode);
/* Developer options (tests, tools): name = FORCE_TILE (128x128|128x64|64x64|128x32|256x128), FORCE_PIPE (0|1), PIPE (0|1),
 * CONV_DIRECT (0 = implicit GEMM only, 1..6 = that direct configuration where it applies), WGRAD_DIRECT (0, 1..5), BN_FOLD (0|1),
 * STEM_CONV1 (0|1), WG_BLOCKS (n), STREAM_FORM (0|1: streaming form of the element-wise passes over more than the memory-side cache), COL_BLOCKS (n),
 * TUNE_LOG (file); a leading "TRIS_" is accepted; value NULL or "" restores the default.  Initial
 * values come from the environment variables TRIS_<name>, read once when the library is loaded -- nothing reads the environment
 * per call.  tris_set_conv_direct_thread: CONV_DIRECT for the products of the calling thread only (-1 = none): batch-invariant
 * evaluation pins the implicit 3x3 kernels this way. */
int tris_set_option(const char* name, const char* value);
int tris_set_conv_direct_thread(int value);

/* (tile, split-K) selection of the dense-product kernels: 1 (default; env TRIS_AUTOTUNE) = every admissible pair is timed
 * once per product shape on first use and the fastest is cached for the process; 0 = the static cycle model (deterministic
 * run-to-run rounding). */
int tris_set_autotune(int on);
/* the current switch (1 | 0), for callers that turn it off around a region and restore it */
int tris_get_autotune(void);
int tris_get_gemm_mode(void);
/* Diagnostics: launches so far of the direct 3x3 convolution kernels (kind 0: forward / data gradient) and of the direct 3x3
 * weight-gradient kernel (kind 1) -- the tests use it to prove which kernel ran.  Host-side counters, not thread-safe. */
long tris_direct_launches(int kind);

/* 3x3 convolution, pad 1, no im2col buffer.  CLIP/clip/model.py:21 (Bottleneck.conv2), :212-229 (stem).
 * fwd: stride 1 or 2.  dgrad: stride 1 only (the only strided conv on the path, the stem's conv1, reads the image and
 * needs no input gradient).  wgrad: split over output pixels; workspace >= 2 slabs of Cout*9*Cin floats, more = faster.
 * Each entry point picks, per shape (timed once like the GEMM tile choice; static table when autotuning is off), between
 * the implicit GEMM and a direct kernel that splits every input value once per window instead of once per tap (x3
 * arithmetic, stride 1, Cin % 16 == 0).  Same result up to fp32 summation order. */
int tris_conv3x3_fwd_f32(const float* X, const float* Wt, float* Y, int B, int H, int W, int Cin, int Cout, int stride,
                         void* stream);
int tris_conv3x3_dgrad_f32(const float* dY, const float* Wt, float* dX, int B, int H, int W, int Cin, int Cout,
                           void* stream);
int tris_conv3x3_wgrad_f32(const float* X, const float* dY, float* dW, int B, int H, int W, int Cin, int Cout,
                           int stride, float* workspace, long workspace_bytes, void* stream);

/* BatchNorm + ReLU folded into the consuming 3x3 convolution (CLIP/clip/model.py:45-46 `relu(bn1(conv1(x)))` -> conv2, and the
 * stem's conv -> bn -> relu -> conv chain :255-258): conv3x3(relu((X - mean) * invstd * gamma + beta)), stride 1, with the
 * normalised tensor formed inside the direct kernels' window staging (tris_bn_apply_f32's expression) -- it never exists in HBM.
 * tris_conv3x3_bnin_ok (host query, x3 arithmetic only) says whether direct kernels serve BOTH the forward product and the weight
 * gradient of the shape; when it returns 0 the caller materialises the BatchNorm output as usual.  fwd: stat_part / stat_rows
 * as in tris_conv3x3_fwd_bnstat_f32 (NULL: no statistics).  The data gradient is tris_conv3x3_dgrad_f32 (it does not read X). */
int tris_conv3x3_bnin_ok(int B, int H, int W, int Cin, int Cout);
int tris_conv3x3_fwd_bnin_f32(const float* X, const float* mean, const float* invstd, const float* gamma, const float* beta,
                              const float* Wt, float* Y, int B, int H, int W, int Cin, int Cout, double* stat_part,
                              int* stat_rows, void* stream);
int tris_conv3x3_wgrad_bnin_f32(const float* X, const float* mean, const float* invstd, const float* gamma, const float* beta,
                                const float* dY, float* dW, int B, int H, int W, int Cin, int Cout, float* workspace,
                                long workspace_bytes, void* stream);

/* Forward conv / 1x1 conv (A[M,K] . B[N,K]^T) with the train-mode BatchNorm statistics of the OUTPUT fused into the
 * epilogue: stat_part <- [rows][2][N] fp64 partial (sum, sum of squares), *stat_rows (HOST int) <- rows, or 0 when the
 * shape is not eligible (then call tris_bn_stats_f32).  stat_part capacity: ceil(M/128)*2*N doubles (rows <= ceil(M/128):
 * one per M tile of the kernel that ran).  Finish with
 * tris_bn_finalize_f32.  (CLIP/clip/model.py:17-29,45-48: conv -> bn pairs of Bottleneck / stem) */
int tris_gemm_bnstat_f32(const float* A, const float* B, float* C, int M, int N, int K, double* stat_part,
                         int* stat_rows, void* stream);
int tris_conv3x3_fwd_bnstat_f32(const float* X, const float* Wt, float* Y, int B, int H, int W, int Cin, int Cout,
                                int stride, double* stat_part, int* stat_rows, void* stream);
int tris_bn_finalize_f32(const double* part, int rows, long M, int C, float eps, float momentum, float* stats,
                         float* running_mean, float* running_var, void* stream);

/* ---- BatchNorm2d (training: batch statistics; CLIP/clip/model.py:18,22,28,39; train_stage1.py:288) ---------------------
 * stats = [mean | invstd | biased var], 3*C floats.  running_* may be NULL (no update).  workspace:
 * tris_col_workspace_bytes(M, C).  Eval mode = tris_bn_apply with mean=running_mean, invstd=rsqrt(running_var+eps). */
long tris_col_workspace_bytes(long M, int C);
int tris_bn_stats_f32(const float* X, long M, int C, float eps, float momentum, float* stats, float* running_mean,
                      float* running_var, float* workspace, void* stream);
/* SyncBatchNorm (train_stage1.py:69): gathered = [world][3*C] = every rank's `stats` block [mean | invstd | var] as written
 * by tris_bn_stats_f32 / tris_bn_finalize_f32 (all_gather it as is); each rank contributed count_per_rank rows. */
int tris_bn_sync_combine_f32(const float* gathered, int world, int C, long count_per_rank, float eps, float momentum,
                             float* stats, float* running_mean, float* running_var, void* stream);
/* Y = (X-mean)*invstd*gamma+beta (+resid) (ReLU) -- also the residual add + relu3 of Bottleneck.forward :52-54 */
int tris_bn_apply_f32(const float* X, const float* mean, const float* invstd, const float* gamma, const float* beta,
                      const float* resid, float* Y, long M, int C, int relu, void* stream);
/* backward: dz = dY * (Y > 0) when Y != NULL.  sum_dz = dbeta, sum_dzx = dgamma.  apply: dZ (optional) receives dz,
 * the gradient of the fused residual branch (Bottleneck identity path).  gamma_mask / beta_mask != NULL (BatchNorm + ReLU
 * without a residual input): the ReLU mask is recomputed from X with tris_bn_apply_f32's own expression -- same sign bit
 * for bit -- and Y is not read (one 4-byte stream less in each of the two passes).  reduce, dz_out != NULL: the masked
 * gradient dz is also written; tris_bn_bwd_apply_f32 may then be given dY = dz_out, Y = NULL, dZ = NULL (dz is already
 * the residual branch's gradient): 7 activation-sized streams over the two passes instead of 8.
 * Every entry point of this family (stats, apply, reduce, bwd_apply and the pool forms) returns hipErrorInvalidValue and launches
 * nothing when C % 4 != 0; the reduce also when exactly one of gamma_mask / beta_mask is given. */
/* The reduce pass fused into the PRODUCER of dY where that is a 1x1-convolution / Linear data gradient (the next layer's
 * backward, CLIP/clip/model.py:42-55 read in reverse): dZ[M,N] = mask(dY[M,K] . Wt[K,N] (+ resid)) with the mask of the
 * BatchNorm(+ReLU) whose raw input is bn_x [M,N] -- from its output bn_y (residual form), or, bn_y == NULL, recomputed from
 * bn_x / gamma / beta -- and part <- [rows][2][N] fp64 partial (sum dz, sum dz*xhat), *part_rows (HOST int) <- rows, or 0 when
 * the shape is not eligible (nothing launched: run tris_gemm_f32 + tris_bn_bwd_reduce_f32).  part capacity: ceil(M/128)*2*N
 * doubles.  Finish with tris_part_finalize_f32 -> sum_dz, sum_dzx, then tris_bn_bwd_apply_f32(dY = dZ, Y = NULL, dZ = NULL,
 * beta_mask = NULL).  One activation-sized read and one write less than the separate reduce pass. */
int tris_gemm_bnbwd_f32(const float* dY, const float* Wt, float* dZ, int M, int N, int K, const float* resid, long ldr,
                        const float* bn_x, const float* bn_y, const float* mean, const float* invstd, const float* gamma,
                        const float* beta, double* part, int* part_rows, void* stream);
/* the same for a 3x3 convolution's data gradient (stride 1, pad 1; bn1 -> conv2 of Bottleneck, the stem's bn1/bn2): the input
 * of the convolution is relu(bn(bn_x)), no residual, mask recomputed from bn_x. */
int tris_conv3x3_dgrad_bnbwd_f32(const float* dY, const float* Wt, float* dZ, int B, int H, int W, int Cin, int Cout,
                                 const float* bn_x, const float* mean, const float* invstd, const float* gamma,
                                 const float* beta, double* part, int* part_rows, void* stream);
int tris_part_finalize_f32(const double* part, int rows, int C, float* out0, float* out1, void* stream);

/* Arithmetic "h2" for single dense products: an operand x, multiplied by a power of two s that brings the
 * largest magnitude of its TENSOR (or an upper bound of it) to [2^13, 2^14), is held as two fp16 pieces, x s = hi + lo' 2^-11
 * (hi = fp16(x s), lo' = fp16((x s - hi) 2^11): 22 significand bits + sign); a product is three f16 MFMAs -- hi x hi into one fp32
 * accumulator, hi x lo' and lo' x hi into a second that joins with the weight 2^-11 in the epilogue -- half the matrix work of the
 * x3 default.  Because lo' is stored pre-scaled it stays a normal fp16 number as long as hi does: an element keeps all 22 bits
 * down to 2^-27 of the tensor's maximum; below that the error is absolute, <= 2^-49 of the maximum.  Error of a product:
 * fp32-class relative term + K amaxA amaxB 2^-49.
 * An amax word is 2048 unsigned words (8 KB: 8 XCDs x 16 cache lines with one used word each; the consumer takes the max).
 * tris_amax_bits_f32: atomic max of |x| as a bit pattern into that block (zero it first).  tris_h2_next: arms the CALLING THREAD -- the
 * next dense product it launches (tris_gemm_f32, tris_gemm_bnstat_f32, tris_gemm_bnbwd_f32, tris_conv3x3_{fwd,fwd_bnstat,dgrad,
 * dgrad_bnbwd,wgrad,fwd_bnin,wgrad_bnin}_f32) runs in h2 with operand A scaled from *amaxA (or, amaxA == NULL, by scaleA; 0 = 1.0)
 * and B likewise; products the fast kernels do not serve run as usual.  One shot: an arming never survives the call it was made for.
 * Operand order: forward / data gradient A = activation, B = weights; weight gradients A = dY, B = the convolution's input (for the
 * *_bnin forms: the bound word of tris_bn_out_bound_f32, since relu(bn(X)) is never materialised). */
int tris_amax_bits_f32(const float* x, long n, unsigned* out, void* stream);
/* the same for nseg tensors base + offs[i] (sizes[i] floats; device arrays) in one launch -> slots[i]: the weights of an arena */
int tris_amax_segments_f32(const float* base, const long* offs, const long* sizes, int nseg, unsigned* slots, void* stream);
/* one shot, calling thread: the next tris_bn_apply_f32 / tris_bn_apply_pool_f32 / tris_bn_bwd_apply_f32 /
 * tris_bn_bwd_apply_pool_f32 / tris_layernorm_fwd_f32 / tris_layernorm_bwd_f32 (dX) / tris_elementwise_f32 / tris_gemm_f32 (C) /
 * tris_mha_fwd_f32 / tris_mha_mfma_fwd_f32 (out) / tris_mha_bwd_f32 / tris_mha_mfma_bwd_f32 (dqkv) also maxes the magnitude bits of
 * what it WRITES into *out (zeroed by the caller): the amax of an h2 operand as a by-product of the pass that produces the tensor,
 * instead of a pass of its own.  Each of these entry points TAKES the arming first thing, whether or not it then launches anything. */
int tris_amax_next(unsigned* out);
int tris_h2_next(const unsigned* amaxA, const unsigned* amaxB, float scaleA, float scaleB);
/* Operand planes ("P8", csrc/planes.h; DESIGN.md "operand planes"): a tensor in the byte geometry of its fp32 original whose every 8
 * consecutive elements of the contiguous dimension are 16 bytes of fp16 hi pieces followed by 16 bytes of pre-scaled fp16 lo pieces,
 * x s = hi + lo' 2^-11 with the power-of-two scale s that *word implies (an amax word holding the tensor's largest magnitude or an
 * upper bound of it, final BEFORE the tensor is written).  tris_h2_planes_f32 / tris_h2_unplanes_f32 convert (n % 8 == 0);
 * tris_h2_planes_segments_f32 converts nseg tensors base + offs[i] (sizes[i] floats, word slots + 2048 slot_index[i]; device arrays)
 * of one flat buffer into out_base + offs[i] in one launch (the convolution weights of an optimiser arena, once per step).
 * tris_h2_next_planes arms the calling thread like tris_h2_next, for a product whose operands A and B are BOTH such plane tensors
 * (same pointers, shapes and leading dimensions as the fp32 form; contiguous dimensions multiples of 8): the kernels store the
 * pieces as they arrive instead of splitting fp32 values, and the result is bit-identical to the h2 product of the fp32 originals at
 * the same scales.  flags bit 0: the bn_y operand of tris_gemm_bnbwd_f32 is a plane tensor as well; bit 1: the weight operand of
 * tris_gemm_bnbwd_f32 is given TRANSPOSED ([N][K] = W^T, tris_h2_planes_t_segments_f32).  A product the fast kernels do not
 * serve FAILS (hipErrorInvalidValue): there is no fp32 operand to fall back on; the *_bnin forms refuse planes. */
/* Bit masks (round 6): tris_bn_mask_next(mask) arms the calling thread's NEXT tris_bn_apply_pl_f32 to write, beside its plane output
 * [M, C], the ReLU mask of that output as one BYTE per 8 channels (M C / 8 bytes; bit t <=> channel 8 g + t is positive, decided as a
 * reader of the planes would); tris_h2_next_planes flags bit 2 tells tris_gemm_bnbwd_f32 that its bn_y argument IS that byte array
 * (1 bit per element read in the fused BatchNorm-backward epilogue instead of the 4-byte plane element: model.py:42-55's
 * relu(bn3(..) + identity) outputs are the widest tensors of a Bottleneck). */
int tris_bn_mask_next(unsigned char* mask);
int tris_h2_planes_f32(const float* x, float* planes_out, long n, const unsigned* word, void* stream);
int tris_h2_planes_segments_f32(const float* base, const long* offs, const long* sizes, const long* slot_index, int nseg,
                                const unsigned* slots, float* out_base, void* stream);
/* the same for nseg row-major matrices [rows[i]][cols[i]] (multiples of 64), written TRANSPOSED: planes of W^T [cols][rows] -- the 1x1
 * convolution weights as the B^T operand of their data gradient */
int tris_h2_planes_t_segments_f32(const float* base, const long* offs, const long* rows, const long* cols, const long* slot_index,
                                  int nseg, const unsigned* slots, float* out_base, void* stream);
int tris_h2_unplanes_f32(const float* planes, float* out, long n, const unsigned* word, void* stream);
int tris_h2_next_planes(const unsigned* amaxA, const unsigned* amaxB, int flags);
/* The RN50 trunk's element-wise passes with plane OUTPUT (csrc/planes.hip; reference: CLIP/clip/model.py:42-55 Bottleneck.forward,
 * the BatchNorm2d / ReLU / AvgPool2d calls between its convolutions).  Same arithmetic as tris_bn_apply_f32 / tris_bn_apply_pool_f32 /
 * tris_avgpool2_fwd_f32 / tris_bn_bwd_apply_f32 / tris_bn_bwd_apply_pool_f32 on groups of 8 channels (C % 8 == 0); the result is split
 * with the scale of *out_word, which must hold an upper bound of the output's magnitude BEFORE the launch:
 *   tris_bn_out_bound2_f32: *out <- bits of max_c(|gamma[c]| xhat_max + |beta[c]|) + (add_word ? value of *add_word : 0) -- Samuelson's
 *     bound of a train-mode BatchNorm output (xhat_max = sqrt(rows - 1)) plus the bound of the residual it is added to;
 *   tris_bn_bwd_bound_f32: *out <- bits of max_c |gamma invstd| (amax_dz + |sum_dz| inv_count + xhat_max |sum_dzx| inv_count), the
 *     bound of dx = gamma invstd (dz - mean(dz) - xhat mean(dz xhat)); *dz_word: amax of the masked upstream gradient, left by the pass
 *     that reduced it (tris_amax_next before tris_bn_bwd_reduce_f32 / _pool_f32 / tris_gemm_bnbwd_f32 / tris_conv3x3_dgrad_bnbwd_f32).
 * resid_kind: 0 none, 1 fp32, 2 planes scaled by *resid_word.  Ypl of the backward: the BatchNorm's OUTPUT as planes (its ReLU mask is
 * "a piece is non-zero"), or NULL with beta_mask (mask recomputed from X) or without (no ReLU).  tris_avgpool2_fwd_pl_f32: planes in,
 * planes out at the SAME scale word (a mean never exceeds the bound of its terms). */
int tris_bn_apply_pl_f32(const float* X, const float* mean, const float* invstd, const float* gamma, const float* beta,
                         const float* resid, int resid_kind, const unsigned* resid_word, float* Ypl, const unsigned* out_word, long M,
                         int C, int relu, void* stream);
/* The closing pass of a down-sampling Bottleneck (reference CLIP/clip/model.py:42-55, out = relu(bn3(conv3) + downsample(x))) with the
 * shortcut's BatchNorm inside it: Ypl = relu(bn3(X3) + bn_s(Xs)), X3 and Xs [M, C] raw convolution outputs.  Bit-identical to
 * tris_bn_apply_f32(Xs, .._s, no residual, no ReLU) followed by tris_bn_apply_pl_f32(X3, .._3, that tensor as resid_kind 1, relu) at
 * the same *out_word -- the shortcut's fp32 output is never written or read back.  *out_word: an upper bound of the output, e.g. the sum
 * of the two Samuelson bounds (tris_bn_finalize_bound_f32 for the shortcut, then for bn3 with the shortcut's word as add_word).  Takes a
 * tris_bn_mask_next arming like tris_bn_apply_pl_f32.  Refused: C % 8, 2048 % C, a null or misaligned pointer. */
int tris_bn_apply_pair_pl_f32(const float* X3, const float* mean3, const float* invstd3, const float* gamma3, const float* beta3,
                              const float* Xs, const float* mean_s, const float* invstd_s, const float* gamma_s, const float* beta_s,
                              float* Ypl, const unsigned* out_word, long M, int C, void* stream);
int tris_bn_bwd_reduce_pl_f32(const float* dY, const float* Ypl, const float* X, const float* mean, const float* invstd, long M, int C,
                              float* sum_dz, float* sum_dzx, float* workspace, float* dz_out, void* stream);
int tris_bn_apply_pool_pl_f32(const float* X, const float* mean, const float* invstd, const float* gamma, const float* beta,
                              float* Ypl, const unsigned* out_word, int B, int H, int W, int C, void* stream);
int tris_avgpool2_fwd_pl_f32(const float* Xpl, float* Ypl, const unsigned* word, int B, int H, int W, int C, void* stream);
int tris_bn_bwd_apply_pl_f32(const float* dY, const float* Ypl, const float* X, const float* mean, const float* invstd,
                             const float* gamma, const float* sum_dz, const float* sum_dzx, float inv_count, float* dXpl,
                             const unsigned* out_word, float* dZ, long M, int C, const float* beta_mask, void* stream);
/* The backward of the pair above, where bn3's sums come out of the consuming product's epilogue (tris_gemm_bnbwd_f32):
 *   tris_gemm_bnbwd_x2_next arms the calling thread's NEXT tris_gemm_bnbwd_f32 with a SECOND BatchNorm that receives the same masked
 *     gradient dZ (the shortcut's): raw input x2 [M, N] (layout of dZ), its mean and invstd; the launch also leaves sum(dz * xhat2) per
 *     column in the first N doubles of each row of part2 [*part_rows][2][N] (the row layout of `part`), summed like the other two
 *     sums; dZ and `part` are the bits of the call without the arming.  Taken first thing; all pointers non-null and 16-byte aligned.
 *   tris_part_finalize_pair_f32: tris_part_finalize_bound_f32 for both BatchNorms in ONE launch -- sum_dz, sum_dzx from `part`,
 *     sum_dzx2 from part2, sum_dz a second time to sum_dz_b (the second BatchNorm's dbeta), and the bound words of the two dx (the
 *     expression of tris_bn_bwd_bound_f32 with the same *dz_word).
 *   tris_bn_bwd_apply_pair_pl_f32: dX3pl, dXspl (planes at *word3 / *word_s) from ONE read of dZ, X3 and Xs; for each of the two the
 *     arithmetic of tris_bn_bwd_apply_pl_f32 without a mask (dZ arrives masked) -- given the same sums, the same bits as two such
 *     launches.  Refused: C % 8, 2048 % C, a null or misaligned pointer, one word or one output for both. */
int tris_gemm_bnbwd_x2_next(const float* x2, const float* mean2, const float* invstd2, double* part2);
int tris_part_finalize_pair_f32(const double* part, const double* part2, int rows, int C, float* sum_dz, float* sum_dzx, float* sum_dz_b,
                                float* sum_dzx2, const float* gamma, const float* invstd, const float* gamma2, const float* invstd2,
                                float inv_count, float xhat_max, const unsigned* dz_word, unsigned* bound_out, unsigned* bound_out2,
                                void* stream);
int tris_bn_bwd_apply_pair_pl_f32(const float* dZ, const float* X3, const float* mean3, const float* invstd3, const float* gamma3,
                                  const float* sum_dzx3, const float* Xs, const float* mean_s, const float* invstd_s,
                                  const float* gamma_s, const float* sum_dzx_s, const float* sum_dz, float inv_count, float* dX3pl,
                                  const unsigned* word3, float* dXspl, const unsigned* word_s, long M, int C, void* stream);
int tris_bn_bwd_apply_pool_pl_f32(const float* dYp, const float* X, const float* mean, const float* invstd, const float* gamma,
                                  const float* beta, const float* sum_dz, const float* sum_dzx, float inv_count, float* dXpl,
                                  const unsigned* out_word, int B, int H, int W, int C, void* stream);
int tris_bn_out_bound2_f32(const float* gamma, const float* beta, int C, float xhat_max, const unsigned* add_word, unsigned* out,
                           void* stream);
/* tris_bn_finalize_f32 + tris_bn_out_bound2_f32, and tris_part_finalize_f32 + tris_bn_bwd_bound_f32, as ONE launch each (the bound is
 * atomically maxed into the zeroed word by the threads that finish the channels) */
int tris_bn_finalize_bound_f32(const double* part, int rows, long M, int C, float eps, float momentum, float* stats,
                               float* running_mean, float* running_var, const float* gamma, const float* beta, float xhat_max,
                               const unsigned* add_word, unsigned* bound_out, void* stream);
int tris_part_finalize_bound_f32(const double* part, int rows, int C, float* out0, float* out1, const float* gamma, const float* invstd,
                                 float inv_count, float xhat_max, const unsigned* dz_word, unsigned* bound_out, void* stream);
int tris_bn_bwd_bound_f32(const float* gamma, const float* invstd, const float* sum_dz, const float* sum_dzx, int C, float inv_count,
                          float xhat_max, const unsigned* dz_word, unsigned* out, void* stream);
/* *out (an amax word, zeroed by the caller) <- bits of max over c of |gamma[c]| * xhat_max + |beta[c]|: an upper bound of
 * |bn(x)| (and of relu(bn(x))) for a train-mode BatchNorm over `count` rows when xhat_max = sqrt(count - 1) (Samuelson's inequality:
 * no element lies further than sqrt(n - 1) standard deviations from the mean) */
int tris_bn_out_bound_f32(const float* gamma, const float* beta, int C, float xhat_max, unsigned* out, void* stream);
int tris_bn_bwd_reduce_f32(const float* dY, const float* Y, const float* X, const float* mean, const float* invstd,
                           long M, int C, float* sum_dz, float* sum_dzx, float* workspace, const float* gamma_mask,
                           const float* beta_mask, float* dz_out, void* stream);
int tris_bn_bwd_apply_f32(const float* dY, const float* Y, const float* X, const float* mean, const float* invstd,
                          const float* gamma, const float* sum_dz, const float* sum_dzx, float inv_count, float* dX,
                          float* dZ, long M, int C, const float* beta_mask, void* stream);
/* out[n] = sum_m X[m*ld+n]  (bias gradients).  workspace: tris_col_workspace_bytes(M, N) */
int tris_colsum_f32(const float* X, long M, int N, long ld, float* out, float* workspace, void* stream);

/* ---- InstanceNorm2d(affine) [+ReLU] on [B, P, C]  (model/attn.py:75,80,85,106) ----------------------------------------
 * (both honour tris_amax_next: the amax word of Y / dX as a by-product)
 * Biased two-pass variance over the P pixels of a (b, c); the forward stores the mean and invstd = rsqrt(var + eps) it used.  The
 * backward's ReLU mask is Y > 0 of the saved output; dgamma_part / dbeta_part are the sums of one image, summed over b by the caller.
 * Contract (hipErrorInvalidValue before any launch otherwise): B, P, C >= 1 (any C, any P); forward: X, gamma, beta, Y, mean, invstd
 * non-NULL; backward: dY, X, gamma, mean, invstd, dX, dgamma_part, dbeta_part non-NULL, and Y non-NULL when relu != 0. */
int tris_instnorm_fwd_f32(const float* X, const float* gamma, const float* beta, float* Y, float* mean, float* invstd,
                          int B, int P, int C, float eps, int relu, void* stream);
int tris_instnorm_bwd_f32(const float* dY, const float* Y, const float* X, const float* gamma, const float* mean,
                          const float* invstd, float* dX, float* dgamma_part /*[B,C]*/, float* dbeta_part /*[B,C]*/,
                          int B, int P, int C, int relu, void* stream);

/* ---- LayerNorm over the last dim W <= 1024  (CLIP/clip/model.py:352-358) ------------------------------------------------
 * Biased two-pass variance; the forward stores the mean and rstd = rsqrt(var + eps) it used (both, or neither: mean = rstd = NULL).
 * The backward writes dX = rstd (dy g - c1 - xhat c2) [+ extra], dgamma = sum_rows dy xhat, dbeta = sum_rows dy; dX == NULL or
 * dgamma == dbeta == NULL leaves that part out.  Both honour tris_amax_next (Y / dX), the forward tris_rows_limit_thread.
 * Contract (hipErrorInvalidValue before any launch otherwise): rows >= 1, 4 <= W <= 1024, W % 4 == 0; forward: X, gamma, beta, Y
 * non-NULL, mean and rstd both NULL or both non-NULL; backward: dY, X, gamma, mean, rstd non-NULL, dgamma and dbeta both NULL or
 * both non-NULL, workspace (tris_layernorm_bwd_workspace_bytes) non-NULL when dgamma is, and not dX == NULL with dgamma == NULL. */
int tris_layernorm_fwd_f32(const float* X, const float* gamma, const float* beta, float* Y, float* mean, float* rstd,
                           long rows, int W, float eps, void* stream);
long tris_layernorm_bwd_workspace_bytes(long rows, int W);
int tris_layernorm_bwd_f32(const float* dY, const float* X, const float* gamma, const float* mean, const float* rstd,
                           float* dX, float* dgamma, float* dbeta, long rows, int W, float* workspace, const float* extra /* optional: added to dX */, void* stream);

/* ---- pooling / elementwise / layout -------------------------------------------------------------------------------- */
/* BatchNorm + ReLU + AvgPool2d(2) as ONE op (the stem's bn3 -> avgpool, model.py:29-31,231-237; bn2 -> avgpool of the stride-2
 * Bottlenecks, :21-25,46-49): Yp [B,H/2,W/2,C] = avgpool2(relu(bn(X))) -- the full-size activation is never written; backward:
 * the two passes read the POOLED upstream gradient dYp (a row's gradient is a quarter of its pooled pixel's), the ReLU mask is
 * recomputed from X.  H and W even. */
int tris_bn_apply_pool_f32(const float* X, const float* mean, const float* invstd, const float* gamma, const float* beta,
                           float* Yp, int B, int H, int W, int C, void* stream);
int tris_bn_bwd_reduce_pool_f32(const float* dYp, const float* X, const float* mean, const float* invstd, int B, int H, int W,
                                int C, float* sum_dz, float* sum_dzx, float* workspace, const float* gamma, const float* beta,
                                void* stream);
int tris_bn_bwd_apply_pool_f32(const float* dYp, const float* X, const float* mean, const float* invstd, const float* gamma,
                               const float* beta, const float* sum_dz, const float* sum_dzx, float inv_count, float* dX, int B,
                               int H, int W, int C, void* stream);
int tris_avgpool2_fwd_f32(const float* X, float* Y, int B, int H, int W, int C, void* stream); /* model.py:25,37,231 */
int tris_avgpool2_bwd_f32(const float* dY, float* dX, int B, int H, int W, int C, void* stream);
#define TRIS_EW_ADD 0       /* O = A + B */
#define TRIS_EW_AXPY 1      /* O = s*A + B          (model_stage1.py:73-74, the 0.1 residual mix) */
#define TRIS_EW_RELU_BWD 2  /* O = A * (B > 0)      A = dY, B = Y */
#define TRIS_EW_QGELU 3     /* O = A*sigmoid(1.702A) (CLIP/clip/model.py:361-363) */
#define TRIS_EW_QGELU_BWD 4 /* O = A * d/dB quickgelu(B) */
#define TRIS_EW_MUL 5       /* O = A * B */
#define TRIS_EW_SCALE 6     /* O = s * A */
#define TRIS_EW_RELU 7      /* O = max(A, 0) */
int tris_elementwise_f32(int op, const float* A, const float* B, float* O, long n, float s, void* stream);
/* the same with B broadcast: B has nb elements and is read modulo nb (A, O: [n / nb, nb]; n % nb == 0, nb % 4 == 0).
 * model_stage1.py:74: the sentence features of the step against every image's attended ones (0.1 * new_lan + norm_lan) */
int tris_elementwise_bcast_f32(int op, const float* A, const float* B, float* O, long n, long nb, float s, void* stream);
/* O = X * exp(ls[0]), e_out[0] = exp(ls[0])  (model_stage1.py:77-78: score * logit_scale.exp(), ls a device scalar).
 * bwd: dX = dO * exp(ls[0]) (dX may be NULL), dls[0] = sum(dO * O) (written; deterministic two-stage sum);
 * workspace: tris_scale_exp_workspace_bytes() */
int tris_scale_exp_fwd_f32(const float* X, const float* ls, float* O, float* e_out, long n, void* stream);
long tris_scale_exp_workspace_bytes(void);
int tris_scale_exp_bwd_f32(const float* dO, const float* O, const float* ls, float* dX, float* dls, float* workspace, long n,
                           void* stream);
int tris_nchw_to_nhwc_f32(const float* X, float* Y, int B, int C, int H, int W, void* stream);

/* ---- text / ViT transformer pieces --------------------------------------------------------------------------------- */
/* nn.MultiheadAttention core on packed QKV [N, L, 3W] -> [N, L, W]; head dim 64, L <= 64; causal = the additive
 * upper-triangular -inf mask of CLIP/clip/model.py:537-543.  (model.py:380-382) */
int tris_mha_fwd_f32(const float* qkv, float* out, int N, int L, int W, int heads, int causal, void* stream);
int tris_mha_bwd_f32(const float* qkv, const float* dout, float* dqkv, int N, int L, int W, int heads, int causal,
                     void* stream);
/* The same attention for ANY sequence length, flash-style on the f32 MFMA (no L x L matrix in memory): used for L > 64
 * (a ViT-B/16 trunk at 320 px has L = 401) and, where faster, for the short sequences too.  lse [N, heads, L] receives
 * the per-query log-sum-exp (saved for backward); delta [N, heads, L] is backward scratch (rowsum(dO * O)).  qkv -- and in the
 * backward out and dout -- are read with 16-byte loads: a pointer off that alignment is hipErrorInvalidValue, nothing is launched. */
int tris_mha_mfma_fwd_f32(const float* qkv, float* out, float* lse, int N, int L, int W, int heads, int causal,
                          void* stream);
int tris_mha_mfma_bwd_f32(const float* qkv, const float* out, const float* dout, const float* lse, float* delta,
                          float* dqkv, int N, int L, int W, int heads, int causal, void* stream);
/* The same flash-style attention in the h2 arithmetic on the 16-bit MFMA (csrc/attn_h2.hip): every product on two fp16 pieces per
 * operand (three v_mfma_f32_16x16x32_f16), one power-of-two scale per tensor from the amax words of the packed qkv and of dout
 * (2048 unsigned each, as tris_h2_next), 2^13 for the probabilities, the wave's block maximum for dS.  Same arguments, saved
 * log-sum-exp, delta and amax by-products (tris_amax_next) as the f32-MFMA entry points above. */
int tris_mha_h2_fwd_f32(const float* qkv, float* out, float* lse, const unsigned* amax_qkv, int N, int L, int W, int heads,
                        int causal, void* stream);
int tris_mha_h2_bwd_f32(const float* qkv, const float* out, const float* dout, const float* lse, float* delta, float* dqkv,
                        const unsigned* amax_qkv, const unsigned* amax_dout, int N, int L, int W, int heads, int causal,
                        void* stream);
/* Packed text rows (round 6).  A causal text tower is read at the EOT row of every sentence (reference CLIP/clip/model.py:552-564: the row at
 * argmax(ids)); under the causal mask (:537-543) no position behind it can reach that row, so the packed pass keeps rows 0 .. eot_n of
 * sentence n back to back and drops the rest (42 % of a RefCOCOg-shaped batch).  Extents live in DEVICE memory -- a captured pass is
 * valid for any ids.  Every packed buffer has R = N L rounded up to 256 rows.  plan (3 + N + R ints) <- tris_text_pack_plan_i64: [0] rows
 * in use P, [1] P rounded up to 256 = the row limit (<= R), [2 + n] first row of sentence n (n = 0 .. N), then the source token of
 * every packed row (-1 behind P).
 * tris_embed_packed_fwd_f32 writes rows < plan[1] of out [R, W] (zeros for P .. plan[1] - 1); tris_mha_packed_fwd_f32 is
 * tris_mha_fwd_f32 over the sentences' row ranges of the packed qkv [R, 3 W] (L <= 64; it keeps rows P .. plan[1] - 1 of out zero);
 * tris_eot_gather_packed_f32 reads each sentence's last row.  tris_rows_limit_thread(limit) makes the calling thread's following
 * tris_gemm_f32 (row-major A, one batch) and tris_layernorm_fwd_f32 launches skip rows >= *limit (a device word, normally &plan[1];
 * a multiple of 256 so that tiles are whole or absent); NULL clears it.  Forward only (the frozen aux tower). */
int tris_text_pack_plan_i64(const long* ids, int N, int L, int* plan, void* stream);
int tris_embed_packed_fwd_f32(const long* ids, const float* tok, const float* pos, const int* plan, float* out, int N, int L, int W,
                              void* stream);
int tris_mha_packed_fwd_f32(const float* qkv, float* out, const int* plan, int N, int Lmax, int W, int heads, int causal, void* stream);
int tris_eot_gather_packed_f32(const float* x, const int* plan, float* out, int N, int W, void* stream);
int tris_rows_limit_thread(const int* limit);
/* token_embedding(ids) + positional_embedding[:L]  (model.py:553-554).  bwd: dtok must be zero-filled by the caller */
int tris_embed_fwd_f32(const long* ids, const float* tok, const float* pos, float* out, int N, int L, int W,
                       void* stream);
int tris_embed_bwd_f32(const long* ids, const float* dout, float* dtok, float* dpos, int N, int L, int W, void* stream);
/* token-embedding gradient from a row list, deterministic (fixed summation order, no atomics): dtok[ids[t]] = scale * sum of
 * rows[t'] over the positions t' with ids[t'] == ids[t]; dtok zero-filled by the caller.  The list is this rank's N*L positions
 * (then tris_embed_bwd_f32 is called with dtok = NULL for the positional part) or, data-parallel, the all-gathered lists of every
 * rank with scale = 1 / world: <= world * B * L rows of W floats travel instead of the dense [vocab, W] table (101 MB at
 * 49408 x 512; reference: DistributedDataParallel all-reduces it densely, train_stage1.py:70). */
int tris_embed_rows_bwd_f32(const long* ids, const float* rows, float* dtok, int R, int W, float scale, void* stream);
/* out = [a; b]: int64 rows of two lists in one (positive + negative queries of a step, train_stage1.py:342-347: batched here) */
int tris_concat_i64(const long* a, long na, const long* b, long nb, long* out, void* stream);
/* x[arange(N), ids.argmax(-1)]  (model.py:562); ids NULL: x[:, 0] -- the ViT class token (model.py:443) */
int tris_eot_gather_fwd_f32(const long* ids, const float* x, float* out, int N, int L, int W, void* stream);
int tris_eot_gather_bwd_f32(const long* ids, const float* dout, float* dx, int N, int L, int W, void* stream);

/* ---- Stage-1 heads ------------------------------------------------------------------------------------------------- */
/* x / x.norm(dim=-1)  (model_stage1.py:68-69; train_stage1.py:268-269).  No eps, as the reference has none: the domain is rows
 * whose sum of squares neither underflows nor overflows float32 (row norms between 2^-40 and 2^40 are inside it; a zero row gives
 * inv_norm = inf and NaNs).  Backward from the saved Y and inv_norm: dX = (dY - Y sum(Y dY)) inv_norm.
 * Contract (hipErrorInvalidValue before any launch otherwise): rows >= 1, C >= 1, every pointer non-NULL. */
int tris_l2norm_fwd_f32(const float* X, float* Y, float* inv_norm, long rows, int C, void* stream);
int tris_l2norm_bwd_f32(const float* dY, const float* Y, const float* inv_norm, float* dX, long rows, int C,
                        void* stream);
/* softmax(scale * x) over rows of length n  (model/attn.py:119,122); the maximum is taken of the SCALED logits (any sign of scale).
 * Backward from the saved Y: dX = scale Y (dY - sum(Y dY)).
 * Contract (hipErrorInvalidValue before any launch otherwise): rows >= 1, n >= 1, every pointer non-NULL, scale finite. */
int tris_softmax_fwd_f32(const float* X, float* Y, long rows, int n, float scale, void* stream);
int tris_softmax_bwd_f32(const float* dY, const float* Y, float* dX, long rows, int n, float scale, void* stream);
/* Fused image<->text cross attention of bilateral_prompt (model/attn.py:117-128), all images in two (x3 arithmetic) or
 * three (f32 arithmetic) launches.
 * Qv,Kv,Vv [B,P,C] (pixels, channels-last), Qt,Kt,Vt [N,C] (sentences, one set shared by every image -- the reference
 * repeats it, model_stage1.py:66), scale = 1/sqrt(C); N <= 64, C % 64 == 0.
 *   new_vis[b] = softmax_n(Qv[b].Kt^T*scale).Vt      [B,P,C]
 *   new_lan[b] = softmax_p(Qt.Kv[b]^T*scale).Vv[b]   [B,N,C]
 * probs [B,4,P,N] (scratch + saved for backward): plane 0 = Av, plane 1 = Kv.Qt^T logits, plane 2 = AtT (pixel-major),
 * plane 3 = Qv.Kt^T logits (x3 path only). */
int tris_xattn_fwd_f32(const float* Qv, const float* Kv, const float* Vv, const float* Qt, const float* Kt,
                       const float* Vt, float* new_vis, float* new_lan, float* probs, int B, int P, int N, int C,
                       void* stream);
/* The same forward as ONE persistent launch (csrc/xattn_fused.hip; split-bf16 arithmetic, C = 512 | 1024, 8 <= P <= 104,
 * N <= 64): eight workgroups per image, the pixel-softmax coupling resolved by an in-kernel exchange of the logit blocks
 * (write-through stores + per-(image, slot) flags, bounded spins; all B * 8 workgroups must be co-resident, otherwise the call
 * declines).  The sentence operands are pre-split once per call into bf16 planes in MFMA
 * fragment order by a small preparation launch on the same stream.  probs: planes 0 (Av) and 2 (AtT) are written, 1 and 3 are
 * not touched.  ws: scratch of tris_xattn_fused_ws_bytes(B, N, C) bytes (0 = shape not supported); sync: caller-owned device
 * words (tris_xattn_fused_sync_words(B) of them), ZEROED once at allocation and then only passed back -- word 0 counts the
 * completed launches (the epoch that tags the exchange flags lives on the device, so a captured launch replays correctly),
 * word 2 != 0 after a launch means a wait timed out (outputs undefined).  One sync buffer per stream that may run the kernel.
 * Returns TRIS_DECLINED (-2) without launching anything when the shape / arithmetic mode is outside its domain. */
#define TRIS_DECLINED (-2)
long tris_xattn_fused_ws_bytes(int B, int N, int C);
long tris_xattn_fused_sync_words(int B);
int tris_xattn_fused_fwd_f32(const float* Qv, const float* Kv, const float* Vv, const float* Qt, const float* Kt,
                             const float* Vt, float* new_vis, float* new_lan, float* probs, int B, int P, int N, int C,
                             float* ws, long ws_bytes, unsigned* sync, void* stream);
/* The same forward as ONE persistent launch cut by PIXEL ROWS (csrc/xattn_px.hip; split-bf16 arithmetic, C = 512 | 1024,
 * P <= 104, N <= 64): S workgroups of 512 threads per image (S = min(8, CUs / B), one workgroup per CU), workgroup s owns pixels
 * [s P / S, (s + 1) P / S).  The pixel -> sentence direction (model/attn.py:118-119, 124) never leaves the workgroup; the
 * sentence -> pixel direction (attn.py:121-122, 127) needs ONE in-kernel hand-off of N x own-pixels logits, hidden behind the
 * former, and is then finished per 32-channel unit.  Same arguments, scratch / sync conventions, probs planes (0 and 2) and
 * TRIS_DECLINED behaviour as tris_xattn_fused_fwd_f32; the sync words may be the same buffer. */
long tris_xattn_px_ws_bytes(int B, int N, int C);
long tris_xattn_px_sync_words(int B);
/* h2 arithmetic for ONE call of the pixel-row launch: arms the calling thread with the amax words (2048 unsigned each, as
 * tris_h2_next) of Qv, Kv, Vv, Qt, Kt, Vt; the next tris_xattn_px_fwd_f32 of the thread computes its four products on two fp16
 * pieces per operand (three MFMAs per product, two sentence planes instead of three) with one power-of-two scale per tensor, the
 * probabilities with the fixed scale 2^13, and disarms.  Unarmed calls run the split-bf16 form. */
/* Backward of the pair on the saved probabilities, cut by pixel rows like the forward (csrc/xattn_px.hip): ONE persistent launch
 * (+ one preparation launch that splits the sentence-side operands into piece planes) produces dQv, dKv, dVv [B, P, C] and leaves
 * dS [3][B, P, N] = (dS1 = soft-max backward of the pixel -> sentence direction, dS2 = of the sentence -> pixel direction, a copy of
 * Av) for the three [N, C] gradients that sum over images and pixels (dVt = Av^T d_vis, dKt = dS1^T Qv, dQt = dS2^T Kv: split-K
 * products of the GEMM core).  probs is the forward's [B][4][P][N] buffer (planes 0 and 2).  Only the column sums of the
 * sentence -> pixel soft-max cross workgroups (N floats each, the forward's sync words and protocol).  Domain, TRIS_DECLINED and
 * the h2 arming (tris_xattn_amax_next with the words of d_vis, Vv, d_lan, Qt, Kt, Vt -- in that order) as for the forward.
 * Replaces the chain of six batched products and two soft-max backward launches of rounds 1-4 (reference model/attn.py:117-128). */
long tris_xattn_px_bwd_ws_bytes(int B, int N, int C);
int tris_xattn_px_bwd_f32(const float* d_vis, const float* d_lan, const float* Vv, const float* Qt, const float* Kt,
                          const float* Vt, const float* probs, float* dQv, float* dKv, float* dVv, float* dS, int B, int P,
                          int N, int C, float* ws, long ws_bytes, unsigned* sync, unsigned* amax_dQv, unsigned* amax_dKv,
                          unsigned* amax_dVv, void* stream);   /* amax_*: NULL or zeroed amax words the launch raises for its outputs */
long tris_xattn_px_last_form(void);   /* arithmetic of the last pixel-row launch: 0 none yet, 1 split-bf16, 2 h2 */
int tris_xattn_amax_next(const unsigned* qv, const unsigned* kv, const unsigned* vv, const unsigned* qt, const unsigned* kt,
                         const unsigned* vt);
/* host-side plan of the pixel-row launch: workgroups per image S on a device of `cus` compute units (0 = the call would decline:
 * B * S workgroups must be resident one per CU, a workgroup owns <= 32 pixels and <= 8 of the C / 32 channel units).  Workgroup s
 * owns pixels [s P / S, (s + 1) P / S) and units [s U / S, (s + 1) U / S), U = C / 32 (integer division). */
long tris_xattn_px_slots(int B, int P, int C, int cus);
int tris_xattn_px_fwd_f32(const float* Qv, const float* Kv, const float* Vv, const float* Qt, const float* Kt,
                          const float* Vt, float* new_vis, float* new_lan, float* probs, int B, int P, int N, int C,
                          float* ws, long ws_bytes, unsigned* sync, void* stream);
/* backward of a softmax taken over the P axis of [B,P,N]: dX = scale*Y*(dY - sum_p Y*dY)  (model/attn.py:122) */
int tris_softmax_col_bwd_f32(const float* dY, const float* Y, float* dX, int B, int P, int N, float scale,
                             void* stream);
/* training cls head on score [B,P,N]: bg channel + channel softmax + mean/max pooling + focal term
 * (model_stage1.py:80-108, focal_loss :122-123).  cls_fg may be NULL.  B, P, N >= 1; with cls_fg (the mean probability of
 * sentence i in image i) N >= B.  One workgroup per image holds its logits in LDS: (P*(N+1) + 2P) floats forward,
 * (P*(N+1) + 3P + 3N) backward, at most 150 KB.  Anything else returns hipErrorInvalidValue before a launch. */
int tris_cls_head_fwd_f32(const float* score, float* cls_out, float* cls_fg, int B, int P, int N, float focal_p,
                          float focal_c, void* stream);
int tris_cls_head_bwd_f32(const float* score, const float* g_cls_out, float* dscore, int B, int P, int N, float focal_p,
                          float focal_c, void* stream);
/* diagonal response maps score[i,:,i] -> bilinear (align_corners=False) to SxS -> relu / sigmoid
 * (model_stage1.py:110-119, model/utils.py:5-10).  sig_map may be NULL (eval).  bwd ACCUMULATES into dscore.
 * B, h, w, S >= 1, h*w <= 1024 and N >= B (image i reads column i), else hipErrorInvalidValue. */
int tris_maps_fwd_f32(const float* score, float* relu_map, float* sig_map, int B, int h, int w, int N, int S,
                      void* stream);
int tris_maps_bwd_f32(const float* score, const float* d_relu, const float* d_sig, float* dscore, int B, int h, int w,
                      int N, int S, void* stream);
/* F.interpolate(mode='bilinear') on [planes, Hi, Wi] (train_stage1.py:328-329, validate.py:180).  Up- and down-scale, both
 * align_corners conventions; planes and all four sizes >= 1, else hipErrorInvalidValue. */
int tris_resize_bilinear_fwd_f32(const float* X, float* Y, int planes, int Hi, int Wi, int Ho, int Wo,
                                 int align_corners, void* stream);
int tris_resize_bilinear_bwd_f32(const float* dY, float* dX, int planes, int Hi, int Wi, int Ho, int Wo,
                                 int align_corners, void* stream);
/* fg = cam * img written directly as the aux ViT's patch-GEMM operand [B, (R/ps)^2, C*ps*ps]
 * (train_stage1.py:333-338 + CLIP/clip/model.py:405,420-422).  cam [B,1,R,R], img [B,C,R,R]: square images of whole patches,
 * B, C, R, ps >= 1 and R % ps == 0, else hipErrorInvalidValue. */
int tris_fg_patch_fwd_f32(const float* cam, const float* img, float* patches, int B, int C, int R, int ps,
                          void* stream);
int tris_fg_patch_bwd_f32(const float* dpatches, const float* img, float* dcam, int B, int C, int R, int ps,
                          void* stream);
/* class token + positional embedding (CLIP/clip/model.py:423-424): emb [B,T-1,W] -> x [B,T,W].  B, W >= 1 and T >= 2 (the
 * class token and at least one patch), else hipErrorInvalidValue. */
int tris_vit_assemble_fwd_f32(const float* emb, const float* cls, const float* pos, float* x, int B, int T, int W,
                              void* stream);
int tris_vit_assemble_bwd_f32(const float* dx, float* demb, int B, int T, int W, void* stream);
/* The whole loss block: fg_loss = MaxLoss(clip_forward) (train_stage1.py:263-284,340), cbs_loss (:342-353),
 * cls_loss = multilabel_soft_margin_loss(cls, eye) (:354), loss = w1*l1 + w4*l4 + w5*l5 (:364).
 * per_img: scratch [B,3]; rowloss: scratch [B]; losses[4] = {total, l1, l4, l5}.  fneg may be NULL when K == 0.
 * bwd: g = device gradient of losses[4]; the kernels form dL/dl1 = g[0]*w1 + g[1], dL/dl4 = g[0]*w4 + g[2], dL/dl5 = g[0]*w5 + g[3]. */
int tris_stage1_loss_fwd_f32(const float* cls, const float* fi, const float* ft, const float* fneg, int B, int N, int E,
                             int K, float w1, float w4, float w5, float* per_img, float* rowloss, float* losses,
                             void* stream);
int tris_stage1_loss_bwd_f32(const float* cls, const float* fi, const float* ft, const float* fneg, const float* g,
                             float w1, float w4, float w5, int B, int N, int E, int K, float* dcls, float* dfi, void* stream);

/* ---- optimiser ----------------------------------------------------------------------------------------------------- */
/* torch.optim.AdamW step over a flat arena (train_stage1.py:135-139, 370); step_count is the 1-based t */
int tris_adamw_f32(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int step_count, void* stream);
/* the same update with the step-dependent scalars in DEVICE memory: hyper = {lr, 1 - beta1^t, sqrt(1 - beta2^t)} (written by
   the host before the launch) -- the form a captured training step replays (tris_amd/graphs.py GraphedTrainStep) */
int tris_adamw_dev_f32(float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2,
                       float eps, float weight_decay, void* stream);

/* ---- evaluation post-processing (validate.py:180-190, utils/util.py:9-15) ------------------------------------------- */
/* relu_map [S,S] of ONE (image, sentence) -> cam [oH,oW] = bilinear(align_corners=True)/(max+1e-5); mask = cam > 1e-9;
 * out_iu (int64[3], device) = {I, U, argmax index of cam}; target: uint8 [oH,oW].  cam may be NULL. */
int tris_eval_post_f32(const float* relu_map, int S, const unsigned char* target, int oH, int oW, float* cam,
                       long* out_iu, float* workspace /* >= 2*1024+8 floats */, void* stream);

/* ---- input pipeline (dataset/transform.py:23-63, dataset/ReferDataset.py:125-252) ---------------------
 * The decoded dataset is kept in HBM as uint8; everything below is bit-exact against Pillow / torchvision semantics. */
/* Pillow's antialiased two-pass resampling of an 8-bit image [Hin][Win][C] -> [Hout][Wout][C] (F.resize on a PIL image,
 * dataset/transform.py:29).  bounds_* int32[out][2] = {first source index, tap count}, kk_* int32[out][ksize] taps in
 * 22-bit fixed point (built on the host exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc do); a NULL
 * bounds pointer skips that pass (size unchanged along it).  tmp: Hin*Wout*C bytes when both passes run. */
int tris_resample_u8(const unsigned char* in, int Hin, int Win, int C, const int* bounds_h, const int* kk_h, int ksize_h,
                     const int* bounds_v, const int* kk_v, int ksize_v, int Hout, int Wout, unsigned char* tmp,
                     unsigned char* out, void* stream);
/* Pillow NEAREST resize (dataset/transform.py:32, ReferDataset.py:187): out[y][x] = in[yidx[y]][xidx[x]] (index < 0 -> 0) */
int tris_gather2d_u8(const unsigned char* in, int Hin, int Win, int C, const int* yidx, const int* xidx, int Hout,
                     int Wout, unsigned char* out, void* stream);
/* Stage-2 pseudo target (dataset/ReferDataset.py:178-186: `(mask*1.0).sum(0)` as an 'F' image, resized with Image.NEAREST):
 * masks uint8 [K][Hin][Win] of 0/1 -> out[y][x] = sum_k masks[k][yidx[y]][xidx[x]] as uint8 [Hout][Wout] (index < 0 -> 0),
 * with the index tables of tris_gather2d_u8.  0 <= K <= 255; K = 0 writes zeros (masks may then be NULL). */
int tris_mask_sum_nearest_u8(const unsigned char* masks, int K, int Hin, int Win, const int* yidx, const int* xidx,
                             int Hout, int Wout, unsigned char* out, void* stream);
/* batch assembly: out[b] = lut[c][cache[index[b]][p][c]]  (to_tensor + normalize, dataset/transform.py:41-53, with the
 * 3x256 float table computed by the host with the reference's float ops).  cache: uint8 [N][HW][3]; index: int64[B];
 * out: fp32 [B][HW][3] (planar=0, channels-last) or [B][3][HW] (planar=1, the reference's NCHW).  HW % 4 == 0. */
int tris_u8_gather_normalize_f32(const unsigned char* cache, const long* index, int B, long HW, const float* lut,
                                 float* out, int planar, void* stream);
/* out[r] = table[index[r]]  for rows of row_bytes (multiple of 4) bytes: token ids of the sampled sentences
 * (ReferDataset.py:172-229) */
int tris_gather_rows(const void* table, const long* index, long rows, long row_bytes, void* out, void* stream);

/* ---- SyncBatchNorm statistics exchange over xGMI peer memory (csrc/comm.hip) --------------------------------------
 * Replaces the per-layer collectives of nn.SyncBatchNorm (reference: train_stage1.py:69 convert_sync_batchnorm; torch's
 * SyncBatchNorm all_gathers [mean|invstd|count] in forward and all_reduces [sum_dy|sum_dy_xmu] in backward) for ranks on
 * ONE node.  Every rank owns a mailbox in uncached device memory (tris_mbox_alloc; capacity `cap_floats` per sender block,
 * a multiple of 4) and maps its peers' mailboxes through HIP IPC (tris_mbox_ipc_handle -> 64-byte handle, exchanged by the
 * host; tris_mbox_ipc_open).  tris_mbox_exchange_f32 is one single-workgroup launch on `stream`: store the block
 * [src0[n0] | src1[n1]] (n = n0 + n1; src1 may be NULL with n1 = 0) into every
 * peer's mailbox, publish per-sender flags (system-scope release), wait for the `world` flags of the own mailbox (bounded
 * spin: after spin_limit polls *err is set to seq, the wait is abandoned and `out` is filled with NaN instead of stale slot
 * contents -- tris_mbox_bn_combine_f32 likewise writes NaN statistics and leaves the running statistics alone), then mode 0:
 * out[world][n] = the gathered
 * blocks in rank order; mode 1: out[n] = their sum in rank order (bit-identical on every rank).  `boxes` is a DEVICE array of
 * the `world` mailbox pointers as mapped in this process (own mailbox at index `rank`).  `seq` points at ONE caller-owned DEVICE
 * word, zeroed once: the number of the exchange is read from it and advanced in it by the kernel itself (exchanges of a rank run
 * on one stream; every rank issues the same sequence, so the counters agree) -- nothing about an exchange depends on host state,
 * the launches can be captured into a hipGraph and replayed.  World size <= TRIS_MBOX_MAX_WORLD. */
#define TRIS_MBOX_MAX_WORLD 16
long tris_mbox_bytes(int cap_floats);
int tris_mbox_alloc(void** ptr, int cap_floats);
int tris_mbox_free(void* ptr);
int tris_mbox_ipc_handle(void* ptr, void* handle64);
int tris_mbox_ipc_open(const void* handle64, void** ptr);
int tris_mbox_ipc_close(void* ptr);
int tris_mbox_exchange_f32(const float* src0, int n0, const float* src1, int n1, float* out, void* const* boxes, int world,
                           int rank, unsigned* seq, int cap_floats, int mode, long spin_limit, int* err, void* stream);
/* SyncBatchNorm forward in ONE launch: exchange the [mean | invstd | biased var] block (3 C floats, what tris_bn_finalize_f32 /
 * tris_bn_stats_f32 write) and combine the `world` blocks into the global statistics stats[3C] + running statistics -- the
 * arithmetic of tris_bn_sync_combine_f32.  Every rank contributes count_per_rank rows: the SAME number on every rank (the global
 * count is count_per_rank * world, as with torch's DistributedSampler, which pads the shards to equal length; ranks with
 * unequal per-step batches are not representable here -- nor in tris_bn_sync_combine_f32 -- and must use equal shards). */
int tris_mbox_bn_combine_f32(const float* local_stats, int C, long count_per_rank, float eps, float momentum, float* stats,
                             float* running_mean, float* running_var, void* const* boxes, int world, int rank, unsigned* seq,
                             int cap_floats, long spin_limit, int* err, void* stream);
/* The same two exchanges with the amax WORD of the plane tensor the following pass writes as a by-product (h2 with operand
 * planes, csrc/planes.h) -- what tris_bn_out_bound2_f32 / tris_bn_bwd_bound_f32 compute in launches of their own:
 * forward bound = max_c |gamma_c| xhat_max + |beta_c| (+ the residual's bound, resid_word or NULL); backward: out[2C] = the sums
 * [sum dz | sum dz xhat] over all ranks and bound = max_c |gamma_c invstd_c| (amax dz + |sum dz| inv_count + xhat_max |sum dz xhat|
 * inv_count), amax dz from dz_word.  Two launches less per SyncBatchNorm layer and pass. */
int tris_mbox_bn_combine_bound_f32(const float* local_stats, int C, long count_per_rank, float eps, float momentum, float* stats,
                                   float* running_mean, float* running_var, void* const* boxes, int world, int rank, unsigned* seq,
                                   int cap_floats, long spin_limit, int* err, const float* gamma, const float* beta, float xhat_max,
                                   const unsigned* resid_word, unsigned* bound_word, void* stream);
int tris_mbox_bn_bwd_exchange_f32(const float* sum_dz, const float* sum_dzx, int C, float* out, void* const* boxes, int world, int rank,
                                  unsigned* seq, int cap_floats, long spin_limit, int* err, const float* gamma, const float* invstd,
                                  float inv_count, float xhat_max, const unsigned* dz_word, unsigned* bound_word, void* stream);

/* ---- Stage-2 decoder (csrc/seg.hip; model/model_stage2.py, train_stage2.py) -------------------------------------------
 * Channels-last activations [M = B*h*w, C].  Every sum is a fixed-order two-stage reduction (fp64 partials), no atomics.  Scalars
 * that training changes (the PReLU slope, the loss gradients) are DEVICE pointers. */
/* workspace of tris_bn_prelu_bwd_reduce_f32 / tris_head1_bwd_f32 (bytes, >= what either needs for M rows of C channels) */
long tris_seg_workspace_bytes(long M, int C);
/* ConvBNRelu's BatchNorm2d + nn.PReLU() with ONE slope (model_stage2.py:11-27): z = (X - mean) * invstd * gamma + beta (the
 * expression of tris_bn_apply_f32), Y = z > 0 ? z : slope[0] * z.  Train mode: mean / invstd from tris_bn_finalize_f32 or
 * tris_bn_stats_f32; eval mode: running statistics.  C % 4 == 0. */
int tris_bn_prelu_fwd_f32(const float* X, const float* mean, const float* invstd, const float* gamma, const float* beta,
                          const float* slope, float* Y, long M, int C, void* stream);
/* backward reduce: z recomputed from X; dz = dY * (z > 0 ? 1 : slope); sum_dz[C] (= dbeta), sum_dzx[C] = sum dz * xhat (= dgamma),
 * *dslope = sum dY * z [z <= 0] over all channels.  1024 % C == 0.  workspace: tris_seg_workspace_bytes(M, C). */
int tris_bn_prelu_bwd_reduce_f32(const float* dY, const float* X, const float* mean, const float* invstd, const float* gamma,
                                 const float* beta, const float* slope, long M, int C, float* sum_dz, float* sum_dzx, float* dslope,
                                 double* workspace, void* stream);
/* backward apply: dX = gamma invstd (dz - sum_dz inv_count - xhat sum_dzx inv_count) (tris_bn_bwd_apply_f32's expression); eval
 * mode: inv_count = 0 (the statistics are constants) */
int tris_bn_prelu_bwd_apply_f32(const float* dY, const float* X, const float* mean, const float* invstd, const float* gamma,
                                const float* beta, const float* slope, const float* sum_dz, const float* sum_dzx, float inv_count,
                                float* dX, long M, int C, void* stream);
/* Upsample (F.interpolate bilinear, align_corners=False, model_stage2.py:29-35) of X [B,Hi,Wi,C] to [B,Ho,Wo,C] with the skip add
 * of the top-down path (:127-129 `Upsample(output_k(.), size) + dem`): up <- the upsampled map, sum <- up + skip (either output may
 * be NULL; skip and sum go together).  Source indices and the blend are tris_resize_bilinear_fwd_f32's, so the NCHW and NHWC
 * results agree bit for bit.  backward (gather form, any Ho >= Hi, Wo >= Wi): dX = sum over the output window of (d_up + d_sum)
 * (either may be NULL); the skip's gradient is d_sum itself.  C % 4 == 0. */
int tris_upsample_nhwc_fwd_f32(const float* X, const float* skip, float* up, float* sum, int B, int Hi, int Wi, int Ho, int Wo,
                               int C, void* stream);
int tris_upsample_nhwc_bwd_f32(const float* d_up, const float* d_sum, float* dX, int B, int Hi, int Wi, int Ho, int Wo, int C,
                               void* stream);
/* the one-channel head nn.Conv2d(C, 1, 1, bias=False) of final_seg1..4 (model_stage2.py:75-86): Y[m] = sum_c X[m,c] w[c];
 * backward dX = g (x) w, dw = sum_m g[m] X[m,:].  C % 32 == 0, 1024 % C == 0.  workspace: tris_seg_workspace_bytes(M, C). */
int tris_head1_fwd_f32(const float* X, const float* w, float* Y, long M, int C, void* stream);
int tris_head1_bwd_f32(const float* g, const float* X, const float* w, float* dX, float* dw, long M, int C, double* workspace,
                       void* stream);
/* criterion = F.binary_cross_entropy_with_logits(out, target.float(), reduction='mean') for the four heads (model_stage2.py:139-141,
 * train_stage2.py:314-319): target int64 (target_f32 = 0, the pseudo masks read as is) or fp32 (target_f32 = 1); element loss
 * max(x,0) - x t + log1p(exp(-|x|)), fp64 partials; losses[5] = {l1 + l2 + l3 + l4, l1, l2, l3, l4}.  x2..x4 may be NULL (absent
 * heads: loss 0, no work).  backward: g = DEVICE gradient of losses[5]; dx_k = (sigmoid(x) - t)(g[0] + g[k+1]) / n.  workspace:
 * tris_bce4_workspace_bytes(n). */
long tris_bce4_workspace_bytes(long n);
int tris_bce4_fwd_f32(const float* x1, const float* x2, const float* x3, const float* x4, const void* target, int target_f32, long n,
                      float* losses, double* workspace, void* stream);
int tris_bce4_bwd_f32(const float* x1, const float* x2, const float* x3, const float* x4, const void* target, int target_f32,
                      const float* g, float* d1, float* d2, float* d3, float* d4, long n, void* stream);
/* The Stage-2 step's whole loss with EMA consistency (train_stage2.py:258-269, 302-319) in one pass over the student maps x_k, the
 * teacher maps e_k and the target: the four BCE terms as tris_bce4_fwd_f32 forms them plus l5 = sum_k mean((sigmoid(x_k) -
 * sigmoid(e_k))^2) (sigmoid_mse_loss; the difference is squared in fp64), fp64 block partials, losses[6] = {l1 + l2 + l3 + l4 + l5,
 * l1, l2, l3, l4, l5}.  x2..x4 may be NULL together with their e_k.  backward, one store per element: dx_k = (sigmoid(x) - t)(g[0] +
 * g[k+1]) / n  [exactly tris_bce4_bwd_f32's value]  + 2 (sigmoid(x) - sigmoid(e)) s (1 - s) (g[0] + g[5]) / n,  s = sigmoid(x); e_k
 * gets no gradient.  16-byte accesses when every base pointer is 16-byte aligned, the same element order with 4-byte accesses
 * otherwise (same bits).  workspace: tris_seg_loss5_workspace_bytes(n). */
long tris_seg_loss5_workspace_bytes(long n);
int tris_seg_loss5_fwd_f32(const float* x1, const float* x2, const float* x3, const float* x4, const float* e1, const float* e2,
                           const float* e3, const float* e4, const void* target, int target_f32, long n, float* losses,
                           double* workspace, void* stream);
int tris_seg_loss5_bwd_f32(const float* x1, const float* x2, const float* x3, const float* x4, const float* e1, const float* e2,
                           const float* e3, const float* e4, const void* target, int target_f32, const float* g, float* d1, float* d2,
                           float* d3, float* d4, long n, void* stream);
/* The mean teacher's update (train_stage2.py:328-332; ema_pytorch's ema_param.lerp_(param, 1 - decay)): dst = lerp(dst, src, w) as
 * torch defines it in fp32 -- w < 0.5 ? a + w (b - a) : b - (b - a)(1 - w), no fused multiply-add -- with w == 1 giving src and
 * w == 0 leaving dst bit for bit.  16-byte accesses where dst and src share their offset inside a 16-byte line (the head and
 * tail are peeled), 4-byte ones otherwise.  The table form does the same for `count` records {dst pointer, src pointer, n} (three
 * 64-bit words each, device memory) in one launch: a workgroup walks whole records. */
int tris_lerp_f32(float* dst, const float* src, long n, float w, void* stream);
int tris_lerp_table_f32(const long* table, int count, float w, void* stream);
/* Evaluation of a SIGNED map (Stage-2 logits; validate.py:179-191 as written): cam = bilinear(align_corners=True) / (max + 1e-5)
 * whatever the sign of the max (a negative max flips the sign), mask = cam > 1e-9, out_iu = {I, U, first arg-max of cam}.
 * tris_eval_post_f32 (the arg-max of the raw map) stays the Stage-1 entry.  map: S x S.  workspace >= 2049 + 4*1024 floats. */
int tris_eval_post_signed_f32(const float* map, int S, const unsigned char* target, int oH, int oW, float* cam, long* out_iu,
                              float* workspace, void* stream);
/* PointM and the box metrics of one (image, sentence) (csrc/boxes.hip; validate.py:106-117, 191-208, utils/box_eval_utils.py:10-73,
 * utils/box_utils.py:50-63), DESIGN section 15.  cam [H,W] is the map tris_eval_post*_f32 left, thresholded here at 1e-9; iu its
 * int64[3] (the arg-max is read from iu[2] on the device); target uint8 [H,W]; gt_box int32[4] (x1, y1, x2, y2), device memory.
 * generate_bbox on a boolean mask, restated: proposals = bounding rectangles of the 8-connected foreground components and of the
 * holes (4-connected background components that do not reach the frame) grown by one pixel, ordered by the raster index of each
 * component's first pixel (the project's tie rule); confidence = foreground share (double); torchvision's CPU NMS at 0.05 on
 * the (x, y, w, h) rows read as (x1, y1, x2, y2), float32; kept = survivors with confidence > 0.5 * max over all proposals.
 * record int32[16] = {hitm, proposals, NMS survivors, kept, bbox_hit x1, y1, x2, y2, box_acc, box_miou (float32 bits),
 * max confidence (float64 bits, low word first), 0, 0, 0, 0}; an all-zero / all-one mask gives the reference's default list:
 * 0 proposals, 0 kept, bbox_hit = (0, 0, 1, 1).  boxes_out int32 [kept][5] = (x, y, w, h, foreground count) in kept order, room
 * for H*W + 1 rows.  workspace: tris_eval_boxes_workspace_bytes(H, W) bytes, 8-byte aligned.  H*W <= 2^24 (float32 areas stay
 * exact), else hipErrorInvalidValue (the size query returns -1). */
long tris_eval_boxes_workspace_bytes(int H, int W);
int tris_eval_boxes_f32(const float* cam, const unsigned char* target, int H, int W, const int* gt_box, const long* iu, int* record,
                        int* boxes_out, void* workspace, void* stream);

/* ---- ReferIt evaluation (csrc/referit.hip; validate_referit.py, dataset/Dataset_referit.py), DESIGN section 17 -------------
 * Targets of the K sentences of one image from run lengths (dataset/Dataset_referit.py:141-144: cocomask.decode(rle), np.sum(axis=2),
 * astype(uint8)).  ends int32: for every segment the inclusive prefix sums of its counts, i.e. the column-major position where each
 * run ends (non-decreasing, <= H*W); seg_off int64 [segments + 1]: the slice of `ends` of each segment; ranges int32 [K][2] =
 * {first segment, one past the last} of sentence k; all in device memory.  out uint8 [K][H][W] row-major: out[k][y][x] = the number
 * of segments of sentence k whose run holding position x*H + y has an odd index -- a first count of 0, zero-length runs, counts
 * that stop short of H*W (the rest is background), a sentence without segments (zeros) and overlapping segments (values above 1)
 * included.  At most 255 segments per sentence (the caller checks), H*W <= 2^24, else hipErrorInvalidValue. */
int tris_rle_decode_sum_u8(const int* ends, const long* seg_off, const int* ranges, int K, int H, int W, unsigned char* out,
                           void* stream);
/* K sentences of one image scored in one call (validate_referit.py:160-171, 104-118): maps float32 [K][S][S], targets uint8
 * [K][oH][oW] (counts: a pixel is target where the count is != 0, as logical_and / logical_or read it), cams float32 [K][oH][oW]
 * or NULL.  records int64 [K][4] = {I, U, first arg-max of cam, target value at that arg-max}.  Per sentence the first three
 * words and cams[k] are bit for bit what tris_eval_post_f32 (is_signed = 0) or tris_eval_post_signed_f32 (is_signed = 1) gives
 * on (targets[k] != 0); the fourth is the raw count, which validate_referit.py:111-113 compares with 1.  Four launches whatever
 * K is.  workspace: tris_eval_post_group_workspace_bytes(K) bytes. */
long tris_eval_post_group_workspace_bytes(int K);
int tris_eval_post_group_f32(const float* maps, int S, const unsigned char* targets, int K, int oH, int oW, float* cams, long* records,
                             int is_signed, float* workspace, void* stream);

/* ---- REFER polygon targets as run-length arenas (csrc/polymask.hip; dataset/refer.py:279-291 getMask, dataset/ReferDataset.py
 * load_mask), DESIGN section 19 ------------------------------------------------------------------------------------------------
 * cocomask.frPyObjects of P polygons on the device (dataset/refer.py:283: mask.frPyObjects(ann['segmentation'], h, w)), bit for
 * bit what dataset/cocomask.py:13-54 gives before its zero-run merge.  verts int32 [V][2] = the x5 upsampled vertices
 * (X, Y) = (int(5 x + 0.5), int(5 y + 0.5)) formed by the host in double arithmetic (cocomask.py:18-19), |X|, |Y| <= 2^20;
 * poly_off int64 [P + 1]: the vertex slice of each polygon (an empty slice marks a segment the host fills itself: n_runs = 1,
 * nothing emitted); hw int32 [P][2] = {H, W} of each polygon's canvas, H*W <= 2^24.  All in device memory; the host has checked
 * the bounds (dataset/poly_arena.py), nothing here reads them back.
 * tris_poly_count_runs: n_runs int32 [P] = the polygon's kept column crossings + 1 (the closing H*W).
 * tris_poly_emit_runs: seg_off int64 [P + 1] = the exclusive scan of n_runs; ends[seg_off[p] .. seg_off[p + 1]) = the column-major
 * positions xc*H + yc of the crossings and H*W, sorted ascending with duplicates kept (a duplicate pair is a zero-length run, which
 * tris_rle_decode_sum_u8 reads as cocomask's merge loop does): the (ends, seg_off) arena of tris_rle_decode_sum_u8.  Slices of up to
 * tris_poly_sort_capacity() ends are sorted in LDS, longer ones in place in global memory; one workgroup per polygon, P <= 2^31 - 1. */
int tris_poly_sort_capacity(void);
int tris_poly_count_runs(const int* verts, const long* poly_off, const int* hw, int P, int* n_runs, void* stream);
int tris_poly_emit_runs(const int* verts, const long* poly_off, const int* hw, const long* seg_off, int P, int* ends, void* stream);
/* Training target of one ref from its runs (dataset/ReferDataset.py load_mask: annot[ref_mask == 1] = 1, then dataset/transform.py:32
 * Image.NEAREST): out uint8 [Hout][Wout], out[y][x] = 1 where exactly one of the segments seg_lo .. seg_hi - 1 covers source pixel
 * (yidx[y], xidx[x]) of the H x W canvas, else 0 (index < 0 -> 0), with the index tables of tris_gather2d_u8.  The full-size mask is
 * never formed.  seg_hi - seg_lo <= 255, H*W <= 2^24, else hipErrorInvalidValue. */
int tris_rle_target_nearest_u8(const int* ends, const long* seg_off, int seg_lo, int seg_hi, int H, int W, const int* yidx,
                               const int* xidx, int Hout, int Wout, unsigned char* out, void* stream);

/* ---- Heat-map overlay of single-image inference (csrc/overlay.hip; demo.py:28-48, 94-96), DESIGN section 18 ---------------
 * The K response maps of ONE image painted in one call, two launches whatever K is.  For sentence k and output pixel (y, x):
 * u = max(bilinear(maps[k], align_corners=True)(y, x), 0); lo, hi = min, max of u over the H x W OUTPUT grid;
 * TRIS_PAINT_MINMAX: n = (u - lo) / (hi - lo + 1e-5f) (get_norm_cam);  TRIS_PAINT_UNIT: n = min(u, 1) (maps already in [0, 1]);
 * i = (int)(n * 255) by truncation (np.uint8), c = lut[i]; heat = (3 c + 2 image + 2) / 5 per channel in integers -- cv2's
 * addWeighted(.6, .4) with round-to-nearest -- or c where image is NULL (visualize_cam's original=None).  norm (may be NULL) gets n;
 * range[k] = {lo, hi}; argmax[k] = raster index of the first pixel whose u equals hi (np.argmax).  The colour table is data: 256
 * RGB rows.  Sh, Sw, H, W >= 1; K = 0 succeeds without a launch; K <= 65535.  heat 4-byte, norm 16-byte, workspace 8-byte
 * aligned, else hipErrorInvalidValue.  A sentence's outputs do not depend on the K it shares the call with.  No host
 * synchronisation, no allocation: the call can be captured.  workspace: tris_cam_paint_workspace_bytes(K, H, W) bytes. */
#define TRIS_PAINT_MINMAX 0
#define TRIS_PAINT_UNIT 1
long tris_cam_paint_workspace_bytes(int K, int H, int W);
int tris_cam_paint_f32(const float* maps /*[K][Sh][Sw]*/, int K, int Sh, int Sw,
                       const unsigned char* image /*[H][W][3] or NULL*/, int H, int W,
                       const unsigned char* lut /*[256][3]*/, int mode,
                       unsigned char* heat /*[K][H][W][3]*/, float* norm /*[K][H][W] or NULL*/,
                       float* range /*[K][2] = {min, max} after the clamp*/, long* argmax /*[K]*/,
                       void* workspace, void* stream);

/* ---- Instance-mask synthesis (csrc/insseg.hip; irn.py): the post-network half of IRNet's make_ins_seg_labels --------------
 * (response map, edge map [h,w], displacement field [2,h,w]) -> instance masks, the pseudo labels Stage 2 trains on.  Reference
 * lines are those of IRNet/step_refer/make_ins_seg_labels.py ("labels.py") and IRNet/misc/indexing.py.  f32 on the vector ALU;
 * the dense N x N transition matrix of indexing.py:112-139 is never formed. */
/* find_centroids_with_refinement (labels.py:18-56): `iterations` steps of bilinear gather at (ceil, floor), move, clip; then
 * round half to even.  centroids int32 [2,h,w] = (y, x).  The reference's numpy expression promotes to float64 (float32 minus
 * int32) and rounds to float32 once per step; the kernel does the same operations in the same order without contraction, so the
 * result is bit-identical. */
int tris_irn_centroids_f32(const float* dp, int h, int w, int iterations, int* centroids, void* stream);
/* cluster_centroids (labels.py:61-64): mask = sqrt(dp[1]^2 + dp[0]^2) < thres, uint8 [h,w] */
int tris_irn_weak_mask_f32(const float* dp, int h, int w, float thres, unsigned char* mask, void* stream);
/* skimage.measure.label(img, connectivity=1, background=0) (labels.py:66, :92) of B images uint8 [B,H,W]: labels int32 [B,H,W]
 * numbered 1..counts[b] by each component's first pixel in raster order, 0 on the background.  Union-find whose root is the
 * component's minimum linear index (pixels start linked to the neighbour above or to the left), then a rank pass over the roots: deterministic and order-exact.  B <= 65535.
 * workspace: tris_cc_workspace_bytes(B, H, W). */
long tris_cc_workspace_bytes(int B, int H, int W);
int tris_cc_label_u8(const unsigned char* img, int B, int H, int W, int* labels, int* counts, int* workspace, void* stream);
/* cluster_centroids (labels.py:67-75): inst_map[p] = rank, among the values that occur, of dp_label[centroid of p]
 * (imutils.compress_range of the label + 1); n_inst[0] = the number of instances K.  dp_label holds 0..n_label.
 * workspace: n_label + 1 ints. */
int tris_irn_cluster_i32(const int* centroids, const int* dp_label, int n_label, int h, int w, int* inst_map, int* n_inst,
                         int* workspace, void* stream);
/* separte_score_by_mask (labels.py:77-80): out[k][p] = inst_map[p] == k ? cam[p] : 0, out [K,n] */
int tris_irn_instance_cam_f32(const float* cam, const int* inst_map, int K, int n, float* out, void* stream);
/* PathIndex + edge_to_affinity + torch.pow + the column sum (indexing.py:18-109, :132-135, :141-158): Wt[d][p] =
 * (1 - max of edge over the path cells from p to p + dirs[d]) ^ beta, 0 where p + dirs[d] is outside the map (the reference's
 * padding with 1.0); colsum[p] = 1 + the weights of the 2 n_dirs pairs incident to p.  dirs int32 [n_dirs,2] = (dy, dx) with
 * dy >= 0; path cells of direction d: path_cells[path_off[d] .. path_off[d+1]) as (dy, dx), both ends included (host tables,
 * irn.search_paths).  Wt [n_dirs, h*w], colsum [h*w]. */
int tris_irn_affinity_f32(const float* edge, int h, int w, const int* dirs, const int* path_off, const int* path_cells, int n_dirs,
                          float beta, float* Wt, float* colsum, void* stream);
/* propagate_to_edge (indexing.py:160-164): v0 = x (1 - edge), then `steps` = 2^exp_times products v <- v T as gathers
 * v[j] <- (v[j] + sum_d Wt[d][j] v[j+dir_d] + Wt[d][j-dir_d] v[j-dir_d]) / colsum[j] for K rows; x, out [K, h*w].
 * One launch per step; the rows ping-pong between out and tmp [K, h*w], any map size. */
int tris_irn_walk_f32(const float* x, const float* edge, const float* Wt, const float* colsum, const int* dirs, int n_dirs, int K,
                      int h, int w, int steps, float* out, float* tmp, void* stream);
/* labels.py:146-157: rw_up = F.interpolate(rw, scale_factor=4, bilinear, align_corners=False) cropped to (H, W), divided by its
 * global maximum; labels = argmax over [bg_thres, rw_up[0], ...] (first maximum wins: the background wins ties).  rw [K,h,w],
 * rw_up [K,H,W], labels int32 [H,W] in 0..K.  H <= 4h, W <= 4w.  workspace >= 1025 floats. */
int tris_irn_finish_f32(const float* rw, int K, int h, int w, int H, int W, float bg_thres, float* rw_up, int* labels,
                        float* workspace, void* stream);
/* pyutils.to_one_hot (labels.py:75, :157): masks[k][i] = labels[i] == k + base, uint8 [K,n]; base = 1 is to_one_hot(labels)[1:] */
int tris_irn_label_masks_u8(const int* labels, int K, long n, int base, unsigned char* masks, void* stream);
/* detect_instance (labels.py:82-105) after tris_cc_label_u8 of the K masks: fragment g = offsets[k] + f - 1 for label f of row k
 * (offsets = exclusive prefix of the counts, F their sum): frag_masks uint8 [F,n], area int32 [F], score [F] =
 * max(rw_up[k] * mask) or 0 where area < min_area.  workspace: F ints. */
int tris_irn_fragments_f32(const int* frag_labels, const float* rw_up, const int* offsets, int K, long n, long min_area, int F,
                           float* score, int* area, unsigned char* frag_masks, int* workspace, void* stream);

/* ---- IRNet edge / displacement network, inference (csrc/irnnet.hip; irn_net.py) --------------------------------------------
 * What IRNet/net/resnet50_irn.py ("irn.py") and IRNet/net/resnet50.py ("resnet50.py") need beyond the dense products
 * (tris_gemm_f32, tris_conv3x3_fwd_f32) and the frozen BatchNorm (tris_bn_apply_f32).  Channels-last, fp32, no atomics: every
 * launch is bitwise reproducible. */
/* stage1 up to the ReLU (resnet50.py:61-64, :95-97) on the loader's batch [img, flip_w(img)] (IRNet/voc12/dataloader.py:338-340):
 * img uint8 [H][W][3]; lut [3][256] = the TorchvisionNormalize table (dataloader.py:77-79, float64 rounded once);
 * Wk = conv1.weight as [7][7][3][64]; Y [2][Ho][Wo][64] = relu(bn1(conv1(x))) with tris_bn_apply_f32's expression,
 * Ho = (H-1)/2 + 1.  Direct fp32 FMA kernel on the vector ALU. */
int tris_irn_stem_f32(const unsigned char* img, const float* lut, const float* Wk, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, float* Y, int H, int W, void* stream);
/* nn.MaxPool2d(kernel_size=3, stride=2, padding=1) (resnet50.py:65): the padding never wins.  Y [B][(H-1)/2+1][(W-1)/2+1][C], C % 4 == 0 */
int tris_maxpool3s2_f32(const float* X, float* Y, int B, int H, int W, int C, void* stream);
/* the input gather of the strided 1x1 downsample convolution (resnet50.py:82-83): Y[b][i][j] = X[b][2i][2j] */
int tris_subsample2_f32(const float* X, float* Y, int B, int H, int W, int C, void* stream);
/* nn.GroupNorm(G, C) statistics (irn.py:31 ... :95) per image over HW pixels x C/G channels: fixed-order fp64 partials per row
 * block, then one finalize; stats [B][G][2] = {mean, 1/sqrt(biased var + eps)}.  C <= 1024, 256 % (C/4) == 0, (C/G) % 4 == 0.
 * workspace: tris_gn_workspace_bytes(B, HW, G). */
long tris_gn_workspace_bytes(int B, long HW, int G);
int tris_gn_stats_f32(const float* X, int B, long HW, int C, int G, float eps, float* stats, double* workspace, void* stream);
/* GroupNorm apply -> nn.Upsample(scale_factor=scale, bilinear, align_corners=False) -> crop to (Ho, Wo) -> ReLU (irn.py:39-44,
 * :125-127, :133-136), written with pixel pitch ldy floats (a channel slice of the torch.cat buffer of irn.py:128, :136-137):
 * Y[b][oy][ox][c] for oy < Ho <= Hi*scale.  The blend is tris_upsample_nhwc_fwd_f32's.  scale = 1: no resampling.
 * stats == NULL: no normalisation (upsample + crop only). */
int tris_gn_apply_up_f32(const float* X, const float* stats, const float* gamma, const float* beta, float* Y, int B, int Hi, int Wi,
                         int C, int G, int scale, int Ho, int Wo, long ldy, int relu, void* stream);
/* the narrow heads fc_edge6 = nn.Conv2d(160, 1, 1, bias=True) (irn.py:57) and fc_dp7's nn.Conv2d(256, 2, 1) + MeanShift
 * (irn.py:97-98, :114: bias = -running_mean): Y[m][n] = sum_c X[m*ldx + c] w[n][c] + bias[n] (bias may be NULL).
 * N = 1 | 2, C % 32 == 0. */
int tris_irn_head_f32(const float* X, long ldx, const float* w, const float* bias, float* Y, long M, int C, int N, void* stream);
/* EdgeDisplacement.forward (irn.py:240-241): edge[y][x] = sigmoid(E[0][y][x]/2 + E[1][y][w-1-x]/2), dp[c][y][x] = D[0][y][x][c];
 * E [2][h][w], D [2][h][w][2] */
int tris_irn_net_finish_f32(const float* E, const float* D, float* edge, float* dp, int h, int w, void* stream);

/* ---- IRNet affinity / displacement training losses (csrc/irnloss.hip; irn_loss.py) -----------------------------------------
 * The loss head of IRNet/step_refer/train_irn.py ("train_irn.py") on AffinityDisplacementLoss of IRNet/net/resnet50_irn.py
 * ("irn.py"), with the pair labels of GetAffinityLabelFromIndices (IRNet/voc12/dataloader.py, "dataloader.py", dataloader.py:83-109)
 * derived from the label map in the kernel.
 * edge_out [B,1,h,w] logits, dp_out [B,2,h,w], label uint8 [B,h,w]; r = radius - 1 <= 15, h >= r + 1, w >= 2r + 1.  Pairs:
 * source (y, x) with y < h - r, r <= x < w - r, destination source + dirs[d] (irn.py:183-199, indexing.py:58-88); tables as for
 * tris_irn_affinity_f32 (n_cells = rows of path_cells).  fp64 arithmetic on the fp32 inputs; integer adds only: every launch is
 * bitwise reproducible. */
/* bytes of the partials buffer of tris_irn_loss_fwd_f32 (5 fp64 sums and 3 integer counts per 16 x 16 tile of source pixels);
 * 0 for a shape the op refuses */
long tris_irn_loss_workspace_bytes(int B, int h, int w, int radius);
/* irn.py:168-181 to_affinity (index_select + max_pool2d over the path cells), irn.py:211-220 (pos = -log(aff + 1e-5), neg =
 * -log(1 + 1e-5 - aff), |pair_disp - (dy, dx)|, |pair_disp|), dataloader.py:97-106 (bg_pos / fg_pos / neg from the labels of the
 * two ends, both < 21) and train_irn.py:57-63: losses[4] = {bg_pos / 2 + fg_pos / 2, neg, dp_fg, dp_bg}, each sum over its class
 * divided by N + 1e-5 (2 N + 1e-5 for the two-channel dp terms); counts[3] = {N_bg, N_fg, N_neg}.  norm[5] = the five scales,
 * kept on the device for the backward.  arg_count int32 [B,3,h,w] (NULL when no backward follows): per class, the pairs whose
 * path maximum is at the cell; among equal maxima the first cell in the reference's path order (indexing.py:48) takes the pair,
 * as max_pool2d's backward does.  workspace: tris_irn_loss_workspace_bytes. */
int tris_irn_loss_fwd_f32(const float* edge_out, const float* dp_out, const unsigned char* label, int B, int h, int w, int radius,
                          const int* dirs, const int* path_off, const int* path_cells, int n_dirs, int n_cells, float* losses,
                          long* counts, double* norm, int* arg_count, void* workspace, void* stream);
/* total_loss.backward() of train_irn.py:68-71 down to edge_out and dp_out: g = DEVICE gradient of losses[4], no host sync.
 * d_edge[q] = s (1 - s) (g0 (norm0 n_bg + norm1 n_fg) / (1 - s + 1e-5) - g1 norm2 n_neg / (s + 1e-5)) with s = sigmoid(edge_out[q])
 * and n_* = arg_count at q; d_dp[q] = g2 norm3 (sum of sign(pair_disp - (dy, dx)) over the fg pairs q is the source of, minus
 * that over the pairs it is the destination of) + g3 norm4 (the same with sign(pair_disp) over the bg pairs); sign(0) = 0.
 * d_edge / d_dp may be NULL (not wanted). */
int tris_irn_loss_bwd_f32(const float* edge_out, const float* dp_out, const unsigned char* label, int B, int h, int w, int radius,
                          const int* dirs, int n_dirs, const int* arg_count, const double* norm, const float* g, float* d_edge,
                          float* d_dp, void* stream);

/* ---- IRNet edge / displacement heads, training (csrc/irntrain.hip, csrc/irnnet.hip, csrc/optim.hip; irn_train.py) ------------
 * What IRNet/step_refer/train_irn.py:55-72 needs below the loss head: the trunk is frozen and its taps detached (irn.py:117-121,
 * :145-147), so only fc_edge1..6 and fc_dp1..7 have a backward.  fp64 block partials summed in index order, no atomics: every
 * launch is bitwise reproducible. */
/* stage1 up to the ReLU (resnet50.py:61-64) on a batch of normalised float images, as the training loader delivers them
 * (dataloader.py:249-256 pads with zeros AFTER the normalisation, which no uint8 + table input can express):
 * img [B][H][W][3] -> Y [B][Ho][Wo][64], no flip row; the same kernel body and arithmetic as tris_irn_stem_f32. */
int tris_irn_stem_batch_f32(const float* img, const float* Wk, const float* mean, const float* invstd, const float* gamma,
                            const float* beta, float* Y, int B, int H, int W, void* stream);
/* autograd's backward of nn.GroupNorm -> nn.Upsample(scale) -> [..., :Ho, :Wo] -> nn.ReLU (irn.py:29-96, :125-137): the adjoint of
 * tris_gn_apply_up_f32 with relu = 1.  dY / Y: gradient and forward output in the concatenation buffer (pixel pitch ldy, both
 * pointers already at the slice's first channel; the mask is Y > 0); T [B][Hi][Wi][C] the GroupNorm input; stats as
 * tris_gn_stats_f32 left them.  dT [B][Hi][Wi][C] = gradient of T; dU (may be NULL): the gradient of the GroupNorm OUTPUT, before
 * the norm's own backward; dgamma, dbeta [C].  scale = 1 | 2 | 4.  workspace: tris_gn_up_bwd_workspace_bytes. */
long tris_gn_up_bwd_workspace_bytes(int B, long HW, int C, int G);
int tris_gn_up_bwd_f32(const float* dY, const float* Y, long ldy, const float* T, const float* stats, const float* gamma, float* dT,
                       float* dU, float* dgamma, float* dbeta, int B, int Hi, int Wi, int C, int G, int scale, int Ho, int Wo,
                       void* workspace, void* stream);
/* backward of tris_irn_head_f32 (fc_edge6, irn.py:57; fc_dp7's last convolution, :97): g [M][N] the gradient of Y;
 * dX[m][c] = sum_n g[m][n] w[n][c] (pitch C), dw[n][c] = sum_m g[m][n] X[m*ldx + c], db[n] = sum_m g[m][n] (db may be NULL).
 * N = 1 | 2, C % 32 == 0, C <= 256.  workspace: tris_irn_head_bwd_workspace_bytes. */
long tris_irn_head_bwd_workspace_bytes(long M, int C, int N);
int tris_irn_head_bwd_f32(const float* g, const float* X, long ldx, const float* w, float* dX, float* dw, float* db, long M, int C,
                          int N, void* workspace, void* stream);
/* one step of torch.optim.SGD as PolyOptimizer drives it (IRNet/misc/torchutils.py:9-31) over a flat arena: g = grad + wd p;
 * buf = g when first != 0, else momentum buf + g; p -= lr buf.  The poly schedule of lr is the host's. */
int tris_sgd_momentum_f32(float* p, const float* g, float* buf, long n, float lr, float momentum, float weight_decay, int first,
                          void* stream);

/* ---- IRNet's training input pipeline (csrc/irndata.hip; dataset/irn_data.py) ------------------------------------------------
 * What ReferAffinityDataset.__getitem__ (IRNet/voc12/dataloader.py:222-285) does per sample on the host, for a whole batch in one
 * launch from uint8 arenas in HBM: random_scale (IRNet/misc/imutils.py:48-55: Pillow BICUBIC image, NEAREST label), the
 * normalisation (dataloader.py:67-81) through lut [3][256], random_lr_flip (imutils.py:57-66), random_crop / top_left_crop with
 * fills 0 / 255 (imutils.py:68-130) and pil_rescale(label, 0.25, 0) (dataloader.py:281).  Bit-exact against Pillow.
 * desc [B][TRIS_IRN_AUG_DESC] longs: image offset (bytes, a multiple of 16; images [H][W][3]), label offset ([H][W]), H, W, target
 * H, target W, the box of imutils.py:91 (cont_top, cont_bottom, cont_left, cont_right, img_top, img_bottom, img_left, img_right),
 * flags (1: horizontal table, 2: vertical table, 4: flipped), taps per column / row entry, and six offsets into `tables` (ints):
 * column bounds [cw][2] and taps [cw][kh], row bounds [ch][2] and taps [ch][kv], the label's source column [cw] and row [ch], all
 * in the order of the box's columns and rows.  An axis without a table is not resampled.  The host checks every entry
 * (irn_data.validate_batch): at most TRIS_IRN_AUG_KMAX taps, at most TRIS_IRN_AUG_PATCH source rows / columns under one
 * TRIS_IRN_AUG_TILE-wide tile.  The image arena ends in 16 spare bytes.
 * img [B][crop][crop][3] f32 (what tris_irn_stem_batch_f32 reads), label [B][crop][crop], label_reduced [B][crop/4][crop/4];
 * crop % 4 == 0.  No atomics: two runs give equal bytes. */
#define TRIS_IRN_AUG_TILE 32
#define TRIS_IRN_AUG_PATCH 80
#define TRIS_IRN_AUG_KMAX 12
#define TRIS_IRN_AUG_DESC 24
int tris_irn_augment_batch_u8(const unsigned char* img_arena, const unsigned char* lab_arena, const long* desc, const int* tables,
                              const float* lut, float* img, unsigned char* label, unsigned char* label_reduced, int B, int crop,
                              void* stream);

/* ---- IRNet's dense-CRF label pass (csrc/crf.hip; crf.py) ---------------------------------------------------------------------
 * IRNet/step_refer/cam_to_ir_label.py:45-76 ("cam_to_ir_label.py") and crf_inference_label of IRNet/misc/imutils.py:169-183
 * ("imutils.py"): DenseCRF2D's mean field (Kraehenbuehl & Koltun 2011) with the Gaussian (imutils.py:178) and bilateral
 * (imutils.py:179) Potts terms filtered on the permutohedral lattice (Adams, Baek & Davis 2010), as DESIGN.md section 14 states it.
 * N = H W pixels, d = 2 (Gaussian) | 5 (bilateral) feature dimensions, M lattice vertices, C = 1 | 2 | 4 channels laid out
 * [N][C] / [M][C].  f32, no atomics: every launch is bitwise reproducible. */
/* the packed vertex key: d signed coordinates of TRIS_CRF_FIELD_BITS bits each, biased by 2^(bits-1), coordinate 0 in the highest
 * field; the host refuses an image whose coordinates could leave the field (crf.check_size) */
#define TRIS_CRF_FIELD_BITS 12
/* addPairwiseGaussian / addPairwiseBilateral's feature embedding (imutils.py:178-179): per pixel the d+1 enclosing lattice vertices
 * keys [N][d+1] (packed) and their barycentric weights bary [N][d+1].  tx [W], ty [H], tc [256]: the host's float32 tables x / sxy,
 * y / sxy, v / srgb; scale [d] = sqrt(2/3) (d+1) / sqrt((i+1)(i+2)) computed in double.  d = 2: features (tx[x], ty[y]), img and tc
 * unused (NULL); d = 5: (tx[x], ty[y], tc[r], tc[g], tc[b]) of img uint8 [H][W][3].  One rounding per operation, no contraction:
 * bit-identical to the float32 restatement.  6 H W < 2^31. */
int tris_crf_lattice_points_f32(const unsigned char* img, const float* tx, const float* ty, const float* tc, const float* scale,
                                int H, int W, int d, long* keys, float* bary, void* stream);
/* the blur's neighbour table (imutils.py:181, the lattice behind d.inference): uniq [M] the sorted distinct keys; nbr [d+1][2][M] =
 * the index of (key - 1 everywhere, + d + 1 at the axis) and of its opposite, found by binary search, -1 where absent */
int tris_crf_neighbours_i64(const long* uniq, int M, int d, int* nbr, void* stream);
/* one filter pass K (imutils.py:181, one Potts term of one mean-field iteration): out = norm * alpha * slice(blur(splat(norm * x))),
 * alpha = 1 / (1 + 2^-d); norm [N] may be NULL (plain K).  inv [N][d+1]: the vertex index of every (pixel, r); order [N (d+1)]: the
 * (pixel, r) pairs e = p (d+1) + r sorted by vertex, ascending within a vertex; off [M+1]: each vertex's span of `order`.  Splat
 * is a segmented sum in list order (no float atomics), then the d+1 blur steps, one launch each, then slice.  x and out may be the
 * same buffer.  workspace: tris_crf_filter_workspace_bytes(M, C). */
long tris_crf_filter_workspace_bytes(int M, int C);
int tris_crf_filter_f32(const float* x, float* out, int N, int C, int d, int M, const float* bary, const int* inv,
                        const int* order, const int* off, const int* nbr, const float* norm, float* workspace, void* stream);
/* the symmetric normalisation of both terms (imutils.py:178-179, NormalizationType.NORMALIZE_SYMMETRIC, the default):
 * norm = 1 / sqrt(k1 + 1e-20) with k1 = K 1 */
int tris_crf_norm_f32(const float* k1, int N, float* norm, void* stream);
/* cam_to_ir_label.py:51-52, :61-62, :66-67 and unary_from_labels (imutils.py:175): c = cam < 0 ? 0 : cam, label = c > thr (strict:
 * the argmax of [thr, cam] gives 0 on a tie) for thr_fg and thr_bg; U [N][2 CRFs][2 labels] = e_same where the label agrees else
 * e_diff (-log(gt_prob), -log(1 - gt_prob) as float32); Q = softmax(-U) */
int tris_crf_unary_cam_f32(const float* cam, int N, float thr_fg, float thr_bg, float e_same, float e_diff, float* U, float* Q,
                           void* stream);
/* the same from R = 1 | 2 given label maps uint8 [R][N] holding 0 / 1 (imutils.py:175 with the caller's labels): U, Q [N][R][2] */
int tris_crf_unary_labels_u8(const unsigned char* labels, int R, int N, float e_same, float e_diff, float* U, float* Q,
                             void* stream);
/* one mean-field update (imutils.py:181): Q = softmax over the two labels of -U + wg g + wb b, the maximum subtracted; g, b the
 * two filtered terms [N][R][2] */
int tris_crf_update_f32(const float* U, const float* g, const float* b, float wg, float wb, int N, int R, float* Q, void* stream);
/* imutils.py:183 and cam_to_ir_label.py:58-74: pred = argmax over the labels (the first on a tie) of both CRFs of Q [N][2][2];
 * conf = fg_pred; conf[fg_pred == 0] = 255; conf[bg_pred + fg_pred == 0] = 0; out uint8 [N] */
int tris_crf_combine_u8(const float* Q, int N, unsigned char* out, void* stream);

/* ---- CLIP attention pooling, inference (csrc/attnpool.hip; CLIP/clip/model.py:58-104 AttentionPool2d), DESIGN section 20 ------
 * f32 memory streams, 16-byte accesses along C, no atomics, every sum in index order: a launch is bitwise repeatable. */
/* The token matrix of AttentionPool2d.forward (CLIP/clip/model.py:70-83: reshape, permute, mean, cat, F.interpolate of the
 * positional grid (:76, bilinear, align_corners=False, no antialiasing also when shrinking), cat, add) in one launch.
 * c4 [B][h][w][C] channels-last, pos [S*S+1][C]; T [B][hw+1][C]: row 0 = the mean over the hw pixels (summed in pixel order, one
 * division) + pos[0]; row 1+i = pixel i + the S x S grid pos[1:] resized to h x w.  Source positions are exact rationals and every
 * weight one float division (csrc/bilinear.h lerp_exact_of); with h = w = S the pixel rows are c4 + pos[1:] bit for bit.
 * B, h, w, S >= 1, hw + 1 <= TRIS_ATTNPOOL_LMAX, C % 4 == 0, B <= 65535, pointers 16-byte aligned, else hipErrorInvalidValue. */
#define TRIS_ATTNPOOL_LMAX 1025
int tris_attnpool_tokens_f32(const float* c4, const float* pos, float* T, int B, int h, int w, int C, int S, void* stream);
/* One-query attention of every head against the tokens themselves (the folded form of CLIP/clip/model.py:84-102 for the global
 * embedding): P[b][hd][j] = softmax_j(scale * T[b][j] . U[b][hd]) -- the maximum subtracted, the sum in key
 * order, one division per element -- and pooled[b][hd] = sum_j P[b][hd][j] T[b][j], summed in key order.
 * T [B][L][C]; U and pooled: element (b, hd, c) at b * strideB + hd * strideH + c (floats; both strides % 4 == 0), the same strides
 * for both, so a head-major [heads][B][C] buffer (what a per-head batched product reads and writes) needs no transpose;
 * P [B][heads][L] contiguous.  One workgroup per image and group of 8 heads (4, 2, 1: the largest that divides heads).
 * B, heads >= 1, 1 <= L <= TRIS_ATTNPOOL_LMAX, C % 4 == 0, B * heads / group <= 2^31 - 1, pointers 16-byte aligned, else
 * hipErrorInvalidValue. */
int tris_attnpool_pool_f32(const float* T, const float* U, long strideB, long strideH, float scale, float* P, float* pooled, int B,
                           int L, int C, int heads, void* stream);

/* ---- Scoring response maps, CRF labels and pseudo masks against REFER ground truth (csrc/labelscore.hip; the passes
 * IRNet/run_sample_refer.py:59,98,102 names and the reference does not ship), DESIGN section 21 -----------------------------------
 * The ground truth stays the (ends, seg_off) arena of tris_rle_decode_sum_u8; no full-size target is formed.  The count c of pixel
 * (y, x) is the number of segments seg_lo .. seg_hi - 1 whose run holding position x*H + y has an odd index (a position past the last
 * run counts 0).  Its bit: gt_rule 0 -> c == 1 (dataset/ReferDataset.py load_mask: annot[ref_mask == 1] = 1), gt_rule 1 -> c != 0
 * (validate.py:183-190 on target != 0, ReferIt).  Every workgroup counts in LDS and stores one int32 partial row; a second launch sums
 * the rows in block order into int64: no global atomics, the same bytes on every run.  A ref's runs are staged in LDS when all of them
 * fit tris_score_stage_capacity() words and searched in global memory otherwise.  workspace: tris_score_workspace_bytes(G, H, W,
 * bins) bytes, bins = T + 1 for the maps and 256 (G = 1) for the counts; -1 for arguments out of range.
 * The host checks what the device cannot refuse: ranges inside the arena and at most 255 segments long, thresholds finite and
 * strictly ascending. */
int tris_score_stage_capacity(void);
long tris_score_workspace_bytes(int G, int H, int W, int bins);
/* validate.py:183-190 and utils/util.py compute_mask_IU (pred = map.gt(thr); I = sum(pred & target), U = sum(pred | target)) for G
 * maps of one size and a whole threshold list in one pass: maps float32 [G][H][W] row-major, ranges int32 [G][2] the ref of each map,
 * thresholds float32 [T] strictly ascending and finite, 1 <= T <= 64.  hist int64 [G][T + 1][2]: hist[g][b][bit] = the pixels of map g
 * with exactly b thresholds strictly below their value (float32 comparison: a value equal to a threshold is not above it, a NaN is
 * above none, +inf above all) and that ground-truth bit.  For threshold j: I = sum_{b > j} hist[b][1],
 * U = sum_{b > j} hist[b][0] + sum_b hist[b][1].  G <= 65535, H*W <= 2^24, else hipErrorInvalidValue. */
int tris_score_maps_f32(const float* maps, const int* ends, const long* seg_off, const int* ranges, int G, int H, int W,
                        const float* thresholds, int T, int gt_rule, long* hist, void* workspace, void* stream);
/* A uint8 stack [K][H][W] against one ref: hist int64 [256][2], hist[s][bit] = the pixels whose byte sum over the K planes (mod 256;
 * a bool stack of K <= 255 cannot wrap) is s and that carry that ground-truth bit.  K = 1: a label image of
 * IRNet/step_refer/cam_to_ir_label.py:72-76 (1 object, 0 background, 255 neither).  A bool stack: the instance masks of
 * IRNet/step_refer/make_ins_seg_labels.py:160-163, whose sum dataset/ReferDataset.py's pseudo loading turns into the Stage-2 target
 * (s > 0 predicted, s > 1 overlapping).  K = 0: nothing is read (stack may be NULL), every pixel has sum 0.  0 <= K <= 255,
 * seg_hi - seg_lo <= 255, H*W <= 2^24, else hipErrorInvalidValue. */
int tris_score_counts_u8(const unsigned char* stack, int K, const int* ends, const long* seg_off, int seg_lo, int seg_hi, int H, int W,
                         int gt_rule, long* hist, void* workspace, void* stream);
/* The same stack against the same ref, plane by plane and optionally at the Stage-2 training resolution (the instance pass
 * IRNet/run_sample_refer.py:102 --eval_ins_seg_pass names; IRNet/step_refer/make_ins_seg_labels.py:95-101 keeps the fragments it
 * scores 0 in 'mask', and dataset/ReferDataset.py sums all planes).  table int64 [K + 3][2], second index the ground-truth bit of the
 * sample; with s = sum_k stack[k] as an integer (no byte wrap): row 0 s == 0, row 1 s == 1, row 2 s >= 2, row 3 + k stack[k] != 0.
 * yidx int32 [Hout], xidx int32 [Wout] are the index tables of tris_gather2d_u8: the samples are the multiset (yidx[y], xidx[x]), a
 * repeated index counts as often as it appears, an entry < 0 (or beyond the canvas) is a sample with every plane 0 and bit 0, as
 * tris_mask_sum_nearest_u8 and tris_rle_target_nearest_u8 write 0 there: rows 0 .. 2 are the histogram of the one against the other.
 * Both NULL: every pixel once, Hout == H and Wout == W.  The host guarantees that the entries >= 0 of a table do not decrease (Pillow's
 * NEAREST tables do not): the run walk goes forward only, and a table that went back would give wrong bits (no read outside the
 * runs).  Tiles are of the output grid; workspace: tris_score_planes_workspace_bytes(K, Hout, Wout) bytes (K + 3 may exceed the 256
 * bins of tris_score_workspace_bytes), -1 for arguments out of range.  0 <= K <= 255 (K = 0: stack may be NULL), seg_hi - seg_lo <=
 * 255, H*W <= 2^24, Hout*Wout <= 2^24, one table NULL and the other not, else hipErrorInvalidValue. */
long tris_score_planes_workspace_bytes(int K, int Hout, int Wout);
int tris_score_planes_u8(const unsigned char* stack, int K, const int* ends, const long* seg_off, int seg_lo, int seg_hi, int H, int W,
                         const int* yidx, const int* xidx, int Hout, int Wout, int gt_rule, long* table, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIS_HIP_H */
