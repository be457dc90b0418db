/* wtpse_hip.h — C ABI of libwtpse_hip.so: the MI355X (gfx950) kernels behind the WT-PSE training hot path.
 *
 * The reference (tonyckc/WT-PSE-code) has no FFI of its own: its boundary is the Python class surface of
 * algorithms.py / shape_networks.py, which wt-pse-code_amd/{algorithms,shape_networks}.py mirror.
 * This library sits directly below that surface.  Each entry point replaces the stock ATen dispatches the
 * reference reaches from the cited lines.  The library itself is compiled against this file: a definition that disagrees
 * with its declaration here does not build.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; every pointer is DEVICE memory unless stated; tensors are NCHW fp32,
 *     contiguous, caller-owned.  No allocation, no host synchronisation and no stream creation inside: scratch
 *     ("partial", "slab", "ws") is passed in, `stream` is a hipStream_t (NULL = default stream), so every call is
 *     legal inside hipGraph capture.
 *   - return 0 on success, -1 (WTPSE_EINVAL) for rejected arguments, otherwise the hipError_t of the launch.
 *   - "pro" (prologue) = optional per-channel [C][2] (scale, shift) applied to an input as it is loaded, followed by
 *     ReLU when the matching relu bit is set: BatchNorm-apply + activation fused into the consumer.
 */
#ifndef WTPSE_HIP_H
#define WTPSE_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- convolution: nn.Conv2d 3x3 pad 1 / 1x1 (algorithms.py:882-888,926-933,404-424,991,1006-1012,1199-1201;
 *      shape_networks.py:182-193,332-338,376-383,459-465) ------------------------------------------------------- */

/* OIHW parameters -> kernel layouts, all convs of a network in one launch.
 * desc: n_desc x 8 ints {w_off, Cout, Cin, taps, wf_off (-1: none), wd_off (-1: none), 0, 0}, offsets in floats into
 * `params` / `packed`.  wf = [ceil4(Cin)][taps][ceil16(Cout)], wd = [ceil4(Cout)][taps][ceil16(Cin)] (tap-flipped). */
int wtpse_pack_conv_weights(const float* params, const int* desc, int n_desc, float* packed, void* stream);

/* out = conv(cat(in0, in1)) [+ bias] [ReLU].  in1 may be NULL (C1 = 0): torch.cat (algorithms.py:955,1018) is virtual.
 * pro0 / pro1: [C0][2] / [C1][2] (scale, shift) for in0 / in1, or NULL; pro_relu bit0 / bit1: ReLU on in0 / in1 after it.
 * Output channels [0, Csplit) go to out0, the rest to out1 (Csplit == Cout, out1 NULL: no split; otherwise Csplit % 16 == 0).
 * stats: NULL or [wtpse_conv_stats_blocks(B,H,W)][Cout][2] per-workgroup (sum, sum^2) of the output (train-mode
 * BatchNorm statistics, algorithms.py:883-889); not combinable with relu_out.
 * mask_ref: NULL or [B][Cout][H][W]: out = mask_ref > 0 ? value : 0 (the ReLU backward of the layer below, fused into
 * its data gradient; not combinable with a split).
 * out_amax: NULL or the amax table (see wtpse_amax; ZERO on entry) of the stored output — what an x2h consumer scales this tensor by
 * when no train-mode BatchNorm sits in between (see wtpse_x3_terms); not combinable with mask_ref.
 * The data gradient is this same call on dY with the `wd` layout. */
int wtpse_conv_fwd(const float* in0, int C0, const float* in1, int C1, const float* wpacked, const float* bias,
                   const float* pro0, const float* pro1, int pro_relu, float* out0, float* out1, int Csplit, float* stats,
                   int B, int H, int W, int Cout, int ksize, int relu_out, const float* mask_ref, unsigned* out_amax, void* stream);
int wtpse_conv_stats_blocks(int B, int H, int W);
/* 3x3 convolution with exactly 16 output channels (DeepWT, algorithms.py:1091-1117) that also emits the per-tile partial
 * Grams of its output in the epilogue: gram_partial [wtpse_conv_stats_blocks(B,H,W)][256] = the WT loss's `partial` layout
 * with S = tiles per image (wtpse_wt_loss_fwd_partials), so that compute_whitening_loss never re-reads z from HBM.
 * relu_out must be 0 (the Gram describes the stored map: the epilogue works on the pre-activation accumulators). */
int wtpse_conv_fwd_gram(const float* in0, int C0, const float* wpacked, const float* bias, const float* pro0, int pro_relu,
                        float* out0, float* gram_partial, int B, int H, int W, int Cout, int relu_out, unsigned* out_amax,
                        void* stream);

/* The same convolution on the BF16 matrix cores at fp32 accuracy (csrc/conv_x3.hip): every fp32 operand is split into three
 * bf16 terms and the product formed from the six leading cross terms with fp32 accumulation (6 bf16 MFMAs instead of 8 fp32
 * MFMAs per 32x32x16 block).  Same contract as wtpse_conv_fwd; requires Cout > 16 and ceil16(C0 + C1) <= 256 (<= 512 when
 * the launch uses 64-channel row blocks: Cout % 64 == 0 and at least 512 of them) — the per-channel prologue coefficients are
 * staged in LDS; anything else fails with WTPSE_ERR_ARG.  `wpacked`: the weights pre-split by
 * wtpse_pack_conv_weights_x3 — desc as for wtpse_pack_conv_weights with offsets {xf_off, xd_off} in unsigned shorts; per
 * conv and direction 32 + ceil16(K) * ceil32(rows) * taps * 3 unsigned shorts (forward: rows = Cout, K = Cin; data gradient:
 * rows = Cin, K = Cout): a 64-byte header (float {1 / scale, scale, 0, 0, 12 words of the packer's scratch}: the layer's
 * power-of-two weight scale, 1 unless wtpse_x3_terms() == 2), then [K chunk 16][row block 32][tap][term slot 3][k half 2][row 32][8 k]. */
int wtpse_conv_x3_stats_blocks(int B, int H, int W, int Cout, int ksize);   /* rows of `stats` for wtpse_conv_fwd_x3 (the tiling depends on the kernel size) */
/* Which 3x3 launches of the x3 entry points run conv_x3r_k (weights fed from registers, input tile double-buffered in LDS) instead
 * of conv_x3_k (weights staged through LDS): on = 1 (default) the launches with 64-channel output blocks, 2 all of them, 0 none;
 * on < 0 only queries (environment: WTPSE_X3R=0|1|2).  Returns the previous setting.  The two kernels give bitwise the same
 * results (tests/test_conv_x3_gpu.py::test_x3r_equals_x3); the choice is by measurement (profiles/r04_microbench_x3.txt). */
int wtpse_x3r_enable(int on);
/* Order in which the workgroups of the x3 convolutions take their (tile, output-channel block) pairs: on = 1 (default) XCD-aware —
 * the hardware deals consecutive workgroups to the 8 XCDs in turn; each XCD is given a contiguous range of tiles and runs a tile's
 * output-channel blocks back to back, so that a tile's input (and the halo it shares with its neighbours) is fetched into ONE L2
 * once; 0 = dispatch order (tile fastest); on < 0 only queries (environment: WTPSE_X3_XCD=0|1).  Returns the previous setting.
 * Same workgroups, bitwise the same results (tests/test_conv_x3_gpu.py::test_xcd_order_equals_dispatch_order). */
int wtpse_x3_xcd(int on);
/* Tiling of the 32-channel-block launches on maps wider than 16 pixels: on = 1: 128-pixel (32 x 4) tiles — twice as many, half as long
 * workgroups, five resident per CU instead of four — on = 0 (default until measured otherwise): 256-pixel (32 x 8) tiles; on < 0 only
 * queries (environment: WTPSE_X3_SMALL_WIDE=0|1).  Returns the previous setting.  Changes the rows of `stats`
 * (wtpse_conv_x3_stats_blocks follows it) and is part of wtpse_tuning_state(). */
int wtpse_x3_small_wide(int on);
/* Arithmetic of the x3 kernels (wtpse_conv_fwd_x3 and the data gradients on it, wtpse_conv_wgrad_r), by the number of 16-bit terms
 * an fp32 operand is split into:
 *   3 = "x3": three bf16 terms, six MFMA products per multiply (round 2);
 *   2 = "x2h" (default since round 5): TWO fp16 terms (11 + 11 significant bits, each rounded to nearest even, the remainder exact
 *       in fp32), THREE products a0 b1 + a1 b0 + a0 b0 on v_mfma_f32_*_f16, fp32 accumulation — half the MFMAs of x3 at the same
 *       measured accuracy (tests/test_conv_x3_gpu.py: against fp64 beside x3 and the fp32-input MFMA).  fp16 has 5 exponent bits, so
 *       every operand tensor is multiplied by a power of two as it is loaded (exact) and the result scaled back: weights per layer
 *       (from the layer's largest magnitude, found by wtpse_pack_conv_weights_x3); an input tensor by the power of two that brings
 *       `in_amax` — an amax table (wtpse_amax below) holding a bound of the largest magnitude of the input AS LOADED, i.e. after the
 *       prologue — into [2^14, 2^15): full 22-bit precision for every element down to 2^-17 of the bound, an absolute error of 2^-39
 *       of the bound below that.  For a GRADIENT the table is left by the tensor's producer (wtpse_bn_bwd_apply_coef,
 *       wtpse_upsample2x_bwd[_bn], ...) or by wtpse_amax.  For a FORWARD ACTIVATION (round 6) it is left by whoever knows a bound:
 *       the train-mode BatchNorm finalize (wtpse_bn_finalize / wtpse_conv_fwd_bnf, `act_amax`: |gamma| sqrt(N - 1) + |beta| per
 *       channel by Samuelson's inequality — no look at the data), the producing convolution's epilogue (`out_amax`: un-normalised
 *       maps), wtpse_act_bound (an eval-mode BatchNorm or any per-channel affine map over a tensor of known amax) or wtpse_amax.
 *       A concat has one table per half (in_amax / in_amax1: the larger counts).  No table at all (NULL): the fixed scale 2^2 of
 *       round 5 — full precision only for 2^-5 <= |x| < 2^14, NaN beyond: right for O(1) data, a fallback for bare callers only
 *       (wtpse_hip/nn.py always passes tables).  Non-finite values: a NaN or inf operand makes every output it feeds NaN (the fp16
 *       terms of an inf are (inf, NaN): an inf does not stay an inf as it can in fp32); forward launches store a NaN accumulator as
 *       NaN, with or without an output ReLU, as torch's conv / ReLU do (the data gradients' epilogues clamp with v_max_f32, which
 *       turns NaN into the clamp bound: -inf or 0 — non-finite, or masked, either way).  A consumer's ReLU-ON-LOAD is v_max_f32 too and
 *       maps NaN to 0 where torch.relu keeps it: a NaN stays loud through BatchNorm statistics (its whole channel turns NaN) and through
 *       un-activated paths (the heads' outputs, mu, the logits), not through an activation;
 *   1 = the `bf16` mode of BASELINE.json configs[1]: operands rounded to ONE bf16 term, one product — outside the 1e-4 parity bar by
 *       construction (tests/test_bf16_mode_gpu.py states its tolerance).
 * The weight gradients of the 16-pixel-wide maps (wtpse_conv_wgrad_x3) stay on x3.  Packed weights are in the format of the setting
 * at the time they were packed: re-pack after a change (wtpse_hip/nn.py does).  Environment: WTPSE_X3_TERMS=1|2|3.  Other values only
 * query; returns the previous setting.  A recorded launch plan (wtpse_plan_*) remembers the setting it was recorded under and
 * refuses to replay under another one. */
int wtpse_x3_terms(int terms);
/* An "amax table" carries the largest magnitude of a gradient tensor from its producer to the x2h kernels that consume it: 1024
 * unsigneds (4 KB, 16-byte aligned) holding float bits of non-negative values in 64 shards, one per 64-byte line (waves / workgroups
 * fold their maximum into shard (index % 64) with one no-return atomic max; consumers take the maximum over the shards).  Producers with an `amax` argument
 * (wtpse_bn_bwd*, wtpse_upsample2x_bwd*) fill the table of the gradient they write when amax != NULL: the table must be ZERO on entry.
 * wtpse_amax zeroes and fills the table of an existing tensor (one extra pass: the slow way). */
int wtpse_amax(const float* x, long long n, unsigned* amax_table, void* stream);
int wtpse_pack_conv_weights_x3(const float* params, const int* desc, int n_desc, unsigned short* packed, void* stream);
int wtpse_conv_fwd_x3(const float* in0, int C0, const float* in1, int C1, const unsigned short* wpacked, const float* bias,
                      const float* pro0, const float* pro1, int pro_relu, float* out0, float* out1, int Csplit, float* stats,
                      int B, int H, int W, int Cout, int ksize, int relu_out, const float* mask_ref, const unsigned* in_amax,
                      const unsigned* in_amax1, unsigned* out_amax, void* stream);      /* in_amax / in_amax1 / out_amax: wtpse_x3_terms, wtpse_conv_fwd */

/* The 16-channel 3x3 layers (inc, DeepWT, the teacher's inc: algorithms.py:897-917,1091-1117,398-413) on v_mfma_f32_16x16x32_* with
 * register-resident weight fragments (csrc/conv.hip, MODE 3 / 4): Cout <= 16, C0 <= 16, one input.  wx16: the layer's fragments
 * (forward or data-gradient direction) from wtpse_pack_conv16_x3, 12808 unsigned shorts per direction (a 16-byte header with the
 * x2h weight scale, the x3 fragments, the x2h fragments), 16-byte aligned.  Arithmetic: wtpse_x3_terms() — x2h when it is 2, except
 * that a GRADIENT input (in_is_grad != 0) without its amax table (in_amax == NULL) runs in x3 (no scale is known for it and a pass
 * to find one costs more than this HBM-bound kernel would gain); in_is_grad == 0: a forward activation, scaled from in_amax (its
 * bound as loaded; NULL: 2^2).  out_amax: as wtpse_conv_fwd.
 * Options as wtpse_conv_fwd (bias, prologue, relu_out, stats [wtpse_conv_stats_blocks][Cout][2], mask_ref) plus gram_partial
 * (as wtpse_conv_fwd_gram; Cout == 16, relu_out == 0) and — with bn_mean — the BatchNorm-backward epilogue of wtpse_dgrad_bnb
 * over all output channels (mask_ref = that layer's raw conv output, stats = its partials). */
int wtpse_conv16_x3(const float* in0, int C0, const unsigned short* wx16, const float* bias, const float* pro0, int pro_relu,
                    float* out0, float* stats, float* gram_partial, const float* mask_ref, const float* bn_ss,
                    const float* bn_mean, int bn_relu, int B, int H, int W, int Cout, int relu_out, int in_is_grad,
                    const unsigned* in_amax, unsigned* out_amax, void* stream);
/* desc: n_desc x 8 ints {w_off, Cout, Cin, 9, fwd_off (-1: none), dgrad_off (-1: none), 0, 0}; w_off in floats, *_off in
 * unsigned shorts (multiples of 8). */
int wtpse_pack_conv16_x3(const float* params, const int* desc, int n_desc, unsigned short* packed, void* stream);

/* A data gradient (= wtpse_conv_fwd / wtpse_conv_fwd_x3 on dY with the `wd` / x3 data-gradient layout: C = the conv's output
 * channels, Cout = its input channels) that also performs the FIRST HALF of the BatchNorm backward of the conv + BatchNorm
 * (+ReLU) layer the gradient flows into (autograd of algorithms.py:883-889,904-917): output channels [bn_c0, bn_c1) — all of
 * them, or exactly one side of the Csplit split — are masked with the ReLU of that layer (bn_relu: [fmaf(bn_y, scale, shift)
 * > 0], bn_ss [Cbn][2], bn_y [B][Cbn][H][W] = its raw conv output, Cbn = bn_c1 - bn_c0) and the per-workgroup partials
 * (sum g, sum g * (bn_y - bn_mean)) are written to stats [wtpse_conv_stats_blocks | wtpse_conv_x3_stats_blocks][Cbn][2]:
 * wtpse_bn_bwd_from_stats finishes the BatchNorm backward without re-reading the two tensors for the reductions.
 * bn_c0, bn_c1 multiples of 16 (bn_c1 may equal Cout). */
int wtpse_dgrad_bnb(const float* dy, int C, const float* wpacked, float* out0, float* out1, int Csplit, const float* bn_y,
                    const float* bn_ss, const float* bn_mean, int bn_relu, int bn_c0, int bn_c1, float* stats, int B, int H, int W,
                    int Cout, int ksize, void* stream);
int wtpse_dgrad_x3_bnb(const float* dy, int C, const unsigned short* wpacked, float* out0, float* out1, int Csplit,
                       const float* bn_y, const float* bn_ss, const float* bn_mean, int bn_relu, int bn_c0, int bn_c1, float* stats,
                       int B, int H, int W, int Cout, int ksize, const unsigned* in_amax, void* stream);

/* A forward convolution in front of a train-mode BatchNorm (algorithms.py:883-889: conv -> bn) whose launch forms the
 * (sum, sum^2) partials of its output in `stats` AND finishes them — wtpse_bn_finalize's work, done by the workgroups that arrive
 * last (two levels of tickets, fixed fold order: bitwise reproducible; see wtpse_dgrad_bnb_coef below for partial2 / tickets,
 * sized with the same two queries).  layout: 0 = wtpse_conv_fwd (fp32 `wf`), 1 = wtpse_conv_fwd_x3, 2 = wtpse_conv16_x3's
 * fragments (one input).  No split, mask or ReLU output: the BatchNorm follows.  in_amax0 / in_amax1: the x2h input bounds of in0 /
 * in1 (layouts 1, 2; NULL: none); act_amax: NULL or the amax table (ZERO on entry) that receives the bound of the BatchNorm's
 * activated output, max_c |gamma_c| sqrt(B H W - 1) + |beta_c| (wtpse_x3_terms: the scale its x2h consumers load it with). */
int wtpse_conv_fwd_bnf(const float* in0, int C0, const float* in1, int C1, const void* wpacked, int layout, const float* bias,
                       const float* pro0, const float* pro1, int pro_relu, float* out0, float* stats, const float* gamma,
                       const float* beta, float* running_mean, float* running_var, long long* num_batches, float momentum, float eps,
                       float* scale_shift, float* save_mean, float* save_invstd, double* partial2, unsigned* tickets, int B, int H,
                       int W, int Cout, int ksize, const unsigned* in_amax0, const unsigned* in_amax1, unsigned* act_amax, void* stream);

/* The same launches, which then ALSO finish the statistics: groups of 64 workgroups fold their partials as their last member
 * arrives, the last group of an output-channel block folds the group sums (fixed order: bitwise reproducible, nobody waits) and
 * writes coef [Cbn][3] = (k1, k2, k3) and dgamma / dbeta (+)= (accumulate) of the BatchNorm'd channels — what
 * wtpse_bn_bwd_from_stats does in its first launch.  wtpse_bn_bwd_apply_coef is then the whole rest of the BatchNorm backward.
 * (Launches of more than 8192 workgroups — WTPSE_TAIL_MAX_WGS; 2048 until round 6 — run that fold as a second launch inside the call instead: the
 * hand-off costs every workgroup ~2.5 us of lifetime, which beats a 6 us launch only where a CU sees few workgroups.)
 * layout: 0 = wtpse_dgrad_bnb (fp32 `wd`), 1 = wtpse_dgrad_x3_bnb, 2 = wtpse_conv16_x3's fragments (Csplit == Cout, all channels).
 * gamma / invstd: of the BatchNorm'd channels.  partial2: wtpse_bnb_tail_partial2(nblk, Cout) doubles of scratch; tickets:
 * wtpse_bnb_tail_tickets(nblk, Cout) unsigneds, ZERO on entry and zero again when the launch has finished (nblk = rows of stats);
 * two launches that may overlap must not share them. */
int wtpse_bnb_tail_partial2(int nblk, int Cout);
int wtpse_bnb_tail_tickets(int nblk, int Cout);
int wtpse_dgrad_bnb_coef(const float* dy, int C, const void* wpacked, int layout, float* out0, float* out1, int Csplit,
                         const float* bn_y, const float* bn_ss, const float* bn_mean, int bn_relu, int bn_c0, int bn_c1,
                         float* stats, const float* gamma, const float* invstd, float* coef, float* dgamma, float* dbeta,
                         int accumulate, double* partial2, unsigned* tickets, int B, int H, int W, int Cout, int ksize,
                         const unsigned* in_amax, void* stream);      /* in_amax: of dy, used by layout 1 (see wtpse_x3_terms) */
/* The same into a BatchNorm on frozen statistics (see wtpse_bn_bwd_frozen below): bn_mean / invstd = the running mean and
 * 1 / sqrt(running_var + eps); the tail leaves coef = (k1, 0, 0) and also writes dbias [Cbn] (+)=, the gradient of the bias of the
 * convolution in front of that BatchNorm. */
int wtpse_dgrad_bnb_coef_frozen(const float* dy, int C, const void* wpacked, int layout, float* out0, float* out1, int Csplit,
                                const float* bn_y, const float* bn_ss, const float* bn_mean, int bn_relu, int bn_c0, int bn_c1,
                                float* stats, const float* gamma, const float* invstd, float* coef, float* dgamma, float* dbeta,
                                float* dbias, int accumulate, double* partial2, unsigned* tickets, int B, int H, int W, int Cout,
                                int ksize, const unsigned* in_amax, void* stream);

/* dW[Cout][C0+C1][k][k] (+)= sum dY * X, dbias (+)= sum dY (dbias/dbias_slab NULL: skip).  slab: [ksplit][Cout*Cin*k*k],
 * dbias_slab: [ksplit][Cout], ksplit = wtpse_wgrad_ksplit(...).  x inputs take the same prologue as the forward. */
int wtpse_conv_wgrad(const float* dy, const float* x0, int C0, const float* x1, int C1, const float* pro0,
                     const float* pro1, int pro_relu, float* slab, float* dbias_slab, int ksplit, float* dw, float* dbias, int accumulate, int B, int H,
                     int W, int Cout, int ksize, void* stream);
int wtpse_wgrad_ksplit(int B, int H, int W, int Cin, int Cout);
/* The weight gradient in the x3 arithmetic of wtpse_conv_fwd_x3 (csrc/conv_x3.hip: dY and X kept pixel-major in LDS as bf16
 * triples, fragments fetched with the transposing LDS read).  3x3 convs with Cin, Cout multiples of 32 (C0 % 8 == 0 for a
 * concat): wtpse_wgrad_x3_supported().  No bias gradient (the conv+BatchNorm layers it serves have none).
 * slab: [ksplit][Cout*Cin*9], ksplit = wtpse_wgrad_x3_ksplit(...). */
int wtpse_wgrad_x3_supported(int Cin, int Cout, int ksize, int C0);
int wtpse_wgrad_x3_ksplit(int B, int H, int W, int Cin, int Cout);
int wtpse_conv_wgrad_x3(const float* dy, const float* x0, int C0, const float* x1, int C1, const float* pro0,
                        const float* pro1, int pro_relu, float* slab, int ksplit, float* dw, int accumulate, int B, int H, int W,
                        int Cout, int ksize, void* stream);

/* The 3x3 weight gradient in the x3 arithmetic with register-resident operands (csrc/wgrad_r.hip: every lane loads its own
 * 8-pixel fragments from global memory, splits them into bf16 triples and feeds v_mfma_f32_16x16x32_bf16 from registers; the
 * horizontal taps are lane shifts, the vertical ones a 3-row ring of registers; no LDS in the main loop).  Maps whose width is a
 * multiple of 32, Cin / Cout multiples of 16 (C0 % 16 == 0 for a concat) — or exactly 16 wide with Cin / Cout multiples of 32 (two images
 * side by side per 32-pixel step; no bias gradient, not the _bn form) —: wtpse_wgrad_r_supported().  With bias gradient
 * (dbias / dbias_slab NULL: skip).  slab: [nslab][Cout*Cin*9], dbias_slab: [nslab][Cout], nslab = wtpse_wgrad_r_slabs(...).
 * Arithmetic by wtpse_x3_terms(); with 2 (x2h) dY is scaled from dy_amax (NULL: like a forward activation — and the 16 x 16-channel
 * blocks, HBM-bound, then stay on x3), X from x_amax0 / x_amax1 (the bounds of x0 / x1 as loaded; both NULL: 2^2); the _bn form below
 * stays on three bf16 terms.  With 1 (bf16 mode) only the blocks of
 * 32 channels on at least one side run with one term: the 16 x 16 blocks (which alone carry a bias gradient), the _bn form and
 * wtpse_conv_wgrad_x3 keep three — the mode is a mix of arithmetics by design (the 16-channel layers are not MFMA-bound). */
int wtpse_wgrad_r_supported(int Cin, int Cout, int ksize, int C0, int W);
int wtpse_wgrad_r_slabs(int B, int H, int W, int Cin, int Cout);
int wtpse_conv_wgrad_r(const float* dy, const float* x0, int C0, const float* x1, int C1, const float* pro0,
                       const float* pro1, int pro_relu, float* slab, float* dbias_slab, int nslab, float* dw, float* dbias,
                       int accumulate, int B, int H, int W, int Cout, const unsigned* dy_amax, const unsigned* x_amax0,
                       const unsigned* x_amax1, void* stream);    /* *_amax: wtpse_x3_terms */

/* wtpse_conv_wgrad_r with dY given as the un-applied second half of a BatchNorm backward (wtpse_bn_bwd_coef):
 * dY = k1[c] * g + k2[c] * bn_y + k3[c], bn_coef [Cout][3] = (k1, k2, k3): the BatchNorm-apply pass of the backward
 * (read g, read y, write dY) never runs, the kernel forms dY from the two tensors as it loads its A fragments. */
int wtpse_conv_wgrad_r_bn(const float* g, const float* bn_y, const float* bn_coef, const float* x0, int C0, const float* x1,
                          int C1, const float* pro0, const float* pro1, int pro_relu, float* slab, int nslab, float* dw,
                          int accumulate, int B, int H, int W, int Cout, void* stream);

/* ---- BatchNorm2d, eps 1e-5, momentum 0.1 (algorithms.py:862-864) ---------------------------------------------- */
/* train mode: fold the conv epilogue's partials -> scale_shift[C][2], save_mean/invstd[C]; update running stats
 * (unbiased variance) and num_batches_tracked (int64) when given.  act_amax: as wtpse_conv_fwd_bnf (NULL: none). */
int wtpse_bn_finalize(const float* stats_partial, int nblk, int C, long long count, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, long long* num_batches, float momentum, float eps,
                      float* scale_shift, float* save_mean, float* save_invstd, unsigned* act_amax, void* stream);
/* eval mode on TARGET statistics (wtpse_hip/adapt.py holds the float64 specification): fold the partials of this call (count values
 * per channel), pool them with acc [C][2] = (sum, sum^2) over the acc_count values of earlier calls (NULL / 0: no history; with acc,
 * the pooled sums are left there), blend mean and biased variance with the running ones at weight w in [0, 1] (w = 1: the target's
 * alone) -> scale_shift [C][2].  Optional: moments [C][4] = (mean_t, var_t, mean_b, var_b), div [C] = KL(N_t || N_s), act_amax (ZERO on
 * entry) = twice the Samuelson bound of |scale y + shift| over this call.  The running buffers are read, never written. */
int wtpse_bn_finalize_blend(const float* stats_partial, int nblk, int C, long long count, const float* gamma, const float* beta,
                            const float* running_mean, const float* running_var, double w, float eps, double* acc, double acc_count,
                            float* scale_shift, double* moments, double* div, unsigned* act_amax, void* stream);
/* act_amax (the WHOLE table is written: it need not be zero) = bound of |scale_shift[c][0] * y + scale_shift[c][1]| over a tensor y whose
 * amax table is raw_amax: max_c |scale| * amax + |shift| — the x2h input bound of an activation behind an eval-mode BatchNorm. */
int wtpse_act_bound(const float* scale_shift, int C, const unsigned* raw_amax, unsigned* act_amax, void* stream);
/* eval mode: scale_shift from the running statistics. */
int wtpse_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                         float eps, int C, float* scale_shift, void* stream);
/* z = act(y * scale + shift), materialised (scale_shift NULL: identity). */
int wtpse_affine_act(const float* y, const float* scale_shift, int relu, float* z, int B, int C, int HW, void* stream);
/* dz (grad wrt z = act(bn(y))) -> dgamma, dbeta, dy.  partial: [wtpse_bn_bwd_nsplit][C][2], coef: [C][3]. */
int wtpse_bn_bwd(const float* dz, const float* y, const float* scale_shift, int relu, const float* gamma,
                 const float* save_mean, const float* save_invstd, float* partial, float* coef, float* dgamma,
                 float* dbeta, int accumulate, float* dy, int B, int C, int HW, unsigned* amax, void* stream);
int wtpse_bn_bwd_nsplit(int B, int C, int HW);
/* Synchronised BatchNorm (data parallel, statistics over the global batch): the backward in two halves around the
 * caller's all-reduce of sums[C][2].  dgamma/dbeta receive this rank's share; dy uses the global sums and count. */
int wtpse_bn_bwd_reduce(const float* dz, const float* y, const float* scale_shift, int relu, const float* save_mean,
                        const float* save_invstd, float* partial, float* sums_local, int B, int C, int HW, void* stream);
int wtpse_bn_bwd_apply(const float* dz, const float* y, const float* scale_shift, int relu, const float* gamma,
                       const float* save_mean, const float* save_invstd, const float* sums_local, const float* sums_global,
                       long long count_global, float* coef, float* dgamma, float* dbeta, int accumulate, float* dy, int B,
                       int C, int HW, unsigned* amax, void* stream);
/* second half of a BatchNorm backward whose reductions came out of a data gradient's epilogue (wtpse_dgrad_bnb /
 * wtpse_dgrad_x3_bnb): g = the already-masked incoming gradient, stats_partial [nblk][C][2] = (sum g, sum g * (y - mean))
 * per workgroup; dgamma / dbeta (+)=, dy = k1 * g + k2 * y + k3.  coef: [C][3] scratch. */
int wtpse_bn_bwd_from_stats(const float* g, const float* y, const float* stats_partial, int nblk, const float* gamma,
                            const float* save_mean, const float* save_invstd, float* coef, float* dgamma, float* dbeta,
                            int accumulate, float* dy, int B, int C, int HW, unsigned* amax, void* stream);

/* partials [nblk][C][2] = (sum g, sum g (y - mean)) -> coef [C][3], dgamma / dbeta (+)=: the first launch of
 * wtpse_bn_bwd_from_stats on its own. */
int wtpse_bn_bwd_finalize_coef(const float* stats_partial, int nblk, int C, long long count, const float* gamma,
                               const float* save_mean, const float* save_invstd, float* coef, float* dgamma, float* dbeta,
                               int accumulate, void* stream);
/* dy = k1 * g + k2 * y + k3 with coef [C][3] from wtpse_dgrad_bnb_coef. */
int wtpse_bn_bwd_apply_coef(const float* g, const float* y, const float* coef, float* dy, int B, int C, int HW, unsigned* amax, void* stream);

/* ---- backward through an EVAL-mode BatchNorm ("frozen" statistics: module.eval() followed by update() and backward(),
 *      algorithms.py:1238, shape_networks.py:524-526 — the module mode changes nothing but BatchNorm) ---------------------------
 * z = act(s y + beta - s m) with s = gamma r, m = running_mean, r = 1 / sqrt(running_var + eps); g = dz [z > 0]:
 *   dy = s g,  dbeta = sum g,  dgamma = r sum g (y - m),  d(bias of the conv in front) = s sum g.
 * The entry points below are the train-mode ones above with mean / invstd = m / r: the same partials, the same fixed-order fp64
 * folds (no float atomics: two runs agree bitwise), the two terms through the batch statistics dropped (coef = (k1, 0, 0), so the
 * consumers that form dy on load — wtpse_upsample2x_bwd_bn, wtpse_conv_wgrad_r_bn — take it as it is) and `dbias` [C] written (+)=.
 * The partials of wtpse_dgrad_bnb / wtpse_dgrad_x3_bnb / wtpse_conv16_x3 / wtpse_maxpool2_bwd_bnb are formed with mean = m.
 * A gradient that is written fills its amax table (ZERO on entry) as wtpse_bn_bwd_apply_coef does. */
/* wtpse_bn_eval_coeffs that also emits (m, r): what the backward takes in place of the saved batch statistics.  scale_shift has
 * the bits wtpse_bn_eval_coeffs gives. */
int wtpse_bn_eval_coeffs_stats(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                               float eps, int C, float* scale_shift, float* save_mean, float* save_invstd, void* stream);
/* wtpse_bn_bwd: dz -> dgamma, dbeta, dbias, dy = k1 * dz [z > 0] (the fp32 product).  partial, coef: as there. */
int wtpse_bn_bwd_frozen(const float* dz, const float* y, const float* scale_shift, int relu, const float* gamma,
                        const float* mean, const float* invstd, float* partial, float* coef, float* dgamma, float* dbeta,
                        float* dbias, int accumulate, float* dy, int B, int C, int HW, unsigned* amax, void* stream);
/* wtpse_bn_bwd_from_stats: g already masked, stats_partial [nblk][C][2] = (sum g, sum g (y - m)); y is not needed: dy = k1 * g. */
int wtpse_bn_bwd_from_stats_frozen(const float* g, const float* stats_partial, int nblk, const float* gamma, const float* invstd,
                                   float* coef, float* dgamma, float* dbeta, float* dbias, int accumulate, float* dy, int B, int C,
                                   int HW, unsigned* amax, void* stream);
/* wtpse_bn_bwd_finalize_coef: the fold alone -> coef = (k1, 0, 0), dgamma / dbeta / dbias (+)=. */
int wtpse_bn_bwd_finalize_coef_frozen(const float* stats_partial, int nblk, int C, const float* gamma, const float* invstd,
                                      float* coef, float* dgamma, float* dbeta, float* dbias, int accumulate, void* stream);
/* wtpse_bn_bwd_apply_coef for such a coef: dy = k1 * g, a third less traffic (y is not read). */
int wtpse_bn_bwd_scale_coef(const float* g, const float* coef, float* dy, int B, int C, int HW, unsigned* amax, void* stream);

/* ---- WT (whitening) loss: compute_whitening_loss + compute_MMD (algorithms.py:1277-1309,59-121;
 *      shape_networks.py:561-594,240-309) ------------------------------------------------------------------------ */
/* z [B,16,HW] -> gram[B][256] (incl. eps*I), v[B][120], offdiag[B], diag[B], rowval[D*n + 1] (fp64; the extra element is
 * an 8-byte ticket word of the launch that merges the MMD rows with the final sums), dmmd_dv[D*n][120],
 * losses[3] = {ins_offdiag, ins_diag, domain}.  partial: [B * wtpse_wt_split(B,HW,&chunk)][256]. */
int wtpse_wt_loss_fwd(const float* z, int B, int C, int HW, float eps, float margin, int domain_num, int per_domain,
                      float* partial, float* gram, float* v, float* offdiag, float* diag, double* rowval,
                      float* dmmd_dv, float* losses, void* stream);
int wtpse_wt_split(int B, int HW, int* chunk_out);
/* The same loss from partial Grams [B][S][256] that a conv epilogue already produced (wtpse_conv_fwd_gram): z is not read. */
int wtpse_wt_loss_fwd_partials(const float* partial, int S, int B, int HW, float eps, float margin, int domain_num,
                               int per_domain, float* gram, float* v, float* offdiag, float* diag, double* rowval,
                               float* dmmd_dv, float* losses, void* stream);
/* The two halves of wtpse_wt_loss_fwd (data parallel: all-gather of v and wtpse_mmd_fwd on the global rows in between).
 * wtpse_wt_final: losses[0..1] = this rank's share of the instance means (divided by Bnorm), losses[2] = sum(rowval). */
int wtpse_wt_gram_fwd(const float* z, int B, int C, int HW, float eps, float* partial, float* gram, float* v, float* offdiag,
                      float* diag, void* stream);
int wtpse_wt_final(const float* offdiag, const float* diag, int B, int Bnorm, float margin, const double* rowval, int R,
                   float* losses, void* stream);
/* dz (+)= d(w_off*g_off*ins_off + w_diag*g_diag*ins_diag + w_dom*g_dom*dom)/dz.  g_*: device scalars (NULL = 1).
 * Mws: [B][256] scratch.  accumulate & 1: add to dz; accumulate & 2 (with & 1): the incoming dz is a gradient wrt relu(z) and is
 * masked with [z > 0] first (the teacher reads relu(z2): algorithms.py:1066) — z is in registers here anyway. */
int wtpse_wt_loss_bwd(const float* z, int B, int C, int HW, float margin, int domain_num, int per_domain,
                      const float* gram, const float* offdiag, const float* diag, const float* dmmd_dv,
                      const float* g_off, const float* g_diag, const float* g_dom, float w_off, float w_diag, float w_dom,
                      float* Mws, float* dz, int accumulate, void* stream);
/* Fold per-map losses [nmaps][3] into out[4] = (ins_total, ins_off, ins_diag, dom) with the reference's quirks:
 * mode 0 = WT_PSE.update (algorithms.py:1259-1267), mode 1 = student incl. accumulator overwrite (shape_networks.py:546-548). */
int wtpse_wt_combine(const float* losses, int nmaps, float den, int mode, float* out, void* stream);
/* MMD alone on v [D*n][120] (data-parallel: after the all-gather of v). sum(rowval) is the loss. */
int wtpse_mmd_fwd(const float* v, int domain_num, int per_domain, double* rowval, float* dmmd_dv, void* stream);

/* ---- pooling / upsampling (algorithms.py:890,901,929,949) ------------------------------------------------------- */
int wtpse_maxpool2_fwd(const float* x, const float* pro, int relu, float* out, int B, int C, int H, int W, void* stream);
/* accumulate & 1: dx += ; accumulate & 2: the result (after the add) is masked with [act(x) > 0], act = the prologue as loaded —
 * the backward of the ReLU that produced x (algorithms.py:1068-1069: fusion conv -> ReLU -> U-Net), fused. */
int wtpse_maxpool2_bwd(const float* x, const float* pro, int relu, const float* dout, float* dx, int accumulate, int B,
                       int C, int H, int W, void* stream);
/* wtpse_maxpool2_bwd(accumulate | 2) where x is the raw output of a conv + BatchNorm + ReLU layer (pro = its scale/shift): the
 * result is the masked gradient wrt that layer's activated output, and the launch also forms the two reductions of its BatchNorm
 * backward: stats [wtpse_maxpool2_bwd_stats_blocks(B,H,W)][C][2] = (sum g, sum g (y - mean)) partials, the layout
 * wtpse_bn_bwd_from_stats folds.  H even, W % 4 == 0, 16-byte aligned tensors, B*C < 32768. */
int wtpse_maxpool2_bwd_stats_blocks(int B, int H, int W);
int wtpse_maxpool2_bwd_bnb(const float* x, const float* pro, int relu, const float* dout, float* dx, int accumulate,
                           const float* mean, float* stats, int B, int C, int H, int W, void* stream);
/* bilinear x2, align_corners=False; H, W are the INPUT sizes. */
int wtpse_upsample2x_fwd(const float* x, const float* pro, int relu, float* out, int B, int C, int H, int W, void* stream);
int wtpse_upsample2x_bwd(const float* dout, float* dx, int accumulate, int B, int C, int H, int W, unsigned* amax, void* stream);
/* ... of a gradient that is the second half of a BatchNorm backward and never written out: dout = k1[c] * g + k2[c] * bn_y + k3[c],
 * bn_coef [C][3] as wtpse_dgrad_bnb_coef leaves it (the expression of wtpse_bn_bwd_apply_coef, same bits); g, bn_y [B][C][2H][2W].
 * W % 4 == 0, 16-byte aligned tensors. */
int wtpse_upsample2x_bwd_bn(const float* g, const float* bn_y, const float* bn_coef, float* dx, int B, int C, int H, int W,
                            unsigned* amax, void* stream);
/* The same with the train-mode BatchNorm statistics of the OUTPUT: stats [wtpse_upsample2x_stats_blocks(B,H,W)][C][2]
 * per-workgroup (sum, sum of squares), the layout wtpse_bn_finalize takes.  Used where the 1x1 conv of a ConvU block
 * (algorithms.py:949-951: upsample -> conv2 -> bn2) runs in front of the upsampling instead (the two commute). W even. */
int wtpse_upsample2x_fwd_stats(const float* x, float* out, float* stats, int B, int C, int H, int W, void* stream);
int wtpse_upsample2x_stats_blocks(int B, int H, int W);

/* F.interpolate(size=(Ho,Wo), mode="bilinear"), align_corners=False: validation resize of the logits (Trainer.py:206-209). */
int wtpse_resize_bilinear(const float* x, float* out, int B, int C, int H, int W, int Ho, int Wo, void* stream);

/* ---- shape attention + fusion (algorithms.py:1126-1129,1243-1248,1342-1344) ------------------------------------- */
/* att = sigmoid(w*z + b), fuse = coef*emb + att*emb, mask = att > 0.75.  wb: device {w, b}.  att/att_pre/mask optional. */
int wtpse_attn_fuse_fwd(const float* z, const float* wb, const float* emb, float coef, float* att, float* att_pre,
                        float* mask, float* fuse, int B, int CE, int HW, void* stream);
/* partial: [2*ceil(B*HW/256)]; d_wb[2] (+)= (dw, db); dz optional. */
int wtpse_attn_fuse_bwd(const float* dfuse, const float* z, const float* emb, const float* att, const float* wb, float coef,
                        float* demb, float* dz, float* partial, float* d_wb, int accumulate, int B, int CE, int HW,
                        void* stream);

/* ---- sampling (algorithms.py:1068-1075; shape_networks.py:490-510) ----------------------------------------------- */
int wtpse_reparam_fwd(const float* mu, const float* logvar, const float* eps, float* z, long long n, void* stream);
int wtpse_reparam_bwd(const float* dz, const float* logvar, const float* eps, float* dlogvar, long long n, void* stream);
int wtpse_exp_half(const float* logvar, float* std_, long long n, void* stream);
int wtpse_reparam_student(const float* mu, const float* std_, const float* eps, float* z, long long n, void* stream);
/* if any element is NaN: nan_to_num the whole tensor (shape_networks.py:490-492: `if torch.isnan(mu).any(): mu = nan_to_num(mu)`).
 * flag: one device int (scratch).  No host sync. */
int wtpse_nan_scrub(float* x, long long n, int* flag, void* stream);
/* Philox4x32-10 + Box-Muller; element i depends only on (seed, position + i): position = offset + *offset_dev (offset_dev
 * NULL: 0) = global element index, a multiple of 4.  Keeping the running position in device memory lets a captured
 * launch (hipGraph) draw fresh numbers on every replay. */
int wtpse_randn(float* out, long long n, unsigned long long seed, unsigned long long offset,
                const unsigned long long* offset_dev, void* stream);
/* *counter += inc on the stream (int32 counter, or uint64 when is64): step / stream-position counters of captured launches. */
int wtpse_counter_add(void* counter, long long inc, int is64, void* stream);

/* ---- caller-side losses and optimiser (Trainer.py:19,787,842-871; shape_networks.py:596-597; train.py:120-138) --- */
/* `partial` scratch: wtpse_reduce_blocks(n) floats (x2 for wtpse_pos_weight).  g: device scalar upstream gradient or NULL. */
int wtpse_reduce_blocks(long long n);
int wtpse_bce_sigmoid_fwd(const float* x, const float* t, long long n, float* partial, float* loss, void* stream);
int wtpse_bce_sigmoid_bwd(const float* x, const float* t, const float* g, float w, long long n, float* dx, void* stream);
int wtpse_pos_weight(const float* mask, const float* t, long long n, float* partial, float* sums, float* pw, void* stream);
int wtpse_pos_weight_from_sums(const float* sums, float* pw, void* stream);
int wtpse_bce_logits_pw_fwd(const float* x, const float* mask, const float* t, const float* pw, long long n, float* partial,
                            float* loss, void* stream);
int wtpse_bce_logits_pw_bwd(const float* x, const float* mask, const float* t, const float* pw, const float* g, float w,
                            long long n, float* dx, void* stream);
int wtpse_mse_fwd(const float* a, const float* b, long long n, float* partial, float* loss, void* stream);
int wtpse_mse_bwd(const float* a, const float* b, const float* g, float w, long long n, float* da, void* stream);
int wtpse_roi(const float* image, const float* logit, float* roi, float* od_pred, int B, int C, int HW, void* stream);
/* torch.optim.Adam (no weight decay / amsgrad), step number t = step + *step_dev (step_dev NULL: t = step; otherwise a
 * device int holding the number of completed steps, so that a captured launch stays valid when replayed). */
int wtpse_adam(float* p, const float* g, float* m, float* v, long long n, double lr, double beta1, double beta2, double eps,
               int step, const int* step_dev, void* stream);
/* wtpse_adam with the learning rate read from device memory: lr_dev = one device float, so that a schedule can change the rate
 * of a recorded launch between replays (a write on the stream, nothing recorded again).  The same kernel body serves both entry
 * points: for the same float value, p / m / v come out bit-identical to wtpse_adam(..., lr = (double)*lr_dev, ...).
 * hold (NULL: never held): one device int, read once per workgroup; when *hold != 0 the launch changes nothing — p, m, v keep
 * their bits (the NaN flag of wtpse_loss_log: a poisoned loss is not applied to the weights). */
int wtpse_adam_dev(float* p, const float* g, float* m, float* v, long long n, const float* lr_dev, double beta1, double beta2,
                   double eps, int step, const int* step_dev, const int* hold, void* stream);
/* wtpse_adam_dev over an index list: p and g are a network's flat buffers, idx a device int32 [n_idx] of DISTINCT element
 * positions in them (0 <= idx[k] < the buffers' length: the caller's duty, nothing is checked on the device), m and v COMPACT,
 * [n_idx]: element k of them belongs to p[idx[k]].  One thread per index; the arithmetic is wtpse_adam_dev's, statement for
 * statement, so p[idx[k]], m[k], v[k] come out bit-identical to a dense wtpse_adam_dev on the same operands.  Elements of p
 * outside idx are never written; *hold != 0: nothing is.  (Test-time entropy minimisation steps the BatchNorm affines alone:
 * wtpse_hip/tent.py.) */
int wtpse_adam_index(float* p, const float* g, float* m, float* v, const int* idx, int n_idx, const float* lr_dev, double beta1,
                     double beta2, double eps, int step, const int* step_dev, const int* hold, void* stream);
/* Device-side loss log (Trainer.py:788-800, 828-832, 874-885, 917-919): one single-wave launch per update() call of a step.
 * s0..s5: device fp32 scalars (trailing ones may be NULL); for every non-NULL sj: acc[j] += (double)*sj — the reference's
 * `running += loss.item()`, so a double accumulator fed in iteration order holds its running sums bit for bit.
 * NaN test: the first k scalars (s0 always, and all k non-NULL) are added left to right in fp32, the reference's order, and the sum is
 * tested (inf + -inf counts):
 *     check_n   k   sum tested
 *     0         0   none
 *     1         1   s0
 *     17        2   s0 + s1
 *     3, 49     3   (s0 + s1) + s2
 *     19, 35    4   ((s0 + s1) + s2) + s3
 *     51        5   (((s0 + s1) + s2) + s3) + s4
 *     115       6   ((((s0 + s1) + s2) + s3) + s4) + s5
 * The codes are historical names for the count k: both names of k = 3 and of k = 4 are accepted, every other value is refused.
 * flag: two device ints, sticky (never cleared here): when the test holds and flag[0] == 0,
 * flag[0] = 1 and flag[1] = *step_dev (the calling network's count of completed steps = the failing iteration; NULL: 0). */
int wtpse_loss_log(const float* s0, const float* s1, const float* s2, const float* s3, const float* s4, const float* s5,
                   double* acc, int check_n, int* flag, const int* step_dev, void* stream);

/* ---- boundary loss (csrc/boundary.hip; specification: wtpse_hip/boundary.py) ---------------------------------------------
 * wtpse_signed_distance: the signed distance map of B label planes t [B][h][w] fp32 (nonzero = object, as wtpse_seg_metrics takes
 * a label).  Per plane, with pos = {t != 0}: d2_out[p] = min over q in pos of |p - q|^2 and d2_in[p] = min over q outside pos,
 * exact integers (-1 where the set is empty); phi[p] = sqrt(d2_out[p]) outside, 1 - sqrt(d2_in[p]) inside (Kervadec's
 * one_hot2dist: edt(neg) neg - (edt(pos) - 1) pos), and phi = 0 on a plane without a contour (pos empty or everything; recognised
 * on the device).  phi is float32 of the float64 expression, bit for bit.  d2_out / d2_in: int32 [B][h][w] or NULL (not wanted).
 * ws: wtpse_signed_distance_ws(B, h, w) 4-byte words (<= 0: unsupported size; 1 <= h, w <= 4096).  Two launches, no atomics,
 * nothing read by the host: results do not depend on scheduling.
 * wtpse_boundary_loss: *loss = (1/n) sum_i sigmoid(x_i m_i) phi_i (mask NULL: m = 1), block partials (wtpse_reduce_blocks(n)
 * floats) folded in a fixed order; the weight is NOT applied to it.  With dx != NULL the same pass adds the gradient of
 * (*alpha_dev) * loss into dx in place: dx_i += (*alpha_dev) / n * phi_i * s_i (1 - s_i) * m_i.  alpha_dev: one device float (a
 * schedule changes the weight of a recorded call between replays); may be NULL when dx is. */
int wtpse_signed_distance_ws(int B, int h, int w);
int wtpse_signed_distance(const float* t, float* phi, int* d2_out, int* d2_in, void* ws, int B, int h, int w, void* stream);
int wtpse_boundary_loss(const float* x, const float* mask, const float* phi, const float* alpha_dev, long long n, float* partial,
                        float* loss, float* dx, void* stream);

/* ---- overlap loss: soft Dice / Tversky / focal Tversky per image (csrc/overlap.hip; specification: wtpse_hip/overlap.py) ----
 * x, t, mask (NULL: m = 1), dx: [B][hw] fp32, one plane per image.  Per plane, with z = x m and s = sigmoid(z) (fp64):
 *     TP = sum m s t,  FP = sum m s - TP,  FN = sum m t - TP,  TI = (TP + smooth) / (TP + fp FP + fn FN + smooth),
 *     L_b = (1 - TI)^focal, and L_b = 0 with a zero gradient where 1 - TI <= 0 (decided before any power is taken);
 * plane_loss[b] = L_b (fp32 [B], or NULL: not wanted), *loss = mean over b of L_b; the weight is NOT applied to either.
 * With dx != NULL the gradient of (*w_dev) * loss is added into dx in place, in fp64 and rounded once on the add:
 *     dx_i += (*w_dev / B) (-focal (1 - TI)^(focal - 1)) m_i [t_i D - N (t_i + fp (1 - t_i) - fn t_i)] / D^2 s_i (1 - s_i) m_i
 * (N, D: numerator and denominator of TI); an increment of exactly 0 leaves the element's bits alone.  w_dev: one device float
 * (a schedule changes the weight of a recorded call between replays); may be NULL when dx is.  fp, fn >= 0 with fp + fn > 0,
 * focal > 0, smooth > 0 go by value: constants of a run.  ws: wtpse_overlap_loss_ws(B, hw) BYTES, 8-byte aligned (-1: refused
 * shape; 1 <= B < 65536, 1 <= hw <= 2^30, B hw < 2^31).  Three launches: fp64 partial sums per workgroup (the number of
 * workgroups per plane depends on hw alone), the per-plane fold + increment, wtpse_reduce_rows with scale 1 / B.  Fixed order of
 * additions, no atomics: results do not depend on scheduling, nor on a plane's place in the batch or its alignment. */
int wtpse_overlap_loss_ws(int B, int hw);
int wtpse_overlap_loss(const float* x, const float* mask, const float* t, const float* w_dev, int B, int hw, float fp, float fn,
                       float focal, float smooth, void* ws, float* plane_loss, float* loss, float* dx, void* stream);

/* ---- prediction entropy per image and its gradient (csrc/entropy.hip; specification: wtpse_hip/tent.py) ----
 * x, mask (NULL: m = 1), dx: [B][hw] fp32, one plane per image.  Per pixel z = x m, e = exp(-|z|) (fp64):
 *     h(z) = log1p(e) + |z| e / (1 + e)   (the binary entropy of sigmoid(z), in nats),   h'(z) = -z e / (1 + e)^2;
 * per plane M_b = sum m, H_b = (sum m h) / M_b (H_b = 0 where M_b = 0), c_b = [M_b > 0 and H_b < margin] (a NaN plane fails the
 * test), w_b = exp(margin - H_b) when reweight != 0 and margin is finite, else 1 (a constant: no gradient through it).
 *     *loss = (1 / B) sum_b c_b w_b H_b   — the mean over ALL B planes, folded in plane order in fp64, rounded once;
 *     dx_i  = (c_b w_b / (B M_b)) m_i^2 h'(z_i)   — WRITTEN (not added), fp64 rounded once; every element of dx is written and an
 *             unselected plane's are +0.0.  dx may be NULL (value only).
 * planes[b] = H_b (fp32 [B]) and selected[b] = c_b (int32 [B]); either may be NULL.  margin > 0 in nats, +inf allowed (plain TENT;
 * EATA's filter for two classes: 0.4 ln 2).  ws: wtpse_entropy_loss_ws(B, hw) BYTES, 8-byte aligned (-1: refused shape; 1 <= B <
 * 65536, 1 <= hw <= 2^30, B hw < 2^31).  Three launches: fp64 partial sums per workgroup (the number of workgroups per plane
 * depends on hw alone), the per-plane fold + gradient, the fold over the planes.  Fixed order of additions, no atomics: results do
 * not depend on scheduling, nor on a plane's place in the batch, its neighbours or its alignment. */
int wtpse_entropy_loss_ws(int B, int hw);
int wtpse_entropy_loss(const float* x, const float* mask, int B, int hw, double margin, int reweight, void* ws, float* planes,
                       int* selected, float* loss, float* dx, void* stream);

/* ---- Lovász hinge loss per image: a segmented stable sort on the device (csrc/lovasz.hip; specification: wtpse_hip/lovasz.py) ----
 * x, t, mask (NULL: every pixel kept), dx: [B][hw] fp32, one plane per image.  A pixel is kept iff mask == NULL or m_i != 0 (an
 * ignored pixel is out of the set; a kept pixel's logit is x_i itself).  Per plane: sign_i = t_i > 0 ? +1 : -1,
 * e_i = fmaf(-x_i, sign_i, 1) in fp32; the kept pixels ordered by e descending, ties by ascending pixel index; G = kept foreground
 * pixels, c_r = foreground among the first r of the order, and in fp64 from these integers
 *     J_r = 1 - (G - c_r) / (G + r - c_r),  g_1 = J_1,  g_r = J_r - J_{r-1},  L_b = sum_r max(e_(r), 0) g_r   (0 without a kept pixel)
 * plane_loss[b] = L_b (fp32 [B], or NULL: not wanted), *loss = mean over b of L_b; the weight is NOT applied to either.  A kept
 * pixel with a non-finite logit makes L_b NaN, and that plane adds nothing into dx.  ranks (int32 [B][hw], or NULL: not wanted):
 * the 0-based place in its plane's order of every kept pixel with e > 0, -1 elsewhere.  With dx != NULL the gradient of
 * (*w_dev) * loss, the order and g held constant, is added into dx in place, in fp64 and rounded once on the add:
 *     dx_i += (*w_dev / B) (-sign_i) g_rank(i)     for a kept pixel with e_i > 0
 * and no other element is written; an increment of exactly 0 leaves the element's bits alone.  w_dev: one device float (a schedule
 * changes the weight of a recorded call between replays); may be NULL when dx is.  ws: wtpse_lovasz_loss_ws(B, hw) BYTES, 8-byte
 * aligned (-1: refused shape; 1 <= B < 65536, 1 <= hw <= 2^30, B hw < 2^31, and the bytes — about 16 B hw — below 2^31).
 * The sort is an LSD radix sort of (key, pixel) pairs over four 8-bit digits, a plane cut into chunks whose number depends on hw
 * alone; every place comes from digit counts and their prefixes, never from the arrival order of an atomic, so the order is stable
 * and the results do not depend on scheduling, nor on a plane's place in the batch or on B.  Allocates nothing, never synchronises. */
int wtpse_lovasz_loss_ws(int B, int hw);
int wtpse_lovasz_loss(const float* x, const float* mask, const float* t, const float* w_dev, int B, int hw, void* ws,
                      float* plane_loss, int* ranks, float* loss, float* dx, void* stream);

/* ---- weight averaging (csrc/average.hip; specification: wtpse_hip/averaging.py) --------------------------------------
 * wtpse_avg_step folds one iterate into running means, up to four segments (a_s, p_s, n_s) in ONE launch; a segment with
 * n_s == 0 is skipped (its pointers may be NULL).  With k = *count + 1, every element of every segment becomes
 *     a[i] = (k == 1) ? p[i] : a[i] + (p[i] - a[i]) / (float)k
 * in IEEE fp32: subtraction, (correctly rounded) division and addition each rounded to nearest, in that order, nothing
 * contracted; then *count = k.  k == 1 copies: a segment is restarted by zeroing the count alone, whatever the buffers hold.
 * gate (NULL: open) / hold (NULL: never held): one device int each; when *gate == 0 or *hold != 0 neither any a nor the count
 * changes a bit (hold: the NaN flag of wtpse_loss_log — a poisoned run is never averaged).  The count is bumped behind the
 * fold (a single-wave launch of its own inside this entry point), so every element of a call sees the same k; nothing that
 * changes from step to step is passed by value: a recorded call stays valid under replay.  k <= 2^24 is the caller's to keep
 * ((float)k is exact up to there).  Bases of non-empty segments 16-byte aligned, a_s and p_s distinct; n_s arbitrary. */
int wtpse_avg_step(float* a0, const float* p0, long long n0, float* a1, const float* p1, long long n1, float* a2, const float* p2,
                   long long n2, float* a3, const float* p3, long long n3, int* count, const int* gate, const int* hold, void* stream);
/* Merges the mean `seg` of n_seg iterates into the mean `acc` of n_acc: n_acc == 0 copies; otherwise
 * w = (float)((double)n_seg / (double)(n_acc + n_seg)), formed on the host, and acc[i] = acc[i] + (seg[i] - acc[i]) * w with the
 * multiply and the add rounded separately.  n > 0, n_seg >= 1, both bases 16-byte aligned and distinct. */
int wtpse_avg_merge(float* acc, const float* seg, long long n, long long n_acc, long long n_seg, void* stream);

/* ---- fused 1x1 heads (csrc/head.hip) ------------------------------------------------------------------------------ */
/* The heads 32 -> 32 (ReLU) -> 8 [-> (ReLU) -> nc] as one kernel per direction: reference algorithms.py:1006-1012
 * (mu_prior / logvar_prior, three layers, nc <= 4) and :1199-1200 (the segmentation net's `mu`, two layers: w3 = b3 = y =
 * NULL and the 8-channel result is h2).  Weights are the plain OIHW parameters ([32][32], [8][32], [nc][8]), HW % 32 == 0.
 * x takes the conv loaders' prologue (pro: [32][2] scale/shift or NULL, pro_relu).  h1 ([B][32][HW], post-ReLU) and h2
 * ([B][8][HW], post-ReLU for three layers) are the tapes: pass NULL to skip storing them (h2 is mandatory for a two-layer
 * head: it is the output).
 * Arithmetic (round 6): under x2h (wtpse_x3_terms() == 2, the default) both layers run on the fp16 matrix cores at fp32 accuracy
 * exactly as the convolutions do — every operand = two fp16 terms of a power-of-two multiple of the value, three products, fp32
 * accumulation (12 v_mfma_f32_32x32x16_f16 per 32-pixel block where the fp32-input form needs 32 v_mfma_f32_32x32x2_f32: the
 * kernels were bound by those, not by their bytes).  x_amax: the amax table BOUNDING THE ACTIVATED INPUT (wtpse_amax /
 * wtpse_act_bound / a producer's table), or NULL: the fixed forward scale 2^2, i.e. |act(x)| < 2^13 or the outputs are NaN; W1 / W2
 * are scaled by their own largest magnitude, h1 by max_m sum_k |W1[m][k]| * bound(x) + max |b1|.  In the other modes (x3, bf16)
 * the fp32-input kernels of rounds 2-5 run and x_amax is ignored. */
int wtpse_head_fwd(const float* x, const float* pro, int pro_relu, const float* w1, const float* b1, const float* w2,
                   const float* b2, const float* w3, const float* b3, int nc, float* h1, float* h2, float* y,
                   const unsigned* x_amax, int B, int HW, void* stream);
/* dy: [B][nc][HW] (three layers) or [B][8][HW] (two layers: gradient of the h2 output).  dx: [B][32][HW] gradient wrt the
 * activated input.  dparams: [32*32 + 32 + 8*32 + 8 (+ 8*nc + nc)] = (dW1, db1, dW2, db2[, dW3, db3]) contiguous, which is
 * the order the head's parameters have in the flat gradient buffer; written, or added to when accumulate != 0.
 * slab: scratch of wtpse_head_slabs(B, HW) * that many floats.
 * x2h: h1 is NOT read (may be NULL; the forward need not store it) — layer 1 is formed again from the x the kernel reads anyway, by
 * the forward kernel's instruction sequence on its operands (the same bits, so the forward's ReLU mask): b1 and dy_amax (the amax
 * table of dy) are required, x_amax as in wtpse_head_fwd (the SAME table, or the masks may differ in the last bit of h1).  The
 * gradients' scales follow from bound(dy) through the weights' absolute row sums.  Other modes: h1 required, b1 / tables ignored. */
int wtpse_head_bwd(const float* dy, const float* x, const float* pro, int pro_relu, const float* h1, const float* h2,
                   const float* w1, const float* b1, const float* w2, const float* w3, int nc, float* dx, float* slab,
                   float* dparams, int accumulate, const unsigned* x_amax, const unsigned* dy_amax, int B, int HW, void* stream);
int wtpse_head_slabs(int B, int HW);

/* ---- device-side training input pipeline (csrc/pipeline.hip) ---------------------------------- */
/* One pass of Pillow's 8-bit separable resampling (the engine behind the reference's Image.resize calls,
 * custom_transforms.py:342-346,375-391).  in [N][Hin][Win][C] uint8; vertical = 0: out [N][Hin][L][C], vertical = 1:
 * out [N][L][Win][C].  bounds [T][L][2] = (first source index, tap count) and kk [T][L][ksize] = 22-bit fixed-point
 * coefficients as Pillow's precompute_coeffs / normalize_coeffs_8bpc produce them; sample n reads table tab[n]
 * (tab NULL: table 0 for every sample). */
int wtpse_resample_u8(const unsigned char* in, unsigned char* out, const int* bounds, const int* kk, const int* tab, int ksize,
                      int N, int Hin, int Win, int C, int L, int vertical, void* stream);
/* Normalize_tf + ToTensor (custom_transforms.py:455-499,581-599) on img [N][S][S][3] uint8 and the resized disc mask od
 * [N][S][S] uint8, read through per-sample index tables xidx / yidx [N][S] (NEAREST resize + crop of the mask):
 * image [N][3][S][S] = img / 127.5 - 1, od_out [N][1][S][S] = (mask <= 200), oc_out = (mask <= 50). */
int wtpse_input_finish(const unsigned char* img, const unsigned char* od, const int* xidx, const int* yidx, float* image,
                       float* od_out, float* oc_out, int N, int S, void* stream);
/* wtpse_input_finish's image alone, for a sample that has no mask (wtpse_hip/segment.py): img [N][S][S][3] uint8 ->
 * image [N][3][S][S] = img / 127.5 - 1 in fp32, two roundings. */
int wtpse_image_finish(const unsigned char* img, float* image, int N, int S, void* stream);

/* ---- training augmentations on the cropped uint8 sample (csrc/augment.hip; custom_transforms.py:22-132,204-217,310-327) ----
 * The optional stage between the crop and wtpse_input_finish: RandomRotate, RandomFlip, elastic_transform,
 * add_salt_pepper_noise, adjust_light, eraser, in that order, bit for bit (the host restatement is
 * input_pipeline.augment_host).  All fp64 arithmetic below is single IEEE adds and multiplies in a fixed order, never fused. */
/* out[i] = uniform double in [0, 1) number `pos + i` of the Philox4x32-10 stream `seed` (the generator of wtpse_randn): counter
 * (pos + i) >> 1, key = seed; an even number takes the block's words (0, 1), an odd one (2, 3); value = ((a >> 5) * 2^26 +
 * (b >> 6)) * 2^-53.  A number depends only on (seed, pos + i): a call continued at pos + n extends the same stream. */
int wtpse_uniform_f64(double* out, long long n, unsigned long long seed, unsigned long long pos, void* stream);
/* One pass of scipy.ndimage.gaussian_filter(mode="constant", cval=0) over `planes` fields of S x S doubles, along axis 0 (rows;
 * axis = 0) or axis 1 (axis = 1).  w [radius + 1]: the kernel's centre and one half (it is symmetric), from the host.  Per
 * output, in correlate1d's order: acc = x[0] * w[0]; for j = radius .. 1: acc += (x[-j] + x[+j]) * w[j]; outside the field x = 0.
 * dst plane p = post * acc.  Source plane of p: src_index NULL: p; else field p % 2 of sample src_index[p / 2] in a [.][2][S][S]
 * array (only the samples whose elastic coin fired are launched).  pre != 0: x = src * 2 - 1 (the uniform field of
 * custom_transforms.py:111).  The strip, its halo and w are staged in LDS ((65 + 2 * radius) * 16 + radius + 1 doubles, at most
 * 64 KiB): radius <= 216.  src != dst. */
int wtpse_aug_blur(const double* src, double* dst, const double* w, const int* src_index, int radius, int planes, int S, int axis,
                   int pre, double post, void* stream);
/* RandomRotate + RandomFlip + the materialisation of the cropped disc mask, one index gather.  img [N][S][S][3] uint8 (scaled and
 * cropped), od [N][S][S] uint8 read through xidx / yidx [N][S] as in wtpse_input_finish; code [N]: bits 0-1 = k (rotation by
 * k * 90 degrees counter-clockwise, Image.rotate on a square picture), bit 2 = FLIP_LEFT_RIGHT, bit 3 = FLIP_TOP_BOTTOM (applied
 * after the rotation, left-right first).  -> img_out [N][S][S][3], mask_out [N][S][S]. */
int wtpse_aug_geometry(const unsigned char* img, const unsigned char* od, const int* xidx, const int* yidx, const int* code,
                       unsigned char* img_out, unsigned char* mask_out, int N, int S, void* stream);
/* elastic_transform's map_coordinates(order=1): sample n with slot[n] < 0 is copied; otherwise pixel (r, c) reads at
 * (r + disp[slot][0][r][c], c + disp[slot][1][r][c]), disp [.][2][S][S] fp64.  Image: a coordinate outside [0, S-1] on either axis
 * gives 0 (mode="constant"); mask: coordinates are clamped to [0, S-1] (mode="nearest").  Value = (1-tx) * ((1-ty) * g00 + ty * g01)
 * + tx * ((1-ty) * g10 + ty * g11) with t = coordinate - floor(coordinate), stored as floor(value + 0.5) (scipy's uint8 output). */
int wtpse_aug_warp(const unsigned char* img, const unsigned char* mask, const double* disp, const int* slot, unsigned char* img_out,
                   unsigned char* mask_out, int N, int S, void* stream);
/* add_salt_pepper_noise, adjust_light and eraser on img [N][S][S][3] uint8, in place.  pts: pixel offsets (row * S + column) of all
 * samples' noise points, sample n owns pts[pt_off[n] .. pt_off[n+1]) and sets all three channels of each to pt_val[n] (salt: 1,
 * as the reference writes it; pepper: 0); lut [N][256]: the gamma table (identity: none); rect [N][5] = (top, left, h, w, fill),
 * h = 0: none.  A pixel ends as fill inside the rectangle, lut[pt_val] on a noise point, lut[pixel] elsewhere.  pts may be NULL
 * when pt_off[N] = 0; max_pts >= the largest point count of a sample. */
int wtpse_aug_photometric(unsigned char* img, const unsigned char* lut, const int* rect, const int* pts, const int* pt_off,
                          const int* pt_val, int max_pts, int N, int S, void* stream);

/* ---- amplitude mixing between source domains (csrc/spectrum.hip) ---------------------------------------------------------
 * The optional stage between the augmentations (or the crop) and wtpse_input_finish; input_pipeline.amplitude_mix_host is its
 * float64 specification.  img [N][S][S][3] uint8; a row n with 0 <= partner[n] < N keeps the phase of its 2-D spectrum F per
 * channel and moves its amplitude towards that of row partner[n] (spectrum G, always of the INPUT) inside the window |k_y| <= b,
 * |k_x| <= b of signed frequencies in [-S/2, S/2 - 1]:  D = lam[n] (|G| - |F|) F / |F| there (F / |F| = 1 where |F| = 0), 0
 * outside;  y = x + real(ifft2(D));  out_u8 = rint(clip(y, 0, 255)), half to even; out_f32 (may be NULL) = y.  Any other
 * partner[n] (-1) copies the row.  fp32 arithmetic; lam = 0 and partner[n] = n return the input bit for bit; no atomics: the same
 * result on every run.  S: a power of two from 32 to 512; 0 <= b <= S/2 (b = S/2: the whole spectrum); N <= 65535.
 * twiddle [S][2] = (cos, -sin)(2 pi t / S), computed in double precision and rounded once.  work: 16-byte aligned,
 * wtpse_amix_workspace(N, S, b) floats.  img != out_u8.  Three launches: row transforms (two real rows per complex transform,
 * columns u <= b kept), column transforms + D + inverse column transforms, inverse row transforms + store. */
/* floats of workspace a call needs: 4 * N * 3 * (b + 1) * S; -1 for a shape wtpse_amplitude_mix refuses.  Host only. */
int wtpse_amix_workspace(int N, int S, int b);
int wtpse_amplitude_mix(const unsigned char* img, const int* partner, const float* lam, const float* twiddle,
                        unsigned char* out_u8, float* out_f32, float* work, int N, int S, int b, void* stream);

/* ---- random appearance networks: GIN + IPA in fixed point (csrc/appearance.hip) -------------------------------------------
 * The optional stage between amplitude mixing (or the augmentations, or the crop) and the image-quality stage;
 * input_pipeline.appearance_host is its specification in integers, and the device equals it byte for byte.  The definition is this
 * project's own, after Ouyang et al. 2022 (GIN / IPA) and Xu et al. 2021 (RandConv): it is NOT byte-equal to anyone's float code.
 * img [N][S][S][3] uint8, 1 <= S <= 512, N <= 65535.  params [N][389] int32 per sample: flags (bit 0: selected, else the sample is
 * copied; bit 1: blend, two nets), alpha_0, alpha_1 (0 .. 256), then per net j = 0, 1 its 193 values: k[4] (1 or 3 per layer), the
 * weights W_l[co][ci][3][3] of layers l = 0 .. 3 one after the other (channels 3 -> 2 -> 2 -> 2 -> 3: 54 + 36 + 36 + 54 values, Q12,
 * |W| <= 16384; with k = 1 only the centre tap [1][1] is used, the others are ignored), the biases (2 + 2 + 2 + 3 values, Q8 grey
 * levels, |bias| <= 2^19).  `>>` is the arithmetic shift, CL = 2^19 - 1, x an input byte:
 *   m8  = (256 sums[n] + cnt/2) / cnt, cnt = 3 S S (the image-quality stage's pivot);  c0 = (x << 8) - m8, 0 outside the picture
 *   layer: v = ((sum_{ci,dy,dx} W[co][ci][dy][dx] h[ci][y + dy - 1][x + dx - 1] + 2048) >> 12) + bias[co] (64-bit sum; h = 0 outside
 *          the picture at EVERY layer); layers 0 .. 2: v < 0 -> (3 v + 128) >> 8; every layer: h' = clip(v, -CL, CL);  y_j = layer 3
 *   z_j = (alpha_j c0 + (256 - alpha_j) y_j + 128) >> 8
 *   E_in = sum ((c0 + 8) >> 4)^2, E_j = sum ((z_j + 8) >> 4)^2 over the sample: exact 64-bit integers below 2^53
 *   R_j = min(rint(sqrt((double)E_in / (double)E_j) * 4096), 2^20) — one fp64 division, square root and multiplication, each correctly
 *         rounded: the only floating-point operations of the stage;  E_j = 0: R_j = 4096 and z_j := c0
 *   g_j = clip((R_j z_j + 2048) >> 12, -CL, CL) (64-bit product)
 *   b   : without the blend flag 256 (net 0 alone; net 1 is not evaluated).  With it, from the control values field [N][G][G] (0 .. 256,
 *         G = ceil(S / spacing) + 3) through axis [S][5] = (first control index i, four cubic B-spline weights in Q12, >= 0, summing to
 *         4096; input_pipeline.appearance_axis_table), the same table for rows and columns:
 *         hx_r = (sum_c wx[c] P[iy + r][ix + c] + 8) >> 4 (r = 0 .. 3),  b = (sum_r wy[r] hx_r + 2^19) >> 20  (0 .. 256)
 *   out = clip((m8 + ((b g_0 + (256 - b) g_1 + 128) >> 8) + 128) >> 8, 0, 255)
 * alpha_0 = 256 without the blend flag returns the input.  No atomics on floats: the same bytes on every run.  out != img; img is not
 * written.  The entry points do not check the ranges of params, field and axis (ops.appearance_nets does): outside them the
 * arithmetic wraps (every index into field is clamped into the grid), inside them nothing leaves the stated widths — 32 bits
 * everywhere but the layers' sums, the energies and R_j z_j.  The spacing is at least 4: a tile of 32 x 64 pixels touches at most
 * 12 x 20 control values. */
/* 4-byte words of workspace a call needs: 7 N (energies and byte sums) rounded up to 4, plus 6 N S S (z_0 and z_1 as int32); -1 for
 * a shape the stage refuses or a size beyond 2^31 - 1 words.  Host only. */
int wtpse_appearance_workspace(int N, int S);
/* pass 1: the byte sums (wtpse_quality_sums into the workspace), then per tile the nets in LDS -> z_j and the energies.  work:
 * 16-byte aligned, wtpse_appearance_workspace(N, S) words.  A memset and two launches. */
int wtpse_appearance_nets(const unsigned char* img, const int* params, void* work, int N, int S, void* stream);
/* pass 2: R_j, the scaling, the field, the blend, the mean and the clip; samples that are not selected are copied.  work as pass 1
 * left it; 4 <= G <= 131.  One launch. */
int wtpse_appearance_finish(const unsigned char* img, const int* params, const int* field, const int* axis, const void* work,
                            unsigned char* out, int N, int S, int G, void* stream);

/* ---- image-quality augmentation: focus, contrast, brightness, noise (csrc/quality.hip) -----------------------------------
 * The optional stage between amplitude mixing (or the augmentations, or the crop) and wtpse_input_finish;
 * input_pipeline.quality_host is its specification in integers, and the device equals it byte for byte.  img [N][S][S][3] uint8,
 * 1 <= S <= 512, N <= 65535.  params [N][13] int32 per sample: a (focus, Q8: -256 the blurred picture, 0 untouched, > 0 unsharp
 * masking; -256 <= a <= 512), c (contrast, Q8, 0 <= c <= 512), beta (brightness shift, Q8 grey levels, |beta| <= 16320), k (noise
 * scale, 0 <= k <= 181000; 0: no noise), w[0..8] (Gaussian taps, Q12: w[j] >= 0, w[0] + 2 (w[1] + .. + w[8]) = 4096).  Per
 * pixel and channel, x the input byte, `>>` the arithmetic shift:
 *   H = sum_j w[|j|] X[y][clamp(x + j)], B = sum_j w[|j|] H[clamp(y + j)][x] (j = -8 .. 8, unsigned 32 bits), b8 = (B + 32768) >> 16,
 *   x8 = x << 8, s = x8 + ((a (x8 - b8) + 128) >> 8), m8 = (256 sums[n] + n/2) / n with n = 3 S S (64 bits, once per sample),
 *   t = m8 + ((c (s - m8) + 128) >> 8) + beta, u = t + ((k g + 2048) >> 12) when k > 0, out = clip((u + 128) >> 8, 0, 255);
 *   g = b0 + b1 + b2 + b3 - 510 of word ch of the Philox4x32-10 block with key `seed` and counter (pos[n] + y S + x, 0, 1): the 1
 *   keeps these blocks apart from those of wtpse_uniform_f64 and wtpse_randn for any seed.
 * A sample with a = 0 skips both blur passes; one with a = 0, c = 256, beta = 0, k = 0 is copied.  Integers only: the same bytes
 * on every run.  out != img; img is not written.  The entry points do not check the ranges of params (ops.image_quality does):
 * outside them the arithmetic wraps, inside them nothing leaves 32 bits. */
/* sums [N] uint32 = the sum of the 3 S S bytes of every sample (a memset and one launch; integer adds in any order). */
int wtpse_quality_sums(const unsigned char* img, unsigned* sums, int N, int S, void* stream);
int wtpse_quality_apply(const unsigned char* img, const int* params, const unsigned* sums, const unsigned long long* pos,
                        unsigned long long seed, unsigned char* out, int N, int S, void* stream);

/* ---- JPEG compression augmentation: baseline JPEG's pixel round trip without the bit stream (csrc/jpeg.hip) -----------------
 * The optional stage between the image-quality stage and CLAHE (or wtpse_input_finish); input_pipeline.jpeg_host is its
 * specification in integers — libjpeg's "islow" codec, pinned byte for byte to what Pillow writes and reads back
 * (tests/test_jpeg_cpu.py) — and the device equals it byte for byte.  img [N][S][S][3] uint8, S a multiple of 16 (no partial MCU),
 * 16 <= S <= 4096, 1 <= N <= 65535.  mode [N] int32: 0 the sample is copied, 1 = 4:4:4, 2 = 4:2:0 (chroma at half resolution both
 * ways).  tables [N][2][64] int32: the luma and the chroma quantisation table Q of every sample in natural (row-major) order,
 * 1 <= Q <= 255; recips [N][2][64] int32 = ceil(2^32 / (8 Q)) (input_pipeline.jpeg_reciprocals): the quantiser's division is
 * mulhi(|c| + (8 Q >> 1), recip), equal to the quotient for every |c| <= 32767 (tests/test_jpeg_cpu.py, exhaustively).  `>>` is the
 * arithmetic shift, DESCALE(x, n) = (x + (1 << (n - 1))) >> n:
 *   Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16,  Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16,
 *   Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16
 *   4:2:0: chroma = (the sum of a 2 x 2 cell + 1 in even output columns, 2 in odd ones) >> 2
 *   per 8 x 8 block of x - 128: libjpeg's jfdctint (CONST_BITS 13, PASS1_BITS 2; rows, then columns; the output carries a factor 8),
 *   k = sign(c) ((|c| + (8 Q >> 1)) / (8 Q)), c' = k Q, libjpeg's jidctint (columns DESCALE 11, rows DESCALE 18), + 128, clamp 0 .. 255
 *   4:2:0: libjpeg's h2v2 "fancy" upsampling: cs = 3 near row + far row (the far row: above for even output rows, below for odd,
 *   the near row itself at the picture's top and bottom), even column (3 cs[x] + cs[x - 1] + 8) >> 4, odd (3 cs[x] + cs[x + 1] + 7) >> 4,
 *   the picture's first column (4 cs[0] + 8) >> 4, its last (4 cs[last] + 7) >> 4
 *   R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16), each
 *   clamped to 0 .. 255 (cb = Cb - 128, cr = Cr - 128)
 * Two launches: the first decodes the half-resolution chroma planes of the 4:2:0 samples into chroma [N][2][S/2][S/2] uint8 (nothing
 * else of a sample ever leaves the chip between the two colour conversions), the second does everything else and, for a 4:2:0
 * sample, upsamples out of `chroma`.  chroma == NULL: the first launch is skipped — the caller asserts that no sample has mode 2.
 * Integers only, no atomics: the same bytes on every run.  img, out 16-byte aligned and distinct, chroma 4-byte aligned; img is
 * not written.  The entry point does not check mode, tables and recips (ops.jpeg_roundtrip does). */
int wtpse_jpeg_roundtrip(const unsigned char* img, const int* mode, const int* tables, const int* recips, unsigned char* chroma,
                         unsigned char* out, int N, int S, void* stream);

/* ---- CLAHE preprocessing: tile histograms, clipped LUTs, bilinear blend (csrc/clahe.hip) ----------------------------------
 * Contrast-limited adaptive histogram equalisation of img [N][H][W][3] uint8 in front of the normalisation (wtpse_input_finish /
 * wtpse_image_finish); input_pipeline.clahe_host is its specification in integers, and the device equals it byte for byte.
 * 1 <= H, W <= 4096, 1 <= N <= 65535, 1 <= ty <= min(16, H), 1 <= tx <= min(16, W), 0 <= floor <= 255, planes = 1 ("luma": the plane
 * Y = (77 R + 150 G + 29 B + 128) >> 8) or 3 ("rgb": the channels), 256 <= clip_q8 <= 65536 (256 times the clip limit).
 *   field : max(R, G, B) >= floor; a pixel outside it is neither counted nor changed.
 *   tiles : boundaries b_k = (k L) / t (floor) along each axis, k = 0 .. t.
 *   LUT of a tile and plane, h[256] its histogram over field pixels, n = sum h: the identity when n = 0; else limit = max(1,
 *     (clip_q8 n) >> 16) (64 bits), excess = sum max(h - limit, 0), h = min(h, limit) + excess / 256, r = excess % 256, and with
 *     step = 256 / r the bins 0, step, .., (r - 1) step get one more; c = the inclusive prefix sum; lut[v] = min((255 c[v] + n / 2) / n, 255).
 *   pixel : rows[y] = k0y | wy << 8, cols[x] = k0x | wx << 8 (input_pipeline.clahe_axis_table: the lower tile and the Q8 weight, 0 ..
 *     256, of the next; cols holds W rounded up to a multiple of 4 entries and is 16-byte aligned), the upper tiles min(k0 + 1,
 *     t - 1); a, b, c, d = the LUT values of tiles (k0y, k0x), (k0y, k0x + 1), (k0y + 1, k0x), (k0y + 1, k0x + 1) at the plane's value:
 *     v' = ((256 - wy) ((256 - wx) a + wx b) + wy ((256 - wx) c + wx d) + 32768) >> 16.
 *     planes = 3: channel c becomes its own v'; planes = 1: every channel becomes clip(channel + (Y' - Y), 0, 255).
 * Integers only: the same bytes on every run, whatever the order of the histogram's atomic adds. */
/* hist [N][planes][ty tx][256] uint32 (a memset and one launch; tiles of more than 4096 pixels are split over workgroups). */
int wtpse_clahe_hist(const unsigned char* img, unsigned* hist, int N, int H, int W, int ty, int tx, int floor, int planes,
                     void* stream);
/* hist [count][256] uint32 -> lut [count][256] uint8, count = N planes ty tx; both 16-byte aligned. */
int wtpse_clahe_lut(const unsigned* hist, unsigned char* lut, int count, int clip_q8, void* stream);
/* bands [ty + 1]: the first row y whose k0y is k (k0y does not decrease with y and takes every value), bands[ty] = H — a workgroup
 * stages the LUTs of tile rows k and min(k + 1, ty - 1) in LDS and works on rows of band k only; rows, cols and bands as
 * input_pipeline.clahe_device_tables builds them (their contents are not checked here).  lut is 4-byte aligned.  out != img; img is
 * not written. */
int wtpse_clahe_apply(const unsigned char* img, const unsigned char* lut, const int* rows, const int* cols, const int* bands,
                      unsigned char* out, int N, int H, int W, int ty, int tx, int floor, int planes, void* stream);

/* ---- validation back half (csrc/postprocess.hip) --------------------------------------------------- */
/* utils.postprocessing (utils.py:267-329) bit for bit: logit [B][h][w] fp32 -> out [B][h][w] uint8 = the largest 8-connected
 * component of sigmoid(logit) > threshold (ties: the first in raster order), holes (background not 4-connected to the border)
 * filled.  ws: wtpse_postprocess_ws(B, h, w) 4-byte words, 8-byte aligned.  1 <= h, w <= 4096. */
int wtpse_postprocess_ws(int B, int h, int w);
int wtpse_postprocess(const float* logit, unsigned char* out, void* ws, float threshold, int B, int h, int w, void* stream);
/* Per-image Dice / ASD / HD95 ingredients of a mask A (uint8, nonzero = object) against a label B (fp32, nonzero = object), both
 * [B][h][w]: rec [B][8] int64 = {|A & B|, |A|, |B|, surface pixels of A, of B, d2_lo, d2_hi, ASD sum}.  Surface = object XOR its
 * erosion by the 4-neighbour cross (outside the image = background); d2 = exact squared Euclidean distance of a surface pixel to
 * the other mask's surface; d2_lo / d2_hi = the two order statistics of the pooled d2 of both directions that numpy.percentile(.,
 * 95) interpolates between (0 when a surface is empty); slot 7 holds the fp64 bits of sum(sqrt(d2)) over A's surface, folded in a
 * fixed order.  ws: wtpse_seg_metrics_ws(B, h, w) 4-byte words, 8-byte aligned.  1 <= h, w <= 4096. */
int wtpse_seg_metrics_ws(int B, int h, int w);
int wtpse_seg_metrics(const unsigned char* mask, const float* label, long long* rec, void* ws, int B, int h, int w, void* stream);

/* ---- test run (csrc/overlay.hip; test_visulization.py:238-269, utils.py:371-463) --------------------------------------- */
/* The per-image pictures of the reference's test program, a batch at a time.  img [B][3][h][w] fp32: the normalised image at the
 * label size; pred_od / pred_oc [B][h][w] uint8: wtpse_postprocess's masks; gt_od / gt_oc [B][h][w] uint8 labels, 0 / 1.
 * original [B][h][w][3] uint8 = (img + 1) * 127.5 (two fp32 roundings) truncated; overlay [B][h][w][3] = the same with the contours
 * painted: composite channel 0 = cup, channel 1 = disc OR cup; the prediction's channels with their border rows and columns zeroed,
 * green for channel 1 then blue for channel 0; the ground truth's channels through largest-component + hole filling
 * (wtpse_postprocess on a +-30 pseudo-logit), red, on top.  A contour vertex sits between every two 4-adjacent pixels that differ
 * and paints seven pixels around itself; an index of -1 wraps as numpy's does, an index of h or w (the reference raises IndexError:
 * ground truth touching the last row / column) is dropped.  ws: wtpse_overlay_ws(B, h, w) 4-byte words, 8-byte aligned; img,
 * original, overlay 4-byte aligned.  2 <= h, w <= 4096. */
int wtpse_overlay_ws(int B, int h, int w);
int wtpse_overlay(const float* img, const unsigned char* pred_od, const unsigned char* pred_oc, const unsigned char* gt_od,
                  const unsigned char* gt_oc, unsigned char* original, unsigned char* overlay, void* ws, int B, int h, int w,
                  void* stream);
/* The test feed's labels at their original size (fundus_dataloader.py:112-134): mask [n] uint8 grey levels ->
 * od [n] = (mask <= 200), oc [n] = (mask <= 50), fp32. */
int wtpse_label_thresholds(const unsigned char* mask, float* od, float* oc, long long n, void* stream);

/* ---- segmenting unlabelled images (csrc/measure.hip, csrc/overlay.hip; wtpse_hip/segment.py) --------------------------------- */
/* wtpse_overlay without a ground truth: the same two pictures with nothing painted red, byte for byte what wtpse_overlay gives for
 * all-zero gt_od / gt_oc, without its largest-component stage and its scratch.  wtpse_overlay_pred_ws: 0 (no workspace is needed) when
 * wtpse_overlay supports the size, -1 otherwise.  img, original, overlay 4-byte aligned.  2 <= h, w <= 4096. */
int wtpse_overlay_pred_ws(int B, int h, int w);
int wtpse_overlay_pred(const float* img, const unsigned char* pred_od, const unsigned char* pred_oc, unsigned char* original,
                       unsigned char* overlay, int B, int h, int w, void* stream);
/* The dataset's grey-level label from two masks (uint8 [n], nonzero = object): out [n] = 0 where cup, else 128 where disc, else 255.
 * The inverse of wtpse_label_thresholds: read back, oc = (cup != 0) and od = ((disc | cup) != 0). */
int wtpse_label_map(const unsigned char* disc, const unsigned char* cup, unsigned char* out, long long n, void* stream);
/* mask [B][h][w] uint8 -> rec [B][8] int64 = {area, top, bottom, left, right, sum_r, sum_c, 0} over the nonzero pixels: their count,
 * the first / last row and column that hold one, and the sums of their row and column indices.  An empty mask: {0, h, -1, w, -1, 0, 0,
 * 0}.  Integer arithmetic only (64-bit sums): exact, the same on every run, no host synchronisation.  rec 8-byte aligned.
 * 1 <= h, w <= 4096. */
int wtpse_mask_geometry(const unsigned char* mask, long long* rec, int B, int h, int w, void* stream);
/* Optic-disc morphometry (csrc/morphometry.hip; morphometry.profile_host is the specification, bit for bit): one pass over a pair of
 * masks disc, cup [B][h][w] uint8 (nonzero = object) behind wtpse_mask_geometry's records geom [B][8] of the disc, read on the device.
 * Centre in half-pixel units: c2y = (4 sum_r + area) / (2 area) (integer division: 2 * centroid rounded half up), c2x from sum_c.
 * A pixel (x, y) has p = (2 x - c2x, c2y - 2 y) (py up the screen), r2 = |p|^2, and lies in the sector s of 0 .. N - 1 with
 * cross(T[s], p) >= 0 > cross(T[s + 1], p), cross(a, p) = a.x p.y - a.y p.x in 64 bits; p = 0 lies in sector 0.  table [N + 1][2]
 * int32 = T, the host's (morphometry.sector_table: 2^20 (cos, sin)(2 pi k / N), rounded); sector 0 starts at image-right, sectors run
 * counter-clockwise on the screen.  No floating point.
 *   profile [B][N][4] uint32 = {max r2 of the disc's pixels, max r2 of the cup's, disc pixels, cup pixels} per sector (the cup is not
 *            clipped to the disc); all zero for an image whose disc is empty
 *   moments [B][2][4] int64: row 0 the disc's {sum y^2, sum x^2, sum x y, c2y}, row 1 the cup's {.., .., .., c2x}; the sums are taken
 *            for an empty disc too, the centre slots then stay 0
 * Both are zeroed on the stream first.  Exact and the same on every run; no host synchronisation.  geom, moments 8-byte aligned.
 * 1 <= B < 8192, 1 <= h, w <= 4096, 8 <= N <= 360 and N % 8 == 0. */
int wtpse_onh_profile(const unsigned char* disc, const unsigned char* cup, const long long* geom, const int* table, unsigned* profile,
                      long long* moments, int N, int B, int h, int w, void* stream);

/* ---- whole fundus photographs (csrc/locate.hip; wtpse_hip/locate.py holds the host specifications, bit for bit) -------------------
 * The one pass over the full-size pictures.  img [N][H][W][3] uint8 (interleaved RGB, any base alignment) -> cells [N][CH][CW][2]
 * int64, CH = ceil(H / c), CW = ceil(W / c): per c x c cell, over its pixels that lie inside the picture and have max(R, G, B) >= t,
 *   {n = their count, s = the sum of 77 R + 150 G + 29 B over them}   (locate.cells_host)
 * (a full 256 x 256 cell of white pixels gives s = 2^32 - 2^24: the sums are 64-bit).  Integer arithmetic only, every cell is written by
 * exactly one workgroup with a plain store: exact, the same on every run, nothing to zero first, no host synchronisation.  Nothing
 * outside the 16-byte-aligned hull of img is read.  1 <= N <= 65535, 1 <= H, W <= 65536, 2 <= c <= 256, 0 <= t <= 255; cells 8-byte
 * aligned. */
int wtpse_locate_cells(const unsigned char* img, long long* cells, int N, int H, int W, int c, int t, void* stream);
/* M square boxes of side s out of one picture img [H][W][C] uint8 (C = 1 or 3): out [M][s][s][C], out[m][y][x] = img[top_m + y][left_m + x]
 * where that lies inside the picture, else 0 (a box may lie partly or wholly outside); boxes [M][2] int32 = (top, left) in DEVICE memory.
 * A pure copy (locate.crop_host).  1 <= H, W <= 65536, 1 <= M <= 65535, 1 <= s <= 8192; img and out distinct. */
int wtpse_crop_u8(const unsigned char* img, const int* boxes, unsigned char* out, int H, int W, int C, int M, int s, void* stream);
/* canvas [H][W][C] uint8 (C = 1 or 3), in place: canvas[top + y][left + x] = patch[y][x] for the pixels of patch [h][w][C] that land
 * inside the canvas (clipped at all four borders; a patch wholly outside launches nothing).  A pure copy (locate.paste_host).
 * 1 <= H, W, h, w <= 65536, |top|, |left| <= 2^24; canvas and patch distinct. */
int wtpse_paste_u8(unsigned char* canvas, const unsigned char* patch, int H, int W, int C, int h, int w, int top, int left, void* stream);

/* ---- gradability check (csrc/gradability.hip; gradability.record_host is the specification, bit for bit) -------------------------
 * One exact-integer pass over the full-size pictures.  img [N][H][W][3] uint8 (interleaved RGB, any base alignment) -> rec
 * [N][WTPSE_GRAD_REC] int64, initialised on the stream first.  Per picture, with
 *   field    f(p) = max(R, G, B) >= t; a position outside the picture is not in the field (wtpse_locate_cells' definition; t = 0: every
 *            pixel of the picture)
 *   luma     Y = (77 R + 150 G + 29 B + 128) >> 8, in 0..255
 * the record is
 *   rec[0 .. 255]           the histogram of Y over the field
 *   rec[256 .. 258]         the sums of R, G, B over the field
 *   rec[259 .. 261]         the field pixels with R, G, B >= sat, per channel
 *   rec[262]                the field's area n
 *   rec[263 .. 266]         top, bottom, left, right of the field's bounding box; (H, -1, W, -1) for an empty field
 *   rec[267 + 3k .. 269 + 3k]   (n_d, E_d, Q_d) for the k-th dilation d of (1, 2, 4)
 * For a dilation d a pixel p is interior when p and its four neighbours at distance d along the rows and the columns all lie in the
 * picture and in the field; over the interior pixels, on the green channel G,
 *   L = 4 G(p) - G(up) - G(down) - G(left) - G(right),   E_d = sum L^2,   Q_d = sum (G(right) - G(left))^2 + (G(down) - G(up))^2,
 * and n_d is their number.  L^2 <= 1020^2, so a 65536 x 65536 picture stays below 2^53; the sums are 64-bit.  Integer arithmetic only,
 * the workgroups' partial records meet in the picture's with 64-bit integer atomics: exact and the same on every run; nothing is
 * allocated, no host synchronisation.  Nothing outside the 16-byte-aligned hull of img is read.
 * 1 <= N <= 65535, 1 <= H, W <= 65536, 0 <= t <= 255, 1 <= sat <= 255; rec 8-byte aligned. */
#define WTPSE_GRAD_REC 276
int wtpse_gradability_record(const unsigned char* img, long long* rec, int N, int H, int W, int t, int sat, void* stream);

/* ---- calibration against labels (csrc/calibration.hip; calibration.hist_host is the specification, bit for bit) ----------------
 * One pass over a probability map prob, a spread map spread (NULL: every spread is 0) and a label (nonzero = object, as
 * wtpse_seg_metrics takes it; y = 1 for an object pixel, else 0), all [B][h][w] fp32, optionally restricted to the pixels where
 * region [B][h][w] uint8 is nonzero (NULL: every pixel).  rec [B][WTPSE_CAL_REC] uint32, zeroed on the stream first, is per image
 *   hist_p [WTPSE_CAL_BINS + 1][2], then hist_s [WTPSE_CAL_BINS + 1][2], then tail [4].
 * Per pixel, in this order:
 *   region == 0                   tail[0 + y] += 1; the pixel is not scored (its prob and spread are not looked at)
 *   prob or spread is NaN         tail[2] += 1; the pixel is not scored
 *   otherwise                     tail[3] += 1 and, with
 *                                   q = (int)rintf(min(max(prob, 0), 1) * 1024.f)        0 .. 1024 (+-inf clamp like any other value)
 *                                   u = (int)rintf(min(max(spread, 0), 0.5f) * 2048.f)   0 .. 1024
 *                                   e = ((prob > threshold) != y)                        the unclamped, unquantised prob
 *                                 hist_p[q][y] += 1 and hist_s[u][e] += 1
 * Both products are exact in fp32 (a power of two times a value of at most 1) and rintf rounds half to even: numpy.rint on float32 is
 * the same function.  Integer arithmetic only — a count is at most h w <= 2^24 — exact and the same on every run; no host
 * synchronisation; no alignment or width premise beyond the element types' own.  hist_p summed over both columns and hist_s summed over
 * both columns each total tail[3]; the four tail counts total h w.
 * 1 <= B < 8192, 1 <= h, w <= 4096. */
#define WTPSE_CAL_BINS 1024
#define WTPSE_CAL_REC (2 * (WTPSE_CAL_BINS + 1) * 2 + 4)
int wtpse_calibration_hist(const float* prob, const float* spread, const float* label, const unsigned char* region, float threshold,
                           unsigned* rec, int B, int h, int w, void* stream);

/* ---- sampled shape latents (csrc/uncertainty.hip; uncertainty.shape_samples_host is the fp64 specification) --------------------
 * K draws of the student's latent and everything behind it in one launch.  Per image b, pixel p and sample k:
 *   z = mu + scale * exp(logvar / 2) * eps[b,k,p]         (a non-finite exp(logvar / 2) counts as 0, as in the student's sampling)
 *   a = sigmoid(w * z + b)                                 wb = device {w, b}: the attention layer
 *   logit = (coef + a) * sum_c wout[c] * emb[b,c,p] + bout[0] (+ wz[0] * z: the latent's own weight of a cat_shape head, else NULL)
 *   prob = sigmoid(logit)
 * (the channel sum is taken once per pixel, outside the K loop: fuse[c] = coef * emb[c] + a * emb[c] is never formed) and
 *   mean [B,HW] = the mean of the K probabilities, std_ [B,HW] = their population standard deviation (running Welford update: K equal
 *   samples give exactly 0), votes [B,HW] uint8 = #{k: prob > threshold}, logits [B,K,HW] = logit (NULL: not stored).
 * eps[b,k,p] is element offset + (b * K + k) * HW + p of the wtpse_randn stream `seed`, drawn in the kernel, or noise[b,k,p] when
 * noise ([B,K,HW]) is given: wtpse_randn(noise, B * K * HW, seed, offset) makes the two bit for bit the same.
 * 1 <= K <= 64, 1 <= CE <= 16, HW % 4 == 0, offset % 4 == 0 (a lane owns four pixels = one Philox block per sample), scale >= 0;
 * emb, mu, logvar, noise, mean, std_, logits 16-byte aligned, votes 4-byte aligned. */
int wtpse_shape_samples(const float* emb, int CE, const float* mu, const float* logvar, const float* wb, float coef,
                        const float* wout, const float* bout, const float* wz, float scale, int K, unsigned long long seed,
                        unsigned long long offset, const float* noise, float threshold, float* mean, float* std_,
                        unsigned char* votes, float* logits, int B, int HW, void* stream);

/* What wtpse_shape_samples would have left had every sampled logit been multiplied by a {0,1} map first (the cup's logits times
 * od_pred, validate.predict_pair): where ref[b,p] <= 0 (or NaN), logits[b,k,p] = 0 for every k, mean = 0.5 (sigmoid(0)), std_ = 0 and
 * votes = 0 (threshold >= 0.5 is the caller's premise); the other pixels are left as they are.  ref, mean, std_ [B,HW], logits
 * [B,K,HW] or NULL; HW % 4 == 0, the same alignments. */
int wtpse_shape_samples_mask(const float* ref, float* mean, float* std_, unsigned char* votes, float* logits, int K, int B, int HW,
                             void* stream);

/* ---- test-time views (csrc/views.hip; wtpse_hip/views.py holds the definition and views.merge_host, the specification) ----------
 * A view code c in 0..7 acts on a square plane a as numpy states it: t = a.T if c & 4; rows of t reversed if c & 2; then columns
 * reversed if c & 1 (0 identity, 1 horizontal flip, 2 vertical flip, 3 half turn, 4..7 the transposing ones).  `codes` is a HOST array
 * of V ints, read during the call.
 * x [N][S][S] fp32 planes -> out [V][N][S][S]: plane n of view v is the view codes[v] of x[n], bit for bit (a pure permutation).
 * 1 <= V <= 8, every code in 0..7, N >= 1, S % 4 == 0 (square planes only: the transposing views need them); x, out 16-byte
 * aligned and distinct. */
int wtpse_dihedral_views(const float* x, float* out, const int* codes, int V, int N, int S, void* stream);

/* The fused merge.  logits [V][B][K][S][S]: K logit maps per view and image, each in its view's own frame.  With s = v * K + k:
 *   logits_out [B][V*K][S][S]  map s = the inverse view of logits[v][b][k] (a pure permutation); NULL: not stored
 *   mean, std_ [B][S][S]       mean and population standard deviation of the V K values sigmoid(logit_s) of a pixel, by a running
 *                              Welford update in order of s (equal samples give exactly 0)
 *   votes [B][S][S] uint8      #{s: sigmoid(logit_s) > threshold}
 *   mean_logit [B][S][S]       the float32 sum of the un-viewed logits in order of s (starting from the first; one addition each),
 *                              times 1.f / (float)(V K): bit for bit views.merge_host's; NULL: not stored
 * One pass, no atomics, results independent of the grid.  1 <= V <= 8, every code in 0..7, K >= 1, V * K <= 64, B >= 1, S % 4 == 0;
 * logits, logits_out, mean, std_, mean_logit 16-byte aligned, votes 4-byte aligned; no output may overlap the input. */
int wtpse_views_merge(const float* logits, const int* codes, int V, int B, int K, int S, float threshold, float* logits_out,
                      float* mean, float* std_, unsigned char* votes, float* mean_logit, void* stream);

/* ---- small utilities ------------------------------------------------------------------------------------------- */
int wtpse_relu_mask(const float* dz, const float* ref, float* dy, int accumulate, long long n, void* stream);
int wtpse_axpy(float* dst, const float* src, float alpha, long long n, void* stream);
int wtpse_reduce_rows(const float* partial, int rows, int cols, float* out, int accumulate, float scale, void* stream);
int wtpse_zero(void* p, long long nbytes, void* stream);
/* dst[0:n] = src[0:n] (n % 4 == 0, 16-byte aligned) with 16 or 4 bytes per lane and access: measurement infrastructure only — the
 * known-byte-count streams the rocprofv3 FETCH_SIZE / WRITE_SIZE factors are calibrated on (tools/pmc_traffic.py, bench.py --kernels-only). */
int wtpse_copy_probe(const float* src, float* dst, long long n, int bytes_per_lane, void* stream);

/* ---- standalone 2-D discrete wavelet transform (csrc/dwt.hip) — NOT part of WT-PSE ---------------------------------------
 * The reference has no wavelet transform (its "WT" is the whitening transform); these two entry points exist only as the
 * HBM-bandwidth micro-benchmark BASELINE.json's wording names and are never called by the training path.
 * Specification (self-defined, parity unpinned): oracle/dwt_cpu.py — separable, orthonormal, periodic extension, lifting,
 * Mallat layout.  x / coef: [planes][H][W] fp32, distinct buffers; wavelet 0 = Haar, 1 = Daubechies 4-tap ("db2");
 * H, W divisible by 2^levels; tmp: 2 * planes * (H/2) * (W/2) floats.  x, coef and tmp must be 8-byte aligned (the kernels move
 * float2; anything else is refused before a launch); on square 256 / 512 planes (levels <= 7 / 8) 16-byte alignment of all three
 * selects the streaming forward path, 8-byte alignment the generic one (tests/dwt_cases.py restates the dispatcher). */
int wtpse_dwt2_fwd(const float* x, float* coef, float* tmp, int planes, int H, int W, int wavelet, int levels, void* stream);
int wtpse_dwt2_inv(const float* coef, float* x, float* tmp, int planes, int H, int W, int wavelet, int levels, void* stream);

/* ---- launch plans (csrc/plan.hip): a recorded sequence of the calls above, replayed with one host call ------------------
 * wtpse_plan_add_call: `fn` indexes the entry points that take a stream (wtpse_plan_fn_name(fn), 0 <= fn < wtpse_plan_fn_count());
 * `args`: its arguments without the trailing stream, one 8-byte slot each (pointer / long long / unsigned long long / double).
 * wtpse_plan_add_wait: stream `waiter` waits for everything issued so far on stream `waited`. */
int wtpse_plan_fn_count(void);
const char* wtpse_plan_fn_name(int id);
void* wtpse_plan_create(void);
int wtpse_plan_destroy(void* plan);
int wtpse_plan_size(void* plan);
int wtpse_plan_add_call(void* plan, int fn, const void* args, int nargs, void* stream);
int wtpse_plan_add_wait(void* plan, void* waiter, void* waited);
int wtpse_plan_replay(void* plan);      /* -2 (WTPSE_ESTATE): wtpse_tuning_state() differs from the recording's */
/* The run-time switches that decide tilings and the packed-weight format (wtpse_x3_terms | wtpse_x3r_enable << 4 | wtpse_x3_xcd << 8 |
 * wtpse_x3_small_wide << 12). */
int wtpse_tuning_state(void);

/* Fingerprint (hex) of the sources and of this header the library was compiled from; the binding refuses a library
 * whose fingerprint differs from the tree's (a stale .so after a signature change would otherwise go unnoticed). */
const char* wtpse_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif
