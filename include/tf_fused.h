/*
 * include/tf_fused.h -- C ABI of the fused element-wise kernels of libtf_msda.so that sit between the
 * library GEMMs / convolutions of the per-frame path (hand-written HIP, gfx950).
 *
 * They replace chains of separate ATen element-wise kernels of the reference's eager PyTorch path:
 *
 *   tf_bias_act_f32        conv -> FrozenBatchNorm2d shift -> (+ identity) -> ReLU
 *                          (reference: models/backbone.py:45-55 FrozenBatchNorm2d.forward + torchvision
 *                          Bottleneck's `out += identity; out = relu(out)`): one in-place pass instead of 3-4
 *   tf_add_layernorm_f32   `src = src + dropout(src2); src = norm(src)` of every transformer layer
 *                          (reference: models/deformable_transformer.py:291-292, :285-286, :371-372, :378-379,
 *                          :360-361): residual add + LayerNorm in one pass
 *
 *   tf_linear_split_f32    nn.Linear (+ ReLU) of the encoder / decoder (ms_deform_attn.py:64-88,
 *                          deformable_transformer.py:282-297) as a split product on the matrix cores (fp16 pieces, three terms:
 *                          fp32-class, what trackformer_amd uses by default; or six bf16 terms -- THE SPLIT PRODUCT below)
 *   tf_linear_packed_f32   the same product with the weight packed once in fragment order (+ tf_linear_pack_weight_f32)
 *   tf_ffn_fused_f32       linear1 -> ReLU -> linear2 -> + residual -> LayerNorm of a transformer layer in one launch
 *   tf_linear_res_ln_f32   linear (256 -> 256) -> + residual -> LayerNorm in one launch (output projection + norm1)
 *   tf_mha_core_f32        softmax(q k^T * scale) v of the decoder's query self-attention
 *                          (deformable_transformer.py:364-383, nn.MultiheadAttention): one launch, fp32
 *
 * Conventions as in tf_msda.h: device pointers, caller-owned buffers, work enqueued on `stream`
 * (hipStream_t as void*), no synchronisation, returns 0 or a negative tf_msda_status.
 */
#ifndef TF_FUSED_H_
#define TF_FUSED_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * x[i] = act(x[i] + bias[i % C] + (residual ? residual[i] : 0)),  act = ReLU if relu != 0 else identity.
 * x / residual: `n` floats, channel-innermost (NHWC storage of a channels_last tensor), in place on x.
 * C % 4 == 0 and 16-byte aligned pointers are required.
 * Non-finite operands: plain IEEE additions in the order (x + bias) + residual, each rounded to fp32; ReLU is `v < 0 ? 0 : v`, which
 * keeps NaN and -0.0.  That is torch.relu on the CPU; on MI355X torch.relu(-0.0) is +0.0, so there the result differs from the ATen
 * chain in the sign of such zeros (and in nothing else).  residual must not overlap x (the kernel's pointers are restrict-qualified);
 * residual == x is refused.
 */
int tf_bias_act_f32(float *x, const float *bias, const float *residual, int64_t n, int C, int relu,
                    void *stream);

/*
 * out[r, :] = LayerNorm(x[r, :] + res[r, :]) * gamma + beta   for r in [0, rows), row length C
 * (C % 4 == 0, C <= 4096).  `res` may be NULL (plain LayerNorm).  out may alias x.
 * Statistics in fp32 with the biased variance and eps inside the square root, as torch.nn.LayerNorm.
 */
int tf_add_layernorm_f32(const float *x, const float *res, const float *gamma, const float *beta,
                         float *out, int64_t rows, int C, float eps, void *stream);

/*
 * Iterative box refinement of the decoder in one pass (reference: models/deformable_transformer.py:331-343 +
 * util/misc.py inverse_sigmoid): out[r, c] = sigmoid(delta[r, c] + (c < ref_dim ? logit_eps(ref[r, c]) : 0)),
 * delta / out [rows, 4], ref [rows, ref_dim], ref_dim in {2, 4}, logit_eps(x) = log(max(x', eps) / max(1 - x', eps)) with
 * x' = clamp(x, 0, 1).  out may alias delta.
 */
int tf_box_refine_f32(const float *delta, const float *ref, float *out, int64_t rows, int ref_dim, float eps, void *stream);

/*
 * The per-frame post-processing of the tracker in one pass (reference: models/deformable_detr.py DeformablePostProcess.forward
 * -- sigmoid, best class and its score, boxes cxcywh -> xyxy scaled to the image -- followed by models/tracker.py:300-303
 * clip_boxes_to_image and the stacking of what the association reads).  logits [Q, C], boxes [Q, 4] (cx, cy, w, h in [0, 1]),
 * out [Q, 6] = (x0, y0, x1, y1, score, label as float):
 *   score = max_c sigmoid(logits[q, c]), label = the first c that attains it;
 *   non-finite logits as `sigmoid().max(-1)`: +inf scores exactly 1, -inf exactly 0; a NaN logit in ANY class makes the score NaN and
 *   the label the FIRST class whose logit is NaN (torch.max, on the CPU and on the device); the boxes are independent of the logits,
 *   and fminf / fmaxf turn a NaN coordinate into 0 when clip != 0 (torch.clamp would keep it: boxes are expected to be finite);
 *   x0 = (cx - 0.5 w) img_w, y0 = (cy - 0.5 h) img_h, x1 = (cx + 0.5 w) img_w, y1 = (cy + 0.5 h) img_h, every operation rounded
 *   on its own (no fused multiply-add: the arithmetic of the separate ATen kernels), then, if clip != 0, clamped to [0, img_w] /
 *   [0, img_h].  Replaces ~17 element-wise launches on [Q, 4] tensors per frame.
 */
int tf_postprocess_pack_f32(const float *logits, const float *boxes, float *out, int64_t Q, int C, float img_h, float img_w,
                            int clip, void *stream);

/*
 * GroupNorm of a channels-innermost activation: x [N, HW, C] (row n starts at x + n * x_image_stride floats; the storage of
 * a channels_last NCHW tensor or a token-major projection output), G groups of C / G consecutive channels, statistics
 * per (image, group) with the biased variance and eps inside the square root (torch.nn.GroupNorm); out may alias x.
 * workspace: 2 * N * G doubles (zeroed by the call).  C <= 1024, C % 4 == 0, 16-byte aligned pointers.
 * For the reference's `input_proj` (models/deformable_detr.py:73-90: Conv2d -> GroupNorm(32, hidden_dim)).
 */
int tf_groupnorm_nhwc_f32(const float *x, const float *gamma, const float *beta, float *out, double *workspace, int N,
                          int HW, int C, int G, float eps, int64_t x_image_stride, int64_t out_image_stride, void *stream);
/* The statistics pass alone: workspace[n][g] = (sum, sum of squares) of x's group g of image n, as doubles: every element is widened
 * to double BEFORE it is squared and summed, so that var = sumsq / cnt - mean^2 (formed in double by the consumers) keeps the variance
 * of a group whose |mean| is thousands of times its spread -- for a consumer that applies the normalisation in its own fetch
 * (tf_conv3x3_merge_packed_f32). */
int tf_groupnorm_stats_nhwc_f32(const float *x, double *workspace, int N, int HW, int C, int G, int64_t x_image_stride, void *stream);
/* The same followed by ReLU in the same pass: `F.relu(gn(conv(x)))` of the mask head (reference: models/detr_segmentation.py:142-156). */
int tf_groupnorm_relu_nhwc_f32(const float *x, const float *gamma, const float *beta, float *out, double *workspace, int N,
                               int HW, int C, int G, float eps, int64_t x_image_stride, int64_t out_image_stride, void *stream);

/*
 * GroupNorm of up to 8 pyramid levels in TWO launches, written into one token buffer: out [N, S, C] (image n at out + n *
 * out_image_stride floats), level l normalised into the rows row0 .. row0 + HW - 1 of every image -- the reference's input projections
 * followed by the flatten + concatenation in front of the encoder (models/deformable_detr.py:73-90, models/deformable_transformer.py:
 * 139-156).  Per level:
 *   pieces == 1   src is y [N, HW, C] (dense: image n at src + n HW C), read by both passes; bias is ignored
 *   pieces  > 1   src holds the split-K partial sums [pieces][N HW C] a GEMM left behind (tf_conv_packed_partials_f32).  The statistics
 *                 pass forms y = ((p0 + p1) + ... + p_last) + bias -- the order of the GEMM's own second pass: bit-identical y --, stores
 *                 it at the level's output rows, and the second pass normalises it in place.  bias [C] or NULL.
 * Statistics as tf_groupnorm_nhwc_f32 (every element widened to double before it is squared and summed; biased variance, clamped at
 * 0; rstd = 1 / sqrt(var + eps) in double), but summed in a fixed order without atomics: two calls give the same bits.  Every
 * operation is rounded on its own (no fused multiply-add).  workspace: tf_groupnorm_levels_workspace_doubles(...) doubles, 16-byte
 * aligned, every one written by the call (nothing to clear); -1 for arguments the entry rejects.
 * C % 4 == 0, C <= 1024, G <= 256 dividing C, N <= 65535, out_image_stride % 4 == 0 and >= (row0 + HW) C for every level; the levels'
 * row ranges must not overlap and no src may lie inside out; 16-byte aligned pointers.  The table is read during the call.
 * NULL pointer -> TF_MSDA_ERR_NULL_POINTER, then dimensions / alignment -> TF_MSDA_ERR_BAD_DIMS, before any GPU work.
 */
typedef struct tf_gn_level {
    const float *src;
    const float *bias;
    const float *gamma;
    const float *beta;
    int pieces;
    int HW;
    int64_t row0;
} tf_gn_level;
int64_t tf_groupnorm_levels_workspace_doubles(const tf_gn_level *levels, int nlevels, int N, int C, int G);
int tf_groupnorm_levels_nhwc_f32(const tf_gn_level *levels, int nlevels, int N, int C, int G, float eps, float *out,
                                 int64_t out_image_stride, double *workspace, void *stream);

/*
 * The FPN merge of the mask head in one pass (reference: models/detr_segmentation.py:142-156 `_expand(adapter(fpn), Q) +
 * F.interpolate(x, size=fpn.shape[-2:], mode="nearest")`): out[n, y, x, c] = low[n, ys, xs, c] + fpn[n / q_per_image, y, x, c] with
 * ys = min(floorf(y * (float)h / H), h - 1), xs likewise (torch's legacy "nearest" index).  low [N, h, w, C], fpn [N / q_per_image, H,
 * W, C], out [N, H, W, C] -- the storage of channels_last NCHW tensors; C % 4 == 0, 16-byte aligned.  The reference's two passes
 * write and re-read the up-sampled tensor (1.1 GB per 128 queries at the finest level of an 800 x 1333 frame).  Any size pair (up-,
 * down-sampling, identity).  Non-finite operands: one IEEE addition per element (NaN and inf - inf = NaN propagate), bit-identical to
 * the two ATen passes.
 */
int tf_upsample_add_nhwc_f32(const float *low, const float *fpn, float *out, int N, int q_per_image, int h, int w, int H, int W, int C,
                             void *stream);

/*
 * A 3 x 3 / padding 1 convolution (split product, halo form) whose input is the mask head's FPN merge, computed in the convolution's
 * fetch and never written (reference: models/detr_segmentation.py:142-156 `x = adapter(fpn) + F.interpolate(x, size=fpn.shape[-2:])`,
 * `x = lay(x)`): input pixel (y, x), channel c of image n = act(low[n, ys, xs, c]) + fpn[n / q_per_image, y, x, c], (ys, xs) torch's
 * legacy nearest index.  act = identity when gn_workspace is NULL; else relu(GroupNorm(low)) from RAW statistics (the 2 * nimg * groups
 * doubles tf_groupnorm_*'s statistics pass leaves: sum | sum of squares per (image, group) over lh * lw * cin / groups values) -- the
 * previous layer's GroupNorm + ReLU folded in as well.  low [nimg, lh, lw, cin], fpn [nimg / q_per_image, H, W, cin], y [nimg, H, W,
 * cout]; cin % 32 == 0, cin <= 320; w_packed: tf_linear_pack_weight_f32 of the [cout, 9 * cin] tap-major weight.
 */
int tf_conv3x3_merge_packed_f32(const float *low, const float *fpn, const double *gn_workspace, const float *gamma, const float *beta,
                                int groups, float eps, const void *w_packed, const float *bias, float *y, int nimg, int q_per_image, int lh,
                                int lw, int H, int W, int cin, int cout, int relu, int terms, void *stream);

/*
 * The end of the mask head in one pass over the last hidden activation (reference: models/detr_segmentation.py:157-160
 * `out_lay(F.relu(gn5(x)))`, a 3 x 3 convolution to ONE channel, padding 1): statistics of x [N, H, W, C] per (image, group) as
 * tf_groupnorm_nhwc_f32 computes them (workspace: 2 * N * G doubles, zeroed by the call), then out[n, y, x] = bias + sum over the
 * 3 x 3 taps and C channels of relu(gn(x))[n, y + dy, x + dx, c] * weight[(dy, dx), c] in fp32 (zero outside the image); the
 * normalised activation is never written.  weight [9, C] tap-major (the [1, C, 3, 3] weight permuted to [3, 3, C]); C in {16, 32},
 * G divides C; 16-byte aligned pointers.
 */
int tf_groupnorm_relu_conv3x3_c1_nhwc_f32(const float *x, const float *gamma, const float *beta, const float *weight, float bias,
                                          float *out, double *workspace, int N, int H, int W, int C, int G, float eps, void *stream);

/*
 * The tracker's mask post-processing in one pass (reference: models/detr_segmentation.py PostProcessSegm.forward -- bilinear resize
 * of the mask logits to the padded batch size, sigmoid, crop of the padding, nearest resize to the original image size -- followed by
 * models/tracker.py:521-532: a pixel belongs to the track with the largest probability there if that probability exceeds the
 * threshold).  logits [n, h, w] (mask-head outputs of n queries), order [n_tracks]: the row of `logits` that is track i's mask (-1: the
 * track has none); label [out_h, out_w] int16: the owning track's index or -1.  Per output pixel: its nearest source pixel in the
 * (img_h, img_w) crop of the (pad_h, pad_w) grid (torch's legacy "nearest" index), there the bilinear sample of every track's logits
 * (align_corners = False, torch's arithmetic operation by operation), its sigmoid; ties go to the first track, as torch.max.
 * n_tracks <= 32767, img <= pad in both directions; any threshold.  Non-finite logits as the chain `stack -> max -> best > threshold`
 * has them: a pixel where ANY track's probability is NaN (a NaN logit under one of its four taps, inf - inf between taps, or 0 * inf
 * at a tap of weight exactly 0) is -1, because torch.max returns the NaN and NaN > threshold is false; +inf samples give probability
 * exactly 1, -inf exactly 0.
 * The reference's chain writes and re-reads n full-size fp32 maps (~0.9 GB per frame at 100 tracks and 1080 x 1920).
 */
int tf_mask_label_map_f32(const float *logits, const int *order, int16_t *label, int n_tracks, int h, int w, int pad_h, int pad_w, int img_h,
                          int img_w, int out_h, int out_w, float threshold, void *stream);

/*
 * THE SPLIT PRODUCT (every matrix-core kernel below; trackformer_amd/csrc/split_product.h).  fp32 operands are cut into 16-bit
 * pieces (round to nearest even, residuals exact in fp32) and a product x . w is formed from v_mfma_f32_32x32x16_{bf16,f16}
 * terms with fp32 accumulation, smallest terms first.  The reference computes these layers in fp32 (nn.Linear / Conv2d;
 * models/ops/src/cuda/ms_deform_attn_cuda.cu:69 dispatches on fp32 tensors, no autocast anywhere).
 *   terms = 6   bf16 pieces hi, mid, lo of both operands:  x_lo.w_hi + x_hi.w_lo + x_mid.w_mid + x_mid.w_hi + x_hi.w_mid + x_hi.w_hi
 *               The three pieces carry all 24 significand bits; the dropped terms are below 2^-24 |x||w|: fp32 arithmetic in
 *               another summation order.
 *   terms = 16  fp16 pieces:  activation  xh = f16(x / 16),  xl = f16((x / 16 - xh) 2^11)
 *                             weight      wh = f16(w t_n),   wl = f16(w t_n - wh)
 *               three terms  xl.(wh 2^-11) + xh.wl + xh.wh,  result times r_n = 16 / t_n  (wh 2^-11 is formed in registers from the
 *               wh fragment: exact).  Two fp16 pieces carry 22 significand bits + the
 *               sign of the lower one (error of an operand <= 2^-23 of it); the only dropped product (lo.lo) is below 2^-22 |x||w|.
 *               t_n: the power of two that puts the largest |w| of output channel n into [2^13, 2^14) -- with the lower
 *               activation piece stored times 2^11 nothing falls into fp16's subnormals (|x| < 1.0e6; beyond that the row becomes
 *               NaN instead of saturating).  Half the matrix work of terms = 6 at fp32-class accuracy (against float64 on random
 *               operands: 3.7e-8 of sum |x||w| for the representation; the fp32 rounding of the sum itself is 2.4e-7).
 *   (terms = 3, two bf16 pieces and three terms with products good to 2^-16 -- the "fast mode" of rounds 2-4 -- was REMOVED in
 *   round 5: the fp16 product runs at the same speed with fp32-class accuracy, and three bf16 terms lost the reference's track ids
 *   at frame 14 of the 64-frame fixture, profiles/r04_id_parity_64.txt.  terms = 3 / (w_hi, w_mid) alone is TF_MSDA_ERR_BAD_DIMS.)
 * Entry points that take the weight as separate piece tensors (16-bit [N, K] each, made once by the caller) select by which are
 * given:  (w_hi, w_mid, w_lo)                 bf16 hi, mid, lo               -> six terms
 *         (w_hi, w_mid, NULL, w_scale)        fp16 wh, wl + r_n [N] fp32     -> the fp16 product
 * Entry points that take a PACKED weight select by `terms` (6 or 16), which must be the value the weight was packed with
 * (tf_linear_pack_weight_f32 computes t_n / r_n itself).  x is split inside the kernels.
 */

/*
 * y[M, N] = x[M, K] . w[N, K]^T + bias[N] (bias may be NULL), ReLU if relu != 0; fp32 in and out, row-major.
 * K % 32 == 0, 16-byte aligned x / w_hi / w_mid / w_lo; w_lo, w_scale: see THE SPLIT PRODUCT.  (trackformer_amd/csrc/linear_split.hip)
 */
int tf_linear_split_f32(const float *x, const void *w_hi, const void *w_mid, const void *w_lo, const float *w_scale, const float *bias,
                        float *y, int64_t M, int K, int N, int relu, void *stream);

/*
 * The same product with a residual in the epilogue: y = act(x . w^T + bias + residual), residual [M, N] fp32 (may alias y).
 * For the 1 x 1 convolutions that close a ResNet bottleneck (conv3 -> FrozenBatchNorm2d -> `out += identity` -> ReLU;
 * reference: models/backbone.py:45-55 + torchvision's Bottleneck.forward): on channels_last activations a stride-1 1 x 1
 * convolution IS this GEMM with M = N_img * H * W rows, the BN scale folded into w and its shift as bias.
 */
int tf_linear_split_res_f32(const float *x, const void *w_hi, const void *w_mid, const void *w_lo, const float *w_scale, const float *bias,
                            const float *residual, float *y, int64_t M, int K, int N, int relu, void *stream);

/*
 * 3 x 3 convolution (padding 1, stride 1 or 2, no groups / dilation) of a channels_last activation as the same split
 * product (an implicit GEMM over the output pixels, K = 9 * Cin): y[n, ho, wo, :] = act(sum_taps x[n, hi, wi, :] . w[:, tap, :]^T
 * + bias).  x [N, Hin, Win, Cin] and y [N, Hout, Wout, Cout] are NHWC (the storage of channels_last NCHW tensors); the weight
 * arrives as bf16 pieces of the [Cout, 3, 3, Cin] tensor (the storage of a channels_last OIHW weight), Cin % 32 == 0.
 * For torchvision's Bottleneck.conv2 + FrozenBatchNorm2d + ReLU (BN scale folded into w, shift as bias).  Input, output and
 * weight pieces below 3 GiB each (buffer-resource offsets), else TF_MSDA_ERR_BAD_DIMS.
 */
int tf_conv3x3_split_f32(const float *x, const void *w_hi, const void *w_mid, const void *w_lo, const float *w_scale, const float *bias,
                         float *y, int nimg, int hin, int win, int cin, int cout, int stride, int relu, void *stream);
/* The same convolution with the K loop (9 Cin) cut into `ksplit` pieces that run as separate workgroups -- for few output
 * pixels under a long K (the extra pyramid level of deformable_detr.py:55-79: 2048 -> 256 at 13 x 21; layer4's 3 x 3
 * convolutions).  The pieces write partial sums to `workspace` (ksplit * N*Hout*Wout * cout floats, 16-byte aligned), a second
 * launch adds them in a fixed order (deterministic, unlike atomics) and applies bias / ReLU.  ksplit in 1..64 (1: no workspace
 * needed, identical to tf_conv3x3_split_f32); cout % 4 == 0 and 16-byte aligned y / bias when ksplit > 1. */
int tf_conv3x3_splitk_f32(const float *x, const void *w_hi, const void *w_mid, const void *w_lo, const float *w_scale, const float *bias,
                          float *y, float *workspace, int ksplit, int nimg, int hin, int win, int cin, int cout, int stride, int relu,
                          void *stream);
/* The same kernel for a strided 1 x 1 convolution without padding (w [Cout, Cin]): the projections of the identity branch
 * (torchvision Bottleneck.downsample, stride 2) -- the rows of the GEMM are every stride-th pixel. */
int tf_conv1x1_strided_split_f32(const float *x, const void *w_hi, const void *w_mid, const void *w_lo, const float *w_scale,
                                 const float *bias, float *y, int nimg, int hin, int win, int cin, int cout, int stride, int relu,
                                 void *stream);
/* The 1 x 1 convolution (stride 1 or 2, w [Cout, Cin]) with the K loop (Cin) cut into `ksplit` pieces, as tf_conv3x3_splitk_f32:
 * ResNet-50's reducing 1 x 1 convolutions of layer3 / layer4 (torchvision Bottleneck.conv1: 1024 -> 256 at 50 x 84, 2048 -> 512 at
 * 25 x 42 for an 800 x 1333 frame) are 132 / 68 workgroups of 32 / 64 K-slices -- fewer than the chip has CUs. */
int tf_conv1x1_splitk_f32(const float *x, const void *w_hi, const void *w_mid, const void *w_lo, const float *w_scale, const float *bias,
                          float *y, float *workspace, int ksplit, int nimg, int hin, int win, int cin, int cout, int stride, int relu,
                          void *stream);

/*
 * The backbone's first convolution (7 x 7, stride 2, padding 3, 3 -> 64 channels; reference: models/backbone.py:93-104 ->
 * torchvision resnet50.conv1) as a split product on the matrix cores (trackformer_amd/csrc/stem_conv.hip).
 *   x         [N, 3, H, W] fp32, planar (NCHW)
 *   w_packed  tf_linear_pack_weight_f32(K = 176, N = 64, terms) of the [64, 176] matrix w2[o][(c * 7 + ky) * 8 + kx] = w[o][c][ky][kx]
 *             (kx = 7 and k >= 168: zeros) -- with a following FrozenBatchNorm2d's scale folded in by the caller
 *   bias      [64] or NULL (the FrozenBatchNorm2d shift), relu != 0: ReLU
 *   y         [N, (H - 1) / 2 + 1, (W - 1) / 2 + 1, 64] fp32, channels_last
 */
int tf_stem_conv7x7_f32(const float *x, const void *w_packed, const float *bias, float *y, int N, int H, int W, int relu,
                        int terms, void *stream);

/*
 * out[n, oy, ox, c] = max over the 3 x 3 window (stride 2, padding 1) of relu(x[n, iy, ix, c] + bias[c]) on channels_last
 * activations: FrozenBatchNorm2d shift + ReLU + MaxPool2d(3, 2, 1) after the backbone's first convolution (reference:
 * models/backbone.py:45-55, torchvision ResNet.relu / .maxpool) in one pass.  x [N, H, W, C], out [N, (H - 1) / 2 + 1,
 * (W - 1) / 2 + 1, C], C % 4 == 0, 16-byte aligned pointers, fewer than 2^31 output quads.  Bit-identical to the separate passes,
 * non-finite operands included: the shift is added to every window element before the maximum, a NaN anywhere in the window (NaN
 * input, NaN shift, -inf under a shift of +inf) is the window's maximum as in torch's max_pool2d, and the ReLU (`v < 0 ? 0 : v`)
 * keeps it.  Zeros: the ReLU keeps -0.0 (relu(-0.0 + -0.0) = -0.0), which is torch.relu on the CPU; torch.relu on MI355X returns +0.0
 * there, so against the ATen chain ON THE DEVICE the output differs in the sign of such zeros and in nothing else.  The sign of a zero
 * maximum over a window that holds both +0.0 and -0.0 follows the order of the scan and is not part of the contract.
 */
int tf_bias_relu_maxpool_f32(const float *x, const float *bias, float *out, int N, int H, int W, int C, void *stream);

/* y[M, N] = (x + x2)[M, K] . w^T + bias: tf_linear_split_f32 with an element-wise add in front, done as the activation tile is
 * staged -- `with_pos_embed(src, pos)` + a projection (models/deformable_transformer.py:279-283, ms_deform_attn.py:67-72)
 * without a separate pass over the tokens.  Bit-identical to adding first. */
int tf_linear_split_add_f32(const float *x, const float *x2, const void *w_hi, const void *w_mid, const void *w_lo, const float *w_scale,
                            const float *bias, float *y, int64_t M, int K, int N, void *stream);

/*
 * The same product with the weight in PACKED form (trackformer_amd/csrc/linear_stream.hip): the weight is split into
 * its bf16 pieces once and stored in matrix-core fragment order, so that the GEMM streams it from L2 into registers and
 * only the activations pass through LDS.  Results are bit-identical to tf_linear_split_f32 with the same number of terms.
 *   tf_linear_packed_bytes(K, N, terms)          size of the packed buffer (N padded to a multiple of 256; terms = 16: + a float
 *                                                per padded output channel behind the fragments), or -1; K % 16 == 0
 *   tf_linear_pack_weight_f32(w, packed, ...)    w [N, K] fp32 row-major -> packed (16-byte aligned pointers); one small kernel
 *   tf_linear_packed_f32                         y[M, N] = act(x[M, K] . w^T + bias + residual); K % 64 == 0, 16-byte aligned x;
 *                                                bias / residual [M, N] may be NULL, residual may alias y; y below 3 GiB
 * terms: 6 or 16 (see THE SPLIT PRODUCT above); a weight packed for 6 holds three pieces per fragment, for 16 two.
 * The residual form is the closing 1 x 1 convolution of a ResNet bottleneck (conv3 -> FrozenBatchNorm2d -> `out += identity` ->
 * ReLU; reference: models/backbone.py:45-55 + torchvision's Bottleneck.forward) on channels_last activations.
 */
int64_t tf_linear_packed_bytes(int K, int N, int terms);
int tf_linear_pack_weight_f32(const float *w, void *packed, int K, int N, int terms, void *stream);
int tf_linear_packed_f32(const float *x, const void *w_packed, const float *bias, const float *residual, float *y, int64_t M, int K,
                         int N, int relu, int terms, void *stream);

/*
 * THE BACKWARD OF A LINEAR  y[M, N] = x[M, K] . w[N, K]^T + b[N]  as split products (trackformer_amd/csrc/linear_bwd.h; reference: the
 * autograd of the nn.Linear layers of models/deformable_transformer.py / models/ops/modules/ms_deform_attn.py, fp32):
 *     dx[M, K] = dy[M, N] . w[N, K]            db[N] = sum_m dy[m, n]            dw[N, K] = sum_m dy[m, n] x[m, k]
 * Scaling.  The forward's fp16 scheme (terms = 16) is cut for O(1) activations: a fixed 2^-4, |x| < 1.0e6.  Gradients have no such
 * range, so the operands of a backward product get powers of two per call, found on the device from their largest magnitudes and
 * written to device memory (no host synchronisation):
 *     role 0 (the operand split as the ACTIVATION: dy): scale2 = {s, 1 / s}; s puts amax|a| of the MATRIX into [2^14, 2^15) -- after the
 *            scheme's 2^-4 the hi piece stays below 2^11.  (One scale: the columns of dy are the contraction of the input gradient.)
 *     role 1 (the operand split as the WEIGHT: x):      scale2 = t[C] | 1 / t[C] (2 C floats, 16-byte aligned); t_c puts the largest
 *            magnitude of COLUMN c into [2^13, 2^14): column k of x is output channel k of dw, what t_n is per output channel in the
 *            forward (a column of fp32 subnormals keeps its bits).
 * A scale depends on the exponent of its amax alone (a -> 2^k a gives s -> 2^-k s exactly; every result below is scale-equivariant bit
 * for bit while nothing leaves fp32's range); it is 1 for an all-zero matrix / column and for one that holds a NaN or an inf; 1 always under
 * terms = 6 (bf16 pieces have fp32's exponent range).  The operand is multiplied by s as it is staged, the result by the inverse
 * in the epilogue: both exact.  An element below 2^-25 of its matrix's amax is held to an absolute 2^-32 / s (THE SPLIT PRODUCT).
 * No atomics anywhere: sums over rows are two-stage reductions in a fixed order, so every result is a pure function of the
 * arguments -- bit-identical from call to call, on any stream and in a captured HIP graph.
 * Non-finite operands: an output whose exact value is NaN or +-inf is non-finite.  Nothing is promised about which OTHER outputs stay
 * finite (a non-finite amax switches the scaling off).
 *
 *   tf_linear_grad_stats_f32     one pass over a[M, C]: scale2 for `role` (0 / 1), and, if colsum != NULL, colsum[c] = sum_m a[m, c]
 *                                (the bias gradient when a = dy), summed in a fixed order.  C % 4 == 0, a / scale2 / colsum 16-byte
 *                                aligned.  workspace: tf_linear_grad_stats_workspace_bytes(M, C, role, colsum != NULL) bytes, 16-byte
 *                                aligned (4 bytes per row block, rounded up to 16, + a row of C floats per row block with colsum, + one
 *                                more for role 1; row blocks: ceil(M / 64) up to 32 768 rows, 512 beyond).
 *   tf_linear_wgrad_split_f32    dw from dy (role 0, scale dy_scale2) and x (role 1, scale x_scale2); fp16 scheme: the epilogue
 *                                multiplies dw[n, k] by 16 / (s t_k).  The row loop is cut into `msplit` chunks that run as separate workgroups
 *                                and write partial sums to `workspace`; a second launch adds them in the order 0, 1, ...  msplit is a
 *                                function of (M, K, N) only (tf_msda_set_option("wgrad_msplit", n) forces it; 0: per shape);
 *                                tf_linear_wgrad_workspace_bytes(M, K, N) = msplit N K 4 bytes (0 for msplit == 1: workspace may be
 *                                NULL), 16-byte aligned.  K % 4 == 0, N % 4 == 0, 16-byte aligned dy / x / dw, dy / x / dw below
 *                                3 GiB each, else TF_MSDA_ERR_BAD_DIMS.  Rows at or beyond M are never read.
 *   tf_linear_dgrad_packed_f32   dx = dy . w: tf_linear_packed_f32 with dy as the activation and wt_packed =
 *                                tf_linear_pack_weight_f32(w^T [K, N] row-major, K = N, N = K, terms); dy is multiplied by s as it
 *                                is staged and the result by 1 / s: bit-identical to (1 / s) . tf_linear_packed_f32(s dy, wt_packed).
 *                                dy_scale2 may be NULL (no scaling).  N % 64 == 0, 16-byte aligned dy / wt_packed, dx below 3 GiB.
 *   tf_linear_dgrad_splitk_packed_f32  the same product with the contraction over N cut into ksplit (1 .. 64) pieces, the stream GEMM's
 *                                split-K: every piece's partial sum leaves its workgroup multiplied by 1 / s into workspace (ksplit M K
 *                                floats), a second launch adds the pieces in the order 0, 1, ...; no accumulator walks the whole sum
 *                                (the matrix cores do not add in round-to-nearest: a long chain collects a one-sided error).
 *                                ksplit = 1: the bits of tf_linear_dgrad_packed_f32, workspace may be NULL.  ksplit > 1 also needs
 *                                K % 4 == 0 and 16-byte aligned dx / workspace.  Checked in this order: NULL dy / wt_packed / dx, or a
 *                                NULL workspace with ksplit > 1 -> TF_MSDA_ERR_NULL_POINTER; dimensions, ksplit, alignment (workspace
 *                                included) -> TF_MSDA_ERR_BAD_DIMS.
 * Checked in this order, before any GPU work: NULL pointer -> TF_MSDA_ERR_NULL_POINTER, dimensions / alignment -> TF_MSDA_ERR_BAD_DIMS,
 * workspace too small or misaligned -> TF_MSDA_ERR_WORKSPACE.  The *_workspace_bytes functions return -1 for dimensions the entry
 * point rejects.
 */
int64_t tf_linear_grad_stats_workspace_bytes(int64_t M, int C, int role, int with_colsum);
int tf_linear_grad_stats_f32(const float *a, float *scale2, float *colsum, void *workspace, int64_t workspace_bytes, int64_t M, int C,
                             int role, int terms, void *stream);
int64_t tf_linear_wgrad_workspace_bytes(int64_t M, int K, int N);
int tf_linear_wgrad_split_f32(const float *dy, const float *x, const float *dy_scale2, const float *x_scale2, float *dw, void *workspace,
                              int64_t workspace_bytes, int64_t M, int K, int N, int terms, void *stream);
int tf_linear_dgrad_packed_f32(const float *dy, const float *dy_scale2, const void *wt_packed, float *dx, int64_t M, int K, int N,
                               int terms, void *stream);
int tf_linear_dgrad_splitk_packed_f32(const float *dy, const float *dy_scale2, const void *wt_packed, float *dx, float *workspace, int ksplit,
                                      int64_t M, int K, int N, int terms, void *stream);

/*
 * THE BACKWARD OF A 3 x 3 CONVOLUTION  y = conv3x3(x, w), padding 1, stride s, no groups, no dilation  as split products
 * (trackformer_amd/csrc/conv_bwd.h; reference: the autograd of the Bottleneck conv2 layers of models/backbone.py's ResNet-50, fp32).
 * Every tensor is NHWC fp32 (the storage of a channels_last tensor): x [nimg, hin, win, cin], dy [nimg, hout, wout, cout] with
 * hout = (hin - 1) / s + 1, wout = (win - 1) / s + 1; the weight is [cout, 3, 3, cin], tap-major (the storage of a channels_last OIHW
 * weight).  With M = nimg hout wout output pixels m = (n, ho, wo):
 *     dw[co, ky, kx, ci] = sum_m dy[m, co] x[n, ho s + ky - 1, wo s + kx - 1, ci]         (input pixels outside the image: exact zeros)
 *     dx = conv3x3(dy, w_rot),  w_rot[ci, ky, kx, co] = w[co, 2 - ky, 2 - kx, ci]          (s = 1)
 * These are the two products of THE BACKWARD OF A LINEAR on the unfolded matrix U[M, 9 cin] (tap-major columns, zeros at the borders),
 * which is never materialised; scaling, the absence of atomics and the behaviour on non-finite operands are as stated there.
 *
 *   tf_conv3x3_wgrad_split_f32   s = 1 or 2.  dy is split as the activation (role 0, dy_scale2 = {s, 1 / s} from tf_linear_grad_stats_f32 of
 *                                dy viewed as [M, cout]); x as the weight (role 1, x_scale2 = t[cin] | 1 / t[cin] from
 *                                tf_linear_grad_stats_f32 of x viewed as [nimg hin win, cin]: one scale per input channel, shared by the
 *                                nine taps).  The kernel is the one of tf_linear_wgrad_split_f32 (128 x 128 outputs per workgroup, slices of
 *                                32 pixels) with the row address of x replaced: column k of the tile decodes once per thread into
 *                                (tap, ci), a row m into (n, ho, wo) once per 8 rows; a shifted pixel that leaves the image contributes a
 *                                zero and is never read.  Epilogue (fp16 scheme): 16 / (s t_ci).  The pixel loop is cut into the chunks of
 *                                tf_linear_wgrad_split_f32 for (M, K = 9 cin, N = cout) -- the same rule, the same "wgrad_msplit" knob, the
 *                                same second launch; tf_conv3x3_wgrad_workspace_bytes(...) = msplit cout 9 cin 4 bytes (0 for one chunk:
 *                                workspace may be NULL).  Summation order per output: m ascending, per 16 pixels smallest term first; then
 *                                the chunks in order.  The result equals tf_linear_wgrad_split_f32(dy, U, dy_scale2, x_scale2 repeated
 *                                nine times) BIT FOR BIT, for both term schemes.
 *                                cin % 4 == 0, cout % 4 == 0, 16-byte aligned dy / x / dw / x_scale2 / workspace, dy / x / dw below
 *                                3 GiB each, M < 2^31, else TF_MSDA_ERR_BAD_DIMS.
 *   tf_conv3x3_dgrad_packed_f32  stride 1 only (hout = hin = h, wout = win = w).  wrot_packed = tf_linear_pack_weight_f32(w_rot viewed as
 *                                [cin, 9 cout], K = 9 cout, N = cin, terms).  This is tf_conv_packed_f32(ks = 3, stride = 1) with dy as
 *                                the input and the same (workspace, ksplit), in the kernels' scaled-activation instantiation: dy is
 *                                multiplied by s as it is staged, the result by 1 / s -- with ksplit = 1 bit-identical to
 *                                (1 / s) . tf_conv_packed_f32(s dy, wrot_packed).  ksplit in 2 .. 64 cuts the contraction of 9 cout
 *                                products into pieces as tf_conv_packed_f32 does (workspace: ksplit . nimg h w cin floats, 16-byte
 *                                aligned; one fp32 accumulator then walks a piece, not the whole sum): every piece leaves its
 *                                workgroup multiplied by 1 / s and the second pass adds them in the order 0, 1, ... -- the bits of
 *                                (1 / s) . tf_conv_packed_f32(s dy, wrot_packed, ksplit) unless a partial sum is an fp32 subnormal.  BOTH
 *                                forms of that entry point take the scaled instantiation with the same bits, so the choice is
 *                                tf_conv_packed_f32's own: the HALO form unless tf_msda_set_option("conv_halo", 0) selects the plain
 *                                stream form (the two differ in summation order; the identity above holds under either setting).
 *                                dy_scale2 may be NULL (no scaling: tf_conv_packed_f32 itself).
 *                                cout % 64 == 0, cin % 4 == 0, 16-byte aligned dy / wrot_packed / dx, dy and dx (+ 256 rows) below 3 GiB.
 * Checked before any GPU work.  tf_conv3x3_wgrad_split_f32, in this order: NULL pointer -> TF_MSDA_ERR_NULL_POINTER, dimensions /
 * alignment -> TF_MSDA_ERR_BAD_DIMS, workspace NULL, too small or misaligned -> TF_MSDA_ERR_WORKSPACE; tf_conv3x3_wgrad_workspace_bytes
 * returns -1 for dimensions the entry point rejects.  tf_conv3x3_dgrad_packed_f32, in this order (as tf_conv_packed_f32, whose
 * workspace has no size argument): NULL dy / wrot_packed / dx, or a NULL workspace with ksplit > 1 -> TF_MSDA_ERR_NULL_POINTER;
 * dimensions, ksplit outside 1 .. 64, alignment (a misaligned workspace included) -> TF_MSDA_ERR_BAD_DIMS.
 */
int64_t tf_conv3x3_wgrad_workspace_bytes(int nimg, int hin, int win, int cin, int cout, int stride);
int tf_conv3x3_wgrad_split_f32(const float *dy, const float *x, const float *dy_scale2, const float *x_scale2, float *dw, void *workspace,
                               int64_t workspace_bytes, int nimg, int hin, int win, int cin, int cout, int stride, int terms, void *stream);
int tf_conv3x3_dgrad_packed_f32(const float *dy, const float *dy_scale2, const void *wrot_packed, float *dx, float *workspace, int ksplit,
                                int nimg, int h, int w, int cin, int cout, int terms, void *stream);

/*
 * THE BACKWARD OF THE STRIDE-2 CONVOLUTIONS  (trackformer_amd/csrc/conv_strided_bwd.h; reference: the autograd of the first bottleneck of
 * ResNet-50's layer2-4 in models/backbone.py: its 3 x 3 conv2, padding 1, and the 1 x 1 projection of its identity branch, no padding).
 * Tensors as in the section above: x / dx [nimg, h, w, cin], dy [nimg, ho, wo, cout], ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1.
 *
 *   tf_conv_dgrad_stride2_packed_f32   ks = 3: the weight is [cout, 3, 3, cin];  ks = 1: [cout, cin].
 *       The input pixel (iy, ix) = (2 a + py, 2 b + px) belongs to the parity class c = 2 py + px, which has
 *       ceil((h - py) / 2) x ceil((w - px) / 2) pixels per image and T_c = (1 + py)(1 + px) taps:
 *           dx[n, 2 a + py, 2 b + px, ci] = sum over the class's taps (da, db) and co of  dy[n, a + da, b + db, co] w[co, ky, kx, ci]
 *           py = 0: da = 0 with ky = 1;   py = 1: da = 0 with ky = 2, then da = 1 with ky = 0;   (db, kx) from px alike
 *       -- a dy row a + 1 = ho or column b + 1 = wo is an exact zero that is never read (not the next row, not the next image).  ks = 1
 *       is the class (0, 0) alone, dx[n, 2 a, 2 b] = dy[n, a, b] . w; the pixels of the other three classes are written as +0.
 *       wcls_packed holds the class weights one behind the other, c = 0, 1, 2, 3 (ks = 1: c = 0 only): class c is
 *       tf_linear_pack_weight_f32 of W_c [cin, T_c cout] with K = T_c cout, N = cin, where column (t cout + co) of W_c is
 *       w[co, ky, kx, ci] for the t-th tap of the class in the order (da, db) = (0, 0), (0, 1), (1, 0), (1, 1) restricted to the class;
 *       the image of class c starts tf_linear_packed_bytes(T_c' cout, cin, terms) bytes behind that of each class c' < c.
 *       Each class is one launch of tf_conv_packed_f32's stream form (a stride-1 window of T_c taps over dy, no padding) in the
 *       scaled-activation instantiation of tf_conv3x3_dgrad_packed_f32: dy is multiplied by s as it is staged, every partial sum leaves
 *       its workgroup multiplied by 1 / s (dy_scale2 = {s, 1 / s}; NULL: the plain instantiation).  The contraction of the longest class
 *       is cut into ksplit pieces (1 .. 64), that of the others in proportion (ceil(ksplit T_c / 4)), never below 64 products per
 *       piece; the launches write compact class images into `workspace` (tf_conv_dgrad_stride2_workspace_bytes(...), 16-byte aligned,
 *       needed for every ksplit), and ONE further launch writes every element of dx exactly once: the pieces of its class added in
 *       the order 0, 1, ...  No zero-inserted copy of dy, no atomics; the order of every sum is a function of the arguments' shape.
 *       Per class the result equals (1 / s) . tf_conv_packed_f32-style products of s dy: the bound of THE BACKWARD OF A LINEAR with
 *       the contraction length T_c cout.
 *       cout % 64 == 0, cin % 4 == 0, 16-byte aligned dy / wcls_packed / dx / workspace, dy and dx (+ 256 rows) below 3 GiB.
 *   tf_conv1x1_strided_wgrad_split_f32   dw[co, ci] = sum_m dy[m, co] x[n, 2 ho, 2 wo, ci], m = (n, ho, wo), stride = 2 only (any other
 *       value: TF_MSDA_ERR_BAD_DIMS -- the stride-1 1 x 1 is tf_linear_wgrad_split_f32 on the pixel matrix): the kernel of
 *       tf_linear_wgrad_split_f32 with the row address of x replaced, as tf_conv3x3_wgrad_split_f32 but without taps or padding.
 *       dy_scale2 from tf_linear_grad_stats_f32 of dy [M, cout] (role 0), x_scale2 = t[cin] | 1 / t[cin] of x viewed as
 *       [nimg hin win, cin] (role 1: one scale per input channel over ALL pixels of x).  The chunks of the pixel loop, the
 *       "wgrad_msplit" knob and the second launch are those of tf_linear_wgrad_split_f32 for (M, K = cin, N = cout);
 *       tf_conv1x1_strided_wgrad_workspace_bytes(...) = msplit cout cin 4 bytes (0 for one chunk).  The result equals
 *       tf_linear_wgrad_split_f32(dy, G, dy_scale2, x_scale2) on the gathered matrix G[M, cin] BIT FOR BIT; G is never built.
 *       cin % 4 == 0, cout % 4 == 0, 16-byte aligned dy / x / dw / x_scale2 / workspace, dy / x / dw below 3 GiB each.
 * Checked before any GPU work, in this order: NULL pointer (tf_conv_dgrad_stride2_packed_f32: dy / wcls_packed / dx / workspace;
 * the weight gradient: all but the workspace) -> TF_MSDA_ERR_NULL_POINTER; dimensions, ks, ksplit outside 1 .. 64, unknown terms,
 * alignment -> TF_MSDA_ERR_BAD_DIMS; workspace too small (the weight gradient: NULL or misaligned too) -> TF_MSDA_ERR_WORKSPACE.  The
 * ..._workspace_bytes functions return -1 for dimensions their entry point rejects.
 */
int64_t tf_conv_dgrad_stride2_workspace_bytes(int nimg, int h, int w, int cin, int cout, int ks, int ksplit);
int tf_conv_dgrad_stride2_packed_f32(const float *dy, const float *dy_scale2, const void *wcls_packed, float *dx, void *workspace,
                                     int64_t workspace_bytes, int ksplit, int nimg, int h, int w, int cin, int cout, int ks, int terms,
                                     void *stream);
int64_t tf_conv1x1_strided_wgrad_workspace_bytes(int nimg, int hin, int win, int cin, int cout, int stride);
int tf_conv1x1_strided_wgrad_split_f32(const float *dy, const float *x, const float *dy_scale2, const float *x_scale2, float *dw,
                                       void *workspace, int64_t workspace_bytes, int nimg, int hin, int win, int cin, int cout, int stride,
                                       int terms, void *stream);

/*
 * THE BACKWARD OF THE RESIDUAL LAYERNORM  out = LayerNorm(x + res) gamma + beta  (trackformer_amd/csrc/layernorm_bwd.h; reference: the
 * autograd of `src = src + dropout(src2); src = norm(src)` of models/deformable_transformer.py, fp32).  With z = x + res (z = x for
 * res == NULL), mean / rstd = 1 / sqrt(var + eps) of the row, xh = (z - mean) rstd and g = gamma dy:
 *     dz[r, :]  = rstd (g - mean_c(g) - xh mean_c(g xh))        dgamma[c] = sum_r dy[r, c] xh[r, c]        dbeta[c] = sum_r dy[r, c]
 * dz is the gradient with respect to x AND to res: one tensor, written once.
 *
 *   tf_add_layernorm_train_f32   tf_add_layernorm_f32 that also saves stats[r] = (mean, rstd) [rows, 2], exactly the two fp32 values row r
 *                                was normalised with.  The kernel and its arithmetic are those of tf_add_layernorm_f32: `out` is
 *                                bit-identical to it on the same operands.  Nothing else is saved: the backward reads x and res again.
 *   tf_add_layernorm_bwd_f32     one pass over the rows, one wave per row: z is formed again by the forward's single fp32 addition, xh
 *                                from the saved statistics; mean_c by a butterfly over the wave; dz written once.  In the same pass
 *                                every lane sums dy and dy xh of its own columns over the rows its wave walks.  The rows are cut into
 *                                blocks by a rule of `rows` alone (16 rows per block up to 32 768 rows, ceil(rows / 2048) beyond: at most
 *                                2048 blocks; never the grid, the CU count or the occupancy -- as the row blocks of
 *                                tf_linear_grad_stats_f32); a block's four waves are added in wave order (rows w, w + 4, ... of the
 *                                block in wave w, ascending) and the block writes one partial row [2, C] to `workspace`.  A second,
 *                                small launch adds the partials: slice s = 0 .. 15 takes blocks s, s + 16, ... in that order, then the
 *                                slices in the order 0, 1, ...  dz / dgamma / dbeta may each be NULL: without dgamma and dbeta the
 *                                column sums are compiled out of the first launch, the second is skipped and workspace may be NULL.
 *                                workspace: tf_add_layernorm_bwd_workspace_bytes(rows, C) = blocks . 2 C . 4 bytes.
 * C % 4 == 0, C <= 4096, rows < 2^31; dy / x / res / gamma / dz / dgamma / dbeta / workspace 16-byte aligned, stats 8-byte aligned.  dz must
 * not overlap an input.
 * No atomics anywhere and every sum in a fixed order: each result is a pure function of the arguments -- bit-identical from call to
 * call, on any stream and in a captured HIP graph.
 * Non-finite operands: rows are independent in dz -- a NaN or an inf in row r of dy, x or res makes the elements of row r non-finite
 * where the exact value is, and changes no bit of any other row; dgamma[c] and dbeta[c] are non-finite exactly when their exact sum is
 * (a NaN in x[r, :] reaches every xh[r, c] through the row's mean, hence every dgamma[c]; a NaN in dy[r, c] reaches column c alone).
 * Checked in this order, before any GPU work: NULL dy / x / gamma / stats (train: x / gamma / beta / out / stats) ->
 * TF_MSDA_ERR_NULL_POINTER, dimensions / alignment -> TF_MSDA_ERR_BAD_DIMS, with dgamma or dbeta a workspace that is NULL, too small
 * or misaligned -> TF_MSDA_ERR_WORKSPACE.  tf_add_layernorm_bwd_workspace_bytes returns -1 for dimensions the entry point rejects.
 */
int tf_add_layernorm_train_f32(const float *x, const float *res, const float *gamma, const float *beta, float *out, float *stats,
                               int64_t rows, int C, float eps, void *stream);
int64_t tf_add_layernorm_bwd_workspace_bytes(int64_t rows, int C);
int tf_add_layernorm_bwd_f32(const float *dy, const float *x, const float *res, const float *gamma, const float *stats, float *dz,
                             float *dgamma, float *dbeta, void *workspace, int64_t workspace_bytes, int64_t rows, int C, void *stream);

/*
 * DROPOUT INSIDE THE TRAINING KERNELS  (trackformer_amd/csrc/dropout_rng.h, dropout_train.h; reference: the nn.Dropout(0.1) in front of
 * every residual add and behind the feed-forward block's ReLU of models/deformable_transformer.py).  The keep decision of an element is
 * computed where it is needed, forward and backward, from a counter: no mask and no dropped tensor are stored.
 *
 * THE GENERATOR CONTRACT.  Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85).
 *     key     = (seed low 32 bits, seed high 32 bits)
 *     counter = (g low, g high, offset low, offset high),   g = i / 4 for element i of the FLAT tensor
 *     output word j = 0 .. 3 decides element 4 g + j:   kept iff word >= T,   T = floor(p 2^32) computed once by the entry point, in
 *     double, from the float p;   survivors are multiplied by the float scale = 1.0f / (1.0f - p), dropped elements are exactly 0
 *     (a select, not a product: also where the operand is inf or NaN).
 * (seed, offset) = rng[0], rng[1]: an int64[2] tensor ON THE DEVICE that the kernels read -- no host synchronisation, safe inside a
 * captured graph (the graph replays whatever the tensor holds then).  The decision is an integer comparison and a function of (seed,
 * offset, p, i) alone: independent of the launch geometry and of the dtype of the data.  Every entry refuses p <= 0, p >= 1 and a
 * non-finite p with TF_MSDA_ERR_BAD_DIMS.
 *
 *   tf_dropout_keep_u8                   keep[k] = 1 / 0 for element first + k, k = 0 .. n - 1 (first and n multiples of 4; keep 4-byte
 *                                        aligned): the mask itself, for tests and for anyone who wants to look at one.
 *   tf_add_dropout_layernorm_train_f32   out = LayerNorm(x + keep scale res) gamma + beta, stats[r] = (mean, rstd).  d = keep scale res is
 *                                        one fp32 product, z = x + d one fp32 addition (never contracted into an fma).  One wave per row,
 *                                        lane j the float4 chunks j, j + 64, ..., as tf_add_layernorm_f32.  res is required (x itself
 *                                        is allowed).
 *   tf_add_dropout_layernorm_bwd_f32     rebuilds z from x, res and the recomputed mask (the forward's bits), then dz as
 *                                        tf_add_layernorm_bwd_f32.  dx = dz, dres = keep scale dz (exactly 0 where dropped); dx / dres /
 *                                        dgamma / dbeta may each be NULL.  The column sums follow tf_add_layernorm_bwd_f32 to the letter:
 *                                        its row blocks (a rule of `rows` alone), its wave order inside a block, its workspace
 *                                        (tf_add_layernorm_bwd_workspace_bytes) and its second launch.  No atomics, LDS included.
 *   tf_dropout_inplace_f32               y <- keep scale y over n elements (n % 4 == 0), element i of y is element i of the stream.
 *   tf_relu_dropout_bwd_f32              out = y > 0 ? dy scale : 0, for y = dropout(relu(h)): scale >= 1 keeps a kept positive
 *                                        activation positive, so y alone encodes both decisions and the backward needs neither the
 *                                        generator nor the ReLU output.  y = +-0 and a NaN y give 0.
 * Gates as tf_add_layernorm_bwd_f32: C % 4 == 0, C <= 4096, rows < 2^31, 16-byte aligned tensors, stats and rng 8-byte aligned; outputs
 * must not overlap inputs (tf_dropout_inplace_f32 excepted).  Checked in this order before any GPU work: NULL -> TF_MSDA_ERR_NULL_POINTER,
 * p / dimensions / alignment -> TF_MSDA_ERR_BAD_DIMS, workspace -> TF_MSDA_ERR_WORKSPACE.  Every result is a pure function of the
 * arguments and of what rng holds: bit-identical from call to call, on any stream and in a captured HIP graph.
 */
int tf_dropout_keep_u8(const int64_t *rng, float p, int64_t first, int64_t n, uint8_t *keep, void *stream);
int tf_add_dropout_layernorm_train_f32(const float *x, const float *res, const float *gamma, const float *beta, const int64_t *rng,
                                       float p, float *out, float *stats, int64_t rows, int C, float eps, void *stream);
int tf_add_dropout_layernorm_bwd_f32(const float *dy, const float *x, const float *res, const float *gamma, const float *stats,
                                     const int64_t *rng, float p, float *dx, float *dres, float *dgamma, float *dbeta, void *workspace,
                                     int64_t workspace_bytes, int64_t rows, int C, void *stream);
int tf_dropout_inplace_f32(float *y, const int64_t *rng, float p, int64_t n, void *stream);
int tf_relu_dropout_bwd_f32(const float *dy, const float *y, float p, float *out, int64_t n, void *stream);

/*
 * THE SET CRITERION AND THE MATCHING COST  (trackformer_amd/csrc/criterion.h; reference: loss_labels_focal / loss_cardinality /
 * loss_boxes of models/detr.py and the focal branch of models/matcher.py, fp32).  The decoder layers' predictions are stacked:
 * logits [L, B, Q, C], boxes [L, B, Q, 4] (cxcywh), contiguous.  tgt_of int32 [L, B, Q] holds the GLOBAL index (into labels / tboxes, the
 * images' targets concatenated) of the target matched to that prediction, or -1; a value outside [0, T) counts as -1 and no target is
 * read for it.  labels int64 [T], tboxes [T, 4], tgt_len int32 [B] (targets per image).
 *
 *   tf_set_criterion_fwd_f32   one launch, one 256-thread workgroup per layer:
 *                                losses[l] = (loss_ce, loss_bbox, loss_giou)   card[l] = mean_b |#{q: argmax_c != C - 1} - tgt_len[b]|
 *                                class_error[0] = 100 - 100 #{matched rows of layer 0 whose argmax is their label} / #{matched rows},
 *                                100 when nothing is matched.
 *                              loss_ce = sum_{b,q,c} focal(x, y) / num_boxes with y = 1 exactly where c == labels[tgt_of] (a label C is the
 *                              no-object class: no positive element).  The focal term is evaluated in its STABLE form: with z = x for
 *                              y = 0 and z = -x for y = 1,
 *                                  focal = a_t softplus(z) exp(-gamma softplus(-z)),   softplus(+-z) = max(+-z, 0) + log1p(exp(-|z|)),
 *                              a_t = alpha for y = 1, 1 - alpha for y = 0, 1 for alpha < 0.  No 1 - sigmoid(x) is formed in fp32: the
 *                              reference's formulation loses the small elements and their gradients beyond |x| ~ 8.
 *                              loss_bbox = sum |box - tbox| / num_boxes and loss_giou = sum (1 - GIoU) / num_boxes over the matched
 *                              rows, operation by operation as l1_loss and box_ops.generalized_box_iou_pairs, compiled without FMA
 *                              contraction; no guards: a zero-area pair gives NaN as in torch.  The arg-max takes the lowest index on
 *                              ties and a NaN as the largest value; for C == 1 the cardinality prediction is 0, as the reference's.
 *                              SUMS: accumulated in fp64, rounded to fp32 once.  Thread t of the layer's workgroup takes queries t,
 *                              t + 256, ... of image 0, then of image 1, ...; a butterfly over the wave; the four waves in wave order
 *                              through LDS: the order is a function of the shape alone.  No atomics; every output is written once.
 *                              T == 0 and images without targets are valid (box losses 0); labels / tboxes may then be NULL.
 *   tf_set_criterion_bwd_f32   one launch, one work-item per (l, b, q).  G [L, 3]: the gradients of the three losses.  Recomputes from
 *                              the forward's inputs (nothing else is saved) and writes grad_logits [L, B, Q, C] and grad_boxes
 *                              [L, B, Q, 4] (zeros in unmatched rows), every element once; no atomics, no workspace.  Either output
 *                              may be NULL and is then skipped.  min / max hand half of the gradient to each operand at a tie and
 *                              clamp passes it at 0, as torch.
 *   tf_match_cost_f32          one launch, one work-item per (r, t): cost [R, T] =
 *                                  w_bbox |boxes[r] - tgt_bbox[t]|_1 + w_class (pos - neg) + w_giou (-GIoU),
 *                                  pos = alpha (1 - p)^gamma (-log(p + 1e-8)),  neg = (1 - alpha) p^gamma (-log(1 - p + 1e-8)),
 *                              p = sigmoid(logits[r, tgt_ids[t]]), with 1 - p formed as sigmoid(-x), never as a subtraction.  The GIoU
 *                              is the device function of the criterion.  R == 0 or T == 0: nothing to do.
 * boxes / tboxes / tgt_bbox / grad_boxes 16-byte aligned, labels / tgt_ids 8-byte, everything else 4-byte; L B Q max(C, 4) < 2^31,
 * R max(C, 4, T) < 2^31; num_boxes > 0.  Each result is a pure function of the arguments: bit-identical from call to call, on any stream
 * and in a captured HIP graph.  Non-finite logits: a NaN logit makes its layer's loss_ce and its own gradient NaN and leaves every other
 * layer and element as it was.
 * Checked in this order, before any GPU work: NULL required pointers -> TF_MSDA_ERR_NULL_POINTER, dimensions / alignment ->
 * TF_MSDA_ERR_BAD_DIMS.  The labels live on the device: a label outside [0, C] is found on the host side of the binding
 * (fused.set_criterion, fused.match_cost: TF_MSDA_ERR_BAD_DIMS), not by a device assert; the kernels never read outside a row for one.
 */
int tf_set_criterion_fwd_f32(const float *logits, const float *boxes, const int *tgt_of, const int64_t *labels, const float *tboxes,
                             const int *tgt_len, float *losses, float *card, float *class_error, int L, int B, int Q, int C, int T,
                             float alpha, float gamma, float num_boxes, void *stream);
int tf_set_criterion_bwd_f32(const float *G, const float *logits, const float *boxes, const int *tgt_of, const int64_t *labels,
                             const float *tboxes, float *grad_logits, float *grad_boxes, int L, int B, int Q, int C, int T, float alpha,
                             float gamma, float num_boxes, void *stream);
int tf_match_cost_f32(const float *logits, const float *boxes, const int64_t *tgt_ids, const float *tgt_bbox, float *cost, int64_t R, int C,
                      int T, float w_class, float w_bbox, float w_giou, float alpha, float gamma, void *stream);

/*
 * THE MASK LOSSES  (trackformer_amd/csrc/mask_loss.h; reference: SetCriterion.loss_masks of models/detr.py with sigmoid_focal_loss and
 * dice_loss of util/misc.py, fp32).  src [BQ, h, w] fp32 is the contiguous pred_masks, tgt uint8 [T, H, W] the padded stack of the images'
 * target masks (bool viewed as bytes; any non-zero byte is 1) -- never converted to float and never gathered: pair i = (row pair_src[i] of
 * src, row pair_tgt[i] of tgt), i < n.  Every matched row of src is upsampled to H x W as F.interpolate(mode="bilinear",
 * align_corners=False) does, with the coordinates in integer arithmetic: output row Y reads rows y0 = num / (2 H) and
 * y1 = y0 + (y0 < h - 1) with weights 1 - l and l, num = max((2 Y + 1) h - H, 0), l = (num % (2 H)) / (2 H) rounded once; the same in x.
 * No full-resolution fp32 tensor is written in either direction.
 *
 *   tf_mask_loss_fwd_f32   two launches.  (1) one 256-thread workgroup per (pair, tile of 8 output rows): x interpolated on the fly,
 *                          the focal term in the STABLE form of the set criterion (alpha < 0: no alpha weight), p = sigmoid(x) from the
 *                          same exp; the tile's four sums (focal, p t, p, t) in fp64 -> workspace [n, tiles, 4], tiles = ceil(H / 8).
 *                          (2) one workgroup adds the tiles in index order -> sums fp64 [n, 4] (kept for the backward) and
 *                              losses[0] = loss_mask = sum_i (focal_i / (H W)) / num_boxes
 *                              losses[1] = loss_dice = sum_i (1 - (2 spt_i + 1) / (sp_i + st_i + 1)) / num_boxes
 *                          the pairs in index order, each loss rounded to fp32 once.  n == 0: both losses are 0, nothing else is read
 *                          or written (src / tgt / pair_* / sums / workspace may be NULL).
 *   tf_mask_loss_bwd_f32   one launch, one work-item per element of grad_src [BQ, h, w]: every element written exactly once, zeros in
 *                          the rows of unmatched queries.  row_pair int32 [BQ]: the pair of that row or -1.  G [2]: the gradients of the
 *                          two losses.  Gather form: a source pixel adds wy wx g_x over the contiguous range of output rows and columns
 *                          that have it as a corner (the bounds from the same integer formula; at the bottom / right edge, where
 *                          y1 == y0, both weights go to the one pixel), in fp64, in a fixed order, rounded once.
 *                              g_x = G[0] / (num_boxes H W) dfocal/dx + G[1] / num_boxes (-(2 t den - num) / den^2) p (1 - p)
 *                          num = 2 spt + 1 and den = sp + st + 1 from `sums`; p (1 - p) = sigmoid(|x|) sigmoid(-|x|); g_x is recomputed
 *                          for each of the four corners (csrc/mask_loss.h says why).  n == 0: all zeros.
 * An index outside its range (pair_src outside [0, BQ), pair_tgt outside [0, T), row_pair outside [0, n)) makes its pair / row count as
 * unmatched: zeros, and nothing is read for it.  Sizes: h, w >= 1, H >= h, W >= w, H and W <= 2^23, (2 H + 1)(h + 1) < 2^31 and the same
 * in x, H W < 2^31, n tiles < 2^31, BQ ceil(h w / 256) < 2^31; num_boxes > 0.  sums / workspace 8-byte aligned, everything else 4-byte
 * (tgt: none).  No atomics anywhere and every sum in an order that is a function of the shape alone: each result is a pure function of
 * the arguments -- bit-identical from call to call, on any stream and in a captured HIP graph.
 * Checked in this order, before any GPU work: NULL required pointers -> TF_MSDA_ERR_NULL_POINTER, dimensions / alignment ->
 * TF_MSDA_ERR_BAD_DIMS, (n > 0) a workspace that is NULL, misaligned or smaller than tf_mask_loss_workspace_bytes(n, H, W) ->
 * TF_MSDA_ERR_WORKSPACE.  tf_mask_loss_workspace_bytes returns -1 for n < 0, H or W <= 0 or n tiles >= 2^31.
 */
int64_t tf_mask_loss_workspace_bytes(int n, int H, int W);
int tf_mask_loss_fwd_f32(const float *src, const uint8_t *tgt, const int *pair_src, const int *pair_tgt, double *sums, float *losses,
                         void *workspace, int64_t workspace_bytes, int n, int BQ, int T, int h, int w, int H, int W, float alpha,
                         float gamma, float num_boxes, void *stream);
int tf_mask_loss_bwd_f32(const float *G, const float *src, const uint8_t *tgt, const int *pair_tgt, const int *row_pair, const double *sums,
                         float *grad_src, int n, int BQ, int T, int h, int w, int H, int W, float alpha, float gamma, float num_boxes,
                         void *stream);

/*
 * Convolution of a channels_last activation through the same kernel (an implicit GEMM over the output pixels; the weight
 * fragments streamed from L2, only the shifted input pixels pass LDS): ks = 3 (padding 1) or 1 (no padding), stride 1 or 2.
 *   x [nimg, hin, win, cin] NHWC fp32, below 3 GiB;  y [nimg, hout, wout, cout] NHWC, below 3 GiB;  cin % 64 == 0
 *   w_packed   tf_linear_pack_weight_f32(K = ks * ks * cin, N = cout, terms) of the [cout, ks, ks, cin] weight (the storage of a
 *              channels_last OIHW tensor: K is tap-major) -- a following FrozenBatchNorm2d's scale folded in by the caller
 *   bias [cout] / residual [nimg, hout, wout, cout]: may be NULL
 *   ksplit     1..64 pieces of the K loop run as separate workgroups (few output pixels under a long K: layer3 / layer4, the
 *              extra pyramid level of deformable_detr.py:55-79); the pieces write partial sums to `workspace` (ksplit * M * cout
 *              floats), a second launch adds them in a fixed order (deterministic) and applies bias / residual / ReLU.
 *              ksplit > 1: cout % 4 == 0, 16-byte aligned y / bias / residual / workspace.
 * Same products in the same order as tf_conv3x3_split_f32 / tf_conv1x1_strided_split_f32: bit-identical for ksplit == 1.
 * (reference: torchvision Bottleneck.conv1 / conv2 / downsample under models/backbone.py:93-104)
 */
int tf_conv_packed_f32(const float *x, const void *w_packed, const float *bias, const float *residual, float *y, float *workspace,
                       int ksplit, int nimg, int hin, int win, int cin, int cout, int ks, int stride, int relu, int terms,
                       void *stream);
/*
 * The same convolution with its split-K second pass DEFERRED to the consumer (tf_groupnorm_levels_nhwc_f32 adds the pieces in its
 * own fetch): only the GEMM launch runs.  *pieces = the number of partial sums [pieces][M * cout] it left in `workspace` (what the
 * launch code made of `ksplit` for this shape), in the order the second pass would add them, WITHOUT the bias; *pieces == 1: the
 * launch was not split and workspace holds the finished y, bias added.  No residual, no ReLU.  workspace: max(ksplit, 1) * M * cout
 * floats, always required; otherwise the arguments and checks of tf_conv_packed_f32 with ksplit > 1.
 */
int tf_conv_packed_partials_f32(const float *x, const void *w_packed, const float *bias, float *workspace, int ksplit, int nimg, int hin,
                                int win, int cin, int cout, int ks, int stride, int terms, int *pieces, void *stream);

/*
 * The feed-forward block of a transformer layer in one launch (trackformer_amd/csrc/ffn_fused.hip):
 *
 *     y[M, d_model] = [LayerNorm]( residual + relu(x . w1^T + b1) . w2^T + b2 )
 *
 * (reference: models/deformable_transformer.py:282-297 forward_ffn + norm2 of the encoder layer, :371-379 of the decoder
 * layer; inference: the dropouts are identities).  The d_ffn-wide intermediate stays on the CU.  Same split
 * product as tf_linear_packed_f32 (same `terms`) for both GEMMs: without the LayerNorm the result is bit-identical to
 * tf_linear_packed_f32(relu) -> tf_linear_packed_f32 -> + residual.
 *   w1_packed, w2_packed   tf_linear_pack_weight_f32 of linear1.weight [d_ffn, d_model] (K = d_model, N = d_ffn) and of
 *                          linear2.weight [d_model, d_ffn] (K = d_ffn, N = d_model)
 *   b1 [d_ffn], b2 [d_model], residual [M, d_model]: each may be NULL;  ln_weight / ln_bias [d_model]: both or neither
 *   (neither: no LayerNorm);  y must not alias x or residual.
 * d_model == 256 or 288 (the reference's hidden sizes), d_ffn a multiple of 16 and >= 128, every pointer 16-byte aligned;
 * anything else: TF_MSDA_ERR_BAD_DIMS.
 */
/*
 * y[M, D] = [LayerNorm]( residual + x[M, D] . w^T + bias ), D = 256 or 288, in one launch: the attention's output projection with the
 * layer's residual add and norm1 (reference: models/ops/modules/ms_deform_attn.py:87 output_proj +
 * models/deformable_transformer.py:285-292).  Same split product as tf_linear_packed_f32 (bit-identical without the
 * LayerNorm); w_packed: tf_linear_pack_weight_f32 of the [D, D] weight.  K == N == D, pointers 16-byte aligned,
 * bias / residual may be NULL, ln_weight / ln_bias both or neither, y must not alias x or residual.
 */
int tf_linear_res_ln_f32(const float *x, const void *w_packed, const float *bias, const float *residual, const float *ln_weight,
                         const float *ln_bias, float ln_eps, float *y, int64_t M, int K, int N, int terms, void *stream);

int tf_ffn_fused_f32(const float *x, const void *w1_packed, const float *b1, const void *w2_packed, const float *b2,
                     const float *residual, const float *ln_weight, const float *ln_bias, float ln_eps, float *y, int64_t M,
                     int d_model, int d_ffn, int terms, void *stream);

/*
 * Several projections of the same rows in one launch (trackformer_amd/csrc/ffn_fused.hip): for each of `ngroups` (1..8) groups
 *
 *     y_g[M, N_g] = (add_x2 ? x + x2 : x)[M, K] . w_g^T + bias_g
 *
 * -- the value projection and the query projection of `with_pos_embed(src, pos)` of an encoder layer (reference:
 * models/ops/modules/ms_deform_attn.py:64-72 under models/deformable_transformer.py:279-283), or the value projections of all
 * decoder layers' cross-attention over the one encoder memory.  A workgroup stages its rows of x once (and once more as x + x2, the
 * fp32 sum rounded before it is split) and walks every group's weight; the groups without add_x2 run first.  Same split product
 * as tf_linear_split_f32 / tf_linear_split_add_f32 with the same `terms`: every y_g is bit-identical to theirs.
 *   w_packed   tf_linear_pack_weight_f32(K, N_g, terms) of that group's weight alone (with its own channel scales)
 *   bias       [N_g] or NULL;  y: its own contiguous [M, N_g] buffer, distinct from x, x2 and every other y
 *   x2         [M, K], required if any group has add_x2
 * K == 256 (else TF_MSDA_ERR_BAD_DIMS: the caller keeps the separate launches), N_g % 32 == 0, (M + 128) N_g 4 < 2^32, every pointer
 * 16-byte aligned.  The descriptors are read during the call (they travel in the kernel's arguments): `groups` may be a temporary.
 * NULL pointer -> TF_MSDA_ERR_NULL_POINTER, then dimensions / alignment -> TF_MSDA_ERR_BAD_DIMS, before any GPU work.
 */
typedef struct tf_proj_group {
    const void *w_packed;
    const float *bias;
    float *y;
    int N;
    int add_x2;
} tf_proj_group;
int tf_linear_groups_f32(const float *x, const float *x2, const tf_proj_group *groups, int ngroups, int64_t M, int K, int terms,
                         void *stream);

/*
 * out[n, l, h, :] = sum_j softmax_j(scale * q[n, l, h, :] . k[n, j, h, :]) v[n, j, h, :]      (fp32)
 * Element (n, l, h, c) of q / k / v / out lives at base + (n * L + l) * ld + h * D + c with ld in floats (so q and
 * k may be the two halves of one projection output).  key_mask: [N, Lk] bytes, non-zero = the key is ignored
 * (nn.MultiheadAttention's key_padding_mask), or NULL.  D in {16, 32, 36, 64}, ld % 4 == 0, 16-byte aligned
 * pointers, Lk up to ~2400 (the 16 x Lk score tile lives in LDS).
 */
int tf_mha_core_f32(const float *q, const float *k, const float *v, float *out, const unsigned char *key_mask,
                    int N, int Lq, int Lk, int H, int D, int ldq, int ldk, int ldv, int ldo, float scale,
                    void *stream);

/*
 * TRAINING THROUGH THE ATTENTION CORE  (trackformer_amd/csrc/mha_bwd.h and the TRAIN instantiation of the default kernel of
 * tf_mha_core_f32; reference: the autograd of nn.MultiheadAttention's softmax(q k^T scale) -> dropout -> . v, fp32).  Layouts, key_mask
 * and scale as tf_mha_core_f32.  With s_ij = q_i . k_j, c = scale log2(e) (the float product scale * 1.44269504088896340736f) and the
 * keys j the mask leaves:
 *     stats[n, h, i, 0] = m_i   = max_j fl(c s_ij)                 (the row maximum in units of log2; 0 for a row without keys)
 *     stats[n, h, i, 1] = inv_i = 1 / sum_j 2^(fl(c s_ij) - m_i)   (the reciprocal row sum; 0 for a row without keys)
 *     P_ij = 2^(c s_ij - m_i) inv_i  (0 for a masked key),   Pd_ij = keep_ij s_p P_ij,   out_i = sum_j Pd_ij v_j
 * stats is [N, H, Lq, 2] fp32, contiguous.  Nothing of size Lq x Lk is stored: the backward rebuilds P from q, k and stats.
 *
 * THE MASK CONTRACT.  THE GENERATOR CONTRACT (above) applied to the weights as a tensor [N, H, Lq, Lk4] with rows PADDED to
 * Lk4 = 4 ceil(Lk / 4) keys: the decision for weight (n, h, i, j) is that of flat element r Lk4 + j of the stream `rng`,
 * r = (n H + h) Lq + i.  A Philox group is therefore always four consecutive keys of one row, whatever Lk is (track queries make it
 * arbitrary).  tf_dropout_keep_u8 over N H Lq Lk4 elements, viewed as [N, H, Lq, Lk4] and sliced to [..., :Lk], IS the mask.  Masked
 * keys consume their positions: the decision does not depend on key_mask.  s_p = 1.0f / (1.0f - p) as a float; a dropped weight is
 * exactly 0 (a select).  rng == NULL: no dropout (keep = 1, s_p = 1; p is not read).
 *
 *   tf_mha_core_train_f32   one launch: the default kernel of tf_mha_core_f32 (option mha_mfma = 1, whatever the option holds), which
 *                           also writes stats and, with rng, drops the weights where P V reads them.  With rng == NULL `out` is
 *                           bit-identical to tf_mha_core_f32 under mha_mfma = 1.  A row whose keys are all masked gives exactly 0.
 *   tf_mha_core_bwd_f32     one launch, no workspace:   dP = dout V^T,   delta_i = sum_c dout_ic out_ic (= sum_j Pd_ij dP_ij),
 *                               dS = P (keep s_p dP - delta),   dq = scale dS K,   dk = scale dS^T Q,   dv = Pd^T dout.
 *                           Workgroups that own 16 queries walk the keys and write dq; workgroups that own 16 keys walk the queries and
 *                           write dk and dv; each recomputes delta.  All products are exact-fp32 matrix instructions.  dq / dk / dv
 *                           have leading dimensions of their own: dq and dk may be the halves of ONE [N, L, 2 E] gradient of a shared
 *                           q | k projection.  No atomics, LDS included; every element is written once and every sum runs in an order
 *                           that is a function of (Lq, Lk) alone: bit-identical from call to call, on any stream, in a captured HIP
 *                           graph and next to concurrent work.
 * Dead elements are selected, not multiplied: masked keys get dk = dv = +0, rows whose keys are all masked get dq = +0 and their dout
 * (NaN included) reaches no output.
 * D in {32, 36}; Lq and Lk in 1 .. 1024, independent; every ld % 4 == 0 and >= H D; tensors 16-byte aligned, stats and rng 8-byte
 * aligned; outputs must not overlap inputs.  Checked in this order before any GPU work: NULL q / k / v / out / stats (bwd: also dout /
 * dq / dk / dv) -> TF_MSDA_ERR_NULL_POINTER; with rng a p outside (0, 1), dimensions, alignment -> TF_MSDA_ERR_BAD_DIMS.
 */
int tf_mha_core_train_f32(const float *q, const float *k, const float *v, float *out, const unsigned char *key_mask, float *stats,
                          const int64_t *rng, float p, int N, int Lq, int Lk, int H, int D, int ldq, int ldk, int ldv, int ldo,
                          float scale, void *stream);
int tf_mha_core_bwd_f32(const float *dout, const float *q, const float *k, const float *v, const float *out, const float *stats,
                        const unsigned char *key_mask, const int64_t *rng, float p, float *dq, float *dk, float *dv, int N, int Lq,
                        int Lk, int H, int D, int lddo, int ldq, int ldk, int ldv, int ldo, int lddq, int lddk, int lddv, float scale,
                        void *stream);

/*
 * Greedy non-maximum suppression on HOST boxes (all pointers host; synchronous): torchvision.ops.nms semantics, which the
 * reference's tracker calls twice per frame (tracker.py:399,495).  boxes [n, 4] xyxy, scores [n]; boxes are visited in
 * stable descending-score order; keep [n] receives the indices of the kept boxes in that order, *n_keep their number.
 * IoU arithmetic: fp32, inter / (area_i + area_j - inter), as box_ops.box_iou.
 */
int tf_nms_host_f32(const float *boxes, const float *scores, int n, float iou_threshold, int64_t *keep, int *n_keep);

#ifdef __cplusplus
}
#endif
#endif /* TF_FUSED_H_ */
