/*
 * include/tf_msda.h -- C ABI of libtf_msda.so, the MI355X (gfx950) implementation of TrackFormer's
 * multi-scale deformable attention operator.
 *
 * This is the drop-in boundary for the reference's native extension `MultiScaleDeformableAttention`:
 *
 *   reference interface (paths under /root/reference/src/trackformer/models/ops/)      replaced by
 *   ---------------------------------------------------------------------------------  -----------------------
 *   ms_deform_attn_forward(value, spatial_shapes, sampling_loc, attn_weight, step)      tf_msda_forward_{f32,f64}
 *     src/vision.cpp:5, src/ms_deform_attn.h:10-28, src/cuda/ms_deform_attn_cuda.cu:19-86
 *   ms_deform_attn_backward(value, spatial_shapes, sampling_loc, attn_weight,           tf_msda_backward_{f32,f64}
 *                           grad_output, step)
 *     src/vision.cpp:6, src/ms_deform_attn.h:30-49, src/cuda/ms_deform_attn_cuda.cu:89-168
 *
 * The binding that exposes these under the reference's Python names
 * (`MultiScaleDeformableAttention.ms_deform_attn_forward/backward`) lives in
 * trackformer_amd/dropin/MultiScaleDeformableAttention.py; see INTEGRATION.md.
 *
 * Conventions
 *   - Plain pointers and sizes only; no torch / ATen types.  All data pointers are DEVICE pointers
 *     on the current HIP device unless marked "host".  The caller owns every buffer.
 *   - Tensors are dense row-major:
 *       value        [N, S, M, D]          S = sum_l H_l*W_l; level l occupies rows start_l .. start_l+H_l*W_l
 *       shapes       [L, 2] int64 (H_l, W_l)
 *       loc          [N, Lq, M, L, P, 2]   (x, y) normalised to [0,1] over the level; pixel = loc*size - 0.5,
 *                                          zero padding outside, in range iff -1 < pixel < size
 *       attn         [N, Lq, M, L, P]
 *       out/grad_out [N, Lq, M*D]
 *   - Work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the default stream) and the
 *     call returns without synchronising.  HIP-graph capturable.  Re-entrant: a call's RESULT depends on its arguments
 *     only.  What IS process-wide: (a) the kernel-selection knobs below (tf_msda_set_tiled / tf_msda_set_option and the
 *     environment variables they mirror) -- performance only, results identical up to fp32 summation order; they exist
 *     for A/B measurements, a deployment leaves them alone; (b) the per-thread last-HIP-error slot; (c) per-(function,
 *     device) one-time attribute calls (the dynamic-LDS limit of a kernel that may ask for more than 64 KB), and the
 *     compute-unit count of the first device a call ran on, which the block-shape rules use for every device.
 *   - Return value: TF_MSDA_OK (0) or a negative tf_msda_status.  Never throws.
 *   - im2col_step of the reference API only chunks the batch (cu:44-66) and does not change results;
 *     this ABI has no such parameter.
 */
#ifndef TF_MSDA_H_
#define TF_MSDA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TF_MSDA_ABI_VERSION 12
#define TF_MSDA_MAX_LEVELS 16

typedef enum tf_msda_status {
    TF_MSDA_OK = 0,
    TF_MSDA_ERR_NULL_POINTER = -1,  /* a required pointer was NULL */
    TF_MSDA_ERR_BAD_DIMS = -2,      /* a dimension <= 0, L > TF_MSDA_MAX_LEVELS, or sizes overflow */
    TF_MSDA_ERR_SHAPE_SUM = -3,     /* sum_l H_l*W_l != S (host-shape entry points only) */
    TF_MSDA_ERR_LAUNCH = -4,        /* HIP reported an error enqueueing work (see tf_msda_last_hip_error) */
    TF_MSDA_ERR_NO_DEVICE = -5,     /* no HIP device available */
    TF_MSDA_ERR_WORKSPACE = -6      /* caller's workspace smaller than the entry point's *_workspace_bytes, or misaligned */
} tf_msda_status;

/* ABI version of the loaded library (== TF_MSDA_ABI_VERSION it was built with). */
int tf_msda_abi_version(void);

/* Human-readable text for a tf_msda_status. Never NULL. */
const char *tf_msda_strerror(int status);

/* hipError_t (as int) of the most recent failing HIP call on this thread, 0 if none.  Covers every entry point of this header
 * and of tf_fused.h: whichever returned TF_MSDA_ERR_LAUNCH last on this thread stored its code here. */
int tf_msda_last_hip_error(void);

/*
 * Name of the device kernel the most recent forward / backward call of THIS thread enqueued (e.g.
 * "msda_fwd_f32_pquad2<fused,4w,2p>"), "" before the first call.  The string is static.  Measurement aid: bench.py labels
 * its roofline with what the library dispatched instead of inferring it from the options.
 */
const char *tf_msda_last_kernel(void);

/*
 * Kernel selection knob (process-wide, performance only -- results are identical up to fp32 summation
 * order) for encoder-shaped forward calls (Lq == S, fp32, D == 32 or 36, P == 4, L <= 4, host shapes):
 * 2 = the LDS-window kernels (msda_fwd_f32_pquad: persistent workgroups, 4 lanes per pair; msda_fwd_f32_quad where it
 * declines; the default), 0 = msda_fwd_f32_direct (row gathers by buffer loads, what every other shape uses),
 * -1 restores the default (environment variable TF_MSDA_TILED, 2 when unset).  Returns the previous setting.
 */
int tf_msda_set_tiled(int mode);

/*
 * Generic form of the knob above (process-wide, performance only).  Sets option `name` to `value` and
 * returns the previous value, or INT_MIN for an unknown name.  Names:
 *   "tiled"         0 / 2 / -1 as tf_msda_set_tiled
 *   "pquad"         1 / 0: the persistent encoder kernel on / off (off: msda_fwd_f32_quad)
 *   "pquad_npass" "pquad_lds_kb" "pquad_wg_per_cu" "pquad_wide" "pquad_prefetch" "pquad_skew" "pquad_halo_y"
 *   "pquad_halo_x" "pquad_tile_h" "pquad_tile_w"    its tile plan (TF_MSDA_PQUAD="npass=2,lds=52,wgs=3,...")
 *   "quad_ta_mask"  bit l set: level l is gathered by buffer loads instead of an LDS window (0, 8 or 12)
 *   "quad_waves"    wavefronts per workgroup (4 or 8);  "quad_npass"  passes of 16 pairs per wave (1..3)
 *   "quad_lds_kb"   LDS per workgroup (decides the workgroups per CU and the window capacity)
 *   "quad_halo_y" / "quad_halo_x"   clamp of the data-adaptive windows around the tile footprint
 *   "quad_tile_h" / "quad_tile_w"   tile size in level-0 pixels (0 = search);  "quad_split"  staging rounds
 *   "direct9"       1 / 0: msda_fwd_f32_direct9 for D == 36 decoder calls (off: msda_fwd_f32_buf)
 * The knobs of the dense kernels (include/tf_fused.h) share one table: the value in force is the environment variable's
 * at the first use (or the default), a value outside the range becomes the one in brackets -- from the variable and from
 * this call alike --, a flag takes 0 / non-zero (from the variable: off only when it starts with '0'), and the call
 * returns the value that was in force.
 *   "ffn_ti"            TF_FFN_TI            1..3 [3], default 3   row tiles per block of tf_ffn_fused_f32
 *   "ffn_tail_split"    TF_FFN_TAIL_SPLIT    flag, default 1       its rows behind the full rounds of 64-row blocks as 32-row blocks
 *   "linln_ti"          TF_LINLN_TI          0..3 [0], default 0   row tiles per block of tf_linear_res_ln_f32 (0 = by row count)
 *   "groups_ti"         -                    1..3 [0], default 0   row tiles per block of tf_linear_groups_f32 with fp16 pieces (0 = by row count)
 *   "linear_stream_ti"  TF_LINEAR_STREAM_TI  1..4 [0], default 0   row tiles per block of tf_linear_packed_f32 / tf_conv_packed_f32 (0 = per shape)
 *   "conv_halo"         TF_CONV_HALO         flag, default 1       the halo form of the stride-1 3 x 3 convolutions (0: the stream form)
 *   "linear_dma"        TF_LINEAR_DMA        0..9 [0], default 0   the LDS-DMA GEMM behind tf_linear_packed_f32: 1..4 = a block shape, 9 = per call
 *   "mha_mfma"          TF_MHA_MFMA          0..2 [1], default 1   tf_mha_core_f32: 1 = operands streamed into registers, 2 = K / V staged in
 *                       LDS, 0 = the vector kernel.  (Until the knobs shared a table this one returned -1 before the first attention
 *                       call, and an out-of-range TF_MHA_MFMA selected the LDS-staged kernel; both follow the common rule now.)
 *   "wgrad_msplit"      -                    1..64 [0], default 0  chunks the row loop of tf_linear_wgrad_split_f32 is cut into (0 = per shape).
 *                       Unlike the other knobs it changes the summation order of dw -- and the workspace tf_linear_wgrad_workspace_bytes asks for
 * Knobs of experiments that were measured and removed (linear_variant, linear_bufstore, linear_deep, linear_astat,
 * conv3_bufload, bwd_sorted2, tiled = 1) are unknown names now.
 */
int tf_msda_set_option(const char *name, int value);

/*
 * Debug aid of tools/msda_bench --trace (not part of the operator contract): while `device_buffer` is not
 * NULL, every workgroup of msda_fwd_f32_quad writes 16 uint64 phase timestamps (s_memrealtime, 100 MHz) to
 * device_buffer[16 * blockIdx + i].  The buffer must hold 16 * grid entries; pass NULL to switch it off.
 */
void tf_msda_debug_trace_buffer(void *device_buffer);

/*
 * Forward.  out[N,Lq,M*D] = sum_{l,p} attn * bilinear(value_l, loc)      (Appendix A of SURVEY.md)
 *
 * shapes_hw_host : HOST pointer to L*2 int64 (H_l, W_l).  Passed by value to the kernel; nothing is
 *                  read from it after the call returns.
 * replaces ms_deform_attn_cuda_forward (cu:19-86) + ms_deformable_im2col_gpu_kernel (cuh:165-237).
 */
int tf_msda_forward_f32(const float *value, const int64_t *shapes_hw_host, const float *loc,
                        const float *attn, float *out, int N, int S, int M, int D, int L, int Lq,
                        int P, void *stream);
int tf_msda_forward_f64(const double *value, const int64_t *shapes_hw_host, const double *loc,
                        const double *attn, double *out, int N, int S, int M, int D, int L, int Lq,
                        int P, void *stream);

/*
 * Same, but the level shapes are read from DEVICE memory inside the kernel (what the reference does,
 * cuh:194-196) -- for callers that only hold the reference's device-resident `spatial_shapes` tensor
 * and must not synchronise.  sum_l H_l*W_l == S is the caller's responsibility (not checkable without a
 * device->host copy).
 */
int tf_msda_forward_f32_dshapes(const float *value, const int64_t *shapes_hw_dev, const float *loc,
                                const float *attn, float *out, int N, int S, int M, int D, int L,
                                int Lq, int P, void *stream);
int tf_msda_forward_f64_dshapes(const double *value, const int64_t *shapes_hw_dev,
                                const double *loc, const double *attn, double *out, int N, int S,
                                int M, int D, int L, int Lq, int P, void *stream);

/*
 * Forward with the operator's prologue fused in (fp32, inference): takes the RAW outputs of the query
 * projections and the reference points and performs softmax + sampling-location arithmetic inside the
 * kernel.  Replaces ops/modules/ms_deform_attn.py:69-86 (view / softmax / location arithmetic /
 * MSDeformAttnFunction.apply) in one launch.
 *   ref_points [N, Lq, L, ref_dim]   ref_dim 2: loc = ref + off / (H_l, W_l)   (x with H_l, y with W_l,
 *                                               exactly as ms_deform_attn.py:78-79 is written)
 *                                    ref_dim 4: loc = ref[:2] + off / P * ref[2:] * 0.5   (:81-82)
 *   qproj      [N*Lq, ld] floats; row r holds the query's M*L*P*2 raw offsets (order m, l, p, xy) starting
 *              at column off_col and its M*L*P attention logits (order m, l, p) at column logit_col
 *              (e.g. one GEMM with the two Linear weights concatenated: ld = 3*M*L*P, off_col = 0,
 *              logit_col = 2*M*L*P).  off_col and ld must be even.
 * Requires D % 4 == 0, P in {1,2,4,8}, 16-byte aligned value/out, tensors < 4 GiB.
 */
int tf_msda_forward_fused_f32(const float *value, const int64_t *shapes_hw_host,
                              const float *ref_points, int ref_dim, const float *qproj, int ld,
                              int off_col, int logit_col, float *out, int N, int S, int M, int D,
                              int L, int Lq, int P, void *stream);

/*
 * Backward.  Writes all three gradients; grad_value is zero-filled on `stream` by the library before
 * accumulation (reference: at::zeros_like, cu:119-121), grad_loc / grad_attn are fully overwritten.
 * grad_value accumulation uses hardware floating-point atomics, so its summation order (and therefore
 * its last bits) is not deterministic -- as in the reference (cuh:301).  tf_msda_backward_det_* below is the
 * bitwise-reproducible form.
 * replaces ms_deform_attn_cuda_backward (cu:89-168) + ms_deformable_col2im_gpu_kernel (cuh:239-306) +
 * ms_deformable_col2im_coord_gpu_kernel (cuh:308-378).
 */
int tf_msda_backward_f32(const float *value, const int64_t *shapes_hw_host, const float *loc,
                         const float *attn, const float *grad_out, float *grad_value,
                         float *grad_loc, float *grad_attn, int N, int S, int M, int D, int L,
                         int Lq, int P, void *stream);
int tf_msda_backward_f64(const double *value, const int64_t *shapes_hw_host, const double *loc,
                         const double *attn, const double *grad_out, double *grad_value,
                         double *grad_loc, double *grad_attn, int N, int S, int M, int D, int L,
                         int Lq, int P, void *stream);
int tf_msda_backward_f32_dshapes(const float *value, const int64_t *shapes_hw_dev, const float *loc,
                                 const float *attn, const float *grad_out, float *grad_value,
                                 float *grad_loc, float *grad_attn, int N, int S, int M, int D,
                                 int L, int Lq, int P, void *stream);
int tf_msda_backward_f64_dshapes(const double *value, const int64_t *shapes_hw_dev,
                                 const double *loc, const double *attn, const double *grad_out,
                                 double *grad_value, double *grad_loc, double *grad_attn, int N,
                                 int S, int M, int D, int L, int Lq, int P, void *stream);

/*
 * Deterministic backward (opt-in; the entry points above are unchanged).  Same arguments and the same three gradients, computed
 * without any floating-point atomic (csrc/msda_bwd_det.h): every contribution a * w_c to grad_value is stored once, the
 * contributions of each (batch, head) block are put in destination-row order by a stable radix sort, and every row is summed
 * in that fixed order and written once by plain stores.  For a fixed build of the library and a fixed device model grad_value,
 * grad_loc and grad_attn are a pure function of the tensor contents and the dimensions: bit-identical across repeated calls,
 * streams, HIP-graph replay, concurrent work on the device, the host-shape / _dshapes entry points, every tf_msda_set_option /
 * environment knob, and whatever the workspace and the output buffers held on entry.  Two consequences:
 *   - batch invariance: the gradients of batch element n do not depend on N or on the other elements;
 *   - no zero-fill pass: every element of grad_value is written exactly once; rows nobody samples get +0.
 * Accuracy is that of the default kernels (fp32 / fp64 products and sums; only the order of the sums differs).  It is slower
 * than the default path and meant for reproducing and bisecting training runs.
 *
 * workspace: DEVICE memory owned by the caller, 8-byte aligned, at least tf_msda_backward_det_workspace_bytes(...) bytes, not
 *   shared with a call that may run at the same time; contents on entry are irrelevant, nothing is kept in it between calls.
 *   Only kernels are enqueued: the call is HIP-graph capturable.
 * tf_msda_backward_det_workspace_bytes(elem_bytes = 4 | 8, ...): the size, or TF_MSDA_ERR_BAD_DIMS (as int64) for a
 *   non-positive dimension, L > TF_MSDA_MAX_LEVELS, another elem_bytes, or a block whose 4*Lq*L*P corner slots do not fit 32
 *   bits.  With I = 4*Lq*L*P (corner slots per (batch, head) block), T = ceil(I / 1024) (radix tiles) and r256 = round up to 256:
 *       per chunk of nb images:  4 * r256(4 * nb*M*I)              keys and slot indices, double-buffered
 *                              +     r256(elem_bytes * nb*M*I)     weights
 *                              +     r256(1024 * nb*M*T)           digit histograms
 *                              +     r256(4 * nb*M*(S + 1))        row bounds
 *   nb = the number of images whose workspace fits 512 MiB (at least 1, at most N): the batch is walked nb images at a time,
 *   which does not change any result.  The 512 MiB are a constant of the build (kDetBatchBudget, csrc/msda_bwd_det.h), not an
 *   option.  The size therefore depends on EVERY dimension, N included (through nb, until the budget is reached): ask again
 *   whenever a dimension changes -- a buffer sized for one image is too small for N = 2 where two images fit the budget, and
 *   the call then returns TF_MSDA_ERR_WORKSPACE.  fp32 at the cfg-2 encoder shape (S = Lq = 22 223, M = 8, L = P = 4): 240 MB per image.
 * Status: NULL pointer (workspace included) -> TF_MSDA_ERR_NULL_POINTER; dimensions -> TF_MSDA_ERR_BAD_DIMS; a short or misaligned
 *   workspace -> TF_MSDA_ERR_WORKSPACE; shape sum != S -> TF_MSDA_ERR_SHAPE_SUM -- checked in that order, before any GPU work.
 * tf_msda_last_kernel() reports "msda_bwd_det<f32>" / "msda_bwd_det<f64>".
 */
int64_t tf_msda_backward_det_workspace_bytes(int elem_bytes, int N, int S, int M, int D, int L, int Lq, int P);
int tf_msda_backward_det_f32(const float *value, const int64_t *shapes_hw_host, const float *loc, const float *attn,
                             const float *grad_out, float *grad_value, float *grad_loc, float *grad_attn, void *workspace,
                             int64_t workspace_bytes, int N, int S, int M, int D, int L, int Lq, int P, void *stream);
int tf_msda_backward_det_f64(const double *value, const int64_t *shapes_hw_host, const double *loc, const double *attn,
                             const double *grad_out, double *grad_value, double *grad_loc, double *grad_attn, void *workspace,
                             int64_t workspace_bytes, int N, int S, int M, int D, int L, int Lq, int P, void *stream);
int tf_msda_backward_det_f32_dshapes(const float *value, const int64_t *shapes_hw_dev, const float *loc, const float *attn,
                                     const float *grad_out, float *grad_value, float *grad_loc, float *grad_attn,
                                     void *workspace, int64_t workspace_bytes, int N, int S, int M, int D, int L, int Lq, int P,
                                     void *stream);
int tf_msda_backward_det_f64_dshapes(const double *value, const int64_t *shapes_hw_dev, const double *loc, const double *attn,
                                     const double *grad_out, double *grad_value, double *grad_loc, double *grad_attn,
                                     void *workspace, int64_t workspace_bytes, int N, int S, int M, int D, int L, int Lq, int P,
                                     void *stream);

/*
 * Training through the fused entry (fp32).  tf_msda_forward_fused_f32 keeps neither loc nor attn; these two entries let a
 * backward recompute them and carry the gradients of the operator's backward back to the RAW projection, so that a caller
 * (trackformer_amd.msda.ms_deform_attn_fused) saves only value, ref_points and qproj:
 *     tf_msda_fused_prologue_f32 -> tf_msda_backward_f32 or tf_msda_backward_det_f32 on (loc, attn) -> tf_msda_fused_backward_epilogue_f32
 * Arguments as tf_msda_forward_fused_f32 (ref_points, ref_dim, qproj, ld, off_col, logit_col, shapes_hw_host); there is no
 * value and no S: the level shapes only supply the divisors of the 2-d formula, so TF_MSDA_ERR_SHAPE_SUM cannot occur here.
 *
 * tf_msda_fused_prologue_f32 writes the fused entry's own prologue (csrc/msda_fused_bwd.h):
 *   loc  [N, Lq, M, L, P, 2]   ref_dim 2: ref + off / (H_l, W_l)   (x over H_l, as above);  ref_dim 4: ref[:2] + off / P * ref[2:] * 0.5
 *   attn [N, Lq, M, L, P]      softmax over the head's L*P logits (max-subtracted exponential)
 *   in plain fp32 (IEEE division and add, __expf): within 2^-22 |off term| + 2^-23 |loc| and within the softmax bound of
 *   tests/util_msda_numerics.py (fused_locations) of the float64 result.  The forward kernels round the same formulas in their
 *   own way (v_rcp_f32 in the LDS-window kernels), so loc / attn agree with what the forward sampled to those bounds, not bit for bit.
 *
 * tf_msda_fused_backward_epilogue_f32: with a = attn, ga = grad_attn, gl = grad_loc (both as tf_msda_backward_* writes them)
 *   grad_logit_i        = a_i (ga_i - sum_j a_j ga_j)                      j over the head's L*P, in index order
 *   grad_off            = gl / (H_l, W_l)        (ref_dim 2)      gl * ref[2:] * 0.5 / P   (ref_dim 4)
 *   grad_ref[n,q,l,:2]  = sum_{m,p} gl                                     (m, p) in index order
 *   grad_ref[n,q,l,2:]  = sum_{m,p} gl * off * 0.5 / P                     (ref_dim 4)
 *   A sample out of range (the operator kernels' test, -1 < fma(loc, size, -0.5) < size per coordinate, on the location the prologue
 *   writes) takes no part in the forward: its ga / gl are read as 0 whatever the buffers hold.  tf_msda_backward_* leaves 0 there for
 *   finite inputs (nothing changes) but NaN * 0 = NaN under a NaN in grad_out, where the gradient is 0.
 *   grad_qproj [N*Lq, ld_g]: row r receives grad_off in columns [goff_col, goff_col + 2*M*L*P) and grad_logit in
 *   [glogit_col, glogit_col + M*L*P) (the layout of qproj, with its own ld_g / columns; the two ranges must not overlap);
 *   every other element of the buffer is left alone.  grad_ref [N, Lq, L, ref_dim] may be NULL: it is then not computed.
 *
 * Both: no atomic of any kind, every output element is written once by a plain store, every sum runs in an order the
 * dimensions fix: the results are bit-identical across calls, streams and HIP-graph replay.  Only kernels are enqueued on
 * `stream` (no memset, no workspace): HIP-graph capturable.
 * Requires L <= TF_MSDA_MAX_LEVELS, P in {1,2,4,8}, ref_dim in {2,4}, M*L*P <= 2048 (a workgroup stages whole rows in LDS),
 * even ld / off_col / ld_g / goff_col, columns inside ld / ld_g, 8-byte aligned qproj / loc / grad_loc / grad_qproj, tensors < 4 GiB.
 * Status: NULL pointer (grad_ref excepted) -> TF_MSDA_ERR_NULL_POINTER, then everything else -> TF_MSDA_ERR_BAD_DIMS, before any GPU work.
 * tf_msda_last_kernel() reports "msda_fused_prologue<f32>" / "msda_fused_bwd_epilogue<f32>".
 */
int tf_msda_fused_prologue_f32(const float *ref_points, int ref_dim, const float *qproj, int ld, int off_col, int logit_col,
                               const int64_t *shapes_hw_host, float *loc, float *attn, int N, int M, int L, int Lq, int P,
                               void *stream);
int tf_msda_fused_backward_epilogue_f32(const float *ref_points, int ref_dim, const float *qproj, int ld, int off_col,
                                        int logit_col, const int64_t *shapes_hw_host, const float *attn, const float *grad_loc,
                                        const float *grad_attn, float *grad_qproj, int ld_g, int goff_col, int glogit_col,
                                        float *grad_ref, int N, int M, int L, int Lq, int P, void *stream);

/*
 * The operator for HOST tensors: every pointer is a host pointer, the call computes synchronously on the calling thread
 * plus worker threads (split by batch x head: no atomics, deterministic gradients) and returns when done.
 * The reference has no CPU implementation -- ms_deform_attn.h:27,48 raise "Not implemented on the CPU",
 * cpu/ms_deform_attn_cpu.cpp:17-40 are stubs -- SURVEY.md section 8(b) asks for a real one in place of the error.  Reached
 * only for tensors that already live in host memory; the device entry points above never fall back to it.
 * grad_value is zero-filled by the call, grad_loc / grad_attn are fully overwritten.
 */
int tf_msda_forward_host_f32(const float *value, const int64_t *shapes_hw, const float *loc, const float *attn,
                             float *out, int N, int S, int M, int D, int L, int Lq, int P);
int tf_msda_forward_host_f64(const double *value, const int64_t *shapes_hw, const double *loc, const double *attn,
                             double *out, int N, int S, int M, int D, int L, int Lq, int P);
int tf_msda_backward_host_f32(const float *value, const int64_t *shapes_hw, const float *loc, const float *attn,
                              const float *grad_out, float *grad_value, float *grad_loc, float *grad_attn, int N,
                              int S, int M, int D, int L, int Lq, int P);
int tf_msda_backward_host_f64(const double *value, const int64_t *shapes_hw, const double *loc, const double *attn,
                              const double *grad_out, double *grad_value, double *grad_loc, double *grad_attn, int N,
                              int S, int M, int D, int L, int Lq, int P);

#ifdef __cplusplus
}
#endif
#endif /* TF_MSDA_H_ */
