// trackformer_amd/csrc/dropout_train.h -- dropout decided inside the training kernels (included from fused_ops.hip next to
// layernorm_bwd.h, whose kernel runs the backward below under its dropout policy; include/tf_fused.h: DROPOUT INSIDE THE TRAINING
// KERNELS; the generator: dropout_rng.h).
//
//   d = keep scale res   (exactly 0 where dropped, whatever res holds there),   z = x + d   (one fp32 product, one fp32 addition, never
//   contracted into an fma: the backward forms the same z again)
//   forward:   out = LayerNorm(z) gamma + beta,  stats[r] = (mean, rstd)
//   backward:  dz as tf_add_layernorm_bwd_f32 from the rebuilt z;  dx = dz,  dres = keep scale dz  (exactly 0 where dropped)
//
// No mask and no dropped tensor exist: both passes compute the keep decision of element i from (seed, offset, i).  The BACKWARD is
// add_layernorm_bwd_kernel<., ., LnDropout> (layernorm_bwd.h): one body, whose instantiations without dropout compile to the instruction
// stream they had alone.  The FORWARD stays a body of its own next to add_layernorm_kernel: that kernel reads blockDim / gridDim, and a
// dropout parameter on its template changed the code of every existing instantiation and the floating-point sequence of `out`, which
// must keep the bits of the inference path (see the comment at its STATS branch).
#ifndef TF_DROPOUT_TRAIN_H_
#define TF_DROPOUT_TRAIN_H_

namespace {

// ---- the keep decisions themselves, one thread per group of four elements
__global__ void __launch_bounds__(256)
dropout_keep_u8_kernel(const long long *__restrict__ rng, unsigned T, long long g0, long long ngroups, unsigned *__restrict__ keep)
{
    const tfd::Stream st = tfd::load_stream(rng);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < ngroups; i += stride) {
        const unsigned b = tfd::keep_bits(st, (unsigned long long)(g0 + i), T);
        keep[i] = (b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21);   // four 0 / 1 bytes, element 4 i first
    }
}

// ---- y <- keep scale y, 16 bytes per lane, grid-stride
__global__ void __launch_bounds__(256)
dropout_inplace_kernel(float *__restrict__ y, const long long *__restrict__ rng, unsigned T, float scale, long long n4)
{
    const tfd::Stream st = tfd::load_stream(rng);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const f32x4_t v = reinterpret_cast<const f32x4_t *>(y)[i];
        tfm::stream_store(reinterpret_cast<f32x4_t *>(y) + i, dropout_apply(v, tfd::keep_bits(st, (unsigned long long)i, T), scale));
    }
}

// ---- out = y > 0 ? dy scale : 0: y is the dropped-and-scaled ReLU output, positive exactly where the unit was active AND kept
__global__ void __launch_bounds__(256)
relu_dropout_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ y, float scale, float *__restrict__ out, long long n4)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const f32x4_t d = reinterpret_cast<const f32x4_t *>(dy)[i];
        const f32x4_t v = reinterpret_cast<const f32x4_t *>(y)[i];
        f32x4_t o;
        o.x = v.x > 0.f ? d.x * scale : 0.f;
        o.y = v.y > 0.f ? d.y * scale : 0.f;
        o.z = v.z > 0.f ? d.z * scale : 0.f;
        o.w = v.w > 0.f ? d.w * scale : 0.f;
        tfm::stream_store(reinterpret_cast<f32x4_t *>(out) + i, o);
    }
}

// ---- the forward: the row layout of add_layernorm_kernel (one wave per row, lane j the float4 chunks j, j + 64, ...)
template <int MAXCH>
__global__ void __launch_bounds__(256)
add_dropout_layernorm_kernel(const float *__restrict__ x, const float *__restrict__ res, const float *__restrict__ gamma,
                             const float *__restrict__ beta, const long long *__restrict__ rng, unsigned T, float scale,
                             float *__restrict__ out, float *__restrict__ stats, long long rows, int C, float eps)
{
    const tfd::Stream st = tfd::load_stream(rng);
    const int lane = threadIdx.x & 63;
    const int C4 = C >> 2;
    const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long r = wave0; r < rows; r += nwaves) {
        const f32x4_t *xr = reinterpret_cast<const f32x4_t *>(x + r * C);
        const f32x4_t *rr = reinterpret_cast<const f32x4_t *>(res + r * C);
        f32x4_t v[MAXCH];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < MAXCH; ++k) {
            const int j = lane + k * 64;
            v[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            if (j < C4) {
                const unsigned bits = tfd::keep_bits(st, (unsigned long long)(r * C4 + j), T);
                v[k] = add_uncontracted(xr[j], dropout_apply(rr[j], bits, scale));
                s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
            }
        }
        const float mean = wave_sum(s) / (float)C;
        float sq = 0.f;
#pragma unroll
        for (int k = 0; k < MAXCH; ++k) {
            const int j = lane + k * 64;
            if (j < C4) {
                const f32x4_t d = v[k] - mean;
                sq += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
            }
        }
        const float rstd = rsqrtf(wave_sum(sq) / (float)C + eps);
        f32x4_t *orow = reinterpret_cast<f32x4_t *>(out + r * C);
#pragma unroll
        for (int k = 0; k < MAXCH; ++k) {
            const int j = lane + k * 64;
            if (j < C4) {
                const f32x4_t g = reinterpret_cast<const f32x4_t *>(gamma)[j];
                const f32x4_t b = reinterpret_cast<const f32x4_t *>(beta)[j];
                tfm::stream_store(orow + j, (v[k] - mean) * rstd * g + b);
            }
        }
        if (lane == 0) reinterpret_cast<f32x2_t *>(stats)[r] = f32x2_t{mean, rstd};
    }
}

}  // namespace

extern "C" int tf_dropout_keep_u8(const int64_t *rng, float p, int64_t first, int64_t n, uint8_t *keep, void *stream)
{
    if (!rng || !keep) return TF_MSDA_ERR_NULL_POINTER;
    if (!tfd::dropout_p_ok(p) || first < 0 || n <= 0 || (first & 3) || (n & 3) || first > INT64_MAX - n) return TF_MSDA_ERR_BAD_DIMS;
    if (!word_aligned8(rng) || (reinterpret_cast<uintptr_t>(keep) & 3)) return TF_MSDA_ERR_BAD_DIMS;
    const long long ngroups = n / 4;
    hipLaunchKernelGGL(dropout_keep_u8_kernel, dim3((unsigned)stream_blocks(ngroups)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const long long *>(rng), tfd::dropout_threshold(p), (long long)(first / 4), ngroups,
                       reinterpret_cast<unsigned *>(keep));
    if (int rc = tfm::launched()) return rc;
    tfm::note_kernel("dropout_keep_u8");
    return TF_MSDA_OK;
}

extern "C" int tf_dropout_inplace_f32(float *y, const int64_t *rng, float p, int64_t n, void *stream)
{
    if (!y || !rng) return TF_MSDA_ERR_NULL_POINTER;
    if (!tfd::dropout_p_ok(p) || n <= 0 || (n & 3) || !aligned16(y) || !word_aligned8(rng)) return TF_MSDA_ERR_BAD_DIMS;
    hipLaunchKernelGGL(dropout_inplace_kernel, dim3((unsigned)stream_blocks(n / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), y,
                       reinterpret_cast<const long long *>(rng), tfd::dropout_threshold(p), tfd::dropout_scale(p), (long long)(n / 4));
    if (int rc = tfm::launched()) return rc;
    tfm::note_kernel("dropout_inplace_f32");
    return TF_MSDA_OK;
}

extern "C" int tf_relu_dropout_bwd_f32(const float *dy, const float *y, float p, float *out, int64_t n, void *stream)
{
    if (!dy || !y || !out) return TF_MSDA_ERR_NULL_POINTER;
    if (!tfd::dropout_p_ok(p) || n <= 0 || (n & 3) || !aligned16(dy) || !aligned16(y) || !aligned16(out)) return TF_MSDA_ERR_BAD_DIMS;
    hipLaunchKernelGGL(relu_dropout_bwd_kernel, dim3((unsigned)stream_blocks(n / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), dy, y,
                       tfd::dropout_scale(p), out, (long long)(n / 4));
    if (int rc = tfm::launched()) return rc;
    tfm::note_kernel("relu_dropout_bwd_f32");
    return TF_MSDA_OK;
}

extern "C" int tf_add_dropout_layernorm_train_f32(const float *x, const float *res, const float *gamma, const float *beta, const int64_t *rng,
                                                  float p, float *out, float *stats, int64_t rows, int C, float eps, void *stream)
{
    if (!x || !res || !gamma || !beta || !rng || !out || !stats) return TF_MSDA_ERR_NULL_POINTER;
    if (!tfd::dropout_p_ok(p) || rows <= 0 || rows > 0x7fffffffLL || C <= 0 || (C & 3) || C > 4096) return TF_MSDA_ERR_BAD_DIMS;
    if (!aligned16(x) || !aligned16(res) || !aligned16(gamma) || !aligned16(beta) || !aligned16(out) || !word_aligned8(stats) || !word_aligned8(rng))
        return TF_MSDA_ERR_BAD_DIMS;
    const unsigned blocks = (unsigned)stream_blocks(rows, 4);   // 4 waves (rows) per 256-thread workgroup
    const unsigned T = tfd::dropout_threshold(p);
    const float scale = tfd::dropout_scale(p);
    with_maxch(C, [&](auto maxch) {
        hipLaunchKernelGGL(add_dropout_layernorm_kernel<decltype(maxch)::value>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), x, res,
                           gamma, beta, reinterpret_cast<const long long *>(rng), T, scale, out, stats, (long long)rows, C, eps);
    });
    if (int rc = tfm::launched()) return rc;
    tfm::note_kernel("add_dropout_layernorm_stats_f32");
    return TF_MSDA_OK;
}

// add_layernorm_bwd_impl (layernorm_bwd.h) with the dropout policy; this entry's own: res is required, rng, p, and dres next to dx
extern "C" int tf_add_dropout_layernorm_bwd_f32(const float *dy, const float *x, const float *res, const float *gamma, const float *stats,
                                                const int64_t *rng, float p, float *dx, float *dres, float *dgamma, float *dbeta, void *workspace,
                                                int64_t workspace_bytes, int64_t rows, int C, void *stream)
{
    const bool p_ok = tfd::dropout_p_ok(p);   // (threshold and scale are defined for such a p only; any other is refused before they are read)
    const LnDropout drop{reinterpret_cast<const long long *>(rng), p_ok ? tfd::dropout_threshold(p) : 0u, p_ok ? tfd::dropout_scale(p) : 0.f, dres};
    return add_layernorm_bwd_impl("add_dropout_layernorm_bwd_f32", !res || !rng, !p_ok || !word_aligned8(rng) || (dres && !aligned16(dres)), dy, x, res,
                                  gamma, stats, dx, dgamma, dbeta, workspace, workspace_bytes, rows, C, stream, drop);
}

#endif /* TF_DROPOUT_TRAIN_H_ */
