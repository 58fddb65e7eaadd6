// trackformer_amd/csrc/dropout_train.h -- dropout decided inside the training kernels (included from fused_ops.hip next to
// layernorm_bwd.h, whose row-block rule, workspace and column reduction the backward below shares; include/tf_fused.h: DROPOUT INSIDE THE
// TRAINING KERNELS; the generator: dropout_rng.h).
//
//   d = keep scale res   (exactly 0 where dropped, whatever res holds there),   z = x + d   (one fp32 product, one fp32 addition, never
//   contracted into an fma: the backward forms the same z again)
//   forward:   out = LayerNorm(z) gamma + beta,  stats[r] = (mean, rstd)
//   backward:  dz as tf_add_layernorm_bwd_f32 from the rebuilt z;  dx = dz,  dres = keep scale dz  (exactly 0 where dropped)
//
// No mask and no dropped tensor exist: both passes compute the keep decision of element i from (seed, offset, i).  The bodies are separate
// from add_layernorm_kernel / add_layernorm_bwd_kernel on purpose: those keep their instruction streams.
#ifndef TF_DROPOUT_TRAIN_H_
#define TF_DROPOUT_TRAIN_H_

namespace {

// keep scale v of one 16-byte group: a select, never a product with 0 (a dropped inf / NaN is 0), and a product the caller cannot
// contract with its next addition
__device__ __forceinline__ f32x4_t dropout_apply(f32x4_t v, unsigned bits, float scale)
{
#pragma clang fp contract(off)
    f32x4_t d;
    d.x = (bits & 1u) ? v.x * scale : 0.f;
    d.y = (bits & 2u) ? v.y * scale : 0.f;
    d.z = (bits & 4u) ? v.z * scale : 0.f;
    d.w = (bits & 8u) ? v.w * scale : 0.f;
    return d;
}

__device__ __forceinline__ f32x4_t add_uncontracted(f32x4_t a, f32x4_t b)
{
#pragma clang fp contract(off)
    return a + b;
}

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

// ---- the backward: the blocks, waves, partial rows and LDS hand-over of add_layernorm_bwd_kernel; z from the recomputed mask
template <int MAXCH, bool PARTIALS>
__global__ void __launch_bounds__(256)
add_dropout_layernorm_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ x, const float *__restrict__ res,
                                 const float *__restrict__ gamma, const float *__restrict__ stats, const long long *__restrict__ rng,
                                 unsigned T, float scale, float *__restrict__ dx, float *__restrict__ dres, float *__restrict__ partial,
                                 long long rows, int C, int rows_per)
{
    __shared__ f32x4_t s_part[3][2][64];   // (PARTIALS) what waves 1 .. 3 hand to wave 0, one chunk at a time
    const tfd::Stream st = tfd::load_stream(rng);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C4 = C >> 2;
    const long long r0 = (long long)blockIdx.x * rows_per;
    const long long r1 = r0 + rows_per < rows ? r0 + rows_per : rows;
    f32x4_t ga[MAXCH], sb[MAXCH], sg[MAXCH];
#pragma unroll
    for (int k = 0; k < MAXCH; ++k) {
        const int j = lane + k * 64;
        ga[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        if (j < C4) ga[k] = reinterpret_cast<const f32x4_t *>(gamma)[j];
        if constexpr (PARTIALS) {
            sb[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            sg[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
    }
    for (long long r = r0 + wave; r < r1; r += 4) {   // (wave-uniform)
        const f32x4_t *xr = reinterpret_cast<const f32x4_t *>(x + r * C);
        const f32x4_t *rr = reinterpret_cast<const f32x4_t *>(res + r * C);
        const f32x4_t *dr = reinterpret_cast<const f32x4_t *>(dy + r * C);
        const f32x2_t sm = reinterpret_cast<const f32x2_t *>(stats)[r];
        const float mean = sm.x, rstd = sm.y;
        f32x4_t xh[MAXCH], g[MAXCH];
        unsigned bits[MAXCH];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < MAXCH; ++k) {
            const int j = lane + k * 64;
            xh[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            g[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            bits[k] = 0u;
            if (j < C4) {
                bits[k] = tfd::keep_bits(st, (unsigned long long)(r * C4 + j), T);
                const f32x4_t z = add_uncontracted(xr[j], dropout_apply(rr[j], bits[k], scale));   // the forward's z, bit for bit
                const f32x4_t d = dr[j];
                xh[k] = (z - mean) * rstd;
                g[k] = ga[k] * d;
                const f32x4_t gx = g[k] * xh[k];
                s1 += (g[k].x + g[k].y) + (g[k].z + g[k].w);
                s2 += (gx.x + gx.y) + (gx.z + gx.w);
                if constexpr (PARTIALS) {
                    sb[k] += d;
                    sg[k] += d * xh[k];
                }
            }
        }
        const float c1 = wave_sum(s1) / (float)C, c2 = wave_sum(s2) / (float)C;
        if (dx != nullptr || dres != nullptr) {   // (uniform)
#pragma unroll
            for (int k = 0; k < MAXCH; ++k) {
                const int j = lane + k * 64;
                if (j < C4) {
                    const f32x4_t dz = (g[k] - c1 - xh[k] * c2) * rstd;
                    if (dx != nullptr) tfm::stream_store(reinterpret_cast<f32x4_t *>(dx + r * C) + j, dz);
                    if (dres != nullptr) tfm::stream_store(reinterpret_cast<f32x4_t *>(dres + r * C) + j, dropout_apply(dz, bits[k], scale));
                }
            }
        }
    }
    if constexpr (PARTIALS) {
        f32x4_t *prow = reinterpret_cast<f32x4_t *>(partial + (size_t)blockIdx.x * 2 * C);
#pragma unroll
        for (int k = 0; k < MAXCH; ++k) {
            if (k * 64 < C4) {   // (uniform)
                if (wave > 0) {
                    s_part[wave - 1][0][lane] = sb[k];
                    s_part[wave - 1][1][lane] = sg[k];
                }
                __syncthreads();
                const int j = lane + k * 64;
                if (wave == 0 && j < C4) {
                    f32x4_t tb = sb[k], tg = sg[k];
#pragma unroll
                    for (int w = 0; w < 3; ++w) {
                        tb += s_part[w][0][lane];
                        tg += s_part[w][1][lane];
                    }
                    prow[j] = tb;
                    prow[C4 + j] = tg;
                }
                __syncthreads();
            }
        }
    }
}

template <int MAXCH>
void launch_add_dropout_layernorm_bwd(bool partials, unsigned blocks, hipStream_t s, const float *dy, const float *x, const float *res,
                                      const float *gamma, const float *stats, const long long *rng, unsigned T, float scale, float *dx,
                                      float *dres, float *partial, long long rows, int C, int rows_per)
{
    if (partials)
        hipLaunchKernelGGL((add_dropout_layernorm_bwd_kernel<MAXCH, true>), dim3(blocks), dim3(256), 0, s, dy, x, res, gamma, stats, rng, T, scale,
                           dx, dres, partial, rows, C, rows_per);
    else
        hipLaunchKernelGGL((add_dropout_layernorm_bwd_kernel<MAXCH, false>), dim3(blocks), dim3(256), 0, s, dy, x, res, gamma, stats, rng, T, scale,
                           dx, dres, partial, rows, C, rows_per);
}

long long stream_blocks(long long n4)   // grid-stride beyond 16 workgroups per CU, as tf_bias_act_f32
{
    const long long blocks = (n4 + 255) / 256;
    return blocks > 256 * 16 ? 256 * 16 : blocks;
}

bool word_aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

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
    if (hipGetLastError() != hipSuccess) return TF_MSDA_ERR_LAUNCH;
    tfm::note_kernel("dropout_keep_u8");
    return TF_MSDA_OK;
}

extern "C" int tf_dropout_inplace_f32(float *y, const int64_t *rng, float p, int64_t n, void *stream)
{
    if (!y || !rng) return TF_MSDA_ERR_NULL_POINTER;
    if (!tfd::dropout_p_ok(p) || n <= 0 || (n & 3) || !aligned16(y) || !word_aligned8(rng)) return TF_MSDA_ERR_BAD_DIMS;
    hipLaunchKernelGGL(dropout_inplace_kernel, dim3((unsigned)stream_blocks(n / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), y,
                       reinterpret_cast<const long long *>(rng), tfd::dropout_threshold(p), tfd::dropout_scale(p), (long long)(n / 4));
    if (hipGetLastError() != hipSuccess) return TF_MSDA_ERR_LAUNCH;
    tfm::note_kernel("dropout_inplace_f32");
    return TF_MSDA_OK;
}

extern "C" int tf_relu_dropout_bwd_f32(const float *dy, const float *y, float p, float *out, int64_t n, void *stream)
{
    if (!dy || !y || !out) return TF_MSDA_ERR_NULL_POINTER;
    if (!tfd::dropout_p_ok(p) || n <= 0 || (n & 3) || !aligned16(dy) || !aligned16(y) || !aligned16(out)) return TF_MSDA_ERR_BAD_DIMS;
    hipLaunchKernelGGL(relu_dropout_bwd_kernel, dim3((unsigned)stream_blocks(n / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), dy, y,
                       tfd::dropout_scale(p), out, (long long)(n / 4));
    if (hipGetLastError() != hipSuccess) return TF_MSDA_ERR_LAUNCH;
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
    long long blocks = (rows + 3) / 4;   // 4 waves (rows) per 256-thread workgroup
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int chunks = (C / 4 + 63) / 64;
    const unsigned T = tfd::dropout_threshold(p);
    const float scale = tfd::dropout_scale(p);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, res, gamma, beta, reinterpret_cast<const long long *>(rng), T, scale,
                           out, stats, (long long)rows, C, eps);
    };
    if (chunks <= 1) launch(add_dropout_layernorm_kernel<1>);
    else if (chunks <= 2) launch(add_dropout_layernorm_kernel<2>);
    else if (chunks <= 4) launch(add_dropout_layernorm_kernel<4>);
    else launch(add_dropout_layernorm_kernel<16>);
    if (hipGetLastError() != hipSuccess) return TF_MSDA_ERR_LAUNCH;
    tfm::note_kernel("add_dropout_layernorm_stats_f32");
    return TF_MSDA_OK;
}

extern "C" int tf_add_dropout_layernorm_bwd_f32(const float *dy, const float *x, const float *res, const float *gamma, const float *stats,
                                                const int64_t *rng, float p, float *dx, float *dres, float *dgamma, float *dbeta, void *workspace,
                                                int64_t workspace_bytes, int64_t rows, int C, void *stream)
{
    if (!dy || !x || !res || !gamma || !stats || !rng) return TF_MSDA_ERR_NULL_POINTER;
    if (!tfd::dropout_p_ok(p) || rows <= 0 || rows > 0x7fffffffLL || C <= 0 || (C & 3) || C > 4096) return TF_MSDA_ERR_BAD_DIMS;
    if (!aligned16(dy) || !aligned16(x) || !aligned16(res) || !aligned16(gamma) || !word_aligned8(stats) || !word_aligned8(rng) || (dx && !aligned16(dx)) ||
        (dres && !aligned16(dres)) || (dgamma && !aligned16(dgamma)) || (dbeta && !aligned16(dbeta)))
        return TF_MSDA_ERR_BAD_DIMS;
    const bool partials = dgamma != nullptr || dbeta != nullptr;
    const int nb = ln_bwd_blocks(rows);
    if (partials && (!workspace || workspace_bytes < (int64_t)nb * 2 * C * 4 || !aligned16(workspace))) return TF_MSDA_ERR_WORKSPACE;
    if (!partials && dx == nullptr && dres == nullptr) return TF_MSDA_OK;   // nothing asked for
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *partial = partials ? static_cast<float *>(workspace) : nullptr;
    const int rows_per = ln_bwd_rows_per(rows);
    const int chunks = (C / 4 + 63) / 64;
    const unsigned T = tfd::dropout_threshold(p);
    const float scale = tfd::dropout_scale(p);
    const long long *rg = reinterpret_cast<const long long *>(rng);
    if (chunks <= 1)
        launch_add_dropout_layernorm_bwd<1>(partials, (unsigned)nb, s, dy, x, res, gamma, stats, rg, T, scale, dx, dres, partial, (long long)rows, C, rows_per);
    else if (chunks <= 2)
        launch_add_dropout_layernorm_bwd<2>(partials, (unsigned)nb, s, dy, x, res, gamma, stats, rg, T, scale, dx, dres, partial, (long long)rows, C, rows_per);
    else if (chunks <= 4)
        launch_add_dropout_layernorm_bwd<4>(partials, (unsigned)nb, s, dy, x, res, gamma, stats, rg, T, scale, dx, dres, partial, (long long)rows, C, rows_per);
    else
        launch_add_dropout_layernorm_bwd<16>(partials, (unsigned)nb, s, dy, x, res, gamma, stats, rg, T, scale, dx, dres, partial, (long long)rows, C, rows_per);
    if (hipGetLastError() != hipSuccess) return TF_MSDA_ERR_LAUNCH;
    tfm::note_kernel("add_dropout_layernorm_bwd_f32");
    if (partials) {
        const dim3 grid((unsigned)((C / 4 + kLnRedQuads - 1) / kLnRedQuads), 2u);
        hipLaunchKernelGGL(add_layernorm_bwd_reduce_kernel, grid, dim3(256), 0, s, (const float *)partial, dgamma, dbeta, C, nb);
        if (hipGetLastError() != hipSuccess) return TF_MSDA_ERR_LAUNCH;
        tfm::note_kernel("add_layernorm_bwd_reduce_f32");
    }
    return TF_MSDA_OK;
}

#endif /* TF_DROPOUT_TRAIN_H_ */
