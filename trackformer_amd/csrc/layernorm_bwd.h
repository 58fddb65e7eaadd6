// trackformer_amd/csrc/layernorm_bwd.h -- the backward of out = LayerNorm(x + res) gamma + beta (included from fused_ops.hip, whose
// add_layernorm_kernel<MAXCH, true> is the forward that saves the statistics; include/tf_fused.h: THE BACKWARD OF THE RESIDUAL LAYERNORM).
//
//   z = x + res,  xh = (z - mean) rstd  with (mean, rstd) = stats[r] as the forward wrote them,  g = gamma dy
//   dz[r, :]  = rstd (g - mean_c(g) - xh mean_c(g xh))            the gradient of x AND of res: one tensor, written once
//   dgamma[c] = sum_r dy[r, c] xh[r, c]        dbeta[c] = sum_r dy[r, c]
//
// One pass over the rows (add_layernorm_bwd_kernel) + a small column reduction (add_layernorm_bwd_reduce_kernel).  No atomics: the rows
// are cut into blocks by a rule of (rows) alone -- as tf_linear_grad_stats_f32's row blocks (linear_bwd.h: stats_rows_per) --, a
// workgroup's four waves combine through LDS in wave order and write one partial row [2, C] per block, and the second launch adds the
// partials in a fixed tree over the block indices.  Every result is a pure function of the arguments: bit-identical from call to call,
// on any stream and in a captured graph.
#ifndef TF_LAYERNORM_BWD_H_
#define TF_LAYERNORM_BWD_H_

namespace {

// rows per block of the backward pass and the number of blocks: a function of `rows` only (never of the grid, the CU count or the
// occupancy).  16 rows (4 per wave) up to 32 768 rows; beyond, the 2048 blocks -- 8 workgroups on each of 256 CUs -- grow instead.
constexpr int kLnBwdMinRowsPer = 16, kLnBwdMaxBlocks = 2048;
inline int ln_bwd_rows_per(long long rows)
{
    return (int)(rows <= (long long)kLnBwdMinRowsPer * kLnBwdMaxBlocks ? kLnBwdMinRowsPer : (rows + kLnBwdMaxBlocks - 1) / kLnBwdMaxBlocks);
}
inline int ln_bwd_blocks(long long rows) { return (int)((rows + ln_bwd_rows_per(rows) - 1) / ln_bwd_rows_per(rows)); }

constexpr int kLnRedSlices = 16, kLnRedQuads = 16;   // the reduction's workgroup: 16 slices of the block list x 16 column quads

// What dropout adds to the pass (tf_add_dropout_layernorm_bwd_f32; dropout_train.h): the forward was LayerNorm(x + keep scale res), so z
// is rebuilt from the recomputed keep decisions and the gradient of res is keep scale dz, a second store.  LnNoDropout is EMPTY and the
// policy is the kernel's LAST argument: the instantiations without dropout keep the instruction stream they had before the policy existed.
struct LnNoDropout { static constexpr float *dres = nullptr; };
struct LnDropout { const long long *rng; unsigned T; float scale; float *dres; };

// Block b walks rows [b rows_per, (b + 1) rows_per); wave w of its four takes rows w, w + 4, ... of them, one row at a time, lane j the
// float4 chunks j, j + 64, ... as in the forward.  PARTIALS: every lane also sums dy and dy xh of its own columns over the rows its wave
// walks (registers); waves 1 .. 3 hand theirs to wave 0 through LDS, which adds them in wave order and writes partial[b][0] = sum dy,
// partial[b][1] = sum dy xh.  dz is the gradient of x, and without dropout of res as well (with it: drop.dres; res is never null then).
template <int MAXCH, bool PARTIALS, typename DROP>
__global__ void __launch_bounds__(256)
add_layernorm_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ x, const float *__restrict__ res,
                         const float *__restrict__ gamma, const float *__restrict__ stats, float *__restrict__ dz,
                         float *__restrict__ partial, long long rows, int C, int rows_per, DROP drop)
{
    constexpr bool kDrop = std::is_same_v<DROP, LnDropout>;
    __shared__ f32x4_t s_part[3][2][64];   // (PARTIALS) what waves 1 .. 3 hand to wave 0, one chunk at a time
    [[maybe_unused]] tfd::Stream st;
    if constexpr (kDrop) st = tfd::load_stream(drop.rng);
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
        const f32x4_t *rr = kDrop || res ? reinterpret_cast<const f32x4_t *>(res + r * C) : nullptr;
        const f32x4_t *dr = reinterpret_cast<const f32x4_t *>(dy + r * C);
        const f32x2_t sm = reinterpret_cast<const f32x2_t *>(stats)[r];
        const float mean = sm.x, rstd = sm.y;
        f32x4_t xh[MAXCH], g[MAXCH];
        [[maybe_unused]] unsigned bits[MAXCH];   // (kDrop) the keep decisions of the lane's chunks, kept for dres
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < MAXCH; ++k) {
            const int j = lane + k * 64;
            xh[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            g[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            if constexpr (kDrop) bits[k] = 0u;
            if (j < C4) {
                f32x4_t z = xr[j];
                if constexpr (kDrop) {
                    bits[k] = tfd::keep_bits(st, (unsigned long long)(r * C4 + j), drop.T);
                    z = add_uncontracted(z, dropout_apply(rr[j], bits[k], drop.scale));   // the forward's z, bit for bit
                } else if (rr) {
                    z += rr[j];   // the forward's single fp32 addition
                }
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
        // The stores are written out per policy on purpose.  One block for both (the row pointer hoisted, the second store under the
        // policy) compiled to other code on BOTH sides: the instantiations without dropout lost their instruction stream at some MAXCH,
        // and the dropout ones went from 58 to 68 VGPRs at MAXCH 1 (the hoisted pointer).  As written each side is what it was alone.
        if constexpr (!kDrop) {
            if (dz != nullptr) {   // (uniform)
                f32x4_t *orow = reinterpret_cast<f32x4_t *>(dz + r * C);
#pragma unroll
                for (int k = 0; k < MAXCH; ++k) {
                    const int j = lane + k * 64;
                    if (j < C4) tfm::stream_store(orow + j, (g[k] - c1 - xh[k] * c2) * rstd);
                }
            }
        } else if (dz != nullptr || drop.dres != nullptr) {   // (uniform)
#pragma unroll
            for (int k = 0; k < MAXCH; ++k) {
                const int j = lane + k * 64;
                if (j < C4) {
                    const f32x4_t v = (g[k] - c1 - xh[k] * c2) * rstd;
                    if (dz != nullptr) tfm::stream_store(reinterpret_cast<f32x4_t *>(dz + r * C) + j, v);
                    if (drop.dres != nullptr) tfm::stream_store(reinterpret_cast<f32x4_t *>(drop.dres + r * C) + j, dropout_apply(v, bits[k], drop.scale));
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

// blockIdx.y = 0: dbeta from partial[.][0], 1: dgamma from partial[.][1].  Thread (s, c) adds blocks s, s + 16, ... of column quad c in
// that order; the 16 slices are added in the order 0, 1, ... through LDS: a fixed tree over the block indices.
__global__ void __launch_bounds__(256)
add_layernorm_bwd_reduce_kernel(const float *__restrict__ partial, float *__restrict__ dgamma, float *__restrict__ dbeta, int C, int nblocks)
{
    __shared__ f32x4_t s_red[kLnRedSlices][kLnRedQuads];
    float *out = blockIdx.y == 0 ? dbeta : dgamma;
    if (out == nullptr) return;   // (uniform)
    const int C4 = C >> 2;
    const int c = threadIdx.x % kLnRedQuads, s = threadIdx.x / kLnRedQuads;
    const int j = blockIdx.x * kLnRedQuads + c;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    if (j < C4) {
        const f32x4_t *p = reinterpret_cast<const f32x4_t *>(partial) + (size_t)blockIdx.y * C4 + j;
#pragma unroll 4
        for (int b = s; b < nblocks; b += kLnRedSlices) acc += p[(size_t)b * 2 * C4];
    }
    s_red[s][c] = acc;
    __syncthreads();
    if (s == 0 && j < C4) {
        f32x4_t t = s_red[0][c];
#pragma unroll
        for (int i = 1; i < kLnRedSlices; ++i) t += s_red[i][c];
        reinterpret_cast<f32x4_t *>(out)[j] = t;
    }
}

// Both backward entries.  own_null / own_bad: what the entry's own arguments (the dropout entry: res, rng, p, dres) add to the first two
// checks; `name`: what the row pass is noted as.  The checks answer in this order: null pointers, dimensions and alignment, workspace.
template <typename DROP>
int add_layernorm_bwd_impl(const char *name, bool own_null, bool own_bad, const float *dy, const float *x, const float *res, const float *gamma,
                           const float *stats, float *dz, float *dgamma, float *dbeta, void *workspace, int64_t workspace_bytes, int64_t rows,
                           int C, void *stream, DROP drop)
{
    if (own_null || !dy || !x || !gamma || !stats) return TF_MSDA_ERR_NULL_POINTER;
    if (own_bad || rows <= 0 || rows > 0x7fffffffLL || C <= 0 || (C & 3) || C > 4096) return TF_MSDA_ERR_BAD_DIMS;
    if (!aligned16(dy) || !aligned16(x) || (res && !aligned16(res)) || !aligned16(gamma) || !word_aligned8(stats) || (dz && !aligned16(dz)) ||
        (dgamma && !aligned16(dgamma)) || (dbeta && !aligned16(dbeta)))
        return TF_MSDA_ERR_BAD_DIMS;
    const bool partials = dgamma != nullptr || dbeta != nullptr;
    const int nb = ln_bwd_blocks(rows);
    if (partials && (!workspace || workspace_bytes < (int64_t)nb * 2 * C * 4 || !aligned16(workspace))) return TF_MSDA_ERR_WORKSPACE;
    if (!partials && dz == nullptr && drop.dres == nullptr) return TF_MSDA_OK;   // nothing asked for
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *partial = partials ? static_cast<float *>(workspace) : nullptr;
    with_maxch(C, [&](auto maxch) {
        constexpr int MAXCH = decltype(maxch)::value;
        hipLaunchKernelGGL((partials ? add_layernorm_bwd_kernel<MAXCH, true, DROP> : add_layernorm_bwd_kernel<MAXCH, false, DROP>), dim3((unsigned)nb),
                           dim3(256), 0, s, dy, x, res, gamma, stats, dz, partial, (long long)rows, C, ln_bwd_rows_per(rows), drop);
    });
    if (int rc = tfm::launched()) return rc;
    tfm::note_kernel(name);
    if (partials) {
        const dim3 grid((unsigned)((C / 4 + kLnRedQuads - 1) / kLnRedQuads), 2u);
        hipLaunchKernelGGL(add_layernorm_bwd_reduce_kernel, grid, dim3(256), 0, s, (const float *)partial, dgamma, dbeta, C, nb);
        if (int rc = tfm::launched()) return rc;
        tfm::note_kernel("add_layernorm_bwd_reduce_f32");
    }
    return TF_MSDA_OK;
}

}  // namespace

extern "C" int64_t tf_add_layernorm_bwd_workspace_bytes(int64_t rows, int C)
{
    if (rows <= 0 || rows > 0x7fffffffLL || C <= 0 || (C & 3) || C > 4096) return -1;
    return (int64_t)ln_bwd_blocks(rows) * 2 * C * 4;
}

extern "C" int tf_add_layernorm_bwd_f32(const float *dy, const float *x, const float *res, const float *gamma, const float *stats, float *dz,
                                        float *dgamma, float *dbeta, void *workspace, int64_t workspace_bytes, int64_t rows, int C,
                                        void *stream)
{
    return add_layernorm_bwd_impl("add_layernorm_bwd_f32", false, false, dy, x, res, gamma, stats, dz, dgamma, dbeta, workspace, workspace_bytes,
                                  rows, C, stream, LnNoDropout{});
}

#endif /* TF_LAYERNORM_BWD_H_ */
