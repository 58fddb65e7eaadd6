// trackformer_amd/csrc/linear_bwd.h -- the backward of y = x . w^T + b as split products (included at the end of linear_stream.hip,
// whose stream GEMM, split-K second pass and split_product.h it builds on; include/tf_fused.h: THE BACKWARD OF A LINEAR).
//
//   dx[M, K] = dy[M, N] . w[N, K]          tf_linear_dgrad_packed_f32: the stream GEMM with dy as the activation and a packed image of w^T
//   dw[N, K] = sum_m dy[m, n] x[m, k]      tf_linear_wgrad_split_f32: both operands are activations, split inside the kernel
//   db[N]    = sum_m dy[m, n]              tf_linear_grad_stats_f32 (colsum), the pass that also finds the operands' scales
//
// What the forward's fp16 scheme does not cover: its range contract is cut for O(1) activations (a fixed 2^-4, |x| < 1.0e6), and a
// gradient of 1e-6 would vanish into fp16's subnormals.  Here the operands get powers of two per call from their largest magnitudes
// (tf_linear_grad_stats_f32, written to device memory: no host synchronisation) -- ONE for the operand split as the activation (dy: its
// columns are the contraction of the input gradient), one PER COLUMN for the operand split as the weight (x: column k is output channel
// k of dw, what t_n is per output channel in the forward; a column of fp32 subnormals keeps its bits) -- applied as the operand is
// staged and taken out again in the epilogue: both exact.  Six bf16 terms need none of it (bf16 has fp32's exponent range): the scales are 1 there.
// No kernel here uses atomics: sums over rows are two-stage reductions in a fixed order, so every result is a pure function of the
// arguments (bit-identical from call to call, on any stream, in a captured graph).
#ifndef TF_LINEAR_BWD_H_
#define TF_LINEAR_BWD_H_

namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// OPERAND STATISTICS.  Stage 1: block b walks rows [b rows_per, (b + 1) rows_per) of a[M, C]: thread (g, c) of G row groups x TC column
// quads adds rows g, g + G, ... of its float4 column, the row groups are added in the order 0, 1, ... through LDS -> psum[b][C]; the
// largest |a| as a BIT PATTERN (unsigned maximum: NaN > inf > every finite number, so a non-finite element survives the reduction
// where fmaxf would drop it) -> pmax[b], and per column -> pcmax[b][C] for the weight role.  Stage 2: the partials in the order
// b = 0, 1, ... -> colsum; the scale(s) from the maxima.
constexpr int kStatsRole_Activation = 0, kStatsRole_Weight = 1;

// rows per block of stage 1 and the number of blocks: a function of (M, C) only
inline int stats_rows_per(long long M) { return (int)(M <= 64 * 512 ? 64 : (M + 511) / 512); }
inline int stats_blocks(long long M) { return (int)((M + stats_rows_per(M) - 1) / stats_rows_per(M)); }

__global__ void __launch_bounds__(256)
grad_stats_partial_kernel(const float *__restrict__ a, unsigned *__restrict__ pmax, float *__restrict__ psum,
                          unsigned *__restrict__ pcmax, long long M, int C, int rows_per)
{
    __shared__ f32x4 s_sum[256];
    __shared__ u32x4 s_cmax[256];
    __shared__ unsigned s_max[256];
    const int C4 = C >> 2;
    const int TC = C4 < 256 ? C4 : 256, G = 256 / TC;
    const int tid = threadIdx.x, g = tid / TC, c = tid - g * TC;
    const long long r0 = (long long)blockIdx.x * rows_per, r1 = r0 + rows_per < M ? r0 + rows_per : M;
    unsigned amax = 0u;
    for (int cb = 0; cb < C4; cb += TC) {   // (uniform)
        const int c4 = cb + c;
        f32x4 sum = {0.f, 0.f, 0.f, 0.f};
        u32x4 cmax = {0u, 0u, 0u, 0u};
        if (g < G && c4 < C4) {
            const f32x4 *p = reinterpret_cast<const f32x4 *>(a) + c4;
#pragma unroll 4
            for (long long r = r0 + g; r < r1; r += G) {
                const f32x4 v = p[r * C4];
                sum += v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float f = v[e];   // (a copy: bit_cast of the vector element itself reads element 0)
                    const unsigned b = __builtin_bit_cast(unsigned, f) & 0x7fffffffu;
                    cmax[e] = b > cmax[e] ? b : cmax[e];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) amax = cmax[e] > amax ? cmax[e] : amax;
        }
        if (pcmax != nullptr) {   // (uniform)
            s_cmax[tid] = cmax;
            __syncthreads();
            if (g == 0 && c4 < C4) {
                u32x4 t = s_cmax[c];
                for (int gg = 1; gg < G; ++gg) {
                    const u32x4 o = s_cmax[gg * TC + c];
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] = o[e] > t[e] ? o[e] : t[e];
                }
                reinterpret_cast<u32x4 *>(pcmax + (size_t)blockIdx.x * C)[c4] = t;
            }
            __syncthreads();
        }
        if (psum != nullptr) {   // (uniform)
            s_sum[tid] = sum;
            __syncthreads();
            if (g == 0 && c4 < C4) {
                f32x4 t = s_sum[c];
                for (int gg = 1; gg < G; ++gg) t += s_sum[gg * TC + c];
                reinterpret_cast<f32x4 *>(psum + (size_t)blockIdx.x * C)[c4] = t;
            }
            __syncthreads();
        }
    }
    s_max[tid] = amax;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (tid < d) s_max[tid] = s_max[tid + d] > s_max[tid] ? s_max[tid + d] : s_max[tid];
        __syncthreads();
    }
    if (tid == 0) pmax[blockIdx.x] = s_max[0];
}

// the power of two that puts a matrix's largest magnitude (as a bit pattern) at the role's exponent: [2^14, 2^15) for the operand that
// is split as an ACTIVATION (2^-4 follows in split4: the hi piece stays below 2^11), [2^13, 2^14) for the one split as a WEIGHT (what
// weight_scale_for() does per channel).  It depends on the exponent alone: a 2^k a  ->  2^-k s, exactly.  1 for an all-zero or a
// non-finite matrix; capped as weight_scale_for() (s and 1 / s both normal).
__device__ __forceinline__ float grad_scale_for(unsigned amax_bits, int role)
{
    const float amax = __builtin_bit_cast(float, amax_bits);
    if (!(amax > 0.f) || !(amax < 3.0e38f)) return 1.f;
    const int e = (int)((amax_bits >> 23) & 0xffu) - 127;
    int s = (role == kStatsRole_Activation ? 14 : 13) - e;
    s = s < -100 ? -100 : (s > 126 ? 126 : s);
    return __builtin_bit_cast(float, (unsigned)(s + 127) << 23);
}

// stage 2: blocks 0 .. gridDim.x - 2: one thread per float4 of colsum / per 4 columns' scales (weight role: scale2 = t[C] | 1 / t[C]);
// the last block: the matrix's one scale (activation role: scale2 = {s, 1 / s})
__global__ void __launch_bounds__(256)
grad_stats_final_kernel(const unsigned *__restrict__ pmax, const float *__restrict__ psum, const unsigned *__restrict__ pcmax,
                        float *__restrict__ scale2, float *__restrict__ colsum, int C, int nblocks, int role, int f16)
{
    __shared__ unsigned s_max[256];
    const int tid = threadIdx.x;
    if (blockIdx.x + 1 == gridDim.x) {
        if (role != kStatsRole_Activation) return;   // (uniform)
        unsigned amax = 0u;
        for (int b = tid; b < nblocks; b += 256) amax = pmax[b] > amax ? pmax[b] : amax;
        s_max[tid] = amax;
        __syncthreads();
        for (int d = 128; d >= 1; d >>= 1) {
            if (tid < d) s_max[tid] = s_max[tid + d] > s_max[tid] ? s_max[tid + d] : s_max[tid];
            __syncthreads();
        }
        if (tid == 0) {
            const float s = f16 ? grad_scale_for(s_max[0], role) : 1.f;
            scale2[0] = s;
            scale2[1] = 1.f / s;   // a power of two between 2^-126 and 2^100: exact
        }
        return;
    }
    const int c4 = blockIdx.x * 256 + tid;
    if (c4 >= (C >> 2)) return;
    if (colsum != nullptr) {
        const f32x4 *p = reinterpret_cast<const f32x4 *>(psum) + c4;
        f32x4 acc = p[0];
        for (int b = 1; b < nblocks; ++b) acc += p[(size_t)b * (C >> 2)];
        reinterpret_cast<f32x4 *>(colsum)[c4] = acc;
    }
    if (pcmax != nullptr) {
        const u32x4 *p = reinterpret_cast<const u32x4 *>(pcmax) + c4;
        u32x4 m = p[0];
        for (int b = 1; b < nblocks; ++b) {
            const u32x4 o = p[(size_t)b * (C >> 2)];
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = o[e] > m[e] ? o[e] : m[e];
        }
        f32x4 t, r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned bits = m[e];
            t[e] = f16 ? grad_scale_for(bits, kStatsRole_Weight) : 1.f;
            r[e] = 1.f / t[e];   // a power of two between 2^-126 and 2^100: exact
        }
        reinterpret_cast<f32x4 *>(scale2)[c4] = t;
        reinterpret_cast<f32x4 *>(scale2 + C)[c4] = r;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// THE WEIGHT GRADIENT  dw[n, k] = sum_m dy[m, n] x[m, k]:  a GEMM whose contraction runs over the ROWS of both operands.
//   block   256 threads = 2 x 2 waves, 128 (n) x 128 (k) outputs, a wave owns 2 x 2 MFMA tiles of 32 x 32; the A operand of the MFMA is
//           dy^T (rows of the accumulator = n, split as the ACTIVATION), the B operand x^T (columns = k, split as the WEIGHT)
//   staging both MFMA operands want 8 consecutive m per lane.  A thread loads 8 consecutive ROWS of one column (dwords, coalesced across
//           the lanes), multiplies by the operand's scale, cuts them into pieces and writes one 16-byte LDS store per piece: the
//           transposition happens while staging.  LDS: [piece][column][32 m + 8 pad] 16-bit, single buffered; the loads of slice s + 1
//           are in flight (registers) during the MFMAs of slice s.  Rows >= M, columns >= N / K: exact zeros.
//   M split blockIdx.y walks `spc` slices of 32 rows and writes its partial sum to out + y N K (the caller's workspace); a second launch
//           (stream_splitk_reduce_kernel) adds the partials in the order 0, 1, ...  One chunk: straight to dw.
//   epilogue  fp16 scheme: acc . (4 / s) . (4 / t_k) = acc . 16 / (s t_k), two exact steps (s t_k itself may leave fp32's range)
// Summation order per output: m ascending, per 16 rows smallest term first; then the chunks in order.
constexpr int kWgTile = 128, kWgSlice = 32, kWgStride = kWgSlice + 8;

// The x operand is reached through a ROW MAP (the tile, the staging, the MFMAs and the epilogue are shared with the weight gradient of
// the 3 x 3 convolution, conv_bwd.h, whose x[m, k] is a shifted input pixel): init(k, ok) takes the thread's column once, load8(m0, M,
// dst) fetches rows m0 .. m0 + 7 of it (exact zeros where there is no such element), scale(k) / inv_scale(k) are t_k and 1 / t_k.
struct WgradRowsLinear {   // x[M, K] row-major
    const float *x, *x_scale2;
    int K;
    const float *bp;
    bool bok;
    __device__ __forceinline__ void init(int k, bool ok)
    {
        bok = ok;
        bp = x + (ok ? k : 0);
    }
    __device__ __forceinline__ void load8(int m0, int M, float (&dst)[8]) const
    {
#pragma unroll
        for (int r = 0; r < 8; ++r) dst[r] = (m0 + r < M && bok) ? bp[(size_t)(m0 + r) * K] : 0.f;
    }
    __device__ __forceinline__ float scale(int k) const { return x_scale2[k]; }
    __device__ __forceinline__ float inv_scale(int k) const { return x_scale2[K + k]; }
};

template <int SP, class XROWS>
__device__ __forceinline__ void wgrad_tile(const float *__restrict__ dy, const float *__restrict__ dy_scale2, float *__restrict__ out,
                                           int M, int N, int K, int ktiles, int spc, XROWS xrows)
{
    constexpr int NA = Split<SP>::NA, NB = Split<SP>::NB;
    __shared__ __attribute__((aligned(16))) unsigned short sA[NA][kWgTile * kWgStride];   // dy^T pieces: [n][m]
    __shared__ __attribute__((aligned(16))) unsigned short sB[NB][kWgTile * kWgStride];   // x^T pieces:  [k][m]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int nt = blockIdx.x / ktiles, kt = blockIdx.x - nt * ktiles;
    const int n0 = nt * kWgTile, k0 = kt * kWgTile;
    const int nslices = (M + kWgSlice - 1) / kWgSlice;
    const int sbeg = (int)blockIdx.y * spc, send = sbeg + spc < nslices ? sbeg + spc : nslices;
    out += (size_t)blockIdx.y * N * K;
    float sa = 1.f, fa = 1.f;
    if constexpr (Split<SP>::F16) {
        sa = dy_scale2[0];
        fa = 4.f * dy_scale2[1];
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // ---- staging: thread -> column c of the tile, row groups g0 and g0 + 1 (8 rows each) of the slice
    const int c = tid & 127, g0 = (tid >> 7) * 2;
    const bool aok = n0 + c < N, bok = k0 + c < K;
    const float *ap = dy + (aok ? n0 + c : 0);
    xrows.init(k0 + c, bok);
    float sb = 1.f;   // the scale of this thread's column of x
    if constexpr (Split<SP>::F16) sb = bok ? xrows.scale(k0 + c) : 1.f;
    float ra[2][8], rb[2][8];
    auto load = [&](int s) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m0 = s * kWgSlice + (g0 + h) * 8;
#pragma unroll
            for (int r = 0; r < 8; ++r) ra[h][r] = (m0 + r < M && aok) ? ap[(size_t)(m0 + r) * N] : 0.f;
            xrows.load8(m0, M, rb[h]);
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int o = c * kWgStride + (g0 + h) * 8;
            const f32x4 a0 = f32x4{ra[h][0], ra[h][1], ra[h][2], ra[h][3]} * sa, a1 = f32x4{ra[h][4], ra[h][5], ra[h][6], ra[h][7]} * sa;
            const f32x4 b0 = f32x4{rb[h][0], rb[h][1], rb[h][2], rb[h][3]} * sb, b1 = f32x4{rb[h][4], rb[h][5], rb[h][6], rb[h][7]} * sb;
            u32x2 pa0[NA], pa1[NA], pb0[NB], pb1[NB];
            split4<SP>(a0, pa0);
            split4<SP>(a1, pa1);
            split4_weight<SP>(b0, pb0);
            split4_weight<SP>(b1, pb1);
#pragma unroll
            for (int p = 0; p < NA; ++p) *reinterpret_cast<u32x4 *>(&sA[p][o]) = u32x4{pa0[p].x, pa0[p].y, pa1[p].x, pa1[p].y};
#pragma unroll
            for (int p = 0; p < NB; ++p) *reinterpret_cast<u32x4 *>(&sB[p][o]) = u32x4{pb0[p].x, pb0[p].y, pb1[p].x, pb1[p].y};
        }
    };

    if (sbeg < send) load(sbeg);
    for (int s = sbeg; s < send; ++s) {   // (block-uniform bounds)
        store();
        __syncthreads();
        if (s + 1 < send) load(s + 1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int koff = kk * 16 + (lane >> 5) * 8;
            u32x4 af[2][NA], bfr[2][NB];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int o = ((wr * 2 + i) * 32 + (lane & 31)) * kWgStride + koff;
#pragma unroll
                for (int p = 0; p < NA; ++p) af[i][p] = *reinterpret_cast<const u32x4 *>(&sA[p][o]);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int o = ((wc * 2 + j) * 32 + (lane & 31)) * kWgStride + koff;
#pragma unroll
                for (int p = 0; p < NB; ++p) bfr[j][p] = *reinterpret_cast<const u32x4 *>(&sB[p][o]);
            }
            mfma_tiles<SP, 2, 2>(acc, af, bfr);
        }
        __syncthreads();
    }

    // ---- epilogue: C/D of the 32 x 32 MFMA: col = lane & 31 (k), row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) (n)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int k = k0 + (wc * 2 + j) * 32 + (lane & 31);
        const bool kok = k < K;
        float fb = 1.f;
        if constexpr (Split<SP>::F16) fb = kok ? 4.f * xrows.inv_scale(k) : 1.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int nrow0 = n0 + (wr * 2 + i) * 32 + 4 * (lane >> 5);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int n = nrow0 + (e & 3) + 8 * (e >> 2);
                float v = acc[i][j][e];
                if constexpr (Split<SP>::F16) v = v * fa * fb;
                if (kok && n < N) out[(size_t)n * K + k] = v;
            }
        }
    }
}

template <int SP>
__global__ void __launch_bounds__(256)
wgrad_kernel(const float *__restrict__ dy, const float *__restrict__ x, const float *__restrict__ dy_scale2,
             const float *__restrict__ x_scale2, float *__restrict__ out, int M, int N, int K, int ktiles, int spc)
{
    wgrad_tile<SP>(dy, dy_scale2, out, M, N, K, ktiles, spc, WgradRowsLinear{x, x_scale2, K, nullptr, false});
}

struct WgradPlan {
    int msplit, spc;   // chunks of the row loop, slices of 32 rows per chunk
};

// chunks of the row loop: a function of (M, K, N) [and the forced value] only.  The output has (N / 128) (K / 128) tiles; about 512
// workgroups fill the chip twice, a chunk walks at least 4 slices, at most 64 partials go through the second pass.
inline WgradPlan wgrad_plan(long long M, int K, int N)
{
    const int nslices = (int)((M + kWgSlice - 1) / kWgSlice);
    const int tiles = ((N + kWgTile - 1) / kWgTile) * ((K + kWgTile - 1) / kWgTile);
    int ms = tfm::dense_knob(tfm::kKnobWgradMsplit);   // 0: per shape
    if (ms <= 0) {
        ms = 512 / tiles;
        if (ms > nslices / 4) ms = nslices / 4;
    }
    ms = ms < 1 ? 1 : (ms > 64 ? 64 : ms);
    if (ms > nslices) ms = nslices;
    const int spc = (nslices + ms - 1) / ms;
    return WgradPlan{(nslices + spc - 1) / spc, spc};
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int64_t tf_linear_grad_stats_workspace_bytes(int64_t M, int C, int role, int with_colsum)
{
    if (M <= 0 || C <= 0 || (C & 3) || M > 0x7fffffffLL || (role != kStatsRole_Activation && role != kStatsRole_Weight)) return -1;
    const int64_t nb = stats_blocks(M);
    return ((nb * 4 + 15) & ~(int64_t)15) + (with_colsum ? nb * C * 4 : 0) + (role == kStatsRole_Weight ? nb * C * 4 : 0);
}

extern "C" int tf_linear_grad_stats_f32(const float *a, float *scale2, float *colsum, void *workspace, int64_t workspace_bytes,
                                        int64_t M, int C, int role, int terms, void *stream)
{
    if (!a || !scale2 || !workspace) return TF_MSDA_ERR_NULL_POINTER;
    const int sp = split_scheme(terms);
    if (M <= 0 || C <= 0 || (C & 3) || M > 0x7fffffffLL || sp == 0 || (role != kStatsRole_Activation && role != kStatsRole_Weight))
        return TF_MSDA_ERR_BAD_DIMS;
    if (!aligned16(a) || (colsum && !aligned16(colsum))) return TF_MSDA_ERR_BAD_DIMS;
    if (!aligned16(scale2)) return TF_MSDA_ERR_BAD_DIMS;
    if (workspace_bytes < tf_linear_grad_stats_workspace_bytes(M, C, role, colsum != nullptr) || !aligned16(workspace)) return TF_MSDA_ERR_WORKSPACE;
    const int nb = stats_blocks(M);
    char *w = static_cast<char *>(workspace);
    unsigned *pmax = reinterpret_cast<unsigned *>(w);
    w += ((size_t)nb * 4 + 15) & ~(size_t)15;
    float *psum = colsum ? reinterpret_cast<float *>(w) : nullptr;
    if (colsum) w += (size_t)nb * C * 4;
    unsigned *pcmax = role == kStatsRole_Weight ? reinterpret_cast<unsigned *>(w) : nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(grad_stats_partial_kernel, dim3((unsigned)nb), dim3(256), 0, s, a, pmax, psum, pcmax, (long long)M, C, stats_rows_per(M));
    if (int rc = tfm::launched()) return rc;
    const int cblocks = (colsum || pcmax) ? ((C >> 2) + 255) / 256 : 0;
    hipLaunchKernelGGL(grad_stats_final_kernel, dim3((unsigned)(cblocks + 1)), dim3(256), 0, s, (const unsigned *)pmax, (const float *)psum,
                       (const unsigned *)pcmax, scale2, colsum, C, nb, role, sp == 16 ? 1 : 0);
    return tfm::launched();
}

extern "C" int64_t tf_linear_wgrad_workspace_bytes(int64_t M, int K, int N)
{
    if (M <= 0 || K <= 0 || N <= 0 || (K & 3) || (N & 3) || M > 0x7fffffffLL) return -1;
    const WgradPlan p = wgrad_plan(M, K, N);
    return p.msplit > 1 ? (int64_t)p.msplit * N * K * 4 : 0;
}

extern "C" int tf_linear_wgrad_split_f32(const float *dy, const float *x, const float *dy_scale2, const float *x_scale2, float *dw,
                                         void *workspace, int64_t workspace_bytes, int64_t M, int K, int N, int terms, void *stream)
{
    if (!dy || !x || !dy_scale2 || !x_scale2 || !dw) return TF_MSDA_ERR_NULL_POINTER;
    const int sp = split_scheme(terms);
    if (M <= 0 || K <= 0 || N <= 0 || (K & 3) || (N & 3) || M > 0x7fffffffLL || sp == 0) return TF_MSDA_ERR_BAD_DIMS;
    if ((long long)M * N * 4 >= 0xC0000000LL || (long long)M * K * 4 >= 0xC0000000LL || (long long)N * K * 4 >= 0xC0000000LL)
        return TF_MSDA_ERR_BAD_DIMS;
    if (!aligned16(dy) || !aligned16(x) || !aligned16(dw) || !aligned16(x_scale2)) return TF_MSDA_ERR_BAD_DIMS;
    const WgradPlan p = wgrad_plan(M, K, N);
    const int64_t need = p.msplit > 1 ? (int64_t)p.msplit * N * K * 4 : 0;
    if (need > 0 && (!workspace || workspace_bytes < need || !aligned16(workspace))) return TF_MSDA_ERR_WORKSPACE;
    const int ntiles = (N + kWgTile - 1) / kWgTile, ktiles = (K + kWgTile - 1) / kWgTile;
    if ((long long)ntiles * ktiles > 0x7fffffffLL) return TF_MSDA_ERR_BAD_DIMS;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *out = p.msplit > 1 ? static_cast<float *>(workspace) : dw;
    const dim3 grid((unsigned)(ntiles * ktiles), (unsigned)p.msplit);
    if (sp == 3)
        hipLaunchKernelGGL(wgrad_kernel<3>, grid, dim3(256), 0, s, dy, x, dy_scale2, x_scale2, out, (int)M, N, K, ktiles, p.spc);
    else
        hipLaunchKernelGGL(wgrad_kernel<16>, grid, dim3(256), 0, s, dy, x, dy_scale2, x_scale2, out, (int)M, N, K, ktiles, p.spc);
    if (int rc = tfm::launched()) return rc;
    return p.msplit > 1 ? launch_splitk_reduce(out, nullptr, nullptr, dw, (long long)N * K, K, p.msplit, 0, s) : TF_MSDA_OK;
}

// dx = dy . w through the stream GEMM: the block shapes of stream_dispatch by the output width alone (every shape gives the same bits:
// the order of the sum along the contraction does not depend on the block)
template <int SP>
static int dgrad_dispatch(const StreamCall &c, hipStream_t s, bool scaled)
{
    if (c.N <= 64) return scaled ? launch_stream<SP, 2, 1, 2, false, true>(c, s) : launch_stream<SP, 2, 1, 2, false>(c, s);
    if (c.N <= 128) return scaled ? launch_stream<SP, 4, 1, 4, false, true>(c, s) : launch_stream<SP, 4, 1, 4, false>(c, s);
    return scaled ? launch_stream<SP, 3, 2, 4, false, true>(c, s) : launch_stream<SP, 3, 2, 4, false>(c, s);
}

extern "C" int tf_linear_dgrad_packed_f32(const float *dy, const float *dy_scale2, const void *wt_packed, float *dx, int64_t M, int K,
                                          int N, int terms, void *stream)
{
    if (!dy || !wt_packed || !dx) return TF_MSDA_ERR_NULL_POINTER;
    const int sp = split_scheme(terms);
    // (the contraction runs over N: pairs of 32-deep slices)
    if (M <= 0 || K <= 0 || N <= 0 || (N % 64) != 0 || M > 0x7fffffffLL || sp == 0) return TF_MSDA_ERR_BAD_DIMS;
    if (!aligned16(dy) || !aligned16(wt_packed)) return TF_MSDA_ERR_BAD_DIMS;
    if ((long long)(M + 256) * K * 4 >= 0xC0000000LL) return TF_MSDA_ERR_BAD_DIMS;
    // (`bias` carries scale2: the XSC form of stream_gemm_kernel)
    StreamCall c{dy, static_cast<const u32x4 *>(wt_packed), dy_scale2, nullptr, dx, (int)M, N, K, 0, false, StreamConv{}, nullptr, 1};
    const bool scaled = dy_scale2 != nullptr;
    return sp == 3 ? dgrad_dispatch<3>(c, static_cast<hipStream_t>(stream), scaled) : dgrad_dispatch<16>(c, static_cast<hipStream_t>(stream), scaled);
}

// the same product with the contraction over N cut into `ksplit` pieces (the stream GEMM's split-K: partial sums to `workspace`, each
// multiplied by 1 / s, a second launch adds them in the order 0, 1, ...): no accumulator walks the whole sum.  ksplit = 1: the bits of
// tf_linear_dgrad_packed_f32
extern "C" int tf_linear_dgrad_splitk_packed_f32(const float *dy, const float *dy_scale2, const void *wt_packed, float *dx, float *workspace,
                                                 int ksplit, int64_t M, int K, int N, int terms, void *stream)
{
    if (!dy || !wt_packed || !dx) return TF_MSDA_ERR_NULL_POINTER;
    if (ksplit > 1 && !workspace) return TF_MSDA_ERR_NULL_POINTER;
    const int sp = split_scheme(terms);
    if (M <= 0 || K <= 0 || N <= 0 || (N % 64) != 0 || M > 0x7fffffffLL || sp == 0 || ksplit < 1 || ksplit > 64) return TF_MSDA_ERR_BAD_DIMS;
    if (!aligned16(dy) || !aligned16(wt_packed)) return TF_MSDA_ERR_BAD_DIMS;
    if (ksplit > 1 && ((K & 3) || !aligned16(dx) || !aligned16(workspace))) return TF_MSDA_ERR_BAD_DIMS;   // (the second pass moves float4)
    if ((long long)(M + 256) * K * 4 >= 0xC0000000LL) return TF_MSDA_ERR_BAD_DIMS;
    StreamCall c{dy, static_cast<const u32x4 *>(wt_packed), dy_scale2, nullptr, dx, (int)M, N, K, 0, false, StreamConv{}, workspace, ksplit};
    const bool scaled = dy_scale2 != nullptr;
    return sp == 3 ? dgrad_dispatch<3>(c, static_cast<hipStream_t>(stream), scaled) : dgrad_dispatch<16>(c, static_cast<hipStream_t>(stream), scaled);
}

#endif /* TF_LINEAR_BWD_H_ */
