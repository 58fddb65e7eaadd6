// trackformer_amd/csrc/mask_loss.h -- the mask losses of the matched pairs: sigmoid focal + dice over the bilinearly upsampled pred_masks
// (included from fused_ops.hip behind criterion.h; include/tf_fused.h: THE MASK LOSSES; reference: SetCriterion.loss_masks).
//
//   mask_loss_fwd_kernel      one workgroup per (pair, tile of kMaskTileRows output rows): interpolates on the fly, reads the targets as
//                             bytes, four fp64 partial sums per tile into the workspace
//   mask_loss_finish_kernel   one workgroup: adds the tiles of every pair in index order -> sums [n, 4], then the two losses
//   mask_loss_bwd_kernel      one work-item per element of pred_masks: the gather form of the interpolation's transpose, zeros in the rows
//                             of unmatched queries
//
// No full-resolution fp32 tensor exists in either direction: the upsampled logits live in registers, the targets stay uint8 and are
// indexed through pair_tgt, never gathered.
// THE COORDINATES are integers.  Output row Y reads source rows y0 and y1 = y0 + (y0 < h - 1) with weights 1 - l and l, where
//     num = max((2 Y + 1) h - H, 0)        y0 = num / (2 H)        l = (num % (2 H)) / (2 H), one rounding
// (F.interpolate(mode="bilinear", align_corners=False) with a size; exact where ATen's fp32 scale (Y + 0.5) - 0.5 is not), and the
// same in x.  The backward inverts the same formula: y0(Y) >= a  <=>  Y >= ceil(((2 a + 1) H - h) / (2 h)) for a >= 1.
// THE TILE RULE is a function of the shape alone: kMaskTileRows = 8 output rows per tile, tiles = ceil(H / 8); inside a tile the
// workgroup walks the row in chunks of 256 columns, thread t owning column 256 c + t of every chunk.  The source rows and columns a
// chunk needs (at most 10 x 258, because H >= h and W >= w) go through LDS.
// THE SUMS (focal, p t, p, t) are accumulated in fp64: a thread adds its elements in (chunk, row) order, a butterfly over the wave, the
// four waves in wave order through LDS, the tiles in index order in the second launch, the pairs in index order for the two losses;
// each loss is rounded once.  No atomics; every output element is written exactly once.
// THE BACKWARD RECOMPUTES g_x PER CORNER instead of staging a strip of g_x in LDS: a source pixel's gradient is the sum of
// wy wx g_x over the output pixels that have it as one of their four corners -- a contiguous range of rows and of columns, walked as
// four quadrants (which of y0 / y1 and x0 / x1 the pixel is) in the fixed order (y0 - 1, x0 - 1), (y0 - 1, x0), (y0, x0 - 1), (y0, x0),
// rows then columns ascending inside each, accumulated in fp64 and rounded once.  Every g_x is therefore evaluated four times.  The
// staged form would evaluate it once (plus the rows two strips share), but a strip of g_x at 800 x 1333 is 5 KB per output row: the
// strip would have to be cut in x as well, with halo columns and two more barriers per piece, and the order of the sum would then
// depend on the cut.  The recomputation keeps one work-item per output element of the gradient, no LDS and no barrier, and its order
// is the one above for every shape; what it costs is arithmetic (three transcendental calls per evaluation) in a kernel whose
// alternative is a dozen full-resolution passes.
#ifndef TF_MASK_LOSS_H_
#define TF_MASK_LOSS_H_

#include "host_dispatch.h"
#include "launch_status.h"

namespace {

constexpr int kMaskTileRows = 8;                   // output rows per forward tile
constexpr int kMaskChunk = 256;                    // output columns per chunk = threads per workgroup
constexpr int kMaskSrcRows = kMaskTileRows + 2;    // source rows a tile can touch (H >= h): at most kMaskTileRows + 1
constexpr int kMaskSrcCols = kMaskChunk + 2;       // source columns a chunk can touch (W >= w): at most kMaskChunk + 1

struct Lerp {
    int i0, i1;   // the two source indices
    float l;      // the weight of i1; 1 - l that of i0
};

// Output index O of an axis of `out` elements over `in` source elements.
__device__ __forceinline__ Lerp mask_lerp(int O, int in, int out)
{
    const int num = (2 * O + 1) * in - out;
    const int den = 2 * out;
    Lerp r;
    r.i0 = num > 0 ? num / den : 0;
    const int rem = num > 0 ? num - r.i0 * den : 0;
    r.l = (float)rem / (float)den;   // both below 2^24: exact operands, one rounding
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    return r;
}

// The first output index whose i0 is >= a (a >= 1; 0 for a <= 0), clamped to `out`.
__device__ __forceinline__ int mask_first_out(int a, int in, int out)
{
    if (a <= 0) return 0;
    const int v = ((2 * a + 1) * out - in + 2 * in - 1) / (2 * in);
    return v < out ? v : out;
}

__device__ __forceinline__ float mask_bilerp(float v00, float v01, float v10, float v11, float ly, float lx)
{
    return (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
}

// blockIdx.x = pair * tiles + tile.  A pair whose pair_src / pair_tgt lies outside [0, BQ) / [0, T) contributes zeros: nothing is
// read for it.
__global__ void __launch_bounds__(kMaskChunk)
mask_loss_fwd_kernel(const float *__restrict__ src, const unsigned char *__restrict__ tgt, const int *__restrict__ pair_src,
                     const int *__restrict__ pair_tgt, double *__restrict__ partial, int tiles, int BQ, int T, int h, int w, int H, int W,
                     float alpha, float gamma)
{
    __shared__ float s_src[kMaskSrcRows][kMaskSrcCols];
    __shared__ double s_sum[kMaskChunk / 64][4];
    __shared__ Lerp s_row[kMaskTileRows];   // the tile's rows, relative to its first source row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pair = blockIdx.x / tiles, tile = blockIdx.x - pair * tiles;
    const int ps = pair_src[pair], pt = pair_tgt[pair];
    const bool valid = ps >= 0 && ps < BQ && pt >= 0 && pt < T;   // (uniform)
    double a_focal = 0.0, a_pt = 0.0, a_p = 0.0;
    int a_t = 0;
    if (valid) {
        const int Y0 = tile * kMaskTileRows;
        const int Y1 = Y0 + kMaskTileRows < H ? Y0 + kMaskTileRows : H;
        const int ylo = mask_lerp(Y0, h, H).i0;
        int nrows = mask_lerp(Y1 - 1, h, H).i1 - ylo + 1;
        nrows = nrows < kMaskSrcRows ? nrows : kMaskSrcRows;
        if (threadIdx.x < Y1 - Y0) {
            Lerp ly = mask_lerp(Y0 + threadIdx.x, h, H);
            ly.i0 -= ylo;
            ly.i1 -= ylo;
            s_row[threadIdx.x] = ly;   // (read behind the first chunk's barriers)
        }
        const float *srow = src + (size_t)ps * h * w;
        const unsigned char *trow = tgt + (size_t)pt * H * W;
        for (int X0 = 0; X0 < W; X0 += kMaskChunk) {   // (uniform)
            const int Xl = X0 + kMaskChunk < W ? X0 + kMaskChunk : W;
            const int xlo = mask_lerp(X0, w, W).i0;
            int ncols = mask_lerp(Xl - 1, w, W).i1 - xlo + 1;
            ncols = ncols < kMaskSrcCols ? ncols : kMaskSrcCols;
            __syncthreads();   // the previous chunk has been read
            for (int r = 0; r < nrows; ++r)
                for (int c = threadIdx.x; c < ncols; c += kMaskChunk) s_src[r][c] = srow[(size_t)(ylo + r) * w + xlo + c];
            __syncthreads();
            const int X = X0 + threadIdx.x;
            if (X < W) {
                const Lerp lx = mask_lerp(X, w, W);
                const int c0 = lx.i0 - xlo, c1 = lx.i1 - xlo;
                if (c1 < kMaskSrcCols) {   // (always: the bound of the header comment; never index LDS on trust)
                    for (int Y = Y0; Y < Y1; ++Y) {
                        const Lerp ly = s_row[Y - Y0];
                        const int r0 = ly.i0, r1 = ly.i1;
                        if (r1 >= kMaskSrcRows) continue;   // (never)
                        const float x = mask_bilerp(s_src[r0][c0], s_src[r0][c1], s_src[r1][c0], s_src[r1][c1], ly.l, lx.l);
                        const bool pos = trow[(size_t)Y * W + X] != 0;
                        const float e = expf(-fabsf(x));   // the exp of focal_term: one evaluation after inlining
                        const float inv = 1.f / (1.f + e);
                        const float p = x >= 0.f ? inv : e * inv;
                        a_focal += (double)focal_term<false>(x, pos, alpha, gamma).loss;
                        a_p += (double)p;
                        if (pos) {
                            a_pt += (double)p;
                            a_t += 1;
                        }
                    }
                }
            }
        }
    }
    a_focal = wave_sum_f64(a_focal);
    a_pt = wave_sum_f64(a_pt);
    a_p = wave_sum_f64(a_p);
    a_t = wave_sum_i32(a_t);
    if (lane == 0) {
        s_sum[wave][0] = a_focal;
        s_sum[wave][1] = a_pt;
        s_sum[wave][2] = a_p;
        s_sum[wave][3] = (double)a_t;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        partial[(size_t)blockIdx.x * 4 + k] = ((s_sum[0][k] + s_sum[1][k]) + s_sum[2][k]) + s_sum[3][k];
    }
}

// One workgroup.  sums[i] = (sum focal, sum p t, sum p, sum t) of pair i: its tiles added in index order.  Then thread 0 adds the
// pairs' focal means and thread 1 their dice terms, in index order; n == 0: both losses are 0.
__global__ void __launch_bounds__(256)
mask_loss_finish_kernel(const double *__restrict__ partial, double *sums, float *__restrict__ losses, int n, int tiles, int H, int W,
                        float num_boxes)
{
    for (int j = threadIdx.x; j < n * 4; j += 256) {
        const int i = j >> 2, k = j & 3;
        double s = 0.0;
        for (int t = 0; t < tiles; ++t) s += partial[((size_t)i * tiles + t) * 4 + k];
        sums[j] = s;
    }
    __syncthreads();   // (the workgroup's own global writes are visible to it behind the barrier)
    if (threadIdx.x < 2) {
        const double hw = (double)H * (double)W;
        double acc = 0.0;
        for (int i = 0; i < n; ++i) {
            const volatile double *s = sums + (size_t)i * 4;
            acc += threadIdx.x == 0 ? s[0] / hw : 1.0 - (2.0 * s[1] + 1.0) / ((s[2] + s[3]) + 1.0);
        }
        losses[threadIdx.x] = (float)(acc / (double)num_boxes);
    }
}

// blockIdx.x = row * blocks_per_row + block of 256 elements of the row.  row_pair[row]: the pair of that row of pred_masks, or -1
// (anything outside [0, n), or a pair whose pair_tgt lies outside [0, T), counts as -1: zeros, nothing read).
__global__ void __launch_bounds__(256)
mask_loss_bwd_kernel(const float *__restrict__ G, const float *__restrict__ src, const unsigned char *__restrict__ tgt,
                     const int *__restrict__ pair_tgt, const int *__restrict__ row_pair, const double *__restrict__ sums,
                     float *__restrict__ grad_src, int blocks_per_row, int n, int T, int h, int w, int H, int W, float alpha, float gamma,
                     float num_boxes)
{
    const int row = blockIdx.x / blocks_per_row;
    const int e0 = (blockIdx.x - row * blocks_per_row) * 256 + threadIdx.x;
    if (e0 >= h * w) return;
    float *out = grad_src + (size_t)row * h * w + e0;
    const int i = row_pair[row];
    const int pt = i >= 0 && i < n ? pair_tgt[i] : -1;
    if (pt < 0 || pt >= T) {   // (uniform)
        *out = 0.f;
        return;
    }
    // the two coefficients of the pair: cm d focal / dx + cd[t] p (1 - p)
    const double num = 2.0 * sums[i * 4 + 1] + 1.0, den = (sums[i * 4 + 2] + sums[i * 4 + 3]) + 1.0;
    const double gd = (double)G[1] / (double)num_boxes;
    const float cm = (float)((double)G[0] / ((double)num_boxes * (double)H * (double)W));
    const float cd0 = (float)(gd * (num / (den * den)));                   // t = 0: -(0 - num) / den^2
    const float cd1 = (float)(gd * (-(2.0 * den - num) / (den * den)));    // t = 1
    const int y = e0 / w, x = e0 - y * w;
    const float *srow = src + (size_t)row * h * w;
    const unsigned char *trow = tgt + (size_t)pt * H * W;
    // the 3 x 3 neighbourhood, clamped: quadrant (dy, dx) interpolates between rows nb[dy], nb[dy + 1] and columns [dx], [dx + 1] (at
    // the bottom / right edge y1 == y0: the clamp makes nb[2] the same row as nb[1])
    float nb[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int yy = y + a - 1 < 0 ? 0 : (y + a - 1 > h - 1 ? h - 1 : y + a - 1);
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int xx = x + b - 1 < 0 ? 0 : (x + b - 1 > w - 1 ? w - 1 : x + b - 1);
            nb[a][b] = srow[(size_t)yy * w + xx];
        }
    }
    const int Yb[3] = {mask_first_out(y - 1, h, H), mask_first_out(y, h, H), mask_first_out(y + 1, h, H)};
    const int Xb[3] = {mask_first_out(x - 1, w, W), mask_first_out(x, w, W), mask_first_out(x + 1, w, W)};
    const float den_y = (float)(2 * H), den_x = (float)(2 * W);
    double acc = 0.0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int y0 = y - 1 + dy;          // the rows Y of this quadrant have y0(Y) == y0
        const bool both_y = dy == 1 && y == h - 1;   // y1 == y0 == this pixel: it takes both weights
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int x0 = x - 1 + dx;
            const bool both_x = dx == 1 && x == w - 1;
            for (int Y = Yb[dy]; Y < Yb[dy + 1]; ++Y) {
                const int ny = (2 * Y + 1) * h - H;
                const float ly = ny > 0 ? (float)(ny - y0 * 2 * H) / den_y : 0.f;
                const float wy = dy == 0 ? ly : 1.f - ly;   // this pixel is y1 (dy == 0) or y0
                for (int X = Xb[dx]; X < Xb[dx + 1]; ++X) {
                    const int nx = (2 * X + 1) * w - W;
                    const float lx = nx > 0 ? (float)(nx - x0 * 2 * W) / den_x : 0.f;
                    const float wx = dx == 0 ? lx : 1.f - lx;
                    const float v = mask_bilerp(nb[dy][dx], nb[dy][dx + 1], nb[dy + 1][dx], nb[dy + 1][dx + 1], ly, lx);
                    const bool pos = trow[(size_t)Y * W + X] != 0;
                    const float e = expf(-fabsf(v));
                    const float inv = 1.f / (1.f + e);
                    const float g = cm * focal_term<true>(v, pos, alpha, gamma).dx + (pos ? cd1 : cd0) * (inv * (e * inv));
                    acc += (double)((wy * wx) * g);
                    if (both_y) acc += (double)((ly * wx) * g);
                    if (both_x) acc += (double)((wy * lx) * g);
                    if (both_y && both_x) acc += (double)((ly * lx) * g);
                }
            }
        }
    }
    *out = (float)acc;
}

// The sizes all three entries take.  The coordinate arithmetic is int32 ((2 H + 1) (h + 1) and the same in x stay below 2^31) and a
// weight's numerator and denominator are exact in fp32 (H, W <= 2^23).
bool mask_loss_dims_ok(int64_t n, int64_t BQ, int64_t T, int64_t h, int64_t w, int64_t H, int64_t W)
{
    if (n < 0 || BQ <= 0 || T < 0 || h <= 0 || w <= 0 || H < h || W < w || H > (1 << 23) || W > (1 << 23)) return false;
    if ((2 * H + 1) * (h + 1) > 0x7fffffffLL || (2 * W + 1) * (w + 1) > 0x7fffffffLL) return false;
    if (h * w > 0x7fffffffLL || H * W > 0x7fffffffLL) return false;
    const int64_t tiles = (H + kMaskTileRows - 1) / kMaskTileRows, bpr = (h * w + 255) / 256;
    return n <= 0x7fffffffLL / 4 && n * tiles <= 0x7fffffffLL && BQ * bpr <= 0x7fffffffLL;
}

}  // namespace

extern "C" int64_t tf_mask_loss_workspace_bytes(int n, int H, int W)
{
    if (n < 0 || H <= 0 || W <= 0) return -1;
    const int64_t tiles = ((int64_t)H + kMaskTileRows - 1) / kMaskTileRows;
    if ((int64_t)n * tiles > 0x7fffffffLL) return -1;
    return (int64_t)n * tiles * 4 * (int64_t)sizeof(double);
}

extern "C" int tf_mask_loss_fwd_f32(const float *src, const uint8_t *tgt, const int *pair_src, const int *pair_tgt, double *sums,
                                    float *losses, void *workspace, int64_t workspace_bytes, int n, int BQ, int T, int h, int w, int H,
                                    int W, float alpha, float gamma, float num_boxes, void *stream)
{
    if (!losses || (n > 0 && (!src || !tgt || !pair_src || !pair_tgt || !sums))) return TF_MSDA_ERR_NULL_POINTER;
    if (!mask_loss_dims_ok(n, BQ, T, h, w, H, W) || !(num_boxes > 0.f)) return TF_MSDA_ERR_BAD_DIMS;
    if (!aligned4(losses) || (n > 0 && (!aligned4(src) || !aligned4(pair_src) || !aligned4(pair_tgt) || !aligned8(sums))))
        return TF_MSDA_ERR_BAD_DIMS;
    const int tiles = (H + kMaskTileRows - 1) / kMaskTileRows;
    if (n > 0 && (!workspace || workspace_bytes < tf_mask_loss_workspace_bytes(n, H, W) || !aligned8(workspace))) return TF_MSDA_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(workspace);
    if (n > 0) {
        const tfm::KernelVariant kv = {(const void *)&mask_loss_fwd_kernel, "mask_loss_fwd_f32"};
        void *argv[] = {(void *)&src, (void *)&tgt, (void *)&pair_src, (void *)&pair_tgt, (void *)&partial, (void *)&tiles, (void *)&BQ,
                        (void *)&T,   (void *)&h,   (void *)&w,        (void *)&H,        (void *)&W,       (void *)&alpha, (void *)&gamma};
        if (int rc = tfm::record_hip(hipLaunchKernel(kv.fn, dim3((unsigned)n * (unsigned)tiles), dim3(kMaskChunk), argv, 0, s))) return rc;
        tfm::note_kernel(kv.name);
    }
    const tfm::KernelVariant kv = {(const void *)&mask_loss_finish_kernel, "mask_loss_finish_f32"};
    const double *cpartial = partial;
    void *argv[] = {(void *)&cpartial, (void *)&sums, (void *)&losses, (void *)&n, (void *)&tiles, (void *)&H, (void *)&W, (void *)&num_boxes};
    if (int rc = tfm::record_hip(hipLaunchKernel(kv.fn, dim3(1), dim3(256), argv, 0, s))) return rc;
    tfm::note_kernel(kv.name);
    return TF_MSDA_OK;
}

extern "C" int tf_mask_loss_bwd_f32(const float *G, const float *src, const uint8_t *tgt, const int *pair_tgt, const int *row_pair,
                                    const double *sums, float *grad_src, int n, int BQ, int T, int h, int w, int H, int W, float alpha,
                                    float gamma, float num_boxes, void *stream)
{
    if (!row_pair || !grad_src || (n > 0 && (!G || !src || !tgt || !pair_tgt || !sums))) return TF_MSDA_ERR_NULL_POINTER;
    if (!mask_loss_dims_ok(n, BQ, T, h, w, H, W) || !(num_boxes > 0.f)) return TF_MSDA_ERR_BAD_DIMS;
    if (!aligned4(row_pair) || !aligned4(grad_src) || (n > 0 && (!aligned4(G) || !aligned4(src) || !aligned4(pair_tgt) || !aligned8(sums))))
        return TF_MSDA_ERR_BAD_DIMS;
    const int bpr = (h * w + 255) / 256;
    const tfm::KernelVariant kv = {(const void *)&mask_loss_bwd_kernel, "mask_loss_bwd_f32"};
    void *argv[] = {(void *)&G, (void *)&src, (void *)&tgt, (void *)&pair_tgt, (void *)&row_pair, (void *)&sums, (void *)&grad_src,
                    (void *)&bpr, (void *)&n, (void *)&T,   (void *)&h,        (void *)&w,        (void *)&H,    (void *)&W,
                    (void *)&alpha, (void *)&gamma, (void *)&num_boxes};
    if (int rc = tfm::record_hip(hipLaunchKernel(kv.fn, dim3((unsigned)BQ * (unsigned)bpr), dim3(256), argv, 0, static_cast<hipStream_t>(stream))))
        return rc;
    tfm::note_kernel(kv.name);
    return TF_MSDA_OK;
}

#endif /* TF_MASK_LOSS_H_ */
