// trackformer_amd/csrc/conv_strided_bwd.h -- the backward of the STRIDE-2 convolutions as split products (included behind conv_bwd.h at the
// end of linear_stream.hip; include/tf_fused.h: THE BACKWARD OF THE STRIDE-2 CONVOLUTIONS).  NHWC fp32 tensors; the 3 x 3 weight
// [cout, 3, 3, cin] tap-major (padding 1), the 1 x 1 weight [cout, cin] (no padding); dy [nimg, ho, wo, cout], ho = (h - 1) / 2 + 1.
//
//   dx      The input pixel (iy, ix) = (2 a + py, 2 b + px) only meets the taps of its parity: py = 0 the tap row ky = 1 (dy row a), py = 1
//           the rows ky = 2 (dy row a) and ky = 0 (dy row a + 1); columns alike.  So dx is FOUR stride-1 convolutions over dy, one per
//           parity class, with windows of 1 x 1, 1 x 2, 2 x 1 and 2 x 2 taps whose origin is the pixel (a, b) itself -- 9 cout products per
//           four input pixels, and a dy row / column ho / wo (the + 1 neighbour of the last odd pixel) is outside dy: an exact zero that
//           is never read.  Each class is ONE launch of the stream GEMM's convolution form as it is (stream_gemm_kernel<.., CONV>: its
//           window is `ks` columns wide and as many rows deep as the contraction K says -- (ks, K) = (1, cout), (2, 2 cout), (1, 2 cout),
//           (2, 4 cout) --, no padding, stride 1, the class extents as its output extents), in the scaled-activation instantiation, its
//           contraction cut into pieces by its own split-K; the launches leave COMPACT class images [pieces][class pixels][cin] in the
//           workspace.  conv_s2_dgrad_assemble_kernel (new) then writes every element of dx once: the pieces of its class added in
//           the order 0, 1, ..., at the pixel the class row maps to.  The 1 x 1 projection is the class (0, 0) alone; the pixels of the
//           other three classes get +0.  No zero-inserted dy, no atomics.
//   dw      (1 x 1, stride 2)  dw[co, ci] = sum_m dy[m, co] x[n, 2 ho, 2 wo, ci]: wgrad_tile of linear_bwd.h with the row address of
//           the x operand replaced (WgradRowsConv1: no taps, no padding -- every row exists), the same products in the same order as
//           tf_linear_wgrad_split_f32 on the gathered matrix, which is never built.
#ifndef TF_CONV_STRIDED_BWD_H_
#define TF_CONV_STRIDED_BWD_H_

namespace {

// ---- dx: the parity classes, c = 2 py + px
struct S2Class {
    long long off, cnt;   // floats: where the class image starts in the workspace, and the size of one piece of it (class pixels x cin)
    int pieces;           // partial sums the class image consists of; 0: nothing was computed (ks = 1: the pixels are exact zeros)
};
struct S2Classes {
    S2Class c00, c01, c10, c11;
    int h0, h1, w0, w1;   // class extents by parity: ceil((h - py) / 2), ceil((w - px) / 2)
};

// one thread per 4 consecutive channels of one input pixel: total4 = nimg h w cin / 4 < 2^28 (dx lies below 3 GiB), the pixel index
// in 32 bits; offsets into the workspace in 64 bits
__global__ void __launch_bounds__(256)
conv_s2_dgrad_assemble_kernel(const float *__restrict__ ws, float *__restrict__ dx, const S2Classes cl, unsigned total4, int h, int w, int c4)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total4) return;
    const unsigned pix = i / (unsigned)c4, q = i - pix * (unsigned)c4;
    const unsigned row = pix / (unsigned)w, ix = pix - row * (unsigned)w;
    const unsigned n = row / (unsigned)h, iy = row - n * (unsigned)h;
    const bool py = iy & 1u, px = ix & 1u;
    const S2Class c = py ? (px ? cl.c11 : cl.c10) : (px ? cl.c01 : cl.c00);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (c.pieces > 0) {
        const long long r = ((long long)n * (py ? cl.h1 : cl.h0) + (iy >> 1)) * (px ? cl.w1 : cl.w0) + (ix >> 1);
        const f32x4 *p = reinterpret_cast<const f32x4 *>(ws + c.off) + r * c4 + q;
        const long long step = c.cnt >> 2;
        acc = p[0];
        for (int z = 1; z < c.pieces; ++z) acc += p[z * step];   // the pieces in the order 0, 1, ...
    }
    tfm::stream_store(reinterpret_cast<f32x4 *>(dx) + i, acc);
}

struct S2Plan {
    int ncls;             // 4 (ks = 3) or 1 (ks = 1)
    int hc[2], wc[2];
    long long M[4];       // class pixels
    int taps[4], win[4];  // taps of the class, columns of its window (the stream form's `ks`)
    int ksplit[4];        // pieces asked of the class's launch (it may use fewer)
    long long off[4];     // floats: the class image in the workspace
    long long floats;     // the whole workspace
    int ho, wo;
};

// false: what the entry points reject.  The class with the longest contraction (all of them for ks = 1) is cut into `ksplit` pieces, the
// shorter ones in proportion -- pieces of about the same length --, never below one pair of 32-deep slices per piece.
inline bool conv_s2_dgrad_plan(int nimg, int h, int w, int cin, int cout, int ks, int ksplit, S2Plan &p)
{
    if (nimg <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || (cout % 64) != 0 || (cin & 3) || (ks != 1 && ks != 3) || ksplit < 1 || ksplit > 64)
        return false;
    p.ho = (h - 1) / 2 + 1;
    p.wo = (w - 1) / 2 + 1;
    const long long pixels = (long long)nimg * h * w;
    if (pixels > 0x7fffffffLL || (pixels + 256) * cin * 4 >= 0xC0000000LL || (long long)nimg * p.ho * p.wo * cout * 4 >= 0xC0000000LL) return false;
    p.ncls = ks == 3 ? 4 : 1;
    p.hc[0] = (h + 1) / 2, p.hc[1] = h / 2, p.wc[0] = (w + 1) / 2, p.wc[1] = w / 2;
    const int tmax = ks == 3 ? 4 : 1;
    p.floats = 0;
    for (int c = 0; c < 4; ++c) {
        const int py = c >> 1, px = c & 1;
        p.taps[c] = (1 + py) * (1 + px);
        p.win[c] = 1 + px;
        p.M[c] = c < p.ncls ? (long long)nimg * p.hc[py] * p.wc[px] : 0;
        const int pairs = p.taps[c] * cout / 64;
        const int want = (ksplit * p.taps[c] + tmax - 1) / tmax;
        p.ksplit[c] = want < pairs ? want : pairs;
        p.off[c] = p.floats;
        p.floats += p.M[c] * cin * p.ksplit[c];
    }
    return true;
}

// bytes of the packed image of class c's weight [cin, taps cout] (tf_linear_pack_weight_f32 with K = taps cout, N = cin)
inline int64_t conv_s2_class_packed_bytes(int taps, int cin, int cout, int terms) { return tf_linear_packed_bytes(taps * cout, cin, terms); }

// ---- dw of the strided 1 x 1: x[m, k] of the gathered matrix: k = ci, m = (n ho + .) wout + wo (decoded once per 8 rows, then stepped)
struct WgradRowsConv1 {
    const float *x, *x_scale2;
    int hin, win, cin, hout, wout, stride;
    int ci;
    bool bok;
    __device__ __forceinline__ void init(int k, bool ok)
    {
        bok = ok;
        ci = ok ? k : 0;
    }
    __device__ __forceinline__ void load8(int m0, int M, float (&dst)[8]) const
    {
        const int hw = hout * wout;
        const int mm = m0 < M ? m0 : 0;
        int n = mm / hw;
        const int rem = mm - n * hw;
        int ho = rem / wout, wo = rem - ho * wout;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const bool ok = bok && m0 + r < M;   // ((hout - 1) stride < hin: every pixel of the map is inside the image)
            dst[r] = ok ? x[((size_t)(n * hin + ho * stride) * win + wo * stride) * cin + ci] : 0.f;
            if (++wo == wout) {
                wo = 0;
                if (++ho == hout) {
                    ho = 0;
                    ++n;
                }
            }
        }
    }
    __device__ __forceinline__ float scale(int k) const { return x_scale2[k]; }
    __device__ __forceinline__ float inv_scale(int k) const { return x_scale2[cin + k]; }
};

template <int SP>
__global__ void __launch_bounds__(256)
conv1x1_strided_wgrad_kernel(const float *__restrict__ dy, const float *__restrict__ x, const float *__restrict__ dy_scale2,
                             const float *__restrict__ x_scale2, float *__restrict__ out, int M, int N, int K, int ktiles, int spc, int hin,
                             int win, int hout, int wout, int stride)
{
    wgrad_tile<SP>(dy, dy_scale2, out, M, N, K, ktiles, spc, WgradRowsConv1{x, x_scale2, hin, win, K, hout, wout, stride, 0, false});
}

}  // namespace

extern "C" int64_t tf_conv_dgrad_stride2_workspace_bytes(int nimg, int h, int w, int cin, int cout, int ks, int ksplit)
{
    S2Plan p;
    if (!conv_s2_dgrad_plan(nimg, h, w, cin, cout, ks, ksplit, p)) return -1;
    return p.floats * 4;
}

extern "C" int tf_conv_dgrad_stride2_packed_f32(const float *dy, const float *dy_scale2, const void *wcls_packed, float *dx, void *workspace,
                                                int64_t workspace_bytes, int ksplit, int nimg, int h, int w, int cin, int cout, int ks, int terms,
                                                void *stream)
{
    if (!dy || !wcls_packed || !dx || !workspace) return TF_MSDA_ERR_NULL_POINTER;
    const int sp = split_scheme(terms);
    S2Plan p;
    if (!conv_s2_dgrad_plan(nimg, h, w, cin, cout, ks, ksplit, p) || sp == 0) return TF_MSDA_ERR_BAD_DIMS;
    if (!aligned16(dy) || !aligned16(wcls_packed) || !aligned16(dx) || !aligned16(workspace)) return TF_MSDA_ERR_BAD_DIMS;
    if (workspace_bytes < p.floats * 4) return TF_MSDA_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *ws = static_cast<float *>(workspace);
    const char *wimg = static_cast<const char *>(wcls_packed);
    S2Class cls[4] = {};
    for (int c = 0; c < p.ncls; ++c) {
        const int K = p.taps[c] * cout;
        if (p.M[c] > 0) {   // (a one-row or one-column image has no odd pixels)
            const StreamConv cv{nimg, p.ho, p.wo, cout, p.hc[c >> 1], p.wc[c & 1], p.win[c], 0, 1};
            int pieces = 0;
            float *img = ws + p.off[c];
            const StreamCall call{dy, reinterpret_cast<const u32x4 *>(wimg), dy_scale2, nullptr, img, (int)p.M[c], K, cin, 0, true, cv, img, p.ksplit[c], &pieces};
            int rc;
            if (dy_scale2 == nullptr) rc = stream_dispatch_scheme<true>(sp, call, s);
            else rc = sp == 3 ? stream_dispatch<3, true, true>(call, s) : stream_dispatch<16, true, true>(call, s);
            if (rc) return rc;
            cls[c] = S2Class{p.off[c], p.M[c] * cin, pieces};
        }
        wimg += conv_s2_class_packed_bytes(p.taps[c], cin, cout, terms);
    }
    const S2Classes cl{cls[0], cls[1], cls[2], cls[3], p.hc[0], p.hc[1], p.wc[0], p.wc[1]};
    const long long total4 = (long long)nimg * h * w * (cin >> 2);
    hipLaunchKernelGGL(conv_s2_dgrad_assemble_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, (const float *)ws, dx, cl,
                       (unsigned)total4, h, w, cin >> 2);
    return tfm::launched();
}

// (stride 2 only: the stride-1 1 x 1 is a linear on the pixel matrix, tf_linear_wgrad_split_f32)
extern "C" int64_t tf_conv1x1_strided_wgrad_workspace_bytes(int nimg, int hin, int win, int cin, int cout, int stride)
{
    return conv_wgrad_workspace_bytes(1, 2, nimg, hin, win, cin, cout, stride);
}

extern "C" int tf_conv1x1_strided_wgrad_split_f32(const float *dy, const float *x, const float *dy_scale2, const float *x_scale2, float *dw,
                                                  void *workspace, int64_t workspace_bytes, int nimg, int hin, int win, int cin, int cout,
                                                  int stride, int terms, void *stream)
{
    // conv_wgrad_entry of conv_bwd.h: the gates, the chunks and the second pass of tf_conv3x3_wgrad_split_f32, with one tap and no padding
    return conv_wgrad_entry(1, 2, dy, x, dy_scale2, x_scale2, dw, workspace, workspace_bytes, nimg, hin, win, cin, cout, stride, terms, stream,
                            [=](int sp, dim3 grid, hipStream_t s, float *out, int M, int N, int K, int ktiles, int spc, const ConvWgradDims &d) {
                                if (sp == 3)
                                    hipLaunchKernelGGL(conv1x1_strided_wgrad_kernel<3>, grid, dim3(256), 0, s, dy, x, dy_scale2, x_scale2, out, M, N, K,
                                                       ktiles, spc, hin, win, d.hout, d.wout, stride);
                                else
                                    hipLaunchKernelGGL(conv1x1_strided_wgrad_kernel<16>, grid, dim3(256), 0, s, dy, x, dy_scale2, x_scale2, out, M, N, K,
                                                       ktiles, spc, hin, win, d.hout, d.wout, stride);
                            });
}

#endif /* TF_CONV_STRIDED_BWD_H_ */
