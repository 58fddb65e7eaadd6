// trackformer_amd/csrc/conv_bwd.h -- the backward of a 3 x 3 convolution (padding 1, no groups, no dilation) as split products (included
// behind linear_bwd.h at the end of linear_stream.hip; include/tf_fused.h: THE BACKWARD OF A 3 x 3 CONVOLUTION).  NHWC fp32 tensors,
// the weight [cout, 3, 3, cin] tap-major; M = nimg hout wout output pixels.
//
//   dw[co, ky, kx, ci] = sum_m dy[m, co] x[n, ho s + ky - 1, wo s + kx - 1, ci]    tf_conv3x3_wgrad_split_f32: wgrad_tile of linear_bwd.h
//                        with the row address of the x operand replaced -- column k of the tile is (tap, ci), row m is (n, ho, wo); nothing
//                        else is new: the same products in the same order as tf_linear_wgrad_split_f32 on the unfolded matrix
//   dx = conv3x3(dy, w_rot)  (stride 1)                                            tf_conv3x3_dgrad_packed_f32: tf_conv_packed_f32's two
//                        kernels (halo form / stream form, chosen by the same rule) in their scaled-activation instantiation
// No atomics: every result is a pure function of the arguments.
#ifndef TF_CONV_BWD_H_
#define TF_CONV_BWD_H_

namespace {

// x[m, k] of the unfolded matrix: k = tap cin + ci (decoded once per thread), m = (n ho + .) wout + wo (decoded once per 8 rows, then
// stepped); a shifted pixel outside the image is an exact zero and is never read -- not the neighbouring row, not the next image
struct WgradRowsConv3 {
    const float *x, *x_scale2;
    int hin, win, cin, hout, wout, stride;
    int ci, dyo, dxo;
    bool bok;
    __device__ __forceinline__ void init(int k, bool ok)
    {
        bok = ok;
        const int kk = ok ? k : 0, tap = kk / cin, ky = tap / 3;
        ci = kk - tap * cin;
        dyo = ky - 1;
        dxo = tap - ky * 3 - 1;
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
            const int hi = ho * stride + dyo, wi = wo * stride + dxo;
            const bool ok = bok && m0 + r < M && (unsigned)hi < (unsigned)hin && (unsigned)wi < (unsigned)win;
            dst[r] = ok ? x[((size_t)(n * hin + hi) * win + wi) * cin + ci] : 0.f;
            if (++wo == wout) {
                wo = 0;
                if (++ho == hout) {
                    ho = 0;
                    ++n;
                }
            }
        }
    }
    // one scale per input channel, shared by the nine taps
    __device__ __forceinline__ float scale(int k) const { return x_scale2[k % cin]; }
    __device__ __forceinline__ float inv_scale(int k) const { return x_scale2[cin + k % cin]; }
};

template <int SP>
__global__ void __launch_bounds__(256)
conv3x3_wgrad_kernel(const float *__restrict__ dy, const float *__restrict__ x, const float *__restrict__ dy_scale2,
                     const float *__restrict__ x_scale2, float *__restrict__ out, int M, int N, int K, int ktiles, int spc, int hin, int win,
                     int cin, int hout, int wout, int stride)
{
    wgrad_tile<SP>(dy, dy_scale2, out, M, N, K, ktiles, spc, WgradRowsConv3{x, x_scale2, hin, win, cin, hout, wout, stride, 0, 0, 0, false});
}

// the dimensions of the weight gradient's GEMM, or false for what the entry point rejects; taps: 9 (3 x 3, padding 1) or 1 (1 x 1, no
// padding: conv_strided_bwd.h), strides min_stride .. 2
struct ConvWgradDims {
    long long M;
    int hout, wout, K;
};
inline bool conv_wgrad_dims(int taps, int min_stride, int nimg, int hin, int win, int cin, int cout, int stride, ConvWgradDims &d)
{
    if (nimg <= 0 || hin <= 0 || win <= 0 || cin <= 0 || cout <= 0 || (cin & 3) || (cout & 3) || stride < min_stride || stride > 2) return false;
    d.hout = (hin - 1) / stride + 1;
    d.wout = (win - 1) / stride + 1;
    d.M = (long long)nimg * d.hout * d.wout;
    if (d.M > 0x7fffffffLL || (long long)taps * cin > 0x7fffffffLL) return false;
    d.K = taps * cin;
    return true;
}

inline int64_t conv_wgrad_workspace_bytes(int taps, int min_stride, int nimg, int hin, int win, int cin, int cout, int stride)
{
    ConvWgradDims d;
    if (!conv_wgrad_dims(taps, min_stride, nimg, hin, win, cin, cout, stride, d)) return -1;
    const WgradPlan p = wgrad_plan(d.M, d.K, cout);
    return p.msplit > 1 ? (int64_t)p.msplit * cout * d.K * 4 : 0;
}

// the gates, the chunks of the pixel loop and the second pass of a convolution's weight gradient (ONE copy for the 3 x 3 and the strided
// 1 x 1); launch(sp, grid, stream, out, M, N, K, ktiles, spc, dims) starts the kernel with the layer's row map
template <class LAUNCH>
int conv_wgrad_entry(int taps, int min_stride, const float *dy, const float *x, const float *dy_scale2, const float *x_scale2, float *dw,
                     void *workspace, int64_t workspace_bytes, int nimg, int hin, int win, int cin, int cout, int stride, int terms, void *stream,
                     LAUNCH launch)
{
    if (!dy || !x || !dy_scale2 || !x_scale2 || !dw) return TF_MSDA_ERR_NULL_POINTER;
    const int sp = split_scheme(terms);
    ConvWgradDims d;
    if (!conv_wgrad_dims(taps, min_stride, nimg, hin, win, cin, cout, stride, d) || sp == 0) return TF_MSDA_ERR_BAD_DIMS;
    const int N = cout, K = d.K;
    if (d.M * N * 4 >= 0xC0000000LL || (long long)nimg * hin * win * cin * 4 >= 0xC0000000LL || (long long)N * K * 4 >= 0xC0000000LL)
        return TF_MSDA_ERR_BAD_DIMS;
    if (!aligned16(dy) || !aligned16(x) || !aligned16(dw) || !aligned16(x_scale2)) return TF_MSDA_ERR_BAD_DIMS;
    const WgradPlan p = wgrad_plan(d.M, K, N);
    const int64_t need = p.msplit > 1 ? (int64_t)p.msplit * N * K * 4 : 0;
    if (need > 0 && (!workspace || workspace_bytes < need || !aligned16(workspace))) return TF_MSDA_ERR_WORKSPACE;
    const int ntiles = (N + kWgTile - 1) / kWgTile, ktiles = (K + kWgTile - 1) / kWgTile;
    if ((long long)ntiles * ktiles > 0x7fffffffLL) return TF_MSDA_ERR_BAD_DIMS;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *out = p.msplit > 1 ? static_cast<float *>(workspace) : dw;
    launch(sp, dim3((unsigned)(ntiles * ktiles), (unsigned)p.msplit), s, out, (int)d.M, N, K, ktiles, p.spc, d);
    if (int rc = tfm::launched()) return rc;
    return p.msplit > 1 ? launch_splitk_reduce(out, nullptr, nullptr, dw, (long long)N * K, K, p.msplit, 0, s) : TF_MSDA_OK;
}

}  // namespace

extern "C" int64_t tf_conv3x3_wgrad_workspace_bytes(int nimg, int hin, int win, int cin, int cout, int stride)
{
    return conv_wgrad_workspace_bytes(9, 1, nimg, hin, win, cin, cout, stride);
}

extern "C" int tf_conv3x3_wgrad_split_f32(const float *dy, const float *x, const float *dy_scale2, const float *x_scale2, float *dw,
                                          void *workspace, int64_t workspace_bytes, int nimg, int hin, int win, int cin, int cout, int stride,
                                          int terms, void *stream)
{
    return conv_wgrad_entry(9, 1, dy, x, dy_scale2, x_scale2, dw, workspace, workspace_bytes, nimg, hin, win, cin, cout, stride, terms, stream,
                            [=](int sp, dim3 grid, hipStream_t s, float *out, int M, int N, int K, int ktiles, int spc, const ConvWgradDims &d) {
                                if (sp == 3)
                                    hipLaunchKernelGGL(conv3x3_wgrad_kernel<3>, grid, dim3(256), 0, s, dy, x, dy_scale2, x_scale2, out, M, N, K, ktiles, spc,
                                                       hin, win, cin, d.hout, d.wout, stride);
                                else
                                    hipLaunchKernelGGL(conv3x3_wgrad_kernel<16>, grid, dim3(256), 0, s, dy, x, dy_scale2, x_scale2, out, M, N, K, ktiles, spc,
                                                       hin, win, cin, d.hout, d.wout, stride);
                            });
}

// dx = conv3x3(dy, w_rot): tf_conv_packed_f32(ks = 3, stride = 1, the same workspace / ksplit) with dy [nimg, h, w, cout] as the input
// and cin output channels -- the same choice between the halo form and the stream form, the same block shapes, the same cut of the
// contraction into ksplit pieces -- in the kernels' scaled-activation instantiation (`bias` carries scale2; a partial sum leaves its
// workgroup multiplied by 1 / s, the second pass adds the pieces in order); without dy_scale2 the plain instantiation, i.e.
// tf_conv_packed_f32 itself
extern "C" int tf_conv3x3_dgrad_packed_f32(const float *dy, const float *dy_scale2, const void *wrot_packed, float *dx, float *workspace,
                                           int ksplit, int nimg, int h, int w, int cin, int cout, int terms, void *stream)
{
    if (!dy || !wrot_packed || !dx) return TF_MSDA_ERR_NULL_POINTER;
    if (ksplit > 1 && !workspace) return TF_MSDA_ERR_NULL_POINTER;
    const int sp = split_scheme(terms);
    // (the contraction runs over 9 cout: pairs of 32-deep slices per tap)
    if (nimg <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || (cout % 64) != 0 || (cin & 3) || sp == 0 || ksplit < 1 || ksplit > 64)
        return TF_MSDA_ERR_BAD_DIMS;
    if (ksplit > 1 && !aligned16(workspace)) return TF_MSDA_ERR_BAD_DIMS;
    const long long M = (long long)nimg * h * w;
    if (M > 0x7fffffffLL || (M + 256) * cin * 4 >= 0xC0000000LL || M * cout * 4 >= 0xC0000000LL) return TF_MSDA_ERR_BAD_DIMS;
    if (!aligned16(dy) || !aligned16(wrot_packed) || !aligned16(dx)) return TF_MSDA_ERR_BAD_DIMS;
    const StreamConv cv{nimg, h, w, cout, h, w, 3, 1, 1};
    const StreamCall c{dy, static_cast<const u32x4 *>(wrot_packed), dy_scale2, nullptr, dx, (int)M, 9 * cout, cin, 0, true, cv, workspace, ksplit};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool halo = tfm::dense_knob(tfm::kKnobConvHalo) != 0;
    if (dy_scale2 == nullptr) {
        if (halo) return sp == 3 ? halo_dispatch<3>(c, s) : halo_dispatch<16>(c, s);
        return stream_dispatch_scheme<true>(sp, c, s);
    }
    if (halo) return sp == 3 ? halo_dispatch<3, true>(c, s) : halo_dispatch<16, true>(c, s);
    return sp == 3 ? stream_dispatch<3, true, true>(c, s) : stream_dispatch<16, true, true>(c, s);
}

#endif /* TF_CONV_BWD_H_ */
