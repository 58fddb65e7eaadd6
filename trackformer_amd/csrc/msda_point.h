// trackformer_amd/csrc/msda_point.h -- the arithmetic of ONE sampling point, defined once for every MSDeformAttn kernel:
//   fused_location   sampling location from the raw offset and the reference point (MSDeformAttn.forward's formulas)
//   pixel_point<T>   location -> pixel coordinates, in-range rule, floor, bilinear fractions
//   point_corners    which of the four corners lie inside the level, and the row index of the first
//   Tap<T> / make_tap<T>   the clamped form of the generic row-gather kernels and msda_bwd_det.h
// Included by msda_hip.hip and msda_pquad.hip (and through them by the kernel headers).  The host-tensor implementation
// (msda_host.cpp: plain C++, no HIP) has a make_taps of its own.
#ifndef TF_MSDA_POINT_H_
#define TF_MSDA_POINT_H_

#include <hip/hip_runtime.h>

namespace tfm {

__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float floor_t(float a) { return __builtin_floorf(a); }
__device__ __forceinline__ double floor_t(double a) { return __builtin_floor(a); }

// The sampling location of one sample: the module's formulas (ops/modules/ms_deform_attn.py:75-85), operation by operation,
//     loc = ref[:2] + off / (H_l, W_l)                (ref_dim == 2; x over H_l and y over W_l, as the reference writes it)
//     loc = ref[:2] + off / P * ref[2:] * 0.5         (ref_dim == 4; inv_p = 1 / P, exact for the power-of-two P of every config)
// Every fused prologue and both kernels of msda_fused_bwd.h call it, so they agree to the bit.  THE ONE DELIBERATE VARIANT:
// msda_fwd_f32_pquad (msda_pquad.hip) and msda_fwd_f32_pquad2 (msda_pquad2.h) form off * (1 / H_l) with a v_rcp_f32
// reciprocal instead of the IEEE division (<= 1 ulp of the location, ~10 instructions per division saved in the hot encoder
// kernel); they keep their own two lines.
__device__ __forceinline__ float2 fused_location(const float *rp, int ref_dim, float2 off, float h, float w, float inv_p)
{
#pragma clang fp contract(off)
    float2 xy;
    if (ref_dim == 2) {
        xy.x = rp[0] + off.x / h;                       // x over H_l, as written
        xy.y = rp[1] + off.y / w;
    } else {
        xy.x = rp[0] + off.x * inv_p * rp[2] * 0.5f;
        xy.y = rp[1] + off.y * inv_p * rp[3] * 0.5f;
    }
    return xy;
}

// One sampling point in pixel coordinates.  Follows SURVEY.md Appendix A / cuh:227-229, :24-67.
template <typename T>
struct PixelPoint {
    T fx, fy, gx, gy;   // lw, lh, hw, hh of the reference
    int x0, y0;         // floor of the pixel coordinates: the top-left corner (-1 is possible: the corner is then outside)
    bool in;            // live AND the reference's range test; when false the other fields are those of pixel (0, 0)
};

template <typename T>
__device__ __forceinline__ PixelPoint<T> pixel_point(T lx, T ly, T Wf, T Hf, bool live)
{
    PixelPoint<T> p;
    // loc*size - 0.5 with a SINGLE rounding (one fma).  The reference's fp32 instantiation rounds twice
    // (cuh:227-228: `loc * spatial` is a float product, then `- 0.5` in double, narrowed to float), its
    // pure-PyTorch path (func.py:40-49, grid_sample at 2*loc-1) rounds three times: the three agree to 1 ulp
    // of the pixel coordinate, i.e. they can differ only for samples within 1 ulp of an integer pixel
    // boundary, where the bilinear weight of the disputed tap is <= 1 ulp as well (outputs differ by ~1e-7;
    // the in-range test at exactly -1 / size can flip, a measure-zero set the golden tests exclude).
    // The oracle (oracle/msda_ref.c) uses the same single rounding; fp64 is exact in all three.
    const T xr = fma_t(lx, Wf, (T)-0.5);
    const T yr = fma_t(ly, Hf, (T)-0.5);
    p.in = live && (yr > (T)-1) && (xr > (T)-1) && (yr < Hf) && (xr < Wf);   // cuh:229
    // Out-of-range samples may carry huge / non-finite coordinates: neutralise them so that every
    // derived quantity stays finite (their taps are all invalid anyway).
    const T x = p.in ? xr : (T)0, y = p.in ? yr : (T)0;
    const T xf = floor_t(x), yf = floor_t(y);
    p.fx = x - xf;
    p.fy = y - yf;
    p.gx = (T)1 - p.fx;
    p.gy = (T)1 - p.fy;
    p.x0 = (int)xf;
    p.y0 = (int)yf;
    return p;
}

// The four corners (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) of a point: corner (i, j) contributes iff
// kx<i> && ky<j>; its row inside the level is r<j> + i.  r0 may be "negative": only used when the corner is valid.
// (With both rows the struct is 12 bytes.  At 8 bytes or less the calling convention returns a struct as packed integers, and
// the four flags then stay packed in one register after inlining: shifts, masks and 2 to 4 more VGPRs in every kernel.)
struct PointCorners {
    bool kx0, kx1, ky0, ky1;
    int r0, r1;   // rows of (x0, y0) and (x0, y0 + 1)
};

__device__ __forceinline__ PointCorners point_corners(int x0, int y0, int W, int H, bool in)
{
    PointCorners c;
    c.kx0 = in && (x0 >= 0);
    c.kx1 = in && (x0 + 1 <= W - 1);
    c.ky0 = in && (y0 >= 0);
    c.ky1 = in && (y0 + 1 <= H - 1);
    c.r0 = y0 * W + x0;
    c.r1 = c.r0 + W;
    return c;
}

// pixel_point plus clamped tap offsets (in units of pixels within the level) and tap validity: for kernels that load
// through plain pointers and select, instead of letting the buffer hardware return zeros.
template <typename T>
struct Tap {
    T fx, fy, gx, gy;       // lw, lh, hw, hh of the reference
    int o1, o2, o3, o4;     // clamped pixel offsets y*W + x of the four taps
    bool k1, k2, k3, k4;    // tap contributes (sample in range AND corner inside the level)
};

template <typename T>
__device__ __forceinline__ Tap<T> make_tap(T lx, T ly, int H, int W)
{
    const PixelPoint<T> p = pixel_point(lx, ly, (T)W, (T)H, true);
    const PointCorners c = point_corners(p.x0, p.y0, W, H, p.in);
    Tap<T> t;
    t.fx = p.fx;
    t.fy = p.fy;
    t.gx = p.gx;
    t.gy = p.gy;
    const int cx0 = max(p.x0, 0), cx1 = min(p.x0 + 1, W - 1);
    const int cy0 = max(p.y0, 0), cy1 = min(p.y0 + 1, H - 1);
    t.o1 = cy0 * W + cx0;
    t.o2 = cy0 * W + cx1;
    t.o3 = cy1 * W + cx0;
    t.o4 = cy1 * W + cx1;
    t.k1 = c.ky0 && c.kx0;
    t.k2 = c.ky0 && c.kx1;
    t.k3 = c.ky1 && c.kx0;
    t.k4 = c.ky1 && c.kx1;
    return t;
}

}  // namespace tfm

#endif  // TF_MSDA_POINT_H_
