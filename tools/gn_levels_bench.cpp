// tools/gn_levels_bench.cpp -- standalone (no Python, no torch) timing harness for tf_groupnorm_levels_nhwc_f32 (include/tf_fused.h):
// the GroupNorm of all four input-projection levels of the 800 x 1333 frame in two launches into the token buffer, against the
// sequence it replaces.
//
//   tools/bin/gn_levels_bench [rounds [sets]]   (built by trackformer_amd/build.py; default 9 4)
//
// cfg-2 shapes: 16 700, 4 200, 1 050 and 273 rows x 256 channels, 32 groups.  The finest level arrives as a finished y (its GEMM is not
// split); the three coarse ones are convolutions whose K loop is cut by the policy of trackformer_amd/fused.py (_conv_ksplit; printed).
// The split-K second pass is not callable on its own, so BOTH sequences carry the three coarse GEMM launches -- the same kernels on the
// same operands -- and differ in what follows them:
//   old   tf_conv_packed_f32 (GEMM + reduce launch) x 3, tf_groupnorm_nhwc_f32 (zero, statistics, apply) x 4 into a staging buffer, one
//         device-to-device copy of the 22 223 x 256 floats standing for torch.cat             3 + 3 + 12 + 1 = 19 launches
//   new   tf_conv_packed_partials_f32 (GEMM only) x 3, tf_groupnorm_levels_nhwc_f32                              3 + 2 =  5 launches
// Timing: one HIP graph per variant holding `sets` sequences, each on its own buffers (sets x ~115 MB is larger than the Infinity
// Cache: every sequence starts cold, as in a frame); HIP events around a replay; the variants ALTERNATE for `rounds` rounds.  One JSON
// line: median / min / max microseconds per sequence, and whether the new median is below the old minimum (the project's rule).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "tf_fused.h"
#include "tf_msda.h"

#define CK(x)                                                                                     \
    do {                                                                                          \
        hipError_t e_ = (x);                                                                      \
        if (e_ != hipSuccess) {                                                                   \
            fprintf(stderr, "%s:%d: %s -> %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));  \
            exit(2);                                                                              \
        }                                                                                         \
    } while (0)
#define TF(x)                                                                           \
    do {                                                                                \
        int rc_ = (x);                                                                  \
        if (rc_ != 0) {                                                                 \
            fprintf(stderr, "%s:%d: %s -> %s\n", __FILE__, __LINE__, #x, tf_msda_strerror(rc_)); \
            exit(2);                                                                    \
        }                                                                               \
    } while (0)

namespace {

constexpr int C = 256, G = 32, T = 16, NLEV = 4;
constexpr float EPS = 1e-5f;

// fused.py _conv_ksplit with the default policy (768, 300, 8, 32)
int conv_ksplit(int m, int k, int cout)
{
    const int blocks = ((m + 63) / 64) * ((cout + 127) / 128), slices = k / 32;
    if (blocks >= 300 || slices < 32) return 1;
    return std::max(1, std::min(64, std::min(768 / blocks, slices / 8)));
}

struct Level {   // a coarse level: its convolution
    int hin, win, cin, ks, stride, hw, ksplit;
    void *packed;
    float *bias, *gamma, *beta;
};

float *device_random(size_t n, float scale, float shift, std::mt19937 &rng)
{
    std::normal_distribution<float> nrm(0.f, 1.f);
    std::vector<float> h(n);
    for (auto &v : h) v = nrm(rng) * scale + shift;
    float *d;
    CK(hipMalloc(&d, n * 4));
    CK(hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice));
    return d;
}

struct Stat {
    double med, lo, hi;
};
Stat stat_of(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return Stat{v[v.size() / 2], v.front(), v.back()};
}

}  // namespace

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 9, sets = argc > 2 ? atoi(argv[2]) : 4;
    hipStream_t s;
    CK(hipStreamCreate(&s));
    std::mt19937 rng(11);
    const int hw0 = 100 * 167;   // the finest level: 16 700 rows, not split
    Level lv[3] = {{50, 84, 1024, 1, 1, 50 * 84, 0, nullptr, nullptr, nullptr, nullptr},
                   {25, 42, 2048, 1, 1, 25 * 42, 0, nullptr, nullptr, nullptr, nullptr},
                   {25, 42, 2048, 3, 2, 13 * 21, 0, nullptr, nullptr, nullptr, nullptr}};
    for (Level &l : lv) {
        const int K = l.ks * l.ks * l.cin;
        l.ksplit = conv_ksplit(l.hw, K, C);
        if (l.ks == 1 && l.ksplit < 3) l.ksplit = 1;
        float *w = device_random((size_t)C * K, 1.f / std::sqrt((float)K), 0.f, rng);
        CK(hipMalloc(&l.packed, (size_t)tf_linear_packed_bytes(K, C, T)));
        TF(tf_linear_pack_weight_f32(w, l.packed, K, C, T, s));
        CK(hipStreamSynchronize(s));
        CK(hipFree(w));
        l.bias = device_random(C, 0.1f, 0.f, rng);
        l.gamma = device_random(C, 0.2f, 1.f, rng);
        l.beta = device_random(C, 0.2f, 0.f, rng);
    }
    float *gamma0 = device_random(C, 0.2f, 1.f, rng), *beta0 = device_random(C, 0.2f, 0.f, rng);
    const int rows[NLEV] = {hw0, lv[0].hw, lv[1].hw, lv[2].hw};
    int row0[NLEV], S = 0;
    for (int i = 0; i < NLEV; ++i) row0[i] = S, S += rows[i];

    struct Set {
        float *y0, *x[3], *y[3], *part[3], *stage, *out_old, *out_new;
        double *gws, *lws;
    };
    std::vector<Set> st(sets);
    tf_gn_level probe[NLEV];
    for (int i = 0; i < NLEV; ++i) probe[i] = tf_gn_level{gamma0, nullptr, gamma0, gamma0, 1, rows[i], row0[i]};   // (sizes only)
    int pieces[3] = {0, 0, 0};
    for (Set &e : st) {
        e.y0 = device_random((size_t)hw0 * C, 1.f, 0.3f, rng);
        for (int i = 0; i < 3; ++i) {
            e.x[i] = (i == 2) ? e.x[1] : device_random((size_t)lv[i].hin * lv[i].win * lv[i].cin, 1.f, 0.2f, rng);   // the extra level reads layer4 too
            CK(hipMalloc(&e.y[i], (size_t)lv[i].hw * C * 4));
            CK(hipMalloc(&e.part[i], (size_t)std::max(lv[i].ksplit, 1) * lv[i].hw * C * 4));
        }
        CK(hipMalloc(&e.stage, (size_t)S * C * 4));
        CK(hipMalloc(&e.out_old, (size_t)S * C * 4));
        CK(hipMalloc(&e.out_new, (size_t)S * C * 4));
        CK(hipMalloc(&e.gws, 2 * G * sizeof(double)));
        e.lws = nullptr;
    }
    auto conv_old = [&](const Set &e, int i) {
        const Level &l = lv[i];
        TF(tf_conv_packed_f32(e.x[i], l.packed, l.bias, nullptr, e.y[i], e.part[i], l.ksplit, 1, l.hin, l.win, l.cin, C, l.ks, l.stride, 0, T, s));
    };
    auto conv_new = [&](const Set &e, int i) {
        const Level &l = lv[i];
        TF(tf_conv_packed_partials_f32(e.x[i], l.packed, l.bias, e.part[i], l.ksplit, 1, l.hin, l.win, l.cin, C, l.ks, l.stride, T, &pieces[i], s));
    };
    auto table_of = [&](const Set &e, tf_gn_level *t) {
        t[0] = tf_gn_level{e.y0, nullptr, gamma0, beta0, 1, rows[0], row0[0]};
        for (int i = 0; i < 3; ++i) t[i + 1] = tf_gn_level{e.part[i], lv[i].bias, lv[i].gamma, lv[i].beta, pieces[i], rows[i + 1], row0[i + 1]};
    };
    auto old_seq = [&](int k) {
        const Set &e = st[k];
        for (int i = 0; i < 3; ++i) conv_old(e, i);
        TF(tf_groupnorm_nhwc_f32(e.y0, gamma0, beta0, e.stage, e.gws, 1, rows[0], C, G, EPS, (int64_t)rows[0] * C, (int64_t)rows[0] * C, s));
        for (int i = 0; i < 3; ++i)
            TF(tf_groupnorm_nhwc_f32(e.y[i], lv[i].gamma, lv[i].beta, e.stage + (size_t)row0[i + 1] * C, e.gws, 1, rows[i + 1], C, G, EPS,
                                     (int64_t)rows[i + 1] * C, (int64_t)rows[i + 1] * C, s));
        CK(hipMemcpyAsync(e.out_old, e.stage, (size_t)S * C * 4, hipMemcpyDeviceToDevice, s));
    };
    auto new_seq = [&](int k) {
        const Set &e = st[k];
        for (int i = 0; i < 3; ++i) conv_new(e, i);
        tf_gn_level t[NLEV];
        table_of(e, t);
        TF(tf_groupnorm_levels_nhwc_f32(t, NLEV, 1, C, G, EPS, e.out_new, (int64_t)S * C, e.lws, s));
    };
    // the piece counts the launch code makes of the policy's ksplit (needed for the workspace size), then the workspaces
    for (int i = 0; i < 3; ++i) conv_new(st[0], i);
    CK(hipStreamSynchronize(s));
    for (int i = 0; i < 3; ++i) probe[i + 1].pieces = pieces[i];
    const int64_t n_ws = tf_groupnorm_levels_workspace_doubles(probe, NLEV, 1, C, G);
    if (n_ws <= 0) return 2;
    for (Set &e : st) CK(hipMalloc(&e.lws, (size_t)n_ws * sizeof(double)));
    printf("rows %d %d %d %d, ksplit (policy) 1 %d %d %d, pieces (launch) 1 %d %d %d, workspace %lld doubles\n", rows[0], rows[1], rows[2], rows[3],
           lv[0].ksplit, lv[1].ksplit, lv[2].ksplit, pieces[0], pieces[1], pieces[2], (long long)n_ws);

    // ---- agreement on set 0 (the old statistics are atomic sums: not bit for bit)
    old_seq(0);
    new_seq(0);
    CK(hipStreamSynchronize(s));
    std::vector<float> a((size_t)S * C), b((size_t)S * C);
    CK(hipMemcpy(a.data(), st[0].out_old, a.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(b.data(), st[0].out_new, b.size() * 4, hipMemcpyDeviceToHost));
    double worst = 0;
    for (size_t k = 0; k < a.size(); ++k) worst = std::max(worst, (double)std::fabs(a[k] - b[k]));
    new_seq(0);
    CK(hipStreamSynchronize(s));
    CK(hipMemcpy(a.data(), st[0].out_new, a.size() * 4, hipMemcpyDeviceToHost));
    long long differ = 0;
    for (size_t k = 0; k < a.size(); ++k) differ += a[k] != b[k] && !(a[k] != a[k] && b[k] != b[k]);

    // ---- timing
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    auto capture = [&](auto &&body) {
        hipGraph_t graph;
        hipGraphExec_t gexec;
        CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        for (int i = 0; i < sets; ++i) body(i);
        CK(hipStreamEndCapture(s, &graph));
        CK(hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0));
        CK(hipGraphDestroy(graph));
        return gexec;
    };
    hipGraphExec_t go = capture(old_seq), gn = capture(new_seq);
    auto replay = [&](hipGraphExec_t ge) {
        CK(hipEventRecord(e0, s));
        CK(hipGraphLaunch(ge, s));
        CK(hipEventRecord(e1, s));
        CK(hipStreamSynchronize(s));
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, e0, e1));
        return ms * 1000.0 / sets;
    };
    replay(go);   // warm-up (code objects, the graphs' first launch)
    replay(gn);
    std::vector<double> to, tn;
    for (int r = 0; r < rounds; ++r) {
        to.push_back(replay(go));
        tn.push_back(replay(gn));
    }
    const Stat so = stat_of(to), sn = stat_of(tn);
    printf("{\"shape\": \"cfg2_input_proj_levels\", \"rows\": %d, \"rounds\": %d, \"sets\": %d, \"pieces\": [1, %d, %d, %d], \"max_abs_diff_old_new\": %.3g, "
           "\"new_differs_between_two_calls\": %lld, \"old_us\": {\"median\": %.2f, \"min\": %.2f, \"max\": %.2f}, "
           "\"new_us\": {\"median\": %.2f, \"min\": %.2f, \"max\": %.2f}, \"saved_us_at_medians\": %.2f, \"new_wins\": %s}\n",
           S, rounds, sets, pieces[0], pieces[1], pieces[2], worst, differ, so.med, so.lo, so.hi, sn.med, sn.lo, sn.hi, so.med - sn.med,
           sn.med < so.lo ? "true" : "false");
    return (differ || !(worst < 1e-3)) ? 1 : 0;
}
