// tools/proj_groups_bench.cpp -- standalone (no Python, no torch) parity + timing harness for tf_linear_groups_f32
// (include/tf_fused.h): several projections of the same rows in one launch, against the launches it replaces.
//
//   tools/bin/proj_groups_bench [M [rounds [sets [TI]]]]  (built by trackformer_amd/build.py; default 22223 7 12: the cfg-2 encoder;
//   TI = 1 | 2 | 3: option "groups_ti", 32 / 64 / 96 rows per block of the grouped kernel)
//
// Two shapes, each checked BIT FOR BIT (rows behind M untouched) and then timed:
//   enc   M x 256 -> {256 of x, 384 of x + x2}   against tf_linear_split_f32 + tf_linear_split_add_f32
//   dec   M x 256 -> 6 x 256 of x                 against six tf_linear_split_f32
// Timing: one HIP graph per variant holding `sets` launches, each on its own input / output buffers (sets x (x, x2, outputs) is
// larger than the Infinity Cache: every launch starts cold, as in a frame); HIP events around a replay; the two variants of a shape
// ALTERNATE for `rounds` rounds.  One JSON line per shape: median / min / max microseconds per launch (or per replaced sequence).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

constexpr int K = 256;
int T = 16;

struct Weight {   // one projection: fp32 source, packed image, separate pieces (what tf_linear_split_f32 takes)
    int N = 0;
    float *w = nullptr, *bias = nullptr, *scale = nullptr;
    void *packed = nullptr;
    unsigned short *p[3] = {nullptr, nullptr, nullptr};
};

Weight make_weight(int N, std::mt19937 &rng, hipStream_t s)
{
    std::normal_distribution<float> nrm(0.f, 1.f);
    Weight wt;
    wt.N = N;
    std::vector<float> W((size_t)N * K), B(N), sc(N, 1.f);
    for (auto &v : W) v = nrm(rng) * 0.0625f;
    for (auto &v : B) v = nrm(rng) * 0.1f;
    std::vector<unsigned short> pc[3];
    for (auto &v : pc) v.assign(W.size(), 0);
    if (T == 16) {   // fp16 pieces wh, wl of w t_n + the channels' factors 16 / t_n
        for (int n = 0; n < N; ++n) {
            float amax = 0.f;
            for (int k = 0; k < K; ++k) amax = std::max(amax, std::fabs(W[(size_t)n * K + k]));
            int e = 0;
            (void)std::frexp(amax, &e);
            const float tn = amax > 0.f ? std::ldexp(1.f, 14 - e) : 1.f;
            sc[n] = 16.f / tn;
            for (int k = 0; k < K; ++k) {
                const size_t i = (size_t)n * K + k;
                const float ws = W[i] * tn;
                const _Float16 h = (_Float16)ws, l = (_Float16)(ws - (float)h);
                memcpy(&pc[0][i], &h, 2);
                memcpy(&pc[1][i], &l, 2);
            }
        }
    } else {
        for (size_t i = 0; i < W.size(); ++i) {
            float r = W[i];
            for (int q = 0; q < 3; ++q) {   // round to nearest even, residual exact
                unsigned u;
                memcpy(&u, &r, 4);
                u += 0x7FFFu + ((u >> 16) & 1u);
                pc[q][i] = (unsigned short)(u >> 16);
                const unsigned hu = (unsigned)pc[q][i] << 16;
                float hf;
                memcpy(&hf, &hu, 4);
                r -= hf;
            }
        }
    }
    CK(hipMalloc(&wt.w, W.size() * 4));
    CK(hipMemcpy(wt.w, W.data(), W.size() * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&wt.bias, B.size() * 4));
    CK(hipMemcpy(wt.bias, B.data(), B.size() * 4, hipMemcpyHostToDevice));
    for (int q = 0; q < (T == 16 ? 2 : 3); ++q) {
        CK(hipMalloc(&wt.p[q], W.size() * 2));
        CK(hipMemcpy(wt.p[q], pc[q].data(), W.size() * 2, hipMemcpyHostToDevice));
    }
    if (T == 16) {
        CK(hipMalloc(&wt.scale, sc.size() * 4));
        CK(hipMemcpy(wt.scale, sc.data(), sc.size() * 4, hipMemcpyHostToDevice));
    }
    CK(hipMalloc(&wt.packed, (size_t)tf_linear_packed_bytes(K, N, T)));
    TF(tf_linear_pack_weight_f32(wt.w, wt.packed, K, N, T, s));
    return wt;
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
    const int M = argc > 1 ? atoi(argv[1]) : 22223, rounds = argc > 2 ? atoi(argv[2]) : 7, sets = argc > 3 ? atoi(argv[3]) : 12;
    if (argc > 4) tf_msda_set_option("groups_ti", atoi(argv[4]));   // rows per block / 32 of the grouped kernel (0: by row count)
    const int Tenv = getenv("TF_SPLIT_TERMS") ? atoi(getenv("TF_SPLIT_TERMS")) : 16;
    T = Tenv == 6 ? 6 : 16;
    const int guard = 128;   // rows behind M that nothing may write
    hipStream_t s;
    CK(hipStreamCreate(&s));
    std::mt19937 rng(7);
    std::normal_distribution<float> nrm(0.f, 1.f);
    std::vector<float> hx((size_t)M * K);
    std::vector<float *> X(sets), X2(sets);
    for (int i = 0; i < sets; ++i) {
        for (auto &v : hx) v = nrm(rng);
        CK(hipMalloc(&X[i], hx.size() * 4));
        CK(hipMemcpy(X[i], hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
        for (auto &v : hx) v = nrm(rng) * 0.5f;
        CK(hipMalloc(&X2[i], hx.size() * 4));
        CK(hipMemcpy(X2[i], hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    long long bad = 0;

    // one shape: widths / add flags of its groups
    auto run_shape = [&](const char *name, const std::vector<int> &widths, const std::vector<int> &adds) {
        const int ng = (int)widths.size();
        std::vector<Weight> wts;
        for (int g = 0; g < ng; ++g) wts.push_back(make_weight(widths[g], rng, s));
        // outputs: per set and group, reference and grouped (the grouped ones with guard rows)
        std::vector<std::vector<float *>> Yr(sets, std::vector<float *>(ng)), Yg(sets, std::vector<float *>(ng));
        double out_mb = 0;
        for (int i = 0; i < sets; ++i)
            for (int g = 0; g < ng; ++g) {
                CK(hipMalloc(&Yr[i][g], (size_t)M * widths[g] * 4));
                CK(hipMalloc(&Yg[i][g], (size_t)(M + guard) * widths[g] * 4));
                CK(hipMemsetAsync(Yg[i][g], 0xFF, (size_t)(M + guard) * widths[g] * 4, s));
                if (i == 0) out_mb += (double)M * widths[g] * 4e-6;
            }
        auto separate = [&](int i) {
            for (int g = 0; g < ng; ++g) {
                const Weight &w = wts[g];
                if (adds[g]) TF(tf_linear_split_add_f32(X[i], X2[i], w.p[0], w.p[1], w.p[2], w.scale, w.bias, Yr[i][g], M, K, w.N, s));
                else TF(tf_linear_split_f32(X[i], w.p[0], w.p[1], w.p[2], w.scale, w.bias, Yr[i][g], M, K, w.N, 0, s));
            }
        };
        auto grouped = [&](int i) {
            tf_proj_group d[8];
            for (int g = 0; g < ng; ++g) d[g] = tf_proj_group{wts[g].packed, wts[g].bias, Yg[i][g], wts[g].N, adds[g]};
            TF(tf_linear_groups_f32(X[i], X2[i], d, ng, M, K, T, s));
        };
        // ---- bit identity on set 0
        separate(0);
        grouped(0);
        CK(hipStreamSynchronize(s));
        long long differ = 0, touched = 0;
        for (int g = 0; g < ng; ++g) {
            std::vector<unsigned> a((size_t)M * widths[g]), b((size_t)(M + guard) * widths[g]);
            CK(hipMemcpy(a.data(), Yr[0][g], a.size() * 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(b.data(), Yg[0][g], b.size() * 4, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < a.size(); ++k) differ += a[k] != b[k];
            for (size_t k = a.size(); k < b.size(); ++k) touched += b[k] != 0xFFFFFFFFu;
        }
        bad += differ + touched;
        // ---- timing: graphs of `sets` launches on rotating buffers, alternating rounds
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
        hipGraphExec_t gs = capture(separate), gg = capture(grouped);
        auto replay = [&](hipGraphExec_t ge) {
            CK(hipEventRecord(e0, s));
            CK(hipGraphLaunch(ge, s));
            CK(hipEventRecord(e1, s));
            CK(hipStreamSynchronize(s));
            float ms = 0.f;
            CK(hipEventElapsedTime(&ms, e0, e1));
            return ms * 1000.0 / sets;
        };
        replay(gs);   // warm-up (code objects, the graphs' first launch)
        replay(gg);
        std::vector<double> ts, tg;
        for (int r = 0; r < rounds; ++r) {
            ts.push_back(replay(gs));
            tg.push_back(replay(gg));
        }
        CK(hipGraphExecDestroy(gs));
        CK(hipGraphExecDestroy(gg));
        const Stat a = stat_of(ts), b = stat_of(tg);
        const double mb = (double)M * K * 4e-6 * (1 + (std::count(adds.begin(), adds.end(), 1) ? 1 : 0)) + out_mb;
        printf("{\"shape\": \"%s\", \"M\": %d, \"terms\": %d, \"groups\": %d, \"rounds\": %d, \"sets\": %d, \"differ\": %lld, \"written_behind_M\": %lld, "
               "\"separate_us\": {\"median\": %.2f, \"min\": %.2f, \"max\": %.2f}, \"grouped_us\": {\"median\": %.2f, \"min\": %.2f, \"max\": %.2f}, "
               "\"grouped_wins\": %s, \"algorithmic_MB\": %.1f, \"grouped_GBps\": %.0f}\n",
               name, M, T, ng, rounds, sets, differ, touched, a.med, a.lo, a.hi, b.med, b.lo, b.hi, b.med < a.lo ? "true" : "false", mb,
               mb / b.med * 1e3);
        fflush(stdout);
        for (int i = 0; i < sets; ++i)
            for (int g = 0; g < ng; ++g) {
                CK(hipFree(Yr[i][g]));
                CK(hipFree(Yg[i][g]));
            }
    };
    run_shape("enc_value256_query384add", {256, 384}, {0, 1});
    run_shape("dec_6x_value256", {256, 256, 256, 256, 256, 256}, {0, 0, 0, 0, 0, 0});
    return bad ? 1 : 0;
}
