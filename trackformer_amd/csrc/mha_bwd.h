// trackformer_amd/csrc/mha_bwd.h -- the training path of the attention core (included at the end of mha_core.hip; include/tf_fused.h:
// TRAINING THROUGH THE ATTENTION CORE states the contract): tf_mha_core_train_f32 launches mha_mfma_stream_kernel<D, NB, true> (mha_core.hip:
// the inference kernel plus the rows' statistics and the dropout of the weights), tf_mha_core_bwd_f32 the kernel below.
//
//   P_ij = 2^(c s_ij - m_i) inv_i  (c = scale log2 e; m_i, inv_i = stats of row i),   Pd = keep s_p P,   dP = dout V^T,
//   delta_i = sum_c dout_ic out_ic,   dS = P (keep s_p dP - delta),   dq = scale dS K,   dk = scale dS^T Q,   dv = Pd^T dout
//
// ONE launch, two kinds of workgroup (256 threads, four waves), nothing stored of size L x L and no workspace:
//   * blockIdx.x < ceil(Lq / 16): owns 16 QUERIES and writes their dq.  Wave w walks the key tiles w, w + 4, ...  The score tile is formed
//     TRANSPOSED (A = K, B = Q: column = query, rows = keys), so the accumulator a lane ends up with -- query lane % 16, keys
//     16 t + 4 (lane / 16) + 0 .. 3 -- is one Philox group of the mask contract AND the A operand of the four steps of dS K: no exchange
//     through LDS between the products.
//   * the others own 16 KEYS and write their dk and dv.  Wave w walks the query tiles w, w + 4, ...; the tile is formed as in the forward
//     (A = Q, B = K: column = key, rows = queries), which is the A operand of dS^T Q and Pd^T dout.  A lane's four elements lie in four
//     rows here: lane 4 a + b of a 16-lane group computes the group of row b, keys 4 a .. + 3, and the quad exchanges the bits.
//   Both recompute delta (D multiply-adds per row, in one order: row_delta) instead of depending on each other.
// The four waves' partial sums meet in LDS and are added in wave order; a wave adds its tiles in ascending order: every sum runs in an
// order that is a function of (Lq, Lk) alone, every output element is written once, no atomics.
// Dead elements are SELECTED to zero, never multiplied: a masked key, a key or query behind the end, a row without keys (inv = 0).  The
// rows of dout that belong to a row without keys enter dv as zeros, and dq / dk / dv of dead rows / keys are stored as +0.
#ifndef TF_MHA_BWD_H_
#define TF_MHA_BWD_H_

namespace {

struct MhaBwdArgs {
    const float *dout, *q, *k, *v, *out, *stats;
    const unsigned char *key_mask;
    const long long *rng;
    float *dq, *dk, *dv;
    int Lq, Lk, lddo, ldq, ldk, ldv, ldo, lddq, lddk, lddv;
    float scale, drop_scale;
    unsigned drop_T;
};

template <int D>
struct MhaOps {
    static constexpr int G16 = D / 16, TAIL = (D % 16) / 4, VW = G16, XT = TAIL > 0 ? 1 : 0, NW = THREADS / 64;
    typedef float vrow_t __attribute__((ext_vector_type(VW)));
    // a row in the order of the score products: channels 16 t + 4 kq .. + 3, then one channel 16 G16 + 4 t + kq per tail step
    struct Score {
        f32x4m_t a[G16];
        float t[TAIL > 0 ? TAIL : 1];
    };
    // four consecutive rows in the order of the output products: channels VW m16 .. + VW - 1 (+ channel 16 G16 + m16 of the extra tile)
    struct Rows {
        vrow_t main[4];
        float extra[4];
    };

    static __device__ __forceinline__ Score load_score(const float *__restrict__ row, int kq)
    {
        Score s;
#pragma unroll
        for (int t = 0; t < G16; ++t) s.a[t] = *reinterpret_cast<const f32x4m_t *>(row + 16 * t + 4 * kq);
#pragma unroll
        for (int t = 0; t < TAIL; ++t) s.t[t] = row[16 * G16 + 4 * t + kq];
        if constexpr (TAIL == 0) s.t[0] = 0.f;
        return s;
    }
    // rows j0 .. j0 + 3 of a head (base: row 0 of the head); rows behind the last (L) count as zero and are read from the last one
    static __device__ __forceinline__ Rows load_rows(const float *__restrict__ base, int ld, int j0, int L, int m16)
    {
        Rows r;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = j0 + s;
            const float *row = base + (size_t)min(j, L - 1) * ld;
            vrow_t x = *reinterpret_cast<const vrow_t *>(row + VW * m16);
            if (j >= L) x = vrow_t(0.f);
            r.main[s] = x;
            r.extra[s] = 0.f;
            if constexpr (XT) r.extra[s] = (m16 < 4 * TAIL && j < L) ? row[16 * G16 + m16] : 0.f;
        }
        return r;
    }
    // C[i][j] = sum_c a_i[c] b_j[c]: column (lane % 16) = the row b was loaded for, rows 4 (lane / 16) + 0 .. 3 = those of a
    static __device__ __forceinline__ f32x4m_t score(const Score &a, const Score &b)
    {
        f32x4m_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < G16; ++t) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.a[t].x, b.a[t].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.a[t].y, b.a[t].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.a[t].z, b.a[t].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.a[t].w, b.a[t].w, acc, 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < TAIL; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.t[t], b.t[t], acc, 0, 0, 0);
        return acc;
    }
    // o[c] += sum_s a[s] (x) rows[s]: output row = the lane's a, column m16 = channel VW m16 + c (tile VW: channel 16 G16 + m16)
    static __device__ __forceinline__ void accumulate(f32x4m_t (&o)[VW + XT], const f32x4m_t &a, const Rows &b)
    {
#pragma unroll
        for (int c = 0; c < VW; ++c) {
            o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.main[0][c], o[c], 0, 0, 0);
            o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.main[1][c], o[c], 0, 0, 0);
            o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.main[2][c], o[c], 0, 0, 0);
            o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.main[3][c], o[c], 0, 0, 0);
        }
        if constexpr (XT) {
            o[VW] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.extra[0], o[VW], 0, 0, 0);
            o[VW] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.extra[1], o[VW], 0, 0, 0);
            o[VW] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.extra[2], o[VW], 0, 0, 0);
            o[VW] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.extra[3], o[VW], 0, 0, 0);
        }
    }
    // delta of the row both operands were loaded for: the lane's channels first, then the four lanes (lane / 16) of the row
    static __device__ __forceinline__ float row_delta(const Score &d, const Score &o)
    {
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < G16; ++t) s += (d.a[t].x * o.a[t].x + d.a[t].y * o.a[t].y) + (d.a[t].z * o.a[t].z + d.a[t].w * o.a[t].w);
#pragma unroll
        for (int t = 0; t < TAIL; ++t) s += d.t[t] * o.t[t];
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        return s;
    }
    // a wave's accumulators -> s_p[wave][row 4 kq + r][channel]
    static __device__ __forceinline__ void park(float *s_p, int wave, int m16, int kq, const f32x4m_t (&o)[VW + XT])
    {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float *dst = s_p + ((size_t)wave * TQ + 4 * kq + r) * D;
            vrow_t x;
#pragma unroll
            for (int c = 0; c < VW; ++c) x[c] = o[c][r];
            *reinterpret_cast<vrow_t *>(dst + VW * m16) = x;
            if constexpr (XT)
                if (m16 < 4 * TAIL) dst[16 * G16 + m16] = o[VW][r];
        }
    }
    // 16-byte chunk c4 of row `row` of the tile: the waves in order
    static __device__ __forceinline__ f32x4m_t gather(const float *s_p, int row, int c4)
    {
        f32x4m_t r = *reinterpret_cast<const f32x4m_t *>(s_p + (size_t)row * D + c4 * 4);
#pragma unroll
        for (int w = 1; w < NW; ++w) r += *reinterpret_cast<const f32x4m_t *>(s_p + ((size_t)w * TQ + row) * D + c4 * 4);
        return r;
    }
};

template <int D>
__global__ void __launch_bounds__(THREADS)
mha_bwd_kernel(const MhaBwdArgs a)
{
    typedef MhaOps<D> O;
    constexpr int D4 = D / 4, NW = O::NW, NT = O::VW + O::XT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *s_p = smem;                       // [NW][TQ][D] partial sums of the waves (dq, or dv)
    float *s_p2 = smem + NW * TQ * D;        // [NW][TQ][D] (dk)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.y, n = blockIdx.z, H = gridDim.y;
    const int m16 = lane & 15, kq = lane >> 4;
    const int Lq = a.Lq, Lk = a.Lk;
    const int nqt = (Lq + 15) >> 4, nkt = (Lk + 15) >> 4;
    const unsigned long long lk4q = (unsigned long long)((Lk + 3) >> 2);   // Philox groups per padded row
    const float c2 = a.scale * 1.44269504088896340736f;
    const float *qh = a.q + (size_t)n * Lq * a.ldq + h * D, *doh = a.dout + (size_t)n * Lq * a.lddo + h * D;
    const float *oh = a.out + (size_t)n * Lq * a.ldo + h * D;
    const float *kh = a.k + (size_t)n * Lk * a.ldk + h * D, *vh = a.v + (size_t)n * Lk * a.ldv + h * D;
    const float *sth = a.stats + 2 * ((size_t)n * H + h) * Lq;
    const unsigned char *mk = a.key_mask != nullptr ? a.key_mask + (size_t)n * Lk : nullptr;
    const unsigned long long row0 = ((unsigned long long)n * H + h) * Lq;
    const bool drop = a.rng != nullptr;
    tfd::Stream st = {0u, 0u, 0u, 0u};
    if (drop) st = tfd::load_stream(a.rng);

    if ((int)blockIdx.x < nqt) {
        // ---- 16 queries: dq
        const int q0 = blockIdx.x * TQ, nq = min(TQ, Lq - q0);
        const int qi = min(q0 + m16, Lq - 1);
        const typename O::Score Qb = O::load_score(qh + (size_t)qi * a.ldq, kq), dOb = O::load_score(doh + (size_t)qi * a.lddo, kq);
        const float delta = O::row_delta(dOb, O::load_score(oh + (size_t)qi * a.ldo, kq));
        const float m2 = sth[2 * qi], inv = sth[2 * qi + 1];
        const bool rowlive = inv > 0.f && q0 + m16 < Lq;
        const unsigned long long grow = (row0 + qi) * lk4q;
        f32x4m_t o[NT];
#pragma unroll
        for (int c = 0; c < NT; ++c) o[c] = f32x4m_t{0.f, 0.f, 0.f, 0.f};
        for (int t16 = wave; t16 < nkt; t16 += NW) {   // wave-uniform
            const int jr = min(16 * t16 + m16, Lk - 1);
            const typename O::Score Ka = O::load_score(kh + (size_t)jr * a.ldk, kq), Va = O::load_score(vh + (size_t)jr * a.ldv, kq);
            const typename O::Rows Kr = O::load_rows(kh, a.ldk, 16 * t16 + 4 * kq, Lk, m16);
            const f32x4m_t s = O::score(Ka, Qb), dp = O::score(Va, dOb);   // column = query m16, rows = keys 16 t16 + 4 kq + r
            unsigned bits = 15u;
            if (drop) bits = tfd::keep_bits(st, grow + (unsigned long long)(4 * t16 + kq), a.drop_T);
            f32x4m_t ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 16 * t16 + 4 * kq + r;
                const bool live = rowlive && j < Lk && !(mk != nullptr && mk[min(j, Lk - 1)]);
                const float p = exp2f(s[r] * c2 - m2) * inv;
                const float g = ((bits >> r) & 1u) ? dp[r] * a.drop_scale : 0.f;
                ds[r] = live ? p * (g - delta) : 0.f;
            }
            O::accumulate(o, ds, Kr);
        }
        O::park(s_p, wave, m16, kq, o);
        __syncthreads();
        for (int i = tid; i < TQ * D4; i += THREADS) {
            const int r = i / D4, c4 = i - r * D4;
            if (r < nq) {
                f32x4m_t x = O::gather(s_p, r, c4) * a.scale;
                if (!(sth[2 * (q0 + r) + 1] > 0.f)) x = f32x4m_t{0.f, 0.f, 0.f, 0.f};   // a row without keys
                *reinterpret_cast<f32x4m_t *>(a.dq + ((size_t)n * Lq + q0 + r) * a.lddq + h * D + c4 * 4) = x;
            }
        }
        return;
    }
    // ---- 16 keys: dk and dv
    const int kt = (int)blockIdx.x - nqt, j0 = kt * TQ, nk = min(TQ, Lk - j0);
    const int jr = min(j0 + m16, Lk - 1);
    const typename O::Score Kb = O::load_score(kh + (size_t)jr * a.ldk, kq), Vb = O::load_score(vh + (size_t)jr * a.ldv, kq);
    const bool keylive = j0 + m16 < Lk && !(mk != nullptr && mk[jr]);
    f32x4m_t ov[NT], ok[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) ov[c] = ok[c] = f32x4m_t{0.f, 0.f, 0.f, 0.f};
    for (int g = wave; g < nqt; g += NW) {   // wave-uniform
        const int qi = min(16 * g + m16, Lq - 1);
        const typename O::Score Qa = O::load_score(qh + (size_t)qi * a.ldq, kq), dOa = O::load_score(doh + (size_t)qi * a.lddo, kq);
        const float delta_m = O::row_delta(dOa, O::load_score(oh + (size_t)qi * a.ldo, kq));   // of query 16 g + m16
        const typename O::Rows Qr = O::load_rows(qh, a.ldq, 16 * g + 4 * kq, Lq, m16);
        typename O::Rows dOr = O::load_rows(doh, a.lddo, 16 * g + 4 * kq, Lq, m16);
        const f32x4m_t s = O::score(Qa, Kb), dp = O::score(dOa, Vb);   // column = key m16, rows = queries 16 g + 4 kq + r
        unsigned mine = 15u;   // lane 4 a + b of a row group: the decisions of query 16 g + 4 kq + b, keys j0 + 4 a .. + 3
        if (drop)
            mine = tfd::keep_bits(st, (row0 + min(16 * g + 4 * kq + (m16 & 3), Lq - 1)) * lk4q + (unsigned long long)(4 * kt + (m16 >> 2)),
                                  a.drop_T);
        f32x4m_t pd, ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * g + 4 * kq + r, ic = min(i, Lq - 1);
            const float m2 = sth[2 * ic], inv = sth[2 * ic + 1];
            const float delta = __shfl(delta_m, 4 * kq + r);
            const unsigned bits = (unsigned)__shfl((int)mine, (lane & ~3) | r);
            const bool keep = (bits >> (m16 & 3)) & 1u;
            const bool rowlive = i < Lq && inv > 0.f;
            const bool live = keylive && rowlive;
            const float p = exp2f(s[r] * c2 - m2) * inv;
            pd[r] = (live && keep) ? p * a.drop_scale : 0.f;
            ds[r] = live ? p * ((keep ? dp[r] * a.drop_scale : 0.f) - delta) : 0.f;
            if (!rowlive) {   // a row without keys: whatever its dout holds stays out of dv
                dOr.main[r] = typename O::vrow_t(0.f);
                dOr.extra[r] = 0.f;
            }
        }
        O::accumulate(ov, pd, dOr);
        O::accumulate(ok, ds, Qr);
    }
    O::park(s_p, wave, m16, kq, ov);
    O::park(s_p2, wave, m16, kq, ok);
    __syncthreads();
    for (int i = tid; i < TQ * D4; i += THREADS) {
        const int r = i / D4, c4 = i - r * D4;
        if (r < nk) {
            f32x4m_t xv = O::gather(s_p, r, c4), xk = O::gather(s_p2, r, c4) * a.scale;
            if (mk != nullptr && mk[j0 + r]) xv = xk = f32x4m_t{0.f, 0.f, 0.f, 0.f};   // a masked key
            *reinterpret_cast<f32x4m_t *>(a.dv + ((size_t)n * Lk + j0 + r) * a.lddv + h * D + c4 * 4) = xv;
            *reinterpret_cast<f32x4m_t *>(a.dk + ((size_t)n * Lk + j0 + r) * a.lddk + h * D + c4 * 4) = xk;
        }
    }
}

inline bool mha_train_dims_ok(int N, int Lq, int Lk, int H, int D)
{
    return N > 0 && N <= 65535 && H > 0 && H <= 65535 && Lq > 0 && Lq <= 1024 && Lk > 0 && Lk <= 1024 && (D == 32 || D == 36);
}
inline bool mha_aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int tf_mha_core_train_f32(const float *q, const float *k, const float *v, float *out, const unsigned char *key_mask, float *stats,
                                     const int64_t *rng, float p, int N, int Lq, int Lk, int H, int D, int ldq, int ldk, int ldv, int ldo,
                                     float scale, void *stream)
{
    if (!q || !k || !v || !out || !stats) return TF_MSDA_ERR_NULL_POINTER;
    if (rng && !tfd::dropout_p_ok(p)) return TF_MSDA_ERR_BAD_DIMS;
    if (!mha_train_dims_ok(N, Lq, Lk, H, D)) return TF_MSDA_ERR_BAD_DIMS;
    if (((ldq | ldk | ldv | ldo) & 3) || ldq < H * D || ldk < H * D || ldv < H * D || ldo < H * D) return TF_MSDA_ERR_BAD_DIMS;
    if (!mha_aligned(q, 16) || !mha_aligned(k, 16) || !mha_aligned(v, 16) || !mha_aligned(out, 16) || !mha_aligned(stats, 8) ||
        !mha_aligned(rng, 8))
        return TF_MSDA_ERR_BAD_DIMS;
    // the launch of tf_mha_core_f32's default kernel (mha_mfma = 1), whatever that option holds
    const int lkp = ((Lk + 15) & ~15) + 4;
    const int per_batch = 16 * (THREADS / 64) * 8;
    const size_t lds = ((size_t)TQ * lkp + 2 * (THREADS / 64) * TQ + (size_t)(THREADS / 64) * TQ * D) * sizeof(float);
    const bool one = Lk <= per_batch;
    const void *fn = D == 32 ? (one ? (const void *)&mha_mfma_stream_kernel<32, 1, true> : (const void *)&mha_mfma_stream_kernel<32, 2, true>)
                             : (one ? (const void *)&mha_mfma_stream_kernel<36, 1, true> : (const void *)&mha_mfma_stream_kernel<36, 2, true>);
    if (lds > 64 * 1024 && !tfm::raise_dynamic_lds_limit(fn)) return tfm::record_hip(hipErrorInvalidValue);
    const long long *rngp = reinterpret_cast<const long long *>(rng);
    unsigned T = rng ? tfd::dropout_threshold(p) : 0u;
    float sp = rng ? tfd::dropout_scale(p) : 1.f;
    const dim3 grid((unsigned)((Lq + TQ - 1) / TQ), (unsigned)H, (unsigned)N);
    void *args[] = {(void *)&q, (void *)&k, (void *)&v, (void *)&out, (void *)&key_mask, (void *)&Lq, (void *)&Lk, (void *)&ldq, (void *)&ldk,
                    (void *)&ldv, (void *)&ldo, (void *)&scale, (void *)&lkp, (void *)&stats, (void *)&rngp, (void *)&T, (void *)&sp};
    return tfm::record_hip(hipLaunchKernel(fn, grid, dim3(THREADS), args, lds, static_cast<hipStream_t>(stream)));
}

extern "C" int tf_mha_core_bwd_f32(const float *dout, const float *q, const float *k, const float *v, const float *out, const float *stats,
                                   const unsigned char *key_mask, const int64_t *rng, float p, float *dq, float *dk, float *dv, int N, int Lq,
                                   int Lk, int H, int D, int lddo, int ldq, int ldk, int ldv, int ldo, int lddq, int lddk, int lddv, float scale,
                                   void *stream)
{
    if (!dout || !q || !k || !v || !out || !stats || !dq || !dk || !dv) return TF_MSDA_ERR_NULL_POINTER;
    if (rng && !tfd::dropout_p_ok(p)) return TF_MSDA_ERR_BAD_DIMS;
    if (!mha_train_dims_ok(N, Lq, Lk, H, D)) return TF_MSDA_ERR_BAD_DIMS;
    const int lds_[] = {lddo, ldq, ldk, ldv, ldo, lddq, lddk, lddv};
    for (int ld : lds_)
        if ((ld & 3) || ld < H * D) return TF_MSDA_ERR_BAD_DIMS;
    const void *ptrs[] = {dout, q, k, v, out, dq, dk, dv};
    for (const void *ptr : ptrs)
        if (!mha_aligned(ptr, 16)) return TF_MSDA_ERR_BAD_DIMS;
    if (!mha_aligned(stats, 8) || !mha_aligned(rng, 8)) return TF_MSDA_ERR_BAD_DIMS;
    MhaBwdArgs a;
    a.dout = dout, a.q = q, a.k = k, a.v = v, a.out = out, a.stats = stats;
    a.key_mask = key_mask;
    a.rng = reinterpret_cast<const long long *>(rng);
    a.dq = dq, a.dk = dk, a.dv = dv;
    a.Lq = Lq, a.Lk = Lk, a.lddo = lddo, a.ldq = ldq, a.ldk = ldk, a.ldv = ldv, a.ldo = ldo, a.lddq = lddq, a.lddk = lddk, a.lddv = lddv;
    a.scale = scale;
    a.drop_scale = rng ? tfd::dropout_scale(p) : 1.f;
    a.drop_T = rng ? tfd::dropout_threshold(p) : 0u;
    const void *fn = D == 32 ? (const void *)&mha_bwd_kernel<32> : (const void *)&mha_bwd_kernel<36>;
    const size_t lds = (size_t)2 * (THREADS / 64) * TQ * D * sizeof(float);
    const dim3 grid((unsigned)((Lq + TQ - 1) / TQ + (Lk + TQ - 1) / TQ), (unsigned)H, (unsigned)N);
    void *args[] = {(void *)&a};
    return tfm::record_hip(hipLaunchKernel(fn, grid, dim3(THREADS), args, lds, static_cast<hipStream_t>(stream)));
}

#endif /* TF_MHA_BWD_H_ */
