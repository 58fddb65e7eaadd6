// trackformer_amd/csrc/msda_fused_bwd.h -- the two kernels that make the fused entry (tf_msda_forward_fused_f32) trainable:
//   msda_fused_prologue<f32>      qproj, reference points -> loc [N, Lq, M, L, P, 2], attn [N, Lq, M, L, P]
//   msda_fused_bwd_epilogue<f32>  grad_loc, grad_attn     -> the offset and logit columns of grad_qproj, grad_ref
// (tf_msda_fused_prologue_f32 / tf_msda_fused_backward_epilogue_f32, include/tf_msda.h).  Included from msda_hip.hip inside its
// anonymous namespace, behind backward_det_impl: it uses that file's is_aligned / note_kernel and launch_status.h's record_hip.
//
// Between the two runs the operator's own backward (tf_msda_backward_* or tf_msda_backward_det_*) on the prologue's loc / attn,
// so autograd keeps value, the reference points and qproj only and the backward never walks an element-wise ATen chain.
//
// Both kernels: a workgroup owns a run of `rows` consecutive (n, q) rows, every work-item walks the rows' M L P samples in
// steps of the workgroup size (consecutive work-items touch consecutive floats of a row: coalesced loads and stores), and what
// a reduction needs lies in LDS between two barriers.  No atomic of any kind, no cross-lane operation; every output element is
// written exactly once by a plain vector store; every sum runs in index order (the head's L P samples for the softmax and its
// gradient, (m, p) for grad_ref), so the results are a function of the tensor contents and the dimensions alone.  `rows` only
// decides which workgroup computes a row, not how.
// The epilogue recomputes each sample's location (fused_location, msda_point.h: the prologue's own arithmetic) for the range
// test only.
#ifndef TF_MSDA_FUSED_BWD_H_
#define TF_MSDA_FUSED_BWD_H_

constexpr int kFusedRowElems = 2048;        // samples a workgroup aims for (rows = kFusedRowElems / (M L P), at least 1)
constexpr int kFusedMaxRowSamples = 2048;   // M L P of one row: 7 floats per sample in LDS (epilogue) stay below 64 KB

struct FusedBwdArgs {
    const float *ref;      // [N * Lq, L, ref_dim]
    const float *qproj;    // [N * Lq, ld]
    int ref_dim, ld, off_col, logit_col;
    int M, L, P;
    long long nrows;       // N * Lq
    int rows;              // rows per workgroup
};

// H_l | W_l as floats (the divisors of the 2-d location formula: x over H_l, y over W_l, as the reference module writes it)
struct FusedLevels {
    float hw[2 * TF_MSDA_MAX_LEVELS];
};

__global__ void __launch_bounds__(kThreads)
msda_fused_prologue_kernel(const FusedBwdArgs fa, const FusedLevels lv, float *__restrict__ loc, float *__restrict__ attn)
{
#pragma clang fp contract(off)   // the operation order of the module's formulas, on the device and under the emulator alike
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int LP = fa.L * fa.P, MLP = fa.M * LP;
    float *s_z = reinterpret_cast<float *>(smem);   // [rows, M L P]  the logits
    float *s_e = s_z + (size_t)fa.rows * MLP;       //                exp(z - max of the head)
    const long long row0 = (long long)blockIdx.x * fa.rows;
    const int nr = (int)min((long long)fa.rows, fa.nrows - row0);
    const int total = nr * MLP;
    const float inv_p = 1.f / (float)fa.P;   // P is a power of two: exact

    for (int i = threadIdx.x; i < total; i += kThreads) {
        const int r = i / MLP, j = i - r * MLP;          // j = (m, l, p)
        const int l = (j % LP) / fa.P;
        const long long row = row0 + r;
        const float *qr = fa.qproj + row * fa.ld;
        const float2 off = *reinterpret_cast<const float2 *>(qr + fa.off_col + 2 * j);
        const float *rp = fa.ref + (row * fa.L + l) * fa.ref_dim;
        const float2 xy = fused_location(rp, fa.ref_dim, off, lv.hw[2 * l], lv.hw[2 * l + 1], inv_p);
        *reinterpret_cast<float2 *>(loc + (row * MLP + j) * 2) = xy;
        s_z[i] = qr[fa.logit_col + j];
    }
    __syncthreads();
    // softmax over the head's L P logits: every work-item of a head walks the same LDS words in the same order
    for (int i = threadIdx.x; i < total; i += kThreads) {
        const float *z = s_z + (i / LP) * LP;
        float mx = z[0];
        for (int t = 1; t < LP; ++t) mx = fmaxf(mx, z[t]);
        s_e[i] = __expf(s_z[i] - mx);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < total; i += kThreads) {
        const float *e = s_e + (i / LP) * LP;
        float sum = 0.f;
        for (int t = 0; t < LP; ++t) sum += e[t];
        attn[row0 * MLP + i] = s_e[i] / sum;
    }
}

__global__ void __launch_bounds__(kThreads)
msda_fused_bwd_epilogue_kernel(const FusedBwdArgs fa, const FusedLevels lv, const float *__restrict__ attn,
                               const float *__restrict__ grad_loc, const float *__restrict__ grad_attn,
                               float *__restrict__ grad_qproj, int ld_g, int goff_col, int glogit_col,
                               float *__restrict__ grad_ref)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int LP = fa.L * fa.P, MLP = fa.M * LP;
    const long long row0 = (long long)blockIdx.x * fa.rows;
    const int nr = (int)min((long long)fa.rows, fa.nrows - row0);
    const int total = nr * MLP;
    float *s_a = reinterpret_cast<float *>(smem);          // [rows, M L P]  attention weights
    float *s_g = s_a + (size_t)fa.rows * MLP;              //                their gradients
    float *s_p = s_g + (size_t)fa.rows * MLP;              //                a g
    // (the float2 arrays start at an even float count: 8-byte aligned also when rows M L P is odd)
    float2 *s_gl = reinterpret_cast<float2 *>(s_a + ((3 * (size_t)fa.rows * MLP + 1) & ~(size_t)1));   // [rows, M L P] grad_loc (grad_ref only)
    float2 *s_glo = s_gl + (size_t)fa.rows * MLP;          //                grad_loc * offset             (4-d grad_ref only)
    const float half_inv_p = 0.5f / (float)fa.P;           // exact
    const float inv_p = 1.f / (float)fa.P;
    const bool want_ref = grad_ref != nullptr;

    for (int i = threadIdx.x; i < total; i += kThreads) {
        const int r = i / MLP, j = i - r * MLP;
        const int l = (j % LP) / fa.P;
        const long long row = row0 + r;
        // A sample out of range takes no part in the forward: its gradients are zero, whatever the operator backward left there (its
        // kernels form grad_out times zeroed corners: 0, but NaN under a NaN in grad_out).  The test is the operator kernels' own
        // (pixel_point: one fma per coordinate) on the prologue's own location, so for finite gradients nothing changes.
        const float hl = lv.hw[2 * l], wl = lv.hw[2 * l + 1];
        const float *rp = fa.ref + (row * fa.L + l) * fa.ref_dim;
        const float2 off = *reinterpret_cast<const float2 *>(fa.qproj + row * fa.ld + fa.off_col + 2 * j);
        const float2 xy = fused_location(rp, fa.ref_dim, off, hl, wl, inv_p);
        const bool in = pixel_point(xy.x, xy.y, wl, hl, true).in;
        const float a = attn[row0 * MLP + i], g = in ? grad_attn[row0 * MLP + i] : 0.f;
        s_a[i] = a;
        s_g[i] = g;
        s_p[i] = a * g;
        float2 gl = *reinterpret_cast<const float2 *>(grad_loc + (row0 * MLP + i) * 2);
        if (!in) gl = make_float2(0.f, 0.f);
        float2 go;
        if (fa.ref_dim == 2) {
            go.x = gl.x / hl;
            go.y = gl.y / wl;
        } else {
            go.x = gl.x * rp[2] * half_inv_p;
            go.y = gl.y * rp[3] * half_inv_p;
            if (want_ref) s_glo[i] = make_float2(gl.x * off.x, gl.y * off.y);
        }
        if (want_ref) s_gl[i] = gl;
        *reinterpret_cast<float2 *>(grad_qproj + row * ld_g + goff_col + 2 * j) = go;
    }
    __syncthreads();
    // grad_logit_i = a_i (g_i - sum_j a_j g_j), j over the head in index order
    for (int i = threadIdx.x; i < total; i += kThreads) {
        const int r = i / MLP, j = i - r * MLP;
        const float *p = s_p + (i / LP) * LP;
        float dot = 0.f;
        for (int t = 0; t < LP; ++t) dot += p[t];
        grad_qproj[(row0 + r) * ld_g + glogit_col + j] = s_a[i] * (s_g[i] - dot);
    }
    if (!want_ref) return;
    // grad_ref[n, q, l, c] = sum_{m, p} grad_loc[.., c]  (c < 2),  sum_{m, p} grad_loc * off * 0.5 / P  (c >= 2), (m, p) in index order
    const int per_row = fa.L * fa.ref_dim;
    for (int i = threadIdx.x; i < nr * per_row; i += kThreads) {
        const int r = i / per_row, k = i - r * per_row;
        const int l = k / fa.ref_dim, c = k - l * fa.ref_dim;
        const float *src = reinterpret_cast<const float *>(c < 2 ? s_gl : s_glo) + (size_t)r * MLP * 2 + (c & 1);
        float sum = 0.f;
        for (int m = 0; m < fa.M; ++m)
            for (int p = 0; p < fa.P; ++p) sum += src[((m * fa.L + l) * fa.P + p) * 2];
        grad_ref[(row0 + r) * per_row + k] = c < 2 ? sum : sum * half_inv_p;
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// The argument contract both entries share with forward_fused_impl; fills the kernel arguments and the level divisors.
int fused_bwd_args(const float *ref, int ref_dim, const float *qproj, int ld, int off_col, int logit_col,
                   const int64_t *shapes_host, int N, int M, int L, int Lq, int P, FusedBwdArgs *fa, FusedLevels *lv)
{
    if (N <= 0 || M <= 0 || L <= 0 || Lq <= 0 || P <= 0 || L > TF_MSDA_MAX_LEVELS || (ref_dim != 2 && ref_dim != 4))
        return TF_MSDA_ERR_BAD_DIMS;
    if (P != 1 && P != 2 && P != 4 && P != 8) return TF_MSDA_ERR_BAD_DIMS;
    const long long mlp = (long long)M * L * P;
    if (mlp > kFusedMaxRowSamples) return TF_MSDA_ERR_BAD_DIMS;
    if (off_col < 0 || logit_col < 0 || (off_col & 1) || (ld & 1) || ld < off_col + 2 * mlp || ld < logit_col + mlp)
        return TF_MSDA_ERR_BAD_DIMS;
    const long long nrows = (long long)N * Lq;
    if (nrows * (ld > 2 * mlp ? ld : 2 * mlp) * 4 >= (1ll << 32)) return TF_MSDA_ERR_BAD_DIMS;   // tensors below 4 GiB
    if (!is_aligned(qproj, 8)) return TF_MSDA_ERR_BAD_DIMS;
    for (int l = 0; l < 2 * TF_MSDA_MAX_LEVELS; ++l) lv->hw[l] = 1.f;
    for (int l = 0; l < L; ++l) {
        const int64_t h = shapes_host[2 * l], w = shapes_host[2 * l + 1];
        if (h <= 0 || w <= 0 || h > INT32_MAX || w > INT32_MAX) return TF_MSDA_ERR_BAD_DIMS;
        lv->hw[2 * l] = (float)h;
        lv->hw[2 * l + 1] = (float)w;
    }
    int rows = (int)(kFusedRowElems / mlp);
    if (rows < 1) rows = 1;
    if (rows > nrows) rows = (int)nrows;
    *fa = FusedBwdArgs{ref, qproj, ref_dim, ld, off_col, logit_col, M, L, P, nrows, rows};
    return TF_MSDA_OK;
}

int fused_prologue_impl(const float *ref, int ref_dim, const float *qproj, int ld, int off_col, int logit_col,
                        const int64_t *shapes_host, float *loc, float *attn, int N, int M, int L, int Lq, int P, void *stream_v)
{
    if (!ref || !qproj || !shapes_host || !loc || !attn) return TF_MSDA_ERR_NULL_POINTER;
    FusedBwdArgs fa;
    FusedLevels lv;
    const int rc = fused_bwd_args(ref, ref_dim, qproj, ld, off_col, logit_col, shapes_host, N, M, L, Lq, P, &fa, &lv);
    if (rc != TF_MSDA_OK) return rc;
    if (!is_aligned(loc, 8)) return TF_MSDA_ERR_BAD_DIMS;
    const size_t lds = (size_t)fa.rows * M * L * P * sizeof(float) * 2;
    const unsigned grid = (unsigned)((fa.nrows + fa.rows - 1) / fa.rows);
    hipLaunchKernelGGL(msda_fused_prologue_kernel, dim3(grid), dim3(kThreads), lds, static_cast<hipStream_t>(stream_v), fa, lv,
                       loc, attn);
    note_kernel("msda_fused_prologue<f32>");
    return record_hip(hipGetLastError());
}

int fused_bwd_epilogue_impl(const float *ref, int ref_dim, const float *qproj, int ld, int off_col, int logit_col,
                            const int64_t *shapes_host, const float *attn, const float *grad_loc, const float *grad_attn,
                            float *grad_qproj, int ld_g, int goff_col, int glogit_col, float *grad_ref, int N, int M, int L,
                            int Lq, int P, void *stream_v)
{
    if (!ref || !qproj || !shapes_host || !attn || !grad_loc || !grad_attn || !grad_qproj) return TF_MSDA_ERR_NULL_POINTER;
    FusedBwdArgs fa;
    FusedLevels lv;
    const int rc = fused_bwd_args(ref, ref_dim, qproj, ld, off_col, logit_col, shapes_host, N, M, L, Lq, P, &fa, &lv);
    if (rc != TF_MSDA_OK) return rc;
    const long long mlp = (long long)M * L * P;
    if (goff_col < 0 || glogit_col < 0 || (goff_col & 1) || (ld_g & 1) || ld_g < goff_col + 2 * mlp || ld_g < glogit_col + mlp ||
        fa.nrows * ld_g * 4 >= (1ll << 32))
        return TF_MSDA_ERR_BAD_DIMS;
    // the two column ranges of a grad_qproj row must not overlap: every element is written once
    if (goff_col < glogit_col + mlp && glogit_col < goff_col + 2 * mlp) return TF_MSDA_ERR_BAD_DIMS;
    if (!is_aligned(grad_qproj, 8) || !is_aligned(grad_loc, 8)) return TF_MSDA_ERR_BAD_DIMS;
    // a g | grad_loc | grad_loc * off: 3 + 2 + 2 floats per sample; without grad_ref the last four are never touched
    const size_t nf = (3 * (size_t)fa.rows * mlp + 1) & ~(size_t)1;   // the float arrays, rounded up to an even count
    const size_t lds = (nf + (size_t)fa.rows * mlp * (grad_ref ? (ref_dim == 4 ? 4 : 2) : 0)) * sizeof(float);
    const unsigned grid = (unsigned)((fa.nrows + fa.rows - 1) / fa.rows);
    hipLaunchKernelGGL(msda_fused_bwd_epilogue_kernel, dim3(grid), dim3(kThreads), lds, static_cast<hipStream_t>(stream_v), fa,
                       lv, attn, grad_loc, grad_attn, grad_qproj, ld_g, goff_col, glogit_col, grad_ref);
    note_kernel("msda_fused_bwd_epilogue<f32>");
    return record_hip(hipGetLastError());
}

#endif  // TF_MSDA_FUSED_BWD_H_
