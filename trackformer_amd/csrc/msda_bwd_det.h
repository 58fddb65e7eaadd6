// trackformer_amd/csrc/msda_bwd_det.h -- msda_bwd_det<T>: the bitwise-reproducible MSDeformAttn backward
// (tf_msda_backward_det_*, include/tf_msda.h).  Included from msda_hip.hip inside its anonymous namespace, behind
// backward_impl: it uses that file's fill_level_table / build_level_table, launch_status.h's record_hip and msda_point.h's Tap / make_tap.
//
// The default backward kernels scatter grad_value with float atomics, whose summation order is whatever the memory system
// makes of it.  Here no float atomic appears anywhere: every contribution is stored once, the contributions of one
// (batch, head) block are put in destination-row order by a STABLE sort, and every row of grad_value is summed in that fixed
// order and written once by plain stores (rows nobody samples get +0: there is no zero-fill pass).
//
//   emit     one work-item per sample (n, m, q, l, p), items laid out in exactly that order inside the (n, m) block.  Each of
//            the four corners gets a fixed slot: a 32-bit key = the destination row inside (n, m), start_l + y W_l + x (S, above
//            every row, for a corner or sample that is out of range) and the weight attn * w_c.  Nothing is compacted, so no
//            position depends on timing.  The same work-item forms grad_loc / grad_attn of its sample with a serial loop over
//            the D channels.
//   sort     LSD radix sort of each (n, m) block by key, 8 bits per pass, ceil(bits(S) / 8) passes (two at S = 22 223), moving
//            (key, slot index).  Per pass: digit histograms of 1024-item tiles (integer LDS atomics: counts do not depend on
//            order), an exclusive scan over (digit, tile), and a scatter whose ranks come from __ballot matches and running
//            counts in work-item order -- never from an atomic's return value.  A stable sort has exactly one result:
//            inside a row the list stays in (q, l, p, corner) order.
//   bounds   the first sorted position of every row (start[r], r = 0 .. S) from neighbouring sorted keys.
//   reduce   one workgroup per destination row: the list is cut BY POSITION into chunks of kDetChunk items, chunks are
//            summed separately (sum of weight * grad_out[n, q, m, :] in list order, one lane per channel) and the partial sums
//            are added in chunk order, so the order of every addition is a function of the list's length alone -- and a row
//            that collects most of the samples is summed by all the waves of its workgroup, not by one.
//
// Nothing depends on the device's CU count, on a tf_msda_set_option knob or on what the workspace held.  The batch is walked
// in chunks of whole images (a function of the dimensions only) to bound the workspace; blocks of different (n, m) never
// meet, so the gradients of image n do not depend on N, on the chunking or on the other images.
#ifndef TF_MSDA_BWD_DET_H_
#define TF_MSDA_BWD_DET_H_

constexpr int kDetWave = 64;                        // one wavefront per sort workgroup
constexpr int kDetTileRounds = 16;
constexpr int kDetTile = kDetWave * kDetTileRounds;  // items per radix tile
constexpr int kDetRadix = 256;                       // 8 bits per pass
#ifndef TF_DET_CHUNK
#define TF_DET_CHUNK 32
#endif
constexpr int kDetChunk = TF_DET_CHUNK;              // items per reduce chunk (measured: profiles/det_backward_bench.json)
constexpr int kDetReduceThreads = 256;
constexpr long long kDetBatchBudget = 512ll << 20;   // the batch chunk is the largest number of images whose workspace fits this

// ---------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kThreads)
msda_bwd_det_emit(const T *__restrict__ value, const T *__restrict__ loc, const T *__restrict__ attn,
                  const T *__restrict__ grad_out, T *__restrict__ grad_loc, T *__restrict__ grad_attn,
                  unsigned *__restrict__ keys, T *__restrict__ wts, const LevelTable lt,
                  const int64_t *__restrict__ dshapes, int S, int M, int D, int L, int Lq, int P, long long total_samples)
{
    __shared__ int s_tab[3 * TF_MSDA_MAX_LEVELS];
    fill_level_table(s_tab, lt, dshapes, L);
    __syncthreads();
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;   // (n, m, q, l, p)
    if (t >= total_samples) return;
    const int LP = L * P;
    const int lp = (int)(t % LP);
    long long r = t / LP;
    const int q = (int)(r % Lq);
    r /= Lq;
    const int m = (int)(r % M);
    const long long b = r / M;
    const int l = lp / P;
    const int H = s_tab[l], W = s_tab[TF_MSDA_MAX_LEVELS + l], start = s_tab[2 * TF_MSDA_MAX_LEVELS + l];

    const long long pair = (b * Lq + q) * M + m;
    const long long si = pair * LP + lp;
    const T a = attn[si];
    const Tap<T> tp = make_tap(loc[2 * si], loc[2 * si + 1], H, W);
    const long long pix = (long long)M * D;
    const T *vl = value + (b * S + start) * pix + (long long)m * D;
    const T *v1 = vl + (long long)tp.o1 * pix, *v2 = vl + (long long)tp.o2 * pix;
    const T *v3 = vl + (long long)tp.o3 * pix, *v4 = vl + (long long)tp.o4 * pix;
    const T *g = grad_out + pair * D;
    const T w1 = tp.gy * tp.gx, w2 = tp.gy * tp.fx, w3 = tp.fy * tp.gx, w4 = tp.fy * tp.fx;
    T dot = (T)0, dx = (T)0, dy = (T)0;
    for (int c = 0; c < D; ++c) {   // serial over the channels: one fixed order (the arithmetic of msda_bwd_rowgather)
        const T a1 = tp.k1 ? v1[c] : (T)0;
        const T a2 = tp.k2 ? v2[c] : (T)0;
        const T a3 = tp.k3 ? v3[c] : (T)0;
        const T a4 = tp.k4 ? v4[c] : (T)0;
        const T gc = g[c];
        dot = fma_t(gc, w1 * a1 + w2 * a2 + w3 * a3 + w4 * a4, dot);      // cuh:365
        dx = fma_t(gc, tp.gy * (a2 - a1) + tp.fy * (a4 - a3), dx);        // cuh:150-160
        dy = fma_t(gc, tp.gx * (a3 - a1) + tp.fx * (a4 - a2), dy);        // cuh:139-149
    }
    grad_loc[2 * si] = dx * (a * (T)W);        // cuh:371,373
    grad_loc[2 * si + 1] = dy * (a * (T)H);    // cuh:371,374
    grad_attn[si] = dot;

    const long long n_items = 4ll * Lq * LP;
    const long long slot = (b * M + m) * n_items + ((long long)q * LP + lp) * 4;
    const unsigned none = (unsigned)S;
    keys[slot + 0] = tp.k1 ? (unsigned)(start + tp.o1) : none;
    keys[slot + 1] = tp.k2 ? (unsigned)(start + tp.o2) : none;
    keys[slot + 2] = tp.k3 ? (unsigned)(start + tp.o3) : none;
    keys[slot + 3] = tp.k4 ? (unsigned)(start + tp.o4) : none;
    wts[slot + 0] = a * w1;                    // cuh:279,296-301: the contribution is (attn w_c) grad_out
    wts[slot + 1] = a * w2;
    wts[slot + 2] = a * w3;
    wts[slot + 3] = a * w4;
}

// digit counts of one tile -> hist[(block, tile)][digit]
__global__ void __launch_bounds__(kDetWave)
msda_bwd_det_hist(const unsigned *__restrict__ keys, unsigned *__restrict__ hist, long long n_items, long long tiles, int shift)
{
    __shared__ unsigned cnt[kDetRadix];
    const long long blk = blockIdx.x;
    const long long seg = blk / tiles, tile = blk - seg * tiles;
    for (int i = threadIdx.x; i < kDetRadix; i += kDetWave) cnt[i] = 0u;
    __syncthreads();
    const unsigned *k = keys + seg * n_items;
    for (int rd = 0; rd < kDetTileRounds; ++rd) {
        const long long i = tile * kDetTile + rd * kDetWave + threadIdx.x;
        if (i < n_items) atomicAdd(&cnt[(k[i] >> shift) & (kDetRadix - 1)], 1u);   // integer: the count has no order
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kDetRadix; i += kDetWave) hist[blk * kDetRadix + i] = cnt[i];
}

// exclusive scan of one block's counts in (digit, tile) order, in place: hist[(block, tile)][digit] becomes the first output
// position of that tile's items with that digit
__global__ void __launch_bounds__(kDetRadix)
msda_bwd_det_scan(unsigned *__restrict__ hist, long long tiles)
{
    __shared__ unsigned tot[kDetRadix];
    unsigned *h = hist + (long long)blockIdx.x * tiles * kDetRadix;
    const int d = threadIdx.x;
    unsigned s = 0u;
    for (long long t = 0; t < tiles; ++t) s += h[t * kDetRadix + d];
    tot[d] = s;
    __syncthreads();
    unsigned base = 0u;
    for (int j = 0; j < d; ++j) base += tot[j];
    for (long long t = 0; t < tiles; ++t) {
        const unsigned v = h[t * kDetRadix + d];
        h[t * kDetRadix + d] = base;
        base += v;
    }
}

// stable scatter of one tile: position = first position of (tile, digit) + the number of earlier items of the tile with the
// same digit.  Earlier rounds: a running count in LDS; the same round: the lanes below in the __ballot match mask.
__global__ void __launch_bounds__(kDetWave)
msda_bwd_det_scatter(const unsigned *__restrict__ keys_in, const unsigned *__restrict__ idx_in,
                     unsigned *__restrict__ keys_out, unsigned *__restrict__ idx_out, const unsigned *__restrict__ hist,
                     long long n_items, long long tiles, int shift)
{
    __shared__ unsigned cnt[kDetRadix];
    const long long blk = blockIdx.x;
    const long long seg = blk / tiles, tile = blk - seg * tiles;
    for (int i = threadIdx.x; i < kDetRadix; i += kDetWave) cnt[i] = hist[blk * kDetRadix + i];
    __syncthreads();
    const long long base = seg * n_items;
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int rd = 0; rd < kDetTileRounds; ++rd) {
        const long long i = tile * kDetTile + rd * kDetWave + lane;
        const bool valid = i < n_items;
        const unsigned key = valid ? keys_in[base + i] : 0u;
        const unsigned idx = valid ? (idx_in ? idx_in[base + i] : (unsigned)i) : 0u;
        const unsigned digit = (key >> shift) & (kDetRadix - 1);
        unsigned long long same = __ballot(valid);
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (digit >> bit) & 1u;
            const unsigned long long bal = __ballot(one);
            same &= one ? bal : ~bal;
        }
        const unsigned rank = (unsigned)__builtin_popcountll(same & below);
        const unsigned first = cnt[digit];
        __syncthreads();
        if (valid && rank == 0u) cnt[digit] = first + (unsigned)__builtin_popcountll(same);
        __syncthreads();
        if (valid) {
            keys_out[base + first + rank] = key;
            idx_out[base + first + rank] = idx;
        }
    }
}

// start[block][r] = the first sorted position whose key is >= r, r = 0 .. S (start[S]: the number of in-range corners).
// Position i writes the rows in (key[i - 1], key[i]]; position n_items stands for a key of S.  Every entry is written once.
__global__ void __launch_bounds__(kThreads)
msda_bwd_det_bounds(const unsigned *__restrict__ keys, unsigned *__restrict__ start, long long n_items,
                    long long blocks_per_seg, int S)
{
    const long long seg = blockIdx.x / blocks_per_seg;
    const long long i = (blockIdx.x - seg * blocks_per_seg) * kThreads + threadIdx.x;
    if (i > n_items) return;
    const unsigned *k = keys + seg * n_items;
    const long long prev = i == 0 ? -1ll : (long long)k[i - 1];
    const long long cur = i == n_items ? (long long)S : (long long)k[i];
    unsigned *st = start + seg * ((long long)S + 1);
    for (long long r = prev + 1; r <= cur; ++r) st[r] = (unsigned)i;
}

// The shape below is the simple one, not a tuned one: a workgroup per row whatever the list length means that at the cfg-2
// encoder (about 64 items per row = two chunks) two of the eight lane groups work and the others only meet the barriers, and
// that a hot row is summed by ONE workgroup (one CU, 256 items per round between two barriers), not by one wave but not by the
// chip either.  Measured times, the split over the kernels and the chunk sizes tried: DESIGN.md section 4.1,
// profiles/det_backward_bench.json.
// One workgroup per destination row: G = 256 / DL groups of DL lanes (DL: the power of two >= D, at most 256; a lane owns
// channel d0 + its index for d0 = 0, DL, ...).  Group j sums chunk c0 + j of the row's list; the partial sums meet in LDS and
// group 0 adds them in chunk order.
template <typename T>
__global__ void __launch_bounds__(kDetReduceThreads)
msda_bwd_det_reduce(const unsigned *__restrict__ idx, const unsigned *__restrict__ start, const T *__restrict__ wts,
                    const T *__restrict__ grad_out, T *__restrict__ grad_value, long long n_items, int S, int M, int D,
                    int Lq, int LP4, int DL)
{
    __shared__ T part[kDetReduceThreads];
    const long long row = blockIdx.x;   // (b M + m) S + r
    const long long seg = row / S;
    const int r = (int)(row - seg * S);
    const int m = (int)(seg % M);
    const long long b = seg / M;
    const unsigned *st = start + seg * ((long long)S + 1);
    const long long lo = st[r], hi = st[r + 1];
    const int G = kDetReduceThreads / DL;
    const int g = threadIdx.x / DL, dl = threadIdx.x - g * DL;
    const unsigned *ix = idx + seg * n_items;
    const T *w = wts + seg * n_items;
    const long long pix = (long long)M * D;
    const T *go = grad_out + b * Lq * pix + (long long)m * D;
    T *out = grad_value + (b * S + r) * pix + (long long)m * D;
    for (int d0 = 0; d0 < D; d0 += DL) {
        const int d = d0 + dl;
        const bool on = d < D;
        T total = (T)0;
        for (long long c0 = lo; c0 < hi; c0 += (long long)G * kDetChunk) {
            const long long cb = c0 + (long long)g * kDetChunk;
            const long long ce = min(cb + kDetChunk, hi);
            T acc = (T)0;
            if (on)
                for (long long i = cb; i < ce; ++i) {
                    const unsigned id = ix[i];
                    const long long q = id / (unsigned)LP4;
                    acc = fma_t(w[id], go[q * pix + d], acc);
                }
            part[threadIdx.x] = acc;
            __syncthreads();
            if (g == 0)
                for (int j = 0; j < G; ++j)
                    if (c0 + (long long)j * kDetChunk < hi) total += part[j * DL + dl];
            __syncthreads();
        }
        if (g == 0 && on) out[d] = total;
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
struct DetPlan {
    int nb;               // images per batch chunk
    int npass;            // radix passes
    long long n_items;    // 4 Lq L P: corner slots of one (n, m) block
    long long tiles;      // radix tiles of one block
    size_t off_keys[2], off_idx[2], off_wts, off_hist, off_start, bytes;
};

inline size_t det_round(size_t v) { return (v + 255) & ~(size_t)255; }

// The workspace of tf_msda_backward_det_* (the formula documented in include/tf_msda.h).
int det_plan(int elem_bytes, int N, int S, int M, int D, int L, int Lq, int P, DetPlan *pl)
{
    if ((elem_bytes != 4 && elem_bytes != 8) || N <= 0 || S <= 0 || M <= 0 || D <= 0 || L <= 0 || Lq <= 0 || P <= 0 ||
        L > TF_MSDA_MAX_LEVELS)
        return TF_MSDA_ERR_BAD_DIMS;
    const long long lp = (long long)L * P;
    if (lp > INT32_MAX / 4 || 4 * lp > INT32_MAX / Lq) return TF_MSDA_ERR_BAD_DIMS;   // the slot index must fit 32 bits
    pl->n_items = 4 * lp * Lq;
    pl->tiles = (pl->n_items + kDetTile - 1) / kDetTile;
    int bits = 0;
    while (bits < 32 && ((unsigned)S >> bits) != 0u) ++bits;   // keys are 0 .. S
    pl->npass = (bits + 7) / 8;
    const auto bytes_of = [&](long long nb, size_t *off) -> size_t {
        const size_t items = (size_t)nb * M * (size_t)pl->n_items;
        size_t at = 0;
        for (int i = 0; i < 4; ++i) {   // keys[2], idx[2]
            off[i] = at;
            at += det_round(items * 4);
        }
        off[4] = at;
        at += det_round(items * (size_t)elem_bytes);
        off[5] = at;
        at += det_round((size_t)nb * M * (size_t)pl->tiles * kDetRadix * 4);
        off[6] = at;
        at += det_round((size_t)nb * M * ((size_t)S + 1) * 4);
        return at;
    };
    size_t off[7];
    const double per_image = (double)M * ((double)pl->n_items * (16.0 + elem_bytes) + (double)pl->tiles * kDetRadix * 4 + ((double)S + 1) * 4);
    if (per_image > 4.0e12) return TF_MSDA_ERR_BAD_DIMS;
    long long nb = (long long)((double)kDetBatchBudget / per_image);
    nb = nb < 1 ? 1 : (nb > N ? N : nb);
    // every launch grid of one batch chunk fits 31 bits
    const double segs = (double)nb * M;
    const double bounds_blocks = (double)((pl->n_items + kThreads) / kThreads);
    if (segs * (double)pl->tiles > 2.0e9 || segs * bounds_blocks > 2.0e9 || segs * (double)S > 2.0e9 ||
        segs * (double)Lq * (double)lp / kThreads > 2.0e9)
        return TF_MSDA_ERR_BAD_DIMS;
    pl->nb = (int)nb;
    pl->bytes = bytes_of(nb, off);
    pl->off_keys[0] = off[0];
    pl->off_keys[1] = off[1];
    pl->off_idx[0] = off[2];
    pl->off_idx[1] = off[3];
    pl->off_wts = off[4];
    pl->off_hist = off[5];
    pl->off_start = off[6];
    return TF_MSDA_OK;
}

template <typename T>
int backward_det_impl(const T *value, const int64_t *shapes_host, const int64_t *shapes_dev, const T *loc, const T *attn,
                      const T *grad_out, T *grad_value, T *grad_loc, T *grad_attn, void *workspace, int64_t workspace_bytes,
                      int N, int S, int M, int D, int L, int Lq, int P, void *stream_v)
{
    // null pointers, dimensions, the workspace, the shape sum: all before any GPU work
    if (!value || !loc || !attn || !grad_out || !grad_value || !grad_loc || !grad_attn || !workspace ||
        (!shapes_host && !shapes_dev))
        return TF_MSDA_ERR_NULL_POINTER;
    DetPlan pl;
    int rc = det_plan((int)sizeof(T), N, S, M, D, L, Lq, P, &pl);
    if (rc != TF_MSDA_OK) return rc;
    if (workspace_bytes < 0 || (uint64_t)workspace_bytes < (uint64_t)pl.bytes || !is_aligned(workspace, 8))
        return TF_MSDA_ERR_WORKSPACE;
    LevelTable lt{};
    if (shapes_host) {
        rc = build_level_table(shapes_host, L, S, &lt);
        if (rc != TF_MSDA_OK) return rc;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    unsigned *keys[2] = {reinterpret_cast<unsigned *>(ws + pl.off_keys[0]), reinterpret_cast<unsigned *>(ws + pl.off_keys[1])};
    unsigned *idx[2] = {reinterpret_cast<unsigned *>(ws + pl.off_idx[0]), reinterpret_cast<unsigned *>(ws + pl.off_idx[1])};
    T *wts = reinterpret_cast<T *>(ws + pl.off_wts);
    unsigned *hist = reinterpret_cast<unsigned *>(ws + pl.off_hist);
    unsigned *start = reinterpret_cast<unsigned *>(ws + pl.off_start);
    int DL = 1;
    while (DL < D && DL < kDetReduceThreads) DL *= 2;
    const long long LP = (long long)L * P;
    const long long bounds_blocks = (pl.n_items + 1 + kThreads - 1) / kThreads;
    for (int n0 = 0; n0 < N; n0 += pl.nb) {
        const int nbc = pl.nb < N - n0 ? pl.nb : N - n0;
        const long long segs = (long long)nbc * M;
        const T *v = value + (size_t)n0 * S * M * D;
        const T *lc = loc + (size_t)n0 * Lq * M * LP * 2;
        const T *at = attn + (size_t)n0 * Lq * M * LP;
        const T *go = grad_out + (size_t)n0 * Lq * M * D;
        T *gv = grad_value + (size_t)n0 * S * M * D;
        T *gl = grad_loc + (size_t)n0 * Lq * M * LP * 2;
        T *ga = grad_attn + (size_t)n0 * Lq * M * LP;
        const long long samples = segs * Lq * LP;
        hipLaunchKernelGGL(msda_bwd_det_emit<T>, dim3((unsigned)((samples + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                           v, lc, at, go, gl, ga, keys[0], wts, lt, shapes_dev, S, M, D, L, Lq, P, samples);
        if ((rc = record_hip(hipGetLastError())) != TF_MSDA_OK) return rc;
        int cur = 0;
        for (int pass = 0; pass < pl.npass; ++pass, cur ^= 1) {
            const int shift = 8 * pass;
            const unsigned *idx_in = pass == 0 ? nullptr : idx[cur];   // first pass: the slot index is the position
            hipLaunchKernelGGL(msda_bwd_det_hist, dim3((unsigned)(segs * pl.tiles)), dim3(kDetWave), 0, stream,
                               (const unsigned *)keys[cur], hist, pl.n_items, pl.tiles, shift);
            if ((rc = record_hip(hipGetLastError())) != TF_MSDA_OK) return rc;
            hipLaunchKernelGGL(msda_bwd_det_scan, dim3((unsigned)segs), dim3(kDetRadix), 0, stream, hist, pl.tiles);
            if ((rc = record_hip(hipGetLastError())) != TF_MSDA_OK) return rc;
            hipLaunchKernelGGL(msda_bwd_det_scatter, dim3((unsigned)(segs * pl.tiles)), dim3(kDetWave), 0, stream,
                               (const unsigned *)keys[cur], idx_in, keys[cur ^ 1], idx[cur ^ 1], (const unsigned *)hist, pl.n_items,
                               pl.tiles, shift);
            if ((rc = record_hip(hipGetLastError())) != TF_MSDA_OK) return rc;
        }
        hipLaunchKernelGGL(msda_bwd_det_bounds, dim3((unsigned)(segs * bounds_blocks)), dim3(kThreads), 0, stream,
                           (const unsigned *)keys[cur], start, pl.n_items, bounds_blocks, S);
        if ((rc = record_hip(hipGetLastError())) != TF_MSDA_OK) return rc;
        hipLaunchKernelGGL(msda_bwd_det_reduce<T>, dim3((unsigned)(segs * S)), dim3(kDetReduceThreads), 0, stream,
                           (const unsigned *)idx[cur], (const unsigned *)start, (const T *)wts, go, gv, pl.n_items, S, M, D, Lq,
                           (int)(4 * LP), DL);
        if ((rc = record_hip(hipGetLastError())) != TF_MSDA_OK) return rc;
    }
    note_kernel(sizeof(T) == 4 ? "msda_bwd_det<f32>" : "msda_bwd_det<f64>");
    return TF_MSDA_OK;
}

#endif  // TF_MSDA_BWD_DET_H_
