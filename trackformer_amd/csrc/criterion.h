// trackformer_amd/csrc/criterion.h -- the set criterion of the stacked decoder layers and the matcher's cost matrix (included from
// fused_ops.hip; include/tf_fused.h: THE SET CRITERION AND THE MATCHING COST).
//
//   set_criterion_fwd_kernel   one workgroup per decoder layer: the focal class loss, the L1 and GIoU losses of the matched pairs, the
//                              cardinality error and (layer 0) the class error, in one launch
//   set_criterion_bwd_kernel   one work-item per (layer, image, query): the gradients of its C logits and of its box, recomputed from
//                              the inputs
//   match_cost_kernel          one work-item per (prediction, target): focal class cost + L1 + GIoU, weighted
//
// These kernels work on a few thousand numbers: what they save is launches, not bytes -- nothing here is tiled for bandwidth.
// THE FOCAL TERM is evaluated in its stable form.  With z = x for a negative and z = -x for a positive element,
//     -log p_t = softplus(z)          (1 - p_t)^gamma = exp(-gamma softplus(-z))          softplus(+-z) = max(+-z, 0) + log1p(exp(-|z|))
// so no 1 - sigmoid(x) is ever formed in fp32 (that subtraction costs the small elements and their gradients all their digits beyond
// |x| ~ 8).  THE BOX TERMS follow box_ops.generalized_box_iou_pairs and l1_loss operation by operation, without FMA contraction, and
// without guards: a zero-area pair gives NaN as in torch.  THE SUMS are accumulated in fp64 and rounded once; their order is a function
// of the shape alone (thread t takes queries t, t + 256, ... of image 0, then of image 1, ...; a butterfly over the wave; the four waves
// in wave order through LDS).  No atomics; every output element is written once.
#ifndef TF_CRITERION_H_
#define TF_CRITERION_H_

namespace {

struct FocalTerm {
    float loss;   // alpha_t softplus(z) exp(-gamma softplus(-z))
    float dx;     // its derivative with respect to the logit
};

// One element of sigmoid_focal_loss: logit x, `pos` = the element's target is 1.  alpha < 0: no alpha weight.
template <bool GRAD>
__device__ __forceinline__ FocalTerm focal_term(float x, bool pos, float alpha, float gamma)
{
    const float z = pos ? -x : x;
    const float e = expf(-fabsf(z));
    const float u = log1pf(e);
    const float sp = fmaxf(z, 0.f) + u;      // softplus(z)  = -log p_t
    const float sn = fmaxf(-z, 0.f) + u;     // softplus(-z) = -log(1 - p_t)
    const float mod = expf(-gamma * sn);     // (1 - p_t)^gamma
    const float a = alpha >= 0.f ? (pos ? alpha : 1.f - alpha) : 1.f;
    FocalTerm r;
    r.loss = a * (sp * mod);
    r.dx = 0.f;
    if constexpr (GRAD) {
        const float inv = 1.f / (1.f + e);
        const float s_hi = inv, s_lo = e * inv;          // sigmoid(|z|), sigmoid(-|z|)
        const float sz = z >= 0.f ? s_hi : s_lo;         // sigmoid(z)  = 1 - p_t
        const float snz = z >= 0.f ? s_lo : s_hi;        // sigmoid(-z) = p_t
        const float dz = a * (mod * (sz + gamma * (sp * snz)));   // a sum of positive terms: no cancellation
        r.dx = pos ? -dz : dz;
    }
    return r;
}

// GIoU of two cxcywh boxes, as box_cxcywh_to_xyxy + generalized_box_iou_pairs compute it (every operation rounded on its own).
__device__ __forceinline__ float giou_cxcywh(f32x4_t a, f32x4_t b)
{
#pragma clang fp contract(off)
    const float ax1 = a.x - 0.5f * a.z, ay1 = a.y - 0.5f * a.w, ax2 = a.x + 0.5f * a.z, ay2 = a.y + 0.5f * a.w;
    const float bx1 = b.x - 0.5f * b.z, by1 = b.y - 0.5f * b.w, bx2 = b.x + 0.5f * b.z, by2 = b.y + 0.5f * b.w;
    const float area1 = (ax2 - ax1) * (ay2 - ay1), area2 = (bx2 - bx1) * (by2 - by1);
    const float iw = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.f), ih = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.f);
    const float inter = iw * ih;
    const float uni = area1 + area2 - inter;
    const float iou = inter / uni;
    const float hw = fmaxf(fmaxf(ax2, bx2) - fminf(ax1, bx1), 0.f), hh = fmaxf(fmaxf(ay2, by2) - fminf(ay1, by1), 0.f);
    const float hull = hw * hh;
    return iou - (hull - uni) / hull;
}

__device__ __forceinline__ float l1_cxcywh(f32x4_t a, f32x4_t b)
{
#pragma clang fp contract(off)
    return ((fabsf(a.x - b.x) + fabsf(a.y - b.y)) + fabsf(a.z - b.z)) + fabsf(a.w - b.w);
}

// share of the gradient that min(a, b) / max(a, b) hands to a: all of it, half at a tie (as torch), none
__device__ __forceinline__ float share_lt(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }

// d(1 - GIoU(a, b)) / da for cxcywh boxes: the chain rule through the operations of giou_cxcywh, as autograd walks them.
__device__ __forceinline__ f32x4_t giou_loss_grad_cxcywh(f32x4_t a, f32x4_t b)
{
#pragma clang fp contract(off)
    const float ax1 = a.x - 0.5f * a.z, ay1 = a.y - 0.5f * a.w, ax2 = a.x + 0.5f * a.z, ay2 = a.y + 0.5f * a.w;
    const float bx1 = b.x - 0.5f * b.z, by1 = b.y - 0.5f * b.w, bx2 = b.x + 0.5f * b.z, by2 = b.y + 0.5f * b.w;
    const float w1 = ax2 - ax1, h1 = ay2 - ay1;
    const float area1 = w1 * h1, area2 = (bx2 - bx1) * (by2 - by1);
    const float iwr = fminf(ax2, bx2) - fmaxf(ax1, bx1), ihr = fminf(ay2, by2) - fmaxf(ay1, by1);
    const float iw = fmaxf(iwr, 0.f), ih = fmaxf(ihr, 0.f);
    const float inter = iw * ih;
    const float uni = area1 + area2 - inter;
    const float hwr = fmaxf(ax2, bx2) - fminf(ax1, bx1), hhr = fmaxf(ay2, by2) - fminf(ay1, by1);
    const float hw = fmaxf(hwr, 0.f), hh = fmaxf(hhr, 0.f);
    const float hull = hw * hh;
    // giou = inter / uni - 1 + uni / hull
    const float g_uni = 1.f / hull - inter / (uni * uni);   // also the gradient of area1
    const float g_inter = 1.f / uni - g_uni;
    const float g_hull = -(uni / (hull * hull));
    const float g_iw = iwr >= 0.f ? g_inter * ih : 0.f, g_ih = ihr >= 0.f ? g_inter * iw : 0.f;
    const float g_hw = hwr >= 0.f ? g_hull * hh : 0.f, g_hh = hhr >= 0.f ? g_hull * hw : 0.f;
    const float gx2 = (g_iw * share_lt(ax2, bx2) + g_hw * share_lt(bx2, ax2)) + g_uni * h1;
    const float gx1 = -((g_iw * share_lt(bx1, ax1) + g_hw * share_lt(ax1, bx1)) + g_uni * h1);
    const float gy2 = (g_ih * share_lt(ay2, by2) + g_hh * share_lt(by2, ay2)) + g_uni * w1;
    const float gy1 = -((g_ih * share_lt(by1, ay1) + g_hh * share_lt(ay1, by1)) + g_uni * w1);
    return f32x4_t{-(gx1 + gx2), -(gy1 + gy2), -(0.5f * (gx2 - gx1)), -(0.5f * (gy2 - gy1))};
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ int wave_sum_i32(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// arg-max of a row of C logits, the lowest index on ties; a NaN counts as the largest value (as torch.argmax)
__device__ __forceinline__ bool argmax_takes(float v, float best) { return v > best || (v != v && best == best); }

// blockIdx.x = the decoder layer.  tgt_of[l, b, q]: the global index of the target matched to that prediction, or -1 (anything
// outside [0, T) counts as unmatched: no target is read for it).
__global__ void __launch_bounds__(256)
set_criterion_fwd_kernel(const float *__restrict__ logits, const float *__restrict__ boxes, const int *__restrict__ tgt_of,
                         const long long *__restrict__ labels, const float *__restrict__ tboxes, const int *__restrict__ tgt_len,
                         float *__restrict__ losses, float *__restrict__ card, float *__restrict__ class_error, int B, int Q, int C, int T,
                         float alpha, float gamma, float num_boxes)
{
    __shared__ double s_sum[4][3];
    __shared__ int s_cnt[2][4];
    __shared__ int s_acc[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l = blockIdx.x;
    double ce = 0.0, l1 = 0.0, gi = 0.0;
    int correct = 0, matched = 0, card_abs = 0;
    for (int b = 0; b < B; ++b) {   // (uniform)
        int cnt = 0;
        for (int q = threadIdx.x; q < Q; q += 256) {
            const long long row = ((long long)l * B + b) * Q + q;
            const int t = tgt_of[row];
            const bool has = t >= 0 && t < T;
            const int label = has ? (int)labels[t] : -1;
            const float *x = logits + row * C;
            float best = x[0];
            int arg = 0;
            for (int c = 0; c < C; ++c) {
                const float v = x[c];
                ce += (double)focal_term<false>(v, c == label, alpha, gamma).loss;
                if (c > 0 && argmax_takes(v, best)) {
                    best = v;
                    arg = c;
                }
            }
            cnt += arg != C - 1 ? 1 : 0;   // (C == 1: never, as the reference)
            if (has) {
                const f32x4_t a = reinterpret_cast<const f32x4_t *>(boxes)[row];
                const f32x4_t tb = reinterpret_cast<const f32x4_t *>(tboxes)[t];
                l1 += (double)l1_cxcywh(a, tb);
                gi += (double)(1.f - giou_cxcywh(a, tb));
                matched += 1;
                correct += arg == label ? 1 : 0;
            }
        }
        cnt = wave_sum_i32(cnt);
        if (lane == 0) s_cnt[b & 1][wave] = cnt;
        __syncthreads();   // one barrier per image: the two halves of s_cnt alternate
        const int total = (s_cnt[b & 1][0] + s_cnt[b & 1][1]) + (s_cnt[b & 1][2] + s_cnt[b & 1][3]);
        const int d = total - tgt_len[b];
        card_abs += d < 0 ? -d : d;
    }
    ce = wave_sum_f64(ce);
    l1 = wave_sum_f64(l1);
    gi = wave_sum_f64(gi);
    correct = wave_sum_i32(correct);
    matched = wave_sum_i32(matched);
    if (lane == 0) {
        s_sum[wave][0] = ce;
        s_sum[wave][1] = l1;
        s_sum[wave][2] = gi;
        s_acc[wave][0] = correct;
        s_acc[wave][1] = matched;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        const double s = ((s_sum[0][k] + s_sum[1][k]) + s_sum[2][k]) + s_sum[3][k];
        losses[l * 3 + k] = (float)(s / (double)num_boxes);
    }
    if (threadIdx.x == 3) card[l] = (float)card_abs / (float)B;
    if (threadIdx.x == 4 && l == 0) {
        // (no contraction: 100 - n (100 / n) is 0 when the product rounds to 100, as in torch; a fused multiply-add leaves its residue)
#pragma clang fp contract(off)
        const int n_ok = (s_acc[0][0] + s_acc[1][0]) + (s_acc[2][0] + s_acc[3][0]);
        const int n = (s_acc[0][1] + s_acc[1][1]) + (s_acc[2][1] + s_acc[3][1]);
        class_error[0] = n > 0 ? 100.f - (float)n_ok * (100.f / (float)n) : 100.f;
    }
}

// One work-item per (l, b, q) row.  G [L, 3]: the gradients of (loss_ce, loss_bbox, loss_giou) of each layer.
__global__ void __launch_bounds__(256)
set_criterion_bwd_kernel(const float *__restrict__ G, const float *__restrict__ logits, const float *__restrict__ boxes,
                         const int *__restrict__ tgt_of, const long long *__restrict__ labels, const float *__restrict__ tboxes,
                         float *__restrict__ grad_logits, float *__restrict__ grad_boxes, long long rows, int rows_per_layer, int C, int T,
                         float alpha, float gamma, float num_boxes)
{
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const int l = (int)(row / rows_per_layer);
    const int t = tgt_of[row];
    const bool has = t >= 0 && t < T;
    if (grad_logits != nullptr) {   // (uniform)
        const float g = G[l * 3 + 0] / num_boxes;
        const int label = has ? (int)labels[t] : -1;
        const float *x = logits + row * C;
        float *gx = grad_logits + row * C;
        for (int c = 0; c < C; ++c) gx[c] = g * focal_term<true>(x[c], c == label, alpha, gamma).dx;
    }
    if (grad_boxes != nullptr) {   // (uniform)
        f32x4_t out = {0.f, 0.f, 0.f, 0.f};
        if (has) {
#pragma clang fp contract(off)
            const float g1 = G[l * 3 + 1] / num_boxes, g2 = G[l * 3 + 2] / num_boxes;
            const f32x4_t a = reinterpret_cast<const f32x4_t *>(boxes)[row];
            const f32x4_t tb = reinterpret_cast<const f32x4_t *>(tboxes)[t];
            const f32x4_t d = a - tb;
            const f32x4_t sg = {d.x > 0.f ? 1.f : (d.x < 0.f ? -1.f : d.x), d.y > 0.f ? 1.f : (d.y < 0.f ? -1.f : d.y),
                                d.z > 0.f ? 1.f : (d.z < 0.f ? -1.f : d.z), d.w > 0.f ? 1.f : (d.w < 0.f ? -1.f : d.w)};
            out = sg * g1 + giou_loss_grad_cxcywh(a, tb) * g2;
        }
        reinterpret_cast<f32x4_t *>(grad_boxes)[row] = out;
    }
}

// One work-item per (r, t): the focal branch of HungarianMatcher.match_many, with 1 - p formed as sigmoid(-x).
__global__ void __launch_bounds__(256)
match_cost_kernel(const float *__restrict__ logits, const float *__restrict__ boxes, const long long *__restrict__ tgt_ids,
                  const float *__restrict__ tgt_bbox, float *__restrict__ cost, long long total, int C, int T, float w_class, float w_bbox,
                  float w_giou, float alpha, float gamma)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long r = i / T;
    const int t = (int)(i - r * T);
    const long long id = tgt_ids[t];
    float c_class = 0.f;
    if (id >= 0 && id < C) {   // (checked on the host side of the binding; never read outside the row)
#pragma clang fp contract(off)
        const float x = logits[r * C + id];
        const float e = expf(-fabsf(x));
        const float inv = 1.f / (1.f + e);
        const float p = x >= 0.f ? inv : e * inv, q = x >= 0.f ? e * inv : inv;   // sigmoid(x), sigmoid(-x)
        const float pg = gamma == 2.f ? p * p : powf(p, gamma), qg = gamma == 2.f ? q * q : powf(q, gamma);
        const float neg = ((1.f - alpha) * pg) * (-logf(q + 1e-8f));
        const float pos = (alpha * qg) * (-logf(p + 1e-8f));
        c_class = pos - neg;
    }
    {
#pragma clang fp contract(off)
        const f32x4_t a = reinterpret_cast<const f32x4_t *>(boxes)[r];
        const f32x4_t b = reinterpret_cast<const f32x4_t *>(tgt_bbox)[t];
        const float c_bbox = l1_cxcywh(a, b);
        const float c_giou = -giou_cxcywh(a, b);
        cost[i] = (w_bbox * c_bbox + w_class * c_class) + w_giou * c_giou;
    }
}

bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// the checks the two criterion entries share; rows = L B Q
int criterion_check(const float *logits, const float *boxes, const int *tgt_of, const int64_t *labels, const float *tboxes, int L, int B,
                    int Q, int C, int T, float num_boxes, long long *rows)
{
    if (!logits || !boxes || !tgt_of || (T > 0 && (!labels || !tboxes))) return TF_MSDA_ERR_NULL_POINTER;
    if (L <= 0 || B <= 0 || Q <= 0 || C <= 0 || T < 0 || !(num_boxes > 0.f)) return TF_MSDA_ERR_BAD_DIMS;
    *rows = (long long)L * B * Q;
    if (*rows > 0x7fffffffLL / (C > 4 ? C : 4)) return TF_MSDA_ERR_BAD_DIMS;
    if (!aligned4(logits) || !aligned16(boxes) || !aligned4(tgt_of) || (T > 0 && (!aligned8(labels) || !aligned16(tboxes))))
        return TF_MSDA_ERR_BAD_DIMS;
    return TF_MSDA_OK;
}

}  // namespace

extern "C" int tf_set_criterion_fwd_f32(const float *logits, const float *boxes, const int *tgt_of, const int64_t *labels,
                                        const float *tboxes, const int *tgt_len, float *losses, float *card, float *class_error, int L,
                                        int B, int Q, int C, int T, float alpha, float gamma, float num_boxes, void *stream)
{
    long long rows = 0;
    if (!tgt_len || !losses || !card || !class_error) return TF_MSDA_ERR_NULL_POINTER;
    const int rc = criterion_check(logits, boxes, tgt_of, labels, tboxes, L, B, Q, C, T, num_boxes, &rows);
    if (rc != TF_MSDA_OK) return rc;
    if (!aligned4(tgt_len) || !aligned4(losses) || !aligned4(card) || !aligned4(class_error)) return TF_MSDA_ERR_BAD_DIMS;
    hipLaunchKernelGGL(set_criterion_fwd_kernel, dim3((unsigned)L), dim3(256), 0, static_cast<hipStream_t>(stream), logits, boxes, tgt_of,
                       reinterpret_cast<const long long *>(labels), tboxes, tgt_len, losses, card, class_error, B, Q, C, T, alpha, gamma,
                       num_boxes);
    if (int rc = tfm::launched()) return rc;
    tfm::note_kernel("set_criterion_fwd_f32");
    return TF_MSDA_OK;
}

extern "C" int tf_set_criterion_bwd_f32(const float *G, const float *logits, const float *boxes, const int *tgt_of, const int64_t *labels,
                                        const float *tboxes, float *grad_logits, float *grad_boxes, int L, int B, int Q, int C, int T,
                                        float alpha, float gamma, float num_boxes, void *stream)
{
    long long rows = 0;
    if (!G) return TF_MSDA_ERR_NULL_POINTER;
    const int rc = criterion_check(logits, boxes, tgt_of, labels, tboxes, L, B, Q, C, T, num_boxes, &rows);
    if (rc != TF_MSDA_OK) return rc;
    if (!aligned4(G) || (grad_logits && !aligned4(grad_logits)) || (grad_boxes && !aligned16(grad_boxes))) return TF_MSDA_ERR_BAD_DIMS;
    if (!grad_logits && !grad_boxes) return TF_MSDA_OK;   // nothing asked for
    hipLaunchKernelGGL(set_criterion_bwd_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), G,
                       logits, boxes, tgt_of, reinterpret_cast<const long long *>(labels), tboxes, grad_logits, grad_boxes, rows, B * Q, C,
                       T, alpha, gamma, num_boxes);
    if (int rc = tfm::launched()) return rc;
    tfm::note_kernel("set_criterion_bwd_f32");
    return TF_MSDA_OK;
}

extern "C" int tf_match_cost_f32(const float *logits, const float *boxes, const int64_t *tgt_ids, const float *tgt_bbox, float *cost,
                                 int64_t R, int C, int T, float w_class, float w_bbox, float w_giou, float alpha, float gamma, void *stream)
{
    if (R < 0 || C <= 0 || T < 0 || R > 0x7fffffffLL / (C > 4 ? C : 4) || (T > 0 && R > 0x7fffffffLL / T)) return TF_MSDA_ERR_BAD_DIMS;
    if (R == 0 || T == 0) return TF_MSDA_OK;   // an empty matrix
    if (!logits || !boxes || !tgt_ids || !tgt_bbox || !cost) return TF_MSDA_ERR_NULL_POINTER;
    if (!aligned4(logits) || !aligned16(boxes) || !aligned8(tgt_ids) || !aligned16(tgt_bbox) || !aligned4(cost)) return TF_MSDA_ERR_BAD_DIMS;
    const long long total = (long long)R * T;
    hipLaunchKernelGGL(match_cost_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), logits, boxes,
                       reinterpret_cast<const long long *>(tgt_ids), tgt_bbox, cost, total, C, T, w_class, w_bbox, w_giou, alpha, gamma);
    if (int rc = tfm::launched()) return rc;
    tfm::note_kernel("match_cost_f32");
    return TF_MSDA_OK;
}

#endif /* TF_CRITERION_H_ */
