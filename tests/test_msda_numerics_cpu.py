"""CPU: the float64 yardstick of MSDeformAttn (tests/util_msda_numerics.py) has power.  It accepts the fp32 C oracle in every
operand profile, fp32 restatements that sum in another order, and the reference's twice-rounded pixel coordinate; it rejects
bilinear weights rounded to bf16 or fp16, corners dropped below a weight of 2^-10, loc rounded to fp16, fp16 accumulation, a
grad_value that misses one contribution on busy rows, a grad_loc with fx / fy swapped in its cross term, and a fused softmax
without its max shift under large logits.  So a kernel that fails it on the GPU computes something other than fp32 MSDA."""
import numpy as np
import pytest
import torch

from oracle import msda_oracle
from tests import util_msda_numerics as U
from tests.util_msda import golden_cases, load_case

SHAPES = [(12, 20), (6, 10), (3, 5), (2, 3)]
S_ENC = sum(h * w for h, w in SHAPES)


@pytest.fixture(autouse=True, scope="module")
def _threads():
    prev = torch.get_num_threads()
    torch.set_num_threads(min(prev, 16))
    yield
    torch.set_num_threads(prev)


def _case(profile, seed=1, N=2, M=4, D=8, P=4, shapes=SHAPES):
    enc = profile == "permuted"
    return U.make_case(profile, N, M, D, S_ENC if enc and shapes is SHAPES else 300, P, shapes, seed, encoder=enc)


def _oracle(v, s, l, a, g=None):
    n = [t.numpy() for t in (v, s, l, a)]
    out = msda_oracle.msda_forward(*n)
    return out if g is None else (out,) + msda_oracle.msda_backward(*n, g.numpy())


# ---- fp32 restatements (torch, fp32 arithmetic) ---------------------------------------------------------------------------------------
def _round(t, fault):
    if fault == "w_bf16":
        return t.bfloat16().float()
    if fault == "w_f16":
        return t.half().float()
    if fault == "drop_small":
        return torch.where(t < 2.0 ** -10, torch.zeros_like(t), t)
    return t


def _geometry(loc_c, size, fault, twice):
    """fp32 pixel coordinate: one rounding of the exact loc * size - 0.5 (what fma gives), or the reference's two."""
    if fault == "loc_f16":
        loc_c = loc_c.half().float()
    if twice:
        return (loc_c * size) - 0.5
    return (loc_c.double() * size - 0.5).float()


def _terms(value, shapes, loc, attn, fault=None, twice=False):
    """Per-sample fp32 terms a * sum_c w_c v_c ([N, Lq, M, D] each, in (l, p) order) and their geometry."""
    hw, st = U._starts(shapes)
    N, S, M, D = value.shape
    P = loc.shape[4]
    n_i = torch.arange(N).view(N, 1, 1)
    m_i = torch.arange(M).view(1, 1, M)
    terms = []
    for l, (H, W) in enumerate(hw):
        for p in range(P):
            px = _geometry(loc[:, :, :, l, p, 0], W, fault, twice)
            py = _geometry(loc[:, :, :, l, p, 1], H, fault, twice)
            inr = (px > -1) & (py > -1) & (px < W) & (py < H)
            px, py = torch.where(inr, px, torch.zeros_like(px)), torch.where(inr, py, torch.zeros_like(py))
            x0, y0 = px.floor(), py.floor()
            fx, fy = px - x0, py - y0
            gx, gy = 1 - fx, 1 - fy
            s = torch.zeros(N, loc.shape[1], M, D)
            for cy, cx, w in ((0, 0, gy * gx), (0, 1, gy * fx), (1, 0, fy * gx), (1, 1, fy * fx)):
                yi, xi = y0 + cy, x0 + cx
                ok = inr & (yi >= 0) & (xi >= 0) & (yi <= H - 1) & (xi <= W - 1)
                pix = st[l] + (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long()
                v = torch.where(ok[..., None], value[n_i, pix, m_i], torch.zeros(()))
                s = s + _round(w, fault)[..., None] * v
            terms.append(torch.where(inr[..., None], s * attn[:, :, :, l, p, None], torch.zeros(())))
    return terms


def fp32_forward(value, shapes, loc, attn, order="natural", fault=None, twice=False):
    terms = _terms(value, shapes, loc, attn, fault, twice)
    if order == "reversed":
        terms = terms[::-1]
    if order == "pairwise":
        while len(terms) > 1:
            terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
        acc = terms[0]
    else:
        acc = torch.zeros_like(terms[0])
        for t in terms:
            acc = acc + t
            if fault == "acc_f16":
                acc = acc.half().float()
    return acc.reshape(value.shape[0], loc.shape[1], -1)


def fp32_backward(value, shapes, loc, attn, grad_out, fault=None):
    """fp32 gradients as msda_ref.c forms them; fault "gv_missing": the first contribution to every row hit 8 or more times is
    lost; "gl_swap": fx and fy trade places in grad_loc's cross term."""
    hw, st = U._starts(shapes)
    N, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    n_i = torch.arange(N).view(N, 1, 1)
    m_i = torch.arange(M).view(1, 1, M)
    g = grad_out.view(N, Lq, M, D)
    gl = torch.zeros_like(loc)
    ga = torch.zeros_like(attn)
    rows_all, vals_all = [], []
    for l, (H, W) in enumerate(hw):
        for p in range(P):
            a = attn[:, :, :, l, p]
            px = _geometry(loc[:, :, :, l, p, 0], W, None, False)
            py = _geometry(loc[:, :, :, l, p, 1], H, None, False)
            inr = (px > -1) & (py > -1) & (px < W) & (py < H)
            px, py = torch.where(inr, px, torch.zeros_like(px)), torch.where(inr, py, torch.zeros_like(py))
            x0, y0 = px.floor(), py.floor()
            fx, fy = px - x0, py - y0
            gx, gy = 1 - fx, 1 - fy
            vs, oks, pixs = [], [], []
            for cy, cx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                yi, xi = y0 + cy, x0 + cx
                ok = inr & (yi >= 0) & (xi >= 0) & (yi <= H - 1) & (xi <= W - 1)
                pix = st[l] + (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long()
                vs.append(torch.where(ok[..., None], value[n_i, pix, m_i], torch.zeros(())))
                oks.append(ok)
                pixs.append(pix)
            v1, v2, v3, v4 = vs
            ws = (gy * gx, gy * fx, fy * gx, fy * fx)
            samp = sum(w[..., None] * v for w, v in zip(ws, vs))
            ga[:, :, :, l, p] = torch.where(inr, (g * samp).sum(-1), torch.zeros(()))
            cy_, fy_ = (gx, fx) if fault == "gl_swap" else (gy, fy)
            cwx = cy_[..., None] * (v2 - v1) + fy_[..., None] * (v4 - v3)
            cwy = gx[..., None] * (v3 - v1) + fx[..., None] * (v4 - v2)
            gl[:, :, :, l, p, 0] = torch.where(inr, (g * cwx).sum(-1) * a * W, torch.zeros(()))
            gl[:, :, :, l, p, 1] = torch.where(inr, (g * cwy).sum(-1) * a * H, torch.zeros(()))
            top = g * a[..., None]
            for w, ok, pix in zip(ws, oks, pixs):
                rows = (n_i * S + pix) * M + m_i
                rows_all.append(rows[ok])
                vals_all.append((w[..., None] * top)[ok])
    rows, vals = torch.cat(rows_all), torch.cat(vals_all)
    if fault == "gv_missing":
        order = torch.sort(rows, stable=True).indices
        rs = rows[order]
        first = torch.ones_like(rs, dtype=torch.bool)
        first[1:] = rs[1:] != rs[:-1]
        busy = torch.bincount(rows, minlength=N * S * M)[rs] >= 8
        keep = torch.ones_like(rows, dtype=torch.bool)
        keep[order[first & busy]] = False
        rows, vals = rows[keep], vals[keep]
    gv = torch.zeros(N * S * M, D).index_add_(0, rows, vals)
    return gv.view(N, S, M, D), gl, ga


def fp32_fused_prologue(shapes, refp, qproj, M, L, P, shift=True):
    """The fused entry's softmax and location arithmetic in fp32 (shift=False: exp of the raw logits)."""
    hw, _ = U._starts(shapes)
    N, Lq = qproj.shape[:2]
    off = qproj[..., :2 * M * L * P].reshape(N, Lq, M, L, P, 2)
    z = qproj[..., 2 * M * L * P:].reshape(N, Lq, M, L * P)
    e = torch.exp(z - z.amax(-1, keepdim=True)) if shift else torch.exp(z)
    a = (e / e.sum(-1, keepdim=True)).reshape(N, Lq, M, L, P)
    hws = torch.tensor(hw, dtype=torch.float32).view(1, 1, 1, L, 1, 2)
    loc = refp[:, :, None, :, None, :] + off / hws
    return loc.contiguous(), a.contiguous()


# ---- the restatement is pinned --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", golden_cases(), ids=lambda p: p.split("msda_")[-1][:-4])
def test_reference_agrees_with_goldens_and_the_oracle_float64_path(path):
    """float64 goldens of the reference's own implementation, and msda_ref.c in float64 on the same inputs, to 1e-12 of S."""
    z = load_case(path)
    v, s, l, a, g = [torch.from_numpy(z[k]) for k in ("value", "shapes", "loc", "attn", "grad_out")]
    r = U.forward_reference(v, s, l, a)
    f64 = torch.from_numpy(U.oracle_f64_forward(v, s, l, a)).reshape(r.ref.shape)
    assert float(((r.ref - f64).abs() / r.scale.clamp_min(1e-300)).max()) <= 1e-12
    rv, rl, ra, _ = U.backward_reference(v, s, l, a, g)
    ov, ol, oa = msda_oracle.msda_backward(*[t.double().numpy() for t in (v, s, l, a, g)])
    assert float(((rv.ref - torch.from_numpy(ov)).abs() / rv.scale.clamp_min(1e-300)).max()) <= 1e-12
    assert float(((ra.ref - torch.from_numpy(oa)).abs() / ra.scale.clamp_min(1e-300)).max()) <= 1e-12
    assert float(((rl.ref - torch.from_numpy(ol)).abs() / rl.scale.clamp_min(1e-300)).max()) <= 1e-12
    if z["value"].dtype == np.float64:
        for got, key in ((r.ref, "out"), (rv.ref, "grad_value"), (ra.ref, "grad_attn")):
            want = torch.from_numpy(z[key]).reshape(got.shape)
            sc = {"out": r.scale, "grad_value": rv.scale, "grad_attn": ra.scale}[key]
            assert float(((got - want).abs() / sc.clamp_min(1e-300)).max()) <= 1e-12, key
        keep = rl.keep & ~torch.from_numpy(np.asarray(_discontinuous(z)))
        assert float(((rl.ref - torch.from_numpy(z["grad_loc"])).abs() / rl.scale.clamp_min(1e-300))[keep].max()) <= 1e-12


def _discontinuous(z):
    from tests.util_msda import discontinuity_mask
    return np.repeat(discontinuity_mask(z["loc"], z["shapes"])[..., None], 2, -1)


# ---- accepts ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", U.PROFILES)
def test_accepts_the_fp32_oracle_and_reordered_fp32_sums(profile):
    v, s, l, a, g = _case(profile)
    r = U.forward_reference(v, s, l, a)
    out, ov, ol, oa = _oracle(v, s, l, a, g)
    U.check(out, r, fp32=out, what="oracle")
    for order in ("natural", "reversed", "pairwise"):
        U.check(fp32_forward(v, s, l, a, order), r, fp32=out, what=order)
    U.check(fp32_forward(v, s, l, a, twice=True), r, fp32=out, what="twice rounded")
    rv, rl, ra, left = U.backward_reference(v, s, l, a, g)
    assert left < U.EXCLUDE_MAX
    for got, want in ((ov, rv), (ol, rl), (oa, ra)):
        U.check(got, want, fp32=got)
    for got, want, o in zip(fp32_backward(v, s, l, a, g), (rv, rl, ra), (ov, ol, oa)):
        U.check(got, want, fp32=o)


@pytest.mark.parametrize("D,P,shapes", [(1, 1, [(5, 7)]), (3, 3, [(1, 1), (1, 9), (7, 1), (4, 4)]), (64, 8, [(3, 2)] * 16)],
                         ids=["d1_p1", "one_pixel_levels", "l16_p8_d64"])
def test_accepts_the_oracle_at_shape_edges(D, P, shapes):
    v, s, l, a, g = U.make_case("wide", 1, 3, D, 40, P, shapes, seed=D + P)
    r = U.forward_reference(v, s, l, a)
    out, ov, ol, oa = _oracle(v, s, l, a, g)
    U.check(out, r, fp32=out)
    rv, rl, ra, left = U.backward_reference(v, s, l, a, g)
    for got, want in ((ov, rv), (ol, rl), (oa, ra)):
        U.check(got, want, fp32=got)


def test_exact_edges_need_no_exclusion():
    v, s, l, a, g = U.exact_edge_case(1, 2, 4, 4, [(4, 8), (2, 2), (1, 1), (1, 4)], seed=3)
    r = U.forward_reference(v, s, l, a, exact=True)
    out, ov, ol, oa = _oracle(v, s, l, a, g)
    U.check(out, r, fp32=out)
    rv, rl, ra, left = U.backward_reference(v, s, l, a, g, exact=True)
    assert left == 0.0
    for got, want in ((ov, rv), (ol, rl), (oa, ra)):
        U.check(got, want, fp32=got)
    # every listed position is reached: px == -1 and px == W (out of range) as well as W - ulp and -1 + ulp (in range)
    px = l[..., 0].double() * 8 - 0.5
    assert bool((px[:, :, :, 0] == -1).any()) and bool((px[:, :, :, 0] == 8).any()) and bool((px[:, :, :, 0] == 8 * (1 - 2.0 ** -23)).any())


def test_nan_pixels_give_exactly_the_expected_nans():
    v, s, l, a, g = _case("unit")
    U.add_nan_pixels(v, l, s, 5, seed=2)
    r = U.forward_reference(v, s, l, a)
    assert bool(r.expect_nan.any()) and not bool(r.expect_nan.all())
    out, ov, ol, oa = _oracle(v, s, l, a, g)
    U.check(out, r, fp32=out)
    rv, rl, ra, _ = U.backward_reference(v, s, l, a, g)
    for got, want in ((ov, rv), (ol, rl), (oa, ra)):
        U.check(got, want, fp32=got)


@pytest.mark.parametrize("profile", U.FUSED_PROFILES)
def test_fused_reference_accepts_the_fp32_prologue(profile):
    M, L, P = 4, len(SHAPES), 4
    v, s, refp, qproj = U.make_fused_case(profile, 2, M, 8, 60, P, SHAPES, seed=4)
    loc, a, dloc, da = U.fused_locations(s, refp, qproj, M, L, P)
    r = U.forward_reference(v, s, loc, a, dloc=dloc, da=da)
    floc, fa = fp32_fused_prologue(s, refp, qproj, M, L, P)
    out = _oracle(v, s, floc, fa)
    U.check(out, r, fp32=out)


# ---- rejects ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", ["w_bf16", "w_f16", "drop_small", "loc_f16", "acc_f16"])
@pytest.mark.parametrize("profile", ["unit", "large", "small", "level_spread"])
def test_rejects_forward_faults(fault, profile):
    v, s, l, a, g = _case(profile)
    r = U.forward_reference(v, s, l, a)
    out = _oracle(v, s, l, a)
    with pytest.raises(AssertionError):
        U.check(fp32_forward(v, s, l, a, fault=fault), r, fp32=out)


@pytest.mark.parametrize("fault", ["gv_missing", "gl_swap"])
@pytest.mark.parametrize("profile", ["unit", "hot_pixel", "permuted"])
def test_rejects_backward_faults(fault, profile):
    v, s, l, a, g = _case(profile)
    rv, rl, ra, _ = U.backward_reference(v, s, l, a, g)
    _, ov, ol, oa = _oracle(v, s, l, a, g)
    gv, gl, ga = fp32_backward(v, s, l, a, g, fault=fault)
    U.check(ga, ra, fp32=oa)        # the fault leaves grad_attn alone ...
    with pytest.raises(AssertionError):   # ... and is caught in the gradient it touches
        if fault == "gv_missing":
            U.check(gv, rv, fp32=ov)
        else:
            U.check(gl, rl, fp32=ol)


def test_rejects_a_softmax_without_max_shift_under_large_logits():
    M, L, P = 4, len(SHAPES), 4
    v, s, refp, qproj = U.make_fused_case("large_logits", 2, M, 8, 60, P, SHAPES, seed=4)
    loc, a, dloc, da = U.fused_locations(s, refp, qproj, M, L, P)
    r = U.forward_reference(v, s, loc, a, dloc=dloc, da=da)
    floc, fa = fp32_fused_prologue(s, refp, qproj, M, L, P, shift=False)
    with pytest.raises(AssertionError):
        U.check(_oracle(v, s, floc, fa), r)
