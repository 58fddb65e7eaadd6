"""CPU: the yardsticks of tests/util_norm_attn_numerics.py tested on themselves, and every attention / LayerNorm / GroupNorm / box
refinement kernel run through the SIMT emulator (tests/emu_lib.py) against them on every operand profile.

Self-test: each bound ACCEPTS the fp32 torch formulation and fp32 sums taken in another order on every profile, and REJECTS every
mutant (a kernel that is subtly wrong in one of the ways kernels of this kind go wrong).  `softmax without the max shift` is
rejected on `huge` (scores of hundreds of nats overflow exp) but not on `peaked`: q, k x 4 gives scores of std 16 nats whose largest,
about 70, is below the 88 where fp32 exp overflows, so the unshifted formula is accurate there -- nothing to reject.

pytest -s prints the worst normalised excess of every case."""
import math

import numpy as np
import pytest
import torch

from tests import emu_lib
from tests import util_norm_attn_numerics as A
from tests import util_split_numerics as U

needs_emu = pytest.mark.skipif(not emu_lib.available(), reason="no host clang++ for the emulated library")


# ---- attention: the bound on itself ------------------------------------------------------------------------------------------------
def _attn_variant(q, k, v, scale, mask, p_dtype=None, s_dtype=None, no_shift=False, exp_err=0.0, drop_last_key=False, drop_tail=False,
                  count_masked=False, sum_before_mask=False, reorder=False):
    """softmax(scale q k^T) v in fp32 with one deliberate defect (or, reorder: the same sums in another order)."""
    qf, kf, vf = (t.float().permute(0, 2, 1, 3) for t in (q, k, v))
    dead = None if mask is None else (mask != 0).clone()
    if reorder:
        kf, vf = kf.flip(2), vf.flip(2)
        qf, kf = qf.flip(3), kf.flip(3)
        dead = None if dead is None else dead.flip(1)
    if drop_tail:
        s = (qf[..., :32] @ kf[..., :32].transpose(-1, -2)) * scale
    else:
        s = (qf @ kf.transpose(-1, -2)) * scale
    if s_dtype is not None:
        s = s.to(s_dtype).float()
    if dead is not None and count_masked:
        for n in range(dead.shape[0]):
            dead[n, int(dead[n].nonzero()[0])] = False
    shift = torch.zeros_like(s[..., :1])
    if not no_shift:
        sm = s if dead is None else s.masked_fill(dead[:, None, None, :], -math.inf)
        shift = sm.amax(-1, keepdim=True)
    e = (s - shift).exp()
    if exp_err:
        sign = torch.where(torch.rand(e.shape, generator=torch.Generator().manual_seed(1)) < 0.5, 1.0, -1.0)
        e = e * (1 + exp_err * sign)
    den_all = e.sum(-1, keepdim=True)
    if dead is not None:
        e = e.masked_fill(dead[:, None, None, :], 0.0)
    den = den_all if sum_before_mask else e.sum(-1, keepdim=True)
    p = e / den
    if p_dtype is not None:
        p = p.to(p_dtype).float()
    if drop_last_key:
        p = p.clone()
        p[..., -1] = 0
    return (p @ vf).permute(0, 2, 1, 3)


ATTN_SHAPE = (2, 35, 400, 2, 32)


def _attn_case(profile, shape=ATTN_SHAPE, masked=True):
    N, Lq, Lk, H, D = shape
    q, k, v, scale = A.attention_operands(profile, N, Lq, Lk, H, D, seed=Lk + D)
    mask = None
    if masked:
        mask = A.attention_masks(N, Lk, seed=Lk)
        mask[:, -1] = 0          # (the mutant that drops the last key needs it alive)
    return q, k, v, scale, mask, A.attention_reference(q, k, v, scale, mask)


@pytest.mark.parametrize("profile", A.ATTN_PROFILES)
def test_attention_bound_accepts_fp32(profile):
    q, k, v, scale, mask, r = _attn_case(profile)
    f32 = A.attention_fp32(q, k, v, scale, mask)
    _, w = A.excess(f32, r)
    print("attention  torch fp32      %-11s %s" % (profile, w))
    assert w.value <= A.BOUND, w
    _, w2 = A.excess(_attn_variant(q, k, v, scale, mask, reorder=True), r, f32)
    print("attention  reordered fp32  %-11s %s" % (profile, w2))
    assert A.passes(w2), w2
    assert float(r.T.max()) < 1e5 and bool((r.S[~r.zero] > 0).all())


ATTN_MUTANTS = {
    "bf16_weights": (dict(p_dtype=torch.bfloat16), ["unit", "voffset", "peaked"]),
    "fp16_weights": (dict(p_dtype=torch.float16), ["unit", "voffset"]),
    "fp16_scores": (dict(s_dtype=torch.float16), ["unit", "peaked", "qoffset"]),
    "no_max_shift": (dict(no_shift=True), ["huge"]),
    "exp_rel_err_2^-16": (dict(exp_err=2.0 ** -16), ["few_keys"]),
    "last_key_dropped": (dict(drop_last_key=True), ["unit", "tiny", "voffset"]),
    "masked_key_counted": (dict(count_masked=True), ["unit", "voffset"]),
    "sum_before_masking": (dict(sum_before_mask=True), ["unit", "voffset", "tiny"]),
}


@pytest.mark.parametrize("mutant", sorted(ATTN_MUTANTS))
def test_attention_bound_rejects(mutant):
    flags, profiles = ATTN_MUTANTS[mutant]
    for profile in profiles:
        if profile == "few_keys":   # errors of random sign in the exponentials average out over 400 keys; over 3 they do not
            q, k, v, scale, mask, r = _attn_case("unit", (2, 35, 3, 2, 32), masked=False)
        else:
            q, k, v, scale, mask, r = _attn_case(profile)
        f32 = A.attention_fp32(q, k, v, scale, mask)
        y = _attn_variant(q, k, v, scale, mask, **flags)
        if bool(torch.isnan(y).any()):      # (a NaN where none is expected is a rejection: U.excess asserts it)
            with pytest.raises(AssertionError):
                A.excess(y, r, f32)
            print("attention  %-20s %-11s NaN outputs: rejected" % (mutant, profile))
            continue
        _, w = A.excess(y, r, f32)
        print("attention  %-20s %-11s %s" % (mutant, profile, w))
        assert not A.passes(w), (mutant, profile, w)


def test_attention_bound_rejects_dropped_tail_channels_of_head_dim_36():
    q, k, v, scale, mask, r = _attn_case("unit", (1, 20, 100, 2, 36))
    f32 = A.attention_fp32(q, k, v, scale, mask)
    _, w = A.excess(_attn_variant(q, k, v, scale, mask, drop_tail=True), r, f32)
    print("attention  channels 32..35 dropped        %s" % w)
    assert not A.passes(w), w


def test_attention_fully_masked_rows_are_exact_zero_and_exempt():
    q, k, v, scale, mask, _ = _attn_case("unit", (2, 5, 40, 2, 16))
    mask[1] = 1
    r = A.attention_reference(q, k, v, scale, mask)
    assert bool(r.zero[1].all()) and not bool(r.zero[0].any())
    y = A.attention_fp32(q, k, v, scale, mask)
    y[1] = 0
    _, w = A.excess(y, r)
    assert w.value <= A.BOUND
    y[1, 2, 1, 3] = 1e-30
    with pytest.raises(AssertionError):
        A.excess(y, r)


# ---- norms: the bound on itself -----------------------------------------------------------------------------------------------------
def _norm_variant(z, gamma, beta, eps, groups, kind):
    """fp32 LayerNorm / GroupNorm with one deliberate defect (or, reordered: two-pass fp32 sums in another order)."""
    z = z.float()
    N, HW, C = z.shape
    if groups is None:
        view = lambda t: t                                       # noqa: E731
        back = lambda s: s                                       # noqa: E731
        cnt = C
    else:
        shift = 1 if kind == "group_shift" else 0
        view = lambda t: A._group_view(torch.roll(t, shift, -1), groups)            # noqa: E731
        back = lambda s: torch.roll(A._group_expand(s, HW, C), -shift, -1)          # noqa: E731
        cnt = HW * (C // groups)
    zg = view(z)
    if kind == "reordered":
        zg = zg.flip(-1)
    mean = zg.sum(-1, keepdim=True) / cnt
    if kind == "one_pass":
        var = ((zg * zg).sum(-1, keepdim=True) / cnt - mean * mean).clamp_min(0)
    else:
        var = ((zg - mean) ** 2).sum(-1, keepdim=True) / (cnt - 1 if kind == "unbiased" else cnt)
    rstd = 1 / (var.sqrt() + eps) if kind == "eps_outside" else 1 / (var + eps).sqrt()
    if kind == "bf16_stats":
        mean, rstd = mean.bfloat16().float(), rstd.bfloat16().float()
    return (z - back(mean)) * back(rstd) * gamma.float() + beta.float()


NORM_SHAPES = {"layernorm": (1, 300, 256, None), "groupnorm_256": (1, 300, 256, 32), "groupnorm_288": (2, 77, 288, 32)}


def _norm_case(profile, which):
    N, HW, C, G = NORM_SHAPES[which]
    x, res, gamma, beta = A.norm_operands(profile, N, HW, C, seed=HW + C, groups=G)
    return x, res, gamma, beta, G, A.norm_reference([x, res], gamma, beta, 1e-5, G)


NORM_ACCEPT = [(p, w) for w in sorted(NORM_SHAPES) for p in (A.LN_PROFILES if w == "layernorm" else A.NORM_PROFILES)]


@pytest.mark.parametrize("profile,which", NORM_ACCEPT, ids=["%s-%s" % c for c in NORM_ACCEPT])
def test_norm_bound_accepts_fp32(profile, which):
    x, res, gamma, beta, G, r = _norm_case(profile, which)
    f32 = A.norm_fp32([x, res], gamma, beta, 1e-5, G)
    _, w = A.excess(f32, r)
    print("%-14s torch fp32      %-11s %s" % (which, profile, w))
    assert w.value <= A.BOUND, w
    z = x if res is None else x + res
    _, w2 = A.excess(_norm_variant(z, gamma, beta, 1e-5, G, "reordered"), r, f32)
    print("%-14s reordered fp32  %-11s %s" % (which, profile, w2))
    assert A.passes(w2), w2
    if profile == "constant":   # var = 0: the reference is exactly beta there
        if G is None:
            got, want = r.ref[:, ::3], beta.double().expand_as(r.ref[:, ::3])
        else:
            got, want = r.ref[-1], beta.double().expand_as(r.ref[-1])
        assert bool((got == want).all())


NORM_MUTANTS = {
    "one_pass": ["offset30", "offset300", "offset3000"],
    "unbiased": ["unit", "chan_spread"],
    "eps_outside": ["unit", "small_1e-4", "small_1e-6"],
    "bf16_stats": ["unit", "offset30", "large"],
}


@pytest.mark.parametrize("which", sorted(NORM_SHAPES))
@pytest.mark.parametrize("mutant", sorted(NORM_MUTANTS))
def test_norm_bound_rejects(mutant, which):
    for profile in NORM_MUTANTS[mutant]:
        x, res, gamma, beta, G, r = _norm_case(profile, which)
        f32 = A.norm_fp32([x, res], gamma, beta, 1e-5, G)
        _, w = A.excess(_norm_variant(x, gamma, beta, 1e-5, G, mutant), r, f32)
        print("%-14s %-12s %-11s %s" % (which, mutant, profile, w))
        assert not A.passes(w), (mutant, profile, w)
        if mutant == "one_pass":     # the statistics pass with fp32 partial sums, in effect: above the fixed bound on its own
            assert w.value > A.BOUND, w


def test_norm_bound_rejects_group_boundaries_off_by_one_channel():
    """C = 288, G = 32: 9 channels per group, a 16-byte quad straddles two groups."""
    for profile in ("unit", "chan_spread", "offset30"):
        x, res, gamma, beta, G, r = _norm_case(profile, "groupnorm_288")
        f32 = A.norm_fp32([x, res], gamma, beta, 1e-5, G)
        _, w = A.excess(_norm_variant(x, gamma, beta, 1e-5, G, "group_shift"), r, f32)
        print("groupnorm_288  group_shift  %-11s %s" % (profile, w))
        assert not A.passes(w), (profile, w)


def test_box_refine_bound_on_itself():
    for ref_dim in (2, 4):
        delta, ref = A.box_refine_operands(64, ref_dim, seed=ref_dim)
        want = A.box_refine_reference(delta, ref, 1e-5)
        A.check_box_refine(A.box_refine_reference(delta, ref, 1e-5, torch.float32), delta, ref, 1e-5, "torch fp32, ref_dim %d" % ref_dim)
        assert float(want[8].min()) == 1.0 and float(want[9].max()) < 1e-40        # delta = +-100 saturates, no NaN
        with pytest.raises(AssertionError):                                        # a bf16-class sigmoid
            A.check_box_refine(want.bfloat16(), delta, ref, 1e-5)
        with pytest.raises(AssertionError):                                        # the clamp of the reference forgotten
            rd = ref.double()
            bad = torch.sigmoid(delta.double() + torch.nn.functional.pad(torch.log(rd.clamp_min(1e-5) / (1 - rd).clamp_min(1e-5)),
                                                                         (0, 4 - ref_dim)))
            A.check_box_refine(bad, delta, ref, 1e-5)


# ---- the kernels on the emulator -----------------------------------------------------------------------------------------------------
MFMA = [1, 2, 0]
MFMA_IDS = ["stream", "lds_staged", "vector"]


def _emu_attention(mfma, q, k, v, scale, mask, **kw):
    prev = emu_lib.set_options(mha_mfma=mfma)
    try:
        return torch.from_numpy(emu_lib.mha_core(q.numpy(), k.numpy(), v.numpy(), scale, None if mask is None else mask.numpy(), **kw))
    finally:
        emu_lib.set_options(**prev)


@needs_emu
@pytest.mark.parametrize("mfma", MFMA, ids=MFMA_IDS)
@pytest.mark.parametrize("profile", A.ATTN_PROFILES)
def test_emulated_attention_profiles(profile, mfma):
    q, k, v, scale, mask, r = _attn_case(profile)
    y = _emu_attention(mfma, q, k, v, scale, mask)
    A.check(y, r, A.attention_fp32(q, k, v, scale, mask), "emu mha_core[%s] %s %s" % (MFMA_IDS[MFMA.index(mfma)], profile, ATTN_SHAPE))


EMU_ATTN_EDGES = [  # N, Lq, Lk, H, D, profile, strides
    (1, 17, 513, 1, 32, "peaked", dict(ldv=40, ldo=36)),
    (1, 16, 1025, 1, 36, "unit", dict(ldv=44, ldo=40)),
    (1, 5, 2100, 1, 16, "voffset", dict(ldq=20, ldk=24)),
    (2, 40, 40, 2, 64, "qoffset", dict(packed_qk=True, ldv=136, ldo=132)),
    (3, 1, 15, 8, 16, "row_spread", dict(ldv=136, ldo=132)),
    (1, 33, 1024, 1, 32, "tiny", dict()),
]


@needs_emu
@pytest.mark.parametrize("mfma", MFMA, ids=MFMA_IDS)
@pytest.mark.parametrize("case", EMU_ATTN_EDGES, ids=["%dx%dx%dx%dx%d_%s" % c[:6] for c in EMU_ATTN_EDGES])
def test_emulated_attention_edges_and_strides(case, mfma):
    """Lq != Lk, operands in strided buffers (NaN in the gaps of q / k / v, a canary in the gaps of out and behind it), key counts on
    both sides of where tf_mha_core_f32 changes kernels."""
    N, Lq, Lk, H, D, profile, strides = case
    q, k, v, scale, mask, r = _attn_case(profile, (N, Lq, Lk, H, D))
    y = _emu_attention(mfma, q, k, v, scale, mask, **strides)
    A.check(y, r, A.attention_fp32(q, k, v, scale, mask), "emu mha_core[%s] %s %s" % (MFMA_IDS[MFMA.index(mfma)], profile, case[:5]))


@needs_emu
@pytest.mark.parametrize("rows,C", [(37, 256), (5, 8), (9, 288), (3, 1024), (2, 4096)])
@pytest.mark.parametrize("profile", A.LN_PROFILES)
def test_emulated_add_layernorm(profile, rows, C):
    x, res, gamma, beta = A.norm_operands(profile, 1, rows, C, seed=rows + C)
    if res is None and rows % 2:          # with and without a residual
        res = torch.randn(1, rows, C, generator=torch.Generator().manual_seed(C)) * float(x.std())
    r = A.norm_reference([x, res], gamma, beta, 1e-5)
    y = emu_lib.add_layernorm(x[0].numpy(), None if res is None else res[0].numpy(), gamma.numpy(), beta.numpy())
    A.check(torch.from_numpy(y)[None], r, A.norm_fp32([x, res], gamma, beta, 1e-5), "emu add_layernorm %s %dx%d" % (profile, rows, C))


EMU_GN = [(1, 300, 256, 32, 0), (2, 77, 288, 32, 8), (3, 1, 64, 8, 0), (2, 100, 16, 8, 4)]


@needs_emu
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("N,HW,C,G,gap", EMU_GN, ids=["%dx%dx%d_g%d_gap%d" % s for s in EMU_GN])
@pytest.mark.parametrize("profile", A.NORM_PROFILES)
def test_emulated_groupnorm(profile, N, HW, C, G, gap, relu):
    """tf_groupnorm_nhwc_f32 / tf_groupnorm_relu_nhwc_f32.  With fp32 partial sums in the statistics pass (as it was before this test
    existed) the offset profiles fail here: the variance of a group whose |mean| is 30 / 300 / 3000 std is lost."""
    x, _, gamma, beta = A.norm_operands(profile, N, HW, C, seed=HW + C, groups=G)
    r = A.norm_reference([x], gamma, beta, 1e-5, G, relu)
    y = emu_lib.groupnorm_nhwc(x.numpy(), gamma.numpy(), beta.numpy(), G, relu=relu, gap=gap)
    A.check(torch.from_numpy(y), r, A.norm_fp32([x], gamma, beta, 1e-5, G, relu),
            "emu groupnorm%s %s %s" % ("_relu" if relu else "", profile, (N, HW, C, G)))


@needs_emu
@pytest.mark.parametrize("profile", ["unit", "offset3000", "chan_spread"])
def test_emulated_groupnorm_long_groups(profile):
    """HW = 4000, C = 32, G = 8: 16 000 elements per group, 63 workgroups' partial sums per image."""
    x, _, gamma, beta = A.norm_operands(profile, 1, 4000, 32, seed=4032, groups=8)
    r = A.norm_reference([x], gamma, beta, 1e-5, 8)
    y = emu_lib.groupnorm_nhwc(x.numpy(), gamma.numpy(), beta.numpy(), 8)
    A.check(torch.from_numpy(y), r, A.norm_fp32([x], gamma, beta, 1e-5, 8), "emu groupnorm %s (1, 4000, 32, 8)" % profile)


def _c1_operands(profile, n, H, W, C, G, seed):
    x, _, gamma, beta = A.norm_operands(profile, n, H * W, C, seed=seed, groups=G)
    g = torch.Generator().manual_seed(seed + 1)
    w = torch.randn(1, 3, 3, C, generator=g) / (3 * C ** 0.5)
    return x, gamma, beta, w, 0.25


@needs_emu
@pytest.mark.parametrize("C,G", [(16, 8), (32, 8)])
@pytest.mark.parametrize("profile", A.NORM_PROFILES)
def test_emulated_groupnorm_relu_conv3x3_c1(profile, C, G):
    n, H, W = 3, 9, 35
    x, gamma, beta, w, bias = _c1_operands(profile, n, H, W, C, G, seed=C + H)
    r, f32 = A.c1_reference(x, gamma, beta, w, bias, n, H, W, C, G)
    y = emu_lib.groupnorm_relu_conv3x3_c1(x.reshape(n, H, W, C).numpy(), gamma.numpy(), beta.numpy(), w.reshape(9, C).numpy(), bias, G)
    A.check(torch.from_numpy(y)[..., None], r, f32, "emu groupnorm_relu_conv3x3_c1 %s C %d" % (profile, C))


@needs_emu
@pytest.mark.parametrize("terms", [6, 16])
@pytest.mark.parametrize("profile", ["unit", "offset30", "offset300", "offset3000", "chan_spread", "constant"])
def test_emulated_conv3x3_merge_with_folded_groupnorm(profile, terms):
    """tf_conv3x3_merge_packed_f32 with relu(GroupNorm(low)) applied in its fetch from the statistics pass's raw sums: the norm's
    bound carried through |w| next to the split product's own (tests/util_split_numerics.py)."""
    n, lh, lw, H, W, cin, cout, G = 2, 5, 6, 10, 12, 32, 16, 8
    low, _, gamma, beta = A.norm_operands(profile, n, lh * lw, cin, seed=cin + lh, groups=G)
    low = low.reshape(n, lh, lw, cin)
    g = torch.Generator().manual_seed(7)
    fpn = torch.randn(1, H, W, cin, generator=g)
    w = torch.randn(cout, 3, 3, cin, generator=g) / (3 * cin ** 0.5)
    b = torch.randn(cout, generator=g)
    prev = emu_lib.set_terms(terms)
    try:
        y = emu_lib.conv3x3_merged(low.numpy(), fpn.numpy(), n, w.numpy(), b.numpy(), gn=(gamma.numpy(), beta.numpy(), G, 1e-5))
    finally:
        emu_lib.set_terms(prev)
    ref, S, floor, nan, k = A.merged_reference(low, fpn, gamma, beta, G, w, b, terms)
    worst = U.check(torch.from_numpy(y).reshape(-1, cout), ref, S, floor, nan, k=k)
    print("emu conv3x3_merge + groupnorm  terms %d  %-11s %s" % (terms, profile, worst))


@needs_emu
@pytest.mark.parametrize("ref_dim", [2, 4])
def test_emulated_box_refine(ref_dim):
    delta, ref = A.box_refine_operands(300, ref_dim, seed=ref_dim)
    delta[20, 1] = float("nan")
    y = torch.from_numpy(emu_lib.box_refine(delta.numpy(), ref.numpy(), 1e-5))
    A.check_box_refine(y, delta, ref, 1e-5, "emu box_refine ref_dim %d" % ref_dim)
    assert int(torch.isnan(y).sum()) == 1 and bool(torch.isnan(y[20, 1]))
    assert bool((y[8] == 1).all()) and bool((y[9] == 0).all())         # delta = +-100 saturates: exactly 1 / 0, not NaN
    assert bool((y[10] == 1).all()) and bool((y[11] < 1e-37).all())


@needs_emu
@pytest.mark.parametrize("profile", ["unit", "offset3000", "chan_spread", "constant"])
def test_emulated_groupnorm_statistics(profile):
    """tf_groupnorm_stats_nhwc_f32 against the float64 sums within A.check_group_sums' bound."""
    N, HW, C, G = 2, 77, 288, 32
    x, _, _, _ = A.norm_operands(profile, N, HW, C, seed=1, groups=G)
    xs = emu_lib._aligned(x.numpy())
    ws = np.full(2 * N * G, np.nan, np.float64)
    rc = emu_lib.lib().tf_groupnorm_stats_nhwc_f32(xs.ctypes.data, ws.ctypes.data, N, HW, C, G, HW * C, None)
    assert rc == 0
    A.check_group_sums(torch.from_numpy(ws), x, G, "emu groupnorm_stats %s" % profile)
