"""GPU (-m gpu): the attention core (tf_mha_core_f32: all three kernels), the LayerNorm / GroupNorm kernels and the box refinement on
the MI355X against float64 computed on the device, with the per-output bounds of tests/util_norm_attn_numerics.py:

    attention   (|y - ref| - floor) / (S (1 + T)) <= 2^-20      norms   |y - ref| / Sn <= 2^-20

and at most 4 x the excess of the fp32 torch formulation on the same operands (2^-23 where that is as good as exact).  Attention runs
through the C ABI on every head dimension, on both sides of every key count at which tf_mha_core_f32 changes kernels, with Lq != Lk,
strided operands (NaN in the gaps of V, a canary in the gaps of the output and behind it), a different mask per image, and its
non-finite contract; the norms on every operand profile at the model's shapes.  Each case prints its worst normalised excess next to
the fp32 torch formulation's own (pytest -s).

MEASURED on an MI355X (the first hardware figures of these kernels): the worst normalised excess per kernel and profile over all cases
of this module, the fp32 torch formulation's own on the same operands in brackets.  Everything is at or below 6.1e-7 (2^-20 = 9.5e-7) and
within 2.7 x the fp32 torch figure next to it; the matrix-core attention kernels' largest figures are on `qoffset` (a common offset of
110 nats and more in the scores: T is large and the score sums carry u T) and `huge`; no instruction needed a term in the floor.

attention, (|y - ref| - floor) / (S (1 + T)):
                                unit                peaked              huge                voffset             tiny                qoffset             row_spread
    mha_core[stream]            8.5e-08 (8.7e-08)   1.7e-07 (1.6e-07)   2.2e-07 (8.3e-08)   8.1e-08 (2.8e-07)   1.9e-07 (1.8e-07)   6.1e-07 (3.9e-07)   2.2e-07 (2.4e-07)
    mha_core[lds_staged]        8.2e-08 (8.7e-08)   1.9e-07 (1.6e-07)   2.1e-07 (8.3e-08)   8.8e-08 (2.8e-07)   1.9e-07 (1.8e-07)   5.8e-07 (3.9e-07)   2.5e-07 (1.6e-07)
    mha_core[vector]            5.6e-08 (6.6e-08)   1.1e-07 (1.6e-07)   6.4e-08 (1.8e-07)   1.5e-07 (2.8e-07)   2.0e-07 (1.8e-07)   2.4e-07 (3.7e-07)   1.5e-07 (1.6e-07)
norms, |y - ref| / Sn:
                                unit                offset30            offset300           offset3000          small_1e-4
    add_layernorm               2.0e-07 (2.3e-07)   1.4e-07 (1.5e-07)   1.5e-07 (1.8e-07)   1.2e-07 (1.2e-07)   8.5e-08 (7.9e-08)
    groupnorm                   1.8e-07 (2.1e-07)   4.2e-08 (1.3e-07)   5.2e-08 (1.6e-07)   4.1e-08 (1.4e-07)   9.5e-08 (1.2e-07)
    groupnorm_relu              1.8e-07 (2.1e-07)   4.1e-08 (1.2e-07)   5.2e-08 (1.6e-07)   4.1e-08 (1.4e-07)   8.4e-08 (1.2e-07)
    groupnorm(strided)          1.5e-07 (1.7e-07)   -                   5.1e-08 (1.4e-07)   4.0e-08 (1.1e-07)   -
    groupnorm_relu_conv3x3_c1   5.6e-08 (8.2e-08)   7.6e-09 (1.9e-08)   1.4e-08 (2.2e-08)   8.2e-09 (1.7e-08)   2.8e-08 (5.2e-08)

                                small_1e-6          large               chan_spread         constant            cancel
    add_layernorm               6.0e-08 (6.0e-08)   1.9e-07 (2.0e-07)   2.0e-07 (2.2e-07)   2.0e-07 (2.3e-07)   1.5e-07 (1.5e-07)
    groupnorm                   6.0e-08 (1.2e-07)   1.6e-07 (1.9e-07)   1.7e-07 (2.0e-07)   1.8e-07 (2.1e-07)   -
    groupnorm_relu              6.0e-08 (1.2e-07)   1.5e-07 (1.7e-07)   1.7e-07 (2.0e-07)   1.7e-07 (2.0e-07)   -
    groupnorm(strided)          -                   -                   1.5e-07 (1.5e-07)   -                   -
    groupnorm_relu_conv3x3_c1   4.0e-08 (5.2e-08)   4.4e-08 (9.3e-08)   6.4e-08 (1.2e-07)   2.4e-09 (1.4e-08)   -

box refinement: max |y - ref| / max(y, 1 - y) = 2.3e-7 (torch fp32: 2.6e-7); the statistics pass's (sum, sum of squares): 1.4e-3 of
the bound of n 2^-53 sum |x| (sum x^2); conv3x3_merged with the folded GroupNorm: within the carried bound on every profile and both
split products.  With fp32 partial sums in the statistics pass (the kernel before this module existed) 41 of the GroupNorm cases fail:
offset30 (2, 273, 288, 32) is at 1.9e-6 (y -4.984151 for -4.984227), offset300 and offset3000 at every shape."""
import ctypes

import pytest
import torch

from tests import util_norm_attn_numerics as A
from tests import util_split_numerics as U

pytestmark = pytest.mark.gpu

MFMA = [1, 2, 0]
MFMA_IDS = ["stream", "lds_staged", "vector"]
CANARY = -1234.5
BAD_DIMS = -2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from trackformer_amd import _cabi
    _cabi.lib()
    return torch.device("cuda:0")


@pytest.fixture(params=MFMA, ids=MFMA_IDS)
def mfma(request):
    from trackformer_amd import _cabi
    prev = _cabi.lib().tf_msda_set_option(b"mha_mfma", request.param)
    try:
        yield MFMA_IDS[MFMA.index(request.param)]
    finally:
        _cabi.lib().tf_msda_set_option(b"mha_mfma", prev)


# ---- attention ---------------------------------------------------------------------------------------------------------------------
def _mha(q, k, v, scale, mask, expect=0):
    """tf_mha_core_f32 on strided device buffers: q | k packed in one buffer (ld 2 E) when Lq == Lk, else buffers of their own with
    NaN gaps; ldv = E + 8 with NaN in the gaps; ldo = E + 4 with a canary in the gaps and in three rows behind row N Lq."""
    from trackformer_amd import _cabi, fused
    N, Lq, H, D = q.shape
    Lk, E, dev = k.shape[1], H * D, q.device
    nan = float("nan")
    if Lq == Lk:
        qk = torch.cat([q.reshape(N * Lq, E), k.reshape(N * Lk, E)], 1).contiguous()
        qp, kp, ldq, ldk = qk.data_ptr(), qk.data_ptr() + 4 * E, 2 * E, 2 * E
    else:
        qb = torch.full((N * Lq, E + 4), nan, device=dev)
        kb = torch.full((N * Lk, E + 12), nan, device=dev)
        qb[:, :E], kb[:, :E] = q.reshape(N * Lq, E), k.reshape(N * Lk, E)
        qp, kp, ldq, ldk = qb.data_ptr(), kb.data_ptr(), E + 4, E + 12
    vb = torch.full((N * Lk, E + 8), nan, device=dev)
    vb[:, :E] = v.reshape(N * Lk, E)
    ob = torch.full((N * Lq + 3, E + 4), CANARY, device=dev)
    mk = None if mask is None else mask.to(torch.uint8).contiguous()
    rc = _cabi.lib().tf_mha_core_f32(qp, kp, vb.data_ptr(), ob.data_ptr(), 0 if mk is None else mk.data_ptr(), N, Lq, Lk, H, D, ldq, ldk,
                                     E + 8, E + 4, ctypes.c_float(scale), fused._stream(dev))
    torch.cuda.synchronize()
    assert rc == expect, "tf_mha_core_f32: status %d" % rc
    assert bool((ob[:N * Lq, E:] == CANARY).all()) and bool((ob[N * Lq:] == CANARY).all()), "tf_mha_core_f32 wrote outside its rows"
    return ob[:N * Lq, :E].reshape(N, Lq, H, D).clone()


def _edge_cases():
    cases, i = [], 0
    lqs, ns, hs = [1, 15, 16, 17, 400], [1, 3], [1, 8]
    for D in (16, 32, 36, 64):
        for Lk in [1, 15, 16, 17, 63, 64, 65] + ([511, 512, 513, 1023, 1024, 1025] if D <= 36 else [255, 256, 257, 511, 512, 513]):
            cases.append((ns[i % 2], lqs[i % 5], Lk, hs[(i // 2) % 2], D))
            i += 1
    cases += [(1, 16, 16, 8, 32), (1, 400, 400, 8, 32), (3, 17, 17, 1, 36), (1, 15, 15, 8, 64), (1, 1, 1, 1, 16)]   # Lq == Lk: q | k packed
    cases += [(3, 400, 300, 8, 32), (1, 560, 1030, 8, 36), (2, 400, 600, 8, 64)]    # > 256 workgroups: the kc = 64 branches
    cases += [(1, 17, 2300, 1, 16), (1, 16, 2240, 1, 32), (1, 33, 2241, 1, 32), (1, 5, 2254, 1, 32), (1, 9, 2126, 1, 64)]   # the most LDS holds
    return cases


EDGE_CASES = _edge_cases()


@pytest.mark.parametrize("N,Lq,Lk,H,D", EDGE_CASES, ids=["%dx%dx%dx%dx%d" % c for c in EDGE_CASES])
def test_attention_dispatch_edges(dev, mfma, N, Lq, Lk, H, D):
    profile = A.ATTN_PROFILES[(Lq + Lk + D) % len(A.ATTN_PROFILES)]
    q, k, v, scale = A.attention_operands(profile, N, Lq, Lk, H, D, seed=Lq + Lk + D, device=dev)
    mask = A.attention_masks(N, Lk, seed=Lk, device=dev) if Lk > 1 else None
    y = _mha(q, k, v, scale, mask)
    w = A.check(y, A.attention_reference(q, k, v, scale, mask), A.attention_fp32(q, k, v, scale, mask),
                "EXCESS mha_core[%s] %s %s" % (mfma, profile, (N, Lq, Lk, H, D)))
    assert w.value <= A.BOUND


@pytest.mark.parametrize("shape", [(1, 400, 400, 8, 32), (1, 800, 800, 8, 36)], ids=["400x400x8x32", "800x800x8x36"])
@pytest.mark.parametrize("profile", A.ATTN_PROFILES)
def test_attention_profiles(dev, mfma, profile, shape):
    N, Lq, Lk, H, D = shape
    q, k, v, scale = A.attention_operands(profile, N, Lq, Lk, H, D, seed=Lk + D, device=dev)
    mask = A.attention_masks(N, Lk, seed=Lk, device=dev)
    y = _mha(q, k, v, scale, mask)
    A.check(y, A.attention_reference(q, k, v, scale, mask), A.attention_fp32(q, k, v, scale, mask),
            "EXCESS mha_core[%s] %s %s" % (mfma, profile, shape))


@pytest.mark.parametrize("D,Lk", [(32, 2255), (64, 2129), (16, 2321)])
def test_attention_more_keys_than_lds_holds_is_an_argument_error(dev, mfma, D, Lk):
    """One key more than the score tile has LDS for: TF_MSDA_ERR_BAD_DIMS from the argument check (nothing is launched, the output
    buffer keeps its canary), and fused.mha_core -> None."""
    from trackformer_amd import fused
    q, k, v, scale = A.attention_operands("unit", 1, 3, Lk, 1, D, seed=1, device=dev)
    y = _mha(q, k, v, scale, None, expect=BAD_DIMS)
    assert bool((y == CANARY).all())
    if D == 32:
        qk = torch.randn(1, 2300, 2 * 8 * D, device=dev)
        assert fused.mha_core(qk, torch.randn(1, 2300, 8 * D, device=dev), 8) is None
        assert fused.mha_core(qk[:, :400].contiguous(), torch.randn(1, 400, 8 * D, device=dev), 8) is not None


SEMANTIC = [(3, 40, 70, 2, 32), (3, 17, 600, 2, 36), (3, 20, 1100, 1, 16), (3, 33, 300, 2, 64)]


@pytest.mark.parametrize("N,Lq,Lk,H,D", SEMANTIC, ids=["%dx%dx%dx%dx%d" % c for c in SEMANTIC])
def test_attention_masked_and_non_finite_contract(dev, mfma, N, Lq, Lk, H, D):
    q, k, v, scale = A.attention_operands("unit", N, Lq, Lk, H, D, seed=D + Lk, device=dev)
    mask = A.attention_masks(N, Lk, seed=Lk, device=dev)
    # every key of image 1 masked: exactly zero (torch: NaN); a third of the rows, the only ones outside the bound
    mask[1] = 1
    r = A.attention_reference(q, k, v, scale, mask)
    assert bool(r.zero[1].all()) and not bool(r.zero[0].any()) and not bool(r.zero[2].any())
    base = _mha(q, k, v, scale, mask)
    assert bool((base[1] == 0).all())
    A.check(base, r, A.attention_fp32(q, k, v, scale, mask), "EXCESS mha_core[%s] masked image %s" % (mfma, (N, Lq, Lk, H, D)))
    # a masked key whose K row holds NaN / Inf changes nothing: bit-equal to the same call with that row zeroed
    dead = [int(j) for j in mask[0].nonzero()[:3, 0]]
    kz, kn = k.clone(), k.clone()
    kz[0, dead] = 0
    kn[0, dead[0]] = float("nan")
    kn[0, dead[1]] = float("inf")
    kn[0, dead[2], :, ::2] = float("-inf")
    assert torch.equal(_mha(q, kn, v, scale, mask), _mha(q, kz, v, scale, mask))
    # NaN in one query row makes only that row of that head NaN
    qn = q.clone()
    qn[2, Lq // 2, H - 1, 3] = float("nan")
    y = _mha(qn, k, v, scale, mask)
    want_nan = torch.zeros_like(y, dtype=torch.bool)
    want_nan[2, Lq // 2, H - 1] = True
    assert torch.equal(torch.isnan(y), want_nan)
    assert torch.equal(y[~want_nan], base[~want_nan])
    # NaN in v[n, j, h, c] of an unmasked key makes channel c of head h of image n NaN and nothing else
    j = int((mask[0] == 0).nonzero()[-1, 0])
    vn = v.clone()
    vn[0, j, 0, D - 1] = float("nan")
    y = _mha(q, k, vn, scale, mask)
    want_nan = torch.zeros_like(y, dtype=torch.bool)
    want_nan[0, :, 0, D - 1] = True
    assert torch.equal(torch.isnan(y), want_nan)
    assert torch.equal(y[~want_nan], base[~want_nan])


def test_mha_core_wrapper_declines_additive_float_masks(dev):
    """nn.MultiheadAttention takes a float key_padding_mask as ADDITIVE (-inf = ignore, 0 = keep); read as "non-zero = ignore" it
    would keep exactly the wrong keys."""
    from trackformer_amd import fused
    qk, v = torch.randn(2, 40, 512, device=dev), torch.randn(2, 40, 256, device=dev)
    keep = torch.zeros(2, 40, dtype=torch.bool, device=dev)
    keep[1, 30:] = True
    add = torch.zeros(2, 40, device=dev).masked_fill(keep, float("-inf"))
    assert fused.mha_core(qk, v, 8, add) is None
    assert fused.mha_core(qk, v, 8, add.half()) is None
    assert fused.mha_core(qk, v, 8, keep.long()) is None
    a, b = fused.mha_core(qk, v, 8, keep), fused.mha_core(qk, v, 8, keep.to(torch.uint8))
    assert a is not None and torch.equal(a, b)


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------
def _layernorm_module(gamma, beta):
    ln = torch.nn.LayerNorm(gamma.numel()).to(gamma.device)
    with torch.no_grad():
        ln.weight.copy_(gamma)
        ln.bias.copy_(beta)
    return ln


LN_GRID = [(rows, C) for C in (8, 256, 288, 1024, 4096) for rows in (1, 7, 22223)]


@pytest.mark.parametrize("rows,C", LN_GRID, ids=["%dx%d" % s for s in LN_GRID])
def test_add_layernorm_shapes(dev, rows, C):
    """fused.add_layernorm on the grid of row lengths (every MAXCH instantiation) and row counts, with and without a residual, and
    through the C ABI with out aliasing x."""
    from trackformer_amd import _cabi, fused
    profile = A.LN_PROFILES[(rows + C // 8) % len(A.LN_PROFILES)]
    x, res, gamma, beta = A.norm_operands(profile, 1, rows, C, seed=rows + C, device=dev)
    ln = _layernorm_module(gamma, beta)
    extra = torch.randn(1, rows, C, generator=torch.Generator().manual_seed(C)).to(dev) * float(x.std().nan_to_num(1.0))
    for r_in in ([res] if res is not None else [None, extra]):
        with torch.no_grad():
            y = fused.add_layernorm(x, r_in, ln)
        assert y is not None
        r = A.norm_reference([x, r_in], gamma, beta, ln.eps)
        A.check(y, r, A.norm_fp32([x, r_in], gamma, beta, ln.eps), "EXCESS add_layernorm %s %dx%d%s" % (profile, rows, C, "" if r_in is None else " +res"))
        alias = x.clone()
        rc = _cabi.lib().tf_add_layernorm_f32(alias.data_ptr(), 0 if r_in is None else r_in.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                              alias.data_ptr(), rows, C, ctypes.c_float(ln.eps), fused._stream(dev))
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(alias, y)


@pytest.mark.parametrize("rows,C", [(22223, 256), (7, 288), (400, 1024)], ids=["22223x256", "7x288", "400x1024"])
@pytest.mark.parametrize("profile", A.LN_PROFILES)
def test_add_layernorm_profiles(dev, profile, rows, C):
    from trackformer_amd import fused
    x, res, gamma, beta = A.norm_operands(profile, 1, rows, C, seed=rows + C + 1, device=dev)
    ln = _layernorm_module(gamma, beta)
    with torch.no_grad():
        y = fused.add_layernorm(x, res, ln)
    assert y is not None
    A.check(y, A.norm_reference([x, res], gamma, beta, ln.eps), A.norm_fp32([x, res], gamma, beta, ln.eps),
            "EXCESS add_layernorm %s %dx%d" % (profile, rows, C))


def test_add_layernorm_declines_other_parameter_types(dev):
    from trackformer_amd import fused
    x = torch.randn(1, 5, 256, device=dev)
    assert fused.add_layernorm(x, None, torch.nn.LayerNorm(256).to(dev)) is not None
    assert fused.add_layernorm(x, None, torch.nn.LayerNorm(256).to(dev).half()) is None
    assert fused.add_layernorm(x, None, torch.nn.LayerNorm(256).to(dev).double()) is None
    assert fused.add_layernorm(x, None, torch.nn.LayerNorm(256)) is None            # parameters on the CPU
    mixed = torch.nn.LayerNorm(256).to(dev)
    mixed.bias = torch.nn.Parameter(mixed.bias.detach().cpu())
    assert fused.add_layernorm(x, None, mixed) is None


# ---- GroupNorm -------------------------------------------------------------------------------------------------------------------------
def _groupnorm_module(gamma, beta, G):
    gn = torch.nn.GroupNorm(G, gamma.numel()).to(gamma.device)
    with torch.no_grad():
        gn.weight.copy_(gamma)
        gn.bias.copy_(beta)
    return gn


# N, HW, C, G: the input projection's largest level, hidden 288 (9 channels per group: a 16-byte quad straddles two groups), the mask
# head's GroupNorms over ~100 queries, one pixel
GN_SHAPES = [(1, 100 * 167, 256, 32), (2, 13 * 21, 288, 32), (100, 100 * 167, 16, 8), (100, 50 * 84, 32, 8), (100, 25 * 42, 64, 8),
             (100, 13 * 21, 128, 8), (3, 1, 64, 8)]


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("N,HW,C,G", GN_SHAPES, ids=["%dx%dx%d_g%d" % s for s in GN_SHAPES])
@pytest.mark.parametrize("profile", A.NORM_PROFILES)
def test_groupnorm(dev, profile, N, HW, C, G, relu):
    """fused.groupnorm_nhwc (tf_groupnorm_nhwc_f32 / tf_groupnorm_relu_nhwc_f32).  With fp32 partial sums in the statistics pass the
    offset profiles fail here (the variance of a group whose |mean| is 30 / 300 / 3000 std is lost)."""
    from trackformer_amd import fused
    x, _, gamma, beta = A.norm_operands(profile, N, HW, C, seed=HW + C, device=dev, groups=G)
    gn = _groupnorm_module(gamma, beta, G)
    with torch.no_grad():
        y = fused.groupnorm_nhwc(x.reshape(N * HW, C), N, gn, relu=relu)
    assert y is not None
    A.check(y, A.norm_reference([x], gamma, beta, gn.eps, G, relu), A.norm_fp32([x], gamma, beta, gn.eps, G, relu),
            "EXCESS groupnorm%s %s %s" % ("_relu" if relu else "", profile, (N, HW, C, G)))


@pytest.mark.parametrize("profile", ["unit", "offset300", "offset3000", "chan_spread"])
def test_groupnorm_strided_images_and_statistics(dev, profile):
    """x_image_stride larger than HW C with NaN between the images (C ABI), and the statistics pass alone: its (sum, sum of squares)
    against the float64 sums."""
    from trackformer_amd import _cabi, fused
    N, HW, C, G, gap = 3, 273, 288, 32, 64
    x, _, gamma, beta = A.norm_operands(profile, N, HW, C, seed=5, device=dev, groups=G)
    xs = torch.full((N, HW * C + gap), float("nan"), device=dev)
    xs[:, :HW * C] = x.reshape(N, HW * C)
    out = torch.full((N, HW * C + 2 * gap), CANARY, device=dev)
    ws = torch.full((2 * N * G,), float("nan"), dtype=torch.float64, device=dev)
    rc = _cabi.lib().tf_groupnorm_nhwc_f32(xs.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), ws.data_ptr(), N, HW, C, G,
                                           ctypes.c_float(1e-5), HW * C + gap, HW * C + 2 * gap, fused._stream(dev))
    torch.cuda.synchronize()
    assert rc == 0 and bool((out[:, HW * C:] == CANARY).all())
    A.check(out[:, :HW * C].reshape(N, HW, C), A.norm_reference([x], gamma, beta, 1e-5, G), A.norm_fp32([x], gamma, beta, 1e-5, G),
            "EXCESS groupnorm(strided) %s %s" % (profile, (N, HW, C, G)))
    ws2 = torch.full_like(ws, float("nan"))
    rc = _cabi.lib().tf_groupnorm_stats_nhwc_f32(xs.data_ptr(), ws2.data_ptr(), N, HW, C, G, HW * C + gap, fused._stream(dev))
    torch.cuda.synchronize()
    assert rc == 0
    A.check_group_sums(ws2, x, G, "EXCESS groupnorm_stats %s" % profile)


@pytest.mark.parametrize("C,G,n,H,W", [(16, 8, 100, 100, 167), (32, 8, 100, 50, 84), (16, 8, 3, 9, 35)])
@pytest.mark.parametrize("profile", A.NORM_PROFILES)
def test_groupnorm_relu_conv3x3_c1(dev, profile, C, G, n, H, W):
    """fused.groupnorm_relu_conv3x3_c1 (the end of the mask head): the norm's bound carried through |w|."""
    from trackformer_amd import fused
    x, _, gamma, beta = A.norm_operands(profile, n, H * W, C, seed=C + H, device=dev, groups=G)
    gn = _groupnorm_module(gamma, beta, G)
    conv = torch.nn.Conv2d(C, 1, 3, padding=1).to(dev)
    w = conv.weight.detach().permute(0, 2, 3, 1).contiguous()        # [1, 3, 3, C]
    with torch.no_grad():
        y = fused.groupnorm_relu_conv3x3_c1(x.reshape(n, H, W, C).permute(0, 3, 1, 2), gn, conv)
    assert y is not None
    r, f32 = A.c1_reference(x, gamma, beta, w, float(conv.bias.detach()), n, H, W, C, G)
    A.check(y.reshape(n, H, W, 1), r, f32, "EXCESS groupnorm_relu_conv3x3_c1 %s %s" % (profile, (n, H, W, C)))


@pytest.mark.parametrize("terms", [16, 6], ids=["fp16_pieces", "six_terms"])
@pytest.mark.parametrize("profile", A.NORM_PROFILES)
def test_conv3x3_merged_with_folded_groupnorm(dev, profile, terms):
    """fused.conv3x3_merged with relu(GroupNorm(low)) applied in its fetch from fused.groupnorm_stats' raw sums: the split product's own
    bound plus the norm's bound carried through |w|."""
    from trackformer_amd import fused
    n, qpi, lh, lw, H, W, cin, cout, G = 6, 3, 13, 21, 25, 42, 64, 32, 8
    low, _, gamma, beta = A.norm_operands(profile, n, lh * lw, cin, seed=cin + lh, device=dev, groups=G)
    low = low.reshape(n, lh, lw, cin)
    g = torch.Generator().manual_seed(7)
    fpn = torch.randn(n // qpi, H, W, cin, generator=g).to(dev)
    w = (torch.randn(cout, 3, 3, cin, generator=g) / (3 * cin ** 0.5)).to(dev)
    b = torch.randn(cout, generator=g).to(dev)
    gn = _groupnorm_module(gamma, beta, G)
    prev = (fused.set_split_linear(True), fused.set_split_terms(terms), fused.set_conv_halo(True), fused.set_check_finite(False))
    try:
        with torch.no_grad():
            ws = fused.groupnorm_stats(low.permute(0, 3, 1, 2), gn)
            assert ws is not None
            y = fused.conv3x3_merged(low.permute(0, 3, 1, 2), fpn.permute(0, 3, 1, 2), qpi, w.reshape(cout, 9 * cin), b, gn, ws)
    finally:
        fused.set_check_finite(prev[3])
        fused.set_conv_halo(prev[2])
        fused.set_split_terms(prev[1])
        fused.set_split_linear(prev[0])
    assert y is not None
    ref, S, floor, nan, k = A.merged_reference(low, fpn, gamma, beta, G, w, b, terms)
    worst = U.check(y.permute(0, 2, 3, 1).reshape(-1, cout), ref, S, floor, nan, k=k)
    print("EXCESS conv3x3_merge+groupnorm %s terms %d: %s" % (profile, terms, worst))


def test_groupnorm_wrappers_decline_other_parameter_types(dev):
    from trackformer_amd import fused
    x2 = torch.randn(2 * 30, 64, device=dev)
    assert fused.groupnorm_nhwc(x2, 2, torch.nn.GroupNorm(8, 64).to(dev)) is not None
    assert fused.groupnorm_nhwc(x2, 2, torch.nn.GroupNorm(8, 64).to(dev).half()) is None
    assert fused.groupnorm_nhwc(x2, 2, torch.nn.GroupNorm(8, 64)) is None
    mixed = torch.nn.GroupNorm(8, 64).to(dev)
    mixed.bias = torch.nn.Parameter(mixed.bias.detach().cpu())
    assert fused.groupnorm_nhwc(x2, 2, mixed) is None


def test_groupnorm_relu_conv3x3_c1_declines_other_parameter_types(dev):
    from trackformer_amd import fused
    x = torch.randn(2, 16, 9, 11, device=dev).contiguous(memory_format=torch.channels_last)
    conv = torch.nn.Conv2d(16, 1, 3, padding=1).to(dev)
    assert fused.groupnorm_relu_conv3x3_c1(x, torch.nn.GroupNorm(8, 16).to(dev), conv) is not None
    assert fused.groupnorm_relu_conv3x3_c1(x, torch.nn.GroupNorm(8, 16).to(dev).half(), conv) is None
    assert fused.groupnorm_relu_conv3x3_c1(x, torch.nn.GroupNorm(8, 16).to(dev), torch.nn.Conv2d(16, 1, 3, padding=1).to(dev).half()) is None
    mixed = torch.nn.GroupNorm(8, 16).to(dev)
    mixed.bias = torch.nn.Parameter(mixed.bias.detach().cpu())       # the weight on the device, the bias not
    assert fused.groupnorm_relu_conv3x3_c1(x, mixed, conv) is None


# ---- box refinement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [12, 300, 4001])
@pytest.mark.parametrize("ref_dim", [2, 4])
def test_box_refine(dev, ref_dim, rows):
    """tf_box_refine_f32: references exactly 0, 1, below 0, above 1 and at eps; delta = +-100 saturates to exactly 1 / 0 (not NaN); a
    NaN stays in its own element."""
    from trackformer_amd import fused
    delta, ref = A.box_refine_operands(rows, ref_dim, seed=rows + ref_dim, device=dev)
    clean = fused.box_refine(delta, ref)
    assert clean is not None
    A.check_box_refine(clean, delta, ref, 1e-5, "EXCESS box_refine ref_dim %d rows %d" % (ref_dim, rows))
    assert bool((clean[8] == 1).all()) and bool((clean[9] == 0).all())
    assert bool((clean[10] == 1).all()) and bool((clean[11] < 1e-37).all()) and not bool(torch.isnan(clean).any())
    dn = delta.clone()
    dn[7, 1] = float("nan")
    y = fused.box_refine(dn, ref)
    want_nan = torch.zeros_like(y, dtype=torch.bool)
    want_nan[7, 1] = True
    assert torch.equal(torch.isnan(y), want_nan) and torch.equal(y[~want_nan], clean[~want_nan])
