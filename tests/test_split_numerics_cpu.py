"""CPU: the float64 yardstick of the split product (tests/util_split_numerics.py) has power.  It rejects a product that is only
"almost" fp32 (one fp16 piece per operand, one bf16 piece per operand) at unit and spread magnitudes, accepts torch's fp32
result, and accepts the fp16 split scheme itself (emulated here with exact products, the pieces fused._split_weight hands the
kernels) in every magnitude profile -- so a kernel that fails it on the GPU has a product that differs from the scheme."""
import pytest
import torch
import torch.nn.functional as F

from tests import util_split_numerics as U


def test_limit_is_the_package_limit():
    from trackformer_amd import fused
    assert U.F16_ACTIVATION_LIMIT == fused.F16_ACTIVATION_LIMIT


def _f16_scheme(x, w):
    """x w^T under the fp16 scheme of split_product.h: x 2^-4 -> (hi, lo' = (x 2^-4 - hi) 2^11) in fp16, the channel-scaled weight
    pieces of fused._split_weight, the three terms lo'.(wh 2^-11) + hi.wl + hi.wh, each product exact (float64), times 16 / t_n."""
    from trackformer_amd import fused
    prev = fused.set_split_terms(16)
    try:
        wh, wl, _, sc = fused._split_weight(w)
    finally:
        fused.set_split_terms(prev)
    xs = x * 0.0625
    hi = xs.half()
    lo = ((xs - hi.float()) * 2048.0).half()
    wh, wl = wh.double(), wl.double()
    acc = lo.double() @ (wh * 2.0 ** -11).t() + hi.double() @ wl.t() + hi.double() @ wh.t()
    return acc * sc.double()


@pytest.mark.parametrize("profile", ["unit", "row_spread", "channel_spread"])
@pytest.mark.parametrize("M,K,N", [(64, 256, 96), (7, 32, 5)])
def test_yardstick_rejects_fp16_and_bf16_products_and_accepts_fp32(profile, M, K, N):
    x, w, b, r = U.linear_operands(profile, M, K, N, seed=M + K + N, bias=True, residual=True)
    ref, S, floor, nan = U.linear_reference(x, w, b, r, terms=16)
    fp32 = U.linear_fp32(x, w, b, r)
    worst = U.check(fp32, ref, S, floor, nan, fp32=fp32)
    assert worst.value < U.BOUND
    for dt in (torch.float16, torch.bfloat16):
        one_piece = x.to(dt).float() @ w.to(dt).float().t() + b + r
        with pytest.raises(AssertionError):
            U.check(one_piece, ref, S, floor, nan, fp32=fp32)
    # a product that keeps the pieces but misses one term by one piece's worth (the lower weight piece dropped) fails as well
    from trackformer_amd import fused
    prev = fused.set_split_terms(16)
    try:
        wh, wl, _, sc = fused._split_weight(w)
    finally:
        fused.set_split_terms(prev)
    no_lo = (x.double() @ (wh.double() * sc.double()[:, None] / 16).t()) + b + r
    with pytest.raises(AssertionError):
        U.check(no_lo, ref, S, floor, nan, fp32=fp32)


@pytest.mark.parametrize("profile", U.PROFILES + ["nonfinite"])
def test_the_fp16_scheme_passes_in_every_profile(profile):
    """The scheme's representation (exact products, float64 sums) within the bound in every profile: the floor the header states is
    enough, nothing falls into the fp16 subnormals beyond it -- also not the all-subnormal weight channel, whose per-channel scale
    must reach far enough to make it normal -- and the non-finite rows are exactly the expected ones."""
    M, K, N = 96, 288, 40
    x, w, b, _ = U.linear_operands(profile, M, K, N, seed=5, bias=False)
    ref, S, floor, nan = U.linear_reference(x, w, None, terms=16)
    y = _f16_scheme(x, w)
    U.check(y, ref, S, floor, nan, fp32=U.linear_fp32(x, w))


def test_profiles_contain_what_they_promise():
    x, w, _, _ = U.linear_operands("large_x", 40, 64, 24, seed=1)
    assert float(x.abs().max()) == pytest.approx(0.9 * U.F16_ACTIVATION_LIMIT)
    x, w, _, _ = U.linear_operands("edge_values", 40, 64, 24, seed=1)
    assert bool((x[1].abs() == U.SUBNORMAL).all()) and bool((x[3] == 0).all()) and bool((w[0] == 0).all())
    assert bool(((w[23].abs() == U.SUBNORMAL) | (w[23] == 0)).all()) and bool(torch.signbit(x[x == 0]).any())
    x, w, _, _ = U.linear_operands("nonfinite", 40, 64, 24, seed=1)
    assert int(torch.isnan(x).sum()) == 1 and int((x.abs() > U.F16_ACTIVATION_LIMIT).sum()) == 1
    x, wt, b = U.conv_operands("channel_spread", 1, 32, 5, 6, 22, 3, seed=2)
    assert x.is_contiguous(memory_format=torch.channels_last) and float(wt[3].abs().max()) > 50 * float(wt[1].abs().max())


@pytest.mark.parametrize("k,stride,padding,cl", [(3, 1, 1, True), (3, 2, 1, False), (1, 2, 0, True), (7, 2, 3, False)])
def test_conv_reference_is_the_convolution(k, stride, padding, cl):
    x, w, b = U.conv_operands("unit", 2, 8, 9, 7, 6, k, seed=k + stride)
    if not cl:
        x = x.contiguous()
    ref, S, floor, nan = U.conv_reference(x, w, b, stride, padding, relu=True)
    want = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=padding).clamp_min(0)
    assert torch.allclose(ref, want.permute(0, 2, 3, 1).reshape(-1, 6), rtol=1e-12, atol=1e-12)
    want_s = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=stride, padding=padding)
    assert torch.allclose(S, want_s.permute(0, 2, 3, 1).reshape(-1, 6), rtol=1e-12, atol=1e-12)
    fp32 = U.conv_fp32(x, w, b, stride, padding, relu=True)
    U.check(fp32, ref, S, floor, nan, fp32=fp32)
    rows = torch.tensor([0, 5, ref.shape[0] - 1])
    r2 = U.conv_reference(x, w, b, stride, padding, relu=True, rows=rows)[0]
    assert torch.allclose(r2, ref[rows], rtol=1e-14, atol=1e-14)
    # a NaN pixel: exactly the outputs whose window holds it
    x2 = x.clone()
    x2[0, 3, 4, 2] = float("nan")
    nan2 = U.conv_reference(x2, w, b, stride, padding, terms=6)[3]
    want_nan = torch.isnan(F.conv2d(x2.double(), w.double().abs() + 1, None, stride=stride, padding=padding)).permute(0, 2, 3, 1).reshape(-1, 6)
    assert torch.equal(nan2, want_nan) and bool(nan2.any())


def test_layernorm_bound_accepts_fp32_and_rejects_a_one_piece_product():
    M, D = 64, 256
    x, w, b, r = U.linear_operands("row_spread", M, D, D, seed=9, residual=True)
    g = torch.Generator().manual_seed(3)
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    pre, S, floor, nan = U.linear_reference(x, w, b, r, terms=16)
    ref, Sn, fn, nan_n = U.layernorm_reference(pre, S, floor, gamma, beta, 1e-5, nan)
    fp32 = F.layer_norm(U.linear_fp32(x, w, b, r), (D,), gamma, beta, 1e-5)
    U.check(fp32, ref, Sn, fn, nan_n)
    one_piece = F.layer_norm(x.half().float() @ w.half().float().t() + b + r, (D,), gamma, beta, 1e-5)
    with pytest.raises(AssertionError):
        U.check(one_piece, ref, Sn, fn, nan_n)
