"""GPU (-m gpu): the backward of a 3 x 3 convolution as split products on the device (include/tf_fused.h: THE BACKWARD OF A 3 x 3
CONVOLUTION; trackformer_amd/csrc/conv_bwd.h; fused.conv_train) -- the float64 cases of tests/test_conv_backward_cpu.py through the
real library, the autograd Function against float64 with the counts that say which path ran, the torch fallback, bit equality across
calls / streams / a captured graph, and the non-finite contract.  The yardsticks are those of the CPU file (check_conv_wgrad /
check_conv_dgrad: the linear backward's bounds on the unfolded matrix, the unfolding itself held against F.conv2d in float64)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import util_split_numerics as U
from tests.test_conv_backward_cpu import (DGRAD_CASES, WGRAD_CASES, check_conv_dgrad, check_conv_wgrad, conv_operands, conv_weight,
                                          conv2d_float64_grads, out_size, rotate)
from tests.test_linear_backward_cpu import check_dgrad, check_wgrad
from tests.test_linear_backward_gpu import scale_for

pytestmark = pytest.mark.gpu

TERMS = (16, 6)
ACT, WEIGHT = 0, 1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from trackformer_amd import _cabi
    _cabi.lib()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _clean_state():
    """Every test starts with per-shape msplit, the default terms and zeroed counters."""
    from trackformer_amd import _cabi, fused
    prev_terms = fused.split_terms()
    prev_ms = _cabi.lib().tf_msda_set_option(b"wgrad_msplit", 0)
    fused.conv_train_counts(reset=True)
    fused.train_route_counts(reset=True)
    try:
        yield
    finally:
        _cabi.lib().tf_msda_set_option(b"wgrad_msplit", prev_ms)
        fused.set_split_terms(prev_terms)


def k_conv_wgrad(dy, x, stride, terms):
    """dy [nimg, hout, wout, cout], x [nimg, h, w, cin] on the device -> (dw [cout, 9 cin], s2, t2)."""
    from trackformer_amd import _cabi, fused
    L = _cabi.lib()
    nimg, h, w, cin = x.shape
    cout = dy.shape[-1]
    s2, _ = fused._grad_stats(dy.view(-1, cout), ACT, terms, False)
    t2, _ = fused._grad_stats(x.view(-1, cin), WEIGHT, terms, False)
    nbytes = int(L.tf_conv3x3_wgrad_workspace_bytes(nimg, h, w, cin, cout, stride))
    assert nbytes >= 0
    ws = torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device=dy.device)
    dw = torch.full((cout, 9 * cin), float("nan"), device=dy.device)
    rc = L.tf_conv3x3_wgrad_split_f32(dy.data_ptr(), x.data_ptr(), s2.data_ptr(), t2.data_ptr(), dw.data_ptr(), ws.data_ptr(), nbytes, nimg, h,
                                      w, cin, cout, stride, terms, fused._stream(dy.device))
    assert rc == 0, rc
    return dw, s2, t2


def k_conv_dgrad(dy, wt, terms, ksplit=1):
    """dy [nimg, h, w, cout] on the device, wt [cout, 3, 3, cin] (numpy) -> (dx [nimg, h, w, cin], s2)."""
    from trackformer_amd import _cabi, fused
    L = _cabi.lib()
    nimg, h, w, cout = dy.shape
    cin = wt.shape[-1]
    wr = torch.from_numpy(rotate(wt)).to(dy.device)
    pk = torch.empty(int(L.tf_linear_packed_bytes(9 * cout, cin, terms)), dtype=torch.uint8, device=dy.device)
    assert L.tf_linear_pack_weight_f32(wr.data_ptr(), pk.data_ptr(), 9 * cout, cin, terms, fused._stream(dy.device)) == 0
    s2, _ = fused._grad_stats(dy.view(-1, cout), ACT, terms, False)
    dx = torch.full((nimg, h, w, cin), float("nan"), device=dy.device)
    ws = torch.full((ksplit, dx.numel()), float("nan"), device=dy.device) if ksplit > 1 else None
    rc = L.tf_conv3x3_dgrad_packed_f32(dy.data_ptr(), s2.data_ptr(), pk.data_ptr(), dx.data_ptr(), fused._ptr(ws), ksplit, nimg, h, w, cin,
                                       cout, terms, fused._stream(dy.device))
    assert rc == 0, rc
    return dx, s2


# ---- 1. the kernels against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("nimg,h,w,cin,cout,stride,force", WGRAD_CASES)
def test_wgrad_against_float64(dev, nimg, h, w, cin, cout, stride, force, terms):
    from trackformer_amd import _cabi
    L = _cabi.lib()
    L.tf_msda_set_option(b"wgrad_msplit", force)
    if force:
        assert L.tf_conv3x3_wgrad_workspace_bytes(nimg, h, w, cin, cout, stride) == force * cout * 9 * cin * 4
    for i, dy_scale in enumerate((1e-6, 1e3)):
        profile = U.PROFILES[(h + cout + i + terms) % len(U.PROFILES)]
        dy, x = conv_operands(profile, nimg, h, w, cin, cout, stride, seed=h + w + cin + i, dy_scale=dy_scale)
        dyd, xd = torch.from_numpy(dy).to(dev), torch.from_numpy(x).to(dev)
        dw, s2, t2 = k_conv_wgrad(dyd, xd, stride, terms)
        s, t = float(s2[0]), t2[:cin].double()
        assert s == scale_for(dyd.view(-1, cout), ACT, terms) and torch.equal(t, scale_for(xd.view(-1, cin), WEIGHT, terms))
        dw = dw.cpu().numpy()
        check_conv_wgrad(dw, dy, x, stride, s, t.cpu().numpy(), terms, "%s x %g %s" % (profile, dy_scale, (nimg, h, w, cin, cout, stride)))
        if h == 1 and w == 1:
            taps = dw.reshape(cout, 9, cin)
            assert (np.delete(taps, 4, axis=1) == 0.0).all() and (taps[:, 4] != 0.0).any()


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("nimg,h,w,cin,cout,stride,ksplit", [c + (1,) for c in DGRAD_CASES] + [DGRAD_CASES[2] + (3,)])
def test_dgrad_against_float64(dev, nimg, h, w, cin, cout, stride, ksplit, terms):
    g = torch.Generator().manual_seed(h * w + cin)
    dy = (torch.randn(nimg, h, w, cout, generator=g) * 3e-5).numpy()
    wt = conv_weight(cout, cin, seed=cin + cout)
    dx, s2 = k_conv_dgrad(torch.from_numpy(dy).to(dev), wt, terms, ksplit)
    check_conv_dgrad(dx.cpu().numpy(), dy, wt, float(s2[0]), terms, str((nimg, h, w, cin, cout)))


@pytest.mark.parametrize("halo", [1, 0])
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("nimg,h,w,cin,cout,stride,ksplit", [c + (1,) for c in DGRAD_CASES] + [DGRAD_CASES[2] + (3,)])
def test_dgrad_is_the_packed_convolution_of_the_scaled_gradient(dev, nimg, h, w, cin, cout, stride, ksplit, terms, halo):
    """Bit for bit (1 / s) . tf_conv_packed_f32(s dy, w_rot packed, the same ksplit) on the device, under either form of that entry."""
    from trackformer_amd import _cabi, fused
    L = _cabi.lib()
    g = torch.Generator().manual_seed(h * w + cin)
    dy = (torch.randn(nimg, h, w, cout, generator=g) * 3e-5).to(dev)
    wt = conv_weight(cout, cin, seed=cin + cout)
    prev = L.tf_msda_set_option(b"conv_halo", halo)
    try:
        dx, s2 = k_conv_dgrad(dy, wt, terms, ksplit)
        wr = torch.from_numpy(rotate(wt)).to(dev)
        pk = torch.empty(int(L.tf_linear_packed_bytes(9 * cout, cin, terms)), dtype=torch.uint8, device=dev)
        assert L.tf_linear_pack_weight_f32(wr.data_ptr(), pk.data_ptr(), 9 * cout, cin, terms, fused._stream(dev)) == 0
        sdy = dy * s2[0]
        y = torch.full((nimg, h, w, cin), float("nan"), device=dev)
        ws = torch.full((ksplit, y.numel()), float("nan"), device=dev) if ksplit > 1 else None
        rc = L.tf_conv_packed_f32(sdy.data_ptr(), pk.data_ptr(), None, None, y.data_ptr(), fused._ptr(ws), ksplit, nimg, h, w, cout, cin, 3, 1,
                                  0, terms, fused._stream(dev))
        assert rc == 0, rc
    finally:
        L.tf_msda_set_option(b"conv_halo", prev)
    assert (float(s2[0]) == 1.0) == (terms == 6)
    assert torch.equal((y * s2[1]).view(torch.int32), dx.view(torch.int32))


@pytest.mark.parametrize("terms", TERMS)
def test_linear_dgrad_splitk_against_float64(dev, terms):
    """The 1 x 1 layers' input gradient with the contraction in pieces (a reducing layer's shape: 1024 products in 4 pieces)."""
    from trackformer_amd import _cabi, fused
    L = _cabi.lib()
    M, N, K, ksplit = 515, 1024, 256, 4
    g = torch.Generator().manual_seed(M)
    dy = (torch.randn(M, N, generator=g) * 3e-5).to(dev)
    w = (torch.randn(N, K, generator=g) / N ** 0.5).to(dev)
    wt = w.t().contiguous()
    pk = torch.empty(int(L.tf_linear_packed_bytes(N, K, terms)), dtype=torch.uint8, device=dev)
    assert L.tf_linear_pack_weight_f32(wt.data_ptr(), pk.data_ptr(), N, K, terms, fused._stream(dev)) == 0
    s2, _ = fused._grad_stats(dy, ACT, terms, False)
    outs = []
    for ks in (1, ksplit):
        dx = torch.full((M, K), float("nan"), device=dev)
        ws = torch.full((ks, M * K), float("nan"), device=dev)
        rc = L.tf_linear_dgrad_splitk_packed_f32(dy.data_ptr(), s2.data_ptr(), pk.data_ptr(), dx.data_ptr(), ws.data_ptr(), ks, M, K, N, terms,
                                                 fused._stream(dev))
        assert rc == 0, rc
        outs.append(dx)
    ref = torch.full((M, K), float("nan"), device=dev)
    assert L.tf_linear_dgrad_packed_f32(dy.data_ptr(), s2.data_ptr(), pk.data_ptr(), ref.data_ptr(), M, K, N, terms, fused._stream(dev)) == 0
    assert torch.equal(outs[0].view(torch.int32), ref.view(torch.int32))
    check_dgrad(outs[1], dy, w, float(s2[0]), terms, "[%d, %d, %d] in %d pieces" % (M, N, K, ksplit))


# ---- 2. conv_train under autograd -------------------------------------------------------------------------------------------------------
def _train_case(dev, n, cin, h, w, cout, ks, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    w4 = (torch.randn(cout, cin, ks, ks, generator=g) / (ks * ks * cin) ** 0.5).to(dev)
    return x, w4


def _run_conv_train(x, w4, stride, up):
    from trackformer_amd import fused
    cout, cin, ks, _ = w4.shape
    xr, wr = x.clone(memory_format=torch.preserve_format).requires_grad_(True), w4.clone().requires_grad_(True)
    w2 = wr.permute(0, 2, 3, 1).reshape(cout, ks * ks * cin)     # taken outside: autograd carries dw back to the OIHW weight
    y = fused.conv_train(xr, w2, stride)
    assert y is not None and y.is_contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        if ks == 3:
            assert torch.equal(y, fused.conv3x3(x, w2.detach(), None, False, stride))      # the forward IS the inference route
        else:
            assert torch.equal(y.permute(0, 2, 3, 1).reshape(-1, cout), fused.linear(x.permute(0, 2, 3, 1).reshape(-1, cin), w2.detach()))
    y.backward(up)
    return y.detach(), xr.grad, wr.grad


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("stride", [1, 2])
def test_conv_train_3x3_against_float64(dev, stride, terms):
    from trackformer_amd import fused
    fused.set_split_terms(terms)
    n, cin, h, w, cout = 2, 64, 13, 18, 128
    x, w4 = _train_case(dev, n, cin, h, w, cout, 3, seed=stride + terms)
    ho, wo = out_size(h, stride), out_size(w, stride)
    up = (torch.randn(n, cout, ho, wo, generator=torch.Generator().manual_seed(5)) * 1e-3).to(dev).contiguous(memory_format=torch.channels_last)
    _, dx, dw4 = _run_conv_train(x, w4, stride, up)
    counts = fused.conv_train_counts()
    assert counts == {"fwd_own": 1, "fwd_torch": 0, "dgrad_own": int(stride == 1), "dgrad_torch": int(stride == 2), "wgrad_own": 1,
                      "wgrad_torch": 0}, counts
    assert dx.shape == x.shape and dw4.shape == w4.shape
    dyn, xn = up.permute(0, 2, 3, 1).contiguous(), x.permute(0, 2, 3, 1).contiguous()
    wn = w4.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    s, t = scale_for(dyn.view(-1, cout), ACT, terms), scale_for(xn.view(-1, cin), WEIGHT, terms)
    check_conv_wgrad(dw4.permute(0, 2, 3, 1).reshape(cout, -1).cpu().numpy(), dyn.cpu().numpy(), xn.cpu().numpy(), stride, s,
                     t.cpu().numpy(), terms, "weight.grad stride %d" % stride)
    dxn = dx.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    if stride == 1:
        check_conv_dgrad(dxn, dyn.cpu().numpy(), wn, s, terms, "x.grad")
    else:
        # torch's fp32 input gradient (counted above): the classical bound of an fp32 sum of K = 9 cout products, K 2^-24 sum |a b|
        ref, _ = conv2d_float64_grads(dyn.cpu().numpy(), xn.cpu().numpy(), wn, stride)
        S, _ = conv2d_float64_grads(np.abs(dyn.cpu().numpy()), xn.cpu().numpy(), np.abs(wn), stride)
        assert ((torch.from_numpy(dxn).double() - ref).abs() <= 9 * cout * 2.0 ** -24 * S + 1e-300).all()


@pytest.mark.parametrize("terms", TERMS)
def test_conv_train_1x1_against_float64(dev, terms):
    from trackformer_amd import fused
    fused.set_split_terms(terms)
    n, cin, h, w, cout = 2, 64, 9, 11, 128
    x, w4 = _train_case(dev, n, cin, h, w, cout, 1, seed=terms)
    up = (torch.randn(n, cout, h, w, generator=torch.Generator().manual_seed(6)) * 1e-3).to(dev).contiguous(memory_format=torch.channels_last)
    _, dx, dw4 = _run_conv_train(x, w4, 1, up)
    counts, linear_counts = fused.conv_train_counts(), fused.train_route_counts()
    assert counts == {"fwd_own": 1, "fwd_torch": 0, "dgrad_own": 0, "dgrad_torch": 0, "wgrad_own": 0, "wgrad_torch": 0}, counts
    assert linear_counts == {"dgrad_own": 1, "dgrad_torch": 0, "wgrad_own": 1, "wgrad_torch": 0, "bias_own": 0, "bias_torch": 0}, linear_counts
    dy2, x2, w2 = up.permute(0, 2, 3, 1).reshape(-1, cout), x.permute(0, 2, 3, 1).reshape(-1, cin), w4.reshape(cout, cin)
    s, t = scale_for(dy2, ACT, terms), scale_for(x2, WEIGHT, terms)
    check_dgrad(dx.permute(0, 2, 3, 1).reshape(-1, cin), dy2, w2, s, terms, "x.grad")
    check_wgrad(dw4.reshape(cout, cin), dy2, x2, s, t, terms, "weight.grad")


# ---- 3. what the kernels do not take ------------------------------------------------------------------------------------------------------
def test_fallback_runs_torch_and_says_so(dev):
    """cout = 32: the contraction of the input gradient is no multiple of 64 -> dx from torch (bitwise torch's own), dw from the kernel."""
    from trackformer_amd import fused
    n, cin, h, w, cout = 2, 64, 10, 12, 32
    x, w4 = _train_case(dev, n, cin, h, w, cout, 3, seed=11)
    up = torch.randn(n, cout, h, w, generator=torch.Generator().manual_seed(7)).to(dev).contiguous(memory_format=torch.channels_last)
    y, dx, dw4 = _run_conv_train(x, w4, 1, up)
    counts = fused.conv_train_counts()
    assert counts["dgrad_torch"] == 1 and counts["dgrad_own"] == 0 and counts["wgrad_own"] == 1 and counts["wgrad_torch"] == 0, counts
    w_cl = w4.contiguous(memory_format=torch.channels_last)
    want, _, _ = torch.ops.aten.convolution_backward(up, x, w_cl, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [True, False, False])
    assert torch.allclose(dx, want, rtol=1e-5, atol=1e-5 * float(want.abs().max()))
    ref = F.conv2d(x.double(), w4.double(), None, 1, 1)
    assert torch.allclose(y.double(), ref, rtol=0, atol=1e-5 * float(ref.abs().max()))
    dyn, xn = up.permute(0, 2, 3, 1).contiguous(), x.permute(0, 2, 3, 1).contiguous()
    s, t = scale_for(dyn.view(-1, cout), ACT, 16), scale_for(xn.view(-1, cin), WEIGHT, 16)
    check_conv_wgrad(dw4.permute(0, 2, 3, 1).reshape(cout, -1).cpu().numpy(), dyn.cpu().numpy(), xn.cpu().numpy(), 1, s, t.cpu().numpy(), 16)


# ---- 4. reproducibility --------------------------------------------------------------------------------------------------------------------
def test_bit_identical_across_calls_streams_and_graph_replay(dev):
    from trackformer_amd import fused
    n, cin, h, w, cout = 2, 64, 21, 23, 128
    x, w4 = _train_case(dev, n, cin, h, w, cout, 3, seed=9)
    up = (torch.randn(n, cout, h, w, generator=torch.Generator().manual_seed(8)) * 1e-2).to(dev).contiguous(memory_format=torch.channels_last)
    params = [x.clone(memory_format=torch.preserve_format).requires_grad_(True),
              w4.permute(0, 2, 3, 1).reshape(cout, 9 * cin).clone().requires_grad_(True)]

    def run():
        y = fused.conv_train(params[0], params[1], 1)
        return torch.autograd.grad(y, params, up)

    def same(a, c):
        return all(torch.equal(p.contiguous().view(torch.int32), q.contiguous().view(torch.int32)) for p, q in zip(a, c))

    first = run()
    assert same(first, run())
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    assert same(first, third)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for t in captured:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize(dev)
    assert same(first, captured)
    counts = fused.conv_train_counts()
    assert counts["dgrad_torch"] == 0 and counts["wgrad_torch"] == 0 and counts["dgrad_own"] == 4 and counts["wgrad_own"] == 4, counts


# ---- 5. non-finite operands -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", TERMS)
def test_a_nan_in_dy_reaches_its_neighbourhood_of_dx_and_its_channel_of_dw(dev, terms):
    nimg, h, w, cin, cout = 2, 7, 9, 36, 64
    dy, x = conv_operands("unit", nimg, h, w, cin, cout, 1, seed=2, dy_scale=1e-3)
    dy[1, 3, 4, 45] = float("nan")     # an interior pixel: all nine taps lie inside the image
    dyd, xd = torch.from_numpy(dy).to(dev), torch.from_numpy(x).to(dev)
    dw, _, _ = k_conv_wgrad(dyd, xd, 1, terms)
    dx, _ = k_conv_dgrad(dyd, conv_weight(cout, cin, seed=3), terms)
    assert not bool(torch.isfinite(dx[1, 2:5, 3:6]).any()) and not bool(torch.isfinite(dw[45]).any())
