"""GPU (-m gpu): the backward of the stride-2 convolutions on the device (include/tf_fused.h: THE BACKWARD OF THE STRIDE-2
CONVOLUTIONS; trackformer_amd/csrc/conv_strided_bwd.h; fused.conv_train under fused.set_strided_conv_training) -- the float64 cases of
tests/test_conv_strided_backward_cpu.py through the real library, the autograd Functions against float64 with the counts that say
which path ran, the torch fallback, bit equality across calls / streams / a captured graph / a whole bottleneck, and the non-finite
contract.  The yardsticks are those of the CPU file: every parity class against check_dgrad on its own unfolded matrix, the strided
1 x 1 weight gradient against check_wgrad on the gathered matrix.

The large case of each kind: the kernels index pixels in 32 bits and the entry points reject tensors of 3 GiB, so no index can wrap
below that gate; what a few MB can reach is a class of 16 770 rows (2 x 130 x 258 input pixels): more than a hundred row blocks per
class, image boundaries inside row blocks, and a pixel loop of the weight gradient in several chunks."""
import numpy as np
import pytest
import torch

from tests import util_split_numerics as U
from tests.test_conv_backward_cpu import conv_operands, conv_weight, out_size
from tests.test_conv_strided_backward_cpu import (DGRAD1_CASES, DGRAD3_CASES, WGRAD1_CASES, check_strided_dgrad, class_weights, gathered)
from tests.test_linear_backward_cpu import check_wgrad
from tests.test_linear_backward_gpu import scale_for

pytestmark = pytest.mark.gpu

TERMS = (16, 6)
ACT, WEIGHT = 0, 1
LARGE = (2, 130, 258, 8, 64)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from trackformer_amd import _cabi
    _cabi.lib()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _clean_state():
    """Every test starts with per-shape msplit, the default terms, the switch off and zeroed counters."""
    from trackformer_amd import _cabi, fused
    prev_terms = fused.split_terms()
    prev_ms = _cabi.lib().tf_msda_set_option(b"wgrad_msplit", 0)
    prev_raw = fused._strided_conv_train
    fused.set_strided_conv_training(False)
    fused.conv_train_counts(reset=True)
    fused.train_route_counts(reset=True)
    try:
        yield
    finally:
        _cabi.lib().tf_msda_set_option(b"wgrad_msplit", prev_ms)
        fused.set_split_terms(prev_terms)
        fused.set_strided_conv_training(prev_raw)


def k_strided_dgrad(dy, wt, h, w, ks, terms, ksplit=1):
    """dy [nimg, ho, wo, cout] on the device, wt [cout, 3, 3, cin] or [cout, cin] (numpy) -> (dx [nimg, h, w, cin], s2)."""
    from trackformer_amd import _cabi, fused
    L = _cabi.lib()
    nimg, ho, wo, cout = dy.shape
    cin = wt.shape[-1]
    classes = [torch.from_numpy(c).to(dy.device) for c in class_weights(wt, ks)]
    sizes = [int(L.tf_linear_packed_bytes(c.shape[1], cin, terms)) for c in classes]
    pk = torch.empty(sum(sizes), dtype=torch.uint8, device=dy.device)
    at = pk.data_ptr()
    for c, nb in zip(classes, sizes):
        assert L.tf_linear_pack_weight_f32(c.data_ptr(), at, c.shape[1], cin, terms, fused._stream(dy.device)) == 0
        at += nb
    s2, _ = fused._grad_stats(dy.view(-1, cout), ACT, terms, False)
    dx = torch.full((nimg, h, w, cin), float("nan"), device=dy.device)
    nbytes = int(L.tf_conv_dgrad_stride2_workspace_bytes(nimg, h, w, cin, cout, ks, ksplit))
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dy.device)
    rc = L.tf_conv_dgrad_stride2_packed_f32(dy.data_ptr(), s2.data_ptr(), pk.data_ptr(), dx.data_ptr(), ws.data_ptr(), nbytes, ksplit, nimg, h, w,
                                            cin, cout, ks, terms, fused._stream(dy.device))
    assert rc == 0, rc
    return dx, s2


def k_strided_wgrad(dy, x, terms):
    """dy [nimg, ho, wo, cout], x [nimg, h, w, cin] on the device -> (dw [cout, cin], s2, t2)."""
    from trackformer_amd import _cabi, fused
    L = _cabi.lib()
    nimg, h, w, cin = x.shape
    cout = dy.shape[-1]
    s2, _ = fused._grad_stats(dy.view(-1, cout), ACT, terms, False)
    t2, _ = fused._grad_stats(x.view(-1, cin), WEIGHT, terms, False)
    nbytes = int(L.tf_conv1x1_strided_wgrad_workspace_bytes(nimg, h, w, cin, cout, 2))
    assert nbytes >= 0
    ws = torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device=dy.device)
    dw = torch.full((cout, cin), float("nan"), device=dy.device)
    rc = L.tf_conv1x1_strided_wgrad_split_f32(dy.data_ptr(), x.data_ptr(), s2.data_ptr(), t2.data_ptr(), dw.data_ptr(), ws.data_ptr(), nbytes,
                                              nimg, h, w, cin, cout, 2, terms, fused._stream(dy.device))
    assert rc == 0, rc
    return dw, s2, t2


def _w1(cout, cin, seed):
    return np.ascontiguousarray(conv_weight(cout, cin, seed)[:, 1, 1]) * np.float32(3.0)


# ---- 1. the kernels against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("nimg,h,w,cin,cout,ksplit", DGRAD3_CASES + [LARGE + (1,)])
def test_dgrad3_against_float64_per_parity_class(dev, nimg, h, w, cin, cout, ksplit, terms):
    for i, dy_scale in enumerate((1e-6, 1e3) if h < 100 else (1e-6,)):
        profile = U.PROFILES[(h + cout + i + terms) % len(U.PROFILES)]
        dy, _ = conv_operands(profile, nimg, h, w, cin, cout, 2, seed=h + w + cin + i, dy_scale=dy_scale)
        wt = conv_weight(cout, cin, seed=cin + cout + i)
        dx, s2 = k_strided_dgrad(torch.from_numpy(dy).to(dev), wt, h, w, 3, terms, ksplit)
        assert float(s2[0]) == scale_for(torch.from_numpy(dy).view(-1, cout), ACT, terms)
        check_strided_dgrad(dx.cpu().numpy(), dy, wt, float(s2[0]), terms, 3, "%s x %g %s" % (profile, dy_scale, (nimg, h, w, cin, cout, ksplit)))


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("nimg,h,w,cin,cout", DGRAD1_CASES + [LARGE])
def test_dgrad1_against_float64_and_exact_zeros(dev, nimg, h, w, cin, cout, terms):
    for i, dy_scale in enumerate((1e-6, 1e3) if h < 100 else (1e3,)):
        profile = U.PROFILES[(h + cout + i + terms) % len(U.PROFILES)]
        dy, _ = conv_operands(profile, nimg, h, w, cin, cout, 2, seed=h + w + cin + i, dy_scale=dy_scale)
        wt = _w1(cout, cin, seed=cin + cout + i)
        dx, s2 = k_strided_dgrad(torch.from_numpy(dy).to(dev), wt, h, w, 1, terms)
        check_strided_dgrad(dx.cpu().numpy(), dy, wt, float(s2[0]), terms, 1, "1 x 1 %s x %g %s" % (profile, dy_scale, (nimg, h, w, cin, cout)))


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("nimg,h,w,cin,cout,force", WGRAD1_CASES + [LARGE + (0,)])
def test_wgrad1_against_float64_and_the_linear_wgrad_of_the_gathered_matrix(dev, nimg, h, w, cin, cout, force, terms):
    from trackformer_amd import _cabi, fused
    L = _cabi.lib()
    L.tf_msda_set_option(b"wgrad_msplit", force)
    if force:
        assert L.tf_conv1x1_strided_wgrad_workspace_bytes(nimg, h, w, cin, cout, 2) == force * cout * cin * 4
    for i, dy_scale in enumerate((1e-6, 1e3) if h < 100 else (1e-6,)):
        profile = U.PROFILES[(h + cout + i + terms) % len(U.PROFILES)]
        dy, x = conv_operands(profile, nimg, h, w, cin, cout, 2, seed=h + w + cin + i, dy_scale=dy_scale)
        dyd, xd = torch.from_numpy(dy).to(dev), torch.from_numpy(x).to(dev)
        dw, s2, t2 = k_strided_wgrad(dyd, xd, terms)
        assert bool(torch.isfinite(dw).all())
        G, dy2 = gathered(x), dy.reshape(-1, cout)
        check_wgrad(dw.cpu().numpy(), dy2, G, float(s2[0]), t2[:cin].double().cpu().numpy(), terms,
                    "1 x 1 %s x %g %s" % (profile, dy_scale, (nimg, h, w, cin, cout)))
        Gd, dy2d = torch.from_numpy(G).to(dev), dyd.view(-1, cout)
        M = Gd.shape[0]
        nbytes = int(L.tf_linear_wgrad_workspace_bytes(M, cin, cout))
        assert nbytes == L.tf_conv1x1_strided_wgrad_workspace_bytes(nimg, h, w, cin, cout, 2)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        want = torch.full((cout, cin), float("nan"), device=dev)
        assert L.tf_linear_wgrad_split_f32(dy2d.data_ptr(), Gd.data_ptr(), s2.data_ptr(), t2.data_ptr(), want.data_ptr(), ws.data_ptr(), nbytes, M,
                                           cin, cout, terms, fused._stream(dev)) == 0
        assert torch.equal(dw.view(torch.int32), want.view(torch.int32))


# ---- 2. conv_train under autograd -------------------------------------------------------------------------------------------------------
def _train_case(dev, n, cin, h, w, cout, ks, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    w4 = (torch.randn(cout, cin, ks, ks, generator=g) / (ks * ks * cin) ** 0.5).to(dev)
    up = (torch.randn(n, cout, out_size(h, 2), out_size(w, 2), generator=g) * 1e-3).to(dev).contiguous(memory_format=torch.channels_last)
    return x, w4, up


def _run_conv_train(x, w4, up):
    from trackformer_amd import fused
    cout, cin, ks, _ = w4.shape
    xr, wr = x.clone(memory_format=torch.preserve_format).requires_grad_(True), w4.clone().requires_grad_(True)
    w2 = wr.permute(0, 2, 3, 1).reshape(cout, ks * ks * cin)     # taken outside: autograd carries dw back to the OIHW weight
    y = fused.conv_train(xr, w2, 2)
    if y is None:
        return None, None, None
    assert y.is_contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        assert torch.equal(y, fused.conv3x3(x, w2.detach(), None, False, 2))      # the forward IS the inference route
    y.backward(up)
    return y.detach(), xr.grad, wr.grad


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("ks,n,cin,h,w,cout", [(3, 2, 64, 13, 18, 128), (1, 2, 64, 9, 11, 128)])
def test_conv_train_stride2_against_float64(dev, ks, n, cin, h, w, cout, terms):
    from tests.test_conv_backward_cpu import check_conv_wgrad
    from trackformer_amd import fused
    fused.set_split_terms(terms)
    x, w4, up = _train_case(dev, n, cin, h, w, cout, ks, seed=ks + terms)
    # the switch off: the counts of before (3 x 3: torch's input gradient; 1 x 1: not conv_train's call)
    y, _, _ = _run_conv_train(x, w4, up)
    off = fused.conv_train_counts(reset=True)
    if ks == 3:
        assert off == {"fwd_own": 1, "fwd_torch": 0, "dgrad_own": 0, "dgrad_torch": 1, "wgrad_own": 1, "wgrad_torch": 0}, off
    else:
        assert y is None and off == {"fwd_own": 0, "fwd_torch": 1, "dgrad_own": 0, "dgrad_torch": 0, "wgrad_own": 0, "wgrad_torch": 0}, off
    fused.set_strided_conv_training(True)
    _, dx, dw4 = _run_conv_train(x, w4, up)
    counts = fused.conv_train_counts()
    assert counts == {"fwd_own": 1, "fwd_torch": 0, "dgrad_own": 1, "dgrad_torch": 0, "wgrad_own": 1, "wgrad_torch": 0}, counts
    assert dx.shape == x.shape and dw4.shape == w4.shape
    dyn, xn = up.permute(0, 2, 3, 1).contiguous(), x.permute(0, 2, 3, 1).contiguous()
    wn = w4.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    s, t = scale_for(dyn.view(-1, cout), ACT, terms), scale_for(xn.view(-1, cin), WEIGHT, terms)
    dxn = dx.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    dwn = dw4.permute(0, 2, 3, 1).reshape(cout, -1).cpu().numpy()
    if ks == 3:
        check_strided_dgrad(dxn, dyn.cpu().numpy(), wn, s, terms, 3, "x.grad")
        check_conv_wgrad(dwn, dyn.cpu().numpy(), xn.cpu().numpy(), 2, s, t.cpu().numpy(), terms, "weight.grad")
    else:
        check_strided_dgrad(dxn, dyn.cpu().numpy(), wn.reshape(cout, cin), s, terms, 1, "x.grad 1 x 1")
        check_wgrad(dwn, dyn.cpu().numpy().reshape(-1, cout), gathered(xn.cpu().numpy()), s, t.cpu().numpy(), terms, "weight.grad 1 x 1")


# ---- 3. what the kernels do not take ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", [3, 1])
def test_fallback_runs_torch_and_says_so(dev, ks):
    """cout = 32: the contraction of the input gradient is no multiple of 64 -> dx from torch, dw from the kernel."""
    from trackformer_amd import fused
    fused.set_strided_conv_training(True)
    n, cin, h, w, cout = 2, 64, 10, 12, 32
    x, w4, up = _train_case(dev, n, cin, h, w, cout, ks, seed=11)
    _, dx, dw4 = _run_conv_train(x, w4, up)
    counts = fused.conv_train_counts()
    assert counts == {"fwd_own": 1, "fwd_torch": 0, "dgrad_own": 0, "dgrad_torch": 1, "wgrad_own": 1, "wgrad_torch": 0}, counts
    pad = 1 if ks == 3 else 0
    want, _, _ = torch.ops.aten.convolution_backward(up, x, w4.contiguous(memory_format=torch.channels_last), None, [2, 2], [pad, pad], [1, 1],
                                                     False, [0, 0], 1, [True, False, False])
    assert torch.allclose(dx, want, rtol=1e-5, atol=1e-5 * float(want.abs().max()))
    assert bool(torch.isfinite(dw4).all())


# ---- 4. reproducibility --------------------------------------------------------------------------------------------------------------------
def _same(a, c):
    return all(torch.equal(p.contiguous().view(torch.int32), q.contiguous().view(torch.int32)) for p, q in zip(a, c))


@pytest.mark.parametrize("ks", [3, 1])
def test_bit_identical_across_calls_streams_and_graph_replay(dev, ks):
    from trackformer_amd import fused
    fused.set_strided_conv_training(True)
    n, cin, h, w, cout = 2, 64, 21, 23, 128
    x, w4, up = _train_case(dev, n, cin, h, w, cout, ks, seed=9)
    params = [x.clone(memory_format=torch.preserve_format).requires_grad_(True),
              w4.permute(0, 2, 3, 1).reshape(cout, ks * ks * cin).clone().requires_grad_(True)]     # a persistent weight: its images are cached

    def run():
        y = fused.conv_train(params[0], params[1], 2)
        return torch.autograd.grad(y, params, up)

    first = run()
    assert _same(first, run())
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    assert _same(first, third)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for t in captured:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize(dev)
    assert _same(first, captured)
    counts = fused.conv_train_counts()
    assert counts["dgrad_torch"] == 0 and counts["wgrad_torch"] == 0 and counts["dgrad_own"] == 4 and counts["wgrad_own"] == 4, counts


def test_a_strided_bottleneck_is_bit_identical_from_run_to_run(dev):
    """The first bottleneck of a stage in the fold mode of the training step, both switches on: every convolution on the own kernels
    (counted), every parameter gradient and the input gradient the same bits in two runs."""
    from trackformer_amd import backbone, fused
    torch.manual_seed(3)
    down = torch.nn.Sequential(torch.nn.Conv2d(128, 256, 1, 2, bias=False), backbone.FrozenBatchNorm2d(256))
    block = backbone.Bottleneck(128, 64, stride=2, downsample=down).to(dev).train()
    x = torch.randn(2, 128, 14, 19, device=dev).contiguous(memory_format=torch.channels_last)
    up = (torch.randn(2, 256, 7, 10, device=dev) * 1e-2).contiguous(memory_format=torch.channels_last)
    prev_conv, prev_fold = backbone._split_conv_train, backbone.set_train_fold(True)
    backbone.set_split_conv_training(True)
    fused.set_strided_conv_training(True)
    try:
        runs = []
        for _ in range(2):
            xr = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
            assert backbone._fold_mode(block, xr) == 2
            grads = torch.autograd.grad(block(xr), [xr] + list(block.parameters()), up)
            runs.append(grads)
        torch.cuda.synchronize(dev)
    finally:
        backbone.set_split_conv_training(prev_conv)
        backbone.set_train_fold(prev_fold)
    assert len(runs[0]) == 5 and all(bool(torch.isfinite(g).all()) for g in runs[0])
    assert _same(runs[0], runs[1])
    counts, linear_counts = fused.conv_train_counts(), fused.train_route_counts()
    # per run: conv2 (3 x 3 stride 2) and the projection through conv_train's own gradients, conv1 / conv3 through the linears'
    assert counts == {"fwd_own": 8, "fwd_torch": 0, "dgrad_own": 4, "dgrad_torch": 0, "wgrad_own": 4, "wgrad_torch": 0}, counts
    assert linear_counts["dgrad_own"] == 4 and linear_counts["wgrad_own"] == 4 and linear_counts["dgrad_torch"] == 0, linear_counts


# ---- 5. non-finite operands -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", TERMS)
def test_a_nan_in_dy_reaches_exactly_its_pixels_of_dx(dev, terms):
    nimg, h, w, cin, cout = 2, 9, 11, 36, 64
    dy, _ = conv_operands("unit", nimg, h, w, cin, cout, 2, seed=2, dy_scale=1e-3)
    dy[1, 2, 3, 45] = float("nan")     # the output pixel (2, 3): input pixels (3 .. 5, 5 .. 7), all inside the image
    dyd = torch.from_numpy(dy).to(dev)
    hit = torch.zeros(nimg, h, w, dtype=torch.bool, device=dev)
    hit[1, 3:6, 5:8] = True
    dx, _ = k_strided_dgrad(dyd, conv_weight(cout, cin, seed=3), h, w, 3, terms)
    assert not bool(torch.isfinite(dx[hit]).any()) and bool(torch.isfinite(dx[~hit]).all())
    hit[:] = False
    hit[1, 4, 6] = True
    dx, _ = k_strided_dgrad(dyd, _w1(cout, cin, seed=3), h, w, 1, terms)
    assert not bool(torch.isfinite(dx[hit]).any()) and bool(torch.isfinite(dx[~hit]).all())
