"""GPU (-m gpu): the backward of a linear as split products on the device (include/tf_fused.h: THE BACKWARD OF A LINEAR;
trackformer_amd/csrc/linear_bwd.h; fused.linear_train) -- the kernels and the autograd Function against float64 computed on the
device with the yardstick of tests/util_split_numerics.py (helpers shared with tests/test_linear_backward_cpu.py), which path ran
(fused.train_route_counts), bit equality across calls / streams / a captured graph, one encoder layer in training mode with the
switch on and off against its float64 copy, and the non-finite contract."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import util_split_numerics as U
from tests.test_linear_backward_cpu import WGRAD_CASES, check_dgrad, check_wgrad, operands

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
    """Every test starts with the switch following the (unset) environment, per-shape msplit and the default terms."""
    from trackformer_amd import _cabi, fused
    prev_sw = fused._split_linear_train
    fused._split_linear_train = None
    prev_terms = fused.split_terms()
    prev_ms = _cabi.lib().tf_msda_set_option(b"wgrad_msplit", 0)
    fused.train_route_counts(reset=True)
    try:
        yield
    finally:
        _cabi.lib().tf_msda_set_option(b"wgrad_msplit", prev_ms)
        fused.set_split_terms(prev_terms)
        fused._split_linear_train = prev_sw


def scale_for(t, role, terms):
    """The scales tf_linear_grad_stats_f32 documents: one from the matrix's largest magnitude (activation role, a float), one per
    column (weight role, a float64 tensor [C])."""
    def one(amax, top):
        if terms == 6 or not (0.0 < amax < 3.0e38):
            return 1.0
        e = math.frexp(amax)[1] - 1
        return 2.0 ** max(-100, min(126, top - e))
    if role == ACT:
        return one(float(t.abs().max()), 14)
    return torch.tensor([one(v, 13) for v in t.abs().amax(0).tolist()], dtype=torch.float64, device=t.device)


def k_stats(a, role, terms, colsum=False):
    from trackformer_amd import fused
    scale2, cs = fused._grad_stats(a, role, terms, colsum)
    return scale2, cs


def k_wgrad(dy, x, terms):
    from trackformer_amd import _cabi, fused
    L = _cabi.lib()
    M, N = dy.shape
    K = x.shape[1]
    s2, _ = k_stats(dy, ACT, terms)
    t2, _ = k_stats(x, WEIGHT, terms)
    nbytes = int(L.tf_linear_wgrad_workspace_bytes(M, K, N))
    assert nbytes >= 0
    ws = torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device=dy.device)
    dw = torch.full((N, K), float("nan"), device=dy.device)
    rc = L.tf_linear_wgrad_split_f32(dy.data_ptr(), x.data_ptr(), s2.data_ptr(), t2.data_ptr(), dw.data_ptr(), ws.data_ptr(), nbytes,
                                     M, K, N, terms, fused._stream(dy.device))
    assert rc == 0, rc
    return dw, s2, t2


def k_dgrad(dy, w, terms):
    from trackformer_amd import _cabi, fused
    L = _cabi.lib()
    M, N = dy.shape
    K = w.shape[1]
    wt = w.t().contiguous()
    pk = torch.empty(int(L.tf_linear_packed_bytes(N, K, terms)), dtype=torch.uint8, device=dy.device)
    assert L.tf_linear_pack_weight_f32(wt.data_ptr(), pk.data_ptr(), N, K, terms, fused._stream(dy.device)) == 0
    s2, _ = k_stats(dy, ACT, terms)
    dx = torch.full((M, K), float("nan"), device=dy.device)
    rc = L.tf_linear_dgrad_packed_f32(dy.data_ptr(), s2.data_ptr(), pk.data_ptr(), dx.data_ptr(), M, K, N, terms, fused._stream(dy.device))
    assert rc == 0, rc
    return dx, s2


def check_bias(db, dy):
    ref = dy.double().sum(0)
    S = dy.double().abs().sum(0)
    fp32 = dy.sum(0)
    worst = U.check(db, ref, S, k=dy.shape[0])
    print("bias gradient: %.3e (torch fp32: %.3e)" % (worst.value, float(U.excess(fp32, ref, S)[1].value)))


# ---- 1. the kernels against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("profile", U.PROFILES)
def test_kernels_against_float64(dev, profile, terms):
    from trackformer_amd import _cabi
    L = _cabi.lib()
    cases = WGRAD_CASES + [(4100, 384, 256, 0)]
    for (M, N, K, force) in cases:
        L.tf_msda_set_option(b"wgrad_msplit", force)
        for i, dy_scale in enumerate((1e-6, 1e3)):
            dy, x = operands(profile, M, N, K, seed=M + N + K + i, dy_scale=dy_scale)
            dy, x = dy.to(dev), x.to(dev)
            label = "%s x %g [%d, %d, %d] msplit %d" % (profile, dy_scale, M, N, K, force)
            dw, s2, t2 = k_wgrad(dy, x, terms)
            s, t = float(s2[0]), t2[:K].double()
            assert s == scale_for(dy, ACT, terms) and torch.equal(t, scale_for(x, WEIGHT, terms)) and float(s2[1]) == 1.0 / s
            assert torch.equal(t2[K:].double(), 1.0 / t)
            check_wgrad(dw, dy, x, s, t, terms, label)
            s2b, db = k_stats(dy, ACT, terms, colsum=True)
            assert torch.equal(s2b, s2)
            check_bias(db, dy)
            if N % 64 == 0:
                w = torch.randn(N, K, generator=torch.Generator().manual_seed(K), dtype=torch.float32).to(dev) / N ** 0.5
                dx, _ = k_dgrad(dy, w, terms)
                check_dgrad(dx, dy, w, s, terms, label)
    L.tf_msda_set_option(b"wgrad_msplit", 0)


# ---- 2. linear_train under autograd -----------------------------------------------------------------------------------------------------
def _train_case(dev, M, K, N, bias, relu, seed, dy_scale=1e-3):
    """Operands of one linear_train call and its float64 reference.  The upstream gradient is NON-CONTIGUOUS (a transposed view) and is
    zero where the pre-activation lies within the forward's own bound of zero: there the sign of the fp32-class forward, and with
    it the ReLU mask, is not determined."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(dev)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    b = torch.randn(N, generator=g).to(dev) if bias else None
    up = (torch.randn(N, M, generator=g) * dy_scale).to(dev)
    pre = F.linear(x.double(), w.double(), None if b is None else b.double())
    if relu:
        S_fwd = x.double().abs() @ w.double().abs().t() + (0 if b is None else b.double().abs())
        up = torch.where((pre.abs() <= 4 * U.BOUND * S_fwd).t().contiguous(), torch.zeros_like(up), up)
    dy_eff = up.t() * (pre > 0).float() if relu else up.t()
    return x, w, b, up.t(), dy_eff.contiguous()


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("bias,relu", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("M,K,N", [(515, 256, 128), (4100, 64, 256)])
def test_linear_train_against_float64(dev, M, K, N, bias, relu, terms):
    from trackformer_amd import fused
    fused.set_split_terms(terms)
    x, w, b, up, dy_eff = _train_case(dev, M, K, N, bias, relu, seed=M + N + terms)
    assert not up.is_contiguous()
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if bias else None
    y = fused.linear_train(xr, wr, br, relu=relu)
    with torch.no_grad():
        assert torch.equal(y, fused.linear(x, w, b, relu=relu))          # the forward IS the inference path
    y.backward(up)
    counts = fused.train_route_counts()
    assert counts == {"dgrad_own": 1, "dgrad_torch": 0, "wgrad_own": 1, "wgrad_torch": 0, "bias_own": int(bias), "bias_torch": 0}, counts
    s, t = scale_for(dy_eff, ACT, terms), scale_for(x, WEIGHT, terms)
    check_dgrad(xr.grad, dy_eff, w, s, terms, "x.grad")
    check_wgrad(wr.grad, dy_eff, x, s, t, terms, "weight.grad")
    if bias:
        check_bias(br.grad, dy_eff)


# ---- 3. shapes the kernels do not take -----------------------------------------------------------------------------------------------------
def test_fallback_runs_torch_and_says_so(dev):
    from trackformer_amd import fused
    M, K, N = 130, 30, 64
    g = torch.Generator().manual_seed(7)
    x, w, b = torch.randn(M, K, generator=g).to(dev), torch.randn(N, K, generator=g).to(dev), torch.randn(N, generator=g).to(dev)
    up = torch.randn(M, N, generator=g).to(dev)
    grads = []
    for own in (True, False):
        xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
        y = fused.linear_train(xr, wr, br) if own else F.linear(xr, wr, br)
        assert y is not None
        y.backward(up)
        grads.append((y.detach(), xr.grad, wr.grad, br.grad))
    for a, c in zip(*grads):
        assert torch.equal(a, c)
    counts = fused.train_route_counts()
    assert counts == {"dgrad_own": 0, "dgrad_torch": 1, "wgrad_own": 0, "wgrad_torch": 1, "bias_own": 0, "bias_torch": 1}, counts
    # the contraction of the input gradient not a multiple of 64 (hidden 288 -> 96): torch for dx alone
    fused.train_route_counts(reset=True)
    x2, w2 = torch.randn(M, 288, generator=g).to(dev).requires_grad_(True), torch.randn(96, 288, generator=g).to(dev).requires_grad_(True)
    fused.linear_train(x2, w2).sum().backward()
    counts = fused.train_route_counts()
    assert (counts["dgrad_torch"], counts["dgrad_own"], counts["wgrad_own"]) == (1, 0, 1), counts
    assert torch.allclose(x2.grad, w2.detach().sum(0).expand(M, 288), rtol=1e-5, atol=1e-5)


# ---- 4. reproducibility --------------------------------------------------------------------------------------------------------------------
def test_bit_identical_across_calls_streams_and_graph_replay(dev):
    from trackformer_amd import fused
    M, K, N = 4100, 64, 256
    x, w, b, up, _ = _train_case(dev, M, K, N, True, True, seed=9)
    up = up.contiguous()
    params = [t.clone().requires_grad_(True) for t in (x, w, b)]

    def run():
        y = fused.linear_train(params[0], params[1], params[2], relu=True)
        return torch.autograd.grad(y, params, up)

    def same(a, c):
        return all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, c))

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
    assert fused.train_route_counts()["dgrad_torch"] == 0 and fused.train_route_counts()["wgrad_torch"] == 0


# ---- 5. one encoder layer in training mode -----------------------------------------------------------------------------------------------
def test_encoder_layer_gradients_switch_on_and_off(dev):
    from trackformer_amd import fused
    from trackformer_amd.deformable_transformer import DeformableTransformerEncoderLayer
    from trackformer_amd.msda import attach_host_shapes
    torch.manual_seed(3)
    layer = DeformableTransformerEncoderLayer(d_model=256, d_ffn=256, dropout=0.0, n_levels=2, n_heads=8, n_points=4)
    with torch.no_grad():
        for p in layer.self_attn.sampling_offsets.weight, layer.self_attn.attention_weights.weight:
            p.copy_(0.02 * torch.randn_like(p))
    layer = layer.to(dev).train()
    layer64 = DeformableTransformerEncoderLayer(d_model=256, d_ffn=256, dropout=0.0, n_levels=2, n_heads=8, n_points=4).double().to(dev).train()
    layer64.load_state_dict({k: v.double() for k, v in layer.state_dict().items()})
    hw = [(12, 16), (6, 8)]
    S = sum(h * w_ for h, w_ in hw)
    shapes = attach_host_shapes(torch.tensor(hw, device=dev), hw)
    src, pos = torch.randn(2, S, 256, device=dev), torch.randn(2, S, 256, device=dev)
    ref_pts = torch.rand(2, S, 2, 2, device=dev)
    up = torch.randn(2, S, 256, device=dev)

    def grads_of(mod, dt):
        mod.zero_grad()
        s = src.to(dt).clone().requires_grad_(True)   # (every linear then has an input gradient to compute)
        out = mod(s, pos.to(dt), ref_pts.to(dt), shapes)
        out.backward(up.to(dt))
        grads = {k: p.grad.clone() for k, p in mod.named_parameters()}
        grads["src"] = s.grad.clone()
        return grads

    want = grads_of(layer64, torch.float64)
    errs = {}
    for on in (False, True):
        fused.set_split_linear_training(on)
        fused.train_route_counts(reset=True)
        got = grads_of(layer, torch.float32)
        counts = fused.train_route_counts()
        if on:
            assert counts["dgrad_own"] == 6 and counts["wgrad_own"] == 6 and counts["bias_own"] == 6 and counts["wgrad_torch"] == 0, counts
        else:
            assert not any(counts.values()), counts
        errs[on] = {k: float((got[k].double() - want[k]).abs().max() / want[k].abs().max()) for k in want}
    fused.set_split_linear_training(None)
    bad = []
    for k in want:
        limit = max(U.FP32_FACTOR * errs[False][k], 2.0 ** -21)
        print("%-40s switch off %.3e  on %.3e  (limit %.3e)" % (k, errs[False][k], errs[True][k], limit))
        if not errs[True][k] <= limit:
            bad.append((k, errs[True][k], limit))
    assert not bad, bad


# ---- 6. non-finite operands -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", TERMS)
def test_a_nan_in_dy_reaches_its_row_of_dx_and_its_channel_of_dw(dev, terms):
    M, N, K = 300, 128, 64
    dy, x = operands("unit", M, N, K, seed=2, dy_scale=1e-3)
    dy, x = dy.to(dev), x.to(dev)
    dy[123, 45] = float("nan")
    w = torch.randn(N, K, device=dev) / N ** 0.5
    dw, _, _ = k_wgrad(dy, x, terms)
    dx, _ = k_dgrad(dy, w, terms)
    assert not bool(torch.isfinite(dx[123]).any()) and not bool(torch.isfinite(dw[45]).any())
