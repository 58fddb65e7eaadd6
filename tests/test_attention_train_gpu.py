"""GPU (-m gpu): the training path of the attention core (include/tf_fused.h: TRAINING THROUGH THE ATTENTION CORE;
trackformer_amd/csrc/mha_bwd.h) and of the decoder layer's self-attention site (fused.set_attention_training) on an MI355X, against the
float64 yardsticks of tests/util_attention_train.py; the mask is the numpy restatement of the mask contract.

Every output lives in a buffer with a canary in three rows behind the last, checked unchanged."""
import contextlib

import pytest
import torch

from tests import util_attention_train as AT
from tests import util_norm_attn_numerics as NA
from tests import util_train_gradients as G

pytestmark = pytest.mark.gpu

CANARY = -4321.5
GUARD = 3
SEED, OFFSET = 0x9E3779B97F4A7C15 - 2 ** 64, 0x7FEDCBA987654321
SMALL = [(1, 1, 16, 16, 32), (2, 2, 37, 50, 32), (1, 2, 50, 37, 36), (1, 1, 17, 70, 32)]
LARGE = [(2, 8, 400, 400, 32), (1, 8, 512, 512, 32), (1, 2, 513, 513, 32), (1, 8, 800, 800, 36)]
MASKED = {(1, 1, 17, 70, 32), (1, 2, 513, 513, 32)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from trackformer_amd import _cabi
    _cabi.lib()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _clean_state():
    from trackformer_amd import fused
    names = ("_attention_train", "_dropout_train", "_layernorm_train", "_split_linear_train")
    prev = [getattr(fused, n) for n in names]
    for n in names:
        setattr(fused, n, None)
    fused.attention_train_counts(reset=True)
    try:
        yield
    finally:
        for n, v in zip(names, prev):
            setattr(fused, n, v)
        fused.attention_train_counts(reset=True)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _rng(dev, seed=SEED, offset=OFFSET):
    return torch.tensor([seed, offset], dtype=torch.int64, device=dev)


def _guarded(rows, cols, dev):
    return torch.full((rows + GUARD, cols), CANARY, dtype=torch.float32, device=dev)


def run_kernels(dev, q, k, v, dout, scale, km, p, rng):
    """tf_mha_core_train_f32 + tf_mha_core_bwd_f32 on [N, L, H, D] operands -> {"out", "dq", "dk", "dv"}, canaries checked."""
    from trackformer_amd import _cabi
    L = _cabi.lib()
    N, Lq, H, D = q.shape
    Lk, E = k.shape[1], H * D
    q, k, v, dout = (t.contiguous() for t in (q, k, v, dout))
    out, dq = _guarded(N * Lq, E, dev), _guarded(N * Lq, E, dev)
    dk, dv = _guarded(N * Lk, E, dev), _guarded(N * Lk, E, dev)
    stats = _guarded(N * H * Lq, 2, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    pp = 0.0 if p is None else p
    rc = L.tf_mha_core_train_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _ptr(km), stats.data_ptr(), _ptr(rng), pp,
                                 N, Lq, Lk, H, D, E, E, E, E, scale, stream)
    assert rc == 0, rc
    rc = L.tf_mha_core_bwd_f32(dout.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), stats.data_ptr(), _ptr(km),
                               _ptr(rng), pp, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), N, Lq, Lk, H, D, E, E, E, E, E, E, E, E, scale,
                               stream)
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    for t, rows in ((out, N * Lq), (dq, N * Lq), (dk, N * Lk), (dv, N * Lk), (stats, N * H * Lq)):
        assert bool((t[rows:] == CANARY).all()), "a kernel wrote behind the last row"
    return {"out": out[:N * Lq].view(N, Lq, H, D), "dq": dq[:N * Lq].view(N, Lq, H, D), "dk": dk[:N * Lk].view(N, Lk, H, D),
            "dv": dv[:N * Lk].view(N, Lk, H, D)}


def check_case(dev, case, profile, p, dead_image=False):
    N, H, Lq, Lk, D = case
    if dead_image:
        N = 2
    q, k, v, scale = NA.attention_operands(profile, N, Lq, Lk, H, D, 3, device=dev)
    dout = AT.grad_operand(N, Lq, H, D, 3, device=dev)
    km = AT.masks(N, Lk, 3, device=dev, last_image_dead=dead_image) if (case in MASKED or dead_image) else None
    rng = _rng(dev) if p is not None else None
    keep = AT.keep_of(rng, p, N, H, Lq, Lk) if p is not None else None
    got = run_kernels(dev, q, k, v, dout, scale, km, p, rng)
    ref = AT.reference(q, k, v, dout, scale, km, keep, p)
    fp32 = AT.formulation(q, k, v, dout, scale, km, keep, p)
    return AT.check(got, ref, fp32, km, "%s %s p=%s" % (case, profile, p))


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [None, 0.1, 0.5])
@pytest.mark.parametrize("profile", ["unit", "peaked", "qoffset"])
@pytest.mark.parametrize("case", SMALL, ids=str)
def test_small_cases_against_float64(dev, case, profile, p):
    check_case(dev, case, profile, p)


@pytest.mark.parametrize("p", [None, 0.1])
@pytest.mark.parametrize("case", LARGE, ids=str)
def test_large_cases_against_float64(dev, case, p):
    check_case(dev, case, "unit", p)


@pytest.mark.parametrize("profile", NA.ATTN_PROFILES)
def test_every_profile_against_float64(dev, profile):
    check_case(dev, (2, 2, 37, 50, 32), profile, 0.1)
    check_case(dev, (1, 2, 50, 37, 36), profile, None)


@pytest.mark.parametrize("p", [None, 0.1])
def test_an_image_without_keys_is_exactly_zero(dev, p):
    check_case(dev, (1, 1, 17, 70, 32), "unit", p, dead_image=True)


@pytest.mark.parametrize("case", SMALL + LARGE[:3], ids=str)
def test_without_rng_out_is_the_inference_kernel(dev, case):
    from trackformer_amd import _cabi
    N, H, Lq, Lk, D = case
    q, k, v, scale = NA.attention_operands("unit", N, Lq, Lk, H, D, 7, device=dev)
    km = AT.masks(N, Lk, 7, device=dev) if case in MASKED else None
    got = run_kernels(dev, q, k, v, torch.zeros_like(q), scale, km, None, None)["out"]
    want = torch.empty_like(q)
    E = H * D
    rc = _cabi.lib().tf_mha_core_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), want.data_ptr(), _ptr(km), N, Lq, Lk, H, D, E, E, E, E, scale,
                                     torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- 2. the Function ------------------------------------------------------------------------------------------------------------------
def _function_operands(dev, N, L, H, D, seed, mask=True):
    q, k, v, _ = NA.attention_operands("unit", N, L, L, H, D, seed, device=dev)
    qk = torch.cat([q.reshape(N, L, H * D), k.reshape(N, L, H * D)], -1).contiguous()
    km = AT.masks(N, L, seed, device=dev).bool() if mask else None
    return qk, v.reshape(N, L, H * D).contiguous(), AT.grad_operand(N, L, H, D, seed, device=dev).reshape(N, L, H * D), km


def _apply(qk, v, H, km, p, rng, up):
    from trackformer_amd import fused
    a, b = qk.clone().requires_grad_(True), v.clone().requires_grad_(True)
    out = fused.mha_core_train(a, b, H, km, p, rng)
    out.backward(up)
    return out.detach(), a.grad, b.grad


@pytest.mark.parametrize("N,L,H,D,p", [(2, 45, 8, 32, 0.1), (1, 314, 8, 36, 0.1), (2, 45, 8, 32, None)])
def test_function_against_float64_autograd(dev, N, L, H, D, p):
    qk, v, up, km = _function_operands(dev, N, L, H, D, 5)
    rng = _rng(dev) if p is not None else None
    out, dqk, dv = _apply(qk, v, H, km, 0.0 if p is None else p, rng, up)
    E = H * D
    q4, k4, v4, up4 = (t.reshape(N, L, H, D) for t in (qk[..., :E], qk[..., E:], v, up))
    keep = AT.keep_of(rng, p, N, H, L, L) if p is not None else None
    want = AT.formulation(q4, k4, v4, up4, float(D) ** -0.5, km, keep, p, dtype=torch.float64)
    ref = AT.reference(q4, k4, v4, up4, float(D) ** -0.5, km, keep, p)
    for name in AT.OUTPUTS:
        assert torch.allclose(ref[name].ref, want[name], rtol=1e-11, atol=1e-13), name
    got = {"out": out.view(N, L, H, D), "dq": dqk[..., :E].reshape(N, L, H, D), "dk": dqk[..., E:].reshape(N, L, H, D), "dv": dv.view(N, L, H, D)}
    AT.check(got, ref, AT.formulation(q4, k4, v4, up4, float(D) ** -0.5, km, keep, p), km, "Function %s" % ((N, L, H, D, p),))


def test_bit_identity_across_calls_streams_a_graph_replay_and_seeds(dev):
    from trackformer_amd import fused
    N, L, H, D, p = 2, 337, 8, 32, 0.1
    qk, v, up, km = _function_operands(dev, N, L, H, D, 11)
    rng = _rng(dev)
    first = _apply(qk, v, H, km, p, rng, up)

    def same(res, what):
        torch.cuda.synchronize(dev)
        for a, b, name in zip(res, first, ("out", "dqk", "dv")):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, name)

    same(_apply(qk, v, H, km, p, rng, up), "second call")
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        res = _apply(qk, v, H, km, p, rng, up)
    torch.cuda.current_stream(dev).wait_stream(side)
    same(res, "side stream")
    # a captured graph that holds forward + backward (one chain of two kernels), with a fixed rng tensor
    a, b = qk.clone().requires_grad_(True), v.clone().requires_grad_(True)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(graph):
        out = fused.mha_core_train(a, b, H, km, p, rng)
        ga, gb = torch.autograd.grad(out, (a, b), up)
    for _ in range(2):
        for t in (out, ga, gb):
            t.detach().fill_(float("nan"))
        graph.replay()
        same((out.detach(), ga, gb), "graph replay")
    rng.copy_(_rng(dev, SEED + 1, OFFSET))   # the graph reads rng when it runs: another stream, another mask
    graph.replay()
    torch.cuda.synchronize(dev)
    assert not torch.equal(out.detach(), first[0])
    # the same torch.manual_seed gives the same masks
    res = []
    for _ in range(2):
        torch.manual_seed(99)
        res.append(_apply(qk, v, H, km, p, fused.dropout_rng(dev), up))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert not torch.equal(res[0][0], first[0])


# ---- 3. one decoder layer in three forms under one seed -------------------------------------------------------------------------------
@contextlib.contextmanager
def _routes(attention, dropout, parents):
    from trackformer_amd import fused
    fused.set_attention_training(attention)
    fused.set_dropout_training(dropout)
    fused.set_layernorm_training(parents)
    fused.set_split_linear_training(parents)
    try:
        yield
    finally:
        for f in (fused.set_attention_training, fused.set_dropout_training, fused.set_layernorm_training, fused.set_split_linear_training):
            f(None)


def test_decoder_layer_three_forms_under_one_seed(dev):
    from tests.test_dropout_train_gpu import recorded_draws
    from trackformer_amd import fused
    from trackformer_amd.deformable_transformer import DeformableTransformerDecoderLayer
    from trackformer_amd.msda import attach_host_shapes
    hw = [(12, 16), (6, 8)]
    S = sum(h * w_ for h, w_ in hw)
    Lq = 42                                  # not a multiple of 4: the padded rows of the mask contract
    shapes = attach_host_shapes(torch.tensor(hw, device=dev), hw)
    g = torch.Generator().manual_seed(10)
    memory = torch.randn(2, S, 256, generator=g).to(dev)
    tgt, qpos, up = (torch.randn(2, Lq, 256, generator=g).to(dev) for _ in range(3))
    ref_pts = torch.rand(2, Lq, 2, 2, generator=g).to(dev)
    filler = torch.zeros(2, Lq, dtype=torch.bool, device=dev)
    filler[1, -5:] = True

    def build():
        return DeformableTransformerDecoderLayer(d_model=256, d_ffn=256, dropout=0.1, n_levels=2, n_heads=8, n_points=4)

    torch.manual_seed(3)
    layer = build()
    with torch.no_grad():
        for p in layer.cross_attn.sampling_offsets.weight, layer.cross_attn.attention_weights.weight:
            p.copy_(0.02 * torch.randn_like(p))
    layer = layer.to(dev).train()
    layer64 = build().double().to(dev).train()
    layer64.load_state_dict({k: v.double() for k, v in layer.state_dict().items()})

    def grads_of(mod, dt, dropout, parents):
        mod.zero_grad()
        torch.manual_seed(1234)
        with _routes(True, dropout, parents), recorded_draws() as draws:
            fused.attention_train_counts(reset=True)
            t = tgt.to(dt).clone().requires_grad_(True)
            m = memory.to(dt).clone().requires_grad_(True)
            out = mod(t, qpos.to(dt), ref_pts.to(dt), m, shapes, filler_key_mask=filler)
            out.backward(up.to(dt))
            grads = {k: p.grad.clone() for k, p in mod.named_parameters()}
            grads["tgt"], grads["memory"] = t.grad.clone(), m.grad.clone()
            counts = fused.attention_train_counts(reset=True)
        return grads, draws, counts

    want, draws64, c64 = grads_of(layer64, torch.float64, "reference", False)
    ref32, draws32, c32 = grads_of(layer, torch.float32, "reference", False)
    own, draws_own, c_own = grads_of(layer, torch.float32, True, True)
    assert len(draws64) == 5                 # the attention weights, three residual sites, the feed-forward hidden activation
    for other in (draws32, draws_own):       # all three saw the same masks
        assert len(other) == len(draws64) and all(torch.equal(a, b) for a, b in zip(draws64, other))
    assert c64 == c32 == {"own": 0, "own_dropout": 0, "reference": 1, "torch": 0}, (c64, c32)
    assert c_own == {"own": 0, "own_dropout": 1, "reference": 0, "torch": 0}, c_own

    bad = []
    for k in want:
        e_ref = float((ref32[k].double() - want[k]).norm() / want[k].norm())
        e_own = float((own[k].double() - want[k]).norm() / want[k].norm())
        limit = max(G.FP32_FACTOR * e_ref, G.CLASS_MIN)
        print("%-44s fp32 reference mode %.3e   own route %.3e   (limit %.3e)" % (k, e_ref, e_own, limit))
        if not e_own <= limit:
            bad.append((k, e_own, limit))
    assert not bad, bad


def test_sites_the_gate_declines_keep_todays_line(dev):
    """Dropout inside nn.MultiheadAttention without set_dropout_training, and a float mask: today's call, counted `torch`, bit for bit."""
    from trackformer_amd import fused
    from trackformer_amd.deformable_transformer import DeformableTransformerDecoderLayer
    torch.manual_seed(0)
    layer = DeformableTransformerDecoderLayer(d_model=256, d_ffn=64, dropout=0.1, n_levels=1, n_heads=8, n_points=1).to(dev).train()
    tgt, pos = torch.randn(2, 21, 256, device=dev, requires_grad=True), torch.randn(2, 21, 256, device=dev)
    torch.manual_seed(5)
    want = layer.self_attention_training(tgt, pos, None)
    fused.set_attention_training(True)
    torch.manual_seed(5)
    got = layer.self_attention_training(tgt, pos, None)
    assert fused.attention_train_counts(reset=True) == {"own": 0, "own_dropout": 0, "reference": 0, "torch": 1}
    assert torch.equal(got, want)
    layer.self_attn.dropout = 0.0
    fmask = torch.zeros(2, 21, device=dev)
    layer.self_attention_training(tgt, pos, fmask)
    layer.self_attention_training(tgt, pos, None).sum().backward()
    assert fused.attention_train_counts(reset=True) == {"own": 1, "own_dropout": 0, "reference": 0, "torch": 1}
    assert layer.self_attn.in_proj_weight.grad is not None and tgt.grad is not None
