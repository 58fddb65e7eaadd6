"""GPU (-m gpu): dropout inside the training kernels on the device (include/tf_fused.h: DROPOUT INSIDE THE TRAINING KERNELS;
trackformer_amd/csrc/dropout_rng.h, dropout_train.h; fused.set_dropout_training) -- the mask against the numpy restatement of the generator
contract, the kernels through the C ABI and the autograd Functions against float64 with the yardstick of tests/util_dropout_train.py, bit
equality across calls / streams / a captured graph, the feed-forward route against a torch multiply with the restated mask, seeding,
what is declined, and one encoder and one decoder layer with dropout 0.1 in three forms under one seed (float64 "reference" mode, fp32
"reference" mode, fp32 on the own kernels): the layer-level test carries the accuracy claim of the route.

First run on an MI355X (pytest -s), worst normalised excess next to the fp32 formulation's own with the same mask; bound 9.5e-07 for
out / dx / dres, dgamma / dbeta 9.5e-07 up to 1152 rows, 1.8e-06 at 4099 rows, 5.1e-06 at 32 769:

    case                       out (torch fp32)       dx (torch fp32)        dres (torch fp32)      dgamma (torch fp32)    dbeta (torch fp32)
    unit x unit [1, 4]         9.8e-09 (9.8e-09)      2.3e-09 (3.2e-09)      2.4e-09 (3.3e-09)      9.6e-09 (1.6e-08)      0.0e+00 (0.0e+00)
    unit x unit [5, 260]       5.1e-08 (4.8e-08)      5.2e-08 (3.3e-08)      3.1e-08 (2.6e-08)      3.0e-08 (4.5e-08)      1.3e-07 (8.5e-08)
    unit x unit [257, 288]     7.2e-08 (7.2e-08)      6.9e-08 (8.9e-08)      5.3e-08 (6.1e-08)      6.5e-09 (6.0e-09)      3.1e-08 (2.8e-08)
    unit x unit [64, 4096]     8.7e-08 (8.7e-08)      9.3e-08 (9.4e-08)      6.1e-08 (5.0e-08)      2.2e-08 (4.1e-08)      6.3e-08 (1.5e-07)
    unit x unit [4099, 256]    8.6e-08 (8.7e-08)      7.6e-08 (1.2e-07)      5.4e-08 (5.4e-08)      2.3e-09 (1.7e-09)      6.9e-09 (6.2e-09)
    unit x unit [32769, 256]   8.6e-08 (1.1e-07)      1.0e-07 (1.1e-07)      6.8e-08 (6.5e-08)      1.4e-09 (7.9e-10)      4.8e-09 (2.6e-09)

Layer level, rel. L2 error against the float64 twin per gradient tensor (own route / fp32 reference mode): encoder layer 1.07e-07 ..
7.99e-07 against 8.16e-08 .. 8.77e-07, decoder layer 7.50e-08 .. 7.83e-07 against 1.02e-07 .. 7.38e-07; the ratio per tensor lies
between 0.43 (decoder norm3.bias) and 1.31 (encoder norm2.bias), bound 4; all three forms saw the same masks, 2 + 1 and 3 + 1 sites on the
own kernels, none under *_torch."""
import contextlib

import numpy as np
import pytest
import torch

from tests import util_dropout_train as D
from tests import util_norm_attn_numerics as NA
from tests import util_train_gradients as G

pytestmark = pytest.mark.gpu

CANARY = -4321.5
GUARD = 3
SEED, OFFSET = 0x9E3779B97F4A7C15 - 2 ** 64, 0x7FEDCBA987654321   # both high halves set
P = 0.1


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
    prev = fused._dropout_train, fused._layernorm_train, fused._split_linear_train
    fused._dropout_train = fused._layernorm_train = fused._split_linear_train = None
    fused.dropout_train_counts(reset=True)
    try:
        yield
    finally:
        fused._dropout_train, fused._layernorm_train, fused._split_linear_train = prev
        fused.dropout_train_counts(reset=True)


@contextlib.contextmanager
def routes(dropout=True, parents=True):
    from trackformer_amd import fused
    prev = fused._dropout_train, fused._layernorm_train, fused._split_linear_train
    fused.set_dropout_training(dropout)
    fused.set_layernorm_training(parents)
    fused.set_split_linear_training(parents)
    try:
        yield fused
    finally:
        fused._dropout_train, fused._layernorm_train, fused._split_linear_train = prev


@contextlib.contextmanager
def recorded_draws(fixed=None):
    """Records every fused.dropout_rng draw (host copies); fixed: hand out clones of this tensor instead of drawing."""
    from trackformer_amd import fused
    real, draws = fused.dropout_rng, []

    def draw(device):
        t = real(device) if fixed is None else fixed.clone()
        draws.append(t.cpu())
        return t
    fused.dropout_rng = draw
    try:
        yield draws
    finally:
        fused.dropout_rng = real


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _rng(dev, seed=SEED, offset=OFFSET):
    return torch.tensor([seed, offset], dtype=torch.int64, device=dev)


def _guarded(rows, cols, dev):
    return torch.full((rows + GUARD, cols), CANARY, dtype=torch.float32, device=dev)


# ---- 1. the mask -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 2 ** 34], ids=["first0", "first2p34"])
@pytest.mark.parametrize("p", [2.0 ** -31, 0.1, 0.5, 0.9999], ids=["tiny", "0.1", "0.5", "0.9999"])
def test_mask_is_the_restatement_on_the_device(dev, p, first):
    from trackformer_amd import _cabi
    for n in (4, 260, 4100):
        keep = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device=dev)
        rc = _cabi.lib().tf_dropout_keep_u8(_rng(dev).data_ptr(), p, first, n, keep.data_ptr(), _stream(dev))
        _cabi.check(rc, "tf_dropout_keep_u8")
        assert _cabi.lib().tf_msda_last_kernel() == b"dropout_keep_u8"
        got = keep.cpu().numpy()
        assert (got[n:] == 0xA5).all(), "tf_dropout_keep_u8 wrote behind its output"
        assert np.array_equal(got[:n], D.keep_mask(SEED, OFFSET, p, n, first)), (p, n, first)


# ---- 2. the kernels through the C ABI ------------------------------------------------------------------------------------------------------
class Pair:
    """One forward + backward through the C ABI with canary rows behind every output and the workspace."""

    def __init__(self, rows, C, dev):
        from trackformer_amd import _cabi
        self.rows, self.C = rows, C
        self.nbytes = int(_cabi.lib().tf_add_layernorm_bwd_workspace_bytes(rows, C))
        self.nb = self.nbytes // (8 * C)
        self.out, self.stats = _guarded(rows, C, dev), _guarded(rows, 2, dev)
        self.dx, self.dres = _guarded(rows, C, dev), _guarded(rows, C, dev)
        self.dg, self.db, self.ws = _guarded(1, C, dev), _guarded(1, C, dev), _guarded(self.nb, 2 * C, dev)

    def __call__(self, x, res, gamma, beta, dy, rng, p=P):
        from trackformer_amd import _cabi
        L, s = _cabi.lib(), _stream(x.device)
        rc = L.tf_add_dropout_layernorm_train_f32(x.data_ptr(), res.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rng.data_ptr(), p,
                                                  self.out.data_ptr(), self.stats.data_ptr(), self.rows, self.C, D.EPS, s)
        _cabi.check(rc, "tf_add_dropout_layernorm_train_f32")
        rc = L.tf_add_dropout_layernorm_bwd_f32(dy.data_ptr(), x.data_ptr(), res.data_ptr(), gamma.data_ptr(), self.stats.data_ptr(),
                                                rng.data_ptr(), p, self.dx.data_ptr(), self.dres.data_ptr(), self.dg.data_ptr(),
                                                self.db.data_ptr(), self.ws.data_ptr(), self.nbytes, self.rows, self.C, s)
        _cabi.check(rc, "tf_add_dropout_layernorm_bwd_f32")
        return self

    def outputs(self):
        r = self.rows
        return {"out": self.out[:r], "dx": self.dx[:r], "dres": self.dres[:r], "dgamma": self.dg[0], "dbeta": self.db[0]}

    def assert_canaries(self):
        for name, t, n in (("out", self.out, self.rows), ("stats", self.stats, self.rows), ("dx", self.dx, self.rows),
                           ("dres", self.dres, self.rows), ("dgamma", self.dg, 1), ("dbeta", self.db, 1), ("workspace", self.ws, self.nb)):
            assert bool((t[n:] == CANARY).all()), "wrote behind " + name


# (32769, 256): the first row count with 2048-block rule of more than 16 rows per block; (3, 516): MAXCH 4, one lane in the third chunk
# and none in the fourth
@pytest.mark.parametrize("rows,C", [(1, 4), (5, 260), (257, 288), (64, 4096), (4099, 256), (32769, 256), (3, 516)])
def test_kernels_against_float64(dev, rows, C):
    from trackformer_amd import _cabi
    x, res, gamma, beta, dy = D.operands("unit", "unit", rows, C, rows + C, device=dev)
    rng = _rng(dev)
    pair = Pair(rows, C, dev)(x, res, gamma, beta, dy, rng)
    torch.cuda.synchronize(dev)
    assert _cabi.lib().tf_msda_last_kernel() == b"add_layernorm_bwd_reduce_f32"
    pair.assert_canaries()
    keep = D.keep_of(rng, P, (rows, C))
    D.check(pair.outputs(), D.reference(x, res, gamma, beta, dy, keep, P), D.fp32_formulation(x, res, gamma, beta, dy, keep, P), rows, keep,
            "unit x unit [%d, %d]" % (rows, C))


@pytest.mark.parametrize("profile", NA.LN_PROFILES)
def test_every_profile_against_float64(dev, profile):
    from tests import util_layernorm_train as Y
    rows, C = 257, 288
    rng = _rng(dev)
    for i, dy_profile in enumerate(Y.DY_PROFILES):
        p = (0.1, 0.5)[i % 2]
        x, res, gamma, beta, dy = D.operands(profile, dy_profile, rows, C, 17 + i, device=dev)
        pair = Pair(rows, C, dev)(x, res, gamma, beta, dy, rng, p)
        keep = D.keep_of(rng, p, (rows, C))
        D.check(pair.outputs(), D.reference(x, res, gamma, beta, dy, keep, p), D.fp32_formulation(x, res, gamma, beta, dy, keep, p), rows, keep,
                "%s x %s p %g" % (profile, dy_profile, p))
        pair.assert_canaries()


# ---- 3. bit identity -------------------------------------------------------------------------------------------------------------------
def test_bit_identity_across_calls_streams_and_a_graph_replay(dev):
    rows, C = 4099, 288
    x, res, gamma, beta, dy = D.operands("unit", "row_spread", rows, C, 11, device=dev)
    rng = _rng(dev)
    first = {k: v.clone() for k, v in Pair(rows, C, dev)(x, res, gamma, beta, dy, rng).outputs().items()}

    def same(pair, what):
        torch.cuda.synchronize(dev)
        pair.assert_canaries()
        for k, v in pair.outputs().items():
            assert torch.equal(v.view(torch.int32), first[k].view(torch.int32)), (what, k)

    same(Pair(rows, C, dev)(x, res, gamma, beta, dy, rng), "second call")
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        pair = Pair(rows, C, dev)(x, res, gamma, beta, dy, rng)
    torch.cuda.current_stream(dev).wait_stream(side)
    same(pair, "side stream")
    # a captured graph that holds forward + backward: one chain of three kernels, no parallel branches
    pair = Pair(rows, C, dev)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(graph):
        pair(x, res, gamma, beta, dy, rng)
    for _ in range(2):
        for t, n in ((pair.out, rows), (pair.dx, rows), (pair.dres, rows), (pair.dg, 1), (pair.db, 1)):
            t[:n].fill_(float("nan"))
        graph.replay()
        same(pair, "graph replay")
    # the graph reads rng when it runs: another stream, another mask
    rng.copy_(_rng(dev, SEED + 1, OFFSET))
    graph.replay()
    torch.cuda.synchronize(dev)
    assert not torch.equal(pair.dres[:rows], first["dres"])
    keep = D.keep_of(rng, P, (rows, C))
    assert bool((pair.dres[:rows][~keep] == 0).all()) and bool((pair.dres[:rows][keep] == pair.dx[:rows][keep] * float(D.scale32(P))).all())


# ---- 4. the autograd Function through residual_norm ------------------------------------------------------------------------------------
def _module(C, dev, gamma, beta):
    norm = torch.nn.LayerNorm(C, eps=D.EPS).to(dev)
    with torch.no_grad():
        norm.weight.copy_(gamma)
        norm.bias.copy_(beta)
    return norm


@pytest.mark.parametrize("case", ["res_requires_grad", "res_constant", "frozen_affine", "noncontiguous_grad_output", "x_is_res",
                                  "noncontiguous_res"])
def test_autograd_through_dropout_residual_norm(dev, case):
    rows, C = 300, 288
    x0, res0, gamma, beta, dy = D.operands("unit", "unit", rows, C, 23, device=dev)
    x0, res0, dy = x0.reshape(2, rows // 2, C), res0.reshape(2, rows // 2, C), dy.reshape(2, rows // 2, C)
    norm = _module(C, dev, gamma, beta)
    drop = torch.nn.Dropout(P).train()
    if case == "frozen_affine":
        norm.weight.requires_grad_(False)
        norm.bias.requires_grad_(False)
    x = x0.clone().requires_grad_(True)
    res = x if case == "x_is_res" else res0.clone().requires_grad_(case != "res_constant")
    calls = []
    handle = drop.register_forward_hook(lambda *a: calls.append(1))
    with routes() as fused, recorded_draws() as draws:
        if case == "noncontiguous_res":   # [Lq, N, C] transposed, as nn.MultiheadAttention hands the decoder its output
            res = res0.transpose(0, 1).contiguous().requires_grad_(True)
            y = fused.residual_norm(x, res.transpose(0, 1), norm, False, dropout=drop)
        else:
            y = fused.residual_norm(x, res, norm, False, dropout=drop)
        assert type(y.grad_fn).__name__ == "_DropoutLayerNormTrainBackward"
        assert fused.dropout_train_counts() == {"ln_own": 1, "ln_torch": 0, "ffn_own": 0, "ffn_torch": 0}
        assert fused.layernorm_train_counts()["own"] == 0
    handle.remove()
    assert not calls and len(draws) == 1          # the module itself never ran; one draw for the site
    if case == "noncontiguous_grad_output":
        wide = torch.zeros(2, rows // 2, 2 * C, device=dev)
        wide[..., ::2] = dy
        g_out = wide[..., ::2]
        assert not g_out.is_contiguous()
    else:
        g_out = dy
    y.backward(g_out)
    torch.cuda.synchronize(dev)
    keep = D.keep_of(draws[0].to(dev), P, (rows, C))
    x2, r2, dy2 = x0.reshape(rows, C), (x0 if case == "x_is_res" else res0).reshape(rows, C), dy.reshape(rows, C)
    ref = D.reference(x2, r2, gamma, beta, dy2, keep, P)
    fp32 = D.fp32_formulation(x2, r2, gamma, beta, dy2, keep, P)
    got = {"out": y.detach().reshape(rows, C), "dx": x.grad.reshape(rows, C), "dgamma": norm.weight.grad, "dbeta": norm.bias.grad}
    if case == "x_is_res":      # one leaf, both gradients: dx + dres
        ref["dx"] = NA.Ref(ref["dx"].ref + ref["dres"].ref, ref["dx"].scale + ref["dres"].scale, ref["dx"].floor + ref["dres"].floor)
        fp32["dx"] = fp32["dx"] + fp32["dres"]
    elif case == "res_constant":
        assert res.grad is None
    elif case == "noncontiguous_res":
        got["dres"] = res.grad.transpose(0, 1).reshape(rows, C)
    else:
        got["dres"] = res.grad.reshape(rows, C)
    if case == "frozen_affine":
        assert norm.weight.grad is None and norm.bias.grad is None
    D.check(got, ref, fp32, rows, keep, case)


# ---- 5. the feed-forward route -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N", [(300, 256, 1024), (37, 64, 192)])
def test_ffn_route_against_a_torch_multiply_with_the_restated_mask(dev, M, K, N):
    torch.manual_seed(5)
    lin = torch.nn.Linear(K, N).to(dev)
    x0 = torch.randn(2, M, K, device=dev)
    up = torch.randn(2, M, N, device=dev)
    drop = torch.nn.Dropout(P).train()
    rng = _rng(dev)
    factor = D.keep_of(rng, P, (2, M, N)).float() * float(D.scale32(P))

    def run(own):
        lin.zero_grad()
        x = x0.clone().requires_grad_(True)
        if own:
            y = fused.linear_train(x, lin.weight, lin.bias, relu=True, dropout=drop)
            assert type(y.grad_fn).__name__ == "_LinearDropoutTrainBackward"
        else:
            y = fused.linear_train(x, lin.weight, lin.bias, relu=True) * factor
        y.backward(up)
        return y.detach(), x.grad.clone(), lin.weight.grad.clone(), lin.bias.grad.clone()

    with routes() as fused, recorded_draws(fixed=rng) as draws:
        a, b = run(True), run(False)
        assert len(draws) == 1
    torch.cuda.synchronize(dev)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))        # forward bits
    for name, p_, q_ in zip(("dx", "dw", "db"), a[1:], b[1:]):
        assert torch.equal(p_, q_), name
    dropped = factor == 0
    assert bool((a[0][dropped] == 0).all()) and 0.05 < float(dropped.float().mean()) < 0.15


# ---- 6. seeding ----------------------------------------------------------------------------------------------------------------------------
def test_torch_manual_seed_governs_the_masks(dev):
    rows, C = 64, 256
    x0, res0, gamma, beta, dy = D.operands("unit", "unit", rows, C, 3, device=dev)
    norm = _module(C, dev, gamma, beta)
    drop = torch.nn.Dropout(P).train()

    def run(seed):
        torch.manual_seed(seed)
        norm.zero_grad()
        x, res = x0.clone().requires_grad_(True), res0.clone().requires_grad_(True)
        with routes() as fused, recorded_draws() as draws:
            y = fused.residual_norm(x, res, norm, False, dropout=drop)
        y.backward(dy)
        return draws[0], (y.detach(), x.grad, res.grad, norm.weight.grad.clone(), norm.bias.grad.clone())

    d1, a = run(7)
    d2, b = run(7)
    d3, c = run(8)
    assert torch.equal(d1, d2) and all(torch.equal(p_.view(torch.int32), q_.view(torch.int32)) for p_, q_ in zip(a, b))
    assert not torch.equal(d1, d3)
    assert not torch.equal(D.keep_of(d1, P, (rows, C)), D.keep_of(d3, P, (rows, C))) and not torch.equal(a[0], c[0])


# ---- 7. what is declined -------------------------------------------------------------------------------------------------------------------
def test_declines_on_the_device_are_counted_and_give_todays_result(dev):
    x = torch.randn(6, 256, device=dev, requires_grad=True)
    cases = [
        (x.detach().reshape(-1)[1:1 + 5 * 256].reshape(5, 256), torch.randn(5, 256, device=dev), torch.nn.LayerNorm(256), P),   # misaligned
        (torch.randn(6, 258, device=dev), torch.randn(6, 258, device=dev), torch.nn.LayerNorm(258), P),                      # C % 4
        (torch.randn(2, 4100, device=dev), torch.randn(2, 4100, device=dev), torch.nn.LayerNorm(4100), P),                   # C > 4096
        (x, torch.randn(6, 256, device=dev), torch.nn.LayerNorm(256, elementwise_affine=False), P),                          # no affine
    ]
    with routes() as fused:
        for i, (xi, ri, norm, p) in enumerate(cases):
            norm = norm.to(dev)
            drop = torch.nn.Dropout(p).train()
            torch.manual_seed(40 + i)
            got = fused.residual_norm(xi, ri, norm, False, dropout=drop)
            torch.manual_seed(40 + i)
            want = norm(xi + drop(ri))
            assert torch.equal(got, want), i
            assert fused.dropout_train_counts()["ln_torch"] == i + 1 and fused.dropout_train_counts()["ln_own"] == 0
        # p out of range: not an active dropout site -- today's lines, uncounted (p = 1 drops everything)
        for p in (0.0, 1.0):
            drop = torch.nn.Dropout(p).train()
            norm = torch.nn.LayerNorm(256).to(dev)
            r = torch.randn(6, 256, device=dev)
            got = fused.residual_norm(x, r, norm, False, dropout=drop)
            assert type(got.grad_fn).__name__ == "_LayerNormTrainBackward"      # today's layernorm_train, untouched
            assert torch.equal(got, fused.residual_norm(x, drop(r), norm, False))
        assert fused.dropout_train_counts() == {"ln_own": 0, "ln_torch": 4, "ffn_own": 0, "ffn_torch": 0}
        # the library itself refuses such a p
        from trackformer_amd import _cabi
        y = torch.zeros(8, device=dev)
        for p in (0.0, 1.0, float("nan")):
            assert _cabi.lib().tf_dropout_inplace_f32(y.data_ptr(), _rng(dev).data_ptr(), p, 8, _stream(dev)) == -2
        # a feed-forward site whose d_ffn is no multiple of 4, and one that is no ReLU
        lin = torch.nn.Linear(256, 258).to(dev)
        drop = torch.nn.Dropout(P).train()
        assert fused.dropout_ffn_hidden(x, lin, True, drop) is None and fused.dropout_ffn_hidden(x, lin, False, drop) is None
        assert fused.dropout_train_counts()["ffn_torch"] == 2
    # parent routes off: counted, today's graph
    with routes(parents=False) as fused:
        fused.dropout_train_counts(reset=True)
        norm = torch.nn.LayerNorm(256).to(dev)
        y = fused.residual_norm(x, torch.randn(6, 256, device=dev), norm, False, dropout=torch.nn.Dropout(P).train())
        assert type(y.grad_fn).__name__ == "NativeLayerNormBackward0"
        assert fused.dropout_train_counts() == {"ln_own": 0, "ln_torch": 1, "ffn_own": 0, "ffn_torch": 0}


# ---- 8. one encoder and one decoder layer, three forms under one seed ---------------------------------------------------------------------
def _three_forms(dev, build, run, n_ln, n_ffn):
    from trackformer_amd import fused
    torch.manual_seed(3)
    layer = build()
    with torch.no_grad():
        for m in layer.modules():
            if type(m).__name__ == "MSDeformAttn":
                for p in m.sampling_offsets.weight, m.attention_weights.weight:
                    p.copy_(0.02 * torch.randn_like(p))
    layer = layer.to(dev).train()
    layer64 = build().double().to(dev).train()
    layer64.load_state_dict({k: v.double() for k, v in layer.state_dict().items()})

    def grads_of(mod, dt, dropout, parents):
        mod.zero_grad()
        torch.manual_seed(1234)
        with routes(dropout, parents), recorded_draws() as draws:
            fused.dropout_train_counts(reset=True)
            grads = run(mod, dt)
            counts = fused.dropout_train_counts(reset=True)
        return grads, draws, counts

    want, draws64, _ = grads_of(layer64, torch.float64, "reference", False)
    ref32, draws32, c32 = grads_of(layer, torch.float32, "reference", False)
    own, draws_own, c_own = grads_of(layer, torch.float32, True, True)
    assert len(draws64) == n_ln + n_ffn
    for other in (draws32, draws_own):          # all three saw the same masks
        assert len(other) == len(draws64) and all(torch.equal(a, b) for a, b in zip(draws64, other))
    assert c_own == {"ln_own": n_ln, "ln_torch": 0, "ffn_own": n_ffn, "ffn_torch": 0}, c_own
    assert c32 == {"ln_own": 0, "ln_torch": 0, "ffn_own": 0, "ffn_torch": 0}

    def rel_l2(a, b):
        return float((a.double() - b).norm() / b.norm())

    bad = []
    for k in want:
        e_ref, e_own = rel_l2(ref32[k], want[k]), rel_l2(own[k], want[k])
        limit = max(G.FP32_FACTOR * e_ref, G.CLASS_MIN)
        print("%-44s fp32 reference mode %.3e   own route %.3e   (limit %.3e)" % (k, e_ref, e_own, limit))
        if not e_own <= limit:
            bad.append((k, e_own, limit))
    assert not bad, bad


def test_encoder_layer_three_forms_under_one_seed(dev):
    from trackformer_amd.deformable_transformer import DeformableTransformerEncoderLayer
    from trackformer_amd.msda import attach_host_shapes
    hw = [(12, 16), (6, 8)]
    S = sum(h * w_ for h, w_ in hw)
    shapes = attach_host_shapes(torch.tensor(hw, device=dev), hw)
    g = torch.Generator().manual_seed(9)
    src, pos, up = (torch.randn(2, S, 256, generator=g).to(dev) for _ in range(3))
    ref_pts = torch.rand(2, S, 2, 2, generator=g).to(dev)

    def run(mod, dt):
        s = src.to(dt).clone().requires_grad_(True)
        out = mod(s, pos.to(dt), ref_pts.to(dt), shapes)
        out.backward(up.to(dt))
        grads = {k: p.grad.clone() for k, p in mod.named_parameters()}
        grads["src"] = s.grad.clone()
        return grads

    _three_forms(dev, lambda: DeformableTransformerEncoderLayer(d_model=256, d_ffn=256, dropout=0.1, n_levels=2, n_heads=8, n_points=4), run, 2, 1)


def test_decoder_layer_three_forms_under_one_seed(dev):
    from trackformer_amd.deformable_transformer import DeformableTransformerDecoderLayer
    from trackformer_amd.msda import attach_host_shapes
    hw = [(12, 16), (6, 8)]
    S = sum(h * w_ for h, w_ in hw)
    Lq = 40
    shapes = attach_host_shapes(torch.tensor(hw, device=dev), hw)
    g = torch.Generator().manual_seed(10)
    memory = torch.randn(2, S, 256, generator=g).to(dev)
    tgt, qpos, up = (torch.randn(2, Lq, 256, generator=g).to(dev) for _ in range(3))
    ref_pts = torch.rand(2, Lq, 2, 2, generator=g).to(dev)

    def build():
        layer = DeformableTransformerDecoderLayer(d_model=256, d_ffn=256, dropout=0.1, n_levels=2, n_heads=8, n_points=4)
        layer.self_attn.dropout = 0.0        # the dropout inside nn.MultiheadAttention is not covered: it would draw from torch's generator
        return layer

    def run(mod, dt):
        t = tgt.to(dt).clone().requires_grad_(True)
        m = memory.to(dt).clone().requires_grad_(True)
        out = mod(t, qpos.to(dt), ref_pts.to(dt), m, shapes)
        out.backward(up.to(dt))
        grads = {k: p.grad.clone() for k, p in mod.named_parameters()}
        grads["tgt"], grads["memory"] = t.grad.clone(), m.grad.clone()
        return grads

    _three_forms(dev, build, run, 3, 1)
