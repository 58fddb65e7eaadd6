"""GPU (-m gpu): the training path of the residual + LayerNorm sites on the device (include/tf_fused.h: THE BACKWARD OF THE RESIDUAL
LAYERNORM; trackformer_amd/csrc/layernorm_bwd.h; fused.layernorm_train) -- the kernels through the C ABI and the autograd Function
against float64 computed on the device with the yardstick of tests/util_layernorm_train.py, canary rows behind every output and the
workspace, bit equality across calls / streams / a captured graph / a busy neighbour stream, and the non-finite contract.

Worst normalised excess per case (pytest -s) as the first run on an MI355X printed it, next to the fp32 formulation's own (autograd
through F.layer_norm(x + res) on the same operands); bounds: dz 9.5e-07, dgamma / dbeta 9.5e-07 up to 1152 rows, 1.8e-06 at 4099 rows,
5.1e-06 at 32 768:

    case                                          dz (torch fp32)        dgamma (torch fp32)    dbeta (torch fp32)
    unit x unit [1, 4] + res                      1.7e-08 (1.3e-08)      3.2e-08 (1.0e-07)      0.0e+00 (0.0e+00)
    unit x unit [5, 260] + res                    9.3e-08 (1.3e-07)      1.3e-07 (1.6e-07)      1.3e-07 (8.5e-08)
    unit x unit [257, 288] + res                  1.6e-07 (1.6e-07)      3.5e-08 (3.5e-08)      3.1e-08 (2.8e-08)
    unit x unit [4099, 256] + res                 1.8e-07 (1.7e-07)      9.8e-09 (8.5e-09)      6.9e-09 (6.2e-09)
    unit x unit [4099, 288] + res                 1.8e-07 (2.1e-07)      1.1e-08 (8.9e-09)      7.2e-09 (6.0e-09)
    unit x unit [64, 4096] + res                  2.0e-07 (1.6e-07)      1.1e-07 (2.0e-07)      6.3e-08 (1.5e-07)
    unit x unit [32768, 256] + res                2.0e-07 (2.0e-07)      6.0e-09 (4.0e-09)      5.3e-09 (2.5e-09)
    unit x unit [32769, 256] + res                2.0e-07 (2.1e-07)      5.8e-09 (3.6e-09)      4.8e-09 (2.6e-09)
    worst of the 51 profile pairs at [4099, 288], dz    : 3.1e-07 (torch fp32 3.6e-07, bound 9.5e-07) at chan_spread x spread [4099, 288] + res
    worst of the 51 profile pairs at [4099, 288], dgamma: 3.6e-08 (torch fp32 2.5e-08, bound 1.8e-06) at large x spread [4099, 288] + res
    worst of the 51 profile pairs at [4099, 288], dbeta : 2.5e-08 (torch fp32 2.1e-08, bound 1.8e-06) at unit x spread [4099, 288] + res
"""
import pytest
import torch
import torch.nn.functional as F

from tests import util_layernorm_train as Y
from tests import util_norm_attn_numerics as NA

pytestmark = pytest.mark.gpu

CANARY = -4321.5
GUARD = 3


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
    prev = fused._layernorm_train
    fused._layernorm_train = None
    fused.layernorm_train_counts(reset=True)
    try:
        yield
    finally:
        fused._layernorm_train = prev


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _guarded(rows, cols, dev, fill=CANARY):
    """[rows + GUARD, cols] of canaries: the first `rows` rows are the output, the rest must stay as they are."""
    return torch.full((rows + GUARD, cols), fill, dtype=torch.float32, device=dev)


def k_forward(x, res, gamma, beta, eps=Y.EPS):
    from trackformer_amd import _cabi
    rows, C = x.shape
    out, stats = _guarded(rows, C, x.device), _guarded(rows, 2, x.device)
    rc = _cabi.lib().tf_add_layernorm_train_f32(x.data_ptr(), _ptr(res), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), stats.data_ptr(),
                                                rows, C, eps, _stream(x.device))
    _cabi.check(rc, "tf_add_layernorm_train_f32")
    assert bool((out[rows:] == CANARY).all()) and bool((stats[rows:] == CANARY).all()), "the forward wrote behind out / stats"
    return out[:rows], stats[:rows]


class Bwd:
    """The buffers of one tf_add_layernorm_bwd_f32 call (canaries in GUARD rows behind dz, dgamma, dbeta and the workspace)."""

    def __init__(self, rows, C, dev):
        from trackformer_amd import _cabi
        self.rows, self.C = rows, C
        self.nbytes = int(_cabi.lib().tf_add_layernorm_bwd_workspace_bytes(rows, C))
        assert self.nbytes > 0 and self.nbytes % (8 * C) == 0
        self.nb = self.nbytes // (8 * C)
        self.dz = _guarded(rows, C, dev)
        self.dg, self.db = _guarded(1, C, dev), _guarded(1, C, dev)
        self.ws = _guarded(self.nb, 2 * C, dev)

    def __call__(self, dy, x, res, gamma, stats):
        from trackformer_amd import _cabi
        rc = _cabi.lib().tf_add_layernorm_bwd_f32(dy.data_ptr(), x.data_ptr(), _ptr(res), gamma.data_ptr(), stats.data_ptr(), self.dz.data_ptr(),
                                                  self.dg.data_ptr(), self.db.data_ptr(), self.ws.data_ptr(), self.nbytes, self.rows, self.C,
                                                  _stream(dy.device))
        _cabi.check(rc, "tf_add_layernorm_bwd_f32")
        return self

    def outputs(self):
        return {"dz": self.dz[:self.rows], "dgamma": self.dg[0], "dbeta": self.db[0]}

    def assert_canaries(self):
        for name, t, n in (("dz", self.dz, self.rows), ("dgamma", self.dg, 1), ("dbeta", self.db, 1), ("workspace", self.ws, self.nb)):
            assert bool((t[n:] == CANARY).all()), "tf_add_layernorm_bwd_f32 wrote behind " + name


def run_case(dev, profile, dy_profile, rows, C, with_res):
    x, res, gamma, beta, dy = Y.operands(profile, dy_profile, rows, C, rows + C, device=dev, with_res=with_res)
    _, stats = k_forward(x, res, gamma, beta)
    b = Bwd(rows, C, dev)(dy, x, res, gamma, stats)
    torch.cuda.synchronize(dev)
    b.assert_canaries()
    what = "%s x %s [%d, %d]%s" % (profile, dy_profile, rows, C, " + res" if res is not None else "")
    return Y.check(b.outputs(), Y.reference(x, res, gamma, dy), Y.fp32_formulation(x, res, gamma, beta, dy), rows, what)


# (32768, 256) | (32769, 256): the last row count with 16 rows per block and the first with 2048 blocks of more; (3, 516): MAXCH 4, one lane
# in the third chunk and none in the fourth
@pytest.mark.parametrize("rows,C", [(1, 4), (5, 260), (257, 288), (4099, 256), (4099, 288), (64, 4096), (32768, 256), (32769, 256), (3, 516)])
def test_kernels_against_float64(dev, rows, C):
    from trackformer_amd import _cabi
    run_case(dev, "unit", "unit", rows, C, with_res=True)
    assert _cabi.lib().tf_msda_last_kernel() == b"add_layernorm_bwd_reduce_f32"
    if (rows, C) == (32768, 256):
        assert Bwd(rows, C, dev).nb == 2048 and Bwd(rows + 1, C, dev).nb == 1928


@pytest.mark.parametrize("profile", NA.LN_PROFILES)
def test_every_profile_pair_against_float64(dev, profile):
    for i, dy_profile in enumerate(Y.DY_PROFILES):
        run_case(dev, profile, dy_profile, 4099, 288, None if i % 2 == 0 else True)


def test_forward_is_the_inference_kernel_bit_for_bit(dev):
    from trackformer_amd import fused
    for rows, C, with_res in ((4099, 256, True), (257, 288, False), (64, 4096, True)):
        x, res, gamma, beta, _ = Y.operands("unit", "unit", rows, C, 3, device=dev, with_res=with_res)
        out, stats = k_forward(x, res, gamma, beta)
        norm = torch.nn.LayerNorm(C, eps=Y.EPS).to(dev)
        with torch.no_grad():
            norm.weight.copy_(gamma)
            norm.bias.copy_(beta)
            want = fused.add_layernorm(x, res, norm)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
        z = (x if res is None else x + res).double()
        mean, rstd = z.mean(1), 1.0 / (z.var(1, unbiased=False) + Y.EPS).sqrt()
        assert float(((stats[:, 1].double() - rstd).abs() / rstd).max()) <= 2.0 ** -20
        assert float(((stats[:, 0].double() - mean).abs() * rstd).max()) <= 2.0 ** -20      # an error in mean, in units of the row's spread


def test_bit_identity_across_calls_streams_graph_and_a_busy_neighbour(dev):
    rows, C = 4099, 288
    x, res, gamma, beta, dy = Y.operands("unit", "row_spread", rows, C, 11, device=dev, with_res=True)
    _, stats = k_forward(x, res, gamma, beta)
    first = {k: v.clone() for k, v in Bwd(rows, C, dev)(dy, x, res, gamma, stats).outputs().items()}

    def same(b, what):
        torch.cuda.synchronize(dev)
        b.assert_canaries()
        for k, v in b.outputs().items():
            assert torch.equal(v.view(torch.int32), first[k].view(torch.int32)), (what, k)

    same(Bwd(rows, C, dev)(dy, x, res, gamma, stats), "second call")
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        b = Bwd(rows, C, dev)(dy, x, res, gamma, stats)
    torch.cuda.current_stream(dev).wait_stream(side)
    same(b, "side stream")
    # a captured graph that holds the backward alone: one chain of two kernels
    b = Bwd(rows, C, dev)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(graph):
        b(dy, x, res, gamma, stats)
    for _ in range(2):
        b.dz[:rows].zero_()
        b.dg[:1].zero_()
        b.db[:1].zero_()
        graph.replay()
        same(b, "graph replay")
    # while another stream runs an unrelated GEMM
    a = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        for _ in range(4):
            a = (a @ a) * 1e-3
    b = Bwd(rows, C, dev)(dy, x, res, gamma, stats)
    torch.cuda.current_stream(dev).wait_stream(side)
    same(b, "next to a GEMM")


def _module(C, dev, gamma, beta):
    norm = torch.nn.LayerNorm(C, eps=Y.EPS).to(dev)
    with torch.no_grad():
        norm.weight.copy_(gamma)
        norm.bias.copy_(beta)
    return norm


def _autograd_reference(x, res_term, gamma, beta, dy):
    """float64 autograd through F.layer_norm(x + res_term(x)) -> (y, dx, dres or None, dgamma, dbeta)."""
    xd = x.double().detach().requires_grad_(True)
    gd, bd = gamma.double().detach().requires_grad_(True), beta.double().detach().requires_grad_(True)
    rd = res_term(xd)
    y = F.layer_norm(xd + rd, (x.shape[-1],), gd, bd, Y.EPS)
    y.backward(dy.double())
    return y.detach(), xd.grad, (rd.grad if rd.is_leaf and rd.requires_grad else None), gd.grad, bd.grad


@pytest.mark.parametrize("case", ["res_requires_grad", "res_constant", "frozen_affine", "noncontiguous_grad_output", "x_is_res",
                                  "noncontiguous_res"])
def test_autograd_through_layernorm_train(dev, case):
    from trackformer_amd import fused
    rows, C = 300, 288
    x0, res0, gamma, beta, dy = Y.operands("unit", "unit", rows, C, 23, device=dev, with_res=True)
    x0, res0, dy = x0.reshape(2, rows // 2, C), res0.reshape(2, rows // 2, C), dy.reshape(2, rows // 2, C)
    norm = _module(C, dev, gamma, beta)
    if case == "frozen_affine":
        norm.weight.requires_grad_(False)
        norm.bias.requires_grad_(False)
    x = x0.clone().requires_grad_(True)
    res = x if case == "x_is_res" else res0.clone().requires_grad_(case != "res_constant")
    if case == "noncontiguous_res":       # [Lq, N, C] transposed, as nn.MultiheadAttention hands the decoder its output: copied, still differentiated
        res = res0.transpose(0, 1).contiguous().requires_grad_(True)
        y = fused.layernorm_train(x, res.transpose(0, 1), norm)
    else:
        y = fused.layernorm_train(x, res, norm)
    assert y is not None and type(y.grad_fn).__name__ == "_LayerNormTrainBackward"
    assert fused.layernorm_train_counts() == {"own": 1, "torch": 0}
    if case == "noncontiguous_grad_output":
        wide = torch.zeros(2, rows // 2, 2 * C, device=dev)
        wide[..., ::2] = dy
        g_out = wide[..., ::2]
        assert not g_out.is_contiguous()
    else:
        g_out = dy
    y.backward(g_out)
    torch.cuda.synchronize(dev)
    # against float64: the yardstick of the operator with dz doubled where x is used twice
    x2, r2, dy2 = x0.reshape(rows, C), (x0 if case == "x_is_res" else res0).reshape(rows, C), dy.reshape(rows, C)
    ref = Y.reference(x2, r2, gamma, dy2)
    fp32 = Y.fp32_formulation(x2, r2, gamma, beta, dy2)
    k = 2.0 if case == "x_is_res" else 1.0
    ref["dz"] = NA.Ref(k * ref["dz"].ref, k * ref["dz"].scale, ref["dz"].floor)
    fp32["dz"] = k * fp32["dz"]
    got = {"dz": x.grad.reshape(rows, C), "dgamma": norm.weight.grad, "dbeta": norm.bias.grad}
    if case == "frozen_affine":
        assert norm.weight.grad is None and norm.bias.grad is None
    Y.check(got, ref, fp32, rows, case)
    _, dxd, _, dgd, dbd = _autograd_reference(x0, (lambda xd: xd) if case == "x_is_res" else (lambda xd: res0.double().requires_grad_(True)),
                                             gamma, beta, dy)
    # (the yardstick's closed forms ARE float64 autograd through F.layer_norm(x + res))
    assert float((ref["dz"].ref.reshape(dxd.shape) - dxd).abs().max()) <= 1e-11 * float(dxd.abs().max())
    assert float((ref["dgamma"].ref - dgd).abs().max()) <= 1e-11 * float(dgd.abs().max())
    assert float((ref["dbeta"].ref - dbd).abs().max()) <= 1e-11 * float(dbd.abs().max())
    NA.check(y.reshape(rows, C), NA.norm_reference([x2, r2], gamma, beta, Y.EPS), None, case + " (forward)")
    if case == "res_constant":
        assert res.grad is None
    elif case == "noncontiguous_res":
        assert torch.equal(res.grad.transpose(0, 1), x.grad)
    elif case != "x_is_res":
        assert torch.equal(res.grad, x.grad)          # ONE tensor for both


def test_layernorm_train_declines_on_the_device(dev):
    from trackformer_amd import fused
    norm = torch.nn.LayerNorm(256).to(dev)
    x = torch.randn(6, 256, device=dev)
    assert fused.layernorm_train(x[:, ::2], None, torch.nn.LayerNorm(128).to(dev)) is None                # non-contiguous
    assert fused.layernorm_train(x, torch.randn(6, 128, device=dev), norm) is None                        # a res of another shape
    assert fused.layernorm_train(x, x.double(), norm) is None
    assert fused.layernorm_train(x.reshape(-1)[1:1 + 5 * 256].reshape(5, 256), None, norm) is None        # misaligned
    assert fused.layernorm_train(x, None, torch.nn.LayerNorm(256, elementwise_affine=False).to(dev)) is None
    assert fused.layernorm_train_counts() == {"own": 0, "torch": 5}
    # the route: off by default; on, residual_norm takes it under gradients only
    res = torch.randn(6, 256, device=dev)
    y0 = fused.residual_norm(x, res, norm, inference=False)
    assert type(y0.grad_fn).__name__ == "NativeLayerNormBackward0"
    prev = fused.set_layernorm_training(True)
    try:
        y1 = fused.residual_norm(x, res, norm, inference=False)
        with torch.no_grad():
            y2 = fused.residual_norm(x, res, norm, inference=False)
            want = fused.add_layernorm(x, res, norm)
    finally:
        fused.set_layernorm_training(prev)
    assert type(y1.grad_fn).__name__ == "_LayerNormTrainBackward" and y2.grad_fn is None
    assert torch.equal(y1.view(torch.int32), want.view(torch.int32))          # the deployed operator, bit for bit
    assert fused.layernorm_train_counts() == {"own": 1, "torch": 5}


def test_non_finite_contract(dev):
    rows, C = 37, 260
    x, res, gamma, beta, dy = Y.operands("unit", "unit", rows, C, 5, device=dev, with_res=True)
    _, stats = k_forward(x, res, gamma, beta)
    clean = {k: v.clone() for k, v in Bwd(rows, C, dev)(dy, x, res, gamma, stats).outputs().items()}
    assert all(bool(torch.isfinite(v).all()) for v in clean.values())
    others = torch.arange(rows, device=dev) != 6
    planted = torch.arange(C, device=dev) == 257
    for bad in (float("nan"), float("inf")):
        d2 = dy.clone()
        d2[6, 257] = bad
        b = Bwd(rows, C, dev)(d2, x, res, gamma, stats)
        got = b.outputs()
        b.assert_canaries()
        assert torch.equal(got["dz"][others], clean["dz"][others]) and not bool(torch.isfinite(got["dz"][6]).any())
        for name in ("dgamma", "dbeta"):
            assert not bool(torch.isfinite(got[name][planted]).any()), name
            assert torch.equal(got[name][~planted], clean[name][~planted]), name
        for which in ("x", "res"):
            x2, r2 = x.clone(), res.clone()
            (x2 if which == "x" else r2)[6, 3] = bad
            _, st2 = k_forward(x2, r2, gamma, beta)
            assert torch.equal(st2[others], stats[others]) and not bool(torch.isfinite(st2[6]).any())
            got = Bwd(rows, C, dev)(dy, x2, r2, gamma, st2).outputs()
            assert torch.equal(got["dz"][others], clean["dz"][others]) and bool(torch.isnan(got["dz"][6]).all()), which
            # the row's mean is lost and with it every xh[6, c]: every dgamma[c] is NaN in exact arithmetic too; dbeta does not read x
            assert bool(torch.isnan(got["dgamma"]).all()) and torch.equal(got["dbeta"], clean["dbeta"]), which
