"""GPU (-m gpu): tf_groupnorm_levels_nhwc_f32 / tf_conv_packed_partials_f32 and the route built on them (fused.input_proj_levels,
DeformableTransformer.encode taking the token buffer) on the device.

  * the cases of tests/test_groupnorm_levels_emu.py: float64 yardstick of tf_groupnorm_nhwc_f32, BITWISE equality with the numpy
    restatement of the summation order, guard rows, two calls equal
  * the deferred-reduce convolution at the two coarse cfg-2 shapes: piece count, partial sums in order + bias == the existing entry
  * the small cfg-2 model, threshold lowered to 1, route on against route off
  * HIP graph capture and replay on two images; weight updates between calls"""
import numpy as np
import pytest
import torch

from tests import util_groupnorm_levels as GL
from tests import util_models as um
from tests import util_norm_attn_numerics as A

pytestmark = pytest.mark.gpu

EPS = 1e-5
CG = [(256, 32), (288, 32)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from trackformer_amd import _cabi
    _cabi.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def backend(dev):
    from trackformer_amd import _cabi
    return GL.device_backend(_cabi.lib(), dev)


def _check_level(got, lv, G, what):
    y = torch.from_numpy(lv["y"])
    gamma, beta = torch.from_numpy(lv["gamma"]), torch.from_numpy(lv["beta"])
    r = A.norm_reference([y], gamma, beta, EPS, G)
    A.check(torch.from_numpy(got), r, A.norm_fp32([y], gamma, beta, EPS, G), what)
    want = GL.restate(lv["y"], lv["gamma"], lv["beta"], G, EPS, lv["pieces"])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s: differs from the restated arithmetic" % what


@pytest.mark.parametrize("C,G", CG, ids=["c256", "c288"])
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("pieces", [1, 3, 5])
@pytest.mark.parametrize("HW", [1, 63, 64, 65, 130])
def test_one_level(backend, HW, pieces, N, C, G):
    profile = A.NORM_PROFILES[(HW + pieces + N) % len(A.NORM_PROFILES)]
    lv = GL.make_level(profile, N, HW, C, G, pieces, seed=HW * 7 + pieces)
    rc, got, untouched, _ = GL.run_levels(backend, [lv], N, C, G, EPS)
    assert rc == 0
    _check_level(got[0], lv, G, "gpu gn_levels %s HW %d pieces %d N %d C %d" % (profile, HW, pieces, N, C))
    assert untouched, "guard rows, the output's padding or the workspace behind its stated size were written (or a slot was not)"


@pytest.mark.parametrize("profile", ["offset3000", "offset300", "large", "chan_spread", "constant", "small_1e-6"])
@pytest.mark.parametrize("pieces", [1, 3])
def test_profiles_with_large_means(backend, profile, pieces):
    N, HW, C, G = 2, 130, 256, 32
    lv = GL.make_level(profile, N, HW, C, G, pieces, seed=11 + pieces)
    rc, got, untouched, _ = GL.run_levels(backend, [lv], N, C, G, EPS)
    assert rc == 0 and untouched
    _check_level(got[0], lv, G, "gpu gn_levels %s pieces %d" % (profile, pieces))


@pytest.mark.parametrize("C,G", CG, ids=["c256", "c288"])
@pytest.mark.parametrize("N", [1, 2])
def test_mixed_levels_in_one_call(backend, N, C, G):
    spec = [(65, 1, "unit"), (1, 5, "offset30"), (130, 3, "offset3000"), (63, 1, "chan_spread"), (64, 5, "large")]
    levels = [GL.make_level(p, N, hw, C, G, pc, seed=100 + i, with_bias=(i != 1)) for i, (hw, pc, p) in enumerate(spec)]
    order = [3, 0, 4, 2, 1]
    rc, got, untouched, _ = GL.run_levels(backend, levels, N, C, G, EPS, order=order)
    assert rc == 0 and untouched
    for i, (lv, g) in enumerate(zip(levels, got)):
        _check_level(g, lv, G, "gpu gn_levels mixed level %d %s N %d C %d" % (i, spec[i], N, C))
    rc2, got2, _, _ = GL.run_levels(backend, levels, N, C, G, EPS, order=order)
    assert rc2 == 0
    for a, b in zip(got, got2):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "two calls on the same inputs differ"


def test_more_slots_than_one_chain_adds_at_once(backend):
    """HW = 2200 at C = 256: 35 statistics blocks, so every one of the 8 chains of the normalising pass takes its four-at-a-time
    loop and a remainder."""
    N, HW, C, G = 1, 2200, 256, 32
    lv = GL.make_level("offset300", N, HW, C, G, 1, seed=5)
    rc, got, untouched, _ = GL.run_levels(backend, [lv], N, C, G, EPS)
    assert rc == 0 and untouched
    _check_level(got[0], lv, G, "gpu gn_levels 35 slots")


@pytest.mark.parametrize("ks,stride,pixels", [(3, 2, 273), (1, 1, 1050)], ids=["273px-3x3s2", "1050px-1x1"])
def test_deferred_reduce_convolution_at_the_coarse_cfg2_shapes(dev, ks, stride, pixels):
    """25 x 42 x 2048 -> 256: the partial sums of tf_conv_packed_partials_f32, added in order plus the bias, are the existing entry's
    output bit for bit; the piece count is what the launch code makes of the policy's ksplit (64 -> 58 pieces of 10 slices; 8 -> 8)."""
    from trackformer_amd import fused
    g = torch.Generator().manual_seed(ks)
    cin, cout = 2048, 256
    x = torch.randn(1, cin, 25, 42, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(cout, ks * ks * cin, generator=g) / (ks * ks * cin) ** 0.5).to(dev)
    bias = (0.1 * torch.randn(cout, generator=g)).to(dev)
    with torch.no_grad():
        y = fused.conv3x3(x, w, bias, False, stride)
        part = fused._conv_partials(x, w, bias, stride)
    assert y is not None and part is not None
    ws, pieces = part
    assert y.shape[2] * y.shape[3] == pixels
    ksplit = fused._conv_ksplit(pixels, ks * ks * cin, cout)
    assert ksplit == (64 if ks == 3 else 8) and pieces == GL.launch_pieces(ks * ks * cin, ksplit) == (58 if ks == 3 else 8)
    acc = ws[0].clone()
    for z in range(1, pieces):
        acc += ws[z]
    acc = acc.view(pixels, cout) + bias
    assert torch.equal(acc.view(torch.int32), y.permute(0, 2, 3, 1).reshape(pixels, cout).view(torch.int32))


def _projs(dev, hidden=256, groups=32, seed=0):
    """Three input projections over two feature maps: a finished y (K = 512: not split), a split 1 x 1 and the split 3 x 3 / stride 2."""
    torch.manual_seed(seed)
    mk = lambda cin, **kw: torch.nn.Sequential(torch.nn.Conv2d(cin, hidden, **kw), torch.nn.GroupNorm(groups, hidden))   # noqa: E731
    projs = torch.nn.ModuleList([mk(512, kernel_size=1), mk(2048, kernel_size=1), mk(2048, kernel_size=3, stride=2, padding=1)]).to(dev).eval()
    with torch.no_grad():
        for p in projs:
            p[1].weight.normal_(1, 0.2)
            p[1].bias.normal_(0, 0.2)
    return projs


def _images(dev, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(1, 512, 26, 22, generator=g).to(dev).contiguous(memory_format=torch.channels_last),
            torch.randn(1, 2048, 13, 11, generator=g).to(dev).contiguous(memory_format=torch.channels_last)]


def _items(projs, feats):
    return [(feats[0], projs[0][0], projs[0][1]), (feats[1], projs[1][0], projs[1][1]), (feats[1], projs[2][0], projs[2][1])]


@pytest.fixture()
def low_threshold():
    from trackformer_amd import fused
    prev = fused.set_input_proj_levels_min_rows(1)
    prev_on = fused.set_input_proj_levels(True)
    yield
    fused.set_input_proj_levels(prev_on)
    fused.set_input_proj_levels_min_rows(prev)


def test_levels_route_against_the_per_level_route(dev, low_threshold):
    from trackformer_amd import fused
    projs, feats = _projs(dev), _images(dev, 1)
    with torch.no_grad():
        got = fused.input_proj_levels(_items(projs, feats))
        want = [fused.input_proj_1x1(x, conv, gn) for x, conv, gn in _items(projs, feats)]
    assert got is not None and all(w is not None for w in want)
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.allclose(a, b, atol=1e-5, rtol=1e-5)


def test_graph_capture_and_replay_on_two_images(dev, low_threshold):
    """Captured in a HIP graph and replayed on two different images: each replay equals the eager result of its image BITWISE."""
    from trackformer_amd import fused
    projs = _projs(dev)
    imgs = [_images(dev, 2), _images(dev, 3)]
    static = [t.clone() for t in imgs[0]]
    with torch.no_grad():
        eager = [torch.cat([s.flatten(2) for s in fused.input_proj_levels(_items(projs, im))], 2).clone() for im in imgs]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fused.input_proj_levels(_items(projs, static))   # warm-up on the capturing stream
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fused.input_proj_levels(_items(projs, static))
        assert out is not None
        for k in (0, 1, 0):
            for s, t in zip(static, imgs[k]):
                s.copy_(t)
            graph.replay()
            torch.cuda.synchronize()
            replayed = torch.cat([s.flatten(2) for s in out], 2)
            assert torch.equal(replayed.view(torch.int32), eager[k].view(torch.int32)), "replay of image %d differs from eager" % k


def test_weight_updates_between_calls_are_seen(dev, low_threshold):
    """gn.weight / conv.weight updated in place and by rebinding between two calls (the pattern of tests/test_weight_coherence_gpu.py):
    the next call computes with the new values -- compared with the per-level route on the same modules."""
    from trackformer_amd import fused
    projs, feats = _projs(dev), _images(dev, 4)

    def both():
        with torch.no_grad():
            got = fused.input_proj_levels(_items(projs, feats))
            want = [fused.input_proj_1x1(x, conv, gn) for x, conv, gn in _items(projs, feats)]
        assert got is not None
        for a, b in zip(got, want):
            assert torch.allclose(a, b, atol=1e-5, rtol=1e-5)
        return [g.clone() for g in got]

    def differs(a, b, levels):
        return [not torch.allclose(x, y, atol=1e-3) for x, y in zip(a, b)] == levels

    r0 = both()
    with torch.no_grad():
        projs[0][1].weight.mul_(1.5)                                             # gn.weight in place
    r1 = both()
    assert differs(r0, r1, [True, False, False])
    with torch.no_grad():
        projs[1][0].weight.add_(0.01 * torch.randn_like(projs[1][0].weight))     # a split 1 x 1 conv.weight in place
        projs[2][0].weight.mul_(0.5).add_(0.01 * torch.randn_like(projs[2][0].weight))   # the 3 x 3 one
    r2 = both()
    assert differs(r1, r2, [False, True, True])
    projs[1][1].weight = torch.nn.Parameter(projs[1][1].weight.detach() * -1.0)  # rebinding
    projs[0][0].weight = torch.nn.Parameter(projs[0][0].weight.detach().flip(0).contiguous())
    projs[2][0].weight = torch.nn.Parameter(projs[2][0].weight.detach().flip(0).contiguous())
    r3 = both()
    assert differs(r2, r3, [True, True, True])


def test_small_cfg2_model_route_on_against_route_off(dev, low_threshold, monkeypatch):
    """The small cfg-2 test model with the threshold at 1: what encode() receives is within the float64 bound of GroupNorm on both routes
    (from the very y the per-level route normalised), the model outputs within the tolerances tests/test_models_gpu.py uses when it
    compares routes, and encode() took the buffer: no concatenation of the levels."""
    from trackformer_amd import config, factory, fused
    model, _post, _args = um.build("cfg2_deformable_tracking", factory.build_model, config.make_args, device=dev)
    model.to(dev).tracking()
    img, _prev, target = um.model_inputs("cfg2_deformable_tracking", model.hidden_dim)
    img = img.to(dev)
    seen = {}
    real_encode = model.transformer.encode
    real_cat = torch.cat

    def encode(srcs, masks, pos):
        seen["srcs"] = [s.clone() for s in srcs]
        ptrs = {s.data_ptr() for s in srcs}
        cats = []

        def cat(tensors, *a, **kw):
            if any(t.data_ptr() in ptrs for t in tensors):
                cats.append(len(tensors))
            return real_cat(tensors, *a, **kw)
        monkeypatch.setattr(torch, "cat", cat)
        try:
            return real_encode(srcs, masks, pos)
        finally:
            monkeypatch.setattr(torch, "cat", real_cat)
            seen["cats"] = cats
    monkeypatch.setattr(model.transformer, "encode", encode)

    ys = []
    real_gn = fused.groupnorm_nhwc

    def gn_spy(x2, n_img, gn, relu=False):
        ys.append((x2.clone(), n_img, gn))
        return real_gn(x2, n_img, gn, relu)

    with torch.no_grad():
        prev = fused.set_input_proj_levels(False)
        monkeypatch.setattr(fused, "groupnorm_nhwc", gn_spy)
        try:
            out_off, *_ = model(img, um.to_device(target, dev))
        finally:
            monkeypatch.setattr(fused, "groupnorm_nhwc", real_gn)
            fused.set_input_proj_levels(prev)
        srcs_off, cats_off = seen["srcs"], seen["cats"]
        out_on, *_ = model(img, um.to_device(target, dev))
        srcs_on, cats_on = seen["srcs"], seen["cats"]
    assert len(ys) == 4 and len(srcs_on) == len(srcs_off) == 4
    assert cats_off == [4] and cats_on == [], (cats_off, cats_on)
    for lvl, ((y2, n_img, gn), s_off, s_on) in enumerate(zip(ys, srcs_off, srcs_on)):
        y = y2.view(n_img, -1, y2.shape[1])
        r = A.norm_reference([y], gn.weight, gn.bias, float(gn.eps), gn.num_groups)
        f32 = A.norm_fp32([y], gn.weight, gn.bias, float(gn.eps), gn.num_groups)
        A.check(s_off.flatten(2).transpose(1, 2), r, f32, "cfg2 small, level %d, per-level route" % lvl)
        A.check(s_on.flatten(2).transpose(1, 2), r, f32, "cfg2 small, level %d, all-levels route" % lvl)
    assert torch.allclose(out_on["pred_boxes"], out_off["pred_boxes"], atol=1e-5)
    assert torch.allclose(out_on["pred_logits"], out_off["pred_logits"], atol=1e-4)
