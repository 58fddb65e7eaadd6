"""CPU: the host-side mapping of the all-levels input-projection route (trackformer_amd/fused.py input_proj_levels,
DeformableDETR._input_proj_all_levels, deformable_transformer._token_buffer_of) with torch stand-ins for the native entries, against
the nn.Sequential(Conv2d, GroupNorm) levels it replaces: row offsets, the views handed back per level, None (and the per-level route)
when a level declines, merge_frame_features models and small inputs never taking the route."""
import types

import pytest
import torch
import torch.nn.functional as F

from trackformer_amd import deformable_transformer, fused
from trackformer_amd.deformable_detr import DeformableDETR

HIDDEN, GROUPS = 32, 8


def _levels(cins=(64, 128, 192)):
    """The reference's input projections: 1 x 1 levels and the extra 3 x 3 / stride 2 one (deformable_detr.py:73-90)."""
    torch.manual_seed(0)
    projs = [torch.nn.Sequential(torch.nn.Conv2d(c, HIDDEN, 1), torch.nn.GroupNorm(GROUPS, HIDDEN)) for c in cins]
    projs.append(torch.nn.Sequential(torch.nn.Conv2d(cins[-1], HIDDEN, 3, stride=2, padding=1), torch.nn.GroupNorm(GROUPS, HIDDEN)))
    with torch.no_grad():
        for p in projs:
            p[1].weight.normal_(1, 0.2)
            p[1].bias.normal_(0, 0.2)
    return torch.nn.ModuleList(projs).eval()


def _features(n=2, sizes=((12, 10), (6, 5), (3, 3)), cins=(64, 128, 192)):
    g = torch.Generator().manual_seed(1)
    return [torch.randn(n, c, h, w, generator=g).contiguous(memory_format=torch.channels_last) for c, (h, w) in zip(cins, sizes)]


class _Calls:
    def __init__(self):
        self.partials, self.conv3x3, self.linear, self.levels = [], [], [], []


def _stand_ins(monkeypatch, calls, split=(1, 3), decline=None):
    """torch stand-ins: the levels `split` leave two partial sums, the others a finished y; `decline`: that level's GEMMs return None."""
    counter = {"level": -1}

    def conv(x, w, bias, stride):
        n, cin, h, wd = x.shape
        cout = w.shape[0]
        ks = 3 if w.shape[1] == 9 * cin else 1
        w4 = w.view(cout, ks, ks, cin).permute(0, 3, 1, 2)
        return F.conv2d(x, w4, None, stride=stride, padding=1 if ks == 3 else 0).permute(0, 2, 3, 1).contiguous()   # NHWC, no bias

    def partials(x, w, bias, stride):
        counter["level"] += 1
        lvl = counter["level"]
        calls.partials.append(lvl)
        if lvl == decline or lvl not in split:
            return None
        y = conv(x, w, bias, stride).reshape(-1)
        return torch.stack([0.25 * y, 0.75 * y]), 2

    def conv3x3(x, w, bias, relu, stride):
        calls.conv3x3.append(counter["level"])
        if counter["level"] == decline:
            return None
        return (conv(x, w, bias, stride) + bias).permute(0, 3, 1, 2)

    def wants(m, cin, cout):
        return True

    def linear(x2, w, bias=None, relu=False, rows=None, residual=None):
        calls.linear.append(counter["level"])
        if counter["level"] == decline:
            return None
        return x2 @ w.t() + bias

    def gn_levels(levels, n, total, c, groups, eps, device):
        calls.levels.append([(pieces, hw) for _s, pieces, _b, _g, hw in levels])
        out = torch.full((n, total, c), float("nan"))
        row0 = 0
        for src, pieces, bias, gn, hw in levels:
            y = src.reshape(n, hw, c) if pieces == 1 else src[:pieces].sum(0).reshape(n, hw, c) + bias
            assert (bias is None) == (pieces == 1)
            out[:, row0:row0 + hw] = F.group_norm(y.transpose(1, 2), groups, gn.weight, gn.bias, eps).transpose(1, 2)
            row0 += hw
        assert row0 == total
        return out

    monkeypatch.setattr(fused, "_conv_partials", partials)
    monkeypatch.setattr(fused, "conv3x3", conv3x3)
    monkeypatch.setattr(fused, "conv1x1_wants_split_k", wants)
    monkeypatch.setattr(fused, "linear", linear)
    monkeypatch.setattr(fused, "_groupnorm_levels", gn_levels)
    monkeypatch.setattr(fused, "_input_proj_fused", True)
    monkeypatch.setattr(fused, "_input_proj_levels", True)
    monkeypatch.setattr(fused, "_split_linear", True)
    monkeypatch.setattr(fused, "_INPUT_PROJ_LEVELS_MIN_ROWS", 1)
    # the route is for GPU tensors; exercise the mapping on the host by lifting the device check
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))


def _items(projs, feats):
    return [(x, projs[i][0], projs[i][1]) for i, x in enumerate(feats + [feats[-1]])]


def test_levels_mapping_matches_the_sequentials_and_encode_takes_the_buffer(monkeypatch):
    projs, feats = _levels(), _features()
    with torch.no_grad():
        ref = [projs[i](x) for i, x in enumerate(feats + [feats[-1]])]
    calls = _Calls()
    _stand_ins(monkeypatch, calls)
    with torch.no_grad():
        got = fused.input_proj_levels(_items(projs, feats))
    assert got is not None and len(got) == 4
    hws = [120, 30, 9, 4]
    assert calls.levels == [[(1, 120), (2, 30), (1, 9), (2, 4)]]     # pieces and rows per level, one call for all of them
    total, row0 = sum(hws), 0
    for g, r, hw in zip(got, ref, hws):
        assert g.shape == r.shape and torch.allclose(g, r, atol=2e-5)
        h, w = g.shape[-2:]
        assert g.stride() == (total * HIDDEN, 1, w * HIDDEN, HIDDEN)                 # channels_last strides inside the token buffer
        assert g.storage_offset() == row0 * HIDDEN and g.untyped_storage().data_ptr() == got[0].untyped_storage().data_ptr()
        row0 += hw
    buf = deformable_transformer._token_buffer_of(got)
    assert buf is not None and buf.shape == (2, total, HIDDEN) and buf.is_contiguous()
    assert buf.data_ptr() == got[0].data_ptr()
    assert torch.equal(buf, torch.cat([s.flatten(2).transpose(1, 2) for s in got], 1))
    # the weight images are the per-level route's, cached on the modules
    assert projs[0][0]._tf_w2d[1].shape == (HIDDEN, 64) and projs[3][0]._tf_wtaps[1].shape == (HIDDEN, 9 * 192)


def test_token_buffer_is_recognised_by_storage_offsets_and_strides_only():
    n, c = 2, 8
    buf = torch.randn(n, 20, c)
    def views(b, sizes=((3, 4), (2, 3), (1, 2))):   # noqa: E306
        out, r = [], 0
        for h, w in sizes:
            out.append(b[:, r:r + h * w].view(n, h, w, c).permute(0, 3, 1, 2))
            r += h * w
        return out
    v = views(buf)
    got = deformable_transformer._token_buffer_of(v)
    assert got is not None and got.data_ptr() == buf.data_ptr() and torch.equal(got, buf)
    tok = deformable_transformer._token_buffer_of
    assert tok([v[0], v[2], v[1]]) is None                                        # not consecutive
    assert tok([v[0], v[1].clone(), v[2]]) is None                                # another storage
    assert tok([v[0].contiguous(), v[1], v[2]]) is None                           # NCHW strides
    assert tok(v[:2]) is None                                                     # image stride of a longer buffer (n > 1)
    assert tok(views(torch.randn(n, 25, c))) is None                              # rows behind the levels: not the whole buffer
    assert tok([t.double() if i == 1 else t for i, t in enumerate(v)]) is None
    ordinary = [torch.randn(n, c, h, w) for h, w in ((3, 4), (2, 3))]
    assert tok(ordinary) is None


@pytest.mark.parametrize("decline", [0, 1, 3])
def test_a_declining_level_returns_none(monkeypatch, decline):
    projs, feats = _levels(), _features()
    calls = _Calls()
    _stand_ins(monkeypatch, calls, decline=decline)
    with torch.no_grad():
        assert fused.input_proj_levels(_items(projs, feats)) is None
    assert calls.levels == []


def test_route_conditions(monkeypatch):
    projs, feats = _levels(), _features()
    calls = _Calls()
    _stand_ins(monkeypatch, calls)
    items = _items(projs, feats)
    assert fused.input_proj_levels(items) is None                                 # gradients enabled
    with torch.no_grad():
        monkeypatch.setattr(fused, "_INPUT_PROJ_LEVELS_MIN_ROWS", 2 * 163 + 1)
        assert fused.input_proj_levels(items) is None                             # one row below the threshold
        monkeypatch.setattr(fused, "_INPUT_PROJ_LEVELS_MIN_ROWS", 2 * 163)
        assert fused.input_proj_levels(items) is not None
        monkeypatch.setattr(fused, "_input_proj_levels", False)
        assert fused.input_proj_levels(items) is None
        monkeypatch.setattr(fused, "_input_proj_levels", True)
        monkeypatch.setattr(fused, "_input_proj_fused", False)
        assert fused.input_proj_levels(items) is None
        monkeypatch.setattr(fused, "_input_proj_fused", True)
        other = torch.nn.Sequential(torch.nn.Conv2d(64, HIDDEN, 3, padding=1), torch.nn.GroupNorm(GROUPS, HIDDEN))
        assert fused.input_proj_levels([(feats[0], other[0], other[1])] + items[1:]) is None      # a convolution of another kind
        gn16 = torch.nn.GroupNorm(16, HIDDEN)
        assert fused.input_proj_levels([(feats[0], projs[0][0], gn16)] + items[1:]) is None       # levels must share the groups
        assert fused.input_proj_levels(items * 3) is None                                        # more than 8 levels
        # per-layer six-term routes, the range audit and the finite check live on the per-layer wrappers: the route steps aside
        monkeypatch.setattr(fused, "_n_six_term_routes", 1)
        assert fused.input_proj_levels(items) is None
        monkeypatch.setattr(fused, "_n_six_term_routes", 0)
        monkeypatch.setattr(fused, "_check_finite", True)
        assert fused.input_proj_levels(items) is None
        monkeypatch.setattr(fused, "_check_finite", False)
        assert fused.input_proj_levels(items) is not None
    assert fused.set_input_proj_levels_min_rows(7) == 2 * 163 and fused.set_input_proj_levels_min_rows(4096) == 7
    assert fused.set_input_proj_levels(False) is True and fused.set_input_proj_levels(True) is False


def _model(projs, **kw):
    """What DeformableDETR._input_proj_all_levels / _input_proj read of the model."""
    m = types.SimpleNamespace(training=False, merge_frame_features=False, num_feature_levels=4, input_proj=projs)
    m.__dict__.update(kw)
    return m


def _frames(feats, n_frames=1):
    return [[types.SimpleNamespace(tensors=x) for x in feats] for _ in range(n_frames)]


def test_model_hook_takes_the_route_in_inference_only(monkeypatch):
    projs, feats = _levels(), _features()
    calls = _Calls()
    _stand_ins(monkeypatch, calls)
    hook = DeformableDETR._input_proj_all_levels
    with torch.no_grad():
        got = hook(_model(projs), _frames(feats))
        assert got is not None and len(got) == 4 and len(calls.levels) == 1
        two = hook(_model(projs), _frames(feats, 2))                               # multi-frame attention: both frames in one call
        assert two is not None and len(two) == 8 and len(calls.levels) == 2 and len(calls.levels[1]) == 8
        assert deformable_transformer._token_buffer_of(two) is not None
        assert hook(_model(projs, merge_frame_features=True), _frames(feats)) is None
        assert hook(_model(projs, training=True), _frames(feats)) is None
        assert hook(_model(projs, num_feature_levels=5), _frames(feats)) is None   # a second extra level reads the first one's output
        monkeypatch.setattr(fused, "_INPUT_PROJ_LEVELS_MIN_ROWS", 4096)
        assert hook(_model(projs), _frames(feats)) is None                         # 326 rows: the per-level route
    assert hook(_model(projs), _frames(feats)) is None                             # gradients enabled
    assert len(calls.levels) == 2


def test_below_the_threshold_the_per_level_route_runs(monkeypatch):
    """DeformableDETR._input_proj falls back to fused.input_proj_1x1 per level when the hook declines: same numbers."""
    projs, feats = _levels(), _features()
    calls = _Calls()
    _stand_ins(monkeypatch, calls)
    monkeypatch.setattr(fused, "_INPUT_PROJ_LEVELS_MIN_ROWS", 4096)
    taken = []

    def per_level(x, conv, gn):
        taken.append(conv)
        return gn(conv(x))
    monkeypatch.setattr(fused, "input_proj_1x1", per_level)
    m = _model(projs)
    with torch.no_grad():
        assert DeformableDETR._input_proj_all_levels(m, _frames(feats)) is None
        ys = [DeformableDETR._input_proj(m, lvl, x) for lvl, x in enumerate(feats + [feats[-1]])]
        ref = [projs[i](x) for i, x in enumerate(feats + [feats[-1]])]
    assert [c for c in taken] == [p[0] for p in projs] and calls.levels == []
    assert all(torch.equal(a, b) for a, b in zip(ys, ref))
