"""GPU: are the real kernels handed the CURRENT weights?  The matrix of tests/test_weight_coherence_cpu.py (c) on the device -- warm
module against its cold twin, bit for bit -- and what only exists there: the training path's input gradient after an optimiser step
(_packed_weight_t), a module moved to the device after its images were built on the host, and GraphedDetector, whose captured
graphs bake the ADDRESSES of the weight images."""
import pytest
import torch
from torch import nn

from tests import util_models as um, util_weight_coherence as wc
from trackformer_amd import backbone, config, factory, fused

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from trackformer_amd import _cabi
    _cabi.lib()
    return torch.device("cuda:0")


_MATRIX = wc.matrix()


@pytest.mark.parametrize("consumer,target,cls,mid,mutation", _MATRIX, ids=wc.matrix_ids(_MATRIX))
def test_warm_module_equals_its_cold_twin_after_a_weight_change(dev, consumer, target, cls, mid, mutation):
    wc.check(consumer, target, mutation, device=dev)


@pytest.mark.parametrize("consumer", [wc.LinearC, wc.LinearRowsC, wc.PackedLinearC, wc.FfnC, wc.BottleneckC], ids=lambda c: c.__name__)
def test_weight_change_reaches_the_six_term_product_too(dev, consumer):
    prev = fused.set_split_terms(6)
    try:
        wc.check(consumer, consumer.TARGETS[0], wc.mut_data_assign, device=dev)
        wc.check(consumer, consumer.TARGETS[0], wc.mut_data_write_then_tell, device=dev)
    finally:
        fused.set_split_terms(prev)


def test_images_built_on_the_host_follow_a_module_to_the_device(dev):
    """The cache functions only: images filled for host tensors, then module.to(device) (same version counters, new storage): what
    they return afterwards lives on the device and equals what never-used caches build there."""
    block = wc.randomize(wc.BottleneckC().block, seed=5)
    lin = wc.randomize(nn.Linear(32, 8, bias=False), seed=8)

    def images(fold, weight):
        with torch.no_grad():
            b = fold.get(block.conv2, block.bn2)
            return [b, fold.weight_taps] + [p for p in fused._split_weight(weight) if p is not None]
    host = [t.clone() for t in images(block._folds[1], lin.weight)]
    block.to(dev)
    lin.to(dev)
    got = images(block._folds[1], lin.weight)
    assert all(t.device.type == "cuda" and t.dtype == h.dtype for t, h in zip(got, host)), [(t.device, t.dtype) for t in got]
    assert wc.bits_equal(got, images(backbone._FoldCache(), lin.weight.detach().clone()))
    assert wc.bits_equal([t.cpu() for t in got[2:]], host[2:])   # (the pieces are exact arithmetic: the same bits on both sides)


@pytest.mark.parametrize("way", ["sgd_step", "data_assign", "data_write_then_weights_changed"])
def test_linear_train_input_gradient_comes_from_the_new_weight(dev, way):
    """fused.linear_train: the forward is the inference kernel on cached images, the input gradient runs on the packed image of the
    TRANSPOSED weight (_packed_weight_t) -- and the weight changes every step."""
    M, K, N = 515, 256, 128
    g = torch.Generator().manual_seed(41)
    x0, dy = torch.randn(M, K, generator=g).to(dev), torch.randn(M, N, generator=g).to(dev)
    lin = wc.randomize(nn.Linear(K, N), seed=9).to(dev).train()

    def step(layer):
        x = x0.clone().requires_grad_(True)
        fused.train_route_counts(reset=True)
        y = fused.linear_train(x, layer.weight, layer.bias)
        assert y is not None
        y.backward(dy)
        assert fused.train_route_counts()["dgrad_own"] == 1
        return [y.detach().clone(), x.grad.clone()]
    prev = fused.set_split_linear_training(True)
    keep = fused._split_linear_train
    try:
        before = step(lin)
        if way == "sgd_step":
            torch.optim.SGD(lin.parameters(), lr=0.05).step()      # the gradients of the step above
        elif way == "data_assign":
            wc.mut_data_assign(lin, "weight")
        else:
            wc.mut_data_write_then_tell(lin, "weight")
        lin.zero_grad()
        after = step(lin)
        twin = nn.Linear(K, N).to(dev).train()
        twin.load_state_dict({k: v.detach().clone() for k, v in lin.state_dict().items()})
        want = step(twin)
    finally:
        fused.set_split_linear_training(prev)
        fused._split_linear_train = keep
    assert wc.bits_equal(after, want), "max |d dx| %.3g" % float((after[1] - want[1]).abs().max())
    assert not wc.bits_equal(after[0], before[0]) and not wc.bits_equal(after[1], before[1])


# --------------------------------------------------------------------------------------------------------------- GraphedDetector
TOL = {'pred_logits': 2e-4, 'hs_embed': 2e-4, 'pred_boxes': 1e-5}   # tests/test_models_gpu.py::test_graphed_detector_equals_eager
# One representative per kind of tensor.  Every perturbation is t <- 1.1 t + 0.1 mean|t| cos(.): measured on the host forward of this
# model and frame, it moves the eager pred_logits by (in units of TOL): conv2 760, running_var 396, linear1 1277, sampling_offsets.bias
# 558, class_embed 3281, level_embed 1619, query_embed 3037 -- the test asserts at least 100.
TENSORS = ["backbone.0.body.layer2.0.conv2.weight", "backbone.0.body.layer2.0.bn1.running_var",
           "transformer.encoder.layers.0.linear1.weight", "transformer.decoder.layers.0.cross_attn.sampling_offsets.bias",
           "class_embed.5.weight", "transformer.level_embed", "query_embed.weight"]
WAYS = ["load_state_dict", "inplace_then_revalidate", "data_write_then_weights_changed"]
S = 0.1


@pytest.fixture(scope="module")
def detector_model(dev):
    model, post, args = um.build("cfg2_deformable_tracking", factory.build_model, config.make_args, device=dev)
    model.to(dev).tracking()
    g = torch.Generator().manual_seed(3)
    img = torch.randn(1, 3, 160, 192, generator=g).to(dev)
    target = [{'track_query_hs_embeds': torch.randn(5, 256, generator=g).to(dev),
               'track_query_boxes': (torch.rand(5, 4, generator=g) * 0.5 + 0.2).to(dev),
               'image_id': torch.tensor([1], device=dev)}]
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return model, post, img, target, state


@pytest.fixture()
def detector(detector_model):
    model, post, img, target, state = detector_model
    yield detector_model
    model.load_state_dict({k: v.clone() for k, v in state.items()})   # (also tells every wrapper: the hook of load_state_dict)


def _eager(model, img, target):
    with torch.no_grad():
        out = model(img, [dict(target[0])], None)[0]
    return {k: out[k].clone() for k in TOL}


def _replayed(det, img, target, calls=3):
    """Call until a graph replays (call 1: eager, first sighting; call 2: capture + replay; call 3: replay) -> the last output."""
    with torch.no_grad():
        for _ in range(calls):
            out = det(img, [dict(target[0])], None)[0]
    assert len(det._graphs) == 1, "no graph was captured"
    return {k: out[k].clone() for k in TOL}


def _agree(replay, eager, what):
    for k in TOL:
        assert torch.allclose(replay[k], eager[k], atol=TOL[k], rtol=1e-5), "%s: %s off by %.3g (tolerance %.1g)" % (
            what, k, float((replay[k] - eager[k]).abs().max()), TOL[k])


def _new_values(t):
    i = torch.arange(t.numel(), dtype=torch.float32)
    return t.detach() * (1 + S) + S * float(t.detach().abs().mean()) * torch.cos(0.7 * i + 0.3).reshape(t.shape).to(t.device)


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("name", TENSORS, ids=[n.split(".", 1)[1] if n.startswith(("backbone", "transformer")) else n for n in TENSORS])
def test_graphed_detector_follows_a_weight_change(detector, name, way):
    from trackformer_amd.graphed import GraphedDetector
    model, post, img, target, state = detector
    det = GraphedDetector(model)
    before = _eager(model, img, target)
    _agree(_replayed(det, img, target), before, "before the change")
    t = wc.tensor_of(model, name)
    new = _new_values(t)
    if way == "load_state_dict":
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        sd[name] = new
        model.load_state_dict(sd)
    elif way == "inplace_then_revalidate":
        with torch.no_grad():
            t.copy_(new)
        assert det.revalidate() is False
    else:
        t.data.copy_(new)
        fused.weights_changed()
    after = _eager(model, img, target)
    moved = float((after['pred_logits'] - before['pred_logits']).abs().max()) / TOL['pred_logits']
    assert moved >= 100, "the perturbation of %s moves the eager logits by only %.1f tolerances: the case could not tell" % (name, moved)
    with torch.no_grad():
        first = det(img, [dict(target[0])], None)[0]        # the graphs are gone: this call runs eagerly
    assert len(det._graphs) == 0
    _agree({k: first[k] for k in TOL}, after, "first call after %s of %s (moved %.0f tolerances)" % (way, name, moved))
    _agree(_replayed(det, img, target, calls=2), after, "replay after %s of %s (moved %.0f tolerances)" % (way, name, moved))


def test_replay_with_nothing_changed_keeps_its_graphs_and_a_switch_drops_them(detector):
    from trackformer_amd.graphed import GraphedDetector
    model, post, img, target, state = detector
    det = GraphedDetector(model)
    want = _eager(model, img, target)
    _replayed(det, img, target)
    entry = next(iter(det._graphs.values()))
    assert det.revalidate() is True
    _agree(_replayed(det, img, target, calls=2), want, "replay")
    assert len(det._graphs) == 1 and next(iter(det._graphs.values())) is entry
    prev = fused.set_split_terms(6)
    try:
        with torch.no_grad():
            out6 = det(img, [dict(target[0])], None)[0]
        assert len(det._graphs) == 0                        # captured under sixteen terms: dropped, this call ran six-term kernels
        eager6 = _eager(model, img, target)
        _agree({k: out6[k] for k in TOL}, eager6, "after set_split_terms(6)")
        _agree(_replayed(det, img, target, calls=2), eager6, "replay under six terms")
    finally:
        fused.set_split_terms(prev)
    with torch.no_grad():
        det(img, [dict(target[0])], None)
    assert len(det._graphs) == 0                            # ... and back


def test_tracker_reset_alone_picks_up_an_optimiser_step(detector):
    from trackformer_amd.graphed import GraphedDetector
    from trackformer_amd.tracker import Tracker
    model, post, img, target, state = detector
    det = GraphedDetector(model)
    tracker = Tracker(det, post, config.tracker_cfg(), False)
    tracker.reset()
    before = _eager(model, img, target)
    _agree(_replayed(det, img, target), before, "before the step")
    p = wc.tensor_of(model, "transformer.encoder.layers.0.linear1.weight")
    p.grad = (p.detach() - _new_values(p)) / 0.5
    torch.optim.SGD([p], lr=0.5).step()                     # outside the wrapper: nothing tells it
    p.grad = None
    after = _eager(model, img, target)
    moved = float((after['pred_logits'] - before['pred_logits']).abs().max()) / TOL['pred_logits']
    assert moved >= 100, moved
    assert len(det._graphs) == 1
    tracker.reset()                                         # once per sequence
    assert len(det._graphs) == 0
    _agree(_replayed(det, img, target), after, "after Tracker.reset() (moved %.0f tolerances)" % moved)
