"""GPU (-m gpu): one full training step per route on the small model of tests/util_models.py (two images, 426 tokens each over four
levels, the second one padded; 40 object queries; M*L*P = 128; no row count a multiple of a tile), EVERY gradient tensor against the
float64 step on the CPU with the bound of tests/util_train_gradients.py, and the proof that the route really ran: which MSDeformAttn
path, which backward kernel, how many linears took the library's own gradient kernels (derived from the model, not from a first run).

The float64 and fp32 CPU steps are computed once per configuration (util_train_gradients caches them); the model is built once per
module and only ever differentiated, never updated.  Every route puts the switches back in `finally`."""
import contextlib

import pytest
import torch

from tests import util_models as um
from tests import util_train_gradients as G

pytestmark = pytest.mark.gpu

ALL_ON = dict(fused=True, det=True, split=True)
ROUTES = {
    "default": dict(),
    "deterministic_backward": dict(det=True),
    "fused_training": dict(fused=True),
    "fused_training_deterministic": dict(fused=True, det=True),
    "split_linear_three_terms": dict(split=True, terms=16),
    "split_linear_six_terms": dict(split=True, terms=6),
    "all_on": ALL_ON,
    "reference_formulations": dict(train_fold=False, layers_at_once=False),     # of the two defaults
    "eval_mode_with_gradients_all_on": dict(ALL_ON, train=False),               # gradient checks, saliency
    "mask_model_default": dict(masks=True),
    "mask_model_all_on": dict(ALL_ON, masks=True),
    # util_models' host-RNG seed appends no track query (util_train_gradients.TRACK_QUERY_SEED): the decoder with track queries
    "track_queries_default": dict(rng_seed=G.TRACK_QUERY_SEED),
    "track_queries_all_on": dict(ALL_ON, rng_seed=G.TRACK_QUERY_SEED),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from trackformer_amd import _cabi
    _cabi.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev):
    from trackformer_amd import config, factory
    built = {}

    def get(masks):
        if masks not in built:
            model, criterion, _ = um.build_train(factory.build_model, config.make_args, device=dev, masks=masks)
            built[masks] = (model.to(dev), criterion.to(dev))
        return built[masks]
    return get


@contextlib.contextmanager
def switches(fused=False, det=False, split=False, terms=16, train_fold=True, layers_at_once=True, **_):
    from trackformer_amd import backbone, criterion, msda
    from trackformer_amd import fused as fused_mod
    prev_fused_raw, prev_split_raw = msda._fused_training, fused_mod._split_linear_train
    prev_det = msda.set_deterministic_backward(det)
    msda.set_fused_training(fused)
    fused_mod.set_split_linear_training(split)
    prev_terms = fused_mod.set_split_terms(terms)
    prev_fold = backbone.set_train_fold(train_fold)
    prev_at_once = criterion.set_layers_at_once(layers_at_once)
    try:
        yield
    finally:
        criterion.set_layers_at_once(prev_at_once)
        backbone.set_train_fold(prev_fold)
        fused_mod.set_split_terms(prev_terms)
        fused_mod.set_split_linear_training(prev_split_raw)
        msda.set_fused_training(prev_fused_raw)
        msda.set_deterministic_backward(prev_det)


class Observed:
    def __init__(self):
        self.attn_calls = 0          # MSDeformAttn forwards with gradients enabled
        self.reference_graph = 0     # ... that reached MSDeformAttnFunction (the reference's module graph)
        self.fused_entry = 0         # ... that reached ms_deform_attn_fused
        self.backward_kernels = []   # tf_msda_last_kernel after every operator backward
        self.linear_train = []       # (parameter name or "cat", weight shape) of every linear_train call
        self.bias_act = 0            # backbone._BiasAct passes (the training fold)
        self.layers_at_once = 0


@contextlib.contextmanager
def observed(model):
    """Counts what a step runs, around the product's own functions (each wrapper calls the original)."""
    from trackformer_amd import backbone, criterion, msda
    from trackformer_amd import fused as fused_mod
    obs = Observed()
    names = {id(p): n for n, p in model.named_parameters()}
    hooks = [m.register_forward_pre_hook(lambda mod, args: setattr(obs, "attn_calls", obs.attn_calls + int(torch.is_grad_enabled())))
             for m in model.modules() if isinstance(m, msda.MSDeformAttn)]
    orig = dict(function=msda.MSDeformAttnFunction, fused=msda.ms_deform_attn_fused, backward=msda.ms_deform_attn_backward,
                linear_train=fused_mod.linear_train, bias_act=backbone._BiasAct.forward,
                at_once=criterion.SetCriterion._layers_at_once)

    class CountingFunction:
        @staticmethod
        def apply(*a):
            obs.reference_graph += int(torch.is_grad_enabled())
            return orig["function"].apply(*a)

    def fused_entry(*a, **k):
        obs.fused_entry += 1
        return orig["fused"](*a, **k)

    def backward(*a, **k):
        out = orig["backward"](*a, **k)
        obs.backward_kernels.append(msda.last_kernel())
        return out

    def linear_train(x, weight, bias=None, relu=False):
        obs.linear_train.append((names.get(id(weight), "cat"), tuple(weight.shape)))
        return orig["linear_train"](x, weight, bias, relu)

    def bias_act(ctx, *a):
        obs.bias_act += 1
        return orig["bias_act"](ctx, *a)

    def at_once(self, *a, **k):
        obs.layers_at_once += 1
        return orig["at_once"](self, *a, **k)

    msda.MSDeformAttnFunction, msda.ms_deform_attn_fused, msda.ms_deform_attn_backward = CountingFunction, fused_entry, backward
    fused_mod.linear_train = linear_train
    backbone._BiasAct.forward = staticmethod(bias_act)
    criterion.SetCriterion._layers_at_once = at_once
    msda.fused_train_counts(reset=True)
    fused_mod.train_route_counts(reset=True)
    try:
        yield obs
    finally:
        msda.MSDeformAttnFunction, msda.ms_deform_attn_fused, msda.ms_deform_attn_backward = orig["function"], orig["fused"], orig["backward"]
        fused_mod.linear_train = orig["linear_train"]
        backbone._BiasAct.forward = orig["bias_act"]
        criterion.SetCriterion._layers_at_once = orig["at_once"]
        for h in hooks:
            h.remove()


def covered_linears(model, fused):
    """What set_split_linear_training covers in one step, from the model: per MSDeformAttn its value and output projection and the
    two query projections (ONE concatenated projection when training through the fused entry), per feed-forward block linear1 (with
    its ReLU) and linear2.  nn.MultiheadAttention, the heads and the convolutions are not covered."""
    from trackformer_amd.msda import MSDeformAttn
    n_attn = sum(isinstance(m, MSDeformAttn) for m in model.transformer.modules())
    n_ffn = sum(hasattr(m, "linear1") and hasattr(m, "linear2") for m in model.transformer.modules())
    return n_attn, n_attn * (3 if fused else 4) + 2 * n_ffn


def assert_route_ran(model, obs, fused_counts, linear_counts, fused=False, det=False, split=False, train_fold=True,
                     layers_at_once=True, train=True, **_):
    n_attn, n_linear = covered_linears(model, fused)
    assert n_attn == 5 and obs.attn_calls == n_attn, (n_attn, obs.attn_calls)
    if fused:
        assert fused_counts == {"fused": obs.attn_calls, "reference": 0}, fused_counts
        assert (obs.fused_entry, obs.reference_graph) == (n_attn, 0), (obs.fused_entry, obs.reference_graph)
    else:
        assert fused_counts == {"fused": 0, "reference": 0}, fused_counts
        assert (obs.fused_entry, obs.reference_graph) == (0, n_attn), (obs.fused_entry, obs.reference_graph)
    assert len(obs.backward_kernels) == n_attn, obs.backward_kernels
    assert all(k.startswith("msda_bwd_det") == det for k in obs.backward_kernels), obs.backward_kernels
    if split:
        # a gradient the library's kernels do not take is computed by torch inside linear_train: which calls those would be
        fallbacks = [(n, s) for n, s in obs.linear_train if s[0] % 64 or s[1] % 4]
        assert len(obs.linear_train) == n_linear and obs.linear_train.count(("cat", (384, 256))) == (n_attn if fused else 0), obs.linear_train
        want = {"dgrad_own": n_linear, "dgrad_torch": 0, "wgrad_own": n_linear, "wgrad_torch": 0, "bias_own": n_linear, "bias_torch": 0}
        assert linear_counts == want, (linear_counts, "torch fallbacks expected from the shapes: %r" % fallbacks)
    else:
        assert not obs.linear_train and not any(linear_counts.values()), (obs.linear_train, linear_counts)
    # ResNet-50: layer2-4 hold 13 bottlenecks = 39 convolutions + 3 projections of the identity branch
    assert obs.bias_act == (42 if train_fold and train else 0), obs.bias_act
    assert obs.layers_at_once == int(layers_at_once), obs.layers_at_once


def run_route(dev, models, name):
    from trackformer_amd import fused as fused_mod
    from trackformer_amd import msda
    cfg = ROUTES[name]
    masks, train, rng_seed = cfg.get("masks", False), cfg.get("train", True), cfg.get("rng_seed", 7)
    model, criterion = models(masks)
    samples, targets = um.train_batch(device=dev, masks=masks)
    with switches(**cfg), observed(model) as obs:
        step = G.run_step(model, criterion, samples, targets, train=train, rng_seed=rng_seed)
        torch.cuda.synchronize(dev)
        fused_counts, linear_counts = msda.fused_train_counts(), fused_mod.train_route_counts(reset=True)
    model.zero_grad(set_to_none=True)
    return step, (model, obs, fused_counts, linear_counts)


@pytest.mark.parametrize("name", list(ROUTES))
def test_every_gradient_of_the_step_against_float64(dev, models, name):
    cfg = ROUTES[name]
    masks, train, rng_seed = cfg.get("masks", False), cfg.get("train", True), cfg.get("rng_seed", 7)
    step, ran = run_route(dev, models, name)
    assert_route_ran(*ran, **cfg)
    if rng_seed == G.TRACK_QUERY_SEED:
        assert all(b["n_track_queries"] > 0 for b in step.bookkeeping), step.bookkeeping
    ref0 = G.reference_step(masks, train, (), rng_seed)
    flips, outside = G.relu_flips(step, ref0)
    ref, yard = G.reference_for(step, masks, train, rng_seed), G.yardstick(masks, train, rng_seed)
    report = G.compare(step, ref, yard)
    print("\n== route %s: %d gradients; ReLU decisions other than float64's: %d (sites %s; %d outside the undetermined set)"
          % (name, len(step.grads), len(flips), sorted({b for b, _ in flips}), outside))
    print(report.table(yard))
    report.assert_ok()


def test_all_switches_on_is_bitwise_reproducible(dev, models):
    """What the three switches together promise, so far tested per operator: two identical steps give bit-identical losses and
    bit-identical gradients for every transformer, head and embedding parameter (the backbone's and input_proj's convolution and
    GroupNorm gradients come from the libraries and are not part of the promise).
    The convolution library is asked for its deterministic solvers (torch.backends.cudnn.deterministic) for the two steps: without
    that, aten::miopen_convolution's FORWARD in layer3 / layer4 of the backbone differs from run to run in the last bits (measured:
    the layer2 feature map is bit-identical, the layer3 / layer4 maps differ by up to 2.6e-5 absolute, with every switch of this
    project on or off), and every loss and gradient of the step depends on those maps."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        a, _ = run_route(dev, models, "all_on")
        b, _ = run_route(dev, models, "all_on")
    finally:
        torch.backends.cudnn.deterministic = prev
    assert a.losses == b.losses and a.total == b.total, {k: (a.losses[k], b.losses[k]) for k in a.losses if a.losses[k] != b.losses[k]}
    promised = [n for n in a.grads if not G.class_of(n).startswith("backbone") and G.class_of(n) != "input_proj"]
    assert len(promised) == 184 - 42 - 16, len(promised)      # ResNet-50 layer2-4: 42 convolutions; input_proj: 4 x (conv w, b + GroupNorm w, b)
    differing = [n for n in a.grads if not torch.equal(a.grads[n].view(torch.int32), b.grads[n].view(torch.int32))]
    print("\n== all switches on, two steps: gradients differing bitwise: %r" % differing)
    assert not set(differing) & set(promised), sorted(set(differing) & set(promised))
