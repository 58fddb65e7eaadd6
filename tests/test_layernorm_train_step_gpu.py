"""GPU (-m gpu): one full training step with the residual + LayerNorm sites on the library's own kernels
(fused.set_layernorm_training; trackformer_amd/csrc/layernorm_bwd.h), alone and with every other training switch on, EVERY gradient
tensor and every loss against the float64 step with the harness of tests/util_train_gradients.py (unchanged: the bound is its own,
4 x the class yardstick), and the proof that the route ran: layernorm_train_counts()["own"] equals the number of nn.LayerNorm modules
under the encoder's and the decoder's layers, counted from the model.

The model, the observers and the other switches are those of tests/test_train_gradients_gpu.py; `switches` here adds the new one.

First run on an MI355X (worst rel. L2 of the class as a multiple of its yardstick; the bound is 4): layernorm_training, all_on,
eval_mode_with_gradients_all_on and track_queries_all_on pass in every class (layernorm_training: encoder 0.27, decoder 0.90, heads
1.12; all_on: 0.25, 0.80, 1.09; eval mode: 0.23, 0.80, 1.26; track queries: 0.69, 0.85, 0.74; backbone and input_proj 0.66-1.10), the
switch-off and the reproducibility tests pass (no gradient differs bitwise between two steps with every switch on).

mask_model_all_on MISSES THE BOUND in one class when it runs in this file's order, as the first step of the mask model in the process:
mask head worst rel. L2 5.886e-05 (bbox_attention.q_linear.weight; bound 4 x 1.486e-06 = 5.94e-06), worst element 1.919e-04 (bound
6.63e-06), 14 failures, all of them bbox_attention.{q,k}_linear and mask-head parameters; every other class of the same step is inside
(backbone 0.61-0.92, input_proj 0.69, encoder 0.24, decoder 0.78, heads 0.92 yardsticks; mask head 39.6), the 13 sites ran the own kernels.  Measured
next to it in one fresh process, the same model and batch: the step with every switch on WITH the LayerNorm route differs from the
step WITHOUT it (which passes the same harness in tests/test_train_gradients_gpu.py at 0.53 yardsticks) by 9.6e-07 rel. L2 in
bbox_attention.q_linear.weight, 9.2e-07 in k_linear.weight, 4.4e-07 in mask_head.lay1.weight -- what two runs of the route without
it differ by (8.1e-07, 7.8e-07, 4.4e-07); two ReLU decisions of the mask head (gn1, gn5; |z| of 3e-07 and 1.7e-06, sites the harness
does not track) fall on the other side.  The cause of the miss in this file's order is not found; the bound stays as the harness has it."""
import contextlib

import pytest
import torch

from tests import test_train_gradients_gpu as T
from tests import util_models as um
from tests import util_train_gradients as G
from tests.test_train_gradients_gpu import dev, models   # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ALL_ON = dict(T.ALL_ON, ln=True)
ROUTES = {
    "layernorm_training": dict(ln=True),
    "all_on": ALL_ON,
    "eval_mode_with_gradients_all_on": dict(ALL_ON, train=False),
    "track_queries_all_on": dict(ALL_ON, rng_seed=G.TRACK_QUERY_SEED),
    "mask_model_all_on": dict(ALL_ON, masks=True),
}


@contextlib.contextmanager
def switches(ln=False, **cfg):
    from trackformer_amd import fused
    prev_raw = fused._layernorm_train
    fused.set_layernorm_training(ln)
    try:
        with T.switches(**cfg):
            yield
    finally:
        fused.set_layernorm_training(prev_raw)


def layer_norms(model):
    """The nn.LayerNorm modules of the encoder's and the decoder's layers: every one of them sits behind one residual_norm site."""
    tr = model.transformer
    return [m for layers in (tr.encoder.layers, tr.decoder.layers) for m in layers.modules() if isinstance(m, torch.nn.LayerNorm)]


def run_route(dev, models, cfg):   # noqa: F811
    from trackformer_amd import fused, msda
    masks, train, rng_seed = cfg.get("masks", False), cfg.get("train", True), cfg.get("rng_seed", 7)
    model, criterion = models(masks)
    samples, targets = um.train_batch(device=dev, masks=masks)
    with switches(**cfg), T.observed(model) as obs:
        fused.layernorm_train_counts(reset=True)
        step = G.run_step(model, criterion, samples, targets, train=train, rng_seed=rng_seed)
        torch.cuda.synchronize(dev)
        counts = (msda.fused_train_counts(), fused.train_route_counts(reset=True), fused.layernorm_train_counts(reset=True))
    model.zero_grad(set_to_none=True)
    return step, model, obs, counts


@pytest.mark.parametrize("name", list(ROUTES))
def test_every_gradient_of_the_step_against_float64(dev, models, name):   # noqa: F811
    cfg = ROUTES[name]
    masks, train, rng_seed = cfg.get("masks", False), cfg.get("train", True), cfg.get("rng_seed", 7)
    step, model, obs, (fused_counts, linear_counts, ln_counts) = run_route(dev, models, cfg)
    T.assert_route_ran(model, obs, fused_counts, linear_counts, **cfg)
    n_norms = len(layer_norms(model))
    assert n_norms > 0 and ln_counts == {"own": n_norms, "torch": 0}, (ln_counts, n_norms)
    if rng_seed == G.TRACK_QUERY_SEED:
        assert all(b["n_track_queries"] > 0 for b in step.bookkeeping), step.bookkeeping
    ref0 = G.reference_step(masks, train, (), rng_seed)
    flips, outside = G.relu_flips(step, ref0)
    ref, yard = G.reference_for(step, masks, train, rng_seed), G.yardstick(masks, train, rng_seed)
    report = G.compare(step, ref, yard)
    print("\n== route %s: %d gradients, %d LayerNorm sites on the own kernels; ReLU decisions other than float64's: %d (%d outside the "
          "undetermined set)" % (name, len(step.grads), n_norms, len(flips), outside))
    print(report.table(yard))
    report.assert_ok()


def _layernorm_parameter_names(model):
    ids = {id(p) for m in layer_norms(model) for p in m.parameters()}
    return [n for n, p in model.named_parameters() if id(p) in ids]


def test_switch_off_is_the_step_of_today(dev, models):   # noqa: F811
    """With the switch off the counters stay 0 and the LayerNorm parameters' gradients are those of the step without this route, bit
    for bit.  Both steps run with the deterministic MSDeformAttn backward and the convolution library's deterministic solvers: the
    `default` route's float atomics (and the library's layer3 / layer4 forward, see test_all_switches_on_is_bitwise_reproducible in
    tests/test_train_gradients_gpu.py) make two runs of the SAME code differ in the last bits, which says nothing about the switch."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        off, model, _, (_, _, ln_counts) = run_route(dev, models, dict(det=True, ln=False))
        today, _ = T.run_route(dev, models, "deterministic_backward")
        default, _, _, (_, _, ln_default) = run_route(dev, models, dict())
    finally:
        torch.backends.cudnn.deterministic = prev
    assert ln_counts == {"own": 0, "torch": 0} and ln_default == {"own": 0, "torch": 0}, (ln_counts, ln_default)
    names = _layernorm_parameter_names(model)
    assert len(names) == 2 * len(layer_norms(model))
    differing = [n for n in names if not torch.equal(off.grads[n].view(torch.int32), today.grads[n].view(torch.int32))]
    assert not differing, differing
    assert set(default.grads) == set(today.grads)


def test_all_switches_on_is_bitwise_reproducible(dev, models):   # noqa: F811
    """Two identical steps with every switch on (set up as tests/test_train_gradients_gpu.py's test of the same name): bit-identical
    losses and gradients for every transformer, head and embedding parameter -- the LayerNorm gradients now among the kernels that
    promise it."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        a, model, _, (_, _, ca) = run_route(dev, models, ROUTES["all_on"])
        b, _, _, (_, _, cb) = run_route(dev, models, ROUTES["all_on"])
    finally:
        torch.backends.cudnn.deterministic = prev
    assert ca == cb == {"own": len(layer_norms(model)), "torch": 0}
    assert a.losses == b.losses and a.total == b.total, {k: (a.losses[k], b.losses[k]) for k in a.losses if a.losses[k] != b.losses[k]}
    promised = [n for n in a.grads if not G.class_of(n).startswith("backbone") and G.class_of(n) != "input_proj"]
    assert set(_layernorm_parameter_names(model)) <= set(promised)
    differing = [n for n in a.grads if not torch.equal(a.grads[n].view(torch.int32), b.grads[n].view(torch.int32))]
    print("\n== all switches on, two steps: gradients differing bitwise: %r" % differing)
    assert not set(differing) & set(promised), sorted(set(differing) & set(promised))
