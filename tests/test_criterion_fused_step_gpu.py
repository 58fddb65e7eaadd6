"""GPU (-m gpu): one full training step with the set criterion and the matching cost on the library's own kernels
(criterion.set_fused, matcher.set_fused_cost; trackformer_amd/csrc/criterion.h), each alone and with every other training switch on,
EVERY gradient tensor and every loss against the float64 step with the harness of tests/util_train_gradients.py (unchanged: the bound
is its own; it also asserts that every assignment of the matcher equals the float64 step's), and the proof that the routes ran: the
counters of both.

The model, the observers and the other switches are those of tests/test_layernorm_train_step_gpu.py; `switches` here adds the two new
ones.

First run on an MI355X (worst rel. L2 of the class as a multiple of its yardstick; the bound is 4): every route passes in every class
(criterion_fused: encoder 0.35, decoder 0.88, heads 1.52; matcher_fused_cost: 0.26, 0.94, 0.95; all_on: 0.27, 0.76, 0.92;
track_queries_all_on: 0.78, 0.82, 0.66; backbone and input_proj 0.64-1.01), the worst loss error is 1.8e-07 (loss_giou; bound 4.8e-07),
the criterion ran once and the cost kernel twice per step (the previous frame's matching and this frame's), the switch-off step equals
today's bit for bit and two steps with every switch on differ in no gradient."""
import contextlib

import pytest
import torch

from tests import test_layernorm_train_step_gpu as LN
from tests import test_train_gradients_gpu as T
from tests import util_models as um
from tests import util_train_gradients as G
from tests.test_train_gradients_gpu import dev, models   # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ALL_ON = dict(LN.ALL_ON, crit=True, cost=True)
ROUTES = {
    "criterion_fused": dict(crit=True),
    "matcher_fused_cost": dict(cost=True),
    "all_on": ALL_ON,
    "track_queries_all_on": dict(ALL_ON, rng_seed=G.TRACK_QUERY_SEED),
}


@contextlib.contextmanager
def switches(crit=False, cost=False, **cfg):
    from trackformer_amd import criterion, matcher
    prev = criterion._fused, matcher._fused_cost
    criterion.set_fused(crit)
    matcher.set_fused_cost(cost)
    try:
        with LN.switches(**cfg):
            yield
    finally:
        criterion.set_fused(prev[0])
        matcher.set_fused_cost(prev[1])


def run_route(dev, models, cfg):   # noqa: F811
    from trackformer_amd import criterion, fused, matcher, msda
    train, rng_seed = cfg.get("train", True), cfg.get("rng_seed", 7)
    model, crit = models(False)
    samples, targets = um.train_batch(device=dev, masks=False)
    with switches(**cfg), T.observed(model) as obs:
        fused.layernorm_train_counts(reset=True)
        criterion.fused_counts(reset=True)
        matcher.fused_cost_counts(reset=True)
        step = G.run_step(model, crit, samples, targets, train=train, rng_seed=rng_seed)
        torch.cuda.synchronize(dev)
        counts = (msda.fused_train_counts(), fused.train_route_counts(reset=True), fused.layernorm_train_counts(reset=True),
                  criterion.fused_counts(reset=True), matcher.fused_cost_counts(reset=True))
    model.zero_grad(set_to_none=True)
    return step, model, obs, counts


@pytest.mark.parametrize("name", list(ROUTES))
def test_every_gradient_of_the_step_against_float64(dev, models, name):   # noqa: F811
    cfg = ROUTES[name]
    train, rng_seed = cfg.get("train", True), cfg.get("rng_seed", 7)
    step, model, obs, (fused_counts, linear_counts, ln_counts, crit_counts, cost_counts) = run_route(dev, models, cfg)
    # with the criterion on the own kernels _layers_at_once is not called: the observer of the harness counts 0 calls of it
    T.assert_route_ran(model, obs, fused_counts, linear_counts, **dict(cfg, layers_at_once=not cfg.get("crit", False)))
    n_matches = len(step.matches)
    assert crit_counts == ({"own": 1, "torch": 0} if cfg.get("crit") else {"own": 0, "torch": 0}), crit_counts
    assert cost_counts["torch"] == 0 and (cost_counts["own"] >= 1 if cfg.get("cost") else cost_counts["own"] == 0), cost_counts
    if rng_seed == G.TRACK_QUERY_SEED:
        assert all(b["n_track_queries"] > 0 for b in step.bookkeeping), step.bookkeeping
    ref, yard = G.reference_for(step, False, train, rng_seed), G.yardstick(False, train, rng_seed)
    assert step.matches == ref.matches and n_matches > 0
    report = G.compare(step, ref, yard)
    print("\n== route %s: %d gradients; criterion %r, matching cost %r" % (name, len(step.grads), crit_counts, cost_counts))
    print(report.table(yard))
    report.assert_ok()


def test_switches_off_is_the_step_of_today(dev, models):   # noqa: F811
    """With both switches off the counters stay 0 and the step's losses and gradients equal the step without these routes bit for bit
    (under the deterministic MSDeformAttn backward and the convolution library's deterministic solvers, as
    tests/test_layernorm_train_step_gpu.py: the default route's float atomics make two runs of the SAME code differ)."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        off, model, _, (_, _, _, crit_counts, cost_counts) = run_route(dev, models, dict(det=True, crit=False, cost=False))
        today, _ = T.run_route(dev, models, "deterministic_backward")
    finally:
        torch.backends.cudnn.deterministic = prev
    assert crit_counts == {"own": 0, "torch": 0} and cost_counts == {"own": 0, "torch": 0}
    assert off.losses == today.losses and off.total == today.total
    assert off.matches == today.matches
    promised = [n for n in off.grads if not G.class_of(n).startswith("backbone") and G.class_of(n) != "input_proj"]
    differing = [n for n in off.grads if not torch.equal(off.grads[n].view(torch.int32), today.grads[n].view(torch.int32))]
    assert set(off.grads) == set(today.grads) and not set(differing) & set(promised), sorted(set(differing) & set(promised))


def test_all_switches_on_is_bitwise_reproducible(dev, models):   # noqa: F811
    """Two identical steps with every switch on: bit-identical losses and gradients for every transformer, head and embedding
    parameter (the backbone's and input_proj's convolution gradients come from the libraries and are not part of the promise)."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        a, _, _, ca = run_route(dev, models, ROUTES["all_on"])
        b, _, _, cb = run_route(dev, models, ROUTES["all_on"])
    finally:
        torch.backends.cudnn.deterministic = prev
    assert ca[3] == cb[3] == {"own": 1, "torch": 0} and ca[4] == cb[4] and ca[4]["own"] >= 1
    assert a.losses == b.losses and a.total == b.total, {k: (a.losses[k], b.losses[k]) for k in a.losses if a.losses[k] != b.losses[k]}
    promised = [n for n in a.grads if not G.class_of(n).startswith("backbone") and G.class_of(n) != "input_proj"]
    differing = [n for n in a.grads if not torch.equal(a.grads[n].view(torch.int32), b.grads[n].view(torch.int32))]
    print("\n== all switches on, two steps: gradients differing bitwise: %r" % differing)
    assert not set(differing) & set(promised), sorted(set(differing) & set(promised))
