"""GPU (-m gpu): one full training step of the mask model with the mask losses on the library's own kernels
(criterion.set_fused_masks; trackformer_amd/csrc/mask_loss.h), alone and with the fused set criterion and matching cost, EVERY gradient
tensor and every loss against the float64 step with the harness of tests/util_train_gradients.py (unchanged: the bound is its own), and
the proof that the route ran once: criterion.fused_mask_counts().

The model, the observers and the other switches are those of tests/test_criterion_fused_step_gpu.py; `switches` here adds the new one.
The residual + LayerNorm switch is NOT part of these routes: tests/test_layernorm_train_step_gpu.py's mask_model_all_on has a documented
miss of its own in the mask-head class.  The routes leave the model's forward as it is (asserted bit for bit below, under the
deterministic settings): only loss_mask, loss_dice and the gradient entering pred_masks differ from mask_model_default."""
import contextlib

import pytest
import torch

from tests import test_criterion_fused_step_gpu as CF
from tests import test_models_cpu as shared
from tests import test_train_gradients_gpu as T
from tests import util_models as um
from tests import util_train_gradients as G
from tests.test_train_gradients_gpu import dev, models   # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ROUTES = {
    "mask_model_mask_losses": dict(masks=True, mask_losses=True),
    "mask_model_criterion_all": dict(masks=True, mask_losses=True, crit=True, cost=True),
}
MASK_KEYS = ("loss_mask", "loss_dice")


@contextlib.contextmanager
def switches(mask_losses=False, **cfg):
    from trackformer_amd import criterion
    prev = criterion._fused_masks
    criterion.set_fused_masks(mask_losses)
    try:
        with CF.switches(**cfg):
            yield
    finally:
        criterion.set_fused_masks(prev)


def run_route(dev, models, cfg, touch_switch=True):   # noqa: F811
    from trackformer_amd import criterion, fused, matcher, msda
    train, rng_seed = cfg.get("train", True), cfg.get("rng_seed", 7)
    model, crit = models(True)
    samples, targets = um.train_batch(device=dev, masks=True)
    with (switches(**cfg) if touch_switch else CF.switches(**cfg)), T.observed(model) as obs:
        criterion.fused_counts(reset=True)
        matcher.fused_cost_counts(reset=True)
        criterion.fused_mask_counts(reset=True)
        step = G.run_step(model, crit, samples, targets, train=train, rng_seed=rng_seed)
        torch.cuda.synchronize(dev)
        counts = (msda.fused_train_counts(), fused.train_route_counts(reset=True), criterion.fused_counts(reset=True),
                  matcher.fused_cost_counts(reset=True), criterion.fused_mask_counts(reset=True))
    model.zero_grad(set_to_none=True)
    return step, model, obs, counts


@pytest.mark.parametrize("name", list(ROUTES))
def test_every_gradient_of_the_step_against_float64(dev, models, name):   # noqa: F811
    cfg = ROUTES[name]
    step, model, obs, (fused_counts, linear_counts, crit_counts, cost_counts, mask_counts) = run_route(dev, models, cfg)
    T.assert_route_ran(model, obs, fused_counts, linear_counts, **dict(cfg, layers_at_once=not cfg.get("crit", False)))
    assert mask_counts == {"own": 1, "torch": 0}, mask_counts
    assert crit_counts == ({"own": 1, "torch": 0} if cfg.get("crit") else {"own": 0, "torch": 0}), crit_counts
    assert cost_counts["torch"] == 0 and (cost_counts["own"] >= 1 if cfg.get("cost") else cost_counts["own"] == 0), cost_counts
    ref, yard = G.reference_for(step, True, True, 7), G.yardstick(True, True, 7)
    assert step.matches == ref.matches and len(step.matches) > 0
    assert all(k in step.losses for k in MASK_KEYS)
    report = G.compare(step, ref, yard)
    print("\n== route %s: %d gradients; mask losses %r, criterion %r, matching cost %r" % (name, len(step.grads), mask_counts, crit_counts,
                                                                                           cost_counts))
    print(report.table(yard))
    print("mask losses: " + ", ".join("%s error %.3e (bound %.3e)" % ((k,) + report.loss[k]) for k in MASK_KEYS))
    report.assert_ok()


def test_switch_off_is_the_step_of_today_and_on_leaves_the_forward_alone(dev, models):   # noqa: F811
    """Under the deterministic MSDeformAttn backward and the convolution library's deterministic solvers (as
    tests/test_criterion_fused_step_gpu.py's test_switches_off_is_the_step_of_today): with the switch off the fused route is never
    consulted, the counter stays 0 and losses and gradients equal, bit for bit, those of a step that never touched the switch.  With
    it on every loss except loss_mask and loss_dice keeps its bits: the model's forward is untouched."""
    from trackformer_amd import criterion
    orig = criterion.SetCriterion._loss_masks_fused

    def boom(*a, **k):
        raise AssertionError("the fused mask route was consulted with the switch off")
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        criterion.SetCriterion._loss_masks_fused = boom
        try:
            off, _, _, counts_off = run_route(dev, models, dict(det=True, mask_losses=False))
            today, _, _, counts_today = run_route(dev, models, dict(det=True), touch_switch=False)
        finally:
            criterion.SetCriterion._loss_masks_fused = orig
        on, _, _, counts_on = run_route(dev, models, dict(det=True, mask_losses=True))
    finally:
        torch.backends.cudnn.deterministic = prev
    assert counts_off[4] == counts_today[4] == {"own": 0, "torch": 0} and counts_on[4] == {"own": 1, "torch": 0}
    assert off.losses == today.losses and off.total == today.total and off.matches == today.matches
    promised = [n for n in off.grads if not G.class_of(n).startswith("backbone") and G.class_of(n) != "input_proj"]
    differing = [n for n in off.grads if not torch.equal(off.grads[n].view(torch.int32), today.grads[n].view(torch.int32))]
    assert set(off.grads) == set(today.grads) and not set(differing) & set(promised), sorted(set(differing) & set(promised))
    assert on.matches == today.matches and set(on.losses) == set(today.losses)
    assert {k for k in today.losses if on.losses[k] != today.losses[k]} <= set(MASK_KEYS)
    for k in MASK_KEYS:
        assert abs(on.losses[k] - today.losses[k]) <= 1e-5 * max(1.0, abs(today.losses[k])), (k, on.losses[k], today.losses[k])


def test_training_step_with_the_switch_on_matches_the_reference(dev):
    """cfg 5's training path with the mask losses on the own kernels against the reference's own losses and gradient norms, at the
    tolerance tests/test_models_gpu.py uses for the same fixture."""
    from trackformer_amd import criterion
    prev = criterion._fused_masks
    criterion.set_fused_masks(True)
    criterion.fused_mask_counts(reset=True)
    try:
        loss_dict, total, grads = shared.run_train_step(device=dev, masks=True)
        counts = criterion.fused_mask_counts(reset=True)
    finally:
        criterion.set_fused_masks(prev)
    assert counts == {"own": 1, "torch": 0}, counts
    shared.compare_train_to_golden(loss_dict, total, grads, rtol=2e-3, fixture="train_cfg5_masks_small.npz")
