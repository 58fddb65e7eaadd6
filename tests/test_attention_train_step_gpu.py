"""GPU (-m gpu): one full training step with the decoder's query self-attention on the library's own kernels
(fused.set_attention_training; trackformer_amd/csrc/mha_bwd.h), alone and with every other training switch on, EVERY gradient tensor and
every loss against the float64 step with the harness of tests/util_train_gradients.py (unchanged: the bound is its own), and the proof
that the route ran: attention_train_counts()["own"] equals the number of decoder layers (the harness's model trains with dropout 0), none
`torch`.

The model, the observers and the other switches are those of tests/test_layernorm_train_step_gpu.py; `switches` here adds the new one."""
import contextlib

import pytest
import torch

from tests import test_layernorm_train_step_gpu as LN
from tests import test_train_gradients_gpu as T
from tests import util_models as um
from tests import util_train_gradients as G
from tests.test_train_gradients_gpu import dev, models   # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ROUTES = {
    "attention_training": dict(attn=True),
    "all_on": dict(LN.ALL_ON, attn=True),
    "track_queries_all_on": dict(LN.ALL_ON, attn=True, rng_seed=G.TRACK_QUERY_SEED),
}
ZERO = {"own": 0, "own_dropout": 0, "reference": 0, "torch": 0}


@contextlib.contextmanager
def switches(attn=False, **cfg):
    from trackformer_amd import fused
    prev_raw = fused._attention_train
    fused.set_attention_training(attn)
    try:
        with LN.switches(**cfg):
            yield
    finally:
        fused.set_attention_training(prev_raw)


def run_route(dev, models, cfg):   # noqa: F811
    from trackformer_amd import fused
    masks, train, rng_seed = cfg.get("masks", False), cfg.get("train", True), cfg.get("rng_seed", 7)
    model, criterion = models(masks)
    samples, targets = um.train_batch(device=dev, masks=masks)
    with switches(**cfg), T.observed(model):
        fused.attention_train_counts(reset=True)
        step = G.run_step(model, criterion, samples, targets, train=train, rng_seed=rng_seed)
        torch.cuda.synchronize(dev)
        counts = fused.attention_train_counts(reset=True)
        fused.train_route_counts(reset=True)
        fused.layernorm_train_counts(reset=True)
    model.zero_grad(set_to_none=True)
    return step, model, counts


@pytest.mark.parametrize("name", list(ROUTES))
def test_every_gradient_of_the_step_against_float64(dev, models, name):   # noqa: F811
    cfg = ROUTES[name]
    masks, train, rng_seed = cfg.get("masks", False), cfg.get("train", True), cfg.get("rng_seed", 7)
    step, model, counts = run_route(dev, models, cfg)
    n_sites = len(model.transformer.decoder.layers)
    assert n_sites > 0 and counts == dict(ZERO, own=n_sites), (counts, n_sites)
    if rng_seed == G.TRACK_QUERY_SEED:
        assert all(b["n_track_queries"] > 0 for b in step.bookkeeping), step.bookkeeping
    ref, yard = G.reference_for(step, masks, train, rng_seed), G.yardstick(masks, train, rng_seed)
    report = G.compare(step, ref, yard)
    print("\n== route %s: %d gradients, %d self-attention sites on the own kernels" % (name, len(step.grads), n_sites))
    print(report.table(yard))
    report.assert_ok()


def test_switch_off_is_the_step_of_today(dev, models):   # noqa: F811
    """With the switch off the counters stay 0 and every transformer gradient is that of a step in which the switch was never touched,
    bit for bit (both with the deterministic MSDeformAttn backward and the convolution library's deterministic solvers, as
    tests/test_layernorm_train_step_gpu.py explains)."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        off, model, counts = run_route(dev, models, dict(det=True, attn=False))
        today, _ = T.run_route(dev, models, "deterministic_backward")
    finally:
        torch.backends.cudnn.deterministic = prev
    assert counts == ZERO, counts
    names = [n for n in off.grads if n.startswith("transformer.decoder")]
    assert any("self_attn.in_proj_weight" in n for n in names)
    differing = [n for n in names if not torch.equal(off.grads[n].view(torch.int32), today.grads[n].view(torch.int32))]
    assert not differing, differing
    assert set(off.grads) == set(today.grads)
