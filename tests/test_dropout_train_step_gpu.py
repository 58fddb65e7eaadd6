"""GPU (-m gpu): one training step of the small training model of tests/util_models.py, REBUILT WITH dropout = 0.1, on the device with every
training switch on and fused.set_dropout_training(True): every residual + LayerNorm site and every feed-forward hidden activation of the
step's forward runs the library's own dropout kernels, the sites' nn.Dropout modules are never called there, and every loss and gradient
is finite; with the switch off the same modules are called once per site and the counters stay 0.

No float64 comparison of the step here: the step harness (tests/util_train_gradients.py) builds its own dropout-free CPU reference and is
not changed.  The layer-level tests of tests/test_dropout_train_gpu.py (one encoder and one decoder layer, float64 "reference" mode
against the own route under one seed) carry the accuracy claim.

The tracking model runs the previous frame first WITHOUT gradients (detr_tracking.py); a forward without gradients is not a site of the
route (it keeps torch's dropout and is not counted), so the hooks below count the calls made with gradients enabled."""
import contextlib
import math

import pytest
import torch

from tests import test_criterion_fused_step_gpu as CF
from tests import util_models as um
from tests.test_train_gradients_gpu import dev   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model_and_criterion(dev):   # noqa: F811
    from trackformer_amd import config, factory
    args = config.make_args("deformable", "tracking", "mot17", device=str(dev), **dict(um.TRAIN_OVERRIDES, dropout=0.1))
    torch.manual_seed(42)
    model, criterion, _ = factory.build_model(args)
    um.perturb_state_dict(model, 2)
    return model.to(dev), criterion.to(dev)


@contextlib.contextmanager
def every_switch(dropout):
    from trackformer_amd import backbone, fused
    prev = fused._dropout_train, backbone._split_conv_train
    fused.set_dropout_training(dropout)
    backbone.set_split_conv_training(True)
    try:
        with CF.switches(**CF.ALL_ON):
            yield
    finally:
        fused._dropout_train = prev[0]
        backbone.set_split_conv_training(prev[1])


def _sites(model):
    """{name: nn.Dropout} of the residual and feed-forward sites of the encoder's and the decoder's layers, and the layers."""
    tr = model.transformer
    layers = list(tr.encoder.layers) + list(tr.decoder.layers)
    sites = {}
    for i, layer in enumerate(layers):
        for name, m in layer.named_children():
            if isinstance(m, torch.nn.Dropout):
                sites["%d.%s" % (i, name)] = m
    return sites, layers


def _step(dev, model, criterion, dropout):   # noqa: F811
    from trackformer_amd import fused
    sites, layers = _sites(model)
    calls = {k: 0 for k in sites}

    def hook(name):
        def fn(*_):
            if torch.is_grad_enabled():
                calls[name] += 1
        return fn
    handles = [m.register_forward_hook(hook(k)) for k, m in sites.items()]
    samples, targets = um.train_batch(device=dev)
    try:
        with every_switch(dropout):
            fused.dropout_train_counts(reset=True)
            fused.layernorm_train_counts(reset=True)
            losses, total, grads = um.train_step(model, criterion, samples, targets)
            torch.cuda.synchronize(dev)
            counts = fused.dropout_train_counts(reset=True)
            ln_counts = fused.layernorm_train_counts(reset=True)
    finally:
        for h in handles:
            h.remove()
        model.zero_grad(set_to_none=True)
    assert all(math.isfinite(v) for v in losses.values()) and math.isfinite(total), losses
    assert grads and all(math.isfinite(v) for v in grads.values()), [k for k, v in grads.items() if not math.isfinite(v)]
    return calls, counts, ln_counts, layers


def test_step_with_dropout_on_the_own_kernels(dev, model_and_criterion):   # noqa: F811
    model, criterion = model_and_criterion
    calls, counts, ln_counts, layers = _step(dev, model, criterion, True)
    n_norms = sum(isinstance(m, torch.nn.LayerNorm) for layer in layers for m in layer.modules())
    assert n_norms == len(calls) - len(layers) > 0          # one residual site per LayerNorm, one feed-forward site per layer
    assert counts == {"ln_own": n_norms, "ln_torch": 0, "ffn_own": len(layers), "ffn_torch": 0}, counts
    assert ln_counts == {"own": 0, "torch": 0}, ln_counts   # every LayerNorm site went through the dropout kernels instead
    assert not any(calls.values()), calls                   # the sites' nn.Dropout modules never ran


def test_switch_off_calls_every_site_once(dev, model_and_criterion):   # noqa: F811
    model, criterion = model_and_criterion
    calls, counts, ln_counts, layers = _step(dev, model, criterion, False)
    assert all(v == 1 for v in calls.values()), calls
    assert counts == {"ln_own": 0, "ln_torch": 0, "ffn_own": 0, "ffn_torch": 0}, counts
    n_norms = sum(isinstance(m, torch.nn.LayerNorm) for layer in layers for m in layer.modules())
    assert ln_counts == {"own": n_norms, "torch": 0}, ln_counts
