"""GPU (-m gpu): one full training step of the detection model with the trainable bottlenecks' convolutions on the library's own
kernels (backbone.set_split_conv_training; trackformer_amd/csrc/conv_bwd.h), alone and with every other training switch on: EVERY
gradient tensor and every loss against the float64 step with the harness of tests/util_train_gradients.py (unchanged: the bound is
its own, 4 x the class yardstick), and the proof from the model that the route ran --
  * conv_train_counts()["wgrad_own"] equals the number of trainable 3 x 3 convolutions (stride 1 and 2) of layer2-layer4,
  * ["dgrad_own"] the number of stride-1 ones (the input gradient of a stride-2 one is torch's: "dgrad_torch"),
  * fused.train_route_counts() rises by the 1 x 1 stride-1 convolutions: "wgrad_own" by their number, "dgrad_own" by one less (the
    input of layer2's first convolution comes from the frozen layer1 and carries no graph: no input gradient is asked for).
The model, the observers and the other switches are those of tests/test_train_gradients_gpu.py and
tests/test_layernorm_train_step_gpu.py; `switches` here adds the new one.  The mask model is left out (its known miss is documented
in tests/test_layernorm_train_step_gpu.py).

Measured on an MI355X (worst rel. L2 / worst element of the class as multiples of its yardstick; the bound is 4), the switch alone in
three steps and every switch on in one: backbone layer2 2.3-2.4 / 2.1-2.3, layer3 2.9-3.0 / 3.1-3.4 (worst: layer3.0.conv1.weight),
layer4 1.1 / 1.1-1.4; with the switch off 0.6 / 0.4, 0.9-1.0 / 0.9-1.2, 1.0 / 1.0.  The counts are as stated: 39 forwards, 10 + 3
input gradients own / torch, 13 weight gradients, 26 + 25 through the linears' kernels.
Why the route cuts long contractions into pieces (fused._conv_ksplit, the inference route's rule, in the 3 x 3 input gradient and in
the 1 x 1 layers' forward and input gradient): with one fp32 accumulator per output over the whole contraction the same step stands at
4.4-4.6 yardsticks in layer3.  Per call, on the step's own tensors against float64, such a 3 x 3 input gradient is 3.7e-07 / 5.2e-07 /
6.6e-07 rel. L2 at 9 x 128 / 256 / 512 products against 1.6-2.2e-07 for the convolution library's, with a one-sided error
(sum(err) / sum |err| = -0.11 ... -0.19); under the emulator, which adds every product in round-to-nearest fp32, the same kernel on
the same operands is unbiased (3.6e-07, 0.00): the matrix cores' accumulation is not round-to-nearest, and a long chain collects the
bias.  With only the 3 x 3 input gradient cut, layer3 stands at 3.6-3.7 / 3.9-4.04; the 1 x 1 layers alone then account for 2.7.
"""
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
    "conv_training": dict(conv=True),
    "all_on": dict(LN.ALL_ON, conv=True),
}


@contextlib.contextmanager
def switches(conv=False, **cfg):
    from trackformer_amd import backbone
    prev_raw = backbone._split_conv_train
    backbone.set_split_conv_training(conv)
    try:
        with LN.switches(**cfg):
            yield
    finally:
        backbone.set_split_conv_training(prev_raw)


def trainable_convs(model):
    """(3 x 3 stride 1, 3 x 3 stride 2, 1 x 1 stride 1, other) convolutions with a trainable weight under the backbone's layer2-layer4."""
    n3s1 = n3s2 = n1 = other = 0
    body = model.backbone[0].body
    for layer in (body.layer2, body.layer3, body.layer4):
        for m in layer.modules():
            if isinstance(m, torch.nn.Conv2d) and m.weight.requires_grad:
                if m.kernel_size == (3, 3) and m.stride == (1, 1):
                    n3s1 += 1
                elif m.kernel_size == (3, 3) and m.stride == (2, 2):
                    n3s2 += 1
                elif m.kernel_size == (1, 1) and m.stride == (1, 1):
                    n1 += 1
                else:
                    other += 1
    return n3s1, n3s2, n1, other


def run_route(dev, models, cfg):   # noqa: F811
    from trackformer_amd import fused, msda
    model, criterion = models(False)
    samples, targets = um.train_batch(device=dev, masks=False)
    with switches(**cfg), T.observed(model) as obs:
        fused.layernorm_train_counts(reset=True)
        fused.conv_train_counts(reset=True)
        step = G.run_step(model, criterion, samples, targets, train=True, rng_seed=7)
        torch.cuda.synchronize(dev)
        counts = (msda.fused_train_counts(), fused.train_route_counts(reset=True), fused.conv_train_counts(reset=True))
    model.zero_grad(set_to_none=True)
    return step, model, obs, counts


@pytest.mark.parametrize("name", list(ROUTES))
def test_every_gradient_of_the_step_against_float64(dev, models, name):   # noqa: F811
    cfg = ROUTES[name]
    step, model, obs, (fused_counts, linear_counts, conv_counts) = run_route(dev, models, cfg)
    n3s1, n3s2, n1, other = trainable_convs(model)
    assert (n3s1, n3s2, n1, other) == (10, 3, 26, 3), (n3s1, n3s2, n1, other)     # ResNet-50 layer2-4: 13 bottlenecks + 3 projections
    assert conv_counts == {"fwd_own": n3s1 + n3s2 + n1, "fwd_torch": 0, "dgrad_own": n3s1, "dgrad_torch": n3s2, "wgrad_own": n3s1 + n3s2,
                           "wgrad_torch": 0}, conv_counts
    # what the 1 x 1 convolutions added to the linears' counters; the rest is what tests/test_train_gradients_gpu.py expects
    rest = dict(linear_counts, dgrad_own=linear_counts["dgrad_own"] - (n1 - 1), wgrad_own=linear_counts["wgrad_own"] - n1)
    T.assert_route_ran(model, obs, fused_counts, rest, **cfg)
    ref0 = G.reference_step(False, True, (), 7)
    flips, outside = G.relu_flips(step, ref0)
    ref, yard = G.reference_for(step, False, True, 7), G.yardstick(False, True, 7)
    report = G.compare(step, ref, yard)
    print("\n== route %s: %d gradients, %d convolutions on the own kernels; ReLU decisions other than float64's: %d (%d outside the "
          "undetermined set)" % (name, len(step.grads), n3s1 + n3s2 + n1, len(flips), outside))
    print(report.table(yard))
    report.assert_ok()


def test_switch_off_is_the_step_of_today(dev, models):   # noqa: F811
    """With the switch off the counters stay 0 and EVERY gradient is the one of the step on the code path without this route, bit for
    bit.  Both steps run with the deterministic MSDeformAttn backward and the convolution library's deterministic solvers (see
    tests/test_layernorm_train_step_gpu.py: two runs of the default route differ in the last bits by themselves)."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        off, _, _, (_, _, conv_counts) = run_route(dev, models, dict(det=True, conv=False))
        today, _ = T.run_route(dev, models, "deterministic_backward")
    finally:
        torch.backends.cudnn.deterministic = prev
    assert not any(conv_counts.values()), conv_counts
    assert set(off.grads) == set(today.grads)
    differing = [n for n in off.grads if not torch.equal(off.grads[n].view(torch.int32), today.grads[n].view(torch.int32))]
    assert not differing, differing
    assert off.losses == today.losses and off.total == today.total
