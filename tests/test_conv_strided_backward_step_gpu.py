"""GPU (-m gpu): the cfg-3 small training step of tests/test_conv_backward_step_gpu.py with the trainable bottlenecks' convolutions on
the library's own kernels AND the stride-2 layers among them (backbone.set_split_conv_training + fused.set_strided_conv_training;
trackformer_amd/csrc/conv_strided_bwd.h), alone and with every other training switch on: EVERY gradient tensor and every loss against
the float64 step with the harness of tests/util_train_gradients.py (unchanged: the bound is its own), and the proof from the model
that no convolution of layer2-layer4 left the own path --
  * conv_train_counts()["fwd_own"] is 42: the 39 of the route without the new switch + the three strided 1 x 1 projections,
  * ["dgrad_own"] is 15: the 10 stride-1 3 x 3, the 3 stride-2 3 x 3 and the two projections whose input carries a graph (layer2.0's
    input comes from the frozen layer1: no input gradient is asked for), ["dgrad_torch"] is 0,
  * ["wgrad_own"] is 16 = 13 + 3, ["wgrad_torch"] is 0,
  * the linears' counters are those of tests/test_conv_backward_step_gpu.py.

Measured on an MI355X (worst rel. L2 / worst element of the class as multiples of its yardstick; the bound is 4), two runs of each
route: backbone layer2 2.7-2.8 / 2.5-2.6, layer3 3.3 / 3.8 with the two switches alone and 3.2-3.3 / 3.4-3.8 with every switch on
(worst: layer3.0.conv1.weight), layer4 1.2 / 1.2-1.4 -- a thinner margin than the 3.0 / 3.1-3.2 of the route without the strided
layers in the second of those runs.  The contraction of the new input gradient is cut by fused._STRIDED_DGRAD_KSPLIT_POLICY (pieces of at least
256 products); pieces of 128 products were tried in one run and stood at 3.6 / 4.2 in layer3, outside the bound, so they were not kept."""
import contextlib

import pytest
import torch

from tests import test_conv_backward_step_gpu as C
from tests import test_layernorm_train_step_gpu as LN
from tests import test_train_gradients_gpu as T
from tests import util_train_gradients as G
from tests.test_train_gradients_gpu import dev, models   # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ROUTES = {
    "strided_conv_training": dict(conv=True),
    "all_on": dict(LN.ALL_ON, conv=True),
}


@contextlib.contextmanager
def strided():
    from trackformer_amd import fused
    prev_raw = fused._strided_conv_train
    fused.set_strided_conv_training(True)
    try:
        yield
    finally:
        fused.set_strided_conv_training(prev_raw)


@pytest.mark.parametrize("name", list(ROUTES))
def test_every_gradient_of_the_step_against_float64(dev, models, name):   # noqa: F811
    cfg = ROUTES[name]
    with strided():
        step, model, obs, (fused_counts, linear_counts, conv_counts) = C.run_route(dev, models, cfg)
    n3s1, n3s2, n1, other = C.trainable_convs(model)
    assert (n3s1, n3s2, n1, other) == (10, 3, 26, 3), (n3s1, n3s2, n1, other)     # ResNet-50 layer2-4: 13 bottlenecks + 3 projections
    assert conv_counts == {"fwd_own": 42, "fwd_torch": 0, "dgrad_own": 15, "dgrad_torch": 0, "wgrad_own": 16, "wgrad_torch": 0}, conv_counts
    # what the 1 x 1 stride-1 convolutions added to the linears' counters; the rest is what tests/test_train_gradients_gpu.py expects
    rest = dict(linear_counts, dgrad_own=linear_counts["dgrad_own"] - (n1 - 1), wgrad_own=linear_counts["wgrad_own"] - n1)
    T.assert_route_ran(model, obs, fused_counts, rest, **cfg)
    ref0 = G.reference_step(False, True, (), 7)
    flips, outside = G.relu_flips(step, ref0)
    ref, yard = G.reference_for(step, False, True, 7), G.yardstick(False, True, 7)
    report = G.compare(step, ref, yard)
    print("\n== route %s: %d gradients, 42 convolutions on the own kernels; ReLU decisions other than float64's: %d (%d outside the "
          "undetermined set)" % (name, len(step.grads), len(flips), outside))
    print(report.table(yard))
    report.assert_ok()
