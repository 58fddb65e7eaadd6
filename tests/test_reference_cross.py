"""CPU: the module surface the reference's scripts rely on, crossed with the reference's own classes through what they produced
(tests/golden/cross_state_dicts.npz, cross_checkpoint_*.npz; tests/golden/make_golden_cross.py).

  * src/track.py:85 does a STRICT `load_state_dict` of a checkpoint written by the reference's `build_model`: for every model
    case the reference model's state_dict loads strictly into the repo's model and the repo's into the reference's (same keys,
    same shapes), and after loading the two models compute the same outputs.  The reference's checkpoints are regenerated from
    their seeds and checked key by key against the sums of the reference's own weights."""
import os

import numpy as np
import pytest
import torch

from tests import util_models as um
from trackformer_amd import config, factory

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "cross_state_dicts.npz"))


def reference_state_dict(ref, case, weight_seed):
    """The reference's state_dict (build_model + um.build(weight_seed)): same entries, each with the reference's sums."""
    sd = um.build(case, factory.build_model, config.make_args, weight_seed=weight_seed)[0].state_dict()
    sums = ref["%s/sums_seed%d" % (case, weight_seed)]
    assert len(sums) == len(sd)
    for (k, v), (s, a) in zip(sd.items(), sums):
        assert abs(float(v.double().sum()) - s) <= 1e-9 * max(1.0, a) and abs(float(v.double().abs().sum()) - a) <= 1e-9 * max(1.0, a), k
    return sd


@pytest.mark.parametrize("case", list(um.MODEL_CASES))
def test_state_dicts_load_strictly_both_ways(ref, case):
    sd_theirs = reference_state_dict(ref, case, 5)
    ours, _, _ = um.build(case, factory.build_model, config.make_args, weight_seed=6)
    sd_ours = ours.state_dict()
    assert str(ref[case + "/keys"]).split("\n") == list(sd_ours)                 # same keys in the same order
    assert str(ref[case + "/shapes"]).split("\n") == ["x".join(map(str, v.shape)) for v in sd_ours.values()]
    missing = ours.load_state_dict(sd_theirs, strict=True)                    # track.py:85
    assert not missing.missing_keys and not missing.unexpected_keys
    for k, v in ours.state_dict().items():
        assert torch.equal(v, sd_theirs[k]), k


@pytest.mark.parametrize("case", ["cfg2_deformable_tracking", "cfg1_plain_detr", "deformable_two_stage"])
def test_reference_checkpoint_gives_reference_outputs(ref, case):
    """A state_dict produced by the reference's build_model, loaded strictly into the repo's model: same outputs."""
    theirs = reference_state_dict(ref, case, 9)
    ours, post_o, args = um.build(case, factory.build_model, config.make_args, weight_seed=10)
    ours.load_state_dict(theirs, strict=True)
    ours.tracking() if hasattr(ours, "tracking") else ours.eval()
    img, prev, target = um.model_inputs(case, args.hidden_dim)
    with torch.no_grad():
        b, *_ = ours(img, [dict(t) for t in target] if target else None, None)
    a = np.load(os.path.join(GOLDEN, "cross_checkpoint_%s.npz" % case))
    np.testing.assert_allclose(b['pred_boxes'].numpy(), a['pred_boxes'], atol=2e-5)
    np.testing.assert_allclose(b['pred_logits'].numpy(), a['pred_logits'], atol=1e-4)
