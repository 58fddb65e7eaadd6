"""CPU (-m "not gpu"): one training step, every gradient tensor against float64 (tests/util_train_gradients.py).

The product's own CPU path -- the real host operator of libtf_msda.so, as in tests/test_models_cpu.py -- must pass the comparator,
and the comparator must reject norm-preserving or small mutations of that passing gradient set, which the existing comparison of 13
gradient norms at rtol 2e-3 (test_models_cpu.compare_train_to_golden) cannot see."""
import pytest
import torch

from tests import test_models_cpu as shared
from tests import util_models as um
from tests import util_train_gradients as G


def _host_step(masks=False, rng_seed=7):
    from trackformer_amd import _cabi, config, factory
    _cabi.lib()      # the host operator is the library's: nothing is patched
    model, criterion, _ = um.build_train(factory.build_model, config.make_args, masks=masks)
    samples, targets = um.train_batch(masks=masks)
    return G.run_step(model, criterion, samples, targets, rng_seed=rng_seed)


@pytest.fixture(scope="module")
def passing():
    """(host step, its float64 reference, the yardstick): computed once, never modified (mutations copy the tensor they change)."""
    step = _host_step()
    return step, G.reference_for(step), G.yardstick()


def test_reference_covers_every_parameter_and_no_gradient_is_zero():
    ref = G.reference_step()
    assert len(ref.grads) == 184 and sum(g.numel() for g in ref.grads.values()) > 33e6
    assert all(float(g.abs().max()) > 0 for g in ref.grads.values())
    assert {G.class_of(n) for n in ref.grads} == set(G.CLASSES) - {"mask head"}
    # previous frame + 3 decoder outputs; ReLU sites: 13 trainable bottlenecks x 3, then 2 + 3 feed-forward blocks
    assert len(ref.matches) == 4 and len(ref.relu) == 39 + 5
    # the undetermined ReLU decisions are a handful: the precondition "equal elsewhere" covers all but ~1 in 25 000 units
    assert sum(int(u.sum()) for u in ref.undetermined) * 10000 < sum(u.numel() for u in ref.undetermined)
    # the loss does not depend on the padded tokens of the second image (85 of 426): no gradient reaches their hidden units
    assert [int(m.reshape(2, -1).any(1).sum()) for m in ref.matters] == [2] * 44
    assert int(ref.matters[39].any(-1).sum()) == 2 * 426 - 85


def test_yardstick_is_an_fp32_yardstick():
    """Every class has one, none is as good as exact, and with the ReLU decisions taken out none is looser than fp32 round-off."""
    yard = G.yardstick()
    for c in set(G.CLASSES) - {"mask head"}:
        assert G.CLASS_MIN / 8 < yard["floor"][c] <= yard["l2"][c] < 2e-5, (c, yard)
    assert max(yard["loss"].values()) < 4e-6


def test_host_path_passes_with_full_tensors(passing):
    step, ref, yard = passing
    report = G.compare(step, ref, yard)
    print(report.table(yard))
    report.assert_ok()


def test_host_path_with_mask_head_passes_with_full_tensors():
    step = _host_step(masks=True)
    ref, yard = G.reference_for(step, True), G.yardstick(True)
    assert len(ref.grads) == 216 and "mask head" in yard["l2"]
    report = G.compare(step, ref, yard)
    print(report.table(yard))
    report.assert_ok()


def test_host_path_with_track_queries_passes_with_full_tensors():
    """util_models' host-RNG seed draws no track query; under TRACK_QUERY_SEED the decoder runs 40 object queries plus appended track
    queries, and the matcher is constrained by them."""
    step = _host_step(rng_seed=G.TRACK_QUERY_SEED)
    assert all(b["n_track_queries"] > 0 and any(b["track_queries_mask"]) for b in step.bookkeeping)
    ref, yard = G.reference_for(step, False, True, G.TRACK_QUERY_SEED), G.yardstick(False, True, G.TRACK_QUERY_SEED)
    report = G.compare(step, ref, yard)
    print(report.table(yard))
    report.assert_ok()


def _norms_pass_the_existing_comparison(step, grads):
    """compare_train_to_golden's arithmetic on the norms of `grads` -- raises if the existing test would notice."""
    mutated = step.with_grads(grads)
    shared.compare_train_to_golden(step.losses, step.total, mutated.norms(), rtol=2e-4)


def _rejected(passing, grads, names, what=("rel L2", "max element")):
    step, ref, yard = passing
    report = G.compare(step.with_grads(grads), ref, yard)
    names = (names,) if isinstance(names, str) else names
    assert not report
    for name in names:
        for w in what:
            assert report.failed(w, name), (w, name, report.failures[:4])
    assert {f[1] for f in report.failures} == set(names)      # and nothing else is blamed
    return report


def test_rejects_x_and_y_swapped_in_a_sampling_offsets_gradient(passing):
    grads, name = G.mutate_xy_swap(passing[0].grads)
    assert name in um.TRAIN_GRAD_KEYS
    _norms_pass_the_existing_comparison(passing[0], grads)       # the gap: the norm comparison does not notice
    _rejected(passing, grads, name)


def test_rejects_two_heads_exchanged_in_a_value_proj_gradient(passing):
    grads, name = G.mutate_heads_swapped(passing[0].grads)
    assert name in um.TRAIN_GRAD_KEYS
    _norms_pass_the_existing_comparison(passing[0], grads)       # the gap: the norm comparison does not notice
    _rejected(passing, grads, name)


def test_rejects_a_transposed_block_in_a_linear1_gradient(passing):
    grads, name = G.mutate_block_transposed(passing[0].grads)
    _rejected(passing, grads, name)


def test_rejects_a_split_of_the_concatenated_projection_shifted_by_one_row(passing):
    grads, names = G.mutate_split_shifted(passing[0].grads)
    _rejected(passing, grads, names)


def test_rejects_gradients_of_two_decoder_layers_exchanged(passing):
    grads, names = G.mutate_layers_exchanged(passing[0].grads)
    _rejected(passing, grads, names)


def test_rejects_a_gradient_scaled_by_1_001(passing):
    grads, name = G.mutate_scaled(passing[0].grads)
    report = _rejected(passing, grads, name)
    l2 = report.failed("rel L2", name)[0][2]
    assert 0.9e-3 < l2 < 1.1e-3


def test_rejects_a_missing_name(passing):
    grads, name = G.mutate_missing(passing[0].grads)
    _rejected(passing, grads, name, what=("missing gradient",))


def test_rejects_other_assignments_and_other_bookkeeping(passing):
    step, ref, yard = passing
    other = G.Step(step.losses, step.total, step.grads, step.matches[:-1] + [step.matches[0]], step.bookkeeping)
    assert G.compare(other, ref, yard).failed("matcher indices")
    book = [dict(b) for b in step.bookkeeping]
    book[0]["n_track_queries"] += 1
    other = G.Step(step.losses, step.total, step.grads, step.matches, book)
    assert G.compare(other, ref, yard).failed("track-query bookkeeping")


def test_a_relu_decision_outside_the_undetermined_set_is_refused(passing):
    step, ref, _ = passing
    relu = [r.clone() for r in step.relu]
    ref0 = G.reference_step()
    determined = (~ref0.undetermined[0] & ref0.matters[0]).view(-1).nonzero()[0, 0]
    relu[0].view(-1)[determined] ^= True
    other = G.Step(step.losses, step.total, step.grads, step.matches, step.bookkeeping, relu)
    with pytest.raises(AssertionError, match="outside the undetermined set"):
        G.reference_for(other)
    assert torch.equal(step.relu[0], ref.relu[0])
