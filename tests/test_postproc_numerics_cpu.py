"""CPU: the yardsticks of tests/util_postproc_numerics.py judge themselves -- the index formulas equal torch's, the ambiguous share of
every table entry (the GPU tables included) stays under its cap on the float64 reference alone, the rules accept the torch fp32 module
chains the kernels replace and reject every named mutant (the test prints which profile rejects which) -- and then judge the kernels of
trackformer_amd/csrc/fused_ops.hip under the SIMT emulator (tests/emu_lib.py) over the same tables."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import emu_lib
from tests import util_postproc_numerics as P

needs_emu = pytest.mark.skipif(not emu_lib.available(), reason="no host clang++ to build the emulated library with")
f32 = np.float32


def _ids(v):
    return str(v).replace(" ", "")


_order = P.order_of


# ---- the utility against torch ----------------------------------------------------------------------------------------------------------
def test_index_formulas_equal_torch_and_differ_from_the_exact_integer_index():
    differ = P.selftest_index_arithmetic()
    print("fp32 nearest index != dst * in // out at %d of the (in < 40, out < 90) pairs, e.g. %s" % (len(differ), differ[:8]))
    assert set(P.FP32_VS_EXACT_PAIRS) <= set(differ)
    pairs = set()
    for lw, pad, img, out, n in P.LABEL_CASES_GPU:
        pairs |= {(img[0], out[0]), (img[1], out[1])}
    assert pairs & set(differ), "no label-map case whose fp32 nearest index differs from the exact one"
    assert pairs & set(P.FP32_VS_EXACT_PAIRS)
    ups = set()
    for N, q, lo, hi, C in P.UPS_CASES_CPU:
        ups |= {(lo[0], hi[0]), (lo[1], hi[1])}
    assert len(ups & set(P.FP32_VS_EXACT_PAIRS)) >= 3


@pytest.mark.parametrize("case", P.LABEL_CASES_GPU, ids=_ids)
def test_label_map_ambiguous_share_is_capped_on_the_reference_alone(case):
    """Every (profile, shape) of the CPU and GPU tables, float64 only.  Maps above 300 rows: every 16th output row here (the GPU test
    asserts the cap on the whole map before it looks at the kernel)."""
    lw, pad, img, out, n = case
    rows = np.arange(0, out[0], 16) if out[0] > 300 else None
    for prof in P.LABEL_PROFILES:
        x = torch.from_numpy(P.label_logits(prof, n, *lw))
        for kind in ("identity", "holes"):
            if kind == "holes" and out[0] > 300:
                continue
            v = P.label_check(None, x, _order(n, kind), pad, img, out, P.threshold_of(prof), rows=rows)
            print("AMBIGUOUS %-12s %s %s: %.2e (owned %.2f)" % (prof, case, kind, v.ambiguous, v.owned))
            assert v.ambiguous <= P.AMBIG_CAP, (prof, case, v.ambiguous)
            assert v.violations == 0 and v.differ == 0


@pytest.mark.parametrize("C", P.POST_C)
def test_postprocess_ambiguous_share_is_capped_on_the_reference_alone(C):
    for prof in P.POST_PROFILES:
        for Q in P.POST_Q:
            share = P.post_ambiguous_share(P.post_inputs(prof, Q, C)[0])
            print("AMBIGUOUS post %-8s Q %d C %d: %.2e" % (prof, Q, C, share))
            assert share <= P.AMBIG_CAP, (prof, Q, C, share)


# ---- the rules accept the torch fp32 chains ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.LABEL_CASES_CPU, ids=_ids)
def test_label_rule_accepts_the_module_chain(case):
    from trackformer_amd.detr_segmentation import PostProcessSegm
    lw, pad, img, out, n = case
    for prof in P.LABEL_PROFILES:
        x = torch.from_numpy(P.label_logits(prof, n, *lw))
        order = _order(n, "holes")
        thr = P.threshold_of(prof)
        want = P.torch_label_chain(x, order, pad, img, out, thr)
        if pad == img:   # the module itself (it resizes to the largest size of the batch: pad == img for one image)
            seg = PostProcessSegm()([{}], {'pred_masks': x[None]}, torch.tensor([list(out)]), torch.tensor([list(img)]),
                                    return_probs=True)[0]['masks'].squeeze(1)
            probs = torch.stack([seg[r] if r >= 0 else torch.full(tuple(out), -1.0) for r in order])
            best, owner = probs.max(dim=0)
            assert torch.equal(torch.where(best > thr, owner, torch.full_like(owner, -1)).to(torch.int16), want)
        v = P.label_check(want, x, order, pad, img, out, thr)
        print("DECISION torch chain %-12s %s: %s" % (prof, case, v))
        assert v.ok, (prof, case, str(v))
        vm = P.label_check(P.label_map_f32(x.numpy(), order, pad, img, out, thr), x, order, pad, img, out, thr)
        assert vm.ok, (prof, case, str(vm))


def _torch_post(logits, boxes, ih, iw, clip):
    from trackformer_amd.box_ops import clip_boxes_to_image
    from trackformer_amd.deformable_detr import DeformablePostProcess
    lt, bt = torch.from_numpy(logits)[None], torch.from_numpy(boxes)[None]
    res = DeformablePostProcess()({'pred_logits': lt, 'pred_boxes': bt}, torch.tensor([[ih, iw]], device=lt.device))[0]
    bx = clip_boxes_to_image(res['boxes'], (ih, iw)) if clip else res['boxes']
    return torch.cat([bx, res['scores'][:, None], res['labels'][:, None].float()], 1).numpy()


@pytest.mark.parametrize("C", P.POST_C)
@pytest.mark.parametrize("clip", [True, False])
def test_post_rule_accepts_the_module_chain(C, clip):
    worst = 0.0
    for prof in P.POST_PROFILES + ["non_finite", "subnormal", "saturated"]:
        for Q, (ih, iw) in ((400, (1080, 1920)), (257, (375, 1242)), (100000 if C == 20 else 300, (1080, 1920)), (255, (1, 1))):
            logits, boxes = P.post_inputs(prof, Q, C)
            got = _torch_post(logits, boxes, ih, iw, clip)
            v = P.post_check(got, logits, boxes, ih, iw, clip, fp32_scores=got[:, 4])
            assert v.ok, (prof, Q, C, str(v))
            worst = max(worst, v.score_ratio)
            vm = P.post_check(P.postprocess_f32(logits, boxes, ih, iw, clip), logits, boxes, ih, iw, clip, fp32_scores=got[:, 4])
            assert vm.ok, (prof, Q, C, str(vm))
    print("EXCESS torch fp32 post-process C %d clip %s: worst |s - p64| / tol %.3f" % (C, clip, worst))


def _torch_pool(x, b):
    t = torch.from_numpy(x).permute(0, 3, 1, 2) + torch.from_numpy(b).view(1, -1, 1, 1)
    return F.max_pool2d(torch.relu(t), 3, 2, 1).permute(0, 2, 3, 1).numpy()


def _torch_ups(low, fpn, q):
    up = F.interpolate(torch.from_numpy(low).permute(0, 3, 1, 2), size=fpn.shape[1:3], mode="nearest")
    want = (up.view(fpn.shape[0], q, *up.shape[1:]) + torch.from_numpy(fpn).permute(0, 3, 1, 2)[:, None]).flatten(0, 1)
    return want.permute(0, 2, 3, 1).numpy()


def _torch_bias_act(x, b, r, relu):
    v = torch.from_numpy(x) + torch.from_numpy(b)
    if r is not None:
        v = v + torch.from_numpy(r)
    return (torch.relu(v) if relu else v).numpy()


@pytest.mark.parametrize("prof", P.ADD_PROFILES)
def test_additive_references_equal_the_torch_chains_bit_for_bit(prof):
    """relu + max_pool2d, interpolate + add, the bias / residual / relu chain on the CPU: the float64-rounded-once references and the
    fp32 models give torch's bits, NaN positions and the signs of zeros included."""
    for shape in P.POOL_SHAPES_CPU:
        x, b, _ = P.additive_operands(prof, shape, shape[3], pool=True)
        want = _torch_pool(x, b)
        assert P.bits_differ(P.maxpool_reference(x, b), want) == 0, (prof, shape)
        assert P.bits_differ(P.maxpool_f32(x, b), want) == 0, (prof, shape)
    for N, q, lo, hi, C in P.UPS_CASES_CPU:
        low, _, _ = P.additive_operands(prof, (N, *lo, C), C)
        fpn, _, _ = P.additive_operands(prof, (N // q, *hi, C), C, seed=1)
        want = _torch_ups(low, fpn, q)
        assert P.bits_differ(P.upsample_add_reference(low, fpn, q), want) == 0, (prof, lo, hi)
        assert P.bits_differ(P.upsample_add_f32(low, fpn, q), want) == 0, (prof, lo, hi)
    for pos, C in P.BIAS_ACT_CASES_CPU:
        x, b, r = P.additive_operands(prof, (pos, C), C)
        for res in (None, r):
            for relu in (False, True):
                want = _torch_bias_act(x, b, res, relu)
                assert P.bits_differ(P.bias_act_reference(x, b, res, relu), want) == 0, (prof, pos, C, relu)
                assert P.bits_differ(P.bias_act_f32(x, b, res, relu), want) == 0, (prof, pos, C, relu)


# ---- exact profiles: saturation, ties, the threshold itself, NaN (the cases live in the utility: the GPU file runs them too) ------------
def test_exact_cases_and_nan_contract_hold_for_the_fp32_model_and_the_torch_chain():
    P.check_exact_label_cases(lambda *a: P.label_map_f32(*a))
    P.check_exact_label_cases(lambda x, *a: P.torch_label_chain(torch.from_numpy(x), *a).numpy())
    P.check_nan_label_contract(lambda *a: P.label_map_f32(*a))


# ---- every mutant is rejected -----------------------------------------------------------------------------------------------------------
def _raises(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_every_mutant_is_rejected():
    rejected = {}

    def note(mutant, profile):
        rejected.setdefault(mutant, profile)

    # label map: the margin rule over the table, then the exact cases
    for mutant in P.LABEL_MUTANTS:
        for prof in P.LABEL_PROFILES:
            for case in P.LABEL_CASES_CPU:
                if mutant in rejected:
                    break
                lw, pad, img, out, n = case
                x = P.label_logits(prof, n, *lw)
                order = _order(n, "holes", seed=1)
                thr = P.threshold_of(prof)
                got = P.label_map_f32(x, order, pad, img, out, thr, mutant=mutant)
                if not P.label_check(got, torch.from_numpy(x), order, pad, img, out, thr).ok:
                    note(mutant, "%s %s" % (prof, case))
        if mutant not in rejected and _raises(lambda: P.check_exact_label_cases(lambda *a: P.label_map_f32(*a, mutant=mutant))):
            note(mutant, "exact cases (zero / subnormal / saturated / equal rows)")
        if mutant not in rejected and _raises(lambda: P.check_nan_label_contract(lambda *a: P.label_map_f32(*a, mutant=mutant))):
            note(mutant, "non-finite contract")
    # post-processing
    for mutant in P.POST_MUTANTS:
        for prof in P.POST_PROFILES + ["saturated", "non_finite"]:
            for (ih, iw), clip in (((1080, 1920), True), ((375, 1242), False)):
                logits, boxes = P.post_inputs(prof, 400, 20)
                got = P.postprocess_f32(logits, boxes, ih, iw, clip, mutant=mutant)
                ok = P.post_check(got, logits, boxes, ih, iw, clip).ok
                if prof == "saturated":
                    ok = ok and bool((got[:, 5] == 0).all()) and bool((got[:, 4] == 1).all())
                if not ok:
                    note("post:" + mutant, "%s %dx%d clip %s" % (prof, ih, iw, clip))
    # pooling, bias_act, upsample + add: bits against the float64-rounded-once reference
    for mutant in P.POOL_MUTANTS:
        for prof in P.ADD_PROFILES:
            for shape in P.POOL_SHAPES_CPU:
                x, b, _ = P.additive_operands(prof, shape, shape[3], pool=True)
                if P.bits_differ(P.maxpool_f32(x, b, mutant=mutant), P.maxpool_reference(x, b)):
                    note("pool:" + mutant, "%s %s" % (prof, shape))
    for prof in P.ADD_PROFILES:
        for pos, C in P.BIAS_ACT_CASES_CPU:
            x, b, r = P.additive_operands(prof, (pos, C), C)
            if P.bits_differ(P.bias_act_f32(x, b, r, True, mutant="bias_quad_off_by_one"), P.bias_act_reference(x, b, r, True)):
                note("bias_act:bias_quad_off_by_one", "%s %s" % (prof, (pos, C)))
        for N, q, lo, hi, C in P.UPS_CASES_CPU:
            low, _, _ = P.additive_operands(prof, (N, *lo, C), C)
            fpn, _, _ = P.additive_operands(prof, (N // q, *hi, C), C, seed=1)
            if P.bits_differ(P.upsample_add_f32(low, fpn, q, mutant="exact_nearest"), P.upsample_add_reference(low, fpn, q)):
                note("upsample:exact_nearest", "%s %s -> %s" % (prof, lo, hi))
    for k, v in rejected.items():
        print("MUTANT %-32s rejected by %s" % (k, v))
    expected = (P.LABEL_MUTANTS + ["post:" + m for m in P.POST_MUTANTS] + ["pool:" + m for m in P.POOL_MUTANTS]
                + ["bias_act:bias_quad_off_by_one", "upsample:exact_nearest"])
    missing = [m for m in expected if m not in rejected]
    assert not missing, "mutants that no profile rejects: %s" % missing


# ---- the kernels under the emulator -----------------------------------------------------------------------------------------------------
@needs_emu
@pytest.mark.parametrize("case", P.LABEL_CASES_CPU, ids=_ids)
def test_emulated_label_map_obeys_the_decision_rule(case):
    lw, pad, img, out, n = case
    for prof in P.LABEL_PROFILES:
        x = P.label_logits(prof, n, *lw)
        thr = P.threshold_of(prof)
        for kind in ("identity", "holes"):
            order = _order(n, kind)
            ref = P.label_check(None, torch.from_numpy(x), order, pad, img, out, thr)
            assert ref.ambiguous <= P.AMBIG_CAP
            got = emu_lib.mask_label_map(x, order, pad, img, out, thr)
            v = P.label_check(got, torch.from_numpy(x), order, pad, img, out, thr)
            print("DECISION emulated label map %-12s %s %s: %s" % (prof, case, kind, v))
            assert v.ok, (prof, case, str(v))
            if prof == "neg":
                assert (got == -1).all()


@needs_emu
def test_emulated_label_map_exact_cases_and_non_finite_contract():
    P.check_exact_label_cases(emu_lib.mask_label_map)
    P.check_nan_label_contract(emu_lib.mask_label_map)
    # the issue's probe: two constant tracks, one NaN in the first: every pixel whose footprint touches it is -1
    x = np.stack([np.full((4, 4), 2.0, f32), np.full((4, 4), 1.0, f32)])
    x[0, 1, 2] = np.nan
    got = emu_lib.mask_label_map(x, [0, 1], (8, 8), (8, 8), (8, 8))
    want = P.torch_label_chain(torch.from_numpy(x), [0, 1], (8, 8), (8, 8), (8, 8)).numpy()
    assert np.array_equal(got, want) and int((got == -1).sum()) >= 16 and not (got == 1).any()


@needs_emu
@pytest.mark.parametrize("C", P.POST_C)
def test_emulated_postprocess_obeys_the_rules(C):
    worst = (0.0, None)
    for prof in P.POST_PROFILES + ["non_finite", "subnormal", "saturated"]:
        for Q in P.POST_Q:
            if Q == 100000 and not (C == 20 and prof in ("unit", "non_finite")):
                continue
            for (ih, iw), clip in (((1080, 1920), True), ((375, 1242), False), ((1, 1), True)):
                logits, boxes = P.post_inputs(prof, Q, C)
                got = emu_lib.postprocess_pack(logits, boxes, float(ih), float(iw), clip)
                ref = _torch_post(logits, boxes, ih, iw, clip)
                v = P.post_check(got, logits, boxes, ih, iw, clip, fp32_scores=ref[:, 4])
                assert v.ok, (prof, Q, C, str(v))
                # the non-finite contract, element for element with the module chain: NaN scores and their labels
                assert np.array_equal(np.isnan(got[:, 4]), np.isnan(ref[:, 4]))
                nan = np.isnan(ref[:, 4])
                assert np.array_equal(got[nan, 5], ref[nan, 5])
                if prof in ("subnormal", "saturated"):
                    assert (got[:, 5] == 0).all() and (got[:, 4] == (0.5 if prof == "subnormal" else 1.0)).all()
                if v.score_ratio > worst[0]:
                    worst = (v.score_ratio, "%s Q %d: %s" % (prof, Q, v))
    print("EXCESS emulated post-process C %d: %s" % (C, worst[1]))


@needs_emu
def test_emulated_postprocess_non_finite_boxes_under_clip():
    """include/tf_fused.h: fminf(fmaxf(v, 0), side) turns a NaN coordinate into 0 and +-inf into the nearer bound; without clip they pass."""
    logits, boxes = P.post_inputs("unit", 64, 4)
    boxes[3, 0], boxes[5, 3], boxes[7, 2], boxes[9, 1] = np.nan, np.nan, np.inf, -np.inf
    for clip in (True, False):
        got = emu_lib.postprocess_pack(logits, boxes, 375.0, 1242.0, clip)
        assert P.bits_differ(got[:, :4], P.postprocess_boxes_f32(boxes, 375, 1242, clip)) == 0
        assert np.isfinite(got[:, 4]).all()
    got = emu_lib.postprocess_pack(logits, boxes, 375.0, 1242.0, True)
    assert np.isfinite(got[:, :4]).all() and got[3, 0] == 0 and got[3, 2] == 0 and got[5, 1] == 0 and got[5, 3] == 0


@needs_emu
@pytest.mark.parametrize("prof", P.ADD_PROFILES)
def test_emulated_additive_kernels_equal_float64_rounded_once(prof):
    for shape in P.POOL_SHAPES_CPU:
        x, b, _ = P.additive_operands(prof, shape, shape[3], pool=True)
        got = emu_lib.bias_relu_maxpool(x, b)
        assert P.bits_differ(got, P.maxpool_reference(x, b)) == 0, (prof, shape)
        assert P.bits_differ(got, _torch_pool(x, b)) == 0, (prof, shape)
    for N, q, lo, hi, C in P.UPS_CASES_CPU:
        low, _, _ = P.additive_operands(prof, (N, *lo, C), C)
        fpn, _, _ = P.additive_operands(prof, (N // q, *hi, C), C, seed=1)
        assert P.bits_differ(emu_lib.upsample_add(low, fpn, q), P.upsample_add_reference(low, fpn, q)) == 0, (prof, lo, hi)
    for pos, C in P.BIAS_ACT_CASES_CPU:
        x, b, r = P.additive_operands(prof, (pos, C), C)
        for res in (None, r):
            for relu in (False, True):
                assert P.bits_differ(emu_lib.bias_act(x, b, res, relu), P.bias_act_reference(x, b, res, relu)) == 0, (prof, pos, C, relu)


@needs_emu
def test_emulated_maxpool_propagates_nan_from_every_window_position():
    """One NaN at a window centre (even, even), one at a never-centre position (odd, odd), one per edge: as max_pool2d(relu(x + b))."""
    x = np.random.default_rng(5).standard_normal((1, 9, 11, 8)).astype(f32)
    b = np.random.default_rng(6).standard_normal(8).astype(f32)
    x[0, 3, 5, 1] = np.nan
    x[0, 4, 4, 1] = np.nan
    x[0, 8, 10, 2] = np.nan
    x[0, 0, 7, 3] = np.inf
    x[0, 5, 5, 4] = -np.inf
    got, want = emu_lib.bias_relu_maxpool(x, b), _torch_pool(x, b)
    assert int(np.isnan(want[..., 1]).sum()) >= 4 and P.bits_differ(got, want) == 0
    assert P.bits_differ(P.maxpool_f32(x, b, mutant="nan_dropped"), want) > 0
