"""GPU: the post-processing and pooling kernels of trackformer_amd/csrc/fused_ops.hip against the float64 yardsticks of
tests/util_postproc_numerics.py -- the decision rule for the label map and the post-process labels (no share of pixels is excused),
bit equality with float64-rounded-once for the additive kernels, the non-finite contract of include/tf_fused.h element for element with
the torch chains on the device, and the wrappers' refusals.  Every case prints one DECISION / EXCESS line (pytest -s is the record)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import util_postproc_numerics as P

pytestmark = pytest.mark.gpu
f32 = np.float32
BAD_DIMS = -2


def _ids(v):
    return str(v).replace(" ", "")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fused():
    from trackformer_amd import fused as f
    return f


def _nhwc(a, dev):
    """numpy [N, H, W, C] -> channels_last NCHW tensor on the device (the same storage)."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).permute(0, 3, 1, 2)


def _back(t):
    """channels_last NCHW tensor -> numpy [N, H, W, C]."""
    return t.permute(0, 2, 3, 1).contiguous().cpu().numpy()


# ---- label map ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prof", P.LABEL_PROFILES)
@pytest.mark.parametrize("case", P.LABEL_CASES_GPU, ids=_ids)
def test_label_map_obeys_the_decision_rule(dev, fused, case, prof):
    lw, pad, img, out, n = case
    x = torch.from_numpy(P.label_logits(prof, n, *lw)).to(dev)
    thr = P.threshold_of(prof)
    for kind in (("holes",) if n >= 100 else ("identity", "holes")):
        order = P.order_of(n, kind)
        got = fused.mask_label_map(x, order, pad, img, out, thr)
        assert got is not None and got.dtype == torch.int16 and tuple(got.shape) == tuple(out)
        v = P.label_check(got, x, order, pad, img, out, thr)
        # the ambiguous share is a property of the float64 reference alone (it does not depend on `got`): the rule is not vacuous here
        assert v.ambiguous <= P.AMBIG_CAP, (prof, case, v.ambiguous)
        print("DECISION label map %-12s %s %s: %s" % (prof, _ids(case), kind, v))
        assert v.ok, (prof, case, str(v))
        if prof == "neg":
            assert bool((got == -1).all())
        if kind == "holes" and n > 1:
            assert not bool((got == 0).any())                             # track 0 has no mask


def _run_label(fused, dev):
    def run(x, order, pad, img, out, thr):
        got = fused.mask_label_map(torch.from_numpy(np.ascontiguousarray(x, dtype=f32)).to(dev), list(order), pad, img, out, thr)
        assert got is not None
        return got.cpu().numpy()
    return run


def test_label_map_exact_cases(dev, fused):
    """Zero logits (0.5 is not > 0.5), subnormal logits, saturated rows, equal rows, thresholds 0.3 and 0.0, order all -1."""
    P.check_exact_label_cases(_run_label(fused, dev))


def test_label_map_non_finite_contract(dev, fused):
    """NaN / +inf / -inf in the first and in a later track, at the clamped corner (weight exactly 0: 0 * inf) and in the last row /
    column: the pixel is -1 wherever a probability is NaN, as the chain on the device has it; the rest within the rule."""
    run = _run_label(fused, dev)
    P.check_nan_label_contract(run)
    for kind in ("nan", "+inf", "-inf"):
        x, order, pad, img, out = P.nan_label_case(kind)
        want = P.torch_label_chain(torch.from_numpy(x).to(dev), order, pad, img, out, 0.5).cpu().numpy()
        got = run(x, order, pad, img, out, 0.5)
        v = P.label_check(got, torch.from_numpy(x).to(dev), order, pad, img, out, 0.5)
        differ = got != want
        print("DECISION label map %s against the chain on the device: %d pixels differ (ambiguous share %.2e)" % (kind, int(differ.sum()), v.ambiguous))
        assert int(differ.sum()) <= int(round(v.ambiguous * got.size))


def test_label_map_track_limit(dev, fused):
    """32767 tracks (the int16 label's limit) over four rows on a tiny map: the first track of the winning row; 32768 decline."""
    from trackformer_amd import _cabi
    lw, pad, img, out = (3, 4), (12, 16), (11, 15), (9, 14)
    x = P.label_logits("unit", 4, *lw, seed=7)
    rng = np.random.default_rng(0)
    order = rng.integers(0, 4, 32767).tolist()
    order[:3] = [-1, 2, 2]
    xd = torch.from_numpy(x).to(dev)
    four = P.label_check(None, xd, [0, 1, 2, 3], pad, img, out, 0.5)
    assert four.ambiguous == 0
    first = np.array([order.index(r) for r in range(4)] + [-1])
    want = first[four.decision.cpu().numpy()]
    got = fused.mask_label_map(xd, order, pad, img, out)
    assert got is not None and np.array_equal(got.cpu().numpy(), want.astype(np.int16))
    assert fused.mask_label_map(xd, order + [1], pad, img, out) is None
    big = torch.zeros(32768, dtype=torch.int32, device=dev)
    lab = torch.empty(out, dtype=torch.int16, device=dev)
    rc = _cabi.lib().tf_mask_label_map_f32(xd.data_ptr(), big.data_ptr(), lab.data_ptr(), 32768, 3, 4, 12, 16, 11, 15, 9, 14, 0.5, 0)
    assert rc == BAD_DIMS


# ---- post-processing ----------------------------------------------------------------------------------------------------------------
def _torch_post(logits, boxes, ih, iw, clip):
    from trackformer_amd.box_ops import clip_boxes_to_image
    from trackformer_amd.deformable_detr import DeformablePostProcess
    res = DeformablePostProcess()({'pred_logits': logits[None], 'pred_boxes': boxes[None]}, torch.tensor([[ih, iw]], device=logits.device))[0]
    bx = clip_boxes_to_image(res['boxes'], (ih, iw)) if clip else res['boxes']
    return torch.cat([bx, res['scores'][:, None], res['labels'][:, None].float()], 1).cpu().numpy()


@pytest.mark.parametrize("C", P.POST_C)
@pytest.mark.parametrize("Q", P.POST_Q)
def test_postprocess_obeys_the_rules(dev, fused, Q, C):
    """Every profile at every (Q, C); every image side with clip on and off."""
    for prof in P.POST_PROFILES + ["non_finite", "subnormal", "saturated"]:
        logits, boxes = P.post_inputs(prof, Q, C)
        if prof in P.POST_PROFILES:
            assert P.post_ambiguous_share(logits) <= P.AMBIG_CAP, (prof, Q, C)     # the reference alone: the rule is not vacuous here
        ld, bd = torch.from_numpy(logits).to(dev), torch.from_numpy(boxes).to(dev)
        worst = None
        for ih, iw in P.POST_SIDES:
            for clip in (True, False):
                got = fused.postprocess_pack(ld, bd, ih, iw, clip)
                assert got is not None and tuple(got.shape) == (Q, 6)
                got = got.cpu().numpy()
                ref = _torch_post(ld, bd, ih, iw, clip)
                v = P.post_check(got, logits, boxes, ih, iw, clip, fp32_scores=ref[:, 4])
                assert v.ok, (prof, Q, C, ih, iw, clip, str(v))
                # element for element with the chain on the device: boxes bit for bit, NaN scores, and the label of a NaN score (several
                # NaN classes in one query: the first of them, as torch.max on the device); a label may differ from the chain's on an
                # ambiguous query only
                assert P.bits_differ(got[:, :4], ref[:, :4]) == 0
                nan = np.isnan(ref[:, 4])
                assert np.array_equal(np.isnan(got[:, 4]), nan) and np.array_equal(got[nan, 5], ref[nan, 5])
                off_chain = ~nan & (got[:, 5] != ref[:, 5])
                assert bool(v.ambiguous_mask[off_chain].all()), (prof, Q, C, int(off_chain.sum()))
                if prof in ("subnormal", "saturated"):
                    assert (got[:, 5] == 0).all() and (got[:, 4] == (0.5 if prof == "subnormal" else 1.0)).all()
                if worst is None or v.score_ratio > worst[0]:
                    worst = (v.score_ratio, "%dx%d clip %s: %s | labels off the chain on the device %d" % (ih, iw, clip, v, int(off_chain.sum())))
        print("EXCESS post-process %-10s Q %d C %d: %s" % (prof, Q, C, worst[1]))


def test_postprocess_non_finite_boxes_under_clip(dev, fused):
    """include/tf_fused.h: with clip the kernel clamps by fminf(fmaxf(v, 0), side), which turns a NaN coordinate into 0 and +-inf into the
    nearer bound; without clip the coordinates pass through.  (torch.clamp would keep the NaN: boxes are expected to be finite.)"""
    logits, boxes = P.post_inputs("unit", 64, 4)
    boxes[3, 0], boxes[5, 3], boxes[7, 2], boxes[9, 1] = np.nan, np.nan, np.inf, -np.inf
    ld, bd = torch.from_numpy(logits).to(dev), torch.from_numpy(boxes).to(dev)
    for clip in (True, False):
        got = fused.postprocess_pack(ld, bd, 375, 1242, clip).cpu().numpy()
        assert P.bits_differ(got[:, :4], P.postprocess_boxes_f32(boxes, 375, 1242, clip)) == 0
        assert np.array_equal(got[:, 5], P.postprocess_f32(logits, boxes, 375, 1242, clip)[:, 5]) and np.isfinite(got[:, 4]).all()   # (the logits' side is untouched)
    got = fused.postprocess_pack(ld, bd, 375, 1242, True).cpu().numpy()
    assert np.isfinite(got[:, :4]).all() and got[3, 0] == 0 and got[3, 2] == 0 and got[5, 1] == 0 and got[5, 3] == 0


def test_postprocess_declines_a_misaligned_boxes_view(dev, fused):
    from trackformer_amd import _cabi
    logits = torch.randn(16, 4, device=dev)
    store = torch.rand(16 * 4 + 1, device=dev)
    boxes = store[1:].view(16, 4)
    assert boxes.data_ptr() % 16 != 0 and boxes.is_contiguous()
    assert fused.postprocess_pack(logits, boxes, 100, 100, True) is None
    out = torch.empty(16, 6, device=dev)
    assert _cabi.lib().tf_postprocess_pack_f32(logits.data_ptr(), boxes.data_ptr(), out.data_ptr(), 16, 4, 100.0, 100.0, 1, 0) == BAD_DIMS


# ---- max-pool -----------------------------------------------------------------------------------------------------------------------
def _torch_pool(xd, bd):
    return F.max_pool2d(torch.relu(xd + bd.view(1, -1, 1, 1)), 3, 2, 1)


@pytest.mark.parametrize("prof", P.ADD_PROFILES)
@pytest.mark.parametrize("shape", P.POOL_SHAPES_GPU, ids=_ids)
def test_maxpool_equals_float64_rounded_once(dev, fused, shape, prof):
    x, b, _ = P.additive_operands(prof, shape, shape[3], pool=True)
    xd, bd = _nhwc(x, dev), torch.from_numpy(b).to(dev)
    got = fused.bias_relu_maxpool(xd, bd)
    assert got is not None and got.is_contiguous(memory_format=torch.channels_last)
    got = _back(got)
    off_ref = P.bits_differ(got, P.maxpool_reference(x, b))
    off_torch, signs = P.against_device_chain(got, _back(_torch_pool(xd, bd)), prof)
    print("EXCESS maxpool %-12s %s: elements off float64-rounded-once %d, off the torch chain on the device %d (+ %d zeros of the other sign)"
          % (prof, _ids(shape), off_ref, off_torch, signs))
    assert off_ref == 0 and off_torch == 0


def test_maxpool_non_finite_contract(dev, fused):
    """A NaN at a window centre (even, even), at a never-centre position (odd, odd), in the last row / column, +-inf: element for element
    with max_pool2d(relu(x + b)) on the device; -inf under a shift of +inf is NaN."""
    x = np.random.default_rng(5).standard_normal((2, 9, 11, 8)).astype(f32)
    b = np.random.default_rng(6).standard_normal(8).astype(f32)
    x[0, 3, 5, 1] = np.nan
    x[0, 4, 4, 1] = np.nan
    x[1, 8, 10, 2] = np.nan
    x[0, 0, 7, 3] = np.inf
    x[1, 5, 5, 4] = -np.inf
    x[1, 2, 3, 5] = -np.inf
    b[5] = np.inf
    xd, bd = _nhwc(x, dev), torch.from_numpy(b).to(dev)
    got, want = _back(fused.bias_relu_maxpool(xd, bd)), _back(_torch_pool(xd, bd))
    assert int(np.isnan(want).sum()) >= 6 and P.bits_differ(got, want) == 0
    assert P.bits_differ(got, P.maxpool_reference(x, b)) == 0
    assert P.bits_differ(P.maxpool_f32(x, b, mutant="nan_dropped"), want) > 0


def test_maxpool_refuses_2_to_the_31_outputs(dev):
    """The size check returns before any launch: small valid buffers, large dimensions."""
    from trackformer_amd import _cabi
    buf = torch.zeros(1024, device=dev)
    rc = _cabi.lib().tf_bias_relu_maxpool_f32(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 65536, 2048, 2048, 64, 0)    # 2^40 quads
    assert rc == BAD_DIMS
    rc = _cabi.lib().tf_bias_relu_maxpool_f32(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 32768, 511, 511, 4, 0)       # 2^31 exactly
    assert rc == BAD_DIMS
    rc = _cabi.lib().tf_bias_relu_maxpool_f32(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 32768, 512, 511, 4, 0)       # 2^31 (H even)
    assert rc == BAD_DIMS
    rc = _cabi.lib().tf_bias_relu_maxpool_f32(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 4, 4, 6, 0)    # C % 4
    assert rc == BAD_DIMS
    torch.cuda.synchronize()


# ---- up-sample + add ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prof", P.ADD_PROFILES)
@pytest.mark.parametrize("case", P.UPS_CASES_GPU, ids=_ids)
def test_upsample_add_equals_float64_rounded_once(dev, fused, case, prof):
    from trackformer_amd.detr_segmentation import MaskHeadSmallConv
    N, q, lo, hi, C = case
    low, _, _ = P.additive_operands(prof, (N, *lo, C), C)
    fpn, _, _ = P.additive_operands(prof, (N // q, *hi, C), C, seed=1)
    ld, fd = _nhwc(low, dev), _nhwc(fpn, dev)
    got = fused.upsample_add(ld, fd, q)
    assert got is not None and got.is_contiguous(memory_format=torch.channels_last)
    got = _back(got)
    off_ref = P.bits_differ(got, P.upsample_add_reference(low, fpn, q))
    off_torch, signs = P.against_device_chain(got, _back(MaskHeadSmallConv._merge(ld, fd, q)), prof)
    print("EXCESS upsample_add %-12s %s: elements off float64-rounded-once %d, off the torch chain on the device %d (+ %d zeros of the other sign)"
          % (prof, _ids(case), off_ref, off_torch, signs))
    assert off_ref == 0 and off_torch == 0


# ---- bias_act ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prof", P.ADD_PROFILES)
@pytest.mark.parametrize("case", P.BIAS_ACT_CASES_GPU, ids=_ids)
def test_bias_act_equals_float64_rounded_twice(dev, fused, case, prof):
    """All four template variants; the table holds sizes whose last iteration has a second element for some threads only, channel-quad
    counts that do and do not divide the grid stride, and more than two grid strides."""
    pos, C = case
    x, b, r = P.additive_operands(prof, (pos, C), C)
    bd = torch.from_numpy(b).to(dev)
    rd = _nhwc(r.reshape(1, pos, 1, C), dev)
    off = []
    for res in (False, True):
        for relu in (False, True):
            xd = _nhwc(x.reshape(1, pos, 1, C), dev).clone(memory_format=torch.preserve_format)
            chain = xd + bd.view(1, -1, 1, 1)
            if res:
                chain = chain + rd
            chain = torch.relu(chain) if relu else chain
            y = fused.bias_act_(xd, bd, rd if res else None, relu)
            assert y is xd
            got = _back(xd).reshape(pos, C)
            o_ref = P.bits_differ(got, P.bias_act_reference(x, b, r if res else None, relu))
            o_torch, signs = P.against_device_chain(got, _back(chain).reshape(pos, C), prof)
            off.append((o_ref, o_torch, signs))
    print("EXCESS bias_act %-12s %s: (off float64-rounded, off the torch chain on the device, zeros of the other sign) per variant %s" % (prof, _ids(case), off))
    assert all(o[:2] == (0, 0) for o in off)


def test_bias_act_declines_a_residual_that_is_x(dev, fused):
    """The kernel's pointers are restrict-qualified: residual == x is refused by the wrapper (None) and by the C ABI (before any launch)."""
    from trackformer_amd import _cabi
    x = torch.randn(1, 8, 5, 5, device=dev).contiguous(memory_format=torch.channels_last)
    b = torch.randn(8, device=dev)
    keep = x.clone(memory_format=torch.preserve_format)
    assert fused.bias_act_(x, b, x, True) is None
    assert _cabi.lib().tf_bias_act_f32(x.data_ptr(), b.data_ptr(), x.data_ptr(), x.numel(), 8, 1, 0) == BAD_DIMS
    torch.cuda.synchronize()
    assert torch.equal(x, keep)


# ---- wrapper contracts ----------------------------------------------------------------------------------------------------------------
def test_wrappers_decline_what_the_kernels_cannot_take(dev, fused):
    cl = torch.channels_last
    x = torch.randn(2, 8, 6, 6, device=dev).contiguous(memory_format=cl)
    b = torch.randn(8, device=dev)
    others = [torch.device("cuda:1")] if torch.cuda.device_count() > 1 else []
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        assert fused.bias_act_(x.to(dt), b.to(dt)) is None
        assert fused.bias_relu_maxpool(x.to(dt), b.to(dt)) is None
        assert fused.upsample_add(x.to(dt), x.to(dt), 1) is None
        assert fused.postprocess_pack(torch.randn(8, 4, device=dev, dtype=dt), torch.rand(8, 4, device=dev, dtype=dt), 10, 10, True) is None
        assert fused.mask_label_map(torch.randn(2, 4, 4, device=dev, dtype=dt), [0, 1], (8, 8), (8, 8), (8, 8)) is None
    # CPU tensors, parameters on the CPU (and on a second device)
    xc, bc = x.cpu().contiguous(memory_format=cl), b.cpu()
    assert fused.bias_act_(xc, bc) is None and fused.bias_relu_maxpool(xc, bc) is None and fused.upsample_add(xc, xc, 1) is None
    assert fused.postprocess_pack(torch.randn(8, 4), torch.rand(8, 4), 10, 10, True) is None
    assert fused.mask_label_map(torch.randn(2, 4, 4), [0, 1], (8, 8), (8, 8), (8, 8)) is None
    for where in [torch.device("cpu")] + others:
        assert fused.bias_act_(x.clone(memory_format=torch.preserve_format), b.to(where)) is None
        assert fused.bias_relu_maxpool(x, b.to(where)) is None
        assert fused.upsample_add(x, x.to(where), 1) is None
        assert fused.postprocess_pack(torch.randn(8, 4, device=dev), torch.rand(8, 4).to(where), 10, 10, True) is None
    # NCHW storage, non-contiguous views
    xn = torch.randn(2, 8, 6, 6, device=dev)
    assert fused.bias_act_(xn, b) is None and fused.bias_relu_maxpool(xn, b) is None and fused.upsample_add(xn, xn, 1) is None
    assert fused.upsample_add(x, xn, 1) is None
    assert fused.bias_act_(x[:, :, ::2], b) is None and fused.bias_relu_maxpool(x[:, :, :, 1:], b) is None
    assert fused.postprocess_pack(torch.randn(8, 8, device=dev)[:, ::2], torch.rand(8, 4, device=dev), 10, 10, True) is None
    assert fused.postprocess_pack(torch.randn(8, 4, device=dev), torch.rand(8, 8, device=dev)[:, :4], 10, 10, True) is None
    assert fused.mask_label_map(torch.randn(2, 4, 8, device=dev)[:, :, ::2], [0, 1], (8, 8), (8, 8), (8, 8)) is None
    # C % 4 != 0
    x6 = torch.randn(1, 6, 4, 4, device=dev).contiguous(memory_format=cl)
    b6 = torch.zeros(6, device=dev)
    assert fused.bias_act_(x6, b6) is None and fused.bias_relu_maxpool(x6, b6) is None and fused.upsample_add(x6, x6, 1) is None
    # img > pad, a row index >= n, no tracks, too many
    lg = torch.randn(2, 4, 4, device=dev)
    assert fused.mask_label_map(lg, [0, 1], (8, 8), (9, 8), (8, 8)) is None and fused.mask_label_map(lg, [0, 1], (8, 8), (8, 9), (8, 8)) is None
    assert fused.mask_label_map(lg, [0, 2], (8, 8), (8, 8), (8, 8)) is None and fused.mask_label_map(lg, [], (8, 8), (8, 8), (8, 8)) is None
    assert fused.mask_label_map(lg, [0, 1], (8, 8), (8, 8), (8, 8)) is not None
    # the switch turns BOTH post-processing kernels off
    lq, bq = torch.randn(8, 4, device=dev), torch.rand(8, 4, device=dev)
    assert fused.postprocess_pack(lq, bq, 10, 10, True) is not None
    prev = fused.set_postprocess_fused(False)
    try:
        assert fused.postprocess_pack(lq, bq, 10, 10, True) is None
        assert fused.mask_label_map(lg, [0, 1], (8, 8), (8, 8), (8, 8)) is None
    finally:
        fused.set_postprocess_fused(prev)
    assert fused.postprocess_pack(lq, bq, 10, 10, True) is not None
    torch.cuda.synchronize()
