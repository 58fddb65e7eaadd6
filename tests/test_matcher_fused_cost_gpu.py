"""GPU (-m gpu): the matching-cost kernel (include/tf_fused.h: tf_match_cost_f32; trackformer_amd/csrc/criterion.h) against float64 with
the yardstick of tests/util_criterion_fused.py, and HungarianMatcher.match_many with matcher.set_fused_cost(True): on fixtures whose
float64 assignment survives every perturbation of the cost by its own bound (asserted here for every seed, on the CPU), the switch must
return exactly float64's pairs, with and without track-query constraints; with the switch off match_many returns what it returns
today."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from tests import util_criterion_fused as Y
from tests.test_criterion_fused_cpu import COST_SEEDS, COST_W, cost_fixture

pytestmark = pytest.mark.gpu

CANARY = -4321.5
GUARD = 3
B, Q = 2, 40


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from trackformer_amd import _cabi
    _cabi.lib()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _clean_state():
    from trackformer_amd import matcher
    prev = matcher._fused_cost
    matcher._fused_cost = None
    matcher.fused_cost_counts(reset=True)
    try:
        yield
    finally:
        matcher._fused_cost = prev


def k_cost(lg, bx, ids, tb, w, alpha, gamma):
    """tf_match_cost_f32 through the C ABI: the matrix starts as NaN, canary rows behind it are checked."""
    from trackformer_amd import _cabi
    R, C = lg.shape
    T = ids.numel()
    buf = torch.full((R + GUARD, T), float("nan"), dtype=torch.float32, device=lg.device)
    buf[R:] = CANARY
    rc = _cabi.lib().tf_match_cost_f32(lg.data_ptr(), bx.data_ptr(), ids.data_ptr(), tb.data_ptr(), buf.data_ptr(), R, C, T, w[0], w[1], w[2],
                                       alpha, gamma, torch.cuda.current_stream(lg.device).cuda_stream)
    _cabi.check(rc, "tf_match_cost_f32")
    torch.cuda.synchronize(lg.device)
    assert _cabi.lib().tf_msda_last_kernel() == b"match_cost_f32"
    assert bool((buf[R:] == CANARY).all()), "wrote behind the cost matrix"
    return buf[:R]


# (257, ., 3): 771 entries, a fourth workgroup of three work-items; (600, 91, 10): the 91-class, 300-query shape of two images
@pytest.mark.parametrize("R,C,T", [(1, 1, 1), (7, 2, 5), (257, 19, 3), (600, 91, 10), (1000, 1, 12)])
@pytest.mark.parametrize("gamma", [2.0, 1.5])
def test_cost_kernel_against_float64(dev, R, C, T, gamma):
    for profile in Y.LOGIT_PROFILES:
        case = Y.Case(1, 1, R, C, [T], profile, "overlapping", seed=R + T)
        lg, bx = case.logits.view(R, C), case.boxes.view(R, 4)
        got = k_cost(lg.to(dev), bx.to(dev), case.labels.to(dev), case.tboxes.to(dev), COST_W, 0.25, gamma)
        ref = Y.cost_reference(lg, bx, case.labels, case.tboxes, *COST_W, 0.25, gamma)
        Y.check_one("cost", got.cpu(), ref, Y.cost_fp32(lg, bx, case.labels, case.tboxes, *COST_W, 0.25, gamma),
                    "%s R%d C%d T%d g%.1f" % (profile, R, C, T, gamma))


def _problem(seed, dev, track_queries):
    """(outputs_list of 3 prediction sets, targets, float64 pairs per set, the matcher) on the fixture of `seed`; the sets are the
    fixture's predictions and two permutations of them (each set's cost is a row permutation of the fixture's)."""
    from trackformer_amd.matcher import HungarianMatcher
    lg, bx, ids, tb, sizes = cost_fixture(seed)
    ref = Y.cost_reference(lg, bx, ids, tb, *COST_W, 0.25, 2.0)
    _, same = Y.perturbed_assignments(ref, sizes, B, Q, seed)
    assert same, "fixture %d: the float64 assignment does not survive a perturbation by the bound" % seed
    g = torch.Generator().manual_seed(seed)
    perms = [torch.arange(Q)] + [torch.randperm(Q, generator=g) for _ in range(2)]
    outputs_list = [{"pred_logits": lg.view(B, Q, -1)[:, p].to(dev), "pred_boxes": bx.view(B, Q, 4)[:, p].to(dev)} for p in perms]
    targets, o = [], 0
    for n in sizes:
        targets.append({"labels": ids[o:o + n].to(dev), "boxes": tb[o:o + n].to(dev)})
        o += n
    if track_queries:   # image 0: queries 0 and 1 are track queries, 0 pinned to target 2, 1 a false positive
        mask = torch.zeros(Q, dtype=torch.bool)
        mask[:2] = True
        fal = torch.zeros(Q, dtype=torch.bool)
        fal[1] = True
        targets[0].update(track_query_match_ids=torch.tensor([2]), track_queries_mask=mask.to(dev), track_queries_fal_pos_mask=fal.to(dev))
    mt = HungarianMatcher(*COST_W, focal_loss=True, focal_alpha=0.25, focal_gamma=2.0)
    # float64's pairs: the matcher's own host side on the float64 cost of every set
    want = []
    for p in perms:
        c = Y.cost_reference(lg.view(B, Q, -1)[:, p].reshape(B * Q, -1), bx.view(B, Q, 4)[:, p].reshape(B * Q, 4), ids, tb, *COST_W, 0.25, 2.0)
        want += mt._assign(c.v.view(1, B, Q, -1).clone(), targets, 1, Q)
    return outputs_list, targets, want, mt


def _lists(result):
    return [[(i.tolist(), j.tolist()) for i, j in per_set] for per_set in result]


@pytest.mark.parametrize("track_queries", [False, True], ids=["plain", "track_queries"])
@pytest.mark.parametrize("seed", COST_SEEDS)
def test_match_many_with_the_switch_returns_float64s_pairs(dev, seed, track_queries):
    from trackformer_amd import matcher
    outputs_list, targets, want, mt = _problem(seed, dev, track_queries)
    today = mt.match_many(outputs_list, targets)
    assert matcher.fused_cost_counts() == {"own": 0, "torch": 0}
    assert _lists(today) == _lists(want)                 # (today's chain on these fixtures: float64's pairs as well)
    matcher.set_fused_cost(True)
    got = mt.match_many(outputs_list, targets)
    assert matcher.fused_cost_counts() == {"own": 1, "torch": 0}
    assert _lists(got) == _lists(want)
    assert all(i.dtype == torch.int64 and j.dtype == torch.int64 for per_set in got for i, j in per_set)
    if track_queries:
        src, tgt = got[0][0]
        assert (0, 2) in list(zip(src.tolist(), tgt.tolist())) and 1 not in src.tolist()
    matcher.set_fused_cost(False)
    again = mt.match_many(outputs_list, targets)
    assert matcher.fused_cost_counts() == {"own": 1, "torch": 0} and _lists(again) == _lists(today)


def test_declines_keep_the_torch_chain(dev):
    """The softmax (plain DETR) cost and float64 predictions keep today's chain, counted under "torch"."""
    from trackformer_amd import matcher
    from trackformer_amd.matcher import HungarianMatcher
    outputs_list, targets, _, mt = _problem(COST_SEEDS[0], dev, False)
    soft = HungarianMatcher(*COST_W, focal_loss=False)
    want_soft, want_64 = soft.match_many(outputs_list, targets), None
    out64 = [{k: v.double() for k, v in o.items()} for o in outputs_list]
    tgt64 = [{k: (v.double() if v.is_floating_point() else v) for k, v in t.items()} for t in targets]
    want_64 = mt.match_many(out64, tgt64)
    matcher.set_fused_cost(True)
    assert _lists(soft.match_many(outputs_list, targets)) == _lists(want_soft)
    assert _lists(mt.match_many(out64, tgt64)) == _lists(want_64)
    assert matcher.fused_cost_counts() == {"own": 0, "torch": 2}
    empty = [{"labels": t["labels"][:0], "boxes": t["boxes"][:0]} for t in targets]      # T == 0: an empty cost, nothing launched
    got = mt.match_many(outputs_list, empty)
    assert all(len(i) == 0 and len(j) == 0 for per_set in got for i, j in per_set)
