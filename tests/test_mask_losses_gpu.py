"""GPU (-m gpu): the fused mask losses (include/tf_fused.h: THE MASK LOSSES; trackformer_amd/csrc/mask_loss.h) through the C ABI, through
fused.mask_losses' autograd Function and through SetCriterion.loss_masks with criterion.set_fused_masks(True), against float64 with the
yardstick of tests/util_mask_losses.py; the fall-backs, and bit equality across calls, a side stream and a captured graph of forward +
backward."""
import pytest
import torch

from tests import util_criterion_fused as Y
from tests import util_mask_losses as M

pytestmark = pytest.mark.gpu

CANARY = -4321.5
GUARD = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from trackformer_amd import _cabi
    _cabi.lib()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _clean_state():
    from trackformer_amd import criterion
    prev = criterion._fused_masks
    criterion._fused_masks = None
    criterion.fused_mask_counts(reset=True)
    try:
        yield
    finally:
        criterion._fused_masks = prev


def _guarded(rows, cols, dev, dtype=torch.float32):
    t = torch.full((rows + GUARD, cols), float("nan"), dtype=dtype, device=dev)
    t[rows:] = CANARY
    return t


def through_operator(case, alpha=0.25, gamma=2.0, row_pair=True):
    from trackformer_amd import fused
    pm = case.pred_masks.clone().requires_grad_(True)
    out = fused.mask_losses(pm, case.tgt, case.pair_src, case.pair_tgt, alpha, gamma, case.num_boxes, row_pair=case.row_pair if row_pair else None)
    assert out.shape == (2,) and out.requires_grad
    grad, = torch.autograd.grad((out * case.G).sum(), pm)
    return {"losses": out.detach(), "grad": grad}


def check_case(case, got, alpha=0.25, gamma=2.0):
    worst = M.check(got, M.reference(case, alpha, gamma), M.fp32_formulation(case, alpha, gamma), "%s g%.1f a%.2f" % (case.what(), gamma, alpha))
    unmatched = (case.row_pair < 0).view(M.B, M.Q)
    assert bool((got["grad"][unmatched] == 0).all())
    return worst


@pytest.mark.parametrize("profile", list(M.LOGIT_PROFILES))
def test_operator_against_float64_every_shape(dev, profile):
    assert M.tiles_of(128) >= 3          # (16, 20, 128, 160): 16 partials per pair meet in the second launch
    for shape in M.SHAPES:
        case = M.Case(shape, 3, profile, "box", seed=1, device=dev)
        check_case(case, through_operator(case))


def test_operator_every_target_kind_pair_count_alpha_and_gamma(dev):
    from trackformer_amd import _cabi
    for kind in M.TARGET_KINDS:
        for n in (0, 1, 3):
            case = M.Case((5, 7, 19, 23), n, "unit", kind, seed=3, device=dev)
            got = through_operator(case, row_pair=(n != 1))              # (n == 1: the operator builds row_pair itself)
            check_case(case, got)
            if n == 0:
                assert bool((got["losses"] == 0).all()) and bool((got["grad"] == 0).all())
    # tf_msda_last_kernel is per thread and autograd runs the backward on a thread of its own: this thread launched the forward (the
    # backward kernel is checked by name in test_entries_write_everything_and_nothing_else, where this thread calls the entry)
    assert _cabi.lib().tf_msda_last_kernel() == b"mask_loss_finish_f32"
    for profile in ("unit", "wide"):
        for gamma, alpha in ((2.0, -1.0), (1.5, 0.25), (1.5, -1.0)):
            case = M.Case((13, 21, 100, 167), 3, profile, "box", seed=5, device=dev)
            check_case(case, through_operator(case, alpha, gamma), alpha, gamma)


@pytest.mark.parametrize("shape", [(5, 7, 19, 23), (3, 50, 10, 300), (16, 20, 128, 160)], ids=lambda s: "x".join(map(str, s)))
def test_entries_write_everything_and_nothing_else(dev, shape):
    """The C ABI with NaN-filled outputs and workspace and canary rows behind each."""
    from trackformer_amd import _cabi
    case = M.Case(shape, 3, "unit", "box", seed=2, device=dev)
    h, w, H, W = shape
    n, rows, T, tiles = 3, M.B * M.Q, case.tgt.shape[0], M.tiles_of(H)
    lib = _cabi.lib()
    nbytes = lib.tf_mask_loss_workspace_bytes(n, H, W)
    assert nbytes == n * tiles * 32
    sums, losses, ws = _guarded(n, 4, dev, torch.float64), _guarded(2, 1, dev), _guarded(n * tiles, 4, dev, torch.float64)
    grad = _guarded(rows, h * w, dev)
    tgt = case.tgt.view(torch.uint8)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.tf_mask_loss_fwd_f32(case.pred_masks.data_ptr(), tgt.data_ptr(), case.pair_src.data_ptr(), case.pair_tgt.data_ptr(), sums.data_ptr(),
                                  losses.data_ptr(), ws.data_ptr(), nbytes, n, rows, T, h, w, H, W, 0.25, 2.0, case.num_boxes, stream)
    _cabi.check(rc, "tf_mask_loss_fwd_f32")
    assert lib.tf_msda_last_kernel() == b"mask_loss_finish_f32"
    rc = lib.tf_mask_loss_bwd_f32(case.G.data_ptr(), case.pred_masks.data_ptr(), tgt.data_ptr(), case.pair_tgt.data_ptr(), case.row_pair.data_ptr(),
                                  sums.data_ptr(), grad.data_ptr(), n, rows, T, h, w, H, W, 0.25, 2.0, case.num_boxes, stream)
    _cabi.check(rc, "tf_mask_loss_bwd_f32")
    torch.cuda.synchronize(dev)
    assert lib.tf_msda_last_kernel() == b"mask_loss_bwd_f32"
    for name, t, k in (("sums", sums, n), ("losses", losses, 2), ("workspace", ws, n * tiles), ("grad", grad, rows)):
        assert bool((t[k:] == CANARY).all()), "wrote behind " + name
        assert not bool(torch.isnan(t[:k]).any()), name + " was not written everywhere"
    check_case(case, {"losses": losses[:2, 0], "grad": grad[:rows].view(M.B, M.Q, h, w)})
    assert torch.equal(sums[:n, 3], case.tgt[case.pair_tgt.long()].double().sum((1, 2)))       # indexed by pair_tgt; a count is exact


def test_loss_masks_with_the_switch_on(dev):
    """SetCriterion.loss_masks takes the route once, returns today's keys as 0-d tensors, within the yardstick of float64, and the
    gradient reaches pred_masks."""
    from trackformer_amd import criterion
    case = M.Case((16, 20, 128, 160), 3, "unit", "box", seed=7, device=dev)
    crit = Y.criterion_for(1, 0.25, 2.0).to(dev)
    off = crit.loss_masks({"pred_masks": case.pred_masks}, case.targets(), case.indices, case.num_boxes)
    assert criterion.fused_mask_counts() == {"own": 0, "torch": 0}
    criterion.set_fused_masks(True)
    pm = case.pred_masks.clone().requires_grad_(True)
    on = crit.loss_masks({"pred_masks": pm}, case.targets(), case.indices, case.num_boxes)
    assert criterion.fused_mask_counts() == {"own": 1, "torch": 0}
    assert list(on.keys()) == list(off.keys()) == ["loss_mask", "loss_dice"] and all(v.dim() == 0 for v in on.values())
    grad, = torch.autograd.grad(on["loss_mask"] * case.G[0] + on["loss_dice"] * case.G[1], pm)
    check_case(case, {"losses": torch.stack([on["loss_mask"], on["loss_dice"]]).detach(), "grad": grad})


def test_fall_backs_run_todays_lines_and_are_counted(dev):
    from trackformer_amd import criterion
    case = M.Case((5, 7, 19, 23), 3, "unit", "box", seed=9, device=dev)
    crit = Y.criterion_for(1, 0.25, 2.0).to(dev)
    want = crit.loss_masks({"pred_masks": case.pred_masks}, case.targets(), case.indices, case.num_boxes)
    criterion.set_fused_masks(True)

    def close(got):
        return got.keys() == want.keys() and all(abs(float(got[k]) - float(want[k])) <= 1e-5 * max(1.0, abs(float(want[k]))) for k in want)
    # fp64 predictions
    got = crit.loss_masks({"pred_masks": case.pred_masks.double()}, case.targets(), case.indices, case.num_boxes)
    assert criterion.fused_mask_counts(reset=True) == {"own": 0, "torch": 1} and close(got)
    # a non-contiguous pred_masks
    wide = torch.zeros(M.B, M.Q, 5, 14, device=dev)
    wide[..., ::2] = case.pred_masks
    view = wide[..., ::2]
    assert not view.is_contiguous()
    got = crit.loss_masks({"pred_masks": view}, case.targets(), case.indices, case.num_boxes)
    assert criterion.fused_mask_counts(reset=True) == {"own": 0, "torch": 1} and close(got)
    # targets smaller than the predictions: H < h
    big = torch.randn(M.B, M.Q, 21, 7, device=dev)
    got = crit.loss_masks({"pred_masks": big}, case.targets(), case.indices, case.num_boxes)
    assert criterion.fused_mask_counts(reset=True) == {"own": 0, "torch": 1} and all(bool(torch.isfinite(v)) for v in got.values())
    # and the plain call takes the route
    crit.loss_masks({"pred_masks": case.pred_masks}, case.targets(), case.indices, case.num_boxes)
    assert criterion.fused_mask_counts(reset=True) == {"own": 1, "torch": 0}


def test_bit_identity_across_calls_a_side_stream_and_a_captured_graph(dev):
    from trackformer_amd import fused
    case = M.Case((16, 20, 128, 160), 3, "wide", "box", seed=13, device=dev)
    first = through_operator(case)

    def same(got, what):
        torch.cuda.synchronize(dev)
        for k in M.OUTPUTS:
            assert torch.equal(got[k].view(torch.int32), first[k].view(torch.int32)), (what, k)

    same(through_operator(case), "second call")
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = through_operator(case)
        for _ in range(2):                                   # (the warm-up a capture of autograd wants, on the side stream)
            through_operator(case)
    torch.cuda.current_stream(dev).wait_stream(side)
    same(got, "side stream")
    # forward + backward captured: one chain of three kernels, no branches
    pm = case.pred_masks.clone().requires_grad_(True)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(graph):
        out = fused.mask_losses(pm, case.tgt, case.pair_src, case.pair_tgt, 0.25, 2.0, case.num_boxes, row_pair=case.row_pair)
        grad, = torch.autograd.grad((out * case.G).sum(), pm)
    for _ in range(2):
        out.detach().zero_()
        grad.zero_()
        graph.replay()
        same({"losses": out.detach(), "grad": grad}, "graph replay")
