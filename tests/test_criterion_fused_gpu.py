"""GPU (-m gpu): the fused set criterion (include/tf_fused.h: THE SET CRITERION AND THE MATCHING COST; trackformer_amd/csrc/criterion.h)
through the C ABI, through fused.set_criterion's autograd Function and through SetCriterion.forward with criterion.set_fused(True),
against float64 with the yardstick of tests/util_criterion_fused.py and against SetCriterion._layers_at_once on the device; the
decline cases, bit equality across calls / streams / a captured graph / a busy neighbour stream, and a NaN logit."""
import pytest
import torch

from tests import util_criterion_fused as Y

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
    from trackformer_amd import criterion, matcher
    prev = criterion._fused, matcher._fused_cost
    criterion._fused = matcher._fused_cost = None
    criterion.fused_counts(reset=True)
    matcher.fused_cost_counts(reset=True)
    try:
        yield
    finally:
        criterion._fused, matcher._fused_cost = prev


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _guarded(rows, cols, dev):
    """[rows + GUARD, cols]: NaN in the rows the entry writes, canaries behind them."""
    t = torch.full((rows + GUARD, cols), float("nan"), dtype=torch.float32, device=dev)
    t[rows:] = CANARY
    return t


class Entries:
    """The buffers of one forward + backward call of the two criterion entries."""

    def __init__(self, case, alpha, gamma):
        self.case, self.alpha, self.gamma = case, alpha, gamma
        d = case.logits.device
        self.rows = case.L * case.B * case.Q
        self.losses, self.card, self.cerr = _guarded(case.L, 3, d), _guarded(case.L, 1, d), _guarded(1, 1, d)
        self.gl, self.gb = _guarded(self.rows, case.C, d), _guarded(self.rows, 4, d)

    def __call__(self, logits=None):
        from trackformer_amd import _cabi
        c = self.case
        lg = c.logits if logits is None else logits
        lab, tb = (c.labels, c.tboxes) if c.T else (None, None)
        lib = _cabi.lib()
        rc = lib.tf_set_criterion_fwd_f32(lg.data_ptr(), c.boxes.data_ptr(), c.tgt_of.data_ptr(), _ptr(lab), _ptr(tb), c.tgt_len.data_ptr(),
                                          self.losses.data_ptr(), self.card.data_ptr(), self.cerr.data_ptr(), c.L, c.B, c.Q, c.C, c.T,
                                          self.alpha, self.gamma, c.num_boxes, _stream(lg.device))
        _cabi.check(rc, "tf_set_criterion_fwd_f32")
        rc = lib.tf_set_criterion_bwd_f32(c.G.data_ptr(), lg.data_ptr(), c.boxes.data_ptr(), c.tgt_of.data_ptr(), _ptr(lab), _ptr(tb),
                                          self.gl.data_ptr(), self.gb.data_ptr(), c.L, c.B, c.Q, c.C, c.T, self.alpha, self.gamma,
                                          c.num_boxes, _stream(lg.device))
        _cabi.check(rc, "tf_set_criterion_bwd_f32")
        return self

    def outputs(self):
        c = self.case
        return {"losses": self.losses[:c.L], "card": self.card[:c.L, 0], "class_error": self.cerr[:1, 0],
                "grad_logits": self.gl[:self.rows].view(c.L, c.B, c.Q, c.C), "grad_boxes": self.gb[:self.rows].view(c.L, c.B, c.Q, 4)}

    def assert_canaries(self):
        c = self.case
        for name, t, n in (("losses", self.losses, c.L), ("card", self.card, c.L), ("class_error", self.cerr, 1), ("grad_logits", self.gl, self.rows),
                           ("grad_boxes", self.gb, self.rows)):
            assert bool((t[n:] == CANARY).all()), "wrote behind " + name


def _what(case, alpha, gamma):
    return "%s / %s L%d B%d Q%d C%d %r g%.1f a%.2f" % (case.logit_profile, case.box_profile, case.L, case.B, case.Q, case.C, case.sizes, gamma,
                                                     alpha)


def check_case(case, got, alpha, gamma, fp32=None):
    box_margin, logit_margin = case.margins()
    assert box_margin >= 1.0 and logit_margin >= 1.0, (box_margin, logit_margin)
    if fp32 is None and any(case.sizes):
        fp32 = Y.fp32_formulation(case, alpha, gamma)
    return Y.check(got, Y.reference(case, alpha, gamma), fp32, _what(case, alpha, gamma))


# (.., 257, ..): a second pass of the workgroup's 256 threads with one row in it; (6, 2, 300, 91): the 91-class, 300-query shape; T = 0; an
# image without targets; more targets than queries
SHAPES = [(1, 1, 1, 1, [1], 2.0, 0.25), (2, 1, 1, 19, [5], 1.5, -1.0), (3, 2, 7, 1, [5, 0], 1.5, 0.25), (6, 2, 40, 19, [0, 0], 2.0, -1.0),
          (3, 1, 257, 1, [5], 2.0, 0.25), (1, 3, 257, 2, [1, 0, 5], 1.5, -1.0), (6, 2, 300, 91, [5, 1], 2.0, 0.25)]


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_entries_against_float64(dev, i):
    from trackformer_amd import _cabi
    L, B, Q, C, per, gamma, alpha = SHAPES[i]
    case = Y.Case(L, B, Q, C, per, seed=i, device=dev)
    e = Entries(case, alpha, gamma)()
    torch.cuda.synchronize(dev)
    assert _cabi.lib().tf_msda_last_kernel() == b"set_criterion_bwd_f32"
    e.assert_canaries()
    check_case(case, e.outputs(), alpha, gamma)


@pytest.mark.parametrize("logit_profile", list(Y.LOGIT_PROFILES))
def test_every_profile_pair_against_float64(dev, logit_profile):
    for j, box_profile in enumerate(Y.BOX_PROFILES):
        gamma, alpha = [(2.0, 0.25), (1.5, 0.25), (2.0, -1.0), (1.5, -1.0)][j]
        case = Y.Case(3, 2, 40, 19, [5, 1], logit_profile, box_profile, seed=21, device=dev)
        e = Entries(case, alpha, gamma)()
        torch.cuda.synchronize(dev)
        e.assert_canaries()
        check_case(case, e.outputs(), alpha, gamma)


def _layers_at_once_on_device(case, alpha, gamma):
    """SetCriterion._layers_at_once and autograd through it, fp32 on the device -> the entries' five outputs."""
    crit = Y.criterion_for(case.C, alpha, gamma).to(case.logits.device)
    lg, bx = case.logits.clone().requires_grad_(True), case.boxes.clone().requires_grad_(True)
    out = crit._layers_at_once(case.layer_outputs(lg, bx), case.targets(), case.all_indices, case.num_boxes)
    losses, card = Y.dict_to_tensors(out, case.L)
    gl, gb = torch.autograd.grad((losses * case.G).sum(), (lg, bx))
    return {"losses": losses.detach().cpu(), "card": card.cpu(), "class_error": out["class_error"].reshape(1).cpu(), "grad_logits": gl.cpu(),
            "grad_boxes": gb.cpu()}


@pytest.mark.parametrize("shape", [(6, 2, 40, 1, [5, 1]), (3, 2, 300, 91, [5, 5])])
def test_autograd_function_against_float64_and_layers_at_once(dev, shape):
    """Values and torch.autograd.grad of a random weighted sum of the losses through fused.set_criterion."""
    from trackformer_amd import fused
    L, B, Q, C, per = shape
    alpha, gamma = 0.25, 2.0
    case = Y.Case(L, B, Q, C, per, seed=5, device=dev)
    lg, bx = case.logits.clone().requires_grad_(True), case.boxes.clone().requires_grad_(True)
    losses, card, cerr = fused.set_criterion(lg, bx, case.tgt_of, case.labels, case.tboxes, case.tgt_len, alpha, gamma, case.num_boxes)
    assert losses.requires_grad and not card.requires_grad and not cerr.requires_grad
    assert losses.shape == (L, 3) and card.shape == (L,) and cerr.shape == (1,)
    gl, gb = torch.autograd.grad((losses * case.G).sum(), (lg, bx))
    got = {"losses": losses.detach(), "card": card, "class_error": cerr, "grad_logits": gl, "grad_boxes": gb}
    check_case(case, got, alpha, gamma, fp32=_layers_at_once_on_device(case, alpha, gamma))
    # one gradient alone: the other output of the backward is skipped
    lg2 = case.logits.clone().requires_grad_(True)
    l2, _, _ = fused.set_criterion(lg2, case.boxes, case.tgt_of, case.labels, case.tboxes, case.tgt_len, alpha, gamma, case.num_boxes)
    g2, = torch.autograd.grad((l2 * case.G).sum(), (lg2,))
    assert torch.equal(g2, gl) and torch.equal(l2, losses)


def test_binding_rejects_a_label_outside_the_classes(dev):
    from trackformer_amd import _cabi, fused
    case = Y.Case(2, 1, 7, 2, [5], seed=3, device=dev)
    bad = case.labels.clone()
    bad[1] = 3                       # C = 2: 0, 1 and the no-object class 2 are labels, 3 is not
    with pytest.raises(_cabi.MSDAError):
        fused.set_criterion(case.logits, case.boxes, case.tgt_of, bad, case.tboxes, case.tgt_len, 0.25, 2.0, case.num_boxes)
    bad[1] = 2
    fused.set_criterion(case.logits, case.boxes, case.tgt_of, bad, case.tboxes, case.tgt_len, 0.25, 2.0, case.num_boxes)
    with pytest.raises(_cabi.MSDAError):
        fused.match_cost(case.logits.view(-1, 2), case.boxes.view(-1, 4), bad, case.tboxes, 2.0, 5.0, 2.0, 0.25, 2.0)
    torch.cuda.synchronize(dev)


def _outputs(case, lg=None, bx=None):
    layers = case.layer_outputs(lg, bx)
    return dict(layers[0], aux_outputs=layers[1:])


def test_criterion_forward_with_the_switch_on(dev):
    """SetCriterion.forward returns the same keys as with the switch off, the values agree to the yardstick, the gradients flow, and the
    own counter goes up.  The matcher here is the criterion's own: the pairs are its assignment of the case's predictions."""
    from trackformer_amd import criterion
    alpha, gamma = 0.25, 2.0
    case = Y.Case(6, 2, 40, 1, [5, 1], seed=7, device=dev)
    crit = Y.criterion_for(1, alpha, gamma).to(dev)
    off = crit(_outputs(case), case.targets())
    assert criterion.fused_counts() == {"own": 0, "torch": 0}
    lg, bx = case.logits.clone().requires_grad_(True), case.boxes.clone().requires_grad_(True)
    criterion.set_fused(True)
    on = crit(_outputs(case, lg, bx), case.targets())
    assert criterion.fused_counts() == {"own": 1, "torch": 0}
    assert list(on.keys()) == list(off.keys())
    assert all(v.dim() == 0 for v in on.values())
    for k in off:
        a, b = float(on[k]), float(off[k])
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (k, a, b)      # (a plausibility check; the bounds are asserted per output above)
    total = sum(v for k, v in on.items() if k.startswith("loss_"))
    total.backward()
    assert bool(torch.isfinite(lg.grad).all()) and bool(torch.isfinite(bx.grad).all()) and float(lg.grad.abs().sum()) > 0


class _FixedMatcher:
    """A matcher that hands out prepared pairs (for the unequal-counts decline)."""

    def __init__(self, per_set):
        self.per_set = per_set

    def match_many(self, outputs_list, targets):
        return self.per_set[:len(outputs_list)]

    def __call__(self, outputs, targets):
        return self.per_set[0]


def test_declines_run_todays_path_and_are_counted(dev):
    from trackformer_amd import criterion
    alpha, gamma = 0.25, 2.0
    case = Y.Case(3, 2, 7, 2, [5, 1], seed=9, device=dev)
    crit = Y.criterion_for(2, alpha, gamma).to(dev)
    want = crit(_outputs(case), case.targets())
    criterion.set_fused(True)
    # not fp32
    d = crit.double()(_outputs(case, case.logits.double(), case.boxes.double()),
                      [{k: (v.double() if v.is_floating_point() else v) for k, v in t.items()} for t in case.targets()])
    assert criterion.fused_counts(reset=True) == {"own": 0, "torch": 1}
    assert d.keys() == want.keys() and all(abs(float(d[k]) - float(want[k])) <= 1e-5 * max(1.0, abs(float(want[k]))) for k in want)
    # the non-focal criterion
    crit = Y.criterion_for(2, alpha, gamma).to(dev)
    plain = criterion.SetCriterion(2, crit.matcher, {}, 0.1, ["labels", "boxes", "cardinality"], False, alpha, gamma, False, 0.0).to(dev)
    with_bg = torch.cat([case.logits, torch.zeros_like(case.logits[..., :1])], -1)
    plain(_outputs(case, with_bg), case.targets())
    assert criterion.fused_counts(reset=True) == {"own": 0, "torch": 1}
    # unequal match counts between the layers
    pairs = [list(ind) for ind in case.all_indices]
    src, tgt = pairs[1][0]
    pairs[1][0] = (src[:-1], tgt[:-1])
    del crit.matcher                                   # (a registered sub-module: make room for a plain object)
    crit.matcher = _FixedMatcher(pairs)
    uneq = crit(_outputs(case), case.targets())
    assert criterion.fused_counts(reset=True) == {"own": 0, "torch": 1}
    assert uneq.keys() == want.keys()
    # and the same criterion with equal counts takes the route
    crit.matcher = _FixedMatcher(case.all_indices)
    got = crit(_outputs(case), case.targets())
    assert criterion.fused_counts(reset=True) == {"own": 1, "torch": 0}
    losses, card = Y.dict_to_tensors(got, case.L)
    ref = Y.reference(case, alpha, gamma)
    Y.check({"losses": losses, "card": card, "class_error": got["class_error"].reshape(1)}, ref, None, "SetCriterion.forward, fixed pairs")


def test_bit_identity_across_calls_streams_graph_and_a_busy_neighbour(dev):
    alpha, gamma = 0.25, 2.0
    case = Y.Case(6, 2, 300, 19, [5, 1], "wide", "nested", seed=13, device=dev)
    first = {k: v.clone() for k, v in Entries(case, alpha, gamma)().outputs().items()}

    def same(e, what):
        torch.cuda.synchronize(dev)
        e.assert_canaries()
        for k, v in e.outputs().items():
            assert torch.equal(v.view(torch.int32), first[k].view(torch.int32)), (what, k)

    same(Entries(case, alpha, gamma)(), "second call")
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        e = Entries(case, alpha, gamma)()
    torch.cuda.current_stream(dev).wait_stream(side)
    same(e, "side stream")
    # a captured graph of the two entries: one chain, no branches
    e = Entries(case, alpha, gamma)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(graph):
        e()
    for _ in range(2):
        for t, n in ((e.losses, case.L), (e.card, case.L), (e.cerr, 1), (e.gl, e.rows), (e.gb, e.rows)):
            t[:n].zero_()
        graph.replay()
        same(e, "graph replay")
    # while another stream runs an unrelated GEMM
    a = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        for _ in range(4):
            a = (a @ a) * 1e-3
    e = Entries(case, alpha, gamma)()
    torch.cuda.current_stream(dev).wait_stream(side)
    same(e, "next to a GEMM")


def test_class_error_is_torchs_when_every_matched_row_is_right(dev):
    """C == 1: every matched row's arg-max is its label.  100 - n (100 / n) is what torch's accuracy() gives in fp32 (0 for n = 11, where
    the product rounds to 100): no fused multiply-add may leave its residue."""
    for per in ([5, 6], [5, 1], [3, 4]):
        case = Y.Case(2, 2, 40, 1, per, seed=2, device=dev)
        got = Entries(case, 0.25, 2.0)().outputs()["class_error"]
        n = float(sum(per))
        want = 100 - torch.tensor(n) * (100.0 / n)
        assert float(got[0]) == float(want), (per, float(got[0]), float(want))


def test_a_nan_logit_stays_in_its_layer_and_its_element(dev):
    alpha, gamma = 0.25, 2.0
    case = Y.Case(3, 2, 40, 19, [5, 1], seed=17, device=dev)
    clean = {k: v.clone() for k, v in Entries(case, alpha, gamma)().outputs().items()}
    lg = case.logits.clone()
    lg[1, 1, 17, 4] = float("nan")
    e = Entries(case, alpha, gamma)(lg)
    torch.cuda.synchronize(dev)
    e.assert_canaries()
    got = e.outputs()
    assert bool(torch.isnan(got["losses"][1, 0])) and bool(torch.isfinite(got["losses"][[0, 2]]).all())
    assert bool(torch.isfinite(got["losses"][1, 1:]).all())
    nan = torch.isnan(got["grad_logits"])
    assert int(nan.sum()) == 1 and bool(nan[1, 1, 17, 4])
    keep = ~nan
    assert torch.equal(got["grad_logits"][keep].view(torch.int32), clean["grad_logits"][keep].view(torch.int32))
    assert torch.equal(got["grad_boxes"].view(torch.int32), clean["grad_boxes"].view(torch.int32))
    assert torch.equal(got["losses"][[0, 2]].view(torch.int32), clean["losses"][[0, 2]].view(torch.int32))
