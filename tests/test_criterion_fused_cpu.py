"""CPU: the fused set criterion and the matching cost (include/tf_fused.h: THE SET CRITERION AND THE MATCHING COST;
trackformer_amd/csrc/criterion.h) on the emulated library -- the kernels' own source under the SIMT emulator -- against float64 with the
yardstick of tests/util_criterion_fused.py, the yardstick's own self-tests, and the host logic of the two routes that needs no GPU."""
import numpy as np
import pytest
import torch

from tests import emu_lib
from tests import util_criterion_fused as Y
from trackformer_amd import box_ops, criterion, fused, matcher

emu = pytest.mark.skipif(not emu_lib.available(), reason="no host clang++ for the emulated library")

CANARY = np.float32(-4321.5)
GUARD = 3            # canary rows behind every output


def _lib():
    return emu_lib.lib()   # bound from the headers (trackformer_amd._cabi.bind)


def _al(a, dt=np.float32):
    return None if a is None else emu_lib._aligned16(np.ascontiguousarray(np.asarray(a), dtype=dt))


def _p(a):
    return None if a is None else a.ctypes.data


def _guarded(rows, cols, fill=np.nan):
    """[rows + GUARD, cols] fp32, 16-byte aligned: `fill` in the rows the entry writes, the canary behind them."""
    buf = _al(np.full((rows + GUARD, cols), fill, np.float32))
    buf[rows:] = CANARY
    return buf


def _inputs(case):
    T = case.T
    return (_al(case.logits.numpy()), _al(case.boxes.numpy()), _al(case.tgt_of.numpy(), np.int32),
            _al(case.labels.numpy(), np.int64) if T else None, _al(case.tboxes.numpy()) if T else None, _al(case.tgt_len.numpy(), np.int32))


def run_entries(case, alpha, gamma, tgt_of=None, want=("grad_logits", "grad_boxes")):
    """Both criterion entries on the emulator -> {name: tensor}.  Outputs start as NaN, canary rows behind each are checked, the kernels
    are checked by name, and nothing may diverge around a wave operation."""
    L, B, Q, C, T = case.L, case.B, case.Q, case.C, case.T
    lg, bx, to, lab, tb, tl = _inputs(case)
    if tgt_of is not None:
        to = _al(tgt_of.numpy(), np.int32)
    losses, card, cerr = _guarded(L, 3), _guarded(L, 1), _guarded(1, 1)
    emu_lib.stats(reset=True)
    lib = _lib()
    rc = lib.tf_set_criterion_fwd_f32(_p(lg), _p(bx), _p(to), _p(lab), _p(tb), _p(tl), _p(losses), _p(card), _p(cerr), L, B, Q, C, T,
                                      alpha, gamma, case.num_boxes, None)
    assert rc == 0, rc
    assert emu_lib.last_kernel() == "set_criterion_fwd_f32"
    rows = L * B * Q
    gl = _guarded(rows, C) if "grad_logits" in want else None
    gb = _guarded(rows, 4) if "grad_boxes" in want else None
    G = _al(case.G.numpy())
    rc = lib.tf_set_criterion_bwd_f32(_p(G), _p(lg), _p(bx), _p(to), _p(lab), _p(tb), _p(gl), _p(gb), L, B, Q, C, T, alpha, gamma,
                                      case.num_boxes, None)
    assert rc == 0, rc
    if want:
        assert emu_lib.last_kernel() == "set_criterion_bwd_f32"
    st = emu_lib.stats()
    assert st["divergent_ops"] == 0 and st["inactive_reads"] == 0, st
    for name, buf, n in (("losses", losses, L), ("card", card, L), ("class_error", cerr, 1), ("grad_logits", gl, rows), ("grad_boxes", gb, rows)):
        if buf is not None:
            assert (buf[n:] == CANARY).all(), "wrote behind " + name
            assert not np.isnan(buf[:n]).any(), name + " was not written everywhere"
    return {"losses": torch.from_numpy(losses[:L].copy()), "card": torch.from_numpy(card[:L, 0].copy()),
            "class_error": torch.from_numpy(cerr[:1, 0].copy()),
            "grad_logits": None if gl is None else torch.from_numpy(gl[:rows].copy()).view(L, B, Q, C),
            "grad_boxes": None if gb is None else torch.from_numpy(gb[:rows].copy()).view(L, B, Q, 4)}


def run_case(case, alpha, gamma):
    got = run_entries(case, alpha, gamma)
    box_margin, logit_margin = case.margins()
    assert box_margin >= 1.0 and logit_margin >= 1.0, (box_margin, logit_margin)
    what = "%s / %s L%d B%d Q%d C%d %r g%.1f a%.2f" % (case.logit_profile, case.box_profile, case.L, case.B, case.Q, case.C, case.sizes,
                                                     gamma, alpha)
    Y.check(got, Y.reference(case, alpha, gamma), Y.fp32_formulation(case, alpha, gamma) if any(case.sizes) else None, what)
    return got


def run_cost(lg, boxes, ids, tb, w, alpha, gamma):
    R, C = lg.shape
    T = ids.numel()
    cost = _guarded(R, max(T, 1))
    lg, boxes, ids, tb = _al(lg.numpy()), _al(boxes.numpy()), _al(ids.numpy(), np.int64), _al(tb.numpy())
    rc = _lib().tf_match_cost_f32(_p(lg), _p(boxes), _p(ids), _p(tb), _p(cost), R, C, T, w[0], w[1], w[2], alpha, gamma, None)
    assert rc == 0, rc
    if T:
        assert emu_lib.last_kernel() == "match_cost_f32"
    flat = cost.reshape(-1)
    assert (flat[R * T:] == CANARY).all() or T == 0, "wrote behind the cost matrix"
    return torch.from_numpy(flat[:R * T].copy()).view(R, T)


# ---- the yardstick itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", list(Y.BOX_PROFILES))
def test_analytic_box_gradients_equal_float64_autograd(profile):
    """The reference writes the gradient of 1 - GIoU by hand (as the kernel does): it is autograd's through
    box_ops.generalized_box_iou_pairs, in float64."""
    a, b = Y.matched_boxes(profile, 64, torch.Generator().manual_seed(5))
    assert float(Y.pair_margins(a, b).min()) >= Y.MARGIN * Y.BOX_PROFILES[profile]
    ad = a.double().requires_grad_(True)
    loss = 1 - box_ops.generalized_box_iou_pairs(box_ops.box_cxcywh_to_xyxy(ad), box_ops.box_cxcywh_to_xyxy(b.double()))
    want, = torch.autograd.grad(loss.sum(), ad)
    giou, grad = Y.giou_reference(Y.V(a.double()), Y.V(b.double()), grad=True)
    assert torch.allclose(1 - giou.v, loss.detach(), rtol=1e-13, atol=0)
    assert torch.allclose(grad.v, want, rtol=1e-10, atol=1e-13 * float(want.abs().max()))
    assert bool((grad.E >= grad.v.abs()).all()) and bool((giou.E >= giou.v.abs()).all())


@pytest.mark.parametrize("gamma,alpha", [(2.0, 0.25), (1.5, -1.0)])
def test_stable_focal_form_is_the_product_formula_and_its_own_derivative(gamma, alpha):
    """On unit logits, where sigmoid_focal_loss in float64 has lost nothing, the stable form equals it; its hand-written derivative is
    autograd's."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 50, 7, generator=g).double().requires_grad_(True)
    pos = torch.rand(4, 50, 7, generator=g) < 0.2
    f, df = Y.focal_reference(x.detach(), pos, alpha, gamma)
    want = criterion.sigmoid_focal_loss(x, pos.double(), 1.0, alpha=alpha, gamma=gamma, reduction=False)
    assert torch.allclose(f.v, want.detach(), rtol=1e-9, atol=0)
    grad, = torch.autograd.grad(want.sum(), x)
    assert torch.allclose(df.v, grad, rtol=1e-8, atol=0)


def _stable_fp32(x, pos, alpha, gamma):
    """The stable form in torch fp32 with autograd: what an fp32 implementation can reach."""
    z = torch.where(pos, -x, x)
    u = torch.log1p(torch.exp(-z.abs()))
    sp, sn = z.clamp_min(0) + u, (-z).clamp_min(0) + u
    a = 1.0 if alpha < 0 else torch.where(pos, alpha, 1 - alpha)
    return a * (sp * torch.exp(-gamma * sn))


@pytest.mark.parametrize("scale", [1.0, 8.0, 30.0, 1e-4])
@pytest.mark.parametrize("gamma,alpha", [(2.0, 0.25), (1.5, -1.0)])
def test_the_focal_bound_is_one_an_fp32_stable_form_meets_and_the_product_formula_does_not(scale, gamma, alpha):
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(3, 200, 5, generator=g) * scale).requires_grad_(True)
    pos = torch.rand(3, 200, 5, generator=g) < 0.2
    f, df = Y.focal_reference(x.detach().double(), pos, alpha, gamma)
    loss = _stable_fp32(x, pos, alpha, gamma)
    grad, = torch.autograd.grad(loss.sum(), x)
    wl, wg = Y.excess_of(loss.detach(), f), Y.excess_of(grad, df)
    xt = x.detach().clone().requires_grad_(True)
    tl = criterion.sigmoid_focal_loss(xt, pos.float(), 1.0, alpha=alpha, gamma=gamma, reduction=False)
    tg, = torch.autograd.grad(tl.sum(), xt)
    t_l, t_g = Y.excess_of(tl.detach(), f), Y.excess_of(tg, df)
    print("scale %g: stable fp32 %.3f / %.3f x 2^-20, sigmoid_focal_loss fp32 %.3g / %.3g x 2^-20"
          % (scale, wl.value / Y.BOUND, wg.value / Y.BOUND, t_l.value / Y.BOUND, t_g.value / Y.BOUND))
    assert wl.value <= Y.BOUND and wg.value <= Y.BOUND, (wl, wg)
    if scale >= 8:
        assert t_l.value > 100 * Y.BOUND, t_l


@pytest.mark.parametrize("profile", list(Y.BOX_PROFILES))
def test_the_box_bounds_are_ones_torch_fp32_meets(profile):
    case = Y.Case(3, 2, 40, 2, [5, 1], "unit", profile, seed=2)
    ref, fp32 = Y.reference(case, 0.25, 2.0), Y.fp32_formulation(case, 0.25, 2.0)
    for name in ("losses", "grad_boxes", "card", "class_error"):
        got = fp32[name]
        ref_v = ref[name]
        if name == "losses":   # the box columns: the focal column is the product formula's (above)
            got, ref_v = got[:, 1:], Y.V(ref_v.v[:, 1:], ref_v.E[:, 1:])
        worst = Y.excess_of(got, ref_v)
        print("%-12s %-12s torch fp32 %.4f x 2^-20" % (profile, name, worst.value / Y.BOUND))
        assert worst.value <= Y.BOUND, (profile, name, worst)


def test_the_yardstick_rejects_what_it_must():
    """One element off by 1 + 2^-12, a swapped x / y box gradient and an off-by-one tgt_of are each rejected."""
    alpha, gamma = 0.25, 2.0
    case = Y.Case(3, 2, 7, 19, [5, 1], seed=4)
    ref = Y.reference(case, alpha, gamma)
    good = {k: v.v.float() for k, v in ref.items()}
    Y.check(good, ref, None, "the reference rounded to fp32")
    for name in Y.OUTPUTS:
        bad = dict(good)
        t = good[name].clone().reshape(-1)
        i = int(t.abs().argmax())
        t[i] = t[i] * (1 + 2.0 ** -12)
        bad[name] = t.view(good[name].shape)
        with pytest.raises(AssertionError):
            Y.check(bad, ref, None, "one element of %s scaled" % name)
    bad = dict(good)
    bad["grad_boxes"] = good["grad_boxes"][..., [1, 0, 2, 3]]
    with pytest.raises(AssertionError):
        Y.check(bad, ref, None, "x / y swapped")
    shifted = case.tgt_of.clone()
    m = shifted >= 0
    shifted[m] = (shifted[m] + 1) % case.T
    off = {k: v.v.float() for k, v in Y.reference(case, alpha, gamma, tgt_of=shifted).items()}
    for name in ("losses", "grad_logits", "grad_boxes"):
        with pytest.raises(AssertionError):
            Y.check({name: off[name]}, ref, None, "tgt_of off by one")


# ---- the criterion kernels on the emulator ---------------------------------------------------------------------------------------------
# L in {1, 3, 6}, B in {1, 2, 3}, Q in {1, 7, 40, 257} (257: a second pass of the workgroup's 256 threads with one row in it), C in {1, 2,
# 19, 91}, targets per image in {0, 1, 5}; T = 0, an image without targets, more targets than queries (Q = 1)
SHAPES = [
    (1, 1, 1, 1, [1]), (1, 1, 1, 2, [0]), (2, 1, 1, 19, [5]), (3, 2, 7, 1, [5, 0]), (3, 2, 7, 19, [1, 5]), (6, 3, 40, 2, [5, 1, 0]),
    (6, 2, 40, 19, [0, 0]), (1, 3, 40, 91, [1, 0, 5]), (3, 1, 257, 1, [5]), (1, 2, 257, 91, [5, 5]),
]
SETTINGS = [(2.0, 0.25), (1.5, 0.25), (2.0, -1.0), (1.5, -1.0)]


@emu
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["L%d-B%d-Q%d-C%d-%s" % (s[0], s[1], s[2], s[3], "".join(map(str, s[4]))) for s in SHAPES])
def test_criterion_kernels_against_float64(i):
    L, B, Q, C, per = SHAPES[i]
    gamma, alpha = SETTINGS[i % 4]
    run_case(Y.Case(L, B, Q, C, per, seed=i), alpha, gamma)


@emu
@pytest.mark.parametrize("box_profile", list(Y.BOX_PROFILES))
@pytest.mark.parametrize("logit_profile", list(Y.LOGIT_PROFILES))
def test_every_profile_pair_against_float64(logit_profile, box_profile):
    run_case(Y.Case(3, 2, 40, 19, [5, 1], logit_profile, box_profile, seed=21), 0.25, 2.0)


@emu
@pytest.mark.parametrize("gamma,alpha", SETTINGS)
def test_every_gamma_and_alpha_on_wide_logits(gamma, alpha):
    run_case(Y.Case(3, 3, 7, 2, [1, 5, 0], "wide", "nested", seed=33), alpha, gamma)


@emu
def test_either_gradient_may_be_skipped_and_results_repeat():
    case = Y.Case(3, 2, 40, 19, [5, 1], seed=8)
    both = run_entries(case, 0.25, 2.0)
    only_l = run_entries(case, 0.25, 2.0, want=("grad_logits",))
    only_b = run_entries(case, 0.25, 2.0, want=("grad_boxes",))
    assert only_l["grad_boxes"] is None and only_b["grad_logits"] is None
    assert torch.equal(only_l["grad_logits"], both["grad_logits"]) and torch.equal(only_b["grad_boxes"], both["grad_boxes"])
    assert torch.equal(only_l["losses"], both["losses"])
    run_entries(case, 0.25, 2.0, want=())
    unmatched = case.tgt_of < 0
    assert bool((both["grad_boxes"][unmatched] == 0).all())


@emu
def test_c1_cardinality_quirk_ties_and_class_error():
    """C == 1: the cardinality prediction is 0, as the reference's.  Ties: the lowest index wins.  Nothing matched: class_error 100."""
    case = Y.Case(2, 2, 7, 1, [5, 1], seed=1)
    got = run_entries(case, 0.25, 2.0)
    assert torch.equal(got["card"], torch.full((2,), 3.0))            # mean(|0 - 5|, |0 - 1|)
    case = Y.Case(1, 1, 7, 2, [1], seed=1)
    case.logits[...] = 0.5                                              # every row a tie: arg-max 0 != C - 1 in all 7 rows
    case.labels[...] = 0
    got = run_entries(case, 0.25, 2.0)
    assert float(got["card"][0]) == 6.0 and float(got["class_error"][0]) == 0.0
    case.labels[...] = 1
    assert float(run_entries(case, 0.25, 2.0)["class_error"][0]) == 100.0
    empty = Y.Case(2, 2, 7, 19, [0, 0], seed=1)
    got = run_entries(empty, 0.25, 2.0)
    assert float(got["class_error"][0]) == 100.0 and bool((got["losses"][:, 1:] == 0).all()) and bool((got["grad_boxes"] == 0).all())


@emu
def test_a_tgt_of_outside_the_targets_counts_as_unmatched():
    case = Y.Case(2, 1, 7, 2, [1], seed=6)
    base = run_entries(case, 0.25, 2.0, tgt_of=torch.full_like(case.tgt_of, -1))
    wild = case.tgt_of.clone()
    wild[wild >= 0] = case.T + 3
    got = run_entries(case, 0.25, 2.0, tgt_of=wild)
    for k in ("losses", "grad_logits", "grad_boxes"):
        assert torch.equal(got[k], base[k]), k


@emu
def test_error_codes():
    lib = _lib()
    case = Y.Case(2, 1, 7, 2, [1], seed=6)
    lg, bx, to, lab, tb, tl = _inputs(case)
    out = [_guarded(2, 3), _guarded(2, 1), _guarded(1, 1)]
    o = [_p(a) for a in out]

    def fwd(lg=_p(lg), bx=_p(bx), to=_p(to), lab=_p(lab), tb=_p(tb), tl=_p(tl), losses=o[0], L=2, B=1, Q=7, C=2, T=1, nb=1.0):
        return lib.tf_set_criterion_fwd_f32(lg, bx, to, lab, tb, tl, losses, o[1], o[2], L, B, Q, C, T, 0.25, 2.0, nb, None)
    assert fwd() == 0
    assert fwd(lg=None) == -1 and fwd(to=None) == -1 and fwd(tl=None) == -1 and fwd(losses=None) == -1 and fwd(lab=None) == -1
    assert fwd(lab=None, tb=None, T=0) == 0                              # T == 0: null target pointers are accepted
    assert fwd(L=0) == -2 and fwd(Q=-1) == -2 and fwd(C=0) == -2 and fwd(T=-1) == -2 and fwd(nb=0.0) == -2
    assert fwd(L=2 ** 20, B=2 ** 10, Q=2 ** 10) == -2                   # the row count leaves int32
    assert fwd(bx=_p(bx) + 4) == -2 and fwd(tb=_p(tb) + 8) == -2 and fwd(lg=_p(lg) + 2) == -2 and fwd(lab=_p(lab) + 4) == -2
    G = _al(case.G.numpy())
    gl, gb = _guarded(14, 2), _guarded(14, 4)

    def bwd(G=_p(G), gl=_p(gl), gb=_p(gb), lg=_p(lg), Q=7):
        return lib.tf_set_criterion_bwd_f32(G, lg, _p(bx), _p(to), _p(lab), _p(tb), gl, gb, 2, 1, Q, 2, 1, 0.25, 2.0, 1.0, None)
    assert bwd() == 0 and bwd(gl=None) == 0 and bwd(gb=None) == 0 and bwd(gl=None, gb=None) == 0
    assert bwd(G=None) == -1 and bwd(lg=None) == -1 and bwd(Q=0) == -2 and bwd(gb=_p(gb) + 4) == -2
    cost = _guarded(14, 1)
    ids = _al(case.labels.numpy(), np.int64)

    def mc(lg=_p(lg), ids=_p(ids), cost=_p(cost), R=14, C=2, T=1):
        return lib.tf_match_cost_f32(lg, _p(bx), ids, _p(tb), cost, R, C, T, 2.0, 5.0, 2.0, 0.25, 2.0, None)
    assert mc() == 0 and mc(T=0) == 0 and mc(R=0) == 0
    assert mc(lg=None) == -1 and mc(cost=None) == -1 and mc(C=0) == -2 and mc(R=-1) == -2 and mc(ids=_p(ids) + 4) == -2
    assert mc(R=2 ** 31, T=4) == -2


# ---- the host side -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 2, 7, [5, 1]), (2, 3, 40, [0, 5, 1]), (1, 1, 1, [5]), (2, 2, 7, [0, 0])])
def test_tgt_of_is_what_layers_at_once_indexes(shape):
    """build_tgt_of against the index tensors _layers_at_once builds from the same pairs (criterion.py: lay / bat / qry / tgt)."""
    L, B, Q, per = shape
    case = Y.Case(L, B, Q, 2, per, seed=9)
    tgt_of, tgt_len = criterion.build_tgt_of(case.all_indices, per, Q)
    assert tgt_of.dtype == np.int32 and tgt_of.shape == (L, B, Q) and tgt_len.dtype == np.int32 and tgt_len.tolist() == per
    n = sum(len(src) for src, _ in case.all_indices[0])
    lay = torch.cat([torch.full((n,), l, dtype=torch.int64) for l in range(L)])
    bat = torch.cat([torch.full_like(src, i) for ind in case.all_indices for i, (src, _) in enumerate(ind)])
    qry = torch.cat([src for ind in case.all_indices for (src, _) in ind])
    offs = criterion.SetCriterion._offsets(case.targets())
    tgt = torch.cat([torch.cat([t_idx + off for (_, t_idx), off in zip(ind, offs)]) for ind in case.all_indices])
    assert tgt_of[lay.numpy(), bat.numpy(), qry.numpy()].tolist() == tgt.tolist()
    assert int((tgt_of >= 0).sum()) == L * n
    assert np.array_equal(tgt_of, case.tgt_of.numpy())


def test_switches_counters_and_declines_without_a_gpu():
    """Both switches are off by default, follow their environment variable, bump the route epoch when their value changes, and a call
    the kernels do not take (CPU tensors here) runs today's path and is counted under "torch"."""
    assert criterion.fused_enabled() is False and matcher.fused_cost_enabled() is False
    case = Y.Case(3, 2, 7, 2, [5, 1], seed=12)
    crit = Y.criterion_for(2, 0.25, 2.0)
    outputs = dict(case.layer_outputs()[0], aux_outputs=case.layer_outputs()[1:])
    want = crit(outputs, case.targets())
    epoch = fused.route_epoch()
    assert criterion.set_fused(True) is False and matcher.set_fused_cost(True) is False
    assert fused.route_epoch() == epoch + 2
    try:
        assert criterion.set_fused(True) is True and fused.route_epoch() == epoch + 2     # no change of value: no new epoch
        criterion.fused_counts(reset=True)
        matcher.fused_cost_counts(reset=True)
        got = crit(outputs, case.targets())
        assert criterion.fused_counts() == {"own": 0, "torch": 1}
        assert matcher.fused_cost_counts() == {"own": 0, "torch": 1}
        assert got.keys() == want.keys() and all(torch.equal(got[k], want[k]) for k in want)
    finally:
        criterion.set_fused(None)
        matcher.set_fused_cost(None)
    assert criterion.fused_enabled() is False and matcher.fused_cost_enabled() is False
    assert criterion.fused_counts(reset=True)["torch"] == 1 and criterion.fused_counts() == {"own": 0, "torch": 0}


def test_environment_switches(monkeypatch):
    monkeypatch.setenv("TF_CRITERION_FUSED", "1")
    monkeypatch.setenv("TF_MATCHER_FUSED_COST", "1")
    assert criterion.fused_enabled() and matcher.fused_cost_enabled()
    monkeypatch.setenv("TF_CRITERION_FUSED", "0")
    monkeypatch.setenv("TF_MATCHER_FUSED_COST", "")
    assert not criterion.fused_enabled() and not matcher.fused_cost_enabled()


# ---- the matching cost -----------------------------------------------------------------------------------------------------------------
COST_W = (2.0, 5.0, 2.0)            # class, bbox, giou: the weights of the tracking configurations
COST_SEEDS = [1, 2, 3, 4]


def cost_fixture(seed, B=2, Q=40, C=19, per=(5, 3), logit_profile="unit"):
    """Predictions of one set against the targets of B images: (logits [B Q, C], boxes [B Q, 4], tgt_ids, tgt_bbox, sizes)."""
    case = Y.Case(1, B, Q, C, list(per), logit_profile, "overlapping", seed=seed)
    return case.logits.view(B * Q, C), case.boxes.view(B * Q, 4), case.labels, case.tboxes, list(per)


@pytest.mark.parametrize("seed", COST_SEEDS)
def test_cost_fixtures_have_one_assignment_within_the_bound(seed):
    """The float64 cost perturbed eight times by +- its own bound gives linear_sum_assignment the same pairs every time: on these
    fixtures any cost within the bound must reproduce float64's assignment."""
    lg, bx, ids, tb, sizes = cost_fixture(seed)
    ref = Y.cost_reference(lg, bx, ids, tb, COST_W[0], COST_W[1], COST_W[2], 0.25, 2.0)
    _, same = Y.perturbed_assignments(ref, sizes, 2, 40, seed)
    assert same, seed


@pytest.mark.parametrize("logit_profile", list(Y.LOGIT_PROFILES))
def test_the_cost_bound_is_one_torch_fp32_meets_where_it_claims(logit_profile):
    lg, bx, ids, tb, _ = cost_fixture(1, logit_profile=logit_profile)
    ref = Y.cost_reference(lg, bx, ids, tb, *COST_W, 0.25, 2.0)
    worst = Y.excess_of(Y.cost_fp32(lg, bx, ids, tb, *COST_W, 0.25, 2.0), ref)
    print("%-6s torch fp32 cost %.4f x 2^-20" % (logit_profile, worst.value / Y.BOUND))
    if logit_profile != "wide":      # (1 - p as an fp32 subtraction: the wide profile is where the chain loses its digits)
        assert worst.value <= Y.BOUND, worst


@emu
@pytest.mark.parametrize("R,C,T", [(1, 1, 1), (7, 2, 5), (257, 19, 3), (40, 91, 6), (300, 1, 5)])
@pytest.mark.parametrize("gamma", [2.0, 1.5])
def test_cost_kernel_against_float64(R, C, T, gamma):
    for profile in Y.LOGIT_PROFILES:
        case = Y.Case(1, 1, R, C, [T], profile, "overlapping", seed=R + T)
        lg, bx = case.logits.view(R, C), case.boxes.view(R, 4)
        got = run_cost(lg, bx, case.labels, case.tboxes, COST_W, 0.25, gamma)
        ref = Y.cost_reference(lg, bx, case.labels, case.tboxes, *COST_W, 0.25, gamma)
        Y.check_one("cost", got, ref, Y.cost_fp32(lg, bx, case.labels, case.tboxes, *COST_W, 0.25, gamma),
                    "%s R%d C%d T%d g%.1f" % (profile, R, C, T, gamma))


@emu
@pytest.mark.parametrize("seed", COST_SEEDS)
def test_cost_kernel_gives_float64s_assignment(seed):
    from scipy.optimize import linear_sum_assignment
    lg, bx, ids, tb, sizes = cost_fixture(seed)
    ref = Y.cost_reference(lg, bx, ids, tb, *COST_W, 0.25, 2.0)
    base, same = Y.perturbed_assignments(ref, sizes, 2, 40, seed)
    assert same
    got = run_cost(lg, bx, ids, tb, COST_W, 0.25, 2.0).view(2, 40, -1)
    pairs = [tuple(np.asarray(i).tolist() for i in linear_sum_assignment(blk[b].numpy())) for b, blk in enumerate(got.split(sizes, -1))]
    assert pairs == base
