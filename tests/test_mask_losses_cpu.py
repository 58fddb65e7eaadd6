"""CPU: the fused mask losses (include/tf_fused.h: THE MASK LOSSES; trackformer_amd/csrc/mask_loss.h) on the emulated library -- the
kernels' own source under the SIMT emulator -- against float64 with the yardstick of tests/util_mask_losses.py, the yardstick's own
self-tests, and the host logic of the route that needs no GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import emu_lib
from tests import util_criterion_fused as Y
from tests import util_mask_losses as M
from trackformer_amd import criterion, fused

emu = pytest.mark.skipif(not emu_lib.available(), reason="no host clang++ for the emulated library")

CANARY = np.float32(-4321.5)
GUARD = 3            # canary rows behind every output and the workspace
EMU_SHAPES = [s for s in M.SHAPES if s[2] * s[3] <= 128 * 160]


def _lib():
    return emu_lib.lib()   # bound from the headers (trackformer_amd._cabi.bind)


def _al(a, dt=np.float32):
    return emu_lib._aligned16(np.ascontiguousarray(np.asarray(a), dtype=dt))


def _p(a):
    return None if a is None else a.ctypes.data


def _guarded(rows, cols, dt=np.float32):
    """[rows + GUARD, cols], 16-byte aligned: NaN in the rows the entry writes, the canary behind them."""
    buf = _al(np.full((rows + GUARD, cols), np.nan, dt), dt)
    buf[rows:] = CANARY
    return buf


def run_entries(case, alpha, gamma):
    """Both entries on the emulator -> {"losses", "grad", "sums"}.  Outputs and the workspace start as NaN and must all be written,
    canary rows behind each are checked, the kernels are checked by name (and the forward's by its number of workgroups), and nothing
    may diverge around a wave operation."""
    h, w, H, W = case.shape
    n, rows, T = case.n, M.B * M.Q, case.tgt.shape[0]
    lib = _lib()
    src = _al(case.pred_masks.numpy())
    tgt = np.ascontiguousarray(case.tgt.numpy().view(np.uint8))
    ps, pt, rp = _al(case.pair_src.numpy(), np.int32), _al(case.pair_tgt.numpy(), np.int32), _al(case.row_pair.numpy(), np.int32)
    tiles = M.tiles_of(H)
    nbytes = lib.tf_mask_loss_workspace_bytes(n, H, W)
    assert nbytes == n * tiles * 4 * 8
    sums, losses, ws = _guarded(n, 4, np.float64), _guarded(2, 1), _guarded(n * tiles, 4, np.float64)
    emu_lib.stats(reset=True)
    rc = lib.tf_mask_loss_fwd_f32(_p(src), _p(tgt), _p(ps), _p(pt), _p(sums), _p(losses), _p(ws), nbytes, n, rows, T, h, w, H, W, alpha,
                                  gamma, case.num_boxes, None)
    assert rc == 0, rc
    assert emu_lib.last_kernel() == "mask_loss_finish_f32"
    assert emu_lib.stats()["blocks"] == n * tiles + 1          # mask_loss_fwd_f32: one workgroup per (pair, tile); the finish: one
    grad = _guarded(rows, h * w)
    G = _al(case.G.numpy())
    rc = lib.tf_mask_loss_bwd_f32(_p(G), _p(src), _p(tgt), _p(pt), _p(rp), _p(sums), _p(grad), n, rows, T, h, w, H, W, alpha, gamma,
                                  case.num_boxes, None)
    assert rc == 0, rc
    assert emu_lib.last_kernel() == "mask_loss_bwd_f32"
    st = emu_lib.stats()
    assert st["divergent_ops"] == 0 and st["inactive_reads"] == 0, st
    for name, buf, k in (("sums", sums, n), ("losses", losses, 2), ("workspace", ws, n * tiles), ("grad", grad, rows)):
        assert (buf[k:] == CANARY).all(), "wrote behind " + name
        assert not np.isnan(buf[:k]).any(), name + " was not written everywhere"
    return {"losses": torch.from_numpy(losses[:2, 0].copy()), "grad": torch.from_numpy(grad[:rows].copy()).view(M.B, M.Q, h, w),
            "sums": torch.from_numpy(sums[:n].copy())}


def run_case(case, alpha=0.25, gamma=2.0):
    got = run_entries(case, alpha, gamma)
    M.check(got, M.reference(case, alpha, gamma), M.fp32_formulation(case, alpha, gamma), "%s g%.1f a%.2f" % (case.what(), gamma, alpha))
    unmatched = (case.row_pair < 0).view(M.B, M.Q)
    assert bool((got["grad"][unmatched] == 0).all())
    return got


# ---- the yardstick itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integer_coordinates_are_float64_interpolate(shape):
    h, w, H, W = shape
    s = torch.randn(3, h, w, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    want = F.interpolate(s[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]
    x, corners = M.upsample(s, H, W)
    # ATen's float64 coordinate scale (Y + 0.5) - 0.5 carries a few roundings of a number up to max(h, w); a weight's error moves the
    # value by at most that times the largest difference of two neighbours (<= 2 max |s|): 16 roundings of margin
    assert torch.allclose(x.v, want, rtol=0, atol=16 * 2.0 ** -52 * max(h, w) * 2 * float(s.abs().max()))
    assert torch.allclose(sum(wgt.v for _, wgt in corners), torch.ones(H, W, dtype=torch.float64), rtol=0, atol=1e-15)
    assert bool((x.E >= x.v.abs()).all())


@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", M.TARGET_KINDS)
def test_reference_is_float64_autograd_through_loss_masks(shape, kind):
    """On unit logits, where sigmoid_focal_loss in float64 has lost nothing, the V reference (stable focal form, integer coordinates,
    hand-written gather) is criterion.loss_masks in float64 and autograd through it."""
    case = M.Case(shape, 3, "unit", kind, seed=2)
    ref = M.reference(case, 0.25, 2.0)
    pm = case.pred_masks.double().requires_grad_(True)
    losses = M.torch_loss_masks(case, pm)
    grad, = torch.autograd.grad((losses * case.G.double()).sum(), pm)
    assert torch.allclose(ref["losses"].v, losses.detach(), rtol=1e-12, atol=0)
    assert torch.allclose(ref["grad"].v, grad, rtol=1e-9, atol=1e-14 * float(grad.abs().max()))
    assert bool((ref["grad"].E >= ref["grad"].v.abs()).all()) and bool((ref["losses"].E >= ref["losses"].v.abs()).all())


def test_the_yardstick_rejects_what_it_must():
    """One element off by 1 + 2^-12, a gradient shifted by one pixel and the targets taken by position are each rejected."""
    case = M.Case((5, 7, 19, 23), 3, "unit", "box", seed=4)
    ref = M.reference(case, 0.25, 2.0)
    good = {k: ref[k].v.float() for k in M.OUTPUTS}
    M.check(good, ref, None, "the reference rounded to fp32")
    for name in M.OUTPUTS:
        t = good[name].clone().reshape(-1)
        i = int(t.abs().argmax())
        t[i] = t[i] * (1 + 2.0 ** -12)
        with pytest.raises(AssertionError):
            M.check(dict(good, **{name: t.view(good[name].shape)}), ref, None, "one element of %s scaled" % name)
    with pytest.raises(AssertionError):
        M.check(dict(good, grad=good["grad"].roll(1, -1)), ref, None, "shifted by a pixel")
    by_position = M.Case((5, 7, 19, 23), 3, "unit", "box", seed=4)
    by_position.pair_tgt = torch.arange(3, dtype=torch.int32)
    off = M.reference(by_position, 0.25, 2.0)
    with pytest.raises(AssertionError):
        M.check({k: off[k].v.float() for k in M.OUTPUTS}, ref, None, "targets by position")


# ---- the kernels on the emulator -------------------------------------------------------------------------------------------------------
@emu
@pytest.mark.parametrize("shape", EMU_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("profile", list(M.LOGIT_PROFILES))
def test_mask_loss_kernels_against_float64(shape, profile):
    if shape == (16, 20, 128, 160):
        assert M.tiles_of(shape[2]) >= 3          # the tile rule: 8 output rows per tile -> 16 partials per pair
    run_case(M.Case(shape, 3, profile, "box", seed=1))


@emu
@pytest.mark.parametrize("kind", M.TARGET_KINDS)
@pytest.mark.parametrize("n", [0, 1, 3])
def test_every_target_kind_and_pair_count(kind, n):
    got = run_case(M.Case((5, 7, 19, 23), n, "unit", kind, seed=3))
    if n == 0:
        assert bool((got["losses"] == 0).all()) and bool((got["grad"] == 0).all())


@emu
@pytest.mark.parametrize("gamma,alpha", [(2.0, -1.0), (1.5, 0.25), (1.5, -1.0)])
@pytest.mark.parametrize("profile", ["unit", "wide"])
def test_other_alpha_and_gamma(gamma, alpha, profile):
    run_case(M.Case((13, 21, 100, 167), 3, profile, "box", seed=5), alpha, gamma)


@emu
def test_targets_are_indexed_by_pair_tgt_and_results_repeat():
    case = M.Case((16, 20, 64, 80), 3, "unit", "box", seed=6)
    a, b = run_entries(case, 0.25, 2.0), run_entries(case, 0.25, 2.0)
    assert all(torch.equal(a[k], b[k]) for k in a)
    st = case.tgt[case.pair_tgt.long()].double().sum((1, 2))
    assert torch.equal(a["sums"][:, 3], st)                              # sum t: exact, of the rows pair_tgt names
    assert not torch.equal(st, case.tgt[:3].double().sum((1, 2)))        # (by position it would be another number)


@emu
def test_indices_outside_their_range_count_as_unmatched():
    case = M.Case((5, 7, 19, 23), 3, "unit", "box", seed=7)
    base = run_entries(M.Case((5, 7, 19, 23), 0, "unit", "box", seed=7), 0.25, 2.0)
    case.pair_tgt[:] = case.tgt.shape[0] + 2
    got = run_entries(case, 0.25, 2.0)
    assert bool((got["grad"] == 0).all()) and bool((got["sums"] == 0).all())
    assert float(got["losses"][0]) == 0.0 and base["losses"].tolist() == [0.0, 0.0]
    case = M.Case((5, 7, 19, 23), 3, "unit", "box", seed=7)
    case.pair_src[:] = -1
    case.row_pair[:] = 99
    got = run_entries(case, 0.25, 2.0)
    assert bool((got["grad"] == 0).all()) and bool((got["sums"] == 0).all())


@emu
def test_error_codes():
    lib = _lib()
    case = M.Case((5, 7, 19, 23), 3, "unit", "box", seed=8)
    h, w, H, W = case.shape
    src, tgt = _al(case.pred_masks.numpy()), np.ascontiguousarray(case.tgt.numpy().view(np.uint8))
    ps, pt, rp = _al(case.pair_src.numpy(), np.int32), _al(case.pair_tgt.numpy(), np.int32), _al(case.row_pair.numpy(), np.int32)
    nbytes = lib.tf_mask_loss_workspace_bytes(3, H, W)
    sums, losses, ws, grad, G = _guarded(3, 4, np.float64), _guarded(2, 1), _guarded(3 * 3, 4, np.float64), _guarded(8, h * w), _al(case.G.numpy())
    assert lib.tf_mask_loss_workspace_bytes(-1, H, W) == -1 and lib.tf_mask_loss_workspace_bytes(3, 0, W) == -1
    assert lib.tf_mask_loss_workspace_bytes(0, H, W) == 0

    def fwd(src=_p(src), tgt=_p(tgt), ps=_p(ps), sums=_p(sums), losses=_p(losses), ws=_p(ws), nbytes=nbytes, n=3, BQ=8, h=h, w=w, H=H, W=W,
            nb=3.0):
        return lib.tf_mask_loss_fwd_f32(src, tgt, ps, _p(pt), sums, losses, ws, nbytes, n, BQ, 6, h, w, H, W, 0.25, 2.0, nb, None)
    assert fwd() == 0
    assert fwd(src=None) == -1 and fwd(tgt=None) == -1 and fwd(ps=None) == -1 and fwd(sums=None) == -1 and fwd(losses=None) == -1
    assert fwd(src=None, tgt=None, ps=None, sums=None, ws=None, nbytes=0, n=0) == 0       # n == 0: only `losses` is needed
    assert fwd(n=-1) == -2 and fwd(BQ=0) == -2 and fwd(h=0) == -2 and fwd(w=-3) == -2 and fwd(nb=0.0) == -2
    assert fwd(h=H + 1) == -2 and fwd(w=W + 1) == -2                                      # no downsampling
    assert fwd(H=2 ** 24, ws=None) == -2 and fwd(H=2 ** 20, h=2 ** 12) == -2                # the coordinates leave int32
    assert fwd(src=_p(src) + 2) == -2 and fwd(sums=_p(sums) + 4) == -2 and fwd(losses=_p(losses) + 1) == -2
    assert fwd(ws=None) == -6 and fwd(nbytes=nbytes - 1) == -6 and fwd(ws=_p(ws) + 4) == -6

    def bwd(G=_p(G), src=_p(src), rp=_p(rp), sums=_p(sums), grad=_p(grad), n=3, h=h, H=H):
        return lib.tf_mask_loss_bwd_f32(G, src, _p(tgt), _p(pt), rp, sums, grad, n, 8, 6, h, w, H, W, 0.25, 2.0, 3.0, None)
    assert bwd() == 0
    assert bwd(G=None) == -1 and bwd(src=None) == -1 and bwd(rp=None) == -1 and bwd(sums=None) == -1 and bwd(grad=None) == -1
    assert bwd(G=None, src=None, sums=None, n=0) == 0
    assert bwd(h=0) == -2 and bwd(h=H + 1) == -2 and bwd(n=-1) == -2 and bwd(grad=_p(grad) + 2) == -2 and bwd(sums=_p(sums) + 4) == -2


# ---- the host side -----------------------------------------------------------------------------------------------------------------------
def test_mask_pairs_are_what_loss_masks_indexes():
    """build_mask_pairs against the index tensors loss_masks builds from the same pairs, on the padded stack."""
    case = M.Case((5, 7, 19, 23), 3, "unit", "box", seed=9)
    ps, pt, rp = criterion.build_mask_pairs(case.indices, M.Q, case.per_image)
    assert ps.dtype == np.int32 and pt.dtype == np.int32 and rp.dtype == np.int32
    assert ps.tolist() == case.pair_src.tolist() and pt.tolist() == case.pair_tgt.tolist() and rp.tolist() == case.row_pair.tolist()
    crit = Y.criterion_for(1, 0.25, 2.0)
    sb, sq = crit._get_src_permutation_idx(case.indices)
    tb, tt = crit._get_tgt_permutation_idx(case.indices)
    assert (sb * M.Q + sq).tolist() == ps.tolist() and (tb * case.per_image + tt).tolist() == pt.tolist()
    stack = criterion.nested_tensor_from_tensor_list([m for m in case.masks]).decompose()[0]
    assert torch.equal(stack.flatten(0, 1), case.tgt)
    empty = criterion.build_mask_pairs([(torch.zeros(0, dtype=torch.int64),) * 2] * 2, M.Q, 3)
    assert empty[0].size == 0 and empty[1].size == 0 and empty[2].tolist() == [-1] * 8


def test_mask_losses_applies():
    pm = torch.zeros(2, 4, 5, 7)
    tg = torch.zeros(6, 19, 23, dtype=torch.bool)
    assert not fused.mask_losses_applies(pm, tg)                         # not on the device
    with pytest.raises(ValueError):
        fused.mask_losses(pm, tg, torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 0.25, 2.0, 1.0)

    class OnDevice:   # what the predicate reads of a tensor, with is_cuda forced: the remaining conditions need no GPU
        def __init__(self, t, device="gpu0"):
            self.t, self.is_cuda, self.device, self.dtype, self.shape = t, True, device, t.dtype, t.shape

        def dim(self):
            return self.t.dim()

        def numel(self):
            return self.t.numel()

        def is_contiguous(self):
            return self.t.is_contiguous()
    ok = fused.mask_losses_applies
    assert ok(OnDevice(pm), OnDevice(tg)) and ok(OnDevice(pm), OnDevice(tg.view(torch.uint8)))
    assert not ok(OnDevice(pm.double()), OnDevice(tg)) and not ok(OnDevice(pm), OnDevice(tg.float()))
    assert not ok(OnDevice(pm.transpose(2, 3)), OnDevice(tg)) and not ok(OnDevice(pm), OnDevice(tg, "gpu1"))
    assert not ok(OnDevice(pm), OnDevice(tg[:, :4])) and not ok(OnDevice(pm), OnDevice(tg[:, :, :6])) and not ok(OnDevice(pm[0]), OnDevice(tg))


def test_switch_counter_and_todays_lines_without_a_gpu(monkeypatch):
    """Off by default; follows its environment variable; None returns to it; bumps the route epoch when its value changes; leaves
    set_fused alone.  With the switch off loss_masks never looks at the fused route; with it on a call the kernels do not take (CPU
    tensors here) runs today's lines and is counted under "torch"."""
    assert criterion.fused_masks_enabled() is False
    case = M.Case((5, 7, 19, 23), 3, "unit", "box", seed=10)
    crit = Y.criterion_for(1, 0.25, 2.0)
    outputs = {"pred_masks": case.pred_masks}

    def boom(*a, **k):
        raise AssertionError("the fused route was consulted with the switch off")
    monkeypatch.setattr(criterion.SetCriterion, "_loss_masks_fused", boom)
    criterion.fused_mask_counts(reset=True)
    want = crit.loss_masks(outputs, case.targets(), case.indices, case.num_boxes)
    assert criterion.fused_mask_counts() == {"own": 0, "torch": 0}
    monkeypatch.undo()
    assert torch.equal(torch.stack([want["loss_mask"], want["loss_dice"]]), M.torch_loss_masks(case, case.pred_masks))
    epoch = fused.route_epoch()
    assert criterion.set_fused_masks(True) is False and fused.route_epoch() == epoch + 1
    try:
        assert criterion.set_fused_masks(True) is True and fused.route_epoch() == epoch + 1     # no change of value: no new epoch
        assert criterion.fused_enabled() is False                                                # the other switch is its own
        got = crit.loss_masks(outputs, case.targets(), case.indices, case.num_boxes)
        assert criterion.fused_mask_counts() == {"own": 0, "torch": 1}
        assert got.keys() == want.keys() and all(torch.equal(got[k], want[k]) for k in want)
    finally:
        criterion.set_fused_masks(None)
    assert criterion.fused_masks_enabled() is False
    assert criterion.fused_mask_counts(reset=True)["torch"] == 1 and criterion.fused_mask_counts() == {"own": 0, "torch": 0}
    monkeypatch.setenv("TF_CRITERION_FUSED_MASKS", "1")
    assert criterion.fused_masks_enabled() and not criterion.fused_enabled()
    assert criterion.set_fused_masks(False) is True and not criterion.fused_masks_enabled()
    criterion.set_fused_masks(None)
    assert criterion.fused_masks_enabled()
    monkeypatch.setenv("TF_CRITERION_FUSED_MASKS", "0")
    assert not criterion.fused_masks_enabled()
