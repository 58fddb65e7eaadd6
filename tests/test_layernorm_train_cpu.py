"""CPU: the training path of the residual + LayerNorm sites (include/tf_fused.h: THE BACKWARD OF THE RESIDUAL LAYERNORM;
trackformer_amd/csrc/layernorm_bwd.h) on the emulated library -- the kernels' own source under the SIMT emulator -- against float64 with
the yardstick of tests/util_layernorm_train.py, plus the host logic of fused.layernorm_train that needs no GPU."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import emu_lib
from tests import util_layernorm_train as Y
from tests import util_norm_attn_numerics as NA

emu = pytest.mark.skipif(not emu_lib.available(), reason="no host clang++ for the emulated library")

CANARY = np.float32(-4321.5)
GUARD = 3            # canary rows behind dz, stats and the workspace


def _lib():
    return emu_lib.lib()   # bound from the headers (trackformer_amd._cabi.bind)


def _al(a):
    return None if a is None else emu_lib._aligned(np.asarray(a, dtype=np.float32))


def _p(a):
    return None if a is None else a.ctypes.data


def _np(t):
    return None if t is None else t.numpy()


def blocks_of(rows, C=8):
    """Row blocks of the backward's partition, from the library's own workspace size (2 C floats per block)."""
    nbytes = _lib().tf_add_layernorm_bwd_workspace_bytes(rows, C)
    assert nbytes > 0 and nbytes % (8 * C) == 0
    return nbytes // (8 * C)


def forward(x, res, gamma, beta, eps=Y.EPS):
    """tf_add_layernorm_train_f32 -> (out, stats [rows, 2]); canary rows behind both are checked."""
    x, res, gamma, beta = _al(x), _al(res), _al(gamma), _al(beta)
    rows, C = x.shape
    out = _al(np.full((rows + GUARD, C), CANARY))
    stats = _al(np.full((rows + GUARD, 2), CANARY))
    rc = _lib().tf_add_layernorm_train_f32(_p(x), _p(res), _p(gamma), _p(beta), _p(out), _p(stats), rows, C, ctypes.c_float(eps), None)
    assert rc == 0, rc
    assert emu_lib.last_kernel() == "add_layernorm_stats_f32"
    assert (out[rows:] == CANARY).all() and (stats[rows:] == CANARY).all()
    return out[:rows].copy(), stats[:rows].copy()


def backward(dy, x, res, gamma, stats, want=Y.OUTPUTS):
    """tf_add_layernorm_bwd_f32 -> {name: array} for the outputs in `want`; the workspace starts as NaN; canary rows behind dz and the
    workspace are checked; the kernels that ran are checked by name."""
    L = _lib()
    dy, x, res, gamma, stats = _al(dy), _al(x), _al(res), _al(gamma), _al(stats)
    rows, C = x.shape
    cols = "dgamma" in want or "dbeta" in want
    dz = _al(np.full((rows + GUARD, C), CANARY)) if "dz" in want else None
    dg = _al(np.full(C, np.nan)) if "dgamma" in want else None
    db = _al(np.full(C, np.nan)) if "dbeta" in want else None
    nbytes = L.tf_add_layernorm_bwd_workspace_bytes(rows, C)
    assert nbytes > 0
    nb = nbytes // (8 * C)
    ws = _al(np.full((nb + GUARD, 2 * C), np.nan)) if cols else None
    if cols:
        ws[nb:] = CANARY
    rc = L.tf_add_layernorm_bwd_f32(_p(dy), _p(x), _p(res), _p(gamma), _p(stats), _p(dz), _p(dg), _p(db), _p(ws), nbytes if cols else 0, rows, C,
                                    None)
    assert rc == 0, rc
    if want:
        assert emu_lib.last_kernel() == ("add_layernorm_bwd_reduce_f32" if cols else "add_layernorm_bwd_f32")
    if dz is not None:
        assert (dz[rows:] == CANARY).all(), "tf_add_layernorm_bwd_f32 wrote behind dz"
    if cols:
        assert (ws[nb:] == CANARY).all(), "tf_add_layernorm_bwd_f32 wrote behind its workspace"
        if all(a is None or np.isfinite(a).all() for a in (dy, x, res)):
            assert not np.isnan(ws[:nb]).any(), "a partial row was not written"
    return {"dz": None if dz is None else dz[:rows].copy(), "dgamma": dg, "dbeta": db}


def run_case(profile, dy_profile, rows, C, with_res, seed=None, want=Y.OUTPUTS):
    x, res, gamma, beta, dy = Y.operands(profile, dy_profile, rows, C, seed if seed is not None else rows + C, with_res=with_res)
    emu_lib.stats(reset=True)
    _, stats = forward(_np(x), _np(res), _np(gamma), _np(beta))
    got = backward(_np(dy), _np(x), _np(res), _np(gamma), stats, want)
    st = emu_lib.stats()
    assert st["divergent_ops"] == 0 and st["inactive_reads"] == 0, st
    ref = Y.reference(x, res, gamma, dy)
    fp32 = Y.fp32_formulation(x, res, gamma, beta, dy)
    what = "%s x %s [%d, %d]%s" % (profile, dy_profile, rows, C, " + res" if res is not None else "")
    Y.check({k: None if v is None else torch.from_numpy(v) for k, v in got.items()}, ref, fp32, rows, what)
    return got


# ---- the yardstick itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", NA.LN_PROFILES)
@pytest.mark.parametrize("rows,C", [(5, 256), (5, 288), (257, 288)])
def test_yardstick_holds_for_the_fp32_formulation_alone(rows, C, profile):
    for dy_profile in Y.DY_PROFILES:
        x, res, gamma, beta, dy = Y.operands(profile, dy_profile, rows, C, rows + C)
        Y.check_fp32_alone(Y.reference(x, res, gamma, dy), Y.fp32_formulation(x, res, gamma, beta, dy), rows,
                           "%s x %s [%d, %d]" % (profile, dy_profile, rows, C))


# ---- the kernels on the emulator -----------------------------------------------------------------------------------------------------
# (1, 4): one lane, one chunk; (3, 256): fewer rows than a workgroup has waves; (5, 260): 65 chunks, one lane in the second; (5, 288): 72
# chunks; (2, 4096): MAXCH 16; (257, 256): 17 row blocks, the last of one row; (3, 516): 129 chunks, MAXCH 4 with one lane in the third
# chunk and none in the fourth
SHAPES = [(1, 4), (3, 256), (5, 260), (5, 288), (2, 4096), (257, 256), (3, 516)]


@emu
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("rows,C", SHAPES)
def test_kernels_against_float64(rows, C, with_res):
    run_case("unit", "unit", rows, C, with_res)


@emu
@pytest.mark.parametrize("profile", NA.LN_PROFILES)
def test_every_profile_pair_against_float64(profile):
    for i, dy_profile in enumerate(Y.DY_PROFILES):
        run_case(profile, dy_profile, 5, 288, None if i % 2 == 0 else True, seed=17 + i)


def _boundary_rows(limit=600):
    """One row count on each side of every row-block boundary of the partition below `limit` rows (from the library itself)."""
    rows = []
    for r in range(1, limit):
        if blocks_of(r + 1) != blocks_of(r):
            rows += [r, r + 1]
    return sorted(set(rows))


@emu
@pytest.mark.parametrize("part", range(16))
def test_both_sides_of_every_row_block_boundary(part):
    rows_list = _boundary_rows()
    assert len(rows_list) >= 16 and rows_list[0] > 1, rows_list
    for rows in rows_list[part::16]:
        run_case("unit", "unit", rows, 8, with_res=rows % 3 == 0)


@emu
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("rows,C", [(5, 288), (37, 260)])
def test_each_subset_of_outputs_is_bitwise_the_full_call(rows, C, with_res):
    x, res, gamma, beta, dy = Y.operands("unit", "unit", rows, C, 3, with_res=with_res)
    _, stats = forward(_np(x), _np(res), _np(gamma), _np(beta))
    full = backward(_np(dy), _np(x), _np(res), _np(gamma), stats)
    for n in range(0, 3):
        for want in itertools.combinations(Y.OUTPUTS, n):
            emu_lib.stats(reset=True)
            got = backward(_np(dy), _np(x), _np(res), _np(gamma), stats, want)
            if not want:
                assert emu_lib.stats()["blocks"] == 0       # nothing asked for: nothing launched
            for name in Y.OUTPUTS:
                if name in want:
                    assert np.array_equal(got[name], full[name]), (want, name)
                else:
                    assert got[name] is None
    again = backward(_np(dy), _np(x), _np(res), _np(gamma), stats)
    assert all(np.array_equal(again[k], full[k]) for k in Y.OUTPUTS)


def _ulps(a, want64):
    """|a - want| in units of the fp32 spacing at `want` (float64 want, fp32 a)."""
    w32 = want64.astype(np.float32)
    ulp = np.abs(np.spacing(w32)).astype(np.float64)
    return np.abs(a.astype(np.float64) - want64) / ulp


@emu
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("rows,C", SHAPES)
def test_forward_is_the_inference_kernel_bit_for_bit_and_saves_its_statistics(rows, C, with_res):
    # offset30: a mean well away from zero, so that "2 ulp of the mean" measures the statistic and not the cancellation in its sum
    x, res, gamma, beta, _ = Y.operands("offset30", "unit", rows, C, rows + C, with_res=with_res)
    out, stats = forward(_np(x), _np(res), _np(gamma), _np(beta))
    assert np.array_equal(out, emu_lib.add_layernorm(_np(x), _np(res), _np(gamma), _np(beta), Y.EPS))
    z = (x if res is None else x + res).numpy().astype(np.float64)         # the fp32 sum, widened
    mean = z.mean(1)
    rstd = 1.0 / np.sqrt(z.var(1) + np.float64(np.float32(Y.EPS)))
    assert _ulps(stats[:, 0], mean).max() <= 2, _ulps(stats[:, 0], mean).max()
    assert _ulps(stats[:, 1], rstd).max() <= 2, _ulps(stats[:, 1], rstd).max()


@emu
def test_status_codes_in_order_before_any_work():
    L = _lib()
    one = ctypes.c_void_p(16)    # never dereferenced: validation fails first
    odd = ctypes.c_void_p(24)    # 8-byte aligned only
    big = 1 << 30
    eps = ctypes.c_float(1e-5)
    # the forward: NULL pointer -> -1 (even with bad dimensions), dimensions / alignment -> -2
    assert L.tf_add_layernorm_train_f32(one, None, one, one, one, None, 5, 258, eps, None) == -1
    assert L.tf_add_layernorm_train_f32(None, None, one, one, one, one, 5, 256, eps, None) == -1
    assert L.tf_add_layernorm_train_f32(one, None, one, one, one, one, 5, 258, eps, None) == -2
    assert L.tf_add_layernorm_train_f32(one, None, one, one, one, one, 5, 4100, eps, None) == -2
    assert L.tf_add_layernorm_train_f32(one, None, one, one, one, one, 0, 256, eps, None) == -2
    assert L.tf_add_layernorm_train_f32(one, odd, one, one, one, one, 5, 256, eps, None) == -2
    assert L.tf_add_layernorm_train_f32(one, None, one, one, one, ctypes.c_void_p(20), 5, 256, eps, None) == -2
    # the backward: NULL pointer -> -1 (even with bad dimensions and no workspace), dimensions / alignment -> -2 (even with a short
    # workspace), workspace -> -6
    assert L.tf_add_layernorm_bwd_f32(None, one, None, one, one, one, one, one, None, 0, 5, 258, None) == -1
    assert L.tf_add_layernorm_bwd_f32(one, one, None, one, None, one, one, one, None, 0, 5, 258, None) == -1
    assert L.tf_add_layernorm_bwd_f32(one, one, None, None, one, one, one, one, one, big, 5, 256, None) == -1
    assert L.tf_add_layernorm_bwd_f32(one, one, None, one, one, one, one, one, None, 0, 5, 258, None) == -2
    assert L.tf_add_layernorm_bwd_f32(one, one, None, one, one, one, one, one, None, 0, 5, 4100, None) == -2
    assert L.tf_add_layernorm_bwd_f32(one, one, None, one, one, one, one, one, None, 0, 0, 256, None) == -2
    assert L.tf_add_layernorm_bwd_f32(one, one, odd, one, one, one, one, one, None, 0, 5, 256, None) == -2
    assert L.tf_add_layernorm_bwd_f32(one, one, None, one, one, odd, one, one, None, 0, 5, 256, None) == -2
    assert L.tf_add_layernorm_bwd_f32(one, one, None, one, one, one, one, odd, None, 0, 5, 256, None) == -2
    need = L.tf_add_layernorm_bwd_workspace_bytes(5, 256)
    assert need == 2 * 256 * 4
    assert L.tf_add_layernorm_bwd_f32(one, one, None, one, one, one, one, one, None, big, 5, 256, None) == -6
    assert L.tf_add_layernorm_bwd_f32(one, one, None, one, one, one, one, None, one, need - 1, 5, 256, None) == -6
    assert L.tf_add_layernorm_bwd_f32(one, one, None, one, one, one, None, one, odd, big, 5, 256, None) == -6
    for rows, C in ((5, 258), (5, 4100), (0, 256), (-1, 256), (5, 0), (1 << 31, 256)):
        assert L.tf_add_layernorm_bwd_workspace_bytes(rows, C) == -1, (rows, C)
    # 16 rows per block up to 32 768 rows, at most 2048 blocks beyond
    assert [blocks_of(r) for r in (1, 16, 17, 32768, 32769, 44446, 10 ** 7)] == [1, 1, 2, 2048, 1928, 2021, 2048]


@emu
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
def test_non_finite_contract(with_res):
    rows, C = 21, 260
    x, res, gamma, beta, dy = Y.operands("unit", "unit", rows, C, 5, with_res=with_res)
    x, res, gamma, beta, dy = _np(x), _np(res), _np(gamma), _np(beta), _np(dy)
    _, stats = forward(x, res, gamma, beta)
    clean = backward(dy, x, res, gamma, stats)
    assert all(np.isfinite(v).all() for v in clean.values())
    others = np.arange(rows) != 6
    for bad in (np.nan, np.inf):
        # in dy[6, 257]: row 6 of dz is non-finite, the other rows keep their bits; column 257 of dgamma / dbeta and no other
        d2 = dy.copy()
        d2[6, 257] = bad
        got = backward(d2, x, res, gamma, stats)
        assert np.array_equal(got["dz"][others], clean["dz"][others]) and not np.isfinite(got["dz"][6]).any()
        planted = np.arange(C) == 257
        for name in ("dgamma", "dbeta"):
            assert not np.isfinite(got[name][planted]).any(), name
            assert np.array_equal(got[name][~planted], clean[name][~planted]), name
        if bad is np.nan:
            assert np.isnan(got["dgamma"][257]) and np.isnan(got["dbeta"][257])
        # in x[6, 3] (and in res[6, 3]): the row's mean is lost, so is every xh[6, c] -- every dgamma[c] is NaN in exact arithmetic
        # too; dbeta does not read x
        for which in ("x", "res") if with_res else ("x",):
            x2, r2 = x.copy(), None if res is None else res.copy()
            (x2 if which == "x" else r2)[6, 3] = bad
            _, st2 = forward(x2, r2, gamma, beta)
            assert np.array_equal(st2[others], stats[others]) and not np.isfinite(st2[6]).any()
            got = backward(dy, x2, r2, gamma, st2)
            assert np.array_equal(got["dz"][others], clean["dz"][others]) and np.isnan(got["dz"][6]).all(), which
            assert np.isnan(got["dgamma"]).all() and np.array_equal(got["dbeta"], clean["dbeta"]), which


# ---- host logic that needs no GPU ----------------------------------------------------------------------------------------------------
def test_switch_and_environment_variable_round_trip(monkeypatch):
    from trackformer_amd import fused
    monkeypatch.delenv("TF_LAYERNORM_TRAIN", raising=False)
    fused.set_layernorm_training(None)
    try:
        assert fused.layernorm_training_enabled() is False          # the default is off
        monkeypatch.setenv("TF_LAYERNORM_TRAIN", "1")
        assert fused.layernorm_training_enabled() is True
        monkeypatch.setenv("TF_LAYERNORM_TRAIN", "0")
        assert fused.layernorm_training_enabled() is False
        epoch = fused.route_epoch()
        assert fused.set_layernorm_training(True) is False
        assert fused.layernorm_training_enabled() is True and fused.route_epoch() == epoch + 1
        assert fused.set_layernorm_training(True) is True and fused.route_epoch() == epoch + 1
        assert fused.set_layernorm_training(False) is True
        assert fused.layernorm_training_enabled() is False
        assert set(fused.layernorm_train_counts()) == {"own", "torch"}
    finally:
        fused.set_layernorm_training(None)


def test_layernorm_train_declines_what_the_kernels_do_not_take():
    from trackformer_amd import fused
    fused.layernorm_train_counts(reset=True)
    norm = torch.nn.LayerNorm(256)
    x = torch.randn(5, 256, requires_grad=True)
    assert fused.layernorm_train(x, torch.randn(5, 256), norm) is None                              # CPU tensors
    assert fused.layernorm_train(x.double(), None, torch.nn.LayerNorm(256).double()) is None        # float64
    assert fused.layernorm_train(x, None, torch.nn.LayerNorm(256, elementwise_affine=False)) is None
    assert fused.layernorm_train(torch.randn(5, 258), None, torch.nn.LayerNorm(258)) is None        # C % 4
    assert not fused.layernorm_train_route(x)
    assert fused.layernorm_train_counts(reset=True) == {"own": 0, "torch": 4}
    assert fused.layernorm_train_counts() == {"own": 0, "torch": 0}


def test_switch_off_builds_todays_graph(monkeypatch):
    from trackformer_amd import fused
    monkeypatch.delenv("TF_LAYERNORM_TRAIN", raising=False)
    fused.set_layernorm_training(None)
    fused.layernorm_train_counts(reset=True)
    norm = torch.nn.LayerNorm(32)
    x, res = torch.randn(3, 32, requires_grad=True), torch.randn(3, 32, requires_grad=True)
    for on in (False, True):      # (on: a CPU tensor is not routed either)
        prev = fused.set_layernorm_training(on)
        try:
            y = fused.residual_norm(x, res, norm, inference=False)
        finally:
            fused.set_layernorm_training(prev)
        assert type(y.grad_fn).__name__ == "NativeLayerNormBackward0"
        assert [type(f[0]).__name__ for f in y.grad_fn.next_functions][0] == "AddBackward0"
        assert torch.equal(y, norm(x + res))
    assert fused.layernorm_train_counts() == {"own": 0, "torch": 0}
