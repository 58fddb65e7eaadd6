"""CPU: dropout inside the training kernels (include/tf_fused.h: DROPOUT INSIDE THE TRAINING KERNELS; trackformer_amd/csrc/dropout_rng.h,
dropout_train.h) on the emulated library -- the kernels' own source under the SIMT emulator -- against the numpy restatement of the
generator contract and the float64 yardstick of tests/util_dropout_train.py, plus the host logic of fused.set_dropout_training that needs
no GPU.

The contract of tf_relu_dropout_bwd_f32 checked here: out = y > 0 ? fl(dy scale) : 0 -- y = +0, y = -0, a negative y and a NaN y all give
exactly +0 (whatever dy holds, NaN and inf included); a NaN dy under a positive y is NaN."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import emu_lib
from tests import util_dropout_train as D
from tests import util_layernorm_train as Y
from tests import util_norm_attn_numerics as NA

emu = pytest.mark.skipif(not emu_lib.available(), reason="no host clang++ for the emulated library")

CANARY = np.float32(-4321.5)
GUARD = 3
SEED, OFFSET = 0x9E3779B97F4A7C15 - 2 ** 64, 0x7FEDCBA987654321   # both high halves set (the seed negative as an int64)


def _lib():
    return emu_lib.lib()   # bound from the headers (trackformer_amd._cabi.bind)


def _al(a):
    return None if a is None else emu_lib._aligned(np.asarray(a, dtype=np.float32))


def _p(a):
    return None if a is None else a.ctypes.data


def _np(t):
    return None if t is None else t.numpy()


def _rng(seed=SEED, offset=OFFSET):
    return np.array([seed, offset], dtype=np.int64)


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN, ids=["zeros", "ones", "pi"])
def test_known_answers_of_the_restatement(counter, key, want):
    got = tuple(int(w[0]) for w in D.philox4x32_10(counter, key))
    assert got == want, [hex(v) for v in got]


def test_threshold_and_scale_of_the_restatement():
    assert D.threshold(0.5) == 2 ** 31 and D.threshold(2.0 ** -32) == 1 and D.threshold(2.0 ** -33) == 0
    assert D.threshold(0.1) == int(np.float64(np.float32(0.1)) * 2 ** 32) == 13421773 * 32     # float(0.1f) = 13421773 . 2^-27
    assert D.threshold(0.9999) < 2 ** 32
    assert D.scale32(0.5) == np.float32(2.0) and D.scale32(0.1).dtype == np.float32
    # element 4 g + j is word j of group g, and `first` only shifts the counter
    w = D.words(SEED, OFFSET, 0, 16)
    assert np.array_equal(D.words(SEED, OFFSET, 8, 8), w[8:])
    g1 = D.philox4x32_10((1, 0, OFFSET & 0xFFFFFFFF, OFFSET >> 32), (SEED & 0xFFFFFFFF, (SEED >> 32) & 0xFFFFFFFF))
    assert [int(v[0]) for v in g1] == [int(v) for v in w[4:8]]


# fixed (seed, offset) for the keep fraction: chosen so that the restatement alone passes (asserted first)
FRACTION_STREAMS = [(12345, 0), (SEED, OFFSET)]


def _fraction_ok(keep, p):
    n = keep.size
    q = 1.0 - D.threshold(p) / 2.0 ** 32
    return abs(float(keep.sum()) - n * q) <= 5.0 * (n * q * (1.0 - q)) ** 0.5


@emu
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed,offset", FRACTION_STREAMS)
def test_keep_fraction(seed, offset, p):
    n = 65536
    assert _fraction_ok(D.keep_mask(seed, offset, p, n), p), "the restatement itself misses the binomial bound for these constants"
    assert _fraction_ok(keep_u8(_rng(seed, offset), p, 0, n), p)


# ---- tf_dropout_keep_u8 ----------------------------------------------------------------------------------------------------------------
def keep_u8(rng, p, first, n):
    buf = np.full(n + 16, 0xA5, np.uint8)
    off = (-buf.ctypes.data) % 4
    keep = buf[off:off + n + 8]
    rc = _lib().tf_dropout_keep_u8(_p(rng), ctypes.c_float(p), first, n, _p(keep), None)
    assert rc == 0, rc
    assert emu_lib.last_kernel() == "dropout_keep_u8"
    assert (keep[n:] == 0xA5).all(), "tf_dropout_keep_u8 wrote behind its output"
    return keep[:n].copy()


@emu
@pytest.mark.parametrize("first", [0, 2 ** 34], ids=["first0", "first2p34"])
@pytest.mark.parametrize("n", [4, 260, 4100])
@pytest.mark.parametrize("p", [2.0 ** -31, 0.1, 0.5, 0.9999], ids=["tiny", "0.1", "0.5", "0.9999"])
def test_keep_u8_is_the_restatement_byte_for_byte(p, n, first):
    got = keep_u8(_rng(), p, first, n)
    want = D.keep_mask(SEED, OFFSET, p, n, first)
    assert np.array_equal(got, want)
    assert set(np.unique(got)) <= {0, 1}


# ---- the LayerNorm pair ----------------------------------------------------------------------------------------------------------------
def forward(x, res, gamma, beta, rng, p, eps=D.EPS):
    x, res, gamma, beta = _al(x), _al(res), _al(gamma), _al(beta)
    rows, C = x.shape
    out = _al(np.full((rows + GUARD, C), CANARY))
    stats = _al(np.full((rows + GUARD, 2), CANARY))
    rc = _lib().tf_add_dropout_layernorm_train_f32(_p(x), _p(res), _p(gamma), _p(beta), _p(rng), ctypes.c_float(p), _p(out), _p(stats), rows, C,
                                                   ctypes.c_float(eps), None)
    assert rc == 0, rc
    assert emu_lib.last_kernel() == "add_dropout_layernorm_stats_f32"
    assert (out[rows:] == CANARY).all() and (stats[rows:] == CANARY).all()
    return out[:rows].copy(), stats[:rows].copy()


def backward(dy, x, res, gamma, stats, rng, p, want=D.GRADS):
    """tf_add_dropout_layernorm_bwd_f32 -> {name: array or None}; NaN-filled workspace, canary rows behind dx, dres and the workspace."""
    L = _lib()
    dy, x, res, gamma, stats = _al(dy), _al(x), _al(res), _al(gamma), _al(stats)
    rows, C = x.shape
    cols = "dgamma" in want or "dbeta" in want
    dx = _al(np.full((rows + GUARD, C), CANARY)) if "dx" in want else None
    dr = _al(np.full((rows + GUARD, C), CANARY)) if "dres" in want else None
    dg = _al(np.full(C, np.nan)) if "dgamma" in want else None
    db = _al(np.full(C, np.nan)) if "dbeta" in want else None
    nbytes = L.tf_add_layernorm_bwd_workspace_bytes(rows, C)
    assert nbytes > 0
    nb = nbytes // (8 * C)
    ws = _al(np.full((nb + GUARD, 2 * C), np.nan)) if cols else None
    if cols:
        ws[nb:] = CANARY
    rc = L.tf_add_dropout_layernorm_bwd_f32(_p(dy), _p(x), _p(res), _p(gamma), _p(stats), _p(rng), ctypes.c_float(p), _p(dx), _p(dr), _p(dg),
                                            _p(db), _p(ws), nbytes if cols else 0, rows, C, None)
    assert rc == 0, rc
    if want:
        assert emu_lib.last_kernel() == ("add_layernorm_bwd_reduce_f32" if cols else "add_dropout_layernorm_bwd_f32")
    for a, name in ((dx, "dx"), (dr, "dres")):
        if a is not None:
            assert (a[rows:] == CANARY).all(), "wrote behind " + name
    if cols:
        assert (ws[nb:] == CANARY).all(), "wrote behind the workspace"
        assert not np.isnan(ws[:nb]).any(), "a partial row was not written"
    return {"dx": None if dx is None else dx[:rows].copy(), "dres": None if dr is None else dr[:rows].copy(), "dgamma": dg, "dbeta": db}


def run_case(profile, dy_profile, rows, C, p=0.1, seed=None):
    x, res, gamma, beta, dy = D.operands(profile, dy_profile, rows, C, seed if seed is not None else rows + C)
    rng = _rng()
    keep = torch.from_numpy(D.keep_mask(SEED, OFFSET, p, rows * C).astype(bool)).view(rows, C)
    emu_lib.stats(reset=True)
    out, stats = forward(_np(x), _np(res), _np(gamma), _np(beta), rng, p)
    got = backward(_np(dy), _np(x), _np(res), _np(gamma), stats, rng, p)
    st = emu_lib.stats()
    assert st["divergent_ops"] == 0 and st["inactive_reads"] == 0, st
    got["out"] = out
    ref = D.reference(x, res, gamma, beta, dy, keep, p)
    fp32 = D.fp32_formulation(x, res, gamma, beta, dy, keep, p)
    what = "%s x %s [%d, %d] p %g" % (profile, dy_profile, rows, C, p)
    D.check({k: torch.from_numpy(v) for k, v in got.items()}, ref, fp32, rows, keep, what)
    return got


@pytest.mark.parametrize("profile", NA.LN_PROFILES)
def test_yardstick_holds_for_the_fp32_formulation_alone(profile):
    rows, C = 37, 288
    keep = torch.from_numpy(D.keep_mask(SEED, OFFSET, 0.1, rows * C).astype(bool)).view(rows, C)
    for dy_profile in Y.DY_PROFILES:
        x, res, gamma, beta, dy = D.operands(profile, dy_profile, rows, C, rows + C)
        D.check_fp32_alone(D.reference(x, res, gamma, beta, dy, keep, 0.1), D.fp32_formulation(x, res, gamma, beta, dy, keep, 0.1), rows,
                           "%s x %s" % (profile, dy_profile))


# (1, 4): one lane; (5, 260): 65 chunks; (257, 288): 17 row blocks, the last of one row; (64, 4096): MAXCH 16; (4099, 256): many blocks;
# (3, 516): 129 chunks, MAXCH 4 with one lane in the third chunk and none in the fourth, fewer rows than a workgroup has waves
SHAPES = [(1, 4), (5, 260), (257, 288), (64, 4096), (4099, 256), (3, 516)]


@emu
@pytest.mark.parametrize("rows,C", SHAPES)
def test_kernels_against_float64(rows, C):
    run_case("unit", "unit", rows, C)


@emu
@pytest.mark.parametrize("profile", NA.LN_PROFILES)
def test_every_profile_against_float64(profile):
    for i, dy_profile in enumerate(Y.DY_PROFILES):
        run_case(profile, dy_profile, 5, 260, p=(0.1, 0.5)[i % 2], seed=17 + i)


@emu
@pytest.mark.parametrize("rows,C", [(5, 288), (37, 260)])
def test_each_subset_of_outputs_is_bitwise_the_full_call(rows, C):
    x, res, gamma, beta, dy = D.operands("unit", "unit", rows, C, 3)
    rng = _rng()
    _, stats = forward(_np(x), _np(res), _np(gamma), _np(beta), rng, 0.1)
    full = backward(_np(dy), _np(x), _np(res), _np(gamma), stats, rng, 0.1)
    for n in range(0, 4):
        for want in itertools.combinations(D.GRADS, n):     # dx only, dres only, frozen affine, ...
            emu_lib.stats(reset=True)
            got = backward(_np(dy), _np(x), _np(res), _np(gamma), stats, rng, 0.1, want)
            if not want:
                assert emu_lib.stats()["blocks"] == 0       # nothing asked for: nothing launched
            for name in D.GRADS:
                if name in want:
                    assert np.array_equal(got[name], full[name]), (want, name)
                else:
                    assert got[name] is None
    # x itself as res (the site norm(x + dropout(x))): inputs may alias
    out2, st2 = forward(_np(x), _np(x), _np(gamma), _np(beta), rng, 0.1)
    xa, ga, be = _al(_np(x)), _al(_np(gamma)), _al(_np(beta))
    out = _al(np.full((rows, C), CANARY))
    sts = _al(np.full((rows, 2), CANARY))
    assert _lib().tf_add_dropout_layernorm_train_f32(_p(xa), _p(xa), _p(ga), _p(be), _p(rng), ctypes.c_float(0.1), _p(out),
                                                     _p(sts), rows, C, ctypes.c_float(D.EPS), None) == 0
    assert np.array_equal(out, out2) and np.array_equal(sts, st2)


@emu
def test_a_dropped_element_is_a_select_not_a_product():
    """inf / NaN in res where the mask drops it reaches nothing; dres is exactly +0 there."""
    rows, C, p = 9, 260, 0.5
    x, res, gamma, beta, dy = (_np(t) for t in D.operands("unit", "unit", rows, C, 5))
    rng = _rng()
    keep = D.keep_mask(SEED, OFFSET, p, rows * C).astype(bool).reshape(rows, C)
    out, stats = forward(x, res, gamma, beta, rng, p)
    clean = backward(dy, x, res, gamma, stats, rng, p)
    r2 = res.copy()
    r2[~keep] = np.where(np.arange((~keep).sum()) % 2 == 0, np.inf, np.nan)
    out2, stats2 = forward(x, r2, gamma, beta, rng, p)
    got = backward(dy, x, r2, gamma, stats2, rng, p)
    assert np.array_equal(out, out2) and np.array_equal(stats, stats2)
    assert all(np.array_equal(got[k], clean[k]) for k in D.GRADS)
    assert (got["dres"][~keep] == 0).all() and not np.signbit(got["dres"][~keep]).any()


# ---- the element-wise pair -------------------------------------------------------------------------------------------------------------
@emu
@pytest.mark.parametrize("n", [4, 260, 4100, 300004])
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9999])
def test_dropout_inplace_bit_for_bit(p, n):
    g = np.random.default_rng(n)
    y0 = (g.standard_normal(n) * np.exp2(g.integers(-20, 20, n))).astype(np.float32)
    y0[:4] = [np.inf, np.nan, -0.0, 1e-45]
    buf = _al(np.concatenate([y0, np.full(8, CANARY, np.float32)]))
    rc = _lib().tf_dropout_inplace_f32(_p(buf), _p(_rng()), ctypes.c_float(p), n, None)
    assert rc == 0 and emu_lib.last_kernel() == "dropout_inplace_f32"
    assert (buf[n:] == CANARY).all()
    keep = D.keep_mask(SEED, OFFSET, p, n).astype(bool)
    with np.errstate(all="ignore"):
        want = np.where(keep, y0 * D.scale32(p), np.float32(0.0)).astype(np.float32)
    assert np.array_equal(buf[:n].view(np.uint32), want.view(np.uint32))


@emu
@pytest.mark.parametrize("n", [4, 260, 4100])
def test_relu_dropout_bwd_against_its_definition(n):
    p = 0.1
    g = np.random.default_rng(n)
    y = np.maximum(g.standard_normal(n), 0).astype(np.float32)
    dy = g.standard_normal(n).astype(np.float32)
    y[:4] = [0.0, -0.0, np.nan, -1.0]
    dy[:4] = [np.nan, np.inf, 3.0, np.nan]
    if n > 8:
        y[4:8] = [1e-45, 2.0, np.inf, 1.0]
        dy[4:8] = [1.0, np.nan, 1.0, np.inf]
    out, dy, y = _al(np.full(n + 8, CANARY)), _al(dy), _al(y)
    rc = _lib().tf_relu_dropout_bwd_f32(_p(dy), _p(y), ctypes.c_float(p), _p(out), n, None)
    assert rc == 0 and emu_lib.last_kernel() == "relu_dropout_bwd_f32"
    assert (out[n:] == CANARY).all()
    with np.errstate(all="ignore"):
        want = np.where(y > 0, dy * D.scale32(p), np.float32(0.0)).astype(np.float32)
    assert np.array_equal(out[:n].view(np.uint32), want.view(np.uint32))
    assert (out[:4].view(np.uint32) == 0).all()        # y = +0, -0, NaN, negative: exactly +0 whatever dy holds


@emu
def test_ffn_identity_the_dropped_activation_encodes_both_decisions():
    """relu_dropout_bwd(dy, dropout(relu(h))) == threshold_backward(dy keep scale, relu(h)) bit for bit (finite operands)."""
    n, p = 4100, 0.1
    g = np.random.default_rng(1)
    h, dy = g.standard_normal(n).astype(np.float32), g.standard_normal(n).astype(np.float32)
    a = np.maximum(h, 0)
    buf = _al(a)
    assert _lib().tf_dropout_inplace_f32(_p(buf), _p(_rng()), ctypes.c_float(p), n, None) == 0
    out, dy = _al(np.zeros(n)), _al(dy)
    assert _lib().tf_relu_dropout_bwd_f32(_p(dy), _p(buf), ctypes.c_float(p), _p(out), n, None) == 0
    keep = D.keep_mask(SEED, OFFSET, p, n).astype(np.float32)
    want = np.where(a > 0, dy * keep * D.scale32(p), np.float32(0)).astype(np.float32)
    assert np.array_equal(out, want)


# ---- status codes ----------------------------------------------------------------------------------------------------------------------
@emu
def test_bad_p_is_refused_by_every_entry_and_status_codes_come_in_order():
    L = _lib()
    one, odd, cf = ctypes.c_void_p(16), ctypes.c_void_p(24), ctypes.c_float
    eps = cf(1e-5)
    big = 1 << 30
    for bad in (0.0, -0.1, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
        p = cf(bad)
        assert L.tf_dropout_keep_u8(one, p, 0, 4, one, None) == -2, bad
        assert L.tf_add_dropout_layernorm_train_f32(one, one, one, one, one, p, one, one, 5, 256, eps, None) == -2, bad
        assert L.tf_add_dropout_layernorm_bwd_f32(one, one, one, one, one, one, p, one, one, one, one, one, big, 5, 256, None) == -2, bad
        assert L.tf_dropout_inplace_f32(one, one, p, 4, None) == -2, bad
        assert L.tf_relu_dropout_bwd_f32(one, one, p, one, 4, None) == -2, bad
    p = cf(0.1)
    # NULL first (res is required), then dimensions / alignment, then the workspace
    assert L.tf_add_dropout_layernorm_train_f32(one, None, one, one, one, p, one, one, 5, 258, eps, None) == -1
    assert L.tf_add_dropout_layernorm_train_f32(one, one, one, one, None, p, one, one, 5, 256, eps, None) == -1
    assert L.tf_add_dropout_layernorm_train_f32(one, one, one, one, one, p, one, one, 5, 258, eps, None) == -2
    assert L.tf_add_dropout_layernorm_train_f32(one, one, one, one, one, p, one, one, 5, 4100, eps, None) == -2
    assert L.tf_add_dropout_layernorm_train_f32(one, odd, one, one, one, p, one, one, 5, 256, eps, None) == -2
    assert L.tf_add_dropout_layernorm_train_f32(one, one, one, one, ctypes.c_void_p(20), p, one, one, 5, 256, eps, None) == -2
    assert L.tf_add_dropout_layernorm_bwd_f32(one, one, None, one, one, one, p, one, one, one, one, None, 0, 5, 258, None) == -1
    assert L.tf_add_dropout_layernorm_bwd_f32(one, one, one, one, one, None, p, one, one, one, one, None, 0, 5, 256, None) == -1
    assert L.tf_add_dropout_layernorm_bwd_f32(one, one, one, one, one, one, p, one, one, one, one, None, 0, 5, 258, None) == -2
    assert L.tf_add_dropout_layernorm_bwd_f32(one, one, one, one, one, one, p, one, odd, one, one, one, big, 5, 256, None) == -2
    assert L.tf_add_dropout_layernorm_bwd_f32(one, one, one, one, one, one, p, one, one, one, one, None, big, 5, 256, None) == -6
    assert L.tf_add_dropout_layernorm_bwd_f32(one, one, one, one, one, one, p, one, one, None, one, one, 2 * 256 * 4 - 1, 5, 256, None) == -6
    assert L.tf_dropout_keep_u8(None, p, 0, 4, one, None) == -1
    assert L.tf_dropout_keep_u8(one, p, 2, 4, one, None) == -2
    assert L.tf_dropout_keep_u8(one, p, 0, 6, one, None) == -2
    assert L.tf_dropout_keep_u8(one, p, -4, 4, one, None) == -2
    assert L.tf_dropout_keep_u8(one, p, 0, 4, ctypes.c_void_p(18), None) == -2
    assert L.tf_dropout_inplace_f32(None, one, p, 4, None) == -1
    assert L.tf_dropout_inplace_f32(one, one, p, 6, None) == -2
    assert L.tf_dropout_inplace_f32(odd, one, p, 4, None) == -2
    assert L.tf_relu_dropout_bwd_f32(one, None, p, one, 4, None) == -1
    assert L.tf_relu_dropout_bwd_f32(one, one, p, odd, 4, None) == -2


# ---- host logic that needs no GPU ------------------------------------------------------------------------------------------------------
@pytest.fixture
def clean_switches(monkeypatch):
    from trackformer_amd import fused
    for var in ("TF_DROPOUT_TRAIN", "TF_LAYERNORM_TRAIN", "TF_SPLIT_LINEAR_TRAIN"):
        monkeypatch.delenv(var, raising=False)
    fused.set_dropout_training(None)
    fused.dropout_train_counts(reset=True)
    yield fused
    fused.set_dropout_training(None)
    fused.set_layernorm_training(None)
    fused.set_split_linear_training(None)
    fused.dropout_train_counts(reset=True)


def test_switch_and_environment_precedence(clean_switches, monkeypatch):
    fused = clean_switches
    assert fused.dropout_training_enabled() is False                       # the default is off
    monkeypatch.setenv("TF_DROPOUT_TRAIN", "1")
    assert fused.dropout_training_enabled() is True
    monkeypatch.setenv("TF_DROPOUT_TRAIN", "reference")
    assert fused.dropout_training_enabled() == "reference"
    monkeypatch.setenv("TF_DROPOUT_TRAIN", "0")
    assert fused.dropout_training_enabled() is False
    epoch = fused.route_epoch()
    assert fused.set_dropout_training(True) is False
    assert fused.dropout_training_enabled() is True and fused.route_epoch() == epoch + 1
    assert fused.set_dropout_training(True) is True and fused.route_epoch() == epoch + 1
    assert fused.set_dropout_training("reference") is True
    assert fused.dropout_training_enabled() == "reference" and fused.route_epoch() == epoch + 2
    monkeypatch.setenv("TF_DROPOUT_TRAIN", "1")
    assert fused.set_dropout_training(False) == "reference"                # a set value wins over the variable
    assert fused.dropout_training_enabled() is False
    assert fused.set_dropout_training(None) is False
    assert fused.dropout_training_enabled() is True                        # None: the variable again
    assert fused.dropout_train_counts() == {"ln_own": 0, "ln_torch": 0, "ffn_own": 0, "ffn_torch": 0}
    assert fused.dropout_scale(0.1) == float(D.scale32(0.1)) and fused.dropout_scale(0.5) == 2.0


class _Calls:
    """Counts the forward calls of modules through forward hooks."""

    def __init__(self, modules):
        self.n = {name: 0 for name in modules}
        self.handles = [m.register_forward_hook(lambda mod, a, out, name=name: self.n.__setitem__(name, self.n[name] + 1))
                        for name, m in modules.items()]

    def close(self):
        for h in self.handles:
            h.remove()


def _forbid_own_entries(monkeypatch, fused):
    def boom(*a, **k):
        raise AssertionError("an own dropout entry was reached")
    for name in ("dropout_rng", "dropout_keep"):
        monkeypatch.setattr(fused, name, boom)
    monkeypatch.setattr(fused._DropoutLayerNormTrain, "apply", boom)
    monkeypatch.setattr(fused._LinearDropoutTrain, "apply", boom)


@pytest.mark.parametrize("mode", [False, True, "reference"])
def test_host_tensors_run_todays_lines_with_one_dropout_call_per_site(clean_switches, monkeypatch, mode):
    """Switch off: the site's nn.Dropout is called exactly once per site at the point it was called before, the generator is consumed
    as before and the own entries are never reached.  Switch on: host tensors are not covered -- the same lines, counted *_torch."""
    fused = clean_switches
    from trackformer_amd.deformable_transformer import DeformableTransformerEncoderLayer
    _forbid_own_entries(monkeypatch, fused)
    torch.manual_seed(3)
    layer = DeformableTransformerEncoderLayer(d_model=32, d_ffn=64, dropout=0.1, n_levels=1, n_heads=8, n_points=2).train()
    src = torch.randn(2, 12, 32)
    sites = {"dropout2": layer.dropout2, "dropout3": layer.dropout3}
    calls = _Calls(sites)
    try:
        fused.set_dropout_training(mode)
        fused.set_layernorm_training(True)
        fused.set_split_linear_training(True)
        torch.manual_seed(11)
        got = layer.forward_ffn(src)
        after = torch.rand(1)
    finally:
        calls.close()
    assert calls.n == {"dropout2": 1, "dropout3": 1}
    # the parent commit's lines, under the same seed: the same result and the same generator state afterwards
    torch.manual_seed(11)
    hidden = layer.dropout2(torch.relu(layer.linear1(src)))
    want = layer.norm2(src + layer.dropout3(layer.linear2(hidden)))
    assert torch.equal(got, want) and torch.equal(after, torch.rand(1))
    assert type(got.grad_fn).__name__ == "NativeLayerNormBackward0"
    want_counts = {"ln_own": 0, "ln_torch": 1, "ffn_own": 0, "ffn_torch": 1} if mode is True else \
        {"ln_own": 0, "ln_torch": 0, "ffn_own": 0, "ffn_torch": 0}
    assert fused.dropout_train_counts() == want_counts


def test_p_zero_and_eval_mode_fall_through_uncounted(clean_switches, monkeypatch):
    fused = clean_switches
    _forbid_own_entries(monkeypatch, fused)
    fused.set_dropout_training(True)
    norm = torch.nn.LayerNorm(32)
    x, res = torch.randn(3, 32, requires_grad=True), torch.randn(3, 32, requires_grad=True)
    seen = []
    monkeypatch.setattr(fused, "layernorm_train_route", lambda t: seen.append(t) or False)
    for drop in (torch.nn.Dropout(0.0).train(), torch.nn.Dropout(0.1).eval(), torch.nn.Dropout(1.0).eval()):
        calls = _Calls({"d": drop})
        y = fused.residual_norm(x, res, norm, inference=False, dropout=drop)
        calls.close()
        assert calls.n == {"d": 1} and torch.equal(y, norm(x + res))
        assert fused.dropout_residual_norm(x, res, norm, drop) is None
        assert fused.dropout_ffn_hidden(x, torch.nn.Linear(32, 64), True, drop) is None
    assert len(seen) == 3                     # today's layernorm_train question was asked each time, after the dropout
    assert fused.dropout_train_counts() == {"ln_own": 0, "ln_torch": 0, "ffn_own": 0, "ffn_torch": 0}


def test_parent_route_off_is_counted_torch(clean_switches, monkeypatch):
    """Switch on, parent routes off (and host tensors): an active site keeps today's lines and is counted."""
    fused = clean_switches
    _forbid_own_entries(monkeypatch, fused)
    fused.set_dropout_training(True)
    drop = torch.nn.Dropout(0.1).train()
    norm = torch.nn.LayerNorm(32)
    x, res = torch.randn(3, 32), torch.randn(3, 32)
    assert fused.dropout_residual_norm(x, res, norm, drop) is None
    assert fused.dropout_ffn_hidden(x, torch.nn.Linear(32, 64), True, drop) is None
    assert fused.dropout_ffn_hidden(x, torch.nn.Linear(32, 64), False, drop) is None      # not a ReLU
    assert fused.dropout_train_counts(reset=True) == {"ln_own": 0, "ln_torch": 1, "ffn_own": 0, "ffn_torch": 2}
    assert fused.linear_train(x, torch.randn(64, 32), None, relu=True, dropout=drop) is None    # a host tensor
    assert fused.linear_train(x, torch.randn(64, 32), None, relu=False, dropout=drop) is None
    fused.set_dropout_training("reference")
    assert fused.dropout_residual_norm(x, res, norm, drop) is None                          # reference mode is for the device
    assert fused.dropout_ffn_hidden(x, torch.nn.Linear(32, 64), True, drop) is None
    assert fused.dropout_train_counts() == {"ln_own": 0, "ln_torch": 0, "ffn_own": 0, "ffn_torch": 0}


def test_reference_mode_computes_with_the_mask_of_the_library(clean_switches, monkeypatch):
    """"reference" with the device's two primitives replaced by the restatement (no GPU here): norm(x + res keep scale) and
    relu(linear(x)) keep scale, one rng draw per site, in site order, float64 included."""
    fused = clean_switches
    draws = []

    def fake_rng(device):
        draws.append(torch.tensor([SEED + len(draws), OFFSET], dtype=torch.int64))
        return draws[-1]

    def fake_keep(rng, p, n, first=0):
        return torch.from_numpy(D.keep_mask(int(rng[0]), int(rng[1]), p, n, first))

    monkeypatch.setattr(fused, "dropout_rng", fake_rng)
    monkeypatch.setattr(fused, "dropout_keep", fake_keep)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    fused.set_dropout_training("reference")
    drop = torch.nn.Dropout(0.1).train()
    for dtype in (torch.float32, torch.float64):
        del draws[:]
        norm, lin = torch.nn.LayerNorm(32).to(dtype), torch.nn.Linear(32, 64).to(dtype)
        x, res = torch.randn(3, 32, dtype=dtype), torch.randn(3, 32, dtype=dtype)
        y = fused.dropout_residual_norm(x, res, norm, drop)
        h = fused.dropout_ffn_hidden(x, lin, True, drop)
        assert len(draws) == 2
        k0 = D.keep_of(draws[0], 0.1, (3, 32)).to(dtype)
        k1 = D.keep_of(draws[1], 0.1, (3, 64)).to(dtype)
        s = float(D.scale32(0.1))
        assert torch.equal(y, norm(x + res * (k0 * s))) and y.dtype == dtype
        assert torch.equal(h, torch.relu(lin(x)) * (k1 * s)) and h.dtype == dtype
